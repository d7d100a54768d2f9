// Derived columns of kind 7 (codegen.hpp DerivedCol) on gfx950: array_remove, array_compact, slice, reverse of an array and array_join over one list column
// (device/list_pick.hpp holds the per-element code; exec.cpp extend_derived_list_pick drives these and array_distinct's tail or one take_column afterwards).
// Every kernel has one lane per ELEMENT row e of [0, hi) — the element rows the column's offsets span (they start at 0: the executor refuses a sliced column).
// Where a lane needs its list it finds it with lf_list_of, a binary search of the offsets whose path neighbouring lanes share; everything after that is O(1),
// so there is no length tier: a list of 5 000 elements takes the path of one of 3.
//   list_pick_kernel        remove / compact / slice: out[e] = 1 when element e stays, else 0.  compact reads one validity bit and needs no list.
//   list_reverse_kernel     out[first + (end - 1 - e)] = e: a permutation inside the list, as array_sort's answer is; every slot is written once.
//   list_join_flag_kernel   array_join: out[e] = 1 when element e is a piece of its row's string (non-NULL, or a replacement is given)
//   list_join_len_kernel    … the bytes the piece brings: its own or the replacement's, and the delimiter's unless it is its list's first piece — which it is
//                           when the flags' exclusive scan F has the same value at e as at the list's first element
//   list_join_write_kernel  … and the bytes themselves at P[e], the lengths' exclusive scan.  The one place where lanes diverge by string length: the byte
//                           loops run as long as the wave's longest piece (accepted for short elements).
// Loads of flags, offsets' scans and validity are coalesced (lane e reads entry e); the element bytes are read where the offsets point.
// Grid-stride, 256 threads, no LDS, no cross-lane operation.  Every lane writes only its own entry — e, its slot inside its own list, or its piece's bytes.
#include <hip/hip_runtime.h>

#include "device/comet_device.hpp"
#define LISTFN __host__ __device__ inline
#include "device/list_pick.hpp"

using namespace comet;

namespace {

int grid_for(i64 n) {
  i64 g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

__global__ __launch_bounds__(256) void list_pick_kernel(LfCol col, const i32* __restrict__ offs, i64 rows, i64 hi, int op, LpKey key, i64 start, i64 length, u32* __restrict__ out) {
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < hi; e += (i64)gridDim.x * 256) {
    if (op == LP_COMPACT) {
      out[e] = lf_is_null(col, e) ? 0u : 1u;
      continue;
    }
    const i64 row = lf_list_of(offs, rows, e);
    out[e] = lp_keep(op, col, row, offs[row], offs[row + 1], e, key, start, length) ? 1u : 0u;
  }
}

__global__ __launch_bounds__(256) void list_reverse_kernel(const i32* __restrict__ offs, i64 rows, i64 hi, u32* __restrict__ out) {
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < hi; e += (i64)gridDim.x * 256) {
    const i64 row = lf_list_of(offs, rows, e);
    const i64 slot = lp_reverse_slot(offs[row], offs[row + 1], e);
    if (slot >= 0 && slot < hi) out[slot] = (u32)e;      // (always, for offsets that ascend)
  }
}

__global__ __launch_bounds__(256) void list_join_flag_kernel(LfCol col, i64 hi, int has_rep, u32* __restrict__ out) {
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < hi; e += (i64)gridDim.x * 256) out[e] = lp_is_piece(col, e, has_rep != 0) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void list_join_len_kernel(LfCol col, const i32* __restrict__ offs, i64 rows, i64 hi, const i32* __restrict__ F, int dn, int rn, int has_rep,
                                                            u32* __restrict__ out) {
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < hi; e += (i64)gridDim.x * 256) {
    if (!lp_is_piece(col, e, has_rep != 0)) {
      out[e] = 0u;
      continue;
    }
    const i64 row = lf_list_of(offs, rows, e);
    out[e] = lp_piece_len(col, e, F[e] == F[offs[row]], dn, rn);
  }
}

__global__ __launch_bounds__(256) void list_join_write_kernel(LfCol col, const i32* __restrict__ offs, i64 rows, i64 hi, const i32* __restrict__ F, const i32* __restrict__ P,
                                                              const u8* __restrict__ d, int dn, const u8* __restrict__ r, int rn, int has_rep, u8* __restrict__ dst) {
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < hi; e += (i64)gridDim.x * 256) {
    if (!lp_is_piece(col, e, has_rep != 0)) continue;
    const i64 row = lf_list_of(offs, rows, e);
    lp_piece_write(col, e, F[e] == F[offs[row]], d, dn, r, rn, dst + (i64)P[e]);
  }
}

LfCol col_of(int kind, const void* data, const uint8_t* aux, const uint8_t* valid, i64 offset) {
  LfCol c;
  c.data = data;
  c.aux = aux;
  c.valid = valid;
  c.offset = offset;
  c.kind = kind;
  return c;
}

}  // namespace

extern "C" {

// offs: the list column's offsets, rows + 1 of them, offs[0] = 0; hi = offs[rows]; out: hi entries.  op LP_REMOVE: the key is the literal (key_hi, key_lo) — for
// Utf8 with its key_len bytes at key_bytes on the device — or, with key_col_data set, row `row` of that column of the elements' kind (validity bits or nullptr,
// Arrow offset key_col_offset).  op LP_SLICE: start != 0 and length >= 0.  kind is read by LP_REMOVE alone
int comet_launch_list_pick(int op, int kind, const void* data, const uint8_t* aux, const uint8_t* valid, const int32_t* offs, int64_t rows, int64_t hi, uint64_t key_hi,
                           uint64_t key_lo, const uint8_t* key_bytes, int32_t key_len, const void* key_col_data, const uint8_t* key_col_valid, int64_t key_col_offset,
                           int64_t start, int64_t length, uint32_t* out, void* stream) {
  if (hi <= 0 || rows <= 0) return 0;
  if (op != LP_REMOVE && op != LP_COMPACT && op != LP_SLICE) return -1;
  LpKey k;
  k.key.hi = key_hi;
  k.key.lo = key_lo;
  k.bytes = key_bytes;
  k.len = key_len;
  k.col = col_of(kind, key_col_data, nullptr, key_col_valid, key_col_offset);
  k.use_col = key_col_data ? 1 : 0;
  hipLaunchKernelGGL(list_pick_kernel, grid_for(hi), 256, 0, (hipStream_t)stream, col_of(kind, data, aux, valid, 0), offs, (i64)rows, (i64)hi, op, k, (i64)start, (i64)length, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_list_reverse(const int32_t* offs, int64_t rows, int64_t hi, uint32_t* out, void* stream) {
  if (hi <= 0 || rows <= 0) return 0;
  hipLaunchKernelGGL(list_reverse_kernel, grid_for(hi), 256, 0, (hipStream_t)stream, offs, (i64)rows, (i64)hi, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// array_join's three kernels over a Utf8 element column (data: its int32 offsets, aux: its bytes).  F and P: the exclusive scans of the flags and of the lengths, hi + 1 entries
int comet_launch_list_join_flags(const void* data, const uint8_t* aux, const uint8_t* valid, int64_t hi, int has_rep, uint32_t* out, void* stream) {
  if (hi <= 0) return 0;
  hipLaunchKernelGGL(list_join_flag_kernel, grid_for(hi), 256, 0, (hipStream_t)stream, col_of(LF_STR, data, aux, valid, 0), (i64)hi, has_rep, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_list_join_len(const void* data, const uint8_t* aux, const uint8_t* valid, const int32_t* offs, int64_t rows, int64_t hi, const int32_t* F, int32_t dn, int32_t rn,
                               int has_rep, uint32_t* out, void* stream) {
  if (hi <= 0 || rows <= 0) return 0;
  hipLaunchKernelGGL(list_join_len_kernel, grid_for(hi), 256, 0, (hipStream_t)stream, col_of(LF_STR, data, aux, valid, 0), offs, (i64)rows, (i64)hi, F, dn, rn, has_rep, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_list_join_write(const void* data, const uint8_t* aux, const uint8_t* valid, const int32_t* offs, int64_t rows, int64_t hi, const int32_t* F, const int32_t* P,
                                 const uint8_t* d, int32_t dn, const uint8_t* r, int32_t rn, int has_rep, uint8_t* dst, void* stream) {
  if (hi <= 0 || rows <= 0) return 0;
  hipLaunchKernelGGL(list_join_write_kernel, grid_for(hi), 256, 0, (hipStream_t)stream, col_of(LF_STR, data, aux, valid, 0), offs, (i64)rows, (i64)hi, F, P, d, dn, r, rn, has_rep,
                     dst);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
