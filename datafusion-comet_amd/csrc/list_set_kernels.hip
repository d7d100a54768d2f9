// Derived columns of kind 6 (codegen.hpp DerivedCol) on gfx950: array_union, array_intersect, array_except and arrays_overlap over two list columns
// (device/list_set.hpp holds the per-element code; exec.cpp extend_derived_list_set drives these between the kind-4 machinery's distinct and sort).
//   list_member_kernel        one lane per probe ELEMENT row e of [0, hi_a).  The lane finds its list (lf_list_of, a binary search of a's offsets that neighbouring
//                             lanes share), then binary-searches [offs_b[row], offs_b[row + 1]) of b SORTED ascending with NULLs first and writes
//                             out[e] = (found == want) ? 1 : 0 — O(log) per lane in both list lengths, so there is no length cap and no second tier.  Lanes of one
//                             list search the same range: the upper levels of the search read the same addresses.
//   list_overlap_row_kernel   one lane per ROW: walks a's list once over the hit flags and validity bits, reads b's first (sorted) element, and writes the
//                             three-valued code; list_overlap_bits_kernel packs eight codes into a value byte and a validity byte.
//   list_concat_len_kernel, list_concat_index_kernel   union: the row lengths of a ++ b (0 where a side is NULL), and — after their scan — every output
//                             element's source row in the two element columns laid end to end.
//   list_concat_bits_kernel, list_rebase_offsets_kernel   laying the element columns end to end where a D2D copy does not do: bit-packed data and validity
//                             at a join that is no multiple of 8 (and a side without a bitmap: ones), Utf8 offsets moved up by a's byte count.
//   list_and_bits_kernel      the result's row validity: the AND of the two lists' bitmaps
// Grid-stride, 256 threads, no LDS, no cross-lane operation.  Every lane writes only its own output entry (element e, row r or byte i), all below the counts the
// launchers pass.
#include <hip/hip_runtime.h>

#include "device/comet_device.hpp"
#define LISTFN __host__ __device__ inline
#include "device/list_set.hpp"

using namespace comet;

namespace {

int grid_for(i64 n) {
  i64 g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

__global__ __launch_bounds__(256) void list_member_kernel(LfCol a, LfCol b, const i32* __restrict__ offs_a, const i32* __restrict__ offs_b, const u8* __restrict__ a_rows,
                                                          const u8* __restrict__ b_rows, i64 rows, i64 hi_a, int want, int values_only, u32* __restrict__ out) {
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < hi_a; e += (i64)gridDim.x * 256) {
    const i64 row = lf_list_of(offs_a, rows, e);
    out[e] = lf_member(a, e, b, offs_b[row], offs_b[row + 1], a_rows, b_rows, row, want != 0, values_only != 0);
  }
}

__global__ __launch_bounds__(256) void list_overlap_row_kernel(const u32* __restrict__ hits, LfCol a, LfCol b, const i32* __restrict__ offs_a, const i32* __restrict__ offs_b,
                                                               const u8* __restrict__ a_rows, const u8* __restrict__ b_rows, i64 rows, u8* __restrict__ code) {
  for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r < rows; r += (i64)gridDim.x * 256)
    code[r] = (u8)lf_overlap_row(hits, a, offs_a[r], offs_a[r + 1], b, offs_b[r], offs_b[r + 1], ls_bit(a_rows, r) && ls_bit(b_rows, r));
}

// byte i of the Boolean column and of its validity bitmap: rows 8 i … 8 i + 7 (bits beyond `rows` are 0)
__global__ __launch_bounds__(256) void list_overlap_bits_kernel(const u8* __restrict__ code, i64 rows, u8* __restrict__ value, u8* __restrict__ valid) {
  const i64 nb = (rows + 7) / 8;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nb; i += (i64)gridDim.x * 256) {
    u32 v = 0, ok = 0;
    for (int k = 0; k < 8; k++) {
      const i64 r = i * 8 + k;
      if (r >= rows) break;
      const u8 c = code[r];
      v |= (c == LS_TRUE ? 1u : 0u) << k;
      ok |= (c != LS_NULL ? 1u : 0u) << k;
    }
    value[i] = (u8)v;
    valid[i] = (u8)ok;
  }
}

__global__ __launch_bounds__(256) void list_concat_len_kernel(const i32* __restrict__ offs_a, const i32* __restrict__ offs_b, const u8* __restrict__ a_rows,
                                                              const u8* __restrict__ b_rows, i64 rows, u32* __restrict__ len) {
  for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r < rows; r += (i64)gridDim.x * 256) len[r] = lf_concat_len(offs_a, offs_b, a_rows, b_rows, r);
}

__global__ __launch_bounds__(256) void list_concat_index_kernel(const i32* __restrict__ offs_a, const i32* __restrict__ offs_b, const i32* __restrict__ offs_out, i64 rows,
                                                                i64 hi_a, i64 total, u32* __restrict__ idx) {
  for (i64 k = (i64)blockIdx.x * 256 + threadIdx.x; k < total; k += (i64)gridDim.x * 256) idx[k] = (u32)lf_concat_src(offs_a, offs_b, offs_out, rows, hi_a, k);
}

// byte i of a's na bits followed by b's nb bits; an absent side reads as ones
__global__ __launch_bounds__(256) void list_concat_bits_kernel(const u8* __restrict__ a, i64 na, const u8* __restrict__ b, i64 nb, u8* __restrict__ out) {
  const i64 n = na + nb, bytes = (n + 7) / 8;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < bytes; i += (i64)gridDim.x * 256) {
    u32 v = 0;
    for (int k = 0; k < 8; k++) {
      const i64 j = i * 8 + k;
      if (j >= n) break;
      v |= (ls_concat_bit(a, na, b, j) ? 1u : 0u) << k;
    }
    out[i] = (u8)v;
  }
}

// out[i] = in[i] + by for the n + 1 offsets of a Utf8 column that follows `by` bytes of another
__global__ __launch_bounds__(256) void list_rebase_offsets_kernel(const i32* __restrict__ in, i64 n, i32 by, i32* __restrict__ out) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i <= n; i += (i64)gridDim.x * 256) out[i] = in[i] + by;
}

__global__ __launch_bounds__(256) void list_and_bits_kernel(const u8* __restrict__ a, const u8* __restrict__ b, i64 bytes, u8* __restrict__ out) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < bytes; i += (i64)gridDim.x * 256) out[i] = (u8)((a ? a[i] : 0xffu) & (b ? b[i] : 0xffu));
}

LfCol col_of(int kind, const void* data, const uint8_t* aux, const uint8_t* valid) {
  LfCol c;
  c.data = data;
  c.aux = aux;
  c.valid = valid;
  c.offset = 0;
  c.kind = kind;
  return c;
}

}  // namespace

extern "C" {

// a: the probe elements [0, hi_a) under offs_a (rows + 1 offsets from 0); b: the other side's elements SORTED per list under offs_b; a_rows / b_rows: the lists'
// validity bits or nullptr; out: hi_a flags
int comet_launch_list_member(int kind, const void* a_data, const uint8_t* a_aux, const uint8_t* a_valid, const void* b_data, const uint8_t* b_aux, const uint8_t* b_valid,
                             const int32_t* offs_a, const int32_t* offs_b, const uint8_t* a_rows, const uint8_t* b_rows, int64_t rows, int64_t hi_a, int want,
                             int values_only, uint32_t* out, void* stream) {
  if (hi_a <= 0 || rows <= 0) return 0;
  hipLaunchKernelGGL(list_member_kernel, grid_for(hi_a), 256, 0, (hipStream_t)stream, col_of(kind, a_data, a_aux, a_valid), col_of(kind, b_data, b_aux, b_valid), offs_a, offs_b,
                     a_rows, b_rows, (i64)rows, (i64)hi_a, want, values_only, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// hits: the member flags of a's elements (values only); code: rows bytes of scratch; value / valid: (rows + 7) / 8 bytes each
int comet_launch_list_overlap(int kind, const uint32_t* hits, const void* a_data, const uint8_t* a_aux, const uint8_t* a_valid, const void* b_data, const uint8_t* b_aux,
                              const uint8_t* b_valid, const int32_t* offs_a, const int32_t* offs_b, const uint8_t* a_rows, const uint8_t* b_rows, int64_t rows, uint8_t* code,
                              uint8_t* value, uint8_t* valid, void* stream) {
  if (rows <= 0) return 0;
  hipLaunchKernelGGL(list_overlap_row_kernel, grid_for(rows), 256, 0, (hipStream_t)stream, hits, col_of(kind, a_data, a_aux, a_valid), col_of(kind, b_data, b_aux, b_valid), offs_a,
                     offs_b, a_rows, b_rows, (i64)rows, code);
  hipLaunchKernelGGL(list_overlap_bits_kernel, grid_for((rows + 7) / 8), 256, 0, (hipStream_t)stream, code, (i64)rows, value, valid);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_list_concat_len(const int32_t* offs_a, const int32_t* offs_b, const uint8_t* a_rows, const uint8_t* b_rows, int64_t rows, uint32_t* len, void* stream) {
  if (rows <= 0) return 0;
  hipLaunchKernelGGL(list_concat_len_kernel, grid_for(rows), 256, 0, (hipStream_t)stream, offs_a, offs_b, a_rows, b_rows, (i64)rows, len);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_list_concat_index(const int32_t* offs_a, const int32_t* offs_b, const int32_t* offs_out, int64_t rows, int64_t hi_a, int64_t total, uint32_t* idx, void* stream) {
  if (total <= 0 || rows <= 0) return 0;
  hipLaunchKernelGGL(list_concat_index_kernel, grid_for(total), 256, 0, (hipStream_t)stream, offs_a, offs_b, offs_out, (i64)rows, (i64)hi_a, (i64)total, idx);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_list_concat_bits(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb, uint8_t* out, void* stream) {
  if (na + nb <= 0) return 0;
  hipLaunchKernelGGL(list_concat_bits_kernel, grid_for((na + nb + 7) / 8), 256, 0, (hipStream_t)stream, a, (i64)na, b, (i64)nb, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_list_rebase_offsets(const int32_t* in, int64_t n, int32_t by, int32_t* out, void* stream) {
  if (n < 0) return 0;
  hipLaunchKernelGGL(list_rebase_offsets_kernel, grid_for(n + 1), 256, 0, (hipStream_t)stream, in, (i64)n, by, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_list_and_bits(const uint8_t* a, const uint8_t* b, int64_t bytes, uint8_t* out, void* stream) {
  if (bytes <= 0) return 0;
  hipLaunchKernelGGL(list_and_bits_kernel, grid_for(bytes), 256, 0, (hipStream_t)stream, a, b, (i64)bytes, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
