// Derived list columns of kind 4 (codegen.hpp DerivedCol) on gfx950: array_sort and array_distinct over a list column's elements, per list, by element row
// numbers (device/list_fn.hpp holds the order and the per-element code; exec.cpp extend_derived_list_fn drives these and takes the element column afterwards).
//   list_rank_kernel      one lane per ELEMENT row e of [0, hi) — the element rows the column's offsets span (they start at 0: the executor refuses a
//                         sliced column).  The lane finds its list (a binary search of the offsets, which neighbouring lanes share), then walks that list's elements: neighbouring lanes belong to the same list almost
//                         always and read the same addresses in the same order, so the walk is served by the cache and the key loads of a wave coalesce.
//                         sort: the number of elements that stand before e is its slot — out[first + rank] = e, a permutation of the list's own rows, so
//                         every lane writes inside [first, end) and each slot is written once.  distinct: out[e] = 1 when no earlier element of the list
//                         has e's NULL-ness and value, else 0.  A list longer than `cap` is left alone (sort: the identity, distinct: nothing kept) and its
//                         length goes to *too_long (one atomicMax, by the lane of the list's first element): the executor then runs the whole column through the
//                         sort route instead.
//   list_offsets_kernel   distinct: the new list's offsets, the keep flags' exclusive scan C read at the old offsets
//   list_row_kernel, list_scatter_keep_kernel   the sort route's two ends: every element row's list row as the radix sort's first key, and distinct's
//                         peer flags scattered from sorted order back to the elements' own rows
// Grid-stride, 256 threads, no LDS, no cross-lane operation.
#include <hip/hip_runtime.h>

#include "device/comet_device.hpp"
#define LISTFN __host__ __device__ inline
#include "device/list_fn.hpp"

using namespace comet;

namespace {

int grid_for(i64 n) {
  i64 g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

__global__ __launch_bounds__(256) void list_rank_kernel(LfCol col, const i32* __restrict__ offs, i64 rows, i64 hi, int op, int flags, i64 cap, u32* __restrict__ out,
                                                        u32* __restrict__ too_long) {
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < hi; e += (i64)gridDim.x * 256) {
    const i64 row = lf_list_of(offs, rows, e);
    const i64 first = offs[row], end = offs[row + 1];
    if (end - first > cap) {
      out[e] = op == LF_OP_SORT ? (u32)e : 0u;
      if (e == first) atomicMax(too_long, (u32)(end - first));
      continue;
    }
    if (op == LF_OP_SORT) out[first + lf_rank(col, first, end, e, flags)] = (u32)e;
    else out[e] = lf_keep(col, first, e) ? 1u : 0u;
  }
}

__global__ __launch_bounds__(256) void list_offsets_kernel(const i32* __restrict__ offs, const i32* __restrict__ C, i64 rows, i32* __restrict__ out) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i <= rows; i += (i64)gridDim.x * 256) out[i] = C[offs[i]];
}

// the sort route (exec.cpp list_fn_sort_route): the list row of every element row of [0, hi) as an Int32 column
__global__ __launch_bounds__(256) void list_row_kernel(const i32* __restrict__ offs, i64 rows, i64 hi, i32* __restrict__ out) {
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < hi; e += (i64)gridDim.x * 256) out[e] = (i32)lf_list_of(offs, rows, e);
}

// … and distinct's keep flags back at the elements' own rows: sorted row k is element row src[k] (a permutation of [0, hi)), which starts a run of equal
// (list, value) key bytes where fpeer[k] is set; the sort is stable, so a run's first row is the value's first occurrence
__global__ __launch_bounds__(256) void list_scatter_keep_kernel(const u32* __restrict__ src, const u32* __restrict__ fpeer, i64 hi, u32* __restrict__ keep) {
  for (i64 k = (i64)blockIdx.x * 256 + threadIdx.x; k < hi; k += (i64)gridDim.x * 256) {
    const u32 e = src[k];
    if ((i64)e < hi) keep[e] = fpeer[k];
  }
}

}  // namespace

extern "C" {

int comet_launch_list_rows(const int32_t* offs, int64_t rows, int64_t hi, int32_t* out, void* stream) {
  if (hi <= 0 || rows <= 0) return 0;
  hipLaunchKernelGGL(list_row_kernel, grid_for(hi), 256, 0, (hipStream_t)stream, offs, (i64)rows, (i64)hi, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_list_scatter_keep(const uint32_t* src, const uint32_t* fpeer, int64_t hi, uint32_t* keep, void* stream) {
  if (hi <= 0) return 0;
  hipLaunchKernelGGL(list_scatter_keep_kernel, grid_for(hi), 256, 0, (hipStream_t)stream, src, fpeer, (i64)hi, keep);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// offs: the list column's offsets, rows + 1 of them, offs[0] = 0; hi = offs[rows]; out: hi entries
int comet_launch_list_rank(int kind, const void* data, const uint8_t* aux, const uint8_t* valid, const int32_t* offs, int64_t rows, int64_t hi, int op,
                           int flags, int64_t cap, uint32_t* out, uint32_t* too_long, void* stream) {
  if (hi <= 0 || rows <= 0) return 0;
  LfCol col;
  col.data = data;
  col.aux = aux;
  col.valid = valid;
  col.offset = 0;
  col.kind = kind;
  hipLaunchKernelGGL(list_rank_kernel, grid_for(hi), 256, 0, (hipStream_t)stream, col, offs, (i64)rows, (i64)hi, op, flags, (i64)cap, out, too_long);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_list_offsets(const int32_t* offs, const int32_t* C, int64_t rows, int32_t* out, void* stream) {
  if (rows < 0) return 0;
  hipLaunchKernelGGL(list_offsets_kernel, grid_for(rows + 1), 256, 0, (hipStream_t)stream, offs, C, (i64)rows, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
