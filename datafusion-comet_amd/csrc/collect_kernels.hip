// collect_list / collect_set on gfx950: the hand-written kernels of exec_collect.cpp.  Their input is one value column of ANY type already sorted by the
// grouping keys (collect_list: a stable sort, arrival order inside a group survives) or by (grouping keys, value) (collect_set), and what the window
// operator's kernels make of the key planes: first[g] = the first row of group g and, for a set, fpeer[i] = 1 where row i starts a new run of equal
// (group, value) key bytes.  They never look at a value — only at validity bits, flags and row numbers — so one pair serves every element type:
//   collect_mask_kernel   Partial with a FILTER: the value's validity AND "the FILTER is TRUE", eight rows per lane — a rejected row becomes a NULL value
//                         (it still makes its group exist)
//   collect_keep_kernel   keep[i] = row i's value is not NULL and, for a set, row i is the first of its (group, value) run — as the u32 flags the engine's
//                         scan consumes; C = the scan's output (exclusive, n + 1 entries)
//   collect_index_kernel  idx[C[i]] = i for the kept rows: lane i reads flag and count i and writes slot C[i], both ascending with i, so a wave reads
//                         contiguous runs and writes one contiguous run (dropped rows only shorten it)
// The list's offsets are pct_offsets_kernel's (offs[g] = C[first[g]]); its elements are one gather of the sorted value column by idx (ascending indices).
// Streaming passes: grid-stride, 256 threads, no atomics, no LDS; every array is read once and written once.
#include <hip/hip_runtime.h>

#include "device/comet_device.hpp"

using namespace comet;

namespace {

int grid_for(i64 n) {
  i64 g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

// out[b] = valid[b] & fvalid[b] & fdata[b] over the nbytes bytes of the bitmaps (valid / fvalid: nullptr = all ones); bits past the last row mean nothing
__global__ __launch_bounds__(256) void collect_mask_kernel(const u8* __restrict__ valid, const u8* __restrict__ fvalid, const u8* __restrict__ fdata, i64 nbytes,
                                                           u8* __restrict__ out) {
  for (i64 b = (i64)blockIdx.x * 256 + threadIdx.x; b < nbytes; b += (i64)gridDim.x * 256) {
    u8 m = fdata[b];
    if (valid) m &= valid[b];
    if (fvalid) m &= fvalid[b];
    out[b] = m;
  }
}

// valid: the value's validity bitmap (nullptr = no NULLs); fpeer: nullptr for a list
__global__ __launch_bounds__(256) void collect_keep_kernel(const u8* __restrict__ valid, const u32* __restrict__ fpeer, i64 n, u32* __restrict__ keep) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
    u32 k = valid ? (u32)((valid[i >> 3] >> (i & 7)) & 1) : 1u;
    if (fpeer) k &= fpeer[i];
    keep[i] = k;
  }
}

// keep[i] ∈ {0, 1}; C[i] = kept rows before row i, so the kept rows' slots are 0 … C[n] − 1, each written once
__global__ __launch_bounds__(256) void collect_index_kernel(const u32* __restrict__ keep, const i32* __restrict__ C, i64 n, u32* __restrict__ idx) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256)
    if (keep[i]) idx[C[i]] = (u32)i;
}

}  // namespace

extern "C" {

int comet_launch_collect_mask(const uint8_t* valid, const uint8_t* fvalid, const uint8_t* fdata, int64_t n, uint8_t* out, void* stream) {
  const i64 nbytes = ((i64)n + 7) / 8;
  if (nbytes > 0) hipLaunchKernelGGL(collect_mask_kernel, grid_for(nbytes), 256, 0, (hipStream_t)stream, valid, fvalid, fdata, nbytes, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_collect_keep(const uint8_t* valid, const uint32_t* fpeer, int64_t n, uint32_t* keep, void* stream) {
  if (n > 0) hipLaunchKernelGGL(collect_keep_kernel, grid_for(n), 256, 0, (hipStream_t)stream, valid, fpeer, (i64)n, keep);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_collect_index(const uint32_t* keep, const int32_t* C, int64_t n, uint32_t* idx, void* stream) {
  if (n > 0) hipLaunchKernelGGL(collect_index_kernel, grid_for(n), 256, 0, (hipStream_t)stream, keep, C, (i64)n, idx);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
