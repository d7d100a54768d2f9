// Spark's exact percentile (native/spark-expr/src/agg_funcs/percentile.rs) on gfx950: the hand-written kernels of exec_percentile.cpp.  Their input is one
// value column already sorted by (grouping keys, value) with the engine's radix sort, NULL values last inside each group, and two arrays the window
// operator's kernels (window_flags_kernel, window_first_kernel, the u32 scan) make of the key planes: first[g] = the first row of group g (first[G] = n) and, where the column has NULLs, C[i] = how many non-NULL
// values stand before row i (an exclusive scan, C[n] = all of them).
//   pct_flatten_kernel   PartialMerge / Final: the incoming List<Float64> states as (input row, value) rows, one per element, and one NULL row for an empty or
//                        NULL list — per OUTPUT row, so a single state that holds every value of a partition (an ungrouped Partial's) is spread over the whole
//                        grid; consecutive lanes read consecutive elements.  The collect aggregates (exec_collect.cpp) flatten their List<any type> states with
//                        it too: they ask for the element's index instead of its value and take the element column by it
//   pct_offsets_kernel   the List<Float64> state's offsets: offs[g] = kept values before group g (G + 1 entries)
//   pct_compact_kernel   the state's values: the kept values in sorted order, NULLs squeezed out — lane i reads row i and writes slot C[i], both ascending
//                        with i, so a wave reads 512 contiguous bytes and writes one contiguous run (a group's NULL tail only shortens the run)
//   pct_pick_kernel      Final: one thread per group reads its lo / hi and runs device/percentile.hpp's formula for each percentage; ok[g] = the group kept a value
// Streaming passes only: every array is read once and written once, by consecutive lanes at consecutive addresses; the pick's two value loads per
// (group, percentage) are the only gathers, and they fall into the group's own rows.
#include <hip/hip_runtime.h>

#include "device/comet_device.hpp"
#include "device/percentile.hpp"

using namespace comet;

namespace {

constexpr int kPctMaxPerLaunch = 16;
struct PctList {
  int n;
  double p[kPctMaxPerLaunch];
};

int grid_for(i64 n) {
  i64 g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

// out_offs: the exclusive scan (n + 1 entries) of each state row's output rows — its elements, or one for an empty / NULL list — so it ascends strictly and
// output row i belongs to the last input row r with out_offs[r] <= i.  ok[i]: there is an element and it is not NULL.  vals (with elems) and elem_idx are
// optional: the element's value as a double, and its index in the element column — 0 where there is none: the gather that follows reads that slot and ok[i]
// discards what it read (the caller gathers only from an element column that holds at least one element)
__global__ __launch_bounds__(256) void pct_flatten_kernel(const i32* __restrict__ offs, const u8* __restrict__ list_valid, const double* __restrict__ elems,
                                                          const u8* __restrict__ elem_valid, i64 n, const i32* __restrict__ out_offs, i64 total, u32* __restrict__ row_idx,
                                                          double* __restrict__ vals, u32* __restrict__ elem_idx, u8* __restrict__ ok) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total; i += (i64)gridDim.x * 256) {
    i64 lo = 0, hi = n - 1;      // out_offs[lo] <= i < out_offs[hi + 1]
    while (lo < hi) {
      const i64 mid = (lo + hi + 1) >> 1;
      if ((i64)out_offs[mid] <= i) lo = mid;
      else hi = mid - 1;
    }
    const i64 r = lo, j = i - (i64)out_offs[r];
    const bool lv = !list_valid || ((list_valid[r >> 3] >> (r & 7)) & 1);
    const i64 src = offs[r], len = lv ? (i64)offs[r + 1] - src : 0;
    const i64 e = src + j;
    bool keep = j < len;
    if (keep && elem_valid) keep = (elem_valid[e >> 3] >> (e & 7)) & 1;
    row_idx[i] = (u32)r;
    if (vals) vals[i] = keep ? elems[e] : 0.0;
    if (elem_idx) elem_idx[i] = j < len ? (u32)e : 0u;
    ok[i] = keep ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void pct_offsets_kernel(const u32* __restrict__ first, const i32* __restrict__ C, i64 G, i32* __restrict__ offs) {
  for (i64 g = (i64)blockIdx.x * 256 + threadIdx.x; g <= G; g += (i64)gridDim.x * 256) {
    const u32 r = first[g];
    offs[g] = C ? C[r] : (i32)r;
  }
}

__global__ __launch_bounds__(256) void pct_compact_kernel(const double* __restrict__ vals, const u8* __restrict__ valid_bits, const i32* __restrict__ C, i64 n,
                                                          double* __restrict__ out) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
    const bool keep = (valid_bits[i >> 3] >> (i & 7)) & 1;
    if (keep) out[C[i]] = vals[i];
  }
}

// out[q · G + g], q < list.n; ok[g].  A group's kept values are its first offs[g + 1] − offs[g] rows (NULLs sort last)
__global__ __launch_bounds__(256) void pct_pick_kernel(const double* __restrict__ vals, const u32* __restrict__ first, const i32* __restrict__ offs, i64 G, PctList list,
                                                       double* __restrict__ out, u8* __restrict__ ok) {
  for (i64 g = (i64)blockIdx.x * 256 + threadIdx.x; g < G; g += (i64)gridDim.x * 256) {
    const i64 cnt = (i64)offs[g + 1] - (i64)offs[g];
    const double* const v = vals + first[g];
    ok[g] = cnt > 0 ? 1 : 0;
    for (int q = 0; q < list.n; q++) out[(size_t)q * (size_t)G + (size_t)g] = cnt > 0 ? pct_pick(v, cnt, list.p[q]) : 0.0;
  }
}

}  // namespace

extern "C" {

int comet_launch_pct_flatten(const int32_t* offs, const uint8_t* list_valid, const double* elems, const uint8_t* elem_valid, int64_t n, const int32_t* out_offs, int64_t total,
                             uint32_t* row_idx, double* vals, uint32_t* elem_idx, uint8_t* ok, void* stream) {
  if (n > 0 && total > 0)
    hipLaunchKernelGGL(pct_flatten_kernel, grid_for(total), 256, 0, (hipStream_t)stream, offs, list_valid, elems, elem_valid, (i64)n, out_offs, (i64)total, row_idx, elems ? vals : nullptr,
                       elem_idx, ok);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_pct_offsets(const uint32_t* first, const int32_t* C, int64_t G, int32_t* offs, void* stream) {
  hipLaunchKernelGGL(pct_offsets_kernel, grid_for(G + 1), 256, 0, (hipStream_t)stream, first, C, (i64)G, offs);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int comet_launch_pct_compact(const double* vals, const uint8_t* valid_bits, const int32_t* C, int64_t n, double* out, void* stream) {
  if (n > 0) hipLaunchKernelGGL(pct_compact_kernel, grid_for(n), 256, 0, (hipStream_t)stream, vals, valid_bits, C, (i64)n, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// nq percentages (any number: kPctMaxPerLaunch per launch) over G groups → out[q · G + g], ok[g]
int comet_launch_pct_pick(const double* vals, const uint32_t* first, const int32_t* offs, int64_t G, const double* pcts, int nq, double* out, uint8_t* ok, void* stream) {
  for (int q0 = 0; q0 < nq && G > 0; q0 += kPctMaxPerLaunch) {
    PctList list;
    list.n = nq - q0 < kPctMaxPerLaunch ? nq - q0 : kPctMaxPerLaunch;
    for (int q = 0; q < kPctMaxPerLaunch; q++) list.p[q] = q < list.n ? pcts[q0 + q] : 0.0;
    hipLaunchKernelGGL(pct_pick_kernel, grid_for(G), 256, 0, (hipStream_t)stream, vals, first, offs, (i64)G, list, out + (size_t)q0 * (size_t)G, ok);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
