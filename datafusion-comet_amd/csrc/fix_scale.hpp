// Exact Float64 sums (device/comet_device.hpp "Exact Float64 sums"): where the fixed-point window [2^s, 2^(s + w)) goes when the sum's
// addends are known to span 2^low (the lowest set bit of any addend) … 2^top (every |x| < 2^top) and nothing has been accumulated yet.
// The grouped aggregate (exec_pipeline.cpp adjust_fix_scales) and the Window operator's frame sums (exec_window.cpp) both ask here.
#pragma once

namespace comet {

constexpr int kFixScaleFloor = -1300;   // below every double's lowest bit (2^-1074)

// s = low when the whole range fits with 10 bits of slack (then every sum is exact); else as low as the top value allows, and the
// addends' bits below 2^s are truncated toward zero (error < rows · 2^s)
inline int fix_scale_for_range(int top, int low, int w) {
  const int s = (top - low <= w - 10) ? low : top + 2 - w;
  return s < kFixScaleFloor ? kFixScaleFloor : s;
}

}  // namespace comet
