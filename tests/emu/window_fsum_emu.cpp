// TEST INFRASTRUCTURE: csrc/device/window_fsum.hpp — the per-row math of the Window operator's float SUM / AVG over frames — compiled for the
// CPU on top of the device header (through hip_host_shim.hpp).  The passes the gfx950 kernels make in parallel run here one row after the other:
// exponent range → the scale of fix_scale.hpp (or several windows where it would truncate) → 192-bit prefix sums and class-word prefix sums → per frame
// the difference, rounded once.
// tests/test_window_float_cpu.py compares the results with math.fsum.
#include "hip_host_shim.hpp"
#include <vector>
#include "comet_device.hpp"
#include "device/window_fsum.hpp"
#include "fix_scale.hpp"

// x: n doubles; valid_bits: Arrow validity bitmap or NULL; frames: nf (start, end) pairs, rows [start, end); fn: 0 = SUM, 1 = AVG.
// out / ok: one result per frame (ok = 0: NULL).  Returns the scale the shared rule gives for the column; *windows_out: how many fixed-point windows
// the column was cut into (more than one where the rule alone would truncate).
extern "C" __attribute__((visibility("default"))) int window_fsum_emu(const double* x, const uint8_t* valid_bits, int64_t n, const int64_t* frames, int64_t nf, int fn, double* out,
                                                                      uint8_t* ok, int* windows_out) {
  using namespace comet;
  u64 hi = 0, lo = 0;
  for (i64 i = 0; i < n; i++) {
    if (!wf_valid(valid_bits, i)) continue;
    const u64 h = f64_exp_hi(x[i]), l = f64_exp_lo(x[i]);
    hi = h > hi ? h : hi;
    lo = l > lo ? l : lo;
  }
  const int top = (int)hi - 1200, low = 1200 - (int)lo;
  const int rule = hi ? fix_scale_for_range(top, low, kFixW) : 0;
  int s = rule, windows = 1;
  if (hi && rule != low) {   // as exec_window.cpp: windows from the lowest bit up instead of truncating
    s = low;
    windows = (top - low + kFixW - 1) / kFixW;
  }
  *windows_out = windows;
  std::vector<U192> S((size_t)n * (size_t)windows);
  std::vector<u128> K((size_t)n);
  for (int j = 0; j < windows; j++) {
    U192 run = {{0, 0, 0}};
    for (i64 i = 0; i < n; i++) {
      const bool v = wf_valid(valid_bits, i);
      run += windows > 1 ? wf_fix_slice(v, wf_value(x, 8, i), s + kFixW * j) : wf_fix(v, wf_value(x, 8, i), s);
      S[(size_t)j * (size_t)n + (size_t)i] = run;
    }
  }
  u128 krun = 0;
  for (i64 i = 0; i < n; i++) {
    krun += wf_class_word(wf_valid(valid_bits, i), x[i]);
    K[(size_t)i] = krun;
  }
  for (i64 f = 0; f < nf; f++) {
    double v;
    const bool k = windows > 1 ? wf_frame_wide(fn, S.data(), n, windows, K.data(), frames[2 * f], frames[2 * f + 1], s, v)
                               : wf_frame(fn, S.data(), K.data(), frames[2 * f], frames[2 * f + 1], s, v);
    ok[f] = k ? 1 : 0;
    out[f] = v;
  }
  return rule;
}
