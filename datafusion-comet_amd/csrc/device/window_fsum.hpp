// Float SUM / AVG over window frames: the per-row math of window_kernels.hip "Float sums over frames", on top of the exact Float64 sums of
// comet_device.hpp (include that first).  A frame's sum is the difference of two inclusive prefix sums; prefix sums of doubles cannot be
// differenced exactly (1e16, 1.0, −1e16 already loses the 1.0), prefix sums of FIXED-POINT integers can: every value becomes
// trunc(x / 2^s) in 192 bits (acc_feed_fix192), the prefix sums wrap modulo 2^192, and S[end − 1] − S[start − 1] is the frame's exact
// integer sum, rounded once by fix192_to_f64 — the same bits for every tiling, whatever earlier frames held.
//   Headroom: row positions are int32, so a column has n < 2^31 rows, and the scale rule (fix_scale.hpp) keeps every |x / 2^s| below
//   2^kFixW = 2^158: a frame's sum stays below 2^(158 + 31) < 2^191, inside the signed 192-bit range — so the wrapping difference is it.
// A column whose values span more than one such window (the rule would truncate) is NOT truncated here: its bits are cut into several
// windows kFixW bits apart, each with its own 192-bit prefix sums (wf_fix_slice), and a frame's differences are put together into one
// wide integer that is rounded once (wf_frame_wide) — exact for every double, at 24 bytes per row and window.
// ±inf, NaN and NULL rows add zero; what a frame holds of them comes from a second prefix sum over a packed class word.
// tests/emu/window_fsum_emu.cpp compiles this file for the host.
#pragma once

namespace comet {

struct U192 {   // three little-endian limbs, wrapping
  u64 w[3];
  CDEV U192& operator+=(const U192& b) { acc_add192(w, b.w); return *this; }
};
CDEV U192 u192_sub(const U192& a, const U192& b) {   // a − b modulo 2^192: a + ~b + 1
  U192 r;
  u128 c = (u128)a.w[0] + (u64)~b.w[0] + 1;
  r.w[0] = (u64)c;
  c = (c >> 64) + a.w[1] + (u64)~b.w[1];
  r.w[1] = (u64)c;
  r.w[2] = (u64)(c >> 64) + a.w[2] + ~b.w[2];
  return r;
}

CDEV bool wf_valid(const u8* valid_bits, i64 i) { return !valid_bits || ((valid_bits[i >> 3] >> (i & 7)) & 1); }
// row i of a Float64 (width 8) or Float32 (width 4: widened exactly) column
CDEV double wf_value(const void* src, int width, i64 i) { return width == 4 ? (double)((const float*)src)[i] : ((const double*)src)[i]; }
// a row's addend: trunc(x / 2^s); zero for a NULL, ±inf or NaN row
CDEV U192 wf_fix(bool valid, double x, int s) {
  U192 r = {{0, 0, 0}};
  if (valid) acc_feed_fix192(r.w, x, s);
  return r;
}
// the same for one of several windows: the bits of |x| of weight 2^s … 2^(s + kFixW − 1), with x's sign.  Windows kFixW apart partition
// every bit of x (53 bits: at most two adjacent windows hold some), so the slices of a value add up to it exactly.
CDEV U192 wf_fix_slice(bool valid, double x, int s) {
  U192 r = {{0, 0, 0}};
  u64 m; int q;
  if (!valid || !f64_parts(x, m, q)) return r;
  const int sh = q - s;
  if (sh >= kFixW || sh <= -53) return r;
  if (sh < 0) {
    r.w[0] = m >> -sh;
  } else {
    const int ws = sh >> 6, bs = sh & 63;
    r.w[ws] = m << bs;                                   // sh < 158: ws ≤ 2
    if (bs && ws + 1 < 3) r.w[ws + 1] = m >> (64 - bs);
  }
  r.w[2] &= (1ull << (kFixW - 128)) - 1;                 // bits from 2^(s + kFixW) on belong to the next window
  if (x < 0) {
    r.w[0] = ~r.w[0]; r.w[1] = ~r.w[1]; r.w[2] = ~r.w[2];
    if (++r.w[0] == 0) { if (++r.w[1] == 0) ++r.w[2]; }
  }
  return r;
}
// a row's class word: four 32-bit counters — non-NULL rows, +inf, −inf, NaN — in one 128-bit integer.  Their prefix sums count at most
// n < 2^31 rows each, so no field carries into the next and the fields of a difference are the frame's counts.
CDEV u128 wf_class_word(bool valid, double x) {
  if (!valid) return 0;
  const u64 c = f64_class(x);
  return (u128)1 | ((u128)(c & 1) << 32) | ((u128)((c >> 1) & 1) << 64) | ((u128)((c >> 2) & 1) << 96);
}
CDEV i64 wf_count(u128 k) { return (i64)(u32)k; }
CDEV u64 wf_class(u128 k) { return ((u32)(k >> 32) ? 1ull : 0ull) | ((u32)(k >> 64) ? 2ull : 0ull) | ((u32)(k >> 96) ? 4ull : 0ull); }   // f64_class bits

enum { WF_SUM = 0, WF_AVG = 1 };
// rows [start, end) of the prefix arrays S (fixed point) and K (class words): SUM is NULL when the frame holds no non-NULL row, else the
// exact sum rounded once (with the IEEE outcome of its inf / NaN rows); AVG divides that by the count in one IEEE division, like the
// grouped aggregate's Final
CDEV bool wf_frame(int fn, const U192* S, const u128* K, i64 start, i64 end, int s, double& out) {
  out = 0.0;
  if (end <= start) return false;
  const u128 k = K[end - 1] - (start ? K[start - 1] : (u128)0);
  const i64 cnt = wf_count(k);
  if (cnt == 0) return false;
  const U192 zero = {{0, 0, 0}};
  const U192 d = u192_sub(S[end - 1], start ? S[start - 1] : zero);
  const double sum = fix192_to_f64(d.w, s, wf_class(k));
  out = fn == WF_AVG ? sum / (double)cnt : sum;
  return true;
}

// ---- several windows ------------------------------------------------------------------------------------------------------------------
constexpr int kWfMaxWindows = 14;   // doubles span 2^-1074 … 2^1024: 2098 bits ≤ 14 · 158
constexpr int kWfBigLimbs = 38;     // 14 · 158 value bits + 31 bits of rows + sign, rounded up, and one spare limb
// big (nl limbs, two's complement) += sext(p) · 2^bit
CDEV void wf_big_add(u64* big, int nl, const U192& p, int bit) {
  const int ws = bit >> 6, bs = bit & 63;
  const u64 ext = (p.w[2] >> 63) ? ~0ull : 0ull;
  u64 carry = 0;
  for (int k = ws; k < nl; k++) {
    const int i = k - ws;
    const u64 cur = i < 3 ? p.w[i] : ext;
    const u64 below = i == 0 ? 0ull : (i - 1 < 3 ? p.w[i - 1] : ext);
    const u64 v = bs ? (cur << bs) | (below >> (64 - bs)) : cur;
    const u128 t = (u128)big[k] + v + carry;
    big[k] = (u64)t;
    carry = (u64)(t >> 64);
  }
}
// the integer big (nl limbs) · 2^s → nearest double, ties to even: fix192_to_f64 for any width
CDEV double wf_big_to_f64(u64* w, int nl, int s, u64 cls) {
  if (cls) { const u64 z[3] = {0, 0, 0}; return fix192_to_f64(z, s, cls); }
  const bool neg = (w[nl - 1] >> 63) != 0;
  if (neg) {
    u64 carry = 1;
    for (int k = 0; k < nl; k++) { w[k] = ~w[k] + carry; carry = (carry && w[k] == 0) ? 1 : 0; }
  }
  int top = nl - 1;
  while (top > 0 && w[top] == 0) top--;
  if (w[top] == 0) return 0.0;
  const int L = 64 * top + 64 - __builtin_clzll(w[top]);
  int e_lsb = s + L - 53;
  if (e_lsb < -1074) e_lsb = -1074;
  const int shift = e_lsb - s;
  u64 mant;
  if (shift <= 0) {
    mant = w[0];
    e_lsb = s;
  } else {
    const int ws = shift >> 6, bs = shift & 63;
    mant = w[ws] >> bs;
    if (bs && ws + 1 < nl) mant |= w[ws + 1] << (64 - bs);
    const int gb = shift - 1;
    const bool guard = (w[gb >> 6] >> (gb & 63)) & 1;
    bool sticky = false;
    for (int k = 0; k < (gb >> 6); k++) sticky |= w[k] != 0;
    sticky |= (w[gb >> 6] & ((1ull << (gb & 63)) - 1)) != 0;
    if (guard && (sticky || (mant & 1))) mant += 1;
  }
  const double r = ldexp((double)mant, e_lsb);
  return neg ? -r : r;
}
// wf_frame over `windows` prefix arrays n rows apart, window j at scale s + kFixW · j
CDEV bool wf_frame_wide(int fn, const U192* S, i64 n, int windows, const u128* K, i64 start, i64 end, int s, double& out) {
  out = 0.0;
  if (end <= start) return false;
  const u128 k = K[end - 1] - (start ? K[start - 1] : (u128)0);
  const i64 cnt = wf_count(k);
  if (cnt == 0) return false;
  u64 big[kWfBigLimbs];
  const int nl = (windows * kFixW + 32) / 64 + 2;
  for (int i = 0; i < nl; i++) big[i] = 0;
  const U192 zero = {{0, 0, 0}};
  for (int j = 0; j < windows; j++) {
    const U192* Sj = S + (size_t)j * (size_t)n;
    wf_big_add(big, nl, u192_sub(Sj[end - 1], start ? Sj[start - 1] : zero), kFixW * j);
  }
  const double sum = wf_big_to_f64(big, nl, s, wf_class(k));
  out = fn == WF_AVG ? sum / (double)cnt : sum;
  return true;
}

}  // namespace comet
