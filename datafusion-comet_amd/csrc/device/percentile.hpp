// Spark's exact percentile (Percentile / median / percentile_cont; restated from native/spark-expr/src/agg_funcs/percentile.rs:280-319): the pick over a
// group's kept values once they are sorted.  Shared by percentile_kernels.hip and — compiled by g++ — by the host diagnostic of include/comet_amd.h.
//
//   n = 0 → NULL;  n = 1 → that value;  else position = (n − 1) · p as a double, lower = floor, higher = ceil, lo / hi the lower-th / higher-th smallest;
//   lower == higher, or lo equals hi → lo;  else (higher − position) · lo + (position − lower) · hi — two products and one sum, EACH ROUNDED.
//
// Fusing either product into the sum moves the last bit in about a quarter of random cases ([-45.5, 28.4] at p = 0.123456789: -0x1.230329214444ep+5, with a
// product left exact inside a fused multiply-add …4444fp+5), and both hipcc and g++ may contract: the device side spells the operations as __dmul_rn / __dadd_rn, the host side keeps each
// product in a volatile.
//
// Order: the reference compares with NaN greatest (any sign, any payload), NaN = NaN and −0.0 = 0.0.  The engine's Float64 sort key (comet_device.hpp
// f64_total_key) is IEEE totalOrder: it puts NaNs with the sign bit set BELOW −inf and separates −0.0 from 0.0.  The percentile's sorts therefore order their
// value column by NormalizeNaNAndZero(value): every NaN becomes the canonical positive one, above +inf, and both zeros become 0.0 — as the key only; the
// values themselves stay as they came.  Which of two equal zeros lands on a position is then the sort's choice, as it is the reference's (an unstable select).
#pragma once

#ifndef CDEV      // the host build
#define PCT_HOST 1
#define CDEV static inline
#include <cmath>
namespace comet {
typedef long long i64;
}
#endif

namespace comet {

// one IEEE product, rounded, that no later sum or difference is fused with
CDEV double pct_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  volatile double r = a * b;
  return r;
#endif
}
CDEV double pct_add(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(a, b);
#else
  return a + b;
#endif
}

// spark_double_cmp(x, y) == Equal
CDEV bool pct_same(double x, double y) { return x == y || (x != x && y != y); }

// the percentile of n ≥ 1 values sorted ascending (NaN last) that start at `sorted`
CDEV double pct_pick(const double* sorted, i64 n, double p) {
  if (n == 1) return sorted[0];
  const double position = pct_mul((double)(n - 1), p);      // (never fused into position − floor)
  const double fl = floor(position), ce = ceil(position);
  i64 lower = (i64)fl, higher = (i64)ce;
  // (0 ≤ p ≤ 1 is the planner's to enforce, and then 0 ≤ lower ≤ higher ≤ n − 1; a caller that let something else through reads inside the group all the same)
  if (!(lower >= 0)) lower = 0;
  if (!(higher >= lower)) higher = lower;
  if (higher > n - 1) higher = n - 1;
  if (lower > higher) lower = higher;
  const double lo = sorted[lower];
  if (lower == higher) return lo;
  const double hi = sorted[higher];
  if (pct_same(lo, hi)) return lo;
  return pct_add(pct_mul(ce - position, lo), pct_mul(position - fl, hi));
}

}  // namespace comet
