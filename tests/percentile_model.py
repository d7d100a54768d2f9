"""Spark's exact percentile as the reference computes it (native/spark-expr/src/agg_funcs/percentile.rs:280-319), in plain Python floats — the model the
percentile tests compare against.  Python's float is an IEEE double and `a * b + c * d` here is two rounded products and one rounded sum, which is the
point: a fused multiply-add gives other bits in about a quarter of the cases.  No NumPy interpolation: numpy.percentile's "linear" method is another formula."""
import functools
import math
from fractions import Fraction


def cmp(x: float, y: float) -> int:
    """spark_double_cmp: NaN is the greatest value and equals NaN, -0.0 equals 0.0"""
    if x == y or (math.isnan(x) and math.isnan(y)):
        return 0
    if math.isnan(x):
        return 1
    if math.isnan(y):
        return -1
    return -1 if x < y else 1


def sort_values(values):
    return sorted(values, key=functools.cmp_to_key(cmp))


def percentile_sorted(s, p: float):
    """the percentile of the values `s`, already in spark_double_cmp order; None for none"""
    n = len(s)
    if n == 0:
        return None
    if n == 1:
        return s[0]
    position = float(n - 1) * p
    lower, higher = math.floor(position), math.ceil(position)
    lo = s[lower]
    if lower == higher:
        return lo
    hi = s[higher]
    if cmp(lo, hi) == 0:
        return lo
    return (float(higher) - position) * lo + (position - float(lower)) * hi


def percentile(values, p: float):
    """percentile(x, p) over `values`, None = NULL (dropped)"""
    return percentile_sorted(sort_values([v for v in values if v is not None]), p)


def same(a, b) -> bool:
    """the tests' equality: NULL = NULL, NaN = NaN, zeros equal, everything else bit for bit (== on doubles is that, zeros and NaN apart)"""
    if a is None or b is None:
        return a is None and b is None
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return a == b


def same_multiset(a, b) -> bool:
    """two lists of kept values as multisets under `same`"""
    if len(a) != len(b):
        return False
    return all(same(x, y) for x, y in zip(sort_values(a), sort_values(b)))


def _round(fr: Fraction) -> float:
    """an exact rational, rounded once to the nearest double (ties to even) — Fraction's own conversion does exactly that"""
    return fr.numerator / fr.denominator


def interpolate_variants(lo: float, hi: float, wl: float, wh: float):
    """wl · lo + wh · hi three ways, in exact rational arithmetic: unfused (each product rounded, then the sum), the first product kept exact inside a fused
    multiply-add, the second one kept exact"""
    L, H, WL, WH = Fraction(lo), Fraction(hi), Fraction(wl), Fraction(wh)
    unfused = _round(Fraction(_round(WL * L)) + Fraction(_round(WH * H)))
    fused_first = _round(WL * L + Fraction(_round(WH * H)))
    fused_second = _round(Fraction(_round(WL * L)) + WH * H)
    return unfused, fused_first, fused_second
