"""Spark's exact percentile without a GPU: the pure-Python model (tests/percentile_model.py) against the reference's own known answers, the host diagnostic —
device/percentile.hpp's pick, compiled for the host — against the model bit for bit, and what createPlan accepts and refuses."""
import math
import random

import pytest

from datafusion_comet_amd import native, serde as S
from tests import percentile_model as M

F64, I32, I64 = S.T_DOUBLE, S.T_INT32, S.T_INT64
WITNESS, WITNESS_P = [-45.5, 28.4], 0.123456789


# --------------------------------------------------------------------------- the model

def test_model_reference_unit_test():
    assert M.percentile([0.0, 1e7], 0.123456789) == 1234567.89
    assert M.percentile([1e7, None, 0.0], 0.123456789) == 1234567.89


def test_model_edges():
    assert M.percentile([], 0.5) is None
    assert M.percentile([None, None], 0.5) is None
    assert M.percentile([3.25], 0.0) == M.percentile([3.25], 0.7) == M.percentile([None, 3.25], 1.0) == 3.25
    v = [5.0, -2.0, 9.5, 0.25, 7.0]
    assert M.percentile(v, 0.0) == -2.0 and M.percentile(v, 1.0) == 9.5
    assert M.percentile(v, 0.5) == 5.0      # lower == higher: no interpolation
    assert math.isnan(M.percentile([1.0, float("nan")], 1.0)) and M.percentile([float("nan"), 1.0], 0.0) == 1.0      # NaN is the greatest


def test_model_returns_lo_without_interpolating_when_lo_equals_hi():
    inf = float("inf")
    assert M.percentile([inf, inf], 0.3) == inf               # (0.7 · inf + 0.3 · inf is inf too, but 1 · inf + 0 · inf would be NaN: p → 0)
    assert M.percentile([inf, inf], 1e-300) == inf
    assert M.percentile([-inf, -inf, 1.0], 0.25) == -inf
    assert math.isnan(M.percentile([float("nan"), float("nan")], 0.5))
    for zs in ([-0.0, 0.0], [0.0, -0.0]):
        r = M.percentile(zs, 0.5)
        assert r == 0.0      # lo itself, whichever zero the sort put first
    assert M.percentile([2.5, 2.5, 2.5], 0.37) == 2.5


def test_witness_tells_fused_from_unfused():
    """[-45.5, 28.4] at p = 0.123456789: the formula with every operation rounded, and the same with one product kept exact inside a fused multiply-add (what
    a contracting compiler emits: fma(wl, lo, wh · hi)), differ in the last bit — shown in exact rational arithmetic"""
    lo, hi = WITNESS
    position = 1.0 * WITNESS_P
    wl, wh = 1.0 - position, position - 0.0
    unfused, fused_first, fused_second = M.interpolate_variants(lo, hi, wl, wh)
    assert unfused.hex() == "-0x1.230329214444ep+5"
    assert fused_first.hex() == "-0x1.230329214444fp+5"
    assert unfused != fused_first
    assert fused_second in (unfused, fused_first)
    assert M.percentile(WITNESS, WITNESS_P) == unfused


# --------------------------------------------------------------------------- the host diagnostic

def test_host_diagnostic_equals_the_model_on_the_witness_and_known_answers(built):
    assert native.spark_percentile_sorted(sorted(WITNESS), WITNESS_P).hex() == "-0x1.230329214444ep+5"
    assert native.spark_percentile_sorted([0.0, 1e7], 0.123456789) == 1234567.89
    assert native.spark_percentile_sorted([], 0.5) is None
    assert native.spark_percentile_sorted([7.5], 0.3) == 7.5
    inf = float("inf")
    assert native.spark_percentile_sorted([inf, inf], 0.3) == inf
    assert math.isnan(native.spark_percentile_sorted([1.0, float("nan"), float("nan")], 0.75))
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            native.spark_percentile_sorted([1.0, 2.0], bad)


def test_host_diagnostic_equals_the_model_bit_for_bit_on_random_cases(built):
    rng = random.Random(20261020)
    fixed = [0.0, 0.25, 0.5, 0.123456789, 0.95, 0.99, 1.0]
    specials = [0.0, -0.0, float("inf"), -float("inf"), float("nan"), 5e-324, -2.5e-310, 1.7976931348623157e308]
    sensitive = 0
    for case in range(10_000):
        n = 1 + case % 50
        scale = 10.0 ** rng.randint(-3, 6)
        vals = [rng.choice(specials) if rng.random() < 0.03 else rng.uniform(-scale, scale) for _ in range(n)]
        if rng.random() < 0.1:
            vals = [rng.choice(vals) for _ in range(n)]      # duplicates: lo == hi
        p = rng.choice(fixed) if rng.random() < 0.5 else rng.random()
        s = M.sort_values(vals)
        want = M.percentile_sorted(s, p)
        got = native.spark_percentile_sorted(s, p)
        assert M.same(got, want), (case, n, p, got, want)
        if n > 1 and not math.isnan(want) and not math.isinf(want):
            position = float(n - 1) * p
            lo_i, hi_i = math.floor(position), math.ceil(position)
            if lo_i != hi_i and M.cmp(s[lo_i], s[hi_i]) != 0 and all(math.isfinite(x) for x in (s[lo_i], s[hi_i])):
                u, f1, f2 = M.interpolate_variants(s[lo_i], s[hi_i], float(hi_i) - position, position - float(lo_i))
                assert u == want
                sensitive += u != f1 or u != f2
    assert sensitive > 1000, sensitive      # the cases really tell a fused multiply-add from the formula


# --------------------------------------------------------------------------- createPlan

def plan_of(mode, grouped, aggs=None, fields=None, keys=None):
    if mode == S.PARTIAL:
        fields = fields or [I32, F64]
        aggs = aggs or [S.percentile(S.col(1, F64), 0.5), S.percentile(S.col(1, F64), 0.25)]
        keys = keys if keys is not None else ([S.col(0, fields[0])] if grouped else [])
        return S.hash_agg(S.scan(fields), keys, aggs, mode)
    lst = S.list_type(F64, True)
    aggs = aggs or [S.percentile(S.col(1, F64), 0.5), S.percentile(S.col(1, F64), 0.25)]
    fields = ([I32] if grouped else []) + [lst] * len(aggs)
    return S.hash_agg(S.scan(fields), [S.col(0, I32)] if grouped else [], aggs, mode)


@pytest.mark.parametrize("mode", [S.PARTIAL, S.PARTIAL_MERGE, S.FINAL], ids=["partial", "partial_merge", "final"])
@pytest.mark.parametrize("grouped", [False, True], ids=["ungrouped", "grouped"])
def test_check_plan_accepts_percentile_only_aggregates(built, mode, grouped):
    ok, text = native.check_plan(plan_of(mode, grouped).encode())
    assert ok, text
    assert "percentile" in text


def refused(plan):
    ok, text = native.check_plan(plan.encode())
    assert not ok, text
    return text


def test_check_plan_accepts_median_with_a_filter_and_four_value_columns(built):
    x = S.col(1, F64)
    flt = S.gt(S.col(0, I32), S.lit(3, I32))
    ok, text = native.check_plan(S.hash_agg(S.scan([I32, F64]), [S.col(0, I32)], [S.percentile(x, 0.5, filter=flt), S.percentile(x, 0.5)], S.PARTIAL).encode())
    assert ok, text
    four = [S.percentile(S.col(1 + i, F64), 0.5) for i in range(4)] + [S.percentile(S.col(1, F64), 0.9)]
    ok, text = native.check_plan(S.hash_agg(S.scan([I32] + [F64] * 4), [], four, S.PARTIAL).encode())
    assert ok, text


def test_check_plan_refuses_by_name(built):
    x = S.col(1, F64)
    # beside another aggregate function
    text = refused(S.hash_agg(S.scan([I32, F64]), [S.col(0, I32)], [S.percentile(x, 0.5), S.sum_(x, F64)], S.PARTIAL))
    assert "percentile" in text and "mixed with other aggregate functions" in text and "sum" in text and "MI355X native engine" in text
    text = refused(S.hash_agg(S.scan([I32, F64]), [], [S.sum_(x, F64), S.percentile(x, 0.5)], S.PARTIAL))
    assert "percentile" in text and "mixed with other aggregate functions" in text
    # p outside [0, 1]: the reference's message
    text = refused(plan_of(S.PARTIAL, True, aggs=[S.percentile(x, 1.5)]))
    assert "Percentile value must be between 0.0 and 1.0 inclusive, got 1.5." in text
    text = refused(plan_of(S.FINAL, False, aggs=[S.percentile(x, float("nan"))]))
    assert "Percentile value must be between 0.0 and 1.0 inclusive, got NaN." in text
    # a column as percentage
    text = refused(plan_of(S.PARTIAL, True, aggs=[S.percentile(x, S.col(1, F64))]))
    assert "percentile" in text and "percentage must be a non-NULL Float64 literal" in text and "MI355X native engine" in text
    text = refused(plan_of(S.PARTIAL, True, aggs=[S.percentile(x, S.lit(1, I32))]))
    assert "percentile" in text and "percentage must be a non-NULL Float64 literal" in text
    # an Int64 child
    text = refused(plan_of(S.PARTIAL, True, fields=[I32, I64], aggs=[S.percentile(S.col(1, I64), 0.5)]))
    assert "SparkPercentile expects Float64 input, got" in text and "percentile" in text and "MI355X native engine" in text
    # a Float64 grouping key
    text = refused(plan_of(S.PARTIAL, True, fields=[F64, F64], aggs=[S.percentile(x, 0.5)]))
    assert "percentile" in text and "grouped by a" in text and "MI355X native engine" in text
    # five distinct value columns
    five = [S.percentile(S.col(1 + i, F64), 0.5) for i in range(5)]
    text = refused(S.hash_agg(S.scan([I32] + [F64] * 5), [S.col(0, I32)], five, S.PARTIAL))
    assert "percentile" in text and "more than 4 distinct value columns" in text and "MI355X native engine" in text
    # mixed per-expression modes
    text = refused(S.hash_agg(S.scan([I32, F64, S.list_type(F64, True)]), [S.col(0, I32)], [S.percentile(x, 0.5), S.percentile(x, 0.9)], S.PARTIAL,
                              expr_modes=[S.PARTIAL, S.PARTIAL_MERGE], initial_input_buffer_offset=2))
    assert "percentile" in text and "mixed-mode" in text and "MI355X native engine" in text
    # a merging aggregate over something that is no List<Float64> state
    text = refused(S.hash_agg(S.scan([I32, F64]), [S.col(0, I32)], [S.percentile(x, 0.5)], S.FINAL))
    assert "percentile" in text and "List<Float64> state" in text
