"""ANSI / TRY integer sums in a HashAggregate and Spark's rewritten decimal sums (unscaled_value / make_decimal) on the GPU.

Semantics restated from the reference (agg_funcs/sum_int.rs; math_funcs/internal/unscaled_value.rs, make_decimal.rs):
  * the reference adds the non-NULL values of a group in row order with add_checked.  ANSI (:178-248, :537-686): an overflowing step fails the task with
    ARITHMETIC_OVERFLOW / "integer"; state = one nullable Int64; a merge is the same checked sum over the partial sums.  TRY (:251-391, :688-890): state =
    (sum: Int64 nullable, has_all_nulls: Boolean); (NULL, false) is "overflowed" and stays so through updates and merges; an untouched state is (0, true); the
    result is NULL for "no value" and for "overflowed".
  * the engine decides from order-independent facts.  P = the exact sum of a group's positive addends, N = of its negative ones, T = P + N:
      case 1  P <= 2^63 - 1 and N >= -2^63: no prefix of any order overflows, the answer is T
      case 2  T outside Int64: every order overflows
      case 3  otherwise the reference's own answer depends on the row order: the task fails with "... cannot be decided order-independently ..."
  * unscaled_value(decimal(p <= 18, s)) is the stored integer; make_decimal(Int64) -> decimal(p, s) takes the integer as the unscaled value; beyond 10^p - 1 it is
    NULL, or under fail_on_error NUMERIC_VALUE_OUT_OF_RANGE naming the value; a NULL slot never raises whatever lies under it.
The expectations are the model below — sum_int.rs in plain Python integers — which ASSERTS case 1 or case 2 of every group it is asked about, so no order-dependent
input can slip into a value comparison; case 3 appears only where the named error is expected.  Results and states are compared per group key (keys are unique: a
multiset comparison) and must be the same for one chunk and for several.
"""
import decimal
import json

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S

pytestmark = pytest.mark.gpu
I8, I32, I64 = S.T_INT8, S.T_INT32, S.T_INT64
MODES = {"ansi": S.ANSI, "try": S.TRY}
TYPES = {"Int8": (I8, np.int8, 7), "Int32": (I32, np.int32, 31), "Int64": (I64, np.int64, 63)}
I64_MIN, I64_MAX = -2**63, 2**63 - 1
ONE_CHUNK = (1 << 20, 1 << 20)      # (most rows per host batch, spark.comet.gpu.chunkRows): the whole input is one batch and one chunk
SEVERAL = (500, 1024)               # … batches of 500 rows, chunks of 1024
D72 = S.decimal(7, 2)


# --------------------------------------------------------------------------- the model (sum_int.rs)

class Overflow(Exception):
    pass


def add_checked(a, b):
    s = a + b
    return s if I64_MIN <= s <= I64_MAX else None


def case_of(vals):
    p, n = sum(v for v in vals if v > 0), sum(v for v in vals if v < 0)
    if p <= I64_MAX and n >= I64_MIN:
        return 1
    return 2 if not (I64_MIN <= p + n <= I64_MAX) else 3


def update(vals, mode):
    """the Partial state of one group's non-NULL values, in row order"""
    assert case_of(vals) in (1, 2), "an order-dependent input in a value comparison"
    if mode == "ansi":      # SumIntegerAccumulatorAnsi::update_batch / SumIntGroupsAccumulatorAnsi
        s = None
        for v in vals:
            s = add_checked(s or 0, v)
            if s is None:
                raise Overflow()
        return (s,)
    s, all_nulls = 0, True      # SumIntGroupsAccumulatorTry::update_batch
    for v in vals:
        if not all_nulls and s is None:
            continue
        s = add_checked(s or 0, v)
        all_nulls = False
    return (s, all_nulls)


def merge(states, mode):
    """merge_batch over one group's state rows, in order"""
    if mode == "ansi":
        return update([st[0] for st in states if st[0] is not None], mode)
    assert case_of([st[0] for st in states if not st[1] and st[0] is not None]) in (1, 2), "an order-dependent input in a value comparison"
    s, all_nulls = 0, True      # SumIntGroupsAccumulatorTry::merge_batch
    for that, that_all_nulls in states:
        if (not that_all_nulls and that is None) or (not all_nulls and s is None):
            s, all_nulls = None, False
        elif that_all_nulls:
            continue
        elif all_nulls:
            s, all_nulls = that, False
        else:
            s = add_checked(s, that)
    return (s, all_nulls)


def evaluate(state, mode):
    return state[0] if mode == "ansi" or not state[1] else None


def make_decimal_model(v, p, s):
    return None if v is None or abs(v) > 10**p - 1 else decimal.Decimal(v).scaleb(-s)


def unscaled_value_model(d, s):
    return None if d is None else int(d.scaleb(s))


# --------------------------------------------------------------------------- helpers

def run(plan, table, ncols, cfg=ONE_CHUNK):
    max_batch, chunk = cfg
    # batches of equal size: a last batch of a few rows may hold no NULL at all, and an aggregate whose chunks differ in which columns carry validity is not what is
    # tested here (the executor wants one accumulator layout for all chunks of a task)
    batch_rows = -(-table.num_rows // max(-(-table.num_rows // max_batch), 1)) or 1
    out = native.execute_to_table([native.HostInput.from_table(table, batch_rows)], ncols, plan.encode(), batch_size=0, config=S.config_map({"spark.comet.gpu.chunkRows": chunk}))
    return pa.Table.from_batches(out) if out else None


def rows_of(t):
    return [] if t is None else list(zip(*[t.column(i).to_pylist() for i in range(t.num_columns)]))


def keyed(t, grouped, width):
    """{key: (columns…)}; an ungrouped result is its one row under the key ()"""
    rows = rows_of(t)
    if not grouped:
        assert len(rows) == 1, rows
        return {(): rows[0]}
    out = {r[0]: r[1:] for r in rows}
    assert len(out) == len(rows) and all(len(v) == width for v in out.values())
    return out


def arity(mode):
    return 1 if mode == "ansi" else 2


def state_types(mode):
    return [pa.int64()] if mode == "ansi" else [pa.int64(), pa.bool_()]


def error_json(excinfo):
    return json.loads(str(excinfo.value))


def raises_integer_overflow(plan, table, ncols, cfg=ONE_CHUNK):
    with pytest.raises(native.CometQueryExecutionException) as e:
        run(plan, table, ncols, cfg)
    j = error_json(e)
    assert j["errorClass"] == "ARITHMETIC_OVERFLOW" and j["params"] == {"fromType": "integer"}, j


def value_table(tname, n, ngroups, seed, rows_per_group):
    """(g: Int32 with NULL keys, x: the type with NULLs, f: Int32) — |x| is bounded so that no group's positive or negative sum can leave Int64 (case 1 everywhere),
    yet an Int64 reaches into the upper limb"""
    _, npt, bits = TYPES[tname]
    rng = np.random.default_rng(seed)
    mag = min(2**bits, 2**62 // max(rows_per_group, 1))
    x = rng.integers(-mag, mag, n).astype(npt)
    g = rng.integers(0, max(ngroups, 1), n).astype(np.int32)
    return pa.table({"g": pa.array(g, mask=rng.random(n) < 0.02), "x": pa.array(x, mask=rng.random(n) < 0.2), "f": pa.array(rng.integers(-5, 6, n).astype(np.int32), mask=rng.random(n) < 0.1)})


def append_rows(t, rows):
    extra = pa.table([pa.array([r[i] for r in rows], t.schema.field(i).type) for i in range(3)], names=t.schema.names)
    return pa.concat_tables([t, extra]).combine_chunks()


def shuffled(t, seed):
    return t.take(pa.array(np.random.default_rng(seed).permutation(t.num_rows)))


def sum_plan(tname, mode, grouped, source=None):
    t = TYPES[tname][0]
    types = [I32, t, I32]
    x = S.col(1, t)
    aggs = [S.sum_(x, I64, MODES[mode]), S.sum_(x, I64, MODES[mode], filter=S.gt(S.col(2, I32), S.lit(0, I32)))]
    return S.hash_agg(source if source is not None else S.scan(types), [S.col(0, I32)] if grouped else [], aggs)


def final_plan(mode, grouped, naggs, plan_mode=S.FINAL):
    nk = 1 if grouped else 0
    st = [I64] if mode == "ansi" else [I64, S.T_BOOL]
    aggs = [S.sum_(S.col(0, I64), I64, MODES[mode]) for _ in range(naggs)]
    return S.hash_agg(S.scan([I32] * nk + st * naggs), [S.col(0, I32)] * nk, aggs, plan_mode)


def expected_states(table, mode, grouped):
    """{key: the state columns of sum(x) and of sum(x) FILTER (WHERE f > 0)} by a walk in row order"""
    groups = {} if grouped else {(): []}
    for g, x, f in rows_of(table):
        groups.setdefault(g if grouped else (), []).append((x, f))
    out = {}
    for k, rs in groups.items():
        out[k] = update([x for x, _ in rs if x is not None], mode) + update([x for x, f in rs if x is not None and f is not None and f > 0], mode)
    return out


def check_partial_then_final(tname, mode, grouped, table, cfgs):
    """Partial at each configuration: the states are the model's and the same everywhere; Final over the engine's own states: the model's results"""
    a = arity(mode)
    want = expected_states(table, mode, grouped)
    plan = sum_plan(tname, mode, grouped)
    states = None
    for cfg in cfgs:
        got = run(plan, table, (1 if grouped else 0) + 2 * a, cfg)
        if grouped and not want:
            assert got is None or got.num_rows == 0
            continue
        k = keyed(got, grouped, 2 * a)
        bad = [(key, k.get(key), want[key]) for key in want if k.get(key) != want[key]]
        assert len(k) == len(want) and not bad, (cfg, len(k), len(want), bad[:5])
        states = got
    if states is None:
        return
    names = [f"s{i}" for i in range(states.num_columns)]
    want_res = {key: (evaluate(st[:a], mode), evaluate(st[a:], mode)) for key, st in want.items()}
    for cfg in (ONE_CHUNK, SEVERAL):
        r = keyed(run(final_plan(mode, grouped, 2), states.rename_columns(names), (1 if grouped else 0) + 2, cfg), grouped, 2)
        assert r == want_res, (cfg, [(key, r.get(key), want_res[key]) for key in want_res if r.get(key) != want_res[key]][:5])


# --------------------------------------------------------------------------- the scalar functions

def test_scalar_functions(built):
    """one Projection over 300 rows (more than one wave, not a multiple of 64) with NULLs; make_decimal(…, 17, 2) at ±(10^17 − 1) and ±10^17"""
    n, p, s = 300, 17, 2
    rng = np.random.default_rng(5)
    xs = [int(v) for v in rng.integers(-10**17 + 1, 10**17, n)]
    for i, v in enumerate((10**p - 1, -(10**p - 1), 10**p, -(10**p), I64_MAX, I64_MIN, 0)):
        xs[7 + 41 * i] = v
    xs = [None if i % 11 == 3 else v for i, v in enumerate(xs)]
    ds = [None if i % 13 == 5 else decimal.Decimal(int(v)).scaleb(-2) for i, v in enumerate(rng.integers(-10**7 + 1, 10**7, n))]
    ds[0], ds[1] = decimal.Decimal(10**7 - 1).scaleb(-2), decimal.Decimal(-(10**7 - 1)).scaleb(-2)
    t = pa.table({"x": pa.array(xs, pa.int64()), "d": pa.array(ds, pa.decimal128(7, 2))})
    x, d = S.col(0, I64), S.col(1, D72)
    plan = S.project(S.scan([I64, D72]), [S.make_decimal(x, p, s), S.unscaled_value(d), S.make_decimal(S.unscaled_value(d), p, s, null_on_overflow=False)])
    got = run(plan, t, 3)
    assert got.schema.field(0).type == pa.decimal128(17, 2) and got.schema.field(1).type == pa.int64()
    assert got.column(0).to_pylist() == [make_decimal_model(v, p, s) for v in xs]
    assert got.column(0).null_count == sum(v is None or abs(v) >= 10**p for v in xs) > sum(v is None for v in xs)
    assert got.column(1).to_pylist() == [unscaled_value_model(v, 2) for v in ds]
    assert got.column(2).to_pylist() == ds      # unscaled_value and make_decimal back: the decimal itself, at the wider precision
    # fail_on_error: the first value that does not fit fails the task, by its unscaled digits
    strict = S.project(S.scan([I64, D72]), [S.make_decimal(x, p, s, null_on_overflow=False)])
    fits = [v if v is None or abs(v) < 10**p else 1 for v in xs]
    assert run(strict, t.set_column(0, "x", pa.array(fits, pa.int64())), 1).column(0).to_pylist() == [make_decimal_model(v, p, s) for v in fits]
    one_bad = list(fits)
    one_bad[130] = -(10**p)
    with pytest.raises(native.CometQueryExecutionException) as e:
        run(strict, t.set_column(0, "x", pa.array(one_bad, pa.int64())), 1)
    j = error_json(e)
    assert j["errorClass"].startswith("NUMERIC_VALUE_OUT_OF_RANGE") and j["params"] == {"value": str(-(10**p)), "precision": p, "scale": s}, j
    # a NULL slot over an out-of-range physical value does not raise
    raw = np.array([5, 10**p, -3, I64_MAX], np.int64)
    hidden = pa.Array.from_buffers(pa.int64(), 4, [pa.py_buffer(bytes([0b0101])), pa.py_buffer(raw.tobytes())], null_count=2)
    got = run(strict, pa.table({"x": hidden, "d": pa.array([None] * 4, pa.decimal128(7, 2))}), 1)
    assert got.column(0).to_pylist() == [decimal.Decimal(5).scaleb(-2), None, decimal.Decimal(-3).scaleb(-2), None]


# --------------------------------------------------------------------------- the sums

# Int64 groups at the edges: (rows, case)
EDGE_FITS = {1_000_001: [2**62, -2**62, 2**62 - 1, -2**62],      # P = 2^63 − 1 and N = −2^63 together (case 1: max|v| · count and the signs prove nothing here), T = −1
             1_000_003: [-2**62, -2**62]}                        # T = −2^63 exactly: fits
EDGE_OVERFLOWS = {1_000_002: [2**62, 2**62]}                     # T = 2^63: case 2


@pytest.mark.parametrize("tname", sorted(TYPES))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_ungrouped(built, mode, tname):
    assert case_of(EDGE_FITS[1_000_001]) == 1 and case_of(EDGE_FITS[1_000_003]) == 1 and case_of(EDGE_OVERFLOWS[1_000_002]) == 2
    for n in (0, 1, 257, 3000):      # 3000 rows: several chunks at the second configuration
        t = value_table(tname, n, 1, 100 + n, n)
        check_partial_then_final(tname, mode, False, t, (ONE_CHUNK, SEVERAL) if n else (ONE_CHUNK,))
    all_null = pa.table({"g": pa.array([1, 1, 1], pa.int32()), "x": pa.array([None] * 3, pa.from_numpy_dtype(TYPES[tname][1])), "f": pa.array([1, 1, 1], pa.int32())})
    check_partial_then_final(tname, mode, False, all_null, (ONE_CHUNK,))
    if tname != "Int64":
        return
    for vals in EDGE_FITS.values():
        t = pa.table({"g": pa.array([1] * len(vals), pa.int32()), "x": pa.array(vals, pa.int64()), "f": pa.array([1] * len(vals), pa.int32())})
        check_partial_then_final(tname, mode, False, t, (ONE_CHUNK,))
    vals = EDGE_OVERFLOWS[1_000_002]
    t = pa.table({"g": pa.array([1] * len(vals), pa.int32()), "x": pa.array(vals, pa.int64()), "f": pa.array([1] * len(vals), pa.int32())})
    if mode == "ansi":
        raises_integer_overflow(sum_plan(tname, mode, False), t, 2)
    else:
        check_partial_then_final(tname, mode, False, t, (ONE_CHUNK,))
        assert rows_of(run(sum_plan(tname, mode, False), t, 4)) == [(None, False, None, False)]


@pytest.mark.parametrize("ngroups", [3, 700, 40_000])      # the private LDS copies; the block's LDS table; the global table / the partitioned merge
@pytest.mark.parametrize("tname", sorted(TYPES))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_grouped(built, mode, tname, ngroups):
    n = {3: 3000, 700: 7000, 40_000: 120_000}[ngroups]
    t = value_table(tname, n, ngroups, ngroups + 7, max(4 * n // ngroups + 64, n // 25))      # (the NULL key's group holds about n / 50 rows)
    t = append_rows(t, [(2_000_000, None, 1)] * 3)      # an all-NULL group
    edge = dict(EDGE_FITS)
    if mode == "try":
        edge.update(EDGE_OVERFLOWS)
    if tname == "Int64":
        t = append_rows(t, [(k, v, 1) for k, vals in edge.items() for v in vals])
    t = shuffled(t, ngroups)
    several = SEVERAL if ngroups < 40_000 else (8192, 32768)
    check_partial_then_final(tname, mode, True, t, (ONE_CHUNK, several))
    if tname == "Int64" and mode == "ansi" and ngroups == 3:
        bad = shuffled(append_rows(t, [(k, v, 0) for k, vals in EDGE_OVERFLOWS.items() for v in vals]), 1)      # (f = 0: only the unfiltered sum overflows)
        raises_integer_overflow(sum_plan(tname, mode, True), bad, 3, SEVERAL)


# --------------------------------------------------------------------------- two and three stages

@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_partial_final_and_partial_merge(built, mode, grouped):
    a = arity(mode)
    nk = 1 if grouped else 0
    # hand-made states: {group: state rows in order}
    if mode == "try":
        groups = {1: [(5, False), (None, False), (7, False)],                     # an overflowed incoming state is sticky
                  2: [(0, True), (0, True)],                                      # all-NULL states merge as nothing
                  3: [(2**62, False), (2**62, False)],                            # only the merge overflows
                  4: [(0, True), (9, False), (0, True)],
                  5: [(2**62, False), (-2**62, False), (2**62 - 1, False), (-2**62, False)]}
    else:
        groups = {1: [(5,), (None,), (7,)], 2: [(None,), (None,)], 4: [(None,), (9,)], 5: [(2**62,), (-2**62,), (2**62 - 1,), (-2**62,)], 6: [(-2**62,), (-2**62,)]}
    def state_table(rows):
        types = ([pa.int32()] if grouped else []) + state_types(mode)
        return pa.table([pa.array(list(c), ty) for c, ty in zip(zip(*rows), types)], names=[f"s{i}" for i in range(len(types))])

    # grouped: all the groups in one table; ungrouped: each group's state rows are an input of their own
    inputs = [(groups, state_table([(k,) + st for k, ss in groups.items() for st in ss]))] if grouped else [({(): ss}, state_table(ss)) for ss in groups.values()]
    for mode_of_plan in (S.FINAL, S.PARTIAL_MERGE):
        width = 1 if mode_of_plan == S.FINAL else a
        for gs, st_table in inputs:
            got = keyed(run(final_plan(mode, grouped, 1, mode_of_plan), st_table, nk + width), grouped, width)
            merged = {k: merge(ss, mode) for k, ss in gs.items()}
            want = {k: ((evaluate(m, mode),) if mode_of_plan == S.FINAL else m) for k, m in merged.items()}
            assert got == want, (mode_of_plan, got, want)
    if mode == "try":
        assert merge(groups[1], mode) == (None, False) and merge(groups[3], mode) == (None, False) and merge(groups[2], mode) == (0, True)
    else:
        # ANSI raises when only the merge overflows
        st_table = state_table([(1, 2**62), (1, 2**62), (2, 1)] if grouped else [(2**62,), (2**62,)])
        for mode_of_plan in (S.FINAL, S.PARTIAL_MERGE):
            raises_integer_overflow(final_plan(mode, grouped, 1, mode_of_plan), st_table, nk + 1)
    # the engine's own states: Partial over three slices → PartialMerge over the first two → Final over (merged, third) = the one-stage answer
    t = shuffled(value_table("Int64", 3000, 40, 77, 400 if grouped else 4000), 4)      # (about 75 rows a group, 60 under the NULL key)
    if mode == "try" and grouped:      # … with a group that overflows in the first slice's Partial and stays overflowed through both merges
        t = append_rows(t.slice(0, 500), [(k, v, 1) for k, vals in EDGE_OVERFLOWS.items() for v in vals] + rows_of(t.slice(500)) + [(1_000_002, 5, 1)])
    one_stage = {k: (evaluate(st[:a], mode), evaluate(st[a:], mode)) for k, st in expected_states(t, mode, grouped).items()}
    plan = sum_plan("Int64", mode, grouped)
    parts = [run(plan, t.slice(i * 1010, 1010), nk + 2 * a) for i in range(3)]
    stack = lambda ts: pa.table([pa.concat_arrays([c for x in ts for c in x.column(i).chunks]) for i in range(ts[0].num_columns)], names=[f"s{i}" for i in range(ts[0].num_columns)])
    merged = run(final_plan(mode, grouped, 2, S.PARTIAL_MERGE), stack(parts[:2]), nk + 2 * a)
    assert keyed(merged, grouped, 2 * a) == expected_states(t.slice(0, 2020), mode, grouped)
    got = run(final_plan(mode, grouped, 2), stack([merged, parts[2]]), nk + 2, (97, 1024))
    assert keyed(got, grouped, 2) == one_stage


# --------------------------------------------------------------------------- case 3: never a value, never ARITHMETIC_OVERFLOW

@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_an_order_dependent_sum_fails_by_name(built, mode, grouped):
    vals = [2**62, 2**62, -2**62]
    assert case_of(vals) == 3
    for order in (vals, vals[::-1]):
        rows = [(7, v, 1) for v in order] + [(8, 1, 1)]
        t = pa.table({"g": pa.array([r[0] for r in rows], pa.int32()), "x": pa.array([r[1] for r in rows], pa.int64()), "f": pa.array([r[2] for r in rows], pa.int32())})
        with pytest.raises(native.CometNativeException, match="cannot be decided order-independently"):
            run(sum_plan("Int64", mode, grouped), t, (1 if grouped else 0) + 2 * arity(mode))
        # … and in a merge of the same partial sums
        st = [((7,) if grouped else ()) + ((v,) if mode == "ansi" else (v, False)) for v in order]
        types = ([pa.int32()] if grouped else []) + state_types(mode)
        st_table = pa.table([pa.array(list(c), ty) for c, ty in zip(zip(*st), types)], names=[f"s{i}" for i in range(len(types))])
        with pytest.raises(native.CometNativeException, match="cannot be decided order-independently"):
            run(final_plan(mode, grouped, 1), st_table, (1 if grouped else 0) + 1)


# --------------------------------------------------------------------------- as Spark plans it

def q95_shaped_table():
    """5 000 rows of decimal(7,2) in 50 groups of 100.  Each group has 1, 3, 7 or 9 NULLs, so its count of values (99, 97, 93, 91) has no factor 2 or 5: the exact
    average, scaled to six digits, then lies at least 1 / (2 · 99) from a rounding tie — far beyond the error of the Float64 route Spark's rewrite takes — and both
    routes must round to the same decimal."""
    rng = np.random.default_rng(95)
    g = np.repeat(np.arange(50, dtype=np.int32), 100)
    v = [decimal.Decimal(int(x)).scaleb(-2) for x in rng.integers(-10**7 + 1, 10**7, 5000)]
    for k in range(50):
        for j in range((1, 3, 7, 9)[k % 4]):
            v[100 * k + 11 * j + 2] = None
    perm = rng.permutation(5000)
    return pa.table({"g": pa.array(g), "x": pa.array(v, pa.decimal128(7, 2))}).take(pa.array(perm))


def test_the_rewritten_decimal_sum_and_average_equal_the_direct_plan(built):
    """DecimalAggregates: sum(x) → MakeDecimal(sum(UnscaledValue(x)), 17, 2); avg(x) → cast(avg(UnscaledValue(x)) / 100.0 as decimal(11,6)).  The yardstick is the
    direct plan sum(x): decimal(17,2) / avg(x): decimal(11,6) over the same table."""
    t = q95_shaped_table()
    counts = {}
    for k, x in rows_of(t):
        counts[k] = counts.get(k, 0) + (x is not None)
    assert len(counts) == 50 and all(c % 2 and c % 5 for c in counts.values())
    D17, D11 = S.decimal(17, 2), S.decimal(11, 6)
    k, x = S.col(0, I32), S.col(1, D72)
    direct = [S.sum_(x, D17), S.avg(x, D11, D17)]
    p = run(S.hash_agg(S.scan([I32, D72]), [k], direct), t, 5, SEVERAL)
    want = keyed(run(S.hash_agg(S.scan([I32, D17, S.T_BOOL, D17, I64]), [k], direct, S.FINAL), p.rename_columns([f"s{i}" for i in range(5)]), 3), True, 2)
    u = S.unscaled_value(x)
    rewritten = [S.sum_(u, I64, S.ANSI), S.avg(u, S.T_DOUBLE, S.T_DOUBLE)]
    p = run(S.hash_agg(S.scan([I32, D72]), [k], rewritten), t, 4, SEVERAL)
    final = S.hash_agg(S.scan([I32, I64, S.T_DOUBLE, I64]), [k], rewritten, S.FINAL)
    top = S.project(final, [S.col(0, I32), S.make_decimal(S.col(1, I64), 17, 2, null_on_overflow=False),
                            S.cast(S.math("divide", S.col(2, S.T_DOUBLE), S.lit(100.0, S.T_DOUBLE), S.T_DOUBLE), D11)])
    res = run(top, p.rename_columns([f"s{i}" for i in range(4)]), 3)
    assert res.schema.field(1).type == pa.decimal128(17, 2) and res.schema.field(2).type == pa.decimal128(11, 6)
    got = keyed(res, True, 2)
    assert got == want, [(key, got.get(key), want[key]) for key in want if got.get(key) != want[key]][:5]
    assert all(v[0] is not None and v[1] is not None for v in want.values())
