"""first / last and bit_and / bit_or / bit_xor in a HashAggregate on the GPU.

Semantics restated from the reference (planner.rs:2679-2735 → DataFusion's FirstValue / LastValue without ORDER BY and bit_and_udaf / bit_or_udaf / bit_xor_udaf;
JVM side aggregates.scala:240-420):
  * first / last: "first" is first in the order rows reach the aggregate — batches in the order executePlan pulls them, rows in batch order, behind the chain's Filters and the
    aggregate's own FILTER.  ignore_nulls = false: that row's value (NULL if it is NULL); ignore_nulls = true: the first non-NULL value, NULL if there is none.  An empty
    ungrouped input gives one row of NULL.  Partial state = (value, is_set); Final / PartialMerge take the first (last) state row with is_set = true, in state-row order.
  * bit aggregates: NULLs and rows failing the FILTER are skipped, a group with no contributing row is NULL; state = result = one nullable column of the input's type.
The expectations are a dict walk in row order / functools.reduce below.  Floats are compared as BITS.  The answer must depend on the row order only: not on batch size,
chunking, grid or which table (registers, LDS, global, partitioned merge) the groups went through.
"""
import decimal
import functools
import operator

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S

pytestmark = pytest.mark.gpu
I8, I32, I64, F64 = S.T_INT8, S.T_INT32, S.T_INT64, S.T_DOUBLE
decimal.getcontext().prec = 60


# --------------------------------------------------------------------------- helpers

def values(col):
    """a column as python values; floats as their bit patterns (ints), so that NaN payloads, -0.0 and ±inf compare exactly"""
    a = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if pa.types.is_floating(a.type):
        w = np.int64 if a.type == pa.float64() else np.int32
        raw = np.frombuffer(a.buffers()[1], dtype=w)[a.offset:a.offset + len(a)]
        ok = a.is_valid().to_pylist()
        return [int(raw[i]) if ok[i] else None for i in range(len(a))]
    if pa.types.is_timestamp(a.type) or pa.types.is_date(a.type):
        return a.cast(pa.int64() if pa.types.is_timestamp(a.type) else pa.int32()).to_pylist()
    return a.to_pylist()


def table_rows(t):
    cols = [values(t.column(i)) for i in range(t.num_columns)]
    return list(zip(*cols)) if cols else []


WIDTH = {"first": 2, "last": 2, "bit_and": 1, "bit_or": 1, "bit_xor": 1, "count": 1, "sum": 1}


def run(plan, table, ncols, batch_rows=8192, config=None):
    kw = {"config": S.config_map(config)} if config else {}
    out = native.execute_to_table([native.HostInput.from_table(table, batch_rows)], ncols, plan.encode(), batch_size=0, **kw)
    return pa.Table.from_batches(out) if out else None


def run_metrics(plan, inputs, ncols):
    it = native.CometExecIterator(inputs, ncols, plan.encode(), batch_size=0)
    batches = []
    while True:
        b = native.Native.executePlan(it.handle, ncols)
        if b is None:
            break
        batches.append(b)
    m = S.decode_metric_node(it.metrics())[0]
    it.close()
    return (pa.Table.from_batches(batches) if batches else None), m


def by_key(t, nkeys=1):
    if t is None:
        return {}
    return {r[:nkeys] if nkeys > 1 else r[0]: r[nkeys:] for r in table_rows(t)}


# the model: spec = (kind, column, ignore_nulls, filter(row) or None)
def model_state(rows, spec):
    """the Partial state of one group's rows (in order): (value, is_set) for first / last, the value for the others"""
    kind, c, ignore, flt = spec
    rows = [r for r in rows if flt is None or flt(r)]
    if kind in ("first", "last"):
        cand = [r[c] for r in rows if not (ignore and r[c] is None)]
        if not cand:
            return (None, False)
        return (cand[0] if kind == "first" else cand[-1], True)
    vals = [r[c] for r in rows if r[c] is not None]
    if kind == "count":
        return (len(vals),)
    if kind == "sum":
        return (sum(vals) if vals else None,)
    op = {"bit_and": operator.and_, "bit_or": operator.or_, "bit_xor": operator.xor}[kind]
    return (functools.reduce(op, vals) if vals else None,)


def model(rows, key_col, specs, final=False):
    """{key: state columns} by a dict walk in row order (key_col None: one group, present even when empty)"""
    groups = {}
    if key_col is None:
        groups[()] = list(rows)
    else:
        for r in rows:
            groups.setdefault(r[key_col], []).append(r)
    out = {}
    for k, rs in groups.items():
        st = []
        for sp in specs:
            s = model_state(rs, sp)
            st.extend(s[:1] if (final and sp[0] in ("first", "last")) else s)
        out[k] = tuple(st)
    return out


def agg_of(spec, types):
    kind, c, ignore, _ = spec[:4]
    e, t = S.col(c, types[c]), types[c]
    flt = spec[4] if len(spec) > 4 else None
    if kind == "first":
        return S.first_(e, t, ignore, filter=flt)
    if kind == "last":
        return S.last_(e, t, ignore, filter=flt)
    if kind == "count":
        return S.count(e)
    if kind == "sum":
        return S.sum_(e, I64)
    return {"bit_and": S.bit_and_agg, "bit_or": S.bit_or_agg, "bit_xor": S.bit_xor_agg}[kind](e, t, filter=flt)


def plan_of(types, key_col, specs, mode=S.PARTIAL, source=None):
    keys = [] if key_col is None else [S.col(key_col, types[key_col])]
    return S.hash_agg(source if source is not None else S.scan(types), keys, [agg_of(sp, types) for sp in specs], mode)


def ncols_of(key_col, specs, final=False):
    return (0 if key_col is None else 1) + sum(1 if (final and sp[0] in ("first", "last")) else WIDTH[sp[0]] for sp in specs)


def check(table, key_col, specs, batch_rows=8192, config=None, label=""):
    types = [S.from_arrow_type(f.type) for f in table.schema]
    got = run(plan_of(types, key_col, specs), table, ncols_of(key_col, specs), batch_rows, config)
    want = model(table_rows(table), key_col, [sp[:4] for sp in specs])
    if key_col is None:
        assert got is not None and got.num_rows == 1, label
        assert table_rows(got)[0] == want[()], (label, table_rows(got)[0], want[()])
    else:
        g = by_key(got)
        assert len(g) == len(want) == (got.num_rows if got is not None else 0), (label, len(g), len(want))
        bad = [(k, g[k], want[k]) for k in want if g[k] != want[k]]
        assert not bad, (label, len(bad), bad[:5])
    return got


# --------------------------------------------------------------------------- the small shapes (first_last.sql's, typed in as values)

SMALL = [  # (group, x)
    (1, None), (1, 10), (1, 20),          # NULL at the start
    (2, 30), (2, None), (2, 40),          # … in the middle
    (3, 50), (3, 60), (3, None),          # … at the end
    (4, None), (4, None),                 # an all-NULL group
    (5, 70),                              # a single row
    (6, None),                            # a single NULL
]


@pytest.mark.parametrize("grouped", [False, True])
def test_small_shapes(built, grouped):
    t = pa.table({"g": pa.array([r[0] for r in SMALL], pa.int32()), "x": pa.array([r[1] for r in SMALL], pa.int64())})
    specs = [("first", 1, False, None), ("first", 1, True, None), ("last", 1, False, None), ("last", 1, True, None), ("count", 1, False, None), ("sum", 1, False, None)]
    got = check(t, 0 if grouped else None, specs)
    if grouped:
        g = by_key(got)
        assert g[1][:8] == (None, True, 10, True, 20, True, 20, True)
        assert g[3][:8] == (50, True, 50, True, None, True, 60, True)
        assert g[4] == (None, True, None, False, None, True, None, False, 0, None)
        assert g[6] == (None, True, None, False, None, True, None, False, 0, None)
    else:
        assert table_rows(got)[0] == (None, True, 10, True, None, True, 70, True, 7, 280)
    for rows in ([(9, 5)], [(9, None)], []):      # a single row, a single NULL, an empty input
        t1 = pa.table({"g": pa.array([r[0] for r in rows], pa.int32()), "x": pa.array([r[1] for r in rows], pa.int64())})
        got = check(t1, 0 if grouped else None, specs, label=str(rows))
        if not rows:
            if grouped:
                assert got is None or got.num_rows == 0
            else:      # an empty ungrouped input: one row, every first / last NULL and not set
                assert table_rows(got)[0] == (None, False) * 4 + (0, None)


# --------------------------------------------------------------------------- every accepted value type, bit for bit

def typed_table(n, ngroups, seed):
    rng = np.random.default_rng(seed)
    f64 = rng.standard_normal(n)
    f64[rng.integers(0, n, n // 8)] = -0.0
    f64[rng.integers(0, n, n // 8)] = np.inf
    f64[rng.integers(0, n, n // 8)] = -np.inf
    nan_payloads = (np.uint64(0x7ff8000000000000) | rng.integers(1, 1 << 40, n // 6).astype(np.uint64)).view(np.float64)
    f64[rng.integers(0, n, n // 6)] = nan_payloads
    f64[rng.integers(0, n, n // 10)] = np.array([0xfff0000000000001], np.uint64).view(np.float64)[0]      # a negative signalling NaN
    f32 = rng.standard_normal(n).astype(np.float32)
    f32[rng.integers(0, n, n // 8)] = np.float32(-0.0)
    f32[rng.integers(0, n, n // 8)] = (np.uint32(0x7fc00000) | rng.integers(1, 1 << 20, n // 8).astype(np.uint32)).view(np.float32)
    big = [decimal.Decimal(int(v) * (10**19 + 7) * (-1 if i % 3 == 0 else 1)).scaleb(-4) for i, v in enumerate(rng.integers(1, 2**62, n))]      # beyond 64 bits
    mask = lambda: rng.random(n) < 0.3
    cols = {
        "g": pa.array(rng.integers(0, ngroups, n).astype(np.int32)),
        "b": pa.array(rng.random(n) < 0.5, pa.bool_(), mask=mask()),
        "i8": pa.array(rng.integers(-128, 128, n).astype(np.int8), mask=mask()),
        "i16": pa.array(rng.integers(-2**15, 2**15, n).astype(np.int16), mask=mask()),
        "i32": pa.array(rng.integers(-2**31, 2**31, n).astype(np.int32), mask=mask()),
        "i64": pa.array(rng.integers(-2**63, 2**63 - 1, n), mask=mask()),
        "f32": pa.array(f32, mask=mask()),
        "f64": pa.array(f64, mask=mask()),
        "d": pa.array(rng.integers(-10_000, 10_000, n).astype(np.int32), mask=mask()).cast(pa.date32()),
        "ts": pa.array(rng.integers(-2**50, 2**50, n), mask=mask()).cast(pa.timestamp("us", tz="UTC")),
        "tsn": pa.array(rng.integers(-2**50, 2**50, n), mask=mask()).cast(pa.timestamp("us")),
        "dec12": pa.array([decimal.Decimal(int(v)).scaleb(-2) for v in rng.integers(-10**11, 10**11, n)], pa.decimal128(12, 2), mask=mask()),
        "dec38": pa.array(big, pa.decimal128(38, 4), mask=mask()),
    }
    return pa.table(cols)


@pytest.mark.parametrize("grouped", [False, True])
def test_every_value_type(built, grouped):
    t = typed_table(3000, 7, 11)
    # the float columns hold what the test means them to hold
    f = values(t.column("f64"))
    assert any(v is not None and (v & 0x7ff0000000000000) == 0x7ff0000000000000 and (v & 0xfffffffffffff) not in (0, 1 << 51) for v in f)      # NaN with a payload
    assert any(v == -(1 << 63) for v in f) and any(v == 0x7ff0000000000000 for v in f)                                                        # -0.0, +inf
    assert any(d is not None and abs(int(d.scaleb(4))) >= 2**64 for d in t.column("dec38").to_pylist())
    cols = list(range(1, t.num_columns))
    for chunk in (cols[:5], cols[5:9], cols[9:]):      # at most 22 output columns per pipeline
        specs = []
        for c in chunk:
            specs += [("first", c, c % 2 == 0, None), ("last", c, c % 2 == 1, None)]
        check(t, 0 if grouped else None, specs, label=str(chunk))


# --------------------------------------------------------------------------- each table path of the grouped aggregate

def big_table(n, ngroups, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, max(ngroups, 1), n).astype(np.int32)
    x = rng.integers(-2**62, 2**62, n)
    return pa.table({"g": pa.array(g), "x": pa.array(x, mask=rng.random(n) < 0.2), "s": pa.array(rng.integers(-2**15, 2**15, n).astype(np.int16), mask=rng.random(n) < 0.2)})


PATH_SPECS = [("first", 1, False, None), ("last", 1, True, None), ("first", 2, True, None), ("bit_and", 2, False, None), ("bit_or", 1, False, None), ("bit_xor", 1, False, None),
              ("count", 1, False, None)]


@pytest.mark.parametrize("ngroups", [0, 5, 40_000])
def test_table_paths(built, ngroups):
    """ungrouped (registers); five groups (private LDS copies and the LDS table); 40 000 groups (more than the LDS table holds: the global table) — 1 M rows in several chunks"""
    t = big_table(1_000_000, ngroups, 21)
    check(t, 0 if ngroups else None, PATH_SPECS, config={"spark.comet.gpu.chunkRows": 300_000})


def test_global_table_that_fills_up_mid_chunk(built):
    """600 K distinct groups arriving in chunks of 70 K rows: the global table starts at 2^17 slots, more than half full after the first chunk and short of slots in the
    second — the pass over that chunk is voided, the table grows and the chunk runs again; first / last take their values only behind the pass that survives.
    (No metric reports a voided pass: the shape is built to reach it — 130 K groups into 2^17 slots with at most 128 probes — rather than asserted to.)"""
    n = 1_000_000
    rng = np.random.default_rng(22)
    g = (rng.integers(0, 600_000, n) * 7919).astype(np.int32)
    t = pa.table({"g": pa.array(g), "x": pa.array(np.arange(n, dtype=np.int64) * 3 - 5, mask=rng.random(n) < 0.2)})
    check(t, 0, [("first", 1, False, None), ("last", 1, True, None), ("bit_xor", 1, False, None)], config={"spark.comet.gpu.chunkRows": 70_000})


def _states_of(table, key_col, specs, slices):
    """Partial over each slice of the rows (the model's states, in slice order), concatenated: the input of a Final / PartialMerge aggregate"""
    rows = table_rows(table)
    bounds = [len(rows) * i // slices for i in range(slices + 1)]
    out = []
    for a, b in zip(bounds, bounds[1:]):
        for k, st in model(rows[a:b], key_col, specs).items():
            out.append(((k,) if key_col is not None else ()) + st)
    return out


def _state_table(table, key_col, specs, state_rows):
    fields = ([table.schema.field(key_col).type] if key_col is not None else [])
    for kind, c, _, _ in specs:
        vt = table.schema.field(c).type
        fields += [vt, pa.bool_()] if kind in ("first", "last") else [pa.int64() if kind in ("count", "sum") else vt]
    cols = list(zip(*state_rows)) if state_rows else [[] for _ in fields]
    return pa.table([pa.array(list(c), ft) for c, ft in zip(cols, fields)], names=[f"s{i}" for i in range(len(fields))])


MERGE_SPECS = [("first", 1, False, None), ("last", 1, True, None), ("first", 1, True, None), ("bit_and", 2, False, None), ("bit_xor", 1, False, None)]


def stack(tables):
    """the tables' rows one behind the other (column by column: the field names and nullability flags of engine outputs are not the point here)"""
    n = tables[0].num_columns
    return pa.table([pa.concat_arrays([c for t in tables for c in t.column(i).chunks]) for i in range(n)], names=[f"s{i}" for i in range(n)])


def _final_plan(table, key_col, specs, states, mode):
    types = [S.from_arrow_type(f.type) for f in table.schema]
    stypes = [S.from_arrow_type(f.type) for f in states.schema]
    keys = [] if key_col is None else [S.col(0, stypes[0])]
    return S.hash_agg(S.scan(stypes), keys, [agg_of(sp, types) for sp in specs], mode)


def test_partitioned_merge(built):
    """a Final aggregate whose whole input is ONE device-resident chunk of about one state row per group: partition → LDS merge → emit (no table in HBM); the winning state
    row's value is picked inside the merge kernel"""
    t = big_table(120_000, 40_000, 23)
    states = _state_table(t, 0, MERGE_SPECS, _states_of(t, 0, MERGE_SPECS, 3))
    assert states.num_rows > 36_000
    plan = _final_plan(t, 0, MERGE_SPECS, states, S.FINAL)
    got, m = run_metrics(plan, [native.DeviceInput(native.DeviceTable.from_arrow(states, "cuda:0"))], ncols_of(0, MERGE_SPECS, True))
    assert m["agg_partitioned_merges"] == 1, m
    want = model(table_rows(t), 0, MERGE_SPECS, final=True)
    g = by_key(got)
    assert len(g) == len(want) == got.num_rows
    bad = [(k, g[k], want[k]) for k in want if g[k] != want[k]]
    assert not bad, (len(bad), bad[:5])
    # host batches of the same states keep the global-table path: the same answer
    got2, m2 = run_metrics(plan, [native.HostInput.from_table(states)], ncols_of(0, MERGE_SPECS, True))
    assert m2["agg_partitioned_merges"] == 0 and by_key(got2) == g


def test_partial_over_a_joins_output_runs_partitioned(built):
    """a Partial aggregate over ONE modest chunk — a join's output — with many groups takes the partitioned path too; first / last then read the join's output rows"""
    n = 200_000
    rng = np.random.default_rng(24)
    k = rng.integers(0, 60_000, n).astype(np.int64) * 104_729
    table = pa.table({"k": pa.array(k), "x": pa.array(rng.integers(-2**40, 2**40, n), mask=rng.random(n) < 0.2), "j": pa.array(np.zeros(n, np.int32))})
    dim = pa.table({"j": pa.array(np.zeros(1, np.int32)), "w": pa.array(np.ones(1, np.int64))})
    join = S.hash_join(S.scan([I64, I64, I32]), S.scan([I32, I64]), [S.col(2, I32)], [S.col(0, I32)], S.INNER, S.BUILD_RIGHT)
    specs = [("first", 1, True, None), ("last", 1, False, None), ("bit_or", 1, False, None), ("count", 1, False, None)]
    plan = plan_of([I64, I64, I32, I32, I64], 0, specs, source=join)
    got, m = run_metrics(plan, [native.HostInput.from_table(table), native.HostInput.from_table(dim)], ncols_of(0, specs))
    assert m["agg_partitioned_merges"] == 1, m
    # a join's output order is unspecified, and it is that order first / last see: the order-free columns are exact, first / last must name a value of their group
    want = model(table_rows(table), 0, specs)
    g = by_key(got)
    assert len(g) == len(want)
    rows_of_group = {}
    for r in table_rows(table):
        rows_of_group.setdefault(r[0], []).append(r[1])
    for key, st in want.items():
        assert g[key][4:] == st[4:], (key, g[key], st)
        assert g[key][1] == st[1] and g[key][3] == st[3]
        assert (g[key][0] in rows_of_group[key]) if st[1] else g[key][0] is None
        assert g[key][2] in rows_of_group[key]


# --------------------------------------------------------------------------- the order of the rows is all that matters

def test_same_bits_for_any_batching_and_chunking(built):
    t = big_table(200_000, 1000, 31)
    specs = [("first", 1, False, None), ("last", 1, False, None), ("first", 1, True, None), ("last", 2, True, None), ("bit_xor", 1, False, None)]
    for key_col in (0, None):
        types = [S.from_arrow_type(f.type) for f in t.schema]
        plan, nc = plan_of(types, key_col, specs), ncols_of(key_col, specs)
        want = model(table_rows(t), key_col, specs)
        outs = []
        for batch_rows, cfg in ((1000, None), (8192, None), (t.num_rows, None), (8192, {"spark.comet.gpu.chunkRows": 8192}), (5000, {"spark.comet.gpu.chunkRows": 50_000})):
            got = run(plan, t, nc, batch_rows, cfg)
            outs.append(by_key(got) if key_col is not None else {(): table_rows(got)[0]})
        assert all(o == want for o in outs), [i for i, o in enumerate(outs) if o != want]
        # reversing the rows swaps first and last
        rev = t.take(pa.array(np.arange(t.num_rows - 1, -1, -1)))
        sw = [("last" if k == "first" else "first" if k == "last" else k, c, ig, f) for k, c, ig, f in specs]
        got = run(plan_of(types, key_col, sw), rev, nc)
        assert (by_key(got) if key_col is not None else {(): table_rows(got)[0]}) == want


# --------------------------------------------------------------------------- FILTER (WHERE …) and a Filter in front

def test_filters(built):
    t = big_table(100_000, 300, 41)
    types = [S.from_arrow_type(f.type) for f in t.schema]
    pos = S.gt(S.col(1, I64), S.lit(0, I64))          # x > 0: NULL x fails it
    f_pos = lambda r: r[1] is not None and r[1] > 0
    f_s = lambda r: r[2] is not None and r[2] > 100
    s_gt = S.gt(S.col(2, S.T_INT16), S.lit(100, S.T_INT16))
    specs = [("first", 1, False, f_pos, pos), ("last", 1, True, f_s, s_gt), ("first", 2, False, f_pos, pos), ("last", 2, False, None), ("bit_xor", 1, False, f_s, s_gt),
             ("bit_or", 2, False, f_pos, pos)]
    for key_col in (0, None):
        check(t, key_col, specs, label=f"agg filter key={key_col}")
        # Filter(s IS NOT NULL AND x < 2^61) in front of the aggregate: the rows that reach it keep their order
        chain = S.filter_(S.scan(types), S.and_(S.is_not_null(S.col(2, S.T_INT16)), S.lt(S.col(1, I64), S.lit(2**61, I64))))
        keep = [r for r in table_rows(t) if r[2] is not None and r[1] is not None and r[1] < 2**61]
        got = run(plan_of(types, key_col, specs, source=chain), t, ncols_of(key_col, specs))
        want = model(keep, key_col, [sp[:4] for sp in specs])
        assert (by_key(got) if key_col is not None else {(): table_rows(got)[0]}) == want


# --------------------------------------------------------------------------- two stages

@pytest.mark.parametrize("grouped", [False, True])
def test_partial_final_and_partial_merge(built, grouped):
    t = big_table(60_000, 500, 51)
    # group 7 has only NULLs in the first third of the rows (is_set = false under ignore_nulls there), values later
    g, x = t.column("g").to_numpy(), np.array(t.column("x").to_pylist(), dtype=object)
    x[(g == 7) & (np.arange(len(g)) < 20_000)] = None
    t = t.set_column(1, "x", pa.array(list(x), pa.int64()))
    key_col = 0 if grouped else None
    types = [S.from_arrow_type(f.type) for f in t.schema]
    rows = table_rows(t)
    one_stage = model(rows, key_col, MERGE_SPECS, final=True)
    # the engine's own Partial over three slices, concatenated in slice order
    parts = []
    for i in range(3):
        sl = t.slice(20_000 * i, 20_000)
        got = run(plan_of(types, key_col, MERGE_SPECS), sl, ncols_of(key_col, MERGE_SPECS))
        want = model(table_rows(sl), key_col, MERGE_SPECS)
        assert (by_key(got) if grouped else {(): table_rows(got)[0]}) == want, i
        parts.append(got)
    if grouped:
        first_slice = by_key(parts[0])
        assert first_slice[7][:6] == (None, True, None, False, None, False)      # first: a NULL row; last(ignore_nulls) and first(ignore_nulls): nothing seen yet
    states = stack(parts)
    fplan = _final_plan(t, key_col, MERGE_SPECS, states, S.FINAL)
    nf = ncols_of(key_col, MERGE_SPECS, True)
    got = run(fplan, states, nf, batch_rows=97)
    assert (by_key(got) if grouped else {(): table_rows(got)[0]}) == one_stage
    # PartialMerge over the first two slices' states, then Final over (merged, third)
    two = stack(parts[:2])
    merged = run(_final_plan(t, key_col, MERGE_SPECS, two, S.PARTIAL_MERGE), two, ncols_of(key_col, MERGE_SPECS))
    assert (by_key(merged) if grouped else {(): table_rows(merged)[0]}) == model(rows[:40_000], key_col, MERGE_SPECS)
    rest = stack([merged, parts[2]])
    got = run(fplan, rest, nf)
    assert (by_key(got) if grouped else {(): table_rows(got)[0]}) == one_stage
    # the states in the other order give the other answer for first / last (it is the state-row order that counts)
    back = stack(parts[::-1])
    got = run(fplan, back, nf)
    sw = model(rows[40_000:] + rows[20_000:40_000] + rows[:20_000], key_col, MERGE_SPECS, final=True)
    assert (by_key(got) if grouped else {(): table_rows(got)[0]}) == sw


# --------------------------------------------------------------------------- the bit aggregates' corners

@pytest.mark.parametrize("grouped", [False, True])
def test_bit_aggregate_corners(built, grouped):
    rows = [(1, -1, 6), (1, 0x55, 6),                 # bit_and(-1, 0x55) = 0x55: the sign extension of -1 must not leak, the result is an Int8
            (2, 9, 5), (2, 9, 5), (2, 9, 5), (2, 9, 5),      # an even number of equal values: bit_xor = 0, not NULL
            (3, None, None),                          # no contributing row: NULL
            (4, -128, -2**63), (4, 127, 2**63 - 1)]   # the extremes
    t = pa.table({"g": pa.array([r[0] for r in rows], pa.int32()), "b": pa.array([r[1] for r in rows], pa.int8()), "x": pa.array([r[2] for r in rows], pa.int64())})
    specs = [(k, c, False, None) for k in ("bit_and", "bit_or", "bit_xor") for c in (1, 2)]
    got = check(t, 0 if grouped else None, specs)
    if grouped:
        g = by_key(got)
        assert g[1] == (0x55, 6, -1, 6, -0x56, 0)
        assert g[2] == (9, 5, 9, 5, 0, 0)
        assert g[3] == (None,) * 6
        assert g[4] == (0, 0, -1, -1, -1, -1)
        assert got.schema.field(1).type == pa.int8() and got.schema.field(2).type == pa.int64()
    # merging states is the same operation
    states = pa.table({"g": pa.array([1, 1, 2, 2, 3], pa.int32()), "b": pa.array([0x0f, None, 0x33, 0x35, None], pa.int8())})
    for kind, want in (("bit_and", {1: 0x0f, 2: 0x31, 3: None}), ("bit_or", {1: 0x0f, 2: 0x37, 3: None}), ("bit_xor", {1: 0x0f, 2: 0x06, 3: None})):
        agg = agg_of((kind, 1, False, None), [I32, I8])
        for mode in (S.FINAL, S.PARTIAL_MERGE):
            if grouped:
                got = run(S.hash_agg(S.scan([I32, I8]), [S.col(0, I32)], [agg], mode), states, 2)
                assert {k: v[0] for k, v in by_key(got).items()} == want, (kind, mode)
            else:
                got = run(S.hash_agg(S.scan([I8]), [], [agg], mode), states.select(["b"]).slice(2, 2), 1)
                assert table_rows(got)[0] == (want[2],), (kind, mode)
