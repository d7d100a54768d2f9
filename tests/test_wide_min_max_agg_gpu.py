"""min / max of a decimal wider than 18 digits in a GROUPED HashAggregate on the GPU.

A Decimal128(p > 18, s) value v does not fit one 64-bit word and no memory has a 128-bit atomic, so a group keeps v as (hi = v >> 64 signed, lo = v mod 2^64 unsigned):
the k_gagg pass settles the extreme hi, a per-slot step and a second pass over the chunk's rows settle the extreme lo among the rows that hold that hi
(comet_device.hpp "wide min / max").  The result must be the exact 128-bit extreme, NULL for a group without a non-NULL value, and the same bits for every batch size,
chunk size, grid and table path (private LDS copies, LDS table, global table, a table that grows or fills up mid-chunk).
The referee is a dict walk over python ints (the unscaled values).  Columns are built from 16-byte numpy buffers, and read back the same way.
"""
import random

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S

pytestmark = pytest.mark.gpu
I32, I64, F64, B = S.T_INT32, S.T_INT64, S.T_DOUBLE, S.T_BOOL
M64 = (1 << 64) - 1


# --------------------------------------------------------------------------- helpers

def split(vals):
    """python ints (None = NULL) → (hi: int64, lo: uint64, mask: True where NULL)"""
    hi = np.array([0 if v is None else v >> 64 for v in vals], dtype=np.int64)
    lo = np.array([0 if v is None else v & M64 for v in vals], dtype=np.uint64)
    return hi, lo, np.array([v is None for v in vals], dtype=bool)


def wide_array(hi, lo, p, s, mask=None):
    """a Decimal128(p, s) column from its words, without a python object per row"""
    n = len(hi)
    words = np.empty((n, 2), dtype=np.uint64)
    words[:, 0] = lo
    words[:, 1] = np.asarray(hi, dtype=np.int64).view(np.uint64)
    validity = None
    if mask is not None and mask.any():
        validity = pa.array(~mask).buffers()[1]
    return pa.Array.from_buffers(pa.decimal128(p, s), n, [validity, pa.py_buffer(words.tobytes())])


def ints_of(hi, lo, mask=None):
    """the unscaled values as python ints (None = NULL)"""
    v = [(int(h) << 64) + int(l) for h, l in zip(hi.tolist(), lo.tolist())]
    if mask is not None:
        v = [None if m else x for x, m in zip(v, mask.tolist())]
    return v


def dec_of(vals, p, s):
    hi, lo, mask = split(vals)
    return wide_array(hi, lo, p, s, mask)


def unscaled(col):
    """a decimal column's unscaled values as python ints (None = NULL), read from its buffers"""
    a = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    assert pa.types.is_decimal128(a.type), a.type
    w = np.frombuffer(a.buffers()[1], dtype=np.uint64)[2 * a.offset:2 * (a.offset + len(a))].reshape(-1, 2)
    ok = a.is_valid().to_pylist()
    hi = w[:, 1].copy().view(np.int64).tolist()
    lo = w[:, 0].tolist()
    return [(hi[i] << 64) + lo[i] if ok[i] else None for i in range(len(a))]


def column_values(col):
    a = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    return unscaled(a) if pa.types.is_decimal128(a.type) else a.to_pylist()


def by_key(t):
    if t is None:
        return {}
    cols = [column_values(t.column(i)) for i in range(t.num_columns)]
    return {r[0]: r[1:] for r in zip(*cols)}


def run(plan, table, ncols, batch_rows=8192, config=None):
    kw = {"config": S.config_map(config)} if config else {}
    out = native.execute_to_table([native.HostInput.from_table(table, batch_rows)], ncols, plan.encode(), batch_size=0, **kw)
    return pa.Table.from_batches(out) if out else None


def run_metrics(plan, inputs, ncols, config=None):
    kw = {"config": S.config_map(config)} if config else {}
    it = native.CometExecIterator(inputs, ncols, plan.encode(), batch_size=0, **kw)
    batches = []
    while True:
        b = native.Native.executePlan(it.handle, ncols)
        if b is None:
            break
        batches.append(b)
    m = S.decode_metric_node(it.metrics())[0]
    it.close()
    return (pa.Table.from_batches(batches) if batches else None), m


def model(keys, vals, kind):
    """{key: min / max of the group's non-NULL values, None if there is none}"""
    out = {}
    better = (lambda a, b: a < b) if kind == "min" else (lambda a, b: a > b)
    for k, v in zip(keys, vals):
        cur = out.setdefault(k, None)
        if v is not None and (cur is None or better(v, cur)):
            out[k] = v
    return out


def mk(kind, e, t, flt=None):
    a = S.min_(e, t) if kind == "min" else S.max_(e, t)
    if flt is not None:
        a.filter = flt
    return a


def assert_groups(got, want, label=""):
    """want: {key: tuple of columns}; every group of the run is compared"""
    g = by_key(got)
    assert len(g) == len(want) == (got.num_rows if got is not None else 0), (label, len(g), len(want))
    bad = [(k, g[k], want[k]) for k in want if g[k] != want[k]]
    assert not bad, (label, len(bad), bad[:5])


def min_max_plan(D, mode=S.PARTIAL, source=None, grouped=True):
    """key (col 0), then max(col 1), min(col 1)"""
    src = source if source is not None else S.scan([I32, D])
    return S.hash_agg(src, [S.col(0, I32)] if grouped else [], [mk("max", S.col(1, D), D), mk("min", S.col(1, D), D)], mode)


def want_min_max(keys, vals):
    mx, mn = model(keys, vals, "max"), model(keys, vals, "min")
    return {k: (mx[k], mn[k]) for k in mx}


# --------------------------------------------------------------------------- 1. corners

def corner_rows(p):
    top = 10**p - 1
    two64 = 1 << 64
    hi_pairs = p >= 21      # (hi = 3 / 4 needs more than 20 digits)
    rows = [
        (1, top), (1, -top), (1, 0), (1, None),
        (2, (3 << 64) + M64 if hi_pairs else two64 + M64), (2, (4 << 64) if hi_pairs else 2 * two64), (2, -1), (2, -two64), (2, -two64 - 1), (2, 0),
        (3, (1 << 64) + (1 << 63) - 1), (3, (1 << 64) + (1 << 63)), (3, (1 << 63) - 1), (3, 1 << 63), (3, None),
        (4, None), (4, None),                     # an all-NULL group
        (5, -two64 - 1),                          # a group of one row
        (6, -((1 << 64) + (1 << 63))), (6, -((1 << 64) + (1 << 63) - 1)), (6, -((2 << 64) + 5)), (6, -(2 << 64)),      # negative: the smaller hi with the larger lo
    ]
    return [(k, v) for k, v in rows if v is None or abs(v) <= top]


@pytest.mark.parametrize("p,s", [(38, 4), (19, 0)])
@pytest.mark.parametrize("with_validity", [True, False])
def test_corners(built, p, s, with_validity):
    D = S.decimal(p, s)
    rows = [(k, v) for k, v in corner_rows(p) if with_validity or v is not None]
    assert any(v is not None and (v & M64) >> 63 for _, v in rows) and any(v is not None and v < 0 for _, v in rows)
    assert p < 21 or any(v is not None and v < -(1 << 64) for _, v in rows)
    keys, vals = [k for k, _ in rows], [v for _, v in rows]
    t = pa.table({"g": pa.array(keys, pa.int32()), "d": dec_of(vals, p, s)})
    got = run(min_max_plan(D), t, 3)
    assert got.schema.field(1).type == pa.decimal128(p, s) and got.schema.field(2).type == pa.decimal128(p, s)
    assert_groups(got, want_min_max(keys, vals), "plain")
    g = by_key(got)
    if with_validity:
        assert g[4] == (None, None)
    if p >= 21:
        assert g[5] == (-(1 << 64) - 1, -(1 << 64) - 1)
    # an aggregate FILTER (d < 2^64, or 2^63 where the type ends below 2^64: drops the maxima of groups 1 to 3) …
    lim = 1 << (64 if p >= 21 else 63)
    flt = S.lt(S.col(1, D), S.lit(lim, D))
    plan = S.hash_agg(S.scan([I32, D]), [S.col(0, I32)], [mk("max", S.col(1, D), D, flt), mk("min", S.col(1, D), D)])
    fv = [v if v is not None and v < lim else None for v in vals]
    mx, mn = model(keys, fv, "max"), model(keys, vals, "min")
    assert_groups(run(plan, t, 3), {k: (mx[k], mn[k]) for k in mx}, "agg filter")
    # … and a Filter in front that drops the would-be extremes on both sides (and the NULLs: a comparison with NULL is not TRUE)
    low = -lim - 1
    chain = S.filter_(S.scan([I32, D]), S.and_(S.lt(S.col(1, D), S.lit(lim, D)), S.gt(S.col(1, D), S.lit(low, D))))
    keep = [(k, v) for k, v in rows if v is not None and low < v < lim]
    assert_groups(run(min_max_plan(D, source=chain), t, 3), want_min_max([k for k, _ in keep], [v for _, v in keep]), "chain filter")


# --------------------------------------------------------------------------- 2. every mode

def spread_table(n, ngroups, seed, p=38, s=4, null_rate=0.2):
    """about half the groups hold one hi for all their rows, the others' hi spread over ±3; lo covers all 64 bits"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, max(ngroups, 1), n).astype(np.int32)
    hi = np.where(g % 2 == 0, (g % 7).astype(np.int64) - 3, rng.integers(-3, 4, n))
    lo = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    mask = rng.random(n) < null_rate
    return pa.table({"g": pa.array(g), "d": wide_array(hi, lo, p, s, mask)}), g.tolist(), ints_of(hi, lo, mask)


def stack(tables):
    n = tables[0].num_columns
    return pa.table([pa.concat_arrays([c for t in tables for c in t.column(i).chunks]) for i in range(n)], names=[f"s{i}" for i in range(n)])


def test_every_mode(built):
    p, s = 38, 4
    D = S.decimal(p, s)
    t, keys, vals = spread_table(3000, 40, 2)
    one_stage = want_min_max(keys, vals)
    parts = []
    for i in range(3):
        sl = t.slice(1000 * i, 1000)
        got = run(min_max_plan(D), sl, 3)
        assert_groups(got, want_min_max(keys[1000 * i:1000 * (i + 1)], vals[1000 * i:1000 * (i + 1)]), f"partial {i}")
        assert [f.type for f in got.schema][1:] == [pa.decimal128(p, s)] * 2
        parts.append(got)
    states = stack(parts)
    fplan = S.hash_agg(S.scan([I32, D, D]), [S.col(0, I32)], [mk("max", S.col(1, D), D), mk("min", S.col(2, D), D)], S.FINAL)
    got = run(fplan, states, 3, batch_rows=97)
    assert_groups(got, one_stage, "final")
    assert [f.type for f in got.schema][1:] == [pa.decimal128(p, s)] * 2
    two = stack(parts[:2])
    mplan = S.hash_agg(S.scan([I32, D, D]), [S.col(0, I32)], [mk("max", S.col(1, D), D), mk("min", S.col(2, D), D)], S.PARTIAL_MERGE)
    merged = run(mplan, two, 3)
    assert_groups(merged, want_min_max(keys[:2000], vals[:2000]), "partial merge")
    assert [f.type for f in merged.schema][1:] == [pa.decimal128(p, s)] * 2
    assert_groups(run(fplan, stack([merged, parts[2]]), 3), one_stage, "final over (merged, third)")
    # mixed modes: max merges the first slices' states (column 2) while min starts over the third slice's values (column 1)
    third = t.slice(2000, 1000)
    m_keys = by_key(merged)
    child = pa.table({"g": third.column("g"), "d": third.column("d"),
                      "st": dec_of([m_keys.get(k, (None, None))[0] for k in keys[2000:]], p, s)})
    xplan = S.hash_agg(S.scan([I32, D, D]), [S.col(0, I32)], [mk("max", S.col(2, D), D), mk("min", S.col(1, D), D)], S.PARTIAL,
                       expr_modes=[S.PARTIAL_MERGE, S.PARTIAL], initial_input_buffer_offset=2)
    got = run(xplan, child, 3)
    mx = model(keys[2000:], [m_keys.get(k, (None, None))[0] for k in keys[2000:]], "max")
    mn = model(keys[2000:], vals[2000:], "min")
    assert_groups(got, {k: (mx[k], mn[k]) for k in mx}, "mixed modes")
    assert [f.type for f in got.schema][1:] == [pa.decimal128(p, s)] * 2


# --------------------------------------------------------------------------- 3. each table path

@pytest.mark.parametrize("ngroups", [0, 5, 40_000])
def test_table_paths(built, ngroups):
    """ungrouped (registers; unchanged); five groups (private LDS copies and the LDS table); 40 000 groups (the global table) — 1 M rows in several chunks"""
    D = S.decimal(38, 4)
    t, keys, vals = spread_table(1_000_000, ngroups, 3)
    cfg = {"spark.comet.gpu.chunkRows": 300_000}
    if ngroups == 0:
        got = run(min_max_plan(D, grouped=False), t, 2, config=cfg)
        nn = [v for v in vals if v is not None]
        assert got.num_rows == 1 and (unscaled(got.column(0))[0], unscaled(got.column(1))[0]) == (max(nn), min(nn))
        return
    got, m = run_metrics(min_max_plan(D), [native.HostInput.from_table(t, 8192)], 3, config=cfg)
    assert m["agg_wide_min_max_passes"] >= 1, m
    assert_groups(got, want_min_max(keys, vals))


# --------------------------------------------------------------------------- 4. H moves between chunks

def test_high_word_moves_between_chunks(built):
    """30 000 rows in chunks of 8192, 50 groups.  Group g % 3 == 0: the extreme hi first appears in the LAST chunk, with a worse lo than earlier chunks offered under the old
    hi.  g % 3 == 1: the extreme hi is in the FIRST chunk, later chunks hold better lo under a worse hi.  g % 3 == 2: hi is constant, the best lo is in the MIDDLE chunk."""
    n, chunk, ng = 30_000, 8192, 50
    D = S.decimal(38, 4)
    keys = [i % ng for i in range(n)]
    last0, mid0, mid1 = (n // chunk) * chunk, chunk, 2 * chunk
    vals_max, vals_min = [], []
    for i, g in enumerate(keys):
        kind = g % 3
        j = i // ng                        # the row's rank within its group
        if kind == 0:
            late = i >= last0
            hi = 7 if late else 2
            lo = (1000 + j) if late else (M64 - j)               # under the old hi the lo was nearly 2^64; under the new one it is small
        elif kind == 1:
            early = i < chunk
            hi = 7 if early else 2
            lo = (5000 + j) if early else (M64 - j)
        else:
            hi = 4
            lo = (1 << 63) + 10**6 + j if mid0 <= i < mid1 else (1 << 63) - 1 - j     # the best lo has its top bit set and sits in the middle chunk
        vals_max.append((hi << 64) + lo)
        vals_min.append(-((hi << 64) + lo))                   # the mirror image for min: hi = -hi - 1, lo = 2^64 - lo
    t = pa.table({"g": pa.array(keys, pa.int32()), "a": dec_of(vals_max, 38, 4), "b": dec_of(vals_min, 38, 4)})
    plan = S.hash_agg(S.scan([I32, D, D]), [S.col(0, I32)], [mk("max", S.col(1, D), D), mk("min", S.col(2, D), D), mk("min", S.col(1, D), D), mk("max", S.col(2, D), D)])
    got, m = run_metrics(plan, [native.HostInput.from_table(t, 8192)], 5, config={"spark.comet.gpu.chunkRows": chunk})
    assert m["agg_wide_min_max_passes"] >= 2, m      # (one per chunk)
    w = [model(keys, v, k) for v, k in ((vals_max, "max"), (vals_min, "min"), (vals_max, "min"), (vals_min, "max"))]
    assert_groups(got, {k: tuple(x[k] for x in w) for k in w[0]})
    g = by_key(got)
    assert g[0][0] >> 64 == 7 and g[0][0] & M64 < 1 << 20 and g[1][0] >> 64 == 7 and g[2][0] & M64 >= 1 << 63


# --------------------------------------------------------------------------- 5. a voided pass

def test_global_table_that_fills_up_mid_chunk(built):
    """600 K distinct groups arriving in chunks of 70 K rows: the global table starts at 2^17 slots, is more than half full after the first chunk and short of slots in the
    second — the pass over that chunk is voided, the table grows and the chunk runs again; the per-slot step and the low-word pass run only behind the pass that survives,
    on the table that replaced the old one.  (No metric reports a voided pass: the shape is built to reach it, as in tests/test_first_last_bit_agg_gpu.py.)"""
    n = 1_000_000
    rng = np.random.default_rng(5)
    g = (rng.integers(0, 600_000, n) * 7919).astype(np.int32)
    hi = rng.integers(-2, 3, n)
    lo = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    mask = rng.random(n) < 0.2
    t = pa.table({"g": pa.array(g), "d": wide_array(hi, lo, 38, 4, mask)})
    got = run(min_max_plan(S.decimal(38, 4)), t, 3, config={"spark.comet.gpu.chunkRows": 70_000})
    assert_groups(got, want_min_max(g.tolist(), ints_of(hi, lo, mask)))


# --------------------------------------------------------------------------- 6. the partitioned merge

def test_partitioned_merge(built):
    """a Final aggregate whose whole input is ONE device-resident chunk of about 40 000 groups × 3 state rows: partition → LDS merge → emit (no table in HBM).  A record
    carries (hi, lo) of its state row; the merge kernel settles the high word per LDS slot, resets the low words and sweeps the partition's records a second time.  Host
    batches of the same states keep the global-table path: the same table."""
    p, s = 38, 4
    D = S.decimal(p, s)
    t, keys, vals = spread_table(120_000, 40_000, 6)
    srows = []
    for i in range(3):
        a, b = 40_000 * i, 40_000 * (i + 1)
        for k, st in want_min_max(keys[a:b], vals[a:b]).items():
            srows.append((k,) + st)
    assert len(srows) > 36_000 * 2
    states = pa.table({"g": pa.array([r[0] for r in srows], pa.int32()), "mx": dec_of([r[1] for r in srows], p, s), "mn": dec_of([r[2] for r in srows], p, s)})
    plan = S.hash_agg(S.scan([I32, D, D]), [S.col(0, I32)], [mk("max", S.col(1, D), D), mk("min", S.col(2, D), D)], S.FINAL)
    got, m = run_metrics(plan, [native.DeviceInput(native.DeviceTable.from_arrow(states, "cuda:0"))], 3)
    assert m["agg_partitioned_merges"] == 1, m
    assert m["agg_wide_min_max_passes"] >= 1, m
    want = want_min_max(keys, vals)
    assert_groups(got, want)
    got2, m2 = run_metrics(plan, [native.HostInput.from_table(states)], 3)
    assert m2["agg_partitioned_merges"] == 0 and m2["agg_wide_min_max_passes"] >= 1 and by_key(got2) == by_key(got)


# --------------------------------------------------------------------------- 7. beside every other aggregate

def test_mixed_aggregates(built):
    """one grouped HashAggregate: wide max, wide min of another column, sum and avg of the wide decimal, count, min of an Int64, max of a Float64, first(x), last(x
    ignore nulls) — k_gpick and the low-word pass behind the same k_gagg pass.  Host batches in order: first / last are the first / last row in row order."""
    n, ng = 100_000, 700
    rng = np.random.default_rng(7)
    D, D2, DS, DA = S.decimal(28, 4), S.decimal(38, 4), S.decimal(38, 4), S.decimal(32, 8)
    g = rng.integers(0, ng, n).astype(np.int32)
    top = 10**28 - 1
    r = random.Random(7)
    a_vals = [None if r.random() < 0.2 else r.randint(-top, top) for _ in range(n)]
    hi2, lo2, mask2 = rng.integers(-3, 4, n), rng.integers(0, 1 << 64, n, dtype=np.uint64), rng.random(n) < 0.2
    x = rng.integers(-2**62, 2**62, n)
    xmask = rng.random(n) < 0.2
    f = rng.standard_normal(n)
    fmask = rng.random(n) < 0.2
    t = pa.table({"g": pa.array(g), "a": dec_of(a_vals, 28, 4), "b": wide_array(hi2, lo2, 38, 4, mask2), "x": pa.array(x, mask=xmask), "f": pa.array(f, mask=fmask)})
    c = lambda i, ty: S.col(i, ty)
    aggs = [mk("max", c(1, D), D), mk("min", c(2, D2), D2), S.sum_(c(1, D), DS), S.avg(c(1, D), DA, DS), S.count(c(1, D)), mk("min", c(3, I64), I64), mk("max", c(4, F64), F64),
            S.first_(c(3, I64), I64), S.last_(c(3, I64), I64, True)]
    plan = S.hash_agg(S.scan([I32, D, D2, I64, F64]), [c(0, I32)], aggs)
    # state columns: max, min, (sum, is_empty), (sum, count), count, min, max, (first, is_set), (last, is_set)
    got, m = run_metrics(plan, [native.HostInput.from_table(t, 8192)], 14, config={"spark.comet.gpu.chunkRows": 30_000})
    assert m["agg_wide_min_max_passes"] >= 1, m
    keys = g.tolist()
    b_vals = ints_of(hi2, lo2, mask2)
    xs = [None if mk_ else int(v) for v, mk_ in zip(x.tolist(), xmask.tolist())]
    fs = [None if mk_ else v for v, mk_ in zip(f.tolist(), fmask.tolist())]
    mx_a, mn_b, mn_x, mx_f = model(keys, a_vals, "max"), model(keys, b_vals, "min"), model(keys, xs, "min"), model(keys, fs, "max")
    sums, counts, first, last_nn = {}, {}, {}, {}
    for k, v, xv in zip(keys, a_vals, xs):
        counts.setdefault(k, 0)
        sums.setdefault(k, None)
        if v is not None:
            sums[k] = (sums[k] or 0) + v
            counts[k] += 1
        first.setdefault(k, xv)
        last_nn.setdefault(k, None)
        if xv is not None:
            last_nn[k] = xv
    want = {}
    for k in mx_a:
        cnt, sm = counts[k], sums[k]
        # SumDecimal's state: (sum, is_empty); AvgDecimal's grouped state: (sum, count), the sum 0 for an empty group
        want[k] = (mx_a[k], mn_b[k], sm if cnt else 0, cnt == 0, sm if cnt else 0, cnt, cnt, mn_x[k], mx_f[k], first[k], True, last_nn[k], last_nn[k] is not None)
    assert_groups(got, want)


# --------------------------------------------------------------------------- 8. the same bits for any batching

def test_same_bits_for_any_batching_and_chunking(built):
    D = S.decimal(38, 4)
    t, keys, vals = spread_table(200_000, 1000, 8)
    want = want_min_max(keys, vals)
    plan = min_max_plan(D)
    for batch_rows, cfg in ((1000, None), (8192, None), (t.num_rows, None), (8192, {"spark.comet.gpu.chunkRows": 8192}), (5000, {"spark.comet.gpu.chunkRows": 50_000})):
        assert_groups(run(plan, t, 3, batch_rows, cfg), want, f"batch {batch_rows} {cfg}")
    rev = t.take(pa.array(np.arange(t.num_rows - 1, -1, -1)))
    assert_groups(run(plan, rev, 3), want, "reversed")


# --------------------------------------------------------------------------- 9. every precision class, values over the type's whole range

@pytest.mark.parametrize("p,s", [(19, 2), (20, 5), (28, 10), (38, 18)])
def test_precisions(built, p, s):
    n, ng = 20_000, 300
    r = random.Random(p)
    top = 10**p - 1
    keys = [r.randrange(ng) for _ in range(n)]
    vals = [None if r.random() < 0.1 else r.randint(-top, top) for _ in range(n)]
    assert sum(1 for v in vals if v is not None and (v & M64) >> 63) > n // 4      # a low word with its top bit set is common
    D = S.decimal(p, s)
    t = pa.table({"g": pa.array(keys, pa.int32()), "d": dec_of(vals, p, s)})
    got = run(min_max_plan(D), t, 3)
    assert got.schema.field(1).type == pa.decimal128(p, s)
    assert_groups(got, want_min_max(keys, vals))
