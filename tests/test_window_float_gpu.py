"""Float64 / Float32 SUM and AVG over window frames (window_kernels.hip "Float sums over frames"): every frame's result is the exact real sum of
its rows rounded once, so the yardstick is math.fsum over the frame's rows — bit for bit, whatever the frame shape, the scan tiling or the
input batching — and fsum / count for AVG.  NULL exactly where the frame holds no non-NULL row; ±inf and NaN follow IEEE while they are in
the frame and are gone when they leave it.  ROWS frames are checked on a unique order key."""
import math

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S

pytestmark = pytest.mark.gpu
F64, F32, I32, I64 = S.T_DOUBLE, S.T_FLOAT, S.T_INT32, S.T_INT64
INF, NAN = float("inf"), float("nan")
FIELDS = [I32, I64, I32, F64, F32]                       # partition, unique order key, tied order key, argument, Float32 argument
G, K, T, X, X32 = (S.col(i, t) for i, t in enumerate(FIELDS))
SIZES = [4500, 900, 500, 80, 19, 1]                      # 6 000 rows; the first partition straddles more than two 2048-row scan tiles
WHOLE = ("rows", "unbounded", "unbounded")
ROWS_FRAMES = [("rows", -2, 2), ("rows", -3, "current"), ("rows", "current", 4), ("rows", -5, -2), ("rows", 1, 3), ("rows", "unbounded", 1), ("rows", -1, "unbounded"),
               ("rows", "current", "unbounded"), ("rows", "current", "current"), ("range", "current", "unbounded"), ("rows", -2000, 2000), WHOLE, ("rows", "unbounded", "current")]


def _bits(v):
    return None if v is None else "nan" if math.isnan(v) else np.float64(v).tobytes()


def _run(plan, table, ncols, batch_rows=8192):
    return pa.Table.from_batches(native.execute_to_table([native.HostInput.from_table(table, batch_rows)], ncols, plan.encode(), batch_size=0))


def _plan(fns, order_col=K, fields=FIELDS):
    order = [(order_col, False, False)]
    return S.window(S.sort(S.scan(fields), [(G, False, False)] + order), [G], order, fns)


def _sorted_columns(tb, by):
    """the output's columns as Python lists, rows ordered by the given column indices (partition first)"""
    idx = np.lexsort([np.asarray(tb.column(c)) for c in reversed(by)])
    return [[col[i] for i in idx] for col in (tb.column(c).to_pylist() for c in range(tb.num_columns))]


def _rows_bounds(frame, i, m):
    """rows [start, end) of row i's ROWS frame in a partition of m rows (a RANGE frame over CURRENT ROW on a unique key is the same)"""
    _, lo, hi = frame
    start = 0 if lo == "unbounded" else i if lo == "current" else i + lo
    end = m if hi == "unbounded" else i + 1 if hi == "current" else i + hi + 1
    start, end = max(start, 0), min(end, m)
    return start, max(end, start)


class Expect:
    """per partition: the argument in key order (NULL as 0.0 — an exact no-op in a sum) and its non-NULL prefix counts; sums are cached per (partition, start, end)"""

    def __init__(self, values_by_partition):
        self.z = [[0.0 if v is None else v for v in vs] for vs in values_by_partition]
        self.c = [np.r_[0, np.cumsum([v is not None for v in vs])] for vs in values_by_partition]
        self.cache = {}

    def sum_count(self, p, start, end):
        key = (p, start, end)
        if key not in self.cache:
            cnt = int(self.c[p][end] - self.c[p][start])
            self.cache[key] = (math.fsum(self.z[p][start:end]) if cnt else None, cnt)
        return self.cache[key]


@pytest.fixture(scope="module")
def frames_table():
    rng = np.random.default_rng(20)
    n = sum(SIZES)
    g = np.repeat(np.arange(len(SIZES), dtype=np.int32), SIZES)
    k = np.concatenate([rng.permutation(m) for m in SIZES]).astype(np.int64) * 3 - 50
    x = rng.standard_normal(n) * rng.choice([1e-3, 1.0, 1e6], n)
    # the cancellation a prefix sum of doubles gets wrong: ±1e15 alternating with small values, along the first partition's key order
    for j in range(600):
        row = int(np.flatnonzero((g == 0) & (k == (1000 + j) * 3 - 50))[0])
        x[row] = 1e15 if j % 4 == 0 else -1e15 if j % 4 == 2 else x[row]
    x32 = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 1e6], n)).astype(np.float32)
    t = rng.integers(0, 40, n).astype(np.int32)
    shuffle = rng.permutation(n)
    table = pa.table({"g": pa.array(g), "k": pa.array(k), "t": pa.array(t), "x": pa.array(x, mask=rng.random(n) < 0.1), "x32": pa.array(x32, mask=rng.random(n) < 0.1)})
    return table.take(pa.array(shuffle))


def _partitions(cols, order_col):
    """rows (already ordered by partition and order key) → per partition the lists of the columns"""
    g = np.asarray(cols[0])
    starts = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])
    return [(int(a), int(b)) for a, b in zip(starts, np.r_[starts[1:], len(g)])]


def test_sum_avg_count_over_every_frame_shape(built, frames_table):
    fns = []
    for fr in ROWS_FRAMES:
        fns += [("agg", S.sum_(X, F64), F64, fr), ("agg", S.avg(X, F64, F64), F64, fr), ("agg", S.count(X), I64, fr)]
    fns += [("agg", S.sum_(X32, F64), F64, ("rows", -2, 2)), ("agg", S.avg(X32, F64, F64), F64, ("rows", "unbounded", "current"))]
    nf = len(FIELDS)
    got = _run(_plan(fns), frames_table, nf + len(fns))
    assert got.schema.types[nf:] == [pa.float64(), pa.float64(), pa.int64()] * len(ROWS_FRAMES) + [pa.float64(), pa.float64()]
    cols = _sorted_columns(got, [0, 1])
    parts = _partitions(cols, 1)
    assert [b - a for a, b in parts] == SIZES
    ex = Expect([cols[3][a:b] for a, b in parts])
    ex32 = Expect([cols[4][a:b] for a, b in parts])
    nulls = 0
    for p, (a, b) in enumerate(parts):
        m = b - a
        for i in range(m):
            for f, fr in enumerate(ROWS_FRAMES):
                s, c = ex.sum_count(p, *_rows_bounds(fr, i, m))
                row = (cols[nf + 3 * f][a + i], cols[nf + 3 * f + 1][a + i], cols[nf + 3 * f + 2][a + i])
                want = (s, None if s is None else s / c, c)
                assert (_bits(row[0]), _bits(row[1]), row[2]) == (_bits(want[0]), _bits(want[1]), want[2]), (p, i, fr, row, want)
                nulls += s is None
            s, c = ex32.sum_count(p, *_rows_bounds(("rows", -2, 2), i, m))
            assert _bits(cols[nf + 3 * len(ROWS_FRAMES)][a + i]) == _bits(s), (p, i, "float32 sum")
            s, c = ex32.sum_count(p, 0, i + 1)
            assert _bits(cols[nf + 3 * len(ROWS_FRAMES) + 1][a + i]) == _bits(None if s is None else s / c), (p, i, "float32 avg")
    assert nulls > 20                     # (5 PRECEDING, 2 PRECEDING) at the head of every partition, frames of NULL rows only
    # the cancellation stretch is what a prefix sum of doubles gets wrong: the running double sum there differs from the exact one
    z = ex.z[0]
    assert any(float(np.cumsum(z[:1300])[j]) != math.fsum(z[:j + 1]) for j in range(1000, 1300))


def test_range_frames_on_a_tied_key(built, frames_table):
    """RANGE frames see peers: UNBOUNDED … CURRENT ROW ends behind the row's last peer, a value offset frames the keys within [t − 3, t + 5] — both invariant
    under the order among ties, which the Sort does not fix"""
    frames = [("range", "unbounded", "current"), ("range", ("value", S.lit(3, I32)), ("value", S.lit(5, I32))), ("range", "current", "unbounded")]
    fns = []
    for fr in frames:
        fns += [("agg", S.sum_(X, F64), F64, fr), ("agg", S.avg(X, F64, F64), F64, fr)]
    nf = len(FIELDS)
    got = _run(_plan(fns, order_col=T), frames_table, nf + len(fns))
    cols = _sorted_columns(got, [0, 2])
    parts = _partitions(cols, 2)
    ex = Expect([cols[3][a:b] for a, b in parts])
    for p, (a, b) in enumerate(parts):
        t = np.asarray(cols[2][a:b])
        left, right = np.searchsorted(t, t, "left"), np.searchsorted(t, t, "right")
        lo3, hi5 = np.searchsorted(t, t - 3, "left"), np.searchsorted(t, t + 5, "right")
        for i in range(b - a):
            for f, (start, end) in enumerate([(0, right[i]), (lo3[i], hi5[i]), (left[i], b - a)]):
                s, c = ex.sum_count(p, int(start), int(end))
                assert (_bits(cols[nf + 2 * f][a + i]), _bits(cols[nf + 2 * f + 1][a + i])) == (_bits(s), _bits(None if s is None else s / c)), (p, i, frames[f])


def test_result_does_not_depend_on_input_batching(built, frames_table):
    fns = [("agg", S.sum_(X, F64), F64, fr) for fr in (("rows", -2, 2), ("rows", "unbounded", "current"), WHOLE)] + [("agg", S.avg(X, F64, F64), F64, ("rows", -3, "current"))]
    plan = _plan(fns)
    a = _sorted_columns(_run(plan, frames_table, len(FIELDS) + len(fns), batch_rows=8192), [0, 1])
    b = _sorted_columns(_run(plan, frames_table, len(FIELDS) + len(fns), batch_rows=777), [0, 1])
    for ca, cb in zip(a[len(FIELDS):], b[len(FIELDS):]):
        assert [_bits(v) for v in ca] == [_bits(v) for v in cb]


def _ieee_sum(rows):
    xs = [v for v in rows if v is not None]
    if not xs:
        return None
    if any(math.isnan(v) for v in xs) or (INF in xs and -INF in xs):
        return NAN
    return math.fsum(xs)


def test_inf_and_nan_are_in_the_frame_or_gone(built):
    """(1 PRECEDING, 1 FOLLOWING): inf while a frame holds one, NaN for both signs or a NaN, and the exact finite sum again two rows behind each special —
    where a retracting accumulator would stay NaN for the rest of the partition"""
    big = 2.0 ** 60
    special = [1.5, 2.25, INF, 4.0, 0.1, 0.2, -INF, INF, 0.3, 0.7, big, NAN, 1e-3, 1e3, None, -INF, 5.0, 6.0, -0.0, 0.0, -0.0, None, 7.0, big, big, -big]
    plain = [float(v) for v in np.random.default_rng(3).standard_normal(300)]
    values = special + plain
    n = len(values)
    g = np.r_[np.zeros(len(special), np.int32), np.ones(len(plain), np.int32)]
    fields = [I32, I64, I32, F64]
    table = pa.table({"g": pa.array(g), "k": pa.array(np.arange(n, dtype=np.int64)), "t": pa.array(np.zeros(n, np.int32)), "x": pa.array(values, pa.float64())})
    frames = [("rows", -1, 1), ("rows", "unbounded", "current"), ("rows", "current", "unbounded"), WHOLE]
    fns = [("agg", S.sum_(X, F64), F64, fr) for fr in frames] + [("agg", S.avg(X, F64, F64), F64, ("rows", -1, 1))]
    got = _run(_plan(fns, fields=fields), table, 4 + len(fns))
    cols = _sorted_columns(got, [0, 1])
    for a, b in ((0, len(special)), (len(special), n)):
        m = b - a
        for i in range(m):
            for f, fr in enumerate(frames):
                start, end = _rows_bounds(fr, i, m)
                assert _bits(cols[4 + f][a + i]) == _bits(_ieee_sum(values[a + start:a + end])), (i, fr, cols[4 + f][a + i])
            start, end = _rows_bounds(frames[0], i, m)
            s, c = _ieee_sum(values[a + start:a + end]), sum(v is not None for v in values[a + start:a + end])
            assert _bits(cols[4 + len(frames)][a + i]) == _bits(None if s is None else s / c), (i, "avg")
    s3 = cols[4]
    assert s3[2] == INF and s3[1] == INF and math.isnan(s3[6]) and math.isnan(s3[7]) and math.isnan(s3[11]) and s3[15] == -INF
    assert s3[4] == math.fsum([4.0, 0.1, 0.2]) and s3[9] == math.fsum([0.3, 0.7, big]) and s3[13] == 1e-3 + 1e3 and s3[17] == 11.0   # two rows behind a special
    assert s3[24] == big and s3[23] == math.fsum([7.0, big, big])
    assert _bits(s3[19]) == _bits(0.0) and s3[21] == 7.0                 # a frame of zeros sums to +0.0, like the grouped sum


def test_scan_tiles_of_tiles_and_partitions_split_inside_a_tile(built):
    """more than 256 scan tiles (the tile totals are then scanned several per thread), a partition boundary inside a tile; integer-valued doubles below 2^20,
    so numpy's cumulative sums are exact and every row is compared"""
    n = 256 * 2048 + 4097
    cut = 300_000 + 777
    rng = np.random.default_rng(8)
    x = rng.integers(-(1 << 20), 1 << 20, n).astype(np.float64)
    null = rng.random(n) < 0.1
    null[:3] = True
    g = (np.arange(n) >= cut).astype(np.int32)
    fields = [I32, I64, I32, F64]
    table = pa.table({"g": pa.array(g), "k": pa.array(np.arange(n, dtype=np.int64)), "t": pa.array(np.zeros(n, np.int32)), "x": pa.array(x, mask=null)})
    fns = [("agg", S.sum_(X, F64), F64, ("rows", "unbounded", "current")), ("agg", S.sum_(X, F64), F64, WHOLE)]
    got = _run(_plan(fns, fields=fields), table, 6, batch_rows=1 << 16)
    order = np.argsort(np.asarray(got.column(1)))
    assert np.array_equal(np.asarray(got.column(1))[order], np.arange(n))
    z = np.where(null, 0.0, x)
    for a, b in ((0, cut), (cut, n)):
        running, seen = np.cumsum(z[a:b]), np.cumsum(~null[a:b])
        for c, want in ((4, running), (5, np.full(b - a, running[-1]))):
            col = got.column(c).combine_chunks()
            valid = np.asarray(col.is_valid())[order][a:b]
            vals = col.fill_null(0.0).to_numpy()[order][a:b]
            assert np.array_equal(valid, seen > 0 if c == 4 else np.ones(b - a, bool))
            assert np.array_equal(vals[valid], want[valid])


@pytest.fixture(scope="module")
def wide_range(built):
    """2^-300 … 2^300 in one column — more than kFixW − 10 = 148 binary orders, where the shared scale rule alone gives s = top + 2 − 158 and would truncate the bits
    below 2^s; the executor cuts such a column into several 158-bit windows instead.  → (n, s, the values, [(frame, got column)]) for two partitions of 1 500 rows"""
    rng = np.random.default_rng(9)
    n = 3000
    x = rng.standard_normal(n) * np.exp2(rng.integers(-300, 300, n).astype(np.float64))
    x[1000:1100] = rng.standard_normal(100) * 2.0 ** 290
    g = (np.arange(n) // 1500).astype(np.int32)
    fields = [I32, I64, I32, F64]
    table = pa.table({"g": pa.array(g), "k": pa.array(np.arange(n, dtype=np.int64)), "t": pa.array(np.zeros(n, np.int32)), "x": pa.array(x)})
    frames = [("rows", -3, 3), ("rows", "unbounded", "current")]
    got = _run(_plan([("agg", S.sum_(X, F64), F64, fr) for fr in frames], fields=fields), table, 6)
    cols = _sorted_columns(got, [0, 1])
    s = max(math.frexp(v)[1] for v in x) + 2 - 158
    return n, s, x.tolist(), [(fr, cols[4 + f]) for f, fr in enumerate(frames)]


def test_truncation_keeps_frames_of_large_values_exact(wide_range):
    n, s, xs, results = wide_range
    fr, col = results[0]
    for i in range(1003, 1097):                  # (3 PRECEDING, 3 FOLLOWING) inside the stretch of values near 2^290
        assert col[i] == math.fsum(xs[i - 3:i + 4]), i


def test_truncation_every_frame_within_rows_times_two_to_the_scale(wide_range):
    """Every frame within n · 2^s of math.fsum, s the scale the shared rule gives for the column.  Truncating at 2^s does not achieve that: in 3 of these 6 000
    frames (row 1117, (3 PRECEDING, 3 FOLLOWING): 3.943629562086103e+82 − 7.815372586081521e+81 + …) two large values sum to an exact tie between two doubles and
    a value below 2^s decides it, which puts a truncated sum one ulp of the RESULT (6.7e66, where n · 2^s = 6.7e46) from fsum.  With the column cut into windows no bit
    is dropped, so every frame is also bit-equal to fsum."""
    n, s, xs, results = wide_range
    beyond, unequal = [], []
    for fr, col in results:
        for i in range(n):
            a = (i // 1500) * 1500
            start, end = _rows_bounds(fr, i - a, 1500)
            want = math.fsum(xs[a + start:a + end])
            if abs(col[i] - want) > n * 2.0 ** s:
                beyond.append((i, fr, col[i], want, abs(col[i] - want) / math.ulp(want)))
            if col[i] != want:
                unequal.append((i, fr, col[i], want))
    print(f"scale 2^{s}: {len(beyond)} of {2 * n} frames beyond n * 2^s, {len(unequal)} not bit-equal")
    assert not beyond, beyond[:3]
    assert not unequal, unequal[:3]
