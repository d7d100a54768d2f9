"""Every path of sort_table (csrc/exec_sort.cpp) at the smallest shape that selects it, with the path asserted through the plan's sort counters
(sort_select_passes, sort_small_sorts, sort_radix_passes, sort_rows_sorted on the root metric node) and the answer checked against tests/sort_model.py —
the numpy model tests/test_sort_model_cpu.py pins to the oracle — never against another device result:

  TopK gate (fetch·8 < rows) → radix select, one pass per varying plane while more than max(4096, needed) candidates are left
  → what is left: at most 4096 rows and at most 16 varying planes: one workgroup's bitonic sort; else one LSD radix pass per varying plane, whose histogram
    scan is one block up to 65 536 rows and three launches above
  → rows [skip, fetch) taken column by column.

The expected counters are read off the data: tests/sort_model.py key_bytes writes the key bytes down in numpy, sort_path walks the rules above over them.
Unless a case says otherwise the last sort key is a unique id, so the output must equal the model row for row; every table carries a nullable Boolean, a
nullable Utf8 of mixed lengths and a Decimal(38,10) behind the id, so that the take crosses its bit-packed, Utf8 and 16-byte paths."""
import functools

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S
from tests import sort_model as M

pytestmark = pytest.mark.gpu

D38 = S.decimal(38, 10)
COUNTERS = ("sort_select_passes", "sort_small_sorts", "sort_radix_passes", "sort_rows_sorted")
_WORDS = ["", "a", "ab", "é", "日本語", "Customer#000000001", "x" * 40, "a much longer value that crosses more than one 64-byte line of the bytes buffer, for the copy's sake", "z"]


def _payload(n, rng):
    """(arrays, fields): id, then a nullable Boolean, a nullable Utf8 of mixed lengths, a Decimal(38,10)"""
    raw = np.zeros(n, np.dtype([("lo", "<u8"), ("hi", "<i8")]))
    raw["lo"], raw["hi"] = rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + 1, rng.integers(-5 * 10**18, 5 * 10**18, n)      # |value| < 5·10^18·2^64 < 10^38
    dec = pa.Array.from_buffers(pa.decimal128(38, 10), n, [None, pa.py_buffer(raw.tobytes())])
    s = pa.array(_WORDS, pa.string()).take(pa.array(rng.integers(0, len(_WORDS), n), pa.int64(), mask=rng.random(n) < 0.15))
    return ([pa.array(np.arange(n, dtype=np.int64)), pa.array(rng.random(n) < 0.5, mask=rng.random(n) < 0.2), s, dec], [S.T_INT64, S.T_BOOL, S.T_STRING, D38])


def _table(keys, key_fields, n, rng):
    arrays, fields = _payload(n, rng)
    cols = list(keys) + arrays
    return pa.table(cols, names=["c%d" % i for i in range(len(cols))]), list(key_fields) + fields


def _run(plan, table, ncols):
    """the plan through CometExecIterator → (its output as one table, or None when it yields no batch; the root node's metrics)"""
    it = native.CometExecIterator([native.HostInput.from_table(table)], ncols, plan.encode(), batch_size=0)
    batches = []
    while True:
        b = native.Native.executePlan(it.handle, ncols)
        if b is None:
            break
        batches.append(b)
    m = S.decode_metric_node(it.metrics())[0]
    it.close()
    return (pa.Table.from_batches(batches) if batches else None), m


def _sort(t, fields, keys, fetch=None, skip=0, exact=True, id_col=None):
    """Sort t by keys = [(column, descending, nulls_last)] on the device; the answer against the model, the counters against the path read off the key bytes.
    → (output, the counters)"""
    plan = S.sort(S.scan(fields), [(S.col(c, fields[c]), d, nl) for c, d, nl in keys], fetch=fetch, skip=skip)
    got, m = _run(plan, t, len(fields))
    want = M.sort_path(M.key_bytes(t, keys), fetch, skip)
    if want is None:
        assert not any(c in m for c in COUNTERS), m
    else:
        assert {c: m.get(c) for c in COUNTERS} == want, (m, want)
    if exact:
        M.assert_same_rows(got, t, M.expected_order(t, keys, fetch, skip))
    else:
        M.check_sorted(got, t, keys, fetch, skip, id_col)
        if got is not None:      # the payload of every row is that id's
            M.assert_same_rows(got, t, np.asarray(got.column(id_col).to_numpy()), cols=range(id_col, t.num_columns))
    return got, {c: m.get(c) for c in COUNTERS}


def _low_card(n, rng):
    return pa.array(rng.integers(-3, 4, n).astype(np.int32), mask=rng.random(n) < 0.15)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1023, 1025, 4095, 4096, 4097])
def test_one_workgroup_up_to_4096_rows(built, n):
    """the bitonic network pads to a power of two (from 2): one row, the powers themselves, one past them, the last size it takes — and 4097 rows, the first
    that go through radix passes"""
    rng = np.random.default_rng(n)
    t, f = _table([_low_card(n, rng)], [S.T_INT32], n, rng)
    _, c = _sort(t, f, [(0, True, False), (1, False, False)], skip=3 if n > 64 else 0)
    if n <= 4096:
        assert c["sort_small_sorts"] == 1 and c["sort_radix_passes"] == 0 and c["sort_select_passes"] == 0 and c["sort_rows_sorted"] == n
    else:
        assert c["sort_small_sorts"] == 0 and c["sort_radix_passes"] >= 3 and c["sort_rows_sorted"] == n


def test_sixteen_varying_planes_one_workgroup_seventeen_radix(built):
    rng = np.random.default_rng(16)
    n = 3000
    a, b = rng.integers(-(1 << 63), (1 << 63) - 1, n), rng.integers(-(1 << 63), (1 << 63) - 1, n)
    assert len(np.unique(b)) == n
    keys = [(0, False, False), (1, True, True)]
    t, f = _table([pa.array(a), pa.array(b)], [S.T_INT64, S.T_INT64], n, rng)
    _, c = _sort(t, f, keys)
    assert c == {"sort_select_passes": 0, "sort_small_sorts": 1, "sort_radix_passes": 0, "sort_rows_sorted": n}      # 2 × 8 value planes; the NULL bytes are constant
    t2 = t.set_column(0, "c0", pa.array(a, mask=rng.random(n) < 0.1))
    _, c = _sort(t2, f, keys)
    assert c == {"sort_select_passes": 0, "sort_small_sorts": 0, "sort_radix_passes": 17, "sort_rows_sorted": n}     # … and the first key's NULL byte
    # the same rows in the same order wherever the first key is not NULL in either
    both = np.flatnonzero(t2.column(0).is_valid().to_numpy(zero_copy_only=False))
    o1, o2 = M.expected_order(t, keys), M.expected_order(t2, keys)
    assert o1[np.isin(o1, both)].tolist() == o2[np.isin(o2, both)].tolist()


@pytest.mark.parametrize("n", [100, 5000])
@pytest.mark.parametrize("fetch", [None, 10])
def test_no_plane_varies(built, n, fetch):
    """a constant key and an all-NULL key: no select pass, no radix pass; any permutation of the input is a right answer, and a fetch may keep any rows"""
    rng = np.random.default_rng(n)
    t, f = _table([pa.array(np.full(n, 7, np.int32)), pa.array([None] * n, pa.int32())], [S.T_INT32, S.T_INT32], n, rng)
    for keys in ([(0, False, False)], [(1, True, False)], [(1, False, True), (0, True, True)]):
        got, c = _sort(t, f, keys, fetch=fetch, exact=False, id_col=2)
        assert c["sort_select_passes"] == 0 and c["sort_radix_passes"] == 0 and c["sort_small_sorts"] == (1 if n <= 4096 else 0) and c["sort_rows_sorted"] == n
        assert got.num_rows == (n if fetch is None else fetch) and got.column(0).to_pylist() == [7] * got.num_rows and got.column(1).null_count == got.num_rows
        if fetch is None:
            assert sorted(got.column(2).to_pylist()) == list(range(n))


def _floats(n, rng):
    """Float64 with both zeros, NaNs of both signs and two payloads, infinities, and NULLs"""
    bits = rng.standard_normal(n).view(np.uint64).copy()
    special = np.array([0, 1 << 63, 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000005, 0xFFF8000000000005, 0x7FF0000000000000, 0xFFF0000000000000], np.uint64)
    at = rng.random(n) < 0.02
    bits[at] = special[rng.integers(0, len(special), int(at.sum()))]
    bits[:len(special)] = special
    return M._float_array(bits, rng.random(n) < 0.05, True)


@pytest.mark.parametrize("n", [65_536, 65_537, 300_007])
def test_radix_passes_single_block_and_three_launch_scan(built, n):
    """256 partitions over 65 536 rows are the last shape whose histogram scan is one block; one row more takes the three-launch scan"""
    rng = np.random.default_rng(n)
    h = pa.array(rng.integers(-2, 3, n).astype(np.int16) * 300)
    t, f = _table([_floats(n, rng), h], [S.T_DOUBLE, S.T_INT16], n, rng)
    keys = [(0, True, True), (1, False, False), (2, False, False)]
    _, c = _sort(t, f, keys, skip=5)
    K = M.key_bytes(t, keys)
    assert c["sort_radix_passes"] == int((K.min(axis=0) != K.max(axis=0)).sum()) >= 12 and c["sort_small_sorts"] == 0 and c["sort_rows_sorted"] == n


@pytest.mark.parametrize("n,fetch,passes", [(8000, 1000, False), (8000, 999, True), (40_000, 4999, True)])
def test_topk_gate(built, n, fetch, passes):
    """fetch·8 < rows opens the TopK branch: 1000 of 8000 stays outside, 999 is inside (8000 candidates are more than max(4096, 999): select passes run); with
    4999 wanted of 40 000 the select stops as soon as at most 4999 candidates are left"""
    rng = np.random.default_rng(fetch)
    t, f = _table([pa.array(rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32), mask=rng.random(n) < 0.03)], [S.T_INT32], n, rng)
    _, c = _sort(t, f, [(0, False, True), (1, True, True)], fetch=fetch, skip=5)
    assert (c["sort_select_passes"] > 0) == passes and (c["sort_rows_sorted"] < n) == passes and c["sort_rows_sorted"] >= fetch


@pytest.mark.parametrize("desc,nulls_last", [(False, True), (True, False)])
def test_select_then_one_workgroup(built, desc, nulls_last):
    """100 000 rows, the first 10 wanted: ASC the select narrows through the value's planes; DESC NULLS FIRST the 5 000 NULL keys come first, their value bytes
    are all zero, and the select has to go on through the id's planes"""
    rng = np.random.default_rng(10)
    n = 100_000
    t, f = _table([pa.array(rng.integers(-(1 << 63), (1 << 63) - 1, n), mask=rng.random(n) < 0.05)], [S.T_INT64], n, rng)
    _, c = _sort(t, f, [(0, desc, nulls_last), (1, False, False)], fetch=10, skip=3)
    assert c["sort_select_passes"] >= (1 if not desc else 10) and c["sort_small_sorts"] == 1 and c["sort_radix_passes"] == 0 and 10 <= c["sort_rows_sorted"] <= 4096


def test_select_then_radix_for_a_large_answer(built):
    rng = np.random.default_rng(6000)
    n = 100_000
    t, f = _table([pa.array(rng.integers(-(1 << 63), (1 << 63) - 1, n), mask=rng.random(n) < 0.05)], [S.T_INT64], n, rng)
    got, c = _sort(t, f, [(0, True, True), (1, False, False)], fetch=6000, skip=5995)
    assert got.num_rows == 5 and c["sort_select_passes"] >= 1 and c["sort_small_sorts"] == 0 and c["sort_radix_passes"] >= 10 and 6000 <= c["sort_rows_sorted"] < n


def test_ties_across_the_kth_place(built):
    """three key values over 100 000 rows and the first 100 wanted: every select pass keeps the whole tied bucket, which then goes through the radix passes"""
    rng = np.random.default_rng(3)
    n = 100_000
    k = np.array([-70_000, 5, 1 << 20], np.int32)[rng.integers(0, 3, n)]
    t, f = _table([pa.array(k)], [S.T_INT32], n, rng)
    keys = [(0, False, False)]
    K = M.key_bytes(t, keys)
    varying = int((K.min(axis=0) != K.max(axis=0)).sum())
    got, c = _sort(t, f, keys, fetch=100, exact=False, id_col=1)
    assert varying >= 3 and c["sort_select_passes"] == varying and c["sort_radix_passes"] == varying and c["sort_small_sorts"] == 0
    assert c["sort_rows_sorted"] == int((k == -70_000).sum()) > 30_000 and got.column(0).to_pylist() == [-70_000] * 100


def test_more_nulls_than_k(built):
    rng = np.random.default_rng(500)
    n = 50_000
    mask = np.zeros(n, bool)
    mask[rng.permutation(n)[:2000]] = True
    t, f = _table([pa.array(rng.integers(-1000, 1000, n).astype(np.int32), mask=mask)], [S.T_INT32], n, rng)
    got, c = _sort(t, f, [(0, False, False)], fetch=500, exact=False, id_col=1)
    assert c == {"sort_select_passes": 1, "sort_small_sorts": 1, "sort_radix_passes": 0, "sort_rows_sorted": 2000}
    assert got.num_rows == 500 and got.column(0).null_count == 500 and mask[got.column(1).to_numpy()].all()


def test_k_lands_on_a_bucket_edge(built):
    """exactly 100 rows hold the smallest Int8 and 100 are wanted: the first select pass finds below + h[d] == needed at its first digit"""
    rng = np.random.default_rng(100)
    n = 10_000
    k = rng.integers(-127, 128, n).astype(np.int8)
    k[rng.permutation(n)[:100]] = -128
    t, f = _table([pa.array(k)], [S.T_INT8], n, rng)
    got, c = _sort(t, f, [(0, False, False), (1, False, False)], fetch=100)
    assert c == {"sort_select_passes": 1, "sort_small_sorts": 1, "sort_radix_passes": 0, "sort_rows_sorted": 100}
    assert got.column(1).to_pylist() == np.flatnonzero(k == -128).tolist()


def test_fetch_and_skip_edges(built):
    rng = np.random.default_rng(9)
    n = 1000
    t, f = _table([_low_card(n, rng)], [S.T_INT32], n, rng)
    keys = [(0, False, True), (1, True, False)]
    for fetch, skip in ((10, 10), (10, 11), (None, n + 1), (None, n), (0, 0)):
        got, _ = _sort(t, f, keys, fetch=fetch, skip=skip)
        assert got is None
    got, _ = _sort(t.slice(0, 0), f, keys)
    assert got is None
    got, c = _sort(t, f, keys, fetch=n + 5, skip=13)
    assert got.num_rows == n - 13 and c["sort_rows_sorted"] == n
    got, _ = _sort(t, f, keys, skip=n - 1)
    assert got.num_rows == 1
    for limit, offset, rows in ((n, n, 0), (n + 10, n + 7, 0), (-1, n, 0), (-1, n + 7, 0), (n + 1, n - 3, 3), (20, 13, 7)):
        got, m = _run(S.limit(S.scan(f), limit, offset), t, len(f))
        M.assert_same_rows(got, t, np.arange(min(offset, n), min(offset, n) + rows))
        assert not any(c in m for c in COUNTERS), m      # the counters are a sorting plan's
    with pytest.raises(native.CometNativeException, match="Invalid limit/offset combination"):      # (an offset beyond the limit is refused at planning, planner.rs:1440)
        _run(S.limit(S.scan(f), 5, n + 7), t, len(f))


def test_utf8_key_wider_than_1000_bytes_is_refused(built):
    t = pa.table({"s": pa.array(["a", "b" * 996, None]), "id": pa.array(np.arange(3, dtype=np.int64))})
    f = [S.T_STRING, S.T_INT64]
    with pytest.raises(native.CometNativeException, match="wider than 1000 bytes"):      # 1 + 996 + 4 = 1001
        _run(S.sort(S.scan(f), [(S.col(0, S.T_STRING), False, False)]), t, 2)
    got, _ = _run(S.sort(S.scan(f), [(S.col(0, S.T_STRING), True, True)]), t.set_column(0, "s", pa.array(["a", "b" * 995, None])), 2)
    assert got.column(1).to_pylist() == [1, 0, 2]


@functools.lru_cache(maxsize=None)
def _type_cases():
    return {c["name"]: c for c in M.key_cases(S, n=5000, seed=21)}


@pytest.mark.parametrize("k,name", list(enumerate(["bool", "int8", "int16", "float32", "timestamp", "decimal(9,2)", "decimal(38,10)", "substring(s,1,3)", "substring(s,1,15)", "a+b"])))
def test_every_key_type_on_the_device(built, k, name):
    """the key types no other GPU test sorts by, each as first key before the id: DESC NULLS FIRST for half of them, ASC NULLS LAST for the others"""
    case = _type_cases()[name]
    arrays, fields = _payload(5000, np.random.default_rng(k))
    t, f = case["table"], case["fields"] + fields[1:]
    for j, a in enumerate(arrays[1:]):
        t = t.append_column("p%d" % j, a)
    desc, nl = (True, False) if k % 2 == 0 else (False, True)
    plan = S.sort(S.scan(f), [(case["key"], desc, nl), (S.col(case["id"], S.T_INT64), False, False)])
    got, m = _run(plan, t, len(f))
    M.assert_same_rows(got, t, M.expected_order(t, [(case["model"], desc, nl), (case["id"], False, False)]))
    assert m["sort_rows_sorted"] == 5000 and m["sort_select_passes"] == 0 and m["sort_radix_passes"] >= 3 and m["sort_small_sorts"] == 0


def _window_table(n, seed):
    rng = np.random.default_rng(seed)
    pool = np.array([0, 1 << 63, 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000005, 0x3FF8000000000000, 0xC004000000000000, 0x7FF0000000000000, 0x0000000000000001], np.uint64)
    f = M._float_array(pool[rng.integers(0, len(pool), n)], rng.random(n) < 0.08, True)
    k8 = pa.array(rng.integers(-128, 128, n).astype(np.int8), mask=rng.random(n) < 0.1)
    return _table([f, k8], [S.T_DOUBLE, S.T_INT8], n, rng)


def _window_plan(f):
    part, order = S.col(0, S.T_DOUBLE), (S.col(1, S.T_INT8), False, False)
    child = S.sort(S.scan(f), [(part, False, False), order, (S.col(2, S.T_INT64), False, False)])
    return S.window(child, [part], [order], [("dense_rank", [], S.T_INT32), ("row_number", [], S.T_INT32)])


def test_window_over_a_three_launch_sort(built):
    """dense_rank and row_number over partitions of a Float64 with both zeros and NaNs of several bit patterns — the partition and peer flags compare the key
    bytes of neighbours, so −0.0 and 0.0 are two partitions and NaNs of one bit pattern are one (arrow-ord's partition: `distinct` under totalOrder), above a
    Sort of 70 001 rows (the three-launch scan): against the oracle on 3 000 rows, against a numpy evaluation at full size"""
    from oracle import oracle as O
    t, f = _window_table(3000, 70)
    plan = _window_plan(f)
    got, m = _run(plan, t, len(f) + 2)
    want = O.run_plan_to_arrow(S, plan, [t])
    assert got.schema.types == want.schema.types
    M.assert_same_rows(got, want, np.arange(3000))
    n = 70_001
    t, f = _window_table(n, 71)
    got, m = _run(plan, t, len(f) + 2)
    keys = [(0, False, False), (1, False, False), (2, False, False)]
    order = M.expected_order(t, keys)
    M.assert_same_rows(got.select(list(range(len(f)))), t, order)
    r = M.rank_keys(t, keys[:2])[order]
    newp = np.r_[True, (r[1:, :2] != r[:-1, :2]).any(axis=1)]
    newg = newp | np.r_[True, (r[1:, 2:] != r[:-1, 2:]).any(axis=1)]
    start = np.maximum.accumulate(np.where(newp, np.arange(n), 0))
    groups = np.cumsum(newg)
    assert got.column(len(f)).to_pylist() == (groups - groups[start] + 1).tolist()
    assert got.column(len(f) + 1).to_pylist() == (np.arange(n) - start + 1).tolist()
    assert int(newp.sum()) == 10      # nine bit patterns and NULL
    K = M.key_bytes(t, keys)
    assert {c: m.get(c) for c in COUNTERS} == {"sort_select_passes": 0, "sort_small_sorts": 0, "sort_radix_passes": int((K.min(axis=0) != K.max(axis=0)).sum()), "sort_rows_sorted": n}
