"""sort_array, array_distinct, array_min / array_max and array_position on the GPU, through the C ABI against the pure-Python model of tests/list_fn_model.py
(pinned by tests/test_list_fn_cpu.py).  Values travel as plain integers / strings (dates as days, timestamps as microseconds, decimals unscaled).

Shapes: some 5 000 lists of 0 to 6 elements from a small domain (duplicates, NULL elements, NULL, empty and all-NULL lists); and one table whose lists have
exactly 0, 1, 2, 63, 64, 65, 255, 256, 257 and 5 000 elements — 256 is the longest list the rank kernel takes, a column with a longer one goes through the
engine's radix sort.  More than one 256-lane block in both."""
import decimal
import random

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S
from tests import list_fn_model as M

pytestmark = pytest.mark.gpu
I32, I64, STR = S.T_INT32, S.T_INT64, S.T_STRING
CAP = 256      # csrc/exec_internal.hpp kListFnMaxElements
D38 = 10 ** 38 - 1
WORDS = ["", "a", "a\0", "bb", "x", "日本", "日本語", "shared prefix, longer than eight bytes: 1", "shared prefix, longer than eight bytes: 2", "shared prefix", "k=v", "\x7f", "é"]

# kind → (serde type, Arrow type, the small domain its values come from)
KINDS = {
    "bool": (S.T_BOOL, pa.bool_(), [False, True]), "i8": (S.T_INT8, pa.int8(), [-128, -1, 0, 1, 127]), "i16": (S.T_INT16, pa.int16(), [-32768, -2, 0, 3, 32767]),
    "i32": (S.T_INT32, pa.int32(), [-2 ** 31, -7, 0, 7, 2 ** 31 - 1]), "i64": (S.T_INT64, pa.int64(), [-2 ** 63, -5, -1, 0, 1, 3, 2 ** 63 - 1]),
    "date": (S.T_DATE, pa.date32(), [-3, -1, 0, 1, 19000]), "ts": (S.T_TIMESTAMP, pa.timestamp("us", tz="UTC"), [-10 ** 15, -1, 0, 1, 10 ** 15]),
    "ntz": (S.DataType(S.TIMESTAMP_NTZ), pa.timestamp("us"), [-10 ** 15, -1, 0, 2, 10 ** 15]), "dec10_2": (S.decimal(10, 2), pa.decimal128(10, 2), [-10 ** 10 + 1, -100, 0, 1, 10 ** 10 - 1]),
    "dec38_0": (S.decimal(38, 0), pa.decimal128(38, 0), [-D38, -2 ** 64, -1, 0, 1, 2 ** 64, 2 ** 64 + 1, D38]), "str": (STR, pa.utf8(), WORDS),
}
INT_BASE = {"i8": pa.int8(), "i16": pa.int16(), "i32": pa.int32(), "i64": pa.int64(), "date": pa.int32(), "ts": pa.int64(), "ntz": pa.int64()}


def LT(kind):
    return S.list_type(KINDS[kind][0], True)


def scalars(kind, values):
    """model values (None = NULL) → an Arrow array of the kind"""
    t = KINDS[kind][1]
    if kind in ("bool", "str"):
        return pa.array(values, t)
    if kind.startswith("dec"):
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            return pa.array([None if v is None else decimal.Decimal(v).scaleb(-t.scale) for v in values], t)
    return pa.array(values, INT_BASE[kind]).cast(t)


def lists(kind, rows):
    """model lists (None = a NULL list) → an Arrow List<kind> column"""
    flat, offs, mask = [], [0], []
    for r in rows:
        flat.extend(r or [])
        offs.append(len(flat))
        mask.append(r is None)
    return pa.ListArray.from_arrays(pa.array(offs, pa.int32()), scalars(kind, flat), mask=pa.array(mask, pa.bool_()) if any(mask) else None)


def plain(kind, arr):
    """an Arrow array of the kind → model values"""
    if kind in ("bool", "str"):
        return arr.to_pylist()
    if kind.startswith("dec"):
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            return [None if d is None else int(d.scaleb(arr.type.scale)) for d in arr.to_pylist()]
    return arr.cast(INT_BASE[kind]).to_pylist()


def plain_lists(kind, col):
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    assert pa.types.is_list(col.type) and col.type.value_type == KINDS[kind][1], col.type
    vals, offs, ok = plain(kind, col.values), col.offsets.to_pylist(), col.is_valid().to_pylist()
    return [vals[offs[r]:offs[r + 1]] if ok[r] else None for r in range(len(col))]


def random_lists(kind, n, seed, max_len=6):
    rng = random.Random(seed)
    dom = KINDS[kind][2]
    rows = [[], [None, None], [dom[0], dom[0]], [None, dom[-1], None, dom[-1], dom[0]], None]
    while len(rows) < n:
        rows.append(None if rng.random() < 0.08 else [None if rng.random() < 0.1 else rng.choice(dom) for _ in range(rng.randrange(0, max_len + 1))])
    rng.shuffle(rows)
    return rows


def run(plan, table, ncols, batch_size=0, batch_rows=8192):
    out = native.execute_to_table([native.HostInput.from_table(table, batch_rows)], ncols, plan.encode(), batch_size=batch_size)
    return pa.Table.from_batches(out) if out else None


def run_metrics(plan, table, ncols):
    it = native.CometExecIterator([native.HostInput.from_table(table)], ncols, plan.encode(), batch_size=0)
    batches = []
    while True:
        b = native.Native.executePlan(it.handle, ncols)
        if b is None:
            break
        batches.append(b)
    m = S.decode_metric_node(it.metrics())[0]
    it.close()
    return pa.Table.from_batches(batches), m


def sort4(x):
    """array_sort under all four combinations of its two literals: (expression, ascending, nulls_last)"""
    out = []
    for asc in (True, False):
        for nl in (False, True):
            out.append((S.scalar_func("array_sort", [x, S.lit("ASC" if asc else "DESC", STR), S.lit("NULLS LAST" if nl else "NULLS FIRST", STR)]), asc, nl))
    return out


@pytest.mark.parametrize("kind", list(KINDS))
def test_all_five_functions(built, kind):
    rows = random_lists(kind, 5000, 7)
    assert any(r and len([v for v in r if v is not None]) > len({v for v in r if v is not None}) for r in rows), "no list with a duplicate"
    assert any(r and r.count(None) >= 2 for r in rows), "no list with two NULLs"
    assert [] in rows and None in rows and [None, None] in rows
    dom = KINDS[kind][2]
    rng = random.Random(8)
    keys = [None if rng.random() < 0.05 else rng.choice(dom) for _ in rows]
    t = pa.table({"l": lists(kind, rows), "k": scalars(kind, keys)})
    ty = KINDS[kind][0]
    l, k = S.col(0, LT(kind)), S.col(1, ty)
    sorts = sort4(l)
    exprs = [e for e, _, _ in sorts] + [S.array_distinct(l), S.array_position(l, S.lit(dom[-1], ty))]
    if kind != "str":
        exprs += [S.array_min(l), S.array_max(l), S.array_position(l, k)]
    plan = S.project(S.scan([LT(kind), ty]), exprs)
    ok, msg = native.check_plan(plan.encode())
    assert ok, msg
    got = run(plan, t, len(exprs))
    for j, (_, asc, nl) in enumerate(sorts):
        assert plain_lists(kind, got.column(j)) == [M.sort_array(r, asc, nl) for r in rows], (asc, nl)
    assert plain_lists(kind, got.column(4)) == [M.array_distinct(r) for r in rows]
    assert got.column(5).type == pa.int64() and got.column(5).to_pylist() == [M.array_position(r, dom[-1]) for r in rows]
    if kind != "str":
        assert got.column(6).type == KINDS[kind][1] and plain(kind, got.column(6).combine_chunks()) == [M.array_min(r) for r in rows]
        assert plain(kind, got.column(7).combine_chunks()) == [M.array_max(r) for r in rows]
        assert got.column(8).to_pylist() == [M.array_position(r, key) for r, key in zip(rows, keys)]


def boundary_rows(kind, lengths):
    """lists of exactly the given lengths (and a NULL list between them), values from the small domain with NULLs"""
    rng = random.Random(11)
    dom = KINDS[kind][2]
    rows = []
    for n in lengths:
        rows.append([None if rng.random() < 0.05 else rng.choice(dom) for _ in range(n)])
        rows.append(None)
    # … and one of distinct values in descending order: every element moves
    if kind == "i64":
        rows.append(list(range(max(lengths), 0, -1)))
    return rows


@pytest.mark.parametrize("long_lists", [False, True])
@pytest.mark.parametrize("kind", ["i64", "str", "dec38_0"])
def test_list_length_boundaries(built, kind, long_lists):
    """up to CAP elements every list is ranked; one list beyond CAP sends the whole column through the radix sort"""
    rows = boundary_rows(kind, (0, 1, 2, 63, 64, 65, CAP - 1, CAP) + ((CAP + 1, 5000) if long_lists else ()))
    t = pa.table({"l": lists(kind, rows)})
    l = S.col(0, LT(kind))
    plan = S.project(S.scan([LT(kind)]), [S.sort_array(l), S.sort_array(l, False), S.array_distinct(l)])
    got, m = run_metrics(plan, t, 3)
    assert plain_lists(kind, got.column(0)) == [M.sort_array(r) for r in rows]
    assert plain_lists(kind, got.column(1)) == [M.sort_array(r, False) for r in rows]
    assert plain_lists(kind, got.column(2)) == [M.array_distinct(r) for r in rows]
    # every list of the three derived columns went the route its column's longest list decides
    assert m.get("list_fn_sort_lists", 0) == (3 * len(rows) if long_lists else 0) and m.get("list_fn_rank_lists", 0) == (0 if long_lists else 3 * len(rows)), m


def test_the_sort_operators_key_limit_comes_with_the_sort_route(built):
    """a Utf8 value beyond the Sort operator's 1000-byte key in a column with an over-long list fails with that operator's message; the scalar functions have no limit"""
    t = pa.table({"l": lists("str", [["b", "a"], ["x" * 1200] + [str(i % 10) for i in range(CAP + 1)], []])})
    l = S.col(0, LT("str"))
    for e in (S.sort_array(l), S.array_distinct(l)):
        with pytest.raises(native.CometNativeException, match="Sort key wider than 1000 bytes"):
            run(S.project(S.scan([LT("str")]), [e]), t, 1)
    n = CAP + 2
    got = run(S.project(S.scan([LT("str")]), [S.array_position(l, S.lit("x" * 1200, STR)), S.scalar_func("size", [l], I32)]), t, 2)
    assert got.column(0).to_pylist() == [0, 1, 0] and got.column(1).to_pylist() == [2, n, 0]


def test_no_metric_without_a_list_function(built):
    t = pa.table({"l": lists("i64", [[1], None])})
    _, m = run_metrics(S.project(S.scan([LT("i64")]), [S.scalar_func("size", [S.col(0, LT("i64"))], I32)]), t, 1)
    assert "list_fn_rank_lists" not in m, m


def test_same_bits_on_every_route_and_batch_size(built, monkeypatch):
    rows = random_lists("str", 3000, 21, max_len=64)
    assert max(len(r) for r in rows if r) > 32
    irows = random_lists("i64", 3000, 22, max_len=64)
    t = pa.table({"l": lists("str", rows), "i": lists("i64", irows)})
    ls, li = S.col(0, LT("str")), S.col(1, LT("i64"))
    plan = S.project(S.scan([LT("str"), LT("i64")]), [S.sort_array(ls), S.array_distinct(ls), S.sort_array(li, False), S.array_distinct(li)])
    seen = []
    for tier in (None, "rank", "sort"):
        if tier:
            monkeypatch.setenv("COMET_LIST_FN_TIER", tier)
        for batch_size, batch_rows in ((0, 8192), (7, 8192), (0, 7) if tier is None else (7, 1000)):
            got = run(plan, t, 4, batch_size=batch_size, batch_rows=batch_rows).combine_chunks()
            seen.append([got.column(j).chunk(0).to_pylist() for j in range(4)])
    assert all(s == seen[0] for s in seen[1:])
    assert seen[0][0] == [M.sort_array(r) for r in rows] and seen[0][3] == [M.array_distinct(r) for r in irows]
    # the forced routes show in the metrics
    _, m = run_metrics(plan, t, 4)
    assert m.get("list_fn_sort_lists") == 4 * len(rows) and "list_fn_rank_lists" not in m, m
    monkeypatch.setenv("COMET_LIST_FN_TIER", "rank")
    _, m = run_metrics(plan, t, 4)
    assert m.get("list_fn_rank_lists") == 4 * len(rows) and "list_fn_sort_lists" not in m, m


def composition_table(n=4000, seed=31):
    rng = np.random.default_rng(seed)
    li, ls = random_lists("i64", n, seed), random_lists("str", n, seed + 1)
    s = [None if rng.random() < 0.05 else ["b,a,c", "x", "", "k=v,x,,a", "two,one,two"][int(rng.integers(0, 5))] for _ in range(n)]
    k = [None if rng.random() < 0.05 else int(rng.choice(KINDS["i64"][2])) for _ in range(n)]
    return pa.table({"li": lists("i64", li), "ls": lists("str", ls), "s": pa.array(s, pa.utf8()), "k": pa.array(k, pa.int64())}), li, ls, s, k


COMP_TYPES = [S.list_type(I64, True), S.list_type(STR, True), STR, I64]


def test_composition(built):
    t, li_rows, ls_rows, s_rows, k_rows = composition_table()
    li, ls, s, k = (S.col(i, ty) for i, ty in enumerate(COMP_TYPES))
    L = lambda v: S.lit(v, I32)
    sp = S.scalar_func("split", [s, S.lit(",", STR), S.lit(-1, I32)], S.list_type(STR, False))
    exprs = [S.sort_array(sp), S.array_distinct(S.sort_array(li)), S.scalar_func("size", [S.array_distinct(li)], I32), S.list_extract(S.sort_array(ls), L(0)),
             S.list_extract(S.sort_array(li), L(-1), one_based=True), S.array_max(S.array_distinct(li)), S.scalar_func("array_contains", [S.sort_array(li), S.lit(3, I64)], S.T_BOOL),
             S.array_distinct(sp), S.sort_array(S.array_distinct(sp), False)]
    plan = S.project(S.scan(COMP_TYPES), exprs)
    # two equal calls in one chain share one derived column: split, sort(split), sort(li), distinct(sort(li)), distinct(li), sort(ls), distinct(split), sort(distinct(split))
    assert native.plan_codegen(plan.encode(), [True] * 4)["derived"] == 8
    got = run(plan, t, len(exprs))
    split = [None if v is None else v.split(",") for v in s_rows]
    first = lambda r: None if not r else r[0]
    assert plain_lists("str", got.column(0)) == [M.sort_array(r) for r in split]
    assert plain_lists("i64", got.column(1)) == [M.array_distinct(M.sort_array(r)) for r in li_rows]
    assert got.column(2).to_pylist() == [-1 if r is None else len(M.array_distinct(r)) for r in li_rows]
    assert got.column(3).to_pylist() == [first(M.sort_array(r)) for r in ls_rows]
    assert got.column(4).to_pylist() == [None if not r else M.sort_array(r)[-1] for r in li_rows]
    assert got.column(5).to_pylist() == [M.array_max(r) for r in li_rows]
    contains = lambda r: None if r is None else True if 3 in r else None if None in r else False
    assert got.column(6).to_pylist() == [contains(r) for r in li_rows]
    assert plain_lists("str", got.column(7)) == [M.array_distinct(r) for r in split]
    assert plain_lists("str", got.column(8)) == [M.sort_array(M.array_distinct(r), False) for r in split]
    # explode of a sorted list
    ex = S.explode(S.project(S.scan(COMP_TYPES), [S.sort_array(li), k]), S.col(0, COMP_TYPES[0]), [S.col(1, I64)])
    got = run(ex, t, 2)
    want = [(key, v) for r, key in zip(li_rows, k_rows) for v in (M.sort_array(r) or [])]
    assert list(zip(got.column(0).to_pylist(), got.column(1).to_pylist())) == want
    # a Filter below that reads array_position(li, k) > 0 with a column key
    flt = S.project(S.filter_(S.scan(COMP_TYPES), S.gt(S.array_position(li, k), S.lit(0, I64))), [S.sort_array(li), k])
    got = run(flt, t, 2)
    keep = [i for i in range(t.num_rows) if (M.array_position(li_rows[i], k_rows[i]) or 0) > 0]
    assert 0 < len(keep) < t.num_rows
    assert plain_lists("i64", got.column(0)) == [M.sort_array(li_rows[i]) for i in keep] and got.column(1).to_pylist() == [k_rows[i] for i in keep]


def test_over_a_collect_aggregate_in_one_plan(built):
    rng = random.Random(41)
    n = 6000
    g = [rng.randrange(0, 300) for _ in range(n)]
    v = [None if rng.random() < 0.1 else rng.randrange(-20, 20) for _ in range(n)]
    t = pa.table({"g": pa.array(g, pa.int32()), "v": pa.array(v, pa.int64())})
    LV = S.list_type(I64, False)
    agg = S.hash_agg(S.scan([I32, I64]), [S.col(0, I32)], [S.collect_list(S.col(1, I64), I64), S.collect_set(S.col(1, I64), I64)])
    plan = S.project(agg, [S.col(0, I32), S.sort_array(S.col(1, LV), False), S.array_min(S.col(1, LV)), S.sort_array(S.col(2, LV)), S.array_distinct(S.col(1, LV)), S.col(1, LV)])
    got = run(plan, t, 6)
    groups = {}
    for key, val in zip(g, v):
        groups.setdefault(key, [])
        if val is not None:
            groups[key].append(val)
    keys = got.column(0).to_pylist()
    assert sorted(keys) == sorted(groups)
    assert plain_lists("i64", got.column(5)) == [groups[key] for key in keys]
    assert plain_lists("i64", got.column(1)) == [M.sort_array(groups[key], False) for key in keys]
    assert got.column(2).to_pylist() == [M.array_min(groups[key]) for key in keys]
    assert plain_lists("i64", got.column(3)) == [sorted(set(groups[key])) for key in keys]
    assert plain_lists("i64", got.column(4)) == [M.array_distinct(groups[key]) for key in keys]


def test_below_a_hash_join(built):
    """a join's side that projects a list function is not fused into the join's kernels (the fold refuses a derived list there): the side is materialised first"""
    t, li_rows, _, _, _ = composition_table(2000, 61)
    other = pa.table({"k": pa.array([0, 1, 2, 3, 3], pa.int32())})
    li = S.col(0, COMP_TYPES[0])
    size = lambda x: S.scalar_func("size", [x], I32)
    side = S.project(S.scan(COMP_TYPES), [size(S.array_distinct(li)), S.list_extract(S.sort_array(li), S.lit(0, I32))])
    want = [(k, len(M.array_distinct(r)), M.sort_array(r)[0] if r else None) for r in li_rows if r is not None for k in (0, 1, 2, 3, 3) if k == len(M.array_distinct(r))]
    key = lambda r: (r[0], r[1], -2 ** 70 if r[2] is None else r[2])
    for build_side in (S.BUILD_LEFT, S.BUILD_RIGHT):
        plan = S.hash_join(S.scan([I32]), side, [S.col(0, I32)], [S.col(0, I32)], S.INNER, build_side)
        out = native.execute_to_table([native.HostInput.from_table(other), native.HostInput.from_table(t)], 3, plan.encode(), batch_size=0)
        got = pa.Table.from_batches(out)
        rows = list(zip(got.column(0).to_pylist(), got.column(1).to_pylist(), got.column(2).to_pylist()))
        assert sorted(rows, key=key) == sorted(want, key=key) and len(rows) > 100


def test_a_sliced_host_table_is_rebased_by_the_scan_leaf(built):
    """rows [100, 100 + n) of a longer host table, NULL lists among them: the list column arrives at the Scan leaf with an Arrow offset and element offsets that
    do not start at 0.  The leaf rebases both when it uploads the batch, so the list functions see an unsliced column — what every producer of a list column in
    the engine delivers; a sliced DEVICE column would be refused by name, and nothing delivers one (DeviceTable inputs carry no lists)."""
    rows = random_lists("i64", 3150, 51)
    srows = random_lists("str", 3150, 52)
    t = pa.table({"l": lists("i64", rows), "s": lists("str", srows)}).slice(100, 3000)
    assert t.column(0).chunk(0).offset == 100 and t.column(0).chunk(0).offsets[0].as_py() > 0 and t.column(0).null_count > 0
    l, s = S.col(0, LT("i64")), S.col(1, LT("str"))
    got = run(S.project(S.scan([LT("i64"), LT("str")]), [S.sort_array(l), S.array_distinct(l), S.array_distinct(s), S.sort_array(s, False)]), t, 4)
    rows, srows = rows[100:3100], srows[100:3100]
    assert plain_lists("i64", got.column(0)) == [M.sort_array(r) for r in rows]
    assert plain_lists("i64", got.column(1)) == [M.array_distinct(r) for r in rows]
    assert plain_lists("str", got.column(2)) == [M.array_distinct(r) for r in srows]
    assert plain_lists("str", got.column(3)) == [M.sort_array(r, False) for r in srows]


def test_a_long_utf8_value(built):
    """a value far beyond the Sort operator's 1000-byte key limit sorts like any other: ties of the 8-byte prefix are decided on the bytes"""
    big = "p" * 1200
    rows = [[big + "b", "z", None, big + "a", big, "a"], [big, big]] + [[big + str(i % 7) for i in range(200)]]
    t = pa.table({"l": lists("str", rows)})
    l = S.col(0, LT("str"))
    got = run(S.project(S.scan([LT("str")]), [S.sort_array(l), S.array_distinct(l)]), t, 2)
    assert plain_lists("str", got.column(0)) == [M.sort_array(r) for r in rows]
    assert plain_lists("str", got.column(1)) == [M.array_distinct(r) for r in rows]
