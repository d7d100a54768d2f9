"""array_union, array_intersect, array_except and arrays_overlap on the GPU, through the C ABI against the pure-Python model of tests/list_set_model.py (pinned
by tests/test_list_set_cpu.py).  Tables, values and helpers are those of tests/test_list_fn_gpu.py.

Shapes: 5 000 rows of two list columns of 0 to 6 elements from a small domain, run in several batches; and one table whose lists have exactly 0, 1, 2, 63, 64,
65, 255, 256, 257 and 5 000 elements on either side — 256 is the rank tier's edge in the distinct and the sort underneath.  More than one 256-lane block in both."""
import random

import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S
from tests import list_fn_model as LM
from tests import list_set_model as M
from tests.test_list_fn_gpu import CAP, KINDS, LT, lists, plain_lists, random_lists, run, run_metrics

pytestmark = pytest.mark.gpu
I32, I64, STR = S.T_INT32, S.T_INT64, S.T_STRING
FOUR = [S.array_union, S.array_intersect, S.array_except, S.arrays_overlap]


def size(x):
    return S.scalar_func("size", [x], I32)


def accepted(plan):
    ok, msg = native.check_plan(plan.encode())
    assert ok, msg


def check_four(kind, got, rows_a, rows_b, first=0):
    pairs = list(zip(rows_a, rows_b))
    assert plain_lists(kind, got.column(first)) == [M.array_union(a, b) for a, b in pairs]
    assert plain_lists(kind, got.column(first + 1)) == [M.array_intersect(a, b) for a, b in pairs]
    assert plain_lists(kind, got.column(first + 2)) == [M.array_except(a, b) for a, b in pairs]
    assert got.column(first + 3).type == pa.bool_() and got.column(first + 3).to_pylist() == [M.arrays_overlap(a, b) for a, b in pairs]


@pytest.mark.parametrize("kind", list(KINDS))
def test_all_four_functions(built, kind):
    rows_a, rows_b = random_lists(kind, 5000, 11), random_lists(kind, 5000, 12)
    pairs = list(zip(rows_a, rows_b))
    # no class of answer is missing from the inputs (the model says so before anything runs)
    overlap = [M.arrays_overlap(a, b) for a, b in pairs]
    inter = [(a, b, M.array_intersect(a, b)) for a, b in pairs if a is not None and b is not None]
    classes = {
        "overlap true": sum(o is True for o in overlap), "overlap false": sum(o is False for o in overlap),
        "overlap NULL from NULL elements": sum(o is None and a is not None and b is not None for o, (a, b) in zip(overlap, pairs)),
        "overlap NULL from a NULL list": sum(a is None or b is None for a, b in pairs),
        "an intersection of two or more that is not in value order": sum(len(r) >= 2 and r != LM.sort_array(r) for _, _, r in inter),
        "… whose left list is the shorter one, where an engine that orders by the longer side reads the other list's order": sum(len(r) >= 2 and len(a) < len(b) for a, b, r in inter),
        "an except that drops some but not all": sum(0 < len(M.array_except(a, b)) < len(LM.array_distinct(a)) for a, b, _ in inter),
        "a union longer than distinct(a)": sum(len(M.array_union(a, b)) > len(LM.array_distinct(a)) for a, b, _ in inter),
    }
    assert all(n >= 100 for n in classes.values()), classes
    t = pa.table({"a": lists(kind, rows_a), "b": lists(kind, rows_b)})
    a, b = S.col(0, LT(kind)), S.col(1, LT(kind))
    plan = S.project(S.scan([LT(kind), LT(kind)]), [fn(a, b) for fn in FOUR])
    accepted(plan)
    got = run(plan, t, 4, batch_rows=1000)      # five batches
    check_four(kind, got, rows_a, rows_b)


LENGTHS = (0, 1, 2, 63, 64, 65, CAP - 1, CAP, CAP + 1, 5000)


def boundary_pairs(kind):
    """every length of LENGTHS on either side, beside a short (2) and a long (300) partner; values with duplicates inside a list, shared between the sides, and NULLs"""
    rng = random.Random(13)

    def one(n):
        span = max(3, (3 * n) // 4)      # about a quarter of a long list's elements repeat an earlier one
        vals = [None if rng.random() < 0.05 else rng.randrange(span) for _ in range(n)]
        if kind == "str":
            vals = [None if v is None else ("shared prefix, longer than eight bytes: %d" % v if v % 3 else "w%d" % v) for v in vals]
        return vals
    rows_a, rows_b = [], []
    for n in LENGTHS:
        for partner in (2, 300):
            rows_a += [one(n), one(partner)]
            rows_b += [one(partner), one(n)]
    rows_a += [None, one(70), one(CAP + 1)]
    rows_b += [one(CAP + 1), None, one(CAP + 1)]
    return rows_a, rows_b


_BOUNDARY = {}


def boundary_table(kind):
    if kind not in _BOUNDARY:
        rows_a, rows_b = boundary_pairs(kind)
        _BOUNDARY[kind] = (pa.table({"a": lists(kind, rows_a), "b": lists(kind, rows_b)}), rows_a, rows_b)
    return _BOUNDARY[kind]


@pytest.mark.parametrize("tier", [None, "rank", "sort"])
@pytest.mark.parametrize("kind", ["i64", "str"])
def test_list_length_boundaries(built, monkeypatch, kind, tier):
    t, rows_a, rows_b = boundary_table(kind)
    assert {len(r) for r in rows_a if r is not None} >= set(LENGTHS) and {len(r) for r in rows_b if r is not None} >= set(LENGTHS)
    assert any(r and None in r for r in rows_a) and any(r and len(r) > len(LM.array_distinct(r)) > CAP for r in rows_a)
    if tier:
        monkeypatch.setenv("COMET_LIST_FN_TIER", tier)
    a, b = S.col(0, LT(kind)), S.col(1, LT(kind))
    plan = S.project(S.scan([LT(kind), LT(kind)]), [fn(a, b) for fn in FOUR])
    accepted(plan)
    got, m = run_metrics(plan, t, 4)
    check_four(kind, got, rows_a, rows_b)
    assert m.get("list_set_rows") == 4 * len(rows_a), m
    # the distinct and the sort underneath went the route the tier forces, or the one their column's longest list decides
    if tier:
        assert ("list_fn_sort_lists" if tier == "rank" else "list_fn_rank_lists") not in m, m


def test_no_metric_without_a_set_function(built):
    t = pa.table({"l": lists("i64", [[1], None])})
    _, m = run_metrics(S.project(S.scan([LT("i64")]), [S.array_distinct(S.col(0, LT("i64")))]), t, 1)
    assert "list_set_rows" not in m, m


def consumer_table(n=4000, seed=71, plain_a=False):
    rng = random.Random(seed)
    rows_a, rows_b = random_lists("i64", n, seed), random_lists("i64", n, seed + 1)
    if plain_a:      # no NULL list and no NULL element on this side: the column arrives without validity bitmaps
        rows_a = [[v for v in r if v is not None] for r in rows_a if r is not None]
        rows_a = (rows_a * 2)[:n]
    k = [None if rng.random() < 0.05 else rng.choice(KINDS["i64"][2]) for _ in range(n)]
    return pa.table({"a": lists("i64", rows_a), "b": lists("i64", rows_b), "k": pa.array(k, pa.int64())}), rows_a, rows_b, k


TYPES = [S.list_type(I64, True), S.list_type(I64, True), I64]
A, B, K = (S.col(i, ty) for i, ty in enumerate(TYPES))


def contains(r, key):
    return None if r is None else True if key in r else None if None in r else False


def test_consumers_and_compositions(built):
    t, rows_a, rows_b, keys = consumer_table()
    pairs = list(zip(rows_a, rows_b))
    exprs = [size(S.array_union(A, B)), S.scalar_func("array_contains", [S.array_except(A, B), S.lit(3, I64)], S.T_BOOL), S.array_intersect(A, A),
             S.array_except(S.array_union(A, B), S.array_intersect(A, B)), S.arrays_overlap(S.array_except(A, B), B), S.sort_array(S.array_intersect(B, A), False)]
    plan = S.project(S.scan(TYPES), exprs)
    accepted(plan)
    got = run(plan, t, len(exprs), batch_rows=1500)
    union = [M.array_union(a, b) for a, b in pairs]
    assert got.column(0).to_pylist() == [-1 if u is None else len(u) for u in union]
    assert got.column(1).to_pylist() == [contains(M.array_except(a, b), 3) for a, b in pairs]
    assert plain_lists("i64", got.column(2)) == [LM.array_distinct(a) for a in rows_a]
    assert plain_lists("i64", got.column(3)) == [M.array_except(M.array_union(a, b), M.array_intersect(a, b)) for a, b in pairs]
    want = [M.arrays_overlap(M.array_except(a, b), b) for a, b in pairs]
    assert got.column(4).to_pylist() == want and True not in want and False in want and sum(w is None for w in want) > 500
    assert plain_lists("i64", got.column(5)) == [LM.sort_array(M.array_intersect(b, a), False) for a, b in pairs]


def test_explode_of_an_intersection_and_a_filter_on_the_overlap(built):
    t, rows_a, rows_b, keys = consumer_table()
    pairs = list(zip(rows_a, rows_b))
    ex = S.explode(S.project(S.scan(TYPES), [S.array_intersect(A, B), K]), S.col(0, TYPES[0]), [S.col(1, I64)])
    accepted(ex)
    got = run(ex, t, 2)
    want = [(key, v) for (a, b), key in zip(pairs, keys) for v in (M.array_intersect(a, b) or [])]
    assert len(want) > 1000 and list(zip(got.column(0).to_pylist(), got.column(1).to_pylist())) == want
    # a Filter on arrays_overlap(a, b): NULL drops the row as false does
    flt = S.project(S.filter_(S.scan(TYPES), S.arrays_overlap(A, B)), [S.array_union(A, B), K, S.arrays_overlap(B, A)])
    accepted(flt)
    got = run(flt, t, 3)
    keep = [i for i, (a, b) in enumerate(pairs) if M.arrays_overlap(a, b) is True]
    assert 100 < len(keep) < t.num_rows - 100 and sum(M.arrays_overlap(a, b) is None for a, b in pairs) > 100
    assert plain_lists("i64", got.column(0)) == [M.array_union(*pairs[i]) for i in keep]
    assert got.column(1).to_pylist() == [keys[i] for i in keep] and got.column(2).to_pylist() == [True] * len(keep)


def test_below_a_hash_join_and_inside_an_aggregates_chain(built):
    """a join's side that projects a set function is not fused into the join's kernels: the side is materialised first and the answers are those of the Projection
    alone; inside an aggregate's fused chain the functions are refused by name"""
    t, rows_a, rows_b, _ = consumer_table(2000, 81)
    other = pa.table({"k": pa.array([0, 1, 2, 3, 3], pa.int32())})
    side = S.project(S.scan(TYPES), [size(S.array_union(A, B)), size(S.array_intersect(A, B)), S.arrays_overlap(A, B)])
    alone = run(side, t, 3)
    rows = list(zip(alone.column(0).to_pylist(), alone.column(1).to_pylist(), alone.column(2).to_pylist()))
    assert rows == [(-1, -1, None) if a is None or b is None else (len(M.array_union(a, b)), len(M.array_intersect(a, b)), M.arrays_overlap(a, b)) for a, b in zip(rows_a, rows_b)]
    want = [(k,) + r for r in rows for k in (0, 1, 2, 3, 3) if k == r[0]]
    key = lambda r: (r[0], r[1], r[2], {None: 0, False: 1, True: 2}[r[3]])
    for build_side in (S.BUILD_LEFT, S.BUILD_RIGHT):
        plan = S.hash_join(S.scan([I32]), side, [S.col(0, I32)], [S.col(0, I32)], S.INNER, build_side)
        accepted(plan)
        out = native.execute_to_table([native.HostInput.from_table(other), native.HostInput.from_table(t)], 4, plan.encode(), batch_size=0)
        got = pa.Table.from_batches(out)
        joined = list(zip(*(got.column(j).to_pylist() for j in range(4))))
        assert sorted(joined, key=key) == sorted(want, key=key) and len(joined) > 100
    for name, fn in (("array_union", S.array_union), ("array_intersect", S.array_intersect), ("array_except", S.array_except)):
        ok, msg = native.check_plan(S.hash_agg(S.project(S.scan(TYPES), [size(fn(A, B))]), [], [S.sum_(S.col(0, I32), I64)]).encode())
        assert not ok and name in msg and "project it below the aggregate" in msg, msg
    ok, msg = native.check_plan(S.hash_agg(S.project(S.scan(TYPES), [S.if_(S.arrays_overlap(A, B), S.lit(1, I32), S.lit(0, I32))]), [], [S.sum_(S.col(0, I32), I64)]).encode())
    assert not ok and "spark_arrays_overlap" in msg and "project it below the aggregate" in msg, msg


@pytest.mark.parametrize("plain_side", [0, 1])
def test_one_side_without_validity_bitmaps(built, plain_side):
    t, rows_a, rows_b, _ = consumer_table(3000, 91, plain_a=True)
    assert t.column(0).null_count == 0 and t.column(0).chunk(0).values.null_count == 0 and t.column(1).null_count > 0
    x, y = (A, B) if plain_side == 0 else (B, A)
    rx, ry = (rows_a, rows_b) if plain_side == 0 else (rows_b, rows_a)
    plan = S.project(S.scan(TYPES), [fn(x, y) for fn in FOUR])
    accepted(plan)
    got = run(plan, t, 4, batch_rows=1024)
    check_four("i64", got, rx, ry)
    assert any(u and None in u for u in (M.array_union(p, q) for p, q in zip(rx, ry)))      # NULL elements reach the union from the one side that has a bitmap
