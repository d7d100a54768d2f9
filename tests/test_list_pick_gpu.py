"""array_remove, array_compact, slice, reverse of an array and array_join on the GPU, through the C ABI against the pure-Python model of
tests/list_pick_model.py (pinned by tests/test_list_pick_cpu.py).  Tables, values and helpers are those of tests/test_list_fn_gpu.py.

Shapes: 5 000 lists of 0 to 6 elements from a small domain, run in five batches; and one table whose lists have exactly 0, 1, 2, 63, 64, 65, 255, 256, 257
and 5 000 elements — every kernel has one lane per element and no length tier, so 256 is only the width of a block here.  More than one 256-lane block in both.
Before this feature createPlan refused every plan of this file by the function's name."""
import random

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S
from tests import list_fn_model as LM
from tests import list_pick_model as M
from tests.test_list_fn_gpu import KINDS, LT, lists, plain_lists, random_lists, run, run_metrics, scalars

pytestmark = pytest.mark.gpu
I32, I64, STR = S.T_INT32, S.T_INT64, S.T_STRING


def size(x):
    return S.scalar_func("size", [x], I32)


def accepted(plan):
    ok, msg = native.check_plan(plan.encode())
    assert ok, msg


_RANDOM = {}


def random_table(kind):
    """the 5 000 lists and the key column of test_all_five_functions, made once per kind"""
    if kind not in _RANDOM:
        rows = random_lists(kind, 5000, 21)
        rng = random.Random(22)
        dom = KINDS[kind][2]
        keys = [None if rng.random() < 0.05 else rng.choice(dom) for _ in rows]
        _RANDOM[kind] = (pa.table({"l": lists(kind, rows), "k": scalars(kind, keys)}), rows, keys)
    return _RANDOM[kind]


def answer_classes(kind, rows, keys):
    """how often every class of answer occurs in the inputs, by the model"""
    lit = KINDS[kind][2][-1]
    some = [r for r in rows if r is not None]
    removed = [(r, M.array_remove(r, lit)) for r in some]
    compacted = [(r, M.array_compact(r)) for r in some]
    c = {
        "remove drops some but not all elements": sum(0 < len(o) < len(r) for r, o in removed),
        "remove drops all": sum(len(r) > 0 and not o for r, o in removed),
        "remove drops none of a non-empty list": sum(len(r) > 0 and o == r for r, o in removed),
        "a NULL element is kept beside a removed value": sum(None in o and len(o) < len(r) for r, o in removed),
        "compact drops some but not all": sum(0 < len(o) < len(r) for r, o in compacted),
        "compact drops all": sum(len(r) > 0 and not o for r, o in compacted),
        "slice is clamped": sum(1 < len(r) < 4 for r in some),                       # slice(2, 3) asks for more than stands behind its start
        "slice is full": sum(len(r) >= 4 for r in some),
        "slice's start is past the end": sum(0 < len(r) < 2 for r in some),           # slice(2, 3)
        "slice's negative start is before the beginning": sum(len(r) < 3 for r in some),      # slice(-3, 2)
        "a reverse that is not a palindrome": sum(r != r[::-1] for r in some),
        "NULL lists": sum(r is None for r in rows),
        "empty lists": sum(r == [] for r in rows),
    }
    if kind != "str":
        c["a NULL key beside a non-NULL list"] = sum(k is None and r is not None for r, k in zip(rows, keys))
    else:
        c["join skips a leading NULL"] = sum(len(r) > 1 and r[0] is None and any(v is not None for v in r) for r in some)
        c["join skips an inner or trailing NULL"] = sum(any(v is None for v in r[1:]) and r[0] is not None for r in some)
        c["join of all-NULL elements gives the empty string"] = sum(len(r) > 0 and all(v is None for v in r) for r in some)
    return c


@pytest.mark.parametrize("kind", list(KINDS))
def test_all_five_functions(built, kind):
    t, rows, keys = random_table(kind)
    classes = answer_classes(kind, rows, keys)
    assert all(n >= 40 for n in classes.values()), classes
    ty = KINDS[kind][0]
    lit = KINDS[kind][2][-1]
    l, k = S.col(0, LT(kind)), S.col(1, ty)
    exprs = [S.array_remove(l, S.lit(lit, ty)), S.array_compact(l), S.array_slice(l, 2, 3), S.array_slice(l, -3, 2), S.array_reverse(l)]
    want = [[M.array_remove(r, lit) for r in rows], [M.array_compact(r) for r in rows], [M.slice_(r, 2, 3) for r in rows], [M.slice_(r, -3, 2) for r in rows],
            [M.array_reverse(r) for r in rows]]
    if kind != "str":
        exprs.append(S.array_remove(l, k))
        want.append([M.array_remove(r, key) for r, key in zip(rows, keys)])
    else:
        exprs += [S.array_join(l, ","), S.array_join(l, ", ", "NULL")]
    plan = S.project(S.scan([LT(kind), ty]), exprs)
    accepted(plan)
    got = run(plan, t, len(exprs), batch_rows=1000)      # five batches
    for j, w in enumerate(want):
        assert plain_lists(kind, got.column(j)) == w, j
    if kind == "str":
        assert got.column(5).type == pa.utf8() and got.column(5).to_pylist() == [M.array_join(r, ",") for r in rows]
        assert got.column(6).to_pylist() == [M.array_join(r, ", ", "NULL") for r in rows]


LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 5000)
_BOUNDARY = {}


def boundary_table(kind):
    """one list of every length of LENGTHS, a NULL list and a second long list behind them; duplicates and NULL elements inside"""
    if kind not in _BOUNDARY:
        rng = random.Random(23)

        def one(n):
            vals = [None if rng.random() < 0.1 else rng.randrange(max(3, n // 4)) for _ in range(n)]
            if kind == "str":
                vals = [None if v is None else ("shared prefix, longer than eight bytes: %d" % v if v % 3 else "w%d" % v) for v in vals]
            return vals
        rows = [one(n) for n in LENGTHS] + [None, one(300)]
        _BOUNDARY[kind] = (pa.table({"l": lists(kind, rows)}), rows)
    return _BOUNDARY[kind]


@pytest.mark.parametrize("kind", ["i64", "str"])
def test_list_length_boundaries(built, kind):
    t, rows = boundary_table(kind)
    assert [len(r) for r in rows[:len(LENGTHS)]] == list(LENGTHS) and sum(len(r or []) for r in rows) > 2 * 256
    ty = KINDS[kind][0]
    key = rows[-1][0] if rows[-1][0] is not None else rows[-1][1]
    l = S.col(0, LT(kind))
    slices = [(1, 1), (-1, 1), (257, 10)]
    exprs = [S.array_remove(l, S.lit(key, ty)), S.array_compact(l), S.array_reverse(l)] + [S.array_slice(l, s, n) for s, n in slices]
    want = [[M.array_remove(r, key) for r in rows], [M.array_compact(r) for r in rows], [M.array_reverse(r) for r in rows]] + [[M.slice_(r, s, n) for r in rows] for s, n in slices]
    assert any(w and len(w) < len(r) for w, r in zip(want[0], rows) if r) and [len(w) for w in want[5] if w is not None].count(10) >= 1
    if kind == "str":
        exprs += [S.array_join(l, ","), S.array_join(l, ", ", "NULL")]
    plan = S.project(S.scan([LT(kind)]), exprs)
    accepted(plan)
    got, m = run_metrics(plan, t, len(exprs))
    for j, w in enumerate(want):
        assert plain_lists(kind, got.column(j)) == w, j
    if kind == "str":
        assert got.column(6).to_pylist() == [M.array_join(r, ",") for r in rows]
        assert got.column(7).to_pylist() == [M.array_join(r, ", ", "NULL") for r in rows]
    assert m.get("list_pick_rows") == len(exprs) * len(rows), m
    # slices that name the list's own length: (n, 1) is its last element, (-n, n) the whole list — for the list of n elements, and whatever Spark says for the others
    for n in LENGTHS[1:]:
        plan = S.project(S.scan([LT(kind)]), [S.array_slice(l, n, 1), S.array_slice(l, -n, n)])
        got = run(plan, t, 2)
        assert plain_lists(kind, got.column(0)) == [M.slice_(r, n, 1) for r in rows], n
        assert plain_lists(kind, got.column(1)) == [M.slice_(r, -n, n) for r in rows], n
        i = LENGTHS.index(n)
        assert plain_lists(kind, got.column(0))[i] == rows[i][-1:] and plain_lists(kind, got.column(1))[i] == rows[i]


def test_a_join_that_may_exceed_2_gib_fails_by_name_before_any_launch(built):
    """element bytes + elements x (|delimiter| + |replacement|) reaching 2 GiB fails the task by name; the bound needs no 2 GiB of data — the 5 000-element list and
    delimiters of a few hundred KB reach it.  The refused task counted no rows and launched nothing; a short delimiter over the same table runs"""
    t, rows = boundary_table("str")
    col = t.column(0).combine_chunks()
    elements, nbytes = len(col.values), sum(len(v.encode()) for r in rows if r for v in r if v is not None)
    per = (2 ** 31 - nbytes + elements - 1) // elements      # the least delimiter + replacement length that reaches the bound
    assert nbytes + elements * per >= 2 ** 31 > nbytes + elements * (per - 1) and per < 2 ** 20
    l = S.col(0, LT("str"))

    def failing(plan):
        it = native.CometExecIterator([native.HostInput.from_table(t)], 1, plan.encode(), batch_size=0)
        try:
            with pytest.raises(Exception) as err:
                native.Native.executePlan(it.handle, 1)
            m = S.decode_metric_node(it.metrics())[0]
        finally:
            it.close()
        return str(err.value), m
    for d, r in (("d" * per, None), ("d" * (per // 2), "r" * (per - per // 2))):
        msg, m = failing(S.project(S.scan([LT("str")]), [S.array_join(l, d, r)]))
        assert "array_to_string" in msg and "2 GiB" in msg, msg
        assert "list_pick_rows" not in m, m      # refused from the two offsets the host reads: no kernel of the column was launched
    got = run(S.project(S.scan([LT("str")]), [S.array_join(l, "d" * 7, "r")]), t, 1)
    assert got.column(0).to_pylist() == [M.array_join(r, "d" * 7, "r") for r in rows]


def test_no_metric_without_a_pick_function(built):
    t = pa.table({"l": lists("i64", [[1], None])})
    _, m = run_metrics(S.project(S.scan([LT("i64")]), [S.array_distinct(S.col(0, LT("i64")))]), t, 1)
    assert "list_pick_rows" not in m, m


def f64_bits(col):
    """a list<double> column → per list the elements' raw 64-bit patterns (None: a NULL element)"""
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    assert col.type == pa.list_(pa.float64()), col.type
    vals = col.values
    bits = np.frombuffer(vals.buffers()[1], dtype=np.uint64, count=len(vals) + vals.offset)[vals.offset:].tolist() if len(vals) else []
    ok, offs, lv = vals.is_valid().to_pylist(), col.offsets.to_pylist(), col.is_valid().to_pylist()
    flat = [b if v else None for b, v in zip(bits, ok)]
    return [flat[offs[r]:offs[r + 1]] if lv[r] else None for r in range(len(col))]


def test_float_lists_are_moved_bit_for_bit(built):
    """slice, array_compact and reverse never compare an element: NaN payloads, both zeros and the infinities come out as they went in"""
    special = [0x0000000000000000, 0x8000000000000000, 0x7ff8000000000000, 0xfff8000000000001, 0x7ff0000000000001, 0x7ff4dead0000beef, 0x7ff0000000000000, 0xfff0000000000000,
               0x3ff0000000000000, 0x0000000000000001]
    rng = random.Random(24)
    rows = [[], None, [None, None], [special[1], None, special[3]]]
    while len(rows) < 1500:
        rows.append(None if rng.random() < 0.08 else [None if rng.random() < 0.15 else rng.choice(special) for _ in range(rng.randrange(0, 7))])
    flat, offs, mask = [], [0], []
    for r in rows:
        flat.extend(r or [])
        offs.append(len(flat))
        mask.append(r is None)
    values = pa.array(np.array([0 if v is None else v for v in flat], dtype=np.uint64).view(np.float64), mask=np.array([v is None for v in flat]))
    col = pa.ListArray.from_arrays(pa.array(offs, pa.int32()), values, mask=pa.array(mask, pa.bool_()))
    t = pa.table({"l": col})
    assert f64_bits(t.column(0)) == rows      # the table holds the patterns
    lt = S.list_type(S.T_DOUBLE, True)
    l = S.col(0, lt)
    plan = S.project(S.scan([lt]), [S.array_slice(l, 2, 3), S.array_compact(l), S.array_reverse(l), S.array_slice(l, -2, 5)])
    accepted(plan)
    got = run(plan, t, 4, batch_rows=512)
    assert f64_bits(got.column(0)) == [M.slice_(r, 2, 3) for r in rows]
    assert f64_bits(got.column(1)) == [M.array_compact(r) for r in rows]
    assert f64_bits(got.column(2)) == [M.array_reverse(r) for r in rows]
    assert f64_bits(got.column(3)) == [M.slice_(r, -2, 5) for r in rows]
    kept = [b for r in f64_bits(got.column(2)) if r for b in r if b is not None]
    assert {0x8000000000000000, 0xfff8000000000001, 0x7ff4dead0000beef} <= set(kept)


def chain_table(n=4000, seed=51):
    rng = random.Random(seed)
    li, ls = random_lists("i64", n, seed), random_lists("str", n, seed + 1)
    s = [None if rng.random() < 0.05 else rng.choice(["b,a,c", "x", "", "k=v,x,,a", "two,one,two", "b,a", "a,b"]) for _ in range(n)]
    k = [None if rng.random() < 0.05 else rng.choice(KINDS["i64"][2]) for _ in range(n)]
    return pa.table({"li": lists("i64", li), "ls": lists("str", ls), "s": pa.array(s, pa.utf8()), "k": pa.array(k, pa.int64())}), li, ls, s, k


TYPES = [S.list_type(I64, True), S.list_type(STR, True), STR, I64]
LI, LS, SS, K = (S.col(i, ty) for i, ty in enumerate(TYPES))
SPLIT = S.scalar_func("split", [SS, S.lit(",", STR), S.lit(-1, I32)], S.list_type(STR, False))


def contains(r, key):
    return None if r is None else True if key in r else None if None in r else False


def test_consumers_and_compositions(built):
    t, li, ls, s, k = chain_table()
    split = [None if v is None else v.split(",") for v in s]
    exprs = [S.array_join(S.sort_array(SPLIT), ","), size(S.array_slice(LI, 2, 3)), S.list_extract(S.array_remove(LI, S.lit(3, I64)), S.lit(1, I32), one_based=True),
             S.scalar_func("array_contains", [S.array_compact(LI), S.lit(3, I64)], S.T_BOOL), S.array_slice(S.array_distinct(LI), 1, 2, I64),
             S.scalar_func("length", [S.array_join(LS, ",")], I32), S.array_reverse(S.array_compact(LS)), S.array_remove(LI, K)]
    halves = [S.project(S.scan(TYPES), exprs[:4]), S.project(S.scan(TYPES), exprs[4:])]      # (all eight at once need more than a pipeline's 24 column slots)
    for plan in halves:
        accepted(plan)
    got = run(halves[0], t, 4, batch_rows=1500)
    for j, col in enumerate(run(halves[1], t, 4, batch_rows=1500).columns):
        got = got.append_column("c%d" % (4 + j), col)
    assert got.column(0).to_pylist() == [M.array_join(LM.sort_array(r), ",") for r in split]
    assert got.column(1).to_pylist() == [-1 if r is None else len(M.slice_(r, 2, 3)) for r in li]
    assert got.column(2).to_pylist() == [None if not M.array_remove(r, 3) else M.array_remove(r, 3)[0] for r in li]
    assert got.column(3).to_pylist() == [contains(M.array_compact(r), 3) for r in li]
    assert plain_lists("i64", got.column(4)) == [M.slice_(LM.array_distinct(r), 1, 2) for r in li]
    # (length counts characters)
    assert got.column(5).to_pylist() == [None if r is None else len(M.array_join(r, ",")) for r in ls]
    assert plain_lists("str", got.column(6)) == [M.array_reverse(M.array_compact(r)) for r in ls]
    assert plain_lists("i64", got.column(7)) == [M.array_remove(r, key) for r, key in zip(li, k)]


def test_explode_and_filters(built):
    t, li, ls, s, k = chain_table()
    ex = S.explode(S.project(S.scan(TYPES), [S.array_slice(LI, 2, 3), K]), S.col(0, TYPES[0]), [S.col(1, I64)])
    accepted(ex)
    got = run(ex, t, 2)
    want = [(key, v) for r, key in zip(li, k) for v in (M.slice_(r, 2, 3) or [])]
    assert len(want) > 1000 and list(zip(got.column(0).to_pylist(), got.column(1).to_pylist())) == want
    # an array_join result as an operand of a Filter: = 'a,b'
    joined = S.array_join(S.sort_array(SPLIT), ",")
    flt = S.project(S.filter_(S.scan(TYPES), S.eq(joined, S.lit("a,b", STR))), [SS, joined, S.array_reverse(LI)])
    accepted(flt)
    got = run(flt, t, 3)
    keep = [i for i, v in enumerate(s) if v in ("b,a", "a,b")]
    assert 100 < len(keep) < t.num_rows - 100 and {s[i] for i in keep} == {"b,a", "a,b"}
    assert got.column(0).to_pylist() == [s[i] for i in keep] and got.column(1).to_pylist() == ["a,b"] * len(keep)
    assert plain_lists("i64", got.column(2)) == [M.array_reverse(li[i]) for i in keep]
    # array_remove(x, k) below a Filter of the same chain that drops rows: the derived column is computed over the source, the chain gathers the kept rows
    flt = S.project(S.filter_(S.scan(TYPES), S.gt(K, S.lit(0, I64))), [S.array_remove(LI, K), K, size(S.array_remove(LI, K))])
    accepted(flt)
    got = run(flt, t, 3, batch_rows=1024)
    keep = [i for i, key in enumerate(k) if key is not None and key > 0]
    assert 100 < len(keep) < t.num_rows - 100
    assert plain_lists("i64", got.column(0)) == [M.array_remove(li[i], k[i]) for i in keep] and got.column(1).to_pylist() == [k[i] for i in keep]
    assert got.column(2).to_pylist() == [-1 if li[i] is None else len(M.array_remove(li[i], k[i])) for i in keep]


def test_over_a_final_collect_aggregate_in_one_plan(built):
    rng = random.Random(61)
    n = 3000
    keys = [rng.randrange(0, 200) for _ in range(n)]
    states = [[rng.randrange(-3, 4) for _ in range(rng.randrange(0, 5))] for _ in range(n)]
    lt = pa.list_(pa.int64())
    t = pa.table({"k": pa.array(keys, pa.int32()), "s": pa.array(states, lt)})
    LV = S.list_type(I64, False)
    agg = S.hash_agg(S.scan([I32, S.list_type(I64, True)]), [S.col(0, I32)], [S.collect_list(S.col(1, I64), I64)], S.FINAL)
    plan = S.project(agg, [S.col(0, I32), S.array_remove(S.col(1, LV), S.lit(3, I64)), S.array_slice(S.col(1, LV), -2, 2, I64), S.col(1, LV)])
    accepted(plan)
    got = run(plan, t, 4)
    groups = {}
    for key, st in zip(keys, states):
        groups.setdefault(key, []).extend(st)
    out_keys = got.column(0).to_pylist()
    assert sorted(out_keys) == sorted(groups)
    assert plain_lists("i64", got.column(3)) == [groups[key] for key in out_keys]
    assert plain_lists("i64", got.column(1)) == [M.array_remove(groups[key], 3) for key in out_keys]
    assert plain_lists("i64", got.column(2)) == [M.slice_(groups[key], -2, 2) for key in out_keys]
    assert any(3 in groups[key] for key in out_keys)


def test_below_a_hash_join_and_inside_an_aggregates_chain(built):
    """a join's side that projects one of the functions is not fused into the join's kernels: the side is materialised first and the answers are those of the
    Projection alone; inside an aggregate's fused chain the functions are refused by name"""
    t, li, ls, s, k = chain_table(2000, 71)
    other = pa.table({"k": pa.array([0, 1, 2, 3, 3], pa.int32())})
    length = lambda x: S.scalar_func("length", [x], I32)
    side = S.project(S.scan(TYPES), [size(S.array_remove(LI, S.lit(3, I64))), size(S.array_compact(LI)), length(S.array_join(LS, ","))])
    alone = run(side, t, 3)
    rows = list(zip(alone.column(0).to_pylist(), alone.column(1).to_pylist(), alone.column(2).to_pylist()))
    assert rows == [(-1 if a is None else len(M.array_remove(a, 3)), -1 if a is None else len(M.array_compact(a)), None if b is None else len(M.array_join(b, ","))) for a, b in zip(li, ls)]
    want = [(key,) + r for r in rows for key in (0, 1, 2, 3, 3) if key == r[0]]
    order = lambda r: (r[0], r[1], r[2], -1 if r[3] is None else r[3])
    for build_side in (S.BUILD_LEFT, S.BUILD_RIGHT):
        plan = S.hash_join(S.scan([I32]), side, [S.col(0, I32)], [S.col(0, I32)], S.INNER, build_side)
        accepted(plan)
        out = native.execute_to_table([native.HostInput.from_table(other), native.HostInput.from_table(t)], 4, plan.encode(), batch_size=0)
        got = pa.Table.from_batches(out)
        joined = list(zip(*(got.column(j).to_pylist() for j in range(4))))
        assert sorted(joined, key=order) == sorted(want, key=order) and len(joined) > 100
    inside = {"array_remove_all": size(S.array_remove(LI, S.lit(3, I64))), "array_compact": size(S.array_compact(LI)), "spark_array_slice": size(S.array_slice(LI, 2, 3)),
              "array_reverse": size(S.array_reverse(LI)), "array_to_string": length(S.array_join(LS, ","))}
    for name, e in inside.items():
        ok, msg = native.check_plan(S.hash_agg(S.project(S.scan(TYPES), [e]), [], [S.sum_(S.col(0, I32), I64)]).encode())
        assert not ok and name in msg and "project it below the aggregate" in msg, msg
