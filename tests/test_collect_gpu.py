"""collect_list / collect_set in HashAggregate on the GPU: Partial / PartialMerge / Final, grouped and not, through the C ABI against the pure-Python model of
tests/collect_model.py (pinned by tests/test_collect_cpu.py).  A collect_list is compared IN ORDER (arrival order: batches in the order pulled, rows in batch
order; merging: state rows in input order, each list in its own order), a collect_set as a set that must come without duplicates and ascending; groups are
compared as a mapping from their key values.  Values travel as plain integers / strings (dates as days, timestamps as microseconds, decimals unscaled).

Row counts: 0, 1, 2, 255 / 257 (one block of the streaming kernels), 4096 / 4097 (the one-workgroup sort ends at 4096 rows) and 20 011 (the radix path, and
some twenty 1024-row scan tiles).  5000 groups are more than one workgroup's threads, most of them of size 1 to 4."""
import decimal
import functools
import random

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S
from tests import collect_model as M

pytestmark = pytest.mark.gpu
I32, I64, STR = S.T_INT32, S.T_INT64, S.T_STRING
N = 20_011
D38 = 10 ** 38 - 1

# kind → (serde type, Arrow type)
KINDS = {
    "bool": (S.T_BOOL, pa.bool_()), "i8": (S.T_INT8, pa.int8()), "i16": (S.T_INT16, pa.int16()), "i32": (S.T_INT32, pa.int32()), "i64": (S.T_INT64, pa.int64()),
    "date": (S.T_DATE, pa.date32()), "ts": (S.T_TIMESTAMP, pa.timestamp("us", tz="UTC")), "ntz": (S.DataType(S.TIMESTAMP_NTZ), pa.timestamp("us")),
    "dec10_2": (S.decimal(10, 2), pa.decimal128(10, 2)), "dec38_0": (S.decimal(38, 0), pa.decimal128(38, 0)), "str": (S.T_STRING, pa.utf8()),
    "f32": (S.T_FLOAT, pa.float32()), "f64": (S.T_DOUBLE, pa.float64()),
}
SET_KINDS = [k for k in KINDS if k not in ("f32", "f64")]


def run(plan, tables, ncols, batch_rows=8192):
    ins = [native.HostInput.from_table(t, batch_rows) for t in tables]
    out = native.execute_to_table(ins, ncols, plan.encode(), batch_size=0)
    return pa.Table.from_batches(out) if out else None


def column(kind, values):
    """model values (None = NULL) → an Arrow column of the kind; floats are given as their bit patterns and keep every bit"""
    t = KINDS[kind][1]
    mask = np.array([v is None for v in values], dtype=bool)
    m = mask if mask.any() else None
    if kind in ("bool", "str"):
        return pa.array(values, t)
    if kind in ("f32", "f64"):
        u = np.array([0 if v is None else v for v in values], dtype=np.uint32 if kind == "f32" else np.uint64)
        return pa.array(u.view(np.float32 if kind == "f32" else np.float64), t, mask=m)
    if kind.startswith("dec"):
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            return pa.array([None if v is None else decimal.Decimal(v).scaleb(-t.scale) for v in values], t)
    base = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "date": np.int32, "ts": np.int64, "ntz": np.int64}[kind]
    a = pa.array(np.array([0 if v is None else v for v in values], dtype=base), mask=m)
    return a.cast(t)


def plain(kind, flat):
    """an Arrow array of the kind → model values"""
    if kind in ("bool", "str"):
        return flat.to_pylist()
    if kind in ("f32", "f64"):
        a = flat.to_numpy(zero_copy_only=False)
        return [int(x) for x in a.view(np.uint32 if kind == "f32" else np.uint64)]
    if kind.startswith("dec"):
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            return [None if d is None else int(d.scaleb(flat.type.scale)) for d in flat.to_pylist()]
    if kind == "date":
        return flat.cast(pa.int32()).to_pylist()
    if kind in ("ts", "ntz"):
        return flat.cast(pa.int64()).to_pylist()
    return flat.to_pylist()


def lists_of(t, j, kind):
    """column j of a result — a List<kind> that is never NULL and holds no NULL, its element field nullable — as one Python list per row"""
    f = t.schema.field(j)
    assert pa.types.is_list(f.type) and f.type.value_type == KINDS[kind][1] and f.type.value_field.nullable, f
    col = t.column(j).combine_chunks()
    assert col.null_count == 0      # an empty group has an empty list, never NULL
    flat = col.flatten()
    assert flat.null_count == 0
    vals = plain(kind, flat)
    offs = (np.asarray(col.offsets) - col.offsets[0].as_py()).tolist()
    return [vals[offs[r]:offs[r + 1]] for r in range(len(col))]


def rows_of(t, nkeys, kinds):
    """result table → key tuple → per aggregate its list; the keys must be distinct"""
    if t is None:
        return {}
    keys = [t.column(i).to_pylist() for i in range(nkeys)]
    aggs = [lists_of(t, nkeys + j, kinds[j]) for j in range(len(kinds))]
    out = {}
    for r in range(t.num_rows):
        k = tuple(c[r] for c in keys)
        assert k not in out, f"group {k} twice"
        out[k] = [a[r] for a in aggs]
    return out


def check(t, nkeys, kinds, want):
    """want[j]: key → a list (collect_list: equal in order) or a set (collect_set: equal as a set, no duplicates, ascending)"""
    got = rows_of(t, nkeys, kinds)
    assert set(got) == set(want[0]), (len(got), len(want[0]))
    for k, lists in got.items():
        for j, lst in enumerate(lists):
            w = want[j][k]
            if isinstance(w, (set, frozenset)):
                assert len(lst) == len(set(lst)), (k, j, "duplicates")
                assert set(lst) == w, (k, j, len(lst), len(w))
                assert lst == sorted(lst), (k, j, "not ascending")
            else:
                assert lst == w, (k, j, len(lst), len(w))


def partial_plan(key_types, other_types, aggs):
    fields = list(key_types) + list(other_types)
    return S.hash_agg(S.scan(fields), [S.col(i, t) for i, t in enumerate(key_types)], aggs, S.PARTIAL)


def merge_plan(key_types, elem_types, aggs, mode):
    fields = list(key_types) + [S.list_type(t, True) for t in elem_types]
    return S.hash_agg(S.scan(fields), [S.col(i, t) for i, t in enumerate(key_types)], aggs, mode)


def values_of(kind, rng, n):
    """n values with many duplicates and the type's extremes, a third of them NULL"""
    if kind == "bool":
        dom = [False, True]
    elif kind == "i8":
        dom = [-128, 127, 0] + list(range(-5, 6))
    elif kind == "i16":
        dom = [-32768, 32767, 0] + list(range(-300, 300, 7))
    elif kind in ("i32", "date"):
        dom = [-2**31, 2**31 - 1, 0, 19723] + [rng.randrange(-10**6, 10**6) for _ in range(200)]
    elif kind in ("i64", "ts", "ntz"):
        dom = [-2**63, 2**63 - 1, 0, 1704067200000000] + [rng.randrange(-10**15, 10**15) for _ in range(200)]
    elif kind == "dec10_2":
        dom = [-9999999999, 9999999999, 0, 150] + [rng.randrange(-10**9, 10**9) for _ in range(200)]
    elif kind == "dec38_0":
        dom = [-D38, D38, 0, 2**64, -2**64, 2**64 - 1] + [rng.randrange(-10**37, 10**37) for _ in range(200)]      # (values that differ only in their high or low word)
    elif kind == "str":
        dom = ["", "a", "ab", "ab\0", "abé", "a value longer than fifteen bytes", "x" * 300, "zz"] + ["s%d" % rng.randrange(100) for _ in range(100)]
    elif kind == "f32":
        dom = [0x7FC00001, 0xFFC00000, 0x80000000, 0x00000000, 0x3F800000, 0x7F800000, 0xFF800000, 0x00000001] + [rng.randrange(2**32) for _ in range(50)]
    else:
        dom = [0xFFF8000000000001, 0x7FF8000000000000, 0x8000000000000000, 0, 0x3FF0000000000000, 0x7FF0000000000000, 1] + [rng.randrange(2**64) for _ in range(50)]
    return [None if rng.random() < 1 / 3 else dom[rng.randrange(len(dom))] for _ in range(n)]


def int_keys(ngroups, n=N, null_every=17):
    rng = random.Random(ngroups)
    return [(None if i % null_every == 3 else rng.randrange(ngroups) - ngroups // 2,) for i in range(n)]


@functools.lru_cache(maxsize=None)
def int_data():
    rng = random.Random(20261020)
    return values_of("i64", rng, N)


# --------------------------------------------------------------------------- Partial: every element type

@pytest.mark.parametrize("kind", list(KINDS))
def test_partial_state_of_every_element_type(built, kind):
    rng = random.Random(sorted(KINDS).index(kind))
    x = values_of(kind, rng, N)
    keys = int_keys(5000)
    present = sorted({k for k in keys if k[0] is not None})
    for i, k in enumerate(keys):
        if k == present[0]:
            x[i] = None      # a group whose values are all NULL
    st = et = KINDS[kind][0]
    both = kind in SET_KINDS
    aggs = [S.collect_list(S.col(1, st), et)] + ([S.collect_set(S.col(1, st), et)] if both else [])
    table = pa.table({"k": pa.array([k[0] for k in keys], pa.int32()), "x": column(kind, x)})
    want = [M.collect_list(keys, x)] + ([M.collect_set(keys, x)] if both else [])
    assert want[0][present[0]] == [] and (None,) in want[0]
    got = run(partial_plan([I32], [st], aggs), [table], 1 + len(aggs), 1000)
    check(got, 1, [kind] * len(aggs), want)


# --------------------------------------------------------------------------- row counts, ungrouped and grouped; Partial → Final

@pytest.mark.parametrize("n", [0, 1, 2, 255, 257, 4096, 4097, N])
def test_ungrouped_partial_and_final_at_every_row_count(built, n):
    x = int_data()[:n]
    aggs = [S.collect_list(S.col(0, I64), I64), S.collect_set(S.col(0, I64), I64)]
    want = [M.collect_list([()] * n, x, ungrouped=True), M.collect_set([()] * n, x, ungrouped=True)]
    table = pa.table({"x": column("i64", x)})
    st = run(partial_plan([], [I64], aggs), [table], 2, 1000)
    assert st is not None and st.num_rows == 1      # no keys: one group, whatever the row count — over zero rows one row holding []
    check(st, 0, ["i64", "i64"], want)
    fin = run(merge_plan([], [I64, I64], aggs, S.FINAL), [st], 2)      # (at N: ONE list of every kept value, spread over the grid)
    assert fin is not None and fin.num_rows == 1
    check(fin, 0, ["i64", "i64"], want)
    if n == 0:
        assert rows_of(fin, 0, ["i64", "i64"]) == {(): [[], []]}
        # … and a Final over no state rows at all
        none = run(merge_plan([], [I64, I64], aggs, S.FINAL), [st.slice(0, 0)], 2)
        assert rows_of(none, 0, ["i64", "i64"]) == {(): [[], []]}


@pytest.mark.parametrize("n", [0, 1, 2, 255, 257, 4096, 4097, N])
def test_four_groups_partial_and_final_at_every_row_count_in_stable_order(built, n):
    """the values of the list are the row numbers, so any reordering inside a group shows; 4096 / 4097 rows: both sides of the switch from the one-workgroup
    sort (ties broken by row) to the radix passes (stable partitions)"""
    keys = int_keys(4, n)
    x = [None if i % 7 == 2 else i for i in range(n)]
    y = [None if v is None else v % 7 for v in int_data()[:n]]      # heavy duplicates for the set
    aggs = [S.collect_list(S.col(1, I64), I64), S.collect_set(S.col(2, I64), I64)]
    want = [M.collect_list(keys, x), M.collect_set(keys, y)]
    table = pa.table({"k": pa.array([k[0] for k in keys], pa.int32()), "x": column("i64", x), "y": column("i64", y)})
    st = run(partial_plan([I32], [I64, I64], aggs), [table], 3, 1000)
    if n == 0:
        assert st is None or st.num_rows == 0
        return
    check(st, 1, ["i64", "i64"], want)
    for k, (lst, _) in rows_of(st, 1, ["i64", "i64"]).items():
        assert lst == sorted(lst), k      # arrival order = ascending row numbers
    fin = run(merge_plan([I32], [I64, I64], aggs, S.FINAL), [st], 3)
    check(fin, 1, ["i64", "i64"], want)


# --------------------------------------------------------------------------- empty lists

def test_final_over_hand_made_states_with_null_and_empty_lists(built):
    lt = pa.list_(pa.int64())
    k = [1, 1, 2, 2, None, 3, 3, 1, 4]
    s = [[3, None, 1], None, [], None, [None, 9], None, None, [1, 8], [None]]
    aggs = [S.collect_list(S.col(1, I64), I64), S.collect_set(S.col(1, I64), I64)]
    table = pa.table({"k": pa.array(k, pa.int32()), "s0": pa.array(s, lt), "s1": pa.array(s, lt)})
    rows = [((kk,), ss) for kk, ss in zip(k, s)]
    want = [M.merge_list(rows), M.merge_set(rows)]
    assert want[0] == {(1,): [3, 1, 1, 8], (2,): [], (None,): [9], (3,): [], (4,): []}
    for mode in (S.FINAL, S.PARTIAL_MERGE):
        check(run(merge_plan([I32], [I64, I64], aggs, mode), [table], 3), 1, ["i64", "i64"], want)
    # ungrouped: nothing but NULL / empty states, and lists without a single element anywhere → one row holding []
    for states in ([None, [], [None]], [None, [], None], [[]]):
        empty = pa.table({"s0": pa.array(states, lt), "s1": pa.array(states, lt)})
        for mode in (S.FINAL, S.PARTIAL_MERGE):
            got = run(merge_plan([], [I64, I64], aggs, mode), [empty], 2)
            assert rows_of(got, 0, ["i64", "i64"]) == {(): [[], []]}
    # the same for Utf8 elements
    slt = pa.list_(pa.utf8())
    saggs = [S.collect_list(S.col(0, STR), STR), S.collect_set(S.col(0, STR), STR)]
    empty = pa.table({"s0": pa.array([None, []], slt), "s1": pa.array([None, []], slt)})
    assert rows_of(run(merge_plan([], [STR, STR], saggs, S.FINAL), [empty], 2), 0, ["str", "str"]) == {(): [[], []]}


def test_groups_with_only_nulls_and_one_key_for_every_row(built):
    n = 5000
    x = int_data()[:n]
    aggs = [S.collect_list(S.col(1, I64), I64), S.collect_set(S.col(1, I64), I64)]
    for vals in (x, [None] * n):      # one group and no NULL key: no byte plane of the key varies
        table = pa.table({"k": pa.array([42] * n, pa.int32()), "x": column("i64", vals)})
        want = [M.collect_list([(42,)] * n, vals), M.collect_set([(42,)] * n, vals)]
        st = run(partial_plan([I32], [I64], aggs), [table], 3, 1000)
        assert st.num_rows == 1
        check(st, 1, ["i64", "i64"], want)
        check(run(merge_plan([I32], [I64, I64], aggs, S.FINAL), [st], 3), 1, ["i64", "i64"], want)


# --------------------------------------------------------------------------- the set's duplicates

def test_set_with_heavy_duplicates_and_equal_values_across_group_boundaries(built):
    """values drawn from 7 distinct ones; group g holds {2g + 1, 2g + 2, 2g + 3}, so a group's greatest value is the next group's least: after the sort the
    last row of one group and the first row of the next hold equal VALUE bytes, and only the key tells them apart"""
    rng = random.Random(3)
    keys, x = [], []
    for _ in range(N):
        g = rng.randrange(3)
        keys.append((g,))
        x.append(None if rng.random() < 0.1 else 2 * g + 1 + rng.randrange(3))
    aggs = [S.collect_set(S.col(1, I64), I64)]
    want = [M.collect_set(keys, x)]
    assert want[0] == {(0,): {1, 2, 3}, (1,): {3, 4, 5}, (2,): {5, 6, 7}}
    table = pa.table({"k": pa.array([k[0] for k in keys], pa.int32()), "x": column("i64", x)})
    st = run(partial_plan([I32], [I64], aggs), [table], 2, 1000)
    check(st, 1, ["i64"], want)
    # without keys the same values are one set
    un = run(partial_plan([], [I32, I64], aggs), [table], 1)
    check(un, 0, ["i64"], [{(): set(range(1, 8))}])
    # 257 rows, one value each in two groups: every row but two is a duplicate
    small = pa.table({"k": pa.array([i % 2 for i in range(257)], pa.int32()), "x": column("i64", [5] * 257)})
    check(run(partial_plan([I32], [I64], aggs), [small], 2), 1, ["i64"], [{(0,): {5}, (1,): {5}}])


# --------------------------------------------------------------------------- Partial → (PartialMerge →) Final

def test_partial_then_final_and_partial_merge(built):
    x = int_data()
    y = [None if v is None else v % 11 for v in x]
    keys = int_keys(300)
    aggs = [S.collect_list(S.col(1, I64), I64), S.collect_set(S.col(2, I64), I64)]
    kinds = ["i64", "i64"]
    cuts = ((0, 9000, 1000), (9000, N, 8192))      # two Partial runs over the halves, with different batch_rows
    states = []
    for a, b, batch_rows in cuts:
        t = pa.table({"k": pa.array([k[0] for k in keys[a:b]], pa.int32()), "x": column("i64", x[a:b]), "y": column("i64", y[a:b])})
        st = run(partial_plan([I32], [I64, I64], aggs), [t], 3, batch_rows)
        check(st, 1, kinds, [M.collect_list(keys[a:b], x[a:b]), M.collect_set(keys[a:b], y[a:b])])
        states.append(st)
    both = pa.concat_tables(states).combine_chunks()
    # the list: the first state's elements, then the second's — which is the arrival order of the whole; the set: de-duplicated ACROSS the states
    want = [M.collect_list(keys, x), M.collect_set(keys, y)]
    fin = run(merge_plan([I32], [I64, I64], aggs, S.FINAL), [both], 3, 1000)
    check(fin, 1, kinds, want)
    merged = run(merge_plan([I32], [I64, I64], aggs, S.PARTIAL_MERGE), [both], 3)
    check(merged, 1, kinds, want)
    assert merged.num_rows == len(want[0]) < both.num_rows
    check(run(merge_plan([I32], [I64, I64], aggs, S.FINAL), [merged], 3), 1, kinds, want)


# --------------------------------------------------------------------------- determinism

def test_the_same_bytes_at_two_batch_sizes(built):
    x = int_data()
    keys = int_keys(5000)
    aggs = [S.collect_list(S.col(1, I64), I64), S.collect_set(S.col(1, I64), I64)]
    table = pa.table({"k": pa.array([k[0] for k in keys], pa.int32()), "x": column("i64", x)})
    seen = []
    for batch_rows in (1000, 8192):
        st = run(partial_plan([I32], [I64], aggs), [table], 3, batch_rows).combine_chunks()
        fin = run(merge_plan([I32], [I64, I64], aggs, S.FINAL), [st], 3, batch_rows).combine_chunks()
        seen.append([(t.column(0).to_pylist(), [(np.asarray(t.column(j).chunk(0).offsets).tobytes(), np.asarray(t.column(j).chunk(0).flatten()).tobytes()) for j in (1, 2)])
                     for t in (st, fin)])
    assert seen[0] == seen[1]


# --------------------------------------------------------------------------- FILTER

def test_filter_in_partial_with_a_group_it_empties(built):
    x = list(int_data())
    rng = random.Random(9)
    flag = [None if rng.random() < 0.1 else rng.randint(0, 1) for _ in range(N)]
    keys = int_keys(7)
    present = sorted({k for k in keys if k[0] is not None})
    emptied = present[-1]
    for i, k in enumerate(keys):
        if k == emptied:
            flag[i] = 0 if i % 2 else None      # a group that only the FILTER empties: FALSE and NULL both reject
            x[i] = 5 if x[i] is None else x[i]
    flt = S.eq(S.col(2, I32), S.lit(1, I32))
    keep = [f == 1 for f in flag]
    aggs = [S.collect_list(S.col(1, I64), I64, filter=flt), S.collect_set(S.col(1, I64), I64, filter=flt), S.collect_list(S.col(1, I64), I64)]
    want = [M.collect_list(keys, x, keep), M.collect_set(keys, x, keep), M.collect_list(keys, x)]
    assert want[0][emptied] == [] and want[2][emptied]
    table = pa.table({"k": pa.array([k[0] for k in keys], pa.int32()), "x": column("i64", x), "f": pa.array(flag, pa.int32())})
    st = run(partial_plan([I32], [I64, I32], aggs), [table], 4, 1000)
    check(st, 1, ["i64"] * 3, want)
    # a Utf8 element under a FILTER, ungrouped
    s = [None if v is None else "v%d" % (v % 50) for v in x]
    saggs = [S.collect_list(S.col(0, STR), STR, filter=S.eq(S.col(1, I32), S.lit(1, I32))), S.collect_set(S.col(0, STR), STR, filter=S.eq(S.col(1, I32), S.lit(1, I32)))]
    stable = pa.table({"s": pa.array(s, pa.utf8()), "f": pa.array(flag, pa.int32())})
    un = run(partial_plan([], [STR, I32], saggs), [stable], 2, 1000)
    check(un, 0, ["str", "str"], [M.collect_list([()] * N, s, keep, ungrouped=True), M.collect_set([()] * N, s, keep, ungrouped=True)])


# --------------------------------------------------------------------------- mixed functions, Utf8 and two-column keys

def test_list_and_set_of_one_child_and_a_filtered_list_of_another_under_utf8_and_two_column_keys(built):
    x = int_data()
    a = [None if v is None else v % 13 for v in x]
    rng = random.Random(7)
    b = [None if i % 5 == 0 else "b%d" % rng.randrange(40) for i in range(N)]
    names = ["", "a", "ab", "abé", "a much longer key than fifteen bytes", None, "zz"]
    k1 = [names[rng.randrange(len(names))] for _ in range(N)]
    k2 = [None if i % 11 == 0 else rng.randrange(3) for i in range(N)]
    keep = [v is not None and v > 5 for v in a]
    kinds = ["i64", "i64", "str"]
    for nk, keys, ktypes, kcols in ((1, [(k,) for k in k1], [STR], {"k1": pa.array(k1, pa.utf8())}),
                                    (2, list(zip(k1, k2)), [STR, I32], {"k1": pa.array(k1, pa.utf8()), "k2": pa.array(k2, pa.int32())})):
        ca, cb = nk, nk + 1
        f = S.gt(S.col(ca, I64), S.lit(5, I64))
        aggs = [S.collect_list(S.col(ca, I64), I64), S.collect_set(S.col(ca, I64), I64), S.collect_list(S.col(cb, STR), STR, filter=f)]
        want = [M.collect_list(keys, a), M.collect_set(keys, a), M.collect_list(keys, b, keep)]
        table = pa.table({**kcols, "a": column("i64", a), "b": pa.array(b, pa.utf8())})
        st = run(partial_plan(ktypes, [I64, STR], aggs), [table], nk + 3, 1000)      # three sorts; the groups line up
        check(st, nk, kinds, want)
        fin = run(merge_plan(ktypes, [I64, I64, STR], aggs, S.FINAL), [st], nk + 3)
        check(fin, nk, kinds, want)


# --------------------------------------------------------------------------- Utf8 elements

def test_utf8_elements_empty_long_and_equal_up_to_a_trailing_nul(built):
    long = "€" * 100      # 300 bytes
    vals = ["", long, "ab", "ab\0", "ab\0\0", None, "ab", "", long, "a", "ab\0", None]
    keys = [(i % 2,) for i in range(len(vals))]
    aggs = [S.collect_list(S.col(1, STR), STR), S.collect_set(S.col(1, STR), STR)]
    table = pa.table({"k": pa.array([k[0] for k in keys], pa.int32()), "s": pa.array(vals, pa.utf8())})
    want = [M.collect_list(keys, vals), M.collect_set(keys, vals)]
    st = run(partial_plan([I32], [STR], aggs), [table], 3)
    check(st, 1, ["str", "str"], want)
    got = rows_of(st, 1, ["str", "str"])
    assert got[(0,)][1] == ["", "ab", "ab\0", "ab\0\0", long]      # padded bytes, then the length: "ab" < "ab\0" < "ab\0\0"
    check(run(merge_plan([I32], [STR, STR], aggs, S.FINAL), [st], 3), 1, ["str", "str"], want)


def test_collect_set_of_an_utf8_value_beyond_the_sort_key_limit_fails_with_the_sort_operators_message(built):
    vals = ["short", "y" * 1200, None]
    table = pa.table({"s": pa.array(vals, pa.utf8())})
    # the list takes it: it sorts by nothing here
    got = run(partial_plan([], [STR], [S.collect_list(S.col(0, STR), STR)]), [table], 1)
    check(got, 0, ["str"], [{(): ["short", "y" * 1200]}])
    with pytest.raises(Exception, match="Sort key wider than 1000 bytes"):
        run(partial_plan([], [STR], [S.collect_set(S.col(0, STR), STR)]), [table], 1)


# --------------------------------------------------------------------------- floats, bit for bit

def test_float_lists_keep_nan_payloads_and_negative_zero(built):
    f64 = [0xFFF8000000000001, 0x8000000000000000, 0, None, 0x7FF8000000000000, 0x7FF0000000000001, 0x3FF0000000000000, 0x8000000000000000, 0xFFF8000000000001]
    f32 = [0xFFC00001, 0x80000000, 0, None, 0x7FC00000, 0x7F800001, 0x3F800000, 0x80000000, 0xFFC00001]
    keys = [(i % 2,) for i in range(len(f64))]
    aggs = [S.collect_list(S.col(1, S.T_DOUBLE), S.T_DOUBLE), S.collect_list(S.col(2, S.T_FLOAT), S.T_FLOAT)]
    table = pa.table({"k": pa.array([k[0] for k in keys], pa.int32()), "d": column("f64", f64), "f": column("f32", f32)})
    want = [M.collect_list(keys, f64), M.collect_list(keys, f32)]
    st = run(partial_plan([I32], [S.T_DOUBLE, S.T_FLOAT], aggs), [table], 3)
    check(st, 1, ["f64", "f32"], want)
    assert rows_of(st, 1, ["f64", "f32"])[(0,)][0] == [0xFFF8000000000001, 0, 0x7FF8000000000000, 0x3FF0000000000000, 0xFFF8000000000001]
    fin = run(merge_plan([I32], [S.T_DOUBLE, S.T_FLOAT], aggs, S.FINAL), [st], 3)
    check(fin, 1, ["f64", "f32"], want)
    un = run(partial_plan([], [I32, S.T_DOUBLE, S.T_FLOAT], aggs), [table], 2)
    check(un, 0, ["f64", "f32"], [M.collect_list([()] * len(f64), f64), M.collect_list([()] * len(f32), f32)])


# --------------------------------------------------------------------------- extremes

def test_int32_int64_and_decimal38_extremes(built):
    i32 = [2**31 - 1, -2**31, 0, None, -1, 2**31 - 1, -2**31]
    i64 = [2**63 - 1, -2**63, 0, None, -1, 2**63 - 1, -2**63]
    d38 = [D38, -D38, 0, None, 2**64, 2**64 - 1, -2**64, D38, -D38, -1]
    for kind, vals in (("i32", i32), ("i64", i64), ("dec38_0", d38)):
        st_t = KINDS[kind][0]
        keys = [(i % 2,) for i in range(len(vals))]
        aggs = [S.collect_list(S.col(1, st_t), st_t), S.collect_set(S.col(1, st_t), st_t)]
        table = pa.table({"k": pa.array([k[0] for k in keys], pa.int32()), "x": column(kind, vals)})
        want = [M.collect_list(keys, vals), M.collect_set(keys, vals)]
        st = run(partial_plan([I32], [st_t], aggs), [table], 3)
        check(st, 1, [kind, kind], want)
        check(run(merge_plan([I32], [st_t, st_t], aggs, S.FINAL), [st], 3), 1, [kind, kind], want)
        un = run(partial_plan([], [I32, st_t], aggs), [table], 2)
        check(un, 0, [kind, kind], [M.collect_list([()] * len(vals), vals, ungrouped=True), M.collect_set([()] * len(vals), vals, ungrouped=True)])
        assert rows_of(un, 0, [kind, kind])[()][1] == sorted({v for v in vals if v is not None})
