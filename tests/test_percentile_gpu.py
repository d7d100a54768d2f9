"""Spark's exact percentile (median, percentile, percentile_cont) in HashAggregate on the GPU: Partial / PartialMerge / Final, grouped and not, against the
pure-Python model of tests/percentile_model.py (the reference's formula in plain floats; pinned by tests/test_percentile_cpu.py).  Results are compared
exactly — zeros equal, NaN by isnan —, state lists as multisets per group, groups as a mapping from their key values.

Row counts: 0, 1, 2, 255 / 257 (one block of the streaming kernels), 4096 / 4097 (the one-workgroup sort ends at 4096 rows) and 20 011 (the radix path, and
some twenty 1024-row scan tiles).  5000 groups are more than one workgroup's threads, most of them of size 1 to 4."""
import functools
import math
import random
import struct

import numpy as np
import pyarrow as pa
import pytest

from datafusion_comet_amd import native, serde as S
from tests import percentile_model as M

pytestmark = pytest.mark.gpu
F64, I32, I64, STR = S.T_DOUBLE, S.T_INT32, S.T_INT64, S.T_STRING
LIST = S.list_type(F64, True)
PCTS = [0.0, 0.25, 0.5, 0.123456789, 0.99, 1.0]
N = 20_011
NEG_NAN = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000001))[0]


def run(plan, tables, ncols, batch_rows=8192):
    ins = [native.HostInput.from_table(t, batch_rows) for t in tables]
    out = native.execute_to_table(ins, ncols, plan.encode(), batch_size=0)
    return pa.Table.from_batches(out) if out else None


def f64_column(values):
    """floats / None → a Float64 column that keeps every bit (NaN payloads and signs too)"""
    a = np.array([0.0 if v is None else v for v in values], dtype=np.float64)
    mask = np.array([v is None for v in values], dtype=bool)
    return pa.array(a, pa.float64(), mask=mask if mask.any() else None)


@functools.lru_cache(maxsize=None)
def data():
    """N doubles over several magnitudes with duplicates, a third of them NULL (as Python values), and a second column with another NULL pattern"""
    rng = random.Random(20261020)
    x = [None if rng.random() < 1 / 3 else (float(rng.randint(-50, 50)) if rng.random() < 0.2 else rng.uniform(-1, 1) * 10.0 ** rng.randint(-3, 6)) for _ in range(N)]
    y = [None if i % 5 == 0 else rng.uniform(-1e3, 1e3) for i in range(N)]
    flag = [None if rng.random() < 0.1 else rng.randint(0, 1) for _ in range(N)]
    return x, y, flag


def groups_of(keys, values, keep=None):
    """key tuple → the kept (non-NULL, not filtered out) values; every key that occurs has an entry"""
    g = {}
    for i, k in enumerate(keys):
        lst = g.setdefault(k, [])
        if values[i] is not None and (keep is None or keep[i]):
            lst.append(values[i])
    return g


def rows_of(t, nkeys):
    """result table → key tuple → the other columns' values of that row; the keys must be distinct"""
    cols = [t.column(i).to_pylist() for i in range(t.num_columns)]
    out = {}
    for r in range(t.num_rows):
        k = tuple(c[r] for c in cols[:nkeys])
        assert k not in out, f"group {k} twice"
        out[k] = [c[r] for c in cols[nkeys:]]
    return out


def check_states(t, nkeys, want_per_agg):
    """Partial / PartialMerge output against want_per_agg[j]: key → kept values"""
    if not want_per_agg[0]:
        assert t is None or t.num_rows == 0
        return
    got = rows_of(t, nkeys)
    assert set(got) == set(want_per_agg[0]), (len(got), len(want_per_agg[0]))
    for j in range(nkeys, t.num_columns):
        f = t.schema.field(j)
        assert pa.types.is_list(f.type) and f.type.value_type == pa.float64() and f.type.value_field.nullable, f
        assert t.column(j).null_count == 0      # the state is never NULL: an empty group has an empty list
    for k, lists in got.items():
        assert len(lists) == len(want_per_agg)
        for j, lst in enumerate(lists):
            assert lst is not None and None not in lst, (k, j)
            assert M.same_multiset(lst, want_per_agg[j][k]), (k, j, len(lst), len(want_per_agg[j][k]))


def check_results(t, nkeys, want_per_agg, pcts):
    """Final output against the model over want_per_agg[j]: key → kept values, pcts[j] the aggregate's percentage"""
    if not want_per_agg[0]:
        assert t is None or t.num_rows == 0
        return
    got = rows_of(t, nkeys)
    assert set(got) == set(want_per_agg[0]), (len(got), len(want_per_agg[0]))
    for j in range(nkeys, t.num_columns):
        assert t.schema.field(j).type == pa.float64()
    for k, vals in got.items():
        for j, v in enumerate(vals):
            want = M.percentile(want_per_agg[j][k], pcts[j])
            assert M.same(v, want), (k, j, pcts[j], v, want, len(want_per_agg[j][k]))


def bits_of(t):
    return [[None if v is None else struct.pack("<d", v) for v in t.column(i).to_pylist()] for i in range(t.num_columns)] if t is not None else None


def agg_plans(key_types, value_types, aggs, mode=S.PARTIAL):
    fields = list(key_types) + list(value_types)
    return S.hash_agg(S.scan(fields), [S.col(i, t) for i, t in enumerate(key_types)], aggs, mode)


def merge_plan(key_types, aggs, mode):
    fields = list(key_types) + [LIST] * len(aggs)
    return S.hash_agg(S.scan(fields), [S.col(i, t) for i, t in enumerate(key_types)], aggs, mode)


# --------------------------------------------------------------------------- ungrouped

@pytest.mark.parametrize("n", [0, 1, 2, 255, 257, 4096, 4097, N])
def test_ungrouped_partial_and_final(built, n):
    x = data()[0][:n]
    aggs = [S.percentile(S.col(0, F64), p) for p in PCTS]      # six percentages over one column in ONE node
    kept = {(): [v for v in x if v is not None]}
    table = pa.table({"x": f64_column(x)})
    seen = []
    for batch_rows in (8192, 1000):
        st = run(agg_plans([], [F64], aggs), [table], len(PCTS), batch_rows)
        assert st is not None and st.num_rows == 1      # no keys: one group, whatever the row count
        check_states(st, 0, [kept] * len(PCTS))
        fin = run(merge_plan([], aggs, S.FINAL), [st], len(PCTS), batch_rows)
        assert fin is not None and fin.num_rows == 1
        check_results(fin, 0, [kept] * len(PCTS), PCTS)
        if not kept[()]:
            assert fin.column(0).null_count == 1
        seen.append(bits_of(fin))
    assert seen[0] == seen[1]      # the same bits for both batch sizes
    # Final over exactly n flattened rows: one state row per 1000 values, NULL elements included
    parts = [x[a:a + 1000] for a in range(0, n, 1000)] or [[]]
    one = pa.array(parts, pa.list_(pa.float64()))
    fin = run(merge_plan([], aggs, S.FINAL), [pa.table({f"s{j}": one for j in range(len(PCTS))})], len(PCTS))
    check_results(fin, 0, [kept] * len(PCTS), PCTS)
    assert bits_of(fin) == seen[0]


# --------------------------------------------------------------------------- grouped

def int_keys(ngroups, null_every=17):
    rng = random.Random(ngroups)
    return [(None if i % null_every == 3 else rng.randrange(ngroups) - ngroups // 2,) for i in range(N)]


@pytest.mark.parametrize("ngroups", [1, 7, 5000])
def test_grouped_by_int32_with_null_key_empty_and_filtered_groups(built, ngroups):
    x, _, flag = data()
    x = list(x)
    flag = list(flag)
    keys = int_keys(ngroups)
    present = sorted({k for k in keys if k[0] is not None})
    all_null, filtered_out = present[0], present[-1]
    for i, k in enumerate(keys):
        if ngroups > 1 and k == all_null:
            x[i] = None               # a group whose values are all NULL
        if ngroups > 1 and k == filtered_out:
            flag[i] = 0               # a group that only the FILTER empties
            x[i] = 1.5 if x[i] is None else x[i]
    flt = S.eq(S.col(2, I32), S.lit(1, I32))
    pcts = [0.5, 0.123456789, 0.5]
    aggs = [S.percentile(S.col(1, F64), pcts[0]), S.percentile(S.col(1, F64), pcts[1]), S.percentile(S.col(1, F64), pcts[2], filter=flt)]
    table = pa.table({"k": pa.array([k[0] for k in keys], pa.int32()), "x": f64_column(x), "f": pa.array(flag, pa.int32())})
    plain, kept_f = groups_of(keys, x), groups_of(keys, x, [f == 1 for f in flag])
    want = [plain, plain, kept_f]
    if ngroups > 1:
        assert plain[all_null] == [] and kept_f[filtered_out] == [] and plain[filtered_out]
    assert (None,) in plain
    st = run(agg_plans([I32], [F64, I32], aggs), [table], 4, 1000)
    check_states(st, 1, want)
    fin = run(merge_plan([I32], aggs, S.FINAL), [st], 4)
    check_results(fin, 1, want, pcts)
    if ngroups > 1:
        got = rows_of(fin, 1)
        assert got[all_null] == [None, None, None] and got[filtered_out][2] is None and got[filtered_out][0] is not None


@pytest.mark.parametrize("n", [100, 5000])
def test_keyed_aggregate_whose_rows_all_share_one_key(built, n):
    """one group and no NULL key: no byte plane of the key varies (100 rows: the one-workgroup sort; 5000: the radix path)"""
    x = data()[0][:n]
    keys = [(42,)] * n
    pcts = [0.5, 0.99]
    aggs = [S.percentile(S.col(1, F64), p) for p in pcts]
    table = pa.table({"k": pa.array([42] * n, pa.int32()), "x": f64_column(x)})
    want = [groups_of(keys, x)] * 2
    assert list(want[0]) == [(42,)]
    st = run(agg_plans([I32], [F64], aggs), [table], 3, 1000)
    assert st.num_rows == 1
    check_states(st, 1, want)
    fin = run(merge_plan([I32], aggs, S.FINAL), [st], 3)
    assert fin.num_rows == 1
    check_results(fin, 1, want, pcts)
    # … and the same key with nothing but NULL values
    nulls = pa.table({"k": pa.array([42] * n, pa.int32()), "x": f64_column([None] * n)})
    st = run(agg_plans([I32], [F64], aggs), [nulls], 3)
    check_states(st, 1, [{(42,): []}] * 2)
    assert rows_of(run(merge_plan([I32], aggs, S.FINAL), [st], 3), 1) == {(42,): [None, None]}


def test_grouped_by_utf8_and_by_two_columns(built):
    x, y, _ = data()
    rng = random.Random(7)
    names = ["", "a", "ab", "abé", "a much longer key than fifteen bytes", None, "zz"]
    k1 = [names[rng.randrange(len(names))] for _ in range(N)]
    k2 = [None if i % 11 == 0 else rng.randrange(3) for i in range(N)]
    pcts = [0.25, 0.99]
    # Utf8 key
    aggs = [S.percentile(S.col(1, F64), p) for p in pcts]
    table = pa.table({"k": pa.array(k1, pa.utf8()), "x": f64_column(x)})
    want = [groups_of([(k,) for k in k1], x)] * 2
    st = run(agg_plans([STR], [F64], aggs), [table], 3, 1000)
    check_states(st, 1, want)
    check_results(run(merge_plan([STR], aggs, S.FINAL), [st], 3), 1, want, pcts)
    # (Utf8, Int32) key, two value columns with different NULL patterns in one node
    aggs = [S.percentile(S.col(2, F64), pcts[0]), S.percentile(S.col(3, F64), pcts[1])]
    table = pa.table({"k1": pa.array(k1, pa.utf8()), "k2": pa.array(k2, pa.int32()), "x": f64_column(x), "y": f64_column(y)})
    keys = list(zip(k1, k2))
    want = [groups_of(keys, x), groups_of(keys, y)]
    st = run(agg_plans([STR, I32], [F64, F64], aggs), [table], 4)
    check_states(st, 2, want)
    check_results(run(merge_plan([STR, I32], aggs, S.FINAL), [st], 4), 2, want, pcts)


def test_one_child_under_two_filters(built):
    x, _, flag = data()
    keys = int_keys(7)
    fa, fb = S.eq(S.col(2, I32), S.lit(1, I32)), S.eq(S.col(2, I32), S.lit(0, I32))
    pcts = [0.5, 0.5, 0.25]
    aggs = [S.percentile(S.col(1, F64), 0.5, filter=fa), S.percentile(S.col(1, F64), 0.5, filter=fb), S.percentile(S.col(1, F64), 0.25, filter=fa)]
    table = pa.table({"k": pa.array([k[0] for k in keys], pa.int32()), "x": f64_column(x), "f": pa.array(flag, pa.int32())})
    ga, gb = groups_of(keys, x, [f == 1 for f in flag]), groups_of(keys, x, [f == 0 for f in flag])
    want = [ga, gb, ga]
    st = run(agg_plans([I32], [F64, I32], aggs), [table], 4)
    check_states(st, 1, want)
    check_results(run(merge_plan([I32], aggs, S.FINAL), [st], 4), 1, want, pcts)
    # ungrouped, too
    st = run(agg_plans([], [I32, F64, I32], [S.percentile(S.col(1, F64), 0.5, filter=fa), S.percentile(S.col(1, F64), 0.5, filter=fb)]), [table], 2)
    check_states(st, 0, [{(): [v for v, f in zip(x, flag) if v is not None and f == 1]}, {(): [v for v, f in zip(x, flag) if v is not None and f == 0]}])


# --------------------------------------------------------------------------- Partial → (PartialMerge →) Final

def test_partial_then_final_and_partial_merge(built):
    x, _, _ = data()
    keys = int_keys(300)
    pcts = [0.5, 0.95]
    aggs = [S.percentile(S.col(1, F64), p) for p in pcts]
    want = [groups_of(keys, x)] * 2
    states = []
    for a, b in ((0, 7000), (7000, 7001), (7001, N)):
        t = pa.table({"k": pa.array([k[0] for k in keys[a:b]], pa.int32()), "x": f64_column(x[a:b])})
        states.append(run(agg_plans([I32], [F64], aggs), [t], 3))
    both = pa.concat_tables(states).combine_chunks()
    check_results(run(merge_plan([I32], aggs, S.FINAL), [both], 3, 1000), 1, want, pcts)
    merged = run(merge_plan([I32], aggs, S.PARTIAL_MERGE), [both], 3)
    check_states(merged, 1, want)
    assert merged.num_rows == len(want[0]) < both.num_rows
    check_results(run(merge_plan([I32], aggs, S.FINAL), [merged], 3), 1, want, pcts)
    # PartialMerge of two states, Final over its output and the third
    pm = run(merge_plan([I32], aggs, S.PARTIAL_MERGE), [pa.concat_tables(states[:2]).combine_chunks()], 3)
    rest = pa.concat_tables([pm.cast(states[2].schema), states[2]]).combine_chunks()
    check_results(run(merge_plan([I32], aggs, S.FINAL), [rest], 3), 1, want, pcts)


def test_final_over_hand_made_states_with_null_rows_and_null_elements(built):
    lt = pa.list_(pa.float64())
    k = [1, 1, 2, 2, None, 3, 3, 1, 4]
    s = [[3.0, None, 1.0], None, [], None, [None, 9.0], None, None, [2.0, 8.0], [None]]
    pcts = [0.5, 0.123456789]
    aggs = [S.percentile(S.col(1, F64), p) for p in pcts]
    table = pa.table({"k": pa.array(k, pa.int32()), "s0": pa.array(s, lt), "s1": pa.array(s, lt)})
    kept = {(1,): [3.0, 1.0, 2.0, 8.0], (2,): [], (None,): [9.0], (3,): [], (4,): []}
    fin = run(merge_plan([I32], aggs, S.FINAL), [table], 3)
    check_results(fin, 1, [kept, kept], pcts)
    got = rows_of(fin, 1)
    assert got[(2,)] == got[(3,)] == got[(4,)] == [None, None] and got[(1,)][0] == 2.5
    check_states(run(merge_plan([I32], aggs, S.PARTIAL_MERGE), [table], 3), 1, [kept, kept])
    # ungrouped: nothing but NULL / empty states → one NULL; no state rows at all → one NULL as well
    empty = pa.table({"s0": pa.array([None, [], [None]], lt)})
    for t in (empty, empty.slice(0, 0)):
        fin = run(merge_plan([], aggs[:1], S.FINAL), [t], 1)
        assert fin.num_rows == 1 and fin.column(0).to_pylist() == [None]
        st = run(merge_plan([], aggs[:1], S.PARTIAL_MERGE), [t], 1)
        assert st.num_rows == 1 and st.column(0).to_pylist() == [[]]


# --------------------------------------------------------------------------- values and bits

def test_special_values_at_selected_positions(built):
    inf, nan = float("inf"), float("nan")
    groups = [
        [-inf, -0.0, 0.0, inf, nan],
        [NEG_NAN, 1.0, 2.0, 3.0, nan],                       # a NaN with its sign bit set is as great as any other
        [5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, -5e-324],
        [0.0, -0.0, -0.0, 0.0, 0.0],
        [inf, inf, inf, -inf, -inf],
        [nan, NEG_NAN, nan, None, None],
        [1.7976931348623157e308, 1.7976931348623157e308, -1.7976931348623157e308, 1e308, -1e308],
    ]
    pcts = [0.0, 0.25, 0.5, 0.75, 1.0, 0.1, 0.6, 0.9]      # the first five land ON the five values, the others between two of them
    rng = random.Random(5)
    rows = [(g, v) for g, vals in enumerate(groups) for v in vals]
    rng.shuffle(rows)
    keys = [(g,) for g, _ in rows]
    x = [v for _, v in rows]
    aggs = [S.percentile(S.col(1, F64), p) for p in pcts]
    table = pa.table({"k": pa.array([g for g, _ in rows], pa.int32()), "x": f64_column(x)})
    want = [groups_of(keys, x)] * len(pcts)
    st = run(agg_plans([I32], [F64], aggs), [table], 1 + len(pcts))
    check_states(st, 1, want)
    fin = run(merge_plan([I32], aggs, S.FINAL), [st], 1 + len(pcts))
    check_results(fin, 1, want, pcts)
    got = rows_of(fin, 1)
    assert got[(1,)][0] == 1.0 and got[(1,)][2] == 3.0 and math.isnan(got[(1,)][3]) and math.isnan(got[(1,)][4])
    assert got[(0,)][0] == -inf and got[(0,)][3] == inf and math.isnan(got[(0,)][4])
    assert all(math.isnan(v) for v in got[(5,)])
    assert got[(4,)][1] == -inf and got[(4,)][2] == inf      # lo == hi = ±inf: no 0 · inf


def test_two_thousand_random_cases_show_no_fused_multiply_add(built):
    """500 groups of up to 50 values and four percentages: by tests/test_percentile_cpu.py about a quarter of such cases change their last bit under a fused multiply-add"""
    rng = random.Random(20261021)
    pcts = [rng.random() for _ in range(3)] + [0.123456789]
    keys, x = [], []
    for g in range(500):
        scale = 10.0 ** rng.randint(-3, 6)
        for _ in range(1 + rng.randrange(50)):
            keys.append((g,))
            x.append(rng.uniform(-scale, scale))
    keys.extend([(500,), (500,)])
    x.extend([-45.5, 28.4])      # the witness
    order = list(range(len(x)))
    rng.shuffle(order)
    keys, x = [keys[i] for i in order], [x[i] for i in order]
    aggs = [S.percentile(S.col(1, F64), p) for p in pcts]
    table = pa.table({"k": pa.array([k[0] for k in keys], pa.int32()), "x": f64_column(x)})
    want = [groups_of(keys, x)] * len(pcts)
    st = run(agg_plans([I32], [F64], aggs), [table], 1 + len(pcts))
    fin = run(merge_plan([I32], aggs, S.FINAL), [st], 1 + len(pcts))
    check_results(fin, 1, want, pcts)
    assert rows_of(fin, 1)[(500,)][3].hex() == "-0x1.230329214444ep+5"
    # how many of the cases could have told: the exact-arithmetic count
    sensitive = 0
    for k, vals in want[0].items():
        s = M.sort_values(vals)
        for p in pcts:
            pos = float(len(s) - 1) * p
            lo, hi = math.floor(pos), math.ceil(pos)
            if lo != hi and s[lo] != s[hi]:
                u, f1, f2 = M.interpolate_variants(s[lo], s[hi], float(hi) - pos, pos - float(lo))
                sensitive += u != f1 or u != f2
    assert sensitive > 200, sensitive
