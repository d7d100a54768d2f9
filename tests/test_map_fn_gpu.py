"""m[k] / element_at(m, k) (map_extract), map_keys, map_values, map_entries and map_contains_key on the GPU, through the C ABI against the pure-Python model of
tests/map_fn_model.py (pinned by tests/test_map_fn_cpu.py).  Values travel as plain integers / strings (dates as days, timestamps as microseconds, decimals
unscaled, floats as their bits).

Shapes: some 5 000 maps of 0 to 6 entries from a small key domain — NULL maps whose offsets span entries, empty maps, NULL values, duplicate keys, missing
keys, the key at the first and at the last entry — fed as one batch and in batches of 1 000 rows (offsets rebased); and one table whose maps have exactly
0, 1, 2, 63, 64, 65 and 300 entries with the wanted key first, last or absent.  More than one 256-lane block in the random tables.

Every plan the tests run is built by a function of this module and listed by every_plan(): tests/test_map_fn_cpu.py compiles each for gfx950 without a device."""
import decimal
import random

import numpy as np
import pyarrow as pa
import pyarrow.parquet as papq
import pytest

from datafusion_comet_amd import native, serde as S
from tests import map_fn_model as M

pytestmark = pytest.mark.gpu
I32, I64, STR, BOOL = S.T_INT32, S.T_INT64, S.T_STRING, S.T_BOOL
D38 = 10 ** 38 - 1
WORDS = ["", "a", "a\0", "bb", "x", "日本", "日本語", "shared prefix, longer than eight bytes: 1", "shared prefix, longer than eight bytes: 2", "shared prefix", "k=v", "é"]

# kind → (serde type, Arrow type, the small domain its values come from)
KINDS = {
    "bool": (S.T_BOOL, pa.bool_(), [False, True]), "i8": (S.T_INT8, pa.int8(), [-128, -1, 0, 1, 127]), "i16": (S.T_INT16, pa.int16(), [-32768, -2, 0, 3, 32767]),
    "i32": (S.T_INT32, pa.int32(), [-2 ** 31, -7, 0, 7, 2 ** 31 - 1]), "i64": (S.T_INT64, pa.int64(), [-2 ** 63, -5, -1, 0, 1, 3, 2 ** 63 - 1]),
    "date": (S.T_DATE, pa.date32(), [-3, -1, 0, 1, 19000]), "ts": (S.T_TIMESTAMP, pa.timestamp("us", tz="UTC"), [-10 ** 15, -1, 0, 1, 10 ** 15]),
    "ntz": (S.DataType(S.TIMESTAMP_NTZ), pa.timestamp("us"), [-10 ** 15, -1, 0, 2, 10 ** 15]), "dec10_2": (S.decimal(10, 2), pa.decimal128(10, 2), [-10 ** 10 + 1, -100, 0, 1, 10 ** 10 - 1]),
    "dec38_0": (S.decimal(38, 0), pa.decimal128(38, 0), [-D38, -2 ** 64, -1, 0, 1, 2 ** 64, 2 ** 64 + 1, D38]), "str": (STR, pa.utf8(), WORDS),
    # values only (a float key is refused): as their bits — NaNs with payloads, both zeros, infinities
    "f32": (S.T_FLOAT, pa.float32(), [0x00000000, 0x80000000, 0x7FC00000, 0xFFC00001, 0x7F800000, 0x3F800000, 0x00000001]),
    "f64": (S.T_DOUBLE, pa.float64(), [0x0000000000000000, 0x8000000000000000, 0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000000, 0x3FF0000000000000, 1]),
}
KEY_KINDS = [k for k in KINDS if k not in ("f32", "f64")]
INT_BASE = {"i8": pa.int8(), "i16": pa.int16(), "i32": pa.int32(), "i64": pa.int64(), "date": pa.int32(), "ts": pa.int64(), "ntz": pa.int64()}
FLOAT_BITS = {"f32": (np.uint32, np.float32), "f64": (np.uint64, np.float64)}


def MT(kkind, vkind):
    return S.map_type(KINDS[kkind][0], KINDS[vkind][0], True)


def scalars(kind, values):
    """model values (None = NULL) → an Arrow array of the kind"""
    t = KINDS[kind][1]
    if kind in ("bool", "str"):
        return pa.array(values, t)
    if kind in FLOAT_BITS:
        bits, fl = FLOAT_BITS[kind]
        raw = np.array([0 if v is None else v for v in values], dtype=bits).view(fl)
        return pa.array(raw, t, mask=np.array([v is None for v in values], dtype=bool)) if len(values) else pa.array([], t)
    if kind.startswith("dec"):
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            return pa.array([None if v is None else decimal.Decimal(v).scaleb(-t.scale) for v in values], t)
    return pa.array(values, INT_BASE[kind]).cast(t)


def plain(kind, arr):
    """an Arrow array of the kind → model values"""
    arr = arr.combine_chunks() if isinstance(arr, pa.ChunkedArray) else arr
    assert arr.type == KINDS[kind][1], (arr.type, kind)
    if kind in ("bool", "str"):
        return arr.to_pylist()
    if kind in FLOAT_BITS:
        bits, fl = FLOAT_BITS[kind]
        ok = arr.is_valid().to_pylist()
        raw = arr.fill_null(0).to_numpy(zero_copy_only=False).astype(fl, copy=False).view(bits).tolist() if len(arr) else []
        return [b if o else None for b, o in zip(raw, ok)]
    if kind.startswith("dec"):
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            return [None if d is None else int(d.scaleb(arr.type.scale)) for d in arr.to_pylist()]
    return arr.cast(INT_BASE[kind]).to_pylist()


def maps(kkind, vkind, rows, garbage=None):
    """model maps (None = a NULL map) → an Arrow Map<kkind, vkind> column, built from raw offsets so that duplicate keys stay.  `garbage`: the entries a NULL
    map's offsets span (Arrow allows it; nothing may read them)"""
    ks, vs, offs, mask = [], [], [0], []
    for r in rows:
        for k, v in (garbage or []) if r is None else r:
            ks.append(k)
            vs.append(v)
        offs.append(len(ks))
        mask.append(r is None)
    t = pa.map_(KINDS[kkind][1], pa.field("value", KINDS[vkind][1], True))
    return pa.MapArray.from_arrays(pa.array(offs, pa.int32()), scalars(kkind, ks), scalars(vkind, vs), type=t, mask=pa.array(mask, pa.bool_()) if any(mask) else None)


def plain_lists(kind, col):
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    assert pa.types.is_list(col.type) and col.type.value_type == KINDS[kind][1], col.type
    vals, offs, ok = plain(kind, col.values), col.offsets.to_pylist(), col.is_valid().to_pylist()
    return [vals[offs[r]:offs[r + 1]] if ok[r] else None for r in range(len(col))]


def random_maps(kkind, vkind, n, seed, max_len=6):
    """maps of 0 … max_len entries; one in five is built with replacement from the key domain, so that some hold a key twice (the first wins)"""
    rng = random.Random(seed)
    kdom, vdom = KINDS[kkind][2], KINDS[vkind][2]
    val = lambda: None if rng.random() < 0.15 else rng.choice(vdom)
    rows = [[], None, [(kdom[0], vdom[0]), (kdom[0], vdom[-1])], [(kdom[-1], None), (kdom[0], vdom[0]), (kdom[-1], vdom[-1])]]
    while len(rows) < n:
        if rng.random() < 0.08:
            rows.append(None)
            continue
        ln = rng.randrange(0, max_len + 1)
        keys = [rng.choice(kdom) for _ in range(ln)] if rng.random() < 0.2 else rng.sample(kdom, min(ln, len(kdom)))
        rows.append([(k, val()) for k in keys])
    rng.shuffle(rows)
    return rows


def random_keys(kind, n, seed):
    rng = random.Random(seed)
    return [None if rng.random() < 0.06 else rng.choice(KINDS[kind][2]) for _ in range(n)]


def run(plan, tables, ncols, batch_size=0, batch_rows=8192):
    tables = tables if isinstance(tables, list) else [tables]
    out = native.execute_to_table([native.HostInput.from_table(t, batch_rows) for t in tables], ncols, plan.encode(), batch_size=batch_size)
    return pa.Table.from_batches(out) if out else None


def accepted(plan):
    ok, msg = native.check_plan(plan.encode())
    assert ok, msg
    return plan


def lit_of(kind, v):
    return S.lit(v, KINDS[kind][0])


# ---- the plans ----
def lookup_plan(kkind, vkind, literals):
    """[m[lit] for every literal] + [m[NULL], m[k]] over Scan(m: Map<kkind, vkind>, k: kkind)"""
    mt, kt = MT(kkind, vkind), KINDS[kkind][0]
    m, k = S.col(0, mt), S.col(1, kt)
    return S.project(S.scan([mt, kt]), [S.map_extract(m, lit_of(kkind, v)) for v in literals] + [S.map_extract(m, S.lit(None, kt)), S.map_extract(m, k)])


def views_plan(kkind, vkind):
    mt = MT(kkind, vkind)
    m = S.col(0, mt)
    return S.project(S.scan([mt]), [S.map_keys(m), S.map_values(m), S.map_entries(m), m])


def consumers_plan(key_lit, value_lit):
    """the consumers of a derived list over Map<Utf8, Int64>"""
    mt = MT("str", "i64")
    m = S.col(0, mt)
    ks, vs = S.map_keys(m), S.map_values(m)
    return S.project(S.scan([mt]), [S.scalar_func("size", [ks], I32), S.list_extract(vs, S.lit(-1, I32), one_based=True), S.list_extract(ks, S.lit(1, I32), one_based=True),
                                    S.scalar_func("array_contains", [ks, S.lit(key_lit, STR)], BOOL), S.sort_array(ks), S.array_distinct(vs), S.array_max(vs),
                                    S.array_position(vs, S.lit(value_lit, I64)), S.array_position(ks, S.lit(key_lit, STR))])


def values_without_nulls_plan(value_contains_null):
    """consumers of map_values(m) over Map<Utf8, Int64> whose values may / may not be NULL by type"""
    mt = S.map_type(STR, I64, value_contains_null)
    vs = S.map_values(S.col(0, mt))
    return S.project(S.scan([mt]), [S.list_extract(vs, S.lit(1, I32), one_based=True), S.array_max(vs), S.array_distinct(vs), vs])


def contains_column_key_plan():
    """map_contains_key(m, k) with a key COLUMN: array_contains(map_keys(m), k) over Map<Int32, Utf8>"""
    mt = MT("i32", "str")
    return S.project(S.scan([mt, I32]), [S.scalar_func("array_contains", [S.map_keys(S.col(0, mt)), S.col(1, I32)], BOOL)])


def explode_keys_plan():
    mt = MT("str", "i64")
    return S.explode(S.project(S.scan([mt, I64]), [S.map_keys(S.col(0, mt)), S.col(1, I64)]), S.col(0, S.list_type(STR, False)), [S.col(1, I64)])


ENTRY = S.struct_type([("key", STR, False), ("value", I64, True)])


def explode_entries_plan():
    mt = MT("str", "i64")
    return S.explode(S.project(S.scan([mt, I64]), [S.map_entries(S.col(0, mt)), S.col(1, I64)]), S.col(0, S.list_type(ENTRY, False)), [S.col(1, I64)])


def filter_plan():
    """SELECT id, m FROM t WHERE m['a'] = 3, and beside it the pass-through of m"""
    mt = MT("str", "i64")
    src = S.scan([mt, I64])
    return S.project(S.filter_(src, S.eq(S.map_extract(S.col(0, mt), S.lit("a", STR)), S.lit(3, I64))), [S.col(1, I64), S.col(0, mt), S.map_extract(S.col(0, mt), S.lit("x", STR))])


def case_when_plan():
    mt = MT("str", "i64")
    m, k = S.col(0, mt), S.col(1, I64)
    a = S.map_extract(m, S.lit("a", STR))
    return S.project(S.scan([mt, I64]), [S.case_when([(S.gt(a, S.lit(0, I64)), a), (S.is_null(a), k)], S.map_extract(m, S.lit("x", STR))), m])


def aggregate_plan():
    """sum(m['a']) and count(*) by id % 3: map_extract inside an aggregate's fused chain"""
    mt = MT("str", "i64")
    proj = S.project(S.scan([mt, I64]), [S.col(1, I64), S.map_extract(S.col(0, mt), S.lit("a", STR))])
    return S.hash_agg(proj, [S.col(0, I64)], [S.sum_(S.col(1, I64), I64), S.count(S.col(1, I64))])


def join_plan():
    """t JOIN other ON m['a'] = other.v: map_extract in the Projection under a join"""
    mt = MT("str", "i64")
    side = S.project(S.scan([mt, I64]), [S.map_extract(S.col(0, mt), S.lit("a", STR)), S.col(1, I64)])
    return S.hash_join(side, S.scan([I64]), [S.col(0, I64)], [S.col(0, I64)], S.INNER, S.BUILD_RIGHT)


def parquet_plan(path, names, types):
    mt = types[1]
    return S.project(S.native_scan([path], names, types), [S.col(0, types[0]), S.map_extract(S.col(1, mt), S.lit("a", STR)), S.map_keys(S.col(1, mt)), S.map_values(S.col(1, mt))])


def first_and_last(kind):
    dom = KINDS[kind][2]
    return [dom[0], dom[-1]] + ([dom[len(dom) // 2]] if len(dom) > 2 else [])


def every_plan():
    """(name, plan) of every Scan-fed plan above, for the compile check of tests/test_map_fn_cpu.py"""
    for kkind in KEY_KINDS:
        yield "lookup by " + kkind, lookup_plan(kkind, "i64", first_and_last(kkind))
    for vkind in KINDS:
        yield "lookup of " + vkind, lookup_plan("i32", vkind, [7])
    yield "lookup of str by str", lookup_plan("str", "str", ["a"])
    yield "views", views_plan("str", "i64")
    yield "views with float values", views_plan("i64", "f64")
    yield "consumers", consumers_plan("a", 3)
    yield "contains, column key", contains_column_key_plan()
    yield "values without NULLs, nullable type", values_without_nulls_plan(True)
    yield "values without NULLs, non-nullable type", values_without_nulls_plan(False)
    yield "explode keys", explode_keys_plan()
    yield "explode entries", explode_entries_plan()
    yield "filter", filter_plan()
    yield "case when", case_when_plan()
    yield "aggregate", aggregate_plan()
    yield "join", join_plan()


# ---- the tests ----
def check_lookup(kkind, vkind, rows, keys, literals, got):
    vt = KINDS[vkind][1]
    for j, lit in enumerate(literals):
        assert got.column(j).type == vt
        assert plain(vkind, got.column(j)) == [M.map_extract(r, lit) for r in rows], (kkind, vkind, lit)
    n = len(literals)
    assert plain(vkind, got.column(n)) == [None] * len(rows), "a NULL key"
    assert plain(vkind, got.column(n + 1)) == [M.map_extract(r, k) for r, k in zip(rows, keys)], "a key column"


@pytest.mark.parametrize("kkind", KEY_KINDS)
def test_lookup_by_every_key_kind(built, kkind):
    rows, keys = random_maps(kkind, "i64", 5000, 11), random_keys(kkind, 5000, 12)
    literals = first_and_last(kkind)
    dom = KINDS[kkind][2]
    # what the table must hold: NULL and empty maps, a duplicate key, a NULL value under a wanted key, the wanted key first / last / absent, a NULL key
    assert None in rows and [] in rows and None in keys
    assert any(r and len({k for k, _ in r}) < len(r) for r in rows), "no duplicate key"
    for lit in literals:
        assert any(r and r[0][0] == lit for r in rows) and any(r and len(r) > 2 and r[-1][0] == lit and all(k != lit for k, _ in r[:-1]) for r in rows), lit
        assert any(r and all(k != lit for k, _ in r) for r in rows) and any(r and any(k == lit and v is None for k, v in r) for r in rows), lit
    garbage = [(dom[0], 1), (dom[-1], 2)]
    t = pa.table({"m": maps(kkind, "i64", rows, garbage), "k": scalars(kkind, keys)})
    plan = accepted(lookup_plan(kkind, "i64", literals))
    ncols = len(literals) + 2
    got = run(plan, t, ncols)
    check_lookup(kkind, "i64", rows, keys, literals, got)
    check_lookup(kkind, "i64", rows, keys, literals, run(plan, t, ncols, batch_rows=1000))      # (offsets rebased per batch)


@pytest.mark.parametrize("vkind", list(KINDS))
def test_lookup_of_every_value_kind(built, vkind):
    rows, keys = random_maps("i32", vkind, 3000, 21), random_keys("i32", 3000, 22)
    if vkind == "str":
        assert any(r and ("" in [v for _, v in r]) and (None in [v for _, v in r]) for r in rows), '"" beside NULL'
    t = pa.table({"m": maps("i32", vkind, rows, [(7, KINDS[vkind][2][0])]), "k": scalars("i32", keys)})
    plan = accepted(lookup_plan("i32", vkind, [7]))
    check_lookup("i32", vkind, rows, keys, [7], run(plan, t, 3))
    check_lookup("i32", vkind, rows, keys, [7], run(plan, t, 3, batch_rows=1000))


def test_utf8_values_by_utf8_keys(built):
    rows, keys = random_maps("str", "str", 3000, 31), random_keys("str", 3000, 32)
    t = pa.table({"m": maps("str", "str", rows, [("a", "garbage")]), "k": scalars("str", keys)})
    check_lookup("str", "str", rows, keys, ["a"], run(accepted(lookup_plan("str", "str", ["a"])), t, 3))


SIZES = [0, 1, 2, 63, 64, 65, 300]


@pytest.mark.parametrize("kkind", ["i64", "str"])
def test_maps_at_the_wave_boundary(built, kkind):
    """maps of exactly 0 … 300 entries; the wanted key (the key column's) is the first, the last or absent"""
    key = (lambda i: i - 150) if kkind == "i64" else (lambda i: "key number %d of a map, longer than eight bytes" % i)
    absent = 10 ** 6 if kkind == "i64" else "key number 1 of a map"
    rows, keys = [], []
    for n in SIZES:
        entries = [(key(i), 1000 * n + i) for i in range(n)]
        for which in ("first", "last", "absent"):
            rows.append(entries)
            keys.append(absent if which == "absent" or n == 0 else entries[0][0] if which == "first" else entries[-1][0])
    t = pa.table({"m": maps(kkind, "i64", rows), "k": scalars(kkind, keys)})
    lits = [key(0), key(62), key(299)]
    plan = accepted(lookup_plan(kkind, "i64", lits))
    got = run(plan, t, 5)
    check_lookup(kkind, "i64", rows, keys, lits, got)
    want = [M.map_extract(r, k) for r, k in zip(rows, keys)]
    assert want[3:6] == [1000, 1000, None] and want[-3:] == [300000, 300299, None]


def entries_of(col):
    """a List<Struct<key: Utf8, value: Int64>> column → the model's entry dicts"""
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    return col.to_pylist()


def test_views_as_output_columns(built):
    rows = random_maps("str", "i64", 5000, 41)
    t = pa.table({"m": maps("str", "i64", rows, [("a", 1)])})
    plan = accepted(views_plan("str", "i64"))
    for batch_rows in (8192, 1000):
        got = run(plan, t, 4, batch_rows=batch_rows)
        # the types: element names and nullability — keys and entries are never NULL, values are where the map says so
        assert got.schema.field(0).type == pa.list_(pa.field("element", pa.utf8(), False)), got.schema.field(0).type
        assert got.schema.field(0).type.value_field.nullable is False and got.schema.field(0).type.value_field.name == "element"
        assert got.schema.field(1).type == pa.list_(pa.field("element", pa.int64(), True)) and got.schema.field(1).type.value_field.nullable is True
        et = got.schema.field(2).type
        assert pa.types.is_list(et) and et.value_field.nullable is False and pa.types.is_struct(et.value_type)
        assert [(f.name, f.type, f.nullable) for f in et.value_type] == [("key", pa.utf8(), False), ("value", pa.int64(), True)]
        assert plain_lists("str", got.column(0)) == [M.map_keys(r) for r in rows]
        assert plain_lists("i64", got.column(1)) == [M.map_values(r) for r in rows]
        assert entries_of(got.column(2)) == [M.map_entries(r) for r in rows]
        assert got.column(3).combine_chunks().to_pylist() == [None if r is None else list(r) for r in rows], "the map itself, beside its views"


def test_views_carry_float_values_bit_for_bit(built):
    rows = random_maps("i64", "f64", 2000, 42)
    got = run(accepted(views_plan("i64", "f64")), pa.table({"m": maps("i64", "f64", rows)}), 4)
    assert plain_lists("i64", got.column(0)) == [M.map_keys(r) for r in rows]
    assert plain_lists("f64", got.column(1)) == [M.map_values(r) for r in rows]


def test_every_consumer_of_a_derived_list(built):
    from tests import list_fn_model as LM
    rows = random_maps("str", "i64", 5000, 51)
    t = pa.table({"m": maps("str", "i64", rows, [("a", 3)])})
    got = run(accepted(consumers_plan("a", 3)), t, 9)
    ks, vs = [M.map_keys(r) for r in rows], [M.map_values(r) for r in rows]
    assert got.column(0).to_pylist() == [M.size(r) for r in rows]
    assert got.column(1).to_pylist() == [v[-1] if v else None for v in vs], "element_at(map_values(m), -1)"
    assert got.column(2).to_pylist() == [k[0] if k else None for k in ks], "element_at(map_keys(m), 1)"
    assert got.column(3).to_pylist() == [M.map_contains_key(r, "a") for r in rows], "map_contains_key"
    assert plain_lists("str", got.column(4)) == [LM.sort_array(k) for k in ks]
    assert plain_lists("i64", got.column(5)) == [LM.array_distinct(v) for v in vs]
    assert got.column(6).to_pylist() == [LM.array_max(v) for v in vs]
    assert got.column(7).to_pylist() == [LM.array_position(v, 3) for v in vs]
    assert got.column(8).to_pylist() == [LM.array_position(k, "a") for k in ks]


@pytest.mark.parametrize("value_contains_null", [True, False])
def test_values_of_a_batch_without_a_null_value(built, value_contains_null):
    """the chain is planned from the map's type; a batch whose value column carries no validity bitmap must read as all valid"""
    from tests import list_fn_model as LM
    rows = [None if r is None else [(k, 0 if v is None else v) for k, v in r] for r in random_maps("str", "i64", 3000, 55)]
    ks, vs, offs, mask = [], [], [0], []
    for r in rows:
        for k, v in r or []:
            ks.append(k)
            vs.append(v)
        offs.append(len(ks))
        mask.append(r is None)
    t = pa.map_(pa.utf8(), pa.field("value", pa.int64(), value_contains_null))
    col = pa.MapArray.from_arrays(pa.array(offs, pa.int32()), pa.array(ks, pa.utf8()), pa.array(vs, pa.int64()), type=t, mask=pa.array(mask, pa.bool_()))
    assert col.items.null_count == 0
    got = run(accepted(values_without_nulls_plan(value_contains_null)), pa.table({"m": col}), 4)
    want = [M.map_values(r) for r in rows]
    assert got.column(0).to_pylist() == [v[0] if v else None for v in want]
    assert got.column(1).to_pylist() == [LM.array_max(v) for v in want]
    assert got.column(2).combine_chunks().to_pylist() == [LM.array_distinct(v) for v in want]
    assert got.column(3).combine_chunks().to_pylist() == want
    assert got.schema.field(3).type.value_field.nullable is value_contains_null


def test_map_contains_key_with_a_key_column(built):
    rows, keys = random_maps("i32", "str", 3000, 61), random_keys("i32", 3000, 62)
    t = pa.table({"m": maps("i32", "str", rows, [(7, "g")]), "k": scalars("i32", keys)})
    got = run(accepted(contains_column_key_plan()), t, 1)
    assert got.column(0).to_pylist() == [M.map_contains_key(r, k) for r, k in zip(rows, keys)]


def test_explode_of_keys_and_of_entries(built):
    rows = random_maps("str", "i64", 3000, 71)
    t = pa.table({"m": maps("str", "i64", rows, [("a", 1)]), "id": pa.array(range(len(rows)), pa.int64())})
    got = run(accepted(explode_keys_plan()), t, 2)
    assert list(zip(got.column(0).to_pylist(), got.column(1).to_pylist())) == [(i, k) for i, r in enumerate(rows) for k, _ in (r or [])]
    got = run(accepted(explode_entries_plan()), t, 2)
    assert got.schema.field(1).type == pa.struct([pa.field("key", pa.utf8(), False), pa.field("value", pa.int64(), True)])
    assert list(zip(got.column(0).to_pylist(), got.column(1).to_pylist())) == [(i, {"key": k, "value": v}) for i, r in enumerate(rows) for k, v in (r or [])]


def plan_table(n, seed):
    rng = random.Random(seed)
    rows = []
    for _ in range(n):
        if rng.random() < 0.1:
            rows.append(None)
            continue
        keys = rng.sample(["a", "b", "x", "a longer key than eight bytes"], rng.randrange(0, 5))
        rows.append([(k, None if rng.random() < 0.1 else rng.randrange(-2, 6)) for k in keys])
    return rows


def test_filter_on_a_lookup_with_live_and_dropped_rows(built):
    rows = plan_table(5000, 81)
    live = [i for i, r in enumerate(rows) if M.map_extract(r, "a") == 3]
    assert 0 < len(live) < len(rows) // 2
    # a dropped row's map must not influence anything: the same live rows among other dropped rows give the same answer
    other = [r if i in set(live) else [("a", 4), ("x", 99)] for i, r in enumerate(rows)]
    plan = accepted(filter_plan())
    answers = []
    for table_rows in (rows, other):
        t = pa.table({"m": maps("str", "i64", table_rows, [("a", 3)]), "id": pa.array(range(len(rows)), pa.int64())})
        got = run(plan, t, 3)
        assert got.column(0).to_pylist() == live
        assert got.column(1).combine_chunks().to_pylist() == [rows[i] for i in live]
        assert got.column(2).to_pylist() == [M.map_extract(rows[i], "x") for i in live]
        answers.append(got)
    assert answers[0].equals(answers[1])


def test_lookup_inside_case_when_beside_the_map_itself(built):
    rows = plan_table(3000, 82)
    ids = list(range(100, 100 + len(rows)))
    t = pa.table({"m": maps("str", "i64", rows, [("a", 3)]), "id": pa.array(ids, pa.int64())})
    got = run(accepted(case_when_plan()), t, 2)

    def want(r, k):
        a = M.map_extract(r, "a")
        return a if a is not None and a > 0 else k if a is None else M.map_extract(r, "x")
    assert got.column(0).to_pylist() == [want(r, k) for r, k in zip(rows, ids)]
    assert got.column(1).combine_chunks().to_pylist() == rows


def test_lookup_under_an_aggregate_and_under_a_join(built):
    rows = plan_table(3000, 83)
    ids = [i % 3 for i in range(len(rows))]
    t = pa.table({"m": maps("str", "i64", rows, [("a", 3)]), "id": pa.array(ids, pa.int64())})
    got = run(accepted(aggregate_plan()), t, 3)
    want = {}
    for r, g in zip(rows, ids):
        a = M.map_extract(r, "a")
        s, c = want.get(g, (None, 0))
        want[g] = ((s or 0) + a, c + 1) if a is not None else (s, c)
    assert {g: (s, c) for g, s, c in zip(*[got.column(j).to_pylist() for j in range(3)])} == want
    other = pa.table({"v": pa.array([3, 5, None, 3], pa.int64())})
    got = run(accepted(join_plan()), [t, other], 3)
    pairs = sorted(zip(got.column(1).to_pylist(), got.column(0).to_pylist(), got.column(2).to_pylist()))
    assert pairs == sorted((g, a, v) for r, g in zip(rows, ids) for a in [M.map_extract(r, "a")] for v in [3, 5, 3] if a is not None and a == v)


def test_a_map_column_read_from_parquet(built, tmp_path):
    rows = plan_table(4000, 84)
    t = pa.table({"id": pa.array(range(len(rows)), pa.int64()), "m": maps("str", "i64", [r if r is not None else None for r in rows])})
    path = str(tmp_path / "maps.parquet")
    papq.write_table(t, path, compression="snappy", row_group_size=1500)
    types = [S.from_arrow_type(f.type) for f in t.schema]
    plan = accepted(parquet_plan(path, t.schema.names, types))
    out = native.execute_to_table([], 4, plan.encode())
    got = pa.Table.from_batches(out)
    assert got.column(0).to_pylist() == list(range(len(rows)))
    assert got.column(1).to_pylist() == [M.map_extract(r, "a") for r in rows]
    assert plain_lists("str", got.column(2)) == [M.map_keys(r) for r in rows]
    assert plain_lists("i64", got.column(3)) == [M.map_values(r) for r in rows]


def test_the_same_bits_for_every_batch_size(built):
    rows, keys = random_maps("str", "f64", 5000, 91), random_keys("str", 5000, 92)
    t = pa.table({"m": maps("str", "f64", rows, [("a", 1)]), "k": scalars("str", keys)})
    mt = MT("str", "f64")
    m = S.col(0, mt)
    plan = accepted(S.project(S.scan([mt, STR]), [S.map_extract(m, S.col(1, STR)), S.map_extract(m, S.lit("a", STR)), S.map_keys(m), S.map_values(m)]))
    whole, small = run(plan, t, 4, batch_size=0), run(plan, t, 4, batch_size=700)
    assert whole.num_rows == small.num_rows == len(rows)
    for j in range(2):
        assert plain("f64", whole.column(j)) == plain("f64", small.column(j)) == [M.map_extract(r, k if j == 0 else "a") for r, k in zip(rows, keys)]
    assert plain_lists("str", whole.column(2)) == plain_lists("str", small.column(2))
    assert plain_lists("f64", whole.column(3)) == plain_lists("f64", small.column(3)) == [M.map_values(r) for r in rows]
