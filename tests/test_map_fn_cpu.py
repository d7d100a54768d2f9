"""m[k] / element_at(m, k) (map_extract), map_keys, map_values, map_entries and map_contains_key without a GPU: the model of tests/map_fn_model.py against
Spark's answers for the reference's SQL tests (tests/golden/map_fn_cases.json); what createPlan accepts and what it refuses by name; the serde helpers'
bytes; every plan of tests/test_map_fn_gpu.py compiled for gfx950 (hiprtc needs no device); and csrc/device/map_fn.hpp under AddressSanitizer / UBSan as a
stand-alone program."""
import json
import os
import shutil
import subprocess

import pytest

from datafusion_comet_amd import native, serde as S
from tests import map_fn_model as M

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "datafusion-comet_amd", "csrc")
I32, I64, STR, BOOL = S.T_INT32, S.T_INT64, S.T_STRING, S.T_BOOL
ENGINE = "MI355X native engine"

with open(os.path.join(_HERE, "golden", "map_fn_cases.json")) as fh:
    GOLDEN = json.load(fh)["cases"]


def test_the_model_reproduces_sparks_answers():
    seen = set()
    for c in GOLDEN:
        rows = [None if r is None else [tuple(e) for e in r] for r in c["input"]]
        seen.add((c["from"], c["fn"]))
        if c["fn"] in ("map_extract", "map_contains_key"):
            got = [getattr(M, c["fn"])(r, c["key"]) for r in rows]
        else:
            got = [getattr(M, c["fn"])(r) for r in rows]
        assert got == c["want"], c
    assert {s for s, _ in seen} == {"get_map_value", "element_at_map", "map_keys", "map_values", "map_entries", "map_contains_key"}
    assert {f for _, f in seen} == {"map_extract", "map_keys", "map_values", "map_entries", "map_contains_key"}


def test_the_model_on_the_rules_the_sql_tests_do_not_reach():
    assert M.map_extract([("a", 1), ("a", 2)], "a") == 1, "a duplicate key: the first entry wins"
    assert M.map_extract([("a", None), ("a", 2)], "a") is None, "… also where its value is NULL"
    assert M.map_extract([(True, 1)], 1) is None and M.map_extract([("a", 1)], "a\0") is None and M.map_extract([], "a") is None
    assert M.map_values([("a", None)]) == [None] and M.map_entries([("a", None)]) == [{"key": "a", "value": None}]
    assert M.map_contains_key([("a", None)], "a") is True and M.map_contains_key(None, "a") is None and M.map_contains_key([], None) is None
    assert M.size(None) == -1 and M.size([]) == 0


# ---- createPlan ----
KEYS = {"bool": S.T_BOOL, "i8": S.T_INT8, "i16": S.T_INT16, "i32": I32, "i64": I64, "date": S.T_DATE, "ts": S.T_TIMESTAMP, "ntz": S.DataType(S.TIMESTAMP_NTZ),
        "dec10_2": S.decimal(10, 2), "dec38_0": S.decimal(38, 0), "str": STR}
VALUES = dict(KEYS, f32=S.T_FLOAT, f64=S.T_DOUBLE)
MSI = S.map_type(STR, I64, True)


def accepts(plan):
    ok, msg = native.check_plan(plan.encode())
    assert ok, msg
    return msg


def refuses(plan, *words):
    ok, msg = native.check_plan(plan.encode())
    assert not ok, msg
    for w in words:
        assert w in msg, (w, msg)


def size(x):
    return S.scalar_func("size", [x], I32)


@pytest.mark.parametrize("kind", list(KEYS))
def test_createplan_accepts_a_lookup_by_each_key_type(kind):
    kt = KEYS[kind]
    mt = S.map_type(kt, I64, True)
    m, k = S.col(0, mt), S.col(1, kt)
    src = S.scan([mt, kt])
    for key in (k, S.lit(None, kt)):      # m[col] with an integer … key column and with a Utf8 key column
        accepts(S.project(src, [S.map_extract(m, key)]))
    accepts(S.project(src, [S.map_keys(m), S.map_values(m), S.map_entries(m)]))
    accepts(S.project(src, [S.scalar_func("array_contains", [S.map_keys(m), S.lit(None, kt)], BOOL)]))
    if kind != "str":
        accepts(S.project(src, [S.scalar_func("array_contains", [S.map_keys(m), k], BOOL)]))


@pytest.mark.parametrize("kind", list(VALUES))
def test_createplan_accepts_a_lookup_of_each_value_type(kind):
    mt = S.map_type(I32, VALUES[kind], True)
    msg = accepts(S.project(S.scan([mt]), [S.map_extract(S.col(0, mt), S.lit(1, I32))]))
    assert ("gathered" in msg) == (kind == "str"), msg      # a Utf8 value is gathered by entry row, the others are loaded by the kernel
    accepts(S.project(S.scan([mt]), [S.map_values(S.col(0, mt))]))


def test_createplan_accepts_each_function_and_each_consumer():
    src = S.scan([MSI, I64, STR])
    m, n, s = S.col(0, MSI), S.col(1, I64), S.col(2, STR)
    a = S.map_extract(m, S.lit("k", STR))
    for e in (a, S.map_keys(m), S.map_values(m), S.map_entries(m),
              S.scalar_func("array_contains", [S.map_keys(m), S.lit("k", STR)], BOOL),      # map_contains_key(m, 'k') as Spark rewrites it
              S.sort_array(S.map_keys(m)), size(S.map_values(m)), S.list_extract(S.map_values(m), S.lit(-1, I32), one_based=True),
              S.array_distinct(S.map_values(m)), S.array_max(S.map_values(m)), S.array_position(S.map_values(m), n), S.map_extract(m, s), size(m)):
        accepts(S.project(src, [e]))
    entries = S.list_type(S.struct_type([("key", STR, False), ("value", I64, True)]), False)
    accepts(S.explode(S.project(src, [S.map_entries(m), n]), S.col(0, entries), [S.col(1, I64)]))
    accepts(S.explode(S.project(src, [S.map_keys(m), n]), S.col(0, S.list_type(STR, False)), [S.col(1, I64)]))
    # a Filter on m['k'] = 3 with a Projection above it
    msg = accepts(S.project(S.filter_(src, S.eq(a, S.lit(3, I64))), [n, m]))
    assert "filter" in msg and "Map(Utf8, Int64) (gathered)" in msg
    accepts(S.project(src, [S.case_when([(S.gt(a, S.lit(0, I64)), a)], n), m]))


def test_equal_views_share_one_derived_column():
    src = S.scan([MSI, I64])
    m = S.col(0, MSI)
    cg = lambda exprs: native.plan_codegen(S.project(src, exprs).encode(), [False] * 2)
    assert cg([S.map_keys(m), size(S.map_keys(m)), S.sort_array(S.map_keys(m))])["derived"] == 2      # the view, and its sort
    assert cg([S.map_keys(m), S.map_keys(m)])["derived"] == 1
    assert cg([S.map_keys(m), S.map_values(m), S.map_entries(m)])["derived"] == 3
    # map_extract is no derived column: a per-row loop of the fused kernel over device/map_fn.hpp
    d = cg([S.map_extract(m, S.lit("k", STR))])
    assert d["derived"] == 0 and '#include "comet_map_fn.hpp"' in d["source"] and "mf_find_lit(" in d["source"]
    # … and a plan without a map function does not see the header
    assert "comet_map_fn" not in cg([size(m), S.col(1, I64)])["source"]


FOUR = {"map_extract": lambda x: S.map_extract(x, S.lit("k", STR)), "map_keys": S.map_keys, "map_values": S.map_values, "map_entries": S.map_entries}


@pytest.mark.parametrize("name", list(FOUR))
def test_createplan_refuses_a_map_that_is_no_source_column(name):
    fn = FOUR[name]
    src = S.scan([MSI, S.struct_type([("m", MSI, True)]), I64])
    m = S.col(0, MSI)
    # a computed map, a map inside a struct, something that is no map
    refuses(S.project(src, [fn(S.case_when([(S.is_not_null(m), m)], m))]), name, ENGINE, "map COLUMN")
    refuses(S.project(src, [fn(S.get_struct_field(S.col(1, S.struct_type([("m", MSI, True)])), 0))]), name, ENGINE, "map COLUMN")
    refuses(S.project(src, [fn(S.col(2, I64))]), name, ENGINE)


@pytest.mark.parametrize("name", ["map_extract", "map_keys", "map_values"])
def test_createplan_refuses_nested_keys_and_values(name):
    st = S.struct_type([("a", I32, True)])
    for mt in (S.map_type(STR, S.list_type(I32, True), True), S.map_type(STR, st, True), S.map_type(st, I64, True), S.map_type(STR, S.map_type(STR, I64, True), True)):
        refuses(S.project(S.scan([mt]), [FOUR[name](S.col(0, mt))]), name, ENGINE, "nested")
        accepts(S.project(S.scan([mt]), [S.map_entries(S.col(0, mt)), S.col(0, mt)]))      # map_entries takes any map the engine passes through


def test_createplan_refuses_the_other_keys_and_values_of_a_lookup():
    for kt, word in ((S.T_FLOAT, "Float32"), (S.T_DOUBLE, "Float64"), (S.T_BINARY, "Binary keys")):
        mt = S.map_type(kt, I64, True)
        refuses(S.project(S.scan([mt]), [S.map_extract(S.col(0, mt), S.lit(None, kt))]), "map_extract", word, ENGINE)
    mb = S.map_type(I32, S.T_BINARY, True)
    refuses(S.project(S.scan([mb]), [S.map_extract(S.col(0, mb), S.lit(1, I32))]), "map_extract", "Binary values", ENGINE)
    # the key is of exactly the map's key type: both are named
    mi = S.map_type(I32, I64, True)
    src = S.scan([mi, I64, MSI, STR])
    refuses(S.project(src, [S.map_extract(S.col(0, mi), S.col(1, I64))]), "map_extract", "Int64", "Int32")
    refuses(S.project(src, [S.map_extract(S.col(0, mi), S.lit(1, I64))]), "map_extract", "Int64", "Int32")
    refuses(S.project(src, [S.map_extract(S.col(0, mi), S.lit("1", STR))]), "map_extract", "Utf8", "Int32")
    refuses(S.project(src, [S.map_extract(S.col(2, MSI), S.col(1, I64))]), "map_extract", "Int64", "Utf8")
    md = S.map_type(S.decimal(10, 2), I64, True)
    refuses(S.project(S.scan([md]), [S.map_extract(S.col(0, md), S.lit(1, S.decimal(12, 2)))]), "map_extract", "key's type")
    # a Utf8 key that is neither a literal nor a column
    upper = S.scalar_func("upper", [S.col(3, STR)], STR)
    refuses(S.project(src, [S.map_extract(S.col(2, MSI), upper)]), "map_extract", "Utf8 COLUMN", ENGINE)
    # a Utf8 value is an output column, not an operand
    ms = S.map_type(I32, STR, True)
    look = S.map_extract(S.col(0, ms), S.lit(1, I32))
    assert "gathered" in accepts(S.project(S.scan([ms]), [look]))
    refuses(S.project(S.scan([ms]), [S.eq(look, S.lit("x", STR))]), "map_extract", "OUTPUT column", ENGINE)
    refuses(S.filter_(S.scan([ms]), S.is_not_null(look)), "map_extract", "OUTPUT column", ENGINE)
    refuses(S.project(S.scan([mi]), [S.scalar_func("map_extract", [S.col(0, mi)])]), "map_extract", "two arguments")


def test_createplan_under_an_aggregate_and_under_a_join():
    src = S.scan([MSI, I32])
    m = S.col(0, MSI)
    # the views are derived columns: inside an aggregate's chain they are refused in array_sort's wording …
    for name in ("map_keys", "map_values", "map_entries"):
        refuses(S.hash_agg(S.project(src, [size(FOUR[name](m))]), [], [S.sum_(S.col(0, I32), I64)]), name, "aggregate", ENGINE)
        refuses(S.hash_agg(S.project(src, [size(FOUR[name](m))]), [S.col(0, I32)], [S.count(S.col(0, I32))]), name, "aggregate", ENGINE)
    # … while under a join the side that holds them is materialised instead of fused, and runs
    other = S.scan([I32])
    for name in ("map_keys", "map_values", "map_entries"):
        side = S.project(src, [size(FOUR[name](m))])
        for build_side in (S.BUILD_LEFT, S.BUILD_RIGHT):
            assert "hash join" in accepts(S.hash_join(other, side, [S.col(0, I32)], [S.col(0, I32)], S.INNER, build_side))
            assert "hash join" in accepts(S.hash_join(side, other, [S.col(0, I32)], [S.col(0, I32)], S.INNER, build_side))
    # map_extract is a per-row loop like array_contains, which runs in both places today: so does map_extract (COMPAT §4)
    LI = S.list_type(I64, True)
    accepts(S.hash_agg(S.project(S.scan([LI]), [S.scalar_func("array_contains", [S.col(0, LI), S.lit(3, I64)], BOOL)]), [], [S.count(S.col(0, BOOL))]))
    look = S.map_extract(m, S.lit("k", STR))
    assert "agg" in accepts(S.hash_agg(S.project(src, [look]), [], [S.sum_(S.col(0, I64), I64)]))
    assert "agg" in accepts(S.hash_agg(S.project(src, [S.col(1, I32), look]), [S.col(0, I32)], [S.sum_(S.col(1, I64), I64)]))
    other64 = S.scan([I64])
    for build_side in (S.BUILD_LEFT, S.BUILD_RIGHT):
        assert "hash join" in accepts(S.hash_join(other64, S.project(src, [look]), [S.col(0, I64)], [S.col(0, I64)], S.INNER, build_side))
        assert "hash join" in accepts(S.hash_join(S.project(src, [look]), other64, [S.col(0, I64)], [S.col(0, I64)], S.INNER, build_side))


def test_a_wide_table_keeps_its_argument_slots():
    """a map's key and value columns are added behind every other column and only while they fit the kernel's 24 argument slots: a table that fills them
    passes its map through as before, and a lookup in that map is refused by name"""
    wide = [I64] * 23 + [MSI]
    m = S.col(23, MSI)
    accepts(S.project(S.scan(wide), [S.col(0, I64), m, size(m)]))
    refuses(S.project(S.scan(wide), [S.map_extract(m, S.lit("k", STR))]), "map_extract", "not addressable", ENGINE)
    fits = [I64] * 21 + [MSI]
    accepts(S.project(S.scan(fits), [S.map_extract(S.col(21, MSI), S.lit("k", STR))]))
    # struct fields and list elements keep the places they had: the maps' columns come last
    st = S.struct_type([("a", I32, True)])
    d = native.plan_codegen(S.project(S.scan([MSI, st]), [S.get_struct_field(S.col(1, st), 0)]).encode(), [False] * 2)
    assert "prm.in[2]" in d["source"] and "prm.in[4]" not in d["source"]


def test_a_plan_without_a_lookup_sees_the_table_it_saw_before():
    """a map's key and value columns are added only to the chains of a plan that holds a map_extract: every other plan over a table with a map column keeps the
    slots it left to derived columns and bloom filters — these plans fill the 24 and ran before maps were addressable"""
    from tests import bloom_model
    LI = S.list_type(I64, True)
    good = S.lit(bloom_model.Filter(1, 3, 2).serialize(), S.T_BINARY)
    mc = S.bloom_filter_might_contain
    # 22 columns (the list's elements among them) + a two-column derived list = 24
    lists = S.scan([I64] * 19 + [LI, MSI])
    accepts(S.project(lists, [S.sort_array(S.col(19, LI)), S.col(0, I64), S.col(20, MSI), size(S.col(20, MSI))]))
    accepts(S.project(lists, [S.map_keys(S.col(20, MSI))]))      # (the views need no virtual column either)
    # 22 columns + a one-column derived string + one bloom filter = 24
    strings = S.scan([I64] * 20 + [STR, MSI])
    rev = S.scalar_func("reverse", [S.col(20, STR)], STR)
    accepts(S.project(strings, [rev, S.col(21, MSI)]))
    accepts(S.project(S.filter_(strings, mc(good, S.col(0, I64))), [rev, S.col(21, MSI)]))
    # 23 columns + one bloom filter = 24; a second filter finds no slot, as before
    flat = S.scan([I64] * 22 + [MSI])
    one = mc(good, S.col(0, I64))
    accepts(S.project(S.filter_(flat, one), [S.col(22, MSI)]))
    refuses(S.project(S.filter_(S.scan([I64] * 23 + [MSI]), one), [S.col(0, I64)]), "might_contain", "slot")
    # under a join too: its sides' column counts are what they were
    assert "hash join" in accepts(S.hash_join(S.scan([I64]), S.project(lists, [S.col(0, I64), size(S.sort_array(S.col(19, LI)))]), [S.col(0, I64)], [S.col(0, I64)], S.INNER, S.BUILD_LEFT))
    # the same tables with a lookup: the two columns are there, and what no longer fits is refused by the usual names
    fits = S.scan([I64] * 21 + [MSI])      # 22 columns + the map's two = 24
    accepts(S.project(fits, [S.map_extract(S.col(21, MSI), S.lit("k", STR))]))
    refuses(S.project(S.filter_(fits, one), [S.map_extract(S.col(21, MSI), S.lit("k", STR))]), "might_contain", "slot")
    refuses(S.project(flat, [S.map_extract(S.col(22, MSI), S.lit("k", STR))]), "map_extract", "not addressable", ENGINE)
    refuses(S.project(lists, [S.map_extract(S.col(20, MSI), S.lit("k", STR)), S.sort_array(S.col(19, LI))]), "too many scan columns")
    # … and the generated source of a plan without a lookup does not move when the table holds a map
    src = lambda fields, e: native.plan_codegen(S.project(S.scan(fields), [e]).encode(), [False] * len(fields))["source"]
    text = src([LI, MSI], size(S.sort_array(S.col(0, LI))))      # columns: the list, the map, the list's elements, the sorted list, its elements
    assert "prm.in[3]" in text and "prm.in[5]" not in text


def test_what_stays_refused_over_a_map_column():
    m = S.col(0, MSI)
    for name, e in (("array_sort", S.sort_array(m)), ("array_distinct", S.array_distinct(m)), ("array_min", S.array_min(m)), ("array_max", S.array_max(m)),
                    ("spark_array_position", S.array_position(m, S.lit(None, I64)))):
        refuses(S.project(S.scan([MSI]), [e]), name, "of a map is not supported")
    refuses(S.project(S.scan([I64]), [size(S.col(0, I64))]), "size", "list / map COLUMN")
    # Explode of a map is never sent and stays refused
    ok, _ = native.check_plan(S.explode(S.scan([MSI]), m, []).encode())
    assert not ok


def test_serde_helpers_encode_what_the_jvm_sends():
    m, k = S.col(0, MSI), S.col(1, STR)
    f = S.scalar_func
    assert S.map_keys(m).encode() == f("map_keys", [m]).encode()
    assert S.map_values(m).encode() == f("map_values", [m]).encode()
    assert S.map_entries(m).encode() == f("map_entries", [m]).encode()
    assert S.map_extract(m, k).encode() == f("map_extract", [m, k]).encode()
    # ScalarFunc{func = 1, args = 2} and no return type (field 3): the name, then one length-delimited argument per child
    arg = lambda x: b"\x12" + bytes([len(x.encode())]) + x.encode()
    assert len(m.encode()) < 128 and len(k.encode()) < 128
    assert S.map_keys(m).encode().endswith(b"\x0a\x08map_keys" + arg(m))
    assert S.map_values(m).encode().endswith(b"\x0a\x0amap_values" + arg(m))
    assert S.map_entries(m).encode().endswith(b"\x0a\x0bmap_entries" + arg(m))
    assert S.map_extract(m, k).encode().endswith(b"\x0a\x0bmap_extract" + arg(m) + arg(k))


def test_every_plan_of_the_gpu_tests_compiles_for_gfx950():
    from tests import test_map_fn_gpu as G
    names = []
    for name, plan in G.every_plan():
        ok, msg = native.check_plan(plan.encode())
        assert ok, (name, msg)
        native.compile_plan(plan.encode())      # (raises with hiprtc's log)
        names.append(name)
    assert len(names) == len(set(names)) >= 30


def test_header_under_the_sanitizers(tmp_path):
    """tests/host/map_fn_check.cpp: map_fn.hpp's entry search and utf8_eq_rows over random maps against std::find_if, as a stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this machine's compiler cannot link the sanitizer runtimes")
    exe = tmp_path / "map_fn_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + flags + ["-I", _CSRC, "-o", str(exe), os.path.join(_HERE, "host", "map_fn_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
