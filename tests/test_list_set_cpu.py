"""array_union, array_intersect, array_except and arrays_overlap without a GPU: the model of tests/list_set_model.py against Spark's answers for the reference's
SQL tests (tests/golden/list_set_cases.json); csrc/device/list_set.hpp on the host (comet_list_set_host) against the model; what createPlan accepts and what it
refuses by name; the serde helpers' bytes; the compatibility sheet; and the header under AddressSanitizer / UBSan as a stand-alone program."""
import json
import os
import random
import shutil
import subprocess

import pytest

from datafusion_comet_amd import native, serde as S
from tests import list_set_model as M

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "datafusion-comet_amd", "csrc")
I32, I64, STR = S.T_INT32, S.T_INT64, S.T_STRING
D38 = 10 ** 38 - 1
OPS = {"array_union": 0, "array_intersect": 1, "array_except": 2, "arrays_overlap": 3}      # csrc/device/list_set.hpp LS_UNION …

with open(os.path.join(_HERE, "golden", "list_set_cases.json")) as fh:
    GOLDEN = json.load(fh)["cases"]


def test_the_model_reproduces_sparks_answers():
    seen, types = set(), set()
    for c in GOLDEN:
        assert len(c["a"]) == len(c["b"]) == len(c["want"]), c
        seen.add(c["fn"])
        types.add(c["type"])
        assert [getattr(M, c["fn"])(a, b) for a, b in zip(c["a"], c["b"])] == c["want"], c
    assert seen == set(OPS)
    assert types == {"int", "bigint", "boolean", "tinyint", "smallint", "decimal(10,2)", "date", "timestamp", "string"}
    # the intersections whose right side is the longer one stand unsorted: a result in the longer side's order, or in value order, would not pass
    assert any(c["fn"] == "array_intersect" and [2, 1] in c["want"] and [3, 1, 2] in c["b"] for c in GOLDEN)


# element layouts of comet_list_set_host → a generator of model values (Utf8 as bytes), as tests/test_list_fn_cpu.py has them
STRS = [b"", b"a", b"a\0", b"ab", "日本".encode(), "日本語".encode(), b"\x7f", b"\x80", b"\xff", b"shared prefix 1", b"shared prefix 2", b"shared prefix", b"shared p"]
HOST_KINDS = {
    0: [False, True], 1: [-128, -1, 0, 1, 127], 2: [-32768, -1, 0, 1, 32767], 4: [-2 ** 31, -1, 0, 1, 2 ** 31 - 1], 8: [-2 ** 63, -2, -1, 0, 1, 2, 2 ** 63 - 1],
    16: [-D38, -2 ** 64 - 1, -2 ** 64, -1, 0, 1, 2 ** 63, 2 ** 64, 2 ** 64 + 1, D38], 32: STRS,
}


def host(fn, kind, a, b):
    got = native.list_set_host(OPS[fn], kind, a, b)
    return got if fn == "arrays_overlap" else [(a + b)[i] for i in got]


@pytest.mark.parametrize("kind", list(HOST_KINDS))
def test_host_code_agrees_with_the_model_on_random_pairs(kind):
    rng = random.Random(100 + kind)
    dom = HOST_KINDS[kind]
    for trial in range(400):
        def one():
            n = rng.randrange(0, 10) if trial % 20 else rng.randrange(60, 140)
            p_null = rng.choice([0.0, 0.15])
            return [None if rng.random() < p_null else rng.choice(dom) for _ in range(n)]
        a, b = one(), one()
        for fn in OPS:
            assert host(fn, kind, a, b) == getattr(M, fn)(a, b), (fn, a, b)


def test_host_code_on_the_type_extremes():
    MAX, MIN = 2 ** 63 - 1, -2 ** 63
    assert host("array_intersect", 8, [MAX, None, MIN, 0], [MIN, MAX, 1]) == [MAX, MIN]
    assert host("array_except", 8, [MAX, None, MIN, 0, None], [MIN, 5]) == [MAX, None, 0]
    assert host("array_union", 16, [D38, -D38, 2 ** 64], [2 ** 64 + 1, -D38, 2 ** 64, D38 - 1]) == [D38, -D38, 2 ** 64, 2 ** 64 + 1, D38 - 1]
    assert host("arrays_overlap", 16, [2 ** 64], [2 ** 64 + 1, 0]) is False and host("arrays_overlap", 16, [2 ** 64, -1], [2 ** 63, 2 ** 64]) is True
    # Utf8: shared prefixes longer than 8 bytes are decided on the bytes, a value that is a prefix of another, "" beside NULL
    p = b"prefix of nine+ bytes"
    a = [p + b" b", p, b"", None, b"a\0", b"a", p + b" a"]
    assert host("array_intersect", 32, a, [p + b" a", b"a", None, p + b" c"]) == [None, b"a", p + b" a"]
    assert host("array_intersect", 32, a, [b"", p]) == [p, b""]
    assert host("array_except", 32, a, [b"", p + b" b", b"a\0"]) == [p, None, b"a", p + b" a"]
    assert host("array_except", 32, [b"", None], [None]) == [b""] and host("array_except", 32, [b"", None], [b""]) == [None]
    assert host("array_union", 32, [b"", None, b""], [None, b"a\0", b"a", b""]) == [b"", None, b"a\0", b"a"]
    assert host("arrays_overlap", 32, [b""], [None]) is None and host("arrays_overlap", 32, [b""], [None, b""]) is True
    assert host("arrays_overlap", 32, [p + b" a"], [p + b" b", p]) is False
    # an empty side answers false even beside [NULL]; two empty sides give empty results
    assert host("arrays_overlap", 8, [], [None]) is False and host("arrays_overlap", 8, [None], []) is False
    for fn in ("array_union", "array_intersect", "array_except"):
        assert host(fn, 8, [], []) == []
    # picks: union reaches into b behind a's elements
    assert native.list_set_host(0, 4, [5, 5, None], [None, 7, 5]) == [0, 2, 4] and native.list_set_host(1, 4, [2, 1], [3, 1, 2]) == [0, 1]


# ---- createPlan ----
ELEMS = {"bool": S.T_BOOL, "i8": S.T_INT8, "i16": S.T_INT16, "i32": I32, "i64": I64, "date": S.T_DATE, "ts": S.T_TIMESTAMP, "ntz": S.DataType(S.TIMESTAMP_NTZ),
         "dec10_2": S.decimal(10, 2), "dec38_0": S.decimal(38, 0), "str": STR}
FUNCS = {"array_union": S.array_union, "array_intersect": S.array_intersect, "array_except": S.array_except, "spark_arrays_overlap": S.arrays_overlap}


def accepts(plan):
    ok, msg = native.check_plan(plan.encode())
    assert ok, msg
    return msg


def refuses(plan, *words):
    ok, msg = native.check_plan(plan.encode())
    assert not ok, msg
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("kind", list(ELEMS))
def test_createplan_accepts_each_function_over_each_type(kind):
    lt = S.list_type(ELEMS[kind], True)
    a, b = S.col(0, lt), S.col(1, lt)
    src = S.scan([lt, lt])
    for fn in FUNCS.values():
        accepts(S.project(src, [fn(a, b)]))
        accepts(S.project(src, [fn(a, a)]))
    accepts(S.project(src, [fn(a, b) for fn in FUNCS.values()]))


def test_createplan_accepts_derived_and_chained_lists():
    LS, LI = S.list_type(STR, True), S.list_type(I64, True)
    MT = S.map_type(I64, STR, True)
    src = S.scan([STR, LI, LS, LI, MT])
    s, li, ls, lj, m = S.col(0, STR), S.col(1, LI), S.col(2, LS), S.col(3, LI), S.col(4, MT)
    sp = S.scalar_func("split", [s, S.lit(",", STR), S.lit(-1, I32)], S.list_type(STR, False))
    size = lambda x: S.scalar_func("size", [x], I32)
    exprs = [S.array_union(sp, ls), S.arrays_overlap(ls, sp), S.array_intersect(S.sort_array(li), lj), S.array_except(li, S.array_distinct(lj)), S.array_union(S.map_keys(m), li),
             S.arrays_overlap(S.map_values(m), sp), S.array_except(S.array_union(li, lj), S.array_intersect(li, lj)), S.arrays_overlap(S.array_except(li, lj), lj),
             size(S.array_union(li, lj)), S.scalar_func("array_contains", [S.array_except(li, lj), S.lit(3, I64)], S.T_BOOL), S.sort_array(S.array_intersect(li, lj)),
             S.list_extract(S.array_union(ls, ls), S.lit(0, I32))]
    for e in exprs:
        accepts(S.project(src, [e]))
    for some in (exprs[:4], exprs[6:11]):      # (all twelve at once need more than a pipeline's 24 column slots)
        accepts(S.project(src, some))
    accepts(S.project(S.filter_(src, S.arrays_overlap(li, lj)), [S.array_union(li, lj)]))
    accepts(S.explode(S.project(src, [S.array_intersect(li, lj), s]), S.col(0, LI), [S.col(1, STR)]))
    # identical calls share one derived column — the same op, src and src2; swapped arguments are another column
    plan = S.project(src, [S.array_union(li, lj), size(S.array_union(li, lj)), S.array_distinct(S.array_union(li, lj))])
    assert native.plan_codegen(plan.encode(), [False] * 5)["derived"] == 2
    plan = S.project(src, [S.array_except(li, lj), S.array_except(lj, li), S.arrays_overlap(li, lj), S.arrays_overlap(li, lj)])
    assert native.plan_codegen(plan.encode(), [False] * 5)["derived"] == 3
    # over a collect below the Projection, in one plan
    agg = S.hash_agg(S.scan([I32, I64]), [S.col(0, I32)], [S.collect_list(S.col(1, I64), I64), S.collect_set(S.col(1, I64), I64)])
    LV = S.list_type(I64, False)
    accepts(S.project(agg, [S.col(0, I32), S.array_except(S.col(1, LV), S.col(2, LV)), S.arrays_overlap(S.col(1, LV), S.col(2, LV))]))


def test_a_set_function_costs_the_column_slots_of_its_result():
    """its intermediates (distinct(a), sorted b, the concatenation) are no columns of the chain: 11 source lists and their element columns leave two slots of 24"""
    LI = S.list_type(I64, True)
    src = S.scan([LI] * 11)
    a, b = S.col(0, LI), S.col(1, LI)
    for fn in (S.array_union, S.array_intersect, S.array_except):
        accepts(S.project(src, [fn(a, b)]))
    accepts(S.project(src, [S.arrays_overlap(a, b), S.arrays_overlap(b, a)]))
    refuses(S.project(src, [S.array_union(a, b), S.arrays_overlap(a, b)]), "too many scan columns")


@pytest.mark.parametrize("name", list(FUNCS))
def test_createplan_refuses_by_name(name):
    fn = FUNCS[name]
    for et, word in ((S.T_FLOAT, "Float32"), (S.T_DOUBLE, "Float64"), (S.T_BINARY, "Binary")):
        lt = S.list_type(et, True)
        refuses(S.project(S.scan([lt, lt]), [fn(S.col(0, lt), S.col(1, lt))]), name, word)
    # struct and list elements; a map argument; something that is neither a list column nor a derived list, on either side
    st = S.struct_type([("a", I32, True)])
    for lt in (S.list_type(st, True), S.list_type(S.list_type(I32, True), True)):
        refuses(S.project(S.scan([lt, lt]), [fn(S.col(0, lt), S.col(1, lt))]), name)
    LI, mt = S.list_type(I64, True), S.map_type(I64, I64, True)
    l, m = S.col(0, LI), S.col(1, mt)
    refuses(S.project(S.scan([LI, mt]), [fn(l, m)]), name, "map")
    refuses(S.project(S.scan([LI, mt]), [fn(m, l)]), name, "map")
    refuses(S.project(S.scan([LI, I64]), [fn(l, S.col(1, I64))]), name)
    computed = S.case_when([(S.is_not_null(l), l)], l)
    refuses(S.project(S.scan([LI]), [fn(l, computed)]), name, "computed array")
    refuses(S.project(S.scan([LI]), [fn(computed, l)]), name, "computed array")
    # a wrong argument count
    rt = S.T_BOOL if name == "spark_arrays_overlap" else None
    for args in ([l], [l, l, l], []):
        refuses(S.project(S.scan([LI]), [S.scalar_func(name, args, rt)]), name, "2 arguments")
    # two element types that are not exactly equal: both are named
    for ta, tb in ((I32, I64), (S.decimal(10, 2), S.decimal(10, 3)), (S.decimal(10, 2), S.decimal(12, 2)), (S.T_DATE, I32), (S.T_TIMESTAMP, S.DataType(S.TIMESTAMP_NTZ)), (STR, I64)):
        la, lb = S.list_type(ta, True), S.list_type(tb, True)
        ok, msg = native.check_plan(S.project(S.scan([la, lb]), [fn(S.col(0, la), S.col(1, lb))]).encode())
        assert not ok and name in msg and "must be equal" in msg, msg
        ok2, msg2 = native.check_plan(S.project(S.scan([la, la]), [fn(S.col(0, la), S.col(1, la))]).encode())
        ok3, msg3 = native.check_plan(S.project(S.scan([lb, lb]), [fn(S.col(0, lb), S.col(1, lb))]).encode())
        assert ok2 and ok3, (msg2, msg3)
    la, lb = S.list_type(S.decimal(10, 2), True), S.list_type(S.decimal(12, 3), True)
    refuses(S.project(S.scan([la, lb]), [fn(S.col(0, la), S.col(1, lb))]), name, "10", "2", "12", "3")


def test_createplan_refuses_the_wrong_return_type_and_fused_chains():
    LI = S.list_type(I64, True)
    a, b = S.col(0, LI), S.col(1, LI)
    src = S.scan([LI, LI])
    for rt in (I32, STR, None):
        refuses(S.project(src, [S.scalar_func("spark_arrays_overlap", [a, b], rt)]), "spark_arrays_overlap", "Boolean")
    # inside an aggregate's chain: its own wording
    size = lambda x: S.scalar_func("size", [x], I32)
    for name, fn in FUNCS.items():
        e = S.if_(fn(a, b), S.lit(1, I32), S.lit(0, I32)) if name == "spark_arrays_overlap" else size(fn(a, b))
        refuses(S.hash_agg(S.project(src, [e]), [], [S.sum_(S.col(0, I32), I64)]), name, "aggregate", "project it below")
        refuses(S.hash_agg(S.project(src, [e]), [S.col(0, I32)], [S.count(S.col(0, I32))]), name, "aggregate")
        # … while a join does not refuse: the fold of its side's chain fails with a wording of its own, which makes the join materialise that side
        other = S.scan([I32])
        side = S.project(src, [e])
        for build_side in (S.BUILD_LEFT, S.BUILD_RIGHT):
            assert "hash join" in accepts(S.hash_join(other, side, [S.col(0, I32)], [S.col(0, I32)], S.INNER, build_side))
            assert "hash join" in accepts(S.hash_join(side, other, [S.col(0, I32)], [S.col(0, I32)], S.INNER, build_side))


def test_serde_helpers_encode_what_the_jvm_sends():
    LI = S.list_type(I64, True)
    a, b = S.col(0, LI), S.col(1, LI)
    f = S.scalar_func
    assert S.array_union(a, b).encode() == f("array_union", [a, b]).encode()
    assert S.array_intersect(a, b).encode() == f("array_intersect", [a, b]).encode()
    assert S.array_except(a, b).encode() == f("array_except", [a, b]).encode()
    assert S.arrays_overlap(a, b).encode() == f("spark_arrays_overlap", [a, b], S.T_BOOL).encode()
    # ScalarFunc{func = 1, args = 2, return_type = 3}: the name, one length-delimited argument per child, and a return type for the overlap only
    args = b"".join(b"\x12" + bytes([len(x.encode())]) + x.encode() for x in (a, b))
    assert S.array_union(a, b).encode().endswith(b"\x0a\x0barray_union" + args)
    ov = S.arrays_overlap(a, b).encode()
    rt = S.T_BOOL.encode()
    assert ov.endswith(b"\x0a\x14spark_arrays_overlap" + args + b"\x1a" + bytes([len(rt)]) + rt)
    assert S.array_union(a, b).encode() != S.array_union(b, a).encode()


def test_the_sheet_lists_the_four_classes_as_accepted():
    from tools import compat_sheet
    text = compat_sheet.render()
    for cls in ("ArrayUnion", "ArraysOverlap", "ArrayIntersect", "ArrayExcept"):
        assert "spark.comet.expression.%s.enabled=false" % cls not in text, cls
        assert cls in text
    with open(os.path.join(_HERE, "..", "COMPAT.md")) as fh:
        assert fh.read() == text


def test_header_under_the_sanitizers(tmp_path):
    """tests/host/list_set_check.cpp: list_set.hpp's find, member flags, overlap row function and concatenation over random lists against a naive O(n·m) check,
    as a stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this machine's compiler cannot link the sanitizer runtimes")
    exe = tmp_path / "list_set_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + flags + ["-I", _CSRC, "-o", str(exe), os.path.join(_HERE, "host", "list_set_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
