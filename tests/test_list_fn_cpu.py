"""sort_array, array_distinct, array_min / array_max and array_position without a GPU: the model of tests/list_fn_model.py against Spark's answers for the
reference's SQL tests (tests/golden/list_fn_cases.json); csrc/device/list_fn.hpp on the host (comet_list_fn_host) against the model; what createPlan accepts
and what it refuses by name; the serde helpers' bytes; and the header under AddressSanitizer / UBSan as a stand-alone program."""
import json
import os
import random
import shutil
import subprocess

import pytest

from datafusion_comet_amd import native, serde as S
from tests import list_fn_model as M

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "datafusion-comet_amd", "csrc")
I32, I64, STR = S.T_INT32, S.T_INT64, S.T_STRING
D38 = 10 ** 38 - 1

with open(os.path.join(_HERE, "golden", "list_fn_cases.json")) as fh:
    GOLDEN = json.load(fh)["cases"]


def test_the_model_reproduces_sparks_answers():
    seen = set()
    for c in GOLDEN:
        rows, fn = c["input"], c["fn"]
        seen.add(fn)
        if fn == "sort_array":
            got = [M.sort_array(r, c["ascending"]) for r in rows]
        elif fn == "array_position":
            keys = c["keys"] if "keys" in c else [c["key"]] * len(rows)
            got = [M.array_position(r, k) for r, k in zip(rows, keys)]
        else:
            got = [getattr(M, fn)(r) for r in rows]
        assert got == c["want"], c
    assert seen == {"sort_array", "array_distinct", "array_min", "array_max", "array_position"}


# element layouts of comet_list_fn_host → a generator of model values (Utf8 as bytes)
STRS = [b"", b"a", b"a\0", b"ab", "日本".encode(), "日本語".encode(), b"\x7f", b"\x80", b"\xff", b"shared prefix 1", b"shared prefix 2", b"shared prefix", b"shared p"]
HOST_KINDS = {
    0: [False, True], 1: [-128, -1, 0, 1, 127], 2: [-32768, -1, 0, 1, 32767], 4: [-2 ** 31, -1, 0, 1, 2 ** 31 - 1], 8: [-2 ** 63, -2, -1, 0, 1, 2, 2 ** 63 - 1],
    16: [-D38, -2 ** 64 - 1, -2 ** 64, -1, 0, 1, 2 ** 63, 2 ** 64, 2 ** 64 + 1, D38], 32: STRS,
}


def host_sort(kind, arr, flags):
    return [arr[i] for i in native.list_fn_host(kind, arr, 0, flags)]


def host_distinct(kind, arr):
    return [v for v, k in zip(arr, native.list_fn_host(kind, arr, 1)) if k]


@pytest.mark.parametrize("kind", list(HOST_KINDS))
def test_host_code_agrees_with_the_model_on_random_lists(kind):
    rng = random.Random(kind)
    dom = HOST_KINDS[kind]
    for trial in range(400):
        n = rng.randrange(0, 10) if trial % 20 else rng.randrange(60, 140)
        arr = [None if rng.random() < 0.15 else rng.choice(dom) for _ in range(n)]
        for flags in range(4):
            assert host_sort(kind, arr, flags) == M.sort_array(arr, not flags & 1, bool(flags & 2)), (arr, flags)
        assert host_distinct(kind, arr) == M.array_distinct(arr), arr


def test_host_code_on_the_type_extremes():
    assert host_sort(8, [2 ** 63 - 1, None, -2 ** 63, 0], 0) == [None, -2 ** 63, 0, 2 ** 63 - 1]
    assert host_sort(8, [2 ** 63 - 1, None, -2 ** 63, 0], 3) == [2 ** 63 - 1, 0, -2 ** 63, None]
    assert host_sort(16, [D38, -D38, 2 ** 64, -2 ** 64, 0, 2 ** 63], 0) == [-D38, -2 ** 64, 0, 2 ** 63, 2 ** 64, D38]
    assert host_distinct(16, [D38, -D38, D38, 2 ** 64, 2 ** 64 + 1, 2 ** 64]) == [D38, -D38, 2 ** 64, 2 ** 64 + 1]
    # Utf8: unsigned bytes (0x80 and above sort behind ASCII), shared prefixes longer than 8 bytes, a value that is a prefix of another, "" beside NULL
    s = [b"\xe6\x97\xa5", b"z", b"\x80", b"\x7f", b"prefix of nine+ bytes b", b"prefix of nine+ bytes a", b"prefix of nine+ bytes", b"", None, b"a\0", b"a"]
    assert host_sort(32, s, 0) == [None, b"", b"a", b"a\0", b"prefix of nine+ bytes", b"prefix of nine+ bytes a", b"prefix of nine+ bytes b", b"z", b"\x7f", b"\x80", b"\xe6\x97\xa5"]
    assert host_sort(32, s, 1 | 2) == host_sort(32, s, 0)[::-1]
    assert host_distinct(32, [b"", None, b"", None, b"a", b"a\0", b"a"]) == [b"", None, b"a", b"a\0"]
    # equal values keep their order in both directions: the sort answers with positions
    assert native.list_fn_host(4, [5, 5, None, 5, None], 0) == [2, 4, 0, 1, 3] and native.list_fn_host(4, [5, 5, None, 5, None], 0, 1 | 2) == [0, 1, 3, 2, 4]
    assert native.list_fn_host(8, [], 0) == [] and native.list_fn_host(8, [], 1) == []


# ---- createPlan ----
ELEMS = {"bool": S.T_BOOL, "i8": S.T_INT8, "i16": S.T_INT16, "i32": I32, "i64": I64, "date": S.T_DATE, "ts": S.T_TIMESTAMP, "ntz": S.DataType(S.TIMESTAMP_NTZ),
         "dec10_2": S.decimal(10, 2), "dec38_0": S.decimal(38, 0), "str": STR}


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
    et = ELEMS[kind]
    lt = S.list_type(et, True)
    l, k = S.col(0, lt), S.col(1, et)
    src = S.scan([lt, et])
    for e in (S.sort_array(l), S.sort_array(l, False), S.array_distinct(l), S.array_position(l, S.lit(None, et))):
        accepts(S.project(src, [e]))
    for asc in ("ASC", "DESC"):
        for nulls in ("NULLS FIRST", "NULLS LAST"):
            accepts(S.project(src, [S.scalar_func("array_sort", [l, S.lit(asc, STR), S.lit(nulls, STR)])]))
    if kind == "str":
        accepts(S.project(src, [S.array_position(l, S.lit("x", STR))]))
        refuses(S.project(src, [S.array_min(l)]), "array_min", "Utf8")
        refuses(S.project(src, [S.array_max(l)]), "array_max", "Utf8")
        refuses(S.project(src, [S.array_position(l, k)]), "spark_array_position", "literal key")
    else:
        for e in (S.array_min(l), S.array_max(l), S.array_position(l, k)):
            accepts(S.project(src, [e]))


def test_createplan_accepts_derived_and_chained_lists():
    LS, LI = S.list_type(STR, True), S.list_type(I64, True)
    src = S.scan([STR, LI, LS, I64])
    s, li, ls, k = S.col(0, STR), S.col(1, LI), S.col(2, LS), S.col(3, I64)
    sp = S.scalar_func("split", [s, S.lit(",", STR), S.lit(-1, I32)], S.list_type(STR, False))
    L = lambda v: S.lit(v, I32)
    exprs = [S.sort_array(sp), S.array_distinct(S.sort_array(li)), S.scalar_func("size", [S.array_distinct(li)], I32), S.list_extract(S.sort_array(ls), L(0)),
             S.list_extract(S.sort_array(li), L(-1), one_based=True), S.array_max(S.array_distinct(li)), S.scalar_func("array_contains", [S.sort_array(li), S.lit(3, I64)], S.T_BOOL),
             S.array_position(sp, S.lit("x", STR)), S.sort_array(S.scalar_func("regexp_extract_all", [s, S.lit("(\\d+)", STR), S.lit(1, I32)], LS))]
    for e in exprs:
        accepts(S.project(src, [e]))
    accepts(S.project(src, exprs))
    accepts(S.project(S.filter_(src, S.gt(S.array_position(li, k), S.lit(0, I64))), [S.sort_array(li)]))
    accepts(S.explode(S.project(src, [S.sort_array(li), k]), S.col(0, LI), [S.col(1, I64)]))
    # two equal calls share one derived column: sort(li), distinct(sort(li))
    plan = S.project(src, [S.sort_array(li), S.array_distinct(S.sort_array(li)), S.list_extract(S.sort_array(li), L(0))])
    assert native.plan_codegen(plan.encode(), [False] * 4)["derived"] == 2
    # over a collect below the Projection, in one plan
    agg = S.hash_agg(S.scan([I32, I64]), [S.col(0, I32)], [S.collect_list(S.col(1, I64), I64), S.collect_set(S.col(1, I64), I64)])
    LV = S.list_type(I64, False)
    accepts(S.project(agg, [S.col(0, I32), S.sort_array(S.col(1, LV)), S.array_min(S.col(2, LV)), S.array_distinct(S.col(1, LV))]))


FUNCS = {"array_sort": lambda x: S.sort_array(x), "array_distinct": S.array_distinct, "array_min": S.array_min, "array_max": S.array_max,
         "spark_array_position": lambda x: S.array_position(x, S.lit(None, I64))}


@pytest.mark.parametrize("name", list(FUNCS))
def test_createplan_refuses_by_name(name):
    fn = FUNCS[name]
    for et, word in ((S.T_FLOAT, "Float32"), (S.T_DOUBLE, "Float64"), (S.T_BINARY, "Binary")):
        lt = S.list_type(et, True)
        e = S.array_position(S.col(0, lt), S.lit(None, et)) if name == "spark_array_position" else fn(S.col(0, lt))
        refuses(S.project(S.scan([lt]), [e]), name, word)
    # struct, list and map elements; a map argument; something that is neither a list column nor a derived list
    st = S.struct_type([("a", I32, True)])
    for lt in (S.list_type(st, True), S.list_type(S.list_type(I32, True), True)):
        refuses(S.project(S.scan([lt]), [fn(S.col(0, lt))]), name)
    mt = S.map_type(I32, I32, True)
    refuses(S.project(S.scan([mt]), [fn(S.col(0, mt))]), name, "map")
    refuses(S.project(S.scan([I64]), [fn(S.col(0, I64))]), name)
    LI = S.list_type(I64, True)
    refuses(S.project(S.scan([LI]), [fn(S.case_when([(S.is_not_null(S.col(0, LI)), S.col(0, LI))], S.col(0, LI)))]), name)


def test_createplan_refuses_the_other_array_sort_arguments_and_fused_chains():
    LI = S.list_type(I64, True)
    l = S.col(0, LI)
    src = S.scan([LI, STR])
    for args in ([l, S.lit("UP", STR), S.lit("NULLS FIRST", STR)], [l, S.lit("ASC", STR), S.lit("NULLS", STR)], [l, S.col(1, STR), S.lit("NULLS FIRST", STR)],
                 [l, S.lit("ASC", STR), S.lit(None, STR)], [l, S.lit("ASC", STR)], [l]):
        refuses(S.project(src, [S.scalar_func("array_sort", args)]), "array_sort")
    # a derived list inside an aggregate's chain: its own wording
    size = lambda x: S.scalar_func("size", [x], I32)
    refuses(S.hash_agg(S.project(src, [size(S.sort_array(l))]), [], [S.sum_(S.col(0, I32), I64)]), "array_sort", "aggregate")
    refuses(S.hash_agg(S.project(src, [size(S.array_distinct(l))]), [S.col(0, I32)], [S.count(S.col(0, I32))]), "array_distinct", "aggregate")
    # … while a join does not refuse: the fold of its side's chain fails with a wording of its own, which makes the join materialise that side instead of fusing it
    other = S.scan([I32])
    for e in (S.sort_array(l), S.array_distinct(l)):
        side = S.project(src, [size(e)])
        for build_side in (S.BUILD_LEFT, S.BUILD_RIGHT):
            assert "hash join" in accepts(S.hash_join(other, side, [S.col(0, I32)], [S.col(0, I32)], S.INNER, build_side))
            assert "hash join" in accepts(S.hash_join(side, other, [S.col(0, I32)], [S.col(0, I32)], S.INNER, build_side))


def test_serde_helpers_encode_what_the_jvm_sends():
    LI = S.list_type(I64, True)
    l, k = S.col(0, LI), S.col(1, I64)
    f = S.scalar_func
    assert S.sort_array(l).encode() == f("array_sort", [l, S.lit("ASC", STR), S.lit("NULLS FIRST", STR)]).encode()
    assert S.sort_array(l, False).encode() == f("array_sort", [l, S.lit("DESC", STR), S.lit("NULLS LAST", STR)]).encode()
    assert S.array_distinct(l).encode() == f("array_distinct", [l]).encode()
    assert S.array_min(l).encode() == f("array_min", [l]).encode() and S.array_max(l).encode() == f("array_max", [l]).encode()
    assert S.array_position(l, k).encode() == f("spark_array_position", [l, k]).encode()
    # ScalarFunc{func = 1, args = 2} and no return type (field 3): the name, then one length-delimited argument per child
    b = S.array_min(l).encode()
    body = b"\x0a\x09array_min" + b"\x12" + bytes([len(l.encode())]) + l.encode()
    assert b.endswith(body)
    assert b"NULLS LAST" in S.sort_array(l, False).encode() and b"DESC" in S.sort_array(l, False).encode()


def test_header_under_the_sanitizers(tmp_path):
    """tests/host/list_fn_check.cpp: list_fn.hpp's rank, keep and list search over random lists against std::stable_sort, as a stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this machine's compiler cannot link the sanitizer runtimes")
    exe = tmp_path / "list_fn_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + flags + ["-I", _CSRC, "-o", str(exe), os.path.join(_HERE, "host", "list_fn_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
