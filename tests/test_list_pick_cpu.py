"""array_remove, array_compact, slice, reverse of an array and array_join without a GPU: the model of tests/list_pick_model.py against Spark's answers for the
reference's SQL tests and every slice edge (tests/golden/list_pick_cases.json); csrc/device/list_pick.hpp on the host (comet_list_pick_host) against the model;
what createPlan accepts and what it refuses by name; the serde helpers' bytes; the compatibility sheet; and the header under AddressSanitizer / UBSan as a
stand-alone program."""
import json
import os
import random
import shutil
import subprocess

import pytest

from datafusion_comet_amd import native, serde as S
from tests import list_pick_model as M
from tests.test_list_fn_gpu import KINDS

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "datafusion-comet_amd", "csrc")
I32, I64, STR = S.T_INT32, S.T_INT64, S.T_STRING
REMOVE, COMPACT, SLICE, REVERSE, JOIN = range(5)      # csrc/device/list_pick.hpp LP_REMOVE …
NAMES = ("array_remove_all", "array_compact", "spark_array_slice", "array_reverse", "array_to_string")

with open(os.path.join(_HERE, "golden", "list_pick_cases.json"), encoding="utf-8") as fh:
    GOLDEN = json.load(fh)["cases"]


def per_row(c, name):
    v = c[name]
    return v if isinstance(v, list) else [v] * len(c["arr"])


def model_answers(c):
    fn = c["fn"]
    if fn == "array_remove":
        return [M.array_remove(a, k) for a, k in zip(c["arr"], per_row(c, "key"))]
    if fn == "slice":
        return [M.slice_(a, s, n) for a, s, n in zip(c["arr"], per_row(c, "start"), per_row(c, "length"))]
    if fn == "array_join":
        return [M.array_join(a, c["delimiter"], c.get("replacement")) for a in c["arr"]]
    return [getattr(M, fn)(a) for a in c["arr"]]


def test_the_model_reproduces_sparks_answers():
    seen = set()
    for c in GOLDEN:
        assert len(c["arr"]) == len(c["want"]), c
        seen.add(c["fn"])
        assert model_answers(c) == c["want"], c
    assert seen == {"array_remove", "slice", "array_join", "array_compact", "array_reverse"}
    # every slice edge stands in the file: (n, start, length) → what it is
    edges = {(len(a), s, n) for c in GOLDEN if c["fn"] == "slice" for a, s, n in zip(c["arr"], per_row(c, "start"), per_row(c, "length")) if a is not None}
    assert any(s > n for n, s, _ in edges if n > 0), "a start past the end"
    assert any(s < -n for n, s, _ in edges if n > 0), "a negative start before the beginning"
    assert any(ln == 0 for _, _, ln in edges) and any(0 < s <= n and s - 1 + ln > n for n, s, ln in edges), "length 0, and a clamped length"
    assert any(n > 0 and s == -n for n, s, _ in edges) and any(n == 0 and s > 0 for n, s, _ in edges) and any(n == 0 and s < 0 for n, s, _ in edges), "start = -n, and n = 0"


# kind of tests/test_list_fn_gpu.KINDS → the element layout of comet_list_pick_host
HOST_KIND = {"bool": 0, "i8": 1, "i16": 2, "i32": 4, "i64": 8, "date": 4, "ts": 8, "ntz": 8, "dec10_2": 16, "dec38_0": 16, "str": 32}
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 5000)


def raw(kind, v):
    return v.encode() if kind == "str" and v is not None else v


def host_list(kind, op, values, **kw):
    """comet_list_pick_host's answer as the list it stands for"""
    got = native.list_pick_host(op, HOST_KIND[kind], [raw(kind, v) for v in values], **kw)
    return None if got is None else [values[i] for i in got]


def host_all(kind, values, rng):
    """every function over one list against the model"""
    dom = KINDS[kind][2]
    n = len(values)
    for key in (dom[-1], rng.choice(dom)):
        assert host_list(kind, REMOVE, values, key=raw(kind, key)) == M.array_remove(values, key), (kind, values, key)
        if kind != "str":
            assert host_list(kind, REMOVE, values, key=key, key_is_column=True) == M.array_remove(values, key)
    if kind != "str":
        assert host_list(kind, REMOVE, values, key=None, key_is_column=True) is None
    assert host_list(kind, COMPACT, values) == M.array_compact(values)
    assert host_list(kind, REVERSE, values) == M.array_reverse(values)
    for start, length in ((1, 1), (2, 3), (-3, 2), (-1, 1), (257, 10), (n + 1, 1), (-n - 1, 2), (1, 0), (1, 2 ** 63 - 1), (2 ** 63 - 1, 1), (-2 ** 63, 2 ** 63 - 1)) + (((n, 1), (-n, n)) if n else ()):
        assert host_list(kind, SLICE, values, start=start, length=length) == M.slice_(values, start, length), (kind, n, start, length)
    if kind == "str":
        for d, r in ((",", None), (", ", "NULL"), ("", None), ("", ""), ("→", "∅")):
            got = native.list_pick_host(JOIN, 32, [raw(kind, v) for v in values], delimiter=d.encode(), replacement=None if r is None else r.encode())
            assert got == M.array_join(values, d, r).encode(), (values, d, r)


@pytest.mark.parametrize("kind", list(KINDS))
def test_host_code_agrees_with_the_model(kind):
    rng = random.Random(300 + HOST_KIND[kind])
    dom = KINDS[kind][2]
    for n in LENGTHS:
        for p_null in (0.0, 0.15):
            host_all(kind, [None if rng.random() < p_null else rng.choice(dom) for _ in range(n)], rng)
    for trial in range(150):
        host_all(kind, [None if rng.random() < rng.choice([0.0, 0.3]) else rng.choice(dom) for _ in range(rng.randrange(0, 9))], rng)
    host_all(kind, [None] * 5, rng)


def test_host_code_on_the_golden_cases():
    kinds = {"int": "i32", "bigint": "i64", "smallint": "i16", "tinyint": "i8", "decimal(38,0)": "dec38_0", "boolean": "bool", "string": "str"}
    for c in GOLDEN:
        kind = kinds[c["type"]]
        for i, (a, want) in enumerate(zip(c["arr"], c["want"])):
            if a is None:
                continue      # (a NULL list is the executor's business: the row's validity bit)
            if c["fn"] == "array_remove":
                key = per_row(c, "key")[i]
                got = None if key is None else host_list(kind, REMOVE, a, key=raw(kind, key))
            elif c["fn"] == "slice":
                got = host_list(kind, SLICE, a, start=per_row(c, "start")[i], length=per_row(c, "length")[i])
            elif c["fn"] == "array_join":
                r = c.get("replacement")
                got = native.list_pick_host(JOIN, 32, [raw(kind, v) for v in a], delimiter=c["delimiter"].encode(), replacement=None if r is None else r.encode()).decode()
            else:
                got = host_list(kind, COMPACT if c["fn"] == "array_compact" else REVERSE, a)
            assert got == want, (c, i)


def test_host_code_on_long_shared_prefixes():
    p = b"prefix of nine+ bytes"
    vals = [p + b" b", p, b"", None, b"a\0", b"a", p + b" a", p]
    assert native.list_pick_host(REMOVE, 32, vals, key=p) == [0, 2, 3, 4, 5, 6]
    assert native.list_pick_host(REMOVE, 32, vals, key=b"a") == [0, 1, 2, 3, 4, 6, 7]
    assert native.list_pick_host(REMOVE, 32, vals, key=b"") == [0, 1, 3, 4, 5, 6, 7]
    assert native.list_pick_host(REMOVE, 32, vals, key=p + b" c") == list(range(8))
    D38 = 10 ** 38 - 1
    assert native.list_pick_host(REMOVE, 16, [2 ** 64, 2 ** 64 + 1, -D38, D38, 0], key=2 ** 64) == [1, 2, 3, 4]
    assert native.list_pick_host(REMOVE, 16, [2 ** 64, 0, 1 - 2 ** 64], key=0, key_is_column=True) == [0, 2]


# ---- createPlan ----
ELEMS = {k: v[0] for k, v in KINDS.items()}
MOVED = dict(ELEMS, f32=S.T_FLOAT, f64=S.T_DOUBLE)      # compact, slice and reverse only move elements


def accepts(plan):
    ok, msg = native.check_plan(plan.encode())
    assert ok, msg
    return msg


def refuses(plan, *words):
    ok, msg = native.check_plan(plan.encode())
    assert not ok, msg
    for w in words:
        assert w in msg, (w, msg)


def key_literal(kind):
    return S.lit(KINDS[kind][2][-1], ELEMS[kind])


@pytest.mark.parametrize("kind", list(MOVED))
def test_createplan_accepts_each_function_over_each_type(kind):
    et = MOVED[kind]
    lt = S.list_type(et, True)
    a = S.col(0, lt)
    src = S.scan([lt, et])
    exprs = [S.array_compact(a), S.array_slice(a, 2, 3), S.array_slice(a, -3, 2), S.array_slice(a, S.lit(1, I64), S.lit(0, I64)), S.array_reverse(a)]
    # slice's literals already folded: no Cast around them
    exprs.append(S.scalar_func("spark_array_slice", [a, S.lit(2, I64), S.lit(3, I64)], S.list_type(et, True)))
    if kind in ELEMS:
        exprs.append(S.array_remove(a, key_literal(kind)))
        if kind != "str":
            exprs.append(S.array_remove(a, S.col(1, et)))
    if kind == "str":
        exprs += [S.array_join(a, ","), S.array_join(a, ", ", "NULL"), S.array_join(a, "", "")]
    for e in exprs:
        accepts(S.project(src, [e]))
    accepts(S.project(src, exprs[:5]))


def test_createplan_accepts_derived_and_chained_lists():
    LS, LI = S.list_type(STR, True), S.list_type(I64, True)
    MT = S.map_type(I64, STR, True)
    src = S.scan([STR, LI, LS, I64, MT])
    s, li, ls, k, m = S.col(0, STR), S.col(1, LI), S.col(2, LS), S.col(3, I64), S.col(4, MT)
    sp = S.scalar_func("split", [s, S.lit(",", STR), S.lit(-1, I32)], S.list_type(STR, False))
    size = lambda x: S.scalar_func("size", [x], I32)
    exprs = [S.array_join(S.sort_array(sp), ","), S.array_join(sp, "-", "?"), S.array_slice(S.array_distinct(li), 1, 2, I64), S.array_remove(S.sort_array(li), k),
             S.array_compact(S.map_values(m)), S.array_reverse(S.map_keys(m)), S.array_remove(S.array_union(li, li), S.lit(3, I64)), S.array_reverse(S.array_reverse(li)),
             S.array_compact(S.array_slice(li, 2, 3)), size(S.array_remove(li, S.lit(3, I64))), S.scalar_func("array_contains", [S.array_compact(li), S.lit(3, I64)], S.T_BOOL),
             S.list_extract(S.array_slice(ls, -2, 2), S.lit(0, I32)), S.scalar_func("length", [S.array_join(ls, ",")], I32), S.sort_array(S.array_remove(ls, S.lit("a", STR)))]
    for e in exprs:
        accepts(S.project(src, [e]))
    accepts(S.project(S.filter_(src, S.eq(S.array_join(ls, ","), S.lit("a,b", STR))), [S.array_remove(li, k)]))
    accepts(S.explode(S.project(src, [S.array_slice(li, 2, 3), s]), S.col(0, LI), [S.col(1, STR)]))
    # identical calls share one derived column; another key, start, length, delimiter or replacement is another column
    plan = S.project(src, [S.array_remove(li, S.lit(3, I64)), size(S.array_remove(li, S.lit(3, I64))), S.array_remove(li, S.lit(4, I64)), S.array_remove(li, k), S.array_remove(li, k)])
    assert native.plan_codegen(plan.encode(), [False] * 5)["derived"] == 3
    plan = S.project(src, [S.array_slice(li, 2, 3), S.array_slice(li, 2, 3), S.array_slice(li, 2, 4), S.array_slice(li, -2, 3), S.array_compact(li), S.array_compact(li), S.array_reverse(li)])
    assert native.plan_codegen(plan.encode(), [False] * 5)["derived"] == 5
    plan = S.project(src, [S.array_join(ls, ","), S.array_join(ls, ","), S.array_join(ls, ",", ""), S.array_join(ls, ",", "x"), S.array_join(ls, ";")])
    assert native.plan_codegen(plan.encode(), [False] * 5)["derived"] == 4
    # over a collect below the Projection, in one plan
    agg = S.hash_agg(S.scan([I32, I64]), [S.col(0, I32)], [S.collect_list(S.col(1, I64), I64)])
    LV = S.list_type(I64, False)
    accepts(S.project(agg, [S.col(0, I32), S.array_remove(S.col(1, LV), S.lit(3, I64)), S.array_reverse(S.col(1, LV))]))


FUNCS = {
    "array_remove_all": lambda a: S.array_remove(a, S.lit(3, I64)), "array_compact": S.array_compact, "spark_array_slice": lambda a: S.array_slice(a, 2, 3, I64),
    "array_reverse": S.array_reverse, "array_to_string": lambda a: S.array_join(a, ","),
}


@pytest.mark.parametrize("name", list(FUNCS))
def test_createplan_refuses_the_argument_by_name(name):
    fn = FUNCS[name]
    et = STR if name == "array_to_string" else I64
    fn_of = (lambda a: S.array_join(a, ",")) if name == "array_to_string" else (lambda a: S.array_slice(a, 2, 3, et)) if name == "spark_array_slice" else fn
    LT_, mt = S.list_type(et, True), S.map_type(et, et, True)
    l, m = S.col(0, LT_), S.col(1, mt)
    refuses(S.project(S.scan([LT_, mt]), [fn_of(m)]), name, "map")
    computed = S.case_when([(S.is_not_null(l), l)], l)
    refuses(S.project(S.scan([LT_]), [fn_of(computed)]), name, "computed array")
    refuses(S.project(S.scan([LT_, et]), [fn_of(S.col(1, et))]), name)
    # element types: Binary and nested for all; floats where elements are compared; anything but Utf8 for the join
    st = S.struct_type([("a", I32, True)])
    for bad in (S.T_BINARY, st, S.list_type(I32, True)):
        lt = S.list_type(bad, True)
        a = S.col(0, lt)
        e = S.array_remove(a, S.lit(3, I64)) if name == "array_remove_all" else S.array_slice(a, 2, 3, bad) if name == "spark_array_slice" else fn_of(a)
        refuses(S.project(S.scan([lt]), [e]), name)
    for ft, word in ((S.T_FLOAT, "Float32"), (S.T_DOUBLE, "Float64")):
        lt = S.list_type(ft, True)
        a = S.col(0, lt)
        if name == "array_remove_all":
            refuses(S.project(S.scan([lt]), [S.array_remove(a, S.lit(1.5, ft))]), name, word, "signed zeros")
        if name == "array_to_string":
            refuses(S.project(S.scan([lt]), [S.array_join(a, ",")]), name, word, "Utf8")
    if name == "array_to_string":
        for kind, ty in ELEMS.items():
            if kind != "str":
                lt = S.list_type(ty, True)
                refuses(S.project(S.scan([lt]), [S.array_join(S.col(0, lt), ",")]), name, "Utf8")
    # a wrong argument count
    counts = {"array_remove_all": ([l], [l, l, l]), "array_compact": ([], [l, l]), "spark_array_slice": ([l], [l, S.lit(1, I64)]), "array_reverse": ([], [l, l]),
              "array_to_string": ([l], [l, S.lit(",", STR), S.lit(",", STR), S.lit(",", STR)])}
    for args in counts[name]:
        refuses(S.project(S.scan([LT_]), [S.scalar_func(name, args, LT_ if name == "spark_array_slice" else None)]), name, "argument")
    # inside an aggregate's chain: its own wording; a join materialises the side instead
    size = lambda x: S.scalar_func("size", [x], I32)
    e = S.scalar_func("length", [fn_of(l)], I32) if name == "array_to_string" else size(fn_of(l))
    src = S.scan([LT_])
    refuses(S.hash_agg(S.project(src, [e]), [], [S.sum_(S.col(0, I32), I64)]), name, "aggregate", "project it below")
    refuses(S.hash_agg(S.project(src, [e]), [S.col(0, I32)], [S.count(S.col(0, I32))]), name, "aggregate")
    other, side = S.scan([I32]), S.project(src, [e])
    for build_side in (S.BUILD_LEFT, S.BUILD_RIGHT):
        assert "hash join" in accepts(S.hash_join(other, side, [S.col(0, I32)], [S.col(0, I32)], S.INNER, build_side))
        assert "hash join" in accepts(S.hash_join(side, other, [S.col(0, I32)], [S.col(0, I32)], S.INNER, build_side))


def test_createplan_refuses_removes_keys_by_name():
    name = "array_remove_all"
    LI, LS = S.list_type(I64, True), S.list_type(STR, True)
    src = S.scan([LI, LS, I64, I32, STR])
    li, ls, k64, k32, ks = S.col(0, LI), S.col(1, LS), S.col(2, I64), S.col(3, I32), S.col(4, STR)
    refuses(S.project(src, [S.array_remove(li, S.lit(None, I64))]), name, "NULL literal key")
    refuses(S.project(src, [S.array_remove(ls, S.lit(None, STR))]), name, "NULL literal key")
    refuses(S.project(src, [S.array_remove(li, S.math("add", k64, S.lit(1, I64), I64))]), name, "computed")
    refuses(S.project(src, [S.array_remove(li, S.cast(k32, I64))]), name, "computed")
    # a key of another type: both are named
    refuses(S.project(src, [S.array_remove(li, S.lit(3, I32))]), name, "Int32", "Int64")
    refuses(S.project(src, [S.array_remove(li, k32)]), name, "Int32", "Int64")
    refuses(S.project(src, [S.array_remove(li, S.lit("3", STR))]), name, "Utf8", "Int64")
    refuses(S.project(src, [S.array_remove(ls, S.lit(3, I64))]), name, "Int64", "Utf8")
    for ta, tb in ((S.decimal(10, 2), S.decimal(10, 3)), (S.decimal(10, 2), S.decimal(12, 2)), (S.T_DATE, I32), (S.T_TIMESTAMP, S.DataType(S.TIMESTAMP_NTZ))):
        la = S.list_type(ta, True)
        refuses(S.project(S.scan([la, tb]), [S.array_remove(S.col(0, la), S.col(1, tb))]), name, "key's type")
        refuses(S.project(S.scan([la, tb]), [S.array_remove(S.col(0, la), S.lit(1, tb))]), name, "key's type")
        accepts(S.project(S.scan([la, ta]), [S.array_remove(S.col(0, la), S.col(1, ta))]))
    # Utf8 elements: a literal only
    refuses(S.project(src, [S.array_remove(ls, ks)]), name, "literal key")
    # a key column must be one of the chain's source: a derived Utf8 column is none
    accepts(S.project(src, [S.array_remove(li, k64)]))


def test_createplan_refuses_slices_arguments_by_name():
    name = "spark_array_slice"
    LI = S.list_type(I64, True)
    src = S.scan([LI, I32, I64])
    li, c32, c64 = S.col(0, LI), S.col(1, I32), S.col(2, I64)
    refuses(S.project(src, [S.array_slice(li, 0, 3)]), name, "start of 0")
    refuses(S.project(src, [S.array_slice(li, 1, -1)]), name, "negative length")
    refuses(S.project(src, [S.array_slice(li, S.lit(None, I32), 2)]), name, "NULL")
    refuses(S.project(src, [S.array_slice(li, 1, S.lit(None, I32))]), name, "NULL")
    refuses(S.project(src, [S.array_slice(li, c32, 2)]), name, "the start", "column")
    refuses(S.project(src, [S.array_slice(li, 1, c32)]), name, "the length", "column")
    refuses(S.project(src, [S.scalar_func(name, [li, c64, S.lit(2, I64)], LI)]), name, "the start")
    refuses(S.project(src, [S.array_slice(li, S.math("add", S.lit(1, I32), S.lit(1, I32), I32), 2)]), name, "computed")
    refuses(S.project(src, [S.array_slice(li, S.lit("1", STR), 2)]), name, "integer literal")
    # the return type: a list of the argument's element type
    for rt in (None, I64, S.list_type(I32, True), S.list_type(STR, True)):
        refuses(S.project(src, [S.scalar_func(name, [li, S.lit(1, I64), S.lit(2, I64)], rt)]), name, "return type")
    accepts(S.project(src, [S.scalar_func(name, [li, S.lit(1, I64), S.lit(2, I64)], S.list_type(I64, False))]))


def test_createplan_refuses_joins_arguments_by_name():
    name = "array_to_string"
    LS = S.list_type(STR, True)
    src = S.scan([LS, STR])
    ls, cs = S.col(0, LS), S.col(1, STR)
    f = lambda *args: S.scalar_func(name, list(args))
    refuses(S.project(src, [f(ls, cs)]), name, "the delimiter", "literal")
    refuses(S.project(src, [f(ls, S.lit(None, STR))]), name, "NULL", "the delimiter")
    refuses(S.project(src, [f(ls, S.lit(1, I32))]), name, "the delimiter", "literal")
    refuses(S.project(src, [f(ls, S.lit(",", STR), cs)]), name, "the null replacement", "literal")
    refuses(S.project(src, [f(ls, S.lit(",", STR), S.lit(None, STR))]), name, "NULL", "the null replacement")
    refuses(S.project(src, [f(ls, S.scalar_func("upper", [cs], STR))]), name, "the delimiter")


def test_serde_helpers_encode_what_the_jvm_sends():
    LI, LS = S.list_type(I64, True), S.list_type(STR, False)
    a, s, k = S.col(0, LI), S.col(1, LS), S.lit(3, I64)
    f = S.scalar_func
    assert S.array_remove(a, k).encode() == f("array_remove_all", [a, k]).encode()
    assert S.array_compact(a).encode() == f("array_compact", [a]).encode()
    assert S.array_reverse(a).encode() == f("array_reverse", [a]).encode()
    assert S.array_join(s, ",").encode() == f("array_to_string", [s, S.lit(",", STR)]).encode()
    assert S.array_join(s, ",", "NULL").encode() == f("array_to_string", [s, S.lit(",", STR), S.lit("NULL", STR)]).encode()
    # slice: both integers under Cast(… AS LONG), and the return type with nullable elements whatever the argument's are
    want = f("spark_array_slice", [s, S.cast(S.lit(2, I32), I64), S.cast(S.lit(3, I32), I64)], S.list_type(STR, True))
    assert S.array_slice(s, 2, 3).encode() == want.encode()
    assert S.array_slice(s, S.lit(2, I32), S.lit(3, I32)).encode() == want.encode()
    assert S.array_compact(a).encode().endswith(b"\x0a\x0darray_compact\x12" + bytes([len(a.encode())]) + a.encode())


def test_the_sheet_lists_the_classes_as_accepted():
    from tools import compat_sheet
    text = compat_sheet.render()
    for cls in ("ArrayRemove", "Slice", "ArrayJoin", "ArrayFilter"):
        assert "spark.comet.expression.%s.enabled=false" % cls not in text, cls
        assert cls in text
    assert "spark.comet.exec.scalaUDF.codegen.enabled=false" in text
    assert "arrays are refused" not in text
    with open(os.path.join(_HERE, "..", "COMPAT.md")) as fh:
        assert fh.read() == text


def test_header_under_the_sanitizers(tmp_path):
    """tests/host/list_pick_check.cpp: list_pick.hpp's keep flags, reverse slots and the join's flags, lengths and bytes over random list columns against a
    naive per-list check, as a stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this machine's compiler cannot link the sanitizer runtimes")
    exe = tmp_path / "list_pick_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + flags + ["-I", _CSRC, "-o", str(exe), os.path.join(_HERE, "host", "list_pick_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
