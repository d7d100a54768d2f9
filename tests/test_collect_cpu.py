"""collect_list / collect_set without a GPU: the pure-Python model (tests/collect_model.py) against the input tables of the reference's own SQL tests
(tests/golden/collect_cases.json), what createPlan accepts and what it refuses by name, and the serde's encoding."""
import json
import os

import pytest

from datafusion_comet_amd import native, serde as S
from tests import collect_model as M

I8, I16, I32, I64, F32, F64, STR, BOOL = S.T_INT8, S.T_INT16, S.T_INT32, S.T_INT64, S.T_FLOAT, S.T_DOUBLE, S.T_STRING, S.T_BOOL
DATE, TS, TS_NTZ, BIN = S.T_DATE, S.T_TIMESTAMP, S.DataType(S.TIMESTAMP_NTZ), S.T_BINARY
ELEMENT_TYPES = [BOOL, I8, I16, I32, I64, DATE, TS, TS_NTZ, S.decimal(10, 2), S.decimal(38, 0), STR]
MODES = [S.PARTIAL, S.PARTIAL_MERGE, S.FINAL]
MODE_IDS = ["partial", "partial_merge", "final"]
FUNCS = {"collect_list": S.collect_list, "collect_set": S.collect_set}

with open(os.path.join(os.path.dirname(__file__), "golden", "collect_cases.json")) as f:
    CASES = json.load(f)["cases"]


# --------------------------------------------------------------------------- the model

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_on_the_reference_sql_tables(case):
    values = [r[0] for r in case["rows"]]
    keys = [(r[1],) if case["grouped"] else () for r in case["rows"]]
    keep = None
    if "filter_gt" in case:
        keep = [v is not None and v > case["filter_gt"] for v in values]      # (a NULL comparison rejects the row)
    unkey = (lambda k: k[0]) if case["grouped"] else (lambda k: "")
    lst = M.collect_list(keys, values, keep, ungrouped=not case["grouped"])
    st = M.collect_set(keys, values, keep, ungrouped=not case["grouped"])
    assert {unkey(k): sorted(v) for k, v in lst.items()} == case["list"]
    assert {unkey(k): sorted(v) for k, v in st.items()} == case["set"]
    for k, v in st.items():
        assert len(v) == len(case["set"][unkey(k)])
    # the rows split in two, collected apart and merged: the same lists (in arrival order) and sets
    half = len(values) // 2
    parts = [M.collect_list(keys[a:b], values[a:b], keep[a:b] if keep else None, ungrouped=not case["grouped"]) for a, b in ((0, half), (half, len(values)))]
    rows = M.state_rows(parts[0]) + M.state_rows(parts[1])
    assert M.merge_list(rows, ungrouped=not case["grouped"]) == lst
    assert M.merge_set(rows, ungrouped=not case["grouped"]) == st


def test_model_keeps_arrival_order_and_merges_in_input_order():
    keys = [(1,), (2,), (1,), (1,), (2,), (3,)]
    vals = [5, 9, None, 3, 9, None]
    assert M.collect_list(keys, vals) == {(1,): [5, 3], (2,): [9, 9], (3,): []}
    assert M.collect_set(keys, vals) == {(1,): {5, 3}, (2,): {9}, (3,): set()}
    assert M.collect_list(keys, vals, keep=[0, 1, 1, 1, None, 1]) == {(1,): [3], (2,): [9], (3,): []}
    assert M.collect_list([], [], ungrouped=True) == {(): []} and M.collect_list([], []) == {}
    rows = [((1,), [7, 7]), ((2,), None), ((1,), []), ((1,), [None, 4]), ((3,), [1])]
    assert M.merge_list(rows) == {(1,): [7, 7, 4], (2,): [], (3,): [1]}
    assert M.merge_set(rows) == {(1,): {7, 4}, (2,): set(), (3,): {1}}
    assert M.merge_list([], ungrouped=True) == {(): []}


# --------------------------------------------------------------------------- createPlan accepts

def plan_of(mode, grouped, aggs, elem_types, extra_fields=()):
    """aggs over columns 1 … (Partial) or over their states behind the key (merging)"""
    if mode == S.PARTIAL:
        fields = [I32] + list(elem_types) + list(extra_fields)
    else:
        fields = ([I32] if grouped else []) + [S.list_type(t, True) for t in elem_types]
    return S.hash_agg(S.scan(fields), [S.col(0, I32)] if grouped else [], aggs, mode)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("grouped", [False, True], ids=["ungrouped", "grouped"])
@pytest.mark.parametrize("func", sorted(FUNCS))
@pytest.mark.parametrize("elem", ELEMENT_TYPES, ids=repr)
def test_check_plan_accepts_every_element_type_mode_and_grouping(built, elem, func, grouped, mode):
    ok, text = native.check_plan(plan_of(mode, grouped, [FUNCS[func](S.col(1, elem), elem)], [elem]).encode())
    assert ok, text
    assert "collect (" in text and "one sort per column" in text


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("elem", [F32, F64], ids=repr)
def test_check_plan_accepts_collect_list_of_floats(built, elem, mode):
    ok, text = native.check_plan(plan_of(mode, True, [S.collect_list(S.col(1, elem), elem)], [elem]).encode())
    assert ok, text


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_check_plan_accepts_list_and_set_mixed_and_four_value_columns(built, mode):
    a, b = S.col(1, I64), S.col(2, STR)
    flt = S.gt(S.col(0, I32), S.lit(3, I32)) if mode == S.PARTIAL else None
    mixed = [S.collect_list(a, I64), S.collect_set(a, I64), S.collect_list(b, STR, filter=flt)]
    ok, text = native.check_plan(plan_of(mode, True, mixed, [I64, I64, STR] if mode != S.PARTIAL else [I64, STR]).encode())
    assert ok, text
    types = [I64, STR, S.decimal(38, 0), BOOL]
    four = [S.collect_set(S.col(1 + i, t), t) for i, t in enumerate(types)]
    ok, text = native.check_plan(plan_of(mode, False, four, types).encode())
    assert ok, text
    # the same (function, child, FILTER) twice is one value column: five aggregates over four columns
    if mode == S.PARTIAL:
        ok, text = native.check_plan(plan_of(mode, True, four + [S.collect_set(S.col(1, I64), I64)], types).encode())
        assert ok, text


def test_check_plan_accepts_an_utf8_and_a_two_column_key(built):
    plan = S.hash_agg(S.scan([STR, I32, I64]), [S.col(0, STR), S.col(1, I32)], [S.collect_list(S.col(2, I64), I64), S.collect_set(S.col(2, I64), I64)], S.PARTIAL)
    ok, text = native.check_plan(plan.encode())
    assert ok, text


# --------------------------------------------------------------------------- createPlan refuses, by name

def refused(plan):
    ok, text = native.check_plan(plan.encode())
    assert not ok, text
    return text


ENGINE = "MI355X native engine"


@pytest.mark.parametrize("func", sorted(FUNCS))
def test_refuses_a_collect_beside_another_aggregate_function(built, func):
    x = S.col(1, I64)
    for aggs in ([FUNCS[func](x, I64), S.sum_(x, I64)], [S.count(x), FUNCS[func](x, I64)]):
        text = refused(S.hash_agg(S.scan([I32, I64]), [S.col(0, I32)], aggs, S.PARTIAL))
        assert func in text and "mixed with other aggregate functions" in text and ENGINE in text
        assert ("sum" in text) or ("count" in text)


@pytest.mark.parametrize("func", sorted(FUNCS))
def test_refuses_percentile_and_collect_in_one_aggregate_from_both_sides(built, func):
    d = S.col(1, F64)
    for aggs in ([S.percentile(d, 0.5), FUNCS[func](S.col(2, I64), I64)], [FUNCS[func](S.col(2, I64), I64), S.percentile(d, 0.5)]):
        text = refused(S.hash_agg(S.scan([I32, F64, I64]), [S.col(0, I32)], aggs, S.PARTIAL))
        assert "percentile" in text and func in text and "mixed with other aggregate functions" in text and ENGINE in text


def test_refuses_mixed_per_expression_modes(built):
    x = S.col(1, I64)
    text = refused(S.hash_agg(S.scan([I32, I64, S.list_type(I64, True)]), [S.col(0, I32)], [S.collect_list(x, I64), S.collect_set(x, I64)], S.PARTIAL,
                              expr_modes=[S.PARTIAL, S.PARTIAL_MERGE], initial_input_buffer_offset=2))
    assert "collect_list" in text and "mixed-mode" in text and ENGINE in text


def test_refuses_more_than_four_distinct_value_columns(built):
    five = [S.collect_list(S.col(1 + i, I64), I64) for i in range(5)]
    text = refused(S.hash_agg(S.scan([I32] + [I64] * 5), [S.col(0, I32)], five, S.PARTIAL))
    assert "collect_list" in text and "more than 4 distinct value columns" in text and ENGINE in text
    # one child under list, set and three FILTERs: five columns as well
    x = S.col(1, I64)
    flts = [S.gt(S.col(0, I32), S.lit(i, I32)) for i in range(3)]
    text = refused(S.hash_agg(S.scan([I32, I64]), [], [S.collect_list(x, I64), S.collect_set(x, I64)] + [S.collect_set(x, I64, filter=f) for f in flts], S.PARTIAL))
    assert "more than 4 distinct value columns" in text and "(got 5)" in text


@pytest.mark.parametrize("elem", [F32, F64], ids=repr)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_refuses_collect_set_of_floats_and_says_why(built, elem, mode):
    text = refused(plan_of(mode, True, [S.collect_set(S.col(1, elem), elem)], [elem]))
    assert "collect_set" in text and ("Float32" in text or "Float64" in text or "float" in text.lower()) and ENGINE in text
    assert "-0.0" in text and "NaN" in text


def test_refuses_float_grouping_keys(built):
    for kt in (F32, F64):
        text = refused(S.hash_agg(S.scan([kt, I64]), [S.col(0, kt)], [S.collect_list(S.col(1, I64), I64)], S.PARTIAL))
        assert "collect_list" in text and "grouped by a" in text and ENGINE in text


@pytest.mark.parametrize("func", sorted(FUNCS))
def test_refuses_binary_struct_list_and_map_children(built, func):
    nested = [BIN, S.struct_type([("x", I32, True)]), S.list_type(I32, True), S.map_type(STR, I32)]
    for t in nested:
        text = refused(S.hash_agg(S.scan([I32, t]), [S.col(0, I32)], [FUNCS[func](S.col(1, t), t)], S.PARTIAL))
        assert func in text and "child" in text and ENGINE in text, text
    assert "Binary" in refused(S.hash_agg(S.scan([I32, BIN]), [], [FUNCS[func](S.col(1, BIN), BIN)], S.PARTIAL))


@pytest.mark.parametrize("func", sorted(FUNCS))
@pytest.mark.parametrize("mode", [S.PARTIAL_MERGE, S.FINAL], ids=["partial_merge", "final"])
def test_refuses_a_state_column_that_is_no_list_of_the_element_type(built, func, mode):
    agg = [FUNCS[func](S.col(1, I64), I64)]
    for state in (I64, S.list_type(I32, True), S.list_type(STR, True), S.list_type(S.list_type(I64, True), True)):
        text = refused(S.hash_agg(S.scan([I32, state]), [S.col(0, I32)], agg, mode))
        assert func in text and "List<" in text and "state in column 1" in text, text
    text = refused(S.hash_agg(S.scan([I32]), [S.col(0, I32)], agg, mode))      # no such column at all
    assert func in text and "state in column 1" in text
    # decimals: the same precision and scale, or it is another type
    dec = [FUNCS[func](S.col(1, S.decimal(10, 2)), S.decimal(10, 2))]
    text = refused(S.hash_agg(S.scan([I32, S.list_type(S.decimal(12, 2), True)]), [S.col(0, I32)], dec, mode))
    assert func in text and "state in column 1" in text


def test_refuses_a_child_whose_type_is_not_the_declared_element_type(built):
    text = refused(S.hash_agg(S.scan([I32, I64]), [S.col(0, I32)], [S.collect_list(S.col(1, I64), I32)], S.PARTIAL))
    assert "collect_list" in text and "the aggregate's datatype says" in text


# --------------------------------------------------------------------------- serde

def _fields(buf):
    """top-level (field number, wire type, payload) of a protobuf message"""
    out, i = [], 0
    while i < len(buf):
        tag, shift = 0, 0
        while True:
            b = buf[i]; i += 1
            tag |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                break
        fno, wt = tag >> 3, tag & 7
        assert wt in (0, 2)
        n, shift = 0, 0
        while True:
            b = buf[i]; i += 1
            n |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                break
        if wt == 2:
            out.append((fno, wt, buf[i:i + n]))
            i += n
        else:
            out.append((fno, wt, n))
    return out


@pytest.mark.parametrize("func,tag", [("collect_list", 21), ("collect_set", 17)])
def test_serde_encodes_the_reference_tags(func, tag):
    child = S.col(3, I64)
    flt = S.gt(S.col(0, I32), S.lit(1, I32))
    plain = _fields(FUNCS[func](child, I64).encode())
    assert [(f, w) for f, w, _ in plain] == [(tag, 2)]
    body = _fields(plain[0][2])
    assert [(f, w) for f, w, _ in body] == [(1, 2), (2, 2)]      # child = 1, datatype = 2
    assert body[0][2] == child.encode()
    assert body[1][2] == S.list_type(I64, False).encode()        # ArrayType(element, containsNull = false)
    with_filter = _fields(FUNCS[func](child, I64, filter=flt).encode())
    assert [(f, w) for f, w, _ in with_filter] == [(tag, 2), (89, 2)] and with_filter[1][2] == flt.encode()
