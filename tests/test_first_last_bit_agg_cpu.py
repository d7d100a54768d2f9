"""first / last and bit_and / bit_or / bit_xor in a HashAggregate, without a GPU: createPlan accepts them in every mode over every accepted type and names the state
columns, hiprtc compiles a grouped and an ungrouped plan that mix them with the older kinds, the refusals name the function, serde.py's bytes follow the reference's
schema.  (That plans WITHOUT the new kinds still generate the kernel source they generated before is checked in test_codegen_corpus_cpu.py.)

Semantics (reference: planner.rs:2679-2735; aggregates.scala:240-420, AggSerde.bitwiseAggTypeSupported): first / last keep (value: child type, is_set: Boolean) as
their Partial state — Spark's own buffer, First.aggBufferAttributes = first :: valueSet — over Boolean, the integers, the floats, Date, Timestamp / TimestampNTZ and
Decimal of any precision; the bitwise aggregates keep one nullable column of the input's type, Byte / Short / Int / Long only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from datafusion_comet_amd import native, serde as S  # noqa: E402

I8, I16, I32, I64, F32, F64 = S.T_INT8, S.T_INT16, S.T_INT32, S.T_INT64, S.T_FLOAT, S.T_DOUBLE
TS_NTZ = S.DataType(S.TIMESTAMP_NTZ)
PICK_TYPES = {"Boolean": S.T_BOOL, "Int8": I8, "Int16": I16, "Int32": I32, "Int64": I64, "Float32": F32, "Float64": F64, "Date": S.T_DATE, "Timestamp": S.T_TIMESTAMP,
              "TimestampNTZ": TS_NTZ, "Decimal(12,2)": S.decimal(12, 2), "Decimal(38,4)": S.decimal(38, 4)}
BIT_TYPES = {"Int8": I8, "Int16": I16, "Int32": I32, "Int64": I64}
BIT = {"bit_and": S.bit_and_agg, "bit_or": S.bit_or_agg, "bit_xor": S.bit_xor_agg}


def accepted(plan):
    ok, text = native.check_plan(plan.encode())
    assert ok, text
    return text


@pytest.mark.parametrize("tname", sorted(PICK_TYPES))
@pytest.mark.parametrize("kind", ["first", "last"])
def test_first_last_accepted_in_every_mode(kind, tname):
    t = PICK_TYPES[tname]
    mk = S.first_ if kind == "first" else S.last_
    for grouped in (False, True):
        for ignore in (False, True):
            agg = mk(S.col(0, t), t, ignore)
            name = kind + ("(ignore_nulls)" if ignore else "")
            text = accepted(S.hash_agg(S.scan([t, I32]), [S.col(1, I32)] if grouped else [], [agg]))
            line = [l for l in text.splitlines() if l.strip().startswith("agg:")]
            assert len(line) == 1 and line[0].strip().startswith(f"agg: {name} -> (") and line[0].rstrip().endswith(", is_set)"), text
            states = S.scan(([I32] if grouped else []) + [t, S.T_BOOL])
            keys = [S.col(0, I32)] if grouped else []
            text = accepted(S.hash_agg(states, keys, [agg], S.FINAL))
            assert f"agg(final): {name} -> " in text and "is_set" not in text, text
            text = accepted(S.hash_agg(states, keys, [agg], S.PARTIAL_MERGE))
            assert f"agg(partial-merge): {name} -> (" in text and ", is_set)" in text, text
    assert "agg: first(ignore_nulls) -> (Int64, is_set)" in accepted(S.hash_agg(S.scan([I64]), [], [S.first_(S.col(0, I64), I64, True)]))


@pytest.mark.parametrize("tname", sorted(BIT_TYPES))
@pytest.mark.parametrize("kind", sorted(BIT))
def test_bit_aggregates_accepted_in_every_mode(kind, tname):
    t = BIT_TYPES[tname]
    agg = BIT[kind](S.col(0, t), t)
    for grouped in (False, True):
        text = accepted(S.hash_agg(S.scan([t, I32]), [S.col(1, I32)] if grouped else [], [agg]))
        assert f"agg: {kind} -> {tname}" in text, text
        states = S.scan(([I32] if grouped else []) + [t])
        keys = [S.col(0, I32)] if grouped else []
        assert f"agg(final): {kind} -> {tname}" in accepted(S.hash_agg(states, keys, [agg], S.FINAL))
        assert f"agg(partial-merge): {kind} -> {tname}" in accepted(S.hash_agg(states, keys, [agg], S.PARTIAL_MERGE))


def test_state_columns_in_the_output_descriptors():
    x, b = S.col(1, I64), S.col(2, I8)
    d = native.plan_codegen(S.hash_agg(S.scan([I32, I64, I8]), [S.col(0, I32)], [S.first_(x, I64), S.last_(x, I64, True), S.bit_and_agg(b, I8), S.count(x)]).encode(), [False, True, True])
    assert [(o["type"], o["nullable"]) for o in d["out"][1:]] == [(S.INT64, True), (S.BOOL, False), (S.INT64, True), (S.BOOL, False), (S.INT8, True), (S.INT64, False)]
    assert "k_gpick" in d["source"] and "P::pick" not in d["source"]      # the pick functor is the plan's own; the kernel body that calls it is the header's
    f = native.plan_codegen(S.hash_agg(S.scan([I64, S.T_BOOL]), [], [S.first_(x, I64)], S.FINAL).encode(), [True, False])
    assert [(o["type"], o["nullable"]) for o in f["out"]] == [(S.INT64, True)]
    # min(x), bit_xor(x) and bit_or(x) over one value and filter share the count word that tells NULL from a value (AggLowering::get): one G_ADD64 besides the row counter
    d2 = native.plan_codegen(S.hash_agg(S.scan([I32, I64]), [S.col(0, I32)], [S.bit_xor_agg(x, I64), S.min_(x, I64), S.bit_or_agg(x, I64)]).encode(), [False, True])
    assert d2["source"].count("comet::G_ADD64;") == 2 * 2, d2["source"]      # (the op and pop switches each list the row counter and the shared count)


def test_mixed_plans_compile_for_gfx950():
    """first, last, the three bit aggregates, count and a decimal sum in one aggregate: decoded, planned, generated and compiled by hiprtc (no GPU needed)"""
    D = S.decimal(38, 4)
    fields = [I32, I64, F64, D, I8]
    x, f, dd, b = S.col(1, I64), S.col(2, F64), S.col(3, D), S.col(4, I8)
    aggs = [S.first_(x, I64), S.last_(x, I64, True), S.first_(dd, D, True), S.last_(f, F64), S.bit_and_agg(b, I8), S.bit_or_agg(x, I64),
            S.bit_xor_agg(x, I64, filter=S.gt(x, S.lit(0, I64))), S.count(x), S.sum_(dd, D)]
    for keys in ([], [S.col(0, I32)]):
        text = native.compile_plan(S.hash_agg(S.scan(fields), keys, aggs).encode())
        for name in ("first", "last(ignore_nulls)", "bit_and", "bit_or", "bit_xor", "count", "sum_decimal"):
            assert f"agg: {name} -> " in text, text


def test_refusals_name_the_function():
    scan = S.scan([S.T_STRING, F64, I32, I64, S.list_type(I64)])
    ok, text = native.check_plan(S.hash_agg(scan, [], [S.first_(S.col(0, S.T_STRING), S.T_STRING)]).encode())
    assert not ok and text.startswith("first over Utf8 is not supported"), text
    ok, text = native.check_plan(S.hash_agg(scan, [S.col(2, I32)], [S.last_(S.col(4, S.list_type(I64)), S.list_type(I64), True)]).encode())
    assert not ok and text.startswith("last over ") and "is not supported" in text, text
    ok, text = native.check_plan(S.hash_agg(scan, [], [S.bit_or_agg(S.col(1, F64), F64)]).encode())
    assert not ok and text.startswith("bit_or over Float64 is not supported"), text
    ok, text = native.check_plan(S.hash_agg(S.scan([S.T_DATE]), [], [S.bit_and_agg(S.col(0, S.T_DATE), S.T_DATE)]).encode())
    assert not ok and text.startswith("bit_and over ") and "is not supported" in text, text
    # a Final first whose second state column is not the Boolean is_set
    ok, text = native.check_plan(S.hash_agg(S.scan([I64, I64]), [], [S.first_(S.col(0, I64), I64)], S.FINAL).encode())
    assert not ok and "first expects (value, is_set)" in text, text
    # over a window frame the bit aggregates stay refused, by their tag
    win = S.window(S.sort(scan, [(S.col(2, I32), False)]), [S.col(2, I32)], [(S.col(3, I64), False)],
                   [("agg", S.bit_or_agg(S.col(3, I64), I64), I64, ("rows", "unbounded", "current"))])
    ok, text = native.check_plan(win.encode())
    assert not ok and "Window: aggregate (tag 10)" in text, text


def test_serde_bytes_parse_under_the_reference_schema():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    from tests.test_proto_wire_cpu import unknown_paths
    fds = descriptor_pb2.FileDescriptorSet()
    with open(os.path.join(ROOT, "tests", "golden", "comet_protos.desc"), "rb") as f:
        fds.ParseFromString(f.read())
    pool = descriptor_pool.DescriptorPool()
    for fd in fds.file:
        pool.Add(fd)
    Agg = message_factory.GetMessageClass(pool.FindMessageTypeByName("spark.spark_expression.AggExpr"))
    x = S.col(1, I64)
    flt = S.gt(x, S.lit(0, I64))
    for kind, tag, field in (("bit_and", 9, "bitAndAgg"), ("bit_or", 10, "bitOrAgg"), ("bit_xor", 11, "bitXorAgg")):
        for with_filter in (False, True):
            a = BIT[kind](x, I64, filter=flt if with_filter else None)
            m = Agg()
            m.ParseFromString(a.encode())
            assert unknown_paths(m) == [], kind
            assert m.WhichOneof("expr_struct") == field and Agg.DESCRIPTOR.fields_by_name[field].number == tag
            body = getattr(m, field)
            assert body.datatype.type_id == S.INT64 and body.child.WhichOneof("expr_struct") == "bound" and body.child.bound.index == 1
            assert m.HasField("filter") == with_filter
            # … and the bytes protobuf itself writes for the same message are the bytes serde.py wrote: proto.cpp reads either
            assert m.SerializeToString(deterministic=True) == a.encode()
            ok, text = native.check_plan(S.hash_agg(S.scan([I32, I64]), [], [a]).encode())
            assert ok and f"agg: {kind} -> Int64" in text, text
    # first / last gained a filter= argument: without it the bytes are what they were (First / Last{child = 1, datatype = 2, ignore_nulls = 3})
    assert S.first_(x, I64, True).encode().hex() == "3a100a081a06080112020804120208041801"
    assert S.last_(x, I64).encode().hex() == "420e0a081a0608011202080412020804"
    for mk, field in ((S.first_, "first"), (S.last_, "last")):
        m = Agg()
        m.ParseFromString(mk(x, I64, True, filter=flt).encode())
        assert unknown_paths(m) == [] and m.WhichOneof("expr_struct") == field and getattr(m, field).ignore_nulls and m.HasField("filter")

