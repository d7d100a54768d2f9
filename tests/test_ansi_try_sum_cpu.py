"""ANSI / TRY integer sums and Spark's rewritten decimal sums (unscaled_value / make_decimal), without a GPU: what createPlan accepts and refuses, the state columns
it names, the words the generator spends on each form, hiprtc compiling the plans Spark 4 sends, and the compatibility sheet's probes.

Semantics (reference: agg_funcs/sum_int.rs, math_funcs/internal/{unscaled_value,make_decimal}.rs; JVM side decimalExpressions.scala:27-75): an ANSI sum keeps one nullable
Int64 and fails the task on overflow; try_sum keeps (sum: Int64 nullable, has_all_nulls: Boolean) where (NULL, false) is "overflowed".  unscaled_value(decimal(p <= 18, s))
is the stored integer, make_decimal(Int64) -> decimal(p, s) takes the integer as the unscaled value, NULL (or NUMERIC_VALUE_OUT_OF_RANGE under fail_on_error) beyond
10^p - 1.  An ANSI / TRY sum whose input bound proves that 2^33 rows cannot reach 2^63 spends exactly LEGACY's words and has no overflow code."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from datafusion_comet_amd import native, serde as S  # noqa: E402

I8, I16, I32, I64 = S.T_INT8, S.T_INT16, S.T_INT32, S.T_INT64
INTS = {"Int8": I8, "Int16": I16, "Int32": I32, "Int64": I64}
MODES = {"ansi": S.ANSI, "try": S.TRY}
D72 = S.decimal(7, 2)


def accepted(plan):
    ok, text = native.check_plan(plan.encode())
    assert ok, text
    return text


def refused(plan):
    ok, text = native.check_plan(plan.encode())
    assert not ok, text
    return text


@pytest.mark.parametrize("tname", sorted(INTS))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_sums_accepted_in_every_mode(mode, tname):
    t, m = INTS[tname], MODES[mode]
    agg = S.sum_(S.col(0, t), I64, m)
    state = S.sum_state_types(agg)
    assert state == ([I64] if mode == "ansi" else [I64, S.T_BOOL])
    partial_text = f"agg: sum_int({mode}) -> " + ("Int64" if mode == "ansi" else "(Int64, has_all_nulls)")
    for grouped in (False, True):
        keys = [S.col(1, I32)] if grouped else []
        assert partial_text in accepted(S.hash_agg(S.scan([t, I32]), keys, [agg])), (mode, tname, grouped)
        assert partial_text in accepted(S.hash_agg(S.scan([t, I32]), keys, [S.sum_(S.col(0, t), I64, m, filter=S.gt(S.col(1, I32), S.lit(0, I32)))]))
        states = S.scan(([I32] if grouped else []) + state)
        skeys = [S.col(0, I32)] if grouped else []
        text = accepted(S.hash_agg(states, skeys, [agg], S.FINAL))
        assert f"sum_int({mode}) -> Int64" in text and "has_all_nulls" not in text, text
        text = accepted(S.hash_agg(states, skeys, [agg], S.PARTIAL_MERGE))
        assert f"sum_int({mode}) -> " + ("Int64" if mode == "ansi" else "(Int64, has_all_nulls)") in text, text


def test_state_columns_in_the_output_descriptors():
    x = S.col(1, I64)
    d = native.plan_codegen(S.hash_agg(S.scan([I32, I64]), [S.col(0, I32)], [S.sum_(x, I64, S.ANSI), S.sum_(x, I64, S.TRY), S.sum_(x, I64)]).encode(), [False, True])
    assert [(o["type"], o["nullable"]) for o in d["out"][1:]] == [(S.INT64, True), (S.INT64, True), (S.BOOL, False), (S.INT64, True)]
    f = native.plan_codegen(S.hash_agg(S.scan([I64, S.T_BOOL]), [], [S.sum_(S.col(0, I64), I64, S.TRY)], S.FINAL).encode(), [True, False])
    assert [(o["type"], o["nullable"]) for o in f["out"]] == [(S.INT64, True)]
    # mixed per-expression modes: the PartialMerge try_sum reads TWO state columns from initial_input_buffer_offset on, the count behind them the next one
    child = S.scan([I32, I64, I64, S.T_BOOL, I64])
    aggs = [S.sum_(S.col(1, I64), I64, S.TRY), S.count(S.col(1, I64)), S.sum_(S.col(1, I64), I64, S.ANSI)]
    text = accepted(S.hash_agg(child, [S.col(0, I32)], aggs, S.PARTIAL, expr_modes=[S.PARTIAL_MERGE, S.PARTIAL_MERGE, S.PARTIAL], initial_input_buffer_offset=2))
    assert "agg(partial-merge): sum_int(try) -> (Int64, has_all_nulls)" in text and "agg: sum_int(ansi) -> Int64" in text, text
    # a Final try_sum whose second state column is not the Boolean
    assert "expects (sum, has_all_nulls)" in refused(S.hash_agg(S.scan([I64, I64]), [], [S.sum_(S.col(0, I64), I64, S.TRY)], S.FINAL))


def test_scalar_functions_accepted_wherever_an_expression_is():
    scan = S.scan([D72, I64, I32])
    d, x, k = S.col(0, D72), S.col(1, I64), S.col(2, I32)
    text = accepted(S.project(scan, [S.unscaled_value(d), S.make_decimal(x, 17, 2), S.make_decimal(x, 17, 2, null_on_overflow=False), S.make_decimal(S.unscaled_value(d), 17, 2)]))
    assert text.count("Decimal128(17, 2)") == 3 and "Int64" in text, text
    accepted(S.filter_(scan, S.gt(S.unscaled_value(d), S.lit(100, I64))))
    # under an aggregate: as Spark's DecimalAggregates rewrites sum(d) and avg(d) of a short decimal — and as a group key
    text = accepted(S.hash_agg(scan, [S.unscaled_value(d)], [S.sum_(S.unscaled_value(d), I64, S.ANSI), S.avg(S.unscaled_value(d), S.T_DOUBLE, S.T_DOUBLE)]))
    assert "agg: sum_int(ansi) -> Int64" in text, text
    # … and above one: Projection(make_decimal(sum)) over the Final aggregate
    final = S.hash_agg(S.scan([I32, I64]), [S.col(0, I32)], [S.sum_(S.unscaled_value(d), I64, S.ANSI)], S.FINAL)
    accepted(S.project(final, [S.col(0, I32), S.make_decimal(S.col(1, I64), 17, 2)]))
    # join keys
    accepted(S.hash_join(S.scan([D72, I64]), S.scan([I64]), [S.unscaled_value(S.col(0, D72))], [S.col(0, I64)], S.INNER, S.BUILD_RIGHT))


def test_refusals_name_the_function():
    D20 = S.decimal(20, 2)
    assert refused(S.project(S.scan([D20]), [S.unscaled_value(S.col(0, D20))])).startswith("unscaled_value over Decimal128(20, 2) is not supported")
    assert refused(S.project(S.scan([I32]), [S.make_decimal(S.col(0, I32), 17, 2)])).startswith("make_decimal over Int32 is not supported")
    assert refused(S.hash_agg(S.scan([D20]), [], [S.sum_(S.unscaled_value(S.col(0, D20)), I64, S.ANSI)])).startswith("unscaled_value over ")
    # over a window frame a non-LEGACY integer sum would wrap silently: refused by name, the LEGACY one stays
    scan = S.scan([I32, I64])
    for mode, ok in ((S.LEGACY, True), (S.ANSI, False), (S.TRY, False)):
        win = S.window(S.sort(scan, [(S.col(0, I32), False)]), [S.col(0, I32)], [(S.col(1, I64), False)], [("agg", S.sum_(S.col(1, I64), I64, mode), I64, ("rows", "unbounded", "current"))])
        got, text = native.check_plan(win.encode())
        assert got == ok, text
        if not ok:
            assert "Window: ANSI/TRY integer SUM over a window frame is not supported" in text, text


def _shape(src):
    """the words a plan's accumulator and its grouped tile spend: (NW, NPW, the op of each accumulator word)"""
    nw = int(re.search(r"static constexpr int NW = (\d+);", src).group(1))
    npw = re.search(r"static constexpr int NPW = (\d+);", src)
    ops = re.search(r"constexpr int op\(int k\) \{(.*?)default", src, re.S)
    return nw, int(npw.group(1)) if npw else None, re.findall(r"comet::(G_\w+);", ops.group(1)) if ops else None


@pytest.mark.parametrize("grouped", [False, True])
def test_a_proven_sum_spends_legacys_words_and_an_unproven_one_the_extra_ones(grouped):
    keys = [S.col(1, I32)] if grouped else []
    src = lambda agg, t: native.plan_codegen(S.hash_agg(S.scan([t, I32]), keys, [agg]).encode(), [True, False])["source"]
    # Spark 4's plan for sum(d: decimal(7,2)): 10^7 · 2^33 < 2^63, nothing can overflow
    u = S.unscaled_value(S.col(0, D72))
    legacy, ansi, try_ = src(S.sum_(u, I64), D72), src(S.sum_(u, I64, S.ANSI), D72), src(S.sum_(u, I64, S.TRY), D72)
    assert _shape(ansi) == _shape(legacy) == _shape(try_)
    for s in (ansi, try_):
        assert "int_sum_decide" not in s and "atomicOr" not in s and "(unsigned int*)prm.out[2]" not in s and "i64_pos_part" not in s, s      # no overflow code, no error-word write
    # … and the per-row feed is LEGACY's, line for line
    feed = lambda s: [l.strip() for l in s.splitlines() if "pv[" in l or ("acc[" in l and "+=" in l)]
    assert feed(ansi) == feed(legacy) == feed(try_) and feed(ansi)
    # Int8 and Int16 inputs are proven the same way
    for t in (I8, I16):
        assert _shape(src(S.sum_(S.col(0, t), I64, S.ANSI), t)) == _shape(src(S.sum_(S.col(0, t), I64), t))
    # a raw Int64 column: count + the positive and the negative sum, 128 bits each; Int32 the same words with one limb each in the grouped tile
    l64, a64, a32 = src(S.sum_(S.col(0, I64), I64), I64), src(S.sum_(S.col(0, I64), I64, S.ANSI), I64), src(S.sum_(S.col(0, I32), I64, S.ANSI), I32)
    nw_l, npw_l, _ = _shape(l64)
    nw_a, npw_a, ops_a = _shape(a64)
    assert nw_a == nw_l + 3 and "int_sum_decide" in a64 and "atomicOr((unsigned int*)prm.out[2], 2u)" in a64
    if grouped:
        assert npw_a == npw_l + 2 and ops_a.count("G_ADD128") == 2
        assert _shape(a32)[0] == nw_a and _shape(a32)[1] == npw_a - 2
    # TRY never writes the overflow flag, only the cannot-be-decided one (inside int_sum_decide)
    t64 = src(S.sum_(S.col(0, I64), I64, S.TRY), I64)
    assert "int_sum_decide" in t64 and "atomicOr" not in t64


def test_make_decimal_checks_only_what_the_bound_does_not_prove():
    scan = S.scan([D72, I64])
    src = lambda e: native.plan_codegen(S.project(scan, [e]).encode(), [True, True])["source"]
    proven = src(S.make_decimal(S.unscaled_value(S.col(0, D72)), 17, 2, null_on_overflow=False))
    assert "dec_fits" not in proven and "err_detail" not in proven
    checked = src(S.make_decimal(S.col(1, I64), 17, 2, null_on_overflow=False))
    assert "dec_fits64" in checked and "err_detail" in checked
    nulling = src(S.make_decimal(S.col(1, I64), 17, 2))
    assert "dec_fits64" in nulling and "err_detail" not in nulling
    assert "dec_fits" not in src(S.make_decimal(S.col(1, I64), 19, 2, null_on_overflow=False))      # every Int64 fits 19 digits


def test_the_plans_spark_4_sends_compile_for_gfx950():
    """decoded, planned, generated and compiled by hiprtc (no GPU needed): the rewritten decimal sum and average, grouped and not, and the dynamic sums in each mode"""
    u = S.unscaled_value(S.col(1, D72))
    for keys in ([], [S.col(0, I32)]):
        text = native.compile_plan(S.hash_agg(S.scan([I32, D72, I64]), keys, [S.sum_(u, I64, S.ANSI), S.avg(u, S.T_DOUBLE, S.T_DOUBLE), S.sum_(S.col(2, I64), I64, S.ANSI),
                                                                             S.sum_(S.col(2, I64), I64, S.TRY), S.sum_(S.col(0, I32), I64, S.TRY)]).encode())
        assert "agg: sum_int(ansi) -> Int64" in text and "agg: sum_int(try) -> (Int64, has_all_nulls)" in text, text
        nk = len(keys)
        states = S.scan([I32] * nk + [I64, I64, S.T_BOOL])
        skeys = [S.col(0, I32)] * nk
        final = S.hash_agg(states, skeys, [S.sum_(u, I64, S.ANSI), S.sum_(S.col(2, I64), I64, S.TRY)], S.FINAL)
        native.compile_plan(S.project(final, [S.make_decimal(S.col(nk, I64), 17, 2, null_on_overflow=False), S.col(nk + 1, I64)]).encode())


def test_compat_sheet_probes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("compat_sheet", os.path.join(ROOT, "tools", "compat_sheet.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    sheet = m.render()
    for name in ("UnscaledValue", "MakeDecimal", "KnownNotNull", "KnownNullable"):
        assert f"spark.comet.expression.{name}.enabled=false" not in sheet, name
    assert "integers (LEGACY / ANSI / TRY)" in sheet
    assert "cannot be decided order-independently" in sheet


def _corpus_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("codegen_corpus", os.path.join(ROOT, "tools", "codegen_corpus.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_new_plans_generate_what_was_recorded_for_them():
    """tools/codegen_corpus.py --ansi-try-sum against tests/golden/ansi_try_sum_codegen.json: the generated source, descriptors and explain / refusal texts of the ANSI /
    TRY sums in every mode, of the mixed and shared forms and of the two scalar functions, as the older corpus holds them for the older aggregates"""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "ansi_try_sum_codegen.json")) as f:
        want = json.load(f)
    got = _corpus_tool().ansi_try_sum_corpus()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name
    refused = [n for n, e in want.items() if any(v.startswith("refused: ") for v in e.values())]
    assert sorted(refused) == ["refuse/final_try_sum_without_its_flag", "refuse/make_decimal_of_an_int", "refuse/unscaled_value_of_a_wide_decimal"]


def test_an_entry_of_the_older_corpus_is_retired_only_because_its_refusal_is_gone():
    """the older corpus (tests/golden/codegen_corpus.json) recorded `refuse/ansi_integer_sum` as a refusal; the tool carries that record over instead of generating it.
    That is honest only while the plan it stood for is accepted — here it must be, and it must be held by the newer corpus"""
    tool = _corpus_tool()
    assert sorted(tool.RETIRED) == ["refuse/ansi_integer_sum"]
    assert "refuse/ansi_integer_sum" not in dict(tool.all_plans())
    plans = dict(tool.ansi_try_sum_plans())
    lifted = plans["lifted/ansi_integer_sum"]
    assert lifted.encode() == S.hash_agg(S.scan([I64]), [], [S.sum_(S.col(0, I64), I64, S.ANSI)]).encode()
    assert accepted(lifted) == "  agg: sum_int(ansi) -> Int64\n"
    assert "int_sum_decide" in native.plan_codegen(lifted.encode(), [True])["source"]
