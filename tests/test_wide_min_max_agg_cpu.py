"""Grouped min / max of a decimal wider than 18 digits, without a GPU: what createPlan accepts, the kernels the generator lists for it — and for the plans that must not
change —, the corpus tool's record of the lifted refusals, and the compatibility sheet.

A wide grouped min / max adds two kernels behind k_gagg (comet_device.hpp "wide min / max"): k_gwreset, one lane per slot, and k_gwlow, one lane per row.  A plan
without one generates none of them and no word for them.  Where the value's static bound proves |v| < 2^63 (a cast of a narrow decimal) the one-word min / max serves.

The older corpus (tests/golden/codegen_corpus.json) recorded the three grouped max_d38 plans as refusals.  tools/codegen_corpus.py carries those records over without
generating them — in RETIRED_WIDE_MIN_MAX, a table beside RETIRED (tests/test_ansi_try_sum_cpu.py pins RETIRED itself to one entry); retired() is both — and holds the
plans in the corpus of tests/golden/wide_min_max_codegen.json under what they generate now."""
import importlib.util
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from datafusion_comet_amd import native, serde as S, tpch  # noqa: E402

I32, I64, F64 = S.T_INT32, S.T_INT64, S.T_DOUBLE
D12, D22, D38 = S.decimal(12, 2), S.decimal(22, 2), S.decimal(38, 4)
WIDE_KERNELS = {"k_gwreset", "k_gwlow"}
REFUSAL = "min/max of a decimal wider than 18 digits is not supported in a grouped GPU aggregate yet"
LIFTED = ["agg/max_d38/final/grouped", "agg/max_d38/partial/grouped", "agg/max_d38/partial_merge/grouped"]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def corpus_tool():
    return _tool("codegen_corpus")


def accepted(plan):
    ok, text = native.check_plan(plan.encode())
    assert ok, text
    return text


def codegen(plan, ncols=16):
    return native.plan_codegen(plan.encode(), [True] * ncols)


def test_the_lifted_plans_are_accepted(corpus_tool):
    plans = dict(corpus_tool.wide_min_max_plans())
    for name in LIFTED:
        text = accepted(plans[name])
        assert "max -> Decimal128(38, 4)" in text and "refused" not in text, (name, text)
    # … and they are the plans the older corpus refused: the same bytes as its generator makes for those names
    kinds = {"max_d38": corpus_tool.aggregate_kinds()["max_d38"]}
    old = {n: p for n, p in corpus_tool.aggregate_plans(kinds)}
    for name in LIFTED:
        assert plans[name].encode() == old[name].encode(), name


def test_the_lifted_plans_list_the_new_kernels(corpus_tool):
    plans = dict(corpus_tool.wide_min_max_plans())
    for name in LIFTED + ["agg/min_d38/partial/grouped", "agg/min_d38/partial_filter/grouped", "mixed/max_d38_first_sum_count/grouped"]:
        d = codegen(plans[name])
        assert WIDE_KERNELS <= set(d["kernels"]), (name, d["kernels"])
        assert "wide_reset" in d["source"] and "wide_tile" in d["source"], name
    assert "k_gpick" in codegen(plans["mixed/max_d38_first_sum_count/grouped"])["kernels"]      # first / last keep their pass beside it
    # a merging plan may run partitioned: its merge kernel sweeps the records a second time
    for name in ("agg/max_d38/final/grouped", "agg/max_d38/partial_merge/grouped"):
        d = codegen(plans[name])
        assert "k_gpmerge" in d["kernels"] and "wide_merge" in d["source"], name
    d = codegen(plans["agg/max_d38/partial/grouped"])
    assert "k_gpmerge" not in d["kernels"] and "wide_merge" not in d["source"]


def test_plans_without_a_wide_grouped_min_max_list_none_of_them(corpus_tool):
    unchanged = {
        "tpch/grouped_min_max": dict(corpus_tool.tpch_plans())["tpch/grouped_min_max"],
        "tpch/q1": tpch.q1_plan(),
        "agg/max_d38/partial/ungrouped": S.hash_agg(S.scan(corpus_tool.FIELDS), [], [S.max_(corpus_tool.DD38, D38)]),
        "agg/max_d38/final/ungrouped": S.hash_agg(S.scan([D38]), [], [S.max_(S.col(0, D38), D38)], S.FINAL),
    }
    for name, plan in unchanged.items():
        d = codegen(plan, 32)
        assert not (WIDE_KERNELS & set(d["kernels"])), (name, d["kernels"])
        assert "wide_" not in d["source"] and "k_gw" not in d["source"], name


def test_static_shortcut(corpus_tool):
    """max(cast(decimal(12,2) AS decimal(22,2))): |v| < 10^12 < 2^63 — the one-word max on the narrow value, widened on the way out; no extra word, no extra pass"""
    plan = dict(corpus_tool.wide_min_max_plans())["shortcut/max_cast_d12_as_d22/grouped"]
    assert "max -> Decimal128(22, 2)" in accepted(plan)
    d = codegen(plan)
    assert not (WIDE_KERNELS & set(d["kernels"])) and "wide_" not in d["source"]
    assert "G_IMAX64" in d["source"]
    # a bare wide column never qualifies (10^19 > 2^63)
    bare = S.hash_agg(S.scan([I32, S.decimal(19, 0)]), [S.col(0, I32)], [S.max_(S.col(1, S.decimal(19, 0)), S.decimal(19, 0))])
    assert WIDE_KERNELS <= set(codegen(bare)["kernels"])


def test_state_column_is_the_values_own_type(corpus_tool):
    plans = dict(corpus_tool.wide_min_max_plans())
    for name in LIFTED:
        out = codegen(plans[name])["out"]
        assert (out[1]["type"], out[1]["precision"], out[1]["scale"], out[1]["nullable"]) == (S.DECIMAL, 38, 4, True), (name, out[1])


def test_the_new_corpus_generates_what_was_recorded(corpus_tool):
    with open(os.path.join(ROOT, "tests", "golden", "wide_min_max_codegen.json")) as f:
        want = json.load(f)
    got = corpus_tool.wide_min_max_corpus()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name
    assert not [n for n, e in want.items() if any(v.startswith("refused: ") for v in e.values())]
    assert set(LIFTED) <= set(want) and "shortcut/max_cast_d12_as_d22/grouped" in want and "mixed/max_d38_first_sum_count/grouped" in want


def test_the_three_entries_are_retired_with_their_recorded_text(corpus_tool):
    assert sorted(corpus_tool.RETIRED_WIDE_MIN_MAX) == LIFTED
    retired = corpus_tool.retired()
    assert set(LIFTED) <= set(retired) and set(corpus_tool.RETIRED) <= set(retired)
    with open(os.path.join(ROOT, "tests", "golden", "codegen_corpus.json")) as f:
        old = json.load(f)
    for name in LIFTED:
        assert retired[name][0] == "refused: " + REFUSAL
        assert old[name] == {"check": retired[name][0], "valid_off": retired[name][0], "valid_on": retired[name][0]}, name
    names = [n for n, _ in corpus_tool.aggregate_plans()]
    assert not (set(LIFTED) & set(names)) and "agg/max_d38/partial/ungrouped" in names
    assert not (set(LIFTED) & set(dict(corpus_tool.all_plans())))


def test_compat_sheet():
    sheet = _tool("compat_sheet").render()
    with open(os.path.join(ROOT, "COMPAT.md")) as f:
        assert f.read() == sheet, "COMPAT.md is stale: python tools/compat_sheet.py --write"
    assert "not decimal(>18) in grouped aggregates" not in sheet
    assert "decimal(> 18) in grouped aggregates" not in sheet
