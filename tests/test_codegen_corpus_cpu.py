"""The pipeline generator's output over a fixed corpus of plans (tools/codegen_corpus.py), without a GPU: every aggregate kind in every mode, grouped and ungrouped,
with validity off and on; every group-key encoder; the Output sink's column kinds; the caps and refusals; the TPC-H plans.  tests/golden/codegen_corpus.json was
recorded at the commit before generate_pipeline was split into one lowering per aggregate family (python tools/codegen_corpus.py --out
tests/golden/codegen_corpus.json on that commit with only the tool added): kernel source, kernels, descriptors, explain and refusal texts are what they were, byte
for byte — the JIT cache key is a hash of the source, and the host emulator patches the source textually."""
import hashlib
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from datafusion_comet_amd import native, serde as S, tpch  # noqa: E402

I32, I64, F64 = S.T_INT32, S.T_INT64, S.T_DOUBLE


def _tool():
    spec = importlib.util.spec_from_file_location("codegen_corpus", os.path.join(ROOT, "tools", "codegen_corpus.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_every_plan_of_the_corpus_generates_what_it_did():
    with open(os.path.join(ROOT, "tests", "golden", "codegen_corpus.json")) as f:
        want = json.load(f)
    got = _tool().corpus()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], f"{name}: the generated code, its descriptors or its explain / refusal text changed"
    # the corpus is wide and mostly generates: refusals (recorded with their text) are at most one entry in ten
    refused = [n for n, e in want.items() if any(v.startswith("refused: ") for v in e.values())]
    assert len(want) >= 300 and 10 * len(refused) <= len(want), (len(want), refused)


def test_plans_without_the_new_kinds_generate_the_source_they_did():
    """The generated kernel source of TPC-H Q1 and Q6 and of a grouped min / max plan, against the SHA-256 recorded from the commit before first / last and the bit
    aggregates (tests/golden/first_last_bit_agg_codegen.json): no word, no functor and no kernel is added to a plan that uses none of them."""
    with open(os.path.join(ROOT, "tests", "golden", "first_last_bit_agg_codegen.json")) as f:
        want = json.load(f)
    mm = S.hash_agg(S.scan([I32, I64, F64]), [S.col(0, I32)], [S.min_(S.col(1, I64), I64), S.max_(S.col(1, I64), I64), S.min_(S.col(2, F64), F64), S.max_(S.col(2, F64), F64),
                                                            S.count(S.col(1, I64))])
    plans = {"q1": (tpch.q1_plan(), [False] * 7), "q1_nullable": (tpch.q1_plan(), [True] * 7), "grouped_min_max": (mm, [False, True, True]), "q6": (tpch.q6_plan(), [False] * 4)}
    assert sorted(plans) == sorted(want)
    for name, (plan, hv) in plans.items():
        src = native.plan_codegen(plan.encode(), hv)["source"].encode()
        assert "pick" not in src.decode() and "iarg[3]" not in src.decode(), name
        assert (hashlib.sha256(src).hexdigest(), len(src)) == (want[name]["sha256"], want[name]["bytes"]), name
