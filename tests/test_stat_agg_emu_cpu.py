"""The statistical-aggregate GPU tests (tests/test_stat_agg_gpu.py) on the HOST: their plans' generated per-row feed, fold, combine and emit code and
the device helpers it calls, compiled with g++ and driven by tests/emu/codegen_emu.py, against the same exact expectations.

Left to the device: test_stddev_above_a_hash_join (two inputs: the join runs in the executor's own kernels) and the 40 000-group case of
test_partial_states_and_final_results_are_exact (the global-table spill is a property of the device's LDS table, which the emulator replaces with a map)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.emu import codegen_emu as E  # noqa: E402

CASES = [("test_reference_vectors", {"grouped": False}), ("test_reference_vectors", {"grouped": True}),
         ("test_partial_states_and_final_results_are_exact", {"ngroups": 0}), ("test_partial_states_and_final_results_are_exact", {"ngroups": 5}),
         ("test_corr_follows_the_grouped_and_ungrouped_formulas", {}), ("test_same_bits_for_any_order_batching_and_window", {}),
         ("test_partial_final_and_partial_merge", {}), ("test_edge_cases", {}), ("test_ill_conditioned_data", {})]


@pytest.mark.parametrize("fn,params", CASES, ids=[f"{f}{''.join(f'-{k}={v}' for k, v in p.items())}" for f, p in CASES])
def test_stat_gpu_test_on_host(built, fn, params):
    assert E.run_gpu_test_on_host("tests.test_stat_agg_gpu", fn, **params) == "ok"
