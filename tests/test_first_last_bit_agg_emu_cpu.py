"""The first / last / bit-aggregate GPU tests (tests/test_first_last_bit_agg_gpu.py) on the HOST: their plans' generated per-row feed, fold, combine, pick and emit
code, compiled with g++ and driven by tests/emu/codegen_emu.py, against the same expectations.

The emulator's grouped driver stands in for the device's tables with a map and knows nothing of first / last; here it is given the one extra step the executor takes for
them: P::pick on every group behind the pass over the chunk, before the groups are emitted (one chunk, so every winning ordinal is a row of it).

Left to the device: everything about WHICH table a group goes through (chunking, the global table's re-run, the partitioned merge) and the cases that read metrics or
take two inputs."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.emu import codegen_emu as E  # noqa: E402

EMIT = "for (auto& k : order) P::emit_group(prm, k.data(), global[k].data(), pos++);"
PICK_THEN_EMIT = ("for (auto& k : order) { if constexpr (requires { P::pick(prm, (u64*)nullptr); }) P::pick(prm, global[k].data()); "
                  "P::emit_group(prm, k.data(), global[k].data(), pos++); }")

CASES = [("test_small_shapes", {"grouped": False}), ("test_small_shapes", {"grouped": True}), ("test_every_value_type", {"grouped": False}),
         ("test_every_value_type", {"grouped": True}), ("test_filters", {}), ("test_partial_final_and_partial_merge", {"grouped": False}),
         ("test_partial_final_and_partial_merge", {"grouped": True}), ("test_bit_aggregate_corners", {"grouped": False}), ("test_bit_aggregate_corners", {"grouped": True})]


@pytest.fixture
def driver_with_pick(monkeypatch):
    assert E.DRIVER.count(EMIT) == 1
    monkeypatch.setattr(E, "DRIVER", E.DRIVER.replace(EMIT, PICK_THEN_EMIT))


@pytest.mark.parametrize("fn,params", CASES, ids=[f"{f}{''.join(f'-{k}={v}' for k, v in p.items())}" for f, p in CASES])
def test_gpu_test_on_host(built, driver_with_pick, fn, params):
    assert E.run_gpu_test_on_host("tests.test_first_last_bit_agg_gpu", fn, **params) == "ok"
