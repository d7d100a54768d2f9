"""The ANSI / TRY integer sum and unscaled_value / make_decimal GPU tests (tests/test_ansi_try_sum_gpu.py) on the HOST: their plans' generated per-row feed, fold,
combine and finalize code, compiled with g++ and driven by tests/emu/codegen_emu.py, against the same model.

The emulator raises the executor's errors for the flags a Filter / Projection chain sets; an aggregate's "cannot be decided order-independently" flag (16) is not among
them, so here it is given the executor's text for it (exec_pipeline.cpp raise_device_errors; ARITHMETIC_OVERFLOW, flag 2, comes first there as well).

Left to the device: which table a group goes through (chunking, the global table, the partitioned merge), and the plan that puts a Projection above the Final
aggregate (the executor materialises the aggregate's output between the two pipelines)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from datafusion_comet_amd import native  # noqa: E402
from tests.emu import codegen_emu as E  # noqa: E402

MODES, TYPES = ("ansi", "try"), ("Int8", "Int32", "Int64")
CASES = ([("test_scalar_functions", {})] + [("test_ungrouped", {"mode": m, "tname": t}) for m in MODES for t in TYPES] +
         [("test_grouped", {"mode": m, "tname": t, "ngroups": g}) for m in MODES for t in TYPES for g in (3, 700)] + [("test_grouped", {"mode": m, "tname": "Int64", "ngroups": 40_000}) for m in MODES] +
         [("test_partial_final_and_partial_merge", {"mode": m, "grouped": g}) for m in MODES for g in (False, True)] +
         [("test_an_order_dependent_sum_fails_by_name", {"mode": m, "grouped": g}) for m in MODES for g in (False, True)])


@pytest.fixture
def undecided_flag_as_the_executor_words_it(monkeypatch):
    raise_flags = E._raise_like_the_executor

    def raise_like_the_executor(flags, block, plan):
        try:
            raise_flags(flags, block, plan)
        except E.DeviceError as e:
            if e.flags & 16:
                raise native.CometNativeException("decimal or ANSI/TRY integer sum overflow cannot be decided order-independently for this input (mixed signs beyond the type's bound); "
                                                  "exact sequential evaluation is not implemented")
            raise
    monkeypatch.setattr(E, "_raise_like_the_executor", raise_like_the_executor)


@pytest.mark.parametrize("fn,params", CASES, ids=[f"{f}{''.join(f'-{k}={v}' for k, v in p.items())}" for f, p in CASES])
def test_gpu_test_on_host(built, undecided_flag_as_the_executor_words_it, fn, params):
    assert E.run_gpu_test_on_host("tests.test_ansi_try_sum_gpu", fn, **params) == "ok"
