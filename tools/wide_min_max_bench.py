#!/usr/bin/env python3
"""What a grouped min / max of a decimal wider than 18 digits costs: min(d), max(d) of an HBM-resident decimal(38,4) column against min(x), max(x) of an Int64 column over
the same Int32 keys, one GPU, 64 M rows in one chunk (Partial stage), at 5, 2^10 and 2^20 groups.  The Int64 plan is the yardstick: it does the same per-row work on one
64-bit word per function and generates the source it always generated.  The wide plan reads wider rows twice (k_gagg settles the high words, k_gwlow the low words), so the
planning figure is  yardstick × 2 × (4 + 16) / (4 + 8).
Three value orders, every row with the same high word so that every row reaches the test before the atomic: random low words, ascending within each group (adversarial
for max: every row beats what it reads) and descending (the same for min).
Per case: the kernel time (HIP events inside libcomet around every launch of the task — k_gagg, k_gwreset, k_gwlow, k_gemit, table growth) as best and median of --reps
runs behind one warm-up run, and the task's wall clock.  The per-kernel split comes from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/wide_min_max_bench.py --reps 1`."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(native, plan_bytes, table, ncols, reps):
    import torch
    ks, ws, rows, nl = [], [], 0, 0
    for r in range(reps + 1):      # (run 0 warms the code objects and the allocator up)
        inp = native.DeviceInput(table)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = native.Native.createPlan([inp], plan_bytes, b"", 1, 0, 0)
        try:
            out = native.Native.executePlanDevice(h, ncols)
            rows = out.num_rows if out is not None else 0
            del out
            torch.cuda.synchronize()
            w = time.perf_counter() - t0
            ms, launches, _ = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
            native.lib().comet_plan_kernel_stats(h, ctypes.byref(ms), ctypes.byref(launches), ctypes.byref(_))
        finally:
            native.Native.releasePlan(h)
        if r:
            ks.append(ms.value)
            ws.append(w * 1e3)
            nl = launches.value
    return ks, ws, rows, nl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64_000_000)
    ap.add_argument("--groups", type=int, nargs="*", default=[5, 1 << 10, 1 << 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import datafusion_comet_amd  # noqa: F401 — before torch: the JIT then compiles with the installed ROCm's compiler (see that module)
    import pyarrow as pa
    import torch
    from datafusion_comet_amd import native, serde as S
    n = a.rows
    I64, I32, D = S.T_INT64, S.T_INT32, S.decimal(38, 4)
    plans = {
        "int64": (S.hash_agg(S.scan([I64, I32]), [S.col(1, I32)], [S.min_(S.col(0, I64), I64), S.max_(S.col(0, I64), I64)]).encode(), pa.int64()),
        "decimal(38,4)": (S.hash_agg(S.scan([D, I32]), [S.col(1, I32)], [S.min_(S.col(0, D), D), S.max_(S.col(0, D), D)]).encode(), pa.decimal128(38, 4)),
    }
    for p, _ in plans.values():
        native.compile_plan(p)
    torch.manual_seed(0)
    results = []
    for groups in a.groups:
        g = torch.randint(0, groups, (n,), dtype=torch.int32, device="cuda")
        x = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device="cuda")
        # the low word as a signed tensor holding the unsigned bits: random covers all 64 bits; the sorted orders climb / fall through them with the row index
        step = ((1 << 64) - 1) // max(n, 1)
        ramp_bits = torch.arange(n, dtype=torch.int64, device="cuda") * step      # (wraps: the bits of i · step < 2^64, climbing in unsigned order)
        orders = {"random": torch.randint(torch.iinfo(torch.int64).min, torch.iinfo(torch.int64).max, (n,), dtype=torch.int64, device="cuda"),
                  "ascending": ramp_bits, "descending": torch.flip(ramp_bits, [0])}
        cases = [("int64", "random", x)]
        for order, lo in orders.items():
            d = torch.empty((n, 2), dtype=torch.int64, device="cuda")
            d[:, 0] = lo
            d[:, 1] = 1      # one high word for every row
            cases.append(("decimal(38,4)", order, d))
            del d
        yard = None
        for vtype, order, col in cases:
            plan, at = plans[vtype]
            dt = native.DeviceTable(pa.schema([("v", at), ("g", pa.int32())]), n, [col.view(torch.uint8).reshape(-1), g.view(torch.uint8)], [None] * 2, "cuda:0")
            ks, ws, rows, launches = run(native, plan, dt, 3, a.reps)
            r = {"value": vtype, "order": order, "rows": n, "groups": groups, "groups_out": rows, "kernel_ms_best": round(min(ks), 3), "kernel_ms_median": round(statistics.median(ks), 3),
                 "kernel_ms_all": [round(k, 3) for k in ks], "task_ms_best": round(min(ws), 3), "timed_launches": launches}
            if vtype == "int64":
                yard = r["kernel_ms_median"]
            else:
                r["expected_ms"] = round(yard * 2 * (4 + 16) / (4 + 8), 3)
                r["over_expected"] = round(r["kernel_ms_median"] / r["expected_ms"], 2)
            print(json.dumps(r), flush=True)
            results.append(r)
            del dt
        del cases, orders, g, x
        torch.cuda.empty_cache()
    if a.out:      # the command that produced the numbers (where they were written is not part of it)
        cmd = ["python", "tools/wide_min_max_bench.py", "--rows", str(a.rows), "--groups"] + [str(v) for v in a.groups] + ["--reps", str(a.reps)]
        with open(a.out, "w") as f:
            json.dump({"command": " ".join(cmd), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
