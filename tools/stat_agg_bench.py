#!/usr/bin/env python3
"""Statistical aggregates on HBM-resident Float64 columns, one GPU, at SF100 lineitem scale (600 M rows): avg(x) vs stddev_samp(x) vs corr(x, y),
ungrouped, Q1-shaped (4 groups) and about 1 M groups (Partial stage).  Prints per case the task time (wall clock, best of --reps), the kernel
time (HIP events inside libcomet), the algorithmic bytes (8 B per row per Float64 column read, 4 B per row of the Int32 key) and that as a fraction
of 8 TB/s.  Kernel-level statistics come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/stat_agg_bench.py --reps 1`."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(native, plan_bytes, table, ncols, reps, grouped):
    import torch
    best_k, best_w, rows = None, None, 0
    for r in range(reps + 1):
        inp = native.DeviceInput(table)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = native.Native.createPlan([inp], plan_bytes, b"", 1, 0, 0)
        try:
            if grouped:
                out = native.Native.executePlanDevice(h, ncols)
                rows = out.num_rows if out is not None else 0
                del out
            else:      # an ungrouped result is one row, exported through executePlan
                rows = 0
                while (b := native.Native.executePlan(h, ncols)) is not None:
                    rows += b.num_rows
            torch.cuda.synchronize()
            w = time.perf_counter() - t0
            ms, launches, _ = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
            native.lib().comet_plan_kernel_stats(h, ctypes.byref(ms), ctypes.byref(launches), ctypes.byref(_))
        finally:
            native.Native.releasePlan(h)
        if r:
            best_k = ms.value if best_k is None else min(best_k, ms.value)
            best_w = w if best_w is None else min(best_w, w)
    return best_k, best_w * 1e3, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=600_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import datafusion_comet_amd  # noqa: F401 — before torch: the JIT then compiles with the installed ROCm's compiler (see that module)
    import pyarrow as pa
    import torch
    from datafusion_comet_amd import native, serde as S
    n = a.rows
    torch.manual_seed(0)
    # prices with cent-level spread around 5 000, a correlated second column; keys: 4 groups (Q1) and 2^20 groups
    x = torch.round((5000.0 + 1000.0 * torch.randn(n, dtype=torch.float64, device="cuda")) * 100.0) / 100.0
    y = 0.5 * x + torch.round(100.0 * torch.randn(n, dtype=torch.float64, device="cuda")) / 100.0
    g4 = torch.randint(0, 4, (n,), dtype=torch.int32, device="cuda")
    g1m = torch.randint(0, 1 << 20, (n,), dtype=torch.int32, device="cuda")
    schema = pa.schema([("x", pa.float64()), ("y", pa.float64()), ("g4", pa.int32()), ("g1m", pa.int32())])
    dt = native.DeviceTable(schema, n, [t.view(torch.uint8) for t in (x, y, g4, g1m)], [None] * 4, "cuda:0")
    F64, I32 = S.T_DOUBLE, S.T_INT32
    cx, cy = S.col(0, F64), S.col(1, F64)
    funcs = {"avg(x)": ([S.avg(cx, F64, F64)], 2, 1), "stddev_samp(x)": ([S.stddev(cx)], 3, 1), "corr(x, y)": ([S.corr(cx, cy)], 6, 2)}
    shapes = {"ungrouped": [], "4 groups": [S.col(2, I32)], "1M groups": [S.col(3, I32)]}
    results = []
    for shape, keys in shapes.items():
        for fn, (aggs, width, ncols_read) in funcs.items():
            plan = S.hash_agg(S.scan([F64, F64, I32, I32]), keys, aggs).encode()
            native.compile_plan(plan)
            k_ms, w_ms, rows = run(native, plan, dt, len(keys) + width, a.reps, bool(keys))
            nbytes = n * (8 * ncols_read + (4 if keys else 0))
            r = {"shape": shape, "fn": fn, "rows": n, "groups_out": rows, "task_ms": round(w_ms, 3), "kernel_ms": round(k_ms, 3),
                 "algorithmic_GB": round(nbytes / 1e9, 3), "fraction_of_8TBps": round(nbytes / (k_ms * 1e-3) / 8e12, 3)}
            print(json.dumps(r), flush=True)
            results.append(r)
    if a.out:      # the command that produced the numbers (where they were written is not part of it)
        cmd = ["python", "tools/stat_agg_bench.py", "--rows", str(a.rows), "--reps", str(a.reps)]
        with open(a.out, "w") as f:
            json.dump({"command": " ".join(cmd), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
