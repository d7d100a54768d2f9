#!/usr/bin/env python3
"""What first / last cost in a grouped aggregate: first(x), last(x) against min(x), max(x) of the same HBM-resident Int64 column, one GPU, 64 M rows in about
1 M groups (Partial stage, one chunk).  min / max is the yardstick because it does the same per-row work on a 64-bit word per function (an LDS / global min and
max) without the pick pass.  Prints per case the task time (wall clock, best of --reps) and the kernel time (HIP events inside libcomet: every launch of the task,
k_gpick included).  The pick kernel's own time comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/first_last_bench.py --reps 1`."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(native, plan_bytes, table, ncols, reps):
    import torch
    best_k, best_w, rows, nl = None, None, 0, 0
    for r in range(reps + 1):
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
            best_k = ms.value if best_k is None else min(best_k, ms.value)
            best_w = w if best_w is None else min(best_w, w)
            nl = launches.value
    return best_k, best_w * 1e3, rows, nl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64_000_000)
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import datafusion_comet_amd  # noqa: F401 — before torch: the JIT then compiles with the installed ROCm's compiler (see that module)
    import pyarrow as pa
    import torch
    from datafusion_comet_amd import native, serde as S
    n = a.rows
    torch.manual_seed(0)
    x = torch.randint(-(1 << 40), 1 << 40, (n,), dtype=torch.int64, device="cuda")
    g = torch.randint(0, a.groups, (n,), dtype=torch.int32, device="cuda")
    schema = pa.schema([("x", pa.int64()), ("g", pa.int32())])
    dt = native.DeviceTable(schema, n, [t.view(torch.uint8) for t in (x, g)], [None] * 2, "cuda:0")
    I64, I32 = S.T_INT64, S.T_INT32
    cx = S.col(0, I64)
    cases = {"min(x), max(x)": ([S.min_(cx, I64), S.max_(cx, I64)], 2), "first(x), last(x)": ([S.first_(cx, I64), S.last_(cx, I64)], 4)}
    results = []
    for name, (aggs, width) in cases.items():
        plan = S.hash_agg(S.scan([I64, I32]), [S.col(1, I32)], aggs).encode()
        native.compile_plan(plan)
        k_ms, w_ms, rows, launches = run(native, plan, dt, 1 + width, a.reps)
        r = {"aggregates": name, "rows": n, "groups_out": rows, "task_ms": round(w_ms, 3), "kernel_ms": round(k_ms, 3), "timed_launches": launches}
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out:      # the command that produced the numbers (where they were written is not part of it)
        cmd = ["python", "tools/first_last_bench.py", "--rows", str(a.rows), "--groups", str(a.groups), "--reps", str(a.reps)]
        with open(a.out, "w") as f:
            json.dump({"command": " ".join(cmd), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
