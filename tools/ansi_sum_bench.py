#!/usr/bin/env python3
"""What an ANSI integer sum costs in a grouped aggregate, and what Spark's rewrite of a short-decimal sum saves: one GPU, 64 M rows of HBM-resident columns in about
1 M groups (Partial stage, one chunk).  Three comparisons, every plan of a comparison run in turn inside each repetition (so drift hits them alike), best of --reps:
  1. LEGACY sum(x: Int64)                   count + one wrapping 64-bit sum
  2. ANSI   sum(x: Int64)                   count + the positive and the negative sum, 128 bits each (two limbs each in LDS)
  3. sum(d: decimal(7,2)) -> decimal(17,2)  the direct plan: Sum128 and its (sum, is_empty) state …
     ANSI sum(unscaled_value(d))            … and what DecimalAggregates makes of it: proven not to overflow, LEGACY's words with one limb
     and, for both forms of 3, the Final stage over the Partial's output (the rewritten one under Projection(make_decimal(sum, 17, 2))).
Prints per plan the task time (wall clock) and the kernel time (HIP events inside libcomet around every launch of the task), and per repetition the kernel times, whose
spread is the yardstick for a difference.  The kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/ansi_sum_bench.py --reps 1`."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_once(native, plan_bytes, table, ncols, keep=False):
    import torch
    inp = native.DeviceInput(table)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = native.Native.createPlan([inp], plan_bytes, b"", 1, 0, 0)
    try:
        out = native.Native.executePlanDevice(h, ncols)
        rows = out.num_rows if out is not None else 0
        kept = out.to_arrow() if keep and out is not None else None
        del out
        torch.cuda.synchronize()
        w = time.perf_counter() - t0
        ms, launches, _ = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
        native.lib().comet_plan_kernel_stats(h, ctypes.byref(ms), ctypes.byref(launches), ctypes.byref(_))
    finally:
        native.Native.releasePlan(h)
    return ms.value, w * 1e3, rows, launches.value, kept


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
    lo = torch.randint(-(10**7 - 1), 10**7, (n,), dtype=torch.int64, device="cuda")
    d = torch.stack([lo, lo >> 63], dim=1).contiguous()      # Decimal128: 16 little-endian bytes a value
    del lo
    schema = pa.schema([("x", pa.int64()), ("g", pa.int32()), ("d", pa.decimal128(7, 2))])
    dt = native.DeviceTable(schema, n, [t.view(torch.uint8).reshape(-1) for t in (x, g, d)], [None] * 3, "cuda:0")
    I64, I32, D72, D17 = S.T_INT64, S.T_INT32, S.decimal(7, 2), S.decimal(17, 2)
    cx, cg, cd = S.col(0, I64), S.col(1, I32), S.col(2, D72)
    scan = lambda: S.scan([I64, I32, D72])
    direct, rewritten = S.sum_(cd, D17), S.sum_(S.unscaled_value(cd), I64, S.ANSI)
    partial = {"legacy sum(int64)": (S.hash_agg(scan(), [cg], [S.sum_(cx, I64)]), 2), "ansi sum(int64)": (S.hash_agg(scan(), [cg], [S.sum_(cx, I64, S.ANSI)]), 2),
               "sum(decimal(7,2)) direct": (S.hash_agg(scan(), [cg], [direct]), 3), "ansi sum(unscaled_value(decimal(7,2)))": (S.hash_agg(scan(), [cg], [rewritten]), 2)}
    final = {"sum(decimal(7,2)) direct": (S.hash_agg(S.scan([I32, D17, S.T_BOOL]), [S.col(0, I32)], [direct], S.FINAL), 2),
             "ansi sum(unscaled_value(decimal(7,2)))": (S.project(S.hash_agg(S.scan([I32, I64]), [S.col(0, I32)], [rewritten], S.FINAL),
                                                                  [S.col(0, I32), S.make_decimal(S.col(1, I64), 17, 2, null_on_overflow=False)]), 2)}
    for plan, _ in list(partial.values()) + list(final.values()):
        native.compile_plan(plan.encode())
    states, results = {}, {}

    def note(stage, name, rep, k_ms, w_ms, rows, launches):
        r = results.setdefault((stage, name), {"stage": stage, "plan": name, "rows_in": None, "rows_out": rows, "timed_launches": launches, "kernel_ms_by_rep": [], "task_ms_by_rep": []})
        if rep:      # (the first turn warms the code-object cache and the allocator)
            r["kernel_ms_by_rep"].append(round(k_ms, 3))
            r["task_ms_by_rep"].append(round(w_ms, 3))

    for rep in range(a.reps + 1):
        for name, (plan, ncols) in partial.items():
            k_ms, w_ms, rows, launches, kept = run_once(native, plan.encode(), dt, ncols, keep=rep == 0 and name in final)
            if kept is not None:
                states[name] = native.DeviceTable.from_arrow(kept, "cuda:0")
            note("partial", name, rep, k_ms, w_ms, rows, launches)
            results[("partial", name)]["rows_in"] = n
        for name, (plan, ncols) in final.items():
            k_ms, w_ms, rows, launches, _ = run_once(native, plan.encode(), states[name], ncols)
            note("final", name, rep, k_ms, w_ms, rows, launches)
            results[("final", name)]["rows_in"] = states[name].num_rows
    out = []
    for r in results.values():
        r["kernel_ms"], r["task_ms"] = min(r["kernel_ms_by_rep"]), min(r["task_ms_by_rep"])
        r["kernel_ms_spread"] = round(max(r["kernel_ms_by_rep"]) - min(r["kernel_ms_by_rep"]), 3)
        print(json.dumps(r), flush=True)
        out.append(r)
    k = lambda stage, name: results[(stage, name)]["kernel_ms"]
    ratios = {"ansi_over_legacy_int64_partial": round(k("partial", "ansi sum(int64)") / k("partial", "legacy sum(int64)"), 3),
              "rewritten_over_direct_decimal_partial": round(k("partial", "ansi sum(unscaled_value(decimal(7,2)))") / k("partial", "sum(decimal(7,2)) direct"), 3),
              "rewritten_over_direct_decimal_final": round(k("final", "ansi sum(unscaled_value(decimal(7,2)))") / k("final", "sum(decimal(7,2)) direct"), 3)}
    print(json.dumps(ratios), flush=True)
    if a.out:      # the command that produced the numbers (where they were written is not part of it)
        cmd = ["python", "tools/ansi_sum_bench.py", "--rows", str(a.rows), "--groups", str(a.groups), "--reps", str(a.reps)]
        with open(a.out, "w") as f:
            json.dump({"command": " ".join(cmd), "results": out, "kernel_ms_ratios": ratios}, f, indent=1)


if __name__ == "__main__":
    main()
