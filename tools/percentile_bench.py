#!/usr/bin/env python3
"""What Spark's exact percentile costs on one GPU next to the engine's Sort, over one HBM-resident table of --rows (Int32 key, Float64 value) rows, at each
--groups count (default: 4 and 1 000 000 groups).  Per group count three plans over the same table, run in turn inside each repetition (so drift hits them alike):
  sort      Sort by (key ASC NULLS FIRST, value ASC NULLS LAST): the yardstick — the aggregate's own first step, alone
  partial   HashAggregate(Partial, [key], [percentile(value, 0.5)]): sort, group boundaries, the List<Float64> state
  final     HashAggregate(Final) over that Partial in ONE plan — a device-resident input stream cannot carry a list column, so the state reaches the Final
            resident, from the Partial below it; final − partial is the Final stage alone: flatten the lists, sort again, pick
No plan's time holds the copy of a 100 M-row result to the host: sort runs under a Limit 1 and partial under a Projection of its key column (not a Limit: taking
one row of a list column gathers that row's elements, 25 M of them at 4 groups); the operator below still produces its whole result in HBM.
Per plan the task time: a host clock around createPlan … the last executePlan, closed by a device synchronise; --warmup repetitions first, then --reps timed
ones; median and best.  The kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/percentile_bench.py --reps 1 --warmup 1`."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_once(native, plan_bytes, table, ncols, keep_result):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    it = native.CometExecIterator([native.DeviceInput(table)], ncols, plan_bytes, batch_size=0)
    rows, first = 0, None
    try:
        while True:
            b = native.Native.executePlan(it.handle, ncols)
            if b is None:
                break
            rows += b.num_rows
            if keep_result and first is None:
                first = b
        torch.cuda.synchronize()
        w = time.perf_counter() - t0
    finally:
        it.close()
    return w * 1e3, rows, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--groups", type=int, nargs="+", default=[4, 1_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import datafusion_comet_amd  # noqa: F401 — before torch: the JIT then compiles with the installed ROCm's compiler (see that module)
    import pyarrow as pa
    import torch
    from datafusion_comet_amd import native, serde as S
    I32, F64 = S.T_INT32, S.T_DOUBLE
    torch.manual_seed(0)
    schema = pa.schema([("k", pa.int32()), ("x", pa.float64())])
    results = []
    for groups in a.groups:
        k = torch.randint(0, groups, (a.rows,), dtype=torch.int32, device="cuda")
        x = torch.rand(a.rows, dtype=torch.float64, device="cuda") * 2e6 - 1e6
        table = native.DeviceTable(schema, a.rows, [k.view(torch.uint8).reshape(-1), x.view(torch.uint8).reshape(-1)], [None, None], "cuda:0")
        scan = S.scan([I32, F64])
        partial = S.hash_agg(scan, [S.col(0, I32)], [S.percentile(S.col(1, F64), 0.5)], S.PARTIAL)
        final = S.hash_agg(partial, [S.col(0, I32)], [S.percentile(S.col(1, F64), 0.5)], S.FINAL)
        plans = {"sort": (S.limit(S.sort(scan, [(S.col(0, I32), False, False), (S.col(1, F64), False, True)]), 1), 2),
                 "partial": (S.project(partial, [S.col(0, I32)]), 1), "final": (final, 2)}
        times = {name: [] for name in plans}
        out_rows = {}
        median_of_group0 = None
        for rep in range(a.warmup + a.reps):
            for name, (plan, ncols) in plans.items():
                ms, rows, first = run_once(native, plan.encode(), table, ncols, name == "final" and rep == 0)
                out_rows[name] = rows
                if first is not None:      # one spot check against torch: the median of the first group the result lists
                    g0 = first.column(0).to_pylist()[0]
                    sel = torch.sort(x[k == g0]).values
                    n = sel.numel()
                    pos = float(n - 1) * 0.5
                    lo_i, hi_i = math.floor(pos), math.ceil(pos)
                    lo, hi = sel[lo_i].item(), sel[hi_i].item()
                    want = lo if lo_i == hi_i or lo == hi else (float(hi_i) - pos) * lo + (pos - float(lo_i)) * hi
                    got = first.column(1).to_pylist()[0]
                    if got != want:
                        raise SystemExit(f"percentile_bench: group {g0}: got {got!r}, torch's sort and the formula give {want!r}")
                    median_of_group0 = got
                if rep >= a.warmup:
                    times[name].append(ms)
        r = {"rows": a.rows, "groups": groups, "out_rows": out_rows, "median_of_first_group": median_of_group0}
        for name, ts in times.items():
            r[name + "_ms_by_rep"] = [round(t, 2) for t in ts]
            r[name + "_ms_median"] = round(statistics.median(ts), 2)
            r[name + "_ms_best"] = round(min(ts), 2)
        r["final_stage_alone_ms_median"] = round(r["final_ms_median"] - r["partial_ms_median"], 2)
        r["partial_over_sort"] = round(r["partial_ms_median"] / r["sort_ms_median"], 3)
        r["final_stage_alone_over_sort"] = round(r["final_stage_alone_ms_median"] / r["sort_ms_median"], 3)
        r["partial_plus_final_over_sort"] = round(r["final_ms_median"] / r["sort_ms_median"], 3)
        print(json.dumps(r), flush=True)
        results.append(r)
        del table, k, x
        torch.cuda.empty_cache()
    if a.out:      # the command that produced the numbers (where they were written is not part of it)
        cmd = ["python", "tools/percentile_bench.py", "--rows", str(a.rows), "--groups", *map(str, a.groups), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        with open(a.out, "w") as f:
            json.dump({"command": " ".join(cmd), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
