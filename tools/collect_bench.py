#!/usr/bin/env python3
"""What collect_list and collect_set cost on one GPU next to the engine's Sort, over one HBM-resident table of --rows (Int32 key, Int64 value) rows, at each
--groups count (default: 4 and 1 000 000 groups).  Per group count six plans over the same table, run in turn inside each repetition (so drift hits them alike):
  sort_k        Sort by (key ASC NULLS FIRST): collect_list's yardstick — the aggregate's own first step, alone
  sort_kv       Sort by (key ASC NULLS FIRST, value ASC NULLS LAST): collect_set's yardstick
  list_partial  HashAggregate(Partial, [key], [collect_list(value)]): sort by the key, group boundaries, the List<Int64> state
  set_partial   HashAggregate(Partial, [key], [collect_set(value)]): sort by (key, value), boundaries and peer flags, kept rows, one gather of the elements
  list_final    HashAggregate(Final) over that Partial in ONE plan — a device-resident input stream cannot carry a list column, so the state reaches the Final
  set_final     resident, from the Partial below it; final − partial is the Final stage alone: flatten the lists, take keys and elements, then the Partial's path again
No plan's time holds the copy of a 100 M-row result to the host: the sorts run under a Limit 1, the aggregates under a Projection of their key column (not a
Limit: taking one row of a list column gathers that row's elements); the operator below still produces its whole result in HBM.
Per plan the task time: a host clock around createPlan … the last executePlan, closed by a device synchronise; --warmup repetitions first, then --reps timed
ones; median and best.  Before the timed runs the first group's list and set, taken from the Finals under a Limit 1, are compared with torch (the group's
values in row order; torch.unique of them)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_once(native, plan_bytes, table, ncols, keep_result=False):
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
    ap.add_argument("--values", type=int, default=1_000_000, help="the values are uniform in [0, VALUES)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import datafusion_comet_amd  # noqa: F401 — before torch: the JIT then compiles with the installed ROCm's compiler (see that module)
    import pyarrow as pa
    import torch
    from datafusion_comet_amd import native, serde as S
    I32, I64 = S.T_INT32, S.T_INT64
    torch.manual_seed(0)
    schema = pa.schema([("k", pa.int32()), ("x", pa.int64())])
    results = []
    for groups in a.groups:
        k = torch.randint(0, groups, (a.rows,), dtype=torch.int32, device="cuda")
        x = torch.randint(0, a.values, (a.rows,), dtype=torch.int64, device="cuda")
        table = native.DeviceTable(schema, a.rows, [k.view(torch.uint8).reshape(-1), x.view(torch.uint8).reshape(-1)], [None, None], "cuda:0")
        scan = S.scan([I32, I64])
        key = [S.col(0, I32)]
        fns = {"list": S.collect_list, "set": S.collect_set}
        partial = {f: S.hash_agg(scan, key, [fn(S.col(1, I64), I64)], S.PARTIAL) for f, fn in fns.items()}
        final = {f: S.hash_agg(partial[f], key, [fn(S.col(1, I64), I64)], S.FINAL) for f, fn in fns.items()}
        # the spot check, outside the timed runs
        checked = {}
        for f in fns:
            _, _, first = run_once(native, S.limit(final[f], 1).encode(), table, 2, True)
            g0 = first.column(0).to_pylist()[0]
            col = first.column(1)
            got = torch.from_numpy((col.chunk(0) if isinstance(col, pa.ChunkedArray) else col).flatten().to_numpy().copy())
            sel = x[k == g0].cpu()
            want = sel if f == "list" else torch.unique(sel, sorted=True)
            if got.numel() != want.numel() or not torch.equal(got, want):
                raise SystemExit(f"collect_bench: collect_{f} of group {g0}: {got.numel()} elements, torch gives {want.numel()}, or they differ")
            checked[f] = int(want.numel())
        plans = {"sort_k": (S.limit(S.sort(scan, [(S.col(0, I32), False, False)]), 1), 2),
                 "sort_kv": (S.limit(S.sort(scan, [(S.col(0, I32), False, False), (S.col(1, I64), False, True)]), 1), 2),
                 "list_partial": (S.project(partial["list"], key), 1), "set_partial": (S.project(partial["set"], key), 1),
                 "list_final": (S.project(final["list"], key), 1), "set_final": (S.project(final["set"], key), 1)}
        times = {name: [] for name in plans}
        out_rows = {}
        for rep in range(a.warmup + a.reps):
            for name, (plan, ncols) in plans.items():
                ms, rows, _ = run_once(native, plan.encode(), table, ncols)
                out_rows[name] = rows
                if rep >= a.warmup:
                    times[name].append(ms)
        r = {"rows": a.rows, "groups": groups, "values": a.values, "out_rows": out_rows, "first_group_elements_checked": checked}
        for name, ts in times.items():
            r[name + "_ms_by_rep"] = [round(t, 2) for t in ts]
            r[name + "_ms_median"] = round(statistics.median(ts), 2)
            r[name + "_ms_best"] = round(min(ts), 2)
        for f, yard in (("list", "sort_k"), ("set", "sort_kv")):
            alone = r[f + "_final_ms_median"] - r[f + "_partial_ms_median"]
            r[f + "_final_stage_alone_ms_median"] = round(alone, 2)
            r[f + "_partial_over_" + yard] = round(r[f + "_partial_ms_median"] / r[yard + "_ms_median"], 3)
            r[f + "_final_stage_alone_over_" + yard] = round(alone / r[yard + "_ms_median"], 3)
            r[f + "_round_trip_over_" + yard] = round(r[f + "_final_ms_median"] / r[yard + "_ms_median"], 3)
        print(json.dumps(r), flush=True)
        results.append(r)
        del table, k, x
        torch.cuda.empty_cache()
    if a.out:      # the command that produced the numbers (where they were written is not part of it)
        cmd = ["python", "tools/collect_bench.py", "--rows", str(a.rows), "--groups", *map(str, a.groups), "--values", str(a.values), "--reps", str(a.reps),
               "--warmup", str(a.warmup)]
        with open(a.out, "w") as f:
            json.dump({"command": " ".join(cmd), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
