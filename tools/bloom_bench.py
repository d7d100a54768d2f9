#!/usr/bin/env python3
"""What Spark's runtime Bloom filter costs on one GPU, over HBM-resident columns:
  1. build   bloom_filter_agg(xxhash64(k)) Partial over --build-rows longs into 2^23 bits with 6 hash functions (Spark's default runtime filter: 1 MiB, the global
             atomicOr path of bloom_put_kernel)
  2. probe   scan -> Filter(o > 0 AND might_contain(filter, xxhash64(fk))) -> count over --probe-rows rows, against the same chain with `o > 0` alone; the filter
             holds --keys keys of the probe column's range, about half of the probe keys are in it
Every plan runs in turn inside each repetition (so drift hits them alike); per plan the task time (wall clock) and the kernel time (HIP events inside libcomet
around the task's launches), best of --reps.  The kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/bloom_bench.py --reps 1`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_once(native, plan_bytes, table, ncols, subqueries=None):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    it = native.CometExecIterator([native.DeviceInput(table)], ncols, plan_bytes, batch_size=0, subqueries=subqueries)
    try:
        out = []
        while True:
            b = native.Native.executePlan(it.handle, ncols)
            if b is None:
                break
            out.append(b)
        torch.cuda.synchronize()
        w = time.perf_counter() - t0
        ms, launches, _ = it.kernel_stats()
    finally:
        it.close()
    return ms, w * 1e3, launches, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-rows", type=int, default=10_000_000)
    ap.add_argument("--probe-rows", type=int, default=100_000_000)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import datafusion_comet_amd  # noqa: F401 — before torch: the JIT then compiles with the installed ROCm's compiler (see that module)
    import pyarrow as pa
    import torch
    from datafusion_comet_amd import native, serde as S
    I64, I32, BIN = S.T_INT64, S.T_INT32, S.T_BINARY
    bits, items = 1 << 23, 969_077      # round(2^23 / 969 077 · ln 2) = 6
    torch.manual_seed(0)

    def table(cols, names):
        n = len(cols[0])
        schema = pa.schema([(nm, pa.int64() if c.dtype == torch.int64 else pa.int32()) for nm, c in zip(names, cols)])
        return native.DeviceTable(schema, n, [c.view(torch.uint8).reshape(-1) for c in cols], [None] * len(cols), "cuda:0")

    xx = S.scalar_func("xxhash64", [S.col(0, I64), S.lit(42, I64)], I64)
    build_plan = S.hash_agg(S.scan([I64]), [], [S.bloom_filter_agg(xx, items, bits)], S.PARTIAL)
    build_t = table([torch.randint(0, 1 << 40, (a.build_rows,), dtype=torch.int64, device="cuda")], ["k"])
    # the probe side: keys of [0, 2 · keys); the filter holds the even ones
    keys_t = table([torch.arange(0, 2 * a.keys, 2, dtype=torch.int64, device="cuda")], ["k"])
    _, _, _, out = run_once(native, S.hash_agg(S.scan([I64]), [], [S.bloom_filter_agg(xx, a.keys, bits)], S.PARTIAL).encode(), keys_t, 1)
    filt = out[0].column(0).to_pylist()[0]
    probe_t = table([torch.randint(0, 2 * a.keys, (a.probe_rows,), dtype=torch.int64, device="cuda"), torch.randint(-50, 50, (a.probe_rows,), dtype=torch.int32, device="cuda")], ["fk", "o"])
    pred = S.gt(S.col(1, I32), S.lit(0, I32))
    mc = S.bloom_filter_might_contain(S.subquery(0, BIN), xx)

    def count(p):
        return S.hash_agg(S.filter_(S.scan([I64, I32]), p), [], [S.count(S.col(0, I64))], S.PARTIAL)
    # the two ways bloom_put_kernel sets bits, side by side: 2^16 bits is the largest filter built per block in LDS, 2^16 + 64 the smallest built in global memory
    small_t = table([torch.randint(0, 1 << 40, (10_000,), dtype=torch.int64, device="cuda")], ["k"])
    ab = {}
    for label, b in (("2^16 bits, LDS", 1 << 16), ("2^16 + 64 bits, global", (1 << 16) + 64)):
        p = S.hash_agg(S.scan([I64]), [], [S.bloom_filter_agg(xx, 7571, b)], S.PARTIAL)      # six hash functions
        ab[f"build: {label}, {a.build_rows} rows"] = (p, build_t, None)
        ab[f"build: {label}, 10000 rows"] = (p, small_t, None)
    plans = {"build: bloom_filter_agg Partial": (build_plan, build_t, None), **ab, "probe: pred alone": (count(pred), probe_t, None),
             "probe: pred AND might_contain": (count(S.and_(pred, mc)), probe_t, {0: filt})}
    results = {}
    for rep in range(a.reps + 1):
        for name, (plan, t, sub) in plans.items():
            k_ms, w_ms, launches, out = run_once(native, plan.encode(), t, 1, sub)
            r = results.setdefault(name, {"plan": name, "rows_in": t.num_rows, "timed_launches": launches, "kernel_ms_by_rep": [], "task_ms_by_rep": []})
            r["result"] = out[0].column(0).to_pylist()[0] if name.startswith("probe") else len(out[0].column(0).to_pylist()[0])
            if rep:      # (the first turn warms the code-object cache and the allocator)
                r["kernel_ms_by_rep"].append(round(k_ms, 3))
                r["task_ms_by_rep"].append(round(w_ms, 3))
    for r in results.values():
        r["kernel_ms"], r["task_ms"] = min(r["kernel_ms_by_rep"]), min(r["task_ms_by_rep"])
        r["kernel_ms_spread"] = round(max(r["kernel_ms_by_rep"]) - min(r["kernel_ms_by_rep"]), 3)
        print(json.dumps(r), flush=True)
    ratio = {"filter_bits": bits, "filter_keys": a.keys,
             "probe_with_might_contain_over_pred_alone_kernel_ms": round(results["probe: pred AND might_contain"]["kernel_ms"] / results["probe: pred alone"]["kernel_ms"], 3)}
    print(json.dumps(ratio), flush=True)
    if a.out:      # the command that produced the numbers (where they were written is not part of it)
        cmd = ["python", "tools/bloom_bench.py", "--build-rows", str(a.build_rows), "--probe-rows", str(a.probe_rows), "--keys", str(a.keys), "--reps", str(a.reps)]
        with open(a.out, "w") as f:
            json.dump({"command": " ".join(cmd), "results": list(results.values()), "ratio": ratio}, f, indent=1)


if __name__ == "__main__":
    main()
