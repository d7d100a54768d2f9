#!/usr/bin/env python3
"""What sort_array / array_distinct cost on the MI355X: one Projection over a host-resident list<bigint> column, timed end to end through the C ABI (upload, derived
column, emit, export — the wall clock around a call that ends with the result on the host), beside the same Projection that only passes the column through; the
difference is the derived column's share.  Each function runs under both forced routes (COMET_LIST_FN_TIER=rank: one lane per element ranks it against its list;
sort: the engine's radix sort over (list row, element)).  Two shapes: --shape short: 1 M lists of 0 to 8 elements; --shape long: 2 000 lists of 1 500 elements.  Best and
median of --reps, the legs alternating in an order that rotates from round to round.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/list_fn_bench.py --reps 1`
(list_rank_kernel is the new kernel).  One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(shape, seed=5):
    import numpy as np
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    if shape == "short":
        lens = rng.integers(0, 9, 1_000_000)
    else:
        lens = np.full(2_000, 1_500)
    offs = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=offs[1:])
    vals = rng.integers(-1000, 1000, int(offs[-1])).astype(np.int64)
    return pa.table({"l": pa.ListArray.from_arrays(pa.array(offs), pa.array(vals))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", choices=["short", "long", "both"], default="both")
    a = ap.parse_args()
    from datafusion_comet_amd import native, serde as S
    LT = S.list_type(S.T_INT64, True)
    l = S.col(0, LT)
    plans = {"pass": S.project(S.scan([LT]), [l]), "sort": S.project(S.scan([LT]), [S.sort_array(l)]), "distinct": S.project(S.scan([LT]), [S.array_distinct(l)])}
    # (leg, plan, COMET_LIST_FN_TIER): each function under both forced routes, and as the engine chooses by itself
    legs = {"pass": ("pass", None), "sort_rank": ("sort", "rank"), "sort_radix": ("sort", "sort"), "distinct_rank": ("distinct", "rank"), "distinct_radix": ("distinct", "sort"),
            "sort_default": ("sort", None), "distinct_default": ("distinct", None)}
    for shape in (["short", "long"] if a.shape == "both" else [a.shape]):
        t = table(shape)
        times = {k: [] for k in legs}
        for rep in range(a.reps + 1):      # (the first round warms every leg up: code objects, pools)
            order = list(legs.items())
            order = order[rep % len(order):] + order[:rep % len(order)]      # (rotated: no leg keeps the same neighbours in every round)
            for k, (pk, tier) in order:
                plan = plans[pk]
                os.environ.pop("COMET_LIST_FN_TIER", None)
                if tier:
                    os.environ["COMET_LIST_FN_TIER"] = tier
                t0 = time.perf_counter()
                out = native.execute_to_table([native.HostInput.from_table(t, 1 << 22)], 1, plan.encode(), batch_size=0)
                dt = time.perf_counter() - t0
                assert sum(b.num_rows for b in out) == t.num_rows
                if rep:
                    times[k].append(dt * 1e3)
        res = {"shape": shape, "lists": t.num_rows, "elements": len(t.column(0).combine_chunks().values), "reps": a.reps}
        for k, v in times.items():
            res[k + "_ms"] = {"best": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
