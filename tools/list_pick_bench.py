#!/usr/bin/env python3
"""What array_remove / array_compact / slice / reverse of an array / array_join cost on the MI355X: one Projection over a host-resident list<bigint> column a (one
element in ten NULL) and a list<string> column s of the same lengths, timed end to end through the C ABI (upload, derived column, emit, export — the wall clock
around a call that ends with the result on the host), beside the same Projection that only passes a through (`pass`) and beside array_distinct(a) (`distinct`:
existing code with the same tail and a ranking in front of it, the yardstick).  remove, compact, slice and reverse read a; join reads s and exports one string per
row.  Two shapes: --shape short: 1 M rows of 0 to 8 elements; --shape long: 2 000 rows of 1 500 elements.  Best and median of --reps, the legs alternating in an
order that rotates from round to round, the first round discarded.  Upload and export dominate these wall clocks: only differences between the legs of one shape
mean anything.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/list_pick_bench.py --reps 3` (list_pick_kernel,
list_reverse_kernel and the list_join_* kernels are the new ones).  One JSON line per shape."""
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
    import pyarrow.compute as pc
    rng = np.random.default_rng(seed)
    if shape == "short":
        lens = rng.integers(0, 9, 1_000_000)
        span = 8
    else:
        lens = np.full(2_000, 1_500)
        span = 1000
    offs = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=offs[1:])
    n = int(offs[-1])
    vals = rng.integers(-span, span, n).astype(np.int64)
    nulls = rng.random(n) < 0.1
    words = pa.array(["v%d" % v for v in range(-span, span)], pa.utf8())
    strs = pc.if_else(pa.array(~nulls), words.take(pa.array(vals + span)), pa.scalar(None, pa.utf8()))
    return pa.table({"a": pa.ListArray.from_arrays(pa.array(offs), pa.array(vals, mask=nulls)), "s": pa.ListArray.from_arrays(pa.array(offs), strs)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", choices=["short", "long", "both"], default="both")
    a = ap.parse_args()
    from datafusion_comet_amd import native, serde as S
    LT, LS = S.list_type(S.T_INT64, True), S.list_type(S.T_STRING, True)
    x, s = S.col(0, LT), S.col(1, LS)
    src = S.scan([LT, LS])
    legs = {"pass": S.project(src, [x]), "distinct": S.project(src, [S.array_distinct(x)]), "remove": S.project(src, [S.array_remove(x, S.lit(3, S.T_INT64))]),
            "compact": S.project(src, [S.array_compact(x)]), "slice": S.project(src, [S.array_slice(x, 2, 3)]), "reverse": S.project(src, [S.array_reverse(x)]),
            "join": S.project(src, [S.array_join(s, ",")])}
    os.environ.pop("COMET_LIST_FN_TIER", None)
    for shape in (["short", "long"] if a.shape == "both" else [a.shape]):
        t = table(shape)
        times = {k: [] for k in legs}
        for rep in range(a.reps + 1):      # (the first round warms every leg up: code objects, pools)
            order = list(legs.items())
            order = order[rep % len(order):] + order[:rep % len(order)]      # (rotated: no leg keeps the same neighbours in every round)
            for k, plan in order:
                t0 = time.perf_counter()
                out = native.execute_to_table([native.HostInput.from_table(t, 1 << 22)], 1, plan.encode(), batch_size=0)
                dt = time.perf_counter() - t0
                assert sum(b.num_rows for b in out) == t.num_rows
                if rep:
                    times[k].append(dt * 1e3)
        res = {"shape": shape, "rows": t.num_rows, "elements": len(t.column(0).combine_chunks().values), "reps": a.reps}
        for k, v in times.items():
            res[k + "_ms"] = {"best": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
