#!/usr/bin/env python3
"""What regexp_replace costs as a derived Utf8 column: regexp_replace(s, '[^0-9]', '') and regexp_replace(s, ',', ';') against split(s, ',') over the same
HBM-resident Utf8 column (20 M short strings of the kind tests/test_split_gpu.py uses), one GPU, one Projection each.  split is the yardstick because it runs
the same matcher iteration per row (rx_for_matches, twice) and writes 16-byte views where regexp_replace writes bytes.  Prints per case the task time (wall
clock around a device synchronise) of every round — the cases alternate within a round, so the spread between rounds is visible beside the difference
between cases.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/regexp_replace_bench.py --rounds 1`
(replace_len_kernel / replace_write_kernel against split_count_kernel / split_write_kernel)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORDS = ["", "a,b,c", "a,b,c,,", ",,,", "x", "one, two ,three", "k1=v1;k2=v2;;k3", "日本,語テ,キスト", "naïve  café   au lait", "foo123bar456baz", "2024-06-30", "a" * 50 + "," + "b" * 60,
         " leading and trailing "]


def run_once(native, plan_bytes, table, ncols):
    import torch
    inp = native.DeviceInput(table)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = native.Native.createPlan([inp], plan_bytes, b"", 1, 0, 0)
    try:
        out = native.Native.executePlanDevice(h, ncols)
        rows = out.num_rows if out is not None else 0
        del out
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, rows
    finally:
        native.Native.releasePlan(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import datafusion_comet_amd  # noqa: F401 — before torch: the JIT then compiles with the installed ROCm's compiler (see that module)
    import numpy as np
    import pyarrow as pa
    from datafusion_comet_amd import native, serde as S
    rng = np.random.default_rng(41)
    s_arr = pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, len(WORDS), a.rows).astype(np.int32)), pa.array(WORDS, pa.utf8())).cast(pa.utf8())
    nbytes = s_arr.buffers()[2].size
    dt = native.DeviceTable.from_arrow(pa.table({"s": s_arr}), "cuda:0")
    STR = S.T_STRING
    s = S.col(0, STR)
    # (an Int32 of each result is what leaves the chain — size / length —, so that the derived column's kernels are what differs, not the export)
    f, I32 = S.scalar_func, S.T_INT32
    cases = {"size(split(s, ','))": f("size", [f("split", [s, S.lit(",", STR), S.lit(-1, I32)], S.list_type(STR, False))], I32),
             "length(regexp_replace(s, '[^0-9]', ''))": f("length", [S.regexp_replace(s, "[^0-9]", "")], I32),
             "length(regexp_replace(s, ',', ';'))": f("length", [S.regexp_replace(s, ",", ";")], I32)}
    plans = {name: S.project(S.scan([STR]), [e]).encode() for name, e in cases.items()}
    for p in plans.values():
        native.compile_plan(p)
    times = {name: [] for name in plans}
    for rnd in range(a.rounds + 1):      # (round 0 warms every shape up and is not kept)
        for name, p in plans.items():
            ms, rows = run_once(native, p, dt, 1)
            assert rows == a.rows
            if rnd:
                times[name].append(round(ms, 2))
    results = []
    for name, t in times.items():
        r = {"case": name, "rows": a.rows, "input_bytes": nbytes, "task_ms": t, "best_ms": min(t), "worst_ms": max(t)}
        print(json.dumps(r, ensure_ascii=False), flush=True)
        results.append(r)
    if a.out:      # the command that produced the numbers (where they were written is not part of it)
        cmd = ["python", "tools/regexp_replace_bench.py", "--rows", str(a.rows), "--rounds", str(a.rounds)]
        with open(a.out, "w") as f:
            json.dump({"command": " ".join(cmd), "results": results}, f, indent=1, ensure_ascii=False)


if __name__ == "__main__":
    main()
