#!/usr/bin/env python3
"""What m['k'] costs on the MI355X: one Projection over a host-resident map column, timed end to end through the C ABI (upload, fused kernel, export — the wall
clock around a call that ends with the result on the host), beside the Projection that only passes size(m) through over the same table; the difference is
the entry search's share (device/map_fn.hpp: one lane per row walks its map's entries).  Legs: `size` (the baseline), `lookup` (m[<literal>] → Int64), for
maps with Int64 keys and for maps with Utf8 keys ("key_0007": eight bytes, compared against a literal).  Two shapes: --shape short: 1 M maps of 0 to 8 entries,
keys from a domain of 16, the wanted key present in about a quarter of the maps; --shape long: 2 000 maps of 1 500 entries, the wanted key the LAST entry, so
every lane walks its whole map.  Best, median and max of --reps after one discarded warm-up round, the legs alternating in an order that rotates from round
to round.  Kernel times are not taken here (k_emit is the fused kernel of every leg).  One JSON line per shape and key type."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(shape, utf8, seed=5):
    """→ (table with one map column, the wanted key)"""
    import numpy as np
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    if shape == "short":
        lens = rng.integers(0, 9, 1_000_000)
        domain = 16
    else:
        lens = np.full(2_000, 1_500)
        domain = 1_500
    offs = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=offs[1:])
    total = int(offs[-1])
    row = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(total) - offs[:-1][row]
    start = rng.integers(0, domain, len(lens)) if shape == "short" else np.zeros(len(lens), dtype=np.int64)
    keys = (start[row] + pos) % domain      # distinct inside a map
    wanted = 7 if shape == "short" else domain - 1
    vals = rng.integers(-1000, 1000, total).astype(np.int64)
    if utf8:
        names = np.char.add("key_", np.char.zfill(np.arange(domain).astype(str), 4))
        karr = pa.array(names, pa.utf8()).take(pa.array(keys))
        wanted = "key_%04d" % wanted
    else:
        karr = pa.array(keys.astype(np.int64))
    return pa.table({"m": pa.MapArray.from_arrays(pa.array(offs), karr, pa.array(vals))}), wanted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shape", choices=["short", "long", "both"], default="both")
    a = ap.parse_args()
    from datafusion_comet_amd import native, serde as S
    for shape in (["short", "long"] if a.shape == "both" else [a.shape]):
        for utf8 in (False, True):
            t, wanted = table(shape, utf8)
            kt = S.T_STRING if utf8 else S.T_INT64
            mt = S.map_type(kt, S.T_INT64, True)
            m = S.col(0, mt)
            legs = {"size": S.project(S.scan([mt]), [S.scalar_func("size", [m], S.T_INT32)]), "lookup": S.project(S.scan([mt]), [S.map_extract(m, S.lit(wanted, kt))])}
            times = {k: [] for k in legs}
            hits = None
            for rep in range(a.reps + 1):      # (the first round warms every leg up: code objects, pools)
                order = list(legs.items())
                order = order[rep % len(order):] + order[:rep % len(order)]
                for k, plan in order:
                    t0 = time.perf_counter()
                    out = native.execute_to_table([native.HostInput.from_table(t, 1 << 22)], 1, plan.encode(), batch_size=0)
                    dt = time.perf_counter() - t0
                    assert sum(b.num_rows for b in out) == t.num_rows
                    if k == "lookup" and hits is None:
                        hits = sum(b.num_rows - b.column(0).null_count for b in out)
                    if rep:
                        times[k].append(dt * 1e3)
            res = {"shape": shape, "keys": "utf8" if utf8 else "int64", "maps": t.num_rows, "entries": len(t.column(0).combine_chunks().keys), "hits": hits, "reps": a.reps}
            for k, v in times.items():
                res[k + "_ms"] = {"best": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}
            res["lookup_minus_size_median_ms"] = round(res["lookup_ms"]["median"] - res["size_ms"]["median"], 3)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
