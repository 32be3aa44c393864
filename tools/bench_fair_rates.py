#!/usr/bin/env python
"""Max-min fair rates of the all-host-pairs demand on the k=48 fat-tree in the
switch-pair form (1,152^2 flows, multiplicity hosts(s) * (hosts(d) - [s == d]),
unit capacities), on the default trees and on the shortest next-hop rows:
sdnr_fair_rates against sdnr_link_loads over the same rows and pairs -- the
yardstick: a round's row kernel does link_loads' subtree sums plus the verdict
of the round before -- and against engine.fair_rates_host.

One GPU.  The device result is compared with fair_rates_host bit for bit before
anything is timed.  The kernel time is the SDNR_TIMING event pair (for
fair_rates: from the first launch to the last, the status read-backs between
the batches included); the call time is the host clock around the engine call
(pair sort, uploads, rounds, results back).  Repetitions alternate the sides.
No time is a pass condition.  One JSON line per route goes to --out.

    python tools/bench_fair_rates.py --out profiles/fair_rates_k48.jsonl
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdn-mpi-router_amd"))

from sdnmpi_amd import engine as EN          # noqa: E402
from sdnmpi_amd import topologies as T       # noqa: E402


def stats(rec, key, ts):
    rec[key + "_ms"] = [round(x, 4) for x in ts]
    rec[key + "_median_ms"] = round(float(np.median(ts)), 4)


def bench_route(eng, fabric, route, reps):
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    hv, _ = fabric.host_table()
    hc = np.bincount(hv, minlength=csr.V).astype(np.int64)
    sw = np.nonzero(hc)[0].astype(np.int32)
    n = int(sw.shape[0])
    rows = np.repeat(np.arange(n), n)
    other = np.tile(sw, n)
    # symmetric demand: row = source, vertex = destination on the default
    # trees; row = destination, vertex = source on the next-hop rows
    mult = (hc[sw[rows]] * (hc[other] - (sw[rows] == other))).astype(np.uint64)
    cap = np.ones(int(csr.E), np.float64)
    if route == "default":
        tree, to_root = eng.dfs_tables(ex, sw)[0], False
    else:
        tree, to_root = eng.shortest_tables(ex, sw)[1], True
    rec = {"fabric": "fat_tree_k48", "route": route, "V": int(csr.V), "E": int(csr.E), "rows": n,
           "flows": int(rows.shape[0]), "demand": int(mult.sum()), "reps": reps}
    got = eng.fair_rates(ex, tree, EN.INT32, rows, other, mult, cap, to_root=to_root)
    rec["kernel"] = eng.ctx.last_kernel()
    rec["launches"] = eng.ctx.last_launches()
    rec["rounds"] = int(got[3].shape[0])
    rec["levels"] = [float(x) for x in got[3]]
    t = time.perf_counter()
    want = EN.fair_rates_host(csr, tree.cpu().numpy(), EN.INT32, rows, other, mult, cap,
                              to_root=to_root)
    rec["host_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(
            g.view(np.uint64) if g.dtype == np.float64 else g,
            w.view(np.uint64) if w.dtype == np.float64 else w)
    rec["equal_host_bit_for_bit"] = True
    eng.link_loads(ex, tree, EN.INT32, rows, other, mult, to_root=to_root)       # warm-up
    rec["link_loads_kernel"] = eng.ctx.last_kernel()
    k_fair, c_fair, k_load, c_load = [], [], [], []
    for _ in range(reps):
        t = time.perf_counter()
        eng.link_loads(ex, tree, EN.INT32, rows, other, mult, to_root=to_root, timing=True)
        c_load.append((time.perf_counter() - t) * 1e3)
        k_load.append(eng.ctx.last_kernel_ms())
        t = time.perf_counter()
        eng.fair_rates(ex, tree, EN.INT32, rows, other, mult, cap, to_root=to_root, timing=True)
        c_fair.append((time.perf_counter() - t) * 1e3)
        k_fair.append(eng.ctx.last_kernel_ms())
    stats(rec, "link_loads_kernel", k_load)
    stats(rec, "link_loads_call", c_load)
    stats(rec, "fair_rates_kernel", k_fair)
    stats(rec, "fair_rates_call", c_fair)
    # the rounds run: rounds + 1 (the closing one) do work, the rest of the
    # batch of 16 return at once
    worked = rec["rounds"] + 1
    rec["fair_rates_kernel_ms_per_round"] = round(rec["fair_rates_kernel_median_ms"] / worked, 4)
    rec["round_over_link_loads_kernel"] = round(
        rec["fair_rates_kernel_ms_per_round"] / rec["link_loads_kernel_median_ms"], 2)
    rec["host_over_fair_rates_call"] = round(rec["host_ms"] / rec["fair_rates_call_median_ms"], 1)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fair_rates_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 alternated repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    fabric = T.fat_tree(48)
    eng = EN.RouteEngine(0)
    try:
        for route in ("default", "shortest"):
            line = json.dumps(bench_route(eng, fabric, route, a.reps))
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
