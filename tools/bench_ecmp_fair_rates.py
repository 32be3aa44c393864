#!/usr/bin/env python
"""Max-min fair rates over ECMP of the all-host-pairs demand on the k=48
fat-tree in the switch-pair form (1,152^2 flows, multiplicity hosts(s) *
(hosts(d) - [s == d]), unit capacities, unit link costs), under both splits:
sdnr_ecmp_fair_rates against one sdnr_cost_ecmp_link_loads pass of the same
demand over the same rows -- the yardstick: a round's row kernel does that
kernel's ordering sweeps and its push, plus the verdict of the round before --
and against engine.ecmp_fair_rates_host.

One GPU.  The device result is compared with ecmp_fair_rates_host (equal
rounds, round and bottleneck; rates, levels and carried rates within the tests'
tolerance) before anything is timed.  The kernel time is the SDNR_TIMING event
pair (for the fair rates: from the first launch to the last, the status
read-backs between the batches included); the call time is the host clock
around the engine call (pair sort, uploads, rounds, results back).  Repetitions
alternate the sides.  No time is a pass condition.  One JSON line per split
goes to --out.

    python tools/bench_ecmp_fair_rates.py --out profiles/ecmp_fair_rates_k48.jsonl
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

TOL = 16 * 3.6e-15                           # tests/test_ecmp_fair_rates.py


def stats(rec, key, ts):
    rec[key + "_ms"] = [round(x, 4) for x in ts]
    rec[key + "_median_ms"] = round(float(np.median(ts)), 4)


def bench_split(eng, fabric, split, reps):
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    hv, _ = fabric.host_table()
    hc = np.bincount(hv, minlength=csr.V).astype(np.int64)
    sw = np.nonzero(hc)[0].astype(np.int32)
    n = int(sw.shape[0])
    rows = np.repeat(np.arange(n), n)                     # row = destination
    srcs = np.tile(sw, n)
    mult = (hc[srcs] * (hc[sw[rows]] - (sw[rows] == srcs))).astype(np.uint64)
    cost = np.ones(int(csr.E), np.uint32)
    cap = np.ones(int(csr.E), np.float64)
    pc = eng.cost_tables(ex, cost, sw)[0]
    rec = {"fabric": "fat_tree_k48", "split": split, "V": int(csr.V), "E": int(csr.E), "rows": n,
           "flows": int(rows.shape[0]), "demand": int(mult.sum()), "reps": reps}
    got = eng.ecmp_fair_rates(ex, cost, pc, rows, srcs, mult, cap, None, split)
    rec["kernel"] = eng.ctx.last_kernel()
    rec["launches"] = eng.ctx.last_launches()
    rec["rounds"] = int(got[3].shape[0])
    rec["levels"] = [float(x) for x in got[3]]
    rec["links_saturated"] = int((got[4] >= cap * (1 - 2.0 ** -30)).sum())
    t = time.perf_counter()
    want = EN.ecmp_fair_rates_host(csr, cost, pc.cpu().numpy(), rows, srcs, mult, cap, None, split)
    rec["host_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    worst = 0.0
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        if g.dtype != np.float64:
            assert np.array_equal(g, w)
            continue
        assert np.allclose(g, w, rtol=TOL, atol=0)
        ok = np.isfinite(w) & (w != 0)
        if ok.any():
            worst = max(worst, float(np.max(np.abs(g[ok] - w[ok]) / w[ok])))
    rec["max_rel_dev_vs_host"] = worst
    eng.cost_ecmp_link_loads(ex, cost, pc, rows, srcs, mult, split)                # warm-up
    rec["loads_kernel"] = eng.ctx.last_kernel()
    k_fair, c_fair, k_load, c_load = [], [], [], []
    for _ in range(reps):
        t = time.perf_counter()
        eng.cost_ecmp_link_loads(ex, cost, pc, rows, srcs, mult, split, timing=True)
        c_load.append((time.perf_counter() - t) * 1e3)
        k_load.append(eng.ctx.last_kernel_ms())
        t = time.perf_counter()
        eng.ecmp_fair_rates(ex, cost, pc, rows, srcs, mult, cap, None, split, timing=True)
        c_fair.append((time.perf_counter() - t) * 1e3)
        k_fair.append(eng.ctx.last_kernel_ms())
    stats(rec, "loads_kernel", k_load)
    stats(rec, "loads_call", c_load)
    stats(rec, "fair_rates_kernel", k_fair)
    stats(rec, "fair_rates_call", c_fair)
    # the rounds run: rounds + 1 (the closing one) do work, the rest of the
    # batch of 16 return at once
    worked = rec["rounds"] + 1
    rec["fair_rates_kernel_ms_per_round"] = round(rec["fair_rates_kernel_median_ms"] / worked, 4)
    rec["round_over_loads_kernel"] = round(
        rec["fair_rates_kernel_ms_per_round"] / rec["loads_kernel_median_ms"], 2)
    rec["host_over_fair_rates_call"] = round(rec["host_ms"] / rec["fair_rates_call_median_ms"], 1)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecmp_fair_rates_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 alternated repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    fabric = T.fat_tree(48)
    eng = EN.RouteEngine(0)
    try:
        for split in EN.SPLITS:
            line = json.dumps(bench_split(eng, fabric, split, a.reps))
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
