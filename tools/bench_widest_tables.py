#!/usr/bin/env python
"""Least-loaded tables of every host-bearing destination: sdnr_widest_tables
(unit utilisation, and seeded utilisation in [0, 1000)) against
sdnr_cost_tables on the same rows -- the yardstick: both walk the same CSR in
the same sweep shape -- and admit_flows end to end for the all-host-pairs
demand at the default slicing (one round per destination switch).

One GPU.  A sample of the rows is compared with engine.widest_tables_host
before anything is timed, and the unit-utilisation next hops with
sdnr_cost_tables'.  The kernel time is the SDNR_TIMING event pair; the call
time is the host clock around a call that ends in a device synchronise (tables
stay on the device).  Repetitions alternate the sides.  No time is a pass
condition.  One JSON line per fabric goes to --out.

    python tools/bench_widest_tables.py --out profiles/widest_tables_k48.jsonl
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
from sdnmpi_amd.util.topology_db import TopologyDB   # noqa: E402

FABRICS = {"fat_tree_k48": lambda: T.fat_tree(48),
           "dragonfly_a16_h8_p8": lambda: T.dragonfly(16, 8, 8)}
CHECK_ROWS = 48


def stats(rec, key, ts):
    rec[key + "_ms"] = [round(x, 4) for x in ts]
    rec[key + "_median_ms"] = round(float(np.median(ts)), 4)


def bench_tables(name, fabric, reps, rec):
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    eng = EN.RouteEngine(0)
    hv, _ = fabric.host_table()
    dsts = np.unique(hv).astype(np.int32)
    D, V, E = int(dsts.shape[0]), int(csr.V), int(csr.E)
    rec.update({"fabric": name, "V": V, "E": E, "rows": D, "reps": reps})
    ones = np.ones(E, np.uint32)
    utils = {"unit": np.ones(E, np.uint32),
             "seeded": np.random.default_rng(48).integers(0, 1000, E).astype(np.uint32)}
    pc, nh0, nhp0 = eng.cost_tables(ex, ones, dsts)      # warm-up, and the rows both sides read
    rec["cost_kernel"] = eng.ctx.last_kernel()
    sample = np.random.default_rng(7).choice(D, min(D, CHECK_ROWS), replace=False)
    pc_host = EN._host(pc)[sample]
    for key, util in utils.items():
        bott, nh, nhp = eng.widest_tables(ex, ones, pc, util, dsts)
        rec["kernel"] = eng.ctx.last_kernel()
        want = EN.widest_tables_host(csr, ones, pc_host, util, dsts[sample])
        got = [EN._host(t)[sample] for t in (bott, nh, nhp)]
        assert np.array_equal(got[0].view(np.uint32), want[0])
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        if key == "unit":
            assert bool((nh == nh0).all()) and bool((nhp == nhp0).all())
            rec["unit_next_hops_equal_cost_tables"] = True
        else:
            rec["seeded_next_hops_differing"] = int((nh != nh0).sum().item())
    rec["sample_rows_equal_host"] = int(sample.shape[0])
    k_cost, k_wide = [], {k: [] for k in utils}
    c_cost, c_wide = [], {k: [] for k in utils}
    for _ in range(reps):
        t = time.perf_counter()
        eng.cost_tables(ex, ones, dsts, timing=True)
        c_cost.append((time.perf_counter() - t) * 1e3)
        k_cost.append(eng.ctx.last_kernel_ms())
        for key, util in utils.items():
            t = time.perf_counter()
            eng.widest_tables(ex, ones, pc, util, dsts, timing=True)
            c_wide[key].append((time.perf_counter() - t) * 1e3)
            k_wide[key].append(eng.ctx.last_kernel_ms())
    stats(rec, "cost_tables_kernel", k_cost)
    stats(rec, "cost_tables_call", c_cost)
    for key in utils:
        stats(rec, "widest_%s_kernel" % key, k_wide[key])
        stats(rec, "widest_%s_call" % key, c_wide[key])
        rec["widest_%s_kernel_over_cost_tables_kernel" % key] = round(
            rec["widest_%s_kernel_median_ms" % key] / rec["cost_tables_kernel_median_ms"], 2)
    eng.close()


def bench_admission(fabric, rec):
    """admit_flows' rounds over the all-host-pairs demand as switch pairs
    (hosts(s) * hosts(d) from s to d), default slicing."""
    db = fabric.populate(TopologyDB())
    try:
        ex = db.graph()
        sv, dv, w, _, _ = db._all_pairs_demand(ex)
        before, _ = db._switch_pair_cost_loads(ex, sv, dv, w)     # also fills the least-cost memo
        slices = db._admission_slices(dv, None, 0, None)
        db._admit(ex, sv[:1], dv[:1], w[:1], [np.arange(1)], None)   # warm-up: one round
        t = time.perf_counter()
        load, reach = db._admit(ex, sv, dv, w, slices, None)
        dt = time.perf_counter() - t
        assert bool(reach.all())
        cost = db._cost_vector(ex)
        assert int((load * cost).sum()) == int((before * cost).sum())
        rec["admit_pairs"] = int(sv.shape[0])
        rec["admit_demand"] = int(w.sum())
        rec["admit_rounds"] = len(slices)
        rec["admit_peak_before"] = db._peak(ex, before, None)[0]
        rec["admit_peak_after"] = db._peak(ex, load, None)[0]
        rec["admit_total_ms"] = round(dt * 1e3, 1)
        rec["admit_ms_per_round"] = round(dt * 1e3 / max(1, len(slices)), 3)
        rec["admit_total_load_equal"] = True
        db.engine.ctx.synchronize()
    finally:
        db.engine.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "widest_tables_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="fat_tree_k48", help="comma-separated fabric names")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 alternated repetitions")
    only = set(x for x in a.only.split(",") if x)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    for name in FABRICS:
        if only and name not in only:
            continue
        fabric = FABRICS[name]()
        rec = {}
        bench_tables(name, fabric, a.reps, rec)
        bench_admission(fabric, rec)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
