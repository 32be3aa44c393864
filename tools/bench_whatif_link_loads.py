#!/usr/bin/env python
"""Link-cost what-if loads of the all-host-pairs demand:
sdnr_whatif_ecmp_link_loads over 64 scenarios in one call -- half raise one
aggregation-to-core link by 1, half take one cable down -- and the cost tuner
over it, against what the tree offered before:

 (a) kernel against kernel on the cable-down half: whatif_ecmp_loads_kernel and
     failure_ecmp_loads_kernel (sdnr_failure_ecmp_link_loads) on the same 32
     scenarios, same process, alternating, the SDNR_TIMING event pair;
 (b) the engine call per scenario with the load planes copied back
     (loads=True) and with the peaks alone (loads=False), and the drop-in
     all_pairs_cost_change_link_loads, host clock around work that ends in a
     device synchronise;
 (c) the public round trip of the parent API per cost scenario: set_link_cost,
     all_pairs_least_cost_ecmp_link_loads, set_link_cost back, wall time;
 (d) one all_pairs_tune_link_costs run: rounds, scenarios evaluated, wall
     time, peak before and after.

One GPU, the k=48 fat-tree with one core group at cost 2 (as
bench_failure_link_loads.py), all 1,152 host-bearing destination rows, the
demand of every ordered switch pair.  Sampled (scenario, row) items are
compared with engine.whatif_ecmp_link_loads_host (rtol 1e-9) first.  Every time
is the median of --reps.  No time is a pass condition.  One JSON line goes to
--out.

    python tools/bench_whatif_link_loads.py --out profiles/whatif_link_loads_k48.jsonl
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sdnmpi_amd import engine as EN          # noqa: E402
from sdnmpi_amd import topologies as T       # noqa: E402
from sdnmpi_amd.util.topology_db import TopologyDB   # noqa: E402
from bench_failure_link_loads import (K, NSCEN, RTOL, SAMPLE_ROWS, SAMPLE_SCEN,   # noqa: E402
                                      cable_scenarios, cost_sets, demand, med, note)

INF = EN.COST_INF


def scenarios(csr, cost, hosts):
    """NSCEN scenarios as (edges, costs): the aggregation-core half of
    cable_scenarios with its upward link raised by 1, then the same cables
    taken down (both directions).  Returns (scenarios, failed edge lists of
    the second half)."""
    cables = cable_scenarios(csr, hosts)[NSCEN // 2:]      # aggregation - core
    col = np.asarray(csr.col)
    esrc = np.repeat(np.arange(int(csr.V)), np.diff(csr.row_ptr))
    up = [e if esrc[e] > col[e] else f for e, f in cables]  # (the cores are the low ids)
    raised = [([e], [int(cost[e]) + 1]) for e in up]
    return raised + [(c, [INF, INF]) for c in cables], cables


def bench(fabric, name, cost, reps, out):
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    E = int(csr.E)
    dsts, rows, srcs, w = demand(fabric, csr)
    scen, cables = scenarios(csr, cost, dsts)
    half = NSCEN // 2
    rec = {"fabric": "fat_tree_k%d" % K, "costs": name, "V": int(csr.V), "E": E,
           "rows": int(dsts.shape[0]), "switch_pairs": int(rows.shape[0]), "scenarios": NSCEN,
           "raised": half, "cable_down": half, "reps": reps}

    eng = EN.RouteEngine(0)
    sel = np.isin(rows, np.asarray(SAMPLE_ROWS))
    sub = [scen[i] for i in SAMPLE_SCEN]
    for split in EN.SPLITS:
        want = EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows[sel], srcs[sel], w[sel], sub,
                                              split)
        part = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows[sel], srcs[sel], w[sel], sub, split)
        z = want[0] == 0
        assert (part[0][z] == 0).all() and \
            np.allclose(part[0][~z], want[0][~z], rtol=RTOL, atol=0), split
        assert np.array_equal(part[1], want[1]) and np.array_equal(part[2], want[2])
        assert np.allclose(part[3], want[3], rtol=RTOL, atol=0)
        rec["max_rel_err_vs_host_sampled_items_" + split] = \
            float(np.max(np.abs(part[0][~z] - want[0][~z]) / want[0][~z]))
    rec["sampled_items"] = len(SAMPLE_SCEN) * len(SAMPLE_ROWS)

    # -- (a) kernel against kernel on the cable-down half, alternating --------
    for split in EN.SPLITS:
        eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, scen[half:], split)   # warm-up
        eng.failure_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, cables, split)
        new, old = [], []
        for _ in range(reps):
            got = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, scen[half:], split,
                                             timing=True)
            new.append(eng.ctx.last_kernel_ms())
            rec["kernel"] = eng.ctx.last_kernel()
            ref = eng.failure_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, cables, split,
                                              timing=True)
            old.append(eng.ctx.last_kernel_ms())
            rec["failure_kernel"] = eng.ctx.last_kernel()
        z = ref[0] == 0
        assert (got[0][z] == 0).all() and np.allclose(got[0][~z], ref[0][~z], rtol=RTOL, atol=0)
        assert not got[1].any() and got[2].all()
        rec["a_whatif_kernel_ms_" + split] = [round(x, 4) for x in new]
        rec["a_failure_kernel_ms_" + split] = [round(x, 4) for x in old]
        rec["a_whatif_kernel_median_ms_per_scenario_" + split] = round(med(new) / half, 5)
        rec["a_failure_kernel_median_ms_per_scenario_" + split] = round(med(old) / half, 5)
        rec["a_kernel_ratio_whatif_over_failure_" + split] = round(med(new) / med(old), 4)
        note(split, "(a) kernel ms whatif / failure", med(new), med(old))

    # -- (b) the engine call with the planes and with the peaks alone ---------
    for split in EN.SPLITS:
        walls = {True: [], False: []}
        kms = []
        for loads in (True, False):
            eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, scen, split, loads=loads,
                                       reach=loads)
            for _ in range(reps):
                t = time.perf_counter()
                got = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, scen, split,
                                                 loads=loads, reach=loads, timing=True)
                walls[loads].append((time.perf_counter() - t) * 1e3)
                if loads:
                    kms.append(eng.ctx.last_kernel_ms())
                    full = got
        assert np.allclose(got[3], full[3], rtol=RTOL, atol=0)
        rec["b_kernel_median_ms_per_scenario_64_" + split] = round(med(kms) / NSCEN, 5)
        rec["b_engine_wall_ms_loads_" + split] = [round(x, 2) for x in walls[True]]
        rec["b_engine_wall_ms_peaks_only_" + split] = [round(x, 2) for x in walls[False]]
        rec["b_engine_wall_median_ms_per_scenario_loads_" + split] = \
            round(med(walls[True]) / NSCEN, 4)
        rec["b_engine_wall_median_ms_per_scenario_peaks_only_" + split] = \
            round(med(walls[False]) / NSCEN, 4)
        rec["b_wall_ratio_peaks_only_over_loads_" + split] = \
            round(med(walls[False]) / med(walls[True]), 4)
        note(split, "(b) engine wall ms loads / peaks only", med(walls[True]), med(walls[False]))
    eng.close()

    # -- the drop-in, and (c) the public round trip of the parent API ---------
    db = fabric.populate(TopologyDB())
    dp = csr.dpids
    esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    link = lambda e: (int(dp[esrc[e]]), int(dp[csr.col[e]]))   # noqa: E731
    costed = np.nonzero(cost != 1)[0]
    if costed.size:
        db.set_link_costs({link(e): int(cost[e]) for e in costed.tolist()})
    changes = [{link(e): (None if c == INF else int(c)) for e, c in zip(es, cs)}
               for es, cs in scen]
    for split in EN.SPLITS:
        base = db.all_pairs_least_cost_ecmp_link_loads(split)     # warm: tables resident
        walls = []
        for _ in range(reps):
            t = time.perf_counter()
            got = db.all_pairs_cost_change_link_loads(changes, split)
            walls.append((time.perf_counter() - t) * 1e3)
        assert not got.lost.any() and np.allclose(got.base.load, base.load, rtol=RTOL, atol=0)
        rec["b_dropin_wall_ms_" + split] = [round(x, 2) for x in walls]
        rec["b_dropin_wall_median_ms_per_scenario_" + split] = round(med(walls) / NSCEN, 3)
        note(split, "(b) drop-in wall ms", med(walls))
        loop = []
        step = max(1, half // reps)
        for k in range(0, step * reps, step):                     # raised links only
            (a, b), c = next(iter(changes[k].items()))
            t = time.perf_counter()
            db.set_link_cost(a, b, c)
            one = db.all_pairs_least_cost_ecmp_link_loads(split)
            db.set_link_cost(a, b, int(cost[scen[k][0][0]]))
            loop.append((time.perf_counter() - t) * 1e3)
            z = one.load == 0
            assert (got.load[k][z] == 0).all() and \
                np.allclose(got.load[k][~z], one.load[~z], rtol=RTOL, atol=0)
        db.all_pairs_least_cost_ecmp_link_loads(split)            # back under the costs as they were
        rec["c_round_trip_wall_ms_" + split] = [round(x, 2) for x in loop]
        rec["c_round_trip_wall_median_ms_per_scenario_" + split] = med(loop)
        rec["c_wall_ratio_dropin_over_round_trip_" + split] = \
            round(rec["b_dropin_wall_median_ms_per_scenario_" + split] / med(loop), 4)
        rec["c_wall_ratio_peaks_only_over_round_trip_" + split] = \
            round(rec["b_engine_wall_median_ms_per_scenario_peaks_only_" + split] / med(loop), 5)
        note(split, "(c) round trip wall ms per scenario", med(loop))

    # -- (d) the tuner on the all-pairs demand ---------------------------------
    seen = []
    inner = db.engine.whatif_ecmp_link_loads

    def counted(*a, **kw):
        seen.append(len(a[6]))
        return inner(*a, **kw)
    db.engine.whatif_ecmp_link_loads = counted
    t = time.perf_counter()
    tuned = db.all_pairs_tune_link_costs()
    wall = (time.perf_counter() - t) * 1e3
    del db.engine.whatif_ecmp_link_loads
    rec["d_tuner"] = {"accepted_steps": len(tuned.history), "engine_calls": len(seen),
                      "scenarios_evaluated": int(sum(seen)), "wall_ms": round(wall, 1),
                      "wall_ms_per_scenario": round(wall / max(1, sum(seen)), 3),
                      "peak_before": tuned.peak_before, "peak_after": tuned.peak_after,
                      "history": [[list(l), c, p] for l, c, p in tuned.history]}
    note("(d) tuner", rec["d_tuner"])
    db.engine.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "whatif_link_loads_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    fabric = T.fat_tree(K)
    name, cost = cost_sets(fabric.csr())[1]
    bench(fabric, name, cost, a.reps, a.out)


if __name__ == "__main__":
    main()
