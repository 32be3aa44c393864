#!/usr/bin/env python
"""Link-failure what-if loads of the all-host-pairs demand:
sdnr_failure_ecmp_link_loads (both splits) over 64 single-cable scenarios in
one call, against its numpy restatement and -- the yardsticks -- against what
the tree offered before it: per scenario, sdnr_cost_tables plus
sdnr_cost_ecmp_link_loads on a context that really has the scenario's graph
uploaded (kernel times), and a TopologyDB round trip delete_link /
all_pairs_least_cost_ecmp_link_loads / add_link (wall time).

One GPU, the k=48 fat-tree, all 1,152 host-bearing destination rows, the demand
of every ordered switch pair.  The scenarios are 64 single cables, both
directions each: 32 edge-aggregation and 32 aggregation-core cables spread over
the pods and positions, so all three switch tiers lose links.  Two cost sets:
unit costs and one aggregation-to-core tier at cost 2 (as
bench_cost_ecmp_link_loads.py).  Per cost set and split the call is warmed up,
sampled (scenario, row) items are compared with
engine.failure_ecmp_link_loads_host (rtol 1e-9), the lost demand is checked to
be 0 in every scenario (no single cable cuts this fabric), then the kernel (the
SDNR_TIMING event pair) and the whole drop-in call (host clock around work that
ends in a device synchronise) are timed, each the median of --reps.  No time is
a pass condition.  One JSON line per cost set goes to --out.

    python tools/bench_failure_link_loads.py --out profiles/failure_link_loads_k48.jsonl
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

RTOL = 1e-9
K = 48
NSCEN = 64
SAMPLE_ROWS = (0, 1, 23, 24, 500, 777, 1150, 1151)
SAMPLE_SCEN = (0, 21, 42, 63)


def demand(fabric, csr):
    """Every ordered pair of host-bearing switches, grouped by destination
    row: (dsts, rows, srcs, w)."""
    hv, _ = fabric.host_table()
    hc = np.bincount(hv, minlength=csr.V).astype(np.int64)
    dsts = np.nonzero(hc)[0]
    n = dsts.shape[0]
    rows = np.repeat(np.arange(n), n)
    srcs = np.tile(dsts, n)
    keep = dsts[rows] != srcs
    rows, srcs = rows[keep], srcs[keep]
    w = (hc[srcs] * hc[dsts][rows]).astype(np.uint64)
    return dsts, rows, srcs, w


def cost_sets(csr):
    h = K // 2
    esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    tier = (esrc < h) | (np.asarray(csr.col) < h)        # cores 0 .. h - 1: aggregation position 0
    return [("unit", np.ones(int(csr.E), np.uint32)),
            ("core_tier_0_at_cost_2", np.where(tier, 2, 1).astype(np.uint32))]


def cable_scenarios(csr, hosts):
    """NSCEN single cables as sorted pairs of edge indices (both directions):
    half between an edge switch and an aggregation switch, half between an
    aggregation switch and a core, evenly strided over each kind."""
    V = int(csr.V)
    esrc = np.repeat(np.arange(V), np.diff(csr.row_ptr))
    col = np.asarray(csr.col)
    is_core = np.arange(V) < (K // 2) ** 2
    is_edge = np.zeros(V, bool)
    is_edge[hosts] = True
    up = np.nonzero(esrc < col)[0]                         # one direction per cable
    key = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(esrc.tolist(), col.tolist()))}
    kinds = [up[is_edge[esrc[up]] | is_edge[col[up]]], up[is_core[esrc[up]] | is_core[col[up]]]]
    scen = []
    for es in kinds:
        pick = es[np.linspace(0, es.shape[0] - 1, NSCEN // 2).astype(np.int64)]
        scen += [sorted([int(e), key[(int(col[e]), int(esrc[e]))]]) for e in pick.tolist()]
    assert len(scen) == NSCEN and len({tuple(s) for s in scen}) == NSCEN
    return scen


def reduced(csr, cost, failed):
    """(csr, cost) with the failed edges really removed."""
    V, E = int(csr.V), int(csr.E)
    keep = np.ones(E, bool)
    keep[np.asarray(failed, np.int64)] = False
    esrc = np.repeat(np.arange(V), np.diff(csr.row_ptr))
    rp = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(esrc[keep], minlength=V), out=rp[1:])
    return T.CSR(csr.dpids, rp, np.asarray(csr.col)[keep], np.asarray(csr.port)[keep]), cost[keep]


def med(ts):
    return round(float(np.median(ts)), 4)


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def bench(fabric, name, cost, reps, out):
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    E = int(csr.E)
    dsts, rows, srcs, w = demand(fabric, csr)
    scen = cable_scenarios(csr, dsts)
    rec = {"fabric": "fat_tree_k%d" % K, "costs": name, "V": int(csr.V), "E": E,
           "rows": int(dsts.shape[0]), "switch_pairs": int(rows.shape[0]), "scenarios": NSCEN,
           "items": NSCEN * int(dsts.shape[0]), "reps": reps}

    # -- the new call: one launch for all scenarios and rows ----------------
    eng = EN.RouteEngine(0)
    sel = np.isin(rows, np.asarray(SAMPLE_ROWS))
    sub = [scen[i] for i in SAMPLE_SCEN]
    for split in EN.SPLITS:
        eng.failure_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, scen, split)   # warm-up
        ks = []
        for _ in range(reps):
            load, lost, routed = eng.failure_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, scen,
                                                             split, timing=True)
            ks.append(eng.ctx.last_kernel_ms())
        rec["kernel"] = eng.ctx.last_kernel()
        assert np.isfinite(load).all() and routed.all()
        assert not lost.any(), "a single cable cuts nothing on this fabric"
        for k, failed in enumerate(scen):
            assert not load[k][failed].any()
        rec["lost_per_scenario_max_" + split] = float(lost.max())
        want = EN.failure_ecmp_link_loads_host(csr, cost, dsts, rows[sel], srcs[sel], w[sel], sub,
                                               split)
        part = eng.failure_ecmp_link_loads(ex, cost, dsts, rows[sel], srcs[sel], w[sel], sub,
                                           split)
        z = want[0] == 0
        assert (part[0][z] == 0).all() and \
            np.allclose(part[0][~z], want[0][~z], rtol=RTOL, atol=0), split
        assert np.array_equal(part[2], want[2]) and np.array_equal(part[1], want[1])
        rec["max_rel_err_vs_host_sampled_items_" + split] = \
            float(np.max(np.abs(part[0][~z] - want[0][~z]) / want[0][~z]))
        rec["sampled_items"] = len(SAMPLE_SCEN) * len(SAMPLE_ROWS)
        rec["kernel_ms_" + split] = [round(x, 4) for x in ks]
        rec["kernel_median_ms_" + split] = med(ks)
        rec["kernel_median_ms_per_scenario_" + split] = round(float(np.median(ks)) / NSCEN, 5)
        note(name, split, "kernel ms", rec["kernel_median_ms_" + split])
    eng.close()

    # -- kernel yardstick: the existing kernels on the really reduced graph --
    eng = EN.RouteEngine(0)
    yt, yl = [], {s: [] for s in EN.SPLITS}
    for failed in scen:
        rcsr, rcost = reduced(csr, cost, failed)
        rex = types.SimpleNamespace(csr=rcsr)
        pc, _, _ = eng.cost_tables(rex, rcost, dsts)       # upload + warm-up
        ts = []
        for _ in range(reps):
            pc, _, _ = eng.cost_tables(rex, rcost, dsts, timing=True)
            ts.append(eng.ctx.last_kernel_ms())
        yt.append(float(np.median(ts)))
        rec["yardstick_tables_kernel"] = eng.ctx.last_kernel()
        for split in EN.SPLITS:
            eng.cost_ecmp_link_loads(rex, rcost, pc, rows, srcs, w, split)
            ts = []
            for _ in range(reps):
                eng.cost_ecmp_link_loads(rex, rcost, pc, rows, srcs, w, split, timing=True)
                ts.append(eng.ctx.last_kernel_ms())
            yl[split].append(float(np.median(ts)))
        rec["yardstick_loads_kernel"] = eng.ctx.last_kernel()
    eng.close()
    note(name, "yardstick kernels done")
    rec["yardstick_cost_tables_kernel_ms_sum"] = round(sum(yt), 4)
    for split in EN.SPLITS:
        total = sum(yt) + sum(yl[split])
        rec["yardstick_cost_ecmp_loads_kernel_ms_sum_" + split] = round(sum(yl[split]), 4)
        rec["yardstick_kernels_ms_per_scenario_" + split] = round(total / NSCEN, 5)
        rec["kernel_ratio_new_over_yardstick_" + split] = \
            round(rec["kernel_median_ms_" + split] / total, 3)

    # -- end to end: the drop-in call against the public round trip ---------
    db = fabric.populate(TopologyDB())
    dp = csr.dpids
    esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    costed = np.nonzero(cost != 1)[0]
    if costed.size:
        db.set_link_costs({(int(dp[esrc[e]]), int(dp[csr.col[e]])): int(cost[e])
                           for e in costed.tolist()})
    failures = [[(int(dp[esrc[e]]), int(dp[csr.col[e]])) for e in failed] for failed in scen]
    for split in EN.SPLITS:
        base = db.all_pairs_least_cost_ecmp_link_loads(split)     # warm: tables resident
        walls = []
        for _ in range(reps):
            t = time.perf_counter()
            got = db.all_pairs_failure_link_loads(failures, split)
            walls.append((time.perf_counter() - t) * 1e3)
        assert not got.lost.any() and np.allclose(got.base.load, base.load, rtol=RTOL, atol=0)
        note(name, split, "call wall ms", med(walls))
        rec["call_wall_ms_" + split] = [round(x, 2) for x in walls]
        rec["call_wall_median_ms_per_scenario_" + split] = round(float(np.median(walls)) / NSCEN, 3)
        # the existing public path, one scenario per round trip (reps of them)
        loop = []
        step = max(1, NSCEN // reps)
        for k in range(0, step * reps, step):
            links = [db.links[a][b] for a, b in failures[k]]
            t = time.perf_counter()
            for lk in links:
                db.delete_link(lk)
            one = db.all_pairs_least_cost_ecmp_link_loads(split)
            for lk in links:
                db.add_link(lk)
            loop.append((time.perf_counter() - t) * 1e3)
            z = one.load == 0
            mine = np.delete(got.load[k], scen[k])         # the twin's graph lacks the failed links
            assert (mine[z] == 0).all() and np.allclose(mine[~z], one.load[~z], rtol=RTOL, atol=0)
        db.all_pairs_least_cost_ecmp_link_loads(split)            # back on the intact graph
        rec["round_trip_wall_ms_" + split] = [round(x, 2) for x in loop]
        rec["round_trip_wall_median_ms_per_scenario_" + split] = med(loop)
        rec["wall_ratio_new_over_round_trip_" + split] = \
            round(rec["call_wall_median_ms_per_scenario_" + split] / float(np.median(loop)), 4)
    db.engine.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "failure_link_loads_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    fabric = T.fat_tree(K)
    for name, cost in cost_sets(fabric.csr()):
        bench(fabric, name, cost, a.reps, a.out)


if __name__ == "__main__":
    main()
