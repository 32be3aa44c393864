#!/usr/bin/env python
"""ECMP link loads over the least-cost routes of the all-host-pairs demand:
sdnr_cost_ecmp_link_loads (both splits) against its numpy restatement, and --
the yardstick -- against sdnr_ecmp_link_loads (ecmp_loads_kernel, the
hop-count kernel) on the same demand.

One GPU, the k=48 fat-tree, the least-cost rows of all 1,152 host-bearing
switches resident.  Two cost sets: unit costs (the least-cost DAG is the
hop-count DAG: the two kernels compute the same loads) and one
aggregation-to-core tier at cost 2 (every link of the first core group, both
directions: the position-0 aggregation switches of the other pods then tie a
3-link route over their own cores with a 5-link route over a neighbouring
edge switch -- next hops at different hop depths).  Per cost set the calls
are warmed up, the device loads are compared with
engine.cost_ecmp_link_loads_host on sampled rows (rtol 1e-9) and with the
conservation sum (sum of load x cost = sum of weight x pcost) on all rows,
then the two kernels are timed in alternation (the SDNR_TIMING event pair,
median of --reps) and so are the whole calls (host clock around work that
ends in a device synchronise).  No time is a pass condition.  One JSON line
per cost set goes to --out.

    python tools/bench_cost_ecmp_link_loads.py --out profiles/cost_ecmp_link_loads_k48.jsonl
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

RTOL = 1e-9
K = 48
SAMPLE = (0, 1, 23, 24, 500, 777, 1150, 1151)


def demand(fabric, csr):
    """Pairs grouped by destination row: (dsts, rows, srcs, w)."""
    hv, _ = fabric.host_table()
    hc = np.bincount(hv, minlength=csr.V).astype(np.int64)
    dsts = np.nonzero(hc)[0]
    n = dsts.shape[0]
    rows = np.repeat(np.arange(n), n)
    srcs = np.tile(dsts, n)
    keep = dsts[rows] != srcs                            # n * (n - 1) ordered switch pairs
    rows, srcs = rows[keep], srcs[keep]
    w = (hc[srcs] * hc[dsts][rows]).astype(np.uint64)
    return dsts, rows, srcs, w


def cost_sets(csr):
    h = K // 2
    esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    tier = (esrc < h) | (np.asarray(csr.col) < h)        # cores 0 .. h - 1: aggregation position 0
    return [("unit", np.ones(int(csr.E), np.uint32)),
            ("core_tier_0_at_cost_2", np.where(tier, 2, 1).astype(np.uint32))]


def chain_stats(csr, cost, pc_row):
    """(longest next-hop chain, vertices whose next hops differ in chain
    length) of one pcost row: the depths the kernel orders by, found here by
    one pass in ascending pcost order."""
    V = int(csr.V)
    rp = np.asarray(csr.row_ptr, np.int64)
    esrc = np.repeat(np.arange(V, dtype=np.int64), np.diff(rp))
    edst = np.asarray(csr.col, np.int64)
    pc = pc_row.astype(np.int64)
    fin = pc != EN.COST_INF
    on = np.nonzero(fin[esrc] & (pc[esrc] > 0) & fin[edst] & (pc[edst] + cost == pc[esrc]))[0]
    depth = np.zeros(V, np.int64)
    lo = np.full(V, V, np.int64)
    for c in np.unique(pc[esrc[on]]).tolist():
        e = on[pc[esrc[on]] == c]
        np.maximum.at(depth, esrc[e], depth[edst[e]] + 1)
        np.minimum.at(lo, esrc[e], depth[edst[e]] + 1)
    mixed = int(((lo < V) & (lo != depth)).sum())
    return int(depth.max()), mixed


def median_ms(ts):
    return round(float(np.median(ts)), 4)


def bench(fabric, name, cost, reps, out):
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    eng = EN.RouteEngine(0)
    dsts, rows, srcs, w = demand(fabric, csr)
    dist, _, _ = eng.shortest_tables(ex, dsts)
    pc, _, _ = eng.cost_tables(ex, cost, dsts)
    hp = EN._host(pc).view(np.uint32)
    p = hp[rows, srcs].astype(np.int64)
    assert (p != EN.COST_INF).all()
    total = int((w.astype(np.int64) * p).sum())
    depth, mixed = chain_stats(csr, cost.astype(np.int64), hp[0])
    rec = {"fabric": "fat_tree_k%d" % K, "costs": name, "V": int(csr.V), "E": int(csr.E),
           "rows": int(dsts.shape[0]), "switch_pairs": int(rows.shape[0]),
           "host_pairs": int(w.sum()), "weight_x_pcost": total,
           "row0_longest_next_hop_chain": depth, "row0_vertices_with_mixed_depth_next_hops": mixed,
           "row0_hops_max": int(EN._host(dist).view(np.uint16)[0].max()), "reps": reps}

    def new(split="route", timing=False):
        return eng.cost_ecmp_link_loads(ex, cost, pc, rows, srcs, w, split, timing=timing)

    def old(split="route", timing=False):
        return eng.ecmp_link_loads(ex, dist, rows, srcs, w, split, timing=timing)

    sel = np.isin(rows, np.asarray(SAMPLE))
    for split in EN.SPLITS:
        new(split)                                       # warm-up
        old(split)
        got = new(split, timing=True)
        rec["kernel"] = eng.ctx.last_kernel()
        assert np.isfinite(got).all()
        assert abs(float((got * cost).sum()) - total) <= RTOL * total, split
        want = EN.cost_ecmp_link_loads_host(csr, cost, hp, rows[sel], srcs[sel], w[sel], split)
        part = eng.cost_ecmp_link_loads(ex, cost, pc, rows[sel], srcs[sel], w[sel], split)
        z = want == 0
        assert (part[z] == 0).all() and np.allclose(part[~z], want[~z], rtol=RTOL, atol=0), split
        rec["max_rel_err_vs_host_sampled_rows_" + split] = \
            float(np.max(np.abs(part[~z] - want[~z]) / want[~z]))
        rec["run_to_run_bits_equal_" + split] = bool(np.array_equal(got, new(split)))
        if name == "unit":
            ref = old(split)
            z = ref == 0
            assert (got[z] == 0).all() and np.allclose(got[~z], ref[~z], rtol=RTOL, atol=0), split
        rec["links_loaded_" + split] = int((got > 0).sum())
    # the same rows with ONE source each: the ordering sweeps and the two
    # passes are unchanged, the adds shrink to one source's DAG
    n = dsts.shape[0]
    r1, s1 = np.arange(n), np.roll(dsts, n // 2)
    eng.cost_ecmp_link_loads(ex, cost, pc, r1, s1, None, "route")
    eng.cost_ecmp_link_loads(ex, cost, pc, r1, s1, None, "route", timing=True)
    rec["kernel_ms_one_source_per_row"] = round(eng.ctx.last_kernel_ms(), 4)
    eng.ecmp_link_loads(ex, dist, r1, s1, None, "route", timing=True)
    rec["ecmp_loads_kernel_ms_one_source_per_row"] = round(eng.ctx.last_kernel_ms(), 4)
    for split in EN.SPLITS:
        k_new, k_old, c_new, c_old = [], [], [], []
        for _ in range(reps):                            # alternated repetitions
            t = time.perf_counter()
            new(split, timing=True)
            c_new.append((time.perf_counter() - t) * 1e3)
            k_new.append(eng.ctx.last_kernel_ms())
            t = time.perf_counter()
            old(split, timing=True)
            c_old.append((time.perf_counter() - t) * 1e3)
            k_old.append(eng.ctx.last_kernel_ms())
            rec["yardstick_kernel"] = eng.ctx.last_kernel()
        rec["kernel_ms_" + split] = [round(x, 4) for x in k_new]
        rec["kernel_median_ms_" + split] = median_ms(k_new)
        rec["ecmp_loads_kernel_ms_" + split] = [round(x, 4) for x in k_old]
        rec["ecmp_loads_kernel_median_ms_" + split] = median_ms(k_old)
        rec["kernel_ratio_" + split] = round(float(np.median(k_new) / np.median(k_old)), 3)
        rec["call_median_ms_" + split] = median_ms(c_new)
        rec["ecmp_loads_call_median_ms_" + split] = median_ms(c_old)
    eng.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "cost_ecmp_link_loads_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 alternated repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    fabric = T.fat_tree(K)
    for name, cost in cost_sets(fabric.csr()):
        bench(fabric, name, cost, a.reps, a.out)


if __name__ == "__main__":
    main()
