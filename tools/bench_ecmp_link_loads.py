#!/usr/bin/env python
"""ECMP link loads of the all-host-pairs demand: sdnr_ecmp_link_loads (both
splits) against its numpy restatement, and -- for scale -- against
sdnr_link_loads over routes[0] of the same shortest-route rows.

One GPU, the distance (and next-hop) rows of every host-bearing switch
resident (1,152 on the k=48 fat-tree).  The calls are warmed up, the device
loads are compared with engine.ecmp_link_loads_host (rtol 1e-9) and with the
conservation sum (loads sum to weight x distance), then the ECMP call and the
single-route call are timed in alternation with the host clock around work
that ends in a device synchronise (both return host arrays).  The kernel time
is the SDNR_TIMING event pair.  No time is a pass condition.  One JSON line
per fabric goes to --out.

    python tools/bench_ecmp_link_loads.py --out profiles/ecmp_link_loads_k48.jsonl
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


def dag_links(csr, hd, chunk=64):
    """Links x -> n with dist[n] == dist[x] - 1, summed over the rows: the most
    global f64 adds one call can make (every such link whose tail has flow)."""
    rp = np.asarray(csr.row_ptr, np.int64)
    esrc = np.repeat(np.arange(csr.V, dtype=np.int64), np.diff(rp))
    edst = np.asarray(csr.col, np.int64)
    total = 0
    for a in range(0, hd.shape[0], chunk):
        d = hd[a:a + chunk]
        x, n = d[:, esrc], d[:, edst]
        total += int(((x != 0xFFFF) & (x == n + 1)).sum())
    return total


def spread(load):
    nz = load[load > 0]
    return {"links_loaded": int(nz.shape[0]), "links_idle": int(load.shape[0] - nz.shape[0]),
            "max_over_mean": round(float(load.max() / load.mean()), 3) if load.any() else None}


def bench(name, fabric, reps, out):
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    eng = EN.RouteEngine(0)
    dsts, rows, srcs, w = demand(fabric, csr)
    dist, nh, _ = eng.shortest_tables(ex, dsts)
    hd = EN._host(dist).view(np.uint16).astype(np.int64)
    total = int((w.astype(np.int64) * hd[rows, srcs]).sum())
    rec = {"fabric": name, "V": int(csr.V), "E": int(csr.E), "rows": int(dsts.shape[0]),
           "switch_pairs": int(rows.shape[0]), "host_pairs": int(w.sum()),
           "levels_max": int(hd[hd != 0xFFFF].max()), "dag_links_all_rows": dag_links(csr, hd),
           "weight_x_distance": total, "reps": reps}

    def ecmp(split="route", timing=False):
        return eng.ecmp_link_loads(ex, dist, rows, srcs, w, split, timing=timing)

    def first_route():
        return eng.link_loads(ex, nh, EN.INT32, rows, srcs, w, to_root=True)

    for split in EN.SPLITS:
        ecmp(split)                                      # warm-up
        got = ecmp(split, timing=True)
        rec["kernel"] = eng.ctx.last_kernel()
        rec["kernel_ms_" + split] = round(eng.ctx.last_kernel_ms(), 4)
        t = time.perf_counter()
        want = EN.ecmp_link_loads_host(csr, EN._host(dist), rows, srcs, w, split)
        rec["host_restatement_ms_" + split] = round((time.perf_counter() - t) * 1e3, 1)
        z = want == 0
        assert (got[z] == 0).all() and np.allclose(got[~z], want[~z], rtol=RTOL, atol=0), split
        assert abs(float(got.sum()) - total) <= RTOL * total, split
        rec["max_rel_err_vs_host_" + split] = float(np.max(np.abs(got[~z] - want[~z]) / want[~z]))
        rec["run_to_run_bits_equal_" + split] = bool(np.array_equal(got, ecmp(split)))
        rec["spread_" + split] = spread(got)
    # the same rows with ONE source each: the level DP and the level sweeps
    # are unchanged, the adds shrink to one source's DAG -- what the kernel
    # costs without the bulk of its atomics
    n = dsts.shape[0]
    r1, s1 = np.arange(n), np.roll(dsts, n // 2)
    eng.ecmp_link_loads(ex, dist, r1, s1, None, "route")
    eng.ecmp_link_loads(ex, dist, r1, s1, None, "route", timing=True)
    rec["kernel_ms_one_source_per_row"] = round(eng.ctx.last_kernel_ms(), 4)
    one = first_route()                                  # warm-up
    assert int(one.sum(dtype=np.uint64)) == total
    rec["spread_first_route"] = spread(one.astype(np.float64))
    rec["loads_equal_host"] = True
    t_new, t_hop, t_one = [], [], []
    for _ in range(reps):                                # alternated repetitions
        t = time.perf_counter()
        ecmp("route")
        t_new.append(time.perf_counter() - t)
        t = time.perf_counter()
        first_route()
        t_one.append(time.perf_counter() - t)
        t = time.perf_counter()
        ecmp("hop")
        t_hop.append(time.perf_counter() - t)
    for key, ts in (("ecmp_route", t_new), ("ecmp_hop", t_hop), ("first_route", t_one)):
        rec[key + "_ms"] = [round(x * 1e3, 3) for x in ts]
        rec[key + "_median_ms"] = round(float(np.median(ts)) * 1e3, 3)
    eng.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecmp_link_loads_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="", help="comma-separated fabric names")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 alternated repetitions")
    fabrics = [("fat_tree_k48", lambda: T.fat_tree(48)),
               ("dragonfly_a16_h8_p8", lambda: T.dragonfly(16, 8, 8))]
    only = set(x for x in a.only.split(",") if x)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    for name, make in fabrics:
        if not only or name in only:
            bench(name, make(), a.reps, a.out)


if __name__ == "__main__":
    main()
