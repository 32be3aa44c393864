#!/usr/bin/env python
"""Multicast trees of MPI_Allgather as broadcasts on the k=48 fat-tree: 1,152
groups, one root per host-bearing switch, every host-bearing switch a member.

Per route mode (default, shortest, least_cost) one JSON line goes to --out:

* kernel ms of sdnr_multicast_trees, count (with the loads) plus fill, on the
  resident rows; the same through RouteEngine.multicast_trees (host clock
  around calls that end in a device synchronise and return host arrays);
* ms per call of the drop-in's multicast_trees and multicast_link_loads on
  one host per switch, tables cached;
* one sdnr_link_loads pass over the same rows and (root, member) pairs, the
  unicast fan-out, on the same box in the same run: kernel and call time, and
  the peak link load of the two -- the number the feature exists to show;
* default route only: the way to the same entries before this call existed,
  TopologyDB.route_entries over every (root, member) pair plus np.unique on
  the host, alternated with the drop-in call, and whether the two agree.

    python tools/bench_multicast_trees.py --out profiles/multicast_trees_k48.jsonl
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


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return out


def ms(ts):
    return [round(x * 1e3, 3) for x in ts]


def med(ts):
    return round(float(np.median(ts)) * 1e3, 3)


def link_costs(csr, seed=48):
    return np.random.default_rng(seed).integers(1, 9, int(csr.E)).astype(np.uint32)


def engine_rows(eng, ex, srcs, route, cost):
    """(device rows, layout, to_root) of the host-bearing switches."""
    if route == "default":
        par, prt, _ = eng.dfs_tables(ex, srcs)
        layout = EN.tree_layout(ex.csr)
        return (par if layout == EN.INT32 else eng.pack_trees(ex, par, prt, layout)), layout, False
    if route == "shortest":
        return eng.shortest_tables(ex, srcs)[1], EN.INT32, True
    return eng.cost_tables(ex, cost, srcs)[1], EN.INT32, True


def bench(fabric, name, route, reps, out):
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    hv, _ = fabric.host_table()
    srcs = np.unique(hv).astype(np.int32)
    n = int(srcs.shape[0])
    cost = link_costs(csr)
    rec = {"fabric": name, "route": route, "V": int(csr.V), "E": int(csr.E), "groups": n,
           "members": n * n, "reps": reps,
           "maps_in_lds": bool(EN.multicast_maps_in_lds(csr.V, csr.E))}

    # -- the engine on resident rows ------------------------------------
    eng = EN.RouteEngine(0)
    tab, layout, to_root = engine_rows(eng, ex, srcs, route, cost)
    rec["layout"] = layout
    slot = np.arange(n, dtype=np.int64)
    off = np.arange(n + 1, dtype=np.int64) * n
    vert = np.tile(srcs.astype(np.int64), n)
    row = np.tile(slot, n) if to_root else np.repeat(slot, n)

    def trees(**kw):
        return eng.multicast_trees(ex, tab, layout, srcs, off, row, vert, to_root=to_root, **kw)

    reached, eo, ee, load = trees()                         # warm-up
    reached, eo, ee, load = trees()
    rec["kernel"] = eng.ctx.last_kernel()
    rec["kernel_ms_count_loads_fill"] = round(eng.last_multicast_ms, 4)
    trees(entries=False)
    rec["kernel_ms_count_loads"] = round(eng.last_multicast_ms, 4)
    assert reached.all()
    rec["union_links_per_group"] = [int(np.diff(eo).min()), int(np.diff(eo).max())]
    rec["union_links_total"] = int(eo[-1])
    assert int(load.sum()) == int(eo[-1])

    # the unicast fan-out: one sdnr_link_loads pass over the same rows and pairs
    pr = np.repeat(slot, n)                                 # the root of each (root, member) pair
    pm = np.tile(srcs.astype(np.int64), n)
    keep = srcs[pr] != pm
    lrows, lother = (np.searchsorted(srcs, pm[keep]), srcs[pr[keep]]) if to_root else \
        (pr[keep], pm[keep])

    def fan_out(timing=False):
        return eng.link_loads(ex, tab, layout, lrows, lother, None, to_root=to_root, timing=timing)

    fan_out()
    uni = fan_out(timing=True)
    rec["link_loads_kernel"] = eng.ctx.last_kernel()
    rec["link_loads_kernel_ms"] = round(eng.ctx.last_kernel_ms(), 4)
    rec["peak_link_load_multicast"] = int(load.max())
    rec["peak_link_load_unicast"] = int(uni.max())
    rec["total_link_load_multicast"] = int(load.sum())
    rec["total_link_load_unicast"] = int(uni.sum())
    assert (load <= uni).all() and ((load > 0) == (uni > 0)).all()
    t_tree, t_loads, t_uni = [], [], []
    for _ in range(reps):                                   # alternated repetitions
        t_tree += timed(trees, 1)
        t_loads += timed(lambda: trees(entries=False), 1)
        t_uni += timed(fan_out, 1)
    rec["engine_trees_ms"], rec["engine_trees_median_ms"] = ms(t_tree), med(t_tree)
    rec["engine_loads_ms"], rec["engine_loads_median_ms"] = ms(t_loads), med(t_loads)
    rec["link_loads_ms"], rec["link_loads_median_ms"] = ms(t_uni), med(t_uni)
    rec["kernel_ratio_link_loads_over_multicast"] = round(
        rec["link_loads_kernel_ms"] / rec["kernel_ms_count_loads"], 3)
    rec["call_ratio_link_loads_over_multicast"] = round(
        float(np.median(t_uni) / np.median(t_loads)), 3)
    eng.close()

    # -- the drop-in on one host per switch -------------------------------
    db = fabric.populate(TopologyDB())
    if route == "least_cost":
        rp = np.asarray(csr.row_ptr, np.int64)
        es = np.repeat(np.arange(csr.V), np.diff(rp))
        dp = np.asarray(csr.dpids).tolist()
        db.set_link_costs({(dp[u], dp[v]): int(c) for u, v, c in
                           zip(es.tolist(), np.asarray(csr.col).tolist(), cost.tolist())})
    macs = fabric.host_macs()
    first = {}
    for m in macs:
        first.setdefault(db.hosts[m].port.dpid, m)
    one = [first[d] for d in sorted(first)]
    assert len(one) == n
    groups = [(a, one) for a in one]
    got = db.multicast_trees(groups, route)                 # warm-up: the tables are computed
    ll = db.multicast_link_loads(groups, None, route)
    assert np.array_equal(ll.load, load)
    rec["dropin_entries_total"] = int(got[0][-1])
    base = None
    if route == "default":
        pairs = [(a, b) for a in one for b in one if a != b]
        pg = np.repeat(np.arange(n, dtype=np.int64), n - 1)

        def base():
            o, dpid, port = db.route_entries(pairs)
            sw = np.searchsorted(np.asarray(csr.dpids), dpid)
            key = (np.repeat(pg, np.diff(o)) * int(csr.V) + sw) * 65536 + port
            return np.unique(key), int(o[-1])

        key, total = base()                                 # warm-up
        rec["baseline_route_entries"] = total
        g_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(got[0]))
        mine = (g_of * int(csr.V) + np.searchsorted(np.asarray(csr.dpids), got[1])) * 65536 + got[2]
        rec["entries_equal_baseline"] = bool(np.array_equal(key, mine))
        assert rec["entries_equal_baseline"], "the two paths disagree"
    t_dt, t_dl, t_old = [], [], []
    for _ in range(reps):                                   # alternated repetitions
        t_dt += timed(lambda: db.multicast_trees(groups, route), 1)
        t_dl += timed(lambda: db.multicast_link_loads(groups, None, route), 1)
        if base is not None:
            t_old += timed(base, 1)
    rec["dropin_trees_ms"], rec["dropin_trees_median_ms"] = ms(t_dt), med(t_dt)
    rec["dropin_loads_ms"], rec["dropin_loads_median_ms"] = ms(t_dl), med(t_dl)
    if base is not None:
        rec["baseline_ms"], rec["baseline_median_ms"] = ms(t_old), med(t_old)
        rec["ratio_baseline_over_dropin_trees"] = round(
            float(np.median(t_old) / np.median(t_dt)), 2)
        rec["faster_in_every_rep"] = bool(all(a < b for a, b in zip(t_dt, t_old)))
    else:
        rec["baseline_ms"] = None       # not measured: route_entries walks the default route only
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multicast_trees_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=48, help="fat-tree arity (48: the recorded workload)")
    ap.add_argument("--routes", default="default,shortest,least_cost")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 alternated repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    fabric = T.fat_tree(a.k)
    for route in a.routes.split(","):
        bench(fabric, "fat_tree_k%d" % a.k, route, a.reps, a.out)


if __name__ == "__main__":
    main()
