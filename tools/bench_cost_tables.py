#!/usr/bin/env python
"""Least-cost tables of every host-bearing destination: sdnr_cost_tables
against sdnr_shortest_tables (unit costs: the same tables from the bit-mask
BFS) and against its CPU restatement engine.cost_tables_host (random costs in
[1, 16], seeded) spread over 16 host processes.

One GPU.  The tables are compared for equality before anything is timed.  The
kernel time is the SDNR_TIMING event pair; the call time is the host clock
around a call that ends in a device synchronise (tables stay on the device).
Repetitions alternate the two sides.  The host side is the whole destination
list cut into slices for a pool of 16 worker processes (started before the GPU
is opened; they never touch it).  No time is a pass condition.  One JSON line
per fabric goes to --out.

    python tools/bench_cost_tables.py --out profiles/cost_tables_k48.jsonl
"""
import argparse
import json
import multiprocessing
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdn-mpi-router_amd"))

from sdnmpi_amd import engine as EN          # noqa: E402
from sdnmpi_amd import topologies as T       # noqa: E402

HOST_PROCS = 16
FABRICS = {"fat_tree_k48": lambda: T.fat_tree(48),
           "dragonfly_a16_h8_p8": lambda: T.dragonfly(16, 8, 8)}


def _host_slice(job):
    """Pool worker: the restatement's tables of one slice of destinations."""
    name, cost, dsts = job
    csr = _host_slice.csr.get(name)
    if csr is None:
        csr = _host_slice.csr[name] = FABRICS[name]().csr()
    return EN.cost_tables_host(csr, cost, dsts)


_host_slice.csr = {}


def host_tables(pool, name, cost, dsts):
    """cost_tables_host over the pool: (pcost, nh, nh_port) of every dst."""
    parts = pool.map(_host_slice, [(name, cost, s) for s in
                                   np.array_split(dsts, min(len(dsts), 4 * HOST_PROCS))])
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def stats(rec, key, ts):
    rec[key + "_ms"] = [round(x * 1e3, 3) for x in ts]
    rec[key + "_median_ms"] = round(float(np.median(ts)) * 1e3, 3)


def bench(name, reps, out, pool):
    import torch
    fabric = FABRICS[name]()
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    eng = EN.RouteEngine(0)
    hv, _ = fabric.host_table()
    dsts = np.unique(hv).astype(np.int32)
    D, V = int(dsts.shape[0]), int(csr.V)
    rec = {"fabric": name, "V": V, "E": int(csr.E), "rows": D, "reps": reps,
           "host_processes": HOST_PROCS}
    td = eng._ids(dsts)
    dist = eng._empty(D, V, torch.int16)
    nh0, nhp0 = eng._empty(D, V, torch.int32), eng._empty(D, V, torch.int32)

    def shortest(timing=False):
        eng.ctx.shortest_tables_device(td.data_ptr(), D, dist.data_ptr(), nh0.data_ptr(),
                                       nhp0.data_ptr(), timing=timing)
        eng.ctx.synchronize()

    # (a) unit costs: the tables of the bit-mask BFS
    ones = np.ones(int(csr.E), np.uint32)
    eng.cost_tables(ex, ones, dsts)                      # warm-up
    pc, nh, nhp = eng.cost_tables(ex, ones, dsts, timing=True)
    rec["kernel"] = eng.ctx.last_kernel()
    rec["kernel_ms_unit"] = round(eng.ctx.last_kernel_ms(), 4)
    shortest()
    shortest(timing=True)
    rec["shortest_kernel"] = eng.ctx.last_kernel()
    rec["shortest_launches"] = eng.ctx.last_launches()
    rec["shortest_kernel_ms"] = round(eng.ctx.last_kernel_ms(), 4)
    wide = dist.to(torch.int32) & 0xFFFF
    wide = wide.masked_fill(wide == 0xFFFF, -1)
    assert bool((pc == wide).all()) and bool((nh == nh0).all()) and bool((nhp == nhp0).all())
    rec["unit_tables_equal_shortest"] = True
    t_cost, t_sp = [], []
    for _ in range(reps):
        t = time.perf_counter()
        eng.cost_tables(ex, ones, dsts)
        t_cost.append(time.perf_counter() - t)
        t = time.perf_counter()
        shortest()
        t_sp.append(time.perf_counter() - t)
    stats(rec, "unit_call", t_cost)
    stats(rec, "shortest_call", t_sp)
    rec["unit_kernel_over_shortest_kernel"] = round(rec["kernel_ms_unit"] /
                                                    rec["shortest_kernel_ms"], 2)

    # (b) random costs in [1, 16]: the restatement on 16 host processes
    cost = np.random.default_rng(48).integers(1, 17, int(csr.E)).astype(np.uint32)
    want = host_tables(pool, name, cost, dsts)
    eng.cost_tables(ex, cost, dsts)                      # warm-up (uploads the costs)
    pc, nh, nhp = eng.cost_tables(ex, cost, dsts, timing=True)
    rec["kernel_ms_random"] = round(eng.ctx.last_kernel_ms(), 4)
    assert np.array_equal(EN._host(pc).view(np.uint32), want[0])
    assert np.array_equal(EN._host(nh), want[1]) and np.array_equal(EN._host(nhp), want[2])
    rec["random_tables_equal_host"] = True
    rec["pcost_max"] = int(want[0][want[0] != EN.COST_INF].max())
    t_cost, t_host = [], []
    for _ in range(reps):
        t = time.perf_counter()
        eng.cost_tables(ex, cost, dsts)
        t_cost.append(time.perf_counter() - t)
        t = time.perf_counter()
        host_tables(pool, name, cost, dsts)
        t_host.append(time.perf_counter() - t)
    stats(rec, "random_call", t_cost)
    stats(rec, "host_16_processes", t_host)
    eng.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_tables_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="", help="comma-separated fabric names")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 alternated repetitions")
    only = set(x for x in a.only.split(",") if x)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    # the host workers start before the GPU is opened and never touch it
    with multiprocessing.get_context("spawn").Pool(HOST_PROCS) as pool:
        for name in FABRICS:
            if not only or name in only:
                bench(name, a.reps, a.out, pool)


if __name__ == "__main__":
    main()
