#!/usr/bin/env python
"""Max-min fair completion times of the all-host-pairs exchange on the k=48
fat-tree in the switch-pair form (1,152^2 flows, multiplicity hosts(s) *
(hosts(d) - [s == d]), unit capacities, the same byte count for every host
pair: MPI_Alltoall with equal blocks), on the default trees and on the shortest
next-hop rows: sdnr_fair_times, whose epochs and fillings advance from state on
the device, against what a caller could do before it -- one engine.fair_rates
call per epoch with the departed flows' multiplicity set to 0, plus the numpy
advance.

One GPU.  Both sides run the same epochs (at most --max-epochs, 256 by
default) and their results are compared bit for bit before anything is timed.
The kernel time is the SDNR_TIMING event pair (from the first launch to the
last, the status read-backs between the batches included; the baseline's is
the sum over its calls); the call time is the host clock around the engine
call or the baseline loop.  Repetitions alternate the sides.  No time is a
pass condition.  One JSON line per route goes to --out.

    python tools/bench_fair_times.py --out profiles/fair_times_k48.jsonl
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


def per_epoch_loop(eng, ex, tree, rows, verts, mult, nbytes, cap, to_root, max_epochs):
    """The completion times by one engine.fair_rates call per epoch and the
    advance in numpy (engine.fair_times_host with the device doing the
    fillings); also returns the summed kernel time."""
    n = rows.shape[0]
    m = np.where(nbytes == 0, np.uint64(0), mult)
    time_, epoch = np.full(n, np.inf), np.full(n, -1, np.int32)
    left = nbytes.copy()
    carried = np.zeros(cap.shape[0])
    e_time, e_rounds, t, kernel_ms = [], [], np.float64(0.0), 0.0
    rate0 = None
    for j in range(max_epochs + 1):
        rate, _, rnd, level, used = eng.fair_rates(ex, tree, EN.INT32, rows, verts, m, cap,
                                                   to_root=to_root, timing=True)
        kernel_ms += eng.ctx.last_kernel_ms()
        if j == 0:
            rate0 = rate
            bare = np.isinf(rate)
            time_[bare], left[bare] = 0.0, 0.0
        fl = np.nonzero(rnd >= 0)[0]
        if fl.size == 0:
            break
        if j == max_epochs:
            epoch[fl] = -2
            break
        q = left[fl] / rate[fl]
        dt = q.min()
        t = t + dt
        carried = carried + used * dt
        rest = left[fl] - rate[fl] * dt
        done = (q == dt) | (rest <= 0.0)
        time_[fl[done]], epoch[fl[done]] = t, j
        left[fl] = np.where(done, 0.0, rest)
        m[fl[done]] = 0
        e_time.append(t)
        e_rounds.append(len(level))
    return (time_, epoch, rate0, left, np.asarray(e_time, np.float64),
            np.asarray(e_rounds, np.int32), carried), kernel_ms


def bench_route(eng, fabric, route, reps, max_epochs, block):
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    hv, _ = fabric.host_table()
    hc = np.bincount(hv, minlength=csr.V).astype(np.int64)
    sw = np.nonzero(hc)[0].astype(np.int32)
    n = int(sw.shape[0])
    rows = np.repeat(np.arange(n), n)
    other = np.tile(sw, n)
    mult = (hc[sw[rows]] * (hc[other] - (sw[rows] == other))).astype(np.uint64)
    nbytes = np.full(rows.shape[0], float(block))
    cap = np.ones(int(csr.E), np.float64)
    if route == "default":
        tree, to_root = eng.dfs_tables(ex, sw)[0], False
    else:
        tree, to_root = eng.shortest_tables(ex, sw)[1], True
    rec = {"fabric": "fat_tree_k48", "route": route, "V": int(csr.V), "E": int(csr.E), "rows": n,
           "flows": int(rows.shape[0]), "demand": int(mult.sum()), "bytes_per_pair": float(block),
           "max_epochs": max_epochs, "reps": reps}
    run = lambda timing: eng.fair_times(ex, tree, EN.INT32, rows, other, mult, nbytes, cap,  # noqa
                                        to_root=to_root, max_epochs=max_epochs, timing=timing)
    got = run(False)
    rec["kernel"] = eng.ctx.last_kernel()
    rec["launches"] = eng.ctx.last_launches()
    rec["epochs"] = int(got[4].shape[0])
    rec["complete"] = not bool((got[1] == -2).any())
    rec["rounds"] = int(got[5].sum())
    rec["steps"] = int((got[5].astype(np.int64) + 2).sum()) + 1
    assert rec["launches"] == EN.fair_times_launches(got[5])
    want, _ = per_epoch_loop(eng, ex, tree, rows, other, mult, nbytes, cap, to_root, max_epochs)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(
            g.view(np.uint64) if g.dtype == np.float64 else g,
            w.view(np.uint64) if w.dtype == np.float64 else w)
    rec["equal_per_epoch_loop_bit_for_bit"] = True
    live = np.isfinite(got[2]) & (got[2] > 0)
    rec["step_time_bound"] = float((nbytes[live] / got[2][live]).max())
    fin = got[0][np.isfinite(got[0])]
    rec["makespan"] = float(fin.max()) if rec["complete"] else None
    rec["last_epoch_time"] = float(got[4][-1]) if rec["epochs"] else 0.0
    if rec["complete"]:
        rec["bound_over_makespan"] = round(rec["step_time_bound"] / rec["makespan"], 4)
    k_new, c_new, k_old, c_old = [], [], [], []
    for _ in range(reps):
        t = time.perf_counter()
        _, ms = per_epoch_loop(eng, ex, tree, rows, other, mult, nbytes, cap, to_root, max_epochs)
        c_old.append((time.perf_counter() - t) * 1e3)
        k_old.append(ms)
        t = time.perf_counter()
        run(True)
        c_new.append((time.perf_counter() - t) * 1e3)
        k_new.append(eng.ctx.last_kernel_ms())
    stats(rec, "fair_times_kernel", k_new)
    stats(rec, "fair_times_call", c_new)
    stats(rec, "per_epoch_loop_kernel", k_old)
    stats(rec, "per_epoch_loop_call", c_old)
    rec["fair_times_kernel_ms_per_epoch"] = round(
        rec["fair_times_kernel_median_ms"] / max(1, rec["epochs"]), 4)
    rec["fair_times_kernel_ms_per_step"] = round(
        rec["fair_times_kernel_median_ms"] / rec["steps"], 4)
    rec["per_epoch_loop_call_over_fair_times_call"] = round(
        rec["per_epoch_loop_call_median_ms"] / rec["fair_times_call_median_ms"], 2)
    rec["per_epoch_loop_kernel_over_fair_times_kernel"] = round(
        rec["per_epoch_loop_kernel_median_ms"] / rec["fair_times_kernel_median_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fair_times_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-epochs", type=int, default=256)
    ap.add_argument("--bytes", type=float, default=1048576.0, help="bytes per host pair")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 alternated repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    fabric = T.fat_tree(48)
    eng = EN.RouteEngine(0)
    try:
        for route in ("default", "shortest"):
            line = json.dumps(bench_route(eng, fabric, route, a.reps, a.max_epochs, a.bytes))
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
