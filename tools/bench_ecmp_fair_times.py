#!/usr/bin/env python
"""Max-min fair completion times over ECMP of the all-host-pairs exchange on
the k=48 fat-tree in the switch-pair form (1,152^2 flows, multiplicity hosts(s)
* (hosts(d) - [s == d]), unit capacities, unit link costs), under both splits:
sdnr_ecmp_fair_times, whose epochs and fillings advance from state on the
device, against what a caller could do before it -- one engine.ecmp_fair_rates
call per epoch with the departed flows' multiplicity set to 0, plus the numpy
advance, tolerance rule included.

Two workloads: "equal", the same block for every host pair (MPI_Alltoall with
equal blocks: one epoch expected), and "mixed", a block of 1, 2, 4 or 8 times
--bytes chosen per destination switch from a fixed seed (several epochs with
refills, at most --max-epochs).

One GPU.  Both sides run the same epochs; before anything is timed their
results are compared: epochs, every flow's epoch and the rounds equal, the
largest relative deviation of a double recorded.  The kernel time is the
SDNR_TIMING event pair (from the first launch to the last, the status
read-backs between the batches included; the baseline's is the sum over its
calls); the call time is the host clock around the engine call or the baseline
loop.  Repetitions alternate the sides.  No time is a pass condition.  One JSON
line per workload and split goes to --out.

    python tools/bench_ecmp_fair_times.py --out profiles/ecmp_fair_times_k48.jsonl
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

TOL = 1e-9                                   # the cap of tests/test_ecmp_fair_times.py's TOL
SEED = 2148                                  # the mixed workload's block sizes


def stats(rec, key, ts):
    rec[key + "_ms"] = [round(x, 4) for x in ts]
    rec[key + "_median_ms"] = round(float(np.median(ts)), 4)


def per_epoch_loop(eng, ex, cost, pc, rows, srcs, mult, nbytes, cap, split, max_epochs):
    """The completion times by one engine.ecmp_fair_rates call per epoch and
    the advance in numpy (engine.ecmp_fair_times_host with the device doing the
    fillings); also returns the summed kernel time."""
    n = rows.shape[0]
    m = np.where(nbytes == 0, np.uint64(0), mult)
    time_, epoch = np.full(n, np.inf), np.full(n, -1, np.int32)
    left = nbytes.copy()
    carried = np.zeros(cap.shape[0])
    e_time, e_rounds, t, kernel_ms = [], [], np.float64(0.0), 0.0
    rate0 = None
    tie = np.float64(EN.FAIR_TIE)
    for j in range(max_epochs + 1):
        rate, _, rnd, level, used = eng.ecmp_fair_rates(ex, cost, pc, rows, srcs, m, cap, None,
                                                        split, timing=True)
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
        slack = dt * tie
        bound = dt + slack
        t = t + dt
        carried = carried + used * dt
        rest = left[fl] - rate[fl] * dt
        done = (q <= bound) | (rest <= 0.0)
        time_[fl[done]], epoch[fl[done]] = t, j
        left[fl] = np.where(done, 0.0, rest)
        m[fl[done]] = 0
        e_time.append(t)
        e_rounds.append(len(level))
    return (time_, epoch, rate0, left, np.asarray(e_time, np.float64),
            np.asarray(e_rounds, np.int32), carried), kernel_ms


def bench_case(eng, fabric, workload, split, reps, max_epochs, block):
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    hv, _ = fabric.host_table()
    hc = np.bincount(hv, minlength=csr.V).astype(np.int64)
    sw = np.nonzero(hc)[0].astype(np.int32)
    n = int(sw.shape[0])
    rows = np.repeat(np.arange(n), n)                     # row = destination
    srcs = np.tile(sw, n)
    mult = (hc[srcs] * (hc[sw[rows]] - (sw[rows] == srcs))).astype(np.uint64)
    if workload == "equal":
        nbytes = np.full(rows.shape[0], float(block))
    else:
        per_dst = np.random.default_rng(SEED).choice(np.asarray([1.0, 2.0, 4.0, 8.0]), n)
        nbytes = float(block) * per_dst[rows]
    cost = np.ones(int(csr.E), np.uint32)
    cap = np.ones(int(csr.E), np.float64)
    pc = eng.cost_tables(ex, cost, sw)[0]
    rec = {"fabric": "fat_tree_k48", "workload": workload, "split": split, "V": int(csr.V),
           "E": int(csr.E), "rows": n, "flows": int(rows.shape[0]), "demand": int(mult.sum()),
           "block_bytes": float(block), "max_epochs": max_epochs, "reps": reps}
    run = lambda timing: eng.ecmp_fair_times(ex, cost, pc, rows, srcs, mult, nbytes, cap,  # noqa
                                             None, split, max_epochs, timing=timing)
    got = run(False)
    rec["kernel"] = eng.ctx.last_kernel()
    rec["launches"] = eng.ctx.last_launches()
    rec["epochs"] = int(got[4].shape[0])
    rec["complete"] = not bool((got[1] == -2).any())
    rec["epoch_rounds"] = [int(x) for x in got[5]]
    rec["rounds"] = int(got[5].sum())
    rec["steps"] = int((got[5].astype(np.int64) + 2).sum()) + 1
    assert rec["launches"] == EN.fair_times_launches(got[5])
    want, _ = per_epoch_loop(eng, ex, cost, pc, rows, srcs, mult, nbytes, cap, split, max_epochs)
    worst = 0.0
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        if g.dtype != np.float64:
            assert np.array_equal(g, w)                   # epochs, every flow's epoch, rounds
            continue
        assert np.allclose(g, w, rtol=TOL, atol=0)
        ok = np.isfinite(w) & (w != 0)
        if ok.any():
            worst = max(worst, float(np.max(np.abs(g[ok] - w[ok]) / w[ok])))
    rec["max_rel_dev_vs_per_epoch_loop"] = worst
    live = np.isfinite(got[2]) & (got[2] > 0)
    rec["step_time"] = float((nbytes[live] / got[2][live]).max())
    fin = got[0][np.isfinite(got[0])]
    rec["makespan"] = float(fin.max()) if rec["complete"] else None
    rec["makespan_equals_step_time"] = rec["makespan"] == rec["step_time"]
    last = rec["epochs"] - 1
    rec["rows_live_in_last_epoch"] = round(
        float(np.unique(rows[(got[1] >= last) | (got[1] == -2)]).shape[0]) / n, 4) \
        if rec["epochs"] else 0.0
    k_new, c_new, k_old, c_old = [], [], [], []
    for _ in range(reps):
        t = time.perf_counter()
        _, ms = per_epoch_loop(eng, ex, cost, pc, rows, srcs, mult, nbytes, cap, split, max_epochs)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecmp_fair_times_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-epochs", type=int, default=64)
    ap.add_argument("--bytes", type=float, default=1048576.0, help="the block, bytes per host pair")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 alternated repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    fabric = T.fat_tree(48)
    eng = EN.RouteEngine(0)
    try:
        for workload in ("equal", "mixed"):
            for split in EN.SPLITS:
                line = json.dumps(bench_case(eng, fabric, workload, split, a.reps, a.max_epochs,
                                             a.bytes))
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
