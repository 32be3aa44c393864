#!/usr/bin/env python
"""Loop-free alternate tables of every destination: sdnr_lfa_tables (node- and
link-protecting) against its two yardsticks -- sdnr_cost_tables' kernel for
the same V rows (it reads the same CSR into the same kind of table: the natural
floor) and the numpy restatement engine.lfa_tables_host.

One GPU; the k=48 fat-tree and the dragonfly a16 h8 p8, all V destinations;
two cost sets each: unit costs, and every link at the first 24 (fat-tree: the
first core group, as bench_failure_link_loads.py) or 16 (dragonfly: the first
group's routers) vertices at cost 2.  Per fabric and cost set the all-pairs
table is computed on the device (sdnr_cost_tables), 64 evenly spread rows of
both flag settings are compared with the restatement (array_equal), then
  * the main kernel (the SDNR_TIMING event pair) and sdnr_cost_tables' kernel
    are timed alternately, the median of --reps each;
  * the pre-pass is the device time of the whole call (events on the call's
    stream around it) minus the main kernel's;
  * the whole RouteEngine.lfa_tables call is timed on the host clock (it ends
    in a device synchronise and allocates its [V, V] outputs);
  * engine.lfa_tables_host is timed on the 64 rows and scaled to V.
No time is a pass condition.  One JSON line per fabric and cost set goes to
--out.

    python tools/bench_lfa_tables.py --out profiles/lfa_tables_k48.jsonl
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

HOST_ROWS = 64


def fabrics():
    return [("fat_tree_k48", T.fat_tree(48), 24), ("dragonfly_a16_h8_p8", T.dragonfly(16, 8, 8), 16)]


def cost_sets(csr, first):
    esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    at = (esrc < first) | (np.asarray(csr.col) < first)
    return [("unit", np.ones(int(csr.E), np.uint32)),
            ("first_%d_vertices_at_cost_2" % first, np.where(at, 2, 1).astype(np.uint32))]


def med(ts):
    return round(float(np.median(ts)), 4)


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def bench(name, fabric, cname, cost, reps, out):
    import torch
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    V, E = int(csr.V), int(csr.E)
    deg = np.diff(csr.row_ptr).astype(np.int64)
    eng = EN.RouteEngine(0)
    ids = np.arange(V, dtype=np.int32)
    rec = {"fabric": name, "costs": cname, "V": V, "E": E, "rows": V, "reps": reps,
           "max_degree": int(deg.max()), "nn_entries": int((deg * deg).sum())}

    d_P = eng.cost_tables(ex, cost, ids)[0]                 # upload + warm-up
    P = d_P.cpu().numpy().view(np.uint32)
    rows = np.unique(np.linspace(0, V - 1, HOST_ROWS).astype(np.int64))
    stream = torch.cuda.Stream(eng.dev)                     # the timed calls' stream
    d_ids = torch.from_numpy(ids).to(eng.dev)
    outs = (torch.empty((V, V), dtype=torch.int32, device=eng.dev),
            torch.empty((V, V), dtype=torch.int32, device=eng.dev),
            torch.empty((V, V), dtype=torch.uint8, device=eng.dev),
            torch.empty((V, 4), dtype=torch.int32, device=eng.dev))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    for tag, link_only in (("node", False), ("link", True)):
        # correctness on the sampled rows, and the host yardstick
        t = time.perf_counter()
        want = EN.lfa_tables_host(csr, cost, P, rows, link_only)
        host_ms = (time.perf_counter() - t) * 1e3
        got = eng.lfa_tables(ex, cost, d_P, rows, link_only=link_only)
        for a, b in zip(got[:3], want[:3]):
            assert np.array_equal(a.cpu().numpy(), b), tag
        assert np.array_equal(got[3], want[3]), tag
        rec["kernel_" + tag] = eng.ctx.last_kernel()
        rec["host_restatement_ms_%d_rows_%s" % (rows.shape[0], tag)] = round(host_ms, 2)
        rec["host_restatement_ms_scaled_to_V_" + tag] = round(host_ms * V / rows.shape[0], 1)

        # kernel and pre-pass (device events), alternated with the yardstick
        eng.ctx.set_stream(stream.cuda_stream)
        ks, totals, ys = [], [], []
        with torch.cuda.stream(stream):
            for rep in range(reps + 1):                         # the first round warms up
                torch.cuda.synchronize(eng.dev)
                e0.record(stream)
                eng.ctx.lfa_tables_device(d_P.data_ptr(), d_ids.data_ptr(), V,
                                          *(o.data_ptr() for o in outs), link_only=link_only,
                                          timing=True)
                e1.record(stream)
                e1.synchronize()
                eng.ctx.synchronize()
                k = eng.ctx.last_kernel_ms()
                eng.cost_tables(ex, cost, ids, timing=True)
                y = eng.ctx.last_kernel_ms()
                if rep:
                    ks.append(k)
                    totals.append(e0.elapsed_time(e1))
                    ys.append(y)
        eng.ctx.set_stream(None)
        rec["yardstick_kernel"] = eng.ctx.last_kernel()
        rec["kernel_ms_" + tag] = [round(x, 4) for x in ks]
        rec["kernel_median_ms_" + tag] = med(ks)
        rec["prepass_median_ms_" + tag] = med(np.asarray(totals) - np.asarray(ks))
        rec["yardstick_cost_tables_kernel_median_ms_" + tag] = med(ys)
        rec["kernel_ratio_lfa_over_cost_tables_" + tag] = round(float(np.median(ks)) /
                                                                float(np.median(ys)), 3)
        counts = outs[3].cpu().numpy().view(np.uint32).astype(np.int64).sum(0)

        # the whole engine call, host clock
        walls = []
        for rep in range(reps + 1):
            t = time.perf_counter()
            full = eng.lfa_tables(ex, cost, d_P, ids, link_only=link_only)
            if rep:
                walls.append((time.perf_counter() - t) * 1e3)
        assert np.array_equal(full[3].astype(np.int64).sum(0), counts)
        del full
        rec["call_wall_ms_" + tag] = [round(x, 3) for x in walls]
        rec["call_wall_median_ms_" + tag] = med(walls)
        rec["wall_ratio_call_over_host_restatement_" + tag] = round(
            float(np.median(walls)) / (host_ms * V / rows.shape[0]), 5)
        rec["primaries"] = int(counts[0])
        rec["backups_" + tag] = int(counts[1])
        rec["coverage_" + tag] = round(float(counts[1]) / float(counts[0]), 4)
        if not link_only:
            rec["node_protecting"] = int(counts[2])
            rec["node_coverage"] = round(float(counts[2]) / float(counts[0]), 4)
        rec["downstream_" + tag] = int(counts[3])
        note(name, cname, tag, "kernel ms", rec["kernel_median_ms_" + tag], "pre-pass ms",
             rec["prepass_median_ms_" + tag], "cost_tables ms",
             rec["yardstick_cost_tables_kernel_median_ms_" + tag], "call ms",
             rec["call_wall_median_ms_" + tag])
    eng.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lfa_tables_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    for name, fabric, first in fabrics():
        for cname, cost in cost_sets(fabric.csr(), first):
            bench(name, fabric, cname, cost, a.reps, a.out)


if __name__ == "__main__":
    main()
