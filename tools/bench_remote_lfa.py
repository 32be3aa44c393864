#!/usr/bin/env python
"""Remote loop-free alternates of every link: sdnr_remote_lfa against its two
yardsticks -- sdnr_lfa_tables' link-protecting kernel over all V destination
rows (the other all-pairs pass over the same table and CSR, in the same
process) and the numpy restatement engine.remote_lfa_host.

One GPU; the k=48 fat-tree and the dragonfly a16 h8 p8, every vertex a unit;
two cost sets each, as tools/bench_lfa_tables.py: unit costs, and every link at
the first 24 (fat-tree) or 16 (dragonfly) vertices at cost 2.  Per fabric and
cost set the all-pairs table is computed on the device (sdnr_cost_tables), the
out-links of 64 evenly spread vertices are compared with the restatement
(array_equal), then
  * the main kernel (the SDNR_TIMING event pair) and the yardstick's main
    kernel are timed alternately, the median of --reps each;
  * the transpose is the device time of the whole call (events on the call's
    stream around it) minus the main kernel's;
  * the whole RouteEngine.remote_lfa call is timed on the host clock (it ends
    in a device synchronise and copies its [E] outputs back);
  * engine.remote_lfa_host is timed on the 64 vertices and scaled to V;
  * the coverage figures come from the tables of the device.
--variants (a diagnostic build named by SDNROUTE_LIB) alternates the main
kernel with the alternatives of VARIANTS: no pruning by the lower bound, LDS
tiles of 64, 32, 24, 8 and 0 slots, and no tile at 4 and 2 workgroups per CU;
each one's settings, kernel name and grid are recorded beside its times.  No
time is a pass condition.  One JSON line per fabric and cost set
goes to --out.

    python tools/bench_remote_lfa.py --out profiles/remote_lfa_k48.jsonl
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
from bench_lfa_tables import cost_sets, fabrics, med, note   # noqa: E402

HOST_VERTS = 64
VARIANTS = (("noprune", {"SDNROUTE_RLFA_NOPRUNE": "1"}),
            ("tile64", {"SDNROUTE_RLFA_TILE": "64"}),
            ("tile32", {"SDNROUTE_RLFA_TILE": "32"}),
            ("tile24", {"SDNROUTE_RLFA_TILE": "24"}),
            ("tile8", {"SDNROUTE_RLFA_TILE": "8"}),
            ("tile0", {"SDNROUTE_RLFA_TILE": "0"}),
            ("tile0_4_per_cu", {"SDNROUTE_RLFA_TILE": "0", "SDNROUTE_RLFA_PER_CU": "4"}),
            ("tile0_2_per_cu", {"SDNROUTE_RLFA_TILE": "0", "SDNROUTE_RLFA_PER_CU": "2"}))


def bench(name, fabric, cname, cost, reps, out, variants):
    import torch
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    V, E = int(csr.V), int(csr.E)
    deg = np.diff(csr.row_ptr).astype(np.int64)
    src = np.repeat(np.arange(V), deg)
    eng = EN.RouteEngine(0)
    ids = np.arange(V, dtype=np.int32)
    rec = {"fabric": name, "costs": cname, "V": V, "E": E, "units": V, "reps": reps,
           "max_degree": int(deg.max()), "tests": int((deg * deg).sum()) * V}

    d_P, d_nh = eng.cost_tables(ex, cost, ids)[:2]          # upload + warm-up
    P = d_P.cpu().numpy().view(np.uint32)
    verts = np.unique(np.linspace(0, V - 1, HOST_VERTS).astype(np.int64))

    # correctness on the sampled vertices, and the host yardstick
    t = time.perf_counter()
    want = EN.remote_lfa_host(csr, cost, P, verts)
    host_ms = (time.perf_counter() - t) * 1e3
    got = eng.remote_lfa(ex, cost, d_P, verts)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    rec["kernel"] = eng.ctx.last_kernel()
    rec["host_restatement_ms_%d_vertices" % verts.shape[0]] = round(host_ms, 2)
    rec["host_restatement_ms_scaled_to_V"] = round(host_ms * V / verts.shape[0], 1)

    stream = torch.cuda.Stream(eng.dev)                     # the timed calls' stream
    d_ids = torch.from_numpy(ids).to(eng.dev)
    r_out = [torch.empty(E, dtype=torch.int32, device=eng.dev) for _ in range(3)] + \
            [torch.empty(E, dtype=torch.int64, device=eng.dev),
             torch.empty(E, dtype=torch.uint8, device=eng.dev),
             torch.empty((V, 4), dtype=torch.int32, device=eng.dev)]
    l_out = (torch.empty((V, V), dtype=torch.int32, device=eng.dev),
             torch.empty((V, V), dtype=torch.int32, device=eng.dev),
             torch.empty((V, V), dtype=torch.uint8, device=eng.dev),
             torch.empty((V, 4), dtype=torch.int32, device=eng.dev))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def remote():
        """(main kernel ms, whole call ms by events, grid) of one call."""
        torch.cuda.synchronize(eng.dev)
        e0.record(stream)
        eng.ctx.remote_lfa_device(d_P.data_ptr(), d_ids.data_ptr(), V,
                                  *(o.data_ptr() for o in r_out), timing=True)
        e1.record(stream)
        e1.synchronize()
        eng.ctx.synchronize()
        return eng.ctx.last_kernel_ms(), e0.elapsed_time(e1), eng.ctx.last_grid()

    eng.ctx.set_stream(stream.cuda_stream)
    ks, totals, ys = [], [], []
    vs = {v: [] for v, _ in variants}
    ref = None
    with torch.cuda.stream(stream):
        for rep in range(reps + 1):                         # the first round warms up
            k, total, grid = remote()
            if ref is None:
                ref = [o.cpu().numpy().copy() for o in r_out]
            eng.ctx.lfa_tables_device(d_P.data_ptr(), d_ids.data_ptr(), V,
                                      *(o.data_ptr() for o in l_out), link_only=True, timing=True)
            eng.ctx.synchronize()
            y = eng.ctx.last_kernel_ms()
            rec["yardstick_kernel"] = eng.ctx.last_kernel()
            for v, env in variants:
                os.environ.update(env)
                vk, _, vgrid = remote()
                rec["kernel_" + v] = eng.ctx.last_kernel()
                rec["grid_" + v] = int(vgrid)
                rec["settings_" + v] = env
                for key in env:
                    del os.environ[key]
                if rep == 0:                                # the variants compute the same tables
                    for o, r in zip(r_out, ref):
                        assert np.array_equal(o.cpu().numpy(), r), v
                else:
                    vs[v].append(vk)
            if rep:
                ks.append(k)
                totals.append(total)
                ys.append(y)
    eng.ctx.set_stream(None)
    rec["grid"] = int(grid)
    rec["kernel_ms"] = [round(x, 4) for x in ks]
    rec["kernel_median_ms"] = med(ks)
    rec["transpose_median_ms"] = med(np.asarray(totals) - np.asarray(ks))
    rec["yardstick_lfa_tables_link_kernel_ms"] = [round(x, 4) for x in ys]
    rec["yardstick_lfa_tables_link_kernel_median_ms"] = med(ys)
    rec["kernel_ratio_remote_lfa_over_lfa_tables_link"] = round(
        float(np.median(ks)) / float(np.median(ys)), 3)
    for v, _ in variants:
        rec["kernel_ms_" + v] = [round(x, 4) for x in vs[v]]
        rec["kernel_median_ms_" + v] = med(vs[v])

    # the whole engine call, host clock
    walls = []
    for rep in range(reps + 1):
        t = time.perf_counter()
        full = eng.remote_lfa(ex, cost, d_P)
        if rep:
            walls.append((time.perf_counter() - t) * 1e3)
    for a, r in zip(full[:3] + (full[3].view(np.int64), full[4], full[5].view(np.int32)), ref):
        assert np.array_equal(a, r)
    rec["call_wall_ms"] = [round(x, 3) for x in walls]
    rec["call_wall_median_ms"] = med(walls)
    rec["wall_ratio_call_over_host_restatement"] = round(
        float(np.median(walls)) / (host_ms * V / verts.shape[0]), 6)

    # coverage: the primaries without a loop-free alternate whose link has a repair
    kind = full[4]
    lk = l_out[2].cpu().numpy()
    nh = d_nh.cpu().numpy()
    dd, ss = np.nonzero((nh >= 0) & ((lk & 1) == 0))
    e = np.searchsorted(src * V + np.asarray(csr.col, np.int64),
                        ss.astype(np.int64) * V + nh[dd, ss])
    prim, bare, remote_b = int((nh >= 0).sum()), int(dd.shape[0]), int((kind[e] & 1).sum())
    tot = full[5].astype(np.int64).sum(0)
    rec.update({"primaries": prim, "primaries_without_lfa": bare, "remote_backups": remote_b,
                "coverage_lfa": round((prim - bare) / prim, 4),
                "coverage_with_remote": round((prim - bare + remote_b) / prim, 4),
                "links": int(tot[0]), "links_repaired": int(tot[1]), "links_plain": int(tot[2]),
                "links_per_link_lfa": int(tot[3]),
                "tunnel_cost_max": int(full[3].max()) if E else 0})
    note(name, cname, "kernel ms", rec["kernel_median_ms"], "transpose ms",
         rec["transpose_median_ms"], "lfa<link> ms",
         rec["yardstick_lfa_tables_link_kernel_median_ms"], "call ms", rec["call_wall_median_ms"],
         {v: rec["kernel_median_ms_" + v] for v, _ in variants})
    eng.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remote_lfa_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--variants", action="store_true",
                    help="alternate the kernel's measured alternatives (SDNROUTE_LIB names a "
                         "diagnostic build)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    if a.variants and "SDNROUTE_LIB" not in os.environ:
        ap.error("--variants needs a diagnostic build named by SDNROUTE_LIB")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    for name, fabric, first in fabrics():
        for cname, cost in cost_sets(fabric.csr(), first):
            bench(name, fabric, cname, cost, a.reps, a.out, VARIANTS if a.variants else ())


if __name__ == "__main__":
    main()
