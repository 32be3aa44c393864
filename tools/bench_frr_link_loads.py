#!/usr/bin/env python
"""Fast-reroute what-if loads: sdnr_frr_link_loads over a chunk of the N-1
cable failures against what the library offered for the same question before
it -- next-hop rows patched on the host and one sdnr_link_loads
(SDNR_LOADS_TO_ROOT) call per scenario.

One GPU; the k=48 fat-tree and the dragonfly a16 h8 p8, unit costs, the
all-host-pairs demand (one pair per ordered pair of host-bearing switches,
weighted by the host counts), node-protecting alternates.  Per fabric:
  * the tables come from the device (sdnr_cost_tables, sdnr_lfa_tables);
  * the scenarios are --chunk cables spread evenly over cable_failures()' list
    (both directions of each);
  * before anything is timed, --sample of them (scaled to the chunk) are
    answered the old way and compared for equality with the planes of one
    sdnr_frr_link_loads call.  The old way has no notion of a dropped pair --
    loads.hip would load the links up to the switch that drops --, so the pairs
    the new call reports undelivered get weight 0 there;
  * then, alternated, --reps times: the whole chunk through
    sdnr_frr_link_loads (item kernel by SDNR_TIMING, every kernel of the call
    by device events around it, RouteEngine.frr_link_loads(planes=False) on
    the host clock) and ONE sampled scenario the old way (loads.hip's kernel
    by SDNR_TIMING; patching, upload and call on the host clock);
  * sdnr_failure_ecmp_link_loads' kernel time per scenario on the sample, as
    context: the state after the controller has re-routed.
No time is a pass condition.  One JSON line per fabric goes to --out.

    python tools/bench_frr_link_loads.py --out profiles/frr_link_loads_k48.jsonl
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


def fabrics():
    return [("fat_tree_k48", T.fat_tree(48)), ("dragonfly_a16_h8_p8", T.dragonfly(16, 8, 8))]


def stats(ts, nd=4):
    ts = np.asarray(ts, np.float64)
    return {"median": round(float(np.median(ts)), nd), "min": round(float(ts.min()), nd),
            "max": round(float(ts.max()), nd)}


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def cables(csr):
    """cable_failures() from the CSR: per connected unordered switch pair, the
    edge ids of its directions, ascending."""
    u = np.repeat(np.arange(int(csr.V)), np.diff(csr.row_ptr))
    v = np.asarray(csr.col, np.int64)
    key = np.minimum(u, v) * int(csr.V) + np.maximum(u, v)
    order = np.argsort(key, kind="stable")
    cut = np.nonzero(np.diff(key[order]))[0] + 1
    return [np.sort(g).astype(np.int32) for g in np.split(order, cut)], u, v


def patched_rows(nh, backup, failed, u, v, keys):
    """nh with the scenario applied on the host: the old way's input."""
    V = nh.shape[1]
    rows = nh.copy()
    down = set((u[failed] * V + v[failed]).tolist())
    for x, n in zip(u[failed].tolist(), v[failed].tolist()):
        hit = np.nonzero(nh[:, x] == n)[0]
        b = backup[hit, x].astype(np.int64)
        ok = (b >= 0) & ~np.isin(x * V + b, list(down))
        rows[hit, x] = np.where(ok, b, -1)
    return rows


def bench(name, fabric, chunk, sample, reps, out):
    import torch
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    V, E = int(csr.V), int(csr.E)
    eng = EN.RouteEngine(0)
    cost = np.ones(E, np.uint32)
    hv_all = np.asarray(fabric.host_table()[0], np.int64)
    dsts, hc = np.unique(hv_all, return_counts=True)
    nrows = int(dsts.shape[0])
    rows = np.tile(np.arange(nrows), nrows)
    sv = np.repeat(dsts, nrows)
    w = (np.repeat(hc, nrows) * (np.tile(hc, nrows) - (sv == dsts[rows]))).astype(np.uint64)

    d_P = eng.cost_tables(ex, cost, np.arange(V, dtype=np.int32))[0]
    d_nh = eng.cost_tables(ex, cost, dsts.astype(np.int32))[1].contiguous()
    d_bk = eng.lfa_tables(ex, cost, d_P, dsts.astype(np.int32))[0].contiguous()
    del d_P
    nh, backup = d_nh.cpu().numpy(), d_bk.cpu().numpy()
    keys, _ = EN._edge_keys_host(csr)

    every, u, v = cables(csr)
    chunk = min(chunk, len(every))
    scen = [every[i] for i in np.unique(np.linspace(0, len(every) - 1, chunk).astype(np.int64))]
    chunk = len(scen)
    sample = max(1, min(sample, chunk))
    picks = np.unique(np.linspace(0, chunk - 1, sample).astype(np.int64)).tolist()
    rec = {"fabric": name, "V": V, "E": E, "rows": nrows, "pairs": int(rows.shape[0]),
           "cables": len(every), "chunk": chunk, "sample": len(picks), "reps": reps}

    # equality first: the sampled scenarios, the old way against the planes
    load, stat, status, peak, pedge, items = eng.frr_link_loads(
        ex, d_nh, d_bk, dsts, rows, sv, w, [scen[k] for k in picks])
    assert not stat[:, 2].any(), "a single cable never loops"
    for j, k in enumerate(picks):
        tree = torch.from_numpy(patched_rows(nh, backup, scen[k], u, v, keys)).to(eng.dev)
        wk = np.where((status[j] == 1) | (status[j] == 2), w, 0).astype(np.uint64)
        old = eng.link_loads(ex, tree, EN.INT32, rows, sv, wk, to_root=True)
        assert np.array_equal(load[j], old), (name, k)
        assert int(peak[j]) == int(old.max()) and int(pedge[j]) == int(old.argmax())
    rec["equal_on_sample"] = True
    rec["sample_repaired_weight"] = [int(x) for x in stat[:, 0]]
    rec["sample_dropped_weight"] = [int(x) for x in stat[:, 1]]
    del load, status

    # the raw call's buffers, for the device-event timing
    order, off, s, ww = EN._pairs_for_device(rows, nrows, sv, V, w, "bench", "dsts")
    d_dst = torch.from_numpy(dsts.astype(np.int32)).to(eng.dev)
    d_off, d_src, d_w = eng._upload_pairs(off, s, ww)
    soff = np.zeros(chunk + 1, np.int64)
    np.cumsum([a.shape[0] for a in scen], out=soff[1:])
    d_soff = torch.from_numpy(soff).to(eng.dev)
    d_edges = torch.from_numpy(np.concatenate(scen + [np.zeros(1, np.int32)])).to(eng.dev)
    d_load = torch.zeros((chunk, E), dtype=torch.int64, device=eng.dev)
    d_stat = torch.zeros((chunk, 4), dtype=torch.int64, device=eng.dev)
    d_peak = torch.zeros(chunk, dtype=torch.int64, device=eng.dev)
    d_pedge = torch.zeros(chunk, dtype=torch.int32, device=eng.dev)
    stream = torch.cuda.Stream(eng.dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    ks, totals, walls, yk, yw, ypatch = [], [], [], [], [], []
    for rep in range(reps + 1):                             # the first round warms up
        eng.ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_load.zero_()
            d_stat.zero_()
            torch.cuda.synchronize(eng.dev)
            e0.record(stream)
            eng.ctx.frr_link_loads_device(
                d_dst.data_ptr(), d_nh.data_ptr(), d_bk.data_ptr(), nrows, d_off.data_ptr(),
                d_src.data_ptr(), d_w.data_ptr(), chunk, d_soff.data_ptr(), d_edges.data_ptr(),
                d_load.data_ptr(), d_stat.data_ptr(), 0, d_peak.data_ptr(), d_pedge.data_ptr(),
                timing=True)
            e1.record(stream)
            e1.synchronize()
            eng.ctx.synchronize()
        k_ms, tot_ms = eng.ctx.last_kernel_ms(), e0.elapsed_time(e1)
        n_items = eng.ctx.last_frr_items()
        eng.ctx.set_stream(None)
        t = time.perf_counter()
        got = eng.frr_link_loads(ex, d_nh, d_bk, dsts, rows, sv, w, scen, planes=False,
                                 table_budget=chunk * (8 * E + rows.shape[0]))
        wall = (time.perf_counter() - t) * 1e3
        assert got[5] == n_items
        # one scenario the old way
        k = picks[rep % len(picks)]
        t = time.perf_counter()
        tree_h = patched_rows(nh, backup, scen[k], u, v, keys)
        t1 = time.perf_counter()
        tree = torch.from_numpy(tree_h).to(eng.dev)
        eng.link_loads(ex, tree, EN.INT32, rows, sv, w, to_root=True, timing=True)
        t2 = time.perf_counter()
        y_ms = eng.ctx.last_kernel_ms()
        if rep:
            ks.append(k_ms)
            totals.append(tot_ms)
            walls.append(wall)
            yk.append(y_ms)
            yw.append((t2 - t1) * 1e3)
            ypatch.append((t1 - t) * 1e3)
    rec["kernel"] = "frr_items_kernel<lds>"
    rec["yardstick_kernel"] = eng.ctx.last_kernel()
    rec["items_affected"] = int(n_items)
    rec["items_all"] = chunk * nrows
    rec["items_share"] = round(n_items / float(chunk * nrows), 5)
    rec["item_kernel_ms_chunk"] = stats(ks)
    rec["all_kernels_ms_chunk"] = stats(totals)
    rec["call_wall_ms_chunk_no_planes"] = stats(walls, 2)
    rec["yardstick_kernel_ms_per_scenario"] = stats(yk)
    rec["yardstick_upload_and_call_wall_ms_per_scenario"] = stats(yw, 2)
    rec["yardstick_host_patch_ms_per_scenario"] = stats(ypatch, 2)
    rec["item_kernel_ms_per_scenario"] = round(float(np.median(ks)) / chunk, 5)
    rec["all_kernels_ms_per_scenario"] = round(float(np.median(totals)) / chunk, 5)
    rec["ratio_all_kernels_per_scenario_over_yardstick_kernel"] = round(
        float(np.median(totals)) / chunk / float(np.median(yk)), 4)
    rec["ratio_call_wall_per_scenario_over_yardstick_wall"] = round(
        float(np.median(walls)) / chunk / float(np.median(yw)), 4)

    # context: the loads after the controller has re-routed, the same sample
    fs = []
    some = [scen[k] for k in picks[:4]]
    for rep in range(3):
        eng.failure_ecmp_link_loads(ex, cost, dsts, rows, sv, w, some, timing=True)
        if rep:
            fs.append(eng.ctx.last_kernel_ms() / len(some))
    rec["failure_link_loads_kernel_ms_per_scenario"] = stats(fs)
    note(name, "items", n_items, "of", chunk * nrows, "item kernel ms", rec["item_kernel_ms_chunk"],
         "all kernels ms", rec["all_kernels_ms_chunk"], "old way kernel ms / scenario",
         rec["yardstick_kernel_ms_per_scenario"])
    eng.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frr_link_loads_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--sample", type=int, default=8)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    for name, fabric in fabrics():
        bench(name, fabric, a.chunk, a.sample, a.reps, a.out)


if __name__ == "__main__":
    main()
