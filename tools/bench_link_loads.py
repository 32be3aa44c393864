#!/usr/bin/env python
"""Link loads of the all-host-pairs demand: sdnr_link_loads against what the
engine offered before it -- RouteEngine.expand of the same switch pairs
followed by a weighted histogram of the entries on the host.

One GPU, the default-route rows of every host-bearing switch resident
(1,152 on the k=48 fat-tree).  Both paths are warmed up, their loads are
compared for equality, then they are timed in alternation with the host
clock around work that ends in a device synchronise (both return host
arrays).  One JSON line per fabric goes to --out; the fat-tree line carries
the comparison, the dragonfly and torus lines (deep trees) are for the
record: their baseline is skipped when its entries would not fit.

    python tools/bench_link_loads.py --out profiles/link_loads_k48.jsonl
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

MAX_BASELINE_ENTRIES = 400 << 20             # entries the baseline may expand in all
CHUNK_ENTRIES = 64 << 20                     # ... and per expand call


def demand(fabric, csr):
    hv, _ = fabric.host_table()
    hc = np.bincount(hv, minlength=csr.V).astype(np.int64)
    srcs = np.nonzero(hc)[0]
    n = srcs.shape[0]
    rows = np.repeat(np.arange(n), n)
    dsts = np.tile(srcs, n)
    keep = srcs[rows] != dsts                            # n * (n - 1) ordered switch pairs
    rows, dsts = rows[keep], dsts[keep]
    w = (hc[srcs][rows] * hc[dsts]).astype(np.uint64)
    return srcs, rows, dsts, w


def baseline_fn(eng, ex, tabs, rows, dsts, w, lens, stride):
    """expand + weighted bincount over switch * stride + port, in row chunks
    of at most CHUNK_ENTRIES entries (chunk bounds fixed beforehand)."""
    n = rows.shape[0]
    starts = np.concatenate([[0], np.flatnonzero(np.diff(rows)) + 1])   # the pairs are row-sorted
    per_row = np.add.reduceat(lens, starts)
    cuts, acc = [0], 0
    for k, e in enumerate(per_row.tolist()):
        if acc and acc + e > CHUNK_ENTRIES:
            cuts.append(int(starts[k]))
            acc = 0
        acc += e
    cuts.append(n)
    last = np.full(n, stride - 1, np.int32)              # a port no link uses: the last hop's bin
    V = ex.csr.V

    def run():
        hist = np.zeros(V * stride, np.float64)
        for a, b in zip(cuts, cuts[1:]):
            off, sw, hp = eng.expand(ex, tabs, rows[a:b], dsts[a:b], last[a:b])
            key = sw.astype(np.int64) * stride + hp
            hist += np.bincount(key, weights=np.repeat(w[a:b].astype(np.float64), np.diff(off)),
                                minlength=V * stride)
        return hist
    return run, len(cuts) - 1


def bench(name, fabric, reps, out):
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    eng = EN.RouteEngine(0)
    srcs, rows, dsts, w = demand(fabric, csr)
    par, prt, hop = eng.dfs_tables(ex, srcs)
    layout = EN.tree_layout(csr)
    tree = par if layout == EN.INT32 else eng.pack_trees(ex, par, prt, layout)
    hp = EN._host(hop)
    lens = hp[rows, dsts].astype(np.int64) + 1
    entries = int(lens.sum())
    rec = {"fabric": name, "V": int(csr.V), "E": int(csr.E), "rows": int(srcs.shape[0]),
           "switch_pairs": int(rows.shape[0]), "host_pairs": int(w.sum()),
           "tree_depth_max": int(hp.max()), "baseline_entries": entries, "layout": layout,
           "reps": reps}

    def loads(timing=False):
        return eng.link_loads(ex, tree, layout, rows, dsts, w, timing=timing)

    got = loads()                                        # warm-up
    got = loads(timing=True)
    rec["kernel"] = eng.ctx.last_kernel()
    rec["kernel_ms"] = round(eng.ctx.last_kernel_ms(), 4)
    assert int(got.sum(dtype=np.uint64)) == int((w.astype(np.int64) * hp[rows, dsts]).sum())
    base = None
    if entries <= MAX_BASELINE_ENTRIES:
        stride = int(np.asarray(csr.port).max()) + 2
        base, calls = baseline_fn(eng, ex, (par, prt, hop), rows, dsts, w, lens, stride)
        hist = base()                                    # warm-up
        rp = np.asarray(csr.row_ptr, np.int64)
        ekey = np.repeat(np.arange(csr.V, dtype=np.int64), np.diff(rp)) * stride + \
            np.asarray(csr.port, np.int64)
        assert len(set(ekey.tolist())) == csr.E, "two links of a switch share a port"
        assert np.array_equal(hist[ekey].astype(np.uint64), got), "the two paths disagree"
        rec["baseline_expand_calls"] = calls
        rec["loads_equal"] = True
    t_new, t_old = [], []
    for _ in range(reps):                                # alternated repetitions
        t = time.perf_counter()
        loads()
        t_new.append(time.perf_counter() - t)
        if base is not None:
            t = time.perf_counter()
            base()
            t_old.append(time.perf_counter() - t)
    rec["link_loads_ms"] = [round(x * 1e3, 3) for x in t_new]
    rec["link_loads_median_ms"] = round(float(np.median(t_new)) * 1e3, 3)
    if base is not None:
        rec["baseline_ms"] = [round(x * 1e3, 3) for x in t_old]
        rec["baseline_median_ms"] = round(float(np.median(t_old)) * 1e3, 3)
        rec["ratio_median"] = round(float(np.median(t_old) / np.median(t_new)), 2)
        rec["faster_in_every_rep"] = bool(all(a < b for a, b in zip(t_new, t_old)))
    else:
        rec["baseline_ms"] = None                        # not measured: too many entries
    eng.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_loads_k48.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="", help="comma-separated fabric names")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 alternated repetitions")
    fabrics = [("fat_tree_k48", lambda: T.fat_tree(48)),
               ("dragonfly_a16_h8_p8", lambda: T.dragonfly(16, 8, 8)),
               ("torus_16x16x16", lambda: T.torus3d(16, 16, 16))]
    only = set(x for x in a.only.split(",") if x)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    for name, make in fabrics:
        if not only or name in only:
            bench(name, make(), a.reps, a.out)


if __name__ == "__main__":
    main()
