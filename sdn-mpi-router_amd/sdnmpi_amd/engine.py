"""Route tables on the GPU and their expansion into fdb lists.

``RouteEngine`` owns one native context (``_native.Context``: one HIP device,
or several of one node, sharded by source) and the graph uploaded to it.
Tables stay in HBM: the engine returns them as torch tensors on the primary
device (torch is only the device-memory plumbing here) and ``TableCache``
keeps, per uploaded graph, the per-source DFS tables (default route,
reference ``_find_route_dfs``, ``sdnmpi/util/topology_db.py:59-84``) and the
per-destination shortest tables (``_find_routes_bfs``, :86-122) computed so
far, within a byte budget, in a fixed-capacity pool of compact rows:

* default route: one 4-byte tree word per vertex -- ``parent | port << 16``
  (V <= 65535, 16-bit ports: sdnr_dfs_tables_packed's layout) or ``parent |
  slot << 26`` (sdnr_dfs_tables_slots') -- plus the tree depth (u16 for
  V <= 65535, else int32): 6 bytes per entry where the int32 parent / port /
  hops tables take 12 (8 on fabrics above 65,535 switches);
* shortest route: u16 distance plus the next hop (u16 for V <= 65535): 4
  bytes per entry; the next hop's port is looked up in the CSR on demand.

Slots are taken from a free list and given back on eviction or when a graph
change invalidates the row; the pool is allocated once (min(budget rows, V)
rows) and no operation copies it, free slots hold all-unreached rows.  A single
``find_route`` copies back one table row (V entries, kept in a small host
cache), a batch is expanded on the device.  Expansion follows the
reference's ``_route_to_fdb`` (:127-138): one ``(dpid, out_port)`` per switch
on the path, the last one being the destination switch's host port or
``OFPP_LOCAL``.

The cache is storage-agnostic: an engine may hand back numpy arrays instead
(the CPU tests' oracle-backed double), and every array operation below
dispatches on the array type.
"""

import collections
import os

import numpy as np

from . import _native
from .graph import empty_csr

__all__ = ["RouteEngine", "TableCache", "tree_path", "expand_tree_paths",
           "shortest_paths_lex", "count_shortest_paths", "ECMP_LIMIT", "DEFAULT_TABLE_BUDGET", "tree_layout", "dfs_row_bytes",
           "sp_row_bytes", "link_loads_host", "ecmp_link_loads_host", "cost_tables_host",
           "check_link_costs", "COST_INF", "COST_MAX", "COST_LDS_MAX_V", "COST_LDS_B8_MAX_V",
           "cost_ecmp_link_loads_host", "least_cost_paths_lex", "count_least_cost_paths",
           "COST_ECMP_LDS_MAX_V", "FAILURE_LDS_MAX_V", "normalise_scenarios",
           "failure_ecmp_link_loads_host", "normalise_cost_scenarios",
           "whatif_ecmp_link_loads_host", "peak_utilisation", "lfa_tables_host", "LFA_MAX_V", "LFA_BACKUP",
           "frr_link_loads_host", "FRR_MAX_V",
           "LFA_DOWNSTREAM", "LFA_NODE", "widest_tables_host", "check_link_utilisation", "UTIL_MAX",
           "WIDEST_LDS_MAX_V", "WIDEST_LDS_B4_MAX_V", "WIDEST_LDS_B6_MAX_V", "fair_rates_host",
           "check_fair_flows", "FAIR_LDS_MAX_V", "FAIR_MULT_LIMIT", "ecmp_fair_rates_host",
           "ECMP_FAIR_LDS_MAX_V", "FAIR_TIE", "multicast_trees_host", "MCAST_LDS_BYTES",
           "multicast_maps_in_lds", "fair_times_host", "check_fair_bytes", "fair_times_launches",
           "FAIR_TIMES_BATCH", "ecmp_fair_times_host", "remote_lfa_host", "RLFA_REPAIR",
           "RLFA_PLAIN", "RLFA_LFA"]

# bytes of device tables one TableCache keeps per route mode before it
# evicts rows (SDNROUTE_TABLE_BUDGET overrides); the torus 32^3 default-route
# tables of every source take 6.4 GB in the pool, Jellyfish 100k's 80 GB
# Largest ECMP set either find_route(..., multiple=True) path builds; above
# it both raise MemoryError (the reference's enumeration runs out of memory
# long before).
ECMP_LIMIT = 1 << 40
DEFAULT_TABLE_BUDGET = int(os.environ.get("SDNROUTE_TABLE_BUDGET", str(24 << 30)))
HOST_ROW_CACHE = 256            # table rows kept on the host for find_route
COMPUTE_ROWS = 4096             # rows per engine call when filling the pool

PORT16, SLOT, INT32 = "port16", "slot", "int32"


# ------------------------------------------------------- array dispatch --

def _is_np(a):
    return isinstance(a, np.ndarray)


def _take(a, idx):
    """Rows ``idx`` (int64 numpy) of a table."""
    if a is None:
        return None
    if _is_np(a):
        return a[idx]
    import torch
    return a.index_select(0, torch.as_tensor(idx, dtype=torch.int64, device=a.device))


def _host(a):
    if a is None or _is_np(a):
        return a
    return a.cpu().numpy()


def _nbytes(a):
    if a is None:
        return 0
    return a.nbytes if _is_np(a) else a.element_size() * a.numel()


def _i64(a):
    return a.astype(np.int64) if _is_np(a) else a.to(dtype=_torch().int64)


def _torch():
    import torch
    return torch


# ------------------------------------------------------- compact layouts --

def tree_layout(csr):
    """4-byte tree layout the cache keeps default-route rows in."""
    V = csr.V
    port = np.asarray(csr.port)
    if V <= 0xFFFF and (port.size == 0 or (port.min() >= 0 and port.max() < 0xFFFF)):
        return PORT16
    if V < (1 << 26) and csr.max_degree() <= 63:
        return SLOT
    return INT32


def _hops_dtype(V):
    return "int16" if V <= 0xFFFF else "int32"


def _nh_dtype(V):
    return "int16" if V <= 0xFFFF else "int32"


def dfs_row_bytes(csr):
    """Bytes of one default-route row in the cache."""
    lay = tree_layout(csr)
    hb = 2 if csr.V <= 0xFFFF else 4
    return (4 + hb if lay != INT32 else 12) * csr.V


def sp_row_bytes(csr):
    return (2 + (2 if csr.V <= 0xFFFF else 4)) * csr.V


def _u16(a):
    """u16 values stored in int16 (0xFFFF: -1) as int64."""
    x = _i64(a) & 0xFFFF
    return (x - ((x == 0xFFFF) * 0x10000)) if _is_np(x) else x.masked_fill(x == 0xFFFF, -1)


class Wide(object):
    """Read view of a compact table: indexing returns int64 values (u16
    planes widened, 0xFFFF -> -1; tree words decoded to parents)."""

    def __init__(self, arr, kind):
        self.arr = arr
        self.kind = kind               # "u16" | "u16raw" | "int" | PORT16 | SLOT
        self.shape = arr.shape

    def __getitem__(self, idx):
        w = self.arr[idx]
        if self.kind == "u16":
            return _u16(w)
        if self.kind == "u16raw":                  # distances: 0xFFFF stays INF
            return _i64(w) & 0xFFFF
        if self.kind == "int":
            return _i64(w)
        return tree_parent(w, self.kind)


def tree_parent(w, layout):
    """Parents (int64, -1 unreached) of tree words (int32 storage)."""
    x = _i64(w) & 0xFFFFFFFF
    if layout == PORT16:
        p = x & 0xFFFF
        bad = p == 0xFFFF
    else:
        p = x & 0x3FFFFFF
        bad = x == 0xFFFFFFFF
    if _is_np(p):
        p[bad] = -1
        return p
    return p.masked_fill(bad, -1)


def tree_port(w, layout, row_ptr, port, parent=None):
    """Ports (int64, -1 for the root / unreached) of tree words.  Slot trees
    look the port up in the CSR (row_ptr / port arrays of the tree's type)."""
    x = _i64(w) & 0xFFFFFFFF
    if layout == PORT16:
        t = x >> 16
        return _where(t == 0xFFFF, -1, t)
    slot = x >> 26
    par = tree_parent(w, layout) if parent is None else parent
    none = (par < 0) | (slot == 63)
    if _is_np(x):
        pz = np.where(none, 0, par)
        idx = np.where(none, 0, row_ptr[pz] + slot)
        return np.where(none, -1, np.asarray(port, np.int64)[idx])
    pz = par.masked_fill(none, 0)
    idx = (row_ptr[pz] + slot).masked_fill(none, 0)
    return port[idx].to(x.dtype).masked_fill(none, -1)


def _empty_rows(a, n):
    """Uninitialised [n] + a.shape[1:] array of a's type (and device)."""
    if _is_np(a):
        return np.empty((n,) + tuple(a.shape[1:]), a.dtype)
    return _torch().empty((n,) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)


def _where(c, a, b):
    if _is_np(b):
        return np.where(c, a, b)
    return b.masked_fill(c, a)


def _edge_keys_host(csr):
    """(keys int64 ascending = x * V + col of every CSR entry, port int32)."""
    rp = np.asarray(csr.row_ptr, np.int64)
    keys = np.repeat(np.arange(csr.V, dtype=np.int64), np.diff(rp)) * csr.V + \
        np.asarray(csr.col, np.int64)
    return keys, np.asarray(csr.port, np.int32)


def _next_hop_port(nh, keys, port, V):
    """CSR port of edge (x, nh[r, x]) for every entry of an int64 next-hop
    block (-1 where nh < 0); numpy or device tensors."""
    if keys.shape[0] == 0:
        return nh * 0 - 1
    n = nh.shape[-1]
    if _is_np(nh):
        x = np.broadcast_to(np.arange(n, dtype=np.int64), nh.shape)
        ok = nh >= 0
        e = np.minimum(np.searchsorted(keys, np.where(ok, x * V + nh, 0)), keys.shape[0] - 1)
        return np.where(ok, port[e].astype(np.int64), -1)
    t = _torch()
    x = t.arange(n, dtype=t.int64, device=nh.device).expand_as(nh)
    ok = nh >= 0
    k = (x * V + nh).masked_fill(~ok, 0)
    e = t.searchsorted(keys, k).clamp_(max=keys.shape[0] - 1)
    return port[e].to(t.int64).masked_fill(~ok, -1)


def pack_host_tree(parent, port, csr, layout):
    """Host (numpy) tables -> tree words (int32 storage): the test double's
    counterpart of sdnr_tree_pack."""
    p = np.asarray(parent, np.int64)
    if layout == PORT16:
        t = (p & 0xFFFF) | ((np.asarray(port, np.int64) & 0xFFFF) << 16)
    else:
        V = csr.V
        rp = np.asarray(csr.row_ptr, np.int64)
        src = np.repeat(np.arange(V, dtype=np.int64), np.diff(rp))
        keys = src * V + np.asarray(csr.col, np.int64)
        v = np.broadcast_to(np.arange(V, dtype=np.int64), p.shape)
        ok = p >= 0
        e = np.searchsorted(keys, np.where(ok, p, 0) * V + v)
        slot = np.where(ok, e - rp[np.where(ok, p, 0)], 0)
        slot = np.where(p == v, 63, slot)
        t = np.where(ok, p | (slot << 26), 0xFFFFFFFF)
    return (t & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _pairs_by_row(rows, nrows):
    """(order, off): a stable order of the pairs by row and the int64
    [nrows + 1] offsets of each row's pairs in it (sdnr_link_loads' pair_off)."""
    if rows.shape[0] < 2 or bool((rows[1:] >= rows[:-1]).all()):
        order = slice(None)                              # already grouped by row
    else:
        order = np.argsort(rows, kind="stable")
    off = np.zeros(nrows + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=nrows), out=off[1:])
    return order, off


def _pairs_for_device(rows, nrows, verts, V, weights, what, table="the table"):
    """The pair list of a row-grouped entry point, pure numpy: ``(order, off,
    verts_i32, weights_u64_or_None)`` -- ``_pairs_by_row``'s order and offsets,
    the pairs' vertices in that order (int32, -1 for one outside [0, V)) and
    their weights in that order (None stays None).  A row outside [0, nrows)
    raises in the caller's name ``what``."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    if rows.size and (rows.min() < 0 or rows.max() >= nrows):
        raise ValueError("%s: a pair names a row outside %s" % (what, table))
    order, off = _pairs_by_row(rows, nrows)
    x = np.asarray(verts, np.int64).reshape(-1)[order]
    x = np.where((x < 0) | (x >= V), -1, x).astype(np.int32)
    if weights is not None:
        weights = np.ascontiguousarray(np.asarray(weights, np.uint64).reshape(-1)[order])
    return order, off, x, weights


def _unsorted(a, order):
    """``a`` (numpy, in ``_pairs_by_row``'s order along its last axis) back in
    the caller's order."""
    if isinstance(order, slice):
        return a
    back = np.empty_like(a)
    back[..., order] = a
    return back


def _ptr(a):
    """The device address of a tensor, 0 for None."""
    return a.data_ptr() if a is not None else 0


def _gather(a, r, c):
    """a[r[i], c[i]] of a [k, V] table (numpy or device tensor) as numpy."""
    if _is_np(a):
        return a[r, c]
    t = _torch()
    return a[t.as_tensor(r, dtype=t.int64, device=a.device),
             t.as_tensor(c, dtype=t.int64, device=a.device)].cpu().numpy()


def link_loads_host(csr, tree, layout, rows, dsts, weights=None, to_root=False):
    """numpy restatement of sdnr_link_loads (the CPU tests' engine double and
    an independent check of loads.hip): uint64 [E] loads of pairs (row
    ``rows[i]`` of ``tree``, switch ``dsts[i]``, weight ``weights[i]`` or 1).

    Deliberately not the kernel's algorithm: the tree depths are found first,
    then the demand is pushed to the parents one level at a time, deepest
    level first (``np.add.at``), so every vertex is final before it is
    passed on; the load of link parent(v) -> v (``to_root``: v -> parent) is
    what v passes on.  u64 sums wrap, as on the device."""
    V, E = int(csr.V), int(csr.E)
    load = np.zeros(E, np.uint64)
    rows = np.asarray(rows, np.int64)
    dsts = np.asarray(dsts, np.int64)
    if rows.size == 0 or E == 0:
        return load
    w = np.ones(rows.shape[0], np.uint64) if weights is None else np.asarray(weights, np.uint64)
    used, rix = np.unique(rows, return_inverse=True)
    words = np.asarray(tree)[used]
    if layout == INT32:
        par = words.astype(np.int64)
    else:
        par = tree_parent(words, layout)
    n = par.shape[0]
    vid = np.broadcast_to(np.arange(V, dtype=np.int64), par.shape)
    par = np.where((par < 0) | (par == vid), -1, par)      # no ancestor: root / unreached
    if (par >= V).any():
        raise ValueError("link_loads_host: a parent that is no vertex")
    # depth = number of ancestors, by pointer jumping
    depth = (par >= 0).astype(np.int64)
    jump = par.copy()
    for _ in range(max(1, V).bit_length() + 1):
        ok = jump >= 0
        if not ok.any():
            break
        jc = np.where(ok, jump, 0)
        depth = depth + np.where(ok, np.take_along_axis(depth, jc, 1), 0)
        jump = np.where(ok, np.take_along_axis(jump, jc, 1), -1)
    else:
        raise ValueError("link_loads_host: a row is not a tree")
    acc = np.zeros((n, V), np.uint64)
    ok = (dsts >= 0) & (dsts < V)
    np.add.at(acc, (rix[ok], dsts[ok]), w[ok])
    flat = np.argsort(depth, axis=None, kind="stable")
    cnt = np.bincount(depth.ravel())
    ends = np.cumsum(cnt)
    for lv in range(cnt.shape[0] - 1, 0, -1):              # deepest level first
        idx = flat[ends[lv] - cnt[lv]:ends[lv]]
        r, v = idx // V, idx % V
        np.add.at(acc, (r, par[r, v]), acc[r, v])
    r, v = np.nonzero((par >= 0) & (acc != 0))
    if r.size == 0:
        return load
    p = par[r, v]
    keys, _ = _edge_keys_host(csr)
    k = (v * V + p) if to_root else (p * V + v)
    e = np.minimum(np.searchsorted(keys, k), E - 1)
    if not np.array_equal(keys[e], k):
        raise ValueError("link_loads_host: a tree link the graph does not have")
    np.add.at(load, e, acc[r, v])
    return load


MCAST_LDS_BYTES = 32 * 1024     # csrc/common.h kMcastLdsBytes: the V- and E-bit maps' words in LDS


def multicast_maps_in_lds(V, E):
    """Whether sdnr_multicast_trees keeps a group's two bit maps in LDS."""
    return 4 * ((int(V) + 31) // 32 + (int(E) + 31) // 32) <= MCAST_LDS_BYTES


def multicast_trees_host(csr, tree, layout, root, mem_off, mem_row, mem_vertex, weights=None,
                         to_root=False):
    """numpy restatement of sdnr_multicast_trees (the CPU tests' engine double
    and what the GPU tests compare multicast.hip against): ``(reached uint8
    [nmem], ent_off int64 [ngroups + 1], ent_edge int32, load uint64 [E])``.

    Group g has root switch ``root[g]`` and the members ``(mem_row[i],
    mem_vertex[i])``, i in ``mem_off[g]:mem_off[g+1]``; its multicast tree is
    the set union of the links of its members' routes -- in a tree row of the
    root (``layout`` PORT16 / SLOT words or INT32 parents) the climb from the
    member to the root, links parent(x) -> x; with ``to_root`` the descent
    from the root along the member's own next-hop row (INT32), links x ->
    nh[x].  ``ent_edge[ent_off[g]:ent_off[g+1]]`` are the union's CSR edge ids,
    ascending; ``load[e]`` sums ``weights[g]`` (u64, None: 1; sums wrap) over
    the groups whose union holds e.  A member is reached when its route exists
    (its word is not none / ``nh[row][root] >= 0``) or it is the root itself;
    roots, rows and vertices outside their ranges are unreached and contribute
    nothing, repeated members count once.

    Deliberately not the kernel's algorithm: all walks advance together one
    hop per step, walkers that meet merge, the (group, link) pairs are
    de-duplicated at the end with ``np.unique``.  A row that is not a tree of
    the graph raises ValueError."""
    V, E = int(csr.V), int(csr.E)
    tree = np.asarray(tree)
    nrows = int(tree.shape[0]) if tree.ndim == 2 else 0
    root = np.asarray(root, np.int64).reshape(-1)
    mem_off = np.asarray(mem_off, np.int64).reshape(-1)
    row = np.asarray(mem_row, np.int64).reshape(-1)
    vert = np.asarray(mem_vertex, np.int64).reshape(-1)
    ng, nmem = root.shape[0], row.shape[0]
    if mem_off.shape[0] != ng + 1 or (ng and (mem_off[0] != 0 or mem_off[-1] != nmem)) or \
            (np.diff(mem_off) < 0).any() or vert.shape[0] != nmem:
        raise ValueError("multicast_trees_host: mem_off is not the offsets of the members")
    w = np.ones(ng, np.uint64) if weights is None else np.asarray(weights, np.uint64).reshape(-1)
    if w.shape[0] != ng:
        raise ValueError("multicast_trees_host: one weight per group")
    reached = np.zeros(nmem, np.uint8)
    load = np.zeros(E, np.uint64)
    ent_off = np.zeros(ng + 1, np.int64)
    if nmem == 0 or V == 0:
        return reached, ent_off, np.zeros(0, np.int32), load
    grp = np.repeat(np.arange(ng, dtype=np.int64), np.diff(mem_off))
    r = root[grp]
    ok = (r >= 0) & (r < V) & (row >= 0) & (row < nrows) & (vert >= 0) & (vert < V)
    idx = np.nonzero(ok)[0]
    g, r, rw, v = grp[idx], r[idx], row[idx], vert[idx]

    def step(rows, xs):
        """parent / next hop of xs in rows (int64, -1: none)"""
        wd = tree[rows, xs]
        if layout == INT32:
            return wd.astype(np.int64)
        return tree_parent(wd, layout)

    if to_root:
        got = (v == r) | (step(rw, r) >= 0)
    elif layout == INT32:
        got = (v == r) | (tree[rw, v].astype(np.int64) != -1)
    else:
        got = (v == r) | (tree_parent(tree[rw, v], layout) >= 0)
    reached[idx[got]] = 1
    act = got & (v != r)
    g, rw = g[act], rw[act]
    cur, end = (r[act], v[act]) if to_root else (v[act], r[act])
    keys, _ = _edge_keys_host(csr)
    found = []
    for _ in range(V):
        if cur.size == 0:
            break
        nxt = step(rw, cur)
        if ((nxt < 0) | (nxt >= V)).any():
            raise ValueError("multicast_trees_host: a walk ends off its root (not a tree row)")
        k = cur * V + nxt if to_root else nxt * V + cur
        e = np.minimum(np.searchsorted(keys, k), max(E, 1) - 1)
        if E == 0 or not np.array_equal(keys[e], k):
            raise ValueError("multicast_trees_host: a tree link the graph does not have")
        found.append(g * E + e)
        cur = nxt
        keep = cur != end
        g, rw, cur, end = g[keep], rw[keep], cur[keep], end[keep]
        if cur.size > 1:                                   # walkers that met go on as one
            if max(ng, 1) * max(nrows, 1) * V * V < (1 << 62):
                _, first = np.unique(((g * nrows + rw) * V + cur) * V + end, return_index=True)
            else:
                _, first = np.unique(np.stack([g, rw, cur, end], 1), axis=0, return_index=True)
            g, rw, cur, end = g[first], rw[first], cur[first], end[first]
    else:
        if cur.size:
            raise ValueError("multicast_trees_host: a walk longer than V (not a tree row)")
    if found:
        pairs = np.unique(np.concatenate(found))
        pg, pe = pairs // E, pairs % E
        np.cumsum(np.bincount(pg, minlength=ng), out=ent_off[1:])
        np.add.at(load, pe, w[pg])
        return reached, ent_off, pe.astype(np.int32), load
    return reached, ent_off, np.zeros(0, np.int32), load


FAIR_LDS_MAX_V = 6800           # csrc/common.h kFairLdsMaxV: fair-rate row state in LDS up to this V
FAIR_MULT_LIMIT = 1 << 53       # the multiplicities of one call sum below this: doubles hold them


def check_fair_flows(E, n, mult, cap, extra):
    """(mult uint64 [n], cap float64 [E + nextra], extra int64 [n, 2], nextra)
    after sdnr_fair_rates' checks, done on the host where they can name the
    culprit: capacities positive and finite, extras -1 or in [E, E + nextra),
    multiplicities summing below 2**53."""
    cap = np.ascontiguousarray(np.asarray(cap, np.float64).reshape(-1))
    if cap.shape[0] < E:
        raise ValueError("fair rates: %d capacities for %d links" % (cap.shape[0], E))
    if not bool((np.isfinite(cap) & (cap > 0)).all()):
        raise ValueError("fair rates: capacities must be positive finite numbers")
    nextra = cap.shape[0] - E
    if mult is None:
        mult = np.ones(n, np.uint64)
    else:
        mult = np.ascontiguousarray(np.asarray(mult, np.uint64).reshape(-1))
        if mult.shape[0] != n:
            raise ValueError("fair rates: %d multiplicities for %d flows" % (mult.shape[0], n))
    # (a u64 sum could wrap: the halves are summed apart)
    if (int((mult >> np.uint64(32)).sum()) << 32) + int((mult & np.uint64(0xFFFFFFFF)).sum()) \
            >= FAIR_MULT_LIMIT:
        raise ValueError("fair rates: the multiplicities must sum below 2**53")
    if extra is None:
        extra = np.full((n, 2), -1, np.int64)
    else:
        extra = np.asarray(extra, np.int64).reshape(n, 2)
        if not bool(((extra == -1) | ((extra >= E) & (extra < E + nextra))).all()):
            raise ValueError("fair rates: an extra constraint outside [E, E + nextra)")
    return mult, cap, extra, nextra


def fair_rates_host(csr, tree, layout, rows, verts, mult, cap, extra=None, to_root=False):
    """numpy restatement of sdnr_fair_rates (the CPU tests' engine double and
    the checker of fair_rates.hip): max-min fair rates by progressive filling
    of flows (row ``rows[i]`` of ``tree``, vertex ``verts[i]``, multiplicity
    ``mult[i]`` or 1, extra constraints ``extra[i]`` -- two indices in [E, E +
    nextra) into ``cap`` or -1).  Returns ``(rate float64 [n], bott int32 [n],
    round int32 [n], level float64 [rounds], used float64 [E + nextra])``.

    The definition is sdnroute.h's, step for step: exact u64 counts, then per
    link and round one multiply, one add, one subtract and one divide, each a
    separate numpy operation (numpy does not fuse them), so the device results
    are these bit for bit.  Every used row is laid out once -- parents, links
    toward the root, and the ancestor tables J, J o J, ... of pointer jumping
    --; a round is then a handful of whole-table gathers and scatters whatever
    the depth of the trees.  A flow at the row's root without an extra reads
    +inf / -1 / -1; a vertex outside [0, V) or unreached in its row and a
    multiplicity 0 read 0.0 / -1 / -1.  In ``to_root`` rows a vertex without a
    next hop is taken as the root (pass -1 for a pair known to be unreachable).
    A row that is no tree of the graph raises ValueError."""
    V, E = int(csr.V), int(csr.E)
    rows = np.asarray(rows, np.int64).reshape(-1)
    verts = np.asarray(verts, np.int64).reshape(-1)
    n = rows.shape[0]
    mult, cap, extra, nextra = check_fair_flows(E, n, mult, cap, extra)
    NE = E + nextra
    rate = np.zeros(n, np.float64)
    bott = np.full(n, -1, np.int32)
    rnd = np.full(n, -1, np.int32)
    used = np.zeros(NE, np.float64)
    if n == 0:
        return rate, bott, rnd, np.zeros(0, np.float64), used
    urows, rix = np.unique(rows, return_inverse=True)
    words = np.asarray(tree)[urows]
    par = words.astype(np.int64) if layout == INT32 else tree_parent(words, layout)
    R = par.shape[0]
    vid = np.broadcast_to(np.arange(V, dtype=np.int64), par.shape)
    own = par == vid
    root = own | (par < 0) if to_root else own
    par = np.where((par < 0) | own, -1, par)
    if (par >= V).any():
        raise ValueError("fair_rates_host: a parent that is no vertex")
    has = par >= 0
    # the link of v toward the root
    ev = np.full(par.shape, -1, np.int64)
    if has.any():
        keys, _ = _edge_keys_host(csr)
        r, v = np.nonzero(has)
        p = par[r, v]
        k = (v * V + p) if to_root else (p * V + v)
        e = np.minimum(np.searchsorted(keys, k), max(E - 1, 0))
        if E == 0 or not np.array_equal(keys[e], k):
            raise ValueError("fair_rates_host: a tree link the graph does not have")
        ev[r, v] = e
    # flat tables: entry r * V + v; J_0 = parent, J_{j+1} = J_j o J_j
    base = (np.arange(R, dtype=np.int64) * V)[:, None]
    jump = np.where(has, par + base, -1).ravel()
    ev, has, root = ev.ravel(), has.ravel(), root.ravel()
    chain = []
    for _ in range(max(1, V).bit_length() + 1):
        ok = jump >= 0
        if not ok.any():
            break
        src = np.nonzero(ok)[0]
        chain.append((jump, src, jump[src]))
        nxt = np.full_like(jump, -1)
        nxt[src] = jump[jump[src]]
        jump = nxt
    else:
        raise ValueError("fair_rates_host: a row is not a tree")

    inside = (verts >= 0) & (verts < V)
    at = rix.reshape(-1) * V + np.where(inside, verts, 0)
    x0, x1 = extra[:, 0], extra[:, 1]
    there = inside & (mult > 0) & (has[at] | root[at])
    bare = there & ~has[at] & (x0 < 0) & (x1 < 0)
    rate[bare] = np.inf
    alive = there & ~bare

    rem = cap.copy()
    n_prev = np.zeros(NE, np.uint64)
    level = []
    r_prev = 0.0
    inf = np.float64(np.inf)
    for k in range(n + 2):
        # 1. the alive multiplicity that crosses every link and extra
        a = np.nonzero(alive)[0]
        A = np.zeros(R * V, np.uint64)
        np.add.at(A, at[a], mult[a])
        for _, src, dst in chain:
            nxt = A.copy()
            np.add.at(nxt, dst, A[src])
            A = nxt
        cnt = np.zeros(NE, np.uint64)
        sel = np.nonzero(has & (A != 0))[0]
        np.add.at(cnt, ev[sel], A[sel])
        a0 = a[x0[a] >= 0]
        np.add.at(cnt, x0[a0], mult[a0])
        a1 = a[(x1[a] >= 0) & (x1[a] != x0[a])]
        np.add.at(cnt, x1[a1], mult[a1])
        # 2. what the flows frozen last round carry
        if k > 0:
            p = r_prev * (n_prev - cnt).astype(np.float64)
            used = used + p
            rem = np.maximum(rem - p, 0.0)
        # 3. the next level
        share = np.full(NE, inf)
        np.divide(rem, cnt.astype(np.float64), out=share, where=cnt != 0)
        r = share.min() if NE else inf
        if r == inf:
            break
        level.append(r)
        # 4. the first saturated link toward the root, else a saturated extra
        B = np.where(has & (share[np.where(has, ev, 0)] == r), ev, -1)
        for jump, _, _ in chain:
            ok = (B < 0) & (jump >= 0)
            B = np.where(ok, B[np.where(ok, jump, 0)], B)
        b = B[at[a]]
        e0, e1 = x0[a], x1[a]
        s0 = (e0 >= 0) & (share[np.where(e0 >= 0, e0, 0)] == r)
        s1 = (e1 >= 0) & (share[np.where(e1 >= 0, e1, 0)] == r)
        b = np.where(b >= 0, b, np.where(s0, e0, np.where(s1, e1, -1)))
        hit = a[b >= 0]
        rate[hit] = r
        rnd[hit] = k
        bott[hit] = b[b >= 0]
        alive[hit] = False
        n_prev, r_prev = cnt, r
    else:
        raise AssertionError("fair_rates_host: a round froze no flow")
    return rate, bott, rnd, np.asarray(level, np.float64), used


FAIR_TIMES_BATCH = 16           # csrc/fair_rows.h kFairBatch: steps queued per status read-back


def check_fair_bytes(n, nbytes):
    """float64 [n] byte sizes of sdnr_fair_times' flows (one number: the same
    for all), finite and >= 0."""
    nbytes = np.asarray(nbytes, np.float64)
    if nbytes.ndim == 0:
        nbytes = np.full(n, float(nbytes), np.float64)
    nbytes = np.ascontiguousarray(nbytes.reshape(-1))
    if nbytes.shape[0] != n:
        raise ValueError("fair times: %d byte sizes for %d flows" % (nbytes.shape[0], n))
    if not bool((np.isfinite(nbytes) & (nbytes >= 0)).all()):
        raise ValueError("fair times: byte sizes must be finite and not negative")
    return nbytes


def _fair_epoch_cap(n, max_epochs):
    """sdnr_fair_times' max_epochs: every epoch removes a flow, so n epochs
    always suffice."""
    if max_epochs is None:
        return n
    if int(max_epochs) < 0:
        raise ValueError("fair times: max_epochs must not be negative")
    return min(int(max_epochs), n)


def fair_times_launches(epoch_rounds):
    """sdnr_last_launches after a sdnr_fair_times call that ran epochs of
    ``epoch_rounds`` rounds: epoch j takes epoch_rounds[j] + 2 steps, the step
    that finds nothing in flight (or the cap reached) one more; a step is two
    launches, steps are queued FAIR_TIMES_BATCH at a time, and one launch
    starts the call."""
    steps = int(np.sum(np.asarray(epoch_rounds, np.int64) + 2)) + 1
    return 1 + 2 * FAIR_TIMES_BATCH * (-(-steps // FAIR_TIMES_BATCH))


def fair_times_host(csr, tree, layout, rows, verts, mult, nbytes, cap, extra=None, to_root=False,
                    max_epochs=None):
    """numpy restatement of sdnr_fair_times (the CPU tests' engine double and
    the checker of fair_times.hip): max-min fair completion times.  The flows
    of ``fair_rates_host`` each send ``nbytes[i]`` bytes (per parallel flow of
    their multiplicity); they share max-min fairly, a flow that has sent its
    bytes leaves, the others are refilled.  Returns ``(time float64 [n], epoch
    int32 [n], rate0 float64 [n], remaining float64 [n], epoch_time float64
    [epochs], epoch_rounds int32 [epochs], carried float64 [E + nextra])``.

    The definition is sdnroute.h's, step for step: every epoch is one
    ``fair_rates_host`` call with the departed flows' multiplicity set to 0,
    then ``q = rem_b / rate``, ``dt = min q``, ``carried += used * dt``, and a
    flow finishes iff ``q == dt`` or ``rem_b - rate * dt <= 0`` -- every
    operation a numpy operation of its own, so the device results are these bit
    for bit.  Absent flows read +inf / -1 / 0.0, a flow at the row's root
    without an extra 0.0 / -1 / +inf, a routed flow without bytes 0.0 / -1 /
    0.0; with ``max_epochs`` reached the flows still in flight read +inf / -2
    and what they have left."""
    E = int(csr.E)
    rows = np.asarray(rows, np.int64).reshape(-1)
    n = rows.shape[0]
    mult, cap, extra_all, nextra = check_fair_flows(E, n, mult, cap, extra)
    nbytes = check_fair_bytes(n, nbytes)
    most = _fair_epoch_cap(n, max_epochs)
    inf = np.float64(np.inf)
    time = np.full(n, inf)
    epoch = np.full(n, -1, np.int32)
    left = nbytes.copy()
    carried = np.zeros(E + nextra, np.float64)
    e_time, e_rounds = [], []
    fill = lambda m: fair_rates_host(csr, tree, layout, rows, verts, m, cap, extra, to_root)  # noqa
    if n == 0:
        return (time, epoch, np.zeros(0, np.float64), left, np.zeros(0, np.float64),
                np.zeros(0, np.int32), carried)
    empty = (nbytes == 0) & (mult > 0)
    m = np.where(empty, np.uint64(0), mult)
    rate0, _, rnd, level, used = fill(m)
    if empty.any():
        # a flow without bytes is classified as it is routed, then takes no share
        r_all, _, k_all, _, _ = fill(mult)
        rate0[empty & np.isinf(r_all)] = inf
        time[empty & (np.isinf(r_all) | (k_all >= 0))] = 0.0
    bare = np.isinf(rate0)
    time[bare] = 0.0
    left[bare] = 0.0
    rate, t = rate0, np.float64(0.0)
    for j in range(n + 1):
        fl = np.nonzero(rnd >= 0)[0]                       # in flight
        if fl.size == 0:
            break
        if j == most:
            epoch[fl] = -2
            if j == 0:
                rate0[fl] = 0.0                            # (no filling ran)
            break
        q = left[fl] / rate[fl]
        dt = q.min()
        if not np.isfinite(dt):
            break
        t = t + dt
        carried = carried + used * dt
        rest = left[fl] - rate[fl] * dt
        done = (q == dt) | (rest <= 0.0)
        time[fl[done]] = t
        epoch[fl[done]] = j
        left[fl] = np.where(done, 0.0, rest)
        m[fl[done]] = 0
        e_time.append(t)
        e_rounds.append(len(level))
        rate, _, rnd, level, used = fill(m)
    else:
        raise AssertionError("fair_times_host: an epoch removed no flow")
    return (time, epoch, rate0, left, np.asarray(e_time, np.float64),
            np.asarray(e_rounds, np.int32), carried)


SPLITS = ("route", "hop")


def ecmp_link_loads_host(csr, dist, rows, srcs, weights=None, split="route"):
    """numpy float64 restatement of sdnr_ecmp_link_loads (the CPU tests' engine
    double and an independent check of ecmp_loads.hip): float64 [E] loads of
    pairs (distance row ``rows[i]`` of ``dist``, source switch ``srcs[i]``,
    weight ``weights[i]`` or 1) split over every shortest route.

    ``dist``: [k, V] hop counts toward each row's destination, uint16 or the
    cache's int16-holding-u16 plane (0xFFFF / -1: unreached).  Per used row
    the links of the shortest-path DAG (level L -> L - 1) are sorted by level
    once; sigma (shortest-route counts; ``split="hop"``: next-hop counts) is
    summed per level ascending with ``np.bincount``, then the flow is pushed
    top level first, a whole level's links at a time.  A row that is not a
    BFS labelling of the graph (a reached vertex of level > 0 without a next
    hop, a route count beyond the double range) raises ValueError."""
    if split not in SPLITS:
        raise ValueError("split must be 'route' or 'hop'")
    V, E = int(csr.V), int(csr.E)
    load = np.zeros(E, np.float64)
    rows = np.asarray(rows, np.int64)
    srcs = np.asarray(srcs, np.int64)
    if rows.size == 0 or E == 0:
        return load
    w = np.ones(rows.shape[0], np.float64) if weights is None else \
        np.asarray(weights, np.uint64).astype(np.float64)
    dist = np.asarray(dist)
    if dist.dtype == np.int16:
        dist = dist.view(np.uint16)
    rp = np.asarray(csr.row_ptr, np.int64)
    esrc = np.repeat(np.arange(V, dtype=np.int64), np.diff(rp))
    edst = np.asarray(csr.col, np.int64)
    ok = np.nonzero((srcs >= 0) & (srcs < V) & (w > 0))[0]
    ok = ok[np.argsort(rows[ok], kind="stable")]           # the pairs grouped by row
    used, first = np.unique(rows[ok], return_index=True)
    bounds = np.append(first, ok.shape[0])
    for k, r in enumerate(used.tolist()):
        lv = dist[r].astype(np.int64)
        lv[lv == 0xFFFF] = -1
        mine = ok[bounds[k]:bounds[k + 1]]
        s = srcs[mine]
        keep = lv[s] > 0                                   # not unreached, not s == d
        flow = np.bincount(s[keep], w[mine][keep], minlength=V).astype(np.float64)
        top = int(lv.max())
        dag = np.nonzero((lv[esrc] > 0) & (lv[edst] == lv[esrc] - 1))[0]
        dag = dag[np.argsort(lv[esrc[dag]], kind="stable")]
        ends = np.searchsorted(lv[esrc[dag]], np.arange(top + 2))   # level L: ends[L]:ends[L+1]
        sigma = np.zeros(V, np.float64)
        if split == "hop":
            sigma += np.bincount(esrc[dag], minlength=V)
        else:
            sigma[lv == 0] = 1.0
            for L in range(1, top + 1):
                e = dag[ends[L]:ends[L + 1]]
                sigma += np.bincount(esrc[e], sigma[edst[e]], minlength=V)
        if ((lv > 0) & ~(sigma > 0)).any() or not np.isfinite(sigma).all():
            raise ValueError("ecmp_link_loads_host: a row is not a BFS labelling of the graph")
        for L in range(top, 0, -1):
            e = dag[ends[L]:ends[L + 1]]
            x, n = esrc[e], edst[e]
            g = flow[x] / sigma[x] if split == "hop" else flow[x] * (sigma[n] / sigma[x])
            load[e] += g                                   # (a link appears once per level)
            flow += np.bincount(n, g, minlength=V)
    return load


COST_INF = _native.COST_INF
COST_MAX = COST_INF - 1         # the largest link cost (on a two-switch fabric)
COST_LDS_MAX_V = 10000          # csrc/common.h kCostLdsMaxV: cost rows in LDS up to this V
COST_LDS_B8_MAX_V = 5000        # ... kCostLdsMaxV8: in batches of 8 destinations up to this V


def check_link_costs(csr, cost):
    """The link costs as uint32 [E], after sdnr_graph_costs' checks: one per
    link, every one >= 1, the largest times (V - 1) below COST_INF."""
    c = np.asarray(cost)
    if c.shape != (int(csr.E),):
        raise ValueError("one cost per link of the graph (%d)" % int(csr.E))
    if c.size:
        if c.dtype.kind not in "iu":
            raise ValueError("link costs are integers")
        lo, hi = int(c.min()), int(c.max())
        if lo < 1:
            raise ValueError("link costs are >= 1")
        if hi * max(0, int(csr.V) - 1) >= COST_INF:
            raise ValueError("largest cost %d * (V - 1) reaches COST_INF" % hi)
    return c.astype(np.uint32)


def cost_tables_host(csr, cost, dsts):
    """CPU restatement of sdnr_cost_tables (the CPU tests' engine double and
    the checker of cost_tables.hip): (pcost uint32 [D, V], nh int32, nh_port
    int32) of the least-cost routes toward each destination of ``dsts`` under
    the per-link costs ``cost`` (uint32 [E], CSR edge order).

    Deliberately not the kernel's algorithm: one Dijkstra per destination on
    the reversed graph (``heapq``, Python ints), then the next-hop scan --
    the first entry of x's ascending row with cost + pcost[n] == pcost[x]."""
    import heapq
    V, E = int(csr.V), int(csr.E)
    cost = check_link_costs(csr, cost)
    rp = np.asarray(csr.row_ptr, np.int64)
    col = np.asarray(csr.col, np.int64)
    port = np.asarray(csr.port, np.int32)
    esrc = np.repeat(np.arange(V, dtype=np.int64), np.diff(rp))
    # reversed graph: in-links of every vertex
    order = np.argsort(col, kind="stable")
    rrp = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(col, minlength=V), out=rrp[1:])
    rsrc = esrc[order].tolist()
    rcost = cost[order].tolist()
    rrp_l = rrp.tolist()
    dsts = np.asarray(dsts, np.int64)
    D = int(dsts.shape[0])
    pcost = np.full((D, V), COST_INF, np.uint32)
    nh = np.full((D, V), -1, np.int32)
    nhp = np.full((D, V), -1, np.int32)
    c64 = cost.astype(np.int64)
    for i, d in enumerate(dsts.tolist()):
        if d < 0 or d >= V:
            continue                                       # unknown destination: empty row
        best = [None] * V
        best[d] = 0
        heap = [(0, d)]
        while heap:
            c, n = heapq.heappop(heap)
            if c != best[n]:
                continue
            for k in range(rrp_l[n], rrp_l[n + 1]):
                x, t = rsrc[k], c + rcost[k]
                if best[x] is None or t < best[x]:
                    best[x] = t
                    heapq.heappush(heap, (t, x))
        pc = np.array([-1 if b is None else b for b in best], np.int64)
        pcost[i] = np.where(pc < 0, COST_INF, pc).astype(np.uint32)
        if E:
            # links on a least-cost route; the first of each row (CSR order)
            on = (pc[col] >= 0) & (pc[esrc] > 0) & (c64 + pc[col] == pc[esrc])
            e = np.nonzero(on)[0]
            x, first = np.unique(esrc[e], return_index=True)
            nh[i, x] = col[e[first]]
            nhp[i, x] = port[e[first]]
    return pcost, nh, nhp


UTIL_MAX = _native.UTIL_MAX     # the largest link utilisation sdnr_widest_tables takes
WIDEST_LDS_MAX_V = 10000        # csrc/common.h kWidestLdsMaxV: pcost + bott records in LDS up to this V
WIDEST_LDS_B4_MAX_V = 5000      # ... kWidestLdsMaxV4: in batches of 4 destinations up to this V
WIDEST_LDS_B6_MAX_V = 3333      # ... kWidestLdsMaxV6: in batches of 6 destinations up to this V


def check_link_utilisation(csr, util):
    """The link utilisations as uint32 [E], after sdnr_widest_tables' checks:
    one per link, integers in [0, UTIL_MAX]."""
    u = np.asarray(util)
    if u.shape != (int(csr.E),):
        raise ValueError("one utilisation per link of the graph (%d)" % int(csr.E))
    if u.size:
        if u.dtype.kind not in "iu":
            raise ValueError("link utilisations are integers")
        if int(u.min()) < 0 or int(u.max()) > UTIL_MAX:
            raise ValueError("link utilisations are in [0, 2**32 - 2]")
    return u.astype(np.uint32)


def widest_tables_host(csr, cost, pcost, util, dsts):
    """numpy / Python restatement of sdnr_widest_tables (the CPU tests' engine
    double and the checker of widest_tables.hip): (bott uint32 [D, V], nh
    int32, nh_port int32) -- per destination of ``dsts`` the least-loaded
    route inside the least-cost DAG.

    ``cost``: uint32 [E] link costs (None: every link costs 1); ``pcost``:
    [D, V] u32 (or int32 holding u32) rows of the least costs toward
    ``dsts[i]`` under them; ``util``: uint32 [E] link utilisations.  Link e =
    (x -> n) is tight when pcost[n] is finite and pcost[n] + cost[e] ==
    pcost[x]; bott[x] = min over tight e of max(util[e], bott[n]), 0 at the
    destination, COST_INF where there is no route; nh[x] the tight link of the
    smallest (max(util[e], bott[n]), util[e], n).  A destination outside
    [0, V) gives an empty row.

    Deliberately not the kernel's algorithm: the vertices of a row are
    processed once, in ascending pcost order -- a tight link leads to a
    strictly cheaper vertex, which is final by then -- with Python ints and
    tuple comparison for the key."""
    V, E = int(csr.V), int(csr.E)
    cost = np.ones(E, np.uint32) if cost is None else check_link_costs(csr, cost)
    util = check_link_utilisation(csr, util)
    P = _pcost_u32(pcost)
    dsts = np.asarray(dsts, np.int64)
    D = int(dsts.shape[0])
    if P.shape != (D, V):
        raise ValueError("pcost holds one [V] row per destination")
    bott = np.full((D, V), COST_INF, np.uint32)
    nh = np.full((D, V), -1, np.int32)
    nhp = np.full((D, V), -1, np.int32)
    rp = np.asarray(csr.row_ptr, np.int64).tolist()
    col = np.asarray(csr.col, np.int64).tolist()
    port = np.asarray(csr.port, np.int64).tolist()
    c, u = cost.tolist(), util.tolist()
    INF = int(COST_INF)
    for i, d in enumerate(dsts.tolist()):
        if d < 0 or d >= V:
            continue                                       # unknown destination: empty row
        pc = P[i].astype(np.int64).tolist()
        if pc[d] != 0:
            raise ValueError("pcost row %d is not a least-cost row of destination %d" % (i, d))
        b = [INF] * V
        b[d] = 0
        for x in sorted((x for x in range(V) if pc[x] != INF and x != d), key=pc.__getitem__):
            best = None
            for e in range(rp[x], rp[x + 1]):
                n = col[e]
                if pc[n] != INF and pc[n] + c[e] == pc[x] and b[n] != INF:
                    key = (max(u[e], b[n]), u[e], n)
                    if best is None or key < best[0]:
                        best = (key, e)
            if best is None:
                if pc[x] != 0:
                    raise ValueError("vertex %d of row %d has finite cost and no tight link"
                                     % (x, i))
                continue
            b[x] = best[0][0]
            nh[i, x] = col[best[1]]
            nhp[i, x] = port[best[1]]
        bott[i] = np.asarray(b, np.uint32)
    return bott, nh, nhp


COST_ECMP_LDS_MAX_V = 7400      # csrc/common.h kCostEcmpLdsMaxV: ECMP-under-costs row state in LDS


def _pcost_u32(pcost):
    """pcost rows as numpy uint32 (the engine keeps u32 costs in int32 planes)."""
    p = np.asarray(pcost)
    if p.dtype == np.int32:
        return p.view(np.uint32)
    if p.dtype != np.uint32:
        p = (p.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    return p


def cost_ecmp_link_loads_host(csr, cost, pcost, rows, srcs, weights=None, split="route"):
    """numpy float64 restatement of sdnr_cost_ecmp_link_loads (the CPU tests'
    engine double and an independent check of cost_ecmp_loads.hip): float64
    [E] loads of pairs (row ``rows[i]`` of ``pcost``, source switch
    ``srcs[i]``, weight ``weights[i]`` or 1) split over every least-cost route
    under the link costs ``cost`` (uint32 [E], CSR edge order).

    ``pcost``: [k, V] least path costs toward each row's destination, uint32
    or the engine's int32-holding-u32 plane (COST_INF / -1: no route).
    Deliberately not the kernel's order (longest next-hop chains): the
    next-hop links (pcost[n] + cost == pcost[x]) of a used row are sorted by
    the pcost of their tail once; a next hop has a strictly smaller pcost, so
    sigma (least-cost route counts; ``split="hop"``: next-hop counts) is
    summed over the groups of equal pcost ascending and the flow is pushed
    over them descending.  A row that is not a least-cost labelling (a vertex
    of finite cost > 0 without a live next hop, a count beyond the double
    range) raises ValueError."""
    if split not in SPLITS:
        raise ValueError("split must be 'route' or 'hop'")
    V, E = int(csr.V), int(csr.E)
    load = np.zeros(E, np.float64)
    rows = np.asarray(rows, np.int64)
    srcs = np.asarray(srcs, np.int64)
    c64 = check_link_costs(csr, cost).astype(np.int64)
    if rows.size == 0 or E == 0:
        return load
    w = np.ones(rows.shape[0], np.float64) if weights is None else \
        np.asarray(weights, np.uint64).astype(np.float64)
    pcost = _pcost_u32(pcost)
    rp = np.asarray(csr.row_ptr, np.int64)
    esrc = np.repeat(np.arange(V, dtype=np.int64), np.diff(rp))
    edst = np.asarray(csr.col, np.int64)
    ok = np.nonzero((srcs >= 0) & (srcs < V) & (w > 0))[0]
    ok = ok[np.argsort(rows[ok], kind="stable")]           # the pairs grouped by row
    used, first = np.unique(rows[ok], return_index=True)
    bounds = np.append(first, ok.shape[0])
    for k, r in enumerate(used.tolist()):
        pc = pcost[r].astype(np.int64)
        fin = pc != COST_INF
        mine = ok[bounds[k]:bounds[k + 1]]
        s = srcs[mine]
        keep = fin[s] & (pc[s] > 0)                        # not unreached, not s == d
        flow = np.bincount(s[keep], w[mine][keep], minlength=V).astype(np.float64)
        dag = np.nonzero(fin[esrc] & (pc[esrc] > 0) & fin[edst] & (pc[edst] + c64 == pc[esrc]))[0]
        dag = dag[np.argsort(pc[esrc[dag]], kind="stable")]
        _, start = np.unique(pc[esrc[dag]], return_index=True)
        end = np.append(start[1:], dag.shape[0])
        sigma = np.zeros(V, np.float64)
        if split == "hop":
            sigma += np.bincount(esrc[dag], minlength=V)
        else:
            sigma[pc == 0] = 1.0
            for a, b in zip(start.tolist(), end.tolist()):
                e = dag[a:b]
                sigma += np.bincount(esrc[e], sigma[edst[e]], minlength=V)
        if (fin & (pc > 0) & ~(sigma > 0)).any() or not np.isfinite(sigma).all():
            raise ValueError("cost_ecmp_link_loads_host: a row is not a least-cost labelling "
                             "of the graph under these costs")
        for a, b in zip(start.tolist()[::-1], end.tolist()[::-1]):
            e = dag[a:b]
            x, n = esrc[e], edst[e]
            g = flow[x] / sigma[x] if split == "hop" else flow[x] * (sigma[n] / sigma[x])
            load[e] += g                                   # (a link appears in one group)
            flow += np.bincount(n, g, minlength=V)
    return load


ECMP_FAIR_LDS_MAX_V = 7400      # csrc/common.h kEcmpFairLdsMaxV: ECMP fair-rate row state in LDS
FAIR_TIE = 2.0 ** -30           # ecmp_fair_rates.hip kFairTie: shares within r * FAIR_TIE of r tie


def ecmp_fair_rates_host(csr, cost, pcost, rows, srcs, mult, cap, extra=None, split="route"):
    """numpy restatement of sdnr_ecmp_fair_rates (the CPU tests' engine double
    and the checker of ecmp_fair_rates.hip): max-min fair rates by progressive
    filling of flows split over every least-cost route -- flow i enters at
    switch ``srcs[i]`` of row ``rows[i]`` of ``pcost``, counts ``mult[i]``
    times (None: once) and is also bound by ``extra[i]`` (two indices in [E, E
    + nextra) into ``cap`` or -1).  ``cost``: uint32 [E], None: every link
    costs 1 (``pcost`` rows are hop counts then).  Returns ``(rate float64
    [n], bott int32 [n], round int32 [n], level float64 [rounds], used float64
    [E + nextra])``.

    The definition is sdnroute.h's, step for step, each arithmetic step a
    separate numpy operation.  Every used row is laid out once: its tight
    links sorted by the pcost of their tail (``cost_ecmp_link_loads_host``'s
    order; a next hop has a strictly smaller pcost) and its route counts.  A
    round pushes the alive multiplicities over the groups of equal pcost
    descending -- group j of every row in one numpy step -- and finds the
    smallest saturated link below every vertex over them ascending.  The sums
    into ``a[e]`` run in this order and the device's in any: equal within
    rounding, bit for bit where every partial sum is exact.  A flow with
    ``srcs[i]`` the destination and no extra reads +inf / -1 / -1; a source
    outside [0, V) or without a route and a multiplicity 0 read 0.0 / -1 / -1.
    A row that is no least-cost labelling raises ValueError."""
    if split not in SPLITS:
        raise ValueError("split must be 'route' or 'hop'")
    V, E = int(csr.V), int(csr.E)
    rows = np.asarray(rows, np.int64).reshape(-1)
    srcs = np.asarray(srcs, np.int64).reshape(-1)
    n = rows.shape[0]
    mult, cap, extra, nextra = check_fair_flows(E, n, mult, cap, extra)
    NE = E + nextra
    c64 = np.ones(E, np.int64) if cost is None else check_link_costs(csr, cost).astype(np.int64)
    rate = np.zeros(n, np.float64)
    bott = np.full(n, -1, np.int32)
    rnd = np.full(n, -1, np.int32)
    used = np.zeros(NE, np.float64)
    if n == 0:
        return rate, bott, rnd, np.zeros(0, np.float64), used
    pcost = _pcost_u32(pcost)
    if rows.min() < 0 or rows.max() >= pcost.shape[0]:
        raise ValueError("ecmp_fair_rates_host: a pair names a row outside the table")
    urows, rix = np.unique(rows, return_inverse=True)
    R = urows.shape[0]
    RV = R * V
    pc = pcost[urows].astype(np.int64)
    fin = pc != COST_INF
    rp = np.asarray(csr.row_ptr, np.int64)
    esrc = np.repeat(np.arange(V, dtype=np.int64), np.diff(rp))
    edst = np.asarray(csr.col, np.int64)
    # the tight links of every used row, with the rank of their tail's pcost in the row
    le, lx, ln, lj = [], [], [], []
    for k in range(R):
        p = pc[k]
        dag = np.nonzero(fin[k][esrc] & (p[esrc] > 0) & fin[k][edst] & (p[edst] + c64 == p[esrc]))[0]
        dag = dag[np.argsort(p[esrc[dag]], kind="stable")]
        _, j = np.unique(p[esrc[dag]], return_inverse=True)
        le.append(dag)
        lx.append(esrc[dag] + k * V)
        ln.append(edst[dag] + k * V)
        lj.append(j.reshape(-1))
    le, lx, ln, lj = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (le, lx, ln, lj))
    order = np.argsort(lj, kind="stable")
    le, lx, ln, lj = le[order], lx[order], ln[order], lj[order]
    ends = np.cumsum(np.bincount(lj)) if lj.size else np.zeros(0, np.int64)
    groups = list(zip(np.append(0, ends[:-1]).tolist(), ends.tolist())) if lj.size else []
    sigma = np.zeros(RV, np.float64)
    if split == "hop":
        sigma += np.bincount(lx, minlength=RV)
        q = None
    else:
        sigma[(pc == 0).ravel()] = 1.0
        for a, b in groups:
            sigma += np.bincount(lx[a:b], sigma[ln[a:b]], minlength=RV)
    if ((fin & (pc > 0)).ravel() & ~(sigma > 0)).any() or not np.isfinite(sigma).all():
        raise ValueError("ecmp_fair_rates_host: a row is not a least-cost labelling of the "
                         "graph under these costs")
    if split != "hop":
        q = sigma[ln] / sigma[lx]

    inside = (srcs >= 0) & (srcs < V)
    at = rix.reshape(-1) * V + np.where(inside, srcs, 0)
    pcs = pc.ravel()[at]
    x0, x1 = extra[:, 0], extra[:, 1]
    there = inside & (mult > 0) & (pcs != COST_INF)
    bare = there & (pcs == 0) & (x0 < 0) & (x1 < 0)
    rate[bare] = np.inf
    alive = there & ~bare
    fmult = mult.astype(np.float64)

    none = np.int64(1) << 62
    rem = cap.copy()
    a_prev = np.zeros(NE, np.float64)
    level = []
    r_prev = np.float64(0.0)
    inf = np.float64(np.inf)
    for k in range(n + 2):
        # 1. the ECMP push of the alive multiplicities
        al = np.nonzero(alive)[0]
        flow = np.bincount(at[al], fmult[al], minlength=RV).astype(np.float64)
        cnt = np.zeros(NE, np.float64)
        for a, b in groups[::-1]:
            x = lx[a:b]
            g = flow[x] / sigma[x] if q is None else flow[x] * q[a:b]
            cnt += np.bincount(le[a:b], g, minlength=NE)
            flow += np.bincount(ln[a:b], g, minlength=RV)
        a0 = al[x0[al] >= 0]
        np.add.at(cnt, x0[a0], fmult[a0])
        a1 = al[(x1[al] >= 0) & (x1[al] != x0[al])]
        np.add.at(cnt, x1[a1], fmult[a1])
        # 2. what the flows frozen last round carry
        if k > 0:
            m = np.maximum(a_prev - cnt, 0.0)
            p = r_prev * m
            used = used + p
            rem = np.maximum(rem - p, 0.0)
        # 3. the next level, never below the last
        share = np.full(NE, inf)
        np.divide(rem, cnt, out=share, where=cnt > 0)
        r = share.min() if NE else inf
        r = max(r, r_prev)
        if r == inf:
            break
        level.append(r)
        # 4. saturated: within the tie tolerance of the level
        t = r * np.float64(FAIR_TIE)
        sat = share <= r + t
        # 5. the smallest saturated link below every vertex, else a saturated extra
        B = np.full(RV, none, np.int64)
        for a, b in groups:
            e = le[a:b]
            np.minimum.at(B, lx[a:b], np.minimum(np.where(sat[e], e, none), B[ln[a:b]]))
        bb = B[at[al]]
        e0, e1 = x0[al], x1[al]
        s0 = (e0 >= 0) & sat[np.where(e0 >= 0, e0, 0)] if NE else e0 >= 0
        s1 = (e1 >= 0) & sat[np.where(e1 >= 0, e1, 0)] if NE else e1 >= 0
        bb = np.where(bb != none, bb, np.where(s0, e0, np.where(s1, e1, -1)))
        hit = al[bb >= 0]
        rate[hit] = r
        rnd[hit] = k
        bott[hit] = bb[bb >= 0]
        alive[hit] = False
        a_prev, r_prev = cnt, r
    else:
        raise AssertionError("ecmp_fair_rates_host: a round froze no flow")
    return rate, bott, rnd, np.asarray(level, np.float64), used


def ecmp_fair_times_host(csr, cost, pcost, rows, srcs, mult, nbytes, cap, extra=None,
                         split="route", max_epochs=None):
    """numpy restatement of sdnr_ecmp_fair_times (the CPU tests' engine double
    and the checker of ecmp_fair_times.hip): max-min fair completion times of
    flows split over every least-cost route.  The flows of
    ``ecmp_fair_rates_host`` each send ``nbytes[i]`` bytes (per parallel flow
    of their multiplicity); they share max-min fairly, a flow that has sent its
    bytes leaves, the others are refilled.  Returns the 7-tuple of
    ``fair_times_host``: ``(time, epoch, rate0, remaining, epoch_time,
    epoch_rounds, carried)``.

    The definition is sdnroute.h's, step for step: every epoch is one
    ``ecmp_fair_rates_host`` call with the departed flows' multiplicity set to
    0, then ``q = rem_b / rate``, ``dt = min q``, ``bound = dt + dt *
    FAIR_TIE``, ``carried += used * dt``, and a flow finishes iff ``q <=
    bound`` or ``rem_b - rate * dt <= 0`` -- every operation a numpy operation
    of its own.  The advance shares the filling's tie tolerance: the link
    counts are float sums, so flows that end together as fractions have q's
    that differ in their last bits, and an exact ``q == dt`` would spread them
    over epochs that another summation order does not have.  The device
    results are these within rounding, and bit for bit where every partial sum
    is exact.  Special values as in ``fair_times_host`` (a flow at the
    destination without an extra is the one at the row's root); a row that is
    no least-cost labelling raises ValueError."""
    E = int(csr.E)
    rows = np.asarray(rows, np.int64).reshape(-1)
    n = rows.shape[0]
    mult, cap, extra_all, nextra = check_fair_flows(E, n, mult, cap, extra)
    nbytes = check_fair_bytes(n, nbytes)
    most = _fair_epoch_cap(n, max_epochs)
    inf = np.float64(np.inf)
    time = np.full(n, inf)
    epoch = np.full(n, -1, np.int32)
    left = nbytes.copy()
    carried = np.zeros(E + nextra, np.float64)
    e_time, e_rounds = [], []
    fill = lambda m: ecmp_fair_rates_host(csr, cost, pcost, rows, srcs, m, cap, extra, split)  # noqa
    if n == 0:
        if split not in SPLITS:
            raise ValueError("split must be 'route' or 'hop'")
        return (time, epoch, np.zeros(0, np.float64), left, np.zeros(0, np.float64),
                np.zeros(0, np.int32), carried)
    empty = (nbytes == 0) & (mult > 0)
    m = np.where(empty, np.uint64(0), mult)
    rate0, _, rnd, level, used = fill(m)
    if empty.any():
        # a flow without bytes is classified as it is routed, then takes no share
        r_all, _, k_all, _, _ = fill(mult)
        rate0[empty & np.isinf(r_all)] = inf
        time[empty & (np.isinf(r_all) | (k_all >= 0))] = 0.0
    bare = np.isinf(rate0)
    time[bare] = 0.0
    left[bare] = 0.0
    rate, t = rate0, np.float64(0.0)
    tie = np.float64(FAIR_TIE)
    for j in range(n + 1):
        fl = np.nonzero(rnd >= 0)[0]                       # in flight
        if fl.size == 0:
            break
        if j == most:
            epoch[fl] = -2
            if j == 0:
                rate0[fl] = 0.0                            # (no filling ran)
            break
        q = left[fl] / rate[fl]
        dt = q.min()
        if not np.isfinite(dt):
            break
        slack = dt * tie
        bound = dt + slack
        t = t + dt
        carried = carried + used * dt
        rest = left[fl] - rate[fl] * dt
        done = (q <= bound) | (rest <= 0.0)
        time[fl[done]] = t
        epoch[fl[done]] = j
        left[fl] = np.where(done, 0.0, rest)
        m[fl[done]] = 0
        e_time.append(t)
        e_rounds.append(len(level))
        rate, _, rnd, level, used = fill(m)
    else:
        raise AssertionError("ecmp_fair_times_host: an epoch removed no flow")
    return (time, epoch, rate0, left, np.asarray(e_time, np.float64),
            np.asarray(e_rounds, np.int32), carried)


FAILURE_LDS_MAX_V = 7100        # csrc/common.h kFailureLdsMaxV: what-if row state in LDS


def normalise_scenarios(scenarios, E):
    """Failure scenarios (a sequence of int arrays of CSR edge indices) as the
    list of their sorted, deduplicated int32 arrays; an index outside [0, E)
    is a ValueError."""
    out = []
    for sc in scenarios:
        a = np.unique(np.asarray(sc, np.int64).reshape(-1))
        if a.size and (a[0] < 0 or a[-1] >= E):
            raise ValueError("a failed link is an edge index in [0, %d)" % E)
        out.append(a.astype(np.int32))
    return out


def failure_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, weights=None, scenarios=(),
                                 split="route"):
    """numpy restatement of sdnr_failure_ecmp_link_loads (the CPU tests' engine
    double and an independent check of failure_loads.hip): (load float64
    [nscen, E], lost float64 [nscen], routed bool [nscen, npairs]) of pairs
    (toward dense switch ``dsts[rows[i]]``, from ``srcs[i]``, weight
    ``weights[i]`` or 1) split over every least-cost route under the link costs
    ``cost`` (uint32 [E]; None: every link costs 1), once per scenario of
    ``scenarios`` (int arrays of failed CSR edge indices) with that scenario's
    links down.

    Deliberately not the kernel's masking: per scenario the failed edges are
    really removed from the CSR, ``cost_tables_host`` and
    ``cost_ecmp_link_loads_host`` run on the reduced graph, and the loads are
    scattered back to the full graph's edge order (a failed link holds 0.0).
    ``routed[k, i]``: the source is a vertex and reaches the destination in
    scenario k (s == d counts); ``lost[k]``: the weight of the pairs with s !=
    d and weight > 0 whose source is a vertex that does not."""
    from .topologies import CSR
    if split not in SPLITS:
        raise ValueError("split must be 'route' or 'hop'")
    V, E = int(csr.V), int(csr.E)
    cost = np.ones(E, np.uint32) if cost is None else check_link_costs(csr, cost)
    scen = normalise_scenarios(scenarios, E)
    dsts = np.asarray(dsts, np.int64)
    rows = np.asarray(rows, np.int64)
    srcs = np.asarray(srcs, np.int64)
    n = int(rows.shape[0])
    w = np.ones(n, np.uint64) if weights is None else np.asarray(weights, np.uint64)
    load = np.zeros((len(scen), E), np.float64)
    lost = np.zeros(len(scen), np.float64)
    routed = np.zeros((len(scen), n), bool)
    if n == 0 or dsts.size == 0:
        return load, lost, routed
    if rows.min() < 0 or rows.max() >= dsts.shape[0]:
        raise ValueError("failure_ecmp_link_loads_host: a pair names a row outside dsts")
    esrc = np.repeat(np.arange(V, dtype=np.int64), np.diff(np.asarray(csr.row_ptr, np.int64)))
    d = dsts[rows]
    s_ok = (srcs >= 0) & (srcs < V)
    d_ok = (d >= 0) & (d < V)
    sc = np.where(s_ok, srcs, 0)
    for k, failed in enumerate(scen):
        keep = np.ones(E, bool)
        keep[failed] = False
        rp = np.zeros(V + 1, np.int64)
        np.cumsum(np.bincount(esrc[keep], minlength=V), out=rp[1:])
        red = CSR(csr.dpids, rp, np.asarray(csr.col)[keep], np.asarray(csr.port)[keep])
        pc = cost_tables_host(red, cost[keep], dsts)[0]
        load[k, keep] = cost_ecmp_link_loads_host(red, cost[keep], pc, rows, srcs, weights, split)
        routed[k] = s_ok & d_ok & (pc[rows, sc] != COST_INF)
        gone = s_ok & (srcs != d) & (w > 0) & ~routed[k]
        lost[k] = float(w[gone].astype(np.float64).sum())
    return load, lost, routed


def normalise_cost_scenarios(scenarios, csr):
    """Cost scenarios (a sequence of ``(edges, costs)``: CSR edge indices and
    the cost each takes, COST_INF: the link is down) as the list of their
    (int32 edges ascending, uint32 costs beside them).  A repeated edge, an
    index outside [0, E), a list of another length and a cost that is neither
    COST_INF nor one ``check_link_costs`` accepts (>= 1, times (V - 1) below
    COST_INF) are ValueErrors."""
    V, E = int(csr.V), int(csr.E)
    out = []
    for edges, costs in scenarios:
        e = np.asarray(edges, np.int64).reshape(-1)
        c = np.asarray(costs).reshape(-1)
        if c.shape != e.shape:
            raise ValueError("one cost per overridden link")
        if c.size and c.dtype.kind not in "iu":
            raise ValueError("link costs are integers")
        for x in c.tolist():
            if x != COST_INF and (x < 1 or x * max(0, V - 1) >= COST_INF):
                raise ValueError("an override is COST_INF or a cost >= 1 with cost * (V - 1) "
                                 "below COST_INF: %r" % (x,))
        order = np.argsort(e, kind="stable")
        e, c = e[order], c.astype(np.uint32)[order]
        if e.size and (e[0] < 0 or e[-1] >= E):
            raise ValueError("an overridden link is an edge index in [0, %d)" % E)
        if (e[1:] == e[:-1]).any():
            raise ValueError("a link is overridden once per scenario")
        out.append((e.astype(np.int32), c))
    return out


def peak_utilisation(load, capacity=None):
    """(peak float64, edge int): the largest ``load[e] / capacity[e]``
    (capacity None: 1.0 each) and the first link that attains it; 0.0 and -1
    when nothing is carried."""
    u = np.asarray(load, np.float64)
    if capacity is not None:
        u = u / np.asarray(capacity, np.float64)
    if u.size == 0 or not (u.max() > 0):
        return 0.0, -1
    return float(u.max()), int(u.argmax())


def _check_capacity(capacity, E):
    """float64 [E] capacities, every one finite and > 0, or None."""
    if capacity is None:
        return None
    cap = np.ascontiguousarray(capacity, np.float64)
    if cap.shape != (E,):
        raise ValueError("one capacity per link of the graph (%d)" % E)
    if not (np.isfinite(cap) & (cap > 0)).all():
        raise ValueError("capacities are positive finite numbers")
    return cap


def whatif_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, weights=None, scenarios=(),
                                split="route", capacity=None):
    """numpy restatement of sdnr_whatif_ecmp_link_loads (the CPU tests' engine
    double and an independent check of whatif_loads.hip): (load float64 [nscen,
    E], lost float64 [nscen], routed bool [nscen, npairs], peak float64
    [nscen], peak_edge int32 [nscen]) of the pairs of
    ``failure_ecmp_link_loads_host`` once per cost scenario of ``scenarios``
    (``(edges, costs)``: the links of ``edges`` cost ``costs``, COST_INF: the
    link is down; every other link keeps its cost of ``cost``, None: 1).
    ``peak[k]``: the largest ``load[k, e] / capacity[e]`` (None: 1.0 each),
    ``peak_edge[k]``: the first link that attains it (0.0 and -1 without load).

    Deliberately not the kernel's cursor: per scenario the full cost vector is
    built, the COST_INF edges are really removed from the CSR,
    ``cost_tables_host`` and ``cost_ecmp_link_loads_host`` run on that graph
    under those costs, and the loads are scattered back to the full graph's
    edge order (a link that is down holds 0.0)."""
    from .topologies import CSR
    if split not in SPLITS:
        raise ValueError("split must be 'route' or 'hop'")
    V, E = int(csr.V), int(csr.E)
    cost = np.ones(E, np.uint32) if cost is None else check_link_costs(csr, cost)
    scen = normalise_cost_scenarios(scenarios, csr)
    cap = _check_capacity(capacity, E)
    dsts = np.asarray(dsts, np.int64)
    rows = np.asarray(rows, np.int64)
    srcs = np.asarray(srcs, np.int64)
    n = int(rows.shape[0])
    w = np.ones(n, np.uint64) if weights is None else np.asarray(weights, np.uint64)
    load = np.zeros((len(scen), E), np.float64)
    lost = np.zeros(len(scen), np.float64)
    routed = np.zeros((len(scen), n), bool)
    peak = np.zeros(len(scen), np.float64)
    peak_edge = np.full(len(scen), -1, np.int32)
    if n == 0 or dsts.size == 0:
        return load, lost, routed, peak, peak_edge
    if rows.min() < 0 or rows.max() >= dsts.shape[0]:
        raise ValueError("whatif_ecmp_link_loads_host: a pair names a row outside dsts")
    esrc = np.repeat(np.arange(V, dtype=np.int64), np.diff(np.asarray(csr.row_ptr, np.int64)))
    d = dsts[rows]
    s_ok = (srcs >= 0) & (srcs < V)
    d_ok = (d >= 0) & (d < V)
    sc = np.where(s_ok, srcs, 0)
    for k, (edges, costs) in enumerate(scen):
        now = cost.copy()
        now[edges] = costs
        keep = now != COST_INF
        rp = np.zeros(V + 1, np.int64)
        np.cumsum(np.bincount(esrc[keep], minlength=V), out=rp[1:])
        red = CSR(csr.dpids, rp, np.asarray(csr.col)[keep], np.asarray(csr.port)[keep])
        pc = cost_tables_host(red, now[keep], dsts)[0]
        load[k, keep] = cost_ecmp_link_loads_host(red, now[keep], pc, rows, srcs, weights, split)
        routed[k] = s_ok & d_ok & (pc[rows, sc] != COST_INF)
        gone = s_ok & (srcs != d) & (w > 0) & ~routed[k]
        lost[k] = float(w[gone].astype(np.float64).sum())
        peak[k], peak_edge[k] = peak_utilisation(load[k], cap)
    return load, lost, routed, peak, peak_edge


LFA_MAX_V = 16384               # csrc/common.h kLfaMaxV: sdnr_lfa_tables' cap (sdnr_apsp's)
LFA_BACKUP, LFA_DOWNSTREAM, LFA_NODE = 1, 2, 4     # bits of sdnr_lfa_tables' kind


def lfa_tables_host(csr, cost, pcost_all, dsts, link_only=False):
    """numpy restatement of sdnr_lfa_tables (the CPU tests' engine double and
    the checker of lfa_tables.hip): (backup int32 [D, V], backup_port int32,
    kind uint8, counts uint32 [D, 4]) -- the loop-free alternate next hop of
    every switch toward each destination of ``dsts``.

    ``pcost_all``: [V, V] u32 (or int32 holding u32), row v = the least costs
    toward v under ``cost`` (uint32 [E]; None: every link costs 1).  For the
    primary p of (s, d) -- the first tight link of s's row; none at s == d or
    where there is no route -- a neighbour n != p of finite P[d][n] is
    loop-free iff P[s][n] is INF or P[d][n] < P[s][n] + P[d][s], downstream iff
    P[d][n] < P[d][s], node-protecting iff loop-free and (P[p][n] is INF or
    P[d][n] < P[p][n] + P[d][p]); the backup is the loop-free one of the
    smallest (not node-protecting, cost + P[d][n], n) -- (cost + P[d][n], n)
    with ``link_only``, which never reports node protection.  ``kind``:
    LFA_BACKUP | LFA_DOWNSTREAM | LFA_NODE bits; ``counts``: primaries,
    backups, node-protecting and downstream backups of each row.

    Deliberately not the kernel's shape: per destination row, masks over all E
    links at once and one ``np.lexsort`` for the choice; of ``pcost_all`` only
    the requested rows, P[s][n] per link and P[p][n] per loop-free candidate
    are gathered.  Python ints / int64 throughout: no sum can wrap."""
    V, E = int(csr.V), int(csr.E)
    cost = np.ones(E, np.uint32) if cost is None else check_link_costs(csr, cost)
    P = _pcost_u32(pcost_all)
    if P.shape != (V, V):
        raise ValueError("pcost_all is the [V, V] all-pairs table (row v: destination v)")
    dsts = np.asarray(dsts, np.int64)
    D = int(dsts.shape[0])
    backup = np.full((D, V), -1, np.int32)
    bport = np.full((D, V), -1, np.int32)
    kind = np.zeros((D, V), np.uint8)
    counts = np.zeros((D, 4), np.uint32)
    if E == 0 or D == 0:
        return backup, bport, kind, counts
    rp = np.asarray(csr.row_ptr, np.int64)
    col = np.asarray(csr.col, np.int64)
    port = np.asarray(csr.port, np.int32)
    esrc = np.repeat(np.arange(V, dtype=np.int64), np.diff(rp))
    c64 = cost.astype(np.int64)
    eid = np.arange(E, dtype=np.int64)
    INF = int(COST_INF)
    back = P[esrc, col].astype(np.int64)                    # P[s][n] of every link
    for i, d in enumerate(dsts.tolist()):
        if d < 0 or d >= V:
            continue                                       # unknown destination: empty row
        Pd = P[d].astype(np.int64)
        Ps, Pn = Pd[esrc], Pd[col]
        reach = (Pn != INF) & (Ps != INF) & (esrc != d)
        # the primary: the first tight link of each row
        te = np.nonzero(reach & (c64 + Pn == Ps))[0]
        x, first = np.unique(esrc[te], return_index=True)
        prim = np.full(V, -1, np.int64)
        prim[x] = te[first]
        pe = prim[esrc]
        lf = reach & (pe >= 0) & (eid != pe)
        lf &= (back == INF) | (Pn < back + Ps)
        ce = np.nonzero(lf)[0]                              # the loop-free candidates
        counts[i, 0] = x.shape[0]
        if ce.size == 0:
            continue
        cs, cn = esrc[ce], col[ce]
        if link_only:
            npro = np.zeros(ce.shape[0], bool)
        else:
            p = col[pe[ce]]
            ppn = P[p, cn].astype(np.int64)                 # P[p][n]
            npro = (ppn == INF) | (Pn[ce] < ppn + Pd[p])
        order = np.lexsort((cn, c64[ce] + Pn[ce], ~npro, cs))
        s_sorted = cs[order]
        head = np.ones(order.shape[0], bool)
        head[1:] = s_sorted[1:] != s_sorted[:-1]
        win = order[head]
        ws, we = cs[win], ce[win]
        backup[i, ws] = col[we]
        bport[i, ws] = port[we]
        k = np.full(win.shape[0], LFA_BACKUP, np.uint8)
        k[Pn[we] < Ps[we]] |= LFA_DOWNSTREAM
        k[npro[win]] |= LFA_NODE
        kind[i, ws] = k
        counts[i, 1] = win.shape[0]
        counts[i, 2] = int(npro[win].sum())
        counts[i, 3] = int((Pn[we] < Ps[we]).sum())
    return backup, bport, kind, counts


RLFA_REPAIR, RLFA_PLAIN, RLFA_LFA = 1, 2, 4        # bits of sdnr_remote_lfa's kind


def remote_lfa_host(csr, cost, pcost_all, verts=None):
    """numpy restatement of sdnr_remote_lfa (the CPU tests' engine double and
    the checker of remote_lfa.hip): (pq, via, via_port int32 [E], tunnel_cost
    uint64 [E], kind uint8 [E], counts uint32 [n, 4]) -- the remote loop-free
    alternate (RFC 7490 PQ-node repair tunnel) of every out-link of the source
    vertices ``verts`` (None: all of them, 0 .. V - 1).

    ``pcost_all`` and ``cost`` as in ``lfa_tables_host``; D(a, b) =
    pcost_all[b][a].  For a link e = (S -> E) of cost c, E != S, a vertex X != S
    is in the Q-space iff D(X,E) is finite and (D(X,S) is INF or D(X,E) <
    D(X,S) + c), and in the extended P-space through the head N of another
    out-link f of S (N != E, N != S) iff D(N,X) is finite and (D(N,S) is INF or
    D(E,X) is INF or D(N,X) < D(N,S) + c + D(E,X)).  The repair is the (X, N)
    in both of the smallest (cost[f] + D(N,X), X, N): ``pq`` = X, ``via`` = N,
    ``via_port`` = f's port, ``tunnel_cost`` the key's first component,
    ``kind`` = RLFA_REPAIR | RLFA_PLAIN (X is in S's own P-space: D(S,X) finite
    and (D(E,X) INF or D(S,X) < c + D(E,X))) | RLFA_LFA (X == N); -1 / -1 / -1
    / 0 / 0 where there is none, and at a self-loop.  Only the out-links of the
    listed vertices are written (the others keep -1 / -1 / -1 / 0 / 0); a vertex
    outside [0, V) is an empty unit.  ``counts``: per unit, the out-links that
    are no self-loops, those repaired, those RLFA_PLAIN, those RLFA_LFA.

    A CSR row is strictly ascending (no two links of a vertex share a head, as
    sdnr_graph_upload requires), so N != E excludes exactly the link's own slot.

    Deliberately not the kernel's shape: per link one [deg, V] mask over every
    (neighbour, X) at once and numpy minima for the choice; int64 throughout:
    no sum can wrap."""
    V, E = int(csr.V), int(csr.E)
    cost = np.ones(E, np.uint32) if cost is None else check_link_costs(csr, cost)
    P = _pcost_u32(pcost_all)
    if P.shape != (V, V):
        raise ValueError("pcost_all is the [V, V] all-pairs table (row v: destination v)")
    verts = np.arange(V, dtype=np.int64) if verts is None else np.asarray(verts, np.int64)
    n = int(verts.shape[0])
    pq = np.full(E, -1, np.int32)
    via = np.full(E, -1, np.int32)
    vport = np.full(E, -1, np.int32)
    tcost = np.zeros(E, np.uint64)
    kind = np.zeros(E, np.uint8)
    counts = np.zeros((n, 4), np.uint32)
    rp = np.asarray(csr.row_ptr, np.int64)
    col = np.asarray(csr.col, np.int64)
    port = np.asarray(csr.port, np.int32)
    INF = int(COST_INF)
    P64 = P.astype(np.int64)
    for u, s in enumerate(verts.tolist()):
        if s < 0 or s >= V:
            continue                                       # unknown vertex: an empty unit
        lo, hi = int(rp[s]), int(rp[s + 1])
        nb = col[lo:hi]
        cs = cost[lo:hi].astype(np.int64)
        DN = P64[:, nb].T                                  # [deg, V]: D(N_j, X)
        back = P64[s, nb]                                  # D(N_j, S)
        DS = P64[s]                                        # D(X, S)
        tc_all = cs[:, None] + DN
        for i in range(hi - lo):
            e, t, c = lo + i, int(nb[i]), int(cs[i])
            pq[e], via[e], vport[e], tcost[e], kind[e] = -1, -1, -1, 0, 0
            if t == s:
                continue
            counts[u, 0] += 1
            DE = P64[t]                                    # D(X, E)
            q = (DE != INF) & ((DS == INF) | (DE < DS + c))
            q[s] = False
            dex = DN[i]                                    # D(E, X)
            ok = (DN != INF) & ((back[:, None] == INF) | (dex[None, :] == INF) |
                                (DN < back[:, None] + c + dex[None, :]))
            ok &= q[None, :]
            ok[i] = False
            ok[nb == s] = False
            if not ok.any():
                continue
            tc = np.where(ok, tc_all, np.int64(1) << 40)
            best = int(tc.min())
            x = int(np.nonzero((tc == best).any(axis=0))[0][0])
            j = int(np.nonzero(tc[:, x] == best)[0][0])
            dsx, dtx = int(P64[x, s]), int(P64[x, t])      # D(S, X), D(E, X)
            k = RLFA_REPAIR
            if dsx != INF and (dtx == INF or dsx < c + dtx):
                k |= RLFA_PLAIN
                counts[u, 2] += 1
            if x == int(nb[j]):
                k |= RLFA_LFA
                counts[u, 3] += 1
            counts[u, 1] += 1
            pq[e], via[e], vport[e], tcost[e], kind[e] = x, int(nb[j]), port[lo + j], best, k
    return pq, via, vport, tcost, kind, counts


FRR_MAX_V = 6200                # csrc/common.h kFrrMaxV: the fast-reroute item state in LDS


def frr_link_loads_host(csr, nh, backup, dsts, rows, srcs, weights=None, scenarios=()):
    """numpy restatement of sdnr_frr_link_loads (the CPU tests' engine double
    and an independent check of frr_loads.hip): ``(load uint64 [nscen, E], stat
    uint64 [nscen, 4], status uint8 [nscen, npairs], peak uint64 [nscen],
    peak_edge int32 [nscen], items)`` of pairs (toward dense switch
    ``dsts[rows[i]]``, from ``srcs[i]``, weight ``weights[i]`` or 1) forwarded
    over the next-hop rows ``nh`` and, where a scenario took a switch's primary
    link, over ``backup`` (int32 [nrows, V] each, -1: none), once per scenario of
    ``scenarios`` (int arrays of failed CSR edge indices).

    ``status``: 0 no base route (or a source or destination that is no
    vertex), 1 delivered over primaries, 2 delivered through a repair, 3
    dropped, 4 looped; only delivered pairs add load.  ``stat[k]``: the weight
    repaired, dropped, looped, without a base route.  ``items``: the (scenario,
    row) items some failed link x -> n touches (``nh[r, x] == n``, the row has
    pairs).

    Per item the row is patched (``fwd``), every vertex is classified by the
    2^t-th successor under ``fwd`` with the switches that forward nowhere as
    fixed points, and the delivered sources are summed over the patched row by
    ``link_loads_host``; the unaffected rows of a scenario keep their base
    loads.  u64 sums wrap, as on the device."""
    V, E = int(csr.V), int(csr.E)
    scen = normalise_scenarios(scenarios, E)
    nscen = len(scen)
    dsts = np.asarray(dsts, np.int64).reshape(-1)
    rows = np.asarray(rows, np.int64).reshape(-1)
    srcs = np.asarray(srcs, np.int64).reshape(-1)
    n, nrows = int(rows.shape[0]), int(dsts.shape[0])
    w = np.ones(n, np.uint64) if weights is None else np.asarray(weights, np.uint64).reshape(-1)
    load = np.zeros((nscen, E), np.uint64)
    stat = np.zeros((nscen, 4), np.uint64)
    status = np.zeros((nscen, n), np.uint8)
    peak = np.zeros(nscen, np.uint64)
    peak_edge = np.full(nscen, -1, np.int32)
    items = 0
    if n and (rows.min() < 0 or rows.max() >= nrows):
        raise ValueError("frr_link_loads_host: a pair names a row outside dsts")
    if n and nscen and V:
        nh = np.asarray(nh, np.int64).reshape(nrows, V)
        backup = np.asarray(backup, np.int64).reshape(nrows, V)
        if (nh >= V).any() or (backup >= V).any() or (backup < -1).any():
            raise ValueError("frr_link_loads_host: a next hop that is no vertex")
        keys, _ = _edge_keys_host(csr)
        ids = np.arange(V, dtype=np.int64)
        rounds = max(1, V).bit_length() + 1
        s_ok = (srcs >= 0) & (srcs < V)
        sc = np.where(s_ok, srcs, 0)
        esrc = np.repeat(ids, np.diff(np.asarray(csr.row_ptr, np.int64)))
        ecol = np.asarray(csr.col, np.int64)
        by_row = [np.nonzero(rows == r)[0] for r in range(nrows)]
        live = [r for r in range(nrows) if by_row[r].size and 0 <= dsts[r] < V]

        def has_link(x, b):
            k = x * V + b
            e = np.minimum(np.searchsorted(keys, k), max(E - 1, 0))
            return E > 0 and keys[e] == k

        def classify(fwd, end, rep):
            """(end kind, repaired) per vertex: end 0 where the walk has none."""
            jump = np.where(end > 0, ids, fwd)
            for _ in range(rounds):
                rep = rep | rep[jump]
                jump = jump[jump]
            return end[jump], rep

        def row_loads(r, fwd, good):
            """[E] loads of the pairs ``good`` of row r over the parents fwd."""
            if not good.size:
                return np.zeros(E, np.uint64)
            return link_loads_host(csr, fwd[None, :].astype(np.int32), INT32,
                                   np.zeros(good.shape[0], np.int64), srcs[good], w[good],
                                   to_root=True)

        base_rows, base_ok = {}, {}
        base = np.zeros(E, np.uint64)
        gone = np.uint64(0)
        for r in range(nrows):
            mine = by_row[r]
            if r not in live:
                gone += w[mine].sum(dtype=np.uint64)
                continue
            d = int(dsts[r])
            fwd = nh[r].copy()
            fwd[d] = -1
            if (fwd == ids).any():
                raise ValueError("frr_link_loads_host: a next hop that is its own vertex")
            end = np.where(ids == d, 1, np.where(fwd < 0, 2, 0))
            got, _ = classify(fwd, end, np.zeros(V, bool))
            if (got == 0).any():
                raise ValueError("frr_link_loads_host: a next-hop row is not an in-tree")
            ok = s_ok[mine] & (got[sc[mine]] == 1)
            base_ok[r] = ok
            base_rows[r] = row_loads(r, np.where(got == 1, fwd, -1), mine[ok])
            base += base_rows[r]
            gone += w[mine[~ok]].sum(dtype=np.uint64)
            status[:, mine[ok]] = 1
        load += base[None, :]
        stat[:, 3] = gone
        for k, failed in enumerate(scen):
            fx, fn = esrc[failed], ecol[failed]
            down = set((fx * V + fn).tolist())
            for r in live:
                d = int(dsts[r])
                hit = np.nonzero((nh[r][fx] == fn) & (fx != d))[0]
                if not hit.size:
                    continue
                items += 1
                mine = by_row[r]
                fwd = nh[r].copy()
                fwd[d] = -1
                end = np.where(ids == d, 1, np.where(fwd < 0, 2, 0))
                rep = np.zeros(V, bool)
                for x in np.unique(fx[hit]).tolist():
                    b = int(backup[r, x])
                    if b >= 0 and not has_link(x, b):
                        raise ValueError("frr_link_loads_host: a backup that is no out-neighbour")
                    if b < 0 or x * V + b in down:
                        fwd[x], end[x] = -1, 3                 # drops
                    elif b == x:
                        fwd[x], end[x] = -1, 4                 # forwards to itself for ever
                    else:
                        fwd[x], rep[x] = b, True
                got, rp = classify(fwd, end, rep)
                ok = base_ok[r]
                cls = got[sc[mine]]
                st = np.where(cls == 1, np.where(rp[sc[mine]], 2, 1),
                              np.where((cls == 2) | (cls == 3), 3, 4))
                st = np.where(ok, st, 0).astype(np.uint8)
                status[k, mine] = st
                for j, code in enumerate((2, 3, 4)):
                    stat[k, j] += w[mine[st == code]].sum(dtype=np.uint64)
                good = mine[(st == 1) | (st == 2)]
                load[k] += row_loads(r, np.where(got == 1, fwd, -1), good) - base_rows[r]
    for k in range(nscen):
        if E and load[k].max() > 0:
            peak[k] = load[k].max()
            peak_edge[k] = int(np.argmax(load[k]))
    return load, stat, status, peak, peak_edge, items


class RouteEngine(object):
    """The GPU route engine of one TopologyDB: HIP device ``device`` (int),
    or the devices of a list (single-process multi-GPU, sources sharded over
    them; tables assembled on the first)."""

    def __init__(self, device=0):
        import torch
        self._torch = torch
        self.ctx = _native.Context(device)
        self.devices = self.ctx.devices
        self.dev = torch.device("cuda", self.devices[0])
        self._loaded = None
        self._csr_dev = None        # (export, row_ptr int64, port int32) on the device
        self._keys_dev = None       # (export, edge keys int64, port int32) on the device
        self._costs = None          # (export, link costs uint32) in force on the context

    # -- plumbing -------------------------------------------------------
    def _ready(self):
        # the library runs on its own stream: torch work that produced its
        # inputs (or last used the memory of its outputs) must be done
        self._torch.cuda.current_stream(self.dev).synchronize()

    def _ids(self, ids):
        return self._torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(self.dev)

    def _empty(self, n, V, dtype):
        return self._torch.empty((n, V), dtype=dtype, device=self.dev)

    def load(self, export):
        if self._loaded is not export:
            self.ctx.upload(export.csr if export.csr.V else empty_csr())
            self._loaded = export
            self._costs = None          # an upload clears the context's link costs

    def csr_device(self, export):
        """(row_ptr int64, port int32) of the export on the device (slot trees
        look their ports up here)."""
        if self._csr_dev is None or self._csr_dev[0] is not export:
            t = self._torch
            c = export.csr
            self._csr_dev = (export, t.from_numpy(np.asarray(c.row_ptr, np.int64)).to(self.dev),
                             t.from_numpy(np.asarray(c.port, np.int32)).to(self.dev))
        return self._csr_dev[1], self._csr_dev[2]

    def edge_keys_device(self, export):
        """(keys int64 = x * V + col per CSR entry, ascending; port int32) on
        the device: the next-hop port lookups of the shortest tables."""
        if self._keys_dev is None or self._keys_dev[0] is not export:
            keys, port = _edge_keys_host(export.csr)
            t = self._torch
            self._keys_dev = (export, t.from_numpy(keys).to(self.dev),
                              t.from_numpy(port).to(self.dev))
        return self._keys_dev[1], self._keys_dev[2]

    # -- tables (device-resident) ---------------------------------------
    def dfs_tables(self, export, srcs, with_hops=True):
        """(parent, port, hops) int32 [S, V] tensors on the primary device."""
        self.load(export)
        t = self._torch
        S, V = len(srcs), export.csr.V
        par = self._empty(S, V, t.int32)
        prt = self._empty(S, V, t.int32)
        hop = self._empty(S, V, t.int32) if with_hops else None
        if S and V:
            ts = self._ids(srcs)
            self._ready()
            self.ctx.dfs_tables_device(ts.data_ptr(), S, par.data_ptr(), prt.data_ptr(),
                                       hop.data_ptr() if hop is not None else 0)
            self.ctx.synchronize()          # also raises on a tripped kernel watchdog
        return par, prt, hop

    def empty_rows(self, n, V, dtypes):
        """Uninitialised [n, V] device tensors of the named dtypes."""
        return tuple(self._empty(n, V, getattr(self._torch, d)) for d in dtypes)

    def dfs_tree_tables(self, export, srcs, layout, out=None):
        """Default-route trees as 4-byte words of ``layout`` (PORT16 / SLOT)
        plus depths (int16 holding u16 for V <= 65535, else int32), from the
        DFS kernels directly (sdnr_dfs_tables_tree) -- into ``out`` (two
        [S, V] tensors, e.g. pool rows) or new tensors."""
        self.load(export)
        t = self._torch
        S, V = len(srcs), export.csr.V
        if out is None:
            out = self.empty_rows(S, V, ("int32", _hops_dtype(V)))
        tree, dep = out
        if S and V:
            ts = self._ids(srcs)
            self._ready()
            self.ctx.dfs_tables_tree_device(
                ts.data_ptr(), S, tree.data_ptr(), dep.data_ptr(),
                _native.TREE_PORT16 if layout == PORT16 else _native.TREE_SLOT,
                dep.element_size())
            self.ctx.synchronize()          # also raises on a tripped kernel watchdog
        return tree, dep

    def pack_trees(self, export, parent, port, layout):
        """int32 tables -> tree words (int32 tensor), sdnr_tree_pack."""
        self.load(export)
        tree = self._torch.empty_like(parent)
        n = parent.numel()
        if n:
            self._ready()
            self.ctx.tree_pack_device(parent.data_ptr(), port.data_ptr(), n, tree.data_ptr(),
                                      _native.TREE_PORT16 if layout == PORT16
                                      else _native.TREE_SLOT)
            self.ctx.synchronize()
        return tree

    def shortest_tables(self, export, dsts):
        """(dist int16 [D, V] holding u16, nh, nh_port int32) on the device."""
        self.load(export)
        t = self._torch
        D, V = len(dsts), export.csr.V
        dist = self._empty(D, V, t.int16)
        nh = self._empty(D, V, t.int32)
        nhp = self._empty(D, V, t.int32)
        if D and V:
            td = self._ids(dsts)
            self._ready()
            self.ctx.shortest_tables_device(td.data_ptr(), D, dist.data_ptr(), nh.data_ptr(),
                                            nhp.data_ptr())
            self.ctx.synchronize()
        return dist, nh, nhp

    def set_link_costs(self, export, cost):
        """Upload the per-link costs (uint32 [E], the export's CSR edge
        order) unless they are the ones in force for this export."""
        self.load(export)
        cost = check_link_costs(export.csr, cost)
        cur = self._costs
        if cur is None or cur[0] is not export or not np.array_equal(cur[1], cost):
            self._costs = None
            self.ctx.set_link_costs(cost)
            self._costs = (export, cost.copy())

    def cost_tables(self, export, cost, dsts, timing=False):
        """Least-cost tables under per-link costs (cost_tables.hip,
        sdnr_cost_tables): (pcost int32 [D, V] holding u32 -- -1 is COST_INF,
        no route --, nh, nh_port int32) on the device, as ``shortest_tables``
        returns its tables."""
        self.set_link_costs(export, cost)
        t = self._torch
        D, V = len(dsts), export.csr.V
        pcost = self._empty(D, V, t.int32)
        nh = self._empty(D, V, t.int32)
        nhp = self._empty(D, V, t.int32)
        if D and V:
            td = self._ids(dsts)
            self._ready()
            self.ctx.cost_tables_device(td.data_ptr(), D, pcost.data_ptr(), nh.data_ptr(),
                                        nhp.data_ptr(), timing=timing)
            self.ctx.synchronize()          # also raises on a tripped sweep bound
        return pcost, nh, nhp

    def ecmp(self, export, dist, rows, srcs):
        """Every shortest route of each (rows[i], srcs[i]) pair, lexicographic
        order (ecmp.hip): list of int32 [n_i, len_i] vertex arrays.  ``dist``
        holds the destination rows the pairs use (device tensor)."""
        self.load(export)
        t = self._torch
        rows = np.asarray(rows, np.int64)
        srcs = np.asarray(srcs, np.int64)
        if rows.size == 0:
            return []
        dist = dist.contiguous()
        R, V = int(dist.shape[0]), export.csr.V
        paths = self._empty(R, V, t.int64)
        self._ready()
        self.ctx.ecmp_counts_device(dist.data_ptr(), R, paths.data_ptr())
        self.ctx.synchronize()
        flat = t.as_tensor(rows * V + srcs, dtype=t.int64, device=self.dev)
        cnt_u = paths.view(-1).index_select(0, flat).cpu().numpy().view(np.uint64)
        if (cnt_u > np.uint64(ECMP_LIMIT)).any():
            raise MemoryError("ECMP set too large to enumerate")
        cnt = cnt_u.astype(np.int64)
        dsel = dist.view(-1).index_select(0, flat).cpu().numpy().view(np.uint16)
        lens = dsel.astype(np.int64) + 1
        total = int(cnt.sum())
        out = []
        if total == 0:
            return [np.zeros((0, 0), np.int32) for _ in range(rows.shape[0])]
        rr = np.repeat(rows, cnt).astype(np.int32)
        ss = np.repeat(srcs, cnt).astype(np.int32)
        starts = np.cumsum(cnt) - cnt
        ranks = (np.arange(total, dtype=np.int64) - np.repeat(starts, cnt)).astype(np.uint64)
        max_len = int(lens[cnt > 0].max())
        d_rr, d_ss = self._ids(rr), self._ids(ss)
        d_rk = t.from_numpy(ranks.view(np.int64)).to(self.dev)
        verts = t.empty((total, max_len), dtype=t.int32, device=self.dev)
        self._ready()
        self.ctx.ecmp_routes_device(dist.data_ptr(), paths.data_ptr(), R, d_rr.data_ptr(),
                                    d_ss.data_ptr(), d_rk.data_ptr(), total, max_len,
                                    verts.data_ptr())
        self.ctx.synchronize()
        verts = verts.cpu().numpy()
        k = 0
        for i in range(rows.shape[0]):
            out.append(verts[k:k + cnt[i], :lens[i]] if cnt[i] else verts[0:0, :0])
            k += int(cnt[i])
        return out

    def expand(self, export, tables, rows, dsts, last_port):
        """Flow entries of many pairs (routes.hip) from device tables:
        (offsets int64 [n+1], switch ids int32, ports int32) on the host.
        ``tables`` = (parent, port, hops) [k, V] of the rows the pairs use
        (int32, or any integer view the cache decodes to)."""
        self.load(export)
        t = self._torch
        par, prt, hop = (a.to(t.int32).contiguous() for a in tables)
        rows = np.asarray(rows, np.int64)
        n = rows.shape[0]
        off = np.zeros(n + 1, np.int64)
        if n == 0:
            return off, np.zeros(0, np.int32), np.zeros(0, np.int32)
        nrows = int(par.shape[0])
        d_rows = self._ids(rows)
        d_dsts = self._ids(dsts)
        d_last = self._ids(last_port)
        d_off = t.empty(n + 1, dtype=t.int64, device=self.dev)
        self._ready()
        self.ctx.route_offsets_device(hop.data_ptr(), d_rows.data_ptr(), d_dsts.data_ptr(), n,
                                      d_off.data_ptr(), nrows=nrows)
        self.ctx.synchronize()
        off = d_off.cpu().numpy()
        total = int(off[-1])
        lp = np.asarray(last_port)
        env = os.environ.get
        if tree_layout(export.csr) == PORT16 and (lp.size == 0 or
                                                  (lp.min() >= 0 and lp.max() < 0xFFFF)) \
                and env("SDNROUTE_ROUTE_OUT", "") != "int32" \
                and env("SDNROUTE_ROUTE_WALK", "") != "serial" and env("SDNROUTE_ROUTE_SEG", "") != "0" \
                and env("SDNROUTE_ROUTE_PACKED", "") != "0":
            # one u32 per entry (switch | port << 16): half the bytes written
            # and copied back; split on the host
            ent = t.empty(max(total, 1), dtype=t.int32, device=self.dev)
            self.ctx.expand_routes_packed_device(par.data_ptr(), prt.data_ptr(), nrows,
                                                 d_rows.data_ptr(), d_dsts.data_ptr(),
                                                 d_last.data_ptr(), n, d_off.data_ptr(),
                                                 ent.data_ptr())
            self.ctx.synchronize()
            e = ent[:total].cpu().numpy().view(np.uint32)
            return off, (e & 0xFFFF).astype(np.int32), (e >> 16).astype(np.int32)
        sw = t.empty(max(total, 1), dtype=t.int32, device=self.dev)
        hp = t.empty(max(total, 1), dtype=t.int32, device=self.dev)
        self.ctx.expand_routes_device(par.data_ptr(), prt.data_ptr(), nrows,
                                      d_rows.data_ptr(), d_dsts.data_ptr(), d_last.data_ptr(), n,
                                      d_off.data_ptr(), sw.data_ptr(), hp.data_ptr())
        self.ctx.synchronize()
        return off, sw[:total].cpu().numpy(), hp[:total].cpu().numpy()

    def dfs_rows_affected(self, export, tree, depth, layout, row_src, diff):
        """bool numpy [rows]: the pool rows (device tree words / int32
        parents ``tree`` and depths ``depth``, [rows, V]; ``row_src`` the
        source of each row, -1 for a free one) that the link changes of
        ``diff`` alter -- one device pass (sdnr_dfs_rows_affected), only
        the verdicts come back."""
        self.load(export)
        t = self._torch
        n = int(tree.shape[0])
        rm = [np.concatenate([diff.removed[0], diff.ported[0]]),
              np.concatenate([diff.removed[1], diff.ported[1]])]
        links = np.concatenate([np.stack(rm, 1).reshape(-1),
                                np.stack([diff.added[0], diff.added[1]], 1).reshape(-1)])
        nrm, nadd = int(rm[0].size), int(diff.added[0].size)
        if n == 0 or nrm + nadd == 0:
            return np.zeros(n, bool)
        tl = self._torch.from_numpy(links.astype(np.int32)).to(self.dev)
        ts = self._ids(row_src)
        out = t.empty(n, dtype=t.uint8, device=self.dev)
        lay = self._layout_code(layout)
        self._ready()
        self.ctx.dfs_rows_affected_device(tree.data_ptr(), depth.data_ptr(), lay,
                                          depth.element_size(), n, ts.data_ptr(),
                                          tl.data_ptr(), nrm, nadd, out.data_ptr())
        self.ctx.synchronize()              # raises if a row was not a tree
        return out.cpu().numpy().astype(bool)

    def _use_costs(self, export, cost):
        """Load ``export`` with the link costs ``cost`` in force; None clears
        the context's costs (every link costs 1)."""
        if cost is None:
            self.load(export)
            if self._costs is not None:
                self._costs = None
                self.ctx.set_link_costs(None)
        else:
            self.set_link_costs(export, cost)

    def _pcost_device(self, pcost):
        """``pcost`` rows as a device tensor (int32 holding u32): a numpy array
        is uploaded, a tensor passes."""
        if _is_np(pcost):
            return self._torch.from_numpy(
                np.ascontiguousarray(_pcost_u32(pcost)).view(np.int32)).to(self.dev)
        return pcost

    @staticmethod
    def _layout_code(layout):
        return {PORT16: _native.TREE_PORT16, SLOT: _native.TREE_SLOT,
                INT32: _native.TREE_INT32}[layout]

    def _upload_pairs(self, off, verts, weights):
        """``_pairs_for_device``'s arrays as device tensors (the u64 weights
        in an int64 tensor, None stays None)."""
        t = self._torch
        d_w = None if weights is None else t.from_numpy(weights.view(np.int64)).to(self.dev)
        return t.from_numpy(off).to(self.dev), t.from_numpy(verts).to(self.dev), d_w

    def link_loads(self, export, tree, layout, rows, dsts, weights=None, to_root=False,
                   timing=False):
        """Per-link loads of a demand routed over device tree rows (loads.hip,
        sdnr_link_loads): numpy uint64 [E] in the CSR's edge order.

        ``tree``: [k, V] int32 device tensor -- tree words of ``layout``
        (PORT16 / SLOT) or int32 parents (INT32); pair i is routed in row
        ``rows[i]`` to dense switch ``dsts[i]`` and weighs ``weights[i]``
        (u64, None: 1).  ``to_root``: the rows are per-destination next-hop
        rows (INT32) and ``dsts`` the pairs' source switches.  The pairs are
        sorted by row here; only the E load words come back."""
        self.load(export)
        t = self._torch
        E = int(export.csr.E)
        rows = np.asarray(rows, np.int64)
        nrows = int(tree.shape[0])
        if rows.size == 0 or nrows == 0 or E == 0:
            return np.zeros(E, np.uint64)
        order, off, d, w = _pairs_for_device(rows, nrows, dsts, int(export.csr.V), weights,
                                             "link_loads")
        tree = tree.contiguous()
        d_off, d_dst, d_w = self._upload_pairs(off, d, w)
        load = t.zeros(E, dtype=t.int64, device=self.dev)
        lay = self._layout_code(layout)
        self._ready()
        self.ctx.link_loads_device(tree.data_ptr(), lay, nrows, d_off.data_ptr(), d_dst.data_ptr(),
                                   _ptr(d_w), load.data_ptr(), to_root=to_root, timing=timing)
        self.ctx.synchronize()              # raises if a row was not a tree
        return load.cpu().numpy().view(np.uint64)

    def multicast_trees(self, export, tree, layout, root, mem_off, mem_row, mem_vertex,
                        weights=None, to_root=False, entries=True, loads=True):
        """Multicast trees of groups over device tree rows (multicast.hip,
        sdnr_multicast_trees): ``(reached uint8 [nmem], ent_off int64
        [ngroups + 1], ent_edge int32, load uint64 [E])`` in numpy, the
        contract of :func:`multicast_trees_host`.

        ``tree``: [k, V] int32 device tensor -- tree words of ``layout``
        (PORT16 / SLOT), int32 parents (INT32) or, with ``to_root``, int32
        next-hop rows.  A count call (which also adds the loads), the prefix
        sum of the counts on the device, then a fill call.  ``entries=False``
        skips the fill (``ent_edge`` is None, ``ent_off`` still the prefix of
        the counts), ``loads=False`` the loads (``load`` is None).  The
        kernel time of the calls made is left in ``last_multicast_ms``."""
        self.load(export)
        t = self._torch
        V, E = int(export.csr.V), int(export.csr.E)
        root = np.ascontiguousarray(root, np.int32).reshape(-1)
        off = np.ascontiguousarray(mem_off, np.int64).reshape(-1)
        mrow = np.ascontiguousarray(mem_row, np.int32).reshape(-1)
        mver = np.ascontiguousarray(mem_vertex, np.int32).reshape(-1)
        ng, nmem = root.shape[0], mrow.shape[0]
        if off.shape[0] != ng + 1 or (ng and (off[0] != 0 or off[-1] != nmem)) or \
                (np.diff(off) < 0).any() or mver.shape[0] != nmem:
            raise ValueError("multicast_trees: mem_off is not the offsets of the members")
        if weights is not None and np.asarray(weights).reshape(-1).shape[0] != ng:
            raise ValueError("multicast_trees: one weight per group")
        reached = np.zeros(nmem, np.uint8)
        ent_off = np.zeros(ng + 1, np.int64)
        none = np.zeros(0, np.int32) if entries else None
        nrows = int(tree.shape[0])
        self.last_multicast_ms = 0.0
        if nmem == 0 or V == 0 or nrows == 0:
            return reached, ent_off, none, (np.zeros(E, np.uint64) if loads else None)
        tree = tree.contiguous()
        d_root = t.from_numpy(root).to(self.dev)
        d_off = t.from_numpy(off).to(self.dev)
        d_row = t.from_numpy(mrow).to(self.dev)
        d_ver = t.from_numpy(mver).to(self.dev)
        d_w = None
        if weights is not None and loads:
            w = np.ascontiguousarray(np.asarray(weights, np.uint64).reshape(-1))
            d_w = t.from_numpy(w.view(np.int64)).to(self.dev)
        d_reach = t.zeros(nmem, dtype=t.uint8, device=self.dev)
        d_cnt = t.zeros(ng, dtype=t.int64, device=self.dev)
        d_load = t.zeros(max(E, 1), dtype=t.int64, device=self.dev) if loads else None
        lay = self._layout_code(layout)
        self._ready()
        self.ctx.multicast_trees_device(
            tree.data_ptr(), lay, nrows, ng, d_root.data_ptr(), d_off.data_ptr(),
            d_row.data_ptr(), d_ver.data_ptr(), _ptr(d_w), d_reach.data_ptr(), d_cnt.data_ptr(),
            0, 0, _ptr(d_load), to_root=to_root, timing=True)
        self.ctx.synchronize()              # raises if a row was not a tree
        self.last_multicast_ms += self.ctx.last_kernel_ms()
        d_eoff = t.zeros(ng + 1, dtype=t.int64, device=self.dev)
        t.cumsum(d_cnt, 0, out=d_eoff[1:])
        ent_off = d_eoff.cpu().numpy()
        ent_edge = none
        if entries and int(ent_off[-1]):
            d_edge = t.empty(int(ent_off[-1]), dtype=t.int32, device=self.dev)
            self._ready()
            self.ctx.multicast_trees_device(
                tree.data_ptr(), lay, nrows, ng, d_root.data_ptr(), d_off.data_ptr(),
                d_row.data_ptr(), d_ver.data_ptr(), 0, 0, 0, d_eoff.data_ptr(),
                d_edge.data_ptr(), 0, to_root=to_root, timing=True)
            self.ctx.synchronize()
            self.last_multicast_ms += self.ctx.last_kernel_ms()
            ent_edge = d_edge.cpu().numpy()
        load = d_load.cpu().numpy().view(np.uint64)[:E] if loads else None
        return d_reach.cpu().numpy(), ent_off, ent_edge, load

    def fair_rates(self, export, tree, layout, rows, verts, mult=None, cap=None, extra=None,
                   to_root=False, timing=False):
        """Max-min fair rates of flows routed over device tree rows
        (fair_rates.hip, sdnr_fair_rates): ``(rate float64 [n], bott int32 [n],
        round int32 [n], level float64 [rounds], used float64 [E + nextra])``
        in the flows' order, bit for bit what ``fair_rates_host`` returns.

        ``tree``, ``layout``, ``rows``, ``to_root`` as in ``link_loads``; flow
        i sits at dense switch ``verts[i]`` of row ``rows[i]``, counts
        ``mult[i]`` times (u64, None: once; the sum stays below 2**53) and is
        also bound by ``extra[i]``: two indices in [E, E + nextra) into
        ``cap``, -1 for none (None: no extras).  ``cap``: float64 [E + nextra]
        positive finite capacities, the links' in the CSR's edge order first
        (None: 1.0 per link, no extras).  The flows are sorted by row here and
        every row stays on the device across the rounds."""
        self.load(export)
        return self._fair_rates_over(
            "fair_rates", export, tree, rows, verts, mult, cap, extra,
            lambda tree, *a: self.ctx.fair_rates_device(tree, self._layout_code(layout), *a,
                                                        to_root=to_root, timing=timing))

    def ecmp_fair_rates(self, export, cost, pcost, rows, srcs, mult=None, cap=None, extra=None,
                        split="route", timing=False):
        """Max-min fair rates of flows split over every least-cost route
        (ecmp_fair_rates.hip, sdnr_ecmp_fair_rates): ``(rate float64 [n], bott
        int32 [n], round int32 [n], level float64 [rounds], used float64 [E +
        nextra])`` in the flows' order, what ``ecmp_fair_rates_host`` returns
        within rounding (bit for bit where every partial sum is exact).

        ``cost``: uint32 [E], uploaded as ``cost_tables`` uploads it; None
        clears the context's costs: every link costs 1 and ``pcost`` holds hop
        counts.  ``pcost``, ``rows``, ``srcs``, ``split`` as in
        ``cost_ecmp_link_loads``; ``mult``, ``cap``, ``extra`` as in
        ``fair_rates``.  The flows are sorted by row here and every row stays
        on the device across the rounds."""
        if split not in SPLITS:
            raise ValueError("split must be 'route' or 'hop'")
        self._use_costs(export, cost)
        return self._fair_rates_over(
            "ecmp_fair_rates", export, self._pcost_device(pcost), rows, srcs, mult, cap, extra,
            lambda pc, *a: self.ctx.ecmp_fair_rates_device(pc, *a, hop=split == "hop",
                                                           timing=timing),
            word=4)

    def _fair_rates_over(self, what, export, table, rows, verts, mult, cap, extra, launch,
                         word=None):
        """``fair_rates`` and ``ecmp_fair_rates`` after their table argument:
        ``table`` is the [k, V] device tensor the flows' rows index (``word``:
        the element size it must have) and ``launch(table pointer, nrows,
        ...)`` the entry point, which returns the number of rounds."""
        t = self._torch
        f = self._fair_flows_device(what, export, table, rows, verts, mult, cap, extra, word)
        n, NE, nextra, nrows, order = f.n, f.NE, f.nextra, f.nrows, f.order
        if order is None:
            return (np.zeros(0, np.float64), np.zeros(0, np.int32), np.zeros(0, np.int32),
                    np.zeros(0, np.float64), np.zeros(NE, np.float64))
        table, d_off, d_x, d_m, d_e, d_cap = f.table, f.d_off, f.d_x, f.d_m, f.d_e, f.d_cap
        max_rounds = min(n, NE)
        rate = t.empty(n, dtype=t.float64, device=self.dev)
        bott = t.empty(n, dtype=t.int32, device=self.dev)
        rnd = t.empty(n, dtype=t.int32, device=self.dev)
        level = t.empty(max_rounds, dtype=t.float64, device=self.dev)
        used = t.zeros(NE, dtype=t.float64, device=self.dev)
        self._ready()
        rounds = launch(
            table.data_ptr(), nrows, d_off.data_ptr(), d_x.data_ptr(), _ptr(d_m), _ptr(d_e),
            d_cap.data_ptr() if NE else 0, nextra, rate.data_ptr(), bott.data_ptr(),
            rnd.data_ptr(), level.data_ptr() if max_rounds else 0, max_rounds,
            used.data_ptr() if NE else 0)
        self.ctx.synchronize()              # raises if a row was no tree / least-cost labelling
        rate, bott, rnd = (_unsorted(a.cpu().numpy(), order) for a in (rate, bott, rnd))
        return rate, bott, rnd, level.cpu().numpy()[:rounds], used.cpu().numpy()

    _FairFlows = collections.namedtuple(
        "_FairFlows", "n NE nextra nrows order table d_off d_x d_m d_e d_cap")

    def _fair_flows_device(self, what, export, table, rows, verts, mult, cap, extra, word=None):
        """The flows of a fair-sharing call, checked (``check_fair_flows``),
        sorted by row and uploaded: what ``_fair_rates_over`` and
        ``fair_times`` launch over.  ``order`` is None when there is no flow
        (nothing was uploaded then)."""
        t = self._torch
        V, E = int(export.csr.V), int(export.csr.E)
        rows = np.asarray(rows, np.int64).reshape(-1)
        n = rows.shape[0]
        if cap is None:
            cap = np.ones(E, np.float64)
        mult_in = mult
        mult, cap, extra_all, nextra = check_fair_flows(E, n, mult, cap, extra)
        NE = E + nextra
        nrows = int(table.shape[0])
        if n == 0 or nrows == 0:
            if n:
                raise ValueError("%s: a pair names a row outside the table" % what)
            return self._FairFlows(n, NE, nextra, nrows, None, table, *([None] * 5))
        order, off, x, m = _pairs_for_device(rows, nrows, verts, V,
                                             None if mult_in is None else mult, what)
        if word is not None and table.element_size() != word:
            raise ValueError("%s: pcost rows are 32-bit" % what)
        table = table.contiguous()
        d_off, d_x, d_m = self._upload_pairs(off, x, m)
        d_e = None
        if extra is not None:
            d_e = t.from_numpy(np.ascontiguousarray(extra_all[order].astype(np.int32))).to(self.dev)
        d_cap = t.from_numpy(cap).to(self.dev)
        return self._FairFlows(n, NE, nextra, nrows, order, table, d_off, d_x, d_m, d_e, d_cap)

    def fair_times(self, export, tree, layout, rows, verts, mult=None, nbytes=1.0, cap=None,
                   extra=None, to_root=False, max_epochs=None, timing=False):
        """Max-min fair completion times of flows routed over device tree rows
        (fair_times.hip, sdnr_fair_times): ``(time float64 [n], epoch int32
        [n], rate0 float64 [n], remaining float64 [n], epoch_time float64
        [epochs], epoch_rounds int32 [epochs], carried float64 [E + nextra])``
        in the flows' order, bit for bit what ``fair_times_host`` returns.

        The flows, ``mult``, ``cap``, ``extra`` and ``to_root`` as in
        ``fair_rates``; ``nbytes``: float64 [n] (or one number for all), the
        size of each of flow i's ``mult[i]`` parallel flows, finite and >= 0;
        ``max_epochs``: stop after that many departures' epochs (None: run to
        the end).  The epochs and their fillings advance on the device; the
        host reads one status word per batch of launches."""
        self.load(export)
        t = self._torch
        f = self._fair_flows_device("fair_times", export, tree, rows, verts, mult, cap, extra)
        n, NE = f.n, f.NE
        nbytes = check_fair_bytes(n, nbytes)
        cap_e = _fair_epoch_cap(n, max_epochs)
        if f.order is None:
            return (np.zeros(0, np.float64), np.zeros(0, np.int32), np.zeros(0, np.float64),
                    np.zeros(0, np.float64), np.zeros(0, np.float64), np.zeros(0, np.int32),
                    np.zeros(NE, np.float64))
        d_b = t.from_numpy(np.ascontiguousarray(nbytes[f.order])).to(self.dev)
        time, rate0, left = (t.empty(n, dtype=t.float64, device=self.dev) for _ in range(3))
        epoch = t.empty(n, dtype=t.int32, device=self.dev)
        e_time = t.empty(cap_e, dtype=t.float64, device=self.dev)
        e_rounds = t.empty(cap_e, dtype=t.int32, device=self.dev)
        carried = t.zeros(NE, dtype=t.float64, device=self.dev)
        self._ready()
        epochs = self.ctx.fair_times_device(
            f.table.data_ptr(), self._layout_code(layout), f.nrows, f.d_off.data_ptr(),
            f.d_x.data_ptr(), _ptr(f.d_m), d_b.data_ptr(), _ptr(f.d_e),
            f.d_cap.data_ptr() if NE else 0, f.nextra, time.data_ptr(), epoch.data_ptr(),
            rate0.data_ptr(), left.data_ptr(), e_time.data_ptr() if cap_e else 0,
            e_rounds.data_ptr() if cap_e else 0, cap_e, carried.data_ptr() if NE else 0,
            to_root=to_root, timing=timing)
        self.ctx.synchronize()              # raises if a row was no tree
        time, epoch, rate0, left = (_unsorted(a.cpu().numpy(), f.order)
                                    for a in (time, epoch, rate0, left))
        return (time, epoch, rate0, left, e_time.cpu().numpy()[:epochs],
                e_rounds.cpu().numpy()[:epochs], carried.cpu().numpy())

    def ecmp_fair_times(self, export, cost, pcost, rows, srcs, mult=None, nbytes=1.0, cap=None,
                        extra=None, split="route", max_epochs=None, timing=False):
        """Max-min fair completion times of flows split over every least-cost
        route (ecmp_fair_times.hip, sdnr_ecmp_fair_times): the 7-tuple of
        ``fair_times`` in the flows' order, what ``ecmp_fair_times_host``
        returns within rounding (bit for bit where every partial sum is
        exact); the epoch count, every flow's epoch and every filling's round
        count are equal unless a decision lies within rounding of the tie
        tolerance 2**-30.

        ``cost``, ``pcost``, ``rows``, ``srcs``, ``split`` as in
        ``ecmp_fair_rates``; ``mult``, ``nbytes``, ``cap``, ``extra`` and
        ``max_epochs`` as in ``fair_times``.  The epochs and their fillings
        advance on the device; the host reads one status word per batch of
        launches."""
        if split not in SPLITS:
            raise ValueError("split must be 'route' or 'hop'")
        self._use_costs(export, cost)
        t = self._torch
        f = self._fair_flows_device("ecmp_fair_times", export, self._pcost_device(pcost), rows,
                                    srcs, mult, cap, extra, word=4)
        n, NE = f.n, f.NE
        nbytes = check_fair_bytes(n, nbytes)
        cap_e = _fair_epoch_cap(n, max_epochs)
        if f.order is None:
            return (np.zeros(0, np.float64), np.zeros(0, np.int32), np.zeros(0, np.float64),
                    np.zeros(0, np.float64), np.zeros(0, np.float64), np.zeros(0, np.int32),
                    np.zeros(NE, np.float64))
        d_b = t.from_numpy(np.ascontiguousarray(nbytes[f.order])).to(self.dev)
        time, rate0, left = (t.empty(n, dtype=t.float64, device=self.dev) for _ in range(3))
        epoch = t.empty(n, dtype=t.int32, device=self.dev)
        e_time = t.empty(cap_e, dtype=t.float64, device=self.dev)
        e_rounds = t.empty(cap_e, dtype=t.int32, device=self.dev)
        carried = t.zeros(NE, dtype=t.float64, device=self.dev)
        self._ready()
        epochs = self.ctx.ecmp_fair_times_device(
            f.table.data_ptr(), f.nrows, f.d_off.data_ptr(), f.d_x.data_ptr(), _ptr(f.d_m),
            d_b.data_ptr(), _ptr(f.d_e), f.d_cap.data_ptr() if NE else 0, f.nextra,
            time.data_ptr(), epoch.data_ptr(), rate0.data_ptr(), left.data_ptr(),
            e_time.data_ptr() if cap_e else 0, e_rounds.data_ptr() if cap_e else 0, cap_e,
            carried.data_ptr() if NE else 0, hop=split == "hop", timing=timing)
        self.ctx.synchronize()              # raises if a row was no least-cost labelling
        time, epoch, rate0, left = (_unsorted(a.cpu().numpy(), f.order)
                                    for a in (time, epoch, rate0, left))
        return (time, epoch, rate0, left, e_time.cpu().numpy()[:epochs],
                e_rounds.cpu().numpy()[:epochs], carried.cpu().numpy())

    def ecmp_link_loads(self, export, dist, rows, srcs, weights=None, split="route",
                        timing=False):
        """Per-link loads of a demand split over every shortest route
        (ecmp_loads.hip, sdnr_ecmp_link_loads): numpy float64 [E] in the CSR's
        edge order.

        ``dist``: [k, V] device tensor of distance rows (int16 holding u16, as
        ``shortest_tables`` and the table cache keep them; rows without pairs
        are skipped); pair i enters at dense switch ``srcs[i]`` of row
        ``rows[i]`` and weighs ``weights[i]`` (u64, None: 1).  ``split``:
        "route" (even over the pair's shortest routes) or "hop" (even over
        each switch's next hops).  The pairs are sorted by row here; only the
        E load words come back.  Sums are f64 atomics: equal to the host
        restatement within rounding, not bit-reproducible."""
        if split not in SPLITS:
            raise ValueError("split must be 'route' or 'hop'")
        self.load(export)
        t = self._torch
        E = int(export.csr.E)
        rows = np.asarray(rows, np.int64)
        nrows = int(dist.shape[0])
        if rows.size == 0 or nrows == 0 or E == 0:
            return np.zeros(E, np.float64)
        order, off, s, w = _pairs_for_device(rows, nrows, srcs, int(export.csr.V), weights,
                                             "ecmp_link_loads")
        if dist.element_size() != 2:
            raise ValueError("ecmp_link_loads: distance rows are 16-bit")
        dist = dist.contiguous()
        d_off, d_src, d_w = self._upload_pairs(off, s, w)
        load = t.zeros(E, dtype=t.float64, device=self.dev)
        self._ready()
        self.ctx.ecmp_link_loads_device(dist.data_ptr(), nrows, d_off.data_ptr(),
                                        d_src.data_ptr(), _ptr(d_w), load.data_ptr(),
                                        hop=split == "hop", timing=timing)
        self.ctx.synchronize()              # raises if a row was no BFS labelling
        return load.cpu().numpy()

    def cost_ecmp_link_loads(self, export, cost, pcost, rows, srcs, weights=None, split="route",
                             timing=False):
        """Per-link loads of a demand split over every least-cost route under
        the per-link costs ``cost`` (cost_ecmp_loads.hip,
        sdnr_cost_ecmp_link_loads): numpy float64 [E] in the CSR's edge order.

        ``cost``: uint32 [E], uploaded as ``cost_tables`` uploads it;
        ``pcost``: [k, V] least-cost rows computed under those costs, a device
        tensor (int32 holding u32, as ``cost_tables`` returns it) or a numpy
        array; rows without pairs are skipped.  Pair i enters at dense switch
        ``srcs[i]`` of row ``rows[i]`` and weighs ``weights[i]`` (u64, None:
        1).  ``split`` as in ``ecmp_link_loads``.  Sums are f64 atomics: equal
        to the host restatement within rounding, not bit-reproducible."""
        if split not in SPLITS:
            raise ValueError("split must be 'route' or 'hop'")
        self.set_link_costs(export, cost)
        t = self._torch
        E = int(export.csr.E)
        rows = np.asarray(rows, np.int64)
        pcost = self._pcost_device(pcost)
        nrows = int(pcost.shape[0])
        if rows.size == 0 or nrows == 0 or E == 0:
            return np.zeros(E, np.float64)
        order, off, s, w = _pairs_for_device(rows, nrows, srcs, int(export.csr.V), weights,
                                             "cost_ecmp_link_loads")
        if pcost.element_size() != 4:
            raise ValueError("cost_ecmp_link_loads: pcost rows are 32-bit")
        pcost = pcost.contiguous()
        d_off, d_src, d_w = self._upload_pairs(off, s, w)
        load = t.zeros(E, dtype=t.float64, device=self.dev)
        self._ready()
        self.ctx.cost_ecmp_link_loads_device(pcost.data_ptr(), nrows, d_off.data_ptr(),
                                             d_src.data_ptr(), _ptr(d_w), load.data_ptr(),
                                             hop=split == "hop", timing=timing)
        self.ctx.synchronize()              # raises if a row was no least-cost labelling
        return load.cpu().numpy()

    def failure_ecmp_link_loads(self, export, cost, dsts, rows, srcs, weights=None,
                                scenarios=(), split="route", timing=False):
        """Link-failure what-if (failure_loads.hip,
        sdnr_failure_ecmp_link_loads): the loads of ``cost_ecmp_link_loads``
        once per failure scenario, nothing uploaded or cached changing: (load
        float64 [nscen, E] in the CSR's edge order, lost float64 [nscen],
        routed bool [nscen, npairs]) on the host.

        ``cost``: uint32 [E] link costs, or None for unit costs (the context's
        costs are then cleared: hop-count ECMP); ``dsts``: the dense
        destination switch of each row; pair i goes from ``srcs[i]`` toward
        ``dsts[rows[i]]`` and weighs ``weights[i]`` (u64, None: 1).
        ``scenarios``: a list of int arrays of failed CSR edge indices; they are
        sorted and deduplicated here (``normalise_scenarios``).  ``lost[k]``:
        the weight that has no route in scenario k (as double); ``routed[k,
        i]``: pair i has one (s == d counts).  ``split`` as in
        ``ecmp_link_loads``.  One launch for all scenarios and rows; sums are
        f64 atomics: equal to ``failure_ecmp_link_loads_host`` within rounding,
        not bit-reproducible."""
        if split not in SPLITS:
            raise ValueError("split must be 'route' or 'hop'")
        self._use_costs(export, cost)
        t = self._torch
        V, E = int(export.csr.V), int(export.csr.E)
        scen = normalise_scenarios(scenarios, E)
        nscen = len(scen)
        rows = np.asarray(rows, np.int64)
        n = int(rows.shape[0])
        d = np.asarray(dsts, np.int64)
        nrows = int(d.shape[0])
        load = np.zeros((nscen, E), np.float64)
        lost = np.zeros(nscen, np.float64)
        routed = np.zeros((nscen, n), bool)
        if n == 0 or nrows == 0 or nscen == 0 or V == 0:
            return load, lost, routed
        order, off, s, w = _pairs_for_device(rows, nrows, srcs, V, weights,
                                             "failure_ecmp_link_loads", "dsts")
        d = np.where((d < 0) | (d >= V), -1, d).astype(np.int32)
        soff = np.zeros(nscen + 1, np.int64)
        np.cumsum([a.shape[0] for a in scen], out=soff[1:])
        edges = np.concatenate(scen + [np.zeros(1, np.int32)]).astype(np.int32)
        d_dst = t.from_numpy(d).to(self.dev)
        d_off, d_src, d_w = self._upload_pairs(off, s, w)
        d_soff = t.from_numpy(soff).to(self.dev)
        d_edges = t.from_numpy(edges).to(self.dev)
        d_load = t.zeros((nscen, max(E, 1)), dtype=t.float64, device=self.dev)
        d_lost = t.zeros(nscen, dtype=t.float64, device=self.dev)
        d_routed = t.zeros((nscen, n), dtype=t.uint8, device=self.dev)
        self._ready()
        self.ctx.failure_ecmp_link_loads_device(
            d_dst.data_ptr(), nrows, d_off.data_ptr(), d_src.data_ptr(), _ptr(d_w), nscen,
            d_soff.data_ptr(), d_edges.data_ptr(), d_load.data_ptr(), d_lost.data_ptr(),
            d_routed.data_ptr(), hop=split == "hop", timing=timing)
        self.ctx.synchronize()              # raises on a bad scenario list
        load = d_load[:, :E].cpu().numpy()
        routed = _unsorted(d_routed.cpu().numpy().astype(bool), order)
        return load, d_lost.cpu().numpy(), routed

    def whatif_ecmp_link_loads(self, export, cost, dsts, rows, srcs, weights=None, scenarios=(),
                               split="route", capacity=None, loads=True, reach=True,
                               timing=False, table_budget=None):
        """Link-cost what-if (whatif_loads.hip, sdnr_whatif_ecmp_link_loads):
        the loads of ``cost_ecmp_link_loads`` once per cost scenario, nothing
        uploaded or cached changing: (load float64 [nscen, E], lost float64
        [nscen], routed bool [nscen, npairs], peak float64 [nscen], peak_edge
        int32 [nscen]) on the host.

        ``cost``, ``dsts``, ``rows``, ``srcs``, ``weights``, ``split`` as in
        ``failure_ecmp_link_loads``.  ``scenarios``: a list of ``(edges,
        costs)`` -- CSR edge indices and the cost each takes in that scenario,
        COST_INF: the link is down -- checked and sorted here
        (``normalise_cost_scenarios``).  ``capacity``: float64 [E] or None (1.0
        per link); ``peak[k]`` is the largest ``load[k, e] / capacity[e]`` and
        ``peak_edge[k]`` the first link that attains it (0.0 and -1 without
        load), reduced on the device.

        The scenarios are processed in chunks whose load planes fit
        ``table_budget`` bytes (None: DEFAULT_TABLE_BUDGET), 8 E + npairs bytes
        per scenario, in one device buffer reused across the chunks.
        ``loads=False``: the planes never leave the device; load and routed
        come back as None -- what a search over costs needs is one number per
        candidate.  ``reach=False``: lost and routed are not computed (finite
        costs never change reachability) and come back as None.  Sums are f64
        atomics: equal to ``whatif_ecmp_link_loads_host`` within rounding, not
        bit-reproducible."""
        if split not in SPLITS:
            raise ValueError("split must be 'route' or 'hop'")
        self._use_costs(export, cost)
        t = self._torch
        V, E = int(export.csr.V), int(export.csr.E)
        scen = normalise_cost_scenarios(scenarios, export.csr)
        cap = _check_capacity(capacity, E)
        nscen = len(scen)
        rows = np.asarray(rows, np.int64)
        n = int(rows.shape[0])
        d = np.asarray(dsts, np.int64)
        nrows = int(d.shape[0])
        load = np.zeros((nscen, E), np.float64) if loads else None
        lost = np.zeros(nscen, np.float64) if reach else None
        routed = np.zeros((nscen, n), bool) if loads and reach else None
        peak = np.zeros(nscen, np.float64)
        peak_edge = np.full(nscen, -1, np.int32)
        if n == 0 or nrows == 0 or nscen == 0 or V == 0:
            return load, lost, routed, peak, peak_edge
        order, off, s, w = _pairs_for_device(rows, nrows, srcs, V, weights,
                                             "whatif_ecmp_link_loads", "dsts")
        d = np.where((d < 0) | (d >= V), -1, d).astype(np.int32)
        d_dst = t.from_numpy(d).to(self.dev)
        d_off, d_src, d_w = self._upload_pairs(off, s, w)
        d_cap = None if cap is None else t.from_numpy(cap).to(self.dev)
        budget = DEFAULT_TABLE_BUDGET if table_budget is None else int(table_budget)
        step = min(nscen, max(1, budget // max(1, 8 * E + n)))
        d_load = t.empty((step, max(E, 1)), dtype=t.float64, device=self.dev)
        d_lost = t.empty(step, dtype=t.float64, device=self.dev) if reach else None
        d_routed = t.empty((step, n), dtype=t.uint8, device=self.dev) if routed is not None \
            else None
        d_peak = t.empty(step, dtype=t.float64, device=self.dev)
        d_pedge = t.empty(step, dtype=t.int32, device=self.dev)
        self._ready()
        for c0 in range(0, nscen, step):
            part = scen[c0:c0 + step]
            m = len(part)
            soff = np.zeros(m + 1, np.int64)
            np.cumsum([a.shape[0] for a, _ in part], out=soff[1:])
            edges = np.concatenate([a for a, _ in part] + [np.zeros(1, np.int32)])
            costs = np.concatenate([c for _, c in part] + [np.zeros(1, np.uint32)])
            d_soff = t.from_numpy(soff).to(self.dev)
            d_edges = t.from_numpy(edges.astype(np.int32)).to(self.dev)
            d_costs = t.from_numpy(costs.astype(np.uint32).view(np.int32)).to(self.dev)
            d_load.zero_()
            if d_lost is not None:
                d_lost.zero_()
            if d_routed is not None:
                d_routed.zero_()
            self.ctx.whatif_ecmp_link_loads_device(
                d_dst.data_ptr(), nrows, d_off.data_ptr(), d_src.data_ptr(), _ptr(d_w), m,
                d_soff.data_ptr(), d_edges.data_ptr(), d_costs.data_ptr(), d_load.data_ptr(),
                _ptr(d_lost), _ptr(d_routed), _ptr(d_cap), d_peak.data_ptr(), d_pedge.data_ptr(),
                hop=split == "hop", timing=timing)
            self.ctx.synchronize()          # raises on a bad override list or capacity
            peak[c0:c0 + m] = d_peak[:m].cpu().numpy()
            peak_edge[c0:c0 + m] = d_pedge[:m].cpu().numpy()
            if reach:
                lost[c0:c0 + m] = d_lost[:m].cpu().numpy()
            if loads:
                load[c0:c0 + m] = d_load[:m, :E].cpu().numpy()
            if routed is not None:
                routed[c0:c0 + m] = _unsorted(d_routed[:m].cpu().numpy().astype(bool), order)
        return load, lost, routed, peak, peak_edge

    def lfa_tables(self, export, cost, pcost_all, dsts, link_only=False, timing=False):
        """Loop-free alternate next hops (lfa_tables.hip, sdnr_lfa_tables):
        (backup, backup_port int32 [D, V], kind uint8 [D, V] on the device,
        counts uint32 [D, 4] on the host) for the destinations ``dsts``, as
        ``lfa_tables_host`` defines them.

        ``cost``: uint32 [E] link costs, or None for unit costs (the context's
        costs are then cleared); ``pcost_all``: the [V, V] all-pairs least-cost
        table under those costs, row v = destination v -- a device tensor
        (int32 holding u32, as ``cost_tables`` returns it) or a numpy array,
        which is uploaded.  ``link_only``: SDNR_LFA_LINK_ONLY.  A destination
        outside [0, V) gives an empty row.  V above ``LFA_MAX_V`` raises."""
        self._use_costs(export, cost)
        t = self._torch
        V = int(export.csr.V)
        d = np.asarray(dsts, np.int64)
        D = int(d.shape[0])
        d = np.where((d < 0) | (d >= V), -1, d).astype(np.int32)
        pcost_all = self._pcost_device(pcost_all)
        if tuple(pcost_all.shape) != (V, V) or pcost_all.element_size() != 4:
            raise ValueError("pcost_all is the [V, V] 4-byte all-pairs table (row v: "
                             "destination v)")
        pcost_all = pcost_all.contiguous()
        backup = self._empty(D, V, t.int32)
        bport = self._empty(D, V, t.int32)
        kind = self._empty(D, V, t.uint8)
        counts = t.zeros((D, 4), dtype=t.int32, device=self.dev)
        if D and V:
            td = t.from_numpy(d).to(self.dev)
            self._ready()
            self.ctx.lfa_tables_device(pcost_all.data_ptr(), td.data_ptr(), D, backup.data_ptr(),
                                       bport.data_ptr(), kind.data_ptr(), counts.data_ptr(),
                                       link_only=link_only, timing=timing)
            self.ctx.synchronize()          # raises on a row that is no least-cost labelling
        return backup, bport, kind, counts.cpu().numpy().view(np.uint32)

    def remote_lfa(self, export, cost, pcost_all, verts=None, timing=False):
        """Remote loop-free alternates (remote_lfa.hip, sdnr_remote_lfa): (pq,
        via, via_port int32 [E], tunnel_cost uint64 [E], kind uint8 [E], counts
        uint32 [n, 4]) on the host, as ``remote_lfa_host`` defines them, for
        the out-links of the source vertices ``verts`` (None: every vertex).

        ``cost`` and ``pcost_all`` as in ``lfa_tables``.  The entries of links
        whose source is not listed read -1 / -1 / -1 / 0 / 0; a vertex outside
        [0, V) is an empty unit.  V above ``LFA_MAX_V`` raises."""
        self._use_costs(export, cost)
        t = self._torch
        V, E = int(export.csr.V), int(export.csr.E)
        v = np.arange(V, dtype=np.int64) if verts is None else np.asarray(verts, np.int64)
        n = int(v.shape[0])
        v = np.where((v < 0) | (v >= V), -1, v).astype(np.int32)
        pcost_all = self._pcost_device(pcost_all)
        if tuple(pcost_all.shape) != (V, V) or pcost_all.element_size() != 4:
            raise ValueError("pcost_all is the [V, V] 4-byte all-pairs table (row v: "
                             "destination v)")
        pcost_all = pcost_all.contiguous()
        i32 = t.full((3, max(E, 1)), -1, dtype=t.int32, device=self.dev)
        tcost = t.zeros(max(E, 1), dtype=t.int64, device=self.dev)
        kind = t.zeros(max(E, 1), dtype=t.uint8, device=self.dev)
        counts = t.zeros((n, 4), dtype=t.int32, device=self.dev)
        if n and V:
            tv = t.from_numpy(v).to(self.dev)
            self._ready()
            self.ctx.remote_lfa_device(pcost_all.data_ptr(), tv.data_ptr(), n, i32[0].data_ptr(),
                                       i32[1].data_ptr(), i32[2].data_ptr(), tcost.data_ptr(),
                                       kind.data_ptr(), counts.data_ptr(), timing=timing)
            self.ctx.synchronize()
        h = i32[:, :E].cpu().numpy()
        return (h[0].copy(), h[1].copy(), h[2].copy(), tcost[:E].cpu().numpy().view(np.uint64),
                kind[:E].cpu().numpy(), counts.cpu().numpy().view(np.uint32))

    def frr_link_loads(self, export, nh, backup, dsts, rows, srcs, weights=None, scenarios=(),
                       planes=True, timing=False, table_budget=None):
        """Fast-reroute what-if (frr_loads.hip, sdnr_frr_link_loads): what the
        links carry while the backup next hops forward, once per failure
        scenario, nothing uploaded or cached changing: ``(load uint64 [nscen,
        E], stat uint64 [nscen, 4], status uint8 [nscen, npairs], peak uint64
        [nscen], peak_edge int32 [nscen], items)`` on the host, as
        ``frr_link_loads_host`` defines them.

        ``nh``, ``backup``: int32 [nrows, V] next-hop and backup rows toward
        ``dsts`` (device tensors or numpy; ``cost_tables`` / ``lfa_tables``
        write them); pair i goes from ``srcs[i]`` toward ``dsts[rows[i]]`` and
        weighs ``weights[i]`` (u64, None: 1).  ``scenarios``: a list of int
        arrays of failed CSR edge indices, sorted and deduplicated here.  The
        scenarios are processed in chunks whose planes fit ``table_budget``
        bytes (None: DEFAULT_TABLE_BUDGET), 8 E + npairs bytes per scenario, in
        one device buffer reused across the chunks.  ``planes=False``: the load
        planes never leave the device and no status is written; load and
        status come back as None -- an N-1 sweep wants the numbers per
        scenario.  ``items``: the (scenario, row) items the kernel recomputed.
        Exact: u64 sums."""
        self.load(export)
        t = self._torch
        V, E = int(export.csr.V), int(export.csr.E)
        if V > FRR_MAX_V:
            raise ValueError("frr_link_loads keeps a row in LDS: %d switches are above its %d"
                             % (V, FRR_MAX_V))
        scen = normalise_scenarios(scenarios, E)
        nscen = len(scen)
        rows = np.asarray(rows, np.int64)
        n = int(rows.shape[0])
        d = np.asarray(dsts, np.int64)
        nrows = int(d.shape[0])
        load = np.zeros((nscen, E), np.uint64) if planes else None
        status = np.zeros((nscen, n), np.uint8) if planes else None
        stat = np.zeros((nscen, 4), np.uint64)
        peak = np.zeros(nscen, np.uint64)
        peak_edge = np.full(nscen, -1, np.int32)
        if n == 0 or nrows == 0 or nscen == 0 or V == 0:
            return load, stat, status, peak, peak_edge, 0
        order, off, s, w = _pairs_for_device(rows, nrows, srcs, V, weights, "frr_link_loads",
                                             "dsts")
        d = np.where((d < 0) | (d >= V), -1, d).astype(np.int32)

        def table(a, what):
            if _is_np(a):
                a = t.from_numpy(np.ascontiguousarray(a, np.int32)).to(self.dev)
            if tuple(a.shape) != (nrows, V) or a.dtype != t.int32:
                raise ValueError("frr_link_loads: %s is int32 [%d, %d]" % (what, nrows, V))
            return a.contiguous()

        d_nh, d_bk = table(nh, "nh"), table(backup, "backup")
        d_dst = t.from_numpy(d).to(self.dev)
        d_off, d_src, d_w = self._upload_pairs(off, s, w)
        budget = DEFAULT_TABLE_BUDGET if table_budget is None else int(table_budget)
        step = min(nscen, max(1, budget // max(1, 8 * E + n)))
        d_load = t.empty((step, max(E, 1)), dtype=t.int64, device=self.dev)
        d_stat = t.empty((step, 4), dtype=t.int64, device=self.dev)
        d_status = t.empty((step, n), dtype=t.uint8, device=self.dev) if planes else None
        d_peak = t.empty(step, dtype=t.int64, device=self.dev)
        d_pedge = t.empty(step, dtype=t.int32, device=self.dev)
        items = 0
        self._ready()
        for c0 in range(0, nscen, step):
            part = scen[c0:c0 + step]
            m = len(part)
            soff = np.zeros(m + 1, np.int64)
            np.cumsum([a.shape[0] for a in part], out=soff[1:])
            edges = np.concatenate(part + [np.zeros(1, np.int32)]).astype(np.int32)
            d_soff = t.from_numpy(soff).to(self.dev)
            d_edges = t.from_numpy(edges).to(self.dev)
            d_load.zero_()
            d_stat.zero_()
            if d_status is not None:
                d_status.zero_()
            self.ctx.frr_link_loads_device(
                d_dst.data_ptr(), d_nh.data_ptr(), d_bk.data_ptr(), nrows, d_off.data_ptr(),
                d_src.data_ptr(), _ptr(d_w), m, d_soff.data_ptr(), d_edges.data_ptr(),
                d_load.data_ptr(), d_stat.data_ptr(), _ptr(d_status), d_peak.data_ptr(),
                d_pedge.data_ptr(), timing=timing)
            self.ctx.synchronize()          # raises on a bad row, backup or scenario list
            items += self.ctx.last_frr_items()
            stat[c0:c0 + m] = d_stat[:m].cpu().numpy().view(np.uint64)
            peak[c0:c0 + m] = d_peak[:m].cpu().numpy().view(np.uint64)
            peak_edge[c0:c0 + m] = d_pedge[:m].cpu().numpy()
            if planes:
                load[c0:c0 + m] = d_load[:m, :E].cpu().numpy().view(np.uint64)
                status[c0:c0 + m] = _unsorted(d_status[:m].cpu().numpy(), order)
        return load, stat, status, peak, peak_edge, items

    def widest_tables(self, export, cost, pcost, util, dsts, timing=False):
        """Least-loaded tables inside the least-cost DAG (widest_tables.hip,
        sdnr_widest_tables): (bott int32 [D, V] holding u32 -- -1 is
        0xFFFFFFFF, no route --, nh, nh_port int32) on the device, as
        ``cost_tables`` returns its tables and as ``widest_tables_host``
        defines them.

        ``cost``: uint32 [E] link costs, or None for unit costs (the context's
        costs are then cleared); ``pcost``: the [D, V] least-cost rows of
        ``dsts`` under those costs -- a device tensor (int32 holding u32, as
        ``cost_tables`` returns it) or a numpy array, which is uploaded;
        ``util``: uint32 [E] link utilisations in [0, UTIL_MAX].  A destination
        outside [0, V) gives an empty row."""
        self._use_costs(export, cost)
        t = self._torch
        V = int(export.csr.V)
        util = check_link_utilisation(export.csr, util)
        d = np.asarray(dsts, np.int64)
        D = int(d.shape[0])
        d = np.where((d < 0) | (d >= V), -1, d).astype(np.int32)
        pcost = self._pcost_device(pcost)
        if tuple(pcost.shape) != (D, V) or pcost.element_size() != 4:
            raise ValueError("pcost holds one 4-byte [V] row per destination")
        pcost = pcost.contiguous()
        bott = self._empty(D, V, t.int32)
        nh = self._empty(D, V, t.int32)
        nhp = self._empty(D, V, t.int32)
        if D and V:
            td = t.from_numpy(d).to(self.dev)
            tu = t.from_numpy(util.view(np.int32)).to(self.dev)
            self._ready()
            self.ctx.widest_tables_device(pcost.data_ptr(), tu.data_ptr(), td.data_ptr(), D,
                                          bott.data_ptr(), nh.data_ptr(), nhp.data_ptr(),
                                          timing=timing)
            self.ctx.synchronize()          # raises on a row that is no least-cost labelling
        return bott, nh, nhp

    def edge_ports(self, ends, ports):
        """Flood-port mask (sdnr_edge_ports, reference topology.py:150-155):
        bool [n] -- ``ports`` keys that are no link end (``ends`` sorted)."""
        return self.ctx.edge_ports(ends, ports)

    def close(self):
        self.ctx.close()


class _Pool(object):
    """Table rows of one route mode in a fixed-capacity store.

    ``arrays`` is a tuple of [capacity, V] tables (device tensors or numpy);
    a row lives in a slot, ``row`` maps vertex -> slot, ``lru`` orders the
    vertices oldest first.  Adding takes slots from the free list (evicting
    the oldest unprotected rows when the budget is full), dropping gives
    them back and refills them with the ``blank`` row (all unreached), so a
    test over the whole store never sees garbage.  The store is allocated
    once, min(cap, V) rows, on first use; it is never grown, concatenated,
    re-indexed or copied."""

    def __init__(self, budget, row_bytes, blanks):
        self.budget = budget
        self.row_bytes = row_bytes
        self.blanks = blanks                   # fill value per table
        self.arrays = None
        self.size = 0                          # allocated slots
        self.row = {}
        self.lru = collections.OrderedDict()
        self.free = []
        self.host = collections.OrderedDict()  # vertex -> host row tuple (LRU)

    def __contains__(self, v):
        return v in self.row

    def __len__(self):
        return len(self.row)

    def cap(self):
        """Rows the budget holds (at least one)."""
        return max(1, self.budget // self.row_bytes) if self.row_bytes else 1 << 62

    def tables(self):
        return self.arrays

    def slot_vertices(self):
        """int64 numpy [size]: vertex of every slot, -1 for free ones."""
        s = np.full(self.size, -1, np.int64)
        if self.row:
            s[np.fromiter(self.row.values(), np.int64, len(self.row))] = \
                np.fromiter(self.row.keys(), np.int64, len(self.row))
        return s

    def _grow(self, need, like):
        """Make at least ``need`` slots exist.  The first call allocates the
        whole store -- min(cap, V) rows: a graph has at most V distinct rows
        -- so it never grows again (and never holds more than the budget)."""
        if need <= self.size:
            return
        V = int(like[0].shape[1]) if like[0].ndim > 1 else 1
        new = max(need, min(self.cap(), V))
        fresh = []
        for a, b in zip(like, self.blanks):
            shape = (new,) + tuple(a.shape[1:])
            if _is_np(a):
                z = np.full(shape, b, a.dtype)
            else:
                z = _torch().full(shape, b, dtype=a.dtype, device=a.device)
            fresh.append(z)
        if self.arrays is not None:
            for z, a in zip(fresh, self.arrays):
                z[:self.size] = a
        self.free.extend(range(new - 1, self.size - 1, -1))   # lowest slot popped first
        self.arrays = tuple(fresh)
        self.size = new

    def make_room(self, n, protect):
        """Evict the oldest rows not in ``protect`` until n more fit."""
        over = len(self.row) + n - self.cap()
        if over <= 0:
            return
        out = []
        for v in self.lru:
            if over <= 0:
                break
            if v not in protect:
                out.append(v)
                over -= 1
        self.drop(out)

    def drop(self, verts):
        """Give the slots of ``verts`` back (blank rows)."""
        slots = [self.row.pop(v) for v in verts if v in self.row]
        for v in verts:
            self.lru.pop(v, None)
            self.host.pop(v, None)
        if not slots:
            return
        self._blank(np.asarray(slots, np.int64))
        self.free.extend(slots)

    def _blank(self, idx):
        """Rows ``idx`` back to all-unreached (every free slot is blank)."""
        for a, b in zip(self.arrays, self.blanks):
            if _is_np(a):
                a[idx] = b
            else:
                a[_torch().as_tensor(idx, device=a.device)] = b

    def add(self, verts, tabs=None, fill=None, like=None):
        """Store rows for ``verts`` (room was made): either ``tabs`` ([n, V]
        each, already computed) or ``fill(out)``, which computes them into
        ``out`` -- views of the store itself when the slots taken are
        contiguous (the kernels write their rows in place: no copy), else
        fresh [n, V] arrays copied in afterwards.  ``like``: [0, V] arrays of
        the tables' types (the first call allocates the store from them)."""
        if not verts:
            return
        self._grow(len(self.row) + len(verts), tabs if tabs is not None else like)
        slots = [self.free.pop() for _ in verts]
        idx = np.asarray(slots, np.int64)
        contiguous = bool(np.all(np.diff(idx) == 1))
        n = len(slots)
        if tabs is None:
            try:
                if contiguous:
                    fill(tuple(a[slots[0]:slots[0] + n] for a in self.arrays))
                else:
                    tabs = tuple(_empty_rows(a, n) for a in self.arrays)
                    fill(tabs)
            except BaseException:
                # the kernels may have written part of the rows in place:
                # blank the slots before they go back
                self._blank(idx)
                self.free.extend(slots)
                raise
        if tabs is not None:
            for a, t in zip(self.arrays, tabs):
                if contiguous:
                    a[slots[0]:slots[0] + n] = t
                elif _is_np(a):
                    a[idx] = t
                else:
                    a.index_copy_(0, _torch().as_tensor(idx, device=a.device), t)
        for v, s in zip(verts, slots):
            self.row[v] = s
            self.lru[v] = None

    def host_row(self, v):
        """One row of every table, on the host (small LRU)."""
        hit = self.host.get(v)
        if hit is not None:
            self.host.move_to_end(v)
            return hit
        r = self.row[v]
        rows = tuple(_host(a[r:r + 1])[0] for a in self.arrays)
        self.host[v] = rows
        if len(self.host) > HOST_ROW_CACHE:
            self.host.popitem(last=False)
        return rows


class TableCache(object):
    """Per-graph cache of computed table rows, keyed by dense vertex id, in
    compact pools (module docstring).  ``retarget`` follows a graph change
    over the same vertex set in place: the rows the change can alter are
    dropped (:mod:`sdnmpi_amd.incremental`), the rest stay in their slots."""

    def __init__(self, export, budget=None):
        self.export = export
        b = DEFAULT_TABLE_BUDGET if budget is None else int(budget)
        csr = export.csr
        self.layout = tree_layout(csr)
        self.V = csr.V
        dfs_blank = (-1, -1, -1) if self.layout == INT32 else (-1, -1)
        self.dfs = _Pool(b, dfs_row_bytes(csr), dfs_blank)
        self.sp = _Pool(b, sp_row_bytes(csr), (-1, -1))
        self.rows_computed = 0     # rows sent to the GPU (both modes)
        self.rows_inherited = 0    # rows kept across a graph change

    # vertex -> row (slot) maps
    @property
    def dfs_row(self):
        return self.dfs.row

    @property
    def sp_row(self):
        return self.sp.row

    # -- decoded views ---------------------------------------------------
    def dfs_parent_hops(self):
        """(parent, hops) read views over the whole DFS pool (Wide)."""
        a = self.dfs.tables()
        if a is None:
            return None, None
        if self.layout == INT32:
            return Wide(a[0], "int"), Wide(a[2], "int")
        return Wide(a[0], self.layout), Wide(a[1], "u16" if self.V <= 0xFFFF else "int")

    def dfs_int32(self, slots, engine=None):
        """(parent, port, hops) int32-valued int64 tables of pool slots
        ``slots`` (array type of the pool)."""
        a = self.dfs.tables()
        sel = [_take(x, slots) for x in a]
        if self.layout == INT32:
            return tuple(_i64(x) for x in sel)
        par = tree_parent(sel[0], self.layout)
        if self.layout == PORT16:
            prt = tree_port(sel[0], PORT16, None, None)
        elif _is_np(sel[0]):
            c = self.export.csr
            prt = tree_port(sel[0], SLOT, np.asarray(c.row_ptr, np.int64), c.port, par)
        else:
            rp, pt = engine.csr_device(self.export)
            prt = tree_port(sel[0], SLOT, rp, pt, par)
        hop = _u16(sel[1]) if self.V <= 0xFFFF else _i64(sel[1])
        return par, prt, hop

    def dfs_host_row(self, v):
        """(parent, port) int64 numpy rows of source v (host LRU)."""
        row = self.dfs.host_row(v)
        if self.layout == INT32:
            return row[0], row[1]
        c = self.export.csr
        par = tree_parent(row[0], self.layout)
        return par, tree_port(row[0], self.layout, np.asarray(c.row_ptr, np.int64), c.port, par)

    def sp_dist_host_row(self, d):
        """u16 distances to destination d (host LRU)."""
        return np.asarray(self.sp.host_row(d)[0]).view(np.uint16)

    def sp_views(self):
        """(dist, nh) read views over the whole shortest pool (Wide)."""
        a = self.sp.tables()
        if a is None:
            return None, None
        return Wide(a[0], "u16raw"), Wide(a[1], "u16" if self.V <= 0xFFFF else "int")

    def sp_decoded(self, slots, engine=None):
        """(dist u16, nh int32, nh_port int32) numpy rows of pool slots.  The
        next hop's port -- ``links[x][nh].src.port_no``, the CSR port of edge
        (x, nh) -- is looked up where the rows live (on the device for a
        device pool), so only the three output planes cross to the host."""
        a = self.sp.tables()
        d = _take(a[0], slots)
        nh = _take(a[1], slots)
        nh = _u16(nh) if self.V <= 0xFFFF else _i64(nh)
        if _is_np(nh):
            keys, port = _edge_keys_host(self.export.csr)
        else:
            keys, port = engine.edge_keys_device(self.export)
        nhp = _next_hop_port(nh, keys, port, self.V)
        return (_host(d).view(np.uint16), _host(nh).astype(np.int32),
                _host(nhp).astype(np.int32))

    # -- graph changes ---------------------------------------------------
    def retarget(self, export, diff, engine=None):
        """Follow a link change over the same vertex set: drop the rows
        ``diff`` can alter (tests run where the tables live), keep the rest.
        Returns False when the compact layout no longer fits the new graph
        (the caller starts a new cache)."""
        from .incremental import dfs_rows_affected, sp_rows_affected
        if tree_layout(export.csr) != self.layout:
            return False
        self.export = export
        if self.dfs.row:
            verts = self.dfs.slot_vertices()
            a = self.dfs.tables()
            if engine is not None and not _is_np(a[0]):
                # the device pool: one kernel climbs the trees (incremental.hip)
                hit = engine.dfs_rows_affected(export, a[0], a[-1], self.layout, verts, diff)
            else:
                par, hop = self.dfs_parent_hops()
                hit = np.asarray(dfs_rows_affected(par, hop, verts, diff), bool)
            hit &= verts >= 0
            self.dfs.drop(verts[hit].tolist())
            if self.layout == SLOT:
                self._reslot(diff)
            self.rows_inherited += len(self.dfs.row)
        if self.sp.row:
            dist, nh = self.sp_views()
            verts = self.sp.slot_vertices()
            hit = np.asarray(sp_rows_affected(dist, nh, diff), bool) & (verts >= 0)
            self.sp.drop(verts[hit].tolist())
            self.rows_inherited += len(self.sp.row)
        self.dfs.host.clear()
        self.sp.host.clear()
        return True

    RESLOT_ROWS = 256             # pool rows per re-slot pass (bounded temporaries)

    def _reslot(self, diff):
        """Slot trees name a position in the parent's CSR row, and a link
        added to or removed from row u moves the later positions of row u.
        The rows kept across the change are still the right trees (the row
        tests above are about the tree, not the encoding), so every kept
        entry whose parent's row changed gets its slot re-derived from the
        new CSR: the position of (parent, v) in the new row of the parent.
        The edge exists: a kept tree's edges are unaffected by the change."""
        rows_changed = np.unique(np.concatenate([diff.removed[0], diff.added[0]]))
        a = self.dfs.tables()
        if a is None or rows_changed.size == 0 or not self.dfs.row:
            return
        csr = self.export.csr
        V = csr.V
        rp = np.asarray(csr.row_ptr, np.int64)
        # keys (p * V + v) -> global edge index, for the changed rows only
        lo, hi = rp[rows_changed], rp[rows_changed + 1]
        eidx = np.concatenate([np.arange(s, e, dtype=np.int64) for s, e in zip(lo, hi)]) \
            if rows_changed.size else np.zeros(0, np.int64)
        src = np.repeat(rows_changed.astype(np.int64), hi - lo)
        keys = src * V + np.asarray(csr.col, np.int64)[eidx]     # ascending: rows sorted
        changed = np.zeros(V, bool)
        changed[rows_changed] = True
        tree = a[0]
        used = np.sort(np.fromiter(self.dfs.row.values(), np.int64, len(self.dfs.row)))
        if _is_np(tree):
            xp_keys, xp_e, xp_rp, xp_ch = keys, eidx, rp, changed
        else:
            t = _torch()
            dv = tree.device
            xp_keys = t.from_numpy(keys).to(dv)
            xp_e = t.from_numpy(eidx).to(dv)
            xp_rp = t.from_numpy(rp).to(dv)
            xp_ch = t.from_numpy(changed).to(dv)
        for i in range(0, used.size, self.RESLOT_ROWS):
            sl = used[i:i + self.RESLOT_ROWS]
            w = _take(tree, sl)
            x = _i64(w) & 0xFFFFFFFF
            par = x & 0x3FFFFFF
            slot = x >> 26
            need = (x != 0xFFFFFFFF) & (slot != 63)
            if _is_np(x):
                need &= xp_ch[np.where(need, par, 0)]
                if not need.any():
                    continue
                r, v = np.nonzero(need)
                p = par[r, v]
                e = np.searchsorted(xp_keys, p * V + v)
                assert np.all(xp_keys[e] == p * V + v), "kept tree edge missing"
                x[r, v] = p | ((xp_e[e] - xp_rp[p]) << 26)
                tree[sl] = (x & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
            else:
                need &= xp_ch[par.masked_fill(~need, 0)]
                if not bool(need.any()):
                    continue
                r, v = t.nonzero(need, as_tuple=True)
                p = par[r, v]
                k = p * V + v
                e = t.searchsorted(xp_keys, k).clamp_(max=xp_keys.shape[0] - 1)
                if not bool((xp_keys[e] == k).all()):     # the kept tree edge must exist
                    raise AssertionError("kept tree edge missing")
                x[r, v] = p | ((xp_e[e] - xp_rp[p]) << 26)
                x = t.where(x >= (1 << 31), x - (1 << 32), x).to(t.int32)
                tree.index_copy_(0, t.as_tensor(sl, device=dv), x)

    # -- filling ---------------------------------------------------------
    def _rows(self, store, compute, wanted, batch):
        """Ensure the rows of ``wanted`` (and as many of ``batch`` as the
        budget allows) exist; return the pool tables."""
        wanted = list(dict.fromkeys(int(v) for v in wanted))
        missing = [v for v in wanted if v not in store]
        miss = set(missing)
        extra = [int(v) for v in batch if int(v) not in store and int(v) not in miss] \
            if batch else []
        for v in wanted:                       # recently used
            if v in store.lru:
                store.lru.move_to_end(v)
        if missing or extra:
            cap = store.cap()
            room = cap - len(store) - len(missing)
            extra = extra[:max(0, room)]
            todo = missing + extra
            store.make_room(len(todo), set(wanted))
            for i in range(0, len(todo), COMPUTE_ROWS):
                part = todo[i:i + COMPUTE_ROWS]
                compute(store, part)
            self.rows_computed += len(todo)
        return store.tables()

    def _dfs_compute(self, engine, store, part):
        """Default-route rows of sources ``part`` into the pool.  Compact
        layouts: the tree words and depths come straight from the DFS
        kernels the bench times (sdnr_dfs_tables_tree), written into the
        pool's own rows when the free slots are contiguous."""
        srcs = np.asarray(part, np.int32)
        if self.layout == INT32:
            store.add(part, engine.dfs_tables(self.export, srcs))
            return
        like = engine.empty_rows(0, self.V, ("int32", _hops_dtype(self.V)))
        store.add(part, fill=lambda out: engine.dfs_tree_tables(self.export, srcs, self.layout,
                                                                out),
                  like=like)

    def _sp_compute(self, engine, store, part):
        dist, nh, _ = engine.shortest_tables(self.export, np.asarray(part, np.int32))
        dt = _nh_dtype(self.V)
        if _is_np(dist):
            store.add(part, (dist.view(np.int16), nh.astype(dt)))
        else:
            store.add(part, (dist, nh.to(getattr(_torch(), dt))))

    def dfs_rows(self, engine, wanted, batch=()):
        return self._rows(self.dfs, lambda st, p: self._dfs_compute(engine, st, p), wanted, batch)

    def sp_rows(self, engine, wanted, batch=()):
        return self._rows(self.sp, lambda st, p: self._sp_compute(engine, st, p), wanted, batch)


def tree_path(parent_row, s, d):
    """Dense vertex sequence s..d along a per-source tree row ([] if d is
    unreachable)."""
    if parent_row[d] < 0:
        return []
    seq = [int(d)]
    x = int(d)
    limit = parent_row.shape[0]
    while x != s:
        x = int(parent_row[x])
        seq.append(x)
        if len(seq) > limit:
            raise RuntimeError("route table corrupt: cycle at vertex %d" % x)
    seq.reverse()
    return seq


def count_shortest_paths(row_ptr, col, dist_row, s, d, limit=None):
    """Number of shortest s->d routes: a DP over the part of the
    shortest-path DAG reachable from s, deepest level first (the host twin of
    ecmp.hip's per-row count).  Stops counting once ``limit`` is passed and
    returns limit + 1."""
    dist_row = np.asarray(dist_row)
    want = int(dist_row[s])
    levels = [[int(s)]]
    seen = {int(s)}
    for _ in range(want):             # BFS down the DAG, one level at a time
        nxt = []
        for x in levels[-1]:
            dn = int(dist_row[x]) - 1
            for e in range(int(row_ptr[x]), int(row_ptr[x + 1])):
                n = int(col[e])
                if int(dist_row[n]) == dn and n not in seen:
                    seen.add(n)
                    nxt.append(n)
        levels.append(nxt)
    cnt = {int(d): 1}
    cap = None if limit is None else int(limit) + 1
    for lv in reversed(levels[:-1]):
        for x in lv:
            dn, c = int(dist_row[x]) - 1, 0
            for e in range(int(row_ptr[x]), int(row_ptr[x + 1])):
                n = int(col[e])
                if int(dist_row[n]) == dn:
                    c += cnt.get(n, 0)
            cnt[x] = c if cap is None else min(c, cap)
    return cnt.get(int(s), 0)


def shortest_paths_lex(row_ptr, col, dist_row, s, d):
    """Every shortest s->d vertex sequence in lexicographic dpid order (the
    order _find_routes_bfs returns them, topology_db.py:95-122): walk the
    shortest-path DAG (dist_row = hops to d) taking successors ascending.
    Sets above ECMP_LIMIT routes raise MemoryError before any is built, as
    the batched device path (RouteEngine.ecmp) does."""
    INF = _native.DIST_INF
    dist_row = np.asarray(dist_row)
    if dist_row.dtype == np.int16:
        dist_row = dist_row.view(np.uint16)
    dist_row = np.where(dist_row < 0, INF, dist_row)
    if int(dist_row[s]) == INF:
        return []
    if count_shortest_paths(row_ptr, col, dist_row, s, d, ECMP_LIMIT) > ECMP_LIMIT:
        raise MemoryError("ECMP set too large to enumerate")
    s, d = int(s), int(d)
    if s == d:
        return [[s]]

    def hops(x):
        want = int(dist_row[x]) - 1
        return (int(col[e]) for e in range(int(row_ptr[x]), int(row_ptr[x + 1]))
                if int(dist_row[int(col[e])]) == want)

    out = []
    # (iterative: a shortest route may be tens of thousands of links long)
    acc, stack = [s], [hops(s)]
    while stack:
        n = next(stack[-1], None)
        if n is None:
            stack.pop()
            acc.pop()
            continue
        acc.append(n)
        if n == d:
            out.append(list(acc))
            acc.pop()
            continue
        stack.append(hops(n))
    return out


def _least_cost_next_hops(row_ptr, col, cost, pc, x):
    """Out-neighbours n of x, ascending, with pc[n] finite and cost(x -> n) +
    pc[n] == pc[x] (pc: Python ints, COST_INF where there is no route)."""
    want = pc[x]
    return [int(col[e]) for e in range(int(row_ptr[x]), int(row_ptr[x + 1]))
            if pc[int(col[e])] != COST_INF and pc[int(col[e])] + int(cost[e]) == want]


def count_least_cost_paths(row_ptr, col, cost, pcost_row, s, d, limit=None):
    """Number of least-cost s->d routes under the link costs: a DP over the
    part of the least-cost DAG reachable from s, in ascending pcost order (the
    weighted twin of count_shortest_paths).  Stops counting once ``limit`` is
    passed and returns limit + 1."""
    pc = _pcost_u32(pcost_row).astype(np.int64).tolist()
    s, d = int(s), int(d)
    if pc[s] == COST_INF:
        return 0
    nxt = {}
    todo = [s]
    while todo:                       # the DAG below s
        x = todo.pop()
        if x in nxt:
            continue
        nxt[x] = [] if x == d else _least_cost_next_hops(row_ptr, col, cost, pc, x)
        todo.extend(n for n in nxt[x] if n not in nxt)
    cap = None if limit is None else int(limit) + 1
    cnt = {}
    for x in sorted(nxt, key=lambda v: pc[v]):            # a next hop costs strictly less
        c = 1 if x == d else sum(cnt[n] for n in nxt[x])
        cnt[x] = c if cap is None else min(c, cap)
    return cnt.get(s, 0)


def least_cost_paths_lex(row_ptr, col, cost, pcost_row, s, d):
    """Every least-cost s->d vertex sequence under the link costs ``cost``
    (uint32 [E]) in lexicographic vertex order -- the weighted counterpart of
    shortest_paths_lex: walk the least-cost DAG (pcost_row = least path costs
    to d) taking successors ascending.  [] without a route; sets above
    ECMP_LIMIT routes raise MemoryError before any is built."""
    pc = _pcost_u32(pcost_row).astype(np.int64).tolist()
    s, d = int(s), int(d)
    if pc[s] == COST_INF:
        return []
    if count_least_cost_paths(row_ptr, col, cost, pcost_row, s, d, ECMP_LIMIT) > ECMP_LIMIT:
        raise MemoryError("ECMP set too large to enumerate")
    if s == d:
        return [[s]]
    out = []
    # (iterative: a least-cost route may be thousands of links long)
    acc, stack = [s], [iter(_least_cost_next_hops(row_ptr, col, cost, pc, s))]
    while stack:
        n = next(stack[-1], None)
        if n is None:
            stack.pop()
            acc.pop()
            continue
        acc.append(n)
        if n == d:
            out.append(list(acc))
            acc.pop()
            continue
        stack.append(iter(_least_cost_next_hops(row_ptr, col, cost, pc, n)))
    return out


def expand_tree_paths(parent, port, rows, dsts, max_len=None):
    """Vectorised tree walks for many (row, dst) pairs.

    Returns ``(off, verts, ports)``: pair i's vertex sequence is
    ``verts[off[i]:off[i+1]]`` (source first) and ``ports[j]`` is the port on
    ``verts[j]`` toward ``verts[j+1]`` (undefined for the last vertex).
    Unreachable pairs get an empty range.
    """
    rows = np.asarray(rows, np.int64)
    dsts = np.asarray(dsts, np.int64)
    n = rows.shape[0]
    reach = parent[rows, dsts] >= 0
    # walk upward from the destinations collecting (vertex, in-port)
    chain_v, chain_p = [dsts.copy()], [np.full(n, -1, np.int64)]
    cur = dsts.copy()
    active = reach.copy()
    limit = parent.shape[1] if max_len is None else max_len
    for _ in range(limit):
        par = parent[rows, cur]
        done = par == cur                          # reached the root
        active &= ~done
        if not active.any():
            break
        prt = port[rows, cur]
        cur = np.where(active, par, cur)
        chain_v.append(np.where(active, cur, -1))
        chain_p.append(np.where(active, prt, -1))
    V = np.stack(chain_v, 1)      # [n, L] dst first
    P = np.stack(chain_p, 1)      # in-port of chain_v[k-1] from chain_v[k]
    lens = np.where(reach, (V >= 0).sum(1), 0)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    verts = np.empty(off[-1], np.int64)
    ports = np.full(off[-1], -1, np.int64)
    for i in np.nonzero(reach)[0]:
        L = lens[i]
        verts[off[i]:off[i + 1]] = V[i, :L][::-1]
        # chain slot k holds V[k] and P[k] = port on V[k] toward V[k-1];
        # source-first position j is V[L-1-j], its out-port P[L-1-j]
        ports[off[i]:off[i + 1] - 1] = P[i, 1:L][::-1]
    return off, verts, ports
