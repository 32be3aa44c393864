"""The C ABI with the vertex count on an id-width bound (boundary_graphs.py):
16-bit ids, sentinels and packed words up to V = 65,535, 17-bit rows up to
131,071, 32-bit rows above.  Every case uploads one fabric of at least 65,533
vertices, runs a handful of rows (sources / destinations = probe_ids(V)) and
compares bit for bit with the CPU reference the suite uses for that entry
point; the float planes of the ECMP load kernels follow the rule of
test_ecmp_link_loads.py (close: rtol 1e-9, atol 0).  The kernel names are
the dispatchers' (csrc/dfs.hip launch_split_ns, csrc/shortest.hip
sdnr_launch_shortest, csrc/ecmp.hip, csrc/routes.hip), read from the code.

What the code says about the bounds at "V < 65534": bfs_dest_kernel,
bfs_dest_lanes_kernel and ecmp_count_rows_kernel also need their row state in
LDS (bfs_dest_words <= 64 KB, bfs_lanes_bytes and ecmp_wave_lds = 12 V bytes
<= 159 KB), which ends far below -- at 65,533 none of them can run, forced or
not, so both sides of that bound run the same kernel here and the cases pin
that.

test_boundary_graphs.py holds the conditions that keep these cases from
passing vacuously."""
import time

import numpy as np
import pytest
import torch

import boundary_graphs as B
from oracle import oracle as O
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd.incremental import dfs_rows_affected, edge_diff
from sdnmpi_amd.topologies import CSR
from test_dfs_fold_live_gpu import gpu_rows
from test_ecmp_link_loads import SPLITS, close
from test_failure_loads_gpu import same as same_failure
from test_incremental import _device_verdict
from test_link_loads_gpu import on
from test_small_kernels_gpu import pack
from test_whatif_loads_gpu import same as same_whatif

pytestmark = pytest.mark.gpu

INVAL = -22
NONE = 0xFFFFFFFF
U64_MAX = (1 << 64) - 1
PLANE = "msbfs_plane_level_kernel+msbfs_plane_tables_kernel"
MSBFS = "msbfs_level_kernel+nexthop_kernel"
RING_SIZES = B.SIZES16 + B.SIZES17
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def drop_references():
    yield
    _dfs.clear()
    _dest.clear()
    _exact.clear()
    B.clear()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def fabric(name, V):
    return {"ring": B.ring, "jelly": B.jelly, "chain": B.chain}[name](V)


_dfs, _dest, _exact = {}, {}, {}


def dfs_ref(name, V):
    """(csr, probe ids, oracle parent / port / hops rows of them), once."""
    if (name, V) not in _dfs:
        csr = fabric(name, V)
        ids = np.array(B.probe_ids(V), np.int32)
        _dfs[(name, V)] = (csr, ids) + O.dfs_tables(csr, ids)
    return _dfs[(name, V)]


def dest_ref(V):
    """(csr, probe ids, oracle dist / nh / nh_port rows toward them), once."""
    if V not in _dest:
        csr = B.ring(V)
        ids = np.array(B.probe_ids(V), np.int32)
        _dest[V] = (csr, ids) + O.dest_tables(csr, ids)
    return _dest[V]


def words(parent, port, csr, layout):
    return np.asarray(EN.pack_host_tree(parent, port, csr, layout)).view(np.uint32)


def depth16(hops):
    return np.where(hops < 0, 0xFFFF, hops).astype(np.uint16)


def refused(call, *needles):
    with pytest.raises(_native.SdnrError) as ei:
        call()
    assert ei.value.code == INVAL
    for n in needles:
        assert n in str(ei.value)


# ----------------------------------------------------------- default route --

def split_kernel(csr, mode, tree):
    """launch_split_ns' name: dictionary rows where upload_dict builds them (V
    <= 65535, rows of <= 8 slots, not switched off), else u16 ids up to 65,535,
    u16 ids + the mask of bit 16 up to 131,071, int32 ids above."""
    V, W = csr.V, csr.max_degree()
    if V <= 65535 and W <= 8 and mode != "dict0":
        fmt = "dict"
    else:
        fmt = "row16" if V <= 65535 else "row17" if V <= 131071 else "row32"
    if tree == "packed":
        assert V <= 65535
    return "dfs_split_kernel<%s%s>" % (fmt, {"int32": "", "packed": ",packed",
                                            "slots": ",slots"}[tree])


DFS_CASES = [("ring", V) for V in RING_SIZES] + [("jelly", 65535), ("jelly", 65536)]


@pytest.mark.parametrize("mode", ["auto", "dict0", "global"])
@pytest.mark.parametrize("name,V", DFS_CASES)
def test_default_route_every_layout(ctx, monkeypatch, name, V, mode):
    """sdnr_dfs_tables (with hops), _packed, _slots and _tree in both layouts
    and depth widths from the probe sources.  At these sizes neither the LDS
    strategies (lds / coop / count / async: their per-source state is 10 V
    bytes and more) nor anything but the split kernel applies; `global` is the
    one SDNROUTE_DFS_STRATEGY value that is accepted, and changes nothing."""
    if mode == "dict0":
        monkeypatch.setenv("SDNROUTE_DFS_DICT", "0")
    if mode == "global":
        monkeypatch.setenv("SDNROUTE_DFS_STRATEGY", "global")
    csr, ids, po, to, ho = dfs_ref(name, V)
    ctx.upload(csr)
    p, t, h = ctx.dfs_tables(ids)
    assert ctx.last_kernel() == split_kernel(csr, mode, "int32")
    for got, want in ((p, po), (t, to), (h, ho)):
        assert got.dtype == np.int32 and np.array_equal(got, want)
    slot = words(po, to, csr, EN.SLOT)
    assert np.array_equal(ctx.dfs_tables_slots(ids), slot)
    assert ctx.last_kernel() == split_kernel(csr, mode, "slots")
    tree, depth = ctx.dfs_tables_tree(ids, _native.TREE_SLOT, 4)
    assert np.array_equal(tree, slot) and np.array_equal(depth, ho)
    # int32 rows carry no 17th bit: slot words with depths go through int32 tables
    assert ctx.last_kernel() == split_kernel(csr, mode, "slots" if V <= 131071 else "int32")
    if V > 65535:
        refused(lambda: ctx.dfs_tables_packed(ids), "65535")
        refused(lambda: ctx.dfs_tables_tree(ids, _native.TREE_PORT16, 4), "65535")
        refused(lambda: ctx.dfs_tables_tree(ids, _native.TREE_SLOT, 2), "u16 depths")
        return
    packed = words(po, to, csr, EN.PORT16)
    if V == 65535:                               # root 65,534: one below SDNR_TREE_NONE
        r = ids.tolist().index(65534)
        assert packed[r, 65534] == 0xFFFFFFFE
        assert name != "ring" or packed[r, B.isolated(V)] == NONE
    assert np.array_equal(ctx.dfs_tables_packed(ids), packed)
    assert ctx.last_kernel() == split_kernel(csr, mode, "packed")
    tree, depth = ctx.dfs_tables_tree(ids, _native.TREE_SLOT, 2)
    assert np.array_equal(tree, slot) and np.array_equal(depth, depth16(ho))
    assert ctx.last_kernel() == split_kernel(csr, mode, "slots")
    for nbytes in (2, 4):
        tree, depth = ctx.dfs_tables_tree(ids, _native.TREE_PORT16, nbytes)
        assert np.array_equal(tree, packed)
        assert np.array_equal(depth, depth16(ho) if nbytes == 2 else ho)
        assert ctx.last_kernel() == split_kernel(csr, mode, "packed")


@pytest.mark.parametrize("V", [65535, 65536, 131071, 131072])
def test_default_route_sources_that_are_no_vertex(ctx, V):
    """Device path: -1, V and V + 5 give empty rows beside real ones."""
    csr, ids, po, to, ho = dfs_ref("ring", V)
    ctx.upload(csr)
    srcs = np.array([-1, V - 1, V, 0, V + 5], np.int32)
    want = [np.full((5, V), -1, np.int32) for _ in range(3)]
    for r, s in ((1, V - 1), (3, 0)):
        k = ids.tolist().index(s)
        for w, x in zip(want, (po, to, ho)):
            w[r] = x[k]
    layouts = ["hops", "slots", "slot32"] + (["packed", "tree16"] if V <= 65535 else [])
    for layout in layouts:
        p, t, h = gpu_rows(ctx, csr, srcs, layout)
        assert np.array_equal(p, want[0]) and np.array_equal(t, want[1]), layout
        if h is not None:
            assert np.array_equal(h, want[2]), layout


def test_twin_fold_at_the_top_ids(ctx, monkeypatch):
    """V - 1 and V - 2 of ring(65535) as twins, the fold forced on: the derived
    row of the one equals the searched row of the other up to the patched
    entries, i.e. both equal the oracle's.  Twice: the second call is the one
    that would take a published live count."""
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")
    V = 65535
    csr = B.with_twins(B.ring(V), V - 1, V - 2)
    ctx.upload(csr)
    rep = ctx.twin_reps()
    assert rep[V - 1] == V - 2 and rep[V - 2] == V - 2 and (rep[:V - 2] == np.arange(V - 2)).all()
    srcs = np.array([V - 1, 0, V - 2, 32768, V - 1], np.int32)
    po, to, ho = O.dfs_tables(csr, srcs)
    assert not np.array_equal(po[0], po[2])
    for layout, tree in (("packed", "packed"), ("tree16", "packed"), ("hops", "int32")):
        for _ in range(2):
            p, t, h = gpu_rows(ctx, csr, srcs, layout)
            assert ctx.last_launches() == 3 and ctx.last_dfs_searched() == 3
            assert ctx.last_kernel() == split_kernel(csr, "auto", tree)
            assert np.array_equal(p, po) and np.array_equal(t, to), layout
            if h is not None:
                assert np.array_equal(h, ho), layout


# ------------------------------------------ shortest tables and ECMP sets --

def exact_counts(csr, dist_row):
    """Shortest-route counts toward one destination as Python ints (not
    saturated): the level DP of oracle.ecmp_counts, a level's links at a time."""
    V = csr.V
    lv = dist_row.astype(np.int64)
    lv[lv == 0xFFFF] = -1
    esrc = np.repeat(np.arange(V, dtype=np.int64), np.diff(csr.row_ptr))
    edst = csr.col.astype(np.int64)
    dag = np.nonzero((lv[esrc] > 0) & (lv[edst] == lv[esrc] - 1))[0]
    dag = dag[np.argsort(lv[esrc[dag]], kind="stable")]
    top = int(lv.max())
    ends = np.searchsorted(lv[esrc[dag]], np.arange(top + 2))
    cnt = np.zeros(V, object)
    cnt[lv == 0] = 1
    for L in range(1, top + 1):
        e = dag[ends[L]:ends[L + 1]]
        np.add.at(cnt, esrc[e], cnt[edst[e]])
    return cnt


def unrank(csr, dist_row, cnt, s, r):
    """The r-th shortest route from s in lexicographic order, or None."""
    if dist_row[s] == 0xFFFF or r >= cnt[s]:
        return None
    seq, x = [s], s
    while dist_row[x] > 0:
        for n in csr.col[csr.row_ptr[x]:csr.row_ptr[x + 1]].tolist():
            if int(dist_row[n]) + 1 != int(dist_row[x]):
                continue
            if r < cnt[n]:
                x = n
                break
            r -= cnt[n]
        seq.append(x)
    return seq


SP_SIZES = B.SIZES16 + (131071, 131072)
SP_CASES = [(V, s) for V in SP_SIZES for s in ("auto", "plane", "msbfs")] + \
    [(V, s) for V in (65533, 65534) for s in ("dest", "lanes")]


@pytest.mark.parametrize("V,strategy", SP_CASES)
def test_shortest_tables(ctx, monkeypatch, V, strategy):
    """Toward every probe id, the isolated vertex among them.  `dest` and
    `lanes` are asked for on both sides of their V < 65534: their LDS bound
    refuses them on either, and the plane BFS runs."""
    if strategy != "auto":
        monkeypatch.setenv("SDNROUTE_SP_STRATEGY", strategy)
    csr, ids, dist, nh, nhp = dest_ref(V)
    ctx.upload(csr)
    got = ctx.shortest_tables(ids)
    assert ctx.last_kernel() == (MSBFS if strategy == "msbfs" else PLANE)
    for g, w, what in zip(got, (dist, nh, nhp), ("dist", "nh", "nh_port")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    r = ids.tolist().index(B.isolated(V))
    assert (np.delete(got[0][r], B.isolated(V)) == 0xFFFF).all()


def ecmp_rows(V):
    """Four of the destination rows: toward 0, V - 1, the isolated vertex, and
    65,535 (65,534 where that is no vertex), with their exact counts."""
    if V not in _exact:
        csr, ids, dist, _, _ = dest_ref(V)
        pick = [ids.tolist().index(x) for x in (0, V - 1, B.isolated(V), min(65535, V - 2))]
        d = np.ascontiguousarray(dist[pick])
        _exact[V] = (csr, ids[pick], d, [exact_counts(csr, row) for row in d])
    return _exact[V]


@pytest.mark.parametrize("counter", ["default", "global"])
@pytest.mark.parametrize("V", SP_SIZES)
def test_ecmp_counts_and_routes(ctx, monkeypatch, V, counter):
    """sdnr_ecmp_counts on the rows above in both counter forms (the rows
    kernel needs 12 V bytes of LDS: the global-memory one runs either way),
    then sdnr_ecmp_routes for ranks 0, count - 1 and count."""
    if counter == "global":
        monkeypatch.setenv("SDNROUTE_ECMP", "global")
    csr, dsts, dist, counts = ecmp_rows(V)
    ctx.upload(csr)
    paths = ctx.ecmp_counts(dist)
    assert ctx.last_kernel() == "ecmp_count_global_kernel"
    want = np.array([[min(c, U64_MAX) for c in row] for row in counts], np.uint64)
    assert paths.dtype == np.uint64 and np.array_equal(paths, want)
    assert np.array_equal(want[0], O.ecmp_counts(csr, dist[0]))
    assert (want == U64_MAX).any() and (want[2] == 0).sum() == V - 1
    srcs_of = [V - 1, min(65535, V - 2), 0, 32768, B.ONE_WAY, B.isolated(V)]
    rows, srcs, ranks, expect = [], [], [], []
    enumerated = 0
    for r in range(len(dsts)):
        # ... and the highest ids with a set that can be listed, and with a large unsaturated one
        size = counts[r].astype(np.float64)
        more = [int(np.nonzero(m)[0][-1]) for m in ((size >= 2) & (size <= 2000),
                                                    (size > 2000) & (size < 1e19)) if m.any()]
        for s in srcs_of + more:
            c = counts[r][s]
            enumerated += 2 <= c <= 2000
            cs = min(c, U64_MAX)                 # what the device holds
            # below a saturated count the exact sums decide every rank <= 2^64 - 2 as the
            # saturated ones do (test_small_kernels_gpu.Unranker); rank == count is no route
            for rank in sorted({0, max(cs - 1, 0), cs}):
                rows.append(r)
                srcs.append(s)
                ranks.append(rank)
                expect.append(None if rank >= cs else unrank(csr, dist[r], counts[r], s, rank))
            if 2 <= c <= 2000:                   # enumerable: the list itself
                routes = EN.shortest_paths_lex(csr.row_ptr, csr.col, dist[r], s, int(dsts[r]))
                assert len(routes) == c and routes[c - 1] == unrank(csr, dist[r], counts[r], s,
                                                                   c - 1)
    L = int(dist[dist != 0xFFFF].max()) + 1
    got = ctx.ecmp_routes(dist, paths, np.array(rows, np.int32), np.array(srcs, np.int32),
                          np.array(ranks, np.uint64), L)
    assert ctx.last_kernel() == "ecmp_unrank_kernel"
    some = 0
    for k, seq in enumerate(expect):
        row = got[k].tolist()
        if seq is None:
            assert row == [-1] * L, (rows[k], srcs[k], ranks[k])
        else:
            assert row == seq + [-1] * (L - len(seq)), (rows[k], srcs[k], ranks[k])
            some += len(seq) > 2
    assert some >= 8 and enumerated >= 3


# ------------------------------------------------------------ flow entries --

def route_pairs(csr, ids, po):
    """(rows, dsts): to V - 1, to 65,534, to the isolated vertex, and to a
    tree child of a probe id (a route that passes through it)."""
    V = csr.V
    rows, dsts, through = [], [], 0
    for r, s in enumerate(ids.tolist()):
        for d in (V - 1, 65534, B.isolated(V)):
            rows.append(r)
            dsts.append(d)
        for p in ids.tolist():
            kids = np.nonzero((po[r] == p) & (np.arange(V) != p))[0]
            if p != s and kids.size:
                rows.append(r)
                dsts.append(int(kids[-1]))
                through += 1
                break
    assert through >= len(ids) - 2
    return np.array(rows, np.int32), np.array(dsts, np.int32)


def host_entries(po, to, ids, rows, dsts, last):
    off, sw, hp = [0], [], []
    for r, d, lp in zip(rows.tolist(), dsts.tolist(), last.tolist()):
        seq = O.tree_path(po[r], int(ids[r]), d)
        if seq:
            sw += seq
            hp += [int(to[r, b]) for b in seq[1:]] + [lp]
        off.append(len(sw))
    return np.array(off, np.int64), np.array(sw, np.int32), np.array(hp, np.int32)


@pytest.mark.parametrize("V", [65535, 65536, 131072])
def test_flow_entries(ctx, V):
    csr, ids, po, to, ho = dfs_ref("ring", V)
    ctx.upload(csr)
    rows, dsts = route_pairs(csr, ids, po)
    n = len(rows)
    last = np.full(n, 0xFFFE, np.int32)
    off, sw, hp = host_entries(po, to, ids, rows, dsts, last)
    iso = dsts == B.isolated(V)
    assert (np.diff(off)[iso & (ids[rows] != B.isolated(V))] == 0).all() and off[-1] > 10000
    assert sw.max() == V - 1 and 0xFFFE in hp and (hp >= 0x8000).any()
    g_off, g_sw, g_hp = ctx.expand_routes(po, to, ho, rows, dsts, last)
    assert ctx.last_kernel() == ("route_seg_packed_kernel<1024>" if V <= 65535
                                 else "route_jump_kernel<16>")
    assert np.array_equal(g_off, off) and np.array_equal(g_sw, sw) and np.array_equal(g_hp, hp)
    tp, tt, th = dev(po), dev(to), dev(ho)
    d_r, d_d, d_l = dev(rows), dev(dsts), dev(last)
    d_off = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    ent = torch.zeros(int(off[-1]), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize(DEV)
    ctx.route_offsets_device(th.data_ptr(), d_r.data_ptr(), d_d.data_ptr(), n, d_off.data_ptr(),
                             nrows=len(ids))
    ctx.synchronize()
    assert np.array_equal(d_off.cpu().numpy(), off)

    def packed(last_ptr):
        ctx.expand_routes_packed_device(tp.data_ptr(), tt.data_ptr(), len(ids), d_r.data_ptr(),
                                        d_d.data_ptr(), last_ptr, n, d_off.data_ptr(),
                                        ent.data_ptr())
    if V > 65535:
        refused(lambda: packed(d_l.data_ptr()), "65535")
        return
    packed(d_l.data_ptr())
    ctx.synchronize()
    assert ctx.last_kernel() == "route_seg_packed_kernel<1024,u32>"
    e = ent.cpu().numpy().view(np.uint32)
    assert np.array_equal(e & 0xFFFF, sw) and np.array_equal(e >> 16, hp)
    wide = last.copy()
    wide[1] = 0xFFFF
    d_w = dev(wide)
    torch.cuda.synchronize(DEV)
    packed(d_w.data_ptr())
    with pytest.raises(_native.SdnrError) as ei:
        ctx.synchronize()
    assert ei.value.code == INVAL and "last port" in str(ei.value)


# --------------------------------------------------------------- row tools --

@pytest.mark.parametrize("V", [65535, 65537])
def test_tree_pack(ctx, V):
    csr, ids, po, to, _ = dfs_ref("ring", V)
    ctx.upload(csr)
    parent, port = dev(po.reshape(-1)), dev(to.reshape(-1))
    n = po.size
    got = pack(ctx, parent, None, n, _native.TREE_SLOT)
    assert np.array_equal(got, words(po, to, csr, EN.SLOT).reshape(-1))
    if V > 65535:
        out = torch.empty(n, dtype=torch.int32, device=DEV)
        refused(lambda: ctx.tree_pack_device(parent.data_ptr(), port.data_ptr(), n,
                                             out.data_ptr(), _native.TREE_PORT16), "65535")
        return
    got = pack(ctx, parent, port, n, _native.TREE_PORT16)
    assert np.array_equal(got, words(po, to, csr, EN.PORT16).reshape(-1))
    assert 0xFFFFFFFE in got and ((got >> 16) == 0xFFFE).any()


def relinked(csr, removed, added):
    """The CSR without the links `removed` and with the links `added` [(u, v)]
    on port 77."""
    V = csr.V
    src = np.repeat(np.arange(V, dtype=np.int64), np.diff(csr.row_ptr))
    key = src * V + csr.col
    keep = ~np.isin(key, [u * V + v for u, v in removed])
    assert (~keep).sum() == len(removed) and not np.isin([u * V + v for u, v in added], key).any()
    s = np.concatenate([src[keep], [u for u, _ in added]]).astype(np.int64)
    d = np.concatenate([csr.col[keep], [v for _, v in added]]).astype(np.int64)
    p = np.concatenate([csr.port[keep], [77] * len(added)]).astype(np.int64)
    order = np.argsort(s * V + d, kind="stable")
    rp = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(s, minlength=V), out=rp[1:])
    return CSR(csr.dpids, rp, d[order], p[order])


@pytest.mark.parametrize("V", [65535, 65537])
def test_rows_affected(ctx, V):
    """Removed and added links between probe ids against the host row test, in
    every layout and depth width the size admits (port16 and slot words with
    u16 depths up to 65,535, int32 depths above; int32 parents with int32
    depths)."""
    csr, ids, po, to, ho = dfs_ref("ring", V)
    changes = [([(V - 1, V - 2)], []), ([(V - 2, V - 1), (0, 1)], [(V - 1, 32768)]),
               ([], [(32767, 65534), (65534, 100)]), ([(32768, 32769)], [(B.ONE_WAY, 65533)])]
    flagged = 0
    for removed, added in changes:
        new = relinked(csr, removed, added)
        diff = edge_diff(csr, new)
        want = np.asarray(dfs_rows_affected(po, ho, ids, diff), bool)
        flagged += int(want.sum())
        for layout in (["port16"] if V <= 65535 else []) + ["slot", "int32"]:
            got = _device_verdict(ctx, csr, new, po, to, ho, ids, diff, layout)
            assert ctx.last_kernel() == "dfs_rows_affected_kernel"
            assert np.array_equal(got, want), (removed, added, layout)
    assert 0 < flagged < len(changes) * len(ids)


# ----------------------------------------- loads and weighted tables, global --

def demand(V, ids, nrows, seed):
    """About 50 pairs per row, the probe ids among the other ends."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(nrows), 50)
    ends = rng.integers(0, V, rows.size)
    ends[::4] = rng.choice(ids, ends[::4].size)
    w = rng.integers(0, 1 << 32, rows.size, dtype=np.uint64)
    w[rng.random(rows.size) < 0.2] = 0
    return rows, ends, w


LOAD_ROWS = (0, -1, -2, 3)            # of the probe ids: 0, V - 1, V - 2, 32768


@pytest.mark.parametrize("V", [65535, 65537])
def test_link_loads_every_layout_and_direction(eng, V):
    csr, ids, po, to, _ = dfs_ref("ring", V)
    pick = list(LOAD_ROWS)
    po, to, src = po[pick], to[pick], ids[pick]
    rows, dsts, w = demand(V, ids, len(pick), 60)
    ex = on(csr)
    want = EN.link_loads_host(csr, po, EN.INT32, rows, dsts, w)
    assert want.any()
    for lay in (EN.INT32, EN.SLOT) + ((EN.PORT16,) if V <= 65535 else ()):
        tree = po if lay == EN.INT32 else EN.pack_host_tree(po, to, csr, lay)
        got = eng.link_loads(ex, dev(np.asarray(tree).view(np.int32)), lay, rows, dsts, w)
        assert np.array_equal(got, want), lay
        assert eng.ctx.last_kernel() == "link_loads_kernel<global>"
    if V > 65535:
        tree = dev(EN.pack_host_tree(po, to, csr, EN.SLOT))
        refused(lambda: eng.link_loads(ex, tree, EN.PORT16, rows, dsts, w), "65535")
    nh = dest_ref(V)[3][pick]
    want = EN.link_loads_host(csr, nh, EN.INT32, rows, dsts, w, to_root=True)
    got = eng.link_loads(ex, dev(nh), EN.INT32, rows, dsts, w, to_root=True)
    assert want.any() and np.array_equal(got, want)


@pytest.mark.parametrize("V", [65535, 65537])
def test_ecmp_and_cost_ecmp_link_loads(eng, V):
    csr, ids, dist, _, _ = dest_ref(V)
    pick = list(LOAD_ROWS)
    dist, dsts = dist[pick], ids[pick]
    rows, srcs, w = demand(V, ids, len(pick), 61)
    ex = on(csr)
    cost = np.random.default_rng(62).integers(1, 5, csr.E).astype(np.uint32)
    pcost = EN.cost_tables_host(csr, cost, dsts)[0]
    d_dist = dev(dist.view(np.int16))
    d_pc = dev(pcost.view(np.int32))
    for split in SPLITS:
        want = EN.ecmp_link_loads_host(csr, dist, rows, srcs, w, split)
        got = eng.ecmp_link_loads(ex, d_dist, rows, srcs, w, split)
        assert want.any() and got.dtype == np.float64 and close(got, want), split
        assert eng.ctx.last_kernel() == "ecmp_loads_kernel<global>"
        want = EN.cost_ecmp_link_loads_host(csr, cost, pcost, rows, srcs, w, split)
        got = eng.cost_ecmp_link_loads(ex, cost, d_pc, rows, srcs, w, split)
        assert want.any() and got.dtype == np.float64 and close(got, want), split
        assert eng.ctx.last_kernel() == "cost_ecmp_loads_kernel<global>"


@pytest.mark.parametrize("V", [65535, 65537])
def test_cost_and_widest_tables(ctx, V):
    csr, ids, _, _, _ = dest_ref(V)
    dsts = ids[[0, -1, -2]]
    rng = np.random.default_rng(63)
    cost = rng.integers(1, 5, csr.E).astype(np.uint32)
    util = rng.integers(0, 1000, csr.E).astype(np.uint32)
    ctx.upload(csr)
    ctx.set_link_costs(cost)
    want = EN.cost_tables_host(csr, cost, dsts)
    got = ctx.cost_tables(dsts)
    assert ctx.last_kernel() == "cost_tables_kernel<global,4>"
    for g, w, what in zip(got, want, ("pcost", "nh", "nh_port")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    assert (want[1] == V - 1).any() and (want[2] >= 0x8000).any()
    wide = EN.widest_tables_host(csr, cost, want[0], util, dsts)
    got = ctx.widest_tables(want[0], util, dsts)
    assert ctx.last_kernel() == "widest_tables_kernel<global,4>"
    for g, w, what in zip(got, wide, ("bott", "nh", "nh_port")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    ctx.set_link_costs(None)
    ctx.synchronize()


@pytest.mark.parametrize("V", [65535, 65537])
def test_failure_and_whatif_link_loads(eng, V):
    """Two scenarios that fail / re-cost the links at V - 1."""
    csr, ids, _, _, _ = dest_ref(V)
    dsts = ids[[0, -1, 3]]
    rows, srcs, w = demand(V, ids, len(dsts), 64)
    srcs[:6] = V - 1
    cost = np.random.default_rng(65).integers(1, 5, csr.E).astype(np.uint32)
    ex = on(csr)
    a, b = int(csr.row_ptr[V - 1]), int(csr.row_ptr[V])
    into = np.nonzero(csr.col == V - 1)[0]
    fail = [sorted([a, a + 1, int(into[0])]), list(range(a, b))]
    recost = [([a, a + 1], [9, EN.COST_INF]), ([int(into[0]), int(into[-1])], [1, 1])]
    for split in SPLITS:
        want = EN.failure_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, fail, split)
        got = eng.failure_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, fail, split)
        same_failure(got, want)
        assert want[0].any() and eng.ctx.last_kernel() == "failure_ecmp_loads_kernel<global>"
        want = EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, recost, split)
        got = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, recost, split)
        same_whatif(got, want)
        assert want[0].any() and eng.ctx.last_kernel() == "whatif_ecmp_loads_kernel<global>"


@pytest.mark.parametrize("V", [65535, 65537])
def test_all_pairs_entry_points_refuse(ctx, V):
    ctx.upload(B.ring(V))
    buf = torch.zeros(64, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize(DEV)
    refused(lambda: ctx.apsp_device(buf.data_ptr()), "16384")
    refused(lambda: ctx.lfa_tables_device(buf.data_ptr(), buf.data_ptr(), 1, buf.data_ptr(),
                                          buf.data_ptr(), buf.data_ptr()), "16384")
    assert not buf.cpu().numpy().any()


# ---------------------------------------------------------- the deep chain --

def test_chain_default_route_rows(ctx, eng):
    """The path of 65,535 vertices from both ends in port16 words with u16
    depths: the far end reads 65,534 = 0xFFFE, reached.  On those rows the
    loads, one route of 65,535 entries, and the row test for an added link
    (V - 1, 0) and a removed (32768, 32769): a climb of 65,534 steps is no
    cycle."""
    V = 65535
    csr = B.chain(V)
    srcs = np.array([0, V - 1], np.int32)
    po, to, ho = O.dfs_tables(csr, srcs)
    ctx.upload(csr)
    tree, depth = ctx.dfs_tables_tree(srcs, _native.TREE_PORT16, 2)
    assert ctx.last_kernel() == "dfs_split_kernel<dict,packed>"
    assert np.array_equal(tree, words(po, to, csr, EN.PORT16))
    assert np.array_equal(depth, depth16(ho))
    assert depth[0, V - 1] == 0xFFFE and depth[1, 0] == 0xFFFE and (depth != 0xFFFF).all()
    assert tree[0, V - 1] == (V - 2) | (0xFFFE << 16) and tree[1, V - 1] == 0xFFFFFFFE
    # the loads: everything toward the far end, and a few short ones
    rows = np.array([0, 0, 1, 1, 1], np.int64)
    dsts = np.array([V - 1, 5, 0, V - 1, 32768], np.int64)
    w = np.array([3, 1 << 40, 5, 7, 11], np.uint64)
    want = EN.link_loads_host(csr, po, EN.INT32, rows, dsts, w)
    got = eng.link_loads(on(csr), dev(tree.view(np.int32)), EN.PORT16, rows, dsts, w)
    assert np.array_equal(got, want) and eng.ctx.last_kernel() == "link_loads_kernel<global>"
    # one route over the whole chain
    last = np.array([0xFFFE], np.int32)
    off, sw, hp = ctx.expand_routes(po, to, ho, np.array([1], np.int32), np.array([0], np.int32),
                                    last)
    assert off.tolist() == [0, V] and np.array_equal(sw, np.arange(V - 1, -1, -1))
    assert (hp[:-1] == 1).all() and hp[-1] == 0xFFFE
    for removed, added in (([], [(V - 1, 0)]), ([(32768, 32769)], [])):
        new = relinked(csr, removed, added)
        diff = edge_diff(csr, new)
        want = np.asarray(dfs_rows_affected(po, ho, srcs, diff), bool)
        for layout in ("port16", "slot", "int32"):
            got = _device_verdict(ctx, csr, new, po, to, ho, srcs, diff, layout)
            assert np.array_equal(got, want), (removed, added, layout)
    ctx.synchronize()                              # no "not a tree" left behind


def test_chain_shortest_distance_65534(ctx):
    """Destination 0 of the chain: distance 65,534 at the far end, one route
    from everywhere.  The BFS is deeper than the 255 levels of the plane
    kernels, so the level loop (one host synchronisation per level) runs."""
    V = 65535
    csr = B.chain(V)
    ctx.upload(csr)
    dsts = np.array([0], np.int32)
    t0 = time.perf_counter()
    dist, nh, nhp = ctx.shortest_tables(dsts)
    print("chain shortest_tables: %.2f s" % (time.perf_counter() - t0))
    assert ctx.last_kernel() == MSBFS
    want = O.dest_tables(csr, dsts)
    for g, w in zip((dist, nh, nhp), want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert np.array_equal(dist[0], np.arange(V, dtype=np.uint16)) and dist[0, V - 1] == 0xFFFE
    assert np.array_equal(nh[0, 1:], np.arange(V - 1)) and (nhp[0, 1:] == 1).all()
    paths = ctx.ecmp_counts(dist)
    assert ctx.last_kernel() == "ecmp_count_global_kernel"
    assert (paths == 1).all()
