"""loads.hip (sdnr_link_loads) on the GPU against engine.link_loads_host and
a plain per-pair walk, and the drop-in's link_loads against the reference's
fdb entries.  All values are integers: every comparison is exact."""
import types

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from test_link_loads import U64, counter_of, golden_pairs, random_csr, walk_loads

pytestmark = pytest.mark.gpu

LAYOUTS = (EN.INT32, EN.PORT16, EN.SLOT)


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def on(csr):
    """The export-shaped handle RouteEngine wants for a bare CSR."""
    return types.SimpleNamespace(csr=csr)


def dev_tree(eng, tree):
    import torch
    a = np.ascontiguousarray(tree)
    if a.dtype != np.int32:
        a = a.astype(np.uint32).view(np.int32) if a.dtype != np.uint32 else a.view(np.int32)
    return torch.from_numpy(a).to(eng.dev)


def rand_weights(rng, n):
    """u64 weights over the whole range, about 30 % zeros."""
    w = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, n, dtype=np.uint64)
    w[rng.random(n) < 0.3] = 0
    return w


def raw_loads(eng, csr, tree, layout, nrows, off, dsts, w, load, to_root=False, timing=False):
    """One sdnr_link_loads call on device copies of the arguments, adding
    into the device tensor ``load``; no synchronize."""
    import torch
    lay = {EN.PORT16: _native.TREE_PORT16, EN.SLOT: _native.TREE_SLOT,
           EN.INT32: _native.TREE_INT32}[layout]
    keep = [dev_tree(eng, tree) if tree is not None else None,
            torch.from_numpy(np.asarray(off, np.int64)).to(eng.dev),
            torch.from_numpy(np.asarray(dsts, np.int32)).to(eng.dev),
            torch.from_numpy(np.asarray(w, np.uint64).view(np.int64)).to(eng.dev)
            if w is not None else None]
    torch.cuda.synchronize()
    eng.ctx.link_loads_device(keep[0].data_ptr() if keep[0] is not None else 0, lay, nrows,
                              keep[1].data_ptr(), keep[2].data_ptr(),
                              keep[3].data_ptr() if keep[3] is not None else 0,
                              load.data_ptr(), to_root=to_root, timing=timing)
    return keep


def zeros_u64(eng, n):
    import torch
    return torch.zeros(max(1, n), dtype=torch.int64, device=eng.dev)


def as_u64(load, n):
    return load.cpu().numpy().view(np.uint64)[:n]


# ------------------------------------------------------ the small fabrics --

@pytest.fixture(scope="module")
def small_cases():
    """Per G.SMALL fabric: tables of every source / destination from the
    oracle, a demand over every row, and the expected loads (walk == host),
    computed once."""
    from oracle import oracle as O
    out = {}
    for k, name in enumerate(G.SMALL):
        csr = G.Golden(name).fabric().csr()
        ids = np.arange(csr.V, dtype=np.int32)
        par, prt, _ = O.dfs_tables(csr, ids)
        _, nh, _ = O.dest_tables(csr, ids)
        rng = np.random.default_rng(40 + k)
        n = 5 * csr.V
        rows = np.repeat(np.arange(csr.V), 5)
        dsts = rng.integers(0, csr.V, n)
        w = rand_weights(rng, n)
        want = {}
        for to_root, tab in ((False, par), (True, nh)):
            for wt in (w, None):
                ww = w if wt is not None else np.ones(n, np.uint64)
                a = walk_loads(csr, tab, rows, dsts, ww, to_root)
                b = EN.link_loads_host(csr, tab, EN.INT32, rows, dsts, wt, to_root)
                assert np.array_equal(a, b)
                want[(to_root, wt is not None)] = a
        out[name] = (csr, par, prt, nh, rows, dsts, w, want)
    return out


@pytest.mark.parametrize("name", G.SMALL)
def test_small_fabrics_every_source_row_all_layouts(eng, small_cases, name):
    csr, par, prt, _, rows, dsts, w, want = small_cases[name]
    ex = on(csr)
    for lay in LAYOUTS:
        tree = par if lay == EN.INT32 else EN.pack_host_tree(par, prt, csr, lay)
        d_tree = dev_tree(eng, tree)
        for wt in (w, None):
            got = eng.link_loads(ex, d_tree, lay, rows, dsts, wt)
            assert np.array_equal(got, want[(False, wt is not None)]), (name, lay)
            assert eng.ctx.last_kernel() == "link_loads_kernel<lds>"
            assert eng.ctx.last_launches() == 1


@pytest.mark.parametrize("name", G.SMALL)
def test_small_fabrics_reversed_direction(eng, small_cases, name):
    csr, _, _, nh, rows, dsts, w, want = small_cases[name]
    ex = on(csr)
    d_nh = dev_tree(eng, nh)
    for wt in (w, None):
        got = eng.link_loads(ex, d_nh, EN.INT32, rows, dsts, wt, to_root=True)
        assert np.array_equal(got, want[(True, wt is not None)]), name


# ------------------------------------------------------------ edge shapes --

def path_csr(V):
    v = np.arange(V - 1)
    return T.build_csr(np.concatenate([v, v + 1]) + 1, np.concatenate([v + 1, v]) + 1,
                       np.ones(2 * (V - 1), np.int64), extra_vertices=list(range(1, V + 1)))


def path_rooted_at_0(csr, layout):
    """The tree row of a path graph rooted at vertex 0 and the CSR index of
    every edge v - 1 -> v (v = 1 .. V - 1), built in numpy."""
    V = csr.V
    v = np.arange(V, dtype=np.int64)
    par = np.maximum(v - 1, 0)
    slot = np.where(v == 0, 63, np.where(v == 1, 0, 1))      # row u = [u - 1, u + 1]
    if layout == EN.INT32:
        tree = par.astype(np.int32)
    else:
        assert layout == EN.SLOT
        tree = (par | (slot << 26)).astype(np.uint32).view(np.int32)
    eidx = np.asarray(csr.row_ptr, np.int64)[par[1:]] + slot[1:]
    assert np.array_equal(np.asarray(csr.col)[eidx], v[1:])
    return tree.reshape(1, V), eidx


def check_path(eng, V, layout, kernel):
    csr = path_csr(V)
    ex = on(csr)
    tree, eidx = path_rooted_at_0(csr, layout)
    rng = np.random.default_rng(V)
    dsts = np.arange(V)
    w = rand_weights(rng, V)
    want = np.zeros(csr.E, np.uint64)
    want[eidx] = np.cumsum(w[::-1])[::-1][1:]                # sum of w[d] over d >= v, wrapping
    got = eng.link_loads(ex, dev_tree(eng, tree), layout, np.zeros(V, np.int64), dsts, w)
    assert np.array_equal(got, want), V
    assert eng.ctx.last_kernel() == kernel


@pytest.mark.parametrize("V", [2, 3, 64, 65, 257, 1025])
def test_path_graphs_rooted_at_an_end(eng, V):
    check_path(eng, V, EN.INT32, "link_loads_kernel<lds>")
    check_path(eng, V, EN.SLOT, "link_loads_kernel<lds>")


def test_both_sides_of_the_lds_threshold(eng):
    """V = 8,000 is the last graph whose sums and ancestors fit LDS (20 bytes
    per vertex); 8,001 takes the global-scratch form."""
    check_path(eng, 8000, EN.INT32, "link_loads_kernel<lds>")
    check_path(eng, 8001, EN.INT32, "link_loads_kernel<global>")


def test_long_path_global_scratch_u32_ancestors(eng):
    """70,000 vertices (ids above 65,535), slot layout, depth 69,999: 17 rounds."""
    check_path(eng, 70000, EN.SLOT, "link_loads_kernel<global>")


def test_single_vertex_and_no_rows(eng):
    csr = T.build_csr([], [], np.zeros(0, np.int64), extra_vertices=[1])
    ex = on(csr)
    eng.load(ex)
    load = zeros_u64(eng, 0)
    keep = raw_loads(eng, csr, np.zeros((1, 1), np.int32), EN.INT32, 1, [0, 3], [0, 0, 5],
                     [1, 2, 3], load)
    eng.ctx.synchronize()
    assert not load.cpu().numpy().any()
    # nrows == 0 and an empty pair list: SDNR_OK, nothing touched (null pointers are fine)
    eng.ctx.link_loads_device(0, _native.TREE_INT32, 0, 0, 0, 0, 0)
    load += 7
    keep = raw_loads(eng, csr, np.zeros((1, 1), np.int32), EN.INT32, 1, [4, 4], [0], None, load)
    eng.ctx.synchronize()
    assert int(load.cpu()[0]) == 7
    del keep


def test_two_components_gaps_repeats_and_bad_destinations(eng):
    from oracle import oracle as O
    csr = random_csr(40, 30, 3)                            # the last fifth is unreachable
    ex = on(csr)
    ids = np.arange(csr.V, dtype=np.int32)
    par, prt, _ = O.dfs_tables(csr, ids)
    assert (par[0] < 0).any()
    rows = np.array([0, 0, 0, 0, 0, 2, 2, 5, 5, 5])       # rows 1, 3, 4 have no pairs
    dsts = np.array([7, 7, 7, 39, -3, 40, 11, 1 << 20, 6, 6])   # repeats, unreached, out of range
    w = np.array([1, 10, 100, 5, 5, 5, 1 << 40, 9, 2, 3], np.uint64)
    want = walk_loads(csr, par, rows, dsts, w, False)
    assert want.any()
    for lay in LAYOUTS:
        tree = par if lay == EN.INT32 else EN.pack_host_tree(par, prt, csr, lay)
        got = eng.link_loads(ex, dev_tree(eng, tree), lay, rows, dsts, w)
        assert np.array_equal(got, want), lay
    assert np.array_equal(EN.link_loads_host(csr, par, EN.INT32, rows, dsts, w), want)


def test_star_rooted_at_a_leaf(eng):
    """300 leaves: every other leaf's demand lands on the hub's accumulator
    in one round."""
    from oracle import oracle as O
    n = 300
    hub, leaves = 1, np.arange(2, n + 2)
    csr = T.build_csr(np.concatenate([np.full(n, hub), leaves]),
                      np.concatenate([leaves, np.full(n, hub)]),
                      np.concatenate([np.arange(1, n + 1), np.ones(n, np.int64)]))
    ex = on(csr)
    root = 17
    par, prt, _ = O.dfs_tables(csr, np.array([root], np.int32))
    rng = np.random.default_rng(8)
    dsts = np.concatenate([np.arange(csr.V), np.arange(csr.V)])
    w = rand_weights(rng, dsts.shape[0])
    rows = np.zeros(dsts.shape[0], np.int64)
    want = walk_loads(csr, par, rows, dsts, w, False)
    for lay in (EN.INT32, EN.PORT16):                       # the hub has 300 links: no slot layout
        tree = par if lay == EN.INT32 else EN.pack_host_tree(par, prt, csr, lay)
        assert np.array_equal(eng.link_loads(ex, dev_tree(eng, tree), lay, rows, dsts, w),
                              want)


def test_sums_pass_2_32_and_wrap_2_64(eng):
    csr = path_csr(3)
    ex = on(csr)
    tree, eidx = path_rooted_at_0(csr, EN.INT32)
    n = 5000
    big = (1 << 32) - 1
    got = eng.link_loads(ex, dev_tree(eng, tree), EN.INT32, np.zeros(n, np.int64),
                         np.full(n, 2), np.full(n, big, np.uint64))
    assert got[eidx].tolist() == [n * big, n * big] and n * big > 1 << 32
    w = np.array([1 << 63, 1 << 63, 5, U64], np.uint64)
    got = eng.link_loads(ex, dev_tree(eng, tree), EN.INT32, np.zeros(4, np.int64),
                         [2, 2, 2, 1], w)
    assert got[eidx].tolist() == [4, 5]                    # (2^64 + 5 + 2^64 - 1) mod 2^64, 5


def test_torus_16_cubed_sampled_rows(eng):
    """V = 4,096 (80 KB of LDS per workgroup), trees about 1,464 hops deep."""
    from oracle import oracle as O
    csr = T.torus3d(16, 16, 16).csr()
    ex = on(csr)
    rng = np.random.default_rng(16)
    srcs = np.sort(rng.choice(csr.V, 64, replace=False)).astype(np.int32)
    par, prt, hops = O.dfs_tables(csr, srcs)
    assert hops.max() > 1000
    n = 64 * 150
    rows = rng.integers(0, 64, n)
    dsts = rng.integers(0, csr.V, n)
    w = rand_weights(rng, n)
    want = EN.link_loads_host(csr, par, EN.INT32, rows, dsts, w)
    assert int(want.sum(dtype=np.uint64)) == \
        sum(int(a) * int(hops[r, d]) for r, d, a in zip(rows, dsts, w)) & U64
    for lay in LAYOUTS:
        tree = par if lay == EN.INT32 else EN.pack_host_tree(par, prt, csr, lay)
        got = eng.link_loads(ex, dev_tree(eng, tree), lay, rows, dsts, w)
        assert np.array_equal(got, want), lay
        assert eng.ctx.last_kernel() == "link_loads_kernel<lds>"


def test_calls_accumulate_into_one_load(eng, small_cases):
    csr, par, _, _, rows, dsts, w, want = small_cases["fat_tree_k8"]
    ex = on(csr)
    eng.load(ex)
    V = csr.V
    order, off = EN._pairs_by_row(rows, V)
    d, ww = dsts[order], w[order]
    half = V // 2
    load = zeros_u64(eng, csr.E)
    k1 = raw_loads(eng, csr, par[:half], EN.INT32, half, off[:half + 1], d, ww, load)
    k2 = raw_loads(eng, csr, par[half:], EN.INT32, V - half, off[half:], d, ww, load, timing=True)
    eng.ctx.synchronize()
    assert np.array_equal(as_u64(load, csr.E), want[(False, True)])
    assert eng.ctx.last_kernel_ms() > 0
    del k1, k2


def test_argument_errors(eng, small_cases):
    csr, par, _, _, rows, dsts, w, _ = small_cases["mock"]
    ex = on(csr)
    eng.load(ex)
    load = zeros_u64(eng, csr.E)
    tree = dev_tree(eng, par)
    import torch
    off = torch.zeros(csr.V + 1, dtype=torch.int64, device=eng.dev)
    L, h = eng.ctx._lib, eng.ctx._h
    import ctypes
    p = lambda t: ctypes.c_void_p(t.data_ptr())           # noqa: E731
    dev = _native.DEVICE_PTRS
    args = (p(tree), 0, csr.V, p(off), p(tree), None, p(load))
    assert L.sdnr_link_loads(h, *args, 0) == -22                          # host pointers
    assert L.sdnr_link_loads(h, p(tree), 7, csr.V, p(off), p(tree), None, p(load), dev) == -22
    assert L.sdnr_link_loads(h, p(tree), _native.TREE_PORT16, csr.V, p(off), p(tree), None,
                             p(load), dev | _native.LOADS_TO_ROOT) == -22
    assert L.sdnr_link_loads(h, None, 0, csr.V, p(off), p(tree), None, p(load), dev) == -22
    assert L.sdnr_link_loads(h, p(tree), 0, csr.V, p(off), p(tree), None, None, dev) == -22
    assert L.sdnr_link_loads(h, p(tree), 0, -1, p(off), p(tree), None, p(load), dev) == -22
    off[0] = 5                                                            # pair_off[0] > pair_off[n]
    torch.cuda.synchronize()
    assert L.sdnr_link_loads(h, *args, dev) == -22
    assert b"monotone" in L.sdnr_last_error()
    with _native.Context(0) as fresh:                                     # no graph uploaded
        assert L.sdnr_link_loads(fresh._h, *args, dev) == -77
    assert not load.cpu().numpy().any()


def test_row_with_a_cycle_is_reported_not_followed(eng, small_cases):
    """A corrupted int32 row holding a 2-cycle: the rounds are bounded, the
    call returns, sdnr_synchronize reports SDNR_ERR_INVAL once, and the
    context goes on working."""
    csr, par, _, _, rows, dsts, w, want = small_cases["fat_tree_k4"]
    ex = on(csr)
    bad = par.copy()
    child = int(np.nonzero((par[0] == 0) & (np.arange(csr.V) != 0))[0][0])
    bad[0, 0] = child                                      # root <-> child
    eng.load(ex)
    load = zeros_u64(eng, csr.E)
    keep = raw_loads(eng, csr, bad[:1], EN.INT32, 1, [0, 2], [child, 3], None, load)
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "not a tree" in str(ei.value)
    eng.ctx.synchronize()                                  # reported once
    got = eng.link_loads(ex, dev_tree(eng, par), EN.INT32, rows, dsts, w)
    assert np.array_equal(got, want[(False, True)])
    del keep


# ------------------------------------------------------------------- k = 48 --

def test_k48_all_host_pairs_demand(eng):
    """All 1,152 host-bearing rows of the k=48 fat-tree with the all-host-pairs
    demand (hosts(s) * hosts(d) per switch pair): the kernel equals the numpy
    restatement, and the loads sum to weight x hops."""
    fabric = T.fat_tree(48)
    csr = fabric.csr()
    ex = on(csr)
    hv, _ = fabric.host_table()
    hc = np.bincount(hv, minlength=csr.V).astype(np.int64)
    srcs = np.nonzero(hc)[0]
    n = srcs.shape[0]
    assert n == 1152
    par, prt, hops = eng.dfs_tables(ex, srcs)
    rows = np.repeat(np.arange(n), n)
    dsts = np.tile(srcs, n)
    w = (hc[srcs][rows] * hc[dsts]).astype(np.uint64)
    got = eng.link_loads(ex, par, EN.INT32, rows, dsts, w, timing=True)
    assert eng.ctx.last_kernel() == "link_loads_kernel<lds>" and eng.ctx.last_kernel_ms() > 0
    hp = hops.cpu().numpy()
    assert int(got.sum(dtype=np.uint64)) == int((w.astype(np.int64) * hp[rows, dsts]).sum())
    want = EN.link_loads_host(csr, par.cpu().numpy(), EN.INT32, rows, dsts, w)
    assert np.array_equal(got, want)
    tree = eng.pack_trees(ex, par, prt, EN.PORT16)
    assert np.array_equal(eng.link_loads(ex, tree, EN.PORT16, rows, dsts, w), want)


# ---------------------------------------------------------------- drop-in --

def fdb_counter(g, n):
    return counter_of([g.fdb(i) for i in range(n)], [1] * n)


@pytest.mark.parametrize("name", ["fat_tree_k48_sample", "torus_32x32x32_sample"])
def test_dropin_golden_pairs_large_fabrics(name):
    from sdnmpi_amd.util.topology_db import TopologyDB
    g = G.Golden(name)
    fabric = g.fabric()
    db = fabric.populate(TopologyDB(batch_sources=False))
    pairs = golden_pairs(g, fabric)
    want = fdb_counter(g, len(pairs))
    assert db.link_loads(pairs).as_dict() == want
    rng = np.random.default_rng(9)
    w = rng.integers(1, 1 << 40, len(pairs)).tolist()
    assert db.link_loads(pairs, w).as_dict() == \
        counter_of([g.fdb(i) for i in range(len(pairs))], w)
    if name.startswith("fat_tree"):
        # a budget of 8 rows: the same loads from several row chunks
        small = fabric.populate(TopologyDB(batch_sources=False,
                                           table_budget=8 * EN.dfs_row_bytes(fabric.csr())))
        assert small.link_loads(pairs).as_dict() == want
        assert small._cache.dfs.cap() == 8 and \
            len(set(a for a, _ in pairs)) > 8


def test_dropin_small_fabric_both_routes_and_link_failure():
    from oracle import oracle as O
    from sdnmpi_amd.util.topology_db import TopologyDB
    fabric = T.fat_tree(8)
    db = fabric.populate(TopologyDB())
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs[::5] for b in macs[::3]]
    w = list(range(1, len(pairs) + 1))

    def check():
        fresh = [db.find_route(a, b) for a, b in pairs]
        assert fresh == [O.find_route_pair(db, a, b) for a, b in pairs]
        assert db.link_loads(pairs, w).as_dict() == counter_of(fresh, w)
        first = [(db.find_route(a, b, True) or [[]])[0] for a, b in pairs]
        assert db.link_loads(pairs, w, route="shortest").as_dict() == counter_of(first, w)

    check()
    allp = [(a, b) for a in macs for b in macs if a != b]
    assert db.all_pairs_link_loads().as_dict() == db.link_loads(allp).as_dict()
    assert db.all_pairs_link_loads("shortest").as_dict() == \
        db.link_loads(allp, route="shortest").as_dict()
    # a failed agg-core tree link (both directions), then the loads again
    t = db.route_tables("dfs")
    a = int(t["dpids"][t["parent"][0][0]])
    ab, ba = db.links[a][1], db.links[1][a]
    db.delete_link(ab)
    db.delete_link(ba)
    check()
    db.add_link(ab)
    db.add_link(ba)
    check()
