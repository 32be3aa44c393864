"""ecmp_loads.hip (sdnr_ecmp_link_loads) on the GPU against
engine.ecmp_link_loads_host, and the drop-in's ecmp_link_loads against the
reference's enumerated route sets.

Tolerance (see test_ecmp_link_loads.py): rtol = 1e-9, atol = 0 where the
expected value is nonzero, exactly 0.0 where it is 0.  The dyadic cases
(power-of-two shares, integer weights: every partial sum exact in any order)
are compared bit for bit."""
import ctypes

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from test_ecmp_link_loads import (RTOL, SPLITS, close, dicts_close, edge_map, ladder_csr,
                                  route_set_loads, splits_differ_csr)
from test_link_loads import golden_pairs, random_csr
from test_link_loads_gpu import on, path_csr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def dev_dist(eng, dist):
    """u16 distance rows as the int16 device plane the engine keeps."""
    import torch
    a = np.ascontiguousarray(np.asarray(dist, np.uint16)).view(np.int16)
    return torch.from_numpy(a).to(eng.dev)


def dest_rows(csr, dsts):
    from oracle import oracle as O
    return O.dest_tables(csr, np.asarray(dsts, np.int32))[0]


def rand_weights(rng, n):
    """u64 weights below 2^32, about 30 % zeros."""
    w = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    w[rng.random(n) < 0.3] = 0
    return w


def raw_ecmp(eng, dist, nrows, off, srcs, w, load, hop=False, timing=False):
    """One sdnr_ecmp_link_loads call on device copies of the arguments, adding
    into the device tensor ``load``; no synchronize."""
    import torch
    keep = [dev_dist(eng, dist),
            torch.from_numpy(np.asarray(off, np.int64)).to(eng.dev),
            torch.from_numpy(np.asarray(srcs, np.int32)).to(eng.dev),
            torch.from_numpy(np.asarray(w, np.uint64).view(np.int64)).to(eng.dev)
            if w is not None else None]
    torch.cuda.synchronize()
    eng.ctx.ecmp_link_loads_device(keep[0].data_ptr(), nrows, keep[1].data_ptr(),
                                   keep[2].data_ptr(),
                                   keep[3].data_ptr() if keep[3] is not None else 0,
                                   load.data_ptr(), hop=hop, timing=timing)
    return keep


def zeros_f64(eng, n):
    import torch
    return torch.zeros(max(1, n), dtype=torch.float64, device=eng.dev)


def check(eng, csr, dist, rows, srcs, w, kernel="ecmp_loads_kernel<lds>"):
    """Both splits on the GPU against the host restatement; returns the
    expected loads per split."""
    ex = on(csr)
    d_dist = dev_dist(eng, dist)
    out = {}
    for split in SPLITS:
        want = EN.ecmp_link_loads_host(csr, dist, rows, srcs, w, split)
        got = eng.ecmp_link_loads(ex, d_dist, rows, srcs, w, split)
        assert got.dtype == np.float64 and close(got, want), split
        if csr.E and len(rows):
            assert eng.ctx.last_kernel() == kernel
            assert eng.ctx.last_launches() == 1
        out[split] = want
    return out


# ------------------------------------------------------ the small fabrics --

@pytest.fixture(scope="module")
def small_cases():
    """Per G.SMALL fabric: the distance rows of every destination from the
    oracle, a demand of 5 random sources per row, and the expected loads,
    computed once."""
    out = {}
    for k, name in enumerate(G.SMALL):
        csr = G.Golden(name).fabric().csr()
        dist = dest_rows(csr, np.arange(csr.V))
        rng = np.random.default_rng(70 + k)
        n = 5 * csr.V
        rows = np.repeat(np.arange(csr.V), 5)
        srcs = rng.integers(0, csr.V, n)
        w = rand_weights(rng, n)
        want = {(split, wt is not None): EN.ecmp_link_loads_host(csr, dist, rows, srcs, wt, split)
                for split in SPLITS for wt in (w, None)}
        out[name] = (csr, dist, rows, srcs, w, want)
    return out


@pytest.mark.parametrize("name", G.SMALL)
def test_small_fabrics_every_destination_row_both_splits(eng, small_cases, name):
    csr, dist, rows, srcs, w, want = small_cases[name]
    ex = on(csr)
    d_dist = dev_dist(eng, dist)
    for split in SPLITS:
        for wt in (w, None):
            got = eng.ecmp_link_loads(ex, d_dist, rows, srcs, wt, split)
            assert close(got, want[(split, wt is not None)]), (name, split)
            assert eng.ctx.last_kernel() == "ecmp_loads_kernel<lds>"
            assert eng.ctx.last_launches() == 1


@pytest.mark.parametrize("name", G.MULTI)
def test_dropin_equals_reference_route_sets(name):
    from sdnmpi_amd.util.topology_db import SplitLinkLoads, TopologyDB
    g = G.Golden(name)
    fabric = g.fabric()
    db = fabric.populate(TopologyDB())
    pairs = golden_pairs(g, fabric)
    sets = [g.multi(i) for i in range(len(pairs))]
    got = db.ecmp_link_loads(pairs)
    assert isinstance(got, SplitLinkLoads)
    assert dicts_close(got.as_dict(), route_set_loads(sets, [1] * len(pairs)))
    rng = np.random.default_rng(6)
    w = rng.integers(0, 1 << 32, len(pairs)).tolist()
    assert dicts_close(db.ecmp_link_loads(pairs, w).as_dict(), route_set_loads(sets, w))
    macs = fabric.host_macs()
    allp = [(a, b) for a in macs for b in macs if a != b]
    for split in SPLITS:
        assert dicts_close(db.all_pairs_ecmp_link_loads(split).as_dict(),
                           db.ecmp_link_loads(allp, split=split).as_dict())


# --------------------------------------------------------- bit-exact cases --

@pytest.mark.parametrize("k", [4, 8])
def test_fat_tree_dyadic_loads_are_bit_exact(eng, k):
    """Between host-bearing (edge) switches every route count of a fat-tree
    is a power of two ((k/2)^2, k/2, 1), so with integer weights every share
    and every partial sum is exact in any order of the atomics."""
    fabric = T.fat_tree(k)
    csr = fabric.csr()
    hv = np.unique(fabric.host_table()[0])
    dist = dest_rows(csr, hv)
    rng = np.random.default_rng(k)
    n = hv.shape[0]
    rows = np.repeat(np.arange(n), n)
    srcs = np.tile(hv, n)
    w = rng.integers(0, 1 << 20, n * n, dtype=np.uint64)
    d_dist = dev_dist(eng, dist)
    for split in SPLITS:
        want = EN.ecmp_link_loads_host(csr, dist, rows, srcs, w, split)
        scaled = want * 2.0 ** 12
        assert np.array_equal(scaled, np.floor(scaled)) and scaled.max() < 2.0 ** 53
        assert want.any()
        got = eng.ecmp_link_loads(on(csr), d_dist, rows, srcs, w, split)
        assert np.array_equal(got, want), split


def test_ladder_of_70_diamonds_where_the_u64_counts_saturate(eng):
    """2^70 shortest routes end to end: sdnr_ecmp_counts saturates on the row,
    the f64 counts do not, and every link toward the far end carries w / 2."""
    csr = ladder_csr(70)
    assert csr.V == 211
    ex = on(csr)
    dist = dest_rows(csr, [csr.V - 1])
    eng.load(ex)
    assert int(eng.ctx.ecmp_counts(dist)[0, 0]) == (1 << 64) - 1
    esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    toward = dist[0][esrc] == dist[0][csr.col].astype(np.int64) + 1
    w = 987654321
    for split in SPLITS:
        got = eng.ecmp_link_loads(ex, dev_dist(eng, dist), [0], [0], [w], split)
        assert np.array_equal(got, np.where(toward, w / 2, 0.0)), split
        assert eng.ctx.last_kernel() == "ecmp_loads_kernel<lds>"


# ------------------------------------------------ shapes that break level DPs --

def test_single_vertex_two_vertices_and_no_rows(eng):
    csr = T.build_csr([], [], np.zeros(0, np.int64), extra_vertices=[1])
    ex = on(csr)
    eng.load(ex)
    load = zeros_f64(eng, 0)
    load += 7
    keep = raw_ecmp(eng, np.zeros((1, 1), np.uint16), 1, [0, 3], [0, 0, 5], [1, 2, 3], load)
    eng.ctx.synchronize()
    # nrows == 0 and an empty pair list: SDNR_OK, nothing touched (null pointers are fine)
    eng.ctx.ecmp_link_loads_device(0, 0, 0, 0, 0, 0)
    keep2 = raw_ecmp(eng, np.zeros((1, 1), np.uint16), 1, [4, 4], [0], None, load)
    eng.ctx.synchronize()
    assert float(load.cpu()[0]) == 7.0
    assert eng.ecmp_link_loads(ex, dev_dist(eng, np.zeros((1, 1))), [0], [0]).shape == (0,)
    del keep, keep2
    csr = path_csr(2)
    dist = dest_rows(csr, [0, 1])
    want = check(eng, csr, dist, [0, 0, 1, 1, 1], [1, 0, 0, 0, 7], np.array([5, 9, 2, 4, 1]))
    edge = edge_map(csr)
    assert want["route"][edge[(1, 0)]] == 5.0 and want["route"][edge[(0, 1)]] == 6.0


def test_path_with_more_levels_than_a_wave_has_lanes(eng):
    csr = path_csr(70)
    dist = dest_rows(csr, [0, 69, 35])
    assert dist.max() == 69
    rng = np.random.default_rng(70)
    rows = rng.integers(0, 3, 200)
    srcs = rng.integers(0, 70, 200)
    check(eng, csr, dist, rows, srcs, rand_weights(rng, 200))
    # one pair end to end: every link toward vertex 0 carries the whole weight
    got = eng.ecmp_link_loads(on(csr), dev_dist(eng, dist), [0], [69], [3], "route")
    edge = edge_map(csr)
    want = np.zeros(csr.E)
    want[[edge[(v, v - 1)] for v in range(1, 70)]] = 3.0
    assert np.array_equal(got, want)


def star_csr(n):
    hub, leaves = 1, np.arange(2, n + 2)
    return T.build_csr(np.concatenate([np.full(n, hub), leaves]),
                       np.concatenate([leaves, np.full(n, hub)]),
                       np.concatenate([np.arange(1, n + 1), np.ones(n, np.int64)]))


def test_star_with_100_leaves(eng):
    """The hub has degree 100 (> 64), and 99 leaves add into its flow word."""
    csr = star_csr(100)
    dist = dest_rows(csr, [17, 0])                         # toward a leaf, toward the hub
    rows = np.concatenate([np.zeros(csr.V, np.int64), np.ones(csr.V, np.int64)])
    srcs = np.concatenate([np.arange(csr.V), np.arange(csr.V)])
    w = rand_weights(np.random.default_rng(8), rows.shape[0]) + np.uint64(1)
    want = check(eng, csr, dist, rows, srcs, w)
    edge = edge_map(csr)
    into_leaf = float(w[:csr.V].astype(np.float64).sum() - float(w[17]))
    assert want["route"][edge[(0, 17)]] == pytest.approx(into_leaf, rel=RTOL)


def test_forty_middles_give_shares_that_are_not_dyadic(eng):
    """s -> 40 middles -> d: every middle link carries w / 40."""
    s, d = 1, 42
    mids = np.arange(2, 42)
    src = np.concatenate([np.full(40, s), mids, mids, np.full(40, d)])
    dst = np.concatenate([mids, np.full(40, s), np.full(40, d), mids])
    order = np.lexsort((dst, src))
    csr = T.build_csr(src[order], dst[order], np.arange(160) % 60 + 1)
    dist = dest_rows(csr, [41])
    assert dist[0, 0] == 2
    want = check(eng, csr, dist, [0], [0], np.array([7], np.uint64))
    edge = edge_map(csr)
    for m in range(1, 41):
        for split in SPLITS:
            assert want[split][edge[(0, m)]] == pytest.approx(7 / 40, rel=RTOL)
            assert want[split][edge[(m, 41)]] == pytest.approx(7 / 40, rel=RTOL)


def test_source_equal_to_destination_and_repeated_pairs(eng, small_cases):
    csr, dist, _, _, _, _ = small_cases["fat_tree_k4"]
    ex = on(csr)
    d_dist = dev_dist(eng, dist)
    far = int(np.argmax(dist[3]))
    for split in SPLITS:
        assert not eng.ecmp_link_loads(ex, d_dist, [3, 5], [3, 5], [10, 20], split).any()
        one = eng.ecmp_link_loads(ex, d_dist, [3], [far], [11], split)
        three = eng.ecmp_link_loads(ex, d_dist, [3, 3, 3], [far, far, far], [11, 11, 11], split)
        assert one.any() and np.array_equal(three, 3 * one)          # (dyadic shares)
    check(eng, csr, dist, [3, 3, 3, 3], [far, 3, far, far], np.array([1, 5, 2, 3]))


# ------------------------------------------------------------ accumulation --

def test_calls_accumulate_and_row_chunks_sum_to_the_whole(eng, small_cases):
    csr, dist, rows, srcs, w, want = small_cases["jellyfish_n60_r5"]
    ex = on(csr)
    eng.load(ex)
    V = csr.V
    order, off = EN._pairs_by_row(rows, V)
    s, ww = srcs[order], w[order]
    half = V // 2
    for split in SPLITS:
        hop = split == "hop"
        whole = want[(split, True)]
        # a demand in two row chunks, into one load
        load = zeros_f64(eng, csr.E)
        k1 = raw_ecmp(eng, dist[:half], half, off[:half + 1], s, ww, load, hop)
        k2 = raw_ecmp(eng, dist[half:], V - half, off[half:], s, ww, load, hop, timing=True)
        eng.ctx.synchronize()
        assert close(load.cpu().numpy()[:csr.E], whole)
        assert eng.ctx.last_kernel_ms() > 0
        # a second call into the un-zeroed load: the sum
        k3 = raw_ecmp(eng, dist, V, off, s, None, load, hop)
        eng.ctx.synchronize()
        assert close(load.cpu().numpy()[:csr.E], whole + want[(split, False)])
        del k1, k2, k3


# ------------------------------------------------------------- global form --

def test_both_sides_of_the_lds_threshold(eng):
    """V = 9,000 is the last graph whose levels, counts and flows fit LDS (18
    bytes per vertex); 9,001 keeps counts and flows in the context scratch."""
    for V, kernel in ((9000, "ecmp_loads_kernel<lds>"), (9001, "ecmp_loads_kernel<global>")):
        csr = random_csr(V, 3 * V, 9)
        dsts = [0, 4321, 7000]
        dist = dest_rows(csr, dsts)
        assert (dist == 0xFFFF).any() and dist[dist != 0xFFFF].max() > 5
        rng = np.random.default_rng(V)
        rows = rng.integers(0, 3, 600)
        srcs = rng.integers(0, V, 600)
        want = check(eng, csr, dist, rows, srcs, rand_weights(rng, 600), kernel)
        assert want["route"].any() and not np.array_equal(want["route"], want["hop"])


# ------------------------------------------------- inconsistent distance rows --

def test_row_that_is_no_bfs_labelling_is_reported_and_its_flow_dropped(eng):
    csr, names = splits_differ_csr()
    s, a, b, m, m1, m2, d = (int(csr.index_of([x])[0]) for x in names)
    ex = on(csr)
    eng.load(ex)
    dist = dest_rows(csr, [d])
    for level in (5, 200):                                 # no next hop; a level >= V
        bad = dist.copy()
        bad[0, a] = level
        load = zeros_f64(eng, csr.E)
        keep = raw_ecmp(eng, bad, 1, [0, 2], [s, a], [6, 6], load)
        with pytest.raises(_native.SdnrError) as ei:
            eng.ctx.synchronize()
        assert ei.value.code == -22 and "BFS labelling" in str(ei.value)
        eng.ctx.synchronize()                              # reported once
        assert np.isfinite(load.cpu().numpy()).all()
        del keep
    check(eng, csr, dist, [0, 0], [s, a], np.array([6, 6]))    # the context goes on working


def test_argument_errors(eng, small_cases):
    import torch
    csr, dist, _, _, _, _ = small_cases["mock"]
    ex = on(csr)
    eng.load(ex)
    load = zeros_f64(eng, csr.E)
    d_dist = dev_dist(eng, dist)
    srcs = torch.zeros(8, dtype=torch.int32, device=eng.dev)
    off = torch.zeros(csr.V + 1, dtype=torch.int64, device=eng.dev)
    L, h = eng.ctx._lib, eng.ctx._h
    p = lambda t: ctypes.c_void_p(t.data_ptr())           # noqa: E731
    dev = _native.DEVICE_PTRS
    args = (p(d_dist), csr.V, p(off), p(srcs), None, p(load))
    assert L.sdnr_ecmp_link_loads(h, *args, 0) == -22                     # host pointers
    assert L.sdnr_ecmp_link_loads(h, None, csr.V, p(off), p(srcs), None, p(load), dev) == -22
    assert L.sdnr_ecmp_link_loads(h, p(d_dist), csr.V, None, p(srcs), None, p(load), dev) == -22
    assert L.sdnr_ecmp_link_loads(h, p(d_dist), csr.V, p(off), p(srcs), None, None, dev) == -22
    assert L.sdnr_ecmp_link_loads(h, p(d_dist), -1, p(off), p(srcs), None, p(load), dev) == -22
    off[csr.V] = 2                                                        # pairs, but no srcs
    torch.cuda.synchronize()
    assert L.sdnr_ecmp_link_loads(h, p(d_dist), csr.V, p(off), None, None, p(load), dev) == -22
    off[0] = 5                                                            # pair_off[0] > pair_off[n]
    torch.cuda.synchronize()
    assert L.sdnr_ecmp_link_loads(h, *args, dev) == -22
    assert b"monotone" in L.sdnr_last_error()
    with _native.Context(0) as fresh:                                     # no graph uploaded
        assert L.sdnr_ecmp_link_loads(fresh._h, *args, dev) == -77
    assert not load.cpu().numpy().any()


# ------------------------------------------------------------------- k = 48 --

@pytest.fixture(scope="module")
def k48(eng):
    fabric = T.fat_tree(48)
    csr = fabric.csr()
    hv = fabric.host_table()[0]
    hc = np.bincount(hv, minlength=csr.V).astype(np.int64)
    srcs = np.nonzero(hc)[0]
    assert srcs.shape[0] == 1152
    dist, _, _ = eng.shortest_tables(on(csr), srcs)
    return csr, hc, srcs, dist


def test_k48_eight_rows_every_host_bearing_source(eng, k48):
    csr, hc, srcs, dist = k48
    n = srcs.shape[0]
    pick = np.array([0, 1, 23, 24, 500, 777, 1150, 1151])
    rows = np.repeat(pick, n)
    s = np.tile(srcs, pick.shape[0])
    w = (hc[s] * hc[srcs[rows]]).astype(np.uint64)
    hd = dist.cpu().numpy()
    for split in SPLITS:
        want = EN.ecmp_link_loads_host(csr, hd, rows, s, w, split)
        got = eng.ecmp_link_loads(on(csr), dist, rows, s, w, split, timing=True)
        assert close(got, want) and want.any(), split
        assert eng.ctx.last_kernel() == "ecmp_loads_kernel<lds>"
        assert eng.ctx.last_kernel_ms() > 0


def test_k48_all_host_pairs_demand_is_conserved(eng, k48):
    """All 1,152 rows of the all-host-pairs demand: whatever the split, a pair
    loads dist(s, d) links with its whole weight, so the loads sum to the
    sum of w x dist(s, d) (computed in integers from the distance rows)."""
    csr, hc, srcs, dist = k48
    n = srcs.shape[0]
    rows = np.repeat(np.arange(n), n)
    s = np.tile(srcs, n)
    w = (hc[s] * hc[srcs[rows]]).astype(np.uint64)
    hd = dist.cpu().numpy().view(np.uint16).astype(np.int64)
    assert hd.max() < 0xFFFF
    total = int((w.astype(np.int64) * hd[rows, s]).sum())
    for split in SPLITS:
        got = eng.ecmp_link_loads(on(csr), dist, rows, s, w, split)
        assert np.isfinite(got).all() and (got >= 0).all()
        assert abs(float(got.sum()) - total) <= RTOL * total, split
        # ECMP loads every core uplink alike, where routes[0] fills the first cores only
        assert got.min() > 0
