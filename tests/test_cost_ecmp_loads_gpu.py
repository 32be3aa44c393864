"""cost_ecmp_loads.hip (sdnr_cost_ecmp_link_loads) on the GPU against
engine.cost_ecmp_link_loads_host, and the drop-in's least_cost_ecmp_link_loads
against the enumerated least-cost route sets.

Tolerance (see test_ecmp_link_loads.py): rtol = 1e-9, atol = 0 where the
expected value is nonzero, exactly 0.0 where it is 0.  The dyadic cases
(power-of-two shares, integer weights: every partial sum exact in any order)
are compared bit for bit.  On the small cases pcost comes from
engine.cost_tables_host, so a fault in this kernel is not one of
cost_tables.hip."""
import ctypes

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from test_cost_ecmp_loads import (chord_ladder_csr, diamond_csr, digraph_csr, both_ways,
                                  edge_costs, paid, path_csr_costs, pcost_rows, random_costs)
from test_ecmp_link_loads import (RTOL, SPLITS, close, dicts_close, edge_map, route_set_loads,
                                  splits_differ_csr)
from test_ecmp_link_loads_gpu import dest_rows, rand_weights, star_csr, zeros_f64
from test_link_loads import golden_pairs, random_csr
from test_link_loads_gpu import on

pytestmark = pytest.mark.gpu

LDS, GLOBAL = "cost_ecmp_loads_kernel<lds>", "cost_ecmp_loads_kernel<global>"


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def dev_pcost(eng, pcost):
    """u32 pcost rows as the int32 device plane the engine keeps."""
    import torch
    a = np.ascontiguousarray(np.asarray(pcost, np.uint32)).view(np.int32)
    return torch.from_numpy(a).to(eng.dev)


def raw(eng, pcost, nrows, off, srcs, w, load, hop=False, timing=False):
    """One sdnr_cost_ecmp_link_loads call on device copies of the arguments,
    adding into the device tensor ``load``; no synchronize."""
    import torch
    keep = [dev_pcost(eng, pcost),
            torch.from_numpy(np.asarray(off, np.int64)).to(eng.dev),
            torch.from_numpy(np.asarray(srcs, np.int32)).to(eng.dev),
            torch.from_numpy(np.asarray(w, np.uint64).view(np.int64)).to(eng.dev)
            if w is not None else None]
    torch.cuda.synchronize()
    eng.ctx.cost_ecmp_link_loads_device(keep[0].data_ptr(), nrows, keep[1].data_ptr(),
                                        keep[2].data_ptr(),
                                        keep[3].data_ptr() if keep[3] is not None else 0,
                                        load.data_ptr(), hop=hop, timing=timing)
    return keep


def check(eng, csr, cost, pcost, rows, srcs, w, kernel=LDS):
    """Both splits, with and without the weights, on the GPU against the host
    restatement; returns the expected weighted loads per split."""
    ex = on(csr)
    d_pc = dev_pcost(eng, pcost)
    out = {}
    for split in SPLITS:
        for wt in (w, None):
            want = EN.cost_ecmp_link_loads_host(csr, cost, pcost, rows, srcs, wt, split)
            got = eng.cost_ecmp_link_loads(ex, cost, d_pc, rows, srcs, wt, split)
            assert got.dtype == np.float64 and close(got, want), split
            assert eng.ctx.last_kernel() == kernel
            assert eng.ctx.last_launches() == 1
            if wt is not None:
                out[split] = want
    return out


# ------------------------------------------------------ the small fabrics --

@pytest.fixture(scope="module")
def small_cases():
    """Per G.SMALL fabric: costs in [1, 5] (a cost per direction), the host's
    pcost rows of every destination, a demand of 5 random sources per row
    (ids outside [0, V) and s == d among them) and the expected loads,
    computed once."""
    out = {}
    for k, name in enumerate(G.SMALL):
        csr = G.Golden(name).fabric().csr()
        V = int(csr.V)
        cost = random_costs(csr, 1, 5, 300 + k)
        pcost = pcost_rows(csr, cost, np.arange(V))
        rng = np.random.default_rng(170 + k)
        n = 5 * V
        rows = np.repeat(np.arange(V), 5)
        srcs = rng.integers(-1, V + 1, n)
        srcs[::11] = rows[::11]                              # s == d
        w = rand_weights(rng, n)
        want = {(split, wt is not None):
                EN.cost_ecmp_link_loads_host(csr, cost, pcost, rows, srcs, wt, split)
                for split in SPLITS for wt in (w, None)}
        out[name] = (csr, cost, pcost, rows, srcs, w, want)
    return out


@pytest.mark.parametrize("name", G.SMALL)
def test_small_fabrics_every_destination_row_both_splits(eng, small_cases, name):
    csr, cost, pcost, rows, srcs, w, want = small_cases[name]
    ex = on(csr)
    d_pc = dev_pcost(eng, pcost)
    assert ((srcs < 0) | (srcs >= csr.V)).any() and (srcs == rows).any()
    for split in SPLITS:
        for wt in (w, None):
            got = eng.cost_ecmp_link_loads(ex, cost, d_pc, rows, srcs, wt, split)
            assert close(got, want[(split, wt is not None)]), (name, split)
            assert eng.ctx.last_kernel() == LDS
            assert eng.ctx.last_launches() == 1
    # a numpy pcost plane is uploaded by the engine
    assert close(eng.cost_ecmp_link_loads(ex, cost, pcost, rows, srcs, w), want[("route", True)])


# ------------------------------------------------ shapes that break level DPs --

def test_direct_link_ties_a_two_link_route(eng):
    csr, cost, (s, m, d) = diamond_csr()
    pcost = pcost_rows(csr, cost, [d])
    edge = edge_map(csr)
    want = np.zeros(int(csr.E))
    want[[edge[(s, d)], edge[(s, m)], edge[(m, d)]]] = 5.0
    for split in SPLITS:
        got = eng.cost_ecmp_link_loads(on(csr), cost, dev_pcost(eng, pcost), [0], [s], [10], split)
        assert np.array_equal(got, want), split
        assert eng.ctx.last_kernel() == LDS and eng.ctx.last_launches() == 1


def test_ladder_of_20_diamonds_with_chords(eng):
    """Depth (40 at the far end) and hop count (20) diverge along the whole
    graph; every least-cost link carries a third of the weight."""
    csr, cost = chord_ladder_csr(20)
    V = int(csr.V)
    pcost = pcost_rows(csr, cost, [V - 1, 0, 30])
    rng = np.random.default_rng(20)
    rows = rng.integers(0, 3, 150)
    srcs = rng.integers(0, V, 150)
    check(eng, csr, cost, pcost, rows, srcs, rand_weights(rng, 150))
    esrc = np.repeat(np.arange(V), np.diff(csr.row_ptr))
    toward = pcost[0][esrc].astype(np.int64) == pcost[0][csr.col].astype(np.int64) + cost
    for split in SPLITS:
        got = eng.cost_ecmp_link_loads(on(csr), cost, dev_pcost(eng, pcost), [0], [0], [9], split)
        assert close(got, np.where(toward, 3.0, 0.0)), split


def test_path_with_more_depths_than_a_wave_has_lanes(eng):
    csr, cost = path_csr_costs(70)
    pcost = pcost_rows(csr, cost, [0, 69, 35])
    rng = np.random.default_rng(70)
    rows = rng.integers(0, 3, 200)
    srcs = rng.integers(0, 70, 200)
    check(eng, csr, cost, pcost, rows, srcs, rand_weights(rng, 200))
    # one pair end to end: every link toward vertex 0 carries the whole weight
    got = eng.cost_ecmp_link_loads(on(csr), cost, dev_pcost(eng, pcost), [0], [69], [3], "route")
    edge = edge_map(csr)
    want = np.zeros(int(csr.E))
    want[[edge[(v, v - 1)] for v in range(1, 70)]] = 3.0
    assert np.array_equal(got, want)


def test_star_with_100_leaves(eng):
    """The hub has degree 100 (> 64), and 99 leaves add into its flow word."""
    csr = star_csr(100)
    cost = random_costs(csr, 1, 5, 8)
    pcost = pcost_rows(csr, cost, [17, 0])                 # toward a leaf, toward the hub
    rows = np.concatenate([np.zeros(csr.V, np.int64), np.ones(csr.V, np.int64)])
    srcs = np.concatenate([np.arange(csr.V), np.arange(csr.V)])
    w = rand_weights(np.random.default_rng(8), rows.shape[0]) + np.uint64(1)
    want = check(eng, csr, cost, pcost, rows, srcs, w)
    edge = edge_map(csr)
    into_leaf = float(w[:csr.V].astype(np.float64).sum() - float(w[17]))
    assert want["route"][edge[(0, 17)]] == pytest.approx(into_leaf, rel=RTOL)


def test_three_middles_give_shares_that_are_not_dyadic(eng):
    """s -> 3 middles -> d at equal costs: every middle link carries w / 3."""
    s, d = 0, 4
    csr = digraph_csr(both_ways([(s, m) for m in (1, 2, 3)] + [(m, d) for m in (1, 2, 3)]))
    cost = np.full(int(csr.E), 4, np.uint32)
    pcost = pcost_rows(csr, cost, [d])
    assert int(pcost[0, s]) == 8
    want = check(eng, csr, cost, pcost, [0], [s], np.array([7], np.uint64))
    edge = edge_map(csr)
    for m in (1, 2, 3):
        for split in SPLITS:
            assert want[split][edge[(s, m)]] == pytest.approx(7 / 3, rel=RTOL)
            assert want[split][edge[(m, d)]] == pytest.approx(7 / 3, rel=RTOL)


def test_route_split_and_hop_split_differ_under_costs(eng):
    """splits_differ_csr with unit costs, then with unit costs on all links but
    one (b -> s at 2, which no route toward d takes): three least-cost routes,
    two of them through b, so s sends 2 : 4 by route and 3 : 3 by hop."""
    csr, names = splits_differ_csr()
    s, a, b, m, m1, m2, d = (int(csr.index_of([x])[0]) for x in names)
    edge = edge_map(csr)
    unit = np.ones(int(csr.E), np.uint32)
    pcost = pcost_rows(csr, unit, [d])
    want = check(eng, csr, unit, pcost, [0], [s], np.array([6], np.uint64))
    assert want["route"][edge[(s, a)]] == pytest.approx(2.0, rel=RTOL)
    assert want["hop"][edge[(s, a)]] == 3.0
    cost = edge_costs(csr, {(b, s): 2})
    want = check(eng, csr, cost, pcost_rows(csr, cost, [d]), [0], [s], np.array([6], np.uint64))
    assert not np.array_equal(want["route"], want["hop"])
    assert want["hop"][edge[(b, m1)]] == 1.5 and want["route"][edge[(b, m1)]] == \
        pytest.approx(2.0, rel=RTOL)


def test_source_equal_to_destination_repeated_pairs_and_no_rows(eng, small_cases):
    csr, cost, pcost, _, _, _, _ = small_cases["fat_tree_k4"]
    ex = on(csr)
    d_pc = dev_pcost(eng, pcost)
    far = int(np.argmax(pcost[3]))
    for split in SPLITS:
        assert not eng.cost_ecmp_link_loads(ex, cost, d_pc, [3, 5], [3, 5], [10, 20], split).any()
        one = eng.cost_ecmp_link_loads(ex, cost, d_pc, [3], [far], [11], split)
        three = eng.cost_ecmp_link_loads(ex, cost, d_pc, [3, 3, 3], [far] * 3, [11] * 3, split)
        assert one.any() and close(three, 3 * one)
    # nrows == 0 and an empty pair list: SDNR_OK, nothing touched (null pointers are fine)
    load = zeros_f64(eng, csr.E)
    load += 7
    eng.ctx.cost_ecmp_link_loads_device(0, 0, 0, 0, 0, 0)
    keep = raw(eng, pcost[:1], 1, [4, 4], [0], None, load)
    eng.ctx.synchronize()
    assert (load.cpu().numpy() == 7.0).all()
    del keep


# --------------------------------------------------------- bit-exact cases --

@pytest.mark.parametrize("k", [4, 8])
def test_fat_tree_uniform_tier_costs_are_bit_exact(eng, k):
    """Edge-aggregation links at 3, aggregation-core links at 5: between edge
    switches the least-cost DAG is the hop-count DAG, every route count a
    power of two, so with integer weights below 2^20 the loads are bit-equal
    to the host checker and to ecmp_link_loads on the hop-distance rows."""
    import torch
    fabric = T.fat_tree(k)
    csr = fabric.csr()
    h = k // 2
    esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    core = (esrc < h * h) | (np.asarray(csr.col) < h * h)
    cost = np.where(core, 5, 3).astype(np.uint32)
    hv = np.unique(fabric.host_table()[0])
    pcost = pcost_rows(csr, cost, hv)
    dist = dest_rows(csr, hv)
    rng = np.random.default_rng(k)
    n = hv.shape[0]
    rows = np.repeat(np.arange(n), n)
    srcs = np.tile(hv, n)
    w = rng.integers(0, 1 << 20, n * n, dtype=np.uint64)
    ex = on(csr)
    d_dist = torch.from_numpy(np.ascontiguousarray(dist).view(np.int16)).to(eng.dev)
    for split in SPLITS:
        want = EN.cost_ecmp_link_loads_host(csr, cost, pcost, rows, srcs, w, split)
        scaled = want * 2.0 ** 12
        assert np.array_equal(scaled, np.floor(scaled)) and scaled.max() < 2.0 ** 53
        assert want.any()
        got = eng.cost_ecmp_link_loads(ex, cost, dev_pcost(eng, pcost), rows, srcs, w, split)
        assert np.array_equal(got, want), split
        assert np.array_equal(got, eng.ecmp_link_loads(ex, d_dist, rows, srcs, w, split)), split


# ------------------------------------------------------------ accumulation --

def test_calls_accumulate_and_row_chunks_sum_to_the_whole(eng, small_cases):
    csr, cost, pcost, rows, srcs, w, want = small_cases["jellyfish_n60_r5"]
    ex = on(csr)
    eng.set_link_costs(ex, cost)
    V = csr.V
    order, off = EN._pairs_by_row(rows, V)
    s = np.where((srcs < 0) | (srcs >= V), -1, srcs)[order]
    ww = w[order]
    half = V // 2
    for split in SPLITS:
        hop = split == "hop"
        whole = want[(split, True)]
        # a demand in two row chunks, into one load
        load = zeros_f64(eng, csr.E)
        k1 = raw(eng, pcost[:half], half, off[:half + 1], s, ww, load, hop)
        k2 = raw(eng, pcost[half:], V - half, off[half:], s, ww, load, hop, timing=True)
        eng.ctx.synchronize()
        assert close(load.cpu().numpy()[:csr.E], whole)
        assert eng.ctx.last_kernel_ms() > 0
        # a second call into the un-zeroed load: the sum
        k3 = raw(eng, pcost, V, off, s, None, load, hop)
        eng.ctx.synchronize()
        assert close(load.cpu().numpy()[:csr.E], whole + want[(split, False)])
        del k1, k2, k3


# ------------------------------------------------------------- global form --

def test_both_sides_of_the_lds_bound(eng):
    """V = kCostEcmpLdsMaxV is the last graph whose counts, flows, costs and
    depths fit LDS (22 bytes per vertex); one more keeps counts, flows and
    depths in the context scratch."""
    bound = EN.COST_ECMP_LDS_MAX_V
    for V, kernel in ((bound, LDS), (bound + 1, GLOBAL)):
        csr = random_csr(V, 3 * V, 9)
        cost = random_costs(csr, 1, 5, V)
        pcost = pcost_rows(csr, cost, [0, 4321, 7000])
        assert (pcost == EN.COST_INF).any()                # at least one vertex is unreachable
        rng = np.random.default_rng(V)
        rows = rng.integers(0, 3, 600)
        srcs = rng.integers(0, V, 600)
        want = check(eng, csr, cost, pcost, rows, srcs, rand_weights(rng, 600), kernel)
        assert want["route"].any() and not np.array_equal(want["route"], want["hop"])


# ---------------------------------------------------- inconsistent pcost rows --

def test_row_that_is_no_least_cost_labelling_is_reported_and_its_flow_dropped(eng):
    csr, names = splits_differ_csr()
    s, a, b, m, m1, m2, d = (int(csr.index_of([x])[0]) for x in names)
    ex = on(csr)
    cost = np.ones(int(csr.E), np.uint32)
    eng.set_link_costs(ex, cost)
    pcost = pcost_rows(csr, cost, [d])
    bad = pcost.copy()
    bad[0, a] = 7                                          # no neighbour of a at cost 6
    for hop in (False, True):
        load = zeros_f64(eng, csr.E)
        keep = raw(eng, bad, 1, [0, 2], [s, a], [6, 6], load, hop)
        with pytest.raises(_native.SdnrError) as ei:
            eng.ctx.synchronize()
        assert ei.value.code == -22 and "least-cost labelling" in str(ei.value)
        eng.ctx.synchronize()                              # reported once
        assert np.isfinite(load.cpu().numpy()).all()
        del keep
    check(eng, csr, cost, pcost, [0, 0], [s, a], np.array([6, 6]))   # the context goes on working


def test_argument_errors(eng, small_cases):
    import torch
    csr, cost, pcost, _, _, _, _ = small_cases["mock"]
    ex = on(csr)
    eng.set_link_costs(ex, cost)
    load = zeros_f64(eng, csr.E)
    d_pc = dev_pcost(eng, pcost)
    srcs = torch.zeros(8, dtype=torch.int32, device=eng.dev)
    off = torch.zeros(csr.V + 1, dtype=torch.int64, device=eng.dev)
    L, h = eng.ctx._lib, eng.ctx._h
    p = lambda t: ctypes.c_void_p(t.data_ptr())           # noqa: E731
    dev = _native.DEVICE_PTRS
    fn = L.sdnr_cost_ecmp_link_loads
    args = (p(d_pc), csr.V, p(off), p(srcs), None, p(load))
    assert fn(h, *args, 0) == -22                                         # host pointers
    assert fn(h, None, csr.V, p(off), p(srcs), None, p(load), dev) == -22
    assert fn(h, p(d_pc), csr.V, None, p(srcs), None, p(load), dev) == -22
    assert fn(h, p(d_pc), csr.V, p(off), p(srcs), None, None, dev) == -22
    assert fn(h, p(d_pc), -1, p(off), p(srcs), None, p(load), dev) == -22
    off[csr.V] = 2                                                        # pairs, but no srcs
    torch.cuda.synchronize()
    assert fn(h, p(d_pc), csr.V, p(off), None, None, p(load), dev) == -22
    off[0] = 5                                                            # pair_off[0] > pair_off[n]
    torch.cuda.synchronize()
    assert fn(h, *args, dev) == -22
    assert b"monotone" in L.sdnr_last_error()
    off[0] = 0
    torch.cuda.synchronize()
    eng.ctx.set_link_costs(None)                                          # no costs uploaded
    eng._costs = None
    assert fn(h, *args, dev) == -77
    assert b"costs" in L.sdnr_last_error()
    with _native.Context(0) as fresh:                                     # no graph uploaded
        assert fn(fresh._h, *args, dev) == -77
    eng.ctx.synchronize()
    assert not load.cpu().numpy().any()


# ------------------------------------------------------------------- k = 48 --

def core_tier_costs(csr, k, cost=2):
    """fat_tree(k): every link of the first core group (the cores of
    aggregation position 0), both directions, at ``cost``; 1 elsewhere."""
    h = k // 2
    esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    return np.where((esrc < h) | (np.asarray(csr.col) < h), cost, 1).astype(np.uint32)


@pytest.fixture(scope="module")
def k48(eng):
    fabric = T.fat_tree(48)
    csr = fabric.csr()
    hv = fabric.host_table()[0]
    hc = np.bincount(hv, minlength=csr.V).astype(np.int64)
    srcs = np.nonzero(hc)[0]
    assert srcs.shape[0] == 1152
    return csr, on(csr), hc, srcs


PICK = np.array([0, 1, 23, 24, 500, 777, 1150, 1151])


def test_k48_eight_rows_every_host_bearing_source_one_core_tier_at_cost_2(eng, k48):
    csr, ex, hc, srcs = k48
    cost = core_tier_costs(csr, 48)
    pc, _, _ = eng.cost_tables(ex, cost, srcs[PICK])
    n = srcs.shape[0]
    rows = np.repeat(np.arange(PICK.shape[0]), n)
    s = np.tile(srcs, PICK.shape[0])
    w = (hc[s] * hc[srcs[PICK][rows]]).astype(np.uint64)
    hp = pc.cpu().numpy()
    for split in SPLITS:
        want = EN.cost_ecmp_link_loads_host(csr, cost, hp, rows, s, w, split)
        got = eng.cost_ecmp_link_loads(ex, cost, pc, rows, s, w, split, timing=True)
        assert close(got, want) and want.any(), split
        assert eng.ctx.last_kernel() == LDS and eng.ctx.last_launches() == 1
        assert eng.ctx.last_kernel_ms() > 0
        # the costed cores carry nothing between pods: their uplinks stay idle
        esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
        assert not got[esrc < 24].any()


def test_k48_unit_costs_equal_the_hop_count_kernel(eng, k48):
    csr, ex, hc, srcs = k48
    ones = np.ones(int(csr.E), np.uint32)
    pc, _, _ = eng.cost_tables(ex, ones, srcs[PICK])
    dist, _, _ = eng.shortest_tables(ex, srcs[PICK])
    n = srcs.shape[0]
    rows = np.repeat(np.arange(PICK.shape[0]), n)
    s = np.tile(srcs, PICK.shape[0])
    w = (hc[s] * hc[srcs[PICK][rows]]).astype(np.uint64)
    for split in SPLITS:
        want = eng.ecmp_link_loads(ex, dist, rows, s, w, split)
        got = eng.cost_ecmp_link_loads(ex, ones, pc, rows, s, w, split)
        assert close(got, want) and want.any(), split


def test_k48_all_rows_pay_their_least_cost(eng, k48):
    """All 1,152 rows of the all-host-pairs demand with one core tier at cost
    2: whatever the split, a pair pays pcost(s, d) over the links it loads, so
    sum(load x cost) is the sum of w x pcost (in integers from the rows), and
    every link on some least-cost route is loaded."""
    csr, ex, hc, srcs = k48
    cost = core_tier_costs(csr, 48)
    pc, _, _ = eng.cost_tables(ex, cost, srcs)
    n = srcs.shape[0]
    rows = np.repeat(np.arange(n), n)
    s = np.tile(srcs, n)
    w = (hc[s] * hc[srcs[rows]]).astype(np.uint64)
    hp = pc.cpu().numpy().view(np.uint32)
    assert hp.max() < EN.COST_INF
    total = paid(hp, rows, s, w)
    # links on a least-cost route between two edge switches: none touches a costed core
    esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    used = (esrc >= 24) & (np.asarray(csr.col) >= 24)
    for split in SPLITS:
        got = eng.cost_ecmp_link_loads(ex, cost, pc, rows, s, w, split)
        assert np.isfinite(got).all() and (got >= 0).all()
        assert abs(float((got * cost).sum()) - total) <= RTOL * total, split
        assert got[used].min() > 0 and not got[~used].any()


# ------------------------------------------------------------- the drop-in --

@pytest.mark.parametrize("name", G.MULTI)
def test_dropin_equals_the_enumerated_least_cost_route_sets(name):
    from sdnmpi_amd.util.topology_db import SplitLinkLoads, TopologyDB
    g = G.Golden(name)
    fabric = g.fabric()
    db = fabric.populate(TopologyDB())
    rng = np.random.default_rng(16)
    links = [(u, v) for u in sorted(db.links) for v in sorted(db.links[u])]
    some = [links[i] for i in rng.choice(len(links), max(1, len(links) // 4), replace=False)]
    db.set_link_costs({k: int(c) for k, c in zip(some, rng.integers(2, 4, len(some)))})
    pairs = golden_pairs(g, fabric)
    sets = db.find_routes_least_cost(pairs, multiple=True)
    assert [r[0] if r else [] for r in sets] == db.find_routes_least_cost(pairs)
    got = db.least_cost_ecmp_link_loads(pairs)
    assert isinstance(got, SplitLinkLoads)
    assert dicts_close(got.as_dict(), route_set_loads(sets, [1] * len(pairs)))
    w = rng.integers(0, 1 << 32, len(pairs)).tolist()
    assert dicts_close(db.least_cost_ecmp_link_loads(pairs, w).as_dict(),
                       route_set_loads(sets, w))
    macs = fabric.host_macs()
    allp = [(a, b) for a in macs for b in macs if a != b]
    for split in SPLITS:
        assert dicts_close(db.all_pairs_least_cost_ecmp_link_loads(split).as_dict(),
                           db.least_cost_ecmp_link_loads(allp, split=split).as_dict())
    ranks = {r: m for r, m in enumerate(macs[:5])}
    assert dicts_close(
        db.mpi_least_cost_ecmp_link_loads(ranks).as_dict(),
        db.least_cost_ecmp_link_loads([(ranks[i], ranks[j]) for i in ranks for j in ranks
                                       if i != j]).as_dict())
