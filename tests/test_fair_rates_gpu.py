"""fair_rates.hip (sdnr_fair_rates) on the GPU against engine.fair_rates_host,
and the drop-in's fair_rates against the engine double of test_fair_rates.py.
The definition is deterministic: every comparison is on the bits of the rates,
the levels and the carried rates, and on equal rounds and bottlenecks."""
import types

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from test_ecmp_link_loads import edge_map
from test_fair_rates import (CAPS, ROUTES, dropin_pairs, fake_db, layout_tree, line_csr,
                             line_to_end, small_case)

pytestmark = pytest.mark.gpu

LAYOUTS = (EN.INT32, EN.PORT16, EN.SLOT)
LDS, GLOBAL = "fair_rows_kernel<lds>", "fair_rows_kernel<global>"


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


def same(got, want):
    """rate, bott, round, level, used: equal bit for bit."""
    for g, w, name in zip(got, want, ("rate", "bott", "round", "level", "used")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if g.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), name
        else:
            assert np.array_equal(g, w), name


def both(eng, csr, tree, layout, rows, verts, mult, cap, extra=None, to_root=False, kernel=LDS):
    """One case on the device and in numpy; the results must be the same."""
    want = EN.fair_rates_host(csr, tree, layout, rows, verts, mult, cap, extra, to_root)
    got = eng.fair_rates(on(csr), dev_tree(eng, tree), layout, rows, verts, mult, cap, extra,
                         to_root=to_root)
    same(got, want)
    assert eng.ctx.last_kernel() == kernel
    # one launch to start, two per round; rounds are queued 16 at a time, up
    # to the closing round after max_rounds = min(flows, E + nextra)
    rounds, most = len(want[3]), min(len(rows), len(cap))
    assert eng.ctx.last_launches() == 1 + 2 * min(16 * (rounds // 16 + 1), most + 1)
    return want


# ------------------------------------------------------ the small fabrics --

@pytest.mark.parametrize("name", G.SMALL)
def test_small_fabrics_every_row_all_layouts_and_to_root(eng, name):
    c = small_case(name)
    csr, rows, verts, mult, cap = c["csr"], c["rows"], c["verts"], c["mult"], c["cap"]
    ex = on(csr)
    want = EN.fair_rates_host(csr, c["par"], EN.INT32, rows, verts, mult, cap)
    assert len(want[3]) > 1
    for lay in LAYOUTS:
        if lay == EN.SLOT and np.diff(csr.row_ptr).max() > 62:
            continue
        got = eng.fair_rates(ex, dev_tree(eng, layout_tree(c, lay)), lay, rows, verts, mult, cap)
        same(got, want)
        assert eng.ctx.last_kernel() == LDS
    both(eng, csr, c["nh"], EN.INT32, rows, verts, mult, cap, to_root=True)
    both(eng, csr, c["nh"], EN.INT32, rows, verts, None, cap, to_root=True)


# ------------------------------------------------------------ closed forms --

def test_one_link_and_three_flow_line(eng):
    csr = line_csr(1)
    nh, fwd = line_to_end(csr)
    cap = np.full(csr.E, 7.0)
    cap[fwd[0]] = 3.0
    r = both(eng, csr, nh, EN.INT32, [0, 0], [0, 0], None, cap, to_root=True)
    assert r[0].tolist() == [1.5, 1.5] and r[3].tolist() == [1.5]
    csr = line_csr(2)
    em = edge_map(csr)
    cap = np.ones(csr.E)
    cap[em[(1, 2)]] = 2.0
    nh = np.array([[1, 2, -1], [1, -1, 1]], np.int32)
    r = both(eng, csr, nh, EN.INT32, [0, 1, 0], [0, 0, 1], None, cap, to_root=True)
    assert r[0].tolist() == [0.5, 0.5, 1.5] and r[2].tolist() == [0, 0, 1]
    # the tie: both unit links fill at 1/2; the long flow's bottleneck is the
    # link nearer its vertex, in either direction of the rows
    cap[:] = 1.0
    r = both(eng, csr, nh, EN.INT32, [0, 1, 0], [0, 0, 1], None, cap, to_root=True)
    assert r[1].tolist() == [em[(0, 1)], em[(0, 1)], em[(1, 2)]]
    par = np.array([[0, 0, 1], [1, 1, 1]], np.int32)
    r = both(eng, csr, par, EN.INT32, [0, 0, 1], [2, 1, 2], None, cap)
    assert r[1].tolist() == [em[(1, 2)], em[(0, 1)], em[(1, 2)]] and r[0].tolist() == [0.5] * 3


@pytest.mark.parametrize("V", [2, 3, 65, 130, 1030])
def test_path_graphs_one_flow_per_round(eng, V):
    """cap[v -> v + 1] = (v + 1)^2 and a flow from every vertex: flow v gets
    2v + 1 in round v.  65 and 130 vertices make the doubling cross the wave
    and the workgroup stride; 1,030 runs 1,029 rounds through the batches."""
    n = V - 1
    csr = line_csr(n)
    nh, fwd = line_to_end(csr)
    cap = np.ones(csr.E)
    cap[fwd] = (np.arange(n) + 1.0) ** 2
    r = both(eng, csr, nh, EN.INT32, np.zeros(V, np.int64), np.arange(V), None, cap, to_root=True)
    assert r[0][:n].tolist() == (2.0 * np.arange(n) + 1).tolist() and r[0][n] == np.inf
    assert r[2].tolist() == list(range(n)) + [-1] and len(r[3]) == n


def star_with_tail(V):
    """Hub 0 with leaves 4 .. V - 1 and the tail 0 - 1 - 2 - 3; the next-hop
    row toward vertex 3."""
    leaves = np.arange(4, V)
    und = [(0, 1), (1, 2), (2, 3)] + [(0, int(x)) for x in leaves]
    src = np.asarray([u for u, _ in und] + [v for _, v in und], np.int64) + 1
    dst = np.asarray([v for _, v in und] + [u for u, _ in und], np.int64) + 1
    csr = T.build_csr(src, dst, np.ones(src.shape[0], np.int64))
    nh = np.zeros((1, V), np.int32)
    nh[0, :4] = [1, 2, 3, -1]
    return csr, nh


@pytest.mark.parametrize("V,kernel", [(EN.FAIR_LDS_MAX_V, LDS), (EN.FAIR_LDS_MAX_V + 1, GLOBAL)])
def test_both_sides_of_the_lds_threshold(eng, V, kernel):
    """V = 6,800 is the last graph whose row state fits LDS (24 bytes per
    vertex); 6,801 takes the global-scratch form."""
    csr, nh = star_with_tail(V)
    assert csr.V == V
    rng = np.random.default_rng(V)
    verts = np.concatenate([np.arange(V), [1, 2, 5, 5]])
    mult = rng.integers(0, 4, verts.shape[0]).astype(np.uint64)
    cap = rng.choice(np.asarray(CAPS, np.float64), int(csr.E))
    em = edge_map(csr)
    cap[[em[(0, 1)], em[(1, 2)], em[(2, 3)]]] = [1e6, 3e4, 1e6]    # the tail fills last
    r = both(eng, csr, nh, EN.INT32, np.zeros(verts.shape[0], np.int64), verts, mult, cap,
             to_root=True, kernel=kernel)
    assert len(r[3]) > 8 and r[1][1] == em[(1, 2)]


def test_multiplicities_past_2_32_on_one_link(eng):
    csr = line_csr(2)
    nh, fwd = line_to_end(csr)
    cap = np.full(csr.E, 3.0 * (1 << 40))
    cap[fwd[1]] *= 2
    mult = np.array([(1 << 32) - 1, 1 << 33, 5, (1 << 52) - (1 << 34)], np.uint64)
    r = both(eng, csr, nh, EN.INT32, [0, 0, 0, 0], [0, 0, 1, 0], mult, cap, to_root=True)
    total = int(mult[[0, 1, 3]].astype(object).sum())
    assert total > 1 << 32 and r[3][0] == 3.0 * (1 << 40) / total and len(r[3]) == 2
    assert r[4][fwd[0]] == r[3][0] * total


# ------------------------------------------------------------------ extras --

def test_extras_before_with_after_and_alone(eng):
    csr = line_csr(2)
    em = edge_map(csr)
    E = csr.E
    nh = np.array([[1, 2, -1]], np.int32)
    for host, bott in ((1.0, E + 1), (10.0, em[(0, 1)]), (40.0, em[(0, 1)])):
        cap = np.concatenate([np.full(E, 10.0), [4.0, host, 6.0]])
        r = both(eng, csr, nh, EN.INT32, [0], [0], None, cap, [[E + 1, -1]], to_root=True)
        assert r[1].tolist() == [bott] and r[0].tolist() == [min(host, 10.0)]
        # more flows: at the root with and without extras, one extra twice
        extra = np.array([[E + 1, -1], [-1, -1], [E, E + 2], [-1, E + 2], [E + 2, E + 2]])
        r = both(eng, csr, nh, EN.INT32, [0] * 5, [0, 2, 2, 1, 1], None, cap, extra, to_root=True)
        assert r[0][1] == np.inf and r[1][1] == -1
        assert r[0][2:].tolist() == [2.0] * 3 and r[1][2:].tolist() == [E + 2] * 3
    # mult given, the second extra fills first
    cap = np.concatenate([np.full(E, 10.0), [5.0, 5.0, 2.0]])
    r = both(eng, csr, nh, EN.INT32, [0, 0], [2, 0], [3, 1], cap, [[E, E + 2], [E + 1, -1]],
             to_root=True)
    assert r[1].tolist() == [E + 2, E + 1] and r[0].tolist() == [2.0 / 3, 5.0]


# ---------------------------------------------------------------- odd input --

def test_unreached_out_of_range_gaps_and_repeats(eng):
    from oracle import oracle as O
    from test_link_loads import random_csr
    csr = random_csr(40, 30, 3)                            # the last fifth is unreachable
    ids = np.arange(csr.V, dtype=np.int32)
    par, prt, _ = O.dfs_tables(csr, ids)
    assert (par[0] < 0).any()
    rows = np.array([5, 0, 0, 0, 0, 0, 2, 2, 5, 5, 0])    # rows 1, 3, 4 have no flows; unsorted
    verts = np.array([6, 7, 7, 7, 39, -3, 40, 11, 1 << 20, 6, 0])
    mult = np.array([2, 1, 10, 100, 5, 5, 5, 1 << 40, 9, 0, 3], np.uint64)
    cap = np.random.default_rng(4).choice(np.asarray(CAPS, np.float64), int(csr.E))
    for lay in LAYOUTS:
        tree = par if lay == EN.INT32 else EN.pack_host_tree(par, prt, csr, lay)
        r = both(eng, csr, tree, lay, rows, verts, mult, cap)
        assert r[0][[4, 5, 6, 8, 9]].tolist() == [0.0] * 5 and r[0][10] == np.inf
        assert (r[0][[0, 1, 2, 3, 7]] > 0).all() and (r[2][[0, 1, 2, 3, 7]] >= 0).all()


def raw(eng, csr, tree, nrows, off, verts, cap, mult=None, extra=None, max_rounds=None,
        to_root=True):
    """One sdnr_fair_rates call on device copies; returns (rounds, rate, bott,
    round, level, used) as numpy, without synchronize."""
    import torch
    eng.load(on(csr))
    n = len(verts)
    nx = len(cap) - csr.E
    mr = min(n, len(cap)) if max_rounds is None else max_rounds
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(eng.dev)  # noqa
    keep = [dev_tree(eng, tree), t(off, np.int64), t(verts, np.int32), t(cap, np.float64),
            t(np.asarray(mult, np.uint64).view(np.int64), np.int64) if mult is not None else None,
            t(extra, np.int32) if extra is not None else None]
    out = [torch.full((n,), 7.0, dtype=torch.float64, device=eng.dev),
           torch.full((n,), 7, dtype=torch.int32, device=eng.dev),
           torch.full((n,), 7, dtype=torch.int32, device=eng.dev),
           torch.full((max(mr, 1),), 7.0, dtype=torch.float64, device=eng.dev),
           torch.full((len(cap),), 7.0, dtype=torch.float64, device=eng.dev)]
    torch.cuda.synchronize()
    p = lambda x: x.data_ptr() if x is not None else 0    # noqa: E731
    rounds = eng.ctx.fair_rates_device(p(keep[0]), _native.TREE_INT32, nrows, p(keep[1]),
                                       p(keep[2]), p(keep[4]), p(keep[5]), p(keep[3]), nx,
                                       p(out[0]), p(out[1]), p(out[2]), p(out[3]), mr, p(out[4]),
                                       to_root=to_root)
    return rounds, out, keep


def test_no_rows_and_no_pairs(eng):
    csr = line_csr(2)
    eng.load(on(csr))
    assert eng.ctx.fair_rates_device(0, _native.TREE_INT32, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                     0) == 0
    nh = np.array([[1, 2, -1]], np.int32)
    rounds, out, keep = raw(eng, csr, nh, 1, [2, 2], [0, 0, 0], np.ones(csr.E))
    eng.ctx.synchronize()
    assert rounds == 0 and all(float(o.cpu()[0]) == 7 for o in out)       # nothing touched
    r = eng.fair_rates(on(csr), dev_tree(eng, nh), EN.INT32, [], [], None, np.ones(csr.E),
                       to_root=True)
    assert [len(x) for x in r] == [0, 0, 0, 0, csr.E]
    del keep


def test_cycle_row_and_bad_offsets_are_reported_not_followed(eng):
    """Row 1 holds a 2-cycle, row 2's offsets leave the pair list: both are
    reported once by synchronize as SDNR_ERR_INVAL, their flows read 0.0 /
    -1 / -1, the doubling is bounded, and rows 0 and 3 are what they are
    alone."""
    csr = line_csr(3)
    nh = np.array([[1, 2, 3, -1], [1, 0, 3, -1], [1, 2, 3, -1], [-1, 0, 1, 2]], np.int32)
    cap = np.arange(1, csr.E + 1, dtype=np.float64)
    verts = [0, 1, 2, 0, 1, 2, 1, 3, 2]
    off = [0, 3, 5, 100, 6, 9]                  # row 2 = [5, 100), row 3 = [100, 6): both bad
    rounds, out, keep = raw(eng, csr, np.concatenate([nh, nh[3:]]), 5, off, verts, cap)
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "sdnr_fair_rates" in str(ei.value)
    eng.ctx.synchronize()                                  # reported once
    rate, bott, rnd = (o.cpu().numpy() for o in out[:3])
    good = [0, 1, 2, 6, 7, 8]
    want = EN.fair_rates_host(csr, nh, EN.INT32, [0, 0, 0, 3, 3, 3], np.asarray(verts)[good], None,
                              cap, to_root=True)
    assert rounds == len(want[3]) > 0
    assert np.array_equal(rate[good].view(np.uint64), want[0].view(np.uint64))
    assert np.array_equal(bott[good], want[1]) and np.array_equal(rnd[good], want[2])
    assert np.array_equal(out[4].cpu().numpy().view(np.uint64), want[4].view(np.uint64))
    assert np.array_equal(out[3].cpu().numpy()[:rounds].view(np.uint64), want[3].view(np.uint64))
    assert not rate[[3, 4, 5]].any() and (bott[[3, 4, 5]] == -1).all() and \
        (rnd[[3, 4, 5]] == -1).all()
    # the context goes on working
    r = eng.fair_rates(on(csr), dev_tree(eng, nh[:1]), EN.INT32, [0], [0], None, cap, to_root=True)
    assert r[0].tolist() == [cap[edge_map(csr)[(0, 1)]]]
    del keep


@pytest.mark.parametrize("bad", [0.0, -2.0, float("nan"), float("inf")])
def test_bad_capacities_are_rejected(eng, bad):
    csr = line_csr(2)
    nh = np.array([[1, 2, -1]], np.int32)
    cap = np.ones(csr.E)
    cap[edge_map(csr)[(1, 2)]] = bad
    with pytest.raises(ValueError):
        eng.fair_rates(on(csr), dev_tree(eng, nh), EN.INT32, [0], [0], None, cap, to_root=True)
    rounds, out, keep = raw(eng, csr, nh, 1, [0, 2], [0, 1], cap)
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "capacity" in str(ei.value)
    eng.ctx.synchronize()
    del keep


def test_argument_errors(eng):
    import ctypes
    import torch
    csr = line_csr(2)
    eng.load(on(csr))
    L, h = eng.ctx._lib, eng.ctx._h
    buf = torch.zeros(64, dtype=torch.int64, device=eng.dev)
    p = ctypes.c_void_p(buf.data_ptr())
    n = ctypes.c_int32(9)
    dev = _native.DEVICE_PTRS
    tail = (p, p, p, p, 2, p, ctypes.byref(n))

    def call(tree, layout, nrows, flags, nextra=0):
        return L.sdnr_fair_rates(h, tree, layout, nrows, p, p, None, None, p, nextra, *tail, flags)

    assert call(p, 0, 1, 0) == -22 and n.value == 0                       # host pointers
    assert call(p, 7, 1, dev) == -22
    assert call(p, _native.TREE_SLOT, 1, dev | _native.LOADS_TO_ROOT) == -22
    assert call(None, 0, 1, dev) == -22
    assert call(p, 0, -1, dev) == -22
    assert call(p, 0, 1, dev, -1) == -22
    buf[0] = 5                                                            # pair_off[0] > pair_off[1]
    torch.cuda.synchronize()
    assert call(p, 0, 1, dev) == -22 and b"monotone" in L.sdnr_last_error()
    with _native.Context(0) as fresh:                                     # no graph uploaded
        assert L.sdnr_fair_rates(fresh._h, p, 0, 1, p, p, None, None, p, 0, *tail, dev) == -77


# ------------------------------------------------------------------- k = 48 --

def test_k48_two_pods_of_destinations_all_edge_sources(eng):
    """The 48 destination rows of pods 0 and 1 on their shortest routes, all
    1,152 edge switches as sources with 576 host pairs each, unit links."""
    fabric = T.fat_tree(48)
    csr = fabric.csr()
    ex = on(csr)
    hv, _ = fabric.host_table()
    edges = np.unique(hv)
    assert edges.shape[0] == 1152
    dsts = edges[:48].astype(np.int32)
    _, nh, _ = eng.shortest_tables(ex, dsts)
    rows = np.repeat(np.arange(48), 1152)
    verts = np.tile(edges, 48)
    mult = np.full(rows.shape[0], 576, np.uint64)
    cap = np.ones(int(csr.E))
    got = eng.fair_rates(ex, nh, EN.INT32, rows, verts, mult, cap, to_root=True, timing=True)
    assert eng.ctx.last_kernel() == LDS and eng.ctx.last_kernel_ms() > 0
    want = EN.fair_rates_host(csr, nh.cpu().numpy(), EN.INT32, rows, verts, mult, cap,
                              to_root=True)
    same(got, want)
    assert len(want[3]) >= 2 and np.isinf(got[0]).sum() == 48


# ---------------------------------------------------------------- drop-in --

def test_dropin_fat_tree_k8_all_routes_and_host_ports():
    from sdnmpi_amd.util.topology_db import TopologyDB
    fabric = T.fat_tree(8)
    db = fabric.populate(TopologyDB())
    double = fake_db(fabric)
    csr = db.graph().csr
    rng = np.random.default_rng(31)
    links = [(int(csr.dpids[u]), int(csr.dpids[v])) for u, v in
             zip(np.repeat(np.arange(csr.V), np.diff(csr.row_ptr)).tolist(),
                 np.asarray(csr.col).tolist())]
    for lk in links:
        c, u = int(rng.integers(1, 4)), int(rng.integers(0, 4))
        for x in (db, double):
            x.set_link_cost(lk[0], lk[1], c)
            x.set_link_utilisation(lk[0], lk[1], u)
    capacity = {lk: int(c) for lk, c in zip(links, rng.choice(CAPS, len(links)))}
    pairs, w = dropin_pairs(fabric)
    for route in ROUTES:
        for hc in (None, 2.5):
            a = db.fair_rates(pairs, w, capacity, hc, route)
            b = double.fair_rates(pairs, w, capacity, hc, route)
            assert np.array_equal(a.rate.view(np.uint64), b.rate.view(np.uint64)), (route, hc)
            assert a.bottleneck == b.bottleneck and np.array_equal(a.round, b.round)
            assert np.array_equal(a.routed, b.routed) and np.array_equal(a.levels, b.levels)
            assert np.array_equal(a.link_rate.load, b.link_rate.load)
            assert a.link_rate.as_dict() == b.link_rate.as_dict()
            assert a.rounds > 1 and a.saturated_links() == b.saturated_links()
        ap, bp = db.all_pairs_fair_rates(capacity, route), double.all_pairs_fair_rates(capacity,
                                                                                        route)
        assert np.array_equal(ap.rate, bp.rate) and ap.bottleneck == bp.bottleneck
    ranks = dict(enumerate(fabric.host_macs()[::4]))
    traffic = {(i, (i + 5) % len(ranks)): 1000 * (i + 1) for i in ranks}
    a = db.mpi_fair_rates(ranks, traffic, capacity, 2.5)
    b = double.mpi_fair_rates(ranks, traffic, capacity, 2.5)
    assert np.array_equal(a.time, b.time) and a.step_time() == b.step_time() > 0
