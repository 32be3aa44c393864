"""ecmp_fair_rates.hip (sdnr_ecmp_fair_rates) on the GPU against
engine.ecmp_fair_rates_host, and the drop-in's multipath fair_rates against the
engine double of test_ecmp_fair_rates.py.  The adds into the link counts arrive
in any order: rates, levels and carried rates agree within the CPU tests' TOL,
rounds, round and bottleneck are equal, and where every partial sum is exact
the comparison is on the bits."""
import types

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from test_cost_ecmp_loads import (both_ways, chord_ladder_csr, diamond_csr, digraph_csr,
                                  edge_costs, pcost_rows)
from test_ecmp_fair_rates import (ECMP_ROUTES, SPLITS, TOL, costed_db, seed_costs,
                                  small_case)
from test_ecmp_link_loads import edge_map
from test_fair_rates import CAPS, dropin_pairs

pytestmark = pytest.mark.gpu

LDS, GLOBAL = "ecmp_fair_rows_kernel<lds>", "ecmp_fair_rows_kernel<global>"
INF = EN.COST_INF


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def on(csr):
    """The export-shaped handle RouteEngine wants for a bare CSR."""
    return types.SimpleNamespace(csr=csr)


def close(got, want, bits=False):
    """rate, bott, round, level, used: equal rounds, round and bott; the
    doubles within TOL, or bit for bit."""
    for g, w, name in zip(got, want, ("rate", "bott", "round", "level", "used")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if g.dtype != np.float64:
            assert np.array_equal(g, w), name
        elif bits:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), name
        else:
            assert np.allclose(g, w, rtol=TOL, atol=0), name


def both(eng, csr, cost, pcost, rows, srcs, mult, cap, extra=None, split="route", kernel=LDS,
         bits=False):
    """One case on the device and in numpy; the results must agree."""
    want = EN.ecmp_fair_rates_host(csr, cost, pcost, rows, srcs, mult, cap, extra, split)
    got = eng.ecmp_fair_rates(on(csr), cost, np.asarray(pcost), rows, srcs, mult, cap, extra,
                              split)
    close(got, want, bits)
    assert eng.ctx.last_kernel() == kernel
    # one launch to start, two per round; rounds are queued 16 at a time, up
    # to the closing round after max_rounds = min(flows, E + nextra)
    rounds, most = len(want[3]), min(len(rows), len(cap))
    assert eng.ctx.last_launches() == 1 + 2 * min(16 * (rounds // 16 + 1), most + 1)
    return want


# ------------------------------------------------------ the small fabrics --

@pytest.mark.parametrize("k", [4, 8])
def test_fat_tree_between_edge_switches_bit_for_bit(eng, k):
    """Edge to edge on a fat-tree every fraction is a power of two; with integer
    multiplicities and capacities every partial sum is exact."""
    fabric = T.fat_tree(k)
    csr = fabric.csr()
    hv, _ = fabric.host_table()
    edges = np.unique(hv)
    n = edges.shape[0]
    pc = pcost_rows(csr, np.ones(int(csr.E), np.uint32), edges)
    rows, srcs = np.repeat(np.arange(n), n), np.tile(edges, n)
    rng = np.random.default_rng(40 + k)
    mult = rng.integers(0, 6, n * n).astype(np.uint64)
    cap = rng.choice(np.asarray([1, 2, 4, 16, 64], np.float64), int(csr.E))
    for split in SPLITS:
        r = both(eng, csr, None, pc, rows, srcs, mult, cap, split=split, bits=True)
        assert len(r[3]) > 1
        both(eng, csr, None, pc, rows, srcs, None, np.ones(int(csr.E)), split=split, bits=True)


@pytest.mark.parametrize("name", G.SMALL)
def test_small_fabrics_every_row_both_splits_unit_and_random_costs(eng, name):
    c = small_case(name)
    for cost, pc in ((None, c["pc_unit"]), (c["cost"], c["pc_cost"])):
        for split in SPLITS:
            r = both(eng, c["csr"], cost, pc, c["rows"], c["srcs"], c["mult"], c["cap"],
                     split=split)
            assert len(r[3]) > 1


# ------------------------------------------------------------ closed forms --

def test_diamond_closed_forms(eng):
    csr, cost, (s, m, d) = diamond_csr()
    em = edge_map(csr)
    E = int(csr.E)
    pc = pcost_rows(csr, cost, [d, s])
    cap = np.full(E, 10.0)
    cap[em[(s, m)]] = 1.0
    cap2 = np.full(E, 10.0)
    cap2[em[(m, d)]] = 1.0
    for split in SPLITS:
        r = both(eng, csr, cost, pc, [0], [s], None, cap, split=split, bits=True)
        assert r[0].tolist() == [2.0] and r[1].tolist() == [em[(s, m)]]
        r = both(eng, csr, cost, pc, [0, 0], [s, m], None, cap, split=split, bits=True)
        assert r[0].tolist() == [2.0, 9.0] and r[2].tolist() == [0, 1]
        r = both(eng, csr, cost, pc, [0, 0], [s, m], [3, 2], cap2, split=split)
        assert r[1].tolist() == [em[(m, d)]] * 2
        # next hops at different hop depths, two rows, unsorted flows, extras
        capx = np.concatenate([np.asarray([3, 1, 2, 10, 40, 100], np.float64)[:E], [0.5, 7.0]])
        extra = [[-1, -1], [E, -1], [E + 1, E], [-1, -1], [E + 1, E + 1], [-1, -1]]
        r = both(eng, csr, cost, pc, [0, 1, 0, 1, 0, 0], [s, d, m, m, d, d], [2, 1, 1, 3, 1, 4],
                 capx, extra, split=split)
        assert r[0][5] == np.inf and r[1][1] == E and r[1][4] == E + 1


@pytest.mark.parametrize("n", [1, 4, 70])
def test_chord_ladder_thirds_and_route_counts_near_2_70(eng, n):
    """Thirds: inexact fractions.  n = 70: 3**70 routes from the first joint,
    sigma far past 2**64, and a longest next-hop chain of 140 links."""
    csr, cost = chord_ladder_csr(n)
    d = 3 * n
    pc = pcost_rows(csr, cost, [d])
    rows, srcs = [0] * (d + 1), list(range(d + 1))
    E = int(csr.E)
    for split in SPLITS:
        r = both(eng, csr, cost, pc, [0], [0], None, np.ones(E), split=split)
        assert np.allclose(r[0], [3.0], rtol=TOL, atol=0)
        both(eng, csr, cost, pc, rows, srcs, [1 + (v % 4) for v in srcs],
             np.asarray(CAPS, np.float64)[np.arange(E) % len(CAPS)], split=split)


def path_case(n):
    """A path of n vertices toward its last one, cap[v -> v + 1] = (v + 1)**2 and
    a flow from every vertex: link v -> v + 1 is the bottleneck of flow v alone."""
    csr = digraph_csr(both_ways([(v, v + 1) for v in range(n - 1)]))
    em = edge_map(csr)
    cap = np.ones(int(csr.E))
    for v in range(n - 1):
        cap[em[(v, v + 1)]] = float((v + 1) ** 2)
    pc = pcost_rows(csr, np.ones(int(csr.E), np.uint32), [n - 1])
    return csr, pc, cap, em


def test_path_of_40_one_flow_per_round_across_two_status_batches(eng):
    csr, pc, cap, em = path_case(40)
    r = both(eng, csr, None, pc, [0] * 40, list(range(40)), None, cap, bits=True)
    assert len(r[3]) == 39 and r[2][:39].tolist() == list(range(39)) and r[0][39] == np.inf
    assert r[1][:39].tolist() == [em[(v, v + 1)] for v in range(39)]
    assert r[0][:3].tolist() == [1.0, 3.0, 5.0]


# ------------------------------------------------------------ global form --

def padded_diamond(V):
    """The diamond with V - 3 leaves hung on m (links both ways, cost 1)."""
    s, m, d = 0, 1, 2
    und = [(s, d), (s, m), (m, d)] + [(m, v) for v in range(3, V)]
    csr = digraph_csr(both_ways(und), V)
    return csr, edge_costs(csr, {(s, d): 2, (d, s): 2}), (s, m, d)


def test_global_form_past_the_lds_threshold(eng):
    V = EN.ECMP_FAIR_LDS_MAX_V + 1
    csr, cost, (s, m, d) = padded_diamond(V)
    assert int(csr.V) == V
    dsts = [d, s, 5, V - 1]
    pc = pcost_rows(csr, cost, dsts)
    E = int(csr.E)
    em = edge_map(csr)
    cap = np.full(E, 10.0)
    cap[[em[(s, m)], em[(m, d)], em[(m, 5)]]] = [1.0, 3.0, 2.0]
    core_rows, core_srcs, core_mult = [0, 0, 1, 1], [s, m, d, m], [1, 2, 1, 1]
    for split in SPLITS:
        big = both(eng, csr, cost, pc, core_rows, core_srcs, core_mult, cap, split=split,
                   kernel=GLOBAL)
        # the same flows on the core alone, in the LDS form
        c3, cost3, _ = diamond_csr()
        em3 = edge_map(c3)
        cap3 = np.full(int(c3.E), 10.0)
        cap3[[em3[(s, m)], em3[(m, d)]]] = [1.0, 3.0]
        small = both(eng, c3, cost3, pcost_rows(c3, cost3, [d, s]), core_rows, core_srcs,
                     core_mult, cap3, split=split, kernel=LDS)
        assert np.array_equal(big[0], small[0]) and np.array_equal(big[2], small[2])
        # leaves as sources and destinations, every row, out-of-range and absent flows
        rows = [0, 0, 1, 2, 2, 3, 3, 0, 2, 3, 0]
        srcs = [s, 7, V - 1, s, 6, 5, d, V, 5, -1, 9]
        mult = [1, 3, 2, 1, 1, 4, 1, 1, 1, 1, 0]
        r = both(eng, csr, cost, pc, rows, srcs, mult, cap, split=split, kernel=GLOBAL)
        assert r[0][8] == np.inf and not r[0][[7, 9, 10]].any() and len(r[3]) > 2


# ---------------------------------------------------------------- odd input --

def raw(eng, csr, cost, pcost, nrows, off, srcs, cap, mult=None, extra=None, max_rounds=None,
        hop=False):
    """One sdnr_ecmp_fair_rates call on device copies; returns (rounds, outputs,
    inputs), without synchronize."""
    import torch
    ex = on(csr)
    eng.load(ex)
    if cost is None:
        eng._costs = None
        eng.ctx.set_link_costs(None)
    else:
        eng.set_link_costs(ex, cost)
    n = len(srcs)
    nx = len(cap) - csr.E
    mr = min(n, len(cap)) if max_rounds is None else max_rounds
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(eng.dev)  # noqa
    keep = [t(np.asarray(pcost, np.uint32).view(np.int32), np.int32), t(off, np.int64),
            t(srcs, np.int32), t(cap, np.float64),
            t(np.asarray(mult, np.uint64).view(np.int64), np.int64) if mult is not None else None,
            t(extra, np.int32) if extra is not None else None]
    out = [torch.full((n,), 7.0, dtype=torch.float64, device=eng.dev),
           torch.full((n,), 7, dtype=torch.int32, device=eng.dev),
           torch.full((n,), 7, dtype=torch.int32, device=eng.dev),
           torch.full((max(mr, 1),), 7.0, dtype=torch.float64, device=eng.dev),
           torch.full((len(cap),), 7.0, dtype=torch.float64, device=eng.dev)]
    torch.cuda.synchronize()
    p = lambda x: x.data_ptr() if x is not None else 0    # noqa: E731
    rounds = eng.ctx.ecmp_fair_rates_device(p(keep[0]), nrows, p(keep[1]), p(keep[2]), p(keep[4]),
                                            p(keep[5]), p(keep[3]), nx, p(out[0]), p(out[1]),
                                            p(out[2]), p(out[3]), mr, p(out[4]), hop=hop)
    return rounds, out, keep


def test_no_rows_and_no_pairs(eng):
    csr, cost, (s, m, d) = diamond_csr()
    eng.load(on(csr))
    assert eng.ctx.ecmp_fair_rates_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == 0
    pc = pcost_rows(csr, cost, [d])
    rounds, out, keep = raw(eng, csr, cost, pc, 1, [2, 2], [0, 0, 0], np.ones(csr.E))
    eng.ctx.synchronize()
    assert rounds == 0 and all(float(o.cpu()[0]) == 7 for o in out)       # nothing touched
    r = eng.ecmp_fair_rates(on(csr), cost, pc, [], [], None, np.ones(csr.E))
    assert [len(x) for x in r] == [0, 0, 0, 0, csr.E]
    del keep


def test_a_row_that_is_no_labelling_is_reported_and_the_others_stand(eng):
    """Row 1 gives m a cost that no link explains: synchronize reports it once as
    SDNR_ERR_INVAL, its flows read 0.0 / -1 / -1, rows 0 and 2 are what they
    are alone."""
    csr, cost, (s, m, d) = diamond_csr()
    good = pcost_rows(csr, cost, [d, s])
    pc = np.vstack([good[:1], good[:1], good[1:]])
    pc[1, m] = 7
    cap = np.arange(1, csr.E + 1, dtype=np.float64)
    srcs = [s, m, s, m, d, m]
    rounds, out, keep = raw(eng, csr, cost, pc, 3, [0, 2, 4, 6], srcs, cap)
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "sdnr_ecmp_fair_rates" in str(ei.value)
    eng.ctx.synchronize()                                  # reported once
    rate, bott, rnd = (o.cpu().numpy() for o in out[:3])
    ok = [0, 1, 4, 5]
    want = EN.ecmp_fair_rates_host(csr, cost, good, [0, 0, 1, 1], np.asarray(srcs)[ok], None, cap)
    assert rounds == len(want[3]) > 0
    assert np.allclose(rate[ok], want[0], rtol=TOL, atol=0)
    assert np.array_equal(bott[ok], want[1]) and np.array_equal(rnd[ok], want[2])
    assert np.allclose(out[4].cpu().numpy(), want[4], rtol=TOL, atol=0)
    assert np.allclose(out[3].cpu().numpy()[:rounds], want[3], rtol=TOL, atol=0)
    assert not rate[[2, 3]].any() and (bott[[2, 3]] == -1).all() and (rnd[[2, 3]] == -1).all()
    # the context goes on working
    r = eng.ecmp_fair_rates(on(csr), cost, good, [0], [m], None, cap)
    assert r[0].tolist() == [cap[edge_map(csr)[(m, d)]]]
    del keep


def test_max_rounds_too_small_leaves_round_minus_2(eng):
    csr, pc, cap, em = path_case(8)
    rounds, out, keep = raw(eng, csr, None, pc, 1, [0, 8], list(range(8)), cap, max_rounds=3)
    eng.ctx.synchronize()
    rate, bott, rnd = (o.cpu().numpy() for o in out[:3])
    assert rounds == 3 and rnd.tolist() == [0, 1, 2, -2, -2, -2, -2, -1]
    assert rate.tolist() == [1.0, 3.0, 5.0, 0.0, 0.0, 0.0, 0.0, np.inf]
    assert bott[3:].tolist() == [-1] * 5 and out[3].cpu().numpy().tolist() == [1.0, 3.0, 5.0]
    del keep


@pytest.mark.parametrize("bad", [0.0, -2.0, float("nan"), float("inf")])
def test_bad_capacities_are_rejected(eng, bad):
    csr, cost, (s, m, d) = diamond_csr()
    pc = pcost_rows(csr, cost, [d])
    cap = np.ones(csr.E)
    cap[edge_map(csr)[(m, d)]] = bad
    with pytest.raises(ValueError):
        eng.ecmp_fair_rates(on(csr), cost, pc, [0], [s], None, cap)
    rounds, out, keep = raw(eng, csr, cost, pc, 1, [0, 2], [s, m], cap)
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "capacity" in str(ei.value)
    eng.ctx.synchronize()
    del keep


def test_argument_errors(eng):
    import ctypes
    import torch
    csr, cost, _ = diamond_csr()
    eng.load(on(csr))
    L, h = eng.ctx._lib, eng.ctx._h
    buf = torch.zeros(64, dtype=torch.int64, device=eng.dev)
    p = ctypes.c_void_p(buf.data_ptr())
    n = ctypes.c_int32(9)
    dev = _native.DEVICE_PTRS
    tail = (p, p, p, p, 2, p, ctypes.byref(n))

    def call(pcost, nrows, flags, nextra=0):
        return L.sdnr_ecmp_fair_rates(h, pcost, nrows, p, p, None, None, p, nextra, *tail, flags)

    assert call(p, 1, 0) == -22 and n.value == 0                          # host pointers
    assert call(None, 1, dev) == -22
    assert call(p, -1, dev) == -22
    assert call(p, 1, dev, -1) == -22
    buf[0] = 5                                                            # pair_off[0] > pair_off[1]
    torch.cuda.synchronize()
    assert call(p, 1, dev) == -22 and b"monotone" in L.sdnr_last_error()
    with _native.Context(0) as fresh:                                     # no graph uploaded
        assert L.sdnr_ecmp_fair_rates(fresh._h, p, 1, p, p, None, None, p, 0, *tail, dev) == -77
    with pytest.raises(ValueError, match="split"):
        eng.ecmp_fair_rates(on(csr), cost, np.zeros((1, 3), np.uint32), [0], [0], split="flow")
    with pytest.raises(ValueError, match="row"):
        eng.ecmp_fair_rates(on(csr), cost, np.zeros((1, 3), np.uint32), [1], [0])


# ---------------------------------------------------------------- drop-in --

def test_dropin_fat_tree_both_routes_both_splits_and_host_ports():
    from sdnmpi_amd.util.topology_db import TopologyDB
    fabric = T.fat_tree(4)
    double, capacity = costed_db(fabric)
    db = fabric.populate(TopologyDB())
    assert seed_costs(db) == capacity
    pairs, w = dropin_pairs(fabric)
    for route in ECMP_ROUTES:
        for split in SPLITS:
            for hc in (None, 2.5):
                a = db.fair_rates(pairs, w, capacity, hc, route, split)
                b = double.fair_rates(pairs, w, capacity, hc, route, split)
                assert np.allclose(a.rate, b.rate, rtol=TOL, atol=0), (route, split, hc)
                assert a.bottleneck == b.bottleneck and np.array_equal(a.round, b.round)
                assert np.array_equal(a.routed, b.routed)
                assert a.rounds == b.rounds > 1
                assert np.allclose(a.levels, b.levels, rtol=TOL, atol=0)
                assert np.allclose(a.link_rate.load, b.link_rate.load, rtol=TOL, atol=0)
                assert a.saturated_links() == b.saturated_links()
            ap = db.all_pairs_fair_rates(capacity, route, split)
            bp = double.all_pairs_fair_rates(capacity, route, split)
            assert np.allclose(ap.rate, bp.rate, rtol=TOL, atol=0)
            assert ap.bottleneck == bp.bottleneck
    ranks = dict(enumerate(fabric.host_macs()[::2]))
    traffic = {(i, (i + 3) % len(ranks)): 1000 * (i + 1) for i in ranks}
    a = db.mpi_fair_rates(ranks, traffic, capacity, 2.5, "least_cost_ecmp", "hop")
    b = double.mpi_fair_rates(ranks, traffic, capacity, 2.5, "least_cost_ecmp", "hop")
    assert np.allclose(a.time, b.time, rtol=TOL, atol=0) and a.step_time() == \
        pytest.approx(b.step_time(), rel=TOL)
