"""whatif_loads.hip (sdnr_whatif_ecmp_link_loads) on the GPU against
engine.whatif_ecmp_link_loads_host -- which builds the changed cost vector and
really removes the links that are down --, against its sister kernels where a
scenario is one they can answer, and the drop-in's cost_change_link_loads and
tune_link_costs against a second TopologyDB on which the changes were made.

Tolerance (see test_ecmp_link_loads.py): rtol = 1e-9, atol = 0 where the
expected value is nonzero, exactly 0.0 where it is 0 -- a link that is down
among them.  The dyadic cases are compared bit for bit.  ``routed`` and
``lost`` are compared exactly.  ``peak`` / ``peak_edge`` are compared bit for
bit with the reduction of the GPU's own loads, and with the host's within rtol
(the edge: one whose host utilisation is within rtol of the host's peak)."""
import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from test_cost_ecmp_loads import both_ways, digraph_csr, random_costs
from test_cost_ecmp_loads_gpu import core_tier_costs
from test_ecmp_link_loads import SPLITS, close, edge_map
from test_ecmp_link_loads_gpu import zeros_f64
from test_failure_loads import cable_edges, small_case, switch_edges, trap_case
from test_failure_loads_gpu import grouped
from test_link_loads import random_csr
from test_link_loads_gpu import on
from test_whatif_loads import (check_dropin, check_fish, cost_scenarios, lowered_ring_case,
                               raised_chord_case)

pytestmark = pytest.mark.gpu

LDS, GLOBAL = "whatif_ecmp_loads_kernel<lds>", "whatif_ecmp_loads_kernel<global>"
INF = EN.COST_INF


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def peaks_ok(load, peak, pe, want, cap):
    """peak / peak_edge [nscen] against the reduction of ``load`` (the GPU's
    own planes, bit for bit) and against the host's results ``want``."""
    for k in range(load.shape[0]):
        u = load[k] if cap is None else load[k] / cap
        top = u.max() if u.size else 0.0
        assert peak[k] == top, k
        assert pe[k] == (int(u.argmax()) if top > 0 else -1), k
        assert close([peak[k]], [want[3][k]]), k
        if want[3][k] > 0:
            hu = want[0][k] if cap is None else want[0][k] / cap
            assert hu[pe[k]] >= want[3][k] * (1 - 1e-9), k
        else:
            assert pe[k] == -1 and peak[k] == 0.0


def same(got, want, exact=False, cap=None):
    """The engine's 5-tuple against the host's: loads within the tolerance (or
    bit for bit), lost and routed exactly, the peaks as peaks_ok has them."""
    if exact:
        assert np.array_equal(got[0], want[0])
    else:
        assert got[0].shape == want[0].shape
        for k in range(want[0].shape[0]):
            assert close(got[0][k], want[0][k]), k
    assert np.array_equal(got[1], want[1])
    assert got[2].dtype == bool and np.array_equal(got[2], want[2])
    assert got[3].dtype == np.float64 and got[4].dtype == np.int32
    peaks_ok(got[0], got[3], got[4], want, cap)


def down_of(cost, E, sc):
    now = np.ones(E, np.uint32) if cost is None else np.asarray(cost, np.uint32).copy()
    now[np.asarray(sc[0], np.int64)] = np.asarray(sc[1], np.int64).astype(np.uint32)
    return np.nonzero(now == INF)[0]


def check(eng, csr, cost, dsts, rows, srcs, w, scen, kernel=LDS, exact=False, cap=None,
          weights=(True, False)):
    """Both splits, with and without the weights, on the GPU against the host
    restatement; returns the expected weighted results per split."""
    ex = on(csr)
    out = {}
    for split in SPLITS:
        for wt in [w if x else None for x in weights]:
            want = EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, wt, scen, split,
                                                  cap)
            got = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, wt, scen, split, cap,
                                             timing=True)
            same(got, want, exact, cap)
            for k, sc in enumerate(scen):
                assert not got[0][k][down_of(cost, int(csr.E), sc)].any()
            assert eng.ctx.last_kernel() == kernel and eng.ctx.last_launches() == 1
            assert eng.ctx.last_kernel_ms() > 0
            if wt is not None:
                out[split] = want
    return out


def raw(eng, dsts, off, srcs, w, soff, edges, costs, load, lost=None, routed=None, cap=None,
        peak=None, pedge=None, hop=False, timing=False):
    """One sdnr_whatif_ecmp_link_loads call on device copies of the arguments
    (the override lists as given: not sorted, not checked), adding into the
    device tensors; no synchronize."""
    import torch
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).to(eng.dev)   # noqa: E731
    c = np.asarray(list(costs) + [0], np.int64).astype(np.uint32).view(np.int32)
    keep = [dev(dsts, np.int32), dev(off, np.int64), dev(srcs, np.int32),
            dev(np.asarray(w, np.uint64).view(np.int64), np.int64) if w is not None else None,
            dev(soff, np.int64), dev(list(edges) + [0], np.int32), dev(c, np.int32),
            dev(cap, np.float64) if cap is not None else None]
    torch.cuda.synchronize()
    p = lambda a: a.data_ptr() if a is not None else 0     # noqa: E731
    eng.ctx.whatif_ecmp_link_loads_device(
        keep[0].data_ptr(), len(dsts), keep[1].data_ptr(), keep[2].data_ptr(), p(keep[3]),
        len(soff) - 1, keep[4].data_ptr(), keep[5].data_ptr(), keep[6].data_ptr(),
        load.data_ptr(), p(lost), p(routed), p(keep[7]), p(peak), p(pedge), hop=hop,
        timing=timing)
    return keep


# ------------------------------------------------------------ the named cases --

def test_a_lowered_cost_opens_the_long_way_round(eng):
    csr, cost, edge, dsts, rows, srcs, w, scen = lowered_ring_case()
    want = check(eng, csr, cost, dsts, rows, srcs, w, scen)
    for split in SPLITS:
        got = eng.whatif_ecmp_link_loads(on(csr), cost, dsts, rows, srcs, w, scen, split)
        # fails if the Bellman-Ford reads the uploaded cost 3 of 0 -> 5
        assert got[0][0][edge[(1, 0)]] > 0 and got[0][1][edge[(1, 0)]] == 0.0
        assert got[2].all() and not got[1].any()
        assert close(got[0][0], want[split][0][0])


def test_a_cost_raised_to_a_tie_across_depths(eng):
    csr, cost, edge, (s, a, b, d), scen = raised_chord_case()
    w = np.array([12], np.uint64)
    check(eng, csr, cost, [d], [0], [s], w, scen)
    check(eng, csr, None, [d], [0], [s], w, scen)          # the unit base without an upload
    for split in SPLITS:
        got = eng.whatif_ecmp_link_loads(on(csr), cost, [d], [0], [s], w, scen, split)
        # one walk on the base cost and another on the override drops flow on the way
        into_d = got[0][0][[edge[(s, d)], edge[(a, d)], edge[(b, d)]]]
        assert close([into_d.sum()], [12.0]) and close(into_d, [4.0, 4.0, 4.0])
        assert got[0][1][edge[(s, d)]] == 12.0 and got[0][1][edge[(s, a)]] == 0.0


@pytest.mark.parametrize("chord", [False, True])
def test_the_trap_an_inf_override_on_a_link_that_stays_tight_carries_nothing(eng, chord):
    csr, cost, edge, (s, a, b, d) = trap_case(chord)
    scen = [([edge[(s, a)]], [INF]), ([], [])]
    w = np.array([8, 4], np.uint64)
    want = check(eng, csr, cost, [d], [0, 0], [s, a], w, scen, exact=True)
    for split in SPLITS:
        got = eng.whatif_ecmp_link_loads(on(csr), cost, [d], [0, 0], [s, a], w, scen, split)
        assert got[0][0][edge[(s, a)]] == 0.0 and got[0][1][edge[(s, a)]] > 0
        assert got[0][0][edge[(s, b)]] == (4.0 if chord else 8.0)
        assert np.array_equal(got[0], want[split][0])


# --------------------------------------------------- against the sister kernels --

def k8_case():
    fabric = T.fat_tree(8)
    csr = fabric.csr()
    h = 4
    esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    core = (esrc < h * h) | (np.asarray(csr.col) < h * h)
    cost = np.where(core, 5, 3).astype(np.uint32)
    hv = np.unique(fabric.host_table()[0])
    n = hv.shape[0]
    rows = np.repeat(np.arange(n), n)
    srcs = np.tile(hv, n)
    w = np.random.default_rng(8).integers(0, 1 << 20, n * n, dtype=np.uint64)
    return csr, cost, hv, rows, srcs, w


def test_all_inf_scenarios_equal_the_failure_kernel(eng):
    # dyadic: an edge switch isolated, every share a power of two -- bit for bit
    csr, cost, hv, rows, srcs, w = k8_case()
    ex = on(csr)
    lists = [switch_edges(csr, int(hv[0])), switch_edges(csr, int(hv[5])), []]
    scen = [(es, [INF] * len(es)) for es in lists]
    for split in SPLITS:
        for wt in (w, None):
            fail = eng.failure_ecmp_link_loads(ex, cost, hv, rows, srcs, wt, lists, split)
            got = eng.whatif_ecmp_link_loads(ex, cost, hv, rows, srcs, wt, scen, split)
            assert eng.ctx.last_kernel() == LDS and eng.ctx.last_launches() == 1
            assert fail[0].any() and np.array_equal(got[0], fail[0]), split
            assert np.array_equal(got[1], fail[1]) and np.array_equal(got[2], fail[2])
            assert got[1][0] > 0
    # single cables leave thirds: within rtol
    csr, cost, dsts, rows, srcs, w, lists = small_case("torus_5x3x2", 5)
    ex = on(csr)
    scen = [(es, [INF] * len(es)) for es in lists]
    for split in SPLITS:
        for wt in (w, None):
            fail = eng.failure_ecmp_link_loads(ex, cost, dsts, rows, srcs, wt, lists, split)
            got = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, wt, scen, split)
            assert all(close(got[0][k], fail[0][k]) for k in range(len(lists)))
            assert np.array_equal(got[1], fail[1]) and np.array_equal(got[2], fail[2])


def test_an_override_equal_to_the_base_cost_and_the_empty_scenario(eng):
    csr, cost, hv, rows, srcs, w = k8_case()
    ex = on(csr)
    some = np.arange(0, int(csr.E), 7)
    scen = [(some, cost[some]), ([], []), ([0, int(csr.E) - 1], cost[[0, -1]])]
    for split in SPLITS:
        for wt in (w, None):
            pc, _, _ = eng.cost_tables(ex, cost, hv)
            sister = eng.cost_ecmp_link_loads(ex, cost, pc, rows, srcs, wt, split)
            got = eng.whatif_ecmp_link_loads(ex, cost, hv, rows, srcs, wt, scen, split)
            assert eng.ctx.last_kernel() == LDS and eng.ctx.last_launches() == 1
            assert sister.any() and got[2].all() and not got[1].any()
            for k in range(len(scen)):
                assert np.array_equal(got[0][k], sister), (split, k)
    # not dyadic: random costs on a torus
    csr, cost, dsts, rows, srcs, w, _ = small_case("torus_5x3x2", 5)
    ex = on(csr)
    for split in SPLITS:
        pc, _, _ = eng.cost_tables(ex, cost, dsts)
        sister = eng.cost_ecmp_link_loads(ex, cost, pc, rows, srcs, w, split)
        got = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, w,
                                         [([3, 4], cost[[3, 4]]), ([], [])], split)
        assert close(got[0][0], sister) and close(got[0][1], sister)


def hub_case():
    """Hub 0 with 100 leaves, neighbouring leaves linked so that costs matter;
    70 of the hub's out-links overridden (more than a wave has lanes) --
    raised, lowered and down, mixed --, edge 0 and edge E - 1 among the
    overrides."""
    csr = digraph_csr(both_ways([(0, v) for v in range(1, 101)] +
                                [(v, v + 1) for v in range(1, 100)]))
    E = int(csr.E)
    cost = random_costs(csr, 2, 4, 70)
    rng = np.random.default_rng(71)
    hub = np.arange(70)                                    # the hub's first 70 out-links
    c = np.where(np.arange(70) % 3 == 0, INF, rng.integers(1, 7, 70)).astype(np.int64)
    c[0] = 1
    scen = [(np.append(hub, E - 1), np.append(c, 6)), ([0, E - 1], [INF, INF]), ([], [])]
    dsts = [5, 80, 0, 99]
    rows = np.repeat(np.arange(4), 101)
    srcs = np.tile(np.arange(101), 4)
    w = rng.integers(1, 1 << 20, rows.shape[0], dtype=np.uint64)
    return csr, cost, dsts, rows, srcs, w, scen


def test_hub_with_70_overridden_out_links(eng):
    csr, cost, dsts, rows, srcs, w, scen = hub_case()
    assert csr.row_ptr[1] == 100 and len(scen[0][0]) == 71
    c = np.asarray(scen[0][1][:70])
    assert (c == INF).any() and (c < cost[:70]).any() and (c > cost[:70]).any()
    want = check(eng, csr, cost, dsts, rows, srcs, w, scen)
    assert not np.array_equal(want["route"][0][0], want["route"][0][2])


def test_no_uploaded_costs_overrides_on_the_unit_base(eng):
    csr, _, dsts, rows, srcs, w, lists = small_case("torus_5x3x2", 5)
    scen = cost_scenarios(csr, None, lists[:6], 77, 3)
    want = check(eng, csr, None, dsts, rows, srcs, w, scen)
    ones = np.ones(int(csr.E), np.uint32)
    again = EN.whatif_ecmp_link_loads_host(csr, ones, dsts, rows, srcs, w, scen)
    assert np.array_equal(want["route"][0], again[0])
    assert not np.array_equal(want["route"][0][0], want["route"][0][-1])


# ------------------------------------------------------------------ bad lists --

def test_bad_lists_are_ignored_entry_by_entry_and_reported(eng):
    import torch
    csr, cost, dsts, rows, srcs, w, _ = small_case("torus_5x3x2", 5)
    V, E = int(csr.V), int(csr.E)
    ex = on(csr)
    bound = -(-INF // (V - 1))                              # the least cost the rule refuses
    good = [([0], [3]), ([7], [3]), ([E - 1], [INF]), ([7, 8, 9], [2, INF, 4]), ([9], [3])]
    want = EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, good)
    eng.set_link_costs(ex, cost)
    order, off, s, ww = grouped(rows, srcs, w, V, V)
    n = len(rows)

    def call(lists, cap=None):
        soff = np.concatenate([[0], np.cumsum([len(x[0]) for x in lists])])
        load = zeros_f64(eng, len(lists) * E).reshape(len(lists), E)
        lost = zeros_f64(eng, len(lists))
        routed = torch.full((len(lists), n), 9, dtype=torch.uint8, device=eng.dev)
        peak = torch.full((len(lists),), -5.0, dtype=torch.float64, device=eng.dev)
        pedge = torch.full((len(lists),), -5, dtype=torch.int32, device=eng.dev)
        keep = raw(eng, dsts, off, s, ww, soff, [e for x in lists for e in x[0]],
                   [c for x in lists for c in x[1]], load, lost, routed, cap, peak, pedge)
        return keep, load, lost, routed, peak, pedge

    def slices_ok(load, lost, routed, pairs):
        assert np.isfinite(load.cpu().numpy()).all()
        for mine, theirs in pairs:
            assert close(load[mine].cpu().numpy(), want[0][theirs]), (mine, theirs)
            assert lost[mine].item() == want[1][theirs]
            r = routed[mine].cpu().numpy()
            assert np.array_equal(r if isinstance(order, slice) else r[np.argsort(order)],
                                  want[2][theirs])

    def reported():
        with pytest.raises(_native.SdnrError) as ei:
            eng.ctx.synchronize()
        assert ei.value.code == -22 and "sdnr_whatif_ecmp_link_loads" in str(ei.value)
        eng.ctx.synchronize()                              # reported once

    # the good lists as they are: no error
    keep, load, lost, routed, peak, pedge = call(good)
    eng.ctx.synchronize()
    slices_ok(load, lost, routed, [(k, k) for k in range(len(good))])
    peaks_ok(load.cpu().numpy(), peak.cpu().numpy(), pedge.cpu().numpy(), want, None)
    # (the bad list, the good scenario it must equal once the bad entry is ignored)
    bads = [(([5, 7], [0, 3]), 1),                          # cost 0
            (([5, 7], [bound, 3]), 1),                      # a cost at the (V - 1) bound
            (([7, 7], [3, 5]), 1),                          # a repeated edge: the second is ignored
            (([9, 7], [3, 4]), 4),                          # a descending pair: 7 is ignored
            (([-1, 7], [2, 3]), 1),                         # index -1
            (([7, E], [3, 2]), 1)]                          # index E
    for bad, equal in bads:
        keep, load, lost, routed, peak, pedge = call([good[0], bad, good[2], good[3]])
        reported()
        slices_ok(load, lost, routed, [(0, 0), (1, equal), (2, 2), (3, 3)])
    # the largest cost the rule accepts is accepted
    keep, load, lost, routed, peak, pedge = call([([5], [bound - 1])])
    eng.ctx.synchronize()
    # a capacity that is 0 or NaN: that link is left out of the peak, and reported
    for x in (0.0, float("nan")):
        top = int(want[4][0])
        cap = np.ones(E)
        cap[top] = x
        keep, load, lost, routed, peak, pedge = call(good, cap)
        reported()
        slices_ok(load, lost, routed, [(k, k) for k in range(len(good))])
        ld = load.cpu().numpy()
        for k in range(len(good)):
            u = ld[k].copy()
            u[top] = 0.0
            assert peak[k].item() == u.max() and pedge[k].item() == int(u.argmax()) != top
    del keep
    # one of peak / peak_edge without the other
    with pytest.raises(_native.SdnrError) as ei:
        raw(eng, dsts, off, s, ww, [0, 0], [], [], load, peak=peak)
    assert ei.value.code == -22
    check(eng, csr, cost, dsts, rows, srcs, w, good)       # the context goes on working


# ------------------------------------------------- several scenarios in one call --

def test_accumulation_permutation_rows_without_pairs_and_a_destination_outside(eng):
    import torch
    fabric = T.fat_tree(4)
    csr = fabric.csr()
    V, E = int(csr.V), int(csr.E)
    ex = on(csr)
    hv = np.unique(fabric.host_table()[0])
    cables = cable_edges(csr)
    cost = random_costs(csr, 1, 3, 44)
    scen = [(cables[0], [3, 3]), (cables[5], [INF, 1]), ([], []), (cables[0], [3, 3]),
            (switch_edges(csr, int(hv[0])), [INF] * len(switch_edges(csr, int(hv[0]))))]
    rng = np.random.default_rng(4)
    dsts = np.append(np.arange(V), V + 2)                  # the core rows have no pairs
    rows = np.append(np.repeat(hv, hv.shape[0]), [V, V])   # ... the last row no vertex
    srcs = np.append(np.tile(hv, hv.shape[0]), [hv[0], hv[1]])
    w = rng.integers(0, 1 << 20, rows.shape[0], dtype=np.uint64)
    w[-2:] = 5, 6
    assert np.setdiff1d(dsts, rows).size
    for split in SPLITS:
        for wt in (w, None):
            want = EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, wt, scen, split)
            got = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, wt, scen, split)
            same(got, want)
            assert eng.ctx.last_kernel() == LDS and eng.ctx.last_launches() == 1
            assert close(got[0][0], got[0][3]) and np.array_equal(got[2][0], got[2][3])
            assert not got[2][:, -2:].any() and (got[1] >= (11 if wt is not None else 2)).all()
            perm = [4, 2, 0, 3, 1]
            again = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, wt,
                                               [scen[i] for i in perm], split)
            for k, i in enumerate(perm):
                assert close(again[0][k], got[0][i]) and close([again[3][k]], [got[3][i]])
                assert again[1][k] == got[1][i] and np.array_equal(again[2][k], got[2][i])
    # the call adds into a pre-filled load, and the peak is over load as it then stands
    want = EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, scen)
    nrows = len(dsts)
    order, off, s, ww = grouped(rows, srcs, w, nrows, V)
    soff = np.concatenate([[0], np.cumsum([len(x[0]) for x in scen])])
    flat = [int(e) for x in scen for e in x[0]]
    flatc = [int(c) for x in scen for c in x[1]]
    load = zeros_f64(eng, len(scen) * E).reshape(len(scen), E)
    load += 7
    lost = zeros_f64(eng, len(scen))
    peak = zeros_f64(eng, len(scen))
    pedge = torch.zeros(len(scen), dtype=torch.int32, device=eng.dev)
    eng.set_link_costs(ex, cost)
    eng.ctx.whatif_ecmp_link_loads_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)     # nscen == 0
    k1 = raw(eng, dsts, off, s, ww, soff, flat, flatc, load, lost, None, None, peak, pedge)
    eng.ctx.synchronize()
    ld = load.cpu().numpy()
    for k in range(len(scen)):
        assert close(ld[k], want[0][k] + 7)
        assert peak[k].item() == ld[k].max() and pedge[k].item() == int(ld[k].argmax())
    k2 = raw(eng, dsts, off, s, ww, soff, flat, flatc, load, lost)
    eng.ctx.synchronize()
    for k in range(len(scen)):
        assert close(load[k].cpu().numpy(), 2 * want[0][k] + 7)
    assert np.array_equal(lost.cpu().numpy(), 2 * want[1])
    # no pairs: nothing is added, the peaks are still written from load as it stands
    load.zero_()
    k3 = raw(eng, dsts, np.zeros(nrows + 1, np.int64), s, ww, soff, flat, flatc, load, lost, None,
             None, peak, pedge)
    eng.ctx.synchronize()
    assert not load.cpu().numpy().any() and not peak.cpu().numpy().any()
    assert (pedge.cpu().numpy() == -1).all()
    del k1, k2, k3


# ----------------------------------------------------------------------- peak --

def test_peak_with_capacities_without_demand_and_in_three_chunks(eng):
    csr, cost, dsts, rows, srcs, w, lists = small_case("fat_tree_k4", 1)
    E = int(csr.E)
    ex = on(csr)
    scen = cost_scenarios(csr, cost, lists[:6], 5, 5)       # 6 and the empty one
    cap = np.random.default_rng(6).uniform(0.5, 4.0, E)
    for c in (None, cap):
        check(eng, csr, cost, dsts, rows, srcs, w, scen, cap=c)
    # a scenario without demand: every weight zero
    got = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, np.zeros(len(rows), np.uint64),
                                     scen[:2], "route", cap)
    assert got[3].tolist() == [0.0, 0.0] and got[4].tolist() == [-1, -1] and not got[0].any()
    # loads=False over three chunks of three, three and one scenarios
    budget = 3 * (8 * E + len(rows))
    for split in SPLITS:
        for c in (None, cap):
            full = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, scen, split, c)
            part = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, scen, split, c,
                                              table_budget=budget)
            same(part, full, cap=c)
            lean = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, scen, split, c,
                                              loads=False, table_budget=budget)
            assert lean[0] is None and lean[2] is None
            assert np.array_equal(lean[1], full[1])
            # (the peak edge of sums that differ in their last bits may be another tied link)
            assert close(lean[3], full[3])
            hu = full[0] if c is None else full[0] / c
            assert all(hu[k][lean[4][k]] >= full[3][k] * (1 - 1e-9) for k in range(len(scen)))
            bare = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, scen, split, c,
                                              loads=False, reach=False, table_budget=budget)
            assert bare[0] is None and bare[1] is None and bare[2] is None
            assert close(bare[3], full[3])


# ---------------------------------------------------------------- global form --

def test_both_sides_of_the_lds_bound(eng):
    """V = kFailureLdsMaxV is the last graph whose row state (23 bytes per
    vertex) fits LDS; one more keeps it in the context scratch.  One link
    raised and one down among the links into destination 4321."""
    bound = EN.FAILURE_LDS_MAX_V
    for V, kernel in ((bound, LDS), (bound + 1, GLOBAL)):
        csr = random_csr(V, 3 * V, 9)
        cost = random_costs(csr, 1, 5, V)
        dsts = [0, 4321, 7000]                             # 7000: in the unreachable fifth
        rng = np.random.default_rng(V)
        rows = rng.integers(0, 3, 600)
        srcs = rng.integers(0, V, 600)
        w = rng.integers(0, 1 << 32, 600, dtype=np.uint64)
        into = np.nonzero(np.asarray(csr.col) == 4321)[0][:2]
        scen = [(into, [int(cost[into[0]]) + 3, INF]), ([], [])]
        ex = on(csr)
        for split in SPLITS:
            want = EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, scen, split)
            got = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, scen, split,
                                             timing=True)
            same(got, want)
            assert eng.ctx.last_kernel() == kernel and eng.ctx.last_launches() == 1
            assert eng.ctx.last_kernel_ms() > 0
        assert want[0].any() and not want[2].all() and want[2].any()
        assert not np.array_equal(want[0][0], want[0][1])


# ------------------------------------------------------------------- k = 48 --

PICK = np.array([0, 1, 23, 24, 500, 777, 1150, 1151])


def k48_case():
    """fat_tree(48) with the first core group at cost 2, eight destination rows,
    every host-bearing source, and four scenarios: empty; an aggregation -> core
    link raised to 2; one lowered from an uploaded 2 to 1; a cable down with a
    raised and a lowered link beside it."""
    fabric = T.fat_tree(48)
    csr = fabric.csr()
    hv = fabric.host_table()[0]
    hc = np.bincount(hv, minlength=csr.V).astype(np.int64)
    srcs = np.nonzero(hc)[0]
    assert srcs.shape[0] == 1152
    edge_sw = int(srcs[PICK[4]])
    esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    col = np.asarray(csr.col)
    cost = core_tier_costs(csr, 48)
    # the aggregation switches above the edge switch: position 0 reaches the
    # core group at cost 2, position 1 a group at cost 1 (the cores are 0 .. 575)
    agg0, agg1 = (int(x) for x in col[csr.row_ptr[edge_sw]:csr.row_ptr[edge_sw] + 2])
    em = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(esrc.tolist(), col.tolist()))
          if a in (edge_sw, agg0, agg1) or b in (edge_sw, agg0, agg1)}
    c1 = [int(c) for c in col[csr.row_ptr[agg1]:csr.row_ptr[agg1 + 1]] if c < 576]
    assert cost[em[(edge_sw, agg0)]] == 1 and all(cost[em[(agg1, c)]] == 1 for c in c1)
    assert cost[em[(agg0, int(col[csr.row_ptr[agg0]]))]] == 2
    cost[[em[(agg1, c1[2])], em[(agg1, c1[3])]]] = 2        # two more links uploaded at 2
    mix = {em[(agg1, c1[1])]: INF, em[(c1[1], agg1)]: INF, em[(edge_sw, agg1)]: 3,
           em[(agg1, c1[3])]: 1}
    scen = [([], []), ([em[(agg1, c1[0])]], [2]), ([em[(agg1, c1[2])]], [1]),
            (sorted(mix), [mix[e] for e in sorted(mix)])]
    dsts = srcs[PICK]
    n = srcs.shape[0]
    rows = np.repeat(np.arange(PICK.shape[0]), n)
    s = np.tile(srcs, PICK.shape[0])
    w = (hc[s] * hc[dsts[rows]]).astype(np.uint64)
    return csr, cost, dsts, rows, s, w, scen


def test_k48_four_scenarios_eight_rows_every_host_bearing_source(eng):
    csr, cost, dsts, rows, s, w, scen = k48_case()
    ex = on(csr)
    for split in SPLITS:
        for wt in (w, None):
            want = EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows, s, wt, scen, split)
            got = eng.whatif_ecmp_link_loads(ex, cost, dsts, rows, s, wt, scen, split,
                                             timing=True)
            same(got, want)
            assert eng.ctx.last_kernel() == LDS and eng.ctx.last_launches() == 1
            assert eng.ctx.last_kernel_ms() > 0
            assert got[2].all() and not got[1].any() and want[0].any()
            for k in (1, 2, 3):
                assert not np.array_equal(want[0][0], want[0][k]), (split, k)


# ------------------------------------------------------------------ the drop-in --

def real_db(eng):
    from sdnmpi_amd.util.topology_db import TopologyDB
    return lambda fabric: fabric.populate(TopologyDB(engine=eng))


@pytest.mark.parametrize("name,with_costs", [("fat_tree_k4", False), ("torus_2x2x2", True)])
def test_dropin_equals_a_twin_with_the_changes_really_made(eng, name, with_costs):
    check_dropin(real_db(eng), name, with_costs)


def test_the_tuner_on_the_fish(eng):
    check_fish(real_db(eng))
    assert eng.ctx.last_kernel() == LDS and eng.ctx.last_launches() == 1
