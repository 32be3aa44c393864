"""failure_loads.hip (sdnr_failure_ecmp_link_loads) on the GPU against
engine.failure_ecmp_link_loads_host -- which really removes the failed links --
and the drop-in's failure_link_loads against a second TopologyDB whose links
were deleted.

Tolerance (see test_ecmp_link_loads.py): rtol = 1e-9, atol = 0 where the
expected value is nonzero, exactly 0.0 where it is 0 -- a failed link among
them.  The dyadic cases (power-of-two shares, integer weights: every partial
sum exact in any order) are compared bit for bit.  ``routed`` is compared
exactly; ``lost`` is a sum of integers below 2^53 in these cases: exact."""
import ctypes

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from test_cost_ecmp_loads import random_costs
from test_cost_ecmp_loads_gpu import core_tier_costs
from test_ecmp_link_loads import SPLITS, close, dicts_close
from test_ecmp_link_loads_gpu import zeros_f64
from test_failure_loads import (cable_edges, cut_case, dropin_case, ring_case, small_case,
                                star_case, switch_edges, trap_case)
from test_link_loads import random_csr
from test_link_loads_gpu import on

pytestmark = pytest.mark.gpu

LDS, GLOBAL = "failure_ecmp_loads_kernel<lds>", "failure_ecmp_loads_kernel<global>"


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def same(got, want, exact=False):
    """(load, lost, routed) triples: loads within the tolerance (or bit for
    bit), lost and routed exactly."""
    if exact:
        assert np.array_equal(got[0], want[0])
    else:
        assert got[0].shape == want[0].shape
        for k in range(want[0].shape[0]):
            assert close(got[0][k], want[0][k]), k
    assert np.array_equal(got[1], want[1])
    assert got[2].dtype == bool and np.array_equal(got[2], want[2])


def check(eng, csr, cost, dsts, rows, srcs, w, scen, kernel=LDS, exact=False):
    """Both splits, with and without the weights, on the GPU against the host
    restatement; returns the expected weighted results per split."""
    ex = on(csr)
    out = {}
    for split in SPLITS:
        for wt in (w, None):
            want = EN.failure_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, wt, scen, split)
            got = eng.failure_ecmp_link_loads(ex, cost, dsts, rows, srcs, wt, scen, split)
            same(got, want, exact)
            for k, failed in enumerate(scen):
                assert not got[0][k][np.asarray(failed, np.int64)].any()
            assert eng.ctx.last_kernel() == kernel and eng.ctx.last_launches() == 1
            if wt is not None:
                out[split] = want
    return out


def raw(eng, dsts, off, srcs, w, soff, edges, load, lost=None, routed=None, hop=False,
        timing=False):
    """One sdnr_failure_ecmp_link_loads call on device copies of the arguments
    (the scenario list as given: not sorted, not deduplicated), adding into the
    device tensors; no synchronize."""
    import torch
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).to(eng.dev)   # noqa: E731
    keep = [dev(dsts, np.int32), dev(off, np.int64), dev(srcs, np.int32),
            dev(np.asarray(w, np.uint64).view(np.int64), np.int64) if w is not None else None,
            dev(soff, np.int64), dev(list(edges) + [0], np.int32)]
    torch.cuda.synchronize()
    eng.ctx.failure_ecmp_link_loads_device(
        keep[0].data_ptr(), len(dsts), keep[1].data_ptr(), keep[2].data_ptr(),
        keep[3].data_ptr() if keep[3] is not None else 0, len(soff) - 1, keep[4].data_ptr(),
        keep[5].data_ptr(), load.data_ptr(), lost.data_ptr() if lost is not None else 0,
        routed.data_ptr() if routed is not None else 0, hop=hop, timing=timing)
    return keep


def grouped(rows, srcs, w, nrows, V):
    """The pairs in row order as the C call wants them: (order, pair_off, srcs, w)."""
    order, off = EN._pairs_by_row(np.asarray(rows, np.int64), nrows)
    s = np.asarray(srcs, np.int64)[order]
    s = np.where((s < 0) | (s >= V), -1, s)
    return order, off, s, (None if w is None else np.asarray(w, np.uint64)[order])


# ------------------------------------------------------------ the named cases --

@pytest.mark.parametrize("chord", [False, True])
def test_the_trap_a_failed_link_that_stays_tight_carries_exactly_nothing(eng, chord):
    csr, cost, edge, (s, a, b, d) = trap_case(chord)
    scen = [[edge[(s, a)]], []]
    want = check(eng, csr, cost, [d], [0, 0], [s, a], np.array([8, 4], np.uint64), scen,
                 exact=True)
    for split in SPLITS:
        got = eng.failure_ecmp_link_loads(on(csr), cost, [d], [0, 0], [s, a], [8, 4], scen, split)
        assert got[0][0][edge[(s, a)]] == 0.0 and got[0][1][edge[(s, a)]] > 0
        assert got[0][0][edge[(s, b)]] == (4.0 if chord else 8.0)
        assert np.array_equal(got[0], want[split][0])
    # and without uploaded costs where every cost is 1
    if not chord:
        check(eng, csr, None, [d], [0, 0], [s, a], np.array([8, 4], np.uint64), scen, exact=True)


def test_cut_pairs_are_lost_and_failures_are_directed(eng):
    csr, edge, dsts, rows, srcs, w = cut_case()
    want = check(eng, csr, None, dsts, rows, srcs, w, [[edge[(1, 2)]]], exact=True)
    load, lost, routed = want["route"]
    assert routed.tolist() == [[False, False, True]] and lost.tolist() == [8.0]
    assert load[0][edge[(2, 1)]] == 7.0 and load[0][edge[(1, 0)]] == 7.0


def test_ring_the_longer_way_round_and_a_tied_direct_link(eng):
    csr, cost, edge, dsts, rows, srcs, w, scen = ring_case()
    want = check(eng, csr, cost, dsts, rows, srcs, w, scen, exact=True)
    assert want["route"][0][0][edge[(1, 2)]] >= 32.0 and want["route"][2].all()


def test_star_with_70_failed_links_at_one_vertex(eng):
    csr, edge, dsts, rows, srcs, w, scen = star_case()
    want = check(eng, csr, None, dsts, rows, srcs, w, scen, exact=True)
    cost = random_costs(csr, 1, 5, 8)
    check(eng, csr, cost, dsts, rows, srcs, w, scen)
    assert want["route"][1][0] == float(w[:101].sum() - w[5])


# ----------------------------------------------------------------- boundaries --

def test_first_and_last_edge_duplicates_and_bad_lists(eng):
    csr, cost, dsts, rows, srcs, w, _ = small_case("torus_5x3x2", 5)
    V, E = int(csr.V), int(csr.E)
    ex = on(csr)
    scen = [[0], [E - 1], [0, E - 1], [7, 8, 9]]
    check(eng, csr, cost, dsts, rows, srcs, w, scen)
    want = EN.failure_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, scen)
    eng.set_link_costs(ex, cost)
    order, off, s, ww = grouped(rows, srcs, w, V, V)
    n = len(rows)
    import torch

    def call(lists):
        soff = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
        load = zeros_f64(eng, len(lists) * E).reshape(len(lists), E)
        lost = zeros_f64(eng, len(lists))
        routed = torch.full((len(lists), n), 9, dtype=torch.uint8, device=eng.dev)
        keep = raw(eng, dsts, off, s, ww, soff, [e for x in lists for e in x], load, lost, routed)
        return keep, load, lost, routed

    def slices_ok(load, lost, routed, pairs):
        for mine, theirs in pairs:
            assert close(load[mine].cpu().numpy(), want[0][theirs])
            assert lost[mine].item() == want[1][theirs]
            assert np.array_equal(routed[mine].cpu().numpy()[np.argsort(order)]
                                  if not isinstance(order, slice) else
                                  routed[mine].cpu().numpy(), want[2][theirs])

    # duplicates in an ascending list are fine
    keep, load, lost, routed = call([[0, 0, 0], [E - 1, E - 1], [0, 0, E - 1], [7, 7, 8, 9, 9]])
    eng.ctx.synchronize()
    slices_ok(load, lost, routed, [(0, 0), (1, 1), (2, 2), (3, 3)])
    # an index outside [0, E) is ignored and reported; the other scenarios stay right
    for bad in ([0, E], [-1, E - 1]):
        keep, load, lost, routed = call([[0], bad, [0, E - 1], [7, 8, 9]])
        with pytest.raises(_native.SdnrError) as ei:
            eng.ctx.synchronize()
        assert ei.value.code == -22 and "sdnr_failure_ecmp_link_loads" in str(ei.value)
        eng.ctx.synchronize()                              # reported once
        slices_ok(load, lost, routed, [(0, 0), (1, 0 if bad[0] == 0 else 1), (2, 2), (3, 3)])
    # a descending list is reported; the other scenarios stay right
    keep, load, lost, routed = call([[0], [9, 8, 7], [0, E - 1], [7, 8, 9]])
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "ascending" in str(ei.value)
    assert np.isfinite(load.cpu().numpy()).all()
    slices_ok(load, lost, routed, [(0, 0), (2, 2), (3, 3)])
    del keep
    check(eng, csr, cost, dsts, rows, srcs, w, scen)       # the context goes on working


# ------------------------------------------------- several scenarios in one call --

def test_scenarios_twice_permuted_rows_without_pairs_and_accumulation(eng):
    import torch
    fabric = T.fat_tree(4)
    csr = fabric.csr()
    V, E = int(csr.V), int(csr.E)
    ex = on(csr)
    hv = np.unique(fabric.host_table()[0])
    cables = cable_edges(csr)
    scen = [cables[0], cables[5], [], cables[0], switch_edges(csr, int(hv[0]))]
    rng = np.random.default_rng(4)
    dsts = np.arange(V)                                    # the core rows have no pairs
    rows = np.repeat(hv, hv.shape[0])
    srcs = np.tile(hv, hv.shape[0])
    w = rng.integers(0, 1 << 20, rows.shape[0], dtype=np.uint64)
    assert np.setdiff1d(dsts, rows).size
    for split in SPLITS:
        want = EN.failure_ecmp_link_loads_host(csr, None, dsts, rows, srcs, w, scen, split)
        got = eng.failure_ecmp_link_loads(ex, None, dsts, rows, srcs, w, scen, split)
        same(got, want)                  # (a failed cable leaves thirds: not dyadic)
        assert close(got[0][0], got[0][3]) and np.array_equal(got[2][0], got[2][3])
        perm = [4, 2, 0, 3, 1]
        again = eng.failure_ecmp_link_loads(ex, None, dsts, rows, srcs, w,
                                            [scen[i] for i in perm], split)
        for k, i in enumerate(perm):
            assert close(again[0][k], got[0][i])
            assert again[1][k] == got[1][i] and np.array_equal(again[2][k], got[2][i])
        assert got[1][4] > 0 and not got[1][:4].any()
    # nscen == 0, nrows == 0 and an empty pair list: SDNR_OK, nothing touched
    eng.failure_ecmp_link_loads(ex, None, dsts, rows, srcs, w, scen[:1])
    order, off, s, ww = grouped(rows, srcs, w, V, V)
    soff = np.concatenate([[0], np.cumsum([len(x) for x in scen])])
    flat = [e for x in scen for e in x]
    load = zeros_f64(eng, len(scen) * E).reshape(len(scen), E)
    lost = zeros_f64(eng, len(scen))
    routed = torch.full((len(scen), len(rows)), 9, dtype=torch.uint8, device=eng.dev)
    load += 7
    eng.ctx.failure_ecmp_link_loads_device(0, 0, 0, 0, 0, 0, 0, 0, 0)
    k0 = raw(eng, dsts, off, s, ww, [0], [], load, lost, routed)             # nscen == 0
    k1 = raw(eng, dsts[:0], off[:1], s, ww, soff, flat, load, lost, routed)  # nrows == 0
    k2 = raw(eng, dsts, np.zeros(V + 1, np.int64), s, ww, soff, flat, load, lost, routed)
    eng.ctx.synchronize()
    assert (load.cpu().numpy() == 7.0).all() and not lost.cpu().numpy().any()
    assert (routed.cpu().numpy() == 9).all()
    # a second call adds into load and lost
    want = EN.failure_ecmp_link_loads_host(csr, None, dsts, rows, srcs, w, scen)
    load -= 7
    k3 = raw(eng, dsts, off, s, ww, soff, flat, load, lost, routed)
    k4 = raw(eng, dsts, off, s, ww, soff, flat, load, lost, None, timing=True)
    eng.ctx.synchronize()
    assert eng.ctx.last_kernel_ms() > 0
    for k in range(len(scen)):
        assert close(load[k].cpu().numpy(), 2 * want[0][k])
    assert np.array_equal(lost.cpu().numpy(), 2 * want[1])
    del k0, k1, k2, k3, k4


# ------------------------------------------------------------- empty scenario --

@pytest.fixture(scope="module")
def small_cases():
    """Per G.SMALL fabric the case of the CPU file plus the empty scenario,
    and the host's results per (split, weighted), computed once."""
    out = {}
    for k, name in enumerate(G.SMALL):
        csr, cost, dsts, rows, srcs, w, scen = small_case(name, k)
        scen = scen + [[]]
        want = {(split, wt is not None):
                EN.failure_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, wt, scen, split)
                for split in SPLITS for wt in (w, None)}
        out[name] = (csr, cost, dsts, rows, srcs, w, scen, want)
    return out


@pytest.mark.parametrize("name", G.SMALL)
def test_small_fabrics_both_splits_routed_and_lost_and_the_empty_scenario(eng, small_cases,
                                                                          name):
    csr, cost, dsts, rows, srcs, w, scen, want = small_cases[name]
    ex = on(csr)
    for split in SPLITS:
        for wt in (w, None):
            got = eng.failure_ecmp_link_loads(ex, cost, dsts, rows, srcs, wt, scen, split)
            same(got, want[(split, wt is not None)])
            assert eng.ctx.last_kernel() == LDS and eng.ctx.last_launches() == 1
        # the empty scenario is the sister kernels' answer on the fabric as it is
        pc, _, _ = eng.cost_tables(ex, cost, dsts)
        assert close(got[0][-1], eng.cost_ecmp_link_loads(ex, cost, pc, rows, srcs, None, split))
        # ... and without uploaded costs the hop-count kernel's
        dist, _, _ = eng.shortest_tables(ex, dsts)
        bare = eng.failure_ecmp_link_loads(ex, None, dsts, rows, srcs, w, [[]], split)
        assert close(bare[0][0], eng.ecmp_link_loads(ex, dist, rows, srcs, w, split))


def test_fat_tree_k8_uniform_tier_costs_empty_scenario_is_bit_exact(eng):
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
    ex = on(csr)
    for split in SPLITS:
        pc, _, _ = eng.cost_tables(ex, cost, hv)
        sister = eng.cost_ecmp_link_loads(ex, cost, pc, rows, srcs, w, split)
        got = eng.failure_ecmp_link_loads(ex, cost, hv, rows, srcs, w, [[], cable_edges(csr)[3]],
                                          split)
        assert sister.any() and np.array_equal(got[0][0], sister), split
        assert got[2].all() and not got[1].any()
        assert not np.array_equal(got[0][1], sister)


# ---------------------------------------------------------------- global form --

def test_both_sides_of_the_lds_bound(eng):
    """V = kFailureLdsMaxV is the last graph whose row state (23 bytes per
    vertex) fits LDS; one more keeps it in the context scratch.  A random graph
    of average degree 8: a dozen relaxation sweeps."""
    bound = EN.FAILURE_LDS_MAX_V
    for V, kernel in ((bound, LDS), (bound + 1, GLOBAL)):
        csr = random_csr(V, 3 * V, 9)
        cost = random_costs(csr, 1, 5, V)
        dsts = [0, 4321, 7000]                             # 7000: in the unreachable fifth
        rng = np.random.default_rng(V)
        rows = rng.integers(0, 3, 600)
        srcs = rng.integers(0, V, 600)
        w = rng.integers(0, 1 << 32, 600, dtype=np.uint64)
        scen = [sorted(rng.choice(int(csr.E), 40, replace=False).tolist()) +
                switch_edges(csr, 4321)[:3], []]
        want = check_one(eng, csr, cost, dsts, rows, srcs, w, scen, kernel)
        assert want[0].any() and not want[2].all() and want[2].any()


def check_one(eng, csr, cost, dsts, rows, srcs, w, scen, kernel):
    """check() with one host evaluation per split (the large shapes)."""
    ex = on(csr)
    for split in SPLITS:
        want = EN.failure_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, scen, split)
        got = eng.failure_ecmp_link_loads(ex, cost, dsts, rows, srcs, w, scen, split, timing=True)
        same(got, want)
        assert eng.ctx.last_kernel() == kernel and eng.ctx.last_launches() == 1
        assert eng.ctx.last_kernel_ms() > 0
    return want


# ------------------------------------------------------------------- k = 48 --

PICK = np.array([0, 1, 23, 24, 500, 777, 1150, 1151])


def test_k48_four_scenarios_eight_rows_every_host_bearing_source(eng):
    fabric = T.fat_tree(48)
    csr = fabric.csr()
    ex = on(csr)
    hv = fabric.host_table()[0]
    hc = np.bincount(hv, minlength=csr.V).astype(np.int64)
    srcs = np.nonzero(hc)[0]
    assert srcs.shape[0] == 1152
    edge_sw = int(srcs[PICK[4]])
    esrc = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    col = np.asarray(csr.col)
    agg = int(col[csr.row_ptr[edge_sw]])                   # an aggregation switch above it
    up = col[csr.row_ptr[agg]:csr.row_ptr[agg + 1]]
    core = int(up[up < 24 * 24][0])                        # the cores are vertices 0 .. 575
    em = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(esrc.tolist(), col.tolist()))
          if a in (edge_sw, agg, core) or b in (edge_sw, agg, core)}
    scen = [sorted([em[(edge_sw, agg)], em[(agg, edge_sw)]]),
            sorted([em[(agg, core)], em[(core, agg)]]),
            switch_edges(csr, core), []]
    cost = core_tier_costs(csr, 48)
    dsts = srcs[PICK]
    n = srcs.shape[0]
    rows = np.repeat(np.arange(PICK.shape[0]), n)
    s = np.tile(srcs, PICK.shape[0])
    w = (hc[s] * hc[dsts[rows]]).astype(np.uint64)
    want = EN.failure_ecmp_link_loads_host(csr, cost, dsts, rows, s, w, scen, "route")
    got = eng.failure_ecmp_link_loads(ex, cost, dsts, rows, s, w, scen, "route", timing=True)
    same(got, want)
    assert eng.ctx.last_kernel() == LDS and eng.ctx.last_launches() == 1
    assert eng.ctx.last_kernel_ms() > 0
    assert got[2].all() and not got[1].any() and want[0].any()
    assert not np.array_equal(got[0][0], got[0][3])
    for split in SPLITS:
        hop = eng.failure_ecmp_link_loads(ex, cost, dsts, rows, s, w, scen[3:], split)
        pc, _, _ = eng.cost_tables(ex, cost, dsts)
        assert close(hop[0][0], eng.cost_ecmp_link_loads(ex, cost, pc, rows, s, w, split)), split


# ------------------------------------------------------------- argument errors --

def test_argument_errors(eng):
    import torch
    csr, cost, dsts, rows, srcs, w, scen = small_case("mock", 0)
    ex = on(csr)
    eng.set_link_costs(ex, cost)
    V, E = int(csr.V), int(csr.E)
    load = zeros_f64(eng, E)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=eng.dev)     # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=eng.dev)     # noqa: E731
    d_dst, d_src, d_edges = i32(V), i32(8), i32(4)
    off, soff = i64(V + 1), i64(2)
    L, h = eng.ctx._lib, eng.ctx._h
    p = lambda t: ctypes.c_void_p(t.data_ptr())           # noqa: E731
    dev = _native.DEVICE_PTRS
    fn = L.sdnr_failure_ecmp_link_loads
    args = [p(d_dst), V, p(off), p(d_src), None, 1, p(soff), p(d_edges), p(load), None, None]

    def with_(i, v):
        a = list(args)
        a[i] = v
        return a
    torch.cuda.synchronize()
    assert fn(h, *args, 0) == -22                                         # host pointers
    for i in (0, 2, 6, 8):                                                # required buffers
        assert fn(h, *with_(i, None), dev) == -22
    assert fn(h, *with_(1, -1), dev) == -22 and fn(h, *with_(5, -1), dev) == -22
    assert fn(h, *args, dev) == 0                                         # no pairs: nothing to do
    off[V] = 2                                                            # pairs, but no srcs
    torch.cuda.synchronize()
    assert fn(h, *with_(3, None), dev) == -22
    soff[1] = 1                                                           # failed links, but no list
    torch.cuda.synchronize()
    assert fn(h, *with_(7, None), dev) == -22
    soff[0] = 3                                                           # scen_off[0] > scen_off[n]
    torch.cuda.synchronize()
    assert fn(h, *args, dev) == -22 and b"scen_off not monotone" in L.sdnr_last_error()
    soff[0] = 0
    off[0] = 5
    torch.cuda.synchronize()
    assert fn(h, *args, dev) == -22 and b"pair_off not monotone" in L.sdnr_last_error()
    with _native.Context(0) as fresh:                                     # no graph uploaded
        assert fn(fresh._h, *args, dev) == -77
    eng.ctx.synchronize()
    assert not load.cpu().numpy().any()
    # offsets of one row / one scenario outside their lists: reported at synchronize
    bad_off = np.zeros(V + 1, np.int64)
    bad_off[1:] = 2
    bad_off[1] = 3
    keep = raw(eng, np.arange(V), bad_off, [0, 1, 0], None, [0, 0], [], load)
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22
    keep = raw(eng, np.arange(V), [0] + [2] * V, [1, 2], None, [0, 5, 1], [0, 1, 2, 3, 4], load)
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22
    del keep
    # a destination outside [0, V) is an empty row: its pairs are not routed, their weight lost
    got = eng.failure_ecmp_link_loads(ex, cost, [V + 3, 1], [0, 0, 1], [0, 2, 0], [5, 6, 7], [[]])
    assert got[2].tolist() == [[False, False, True]] and got[1].tolist() == [11.0]
    want = EN.failure_ecmp_link_loads_host(csr, cost, [V + 3, 1], [0, 0, 1], [0, 2, 0], [5, 6, 7],
                                           [[]])
    same(got, want)


# ------------------------------------------------------------------ the drop-in --

@pytest.mark.parametrize("name,with_costs", [("fat_tree_k4", False), ("random_V12", False),
                                             ("torus_2x2x2", True)])
def test_dropin_equals_a_twin_with_the_links_really_deleted(eng, name, with_costs):
    from sdnmpi_amd.util.topology_db import FailureLoads, TopologyDB
    fabric, _, costs, failures, pairs, w = dropin_case(name, with_costs)
    db = fabric.populate(TopologyDB(engine=eng))
    if costs:
        db.set_link_costs(costs)
    links_before = db.links
    snap = {u: dict(nb) for u, nb in db.links.items()}
    ex = db.graph()
    routes_before = db.find_routes(pairs, multiple=True)
    results = {}
    for split in SPLITS:
        got = results[split] = db.failure_link_loads(failures, pairs, w, split)
        assert isinstance(got, FailureLoads) and got.lost.dtype == np.uint64
        assert dicts_close(got.scenario(len(failures) - 2).as_dict(), got.base.as_dict())
        top, at = got.worst()
        assert np.array_equal(top, got.load.max(0))
        assert np.array_equal(got.load[at, np.arange(ex.csr.E)], top)
        assert all((got.load[:k, e] < top[e]).all() for e, k in enumerate(at.tolist()))
        wd = got.worst_dict()
        assert len(wd) == int((top != 0).sum())
        for (d, p), (x, k) in wd.items():
            assert got.scenario(k).as_dict()[(d, p)] == x
        macs = fabric.host_macs()
        allp = db.all_pairs_failure_link_loads(failures, split)
        byp = db.failure_link_loads(failures, [(a, b) for a in macs for b in macs if a != b],
                                    None, split)
        assert np.array_equal(allp.lost, byp.lost)
        for k in range(len(failures)):
            assert dicts_close(allp.scenario(k).as_dict(), byp.scenario(k).as_dict()), k
    # nothing of the live object changed
    assert db.links is links_before and {u: dict(nb) for u, nb in db.links.items()} == snap
    assert db.graph() is ex and db._link_costs == costs
    assert db.find_routes(pairs, multiple=True) == routes_before
    # the defining property: a second TopologyDB with the links really deleted
    for k, sc in enumerate(failures):
        twin = fabric.populate(TopologyDB(engine=eng))
        if costs:
            twin.set_link_costs(costs)
        for a, b in sc:
            if a in twin.links and b in twin.links[a]:
                twin.delete_link(twin.links[a][b])
        sets = twin.find_routes_least_cost(pairs, multiple=True)
        known = [db._endpoint(a) is not None and db._endpoint(b) is not None for a, b in pairs]
        for split in SPLITS:
            assert dicts_close(results[split].scenario(k).as_dict(),
                               twin.least_cost_ecmp_link_loads(pairs, w, split).as_dict()), k
            assert int(results[split].lost[k]) == \
                sum(x for x, r, ok in zip(w, sets, known) if ok and not r)
