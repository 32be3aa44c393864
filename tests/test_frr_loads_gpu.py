"""frr_loads.hip (sdnr_frr_link_loads) on the GPU against
engine.frr_link_loads_host, against sdnr_link_loads over host-patched rows,
against values written out by hand, and the drop-in's frr_link_loads against
the drop-in over the engine double.  Everything is integer (u64 sums that
wrap): every comparison is array_equal."""
import numpy as np
import pytest

import golden_util as G
import over_grid as OG
import test_frr_loads as TF
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd.util.topology_db import TopologyDB
from test_cost_ecmp_loads import both_ways, digraph_csr, random_costs
from test_ecmp_link_loads import edge_map
from test_lfa_tables_gpu import ring_csr
from test_link_loads_gpu import on

pytestmark = pytest.mark.gpu

KERNEL = "frr_items_kernel<lds>"
# the restatement takes 4 to 6 seconds on these two; the others stay below 3
FABRICS = [n for n in G.SMALL if n not in ("fat_tree_k8", "torus_4x4x4")]
NAMES = ("load", "stat", "status", "peak", "peak_edge", "items")


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def same(got, want):
    for g, w, what in zip(got, want, NAMES):
        if what == "items":
            assert g == w, (what, g, w)
        else:
            assert g.dtype == w.dtype and g.shape == w.shape, what
            assert np.array_equal(g, w), what


_SMALL = {}


def small_case(name):
    """(csr, nh, backup, demand, the four scenario lists in one, the
    restatement's answer), computed once per fabric."""
    if name not in _SMALL:
        csr = G.Golden(name).fabric().csr()
        V = int(csr.V)
        cost = random_costs(csr, 1, 4, 3 * V + 4)
        nh, backup = TF.tables(csr, cost)
        dem = TF.demand(csr, V)
        pad = np.full((1, V), -1, np.int32)                # the row of the bad destination
        nh, backup = np.concatenate([nh, pad]), np.concatenate([backup, pad])
        lists = TF.scenario_lists(csr)
        scen = [s for m in TF.LISTS for s in lists[m]]
        want = EN.frr_link_loads_host(csr, nh, backup, *dem, scen)
        _SMALL[name] = (csr, nh, backup, dem, lists, scen, want)
    return _SMALL[name]


@pytest.mark.parametrize("name", FABRICS)
def test_small_fabrics_equal_the_restatement(eng, name):
    csr, nh, backup, dem, lists, scen, want = small_case(name)
    got = eng.frr_link_loads(on(csr), nh, backup, *dem, scen)
    same(got, want)
    assert eng.ctx.last_kernel() == KERNEL and eng.ctx.last_launches() == 1
    assert want[5] > 0 and want[5] < len(scen) * nh.shape[0]
    assert set(np.unique(want[2]).tolist()) >= {0, 1, 2, 3}
    # without the planes: the same numbers
    bare = eng.frr_link_loads(on(csr), nh, backup, *dem, scen, planes=False)
    assert bare[0] is None and bare[2] is None
    assert all(np.array_equal(bare[i], want[i]) for i in (1, 3, 4)) and bare[5] == want[5]
    # chunks of three scenarios
    dsts, rows, srcs, w = dem
    part = eng.frr_link_loads(on(csr), nh, backup, *dem, scen[:10],
                              table_budget=3 * (8 * int(csr.E) + len(rows)))
    same(part[:5], tuple(x[:10] for x in want[:5]))


@pytest.mark.parametrize("name", ["fat_tree_k4", "dragonfly_a4_h2_p2", "random_V40_loops"])
def test_planes_equal_link_loads_over_host_patched_rows(eng, name):
    """The second oracle: loads.hip's SDNR_LOADS_TO_ROOT over rows patched on
    the host, the pairs the kernel reports undelivered at weight 0.  Over the
    link and cable scenarios, which have no loop (test_frr_loads.py)."""
    csr, nh, backup, (dsts, rows, srcs, w), lists, _, _ = small_case(name)
    V = int(csr.V)
    scen = lists["links"] + lists["cables"]
    load, stat, status, _, _, _ = eng.frr_link_loads(on(csr), nh, backup, dsts, rows, srcs, w, scen)
    assert not stat[:, 2].any()
    u, v = TF.esrc_of(csr), np.asarray(csr.col, np.int64)
    edge = edge_map(csr)
    import torch
    for k, failed in enumerate(scen):
        rowsk = nh.copy()
        down = set(failed)
        for e in failed:
            x, n = int(u[e]), int(v[e])
            hit = np.nonzero(nh[:, x] == n)[0]
            for r in hit.tolist():
                b = int(backup[r, x])
                rowsk[r, x] = b if b >= 0 and edge[(x, b)] not in down else -1
        wk = np.where((status[k] == 1) | (status[k] == 2), w, 0).astype(np.uint64)
        tree = torch.from_numpy(np.ascontiguousarray(rowsk, np.int32)).to(eng.dev)
        want = eng.link_loads(on(csr), tree, EN.INT32, rows, srcs, wk, to_root=True)
        assert np.array_equal(load[k], want), k


# -------------------------------------------------------------- the raw call --

def dev(eng, a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(eng.dev)


def grouped(rows, srcs, w, nrows, V):
    """The pairs in row order as the C call wants them: (order, pair_off, srcs, w)."""
    order, off = EN._pairs_by_row(np.asarray(rows, np.int64), nrows)
    s = np.asarray(srcs, np.int64)[order]
    s = np.where((s < 0) | (s >= V), -1, s)
    return order, off, s, np.asarray(w, np.uint64)[order]


def raw(eng, dsts, nh, backup, off, srcs, w, lists, load, stat=None, status=None, peak=None,
        pedge=None, soff=None):
    """One sdnr_frr_link_loads call on device copies of the arguments (the
    scenario lists as given: not sorted, not deduplicated, not checked), into
    the device tensors given; no synchronize."""
    import torch
    if soff is None:
        soff = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    V = nh.shape[1] if nh.ndim == 2 else 1
    d = np.asarray(dsts, np.int64)
    keep = [dev(eng, np.where((d < 0) | (d >= V), -1, d), np.int32), dev(eng, nh, np.int32),
            dev(eng, backup, np.int32), dev(eng, off, np.int64), dev(eng, srcs, np.int32),
            dev(eng, w, np.uint64), dev(eng, soff, np.int64),
            dev(eng, [e for x in lists for e in x] + [0], np.int32)]
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr() if t is not None else 0     # noqa: E731
    eng.ctx.frr_link_loads_device(
        keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), len(dsts), keep[3].data_ptr(),
        keep[4].data_ptr(), keep[5].data_ptr(), len(soff) - 1, keep[6].data_ptr(),
        keep[7].data_ptr(), p(load), p(stat), p(status), p(peak), p(pedge))
    return keep


def outputs(eng, nscen, E, n, fill=0):
    import torch
    mk = lambda shape, dt, x: torch.full(shape, x, dtype=dt, device=eng.dev)   # noqa: E731
    return (mk((nscen, max(E, 1)), torch.int64, fill), mk((nscen, 4), torch.int64, fill),
            mk((nscen, max(n, 1)), torch.uint8, 9 if fill else 0),
            mk((max(nscen, 1),), torch.int64, fill), mk((max(nscen, 1),), torch.int32, fill))


def host_of(t, E=None, n=None):
    load, stat, status, peak, pedge = t
    return (load.cpu().numpy().view(np.uint64)[:, :E], stat.cpu().numpy().view(np.uint64),
            status.cpu().numpy()[:, :n], peak.cpu().numpy().view(np.uint64), pedge.cpu().numpy())


def test_outputs_add_or_write_optional_ones_and_empty_calls(eng):
    import torch
    csr, nh, backup, (dsts, rows, srcs, w), lists, _, _ = small_case("fat_tree_k4")
    V, E, n, nrows = int(csr.V), int(csr.E), len(rows), len(dsts)
    scen = lists["switches"][:5] + lists["cables"][:4] + [[]]
    want = EN.frr_link_loads_host(csr, nh, backup, dsts, rows, srcs, w, scen)
    order, off, s, ww = grouped(rows, srcs, w, nrows, V)
    eng.load(on(csr))
    K = len(scen)
    FILL = 7

    def expect(got, filled, skip=()):
        gl, gs, gst, gp, ge = host_of(got, E, n)
        add = np.uint64(FILL if filled else 0)
        if "load" not in skip:
            assert np.array_equal(gl, want[0] + add)       # ADDED
        if "stat" not in skip:
            assert np.array_equal(gs, want[1] + add)       # ADDED
        if "status" not in skip:
            assert np.array_equal(gst[:, np.argsort(order)] if not isinstance(order, slice)
                                  else gst, want[2])        # WRITTEN
        if "peak" not in skip:
            full = want[0] + add
            pk, pe = TF.peaks_of(full)
            assert np.array_equal(gp, pk) and np.array_equal(ge, pe)   # WRITTEN, from load

    out = outputs(eng, K, E, n, FILL)
    keep = raw(eng, dsts, nh, backup, off, s, ww, scen, *out)
    eng.ctx.synchronize()
    expect(out, True)
    assert eng.ctx.last_frr_items() == want[5]
    # one optional output NULL at a time
    for drop in ("stat", "status", "peak"):
        out = list(outputs(eng, K, E, n))
        args = list(out)
        if drop == "stat":
            args[1] = None
        elif drop == "status":
            args[2] = None
        else:
            args[3] = args[4] = None
        keep = raw(eng, dsts, nh, backup, off, s, ww, scen, *args)
        eng.ctx.synchronize()
        if drop == "status":
            out[2] = torch.from_numpy(want[2][:, order] if not isinstance(order, slice)
                                      else want[2]).to(eng.dev)
        if drop == "stat":
            assert not out[1].any()
        if drop == "peak":
            assert not out[3].any() and not out[4].any()
        expect(out, False, skip=(drop,))
    # peak without peak_edge: refused, nothing touched
    out = outputs(eng, K, E, n, FILL)
    with pytest.raises(_native.SdnrError) as ei:
        raw(eng, dsts, nh, backup, off, s, ww, scen, out[0], out[1], out[2], out[3], None)
    assert ei.value.code == -22
    eng.ctx.synchronize()
    assert all(bool((t == (9 if t.dtype == torch.uint8 else FILL)).all()) for t in out)
    # no scenarios: nothing touched
    out = outputs(eng, 0, E, n, FILL)
    keep = raw(eng, dsts, nh, backup, off, s, ww, [], *out)
    eng.ctx.synchronize()
    assert all(bool((t == (9 if t.dtype == torch.uint8 else FILL)).all()) for t in out)
    assert eng.ctx.last_frr_items() == 0
    # no rows, and rows without a pair: nothing added, the peak is the plane's as it stands
    for case in ("nrows", "pairs"):
        out = outputs(eng, K, E, n, FILL)
        out[0][1, 5] = 40
        if case == "nrows":
            keep = raw(eng, dsts[:0], nh[:0], backup[:0], [0], s[:0], ww[:0], scen, *out)
        else:
            keep = raw(eng, dsts, nh, backup, np.zeros(nrows + 1, np.int64), s[:0], ww[:0], scen,
                       *out)
        eng.ctx.synchronize()
        gl, gs, gst, gp, ge = host_of(out, E, n)
        assert (gl == FILL).sum() == K * E - 1 and gl[1, 5] == 40
        assert (gs == FILL).all() and (gst == 9).all()
        assert gp.tolist() == [FILL, 40] + [FILL] * (K - 2)
        assert ge.tolist() == [0, 5] + [0] * (K - 2)
        assert eng.ctx.last_frr_items() == 0
    del keep


# ----------------------------------------------------- values written by hand --

def chain_ring(V):
    """A bidirectional ring 0 .. V - 1 whose row toward 0 is the chain x -> x - 1
    (an in-tree of depth V - 1, taken as given): (csr, edge, nh row)."""
    csr = ring_csr(V)
    nh = np.arange(-1, V - 1, dtype=np.int32)
    return csr, nh


def ring_edges(V):
    """Edge ids of ring_csr(V): down[x] = (x -> x - 1), up[x] = (x -> x + 1 mod V)."""
    # row x holds its two neighbours ascending
    down, up = np.zeros(V, np.int64), np.zeros(V, np.int64)
    for x in range(V):
        a, b = (x - 1) % V, (x + 1) % V
        lo, hi = (0, 1) if a < b else (1, 0)
        down[x], up[x] = 2 * x + lo, 2 * x + hi
    return down, up


def ring_expect(V, w, m, what):
    """Toward 0 over the chain, every vertex a source of weight w[x] (w[0] the
    pair 0 -> 0).  With ``m`` the first failed vertex:
      repair  m .. V-1 lose their primary and go up the ring to 0: status 2;
      pingpong  only m loses it and hands to m + 1, whose primary is m: the
              sources m .. V-1 loop (a cycle of two with a tail behind it);
      drop    m + 1 loses it and hands to m + 2 (a repair), m + 2 loses it too
              and has no backup: the sources m + 1 .. V-1 drop at m + 2 or before
    -> (failed edges, backup row, load [E], stat [4], status [V])."""
    down, up = ring_edges(V)
    load = np.zeros(2 * V, np.uint64)
    backup = np.full(V, -1, np.int32)
    status = np.ones(V, np.uint8)
    stat = [0, 0, 0, 0]
    csum = lambda a, b: int(w[a:b].sum(dtype=np.uint64))   # noqa: E731
    if what == "repair":
        failed = [int(down[x]) for x in range(m, V)]
        backup[m:] = (np.arange(m, V) + 1) % V
        for x in range(1, m):
            load[down[x]] = csum(x, m)
        for x in range(m, V):
            load[up[x]] = csum(m, x + 1)
        status[m:] = 2
        stat[0] = csum(m, V)
    elif what == "pingpong":
        failed = [int(down[m])]
        backup[m] = m + 1
        for x in range(1, m):
            load[down[x]] = csum(x, m)
        status[m:] = 4
        stat[2] = csum(m, V)
    else:
        failed = [int(down[m + 1]), int(down[m + 2])]
        backup[m + 1] = m + 2
        for x in range(1, m + 1):
            load[down[x]] = csum(x, m + 1)
        status[m + 1:] = 3
        stat[1] = csum(m + 1, V)
    return sorted(failed), backup, load, np.asarray(stat, np.uint64), status


def check_ring(eng, V, rows_too=False):
    csr, nh = chain_ring(V)
    rng = np.random.default_rng(V)
    w = rng.integers(1, 1 << 40, V, dtype=np.uint64)
    m = V // 2
    cases = [ring_expect(V, w, m, what) for what in ("repair", "pingpong", "drop")]
    got = []
    for failed, backup, load, stat, status in cases:       # one backup row each: one call each
        g = eng.frr_link_loads(on(csr), nh[None, :], backup[None, :], [0], np.zeros(V, np.int64),
                               np.arange(V), w, [failed, []])
        assert np.array_equal(g[0][0], load)
        assert np.array_equal(g[1][0], stat) and np.array_equal(g[2][0], status)
        pk, pe = TF.peaks_of(load[None, :])
        assert g[3][0] == pk[0] and g[4][0] == pe[0] and g[5] == 1
        # the empty scenario beside it: the chain
        down, _ = ring_edges(V)
        base = np.zeros(2 * V, np.uint64)
        for x in range(1, V):
            base[down[x]] = w[x:].sum(dtype=np.uint64)
        assert np.array_equal(g[0][1], base) and not g[1][1].any() and (g[2][1] == 1).all()
        got.append(g)
    return got


@pytest.mark.parametrize("V", [63, 64, 65])
def test_rings_around_a_wavefront_by_hand(eng, V):
    check_ring(eng, V)


def test_wheel_with_hand_made_backups(eng):
    """Hub 0 and a rim 1 .. 65 (130 cables).  Toward rim vertex 1 every switch
    forwards to the hub, the hub to 1, and 2 straight to 1."""
    rim = 65
    und = [(0, v) for v in range(1, rim + 1)] + [(v, v % rim + 1) for v in range(1, rim + 1)]
    csr = digraph_csr(both_ways(und))
    V, E = rim + 1, int(csr.E)
    assert E == 260
    edge = edge_map(csr)
    nh = np.zeros(V, np.int32)
    nh[0], nh[1], nh[2] = 1, -1, 1
    w = np.random.default_rng(rim).integers(1, 1 << 40, V, dtype=np.uint64)
    tot = lambda idx: int(w[idx].sum(dtype=np.uint64))     # noqa: E731
    via_hub = [0] + list(range(3, V))

    def run(backup, failed):
        g = eng.frr_link_loads(on(csr), nh[None, :], np.asarray([backup], np.int32), [1],
                               np.zeros(V, np.int64), np.arange(V), w, [sorted(failed)])
        return g[0][0], g[1][0].tolist(), g[2][0]

    none = np.full(V, -1, np.int32)
    # the hub's link to 1 fails and the hub repairs over 2
    b = none.copy()
    b[0] = 2
    load, stat, status = run(b, [edge[(0, 1)]])
    want = np.zeros(E, np.uint64)
    for v in range(3, V):
        want[edge[(v, 0)]] = w[v]
    want[edge[(0, 2)]] = tot(via_hub)
    want[edge[(2, 1)]] = tot(via_hub) + int(w[2])
    assert np.array_equal(load, want) and stat == [tot(via_hub), 0, 0, 0]
    assert status.tolist() == [2, 1, 1] + [2] * (V - 3)
    # the hub hands to 5, 5 lost its link to the hub and hands to 6, 6 forwards
    # to the hub: a cycle of three, every other switch behind it
    b = none.copy()
    b[0], b[5] = 5, 6
    load, stat, status = run(b, [edge[(0, 1)], edge[(5, 0)]])
    want = np.zeros(E, np.uint64)
    want[edge[(2, 1)]] = w[2]
    assert np.array_equal(load, want) and stat == [0, 0, tot(via_hub), 0]
    assert status.tolist() == [4, 1, 1] + [4] * (V - 3)
    # ... and 5 has no backup: everything behind the hub drops at 5
    b = none.copy()
    b[0] = 5
    load, stat, status = run(b, [edge[(0, 1)], edge[(5, 0)]])
    assert np.array_equal(load, want) and stat == [0, tot(via_hub), 0, 0]
    assert status.tolist() == [3, 1, 1] + [3] * (V - 3)


def test_the_cap_and_one_vertex_above_it(eng):
    import torch
    V = EN.FRR_MAX_V
    got = check_ring(eng, V)
    assert eng.ctx.last_kernel() == KERNEL
    assert all(g[5] == 1 for g in got)
    # above the cap: refused before anything is read, the outputs untouched
    csr, nh = chain_ring(V + 1)
    with pytest.raises(ValueError):
        eng.frr_link_loads(on(csr), nh[None, :], nh[None, :], [0], [0], [1], None, [[0]])
    eng.load(on(csr))
    out = outputs(eng, 1, 2 * (V + 1), 1, 7)
    with pytest.raises(_native.SdnrError) as ei:
        raw(eng, [0], nh[None, :], nh[None, :], [0, 1], [1], [1], [[0]], *out)
    assert ei.value.code == -22 and str(V) in str(ei.value)
    eng.ctx.synchronize()
    assert all(bool((t == (9 if t.dtype == torch.uint8 else 7)).all()) for t in out)


# -------------------------------------------------- more items than workgroups --

def test_more_rows_and_items_than_workgroups(eng):
    """The base pass gives workgroup b the rows b, b + grid, ..., the item
    kernel the listed items b, b + grid, ... (in the order the pre-pass listed
    them, which differs from run to run).  Rows: over_grid's mix, skipped
    kinds between working rows at every candidate grid, a workgroup's
    consecutive rows toward different destinations; items: more than two per
    workgroup."""
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    csr, comp = OG.graph()
    V = int(csr.V)
    n = OG.units(cus)
    strides = OG.strides_for(cus, n)
    m = OG.row_mix(csr, comp, n, 921, strides, bad_dst=True)
    cost = random_costs(csr, 1, 5, 900)
    nh1, bk1 = TF.tables(csr, cost)
    at = np.where((m.dst >= 0) & (m.dst < V), m.dst, 0)
    nh, backup = nh1[at], bk1[at].copy()
    # backups are taken as given: a third of them any neighbour at all -- loops
    rng = np.random.default_rng(922)
    rp, deg = np.asarray(csr.row_ptr, np.int64), np.diff(csr.row_ptr)
    rr, xx = np.nonzero((nh >= 0) & (rng.random(nh.shape) < 0.3))
    backup[rr, xx] = np.asarray(csr.col)[rp[xx] + rng.integers(0, 1 << 30, xx.shape[0]) % deg[xx]]
    victim = int(np.bincount(m.dst[m.kind == OG.WORK]).argmax())
    scen = OG.failure_scenarios(csr, victim)
    scen += TF.scenario_lists(csr)["cables"][:6]
    want = EN.frr_link_loads_host(csr, nh, backup, m.dst, m.rows, m.ends, m.w, scen)
    got = eng.frr_link_loads(on(csr), nh, backup, m.dst, m.rows, m.ends, m.w, scen)
    assert eng.ctx.last_kernel() == KERNEL
    grid = eng.ctx.last_grid()
    assert grid > 0 and n >= 2 * grid + 1 and want[5] >= 2 * grid + 1, (n, want[5], grid)
    OG.check_units(m.kind, m.key, grid)
    same(got, want)
    assert set(np.unique(want[2]).tolist()) == {0, 1, 2, 3, 4}


# ---------------------------------------------------------------- data errors --

def test_data_errors_are_reported_and_contained(eng):
    """Bad INPUT, each kind once: every loop of the kernels is bounded, so none
    of these can hang.  Each is SDNR_ERR_INVAL at the synchronize, the failing
    row / item / scenario adds nothing of its own, the others are exact, and
    the next call is clean."""
    csr, nh, backup, (dsts, rows, srcs, w), lists, _, _ = small_case("fat_tree_k4")
    V, E, n, nrows = int(csr.V), int(csr.E), len(rows), len(dsts)
    u, v = TF.esrc_of(csr), np.asarray(csr.col, np.int64)
    scen = lists["switches"][:4] + lists["cables"][:6] + [[]]
    K = len(scen)
    order, off, s, ww = grouped(rows, srcs, w, nrows, V)
    inv = np.argsort(order)
    eng.load(on(csr))

    def host(keep_pairs=None, scenarios=scen, nh_=nh, bk_=backup):
        """The restatement over the pairs kept; the others read status 0 and
        count for nothing."""
        if keep_pairs is None:
            keep_pairs = np.ones(n, bool)
        r = EN.frr_link_loads_host(csr, nh_, bk_, dsts, rows[keep_pairs], srcs[keep_pairs],
                                   w[keep_pairs], scenarios)
        status = np.zeros((len(scenarios), n), np.uint8)
        status[:, keep_pairs] = r[2]
        return r[0], r[1], status

    def call(nh_=nh, bk_=backup, off_=off, lists_=scen, soff=None):
        k = len(lists_) if soff is None else len(soff) - 1
        out = outputs(eng, k, E, n)
        keep = raw(eng, dsts, nh_, bk_, off_, s, ww, lists_, *out, soff=soff)
        with pytest.raises(_native.SdnrError) as ei:
            eng.ctx.synchronize()
        assert ei.value.code == -22 and "sdnr_frr_link_loads" in str(ei.value)
        eng.ctx.synchronize()                              # reported once
        del keep
        gl, gs, gst, gp, ge = host_of(out, E, n)
        pk, pe = TF.peaks_of(gl)
        assert np.array_equal(gp, pk) and np.array_equal(ge, pe)
        return gl, gs, gst[:, inv]

    def clean():
        got = eng.frr_link_loads(on(csr), nh, backup, dsts, rows, srcs, w, scen)
        same(got[:3], host())

    def expect(got, want):
        for g, x, what in zip(got, want, NAMES):
            assert np.array_equal(g, x), what

    # an nh row with a cycle, one with an entry that is no vertex, one whose
    # link the graph lacks under a vertex that carries demand
    for r, kind in ((3, "cycle"), (7, "vertex"), (11, "link")):
        bad = nh.copy()
        x = int(np.nonzero(nh[r] >= 0)[0][0])
        y = int(nh[r, x])
        if kind == "cycle":
            bad[r, y] = x                                  # x -> y -> x
        elif kind == "vertex":
            bad[r, x] = V + 2
        else:
            far = [z for z in range(V) if z != x and (x, z) not in edge_map(csr)]
            bad[r, x] = far[0]
        expect(call(nh_=bad), host(rows != r))
        clean()
    # a backup that is no out-neighbour: the items that use it keep the row's base
    r = 5
    x = int(np.nonzero(backup[r] >= 0)[0][0])
    prim = edge_map(csr)[(x, int(nh[r, x]))]
    far = [z for z in range(V) if z != x and (x, z) not in edge_map(csr)]
    use = [[prim]] + scen
    for wrong in (far[0], V + 1, -2):
        bad = backup.copy()
        bad[r, x] = wrong
        got = call(bk_=bad, lists_=use)
        rest, mine = host(rows != r, use), host(rows == r, [[]])
        full = host(scenarios=use)
        for k, failed in enumerate(use):
            if prim in failed:
                assert np.array_equal(got[0][k], rest[0][k] + mine[0][0])
                assert np.array_equal(got[1][k], rest[1][k] + mine[1][0])
                assert np.array_equal(got[2][k], rest[2][k] + mine[2][0])
            else:
                assert all(np.array_equal(g[k], f[k]) for g, f in zip(got, full))
        clean()
    # pair offsets outside the pair list: the two rows they spoil add nothing
    r = 9
    off2 = off.copy()
    off2[r + 1] = off[-1] + 7
    expect(call(off_=off2), host((rows != r) & (rows != r + 1)))
    clean()
    # scenario offsets outside the list: the two scenarios they spoil are empty
    soff = np.concatenate([[0], np.cumsum([len(x) for x in scen])])
    soff2 = soff.copy()
    soff2[3] = soff[-1] + 5
    spoiled = [sc if k not in (2, 3) else [] for k, sc in enumerate(scen)]
    expect(call(soff=soff2), host(scenarios=spoiled))
    clean()
    # a scenario that does not ascend is taken as empty
    worst = max(range(K), key=lambda k: len(scen[k]))
    lists2 = [list(sc) for sc in scen]
    lists2[worst] = lists2[worst][::-1]
    spoiled = [sc if k != worst else [] for k, sc in enumerate(scen)]
    expect(call(lists_=lists2), host(scenarios=spoiled))
    clean()
    # an index outside [0, E) is ignored
    for extra in ([-3], [E], [E + 9]):
        lists2 = [list(sc) for sc in scen]
        lists2[1] = sorted(lists2[1] + extra)
        expect(call(lists_=lists2), host())
        clean()


# ------------------------------------------------------------------ the drop-in --

@pytest.mark.parametrize("name", ["fat_tree_k4", "dragonfly_a4_h2_p2"])
def test_dropin_on_the_gpu_equals_the_dropin_over_the_double(name):
    fake, pairs, weights, failures = TF.dropin_case(name)
    g = G.Golden(name)
    db = g.fabric().populate(TopologyDB())
    db.set_link_costs(dict(fake._link_costs))
    for node_protect in (True, False):
        want = fake.frr_link_loads(failures, pairs, weights, node_protect=node_protect)
        got = db.frr_link_loads(failures, pairs, weights, node_protect=node_protect)
        assert got.scenarios == want.scenarios
        for k in range(len(failures)):
            assert got.scenario(k).as_dict() == want.scenario(k).as_dict()
        for what in ("repaired", "dropped", "looped", "unrouted", "peak", "load"):
            assert np.array_equal(getattr(got, what), getattr(want, what)), what
        assert got.peak_link == want.peak_link and got.items == want.items
        assert got.base.as_dict() == want.base.as_dict()
    bare = db.all_pairs_frr_link_loads(failures, planes=False)
    full = fake.all_pairs_frr_link_loads(failures)
    assert bare.load is None and np.array_equal(bare.peak, full.peak)
    assert np.array_equal(bare.dropped, full.dropped) and bare.items == full.items
