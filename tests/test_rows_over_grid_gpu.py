"""The row-persistent kernels with more units of work than workgroups: every
kernel of loads.hip, ecmp_loads.hip, cost_ecmp_loads.hip, cost_tables.hip,
widest_tables.hip, failure_loads.hip, whatif_loads.hip, lfa_tables.hip,
fair_rates.hip, ecmp_fair_rates.hip, multicast.hip and the counts of ecmp.hip
loops `for (r = blockIdx.x; r < n; r += gridDim.x)` over rows (batches, items,
groups) and keeps a row's state in LDS or a scratch slice that the next row
reuses.  Here a workgroup takes two or three units (over_grid.units), the
units of one workgroup differ, and every unit a kernel skips early sits
between two it works on; sdnr_last_grid proves it for the launch made.

Every output is compared with the host restatement of engine.py by the
comparison helper of the kernel's own test module: integers bit for bit, the
f64 loads within RTOL = 1e-9 (a load word sums at most a few thousand
non-negative terms: rounding in any order stays below n * 2^-53, about 1e-12)
with exact zeros.  The rates of sdnr_ecmp_fair_rates are held to the same RTOL,
not to test_ecmp_fair_rates.TOL, which is a measurement over that file's cases.

Graph: over_grid.graph(), 44 vertices in a component of 32, one of 4 and 8
single ones.  The global-scratch forms run on jellyfish(10002, 6): 16 distinct
table rows repeated on the device; their reference is the restatement over the
16 rows with every pair moved to its row's original -- the same sums, as
test_over_grid.py checks for the restatements."""
import types

import numpy as np
import pytest

import over_grid as OG
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from test_cost_ecmp_loads import pcost_rows, random_costs
from test_ecmp_link_loads import RTOL, SPLITS, close
from test_fair_rates import CAPS
from test_multicast_trees import same as same_groups

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def fab(cus):
    """The 44-vertex graph, its tables of every vertex (oracle / restatement)
    and the unit count, computed once."""
    from oracle import oracle as O
    csr, comp = OG.graph()
    ids = np.arange(csr.V, dtype=np.int32)
    par, prt, _ = O.dfs_tables(csr, ids)
    dist, nh, _ = O.dest_tables(csr, ids)
    cost = random_costs(csr, 1, 5, 900)
    n = OG.units(cus)
    return types.SimpleNamespace(
        csr=csr, comp=comp, V=int(csr.V), E=int(csr.E), ex=types.SimpleNamespace(csr=csr),
        par=par, prt=prt, dist=dist, nh=nh, cost=cost, pcost=pcost_rows(csr, cost, ids),
        hops=pcost_rows(csr, np.ones(int(csr.E), np.uint32), ids),
        n=n, strides=OG.strides_for(cus, n))


def dev(eng, a):
    """A numpy table as the device plane the engine keeps (u16 / u32 words in
    int16 / int32 tensors)."""
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
            np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(eng.dev)


def over_grid(eng, kind, key, kernel, launches=1):
    """The launch just made took more than two units per workgroup, of the
    form named, and the mix holds what it must at that grid."""
    c = eng.ctx
    assert c.last_kernel() == kernel
    assert c.last_launches() == launches
    grid = c.last_grid()
    assert grid > 0 and len(kind) >= 2 * grid + 1, (len(kind), grid)
    OG.check_units(kind, key, grid)
    return grid


# ------------------------------------------------- one test per kernel family --

def test_link_loads_all_layouts_and_next_hop_rows(eng, fab):
    m = OG.row_mix(fab.csr, fab.comp, fab.n, 901, fab.strides)
    for lay in (EN.INT32, EN.PORT16, EN.SLOT):
        tab = fab.par if lay == EN.INT32 else EN.pack_host_tree(fab.par, fab.prt, fab.csr, lay)
        tree = tab[m.dst]
        want = EN.link_loads_host(fab.csr, tree, lay, m.rows, m.ends, m.w)
        got = eng.link_loads(fab.ex, dev(eng, tree), lay, m.rows, m.ends, m.w)
        over_grid(eng, m.kind, m.key, "link_loads_kernel<lds>")
        assert want.any() and got.dtype == np.uint64 and np.array_equal(got, want), lay
    tree = fab.nh[m.dst]
    want = EN.link_loads_host(fab.csr, tree, EN.INT32, m.rows, m.ends, m.w, True)
    got = eng.link_loads(fab.ex, dev(eng, tree), EN.INT32, m.rows, m.ends, m.w, to_root=True)
    over_grid(eng, m.kind, m.key, "link_loads_kernel<lds>")
    assert want.any() and np.array_equal(got, want)


def test_ecmp_link_loads_both_splits(eng, fab):
    m = OG.row_mix(fab.csr, fab.comp, fab.n, 902, fab.strides)
    dist = fab.dist[m.dst]
    d_dist = dev(eng, dist)
    for split in SPLITS:
        want = EN.ecmp_link_loads_host(fab.csr, dist, m.rows, m.ends, m.w, split)
        got = eng.ecmp_link_loads(fab.ex, d_dist, m.rows, m.ends, m.w, split)
        over_grid(eng, m.kind, m.key, "ecmp_loads_kernel<lds>")
        assert want.any() and got.dtype == np.float64 and close(got, want), split


def test_cost_ecmp_link_loads_both_splits(eng, fab):
    m = OG.row_mix(fab.csr, fab.comp, fab.n, 903, fab.strides)
    pcost = fab.pcost[m.dst]
    d_pc = dev(eng, pcost)
    for split in SPLITS:
        want = EN.cost_ecmp_link_loads_host(fab.csr, fab.cost, pcost, m.rows, m.ends, m.w, split)
        got = eng.cost_ecmp_link_loads(fab.ex, fab.cost, d_pc, m.rows, m.ends, m.w, split)
        over_grid(eng, m.kind, m.key, "cost_ecmp_loads_kernel<lds>")
        assert want.any() and got.dtype == np.float64 and close(got, want), split


def rows_of(tables, dsts, V):
    """Per-destination tables for a list with repeats: ``tables`` are the
    restatement's rows of the destinations 0 .. V - 1 and then of one id that
    is no vertex (the empty row); a row depends on its destination alone."""
    at = np.where((dsts >= 0) & (dsts < V), dsts, V)
    return tuple(t[at] for t in tables)


def test_cost_tables_batches_of_eight(eng, fab):
    B = 8
    dsts, kind = OG.dest_mix(fab.csr, fab.n, B, 904, fab.strides)
    assert (dsts.shape[0] + B - 1) // B == fab.n and dsts.shape[0] % B
    one = EN.cost_tables_host(fab.csr, fab.cost, np.arange(fab.V + 1))
    want = rows_of(one, dsts, fab.V)
    got = eng.cost_tables(fab.ex, fab.cost, dsts)
    over_grid(eng, kind, OG.batch_keys(dsts, B), "cost_tables_kernel<lds,8>")
    for g, w, what in zip(got, want, ("pcost", "nh", "nh_port")):
        g = EN._host(g)
        g = g.view(np.uint32) if what == "pcost" else g
        assert g.dtype == w.dtype and np.array_equal(g, w), what


def test_widest_tables_batches_of_six(eng, fab):
    B = 6
    dsts, kind = OG.dest_mix(fab.csr, fab.n, B, 905, fab.strides)
    assert (dsts.shape[0] + B - 1) // B == fab.n and dsts.shape[0] % B
    util = np.random.default_rng(906).integers(0, 50, fab.E).astype(np.uint32)
    every = np.arange(fab.V + 1)
    pc_one = EN.cost_tables_host(fab.csr, fab.cost, every)[0]
    one = EN.widest_tables_host(fab.csr, fab.cost, pc_one, util, every)
    want = rows_of(one, dsts, fab.V)
    pcost = rows_of((pc_one,), dsts, fab.V)[0]
    got = eng.widest_tables(fab.ex, fab.cost, pcost, util, dsts)
    over_grid(eng, kind, OG.batch_keys(dsts, B), "widest_tables_kernel<lds,6>")
    for g, w, what in zip(got, want, ("bott", "nh", "nh_port")):
        g = EN._host(g)
        g = g.view(np.uint32) if what == "bott" else g
        assert g.dtype == w.dtype and np.array_equal(g, w), what


def item_mix(fab, cus, seed):
    """Rows and four failure scenarios for at least fab.n (scenario, row)
    items: item k * nrows + r.  A workgroup's next item is ``grid`` further:
    another row, and past the end of a scenario another scenario too.  Returns
    (mix, victim, the kinds and keys of the items)."""
    nrows = (fab.n + 3) // 4
    grids = OG.strides_for(cus, fab.n)
    folded = sorted({s for g in grids for s in (g % nrows, nrows - g % nrows) if s})
    plant = tuple(s for s in folded if 2 * s + 64 < nrows)
    m = OG.row_mix(fab.csr, fab.comp, nrows, seed, plant, bad_dst=True, distinct=folded)
    victim = int(np.bincount(m.dst[m.kind == OG.WORK]).argmax())
    kind = np.tile(m.kind, 4)
    key = np.stack([np.tile(m.key, 4), np.repeat(np.arange(4), nrows)], 1)
    return m, victim, kind, key


def test_failure_loads_items(eng, fab, cus):
    from test_failure_loads_gpu import same
    m, victim, kind, key = item_mix(fab, cus, 907)
    scen = OG.failure_scenarios(fab.csr, victim)
    for split in SPLITS:
        want = EN.failure_ecmp_link_loads_host(fab.csr, fab.cost, m.dst, m.rows, m.ends, m.w,
                                               scen, split)
        got = eng.failure_ecmp_link_loads(fab.ex, fab.cost, m.dst, m.rows, m.ends, m.w, scen,
                                          split)
        over_grid(eng, kind, key, "failure_ecmp_loads_kernel<lds>")
        same(got, want)
        for k, failed in enumerate(scen):
            assert not got[0][k][failed].any()
        assert want[0].any(axis=1).all() and want[1][3] > want[1][0] > 0
        assert want[2].any() and not want[2].all()


def test_whatif_loads_items(eng, fab, cus):
    from test_whatif_loads_gpu import same
    m, victim, kind, key = item_mix(fab, cus, 908)
    none, cable, switch, cut = OG.failure_scenarios(fab.csr, victim)
    inf = EN.COST_INF
    scen = [([], []), (cable, [inf] * len(cable)), (switch, [3 * int(fab.cost[e]) for e in switch]),
            (cut, [inf] * len(cut))]
    for split in SPLITS:
        want = EN.whatif_ecmp_link_loads_host(fab.csr, fab.cost, m.dst, m.rows, m.ends, m.w, scen,
                                              split, None)
        got = eng.whatif_ecmp_link_loads(fab.ex, fab.cost, m.dst, m.rows, m.ends, m.w, scen,
                                         split, None)
        over_grid(eng, kind, key, "whatif_ecmp_loads_kernel<lds>")
        same(got, want)
        assert not got[0][1][cable].any() and not got[0][3][cut].any()
        assert want[0].any(axis=1).all() and want[1][3] > want[1][0] > 0
        assert not np.array_equal(want[0][2], want[0][0])


def test_lfa_tables_rows(eng, fab):
    from test_lfa_tables_gpu import same
    dsts, kind = OG.dest_mix(fab.csr, fab.n, 1, 909, fab.strides, p_bad=0.05)
    assert dsts.shape[0] == fab.n
    P = fab.pcost
    every = np.arange(fab.V + 1)
    for link_only, kernel in ((False, "lfa_tables_kernel<node>"),
                              (True, "lfa_tables_kernel<link>")):
        one = EN.lfa_tables_host(fab.csr, fab.cost, P, every, link_only)
        want = rows_of(one, dsts, fab.V)
        got = eng.lfa_tables(fab.ex, fab.cost, P, dsts, link_only=link_only)
        over_grid(eng, kind, dsts, kernel)
        same(got, want)
        assert (want[2] != 0).any() and want[3].any()


def fair_launches(rounds, flows, ncap):
    """One launch to start, two per round; the rounds are queued 16 at a time,
    up to the closing round after max_rounds = min(flows, E + nextra)."""
    return 1 + 2 * min(16 * (rounds // 16 + 1), min(flows, ncap) + 1)


def test_fair_rates_rows(eng, fab):
    from test_fair_rates_gpu import same
    m = OG.row_mix(fab.csr, fab.comp, fab.n, 910, fab.strides)
    cap = np.random.default_rng(911).choice(np.asarray(CAPS, np.float64), fab.E)
    for tab, to_root in ((fab.par, False), (fab.nh, True)):
        tree = tab[m.dst]
        want = EN.fair_rates_host(fab.csr, tree, EN.INT32, m.rows, m.ends, m.w, cap, None,
                                  to_root)
        got = eng.fair_rates(fab.ex, dev(eng, tree), EN.INT32, m.rows, m.ends, m.w, cap,
                             to_root=to_root)
        over_grid(eng, m.kind, m.key, "fair_rows_kernel<lds>",
                  fair_launches(len(want[3]), len(m.rows), fab.E))
        same(got, want)
        assert len(want[3]) > 1 and (want[2] >= 0).any() and (want[2] < 0).any()


def close_rates(got, want):
    """rate, bott, round, level, used: equal rounds, round and bott, the
    doubles within RTOL (+inf equal)."""
    for g, w, name in zip(got, want, ("rate", "bott", "round", "level", "used")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if g.dtype != np.float64:
            assert np.array_equal(g, w), name
        else:
            assert np.array_equal(g == 0, w == 0), name
            assert np.allclose(g, w, rtol=RTOL, atol=0), name


def test_ecmp_fair_rates_rows(eng, fab):
    m = OG.row_mix(fab.csr, fab.comp, fab.n, 912, fab.strides)
    cap = np.random.default_rng(913).choice(np.asarray(CAPS, np.float64), fab.E)
    for cost, tab, split in ((None, fab.hops, "route"), (fab.cost, fab.pcost, "hop")):
        pcost = tab[m.dst]
        want = EN.ecmp_fair_rates_host(fab.csr, cost, pcost, m.rows, m.ends, m.w, cap, None,
                                       split)
        got = eng.ecmp_fair_rates(fab.ex, cost, dev(eng, pcost), m.rows, m.ends, m.w, cap, None,
                                  split)
        over_grid(eng, m.kind, m.key, "ecmp_fair_rows_kernel<lds>",
                  fair_launches(len(want[3]), len(m.rows), fab.E))
        close_rates(got, want)
        assert len(want[3]) > 1 and (want[2] >= 0).any() and (want[2] < 0).any()


def test_multicast_groups_all_layouts_and_next_hop_rows(eng, fab):
    m = OG.group_mix(fab.csr, fab.comp, fab.n, 914, fab.strides)
    batch = (m.root, m.mem_off, m.mem_row, m.mem_vertex)
    for lay in (EN.INT32, EN.PORT16, EN.SLOT):
        tab = fab.par if lay == EN.INT32 else EN.pack_host_tree(fab.par, fab.prt, fab.csr, lay)
        want = EN.multicast_trees_host(fab.csr, tab, lay, *batch, weights=m.w)
        got = eng.multicast_trees(fab.ex, dev(eng, tab), lay, *batch, weights=m.w)
        over_grid(eng, m.kind, m.key, "multicast_trees_kernel<lds>")
        assert same_groups(got, want), lay
        assert want[0].any() and not want[0].all() and want[2].size and want[3].any()
    d = OG.group_mix(fab.csr, fab.comp, fab.n, 915, fab.strides, to_root=True)
    batch = (d.root, d.mem_off, d.mem_row, d.mem_vertex)
    want = EN.multicast_trees_host(fab.csr, fab.nh, EN.INT32, *batch, weights=d.w, to_root=True)
    got = eng.multicast_trees(fab.ex, dev(eng, fab.nh), EN.INT32, *batch, weights=d.w,
                              to_root=True)
    over_grid(eng, d.kind, d.key, "multicast_trees_kernel<lds>")
    assert same_groups(got, want) and want[0].any() and want[2].size


def wheel_csr(rim):
    """A hub joined to ``rim`` vertices on a ring: the hub's out-degree is
    above 64, so no 64-wide rows are uploaded and the counts run in
    ecmp_count_kernel.  A square beside it is a second component, so the
    reached set changes from row to row here too."""
    r = np.arange(rim)
    q = rim + 1 + np.arange(4)
    a = np.concatenate([np.zeros(rim, np.int64), r + 1, q])
    b = np.concatenate([r + 1, (r + 1) % rim + 1, np.roll(q, -1)])
    s, d = np.concatenate([a, b]) + 1, np.concatenate([b, a]) + 1
    return T.build_csr(s, d, np.arange(s.shape[0]) % 90 + 1)


@pytest.mark.parametrize("form", ["rows", "global", "lds"])
def test_ecmp_counts_rows(eng, fab, cus, monkeypatch, form):
    """The three count kernels of ecmp.hip (8, 4 and 2 workgroups per CU)
    against the exact level DP of test_small_kernels_gpu.py."""
    from oracle import oracle as O
    from test_small_kernels_gpu import clipped, exact_counts
    if form == "global":
        monkeypatch.setenv("SDNROUTE_ECMP", "global")
    if form == "lds":
        csr = wheel_csr(70)
        assert csr.max_degree() == 70
        ex = types.SimpleNamespace(csr=csr)
        dist = O.dest_tables(csr, np.arange(csr.V, dtype=np.int32))[0]
    else:
        csr, ex, dist = fab.csr, fab.ex, fab.dist
    kernel = {"rows": "ecmp_count_rows_kernel<stage>", "global": "ecmp_count_global_kernel",
              "lds": "ecmp_count_kernel"}[form]
    n = OG.units(cus, 8)
    pick = OG.repeat_rows(n, int(csr.V), 916, OG.strides_for(cus, n))
    one = clipped(exact_counts(csr, dist))
    assert one.max() > 1
    eng.load(ex)
    got = eng.ctx.ecmp_counts(dist[pick])
    grid = over_grid(eng, np.full(n, OG.WORK), pick, kernel)
    assert grid == cus * {"rows": 8, "global": 4, "lds": 2}[form]
    assert got.dtype == np.uint64 and np.array_equal(got, one[pick])


# --------------------------------------------------------- dyadic, bit for bit --

def test_fat_tree_dyadic_loads_over_the_grid_are_bit_exact(eng, cus):
    """Between the edge switches of a fat-tree every route count is a power of
    two; with integer weights below 2^20 every share and every partial sum is
    exact in any order of the atomics (the expected values, scaled by 2^12, are
    integers below 2^53), so the repeated rows must come out bit for bit."""
    fabric = T.fat_tree(4)
    csr = fabric.csr()
    ex = types.SimpleNamespace(csr=csr)
    hv = np.unique(fabric.host_table()[0])
    n = OG.units(cus)
    strides = OG.strides_for(cus, n)
    pick = OG.repeat_rows(n, hv.shape[0], 917, strides)
    rng = np.random.default_rng(918)
    rows = np.repeat(np.arange(n), 3)
    srcs = hv[rng.integers(0, hv.shape[0], 3 * n)]
    w = rng.integers(0, 1 << 20, 3 * n, dtype=np.uint64)
    ones = np.ones(int(csr.E), np.uint32)
    dist = EN.cost_tables_host(csr, ones, hv)[0]
    assert dist.max() == 4
    d16, d32 = dist.astype(np.uint16)[pick], dist[pick]
    kind = np.full(n, OG.WORK)
    for split in SPLITS:
        want = EN.ecmp_link_loads_host(csr, d16, rows, srcs, w, split)
        scaled = want * 2.0 ** 12
        assert np.array_equal(scaled, np.floor(scaled)) and scaled.max() < 2.0 ** 53
        assert want.any()
        got = eng.ecmp_link_loads(ex, dev(eng, d16), rows, srcs, w, split)
        over_grid(eng, kind, pick, "ecmp_loads_kernel<lds>")
        assert np.array_equal(got, want), split
        assert np.array_equal(EN.cost_ecmp_link_loads_host(csr, ones, d32, rows, srcs, w, split),
                              want)
        got = eng.cost_ecmp_link_loads(ex, ones, dev(eng, d32), rows, srcs, w, split)
        over_grid(eng, kind, pick, "cost_ecmp_loads_kernel<lds>")
        assert np.array_equal(got, want), split


# ------------------------------------------------------------------ error rows --

def raises_once(eng):
    """The data error of the call just queued is reported by one synchronize
    and not by the next."""
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22
    eng.ctx.synchronize()


def test_link_loads_error_rows_add_nothing_and_the_context_goes_on(eng, fab):
    """Rows whose offsets leave the pair list and rows that are no tree (a
    2-cycle) among working rows: the loads are those of the other rows."""
    from test_link_loads_gpu import as_u64, raw_loads, zeros_u64
    m = OG.row_mix(fab.csr, fab.comp, fab.n, 919, fab.strides, errors=True)
    off, live = OG.bad_offsets(m)
    tree = fab.par[m.dst].copy()
    a, b = 0, int(fab.csr.col[0])
    for r in np.nonzero(m.kind == OG.ERR_ROW)[0]:
        tree[r, a], tree[r, b] = b, a
    want = EN.link_loads_host(fab.csr, fab.par[m.dst], EN.INT32, m.rows[live], m.ends[live],
                              m.w[live])
    ends = np.where((m.ends < 0) | (m.ends >= fab.V), -1, m.ends)
    eng.load(fab.ex)
    load = zeros_u64(eng, fab.E)
    keep = raw_loads(eng, fab.csr, tree, EN.INT32, fab.n, off, ends, m.w, load)
    over_grid(eng, m.effective, m.key, "link_loads_kernel<lds>")
    raises_once(eng)
    assert want.any() and np.array_equal(as_u64(load, fab.E), want)
    got = eng.link_loads(fab.ex, dev(eng, fab.par[m.dst]), EN.INT32, m.rows[live], m.ends[live],
                         m.w[live])
    assert np.array_equal(got, want)
    del keep


def test_ecmp_link_loads_error_rows_add_nothing_and_the_context_goes_on(eng, fab):
    """Rows whose offsets leave the pair list and distance rows with a level
    >= V among working rows."""
    from test_ecmp_link_loads_gpu import raw_ecmp, zeros_f64
    m = OG.row_mix(fab.csr, fab.comp, fab.n, 920, fab.strides, errors=True)
    off, live = OG.bad_offsets(m)
    dist = fab.dist[m.dst].copy()
    for r in np.nonzero(m.kind == OG.ERR_ROW)[0]:
        x = np.nonzero(dist[r] == 1)[0]
        dist[r, x[0] if x.size else (m.dst[r] + 1) % fab.V] = fab.V
    ends = np.where((m.ends < 0) | (m.ends >= fab.V), -1, m.ends)
    eng.load(fab.ex)
    for split in SPLITS:
        want = EN.ecmp_link_loads_host(fab.csr, fab.dist[m.dst], m.rows[live], m.ends[live],
                                       m.w[live], split)
        load = zeros_f64(eng, fab.E)
        keep = raw_ecmp(eng, dist, fab.n, off, ends, m.w, load, hop=split == "hop")
        over_grid(eng, m.effective, m.key, "ecmp_loads_kernel<lds>")
        raises_once(eng)
        assert want.any() and close(load.cpu().numpy()[:fab.E], want), split
        got = eng.ecmp_link_loads(fab.ex, dev(eng, fab.dist[m.dst]), m.rows[live], m.ends[live],
                                  m.w[live], split)
        assert close(got, want), split
        del keep


def test_multicast_error_groups_add_nothing_and_the_context_goes_on(eng, fab):
    """Groups whose offsets leave the member list and groups that walk a row
    of 2-cycles among working groups: counts 0, no entries, no load."""
    from test_multicast_trees_gpu import Raw
    V = fab.V
    m = OG.group_mix(fab.csr, fab.comp, fab.n, 921, fab.strides, errors=True)
    off, dead = OG.break_offsets(m.mem_off, m.kind)
    per = np.diff(m.mem_off)
    grp = np.repeat(np.arange(fab.n), per)
    # row V of the table: x <-> x ^ 1; rows outside the table move up by one
    table = np.concatenate([fab.par, (np.arange(V, dtype=np.int32) ^ 1)[None, :]])
    row = np.where(m.mem_row == V, V + 1, m.mem_row)
    vert = m.mem_vertex.copy()
    for g in np.nonzero(m.kind == OG.ERR_ROW)[0]:
        lo, hi = m.mem_off[g], m.mem_off[g + 1]
        row[lo:hi] = V
        vert[lo] = (m.key[g] + 2) % V                      # neither the root nor its partner
    root = m.root.copy()
    root[m.kind == OG.ERR_ROW] = m.key[m.kind == OG.ERR_ROW]
    # the reference: the groups that count, the others without a member
    live = ~dead[grp]
    ref_off = np.zeros(fab.n + 1, np.int64)
    np.cumsum(np.where(dead, 0, per), out=ref_off[1:])
    want = EN.multicast_trees_host(fab.csr, table, EN.INT32, root, ref_off, row[live], vert[live],
                                   weights=m.w)
    eng.load(fab.ex)
    a = Raw(eng, fab.csr, table, EN.INT32, root, off, row, vert, w=m.w)
    a.call()
    over_grid(eng, m.effective, m.key, "multicast_trees_kernel<lds>")
    raises_once(eng)
    assert np.array_equal(a.cnt.cpu().numpy(), np.diff(want[1]))
    assert np.array_equal(a.reached.cpu().numpy()[:a.nmem][live], want[0])
    assert want[3].any() and np.array_equal(a.loads(), want[3])
    # the fill: the broken offsets again, entries of the groups that count
    edge = a.fill(want[1], want[1][-1])
    raises_once(eng)
    e = edge.cpu().numpy()
    assert np.array_equal(e[:want[1][-1]], want[2]) and (e[want[1][-1]:] == -7).all()
    got = eng.multicast_trees(fab.ex, dev(eng, table), EN.INT32, root, ref_off, row[live],
                              vert[live], weights=m.w)
    assert same_groups(got, want)


# ------------------------------------------------------- global-scratch forms --

@pytest.fixture(scope="module")
def fish(cus):
    """jellyfish(10002, 6): above every LDS bound of loads.hip, ecmp_loads.hip,
    cost_ecmp_loads.hip and cost_tables.hip, levels <= 8; 16 distinct table
    rows (oracle / restatement) and the rows' repeats, computed once."""
    from oracle import oracle as O
    csr = T.jellyfish(10002, 6, seed=2).csr()
    V = int(csr.V)
    assert V > max(EN.COST_LDS_MAX_V, EN.COST_ECMP_LDS_MAX_V, 9000)
    ids = (np.arange(16, dtype=np.int32) * 613 + 5) % V
    par, _, _ = O.dfs_tables(csr, ids)
    dist, _, _ = O.dest_tables(csr, ids)
    assert dist.max() <= 8
    cost = random_costs(csr, 1, 3, 930)
    n = OG.units(cus)
    strides = OG.strides_for(cus, n)
    rng = np.random.default_rng(931)
    ends = rng.integers(0, V, n)
    ends[::17] = rng.choice([-1, V], ends[::17].shape[0])
    return types.SimpleNamespace(
        csr=csr, V=V, E=int(csr.E), ex=types.SimpleNamespace(csr=csr), ids=ids, par=par,
        dist=dist, cost=cost, tables=EN.cost_tables_host(csr, cost, ids), n=n, strides=strides,
        pick=OG.repeat_rows(n, 16, 932, strides), rows=np.arange(n), ends=ends,
        w=OG.rand_weights(rng, n), kind=np.full(n, OG.WORK))


def repeated(eng, table, pick):
    """table[pick] made on the device: [n, V] from the 16 distinct rows."""
    import torch
    return dev(eng, table).index_select(0, torch.from_numpy(pick).to(eng.dev))


def test_global_link_loads(eng, fish):
    f = fish
    want = EN.link_loads_host(f.csr, f.par, EN.INT32, f.pick, f.ends, f.w)
    got = eng.link_loads(f.ex, repeated(eng, f.par, f.pick), EN.INT32, f.rows, f.ends, f.w)
    over_grid(eng, f.kind, f.pick, "link_loads_kernel<global>")
    assert want.any() and np.array_equal(got, want)


def test_global_ecmp_link_loads(eng, fish):
    f = fish
    d_dist = repeated(eng, f.dist, f.pick)
    for split in SPLITS:
        want = EN.ecmp_link_loads_host(f.csr, f.dist, f.pick, f.ends, f.w, split)
        got = eng.ecmp_link_loads(f.ex, d_dist, f.rows, f.ends, f.w, split)
        over_grid(eng, f.kind, f.pick, "ecmp_loads_kernel<global>")
        assert want.any() and close(got, want), split


def test_global_cost_ecmp_link_loads(eng, fish):
    f = fish
    d_pc = repeated(eng, f.tables[0], f.pick)
    for split in SPLITS:
        want = EN.cost_ecmp_link_loads_host(f.csr, f.cost, f.tables[0], f.pick, f.ends, f.w, split)
        got = eng.cost_ecmp_link_loads(f.ex, f.cost, d_pc, f.rows, f.ends, f.w, split)
        over_grid(eng, f.kind, f.pick, "cost_ecmp_loads_kernel<global>")
        assert want.any() and close(got, want), split


def test_global_multicast_next_hop_rows(eng, cus):
    """jellyfish(40000, 6): V + E = 280,000 bits are above the 32 KiB of maps in
    LDS.  Next-hop rows of 16 destinations (walks of at most 10 links, so the
    restatement stays cheap where a first-push tree is thousands deep); the
    roots are drawn over all vertices, the members among the 16."""
    from oracle import oracle as O
    csr = T.jellyfish(40000, 6, seed=3).csr()
    V, E = int(csr.V), int(csr.E)
    assert not EN.multicast_maps_in_lds(V, E)
    ids = (np.arange(16, dtype=np.int32) * 2477 + 11) % V
    dist, nh, _ = O.dest_tables(csr, ids)
    assert dist.max() <= 10
    n = OG.units(cus)
    m = OG.group_mix(csr, None, n, 934, OG.strides_for(cus, n), pool=ids)
    batch = (m.root, m.mem_off, m.mem_row, m.mem_vertex)
    want = EN.multicast_trees_host(csr, nh, EN.INT32, *batch, weights=m.w, to_root=True)
    got = eng.multicast_trees(types.SimpleNamespace(csr=csr), dev(eng, nh), EN.INT32, *batch,
                              weights=m.w, to_root=True)
    over_grid(eng, m.kind, m.key, "multicast_trees_kernel<global>")
    assert same_groups(got, want)
    assert want[0].any() and not want[0].all() and want[2].size and want[3].any()


def test_global_cost_tables_batches_of_four(eng, fish):
    """n batches of 4 destinations drawn from the 16 (and ids that are no
    vertex); the three tables are compared on the device."""
    import torch
    f = fish
    B = 4
    at, kind = OG.dest_mix(types.SimpleNamespace(V=16), f.n, B, 933, f.strides)
    inside = (at >= 0) & (at < 16)
    dsts = np.where(inside, f.ids[np.where(inside, at, 0)], np.where(at < 0, -1, f.V))
    got = eng.cost_tables(f.ex, f.cost, dsts)
    over_grid(eng, kind, OG.batch_keys(dsts, B), "cost_tables_kernel<global,4>")
    idx = torch.from_numpy(np.where(inside, at, 16)).to(eng.dev)
    for g, w, fill, what in zip(got, f.tables, (EN.COST_INF, -1, -1), ("pcost", "nh", "nh_port")):
        w = np.concatenate([w, np.full((1, f.V), fill, w.dtype)])
        assert g.dtype == torch.int32 and torch.equal(g, dev(eng, w).index_select(0, idx)), what
