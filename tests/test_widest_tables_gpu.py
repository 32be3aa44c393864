"""widest_tables.hip (sdnr_widest_tables) on the GPU against
engine.widest_tables_host, and the drop-in's least-loaded routes, loads and
admission against the engine double of test_widest_tables.py.  Everything is
integer: every comparison is array_equal / ==."""
import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import TopologyDB
from test_cost_ecmp_loads import digraph_csr, edge_costs
from test_cost_tables import follow, seeded_costs
from test_cost_tables_gpu import edge, sym_csr
from test_widest_tables import (COST_KINDS, UTIL_HI, UTIL_MAX, dropin_results, fake_db,
                                seeded_util, small_case)

pytestmark = pytest.mark.gpu

INF = EN.COST_INF
NONE = 0xFFFFFFFF
LDS6, LDS4, LDS2, GLOBAL = ("widest_tables_kernel<lds,6>", "widest_tables_kernel<lds,4>",
                            "widest_tables_kernel<lds,2>", "widest_tables_kernel<global,4>")
BATCH = 6                                   # destinations per workgroup on the small fabrics


def form(V):
    """The kernel form widest_tables.hip picks for V vertices (from V alone)."""
    return LDS6 if V <= EN.WIDEST_LDS_B6_MAX_V else LDS4 if V <= EN.WIDEST_LDS_B4_MAX_V else \
        LDS2 if V <= EN.WIDEST_LDS_MAX_V else GLOBAL


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_error_left(ctx):
    """After every case the context reports no error word."""
    yield
    ctx.set_stream(None)
    ctx.synchronize()


def host_tables(csr, cost, util, dsts):
    ones = np.ones(int(csr.E), np.uint32)
    pcost = EN.cost_tables_host(csr, ones if cost is None else cost, dsts)[0]
    return pcost, EN.widest_tables_host(csr, cost, pcost, util, dsts)


def check(ctx, csr, cost, util, dsts, kernel=LDS6, want=None):
    """Upload, compute on the GPU, compare all three tables with the host's.
    ``cost`` None: no costs uploaded, every link costs 1."""
    ctx.upload(csr)
    ctx.set_link_costs(cost)
    dsts = np.asarray(dsts, np.int32)
    if want is None:
        want = host_tables(csr, cost, util, dsts)
    pcost, tabs = want
    got = ctx.widest_tables(pcost, util, dsts)
    for g, w, what in zip(got, tabs, ("bott", "nh", "nh_port")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    assert ctx.last_kernel() == kernel
    assert ctx.last_launches() == 1
    ctx.synchronize()
    return got


def util_of(csr, values, default=0):
    return edge_costs(csr, values, default)


# ------------------------------------------------------ the small fabrics --

@pytest.fixture(scope="module")
def small_cases():
    """Per G.SMALL fabric, cost kind and utilisation range: the host's tables
    of every destination, computed once (the CPU file's seeds)."""
    out = {}
    for name in G.SMALL:
        for kind in COST_KINDS:
            for hi in UTIL_HI:
                csr, cost, util = small_case(name, kind, hi)
                cost = None if kind == "unit" else cost
                dsts = np.arange(csr.V, dtype=np.int32)
                out[(name, kind, hi)] = (csr, cost, util, dsts,
                                         host_tables(csr, cost, util, dsts))
    return out


@pytest.mark.parametrize("hi", UTIL_HI)
@pytest.mark.parametrize("kind", COST_KINDS)
@pytest.mark.parametrize("name", G.SMALL)
def test_small_fabrics_every_destination(ctx, small_cases, name, kind, hi):
    csr, cost, util, dsts, want = small_cases[(name, kind, hi)]
    check(ctx, csr, cost, util, dsts, want=want)
    # a destination count that is no multiple of the batch, and a single one
    n = csr.V - 1 if (csr.V - 1) % BATCH else csr.V - 2
    assert n % BATCH
    cut = lambda a, b: (want[0][a:b], tuple(t[a:b] for t in want[1]))    # noqa: E731
    check(ctx, csr, cost, util, dsts[:n], want=cut(0, n))
    check(ctx, csr, cost, util, dsts[-1:], want=cut(csr.V - 1, csr.V))
    # bottlenecks only
    bott, nh, nhp = ctx.widest_tables(want[0], util, dsts, with_nexthop=False)
    assert nh is None and nhp is None and np.array_equal(bott, want[1][0])


# ------------------------------------------------------------ the tie key --

def two_routes():
    """0 -> 1 -> 3 -> 5 and 0 -> 2 -> 4 -> 5, links one way."""
    return digraph_csr([(0, 1), (1, 3), (3, 5), (0, 2), (2, 4), (4, 5)], 6)


def test_better_bottleneck_beats_the_emptier_first_link(ctx):
    csr = two_routes()
    util = util_of(csr, {(0, 1): 1, (1, 3): 9, (0, 2): 5, (2, 4): 5})
    bott, nh, nhp = check(ctx, csr, None, util, [5])
    assert int(nh[0, 0]) == 2 and int(bott[0, 0]) == 5          # greedy would take 0 -> 1
    assert bott[0].tolist() == [5, 9, 5, 0, 0, 0]
    assert int(nhp[0, 0]) == int(csr.port[edge(csr, 0, 2)])
    assert follow(nh[0], 0, 5, 6) == [0, 2, 4, 5]


def test_equal_bottleneck_first_link_then_neighbour(ctx):
    csr = two_routes()
    # both routes peak at 6 further down: the emptier first link decides
    util = util_of(csr, {(0, 1): 4, (1, 3): 6, (0, 2): 2, (2, 4): 6})
    bott, nh, _ = check(ctx, csr, None, util, [5])
    assert int(nh[0, 0]) == 2 and int(bott[0, 0]) == 6
    util = util_of(csr, {(0, 1): 2, (1, 3): 6, (0, 2): 4, (2, 4): 6})
    bott, nh, _ = check(ctx, csr, None, util, [5])
    assert int(nh[0, 0]) == 1 and int(bott[0, 0]) == 6
    # a full tie: the smaller neighbour, sdnr_cost_tables' rule
    util = util_of(csr, {(0, 1): 3, (1, 3): 6, (0, 2): 3, (4, 5): 6})
    bott, nh, _ = check(ctx, csr, None, util, [5])
    assert int(nh[0, 0]) == 1 and int(bott[0, 0]) == 6


def test_next_hops_at_different_hop_depths(ctx):
    """A direct link of cost 2 ties two links of cost 1."""
    csr = digraph_csr([(0, 1), (1, 2), (0, 2)], 3)
    cost = edge_costs(csr, {(0, 2): 2})
    bott, nh, _ = check(ctx, csr, cost, util_of(csr, {(0, 2): 3, (0, 1): 1, (1, 2): 1}), [2])
    assert int(nh[0, 0]) == 1 and int(bott[0, 0]) == 1
    bott, nh, _ = check(ctx, csr, cost, util_of(csr, {(0, 2): 0, (0, 1): 1, (1, 2): 1}), [2])
    assert int(nh[0, 0]) == 2 and int(bott[0, 0]) == 0
    bott, nh, _ = check(ctx, csr, cost, util_of(csr, {(0, 2): 1, (0, 1): 1, (1, 2): 1}), [2])
    assert int(nh[0, 0]) == 1                                    # full tie: the smaller neighbour


def test_an_empty_detour_that_is_not_tight_stays_unused(ctx):
    csr = digraph_csr([(0, 1), (1, 2), (0, 3), (3, 4), (4, 2)], 5)
    util = util_of(csr, {(0, 1): 9, (1, 2): 9})                  # 0 -> 3 -> 4 -> 2 carries nothing
    bott, nh, _ = check(ctx, csr, None, util, [2])
    assert int(nh[0, 0]) == 1 and int(bott[0, 0]) == 9
    assert int(nh[0, 3]) == 4 and int(bott[0, 3]) == 0


@pytest.mark.parametrize("fabric", [lambda: T.fat_tree(8), lambda: T.torus3d(4, 4, 4)])
def test_equal_utilisation_is_the_least_cost_table(ctx, fabric):
    csr = fabric().csr()
    ctx.upload(csr)
    ctx.set_link_costs(np.ones(csr.E, np.uint32))
    dsts = np.arange(csr.V, dtype=np.int32)
    pcost, nh0, nhp0 = ctx.cost_tables(dsts)
    for x in (0, 7):
        bott, nh, nhp = ctx.widest_tables(pcost, np.full(csr.E, x, np.uint32), dsts)
        assert ctx.last_kernel() == LDS6
        assert np.array_equal(nh, nh0) and np.array_equal(nhp, nhp0)
        assert (bott[pcost != 0] == x).all() and (bott[pcost == 0] == 0).all()


def test_full_utilisation_is_not_no_route(ctx):
    csr = sym_csr(np.array([0, 1]), np.array([1, 2]), 4)         # 0 - 1 - 2, vertex 3 apart
    bott, nh, _ = check(ctx, csr, None, np.full(csr.E, UTIL_MAX, np.uint32), [2])
    assert bott[0].tolist() == [UTIL_MAX, UTIL_MAX, 0, NONE]
    assert nh[0].tolist() == [1, 2, -1, -1]


# ---------------------------------------------------------- form boundary --

@pytest.mark.parametrize("V,kernel", [(EN.WIDEST_LDS_B6_MAX_V, LDS6),
                                      (EN.WIDEST_LDS_B6_MAX_V + 1, LDS4),
                                      (EN.WIDEST_LDS_B4_MAX_V, LDS4),
                                      (EN.WIDEST_LDS_B4_MAX_V + 1, LDS2),
                                      (EN.WIDEST_LDS_MAX_V, LDS2),
                                      (EN.WIDEST_LDS_MAX_V + 1, GLOBAL)])
def test_form_boundary(ctx, V, kernel):
    assert form(V) == kernel
    chain = 300                                          # many sweeps
    R = V - chain                                        # the random part: vertices 0 .. R - 1
    rng = np.random.default_rng(V)
    src = np.repeat(np.arange(R), 3)
    dst = rng.integers(0, R, src.shape[0])
    keep = src != dst
    c = np.arange(R - 1, V - 1)                          # R - 1 -> R -> ... -> V - 1
    csr = sym_csr(np.concatenate([src[keep], c]), np.concatenate([dst[keep], c + 1]), V)
    assert csr.V == V
    cost = seeded_costs(csr, 1, 2, 7)                    # few values: equal-cost choices
    util = seeded_util(csr, 5, 8)
    dsts = [int(rng.integers(0, R)), V - 1, int(rng.integers(0, R))]
    bott, nh, _ = check(ctx, csr, cost, util, dsts, kernel)
    want = max(int(util[edge(csr, x, x + 1)]) for x in range(R - 1, V - 1))
    assert int(bott[1, R - 1]) == want
    assert follow(nh[1], R - 1, V - 1, V) == list(range(R - 1, V))


# ------------------------------------------------------------ disconnected --

def test_disconnected_graph_and_isolated_destination(ctx):
    a = np.array([0, 1, 2, 3, 0])                        # component 0..4
    b = np.array([1, 2, 3, 4, 2])
    c = np.array([5, 6, 7])                              # component 5..8; vertex 9 isolated
    csr = sym_csr(np.concatenate([a, c]), np.concatenate([b, c + 1]), 10)
    cost = seeded_costs(csr, 1, 3, 11)
    bott, nh, nhp = check(ctx, csr, cost, seeded_util(csr, 9, 12), [0, 7, 9, 4])
    assert (bott[0, 5:] == NONE).all() and (nh[0, 5:] == -1).all() and (nhp[0, 5:] == -1).all()
    assert (bott[0, :5] != NONE).all()
    assert (bott[1, :5] == NONE).all() and bott[1, 9] == NONE and (bott[1, 5:9] != NONE).all()
    assert bott[2, 9] == 0 and (bott[2, :9] == NONE).all() and (nh[2] == -1).all()


# -------------------------------------------------------------- validation --

def test_validation(ctx):
    L = _native.library()
    p = _native._ptr
    csr = sym_csr(np.array([0, 1]), np.array([1, 2]), 3)
    dsts = np.zeros(1, np.int32)
    util = np.zeros(csr.E, np.uint32)
    pc = EN.cost_tables_host(csr, np.ones(csr.E, np.uint32), dsts)[0]
    bott = np.empty((1, 3), np.uint32)
    nh = np.empty((1, 3), np.int32)
    nhp = np.empty((1, 3), np.int32)
    with _native.Context(0) as fresh:                    # no graph uploaded
        rc = L.sdnr_widest_tables(fresh._h, p(pc), p(util), p(dsts), 1, p(bott), p(nh), p(nhp), 0)
        assert rc == -77 and L.sdnr_last_error()
    ctx.upload(csr)

    def call(*a):
        return L.sdnr_widest_tables(ctx._h, *a)

    assert call(None, p(util), p(dsts), 1, p(bott), p(nh), p(nhp), 0) == -22     # NULL buffers
    assert call(p(pc), None, p(dsts), 1, p(bott), p(nh), p(nhp), 0) == -22
    assert call(p(pc), p(util), None, 1, p(bott), p(nh), p(nhp), 0) == -22
    assert call(p(pc), p(util), p(dsts), 1, None, p(nh), p(nhp), 0) == -22
    assert call(p(pc), p(util), p(dsts), -1, p(bott), p(nh), p(nhp), 0) == -22
    assert call(p(pc), p(util), p(dsts), 1, p(bott), p(nh), None, 0) == -22      # nh alone
    assert b"go together" in L.sdnr_last_error()
    assert call(None, None, None, 0, None, None, None, 0) == 0                   # ndst == 0
    assert call(None, None, None, 0, None, None, None, _native.DEVICE_PTRS) == 0
    for bad in (3, -1):                                                          # host ids are checked
        with pytest.raises(_native.SdnrError) as ei:
            ctx.widest_tables(pc, util, np.array([bad], np.int32))
        assert ei.value.code == -22
    full = util.copy()
    full[1] = 0xFFFFFFFF
    with pytest.raises(_native.SdnrError) as ei:                                 # above UTIL_MAX
        ctx.widest_tables(pc, full, dsts)
    assert ei.value.code == -22
    got = ctx.widest_tables(pc, util, dsts)                                      # no costs: unit
    assert all(np.array_equal(g, w) for g, w in
               zip(got, EN.widest_tables_host(csr, None, pc, util, dsts)))


def test_a_row_that_is_no_least_cost_row_is_reported(ctx):
    import torch
    csr = G.Golden("jellyfish_n60_r5").fabric().csr()
    cost = seeded_costs(csr, 1, 4, 5)
    util = seeded_util(csr, 3, 6)
    dsts = np.array([3, 17, 41], np.int32)
    ctx.upload(csr)
    ctx.set_link_costs(cost)
    pcost, want = host_tables(csr, cost, util, dsts)
    bad = pcost.copy()
    bad[1, 17] = 5                                       # pcost[d] != 0
    with pytest.raises(_native.SdnrError) as ei:         # host buffers: the call reports it
        ctx.widest_tables(bad, util, dsts)
    assert ei.value.code == -22 and "least-cost labelling" in str(ei.value)
    ctx.synchronize()                                    # ... and the error is cleared
    dev = torch.device("cuda", 0)
    td = torch.from_numpy(dsts).to(dev)
    tu = torch.from_numpy(util.view(np.int32)).to(dev)
    tp = torch.from_numpy(bad.view(np.int32)).to(dev)
    out = [torch.full((3, csr.V), 7, dtype=torch.int32, device=dev) for _ in range(3)]
    torch.cuda.synchronize(dev)
    ctx.widest_tables_device(tp.data_ptr(), tu.data_ptr(), td.data_ptr(), 3, out[0].data_ptr(),
                             out[1].data_ptr(), out[2].data_ptr())
    with pytest.raises(_native.SdnrError) as ei:         # device pointers: at synchronize
        ctx.synchronize()
    assert ei.value.code == -22
    ctx.synchronize()                                    # cleared
    got = [t.cpu().numpy() for t in out]
    for r in (0, 2):                                     # the other rows are intact
        assert np.array_equal(got[0][r].view(np.uint32), want[0][r])
        assert np.array_equal(got[1][r], want[1][r]) and np.array_equal(got[2][r], want[2][r])
    # a vertex of finite cost without a tight link
    bad = pcost.copy()
    x = int(np.argmax(pcost[0]))
    bad[0, x] += 1000
    with pytest.raises(_native.SdnrError) as ei:
        ctx.widest_tables(bad, util, dsts)
    assert ei.value.code == -22
    ctx.synchronize()


# ------------------------------------------------------ device-pointer mode --

def test_device_pointers_on_the_torch_stream(ctx):
    import torch
    csr = G.Golden("jellyfish_n60_r5").fabric().csr()
    cost = seeded_costs(csr, 1, 4, 5)
    util = seeded_util(csr, 3, 6)
    dsts = np.array([3, 59, 17, 17, 0, -1, csr.V], np.int32)     # device ids: unknown -> empty row
    ctx.upload(csr)
    ctx.set_link_costs(cost)
    pcost, want = host_tables(csr, cost, util, dsts[:5])
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        td = torch.from_numpy(dsts).to(dev)
        tu = torch.from_numpy(util.view(np.int32)).to(dev)
        tp = torch.zeros((len(dsts), csr.V), dtype=torch.int32, device=dev)   # rows 5, 6: not read
        tp[:5] = torch.from_numpy(pcost.view(np.int32)).to(dev)
        bt = torch.full((len(dsts), csr.V), 7, dtype=torch.int32, device=dev)
        nh = torch.full_like(bt, 7)
        nhp = torch.full_like(bt, 7)
        ctx.widest_tables_device(tp.data_ptr(), tu.data_ptr(), td.data_ptr(), len(dsts),
                                 bt.data_ptr(), nh.data_ptr(), nhp.data_ptr(), timing=True)
        got = [t.cpu().numpy() for t in (bt, nh, nhp)]
    stream.synchronize()
    assert ctx.last_kernel_ms() >= 0.0
    assert ctx.last_launches() == 1 and ctx.last_kernel() == LDS6
    assert np.array_equal(got[0][:5].view(np.uint32), want[0])
    assert np.array_equal(got[1][:5], want[1]) and np.array_equal(got[2][:5], want[2])
    assert (got[0][5:] == -1).all() and (got[1][5:] == -1).all() and (got[2][5:] == -1).all()
    # bottlenecks only
    with torch.cuda.stream(stream):
        b2 = torch.empty_like(bt)
        ctx.widest_tables_device(tp.data_ptr(), tu.data_ptr(), td.data_ptr(), 5, b2.data_ptr())
        got2 = b2.cpu().numpy()
    assert np.array_equal(got2[:5].view(np.uint32), want[0])
    ctx.set_stream(None)
    ctx.synchronize()                                    # the empty rows raised no error


# -------------------------------------------------------------- the drop-in --

def test_dropin_fat_tree_k4():
    g = G.Golden("fat_tree_k4")
    fabric = T.fat_tree(4)
    want = dropin_results(fake_db(fabric), fabric, g)
    db = fabric.populate(TopologyDB())
    try:
        got = dropin_results(db, fabric, g)
        for key in ("routes", "loads", "default", "batch5", "cap"):
            assert got[key] == want[key], key
        multi = db.find_routes_least_cost(got["pairs"], multiple=True)
        assert all(r in m for r, m in zip(got["routes"], multi) if m)
        t = db.least_loaded_tables()
        ex = db.graph()
        pc = db.least_cost_tables()["pcost"]
        ref = EN.widest_tables_host(ex.csr, db._cost_vector(ex), pc, db._util_vector(ex),
                                    t["destinations"])
        assert np.array_equal(t["bott"], ref[0]) and np.array_equal(t["nh"], ref[1])
        assert np.array_equal(t["nh_port"], ref[2])
        db.engine.ctx.synchronize()
    finally:
        db.engine.close()
