"""cost_tables.hip (sdnr_graph_costs / sdnr_cost_tables) on the GPU against
engine.cost_tables_host, and the drop-in's least-cost routes and loads.
Everything is integer: every comparison is array_equal / ==."""
import copy

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import TopologyDB
from test_cost_tables import INF, follow, seeded_costs
from test_ecmp_link_loads import ladder_csr
from test_link_loads import counter_of, golden_pairs

pytestmark = pytest.mark.gpu

LDS8, LDS4, GLOBAL = ("cost_tables_kernel<lds,8>", "cost_tables_kernel<lds,4>",
                      "cost_tables_kernel<global,4>")
BATCH = 8                                   # destinations per workgroup on the small fabrics


def form(V):
    """The kernel form cost_tables.hip picks for V vertices (from V alone)."""
    return LDS8 if V <= EN.COST_LDS_B8_MAX_V else LDS4 if V <= EN.COST_LDS_MAX_V else GLOBAL


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_error_left(ctx):
    """After every case the context reports no tripped sweep bound."""
    yield
    ctx.set_stream(None)
    ctx.synchronize()


def check(ctx, csr, cost, dsts, kernel=LDS8, want=None):
    """Upload, compute on the GPU, compare all three tables with the host's."""
    ctx.upload(csr)
    ctx.set_link_costs(cost)
    dsts = np.asarray(dsts, np.int32)
    if want is None:
        want = EN.cost_tables_host(csr, cost, dsts)
    got = ctx.cost_tables(dsts)
    for g, w, what in zip(got, want, ("pcost", "nh", "nh_port")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    assert ctx.last_kernel() == kernel
    assert ctx.last_launches() == 1
    ctx.synchronize()
    return got


def edge(csr, u, v):
    lo, hi = int(csr.row_ptr[u]), int(csr.row_ptr[u + 1])
    e = lo + int(np.searchsorted(csr.col[lo:hi], v))
    assert e < hi and int(csr.col[e]) == v
    return e


def sym_csr(src, dst, V):
    """Links both ways over vertices 0..V-1 (dpid = id + 1), ports 1.."""
    s = np.concatenate([src, dst]) + 1
    d = np.concatenate([dst, src]) + 1
    return T.build_csr(s, d, np.arange(s.shape[0]) % 7 + 1, extra_vertices=list(range(1, V + 1)))


# ------------------------------------------------------ the small fabrics --

@pytest.fixture(scope="module")
def small_cases():
    """Per G.SMALL fabric and cost range: the costs and the host's tables of
    every destination, computed once."""
    out = {}
    for k, name in enumerate(G.SMALL):
        csr = G.Golden(name).fabric().csr()
        dsts = np.arange(csr.V, dtype=np.int32)
        for hi in (4, 65535):
            cost = seeded_costs(csr, 1, hi, 100 + k)
            out[(name, hi)] = (csr, cost, dsts, EN.cost_tables_host(csr, cost, dsts))
    return out


@pytest.mark.parametrize("hi", [4, 65535])
@pytest.mark.parametrize("name", G.SMALL)
def test_small_fabrics_every_destination(ctx, small_cases, name, hi):
    csr, cost, dsts, want = small_cases[(name, hi)]
    check(ctx, csr, cost, dsts, want=want)
    # a destination count that is no multiple of the batch, and a single one
    n = csr.V - 1 if (csr.V - 1) % BATCH else csr.V - 2
    assert n % BATCH
    check(ctx, csr, cost, dsts[:n], want=tuple(t[:n] for t in want))
    check(ctx, csr, cost, dsts[-1:], want=tuple(t[-1:] for t in want))
    # costs only
    pc, nh, nhp = ctx.cost_tables(dsts, with_nexthop=False)
    assert nh is None and nhp is None and np.array_equal(pc, want[0])


@pytest.mark.parametrize("fabric", [lambda: T.fat_tree(8), lambda: T.torus3d(4, 4, 4)])
def test_unit_costs_equal_shortest_tables(ctx, fabric):
    csr = fabric().csr()
    ctx.upload(csr)
    ctx.set_link_costs(np.ones(csr.E, np.uint32))
    dsts = np.arange(csr.V, dtype=np.int32)
    pcost, nh, nhp = ctx.cost_tables(dsts)
    assert ctx.last_kernel() == LDS8
    dist, nh0, nhp0 = ctx.shortest_tables(dsts)
    assert np.array_equal(pcost, np.where(dist == 0xFFFF, INF, dist.astype(np.uint32)))
    assert np.array_equal(nh, nh0) and np.array_equal(nhp, nhp0)


# ------------------------------------------------- long relaxation chains --

@pytest.mark.parametrize("shortcut,wins", [(5000, False), (1000, True)])
def test_long_chain_against_a_shortcut(ctx, shortcut, wins):
    V = 2000
    v = np.arange(V - 1)
    src = np.concatenate([v, v + 1, [0]]) + 1
    dst = np.concatenate([v + 1, v, [V - 1]]) + 1
    csr = T.build_csr(src, dst, np.arange(src.shape[0]) % 5 + 1)
    assert csr.V == V and csr.E == 2 * (V - 1) + 1
    cost = np.ones(csr.E, np.uint32)
    cost[edge(csr, 0, V - 1)] = shortcut
    pcost, nh, _ = check(ctx, csr, cost, [0, V - 1])
    # toward V - 1 from vertex 0: 1,999 unit hops or the shortcut
    assert int(pcost[1, 0]) == (shortcut if wins else V - 1)
    assert int(nh[1, 0]) == (V - 1 if wins else 1)
    assert follow(nh[1], 0, V - 1, V) == ([0, V - 1] if wins else list(range(V)))
    # toward 0 the shortcut points the wrong way: the whole chain
    assert int(pcost[0, V - 1]) == V - 1
    assert follow(nh[0], V - 1, 0, V) == list(range(V - 1, -1, -1))


# --------------------------------------------------------------- tie rule --

def test_tie_rule_smallest_neighbour_only_on_equal_cost(ctx):
    n = 5
    csr = ladder_csr(n)
    d = 3 * n
    cost = np.full(csr.E, 2, np.uint32)
    _, nh, _ = check(ctx, csr, cost, [d])
    for k in range(n):                                   # both sides cost 4: the smaller id
        assert int(nh[0, 3 * k]) == 3 * k + 1
    for k in range(n):                                   # the higher-numbered side cheaper by 1
        cost[edge(csr, 3 * k, 3 * k + 2)] = 1
    pcost, nh, _ = check(ctx, csr, cost, [d])
    for k in range(n):
        assert int(nh[0, 3 * k]) == 3 * k + 2
    assert int(pcost[0, 0]) == 3 * n


# ---------------------------------------------------------- form boundary --

@pytest.mark.parametrize("V,kernel", [(EN.COST_LDS_B8_MAX_V, LDS8), (EN.COST_LDS_B8_MAX_V + 1, LDS4),
                                      (EN.COST_LDS_MAX_V, LDS4), (EN.COST_LDS_MAX_V + 1, GLOBAL)])
def test_form_boundary(ctx, V, kernel):
    assert form(V) == kernel
    chain = 300
    R = V - chain                                        # the random part: vertices 0 .. R - 1
    rng = np.random.default_rng(V)
    src = np.repeat(np.arange(R), 3)
    dst = rng.integers(0, R, src.shape[0])
    keep = src != dst
    c = np.arange(R - 1, V - 1)                          # R - 1 -> R -> ... -> V - 1
    csr = sym_csr(np.concatenate([src[keep], c]), np.concatenate([dst[keep], c + 1]), V)
    assert csr.V == V
    cost = seeded_costs(csr, 1, 16, 7)
    dsts = [int(rng.integers(0, R)), V - 1, int(rng.integers(0, R))]
    pcost, _, _ = check(ctx, csr, cost, dsts, kernel)
    assert int(pcost[1, R - 1]) == sum(int(cost[edge(csr, x, x + 1)]) for x in range(R - 1, V - 1))


# ------------------------------------------------------------ disconnected --

def test_disconnected_graph_and_isolated_destination(ctx):
    a = np.array([0, 1, 2, 3, 0])                        # component 0..4
    b = np.array([1, 2, 3, 4, 2])
    c = np.array([5, 6, 7])                              # component 5..8; vertex 9 isolated
    csr = sym_csr(np.concatenate([a, c]), np.concatenate([b, c + 1]), 10)
    cost = seeded_costs(csr, 1, 9, 11)
    pcost, nh, nhp = check(ctx, csr, cost, [0, 7, 9, 4])
    assert (pcost[0, 5:] == INF).all() and (nh[0, 5:] == -1).all() and (nhp[0, 5:] == -1).all()
    assert (pcost[0, :5] != INF).all()
    assert (pcost[1, :5] == INF).all() and pcost[1, 9] == INF and (pcost[1, 5:9] != INF).all()
    assert pcost[2, 9] == 0 and (pcost[2, :9] == INF).all() and (nh[2] == -1).all()


# -------------------------------------------------------------- validation --

def test_validation(ctx):
    L = _native.library()
    csr = sym_csr(np.array([0, 1]), np.array([1, 2]), 3)
    ctx.upload(csr)
    dsts = np.zeros(1, np.int32)

    def fails(code, call, *a, **kw):
        with pytest.raises(_native.SdnrError) as ei:
            call(*a, **kw)
        assert ei.value.code == code, ei.value
        assert L.sdnr_last_error()

    fails(-77, ctx.cost_tables, dsts)                    # no costs yet
    ones = np.ones(csr.E, np.uint32)
    bad = ones.copy()
    bad[1] = 0
    fails(-22, ctx.set_link_costs, bad)                  # a zero cost
    bad[1] = 0x7FFFFFFF + 1
    fails(-22, ctx.set_link_costs, bad)                  # cmax * (V - 1) reaches COST_INF
    fails(-77, ctx.cost_tables, dsts)                    # ... and nothing was uploaded
    bad[1] = 0x7FFFFFFF
    ctx.set_link_costs(bad)                              # 0x7FFFFFFF * 2 < COST_INF: accepted
    pcost, _, _ = ctx.cost_tables(dsts)
    assert np.array_equal(pcost, EN.cost_tables_host(csr, bad, dsts)[0])
    ctx.set_link_costs(ones)
    fails(-22, ctx.cost_tables, np.array([3], np.int32))  # host ids are checked
    fails(-22, ctx.cost_tables, np.array([-1], np.int32))
    pc = np.empty((1, 3), np.uint32)
    nh = np.empty((1, 3), np.int32)
    rc = L.sdnr_cost_tables(ctx._h, _native._ptr(dsts), 1, _native._ptr(pc), _native._ptr(nh),
                            None, 0)
    assert rc == -22 and b"go together" in L.sdnr_last_error()       # nh without nh_port
    rc = L.sdnr_cost_tables(ctx._h, _native._ptr(dsts), 1, None, None, None, 0)
    assert rc == -22 and L.sdnr_last_error()
    ctx.set_link_costs(None)                             # cleared
    fails(-77, ctx.cost_tables, dsts)
    ctx.set_link_costs(ones)
    ctx.cost_tables(dsts)
    ctx.upload(csr)                                      # a re-upload clears the costs
    fails(-77, ctx.cost_tables, dsts)


# ------------------------------------------------------ device-pointer mode --

def test_device_pointers_on_the_torch_stream(ctx):
    import torch
    csr = G.Golden("jellyfish_n60_r5").fabric().csr()
    cost = seeded_costs(csr, 1, 9, 5)
    dsts = np.array([3, 59, 17, 17, 0, -1, csr.V], np.int32)     # device ids: unknown -> empty row
    ctx.upload(csr)
    ctx.set_link_costs(cost)
    want = ctx.cost_tables(dsts[:5])
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        td = torch.from_numpy(dsts).to(dev)
        pc = torch.full((len(dsts), csr.V), 7, dtype=torch.int32, device=dev)
        nh = torch.full_like(pc, 7)
        nhp = torch.full_like(pc, 7)
        ctx.cost_tables_device(td.data_ptr(), len(dsts), pc.data_ptr(), nh.data_ptr(),
                               nhp.data_ptr(), timing=True)
        got = [t.cpu().numpy() for t in (pc, nh, nhp)]
    stream.synchronize()
    assert ctx.last_kernel_ms() >= 0.0
    assert np.array_equal(got[0][:5].view(np.uint32), want[0])
    assert np.array_equal(got[1][:5], want[1]) and np.array_equal(got[2][:5], want[2])
    assert (got[0][5:] == -1).all() and (got[1][5:] == -1).all() and (got[2][5:] == -1).all()
    # costs only
    with torch.cuda.stream(stream):
        pc2 = torch.empty_like(pc)
        ctx.cost_tables_device(td.data_ptr(), 5, pc2.data_ptr())
        got2 = pc2.cpu().numpy()
    assert np.array_equal(got2[:5].view(np.uint32), want[0])
    ctx.set_stream(None)
    ctx.synchronize()


# -------------------------------------------------------------- the drop-in --

def test_dropin_fat_tree_k4():
    g = G.Golden("fat_tree_k4")
    fabric = T.fat_tree(4)
    db = fabric.populate(TopologyDB())
    try:
        pairs = golden_pairs(g, fabric)
        first = [db.find_route(a, b, multiple=True)[0] for a, b in pairs]
        assert db.find_routes_least_cost(pairs) == first
        assert all(db.find_route_least_cost(a, b) == r for (a, b), r in zip(pairs[:8], first))
        plain = copy.deepcopy([db.find_route(a, b) for a, b in pairs])
        multi = copy.deepcopy([db.find_route(a, b, multiple=True) for a, b in pairs])

        ex = db.graph()
        e_sw = int(ex.csr.dpids[ex.host_vertices()[0]])          # an edge switch
        a_sw = sorted(db.links[e_sw])[0]                         # ... and an aggregation switch
        up, down = db.links[e_sw][a_sw].src.port_no, db.links[a_sw][e_sw].src.port_no
        db.set_link_costs({(e_sw, a_sw): 100, (a_sw, e_sw): 100})
        routes = db.find_routes_least_cost(pairs)
        assert all(routes)
        # the edge switch has a second uplink: nothing crosses the costed link
        assert not any((e_sw, up) in r[:-1] or (a_sw, down) in r[:-1] for r in routes)
        assert any((e_sw, up) in r[:-1] or (a_sw, down) in r[:-1] for r in first)
        assert [db.find_route(a, b) for a, b in pairs] == plain
        assert [db.find_route(a, b, multiple=True) for a, b in pairs] == multi

        w = np.random.default_rng(9).integers(0, 1 << 32, len(pairs)).tolist()
        ll = db.least_cost_link_loads(pairs, w)
        want = counter_of(routes, w)
        assert ll.as_dict() == want
        links = {(int(s), int(p)): int(x) for s, p, x in
                 zip(ll.src_dpid.tolist(), ll.port.tolist(), ll.load.tolist()) if x}
        hist = counter_of([r[:-1] for r in routes], w)
        assert links == hist
        # conservation: sum_e load[e] * cost[e] == sum_pairs w * pcost[s -> d]
        ex = db.graph()
        cost = [db.link_cost(int(s), int(d)) for s, d in
                zip(ll.src_dpid.tolist(), ll.dst_dpid.tolist())]
        t = db.least_cost_tables()
        row = {int(d): i for i, d in enumerate(t["destinations"])}
        paid = 0
        for (a, b), x in zip(pairs, w):
            s, d = ex.index[db.hosts[a].port.dpid], ex.index[db.hosts[b].port.dpid]
            assert t["pcost"][row[d], s] != INF
            paid += x * int(t["pcost"][row[d], s])
        assert sum(x * c for x, c in zip(ll.load.tolist(), cost)) == paid
        assert db.all_pairs_least_cost_link_loads().as_dict() == counter_of(
            db.find_routes_least_cost([(a, b) for a in fabric.host_macs()
                                       for b in fabric.host_macs() if a != b]),
            [1] * (len(fabric.host_macs()) * (len(fabric.host_macs()) - 1)))

        link = db.links[e_sw][a_sw]
        db.delete_link(link)
        assert all(db.find_routes_least_cost(pairs))
        db.add_link(link)
        assert db.find_routes_least_cost(pairs) == routes        # the cost is still in force
        db.clear_link_costs()
        assert db.find_routes_least_cost(pairs) == first
        db.engine.ctx.synchronize()
    finally:
        db.engine.close()
