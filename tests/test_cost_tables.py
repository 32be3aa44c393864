"""Least-cost routes under per-link costs, without a GPU: the CPU restatement
(engine.cost_tables_host, the checker of cost_tables.hip) against brute-force
path enumeration and, with unit costs, against the oracle's shortest tables;
TopologyDB's cost state; the drop-in over an engine double that answers
cost_tables from the restatement; the C ABI's device-free error paths."""
import numpy as np
import pytest

import golden_util as G
from oracle import oracle as O
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import TopologyDB
from test_link_loads import FakeLoadsEngine, counter_of, golden_pairs

INF = EN.COST_INF


def seeded_costs(csr, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, int(csr.E)).astype(np.uint32)


def follow(nh_row, x, d, V):
    """Vertex sequence x .. d along a next-hop row (None if it leaves it)."""
    seq = [x]
    while x != d:
        x = int(nh_row[x])
        if x < 0 or len(seq) > V:
            return None
        seq.append(x)
    return seq


# ------------------------------------------------------------ brute force --

def best_simple_paths(csr, cost):
    """{(x, d): (cost, vertex tuple)}: over every simple path x -> d the least
    cost, then the lexicographically smallest vertex sequence."""
    V = int(csr.V)
    rp, col = csr.row_ptr.tolist(), csr.col.tolist()
    cost = [int(c) for c in cost]
    best = {}

    def walk(path, seen, c):
        x = path[-1]
        key = (path[0], x)
        cand = (c, tuple(path))
        if key not in best or cand < best[key]:
            best[key] = cand
        for e in range(rp[x], rp[x + 1]):
            n = col[e]
            if n not in seen:
                seen.add(n)
                path.append(n)
                walk(path, seen, c + cost[e])
                path.pop()
                seen.discard(n)

    for s in range(V):
        walk([s], {s}, 0)
    return best


@pytest.mark.parametrize("name", ["random_V9", "random_V12"])
@pytest.mark.parametrize("lo,hi,seed", [(1, 4, 1), (1, 4, 2), (1, 4, 3), (1, 65535, 4)])
def test_host_tables_equal_brute_force(name, lo, hi, seed):
    csr = G.Golden(name).fabric().csr()
    V = int(csr.V)
    cost = seeded_costs(csr, lo, hi, seed)
    best = best_simple_paths(csr, cost)
    dsts = np.arange(V)
    pcost, nh, nhp = EN.cost_tables_host(csr, cost, dsts)
    assert pcost.dtype == np.uint32 and nh.dtype == np.int32 and nhp.dtype == np.int32
    for d in range(V):
        for x in range(V):
            if (x, d) not in best:
                assert pcost[d, x] == INF and nh[d, x] == -1 and nhp[d, x] == -1
                continue
            c, seq = best[(x, d)]
            assert int(pcost[d, x]) == c
            assert follow(nh[d], x, d, V) == list(seq)
            if x == d:
                assert nh[d, x] == -1 and nhp[d, x] == -1
            else:
                lo_e = int(csr.row_ptr[x])
                e = lo_e + int(np.searchsorted(csr.col[lo_e:int(csr.row_ptr[x + 1])], seq[1]))
                assert int(nhp[d, x]) == int(csr.port[e])


# ------------------------------------------------------------- unit costs --

@pytest.mark.parametrize("name", G.SMALL)
def test_unit_costs_equal_the_oracles_shortest_tables(name):
    csr = G.Golden(name).fabric().csr()
    dsts = np.arange(int(csr.V), dtype=np.int32)
    pcost, nh, nhp = EN.cost_tables_host(csr, np.ones(int(csr.E), np.uint32), dsts)
    dist, nho, nhpo = O.dest_tables(csr, dsts)
    wide = np.where(dist == 0xFFFF, INF, dist.astype(np.uint32)).astype(np.uint32)
    assert np.array_equal(pcost, wide)
    assert np.array_equal(nh, nho)
    assert np.array_equal(nhp, nhpo)


def test_host_tables_check_their_costs():
    csr = G.Golden("random_V9").fabric().csr()
    E = int(csr.E)
    ones = np.ones(E, np.uint32)
    with pytest.raises(ValueError):
        EN.cost_tables_host(csr, ones[:-1], [0])
    bad = ones.copy()
    bad[3] = 0
    with pytest.raises(ValueError):
        EN.cost_tables_host(csr, bad, [0])
    bad[3] = 0xFFFFFFFE
    with pytest.raises(ValueError):
        EN.cost_tables_host(csr, bad, [0])
    # an unknown destination is an empty row
    pcost, nh, nhp = EN.cost_tables_host(csr, ones, [-1, int(csr.V)])
    assert (pcost == INF).all() and (nh == -1).all() and (nhp == -1).all()
    assert EN.COST_LDS_B8_MAX_V == 5000 and EN.COST_LDS_MAX_V == 10000


# ------------------------------------------------- TopologyDB: cost state --

def test_topologydb_cost_state():
    fabric = T.fat_tree(4)
    db = fabric.populate(TopologyDB())
    before = db.to_dict()
    u = sorted(db.links)[0]
    v = sorted(db.links[u])[0]
    assert db.link_cost(u, v) == 1
    for bad in (0, -1, 2 ** 32 - 1, 2 ** 40, 1.5, "3", None, True):
        with pytest.raises(ValueError):
            db.set_link_cost(u, v, bad)
    with pytest.raises(ValueError):
        db.set_link_costs({(u, v): 7, (v, u): 0})
    assert db.link_cost(u, v) == 1                  # nothing set by a refused mapping
    db.set_link_cost(u, v, 2 ** 32 - 2)
    assert db.link_cost(u, v) == 2 ** 32 - 2
    db.set_link_costs({(u, v): 100, (v, u): np.int64(100)})
    assert db.link_cost(u, v) == 100 and db.link_cost(v, u) == 100
    db.set_link_cost(12345, 54321, 9)               # a link that does not exist (yet)
    assert db.link_cost(12345, 54321) == 9
    assert db.to_dict() == before                   # costs are no part of the snapshot
    # operator configuration: independent of the links dict
    link = db.links[u][v]
    db.delete_link(link)
    assert db.link_cost(u, v) == 100
    db.add_link(link)
    assert db.link_cost(u, v) == 100
    flapped = db.to_dict()                          # (the re-added link moved to its row's end)
    db.clear_link_costs()
    assert db.link_cost(u, v) == 1 and db.link_cost(12345, 54321) == 1
    assert db.to_dict() == flapped


# ----------------------------------- the drop-in over the host restatement --

class FakeCostEngine(FakeLoadsEngine):
    """The oracle-table double plus cost_tables from the restatement."""

    def cost_tables(self, export, cost, dsts, timing=False):
        self.calls.append(("cost", export.key, len(dsts)))
        return EN.cost_tables_host(export.csr, cost, dsts)


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeCostEngine()
    return db


@pytest.mark.parametrize("name", G.MULTI)
def test_no_costs_is_the_first_shortest_route(name):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    pairs = golden_pairs(g, fabric)
    want = [(g.multi(i) or [[]])[0] for i in range(len(pairs))]
    assert db.find_routes_least_cost(pairs) == want
    assert db.find_route_least_cost(*pairs[0]) == want[0]
    assert db.least_cost_link_loads(pairs).as_dict() == counter_of(want, [1] * len(pairs))
    t, s = db.least_cost_tables(), db.route_tables("shortest")
    assert np.array_equal(t["destinations"], s["destinations"])
    assert np.array_equal(t["nh"], s["nh"]) and np.array_equal(t["nh_port"], s["nh_port"])
    assert np.array_equal(t["pcost"], np.where(s["dist"] == 0xFFFF, INF,
                                               s["dist"].astype(np.uint32)))


def test_costed_link_is_avoided_and_loads_follow_the_routes():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs for b in macs if a != b]
    plain = db.find_routes(pairs[:40])
    ex = db.graph()
    hv = ex.host_vertices()
    e_sw = int(ex.csr.dpids[hv[0]])                      # an edge switch
    a_sw = sorted(db.links[e_sw])[0]                     # ... and its first aggregation switch
    port = db.links[e_sw][a_sw].src.port_no
    db.set_link_costs({(e_sw, a_sw): 100, (a_sw, e_sw): 100})
    routes = db.find_routes_least_cost(pairs)
    assert all(r for r in routes)
    assert not any((e_sw, port) in r[:-1] for r in routes)
    assert db.find_routes(pairs[:40]) == plain           # hop-count routes ignore costs
    w = np.random.default_rng(3).integers(0, 1 << 32, len(pairs)).tolist()
    ll = db.least_cost_link_loads(pairs, w)
    assert ll.as_dict() == counter_of(routes, w)
    # conservation: every unit of demand pays its route's cost, link by link
    cost = db._cost_vector(ex).astype(object)
    t = db.least_cost_tables()
    row = {int(d): i for i, d in enumerate(t["destinations"])}
    paid = 0
    for (a, b), x in zip(pairs, w):
        s, d = ex.index[db.hosts[a].port.dpid], ex.index[db.hosts[b].port.dpid]
        paid += x * int(t["pcost"][row[d], s])
    assert sum(int(x) * int(c) for x, c in zip(ll.load.tolist(), cost)) == paid
    assert db.all_pairs_least_cost_link_loads().as_dict() == \
        db.least_cost_link_loads(pairs).as_dict()
    ranks = {r: m for r, m in enumerate(macs[:6])}
    assert db.mpi_least_cost_link_loads(ranks).as_dict() == db.least_cost_link_loads(
        [(ranks[i], ranks[j]) for i in ranks for j in ranks if i != j]).as_dict()
    # the cost outlives a flap of the link
    link = db.links[e_sw][a_sw]
    db.delete_link(link)
    db.add_link(link)
    assert db.find_routes_least_cost(pairs) == routes
    db.clear_link_costs()
    assert db.find_routes_least_cost(pairs[:40]) == \
        [db.find_route(a, b, multiple=True)[0] for a, b in pairs[:40]]


def test_rows_are_memoised_and_chunked_under_a_small_budget():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs for b in macs if a != b]
    want = db.find_routes_least_cost(pairs)
    n = len([c for c in db.engine.calls if c[0] == "cost"])
    assert db.find_routes_least_cost(pairs) == want           # every row memoised
    assert len([c for c in db.engine.calls if c[0] == "cost"]) == n
    db.set_link_cost(1, 2, 3)                                 # the costs changed: recomputed
    db.find_routes_least_cost(pairs[:1])
    assert len([c for c in db.engine.calls if c[0] == "cost"]) == n + 1
    V = int(db.graph().csr.V)
    small = fake_db(fabric, table_budget=3 * 12 * V)          # three rows at a time
    assert small.find_routes_least_cost(pairs) == want
    assert small.least_cost_link_loads(pairs).as_dict() == \
        db.least_cost_link_loads(pairs).as_dict()
    assert all(c[2] <= 3 for c in small.engine.calls if c[0] == "cost")
    full, part = db.least_cost_tables(), small.least_cost_tables()
    for k in ("pcost", "nh", "nh_port"):
        assert np.array_equal(full[k], part[k])


def test_endpoint_rules_follow_find_route():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    assert db.find_route_least_cost(macs[0], "00:00:00:00:ff:ff") == []
    assert db.find_route_least_cost("00:00:00:00:ff:ff", macs[0]) == []
    with pytest.raises(ValueError):
        db.find_route_least_cost("no:th:ex", macs[0])
    same = [m for m in macs if db.hosts[m].port.dpid == db.hosts[macs[0]].port.dpid]
    assert db.find_route_least_cost(same[0], same[1]) == db.find_route(same[0], same[1])
    sw = sorted(db.switches)[0]
    local = ":".join("%02x" % ((sw >> s) & 0xFF) for s in range(40, -8, -8))
    assert db.find_route_least_cost(macs[-1], local) == \
        db.find_route(macs[-1], local, multiple=True)[0]
    # unreachable: the destination's switch loses every link
    d_sw = db.hosts[macs[-1]].port.dpid
    for u in list(db.links):
        for v in list(db.links[u]):
            if u == d_sw or v == d_sw:
                db.delete_link(db.links[u][v])
    assert db.find_route_least_cost(macs[0], macs[-1]) == []
    assert db.find_route(macs[0], macs[-1]) == []


# ------------------------------------------------------------------ C ABI --

def test_null_context_is_einval():
    L = _native.library()
    assert L.sdnr_graph_costs(None, None) == -22
    assert b"null context" in L.sdnr_last_error()
    assert L.sdnr_cost_tables(None, None, 0, None, None, None, 0) == -22
    assert b"null context" in L.sdnr_last_error()
