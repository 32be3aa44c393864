"""ECMP over the least-cost routes, CPU only: engine.cost_ecmp_link_loads_host
(the checker of cost_ecmp_loads.hip), least_cost_paths_lex and its counting
twin against a brute-force enumeration of the simple paths; the unit-cost case
against the hop-count restatement and the reference's golden route sets; the
drop-in over an engine double built from the restatements.

Tolerance: that of test_ecmp_link_loads.py (every term of a load is
non-negative: rtol = 1e-9, atol = 0, exactly 0.0 where 0 is expected)."""
import numpy as np
import pytest

import golden_util as G
from oracle import oracle as O
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import SplitLinkLoads, TopologyDB
from test_cost_tables import FakeCostEngine, follow
from test_ecmp_link_loads import (RTOL, SPLITS, FakeEcmpLoadsEngine, close, dicts_close, edge_map,
                                  route_set_loads, splits_differ_csr)
from test_link_loads import golden_pairs

INF = EN.COST_INF


class FakeCostEcmpEngine(FakeCostEngine, FakeEcmpLoadsEngine):
    """The oracle-table double plus cost_tables, ecmp_link_loads and
    cost_ecmp_link_loads from the restatements."""

    def cost_ecmp_link_loads(self, export, cost, pcost, rows, srcs, weights=None, split="route",
                             timing=False):
        self.calls.append(("cost_ecmp", export.key, len(rows)))
        return EN.cost_ecmp_link_loads_host(export.csr, cost, pcost, rows, srcs, weights, split)


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeCostEcmpEngine()
    return db


# ------------------------------------------------------------ helper graphs --

def digraph_csr(edges, V=None):
    """CSR of directed links (u, v) between dense vertices 0..V-1 (dpid u + 1)."""
    src = np.asarray([u for u, _ in edges], np.int64) + 1
    dst = np.asarray([v for _, v in edges], np.int64) + 1
    extra = [] if V is None else list(range(1, V + 1))
    return T.build_csr(src, dst, np.arange(len(edges)) % 60 + 1, extra_vertices=extra)


def both_ways(und):
    return [(u, v) for u, v in und] + [(v, u) for u, v in und]


def edge_costs(csr, costs, default=1):
    """uint32 [E] from {(u, v): cost} over dense ids, ``default`` elsewhere."""
    edge = edge_map(csr)
    c = np.full(int(csr.E), default, np.uint32)
    for k, x in costs.items():
        c[edge[k]] = x
    return c


def random_costs(csr, lo, hi, seed):
    """A cost per directed link: the two directions of a link differ."""
    return np.random.default_rng(seed).integers(lo, hi + 1, int(csr.E)).astype(np.uint32)


def diamond_csr():
    """s -> d direct (cost 2) beside s -> m -> d (1 + 1), links both ways:
    (csr, cost, (s, m, d))."""
    s, m, d = 0, 1, 2
    csr = digraph_csr(both_ways([(s, d), (s, m), (m, d)]))
    return csr, edge_costs(csr, {(s, d): 2, (d, s): 2}), (s, m, d)


def chord_ladder_csr(n):
    """n diamonds in a row, j_k -> {u_k, l_k} -> j_{k+1} at cost 1 each, every
    one with a direct chord j_k -> j_{k+1} at cost 2 (links both ways; vertex
    ids 3k, 3k + 1, 3k + 2): three least-cost routes per diamond, and the
    longest next-hop chain of j_0 has 2n links where its shortest has n."""
    und, chord = [], {}
    for k in range(n):
        j, u, lo, nx = 3 * k, 3 * k + 1, 3 * k + 2, 3 * k + 3
        und += [(j, u), (j, lo), (u, nx), (lo, nx), (j, nx)]
        chord[(j, nx)] = chord[(nx, j)] = 2
    csr = digraph_csr(both_ways(und))
    return csr, edge_costs(csr, chord)


def path_csr_costs(n):
    """A path of n vertices, links both ways, costs cycling 1, 2, 3."""
    csr = digraph_csr(both_ways([(v, v + 1) for v in range(n - 1)]))
    return csr, (np.arange(int(csr.E)) % 3 + 1).astype(np.uint32)


def pcost_rows(csr, cost, dsts):
    return EN.cost_tables_host(csr, cost, np.asarray(dsts, np.int64))[0]


# ------------------------------------------------------------- brute force --

def all_least_cost_paths(csr, cost):
    """{(s, d): (cost, sorted list of vertex tuples)} over every simple path."""
    V = int(csr.V)
    rp, col = csr.row_ptr.tolist(), csr.col.tolist()
    cost = [int(c) for c in cost]
    best = {}

    def walk(path, seen, c):
        x = path[-1]
        key = (path[0], x)
        if key not in best or c < best[key][0]:
            best[key] = (c, [tuple(path)])
        elif c == best[key][0]:
            best[key][1].append(tuple(path))
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
    return {k: (c, sorted(p)) for k, (c, p) in best.items()}


def random_connected_digraph(V, extra, seed):
    """A random spanning tree with both directions of every tree link, plus
    ``extra`` random one-way links."""
    rng = np.random.default_rng(seed)
    edges = set()
    for v in range(1, V):
        u = int(rng.integers(0, v))
        edges |= {(u, v), (v, u)}
    while len(edges) < 2 * (V - 1) + extra:
        u, v = (int(x) for x in rng.integers(0, V, 2))
        if u != v:
            edges.add((u, v))
    return digraph_csr(sorted(edges), V)


@pytest.mark.parametrize("V,extra,seed", [(2, 0, 0), (5, 4, 1), (7, 8, 2), (8, 10, 3), (9, 9, 4),
                                          (9, 14, 5)])
def test_host_checker_routes_and_count_equal_brute_force(V, extra, seed):
    csr = random_connected_digraph(V, extra, seed)
    cost = random_costs(csr, 1, 4, 100 + seed)
    best = all_least_cost_paths(csr, cost)
    pcost = pcost_rows(csr, cost, np.arange(V))
    edge = edge_map(csr)
    rng = np.random.default_rng(200 + seed)
    n = 5 * V
    rows = rng.integers(0, V, n)
    srcs = rng.integers(-1, V + 1, n)                     # out-of-range ones included
    w = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    w[rng.random(n) < 0.3] = 0
    want = np.zeros(int(csr.E))
    ties = 0
    for r, s, x in zip(rows.tolist(), srcs.tolist(), w.tolist()):
        if not 0 <= s < V or s == r or (s, r) not in best:
            continue
        routes = best[(s, r)][1]
        for q in routes:
            for a, b in zip(q[:-1], q[1:]):
                want[edge[(a, b)]] += float(x) / len(routes)
    for d in range(V):
        for s in range(V):
            got = EN.least_cost_paths_lex(csr.row_ptr, csr.col, cost, pcost[d], s, d)
            cnt = EN.count_least_cost_paths(csr.row_ptr, csr.col, cost, pcost[d], s, d)
            if (s, d) not in best:
                assert got == [] and cnt == 0 and pcost[d, s] == INF
                continue
            c, routes = best[(s, d)]
            assert int(pcost[d, s]) == c
            assert got == [list(q) for q in routes]
            assert cnt == len(routes)
            assert EN.count_least_cost_paths(csr.row_ptr, csr.col, cost, pcost[d], s, d, 1) == \
                min(cnt, 2)
            ties += len(routes) > 1
    assert close(EN.cost_ecmp_link_loads_host(csr, cost, pcost, rows, srcs, w, "route"), want)
    # the engine's plane: the same u32 values held in int32
    assert np.array_equal(
        EN.cost_ecmp_link_loads_host(csr, cost, pcost.view(np.int32), rows, srcs, w, "route"),
        EN.cost_ecmp_link_loads_host(csr, cost, pcost, rows, srcs, w, "route"))
    if V >= 7:
        assert ties and want.any()


# -------------------------------------------------------------- unit costs --

@pytest.mark.parametrize("name", G.SMALL)
def test_unit_costs_equal_the_hop_count_restatement(name):
    csr = G.Golden(name).fabric().csr()
    V = int(csr.V)
    dist, _, _ = O.dest_tables(csr, np.arange(V, dtype=np.int32))
    pcost = np.where(dist == 0xFFFF, INF, dist.astype(np.uint32)).astype(np.uint32)
    ones = np.ones(int(csr.E), np.uint32)
    rng = np.random.default_rng(V)
    n = 4 * V
    rows, srcs = rng.integers(0, V, n), rng.integers(0, V, n)
    w = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    for split in SPLITS:
        for wt in (w, None):
            want = EN.ecmp_link_loads_host(csr, dist, rows, srcs, wt, split)
            assert close(EN.cost_ecmp_link_loads_host(csr, ones, pcost, rows, srcs, wt, split),
                         want), (name, split)


@pytest.mark.parametrize("name", G.MULTI)
def test_unit_costs_multiple_routes_equal_the_reference_route_sets(name):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    pairs = golden_pairs(g, fabric)
    sets = [g.multi(i) for i in range(len(pairs))]
    assert db.find_routes_least_cost(pairs, multiple=True) == sets
    assert db.find_route_least_cost(*pairs[0], multiple=True) == sets[0]
    got = db.least_cost_ecmp_link_loads(pairs)
    assert isinstance(got, SplitLinkLoads) and got.load.dtype == np.float64
    assert dicts_close(got.as_dict(), route_set_loads(sets, [1] * len(pairs)))
    assert dicts_close(got.as_dict(), db.ecmp_link_loads(pairs).as_dict())


# ------------------------------------------------- the case level DPs break --

def test_direct_link_ties_a_two_link_route():
    csr, cost, (s, m, d) = diamond_csr()
    pcost = pcost_rows(csr, cost, [d])
    assert pcost[0].tolist() == [2, 1, 0]
    assert EN.count_least_cost_paths(csr.row_ptr, csr.col, cost, pcost[0], s, d) == 2   # sigma[s]
    assert EN.least_cost_paths_lex(csr.row_ptr, csr.col, cost, pcost[0], s, d) == \
        [[s, m, d], [s, d]]
    edge = edge_map(csr)
    w = 10
    want = np.zeros(int(csr.E))
    want[[edge[(s, d)], edge[(s, m)], edge[(m, d)]]] = w / 2
    for split in SPLITS:
        got = EN.cost_ecmp_link_loads_host(csr, cost, pcost, [0], [s], [w], split)
        assert np.array_equal(got, want), split
    # the hop-level rule (next hops one level down) puts it all on the direct link
    dist, _, _ = O.dest_tables(csr, np.array([d], np.int32))
    hop_rule = EN.ecmp_link_loads_host(csr, dist, [0], [s], [w], "route")
    assert hop_rule[edge[(s, d)]] == w and hop_rule[edge[(s, m)]] == 0


def test_chord_ladder_shares_are_thirds():
    csr, cost = chord_ladder_csr(20)
    V = int(csr.V)
    assert V == 61
    pcost = pcost_rows(csr, cost, [V - 1])
    assert int(pcost[0, 0]) == 40
    assert EN.count_least_cost_paths(csr.row_ptr, csr.col, cost, pcost[0], 0, V - 1) == 3 ** 20
    esrc = np.repeat(np.arange(V), np.diff(csr.row_ptr))
    toward = pcost[0][esrc].astype(np.int64) == pcost[0][csr.col].astype(np.int64) + cost
    for split in SPLITS:
        got = EN.cost_ecmp_link_loads_host(csr, cost, pcost, [0], [0], [9], split)
        assert close(got, np.where(toward, 3.0, 0.0)), split


def test_host_checker_rejects_a_row_that_is_no_least_cost_labelling():
    csr, _ = splits_differ_csr()
    cost = np.ones(int(csr.E), np.uint32)
    pcost = pcost_rows(csr, cost, [6])
    bad = pcost.copy()
    bad[0, 1] = 7                                         # no neighbour of a at cost 6
    for split in SPLITS:
        with pytest.raises(ValueError):
            EN.cost_ecmp_link_loads_host(csr, cost, bad, [0], [0], None, split)
    with pytest.raises(ValueError):
        EN.cost_ecmp_link_loads_host(csr, cost, pcost, [0], [0], None, "flow")
    with pytest.raises(ValueError):
        EN.cost_ecmp_link_loads_host(csr, cost[:-1], pcost, [0], [0])
    assert EN.COST_ECMP_LDS_MAX_V == 7400


# ------------------------------------------------------- cost conservation --

def paid(pcost, rows, srcs, w):
    """sum of w_i * pcost[d_i][s_i] over the reachable pairs, in integers."""
    p = pcost[rows, srcs].astype(np.int64)
    ok = p != INF
    return int((w.astype(np.int64)[ok] * p[ok]).sum())


def test_cost_conservation_on_jellyfish_with_random_costs():
    csr = G.Golden("jellyfish_n60_r5").fabric().csr()
    V = int(csr.V)
    cost = random_costs(csr, 1, 5, 11)
    pcost = pcost_rows(csr, cost, np.arange(V))
    rng = np.random.default_rng(12)
    n = 8 * V
    rows, srcs = rng.integers(0, V, n), rng.integers(0, V, n)
    w = rng.integers(0, 1 << 20, n, dtype=np.uint64)
    total = paid(pcost, rows, srcs, w)
    assert total > 0
    loads = {}
    for split in SPLITS:
        loads[split] = EN.cost_ecmp_link_loads_host(csr, cost, pcost, rows, srcs, w, split)
        assert abs(float((loads[split] * cost).sum()) - total) <= RTOL * total, split
    assert not np.array_equal(loads["route"], loads["hop"])


# ------------------------------------------------------------- the drop-in --

def costed_fat_tree_db(**kw):
    """fat_tree(4) with one edge -> aggregation link costed up both ways and
    one aggregation -> core link at cost 2 one way."""
    fabric = T.fat_tree(4)
    db = fake_db(fabric, **kw)
    ex = db.graph()
    e_sw = int(ex.csr.dpids[ex.host_vertices()[0]])
    a_sw = sorted(db.links[e_sw])[0]
    c_sw = [x for x in sorted(db.links[a_sw]) if x not in db.links[e_sw] and x != e_sw
            and not any(h.port.dpid == x for h in db.hosts.values())][-1]
    db.set_link_costs({(e_sw, a_sw): 3, (a_sw, e_sw): 3, (a_sw, c_sw): 2})
    return fabric, db


def test_single_route_form_is_unchanged_under_costs():
    fabric, db = costed_fat_tree_db()
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs for b in macs if a != b]
    ex = db.graph()
    t = db.least_cost_tables()
    row = {int(d): i for i, d in enumerate(t["destinations"])}
    routes = db.find_routes_least_cost(pairs)
    assert routes == db.find_routes_least_cost(pairs, multiple=False)
    every = db.find_routes_least_cost(pairs, multiple=True)
    V = int(ex.csr.V)
    for (a, b), r, rs in zip(pairs, routes, every):
        s, d = ex.index[db.hosts[a].port.dpid], ex.index[db.hosts[b].port.dpid]
        seq = follow(t["nh"][row[d]], s, d, V)             # the next-hop row, walked here
        assert [p[0] for p in r] == [int(ex.csr.dpids[v]) for v in seq]
        assert r[-1] == (db.hosts[b].port.dpid, db.hosts[b].port.port_no)
        assert rs[0] == r and sorted(rs) == rs and len(set(map(tuple, rs))) == len(rs)
    assert db.find_route_least_cost(*pairs[5]) == routes[5]
    assert db.find_route_least_cost(*pairs[5], multiple=True) == every[5]
    assert db.find_route_least_cost("02:00:00:00:ff:ff", macs[0], multiple=True) == []
    assert any(len(rs) > 1 for rs in every) and len({len(rs) for rs in every}) > 2


@pytest.mark.parametrize("split", SPLITS)
def test_dropin_loads_equal_the_enumerated_least_cost_sets(split):
    fabric, db = costed_fat_tree_db()
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs for b in macs if a != b]
    w = np.random.default_rng(3).integers(0, 1 << 32, len(pairs)).tolist()
    got = db.least_cost_ecmp_link_loads(pairs, w, split)
    assert isinstance(got, SplitLinkLoads)
    if split == "route":
        sets = db.find_routes_least_cost(pairs, multiple=True)
        assert dicts_close(got.as_dict(), route_set_loads(sets, w))
        assert not dicts_close(got.as_dict(), db.ecmp_link_loads(pairs, w).as_dict())
    # conservation, link by link
    ex = db.graph()
    cost = db._cost_vector(ex).astype(np.float64)
    t = db.least_cost_tables()
    row = {int(d): i for i, d in enumerate(t["destinations"])}
    total = sum(x * int(t["pcost"][row[ex.index[db.hosts[b].port.dpid]],
                                   ex.index[db.hosts[a].port.dpid]])
                for (a, b), x in zip(pairs, w))
    assert abs(float((got.load * cost).sum()) - total) <= RTOL * total
    allp = db.all_pairs_least_cost_ecmp_link_loads(split)
    assert dicts_close(allp.as_dict(), db.least_cost_ecmp_link_loads(pairs, None, split).as_dict())
    ranks = {r: m for r, m in enumerate(macs[:6])}
    assert dicts_close(
        db.mpi_least_cost_ecmp_link_loads(ranks, None, split).as_dict(),
        db.least_cost_ecmp_link_loads([(ranks[i], ranks[j]) for i in ranks for j in ranks
                                       if i != j], None, split).as_dict())
    with pytest.raises(ValueError):
        db.least_cost_ecmp_link_loads(pairs, None, "flow")


def test_row_chunks_under_a_small_budget():
    fabric, db = costed_fat_tree_db()
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs for b in macs if a != b]
    V = int(db.graph().csr.V)
    _, small = costed_fat_tree_db(table_budget=3 * 12 * V)     # three rows at a time
    for split in SPLITS:
        assert dicts_close(small.least_cost_ecmp_link_loads(pairs, None, split).as_dict(),
                           db.least_cost_ecmp_link_loads(pairs, None, split).as_dict())
    assert sum(1 for c in small.engine.calls if c[0] == "cost_ecmp") > 2
    assert small.find_routes_least_cost(pairs, multiple=True) == \
        db.find_routes_least_cost(pairs, multiple=True)


def test_null_context_is_einval():
    from sdnmpi_amd import _native
    L = _native.library()
    assert L.sdnr_cost_ecmp_link_loads(None, None, 0, None, None, None, None,
                                       _native.DEVICE_PTRS) == -22
