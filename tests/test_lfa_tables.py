"""Loop-free alternate (fast-reroute) next hops, CPU only:
engine.lfa_tables_host (the checker of lfa_tables.hip) against the definition
by enumeration -- "no least-cost route n -> d visits s" (loop-free) and "...
visits p" (node-protecting), over engine.least_cost_paths_lex's route lists --
the named small cases with their tables written out, and the drop-in over an
engine double built from the restatements.  Everything is integer: every
comparison is exact."""
import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.objects import Link, Port
from sdnmpi_amd.util.topology_db import TopologyDB
from test_cost_ecmp_loads import both_ways, digraph_csr, edge_costs, random_costs
from test_ecmp_link_loads import edge_map
from test_failure_loads import FakeFailureEngine
from test_link_loads import golden_pairs

INF = EN.COST_INF
BIG = 2 ** 31 - 1
ENUM_FABRICS = ["mock", "random_V9", "random_V12", "torus_2x2x2", "fat_tree_k4",
                "dragonfly_a4_h2_p2"]


class FakeLfaEngine(FakeFailureEngine):
    """The restatement double plus lfa_tables."""

    def lfa_tables(self, export, cost, pcost_all, dsts, link_only=False, timing=False):
        self.calls.append(("lfa", export.key, len(dsts), bool(link_only)))
        return EN.lfa_tables_host(export.csr, cost, pcost_all, dsts, link_only)


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeLfaEngine()
    return db


def all_pairs(csr, cost):
    """pcost_all [V, V]: row v = the least costs toward v."""
    return EN.cost_tables_host(csr, cost, np.arange(int(csr.V)))[0]


# -------------------------------------------------- the definition, enumerated --

def enum_lfa(csr, cost, P, link_only):
    """(backup, kind) [V, V] from the definition: the routes of
    engine.least_cost_paths_lex decide loop-free and node-protecting, the
    selection key is (not node-protecting, cost + P[d][n], n)."""
    V = int(csr.V)
    rp, col = csr.row_ptr, csr.col
    visits = {}

    def visited(n, d):
        if (n, d) not in visits:
            seen = set()
            for q in EN.least_cost_paths_lex(rp, col, cost, P[d], n, d):
                seen.update(q)
            visits[(n, d)] = seen
        return visits[(n, d)]

    backup = np.full((V, V), -1, np.int32)
    kind = np.zeros((V, V), np.uint8)
    for d in range(V):
        for s in range(V):
            if s == d or P[d, s] == INF:
                continue
            row = range(int(rp[s]), int(rp[s + 1]))
            tight = [e for e in row if P[d, col[e]] != INF and
                     int(cost[e]) + int(P[d, col[e]]) == int(P[d, s])]
            assert tight, "a reached vertex has a next hop"
            p = int(col[tight[0]])
            best = None
            for e in row:
                n = int(col[e])
                if n == p or P[d, n] == INF:
                    continue
                via = visited(n, d)
                if s in via:
                    continue
                npro = (not link_only) and p not in via
                key = (not npro, int(cost[e]) + int(P[d, n]), n)
                if best is None or key < best[0]:
                    best = (key, n, npro, int(P[d, n]) < int(P[d, s]))
            if best is not None:
                backup[d, s] = best[1]
                kind[d, s] = 1 | (2 if best[3] else 0) | (4 if best[2] else 0)
    return backup, kind


def ports_of(csr, backup):
    """The port of the link s -> backup[d, s] (-1 where there is none)."""
    edge = edge_map(csr)
    out = np.full(backup.shape, -1, np.int32)
    for d, s in zip(*np.nonzero(backup >= 0)):
        out[d, s] = csr.port[edge[(int(s), int(backup[d, s]))]]
    return out


def counts_of(csr, cost, P, kind):
    """[D, 4] from the tables: the primaries are the vertices with a route."""
    V = int(csr.V)
    prim = ((P != INF) & ~np.eye(V, dtype=bool)).sum(1)
    return np.stack([prim, (kind & 1 != 0).sum(1), (kind & 4 != 0).sum(1),
                     (kind & 2 != 0).sum(1)], 1).astype(np.uint32)


@pytest.mark.parametrize("hi", [1, 3])
@pytest.mark.parametrize("name", ENUM_FABRICS)
def test_restatement_equals_the_enumerated_definition(name, hi):
    csr = G.Golden(name).fabric().csr()
    V = int(csr.V)
    cost = random_costs(csr, 1, hi, 7 * V + hi)
    P = all_pairs(csr, cost)
    kinds = set()
    for link_only in (False, True):
        backup, bport, kind, counts = EN.lfa_tables_host(csr, cost, P, np.arange(V), link_only)
        eb, ek = enum_lfa(csr, cost, P, link_only)
        assert np.array_equal(backup, eb)
        assert np.array_equal(kind, ek)
        assert np.array_equal(bport, ports_of(csr, eb))
        assert np.array_equal(counts, counts_of(csr, cost, P, ek))
        assert backup.dtype == np.int32 and bport.dtype == np.int32
        assert kind.dtype == np.uint8 and counts.dtype == np.uint32
        if link_only:
            assert not (kind & 4).any()
        kinds |= set(np.unique(kind).tolist())
    assert 0 in kinds and len(kinds) > 1


def test_unit_costs_need_no_cost_vector():
    csr = G.Golden("fat_tree_k4").fabric().csr()
    V = int(csr.V)
    ones = np.ones(int(csr.E), np.uint32)
    P = all_pairs(csr, ones)
    a = EN.lfa_tables_host(csr, None, P, np.arange(V))
    b = EN.lfa_tables_host(csr, ones, P.view(np.int32), np.arange(V))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the issue's prototype figure: half of the fat-tree's primaries (the
    # up-links' ECMP twins) have an alternate
    tot = a[3].sum(0)
    assert (int(tot[0]), int(tot[1])) == (380, 188)


# ------------------------------------------------------------ the named cases --

def named_case(name):
    """(csr, cost, {link_only: (backup, kind)}) of a named small graph; the
    tables are written out, row d = destination d."""
    if name == "triangle":                       # an alternate everywhere; p == d: never node-protecting
        csr = digraph_csr(both_ways([(0, 1), (1, 2), (0, 2)]))
        b = [[-1, 2, 1], [2, -1, 0], [1, 0, -1]]
        k = [[0, 1, 1], [1, 0, 1], [1, 1, 0]]
        return csr, edge_costs(csr, {}), {False: (b, k), True: (b, k)}
    if name == "ring4":                          # adjacent pairs have none, the antipode has one
        csr = digraph_csr(both_ways([(0, 1), (1, 2), (2, 3), (3, 0)]))
        b = [[-1, -1, 3, -1], [-1, -1, -1, 2], [3, -1, -1, -1], [-1, 2, -1, -1]]
        k7 = [[0, 0, 7, 0], [0, 0, 0, 7], [7, 0, 0, 0], [0, 7, 0, 0]]
        k3 = [[0, 0, 3, 0], [0, 0, 0, 3], [3, 0, 0, 0], [0, 3, 0, 0]]
        return csr, edge_costs(csr, {}), {False: (b, k7), True: (b, k3)}
    if name == "ring4_cost3":                    # 0 - 1 at cost 3: the adjacent pair gets one
        csr = digraph_csr(both_ways([(0, 1), (1, 2), (2, 3), (3, 0)]))
        b = [[-1, 2, -1, -1], [3, -1, -1, -1], [1, 0, -1, -1], [1, 0, -1, -1]]
        kn = [[0, 3, 0, 0], [3, 0, 0, 0], [7, 1, 0, 0], [1, 7, 0, 0]]
        kl = [[0, 3, 0, 0], [3, 0, 0, 0], [3, 1, 0, 0], [1, 3, 0, 0]]
        return csr, edge_costs(csr, {(0, 1): 3, (1, 0): 3}), {False: (b, kn), True: (b, kl)}
    if name == "dearer_node_protecting":
        # toward 2, switch 0 (primary 1): neighbour 3 is the cheapest loop-free
        # one but routes through 1; neighbour 4 costs more and avoids it
        csr = digraph_csr(both_ways([(0, 1), (1, 2), (0, 3), (3, 1), (0, 4), (4, 2)]))
        cost = edge_costs(csr, {(0, 4): 2, (4, 0): 2, (4, 2): 2, (2, 4): 2})
        bn = [[-1, 3, 4, 1, 2], [3, -1, -1, 0, 2], [4, -1, -1, 0, 0], [1, 0, 4, -1, 2],
              [-1, 2, -1, 1, -1]]
        kn = [[0, 1, 5, 1, 1], [1, 0, 0, 1, 7], [5, 0, 0, 1, 1], [1, 1, 5, 0, 7], [0, 7, 0, 1, 0]]
        bl = [[-1, 3, 4, 1, 2], [3, -1, -1, 0, 2], [3, -1, -1, 0, 0], [1, 0, 4, -1, 2],
              [-1, 2, -1, 1, -1]]
        kl = [[0, 1, 1, 1, 1], [1, 0, 0, 1, 3], [1, 0, 0, 1, 1], [1, 1, 1, 0, 3], [0, 3, 0, 1, 0]]
        return csr, cost, {False: (bn, kn), True: (bl, kl)}
    if name == "one_way":                        # 3 cannot reach 0: loop-free by the INF clause
        csr = digraph_csr([(0, 1), (1, 2), (0, 3), (3, 2)], 4)
        b = [[-1] * 4, [-1] * 4, [3, -1, -1, -1], [-1] * 4]
        kn = [[0] * 4, [0] * 4, [7, 0, 0, 0], [0] * 4]
        kl = [[0] * 4, [0] * 4, [3, 0, 0, 0], [0] * 4]
        return csr, edge_costs(csr, {}), {False: (b, kn), True: (b, kl)}
    if name == "two_components":
        csr = digraph_csr(both_ways([(0, 1), (1, 2), (0, 2), (3, 4)]))
        b = [[-1, 2, 1, -1, -1], [2, -1, 0, -1, -1], [1, 0, -1, -1, -1], [-1] * 5, [-1] * 5]
        k = [[0, 1, 1, 0, 0], [1, 0, 1, 0, 0], [1, 1, 0, 0, 0], [0] * 5, [0] * 5]
        return csr, edge_costs(csr, {}), {False: (b, k), True: (b, k)}
    if name == "degree_one":                     # 3 hangs off the triangle: never a candidate
        csr = digraph_csr(both_ways([(0, 1), (1, 2), (0, 2), (2, 3)]))
        b = [[-1, 2, 1, -1], [2, -1, 0, -1], [1, 0, -1, -1], [1, 0, -1, -1]]
        k = [[0, 1, 1, 0], [1, 0, 1, 0], [1, 1, 0, 0], [1, 1, 0, 0]]
        return csr, edge_costs(csr, {}), {False: (b, k), True: (b, k)}
    if name == "big_triangle":                   # costs 2^31 - 1: sums reach 2^32 - 2
        csr = digraph_csr(both_ways([(0, 1), (1, 2), (0, 2)]))
        b = [[-1, 2, 1], [2, -1, 0], [1, 0, -1]]
        k = [[0, 1, 1], [1, 0, 1], [1, 1, 0]]
        return csr, np.full(int(csr.E), BIG, np.uint32), {False: (b, k), True: (b, k)}
    if name == "big_triangle_one_way":
        # no link 2 -> 1: P[1][2] = 2 (2^31 - 1) and P[1][2] + P[0][1] =
        # 3 (2^31 - 1) = 2^32 + 2^31 - 3; a 32-bit sum would wrap to 2^31 - 3,
        # below P[0][2] = 2^31 - 1, and lose switch 1's alternate toward 0
        csr = digraph_csr([(1, 0), (1, 2), (2, 0), (0, 1), (0, 2)])
        b = [[-1, 2, -1], [-1, -1, -1], [1, 0, -1]]
        k = [[0, 1, 0], [0, 0, 0], [1, 1, 0]]
        return csr, np.full(int(csr.E), BIG, np.uint32), {False: (b, k), True: (b, k)}
    raise KeyError(name)


NAMED = ["triangle", "ring4", "ring4_cost3", "dearer_node_protecting", "one_way",
         "two_components", "degree_one", "big_triangle", "big_triangle_one_way"]


@pytest.mark.parametrize("name", NAMED)
def test_named_cases(name):
    csr, cost, want = named_case(name)
    V = int(csr.V)
    P = all_pairs(csr, cost)
    for link_only in (False, True):
        backup, bport, kind, counts = EN.lfa_tables_host(csr, cost, P, np.arange(V), link_only)
        wb, wk = (np.asarray(a) for a in want[link_only])
        assert np.array_equal(backup, wb), link_only
        assert np.array_equal(kind, wk), link_only
        assert np.array_equal(bport, ports_of(csr, wb))
        assert np.array_equal(counts, counts_of(csr, cost, P, wk))
        eb, ek = enum_lfa(csr, cost, P, link_only)
        assert np.array_equal(eb, wb) and np.array_equal(ek, wk)


def test_named_cases_show_what_they_are_named_for():
    csr, cost, want = named_case("dearer_node_protecting")
    assert want[False][0][2][0] == 4 and want[True][0][2][0] == 3
    csr, cost, _ = named_case("one_way")
    assert all_pairs(csr, cost)[0, 3] == INF
    csr, cost, _ = named_case("big_triangle_one_way")
    P = all_pairs(csr, cost).astype(np.int64)
    assert P[1, 2] + P[0, 1] >= 2 ** 32 and (P[1, 2] + P[0, 1]) % 2 ** 32 < P[0, 2]


def test_rows_follow_the_destination_list():
    csr = G.Golden("random_V12").fabric().csr()
    V = int(csr.V)
    cost = random_costs(csr, 1, 4, 5)
    P = all_pairs(csr, cost)
    full = EN.lfa_tables_host(csr, cost, P, np.arange(V))
    dsts = np.asarray([5, -1, 0, 5, V, 11])
    got = EN.lfa_tables_host(csr, cost, P, dsts)
    for i, d in enumerate(dsts.tolist()):
        for a, f in zip(got, full):
            if 0 <= d < V:
                assert np.array_equal(a[i], f[d])
            else:
                assert np.array_equal(a[i], np.full_like(a[i], -1 if a.dtype == np.int32 else 0))
    with pytest.raises(ValueError):
        EN.lfa_tables_host(csr, cost, P[:-1], dsts)


# ------------------------------------------------------------------ the drop-in --

def dropin_state(db, pairs):
    """Everything the LFA methods answer, for comparing two databases."""
    V = int(db.graph().csr.V)
    t = db.lfa_tables(vertices=range(V))
    lt = db.lfa_tables(vertices=range(V), node_protect=False)
    return (t["backup"].tolist(), t["backup_port"].tolist(), t["kind"].tolist(),
            lt["backup"].tolist(), lt["kind"].tolist(), db.find_routes_protected(pairs),
            db.lfa_coverage(), db.lfa_coverage(node_protect=False), db.unprotected_links())


@pytest.mark.parametrize("name", ["fat_tree_k4", "random_V12", "dragonfly_a4_h2_p2"])
def test_dropin_over_the_engine_double(name):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    ex = db.graph()
    csr = ex.csr
    V = int(csr.V)
    rng = np.random.default_rng(V)
    links = [(a, b) for a in db.links for b in db.links[a]]
    db.set_link_costs({links[i]: int(rng.integers(1, 4)) for i in
                       rng.choice(len(links), len(links) // 3, replace=False)})
    cost = db._cost_vector(ex)
    P = all_pairs(csr, cost)
    want = EN.lfa_tables_host(csr, cost, P, np.arange(V))
    pairs = golden_pairs(g, fabric)

    # the tables, for the host-bearing switches by default
    t = db.lfa_tables()
    hv = np.asarray(ex.host_vertices(), np.int64)
    assert np.array_equal(t["destinations"], hv)
    assert np.array_equal(t["backup"], want[0][hv])
    assert np.array_equal(t["backup_port"], want[1][hv])
    assert np.array_equal(t["kind"], want[2][hv])
    assert t["kind"].dtype == np.uint8
    lt = db.lfa_tables(vertices=[0, V - 1], node_protect=False)
    lw = EN.lfa_tables_host(csr, cost, P, [0, V - 1], link_only=True)
    assert np.array_equal(lt["backup"], lw[0]) and np.array_equal(lt["kind"], lw[2])

    # protected routes: the projection is the least-cost route, the backup
    # port is a real port of that switch toward the backup
    routes = db.find_routes_least_cost(pairs)
    prot = db.find_routes_protected(pairs)
    assert [[(h[0], h[1]) for h in r] for r in prot] == routes
    assert db.find_route_protected(*pairs[0]) == prot[0]
    assert db.find_route_protected("00:00:00:00:00:00:00:fe", pairs[0][1]) == []
    seen = 0
    for r in prot:
        if not r:
            continue
        assert r[-1][2] is None and r[-1][3] == 0
        d = ex.index[r[-1][0]]
        for dpid, out_port, bport, kind in r[:-1]:
            s = ex.index[dpid]
            assert kind == int(want[2][d, s])
            if kind == 0:
                assert bport is None
                continue
            seen += 1
            b_dpid = int(csr.dpids[want[0][d, s]])
            assert db.links[dpid][b_dpid].src.port_no == bport and bport != out_port
    assert seen > 0

    # coverage and the unprotected cables, from the tables
    tot = want[3].astype(np.int64).sum(0)
    cov = db.lfa_coverage()
    assert (cov["primaries"], cov["backups"], cov["node_protecting"], cov["downstream"]) == \
        tuple(int(x) for x in tot)
    assert cov["coverage"] == tot[1] / tot[0] and cov["node_coverage"] == tot[2] / tot[0]
    assert cov["downstream_coverage"] == tot[3] / tot[0]
    lcov = db.lfa_coverage(node_protect=False)
    assert lcov["backups"] == cov["backups"] and lcov["node_protecting"] == 0
    nh = EN.cost_tables_host(csr, cost, np.arange(V))[1]
    bare = {}
    for d in range(V):
        for s in range(V):
            if nh[d, s] >= 0 and want[2][d, s] == 0:
                key = (int(csr.dpids[s]), int(csr.dpids[nh[d, s]]))
                bare[key] = bare.get(key, 0) + 1
    assert db.unprotected_links() == bare
    assert sum(bare.values()) == cov["primaries"] - cov["backups"]

    # one all-pairs cost table and one LFA call per flag setting, then memoised
    n_lfa = [c for c in db._engine.calls if c[0] == "lfa"]
    assert len(n_lfa) == 2
    db.lfa_tables()
    db.find_routes_protected(pairs)
    assert len([c for c in db._engine.calls if c[0] == "lfa"]) == 2


def mutate(db, links, step):
    a, b = links[0]
    if step == "set_link_cost":
        db.set_link_cost(a, b, 5)
        db.set_link_cost(b, a, 5)
    elif step == "delete_link":
        db.delete_link(Link(Port(a, db.links[a][b].src.port_no), Port(b, 1)))
    elif step == "add_link":
        u, v = links[1][0], links[-1][0]
        if v not in db.links.get(u, {}) and u != v:
            db.add_link(Link(Port(u, 900), Port(v, 901)))
            db.add_link(Link(Port(v, 901), Port(u, 900)))


@pytest.mark.parametrize("name", ["fat_tree_k4", "random_V12"])
def test_dropin_follows_cost_and_link_changes(name):
    g = G.Golden(name)
    fabric = g.fabric()
    pairs = golden_pairs(g, fabric)
    db = fake_db(fabric)
    links = sorted((a, b) for a in db.links for b in db.links[a])
    before = dropin_state(db, pairs)
    done = []
    for step in ("set_link_cost", "delete_link", "add_link"):
        mutate(db, links, step)
        done.append(step)
        fresh = fake_db(fabric)
        for s in done:
            mutate(fresh, links, s)
        got = dropin_state(db, pairs)
        assert got == dropin_state(fresh, pairs), step
    assert got != before
    # find_route and the least-cost route are untouched by the LFA methods
    assert db.find_routes(pairs) == fresh.find_routes(pairs)
    assert db.find_routes_least_cost(pairs) == fresh.find_routes_least_cost(pairs)


def test_dropin_refuses_what_does_not_fit():
    fabric = T.fat_tree(4)
    db = fake_db(fabric, table_budget=12 * 20 * 19)       # 19 of the 20 rows
    with pytest.raises(ValueError) as ei:
        db.lfa_tables()
    assert "table budget" in str(ei.value)
    assert not [c for c in db._engine.calls if c[0] == "lfa"]
