"""Remote loop-free alternates (PQ-node repair tunnels per link), CPU only:
engine.remote_lfa_host (the checker of remote_lfa.hip) against the definition
by enumeration -- "no least-cost route uses the link S -> E as consecutive
vertices", over engine.least_cost_paths_lex's route lists, and "the repair
delivers" --, the named small cases with their tables written out, the pinned
coverage figures, the vertex-list semantics and the drop-in over an engine
double built from the restatements.  Everything is integer: every comparison
is exact."""
import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import TopologyDB
from test_cost_ecmp_loads import both_ways, digraph_csr, random_costs
from test_ecmp_link_loads import edge_map
from test_lfa_tables import (BIG, ENUM_FABRICS, FakeLfaEngine, all_pairs, dropin_state, mutate)
from test_link_loads import golden_pairs

INF = EN.COST_INF
NAMES = ("pq", "via", "via_port", "tunnel_cost", "kind", "counts")
DTYPES = (np.int32, np.int32, np.int32, np.uint64, np.uint8, np.uint32)


class FakeRemoteLfaEngine(FakeLfaEngine):
    """The restatement double plus remote_lfa."""

    def remote_lfa(self, export, cost, pcost_all, verts=None, timing=False):
        self.calls.append(("rlfa", export.key, None if verts is None else len(verts)))
        return EN.remote_lfa_host(export.csr, cost, pcost_all, verts)


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeRemoteLfaEngine()
    return db


def same(got, want):
    """The six arrays equal, in value, shape and type."""
    for a, b, name, dt in zip(got, want, NAMES, DTYPES):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == dt and b.dtype == dt, name
        assert a.shape == b.shape and np.array_equal(a, b), name


def edge_src(csr):
    return np.repeat(np.arange(int(csr.V)), np.diff(csr.row_ptr))


# -------------------------------------------------- the definition, enumerated --

def uses(paths, s, t):
    """Some route of the list has s, t as consecutive vertices."""
    return any(any(q[i] == s and q[i + 1] == t for i in range(len(q) - 1)) for q in paths)


def enum_remote_lfa(csr, cost, P, nh):
    """{edge: (tunnel cost, X, N)} from the definition -- the routes of
    engine.least_cost_paths_lex decide the Q-space and the extended P-space --
    and, per repaired link, whether every destination whose primary is the
    link is reached from X without it."""
    V = int(csr.V)
    rp, col = csr.row_ptr, csr.col
    paths = {}

    def routes(a, b):
        if a == b:
            return [[a]]
        if (a, b) not in paths:
            paths[(a, b)] = (EN.least_cost_paths_lex(rp, col, cost, P[b], a, b)
                             if P[b, a] != INF else [])
        return paths[(a, b)]

    out = {}
    for s in range(V):
        row = range(int(rp[s]), int(rp[s + 1]))
        for e in row:
            t = int(col[e])
            if t == s:
                continue
            best = None
            for x in range(V):
                if x == s or not routes(x, t) or uses(routes(x, t), s, t):
                    continue
                for f in row:
                    n = int(col[f])
                    if n in (s, t) or not routes(n, x) or uses(routes(n, x), s, t):
                        continue
                    key = (int(cost[f]) + int(P[x, n]), x, n)
                    if best is None or key < best:
                        best = key
            if best is None:
                continue
            out[e] = best
            for d in range(V):                             # the repair delivers
                if nh[d, s] == t and best[1] != d:
                    assert routes(best[1], d) and not uses(routes(best[1], d), s, t)
    return out


@pytest.mark.parametrize("hi", [1, 3])
@pytest.mark.parametrize("name", ENUM_FABRICS)
def test_restatement_equals_the_enumerated_definition(name, hi):
    csr = G.Golden(name).fabric().csr()
    V = int(csr.V)
    cost = random_costs(csr, 1, hi, 7 * V + hi)
    P, nh = EN.cost_tables_host(csr, cost, np.arange(V))[:2]
    pq, via, vport, tc, kind, counts = got = EN.remote_lfa_host(csr, cost, P)
    for a, dt in zip(got, DTYPES):
        assert a.dtype == dt
    want = enum_remote_lfa(csr, cost, P, nh)
    assert set(np.nonzero(kind & 1)[0].tolist()) == set(want)
    for e, (c, x, n) in want.items():
        assert (int(tc[e]), int(pq[e]), int(via[e])) == (c, x, n)
    check_derived(csr, cost, P, got)


def check_derived(csr, cost, P, got):
    """via_port, the kind bits 2 and 4, the empty entries and the counts, from
    pq / via / kind & 1 and the table."""
    pq, via, vport, tc, kind, counts = got
    V = int(csr.V)
    src, edge = edge_src(csr), edge_map(csr)
    D = lambda a, b: int(P[b, a])                          # noqa: E731
    want_counts = np.zeros((V, 4), np.int64)
    for e in range(int(csr.E)):
        s, t, c = int(src[e]), int(csr.col[e]), int(cost[e])
        want_counts[s, 0] += t != s
        if not kind[e] & 1:
            assert (pq[e], via[e], vport[e], tc[e], kind[e]) == (-1, -1, -1, 0, 0)
            continue
        x, n = int(pq[e]), int(via[e])
        assert t != s and x != s and n not in (s, t)
        assert vport[e] == csr.port[edge[(s, n)]]
        assert int(tc[e]) == int(cost[edge[(s, n)]]) + D(n, x)
        plain = D(s, x) != INF and (D(t, x) == INF or D(s, x) < c + D(t, x))
        assert kind[e] == 1 | (2 if plain else 0) | (4 if x == n else 0)
        want_counts[s, 1:] += [1, plain, x == n]
    assert np.array_equal(counts, want_counts)


# ------------------------------------------------------------ the named cases --

def ring_case(n, pq_off, via_off, tcost, kind):
    """The n-ring with unit costs: link v -> v + 1 is repaired through
    v + via_off at v + pq_off, link v -> v - 1 is its mirror image."""
    csr = digraph_csr(both_ways([(i, (i + 1) % n) for i in range(n)]))
    want = {}
    for v in range(n):
        want[(v, (v + 1) % n)] = ((v + pq_off) % n, (v + via_off) % n, tcost, kind)
        want[(v, (v - 1) % n)] = ((v - pq_off) % n, (v - via_off) % n, tcost, kind)
    return csr, np.ones(int(csr.E), np.uint32), want


def named_case(name):
    """(csr, cost, {(s, e): (pq, via, tunnel cost, kind)}) of a named small
    graph, written out; a link that is absent has no repair."""
    ones = lambda csr: np.ones(int(csr.E), np.uint32)      # noqa: E731
    if name == "ring4":                          # 0 -> 1: through 3 to the antipode 2
        return ring_case(4, 2, 3, 2, 1)
    if name == "ring5":                          # the PQ node is in 0's own P-space
        return ring_case(5, 3, 4, 2, 3)
    if name == "ring6":
        return ring_case(6, 3, 5, 3, 1)
    if name == "ring8":
        return ring_case(8, 4, 7, 4, 1)
    if name == "triangle":                       # the third vertex is a per-link LFA
        csr = digraph_csr(both_ways([(0, 1), (1, 2), (0, 2)]))
        want = {(s, e): (3 - s - e, 3 - s - e, 1, 7) for s in range(3) for e in range(3)
                if s != e}
        return csr, ones(csr), want
    if name == "one_way":                        # 3 reaches neither 1 nor 0: nothing to tunnel to
        csr = digraph_csr([(0, 1), (1, 2), (0, 3), (3, 2)], 4)
        return csr, ones(csr), {}
    if name == "one_way_chord":
        # one_way plus 3 -> 1.  Link 0 -> 1: nothing comes back to 0, so 3 is in
        # the Q-space (D(3,0) INF) and in its own extended P-space (D(3,0) INF
        # again), and in 0's own P-space because D(1,3) is INF.  Link 3 -> 2
        # likewise falls back on 1 (D(1,3), D(2,1) INF).  Link 3 -> 1: only 2 is
        # reached through the other neighbour, and 2 does not reach 1
        csr = digraph_csr([(0, 1), (1, 2), (0, 3), (3, 2), (3, 1)], 4)
        return csr, ones(csr), {(0, 1): (3, 3, 1, 7), (3, 2): (1, 1, 1, 7)}
    if name == "two_components":                 # the pair 3 - 4 has no third vertex
        csr = digraph_csr(both_ways([(0, 1), (1, 2), (0, 2), (3, 4)]))
        want = {(s, e): (3 - s - e, 3 - s - e, 1, 7) for s in range(3) for e in range(3)
                if s != e}
        return csr, ones(csr), want
    if name == "degree_one":                     # 3 hangs off the triangle: 2 - 3 has no repair
        csr = digraph_csr(both_ways([(0, 1), (1, 2), (0, 2), (2, 3)]))
        want = {(s, e): (3 - s - e, 3 - s - e, 1, 7) for s in range(3) for e in range(3)
                if s != e}
        return csr, ones(csr), want
    if name == "big_triangle_one_way":
        # no link 2 -> 1, costs B = 2^31 - 1.  Link 1 -> 0: 2 is in the Q-space
        # because D(2,0) = B < D(2,1) + B = 3 B = 2^32 + 2^31 - 3; a 32-bit sum
        # would wrap to 2^31 - 3, below B, and lose the repair
        csr = digraph_csr([(1, 0), (1, 2), (2, 0), (0, 1), (0, 2)])
        want = {(0, 2): (1, 1, BIG, 7), (1, 0): (2, 2, BIG, 7), (1, 2): (0, 0, BIG, 7)}
        return csr, np.full(int(csr.E), BIG, np.uint32), want
    raise KeyError(name)


NAMED = ["ring4", "ring5", "ring6", "ring8", "triangle", "one_way", "one_way_chord",
         "two_components", "degree_one", "big_triangle_one_way"]


def named_tables(csr, cost, want):
    """The six arrays of a named case's written-out repairs."""
    V, E = int(csr.V), int(csr.E)
    src, edge = edge_src(csr), edge_map(csr)
    pq, via, vport = (np.full(E, -1, np.int32) for _ in range(3))
    tc, kind = np.zeros(E, np.uint64), np.zeros(E, np.uint8)
    counts = np.zeros((V, 4), np.uint32)
    np.add.at(counts[:, 0], src[src != csr.col], 1)
    for (s, t), (x, n, c, k) in want.items():
        e = edge[(s, t)]
        pq[e], via[e], vport[e], tc[e], kind[e] = x, n, csr.port[edge[(s, n)]], c, k
        counts[s, 1:] += np.asarray([1, k >> 1 & 1, k >> 2 & 1], np.uint32)
    return pq, via, vport, tc, kind, counts


@pytest.mark.parametrize("name", NAMED)
def test_named_cases(name):
    csr, cost, want = named_case(name)
    P = all_pairs(csr, cost)
    got = EN.remote_lfa_host(csr, cost, P)
    same(got, named_tables(csr, cost, want))
    check_derived(csr, cost, P, got)
    nh = EN.cost_tables_host(csr, cost, np.arange(int(csr.V)))[1]
    edge = edge_map(csr)
    assert {edge[k]: (v[2], v[0], v[1]) for k, v in want.items()} == \
        enum_remote_lfa(csr, cost, P, nh)


def repair_of(name, s, t):
    """(pq, via, tunnel cost, kind) the restatement gives link s -> t of a
    named case, and the case's all-pairs table."""
    csr, cost, _ = named_case(name)
    P = all_pairs(csr, cost)
    pq, via, _, tc, kind, _ = EN.remote_lfa_host(csr, cost, P)
    e = edge_map(csr)[(s, t)]
    return (int(pq[e]), int(via[e]), int(tc[e]), int(kind[e])), P


def test_the_restatement_on_what_the_named_cases_are_named_for():
    assert repair_of("ring4", 0, 1)[0] == (2, 3, 2, 1)
    assert repair_of("ring4", 1, 2)[0] == (3, 0, 2, 1)
    assert repair_of("ring5", 0, 1)[0] == (3, 4, 2, 3)
    assert repair_of("ring6", 0, 1)[0] == (3, 5, 3, 1)
    assert repair_of("ring8", 0, 1)[0] == (4, 7, 4, 1)
    for s, t in ((0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)):
        r, _ = repair_of("triangle", s, t)
        assert r[0] == r[1] == 3 - s - t and r[3] == 7
    r, P = repair_of("one_way_chord", 0, 1)               # every INF clause decides here
    assert r == (3, 3, 1, 7) and P[0, 3] == INF and P[3, 1] == INF and P[1, 2] == INF
    assert repair_of("degree_one", 2, 3)[0] == (-1, -1, 0, 0)
    assert repair_of("degree_one", 3, 2)[0] == (-1, -1, 0, 0)
    r, P = repair_of("big_triangle_one_way", 1, 0)        # lost by a 32-bit sum
    P = P.astype(np.int64)
    assert r == (2, 2, BIG, 7)
    assert P[1, 2] + BIG >= 2 ** 32 and (P[1, 2] + BIG) % 2 ** 32 < P[0, 2]


@pytest.mark.parametrize("name", G.LOOPS)
def test_self_loops_get_no_repair_and_change_no_other_link(name):
    loops = G.Golden(name).fabric().csr()
    plain = G.Golden(name[:-len("_loops")]).fabric().csr()
    assert np.array_equal(loops.dpids, plain.dpids) and int(loops.E) > int(plain.E)
    V = int(plain.V)
    for hi in (1, 3):
        ca = random_costs(plain, 1, hi, V + hi)
        cb = np.ones(int(loops.E), np.uint32)
        ea, eb = edge_map(plain), edge_map(loops)
        for k, e in ea.items():
            cb[eb[k]] = ca[e]
        a = EN.remote_lfa_host(plain, ca, all_pairs(plain, ca))
        b = EN.remote_lfa_host(loops, cb, all_pairs(loops, cb))
        at = np.asarray([eb[k] for k in ea], np.int64)
        order = np.asarray(list(ea.values()), np.int64)
        for x, y, what in zip(a[:5], b[:5], NAMES):
            assert np.array_equal(x[order], y[at]), what
        assert np.array_equal(a[5], b[5])
        self_loops = np.nonzero(edge_src(loops) == loops.col)[0]
        assert self_loops.size == int(loops.E) - int(plain.E)
        assert not b[4][self_loops].any() and (b[0][self_loops] == -1).all()
        assert (b[1][self_loops] == -1).all() and (b[2][self_loops] == -1).all()
        assert not b[3][self_loops].any()


# ------------------------------------------------------- the prototype's figures --

def coverage_figures(csr):
    """(primaries, primaries without an LFA, of those with a repaired primary
    link, links repaired, links) with unit costs."""
    V = int(csr.V)
    P, nh = EN.cost_tables_host(csr, np.ones(int(csr.E), np.uint32), np.arange(V))[:2]
    k = EN.lfa_tables_host(csr, None, P, np.arange(V), True)[2]
    rk = EN.remote_lfa_host(csr, None, P)[4]
    edge = edge_map(csr)
    dd, ss = np.nonzero((nh >= 0) & (k == 0))
    rep = sum(int(rk[edge[(int(s), int(nh[d, s]))]] & 1) for d, s in zip(dd, ss))
    return int((nh >= 0).sum()), int(dd.shape[0]), rep, int((rk & 1).sum()), int(csr.E)


def test_the_prototype_figures():
    assert coverage_figures(G.Golden("fat_tree_k4").fabric().csr()) == (380, 192, 192, 64, 64)
    assert coverage_figures(G.Golden("random_V12").fabric().csr()) == (121, 57, 7, 18, 26)
    # the fat-tree's PQ nodes are reached through a neighbour only: none lies in
    # the switch's own P-space
    csr = G.Golden("fat_tree_k4").fabric().csr()
    kind = EN.remote_lfa_host(csr, None, all_pairs(csr, np.ones(int(csr.E), np.uint32)))[4]
    assert (kind == 1).all()


# ------------------------------------------------------------ the vertex list --

def test_units_follow_the_vertex_list():
    csr = G.Golden("random_V12").fabric().csr()
    V, E = int(csr.V), int(csr.E)
    cost = random_costs(csr, 1, 4, 5)
    P = all_pairs(csr, cost)
    full = EN.remote_lfa_host(csr, cost, P)
    same(EN.remote_lfa_host(csr, cost, P, np.arange(V)), full)
    assert (full[4] != 0).any() and (full[4] == 0).any()
    verts = np.asarray([5, -1, 0, 5, V, 11])
    got = EN.remote_lfa_host(csr, cost, P, verts)
    src = edge_src(csr)
    mine = np.isin(src, [0, 5, 11])
    for a, f, name in zip(got[:5], full[:5], NAMES):
        assert np.array_equal(a[mine], f[mine]), name
        assert (a[~mine] == (-1 if a.dtype == np.int32 else 0)).all(), name     # untouched
    for i, v in enumerate(verts.tolist()):
        assert np.array_equal(got[5][i], full[5][v] if 0 <= v < V else [0, 0, 0, 0])
    assert got[5].shape == (6, 4)
    empty = EN.remote_lfa_host(csr, cost, P, [])
    assert empty[5].shape == (0, 4) and not empty[4].any() and (empty[0] == -1).all()
    assert empty[0].shape == (E,)
    with pytest.raises(ValueError):
        EN.remote_lfa_host(csr, cost, P[:-1])


def test_unit_costs_need_no_cost_vector():
    csr = G.Golden("fat_tree_k4").fabric().csr()
    ones = np.ones(int(csr.E), np.uint32)
    P = all_pairs(csr, ones)
    same(EN.remote_lfa_host(csr, None, P), EN.remote_lfa_host(csr, ones, P.view(np.int32)))


# ------------------------------------------------------------------ the drop-in --

def remote_state(db):
    """Everything the remote-LFA methods answer, for comparing two databases."""
    t = db.remote_lfa_tables()
    return ({k: v.tolist() for k, v in t.items()}, db.repair_tunnels(), db.remote_lfa_coverage(),
            db.unrepaired_links())


def rlfa_calls(db):
    return [c for c in db._engine.calls if c[0] == "rlfa"]


@pytest.mark.parametrize("name", ["fat_tree_k4", "random_V12", "dragonfly_a4_h2_p2"])
def test_dropin_over_the_engine_double(name):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    ex = db.graph()
    csr = ex.csr
    V, E = int(csr.V), int(csr.E)
    rng = np.random.default_rng(V)
    links = [(a, b) for a in db.links for b in db.links[a]]
    db.set_link_costs({links[i]: int(rng.integers(1, 4)) for i in
                       rng.choice(len(links), len(links) // 3, replace=False)})
    cost = db._cost_vector(ex)
    P, nh = EN.cost_tables_host(csr, cost, np.arange(V))[:2]
    want = EN.remote_lfa_host(csr, cost, P)
    src = edge_src(csr)
    dp = csr.dpids

    t = db.remote_lfa_tables()
    for key, w in zip(NAMES[:5], want[:5]):
        assert np.array_equal(t[key], w) and t[key].dtype == w.dtype, key
    assert np.array_equal(t["src"], src) and np.array_equal(t["dst"], csr.col)
    assert np.array_equal(t["dpids"], dp)

    tun = db.repair_tunnels()
    rep = np.nonzero(want[4] & 1)[0]
    assert len(tun) == rep.shape[0] > 0
    for e in rep.tolist():
        key = (int(dp[src[e]]), int(dp[csr.col[e]]))
        assert tun[key] == (int(dp[want[0][e]]), int(dp[want[1][e]]), int(want[2][e]),
                            int(want[3][e]), int(want[4][e]))
        assert db.links[key[0]][tun[key][1]].src.port_no == tun[key][2]

    # coverage: the primaries without an LFA whose primary link has a repair
    lk = EN.lfa_tables_host(csr, cost, P, np.arange(V), True)[2]
    edge = edge_map(csr)
    bare = [(int(s), int(nh[d, s])) for d, s in zip(*np.nonzero((nh >= 0) & (lk == 0)))]
    remote = sum(int(want[4][edge[k]] & 1) for k in bare)
    lcov = db.lfa_coverage(node_protect=False)
    cov = db.remote_lfa_coverage()
    assert cov == {"primaries": lcov["primaries"], "backups": lcov["backups"],
                   "remote_backups": remote,
                   "coverage_with_remote": (lcov["backups"] + remote) / lcov["primaries"],
                   "links": int((src != csr.col).sum()), "links_repaired": int(rep.shape[0]),
                   "links_plain": int((want[4] & 2 != 0).sum())}
    assert lcov["backups"] + len(bare) == lcov["primaries"]

    unrep = {}
    for s, n in bare:
        if not want[4][edge[(s, n)]] & 1:
            key = (int(dp[s]), int(dp[n]))
            unrep[key] = unrep.get(key, 0) + 1
    assert db.unrepaired_links() == unrep
    assert set(unrep) <= set(db.unprotected_links())
    assert sum(unrep.values()) == len(bare) - remote

    # one engine call, then memoised
    assert len(rlfa_calls(db)) == 1
    remote_state(db)
    assert len(rlfa_calls(db)) == 1


@pytest.mark.parametrize("name", ["fat_tree_k4", "random_V12"])
def test_dropin_follows_cost_and_link_changes(name):
    g = G.Golden(name)
    fabric = g.fabric()
    pairs = golden_pairs(g, fabric)
    db = fake_db(fabric)
    links = sorted((a, b) for a in db.links for b in db.links[a])
    before = remote_state(db)
    done = []
    for step in ("set_link_cost", "delete_link", "add_link"):
        mutate(db, links, step)
        done.append(step)
        fresh = fake_db(fabric)
        for s in done:
            mutate(fresh, links, s)
        got = remote_state(db)
        assert got == remote_state(fresh), step
    assert got != before and len(rlfa_calls(db)) > 1       # dropped with the memo
    # the other answers are what a database that never asked for a repair gives
    quiet = fake_db(fabric)
    for s in done:
        mutate(quiet, links, s)
    assert dropin_state(db, pairs) == dropin_state(quiet, pairs)
    assert db.find_routes(pairs) == quiet.find_routes(pairs)
    assert db.find_routes_least_cost(pairs) == quiet.find_routes_least_cost(pairs)
    assert not rlfa_calls(quiet)


def test_dropin_refuses_what_does_not_fit():
    fabric = T.fat_tree(4)
    db = fake_db(fabric, table_budget=12 * 20 * 19)       # 19 of the 20 rows
    for ask in (db.remote_lfa_tables, db.repair_tunnels, db.remote_lfa_coverage,
                db.unrepaired_links):
        with pytest.raises(ValueError) as ei:
            ask()
        assert "table budget" in str(ei.value)
    assert not rlfa_calls(db) and not [c for c in db._engine.calls if c[0] == "lfa"]
