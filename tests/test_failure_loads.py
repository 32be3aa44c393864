"""Link-failure what-if loads, CPU only: engine.failure_ecmp_link_loads_host
(the checker of failure_loads.hip) against route sets enumerated on a graph
rebuilt without the failed links (engine.least_cost_paths_lex per pair; the hop
split by a recursive walk); the named small cases; the drop-in over an engine
double built from the restatements, against a second TopologyDB whose links
were really deleted.

Tolerance: that of test_ecmp_link_loads.py (every term of a load is
non-negative: rtol = 1e-9, atol = 0, exactly 0.0 where 0 is expected); the
dyadic cases are compared bit for bit."""
import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import FailureLoads, SplitLinkLoads, TopologyDB
from test_cost_ecmp_loads import (FakeCostEcmpEngine, both_ways, digraph_csr, edge_costs,
                                  pcost_rows, random_costs)
from test_ecmp_link_loads import SPLITS, close, dicts_close, edge_map, route_set_loads
from test_link_loads import golden_pairs

INF = EN.COST_INF


class FakeFailureEngine(FakeCostEcmpEngine):
    """The restatement double plus failure_ecmp_link_loads."""

    def failure_ecmp_link_loads(self, export, cost, dsts, rows, srcs, weights=None,
                                scenarios=(), split="route", timing=False):
        self.calls.append(("failure", export.key, len(scenarios)))
        return EN.failure_ecmp_link_loads_host(export.csr, cost, dsts, rows, srcs, weights,
                                               scenarios, split)


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeFailureEngine()
    return db


# ------------------------------------------------- enumeration on a rebuilt graph --

def esrc_of(csr):
    return np.repeat(np.arange(int(csr.V)), np.diff(csr.row_ptr))


def rebuilt_without(csr, cost, failed):
    """(csr, cost) rebuilt from the link LIST without the failed edge indices."""
    esrc = esrc_of(csr)
    dead = set(int(e) for e in failed)
    live = [e for e in range(int(csr.E)) if e not in dead]
    red = T.build_csr(csr.dpids[esrc[live]], csr.dpids[np.asarray(csr.col)[live]],
                      np.asarray(csr.port)[live], extra_vertices=csr.dpids)
    at = edge_map(red)
    c = np.zeros(int(red.E), np.uint32)
    for e in live:
        c[at[(int(esrc[e]), int(csr.col[e]))]] = cost[e]
    return red, c


def enum_failure_loads(csr, cost, dsts, rows, srcs, weights, failed, split):
    """(load [E], lost, routed [n]) of one scenario by per-pair enumeration on
    the rebuilt graph: the route split over engine.least_cost_paths_lex's list,
    the hop split by dividing the weight at every vertex of a recursive walk."""
    V = int(csr.V)
    red, rcost = rebuilt_without(csr, cost, failed)
    pc = pcost_rows(red, rcost, dsts)
    edge = edge_map(csr)
    load = np.zeros(int(csr.E))
    routed = np.zeros(len(rows), bool)
    lost = 0.0
    rp, col = red.row_ptr, red.col

    def walk(row, x, f):
        if pc[row, x] == 0:
            return
        nxt = [int(col[e]) for e in range(int(rp[x]), int(rp[x + 1]))
               if pc[row, col[e]] != INF and int(pc[row, col[e]]) + int(rcost[e]) == int(pc[row, x])]
        for n in nxt:
            load[edge[(x, n)]] += f / len(nxt)
            walk(row, n, f / len(nxt))

    for i, (r, s) in enumerate(zip(rows, srcs)):
        r, s, d = int(r), int(s), int(dsts[int(r)])
        w = 1 if weights is None else int(weights[i])
        if not 0 <= s < V:
            continue
        if not 0 <= d < V or pc[r, s] == INF:
            lost += float(w) if s != d else 0.0
            continue
        routed[i] = True
        if s == d or not w:
            continue
        if split == "hop":
            walk(r, s, float(w))
            continue
        routes = EN.least_cost_paths_lex(rp, col, rcost, pc[r], s, d)
        for q in routes:
            for a, b in zip(q[:-1], q[1:]):
                load[edge[(a, b)]] += float(w) / len(routes)
    return load, lost, routed


def check_host(csr, cost, dsts, rows, srcs, w, scen):
    """The restatement against the enumeration, both splits, with and without
    the weights; returns the restatement's weighted results per split."""
    out = {}
    for split in SPLITS:
        for wt in (w, None):
            load, lost, routed = EN.failure_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, wt,
                                                                 scen, split)
            assert load.shape == (len(scen), int(csr.E)) and load.dtype == np.float64
            assert routed.shape == (len(scen), len(rows)) and routed.dtype == bool
            for k, failed in enumerate(scen):
                el, elost, erouted = enum_failure_loads(
                    csr, np.ones(int(csr.E), np.uint32) if cost is None else cost, dsts, rows,
                    srcs, wt, failed, split)
                assert close(load[k], el), (split, k)
                assert not load[k][np.asarray(failed, np.int64)].any()
                assert np.array_equal(routed[k], erouted), (split, k)
                assert close([lost[k]], [elost]), (split, k)
            if wt is not None:
                out[split] = (load, lost, routed)
    return out


def cable_edges(csr):
    """The cables of a graph as lists of edge indices (one or two directions),
    ascending by (min, max) vertex."""
    edge = edge_map(csr)
    cables = {}
    for (u, v), e in edge.items():
        cables.setdefault((min(u, v), max(u, v)), []).append(e)
    return [sorted(cables[k]) for k in sorted(cables)]


def switch_edges(csr, x):
    esrc = esrc_of(csr)
    return np.nonzero((esrc == x) | (np.asarray(csr.col) == x))[0].tolist()


def small_case(name, k):
    """A G.SMALL fabric with costs in [1, 5], every destination row, 2 random
    sources per row (ids outside [0, V) and s == d among them), u32 weights,
    and its scenarios: every single cable where there are at most 40, else 8
    sampled ones, plus every link of one switch."""
    csr = G.Golden(name).fabric().csr()
    V = int(csr.V)
    cost = random_costs(csr, 1, 5, 400 + k)
    rng = np.random.default_rng(410 + k)
    dsts = np.arange(V)
    rows = np.repeat(np.arange(V), 2)
    srcs = rng.integers(-1, V + 1, 2 * V)
    srcs[::9] = rows[::9]
    srcs[1], srcs[4] = -1, V
    w = rng.integers(0, 1 << 32, 2 * V, dtype=np.uint64)
    w[rng.random(2 * V) < 0.2] = 0
    cables = cable_edges(csr)
    if len(cables) > 40:
        cables = [cables[i] for i in sorted(rng.choice(len(cables), 8, replace=False).tolist())]
    scen = cables + [switch_edges(csr, int(rng.integers(0, V)))]
    return csr, cost, dsts, rows, srcs, w, scen


@pytest.mark.parametrize("k,name", list(enumerate(G.SMALL)))
def test_small_fabrics_equal_the_enumeration_on_the_rebuilt_graph(k, name):
    csr, cost, dsts, rows, srcs, w, scen = small_case(name, k)
    got = check_host(csr, cost, dsts, rows, srcs, w, scen)
    assert got["route"][0].any()
    assert ((srcs < 0) | (srcs >= csr.V)).any() and (srcs == rows).any()


# ------------------------------------------------------------ the named cases --

def trap_case(chord=False):
    """The diamond s -> {a, b} -> d at unit costs with s -> a failed: s -> a
    stays tight (pcost[a] + 1 == pcost[s] through b).  ``chord``: a direct link
    s -> d of cost 2 ties the two-link routes, so a's level is shared by d."""
    s, a, b, d = 0, 1, 2, 3
    und = [(s, a), (s, b), (a, d), (b, d)] + ([(s, d)] if chord else [])
    csr = digraph_csr(both_ways(und))
    cost = edge_costs(csr, {(s, d): 2, (d, s): 2} if chord else {})
    edge = edge_map(csr)
    return csr, cost, edge, (s, a, b, d)


@pytest.mark.parametrize("chord", [False, True])
def test_the_trap_a_failed_link_that_stays_tight_carries_nothing(chord):
    csr, cost, edge, (s, a, b, d) = trap_case(chord)
    scen = [[edge[(s, a)]], []]
    got = check_host(csr, cost, [d], [0, 0], [s, a], np.array([8, 4], np.uint64), scen)
    for split in SPLITS:
        load, lost, routed = got[split]
        want = np.zeros(int(csr.E))
        if chord:                                          # s - b - d and s - d, halves
            want[[edge[(s, b)], edge[(b, d)], edge[(s, d)]]] = 4.0
        else:
            want[[edge[(s, b)], edge[(b, d)]]] = 8.0
        want[edge[(a, d)]] = 4.0
        assert np.array_equal(load[0], want), split
        assert load[0][edge[(s, a)]] == 0.0 and routed.all() and not lost.any()
        assert load[1][edge[(s, a)]] > 0                   # intact: s -> a carries its share
    # the unmasked push over masked cost rows is what must not happen
    red, rcost = rebuilt_without(csr, cost, scen[0])
    pc = pcost_rows(red, rcost, [d])
    naive = EN.cost_ecmp_link_loads_host(csr, cost, pc, [0], [s], [8])
    assert naive[edge[(s, a)]] > 0


def cut_case():
    csr = digraph_csr(both_ways([(0, 1), (1, 2)]))
    edge = edge_map(csr)
    # a -> c, b -> c, c -> a
    return csr, edge, [2, 0], [0, 0, 1], [0, 1, 2], np.array([3, 5, 7], np.uint64)


def test_cut_failures_are_directed():
    csr, edge, dsts, rows, srcs, w = cut_case()
    got = check_host(csr, None, dsts, rows, srcs, w, [[edge[(1, 2)]]])
    for split in SPLITS:
        load, lost, routed = got[split]
        assert routed.tolist() == [[False, False, True]] and lost.tolist() == [8.0]
        want = np.zeros(int(csr.E))
        want[[edge[(2, 1)], edge[(1, 0)]]] = 7.0
        assert np.array_equal(load[0], want)


def ring_case():
    """A ring of 6 at unit costs with a chord 2 - 4 of cost 2 tying 2 - 3 - 4;
    every vertex sends to 0 and to 4."""
    csr = digraph_csr(both_ways([(v, (v + 1) % 6) for v in range(6)] + [(2, 4)]))
    cost = edge_costs(csr, {(2, 4): 2, (4, 2): 2})
    edge = edge_map(csr)
    scen = [sorted([edge[(0, 1)], edge[(1, 0)]]), [edge[(2, 3)]], [edge[(2, 4)]],
            sorted([edge[(0, 1)], edge[(1, 0)], edge[(3, 4)]]), []]
    rows = np.repeat([0, 1], 6)
    srcs = np.tile(np.arange(6), 2)
    w = np.arange(1, 13).astype(np.uint64) * np.uint64(16)
    return csr, cost, edge, [0, 4], rows, srcs, w, scen


def test_ring_the_longer_way_round_and_a_tied_direct_link():
    csr, cost, edge, dsts, rows, srcs, w, scen = ring_case()
    got = check_host(csr, cost, dsts, rows, srcs, w, scen)
    load, lost, routed = got["route"]
    assert routed.all() and not lost.any()
    # vertex 1 reaches 0 the long way: five links, each carries its 32
    for a, b in [(1, 2), (4, 5), (5, 0)]:
        assert load[0][edge[(a, b)]] >= 32.0
    assert load[0][edge[(1, 0)]] == 0.0 and load[4][edge[(1, 0)]] >= 32.0
    # toward 4 from 2: 2 - 3 - 4 ties the chord; with one failed the other takes all
    two = float(w[6 + 2])
    assert load[4][edge[(2, 4)]] == load[4][edge[(2, 3)]]
    assert load[1][edge[(2, 3)]] == 0.0 and load[1][edge[(2, 4)]] >= two
    assert load[2][edge[(2, 4)]] == 0.0 and load[2][edge[(2, 3)]] >= two


def star_case():
    """Hub 0 with 100 leaves: 70 of the hub's out-links failed (more than a
    wave has lanes), and every in-link of leaf 80."""
    csr = digraph_csr(both_ways([(0, v) for v in range(1, 101)]))
    edge = edge_map(csr)
    scen = [[edge[(0, v)] for v in range(1, 71)], [edge[(0, 80)]]]
    dsts = [5, 80, 0, 99]
    rows = np.repeat(np.arange(4), 101)
    srcs = np.tile(np.arange(101), 4)
    w = np.random.default_rng(7).integers(1, 1 << 20, rows.shape[0], dtype=np.uint64)
    return csr, edge, dsts, rows, srcs, w, scen


def test_star_with_70_failed_links_at_one_vertex():
    csr, edge, dsts, rows, srcs, w, scen = star_case()
    got = check_host(csr, None, dsts, rows, srcs, w, scen)
    load, lost, routed = got["route"]
    assert csr.row_ptr[1] == 100 and len(scen[0]) == 70
    r = routed.reshape(2, 4, 101)
    assert r[0, 0].sum() == 1 and r[0, 0, 5]               # leaf 5 is cut off from all but itself
    assert r[0, 1].all() and r[0, 2].all() and r[0, 3].all()
    assert r[1, 1].sum() == 1 and r[1, 0].all()
    assert lost[0] == float(w[:101].sum() - w[5]) and lost[1] == float(w[101:202].sum() - w[181])


# ---------------------------------------------------------- argument handling --

def test_empty_scenario_duplicates_and_no_scenarios():
    csr, cost, dsts, rows, srcs, w, scen = small_case("fat_tree_k4", 1)
    pc = pcost_rows(csr, cost, dsts)
    for split in SPLITS:
        want = EN.cost_ecmp_link_loads_host(csr, cost, pc, rows, srcs, w, split)
        load, lost, routed = EN.failure_ecmp_link_loads_host(
            csr, cost, dsts, rows, srcs, w, [[], scen[0], scen[0] + scen[0][::-1]], split)
        assert np.array_equal(load[0], want) and not lost.any()
        assert np.array_equal(load[1], load[2]) and np.array_equal(routed[1], routed[2])
        assert not np.array_equal(load[1], load[0])
        ok = (srcs >= 0) & (srcs < csr.V)
        assert np.array_equal(routed[0], ok)
    load, lost, routed = EN.failure_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, [])
    assert load.shape == (0, csr.E) and lost.shape == (0,) and routed.shape == (0, len(rows))
    # no costs: hop-count ECMP
    from oracle import oracle as O
    dist, _, _ = O.dest_tables(csr, np.arange(csr.V, dtype=np.int32))
    load, _, _ = EN.failure_ecmp_link_loads_host(csr, None, dsts, rows, srcs, w, [[]])
    assert close(load[0], EN.ecmp_link_loads_host(csr, dist, rows, srcs, w))
    assert EN.normalise_scenarios([[3, 1, 3], []], 4)[0].tolist() == [1, 3]
    for bad in ([[csr.E]], [[-1]]):
        with pytest.raises(ValueError):
            EN.failure_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, bad)
    with pytest.raises(ValueError):
        EN.failure_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, [[]], "flow")
    with pytest.raises(ValueError):
        EN.failure_ecmp_link_loads_host(csr, cost, dsts, [csr.V], [0], None, [[]])
    assert EN.FAILURE_LDS_MAX_V == 7100


def test_null_context_and_symbol():
    from sdnmpi_amd import _native
    L = _native.library()
    assert "sdnr_failure_ecmp_link_loads" in _native.EXPORTED_SYMBOLS
    assert L.sdnr_failure_ecmp_link_loads(None, None, 0, None, None, None, 0, None, None, None,
                                          None, None, _native.DEVICE_PTRS) == -22


# ------------------------------------------------------------------ the drop-in --

def deleted_twin(fabric, costs, scenario):
    """A second TopologyDB with the same switches, hosts, links and costs on
    which the links of ``scenario`` were really removed with delete_link."""
    db = fake_db(fabric)
    if costs:
        db.set_link_costs(costs)
    for a, b in scenario:
        if a in db.links and b in db.links[a]:
            db.delete_link(db.links[a][b])
    return db


def dropin_case(name, with_costs):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    rng = np.random.default_rng(len(name))
    links = [(u, v) for u in sorted(db.links) for v in sorted(db.links[u])]
    costs = {}
    if with_costs:
        some = [links[i] for i in rng.choice(len(links), max(1, len(links) // 4), replace=False)]
        costs = {k: int(c) for k, c in zip(some, rng.integers(2, 4, len(some)))}
        db.set_link_costs(costs)
    cables = db.cable_failures()
    pick = sorted(rng.choice(len(cables), min(5, len(cables)), replace=False).tolist())
    sw = sorted(db.switches)[int(rng.integers(0, len(db.switches)))]
    failures = [cables[i] for i in pick] + [db.switch_links(sw), (),
                                            [(10 ** 9, 1), links[0], links[0]]]
    macs = fabric.host_macs()
    pairs = golden_pairs(g, fabric) + [(macs[0], "02:00:00:00:ff:ff"), (macs[0], macs[0])]
    w = rng.integers(0, 1 << 32, len(pairs)).tolist()
    return fabric, db, costs, failures, pairs, w


@pytest.mark.parametrize("name,with_costs", [("fat_tree_k4", False), ("random_V12", False),
                                             ("torus_2x2x2", True)])
def test_dropin_equals_a_twin_with_the_links_really_deleted(name, with_costs):
    fabric, db, costs, failures, pairs, w = dropin_case(name, with_costs)
    links_before = db.links
    snap = {u: dict(nb) for u, nb in db.links.items()}
    ex = db.graph()
    routes_before = [db.find_route(a, b) for a, b in pairs[:20]]
    for split in SPLITS:
        got = db.failure_link_loads(failures, pairs, w, split)
        assert isinstance(got, FailureLoads) and len(got) == len(failures)
        assert got.load.shape == (len(failures), ex.csr.E) and got.load.dtype == np.float64
        assert got.lost.dtype == np.uint64
        assert got.scenarios[-1] == (failures[-1][1],)      # missing ignored, duplicates once
        assert got.scenarios[-2] == ()
        assert dicts_close(got.base.as_dict(),
                           db.least_cost_ecmp_link_loads(pairs, w, split).as_dict())
        assert dicts_close(got.scenario(len(failures) - 2).as_dict(), got.base.as_dict())
        for k, sc in enumerate(failures):
            twin = deleted_twin(fabric, costs, sc)
            one = got.scenario(k)
            assert isinstance(one, SplitLinkLoads)
            assert dicts_close(one.as_dict(),
                               twin.least_cost_ecmp_link_loads(pairs, w, split).as_dict()), k
            sets = twin.find_routes_least_cost(pairs, multiple=True)
            if split == "route":
                assert dicts_close(one.as_dict(), route_set_loads(sets, w)), k
            known = [db._endpoint(a) is not None and db._endpoint(b) is not None
                     for a, b in pairs]
            assert int(got.lost[k]) == sum(x for x, r, ok in zip(w, sets, known) if ok and not r)
        top, at = got.worst()
        assert np.array_equal(top, got.load.max(0)) and at.dtype == np.int64
        assert np.array_equal(got.load[at, np.arange(ex.csr.E)], top)
        assert all((got.load[:k, e] < top[e]).all() for e, k in enumerate(at.tolist()))
        wd = got.worst_dict()
        assert len(wd) == int((top != 0).sum())
        for (d, p), (x, k) in wd.items():
            assert got.scenario(k).as_dict()[(d, p)] == x
    # nothing of the live object changed
    assert db.links is links_before and {u: dict(nb) for u, nb in db.links.items()} == snap
    assert db.graph() is ex and db._link_costs == costs
    assert [db.find_route(a, b) for a, b in pairs[:20]] == routes_before


@pytest.mark.parametrize("split", SPLITS)
def test_all_pairs_mpi_forms_and_scenario_chunks(split):
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    ex = db.graph()
    e_sw = int(ex.csr.dpids[ex.host_vertices()[0]])
    failures = db.cable_failures()[:6] + [db.switch_links(e_sw), db.cable(e_sw, 10 ** 9)]
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs for b in macs if a != b]
    allp = db.all_pairs_failure_link_loads(failures, split)
    byp = db.failure_link_loads(failures, pairs, None, split)
    assert np.array_equal(allp.lost, byp.lost) and allp.scenarios == byp.scenarios
    for k in range(len(failures)):
        assert dicts_close(allp.scenario(k).as_dict(), byp.scenario(k).as_dict()), k
    # the edge switch is isolated: its hosts still reach each other, nobody else does
    on_sw = sum(1 for h in db.hosts.values() if h.port.dpid == e_sw)
    assert int(byp.lost[6]) == 2 * on_sw * (len(macs) - on_sw) and not byp.lost[:6].any()
    assert any(k[0] == e_sw for k in byp.scenario(6).as_dict())
    ranks = {r: m for r, m in enumerate(macs[:6])}
    mp = db.mpi_failure_link_loads(failures, ranks, None, split)
    rp = db.failure_link_loads(failures, [(ranks[i], ranks[j]) for i in ranks for j in ranks
                                          if i != j], None, split)
    assert np.array_equal(mp.load, rp.load) and np.array_equal(mp.lost, rp.lost)
    # scenario chunks under a small budget: two scenarios per engine call
    small = fake_db(fabric, table_budget=2 * (8 * int(ex.csr.E) + len(ex.host_vertices()) ** 2))
    got = small.all_pairs_failure_link_loads(failures, split)
    assert np.array_equal(got.load, allp.load) and np.array_equal(got.lost, allp.lost)
    assert sum(1 for c in small.engine.calls if c[0] == "failure") == 4
    none = db.failure_link_loads([], pairs, None, split)
    assert none.load.shape == (0, ex.csr.E) and none.worst()[1].tolist() == [-1] * ex.csr.E
    assert none.worst_dict() == {} and dicts_close(none.base.as_dict(), byp.base.as_dict())
    with pytest.raises(ValueError):
        db.failure_link_loads(failures, pairs, None, "flow")
    with pytest.raises(IndexError):
        byp.scenario(len(failures))
