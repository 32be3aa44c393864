"""Link-cost what-if loads and the cost tuner, CPU only:
engine.whatif_ecmp_link_loads_host (the checker of whatif_loads.hip) against
route sets enumerated on a graph rebuilt with the changed costs and without the
links that are down (test_failure_loads.enum_failure_loads); the drop-in over
an engine double built from the restatements, against a second TopologyDB on
which the changes were really made; the tuner on the fish.

Tolerance: that of test_ecmp_link_loads.py (rtol = 1e-9, atol = 0, exactly 0.0
where 0 is expected); the dyadic cases are compared bit for bit."""
import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import (CostChangeLoads, CostTuning, FailureLoads,
                                         SplitLinkLoads, TopologyDB)
from test_cost_ecmp_loads import random_costs
from test_ecmp_link_loads import SPLITS, close, dicts_close
from test_failure_loads import (FakeFailureEngine, dropin_case, enum_failure_loads, ring_case,
                                small_case, trap_case)

INF = EN.COST_INF


class FakeWhatifEngine(FakeFailureEngine):
    """The restatement double plus whatif_ecmp_link_loads."""

    def whatif_ecmp_link_loads(self, export, cost, dsts, rows, srcs, weights=None, scenarios=(),
                               split="route", capacity=None, loads=True, reach=True,
                               timing=False, table_budget=None):
        self.calls.append(("whatif", export.key, len(scenarios), loads, reach))
        load, lost, routed, peak, pe = EN.whatif_ecmp_link_loads_host(
            export.csr, cost, dsts, rows, srcs, weights, scenarios, split, capacity)
        return (load if loads else None, lost if reach else None,
                routed if loads and reach else None, peak, pe)


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeWhatifEngine()
    return db


def cost_scenarios(csr, cost, lists, seed, hi):
    """Per edge list of ``lists`` one cost scenario over those links: a third
    of them down, the others at a random cost in [1, hi] (raised, lowered or
    as it is); plus the empty scenario."""
    rng = np.random.default_rng(seed)
    out = []
    for es in lists:
        es = np.unique(np.asarray(es, np.int64))
        c = rng.integers(1, hi + 1, es.shape[0]).astype(np.int64)
        c[rng.random(es.shape[0]) < 1 / 3] = INF
        perm = rng.permutation(es.shape[0])                # (given unsorted)
        out.append((es[perm], c[perm]))
    return out + [([], [])]


def changed(csr, cost, sc):
    """(cost vector in force, indices of the links that are down) of one scenario."""
    now = (np.ones(int(csr.E), np.uint32) if cost is None else np.asarray(cost, np.uint32)).copy()
    now[np.asarray(sc[0], np.int64)] = np.asarray(sc[1], np.int64).astype(np.uint32)
    return now, np.nonzero(now == INF)[0]


def check_host(csr, cost, dsts, rows, srcs, w, scen, capacity=None):
    """The restatement against the enumeration on the rebuilt graph, both
    splits, with and without the weights; returns the weighted results."""
    out = {}
    for split in SPLITS:
        for wt in (w, None):
            load, lost, routed, peak, pe = EN.whatif_ecmp_link_loads_host(
                csr, cost, dsts, rows, srcs, wt, scen, split, capacity)
            assert load.shape == (len(scen), int(csr.E)) and load.dtype == np.float64
            assert peak.dtype == np.float64 and pe.dtype == np.int32
            for k, sc in enumerate(scen):
                now, down = changed(csr, cost, sc)
                live = np.where(now == INF, 1, now)         # (removed before anything reads them)
                el, elost, erouted = enum_failure_loads(csr, live, dsts, rows, srcs, wt, down,
                                                        split)
                assert close(load[k], el), (split, k)
                assert not load[k][down].any()
                assert np.array_equal(routed[k], erouted) and close([lost[k]], [elost])
                u = load[k] if capacity is None else load[k] / capacity
                assert peak[k] == (u.max() if u.size else 0.0)
                assert pe[k] == (int(u.argmax()) if peak[k] > 0 else -1)
            if wt is not None:
                out[split] = (load, lost, routed, peak, pe)
    return out


@pytest.mark.parametrize("hi", [5, 200])
@pytest.mark.parametrize("k,name", list(enumerate(G.SMALL)))
def test_small_fabrics_equal_the_enumeration_on_the_rebuilt_graph(k, name, hi):
    csr, _, dsts, rows, srcs, w, lists = small_case(name, k)
    cost = random_costs(csr, 1, hi, 500 + k)
    scen = cost_scenarios(csr, cost, lists, 510 + k, hi)
    cap = np.random.default_rng(k).uniform(0.5, 4.0, int(csr.E))
    got = check_host(csr, cost, dsts, rows, srcs, w, scen, cap if hi == 5 else None)
    assert got["route"][0].any() and got["route"][3].any()
    assert any((np.asarray(c) == INF).any() for _, c in scen[:-1])
    assert any((np.asarray(c) < cost[np.asarray(e)]).any() for e, c in scen[:-1])   # lowered
    assert any((np.asarray(c) > cost[np.asarray(e)]).any() for e, c in scen[:-1])   # raised


def lowered_ring_case():
    """ring_case with 0 -> 5 uploaded at cost 3 and overridden to 1: toward 4,
    vertex 1 then has the long way round 1 - 0 - 5 - 4 (cost 3) beside 1 - 2 - 4
    and 1 - 2 - 3 - 4; at the uploaded cost 1 -> 0 carries nothing toward 4."""
    csr, cost, edge, dsts, rows, srcs, w, _ = ring_case()
    cost = cost.copy()
    cost[edge[(0, 5)]] = 3
    keep = rows == 1                                       # the pairs toward 4
    return csr, cost, edge, dsts, rows[keep], srcs[keep], w[keep], [([edge[(0, 5)]], [1]),
                                                                    ([], [])]


def raised_chord_case():
    """The diamond s -> {a, b} -> d with a direct unit link s -> d, raised to 2:
    it ties the two-link routes, the next hops of s sit at two depths."""
    csr, _, edge, (s, a, b, d) = trap_case(chord=True)
    cost = np.ones(int(csr.E), np.uint32)
    return csr, cost, edge, (s, a, b, d), [([edge[(s, d)]], [2]), ([], [])]


def test_named_cases_lowered_raised_to_a_tie_and_the_trap():
    csr, cost, edge, dsts, rows, srcs, w, scen = lowered_ring_case()
    got = check_host(csr, cost, dsts, rows, srcs, w, scen)["route"]
    assert got[0][0][edge[(1, 0)]] > 0 and got[0][1][edge[(1, 0)]] == 0.0
    csr, cost, edge, (s, a, b, d), scen = raised_chord_case()
    got = check_host(csr, cost, [d], [0], [s], np.array([12], np.uint64), scen)
    assert got["route"][0][0][edge[(s, d)]] == 4.0 and got["hop"][0][0][edge[(s, a)]] == 4.0
    assert got["route"][0][1][edge[(s, d)]] == 12.0
    # the trap: INF on a link that stays tight
    csr, cost, edge, (s, a, b, d) = trap_case()
    got = check_host(csr, cost, [d], [0, 0], [s, a], np.array([8, 4], np.uint64),
                     [([edge[(s, a)]], [INF])])
    assert got["route"][0][0][edge[(s, a)]] == 0.0 and got["route"][0][0][edge[(s, b)]] == 8.0
    assert got["route"][3][0] == 8.0 and got["route"][4][0] == edge[(s, b)]


def test_all_inf_is_the_failure_restatement_and_argument_errors():
    csr, cost, dsts, rows, srcs, w, lists = small_case("fat_tree_k4", 1)
    scen = [(es, [INF] * len(es)) for es in lists]
    for split in SPLITS:
        want = EN.failure_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, lists, split)
        got = EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, scen, split)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want))
        same = EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w,
                                              [([3, 9], cost[[3, 9]]), ([], [])], split)
        assert np.array_equal(same[0][0], same[0][1])
    V, E = int(csr.V), int(csr.E)
    norm = EN.normalise_cost_scenarios([([5, 2], [7, INF]), ([], [])], csr)
    assert norm[0][0].tolist() == [2, 5] and norm[0][1].tolist() == [INF, 7]
    assert norm[0][0].dtype == np.int32 and norm[0][1].dtype == np.uint32 and norm[1][0].size == 0
    bound = -(-INF // (V - 1))                              # the least cost the rule refuses
    EN.normalise_cost_scenarios([([0], [bound - 1])], csr)
    for bad in (([3, 3], [2, 2]), ([E], [2]), ([-1], [2]), ([0], [0]), ([0], [bound]),
                ([0, 1], [2]), ([0], [1.5])):
        with pytest.raises(ValueError):
            EN.normalise_cost_scenarios([bad], csr)
    for cap in (np.ones(E - 1), np.zeros(E), np.full(E, np.nan), np.full(E, np.inf)):
        with pytest.raises(ValueError):
            EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, [([], [])], "route", cap)
    with pytest.raises(ValueError):
        EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, [([], [])], "flow")
    with pytest.raises(ValueError):
        EN.whatif_ecmp_link_loads_host(csr, cost, dsts, [V], [0], None, [([], [])])
    none = EN.whatif_ecmp_link_loads_host(csr, cost, dsts, rows, srcs, w, [])
    assert none[0].shape == (0, E) and none[3].shape == (0,) and none[4].shape == (0,)
    assert EN.peak_utilisation(np.zeros(4)) == (0.0, -1)
    assert EN.peak_utilisation([1.0, 4.0, 4.0], [1.0, 2.0, 2.0]) == (2.0, 1)


def test_null_context_and_symbol():
    from sdnmpi_amd import _native
    L = _native.library()
    assert "sdnr_whatif_ecmp_link_loads" in _native.EXPORTED_SYMBOLS
    assert L.sdnr_whatif_ecmp_link_loads(None, None, 0, None, None, None, 0, None, None, None,
                                         None, None, None, None, None, None,
                                         _native.DEVICE_PTRS) == -22


# ------------------------------------------------------------------ the drop-in --

def changes_of(failures, seed):
    """The failure scenarios of dropin_case as cost changes: per link None
    (down) or a cost in [1, 4], alternating; the last two forms of a scenario
    (mapping, iterable of pairs) both occur."""
    rng = np.random.default_rng(seed)
    out = []
    for i, sc in enumerate(failures):
        links = list(dict.fromkeys(sc))                    # (a link once per scenario)
        items = [(l, None if (i + j) % 3 == 0 else int(rng.integers(1, 5)))
                 for j, l in enumerate(links)]
        out.append(dict(items) if i % 2 else items)
    return out


def changed_twin(make, fabric, costs, scenario):
    """A second TopologyDB with the same switches, hosts, links and costs on
    which the changes of ``scenario`` were really made."""
    db = make(fabric)
    if costs:
        db.set_link_costs(costs)
    for (a, b), c in (scenario.items() if hasattr(scenario, "items") else scenario):
        if a in db.links and b in db.links[a]:
            if c is None:
                db.delete_link(db.links[a][b])
            else:
                db.set_link_cost(a, b, c)
    return db


def link_peak(loads, capacity):
    """(peak, {link: utilisation}) of a SplitLinkLoads over its switch links."""
    u = {(a, b): x / capacity.get((a, b), 1.0) for a, b, x in
         zip(loads.src_dpid.tolist(), loads.dst_dpid.tolist(), loads.load.tolist())}
    return max(list(u.values()) + [0.0]), u


def check_dropin(make, name, with_costs):
    """cost_change_link_loads of ``make(fabric)`` against twins with the changes
    really made (shared with the GPU file: ``make`` chooses the engine)."""
    fabric, _, costs, failures, pairs, w = dropin_case(name, with_costs)
    db = make(fabric)
    if costs:
        db.set_link_costs(costs)
    changes = changes_of(failures, len(name))
    links = [(u, v) for u in sorted(db.links) for v in sorted(db.links[u])]
    capacity = {l: float(x) for l, x in zip(links[::2], np.random.default_rng(3).uniform(
        0.5, 4.0, len(links[::2])))}
    capacity[(10 ** 9, 1)] = 2.0                           # no such link: ignored
    links_before = db.links
    snap = {u: dict(nb) for u, nb in db.links.items()}
    ex = db.graph()
    version, costs_before = db._cost_version, dict(db._link_costs)
    routes_before = db.find_routes_least_cost(pairs[:20], multiple=True)
    known = [db._endpoint(a) is not None and db._endpoint(b) is not None for a, b in pairs]
    twins = [changed_twin(make, fabric, costs, sc) for sc in changes]
    sets = [twin.find_routes_least_cost(pairs, multiple=True) for twin in twins]
    for split in SPLITS:
        for wt in (w, None):
            ws = wt if wt is not None else [1] * len(pairs)
            theirs = [twin.least_cost_ecmp_link_loads(pairs, wt, split) for twin in twins]
            for cap in (None, capacity):
                got = db.cost_change_link_loads(changes, pairs, wt, split, cap)
                assert isinstance(got, CostChangeLoads) and isinstance(got, FailureLoads)
                assert len(got) == len(changes) and got.lost.dtype == np.uint64
                assert got.load.shape == (len(changes), ex.csr.E) and got.peak.dtype == np.float64
                assert got.scenarios[-2] == () and len(got.scenarios[-1]) == 1   # missing ignored
                assert dicts_close(got.scenario(len(changes) - 2).as_dict(), got.base.as_dict())
                assert close([got.base_peak], [link_peak(got.base, cap or {})[0]])
                assert close([got.peak[len(changes) - 2]], [got.base_peak])
                for k in range(len(changes)):
                    one = got.scenario(k)
                    assert isinstance(one, SplitLinkLoads)
                    assert dicts_close(one.as_dict(), theirs[k].as_dict()), k
                    assert int(got.lost[k]) == sum(x for x, r, ok in zip(ws, sets[k], known)
                                                   if ok and not r)
                    peak, util = link_peak(theirs[k], cap or {})
                    assert close([got.peak[k]], [peak]), k
                    if peak > 0:
                        assert util[got.peak_link[k]] >= peak * (1 - 1e-9)
                    else:
                        assert got.peak_link[k] is None
                top, at = got.worst()
                assert np.array_equal(top, got.load.max(0))
                assert len(got.worst_dict()) == int((top != 0).sum())
    # nothing of the live object changed
    assert db.links is links_before and {u: dict(nb) for u, nb in db.links.items()} == snap
    assert db.graph() is ex and db._link_costs == costs_before and db._cost_version == version
    assert db.find_routes_least_cost(pairs[:20], multiple=True) == routes_before
    return db


@pytest.mark.parametrize("name,with_costs", [("fat_tree_k4", False), ("random_V12", False),
                                             ("torus_2x2x2", True)])
def test_dropin_equals_a_twin_with_the_changes_really_made(name, with_costs):
    db = check_dropin(fake_db, name, with_costs)
    assert not any(c[0] == "failure" for c in db.engine.calls)
    assert any(c[0] == "whatif" for c in db.engine.calls)


def test_all_pairs_and_mpi_forms_and_value_errors():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    links = [(u, v) for u in sorted(db.links) for v in sorted(db.links[u])]
    changes = [{links[0]: 3}, {links[5]: None, links[6]: 2}, {}, [(links[9], None)]]
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs for b in macs if a != b]
    cap = {links[0]: 0.5}
    for split in SPLITS:
        allp = db.all_pairs_cost_change_link_loads(changes, split, cap)
        byp = db.cost_change_link_loads(changes, pairs, None, split, cap)
        assert np.array_equal(allp.lost, byp.lost) and allp.scenarios == byp.scenarios
        assert np.array_equal(allp.peak, byp.peak) and allp.peak_link == byp.peak_link
        assert allp.base_peak == byp.base_peak
        for k in range(len(changes)):
            assert dicts_close(allp.scenario(k).as_dict(), byp.scenario(k).as_dict()), k
        ranks = {r: m for r, m in enumerate(macs[:6])}
        mp = db.mpi_cost_change_link_loads(changes, ranks, None, split, cap)
        rp = db.cost_change_link_loads(changes, [(ranks[i], ranks[j]) for i in ranks for j in ranks
                                                 if i != j], None, split, cap)
        assert np.array_equal(mp.load, rp.load) and np.array_equal(mp.peak, rp.peak)
    assert byp.scenarios[1] == ((links[5], None), (links[6], 2))
    V = len(db.switches)
    for bad in ([[(links[0], 2), (links[0], 3)]], [{links[0]: 0}], [{links[0]: True}],
                [{links[0]: 1.5}], [{links[0]: INF}], [{links[0]: -(-INF // (V - 1))}],
                [{(10 ** 9, 1): 0}], [{1: 2}]):
        with pytest.raises(ValueError):
            db.cost_change_link_loads(bad, pairs[:3])
    for bad in ({links[0]: 0}, {links[0]: float("nan")}, {links[0]: -1.0}, {links[0]: True},
                {links[0]: float("inf")}):
        with pytest.raises(ValueError):
            db.cost_change_link_loads(changes, pairs[:3], capacity=bad)
    with pytest.raises(ValueError):
        db.cost_change_link_loads(changes, pairs[:3], None, "flow")
    none = db.cost_change_link_loads([], pairs[:3])
    assert none.load.shape[0] == 0 and none.peak.shape == (0,) and none.peak_link == []


# -------------------------------------------------------------------- the tuner --

S, A, B, C, D = 1, 2, 3, 4, 5


def fish_fabric():
    """The fish: switches s - a - d and s - b - c - d, a host on s and one on d."""
    links = [(S, A), (A, D), (S, B), (B, C), (C, D)]
    nxt = {}
    src, sport, dst, dport = [], [], [], []
    for u, v in links:
        pu, pv = nxt.get(u, 2), nxt.get(v, 2)
        nxt[u], nxt[v] = pu + 1, pv + 1
        src += [u, v]
        sport += [pu, pv]
        dst += [v, u]
        dport += [pv, pu]
    return T.Fabric("fish", src, sport, dst, dport, [0x020000000001, 0x020000000005], [S, D],
                    [1, 1], [S, A, B, C, D], {})


def check_fish(make):
    """The tuner on the fish with one pair s -> d of weight 4, and of weight 1
    without weights (shared with the GPU file): every load is dyadic, the peaks
    are exact, and at s both splits halve."""
    fabric = fish_fabric()
    ms, md = fabric.host_macs()
    first = None
    for split in SPLITS:
        for wt, x in (([4], 4.0), (None, 1.0)):
            db = make(fabric)
            first = first or db
            got = db.tune_link_costs([(ms, md)], wt, split=split)
            assert isinstance(got, CostTuning)
            assert got.peak_before == x and got.peak_after == x / 2
            assert got.history == [((S, A), 2, x / 2)] and got.costs == {(S, A): 2}
            assert db.link_cost(S, A) == 1 and db._link_costs == {}    # apply=False
            twin = make(fabric)
            twin.set_link_costs(got.costs)
            loads = twin.least_cost_ecmp_link_loads([(ms, md)], wt, split)
            assert link_peak(loads, {})[0] == got.peak_after
            # applied; from there nothing improves
            assert db.tune_link_costs([(ms, md)], wt, split=split, apply=True).costs == \
                {(S, A): 2}
            assert db.link_cost(S, A) == 2
            again = db.tune_link_costs([(ms, md)], wt, split=split)
            assert again.costs == {} and again.history == []
            assert again.peak_before == x / 2 and again.peak_after == x / 2
    # a capacity of 4 on the short way: it is the better route, nothing to do
    fresh = make(fabric)
    cap = {(S, A): 4.0, (A, D): 4.0}
    got = fresh.tune_link_costs([(ms, md)], [4], capacity=cap)
    assert got.peak_before == 1.0 and got.costs == {}
    assert fresh.tune_link_costs([(ms, md)], [4], rounds=0).peak_before == 4.0
    assert fresh.mpi_tune_link_costs({0: ms, 1: md}, {(0, 1): 4}).costs == {(S, A): 2}
    assert fresh.all_pairs_tune_link_costs().peak_before == 1.0
    with pytest.raises(ValueError):
        fresh.tune_link_costs([(ms, md)], [4], top=0)
    with pytest.raises(ValueError):
        fresh.tune_link_costs([(ms, md)], [4], steps=(0,))
    return first


def test_the_tuner_on_the_fish():
    db = check_fish(fake_db)
    # each round: one single-scenario call with loads, one with the peaks only
    first = [c for c in db.engine.calls if c[0] == "whatif"][:4]
    assert [(c[2], c[3], c[4]) for c in first] == [(1, True, False), (7, False, False),
                                                   (1, True, False), (16, False, False)]
