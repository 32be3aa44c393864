"""Least-loaded routes (min-max link utilisation inside the least-cost set),
CPU only: engine.widest_tables_host (the checker of widest_tables.hip) against
the definition by enumeration -- every least-cost route from
engine.least_cost_paths_lex, its busiest link, the minimum over the routes --,
the drop-in over an engine double built from the restatements, and admit_flows
against a plain-Python sequential restatement.  Everything is integer: every
comparison is exact."""
import collections

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import Admission, TopologyDB
from test_cost_ecmp_loads import both_ways, digraph_csr
from test_cost_tables import follow, seeded_costs
from test_ecmp_link_loads import edge_map
from test_link_loads import counter_of, golden_pairs
from test_whatif_loads import FakeWhatifEngine

INF = EN.COST_INF
UTIL_MAX = EN.UTIL_MAX
UTIL_HI = (3, UTIL_MAX)                     # many ties / the whole range
COST_KINDS = ("unit", "seeded")


class FakeWidestEngine(FakeWhatifEngine):
    """The restatement double plus widest_tables."""

    def widest_tables(self, export, cost, pcost, util, dsts, timing=False):
        self.calls.append(("widest", export.key, len(dsts)))
        return EN.widest_tables_host(export.csr, cost, pcost, util, dsts)


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeWidestEngine()
    return db


def seeded_util(csr, hi, seed):
    """A utilisation per directed link in [0, hi]: the two directions differ."""
    return np.random.default_rng(seed).integers(0, hi, int(csr.E), dtype=np.uint64,
                                                endpoint=True).astype(np.uint32)


def small_case(name, kind, hi):
    """(csr, cost, util) of one G.SMALL fabric: the seeds the GPU file shares."""
    k = G.SMALL.index(name)
    csr = G.Golden(name).fabric().csr()
    cost = np.ones(int(csr.E), np.uint32) if kind == "unit" else seeded_costs(csr, 1, 4, 100 + k)
    return csr, cost, seeded_util(csr, hi, 200 + k)


def random_graph(V=12, seed=3):
    """A seeded random connected-ish graph, links both ways."""
    rng = np.random.default_rng(seed)
    und = {(int(a), int(a) + 1) for a in range(V - 2)}          # a chain; vertex V - 1 apart
    while len(und) < 2 * V:
        a, b = sorted(int(x) for x in rng.integers(0, V - 1, 2))
        if a != b:
            und.add((a, b))
    return digraph_csr(both_ways(sorted(und)), V)


# ------------------------------------------------- the definition, enumerated --

def check_against_enumeration(csr, cost, util, dsts):
    V = int(csr.V)
    rp, col = csr.row_ptr, csr.col
    edge = edge_map(csr)
    pcost = EN.cost_tables_host(csr, cost, dsts)[0]
    bott, nh, nhp = EN.widest_tables_host(csr, cost, pcost, util, dsts)
    assert bott.dtype == np.uint32 and nh.dtype == np.int32 and nhp.dtype == np.int32
    u = [int(x) for x in util]
    for i, d in enumerate(int(x) for x in dsts):
        assert bott[i, d] == 0 and nh[i, d] == -1 and nhp[i, d] == -1
        for x in range(V):
            if x == d:
                continue
            routes = EN.least_cost_paths_lex(rp, col, cost, pcost[i], x, d)
            if not routes:
                assert pcost[i, x] == INF
                assert bott[i, x] == 0xFFFFFFFF and nh[i, x] == -1 and nhp[i, x] == -1
                continue
            busiest = [max(u[edge[(a, b)]] for a, b in zip(q, q[1:])) for q in routes]
            assert int(bott[i, x]) == min(busiest)
            # the nh route is least-cost and attains the bottleneck
            seq = follow(nh[i], x, d, V)
            assert seq in routes
            assert busiest[routes.index(seq)] == int(bott[i, x])
            # the step obeys the tie key over the tight links (the routes' first links)
            keys = {}
            for q in routes:
                e = edge[(x, q[1])]
                keys[q[1]] = (max(u[e], int(bott[i, q[1]])), u[e], q[1])
            n = int(nh[i, x])
            assert keys[n] == min(keys.values())
            assert int(nhp[i, x]) == int(csr.port[edge[(x, n)]])


@pytest.mark.parametrize("hi", UTIL_HI)
@pytest.mark.parametrize("kind", COST_KINDS)
@pytest.mark.parametrize("name", G.SMALL)
def test_restatement_equals_the_enumerated_definition(name, kind, hi):
    """Every destination of the fabrics up to 24 switches, five seeded ones of
    the larger (every source either way)."""
    csr, cost, util = small_case(name, kind, hi)
    V = int(csr.V)
    dsts = np.arange(V) if V <= 24 else \
        np.random.default_rng(V + hi).choice(V, 5, replace=False)
    check_against_enumeration(csr, cost, util, dsts)


@pytest.mark.parametrize("hi", UTIL_HI)
@pytest.mark.parametrize("kind", COST_KINDS)
def test_restatement_on_a_random_graph(kind, hi):
    csr = random_graph()
    assert csr.V == 12
    cost = np.ones(int(csr.E), np.uint32) if kind == "unit" else seeded_costs(csr, 1, 4, 31)
    check_against_enumeration(csr, cost, seeded_util(csr, hi, 32), np.arange(12))


def test_equal_utilisation_is_the_least_cost_table():
    for name in ("fat_tree_k4", "torus_2x2x2", "random_V12"):
        csr, cost, _ = small_case(name, "seeded", 3)
        dsts = np.arange(int(csr.V))
        pcost, nh0, nhp0 = EN.cost_tables_host(csr, cost, dsts)
        for x in (0, 7, UTIL_MAX):
            bott, nh, nhp = EN.widest_tables_host(csr, cost, pcost,
                                                  np.full(int(csr.E), x, np.uint32), dsts)
            assert np.array_equal(nh, nh0) and np.array_equal(nhp, nhp0)
            away = (pcost != INF) & (pcost != 0)
            assert (bott[away] == x).all() and (bott[pcost == 0] == 0).all()
            assert (bott[pcost == INF] == 0xFFFFFFFF).all()
        # unit costs need no cost vector; int32 rows holding u32 are taken
        ones = np.ones(int(csr.E), np.uint32)
        p1 = EN.cost_tables_host(csr, ones, dsts)[0]
        util = seeded_util(csr, 3, 1)
        a = EN.widest_tables_host(csr, None, p1.view(np.int32), util, dsts)
        b = EN.widest_tables_host(csr, ones, p1, util, dsts)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_check_link_utilisation():
    csr = G.Golden("mock").fabric().csr()
    E = int(csr.E)
    ok = EN.check_link_utilisation(csr, [UTIL_MAX] * E)
    assert ok.dtype == np.uint32 and ok.shape == (E,) and (ok == UTIL_MAX).all()
    for bad in ([0] * (E - 1), [0.5] * E, [-1] + [0] * (E - 1), [UTIL_MAX + 1] + [0] * (E - 1)):
        with pytest.raises(ValueError):
            EN.check_link_utilisation(csr, bad)
    pcost = EN.cost_tables_host(csr, np.ones(E, np.uint32), [0])[0]
    with pytest.raises(ValueError):
        EN.widest_tables_host(csr, None, pcost, np.full(E, 0xFFFFFFFF, np.uint64), [0])


# ------------------------------------------------------------- the drop-in --

def seed_utilisation(db, hi, seed):
    """Seeded utilisation on every link of the database, keyed by dpid pair."""
    rng = np.random.default_rng(seed)
    links = [(a, b) for a in sorted(db.links) for b in sorted(db.links[a])]
    util = {k: int(x) for k, x in zip(links, rng.integers(0, hi, len(links), endpoint=True))}
    db.set_link_utilisations(util)
    return util


def test_utilisation_state_and_validation():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    a = sorted(db.links)[0]
    b = sorted(db.links[a])[0]
    assert db.link_utilisation(a, b) == 0
    db.set_link_utilisation(a, b, 5)
    db.set_link_utilisations({(b, a): UTIL_MAX, (a, b): np.int64(6)})
    assert db.link_utilisation(a, b) == 6 and db.link_utilisation(b, a) == UTIL_MAX
    for bad in (-1, UTIL_MAX + 1, 1.5, True, "3", None):
        with pytest.raises(ValueError):
            db.set_link_utilisation(a, b, bad)
    with pytest.raises(ValueError):
        db.set_link_utilisations({(a, b): 1, (b, a): -1})       # one refused: nothing set
    with pytest.raises(ValueError):
        db.set_link_utilisations({(a, b): 1, a: 2})
    assert db.link_utilisation(a, b) == 6 and db.link_utilisation(b, a) == UTIL_MAX
    # kept across a link flap, as the costs are
    link = db.links[a][b]
    db.delete_link(link)
    assert db.link_utilisation(a, b) == 6
    db.add_link(link)
    ex = db.graph()
    assert int(db._util_vector(ex)[db._link_edge(ex, a, b)]) == 6
    db.clear_link_utilisations()
    assert db.link_utilisation(a, b) == 0 and not db._util_vector(db.graph()).any()


def test_port_keyed_utilisation():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    a = sorted(db.links)[0]
    nbrs = sorted(db.links[a])
    ports = {(a, db.links[a][b].src.port_no): 10 + i for i, b in enumerate(nbrs)}
    host = next(iter(db.hosts.values()))
    ports[(host.port.dpid, host.port.port_no)] = 99             # a host port: ignored
    ports[(0xDEAD, 1)] = 98                                      # an unknown switch: ignored
    db.set_port_utilisations(ports)
    for i, b in enumerate(nbrs):
        assert db.link_utilisation(a, b) == 10 + i
    assert sum(1 for x in db._link_utils.values() if x) == len(nbrs)
    with pytest.raises(ValueError):
        db.set_port_utilisations({(a, db.links[a][nbrs[0]].src.port_no): 1, (a, 0): UTIL_MAX + 1})
    assert db.link_utilisation(a, nbrs[0]) == 10


@pytest.mark.parametrize("name", G.MULTI)
def test_zero_utilisation_is_the_least_cost_route(name):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    pairs = golden_pairs(g, fabric)
    want = db.find_routes_least_cost(pairs)
    assert db.find_routes_least_loaded(pairs) == want
    assert db.find_route_least_loaded(*pairs[0]) == want[0]
    assert db.least_loaded_link_loads(pairs).as_dict() == \
        db.least_cost_link_loads(pairs).as_dict()
    t, c = db.least_loaded_tables(), db.least_cost_tables()
    assert np.array_equal(t["destinations"], c["destinations"])
    assert np.array_equal(t["nh"], c["nh"]) and np.array_equal(t["nh_port"], c["nh_port"])
    assert np.array_equal(t["bott"] == 0xFFFFFFFF, c["pcost"] == INF)
    assert not t["bott"][c["pcost"] != INF].any()
    assert db.find_route_least_loaded("00:00:00:00:ff:ff", pairs[0][1]) == []


def dropin_results(db, fabric, g):
    """What the GPU file compares between the real engine and the double:
    routes, loads and admissions of the golden pairs under seeded utilisation
    (and seeded costs on a few links)."""
    pairs = golden_pairs(g, fabric)
    seed_utilisation(db, 3, 17)
    links = [(a, b) for a in sorted(db.links) for b in sorted(db.links[a])]
    db.set_link_costs({k: 2 for k in links[::5]})
    w = np.random.default_rng(9).integers(0, 1 << 32, len(pairs)).tolist()
    out = {"pairs": pairs, "w": w}
    out["routes"] = db.find_routes_least_loaded(pairs)
    out["loads"] = db.least_loaded_link_loads(pairs, w).as_dict()
    for name, kw in (("default", {}), ("batch5", {"batch": 5}),
                     ("cap", {"batch": 7, "capacity": 1 << 30})):
        ad = db.admit_flows(pairs, w, routes=True, **kw)
        out[name] = (ad.loads.as_dict(), ad.peak_before, ad.peak_link_before, ad.peak_after,
                     ad.peak_link_after, ad.lost, ad.rounds, ad.routes)
    return out


@pytest.mark.parametrize("name", ["fat_tree_k4", "torus_2x2x2", "random_V12", "mock"])
def test_seeded_utilisation_routes_and_loads(name):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    res = dropin_results(db, fabric, g)
    pairs, w = res["pairs"], res["w"]
    multi = db.find_routes_least_cost(pairs, multiple=True)
    for r, m in zip(res["routes"], multi):
        assert (r in m) if m else r == []
    if name in ("fat_tree_k4", "torus_2x2x2"):              # fabrics with equal-cost choices
        assert res["routes"] != db.find_routes_least_cost(pairs)
    assert res["loads"] == counter_of(res["routes"], w)
    # memoised on (graph, costs, utilisation): a second query computes nothing
    n = len(db._engine.calls)
    assert db.find_routes_least_loaded(pairs) == res["routes"]
    assert len(db._engine.calls) == n
    db.set_link_utilisation(*next(iter(db._link_utils)), value=UTIL_MAX)
    db.find_routes_least_loaded(pairs[:1])
    assert db._engine.calls[-1][0] == "widest"
    # a tiny table budget chunks the rows and changes nothing
    small = fake_db(fabric, table_budget=1)
    assert small._widest_cap(small.graph()) == 1
    assert dropin_results(small, fabric, g)["routes"] == res["routes"]
    assert dropin_results(small, fabric, g)["default"] == res["default"]


# --------------------------------------------------------------- admission --

def admit_restated(db, pairs, weights, capacity=None, batch=None):
    """admit_flows in plain Python: the pairs one slice after the other, each
    pair walked along engine.widest_tables_host's next hops of its slice,
    dict sums of Python ints.  -> (loads {(dpid, port): load} with last hops,
    link loads {(src_dpid, dst_dpid): load}, lost, rounds, routes)."""
    ex = db.graph()
    csr = ex.csr
    E = int(csr.E)
    edge = edge_map(csr)
    link = db._edge_links(ex)
    cost = db._cost_vector(ex)
    base = [int(x) for x in db._util_vector(ex)]
    cap = [1] * E
    if isinstance(capacity, dict):
        for (a, b), x in capacity.items():
            e = db._link_edge(ex, a, b)
            if e is not None:
                cap[e] = x
    elif capacity is not None:
        cap = [capacity] * E
    known = [i for i, (a, b) in enumerate(pairs)
             if db._endpoint(a) is not None and db._endpoint(b) is not None]
    dsw = {i: ex.index[db._endpoint(pairs[i][1])[0]] for i in known}
    if batch is None:
        order = []
        for i in known:
            if dsw[i] not in order:
                order.append(dsw[i])
        slices = [[i for i in known if dsw[i] == d] for d in order]
    else:
        slices = [[i for i in known if c0 <= i < c0 + batch]
                  for c0 in range(0, len(pairs), batch)]
    admitted = [0] * E
    loads = collections.Counter()
    lost = 0
    routes = [[] for _ in pairs]
    for sl in slices:
        util = []
        for e in range(E):
            a = admitted[e] if capacity is None else admitted[e] * 1024 // cap[e]
            util.append(min(base[e] + min(a, UTIL_MAX), UTIL_MAX))
        dsts = sorted(set(dsw[i] for i in sl))
        pcost = EN.cost_tables_host(csr, cost, dsts)[0]
        bott, nh, nhp = EN.widest_tables_host(csr, cost, pcost, np.asarray(util, np.uint64), dsts)
        add = [0] * E
        for i in sl:
            a, b = pairs[i]
            s, d = ex.index[db._endpoint(a)[0]], dsw[i]
            r = dsts.index(d)
            if pcost[r, s] == INF:
                lost += weights[i]
                continue
            seq = follow(nh[r], s, d, int(csr.V))
            for x, y in zip(seq, seq[1:]):
                add[edge[(x, y)]] += weights[i]
                loads[(int(csr.dpids[x]), int(csr.port[edge[(x, y)]]))] += weights[i]
                routes[i].append((int(csr.dpids[x]), int(csr.port[edge[(x, y)]])))
            eb = db._endpoint(b)
            last = db._last_hop(eb[0], eb[1], b)
            loads[last] += weights[i]
            routes[i].append(last)
        admitted = [(x + y) & ((1 << 64) - 1) for x, y in zip(admitted, add)]
    per_link = {link(e): admitted[e] for e in range(E)}
    peak = [x if capacity is None else x * 1024 // c for x, c in zip(admitted, cap)]
    top = max(peak) if peak else 0
    return ({k: v & ((1 << 64) - 1) for k, v in loads.items() if v & ((1 << 64) - 1)}, per_link,
            lost, len(slices), routes, top, link(peak.index(top)) if peak else None)


def link_loads_of(ll):
    return {(int(a), int(b)): int(x) for a, b, x in
            zip(ll.src_dpid.tolist(), ll.dst_dpid.tolist(), ll.load.tolist())}


@pytest.mark.parametrize("name", ["fat_tree_k4", "torus_2x2x2", "random_V12", "mock"])
@pytest.mark.parametrize("kw", [{}, {"batch": 1}, {"batch": 5}, {"batch": 10 ** 6},
                                {"batch": 3, "capacity": 1000},
                                {"batch": 4, "capacity": "some"}])
def test_admit_flows_equals_the_sequential_restatement(name, kw):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    pairs = golden_pairs(g, fabric) + [("00:00:00:00:ff:ff", fabric.host_macs()[0])]
    seed_utilisation(db, 40, 5)
    links = [(a, b) for a in sorted(db.links) for b in sorted(db.links[a])]
    db.set_link_costs({k: 3 for k in links[::4]})
    kw = dict(kw)
    if kw.get("capacity") == "some":
        kw["capacity"] = {k: 7 + i for i, k in enumerate(links[::3])}
    w = np.random.default_rng(2).integers(1, 50, len(pairs)).tolist()
    state = (dict(db._link_utils), dict(db._link_costs), db._util_version, db._cost_version)
    ad = db.admit_flows(pairs, w, routes=True, **kw)
    assert isinstance(ad, Admission)
    loads, per_link, lost, rounds, routes, top, top_link = admit_restated(db, pairs, w, **kw)
    assert ad.loads.as_dict() == loads
    assert link_loads_of(ad.loads) == per_link
    assert (ad.lost, ad.rounds, ad.routes) == (lost, rounds, routes)
    assert (ad.peak_after, ad.peak_link_after) == (top, top_link)
    before = db.least_cost_link_loads(pairs, w)
    cap = db._int_capacity_vector(db.graph(), kw.get("capacity"))
    assert (ad.peak_before, ad.peak_link_before) == db._peak(db.graph(), before.load, cap)
    # every route stays least-cost: the same total carried
    cost = db._cost_vector(db.graph())
    assert int((ad.loads.load * cost).sum()) == int((before.load * cost).sum())
    assert db.admit_flows(pairs, w, **kw).routes is None
    assert state == (dict(db._link_utils), dict(db._link_costs), db._util_version,
                     db._cost_version)
    # a slice computes the rows of its own destinations only
    ex = db.graph()
    db._engine.calls[:] = []
    db.admit_flows(pairs, w, **kw)
    widest = [c[2] for c in db._engine.calls if c[0] == "widest"]
    known = [i for i, (a, b) in enumerate(pairs) if db._endpoint(a) and db._endpoint(b)]
    dsw = [ex.index[db._endpoint(pairs[i][1])[0]] for i in known]
    if "batch" not in kw:
        assert widest == [1] * len(set(dsw))
    else:
        b = kw["batch"]
        per = [len(set(d for i, d in zip(known, dsw) if c0 <= i < c0 + b))
               for c0 in range(0, len(pairs), b)]
        assert widest == [n for n in per if n]


def test_admit_flows_validation():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    pairs = [(macs[0], macs[-1])]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            db.admit_flows(pairs, batch=bad)
    a = sorted(db.links)[0]
    b = sorted(db.links[a])[0]
    for bad in (0, -3, 2.0, (1 << 53) + 1, {(a, b): 0}, {a: 1}):
        with pytest.raises(ValueError):
            db.admit_flows(pairs, capacity=bad)
    ad = db.admit_flows([])
    assert ad.rounds == 0 and ad.lost == 0 and ad.loads.as_dict() == {} and ad.peak_after == 0
    assert db.mpi_admit_flows({0: macs[0], 1: macs[-1]}).loads.as_dict() == \
        db.admit_flows([(macs[0], macs[-1]), (macs[-1], macs[0])]).loads.as_dict()
    assert db.mpi_least_loaded_link_loads({0: macs[0], 1: macs[-1]}).as_dict() == \
        db.least_loaded_link_loads([(macs[0], macs[-1]), (macs[-1], macs[0])]).as_dict()


def fat_tree_all_pairs(fabric, db):
    """Every ordered pair of distinct hosts, destination switch major, one
    switch pair's host pairs side by side; the pairs inside a switch last."""
    by_sw = collections.OrderedDict()
    for m in fabric.host_macs():
        by_sw.setdefault(db.hosts[m].port.dpid, []).append(m)
    cross = [(a, b) for d in by_sw for s in by_sw if s != d for a in by_sw[s] for b in by_sw[d]]
    local = [(a, b) for s in by_sw for a in by_sw[s] for b in by_sw[s] if a != b]
    return cross + local, len(by_sw)


def test_fat_tree_k4_all_host_pairs_peaks():
    """16 hosts on 8 edge switches, every ordered host pair at weight 1: a
    switch pair is 4 host pairs.  The lexicographic routes pile every edge
    switch's traffic onto its first uplink (peak 48); admitted one switch pair
    per round the peak is a third of that; one round holding everything routes
    on zero utilisation and is the lexicographic choice again."""
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    pairs, nsw = fat_tree_all_pairs(fabric, db)
    assert len(pairs) == 16 * 15 and nsw == 8
    w = [1] * len(pairs)
    # the pinned peaks, first from the restatement
    _, per_link, lost, rounds, _, top, _ = admit_restated(db, pairs, w, batch=4)
    assert (top, lost, rounds) == (16, 0, 60)
    _, one, _, _, _, top_all, _ = admit_restated(db, pairs, w, batch=len(pairs))
    assert top_all == 48
    ad = db.admit_flows(pairs, w, batch=4)
    assert (ad.peak_before, ad.peak_after) == (48, 16) and ad.peak_after < ad.peak_before
    assert link_loads_of(ad.loads) == per_link
    whole = db.admit_flows(pairs, w, batch=len(pairs))
    assert whole.peak_after == whole.peak_before == 48 and whole.rounds == 1
    assert link_loads_of(whole.loads) == one
    assert whole.loads.as_dict() == db.least_cost_link_loads(pairs, w).as_dict()
    # the default slicing: one round per destination switch
    by_dst = db.admit_flows(pairs, w)
    assert by_dst.rounds == 8
    assert by_dst.peak_after == admit_restated(db, pairs, w)[5] < 48
    # the same total carried in every case
    total = int(whole.loads.load.sum())
    assert int(ad.loads.load.sum()) == total == int(by_dst.loads.load.sum())
    assert sum(per_link.values()) == total
