"""Fast-reroute what-if loads, CPU only: engine.frr_link_loads_host (the
checker of frr_loads.hip) against the definition -- one pair at a time, one
hop at a time over the primary and backup next hops --, the conditions that
make the comparison mean something, and the drop-in over an engine double
built from the restatements.  Everything is integer: every comparison is
exact."""
import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import engine as EN
from sdnmpi_amd.util.topology_db import FrrLoads, LinkLoads, TopologyDB
from test_cost_ecmp_loads import both_ways, digraph_csr, random_costs
from test_ecmp_link_loads import edge_map
from test_lfa_tables import FakeLfaEngine, all_pairs
from test_link_loads import golden_pairs

FABRICS = ["mock", "random_V9", "random_V12", "random_V12_loops", "torus_2x2x2", "fat_tree_k4",
           "dragonfly_a4_h2_p2"]
LISTS = ("empty", "links", "cables", "switches")
# where a switch failure shows every status at once (checked below)
ALL_STATUSES = {("dragonfly_a4_h2_p2", 1), ("dragonfly_a4_h2_p2", 4), ("random_V9", 1),
                ("random_V9", 4), ("random_V12", 1), ("random_V12", 4), ("fat_tree_k4", 4),
                ("torus_2x2x2", 4)}


class FakeFrrEngine(FakeLfaEngine):
    """The restatement double plus frr_link_loads."""

    def frr_link_loads(self, export, nh, backup, dsts, rows, srcs, weights=None, scenarios=(),
                       planes=True, timing=False, table_budget=None):
        self.calls.append(("frr", export.key, len(scenarios), bool(planes)))
        E, n = int(export.csr.E), len(rows)
        budget = EN.DEFAULT_TABLE_BUDGET if table_budget is None else int(table_budget)
        step = max(1, budget // max(1, 8 * E + n))
        parts = [EN.frr_link_loads_host(export.csr, nh, backup, dsts, rows, srcs, weights,
                                        scenarios[c:c + step])
                 for c in range(0, len(scenarios), step)]
        self.calls.append(("frr_chunks", len(parts)))
        if not parts:
            parts = [EN.frr_link_loads_host(export.csr, nh, backup, dsts, rows, srcs, weights, [])]
        load, stat, status, peak, pedge = (np.concatenate([p[j] for p in parts])
                                           for j in range(5))
        items = sum(p[5] for p in parts)
        if not planes:
            load = status = None
        return load, stat, status, peak, pedge, items


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeFrrEngine()
    return db


def esrc_of(csr):
    return np.repeat(np.arange(int(csr.V)), np.diff(np.asarray(csr.row_ptr, np.int64)))


def scenario_lists(csr):
    """{name: list of edge-id lists}: no failure, every directed link, every
    cable (the directions that exist), every switch (all its links, both ways)."""
    V, E = int(csr.V), int(csr.E)
    u, v = esrc_of(csr), np.asarray(csr.col, np.int64)
    cables = {}
    for e in range(E):
        cables.setdefault((min(u[e], v[e]), max(u[e], v[e])), []).append(e)
    return {"empty": [[]],
            "links": [[e] for e in range(E)],
            "cables": [cables[k] for k in sorted(cables)],
            "switches": [np.nonzero((u == x) | (v == x))[0].tolist() for x in range(V)]}


def tables(csr, cost, node_protect=True):
    """(nh, backup) [V, V]: row d toward d."""
    V = int(csr.V)
    P = all_pairs(csr, cost)
    nh = EN.cost_tables_host(csr, cost, np.arange(V))[1]
    backup = EN.lfa_tables_host(csr, cost, P, np.arange(V), link_only=not node_protect)[0]
    return nh, backup


def demand(csr, seed):
    """Every ordered switch pair, s == d included, a few sources that are no
    vertex and a row whose destination is none: (dsts, rows, srcs, w), in no
    particular row order."""
    V = int(csr.V)
    rng = np.random.default_rng(seed)
    dsts = np.concatenate([np.arange(V), [V + 3]])
    rows = np.concatenate([np.repeat(np.arange(V), V), [0, V - 1, V, V]])
    srcs = np.concatenate([np.tile(np.arange(V), V), [-1, V, 0, 1]])
    w = rng.integers(0, 1 << 32, rows.shape[0], dtype=np.uint64)
    w[rng.random(rows.shape[0]) < 0.2] = 0
    order = rng.permutation(rows.shape[0])
    return dsts, rows[order], srcs[order], w[order]


def walk_frr(csr, nh, backup, dsts, rows, srcs, w, scen):
    """The definition, one pair and one hop at a time (plain Python): (load,
    stat, status, items)."""
    V, E = int(csr.V), int(csr.E)
    edge = edge_map(csr)
    u, v = esrc_of(csr), np.asarray(csr.col, np.int64)
    load = [[0] * E for _ in scen]
    stat = [[0, 0, 0, 0] for _ in scen]
    status = [[0] * len(rows) for _ in scen]
    items = 0
    has_pairs = set(int(r) for r in rows)
    for k, failed in enumerate(scen):
        down = set(int(e) for e in failed)
        for r in sorted(has_pairs):
            d = int(dsts[r])
            if 0 <= d < V and any(u[e] != d and nh[r][u[e]] == v[e] for e in down):
                items += 1
        for i in range(len(rows)):
            r, s, wi = int(rows[i]), int(srcs[i]), int(w[i])
            d = int(dsts[r])
            code, path = 0, []
            if 0 <= s < V and 0 <= d < V:
                x, hops = s, 0
                while x != d and x >= 0:                   # the base route
                    x = int(nh[r][x])
                    hops += 1
                    assert hops <= V
                if x == d:
                    x, seen, code = s, set(), 1
                    while x != d:
                        if x in seen:
                            code = 4
                            break
                        seen.add(x)
                        p = int(nh[r][x])
                        if p < 0:
                            code = 3
                            break
                        if edge[(x, p)] in down:
                            b = int(backup[r][x])
                            if b < 0 or edge[(x, b)] in down:
                                code = 3
                                break
                            p, code = b, 2
                        path.append(edge[(x, p)])
                        x = p
            status[k][i] = code
            if code in (1, 2):
                for e in path:
                    load[k][e] = (load[k][e] + wi) & (2 ** 64 - 1)
            for j, c in enumerate((2, 3, 4, 0)):
                if code == c:
                    stat[k][j] = (stat[k][j] + wi) & (2 ** 64 - 1)
    return (np.asarray(load, np.uint64).reshape(len(scen), E), np.asarray(stat, np.uint64),
            np.asarray(status, np.uint8).reshape(len(scen), len(rows)), items)


def peaks_of(load):
    peak = load.max(1) if load.shape[1] else np.zeros(load.shape[0], np.uint64)
    edge = np.where(peak > 0, load.argmax(1) if load.shape[1] else 0, -1)
    return peak.astype(np.uint64), edge.astype(np.int32)


_CASES = {}


def case(name, hi, node_protect):
    """The inputs of one (fabric, cost range, protection) and the restatement's
    and the walker's answers per scenario list, computed once."""
    key = (name, hi, node_protect)
    if key not in _CASES:
        csr = G.Golden(name).fabric().csr()
        V = int(csr.V)
        cost = random_costs(csr, 1, hi, 3 * V + hi)
        nh, backup = tables(csr, cost, node_protect)
        dsts, rows, srcs, w = demand(csr, V + hi)
        pad = np.full((1, V), -1, np.int32)                # the row of the bad destination
        nh, backup = np.concatenate([nh, pad]), np.concatenate([backup, pad])
        lists = scenario_lists(csr)
        host = {m: EN.frr_link_loads_host(csr, nh, backup, dsts, rows, srcs, w, lists[m])
                for m in LISTS}
        walk = {m: walk_frr(csr, nh, backup, dsts, rows, srcs, w, lists[m]) for m in LISTS}
        _CASES[key] = (csr, cost, nh, backup, (dsts, rows, srcs, w), lists, host, walk)
    return _CASES[key]


@pytest.mark.parametrize("node_protect", [True, False])
@pytest.mark.parametrize("hi", [1, 4])
@pytest.mark.parametrize("name", FABRICS)
def test_restatement_equals_the_walk_by_definition(name, hi, node_protect):
    csr, _, _, _, _, lists, host, walk = case(name, hi, node_protect)
    for m in LISTS:
        load, stat, status, peak, pedge, items = host[m]
        wl, ws, wst, wi = walk[m]
        assert np.array_equal(load, wl), m
        assert np.array_equal(stat, ws), m
        assert np.array_equal(status, wst), m
        assert items == wi, m
        pk, pe = peaks_of(wl)
        assert np.array_equal(peak, pk) and np.array_equal(pedge, pe), m
        assert load.dtype == np.uint64 and stat.dtype == np.uint64
        assert status.dtype == np.uint8 and peak.dtype == np.uint64 and pedge.dtype == np.int32
        assert load.shape == (len(lists[m]), int(csr.E))


@pytest.mark.parametrize("node_protect", [True, False])
@pytest.mark.parametrize("hi", [1, 4])
@pytest.mark.parametrize("name", FABRICS)
def test_single_failures_never_loop_and_switch_failures_show_every_status(name, hi, node_protect):
    csr, _, nh, backup, (dsts, rows, srcs, w), lists, host, _ = case(name, hi, node_protect)
    # RFC 5286: an alternate is loop-free for the failure it was computed for
    for m in ("links", "cables"):
        load, stat, status, _, _, _ = host[m]
        assert not stat[:, 2].any() and not (status == 4).any(), m
        # a failed link carries nothing
        for k, failed in enumerate(lists[m]):
            assert not load[k][failed].any()
    load, stat, status, _, _, _ = host["switches"]
    for k, failed in enumerate(lists["switches"]):
        assert not load[k][failed].any()
    if (name, hi) in ALL_STATUSES:
        assert set(np.unique(status).tolist()) == {0, 1, 2, 3, 4}
    # the empty scenario is the fabric as it is
    load, stat, status, peak, pedge, items = host["empty"]
    V = int(csr.V)
    ok = (srcs >= 0) & (srcs < V) & (dsts[rows] < V)
    base = EN.link_loads_host(csr, nh.astype(np.int32), EN.INT32, rows[ok], srcs[ok], w[ok],
                              to_root=True)
    assert np.array_equal(load[0], base) and items == 0
    routed = ok.copy()
    P = EN.cost_tables_host(csr, case(name, hi, node_protect)[1], np.arange(V))[0]
    routed[ok] = P[dsts[rows[ok]], srcs[ok]] != EN.COST_INF
    assert np.array_equal(status[0], routed.astype(np.uint8))
    assert stat[0].tolist() == [0, 0, 0, int(w[~routed].sum(dtype=np.uint64))]


@pytest.mark.parametrize("name", ["fat_tree_k4", "random_V12", "dragonfly_a4_h2_p2"])
def test_a_link_drops_what_its_unprotected_primaries_carry(name):
    hi = 4
    csr, cost, nh, backup, (dsts, rows, srcs, w), lists, host, _ = case(name, hi, True)
    V = int(csr.V)
    u, v = esrc_of(csr), np.asarray(csr.col, np.int64)
    stat = host["links"][1]
    want = [0] * int(csr.E)
    for i in range(rows.shape[0]):
        s, d = int(srcs[i]), int(dsts[rows[i]])
        if not (0 <= s < V and 0 <= d < V):
            continue
        x, path = s, []
        while x != d and x >= 0:
            path.append(x)
            x = int(nh[d][x])
        if x != d:
            continue
        for x in path:                                     # (switch x, destination d) unprotected
            if backup[d][x] < 0:
                e = edge_map(csr)[(x, int(nh[d][x]))]
                want[e] = (want[e] + int(w[i])) & (2 ** 64 - 1)
    assert stat[:, 1].tolist() == want
    assert any(want)
    # ... and those are unprotected_links()' pairs
    db = fake_db(G.Golden(name).fabric())
    ex = db.graph()
    db.set_link_costs({(int(csr.dpids[u[e]]), int(csr.dpids[v[e]])): int(cost[e])
                       for e in range(int(csr.E))})
    bare = db.unprotected_links()
    count = {}
    for d in range(V):
        for x in range(V):
            if nh[d][x] >= 0 and backup[d][x] < 0:
                key = (int(csr.dpids[x]), int(csr.dpids[nh[d][x]]))
                count[key] = count.get(key, 0) + 1
    assert bare == count and ex.csr.E == csr.E


def test_backups_are_taken_as_given():
    """Hand-made backups on a ring of 6: a loop of two, a longer cycle, a backup
    into a switch that drops, and a backup whose link is down too."""
    V = 6
    csr = digraph_csr(both_ways([(i, (i + 1) % V) for i in range(V)]))
    edge = edge_map(csr)
    # toward 0 every switch forwards downwards: 5 -> 4 -> 3 -> 2 -> 1 -> 0
    nh = np.asarray([[-1, 0, 1, 2, 3, 4]], np.int32)
    srcs = np.arange(V)
    rows = np.zeros(V, np.int64)
    w = np.asarray([1, 2, 4, 8, 16, 32], np.uint64)

    def run(backup, failed):
        return EN.frr_link_loads_host(csr, nh, np.asarray([backup], np.int32), [0], rows, srcs, w,
                                      [failed])

    # 3 -> 2 fails, 3 sends back to 4, whose primary is 3: a loop of two
    load, stat, status, peak, pedge, items = run([-1, -1, -1, 4, -1, -1], [edge[(3, 2)]])
    assert status[0].tolist() == [1, 1, 1, 4, 4, 4] and items == 1
    assert stat[0].tolist() == [0, 0, 8 + 16 + 32, 0]
    want = np.zeros(int(csr.E), np.uint64)
    want[edge[(1, 0)]], want[edge[(2, 1)]] = 2 + 4, 4
    assert np.array_equal(load[0], want)
    assert int(peak[0]) == 6 and int(pedge[0]) == edge[(1, 0)]
    # 1 -> 0 and 2 -> 1 fail; 1 backs up to 2, 2 to 3, whose primary is 2: the
    # cycle 2 -> 3 -> 2 with 1 behind it, and everything above feeds it
    load, stat, status, _, _, _ = run([-1, 2, 3, -1, -1, -1], [edge[(1, 0)], edge[(2, 1)]])
    assert status[0].tolist() == [1, 4, 4, 4, 4, 4]
    assert not load[0].any()
    # 5's way round: 3 -> 2 fails and 3, 4, 5 have backups up the ring to 0
    load, stat, status, _, _, _ = run([-1, -1, -1, 4, 5, 0], [edge[(3, 2)]])
    # 4's and 5's primaries are up: 3 -> 4 -> 3 loops; only a full detour repairs
    assert status[0].tolist() == [1, 1, 1, 4, 4, 4]
    load, stat, status, _, _, _ = run([-1, -1, -1, 4, 5, 0],
                                      [edge[(3, 2)], edge[(4, 3)], edge[(5, 4)]])
    assert status[0].tolist() == [1, 1, 1, 2, 2, 2]
    assert stat[0].tolist() == [8 + 16 + 32, 0, 0, 0]
    want = np.zeros(int(csr.E), np.uint64)
    want[edge[(1, 0)]], want[edge[(2, 1)]] = 2 + 4, 4
    want[edge[(3, 4)]], want[edge[(4, 5)]], want[edge[(5, 0)]] = 8, 8 + 16, 8 + 16 + 32
    assert np.array_equal(load[0], want)
    # a backup into a drop: 4 -> 3 fails, 4 has none; 5 is untouched and feeds 4
    load, stat, status, _, _, _ = run([-1, -1, -1, -1, -1, 0], [edge[(4, 3)]])
    assert status[0].tolist() == [1, 1, 1, 1, 3, 3] and stat[0].tolist() == [0, 16 + 32, 0, 0]
    # the backup's own link is down as well
    load, stat, status, _, _, _ = run([-1, -1, -1, -1, -1, 0], [edge[(5, 0)], edge[(5, 4)]])
    assert status[0].tolist() == [1, 1, 1, 1, 1, 3]
    # a backup that is the primary itself goes down with it
    load, stat, status, _, _, _ = run([-1, -1, -1, 2, -1, -1], [edge[(3, 2)]])
    assert status[0].tolist() == [1, 1, 1, 3, 3, 3] and stat[0].tolist() == [0, 8 + 16 + 32, 0, 0]
    with pytest.raises(ValueError):
        run([-1, -1, -1, 0, -1, -1], [edge[(3, 2)]])      # 3 -> 0 is no link


def test_no_scenarios_no_pairs_and_errors():
    csr = G.Golden("fat_tree_k4").fabric().csr()
    V, E = int(csr.V), int(csr.E)
    nh, backup = tables(csr, np.ones(E, np.uint32))
    out = EN.frr_link_loads_host(csr, nh, backup, np.arange(V), [0, 1], [3, 4], None, [])
    assert out[0].shape == (0, E) and out[1].shape == (0, 4) and out[2].shape == (0, 2)
    assert out[5] == 0
    out = EN.frr_link_loads_host(csr, nh, backup, np.arange(V), [], [], None, [[0], [1, 2]])
    assert out[0].shape == (2, E) and not out[0].any() and out[2].shape == (2, 0)
    assert out[3].tolist() == [0, 0] and out[4].tolist() == [-1, -1] and out[5] == 0
    with pytest.raises(ValueError):
        EN.frr_link_loads_host(csr, nh, backup, np.arange(V), [V], [0], None, [[0]])
    with pytest.raises(ValueError):
        EN.frr_link_loads_host(csr, nh, backup, np.arange(V), [0], [1], None, [[E]])
    # duplicates and the order inside a scenario do not matter
    a = EN.frr_link_loads_host(csr, nh, backup, np.arange(V), [0, 0], [5, 9], [3, 4], [[7, 2, 7]])
    b = EN.frr_link_loads_host(csr, nh, backup, np.arange(V), [0, 0], [5, 9], [3, 4], [[2, 7]])
    assert all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5])) and a[5] == b[5]


# ------------------------------------------------------------------ the drop-in --

def walk_entries(db, pairs, weights, scenario, node_protect=True):
    """{(dpid, out_port): weight} of the delivered pairs' walks over
    least_cost_tables() and lfa_tables(), and the weights (repaired, dropped,
    looped, unrouted)."""
    ex = db.graph()
    csr = ex.csr
    V = int(csr.V)
    lt = db.least_cost_tables(vertices=range(V))
    bt = db.lfa_tables(vertices=range(V), node_protect=node_protect)
    nh, nhp, bk, bkp = lt["nh"], lt["nh_port"], bt["backup"], bt["backup_port"]
    down = set(scenario)
    dp = csr.dpids
    out, stat = {}, [0, 0, 0, 0]
    for (a, b), wi in zip(pairs, weights):
        ea, eb = db._endpoint(a), db._endpoint(b)
        if ea is None or eb is None:
            continue
        s, d = ex.index[ea[0]], ex.index[eb[0]]
        if s != d and lt["pcost"][d, s] == EN.COST_INF:
            stat[3] += wi
            continue
        x, seen, fdb, code = s, set(), [], 1
        while x != d:
            if x in seen:
                code = 4
                break
            seen.add(x)
            n, port = int(nh[d, x]), int(nhp[d, x])
            if (int(dp[x]), int(dp[n])) in down:
                n, port = int(bk[d, x]), int(bkp[d, x])
                if n < 0 or (int(dp[x]), int(dp[n])) in down:
                    code = 3
                    break
                code = 2
            fdb.append((int(dp[x]), port))
            x = n
        if code in (1, 2):
            fdb.append(db._last_hop(eb[0], eb[1], b))
            for key in fdb:
                out[key] = out.get(key, 0) + wi
        if code > 1:
            stat[code - 2] += wi
    return out, stat


def dropin_case(name):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    rng = np.random.default_rng(int(db.graph().csr.V))
    links = [(a, b) for a in db.links for b in db.links[a]]
    db.set_link_costs({links[i]: int(rng.integers(1, 5)) for i in
                       rng.choice(len(links), len(links) // 2, replace=False)})
    pairs = golden_pairs(g, fabric)[:60] + [("00:00:00:00:00:00:00:fe", fabric.host_macs()[0])]
    weights = rng.integers(0, 1 << 20, len(pairs)).tolist()
    some = sorted(db.links)
    failures = [(), db.cable(*links[0]), db.switch_links(some[len(some) // 2]),
                db.switch_links(some[0]) + db.switch_links(some[-1])] + db.cable_failures()[:6]
    return db, pairs, weights, failures


@pytest.mark.parametrize("node_protect", [True, False])
@pytest.mark.parametrize("name", ["fat_tree_k4", "random_V12", "dragonfly_a4_h2_p2"])
def test_dropin_equals_the_walks_over_its_own_tables(name, node_protect):
    db, pairs, weights, failures = dropin_case(name)
    before = (db.to_dict(), dict(db._link_costs), db.graph().key)
    got = db.frr_link_loads(failures, pairs, weights, node_protect=node_protect)
    assert isinstance(got, FrrLoads) and len(got) == len(failures)
    repairs = 0
    for k in range(len(failures)):
        want, stat = walk_entries(db, pairs, weights, got.scenarios[k], node_protect)
        sc = got.scenario(k)
        assert isinstance(sc, LinkLoads) and sc.as_dict() == want, k
        assert [int(got.repaired[k]), int(got.dropped[k]), int(got.looped[k]),
                int(got.unrouted[k])] == stat
        top = int(got.load[k].max())
        assert int(got.peak[k]) == top
        if top:
            e = int(got.load[k].argmax())
            assert got.peak_link[k] == (int(sc.src_dpid[e]), int(sc.dst_dpid[e]))
        else:
            assert got.peak_link[k] is None
        repairs += stat[0]
    assert repairs > 0
    assert got.scenario(0).as_dict() == got.base.as_dict()
    assert got.base.as_dict() == db.least_cost_link_loads(pairs, weights).as_dict()
    with pytest.raises(IndexError):
        got.scenario(len(failures))
    # the numbers alone
    bare = db.frr_link_loads(failures, pairs, weights, node_protect=node_protect, planes=False)
    assert bare.load is None
    for name_ in ("repaired", "dropped", "looped", "unrouted", "peak"):
        assert np.array_equal(getattr(bare, name_), getattr(got, name_))
    assert bare.peak_link == got.peak_link and bare.items == got.items
    with pytest.raises(ValueError):
        bare.scenario(0)
    # nothing of the object changed
    assert (db.to_dict(), dict(db._link_costs), db.graph().key) == before


def test_dropin_all_pairs_mpi_forms_and_chunks():
    g = G.Golden("fat_tree_k4")
    fabric = g.fabric()
    db = fake_db(fabric)
    macs = fabric.host_macs()
    failures = [()] + db.cable_failures()[:12] + [db.switch_links(sorted(db.links)[3])]
    pairs = [(a, b) for a in macs for b in macs if a != b]
    want = db.frr_link_loads(failures, pairs)
    got = db.all_pairs_frr_link_loads(failures)
    for k in range(len(failures)):
        assert got.scenario(k).as_dict() == want.scenario(k).as_dict()
    for name in ("repaired", "dropped", "looped", "unrouted", "peak"):
        assert np.array_equal(getattr(got, name), getattr(want, name))
    assert got.base.as_dict() == want.base.as_dict()
    ranks = {i: m for i, m in enumerate(macs[:6])}
    traffic = {(0, 1): 5, (2, 3): 7, (4, 0): 1, (9, 0): 3}
    a = db.mpi_frr_link_loads(failures, ranks, traffic)
    b = db.frr_link_loads(failures, [(ranks[0], ranks[1]), (ranks[2], ranks[3]),
                                     (ranks[4], ranks[0])], [5, 7, 1])
    assert all(a.scenario(k).as_dict() == b.scenario(k).as_dict() for k in range(len(failures)))
    # a budget of a few scenarios per call: the chunks are invisible
    E = int(db.graph().csr.E)
    n = len(set((db._endpoint(a_)[0], db._endpoint(b_)[0]) for a_, b_ in pairs))
    small = fake_db(fabric, table_budget=max(2 * (8 * E + n), 12 * 20 * 20))
    step = small._budget // (8 * E + n)
    assert 1 <= step < len(failures)
    part = small.frr_link_loads(failures, pairs)
    chunks = [c for c in small._engine.calls if c[0] == "frr_chunks"]
    assert chunks and chunks[0][1] == -(-len(failures) // step) > 1
    for k in range(len(failures)):
        assert part.scenario(k).as_dict() == want.scenario(k).as_dict()
    assert part.items == want.items
