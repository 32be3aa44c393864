"""TopologyDB on 16-bit vertex ids above 32,767 and just past them
(boundary_graphs.py): ring(65535) keeps port16 tree words with int16 depth /
distance / next-hop planes, whose stored values are negative for ids and ports
from 32,768 up; the small-port ring(65536) is the first size in slot words with
int32 planes.  Hosts sit on the probe switches; every answer is compared with
the oracle on the same fabric.  The ring's DFS trees are ~24,100 deep, so a
stored depth never reaches 32,768 there: chain(65535) adds that."""
import numpy as np
import pytest

import boundary_graphs as B
from oracle import oracle as O
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import TopologyDB
from test_cost_tables import follow
from test_ecmp_link_loads import dicts_close, route_set_loads
from test_id_width_gpu import exact_counts
from test_link_loads import counter_of

pytestmark = pytest.mark.gpu


class Case(object):
    """One populated drop-in with the oracle's tables of its fabric."""

    def __init__(self, fabric):
        self.fabric = fabric
        self.csr = csr = fabric.csr()
        self.V = csr.V
        # a pool of 64 rows (the default budget would allocate 49,152 of them, 24 GB)
        self.db = fabric.populate(TopologyDB(table_budget=64 * 8 * csr.V))
        self.macs = fabric.host_macs()
        self.hv, self.hp = fabric.host_table()
        self.pairs = [(a, b) for a in range(len(self.macs)) for b in range(len(self.macs))]
        self.mac_pairs = [(self.macs[a], self.macs[b]) for a, b in self.pairs]
        self.tables()

    def tables(self):
        """The oracle's default-route and shortest tables of the drop-in's
        present links (the CSR rebuilt from its dicts)."""
        links = [(u, v, lk.src.port_no) for u, nb in self.db.links.items() for v, lk in nb.items()]
        s, d, p = (np.array(x, np.int64) for x in zip(*links))
        self.csr = T.build_csr(s, d, p, extra_vertices=list(self.db.switches))
        assert self.csr.V == self.V
        self.po, self.to, self.ho = O.dfs_tables(self.csr, self.hv)
        self.dist, self.nh, self.nhp = O.dest_tables(self.csr, self.hv)

    def fdb(self, a, b):
        return O.tree_fdb(self.csr, self.po[a], self.to[a], int(self.hv[a]), int(self.hv[b]),
                          int(self.hp[b]))

    def routes(self):
        return [self.fdb(a, b) for a, b in self.pairs]

    def near(self):
        """Host pairs whose route set can be listed: 1 to 2,000 shortest
        routes, by the exact counts (the probe switches 1-3 hops apart have
        one route each; the ones up to 13 hops apart up to 40)."""
        out = []
        for b in range(len(self.hv)):
            cnt = exact_counts(self.csr, self.dist[b])
            out += [(a, b) for a in range(len(self.hv)) if a != b and 1 <= cnt[self.hv[a]] <= 2000]
        return sorted(out, key=lambda p: (-int(self.dist[p[1], self.hv[p[0]]]), p))


def close_case(c):
    c.db.engine.ctx.synchronize()
    c.db.engine.close()


@pytest.fixture(scope="module")
def ring16():
    c = Case(B.ring_fabric(65535))
    yield c
    close_case(c)


@pytest.fixture(scope="module")
def ring17():
    c = Case(B.ring_fabric(65536, small_ports=True))
    yield c
    close_case(c)


@pytest.fixture(scope="module", autouse=True)
def drop_fabrics():
    yield
    B.clear()


def case_of(request, name):
    return request.getfixturevalue(name)


def test_layouts_picked(ring16, ring17):
    for c, lay, plane in ((ring16, EN.PORT16, "int16"), (ring17, EN.SLOT, "int32")):
        c.db.find_route(c.macs[0], c.macs[-1])
        c.db.find_route(c.macs[0], c.macs[-1], multiple=True)
        cache = c.db._cache
        assert cache.layout == lay
        tree, depth = cache.dfs.tables()
        dist, nh = cache.sp.tables()
        assert str(tree.dtype).endswith("int32") and str(depth.dtype).endswith(plane)
        assert str(dist.dtype).endswith("int16") and str(nh.dtype).endswith(plane)


def test_expected_values_are_negative_in_their_stored_type(ring16):
    """What the 65,535 case compares: parents and next hops from 32,768 up
    (negative as int16), tree words whose port half is from 0x8000 up (negative
    as int32), a host port from 0x8000 up."""
    c = ring16
    reached = c.po >= 0
    assert (c.po[reached] >= 32768).any() and (c.nh >= 32768).any()
    assert (c.to[reached] >= 0x8000).any() and (c.nhp >= 0x8000).any()
    assert (c.hp >= 0x8000).any()
    fdbs = c.routes()
    assert any(p >= 0x8000 for r in fdbs for _, p in r)
    assert any(d > 32768 for r in fdbs for d, _ in r)
    assert max(len(r) for r in fdbs) > 10000 and int(c.ho.max()) < 32768


@pytest.mark.parametrize("name", ["ring16", "ring17"])
def test_default_routes(request, name):
    c = case_of(request, name)
    db, want = c.db, c.routes()
    assert sum(1 for r in want if not r) >= 2 * len(c.macs) - 2   # the isolated / one-way switches
    assert [db.find_route(a, b) for a, b in c.mac_pairs] == want
    for k in range(0, len(c.pairs), 6):                 # the per-pair oracle on a sample
        assert O.find_route_pair(db, *c.mac_pairs[k]) == want[k]
    assert db.find_routes(c.mac_pairs) == want
    off, dp, pt = db.route_entries(c.mac_pairs)
    o = off.tolist()
    assert [list(zip(dp[o[i]:o[i + 1]].tolist(), pt[o[i]:o[i + 1]].tolist()))
            for i in range(len(want))] == want
    dpids, soff, pid, port, last = db.switch_fdb_entries(c.mac_pairs)
    table = {}
    for i, r in enumerate(want):
        for j, (d, p) in enumerate(r):
            table.setdefault(d, []).append((i, p, j == len(r) - 1))
    assert dpids.tolist() == sorted(table)
    for k in (0, len(dpids) // 2, len(dpids) - 1):
        got = list(zip(pid[soff[k]:soff[k + 1]].tolist(), port[soff[k]:soff[k + 1]].tolist(),
                       last[soff[k]:soff[k + 1]].tolist()))
        assert got == table[int(dpids[k])]
    assert int(soff[-1]) == sum(len(r) for r in want)
    w = np.random.default_rng(70).integers(0, 1 << 40, len(want)).tolist()
    assert db.link_loads(c.mac_pairs, w).as_dict() == counter_of(want, w)


@pytest.mark.parametrize("name", ["ring16", "ring17"])
def test_shortest_route_sets(request, name):
    c = case_of(request, name)
    db = c.db
    near = c.near()
    assert len(near) >= 6 and any(c.hv[a] >= 32768 and c.hv[b] >= 32768 for a, b in near)
    near = near[:8]                                              # the farthest of them
    pairs = [(c.macs[a], c.macs[b]) for a, b in near]
    sets = [O.find_routes_all_shortest(db, a, b) for a, b in pairs]
    assert all(sets)
    if name == "ring17":                                         # (at 65,535 they have one route each)
        assert max(len(s) for s in sets) >= 12
    assert [db.find_route(a, b, multiple=True) for a, b in pairs] == sets
    assert db.find_routes(pairs * 2, True) == sets * 2           # 16 pairs: the device unranking
    assert db.engine.ctx.last_kernel() == "ecmp_unrank_kernel"
    w = np.random.default_rng(71).integers(1, 1 << 32, len(pairs)).tolist()
    assert dicts_close(db.ecmp_link_loads(pairs, w).as_dict(), route_set_loads(sets, w))
    assert db.link_loads(pairs, w, route="shortest").as_dict() == \
        counter_of([s[0] for s in sets], w)
    # every host pair, against the host restatement on the oracle's distance rows
    rows = [b for _, b in c.pairs]
    srcs = [int(c.hv[a]) for a, _ in c.pairs]
    wa = np.random.default_rng(72).integers(1, 1 << 32, len(c.pairs), dtype=np.uint64)
    for split in EN.SPLITS:
        want = EN.ecmp_link_loads_host(c.csr, c.dist, rows, srcs, wa, split)
        got = db.ecmp_link_loads(c.mac_pairs, wa.tolist(), split)
        have = {(int(d), int(p)): x for d, p, x in zip(got.src_dpid.tolist(), got.port.tolist(),
                                                       got.load.tolist()) if x}
        src = np.repeat(np.arange(c.V), np.diff(c.csr.row_ptr))
        ref = {(int(src[e]) + 1, int(c.csr.port[e])): float(want[e]) for e in np.nonzero(want)[0]}
        assert ref and dicts_close(have, ref), split


@pytest.mark.parametrize("name", ["ring16", "ring17"])
def test_least_cost_routes(request, name):
    c = case_of(request, name)
    db, V = c.db, c.V
    costs = {(V, 1): 5, (V - 1, V): 3, (32769, 32770): 4, (1, V): 2}      # dpid = id + 1
    try:
        db.set_link_cost(V, 1, 5)
        db.set_link_costs({k: v for k, v in costs.items() if k != (V, 1)})
        src = np.repeat(np.arange(V), np.diff(c.csr.row_ptr))
        cost = np.ones(c.csr.E, np.uint32)
        for (a, b), x in costs.items():
            e = np.nonzero((src == a - 1) & (c.csr.col == b - 1))[0]
            assert e.size == 1
            cost[e[0]] = x
        pcost, nh, nhp = EN.cost_tables_host(c.csr, cost, c.hv)
        assert (nh >= 32768).any() and not np.array_equal(nh, c.nh)
        want = []
        for a, b in c.pairs:
            seq = follow(nh[b], int(c.hv[a]), int(c.hv[b]), V) if pcost[b, c.hv[a]] != EN.COST_INF \
                else None
            want.append([] if seq is None else
                        [(x + 1, int(nhp[b, x])) for x in seq[:-1]] + [(seq[-1] + 1, int(c.hp[b]))])
        assert db.find_routes_least_cost(c.mac_pairs) == want
        assert all(db.find_route_least_cost(*c.mac_pairs[k]) == want[k]
                   for k in range(0, len(want), 5))
        w = np.random.default_rng(73).integers(0, 1 << 32, len(want)).tolist()
        assert db.least_cost_link_loads(c.mac_pairs, w).as_dict() == counter_of(want, w)
    finally:
        db.clear_link_costs()


@pytest.mark.parametrize("name", ["ring16", "ring17"])
def test_link_events_at_the_top_ids(request, name):
    """delete_link and add_link of (V - 1, V - 2), both directions as the
    controller reports them, each followed by a requery: the incremental row
    test reads the stored depths and tree words of the top ids."""
    c = case_of(request, name)
    db, V = c.db, c.V
    before = c.routes()
    assert [db.find_route(a, b) for a, b in c.mac_pairs] == before     # the rows are resident
    ab, ba = db.links[V][V - 1], db.links[V - 1][V]
    db.delete_link(ab)
    db.delete_link(ba)
    try:
        c.tables()
        after = c.routes()
        assert after != before
        inherited = db._cache.rows_inherited
        assert [db.find_route(a, b) for a, b in c.mac_pairs] == after
        assert db._cache.rows_inherited > inherited                    # not recomputed whole
        for k in range(0, len(c.pairs), 9):
            assert O.find_route_pair(db, *c.mac_pairs[k]) == after[k]
        near = [(c.macs[a], c.macs[b]) for a, b in c.near()][:4]
        assert [db.find_route(a, b, True) for a, b in near] == \
            [O.find_routes_all_shortest(db, a, b) for a, b in near]
    finally:
        db.add_link(ab)
        db.add_link(ba)
        c.tables()
    assert c.routes() == before
    assert [db.find_route(a, b) for a, b in c.mac_pairs] == before
    assert db.find_routes(c.mac_pairs) == before


def test_chain_depths_from_32768_up():
    """chain(65535) with a host at either end and one in the middle: stored u16
    depths and distances up to 65,534 (negative as int16), one route of 65,535
    entries with port 0xFFFE all the way."""
    V = 65535
    a = np.arange(V - 1, dtype=np.int64) + 1
    fabric = T.Fabric("chain_65535", np.concatenate([a, a + 1]),
                      np.concatenate([np.full(V - 1, 0xFFFE), np.full(V - 1, 1)]),
                      np.concatenate([a + 1, a]),
                      np.concatenate([np.full(V - 1, 1), np.full(V - 1, 0xFFFE)]),
                      [T.HOST_MAC_BASE, T.HOST_MAC_BASE + 1, T.HOST_MAC_BASE + 2],
                      [1, 32769, V], [0x9000, 7, 8], range(1, V + 1))
    assert np.array_equal(fabric.csr().port, B.chain(V).port)
    c = Case(fabric)
    try:
        db = c.db
        want = c.routes()
        assert int(c.ho.max()) == 0xFFFE and len(want[2]) == V and want[2][0] == (1, 0xFFFE)
        assert [db.find_route(a, b) for a, b in c.mac_pairs] == want
        assert db._cache.layout == EN.PORT16
        off, dp, pt = db.route_entries(c.mac_pairs)
        o = off.tolist()
        assert [list(zip(dp[o[i]:o[i + 1]].tolist(), pt[o[i]:o[i + 1]].tolist()))
                for i in range(len(want))] == want
        w = [3, 5, 7, 11, 13, 17, 19, 23, 29]
        assert db.link_loads(c.mac_pairs, w).as_dict() == counter_of(want, w)
        far = db.find_route(c.macs[2], c.macs[0], multiple=True)
        assert far == [want[6]] and len(far[0]) == V
        mid = db.links[32769][32770], db.links[32770][32769]
        for lk in mid:
            db.delete_link(lk)
        c.tables()
        cut = c.routes()
        assert cut != want and [db.find_route(a, b) for a, b in c.mac_pairs] == cut
        for lk in mid:
            db.add_link(lk)
        assert [db.find_route(a, b) for a, b in c.mac_pairs] == want
    finally:
        close_case(c)
