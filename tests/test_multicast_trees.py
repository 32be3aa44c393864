"""Multicast trees (TopologyDB.multicast_trees and friends), CPU only:
engine.multicast_trees_host against a plain per-member walk, the tree property
of the unions, and the drop-in over an oracle-backed engine double, pinned to
the reference's own fdb entries of the golden fixtures.  Every comparison is
exact integer equality."""
import collections

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.objects import Host, Link, Port, Switch
from sdnmpi_amd.util.topology_db import OFPP_LOCAL, LinkLoads, MulticastTree, TopologyDB
from test_cost_tables import FakeCostEngine

U64 = (1 << 64) - 1


# ------------------------------------------- multicast_trees_host itself --

def edge_map(csr):
    return {(u, int(csr.col[e])): e for u in range(csr.V)
            for e in range(int(csr.row_ptr[u]), int(csr.row_ptr[u + 1]))}


def walk_groups(csr, table, nrows, root, mem_off, mem_row, mem_vertex, weights, to_root):
    """One member at a time, one link at a time (plain Python): ``table`` holds
    int parents (root: itself or -1; unreached: -1) or next hops."""
    V = csr.V
    edge = edge_map(csr)
    reached = [0] * len(mem_row)
    sets = []
    load = [0] * csr.E
    for g, r in enumerate(root):
        links = set()
        for i in range(int(mem_off[g]), int(mem_off[g + 1])):
            row, v = int(mem_row[i]), int(mem_vertex[i])
            if not (0 <= r < V and 0 <= row < nrows and 0 <= v < V):
                continue
            if v == r:
                reached[i] = 1
                continue
            if to_root:
                if int(table[row][r]) < 0:
                    continue
                reached[i] = 1
                x = int(r)
                while x != v:
                    n = int(table[row][x])
                    links.add(edge[(x, n)])
                    x = n
            else:
                if int(table[row][v]) < 0:
                    continue
                reached[i] = 1
                x = v
                while x != r:
                    p = int(table[row][x])
                    links.add(edge[(p, x)])
                    x = p
        sets.append(sorted(links))
        for e in links:
            load[e] = (load[e] + int(weights[g])) & U64
    off = np.zeros(len(root) + 1, np.int64)
    np.cumsum([len(s) for s in sets], out=off[1:])
    ent = np.asarray([e for s in sets for e in s], np.int32)
    return np.asarray(reached, np.uint8), off, ent, np.asarray(load, np.uint64)


def random_groups(V, rng, to_root):
    """Every vertex as a root (and two roots outside [0, V)); member sets:
    empty, singleton, all vertices, random ones with repeats, the root itself
    and ids outside [0, V)."""
    root, off, row, vert = [], [0], [], []
    for g in list(range(V)) + [-1, V]:
        kind = g % 5 if 0 <= g < V else 3
        if kind == 0:
            ms = []
        elif kind == 1:
            ms = [int(rng.integers(0, V))]
        elif kind == 2:
            ms = list(range(V))
        else:
            ms = rng.integers(-1, V + 2, int(rng.integers(2, 14))).tolist()
            ms += ms[:3] + [g]                            # repeats, the root itself
        for v in ms:
            vert.append(v)
            # the row: the root's tree / the member's own next-hop row; some outside the table
            r = v if to_root else g
            row.append(r if rng.integers(0, 9) else int(rng.choice([-1, V])))
        root.append(g)
        off.append(len(vert))
    return (np.asarray(root, np.int64), np.asarray(off, np.int64), np.asarray(row, np.int64),
            np.asarray(vert, np.int64))


def full_weights(n, rng):
    w = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, n, dtype=np.uint64)
    w[::3] = np.uint64(U64)                               # sums wrap
    w[1::7] = np.uint64(0)
    return w


def same(got, want):
    return all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))


def fabric_cost(csr, seed):
    return np.random.default_rng(seed).integers(1, 9, int(csr.E)).astype(np.uint32)


@pytest.mark.parametrize("name", G.SMALL)
def test_host_trees_equal_per_member_walk(name):
    from oracle import oracle as O
    csr = G.Golden(name).fabric().csr()
    V = csr.V
    ids = np.arange(V, dtype=np.int32)
    rng = np.random.default_rng(len(name) + V)
    par, prt, _ = O.dfs_tables(csr, ids)
    root, off, row, vert = random_groups(V, rng, False)
    w = full_weights(root.shape[0], rng)
    for weights in (w, None):
        ww = w if weights is not None else np.ones(root.shape[0], np.uint64)
        want = walk_groups(csr, par, V, root, off, row, vert, ww, False)
        assert want[2].size and want[0].any() and not want[0].all()
        assert same(EN.multicast_trees_host(csr, par, EN.INT32, root, off, row, vert, weights),
                    want)
        for lay in (EN.PORT16, EN.SLOT):
            tree = EN.pack_host_tree(par, prt, csr, lay)
            assert same(EN.multicast_trees_host(csr, tree, lay, root, off, row, vert, weights),
                        want)
    _, nh, _ = O.dest_tables(csr, ids)
    _, cnh, _ = EN.cost_tables_host(csr, fabric_cost(csr, V), ids)
    root, off, row, vert = random_groups(V, rng, True)
    for tab in (nh, cnh):
        want = walk_groups(csr, tab, V, root, off, row, vert, w, True)
        assert want[2].size and want[0].any()
        assert same(EN.multicast_trees_host(csr, tab, EN.INT32, root, off, row, vert, w, True),
                    want)


@pytest.mark.parametrize("name", G.SMALL)
def test_unions_are_trees(name):
    """Every switch of a union has at most one incoming link; with every vertex
    a member the union has exactly (reached - 1) links (the root reads reached)."""
    from oracle import oracle as O
    csr = G.Golden(name).fabric().csr()
    V = csr.V
    ids = np.arange(V, dtype=np.int32)
    par, _, _ = O.dfs_tables(csr, ids)
    _, nh, _ = O.dest_tables(csr, ids)
    _, cnh, _ = EN.cost_tables_host(csr, fabric_cost(csr, V + 1), ids)
    root = np.arange(V)
    off = np.arange(V + 1) * V
    vert = np.tile(np.arange(V), V)
    for tab, to_root in ((par, False), (nh, True), (cnh, True)):
        row = vert if to_root else np.repeat(root, V)
        reached, eo, ee, load = EN.multicast_trees_host(csr, tab, EN.INT32, root, off, row, vert,
                                                        None, to_root)
        cnt = reached.reshape(V, V).sum(1)
        assert np.array_equal(np.diff(eo), cnt - 1)
        for g in range(V):
            heads = np.asarray(csr.col)[ee[eo[g]:eo[g + 1]]]
            assert np.unique(heads).size == heads.size and g not in heads
        assert int(load.sum()) == int(eo[-1])


def test_host_trees_reject_rows_that_are_no_trees():
    from oracle import oracle as O
    csr = G.Golden("random_V12").fabric().csr()
    par, _, _ = O.dfs_tables(csr, np.arange(2, dtype=np.int32))
    kids = np.nonzero(par[0] == 0)[0]
    a = int(kids[kids != 0][0])                           # a child of the root 0
    deep = int(np.nonzero((par[0] >= 0) & (par[0] != 0) & (np.arange(csr.V) != 0))[0][0])
    cyc = par.copy()
    cyc[0, a] = deep                                      # a climbs into its own subtree or a cycle
    cyc[0, deep] = a
    with pytest.raises(ValueError):
        EN.multicast_trees_host(csr, cyc, EN.INT32, [0], [0, 1], [0], [deep])
    has = edge_map(csr)
    far = next(v for v in range(1, csr.V) if (v, a) not in has and v != a and par[0, v] >= 0)
    bad = par.copy()
    bad[0, a] = far                                       # far -> a is no link of the graph
    with pytest.raises(ValueError):
        EN.multicast_trees_host(csr, bad, EN.INT32, [0], [0, 1], [0], [a])
    with pytest.raises(ValueError):
        EN.multicast_trees_host(csr, par, EN.INT32, [0], [0, 2], [0], [a])


def test_null_context_is_einval():
    from sdnmpi_amd import _native
    L = _native.library()
    assert L.sdnr_multicast_trees(None, None, 0, 0, 0, None, None, None, None, None, None, None,
                                  None, None, None, _native.DEVICE_PTRS) == -22
    assert b"null context" in L.sdnr_last_error()
    assert _native.MCAST_TO_ROOT == 0x40
    assert EN.multicast_maps_in_lds(2880, 110592) and not EN.multicast_maps_in_lds(40000, 230000)


# ------------------------------------- the drop-in over the restatement --

class FakeMcastEngine(FakeCostEngine):
    """The oracle-table double plus multicast_trees from the restatement."""

    def multicast_trees(self, export, tree, layout, root, mem_off, mem_row, mem_vertex,
                        weights=None, to_root=False, entries=True, loads=True):
        self.calls.append(("mcast", export.key, len(mem_row)))
        r, eo, ee, ld = EN.multicast_trees_host(export.csr, tree, layout, root, mem_off, mem_row,
                                                mem_vertex, weights, to_root)
        return r, eo, (ee if entries else None), (ld if loads else None)


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeMcastEngine()
    return db


def union_of(fdbs):
    return sorted(set(e for fdb in fdbs for e in fdb))


def golden_groups(g, fabric, route_of):
    """{src index: (member macs, union of the reference's fdbs)} of the golden pairs."""
    macs = fabric.host_macs()
    by = collections.OrderedDict()
    for i, (a, b) in enumerate(zip(g.pair_src.tolist(), g.pair_dst.tolist())):
        ms, fdbs = by.setdefault(a, ([], []))
        ms.append(macs[b])
        if a != b:                                        # m == src drops out
            fdbs.append(route_of(i))
    return [(macs[a], ms, union_of(fdbs)) for a, (ms, fdbs) in by.items()]


def slices(off, dpid, port):
    return [list(zip(dpid[off[i]:off[i + 1]].tolist(), port[off[i]:off[i + 1]].tolist()))
            for i in range(len(off) - 1)]


def loads_of(unions, weights):
    c = collections.Counter()
    for u, w in zip(unions, weights):
        for ent in u:
            c[ent] += int(w)
    return {k: v & U64 for k, v in c.items() if v & U64}


@pytest.mark.parametrize("name", G.SMALL)
def test_default_trees_are_unions_of_reference_fdbs(name):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    groups = golden_groups(g, fabric, g.fdb)
    assert any(len(u) > 2 for _, _, u in groups)
    for src, ms, want in groups[:6]:
        t = db.multicast_tree(src, ms)
        assert isinstance(t, MulticastTree) and t.entries == want
    off, dpid, port = db.multicast_trees([(s, ms) for s, ms, _ in groups])
    assert slices(off, dpid, port) == [u for _, _, u in groups]
    assert off.dtype == np.int64 and port.dtype == np.int32
    w = full_weights(len(groups), np.random.default_rng(9)).tolist()
    ll = db.multicast_link_loads([(s, ms) for s, ms, _ in groups], w)
    assert isinstance(ll, LinkLoads)
    assert ll.as_dict() == loads_of([u for _, _, u in groups], w)


@pytest.mark.parametrize("name", G.MULTI)
def test_shortest_trees_are_unions_of_reference_first_routes(name):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    groups = golden_groups(g, fabric, lambda i: (g.multi(i) or [[]])[0])
    off, dpid, port = db.multicast_trees([(s, ms) for s, ms, _ in groups], route="shortest")
    assert slices(off, dpid, port) == [u for _, _, u in groups]
    assert db.multicast_tree(*groups[0][:2], route="shortest").entries == groups[0][2]
    w = list(range(1, len(groups) + 1))
    assert db.multicast_link_loads([(s, ms) for s, ms, _ in groups], w, "shortest").as_dict() == \
        loads_of([u for _, _, u in groups], w)


@pytest.mark.parametrize("name", ["fat_tree_k4", "torus_2x2x2_loops", "random_V40", "mock"])
def test_least_cost_trees_are_unions_of_least_cost_routes(name):
    fabric = G.Golden(name).fabric()
    db = fake_db(fabric)
    rng = np.random.default_rng(4)
    db.set_link_costs({(a, b): int(rng.integers(1, 9)) for a in db.links for b in db.links[a]})
    macs = fabric.host_macs()
    groups = [(macs[i], [macs[j] for j in rng.permutation(len(macs))[:7].tolist()])
              for i in range(0, len(macs), max(1, len(macs) // 5))]
    want = [union_of(db.find_route_least_cost(s, m) for m in ms if m != s) for s, ms in groups]
    off, dpid, port = db.multicast_trees(groups, route="least_cost")
    assert slices(off, dpid, port) == want and any(len(u) > 2 for u in want)
    w = [3 * i + 1 for i in range(len(groups))]
    assert db.multicast_link_loads(groups, w, "least_cost").as_dict() == loads_of(want, w)


def bcast_restatement(db, r2m, roots, route_of):
    """Per root rank, per member rank, one route at a time."""
    per = collections.defaultdict(list)                   # dpid -> [(root, transit?, key, port, dst)]
    for r in roots:
        transit, deliver = set(), []
        for j in sorted(r2m):
            if j == r or r2m[j] == r2m[r]:
                continue
            fdb = route_of(r2m[r], r2m[j])
            if not fdb:
                continue
            transit.update(fdb[:-1])
            deliver.append((fdb[-1], j))
        for d, p in sorted(transit):
            per[d].append((r, p, -1))
        for (d, p), j in deliver:
            per[d].append((r, p, j))
    dpids = sorted(per)
    off = np.zeros(len(dpids) + 1, np.int64)
    rr, pt, dr = [], [], []
    for k, d in enumerate(dpids):
        ents = sorted(per[d], key=lambda t: (t[0], t[2] >= 0, t[2], t[1]))
        off[k + 1] = off[k] + len(ents)
        rr += [t[0] for t in ents]
        pt += [t[1] for t in ents]
        dr += [t[2] for t in ents]
    return dpids, off.tolist(), rr, pt, dr


def test_mpi_bcast_entries_follow_the_per_rank_routes():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    r2m = {r: macs[(5 * r) % len(macs)] for r in range(7)}
    r2m[7] = r2m[0]                                       # two ranks on one host
    r2m[8] = "00:00:00:00:00:05"                          # a rank on a switch-local MAC
    r2m[9] = "02:00:00:00:00:77"                          # ... and on an unknown one
    for route, route_of in (("default", db.find_route),
                            ("shortest", lambda a, b: (db.find_route(a, b, True) or [[]])[0])):
        for roots in (None, [3, 8, 0, 42]):
            got = db.mpi_bcast_entries(r2m, roots, route)
            want = bcast_restatement(db, r2m, sorted(r2m) if roots is None else
                                     [r for r in roots if r in r2m], route_of)
            assert [x.tolist() for x in got] == [list(x) for x in want]
            assert got[3].dtype == np.int32
    dpids, off, rr, pt, dr = db.mpi_bcast_entries(r2m)
    assert ((pt == OFPP_LOCAL) & (dr == 8)).any()
    k = dpids.tolist().index(db.hosts[r2m[0]].port.dpid)
    mine = slice(off[k], off[k + 1])
    both = set(zip(rr[mine][dr[mine] == 0].tolist(), pt[mine][dr[mine] == 0].tolist()))
    assert both and both == set(zip(rr[mine][dr[mine] == 7].tolist(),
                                    pt[mine][dr[mine] == 7].tolist()))
    assert not (rr == 9).any() and not (dr == 9).any()
    # the loads of the same broadcasts: each tree's links and last-hop ports once
    ranks = sorted(r2m)
    groups = [(r2m[a], [r2m[b] for b in ranks if b != a]) for a in ranks]
    assert db.mpi_bcast_link_loads(r2m).as_dict() == db.multicast_link_loads(groups).as_dict()
    traffic = {0: 10, 3: 1 << 40, 8: 7, 42: 5}            # rank 42 unknown
    assert db.mpi_bcast_link_loads(r2m, traffic, "shortest").as_dict() == \
        db.multicast_link_loads([groups[0], groups[3], groups[8]], [10, 1 << 40, 7],
                                "shortest").as_dict()


def two_component_db():
    db = TopologyDB()
    for d in (1, 2, 3, 4):
        db.add_switch(Switch(d))
    for u, pu, v, pv in ((1, 1, 2, 1), (3, 1, 4, 1)):
        db.add_link(Link(Port(u, pu), Port(v, pv)))
        db.add_link(Link(Port(v, pv), Port(u, pu)))
    for i, d in enumerate((1, 2, 3, 4)):
        db.add_host(Host("02:00:00:00:00:%02x" % (i + 1), Port(d, 9)))
    db._engine = FakeMcastEngine()
    return db


@pytest.mark.parametrize("route", ["default", "shortest", "least_cost"])
def test_unknown_and_unreachable_members(route):
    db = two_component_db()
    m = ["02:00:00:00:00:%02x" % i for i in (1, 2, 3, 4)]
    ghost = "02:00:00:00:00:77"
    t = db.multicast_tree(m[0], [m[1], m[2], ghost, m[0], m[3], m[1]], route)
    assert t.entries == [(1, 1), (2, 9)] and t.as_dict() == {1: (1,), 2: (9,)}
    assert t.unreached == [m[2], ghost, m[3]]
    t = db.multicast_tree(ghost, [m[0], m[1]], route)
    assert t.entries == [] and t.unreached == [m[0], m[1]] and t.as_dict() == {}
    t = db.multicast_tree(m[2], [], route)
    assert t.entries == [] and t.unreached == []
    off, dpid, port = db.multicast_trees([], route)
    assert off.tolist() == [0] and dpid.size == 0 and port.size == 0
    off, dpid, port = db.multicast_trees([(m[0], [m[0]]), (m[2], [m[3], m[0]]), (ghost, [m[1]])],
                                         route)
    assert slices(off, dpid, port) == [[], [(3, 1), (4, 9)], []]
    ll = db.multicast_link_loads([(m[0], [m[1], m[2]]), (m[3], [m[2], ghost])], [5, 9], route)
    assert ll.as_dict() == {(1, 1): 5, (2, 9): 5, (4, 1): 9, (3, 9): 9}
    assert db.multicast_link_loads([], None, route).as_dict() == {}
    with pytest.raises(ValueError):
        db.multicast_link_loads([(m[0], [m[1]])], [1, 2], route)
    with pytest.raises(ValueError):
        db.multicast_tree("zz:00:00:00:00:01", [m[1]], route)


def test_switch_local_and_same_switch_members():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    sw = db.hosts[macs[0]].port.dpid
    mate = next(x for x in macs[1:] if db.hosts[x].port.dpid == sw)
    local = "00:00:00:00:00:05"
    t = db.multicast_tree(macs[0], [mate, local, macs[-1]])
    want = union_of(db.find_route(macs[0], x) for x in (mate, local, macs[-1]))
    assert t.entries == want and (5, OFPP_LOCAL) in want
    assert (sw, db.hosts[mate].port.port_no) in want
    assert t.unreached == [] and len(t.as_dict()[sw]) >= 2


def test_refused_routes_and_engines():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    for call in (lambda r: db.multicast_tree(macs[0], macs[1:4], r),
                 lambda r: db.multicast_trees([(macs[0], macs[1:4])], r),
                 lambda r: db.multicast_link_loads([(macs[0], macs[1:4])], None, r),
                 lambda r: db.mpi_bcast_entries({0: macs[0], 1: macs[5]}, None, r),
                 lambda r: db.mpi_bcast_link_loads({0: macs[0], 1: macs[5]}, None, r)):
        for route in ("least_loaded", "ecmp"):
            with pytest.raises(ValueError):
                call(route)
    old = fabric.populate(TopologyDB())
    old._engine = FakeCostEngine()                        # the double without multicast_trees
    with pytest.raises(ValueError):
        old.multicast_tree(macs[0], macs[1:4])
    with pytest.raises(ValueError):
        old.multicast_link_loads([(macs[0], macs[1:4])])


@pytest.mark.parametrize("route", ["default", "shortest", "least_cost"])
def test_row_chunks_under_a_small_budget(route):
    fabric = T.fat_tree(4)
    csr = fabric.csr()
    macs = fabric.host_macs()
    groups = [(a, macs[i % 3::3]) for i, a in enumerate(macs)]
    w = list(range(1, len(groups) + 1))
    whole = fake_db(fabric)
    row_bytes = {"default": EN.dfs_row_bytes(csr), "shortest": EN.sp_row_bytes(csr),
                 "least_cost": 12 * csr.V}[route]
    db = fake_db(fabric, table_budget=3 * row_bytes)
    a, b = whole.multicast_trees(groups, route), db.multicast_trees(groups, route)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[0][-1] > 0
    assert sum(1 for c in db._engine.calls if c[0] == "mcast") > 1
    assert sum(1 for c in whole._engine.calls if c[0] == "mcast") == 1
    assert db.multicast_link_loads(groups, w, route).as_dict() == \
        whole.multicast_link_loads(groups, w, route).as_dict()


@pytest.mark.parametrize("name", ["fat_tree_k8", "dragonfly_a4_h2_p2", "torus_4x4x4"])
@pytest.mark.parametrize("route", ["default", "shortest"])
def test_multicast_peak_is_no_greater_than_the_unicast_fan_out(name, route):
    fabric = G.Golden(name).fabric()
    db = fake_db(fabric)
    macs = fabric.host_macs()
    groups = [(a, [m for m in macs[i % 2::2] if m != a]) for i, a in enumerate(macs[::3])]
    assert all(len(set(db.hosts[m].port.dpid for m in ms)) > 1 for _, ms in groups)
    w = [7 * i + 1 for i in range(len(groups))]
    multi = db.multicast_link_loads(groups, w, route)
    fan = db.link_loads([(a, m) for a, ms in groups for m in ms],
                        [x for (a, ms), x in zip(groups, w) for _ in ms], route)
    assert 0 < int(multi.load.max()) <= int(fan.load.max())
    assert max(multi.as_dict().values()) <= max(fan.as_dict().values())
    assert (multi.load <= fan.load).all()
    # a single member: the multicast tree is the route
    single = [(a, ms[:1]) for a, ms in groups]
    assert db.multicast_link_loads(single, w, route).as_dict() == \
        db.link_loads([(a, ms[0]) for a, ms in single], w, route).as_dict()
