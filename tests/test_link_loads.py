"""Predicted link loads (TopologyDB.link_loads and friends), CPU only: the
drop-in over an oracle-backed engine double whose loads come from
engine.link_loads_host, pinned to the reference's own fdb entries of the
golden fixtures; link_loads_host against a plain per-pair walk."""
import collections

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.objects import Host, Link, Port, Switch
from sdnmpi_amd.util.topology_db import OFPP_LOCAL, LinkLoads, TopologyDB
from test_topologydb_dropin import _FakeEngine

U64 = (1 << 64) - 1


class FakeLoadsEngine(_FakeEngine):
    """The oracle-table double plus link_loads from the numpy restatement."""

    def link_loads(self, export, tree, layout, rows, dsts, weights=None, to_root=False):
        self.calls.append(("loads", export.key, len(rows)))
        return EN.link_loads_host(export.csr, tree, layout, rows, dsts, weights, to_root)


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeLoadsEngine()
    return db


def counter_of(fdbs, weights):
    """{(dpid, port): sum of w[i] over fdb i's entries}, zero sums dropped."""
    c = collections.Counter()
    for fdb, w in zip(fdbs, weights):
        for ent in fdb:
            c[(int(ent[0]), int(ent[1]))] += int(w)
    return {k: v & U64 for k, v in c.items() if v & U64}


def golden_pairs(g, fabric):
    macs = fabric.host_macs()
    return [(macs[a], macs[b]) for a, b in zip(g.pair_src, g.pair_dst)]


@pytest.mark.parametrize("name", G.SMALL)
def test_default_loads_equal_reference_fdb_counts(name):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    pairs = golden_pairs(g, fabric)
    fdbs = [g.fdb(i) for i in range(len(pairs))]
    assert db.link_loads(pairs).as_dict() == counter_of(fdbs, [1] * len(pairs))
    rng = np.random.default_rng(5)
    w = rng.integers(0, 1 << 32, len(pairs)).tolist()
    w[::7] = [0] * len(w[::7])
    assert db.link_loads(pairs, w).as_dict() == counter_of(fdbs, w)


@pytest.mark.parametrize("name", G.MULTI)
def test_shortest_loads_equal_reference_first_route(name):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    pairs = golden_pairs(g, fabric)
    fdbs = [(g.multi(i) or [[]])[0] for i in range(len(pairs))]
    assert db.link_loads(pairs, route="shortest").as_dict() == counter_of(fdbs, [1] * len(pairs))
    rng = np.random.default_rng(6)
    w = rng.integers(0, 1 << 32, len(pairs)).tolist()
    assert db.link_loads(pairs, w, route="shortest").as_dict() == counter_of(fdbs, w)


def test_endpoint_cases_follow_find_route():
    from oracle import oracle as O
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs() + ["00:00:00:00:00:05", "02:00:00:00:00:77"]   # local, unknown
    pairs = [(a, b) for a in macs for b in macs]          # src == dst included
    pairs += pairs[3:40]                                  # duplicated pairs add
    w = list(range(1, len(pairs) + 1))
    want = counter_of([O.find_route_pair(db, a, b) for a, b in pairs], w)
    got = db.link_loads(pairs, w)
    assert got.as_dict() == want
    assert (5, OFPP_LOCAL) in want                        # the switch-local last hop
    sp = counter_of([(O.find_routes_all_shortest(db, a, b) or [[]])[0] for a, b in pairs], w)
    assert db.link_loads(pairs, w, route="shortest").as_dict() == sp
    # records: one per CSR edge in CSR order, zeros included; last hops sorted, nonzero
    csr = db.graph().csr
    assert got.load.shape == (csr.E,) and got.load.dtype == np.uint64
    assert np.array_equal(got.src_dpid, csr.dpids[np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))])
    assert np.array_equal(got.dst_dpid, csr.dpids[csr.col])
    assert np.array_equal(got.port, csr.port)
    hk = list(zip(got.host_dpid.tolist(), got.host_port.tolist()))
    assert hk == sorted(hk) and (got.host_load > 0).all()


def test_empty_unknown_and_bad_arguments():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    ll = db.link_loads([])
    assert isinstance(ll, LinkLoads) and ll.as_dict() == {} and not ll.load.any()
    assert db.link_loads([("02:00:00:00:00:77", macs[0]), (macs[0], "02:00:00:00:00:78")]) \
        .as_dict() == {}
    assert db.link_loads([(macs[0], macs[5])], [0]).as_dict() == {}
    with pytest.raises(ValueError):
        db.link_loads([(macs[0], macs[1])], [-1])
    with pytest.raises(ValueError):
        db.link_loads([(macs[0], macs[1])], [1, 2])
    with pytest.raises(ValueError):
        db.link_loads([(macs[0], macs[1])], route="ecmp")
    with pytest.raises(ValueError):
        db.link_loads([("zz:00:00:00:00:01", macs[1])])


def two_component_db():
    db = TopologyDB()
    for d in (1, 2, 3, 4):
        db.add_switch(Switch(d))
    for u, pu, v, pv in ((1, 1, 2, 1), (3, 1, 4, 1)):
        db.add_link(Link(Port(u, pu), Port(v, pv)))
        db.add_link(Link(Port(v, pv), Port(u, pu)))
    for i, d in enumerate((1, 2, 3, 4)):
        db.add_host(Host("02:00:00:00:00:%02x" % (i + 1), Port(d, 9)))
    db._engine = FakeLoadsEngine()
    return db


@pytest.mark.parametrize("route", ["default", "shortest"])
def test_other_component_contributes_nothing(route):
    db = two_component_db()
    m = ["02:00:00:00:00:%02x" % i for i in (1, 2, 3, 4)]
    pairs = [(m[0], m[1]), (m[0], m[2]), (m[3], m[0]), (m[2], m[3])]
    assert db.find_route(m[0], m[2]) == []
    got = db.link_loads(pairs, [3, 100, 1000, 5], route=route).as_dict()
    assert got == {(1, 1): 3, (2, 9): 3, (3, 1): 5, (4, 9): 5}
    ap = db.all_pairs_link_loads(route).as_dict()
    assert ap == {(1, 1): 1, (2, 9): 1, (2, 1): 1, (1, 9): 1,
                  (3, 1): 1, (4, 9): 1, (4, 1): 1, (3, 9): 1}


def test_per_switch_counts_installed_entries():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs[::2] for b in macs[::3] if a != b]
    dpids, off, _, _, _ = db.switch_fdb_entries(pairs)
    want = dict(zip(dpids.tolist(), np.diff(off).tolist()))
    dp, total = db.link_loads(pairs).per_switch()
    assert np.array_equal(dp, db.graph().csr.dpids)
    assert {int(d): int(x) for d, x in zip(dp, total) if x} == want


def test_mpi_link_loads_are_the_rank_pairs():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    r2m = {r: macs[(5 * r) % len(macs)] for r in range(6)}
    r2m[6] = r2m[0]                                       # two ranks on one host
    ranks = sorted(r2m)
    pairs = [(r2m[a], r2m[b]) for a in ranks for b in ranks if a != b]
    assert db.mpi_link_loads(r2m).as_dict() == db.link_loads(pairs).as_dict()
    traffic = {(0, 1): 10, (1, 0): 7, (2, 5): 1 << 40, (6, 3): 2, (9, 1): 4}   # rank 9 unknown
    pw = [(r2m[a], r2m[b]) for (a, b) in traffic if a in r2m and b in r2m]
    ww = [x for (a, b), x in traffic.items() if a in r2m and b in r2m]
    for route in ("default", "shortest"):
        assert db.mpi_link_loads(r2m, traffic, route).as_dict() == \
            db.link_loads(pw, ww, route).as_dict()


@pytest.mark.parametrize("route", ["default", "shortest"])
def test_all_pairs_equals_explicit_host_pairs(route):
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs for b in macs if a != b]
    a, b = db.all_pairs_link_loads(route), db.link_loads(pairs, route=route)
    assert np.array_equal(a.load, b.load) and a.load.any()
    assert a.as_dict() == b.as_dict()
    assert np.array_equal(a.host_dpid, b.host_dpid) and np.array_equal(a.host_load, b.host_load)


def test_row_chunks_under_a_small_budget():
    fabric = T.fat_tree(4)
    csr = fabric.csr()
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs for b in macs[::3]]
    want = fake_db(fabric).link_loads(pairs).as_dict()
    db = fake_db(fabric, table_budget=3 * EN.dfs_row_bytes(csr))
    assert db.link_loads(pairs).as_dict() == want
    assert sum(1 for c in db._engine.calls if c[0] == "loads") > 1
    assert db.link_loads(pairs, route="shortest").as_dict() == \
        fake_db(fabric).link_loads(pairs, route="shortest").as_dict()


# ------------------------------------------------- link_loads_host itself --

def walk_loads(csr, parent, rows, dsts, weights, to_root):
    """Per-pair walk up the parent row, one edge at a time (plain Python)."""
    V = csr.V
    edge = {}
    for u in range(V):
        for e in range(int(csr.row_ptr[u]), int(csr.row_ptr[u + 1])):
            edge[(u, int(csr.col[e]))] = e
    load = [0] * csr.E
    for r, d, w in zip(rows, dsts, weights):
        if not 0 <= d < V:
            continue
        row = parent[r]
        x = int(d)
        # an unreached d has no parent at all; a reached one climbs to the root
        while int(row[x]) >= 0 and int(row[x]) != x:
            p = int(row[x])
            e = edge[(x, p)] if to_root else edge[(p, x)]
            load[e] = (load[e] + int(w)) & U64
            x = p
    return np.array(load, np.uint64)


def random_csr(V, extra, seed):
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for v in range(1, V - V // 5):                        # the last fifth stays unreachable
        u = int(rng.integers(0, v))
        src += [u, v]
        dst += [v, u]
    for _ in range(extra):
        u, v = (int(x) for x in rng.integers(0, V - V // 5, 2))
        if u != v:
            src += [u, v]
            dst += [v, u]
    keys = sorted(set(zip(src, dst)))
    src = np.asarray([k[0] for k in keys]) + 1
    dst = np.asarray([k[1] for k in keys]) + 1
    return T.build_csr(src, dst, np.arange(len(keys)) % 50 + 1,
                       extra_vertices=list(range(1, V + 1)))


@pytest.mark.parametrize("V,extra,seed", [(1, 0, 0), (2, 0, 1), (13, 6, 2), (40, 30, 3),
                                          (90, 200, 4)])
def test_host_loads_equal_per_pair_walk(V, extra, seed):
    from oracle import oracle as O
    csr = random_csr(V, extra, seed) if V > 1 else T.build_csr([], [], np.zeros(0, np.int64),
                                                                extra_vertices=[1])
    rng = np.random.default_rng(seed + 100)
    srcs = np.arange(csr.V, dtype=np.int32)
    par, prt, _ = O.dfs_tables(csr, srcs)
    _, nh, _ = O.dest_tables(csr, srcs)
    n = 6 * csr.V + 3
    rows = rng.integers(0, csr.V, n)
    dsts = rng.integers(-1, csr.V + 1, n)                 # out-of-range ones included
    w = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    for weights in (w, None):
        ww = w if weights is not None else np.ones(n, np.uint64)
        want = walk_loads(csr, par, rows, dsts, ww, False)
        assert np.array_equal(EN.link_loads_host(csr, par, EN.INT32, rows, dsts, weights), want)
        for lay in (EN.PORT16, EN.SLOT):
            tree = EN.pack_host_tree(par, prt, csr, lay)
            assert np.array_equal(EN.link_loads_host(csr, tree, lay, rows, dsts, weights), want)
        want = walk_loads(csr, nh, rows, dsts, ww, True)
        assert np.array_equal(EN.link_loads_host(csr, nh, EN.INT32, rows, dsts, weights, True),
                              want)


def test_host_loads_reject_a_cycle():
    csr = random_csr(13, 6, 2)
    from oracle import oracle as O
    par, _, _ = O.dfs_tables(csr, np.arange(2, dtype=np.int32))
    par = par.copy()
    a = int(np.nonzero(par[0] == 0)[0][1])                # a child of the root 0
    par[0, 0] = a                                         # 2-cycle root <-> child
    with pytest.raises(ValueError):
        EN.link_loads_host(csr, par, EN.INT32, [0], [a], None)


def test_null_context_is_einval():
    from sdnmpi_amd import _native
    L = _native.library()
    assert L.sdnr_link_loads(None, None, 0, 0, None, None, None, None, _native.DEVICE_PTRS) == -22
    assert b"null context" in L.sdnr_last_error()
    assert _native.LOADS_TO_ROOT == 0x8


def test_pairs_for_device_orders_clamps_and_names_the_caller():
    """_pairs_for_device, the marshalling every pair-list engine call shares:
    a stable order by row, the offsets, vertices outside [0, V) at -1, the
    weights in the same order."""
    V, nrows = 5, 4
    rows = np.array([2, 0, 3, 0, 2], np.int64)                    # unsorted; row 1 has no pairs
    verts = np.array([4, -1, V, 0, 3], np.int64)                  # -1 and V are no vertices
    w = np.array([10, 20, 30, 40, U64], np.uint64)
    order, off, x, wo = EN._pairs_for_device(rows, nrows, verts, V, w, "link_loads")
    assert order.tolist() == [1, 3, 0, 4, 2]                      # stable within a row
    assert off.dtype == np.int64 and off.tolist() == [0, 2, 2, 4, 5]
    assert x.dtype == np.int32 and x.tolist() == [-1, 0, 4, 3, -1]
    assert wo.dtype == np.uint64 and wo.flags.c_contiguous
    assert wo.tolist() == [20, 40, 10, U64, 30]
    got = np.array([7, 8, 9, 10, 11])                             # results in device order
    assert EN._unsorted(got, order).tolist() == [9, 7, 11, 8, 10]
    assert EN._unsorted(np.stack([got, got + 10]), order).tolist() == \
        [[9, 7, 11, 8, 10], [19, 17, 21, 18, 20]]

    # no weights: every pair weighs 1 on the device
    assert EN._pairs_for_device(rows, nrows, verts, V, None, "link_loads")[3] is None

    # rows already grouped: nothing is permuted
    srt = np.array([0, 0, 2, 3], np.int64)
    order, off, x, wo = EN._pairs_for_device(srt, nrows, [1, 2, 3, 4], V, [1, 2, 3, 4], "f")
    assert isinstance(order, slice) and off.tolist() == [0, 2, 2, 3, 4]
    assert x.tolist() == [1, 2, 3, 4] and wo.tolist() == [1, 2, 3, 4]
    assert EN._unsorted(got, order) is got

    # an empty list
    order, off, x, wo = EN._pairs_for_device(np.zeros(0, np.int64), nrows, [], V, None, "f")
    assert isinstance(order, slice) and off.tolist() == [0] * (nrows + 1)
    assert x.dtype == np.int32 and x.shape == (0,) and wo is None

    # a row index outside [0, nrows) raises in the caller's name
    with pytest.raises(ValueError,
                       match=r"^ecmp_link_loads: a pair names a row outside the table$"):
        EN._pairs_for_device([0, nrows], nrows, [0, 0], V, None, "ecmp_link_loads")
    with pytest.raises(ValueError,
                       match=r"^whatif_ecmp_link_loads: a pair names a row outside dsts$"):
        EN._pairs_for_device([-1], nrows, [0], V, None, "whatif_ecmp_link_loads", "dsts")
