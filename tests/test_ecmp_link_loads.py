"""ECMP link loads (TopologyDB.ecmp_link_loads and friends), CPU only: the
drop-in over an oracle-backed engine double whose loads come from
engine.ecmp_link_loads_host, pinned to the reference's own enumerated route
sets of the golden fixtures; ecmp_link_loads_host against a per-pair
enumeration of the shortest routes.

Tolerance: every term of a load is non-negative (no cancellation), so its
relative error is bounded by (float operations feeding it) x 2^-53; that
count is below 10^6 on every shape here: about 1.1e-10.  rtol = 1e-9, atol = 0
where the expected value is nonzero, exactly 0.0 where it is 0."""
import collections

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.objects import Host, Link, Port, Switch
from sdnmpi_amd.util.topology_db import SplitLinkLoads, TopologyDB
from test_link_loads import FakeLoadsEngine, golden_pairs, random_csr

RTOL = 1e-9
SPLITS = ("route", "hop")


class FakeEcmpLoadsEngine(FakeLoadsEngine):
    """The oracle-table double plus ecmp_link_loads from the numpy restatement."""

    def ecmp_link_loads(self, export, dist, rows, srcs, weights=None, split="route",
                        timing=False):
        self.calls.append(("ecmp_loads", export.key, len(rows)))
        return EN.ecmp_link_loads_host(export.csr, dist, rows, srcs, weights, split)


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeEcmpLoadsEngine()
    return db


def close(got, want):
    """Arrays: rtol where the expected value is nonzero, exact zeros elsewhere."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.isfinite(got).all():
        return False
    z = want == 0
    return bool((got[z] == 0).all()) and \
        bool(np.allclose(got[~z], want[~z], rtol=RTOL, atol=0))


def dicts_close(got, want):
    """{(dpid, port): load}: the same nonzero entries, each within rtol."""
    if set(got) != set(want):
        return False
    return all(abs(got[k] - want[k]) <= RTOL * abs(want[k]) for k in want)


def route_set_loads(route_sets, weights):
    """{(dpid, port): sum of w[i] / N_i over the routes of pair i that hold the
    entry} from enumerated route sets (lists of fdb lists), zeros dropped."""
    c = collections.defaultdict(float)
    for routes, w in zip(route_sets, weights):
        for fdb in routes:
            for ent in fdb:
                c[(int(ent[0]), int(ent[1]))] += float(w) / len(routes)
    return {k: v for k, v in c.items() if v}


# ------------------------------------------- pinned to the reference's routes --

@pytest.mark.parametrize("name", G.MULTI)
def test_route_split_equals_reference_route_sets(name):
    g = G.Golden(name)
    fabric = g.fabric()
    db = fake_db(fabric)
    pairs = golden_pairs(g, fabric)
    sets = [g.multi(i) for i in range(len(pairs))]
    got = db.ecmp_link_loads(pairs)
    assert isinstance(got, SplitLinkLoads) and got.load.dtype == np.float64
    assert dicts_close(got.as_dict(), route_set_loads(sets, [1] * len(pairs)))
    rng = np.random.default_rng(6)
    w = rng.integers(0, 1 << 32, len(pairs)).tolist()
    w[::7] = [0] * len(w[::7])
    got = db.ecmp_link_loads(pairs, w)
    assert dicts_close(got.as_dict(), route_set_loads(sets, w))
    # every route of a pair ends on the same last hop: exact integers
    assert got.host_load.dtype == np.uint64
    last = collections.Counter()
    for routes, x in zip(sets, w):
        if routes:
            last[routes[0][-1]] += x
    hk = zip(got.host_dpid.tolist(), got.host_port.tolist())
    assert dict(zip(hk, got.host_load.tolist())) == {k: v for k, v in last.items() if v}


# -------------------------------------------- ecmp_link_loads_host itself --

def edge_map(csr):
    return {(u, int(csr.col[e])): e for u in range(csr.V)
            for e in range(int(csr.row_ptr[u]), int(csr.row_ptr[u + 1]))}


def enum_loads(csr, dist, rows, srcs, weights, split):
    """Per-pair enumeration (plain Python): route split from the list of
    shortest routes (engine.shortest_paths_lex), hop split by halving,
    thirding, ... the pair's weight at every vertex of a recursive walk."""
    V = csr.V
    edge = edge_map(csr)
    load = [0.0] * csr.E
    dist = np.asarray(dist).astype(np.int64)

    def walk(r, x, f):
        if dist[r, x] == 0:
            return
        nxt = [int(n) for n in csr.col[csr.row_ptr[x]:csr.row_ptr[x + 1]]
               if dist[r, n] == dist[r, x] - 1]
        for n in nxt:
            load[edge[(x, n)]] += f / len(nxt)
            walk(r, n, f / len(nxt))

    for r, s, w in zip(rows, srcs, weights):
        r, s = int(r), int(s)
        if not 0 <= s < V or dist[r, s] == 0xFFFF or not w:
            continue
        if split == "hop":
            walk(r, s, float(w))
            continue
        d = int(np.nonzero(dist[r] == 0)[0][0])
        routes = EN.shortest_paths_lex(csr.row_ptr, csr.col, dist[r].astype(np.uint16), s, d)
        for q in routes:
            for a, b in zip(q[:-1], q[1:]):
                load[edge[(a, b)]] += float(w) / len(routes)
    return np.array(load, np.float64)


@pytest.mark.parametrize("V,extra,seed", [(1, 0, 0), (2, 0, 1), (13, 6, 2), (40, 30, 3),
                                          (90, 200, 4)])
def test_host_loads_equal_per_pair_enumeration(V, extra, seed):
    from oracle import oracle as O
    csr = random_csr(V, extra, seed) if V > 1 else T.build_csr([], [], np.zeros(0, np.int64),
                                                                extra_vertices=[1])
    rng = np.random.default_rng(seed + 200)
    dist, _, _ = O.dest_tables(csr, np.arange(csr.V, dtype=np.int32))
    n = 6 * csr.V + 3
    rows = rng.integers(0, csr.V, n)
    srcs = rng.integers(-1, csr.V + 1, n)                 # out-of-range ones included
    w = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    w[rng.random(n) < 0.3] = 0
    for split in SPLITS:
        for weights in (w, None):
            ww = w if weights is not None else np.ones(n, np.uint64)
            want = enum_loads(csr, dist, rows, srcs, ww, split)
            got = EN.ecmp_link_loads_host(csr, dist, rows, srcs, weights, split)
            assert got.dtype == np.float64 and got.shape == (csr.E,)
            assert close(got, want), (V, split)
            # the cache's plane: the same u16 values held in int16
            assert np.array_equal(
                EN.ecmp_link_loads_host(csr, dist.view(np.int16), rows, srcs, weights, split), got)
    if V >= 13:
        assert want.any() and (dist == 0xFFFF).any()


def splits_differ_csr():
    """s -> a -> m -> d, s -> b -> m1 -> d, s -> b -> m2 -> d (links both ways):
    three shortest routes, two of them through b."""
    s, a, b, m, m1, m2, d = 1, 2, 3, 4, 5, 6, 7
    und = [(s, a), (s, b), (a, m), (b, m1), (b, m2), (m, d), (m1, d), (m2, d)]
    src = [u for u, v in und] + [v for u, v in und]
    dst = [v for u, v in und] + [u for u, v in und]
    return T.build_csr(src, dst, np.arange(len(src)) + 1), (s, a, b, m, m1, m2, d)


def test_hand_computed_example_where_the_splits_differ():
    from oracle import oracle as O
    csr, names = splits_differ_csr()
    s, a, b, m, m1, m2, d = (int(csr.index_of([x])[0]) for x in names)
    dist, _, _ = O.dest_tables(csr, np.array([d], np.int32))
    assert dist[0, s] == 3
    edge = edge_map(csr)
    w = 6
    route = EN.ecmp_link_loads_host(csr, dist, [0], [s], [w], "route")
    hop = EN.ecmp_link_loads_host(csr, dist, [0], [s], [w], "hop")
    want_route = {(s, a): 2.0, (a, m): 2.0, (m, d): 2.0, (s, b): 4.0, (b, m1): 2.0,
                  (m1, d): 2.0, (b, m2): 2.0, (m2, d): 2.0}           # w/3 per route
    want_hop = {(s, a): 3.0, (a, m): 3.0, (m, d): 3.0, (s, b): 3.0, (b, m1): 1.5,
                (m1, d): 1.5, (b, m2): 1.5, (m2, d): 1.5}             # w/2 at s, then at b
    for got, want in ((route, want_route), (hop, want_hop)):
        exp = np.zeros(csr.E)
        for k, x in want.items():
            exp[edge[k]] = x
        assert close(got, exp)
    assert route[edge[(s, a)]] == pytest.approx(w / 3, rel=RTOL)
    assert hop[edge[(s, a)]] == w / 2


def test_host_loads_reject_a_row_that_is_no_bfs_labelling():
    from oracle import oracle as O
    csr, names = splits_differ_csr()
    s, a, b, m, m1, m2, d = (int(csr.index_of([x])[0]) for x in names)
    dist, _, _ = O.dest_tables(csr, np.array([d], np.int32))
    bad = dist.copy()
    bad[0, a] = 5                                         # no neighbour of a at level 4
    for split in SPLITS:
        with pytest.raises(ValueError):
            EN.ecmp_link_loads_host(csr, bad, [0], [s], None, split)
    with pytest.raises(ValueError):
        EN.ecmp_link_loads_host(csr, dist, [0], [s], None, "flow")


def test_counts_beyond_u64_do_not_saturate():
    """A ladder of 70 diamonds: 2^70 shortest routes end to end, every link
    carries exactly w / 2 under both splits."""
    from oracle import oracle as O
    csr = ladder_csr(70)
    assert csr.V == 211
    dist, _, _ = O.dest_tables(csr, np.array([csr.V - 1], np.int32))
    assert dist[0, 0] == 140
    for split in SPLITS:
        got = EN.ecmp_link_loads_host(csr, dist, [0], [0], [12345], split)
        toward = dist[0][np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))] == \
            dist[0][csr.col].astype(np.int64) + 1
        assert np.array_equal(got, np.where(toward, 12345 / 2, 0.0))


def ladder_csr(n):
    """n diamonds in a row: j_k -> {u_k, l_k} -> j_{k+1}; vertex ids (dpid - 1)
    3k, 3k + 1, 3k + 2; links both ways."""
    src, dst = [], []
    for k in range(n):
        j, u, lo, nx = 3 * k, 3 * k + 1, 3 * k + 2, 3 * k + 3
        for x, y in ((j, u), (j, lo), (u, nx), (lo, nx)):
            src += [x, y]
            dst += [y, x]
    order = sorted(range(len(src)), key=lambda i: (src[i], dst[i]))
    src = np.asarray(src)[order] + 1
    dst = np.asarray(dst)[order] + 1
    return T.build_csr(src, dst, np.arange(len(order)) % 4 + 1)


# ------------------------------------------------------------- the drop-in --

@pytest.mark.parametrize("split", SPLITS)
def test_all_pairs_equals_explicit_host_pairs(split):
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs for b in macs if a != b]
    a, b = db.all_pairs_ecmp_link_loads(split), db.ecmp_link_loads(pairs, split=split)
    assert isinstance(a, SplitLinkLoads)
    assert close(a.load, b.load) and a.load.any()
    assert dicts_close(a.as_dict(), b.as_dict())
    assert np.array_equal(a.host_dpid, b.host_dpid) and np.array_equal(a.host_load, b.host_load)
    # per_switch: every switch, float64, links and last hops included
    dp, total = a.per_switch()
    assert np.array_equal(dp, db.graph().csr.dpids) and total.dtype == np.float64
    assert total.sum() == pytest.approx(a.load.sum() + float(a.host_load.sum()), rel=RTOL)


def test_mpi_loads_are_the_rank_pairs():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    r2m = {r: macs[(5 * r) % len(macs)] for r in range(6)}
    r2m[6] = r2m[0]                                       # two ranks on one host
    ranks = sorted(r2m)
    pairs = [(r2m[a], r2m[b]) for a in ranks for b in ranks if a != b]
    assert dicts_close(db.mpi_ecmp_link_loads(r2m).as_dict(),
                       db.ecmp_link_loads(pairs).as_dict())
    traffic = {(0, 1): 10, (1, 0): 7, (2, 5): 1 << 40, (6, 3): 2, (9, 1): 4}   # rank 9 unknown
    pw = [(r2m[a], r2m[b]) for (a, b) in traffic if a in r2m and b in r2m]
    ww = [x for (a, b), x in traffic.items() if a in r2m and b in r2m]
    for split in SPLITS:
        assert dicts_close(db.mpi_ecmp_link_loads(r2m, traffic, split).as_dict(),
                           db.ecmp_link_loads(pw, ww, split).as_dict())


def two_component_db():
    db = TopologyDB()
    for d in (1, 2, 3, 4):
        db.add_switch(Switch(d))
    for u, pu, v, pv in ((1, 1, 2, 1), (3, 1, 4, 1)):
        db.add_link(Link(Port(u, pu), Port(v, pv)))
        db.add_link(Link(Port(v, pv), Port(u, pu)))
    for i, d in enumerate((1, 2, 3, 4)):
        db.add_host(Host("02:00:00:00:00:%02x" % (i + 1), Port(d, 9)))
    db._engine = FakeEcmpLoadsEngine()
    return db


@pytest.mark.parametrize("split", SPLITS)
def test_other_component_contributes_nothing(split):
    db = two_component_db()
    m = ["02:00:00:00:00:%02x" % i for i in (1, 2, 3, 4)]
    pairs = [(m[0], m[1]), (m[0], m[2]), (m[3], m[0]), (m[2], m[3])]
    assert db.find_route(m[0], m[2], True) == []
    got = db.ecmp_link_loads(pairs, [3, 100, 1000, 5], split=split).as_dict()
    assert got == {(1, 1): 3.0, (2, 9): 3.0, (3, 1): 5.0, (4, 9): 5.0}
    ap = db.all_pairs_ecmp_link_loads(split).as_dict()
    assert ap == {(1, 1): 1.0, (2, 9): 1.0, (2, 1): 1.0, (1, 9): 1.0,
                  (3, 1): 1.0, (4, 9): 1.0, (4, 1): 1.0, (3, 9): 1.0}


def test_row_chunks_under_a_small_budget():
    fabric = T.fat_tree(4)
    csr = fabric.csr()
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs for b in macs[::3]]
    for split in SPLITS:
        want = fake_db(fabric).ecmp_link_loads(pairs, split=split)
        db = fake_db(fabric, table_budget=3 * EN.sp_row_bytes(csr))
        got = db.ecmp_link_loads(pairs, split=split)
        assert close(got.load, want.load) and np.array_equal(got.host_load, want.host_load)
        assert sum(1 for c in db._engine.calls if c[0] == "ecmp_loads") > 1


def test_empty_unknown_and_bad_arguments():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    ll = db.ecmp_link_loads([])
    assert isinstance(ll, SplitLinkLoads) and ll.as_dict() == {} and not ll.load.any()
    assert ll.load.dtype == np.float64 and ll.load.shape == (db.graph().csr.E,)
    assert db.ecmp_link_loads([("02:00:00:00:00:77", macs[0]), (macs[0], "02:00:00:00:00:78")]) \
        .as_dict() == {}
    assert db.ecmp_link_loads([(macs[0], macs[5])], [0]).as_dict() == {}
    with pytest.raises(ValueError):
        db.ecmp_link_loads([(macs[0], macs[1])], [-1])
    with pytest.raises(ValueError):
        db.ecmp_link_loads([(macs[0], macs[1])], [1, 2])
    with pytest.raises(ValueError):
        db.ecmp_link_loads([(macs[0], macs[1])], split="even")
    with pytest.raises(ValueError):
        db.all_pairs_ecmp_link_loads("even")
    with pytest.raises(ValueError):
        db.mpi_ecmp_link_loads({0: macs[0], 1: macs[1]}, None, "even")
    with pytest.raises(ValueError):
        db.ecmp_link_loads([("zz:00:00:00:00:01", macs[1])])
    with pytest.raises(ValueError):                       # ECMP is its own method, not a route
        db.link_loads([(macs[0], macs[1])], route="ecmp")


def test_null_context_is_einval():
    from sdnmpi_amd import _native
    L = _native.library()
    assert L.sdnr_ecmp_link_loads(None, None, 0, None, None, None, None,
                                  _native.DEVICE_PTRS) == -22
    assert b"null context" in L.sdnr_last_error()
    assert _native.LOADS_SPLIT_HOP == 0x10
