"""Max-min fair completion times (engine.fair_times_host,
TopologyDB.fair_completion_times and friends), CPU only: the numpy restatement
of fair_times.hip against an event simulation in exact fractions -- textbook
progressive filling (test_fair_rates.exact_fair), advance to the first
departure, refill --, closed forms, conservation of bytes, the relations to
fair_rates, and the drop-in over an engine double built from the restatements.

With seeded integer byte sizes the epochs, every flow's epoch and the rounds
of every filling must equal the exact simulation; times, epoch times and
carried bytes agree within TOL (16 times the largest relative
deviation measured over the seeded cases of this file, capped at 1e-9).  Byte
sizes with many exact ties are compared on times and carried bytes only: ties
may round one ulp of dt apart and leave in consecutive epochs."""
from fractions import Fraction

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import FlowTimes, SplitLinkLoads, TopologyDB
from test_ecmp_link_loads import edge_map
from test_fair_rates import (CAPS, ROUTES, FakeFairEngine, dropin_pairs, exact_fair, line_csr,
                             line_to_end, route_of, small_case, table_paths)
from test_fair_rates import layout_tree

# largest relative deviation of a time, an epoch time, a flow's bytes left or a
# link's carried bytes measured over the seeded cases below (integer, {1, 2, 3,
# 8} and unit byte sizes, the drop-in cases included; the tests print it per
# case): 1.58e-15 (fat_tree_k4, integer sizes, 320 epochs and 5,623 rounds on
# the next-hop rows); 16 times that, far below the 1e-9 cap
MEASURED_DEV = 1.58e-15
TOL = min(16 * MEASURED_DEV, 1e-9)
LAYOUTS = (EN.INT32, EN.PORT16, EN.SLOT)
FABRICS = ["mock", "torus_2x2x2", "random_V9", "random_V12", "fat_tree_k4",
           "fat_tree_k4_loops", "torus_2x2x2_loops", "random_V12_loops"]
INF = float("inf")


class FakeTimesEngine(FakeFairEngine):
    """The restatement double plus fair_times."""

    def fair_times(self, export, tree, layout, rows, verts, mult=None, nbytes=1.0, cap=None,
                   extra=None, to_root=False, max_epochs=None, timing=False):
        self.calls.append(("times", export.key, len(rows)))
        if cap is None:
            cap = np.ones(int(export.csr.E))
        return EN.fair_times_host(export.csr, tree, layout, rows, verts, mult, nbytes, cap, extra,
                                  to_root, max_epochs)


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeTimesEngine()
    return db


# ------------------------------------------------ the exact reference --

def exact_times(paths, mult, nbytes, cap, max_epochs=None):
    """The event simulation in exact fractions: fill (exact_fair), advance to
    the first departure, drop the flows that are done, again.  Returns (time
    -- Fractions, inf for a flow that never ends --, epoch, rate0, left,
    epoch_time, epoch_rounds, carried)."""
    n = len(paths)
    m = np.asarray(mult, np.int64).copy()
    left = [Fraction(b) for b in nbytes]
    time, epoch = [INF] * n, [-1] * n
    for i, p in enumerate(paths):
        if p is not None and m[i] > 0 and (not p or left[i] == 0):
            time[i] = Fraction(0)
            if not p:
                left[i] = Fraction(0)
    rate0 = exact_fair(paths, np.where([b == 0 for b in left], 0, m), cap)[0]
    for i, p in enumerate(paths):
        if p is not None and m[i] > 0 and not p:
            rate0[i] = INF
    m[[i for i in range(n) if left[i] == 0]] = 0
    carried = [Fraction(0)] * len(cap)
    t = Fraction(0)
    e_time, e_rounds = [], []
    j = 0
    while True:
        rate, _, rnd, levels, used = exact_fair(paths, m, cap)
        fl = [i for i in range(n) if rnd[i] >= 0]
        if not fl:
            break
        if max_epochs is not None and j == max_epochs:
            for i in fl:
                epoch[i] = -2
            break
        dt = min(left[i] / rate[i] for i in fl)
        t += dt
        carried = [c + u * dt for c, u in zip(carried, used)]
        for i in fl:
            left[i] -= rate[i] * dt
            if left[i] == 0:
                time[i], epoch[i], m[i] = t, j, 0
        e_time.append(t)
        e_rounds.append(len(levels))
        j += 1
    return time, epoch, rate0, left, e_time, e_rounds, carried


def rel_dev(got, want):
    """Largest |got - want| / want over the finite nonzero entries of ``want``
    (Fractions); everything else must be equal."""
    worst = 0.0
    for g, w in zip(np.asarray(got).tolist(), want):
        if w == INF or w == 0:
            assert g == w
        else:
            worst = max(worst, float(abs(Fraction(g) - w) / w))
    return worst


def check_case(csr, tab, layout, tree, rows, verts, mult, nbytes, cap, to_root, extra=None,
               exact=None, same_epochs=True, max_epochs=None):
    """fair_times_host of one case against the exact simulation; returns the
    largest relative deviation and the simulation."""
    paths = table_paths(csr, tab, rows, verts, to_root, extra)
    m = np.ones(len(paths), np.int64) if mult is None else np.asarray(mult).astype(np.int64)
    if exact is None:
        exact = exact_times(paths, m, nbytes, cap, max_epochs)
    got = EN.fair_times_host(csr, tree, layout, rows, verts, mult, nbytes, cap, extra, to_root,
                             max_epochs)
    time, epoch, rate0, left, e_time, e_rounds, carried = got
    assert time.dtype == np.float64 and epoch.dtype == np.int32 and e_rounds.dtype == np.int32
    dev = max(rel_dev(time, exact[0]), rel_dev(carried, exact[6]))
    if same_epochs:
        assert len(e_time) == len(exact[4])
        assert epoch.tolist() == exact[1] and e_rounds.tolist() == exact[5]
        dev = max(dev, rel_dev(e_time, exact[4]), rel_dev(left, exact[3]))
    assert dev <= TOL, dev
    assert (np.diff(e_time) > 0).all() if same_epochs else (np.diff(e_time) >= 0).all()
    return dev, exact, got


def conserved(paths, mult, nbytes, carried):
    """carried[e] = sum of mult * bytes over the flows crossing e."""
    want = [Fraction(0)] * len(carried)
    for p, m, b in zip(paths, mult, nbytes):
        if p and m > 0:
            for e in set(p):
                want[e] += int(m) * Fraction(b)
    assert rel_dev(carried, want) <= TOL


@pytest.mark.parametrize("name", FABRICS)
def test_restatement_equals_exact_simulation_integer_bytes(name):
    c = small_case(name)
    csr, rows, verts, mult, cap = c["csr"], c["rows"], c["verts"], c["mult"], c["cap"]
    assert csr.V <= 20
    nbytes = np.random.default_rng(900 + G.SMALL.index(name)).integers(
        1, 1001, rows.shape[0]).astype(np.float64)
    exact, worst = None, 0.0
    for lay in LAYOUTS:
        if lay == EN.SLOT and np.diff(csr.row_ptr).max() > 62:
            continue
        dev, exact, got = check_case(csr, c["par"], lay, layout_tree(c, lay), rows, verts, mult,
                                     nbytes, cap, False, exact=exact)
        worst = max(worst, dev)
    assert len(got[4]) > 1 and (got[1] != -2).all()
    conserved(table_paths(csr, c["par"], rows, verts, False), mult, nbytes, got[6])
    tree = got
    dev, _, got = check_case(csr, c["nh"], EN.INT32, c["nh"], rows, verts, mult, nbytes, cap, True)
    conserved(table_paths(csr, c["nh"], rows, verts, True), mult, nbytes, got[6])
    print("fair times %s: %d / %d epochs, %d / %d rounds (trees / next-hop rows), largest "
          "relative deviation %.3g" % (name, len(tree[4]), len(got[4]), int(tree[5].sum()),
                                       int(got[5].sum()), max(worst, dev)))


@pytest.mark.parametrize("name", FABRICS)
def test_tied_byte_sizes_times_and_carried_bytes(name):
    c = small_case(name)
    csr, rows, verts, mult, cap = c["csr"], c["rows"], c["verts"], c["mult"], c["cap"]
    rng = np.random.default_rng(950 + G.SMALL.index(name))
    few = rng.choice(np.asarray([1.0, 2.0, 3.0, 8.0]), rows.shape[0])
    dev, _, got = check_case(csr, c["par"], EN.INT32, c["par"], rows, verts, mult, few, cap, False,
                             same_epochs=False)
    conserved(table_paths(csr, c["par"], rows, verts, False), mult, few, got[6])
    unit, _, got = check_case(csr, c["nh"], EN.INT32, c["nh"], rows, verts, mult,
                              np.ones(rows.shape[0]), cap, True, same_epochs=False)
    conserved(table_paths(csr, c["nh"], rows, verts, True), mult, np.ones(rows.shape[0]), got[6])
    print("fair times %s, tied sizes: largest relative deviation %.3g" % (name, max(dev, unit)))


# ------------------------------------------- relations to fair_rates --

@pytest.mark.parametrize("name", ["mock", "random_V12", "fat_tree_k4"])
def test_relations_to_fair_rates(name):
    c = small_case(name)
    csr, rows, verts, mult, cap = c["csr"], c["rows"], c["verts"], c["mult"], c["cap"]
    nbytes = np.random.default_rng(7).integers(1, 1001, rows.shape[0]).astype(np.float64)
    time, epoch, rate0, left, e_time, e_rounds, _ = EN.fair_times_host(
        csr, c["nh"], EN.INT32, rows, verts, mult, nbytes, cap, to_root=True)
    rate, _, rnd, level, _ = EN.fair_rates_host(csr, c["nh"], EN.INT32, rows, verts, mult, cap,
                                                to_root=True)
    assert np.array_equal(rate0.view(np.uint64), rate.view(np.uint64))
    assert e_rounds[0] == len(level)
    live = rnd >= 0
    assert time[live].min() == (nbytes[live] / rate[live]).min() == e_time[0]
    # (a single flow may end later than bytes / rate0: a departure can speed up
    # a flow that then takes from a third; the exchange as a whole does not)
    assert e_time[-1] <= (nbytes[live] / rate[live]).max() * (1 + TOL)
    assert time[live].max() == e_time[-1] and not left[live].any()


def test_makespan_is_below_the_step_time_of_mpi_fair_rates():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    ranks = dict(enumerate(macs))
    rng = np.random.default_rng(8)
    traffic = {(i, j): int(rng.integers(1, 5000)) for i in ranks for j in ranks
               if i != j and rng.random() < 0.4}
    for route in ROUTES:
        for hc in (None, 2.0):
            old = db.mpi_fair_rates(ranks, traffic, 10, hc, route)
            new = db.mpi_exchange_times(ranks, traffic, 10, hc, route)
            assert new.complete and new.pairs == old.pairs
            assert np.array_equal(new.rate0, old.rate) and np.array_equal(new.bytes, old.bytes)
            assert 0 < new.makespan() <= old.step_time() * (1 + TOL)
            assert new.time.min() == old.time.min()


# ------------------------------------------------------- closed forms --

def test_one_link_bytes_three_and_six():
    csr = line_csr(1)
    nh, fwd = line_to_end(csr)
    cap = np.full(csr.E, 7.0)
    cap[fwd[0]] = 3.0
    time, epoch, rate0, left, e_time, e_rounds, carried = EN.fair_times_host(
        csr, nh, EN.INT32, [0, 0], [0, 0], None, [3.0, 6.0], cap, to_root=True)
    assert time.tolist() == [2.0, 3.0] and epoch.tolist() == [0, 1]
    assert rate0.tolist() == [1.5, 1.5] and left.tolist() == [0.0, 0.0]
    assert e_time.tolist() == [2.0, 3.0] and e_rounds.tolist() == [1, 1]
    assert carried[fwd[0]] == 9.0 and carried.sum() == 9.0


def test_three_flow_line_a_departure_raises_a_survivor():
    """0 - 1 - 2 with capacities 1 and 2 (test_fair_rates): the long flow and
    the short one on the first link run at 1/2, the short one on the second
    link at 3/2.  With 1, 2 and 6 bytes the long flow leaves at t = 2; the
    flow 0 -> 1 then has the first link alone (rate 1: 1 byte more, t = 3) and
    the flow 1 -> 2 the second (rate 2: 3 bytes more, t = 3.5)."""
    csr = line_csr(2)
    em = edge_map(csr)
    cap = np.ones(csr.E)
    cap[em[(0, 1)]], cap[em[(1, 2)]] = 1.0, 2.0
    nh = np.array([[1, 2, -1], [1, -1, 1]], np.int32)
    time, epoch, rate0, left, e_time, e_rounds, carried = EN.fair_times_host(
        csr, nh, EN.INT32, [0, 1, 0], [0, 0, 1], None, [1.0, 2.0, 6.0], cap, to_root=True)
    assert rate0.tolist() == [0.5, 0.5, 1.5]
    assert time.tolist() == [2.0, 3.0, 3.5] and epoch.tolist() == [0, 1, 2]
    assert e_time.tolist() == [2.0, 3.0, 3.5] and e_rounds.tolist() == [2, 2, 1]
    assert carried[em[(0, 1)]] == 3.0 and carried[em[(1, 2)]] == 7.0
    # bytes / rate0, the old estimate, says 2, 4 and 4
    assert (np.array([1.0, 2.0, 6.0]) / rate0).tolist() == [2.0, 4.0, 4.0]


@pytest.mark.parametrize("n", [2, 19, 39])
def test_path_with_square_capacities_one_flow_per_epoch(n):
    """Line 0 .. n toward n, a flow from every vertex, cap[v -> v + 1] =
    (v + 1)^2: flow v starts at 2v + 1.  With (2v + 1) * (n - v) bytes the
    flows would all end at n - v if the rates held, so the one nearest the end
    goes first -- one flow per epoch, the last after n epochs."""
    csr = line_csr(n)
    nh, fwd = line_to_end(csr)
    cap = np.ones(csr.E)
    cap[fwd] = (np.arange(n) + 1.0) ** 2
    v = np.arange(n + 1)
    nbytes = (2.0 * v + 1) * (n - v)
    time, epoch, rate0, left, e_time, e_rounds, carried = EN.fair_times_host(
        csr, nh, EN.INT32, np.zeros(n + 1, np.int64), v, None, nbytes, cap, to_root=True)
    assert epoch[:n].tolist() == list(range(n - 1, -1, -1)) and epoch[n] == -1
    assert time[n] == 0.0 and rate0[n] == np.inf and len(e_time) == n
    assert e_rounds.tolist() == list(range(n, 0, -1))
    paths = table_paths(csr, nh, np.zeros(n + 1, np.int64), v, True)
    conserved(paths, np.ones(n + 1, np.int64), nbytes, carried)


# ------------------------------------------------------ special values --

def test_special_values_extras_and_the_epoch_cap():
    csr = line_csr(2)
    em = edge_map(csr)
    E = csr.E
    nh = np.array([[1, 2, -1]], np.int32)
    par = np.array([[0, 0, -1]], np.int32)                   # tree of 0; 2 unreached
    cap = np.concatenate([np.full(E, 10.0), [4.0, 1.0, 6.0]])
    ex = lambda *a: np.asarray(a, np.int64).reshape(-1, 2)   # noqa: E731
    # at the root without extras: done at once; with extras: the host ports limit it
    t, k, r0, left, et, er, carried = EN.fair_times_host(
        csr, nh, EN.INT32, [0, 0], [2, 2], None, [5.0, 8.0], cap, ex(-1, -1, E, E + 2),
        to_root=True)
    assert t.tolist() == [0.0, 2.0] and k.tolist() == [-1, 0] and r0.tolist() == [np.inf, 4.0]
    assert left.tolist() == [0.0, 0.0] and carried[E] == 8.0 and carried[E + 2] == 8.0
    # zero bytes never share: the other flow has the link alone; multiplicity 0,
    # unreached and out-of-range vertices are absent
    t, k, r0, left, et, er, carried = EN.fair_times_host(
        csr, par, EN.INT32, [0] * 6, [1, 1, 1, 2, 7, -1], [1, 3, 0, 1, 1, 1],
        [0.0, 5.0, 4.0, 4.0, 4.0, 0.0], cap[:E])
    assert t.tolist() == [0.0, 5.0 / (10 / 3), INF, INF, INF, INF]
    assert k.tolist() == [-1, 0, -1, -1, -1, -1] and r0.tolist() == [0.0, 10 / 3, 0.0, 0.0, 0.0, 0.0]
    assert left.tolist() == [0.0, 0.0, 4.0, 4.0, 4.0, 0.0] and carried[em[(0, 1)]] == 10.0 * t[1]
    # zero bytes at the root: as the root
    t, k, r0, _, _, _, _ = EN.fair_times_host(csr, nh, EN.INT32, [0], [2], None, [0.0], cap[:E],
                                              to_root=True)
    assert t.tolist() == [0.0] and r0.tolist() == [np.inf] and k.tolist() == [-1]
    # the epoch cap: three flows that end one by one on one link
    cap1 = np.full(E, 6.0)
    full = EN.fair_times_host(csr, nh, EN.INT32, [0] * 3, [1, 1, 1], None, [2.0, 5.0, 14.0], cap1,
                              to_root=True)
    assert full[0].tolist() == [1.0, 2.0, 3.5] and full[1].tolist() == [0, 1, 2]
    for most in (0, 1, 2, 3, 9):
        t, k, r0, left, et, er, carried = EN.fair_times_host(
            csr, nh, EN.INT32, [0] * 3, [1, 1, 1], None, [2.0, 5.0, 14.0], cap1, to_root=True,
            max_epochs=most)
        done = min(most, 3)
        assert len(et) == len(er) == done and et.tolist() == full[4][:done].tolist()
        assert k.tolist() == [0, 1, 2][:done] + [-2] * (3 - done)
        assert t[:done].tolist() == full[0][:done].tolist() and np.isinf(t[done:]).all()
        assert left.tolist() == [[2.0, 5.0, 14.0], [0.0, 3.0, 12.0], [0.0, 0.0, 9.0],
                                 [0.0, 0.0, 0.0]][done]
        assert carried[em[(1, 2)]] == [0.0, 6.0, 12.0, 21.0][done]
        assert np.array_equal(r0, full[2] if most else np.zeros(3))    # (0: no filling ran)
    # no flows at all
    out = EN.fair_times_host(csr, nh, EN.INT32, [], [], None, [], cap[:E], to_root=True)
    assert [x.size for x in out[:6]] == [0] * 6 and not out[6].any()
    # the launches of a call: one to start, two per step, sixteen steps a batch
    assert EN.fair_times_launches([]) == 33 and EN.fair_times_launches([1, 1, 1]) == 33
    assert EN.fair_times_launches([3] * 3) == 33 and EN.fair_times_launches([3] * 4) == 65


def test_rejected_arguments():
    csr = line_csr(2)
    nh = np.array([[1, 2, -1]], np.int32)
    cap = np.ones(csr.E)
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            EN.fair_times_host(csr, nh, EN.INT32, [0, 0], [0, 1], None, [1.0, bad], cap,
                               to_root=True)
    with pytest.raises(ValueError):                           # one size per flow
        EN.fair_times_host(csr, nh, EN.INT32, [0, 0], [0, 1], None, [1.0], cap, to_root=True)
    with pytest.raises(ValueError):
        EN.fair_times_host(csr, nh, EN.INT32, [0], [0], None, 1.0, cap, to_root=True,
                           max_epochs=-1)
    with pytest.raises(ValueError):                           # what fair_rates_host rejects
        EN.fair_times_host(csr, nh, EN.INT32, [0], [0], None, 1.0, 0.0 * cap, to_root=True)
    with pytest.raises(ValueError):                           # a 2-cycle is no tree
        EN.fair_times_host(csr, np.array([[1, 0, -1]], np.int32), EN.INT32, [0], [0], None, 1.0,
                           cap, to_root=True)
    one = EN.fair_times_host(csr, nh, EN.INT32, [0, 0], [0, 1], None, 2.0, cap, to_root=True)
    assert one[0].tolist() == [4.0, 4.0]                      # one number: the same for all


# ------------------------------------------------------------ drop-in --

def dropin_exact(db, pairs, weights, nbytes, capacity, host_capacity, route):
    """The exact simulation over the routes the drop-in itself returns (as
    test_fair_rates.dropin_exact builds them); also returns the links' names."""
    names, cap, paths = {}, [], []

    def idx(key, c):
        if key not in names:
            names[key] = len(cap)
            cap.append(c)
        return names[key]

    for a, b in pairs:
        fdb = route_of(db, route, a, b)
        if not fdb:
            paths.append(None)
            continue
        p = [idx(lk, capacity.get(lk, 1)) for lk in
             [(fdb[i][0], fdb[i + 1][0]) for i in range(len(fdb) - 1)]]
        if host_capacity is not None:
            p += [idx(("in", a), host_capacity), idx(("out", b), host_capacity)]
        paths.append(p)
    return exact_times(paths, weights, nbytes, cap), names


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("host_capacity", [None, 1.5])
def test_dropin_equals_exact_simulation_over_its_routes(route, host_capacity):
    from test_widest_tables import seed_utilisation
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    csr = db.graph().csr
    rng = np.random.default_rng(22)
    links = [(int(csr.dpids[u]), int(csr.dpids[v])) for u, v in
             zip(np.repeat(np.arange(csr.V), np.diff(csr.row_ptr)).tolist(),
                 np.asarray(csr.col).tolist())]
    for lk in links:
        db.set_link_cost(lk[0], lk[1], int(rng.integers(1, 4)))
    seed_utilisation(db, 3, 23)
    pairs, w = dropin_pairs(fabric)
    capacity = {lk: int(c) for lk, c in zip(links, rng.choice(CAPS, len(links)))}
    nbytes = rng.integers(0, 1001, len(pairs)).astype(np.float64)
    got = db.fair_completion_times(pairs, nbytes, w, capacity, host_capacity, route)
    assert isinstance(got, FlowTimes) and isinstance(got.link_bytes, SplitLinkLoads)
    exact, names = dropin_exact(db, pairs, w, nbytes, capacity, host_capacity, route)
    assert got.routed.tolist() == [bool(route_of(db, route, a, b)) for a, b in pairs]
    assert not got.routed[-2:].any() and got.complete
    assert got.epoch.tolist() == exact[1] and got.epochs == len(exact[4])
    assert got.epoch_rounds.tolist() == exact[5]
    dev = max(rel_dev(got.time, exact[0]), rel_dev(got.epoch_time, exact[4]))
    assert dev <= TOL, dev
    lb = got.link_bytes
    ld = dict(zip(zip(lb.src_dpid.tolist(), lb.dst_dpid.tolist()), lb.load.tolist()))
    want = {k: v for k, v in names.items() if not (isinstance(k[0], str))}
    assert rel_dev([ld.get(k, 0.0) for k in want], [exact[6][v] for v in want.values()]) <= TOL
    live = got.routed & (np.asarray(w) > 0)
    lost = ~got.routed & (nbytes > 0) & (np.asarray(w) > 0)   # bytes for an unknown host
    assert got.makespan() == (INF if lost.any() else got.epoch_time[-1])
    assert got.time[live].max() == got.epoch_time[-1] and not got.remaining[live].any()
    rates = db.fair_rates(pairs, np.where(nbytes > 0, w, 0).tolist(), capacity, host_capacity,
                          route)
    assert np.array_equal(got.rate0[nbytes > 0], rates.rate[nbytes > 0])
    if host_capacity is not None:
        assert sum(got.link_bytes.host_load) > 0
    # the cap: what ran is the same, the rest is still sending
    part = db.fair_completion_times(pairs, nbytes, w, capacity, host_capacity, route,
                                    max_epochs=3)
    assert not part.complete and part.epochs == 3
    assert np.array_equal(part.epoch_time, got.epoch_time[:3])
    late = got.epoch >= 3
    assert (part.epoch[late] == -2).all() and np.array_equal(part.epoch[~late], got.epoch[~late])
    assert np.isinf(part.time[late]).all() and (part.remaining[late] > 0).all()
    print("fair times drop-in %s: largest relative deviation %.3g" % (route, dev))


def test_pairs_merge_only_with_equal_bytes():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    a, b, c, d = macs[0], macs[1], macs[4], macs[5]          # a, b and c, d share a switch
    db.fair_completion_times([(a, c), (b, d), (a, d)], [5.0, 5.0, 5.0])
    assert db._engine.calls[-1][0] == "times" and db._engine.calls[-1][2] == 1
    got = db.fair_completion_times([(a, c), (b, d), (a, d)], [5.0, 7.0, 5.0])
    assert db._engine.calls[-1][2] == 2
    assert got.time[0] == got.time[2] < got.time[1] and got.epochs == 2


def test_all_pairs_form_equals_the_mac_pair_form():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    allp = [(a, b) for a in macs for b in macs if a != b]
    sw = {m: db.hosts[m].port.dpid for m in macs}
    for route in ROUTES:
        ap = db.all_pairs_fair_completion_times(3.0, route=route)
        mp = db.fair_completion_times(allp, 3.0, route=route)
        assert np.array_equal(ap.epoch_time, mp.epoch_time)
        assert np.array_equal(ap.epoch_rounds, mp.epoch_rounds)
        assert np.array_equal(ap.link_bytes.load, mp.link_bytes.load)
        assert ap.makespan() == mp.makespan() > 0 and ap.complete
        assert int(ap.weights.sum()) == len(allp)
        by = dict(zip(ap.pairs, ap.time.tolist()))
        assert [by[(sw[a], sw[b])] for a, b in allp] == mp.time.tolist()


def test_mpi_exchange_times():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    ranks = {r: macs[r] for r in range(8)}
    traffic = {(0, 5): 1000, (1, 5): 3000, (2, 6): 0, (3, 9): 50, (0, 4): 10}    # rank 9 unknown
    got = db.mpi_exchange_times(ranks, traffic, capacity=100, host_capacity=2.0)
    assert got.pairs == [(macs[0], macs[5]), (macs[1], macs[5]), (macs[2], macs[6]),
                         (macs[0], macs[4])]
    assert got.bytes.tolist() == [1000.0, 3000.0, 0.0, 10.0]
    # the port out to host 5 is shared by two flows, the port in from host 0 too
    assert got.rate0.tolist() == [1.0, 1.0, 0.0, 1.0]
    # 0 -> 4 is done at 10; 0 -> 5 still shares host 5's port and is done at 1000;
    # 1 -> 5 then has it alone: the 2000 bytes left go at 2.0
    assert got.time.tolist() == [1000.0, 2000.0, 0.0, 10.0] and got.makespan() == 2000.0
    old = db.mpi_fair_rates(ranks, traffic, capacity=100, host_capacity=2.0)
    assert old.step_time() == 3000.0
    every = db.mpi_exchange_times(ranks)
    assert len(every.pairs) == 56 and every.complete and every.makespan() > 0


def test_link_events_equal_a_fresh_database():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    pairs, w = dropin_pairs(fabric)
    nbytes = np.random.default_rng(5).integers(1, 100, len(pairs)).astype(np.float64)
    before = db.fair_completion_times(pairs, nbytes, w, host_capacity=2.0)
    t = db.route_tables("dfs")
    a = int(t["dpids"][t["parent"][0][0]])
    ab, ba = db.links[a][1], db.links[1][a]
    db.delete_link(ab)
    db.delete_link(ba)
    cut = db.fair_completion_times(pairs, nbytes, w, host_capacity=2.0)
    fresh = fake_db(fabric)
    fresh.delete_link(fresh.links[a][1])
    fresh.delete_link(fresh.links[1][a])
    other = fresh.fair_completion_times(pairs, nbytes, w, host_capacity=2.0)
    assert np.array_equal(cut.time, other.time) and np.array_equal(cut.epoch, other.epoch)
    assert np.array_equal(cut.link_bytes.load, other.link_bytes.load)
    db.add_link(ab)
    db.add_link(ba)
    again = db.fair_completion_times(pairs, nbytes, w, host_capacity=2.0)
    assert np.array_equal(again.time, before.time)
    assert np.array_equal(again.link_bytes.load, before.link_bytes.load)


def test_bad_arguments_and_the_multipath_refusal():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    p = [(macs[0], macs[5])]
    empty = db.fair_completion_times([], [])
    assert empty.time.size == 0 and empty.epochs == 0 and empty.makespan() == 0.0
    assert empty.complete
    for route in ("ecmp", "least_cost_ecmp"):
        with pytest.raises(ValueError) as ei:
            db.fair_completion_times(p, 1.0, route=route)
        assert all(repr(r) in str(ei.value) for r in ROUTES)
    for kw in (dict(nbytes=-1.0), dict(nbytes=float("nan")), dict(nbytes=float("inf")),
               dict(nbytes=[1.0, 2.0]), dict(nbytes=1.0, weights=[-1]),
               dict(nbytes=1.0, capacity=0), dict(nbytes=1.0, host_capacity=0),
               dict(nbytes=1.0, max_epochs=-1), dict(nbytes=1.0, route="widest")):
        with pytest.raises(ValueError):
            db.fair_completion_times(p, **kw)
    with pytest.raises(ValueError):
        db.all_pairs_fair_completion_times(float("nan"))
    with pytest.raises(ValueError):
        db.all_pairs_fair_completion_times([1.0, 2.0])
    with pytest.raises(ValueError):
        db.mpi_exchange_times({0: macs[0], 1: macs[1]}, {(0, 1): -5})
