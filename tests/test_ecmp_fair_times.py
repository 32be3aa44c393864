"""Max-min fair completion times over ECMP (engine.ecmp_fair_times_host,
TopologyDB.fair_completion_times and friends with route="ecmp" /
"least_cost_ecmp"), CPU only: the numpy restatement of ecmp_fair_times.hip
against an event simulation in exact fractions -- textbook progressive filling
over explicit per-flow link fractions (test_ecmp_fair_rates.exact_ecmp_fair),
advance to the first departure, drop the finished flows, again --, closed
forms, conservation of bytes, the relations to ecmp_fair_rates and fair_times,
and the drop-in over an engine double built from the restatements.

The simulation ties exactly; the restatement ties within kFairTie = 2**-30,
in the filling and in the advance.  Every simulated case is held to a guard,
checked on the simulation alone: in every epoch every flow's exact q / dt - 1
and every link's exact share / level - 1 is 0 or above GUARD = 2**-20, 1,024
times the tolerance, so neither rounding nor the tolerance can move a decision.
Under the guard the epoch count, every flow's epoch and every filling's round
count must equal the simulation; times, epoch times, bytes left and carried
bytes agree within TOL (16 times the largest relative deviation
measured over the seeded cases of this file, capped at 1e-9)."""
from fractions import Fraction

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import FlowTimes, SplitLinkLoads
from test_cost_ecmp_loads import (both_ways, diamond_csr, digraph_csr, path_csr_costs, pcost_rows)
from test_ecmp_fair_rates import (ECMP_ROUTES, SPLITS, FakeEcmpFairEngine, exact_ecmp_fair,
                                  flow_fractions, route_set_fractions, routes_of, seed_costs,
                                  small_case, unit_or)
from test_ecmp_link_loads import edge_map
from test_fair_rates import CAPS, ROUTES, dropin_pairs, fake_db, line_csr
from test_fair_times import FABRICS, FakeTimesEngine, rel_dev

# largest relative deviation of a time, an epoch time, a flow's bytes left or a
# link's carried bytes measured over the seeded cases below (the fabrics, both
# splits, unit and seeded costs, and the drop-in cases; the tests print it per
# case): 2.46e-15 (fat_tree_k4_loops, seeded costs, hop split, 297 epochs and
# 5,408 rounds); 16 times that, far below the 1e-9 cap
MEASURED_DEV = 2.46e-15
TOL = min(16 * MEASURED_DEV, 1e-9)
GUARD = Fraction(1, 1 << 20)
INF = float("inf")

# the seed of every fabric's byte sizes: 900 + its index in G.SMALL, plus 100
# until the simulation of all four of its cases (splits x costs) passes the guard
# (none needed that: the smallest margin met is 1.35e-5, fat_tree_k4_loops)
BYTES_SEED = {name: 900 + G.SMALL.index(name) for name in FABRICS}
# the seed of the drop-in cases' byte sizes: 22, plus 100 until all eight pass
# the guard (22 does)
DROPIN_SEED = 22


class FakeEcmpTimesEngine(FakeEcmpFairEngine, FakeTimesEngine):
    """The restatement double plus ecmp_fair_times."""

    def ecmp_fair_times(self, export, cost, pcost, rows, srcs, mult=None, nbytes=1.0, cap=None,
                        extra=None, split="route", max_epochs=None, timing=False):
        self.calls.append(("ecmp_times", export.key, len(rows)))
        if cap is None:
            cap = np.ones(int(export.csr.E))
        return EN.ecmp_fair_times_host(export.csr, cost, pcost, rows, srcs, mult, nbytes, cap,
                                       extra, split, max_epochs)


def times_db(fabric, **kw):
    db = fake_db(fabric, **kw)
    db._engine = FakeEcmpTimesEngine()
    return db


# ------------------------------------------------ the exact reference --

def fill_margin(fracs, extras, mult, cap, rnd, levels):
    """The smallest nonzero share / level - 1 over the rounds of one exact
    filling (exact_ecmp_fair's result): what the guard bounds from below."""
    m = len(cap)
    a = [Fraction(0)] * m
    frozen = [Fraction(0)] * m
    by_round = [[] for _ in levels]
    share_of = {}
    for i, k in enumerate(rnd):
        if k < 0:
            continue
        sh = dict(fracs[i])
        for x in extras[i]:
            sh[x] = Fraction(1)
        share_of[i] = sh
        by_round[k].append(i)
        for e, f in sh.items():
            a[e] += int(mult[i]) * f
    worst = None
    for k, r in enumerate(levels):
        for e in range(m):
            if a[e] > 0:
                s = (Fraction(cap[e]) - frozen[e]) / a[e]
                assert s >= r
                if s != r and (worst is None or s / r - 1 < worst):
                    worst = s / r - 1
        for i in by_round[k]:
            for e, f in share_of[i].items():
                w = int(mult[i]) * f
                a[e] -= w
                frozen[e] += r * w
    return worst


def exact_ecmp_times(fracs, extras, mult, nbytes, cap, max_epochs=None):
    """The event simulation in exact fractions: fill (exact_ecmp_fair), advance
    to the first departure, drop the flows that are done, again.  Returns
    (time -- Fractions, inf for a flow that never ends --, epoch, rate0, left,
    epoch_time, epoch_rounds, carried, margin): margin is the smallest nonzero
    q / dt - 1 and share / level - 1 met (None: every comparison was a tie)."""
    n = len(fracs)
    m = np.asarray(mult, np.int64).copy()
    left = [Fraction(b) for b in nbytes]
    time, epoch = [INF] * n, [-1] * n
    bare = [f is not None and not f and not x for f, x in zip(fracs, extras)]
    for i in range(n):
        if fracs[i] is not None and m[i] > 0 and (bare[i] or left[i] == 0):
            time[i] = Fraction(0)
            if bare[i]:
                left[i] = Fraction(0)
    rate0 = exact_ecmp_fair(fracs, extras, np.where([b == 0 for b in left], 0, m), cap)[0]
    for i in range(n):
        if fracs[i] is not None and m[i] > 0 and bare[i]:
            rate0[i] = INF
    m[[i for i in range(n) if left[i] == 0]] = 0
    carried = [Fraction(0)] * len(cap)
    t = Fraction(0)
    e_time, e_rounds = [], []
    margin = None
    j = 0
    while True:
        rate, _, rnd, levels, used = exact_ecmp_fair(fracs, extras, m, cap)
        fl = [i for i in range(n) if rnd[i] >= 0]
        if not fl:
            break
        if max_epochs is not None and j == max_epochs:
            for i in fl:
                epoch[i] = -2
            break
        g = fill_margin(fracs, extras, m, cap, rnd, levels)
        if g is not None and (margin is None or g < margin):
            margin = g
        q = [left[i] / rate[i] for i in fl]
        dt = min(q)
        for x in q:
            if x != dt and (margin is None or x / dt - 1 < margin):
                margin = x / dt - 1
        t += dt
        carried = [c + u * dt for c, u in zip(carried, used)]
        for i in fl:
            left[i] -= rate[i] * dt
            if left[i] == 0:
                time[i], epoch[i], m[i] = t, j, 0
        e_time.append(t)
        e_rounds.append(len(levels))
        j += 1
    return time, epoch, rate0, left, e_time, e_rounds, carried, margin


def extras_of(n, extra):
    return [[] for _ in range(n)] if extra is None else \
        [list(dict.fromkeys(int(x) for x in row if x >= 0)) for row in np.asarray(extra)]


def compare(got, exact):
    """One result 7-tuple against the simulation under the guard; returns the
    largest relative deviation."""
    time, epoch, rate0, left, e_time, e_rounds, carried = got
    assert exact[7] is None or exact[7] > GUARD, "the simulation fails the guard: %r" % exact[7]
    assert time.dtype == np.float64 and epoch.dtype == np.int32 and e_rounds.dtype == np.int32
    assert len(e_time) == len(exact[4])
    assert epoch.tolist() == exact[1] and e_rounds.tolist() == exact[5]
    dev = max(rel_dev(time, exact[0]), rel_dev(carried, exact[6]), rel_dev(e_time, exact[4]),
              rel_dev(left, exact[3]))
    assert dev <= TOL, dev
    assert (np.diff(e_time) > 0).all()
    return dev


def check_case(csr, cost, pcost, rows, srcs, mult, nbytes, cap, split, extra=None, fracs=None,
               max_epochs=None):
    """ecmp_fair_times_host of one case against the exact simulation; returns
    the largest relative deviation, the simulation and the result."""
    n = len(rows)
    if fracs is None:
        fracs = flow_fractions(csr, unit_or(cost, csr), pcost, rows, srcs, split)
    m = np.ones(n, np.int64) if mult is None else np.asarray(mult).astype(np.int64)
    exact = exact_ecmp_times(fracs, extras_of(n, extra), m, nbytes, cap, max_epochs)
    got = EN.ecmp_fair_times_host(csr, cost, pcost, rows, srcs, mult, nbytes, cap, extra, split,
                                  max_epochs)
    return compare(got, exact), exact, got


def conserved(fracs, extras, mult, nbytes, carried):
    """carried[e] against sum of mult * bytes * phi(e): a flow that left within
    the tolerance sent at least rem_b / (1 + 2**-30), so carried may fall short
    by 2**-30 relative and exceeds the sum only by rounding."""
    want = [Fraction(0)] * len(carried)
    for f, x, m, b in zip(fracs, extras, mult, nbytes):
        if f is not None and m > 0:
            for e, p in list(f.items()) + [(e, 1) for e in x]:
                want[e] += int(m) * Fraction(b) * p
    for c, w in zip(np.asarray(carried).tolist(), want):
        w = float(w)
        assert (1 - 2.0 ** -30) * w - TOL * w <= c <= w * (1 + TOL)


def case_bytes(name, n):
    return np.random.default_rng(BYTES_SEED[name]).integers(1, 1001, n).astype(np.float64)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("costs", ["unit", "seeded"])
@pytest.mark.parametrize("name", FABRICS)
def test_restatement_equals_exact_simulation(name, costs, split):
    c = small_case(name)
    csr, rows, srcs, mult, cap = c["csr"], c["rows"], c["srcs"], c["mult"], c["cap"]
    assert csr.V <= 20
    cost, pc = (None, c["pc_unit"]) if costs == "unit" else (c["cost"], c["pc_cost"])
    nbytes = case_bytes(name, rows.shape[0])
    fracs = flow_fractions(csr, unit_or(cost, csr), pc, rows, srcs, split)
    dev, exact, got = check_case(csr, cost, pc, rows, srcs, mult, nbytes, cap, split, fracs=fracs)
    assert len(got[4]) > 1 and (got[1] != -2).all()
    conserved(fracs, extras_of(len(rows), None), mult, nbytes, got[6])
    rate = EN.ecmp_fair_rates_host(csr, cost, pc, rows, srcs, mult, cap, None, split)
    assert np.array_equal(got[2].view(np.uint64), rate[0].view(np.uint64))
    assert got[5][0] == len(rate[3])
    print("ecmp fair times %s, %s costs, %s split: %d epochs, %d rounds, margin %.3g, largest "
          "relative deviation %.3g" % (name, costs, split, len(got[4]), int(got[5].sum()),
                                       float(exact[7]), dev))


# ------------------------------------------------------ the tolerance --

def star_49():
    """0 -> 2 and 1 -> 2 with unit links; flow A from 0 counts 49 times and
    sends 1 byte, flow B from 1 sends 49 bytes.  Both end at t = 49 as
    fractions; in float64 1 / (1 / 49) = 49.00000000000001 and 1 - (1 / 49) *
    49 = 1.1e-16."""
    csr = digraph_csr(both_ways([(0, 2), (1, 2)]))
    pc = pcost_rows(csr, np.ones(int(csr.E), np.uint32), [2])
    return csr, pc, [0, 0], [0, 1], [49, 1], [1.0, 49.0], np.ones(int(csr.E))


def test_the_advance_shares_the_tie_tolerance():
    csr, pc, rows, srcs, mult, nbytes, cap = star_49()
    assert 1.0 / (1.0 / 49.0) > 49.0 and 1.0 - (1.0 / 49.0) * 49.0 > 0.0
    nh = np.array([[2, 2, -1]], np.int32)
    one = EN.fair_times_host(csr, nh, EN.INT32, rows, srcs, mult, nbytes, cap, to_root=True)
    assert len(one[4]) == 2 and one[1].tolist() == [1, 0]     # an ulp apart: two epochs
    for split in SPLITS:
        t, k, r0, left, et, er, carried = EN.ecmp_fair_times_host(csr, None, pc, rows, srcs, mult,
                                                                  nbytes, cap, split=split)
        assert t.tolist() == [49.0, 49.0] and k.tolist() == [0, 0]
        assert et.tolist() == [49.0] and er.tolist() == [2] and left.tolist() == [0.0, 0.0]
        assert r0.tolist() == [1.0 / 49.0, 1.0]
        em = edge_map(csr)
        # ((1 / 49) * 49 rounds below 1: the 49 flows' link carried 49 within rounding)
        assert carried[em[(0, 2)]] == pytest.approx(49.0, rel=TOL) and carried[em[(1, 2)]] == 49.0


# ------------------------------------------------------- closed forms --

def test_diamond_a_departure_raises_the_survivor():
    """The diamond s -> m -> d / s -> d with s -> m thin (capacity 1): a pair
    s -> d puts half its rate there and runs at 2; a flow m -> d shares m -> d
    (capacity 10) with that half.  Round 0 freezes the pair at 2 (s -> m),
    round 1 the flow at 10 - 1 = 9.  With 4 bytes for the pair and 36 for the
    flow the pair leaves at t = 2; the flow has sent 18 and then has m -> d
    alone: 18 more at 10, t = 3.8.  bytes / rate0 says 4."""
    csr, cost, (s, m, d) = diamond_csr()
    em = edge_map(csr)
    E = int(csr.E)
    pc = pcost_rows(csr, cost, [d])
    cap = np.full(E, 10.0)
    cap[em[(s, m)]] = 1.0
    for split in SPLITS:
        t, k, r0, left, et, er, carried = EN.ecmp_fair_times_host(
            csr, cost, pc, [0, 0], [s, m], None, [4.0, 36.0], cap, split=split)
        assert r0.tolist() == [2.0, 9.0] and k.tolist() == [0, 1]
        assert t.tolist() == [2.0, 3.8] and et.tolist() == [2.0, 3.8] and er.tolist() == [2, 1]
        assert carried[em[(s, m)]] == 2.0 and carried[em[(s, d)]] == 2.0
        assert carried[em[(m, d)]] == 38.0 and not left.any()
        assert (np.array([4.0, 36.0]) / r0).tolist() == [2.0, 4.0]
        check_case(csr, cost, pc, [0, 0], [s, m], [3, 2], [4.0, 37.0], cap, split)


def test_three_flow_line_through_single_route_rows():
    """test_fair_times' line 0 - 1 - 2 with capacities 1 and 2: 3.5, where
    bytes / rate0 says 4."""
    csr = line_csr(2)
    em = edge_map(csr)
    cap = np.ones(csr.E)
    cap[em[(0, 1)]], cap[em[(1, 2)]] = 1.0, 2.0
    pc = pcost_rows(csr, np.ones(int(csr.E), np.uint32), [2, 1])
    for split in SPLITS:
        t, k, r0, left, et, er, carried = EN.ecmp_fair_times_host(
            csr, None, pc, [0, 1, 0], [0, 0, 1], None, [1.0, 2.0, 6.0], cap, split=split)
        assert r0.tolist() == [0.5, 0.5, 1.5]
        assert t.tolist() == [2.0, 3.0, 3.5] and k.tolist() == [0, 1, 2]
        assert et.tolist() == [2.0, 3.0, 3.5] and er.tolist() == [2, 2, 1]
        assert carried[em[(0, 1)]] == 3.0 and carried[em[(1, 2)]] == 7.0


def test_single_route_flows_equal_the_single_path_times_on_the_bits():
    for csr, cost in (path_csr_costs(9),
                      (digraph_csr(both_ways([(0, 1), (1, 2), (1, 3), (3, 4), (3, 5), (0, 6)])),
                       None)):
        V, E = int(csr.V), int(csr.E)
        pc, nh, _ = EN.cost_tables_host(csr, unit_or(cost, csr), np.arange(V))
        rows, srcs = np.repeat(np.arange(V), V), np.tile(np.arange(V), V)
        rng = np.random.default_rng(5)
        mult = rng.integers(0, 6, V * V).astype(np.uint64)
        cap = rng.choice(np.asarray(CAPS, np.float64), E)
        nbytes = rng.integers(1, 1001, V * V).astype(np.float64)
        want = EN.fair_times_host(csr, nh, EN.INT32, rows, srcs, mult, nbytes, cap, to_root=True)
        # no near-tie: the tolerance decides nothing that the exact rule does not
        fracs = flow_fractions(csr, unit_or(cost, csr), pc, rows, srcs, "route")
        exact = exact_ecmp_times(fracs, extras_of(V * V, None), mult.astype(np.int64), nbytes, cap)
        assert exact[7] > GUARD and len(want[4]) > 3
        for split in SPLITS:
            got = EN.ecmp_fair_times_host(csr, cost, pc, rows, srcs, mult, nbytes, cap,
                                          split=split)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
            compare(got, exact)


# ------------------------------------------- relations and special values --

def test_makespan_is_below_the_step_time_of_mpi_fair_rates():
    fabric = T.fat_tree(4)
    db = times_db(fabric)
    capacity = seed_costs(db)
    macs = fabric.host_macs()
    ranks = dict(enumerate(macs))
    rng = np.random.default_rng(8)
    traffic = {(i, j): int(rng.integers(1, 5000)) for i in ranks for j in ranks
               if i != j and rng.random() < 0.4}
    for route in ECMP_ROUTES:
        for split in SPLITS:
            for hc in (None, 2.0):
                old = db.mpi_fair_rates(ranks, traffic, capacity, hc, route, split)
                new = db.mpi_exchange_times(ranks, traffic, capacity, hc, route, split=split)
                assert new.complete and new.pairs == old.pairs and new.split == split
                # (the two calls merge the pairs into different flows: the float sums differ)
                assert np.allclose(new.rate0, old.rate, rtol=TOL, atol=0)
                assert np.array_equal(new.bytes, old.bytes)
                assert 0 < new.makespan() <= old.step_time() * (1 + 2.0 ** -29)
                assert new.time.min() == pytest.approx(old.time.min(), rel=2.0 ** -29)


def test_special_values_extras_and_the_epoch_cap():
    csr, cost, (s, m, d) = diamond_csr()
    E = int(csr.E)
    em = edge_map(csr)
    # row 0 toward d; row 1 toward an isolated destination: nothing reaches it
    pc = np.vstack([pcost_rows(csr, cost, [d]), np.full((1, 3), EN.COST_INF, np.uint32)])
    pc[1, m] = 0
    cap = np.concatenate([np.full(E, 10.0), [1.0, 4.0]])
    extra = [[-1, -1], [E, -1], [-1, -1], [-1, -1], [-1, -1], [E, E + 1], [E + 1, E + 1],
             [-1, -1], [-1, -1]]
    rows = [0, 0, 1, 0, 0, 0, 1, 0, 0]
    srcs = [d, d, s, 7, -1, s, m, m, d]
    mult = [1, 1, 1, 1, 1, 0, 2, 1, 1]
    nbytes = [5.0, 3.0, 2.0, 2.0, 2.0, 2.0, 8.0, 0.0, 0.0]
    t, k, r0, left, et, er, carried = EN.ecmp_fair_times_host(csr, cost, pc, rows, srcs, mult,
                                                              nbytes, cap, extra)
    # s == d without an extra; s == d bound by its extra (host ports: s == d with
    # extras shares); unreachable; out of range twice; multiplicity 0; s == d with
    # the same extra named twice; zero bytes routed; zero bytes at the destination
    assert t.tolist() == [0.0, 3.0, INF, INF, INF, INF, 4.0, 0.0, 0.0]
    assert k.tolist() == [-1, 0, -1, -1, -1, -1, 1, -1, -1]
    assert r0.tolist() == [INF, 1.0, 0.0, 0.0, 0.0, 0.0, 2.0, 0.0, INF]
    assert left.tolist() == [0.0, 0.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0]
    assert et.tolist() == [3.0, 4.0] and er.tolist() == [2, 1]
    assert carried[E:].tolist() == [3.0, 16.0] and not carried[:E].any()
    # the epoch cap: three flows that end one by one on the direct link s -> d ...
    # through the pair's two routes: s -> d carries half of each
    cap1 = np.full(E, 3.0)
    args = (csr, cost, pc, [0] * 3, [s] * 3, None, [2.0, 5.0, 14.0], cap1)
    full = EN.ecmp_fair_times_host(*args)
    assert full[0].tolist() == [1.0, 2.0, 3.5] and full[1].tolist() == [0, 1, 2]
    for most in (0, 1, 2, 3, 9):
        t, k, r0, left, et, er, carried = EN.ecmp_fair_times_host(*args, max_epochs=most)
        done = min(most, 3)
        assert len(et) == len(er) == done and et.tolist() == full[4][:done].tolist()
        assert k.tolist() == [0, 1, 2][:done] + [-2] * (3 - done)
        assert t[:done].tolist() == full[0][:done].tolist() and np.isinf(t[done:]).all()
        assert left.tolist() == [[2.0, 5.0, 14.0], [0.0, 3.0, 12.0], [0.0, 0.0, 9.0],
                                 [0.0, 0.0, 0.0]][done]
        assert carried[em[(s, d)]] == [0.0, 3.0, 6.0, 10.5][done]
        assert np.array_equal(r0, full[2] if most else np.zeros(3))    # (0: no filling ran)
    # no flows at all
    out = EN.ecmp_fair_times_host(csr, cost, pc, [], [], None, [], np.ones(E))
    assert [x.size for x in out[:6]] == [0] * 6 and not out[6].any()


def test_rejected_arguments():
    csr, cost, (s, m, d) = diamond_csr()
    E = int(csr.E)
    pc = pcost_rows(csr, cost, [d])
    cap = np.ones(E)
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            EN.ecmp_fair_times_host(csr, cost, pc, [0, 0], [s, m], None, [1.0, bad], cap)
    with pytest.raises(ValueError):                           # one size per flow
        EN.ecmp_fair_times_host(csr, cost, pc, [0, 0], [s, m], None, [1.0], cap)
    with pytest.raises(ValueError):
        EN.ecmp_fair_times_host(csr, cost, pc, [0], [s], None, 1.0, cap, max_epochs=-1)
    with pytest.raises(ValueError, match="split"):
        EN.ecmp_fair_times_host(csr, cost, pc, [0], [s], None, 1.0, cap, split="flow")
    with pytest.raises(ValueError, match="split"):
        EN.ecmp_fair_times_host(csr, cost, pc, [], [], None, [], cap, split="flow")
    with pytest.raises(ValueError):                           # what ecmp_fair_rates_host rejects
        EN.ecmp_fair_times_host(csr, cost, pc, [0], [s], None, 1.0, 0.0 * cap)
    with pytest.raises(ValueError):
        EN.ecmp_fair_times_host(csr, cost, pc, [1], [s], None, 1.0, cap)          # no such row
    bad = pc.copy()
    bad[0, m] = 7                                             # no link explains that cost
    with pytest.raises(ValueError, match="labelling"):
        EN.ecmp_fair_times_host(csr, cost, bad, [0], [s], None, 1.0, cap)
    one = EN.ecmp_fair_times_host(csr, cost, pc, [0, 0], [s, m], None, 2.0, cap)
    assert one[0].tolist() == [3.0, 3.0]                      # one number: the same for all


# ------------------------------------------------------------ drop-in --

def dropin_exact(db, pairs, weights, nbytes, capacity, host_capacity, route, split):
    """The exact simulation over the route sets the drop-in itself returns
    (as test_ecmp_fair_rates.dropin_exact builds them); also returns the
    links' numbers by name."""
    csr = db.graph().csr
    dp = [int(x) for x in csr.dpids]
    links = list(zip(np.repeat(np.arange(csr.V), np.diff(csr.row_ptr)).tolist(),
                     np.asarray(csr.col).tolist()))
    edge = {(dp[u], dp[v]): e for e, (u, v) in enumerate(links)}
    cap = [capacity.get((dp[u], dp[v]), 1) for u, v in links]
    names = {}
    fracs, extras = [], []
    for a, b in pairs:
        fdbs = routes_of(db, route, a, b)
        if not fdbs:
            fracs.append(None)
            extras.append([])
            continue
        fracs.append(route_set_fractions([tuple(x[0] for x in f) for f in fdbs], edge, split))
        ex = []
        if host_capacity is not None:
            for key in (("in", a), ("out", b)):
                if key not in names:
                    names[key] = len(cap)
                    cap.append(host_capacity)
                ex.append(names[key])
        extras.append(ex)
    return exact_ecmp_times(fracs, extras, weights, nbytes, cap), edge


@pytest.mark.parametrize("route", ECMP_ROUTES)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("host_capacity", [None, 1.5])
def test_dropin_equals_exact_simulation_over_its_route_sets(route, split, host_capacity):
    fabric = T.fat_tree(4)
    db = times_db(fabric)
    capacity = seed_costs(db)
    pairs, w = dropin_pairs(fabric)
    nbytes = np.random.default_rng(DROPIN_SEED).integers(0, 1001, len(pairs)).astype(np.float64)
    got = db.fair_completion_times(pairs, nbytes, w, capacity, host_capacity, route, split=split)
    assert isinstance(got, FlowTimes) and isinstance(got.link_bytes, SplitLinkLoads)
    assert got.split == split
    exact, edge = dropin_exact(db, pairs, w, nbytes, capacity, host_capacity, route, split)
    assert exact[7] is None or exact[7] > GUARD, "the simulation fails the guard: %r" % exact[7]
    assert got.routed.tolist() == [bool(routes_of(db, route, a, b)) for a, b in pairs]
    assert any(len(routes_of(db, route, a, b)) > 1 for a, b in pairs)
    assert not got.routed[-2:].any() and got.complete
    assert got.epoch.tolist() == exact[1] and got.epochs == len(exact[4])
    assert got.epoch_rounds.tolist() == exact[5]
    dev = max(rel_dev(got.time, exact[0]), rel_dev(got.epoch_time, exact[4]))
    lb = got.link_bytes
    ld = dict(zip(zip(lb.src_dpid.tolist(), lb.dst_dpid.tolist()), lb.load.tolist()))
    dev = max(dev, rel_dev([ld.get(k, 0.0) for k in edge], [exact[6][v] for v in edge.values()]))
    assert dev <= TOL, dev
    live = got.routed & (np.asarray(w) > 0)
    lost = ~got.routed & (nbytes > 0) & (np.asarray(w) > 0)   # bytes for an unknown host
    assert got.makespan() == (INF if lost.any() else got.epoch_time[-1])
    assert got.time[live].max() == got.epoch_time[-1] and not got.remaining[live].any()
    rates = db.fair_rates(pairs, np.where(nbytes > 0, w, 0).tolist(), capacity, host_capacity,
                          route, split)
    # (the two calls merge the pairs into different flows: the float sums differ)
    assert np.allclose(got.rate0[nbytes > 0], rates.rate[nbytes > 0], rtol=TOL, atol=0)
    if host_capacity is not None:
        assert sum(got.link_bytes.host_load) > 0
    # the cap: what ran is the same, the rest is still sending
    part = db.fair_completion_times(pairs, nbytes, w, capacity, host_capacity, route, 3, split)
    assert not part.complete and part.epochs == 3
    assert np.array_equal(part.epoch_time, got.epoch_time[:3])
    late = got.epoch >= 3
    assert (part.epoch[late] == -2).all() and np.array_equal(part.epoch[~late], got.epoch[~late])
    assert np.isinf(part.time[late]).all() and (part.remaining[late] > 0).all()
    print("ecmp fair times drop-in %s, %s split: %d epochs, largest relative deviation %.3g"
          % (route, split, got.epochs, dev))


def test_all_pairs_form_equals_the_mac_pair_form():
    fabric = T.fat_tree(4)
    db = times_db(fabric)
    macs = fabric.host_macs()
    allp = [(a, b) for a in macs for b in macs if a != b]
    sw = {m: db.hosts[m].port.dpid for m in macs}
    for route in ECMP_ROUTES:
        for split in SPLITS:
            ap = db.all_pairs_fair_completion_times(3.0, route=route, split=split)
            mp = db.fair_completion_times(allp, 3.0, route=route, split=split)
            assert np.array_equal(ap.epoch_time, mp.epoch_time)
            assert np.array_equal(ap.epoch_rounds, mp.epoch_rounds)
            assert np.array_equal(ap.link_bytes.load, mp.link_bytes.load)
            assert ap.makespan() == mp.makespan() > 0 and ap.complete
            assert int(ap.weights.sum()) == len(allp)
            by = dict(zip(ap.pairs, ap.time.tolist()))
            assert [by[(sw[a], sw[b])] for a, b in allp] == mp.time.tolist()
    # equal blocks all-to-all over ECMP on a fat-tree with unit capacities: one
    # level, one epoch, and the step time of the rates
    assert ap.epochs == 1 and ap.epoch_rounds.tolist() == [1]
    assert ap.makespan() == 3.0 / db.all_pairs_fair_rates(route=route, split=split).min_rate


def test_mpi_exchange_times():
    fabric = T.fat_tree(4)
    db = times_db(fabric)
    macs = fabric.host_macs()
    ranks = {r: macs[r] for r in range(8)}
    traffic = {(0, 5): 1000, (1, 5): 3000, (2, 6): 0, (3, 9): 50, (0, 4): 10}    # rank 9 unknown
    for route in ECMP_ROUTES:
        got = db.mpi_exchange_times(ranks, traffic, capacity=100, host_capacity=2.0, route=route,
                                    split="hop")
        assert got.pairs == [(macs[0], macs[5]), (macs[1], macs[5]), (macs[2], macs[6]),
                             (macs[0], macs[4])]
        assert got.bytes.tolist() == [1000.0, 3000.0, 0.0, 10.0]
        # the port out to host 5 is shared by two flows, the port in from host 0 too
        assert got.rate0.tolist() == [1.0, 1.0, 0.0, 1.0]
        # 0 -> 4 is done at 10; 0 -> 5 still shares host 5's port and is done at 1000;
        # 1 -> 5 then has it alone: the 2000 bytes left go at 2.0
        assert got.time.tolist() == [1000.0, 2000.0, 0.0, 10.0] and got.makespan() == 2000.0
        assert got.split == "hop"
        every = db.mpi_exchange_times(ranks, route=route)
        assert len(every.pairs) == 56 and every.complete and every.makespan() > 0


def test_link_events_and_cost_changes_equal_a_fresh_database():
    fabric = T.fat_tree(4)
    db = times_db(fabric)
    capacity = seed_costs(db)
    pairs, w = dropin_pairs(fabric)
    nbytes = np.random.default_rng(5).integers(1, 100, len(pairs)).astype(np.float64)
    call = lambda x, r: x.fair_completion_times(pairs, nbytes, w, capacity, 2.0, r)  # noqa: E731
    before = {r: call(db, r) for r in ECMP_ROUTES}
    csr = db.graph().csr
    a, b = int(csr.dpids[0]), int(csr.dpids[int(csr.col[csr.row_ptr[0]])])
    ab, ba = db.links[a][b], db.links[b][a]
    db.delete_link(ab)
    db.delete_link(ba)
    fresh = times_db(fabric)
    seed_costs(fresh)
    fresh.delete_link(fresh.links[a][b])
    fresh.delete_link(fresh.links[b][a])
    for r in ECMP_ROUTES:
        # (the two databases hold their table rows in different slots: the
        # float sums run in another order)
        cut, other = call(db, r), call(fresh, r)
        assert np.allclose(cut.time, other.time, rtol=TOL, atol=0)
        assert np.array_equal(cut.epoch, other.epoch)
        assert np.allclose(cut.link_bytes.load, other.link_bytes.load, rtol=TOL, atol=0)
        assert not np.array_equal(cut.link_bytes.load, before[r].link_bytes.load)
    db.add_link(ab)
    db.add_link(ba)
    for r in ECMP_ROUTES:
        again = call(db, r)
        assert np.array_equal(again.time, before[r].time)
        assert np.array_equal(again.link_bytes.load, before[r].link_bytes.load)
    # a cost change moves the least-cost route sets and leaves the hop-count ones
    x, y = int(csr.dpids[0]), int(csr.dpids[int(csr.col[csr.row_ptr[0] + 1])])
    db.set_link_cost(x, y, 9)
    fresh = times_db(fabric)
    seed_costs(fresh)
    fresh.set_link_cost(x, y, 9)
    moved, other = call(db, "least_cost_ecmp"), call(fresh, "least_cost_ecmp")
    assert np.allclose(moved.time, other.time, rtol=TOL, atol=0)
    assert np.array_equal(moved.epoch, other.epoch)
    assert moved.link_bytes.as_dict() != before["least_cost_ecmp"].link_bytes.as_dict()
    assert np.array_equal(call(db, "ecmp").time, before["ecmp"].time)


def test_bad_arguments_and_the_single_path_routes():
    fabric = T.fat_tree(4)
    db = times_db(fabric)
    macs = fabric.host_macs()
    p = [(macs[0], macs[5])]
    empty = db.fair_completion_times([], [], route="ecmp", split="hop")
    assert empty.time.size == 0 and empty.epochs == 0 and empty.makespan() == 0.0
    assert empty.complete and empty.split == "hop"
    for kw in (dict(route="ecmp", split="flow"), dict(route="valiant"),
               dict(route="shortest", split="hop"), dict(route="default", split="hop"),
               dict(route="least_cost", split="hop"), dict(route="least_loaded", split="hop"),
               dict(route="ecmp", weights=[-1]), dict(route="ecmp", capacity=0),
               dict(route="least_cost_ecmp", host_capacity=0), dict(route="ecmp", max_epochs=-1)):
        with pytest.raises(ValueError):
            db.fair_completion_times(p, 1.0, **kw)
    for bad in (-1.0, float("nan"), float("inf"), [1.0, 2.0]):
        with pytest.raises(ValueError):
            db.fair_completion_times(p, bad, route="ecmp")
    with pytest.raises(ValueError):
        db.all_pairs_fair_completion_times(1.0, route="shortest", split="hop")
    with pytest.raises(ValueError):
        db.mpi_exchange_times({0: macs[0], 1: macs[5]}, route="default", split="hop")
    # the single-path routes go on through fair_times, with the default split
    for route in ROUTES:
        got = db.fair_completion_times(p, 1.0, route=route, split="route")
        assert got.routed.all() and got.split == "route"
        assert db._engine.calls[-1][0] == "times"
    assert db.fair_completion_times(p, 1.0, route="ecmp").routed.all()
    assert db._engine.calls[-1][0] == "ecmp_times"
    # an engine with the multipath filling but without the multipath epochs
    # rejects the multipath routes rather than put the pair on one path
    older = fake_db(fabric)
    older._engine = FakeEcmpFairEngine()
    assert not hasattr(older.engine, "ecmp_fair_times")
    for route in ECMP_ROUTES:
        with pytest.raises(ValueError, match="ecmp_fair_times") as ei:
            older.fair_completion_times(p, 1.0, route=route)
        assert all(repr(r) in str(ei.value) for r in ROUTES)
