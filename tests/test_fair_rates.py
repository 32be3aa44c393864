"""Max-min fair flow rates (engine.fair_rates_host, TopologyDB.fair_rates and
friends), CPU only: the numpy restatement of fair_rates.hip against textbook
progressive filling in exact fractions over explicit link lists, closed forms,
the max-min certificate, and the drop-in over an engine double built from the
restatements against the same exact filling over the routes find_route returns.

Rounds, round and bottleneck must be equal; rates and carried rates agree
within TOL (16 times the largest relative deviation measured
over the seeded cases of this file, capped at 1e-9 -- a wrong freeze order
changes a rate by a fraction like 1/3 against 1/2)."""
from fractions import Fraction

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import FairRates, SplitLinkLoads, TopologyDB
from test_cost_ecmp_loads import both_ways, digraph_csr
from test_ecmp_link_loads import edge_map
from test_widest_tables import FakeWidestEngine, seed_utilisation

# largest relative deviation of a rate, a level or a carried rate measured over
# the seeded G.SMALL cases below: 2.4e-15 (fat_tree_k8, 305 rounds); 16 times
# that, far below the 1e-9 cap
TOL = 16 * 2.4e-15
CAPS = (1, 2, 3, 10, 40, 100)
LAYOUTS = (EN.INT32, EN.PORT16, EN.SLOT)
ROUTES = ("default", "shortest", "least_cost", "least_loaded")
BIG = 1 << 60


class FakeFairEngine(FakeWidestEngine):
    """The restatement double plus fair_rates."""

    def fair_rates(self, export, tree, layout, rows, verts, mult=None, cap=None, extra=None,
                   to_root=False, timing=False):
        self.calls.append(("fair", export.key, len(rows)))
        if cap is None:
            cap = np.ones(int(export.csr.E))
        return EN.fair_rates_host(export.csr, tree, layout, rows, verts, mult, cap, extra, to_root)


def fake_db(fabric, **kw):
    db = fabric.populate(TopologyDB(**kw))
    db._engine = FakeFairEngine()
    return db


# ------------------------------------------------ the exact reference --

def exact_fair(paths, mult, cap):
    """Textbook progressive filling in exact fractions.  ``paths[i]``: the
    constraints flow i crosses, in the order its bottleneck is looked for, or
    None for a flow without a route; ``mult[i]`` identical flows each; ``cap``
    per constraint.  All alive rates rise together; a constraint is full when
    its spare capacity over its alive flows is the smallest; its flows freeze.
    Returns (rate -- Fractions, inf for a routed flow that crosses nothing --,
    bott, round, levels, used)."""
    n, m = len(paths), len(cap)
    mult = np.asarray(mult, np.int64)
    cap = [Fraction(c) for c in cap]
    fl = np.asarray([i for i, p in enumerate(paths) if p for _ in p], np.int64)
    ln = np.asarray([e for p in paths if p for e in p], np.int64)
    pos = np.asarray([j for p in paths if p for j in range(len(p))], np.int64)
    rate = [Fraction(0)] * n
    bott, rnd = [-1] * n, [-1] * n
    alive = np.zeros(n, bool)
    for i, p in enumerate(paths):
        if p is not None and mult[i] > 0:
            if len(p):
                alive[i] = True
            else:
                rate[i] = float("inf")
    frozen_load = [Fraction(0)] * m
    levels = []
    while alive.any():
        sel = alive[fl]
        cnt = np.zeros(m, np.int64)
        np.add.at(cnt, ln[sel], mult[fl[sel]])
        share = {e: (cap[e] - frozen_load[e]) / int(cnt[e]) for e in np.nonzero(cnt)[0].tolist()}
        r = min(share.values())
        full = np.zeros(m, bool)
        full[[e for e, s in share.items() if s == r]] = True
        hit = sel & full[ln]
        first = np.full(n, BIG, np.int64)
        np.minimum.at(first, fl[hit], pos[hit])
        out = np.nonzero(first < BIG)[0]
        assert out.size
        for i in out.tolist():
            rate[i], rnd[i], bott[i] = r, len(levels), paths[i][first[i]]
        gone = np.zeros(n, bool)
        gone[out] = True
        took = np.zeros(m, np.int64)
        sel = gone[fl]
        np.add.at(took, ln[sel], mult[fl[sel]])
        for e in np.nonzero(took)[0].tolist():
            frozen_load[e] += r * int(took[e])
        alive[out] = False
        levels.append(r)
    return rate, bott, rnd, levels, frozen_load


def table_paths(csr, tab, rows, verts, to_root, extra=None):
    """The link lists of flows by following int32 table rows from the flow's
    vertex to the root (None: unreached or no vertex), extras appended."""
    em = edge_map(csr)
    out = []
    for i, (r, x) in enumerate(zip(np.asarray(rows).tolist(), np.asarray(verts).tolist())):
        if not 0 <= x < csr.V:
            out.append(None)
            continue
        path, ok = [], True
        while True:
            p = int(tab[r, x])
            if p == x or (p < 0 and to_root):
                break
            if p < 0:
                ok = False
                break
            path.append(em[(x, p)] if to_root else em[(p, x)])
            x = p
            assert len(path) <= csr.V
        if ok and extra is not None:
            path += [int(e) for e in extra[i] if e >= 0]
        out.append(path if ok else None)
    return out


def rel_dev(got, want):
    """Largest |got - want| / want over the finite nonzero entries of ``want``
    (Fractions); everything else must be equal."""
    worst = 0.0
    for g, w in zip(np.asarray(got).tolist(), want):
        if w == float("inf") or w == 0:
            assert g == w
        else:
            worst = max(worst, float(abs(Fraction(g) - w) / w))
    return worst


def certificate(paths, mult, cap, rate, used, tol):
    """used <= cap, and every finite-rate flow has a full link on which no
    flow has a larger rate: the allocation is max-min fair."""
    cap = np.asarray(cap, np.float64)
    assert (used <= cap * (1 + tol)).all()
    full = used >= cap * (1 - tol)
    top = np.zeros(cap.shape[0])
    for p, m, r in zip(paths, mult, rate):
        if p and m > 0:
            for e in p:
                top[e] = max(top[e], r)
    for p, m, r in zip(paths, mult, rate):
        if p and m > 0:
            assert np.isfinite(r) and r > 0
            assert any(full[e] and top[e] <= r * (1 + tol) for e in p)


def check_case(csr, tab, layout, tree, rows, verts, mult, cap, to_root, extra=None, exact=None,
               same_rounds=True):
    """fair_rates_host of one case against the exact filling; returns the
    largest relative deviation of the rates and the carried rates.
    ``same_rounds`` False: only the rates, the carried rates and the
    certificate are compared -- links whose shares tie exactly can round one
    unit in the last place apart and then freeze in two consecutive rounds
    (DESIGN.md 4.16)."""
    paths = table_paths(csr, tab, rows, verts, to_root, extra)
    m = np.ones(len(paths), np.int64) if mult is None else np.asarray(mult).astype(np.int64)
    if exact is None:
        exact = exact_fair(paths, m, cap)
    rate, bott, rnd, level, used = EN.fair_rates_host(csr, tree, layout, rows, verts, mult, cap,
                                                      extra, to_root)
    assert rate.dtype == np.float64 and bott.dtype == np.int32 and rnd.dtype == np.int32
    dev = max(rel_dev(rate, exact[0]), rel_dev(used, exact[4]))
    if same_rounds:
        assert rnd.tolist() == exact[2] and bott.tolist() == exact[1]
        assert len(level) == len(exact[3])
        dev = max(dev, rel_dev(level, exact[3]))
    assert dev <= TOL
    assert (np.diff(level) > 0).all()
    certificate(paths, m, cap, rate, used, TOL)
    return dev, exact


def small_case(name):
    """One G.SMALL fabric with the oracle's tables, every switch pair as a
    flow, and seeded multiplicities and capacities: the seeds the GPU file
    shares.  Returns a dict."""
    from oracle import oracle as O
    k = G.SMALL.index(name)
    csr = G.Golden(name).fabric().csr()
    ids = np.arange(csr.V, dtype=np.int32)
    par, prt, _ = O.dfs_tables(csr, ids)
    _, nh, _ = O.dest_tables(csr, ids)
    rng = np.random.default_rng(300 + k)
    rows = np.repeat(np.arange(csr.V), csr.V)
    verts = np.tile(np.arange(csr.V), csr.V)
    mult = rng.integers(0, 6, rows.shape[0]).astype(np.uint64)
    cap = rng.choice(np.asarray(CAPS, np.float64), int(csr.E))
    return dict(csr=csr, par=par, prt=prt, nh=nh, rows=rows, verts=verts, mult=mult, cap=cap)


def layout_tree(c, layout):
    return c["par"] if layout == EN.INT32 else EN.pack_host_tree(c["par"], c["prt"], c["csr"],
                                                                 layout)


@pytest.mark.parametrize("name", G.SMALL)
def test_restatement_equals_exact_filling(name):
    c = small_case(name)
    csr, rows, verts, mult, cap = c["csr"], c["rows"], c["verts"], c["mult"], c["cap"]
    exact = None
    worst = 0.0
    for lay in LAYOUTS:
        if lay == EN.SLOT and np.diff(csr.row_ptr).max() > 62:
            continue
        dev, exact = check_case(csr, c["par"], lay, layout_tree(c, lay), rows, verts, mult, cap,
                                False, exact=exact)
        worst = max(worst, dev)
    dev, _ = check_case(csr, c["nh"], EN.INT32, c["nh"], rows, verts, mult, cap, True)
    # unit multiplicities (mult None) on the next-hop rows: many exact ties
    unit, _ = check_case(csr, c["nh"], EN.INT32, c["nh"], rows, verts, None, cap, True,
                         same_rounds=False)
    print("fair rates %s: largest relative deviation %.3g" % (name, max(worst, dev, unit)))


# ------------------------------------------------------- closed forms --

def line_csr(n):
    """Vertices 0 .. n on a line, links both ways."""
    return digraph_csr(both_ways([(i, i + 1) for i in range(n)]), n + 1)


def line_to_end(csr):
    """The next-hop row of a line toward its last vertex, and the edge index
    of every link v -> v + 1."""
    n = csr.V - 1
    em = edge_map(csr)
    nh = np.full((1, n + 1), -1, np.int32)
    nh[0, :n] = np.arange(1, n + 1)
    return nh, np.asarray([em[(v, v + 1)] for v in range(n)], np.int64)


def test_one_link_two_flows():
    csr = line_csr(1)
    nh, fwd = line_to_end(csr)
    cap = np.full(csr.E, 7.0)
    cap[fwd[0]] = 3.0
    rate, bott, rnd, level, used = EN.fair_rates_host(csr, nh, EN.INT32, [0, 0], [0, 0], None,
                                                      cap, to_root=True)
    assert rate.tolist() == [1.5, 1.5] and bott.tolist() == [fwd[0]] * 2 and rnd.tolist() == [0, 0]
    assert level.tolist() == [1.5] and used[fwd[0]] == 3.0 and used.sum() == 3.0
    # one flow of multiplicity 2 is the same two flows
    rate, _, _, _, used = EN.fair_rates_host(csr, nh, EN.INT32, [0], [0], [2], cap, to_root=True)
    assert rate.tolist() == [1.5] and used[fwd[0]] == 3.0


def test_three_flow_line():
    """0 - 1 - 2 with capacities 1 and 2: the long flow and the short one on
    the first link get 1/2 each, the short one on the second link 3/2."""
    csr = line_csr(2)
    em = edge_map(csr)
    cap = np.ones(csr.E)
    cap[em[(0, 1)]], cap[em[(1, 2)]] = 1.0, 2.0
    nh = np.array([[1, 2, -1], [1, -1, 1]], np.int32)         # toward 2, toward 1
    rate, bott, rnd, level, used = EN.fair_rates_host(csr, nh, EN.INT32, [0, 1, 0], [0, 0, 1],
                                                      None, cap, to_root=True)
    assert rate.tolist() == [0.5, 0.5, 1.5] and rnd.tolist() == [0, 0, 1]
    assert bott.tolist() == [em[(0, 1)], em[(0, 1)], em[(1, 2)]]
    assert level.tolist() == [0.5, 1.5]
    assert used[em[(0, 1)]] == 1.0 and used[em[(1, 2)]] == 2.0


@pytest.mark.parametrize("n", [1, 2, 5, 64, 200])
def test_path_with_square_capacities(n):
    """Line 0 .. n toward n, a flow from every vertex, cap[v -> v + 1] =
    (v + 1)^2: flow v gets 2v + 1, one flow per round, all exact in doubles."""
    csr = line_csr(n)
    nh, fwd = line_to_end(csr)
    cap = np.ones(csr.E)
    cap[fwd] = (np.arange(n) + 1.0) ** 2
    rate, bott, rnd, level, used = EN.fair_rates_host(
        csr, nh, EN.INT32, np.zeros(n + 1, np.int64), np.arange(n + 1), None, cap, to_root=True)
    assert rate[:n].tolist() == (2.0 * np.arange(n) + 1).tolist() and rate[n] == np.inf
    assert rnd.tolist() == list(range(n)) + [-1] and bott.tolist() == fwd.tolist() + [-1]
    assert level.tolist() == rate[:n].tolist()
    assert used[fwd].tolist() == cap[fwd].tolist() and used.sum() == cap[fwd].sum()


def test_tie_takes_the_link_nearer_the_vertex():
    """Two links full in the same round and a flow over both: its bottleneck
    is the one met first walking from its vertex toward the root."""
    csr = line_csr(2)
    em = edge_map(csr)
    cap = np.ones(csr.E)
    nh = np.array([[1, 2, -1], [1, -1, 1]], np.int32)
    # flows 0 -> 2, 0 -> 1, 1 -> 2 on unit links: both links fill at 1/2
    rate, bott, rnd, _, _ = EN.fair_rates_host(csr, nh, EN.INT32, [0, 1, 0], [0, 0, 1], None,
                                               cap, to_root=True)
    assert rate.tolist() == [0.5] * 3 and rnd.tolist() == [0] * 3
    assert bott.tolist() == [em[(0, 1)], em[(0, 1)], em[(1, 2)]]
    # the same flows in the tree of source 0 (vertex = destination): walking
    # from 2 toward 0 the long flow meets 1 -> 2 first
    par = np.array([[0, 0, 1], [1, 1, 1]], np.int32)          # trees of sources 0 and 1
    rate, bott, _, _, _ = EN.fair_rates_host(csr, par, EN.INT32, [0, 0, 1], [2, 1, 2], None, cap)
    assert rate.tolist() == [0.5] * 3
    assert bott.tolist() == [em[(1, 2)], em[(0, 1)], em[(1, 2)]]


# ------------------------------------------------------ special values --

def test_special_values_and_extras():
    csr = line_csr(2)
    em = edge_map(csr)
    E = csr.E
    nh = np.array([[1, 2, -1]], np.int32)
    par = np.array([[0, 0, -1]], np.int32)                   # tree of 0; 2 unreached
    cap = np.concatenate([np.full(E, 10.0), [4.0, 1.0, 6.0]])
    ex = lambda *a: np.asarray(a, np.int64).reshape(-1, 2)   # noqa: E731
    # s == d without extras: +inf; with extras: the host ports limit it
    r, b, k, lv, used = EN.fair_rates_host(csr, nh, EN.INT32, [0, 0], [2, 2], None, cap,
                                           ex(-1, -1, E, E + 2), to_root=True)
    assert r.tolist() == [np.inf, 4.0] and b.tolist() == [-1, E] and k.tolist() == [-1, 0]
    assert lv.tolist() == [4.0] and used[E] == 4.0 and used[E + 2] == 4.0
    # an extra full before, with and after the path links
    for host, want, bott in ((1.0, 1.0, E + 1), (10.0, 10.0, em[(0, 1)]), (40.0, 10.0, em[(0, 1)])):
        cap[E + 1] = host
        r, b, _, _, _ = EN.fair_rates_host(csr, nh, EN.INT32, [0], [0], None, cap,
                                           ex(E + 1, -1), to_root=True)
        assert r.tolist() == [want] and b.tolist() == [bott]
    # the second extra only when the first is not full
    cap[E:] = [5.0, 5.0, 2.0]
    r, b, _, _, _ = EN.fair_rates_host(csr, nh, EN.INT32, [0], [2], None, cap, ex(E, E + 2),
                                       to_root=True)
    assert r.tolist() == [2.0] and b.tolist() == [E + 2]
    # multiplicity 0 is absent; unreached and out-of-range vertices read 0.0
    r, b, k, lv, used = EN.fair_rates_host(csr, par, EN.INT32, [0] * 5, [1, 1, 2, 7, -1],
                                           [0, 3, 1, 1, 1], cap[:E])
    assert r.tolist() == [0.0, 10 / 3, 0.0, 0.0, 0.0] and k.tolist() == [-1, 0, -1, -1, -1]
    assert b.tolist() == [-1, em[(0, 1)], -1, -1, -1] and used[em[(0, 1)]] == 10.0
    # no flows at all
    r, b, k, lv, used = EN.fair_rates_host(csr, nh, EN.INT32, [], [], None, cap[:E], to_root=True)
    assert r.size == b.size == k.size == lv.size == 0 and not used.any()


def test_rejected_arguments():
    csr = line_csr(2)
    nh = np.array([[1, 2, -1]], np.int32)
    cap = np.ones(csr.E)
    with pytest.raises(ValueError):                           # a total of 2**53
        EN.fair_rates_host(csr, nh, EN.INT32, [0, 0], [0, 1], [1 << 52, 1 << 52], cap, to_root=True)
    EN.fair_rates_host(csr, nh, EN.INT32, [0, 0], [0, 1], [1 << 52, (1 << 52) - 1], cap,
                       to_root=True)
    for bad in (0.0, -1.0, np.nan, np.inf):
        c = cap.copy()
        c[1] = bad
        with pytest.raises(ValueError):
            EN.fair_rates_host(csr, nh, EN.INT32, [0], [0], None, c, to_root=True)
    with pytest.raises(ValueError):                           # an extra that is no constraint
        EN.fair_rates_host(csr, nh, EN.INT32, [0], [0], None, cap, [[csr.E, -1]], to_root=True)
    with pytest.raises(ValueError):                           # a 2-cycle is no tree
        EN.fair_rates_host(csr, np.array([[1, 0, -1]], np.int32), EN.INT32, [0], [0], None, cap,
                           to_root=True)
    with pytest.raises(ValueError):                           # a tree link the graph lacks
        EN.fair_rates_host(csr, np.array([[2, 2, -1]], np.int32), EN.INT32, [0], [0], None, cap,
                           to_root=True)


# ------------------------------------------------------------ drop-in --

def route_of(db, route, a, b):
    if route == "default":
        return db.find_route(a, b)
    if route == "shortest":
        return (db.find_route(a, b, True) or [[]])[0]
    if route == "least_cost":
        return db.find_route_least_cost(a, b)
    return db.find_route_least_loaded(a, b)


def dropin_exact(db, pairs, weights, capacity, host_capacity, route):
    """Exact filling over the routes the drop-in itself returns: per pair the
    fabric links of its fdb entries (walked from the destination for the
    default trees, from the source for the next-hop rows, as the kernel looks
    for the bottleneck), plus the two host ports when they are modelled."""
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
        links = [(fdb[i][0], fdb[i + 1][0]) for i in range(len(fdb) - 1)]
        if route == "default":
            links.reverse()
        p = [idx(lk, capacity(lk)) for lk in links]
        if host_capacity is not None:
            p += [idx(("in", a), host_capacity), idx(("out", b), host_capacity)]
        paths.append(p)
    w = [1] * len(pairs) if weights is None else weights
    rate, bott, rnd, levels, _ = exact_fair(paths, w, cap)
    back = {v: k for k, v in names.items()}
    bott = [None if e < 0 else back[e] for e in bott]
    bott = [("host", x[1]) if x is not None and x[0] in ("in", "out") else x for x in bott]
    return rate, bott, rnd, levels


def check_dropin(db, pairs, weights, capacity, host_capacity, route):
    capf = (lambda lk: 1) if capacity is None else \
        (lambda lk: capacity) if not isinstance(capacity, dict) else \
        (lambda lk: capacity.get(lk, 1))
    rate, bott, rnd, levels = dropin_exact(db, pairs, weights, capf, host_capacity, route)
    got = db.fair_rates(pairs, weights, capacity, host_capacity, route)
    assert isinstance(got, FairRates) and isinstance(got.link_rate, SplitLinkLoads)
    assert got.routed.tolist() == [bool(route_of(db, route, a, b)) for a, b in pairs]
    w = np.ones(len(pairs), np.int64) if weights is None else np.asarray(weights)
    live = got.routed & (w > 0)
    assert rel_dev(got.rate[live], [r for r, ok in zip(rate, live) if ok]) <= TOL
    assert not got.rate[~live].any()
    assert [x for x, ok in zip(got.bottleneck, live) if ok] == \
        [x for x, ok in zip(bott, live) if ok]
    assert got.round[live].tolist() == [k for k, ok in zip(rnd, live) if ok]
    assert got.rounds == len(levels) and rel_dev(got.levels, levels) <= TOL
    return got


def dropin_pairs(fabric):
    macs = fabric.host_macs()
    pairs = [(a, b) for a in macs[::3] for b in macs[::2]]
    pairs += [(macs[0], "02:00:00:00:00:77"), ("02:00:00:00:00:78", macs[1])]   # unknown hosts
    rng = np.random.default_rng(21)
    return pairs, rng.integers(0, 4, len(pairs)).tolist()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("host_capacity", [None, 1.5])
def test_dropin_equals_exact_filling_over_its_routes(route, host_capacity):
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    csr = db.graph().csr
    rng = np.random.default_rng(22)
    for (u, v) in zip(np.repeat(np.arange(csr.V), np.diff(csr.row_ptr)).tolist(),
                      np.asarray(csr.col).tolist()):
        db.set_link_cost(int(csr.dpids[u]), int(csr.dpids[v]), int(rng.integers(1, 4)))
    seed_utilisation(db, 3, 23)
    pairs, w = dropin_pairs(fabric)
    links = [(int(csr.dpids[u]), int(csr.dpids[v])) for u, v in
             zip(np.repeat(np.arange(csr.V), np.diff(csr.row_ptr)).tolist(),
                 np.asarray(csr.col).tolist())]
    capacity = {lk: int(c) for lk, c in zip(links, rng.choice(CAPS, len(links)))}
    got = check_dropin(db, pairs, w, capacity, host_capacity, route)
    assert not got.routed[-2:].any() and got.bottleneck[-1] is None
    check_dropin(db, pairs, None, None, host_capacity, route)
    check_dropin(db, pairs, None, 2.5, host_capacity, route)
    # the result's summaries
    live = got.routed & (np.asarray(w) > 0)
    assert got.min_rate == got.levels[0] == got.rate[live].min()
    assert got.slowest() == [p for p, k in zip(pairs, got.round.tolist()) if k == 0]
    fin = live & np.isfinite(got.rate)
    assert got.total == pytest.approx(float((got.rate[fin] * np.asarray(w)[fin]).sum()))
    full = got.saturated_links()
    assert set(b for b, ok in zip(got.bottleneck, fin) if ok) <= set(full)
    ld = got.link_rate.as_dict()
    assert all(x > 0 for x in ld.values())
    if host_capacity is not None:
        assert any(isinstance(b, tuple) and b[0] == "host" for b in got.bottleneck if b)
        assert max(got.link_rate.host_load) <= host_capacity * (1 + TOL)


def test_same_switch_pairs_and_host_ports():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    a, b = macs[0], macs[1]
    assert db.find_route(a, b) and len(db.find_route(a, b)) == 1        # the same edge switch
    got = db.fair_rates([(a, b), (a, a)])
    assert got.rate.tolist() == [np.inf, np.inf] and got.routed.all() and got.rounds == 0
    assert got.bottleneck == [None, None] and got.min_rate == np.inf and got.total == 0.0
    got = db.fair_rates([(a, b), (a, macs[2])], capacity=10, host_capacity=3.0)
    assert got.rate.tolist() == [1.5, 1.5] and got.bottleneck == [("host", a)] * 2
    assert got.saturated_links() == [("host", a)]
    assert got.link_rate.as_dict()[db.find_route(a, b)[0]] == 1.5


def test_all_pairs_form_equals_the_mac_pair_form():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    allp = [(a, b) for a in macs for b in macs if a != b]
    for route in ROUTES:
        ap = db.all_pairs_fair_rates(route=route)
        mp = db.fair_rates(allp, route=route)
        assert np.array_equal(ap.levels, mp.levels)
        assert np.array_equal(ap.link_rate.load, mp.link_rate.load)
        assert ap.total == pytest.approx(mp.total) and ap.min_rate == mp.min_rate
        assert int(ap.weights.sum()) == len(allp)
        sw = {m: db.hosts[m].port.dpid for m in macs}
        by = dict(zip(ap.pairs, ap.rate.tolist()))
        assert [by[(sw[a], sw[b])] for a, b in allp] == mp.rate.tolist()


def test_mpi_times():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    ranks = {r: macs[r] for r in range(8)}
    traffic = {(0, 5): 1000, (1, 5): 3000, (2, 6): 0, (3, 9): 50, (0, 4): 10}    # rank 9 unknown
    got = db.mpi_fair_rates(ranks, traffic, capacity=100, host_capacity=2.0)
    assert got.pairs == [(macs[0], macs[5]), (macs[1], macs[5]), (macs[2], macs[6]),
                         (macs[0], macs[4])]
    assert got.bytes.tolist() == [1000.0, 3000.0, 0.0, 10.0]
    assert np.array_equal(got.time, np.where(got.bytes == 0, 0.0, got.bytes / got.rate))
    assert got.rate[:2].tolist() == [1.0, 1.0] and got.step_time() == 3000.0
    every = db.mpi_fair_rates(ranks)
    assert len(every.pairs) == 56 and every.step_time() == 1.0 / every.min_rate
    with pytest.raises(ValueError):
        db.fair_rates([(macs[0], macs[5])]).step_time()


def test_link_events_equal_a_fresh_database():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    pairs, w = dropin_pairs(fabric)
    before = db.fair_rates(pairs, w, host_capacity=2.0)
    t = db.route_tables("dfs")
    a = int(t["dpids"][t["parent"][0][0]])
    ab, ba = db.links[a][1], db.links[1][a]
    db.delete_link(ab)
    db.delete_link(ba)
    cut = check_dropin(db, pairs, w, None, 2.0, "default")
    fresh = fake_db(fabric)
    fresh.delete_link(fresh.links[a][1])
    fresh.delete_link(fresh.links[1][a])
    other = fresh.fair_rates(pairs, w, host_capacity=2.0)
    assert np.array_equal(cut.rate, other.rate) and cut.bottleneck == other.bottleneck
    db.add_link(ab)
    db.add_link(ba)
    again = db.fair_rates(pairs, w, host_capacity=2.0)
    assert np.array_equal(again.rate, before.rate) and again.bottleneck == before.bottleneck
    assert np.array_equal(again.link_rate.load, before.link_rate.load)


def test_bad_arguments_and_the_budget():
    fabric = T.fat_tree(4)
    db = fake_db(fabric)
    macs = fabric.host_macs()
    p = [(macs[0], macs[5])]
    empty = db.fair_rates([])
    assert empty.rate.size == 0 and empty.rounds == 0 and empty.min_rate is None
    for kw in (dict(route="ecmp"), dict(weights=[-1]), dict(weights=[1 << 53]),
               dict(capacity=0), dict(capacity={(1, 2): -1.0}), dict(host_capacity=0),
               dict(host_capacity=float("inf")), dict(capacity=float("nan"))):
        with pytest.raises(ValueError):
            db.fair_rates(p, **kw)
    with pytest.raises(ValueError):
        db.fair_rates([(macs[0], macs[5]), (macs[1], macs[6])], weights=[1 << 52, 1 << 52])
    # every row of a call stays resident: a budget of 2 rows cannot hold 4
    csr = fabric.csr()
    for route, row_bytes in (("default", EN.dfs_row_bytes(csr)), ("shortest", EN.sp_row_bytes(csr)),
                             ("least_cost", 12 * csr.V), ("least_loaded", 24 * csr.V)):
        small = fake_db(fabric, batch_sources=False, table_budget=3 * row_bytes)
        pairs = [(macs[i], macs[j]) for i in (0, 2, 4, 6) for j in (1, 3, 5, 7)]
        with pytest.raises(ValueError, match="budget"):
            small.fair_rates(pairs, route=route)
        assert small.fair_rates(pairs[:2], route=route).routed.all()
