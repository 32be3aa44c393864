"""Self-loop links (a cable between two ports of one switch, stored by the
reference as links[u][u], topology_db.py:30-35) through every kernel entry
point, on a gfx950 device.

A self-loop is inert: the reference answers as without it (pinned by
make_golden.run_fabric for the four *_loops fixtures).  What it changes is the
shape of what the kernels read -- a row holds its own vertex, slot positions
shift, in- and out-degree grow by one -- so every call is checked two ways:
against the oracle / the host restatement on the graph as it is, and against
the same call on the graph with the self-loops deleted (V unchanged): tables
bit-equal, loads equal edge by edge with exactly 0 on every self-loop edge.

Graphs (V <= 131): the four fixtures; a hub whose out-degree, its self-loop
counted, is 32, 33, 63, 64 or 65 (paired in-rows up to 32, the slot layout's
63-link cap, the 64-wide rows), alone and with a self-loop on every leaf; a
star in which two leaves that would be twins carry a self-loop each.

Tolerance: integer results exactly; the float64 loads with
test_ecmp_link_loads.dicts_close (rtol 1e-9, identical key sets, exact zeros;
derived there)."""
import numpy as np
import pytest

import golden_util as G
from oracle import oracle as O
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd.topologies import CSR
from test_dfs_fold_live_gpu import check as fold_check
from test_dfs_fold_live_gpu import twin_reps_py
from test_ecmp_link_loads import SPLITS, dicts_close
from test_ecmp_link_loads_gpu import dev_dist
from test_failure_loads import cable_edges
from test_link_loads_gpu import dev_tree, on

pytestmark = pytest.mark.gpu

HUB_DEGREES = (32, 33, 63, 64, 65)
GRAPHS = list(G.LOOPS) + ["hub%d" % d for d in HUB_DEGREES] + \
    ["hub%d_leaf_loops" % d for d in HUB_DEGREES] + ["twins"]
DFS_STRATEGIES = ["auto", "async", "count", "lds", "global"]


# ----------------------------------------------------------------- graphs --

def csr_from_rows(nb):
    """CSR of ascending neighbour lists; vertex u has dpid 3 u + 5, the k-th
    link of the graph port k + 1 (distinct, 16-bit)."""
    rp = np.concatenate([[0], np.cumsum([len(a) for a in nb])])
    col = np.array([v for a in nb for v in a], np.int64)
    return CSR(3 * np.arange(len(nb)) + 5, rp, col, np.arange(1, len(col) + 1))


def hub_ladder(degree, leaf_loops):
    """Hub 0 with ``degree`` out-links, its self-loop among them, symmetric
    links to the leaves 1 .. degree - 1 (in-degree == out-degree), neighbouring
    leaves (1-2, 3-4, ...) joined so that the trees are no plain star, and a
    vertex nothing reaches."""
    V = degree + 1
    nb = [set() for _ in range(V)]
    nb[0].add(0)
    for v in range(1, degree):
        nb[0].add(v)
        nb[v].add(0)
        if leaf_loops:
            nb[v].add(v)
    for v in range(1, degree - 1, 2):
        nb[v].add(v + 1)
        nb[v + 1].add(v)
    nb[degree].add(1)                        # V - 1 reaches the rest, nothing reaches it
    assert len(nb[0]) == degree
    return csr_from_rows([sorted(a) for a in nb])


def twins_star():
    """Hub 0 and 40 leaves, links both ways (the hub's in-degree is above 32:
    no paired in-rows).  Leaves 1 and 2 carry a self-loop each: without it they
    would be twins of the others, with it they stay alone; 3 .. 40 are one
    class."""
    nb = [list(range(1, 41))] + [[0] for _ in range(40)]
    nb[1].append(1)
    nb[2].append(2)
    return csr_from_rows(nb)


class Case(object):
    """One graph, the same graph without its self-loop links, and the oracle's
    tables of both (computed once, never changed)."""

    def __init__(self, name):
        if name in G.LOOPS:
            csr = G.Golden(name).fabric().csr()
        elif name == "twins":
            csr = twins_star()
        else:
            csr = hub_ladder(int(name[3:5]), name.endswith("leaf_loops"))
        self.name, self.csr = name, csr
        V = self.V = int(csr.V)
        self.esrc = np.repeat(np.arange(V), np.diff(csr.row_ptr))
        self.keep = self.esrc != csr.col                 # the links that are no self-loop
        self.loops = np.nonzero(~self.keep)[0]
        assert self.loops.size and V <= 131
        rp = np.zeros(V + 1, np.int64)
        np.cumsum(np.bincount(self.esrc[self.keep], minlength=V), out=rp[1:])
        self.bare = CSR(csr.dpids, rp, csr.col[self.keep], csr.port[self.keep])
        self.to_bare = np.cumsum(self.keep) - 1          # edge index in the bare graph
        self.ids = np.arange(V, dtype=np.int32)
        self.dfs = O.dfs_tables(csr, self.ids)
        self.sp = O.dest_tables(csr, self.ids)
        # inert on the host: the oracle's tables of both graphs are the same
        for a, b in zip(self.dfs + self.sp, O.dfs_tables(self.bare, self.ids) +
                        O.dest_tables(self.bare, self.ids)):
            assert np.array_equal(a, b), name
        self.exports = {True: on(csr), False: on(self.bare)}

    def both(self):
        """(graph, looped?) for the graph and for its loop-free twin."""
        return [(self.csr, True), (self.bare, False)]

    def costs(self, seed, loop_cost):
        """Random costs in [1, 9] on the links, ``loop_cost`` on the self-loops:
        (cost of the graph, cost of the bare graph)."""
        c = np.random.default_rng(seed).integers(1, 10, int(self.csr.E)).astype(np.uint32)
        c[self.loops] = loop_cost
        return c, c[self.keep]

    def max_cost(self):
        """The largest cost sdnr_graph_costs takes: cost * (V - 1) < COST_INF."""
        return (EN.COST_INF - 1) // (self.V - 1)

    def pairs(self, seed, n=None):
        """(rows, others, weights): random rows, switches from -1 to V (both
        outside the graph), u32 weights with zeros."""
        rng = np.random.default_rng(seed)
        n = n or 4 * self.V
        rows = rng.integers(0, self.V, n)
        other = rng.integers(-1, self.V + 1, n)
        w = rng.integers(0, 1 << 32, n, dtype=np.uint64)
        w[rng.random(n) < 0.2] = 0
        return rows, other, w


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def host(a, dtype=None):
    a = a.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def loads_equal(c, looped, bare, exact):
    """Loads of the graph against those of the bare graph, edge by edge; every
    self-loop edge carries exactly 0."""
    looped, bare = np.asarray(looped), np.asarray(bare)
    assert looped.shape[-1] == c.csr.E and bare.shape[-1] == c.bare.E
    assert not looped[..., c.loops].any(), "a self-loop link carries load"
    a, b = looped[..., c.keep].reshape(-1), bare.reshape(-1)
    if exact:
        return bool(np.array_equal(a, b))
    return dicts_close(as_dict(a), as_dict(b))


def as_dict(load):
    """{edge: load} of the nonzero entries, for dicts_close."""
    load = np.asarray(load, np.float64).reshape(-1)
    assert np.isfinite(load).all()
    return {int(e): float(load[e]) for e in np.nonzero(load)[0]}


def loads_close(got, want):
    assert np.asarray(got).dtype == np.float64
    return dicts_close(as_dict(got), as_dict(want))


# ------------------------------------------------------- default routes --

def expected_slots(csr, po):
    """Slot-tree words from oracle parents: the child's position in its
    parent's ascending CSR row (the row's self-loop entry counts), 63 for the
    root."""
    S, V = po.shape
    want = np.full((S, V), 0xFFFFFFFF, np.uint64)
    for i in range(S):
        for v in range(V):
            p = int(po[i, v])
            if p < 0:
                continue
            if p == v:
                want[i, v] = p | (63 << 26)
            else:
                row = csr.col[csr.row_ptr[p]:csr.row_ptr[p + 1]]
                k = int(np.searchsorted(row, v))
                assert row[k] == v
                want[i, v] = p | (k << 26)
    return want.astype(np.uint32)


def pack16(p, t):
    return ((p.astype(np.int64) & 0xFFFF) | ((t.astype(np.int64) & 0xFFFF) << 16)).astype(np.uint32)


@pytest.mark.parametrize("strategy", DFS_STRATEGIES)
@pytest.mark.parametrize("name", GRAPHS)
def test_dfs_tables_every_layout(eng, monkeypatch, name, strategy):
    """sdnr_dfs_tables, _packed, _slots and _tree (both layouts, both depth
    widths), every vertex a source, under each search strategy and with and
    without the ELL copy: the oracle's tables, on the graph and on its
    loop-free twin alike.  The slot layout holds rows of at most 63 links
    (sdnr_dfs_tables_slots: SDNR_ERR_INVAL above): hub64 and hub65 are refused
    with their self-loop and hub64's twin, 63 links, is taken."""
    if strategy != "auto":
        monkeypatch.setenv("SDNROUTE_DFS_STRATEGY", strategy)
    c = case(name)
    ctx = eng.ctx
    po, to, ho = c.dfs
    for ell in ("1", "0"):
        monkeypatch.setenv("SDNROUTE_ELL", ell)
        for csr, looped in c.both():
            ctx.upload(csr)
            eng._loaded = None
            where = (name, strategy, ell, looped)
            p, t, h = ctx.dfs_tables(c.ids)
            assert np.array_equal(p, po) and np.array_equal(t, to) and np.array_equal(h, ho), where
            p, t, _ = ctx.dfs_tables(c.ids, with_hops=False)
            assert np.array_equal(p, po) and np.array_equal(t, to), where
            tree = ctx.dfs_tables_packed(c.ids)
            assert np.array_equal(tree, pack16(po, to)), where
            trees = [(_native.TREE_PORT16, pack16(po, to))]
            if csr.max_degree() <= 63:
                slots = expected_slots(csr, po)
                trees.append((_native.TREE_SLOT, slots))
                tree = ctx.dfs_tables_slots(c.ids)
                assert np.array_equal(tree, slots), where
                # the slots decode back to the ports of the links
                p, t = _native.unpack_slots(tree, csr)
                assert np.array_equal(p, po) and np.array_equal(t, to), where
            else:
                assert name[:5] in ("hub64", "hub65"), where
                with pytest.raises(_native.SdnrError) as ei:
                    ctx.dfs_tables_slots(c.ids)
                assert ei.value.code == -22, where
                with pytest.raises(_native.SdnrError) as ei:
                    ctx.dfs_tables_tree(c.ids, _native.TREE_SLOT, 2)
                assert ei.value.code == -22, where
            for lay, want in trees:
                for depth_bytes in (2, 4):
                    tree, depth = ctx.dfs_tables_tree(c.ids, lay, depth_bytes)
                    assert np.array_equal(tree, want), where + (lay, depth_bytes)
                    assert np.array_equal(depth, ho.astype(np.uint16) if depth_bytes == 2 else ho), \
                        where + (lay, depth_bytes)


def test_would_be_twins_with_self_loops(eng, monkeypatch):
    """Two leaves that differ from a twin class only by their self-loops: the
    library leaves them unfolded (twin_reps_py's rule), a folded batch derives
    the class's rows and searches the rest, in the full and in the low-load
    form of the search."""
    c = case("twins")
    ctx = eng.ctx
    want = twin_reps_py(c.csr)
    assert want.tolist() == [0, 1, 2] + [3] * 38
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")
    monkeypatch.setenv("SDNROUTE_DFS_STRATEGY", "async")
    ctx.upload(c.csr)
    eng._loaded = None
    assert np.array_equal(ctx.twin_reps(), want)
    batches = [c.ids, np.array([2, 40, 1, 3, 0, 17, 2], np.int32)]
    for form in ("full", "low"):
        monkeypatch.setenv("SDNROUTE_DFS_FOLD_FORM", form)
        for layout in ("hops", "packed", "tree16", "slot32"):
            for k, srcs in enumerate(batches):
                assert fold_check(ctx, "self-loop twins", c.csr, srcs, layout) == 4
                if layout != "slot32":             # the slot layout goes through a pack pass
                    assert ctx.last_kernel().startswith("dfs_async_kernel"), ctx.last_kernel()
                    assert ctx.last_dfs_form() == form, (form, layout, k)
    # without the self-loops the two leaves join the class
    ctx.upload(c.bare)
    assert np.array_equal(ctx.twin_reps(), twin_reps_py(c.bare))
    assert ctx.twin_reps().tolist() == [0] + [1] * 40


# ------------------------------------------------------- shortest routes --

@pytest.mark.parametrize("strategy", ["auto", "plane", "msbfs"])
@pytest.mark.parametrize("name", GRAPHS)
def test_shortest_tables_apsp_and_ecmp(eng, monkeypatch, name, strategy):
    """sdnr_shortest_tables, sdnr_apsp, sdnr_ecmp_counts and the first and last
    route of every pair from sdnr_ecmp_routes, on both graphs."""
    if strategy != "auto":
        monkeypatch.setenv("SDNROUTE_SP_STRATEGY", strategy)
    c = case(name)
    ctx = eng.ctx
    do, nho, nhpo = c.sp
    V = c.V
    counts = np.stack([O.ecmp_counts(c.csr, do[d]) for d in range(V)])
    rows, srcs = (x.reshape(-1).astype(np.int32) for x in np.divmod(np.arange(V * V), V))
    routes = {}
    for csr, looped in c.both():
        ctx.upload(csr)
        eng._loaded = None
        dist, nh, nhp = ctx.shortest_tables(c.ids)
        assert np.array_equal(dist, do) and np.array_equal(nh, nho) and np.array_equal(nhp, nhpo)
        assert np.array_equal(ctx.apsp(), do.T)         # row d of dest tables = column d
        paths = ctx.ecmp_counts(dist)
        assert np.array_equal(paths, counts), (name, looped)
        L = int(do[do != 0xFFFF].max()) + 2
        last = np.where(counts > 0, counts - 1, 0).reshape(-1).astype(np.uint64)
        routes[looped] = (ctx.ecmp_routes(dist, paths, rows, srcs, np.zeros(V * V, np.uint64), L),
                          ctx.ecmp_routes(dist, paths, rows, srcs, last, L))
    for k in range(2):
        assert np.array_equal(routes[True][k], routes[False][k]), (name, k)
    first, final = routes[True]
    rp, col = c.bare.row_ptr, c.bare.col
    for i in range(0, V * V, 7):
        d, s = int(rows[i]), int(srcs[i])
        want = EN.shortest_paths_lex(rp, col, do[d], s, d)
        assert len(want) == int(counts[d, s])
        for got, w in ((first[i], want[:1]), (final[i], want[-1:])):
            w = w[0] if w else []
            assert got.tolist() == w + [-1] * (len(got) - len(w)), (name, d, s)


# ----------------------------------------------------- least-cost routes --

@pytest.mark.parametrize("loop_cost", ["one", "max"])
@pytest.mark.parametrize("name", GRAPHS)
def test_cost_widest_and_lfa_tables(eng, name, loop_cost):
    """sdnr_cost_tables under random costs in [1, 9] with the self-loops at
    cost 1 or at the largest cost the upload takes; sdnr_widest_tables with
    the self-loops' utilisation 0 or UTIL_MAX; sdnr_lfa_tables with and without
    SDNR_LFA_LINK_ONLY: the host restatements, and the same tables as on the
    loop-free graph.  No switch is its own backup."""
    c = case(name)
    cost, cost_bare = c.costs(31, 1 if loop_cost == "one" else c.max_cost())
    rng = np.random.default_rng(32)
    util = rng.integers(0, 1000, int(c.csr.E)).astype(np.uint32)
    util[c.loops] = 0 if loop_cost == "one" else EN.UTIL_MAX
    got = {}
    for csr, looped in c.both():
        ex = c.exports[looped]
        cs, ut = (cost, util) if looped else (cost_bare, util[c.keep])
        want = EN.cost_tables_host(csr, cs, c.ids)
        t = eng.cost_tables(ex, cs, c.ids)
        pc = (host(t[0], np.uint32), host(t[1]), host(t[2]))
        for a, b, what in zip(pc, want, ("pcost", "nh", "nh_port")):
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, looped, what)
        wd = eng.widest_tables(ex, cs, t[0], ut, c.ids)
        wd = (host(wd[0], np.uint32), host(wd[1]), host(wd[2]))
        for a, b, what in zip(wd, EN.widest_tables_host(csr, cs, want[0], ut, c.ids),
                              ("bott", "nh", "nh_port")):
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, looped, what)
        lfa = []
        for link_only in (False, True):
            x = eng.lfa_tables(ex, cs, t[0], c.ids, link_only=link_only)
            x = (host(x[0]), host(x[1]), host(x[2]), x[3])
            for a, b, what in zip(x, EN.lfa_tables_host(csr, cs, want[0], c.ids, link_only),
                                  ("backup", "backup_port", "kind", "counts")):
                assert a.dtype == b.dtype and np.array_equal(a, b), (name, looped, link_only, what)
            assert not (x[0] == c.ids[None, :]).any(), "a switch is its own backup"
            lfa.append(x)
        got[looped] = pc + wd + lfa[0] + lfa[1]
    for a, b in zip(got[True], got[False]):
        assert np.array_equal(a, b), name


# ------------------------------------------------------------------ loads --

@pytest.mark.parametrize("name", GRAPHS)
def test_link_loads_every_layout(eng, name):
    """sdnr_link_loads over the default-route trees as int32 parents, port16
    and slot words (where the rows fit the slot layout), and over next-hop rows
    with SDNR_LOADS_TO_ROOT."""
    c = case(name)
    rows, dsts, w = c.pairs(41)
    po, to, _ = c.dfs
    nh = c.sp[1]
    for layout in (EN.INT32, EN.PORT16, EN.SLOT, "to_root"):
        got = {}
        for csr, looped in c.both():
            if layout == EN.SLOT and csr.max_degree() > 63:
                continue                       # no slot words for a 64-link row
            ex = c.exports[looped]
            if layout == "to_root":
                tree, lay, kw = nh, EN.INT32, {"to_root": True}
            else:
                tree = po if layout == EN.INT32 else EN.pack_host_tree(po, to, csr, layout)
                lay, kw = layout, {}
            want = EN.link_loads_host(csr, tree, lay, rows, dsts, w, **kw)
            got[looped] = eng.link_loads(ex, dev_tree(eng, tree), lay, rows, dsts, w, **kw)
            assert got[looped].dtype == np.uint64 and np.array_equal(got[looped], want), \
                (name, layout, looped)
            assert want.any()
        if len(got) == 2:
            assert loads_equal(c, got[True], got[False], exact=True), (name, layout)
        elif True in got:
            assert not got[True][c.loops].any()


@pytest.mark.parametrize("name", GRAPHS)
def test_ecmp_link_loads_both_splits(eng, name):
    """sdnr_ecmp_link_loads and sdnr_cost_ecmp_link_loads (self-loops at cost 1
    and at the largest cost), route and hop split."""
    c = case(name)
    rows, srcs, w = c.pairs(51)
    dist = c.sp[0]
    for split in SPLITS:
        got = {}
        for csr, looped in c.both():
            want = EN.ecmp_link_loads_host(csr, dist, rows, srcs, w, split)
            got[looped] = eng.ecmp_link_loads(c.exports[looped], dev_dist(eng, dist), rows, srcs,
                                              w, split)
            assert loads_close(got[looped], want), (name, split, looped)
            assert want.any()
        assert loads_equal(c, got[True], got[False], exact=False), (name, split)
        for loop_cost in (1, c.max_cost()):
            cost, cost_bare = c.costs(52, loop_cost)
            got = {}
            for csr, looped in c.both():
                cs = cost if looped else cost_bare
                pc = EN.cost_tables_host(csr, cs, c.ids)[0]
                want = EN.cost_ecmp_link_loads_host(csr, cs, pc, rows, srcs, w, split)
                got[looped] = eng.cost_ecmp_link_loads(c.exports[looped], cs, pc, rows, srcs, w,
                                                       split)
                assert loads_close(got[looped], want), (name, split, loop_cost, looped)
            assert loads_equal(c, got[True], got[False], exact=False), (name, split, loop_cost)


@pytest.mark.parametrize("costed", [False, True])
@pytest.mark.parametrize("name", GRAPHS)
def test_failure_and_whatif_scenarios(eng, name, costed):
    """sdnr_failure_ecmp_link_loads and sdnr_whatif_ecmp_link_loads: a scenario
    that fails or re-costs only self-loop links equals the empty one and loses
    nothing; a mixed scenario equals the one without its self-loop entries, on
    the graph and on the loop-free graph; no peak link is a self-loop."""
    c = case(name)
    rows, srcs, w = c.pairs(61, 2 * c.V)
    cost, cost_bare = c.costs(62, 3) if costed else (None, None)
    real = np.nonzero(c.keep)[0]
    cables = [x for x in cable_edges(c.csr) if c.keep[x].all()]
    pick = [cables[0], cables[len(cables) // 2], cables[-1]]
    loops = c.loops.tolist()
    INF = EN.COST_INF
    for split in SPLITS:
        # failures: [], the self-loops, one of them, cables with and without self-loops beside
        scen = [[], loops, loops[:1]] + [sorted(x + loops) for x in pick] + pick
        bare = [[]] * 3 + [c.to_bare[x].tolist() for x in pick] * 2
        want = EN.failure_ecmp_link_loads_host(c.csr, cost, c.ids, rows, srcs, w, scen, split)
        load, lost, routed = eng.failure_ecmp_link_loads(c.exports[True], cost, c.ids, rows, srcs,
                                                         w, scen, split)
        b_load, b_lost, b_routed = eng.failure_ecmp_link_loads(c.exports[False], cost_bare, c.ids,
                                                               rows, srcs, w, bare, split)
        where = (name, costed, split)
        for k in range(len(scen)):
            assert loads_close(load[k], want[0][k]), where + (k,)
            assert loads_equal(c, load[k], b_load[k], exact=False), where + (k,)
        assert np.array_equal(lost, want[1]) and np.array_equal(lost, b_lost), where
        assert np.array_equal(routed, want[2]) and np.array_equal(routed, b_routed), where
        for k in (1, 2):                       # only self-loops fail: the empty scenario
            assert lost[k] == lost[0] and np.array_equal(routed[k], routed[0]), where + (k,)
            assert loads_close(load[k], load[0]), where + (k,)
        for k in range(3, 6):                  # the self-loop entries change nothing
            assert lost[k] == lost[k + 3] and np.array_equal(routed[k], routed[k + 3])
            assert loads_close(load[k], load[k + 3]), where + (k,)
        # cost overrides: raise, lower or take down the self-loops, alone and beside real links
        hi = c.max_cost()
        some = real[np.random.default_rng(63).choice(real.size, 3, replace=False)].tolist()
        mixed = (some, [7, INF, 2])
        with_loops = (some + loops, [7, INF, 2] + [hi, INF, 1][:len(loops)] +
                      [5] * max(0, len(loops) - 3))
        scen = [([], []), (loops, [hi] * len(loops)), (loops, [INF] * len(loops)),
                (loops[:1], [1]), with_loops, mixed]
        bare = [([], [])] * 4 + [(c.to_bare[some].tolist(), [7, INF, 2])] * 2
        want = EN.whatif_ecmp_link_loads_host(c.csr, cost, c.ids, rows, srcs, w, scen, split)
        got = eng.whatif_ecmp_link_loads(c.exports[True], cost, c.ids, rows, srcs, w, scen, split)
        b_got = eng.whatif_ecmp_link_loads(c.exports[False], cost_bare, c.ids, rows, srcs, w, bare,
                                           split)
        load, lost, routed, peak, peak_edge = got
        for k in range(len(scen)):
            assert loads_close(load[k], want[0][k]), where + ("whatif", k)
            assert loads_equal(c, load[k], b_got[0][k], exact=False), where + ("whatif", k)
            # the peak of the GPU's own plane, bit for bit; never a self-loop link
            assert load[k].max() > 0 and peak[k] == load[k].max(), where + ("whatif", k)
            assert peak_edge[k] == int(load[k].argmax()), where + ("whatif", k)
            assert peak_edge[k] not in loops, where + ("whatif", k)
        assert np.array_equal(lost, want[1]) and np.array_equal(lost, b_got[1]), where
        assert np.array_equal(routed, want[2]) and np.array_equal(routed, b_got[2]), where
        for k in (1, 2, 3):                    # only self-loops change: the empty scenario
            assert lost[k] == lost[0], where + ("whatif", k)
            assert np.array_equal(routed[k], routed[0]), where + ("whatif", k)
            assert loads_close(load[k], load[0]), where + ("whatif", k)
        assert lost[4] == lost[5] and np.array_equal(routed[4], routed[5])
        assert loads_close(load[4], load[5]), where + ("whatif", "mixed")
        # pairs that all have a route: nothing is lost when only self-loops go down
        ok = (srcs >= 0) & (srcs < c.V)
        ok[ok] = c.sp[0][rows[ok], srcs[ok]] != 0xFFFF
        assert ok.sum() > c.V // 2
        r, s, ww = rows[ok], srcs[ok], w[ok]
        lost = eng.failure_ecmp_link_loads(c.exports[True], cost, c.ids, r, s, ww,
                                           [[], loops], split)[1]
        assert lost.tolist() == [0.0, 0.0], where
        lost = eng.whatif_ecmp_link_loads(c.exports[True], cost, c.ids, r, s, ww,
                                          [([], []), (loops, [INF] * len(loops))], split)[1]
        assert lost.tolist() == [0.0, 0.0], where


# --------------------------------------------------------- route expansion --

@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("name", GRAPHS)
def test_route_offsets_and_expand(eng, monkeypatch, name, packed):
    """sdnr_route_offsets and sdnr_route_expand (int32 entries, and one u32
    word per entry) over the default-route trees: every (source, destination)
    pair, the entries of the oracle's tree walk; the same on both graphs."""
    if not packed:
        monkeypatch.setenv("SDNROUTE_ROUTE_PACKED", "0")
    c = case(name)
    V = c.V
    po, to, ho = c.dfs
    rows, dsts = (x.reshape(-1) for x in np.divmod(np.arange(V * V), V))
    last = 200 + (rows + dsts) % 50
    import torch
    tabs = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(eng.dev) for a in (po, to, ho))
    got = {}
    for csr, looped in c.both():
        got[looped] = eng.expand(c.exports[looped], tabs, rows, dsts, last)
    for a, b in zip(got[True], got[False]):
        assert np.array_equal(a, b), name
    off, sw, hp = got[True]
    assert off[0] == 0 and off.dtype == np.int64
    for i in range(V * V):
        s, d = int(rows[i]), int(dsts[i])
        path = EN.tree_path(po[s], s, d)
        ports = [int(to[s, v]) for v in path[1:]] + [int(last[i])] if path else []
        assert sw[off[i]:off[i + 1]].tolist() == path, (name, s, d)
        assert hp[off[i]:off[i + 1]].tolist() == ports, (name, s, d)
