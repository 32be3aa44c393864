"""Three entry points that were reached only through larger paths, alone on a
gfx950 device:

* sdnr_tree_pack (dfs_pack_kernel, dfs_slot_pack_kernel) against
  engine.pack_host_tree and against the words sdnr_dfs_tables_tree writes;
* sdnr_edge_ports (edge_port_kernel) against the reference's loop over every
  link (test_event_replay.ref_is_edge);
* sdnr_ecmp_routes (ecmp_unrank_kernel) against the enumeration of every
  shortest route (engine.shortest_paths_lex) and, where the set is too large to
  enumerate, against an unranking over exact Python-int route counts.

All results are integers and compared exactly."""
import ctypes
import types

import numpy as np
import pytest
import torch

import golden_util as G
from oracle import oracle as O
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.objects import Link, Port
from sdnmpi_amd.topologies import CSR
from test_event_replay import ref_is_edge
from test_self_loops_gpu import case, csr_from_rows

pytestmark = pytest.mark.gpu

INVAL = -22
NONE = 0xFFFFFFFF
U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def drop_route_cases():
    """The expected routes of the ladder are some hundred MB: free them when
    the module is done."""
    yield
    _route_cases.clear()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


# ---------------------------------------------------------- sdnr_tree_pack --

PACK_GRAPHS = list(G.LOOPS) + ["hub32", "hub63_leaf_loops", "hub65_leaf_loops"]
GUARD = 0x5A5A5A5A


def pack(ctx, parent, port, n, layout):
    """sdnr_tree_pack of the first n entries into a buffer with 8 guard words
    behind them; returns the n words (the guard words must be untouched)."""
    out = torch.full((n + 8,), GUARD, dtype=torch.int32, device=parent.device)
    torch.cuda.synchronize()
    ctx.tree_pack_device(parent.data_ptr(), port.data_ptr() if port is not None else 0, n,
                         out.data_ptr(), layout)
    ctx.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[n:] == GUARD).all(), "wrote past n entries"
    return got[:n]


@pytest.mark.parametrize("name", PACK_GRAPHS)
def test_tree_pack_both_layouts(ctx, name):
    """The int32 tables of every source, packed whole and in prefixes of 1,
    255, 256 and 257 entries: pack_host_tree's words, and the words the DFS
    kernels write themselves.  Unreachable entries pack to 0xFFFFFFFF, the root
    to port 0xFFFF / slot 63; a row's self-loop entry shifts the slots behind
    it."""
    c = case(name)
    csr, V = c.csr, c.V
    po, to, _ = c.dfs
    ctx.upload(csr)
    parent, port = dev(po.reshape(-1)), dev(to.reshape(-1))
    sizes = [n for n in (1, 255, 256, 257) if n <= V * V] + [V * V]
    layouts = [(_native.TREE_PORT16, EN.PORT16)]
    if csr.max_degree() <= 63:
        layouts.append((_native.TREE_SLOT, EN.SLOT))
    for lay, host_lay in layouts:
        want = np.asarray(EN.pack_host_tree(po, to, csr, host_lay)).view(np.uint32).reshape(-1)
        unreached, root = want == NONE, np.arange(V * V) // V == np.arange(V * V) % V
        assert not unreached[root].any()
        if name not in ("fat_tree_k4_loops", "torus_2x2x2_loops"):      # the connected ones
            assert unreached.any()
        if lay == _native.TREE_PORT16:
            assert ((want[root] >> 16) == 0xFFFF).all() and ((want[root] & 0xFFFF) ==
                                                             np.arange(V)).all()
        else:
            assert ((want[root] >> 26) == 63).all()
            assert ((want[~unreached & ~root] >> 26) < 63).all()
        for n in sizes:
            got = pack(ctx, parent, port, n, lay)
            assert np.array_equal(got, want[:n]), (name, host_lay, n)
        if lay == _native.TREE_SLOT:               # the slot layout reads no port table
            assert np.array_equal(pack(ctx, parent, None, V * V, lay), want)
        tree, _ = ctx.dfs_tables_tree(c.ids, lay, 2)
        assert np.array_equal(tree.reshape(-1), want), (name, host_lay)
    if name.endswith("leaf_loops"):
        # a leaf's row is (hub, leaf, neighbour): the neighbour sits in slot 2, not 1
        if csr.max_degree() <= 63:
            slot = want.reshape(V, V) >> 26
            assert slot[1, 2] == 2 and (want.reshape(V, V)[1, 2] & 0x3FFFFFF) == 1


def test_tree_pack_refusals(ctx):
    c = case("hub64")
    po, to, _ = c.dfs
    parent, port = dev(po.reshape(-1)), dev(to.reshape(-1))
    out = torch.empty_like(parent)
    n = parent.numel()
    ctx.upload(c.csr)                              # a 64-link row: no slot words
    with pytest.raises(_native.SdnrError) as ei:
        ctx.tree_pack_device(parent.data_ptr(), 0, n, out.data_ptr(), _native.TREE_SLOT)
    assert ei.value.code == INVAL and "63" in str(ei.value)
    pack(ctx, parent, port, n, _native.TREE_PORT16)            # the other layout is taken
    with pytest.raises(_native.SdnrError) as ei:               # no layout 0 / 3
        ctx.tree_pack_device(parent.data_ptr(), port.data_ptr(), n, out.data_ptr(), 3)
    assert ei.value.code == INVAL
    with pytest.raises(_native.SdnrError) as ei:               # port16 without a port table
        ctx.tree_pack_device(parent.data_ptr(), 0, n, out.data_ptr(), _native.TREE_PORT16)
    assert ei.value.code == INVAL
    # a 17-bit port: no port16 words, slot words as ever
    wide = CSR(c.bare.dpids, c.bare.row_ptr, c.bare.col,
               np.where(np.arange(c.bare.E) == 5, 0x10000, c.bare.port))
    ctx.upload(wide)
    with pytest.raises(_native.SdnrError) as ei:
        ctx.tree_pack_device(parent.data_ptr(), port.data_ptr(), n, out.data_ptr(),
                             _native.TREE_PORT16)
    assert ei.value.code == INVAL and "port16" in str(ei.value)
    want = np.asarray(EN.pack_host_tree(po, to, wide, EN.SLOT)).view(np.uint32).reshape(-1)
    assert np.array_equal(pack(ctx, parent, None, n, _native.TREE_SLOT), want)
    # host pointers are refused before anything is read
    hp, ht, ho = po.reshape(-1).copy(), to.reshape(-1).copy(), np.zeros(n, np.uint32)
    rc = ctx._lib.sdnr_tree_pack(ctx._h, hp.ctypes.data_as(ctypes.c_void_p),
                                 ht.ctypes.data_as(ctypes.c_void_p), n,
                                 ho.ctypes.data_as(ctypes.c_void_p), _native.TREE_SLOT, 0)
    assert rc == INVAL and not ho.any()


# --------------------------------------------------------- sdnr_edge_ports --

def key(d, p):
    return (d << 32) | (p & 0xFFFFFFFF)


def links_db(links):
    """The reference's links dict for (u, pu, v, pv) tuples."""
    db = types.SimpleNamespace(links={})
    for u, pu, v, pv in links:
        db.links.setdefault(u, {})[v] = Link(Port(u, pu), Port(v, pv))
    return db


def ends_of(db):
    return np.array(sorted(set(key(p.dpid, p.port_no) for nb in db.links.values()
                               for lk in nb.values() for p in (lk.src, lk.dst))), np.uint64)


def edge_ports_case():
    """Links over the switches 0 .. 39 with ports up to 2^32 - 1: ordinary
    ones, a self-loop (both ends on switch 7), switches 0 / 1 and 2^31 - 1 whose
    keys differ only in the high word, ports 5 / 6 and 2^32 - 1 that differ
    only in the low one."""
    rng = np.random.default_rng(71)
    links = [(7, 70, 7, 71), (0, 5, 1, 5), (1, 6, 0, 6), ((1 << 31) - 1, 5, 3, 0xFFFFFFFF),
             (3, 1, (1 << 31) - 1, 0xFFFFFFFF)]
    for _ in range(60):
        u, v = (int(x) for x in rng.choice(40, 2, replace=False))
        links.append((u, int(rng.integers(1, 300)), v, int(rng.integers(1, 300))))
    return links_db(links)


def queries(db, n, seed):
    """n ports: link ends, the same port on another switch, another port on
    the same switch, and ports of switches without links."""
    rng = np.random.default_rng(seed)
    ends = [(p.dpid, p.port_no) for nb in db.links.values() for lk in nb.values()
            for p in (lk.src, lk.dst)]
    out = []
    for i in range(n):
        d, p = ends[int(rng.integers(len(ends)))]
        k = i % 4
        out.append([(d, p), (d + 1, p), (d, p + 1), (int(rng.integers(40, 50)), p)][k])
    return [Port(d, p) for d, p in out]


NAMED_PORTS = [Port(7, 70), Port(7, 71), Port(7, 72), Port(0, 5), Port(1, 5), Port(2, 5),
               Port(0, 6), Port(1, 6), Port(0, 7), Port((1 << 31) - 1, 5),
               Port((1 << 31) - 1, 0xFFFFFFFF), Port(3, 0xFFFFFFFF), Port(3, 0xFFFFFFFE),
               Port(0, 0xFFFFFFFF)]


@pytest.mark.parametrize("nports", [0, 1, 255, 256, 257])
def test_edge_ports_against_the_reference_loop(ctx, nports):
    db = edge_ports_case()
    ends = ends_of(db)
    # first the named keys: the self-loop's two ends, the high-word and low-word neighbours
    ports = (NAMED_PORTS + queries(db, nports, 72 + nports))[:nports]
    keys = np.array([key(p.dpid, p.port_no) for p in ports], np.uint64)
    want = np.array([ref_is_edge(db, p) for p in ports], bool)
    got = ctx.edge_ports(ends, keys)
    assert got.dtype == bool and np.array_equal(got, want), nports
    if nports:
        assert ctx.last_kernel() == "edge_port_kernel"
    if nports >= 255:
        assert want.any() and not want.all()
    # the same ends with every key twice: the answers do not change
    assert np.array_equal(ctx.edge_ports(np.repeat(ends, 2), keys), want)
    # no link at all: every port floods
    assert ctx.edge_ports(np.zeros(0, np.uint64), keys).all()


def test_edge_ports_self_loop_and_unsorted_ends(ctx):
    """A self-loop link puts two ends on one switch: both are link ends, the
    switch's other ports are not.  Unsorted ends from host buffers are refused."""
    db = links_db([(4, 70, 4, 71)])
    ends = ends_of(db)
    assert ends.tolist() == [key(4, 70), key(4, 71)]
    ports = [Port(4, 69), Port(4, 70), Port(4, 71), Port(4, 72), Port(3, 70), Port(5, 71)]
    keys = np.array([key(p.dpid, p.port_no) for p in ports], np.uint64)
    want = [ref_is_edge(db, p) for p in ports]
    assert want == [True, False, False, True, True, True]
    assert ctx.edge_ports(ends, keys).tolist() == want
    with pytest.raises(_native.SdnrError) as ei:
        ctx.edge_ports(ends[::-1].copy(), keys)
    assert ei.value.code == INVAL and "sorted" in str(ei.value)
    big = ends_of(edge_ports_case())
    swapped = big.copy()
    swapped[[-2, -1]] = swapped[[-1, -2]]           # only the last two out of order
    with pytest.raises(_native.SdnrError) as ei:
        ctx.edge_ports(swapped, keys)
    assert ei.value.code == INVAL


# -------------------------------------------------------- sdnr_ecmp_routes --

def ladder(R):
    """R rungs of two vertices (2 i, 2 i + 1), each joined to both vertices of
    the next rung: 2^(k - 1) shortest routes between vertices k rungs apart."""
    nb = [[] for _ in range(2 * R)]
    for i in range(R - 1):
        for a in (2 * i, 2 * i + 1):
            for b in (2 * i + 2, 2 * i + 3):
                nb[a].append(b)
                nb[b].append(a)
    return csr_from_rows([sorted(x) for x in nb])


def exact_counts(csr, dist):
    """counts[d][x]: the number of shortest x -> d routes as Python ints (no
    saturation), by the level DP over the dist rows."""
    D, V = dist.shape
    rp, col = csr.row_ptr.tolist(), csr.col.tolist()
    out = []
    for r in range(D):
        dr = dist[r].tolist()
        cnt = [0] * V
        for x in sorted(range(V), key=lambda v: dr[v]):
            if dr[x] == 0xFFFF:
                break
            cnt[x] = 1 if dr[x] == 0 else sum(cnt[col[e]] for e in range(rp[x], rp[x + 1])
                                              if dr[col[e]] == dr[x] - 1)
        out.append(cnt)
    return out


def clipped(counts):
    return np.array([[min(c, U64_MAX) for c in row] for row in counts], np.uint64)


class Unranker(object):
    """Lexicographic unranking over exact route counts, all queries at once,
    one hop per pass.  Per (row d, vertex x): ``hop[d, x, k]`` the k-th
    ascending out-neighbour of x one hop closer to d, ``cum[d, x, k]`` the
    number of routes through the first k + 1 of them.

    The sums are Python ints, clipped to 2^64 - 1 only for the comparison.
    That is exact for every rank <= 2^64 - 2: such a rank is >= an exact sum c
    iff it is >= min(c, 2^64 - 1), and a sum is subtracted only when it is <=
    the rank, so it and the difference fit in 64 bits.  Rank 2^64 - 1 is below
    no clipped count: a row of -1."""

    def __init__(self, csr, dist, counts):
        D, V = dist.shape
        rp, col = csr.row_ptr.tolist(), csr.col.tolist()
        hops = {}
        for d in range(D):
            dr, cnt = dist[d].tolist(), counts[d]
            for x in range(V):
                if dr[x] in (0, 0xFFFF):
                    continue
                nh = [col[e] for e in range(rp[x], rp[x + 1]) if dr[col[e]] == dr[x] - 1]
                assert sum(cnt[n] for n in nh) == cnt[x]
                hops[d * V + x] = nh
        K = max([1] + [len(nh) for nh in hops.values()])
        self.V, self.K = V, K
        self.dist = dist.astype(np.int64).reshape(-1)
        self.total = clipped(counts).reshape(-1)
        self.hop = np.full((D * V, K), -1, np.int32)
        self.cum = np.full((D * V, K), U64_MAX, np.uint64)      # padding: never skipped
        for at, nh in hops.items():
            acc = 0
            for k, n in enumerate(nh):
                acc += counts[at // V][n]
                self.hop[at, k], self.cum[at, k] = n, min(acc, U64_MAX)
        self.hop_flat = self.hop.reshape(-1)
        self.cum_cols = [np.ascontiguousarray(self.cum[:, k]) for k in range(K)]

    def routes(self, rows, srcs, ranks, max_len):
        """int32 [n, max_len] as sdnr_ecmp_routes lays the routes out."""
        n = len(rows)
        out = np.full((max_len, n), -1, np.int32)              # hop-major while it is filled
        base = np.asarray(rows, np.int64) * self.V
        x = np.asarray(srcs, np.int64).copy()
        r = np.asarray(ranks, np.uint64).copy()
        dx = self.dist[base + x]
        live = (dx != 0xFFFF) & (r < self.total[base + x]) & (dx + 1 <= max_len)
        out[0, live] = x[live]
        dx[~live] = 0
        j = 0
        while True:
            idx = np.nonzero(dx > 0)[0]
            if not idx.size:
                return np.ascontiguousarray(out.T)
            whole = idx.size == n                                # no gather when all walk on
            at = base + x if whole else base[idx] + x[idx]
            ri = r if whole else r[idx]
            k = np.zeros(idx.size, np.int64)                    # next hops skipped whole
            sub = np.zeros(idx.size, np.uint64)                 # ... and the routes through them
            for col in self.cum_cols:                           # ascending sums: a prefix is skipped
                c = col[at]
                ge = ri >= c
                k += ge
                sub = np.where(ge, c, sub)
            ri = ri - sub
            nxt = self.hop_flat[at * self.K + k]
            assert (nxt >= 0).all()
            j += 1
            if whole:
                r, x = ri, nxt.astype(np.int64)
                dx -= 1
                out[j] = nxt
            else:
                r[idx], x[idx] = ri, nxt
                dx[idx] -= 1
                out[j, idx] = nxt


def unrank_host(csr, dist, counts, rows, srcs, ranks, max_len):
    return Unranker(csr, dist, counts).routes(rows, srcs, ranks, max_len)


def rank_samples(count, rng):
    """Every rank of a set of at most 4,096 routes; of a larger one the first
    64, the last 64 expressible (up to 2^64 - 2) and 64 random ones between."""
    if count <= 4096:
        return np.arange(count, dtype=np.uint64)
    top = min(count, U64_MAX)                 # ranks are below this
    mid = rng.integers(64, top - 64, 64, dtype=np.uint64)
    return np.concatenate([np.arange(64, dtype=np.uint64),
                           np.arange(top - 64, top, dtype=np.uint64), mid])


ROUTE_GRAPHS = list(G.LOOPS) + ["fat_tree:4", "ladder70"]
_route_cases = {}


def route_case(name):
    """(csr, dist rows of every destination, exact counts, the queries grouped
    by route length with their expected rows), computed once."""
    if name in _route_cases:
        return _route_cases[name]
    if name in G.LOOPS:
        csr = case(name).csr
    elif name == "ladder70":
        csr = ladder(70)
    else:
        csr = T.by_name(name).csr()
    V = int(csr.V)
    dist = O.dest_tables(csr, np.arange(V, dtype=np.int32))[0]
    counts = exact_counts(csr, dist)
    rng = np.random.default_rng(81)
    groups = {}
    for d in range(V):
        for s in range(V):
            c = counts[d][s]
            if c == 0:
                continue
            rk = rank_samples(c, rng)
            g = groups.setdefault(int(dist[d, s]), ([], [], []))
            g[0].append(np.full(rk.size, d, np.int32))
            g[1].append(np.full(rk.size, s, np.int32))
            g[2].append(rk)
    out, un = {}, Unranker(csr, dist, counts)
    for L, (r, s, k) in groups.items():
        r, s, k = np.concatenate(r), np.concatenate(s), np.concatenate(k)
        out[L] = (r, s, k, un.routes(r, s, k, L + 1))
    _route_cases[name] = (csr, dist, counts, out)
    return _route_cases[name]


@pytest.mark.parametrize("counter", ["default", "global"])
@pytest.mark.parametrize("name", ROUTE_GRAPHS)
def test_ecmp_routes_every_rank(ctx, monkeypatch, name, counter):
    """Every rank of every (source, destination) pair (rank_samples where a
    set is large), the counts from sdnr_ecmp_counts -- saturated on the ladder
    -- in its default and its global-memory form."""
    if counter == "global":
        monkeypatch.setenv("SDNROUTE_ECMP", "global")
    csr, dist, counts, groups = route_case(name)
    V = int(csr.V)
    ctx.upload(csr)
    paths = ctx.ecmp_counts(dist)
    if counter == "global":
        assert ctx.last_kernel() == "ecmp_count_global_kernel"
    want = clipped(counts)
    assert paths.dtype == np.uint64 and np.array_equal(paths, want)
    total = 0
    for L, (rows, srcs, ranks, expect) in sorted(groups.items()):
        got = ctx.ecmp_routes(dist, paths, rows, srcs, ranks, L + 1)
        assert np.array_equal(got, expect), (name, L)
        assert (got[:, 0] == srcs).all() and (got[:, L] == rows).all()
        total += len(rows)
    if name == "ladder70":
        assert int(paths[V - 1, 0]) == U64_MAX and counts[V - 1][0] == 1 << 68
        assert total > 1_000_000
    else:
        # enumerable: the lexicographic list itself
        rp, col = csr.row_ptr, csr.col
        for L, (rows, srcs, ranks, expect) in groups.items():
            at = 0
            while at < len(rows):
                d, s = int(rows[at]), int(srcs[at])
                routes = EN.shortest_paths_lex(rp, col, dist[d], s, d)
                assert len(routes) == counts[d][s]
                assert expect[at:at + len(routes)].tolist() == routes, (name, d, s)
                at += len(routes)


def test_ecmp_routes_out_of_range_ranks_and_lengths(ctx):
    """rank == count, a buffer one entry too short, a longer one, an
    unreachable source, on a fixture; on the ladder rank 2^64 - 2 of a
    saturated set is a route and rank 2^64 - 1 is none."""
    csr, dist, counts, _ = route_case("random_V12_loops")
    V = int(csr.V)
    ctx.upload(csr)
    paths = ctx.ecmp_counts(dist)
    pairs = [(d, s) for d in range(V) for s in range(V)]
    rows = np.array([d for d, _ in pairs], np.int32)
    srcs = np.array([s for _, s in pairs], np.int32)
    cnt = np.array([counts[d][s] for d, s in pairs], np.uint64)
    dd = dist[rows, srcs].astype(np.int64)
    reach = dd != 0xFFFF
    assert reach.any() and (~reach).any() and (cnt[reach] > 0).all() and not cnt[~reach].any()
    L = int(dd[reach].max()) + 1
    got = ctx.ecmp_routes(dist, paths, rows, srcs, cnt, L)               # rank == count
    assert (got == -1).all()
    first = ctx.ecmp_routes(dist, paths, rows, srcs, np.zeros(len(pairs), np.uint64), L + 3)
    assert (first[~reach] == -1).all()                                   # unreachable source
    want = unrank_host(csr, dist, counts, rows, srcs, np.zeros(len(pairs), np.uint64), L + 3)
    assert np.array_equal(first, want)
    for i in np.nonzero(reach)[0]:
        assert (first[i, :dd[i] + 1] >= 0).all() and (first[i, dd[i] + 1:] == -1).all()
    for length in sorted(set(dd[reach].tolist()) - {0}):
        sel = reach & (dd == length)
        short = ctx.ecmp_routes(dist, paths, rows[sel], srcs[sel],
                                np.zeros(int(sel.sum()), np.uint64), length)
        assert (short == -1).all(), length                               # max_len == dist
        fits = ctx.ecmp_routes(dist, paths, rows[sel], srcs[sel],
                               np.zeros(int(sel.sum()), np.uint64), length + 1)
        assert np.array_equal(fits, first[sel, :length + 1])
    csr, dist, counts, _ = route_case("ladder70")
    V = int(csr.V)
    ctx.upload(csr)
    paths = ctx.ecmp_counts(dist)
    rows = np.full(4, V - 1, np.int32)
    srcs = np.zeros(4, np.int32)
    ranks = np.array([0, U64_MAX - 1, U64_MAX, 1 << 63], np.uint64)
    got = ctx.ecmp_routes(dist, paths, rows, srcs, ranks, 70)
    assert np.array_equal(got, unrank_host(csr, dist, counts, rows, srcs, ranks, 70))
    assert (got[2] == -1).all() and (got[[0, 1, 3]] >= 0).all()
    # the 68 two-way choices of a route are the bits of its rank, first rung first, a set bit
    # the odd vertex: 2^64 - 2 is 0000, 63 ones, 0
    assert (got[1] % 2).tolist() == [0] + [0] * 4 + [1] * 63 + [0] + [1]
    assert (got[1] // 2).tolist() == list(range(70))
