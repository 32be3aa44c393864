"""Inputs with more units of work than a row-persistent kernel launches
workgroups, for test_over_grid.py and test_rows_over_grid_gpu.py.  A plain
helper module like boundary_graphs.

Every kernel of loads.hip, ecmp_loads.hip, cost_ecmp_loads.hip,
cost_tables.hip, widest_tables.hip, failure_loads.hip, whatif_loads.hip,
lfa_tables.hip, fair_rates.hip, ecmp_fair_rates.hip, multicast.hip and the
counts of ecmp.hip gives workgroup b the units b, b + grid, b + 2 grid, ...
(rows, batches of destinations, scenario x row items, groups) and keeps a
unit's state in LDS or in a scratch slice that the next unit reuses.  The
builders here make unit lists in which

  * consecutive units of one workgroup differ: unit u and unit u - s never
    have the same destination (root, batch), for every stride s they are
    given -- the candidates for the grid;
  * every kind of unit that a kernel skips early sits between two working
    units, u - s and u + s, for every such stride.

graph()   the 44-vertex test graph: test_link_loads.random_csr(40, 30, 3) -- 32
          connected vertices and 8 without a link -- and, as a second
          component, the 4-switch "mock" fabric of golden_util.SMALL.  A
          destination drawn over all its vertices reaches 32, 4 or 1 of them.
"""
import types

import numpy as np

import golden_util as G
from sdnmpi_amd import topologies as T
from test_link_loads import random_csr

WORK, EMPTY, BAD_DST, ERR_OFF, ERR_ROW = 0, 1, 2, 3, 4
KIND_NAMES = ("work", "empty", "bad_dst", "err_off", "err_row")
P_EMPTY, P_BAD_DST, P_ERROR = 0.15, 0.05, 0.02


def units(cus, mult=4):
    """Units for a grid of cus * mult workgroups: half of them take three,
    the others two."""
    return 2 * cus * mult + cus * mult // 2


def strides_for(cus, n):
    """The grids the covered launches may take on ``cus`` compute units, as
    strides that leave room for u - s and u + s among n units."""
    return tuple(cus * m for m in (1, 2, 4, 8) if 2 * cus * m < n)


_graph = []


def graph():
    """(csr, comp): the test graph and the component label of every vertex."""
    if not _graph:
        a = random_csr(40, 30, 3)
        b = G.Golden(G.SMALL[0]).fabric().csr()
        src, dst, port = [], [], []
        for c, base in ((a, 1), (b, 1 + a.V)):
            src.append(np.repeat(np.arange(c.V), np.diff(c.row_ptr)) + base)
            dst.append(np.asarray(c.col, np.int64) + base)
            port.append(np.asarray(c.port, np.int64))
        V = a.V + b.V
        csr = T.build_csr(np.concatenate(src), np.concatenate(dst), np.concatenate(port),
                          extra_vertices=list(range(1, V + 1)))
        _graph.append((csr, components(csr)))
    return _graph[0]


def components(csr):
    """comp[v]: the smallest vertex of v's component (links taken both ways)."""
    V = int(csr.V)
    comp = np.arange(V)
    u = np.repeat(np.arange(V), np.diff(csr.row_ptr))
    v = np.asarray(csr.col, np.int64)
    for _ in range(V):
        low = np.minimum(comp[u], comp[v])
        new = comp.copy()
        np.minimum.at(new, u, low)
        np.minimum.at(new, v, low)
        if np.array_equal(new, comp):
            break
        comp = new
    return comp


def rand_weights(rng, n):
    """u64 weights below 2^32, about 30 % zeros (the loads modules' own)."""
    w = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    w[rng.random(n) < 0.3] = 0
    return w


def sandwiched(kind, stride):
    """The kinds other than WORK that have a unit u with WORK units at
    u - stride and u + stride."""
    kind = np.asarray(kind)
    n, s = kind.shape[0], int(stride)
    if 2 * s >= n:
        return set()
    mid = kind[s:n - s]
    ok = (kind[:n - 2 * s] == WORK) & (kind[2 * s:] == WORK) & (mid != WORK)
    return set(mid[ok].tolist())


def check_units(kind, key, grid):
    """What makes a run over ``grid`` workgroups mean something: more than
    two units for some workgroup, every skipped kind present between two
    working units of one workgroup, and no two consecutive units of a
    workgroup with the same key (destination, root, batch)."""
    kind = np.asarray(kind)
    n, g = kind.shape[0], int(grid)
    assert n >= 2 * g + 1, (n, g)
    want = set(kind.tolist()) - {WORK}
    assert sandwiched(kind, g) == want, (sandwiched(kind, g), want)
    key = np.asarray(key)
    key = key.reshape(n, -1)
    assert not (key[g:] == key[:-g]).all(axis=1).any()


def _kinds(rng, n, strides, probs):
    """Random kinds with the given probabilities, then every kind planted
    between two working units at every stride."""
    kind = np.full(n, WORK)
    x = rng.random(n)
    lo = 0.0
    for k, p in probs:
        kind[(x >= lo) & (x < lo + p)] = k
        lo += p
    for j, s in enumerate(strides):
        for i, (k, _) in enumerate(probs):
            c = 1 + 2 * i + 16 * j
            assert c + 1 < min(strides) and 2 * s + c < n
            kind[[c, 2 * s + c]] = WORK
            kind[s + c] = k
    for s in strides:
        assert sandwiched(kind, s) >= {k for k, _ in probs}
    return kind


def _pair_errors(kind, strides):
    """An ERR_OFF row r takes row r + 1 with it (``bad_offsets``): keep those
    whose follower is a WORK or EMPTY row.  Returns the kinds in effect, the
    followers marked ERR_OFF too; every stride still has its sandwich."""
    n = kind.shape[0]
    at = np.nonzero(kind == ERR_OFF)[0]
    kind[at] = WORK
    at = [r for r in at.tolist() if r + 1 < n and kind[r + 1] in (WORK, EMPTY)]
    kind[at] = ERR_OFF
    eff = kind.copy()
    eff[np.asarray(at, np.int64) + 1] = ERR_OFF
    for s in strides:
        assert sandwiched(eff, s) >= set(kind.tolist()) - {WORK}, s
    return eff


def _distinct_draw(rng, n, V, strides):
    """n vertices in [0, V), unit u different from every unit u - s."""
    out = np.empty(n, np.int64)
    for u in range(n):
        while True:
            out[u] = rng.integers(0, V)
            if all(u < s or out[u - s] != out[u] for s in strides):
                break
    return out


def _other_component(rng, comp, d):
    other = np.nonzero(comp != comp[d])[0]
    return int(rng.choice(other))


def row_mix(csr, comp, n, seed, strides, bad_dst=False, errors=False, distinct=None):
    """n rows for the kernels that take one destination (or tree root) per row
    and a list of pairs grouped by row.

    kind [n]   WORK; EMPTY (about 15 %: no pair); with ``bad_dst`` BAD_DST
               (about 5 %: dst is -1 or >= V, the row still has pairs); with
               ``errors`` ERR_OFF and ERR_ROW (about 1 % each, with pairs; the
               caller makes them data errors: offsets outside the pair list --
               they come as two rows, see ``bad_offsets`` -- or a table row the
               kernel rejects)
    dst [n]    the row's destination or root over all vertices, != dst[r - s]
               for the strides s (``distinct``: for those instead -- the item
               kernels fold the grid into the rows of a scenario)
    rows, ends, w   the pairs: 1 to 5 per row with pairs, the row index, the
               other end (a source, or a destination in the row's tree) and a
               u64 weight below 2^32, 30 % zeros.  Of the ends about a tenth
               each is the row's own dst, an id outside [0, V), a vertex of
               another component; the others are drawn over all vertices."""
    rng = np.random.default_rng(seed)
    V = int(csr.V)
    probs = [(EMPTY, P_EMPTY)]
    if bad_dst:
        probs.append((BAD_DST, P_BAD_DST))
    if errors:
        probs += [(ERR_OFF, P_ERROR / 2), (ERR_ROW, P_ERROR / 2)]
    kind = _kinds(rng, n, strides, probs)
    eff = _pair_errors(kind, strides) if errors else kind
    dst = _distinct_draw(rng, n, V, strides if distinct is None else distinct)
    key = dst.copy()
    rows, ends = [], []
    for r in range(n):
        if kind[r] == EMPTY:
            continue
        d = int(dst[r])
        for _ in range(int(rng.integers(1, 6))):
            x = rng.random()
            if x < 0.1:
                e = d
            elif x < 0.2:
                e = int(rng.choice([-1, V, V + 7]))
            elif x < 0.3:
                e = _other_component(rng, comp, d)
            else:
                e = int(rng.integers(0, V))
            rows.append(r)
            ends.append(e)
    bad = np.nonzero(kind == BAD_DST)[0]
    dst[bad] = rng.choice([-1, V, V + 7], bad.shape[0])
    rows, ends = np.asarray(rows, np.int64), np.asarray(ends, np.int64)
    return types.SimpleNamespace(n=n, kind=kind, effective=eff, dst=dst, key=key, rows=rows,
                                 ends=ends, w=rand_weights(rng, rows.shape[0]))


def pair_offsets(mix):
    """int64 [n + 1]: the offsets of each row's pairs (they are in row order)."""
    off = np.zeros(mix.n + 1, np.int64)
    np.cumsum(np.bincount(mix.rows, minlength=mix.n), out=off[1:])
    return off


def break_offsets(off, kind):
    """Offsets [n + 1] with every ERR_OFF unit r broken: off[r + 1] lies past
    the end of the list, so unit r ends outside it and unit r + 1 starts after
    its own end -- both are rejected, whatever unit r + 1 was, and their
    entries are nobody's.  Returns (off, dead): dead [n] marks the units that
    count for nothing (those two, and every ERR_ROW unit)."""
    off = np.array(off, np.int64)
    n = off.shape[0] - 1
    dead = np.zeros(n, bool)
    for r in np.nonzero(kind == ERR_OFF)[0].tolist():
        off[r + 1] = off[-1] + 7
        dead[[r, r + 1]] = True
    dead |= kind == ERR_ROW
    return off, dead


def bad_offsets(mix):
    """``break_offsets`` of a row mix: (off, live), live [npairs] marking the
    pairs that still count."""
    off, dead = break_offsets(pair_offsets(mix), mix.kind)
    return off, ~dead[mix.rows]


def dest_mix(csr, nbatch, B, seed, strides, p_bad=0.01):
    """Destinations for ``nbatch`` batches of B (cost_tables.hip,
    widest_tables.hip; B = 1: the rows of lfa_tables.hip), their number no
    multiple of B: about 5 % are -1 or >= V, batch b differs from every batch
    b - s, and whole batches of ids that are no vertex (kind BAD_DST, a share
    ``p_bad``) sit between working batches.  Returns (dsts, kind [nbatch])."""
    rng = np.random.default_rng(seed)
    V = int(csr.V)
    ndst = nbatch * B - (B // 2 + 1 if B > 1 else 0)
    kind = _kinds(rng, nbatch, strides, [(BAD_DST, p_bad)])
    kind[-1] = WORK
    d = rng.integers(0, V, nbatch * B)
    flip = rng.random(nbatch * B) < P_BAD_DST
    flip[0::B] = False                                     # a working batch has a vertex
    d[flip] = rng.choice([-1, V, V + 7], int(flip.sum()))
    d = d.reshape(nbatch, B)
    d[:, 0] = _distinct_draw(rng, nbatch, V, strides)
    for b in np.nonzero(kind == BAD_DST)[0].tolist():      # (in order: b - s is final)
        d[b] = rng.choice([-1, V], B)
        taken = [int(d[b - s, 0]) for s in strides if b >= s]
        d[b, 0] = [x for x in (-1, V, V + 7, -5, V + 1) if x not in taken][0]
    return d.reshape(-1)[:ndst].copy(), kind


def batch_keys(dsts, B):
    """[nbatch][B]: the batches of a destination list, the last one padded."""
    nb = (dsts.shape[0] + B - 1) // B
    out = np.full(nb * B, -9, np.int64)
    out[:dsts.shape[0]] = dsts
    return out.reshape(nb, B)


def failure_scenarios(csr, victim):
    """Four failure scenarios as lists of CSR edge ids: none, one cable (both
    directions), every link of one switch, and every link into ``victim`` --
    rows toward it lose every pair."""
    u = np.repeat(np.arange(int(csr.V)), np.diff(csr.row_ptr))
    v = np.asarray(csr.col, np.int64)
    a, b = int(u[0]), int(v[0])
    cable = np.nonzero(((u == a) & (v == b)) | ((u == b) & (v == a)))[0]
    hub = int(np.argmax(np.diff(csr.row_ptr)))
    switch = np.nonzero((u == hub) | (v == hub))[0]
    cut = np.nonzero(v == victim)[0]
    assert cable.size == 2 and switch.size and cut.size
    return [[], cable.tolist(), switch.tolist(), cut.tolist()]


def group_mix(csr, comp, n, seed, strides, errors=False, to_root=False, pool=None):
    """n multicast groups over the tree rows of every vertex (row v = the tree
    of root v; ``to_root``: the next-hop row of destination v, and a member's
    row is its own; ``pool``: next-hop rows of these destinations only, the
    members are drawn among them -- 1 to 6, the first again and an id outside
    [0, V), ``comp`` is not used): kind WORK, EMPTY (no member), BAD_DST (the
    root is no vertex)
    and, with ``errors``, ERR_OFF / ERR_ROW as in ``row_mix``.  The members of
    a group: 1 to 6 vertices over all of the graph, then the first of them
    again, the root itself, a vertex of another component and an id outside
    [0, V); one member in nine names a row outside the table.  Returns the
    mix with root, mem_off, mem_row, mem_vertex, w (u64 per group, whole
    range) and key."""
    rng = np.random.default_rng(seed)
    V = int(csr.V)
    probs = [(EMPTY, P_EMPTY), (BAD_DST, P_BAD_DST)]
    if errors:
        probs += [(ERR_OFF, P_ERROR / 2), (ERR_ROW, P_ERROR / 2)]
    kind = _kinds(rng, n, strides, probs)
    eff = _pair_errors(kind, strides) if errors else kind
    root = _distinct_draw(rng, n, V, strides)
    key = root.copy()
    off, row, vert = [0], [], []
    for g in range(n):
        r = int(root[g])
        if kind[g] != EMPTY:
            if pool is not None:                           # (row i: toward pool[i])
                at = rng.integers(0, len(pool), int(rng.integers(1, 7))).tolist()
                at += [at[0], at[-1]]
                ms = [int(pool[i]) for i in at[:-1]] + [int(rng.choice([-1, V]))]
                vert += ms
                row += [i if rng.integers(0, 9) else int(rng.choice([-1, len(pool)]))
                        for i in at]
                off.append(len(vert))
                continue
            ms = rng.integers(0, V, int(rng.integers(1, 7))).tolist()
            ms += [ms[0], r, _other_component(rng, comp, r), int(rng.choice([-1, V]))]
            for v in ms:
                vert.append(v)
                row.append((v if to_root else r) if rng.integers(0, 9)
                           else int(rng.choice([-1, V])))
        off.append(len(vert))
    bad = np.nonzero(kind == BAD_DST)[0]
    root[bad] = rng.choice([-1, V], bad.shape[0])
    w = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, n, dtype=np.uint64)
    return types.SimpleNamespace(n=n, kind=kind, effective=eff, root=root, key=key,
                                 mem_off=np.asarray(off, np.int64),
                                 mem_row=np.asarray(row, np.int64),
                                 mem_vertex=np.asarray(vert, np.int64), w=w)


def repeat_rows(n, distinct, seed, strides):
    """n picks among ``distinct`` table rows, pick u different from every pick
    u - s (the global-scratch forms: a few rows of a large graph, repeated)."""
    return _distinct_draw(np.random.default_rng(seed), n, distinct, strides)
