"""The twin fold's derive kernel (csrc/dfs.hip): a workgroup
per batch position copies its leader's row, and every patched word is stored
by the wave whose copy store covered it, after that store, with no barrier on
global memory in between; a further wave works the patches out and hands them
over in LDS.

Every table is compared with the oracle bit for bit; the fold is forced and
`last_launches` / `last_dfs_searched` show that it ran.  The shapes are the
smallest at which the list handling and the owner rule can go wrong:

* list shapes: lists of every length 1 .. 17 built from twins -- class after
  class, behind one vertex without twins, leader after leader, and reversed
  (the leader is not the class's smallest vertex) -- in all six layouts;
* awkward lists: ids that are no vertex, a source twice, a non-leader on both
  sides of an invalid id, a leader 1 .. 9 positions ahead of a member;
* the owner rule: planted-twin graphs with V = 4 m .. 4 m + 3 (rows that are no
  whole vectors: the element paths) and V a multiple of 8 (the 16-byte paths;
  V = 2056 gives a thread two or three vectors of a row), the twins relabelled
  to every ordered pair of {0, 3, 4, 7, V - 1};
* output tensors 4 bytes off a 16-byte boundary, one table at a time;
* twins with 300 out-links: a patch list longer than the workgroup."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from sdnmpi_amd import _native
from sdnmpi_amd import topologies as T
from test_dfs_twin_fold import LAYOUTS, csr_of, twin_reps_py

pytestmark = pytest.mark.gpu

NMAX = 17                                        # the longest list of the shape tests


def ENDS(V):
    """Where the twins are put."""
    return (0, 3, 4, 7, V - 1)


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def forced(monkeypatch):
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")


# ---------------------------------------------------------------- helpers --

_oracle = {}


def oracle_rows(key, csr, srcs):
    """Oracle rows of the ids in srcs (empty rows for ids that are no vertex),
    each distinct source of a graph computed once."""
    srcs = np.asarray(srcs, np.int64)
    have = _oracle.setdefault(key, {})
    new = sorted({int(s) for s in srcs if 0 <= s < csr.V} - set(have))
    if new:
        po, to, ho = O.dfs_tables(csr, np.asarray(new, np.int32), with_hops=True)
        for i, s in enumerate(new):
            have[s] = tuple(np.asarray(x[i], np.int32).copy() for x in (po, to, ho))
    empty = np.full(csr.V, -1, np.int32)
    rows = [have.get(int(s), (empty, empty, empty)) for s in srcs]
    return tuple(np.stack([r[k] for r in rows]) for k in range(3))


def table(S, V, dtype, dev, off):
    """An (S, V) device tensor whose data pointer is `off` bytes behind a
    16-byte boundary."""
    item = torch.empty((), dtype=dtype).element_size()
    assert off % item == 0
    flat = torch.empty(S * V + 16, dtype=dtype, device=dev)
    assert flat.data_ptr() % 16 == 0
    t = flat[off // item:off // item + S * V].view(S, V)
    assert t.data_ptr() % 16 == off and t.is_contiguous()
    return t


def gpu_rows(ctx, csr, srcs, layout, off=(0, 0, 0)):
    """(parent, port, hops or None) as int32 through the device-pointer calls;
    off: byte offsets of table 0, table 1 and the depth plane."""
    dev = torch.device("cuda", ctx.device)
    ts = torch.from_numpy(np.ascontiguousarray(srcs, np.int32)).to(dev)
    S, V = len(srcs), csr.V
    a = table(S, V, torch.int32, dev, off[0])
    h = None
    if layout in ("int32", "hops"):
        b = table(S, V, torch.int32, dev, off[1])
        if layout == "hops":
            h = table(S, V, torch.int32, dev, off[2])
        ctx.dfs_tables_device(ts.data_ptr(), S, a.data_ptr(), b.data_ptr(),
                              h.data_ptr() if h is not None else 0)
        ctx.synchronize()
        return a.cpu().numpy(), b.cpu().numpy(), None if h is None else h.cpu().numpy()
    if layout == "packed":
        ctx.dfs_tables_packed_device(ts.data_ptr(), S, a.data_ptr())
    elif layout == "slots":
        ctx.dfs_tables_slots_device(ts.data_ptr(), S, a.data_ptr())
    elif layout == "tree16":
        h = table(S, V, torch.int16, dev, off[2])
        ctx.dfs_tables_tree_device(ts.data_ptr(), S, a.data_ptr(), h.data_ptr(),
                                   _native.TREE_PORT16, 2)
    else:
        h = table(S, V, torch.int32, dev, off[2])
        ctx.dfs_tables_tree_device(ts.data_ptr(), S, a.data_ptr(), h.data_ptr(),
                                   _native.TREE_SLOT, 4)
    ctx.synchronize()
    tree = a.cpu().numpy().view(np.uint32)
    p, t = _native.unpack_slots(tree, csr) if layout in ("slots", "slot32") \
        else _native.unpack_tree(tree)
    if h is not None:
        h = h.cpu().numpy()
        if h.dtype == np.int16:
            h = h.view(np.uint16).astype(np.int32)
            h[h == 0xFFFF] = -1
    return p, t, h


def check(ctx, key, csr, rep, srcs, layout, off=(0, 0, 0)):
    """One folded call against the oracle; the searched count is the number of
    twin classes in the list."""
    srcs = np.asarray(srcs, np.int32)
    p, t, h = gpu_rows(ctx, csr, srcs, layout, off)
    assert ctx.last_launches() == 3, (ctx.last_launches(), srcs)
    ok = srcs[(srcs >= 0) & (srcs < csr.V)]
    assert ctx.last_dfs_searched() == len(np.unique(rep[ok])), srcs
    po, to, ho = oracle_rows(key, csr, srcs)
    np.testing.assert_array_equal(p, po, err_msg=str(srcs))
    np.testing.assert_array_equal(t, to, err_msg=str(srcs))
    if h is not None:
        np.testing.assert_array_equal(h, ho, err_msg=str(srcs))


def classes_of(rep):
    """The twin classes with at least two members, and the vertices alone in
    theirs, both ascending."""
    members = {}
    for v, r in enumerate(rep):
        members.setdefault(int(r), []).append(v)
    big = [m for _, m in sorted(members.items()) if len(m) >= 2]
    alone = [m[0] for _, m in sorted(members.items()) if len(m) == 1]
    return big, alone


def planted(seed, V, a, b, extra=(), p=None):
    """The generator of test_dfs_twin_fold.planted with V and the twins (a, b)
    given: a random directed graph in which a and b have equal out- and in-rows
    and no link between them; every fourth seed gives the pair no in-links (ls
    is then unreached from s); extra: columns put into the twins' out-row."""
    rng = np.random.default_rng(seed)
    adj = rng.random((V, V)) < (rng.uniform(0.1, 0.5) if p is None else p)
    for x in extra:
        adj[a, x] = True
    adj[b, :] = adj[a, :]
    adj[:, b] = adj[:, a]
    if seed % 4 == 0:
        adj[:, a] = adj[:, b] = False
    for x in (a, b):
        for y in (a, b):
            adj[x, y] = False
    return csr_of(adj, rng)


def pair_of(seed, V):
    """Ordered pair number `seed` of ENDS(V): 20 of them."""
    pairs = [(a, b) for a in ENDS(V) for b in ENDS(V) if a != b]
    assert len(pairs) == 20
    return pairs[seed % 20]


# ------------------------------------------------------------ list shapes --

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["fat_tree:4", "fat_tree:8"])
def test_group_boundaries(ctx, name, layout):
    csr = T.by_name(name).csr()
    ctx.upload(csr)
    rep = twin_reps_py(csr)
    big, alone = classes_of(rep)
    assert len(np.unique(rep)) == {20: 14, 80: 44}[csr.V]
    adjacent = [v for m in big for v in m]                   # class after class
    width = max(len(m) for m in big)
    mixed = [m[i] for i in range(width) for m in big if i < len(m)]    # leader after leader
    assert len(adjacent) >= NMAX or name == "fat_tree:4"
    for n in range(1, NMAX + 1):
        pool = adjacent * 2                      # fat_tree:4 has 12 twins: go round again
        check(ctx, name, csr, rep, pool[:n], layout)
        check(ctx, name, csr, rep, (alone[:1] + pool)[:n], layout)     # shifted by one
        check(ctx, name, csr, rep, (mixed * 2)[:n], layout)
        check(ctx, name, csr, rep, pool[:n][::-1], layout)   # the leader is not the smallest


# ---------------------------------------------------------- awkward lists --

@pytest.mark.parametrize("layout", LAYOUTS)
def test_awkward_groups(ctx, layout):
    name = "fat_tree:8"
    csr = T.by_name(name).csr()
    ctx.upload(csr)
    rep = twin_reps_py(csr)
    V = csr.V
    big, alone = classes_of(rep)
    c0, c1 = big[0], big[1]
    assert len(c0) >= 4 and len(c1) >= 3
    lst = [c0[1], c0[2], -1, c0[3], V, c0[2], c0[2], c1[0],
           c1[1], -1, c0[0], V, c1[1], c1[2], alone[0], c0[1], c1[0], c0[3]]
    for lead_in in range(9):                     # the list moves through the batch positions
        check(ctx, name, csr, rep, alone[1:1 + lead_in] + lst, layout)
    check(ctx, name, csr, rep, [-1, V, -1, V, -1], layout)
    check(ctx, name, csr, rep, [-1, c0[2], V], layout)
    check(ctx, name, csr, rep, [c0[2]] * 9 + [c0[1]], layout)
    # the leader 1 .. 9 positions ahead of a member
    for gap in (1, 2, 3, 7, 8, 9):
        check(ctx, name, csr, rep, [c0[3]] + alone[:gap - 1] + [c0[0], c0[3]], layout)


# ------------------------------------------------------------- owner rule --

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("base", [20, 24])
def test_owner_rule_small_rows(ctx, layout, base):
    """base 20: V = 20 .. 23, int32 rows of 80 .. 92 bytes and u16 rows of 40 ..
    46 (element paths but for V = 20's int32 tables); base 24: V = 24, every
    table on its 16-byte path."""
    unreached = 0
    for seed in range(20):
        V = base + (seed % 4 if base == 20 else 0)
        a, b = pair_of(seed, V)
        csr = planted(seed, V, a, b)
        ctx.upload(csr)
        rep = twin_reps_py(csr)
        assert rep[a] == rep[b]
        unreached += not np.any(csr.col == a)
        key = "p%d_%d" % (base, seed)
        check(ctx, key, csr, rep, np.arange(V), layout)
        check(ctx, key, csr, rep, [b, a], layout)
        check(ctx, key, csr, rep, [b, a, b, -1, a, a, b, b, a, b], layout)
    assert unreached == 5


BIG_V = 2056         # 514 vectors of int32, 257 of u16: threads hold 1 .. 3 vectors of a row


def big_graph(seed):
    a, b = pair_of(3 * seed + 1, BIG_V)
    # patched columns in a thread's first vector (0 .. 7), its second (1024 ..),
    # its last (2048 ..), beside the twins' own and in the row's last vector
    extra = [x for x in (1, 2, 5, 6, 1024, 1025, 1027, 1031, 2048, 2050, 2051, BIG_V - 2)
             if x not in (a, b)]
    return planted(seed, BIG_V, a, b, extra, p=0.002), a, b


@pytest.mark.parametrize("layout", LAYOUTS)
def test_owner_rule_vectors_of_one_thread(ctx, layout):
    for seed in range(4):
        csr, a, b = big_graph(seed)
        ctx.upload(csr)
        rep = ctx.twin_reps()
        assert rep[a] == rep[b]
        check(ctx, "big%d" % seed, csr, rep, [b, a, 5, b, a], layout)
        check(ctx, "big%d" % seed, csr, rep, [a, b], layout)


# ------------------------------------------------------ unaligned outputs --

@pytest.mark.parametrize("layout,off", [
    ("hops", (4, 0, 0)), ("hops", (0, 4, 0)), ("hops", (0, 0, 4)), ("hops", (4, 4, 4)),
    ("packed", (4, 0, 0)), ("slots", (4, 0, 0)),
    ("tree16", (4, 0, 0)), ("tree16", (0, 0, 4)), ("slot32", (0, 0, 4))])
def test_unaligned_output(ctx, layout, off):
    """Row sizes are multiples of 16 bytes, the input tables aligned: the table
    whose pointer is 4 bytes off takes the element path, the others stay on
    the 16-byte path."""
    for seed in range(0, 20, 3):
        a, b = pair_of(seed, 24)
        csr = planted(seed, 24, a, b)
        ctx.upload(csr)
        rep = twin_reps_py(csr)
        check(ctx, "p24_%d" % seed, csr, rep, np.arange(24), layout, off)
        check(ctx, "p24_%d" % seed, csr, rep, [b, a, b, b, a], layout, off)
    csr, a, b = big_graph(0)
    ctx.upload(csr)
    check(ctx, "big0", csr, ctx.twin_reps(), [b, a, 5, b, a], layout, off)


# ----------------------------------------- a row wider than the workgroup --

@pytest.mark.parametrize("layout", ["packed", "hops"])
def test_patch_list_longer_than_the_workgroup(ctx, layout):
    """Twins 0 and 1 with out-degree 300 in 310 vertices: 302 patches a row,
    the second chunk of the list holds row entries and the root."""
    rng = np.random.default_rng(7)
    V = 310
    adj = rng.random((V, V)) < 0.01
    adj[:, :2] = False
    adj[:2, :] = False
    adj[0, 2:302] = adj[1, 2:302] = True
    adj[7, :2] = adj[99, :2] = adj[305, :2] = True
    np.fill_diagonal(adj, False)
    csr = csr_of(adj, rng)
    ctx.upload(csr)
    rep = ctx.twin_reps()
    assert rep[1] == 0 and csr.row_ptr[1] - csr.row_ptr[0] == 300
    check(ctx, "wide300", csr, rep, [1, 0, 7, 1], layout)
    check(ctx, "wide300", csr, rep, [0, 1, 1, 305, 1, 0, -1, 1, 1], layout)
    check(ctx, "wide300", csr, rep, np.arange(V), layout)
