"""The DFS twin fold (csrc/dfs.hip): a batch searches one
source per twin class and derives the other rows.  Every table is compared
with the oracle, bit for bit, in every layout; `last_dfs_searched` shows that
the fold really ran."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from sdnmpi_amd import _native
from sdnmpi_amd import topologies as T

pytestmark = pytest.mark.gpu

LAYOUTS = ["int32", "hops", "packed", "slots", "tree16", "slot32"]


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def twin_reps_py(csr):
    """rep[v] = smallest vertex with v's out-row and in-row; a vertex whose row
    holds a self-loop stays alone."""
    V = csr.V
    out = [tuple(csr.col[csr.row_ptr[u]:csr.row_ptr[u + 1]].tolist()) for u in range(V)]
    ins = [[] for _ in range(V)]
    for u in range(V):
        for v in out[u]:
            ins[v].append(u)
    seen, rep = {}, np.arange(V, dtype=np.int32)
    for v in range(V):
        if v in out[v]:
            continue
        rep[v] = seen.setdefault((out[v], tuple(ins[v])), v)
    return rep


def csr_of(adj, rng):
    """CSR of a boolean adjacency matrix, ports drawn below 60,000."""
    V = adj.shape[0]
    rows, cols = np.nonzero(adj)
    row_ptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=V), out=row_ptr[1:])
    return T.CSR(np.arange(1, V + 1), row_ptr, cols, rng.integers(0, 60000, size=cols.size))


def planted(seed):
    """A random directed graph (V <= 24) in which a and b are twins; every
    fourth one gives the pair no in-links."""
    rng = np.random.default_rng(seed)
    V = int(rng.integers(4, 25))
    adj = rng.random((V, V)) < rng.uniform(0.1, 0.5)
    a, b = (int(x) for x in rng.choice(V, 2, replace=False))
    adj[b, :] = adj[a, :]
    adj[:, b] = adj[:, a]
    if seed % 4 == 0:
        adj[:, a] = adj[:, b] = False
    for x in (a, b):
        for y in (a, b):
            adj[x, y] = False
    return csr_of(adj, rng), a, b


_oracle = {}


def oracle_rows(key, csr, srcs):
    """Oracle rows for the ids in srcs (empty rows for ids that are no
    vertex); the all-vertex tables are computed once per graph."""
    if key not in _oracle:
        _oracle[key] = O.dfs_tables(csr, np.arange(csr.V, dtype=np.int32), with_hops=True)
    po, to, ho = _oracle[key]
    srcs = np.asarray(srcs)
    ok = (srcs >= 0) & (srcs < csr.V)
    pick = np.where(ok, srcs, 0)
    return tuple(np.where(ok[:, None], x[pick], -1).astype(np.int32) for x in (po, to, ho))


def gpu_rows(ctx, csr, srcs, layout):
    """(parent, port, hops or None) as int32, through the device-pointer calls
    (they take ids that are no vertex)."""
    dev = torch.device("cuda", ctx.device)
    ts = torch.from_numpy(np.ascontiguousarray(srcs, np.int32)).to(dev)
    S, V = len(srcs), csr.V
    a = torch.empty((S, V), dtype=torch.int32, device=dev)
    b = torch.empty((S, V), dtype=torch.int32, device=dev)
    h = None
    if layout in ("int32", "hops"):
        if layout == "hops":
            h = torch.empty((S, V), dtype=torch.int32, device=dev)
        ctx.dfs_tables_device(ts.data_ptr(), S, a.data_ptr(), b.data_ptr(),
                              h.data_ptr() if h is not None else 0)
        ctx.synchronize()
        return a.cpu().numpy(), b.cpu().numpy(), None if h is None else h.cpu().numpy()
    if layout == "packed":
        ctx.dfs_tables_packed_device(ts.data_ptr(), S, a.data_ptr())
    elif layout == "slots":
        ctx.dfs_tables_slots_device(ts.data_ptr(), S, a.data_ptr())
    elif layout == "tree16":
        h = torch.empty((S, V), dtype=torch.int16, device=dev)
        ctx.dfs_tables_tree_device(ts.data_ptr(), S, a.data_ptr(), h.data_ptr(),
                                   _native.TREE_PORT16, 2)
    else:
        h = torch.empty((S, V), dtype=torch.int32, device=dev)
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


def check(ctx, key, csr, srcs, layout, folded=None):
    """One call against the oracle; folded: what `last_dfs_searched` must show
    (True: fewer than the batch, False: the batch, None: not looked at)."""
    srcs = np.asarray(srcs, np.int32)
    p, t, h = gpu_rows(ctx, csr, srcs, layout)
    searched = ctx.last_dfs_searched()
    po, to, ho = oracle_rows(key, csr, srcs)
    np.testing.assert_array_equal(p, po)
    np.testing.assert_array_equal(t, to)
    if h is not None:
        np.testing.assert_array_equal(h, ho)
    if folded is True:
        assert searched < len(srcs), (searched, len(srcs))
    elif folded is False:
        assert searched == len(srcs), (searched, len(srcs))
    return searched


# ---------------------------------------------------------------- classes --

@pytest.mark.parametrize("name,classes", [("fat_tree:4", 14), ("fat_tree:8", 44), ("mock", None),
                                          ("dragonfly:4,2,2", 0), ("torus:5,3,2", 0)])
def test_twin_classes_of_fabrics(ctx, name, classes):
    csr = T.by_name(name).csr()
    ctx.upload(csr)
    rep = ctx.twin_reps()
    np.testing.assert_array_equal(rep, twin_reps_py(csr))
    if classes == 0:
        np.testing.assert_array_equal(rep, np.arange(csr.V))
    elif classes:
        assert len(np.unique(rep)) == classes and csr.V == {14: 20, 44: 80}[classes]


def test_twin_classes_need_the_in_row_and_no_link_between(ctx):
    rng = np.random.default_rng(3)
    # 0 and 1 share the out-row {2, 3}; 4 links to 0 only: no twins.  With
    # the link 4 -> 1 as well they are (2 -> 4 keeps 2 and 3 apart)
    adj = np.zeros((5, 5), bool)
    adj[0, [2, 3]] = adj[1, [2, 3]] = True
    adj[4, 0] = adj[2, 4] = True
    ctx.upload(csr_of(adj, rng))
    np.testing.assert_array_equal(ctx.twin_reps(), np.arange(5))
    adj[4, 1] = True
    ctx.upload(csr_of(adj, rng))
    np.testing.assert_array_equal(ctx.twin_reps(), [0, 0, 2, 3, 4])
    # equal out-rows {0, 1, 2} and equal in-rows, but 0 and 1 are in them
    adj = np.zeros((4, 4), bool)
    adj[0, [0, 1, 2]] = adj[1, [0, 1, 2]] = True
    adj[3, [0, 1]] = True
    csr = csr_of(adj, rng)
    ctx.upload(csr)
    np.testing.assert_array_equal(ctx.twin_reps(), np.arange(4))
    np.testing.assert_array_equal(ctx.twin_reps(), twin_reps_py(csr))


# ----------------------------------------------------------------- parity --

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["fat_tree:4", "fat_tree:8", "mock"])
def test_fold_parity_fabrics(ctx, monkeypatch, name, layout):
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")
    csr = T.by_name(name).csr()
    ctx.upload(csr)
    check(ctx, name, csr, np.arange(csr.V), layout, folded=True)


@pytest.mark.parametrize("strategy", ["async", "count", "coop", "lds", "global"])
def test_fold_parity_every_strategy(ctx, monkeypatch, strategy):
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")
    monkeypatch.setenv("SDNROUTE_DFS_STRATEGY", strategy)
    csr = T.by_name("fat_tree:8").csr()
    ctx.upload(csr)
    for layout in ("hops", "tree16", "slots"):
        check(ctx, "fat_tree:8", csr, np.arange(csr.V), layout, folded=True)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fold_parity_random_planted_twins(ctx, monkeypatch, layout):
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")
    no_in = 0
    for seed in range(20):
        csr, a, b = planted(seed)
        ctx.upload(csr)
        rep = ctx.twin_reps()
        np.testing.assert_array_equal(rep, twin_reps_py(csr))
        assert rep[a] == rep[b]
        no_in += not np.any(csr.col == a)
        check(ctx, "planted%d" % seed, csr, np.arange(csr.V), layout, folded=True)
        check(ctx, "planted%d" % seed, csr, [b, a], layout, folded=True)
    assert no_in >= 1


# ----------------------------------------------------------- source lists --

@pytest.mark.parametrize("layout", ["hops", "packed"])
def test_fold_rows_wider_than_a_workgroup(ctx, monkeypatch, layout):
    """Twins with 298 out-links: more patched entries than the derive kernel
    has threads."""
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")
    rng = np.random.default_rng(5)
    V = 300
    adj = rng.random((V, V)) < 0.01
    adj[:, :2] = False
    adj[:2, :] = False
    adj[0, 2:] = adj[1, 2:] = True
    adj[7, :2] = adj[99, :2] = True
    np.fill_diagonal(adj, False)
    csr = csr_of(adj, rng)
    ctx.upload(csr)
    assert ctx.twin_reps()[1] == 0
    check(ctx, "wide", csr, [1, 0, 7, 1], layout, folded=True)
    check(ctx, "wide", csr, np.arange(V), layout, folded=True)


@pytest.mark.parametrize("tables", ["lds", "global"])
@pytest.mark.parametrize("layout", ["hops", "tree16", "slots"])
def test_fold_source_lists(ctx, monkeypatch, layout, tables):
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")
    if tables == "global":                       # the prep kernel's class tables
        monkeypatch.setenv("SDNROUTE_DFS_FOLD_LDS", "0")
    name = "fat_tree:8"
    csr = T.by_name(name).csr()
    ctx.upload(csr)
    rep = twin_reps_py(csr)
    V = csr.V
    members = {}
    for v in range(V):
        members.setdefault(int(rep[v]), []).append(v)
    big = [m for m in members.values() if len(m) >= 3]
    assert len(big) >= 2
    rng = np.random.default_rng(11)
    check(ctx, name, csr, rng.permutation(V), layout, folded=True)             # shuffled
    # more positions than the prep kernel has threads, every id many times
    assert check(ctx, name, csr, rng.integers(-1, V + 1, 2500), layout, folded=True) == 44
    assert check(ctx, name, csr, [5, 5], layout, folded=True) == 1             # a source twice
    assert check(ctx, name, csr, big[0][1:3], layout, folded=True) == 1        # no smallest vertex
    assert check(ctx, name, csr, [big[0][2], -1, big[0][1], V, big[1][1]], layout) == 2
    assert check(ctx, name, csr, [-1, V], layout) == 0
    assert check(ctx, name, csr, [big[1][1]], layout, folded=False) == 1       # a single source
    # only non-leaders, of different classes: nothing to derive from another
    assert check(ctx, name, csr, [m[1] for m in big], layout, folded=False) == len(big)


# ------------------------------------------------------ knob and threshold --

def test_fold_knob_and_threshold(ctx, monkeypatch):
    name = "fat_tree:8"
    csr = T.by_name(name).csr()
    ctx.upload(csr)
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "0")
    check(ctx, name, csr, np.arange(csr.V), "packed", folded=False)
    assert ctx.last_launches() == 1
    monkeypatch.delenv("SDNROUTE_DFS_FOLD")
    check(ctx, name, csr, np.arange(csr.V), "packed", folded=False)            # a tiny batch
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")
    check(ctx, name, csr, np.arange(csr.V), "packed", folded=True)
    assert ctx.last_launches() == 3
    # a graph without twins has nothing to fold
    csr = T.by_name("dragonfly:4,2,2").csr()
    ctx.upload(csr)
    check(ctx, "dragonfly:4,2,2", csr, np.arange(csr.V), "packed", folded=False)
