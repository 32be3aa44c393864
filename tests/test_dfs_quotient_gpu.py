"""The twin-class quotient in dfs_async_kernel (csrc/dfs.hip):
the search runs over the graph's twin classes and the flush expands the class
records to the vertices.  Every table is compared bit for bit with the oracle
and with the same call on the graph itself (SDNROUTE_DFS_QUOTIENT=0), and what
the context reports about the call -- kernel name, launches, searched count,
form -- has to be what it is without the quotient."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from sdnmpi_amd import _native
from sdnmpi_amd import topologies as T

import golden_util as G

pytestmark = pytest.mark.gpu

LAYOUTS = ["packed", "int32", "hops", "tree16", "slots"]


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("SDNROUTE_DFS_QUOTIENT", "SDNROUTE_DFS_FOLD", "SDNROUTE_DFS_FOLD_FORM",
              "SDNROUTE_DFS_ASYNC_WAVES", "SDNROUTE_DFS_STRATEGY"):
        monkeypatch.delenv(k, raising=False)


def csr_of(adj, rng):
    V = adj.shape[0]
    rows, cols = np.nonzero(adj)
    row_ptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=V), out=row_ptr[1:])
    return T.CSR(np.arange(1, V + 1), row_ptr, cols, rng.integers(0, 60000, size=cols.size))


def planted12():
    """12 vertices, one-way links and a self-loop; 3, 7 and 9 are twins, 1 and
    5 twins nobody links to."""
    rng = np.random.default_rng(12)
    adj = rng.random((12, 12)) < 0.25
    np.fill_diagonal(adj, False)
    for b in (7, 9):
        adj[b, :] = adj[3, :]
        adj[:, b] = adj[:, 3]
    adj[5, :] = adj[1, :]
    adj[:, [1, 5]] = False
    for g in ((3, 7, 9), (1, 5)):
        for x in g:
            for y in g:
                adj[x, y] = False
    adj[4, 4] = True
    adj[0, 3] = adj[0, 7] = adj[0, 9] = True     # the class is reached
    return csr_of(adj, rng)


def class65():
    """65 switches without a link (one class of 65, reached by no one), and a
    small fabric beside them: 65 -> {66, 67, 68} twins -> 69 -> 65."""
    rng = np.random.default_rng(65)
    adj = np.zeros((70, 70), bool)
    adj[65, 66:69] = True
    adj[66:69, 69] = True
    adj[69, 65] = True
    return csr_of(adj, rng)


_graphs = {}


def graph(key):
    """(csr, oracle tables of every vertex), built once per graph."""
    if key not in _graphs:
        if key == "planted12":
            csr = planted12()
        elif key == "class65":
            csr = class65()
        elif key in G.LOOPS:
            csr = G.Golden(key).fabric().csr()
        else:
            csr = T.by_name(key).csr()
        _graphs[key] = (csr, O.dfs_tables(csr, np.arange(csr.V, dtype=np.int32), with_hops=True))
    return _graphs[key]


def oracle_rows(key, srcs):
    csr, tabs = graph(key)
    ok = (srcs >= 0) & (srcs < csr.V)
    pick = np.where(ok, srcs, 0)
    return tuple(np.where(ok[:, None], x[pick], -1).astype(np.int32) for x in tabs)


def gpu_rows(ctx, csr, srcs, layout):
    """(parent, port, hops or None) as int32 through the device-pointer calls."""
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
    else:
        h = torch.empty((S, V), dtype=torch.int16, device=dev)
        ctx.dfs_tables_tree_device(ts.data_ptr(), S, a.data_ptr(), h.data_ptr(),
                                   _native.TREE_PORT16, 2)
    ctx.synchronize()
    tree = a.cpu().numpy().view(np.uint32)
    p, t = _native.unpack_slots(tree, csr) if layout == "slots" else _native.unpack_tree(tree)
    if h is not None:
        h = h.cpu().numpy().view(np.uint16).astype(np.int32)
        h[h == 0xFFFF] = -1
    return p, t, h


def call(ctx, monkeypatch, key, srcs, layout, quotient, fold, calls=1):
    """A fresh upload (no published count from another call), then `calls`
    equal calls, each against the oracle; returns the last call's tables and
    what the context reports about every call."""
    csr = graph(key)[0]
    srcs = np.asarray(srcs, np.int32)
    monkeypatch.setenv("SDNROUTE_DFS_QUOTIENT", "1" if quotient else "0")
    if fold is not None:
        monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1" if fold else "0")
    ctx.upload(csr)
    po, to, ho = oracle_rows(key, srcs)
    seen = []
    for _ in range(calls):
        p, t, h = gpu_rows(ctx, csr, srcs, layout)
        seen.append((ctx.last_dfs_quotient(), ctx.last_kernel(), ctx.last_launches(),
                     ctx.last_dfs_searched(), ctx.last_dfs_form()))
        np.testing.assert_array_equal(p, po)
        np.testing.assert_array_equal(t, to)
        if h is not None:
            np.testing.assert_array_equal(h, ho)
    return (p, t, h), seen


def both(ctx, monkeypatch, key, srcs, layout, fold, calls=1, expect=1):
    """The call with the quotient forced off and on: equal tables, the pinned
    reports equal, and last_dfs_quotient() 0 and `expect`."""
    off, seen0 = call(ctx, monkeypatch, key, srcs, layout, False, fold, calls)
    on, seen1 = call(ctx, monkeypatch, key, srcs, layout, True, fold, calls)
    for x, y in zip(off, on):
        if x is not None:
            np.testing.assert_array_equal(x, y)
    assert [s[0] for s in seen0] == [0] * calls
    assert [s[0] for s in seen1] == [expect] * calls
    assert [s[1:] for s in seen0] == [s[1:] for s in seen1]
    if fold:
        assert all(s[2] == 3 for s in seen1)
    return seen1


def has_twins(ctx, key):
    ctx.upload(graph(key)[0])
    rep = np.asarray(ctx.twin_reps())
    return int(np.any(rep != np.arange(len(rep))))


# ---------------------------------------------------------------- every root --

@pytest.mark.parametrize("fold", [False, True], ids=["unfolded", "folded"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("key", ["fat_tree:4", "fat_tree:8", "planted12", "class65"] + G.LOOPS)
def test_every_root(ctx, monkeypatch, key, layout, fold):
    csr = graph(key)[0]
    expect = has_twins(ctx, key)
    if key in ("fat_tree:4", "fat_tree:8", "planted12", "class65", "fat_tree_k4_loops"):
        assert expect == 1
    fold = fold and expect == 1                  # a graph without twins never folds
    ids = np.concatenate([np.arange(csr.V), [-1, csr.V]]).astype(np.int32)
    both(ctx, monkeypatch, key, ids, layout, fold, expect=expect)


def test_sizes_of_the_small_graphs():
    assert graph("fat_tree:4")[0].V == 20 and graph("planted12")[0].V == 12
    csr = graph("class65")[0]
    assert csr.V == 70 and not np.diff(csr.row_ptr)[:65].any()
    assert not np.isin(csr.col, np.arange(65)).any()


# -------------------------------------------------------------- source lists --

@pytest.mark.parametrize("fold", [False, True], ids=["unfolded", "folded"])
@pytest.mark.parametrize("layout", ["packed", "hops", "slots"])
def test_source_lists(ctx, monkeypatch, layout, fold):
    key = "fat_tree:8"
    csr = graph(key)[0]
    ctx.upload(csr)
    rep = np.asarray(ctx.twin_reps())
    V = csr.V
    members = {}
    for v in range(V):
        members.setdefault(int(rep[v]), []).append(v)
    big = [m for m in members.values() if len(m) >= 3]
    single = [m[0] for m in members.values() if len(m) == 1]
    assert len(big) >= 2 and len(single) == 32   # k=8: 32 aggregation switches
    lists = {
        "twins of one class": big[0],
        "non-leaders first": big[0][::-1] + big[1][1:] + big[1][:1],
        "the largest member alone": big[0][-1:],
        "aggregation switches": single[:9],
        "repeats": [big[0][1]] * 3 + single[:2] * 2 + [big[1][2]] * 2,
        "no vertex": [-1, V, big[0][1], V, -1, single[0]],
        "only no vertex": [-1, V],
    }
    for what, ids in lists.items():
        seen = both(ctx, monkeypatch, key, ids, layout, fold)
        if fold and what == "twins of one class":
            assert seen[0][3] == 1, what         # one search, the other rows derived


# -------------------------------------------------------- the folded 8-wave form --

@pytest.mark.parametrize("layout", ["packed", "tree16", "hops"])
def test_k34_lists(ctx, monkeypatch, layout):
    """fat_tree:34's 578 edge switches (34 classes) and 578 aggregation
    switches, two equal folded calls each: the second takes the low-load form
    from the first one's count, with and without the quotient."""
    key = "fat_tree:34"
    fabric = T.by_name(key)
    csr = graph(key)[0]
    A = np.unique(fabric.host_table()[0]).astype(np.int32)
    nb = np.concatenate([csr.col[csr.row_ptr[s]:csr.row_ptr[s + 1]] for s in A])
    B = np.unique(nb).astype(np.int32)
    assert len(A) == 578 and len(B) == 578 and not np.intersect1d(A, B).size
    seen = both(ctx, monkeypatch, key, A, layout, True, calls=2)
    assert [s[3] for s in seen] == [34, 34] and [s[4] for s in seen] == ["full", "low"]
    if layout == "packed":
        seen = both(ctx, monkeypatch, key, B, layout, True, calls=2)
        assert [s[3] for s in seen] == [578, 578]
        both(ctx, monkeypatch, key, A[::7], layout, False)


# ------------------------------------------------------------- rule and knob --

def test_default_rule_and_twin_free_graphs(ctx, monkeypatch):
    """Without the knob: a fat tree's quotient (1 / k of the links) is taken,
    a graph with one small class stays on its own rows; a graph without twins
    has no quotient, whatever the knob says."""
    def default(key):
        csr = graph(key)[0]
        ctx.upload(csr)
        ids = np.arange(csr.V, dtype=np.int32)
        p, t, _ = gpu_rows(ctx, csr, ids, "packed")
        po, to, _ = oracle_rows(key, ids)
        np.testing.assert_array_equal(p, po)
        np.testing.assert_array_equal(t, to)
        return ctx.last_dfs_quotient()

    assert default("fat_tree:8") == 1
    assert default("planted12") == 0
    for key in ("dragonfly:4,2,2", "torus:5,3,2"):
        assert has_twins(ctx, key) == 0
        assert default(key) == 0
        csr = graph(key)[0]
        both(ctx, monkeypatch, key, np.arange(csr.V), "packed", None, expect=0)
        both(ctx, monkeypatch, key, np.arange(csr.V), "hops", None, expect=0)
        monkeypatch.delenv("SDNROUTE_DFS_QUOTIENT")


def test_other_strategies_report_no_quotient(ctx, monkeypatch):
    monkeypatch.setenv("SDNROUTE_DFS_STRATEGY", "count")
    both(ctx, monkeypatch, "fat_tree:8", np.arange(80), "hops", False, expect=0)


# --------------------------------------------- the benchmark's own path, once --

def test_k48_second_call(ctx):
    """k=48, its 1,152 edge switches, packed tables, nothing forced: the call
    the benchmark times is the second and later ones."""
    fabric = T.by_name("fat_tree:48")
    csr = fabric.csr()
    srcs = np.unique(fabric.host_table()[0]).astype(np.int32)
    assert len(srcs) == 1152
    po, to, _ = O.dfs_tables(csr, srcs, with_hops=False, nthreads=8)
    ctx.upload(csr)
    seen = []
    for _ in range(2):
        p, t, _ = gpu_rows(ctx, csr, srcs, "packed")
        seen.append((ctx.last_dfs_quotient(), ctx.last_launches(), ctx.last_dfs_searched(),
                     ctx.last_dfs_form()))
        np.testing.assert_array_equal(p, po)
        np.testing.assert_array_equal(t, to)
    assert seen == [(1, 3, 48, "full"), (1, 3, 48, "low")]
