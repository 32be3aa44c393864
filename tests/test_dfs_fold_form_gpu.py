"""The folded search's two forms (csrc/dfs.hip, DESIGN.md 4.1e "low-load
form"): the 4-wave kernel as the caller's batch size selects it, or -- when the
previous folded call on the context left few live searches -- its low-load
instantiation.  The host learns the live count from a word the derive kernel
publishes, never by waiting, so the count it acts on may be stale: every table
is compared with the oracle, bit for bit, whatever form ran, and
`last_dfs_form` must follow the rule (same context, same upload, same batch
size, count <= 2 per CU).

`fat_tree:34` is the smallest fat-tree whose aggregation switches have more
than 32 in-neighbours, so the smallest on which the rows are not paired and the
low-load form exists: 578 edge switches in 34 classes of 17, 578 aggregation
switches that are classes of their own.  A batch of 578 is above 2 sources per
CU and a count of 578 above 2 live searches per CU on the 256 CUs the library
is built for, which the life-cycle tests rely on."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from sdnmpi_amd import _native
from sdnmpi_amd import topologies as T

pytestmark = pytest.mark.gpu

LAYOUTS = ["packed", "tree16", "int32", "hops"]


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def fold_on(monkeypatch):
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")
    monkeypatch.delenv("SDNROUTE_DFS_FOLD_FORM", raising=False)


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


_graphs = {}


def graph(key):
    """(csr, oracle tables of every vertex), built once per graph."""
    if key not in _graphs:
        csr = planted(int(key[7:]))[0] if key.startswith("planted") else T.by_name(key).csr()
        _graphs[key] = (csr, O.dfs_tables(csr, np.arange(csr.V, dtype=np.int32), with_hops=True))
    return _graphs[key]


def k34_lists():
    """fat_tree:34: list A, the 578 edge switches (34 classes), and list B, the
    578 aggregation switches (singleton classes)."""
    fabric = T.by_name("fat_tree:34")
    csr = graph("fat_tree:34")[0]
    A = np.unique(fabric.host_table()[0]).astype(np.int32)
    nb = np.concatenate([csr.col[csr.row_ptr[s]:csr.row_ptr[s + 1]] for s in A])
    B = np.unique(nb).astype(np.int32)
    assert len(A) == 578 and len(B) == 578 and not np.intersect1d(A, B).size
    return A, B


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
    else:
        h = torch.empty((S, V), dtype=torch.int16, device=dev)
        ctx.dfs_tables_tree_device(ts.data_ptr(), S, a.data_ptr(), h.data_ptr(),
                                   _native.TREE_PORT16, 2)
    ctx.synchronize()
    p, t = _native.unpack_tree(a.cpu().numpy().view(np.uint32))
    if h is not None:
        h = h.cpu().numpy().view(np.uint16).astype(np.int32)
        h[h == 0xFFFF] = -1
    return p, t, h


def check(ctx, key, srcs, layout="packed"):
    """One folded call (it has finished on return) against the oracle; returns
    the form it reports."""
    csr, (po, to, ho) = graph(key)
    srcs = np.asarray(srcs, np.int32)
    p, t, h = gpu_rows(ctx, csr, srcs, layout)
    assert ctx.last_launches() == 3
    form = ctx.last_dfs_form()
    np.testing.assert_array_equal(p, po[srcs])
    np.testing.assert_array_equal(t, to[srcs])
    if h is not None:
        np.testing.assert_array_equal(h, ho[srcs])
    return form


# ------------------------------------------------------------ 1. forced forms --

@pytest.mark.parametrize("layout", LAYOUTS)
def test_forced_forms_are_exact(ctx, monkeypatch, layout):
    """Either form forced, every shape: exact tables, three launches, and the
    same kernel name.  Where the in-rows are paired (in-degree <= 32:
    fat_tree:8, the planted graphs) forcing `low` changes nothing, and says
    so."""
    A, B = k34_lists()
    mixed = np.concatenate([A[::2], B[:300], A[:5]])         # leaders, singletons, repeats
    assert len(mixed) > 2 * 256                              # a batch of the 4-wave kernel
    shapes = [("fat_tree:34", [A, mixed], True),
              ("fat_tree:8", [np.arange(80)], False)]
    for seed in range(10):
        V = planted(seed)[0].V
        _, a, b = planted(seed)
        shapes.append(("planted%d" % seed, [np.arange(V), [b, a]], False))
    for key, lists, has_low in shapes:
        ctx.upload(graph(key)[0])
        for srcs in lists:
            names = {}
            for form in ("low", "full"):
                monkeypatch.setenv("SDNROUTE_DFS_FOLD_FORM", form)
                got = check(ctx, key, srcs, layout)
                assert got == (form if has_low else "full"), (key, form, got)
                names[form] = ctx.last_kernel()
            assert names["low"] == names["full"], (key, names)
            if has_low:                          # the 4-wave kernel, in either form
                assert names["low"].startswith("dfs_async_kernel<4"), names


# --------------------------------------------------------- 2. hint life cycle --

def test_hint_life_cycle(ctx):
    key = "fat_tree:34"
    A, B = k34_lists()
    ctx.upload(graph(key)[0])
    assert check(ctx, key, A) == "full"          # nothing published yet
    assert ctx.last_dfs_searched() == 34
    assert check(ctx, key, A) == "low"           # 34 live searches last time
    # B on A's stale count: 578 live searches in the low-load form
    assert check(ctx, key, B) == "low"
    assert ctx.last_dfs_searched() == 578
    assert check(ctx, key, B) == "full"          # 578 > 2 per CU
    assert check(ctx, key, A) == "full"          # ... and still B's count
    assert check(ctx, key, A) == "low"
    # the same graph uploaded again: its counts are no hint
    ctx.upload(graph(key)[0])
    assert check(ctx, key, A) == "full"
    assert check(ctx, key, A) == "low"
    # another batch size does not take A's count
    assert check(ctx, key, A[:-1]) == "full"
    assert check(ctx, key, A[:-1]) == "low"
    assert check(ctx, key, A) == "full"          # nor A that of the 577


def test_host_runs_ahead_of_the_device(ctx):
    """Twenty equal calls queued without a wait: whichever of them the device
    has finished when the host looks, its count is theirs, so all take the
    low-load form (more calls than the ring has entries: a run of equal
    launches is one entry)."""
    key = "fat_tree:34"
    A, _ = k34_lists()
    csr, (po, to, _) = graph(key)
    ctx.upload(csr)
    assert check(ctx, key, A) == "full"
    dev = torch.device("cuda", ctx.device)
    ts = torch.from_numpy(A).to(dev)
    out = torch.empty((len(A), csr.V), dtype=torch.int32, device=dev)
    forms = []
    for _ in range(20):
        ctx.dfs_tables_packed_device(ts.data_ptr(), len(A), out.data_ptr())
        forms.append(ctx.last_dfs_form())
    ctx.synchronize()
    assert forms == ["low"] * 20
    p, t = _native.unpack_tree(out.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(p, po[A])
    np.testing.assert_array_equal(t, to[A])


@pytest.mark.parametrize("layout", ["tree16", "hops"])
def test_hint_in_other_layouts(ctx, layout):
    key = "fat_tree:34"
    A, B = k34_lists()
    ctx.upload(graph(key)[0])
    assert [check(ctx, key, s, layout) for s in (A, A, B, B)] == ["full", "low", "low", "full"]


# ------------------------------------------------- 3. low form, every vertex --

@pytest.mark.parametrize("layout", ["packed", "hops"])
def test_low_form_every_vertex(ctx, monkeypatch, layout):
    """All 1,445 vertices as sources in the low-load form: 629 live searches
    (34 edge and 17 core classes, 578 aggregation switches), 2.5 per CU, more
    than the form is chosen for.  (They do not exceed the grid: 8 workgroups
    of this graph fit a CU.)"""
    monkeypatch.setenv("SDNROUTE_DFS_FOLD_FORM", "low")
    key = "fat_tree:34"
    csr = graph(key)[0]
    ctx.upload(csr)
    assert check(ctx, key, np.arange(csr.V), layout) == "low"
    assert ctx.last_dfs_searched() == 34 + 578 + 17


# ------------------------------------------------------------ 4. two contexts --

def test_two_contexts_keep_their_own_history():
    key = "fat_tree:34"
    A, B = k34_lists()
    c1, c2 = _native.Context(0), _native.Context(0)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        c1.set_stream(s1.cuda_stream)
        c2.set_stream(s2.cuda_stream)
        c1.upload(graph(key)[0])
        c2.upload(graph(key)[0])
        steps = [(c1, A, "full"), (c2, B, "full"),
                 (c1, A, "low"), (c2, B, "full"),      # c1 saw 34, c2 saw 578
                 (c1, B, "low"), (c2, A, "full"),      # each on its own stale count
                 (c1, A, "full"), (c2, A, "low"),      # c1 saw 578, c2 saw 34
                 (c1, A, "low"), (c2, B, "low")]
        for c, srcs, want in steps:
            assert check(c, key, srcs) == want
    finally:
        c1.close()
        c2.close()
