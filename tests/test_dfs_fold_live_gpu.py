"""The trimmed twin fold (csrc/dfs.hip): the search bounded by
the live count on the device, the prep kernel's short form, and the derive
kernel's patches in every layout, row width and alignment.  Every table is
compared with the oracle, bit for bit, with the fold forced on;
`last_dfs_searched` must equal the number of twin classes among the batch's
vertices."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from sdnmpi_amd import _native
from sdnmpi_amd import topologies as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def fold_on(monkeypatch):
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")


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


def wide():
    """300 vertices, 0 and 1 twins with 298 out-links: more patched entries
    than the derive kernel has threads."""
    rng = np.random.default_rng(5)
    V = 300
    adj = rng.random((V, V)) < 0.01
    adj[:, :2] = False
    adj[:2, :] = False
    adj[0, 2:] = adj[1, 2:] = True
    adj[7, :2] = adj[99, :2] = True
    np.fill_diagonal(adj, False)
    return csr_of(adj, rng)


def sparse_with_pair(V, seed):
    """A random directed graph of out-degree <= 8 in which 0 and 1 are twins
    (1 to 7 links drawn per vertex; a link to 0 brings the one to 1)."""
    rng = np.random.default_rng(seed)
    adj = np.zeros((V, V), bool)
    for u in range(V):
        adj[u, rng.choice(V, int(rng.integers(1, 8)), replace=False)] = True
    adj[1, :] = adj[0, :]
    adj[:, 1] = adj[:, 0]
    adj[:2, :2] = False
    np.fill_diagonal(adj, False)
    return csr_of(adj, rng)


_oracle = {}
_reps = {}


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


def classes_in(key, csr, srcs):
    """The twin classes among the vertices of srcs: what a fold searches."""
    if key not in _reps:
        _reps[key] = twin_reps_py(csr)
    srcs = np.asarray(srcs)
    ok = (srcs >= 0) & (srcs < csr.V)
    return len(np.unique(_reps[key][srcs[ok]]))


def gpu_rows(ctx, csr, srcs, layout, off=0):
    """(parent, port, hops or None) as int32, through the device-pointer calls
    (they take ids that are no vertex).  off: every output table starts `off`
    4-byte words into its allocation (a base that is not 16-byte aligned)."""
    dev = torch.device("cuda", ctx.device)
    ts = torch.from_numpy(np.ascontiguousarray(srcs, np.int32)).to(dev)
    S, V = len(srcs), csr.V

    def table(dtype):
        per = 4 // torch.empty((), dtype=dtype).element_size()
        flat = torch.empty(S * V + off * per, dtype=dtype, device=dev)
        t = flat[off * per:].view(S, V)
        assert t.data_ptr() % 16 == (4 * off) % 16
        return t

    a, b = table(torch.int32), table(torch.int32)
    h = None
    if layout in ("int32", "hops"):
        if layout == "hops":
            h = table(torch.int32)
        ctx.dfs_tables_device(ts.data_ptr(), S, a.data_ptr(), b.data_ptr(),
                              h.data_ptr() if h is not None else 0)
        ctx.synchronize()
        return a.cpu().numpy(), b.cpu().numpy(), None if h is None else h.cpu().numpy()
    if layout == "packed":
        ctx.dfs_tables_packed_device(ts.data_ptr(), S, a.data_ptr())
    elif layout == "slots":
        ctx.dfs_tables_slots_device(ts.data_ptr(), S, a.data_ptr())
    elif layout == "tree16":
        h = table(torch.int16)
        ctx.dfs_tables_tree_device(ts.data_ptr(), S, a.data_ptr(), h.data_ptr(),
                                   _native.TREE_PORT16, 2)
    else:
        h = table(torch.int32)
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


def check(ctx, key, csr, srcs, layout, off=0):
    """One folded call against the oracle; the searched count must be the
    number of classes in the batch.  Returns that count."""
    srcs = np.asarray(srcs, np.int32)
    p, t, h = gpu_rows(ctx, csr, srcs, layout, off)
    searched = ctx.last_dfs_searched()
    assert ctx.last_launches() == 3
    po, to, ho = oracle_rows(key, csr, srcs)
    np.testing.assert_array_equal(p, po)
    np.testing.assert_array_equal(t, to)
    if h is not None:
        np.testing.assert_array_equal(h, ho)
    assert searched == classes_in(key, csr, srcs), (searched, len(srcs))
    return searched


# -------------------------------------------------- 1. more live than grid --

@pytest.mark.parametrize("waves", [None, "8"])
@pytest.mark.parametrize("layout", ["packed", "hops"])
def test_live_searches_exceed_the_grid(ctx, monkeypatch, layout, waves):
    """About 1,499 live searches.  With 8 waves per search at most 4 workgroups fit
    a CU's 32 wave slots, so the grid is 4 per CU and the source loop strides
    with the count read from the device; the default variant is run too."""
    if waves:
        monkeypatch.setenv("SDNROUTE_DFS_ASYNC_WAVES", waves)
    V = 1500
    csr = sparse_with_pair(V, 21)
    ctx.upload(csr)
    assert ctx.twin_reps()[1] == 0
    live = check(ctx, "sparse1500", csr, np.arange(V), layout)
    assert V - 4 <= live <= V - 1              # the planted pair; a chance pair at most
    assert ctx.last_kernel().startswith("dfs_async_kernel")
    if waves:
        cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
        assert live > 4 * cus


# ---------------------------------------------------------- 2. stale count --

@pytest.mark.parametrize("layout", ["packed", "hops"])
def test_count_is_read_at_every_call(ctx, layout):
    name = "fat_tree:8"
    csr = T.by_name(name).csr()
    ctx.upload(csr)
    V = csr.V
    rep = twin_reps_py(csr)
    members = {}
    for v in range(V):
        members.setdefault(int(rep[v]), []).append(v)
    big = [m for m in members.values() if len(m) >= 3]
    assert check(ctx, name, csr, np.arange(V), layout) == 44
    assert check(ctx, name, csr, [big[1][1]], layout) == 1
    assert check(ctx, name, csr, [-1, V], layout) == 0
    assert check(ctx, name, csr, np.arange(V), layout) == 44


# ------------------------------------------------------- 3. every strategy --

@pytest.mark.parametrize("strategy", ["async", "count", "coop", "lds", "global"])
def test_every_strategy_padded_or_live(ctx, monkeypatch, strategy):
    """The strategies that do not take the count keep their -1 padding."""
    monkeypatch.setenv("SDNROUTE_DFS_STRATEGY", strategy)
    name = "fat_tree:8"
    csr = T.by_name(name).csr()
    ctx.upload(csr)
    ids = np.random.default_rng(17).integers(-1, csr.V + 1, 2500)
    assert (ids < 0).any() and (ids >= csr.V).any()
    for layout in ("packed", "slots"):
        assert check(ctx, name, csr, ids, layout) == 44


# ------------------------------------------------------ 4. derive patches --

@pytest.mark.parametrize("layout", ["int32", "tree16", "hops"])
def test_derive_more_patches_than_threads(ctx, layout):
    """The slot encoding holds rows of at most 63 links, so the library takes
    no slot layout on this graph: its int32 hop plane is run with the int32
    tables instead (slot32 is in test_derive_planted_twins)."""
    csr = wide()
    ctx.upload(csr)
    assert ctx.twin_reps()[1] == 0
    check(ctx, "wide", csr, [1, 0, 7, 1], layout)
    check(ctx, "wide", csr, np.arange(csr.V), layout)


@pytest.mark.parametrize("layout", ["int32", "tree16", "slot32"])
def test_derive_planted_twins(ctx, layout):
    no_in = unreached = 0
    for seed in range(8):
        csr, a, b = planted(seed)
        ctx.upload(csr)
        key = "planted%d" % seed
        no_in += not np.any(csr.col == a)
        unreached += oracle_rows(key, csr, [a])[0][0, b] < 0
        check(ctx, key, csr, np.arange(csr.V), layout)
        check(ctx, key, csr, [b, a], layout)
    assert no_in >= 1 and unreached >= 1


# ----------------------------------------------------- 5. unaligned tables --

@pytest.mark.parametrize("layout", ["hops", "packed", "tree16", "slot32"])
def test_tables_not_16_byte_aligned(ctx, layout):
    """Odd V (no row is a whole number of 16-byte words) and every table, the
    u16 hop plane too, based 4 bytes off a 16-byte boundary; then rows of
    whole 16-byte words (fat_tree:8, V = 80) on such a base."""
    odd = [s for s in range(20) if planted(s)[0].V % 2 == 1][:3]
    assert len(odd) == 3
    for seed in odd:
        csr, a, b = planted(seed)
        ctx.upload(csr)
        key = "planted%d" % seed
        check(ctx, key, csr, np.arange(csr.V), layout, off=1)
        check(ctx, key, csr, [b, a], layout, off=3)
    csr = T.by_name("fat_tree:8").csr()
    ctx.upload(csr)
    check(ctx, "fat_tree:8", csr, np.arange(csr.V), layout, off=1)


# -------------------------------------------------------- 6. prep fallback --

@pytest.mark.parametrize("tables", ["lds", "global"])
@pytest.mark.parametrize("layout", ["packed", "hops"])
def test_prep_list_longer_than_lds_form(ctx, monkeypatch, layout, tables):
    """The prep kernel's short form holds 2,048 positions; one more takes the
    general path (and SDNROUTE_DFS_FOLD_LDS=0 its global class tables)."""
    if tables == "global":
        monkeypatch.setenv("SDNROUTE_DFS_FOLD_LDS", "0")
    name = "fat_tree:8"
    csr = T.by_name(name).csr()
    ctx.upload(csr)
    rng = np.random.default_rng(23)
    for n in (2047, 2048, 2049, 2500):
        ids = rng.integers(-1, csr.V + 1, n)
        assert check(ctx, name, csr, ids, layout) == 44
    # the leaders late in a long list: 2,100 copies of one vertex first
    ids = np.concatenate([np.full(2100, 5), rng.permutation(csr.V)])
    assert check(ctx, name, csr, ids, layout) == 44
