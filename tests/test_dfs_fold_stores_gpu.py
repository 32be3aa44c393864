"""The stores of the twin fold's derive kernel (csrc/dfs.hip, DESIGN.md 4.1e
"The derive kernel's store policy"): the copy stores of a row and the patch
stores that follow them in the same wave carry one cache policy, and a patch
has to land after the 16-, 4- or 2-byte copy store that covered its word,
whatever that policy is.

Every table is compared with the oracle bit for bit; the fold is forced, and
`last_launches` / `last_dfs_searched` (against `twin_reps()`) show that it ran.
The shapes are the smallest at which a change of the store policy can go
wrong:

* fat_tree:4 / fat_tree:8 (V = 20 / 80, rows of whole 16-byte vectors): the
  patches of a row inside one or two 16-byte stores of their wave, every layout;
* planted twins at V = 9 and 13 (no whole vectors): the 4-byte element path,
  and the 2-byte one under u16 depths;
* table 0 four bytes off a 16-byte boundary beside aligned tables: element
  and vector paths in one call;
* twins with 300 out-links (a patch list in chunks); twins whose row holds a
  parallel link (two patches for one column) are refused at upload, which is
  asserted, and the graph runs with the link once;
* leader, member, the member again, -1, V, the leader again: empty rows, a row
  twice, the leader's row copied as it is;
* one batch twice into one buffer with no host wait between the calls."""
import numpy as np
import pytest
import torch

from sdnmpi_amd import _native
from sdnmpi_amd import topologies as T
from test_dfs_twin_fold import LAYOUTS, csr_of
from test_dfs_fold_derive_gpu import check, classes_of, oracle_rows, planted

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def forced(monkeypatch):
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")


def searched(rep, srcs, V):
    srcs = np.asarray(srcs, np.int64)
    return len(np.unique(rep[srcs[(srcs >= 0) & (srcs < V)]]))


# ---------------------------------------------------------- 16-byte rows --

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["fat_tree:4", "fat_tree:8"])
def test_vector_rows(ctx, name, layout):
    csr = T.by_name(name).csr()
    assert csr.V in (20, 80)
    ctx.upload(csr)
    rep = ctx.twin_reps()
    big, _ = classes_of(rep)
    assert big
    key = "st_" + name
    check(ctx, key, csr, rep, np.arange(csr.V), layout)
    check(ctx, key, csr, rep, np.arange(csr.V)[::-1], layout)
    check(ctx, key, csr, rep, [big[0][1], big[0][0]], layout)


# ----------------------------------------------------------- element rows --

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("V", [9, 13])
def test_element_rows(ctx, V, layout):
    """int32 rows of 36 / 52 bytes, u16 rows of 18 / 26: no table on the
    16-byte path; seed 4 gives the pair no in-links (ls unreached from s)."""
    for seed, (a, b) in ((1, (3, 7)), (2, (V - 1, 0)), (4, (4, 5))):
        csr = planted(seed, V, a, b)
        ctx.upload(csr)
        rep = ctx.twin_reps()
        assert rep[a] == rep[b]
        key = "st_e%d_%d" % (V, seed)
        check(ctx, key, csr, rep, np.arange(V), layout)
        check(ctx, key, csr, rep, [b, a, b], layout)


# ------------------------------------------------- table 0 off by 4 bytes --

@pytest.mark.parametrize("layout", ["packed", "int32", "hops", "tree16", "slot32"])
def test_table0_off_a_vector_boundary(ctx, layout):
    """The rows are whole vectors, table 0 a view 4 bytes into a larger
    allocation: it takes the element path, the other tables the 16-byte one."""
    name = "fat_tree:8"
    csr = T.by_name(name).csr()
    ctx.upload(csr)
    rep = ctx.twin_reps()
    big, _ = classes_of(rep)
    check(ctx, "st_" + name, csr, rep, np.arange(csr.V), layout, (4, 0, 0))
    check(ctx, "st_" + name, csr, rep, [big[1][2], big[1][0], big[1][1]], layout, (4, 0, 0))


# ------------------------------------------------------------ patch lists --

@pytest.mark.parametrize("layout", ["packed", "hops", "tree16"])
def test_patch_list_in_chunks(ctx, layout):
    """Twins 0 and 1 with 300 out-links in 310 vertices: 302 patches a row."""
    rng = np.random.default_rng(11)
    V = 310
    adj = rng.random((V, V)) < 0.01
    adj[:, :2] = False
    adj[:2, :] = False
    adj[0, 5:305] = adj[1, 5:305] = True
    adj[9, :2] = adj[200, :2] = adj[309, :2] = True
    np.fill_diagonal(adj, False)
    csr = csr_of(adj, rng)
    ctx.upload(csr)
    rep = ctx.twin_reps()
    assert rep[1] == 0 and csr.row_ptr[1] - csr.row_ptr[0] == 300
    check(ctx, "st_wide", csr, rep, [1, 0, 9, 1], layout)
    check(ctx, "st_wide", csr, rep, [0, 1, -1, 1], layout)


def parallel_graph(parallel):
    """V = 12, twins 2 and 5; parallel: their rows hold column 7 twice, with
    two ports."""
    rng = np.random.default_rng(5)
    V, a, b, x = 12, 2, 5, 7
    adj = rng.random((V, V)) < 0.25
    np.fill_diagonal(adj, False)
    adj[a, :] = False
    adj[a, [1, x, 9]] = True
    adj[b, :] = adj[a, :]
    adj[:, b] = adj[:, a]
    adj[a, b] = adj[b, a] = adj[a, a] = adj[b, b] = False
    rows = [np.flatnonzero(adj[u]).tolist() for u in range(V)]
    if parallel:
        for u in (a, b):
            rows[u] = sorted(rows[u] + [x])
    col = np.concatenate([np.asarray(r, np.int64) for r in rows])
    row_ptr = np.zeros(V + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=row_ptr[1:])
    port = np.arange(100, 100 + col.size)            # every entry its own port
    return T.CSR(np.arange(1, V + 1), row_ptr, col, port), a, b


@pytest.mark.parametrize("layout", ["packed", "slots", "int32", "hops", "tree16"])
def test_parallel_link_in_the_twins_row(ctx, layout):
    """Two list entries for one column would leave it to the hardware which
    patch stays.  They cannot reach the kernel: a row with a parallel link is
    refused at upload (rows are strictly ascending; the topology keeps one link
    per ordered pair).  The same graph with the link once goes through."""
    csr, a, b = parallel_graph(True)
    with pytest.raises(_native.SdnrError, match="not strictly ascending"):
        ctx.upload(csr)
    csr, a, b = parallel_graph(False)
    ctx.upload(csr)
    rep = ctx.twin_reps()
    assert rep[a] == rep[b]
    check(ctx, "st_par", csr, rep, [a, b, 0, b], layout)
    check(ctx, "st_par", csr, rep, [b, a], layout)


# ------------------------------------------------------------- the batch --

@pytest.mark.parametrize("layout", LAYOUTS)
def test_leader_member_and_empty_rows(ctx, layout):
    name = "fat_tree:8"
    csr = T.by_name(name).csr()
    ctx.upload(csr)
    rep = ctx.twin_reps()
    big, _ = classes_of(rep)
    lead, member = big[0][0], big[0][1]
    check(ctx, "st_" + name, csr, rep, [lead, member, member, -1, csr.V, lead], layout)


# ------------------------------------------- two calls into one buffer --

@pytest.mark.parametrize("layout", ["packed", "hops"])
def test_two_calls_one_buffer(ctx, layout):
    """The stores of the second call follow those of the first to the same
    addresses, with no host wait in between."""
    name = "fat_tree:8"
    csr = T.by_name(name).csr()
    ctx.upload(csr)
    rep = ctx.twin_reps()
    dev = torch.device("cuda", ctx.device)
    S, V = csr.V, csr.V
    srcs = np.arange(V, dtype=np.int32)[::-1].copy()
    ts = torch.from_numpy(srcs).to(dev)
    n = 1 if layout == "packed" else 3
    out = [torch.full((S, V), 0x5A5A5A5A, dtype=torch.int32, device=dev) for _ in range(n)]
    for _ in range(2):
        if layout == "packed":
            ctx.dfs_tables_packed_device(ts.data_ptr(), S, out[0].data_ptr())
        else:
            ctx.dfs_tables_device(ts.data_ptr(), S, out[0].data_ptr(), out[1].data_ptr(),
                                  out[2].data_ptr())
    ctx.synchronize()
    assert ctx.last_launches() == 3
    assert ctx.last_dfs_searched() == searched(rep, srcs, V)
    po, to, ho = oracle_rows("st_" + name, csr, srcs)
    if layout == "packed":
        p, t = _native.unpack_tree(out[0].cpu().numpy().view(np.uint32))
    else:
        p, t = out[0].cpu().numpy(), out[1].cpu().numpy()
        np.testing.assert_array_equal(out[2].cpu().numpy(), ho)
    np.testing.assert_array_equal(p, po)
    np.testing.assert_array_equal(t, to)
