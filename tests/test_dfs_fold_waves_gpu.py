"""The folded search's wave count (csrc/dfs.hip, DESIGN.md 4.1e "the wave
count follows the live count").  When a folded call takes its form from the
count an earlier equal call published, the search is dispatched as that count
selects -- its wave count, rows, grid and name -- not as the caller's batch
size does: 34 live searches of a batch of 578 run the 8-wave kernel.  Without a
count (first call, new upload, new batch size, a forced form) the batch size
selects, as before.  Every table is compared with the oracle, bit for bit.

`fat_tree:34` (V = 1,445) is the smallest fat-tree whose in-rows are not
paired, so the smallest on which the rule applies: list A, its 578 edge
switches, is 34 classes; list B, its 578 aggregation switches, 578 classes of
their own.  The wave counts expected are computed from the device's CU count,
as `dfs_async_waves` does (8 up to 2 searches per CU, else 4)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from sdnmpi_amd import _native
from sdnmpi_amd import topologies as T

pytestmark = pytest.mark.gpu

KEY = "fat_tree:34"


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def fold_on(monkeypatch):
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")
    monkeypatch.delenv("SDNROUTE_DFS_FOLD_FORM", raising=False)
    monkeypatch.delenv("SDNROUTE_DFS_ASYNC_WAVES", raising=False)


_graphs = {}


def graph(key):
    """(csr, oracle tables of every vertex), built once per graph."""
    if key not in _graphs:
        csr = T.by_name(key).csr()
        _graphs[key] = (csr, O.dfs_tables(csr, np.arange(csr.V, dtype=np.int32), with_hops=True))
    return _graphs[key]


def k34_lists():
    fabric = T.by_name(KEY)
    csr = graph(KEY)[0]
    A = np.unique(fabric.host_table()[0]).astype(np.int32)
    nb = np.concatenate([csr.col[csr.row_ptr[s]:csr.row_ptr[s + 1]] for s in A])
    B = np.unique(nb).astype(np.int32)
    assert len(A) == 578 and len(B) == 578 and not np.intersect1d(A, B).size
    return A, B


def cus(ctx):
    return torch.cuda.get_device_properties(ctx.device).multi_processor_count


def waves(ctx, n):
    """dfs_async_waves for n searches on rows that are not paired."""
    return 8 if n <= 2 * cus(ctx) else 4


def name(nw, layout):
    if layout == "packed":
        return "dfs_async_kernel<%d,packed>" % nw
    if layout == "tree16":                       # 3, 4 and 6 waves exist with a depth plane
        return "dfs_async_kernel<%d,packed,hops>" % (3 if nw <= 3 else (6 if nw >= 6 else 4))
    return "dfs_async_kernel<%d>" % nw


def oracle_rows(key, srcs):
    """Oracle rows for the ids in srcs, empty rows for ids that are no vertex."""
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
    (form, kernel name) as the context reports them."""
    csr = graph(key)[0]
    srcs = np.asarray(srcs, np.int32)
    p, t, h = gpu_rows(ctx, csr, srcs, layout)
    assert ctx.last_launches() == 3
    got = (ctx.last_dfs_form(), ctx.last_kernel())
    po, to, ho = oracle_rows(key, srcs)
    np.testing.assert_array_equal(p, po)
    np.testing.assert_array_equal(t, to)
    if h is not None:
        np.testing.assert_array_equal(h, ho)
    return got


# ------------------------------------------------------ 1. life cycle of the name --

def test_name_life_cycle(ctx):
    A, B = k34_lists()
    assert len(A) > 2 * cus(ctx) >= 34           # a batch of the 4-wave kernel, a count of the 8-wave one
    by_nsrc = name(waves(ctx, len(A)), "packed")             # <4,packed>
    by_count = name(waves(ctx, 34), "packed")                # <8,packed>
    assert by_nsrc != by_count
    ctx.upload(graph(KEY)[0])
    assert check(ctx, KEY, A) == ("full", by_nsrc)           # nothing published yet
    assert ctx.last_dfs_searched() == 34
    assert check(ctx, KEY, A) == ("low", by_count)           # 34 live searches last time
    # B on A's stale count: 578 searches in the kernel that 34 select
    assert check(ctx, KEY, B) == ("low", by_count)
    assert ctx.last_dfs_searched() == 578
    assert check(ctx, KEY, B) == ("full", by_nsrc)           # 578 > 2 per CU
    # the same graph uploaded again: its counts are no hint
    ctx.upload(graph(KEY)[0])
    assert check(ctx, KEY, A) == ("full", by_nsrc)
    assert check(ctx, KEY, A) == ("low", by_count)
    # another batch size does not take A's count
    assert check(ctx, KEY, A[:-1]) == ("full", by_nsrc)


# ------------------------------------------- 2. layouts on the second equal call --

@pytest.mark.parametrize("layout", ["packed", "tree16", "int32", "hops"])
def test_layouts_on_the_second_equal_call(ctx, layout):
    A, _ = k34_lists()
    ctx.upload(graph(KEY)[0])
    assert check(ctx, KEY, A, layout) == ("full", name(waves(ctx, len(A)), layout))
    assert check(ctx, KEY, A, layout) == ("low", name(waves(ctx, 34), layout))
    assert ctx.last_dfs_searched() == 34


# ------------------------------------------------ 3. forced forms are untouched --

def test_forced_form_keeps_the_batch_size_wave_count(ctx, monkeypatch):
    A, _ = k34_lists()
    ctx.upload(graph(KEY)[0])
    check(ctx, KEY, A)
    assert check(ctx, KEY, A) == ("low", name(waves(ctx, 34), "packed"))     # hinted
    monkeypatch.setenv("SDNROUTE_DFS_FOLD_FORM", "low")
    assert check(ctx, KEY, A) == ("low", name(waves(ctx, len(A)), "packed"))
    monkeypatch.setenv("SDNROUTE_DFS_FOLD_FORM", "full")
    assert check(ctx, KEY, A) == ("full", name(waves(ctx, len(A)), "packed"))


def test_wave_override_wins_over_the_count(ctx, monkeypatch):
    A, _ = k34_lists()
    ctx.upload(graph(KEY)[0])
    check(ctx, KEY, A)
    monkeypatch.setenv("SDNROUTE_DFS_ASYNC_WAVES", "5")
    assert check(ctx, KEY, A) == ("low", "dfs_async_kernel<5,packed>")       # hinted


# --------------------------------------------------- 4. host ahead of the device --

def test_host_runs_ahead_of_the_device(ctx):
    """One call, then twenty equal ones queued without a wait: each finds the
    count of whichever of them the device has finished."""
    A, _ = k34_lists()
    csr = graph(KEY)[0]
    ctx.upload(csr)
    assert check(ctx, KEY, A)[0] == "full"
    dev = torch.device("cuda", ctx.device)
    ts = torch.from_numpy(A).to(dev)
    out = torch.empty((len(A), csr.V), dtype=torch.int32, device=dev)
    got = []
    for _ in range(20):
        ctx.dfs_tables_packed_device(ts.data_ptr(), len(A), out.data_ptr())
        got.append((ctx.last_dfs_form(), ctx.last_kernel()))
    ctx.synchronize()
    assert got == [("low", name(waves(ctx, 34), "packed"))] * 20
    p, t = _native.unpack_tree(out.cpu().numpy().view(np.uint32))
    po, to, _ = oracle_rows(KEY, A)
    np.testing.assert_array_equal(p, po)
    np.testing.assert_array_equal(t, to)


# ------------------------------------------- 5. awkward lists in the 8-wave form --

@pytest.mark.parametrize("layout", ["packed", "hops"])
def test_awkward_list_on_the_hint(ctx, layout):
    """578 ids, so the list runs on A's count: the leaders of some classes,
    then non-leaders of the same classes in reverse order, repeats, -1 and V
    in between, and a few aggregation switches."""
    A, B = k34_lists()
    csr = graph(KEY)[0]
    ctx.upload(csr)
    rep = np.asarray(ctx.twin_reps())
    leaders = A[rep[A] == A]
    assert len(leaders) == 34
    others = np.array([A[(rep[A] == r) & (A != r)][-1] for r in leaders[:20]], np.int32)
    parts = [leaders[:20], np.array([-1, csr.V], np.int32), others[::-1], leaders[5:10],
             B[:7], np.array([csr.V, -1], np.int32), others[:12]]
    head = np.concatenate(parts).astype(np.int32)
    ids = np.concatenate([head, np.resize(others, len(A) - len(head))]).astype(np.int32)
    assert len(ids) == len(A)
    check(ctx, KEY, A, layout)
    assert check(ctx, KEY, ids, layout) == ("low", name(waves(ctx, 34), layout))
    ok = (ids >= 0) & (ids < csr.V)
    assert ctx.last_dfs_searched() == len(np.unique(rep[ids[ok]])) == 27


# --------------------------------------------- 6. the benchmark's own path, once --

def test_k48_second_call(ctx):
    """k=48, its 1,152 edge switches, packed tables: the call the benchmark
    times is the second and later ones."""
    fabric = T.by_name("fat_tree:48")
    csr = fabric.csr()
    srcs = np.unique(fabric.host_table()[0]).astype(np.int32)
    assert len(srcs) == 1152
    po, to, _ = O.dfs_tables(csr, srcs, with_hops=False, nthreads=8)
    ctx.upload(csr)
    names = []
    for _ in range(2):
        p, t, _ = gpu_rows(ctx, csr, srcs, "packed")
        assert ctx.last_launches() == 3 and ctx.last_dfs_searched() == 48
        names.append((ctx.last_dfs_form(), ctx.last_kernel()))
        np.testing.assert_array_equal(p, po)
        np.testing.assert_array_equal(t, to)
    assert names == [("full", name(waves(ctx, 1152), "packed")),
                     ("low", name(waves(ctx, 48), "packed"))]
