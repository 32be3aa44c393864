"""The quotient's flush in dfs_async_kernel (csrc/dfs.hip, DESIGN.md 4.1e, "The
quotient's flush"): a class's slot-table offset is kept in LDS by the worker
that drains the class, and the tree link's port comes from the composed table
(the root's children: from the root's own row in LDS).  Every table is compared
bit for bit with the oracle, with the async strategy and the quotient forced so
that small graphs take the path (tests/test_dfs_quotient_flush.py states the
expansion in Python)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from sdnmpi_amd import _native
from sdnmpi_amd import topologies as T

import boundary_graphs as B
import golden_util as G
from test_dfs_quotient import Quotient, planted

pytestmark = pytest.mark.gpu

LAYOUTS = ["int32", "hops", "packed", "tree16", "slots"]
KNOBS = ("SDNROUTE_DFS_QUOTIENT", "SDNROUTE_DFS_FOLD", "SDNROUTE_DFS_FOLD_FORM",
         "SDNROUTE_DFS_ASYNC_WAVES", "SDNROUTE_DFS_STRATEGY", "SDNROUTE_DFS_C16",
         "SDNROUTE_DFS_PRESWZ", "SDNROUTE_DFS_DW", "SDNROUTE_ELL")
# planted(seed) of test_dfs_quotient.py: 12 and 16 have twins without in-links
# (a class no other root reaches, class mates nobody reaches), 5 and 10 a class
# of three
SEEDS = (3, 5, 10, 12, 16, 21)


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def forced(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDNROUTE_DFS_STRATEGY", "async")
    monkeypatch.setenv("SDNROUTE_DFS_QUOTIENT", "1")


def with_ports(csr, ports):
    return T.CSR(np.arange(1, csr.V + 1), csr.row_ptr, csr.col, ports)


def hub():
    """90 switches: 0 links to the 40 twins 1 .. 40, which link on to 41 and 42;
    41 -> 0, 42 -> 43 -> ... -> 89 a path, 50 and 51 twins off it.  One long row
    among short ones: the padded rows would be more than twice the links, so
    the ports stay in the CSR arrays."""
    rng = np.random.default_rng(90)
    adj = np.zeros((90, 90), bool)
    adj[0, 1:41] = True
    adj[1:41, 41] = adj[1:41, 42] = True
    adj[41, 0] = True
    for u in range(42, 89):
        adj[u, u + 1] = True
    adj[51, :] = adj[50, :]
    adj[:, 51] = adj[:, 50]
    adj[50, 51] = adj[51, 50] = adj[51, 51] = False
    rows, cols = np.nonzero(adj)
    row_ptr = np.zeros(91, np.int64)
    np.cumsum(np.bincount(rows, minlength=90), out=row_ptr[1:])
    return T.CSR(np.arange(1, 91), row_ptr, cols, rng.integers(0, 60000, size=cols.size))


def ring_twins(V):
    """boundary_graphs.ring(V) with three pairs of twins, one of them the last
    vertex: V - 3 classes, a quotient nearly the graph's size."""
    csr = B.ring(V)
    for a, b in ((10, 300), (20, 500), (5, V - 1)):
        csr = B.with_twins(csr, a, b)
    return csr


_graphs = {}


def graph(key):
    """(csr, oracle tables of every vertex), built once per graph."""
    if key not in _graphs:
        if key.startswith("planted"):
            csr = planted(int(key[7:]))
        elif key.startswith("wide"):             # ports beyond 16 bits: the int32 layouts only
            csr = planted(int(key[4:]))
            rng = np.random.default_rng(int(key[4:]))
            csr = with_ports(csr, rng.integers(65536, 1 << 30, size=csr.col.size))
        elif key == "hub":
            csr = hub()
        elif key.startswith("ring"):
            csr = ring_twins(int(key[4:]))
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


def check(ctx, key, srcs, layout, upload=True, quotient=1):
    """One call against the oracle, on the quotient and in the async kernel."""
    csr = graph(key)[0]
    srcs = np.asarray(srcs, np.int32)
    if upload:
        ctx.upload(csr)
    po, to, ho = oracle_rows(key, srcs)
    p, t, h = gpu_rows(ctx, csr, srcs, layout)
    assert ctx.last_dfs_quotient() == quotient
    assert ctx.last_kernel().startswith("dfs_async_kernel<"), ctx.last_kernel()
    np.testing.assert_array_equal(p, po)
    np.testing.assert_array_equal(t, to)
    if h is not None:
        np.testing.assert_array_equal(h, ho)


def every_id(key):
    V = graph(key)[0].V
    return np.concatenate([np.arange(V), [-1, V]]).astype(np.int32)


SMALL = ["fat_tree:4", "fat_tree:8", "hub"] + ["planted%d" % s for s in SEEDS]


# ---------------------------------------------------------------- every root --

def test_the_graphs_hold_every_case():
    """By assertion: roots that are their class's largest member, another
    member, a class of one; root children whose port from the root is not the
    port from the class's largest member; classes never pushed and class mates
    nobody reaches; a member of rank 2."""
    seen = dict.fromkeys(["largest", "other", "single", "other_port", "never_pushed",
                          "mates_unreachable", "rank2"], 0)
    for key in SMALL:
        csr, (po, to, _) = graph(key)
        q = Quotient(csr)
        V = csr.V
        rank = [sum(1 for x in range(v) if q.cid[x] == q.cid[v]) for v in range(V)]
        seen["rank2"] += max(rank) >= 2
        for s in range(V):
            C = q.cid[s]
            seen["single" if q.size[C] == 1 else ("largest" if q.cmax[C] == s else "other")] += 1
            for v in np.nonzero(po[s] == s)[0]:
                if v != s and s != q.cmax[C]:
                    seen["other_port"] += to[s][v] != q.port_of[(q.cmax[C], int(v))]
            mates = [v for v in range(V) if q.cid[v] == C and v != s]
            seen["mates_unreachable"] += bool(mates) and not (po[s][mates] >= 0).any()
            for c in range(len(q.size)):
                if q.size[c] > 1 and c != C:
                    seen["never_pushed"] += not any(po[s][v] >= 0 for v in range(V)
                                                    if q.cid[v] == c)
    assert all(n > 0 for n in seen.values()), seen


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("key", SMALL + G.LOOPS)
def test_every_root(ctx, key, layout):
    ctx.upload(graph(key)[0])
    rep = np.asarray(ctx.twin_reps())
    twins = int(np.any(rep != np.arange(len(rep))))
    if key in SMALL:
        assert twins == 1
    check(ctx, key, every_id(key), layout, upload=False, quotient=twins)


@pytest.mark.parametrize("layout", ["int32", "hops"])
@pytest.mark.parametrize("key", ["wide5", "wide12"])
def test_ports_beyond_16_bits(ctx, key, layout):
    assert graph(key)[0].port.min() >= 65536
    check(ctx, key, every_id(key), layout)


@pytest.mark.parametrize("ell", ["1", "0"], ids=["ell_ports", "csr_ports"])
@pytest.mark.parametrize("layout", ["int32", "packed"])
@pytest.mark.parametrize("key", ["fat_tree:8", "planted5", "hub"])
def test_both_port_paths(ctx, monkeypatch, key, layout, ell):
    """The root's port row comes from the padded rows where the upload made
    them, else from the CSR arrays; SDNROUTE_ELL=0 keeps any graph on the
    latter, and the hub's rows are never padded."""
    if ell == "0":
        monkeypatch.setenv("SDNROUTE_ELL", "0")
    csr = graph(key)[0]
    deg = np.diff(csr.row_ptr)
    padded = csr.V * int(deg.max()) <= 2 * csr.col.size + 64
    assert padded == (key != "hub")
    check(ctx, key, every_id(key), layout)


# ------------------------------ several sources over one workgroup's LDS state --

@pytest.mark.parametrize("waves", ["2", "8"])
@pytest.mark.parametrize("layout", ["packed", "hops"])
@pytest.mark.parametrize("key", ["planted12", "planted16", "hub"])
def test_sparse_sources_after_full_ones(ctx, monkeypatch, key, layout, waves):
    """Unfolded, a batch of twice the largest grid (16 workgroups of 2 waves
    per CU): every workgroup first searches sources that reach the most, then
    -- over the same LDS words -- every root in turn, those that push few
    classes, leave class mates unreached or are reached by no one among them.
    An offset word of an earlier source must not be read."""
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "0")
    monkeypatch.setenv("SDNROUTE_DFS_ASYNC_WAVES", waves)
    csr, (po, _, _) = graph(key)
    V = csr.V
    half = 16 * torch.cuda.get_device_properties(ctx.device).multi_processor_count
    reach = (po >= 0).sum(axis=1)
    full = np.nonzero(reach == reach.max())[0]
    assert reach.min() < reach.max()
    ids = np.concatenate([np.resize(full, half), np.resize(np.arange(V), half)])
    check(ctx, key, ids, layout)


# --------------------------------------------------------------------- forms --

@pytest.mark.parametrize("layout", ["packed", "hops", "tree16"])
@pytest.mark.parametrize("waves", ["2", "3", "4", "5", "6", "8"])
def test_wave_counts(ctx, monkeypatch, waves, layout):
    monkeypatch.setenv("SDNROUTE_DFS_ASYNC_WAVES", waves)
    for key in ("fat_tree:8", "planted10"):
        check(ctx, key, every_id(key), layout)


@pytest.mark.parametrize("layout", ["packed", "hops"])
@pytest.mark.parametrize("knob,value", [("SDNROUTE_DFS_C16", "1"), ("SDNROUTE_DFS_PRESWZ", "0"),
                                        ("SDNROUTE_DFS_DW", "0"), ("SDNROUTE_DFS_DW", "1")])
def test_row_forms(ctx, monkeypatch, knob, value, layout):
    monkeypatch.setenv(knob, value)
    for waves in ("4", "8"):
        monkeypatch.setenv("SDNROUTE_DFS_ASYNC_WAVES", waves)
        for key in ("fat_tree:8", "planted5", "hub"):
            check(ctx, key, every_id(key), layout)


@pytest.mark.parametrize("form", ["low", "full"])
@pytest.mark.parametrize("layout", ["packed", "tree16", "hops"])
def test_folded_forms(ctx, monkeypatch, form, layout):
    monkeypatch.setenv("SDNROUTE_DFS_FOLD", "1")
    monkeypatch.setenv("SDNROUTE_DFS_FOLD_FORM", form)
    for key in ("fat_tree:8", "planted10"):      # paired rows: one form whatever is asked
        check(ctx, key, every_id(key), layout)
        assert ctx.last_launches() == 3
        check(ctx, key, every_id(key)[::-1].copy(), layout, upload=False)   # a second call
        assert ctx.last_launches() == 3
    # rows of 34 in-neighbours: the forced form is the one that runs; two pods'
    # edge switches, some aggregation and core switches, ids that are none
    key = "fat_tree:34"
    fabric = T.by_name(key)
    csr = graph(key)[0]
    edge = np.unique(fabric.host_table()[0]).astype(np.int32)
    ids = np.concatenate([edge[:34], edge[34:40][::-1], [-1, csr.V, csr.V - 1, csr.V - 40],
                          csr.col[csr.row_ptr[edge[0]]:csr.row_ptr[edge[0]] + 5]])
    for _ in range(2):
        check(ctx, key, ids, layout, upload=_ == 0)
        assert ctx.last_launches() == 3 and ctx.last_dfs_form() == form


# ------------------------------------ the flush's pass size, a quotient of nearly V --

@pytest.mark.parametrize("layout", ["packed", "hops"])
@pytest.mark.parametrize("V", [767, 768, 769])
def test_rows_around_one_pass(ctx, monkeypatch, V, layout):
    """2 waves flush 6 x 128 = 768 vertices per pass.  The graphs have V - 3
    classes: the quotient's layout with the flush's words is larger than the
    graph's own, which the launch then reserves."""
    monkeypatch.setenv("SDNROUTE_DFS_ASYNC_WAVES", "2")
    key = "ring%d" % V
    csr = graph(key)[0]
    assert csr.V == V
    ctx.upload(csr)
    rep = np.asarray(ctx.twin_reps())
    assert len(np.unique(rep)) == V - 3
    check(ctx, key, every_id(key), layout, upload=False)
    monkeypatch.setenv("SDNROUTE_DFS_ASYNC_WAVES", "8")
    check(ctx, key, [5, V - 1, 10, 300, 0, V - 3, 7], layout, upload=False)


# --------------------------------------------- the benchmark's own path, once --

def test_k48_second_call(ctx, monkeypatch):
    """k=48, its 1,152 edge switches, packed tables, nothing forced: the call
    the benchmark times is the second and later ones."""
    monkeypatch.delenv("SDNROUTE_DFS_STRATEGY")
    monkeypatch.delenv("SDNROUTE_DFS_QUOTIENT")
    fabric = T.by_name("fat_tree:48")
    csr = fabric.csr()
    srcs = np.unique(fabric.host_table()[0]).astype(np.int32)
    assert len(srcs) == 1152
    po, to, _ = O.dfs_tables(csr, srcs, with_hops=False, nthreads=8)
    ctx.upload(csr)
    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    seen = []
    for _ in range(2):
        p, t, _ = gpu_rows(ctx, csr, srcs, "packed")
        seen.append((ctx.last_dfs_quotient(), ctx.last_launches(), ctx.last_dfs_searched(),
                     ctx.last_dfs_form(), ctx.last_kernel()))
        np.testing.assert_array_equal(p, po)
        np.testing.assert_array_equal(t, to)
    nw = [8 if n <= 2 * cus else 4 for n in (1152, 48)]
    assert seen == [(1, 3, 48, "full", "dfs_async_kernel<%d,packed>" % nw[0]),
                    (1, 3, 48, "low", "dfs_async_kernel<%d,packed>" % nw[1])]
