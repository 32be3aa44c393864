"""fair_times.hip (sdnr_fair_times) on the GPU against engine.fair_times_host,
and the drop-in's completion times against the engine double of
test_fair_times.py.  The definition is deterministic: every comparison is on
the bits of the times, the rates, the bytes left and carried, and on equal
epochs and rounds.  The launch count of every call is the documented function
of the restatement's epochs and rounds: the host read nothing in between but
the status word of each batch."""
import types

import numpy as np
import pytest

import boundary_graphs as BG
import golden_util as G
import over_grid as OG
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from test_ecmp_link_loads import edge_map
from test_fair_rates import CAPS, dropin_pairs, layout_tree, line_csr, line_to_end, small_case
from test_fair_times import FABRICS, fake_db

pytestmark = pytest.mark.gpu

LAYOUTS = (EN.INT32, EN.PORT16, EN.SLOT)
LDS, GLOBAL = "fair_times_rows_kernel<lds>", "fair_times_rows_kernel<global>"
NAMES = ("time", "epoch", "rate0", "remaining", "epoch_time", "epoch_rounds", "carried")


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def on(csr):
    """The export-shaped handle RouteEngine wants for a bare CSR."""
    return types.SimpleNamespace(csr=csr)


def dev_tree(eng, tree):
    import torch
    a = np.ascontiguousarray(tree)
    if a.dtype != np.int32:
        a = a.astype(np.uint32).view(np.int32) if a.dtype != np.uint32 else a.view(np.int32)
    return torch.from_numpy(a).to(eng.dev)


def same(got, want):
    """Every output equal bit for bit."""
    for g, w, name in zip(got, want, NAMES):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if g.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), name
        else:
            assert np.array_equal(g, w), name


def run(eng, want, csr, tree, layout, rows, verts, mult, nbytes, cap, extra=None, to_root=False,
        kernel=LDS, max_epochs=None):
    """One case on the device; it must be what the restatement gave."""
    got = eng.fair_times(on(csr), dev_tree(eng, tree), layout, rows, verts, mult, nbytes, cap,
                         extra, to_root=to_root, max_epochs=max_epochs)
    same(got, want)
    assert eng.ctx.last_kernel() == kernel
    assert eng.ctx.last_launches() == EN.fair_times_launches(want[5])


def both(eng, csr, tree, layout, rows, verts, mult, nbytes, cap, extra=None, to_root=False,
         kernel=LDS, max_epochs=None):
    want = EN.fair_times_host(csr, tree, layout, rows, verts, mult, nbytes, cap, extra, to_root,
                              max_epochs)
    run(eng, want, csr, tree, layout, rows, verts, mult, nbytes, cap, extra, to_root, kernel,
        max_epochs)
    return want


def seeded_bytes(name, n):
    return np.random.default_rng(900 + G.SMALL.index(name)).integers(1, 1001, n).astype(np.float64)


# ------------------------------------------------------------ closed forms --

def test_one_link_and_three_flow_line(eng):
    csr = line_csr(1)
    nh, fwd = line_to_end(csr)
    cap = np.full(csr.E, 7.0)
    cap[fwd[0]] = 3.0
    r = both(eng, csr, nh, EN.INT32, [0, 0], [0, 0], None, [3.0, 6.0], cap, to_root=True)
    assert r[0].tolist() == [2.0, 3.0] and r[1].tolist() == [0, 1]
    csr = line_csr(2)
    em = edge_map(csr)
    cap = np.ones(csr.E)
    cap[em[(1, 2)]] = 2.0
    nh = np.array([[1, 2, -1], [1, -1, 1]], np.int32)
    r = both(eng, csr, nh, EN.INT32, [0, 1, 0], [0, 0, 1], None, [1.0, 2.0, 6.0], cap,
             to_root=True)
    assert r[0].tolist() == [2.0, 3.0, 3.5] and r[1].tolist() == [0, 1, 2]
    assert r[5].tolist() == [2, 2, 1]
    # the same flows in the trees of sources 0 and 1
    par = np.array([[0, 0, 1], [1, 1, 1]], np.int32)
    r = both(eng, csr, par, EN.INT32, [0, 0, 1], [2, 1, 2], None, [1.0, 2.0, 6.0], cap)
    assert r[0].tolist() == [2.0, 3.0, 3.5]


# ------------------------------------------------------ the small fabrics --

@pytest.mark.parametrize("name", FABRICS)
def test_small_fabrics_to_completion_all_layouts_and_to_root(eng, name):
    c = small_case(name)
    csr, rows, verts, mult, cap = c["csr"], c["rows"], c["verts"], c["mult"], c["cap"]
    nbytes = seeded_bytes(name, rows.shape[0])
    want = EN.fair_times_host(csr, c["par"], EN.INT32, rows, verts, mult, nbytes, cap)
    assert len(want[4]) > 8 and (want[1] != -2).all()
    for lay in LAYOUTS:
        if lay == EN.SLOT and np.diff(csr.row_ptr).max() > 62:
            continue
        run(eng, want, csr, layout_tree(c, lay), lay, rows, verts, mult, nbytes, cap)
    both(eng, csr, c["nh"], EN.INT32, rows, verts, mult, nbytes, cap, to_root=True)


@pytest.mark.parametrize("name", ["fat_tree_k8", "dragonfly_a4_h2_p2", "jellyfish_n60_r5"])
def test_larger_fabrics_four_epochs(eng, name):
    c = small_case(name)
    csr, rows, verts, mult, cap = c["csr"], c["rows"], c["verts"], c["mult"], c["cap"]
    nbytes = seeded_bytes(name, rows.shape[0])
    r = both(eng, csr, c["par"], EN.INT32, rows, verts, mult, nbytes, cap, max_epochs=4)
    assert len(r[4]) == 4 and (r[1] == -2).any() and (r[1] >= 0).any()
    r = both(eng, csr, c["nh"], EN.INT32, rows, verts, None, nbytes, cap, to_root=True,
             max_epochs=4)
    assert len(r[4]) == 4 and (r[1] == -2).any() and r[5].min() >= 1


# ------------------------------------------------------------ path graphs --

def path_case(V):
    """cap[v -> v + 1] = (v + 1)^2 and a flow from every vertex with (2v + 1)
    (n - v) bytes: flow v runs at 2v + 1 throughout and ends at n - v, one flow
    per epoch, and epoch j's filling has n - j rounds."""
    n = V - 1
    csr = line_csr(n)
    nh, fwd = line_to_end(csr)
    cap = np.ones(csr.E)
    cap[fwd] = (np.arange(n) + 1.0) ** 2
    v = np.arange(V)
    return csr, nh, cap, v, (2.0 * v + 1) * (n - v)


@pytest.mark.parametrize("V", [3, 20, 40])
def test_path_graphs_one_flow_per_epoch_to_completion(eng, V):
    """20 and 40 vertices run more than 16 epochs and fillings of more than 16
    rounds: the clock survives the batch boundaries of both."""
    csr, nh, cap, v, nbytes = path_case(V)
    r = both(eng, csr, nh, EN.INT32, np.zeros(V, np.int64), v, None, nbytes, cap, to_root=True)
    n = V - 1
    assert r[1].tolist() == list(range(n - 1, -1, -1)) + [-1]
    assert r[0][:n].tolist() == (n - v[:n]).astype(np.float64).tolist() and r[0][n] == 0.0
    assert r[5].tolist() == list(range(n, 0, -1)) and r[2][n] == np.inf


@pytest.mark.parametrize("V", [65, 130])
def test_path_graphs_three_epochs(eng, V):
    """65 and 130 vertices make the doublings cross the wave and the workgroup
    stride."""
    csr, nh, cap, v, nbytes = path_case(V)
    r = both(eng, csr, nh, EN.INT32, np.zeros(V, np.int64), v, None, nbytes, cap, to_root=True,
             max_epochs=3)
    assert r[4].tolist() == [1.0, 2.0, 3.0] and r[5].tolist() == [V - 1, V - 2, V - 3]
    assert (r[1][:V - 4] == -2).all() and r[1][V - 4:].tolist() == [2, 1, 0, -1]


# -------------------------------------------------- LDS and global scratch --

@pytest.mark.parametrize("V,kernel", [(EN.FAIR_LDS_MAX_V, LDS), (EN.FAIR_LDS_MAX_V + 1, GLOBAL)])
def test_both_sides_of_the_lds_threshold(eng, V, kernel):
    from test_fair_rates_gpu import star_with_tail
    csr, nh = star_with_tail(V)
    assert csr.V == V
    em = edge_map(csr)
    verts = np.array([V - 1, V - 2, 5, 5, 1, 2, 0, 3])
    mult = np.array([2, 1, 3, 1, 1, 4, 1, 1], np.uint64)
    nbytes = np.array([40.0, 7.0, 900.0, 13.0, 250.0, 5.0, 77.0, 9.0])
    cap = np.random.default_rng(V).choice(np.asarray(CAPS, np.float64), int(csr.E))
    cap[[em[(0, 1)], em[(1, 2)], em[(2, 3)]]] = [50.0, 30.0, 60.0]
    r = both(eng, csr, nh, EN.INT32, np.zeros(8, np.int64), verts, mult, nbytes, cap,
             to_root=True, kernel=kernel)
    assert len(r[4]) >= 3 and (r[1][:7] >= 0).all() and r[0][7] == 0.0


@pytest.mark.parametrize("V", [65536, 65537])
def test_vertex_id_boundaries(eng, V):
    csr = BG.chain(V)
    nh = np.arange(1, V + 1, dtype=np.int32).reshape(1, V)
    nh[0, V - 1] = -1
    verts = np.array([V - 2, V - 3, 65534, 32768, 0, V - 1, V])
    nbytes = np.array([9.0, 100.0, 31.0, 64.0, 5.0, 3.0, 3.0])
    cap = np.random.default_rng(V).choice(np.asarray(CAPS, np.float64), int(csr.E))
    r = both(eng, csr, nh, EN.INT32, np.zeros(7, np.int64), verts, None, nbytes, cap,
             to_root=True, kernel=GLOBAL)
    assert (r[1][:5] >= 0).all() and r[0][5] == 0.0 and r[0][6] == np.inf and len(r[4]) >= 3


# ----------------------------------------------------------- special inputs --

def test_big_multiplicities_extras_zero_bytes_roots_and_unrouted(eng):
    csr = line_csr(2)
    nh, fwd = line_to_end(csr)
    E = csr.E
    cap = np.full(E, 3.0 * (1 << 40))
    cap[fwd[1]] *= 2
    mult = np.array([(1 << 32) - 1, 1 << 33, 5, (1 << 52) - (1 << 34)], np.uint64)
    r = both(eng, csr, nh, EN.INT32, [0, 0, 0, 0], [0, 0, 1, 0], mult, [8.0, 1.0, 4.0, 2.0], cap,
             to_root=True)
    assert (r[1] >= 0).all() and len(r[4]) == 4 and r[1][2] == 0
    # extras, a flow at the root with and without them, zero bytes, unrouted
    cap = np.concatenate([np.full(E, 10.0), [4.0, 1.0, 6.0]])
    extra = np.array([[E + 1, -1], [-1, -1], [E, E + 2], [-1, E + 2], [E + 2, E + 2], [E, -1],
                      [-1, -1], [-1, -1]])
    verts = [0, 2, 2, 1, 1, 0, 7, -1]
    nbytes = [3.0, 5.0, 8.0, 20.0, 6.0, 0.0, 4.0, 4.0]
    r = both(eng, csr, nh, EN.INT32, [0] * 8, verts, None, nbytes, cap, extra, to_root=True)
    assert r[0][1] == 0.0 and r[2][1] == np.inf and r[0][5] == 0.0 and r[2][5] == 0.0
    assert np.isinf(r[0][6:]).all() and (r[1][[1, 5, 6, 7]] == -1).all()
    assert (r[1][[0, 2, 3, 4]] >= 0).all() and r[6][E:].all()
    both(eng, csr, nh, EN.INT32, [0] * 8, verts, [2, 1, 3, 0, 1, 1, 1, 1], nbytes, cap, extra,
         to_root=True, max_epochs=2)
    both(eng, csr, nh, EN.INT32, [0] * 8, verts, None, nbytes, cap, extra, to_root=True,
         max_epochs=0)
    # the tree of source 0 with 2 unreached
    par = np.array([[0, 0, -1]], np.int32)
    r = both(eng, csr, par, EN.INT32, [0] * 4, [1, 1, 2, 0], [1, 3, 1, 1], [0.0, 5.0, 4.0, 1.0],
             cap[:E])
    assert r[0][2] == np.inf and r[0][3] == 0.0 and r[0][0] == 0.0


def raw(eng, csr, tree, nrows, off, verts, nbytes, cap, max_epochs=None, to_root=True):
    """One sdnr_fair_times call on device copies; returns (epochs, outputs,
    inputs) without synchronize."""
    import torch
    eng.load(on(csr))
    n = len(verts)
    me = n if max_epochs is None else max_epochs
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(eng.dev)  # noqa
    keep = [dev_tree(eng, tree), t(off, np.int64), t(verts, np.int32), t(nbytes, np.float64),
            t(cap, np.float64)]
    f64 = lambda k: torch.full((max(k, 1),), 7.0, dtype=torch.float64, device=eng.dev)  # noqa
    i32 = lambda k: torch.full((max(k, 1),), 7, dtype=torch.int32, device=eng.dev)      # noqa
    out = [f64(n), i32(n), f64(n), f64(n), f64(me), i32(me), f64(len(cap))]
    torch.cuda.synchronize()
    p = lambda x: x.data_ptr()    # noqa: E731
    epochs = eng.ctx.fair_times_device(p(keep[0]), _native.TREE_INT32, nrows, p(keep[1]),
                                       p(keep[2]), 0, p(keep[3]), 0, p(keep[4]), 0, p(out[0]),
                                       p(out[1]), p(out[2]), p(out[3]), p(out[4]), p(out[5]), me,
                                       p(out[6]), to_root=to_root)
    return epochs, out, keep


def test_no_rows_and_no_pairs(eng):
    csr = line_csr(2)
    eng.load(on(csr))
    assert eng.ctx.fair_times_device(0, _native.TREE_INT32, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                     0, 0, 0, 0) == 0
    nh = np.array([[1, 2, -1]], np.int32)
    epochs, out, keep = raw(eng, csr, nh, 1, [2, 2], [0, 0, 0], [1.0] * 3, np.ones(csr.E))
    eng.ctx.synchronize()
    assert epochs == 0 and all(float(o.cpu()[0]) == 7 for o in out)       # nothing touched
    r = eng.fair_times(on(csr), dev_tree(eng, nh), EN.INT32, [], [], None, [], np.ones(csr.E),
                       to_root=True)
    assert [len(x) for x in r] == [0] * 6 + [csr.E]
    del keep


def check_raw(eng, epochs, out, csr, tree, rows, verts, nbytes, cap, good, absent, what):
    """The call reported ``what`` once as SDNR_ERR_INVAL; the flows ``good``
    are what they are alone and the flows ``absent`` read +inf / -1 / 0.0."""
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "sdnr_fair_times" in str(ei.value) and what in str(ei.value)
    eng.ctx.synchronize()                                  # reported once
    want = EN.fair_times_host(csr, tree, EN.INT32, np.asarray(rows)[good],
                              np.asarray(verts)[good], None, np.asarray(nbytes)[good], cap,
                              to_root=True)
    got = [o.cpu().numpy() for o in out]
    assert epochs == len(want[4]) > 0
    for k in range(4):
        assert np.array_equal(got[k][good].view(np.uint8), want[k].view(np.uint8)), NAMES[k]
    assert np.array_equal(got[4][:epochs].view(np.uint64), want[4].view(np.uint64))
    assert np.array_equal(got[5][:epochs], want[5])
    assert np.array_equal(got[6].view(np.uint64), want[6].view(np.uint64))
    assert np.isinf(got[0][absent]).all() and (got[1][absent] == -1).all()
    assert not got[2][absent].any()


def test_cycle_row_and_bad_offsets_are_reported_not_followed(eng):
    csr = line_csr(3)
    nh = np.array([[1, 2, 3, -1], [1, 0, 3, -1], [1, 2, 3, -1], [-1, 0, 1, 2]], np.int32)
    tree = np.concatenate([nh, nh[3:]])
    cap = np.arange(1, csr.E + 1, dtype=np.float64)
    verts = [0, 1, 2, 0, 1, 2, 1, 3, 2]
    nbytes = [5.0, 9.0, 2.0, 4.0, 4.0, 4.0, 7.0, 1.0, 30.0]
    off = [0, 3, 5, 100, 6, 9]                  # row 2 = [5, 100), row 3 = [100, 6): both bad
    epochs, out, keep = raw(eng, csr, tree, 5, off, verts, nbytes, cap)
    good = [0, 1, 2, 6, 7, 8]
    rows = [0, 0, 0, 1, 1, 2, 4, 4, 4]
    check_raw(eng, epochs, out, csr, tree, rows, verts, nbytes, cap, good, [3, 4, 5], "tree")
    # the context goes on working
    r = eng.fair_times(on(csr), dev_tree(eng, nh[:1]), EN.INT32, [0], [0], None, [2.0], cap,
                       to_root=True)
    assert r[0].tolist() == [2.0 / cap[edge_map(csr)[(0, 1)]]]
    del keep


@pytest.mark.parametrize("bad", [-2.0, float("nan"), float("inf")])
def test_bad_byte_sizes_are_reported_and_absent(eng, bad):
    csr = line_csr(3)
    nh = np.array([[1, 2, 3, -1], [-1, 0, 1, 2]], np.int32)
    cap = np.arange(1, csr.E + 1, dtype=np.float64)
    verts = [0, 1, 2, 1, 3, 2]
    nbytes = [5.0, bad, 2.0, 7.0, 1.0, 30.0]
    with pytest.raises(ValueError):
        eng.fair_times(on(csr), dev_tree(eng, nh), EN.INT32, [0, 0, 0, 1, 1, 1], verts, None,
                       nbytes, cap, to_root=True)
    epochs, out, keep = raw(eng, csr, nh, 2, [0, 3, 6], verts, nbytes, cap)
    check_raw(eng, epochs, out, csr, nh, [0, 0, 0, 1, 1, 1], verts, nbytes, cap, [0, 2, 3, 4, 5],
              [1], "byte size")
    del keep


@pytest.mark.parametrize("bad", [0.0, -2.0, float("nan"), float("inf")])
def test_bad_capacities_are_rejected(eng, bad):
    csr = line_csr(2)
    nh = np.array([[1, 2, -1]], np.int32)
    cap = np.ones(csr.E)
    cap[edge_map(csr)[(1, 2)]] = bad
    with pytest.raises(ValueError):
        eng.fair_times(on(csr), dev_tree(eng, nh), EN.INT32, [0], [0], None, [1.0], cap,
                       to_root=True)
    epochs, out, keep = raw(eng, csr, nh, 1, [0, 2], [0, 1], [1.0, 2.0], cap)
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "capacity" in str(ei.value)
    eng.ctx.synchronize()
    assert 0 <= epochs <= 2
    del keep


def test_argument_errors(eng):
    import ctypes
    import torch
    csr = line_csr(2)
    eng.load(on(csr))
    L, h = eng.ctx._lib, eng.ctx._h
    buf = torch.zeros(64, dtype=torch.int64, device=eng.dev)
    p = ctypes.c_void_p(buf.data_ptr())
    n = ctypes.c_int32(9)
    dev = _native.DEVICE_PTRS

    def call(tree, layout, nrows, flags, nextra=0, max_epochs=2, nep=ctypes.byref(n)):
        return L.sdnr_fair_times(h, tree, layout, nrows, p, p, None, p, None, p, nextra, p, p, p,
                                 p, p, p, max_epochs, p, nep, flags)

    assert call(p, 0, 1, 0) == -22 and n.value == 0                       # host pointers
    assert call(p, 7, 1, dev) == -22
    assert call(p, _native.TREE_SLOT, 1, dev | _native.LOADS_TO_ROOT) == -22
    assert call(None, 0, 1, dev) == -22
    assert call(p, 0, -1, dev) == -22
    assert call(p, 0, 1, dev, -1) == -22
    assert call(p, 0, 1, dev, 0, -1) == -22
    assert call(p, 0, 1, dev, nep=None) == -22
    buf[0] = 5                                                            # pair_off[0] > pair_off[1]
    torch.cuda.synchronize()
    assert call(p, 0, 1, dev) == -22 and b"monotone" in L.sdnr_last_error()
    with _native.Context(0) as fresh:                                     # no graph uploaded
        assert L.sdnr_fair_times(fresh._h, p, 0, 1, p, p, None, p, None, p, 0, p, p, p, p, p, p,
                                 2, p, ctypes.byref(n), dev) == -77


# ------------------------------------------------- more rows than workgroups --

def test_more_rows_than_workgroups_three_epochs(eng):
    import torch
    from oracle import oracle as O
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    csr, comp = OG.graph()
    ids = np.arange(csr.V, dtype=np.int32)
    par, _, _ = O.dfs_tables(csr, ids)
    _, nh, _ = O.dest_tables(csr, ids)
    n = OG.units(cus)
    m = OG.row_mix(csr, comp, n, 920, OG.strides_for(cus, n))
    cap = np.random.default_rng(921).choice(np.asarray(CAPS, np.float64), int(csr.E))
    nbytes = np.random.default_rng(922).integers(0, 200, len(m.rows)).astype(np.float64)
    for tab, to_root in ((par, False), (nh, True)):
        tree = tab[m.dst]
        want = both(eng, csr, tree, EN.INT32, m.rows, m.ends, m.w, nbytes, cap, to_root=to_root,
                    max_epochs=3)
        grid = eng.ctx.last_grid()
        assert grid > 0 and len(m.kind) >= 2 * grid + 1
        OG.check_units(m.kind, m.key, grid)
        assert len(want[4]) == 3 and (want[1] >= 0).any() and (want[1] == -2).any()


# ---------------------------------------------------------------- drop-in --

def test_dropin_fat_tree_k4_all_table_kinds_and_host_ports():
    from sdnmpi_amd.util.topology_db import TopologyDB
    fabric = T.fat_tree(4)
    db = fabric.populate(TopologyDB())
    double = fake_db(fabric)
    csr = db.graph().csr
    rng = np.random.default_rng(31)
    links = [(int(csr.dpids[u]), int(csr.dpids[v])) for u, v in
             zip(np.repeat(np.arange(csr.V), np.diff(csr.row_ptr)).tolist(),
                 np.asarray(csr.col).tolist())]
    for lk in links:
        c, u = int(rng.integers(1, 4)), int(rng.integers(0, 4))
        for x in (db, double):
            x.set_link_cost(lk[0], lk[1], c)
            x.set_link_utilisation(lk[0], lk[1], u)
    capacity = {lk: int(c) for lk, c in zip(links, rng.choice(CAPS, len(links)))}
    pairs, w = dropin_pairs(fabric)
    nbytes = rng.integers(0, 1001, len(pairs)).astype(np.float64)
    for route in ("default", "shortest", "least_cost", "least_loaded"):
        for hc in (None, 2.5):
            a = db.fair_completion_times(pairs, nbytes, w, capacity, hc, route)
            b = double.fair_completion_times(pairs, nbytes, w, capacity, hc, route)
            for name in ("time", "rate0", "remaining", "epoch_time", "link_bytes.load"):
                x, y = a, b
                for part in name.split("."):
                    x, y = getattr(x, part), getattr(y, part)
                assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (route, hc, name)
            assert np.array_equal(a.epoch, b.epoch) and np.array_equal(a.routed, b.routed)
            assert np.array_equal(a.epoch_rounds, b.epoch_rounds) and a.epochs > 4
            assert a.link_bytes.as_dict() == b.link_bytes.as_dict()
            assert a.makespan() == b.makespan() and a.complete
        ap = db.all_pairs_fair_completion_times(64.0, capacity, route, max_epochs=5)
        bp = double.all_pairs_fair_completion_times(64.0, capacity, route, max_epochs=5)
        assert np.array_equal(ap.time, bp.time) and np.array_equal(ap.epoch, bp.epoch)
        assert np.array_equal(ap.remaining, bp.remaining) and ap.complete == bp.complete
    ranks = dict(enumerate(fabric.host_macs()[::2]))
    traffic = {(i, (i + 3) % len(ranks)): 1000 * (i + 1) for i in ranks}
    a = db.mpi_exchange_times(ranks, traffic, capacity, 2.5)
    b = double.mpi_exchange_times(ranks, traffic, capacity, 2.5)
    assert np.array_equal(a.time, b.time) and a.makespan() == b.makespan() > 0
    assert a.makespan() <= db.mpi_fair_rates(ranks, traffic, capacity, 2.5).step_time() * (1 + 1e-9)
