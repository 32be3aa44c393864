"""multicast.hip (sdnr_multicast_trees) on the GPU against
engine.multicast_trees_host, and the drop-in's multicast calls against the same
calls over the CPU engine double.  All values are integers: every comparison
is exact."""
import ctypes
import types

import numpy as np
import pytest

import boundary_graphs as B
import golden_util as G
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from test_multicast_trees import (fabric_cost, fake_db, full_weights, random_groups, same,
                                  walk_groups)

pytestmark = pytest.mark.gpu

LAYOUTS = (EN.INT32, EN.PORT16, EN.SLOT)
LDS, GLOBAL = "multicast_trees_kernel<lds>", "multicast_trees_kernel<global>"


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


LAY = {EN.PORT16: _native.TREE_PORT16, EN.SLOT: _native.TREE_SLOT, EN.INT32: _native.TREE_INT32}


class Raw(object):
    """Device copies of one batch and the output tensors of raw
    sdnr_multicast_trees calls on them (no synchronize inside)."""

    def __init__(self, eng, csr, tree, layout, root, off, row, vert, w=None, to_root=False):
        import torch
        t = torch
        self.eng, self.E, self.lay, self.to_root = eng, int(csr.E), LAY[layout], to_root
        self.tree = dev_tree(eng, tree)
        self.ng, self.nmem = len(root), len(row)
        i32 = lambda a: t.from_numpy(np.asarray(a, np.int32).reshape(-1)).to(eng.dev)  # noqa: E731
        self.root, self.row, self.vert = i32(root), i32(row), i32(vert)
        self.off = t.from_numpy(np.asarray(off, np.int64)).to(eng.dev)
        self.w = t.from_numpy(np.asarray(w, np.uint64).view(np.int64)).to(eng.dev) \
            if w is not None else None
        self.reached = t.full((max(1, self.nmem),), 9, dtype=t.uint8, device=eng.dev)
        self.cnt = t.full((max(1, self.ng),), -5, dtype=t.int64, device=eng.dev)
        self.load = t.zeros(max(1, self.E), dtype=t.int64, device=eng.dev)
        t.cuda.synchronize()

    def call(self, reached=True, cnt=True, ent_off=None, ent_edge=None, load=True):
        p = lambda x: x.data_ptr() if x is not None else 0           # noqa: E731
        self.eng.ctx.multicast_trees_device(
            p(self.tree), self.lay, int(self.tree.shape[0]), self.ng, p(self.root), p(self.off),
            p(self.row), p(self.vert), p(self.w), p(self.reached) if reached else 0,
            p(self.cnt) if cnt else 0, p(ent_off), p(ent_edge), p(self.load) if load else 0,
            to_root=self.to_root)

    def fill(self, ent_off, total, load=False):
        import torch
        eo = torch.from_numpy(np.asarray(ent_off, np.int64)).to(self.eng.dev)
        edge = torch.full((max(1, int(total)) + 8,), -7, dtype=torch.int32, device=self.eng.dev)
        torch.cuda.synchronize()
        self.call(reached=False, cnt=False, ent_off=eo, ent_edge=edge, load=load)
        self.keep = eo
        return edge

    def loads(self):
        return self.load.cpu().numpy().view(np.uint64)[:self.E]


# ------------------------------------------------------ the small fabrics --

@pytest.fixture(scope="module")
def small_cases():
    """Per G.SMALL fabric: oracle tables of every vertex, one batch of groups
    per row form, and the restatement's outputs, computed once."""
    from oracle import oracle as O
    out = {}
    for k, name in enumerate(G.SMALL):
        csr = G.Golden(name).fabric().csr()
        V = csr.V
        ids = np.arange(V, dtype=np.int32)
        par, prt, _ = O.dfs_tables(csr, ids)
        _, nh, _ = O.dest_tables(csr, ids)
        _, cnh, _ = EN.cost_tables_host(csr, fabric_cost(csr, V), ids)
        rng = np.random.default_rng(70 + k)
        up = random_groups(V, rng, False)
        down = random_groups(V, rng, True)
        w = full_weights(up[0].shape[0], rng)
        want = {"up": EN.multicast_trees_host(csr, par, EN.INT32, *up, weights=w),
                "nh": EN.multicast_trees_host(csr, nh, EN.INT32, *down, weights=w, to_root=True),
                "cnh": EN.multicast_trees_host(csr, cnh, EN.INT32, *down, weights=w, to_root=True)}
        out[name] = dict(csr=csr, par=par, prt=prt, nh=nh, cnh=cnh, up=up, down=down, w=w,
                         want=want)
    return out


def check_engine(eng, csr, tree, layout, batch, w, want, to_root=False):
    ex = on(csr)
    d = tree if not isinstance(tree, np.ndarray) else dev_tree(eng, tree)
    got = eng.multicast_trees(ex, d, layout, *batch, weights=w, to_root=to_root)
    assert same(got, want), layout
    r, eo, ee, ld = eng.multicast_trees(ex, d, layout, *batch, weights=w, to_root=to_root,
                                        entries=False, loads=False)            # count only
    assert np.array_equal(r, want[0]) and np.array_equal(eo, want[1]) and ee is None and ld is None
    r, eo, ee, ld = eng.multicast_trees(ex, d, layout, *batch, weights=w, to_root=to_root,
                                        entries=False)                         # loads only
    assert ee is None and np.array_equal(ld, want[3]) and ld.dtype == np.uint64
    r, eo, ee, ld = eng.multicast_trees(ex, d, layout, *batch, weights=None, to_root=to_root,
                                        loads=False)                           # entries only
    assert ld is None and np.array_equal(ee, want[2]) and ee.dtype == np.int32


@pytest.mark.parametrize("name", G.SMALL)
def test_small_fabrics_tree_rows_all_layouts(eng, small_cases, name):
    c = small_cases[name]
    for lay in LAYOUTS:
        tree = c["par"] if lay == EN.INT32 else EN.pack_host_tree(c["par"], c["prt"], c["csr"], lay)
        check_engine(eng, c["csr"], tree, lay, c["up"], c["w"], c["want"]["up"])
        assert eng.ctx.last_kernel() == LDS and eng.ctx.last_launches() == 1


@pytest.mark.parametrize("name", G.SMALL)
def test_small_fabrics_next_hop_rows(eng, small_cases, name):
    c = small_cases[name]
    for key in ("nh", "cnh"):
        check_engine(eng, c["csr"], c[key], EN.INT32, c["down"], c["w"], c["want"][key], True)
        assert eng.ctx.last_kernel() == LDS


@pytest.mark.parametrize("form", ["up", "nh"])
def test_loads_add_and_calls_repeat_bit_for_bit(eng, small_cases, form):
    c = small_cases["fat_tree_k8"]
    csr = c["csr"]
    eng.load(on(csr))
    tab, batch, to_root = (c["par"], c["up"], False) if form == "up" else (c["nh"], c["down"], True)
    reached, eo, ee, load = c["want"][form]
    a = Raw(eng, csr, tab, EN.INT32, *batch, w=c["w"], to_root=to_root)
    b = Raw(eng, csr, tab, EN.INT32, *batch, w=c["w"], to_root=to_root)
    a.call()
    a.call()                                               # the loads are added a second time
    b.call()
    edge_a = a.fill(eo, eo[-1])
    edge_b = b.fill(eo, eo[-1], load=True)                 # ... here by the fill call
    eng.ctx.synchronize()
    assert np.array_equal(a.loads(), load * np.uint64(2)) and np.array_equal(b.loads(), a.loads())
    for x, edge in ((a, edge_a), (b, edge_b)):
        assert np.array_equal(x.reached.cpu().numpy()[:x.nmem], reached)
        assert np.array_equal(x.cnt.cpu().numpy(), np.diff(eo))
        e = edge.cpu().numpy()
        assert np.array_equal(e[:eo[-1]], ee) and (e[eo[-1]:] == -7).all()
    assert edge_a.cpu().numpy().tobytes() == edge_b.cpu().numpy().tobytes()
    assert a.cnt.cpu().numpy().tobytes() == b.cnt.cpu().numpy().tobytes()


# ------------------------------------------------------------ edge shapes --

@pytest.fixture(scope="module")
def torus8():
    """The 8 x 8 x 8 torus (V = 512): tree rows of 301 roots, next-hop rows of
    every vertex."""
    from oracle import oracle as O
    csr = T.torus3d(8, 8, 8).csr()
    rng = np.random.default_rng(88)
    roots = np.sort(rng.choice(csr.V, 301, replace=False)).astype(np.int32)
    par, prt, _ = O.dfs_tables(csr, roots)
    _, nh, _ = O.dest_tables(csr, np.arange(csr.V, dtype=np.int32))
    return csr, roots, par, prt, nh


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_member_counts_at_the_wave_and_workgroup_bounds(eng, torus8, n):
    csr, roots, par, prt, nh = torus8
    rng = np.random.default_rng(n)
    vert = rng.permutation(csr.V)[:n]
    w = np.array([U64_ODD], np.uint64)
    for lay in LAYOUTS:
        tree = par if lay == EN.INT32 else EN.pack_host_tree(par, prt, csr, lay)
        batch = ([int(roots[5])], [0, n], np.full(n, 5), vert)
        want = EN.multicast_trees_host(csr, tree, lay, *batch, weights=w)
        assert want[0].all() and want[1][-1] >= min(n, 2) - 1
        assert same(eng.multicast_trees(on(csr), dev_tree(eng, tree), lay, *batch, weights=w), want)
    batch = ([int(roots[5])], [0, n], vert, vert)
    want = EN.multicast_trees_host(csr, nh, EN.INT32, *batch, weights=w, to_root=True)
    assert same(eng.multicast_trees(on(csr), dev_tree(eng, nh), EN.INT32, *batch, weights=w,
                                    to_root=True), want)


U64_ODD = (1 << 64) - 3


def test_one_group_beside_300_groups(eng, torus8):
    csr, roots, par, _, _ = torus8
    rng = np.random.default_rng(300)
    sizes = rng.integers(0, 40, 301)
    sizes[0] = 33
    off = np.concatenate([[0], np.cumsum(sizes)])
    row = np.repeat(np.arange(301), sizes)
    vert = rng.integers(0, csr.V, int(off[-1]))
    w = full_weights(301, rng)
    d = dev_tree(eng, par)
    want = EN.multicast_trees_host(csr, par, EN.INT32, roots, off, row, vert, w)
    got = eng.multicast_trees(on(csr), d, EN.INT32, roots, off, row, vert, w)
    assert same(got, want) and (np.diff(want[1])[sizes > 1] > 0).all()
    alone = eng.multicast_trees(on(csr), d, EN.INT32, roots[:1], off[:2], row[:33], vert[:33],
                                w[:1])
    assert np.array_equal(alone[2], got[2][:got[1][1]]) and alone[1][1] == got[1][1]
    assert np.array_equal(alone[0], got[0][:33])


def test_no_groups_no_members_and_the_root_itself(eng, small_cases):
    c = small_cases["fat_tree_k4"]
    csr, par = c["csr"], c["par"]
    ex = on(csr)
    d = dev_tree(eng, par)
    r, eo, ee, ld = eng.multicast_trees(ex, d, EN.INT32, [], [0], [], [])
    assert r.size == 0 and eo.tolist() == [0] and ee.size == 0 and not ld.any()
    # ngroups == 0 and an empty member list: SDNR_OK, nothing touched (null pointers are fine)
    eng.load(ex)
    eng.ctx.multicast_trees_device(0, _native.TREE_INT32, 0, 0, 0, 0, 0, 0)
    x = Raw(eng, csr, par, EN.INT32, [3, 4], [2, 2, 2], [], [])
    x.call()
    eng.ctx.synchronize()
    assert (x.cnt.cpu().numpy() == -5).all() and not x.loads().any()
    # a group without members between two with; a member that is its group's root
    batch = ([3, 4, 5], [0, 2, 2, 4], [3, 3, 5, 5], [3, 7, 5, 5])
    want = EN.multicast_trees_host(csr, par, EN.INT32, *batch)
    assert want[0].tolist() == [1, 1, 1, 1] and np.diff(want[1]).tolist()[1:] == [0, 0]
    assert same(eng.multicast_trees(ex, d, EN.INT32, *batch), want)
    nh = c["nh"]
    batch = ([3, 4, 5], [0, 2, 2, 4], [3, 7, 5, 5], [3, 7, 5, 5])
    want = EN.multicast_trees_host(csr, nh, EN.INT32, *batch, to_root=True)
    assert same(eng.multicast_trees(ex, dev_tree(eng, nh), EN.INT32, *batch, to_root=True), want)


def test_unreached_members_in_a_two_component_graph(eng):
    from oracle import oracle as O
    from test_link_loads import random_csr
    csr = random_csr(40, 30, 3)                            # the last fifth is unreachable
    ids = np.arange(csr.V, dtype=np.int32)
    par, prt, _ = O.dfs_tables(csr, ids)
    _, nh, _ = O.dest_tables(csr, ids)
    assert (par[0] < 0).any()
    vert = np.array([7, 39, 38, 11, 39, 3, 0, 39])
    batch = ([0, 39], [0, 5, 8], [0, 0, 0, 0, 0, 39, 39, 39], vert)
    want = walk_groups(csr, par, csr.V, *batch, [1, 1], False)
    assert want[0].tolist() == [1, 0, 0, 1, 0, 0, 0, 1]
    for lay in LAYOUTS:
        tree = par if lay == EN.INT32 else EN.pack_host_tree(par, prt, csr, lay)
        assert same(eng.multicast_trees(on(csr), dev_tree(eng, tree), lay, *batch), want)
    batch = ([0, 39], [0, 5, 8], vert, vert)
    want = walk_groups(csr, nh, csr.V, *batch, [1, 1], True)
    assert want[0].tolist() == [1, 0, 0, 1, 0, 0, 0, 1]
    assert same(eng.multicast_trees(on(csr), dev_tree(eng, nh), EN.INT32, *batch, to_root=True),
                want)


@pytest.mark.parametrize("name", G.LOOPS)
def test_self_loop_links_at_the_root_and_at_a_member(eng, small_cases, name):
    c = small_cases[name]
    csr = c["csr"]
    src = np.repeat(np.arange(csr.V), np.diff(csr.row_ptr))
    loops = src[src == np.asarray(csr.col)]
    plain = np.setdiff1d(np.arange(csr.V), loops)
    assert loops.size > 1 and plain.size
    a, b, p = int(loops[0]), int(loops[-1]), int(plain[0])
    roots = [a, p, a]                                      # loop at the root, at a member, at both
    vert = [p, b, p, a, b, b, a]
    off = [0, 2, 5, 7]
    for lay in LAYOUTS:
        tree = c["par"] if lay == EN.INT32 else EN.pack_host_tree(c["par"], c["prt"], csr, lay)
        batch = (roots, off, np.repeat(roots, np.diff(off)), vert)
        want = EN.multicast_trees_host(csr, tree, lay, *batch)
        assert want[2].size and not np.isin(want[2], np.nonzero(src == csr.col)[0]).any()
        assert same(eng.multicast_trees(on(csr), dev_tree(eng, tree), lay, *batch), want)
    batch = (roots, off, vert, vert)
    want = EN.multicast_trees_host(csr, c["nh"], EN.INT32, *batch, to_root=True)
    assert same(eng.multicast_trees(on(csr), dev_tree(eng, c["nh"]), EN.INT32, *batch,
                                    to_root=True), want)


# --------------------------------------------------------- map placement --

def ring_with_chords(extra):
    """32,768 switches on a ring plus 81,920 chords (+ ``extra``): with extra
    = 0 the V-bit and E-bit maps take exactly the 8,192 words LDS holds."""
    V = 32768
    u = np.arange(V, dtype=np.int64)
    half = np.arange(V // 2 + extra, dtype=np.int64)
    a = np.concatenate([u, u, u, half])
    b = np.concatenate([u + 1, u + 5, u + 11, half + 17]) % V
    src, dst = np.concatenate([a, b]) + 1, np.concatenate([b, a]) + 1
    port = np.concatenate([np.repeat([1, 2, 3, 4], [V, V, V, half.size]),
                           np.repeat([5, 6, 7, 8], [V, V, V, half.size])])
    return T.build_csr(src, dst, port, extra_vertices=range(1, V + 1))


@pytest.mark.parametrize("extra,kernel", [(0, LDS), (1, GLOBAL)])
def test_maps_in_lds_and_in_scratch(eng, extra, kernel):
    from oracle import oracle as O
    csr = ring_with_chords(extra)
    words = (csr.V + 31) // 32 + (csr.E + 31) // 32
    assert words == 8192 + extra and EN.multicast_maps_in_lds(csr.V, csr.E) == (extra == 0)
    rng = np.random.default_rng(extra)
    root = 12345
    par, prt, _ = O.dfs_tables(csr, np.array([root], np.int32))
    vert = np.concatenate([rng.integers(0, csr.V, 200), [root, 0, csr.V - 1]])
    w = np.array([U64_ODD], np.uint64)
    for lay in (EN.INT32, EN.SLOT):
        tree = par if lay == EN.INT32 else EN.pack_host_tree(par, prt, csr, lay)
        batch = ([root], [0, vert.size], np.zeros(vert.size, np.int64), vert)
        want = EN.multicast_trees_host(csr, tree, lay, *batch, weights=w)
        assert want[1][-1] > 200
        assert same(eng.multicast_trees(on(csr), dev_tree(eng, tree), lay, *batch, weights=w), want)
        assert eng.ctx.last_kernel() == kernel
    m = csr.V - 1
    _, nh, _ = O.dest_tables(csr, np.array([m], np.int32))
    batch = ([root], [0, 1], [0], [m])
    want = EN.multicast_trees_host(csr, nh, EN.INT32, *batch, weights=w, to_root=True)
    assert want[1][-1] > 1
    assert same(eng.multicast_trees(on(csr), dev_tree(eng, nh), EN.INT32, *batch, weights=w,
                                    to_root=True), want)
    assert eng.ctx.last_kernel() == kernel


# ------------------------------------------------------------- id widths --

@pytest.mark.parametrize("V", [65535, 65536, 65537])
def test_vertex_ids_at_the_16_bit_boundary(eng, V):
    from oracle import oracle as O
    csr = B.ring(V)
    ids = np.array(B.probe_ids(V), np.int32)
    pick = [0, len(ids) - 1, len(ids) - 2]                 # rows of 0, V - 1, V - 2
    par, prt, _ = O.dfs_tables(csr, ids[pick])
    rng = np.random.default_rng(V)
    sizes = [ids.size, 30, 1]
    off = np.concatenate([[0], np.cumsum(sizes)])
    vert = np.concatenate([ids, rng.integers(0, V, 30), [V - 1]])
    row = np.repeat(np.arange(3), sizes)
    w = full_weights(3, rng)
    ex = on(csr)
    batch = (ids[pick], off, row, vert)
    want = EN.multicast_trees_host(csr, par, EN.INT32, *batch, weights=w)
    assert want[0].any() and not want[0].all() and want[2].max() > 0xFFFF
    for lay in (EN.INT32, EN.SLOT) + ((EN.PORT16,) if V <= 65535 else ()):
        tree = par if lay == EN.INT32 else EN.pack_host_tree(par, prt, csr, lay)
        assert same(eng.multicast_trees(ex, dev_tree(eng, tree), lay, *batch, weights=w), want), lay
        assert eng.ctx.last_kernel() == GLOBAL
    if V > 65535:
        tree = dev_tree(eng, EN.pack_host_tree(par, prt, csr, EN.SLOT))
        with pytest.raises(_native.SdnrError) as ei:
            eng.multicast_trees(ex, tree, EN.PORT16, *batch, weights=w)
        assert ei.value.code == -22 and "65535" in str(ei.value)
    _, nh, _ = O.dest_tables(csr, ids)
    mem = np.arange(ids.size)
    batch = ([int(ids[3]), V - 2], [0, ids.size, 2 * ids.size], np.tile(mem, 2), np.tile(ids, 2))
    want = EN.multicast_trees_host(csr, nh, EN.INT32, *batch, weights=w[:2], to_root=True)
    assert want[0].any() and want[1][-1] > 0
    assert same(eng.multicast_trees(ex, dev_tree(eng, nh), EN.INT32, *batch, weights=w[:2],
                                    to_root=True), want)


# ----------------------------------------------------------------- errors --

def test_argument_errors(eng, small_cases):
    import torch
    c = small_cases["mock"]
    csr, par = c["csr"], c["par"]
    eng.load(on(csr))
    V = csr.V
    x = Raw(eng, csr, par, EN.INT32, [0, 1], [0, 2, 3], [0, 0, 1], [1, 2, 0])
    L, h = eng.ctx._lib, eng.ctx._h
    p = lambda t: ctypes.c_void_p(t.data_ptr())           # noqa: E731
    dev = _native.DEVICE_PTRS
    eo = torch.zeros(3, dtype=torch.int64, device=eng.dev)
    edge = torch.zeros(64, dtype=torch.int32, device=eng.dev)
    torch.cuda.synchronize()

    def call(tree=p(x.tree), lay=0, nrows=V, ng=2, root=p(x.root), off=p(x.off), row=p(x.row),
             vert=p(x.vert), ent_off=None, ent_edge=None, flags=dev, ctx=h):
        return L.sdnr_multicast_trees(ctx, tree, lay, nrows, ng, root, off, row, vert, None,
                                      p(x.reached), p(x.cnt), ent_off, ent_edge, p(x.load), flags)

    def refused(code=-22, **kw):
        assert call(**kw) == code
        assert b"sdnr_multicast_trees" in L.sdnr_last_error()

    refused(flags=0)                                                      # host pointers
    refused(lay=7)
    refused(lay=_native.TREE_PORT16, flags=dev | _native.MCAST_TO_ROOT)
    refused(lay=_native.TREE_SLOT, flags=dev | _native.MCAST_TO_ROOT)
    refused(tree=None)
    refused(root=None)
    refused(off=None)
    refused(row=None)
    refused(vert=None)
    refused(ent_off=p(eo))                                                # without ent_edge
    refused(ent_edge=p(edge))
    refused(nrows=-1)
    refused(ng=-1)
    x.off[0] = 5                                                          # mem_off[0] > mem_off[n]
    torch.cuda.synchronize()
    refused()
    assert b"monotone" in L.sdnr_last_error()
    x.off[0] = 0
    eo[0] = 9
    torch.cuda.synchronize()
    refused(ent_off=p(eo), ent_edge=p(edge))
    assert b"monotone" in L.sdnr_last_error()
    with _native.Context(0) as fresh:                                     # no graph uploaded
        refused(code=-77, ctx=fresh._h)
    eng.ctx.synchronize()
    assert not x.loads().any() and (x.cnt.cpu().numpy() == -5).all()
    assert call() == 0
    eng.ctx.synchronize()
    assert x.cnt.cpu().numpy().tolist() == np.diff(
        EN.multicast_trees_host(csr, par, EN.INT32, [0, 1], [0, 2, 3], [0, 0, 1], [1, 2, 0])[1]
    ).tolist()


def bad_tree_rows(csr, par):
    """Tree row 1 of the first four, hand-edited two ways -- a parent cycle
    below the root, a parent that is no neighbour -- and a member inside each."""
    V = csr.V
    r = 1
    kids = [v for v in range(V) if v != r and par[r, v] == r]
    a = next(v for v in kids if (par[r] == v).any())                     # a child with children
    x = int(np.nonzero(par[r] == a)[0][0])
    cyc = par[:4].copy()
    cyc[r, a] = x                                                         # a <-> x
    has = set(zip(np.repeat(np.arange(V), np.diff(csr.row_ptr)).tolist(), csr.col.tolist()))
    far = next(v for v in range(V) if v not in (a, r, x) and (v, a) not in has and par[r, v] >= 0)
    nol = par[:4].copy()
    nol[r, a] = far                                                       # far -> a is no link
    return (cyc, x), (nol, a)


def bad_next_hop_rows(csr, nh):
    """Next-hop row 1 of the first four, hand-edited the same two ways, and a
    root whose walk toward 1 meets each edit."""
    V = csr.V
    s = next(v for v in range(V) if nh[1, v] >= 0 and nh[1, v] != 1)      # two hops or more from 1
    n = int(nh[1, s])
    cyc = nh[:4].copy()
    cyc[1, n] = s                                                         # s -> n -> s
    has = set(zip(np.repeat(np.arange(V), np.diff(csr.row_ptr)).tolist(), csr.col.tolist()))
    far = next(v for v in range(V) if v not in (s, 1) and (s, v) not in has)
    nol = nh[:4].copy()
    nol[1, s] = far                                                       # s -> far is no link
    return (cyc, s), (nol, s)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("to_root", [False, True])
@pytest.mark.parametrize("name", ["fat_tree_k4", "torus_4x4x4"])
def test_rows_that_are_no_trees_are_reported_not_followed(eng, small_cases, name, to_root, which):
    """The walk bound doing its job: the call returns, sdnr_synchronize
    reports SDNR_ERR_INVAL once, the bad group adds nothing and the other
    groups' outputs are the restatement's."""
    c = small_cases[name]
    csr, par = c["csr"], c["par"]
    V = csr.V
    rng = np.random.default_rng(which)
    eng.load(on(csr))
    if to_root:
        good = c["nh"][:4]
        bad, s = bad_next_hop_rows(csr, c["nh"])[which]
        roots = [V - 1, s, V - 2, V - 3]
        off = [0, 2, 3, 5, 7]
        vert = np.array([0, 2, 1, 0, 3, 2, 3])             # only group 1 walks row 1
        row = vert.copy()
    else:
        good = par[:4]
        bad, m = bad_tree_rows(csr, par)[which]
        roots = [0, 1, 2, 3]
        sizes = [6, 5, 6, 6]
        off = np.concatenate([[0], np.cumsum(sizes)])
        row = np.repeat(np.arange(4), sizes)
        vert = rng.integers(0, V, int(off[-1]))
        vert[6] = m
    w = np.array([3, 5, 7, 11], np.uint64)
    want = EN.multicast_trees_host(csr, good, EN.INT32, roots, off, row, vert, w, to_root)
    with pytest.raises(ValueError):
        EN.multicast_trees_host(csr, bad, EN.INT32, roots, off, row, vert, w, to_root)
    x = Raw(eng, csr, bad, EN.INT32, roots, off, row, vert, w, to_root)
    x.call()
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "sdnr_multicast_trees" in str(ei.value)
    eng.ctx.synchronize()                                  # reported once
    cnt = x.cnt.cpu().numpy()
    ok = np.array([0, 2, 3])
    assert np.array_equal(cnt[ok], np.diff(want[1])[ok]) and cnt[1] == 0 and cnt.sum() > 0
    # the fill of the groups that stand, the bad group's slice empty
    eo = np.concatenate([[0], np.cumsum(cnt)])
    edge = x.fill(eo, eo[-1])
    with pytest.raises(_native.SdnrError):
        eng.ctx.synchronize()
    e = edge.cpu().numpy()
    keep = np.repeat(np.arange(4), np.diff(want[1])) != 1
    assert np.array_equal(e[:eo[-1]], want[2][keep]) and (e[eo[-1]:] == -7).all()
    good_load = EN.multicast_trees_host(csr, good, EN.INT32, roots, off, row, vert,
                                        w * np.array([1, 0, 1, 1], np.uint64), to_root)[3]
    assert np.array_equal(x.loads(), good_load)
    keep_m = np.repeat(np.arange(4), np.diff(off)) != 1
    assert np.array_equal(x.reached.cpu().numpy()[:len(vert)][keep_m], want[0][keep_m])
    # the context goes on working
    got = eng.multicast_trees(on(csr), dev_tree(eng, par), EN.INT32, *c["up"], weights=c["w"])
    assert same(got, c["want"]["up"])


def test_fill_with_offsets_that_are_not_the_prefix_writes_nothing_outside(eng, small_cases):
    c = small_cases["fat_tree_k8"]
    csr = c["csr"]
    eng.load(on(csr))
    reached, eo, ee, _ = c["want"]["up"]
    g = int(np.nonzero(np.diff(eo) > 2)[0][0])
    wrong = eo.copy()
    wrong[g + 1:] -= 1                                     # group g's slice one short
    x = Raw(eng, csr, c["par"], EN.INT32, *c["up"])
    edge = x.fill(wrong, wrong[-1])
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "ent_off" in str(ei.value)
    e = edge.cpu().numpy()
    assert (e[wrong[g]:wrong[g + 1]] == -7).all() and (e[wrong[-1]:] == -7).all()
    assert np.array_equal(e[:wrong[g]], ee[:eo[g]])
    assert np.array_equal(e[wrong[g + 1]:wrong[-1]], ee[eo[g + 1]:])


# ---------------------------------------------------------------- drop-in --

@pytest.mark.parametrize("name", ["fat_tree_k8", "dragonfly_a4_h2_p2"])
def test_dropin_equals_the_cpu_double(name):
    from sdnmpi_amd.util.topology_db import TopologyDB
    fabric = G.Golden(name).fabric()
    db = fabric.populate(TopologyDB())
    cpu = fake_db(fabric)
    macs = fabric.host_macs()
    for d in (db, cpu):
        rng = np.random.default_rng(12)
        d.set_link_costs({(a, b): int(rng.integers(1, 9)) for a in sorted(d.links)
                          for b in sorted(d.links[a])})
    groups = [(a, [macs[j] for j in rng.permutation(len(macs))[:9].tolist()] +
               ["02:00:00:00:00:77"]) for a in macs[::4]]
    r2m = {r: macs[(7 * r) % len(macs)] for r in range(12)}
    r2m[12] = r2m[0]
    traffic = {0: 10, 5: 1 << 40, 12: 3}
    for route in ("default", "shortest", "least_cost"):
        got, want = db.multicast_trees(groups, route), cpu.multicast_trees(groups, route)
        assert all(np.array_equal(x, y) for x, y in zip(got, want)) and want[0][-1] > 0
        for tr in (None, traffic):
            a, b = db.mpi_bcast_link_loads(r2m, tr, route), cpu.mpi_bcast_link_loads(r2m, tr, route)
            assert np.array_equal(a.load, b.load) and a.load.any() and a.as_dict() == b.as_dict()
        ga, gb = db.mpi_bcast_entries(r2m, [0, 5], route), cpu.mpi_bcast_entries(r2m, [0, 5], route)
        assert all(np.array_equal(x, y) for x, y in zip(ga, gb))
    assert db.multicast_tree(macs[0], macs[1:6]).entries == \
        cpu.multicast_tree(macs[0], macs[1:6]).entries
