"""remote_lfa.hip (sdnr_remote_lfa) on the GPU against engine.remote_lfa_host:
the small fabrics, the named cases' written-out tables, rows wider than the
LDS tile and than one pass of links, the wavefront edge in X, more units than
workgroups, the argument errors, and the drop-in on the real engine.  Integer
tables: every comparison is array_equal."""
import ctypes

import numpy as np
import pytest

import golden_util as G
import over_grid as OG
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd.util.topology_db import TopologyDB
from test_cost_ecmp_loads import both_ways, digraph_csr, random_costs
from test_lfa_tables import all_pairs
from test_lfa_tables_gpu import ring_csr
from test_link_loads_gpu import on
from test_remote_lfa import (NAMED, NAMES, check_derived, edge_src, fake_db, named_case,
                             named_tables, remote_state, same)

pytestmark = pytest.mark.gpu

KERNEL = "remote_lfa_kernel"
FABRICS = ["mock", "random_V9", "random_V12", "random_V40", "random_V40_loops", "torus_2x2x2",
           "torus_5x3x2", "fat_tree_k4", "fat_tree_k8", "dragonfly_a4_h2_p2", "jellyfish_n60_r5"]


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def check(eng, csr, cost, P, verts=None, ex=None):
    """One engine call against the restatement."""
    ex = ex or on(csr)
    want = EN.remote_lfa_host(csr, cost, P, verts)
    got = eng.remote_lfa(ex, cost, P, verts)
    same(got, want)
    assert eng.ctx.last_kernel() == KERNEL and eng.ctx.last_launches() == 1
    return ex, want


def dev(eng, a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(eng.dev)


def dev_table(eng, P):
    return dev(eng, np.ascontiguousarray(P, np.uint32).view(np.int32), np.int32)


def raw(eng, d_P, verts, E, counts=True, fill=7, timing=False):
    """One sdnr_remote_lfa call into tensors prefilled with ``fill``; no
    synchronize.  ``verts`` None: the NULL list, 0 .. V - 1.  Returns the six
    tensors (counts None without) and what must stay alive."""
    import torch
    V = int(d_P.shape[0])
    n = V if verts is None else len(verts)
    d_v = None if verts is None else dev(eng, verts, np.int32)
    i32 = [torch.full((E,), fill, dtype=torch.int32, device=eng.dev) for _ in range(3)]
    tc = torch.full((E,), fill, dtype=torch.int64, device=eng.dev)
    k = torch.full((E,), fill, dtype=torch.uint8, device=eng.dev)
    c = torch.full((n, 4), fill, dtype=torch.int32, device=eng.dev) if counts else None
    torch.cuda.synchronize()
    eng.ctx.remote_lfa_device(d_P.data_ptr(), 0 if d_v is None else d_v.data_ptr(), n,
                              i32[0].data_ptr(), i32[1].data_ptr(), i32[2].data_ptr(),
                              tc.data_ptr(), k.data_ptr(), c.data_ptr() if counts else 0,
                              timing=timing)
    return i32 + [tc, k, c], (d_v, d_P)


def host6(t):
    out = [np.asarray(EN._host(a)) for a in t[:5]]
    out[3] = out[3].view(np.uint64)
    return out + [None if t[5] is None else EN._host(t[5]).view(np.uint32)]


# ------------------------------------------------------------ the small fabrics --

@pytest.mark.parametrize("hi", [1, 3])
@pytest.mark.parametrize("name", FABRICS)
def test_small_fabrics_against_the_restatement(eng, name, hi):
    csr = G.Golden(name).fabric().csr()
    V, E = int(csr.V), int(csr.E)
    cost = None if hi == 1 else random_costs(csr, 1, 3, 3 * V + hi)    # None: no costs uploaded
    P = all_pairs(csr, np.ones(E, np.uint32) if cost is None else cost)
    ex, full = check(eng, csr, cost, P)
    assert (full[4] & 1).any()
    rng = np.random.default_rng(V + hi)
    check(eng, csr, cost, P, np.arange(min(V, 7)), ex)
    check(eng, csr, cost, P, [V - 1], ex)
    perm = rng.permutation(V)
    check(eng, csr, cost, P, np.concatenate([perm, perm[:1], [-1, V]]), ex)
    # the raw call: a list with repeats and ids that are no vertex writes the
    # out-links of its vertices and nothing else; counts == NULL; verts == NULL
    d_P = dev_table(eng, P)                                 # (the graph and costs are in force)
    verts = [int(perm[0]), -1, int(perm[1]), int(perm[0]), V, V + 7]
    t, keep = raw(eng, d_P, verts, E)
    eng.ctx.synchronize()
    got = host6(t)
    mine = np.isin(edge_src(csr), verts[:3:2])
    for a, f, what in zip(got[:5], full[:5], NAMES):
        assert np.array_equal(a[mine], f[mine]), what
        assert (a[~mine] == 7).all(), what
    for i, v in enumerate(verts):
        assert np.array_equal(got[5][i], full[5][v] if 0 <= v < V else [0, 0, 0, 0])
    t, keep = raw(eng, d_P, None, E, counts=False)
    eng.ctx.synchronize()
    got = host6(t)
    assert got[5] is None
    same(got[:5] + [full[5]], full)


@pytest.mark.parametrize("name", NAMED)
def test_named_cases(eng, name):
    csr, cost, want = named_case(name)
    P = all_pairs(csr, cost)
    ex, host = check(eng, csr, cost, P)
    same(eng.remote_lfa(ex, cost, P), named_tables(csr, cost, want))


# ------------------------- rows past the tile and the pass, the wavefront edge in X --

def wheel_csr(rim):
    """Hub 0 and a rim ring 1 .. rim: the hub's row has ``rim`` links."""
    und = [(0, v) for v in range(1, rim + 1)] + [(v, v % rim + 1) for v in range(1, rim + 1)]
    return digraph_csr(both_ways(und))


@pytest.mark.parametrize("rim", [15, 16, 17, 62, 63, 64, 65, 130])
def test_wheels_hub_rows_at_the_tile_and_pass_edges_and_v_of_63_64_65(eng, rim):
    """The hub's row has ``rim`` links.  15, 16, 17: the 16-slot LDS tile not
    full, exactly full with no slot read from L2 (the tile is the widest row),
    and one slot past it.  62 .. 65: V = rim + 1 is 63, 64, 65 (one wavefront
    of X short of a lane, full, and one lane into the second) and 66, and the
    row is one pass of 64 links exactly full, then one link into a second
    pass.  130: three passes, 114 slots read from L2."""
    csr = wheel_csr(rim)
    V = rim + 1
    assert int(csr.V) == V and int(csr.row_ptr[1]) == rim
    cost = random_costs(csr, 1, 4, rim)
    P = all_pairs(csr, cost)
    ex, want = check(eng, csr, cost, P)
    check_derived(csr, cost, P, want)
    check(eng, csr, cost, P, [0, 5, 0], ex)
    ones = np.ones(int(csr.E), np.uint32)
    P = all_pairs(csr, ones)
    ex, want = check(eng, csr, ones, P, None, ex)
    check_derived(csr, ones, P, want)
    # unit costs: the hub's link to rim vertex d (edge d - 1) is repaired by d's
    # smaller rim neighbour, itself a neighbour of the hub: a per-link LFA
    for d in (1, 2, rim // 2, rim):
        nb = min((d - 2) % rim + 1, d % rim + 1)
        assert (want[0][d - 1], want[1][d - 1], want[3][d - 1], want[4][d - 1]) == (nb, nb, 1, 7)


# ------------------------------------------------------- more units than workgroups --

def test_more_units_than_workgroups(eng):
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    csr, comp = OG.graph()
    V = int(csr.V)
    n = OG.units(cus, 8)                                   # the grid is at most 8 per CU
    strides = OG.strides_for(cus, n)
    verts, kind = OG.dest_mix(csr, n, 1, 941, strides, p_bad=0.05)
    assert verts.shape[0] == n
    cost = random_costs(csr, 1, 5, 900)
    P = all_pairs(csr, cost)
    full = EN.remote_lfa_host(csr, cost, P)
    ok = (verts >= 0) & (verts < V)
    got = eng.remote_lfa(on(csr), cost, P, verts)
    assert eng.ctx.last_kernel() == KERNEL and eng.ctx.last_launches() == 1
    grid = eng.ctx.last_grid()
    assert 0 < grid < n and n >= 2 * grid + 1, (grid, n)
    OG.check_units(kind, verts, grid)
    mine = np.isin(edge_src(csr), verts[ok])
    for a, f, what in zip(got[:5], full[:5], NAMES):
        assert np.array_equal(a[mine], f[mine]), what
        assert (a[~mine] == (-1 if a.dtype == np.int32 else 0)).all(), what
    want_counts = np.where(ok[:, None], full[5][np.where(ok, verts, 0)], 0)
    assert np.array_equal(got[5], want_counts) and got[5].dtype == np.uint32
    assert (got[4][mine] & 1).any() and want_counts[:, 1].any()


# ------------------------------------------------------- argument and size errors --

def test_above_the_v_bound_is_refused_before_anything_is_read(eng):
    import torch
    V = EN.LFA_MAX_V + 1
    ex = on(ring_csr(V))
    eng.load(ex)
    small = torch.zeros(16, dtype=torch.int32, device=eng.dev)
    out8 = torch.zeros(16, dtype=torch.uint8, device=eng.dev)
    torch.cuda.synchronize()
    before = eng.ctx.last_kernel()
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.remote_lfa_device(small.data_ptr(), small.data_ptr(), 1, small.data_ptr(),
                                  small.data_ptr(), small.data_ptr(), small.data_ptr(),
                                  out8.data_ptr())
    assert ei.value.code == -22 and "16384" in str(ei.value)
    assert eng.ctx.last_kernel() == before
    eng.ctx.synchronize()
    with pytest.raises(ValueError):
        TopologyDB(engine=eng)._remote_lfa_rows(ex)


def test_argument_errors_timing_and_the_kernel_name(eng):
    import torch
    csr = G.Golden("random_V12").fabric().csr()
    V, E = int(csr.V), int(csr.E)
    cost = random_costs(csr, 1, 4, 11)
    P = all_pairs(csr, cost)
    ex = on(csr)
    eng.set_link_costs(ex, cost)
    d_P = dev_table(eng, P)
    d_v = dev(eng, np.arange(V), np.int32)
    i32 = [torch.full((E,), 7, dtype=torch.int32, device=eng.dev) for _ in range(3)]
    tc = torch.full((E,), 7, dtype=torch.int64, device=eng.dev)
    k = torch.full((E,), 7, dtype=torch.uint8, device=eng.dev)
    L, h = eng.ctx._lib, eng.ctx._h
    p = lambda t: ctypes.c_void_p(t.data_ptr())           # noqa: E731
    flag = _native.DEVICE_PTRS
    fn = L.sdnr_remote_lfa
    args = [p(d_P), p(d_v), V, p(i32[0]), p(i32[1]), p(i32[2]), p(tc), p(k), None]

    def with_(i, v):
        a = list(args)
        a[i] = v
        return a
    torch.cuda.synchronize()
    assert fn(None, *args, flag) == -22
    assert fn(h, *args, 0) == -22 and b"device pointers only" in L.sdnr_last_error()
    for i in (0, 3, 4, 5, 6, 7):                                          # required buffers
        assert fn(h, *with_(i, None), flag) == -22
    assert fn(h, *with_(2, -1), flag) == -22
    assert fn(h, *with_(2, 0), flag) == 0                                 # nverts == 0: nothing touched
    with _native.Context(0) as fresh:                                     # no graph uploaded
        assert fn(fresh._h, *args, flag) == -77
    eng.ctx.synchronize()
    assert all((t == 7).all() for t in i32 + [tc, k])
    # the timed call: the main kernel's name, its time and its grid
    t, keep = raw(eng, d_P, list(range(V)), E, timing=True)
    eng.ctx.synchronize()
    assert eng.ctx.last_kernel() == KERNEL and eng.ctx.last_launches() == 1
    assert eng.ctx.last_kernel_ms() > 0 and eng.ctx.last_grid() == V
    same(host6(t), EN.remote_lfa_host(csr, cost, P))


# ------------------------------------------------------------------ the drop-in --

def test_dropin_on_the_engine_fat_tree_k8_is_fully_covered(eng):
    fabric = G.Golden("fat_tree_k8").fabric()
    db = fabric.populate(TopologyDB(engine=eng))
    cov = db.remote_lfa_coverage()
    assert (cov["primaries"], cov["remote_backups"]) == (6320, 2816)
    assert cov["backups"] + cov["remote_backups"] == cov["primaries"]
    assert cov["coverage_with_remote"] == 1.0
    assert (cov["links"], cov["links_repaired"], cov["links_plain"]) == (512, 512, 0)
    assert db.unrepaired_links() == {} and len(db.unprotected_links()) > 0
    assert remote_state(db) == remote_state(fake_db(fabric))


def test_dropin_on_the_engine_equals_the_engine_double_under_costs(eng):
    fabric = G.Golden("random_V12").fabric()
    db = fabric.populate(TopologyDB(engine=eng))
    twin = fake_db(fabric)
    links = sorted((a, b) for a in db.links for b in db.links[a])
    costs = {links[i]: 1 + i % 3 for i in range(0, len(links), 2)}
    db.set_link_costs(costs)
    twin.set_link_costs(costs)
    assert remote_state(db) == remote_state(twin)
    assert db.unrepaired_links()
