"""lfa_tables.hip (sdnr_lfa_tables) on the GPU against engine.lfa_tables_host,
the named cases' written-out tables, an analytic ring at the V bound, and the
drop-in on the real engine against the engine double.  Integer tables: every
comparison is array_equal."""
import ctypes

import numpy as np
import pytest

import golden_util as G
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from sdnmpi_amd.util.topology_db import TopologyDB
from test_cost_ecmp_loads import both_ways, digraph_csr, random_costs
from test_cost_ecmp_loads_gpu import core_tier_costs
from test_ecmp_link_loads import edge_map
from test_lfa_tables import (NAMED, all_pairs, dropin_state, fake_db, mutate, named_case,
                             ports_of)
from test_link_loads import golden_pairs
from test_link_loads_gpu import on

pytestmark = pytest.mark.gpu

INF = EN.COST_INF
NODE, LINK = "lfa_tables_kernel<node>", "lfa_tables_kernel<link>"


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def host4(t):
    return tuple(np.asarray(EN._host(a)) for a in t)


def same(got, want):
    got = host4(got)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert got[2].dtype == np.uint8 and got[3].dtype == np.uint32
    for a, b, what in zip(got, want, ("backup", "backup_port", "kind", "counts")):
        assert a.shape == b.shape and np.array_equal(a, b), what


def check(eng, csr, cost, P, dsts, ex=None):
    """Both flag settings on the GPU against the restatement."""
    ex = ex or on(csr)
    for link_only, kernel in ((False, NODE), (True, LINK)):
        want = EN.lfa_tables_host(csr, cost, P, dsts, link_only)
        got = eng.lfa_tables(ex, cost, P, dsts, link_only=link_only)
        same(got, want)
        assert eng.ctx.last_kernel() == kernel and eng.ctx.last_launches() == 1
    return ex


def dev(eng, a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(eng.dev)


def dev_table(eng, P):
    return dev(eng, np.ascontiguousarray(P, np.uint32).view(np.int32), np.int32)


def raw(eng, d_P, dsts, V, counts=True, link_only=False, fill=7, timing=False):
    """One sdnr_lfa_tables call into tensors prefilled with ``fill``; no
    synchronize.  Returns (backup, backup_port, kind, counts or None, keep)."""
    import torch
    D = len(dsts)
    d_dst = dev(eng, dsts, np.int32)
    b = torch.full((D, V), fill, dtype=torch.int32, device=eng.dev)
    bp = torch.full((D, V), fill, dtype=torch.int32, device=eng.dev)
    k = torch.full((D, V), fill, dtype=torch.uint8, device=eng.dev)
    c = torch.full((D, 4), fill, dtype=torch.int32, device=eng.dev) if counts else None
    torch.cuda.synchronize()
    eng.ctx.lfa_tables_device(d_P.data_ptr(), d_dst.data_ptr(), D, b.data_ptr(), bp.data_ptr(),
                              k.data_ptr(), c.data_ptr() if counts else 0, link_only=link_only,
                              timing=timing)
    return b, bp, k, c, (d_dst, d_P)


# ------------------------------------------------------------ the small fabrics --

@pytest.mark.parametrize("hi", [1, 4, 65535])
@pytest.mark.parametrize("name", G.SMALL)
def test_small_fabrics_against_the_restatement(eng, name, hi):
    csr = G.Golden(name).fabric().csr()
    V = int(csr.V)
    cost = random_costs(csr, 1, hi, 3 * V + hi)
    P = all_pairs(csr, cost)
    ex = check(eng, csr, cost, P, np.arange(V))
    rng = np.random.default_rng(V + hi)
    # a count that is no multiple of anything, a single one, a permuted list
    # with a duplicate and ids outside [0, V)
    check(eng, csr, cost, P, np.arange(min(V, 7)), ex)
    check(eng, csr, cost, P, [V - 1], ex)
    perm = rng.permutation(V)
    check(eng, csr, cost, P, np.concatenate([perm, perm[:1], [-1, V]]), ex)
    # counts == NULL: the three tables alone
    eng.set_link_costs(ex, cost)
    want = EN.lfa_tables_host(csr, cost, P, perm)
    b, bp, k, c, keep = raw(eng, dev_table(eng, P), perm, V, counts=False)
    eng.ctx.synchronize()
    assert c is None
    same((b, bp, k, want[3]), want)
    if hi == 1:                                            # no costs uploaded: every link costs 1
        got = eng.lfa_tables(ex, None, P, np.arange(V))
        same(got, EN.lfa_tables_host(csr, None, P, np.arange(V)))


@pytest.mark.parametrize("name", NAMED)
def test_named_cases(eng, name):
    csr, cost, want = named_case(name)
    V = int(csr.V)
    P = all_pairs(csr, cost)
    ex = check(eng, csr, cost, P, np.arange(V))
    for link_only in (False, True):
        b, bp, k, _ = host4(eng.lfa_tables(ex, cost, P, np.arange(V), link_only=link_only))
        wb, wk = (np.asarray(a) for a in want[link_only])
        assert np.array_equal(b, wb) and np.array_equal(k, wk)
        assert np.array_equal(bp, ports_of(csr, wb))


# -------------------------------------------- rows wider than one / two wavefronts --

@pytest.mark.parametrize("rim", [70, 130])
def test_wheel_hub_rows_above_one_and_two_wavefronts(eng, rim):
    """Hub 0 and a rim ring 1 .. rim: the hub's row has ``rim`` links."""
    und = [(0, v) for v in range(1, rim + 1)] + \
          [(v, v % rim + 1) for v in range(1, rim + 1)]
    csr = digraph_csr(both_ways(und))
    V = rim + 1
    assert int(csr.row_ptr[1]) == rim
    for cost in (np.ones(int(csr.E), np.uint32), random_costs(csr, 1, 4, rim)):
        P = all_pairs(csr, cost)
        check(eng, csr, cost, P, np.arange(V))
    # unit costs: toward rim vertex d the hub's primary is d itself and its
    # alternate the smaller rim neighbour of d; toward the hub every rim
    # vertex falls back on a rim neighbour
    ones = np.ones(int(csr.E), np.uint32)
    b, bp, k, c = host4(eng.lfa_tables(on(csr), ones, all_pairs(csr, ones), np.arange(V)))
    for d in (1, 2, 64, 65, rim):
        nb = sorted(((d - 2) % rim + 1, d % rim + 1))
        assert b[d, 0] == nb[0] and k[d, 0] == 1
    assert (k[0, 1:] == 1).all() and k[0, 0] == 0
    assert b[0, 1] == 2 and b[0, rim] == 1 and b[0, 5] == 4
    assert c[0].tolist() == [rim, rim, 0, 0]


# ------------------------------------------------------------------ the V bound --

def ring_csr(V):
    v = np.arange(V, dtype=np.int64)
    src = np.concatenate([v, v]) + 1
    dst = np.concatenate([(v + 1) % V, (v - 1) % V]) + 1
    return T.build_csr(src, dst, np.repeat([1, 2], V))


def test_unit_ring_at_the_v_bound_alternate_only_at_the_antipode(eng):
    import torch
    V = EN.LFA_MAX_V
    csr = ring_csr(V)
    assert int(csr.V) == V and int(csr.E) == 2 * V
    ex = on(csr)
    a = torch.arange(V, dtype=torch.int32, device=eng.dev)
    P = (a[:, None] - a[None, :]).abs_()
    P = torch.minimum(P, V - P)
    dsts = [0, 5000, V - 1]
    edge = edge_map(csr)
    for link_only in (False, True):
        b, bp, k, c = host4(eng.lfa_tables(ex, None, P, dsts, link_only=link_only))
        wb = np.full((3, V), -1, np.int32)
        wp = np.full((3, V), -1, np.int32)
        wk = np.zeros((3, V), np.uint8)
        for i, d in enumerate(dsts):
            s = (d + V // 2) % V                            # both neighbours tie: smaller is primary
            n = max((s - 1) % V, (s + 1) % V)
            wb[i, s], wp[i, s] = n, csr.port[edge[(s, n)]]
            wk[i, s] = 3 if link_only else 7
        assert np.array_equal(b, wb) and np.array_equal(bp, wp) and np.array_equal(k, wk)
        assert c.tolist() == [[V - 1, 1, 0 if link_only else 1, 1]] * 3
    assert eng.ctx.last_kernel() == LINK


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
        eng.ctx.lfa_tables_device(small.data_ptr(), small.data_ptr(), 1, small.data_ptr(),
                                  small.data_ptr(), out8.data_ptr())
    assert ei.value.code == -22 and "16384" in str(ei.value)
    assert eng.ctx.last_kernel() == before
    eng.ctx.synchronize()
    with pytest.raises(ValueError):
        fake = TopologyDB(engine=eng)
        fake._lfa_rows(ex)


# --------------------------------------------------------------- the full fabrics --

def test_k48_first_core_group_at_cost_2_eight_rows(eng):
    csr = T.fat_tree(48).csr()
    V = int(csr.V)
    ex = on(csr)
    cost = core_tier_costs(csr, 48)
    d_P = eng.cost_tables(ex, cost, np.arange(V, dtype=np.int32))[0]
    P = d_P.cpu().numpy().view(np.uint32)
    deg = np.diff(csr.row_ptr)
    dsts = np.asarray([0, 575, 576, 1000, 1727, 1728, 2500, V - 1])
    assert set(deg[dsts].tolist()) == {24, 48}
    for link_only, kernel in ((False, NODE), (True, LINK)):
        want = EN.lfa_tables_host(csr, cost, P, dsts, link_only)
        got = eng.lfa_tables(ex, cost, d_P, dsts, link_only=link_only, timing=True)
        same(got, want)
        assert eng.ctx.last_kernel() == kernel and eng.ctx.last_launches() == 1
        assert eng.ctx.last_kernel_ms() > 0
        assert want[3][:, 1].all() and (want[3][:, 1] < want[3][:, 0]).all()


def test_dragonfly_a16_h8_p8_unit_costs_eight_rows(eng):
    csr = T.dragonfly(16, 8, 8).csr()
    V = int(csr.V)
    ex = on(csr)
    d_P = eng.cost_tables(ex, np.ones(int(csr.E), np.uint32), np.arange(V, dtype=np.int32))[0]
    P = d_P.cpu().numpy().view(np.uint32)
    dsts = np.asarray([0, 1, 15, 16, 1000, 1031, 2048, V - 1])
    for link_only, kernel in ((False, NODE), (True, LINK)):
        want = EN.lfa_tables_host(csr, None, P, dsts, link_only)
        got = eng.lfa_tables(ex, None, d_P, dsts, link_only=link_only)   # no costs uploaded
        same(got, want)
        assert eng.ctx.last_kernel() == kernel and eng.ctx.last_launches() == 1
        if not link_only:                                  # all three kinds of alternate occur
            kinds = set(np.unique(want[2]).tolist())
            assert {0, 1} <= kinds and kinds & {5, 7} and kinds & {3, 7}


# ------------------------------------------------------- argument and data errors --

def test_argument_errors(eng):
    import torch
    csr = G.Golden("random_V12").fabric().csr()
    V = int(csr.V)
    cost = random_costs(csr, 1, 4, 11)
    P = all_pairs(csr, cost)
    ex = on(csr)
    eng.set_link_costs(ex, cost)
    d_P = dev_table(eng, P)
    d_dst = dev(eng, np.arange(V), np.int32)
    i32 = lambda: torch.full((V, V), 7, dtype=torch.int32, device=eng.dev)     # noqa: E731
    b, bp = i32(), i32()
    k = torch.full((V, V), 7, dtype=torch.uint8, device=eng.dev)
    L, h = eng.ctx._lib, eng.ctx._h
    p = lambda t: ctypes.c_void_p(t.data_ptr())           # noqa: E731
    flag = _native.DEVICE_PTRS
    fn = L.sdnr_lfa_tables
    args = [p(d_P), p(d_dst), V, p(b), p(bp), p(k), None]

    def with_(i, v):
        a = list(args)
        a[i] = v
        return a
    torch.cuda.synchronize()
    assert fn(None, *args, flag) == -22
    assert fn(h, *args, 0) == -22 and b"device pointers only" in L.sdnr_last_error()
    for i in (0, 1, 3, 4, 5):                                             # required buffers
        assert fn(h, *with_(i, None), flag) == -22
    assert fn(h, *with_(2, -1), flag) == -22
    assert fn(h, *with_(2, 0), flag) == 0                                 # ndst == 0: nothing touched
    with _native.Context(0) as fresh:                                     # no graph uploaded
        assert fn(fresh._h, *args, flag) == -77
    eng.ctx.synchronize()
    assert (b == 7).all() and (bp == 7).all() and (k == 7).all()
    # a destination outside [0, V) is an empty row
    got = raw(eng, d_P, [3, V, -1, 0], V)
    eng.ctx.synchronize()
    want = EN.lfa_tables_host(csr, cost, P, [3, V, -1, 0])
    same((got[0], got[1], got[2], got[3].cpu().numpy().view(np.uint32)), want)
    assert (got[0][1:3] == -1).all() and (got[2][1:3] == 0).all() and not got[3][1:3].any()


@pytest.mark.parametrize("bad", ["diagonal", "tightless"])
def test_a_bad_row_is_reported_and_the_others_stand(eng, bad):
    csr = G.Golden("random_V12").fabric().csr()
    V = int(csr.V)
    cost = random_costs(csr, 1, 4, 11)
    P = all_pairs(csr, cost)
    ex = on(csr)
    eng.set_link_costs(ex, cost)
    Pb = P.copy()
    if bad == "diagonal":
        Pb[4, 4] = 5
    else:
        x = int(np.nonzero((P[4] != INF) & (P[4] != 0))[0][0])
        Pb[4, x] += 100000                    # finite, and no link of x is tight any more
    dsts = [2, 4, 7]
    got = raw(eng, dev_table(eng, Pb), dsts, V)
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "sdnr_lfa_tables" in str(ei.value)
    # rows 2 and 7 are what the table as given defines (an edited P[4][x] is
    # also P[s][n] of the link 4 -> x in every row): the restatement on it
    want = EN.lfa_tables_host(csr, cost, Pb, dsts)
    for i in (0, 2):
        for a, w in zip(host4(got[:3]), want[:3]):
            assert np.array_equal(a[i], w[i])
        assert np.array_equal(got[3][i].cpu().numpy().view(np.uint32), want[3][i])
    # the context stays usable: the next call is clean
    same(eng.lfa_tables(ex, cost, P, dsts), EN.lfa_tables_host(csr, cost, P, dsts))


def test_neighbour_pair_scratch_above_the_cap_is_nomem_naming_the_flag(eng):
    """The complete digraph on 650 vertices: 650 * 649^2 * 4 bytes of
    neighbour-pair matrices, just above the 1 GiB of scratch -- refused from
    the degrees alone, before any allocation or launch."""
    import torch
    n = 650
    assert n * (n - 1) ** 2 * 4 > 1 << 30
    u, v = np.nonzero(~np.eye(n, dtype=bool))
    csr = T.build_csr(u + 1, v + 1, np.ones(u.shape[0], np.int64))
    eng.load(on(csr))
    z = torch.zeros((n, n), dtype=torch.int32, device=eng.dev)
    k = torch.zeros((1, n), dtype=torch.uint8, device=eng.dev)
    torch.cuda.synchronize()
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.lfa_tables_device(z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), z.data_ptr(),
                                  k.data_ptr())
    assert ei.value.code == -12 and "SDNR_LFA_LINK_ONLY" in str(ei.value)
    eng.ctx.synchronize()


# ------------------------------------------------------------------ the drop-in --

@pytest.mark.parametrize("name", ["fat_tree_k4", "random_V12"])
def test_dropin_on_the_engine_equals_the_engine_double(eng, name):
    g = G.Golden(name)
    fabric = g.fabric()
    pairs = golden_pairs(g, fabric)
    db = fabric.populate(TopologyDB(engine=eng))
    twin = fake_db(fabric)
    links = sorted((a, b) for a in db.links for b in db.links[a])
    costs = {links[i]: 1 + i % 3 for i in range(0, len(links), 2)}
    db.set_link_costs(costs)
    twin.set_link_costs(costs)
    assert dropin_state(db, pairs) == dropin_state(twin, pairs)
    assert db.lfa_coverage()["backups"] > 0
    for step in ("set_link_cost", "delete_link", "add_link"):
        mutate(db, links, step)
        mutate(twin, links, step)
        assert dropin_state(db, pairs) == dropin_state(twin, pairs), step
