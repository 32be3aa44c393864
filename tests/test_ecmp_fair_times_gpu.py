"""sdnr_ecmp_fair_times on the GPU (ecmp_fair_times.hip) against its numpy
restatement engine.ecmp_fair_times_host: the epoch count, every flow's epoch
and every filling's round count equal, the doubles within
test_ecmp_fair_times.TOL -- bit for bit where every partial sum is exact --,
with the launch count engine.fair_times_launches(epoch_rounds) on every call.
The restatement itself is checked against an exact simulation in
test_ecmp_fair_times.py."""
import types

import numpy as np
import pytest

import over_grid as OG
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from test_cost_ecmp_loads import chord_ladder_csr, diamond_csr, pcost_rows, random_costs
from test_ecmp_fair_rates import ECMP_ROUTES, SPLITS, seed_costs, small_case
from test_ecmp_fair_rates_gpu import padded_diamond, path_case
from test_ecmp_fair_times import TOL, case_bytes, star_49, times_db
from test_ecmp_link_loads import edge_map
from test_fair_rates import CAPS, dropin_pairs
from test_fair_times import FABRICS

pytestmark = pytest.mark.gpu

LDS, GLOBAL = "ecmp_fair_times_rows_kernel<lds>", "ecmp_fair_times_rows_kernel<global>"
NAMES = ("time", "epoch", "rate0", "remaining", "epoch_time", "epoch_rounds", "carried")


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def on(csr):
    """The export-shaped handle RouteEngine wants for a bare CSR."""
    return types.SimpleNamespace(csr=csr)


def close(got, want, bits=False):
    """The 7-tuple: epochs, epoch and epoch_rounds equal; the doubles within
    TOL (+inf and 0.0 equal), or bit for bit."""
    for g, w, name in zip(got, want, NAMES):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if g.dtype != np.float64:
            assert np.array_equal(g, w), name
        elif bits:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), name
        else:
            assert np.array_equal(g == 0, w == 0), name
            assert np.allclose(g, w, rtol=TOL, atol=0), name


def both(eng, csr, cost, pcost, rows, srcs, mult, nbytes, cap, extra=None, split="route",
         kernel=LDS, bits=False, max_epochs=None):
    """One case on the device and in numpy; the results must agree."""
    want = EN.ecmp_fair_times_host(csr, cost, pcost, rows, srcs, mult, nbytes, cap, extra, split,
                                   max_epochs)
    got = eng.ecmp_fair_times(on(csr), cost, np.asarray(pcost), rows, srcs, mult, nbytes, cap,
                              extra, split, max_epochs)
    close(got, want, bits)
    assert eng.ctx.last_kernel() == kernel
    assert eng.ctx.last_launches() == EN.fair_times_launches(want[5])
    return want


# ------------------------------------------------------ the small fabrics --

@pytest.mark.parametrize("name", FABRICS)
def test_small_fabrics_to_completion_both_splits_unit_and_random_costs(eng, name):
    c = small_case(name)
    assert c["csr"].V <= 20
    nbytes = case_bytes(name, c["rows"].shape[0])
    for cost, pc in ((None, c["pc_unit"]), (c["cost"], c["pc_cost"])):
        for split in SPLITS:
            r = both(eng, c["csr"], cost, pc, c["rows"], c["srcs"], c["mult"], nbytes, c["cap"],
                     split=split)
            assert len(r[4]) > 1 and (r[1] != -2).all()


@pytest.mark.parametrize("k,most", [(4, None), (8, 4)])
def test_fat_tree_between_edge_switches_bit_for_bit(eng, k, most):
    """Edge to edge on a fat-tree every fraction is a power of two; with integer
    multiplicities and power-of-two capacities every partial sum is exact."""
    fabric = T.fat_tree(k)
    csr = fabric.csr()
    hv, _ = fabric.host_table()
    edges = np.unique(hv)
    n = edges.shape[0]
    pc = pcost_rows(csr, np.ones(int(csr.E), np.uint32), edges)
    rows, srcs = np.repeat(np.arange(n), n), np.tile(edges, n)
    rng = np.random.default_rng(40 + k)
    mult = rng.integers(0, 6, n * n).astype(np.uint64)
    cap = rng.choice(np.asarray([1, 2, 4, 16, 64], np.float64), int(csr.E))
    nbytes = rng.integers(1, 1001, n * n).astype(np.float64)
    for split in SPLITS:
        r = both(eng, csr, None, pc, rows, srcs, mult, nbytes, cap, split=split, bits=True,
                 max_epochs=most)
        assert len(r[4]) == (most or len(r[4])) > 3 and int(r[5].max()) > 1
        assert ((r[1] == -2).any()) == (most is not None)


def test_diamond_closed_forms_and_the_49_case(eng):
    csr, cost, (s, m, d) = diamond_csr()
    em = edge_map(csr)
    E = int(csr.E)
    pc = pcost_rows(csr, cost, [d, s])
    cap = np.full(E, 10.0)
    cap[em[(s, m)]] = 1.0
    for split in SPLITS:
        r = both(eng, csr, cost, pc, [0, 0], [s, m], None, [4.0, 36.0], cap, split=split,
                 bits=True)
        assert r[0].tolist() == [2.0, 3.8] and r[2].tolist() == [2.0, 9.0]
        assert r[5].tolist() == [2, 1]
        # next hops at different hop depths (the direct link of cost 2 against
        # two links of cost 1), two rows, unsorted flows, extras, zero bytes
        capx = np.concatenate([np.asarray([3, 1, 2, 10, 40, 100], np.float64)[:E], [0.5, 7.0]])
        extra = [[-1, -1], [E, -1], [E + 1, E], [-1, -1], [E + 1, E + 1], [-1, -1], [-1, -1]]
        r = both(eng, csr, cost, pc, [0, 1, 0, 1, 0, 0, 0], [s, d, m, m, d, d, m],
                 [2, 1, 1, 3, 1, 4, 1], [7.0, 3.0, 9.0, 100.0, 5.0, 6.0, 0.0], capx, extra,
                 split=split)
        assert r[2][5] == np.inf and r[0][5] == 0.0 and r[0][6] == 0.0 and len(r[4]) > 2
    csr, pc, rows, srcs, mult, nbytes, cap = star_49()
    for split in SPLITS:
        r = both(eng, csr, None, pc, rows, srcs, mult, nbytes, cap, split=split, bits=True)
        assert r[0].tolist() == [49.0, 49.0] and r[4].tolist() == [49.0] and r[5].tolist() == [2]


def test_path_of_40_one_flow_per_epoch_across_clock_batches(eng):
    """39 epochs of 39, 38, ... 1 rounds: more than 16 epochs, and fillings that
    cross a batch boundary of the clock."""
    csr, pc, cap, em = path_case(40)
    v = np.arange(40)
    nbytes = (2.0 * v + 1) * (39 - v)
    r = both(eng, csr, None, pc, [0] * 40, v, None, nbytes, cap, bits=True)
    assert r[1][:39].tolist() == list(range(38, -1, -1)) and r[1][39] == -1
    assert r[5].tolist() == list(range(39, 0, -1)) and r[2][39] == np.inf and r[0][39] == 0.0


def test_chord_ladder_70_thirds_and_deep_chains(eng):
    """Thirds: inexact fractions; 3**70 routes from the first joint and a
    longest next-hop chain of 140 links."""
    csr, cost = chord_ladder_csr(70)
    d = 210
    pc = pcost_rows(csr, cost, [d])
    rows, srcs = [0] * (d + 1), list(range(d + 1))
    E = int(csr.E)
    nbytes = np.random.default_rng(77).integers(1, 1001, d + 1).astype(np.float64)
    for split in SPLITS:
        r = both(eng, csr, cost, pc, rows, srcs, [1 + (v % 4) for v in srcs], nbytes,
                 np.asarray(CAPS, np.float64)[np.arange(E) % len(CAPS)], split=split,
                 max_epochs=8)
        assert len(r[4]) == 8 and (r[1] == -2).any()


# ------------------------------------------------------------ global form --

def test_global_form_past_the_lds_threshold(eng):
    V = EN.ECMP_FAIR_LDS_MAX_V + 1
    csr, cost, (s, m, d) = padded_diamond(V)
    assert int(csr.V) == V
    dsts = [d, s, 5, V - 1]
    pc = pcost_rows(csr, cost, dsts)
    E = int(csr.E)
    em = edge_map(csr)
    cap = np.full(E, 10.0)
    cap[[em[(s, m)], em[(m, d)], em[(m, 5)]]] = [1.0, 3.0, 2.0]
    core_rows, core_srcs, core_mult = [0, 0, 1, 1], [s, m, d, m], [1, 2, 1, 1]
    core_bytes = [4.0, 30.0, 11.0, 50.0]
    for split in SPLITS:
        big = both(eng, csr, cost, pc, core_rows, core_srcs, core_mult, core_bytes, cap,
                   split=split, kernel=GLOBAL)
        # the same flows on the core alone, in the LDS form
        c3, cost3, _ = diamond_csr()
        em3 = edge_map(c3)
        cap3 = np.full(int(c3.E), 10.0)
        cap3[[em3[(s, m)], em3[(m, d)]]] = [1.0, 3.0]
        small = both(eng, c3, cost3, pcost_rows(c3, cost3, [d, s]), core_rows, core_srcs,
                     core_mult, core_bytes, cap3, split=split, kernel=LDS)
        assert np.array_equal(big[0], small[0]) and np.array_equal(big[1], small[1])
        assert np.array_equal(big[5], small[5]) and len(big[4]) > 1
        # leaves as sources and destinations, every row, out-of-range and absent flows
        rows = [0, 0, 1, 2, 2, 3, 3, 0, 2, 3, 0]
        srcs = [s, 7, V - 1, s, 6, 5, d, V, 5, -1, 9]
        mult = [1, 3, 2, 1, 1, 4, 1, 1, 1, 1, 0]
        nbytes = [5.0, 9.0, 2.0, 40.0, 4.0, 4.0, 7.0, 1.0, 30.0, 3.0, 8.0]
        r = both(eng, csr, cost, pc, rows, srcs, mult, nbytes, cap, split=split, kernel=GLOBAL)
        assert r[2][8] == np.inf and np.isinf(r[0][[7, 9, 10]]).all() and len(r[4]) > 2


def test_lds_form_at_the_threshold(eng):
    V = EN.ECMP_FAIR_LDS_MAX_V
    csr, cost, (s, m, d) = padded_diamond(V)
    pc = pcost_rows(csr, cost, [d, V - 1])
    cap = np.full(int(csr.E), 10.0)
    cap[edge_map(csr)[(s, m)]] = 1.0
    r = both(eng, csr, cost, pc, [0, 0, 1, 1], [s, m, s, 9], [1, 2, 1, 3],
             [4.0, 30.0, 11.0, 50.0], cap, kernel=LDS)
    assert len(r[4]) > 1


# ------------------------------------------------- more rows than workgroups --

def test_more_rows_than_workgroups_three_epochs(eng):
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    csr, comp = OG.graph()
    ids = np.arange(csr.V, dtype=np.int32)
    cost = random_costs(csr, 1, 5, 900)
    n = OG.units(cus)
    m = OG.row_mix(csr, comp, n, 930, OG.strides_for(cus, n))
    cap = np.random.default_rng(931).choice(np.asarray(CAPS, np.float64), int(csr.E))
    nbytes = np.random.default_rng(932).integers(0, 200, len(m.rows)).astype(np.float64)
    for c, split in ((None, "route"), (cost, "hop")):
        pc = pcost_rows(csr, np.ones(int(csr.E), np.uint32) if c is None else c, ids)[m.dst]
        want = both(eng, csr, c, pc, m.rows, m.ends, m.w, nbytes, cap, split=split, max_epochs=3)
        grid = eng.ctx.last_grid()
        assert 0 < grid < len(m.kind) and len(m.kind) >= 2 * grid + 1
        OG.check_units(m.kind, m.key, grid)
        assert len(want[4]) == 3 and (want[1] >= 0).any() and (want[1] == -2).any()


# ---------------------------------------------------------------- odd input --

def raw(eng, csr, cost, pcost, nrows, off, srcs, nbytes, cap, extra=None, max_epochs=None,
        hop=False):
    """One sdnr_ecmp_fair_times call on device copies; returns (epochs, outputs,
    inputs) without synchronize."""
    import torch
    ex = on(csr)
    eng.load(ex)
    if cost is None:
        eng._costs = None
        eng.ctx.set_link_costs(None)
    else:
        eng.set_link_costs(ex, cost)
    n = len(srcs)
    nx = len(cap) - csr.E
    me = n if max_epochs is None else max_epochs
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(eng.dev)  # noqa
    keep = [t(np.asarray(pcost, np.uint32).view(np.int32), np.int32), t(off, np.int64),
            t(srcs, np.int32), t(nbytes, np.float64), t(cap, np.float64),
            t(extra, np.int32) if extra is not None else None]
    f64 = lambda k: torch.full((max(k, 1),), 7.0, dtype=torch.float64, device=eng.dev)  # noqa
    i32 = lambda k: torch.full((max(k, 1),), 7, dtype=torch.int32, device=eng.dev)      # noqa
    out = [f64(n), i32(n), f64(n), f64(n), f64(me), i32(me), f64(len(cap))]
    torch.cuda.synchronize()
    p = lambda x: x.data_ptr() if x is not None else 0    # noqa: E731
    epochs = eng.ctx.ecmp_fair_times_device(p(keep[0]), nrows, p(keep[1]), p(keep[2]), 0,
                                            p(keep[3]), p(keep[5]), p(keep[4]), nx, p(out[0]),
                                            p(out[1]), p(out[2]), p(out[3]), p(out[4]), p(out[5]),
                                            me, p(out[6]), hop=hop)
    return epochs, out, keep


def test_no_rows_and_no_pairs(eng):
    csr, cost, (s, m, d) = diamond_csr()
    eng.load(on(csr))
    assert eng.ctx.ecmp_fair_times_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                          0) == 0
    pc = pcost_rows(csr, cost, [d])
    epochs, out, keep = raw(eng, csr, cost, pc, 1, [2, 2], [0, 0, 0], [1.0] * 3, np.ones(csr.E))
    eng.ctx.synchronize()
    assert epochs == 0 and all(float(o.cpu()[0]) == 7 for o in out)       # nothing touched
    r = eng.ecmp_fair_times(on(csr), cost, pc, [], [], None, [], np.ones(csr.E))
    assert [len(x) for x in r] == [0] * 6 + [csr.E]
    del keep


def check_raw(eng, epochs, out, csr, cost, pcost, rows, srcs, nbytes, cap, good, absent, what,
              extra=None):
    """The call reported ``what`` once as SDNR_ERR_INVAL; the flows ``good``
    are what they are alone and the flows ``absent`` read +inf / -1 / 0.0."""
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "sdnr_ecmp_fair_times" in str(ei.value)
    assert what in str(ei.value)
    eng.ctx.synchronize()                                  # reported once
    want = EN.ecmp_fair_times_host(csr, cost, pcost, np.asarray(rows)[good],
                                   np.asarray(srcs)[good], None, np.asarray(nbytes)[good], cap,
                                   extra)
    got = [o.cpu().numpy() for o in out]
    assert epochs == len(want[4]) > 0
    assert np.array_equal(got[1][good], want[1])
    for k in (0, 2, 3):
        assert np.allclose(got[k][good], want[k], rtol=TOL, atol=0), NAMES[k]
    assert np.allclose(got[4][:epochs], want[4], rtol=TOL, atol=0)
    assert np.array_equal(got[5][:epochs], want[5])
    assert np.allclose(got[6], want[6], rtol=TOL, atol=0)
    assert np.isinf(got[0][absent]).all() and (got[1][absent] == -1).all()
    assert not got[2][absent].any()
    assert np.array_equal(got[3][absent], np.asarray(nbytes, np.float64)[absent], equal_nan=True)


def test_a_row_that_is_no_labelling_and_bad_offsets_are_reported_the_others_stand(eng):
    """Row 1 gives m a cost that no link explains; rows 3 and 4 have offsets
    outside the pair list."""
    csr, cost, (s, m, d) = diamond_csr()
    good = pcost_rows(csr, cost, [d, s])
    pc = np.vstack([good[:1], good[:1], good[1:], good[:1], good[:1], good[:1]])
    pc[1, m] = 7
    cap = np.arange(1, csr.E + 1, dtype=np.float64)
    srcs = [s, m, s, m, d, m, s, m]
    nbytes = [5.0, 9.0, 2.0, 4.0, 14.0, 3.0, 6.0, 1.0]
    off = [0, 2, 4, 6, 100, 6, 8]               # row 3 = [6, 100), row 4 = [100, 6): both bad
    epochs, out, keep = raw(eng, csr, cost, pc, 6, off, srcs, nbytes, cap)
    ok = [0, 1, 4, 5, 6, 7]
    rows = [0, 0, 1, 1, 2, 2, 5, 5]
    check_raw(eng, epochs, out, csr, cost, pc, rows, srcs, nbytes, cap, ok, [2, 3], "labelling")
    # the context goes on working
    r = eng.ecmp_fair_times(on(csr), cost, good, [0], [m], None, [3.0], cap)
    assert r[0].tolist() == [3.0 / cap[edge_map(csr)[(m, d)]]]
    del keep


@pytest.mark.parametrize("bad", [-2.0, float("nan"), float("inf")])
def test_bad_byte_sizes_are_reported_and_absent(eng, bad):
    csr, cost, (s, m, d) = diamond_csr()
    pc = pcost_rows(csr, cost, [d, s])
    cap = np.arange(1, csr.E + 1, dtype=np.float64)
    rows, srcs = [0, 0, 0, 1, 1, 1], [s, m, s, m, d, m]
    nbytes = [5.0, bad, 2.0, 7.0, 1.0, 30.0]
    with pytest.raises(ValueError):
        eng.ecmp_fair_times(on(csr), cost, pc, rows, srcs, None, nbytes, cap)
    epochs, out, keep = raw(eng, csr, cost, pc, 2, [0, 3, 6], srcs, nbytes, cap)
    check_raw(eng, epochs, out, csr, cost, pc, rows, srcs, nbytes, cap, [0, 2, 3, 4, 5], [1],
              "byte size")
    del keep


@pytest.mark.parametrize("bad", [0.0, -2.0, float("nan"), float("inf")])
def test_bad_capacities_are_reported(eng, bad):
    csr, cost, (s, m, d) = diamond_csr()
    pc = pcost_rows(csr, cost, [d])
    cap = np.ones(csr.E)
    cap[edge_map(csr)[(m, d)]] = bad
    with pytest.raises(ValueError):
        eng.ecmp_fair_times(on(csr), cost, pc, [0], [s], None, [1.0], cap)
    epochs, out, keep = raw(eng, csr, cost, pc, 1, [0, 2], [s, m], [1.0, 2.0], cap)
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "capacity" in str(ei.value)
    eng.ctx.synchronize()
    assert 0 <= epochs <= 2
    del keep


def test_an_extra_out_of_range_is_reported_and_ignored(eng):
    csr, cost, (s, m, d) = diamond_csr()
    E = int(csr.E)
    pc = pcost_rows(csr, cost, [d])
    cap = np.concatenate([np.arange(1, E + 1, dtype=np.float64), [0.5]])
    srcs, nbytes = [s, m, m], [5.0, 9.0, 2.0]
    extra = [[E, -1], [E + 1, -1], [-1, 3]]      # E + 1 and 3 are no extras: ignored
    with pytest.raises(ValueError):
        eng.ecmp_fair_times(on(csr), cost, pc, [0] * 3, srcs, None, nbytes, cap, extra)
    epochs, out, keep = raw(eng, csr, cost, pc, 1, [0, 3], srcs, nbytes, cap, extra)
    check_raw(eng, epochs, out, csr, cost, pc, [0] * 3, srcs, nbytes, cap, [0, 1, 2], [], "extra",
              extra=[[E, -1], [-1, -1], [-1, -1]])
    del keep


def test_max_epochs_reached_leaves_epoch_minus_2_and_what_is_left(eng):
    csr, cost, (s, m, d) = diamond_csr()
    pc = pcost_rows(csr, cost, [d])
    cap1 = np.full(int(csr.E), 3.0)
    em = edge_map(csr)
    for most, left, carried in ((0, [2.0, 5.0, 14.0], 0.0), (1, [0.0, 3.0, 12.0], 3.0),
                                (2, [0.0, 0.0, 9.0], 6.0), (3, [0.0] * 3, 10.5),
                                (9, [0.0] * 3, 10.5)):
        r = both(eng, csr, cost, pc, [0] * 3, [s] * 3, None, [2.0, 5.0, 14.0], cap1, bits=True,
                 max_epochs=most)
        done = min(most, 3)
        assert r[1].tolist() == [0, 1, 2][:done] + [-2] * (3 - done) and len(r[4]) == done
        assert r[3].tolist() == left and r[6][em[(s, d)]] == carried
        assert np.isinf(r[0][done:]).all() and r[0][:done].tolist() == [1.0, 2.0, 3.5][:done]


def test_argument_errors(eng):
    import ctypes
    import torch
    csr, cost, _ = diamond_csr()
    eng.load(on(csr))
    L, h = eng.ctx._lib, eng.ctx._h
    buf = torch.zeros(64, dtype=torch.int64, device=eng.dev)
    p = ctypes.c_void_p(buf.data_ptr())
    n = ctypes.c_int32(9)
    dev = _native.DEVICE_PTRS

    def call(pcost, nrows, flags, nextra=0, max_epochs=2, nep=ctypes.byref(n), ctx=h):
        return L.sdnr_ecmp_fair_times(ctx, pcost, nrows, p, p, None, p, None, p, nextra, p, p, p, p,
                                      p, p, max_epochs, p, nep, flags)

    assert call(p, 1, 0) == -22 and n.value == 0                          # host pointers
    assert call(None, 1, dev) == -22
    assert call(p, -1, dev) == -22
    assert call(p, 1, dev, -1) == -22
    assert call(p, 1, dev, 0, -1) == -22
    assert call(p, 1, dev, nep=None) == -22
    buf[0] = 5                                                            # pair_off[0] > pair_off[1]
    torch.cuda.synchronize()
    assert call(p, 1, dev) == -22 and b"monotone" in L.sdnr_last_error()
    with _native.Context(0) as fresh:                                     # no graph uploaded
        assert call(p, 1, dev, ctx=fresh._h) == -77
    with pytest.raises(ValueError, match="split"):
        eng.ecmp_fair_times(on(csr), cost, np.zeros((1, 3), np.uint32), [0], [0], split="flow")
    with pytest.raises(ValueError, match="row"):
        eng.ecmp_fair_times(on(csr), cost, np.zeros((1, 3), np.uint32), [1], [0])
    assert "sdnr_ecmp_fair_times" in _native.EXPORTED_SYMBOLS


# ---------------------------------------------------------------- drop-in --

def test_dropin_fat_tree_both_routes_both_splits_and_host_ports():
    from sdnmpi_amd.util.topology_db import TopologyDB
    fabric = T.fat_tree(4)
    double = times_db(fabric)
    capacity = seed_costs(double)
    db = fabric.populate(TopologyDB())
    assert seed_costs(db) == capacity
    pairs, w = dropin_pairs(fabric)
    nbytes = np.random.default_rng(33).integers(0, 1001, len(pairs)).astype(np.float64)
    for route in ECMP_ROUTES:
        for split in SPLITS:
            for hc in (None, 2.5):
                a = db.fair_completion_times(pairs, nbytes, w, capacity, hc, route, split=split)
                b = double.fair_completion_times(pairs, nbytes, w, capacity, hc, route,
                                                 split=split)
                for name in ("time", "rate0", "remaining", "epoch_time", "link_bytes.load"):
                    x, y = a, b
                    for part in name.split("."):
                        x, y = getattr(x, part), getattr(y, part)
                    assert np.allclose(x, y, rtol=TOL, atol=0), (route, split, hc, name)
                assert np.array_equal(a.epoch, b.epoch) and np.array_equal(a.routed, b.routed)
                assert np.array_equal(a.epoch_rounds, b.epoch_rounds) and a.epochs > 4
                assert a.makespan() == pytest.approx(b.makespan(), rel=TOL) and a.complete
                assert a.split == b.split == split
            ap = db.all_pairs_fair_completion_times(64.0, capacity, route, 5, split)
            bp = double.all_pairs_fair_completion_times(64.0, capacity, route, 5, split)
            assert np.allclose(ap.time, bp.time, rtol=TOL, atol=0)
            assert np.array_equal(ap.epoch, bp.epoch) and ap.complete == bp.complete
            assert np.allclose(ap.remaining, bp.remaining, rtol=TOL, atol=0)
    ranks = dict(enumerate(fabric.host_macs()[::2]))
    traffic = {(i, (i + 3) % len(ranks)): 1000 * (i + 1) for i in ranks}
    a = db.mpi_exchange_times(ranks, traffic, capacity, 2.5, "least_cost_ecmp", split="hop")
    b = double.mpi_exchange_times(ranks, traffic, capacity, 2.5, "least_cost_ecmp", split="hop")
    assert np.allclose(a.time, b.time, rtol=TOL, atol=0)
    assert a.makespan() == pytest.approx(b.makespan(), rel=TOL) and a.makespan() > 0
