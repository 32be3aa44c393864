"""The input builder of the over-grid GPU tests (over_grid.py), CPU only: the
unit mixes hold every kind of unit where the GPU tests need it, and the host
restatements the GPU tests compare against are linear over repeated rows --
the restatement of the whole mix equals the sum of the restatements of its
distinct destinations, exactly for the integer kernels and within RTOL for the
float ones -- so the fixture is checked without a GPU."""
import numpy as np
import pytest

import over_grid as OG
from sdnmpi_amd import engine as EN
from test_cost_ecmp_loads import pcost_rows, random_costs
from test_ecmp_link_loads import SPLITS, close

CUS = 256
N = 2560


def tables():
    from oracle import oracle as O
    csr, comp = OG.graph()
    ids = np.arange(csr.V, dtype=np.int32)
    par, _, _ = O.dfs_tables(csr, ids)
    dist, _, _ = O.dest_tables(csr, ids)
    return csr, comp, par, dist


def test_units_arithmetic():
    assert OG.units(256) == 2560 and OG.units(256, 8) == 5120 and OG.units(256, 1) == 640
    for cus in (1, 3, 8, 256, 304):
        for mult in (1, 2, 4, 8):
            g, n = cus * mult, OG.units(cus, mult)
            assert n >= 2 * g + 1 or g == 1
            per = np.bincount(np.arange(n) % g, minlength=g)       # units of each workgroup
            assert per.max() == 3 or g == 1
            assert (per == 3).sum() == g // 2 and (per == 2).sum() == g - g // 2
    assert OG.strides_for(256, 2560) == (256, 512, 1024)
    assert OG.strides_for(256, 5120) == (256, 512, 1024, 2048)


def test_graph_has_two_components_and_isolated_vertices():
    csr, comp = OG.graph()
    assert csr.V == 44
    sizes = sorted(np.bincount(comp)[np.unique(comp)].tolist())
    assert sizes == [1] * 8 + [4, 32]


def test_row_mix_holds_every_kind_between_working_rows():
    csr, comp = OG.graph()
    V = csr.V
    strides = OG.strides_for(CUS, N)
    for bad_dst, errors in ((False, False), (True, False), (False, True)):
        m = OG.row_mix(csr, comp, N, 11, strides, bad_dst=bad_dst, errors=errors)
        want = {OG.EMPTY} | ({OG.BAD_DST} if bad_dst else set()) | \
            ({OG.ERR_OFF, OG.ERR_ROW} if errors else set())
        assert set(m.kind.tolist()) == want | {OG.WORK}
        for s in strides:
            OG.check_units(m.effective, m.key, s)
        share = np.bincount(m.kind, minlength=5) / N
        assert 0.12 < share[OG.EMPTY] < 0.18
        if bad_dst:
            assert 0.03 < share[OG.BAD_DST] < 0.07
            bad = m.dst[m.kind == OG.BAD_DST]
            assert ((bad < 0) | (bad >= V)).all() and (bad < 0).any() and (bad >= V).any()
        if errors:
            assert 0.01 < share[OG.ERR_OFF] + share[OG.ERR_ROW] < 0.03
        ok = m.kind != OG.BAD_DST
        assert ((m.dst[ok] >= 0) & (m.dst[ok] < V)).all()
        assert len(set(m.dst[ok].tolist())) == V               # every vertex is a destination
        # pairs: none on an empty row, 1 to 5 elsewhere, in row order
        per = np.bincount(m.rows, minlength=N)
        assert (per[m.kind == OG.EMPTY] == 0).all()
        rest = per[m.kind != OG.EMPTY]
        assert rest.min() == 1 and rest.max() == 5 and (np.diff(m.rows) >= 0).all()
        # the ends: the row's own destination, ids outside [0, V), another component
        d = m.key[m.rows]
        inside = (m.ends >= 0) & (m.ends < V)
        assert (m.ends == d).any() and (m.ends < 0).any() and (m.ends >= V).any()
        other = inside & (comp[np.where(inside, m.ends, 0)] != comp[d])
        same = inside & (comp[np.where(inside, m.ends, 0)] == comp[d]) & (m.ends != d)
        assert other.sum() > N // 10 and same.sum() > N // 10
        assert m.w.dtype == np.uint64 and m.w.max() < 1 << 32
        assert 0.25 < (m.w == 0).mean() < 0.35


def test_broken_offsets_reject_two_rows_and_keep_the_ends():
    csr, comp = OG.graph()
    m = OG.row_mix(csr, comp, N, 12, OG.strides_for(CUS, N), errors=True)
    good = OG.pair_offsets(m)
    off, live = OG.bad_offsets(m)
    assert off[0] == good[0] == 0 and off[-1] == good[-1] == m.rows.shape[0]
    lo, hi = off[:-1], off[1:]
    rejected = (lo < off[0]) | (hi > off[-1]) | (hi < lo)
    want = m.effective == OG.ERR_OFF
    assert np.array_equal(rejected, want) and want.sum() >= 2 * (m.kind == OG.ERR_OFF).sum() - 2
    assert np.array_equal(off[:-1][~rejected], good[:-1][~rejected])
    assert np.array_equal(off[1:][~rejected], good[1:][~rejected])
    dead = rejected | (m.kind == OG.ERR_ROW)
    assert np.array_equal(live, ~dead[m.rows]) and not live.all() and live.mean() > 0.9


@pytest.mark.parametrize("B", [1, 4, 6, 8])
def test_dest_mix(B):
    csr, _ = OG.graph()
    V = csr.V
    strides = OG.strides_for(CUS, N)
    d, kind = OG.dest_mix(csr, N, B, 13, strides, p_bad=0.05 if B == 1 else 0.01)
    assert (d.shape[0] + B - 1) // B == N and (B == 1 or d.shape[0] % B)
    keys = OG.batch_keys(d, B)
    for s in strides:
        OG.check_units(kind, keys, s)
    bad = (d < 0) | (d >= V)
    assert (d < 0).any() and (d >= V).any() and 0.01 < bad.mean() < 0.1
    whole = bad_batches = ((keys < 0) | (keys >= V)).all(axis=1)
    assert np.array_equal(whole, kind == OG.BAD_DST) and bad_batches.any()


def test_group_mix():
    csr, comp = OG.graph()
    V = csr.V
    strides = OG.strides_for(CUS, N)
    for errors in (False, True):
        m = OG.group_mix(csr, comp, N, 14, strides, errors=errors)
        for s in strides:
            OG.check_units(m.effective, m.key, s)
        per = np.diff(m.mem_off)
        assert (per[m.kind == OG.EMPTY] == 0).all() and per[m.kind != OG.EMPTY].min() >= 5
        grp = np.repeat(np.arange(N), per)
        r, v = m.key[grp], m.mem_vertex
        inside = (v >= 0) & (v < V)
        assert (v == r).any() and (~inside).any()
        assert (inside & (comp[np.where(inside, v, 0)] != comp[r])).any()
        assert ((m.mem_row < 0) | (m.mem_row >= V)).any()
        first = m.mem_off[:-1][per > 0]
        assert (m.mem_vertex[first] == m.mem_vertex[first + per[per > 0] - 4]).all()   # a repeat
        bad = m.root[m.kind == OG.BAD_DST]
        assert ((bad < 0) | (bad >= V)).all() and bad.size


def test_group_mix_over_a_pool_of_destinations():
    csr, _ = OG.graph()
    V = csr.V
    pool = np.asarray([3, 9, 20, 41])
    strides = OG.strides_for(CUS, N)
    m = OG.group_mix(csr, None, N, 18, strides, pool=pool)
    for s in strides:
        OG.check_units(m.kind, m.key, s)
    assert {OG.EMPTY, OG.BAD_DST} <= set(m.kind.tolist())
    inside = (m.mem_row >= 0) & (m.mem_row < pool.shape[0])
    v_ok = (m.mem_vertex >= 0) & (m.mem_vertex < V)
    assert (~inside).any() and (~v_ok).any()
    both = inside & v_ok
    assert np.array_equal(pool[m.mem_row[both]], m.mem_vertex[both])   # a member's row is its own


def test_failure_scenarios():
    csr, _ = OG.graph()
    scen = OG.failure_scenarios(csr, 5)
    assert scen[0] == [] and len(scen[1]) == 2
    assert (np.asarray(csr.col)[scen[3]] == 5).all()
    assert len(scen[3]) == int((np.asarray(csr.col) == 5).sum())
    for s in scen:
        assert s == sorted(set(s))


def by_destination(mix):
    """(d, pair indices) per distinct destination of the working rows."""
    d = mix.dst[mix.rows]
    for x in np.unique(d):
        yield int(x), np.nonzero(d == x)[0]


def test_restatements_are_linear_over_repeated_rows():
    csr, comp, par, dist = tables()
    m = OG.row_mix(csr, comp, N, 15, OG.strides_for(CUS, N))
    zero = np.zeros(1, np.int64)
    # integer: exact
    whole = EN.link_loads_host(csr, par[m.dst], EN.INT32, m.rows, m.ends, m.w)
    parts = np.zeros(csr.E, np.uint64)
    for x, idx in by_destination(m):
        parts += EN.link_loads_host(csr, par[x:x + 1], EN.INT32, np.repeat(zero, idx.size),
                                    m.ends[idx], m.w[idx])
    assert whole.any() and np.array_equal(whole, parts)
    # float: within RTOL, zeros exact
    cost = random_costs(csr, 1, 5, 16)
    pcost = pcost_rows(csr, cost, np.arange(csr.V))
    for split in SPLITS:
        whole = EN.ecmp_link_loads_host(csr, dist[m.dst], m.rows, m.ends, m.w, split)
        parts = np.zeros(csr.E)
        for x, idx in by_destination(m):
            parts += EN.ecmp_link_loads_host(csr, dist[x:x + 1], np.repeat(zero, idx.size),
                                             m.ends[idx], m.w[idx], split)
        assert whole.any() and close(whole, parts)
        whole = EN.cost_ecmp_link_loads_host(csr, cost, pcost[m.dst], m.rows, m.ends, m.w, split)
        parts = np.zeros(csr.E)
        for x, idx in by_destination(m):
            parts += EN.cost_ecmp_link_loads_host(csr, cost, pcost[x:x + 1],
                                                  np.repeat(zero, idx.size), m.ends[idx],
                                                  m.w[idx], split)
        assert whole.any() and close(whole, parts)


def test_failure_restatement_is_linear_and_the_cut_rows_lose_everything():
    csr, comp, _, _ = tables()
    n = N // 4
    m = OG.row_mix(csr, comp, n, 17, OG.strides_for(CUS // 4, n), bad_dst=True)
    victim = int(np.bincount(m.dst[m.kind == OG.WORK]).argmax())
    scen = OG.failure_scenarios(csr, victim)
    load, lost, routed = EN.failure_ecmp_link_loads_host(csr, None, m.dst, m.rows, m.ends, m.w,
                                                         scen)
    assert load.shape == (4, csr.E) and routed.shape == (4, m.rows.shape[0])
    for k, failed in enumerate(scen):
        assert not load[k][failed].any()
    parts = np.zeros_like(load)
    gone = np.zeros(4)
    for x, idx in by_destination(m):
        a, b, c = EN.failure_ecmp_link_loads_host(csr, None, [x], np.zeros(idx.size, np.int64),
                                                  m.ends[idx], m.w[idx], scen)
        parts += a
        gone += b
        assert np.array_equal(routed[:, idx], c)
    for k in range(4):
        assert close(load[k], parts[k])
    assert np.array_equal(lost, gone)                      # sums of integers below 2^53
    # toward the victim only the pairs s == d stay routed in the cut scenario
    to_victim = m.dst[m.rows] == victim
    assert to_victim.sum() > 3
    assert np.array_equal(routed[3][to_victim], m.ends[to_victim] == victim)
    assert routed[0][to_victim].sum() > routed[3][to_victim].sum()
    # a row whose destination is no vertex routes nothing
    assert not routed[:, m.kind[m.rows] == OG.BAD_DST].any()
