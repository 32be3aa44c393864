"""The conditions that keep the id-width GPU tests (test_id_width_gpu.py,
test_id_width_dropin_gpu.py) from passing vacuously, from the oracle alone, for
every fabric and size those tests use."""
import numpy as np
import pytest

import boundary_graphs as B
from oracle import oracle as O
from sdnmpi_amd import engine as EN

RING_SIZES = B.SIZES16 + B.SIZES17
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def drop_fabrics():
    yield
    B.clear()


def test_probe_ids():
    assert B.probe_ids(65535) == [0, 7, 32767, 32768, 65532, 65533, 65534]
    assert B.probe_ids(65537) == [0, 7, 32767, 32768, 65532, 65533, 65534, 65535, 65536]
    assert B.probe_ids(131072) == [0, 7, 32767, 32768, 65532, 65533, 65534, 65535, 65536,
                                   131069, 131070, 131071]
    for V in RING_SIZES:
        ids = B.probe_ids(V)
        assert len(ids) <= 16 and len(set(ids)) == len(ids) and max(ids) == V - 1
        assert {V - 3, V - 2, V - 1} <= set(ids)


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("V", RING_SIZES)
def test_ring_shape_and_ports(V, small):
    csr = B.ring(V, small)
    rp, col, port = csr.row_ptr, csr.col, csr.port
    assert csr.V == V and (csr.dpids == np.arange(1, V + 1, dtype=np.uint64)).all()
    deg = np.diff(rp)
    assert deg.max() == 6 and deg[B.isolated(V)] == 0 and deg[B.ONE_WAY] == 0
    assert not (col == B.isolated(V)).any() and (col == B.ONE_WAY).sum() == 6
    src = np.repeat(np.arange(V), deg)
    # a vertex's own out-links carry distinct ports
    key = src.astype(np.int64) << 32 | port.astype(np.int64)
    assert np.unique(key).size == key.size
    if small:
        assert port.min() == 1 and port.max() == 6
        assert EN.tree_layout(csr) == (EN.PORT16 if V <= 0xFFFF else EN.SLOT)
        return
    assert port.min() == 0 and port.max() == 0xFFFE
    assert {0, 0x7FFF, 0x8000, 0xFFFE} <= set(port.tolist())
    assert 0xFFFE in port[rp[V - 1]:rp[V]].tolist()
    e = rp[V - 2] + int(np.nonzero(col[rp[V - 2]:rp[V - 1]] == V - 1)[0][0])
    assert port[e] == 0xFFFE
    f = B.ring_fabric(V)
    hv, hp = f.host_table()
    assert hv.tolist() == B.probe_ids(V) and hp.max() >= 0x8000
    assert (f.host_dpid == hv + 1).all()


def roundtrip(csr, parent, port):
    layouts = [EN.SLOT]
    if EN.tree_layout(csr) == EN.PORT16:
        layouts.append(EN.PORT16)
    rp = csr.row_ptr.astype(np.int64)
    for lay in layouts:
        w = EN.pack_host_tree(parent, port, csr, lay)
        p = EN.tree_parent(w, lay)
        assert np.array_equal(p, parent), lay
        assert np.array_equal(EN.tree_port(w, lay, rp, csr.port, p), port), lay
    return layouts


@pytest.mark.parametrize("V", RING_SIZES)
def test_ring_trees_are_not_vacuous(V):
    csr = B.ring(V)
    ids = np.array(B.probe_ids(V), np.int32)
    iso = B.isolated(V)
    parent, port, hops = O.dfs_tables(csr, ids)
    vid = np.arange(V)
    for r, s in enumerate(ids.tolist()):
        reached = int((parent[r] >= 0).sum())
        if s in (iso, B.ONE_WAY):
            assert reached == 1 and parent[r, s] == s
        else:
            assert reached == V - 1 and parent[r, iso] == -1, s
    depth = int(hops.max())
    assert 1000 < depth <= 65534
    as_parent = set(np.unique(parent[parent != vid[None, :]]).tolist())
    dist, nh, nhp = O.dest_tables(csr, ids)
    assert int(dist[dist != 0xFFFF].max()) <= 255       # the bit-plane BFS holds 255 levels
    as_hop = set(np.unique(nh).tolist())
    for x in ids.tolist() + [V - 1, V - 2] + ([65535] if V > 65535 else []):
        if x not in (iso, B.ONE_WAY):
            assert x in as_parent, x
        if x != iso:
            assert x in as_hop, x
    for r, d in enumerate(ids.tolist()):
        reach = int((dist[r] != 0xFFFF).sum())
        # vertex 7 has no way out: it reaches itself alone
        assert reach == (1 if d == iso else V - 1 if d == B.ONE_WAY else V - 2), d
    layouts = roundtrip(csr, parent, port)
    assert layouts == ([EN.SLOT, EN.PORT16] if V <= 0xFFFF else [EN.SLOT])
    if V == 65535:                                       # root 65,534: one below the sentinel
        r = ids.tolist().index(65534)
        w = EN.pack_host_tree(parent[r:r + 1], port[r:r + 1], csr, EN.PORT16).view(np.uint32)
        assert w[0, 65534] == 0xFFFFFFFE and (w[0, iso] == NONE)


@pytest.mark.parametrize("V", [65535, 65536])
def test_jelly_trees_are_not_vacuous(V):
    csr = B.jelly(V)
    deg = np.diff(csr.row_ptr)
    assert 9 <= deg.max() <= 16 and deg.min() >= 1
    ids = np.array(B.probe_ids(V), np.int32)
    parent, port, hops = O.dfs_tables(csr, ids)
    assert ((parent >= 0).sum(1) == V).all() and int(hops.max()) <= 65534
    as_parent = set(np.unique(parent[parent != np.arange(V)[None, :]]).tolist())
    assert set(ids.tolist()) <= as_parent
    roundtrip(csr, parent, port)


def test_chain_is_as_deep_as_u16_holds():
    V = 65535
    csr = B.chain(V)
    parent, port, hops = O.dfs_tables(csr, np.array([0, V - 1], np.int32))
    assert hops[0, V - 1] == 0xFFFE and hops[1, 0] == 0xFFFE and (parent >= 0).all()
    assert (port[0, 1:] == 0xFFFE).all() and (port[1, :-1] == 1).all()
    roundtrip(csr, parent, port)
    dist = O.dest_tables(csr, np.array([0], np.int32))[0]
    assert dist[0, V - 1] == 0xFFFE and (dist[0] == np.arange(V)).all()


def test_twins_at_the_top_ids():
    V = 65535
    csr = B.with_twins(B.ring(V), V - 1, V - 2)
    rp, col = csr.row_ptr, csr.col
    a, b = col[rp[V - 1]:rp[V]], col[rp[V - 2]:rp[V - 1]]
    assert a.size >= 4 and np.array_equal(a, b) and V - 2 not in a and V - 1 not in a
    rrow, rcol = O.reverse_csr(csr)
    assert np.array_equal(rcol[rrow[V - 1]:rrow[V]], rcol[rrow[V - 2]:rrow[V - 1]])
    src = np.repeat(np.arange(V), np.diff(rp))
    key = src.astype(np.int64) << 32 | csr.port.astype(np.int64)
    assert np.unique(key).size == key.size
    assert EN.tree_layout(csr) == EN.PORT16
