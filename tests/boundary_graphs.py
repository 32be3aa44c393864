"""Fabrics whose vertex count sits on an id-width bound of the library (16-bit
ids up to 65,535, 17-bit rows up to 131,071), for test_boundary_graphs.py and
the test_id_width_*_gpu.py modules.  A plain helper module like golden_util.

Dense vertex v has dpid v + 1 everywhere, so dense ids and CSR order agree.

ring(V)   the circulant u <-> u +- 1, u +- 41, u +- 1693 (mod V): degree 6 (rows
          of <= 8 slots, few distinct offset tuples: the dictionary rows apply
          up to 65,535).  Three edits: vertex V - 3 loses every link (isolated),
          vertex 7 loses its out-links (one-way: the in-rows differ from the
          out-rows), and the ports are spread over 0 .. 0xFFFE.
jelly(V)  topologies.jellyfish(V, 12): rows of 12 slots, no dictionary.
chain(V)  the path 0 - 1 - ... - V - 1, port 0xFFFE forward and 1 backward.
"""
import numpy as np

from sdnmpi_amd import topologies as T

SIZES16 = (65533, 65534, 65535, 65536, 65537)
SIZES17 = (131070, 131071, 131072)
OFFSETS = (1, -1, 41, -41, 1693, -1693)
ONE_WAY = 7                       # no out-links
HOST_PORT_HIGH = 0x9000           # the first host's port: negative as int16

_cache = {}


def probe_ids(V):
    """The ids next to every width bound and sentinel, below V, in this order,
    each once."""
    want = [0, 7, 32767, 32768] + list(range(65532, 65537)) + list(range(131069, 131072)) + \
        [V - 3, V - 2, V - 1]
    out = []
    for x in want:
        if 0 <= x < V and x not in out:
            out.append(x)
    return out


def isolated(V):
    return V - 3


def _ring_links(V, small_ports):
    """(src, dst, sport, dport) dense ids of every directed ring link after the
    edits, in creation order."""
    u = np.repeat(np.arange(V, dtype=np.int64), len(OFFSETS))
    k = np.tile(np.arange(len(OFFSETS), dtype=np.int64), V)
    v = (u + np.asarray(OFFSETS, np.int64)[k]) % V
    kb = k ^ 1                                   # the slot of the link back: the offset negated

    def ports(x, kk, y):
        if small_ports:
            return kk + 1                        # 1 .. 6
        p = (7 * x + kk) % 0xFFFF                # 0 .. 0xFFFE, six distinct ones per vertex
        p = np.where((x == 32768) & (kk == 0), 0x7FFF, p)
        p = np.where((x == 32768) & (kk == 1), 0x8000, p)
        p = np.where((x == V - 1) & (kk == 0), 0xFFFE, p)           # V - 1 -> 0
        p = np.where((x == V - 2) & (y == V - 1), 0xFFFE, p)
        return p

    sport, dport = ports(u, k, v), ports(v, kb, u)
    iso = isolated(V)
    keep = (u != iso) & (v != iso) & (u != ONE_WAY)
    return u[keep], v[keep], sport[keep], dport[keep]


def _hosts(V):
    ids = probe_ids(V)
    macs = [T.HOST_MAC_BASE + i for i in range(len(ids))]
    hp = [HOST_PORT_HIGH if i == 0 else 200 + i for i in range(len(ids))]
    return macs, [x + 1 for x in ids], hp


def _fabric(name, V, src, sport, dst, dport):
    macs, hd, hp = _hosts(V)
    return T.Fabric(name, src + 1, sport, dst + 1, dport, macs, hd, hp, range(1, V + 1), {"V": V})


def ring_fabric(V, small_ports=False):
    key = ("ring", V, small_ports)
    if key not in _cache:
        u, v, sp, dp = _ring_links(V, small_ports)
        _cache[key] = _fabric("ring_%d%s" % (V, "_small" if small_ports else ""), V, u, sp, v, dp)
    return _cache[key]


def ring(V, small_ports=False):
    """CSR of the edited circulant; small_ports: every port in 1 .. 6."""
    return ring_fabric(V, small_ports).csr()


def jelly_fabric(V):
    key = ("jelly", V)
    if key not in _cache:
        f = T.jellyfish(V, 12)
        _cache[key] = _fabric("jelly_%d" % V, V, f.link_src - 1, f.link_sport, f.link_dst - 1,
                              f.link_dport)
    return _cache[key]


def jelly(V):
    return jelly_fabric(V).csr()


def chain(V):
    key = ("chain", V)
    if key not in _cache:
        a = np.arange(V - 1, dtype=np.int64)
        src = np.concatenate([a, a + 1]) + 1
        dst = np.concatenate([a + 1, a]) + 1
        port = np.concatenate([np.full(V - 1, 0xFFFE), np.full(V - 1, 1)])
        _cache[key] = T.build_csr(src, dst, port, extra_vertices=range(1, V + 1))
    return _cache[key]


def with_twins(csr, a, b):
    """The CSR with b's links replaced by a's: the same out- and in-row, the
    two not linked to each other (every neighbour of a gains the link to and
    from b on the port of its link to a; b's ports are a's)."""
    rp, col, port = csr.row_ptr, csr.col, csr.port
    V = csr.V
    src = np.repeat(np.arange(V, dtype=np.int64), np.diff(rp))
    keep = (src != b) & (col != b) & ~((src == a) & (col == b)) & ~((src == b) & (col == a))
    s, d, p = src[keep], col[keep].astype(np.int64), port[keep].astype(np.int64)
    out_a, in_a = s == a, d == a
    s = np.concatenate([s, np.full(int(out_a.sum()), b), s[in_a]])
    d = np.concatenate([d, d[out_a], np.full(int(in_a.sum()), b)])
    p = np.concatenate([p, p[out_a], (p[in_a] + 0x4000) % 0xFFFF])
    return T.build_csr(s + 1, d + 1, p, extra_vertices=range(1, V + 1))


def clear():
    _cache.clear()
