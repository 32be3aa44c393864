"""The twin-class quotient search (csrc/dfs.hip), restated in
Python and compared with the oracle for every root: the search runs over the
twin classes, numbered by ascending largest member, and the records of the
classes are expanded to the vertices afterwards.  No GPU: this is the fact the
kernel builds on, checked on its own."""
import numpy as np
import pytest

from oracle import oracle as O
from sdnmpi_amd import topologies as T

import golden_util as G


def rows_of(csr):
    V = csr.V
    out = [tuple(int(x) for x in csr.col[csr.row_ptr[u]:csr.row_ptr[u + 1]]) for u in range(V)]
    ins = [[] for _ in range(V)]
    for u in range(V):
        for v in out[u]:
            ins[v].append(u)
    return out, [tuple(r) for r in ins]


def twin_reps_py(csr):
    """rep[v] = smallest vertex with v's out-row and in-row; a vertex whose row
    holds a self-loop stays alone."""
    out, ins = rows_of(csr)
    seen, rep = {}, list(range(csr.V))
    for v in range(csr.V):
        if v in out[v]:
            continue
        rep[v] = seen.setdefault((out[v], ins[v]), v)
    return rep


class Quotient(object):
    """Classes numbered by ascending largest member; the out-row of a class is
    the sorted set of the classes of its members' common out-row."""

    def __init__(self, csr):
        self.csr = csr
        V = csr.V
        self.out, self.ins = rows_of(csr)
        rep = twin_reps_py(csr)
        largest = {}
        for v in range(V):
            largest[rep[v]] = v
        order = sorted(largest, key=lambda r: largest[r])
        num = {r: i for i, r in enumerate(order)}
        self.cid = [num[rep[v]] for v in range(V)]
        self.cmax = [largest[r] for r in order]
        self.size = [0] * len(order)
        for v in range(V):
            self.size[self.cid[v]] += 1
        self.rows = [sorted({self.cid[x] for x in self.out[m]}) for m in self.cmax]
        self.port_of = {}
        for u in range(V):
            for e in range(csr.row_ptr[u], csr.row_ptr[u + 1]):
                self.port_of[(u, int(csr.col[e]))] = int(csr.port[e])

    def tables(self, s):
        """(parent, port, hops) of root s by the quotient search."""
        V = self.csr.V
        C = self.cid[s]
        visited = set()
        if self.size[C] == 1:
            visited.add(C)                       # a class of several members is not marked
        rec, depth, stack = {}, {C: 0}, [C]
        while stack:
            u = stack.pop()
            for d in self.rows[u]:
                if d not in visited:
                    visited.add(d)
                    rec[d] = (u, depth[u] + 1)
                    depth[d] = depth[u] + 1
                    stack.append(d)
        parent = np.full(V, -1, np.int32)
        port = np.full(V, -1, np.int32)
        hops = np.full(V, -1, np.int32)
        for v in range(V):
            if v == s:
                parent[v], hops[v] = s, 0
            elif self.cid[v] in rec:
                pc, d = rec[self.cid[v]]
                p = s if pc == C else self.cmax[pc]
                parent[v], port[v], hops[v] = p, self.port_of[(p, v)], d
        return parent, port, hops


def csr_of(adj, rng):
    V = adj.shape[0]
    rows, cols = np.nonzero(adj)
    row_ptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=V), out=row_ptr[1:])
    return T.CSR(np.arange(1, V + 1), row_ptr, cols, rng.integers(0, 60000, size=cols.size))


def planted(seed):
    """A random directed graph of 4-14 vertices (one-way links, self-loops) in
    which a and b are twins; every fourth one gives the pair no in-links, every
    fifth one plants a third twin."""
    rng = np.random.default_rng(1000 + seed)
    V = int(rng.integers(4, 15))
    adj = rng.random((V, V)) < rng.uniform(0.1, 0.5)
    group = [int(x) for x in rng.choice(V, 3 if seed % 5 == 0 else 2, replace=False)]
    a = group[0]
    for b in group[1:]:
        adj[b, :] = adj[a, :]
        adj[:, b] = adj[:, a]
    if seed % 4 == 0:
        adj[:, group] = False
    for x in group:
        for y in group:
            adj[x, y] = False
    return csr_of(adj, rng)


def special():
    """Hand-made graphs for the cases a random draw may miss."""
    rng = np.random.default_rng(7)
    out = {}
    # 0 and 1 share the out-row {2, 3}; 4 links to 0 only: no twins
    adj = np.zeros((5, 5), bool)
    adj[0, [2, 3]] = adj[1, [2, 3]] = True
    adj[4, 0] = adj[2, 4] = True
    out["same_out_row_other_in_row"] = csr_of(adj, rng)
    # 1 and 2 are twins but for 2's self-loop
    adj = np.zeros((6, 6), bool)
    adj[1, [3, 4]] = adj[2, [3, 4]] = True
    adj[0, [1, 2]] = adj[5, [1, 2]] = True
    adj[3, 0] = adj[4, 5] = True
    adj[2, 2] = True
    out["self_loop_twin"] = csr_of(adj, rng)
    # 70 twins under one hub, all linking on to 71 and 72; 73 .. 75 a class no
    # root but its own reaches; 76 .. 78 twins nobody links to
    V = 79
    adj = np.zeros((V, V), bool)
    adj[0, 1:71] = True
    adj[1:71, 71] = adj[1:71, 72] = True
    adj[71, 0] = True
    adj[73:76, 0] = True
    adj[76:79, 71] = True
    out["class_of_70"] = csr_of(adj, rng)
    return out


def graphs():
    out = []
    for name in ("fat_tree:4", "fat_tree:8"):
        out.append((name, T.by_name(name).csr()))
    for name in G.SMALL:
        out.append((name, G.Golden(name).fabric().csr()))
    out += sorted(special().items())
    out += [("planted%d" % seed, planted(seed)) for seed in range(200)]
    return out


GRAPHS = graphs()


def test_the_graphs_hold_every_case():
    """By assertion, so that a change of the generators cannot make the parity
    test below vacuous."""
    seen = dict.fromkeys(["root_in_class", "root_is_largest", "root_not_largest",
                          "mates_unreachable", "class_never_reached", "same_out_other_in",
                          "self_loop_equal_row", "class_over_64", "loops_fixture"], 0)
    for name, csr in GRAPHS:
        q = Quotient(csr)
        V = csr.V
        seen["loops_fixture"] += name.endswith("_loops")
        seen["class_over_64"] += max(q.size) > 64
        for a in range(V):
            for b in range(a + 1, V):
                if q.cid[a] == q.cid[b]:
                    continue
                la, lb = a in q.out[a], b in q.out[b]
                if q.out[a] == q.out[b] and q.ins[a] != q.ins[b] and not la and q.out[a]:
                    seen["same_out_other_in"] += 1
                if la != lb:
                    strip = lambda r: tuple(x for x in r if x not in (a, b))  # noqa: E731
                    if strip(q.out[a]) == strip(q.out[b]) and strip(q.ins[a]) == strip(q.ins[b]) \
                            and strip(q.out[a]):
                        seen["self_loop_equal_row"] += 1
        multi = [c for c in range(len(q.size)) if q.size[c] > 1]
        if not multi or V > 100:
            continue
        po, _, _ = O.dfs_tables(csr, np.arange(V, dtype=np.int32), with_hops=True)
        for s in range(V):
            C = q.cid[s]
            reached = po[s] >= 0
            if q.size[C] > 1:
                seen["root_in_class"] += 1
                seen["root_is_largest" if q.cmax[C] == s else "root_not_largest"] += 1
                mates = [v for v in range(V) if q.cid[v] == C and v != s]
                seen["mates_unreachable"] += not reached[mates].any()
            for c in multi:
                if c != C and not reached[[v for v in range(V) if q.cid[v] == c]].any():
                    seen["class_never_reached"] += 1
    assert all(n > 0 for n in seen.values()), seen


@pytest.mark.parametrize("name,csr", GRAPHS, ids=[n for n, _ in GRAPHS])
def test_quotient_search_is_the_reference_search(name, csr):
    V = csr.V
    po, to, ho = O.dfs_tables(csr, np.arange(V, dtype=np.int32), with_hops=True)
    q = Quotient(csr)
    assert q.cmax == sorted(q.cmax)
    for s in range(V):
        p, t, h = q.tables(s)
        np.testing.assert_array_equal(p, po[s], err_msg="parent, root %d" % s)
        np.testing.assert_array_equal(t, to[s], err_msg="port, root %d" % s)
        np.testing.assert_array_equal(h, ho[s], err_msg="hops, root %d" % s)
