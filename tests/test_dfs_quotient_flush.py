"""The quotient's flush (csrc/dfs.hip), restated in Python: the
expansion of test_dfs_quotient.py's class records through the tables the upload
builds (csrc/capi.hip, q_loff / q_slot / q_port) -- a tree link's port is the
composed table's entry at (quotient link, rank of the child in its class), and
for a child of the root the slot at that index, looked up in the root's own port
row.  Compared with the oracle for every root.  No GPU: the upload's loop and
the kernel's flush have this statement to be read against."""
import numpy as np
import pytest

from oracle import oracle as O

from test_dfs_quotient import GRAPHS, Quotient


class Composed(Quotient):
    """Quotient, with the upload's tables: rank[v] = v's position among its
    class's members (ascending); loff[c][j] = where the links of cmax[c] into
    the j-th class of c's quotient row start; slot / port at loff + rank = the
    slot in cmax[c]'s row, and the port, of the link to the member of that
    rank."""

    def __init__(self, csr):
        super().__init__(csr)
        V = csr.V
        seen = [0] * len(self.cmax)
        self.rank = [0] * V
        for v in range(V):
            self.rank[v] = seen[self.cid[v]]
            seen[self.cid[v]] += 1
        assert seen == self.size
        self.loff, self.slot, self.port = [], [], []
        for c, P in enumerate(self.cmax):
            row = self.rows[c]
            offs = []
            for d in row:
                offs.append(len(self.slot))
                self.slot += [None] * self.size[d]
                self.port += [None] * self.size[d]
            for e in range(csr.row_ptr[P], csr.row_ptr[P + 1]):
                x = int(csr.col[e])
                at = offs[row.index(self.cid[x])] + self.rank[x]
                assert self.slot[at] is None
                self.slot[at] = e - int(csr.row_ptr[P])
                self.port[at] = int(csr.port[e])
            self.loff.append(offs)
        assert None not in self.slot and None not in self.port

    def tables(self, s, seen=None):
        """(parent, port, hops) of root s: the quotient search keeps, per pushed
        class, the pusher, the slot of the link in the pusher's quotient row --
        from which the offset follows at the push -- and the depth."""
        csr, V = self.csr, self.csr.V
        C = self.cid[s]
        visited = set()
        if self.size[C] == 1:
            visited.add(C)
        rec, depth, stack = {}, {C: 0}, [C]
        while stack:
            u = stack.pop()
            for j, d in enumerate(self.rows[u]):
                if d not in visited:
                    visited.add(d)
                    rec[d] = (u, self.loff[u][j], depth[u] + 1)
                    depth[d] = depth[u] + 1
                    stack.append(d)
        own = [int(x) for x in csr.port[csr.row_ptr[s]:csr.row_ptr[s + 1]]]
        parent = np.full(V, -1, np.int32)
        port = np.full(V, -1, np.int32)
        hops = np.full(V, -1, np.int32)
        for v in range(V):
            if v == s:
                parent[v], hops[v] = s, 0
            elif self.cid[v] in rec:
                pc, off, d = rec[self.cid[v]]
                at = off + self.rank[v]
                if pc == C:                      # a child of the root: the root's own row
                    parent[v], port[v] = s, own[self.slot[at]]
                    if seen is not None:
                        seen["root_child"] += 1
                        seen["root_child_other_port"] += s != self.cmax[C] and \
                            own[self.slot[at]] != self.port[at]
                else:
                    parent[v], port[v] = self.cmax[pc], self.port[at]
                hops[v] = d
                if seen is not None:
                    seen["member_of_rank_above_0"] += self.rank[v] > 0
        return parent, port, hops


def test_composed_table_is_the_slot_table_through_the_port_row():
    """q_port[i] = port row of cmax[c] at q_slot[i], link by link."""
    for name, csr in GRAPHS:
        q = Composed(csr)
        for c, P in enumerate(q.cmax):
            own = csr.port[csr.row_ptr[P]:csr.row_ptr[P + 1]]
            for j, d in enumerate(q.rows[c]):
                for r in range(q.size[d]):
                    at = q.loff[c][j] + r
                    assert q.port[at] == int(own[q.slot[at]]), (name, c, j, r)
                    x = int(csr.col[csr.row_ptr[P] + q.slot[at]])
                    assert q.cid[x] == d and q.rank[x] == r, (name, c, j, r)


SEEN = dict.fromkeys(["root_child", "root_child_other_port", "member_of_rank_above_0"], 0)


@pytest.mark.parametrize("name,csr", GRAPHS, ids=[n for n, _ in GRAPHS])
def test_composed_expansion_is_the_reference_search(name, csr):
    V = csr.V
    po, to, ho = O.dfs_tables(csr, np.arange(V, dtype=np.int32), with_hops=True)
    q = Composed(csr)
    for s in range(V):
        p, t, h = q.tables(s, SEEN)
        np.testing.assert_array_equal(p, po[s], err_msg="parent, root %d" % s)
        np.testing.assert_array_equal(t, to[s], err_msg="port, root %d" % s)
        np.testing.assert_array_equal(h, ho[s], err_msg="hops, root %d" % s)


def test_the_graphs_hold_every_case():
    """After the parity cases above (the file's order): they met root children
    whose port from the root differs from the port from the class's largest
    member, and members of every rank."""
    if not SEEN["root_child"]:
        for name, csr in GRAPHS:
            q = Composed(csr)
            for s in range(csr.V):
                q.tables(s, SEEN)
    assert all(n > 0 for n in SEEN.values()), SEEN
