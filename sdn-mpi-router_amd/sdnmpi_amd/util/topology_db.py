"""Drop-in ``TopologyDB`` whose routes come from the MI355X route engine.

Mirrors ``sdnmpi/util/topology_db.py`` of keichi/sdn-mpi-router: the same
attributes (``switches``, ``links``, ``hosts`` dicts), mutators
(``add_host``/``add_switch``/``delete_switch``/``add_link``/``delete_link``,
:20-42), ``to_dict`` (:44-57) and ``find_route(src_mac, dst_mac,
multiple=False)`` (:140-188) with the same return values and error
behaviour: a list of ``(dpid, out_port)`` tuples, ``[]`` for unknown hosts
or unreachable destinations, ``ValueError`` for a MAC that is not hex.

What changes is how a route is found.  Instead of one Python stack search
per (src, dst) pair, the switch graph is exported as a CSR and the GPU
computes whole tables -- per source the tree of the reference's LIFO
traversal (every destination at once), per destination the hop distances
of the shortest-route mode -- which are cached and walked per query.  A
topology event patches the export (one CSR row per link event, nothing for a
host on a known switch) and drops only the cached rows it can alter.
``route_tables()`` / ``find_routes()`` expose the batched all-pairs form the
MPI router needs.

There is no CPU fallback: without ``libsdnroute.so`` or a gfx950 device the
first route query raises (``sdnmpi_amd._native.NativeUnavailable`` /
``SdnrError``), and so does the first flood-port query (``is_edge_port`` /
``edge_ports`` / ``broadcast_ports``: their bulk pass is sdnr_edge_ports).
"""

import numpy as np

from ..engine import (COST_INF, COST_MAX, DEFAULT_TABLE_BUDGET, FAIR_MULT_LIMIT, INT32, LFA_MAX_V, UTIL_MAX, RouteEngine, TableCache, _gather,
                      _edge_keys_host, _host, _take, _torch, _u16, check_link_costs,
                      least_cost_paths_lex,
                      peak_utilisation,
                      shortest_paths_lex, tree_path)
from ..graph import TrackedDict, Versions, export_graph, update_export
from ..incremental import edge_diff

try:   # the reference takes OFPP_LOCAL from Ryu's OpenFlow 1.0 module (:5)
    from ryu.ofproto.ofproto_v1_0 import OFPP_LOCAL
except Exception:   # noqa: BLE001 - Ryu is not a dependency of the engine
    OFPP_LOCAL = 0xfffe

__all__ = ["TopologyDB", "LinkLoads", "SplitLinkLoads", "FailureLoads", "CostChangeLoads", "FrrLoads",
           "CostTuning", "Admission", "FairRates", "MulticastTree", "OFPP_LOCAL",
           "sdn_mpi_mac"]

_INF = 0xFFFF
_U64 = (1 << 64) - 1
TABLE_SLICE_ENTRIES = 1 << 24     # table entries decoded per slice by route_tables()


class LinkLoads(object):
    """Predicted traffic per link (:meth:`TopologyDB.link_loads`).

    One record per link of the switch graph, in the CSR's order (ascending
    source dpid, then destination dpid), zeros included: ``src_dpid``,
    ``dst_dpid``, ``port`` (``links[src][dst].src.port_no``) and ``load``
    (uint64).  The last hops -- a route's entry on its destination switch,
    out of the host's port or ``OFPP_LOCAL`` -- are ``host_dpid``,
    ``host_port``, ``host_load``: the nonzero ones, ascending."""

    def __init__(self, dpids, esrc, edst, port, load, hsw, hport, hload):
        self._dpids = dpids
        self._esrc, self._hsw = esrc, np.asarray(hsw, np.int64)
        self.src_dpid = dpids[esrc]
        self.dst_dpid = dpids[edst]
        self.port = port
        self.load = load
        self.host_dpid = dpids[self._hsw]
        self.host_port = np.asarray(hport, np.int64)
        self.host_load = hload

    def as_dict(self):
        """{(dpid, out_port): load} of the nonzero entries, links and last
        hops alike: the weighted count of the ``(dpid, out_port)`` tuples
        ``find_route`` returns for the pairs."""
        out = {}
        nz = np.nonzero(self.load)[0]
        for d, p, x in zip(self.src_dpid[nz].tolist(), self.port[nz].tolist(),
                           self.load[nz].tolist()):
            out[(d, p)] = (out.get((d, p), 0) + x) & _U64
        for d, p, x in zip(self.host_dpid.tolist(), self.host_port.tolist(),
                           self.host_load.tolist()):
            out[(d, p)] = (out.get((d, p), 0) + x) & _U64
        return out

    def per_switch(self):
        """(dpids, total): every switch of the graph (ascending dpid) and the
        load leaving it, last hops included.  With unit weights and distinct
        pairs ``total`` is the number of flow entries the router would
        install on each switch."""
        total = np.zeros(self._dpids.shape[0], np.uint64)
        np.add.at(total, self._esrc, self.load)
        np.add.at(total, self._hsw, self.host_load)
        return self._dpids, total


class SplitLinkLoads(LinkLoads):
    """Predicted traffic per link under ECMP (:meth:`TopologyDB.
    ecmp_link_loads`): the records of :class:`LinkLoads` with a float64
    ``load`` -- a pair's traffic is split over its shortest routes, so a link
    carries fractions of weights.  ``host_load`` stays exact uint64: every
    route of a pair ends on the same last hop."""

    def as_dict(self):
        """{(dpid, out_port): float load} of the nonzero entries, links and
        last hops alike."""
        out = {}
        nz = np.nonzero(self.load)[0]
        for d, p, x in zip(self.src_dpid[nz].tolist(), self.port[nz].tolist(),
                           self.load[nz].tolist()):
            out[(d, p)] = out.get((d, p), 0.0) + x
        for d, p, x in zip(self.host_dpid.tolist(), self.host_port.tolist(),
                           self.host_load.tolist()):
            out[(d, p)] = out.get((d, p), 0.0) + float(x)
        return out

    def per_switch(self):
        """(dpids, total float64): every switch of the graph (ascending dpid)
        and the load leaving it, last hops included."""
        total = np.zeros(self._dpids.shape[0], np.float64)
        np.add.at(total, self._esrc, self.load)
        np.add.at(total, self._hsw, self.host_load.astype(np.float64))
        return self._dpids, total


class MulticastTree(object):
    """One group's multicast tree (:meth:`TopologyDB.multicast_tree`):
    ``entries`` -- the sorted set of ``(dpid, out_port)`` tuples of the routes
    from ``src`` to the members, each once --, ``unreached`` -- the member
    MACs without a route (unknown hosts included), in the caller's order."""

    def __init__(self, src, entries, unreached):
        self.src = src
        self.entries = entries
        self.unreached = unreached

    def as_dict(self):
        """{dpid: (out_port, ...)}: the output actions of the one flow entry
        each switch of the tree gets, ports ascending."""
        out = {}
        for d, p in self.entries:
            out.setdefault(d, []).append(p)
        return {d: tuple(ps) for d, ps in out.items()}


class _EntryLoads(LinkLoads):
    """:class:`LinkLoads` of multicast trees on a fabric that reuses a port
    number on one switch: ``entry_loads`` holds the load of every ``(dpid,
    out_port)`` entry, an entry that several links or last hops of a group
    share counted once for that group; ``load`` and ``host_load`` stay per
    link and per last hop."""

    entry_loads = None

    def as_dict(self):
        return dict(self.entry_loads)


class FailureLoads(object):
    """Predicted traffic per link under each of a list of link-failure
    scenarios (:meth:`TopologyDB.failure_link_loads`).

    ``scenarios``: the scenarios as they were applied -- per scenario the tuple
    of its directed links ``(src_dpid, dst_dpid)`` that exist, in the CSR's
    link order, each once.  ``load``: float64 [nscen, E], row k the link loads
    of scenario k in the order of :class:`LinkLoads`' records (a failed link
    holds exactly 0.0).  ``lost``: uint64 [nscen], the weight that has no route
    in scenario k, exact.  ``base``: the :class:`SplitLinkLoads` of the intact
    fabric."""

    def __init__(self, scenarios, load, lost, base, hkey, hload, result):
        self.scenarios = scenarios
        self.load = load
        self.lost = lost
        self.base = base
        self._hkey, self._hload, self._result = hkey, hload, result

    def __len__(self):
        return len(self.scenarios)

    def scenario(self, i):
        """The :class:`SplitLinkLoads` of scenario ``i``: its link loads, and
        the last hops of the pairs that still have a route."""
        if not 0 <= i < len(self.scenarios):
            raise IndexError("no scenario %r" % (i,))
        return self._result(self.load[i], self._hkey, self._hload[i])

    def worst(self):
        """(load float64 [E], scenario int64 [E]): per link the largest load
        over the scenarios and the first scenario that attains it (0.0 and -1
        without scenarios)."""
        if not len(self.scenarios):
            E = self.load.shape[1]
            return np.zeros(E, np.float64), np.full(E, -1, np.int64)
        return self.load.max(0), self.load.argmax(0).astype(np.int64)

    def worst_dict(self):
        """{(dpid, out_port): (load, scenario index)} of :meth:`worst` over the
        links whose largest load is nonzero."""
        top, at = self.worst()
        nz = np.nonzero(top)[0]
        return {(d, p): (x, k) for d, p, x, k in
                zip(self.base.src_dpid[nz].tolist(), self.base.port[nz].tolist(),
                    top[nz].tolist(), at[nz].tolist())}


class CostChangeLoads(FailureLoads):
    """Predicted traffic per link under each of a list of link-cost scenarios
    (:meth:`TopologyDB.cost_change_link_loads`): everything of
    :class:`FailureLoads`, with ``scenarios`` holding per scenario the tuple
    of its changes ``((src_dpid, dst_dpid), cost)`` that name existing links,
    in the CSR's link order (``cost`` None: the link is down).

    ``peak``: float64 [nscen], the largest utilisation ``load / capacity`` over
    the switch links (last hops are not links of the fabric) in scenario k;
    ``peak_link``: the first ``(src_dpid, dst_dpid)`` in link order that
    attains it, None where nothing is carried; ``base_peak``: the peak of the
    intact fabric."""

    def __init__(self, scenarios, load, lost, base, hkey, hload, result, peak, peak_link,
                 base_peak):
        FailureLoads.__init__(self, scenarios, load, lost, base, hkey, hload, result)
        self.peak = peak
        self.peak_link = peak_link
        self.base_peak = base_peak


class FrrLoads(object):
    """Predicted traffic per link while fast reroute is forwarding, under each
    of a list of link-failure scenarios (:meth:`TopologyDB.frr_link_loads`).

    ``scenarios``: as in :class:`FailureLoads`.  ``load``: uint64 [nscen, E],
    row k the exact link loads of scenario k in the order of
    :class:`LinkLoads`' records, None when the planes were not asked for.  Per
    scenario, uint64 [nscen]: ``repaired`` -- the weight delivered through at
    least one backup next hop --, ``dropped`` -- the weight that reached a
    switch whose primary link is down and that has no usable backup --,
    ``looped`` -- the weight the backups forward in a circle --, ``unrouted``
    -- the weight without a route on the intact fabric; ``peak`` -- the largest
    link load -- and ``peak_link``, the first ``(src_dpid, dst_dpid)`` in link
    order that attains it, None where nothing is carried.  ``base``: the
    :class:`LinkLoads` of the intact fabric
    (:meth:`TopologyDB.least_cost_link_loads`).  ``items``: the (scenario,
    destination switch) items the kernel had to recompute."""

    def __init__(self, scenarios, load, stat, peak, peak_link, base, hkey, hload, result, items):
        self.scenarios = scenarios
        self.load = load
        self.repaired, self.dropped = stat[:, 0].copy(), stat[:, 1].copy()
        self.looped, self.unrouted = stat[:, 2].copy(), stat[:, 3].copy()
        self.peak = peak
        self.peak_link = peak_link
        self.base = base
        self.items = items
        self._hkey, self._hload, self._result = hkey, hload, result

    def __len__(self):
        return len(self.scenarios)

    def scenario(self, i):
        """The :class:`LinkLoads` of scenario ``i``: its link loads, and the
        last hops of the pairs that are delivered."""
        if self.load is None:
            raise ValueError("the load planes were not kept (planes=False)")
        if not 0 <= i < len(self.scenarios):
            raise IndexError("no scenario %r" % (i,))
        return self._result(self.load[i], self._hkey, self._hload[i])


class CostTuning(object):
    """What :meth:`TopologyDB.tune_link_costs` found.  ``costs``: the changed
    costs ``{(src_dpid, dst_dpid): cost}``; ``peak_before`` / ``peak_after``:
    the peak utilisation under the costs in force and with ``costs`` on top of
    them; ``history``: per accepted step ``((src_dpid, dst_dpid), cost,
    peak)``."""

    def __init__(self, costs, peak_before, peak_after, history):
        self.costs = costs
        self.peak_before = peak_before
        self.peak_after = peak_after
        self.history = history


class Admission(object):
    """Result of :meth:`TopologyDB.admit_flows`: what the links carry once the
    flows were admitted in order, each slice on its least-loaded routes.

    ``loads``: :class:`LinkLoads` of the admitted traffic (exact uint64).
    ``peak_before`` / ``peak_link_before``: the largest per-link figure -- the
    load, or ``load * 1024 // capacity`` where capacities were given, a Python
    int -- and the first link ``(src_dpid, dst_dpid)`` that attains it (None
    on a fabric without links) when every pair takes the lexicographic
    least-cost route instead (:meth:`TopologyDB.least_cost_link_loads`);
    ``peak_after`` / ``peak_link_after``: the same of ``loads``.  ``lost``:
    the weight of the known pairs that have no route.  ``rounds``: the slices
    the pairs were admitted in.  ``routes``: with ``routes=True`` the fdb of
    every pair, in ``find_route``'s format ([] where there is none), else
    None."""

    def __init__(self, loads, peak_before, peak_link_before, peak_after, peak_link_after, lost,
                 rounds, routes):
        self.loads = loads
        self.peak_before, self.peak_link_before = peak_before, peak_link_before
        self.peak_after, self.peak_link_after = peak_after, peak_link_after
        self.lost = lost
        self.rounds = rounds
        self.routes = routes


CAPACITY_MAX = 1 << 53            # admit_flows: load * 1024 // capacity stays in 64 bits


class FairRates(object):
    """Predicted max-min fair throughput (:meth:`TopologyDB.fair_rates`).

    Per input pair, in the order given: ``pairs``, ``weights`` (uint64
    multiplicities), ``rate`` (float64: what ONE flow of the pair gets, in the
    capacities' unit; ``inf`` for a pair that crosses nothing modelled),
    ``routed`` (bool: unknown hosts and unreachable pairs are False and have
    rate 0.0), ``round`` (int32: the filling round that froze the pair, -1
    where none did) and ``bottleneck`` (the link that limits the pair as
    ``(src_dpid, dst_dpid)``, a host port as ``("host", mac)``, or None).
    ``levels`` are the rates of the rounds, ascending, ``rounds`` their number;
    ``link_rate`` is a :class:`SplitLinkLoads` of the rate every link carries
    (last hops: the rate out of every host port, when host ports are
    modelled).  An MPI result also has ``bytes`` and ``time`` per pair."""

    #: a link counts as saturated when its spare capacity is below this share
    SATURATED = 1e-9

    def __init__(self, pairs, weights, rate, routed, rnd, bottleneck, levels, link_rate, cap,
                 used, names):
        self.pairs = pairs
        self.weights = weights
        self.rate = rate
        self.routed = routed
        self.round = rnd
        self.bottleneck = bottleneck
        self.levels = levels
        self.rounds = int(levels.shape[0])
        self.link_rate = link_rate
        self._cap, self._used, self._names = cap, used, names
        self.bytes = None
        self.time = None

    def saturated_links(self):
        """The links, as ``(src_dpid, dst_dpid)``, and host ports, as
        ``("host", mac)``, that are full: spare capacity below ``SATURATED``
        (1e-9) of the capacity, the rounding of the rounds' sums allowed for."""
        full = np.nonzero(self._cap - self._used <= self.SATURATED * self._cap)[0]
        out = []
        for e in full.tolist():
            x = self._names(e)
            if x not in out:
                out.append(x)
        return out

    @property
    def min_rate(self):
        """The smallest rate of a routed pair of nonzero weight (``levels[0]``
        when a round ran; ``inf`` when nothing is constrained; None without
        such a pair)."""
        ok = self.routed & (self.weights != 0)
        return float(self.rate[ok].min()) if ok.any() else None

    def slowest(self):
        """The pairs frozen in round 0: those at ``levels[0]``, the job's
        slowest flows."""
        return [self.pairs[i] for i in np.nonzero(self.round == 0)[0].tolist()]

    @property
    def total(self):
        """Sum of rate * weight over the routed pairs of finite rate: the
        fabric's aggregate throughput under this traffic."""
        ok = self.routed & np.isfinite(self.rate)
        return float((self.rate[ok] * self.weights[ok].astype(np.float64)).sum())

    def step_time(self):
        """The largest ``time`` (MPI results): how long the exchange takes if
        every pair kept its rate throughout -- an upper estimate, since flows
        that finish early leave their share to the others.  ``inf`` when a
        pair with bytes to send is not routed; 0.0 without pairs."""
        if self.time is None:
            raise ValueError("step_time needs the bytes of mpi_fair_rates")
        return float(self.time.max()) if self.time.size else 0.0


class FlowTimes(object):
    """Predicted max-min fair completion times
    (:meth:`TopologyDB.fair_completion_times`).

    Per input pair, in the order given: ``pairs``, ``weights`` (uint64
    multiplicities), ``bytes`` (float64, per flow), ``time`` (float64: when
    each flow of the pair has sent its bytes; 0.0 for a routed pair without
    bytes or one that crosses nothing modelled, ``inf`` for an unrouted pair,
    one of weight 0 and one still sending when ``max_epochs`` ran out),
    ``epoch`` (int32: the epoch the pair left in; -1 where it never shared, -2
    still sending), ``routed`` (bool), ``rate0`` (float64: the pair's rate at
    t = 0, :meth:`TopologyDB.fair_rates`' ``rate``) and ``remaining`` (float64:
    bytes not sent yet).  ``epoch_time[j]`` is when epoch j ended and
    ``epoch_rounds[j]`` the rounds of its filling, ``epochs`` their number;
    ``link_bytes`` is a :class:`SplitLinkLoads` of the bytes every link
    carried (last hops: the bytes out of every host port, when host ports are
    modelled); ``complete`` says that no pair is still sending; ``split`` is
    how a multipath route divided a pair ("route" for the single-path routes)."""

    def __init__(self, pairs, weights, nbytes, time, epoch, routed, rate0, remaining, epoch_time,
                 epoch_rounds, link_bytes, split="route"):
        self.split = split
        self.pairs = pairs
        self.weights = weights
        self.bytes = nbytes
        self.time = time
        self.epoch = epoch
        self.routed = routed
        self.rate0 = rate0
        self.remaining = remaining
        self.epoch_time = epoch_time
        self.epoch_rounds = epoch_rounds
        self.epochs = int(epoch_time.shape[0])
        self.link_bytes = link_bytes
        self.complete = not bool((epoch == -2).any())

    def makespan(self):
        """How long the exchange takes: the largest finite ``time`` (0.0
        without one), or ``inf`` if a pair of nonzero weight with bytes to
        send has no route."""
        if bool((~self.routed & (self.bytes > 0) & (self.weights != 0)).any()):
            return float("inf")
        t = self.time[np.isfinite(self.time)]
        return float(t.max()) if t.size else 0.0


def _weights(weights, n):
    """u64 weights of n pairs (None: ones); negative or oversized: ValueError."""
    if weights is None:
        return np.ones(n, np.uint64)
    ws = [int(x) for x in weights]
    if len(ws) != n:
        raise ValueError("one weight per pair")
    if any(x < 0 or x > _U64 for x in ws):
        raise ValueError("weights are unsigned 64-bit integers")
    return np.array(ws, np.uint64) if ws else np.zeros(0, np.uint64)


class TopologyDB(object):
    """Reference-compatible topology store with GPU route tables.

    ``engine``: a :class:`~sdnmpi_amd.engine.RouteEngine` to share between
    databases (default: one on HIP device ``device`` -- or, with
    ``devices=[...]``, one context over several GPUs of the node with the
    sources sharded across them -- created lazily).
    ``table_budget``: bytes of device tables kept per route mode (default
    ``engine.DEFAULT_TABLE_BUDGET``); beyond it the oldest rows are evicted
    and batches shrink to what fits.
    ``batch_sources``: when a table must be computed, compute it for every
    host-bearing switch at once (the all-pairs batch) instead of only the
    switch asked about.
    ``incremental``: after a link change over the same switch set, keep the
    cached rows the change cannot alter (:mod:`sdnmpi_amd.incremental`) and
    recompute only the others.
    """

    def __init__(self, engine=None, device=0, batch_sources=True, incremental=True,
                 devices=None, table_budget=None):
        super(TopologyDB, self).__init__()
        self._versions = Versions()
        self._engine = engine
        self._device = list(devices) if devices else device
        self._budget = table_budget
        self._batch = batch_sources
        self._incremental = incremental
        self._export = None
        self._cache = None
        self._em = (None, None, None)    # (links/switches version, edge-port state, export)
        self._link_costs = {}            # (src dpid, dst dpid) -> cost (operator configuration)
        self._cost_version = 0
        self._cost_vec = None            # (export, cost version, uint32 [E] costs)
        self._cost_memo = None           # least-cost rows per destination (_cost_rows)
        self._link_utils = {}            # (src dpid, dst dpid) -> utilisation (monitor data)
        self._util_version = 0
        self._util_vec = None            # (export, utilisation version, uint32 [E])
        self._util_memo = None           # least-loaded rows per destination (_widest_rows)
        # Switch DPID -> Switch; src DPID -> dst DPID -> Link; MAC -> Host
        self.switches = {}
        self.links = {}
        self.hosts = {}

    # -- dict state (assignable, as the reference tests do) -----------
    @property
    def switches(self):
        return self._switches

    @switches.setter
    def switches(self, d):
        self._switches = TrackedDict(self._versions, "switches", d)

    @property
    def links(self):
        return self._links

    @links.setter
    def links(self, d):
        self._links = TrackedDict(self._versions, "links", d, nested=True)

    @property
    def hosts(self):
        return self._hosts

    @hosts.setter
    def hosts(self, d):
        self._hosts = TrackedDict(self._versions, "hosts", d)

    # -- mutators (topology_db.py:20-42) -------------------------------
    def add_host(self, host):
        self.hosts[host.mac] = host

    def add_switch(self, switch):
        self.switches[switch.dp.id] = switch

    def delete_switch(self, switch):
        if switch.dp.id in self.switches:
            del self.switches[switch.dp.id]

    def add_link(self, link):
        src_dpid = link.src.dpid
        dst_dpid = link.dst.dpid
        if src_dpid not in self.links:
            self.links[src_dpid] = {}
        self.links[src_dpid][dst_dpid] = link

    def delete_link(self, link):
        src_dpid = link.src.dpid
        dst_dpid = link.dst.dpid
        if src_dpid in self.links and dst_dpid in self.links[src_dpid]:
            del self.links[src_dpid][dst_dpid]

    def to_dict(self):
        """JSON-serialisable snapshot (topology_db.py:44-57)."""
        return {
            "switches": [s.to_dict() for s in self.switches.values()],
            "links": [lk.to_dict() for nb in self.links.values() for lk in nb.values()],
            "hosts": [h.to_dict() for h in self.hosts.values()],
        }

    # -- engine / cache ------------------------------------------------
    @property
    def engine(self):
        if self._engine is None:
            self._engine = RouteEngine(self._device)
        return self._engine

    def graph(self):
        """Current CSR export.  Mutations since the last export are followed
        from the dicts' journal (graph.update_export: O(changed rows)); a
        vertex-set change or a whole-dict assignment re-exports."""
        key = self._versions.key()
        ex = self._export
        if ex is not None and ex.key == key:
            return ex
        journal = self._versions.take()
        res = None
        if ex is not None and journal is not None:
            res = update_export(ex, journal, self.links, self.switches, self.hosts, key)
        if res is None:
            new = export_graph(self.links, self.switches, self.hosts, key)
            if ex is not None and _same_graph(ex.csr, new.csr):
                # same links over the same vertex set (e.g. hosts moved)
                ex.key = key
                ex.host_count, ex.is_switch, ex._hv = new.host_count, new.is_switch, None
                ex.dport = new.dport
                return ex
            diff = edge_diff(ex.csr, new.csr) if ex is not None else None
        else:
            new, diff = res
            if new is ex:                # hosts / switch entries only
                return ex
        old = self._cache
        self._export = new
        if not (self._incremental and old is not None and diff is not None and
                old.retarget(new, diff, self._engine)):
            self._cache = TableCache(new, self._budget)
        return new

    def _host_vertices(self, ex):
        return ex.host_vertices()

    def _dfs(self, ex, s):
        """(parent, port) host rows of source s (one row copied back from
        the device tables, kept in a small host cache)."""
        c = self._cache
        if s not in c.dfs:
            batch = self._host_vertices(ex) if self._batch else ()
            c.dfs_rows(self.engine, [s], batch)
        return c.dfs_host_row(s)

    def _dist(self, ex, d):
        c = self._cache
        if d not in c.sp:
            batch = self._host_vertices(ex) if self._batch else ()
            c.sp_rows(self.engine, [d], batch)
        return c.sp_dist_host_row(d)

    # -- route lookup (topology_db.py:124-188) ---------------------------
    def _mac_to_int(self, mac):
        return int(mac.replace(":", ""), 16)

    def _endpoint(self, mac):
        """(dpid, is_local) for a MAC, or None when it is neither a switch
        local port nor a known host (topology_db.py:143-166)."""
        if self._mac_to_int(mac) in self.switches:
            return self._mac_to_int(mac), True
        if mac not in self.hosts:
            return None
        return self.hosts[mac].port.dpid, False

    def _last_hop(self, dst_dpid, dst_local, dst_mac):
        if dst_local:
            return (dst_dpid, OFPP_LOCAL)
        return (dst_dpid, self.hosts[dst_mac].port.port_no)

    def find_route(self, src_mac, dst_mac, multiple=False):
        """Route between two hosts (or switch-local ports) as a list of
        (datapath id, output port); with ``multiple=True`` the list of every
        shortest route in the reference's order."""
        s_local = self._mac_to_int(src_mac) in self.switches
        d_local = self._mac_to_int(dst_mac) in self.switches
        if not s_local and src_mac not in self.hosts:
            return []
        elif not d_local and dst_mac not in self.hosts:
            return []
        src_dpid = self._mac_to_int(src_mac) if s_local else self.hosts[src_mac].port.dpid
        dst_dpid = self._mac_to_int(dst_mac) if d_local else self.hosts[dst_mac].port.dpid

        ex = self.graph()
        s, d = ex.index[src_dpid], ex.index[dst_dpid]
        dpids = ex.csr.dpids
        last = self._last_hop(dst_dpid, d_local, dst_mac)
        if multiple:
            seqs = shortest_paths_lex(ex.csr.row_ptr, ex.csr.col, self._dist(ex, d), s, d)
            return [self._seq_fdb(ex, q, last) for q in seqs]
        parent_row, port_row = self._dfs(ex, s)
        seq = tree_path(parent_row, s, d)
        if not seq:
            return []
        fdb = [(int(dpids[a]), int(port_row[b])) for a, b in zip(seq, seq[1:])]
        fdb.append(last)
        return fdb

    def _seq_fdb(self, ex, seq, last):
        c, out = ex.csr, []
        for a, b in zip(seq, seq[1:]):
            lo, hi = int(c.row_ptr[a]), int(c.row_ptr[a + 1])
            e = lo + int(np.searchsorted(c.col[lo:hi], b))
            out.append((int(c.dpids[a]), int(c.port[e])))
        out.append(last)
        return out

    # -- flood helper --------------------------------
    def _edge_state(self):
        """(sorted link-end keys, {(dpid, port_no): is_edge} of every switch
        port) for the current links/switches, from one device pass
        (sdnr_edge_ports) per version instead of the reference's scan over
        every link per port.  Keys: dense switch id << 32 | port_no; the link
        ends come from the export (both ends of every CSR entry), keyed with
        the same dense ids (the cache is tied to the export object)."""
        key = (self._versions.links, self._versions.switches)
        ex = self.graph()
        if self._em[0] != key or self._em[2] is not ex:
            idx = ex.index
            ends = ex.link_ends()
            ports, keys = [], []
            for sw in self.switches.values():
                for p in getattr(sw, "ports", ()):
                    d = idx.get(p.dpid)
                    if d is not None:
                        ports.append((p.dpid, p.port_no))
                        keys.append((d << 32) | (int(p.port_no) & 0xFFFFFFFF))
            mask = self.engine.edge_ports(ends, np.asarray(keys, np.uint64)) if keys else []
            self._em = (key, (ends, dict(zip(ports, (bool(m) for m in mask)))), ex)
        return self._em[1]

    def is_edge_port(self, port):
        """``TopologyManager._is_edge_port`` (reference sdnmpi/topology.py:
        150-155): the port is neither end of any link.  Ports of the
        switches' port lists come from the device pass; any other port is
        one binary search in the sorted link ends."""
        ends, known = self._edge_state()
        hit = known.get((port.dpid, port.port_no))
        if hit is not None:
            return hit
        d = self.graph().index.get(port.dpid)
        if d is None:                     # not a switch of the graph: no link end
            return True
        k = np.uint64((d << 32) | (int(port.port_no) & 0xFFFFFFFF))
        i = int(np.searchsorted(ends, k))
        return not (i < ends.shape[0] and ends[i] == k)

    def edge_ports(self, switch, in_port=None):
        """The ports ``_do_broadcast`` floods on ``switch`` (topology.py:
        157-168): edge ports that are not reserved, minus ``in_port``."""
        return [p for p in switch.ports
                if self.is_edge_port(p) and not p.is_reserved()
                and (in_port is None or p.port_no != in_port)]

    def broadcast_ports(self, dpid, in_port):
        """{switch dpid: [port_no, ...]} -- every OFPActionOutput
        ``_do_broadcast(data, dpid, in_port)`` emits (topology.py:157-177):
        each switch's non-reserved edge ports, the ingress port excluded on
        the switch the packet came from."""
        _, known = self._edge_state()
        out = {}
        for sw in self.switches.values():
            out[sw.dp.id] = [p.port_no for p in sw.ports
                             if known.get((p.dpid, p.port_no), True) and not p.is_reserved()
                             and not (sw.dp.id == dpid and p.port_no == in_port)]
        return out

    # -- batched (all-pairs) interface ---------------------------------
    def route_tables(self, mode="dfs", vertices=None):
        """Tables for every host-bearing switch (or the dense ``vertices``
        given, e.g. one rank's shard: :func:`sdnmpi_amd.distributed.
        sharded_route_tables`).

        ``mode="dfs"``: per-source trees of the default route,
        dict(sources, parent, port, hops, dpids);  ``mode="shortest"``:
        per-destination dict(destinations, dist, nh, nh_port, dpids).
        """
        if mode not in ("dfs", "shortest"):
            raise ValueError("mode must be 'dfs' or 'shortest'")
        ex = self.graph()
        hv = self._host_vertices(ex) if vertices is None else [int(v) for v in vertices]
        c = self._cache
        store = c.dfs if mode == "dfs" else c.sp
        get = c.dfs_rows if mode == "dfs" else c.sp_rows
        V = ex.csr.V
        n = len(hv)
        cols = [np.empty((n, V), np.int32), np.empty((n, V), np.int32),
                np.empty((n, V), np.int32)] if mode == "dfs" else \
            [np.empty((n, V), np.uint16), np.empty((n, V), np.int32), np.empty((n, V), np.int32)]
        step = max(1, store.cap())
        # decoded a bounded slice at a time (int64 temporaries of a whole
        # budget's rows would be tens of GB on the torus / Jellyfish)
        sl = max(1, TABLE_SLICE_ENTRIES // max(1, V))
        for i in range(0, n, step):                 # a budget's worth of rows at a time
            chunk = hv[i:i + step]
            get(self.engine, chunk)
            idx = np.asarray([store.row[v] for v in chunk], np.int64)
            for j in range(0, len(chunk), sl):
                part = idx[j:j + sl]
                r0, r1 = i + j, i + j + part.size
                if mode == "dfs":
                    for k, a in enumerate(c.dfs_int32(part, self.engine)):
                        cols[k][r0:r1] = _host(a)
                else:
                    d, nh, nhp = c.sp_decoded(part, self.engine)
                    cols[0][r0:r1] = d
                    cols[1][r0:r1] = nh
                    cols[2][r0:r1] = nhp
        if mode == "dfs":
            return {"sources": np.asarray(hv, np.int32), "parent": cols[0],
                    "port": cols[1], "hops": cols[2], "dpids": ex.csr.dpids}
        return {"destinations": np.asarray(hv, np.int32), "dist": cols[0],
                "nh": cols[1], "nh_port": cols[2], "dpids": ex.csr.dpids}

    def _find_routes_multiple(self, pairs):
        """find_route(a, b, multiple=True) for many pairs: per-destination
        distances from the GPU tables, the ECMP sets counted and unranked on the
        GPU (ecmp.hip), each route turned into its fdb as _route_to_fdb does."""
        ex = self.graph()
        n = len(pairs)
        ends = [None] * n
        want = []
        for i, (a, b) in enumerate(pairs):
            ea, eb = self._endpoint(a), self._endpoint(b)
            if ea is None or eb is None:
                continue
            s, d = ex.index[ea[0]], ex.index[eb[0]]
            ends[i] = (s, d, self._last_hop(eb[0], eb[1], b))
            want.append(d)
        out = [[] for _ in range(n)]
        if not want:
            return out
        batch = self._host_vertices(ex) if self._batch else ()
        idx_all = [i for i in range(n) if ends[i] is not None]
        uniq = sorted(set(want))
        step = max(1, self._cache.sp.cap() - 1) if self._cache.sp.row_bytes else len(uniq)
        for c0 in range(0, len(uniq), step):          # a budget's worth of rows at a time
            chunk = set(uniq[c0:c0 + step])
            tabs = self._cache.sp_rows(self.engine, sorted(chunk), batch if c0 == 0 else ())
            idx = [i for i in idx_all if ends[i][1] in chunk]
            rows = [self._cache.sp_row[ends[i][1]] for i in idx]
            srcs = [ends[i][0] for i in idx]
            # only the destination rows these pairs use go to the GPU
            urows, inv = np.unique(np.asarray(rows, np.int64), return_inverse=True)
            sets = self.engine.ecmp(ex, _take(tabs[0], urows), inv, srcs)
            for i, seqs in zip(idx, sets):
                last = ends[i][2]
                out[i] = [self._seq_fdb(ex, [int(v) for v in q], last) for q in seqs]
        return out

    def route_entries(self, pairs):
        """Flow entries of many (src_mac, dst_mac) pairs in one GPU pass --
        what ``Router._add_flows_for_path`` installs for each pair (reference
        ``sdnmpi/router.py:83-104``), e.g. for every MPI rank pair of a job.

        Returns ``(offsets, dpid, port)`` numpy arrays: pair i's fdb is
        ``list(zip(dpid[o[i]:o[i+1]], port[o[i]:o[i+1]]))``, equal to
        ``find_route(*pairs[i])`` (empty for unknown hosts or unreachable
        destinations).
        """
        pairs = list(pairs)
        n = len(pairs)
        ex = self.graph()
        sv = np.full(n, -1, np.int64)
        dv = np.full(n, -1, np.int64)
        last = np.zeros(n, np.int64)
        for i, (a, b) in enumerate(pairs):
            ea, eb = self._endpoint(a), self._endpoint(b)
            if ea is None or eb is None:
                continue
            sv[i] = ex.index[ea[0]]
            dv[i] = ex.index[eb[0]]
            last[i] = self._last_hop(eb[0], eb[1], b)[1]
        ok = np.nonzero(sv >= 0)[0]
        off = np.zeros(n + 1, np.int64)
        if ok.size == 0:
            return off, np.zeros(0, np.int64), np.zeros(0, np.int32)
        want = sorted(set(sv[ok].tolist()))
        batch = self._host_vertices(ex) if self._batch else ()
        c = self._cache
        step = max(1, c.dfs.cap() - 1) if c.dfs.row_bytes else len(want)
        lens = np.zeros(n, np.int64)
        pieces = []                   # (pair ids, offsets, switches, ports) per source chunk
        for c0 in range(0, len(want), step):        # a budget's worth of sources at a time
            chunk = want[c0:c0 + step]
            c.dfs_rows(self.engine, chunk, batch if c0 == 0 else ())
            mine = ok[np.isin(sv[ok], np.asarray(chunk, np.int64))]
            slots = np.asarray([c.dfs_row[v] for v in sv[mine].tolist()], np.int64)
            # only the rows these pairs use are decoded for the expansion
            urows, inv = np.unique(slots, return_inverse=True)
            tabs = c.dfs_int32(urows, self.engine)
            o, sw, hp = self.engine.expand(ex, tabs, inv, dv[mine], last[mine])
            lens[mine] = np.diff(o)
            pieces.append((mine, o, sw, hp))
        np.cumsum(lens, out=off[1:])
        total = int(off[-1])
        sw_all = np.zeros(total, np.int64)
        hp_all = np.zeros(total, np.int32)
        for mine, o, sw, hp in pieces:
            if len(pieces) == 1 and mine.size == n:
                sw_all, hp_all = sw, hp
                break
            dst0 = off[mine]                      # pair starts in the full output
            ln = np.diff(o)
            pos = np.repeat(dst0 - o[:-1], ln) + np.arange(int(o[-1]))
            sw_all[pos] = sw
            hp_all[pos] = hp
        return off, ex.csr.dpids[np.asarray(sw_all, np.int64)], hp_all

    def switch_fdb_entries(self, pairs, keys=None):
        """The flow entries of many (src_mac, dst_mac) pairs grouped by switch
        -- what ``Router._add_flows_for_path`` records in ``SwitchFDB``
        (reference ``sdnmpi/router.py:83-104``, ``util/switch_fdb.py:6-9``:
        ``_dpid_to_fdb[dpid][(src, dst)] = out_port``) when every pair's route
        is installed in order.  A (src, dst) key already recorded on a switch
        keeps its first out_port, as the router's ``exists`` check does.

        Returns ``(dpids, off, pair, out_port, last)`` numpy arrays: switch
        ``dpids[k]`` holds the entries ``off[k]:off[k+1]``, entry j being
        pair ``pair[j]`` (index into ``pairs``) leaving on ``out_port[j]``;
        ``last[j]`` marks the pair's destination switch (where the router
        adds the SetDlDst action for an MPI flow, :97-100).  Switches ascend
        by dpid, entries keep pair order within a switch.

        ``keys``: the SwitchFDB key of each pair when it is not the pair
        itself -- an MPI flow is recorded under (src MAC, the virtual
        destination MAC), ``router.py:189-193`` (see :meth:`mpi_flow_entries`)."""
        pairs = list(pairs)
        keys = pairs if keys is None else list(keys)
        if len(keys) != len(pairs):
            raise ValueError("one SwitchFDB key per pair")
        off, dp, pt = self.route_entries(pairs)
        n = len(pairs)
        lens = np.diff(off)
        pid = np.repeat(np.arange(n, dtype=np.int64), lens)
        last = np.zeros(int(off[-1]), bool)
        ends = off[1:][lens > 0] - 1
        last[ends] = True
        # first occurrence of every (src, dst) key wins (SwitchFDB.exists)
        seen = {}
        first = np.fromiter((seen.setdefault(k, i) for i, k in enumerate(keys)), np.int64, n)
        keep = first[pid] == pid          # (routes are simple paths: one entry per switch)
        pid, dp, pt, last = pid[keep], np.asarray(dp)[keep], np.asarray(pt)[keep], last[keep]
        order = np.lexsort((np.arange(pid.shape[0]), dp))           # by dpid, stable
        dp, pid, pt, last = dp[order], pid[order], pt[order], last[order]
        if dp.shape[0]:
            newsw = np.ones(dp.shape[0], bool)
            newsw[1:] = dp[1:] != dp[:-1]
            starts = np.nonzero(newsw)[0]
            dpids = dp[starts]
            soff = np.append(starts, dp.shape[0]).astype(np.int64)
        else:
            dpids = np.zeros(0, np.int64)
            soff = np.zeros(1, np.int64)
        return dpids.astype(np.int64), soff, pid, pt.astype(np.int32), last

    def mpi_flow_entries(self, rank_to_mac, coll_type=0):
        """The SDN-MPI flows of every ordered rank pair of a job, grouped by
        switch: for ranks i != j (``rank_to_mac``: ProcessManager's
        RankAllocationDB map, reference ``process.py:107-110``) the router
        installs, per switch of ``find_route(mac_i, mac_j)``, a flow matching
        (src ``mac_i``, dst the virtual address ``sdn_mpi_mac(coll_type, i,
        j)``) whose last hop rewrites the destination to ``mac_j``
        (``router.py:166-200``).  The router records each flow in SwitchFDB
        under (``mac_i``, virtual MAC), so ranks sharing a host keep one flow
        per rank pair (``router.py:189-193``, ``switch_fdb.py:6-13``).
        Returns ``(dpids, off, src_rank, dst_rank, out_port, last)`` as
        :meth:`switch_fdb_entries` lays them out."""
        ranks = sorted(rank_to_mac)
        src_r = [a for a in ranks for b in ranks if a != b]
        dst_r = [b for a in ranks for b in ranks if a != b]
        pairs = [(rank_to_mac[a], rank_to_mac[b]) for a, b in zip(src_r, dst_r)]
        keys = [(rank_to_mac[a], sdn_mpi_mac(coll_type, a, b)) for a, b in zip(src_r, dst_r)]
        dpids, off, pid, pt, last = self.switch_fdb_entries(pairs, keys)
        sr = np.asarray(src_r, np.int64)[pid] if pid.size else np.zeros(0, np.int64)
        dr = np.asarray(dst_r, np.int64)[pid] if pid.size else np.zeros(0, np.int64)
        return dpids, off, sr, dr, pt, last

    # -- predicted link loads -------------------------------------------
    def _switch_pair_loads(self, ex, sv, dv, w, route):
        """(load uint64 [E], reach bool [n]) of switch pairs (dense ids sv ->
        dv, weights w u64) routed the default way (per-source trees) or along
        routes[0] of the shortest mode (per-destination next-hop rows): one
        sdnr_link_loads call per budget-sized chunk of table rows."""
        if route not in ("default", "shortest"):
            raise ValueError("route must be 'default' or 'shortest'")
        E, V = int(ex.csr.E), int(ex.csr.V)
        load = np.zeros(E, np.uint64)
        reach = np.zeros(sv.shape[0], bool)
        if sv.size == 0:
            return load, reach
        c = self._cache
        short = route == "shortest"
        store = c.sp if short else c.dfs
        key, other = (dv, sv) if short else (sv, dv)       # table row / vertex inside it
        want = sorted(set(key.tolist()))
        batch = self._host_vertices(ex) if self._batch else ()
        step = max(1, store.cap() - 1) if store.row_bytes else len(want)
        if short:      # the next-hop rows are widened to int32: bounded temporaries
            step = min(step, max(1, TABLE_SLICE_ENTRIES // max(1, V)))
        for c0 in range(0, len(want), step):      # a budget's worth of rows at a time
            chunk = want[c0:c0 + step]
            get = c.sp_rows if short else c.dfs_rows
            tabs = get(self.engine, chunk, batch if c0 == 0 else ())
            mine = np.nonzero(np.isin(key, np.asarray(chunk, np.int64)))[0]
            slots = np.asarray([store.row[v] for v in key[mine].tolist()], np.int64)
            # hops / distance planes hold -1 (u16 0xFFFF as int16) where unreached
            reach[mine] = _gather(tabs[0] if short else tabs[-1], slots, other[mine]) != -1
            if short:
                urows, inv = np.unique(slots, return_inverse=True)
                nh = _take(tabs[1], urows)
                nh = _u16(nh) if V <= 0xFFFF else nh
                nh = nh.astype(np.int32) if isinstance(nh, np.ndarray) else \
                    nh.to(dtype=_torch().int32)
                load += self.engine.link_loads(ex, nh, INT32, inv, other[mine], w[mine],
                                               to_root=True)
            else:
                load += self.engine.link_loads(ex, tabs[0], c.layout, slots, other[mine],
                                               w[mine])
        return load, reach

    def _link_loads_result(self, ex, load, hkey, hload, cls=LinkLoads):
        """LinkLoads of CSR-ordered link loads plus last hops ``hkey`` ([k, 2]
        int64 rows (dense switch, port), unique) with loads ``hload``."""
        csr = ex.csr
        rp = np.asarray(csr.row_ptr, np.int64)
        esrc = np.repeat(np.arange(csr.V, dtype=np.int64), np.diff(rp))
        dp = np.asarray(csr.dpids)
        nz = np.nonzero(hload)[0]
        hkey, hload = hkey[nz], hload[nz]
        return cls(dp, esrc, np.asarray(csr.col, np.int64), np.asarray(csr.port, np.int64),
                   load, hkey[:, 0], hkey[:, 1], hload)

    def _switch_pairs(self, ex, pairs, weights):
        """MAC pairs resolved to switches and summed to switch pairs: (w u64
        per pair, dv, last -- destination switch and last-hop port per pair --,
        ok -- the pairs whose hosts are known --, inv -- the switch pair of
        each of those --, and the switch pairs' dense sources, destinations
        and summed weights)."""
        pairs = list(pairs)
        n = len(pairs)
        w = _weights(weights, n)
        V = int(ex.csr.V)
        sv = np.full(n, -1, np.int64)
        dv = np.full(n, -1, np.int64)
        last = np.zeros(n, np.int64)
        for i, (a, b) in enumerate(pairs):
            ea, eb = self._endpoint(a), self._endpoint(b)
            if ea is None or eb is None:
                continue
            sv[i] = ex.index[ea[0]]
            dv[i] = ex.index[eb[0]]
            last[i] = self._last_hop(eb[0], eb[1], b)[1]
        ok = np.nonzero(sv >= 0)[0]
        # MAC pairs -> switch pairs, weights summed
        skey, inv = np.unique(sv[ok] * max(1, V) + dv[ok], return_inverse=True)
        sw = np.zeros(skey.shape[0], np.uint64)
        np.add.at(sw, inv, w[ok])
        return w, dv, last, ok, inv, skey // max(1, V), skey % max(1, V), sw

    def _pair_loads(self, pairs, weights, switch_loads, cls):
        """The MAC-pair form shared by :meth:`link_loads` and
        :meth:`ecmp_link_loads`: the pairs are resolved to switches, summed to
        switch pairs, handed to ``switch_loads(ex, sv, dv, w)`` -> (load [E],
        reach bool per switch pair), and the last hops -- (destination
        switch, host port or OFPP_LOCAL) of the pairs whose route exists --
        are added."""
        ex = self.graph()
        w, dv, last, ok, inv, ssv, sdv, sw = self._switch_pairs(ex, pairs, weights)
        load, reach = switch_loads(ex, ssv, sdv, sw)
        got = ok[reach[inv]] if ok.size else ok              # pairs whose route exists
        hkey, hinv = np.unique(np.stack([dv[got], last[got]], 1), axis=0, return_inverse=True)
        hload = np.zeros(hkey.shape[0], np.uint64)
        np.add.at(hload, hinv.reshape(-1), w[got])
        return self._link_loads_result(ex, load, hkey.reshape(-1, 2), hload, cls)

    def _all_pairs_loads(self, switch_loads, cls):
        """The all-host-pairs form shared by :meth:`all_pairs_link_loads` and
        :meth:`all_pairs_ecmp_link_loads`, from the per-switch host counts:
        the demand of switch pair (s, d) is hosts(s) * hosts(d), never
        expanded to MAC pairs.  None when a host MAC names a switch (it
        resolves to the switch's local port: the caller takes the MAC-pair
        form)."""
        if any(self._mac_to_int(m) in self.switches for m in self.hosts):
            return None
        ex = self.graph()
        hv = np.asarray(self._host_vertices(ex), np.int64)
        hc = np.asarray(ex.host_count, np.int64)
        n = hv.shape[0]
        sv, dv = np.repeat(hv, n), np.tile(hv, n)
        w = (hc[sv] * (hc[dv] - (sv == dv))).astype(np.uint64)
        load, reach = switch_loads(ex, sv, dv, w)
        # hosts that reach switch d: every host on d gets that many flows, less itself
        cnt = (reach.reshape(n, n) * hc[hv][:, None]).sum(0)
        into = np.zeros(int(ex.csr.V), np.int64)
        into[hv] = cnt - 1
        hd = np.asarray([ex.index[h.port.dpid] for h in self.hosts.values()], np.int64)
        hp = np.asarray([int(h.port.port_no) for h in self.hosts.values()], np.int64)
        hkey, hinv = np.unique(np.stack([hd, hp], 1).reshape(-1, 2), axis=0, return_inverse=True)
        hload = np.zeros(hkey.shape[0], np.uint64)
        np.add.at(hload, hinv.reshape(-1), into[hd].astype(np.uint64))
        return self._link_loads_result(ex, load, hkey.reshape(-1, 2), hload, cls)

    @staticmethod
    def _rank_pairs(rank_to_mac, traffic):
        """(pairs, weights) of an MPI job's traffic: {(src_rank, dst_rank):
        weight} between known ranks; None: every ordered rank pair, weight 1."""
        if traffic is None:
            ranks = sorted(rank_to_mac)
            return [(rank_to_mac[a], rank_to_mac[b]) for a in ranks for b in ranks if a != b], None
        items = [(k, x) for k, x in traffic.items() if k[0] in rank_to_mac and k[1] in rank_to_mac]
        return [(rank_to_mac[a], rank_to_mac[b]) for (a, b), _ in items], [x for _, x in items]

    def link_loads(self, pairs, weights=None, route="default"):
        """How much traffic crosses each link when every (src_mac, dst_mac)
        pair of ``pairs`` sends ``weights[i]`` (non-negative ints, e.g. bytes;
        None: 1 each) along the controller's route -- the per-port traffic
        ``sdnmpi/monitor.py`` would log for the flows ``Router.
        _add_flows_for_path`` installs (reference ``router.py:83-104``) -- as a
        :class:`LinkLoads`.

        Defining property: ``link_loads(pairs, w).as_dict()`` equals the sum
        over i of ``w[i]`` on every ``(dpid, out_port)`` entry of
        ``find_route(*pairs[i])``; with ``route="shortest"`` the entries are
        those of ``find_route(*pairs[i], multiple=True)[0]``.  Unknown hosts
        and unreachable pairs contribute nothing (``find_route`` returns
        ``[]``); repeated pairs add.  No flow entry is built: the MAC pairs
        are summed to switch pairs, the GPU turns each table row's demand
        into subtree sums (loads.hip), and the last hops -- (destination
        switch, host port or OFPP_LOCAL) -- are added here.  Sums are
        unsigned 64-bit and wrap."""
        return self._pair_loads(
            pairs, weights, lambda ex, sv, dv, w: self._switch_pair_loads(ex, sv, dv, w, route),
            LinkLoads)

    def all_pairs_link_loads(self, route="default"):
        """:meth:`link_loads` over every ordered pair of distinct hosts with
        weight 1 (all-to-all traffic), from the per-switch host counts: the
        demand of switch pair (s, d) is hosts(s) * hosts(d), never expanded
        to MAC pairs (764 M host pairs on the k=48 fat-tree are 1,152^2
        switch demands)."""
        got = self._all_pairs_loads(
            lambda ex, sv, dv, w: self._switch_pair_loads(ex, sv, dv, w, route), LinkLoads)
        if got is None:
            macs = list(self.hosts)
            return self.link_loads([(a, b) for a in macs for b in macs if a != b], None, route)
        return got

    def mpi_link_loads(self, rank_to_mac, traffic=None, route="default"):
        """:meth:`link_loads` of an MPI job: ``traffic`` = {(src_rank,
        dst_rank): weight} between the ranks of ``rank_to_mac`` (a rank the
        map lacks is an unknown host); None: every ordered rank pair i != j
        with weight 1 -- the pairs of :meth:`mpi_flow_entries`."""
        pairs, weights = self._rank_pairs(rank_to_mac, traffic)
        return self.link_loads(pairs, weights, route)

    # -- multicast trees ---------------------------------------------------
    def _multicast_union(self, ex, rv, moff, mv, w, route, entries, loads):
        """The multicast trees of switch-level groups: group g has root
        ``rv[g]`` and the member switches ``mv[moff[g]:moff[g+1]]`` (dense
        ids), weight ``w[g]``.  Returns ``(reached bool per member, ent_off,
        ent_edge, load)`` as :meth:`RouteEngine.multicast_trees` does
        (``ent_edge`` / ``load`` None when not asked for).  Rows come from the
        caches in budget-sized chunks -- the roots' trees for the default
        route, the members' next-hop rows for the shortest and least-cost
        routes; when one chunk does not hold them all, the chunks' entries are
        merged here (a group's members may lie in several chunks) and the
        loads are counted from the merged entries."""
        if route == "least_loaded":
            raise ValueError("least-loaded routes are not prefix-consistent: the union of "
                             "their entries is no tree")
        if route not in ("default", "shortest", "least_cost"):
            raise ValueError("route must be 'default', 'shortest' or 'least_cost'")
        eng = self.engine
        if not hasattr(eng, "multicast_trees"):
            raise ValueError("the engine has no multicast_trees")
        E, V = int(ex.csr.E), int(ex.csr.V)
        ng, nmem = int(rv.shape[0]), int(mv.shape[0])
        reached = np.zeros(nmem, bool)
        if nmem == 0:
            return (reached, np.zeros(ng + 1, np.int64), np.zeros(0, np.int32) if entries else None,
                    np.zeros(E, np.uint64) if loads else None)
        grp = np.repeat(np.arange(ng, dtype=np.int64), np.diff(moff))
        c = self._cache
        default = route == "default"
        key = rv[grp] if default else mv               # the table row each member is walked in
        want = np.unique(key).tolist()
        batch = self._host_vertices(ex) if self._batch else ()
        if route == "least_cost":
            step = self._cost_cap(ex)
        else:
            store = c.dfs if default else c.sp
            step = max(1, store.cap() - 1) if store.row_bytes else len(want)
            if not default:    # the next-hop rows are widened to int32: bounded temporaries
                step = min(step, max(1, TABLE_SLICE_ENTRIES // max(1, V)))
        single = len(want) <= step

        def slots_of(slot, verts):
            """(the distinct table slots of the vertices, ascending; each vertex's index
            among them) -- one dict lookup per distinct vertex"""
            uv, inv = np.unique(verts, return_inverse=True)
            sl = np.asarray([slot[v] for v in uv.tolist()], np.int64).reshape(-1)
            us, pos = np.unique(sl, return_inverse=True)
            return us, pos.reshape(-1)[inv.reshape(-1)]

        found = []
        for c0 in range(0, len(want), step):      # a budget's worth of rows at a time
            chunk = want[c0:c0 + step]
            sel = np.nonzero(np.isin(key, np.asarray(chunk, np.int64)))[0]
            off = np.zeros(ng + 1, np.int64)
            np.cumsum(np.bincount(grp[sel], minlength=ng), out=off[1:])
            if route == "least_cost":
                m = self._cost_rows(ex, chunk)
                urows, rows = slots_of(m["slot"], key[sel])
                tab, lay = _take(m["tabs"][1], urows), INT32
            elif default:
                tabs = c.dfs_rows(eng, chunk, batch if c0 == 0 else ())
                urows, rows = slots_of(store.row, key[sel])
                rows = urows[rows]
                tab, lay = tabs[0], c.layout
            else:
                tabs = c.sp_rows(eng, chunk, batch if c0 == 0 else ())
                urows, rows = slots_of(store.row, key[sel])
                nh = _take(tabs[1], urows)
                nh = _u16(nh) if V <= 0xFFFF else nh
                tab = nh.astype(np.int32) if isinstance(nh, np.ndarray) else \
                    nh.to(dtype=_torch().int32)
                lay = INT32
            r, eo, ee, ld = eng.multicast_trees(ex, tab, lay, rv, off, rows.reshape(-1), mv[sel],
                                                w, to_root=not default,
                                                entries=entries or not single,
                                                loads=loads and single)
            reached[sel] = np.asarray(r, bool)
            if single:
                return reached, eo, ee, ld
            found.append(np.repeat(np.arange(ng, dtype=np.int64), np.diff(eo)) * max(E, 1) +
                         np.asarray(ee, np.int64))
        pairs = np.unique(np.concatenate(found))
        pg, pe = pairs // max(E, 1), pairs % max(E, 1)
        ent_off = np.zeros(ng + 1, np.int64)
        np.cumsum(np.bincount(pg, minlength=ng), out=ent_off[1:])
        load = None
        if loads:
            load = np.zeros(E, np.uint64)
            np.add.at(load, pe, w[pg])
        return reached, ent_off, pe.astype(np.int32) if entries else None, load

    def _multicast_resolve(self, ex, groups):
        """MAC groups -> switch groups.  Per member MAC that is known, is not
        the group's source and whose source is known: its group ``mg``, its
        position among the group's members ``mi``, its switch ``dv`` and last-
        hop port ``last``; then the switch-level groups -- roots ``rv`` (-1:
        unknown source), offsets ``moff`` and member switches ``mv``, unique
        per group -- and ``inv``, the switch-level member of each MAC member."""
        groups = [(a, list(ms)) for a, ms in groups]
        ng = len(groups)
        rv = np.full(ng, -1, np.int64)
        # every distinct MAC is resolved once, to an id into ``info`` = (switch
        # or -1 when unknown, last-hop port); the rest is array work
        mid, info = {}, []

        def ident(m):
            if m not in mid:
                ep = self._endpoint(m)
                mid[m] = len(info)
                info.append((-1, 0) if ep is None else
                            (ex.index[ep[0]], self._last_hop(ep[0], ep[1], m)[1]))
            return mid[m]

        src = np.asarray([ident(a) for a, _ in groups], np.int64).reshape(-1)
        ids = []
        for _, ms in groups:
            got = [mid.get(m, -1) for m in ms]
            if -1 in got:                                  # (every MAC is checked)
                got = [ident(m) for m in ms]
            ids.append(np.asarray(got, np.int64).reshape(-1))
        lens = np.asarray([x.shape[0] for x in ids], np.int64).reshape(-1)
        ids = np.concatenate(ids) if ids else np.zeros(0, np.int64)
        tab = np.asarray(info, np.int64).reshape(-1, 2)
        if ng:
            rv = tab[src, 0]
        mg = np.repeat(np.arange(ng, dtype=np.int64), lens)
        mi = np.arange(ids.shape[0], dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
        keep = (tab[ids, 0] >= 0) & (ids != src[mg]) & (rv[mg] >= 0) if ids.size else \
            np.zeros(0, bool)
        mg, mi = mg[keep], mi[keep]
        dv, last = tab[ids[keep], 0], tab[ids[keep], 1]
        V = max(1, int(ex.csr.V))
        skey, inv = np.unique(mg * V + dv, return_inverse=True)
        moff = np.zeros(ng + 1, np.int64)
        np.cumsum(np.bincount(skey // V, minlength=ng), out=moff[1:])
        return groups, rv, mg, mi, dv, last, moff, skey % V, inv.reshape(-1)

    def _multicast_entries(self, groups, route):
        """(groups, off, dpid, port, got): the sorted entry set of every group
        and ``got`` = (mg, mi) of the member MACs whose route exists."""
        ex = self.graph()
        groups, rv, mg, mi, dv, last, moff, mv, inv = self._multicast_resolve(ex, groups)
        ng = len(groups)
        w = np.ones(ng, np.uint64)
        reach, eo, ee, _ = self._multicast_union(ex, rv, moff, mv, w, route, True, False)
        ok = reach[inv] if inv.size else np.zeros(0, bool)
        csr = ex.csr
        rp = np.asarray(csr.row_ptr, np.int64)
        esrc = np.repeat(np.arange(csr.V, dtype=np.int64), np.diff(rp))
        ee = np.asarray(ee, np.int64)
        eg = np.repeat(np.arange(ng, dtype=np.int64), np.diff(eo))
        dp = np.asarray(csr.dpids, np.int64)
        V = max(1, int(csr.V))
        eport = np.asarray(csr.port, np.int64)[ee]
        if ng * V < (1 << 31) and (eport.size == 0 or 0 <= eport.min()) and \
                (not ok.any() or 0 <= last[ok].min()) and \
                max(int(eport.max()) if eport.size else 0, int(last.max()) if last.size else 0) \
                < (1 << 32):
            # one int64 key per entry -- (group, dense switch, port), the order of (group,
            # dpid, port) since dense ids ascend with the dpids --, each entry once
            key = np.unique(np.concatenate([((eg * V + esrc[ee]) << 32) | eport,
                                            ((mg[ok] * V + dv[ok]) << 32) | last[ok]]))
            gs, pt = key >> 32, key & 0xFFFFFFFF
            g_of, sw = gs // V, dp[gs % V]
        else:
            rec = np.unique(np.concatenate([np.stack([eg, esrc[ee], eport], 1),
                                            np.stack([mg[ok], dv[ok], last[ok]], 1)]
                                           ).reshape(-1, 3), axis=0)
            g_of, sw, pt = rec[:, 0], dp[rec[:, 1]], rec[:, 2]
        off = np.zeros(ng + 1, np.int64)
        np.cumsum(np.bincount(g_of, minlength=ng), out=off[1:])
        return groups, off, sw.astype(np.asarray(csr.dpids).dtype), pt.astype(np.int32), \
            (mg[ok], mi[ok])

    def multicast_trees(self, groups, route="default"):
        """The flow entries of one-to-many groups with in-network replication:
        ``groups = [(src_mac, [dst_mac, ...]), ...]``; group i's multicast tree
        is installed as one entry per (switch, out port) -- OpenFlow 1.0 lets
        an entry carry several output actions, so a switch on several members'
        routes forwards the frame once per distinct port.

        Returns ``(off, dpid, port)`` numpy arrays shaped as
        :meth:`route_entries` returns them.  Defining property: group i's
        slice ``zip(dpid[off[i]:off[i+1]], port[off[i]:off[i+1]])`` equals
        ``sorted(set(e for m in members for e in route(src, m)))`` where
        ``route`` is ``find_route(src, m)`` (``"default"``),
        ``find_route(src, m, multiple=True)[0]`` (``"shortest"``) or
        ``find_route_least_cost(src, m)`` (``"least_cost"``).  Unknown hosts,
        unreachable members and ``m == src`` drop out.  The shortest and
        least-cost routes are the lexicographically smallest ones, so they are
        prefix-consistent and the union is a tree, like the default route's;
        ``"least_loaded"`` raises ValueError (its routes are not), and so does
        an engine without ``multicast_trees``.  No per-member route is built:
        the GPU marks the links of all members' walks in one bit map per group
        (multicast.hip) and only the union comes back; the last hops -- the
        member's host port or OFPP_LOCAL -- are added here."""
        _, off, dpid, port, _ = self._multicast_entries(groups, route)
        return off, dpid, port

    def multicast_tree(self, src_mac, dst_macs, route="default"):
        """:meth:`multicast_trees` of one group, as a :class:`MulticastTree`."""
        dst_macs = list(dst_macs)
        _, off, dpid, port, (_, mi) = self._multicast_entries([(src_mac, dst_macs)], route)
        have = set(mi.tolist())
        unreached = [m for i, m in enumerate(dst_macs) if i not in have and m != src_mac]
        return MulticastTree(src_mac, list(zip(dpid.tolist(), port.tolist())), unreached)

    def multicast_link_loads(self, groups, weights=None, route="default"):
        """What the links carry when every group's source sends ``weights[g]``
        (non-negative ints, e.g. bytes; None: 1 each) to its members down its
        multicast tree (:meth:`multicast_trees`): every link and every
        last-hop port of group g's tree carries ``weights[g]`` ONCE, however
        many members lie behind it -- as a :class:`LinkLoads`.  Its counterpart
        for the unicast fan-out, where the source sends one copy per member, is
        :meth:`link_loads` over the (src, member) pairs with the group's weight
        on each; the peak of the two is what in-network replication saves.
        Unknown hosts, unreachable members and ``m == src`` contribute nothing;
        ``route`` as in :meth:`multicast_trees`.  The loads are summed on the
        GPU from the groups' bit maps (no entry is built); sums are unsigned
        64-bit and wrap."""
        ex = self.graph()
        groups, rv, mg, mi, dv, last, moff, mv, inv = self._multicast_resolve(ex, groups)
        w = _weights(weights, len(groups))
        csr = ex.csr
        esrc = np.repeat(np.arange(csr.V, dtype=np.int64),
                         np.diff(np.asarray(csr.row_ptr, np.int64)))
        port = np.asarray(csr.port, np.int64)
        # a fabric that reuses a port number on one switch (two links, or a
        # link and a host: the random fixtures do) has entries that several
        # links or last hops share; an entry is one output action, so as_dict
        # counts it once per group, from the entries themselves
        lkey = (esrc << 32) | (port & 0xFFFFFFFF)
        reuse = np.unique(lkey).size != lkey.size or \
            bool(np.isin((dv << 32) | (last & 0xFFFFFFFF), lkey).any())
        reach, eo, ee, load = self._multicast_union(ex, rv, moff, mv, w, route, reuse, True)
        ok = reach[inv] if inv.size else np.zeros(0, bool)
        # the last hops: each (group, switch, port) once
        V = max(1, int(csr.V))
        lo = last[ok]
        if len(groups) * V < (1 << 31) and (lo.size == 0 or (0 <= lo.min() and
                                                             lo.max() < (1 << 32))):
            k = np.unique(((mg[ok] * V + dv[ok]) << 32) | lo)       # one int64 key per last hop
            rec = np.stack([(k >> 32) // V, (k >> 32) % V, k & 0xFFFFFFFF], 1)
        else:
            rec = np.unique(np.stack([mg[ok], dv[ok], lo], 1).reshape(-1, 3), axis=0)
        if rec.shape[0] and 0 <= rec[:, 2].min() and rec[:, 2].max() < (1 << 32):
            hk, hinv = np.unique((rec[:, 1] << 32) | rec[:, 2], return_inverse=True)
            hkey = np.stack([hk >> 32, hk & 0xFFFFFFFF], 1)
        else:
            hkey, hinv = np.unique(rec[:, 1:], axis=0, return_inverse=True)
        hload = np.zeros(hkey.shape[0], np.uint64)
        np.add.at(hload, hinv.reshape(-1), w[rec[:, 0]])
        if not reuse:
            return self._link_loads_result(ex, load, hkey.reshape(-1, 2), hload)
        out = self._link_loads_result(ex, load, hkey.reshape(-1, 2), hload, _EntryLoads)
        ee = np.asarray(ee, np.int64)
        eg = np.repeat(np.arange(len(groups), dtype=np.int64), np.diff(eo))
        ent = np.unique(np.concatenate([np.stack([eg, esrc[ee], port[ee]], 1), rec]).reshape(-1, 3),
                        axis=0)
        dp = np.asarray(csr.dpids, np.int64)
        sums = {}
        for g, d, p in zip(ent[:, 0].tolist(), dp[ent[:, 1]].tolist(), ent[:, 2].tolist()):
            sums[(d, p)] = (sums.get((d, p), 0) + int(w[g])) & _U64
        out.entry_loads = {k: x for k, x in sums.items() if x}
        return out

    def mpi_bcast_entries(self, rank_to_mac, roots=None, route="default"):
        """The flow entries of MPI broadcasts with in-network replication: for
        every root rank of ``roots`` (default: every rank of ``rank_to_mac``)
        the multicast tree from its host to the hosts of all other ranks,
        grouped by switch as :meth:`switch_fdb_entries` lays entries out.

        Returns ``(dpids, off, root_rank, out_port, dst_rank)``: switch
        ``dpids[k]`` holds the entries ``off[k]:off[k+1]``; an entry forwards
        root ``root_rank[j]``'s broadcast out of ``out_port[j]``.  On a
        delivering entry -- a member's host port or OFPP_LOCAL, where the
        router would add SetDlDst (reference ``router.py:97-100``) --
        ``dst_rank[j]`` is the member rank, one entry per member rank (two
        ranks of one host give two); on a transit entry it is -1.  Switches
        ascend by dpid; within a switch the entries ascend by root rank, the
        transit entries (by port) before the delivering ones (by member rank).
        A rank whose MAC is the root's own, an unknown MAC and an unreachable
        host get no entry."""
        ranks = sorted(rank_to_mac)
        roots = ranks if roots is None else [r for r in roots if r in rank_to_mac]
        members = [[b for b in ranks if b != a] for a in roots]
        groups = [(rank_to_mac[a], [rank_to_mac[b] for b in ms]) for a, ms in zip(roots, members)]
        ex = self.graph()
        groups, rv, mg, mi, dv, last, moff, mv, inv = self._multicast_resolve(ex, groups)
        ng = len(groups)
        reach, eo, ee, _ = self._multicast_union(ex, rv, moff, mv, np.ones(ng, np.uint64), route,
                                                 True, False)
        ok = reach[inv] if inv.size else np.zeros(0, bool)
        csr = ex.csr
        esrc = np.repeat(np.arange(csr.V, dtype=np.int64), np.diff(np.asarray(csr.row_ptr, np.int64)))
        ee = np.asarray(ee, np.int64)
        eg = np.repeat(np.arange(ng, dtype=np.int64), np.diff(eo))
        root_r = np.asarray(roots, np.int64).reshape(-1)
        mrank = np.asarray([members[g][i] for g, i in zip(mg[ok].tolist(), mi[ok].tolist())],
                           np.int64)
        sw = np.concatenate([esrc[ee], dv[ok]])
        rr = np.concatenate([root_r[eg], root_r[mg[ok]]]) if ng else np.zeros(0, np.int64)
        pt = np.concatenate([np.asarray(csr.port, np.int64)[ee], last[ok]])
        dr = np.concatenate([np.full(ee.shape[0], -1, np.int64), mrank])
        order = np.lexsort((pt, dr, dr >= 0, rr, sw))
        sw, rr, pt, dr = sw[order], rr[order], pt[order], dr[order]
        cnt = np.bincount(sw, minlength=int(csr.V)) if sw.size else np.zeros(int(csr.V), np.int64)
        has = np.nonzero(cnt)[0]
        off = np.zeros(has.shape[0] + 1, np.int64)
        np.cumsum(cnt[has], out=off[1:])
        return np.asarray(csr.dpids, np.int64)[has], off, rr, pt.astype(np.int32), dr

    def mpi_bcast_link_loads(self, rank_to_mac, traffic=None, route="default"):
        """:meth:`multicast_link_loads` of an MPI job's broadcasts: ``traffic``
        = {root_rank: bytes} (a rank the map lacks is skipped); None: every
        rank broadcasts 1 -- MPI_Allgather as broadcasts.  Each root's group
        is the hosts of all other ranks."""
        ranks = sorted(rank_to_mac)
        if traffic is None:
            roots, weights = ranks, None
        else:
            roots = [r for r in traffic if r in rank_to_mac]
            weights = [traffic[r] for r in roots]
        groups = [(rank_to_mac[a], [rank_to_mac[b] for b in ranks if b != a]) for a in roots]
        return self.multicast_link_loads(groups, weights, route)

    # -- predicted link loads under ECMP ----------------------------------
    def _switch_pair_ecmp_loads(self, ex, sv, dv, w, split):
        """(load float64 [E], reach bool [n]) of switch pairs (dense ids sv ->
        dv, weights w u64) split over every shortest route: one
        sdnr_ecmp_link_loads call per budget-sized chunk of destination rows,
        over the pool's distance plane as it is (rows without pairs are
        skipped by the kernel)."""
        if split not in ("route", "hop"):
            raise ValueError("split must be 'route' or 'hop'")
        E = int(ex.csr.E)
        load = np.zeros(E, np.float64)
        reach = np.zeros(sv.shape[0], bool)
        if sv.size == 0:
            return load, reach
        c = self._cache
        store = c.sp
        want = sorted(set(dv.tolist()))
        batch = self._host_vertices(ex) if self._batch else ()
        step = max(1, store.cap() - 1) if store.row_bytes else len(want)
        for c0 in range(0, len(want), step):      # a budget's worth of rows at a time
            chunk = want[c0:c0 + step]
            tabs = c.sp_rows(self.engine, chunk, batch if c0 == 0 else ())
            mine = np.nonzero(np.isin(dv, np.asarray(chunk, np.int64)))[0]
            slots = np.asarray([store.row[v] for v in dv[mine].tolist()], np.int64)
            # the distance plane holds -1 (u16 0xFFFF as int16) where unreached
            reach[mine] = _gather(tabs[0], slots, sv[mine]) != -1
            load += self.engine.ecmp_link_loads(ex, tabs[0], slots, sv[mine], w[mine], split)
        return load, reach

    def ecmp_link_loads(self, pairs, weights=None, split="route"):
        """How much traffic crosses each link when every (src_mac, dst_mac)
        pair of ``pairs`` spreads ``weights[i]`` (non-negative ints; None: 1
        each) over ALL its shortest routes -- ECMP, what fat-trees,
        dragonflies and Jellyfish are sized for -- as a
        :class:`SplitLinkLoads`.

        Defining property: ``ecmp_link_loads(pairs, w).as_dict()[(dpid,
        port)]`` is the sum over i of ``w[i] / N_i`` times the number of
        routes in ``find_route(*pairs[i], multiple=True)`` that hold that
        entry, where N_i is the number of those routes (``split="route"``: a
        controller choosing uniformly among the routes).  ``split="hop"``
        instead halves, thirds, ... the traffic at every switch over its next
        hops (an OpenFlow select group per switch); the two differ where the
        routes are not spread evenly over the next hops.  Unknown hosts and
        unreachable pairs contribute nothing; repeated pairs add.  No route
        is enumerated and no count saturates (ecmp_loads.hip pushes the
        demand down the shortest-path DAG of each destination, O(links) per
        destination switch); link loads are float64 sums, equal to the
        definition within rounding (not bit-reproducible between runs), the
        last hops exact uint64."""
        return self._pair_loads(
            pairs, weights,
            lambda ex, sv, dv, w: self._switch_pair_ecmp_loads(ex, sv, dv, w, split),
            SplitLinkLoads)

    def all_pairs_ecmp_link_loads(self, split="route"):
        """:meth:`ecmp_link_loads` over every ordered pair of distinct hosts
        with weight 1, from the per-switch host counts (as
        :meth:`all_pairs_link_loads`)."""
        got = self._all_pairs_loads(
            lambda ex, sv, dv, w: self._switch_pair_ecmp_loads(ex, sv, dv, w, split),
            SplitLinkLoads)
        if got is None:
            macs = list(self.hosts)
            return self.ecmp_link_loads([(a, b) for a in macs for b in macs if a != b], None,
                                        split)
        return got

    def mpi_ecmp_link_loads(self, rank_to_mac, traffic=None, split="route"):
        """:meth:`ecmp_link_loads` of an MPI job (``traffic`` as in
        :meth:`mpi_link_loads`)."""
        pairs, weights = self._rank_pairs(rank_to_mac, traffic)
        return self.ecmp_link_loads(pairs, weights, split)

    # -- link costs and least-cost routes ---------------------------------
    def set_link_cost(self, src_dpid, dst_dpid, cost):
        """Cost of the directed link src_dpid -> dst_dpid for the least-cost
        routes (an OSPF / IS-IS style metric; default 1): an int in
        [1, 2**32 - 2], else ValueError.  Operator configuration, kept by dpid
        pair independently of ``links``: it applies whenever that link
        exists, so a flapping link keeps its cost.  ``find_route``,
        ``route_tables`` and the hop-count load methods ignore costs."""
        self.set_link_costs({(src_dpid, dst_dpid): cost})

    def set_link_costs(self, mapping):
        """:meth:`set_link_cost` for every {(src_dpid, dst_dpid): cost} of
        ``mapping``; nothing is set when one of them is refused."""
        items = list(dict(mapping).items())
        for k, c in items:
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or \
                    not 1 <= int(c) <= COST_MAX:
                raise ValueError("link cost of %r must be an int in [1, 2**32 - 2]: %r" % (k, c))
            if not isinstance(k, tuple) or len(k) != 2:
                raise ValueError("link costs are keyed by (src_dpid, dst_dpid): %r" % (k,))
        for k, c in items:
            self._link_costs[(k[0], k[1])] = int(c)
        self._cost_version += 1

    def link_cost(self, src_dpid, dst_dpid):
        """The cost set for src_dpid -> dst_dpid (1 when none was)."""
        return self._link_costs.get((src_dpid, dst_dpid), 1)

    def clear_link_costs(self):
        """Every link back to cost 1."""
        self._link_costs.clear()
        self._cost_version += 1

    def _cost_vector(self, ex):
        """uint32 [E]: the cost of every link of the export, CSR edge order."""
        got = self._cost_vec
        if got is not None and got[0] is ex and got[1] == self._cost_version:
            return got[2]
        csr = ex.csr
        cost = np.ones(int(csr.E), np.uint32)
        rp, col = csr.row_ptr, csr.col
        for (a, b), c in self._link_costs.items():
            u, v = ex.index.get(a), ex.index.get(b)
            if u is None or v is None:
                continue
            lo, hi = int(rp[u]), int(rp[u + 1])
            e = lo + int(np.searchsorted(col[lo:hi], v))
            if e < hi and int(col[e]) == v:
                cost[e] = c
        check_link_costs(csr, cost)      # the largest cost * (V - 1) stays below COST_INF
        self._cost_vec = (ex, self._cost_version, cost)
        return cost

    def _cost_rows(self, ex, want):
        """Memo of least-cost rows holding every destination of ``want`` (at
        most :meth:`_cost_cap` of them): dict(slot {destination: row}, pcost,
        nh, nh_port [n, V] tables as the engine returned them).  Rows are kept
        per destination until the graph or the costs change, or the table
        budget is exceeded; then the memo is dropped wholesale."""
        m = self._cost_memo
        if m is None or m["ex"] is not ex or m["version"] != self._cost_version:
            m = self._cost_memo = {"ex": ex, "version": self._cost_version, "slot": {},
                                   "tabs": None}
        new = [d for d in want if d not in m["slot"]]
        if not new:
            return m
        if len(m["slot"]) + len(new) > self._cost_cap(ex):
            m["slot"], m["tabs"] = {}, None
            new = list(want)
        tabs = tuple(self.engine.cost_tables(ex, self._cost_vector(ex), new))
        if isinstance(tabs[0], np.ndarray):         # u32 costs are held as int32: COST_INF is -1
            tabs = (np.ascontiguousarray(tabs[0], np.uint32).view(np.int32),) + tabs[1:]
        base = len(m["slot"])
        if m["tabs"] is None:
            m["tabs"] = tuple(tabs)
        elif isinstance(tabs[0], np.ndarray):
            m["tabs"] = tuple(np.concatenate([a, b]) for a, b in zip(m["tabs"], tabs))
        else:
            m["tabs"] = tuple(_torch().cat([a, b]) for a, b in zip(m["tabs"], tabs))
        for k, d in enumerate(new):
            m["slot"][d] = base + k
        return m

    def _cost_cap(self, ex):
        """Least-cost rows (12 bytes per vertex) the table budget holds."""
        budget = DEFAULT_TABLE_BUDGET if self._budget is None else self._budget
        return max(1, int(budget) // max(1, 12 * int(ex.csr.V)))

    def least_cost_tables(self, vertices=None):
        """Per-destination tables of the least-cost routes under the link
        costs (:meth:`set_link_cost`; cost_tables.hip) for every host-bearing
        switch, or the dense ``vertices`` given: dict(destinations, pcost
        uint32 [n, V] -- ``COST_INF`` 0xFFFFFFFF where there is no route --,
        nh, nh_port int32, dpids).  Following ``nh`` gives the
        lexicographically smallest least-cost route; with no cost set the
        tables are ``route_tables("shortest")``'s."""
        ex = self.graph()
        hv = self._host_vertices(ex) if vertices is None else [int(v) for v in vertices]
        V, n = int(ex.csr.V), len(hv)
        pcost = np.empty((n, V), np.uint32)
        nh = np.empty((n, V), np.int32)
        nhp = np.empty((n, V), np.int32)
        step = self._cost_cap(ex)
        for i in range(0, n, step):                 # a budget's worth of rows at a time
            chunk = hv[i:i + step]
            m = self._cost_rows(ex, sorted(set(chunk)))
            idx = np.asarray([m["slot"][v] for v in chunk], np.int64)
            p, a, b = (_host(_take(t, idx)) for t in m["tabs"])
            pcost[i:i + len(chunk)] = p.view(np.uint32)
            nh[i:i + len(chunk)] = a
            nhp[i:i + len(chunk)] = b
        return {"destinations": np.asarray(hv, np.int32), "pcost": pcost, "nh": nh,
                "nh_port": nhp, "dpids": ex.csr.dpids}

    def _least_cost_fdb(self, ex, s, d, last, rows):
        """fdb of the route that follows the next-hop row ``rows`` = (pcost,
        nh, nh_port host rows of destination d) from s; [] without a route."""
        pc, nh, nhp = rows
        if s != d and int(pc[s]) == -1:
            return []
        out, x, dpids = [], s, ex.csr.dpids
        while x != d:
            out.append((int(dpids[x]), int(nhp[x])))
            x = int(nh[x])
            if x < 0 or len(out) > int(ex.csr.V):
                raise RuntimeError("least-cost next-hop row is not an in-tree")
        out.append(last)
        return out

    def find_route_least_cost(self, src_mac, dst_mac, multiple=False):
        """The least-cost route between two hosts (or switch-local ports)
        under the link costs, in ``find_route``'s format and with its endpoint
        rules: [] for an unknown MAC or an unreachable destination, the one
        last-hop entry for two endpoints on one switch.  Among equal-cost
        routes the lexicographically smallest dpid sequence, the tie rule of
        ``find_route(multiple=True)[0]`` -- which it equals while every cost
        is 1.  With ``multiple=True`` the list of EVERY least-cost route, in
        ``find_route(multiple=True)``'s format and order (lexicographic dpid
        sequences; [] where the single form returns []): the ECMP set an OSPF
        fabric balances over, and ``find_route(multiple=True)`` itself while
        every cost is 1."""
        return self.find_routes_least_cost([(src_mac, dst_mac)], multiple)[0]

    def find_routes_least_cost(self, pairs, multiple=False):
        """:meth:`find_route_least_cost` over many (src_mac, dst_mac) pairs;
        the destination rows are computed once for all of them."""
        pairs = list(pairs)
        ex = self.graph()
        out = [[] for _ in pairs]
        ends = {}
        for i, (a, b) in enumerate(pairs):
            ea, eb = self._endpoint(a), self._endpoint(b)
            if ea is None or eb is None:
                continue
            ends[i] = (ex.index[ea[0]], ex.index[eb[0]], self._last_hop(eb[0], eb[1], b))
        want = sorted(set(e[1] for e in ends.values()))
        step = self._cost_cap(ex)
        cost = self._cost_vector(ex) if multiple and want else None
        for c0 in range(0, len(want), step):        # a budget's worth of rows at a time
            chunk = want[c0:c0 + step]
            m = self._cost_rows(ex, chunk)
            idx = np.asarray([m["slot"][d] for d in chunk], np.int64)
            host = [_host(_take(t, idx)) for t in m["tabs"]]
            at = {d: k for k, d in enumerate(chunk)}
            for i, (s, d, last) in ends.items():
                if d in at and multiple:
                    seqs = least_cost_paths_lex(ex.csr.row_ptr, ex.csr.col, cost,
                                                host[0][at[d]], s, d)
                    out[i] = [self._seq_fdb(ex, q, last) for q in seqs]
                elif d in at:
                    k = at[d]
                    out[i] = self._least_cost_fdb(ex, s, d, last,
                                                  (host[0][k].view(np.int32), host[1][k],
                                                   host[2][k]))
        return out

    # -- loop-free alternates (fast reroute) -------------------------------
    def _lfa_rows(self, ex, node_protect=True):
        """(backup, backup_port, kind [V, V] tables as the engine returned
        them, row d = destination d; counts uint32 [V, 4] on the host) of every
        destination, kept in the least-cost memo: dropped with it when the
        export or the costs change."""
        V = int(ex.csr.V)
        if V > LFA_MAX_V:
            raise ValueError("loop-free alternates need the all-pairs least-cost table: %d "
                             "switches are above the %d it is computed for" % (V, LFA_MAX_V))
        if V > self._cost_cap(ex):
            raise ValueError("loop-free alternates need the all-pairs least-cost table: %d x %d "
                             "rows of 12 bytes per vertex do not fit the table budget" % (V, V))
        m = self._cost_rows(ex, [])
        if "pall" not in m:
            # (pcost, nh) [V, V] with row d = destination d, out of the memo's slots
            m = self._cost_rows(ex, list(range(V)))
            idx = np.asarray([m["slot"][v] for v in range(V)], np.int64)
            same = len(m["slot"]) == V and np.array_equal(idx, np.arange(V))
            m["pall"] = tuple(t if same else _take(t, idx) for t in m["tabs"][:2])
        lfa = m.setdefault("lfa", {})
        key = bool(node_protect)
        if key not in lfa:
            lfa[key] = tuple(self.engine.lfa_tables(ex, self._cost_vector(ex), m["pall"][0],
                                                    np.arange(V, dtype=np.int32),
                                                    link_only=not key))
        return lfa[key]

    def lfa_tables(self, vertices=None, node_protect=True):
        """Loop-free alternate (RFC 5286 fast-reroute) next hops under the link
        costs (lfa_tables.hip) toward every host-bearing switch, or the dense
        ``vertices`` given: dict(destinations, backup, backup_port int32
        [n, V] -- -1 where a switch has no primary or no alternate toward that
        destination --, kind uint8 [n, V] with bits 1 = an alternate exists, 2 =
        it is downstream (strictly closer to the destination), 4 = it is
        node-protecting (avoids the primary next hop too), dpids).  The primary
        is ``least_cost_tables``' ``nh``.  ``node_protect=False``: the cheapest
        link-protecting alternate, node protection not evaluated.  Needs the
        all-pairs least-cost table (reused from the least-cost memo): a
        ValueError above 16,384 switches or when it does not fit the table
        budget."""
        ex = self.graph()
        hv = self._host_vertices(ex) if vertices is None else [int(v) for v in vertices]
        b, bp, k, _ = self._lfa_rows(ex, node_protect)
        idx = np.asarray(hv, np.int64)
        return {"destinations": np.asarray(hv, np.int32), "backup": _host(_take(b, idx)),
                "backup_port": _host(_take(bp, idx)), "kind": _host(_take(k, idx)),
                "dpids": ex.csr.dpids}

    def find_route_protected(self, src_mac, dst_mac):
        """``find_route_least_cost``'s route with the fast-failover bucket of
        every hop: a list of (dpid, out_port, backup_port, kind) -- the port
        of the switch's loop-free alternate toward the destination switch and
        its ``lfa_tables`` kind bits, or (None, 0) where it has none and at the
        last hop (the host port).  [] where there is no route."""
        return self.find_routes_protected([(src_mac, dst_mac)])[0]

    def find_routes_protected(self, pairs):
        """:meth:`find_route_protected` over many (src_mac, dst_mac) pairs."""
        pairs = list(pairs)
        routes = self.find_routes_least_cost(pairs)
        if not any(routes):
            return [[] for _ in routes]
        ex = self.graph()
        _, bp, k, _ = self._lfa_rows(ex)
        want = sorted(set(ex.index[r[-1][0]] for r in routes if r))
        idx = np.asarray(want, np.int64)
        hbp, hk = _host(_take(bp, idx)), _host(_take(k, idx))
        at = {d: i for i, d in enumerate(want)}
        out = []
        for r in routes:
            hops = []
            if r:
                row = at[ex.index[r[-1][0]]]
                for dpid, op in r[:-1]:
                    s = ex.index[dpid]
                    kd = int(hk[row, s])
                    hops.append((dpid, op, int(hbp[row, s]) if kd else None, kd))
                hops.append((r[-1][0], r[-1][1], None, 0))
            out.append(hops)
        return out

    def lfa_coverage(self, node_protect=True):
        """How much of the fabric a fast-failover deployment protects, over
        all destinations: dict(primaries -- the (switch, destination) pairs
        that forward at all --, backups, node_protecting, downstream, and the
        fractions coverage = backups / primaries, node_coverage,
        downstream_coverage; 0.0 on a fabric without primaries)."""
        ex = self.graph()
        tot = self._lfa_rows(ex, node_protect)[3].astype(np.int64).sum(axis=0)
        n = [int(x) for x in tot]
        frac = (lambda a: float(a) / n[0] if n[0] else 0.0)
        return {"primaries": n[0], "backups": n[1], "node_protecting": n[2], "downstream": n[3],
                "coverage": frac(n[1]), "node_coverage": frac(n[2]),
                "downstream_coverage": frac(n[3])}

    def unprotected_links(self):
        """{(src_dpid, dst_dpid): number of destinations whose primary next hop
        is this link and has no loop-free alternate}, links with none omitted:
        the cables a fast-failover deployment cannot cover."""
        ex = self.graph()
        V = int(ex.csr.V)
        kind = _host(self._lfa_rows(ex)[2])
        nh = _host(self._cost_memo["pall"][1])
        dd, ss = np.nonzero((nh >= 0) & ((kind & 1) == 0))
        keys, n = np.unique(ss.astype(np.int64) * V + nh[dd, ss], return_counts=True)
        dpids = ex.csr.dpids
        return {(int(dpids[q // V]), int(dpids[q % V])): int(c) for q, c in zip(keys, n)}

    # -- remote loop-free alternates (PQ-node repair tunnels) ----------------
    def _remote_lfa_rows(self, ex):
        """(pq, via, via_port, tunnel_cost, kind [E], counts [V, 4]) of every
        link, on the host, kept in the least-cost memo beside the LFA tables
        and dropped with them; :meth:`_lfa_rows`' ValueErrors."""
        self._lfa_rows(ex, node_protect=False)      # the checks, the all-pairs table
        m = self._cost_memo
        if "rlfa" not in m:
            m["rlfa"] = tuple(self.engine.remote_lfa(ex, self._cost_vector(ex), m["pall"][0]))
        return m["rlfa"]

    def remote_lfa_tables(self):
        """Remote loop-free alternates (RFC 7490) under the link costs
        (remote_lfa.hip), one repair per directed link e = (src -> dst): dict(pq
        -- the PQ node the packet is tunnelled to --, via -- the neighbour it
        leaves through --, via_port int32 [E], -1 where the link has no repair;
        tunnel_cost uint64 [E] -- the cost src -> via -> pq --; kind uint8 [E]
        with bits 1 = a repair exists, 2 = pq is in src's own P-space (an
        ordinary tunnel reaches it), 4 = pq is via itself (a per-link
        loop-free alternate, no tunnel); src, dst int32 [E] dense; dpids).
        Needs the all-pairs least-cost table as :meth:`lfa_tables` does (the
        same ValueErrors)."""
        ex = self.graph()
        pq, via, vp, tc, k, _ = self._remote_lfa_rows(ex)
        csr = ex.csr
        src = np.repeat(np.arange(int(csr.V), dtype=np.int32), np.diff(csr.row_ptr))
        return {"pq": pq, "via": via, "via_port": vp, "tunnel_cost": tc, "kind": k, "src": src,
                "dst": np.asarray(csr.col, np.int32), "dpids": csr.dpids}

    def repair_tunnels(self):
        """{(src_dpid, dst_dpid): (pq_dpid, via_dpid, via_port, tunnel_cost,
        kind)} of every link with a repair (:meth:`remote_lfa_tables`)."""
        t = self.remote_lfa_tables()
        d = t["dpids"]
        return {(int(d[t["src"][e]]), int(d[t["dst"][e]])):
                (int(d[t["pq"][e]]), int(d[t["via"][e]]), int(t["via_port"][e]),
                 int(t["tunnel_cost"][e]), int(t["kind"][e]))
                for e in np.nonzero(t["kind"] & 1)[0].tolist()}

    def remote_lfa_coverage(self):
        """What remote LFA adds to ``lfa_coverage(node_protect=False)``:
        dict(primaries, backups -- as there --, remote_backups -- the primaries
        without a loop-free alternate whose primary link has a repair --,
        coverage_with_remote = (backups + remote_backups) / primaries (0.0
        without primaries), links -- the links that are no self-loops --,
        links_repaired, links_plain -- those whose PQ node needs no directed
        forwarding)."""
        ex = self.graph()
        V = int(ex.csr.V)
        _, _, _, _, k, counts = self._remote_lfa_rows(ex)
        lk = _host(self._lfa_rows(ex, node_protect=False)[2])
        cov = self.lfa_coverage(node_protect=False)
        nh = _host(self._cost_memo["pall"][1])
        dd, ss = np.nonzero((nh >= 0) & ((lk & 1) == 0))
        keys, _ = _edge_keys_host(ex.csr)
        e = np.searchsorted(keys, ss.astype(np.int64) * V + nh[dd, ss])
        remote = int((k[e] & 1).sum()) if e.size else 0
        tot = counts.astype(np.int64).sum(axis=0)
        prim = cov["primaries"]
        return {"primaries": prim, "backups": cov["backups"], "remote_backups": remote,
                "coverage_with_remote": float(cov["backups"] + remote) / prim if prim else 0.0,
                "links": int(tot[0]), "links_repaired": int(tot[1]), "links_plain": int(tot[2])}

    def unrepaired_links(self):
        """:meth:`unprotected_links` restricted to the links without a remote
        repair either: the cables neither a loop-free alternate nor a PQ-node
        tunnel covers."""
        fixed = self.repair_tunnels()
        return {key: c for key, c in self.unprotected_links().items() if key not in fixed}

    def _switch_pair_cost_loads(self, ex, sv, dv, w):
        """(load uint64 [E], reach bool [n]) of switch pairs (dense ids sv ->
        dv, weights w u64) on their least-cost routes: sdnr_link_loads with
        SDNR_LOADS_TO_ROOT over the least-cost next-hop rows, a budget-sized
        chunk of destination rows at a time."""
        E = int(ex.csr.E)
        load = np.zeros(E, np.uint64)
        reach = np.zeros(sv.shape[0], bool)
        if sv.size == 0:
            return load, reach
        want = sorted(set(dv.tolist()))
        step = self._cost_cap(ex)
        for c0 in range(0, len(want), step):
            chunk = want[c0:c0 + step]
            m = self._cost_rows(ex, chunk)
            mine = np.nonzero(np.isin(dv, np.asarray(chunk, np.int64)))[0]
            slots = np.asarray([m["slot"][v] for v in dv[mine].tolist()], np.int64)
            pc, nh = m["tabs"][0], m["tabs"][1]
            # pcost is held as int32: COST_INF reads -1
            reach[mine] = _gather(pc, slots, sv[mine]) != -1
            urows, inv = np.unique(slots, return_inverse=True)
            load += self.engine.link_loads(ex, _take(nh, urows), INT32, inv, sv[mine], w[mine],
                                           to_root=True)
        return load, reach

    def least_cost_link_loads(self, pairs, weights=None):
        """:meth:`link_loads` with every pair on its least-cost route
        (:meth:`find_route_least_cost`) -- what the links would carry after
        the costs were changed: ``as_dict()`` is the weighted count of the
        ``(dpid, out_port)`` entries of those routes.  Exact uint64 sums."""
        return self._pair_loads(pairs, weights, self._switch_pair_cost_loads, LinkLoads)

    def all_pairs_least_cost_link_loads(self):
        """:meth:`least_cost_link_loads` over every ordered pair of distinct
        hosts with weight 1, from the per-switch host counts (as
        :meth:`all_pairs_link_loads`)."""
        got = self._all_pairs_loads(self._switch_pair_cost_loads, LinkLoads)
        if got is None:
            macs = list(self.hosts)
            return self.least_cost_link_loads([(a, b) for a in macs for b in macs if a != b])
        return got

    def mpi_least_cost_link_loads(self, rank_to_mac, traffic=None):
        """:meth:`least_cost_link_loads` of an MPI job (``traffic`` as in
        :meth:`mpi_link_loads`)."""
        pairs, weights = self._rank_pairs(rank_to_mac, traffic)
        return self.least_cost_link_loads(pairs, weights)

    # -- link utilisation and least-loaded routes ---------------------------
    def set_link_utilisation(self, src_dpid, dst_dpid, value):
        """Utilisation of the directed link src_dpid -> dst_dpid for the
        least-loaded routes (what the port counters measured, in any unit;
        default 0): an int in [0, 2**32 - 2], else ValueError.  Monitor data,
        kept by dpid pair independently of ``links`` as the costs are: it
        applies whenever that link exists, so a flapping link keeps its
        figure.  Only the ``least_loaded`` methods and ``admit_flows`` read
        it."""
        self.set_link_utilisations({(src_dpid, dst_dpid): value})

    @staticmethod
    def _checked_utilisations(mapping, what):
        items = list(dict(mapping).items())
        for k, x in items:
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or \
                    not 0 <= int(x) <= UTIL_MAX:
                raise ValueError("link utilisation of %r must be an int in [0, 2**32 - 2]: %r"
                                 % (k, x))
            if not isinstance(k, tuple) or len(k) != 2:
                raise ValueError("link utilisations are keyed by %s: %r" % (what, k))
        return items

    def set_link_utilisations(self, mapping):
        """:meth:`set_link_utilisation` for every {(src_dpid, dst_dpid):
        value} of ``mapping``; nothing is set when one of them is refused."""
        for k, x in self._checked_utilisations(mapping, "(src_dpid, dst_dpid)"):
            self._link_utils[(k[0], k[1])] = int(x)
        self._util_version += 1

    def set_port_utilisations(self, mapping):
        """:meth:`set_link_utilisations` keyed as the Monitor keys its port
        statistics: {(dpid, port_no): value}, resolved to the link whose
        source port it is (``links[dpid][*].src.port_no``).  Ports that are no
        link's source (host ports, unknown switches) are ignored; nothing is
        set when one value is refused."""
        items = self._checked_utilisations(mapping, "(dpid, port_no)")
        by_port = {(a, lk.src.port_no): (a, b) for a, nb in self.links.items()
                   for b, lk in nb.items()}
        self.set_link_utilisations({by_port[k]: x for k, x in items if k in by_port})

    def link_utilisation(self, src_dpid, dst_dpid):
        """The utilisation set for src_dpid -> dst_dpid (0 when none was)."""
        return self._link_utils.get((src_dpid, dst_dpid), 0)

    def clear_link_utilisations(self):
        """Every link back to utilisation 0."""
        self._link_utils.clear()
        self._util_version += 1

    def _util_vector(self, ex):
        """uint32 [E]: the utilisation of every link of the export, CSR edge order."""
        got = self._util_vec
        if got is not None and got[0] is ex and got[1] == self._util_version:
            return got[2]
        util = np.zeros(int(ex.csr.E), np.uint32)
        for (a, b), x in self._link_utils.items():
            e = self._link_edge(ex, a, b)
            if e is not None:
                util[e] = x
        self._util_vec = (ex, self._util_version, util)
        return util

    def _widest_cap(self, ex):
        """Destinations per engine call: the least-cost rows and the
        least-loaded rows of a chunk (12 bytes per vertex each) fit the table
        budget together."""
        budget = DEFAULT_TABLE_BUDGET if self._budget is None else self._budget
        return max(1, int(budget) // max(1, 24 * int(ex.csr.V)))

    def _widest_compute(self, ex, dsts, util):
        """(bott, nh, nh_port) [n, V] as the engine returns them -- bott held
        as int32, -1: no route -- of the distinct destinations ``dsts`` (at
        most :meth:`_widest_cap`) under the utilisation vector ``util``; the
        least-cost rows come from the least-cost memo."""
        m = self._cost_rows(ex, dsts)
        idx = np.asarray([m["slot"][d] for d in dsts], np.int64)
        tabs = tuple(self.engine.widest_tables(ex, self._cost_vector(ex), _take(m["tabs"][0], idx),
                                               util, dsts))
        if isinstance(tabs[0], np.ndarray):
            tabs = (np.ascontiguousarray(tabs[0], np.uint32).view(np.int32),) + tabs[1:]
        return tabs

    def _widest_rows(self, ex, want):
        """Memo of least-loaded rows holding every destination of ``want`` (at
        most :meth:`_widest_cap` of them), in :meth:`_cost_rows`' form: kept
        until the graph, the costs or the utilisation change, or the table
        budget is exceeded."""
        m = self._util_memo
        key = (self._cost_version, self._util_version)
        if m is None or m["ex"] is not ex or m["version"] != key:
            m = self._util_memo = {"ex": ex, "version": key, "slot": {}, "tabs": None}
        new = [d for d in want if d not in m["slot"]]
        if not new:
            return m
        if len(m["slot"]) + len(new) > self._widest_cap(ex):
            m["slot"], m["tabs"] = {}, None
            new = list(want)
        tabs = self._widest_compute(ex, new, self._util_vector(ex))
        base = len(m["slot"])
        if m["tabs"] is None:
            m["tabs"] = tabs
        elif isinstance(tabs[0], np.ndarray):
            m["tabs"] = tuple(np.concatenate([a, b]) for a, b in zip(m["tabs"], tabs))
        else:
            m["tabs"] = tuple(_torch().cat([a, b]) for a, b in zip(m["tabs"], tabs))
        for k, d in enumerate(new):
            m["slot"][d] = base + k
        return m

    def least_loaded_tables(self, vertices=None):
        """Per-destination tables of the least-loaded routes (widest_tables
        .hip): inside the least-cost routes under the link costs, the route
        whose busiest link has the smallest utilisation (:meth:`set_link_
        utilisation`), for every host-bearing switch or the dense ``vertices``
        given: dict(destinations, bott uint32 [n, V] -- the utilisation of
        that busiest link, 0xFFFFFFFF where there is no route --, nh, nh_port
        int32, dpids).  ``nh`` is the tight link of the smallest (bottleneck,
        utilisation of the link itself, neighbour); with no utilisation set
        the tables are :meth:`least_cost_tables`'."""
        ex = self.graph()
        hv = self._host_vertices(ex) if vertices is None else [int(v) for v in vertices]
        V, n = int(ex.csr.V), len(hv)
        bott = np.empty((n, V), np.uint32)
        nh = np.empty((n, V), np.int32)
        nhp = np.empty((n, V), np.int32)
        step = self._widest_cap(ex)
        for i in range(0, n, step):                 # a budget's worth of rows at a time
            chunk = hv[i:i + step]
            m = self._widest_rows(ex, sorted(set(chunk)))
            idx = np.asarray([m["slot"][v] for v in chunk], np.int64)
            b, a, p = (_host(_take(t, idx)) for t in m["tabs"])
            bott[i:i + len(chunk)] = b.view(np.uint32)
            nh[i:i + len(chunk)] = a
            nhp[i:i + len(chunk)] = p
        return {"destinations": np.asarray(hv, np.int32), "bott": bott, "nh": nh,
                "nh_port": nhp, "dpids": ex.csr.dpids}

    def find_route_least_loaded(self, src_mac, dst_mac):
        """The least-loaded route between two hosts (or switch-local ports):
        of the least-cost routes the one whose busiest link is the least
        utilised, in ``find_route``'s format and with its endpoint rules.
        Always one of ``find_route_least_cost(..., multiple=True)``, and
        ``find_route_least_cost(...)`` itself while no utilisation is set."""
        return self.find_routes_least_loaded([(src_mac, dst_mac)])[0]

    def find_routes_least_loaded(self, pairs):
        """:meth:`find_route_least_loaded` over many (src_mac, dst_mac) pairs;
        the destination rows are computed once for all of them."""
        pairs = list(pairs)
        ex = self.graph()
        out = [[] for _ in pairs]
        ends = {}
        for i, (a, b) in enumerate(pairs):
            ea, eb = self._endpoint(a), self._endpoint(b)
            if ea is None or eb is None:
                continue
            ends[i] = (ex.index[ea[0]], ex.index[eb[0]], self._last_hop(eb[0], eb[1], b))
        want = sorted(set(e[1] for e in ends.values()))
        step = self._widest_cap(ex)
        for c0 in range(0, len(want), step):        # a budget's worth of rows at a time
            chunk = want[c0:c0 + step]
            m = self._widest_rows(ex, chunk)
            idx = np.asarray([m["slot"][d] for d in chunk], np.int64)
            host = [_host(_take(t, idx)) for t in m["tabs"]]
            at = {d: k for k, d in enumerate(chunk)}
            for i, (s, d, last) in ends.items():
                if d in at:
                    k = at[d]
                    out[i] = self._least_cost_fdb(ex, s, d, last,
                                                  (host[0][k], host[1][k], host[2][k]))
        return out

    def _switch_pair_widest_loads(self, ex, sv, dv, w, util=None, rows_out=None):
        """(load uint64 [E], reach bool [n]) of switch pairs (dense ids sv ->
        dv, weights w u64) on their least-loaded routes: sdnr_link_loads with
        SDNR_LOADS_TO_ROOT over the least-loaded next-hop rows, a budget-sized
        chunk of destination rows at a time.  ``util``: a utilisation vector
        in place of the one set (its rows are not memoised); ``rows_out``: a
        dict that receives {destination: (bott, nh, nh_port) host rows}."""
        E = int(ex.csr.E)
        load = np.zeros(E, np.uint64)
        reach = np.zeros(sv.shape[0], bool)
        if sv.size == 0:
            return load, reach
        want = sorted(set(dv.tolist()))
        step = self._widest_cap(ex)
        for c0 in range(0, len(want), step):
            chunk = want[c0:c0 + step]
            if util is None:
                m = self._widest_rows(ex, chunk)
                slot, tabs = m["slot"], m["tabs"]
            else:
                slot, tabs = {d: k for k, d in enumerate(chunk)}, self._widest_compute(ex, chunk,
                                                                                       util)
            mine = np.nonzero(np.isin(dv, np.asarray(chunk, np.int64)))[0]
            slots = np.asarray([slot[v] for v in dv[mine].tolist()], np.int64)
            # bott is held as int32: no route reads -1
            reach[mine] = _gather(tabs[0], slots, sv[mine]) != -1
            urows, inv = np.unique(slots, return_inverse=True)
            load += self.engine.link_loads(ex, _take(tabs[1], urows), INT32, inv, sv[mine],
                                           w[mine], to_root=True)
            if rows_out is not None:
                idx = np.asarray([slot[d] for d in chunk], np.int64)
                host = [_host(_take(t, idx)) for t in tabs]
                for k, d in enumerate(chunk):
                    rows_out[d] = (host[0][k], host[1][k], host[2][k])
        return load, reach

    def least_loaded_link_loads(self, pairs, weights=None):
        """:meth:`link_loads` with every pair on its least-loaded route
        (:meth:`find_route_least_loaded`) under the utilisation as set -- what
        the pairs add to the links if all of them are routed on the tables as
        they stand: ``as_dict()`` is the weighted count of the ``(dpid,
        out_port)`` entries of those routes.  Exact uint64 sums."""
        return self._pair_loads(pairs, weights, self._switch_pair_widest_loads, LinkLoads)

    def mpi_least_loaded_link_loads(self, rank_to_mac, traffic=None):
        """:meth:`least_loaded_link_loads` of an MPI job (``traffic`` as in
        :meth:`mpi_link_loads`)."""
        pairs, weights = self._rank_pairs(rank_to_mac, traffic)
        return self.least_loaded_link_loads(pairs, weights)

    # -- admission: the flows of a job, routed round by round ---------------
    def _int_capacity_vector(self, ex, capacity):
        """uint64 [E] capacities in CSR edge order from one int for every link
        or ``{(src_dpid, dst_dpid): int}`` (links not named: 1; links that do
        not exist are ignored), each in [1, 2**53]; None when none is given."""
        if capacity is None:
            return None

        def checked(key, x):
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or \
                    not 1 <= int(x) <= CAPACITY_MAX:
                raise ValueError("capacity of %r must be an int in [1, 2**53]: %r" % (key, x))
            return int(x)

        E = int(ex.csr.E)
        if not hasattr(capacity, "items") and not hasattr(capacity, "__iter__"):
            return np.full(E, checked("every link", capacity), np.uint64)
        cap = np.ones(E, np.uint64)
        for key, x in dict(capacity).items():
            if not isinstance(key, tuple) or len(key) != 2:
                raise ValueError("capacities are keyed by (src_dpid, dst_dpid): %r" % (key,))
            x = checked(key, x)
            e = self._link_edge(ex, key[0], key[1])
            if e is not None:
                cap[e] = x
        return cap

    @staticmethod
    def _admission_util(base, admitted, cap):
        """uint32 [E]: min(base + min(u(admitted), UTIL_MAX), UTIL_MAX) with
        u(load) = load * 1024 // capacity, or the load itself without
        capacities -- in 64-bit integers that cannot wrap."""
        top = np.uint64(UTIL_MAX)
        if cap is None:
            a = np.minimum(admitted, top)
        else:
            # load = q * cap + r: load * 1024 // cap = q * 1024 + r * 1024 // cap
            q, r = admitted // cap, admitted % cap
            a = np.minimum(np.minimum(q, top) * np.uint64(1024) + r * np.uint64(1024) // cap, top)
        return np.minimum(base.astype(np.uint64) + a, top).astype(np.uint32)

    def _peak(self, ex, load, cap):
        """(peak, link): the largest load[e] (load[e] * 1024 // capacity[e]
        with capacities) as a Python int and the first link (src_dpid,
        dst_dpid) that attains it; (0, None) on a fabric without links."""
        vals = load.tolist()
        if cap is not None:
            vals = [x * 1024 // c for x, c in zip(vals, cap.tolist())]
        if not vals:
            return 0, None
        peak = max(vals)
        return peak, self._edge_links(ex)(vals.index(peak))

    @staticmethod
    def _admission_slices(dv, pos, n, batch):
        """Index arrays into the known pairs, one per round: ``batch`` None --
        the pairs of one destination switch, the switches in order of first
        appearance; else the known ones of each ``batch`` consecutive pairs of
        the list as given (``pos``: the known pairs' positions in it, ``n``
        its length)."""
        if batch is None:
            perm = np.argsort(dv, kind="stable")
            cut = np.nonzero(np.diff(dv[perm]))[0] + 1
            groups = [g for g in np.split(perm, cut) if g.size]
            return sorted(groups, key=lambda g: int(g[0]))
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or int(batch) < 1:
            raise ValueError("batch is a positive number of pairs per round, or None")
        cuts = np.searchsorted(pos, np.arange(0, n + int(batch), int(batch)))
        return [np.arange(a, b) for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist())]

    def _admit(self, ex, sv, dv, w, slices, cap, rows_out=None):
        """(admitted load uint64 [E], reach bool per pair) of pairs (dense
        switches sv -> dv, weights w u64) admitted slice by slice: each slice
        is routed on the least-loaded tables under the utilisation as set plus
        what the earlier slices put on the links.  ``rows_out``: a list that
        receives, per slice, {destination: (bott, nh, nh_port) host rows}."""
        V = max(1, int(ex.csr.V))
        base = self._util_vector(ex)
        admitted = np.zeros(int(ex.csr.E), np.uint64)
        reach = np.zeros(sv.shape[0], bool)
        want = sorted(set(dv.tolist()))
        if 0 < len(want) <= self._cost_cap(ex):
            self._cost_rows(ex, want)               # the least-cost rows of every round, once
        for sl in slices:
            rows = None if rows_out is None else {}
            if sl.size:
                # the slice's pairs summed to switch pairs
                key, inv = np.unique(sv[sl] * V + dv[sl], return_inverse=True)
                inv = inv.reshape(-1)
                sw = np.zeros(key.shape[0], np.uint64)
                np.add.at(sw, inv, w[sl])
                load, got = self._switch_pair_widest_loads(
                    ex, key // V, key % V, sw, self._admission_util(base, admitted, cap), rows)
                admitted += load
                reach[sl] = got[inv]
            if rows_out is not None:
                rows_out.append(rows)
        return admitted, reach

    def admit_flows(self, pairs, weights=None, capacity=None, batch=None, routes=False):
        """Admit the flows of ``pairs`` (weights as in :meth:`link_loads`) in
        order, a slice at a time, every slice on its least-loaded routes under
        what the links carry by then -- the routes a controller would install
        if it looked at its port counters before each batch of flows -- and
        return an :class:`Admission`.

        Slices: ``batch`` consecutive pairs of the list each; by default
        (``batch=None``) one slice per distinct destination switch, the
        switches in order of first appearance in ``pairs`` (the pairs of a
        slice share their destination row, so a round is one row of tables).
        A slice is routed on the least-loaded tables (:meth:`least_loaded_
        tables`' rule) under ``util = min(base + u(admitted), 2**32 - 2)``:
        ``base`` the utilisation as set, ``admitted`` the exact uint64 link
        loads of the slices before it, and ``u(load) = min(load * 1024 //
        capacity[e], 2**32 - 2)`` with ``capacity`` -- one int for every link
        or ``{(src_dpid, dst_dpid): int}``, links not named 1, each in
        [1, 2**53] -- or ``min(load, 2**32 - 2)`` without.  All in integers.
        One slice holding everything is :meth:`least_loaded_link_loads`; one
        pair per slice is greedy sequential admission.

        Every route stays least-cost, so the total carried load equals that of
        :meth:`least_cost_link_loads`; only the peak moves.  Nothing of this
        object changes: not ``links``, the costs, the utilisation as set, the
        least-loaded tables or the graph on the GPU.  Only the destination
        rows a slice needs are computed for it (widest_tables.hip, then the
        loads kernel over its next-hop rows)."""
        pairs = list(pairs)
        weights = None if weights is None else list(weights)
        ex = self.graph()
        cap = self._int_capacity_vector(ex, capacity)
        w, dv, last, ok, inv, ssv, sdv, _ = self._switch_pairs(ex, pairs, weights)
        sv_ok, dv_ok, w_ok = ssv[inv.reshape(-1)], sdv[inv.reshape(-1)], w[ok]
        slices = self._admission_slices(dv_ok, ok, len(pairs), batch)
        rows = [] if routes else None
        load, reach = self._admit(ex, sv_ok, dv_ok, w_ok, slices, cap, rows)
        got = ok[reach]
        hkey, hinv = np.unique(np.stack([dv[got], last[got]], 1), axis=0, return_inverse=True)
        hload = np.zeros(hkey.shape[0], np.uint64)
        np.add.at(hload, hinv.reshape(-1), w[got])
        fdbs = None
        if routes:
            fdbs = [[] for _ in pairs]
            for sl, tabs in zip(slices, rows):
                for k in sl.tolist():
                    i, d = int(ok[k]), int(dv_ok[k])
                    b = pairs[i][1]
                    eb = self._endpoint(b)
                    fdbs[i] = self._least_cost_fdb(ex, int(sv_ok[k]), d,
                                                   self._last_hop(eb[0], eb[1], b), tabs[d])
        before = self.least_cost_link_loads(pairs, weights)
        pb, lb = self._peak(ex, before.load, cap)
        pa, la = self._peak(ex, load, cap)
        return Admission(self._link_loads_result(ex, load, hkey.reshape(-1, 2), hload), pb, lb,
                         pa, la, int(w_ok[~reach].sum(dtype=np.uint64)), len(slices), fdbs)

    def mpi_admit_flows(self, rank_to_mac, traffic=None, capacity=None, batch=None, routes=False):
        """:meth:`admit_flows` of an MPI job (``traffic`` as in
        :meth:`mpi_link_loads`)."""
        pairs, weights = self._rank_pairs(rank_to_mac, traffic)
        return self.admit_flows(pairs, weights, capacity, batch, routes)

    # -- ECMP over the least-cost routes ----------------------------------
    def _switch_pair_cost_ecmp_loads(self, ex, sv, dv, w, split):
        """(load float64 [E], reach bool [n]) of switch pairs (dense ids sv ->
        dv, weights w u64) split over every least-cost route: one
        sdnr_cost_ecmp_link_loads call per budget-sized chunk of destination
        rows, over the memoised pcost plane as it is (rows without pairs are
        skipped by the kernel)."""
        if split not in ("route", "hop"):
            raise ValueError("split must be 'route' or 'hop'")
        E = int(ex.csr.E)
        load = np.zeros(E, np.float64)
        reach = np.zeros(sv.shape[0], bool)
        if sv.size == 0:
            return load, reach
        want = sorted(set(dv.tolist()))
        step = self._cost_cap(ex)
        cost = self._cost_vector(ex)
        for c0 in range(0, len(want), step):
            chunk = want[c0:c0 + step]
            m = self._cost_rows(ex, chunk)
            mine = np.nonzero(np.isin(dv, np.asarray(chunk, np.int64)))[0]
            slots = np.asarray([m["slot"][v] for v in dv[mine].tolist()], np.int64)
            pc = m["tabs"][0]
            # pcost is held as int32: COST_INF reads -1
            reach[mine] = _gather(pc, slots, sv[mine]) != -1
            load += self.engine.cost_ecmp_link_loads(ex, cost, pc, slots, sv[mine], w[mine],
                                                     split)
        return load, reach

    def least_cost_ecmp_link_loads(self, pairs, weights=None, split="route"):
        """:meth:`ecmp_link_loads` under the link costs: every (src_mac,
        dst_mac) pair spreads ``weights[i]`` over ALL its least-cost routes --
        what the links carry once a link is costed up and the traffic spreads
        over the surviving equal-cost routes -- as a :class:`SplitLinkLoads`.

        Defining property: ``least_cost_ecmp_link_loads(pairs, w).as_dict()
        [(dpid, port)]`` is the sum over i of ``w[i] / N_i`` times the number
        of routes in ``find_route_least_cost(*pairs[i], multiple=True)`` that
        hold that entry, where N_i is the number of those routes.
        ``split="hop"`` divides the traffic at every switch evenly over its
        least-cost next hops instead.  Unknown hosts and unreachable pairs
        contribute nothing; repeated pairs add.  No route is enumerated
        (cost_ecmp_loads.hip pushes the demand down the least-cost DAG of each
        destination); link loads are float64 sums, equal to the definition
        within rounding (not bit-reproducible between runs), the last hops
        exact uint64.  With no cost set it is :meth:`ecmp_link_loads`."""
        return self._pair_loads(
            pairs, weights,
            lambda ex, sv, dv, w: self._switch_pair_cost_ecmp_loads(ex, sv, dv, w, split),
            SplitLinkLoads)

    def all_pairs_least_cost_ecmp_link_loads(self, split="route"):
        """:meth:`least_cost_ecmp_link_loads` over every ordered pair of
        distinct hosts with weight 1, from the per-switch host counts (as
        :meth:`all_pairs_link_loads`)."""
        got = self._all_pairs_loads(
            lambda ex, sv, dv, w: self._switch_pair_cost_ecmp_loads(ex, sv, dv, w, split),
            SplitLinkLoads)
        if got is None:
            macs = list(self.hosts)
            return self.least_cost_ecmp_link_loads(
                [(a, b) for a in macs for b in macs if a != b], None, split)
        return got

    def mpi_least_cost_ecmp_link_loads(self, rank_to_mac, traffic=None, split="route"):
        """:meth:`least_cost_ecmp_link_loads` of an MPI job (``traffic`` as in
        :meth:`mpi_link_loads`)."""
        pairs, weights = self._rank_pairs(rank_to_mac, traffic)
        return self.least_cost_ecmp_link_loads(pairs, weights, split)

    # -- link-failure what-if ---------------------------------------------
    @staticmethod
    def cable(a, b):
        """Both directions of the cable between switches ``a`` and ``b``, for
        a failure scenario."""
        return ((a, b), (b, a))

    def switch_links(self, dpid):
        """Every link into or out of switch ``dpid``, for a failure scenario.
        Failing them isolates the switch from the fabric; the switch itself
        stays, so two hosts on it still reach each other."""
        out = [(dpid, v) for v in sorted(self.links.get(dpid, {}))]
        out += [(u, dpid) for u in sorted(self.links) if u != dpid and dpid in self.links[u]]
        return tuple(out)

    def cable_failures(self):
        """One scenario per connected unordered switch pair -- the N-1 set --
        ascending: each holds the directions of that cable that exist."""
        cables = {}
        for u, nbrs in self.links.items():
            for v in nbrs:
                cables.setdefault((min(u, v), max(u, v)), []).append((u, v))
        return [tuple(sorted(cables[k])) for k in sorted(cables)]

    def _failure_edges(self, ex, failures):
        """(scenarios, edges): per scenario the tuple of its existing directed
        links, each once, in CSR order, and their CSR edge indices (int32)."""
        rp, col = ex.csr.row_ptr, ex.csr.col
        dp = ex.csr.dpids
        esrc = None
        scen, edges = [], []
        for sc in failures:
            es = set()
            for a, b in sc:
                u, v = ex.index.get(a), ex.index.get(b)
                if u is None or v is None:
                    continue
                lo, hi = int(rp[u]), int(rp[u + 1])
                e = lo + int(np.searchsorted(col[lo:hi], v))
                if e < hi and int(col[e]) == v:
                    es.add(e)
            es = np.asarray(sorted(es), np.int32)
            if esrc is None and es.size:
                esrc = np.repeat(np.arange(ex.csr.V), np.diff(np.asarray(rp, np.int64)))
            scen.append(tuple((int(dp[esrc[e]]), int(dp[col[e]])) for e in es.tolist()))
            edges.append(es)
        return scen, edges

    @staticmethod
    def _scenario_last_hops(routed, w, dv, last, ok, inv):
        """(hkey, hload uint64 [nscen, k], lost uint64 [nscen]) of MAC pairs
        under scenarios: the last hops of the pairs whose switch pair is
        routed in scenario k, and the weight of the known pairs that are not
        (``w``, ``dv``, ``last``, ``ok``, ``inv`` from :meth:`_switch_pairs`)."""
        nscen = routed.shape[0]
        hkey, hinv = np.unique(np.stack([dv[ok], last[ok]], 1), axis=0, return_inverse=True)
        hkey, hinv = hkey.reshape(-1, 2), hinv.reshape(-1)
        hload = np.zeros((nscen, hkey.shape[0]), np.uint64)
        lost = np.zeros(nscen, np.uint64)
        for k in range(nscen):
            got = routed[k][inv] if ok.size else np.zeros(0, bool)
            np.add.at(hload[k], hinv[got], w[ok][got])
            lost[k] = w[ok][~got].sum(dtype=np.uint64)
        return hkey, hload, lost

    def _all_pairs_scenario_last_hops(self, ex, routed, hv, hc, w):
        """:meth:`_scenario_last_hops` of the all-host-pairs demand (switch
        pairs ``repeat(hv) x tile(hv)`` with weights ``w``), from the per-switch
        host counts ``hc``."""
        nscen, n = routed.shape[0], hv.shape[0]
        hd = np.asarray([ex.index[h.port.dpid] for h in self.hosts.values()], np.int64)
        hp = np.asarray([int(h.port.port_no) for h in self.hosts.values()], np.int64)
        hkey, hinv = np.unique(np.stack([hd, hp], 1).reshape(-1, 2), axis=0, return_inverse=True)
        hkey, hinv = hkey.reshape(-1, 2), hinv.reshape(-1)
        hload = np.zeros((nscen, hkey.shape[0]), np.uint64)
        lost = np.zeros(nscen, np.uint64)
        for k in range(nscen):
            # hosts that reach switch d: every host on d gets that many flows, less itself
            cnt = (routed[k].reshape(n, n) * hc[hv][:, None]).sum(0)
            into = np.zeros(int(ex.csr.V), np.int64)
            into[hv] = cnt - 1
            np.add.at(hload[k], hinv, into[hd].astype(np.uint64))
            lost[k] = w[~routed[k]].sum(dtype=np.uint64)
        return hkey, hload, lost

    def _failure_switch_loads(self, ex, edges, sv, dv, w, split):
        """(load float64 [nscen, E], routed bool [nscen, n]) of switch pairs
        (dense ids sv -> dv, weights w u64) per failure scenario: one
        sdnr_failure_ecmp_link_loads call per chunk of scenarios whose load
        and routed planes fit the table budget."""
        if split not in ("route", "hop"):
            raise ValueError("split must be 'route' or 'hop'")
        E, n = int(ex.csr.E), int(sv.shape[0])
        load = np.zeros((len(edges), E), np.float64)
        routed = np.zeros((len(edges), n), bool)
        if n == 0 or not edges:
            return load, routed
        dsts, rows = np.unique(dv, return_inverse=True)
        budget = DEFAULT_TABLE_BUDGET if self._budget is None else self._budget
        step = max(1, int(budget) // max(1, 8 * E + n))
        cost = self._cost_vector(ex)
        for c0 in range(0, len(edges), step):
            got = self.engine.failure_ecmp_link_loads(ex, cost, dsts, rows.reshape(-1), sv, w,
                                                      edges[c0:c0 + step], split)
            load[c0:c0 + step], routed[c0:c0 + step] = got[0], got[2]
        return load, routed

    def failure_link_loads(self, failures, pairs, weights=None, split="route"):
        """What every link carries if links go down: :meth:`least_cost_ecmp_
        link_loads` of the pairs once per scenario of ``failures``, as a
        :class:`FailureLoads`.  A scenario is an iterable of directed links
        ``(src_dpid, dst_dpid)`` (the keys of :meth:`set_link_cost`; see
        :meth:`cable`, :meth:`switch_links`, :meth:`cable_failures`); links
        that do not exist are ignored, repeated ones count once, the empty
        scenario is the fabric as it is.  The routes are the least-cost ECMP
        sets under the costs in force -- with no cost set,
        ``find_route(multiple=True)``'s.

        Defining property: ``failure_link_loads(F, pairs, w, split).scenario(k)
        .as_dict()`` equals ``least_cost_ecmp_link_loads(pairs, w, split)
        .as_dict()`` of a second ``TopologyDB`` with the same switches, hosts,
        links and costs on which every link of ``F[k]`` was really removed
        with ``delete_link`` -- within rounding, and exactly where every share
        is a power of two.  A failed link carries exactly 0.0, also one that
        would still lie on a least-cost route by its cost.  A pair that loses
        every route contributes nothing to scenario k, not its last hop
        either, and its weight is counted in ``lost[k]``.

        Nothing of this object changes: not ``links``, the export, the cached
        tables, the costs or the graph on the GPU.  One kernel
        (failure_loads.hip) recomputes the least costs of every (scenario,
        destination switch) with the scenario's links masked out and pushes
        the demand down the surviving least-cost DAG; scenarios are processed
        in chunks whose results fit the table budget."""
        pairs = list(pairs)
        weights = None if weights is None else list(weights)
        ex = self.graph()
        scen, edges = self._failure_edges(ex, failures)
        w, dv, last, ok, inv, ssv, sdv, sw = self._switch_pairs(ex, pairs, weights)
        load, routed = self._failure_switch_loads(ex, edges, ssv, sdv, sw, split)
        hkey, hload, lost = self._scenario_last_hops(routed, w, dv, last, ok, inv)
        base = self.least_cost_ecmp_link_loads(pairs, weights, split)
        return FailureLoads(
            scen, load, lost, base, hkey, hload,
            lambda ld, hk, hl: self._link_loads_result(ex, ld, hk, hl, SplitLinkLoads))

    def all_pairs_failure_link_loads(self, failures, split="route"):
        """:meth:`failure_link_loads` over every ordered pair of distinct
        hosts with weight 1, from the per-switch host counts (as
        :meth:`all_pairs_link_loads`)."""
        if any(self._mac_to_int(m) in self.switches for m in self.hosts):
            macs = list(self.hosts)
            return self.failure_link_loads(
                failures, [(a, b) for a in macs for b in macs if a != b], None, split)
        ex = self.graph()
        scen, edges = self._failure_edges(ex, failures)
        sv, dv, w, hv, hc = self._all_pairs_demand(ex)
        load, routed = self._failure_switch_loads(ex, edges, sv, dv, w, split)
        hkey, hload, lost = self._all_pairs_scenario_last_hops(ex, routed, hv, hc, w)
        base = self.all_pairs_least_cost_ecmp_link_loads(split)
        return FailureLoads(
            scen, load, lost, base, hkey, hload,
            lambda ld, hk, hl: self._link_loads_result(ex, ld, hk, hl, SplitLinkLoads))

    def mpi_failure_link_loads(self, failures, rank_to_mac, traffic=None, split="route"):
        """:meth:`failure_link_loads` of an MPI job (``traffic`` as in
        :meth:`mpi_link_loads`)."""
        pairs, weights = self._rank_pairs(rank_to_mac, traffic)
        return self.failure_link_loads(failures, pairs, weights, split)

    # -- fast-reroute what-if ----------------------------------------------
    def _frr_switch_loads(self, ex, edges, sv, dv, w, node_protect, planes):
        """(load uint64 [nscen, E] or None, stat uint64 [nscen, 4], delivered
        bool [nscen, n] or None, peak, peak_edge, items) of switch pairs (dense
        ids sv -> dv, weights w u64) per failure scenario while the loop-free
        alternates forward: sdnr_frr_link_loads over the least-cost memo's
        next-hop rows and :meth:`_lfa_rows`, the scenarios in chunks that fit
        the table budget."""
        E, n = int(ex.csr.E), int(sv.shape[0])
        nscen = len(edges)
        bk = self._lfa_rows(ex, node_protect)[0]
        nh = self._cost_memo["pall"][1]
        if n == 0 or not edges:
            return (np.zeros((nscen, E), np.uint64) if planes else None,
                    np.zeros((nscen, 4), np.uint64),
                    np.zeros((nscen, n), bool) if planes else None, np.zeros(nscen, np.uint64),
                    np.full(nscen, -1, np.int32), 0)
        dsts, rows = np.unique(dv, return_inverse=True)
        load, stat, status, peak, pedge, items = self.engine.frr_link_loads(
            ex, _take(nh, dsts), _take(bk, dsts), dsts, rows.reshape(-1), sv, w, edges,
            planes=planes, table_budget=self._budget)
        delivered = None if status is None else (status == 1) | (status == 2)
        return load, stat, delivered, peak, pedge, items

    def _frr_result(self, ex, scen, got, base, hkey, hload):
        load, stat, _, peak, pedge, items = got
        link_of = self._edge_links(ex)
        link = [None if e < 0 else link_of(e) for e in pedge.tolist()]
        return FrrLoads(scen, load, stat, peak, link, base, hkey, hload,
                        lambda ld, hk, hl: self._link_loads_result(ex, ld, hk, hl, LinkLoads),
                        items)

    def frr_link_loads(self, failures, pairs, weights=None, node_protect=True, planes=True):
        """What every link carries while FAST REROUTE bridges a failure: the
        switches forward over their primaries (:meth:`least_cost_tables`'
        ``nh``) and, where a scenario of ``failures`` took a primary link, over
        their loop-free alternate (:meth:`lfa_tables`' ``backup``, the second
        bucket of a fast-failover group) -- before the controller re-routes;
        :meth:`failure_link_loads` is the state after it has.  A
        :class:`FrrLoads`; scenarios as in :meth:`failure_link_loads`.

        A switch whose primary link toward a destination is down and that has
        no alternate, or whose alternate's link is down too, drops that
        destination's traffic.  With more than one link down the alternates
        of different switches may forward in a circle (RFC 5286 promises loop
        freedom for the one failure an alternate was computed for).  Only
        delivered pairs load links and last hops; the weights of the others
        are in ``dropped``, ``looped`` and ``unrouted``.

        Defining property: ``scenario(k).as_dict()`` is the weighted count of
        the ``(dpid, out_port)`` entries of the delivered pairs' walks over
        those two tables.  Exact uint64 sums.  ``node_protect`` as in
        :meth:`lfa_tables` (and its ValueErrors).  ``planes=False``: only the
        per-scenario numbers are kept and ``scenario(k)`` raises -- the form
        for an N-1 sweep.  Nothing of this object changes: not ``links``, the
        costs, the memo or the graph on the GPU.  One kernel (frr_loads.hip)
        recomputes the (scenario, destination) items a failed link touches;
        scenarios are processed in chunks whose planes fit the table budget."""
        pairs = list(pairs)
        weights = None if weights is None else list(weights)
        ex = self.graph()
        scen, edges = self._failure_edges(ex, failures)
        w, dv, last, ok, inv, ssv, sdv, sw = self._switch_pairs(ex, pairs, weights)
        got = self._frr_switch_loads(ex, edges, ssv, sdv, sw, node_protect, planes)
        hkey = hload = None
        if planes:
            hkey, hload, _ = self._scenario_last_hops(got[2], w, dv, last, ok, inv)
        base = self.least_cost_link_loads(pairs, weights)
        return self._frr_result(ex, scen, got, base, hkey, hload)

    def all_pairs_frr_link_loads(self, failures, node_protect=True, planes=True):
        """:meth:`frr_link_loads` over every ordered pair of distinct hosts
        with weight 1, from the per-switch host counts (as
        :meth:`all_pairs_link_loads`)."""
        if any(self._mac_to_int(m) in self.switches for m in self.hosts):
            macs = list(self.hosts)
            return self.frr_link_loads(failures, [(a, b) for a in macs for b in macs if a != b],
                                       None, node_protect, planes)
        ex = self.graph()
        scen, edges = self._failure_edges(ex, failures)
        sv, dv, w, hv, hc = self._all_pairs_demand(ex)
        got = self._frr_switch_loads(ex, edges, sv, dv, w, node_protect, planes)
        hkey = hload = None
        if planes:
            hkey, hload, _ = self._all_pairs_scenario_last_hops(ex, got[2], hv, hc, w)
        base = self.all_pairs_least_cost_link_loads()
        return self._frr_result(ex, scen, got, base, hkey, hload)

    def mpi_frr_link_loads(self, failures, rank_to_mac, traffic=None, node_protect=True,
                           planes=True):
        """:meth:`frr_link_loads` of an MPI job (``traffic`` as in
        :meth:`mpi_link_loads`)."""
        pairs, weights = self._rank_pairs(rank_to_mac, traffic)
        return self.frr_link_loads(failures, pairs, weights, node_protect, planes)

    # -- link-cost what-if and the cost tuner -----------------------------
    @staticmethod
    def _link_edge(ex, a, b):
        """The CSR edge index of the link a -> b (dpids), None if there is none."""
        u, v = ex.index.get(a), ex.index.get(b)
        if u is None or v is None:
            return None
        rp, col = ex.csr.row_ptr, ex.csr.col
        lo, hi = int(rp[u]), int(rp[u + 1])
        e = lo + int(np.searchsorted(col[lo:hi], v))
        return e if e < hi and int(col[e]) == v else None

    @staticmethod
    def _edge_links(ex):
        """[(src_dpid, dst_dpid)] of every CSR edge, as a function of the edge."""
        csr = ex.csr
        esrc = np.repeat(np.arange(int(csr.V)), np.diff(np.asarray(csr.row_ptr, np.int64)))
        dp = csr.dpids
        return lambda e: (int(dp[esrc[e]]), int(dp[csr.col[e]]))

    def _cost_changes(self, ex, changes):
        """(scenarios, overrides): per scenario the tuple of its changes
        ``((src_dpid, dst_dpid), cost or None)`` on existing links in CSR
        order, and ``(edges int32, costs uint32)`` for the engine (None ->
        COST_INF).  A cost outside :meth:`set_link_cost`'s rule or one that
        reaches COST_INF times (V - 1), and a link given twice, are
        ValueErrors."""
        V = int(ex.csr.V)
        link = self._edge_links(ex)
        scen, over = [], []
        for sc in changes:
            seen, got = set(), {}
            for key, c in (sc.items() if hasattr(sc, "items") else sc):
                if not isinstance(key, tuple) or len(key) != 2:
                    raise ValueError("cost changes are keyed by (src_dpid, dst_dpid): %r" % (key,))
                if key in seen:
                    raise ValueError("link %r is given twice in one scenario" % (key,))
                seen.add(key)
                if c is not None:
                    if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or \
                            not 1 <= int(c) <= COST_MAX:
                        raise ValueError("link cost of %r must be an int in [1, 2**32 - 2] or "
                                         "None (down): %r" % (key, c))
                    if int(c) * max(0, V - 1) >= COST_INF:
                        raise ValueError("cost %d * (V - 1) reaches COST_INF" % int(c))
                e = self._link_edge(ex, key[0], key[1])
                if e is not None:
                    got[e] = COST_INF if c is None else int(c)
            es = sorted(got)
            scen.append(tuple((link(e), None if got[e] == COST_INF else got[e]) for e in es))
            over.append((np.asarray(es, np.int32), np.asarray([got[e] for e in es], np.uint32)))
        return scen, over

    def _capacity_vector(self, ex, capacity):
        """float64 [E] capacities in CSR edge order from ``{(src_dpid,
        dst_dpid): positive number}`` (links not named: 1.0; links that do not
        exist are ignored), or None when none is given."""
        if capacity is None:
            return None
        cap = np.ones(int(ex.csr.E), np.float64)
        for key, x in dict(capacity).items():
            if not isinstance(key, tuple) or len(key) != 2:
                raise ValueError("capacities are keyed by (src_dpid, dst_dpid): %r" % (key,))
            if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) \
                    or not (float(x) > 0 and np.isfinite(float(x))):
                raise ValueError("capacity of %r must be a positive finite number: %r" % (key, x))
            e = self._link_edge(ex, key[0], key[1])
            if e is not None:
                cap[e] = float(x)
        return cap

    def _cost_change_switch_loads(self, ex, over, sv, dv, w, split, cap, loads=True, reach=True):
        """The engine's (load, lost, routed, peak, peak_edge) of switch pairs
        (dense ids sv -> dv, weights w u64) per cost scenario: one
        sdnr_whatif_ecmp_link_loads call per chunk of scenarios whose planes
        fit the table budget."""
        if split not in ("route", "hop"):
            raise ValueError("split must be 'route' or 'hop'")
        dsts, rows = np.unique(dv, return_inverse=True)
        return self.engine.whatif_ecmp_link_loads(
            ex, self._cost_vector(ex), dsts, rows.reshape(-1), sv, w, over, split, cap,
            loads=loads, reach=reach, table_budget=self._budget)

    def _cost_change_result(self, ex, scen, load, lost, base, hkey, hload, peak, pedge, cap):
        link = self._edge_links(ex)
        return CostChangeLoads(
            scen, load, lost, base, hkey, hload,
            lambda ld, hk, hl: self._link_loads_result(ex, ld, hk, hl, SplitLinkLoads),
            peak, [link(e) if e >= 0 else None for e in pedge.tolist()],
            peak_utilisation(base.load, cap)[0])

    def cost_change_link_loads(self, changes, pairs, weights=None, split="route", capacity=None):
        """What every link carries if link costs change: :meth:`least_cost_
        ecmp_link_loads` of the pairs once per scenario of ``changes``, as a
        :class:`CostChangeLoads` -- cost a hot link up, or a link out for
        maintenance, and see the loads before anything is installed.  A
        scenario is a mapping or an iterable of ``((src_dpid, dst_dpid),
        cost)``: ``cost`` an int under :meth:`set_link_cost`'s rule, or None
        for link down; every link not named keeps the cost in force.  Links
        that do not exist are ignored, a link given twice in one scenario is a
        ValueError, the empty scenario is the fabric as it is.  ``capacity``:
        ``{(src_dpid, dst_dpid): positive number}`` for the peak utilisation,
        links not named have capacity 1.0.

        Defining property: ``cost_change_link_loads(C, pairs, w, split)
        .scenario(k).as_dict()`` equals ``least_cost_ecmp_link_loads(pairs, w,
        split).as_dict()`` of a second ``TopologyDB`` on which the changes of
        ``C[k]`` were really made with ``set_link_cost`` / ``delete_link`` --
        within rounding, and exactly where every share is a power of two.
        ``lost`` and the last hops as in :meth:`failure_link_loads`.

        Nothing of this object changes: not ``links``, the export, the cost
        settings, the cached tables or the graph on the GPU.  One kernel
        (whatif_loads.hip) recomputes the least costs of every (scenario,
        destination switch) under the scenario's costs and pushes the demand
        down that least-cost DAG; the peaks are reduced on the device."""
        pairs = list(pairs)
        weights = None if weights is None else list(weights)
        ex = self.graph()
        scen, over = self._cost_changes(ex, changes)
        cap = self._capacity_vector(ex, capacity)
        w, dv, last, ok, inv, ssv, sdv, sw = self._switch_pairs(ex, pairs, weights)
        load, _, routed, peak, pedge = self._cost_change_switch_loads(ex, over, ssv, sdv, sw,
                                                                     split, cap)
        hkey, hload, lost = self._scenario_last_hops(routed, w, dv, last, ok, inv)
        base = self.least_cost_ecmp_link_loads(pairs, weights, split)
        return self._cost_change_result(ex, scen, load, lost, base, hkey, hload, peak, pedge, cap)

    def all_pairs_cost_change_link_loads(self, changes, split="route", capacity=None):
        """:meth:`cost_change_link_loads` over every ordered pair of distinct
        hosts with weight 1, from the per-switch host counts (as
        :meth:`all_pairs_link_loads`)."""
        if any(self._mac_to_int(m) in self.switches for m in self.hosts):
            macs = list(self.hosts)
            return self.cost_change_link_loads(
                changes, [(a, b) for a in macs for b in macs if a != b], None, split, capacity)
        ex = self.graph()
        scen, over = self._cost_changes(ex, changes)
        cap = self._capacity_vector(ex, capacity)
        sv, dv, w, hv, hc = self._all_pairs_demand(ex)
        load, _, routed, peak, pedge = self._cost_change_switch_loads(ex, over, sv, dv, w, split,
                                                                     cap)
        hkey, hload, lost = self._all_pairs_scenario_last_hops(ex, routed, hv, hc, w)
        base = self.all_pairs_least_cost_ecmp_link_loads(split)
        return self._cost_change_result(ex, scen, load, lost, base, hkey, hload, peak, pedge, cap)

    def mpi_cost_change_link_loads(self, changes, rank_to_mac, traffic=None, split="route",
                                   capacity=None):
        """:meth:`cost_change_link_loads` of an MPI job (``traffic`` as in
        :meth:`mpi_link_loads`)."""
        pairs, weights = self._rank_pairs(rank_to_mac, traffic)
        return self.cost_change_link_loads(changes, pairs, weights, split, capacity)

    def _all_pairs_demand(self, ex):
        """(sv, dv, w, hv, hc): the all-host-pairs demand as switch pairs --
        hosts(s) * hosts(d) from s to d, less the hosts themselves."""
        hv = np.asarray(self._host_vertices(ex), np.int64)
        hc = np.asarray(ex.host_count, np.int64)
        n = hv.shape[0]
        sv, dv = np.repeat(hv, n), np.tile(hv, n)
        return sv, dv, (hc[sv] * (hc[dv] - (sv == dv))).astype(np.uint64), hv, hc

    def _tune(self, ex, sv, dv, w, capacity, split, rounds, top, steps, apply):
        """:meth:`tune_link_costs` on switch pairs (dense ids sv -> dv, weights
        w u64)."""
        steps = [int(x) for x in steps]
        if int(top) < 1 or not steps or min(steps) < 1:
            raise ValueError("top and every step are positive integers")
        cap = self._capacity_vector(ex, capacity)
        base = self._cost_vector(ex)
        V, E = int(ex.csr.V), int(ex.csr.E)
        link = self._edge_links(ex)
        accepted, history = {}, []          # edge -> cost; (link, cost, peak)
        peak_before = peak_after = None

        def scenario(extra=()):
            now = dict(accepted)
            now.update(extra)
            es = sorted(now)
            return np.asarray(es, np.int32), np.asarray([now[e] for e in es], np.uint32)

        def run(scen, loads):
            return self._cost_change_switch_loads(ex, scen, sv, dv, w, split, cap, loads=loads,
                                                  reach=False)

        for _ in range(max(0, int(rounds))):
            # the hottest links under the changes accepted so far
            util = run([scenario()], True)[0][0]
            if cap is not None:
                util = util / cap
            hot = [int(e) for e in np.lexsort((np.arange(E), -util))[:int(top)] if util[e] > 0]
            cands = [(e, c) for e in hot for c in (accepted.get(e, int(base[e])) + s for s in steps)
                     if c * max(0, V - 1) < COST_INF]
            peaks = run([scenario()] + [scenario([c]) for c in cands], False)[3]
            if peak_before is None:
                peak_before = peak_after = float(peaks[0])
            if not cands:
                break
            m = float(peaks[1:].min())
            if not m < float(peaks[0]) * (1 - 1e-9):
                break
            i = int(np.nonzero(peaks[1:] <= m * (1 + 1e-9))[0][0])
            e, c = cands[i]
            accepted[e] = c
            peak_after = float(peaks[1 + i])
            history.append((link(e), c, peak_after))
        if peak_before is None:
            peak_before = peak_after = float(run([scenario()], False)[3][0])
        costs = {link(e): c for e, c in sorted(accepted.items())}
        if apply and costs:
            self.set_link_costs(costs)
        return CostTuning(costs, peak_before, peak_after, history)

    def tune_link_costs(self, pairs, weights=None, capacity=None, split="route", rounds=8, top=8,
                        steps=(1, 2, 4), apply=False):
        """Which cost, on which link, flattens the fabric: a deterministic
        greedy descent on the peak utilisation (``load / capacity`` over the
        switch links, ``capacity`` as in :meth:`cost_change_link_loads`) of
        the pairs' :meth:`least_cost_ecmp_link_loads`, as a :class:`CostTuning`.

        Each of at most ``rounds`` rounds takes the ``top`` most utilised links
        under the changes accepted so far (ties by link order) and evaluates,
        for each of them and each step of ``steps``, "the accepted changes
        plus this link at its current cost + step" -- all of them, and the
        accepted changes alone, as the scenarios of one what-if call that
        returns only the peaks.  Candidates whose cost would break the cost
        rule are left out.  With m the smallest candidate peak, the first
        candidate in link-then-step order whose peak is <= m (1 + 1e-9) is
        accepted if m < the current peak (1 - 1e-9); otherwise the descent
        stops.  ``apply=True`` ends with one ``set_link_costs(costs)``; by
        default nothing of this object changes."""
        ex = self.graph()
        _, _, _, _, _, sv, dv, sw = self._switch_pairs(ex, list(pairs), weights)
        return self._tune(ex, sv, dv, sw, capacity, split, rounds, top, steps, apply)

    def all_pairs_tune_link_costs(self, capacity=None, split="route", rounds=8, top=8,
                                  steps=(1, 2, 4), apply=False):
        """:meth:`tune_link_costs` over every ordered pair of distinct hosts
        with weight 1, from the per-switch host counts (as
        :meth:`all_pairs_link_loads`)."""
        if any(self._mac_to_int(m) in self.switches for m in self.hosts):
            macs = list(self.hosts)
            return self.tune_link_costs([(a, b) for a in macs for b in macs if a != b], None,
                                        capacity, split, rounds, top, steps, apply)
        ex = self.graph()
        sv, dv, w, _, _ = self._all_pairs_demand(ex)
        return self._tune(ex, sv, dv, w, capacity, split, rounds, top, steps, apply)

    def mpi_tune_link_costs(self, rank_to_mac, traffic=None, capacity=None, split="route",
                            rounds=8, top=8, steps=(1, 2, 4), apply=False):
        """:meth:`tune_link_costs` of an MPI job (``traffic`` as in
        :meth:`mpi_link_loads`)."""
        pairs, weights = self._rank_pairs(rank_to_mac, traffic)
        return self.tune_link_costs(pairs, weights, capacity, split, rounds, top, steps, apply)

    # -- max-min fair rates ------------------------------------------------
    FAIR_ROUTES = ("default", "shortest", "least_cost", "least_loaded")
    FAIR_ECMP_ROUTES = ("ecmp", "least_cost_ecmp")

    def _fair_rows(self, ex, route, sv, dv):
        """The single-path tables of ``route`` for switch pairs sv -> dv, all
        of their rows resident at once: (tree, layout, rows, verts, to_root,
        reach) as ``engine.fair_rates`` takes them -- per-source default trees
        (row of sv, vertex dv) or per-destination next-hop rows (row of dv,
        vertex sv); reach: the pairs that have a route.  The rounds revisit
        every row, so a call is not chunked: rows beyond the table budget are
        a ValueError."""
        if route not in self.FAIR_ROUTES:
            raise ValueError("route must be one of %s" % ", ".join(
                map(repr, self.FAIR_ROUTES + self.FAIR_ECMP_ROUTES)))
        V = int(ex.csr.V)
        budget = int(DEFAULT_TABLE_BUDGET if self._budget is None else self._budget)
        c = self._cache
        if route == "default":
            key, other, store = sv, dv, c.dfs
            room = max(1, store.cap() - 1) if store.row_bytes else 1 << 62
        elif route == "shortest":
            key, other, store = dv, sv, c.sp
            room = max(1, store.cap() - 1) if store.row_bytes else 1 << 62
            room = min(room, max(1, budget // max(1, 4 * V)))   # the rows are widened to int32
        else:
            key, other = dv, sv
            room = self._cost_cap(ex) if route == "least_cost" else self._widest_cap(ex)
        want = sorted(set(key.tolist()))
        if len(want) > room:
            raise ValueError("fair rates keep every table row of a call resident across the "
                             "rounds: %d %s rows exceed the table budget of %d bytes (%d rows)"
                             % (len(want), route, budget, room))
        if route in ("default", "shortest"):
            batch = self._host_vertices(ex) if self._batch else ()
            get = c.sp_rows if route == "shortest" else c.dfs_rows
            tabs = get(self.engine, want, batch)
            slots = np.asarray([store.row[v] for v in key.tolist()], np.int64)
            if route == "default":
                # the hops plane holds -1 where unreached
                reach = _gather(tabs[-1], slots, other) != -1
                return tabs[0], c.layout, slots, other, False, reach
            plane, nh = tabs[0], tabs[1]
        else:
            m = self._cost_rows(ex, want) if route == "least_cost" else self._widest_rows(ex, want)
            slots = np.asarray([m["slot"][v] for v in key.tolist()], np.int64)
            plane, nh = m["tabs"][0], m["tabs"][1]
        # distances, costs and bottlenecks are held signed: no route reads -1
        reach = _gather(plane, slots, other) != -1
        urows, inv = np.unique(slots, return_inverse=True)
        nh = _take(nh, urows)
        if route == "shortest" and V <= 0xFFFF:
            nh = _u16(nh)
        nh = nh.astype(np.int32) if isinstance(nh, np.ndarray) else nh.to(dtype=_torch().int32)
        return nh, INT32, inv.reshape(-1), other, True, reach

    def _fair_ecmp_rows(self, ex, route, sv, dv):
        """The multipath tables of ``route`` for switch pairs sv -> dv, all of
        their rows resident at once: (cost, pcost, rows, reach) as
        ``engine.ecmp_fair_rates`` takes them.  ``"ecmp"``: the cached
        distance rows of the destinations widened to 32 bits, no costs (every
        link costs 1); ``"least_cost_ecmp"``: the memoised least-cost rows
        under the link costs in force.  More rows than the table budget holds
        are a ValueError, as in :meth:`_fair_rows`."""
        V = int(ex.csr.V)
        budget = int(DEFAULT_TABLE_BUDGET if self._budget is None else self._budget)
        want = sorted(set(dv.tolist()))
        if route == "ecmp":
            store = self._cache.sp
            room = max(1, store.cap() - 1) if store.row_bytes else 1 << 62
            room = min(room, max(1, budget // max(1, 4 * V)))   # the rows are widened to 32 bits
        else:
            room = self._cost_cap(ex)
        if len(want) > room:
            raise ValueError("fair rates keep every table row of a call resident across the "
                             "rounds: %d %s rows exceed the table budget of %d bytes (%d rows)"
                             % (len(want), route, budget, room))
        if route == "ecmp":
            batch = self._host_vertices(ex) if self._batch else ()
            tabs = self._cache.sp_rows(self.engine, want, batch)
            slots = np.asarray([store.row[v] for v in dv.tolist()], np.int64)
            # the distance plane holds -1 (u16 0xFFFF as int16) where unreached
            reach = _gather(tabs[0], slots, sv) != -1
            urows, inv = np.unique(slots, return_inverse=True)
            d = _u16(_take(tabs[0], urows))                      # unreached: -1, COST_INF as u32
            d = d.astype(np.int32) if isinstance(d, np.ndarray) else d.to(dtype=_torch().int32)
            return None, d, inv.reshape(-1), reach
        m = self._cost_rows(ex, want)
        slots = np.asarray([m["slot"][v] for v in dv.tolist()], np.int64)
        pc = m["tabs"][0]
        # pcost is held as int32: COST_INF reads -1
        reach = _gather(pc, slots, sv) != -1
        return self._cost_vector(ex), pc, slots, reach

    def _fair_capacity(self, ex, capacity):
        """float64 [E] link capacities: None 1.0 each, a positive number for
        every link, or a mapping as :meth:`_capacity_vector` takes it."""
        E = int(ex.csr.E)
        if capacity is None:
            return np.ones(E, np.float64)
        if isinstance(capacity, (int, float, np.integer, np.floating)) and \
                not isinstance(capacity, bool):
            if not (float(capacity) > 0 and np.isfinite(float(capacity))):
                raise ValueError("capacity must be a positive finite number: %r" % (capacity,))
            return np.full(E, float(capacity), np.float64)
        return self._capacity_vector(ex, capacity)

    def _fair_classes(self, ex, w, sv, dv, ports, capacity, host_capacity):
        """What the pairs of a fair-sharing call are told apart by: (cap
        float64 [E + extras], ok -- the pairs with known hosts --, hkey -- the
        last hops' (switch, port) --, nin -- the number of ports into the
        fabric, the first extras --, macs -- a MAC per extra --, cols -- per ok
        pair its switches and, with host ports, its two extras)."""
        E = int(ex.csr.E)
        if sum(int(x) for x in w.tolist()) >= FAIR_MULT_LIMIT:
            raise ValueError("fair rates: the weights must sum below 2**53")
        cap = self._fair_capacity(ex, capacity)
        if host_capacity is not None:
            if isinstance(host_capacity, bool) or \
                    not isinstance(host_capacity, (int, float, np.integer, np.floating)) or \
                    not (float(host_capacity) > 0 and np.isfinite(float(host_capacity))):
                raise ValueError("host_capacity must be a positive finite number: %r"
                                 % (host_capacity,))
            if ports is None:
                raise ValueError("host ports need MAC pairs")
        ok = np.nonzero(sv >= 0)[0]
        hkey = np.zeros((0, 2), np.int64)
        nin = 0
        macs = []
        if host_capacity is None:
            cols = np.stack([sv[ok], dv[ok]], 1).reshape(-1, 2)
        else:
            # extras: the ports into the fabric first, then the last hops
            ikey, iinv = np.unique(np.stack([sv[ok], ports[0][ok]], 1).reshape(-1, 2), axis=0,
                                   return_inverse=True)
            hkey, hinv = np.unique(np.stack([dv[ok], ports[1][ok]], 1).reshape(-1, 2), axis=0,
                                   return_inverse=True)
            iinv, hinv = iinv.reshape(-1), hinv.reshape(-1)
            nin = ikey.shape[0]
            macs = [None] * (nin + hkey.shape[0])
            for j, i in enumerate(ok.tolist()):
                macs[iinv[j]] = macs[iinv[j]] or ports[2][i]
                macs[nin + hinv[j]] = macs[nin + hinv[j]] or ports[3][i]
            cols = np.stack([sv[ok], dv[ok], E + iinv, E + nin + hinv], 1).reshape(-1, 4)
            cap = np.concatenate([cap, np.full(len(macs), float(host_capacity), np.float64)])
        return cap, ok, hkey, nin, macs, cols

    def _fair(self, ex, pairs, w, sv, dv, ports, capacity, host_capacity, route, split="route"):
        """FairRates of pairs already resolved: dense switches sv -> dv (-1:
        unknown host), multiplicities w, and per pair ``ports`` = (source
        switch port, destination switch port, source MAC, destination MAC) for
        the host-port constraints (None: not modelled)."""
        if split not in ("route", "hop"):
            raise ValueError("split must be 'route' or 'hop'")
        if route not in self.FAIR_ROUTES + self.FAIR_ECMP_ROUTES:
            raise ValueError("route must be one of %s" % ", ".join(
                map(repr, self.FAIR_ROUTES + self.FAIR_ECMP_ROUTES)))
        if route in self.FAIR_ECMP_ROUTES and not hasattr(self.engine, "ecmp_fair_rates"):
            # (a missing kernel is an error, never a fall-back to one path per pair)
            raise ValueError("route=%r needs an engine with ecmp_fair_rates (the multipath "
                             "filling); this one offers only the single-path routes %s"
                             % (route, ", ".join(map(repr, self.FAIR_ROUTES))))
        if split != "route" and route not in self.FAIR_ECMP_ROUTES:
            raise ValueError("split=%r needs a multipath route (%s): %r puts a pair on one path"
                             % (split, ", ".join(map(repr, self.FAIR_ECMP_ROUTES)), route))
        n = sv.shape[0]
        E, V = int(ex.csr.E), int(ex.csr.V)
        cap, ok, hkey, nin, macs, cols = self._fair_classes(ex, w, sv, dv, ports, capacity,
                                                            host_capacity)
        # pairs -> flows: equal (switches, extras) merge, multiplicities summed
        fkey, finv = np.unique(cols, axis=0, return_inverse=True)
        finv = finv.reshape(-1)
        fw = np.zeros(fkey.shape[0], np.uint64)
        np.add.at(fw, finv, w[ok])
        rate = np.zeros(n, np.float64)
        routed = np.zeros(n, bool)
        rnd = np.full(n, -1, np.int32)
        bott = np.full(n, -1, np.int64)
        levels = np.zeros(0, np.float64)
        used = np.zeros(cap.shape[0], np.float64)
        if fkey.shape[0]:
            fs, fd = fkey[:, 0], fkey[:, 1]
            extra = fkey[:, 2:4] if host_capacity is not None else None
            if route in self.FAIR_ECMP_ROUTES:
                cost, pcost, rows, reach = self._fair_ecmp_rows(ex, route, fs, fd)
                r, b, k, levels, used = self.engine.ecmp_fair_rates(ex, cost, pcost, rows, fs, fw,
                                                                    cap, extra, split)
            else:
                tree, layout, rows, verts, to_root, reach = self._fair_rows(ex, route, fs, fd)
                # (next-hop rows cannot tell an unreached vertex from the root)
                verts = np.where(reach, verts, -1)
                r, b, k, levels, used = self.engine.fair_rates(ex, tree, layout, rows, verts, fw,
                                                               cap, extra, to_root=to_root)
            rate[ok], rnd[ok], bott[ok], routed[ok] = r[finv], k[finv], b[finv], reach[finv]
        link = self._edge_links(ex)

        def names(e):
            return link(e) if e < E else ("host", macs[e - E])

        bottleneck = [None if e < 0 else names(e) for e in bott.tolist()]
        link_rate = self._link_loads_result(ex, used[:E], hkey, used[E + nin:], SplitLinkLoads)
        return FairRates(pairs, w, rate, routed, rnd, bottleneck, levels, link_rate, cap, used,
                         names)

    def fair_rates(self, pairs, weights=None, capacity=None, host_capacity=None, route="default",
                   split="route"):
        """What every (src_mac, dst_mac) pair of ``pairs`` gets when all of
        them send at once and share the links max-min fairly, as TCP or RoCE
        (DCQCN) flows approximately do: the rate of each pair, the link that
        limits it and the rate every link carries, as a :class:`FairRates`.
        A link load says how much crosses a link; this says how fast.

        ``route``: which single path a pair takes -- ``"default"``
        (:meth:`find_route`), ``"shortest"`` (``find_route(multiple=True)[0]``),
        ``"least_cost"`` (:meth:`find_route_least_cost`) or ``"least_loaded"``
        (:meth:`find_route_least_loaded`) --, or the set it is spread over:
        ``"ecmp"`` (every route of ``find_route(multiple=True)``, hop-count
        ECMP) or ``"least_cost_ecmp"`` (every route of
        ``find_route_least_cost(multiple=True)``).  ``split``: how a multipath
        route divides a pair, as in :meth:`ecmp_link_loads` -- ``"route"``
        (evenly over its routes) or ``"hop"`` (evenly over the next hops of
        every switch); anything but ``"route"`` with a single-path ``route``
        is a ValueError.  ``weights``: multiplicities --
        pair i stands for ``weights[i]`` identical parallel flows, each of
        which gets ``rate[i]`` (non-negative ints, None: 1; 0: absent; the sum
        must stay below 2**53, else ValueError).  ``capacity``: ``{(src_dpid,
        dst_dpid): positive number}`` (links not named: 1.0), one positive
        number for every link, or None: 1.0 each.  ``host_capacity`` None: the
        host ports are not modelled and pairs between the same two switches
        are one flow class; a positive number: every host port carries that
        much in each direction, and a pair is also bound by its source host's
        port into the fabric and by its last hop.

        The allocation is the max-min fair one (progressive filling: raise
        every rate together, freeze the flows of a link when it fills), which
        is unique; the GPU runs the rounds (fair_rates.hip), bit for bit equal
        to ``engine.fair_rates_host``.  Every table row the pairs need stays
        resident across the rounds: more rows than the table budget holds are
        a ValueError, not chunked.  Under the multipath routes a pair puts its
        ECMP fraction of its rate on every link of its route set
        (ecmp_fair_rates.hip; ``engine.ecmp_fair_rates_host`` within
        rounding); the link counts are float sums there, so links whose shares
        lie within 2**-30 (relative) of a level saturate with it, and a pair
        within that of a level is frozen at it."""
        ex = self.graph()
        pairs = list(pairs)
        n = len(pairs)
        w = _weights(weights, n)
        sv = np.full(n, -1, np.int64)
        dv = np.full(n, -1, np.int64)
        sport = np.zeros(n, np.int64)
        dport = np.zeros(n, np.int64)
        for i, (a, b) in enumerate(pairs):
            ea, eb = self._endpoint(a), self._endpoint(b)
            if ea is None or eb is None:
                continue
            sv[i] = ex.index[ea[0]]
            dv[i] = ex.index[eb[0]]
            sport[i] = self._last_hop(ea[0], ea[1], a)[1]
            dport[i] = self._last_hop(eb[0], eb[1], b)[1]
        ports = (sport, dport, [a for a, _ in pairs], [b for _, b in pairs])
        return self._fair(ex, pairs, w, sv, dv, ports, capacity, host_capacity, route, split)

    def all_pairs_fair_rates(self, capacity=None, route="default", split="route"):
        """:meth:`fair_rates` of every ordered pair of distinct hosts at once
        (all-to-all traffic), in the switch-pair form: ``pairs`` of the result
        are ``(src_dpid, dst_dpid)`` over the host-bearing switches and
        ``weights`` their host pairs, hosts(s) * (hosts(d) - [s == d]); host
        ports are not modelled.  ``route`` and ``split`` as in
        :meth:`fair_rates`.  When a host MAC names a switch the MAC-pair
        form is taken (``pairs`` are MAC pairs then), as in
        :meth:`all_pairs_link_loads`."""
        if any(self._mac_to_int(m) in self.switches for m in self.hosts):
            macs = list(self.hosts)
            return self.fair_rates([(a, b) for a in macs for b in macs if a != b], None, capacity,
                                   None, route, split)
        ex = self.graph()
        hv = np.asarray(self._host_vertices(ex), np.int64)
        hc = np.asarray(ex.host_count, np.int64)
        n = hv.shape[0]
        sv, dv = np.repeat(hv, n), np.tile(hv, n)
        w = (hc[sv] * (hc[dv] - (sv == dv))).astype(np.uint64)
        dp = ex.csr.dpids
        pairs = list(zip(dp[sv].tolist(), dp[dv].tolist()))
        return self._fair(ex, pairs, w, sv, dv, None, capacity, None, route, split)

    def mpi_fair_rates(self, rank_to_mac, traffic=None, capacity=None, host_capacity=None,
                       route="default", split="route"):
        """:meth:`fair_rates` of an MPI job's exchange: the keys of ``traffic``
        = {(src_rank, dst_rank): bytes} give the pairs, one flow each (None:
        every ordered rank pair i != j, one byte each).  The result also has
        ``bytes`` and ``time`` = bytes / rate per pair (``inf`` for bytes on a
        pair without a route, 0.0 for no bytes), and ``step_time()``, the
        largest: the exchange's duration if the rates held throughout -- flows
        that finish early would leave their share to the rest, so the real
        exchange is no slower than that (:meth:`mpi_exchange_times` follows
        the departures and gives the duration itself).  ``route`` and ``split``
        as in :meth:`fair_rates`."""
        pairs, nbytes = self._rank_pairs(rank_to_mac, traffic)
        res = self.fair_rates(pairs, None, capacity, host_capacity, route, split)
        b = np.ones(len(pairs), np.float64) if nbytes is None else \
            np.asarray([float(x) for x in nbytes], np.float64).reshape(-1)
        if (b < 0).any():
            raise ValueError("bytes are non-negative")
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(b == 0, 0.0, b / res.rate)
        res.bytes, res.time = b, t
        return res

    # -- max-min fair completion times ---------------------------------------
    def _fair_times(self, ex, pairs, w, nbytes, sv, dv, ports, capacity, host_capacity, route,
                    max_epochs, split="route"):
        """FlowTimes of pairs already resolved, as :meth:`_fair` takes them,
        each sending ``nbytes[i]`` bytes per flow."""
        if split not in ("route", "hop"):
            raise ValueError("split must be 'route' or 'hop'")
        if route not in self.FAIR_ROUTES + self.FAIR_ECMP_ROUTES:
            raise ValueError("route must be one of %s (got %r)" % (", ".join(
                map(repr, self.FAIR_ROUTES + self.FAIR_ECMP_ROUTES)), route))
        if route in self.FAIR_ECMP_ROUTES and not hasattr(self.engine, "ecmp_fair_times"):
            # (a missing kernel is an error, never a fall-back to one path per pair)
            raise ValueError("route=%r needs an engine with ecmp_fair_times (the multipath "
                             "epochs); this one offers only the single-path routes %s"
                             % (route, ", ".join(map(repr, self.FAIR_ROUTES))))
        if split != "route" and route not in self.FAIR_ECMP_ROUTES:
            raise ValueError("split=%r needs a multipath route (%s): %r puts a pair on one path"
                             % (split, ", ".join(map(repr, self.FAIR_ECMP_ROUTES)), route))
        n = sv.shape[0]
        E = int(ex.csr.E)
        b = np.asarray(nbytes, np.float64)
        b = np.full(n, float(b), np.float64) if b.ndim == 0 else b.reshape(-1)
        if b.shape[0] != n:
            raise ValueError("one byte size per pair")
        if not bool((np.isfinite(b) & (b >= 0)).all()):
            raise ValueError("byte sizes must be finite and not negative")
        b = b + 0.0                                             # (-0.0 is 0.0)
        if max_epochs is not None and int(max_epochs) < 0:
            raise ValueError("max_epochs must not be negative")
        cap, ok, hkey, nin, macs, cols = self._fair_classes(ex, w, sv, dv, ports, capacity,
                                                            host_capacity)
        # pairs -> flows: equal (switches, extras, bytes) merge, multiplicities summed
        cols = np.concatenate([cols, b[ok].view(np.int64).reshape(-1, 1)], 1)
        fkey, finv = np.unique(cols, axis=0, return_inverse=True)
        finv = finv.reshape(-1)
        fw = np.zeros(fkey.shape[0], np.uint64)
        np.add.at(fw, finv, w[ok])
        time = np.full(n, np.inf)
        epoch = np.full(n, -1, np.int32)
        rate0 = np.zeros(n, np.float64)
        left = b.copy()
        routed = np.zeros(n, bool)
        e_time, e_rounds = np.zeros(0, np.float64), np.zeros(0, np.int32)
        carried = np.zeros(cap.shape[0], np.float64)
        if fkey.shape[0]:
            fs, fd = fkey[:, 0], fkey[:, 1]
            extra = fkey[:, 2:4] if host_capacity is not None else None
            fb = np.ascontiguousarray(fkey[:, -1]).view(np.float64)
            if route in self.FAIR_ECMP_ROUTES:
                cost, pcost, rows, reach = self._fair_ecmp_rows(ex, route, fs, fd)
                t, k, r0, rest, e_time, e_rounds, carried = self.engine.ecmp_fair_times(
                    ex, cost, pcost, rows, fs, fw, fb, cap, extra, split, max_epochs=max_epochs)
            else:
                tree, layout, rows, verts, to_root, reach = self._fair_rows(ex, route, fs, fd)
                # (next-hop rows cannot tell an unreached vertex from the root)
                verts = np.where(reach, verts, -1)
                t, k, r0, rest, e_time, e_rounds, carried = self.engine.fair_times(
                    ex, tree, layout, rows, verts, fw, fb, cap, extra, to_root=to_root,
                    max_epochs=max_epochs)
            time[ok], epoch[ok], rate0[ok], left[ok] = t[finv], k[finv], r0[finv], rest[finv]
            routed[ok] = reach[finv]
        link_bytes = self._link_loads_result(ex, carried[:E], hkey, carried[E + nin:],
                                             SplitLinkLoads)
        return FlowTimes(pairs, w, b, time, epoch, routed, rate0, left, e_time, e_rounds,
                         link_bytes, split)

    def fair_completion_times(self, pairs, nbytes, weights=None, capacity=None,
                              host_capacity=None, route="default", max_epochs=None,
                              split="route"):
        """When every (src_mac, dst_mac) pair of ``pairs`` has sent its
        ``nbytes[i]`` bytes (one number: the same for all) if all start at
        once and share the links max-min fairly throughout: a pair that is
        done leaves and the others are refilled, which :meth:`fair_rates`'
        ``bytes / rate`` ignores.  Returns a :class:`FlowTimes`.

        ``weights``, ``capacity`` and ``host_capacity`` as in
        :meth:`fair_rates`; pair i stands for ``weights[i]`` parallel flows of
        ``nbytes[i]`` bytes each.  ``route`` and ``split`` as in
        :meth:`fair_rates`: one of the single-path tables ``"default"``,
        ``"shortest"``, ``"least_cost"``, ``"least_loaded"``, or the multipath
        sets ``"ecmp"`` and ``"least_cost_ecmp"``, which ``split`` divides by
        ``"route"`` or ``"hop"`` (anything but ``"route"`` with a single-path
        route is a ValueError; so is a multipath route on an engine without
        the multipath epochs).  ``max_epochs``: stop after
        that many departure epochs; the pairs still sending read ``time`` inf,
        ``epoch`` -2 and what they have left in ``remaining``.  Byte sizes that
        are negative, NaN or inf are a ValueError.  Pairs merge into one flow
        class only when switches, host ports and bytes are equal.  The GPU
        runs the epochs and their fillings from state on the device.  Under
        the single-path routes (fair_times.hip) the result is bit for bit
        ``engine.fair_times_host``; there is no tie tolerance, so pairs that
        end together as fractions may leave one ulp apart in consecutive
        epochs.  Under the multipath routes
        (ecmp_fair_times.hip; ``engine.ecmp_fair_times_host`` within rounding)
        the link counts are float sums, so the advance shares the filling's
        tolerance: a pair whose bytes would last within 2**-30 (relative) of
        the epoch's length leaves with it, and the links then carried that
        much less than its bytes."""
        ex = self.graph()
        pairs = list(pairs)
        n = len(pairs)
        w = _weights(weights, n)
        sv = np.full(n, -1, np.int64)
        dv = np.full(n, -1, np.int64)
        sport = np.zeros(n, np.int64)
        dport = np.zeros(n, np.int64)
        for i, (a, b) in enumerate(pairs):
            ea, eb = self._endpoint(a), self._endpoint(b)
            if ea is None or eb is None:
                continue
            sv[i] = ex.index[ea[0]]
            dv[i] = ex.index[eb[0]]
            sport[i] = self._last_hop(ea[0], ea[1], a)[1]
            dport[i] = self._last_hop(eb[0], eb[1], b)[1]
        ports = (sport, dport, [a for a, _ in pairs], [b for _, b in pairs])
        return self._fair_times(ex, pairs, w, nbytes, sv, dv, ports, capacity, host_capacity,
                                route, max_epochs, split)

    def all_pairs_fair_completion_times(self, nbytes=1.0, capacity=None, route="default",
                                        max_epochs=None, split="route"):
        """:meth:`fair_completion_times` of every ordered pair of distinct
        hosts at once, ``nbytes`` bytes each (MPI_Alltoall with equal blocks),
        in the switch-pair form of :meth:`all_pairs_fair_rates` (the MAC-pair
        form when a host MAC names a switch).  ``route`` and ``split`` as in
        :meth:`fair_completion_times`."""
        if isinstance(nbytes, bool) or not isinstance(nbytes, (int, float, np.integer,
                                                               np.floating)):
            raise ValueError("nbytes is one number for every pair")
        if any(self._mac_to_int(m) in self.switches for m in self.hosts):
            macs = list(self.hosts)
            return self.fair_completion_times([(a, b) for a in macs for b in macs if a != b],
                                              nbytes, None, capacity, None, route, max_epochs,
                                              split)
        ex = self.graph()
        hv = np.asarray(self._host_vertices(ex), np.int64)
        hc = np.asarray(ex.host_count, np.int64)
        n = hv.shape[0]
        sv, dv = np.repeat(hv, n), np.tile(hv, n)
        w = (hc[sv] * (hc[dv] - (sv == dv))).astype(np.uint64)
        dp = ex.csr.dpids
        pairs = list(zip(dp[sv].tolist(), dp[dv].tolist()))
        return self._fair_times(ex, pairs, w, nbytes, sv, dv, None, capacity, None, route,
                                max_epochs, split)

    def mpi_exchange_times(self, rank_to_mac, traffic=None, capacity=None, host_capacity=None,
                           route="default", max_epochs=None, split="route"):
        """:meth:`fair_completion_times` of an MPI job's exchange: the keys of
        ``traffic`` = {(src_rank, dst_rank): bytes} give the pairs, one flow
        each (None: every ordered rank pair i != j, one byte each).
        ``makespan()`` of the result is how long the exchange takes; it is
        never above ``mpi_fair_rates(...).step_time()`` beyond rounding (under
        the multipath routes: beyond their tolerance, 2**-30 relative).
        ``route`` and ``split`` as in :meth:`fair_completion_times`."""
        pairs, nbytes = self._rank_pairs(rank_to_mac, traffic)
        b = np.ones(len(pairs), np.float64) if nbytes is None else \
            np.asarray([float(x) for x in nbytes], np.float64).reshape(-1)
        return self.fair_completion_times(pairs, b, None, capacity, host_capacity, route,
                                          max_epochs, split)

    def find_routes(self, pairs, multiple=False):
        """find_route over many (src_mac, dst_mac) pairs; tables are computed
        once for all of them, and the default-route fdbs of large batches are
        expanded on the GPU (``route_entries``)."""
        pairs = list(pairs)
        if multiple and len(pairs) >= 16:
            return self._find_routes_multiple(pairs)
        if not multiple and len(pairs) >= 64:
            off, dp, pt = self.route_entries(pairs)
            dp, pt = dp.tolist(), pt.tolist()
            o = off.tolist()
            return [list(zip(dp[o[i]:o[i + 1]], pt[o[i]:o[i + 1]])) for i in range(len(pairs))]
        if not multiple and self._batch:
            ex = self.graph()
            want = set()
            for a, _ in pairs:
                ep = self._endpoint(a)
                if ep is not None:
                    want.add(ex.index[ep[0]])
            if len(want) < self._cache.dfs.cap():
                self._cache.dfs_rows(self.engine, sorted(want), self._host_vertices(ex))
        return [self.find_route(a, b, multiple) for a, b in pairs]


def sdn_mpi_mac(coll_type, src_rank, dst_rank):
    """The virtual destination MAC of an SDN-MPI message, as the router
    decodes it (reference ``sdnmpi/router.py:163-178``): locally administered
    bit 0x02 and the collective type << 2 in byte 0, the source and
    destination ranks as little-endian int16 in bytes 2-3 and 4-5."""
    b = [((int(coll_type) << 2) | 0x02) & 0xFF, 0,
         src_rank & 0xFF, (src_rank >> 8) & 0xFF, dst_rank & 0xFF, (dst_rank >> 8) & 0xFF]
    return ":".join("%02x" % x for x in b)


def _same_graph(a, b):
    return (a.V == b.V and a.E == b.E and np.array_equal(a.dpids, b.dpids)
            and np.array_equal(a.row_ptr, b.row_ptr) and np.array_equal(a.col, b.col)
            and np.array_equal(a.port, b.port))
