"""Random topology and cost events replayed on a live TopologyDB, every query
family compared after every event with an uncached twin.

What survives between calls -- the table cache across events
(TableCache.retarget, the re-slot of slot trees), pool eviction under a table
budget, the least-cost memo keyed on (export, cost version), the edge-port
memo -- returns a plausible wrong answer when it is stale, not an error.  The
twin is a fresh TopologyDB over copies of the dicts with a fresh restatement
double (test_failure_loads.FakeFailureEngine): it shares no cache, no export
and no engine with the live object, and its restatements are pinned to
enumeration by the rest of the CPU suite.

CPU only: the live object runs over the same double.  test_event_replay_gpu.py
runs the same replay with the real engine as the live object.

Tolerance: integer results (routes, tables, uint64 loads, lost weight) are
compared exactly; the float64 ECMP loads with test_ecmp_link_loads.dicts_close
(rtol 1e-9, identical key sets, exact zeros; derived there)."""
import collections

import numpy as np
import pytest

from oracle import oracle as O
from sdnmpi_amd import topologies as T
from sdnmpi_amd.engine import SLOT, dfs_row_bytes
from sdnmpi_amd.objects import Link, Port, Switch
from sdnmpi_amd.util.topology_db import TopologyDB
from test_ecmp_link_loads import SPLITS, dicts_close
from test_events import _events
from test_failure_loads import FakeFailureEngine

UNKNOWN_MAC = "02:00:00:00:ff:ff"
COST_KINDS = ("cost_link", "cost_absent", "cost_clear")
NEEDED_KINDS = ("delete_link", "add_link", "report", "new_vertex")
TWIN_FREE = "dragonfly:4,1,1"          # no two switches share their neighbour rows


def step_event(db, rng, dpids, nxt):
    """One random mutation: with probability 1/4 a cost event (a cost in
    [1, 9] on an existing link, or on a dpid pair without a link, or every
    cost cleared), else one of test_events._events.  Returns the kind."""
    if rng.random() >= 0.25:
        return _events(db, rng, dpids, nxt)
    links = [(u, v) for u in sorted(db.links) for v in sorted(db.links[u])]
    k = int(rng.integers(0, 4))
    if k <= 1 and links:
        u, v = links[int(rng.integers(len(links)))]
        db.set_link_cost(u, v, int(rng.integers(1, 10)))
        return "cost_link"
    if k == 2:
        for _ in range(8):
            u, v = (int(x) for x in rng.choice(dpids, 2, replace=False))
            if v not in db.links.get(u, {}):
                db.set_link_cost(u, v, int(rng.integers(1, 10)))
                return "cost_absent"
    db.clear_link_costs()
    return "cost_clear"


LOOP_KINDS = ("loop_delete", "loop_report", "loop_cost", "loop_add")


def loop_switches(db):
    """The switches that have a link to themselves, ascending."""
    return sorted(u for u, nb in db.links.items() if u in nb)


def step_event_loops(db, rng, dpids, nxt):
    """step_event with self-loop links mixed in (a cable between two ports of
    one switch, stored as links[u][u]): with probability 0.3 one existing loop
    is deleted, re-ported or given a cost, or a loop is added on a random
    dpid; else step_event.  Returns the kind."""
    if rng.random() >= 0.3:
        return step_event(db, rng, dpids, nxt)
    have = loop_switches(db)
    k = int(rng.integers(0, 5))
    if k <= 2 and have:
        u = have[int(rng.integers(len(have)))]
        if k == 0:
            db.delete_link(db.links[u][u])
            return "loop_delete"
        if k == 1:
            db.add_link(Link(Port(u, int(rng.integers(100, 200))), Port(u, 8)))
            return "loop_report"
        db.set_link_cost(u, u, int(rng.integers(1, 10)))
        return "loop_cost"
    u = int(dpids[int(rng.integers(len(dpids)))])
    db.add_link(Link(Port(u, 61), Port(u, 62)))
    return "loop_add"


def twin_of(db):
    """A fresh TopologyDB over copies of the live object's dicts and costs,
    with a fresh restatement double: the uncached reference."""
    twin = TopologyDB()
    twin._engine = FakeFailureEngine()
    twin.switches = dict(db.switches)
    twin.links = {u: dict(nb) for u, nb in db.links.items()}
    twin.hosts = dict(db.hosts)
    twin.set_link_costs(dict(db._link_costs))
    return twin


def with_ports(db):
    """Give every switch its port list (link ends, host ports, one reserved
    port), so the flood-port queries take the bulk pass."""
    ports = collections.defaultdict(set)
    for nb in db.links.values():
        for lk in nb.values():
            ports[lk.src.dpid].add(lk.src.port_no)
            ports[lk.dst.dpid].add(lk.dst.port_no)
    for h in db.hosts.values():
        ports[h.port.dpid].add(h.port.port_no)
    for d in list(db.switches):
        db.add_switch(Switch(d, [Port(d, n) for n in sorted(ports[d])] + [Port(d, 0xfffe)]))
    return db


def same(a, b):
    """Exact equality of nested results: dicts, sequences, numpy arrays (dtype
    and shape included), scalars."""
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(a, b))
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and \
            all(same(x, y) for x, y in zip(a, b))
    return a == b


def ref_is_edge(db, port):
    """The reference's loop (sdnmpi/topology.py:150-155), restated."""
    for nb in db.links.values():
        for lk in nb.values():
            if port == lk.src or port == lk.dst:
                return False
    return True


def draw_queries(db, rng):
    """The queries of one step: 24 sampled host pairs (repeats and a == b
    allowed) plus one unknown MAC and one switch-local port, integer weights
    below 2^20 with some zeros, the switches whose flood ports are asked, and
    the failure scenarios (three cables, every link of one switch, none) with
    the split they are asked under."""
    macs = sorted(db.hosts)
    pairs = [(macs[int(i)], macs[int(j)]) for i, j in rng.integers(0, len(macs), (24, 2))]
    sampled = len(pairs)
    pairs.append((macs[int(rng.integers(len(macs)))], UNKNOWN_MAC))
    if db.switches:
        local = sorted(db.switches)[int(rng.integers(len(db.switches)))]
        if local < 1 << 48:                        # a switch's local port: MAC == dpid
            h = "%012x" % local
            pairs.append((macs[int(rng.integers(len(macs)))],
                          ":".join(h[i:i + 2] for i in range(0, 12, 2))))
    w = rng.integers(0, 1 << 20, len(pairs))
    w[rng.random(len(pairs)) < 0.2] = 0
    probes = []
    if db.switches:
        for d in rng.choice(sorted(db.switches), min(3, len(db.switches)), replace=False).tolist():
            probes.append((d, [Port(d, 999), Port(d, int(rng.integers(1, 200)))]))
    cables = db.cable_failures()
    pick = sorted(rng.choice(len(cables), min(3, len(cables)), replace=False).tolist())
    dp = sorted(set(db.switches) | set(db.links))
    failures = [cables[i] for i in pick] + [db.switch_links(dp[int(rng.integers(len(dp)))]), ()]
    return {"pairs": pairs, "sampled": sampled, "w": w.tolist(), "probes": probes,
            "failures": failures, "split": SPLITS[int(rng.integers(2))]}


def answers(db, q):
    """(family, close, value) of every query family on ``db``, lazily: ``close``
    marks the float64 families (compared with dicts_close), the others are
    compared exactly."""
    pairs, w = q["pairs"], q["w"]
    yield "find_routes", False, db.find_routes(pairs)
    yield "find_routes_multiple", False, db.find_routes(pairs, multiple=True)
    yield "route_entries", False, db.route_entries(pairs)
    yield "switch_fdb_entries", False, db.switch_fdb_entries(pairs)
    for mode in ("dfs", "shortest"):
        yield "route_tables/" + mode, False, db.route_tables(mode)
    for route in ("default", "shortest"):
        got = db.link_loads(pairs, w, route)
        assert got.load.dtype == np.uint64
        yield "link_loads/" + route, False, (got.load, got.as_dict())
    for split in SPLITS:
        yield "ecmp_link_loads/" + split, True, db.ecmp_link_loads(pairs, w, split).as_dict()
    yield "least_cost_tables", False, db.least_cost_tables()
    yield "find_routes_least_cost", False, db.find_routes_least_cost(pairs)
    yield "find_routes_least_cost_multiple", False, db.find_routes_least_cost(pairs, multiple=True)
    got = db.least_cost_link_loads(pairs, w)
    yield "least_cost_link_loads", False, (got.load, got.as_dict())
    for split in SPLITS:
        yield "least_cost_ecmp_link_loads/" + split, True, \
            db.least_cost_ecmp_link_loads(pairs, w, split).as_dict()
    flags, flood = [], []
    for d, extra in q["probes"]:
        sw = db.switches[d]
        flags.append([db.is_edge_port(p) for p in list(sw.ports) + extra])
        flood.append(db.edge_ports(sw, 3))
    yield "is_edge_port", False, flags
    yield "edge_ports", False, flood
    split = q["split"]
    got = db.failure_link_loads(q["failures"], pairs, w, split)
    yield "failure_link_loads.lost/" + split, False, (got.scenarios, got.lost)
    yield "failure_link_loads.base/" + split, True, got.base.as_dict()
    for k in range(len(got)):
        yield "failure_link_loads[%d]/%s" % (k, split), True, got.scenario(k).as_dict()


def reference_answers(twin, q):
    """What the uncached ``twin`` answers to the queries, plus the oracle's
    restatements of the reference on the twin's dicts (routes, both modes) and
    the reference's own edge-port loop."""
    pairs = q["pairs"]
    oracle = {
        "find_routes": [O.find_route_pair(twin, a, b) for a, b in pairs],
        "find_routes_multiple": [O.find_routes_all_shortest(twin, a, b) for a, b in pairs],
        "is_edge_port": [[ref_is_edge(twin, p) for p in list(twin.switches[d].ports) + extra]
                         for d, extra in q["probes"]],
    }
    return {"oracle": oracle, "twin": {f: v for f, _, v in answers(twin, q)}}


def compare(db, q, ref, where=()):
    """Every family of the live ``db`` against the reference answers: the
    oracle first, then the twin.  Returns dict(no_route, all_routed, lost): a
    sampled pair had no route / every one had / a failure scenario lost
    weight."""
    lost = False
    for family, close, got in answers(db, q):
        if family in ref["oracle"]:
            assert same(got, ref["oracle"][family]), where + (family + "/oracle",)
        want = ref["twin"][family]
        assert dicts_close(got, want) if close else same(got, want), where + (family,)
        if family.startswith("failure_link_loads.lost"):
            lost = lost or bool(got[1].any())
    routed = [bool(r) for r in ref["oracle"]["find_routes"][:q["sampled"]]]
    return {"no_route": not all(routed), "all_routed": all(routed), "lost": lost}


def compare_all(db, twin, rng, where=()):
    """Draw one step's queries and compare every family of ``db`` with
    ``twin``."""
    q = draw_queries(db, rng)
    return compare(db, q, reference_answers(twin, q), where)


def fingerprint(db, q):
    """Everything a reference answer depends on: the dicts, the costs, the
    queries."""
    return (tuple((d, tuple(p.port_no for p in sw.ports)) for d, sw in sorted(db.switches.items())),
            tuple(sorted((u, v, lk.src.port_no, lk.dst.port_no)
                         for u, nb in db.links.items() for v, lk in nb.items())),
            tuple(sorted((m, h.port.dpid, h.port.port_no) for m, h in db.hosts.items())),
            tuple(sorted(db._link_costs.items())), repr(q))


_REFERENCES = {}      # (share tag, seed, step) -> (fingerprint, reference answers)


class Replay(object):
    """Event, then the comparison, step by step on one live object; the
    counters of the run.  ``share``: a tag naming the start state (fabric and
    what was done to it before the run); runs of one tag and seed make the
    same events and draw the same queries, so the twin's answers of a step are
    computed once, checked against the state they were computed from, and
    left unchanged.  ``costs=False``: topology events only.  ``event``: the
    step function (step_event, or _events without costs)."""

    def __init__(self, db, seed, fabric, share=None, costs=True, event=None):
        self.db, self.seed, self.share, self.costs = db, seed, share, costs
        self.event = event or (step_event if costs else _events)
        self.with_loop = 0            # compared steps with a self-loop link present
        self.rng = np.random.default_rng(seed)
        self.dpids = [int(d) for d in fabric.csr().dpids]
        self.nxt = [10 ** 6]
        self.kinds = collections.Counter()
        self.steps = self.compared = self.no_route = self.all_routed = self.lost = 0
        self.inherited = 0
        self._cache, self._seen = None, 0

    def _note_inherited(self):
        # db._cache is replaced on a re-export and its counter restarts: sum
        c = self.db._cache
        if c is None:
            return
        if c is not self._cache:
            self._cache, self._seen = c, 0
        self.inherited += c.rows_inherited - self._seen
        self._seen = c.rows_inherited

    def _reference(self, q, step):
        if self.share is None:
            return reference_answers(twin_of(self.db), q)
        key, fp = (self.share, self.seed, step), fingerprint(self.db, q)
        hit = _REFERENCES.get(key)
        if hit is None or hit[0] != fp:
            hit = _REFERENCES[key] = (fp, reference_answers(twin_of(self.db), q))
        return hit[1]

    def step(self):
        kind = self.event(self.db, self.rng, self.dpids, self.nxt)
        self.kinds[kind] += 1
        step = self.steps
        self.steps += 1
        if len(self.db.hosts) < 2:
            return kind
        q = draw_queries(self.db, self.rng)
        got = compare(self.db, q, self._reference(q, step), (self.seed, step, kind))
        self.compared += 1
        self.with_loop += bool(loop_switches(self.db))
        self.no_route += got["no_route"]
        self.all_routed += got["all_routed"]
        self.lost += got["lost"]
        self._note_inherited()
        return kind

    def counters(self):
        return {"kinds": dict(self.kinds), "steps": self.steps, "compared": self.compared,
                "no_route_steps": self.no_route, "all_routed_steps": self.all_routed,
                "lost_steps": self.lost, "rows_inherited": self.inherited,
                "loop_steps": self.with_loop}


def replay(db, seed, steps, fabric, after_step=None, share=None, event=None):
    """``steps`` times: one event, then every family against a fresh twin.
    Returns the counters; assertion messages carry (seed, step, kind, family)."""
    r = Replay(db, seed, fabric, share, event=event)
    for _ in range(steps):
        r.step()
        if after_step is not None:
            after_step(db, r)
    return r.counters()


def assert_conditions(c, incremental=True, costs=True):
    """A replay that compared nothing cannot pass: enough event kinds (a cost
    event among them, unless the run makes none), enough compared steps,
    cut-off and fully routed samples, lost weight, rows kept across events
    (none for the incremental=False control)."""
    kinds = set(k for k in c["kinds"] if k != "none")
    assert len(kinds) >= 8, c
    assert all(k in kinds for k in NEEDED_KINDS) and bool(kinds & set(COST_KINDS)) == costs, c
    assert 4 * c["compared"] >= 3 * c["steps"], c
    assert c["no_route_steps"] >= 1 and c["all_routed_steps"] >= 1, c
    assert c["lost_steps"] >= 1, c
    if incremental:
        assert c["rows_inherited"] > 0, c
    else:
        assert c["rows_inherited"] == 0, c


def live_db(fabric, engine, **kw):
    db = with_ports(fabric.populate(TopologyDB(**kw)))
    db._engine = engine
    return db


def wide_port(db):
    return any(lk.src.port_no >= 0xFFFF for nb in db.links.values() for lk in nb.values())


def slot_replay(engine, name, seed, steps):
    """The replay on slot trees: the fabric's first link is re-ported to port
    70000 before the run (test_events._slot_event_replay), and the layout must
    be SLOT for as long as that port is there.  Returns (counters, steps on
    slot trees, rows inherited on slot trees)."""
    fabric = T.by_name(name)
    db = fabric.populate(TopologyDB())
    u0 = sorted(db.links)[0]
    v0 = sorted(db.links[u0])[0]
    db.links[u0][v0] = Link(Port(u0, 70000), Port(v0, db.links[u0][v0].dst.port_no))
    with_ports(db)._engine = engine
    seen = {"steps": 0, "inherited": 0, "before": 0}

    def after(d, r):
        d.graph()
        assert (d._cache.layout == SLOT) == wide_port(d), (seed, r.steps)
        if d._cache.layout == SLOT:
            seen["steps"] += 1
            seen["inherited"] += r.inherited - seen["before"]
        seen["before"] = r.inherited

    c = replay(db, seed, steps, fabric, after, share=name + "/slot")
    return c, seen["steps"], seen["inherited"]


def tiny_budget(fabric):
    return 3 * dfs_row_bytes(fabric.csr())


def within_budget(db, budget):
    """The pools never outgrow the table budget (one row always fits)."""
    for pool in (db._cache.dfs, db._cache.sp):
        assert len(pool) <= pool.size <= pool.cap(), (len(pool), pool.size, pool.cap())
        assert pool.size <= 1 or pool.size * pool.row_bytes <= budget, (pool.size, budget)


FABRICS = {"fat_tree:4": (1, 7), TWIN_FREE: (1, 7)}    # seeds that meet assert_conditions


@pytest.mark.parametrize("budget", ["default", "tiny"])
@pytest.mark.parametrize("name,seed", [(n, s) for n, seeds in FABRICS.items() for s in seeds])
def test_replay_on_the_restatement_double(name, seed, budget):
    fabric = T.by_name(name)
    kw = {"table_budget": tiny_budget(fabric)} if budget == "tiny" else {}
    db = live_db(fabric, FakeFailureEngine(), **kw)
    after = (lambda d, r: within_budget(d, kw["table_budget"])) if kw else None
    c = replay(db, seed, 40, fabric, after, share=name)
    print("replay %s seed %d budget %s: %r" % (name, seed, budget, c))
    assert_conditions(c)


LOOP_STEPS = 60
LOOP_FABRICS = {"fat_tree:4": (1, 7), TWIN_FREE: (1, 7)}    # seeds that meet the conditions below


def assert_loop_conditions(c):
    """assert_conditions, every kind of self-loop event at least once, and a
    self-loop link present in at least 40 compared steps."""
    assert_conditions(c)
    assert all(c["kinds"].get(k, 0) >= 1 for k in LOOP_KINDS), c
    assert c["loop_steps"] >= 40, c


def loop_ports_are_no_edge_ports(db, r):
    """Both ports of every self-loop link are link ends: no flood ports."""
    for u in loop_switches(db):
        lk = db.links[u][u]
        assert not db.is_edge_port(lk.src) and not db.is_edge_port(lk.dst), (r.seed, r.steps, u)


@pytest.mark.parametrize("budget", ["default", "tiny"])
@pytest.mark.parametrize("name,seed", [(n, s) for n, seeds in LOOP_FABRICS.items() for s in seeds])
def test_replay_with_self_loop_events(name, seed, budget):
    fabric = T.by_name(name)
    kw = {"table_budget": tiny_budget(fabric)} if budget == "tiny" else {}
    db = live_db(fabric, FakeFailureEngine(), **kw)

    def after(d, r):
        loop_ports_are_no_edge_ports(d, r)
        if kw:
            within_budget(d, kw["table_budget"])

    c = replay(db, seed, LOOP_STEPS, fabric, after, share=name + "/loops",
               event=step_event_loops)
    print("replay %s seed %d budget %s with self-loops: %r" % (name, seed, budget, c))
    assert_loop_conditions(c)
