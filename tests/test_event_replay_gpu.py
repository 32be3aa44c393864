"""The event replay of test_event_replay.py with the real engine as the live
object: random topology and cost events on a TopologyDB over one shared
RouteEngine, every query family compared after every event with a host-only
twin (fresh dicts, fresh restatement double).  What is exercised is the state
that survives between calls on the device paths: the table cache across events
(incremental.hip's row test, the torch re-slot of slot trees), pool eviction
under a table budget, the least-cost memo, the engine's loaded graph and the
costs in force on the context, the DFS twin fold inside the small recompute
batches.  Then the engine alone: every table and load call on two exports in
shuffled orders, each answer against an expectation computed once.

Tolerance: as test_event_replay.py (integers exactly; float64 loads rtol 1e-9
with identical key sets and exact zeros, test_ecmp_link_loads.py)."""
import numpy as np
import pytest

from oracle import oracle as O
from sdnmpi_amd import _native
from sdnmpi_amd import engine as EN
from sdnmpi_amd import topologies as T
from test_cost_ecmp_loads import random_costs
from test_ecmp_link_loads import SPLITS, close
from test_ecmp_link_loads_gpu import dev_dist, zeros_f64
from test_event_replay import (COST_KINDS, LOOP_STEPS, TWIN_FREE, Replay, assert_conditions,
                               assert_loop_conditions, live_db, loop_ports_are_no_edge_ports,
                               replay, slot_replay, step_event_loops, tiny_budget, within_budget)
from test_failure_loads import cable_edges, switch_edges
from test_failure_loads_gpu import grouped, raw, same
from test_link_loads_gpu import on

pytestmark = pytest.mark.gpu

FAT = "fat_tree:4"
STEPS = 30


@pytest.fixture(scope="module")
def eng():
    e = EN.RouteEngine(0)
    yield e
    e.close()


def report(label, c):
    print("replay %s: %r" % (label, c))


@pytest.mark.parametrize("name,seed,fold", [(FAT, 1, None), (TWIN_FREE, 1, None),
                                            (FAT, 7, "1"), (TWIN_FREE, 7, "1")])
def test_replay_default_budget(eng, monkeypatch, name, seed, fold):
    """The default budget, with the twin fold as the library chooses and
    forced on: forced, it runs inside the recompute batches after an event."""
    if fold is not None:
        monkeypatch.setenv("SDNROUTE_DFS_FOLD", fold)
    fabric = T.by_name(name)
    if name == TWIN_FREE:
        eng.load(on(fabric.csr()))
        assert np.array_equal(eng.ctx.twin_reps(), np.arange(fabric.csr().V))
    batches = []
    tree_tables = eng.dfs_tree_tables

    def counted(export, srcs, layout, out=None):
        got = tree_tables(export, srcs, layout, out)
        batches.append((len(srcs), eng.ctx.last_dfs_searched()))
        return got

    monkeypatch.setattr(eng, "dfs_tree_tables", counted)
    c = replay(live_db(fabric, eng), seed, STEPS, fabric, share=name)
    report("%s seed %d fold %s" % (name, seed, fold), c)
    assert_conditions(c)
    assert batches and all(0 <= searched <= n for n, searched in batches)
    if fold == "1" and name == FAT:
        assert any(searched < n for n, searched in batches), batches


@pytest.mark.parametrize("name,seed", [(FAT, 1), (TWIN_FREE, 7)])
def test_replay_tiny_budget(eng, name, seed):
    """Three default-route rows fit: rows are evicted between and within the
    queries, and the pools never outgrow the budget."""
    fabric = T.by_name(name)
    budget = tiny_budget(fabric)
    db = live_db(fabric, eng, table_budget=budget)
    c = replay(db, seed, STEPS, fabric, lambda d, r: within_budget(d, budget), share=name)
    report("%s seed %d tiny budget" % (name, seed), c)
    assert_conditions(c)


@pytest.mark.parametrize("budget", ["default", "tiny"])
@pytest.mark.parametrize("name,seed", [(FAT, 1), (TWIN_FREE, 7)])
def test_replay_with_self_loop_events(eng, name, seed, budget):
    """Self-loop links added, deleted, re-ported and costed between the other
    events (test_event_replay.step_event_loops): the kernels read rows that
    hold their own vertex, the row test sees (u, u) changes, the cost upload a
    cost on (u, u), the cable scenarios a one-link cable."""
    fabric = T.by_name(name)
    kw = {"table_budget": tiny_budget(fabric)} if budget == "tiny" else {}
    db = live_db(fabric, eng, **kw)

    def after(d, r):
        loop_ports_are_no_edge_ports(d, r)
        if kw:
            within_budget(d, kw["table_budget"])

    c = replay(db, seed, LOOP_STEPS, fabric, after, share=name + "/loops",
               event=step_event_loops)
    report("%s seed %d budget %s with self-loops" % (name, seed, budget), c)
    assert_loop_conditions(c)


def test_replay_one_source_at_a_time(eng):
    fabric = T.by_name(FAT)
    c = replay(live_db(fabric, eng, batch_sources=False), 7, STEPS, fabric, share=FAT)
    report("%s seed 7 batch_sources=False" % FAT, c)
    assert_conditions(c)


def test_replay_control_without_the_incremental_cache(eng):
    """incremental=False: every link event starts a new cache.  The same
    answers, no row inherited."""
    fabric = T.by_name(TWIN_FREE)
    c = replay(live_db(fabric, eng, incremental=False), 1, STEPS, fabric, share=TWIN_FREE)
    report("%s seed 1 incremental=False" % TWIN_FREE, c)
    assert_conditions(c, incremental=False)


@pytest.mark.parametrize("name,seed", [(FAT, 1), (TWIN_FREE, 7)])
def test_replay_slot_layout(eng, name, seed):
    c, slot_steps, slot_inherited = slot_replay(eng, name, seed, STEPS)
    report("%s seed %d slot layout (%d steps, %d rows inherited on slot trees)"
           % (name, seed, slot_steps, slot_inherited), c)
    assert_conditions(c)
    assert slot_steps >= 1 and slot_inherited > 0


def test_two_live_objects_on_one_engine(eng):
    """Fabric A carries costs and cost events, fabric B none; they take turns
    on one engine, so every step swaps the loaded graph and clears or
    re-uploads the context's costs."""
    fa, fb = T.by_name(FAT), T.by_name(TWIN_FREE)
    a, b = live_db(fa, eng), live_db(fb, eng)
    rng = np.random.default_rng(3)
    links = [(u, v) for u in sorted(a.links) for v in sorted(a.links[u])]
    a.set_link_costs({k: int(c) for k, c in zip(links, rng.integers(1, 6, len(links)))})
    ra = Replay(a, 1, fa, share=FAT + "/costed")
    rb = Replay(b, 9, fb, share=TWIN_FREE + "/no cost events", costs=False)
    hands = 0
    for _ in range(20):
        for r in (ra, rb):
            before = eng._loaded
            r.step()
            assert eng._loaded is r.db._export
            hands += eng._loaded is not before
    assert not b._link_costs and not set(rb.kinds) & set(COST_KINDS)
    report("two objects, A %s seed 1" % FAT, ra.counters())
    report("two objects, B %s seed 9" % TWIN_FREE, rb.counters())
    assert_conditions(ra.counters())
    assert_conditions(rb.counters(), costs=False)
    assert hands >= 39, hands


# ------------------------------------------------------ engine-level call order --

class Case(object):
    """One export with its costs, its inputs on the device, and the expected
    result of every call, computed once from the host restatements."""

    def __init__(self, eng, name, cost, seed):
        import torch
        csr = T.by_name(name).csr()
        self.name, self.csr, self.cost, self.ex = name, csr, cost, on(csr)
        V = int(csr.V)
        rng = np.random.default_rng(seed)
        self.ids = np.arange(V, dtype=np.int32)
        self.dfs = O.dfs_tables(csr, self.ids)
        self.sp = O.dest_tables(csr, self.ids)
        self.pc = EN.cost_tables_host(csr, cost, self.ids)
        self.rows = np.repeat(np.arange(V), 2)
        self.other = rng.integers(-1, V + 1, 2 * V)
        self.w = rng.integers(0, 1 << 20, 2 * V, dtype=np.uint64)
        self.w[rng.random(2 * V) < 0.2] = 0
        cables = cable_edges(csr)
        pick = sorted(rng.choice(len(cables), 3, replace=False).tolist())
        self.scen = [cables[i] for i in pick] + [switch_edges(csr, int(rng.integers(0, V))), []]
        self.parent = torch.from_numpy(np.ascontiguousarray(self.dfs[0], np.int32)).to(eng.dev)
        self.dist = dev_dist(eng, self.sp[0])
        self.pcost = torch.from_numpy(np.ascontiguousarray(self.pc[0]).view(np.int32)).to(eng.dev)
        r, o, w = self.rows, self.other, self.w
        self.want = {
            "dfs_tables": self.dfs, "shortest_tables": self.sp, "cost_tables": self.pc,
            "link_loads": EN.link_loads_host(csr, self.dfs[0], EN.INT32, r, o, w),
        }
        for key, c in (("failure/cost", cost), ("failure/none", None)):
            self.want[key] = EN.failure_ecmp_link_loads_host(csr, c, self.ids, r, o, w, self.scen)
        for split in SPLITS:
            self.want["ecmp_link_loads/" + split] = \
                EN.ecmp_link_loads_host(csr, self.sp[0], r, o, w, split)
            self.want["cost_ecmp_link_loads/" + split] = \
                EN.cost_ecmp_link_loads_host(csr, cost, self.pc[0], r, o, w, split)

    def call(self, eng, what):
        """Make the call ``what`` on the engine and compare its result."""
        ex, r, o, w = self.ex, self.rows, self.other, self.w
        want = self.want[what]
        if what == "dfs_tables":
            got = [g.cpu().numpy() for g in eng.dfs_tables(ex, self.ids)]
            ok = all(np.array_equal(g, x) for g, x in zip(got, want))
        elif what == "shortest_tables":
            got = [g.cpu().numpy() for g in eng.shortest_tables(ex, self.ids)]
            got[0] = got[0].view(np.uint16)
            ok = all(np.array_equal(g, x) for g, x in zip(got, want))
        elif what == "cost_tables":
            got = [g.cpu().numpy() for g in eng.cost_tables(ex, self.cost, self.ids)]
            got[0] = got[0].view(np.uint32)
            ok = all(np.array_equal(g, x) for g, x in zip(got, want))
        elif what == "link_loads":
            got = eng.link_loads(ex, self.parent, EN.INT32, r, o, w)
            ok = got.dtype == np.uint64 and np.array_equal(got, want)
        elif what.startswith("ecmp_link_loads/"):
            ok = close(eng.ecmp_link_loads(ex, self.dist, r, o, w, what.split("/")[1]), want)
        elif what.startswith("cost_ecmp_link_loads/"):
            ok = close(eng.cost_ecmp_link_loads(ex, self.cost, self.pcost, r, o, w,
                                                what.split("/")[1]), want)
        else:
            cost = self.cost if what == "failure/cost" else None
            same(eng.failure_ecmp_link_loads(ex, cost, self.ids, r, o, w, self.scen), want)
            ok = True
        return ok


CALLS = ["dfs_tables", "shortest_tables", "cost_tables", "link_loads", "ecmp_link_loads/route",
         "ecmp_link_loads/hop", "cost_ecmp_link_loads/route", "cost_ecmp_link_loads/hop",
         "failure/cost", "failure/none"]


@pytest.fixture(scope="module")
def cases(eng):
    fat = T.by_name(FAT).csr()
    free = T.by_name(TWIN_FREE).csr()
    return [Case(eng, FAT, random_costs(fat, 1, 5, 11), 21),
            Case(eng, TWIN_FREE, np.ones(int(free.E), np.uint32), 22)]


def bad_scenario_call(eng, case):
    """sdnr_failure_ecmp_link_loads with a descending scenario list on the
    case's graph and costs: the argument error -22 at synchronize (the call of
    test_failure_loads_gpu.test_first_and_last_edge_duplicates_and_bad_lists)."""
    import torch
    V, E = int(case.csr.V), int(case.csr.E)
    eng.set_link_costs(case.ex, case.cost)
    order, off, s, ww = grouped(case.rows, case.other, case.w, V, V)
    lists = [[0], [9, 8, 7], [0, E - 1]]
    soff = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    load = zeros_f64(eng, len(lists) * E).reshape(len(lists), E)
    lost = zeros_f64(eng, len(lists))
    routed = torch.zeros((len(lists), len(case.rows)), dtype=torch.uint8, device=eng.dev)
    keep = raw(eng, case.ids, off, s, ww, soff, [e for x in lists for e in x], load, lost, routed)
    with pytest.raises(_native.SdnrError) as ei:
        eng.ctx.synchronize()
    assert ei.value.code == -22 and "ascending" in str(ei.value)
    del keep


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_engine_answers_do_not_depend_on_the_call_order(eng, cases, seed):
    """40 calls drawn with repetition over both exports, then the what-if
    without costs (it clears the context's costs) right before calls that
    need them; shuffle 1 also holds the call that ends in an argument error.
    Every answer equals the expectation computed once, whatever ran before."""
    rng = np.random.default_rng(100 + seed)
    order = [(int(rng.integers(2)), CALLS[int(rng.integers(len(CALLS)))]) for _ in range(40)]
    # every call on every export at least once
    todo = [(k, c) for k in range(2) for c in CALLS if (k, c) not in order]
    for i, kc in zip(rng.choice(40, len(todo), replace=False).tolist(), todo):
        order.insert(i, kc)
    order += [(0, "failure/none"), (0, "cost_ecmp_link_loads/route"), (0, "failure/none"),
              (0, "cost_tables"), (0, "failure/none"), (0, "failure/cost")]
    bad_at = 13 if seed == 1 else -1
    assert set(order) == set((k, c) for k in range(2) for c in CALLS)
    assert sum(a[0] != b[0] for a, b in zip(order, order[1:])) >= 10    # the graph changes hands
    for i, (k, what) in enumerate(order):
        if i == bad_at:
            bad_scenario_call(eng, cases[0])
        assert cases[k].call(eng, what), (seed, i, cases[k].name, what,
                                          [(cases[j].name, c) for j, c in order[:i]][-3:])
        assert eng._loaded is cases[k].ex
