"""GPU: the answers of an engine do not depend on which consumer asks first.  The engine derives its views of the
global graph (edge pool, node grid, node tree and its order, host CSR, ...) lazily, so a view that is served stale
shows up as a dependence on the order of the calls.  Every state below is reached on three engines; each runs the
same consumers in another order (forward, reversed, rotated by half), and every answer must be the same bit for
bit.  graph("global"), plan and is_frontier must also be the oracle's, driven through the same steps.

On the way to a state nothing asks the engine for a lazy view: the build goes through graph_support.drive, whose one
question after it, graph("global"), is answered from the CSR that every build leaves; the local map and the update
of a state are given to the engine without a probe, so that update is the first to need the pool, the grid and the
order after a device build.

Cloud "B" under the parameters of update_scenarios.py (MOUNTAIN with UPDATE_OVERRIDES, seed 5, START_B, V = 2288)."""
import json

import numpy as np
import pytest

import update_scenarios as us
from conftest import assert_graph_equal, weight_report
from graph_support import GRAPH_FIELDS, drive, first_difference

pytestmark = pytest.mark.gpu

_BUILD = [("map", "B"), ("init", us.START_B)]
_HOST = [("replay", "host")] + _BUILD
# state -> (steps of graph_support.drive, what follows them on the engine and the oracle, without a probe)
STATES = {
    "device_build": (_BUILD, None),
    "host_build": (_HOST, None),
    "declined_build": ([("map", "B"), ("init_declined", us.START_B, 2)], None),
    "device_build_update": (_BUILD, "update"),  # a local map at a node's pose, then update_graph
    "host_build_update": (_HOST, "update"),
    "load_json": (_BUILD, "load"),    # a second engine loads the file the driven one saved
    "reset": (_BUILD, "reset"),       # reset_graph("global")
    # The reset after a HOST build is a state of its own.  Before the views had stamps that reset left the
    # node grid marked current over the nodes of the graph that was, and is_frontier answered from them (159 of the
    # 200 points no frontier); the reset commits like every other change now and names no grid.
    "host_build_reset": (_HOST, "reset"),
}
PLAN = us._PLAN_B[1:]
ORDERS = ("forward", "reversed", "rotated")
# What the consumers answer after reset_graph("global"), as the parent commit answered: an empty global and local
# graph, a file without nodes or edges, plan and cost_field refused, and every point a frontier (no node blocks
# it and there is no local map).
EMPTY_REFUSAL = "graph is empty"


@pytest.fixture(scope="module")
def clouds(synth):
    return {"B": synth.mountain_cloud(200, 200, seed=1)}


@pytest.fixture(scope="module")
def points():
    """200 seeded points of a box 1 m larger than the map's."""
    return np.random.default_rng(77).uniform(-1.0, 21.0, size=(200, 2)).astype(np.float32)


def as_bits(answer):
    """An answer in a form that == compares bit for bit (a graph: V, E and every array)."""
    if hasattr(answer, "rowptr"):
        return (answer.V, answer.E) + tuple(getattr(answer, n).tobytes() for n in GRAPH_FIELDS + ("w",))
    return answer


def assert_oracle_graph(g, ref, where):
    diff = first_difference(g, ref, weights=None)
    assert diff is None, f"{where}: {diff}"
    assert_graph_equal(g, ref, 1e-5)


def consumers(e, points, tmp):
    import trg_planner

    def refusable(call):
        def run():
            try:
                return call()
            except trg_planner.TrgError as err:
                return ("refused", str(err))
        return run

    def save():
        e.save_json(tmp)
        return tmp.read_bytes()

    def plan():
        path, info = e.plan(*PLAN)
        return path.tobytes(), info.num_points, info.direct_dist, info.path_length, info.avg_risk

    def field():
        cost, hops, parent, _ = e.cost_field(source_id=0)
        return cost.tobytes(), hops.tobytes(), parent.tobytes()

    return [("graph_global", lambda: e.graph("global")),
            ("graph_local", lambda: e.graph("local")),
            ("save_json", save),
            ("plan", refusable(plan)),
            ("is_frontier", lambda: e.is_frontier(points).tobytes()),
            ("cost_field", refusable(field))]


def ordered(calls, order):
    if order == "reversed":
        return calls[::-1]
    if order == "rotated":
        return calls[len(calls) // 2:] + calls[:len(calls) // 2]
    return calls


def assert_loaded_graph(g, saved, ref):
    """The graph after load_json against the graph of the engine that saved it and against the oracle's.  The file
    carries ids, positions, states and every edge's dist and weight exactly (%.9g gives every fp32 back), so all of
    them are compared bit for bit.  It carries no creation index (a loaded node's is its id), and it lists a node's
    edges in the order of the saving engine's pool, which the loading pool may turn round: rows are compared entry
    by entry under their (row, col) keys."""
    assert (g.V, g.E) == (ref.V, ref.E) == (saved.V, saved.E), (g.V, g.E, ref.V, ref.E)
    for name in ("rowptr", "state", "xyz"):
        for other in (ref, saved):
            assert getattr(g, name).tobytes() == getattr(other, name).tobytes(), f"load_json: {name}"
    assert np.array_equal(g.cid, np.arange(g.V)), "load_json: cid"
    rows = np.repeat(np.arange(g.V), np.diff(g.rowptr))
    pg, pr, ps = (np.lexsort((x.col, rows)) for x in (g, ref, saved))
    assert np.array_equal(g.col[pg], ref.col[pr]) and np.array_equal(g.col[pg], saved.col[ps]), "load_json: col"
    assert g.dist[pg].tobytes() == ref.dist[pr].tobytes() == saved.dist[ps].tobytes(), "load_json: dist"
    assert g.w[pg].tobytes() == saved.w[ps].tobytes(), "load_json: w against the saving engine's"
    flips, others, mx = weight_report(g.w[pg], ref.w[pr], 1e-5)  # the engine's weights against the oracle's, as ever
    assert (flips, others) == (0, 0), (flips, others, mx)


def reach(oa, clouds, state, tmp_path, order):
    """An engine in `state`, the oracle that went through the same steps, and for load_json the graph of the engine
    that saved the file."""
    import trg_planner
    steps, then = STATES[state]
    prm = dict(oa.MOUNTAIN, **us.UPDATE_OVERRIDES)
    e = trg_planner.Engine(**prm)
    e.set_sampler(5, 16)
    o, w = oa.Oracle(**prm), oa.Oracle(**prm)
    for x in (o, w):
        x.set_sampler(5, 0, 16)
    w.set_cov_f64(True)
    hist = drive(e, o, w, steps, clouds=clouds, prm=prm)
    assert hist[0]["V"] == 2288, hist[0]["V"]
    fallbacks = hist[0]["stats"]["bfs_fallbacks"]
    assert fallbacks == (1 if state == "declined_build" else 0), fallbacks
    saved = None
    if then == "update":
        graph, memo = o.graph(0), {}
        pose = us.node_fraction(1, 2)(graph, memo)
        local = np.ascontiguousarray(us.crop(3.0)(clouds["B"], pose, graph, memo), dtype=np.float32)
        for x in (e, o):
            x.set_local_map(pose, local)
            x.update_graph()
    elif then == "load":
        file = tmp_path / f"built_{order}.json"
        e.save_json(file)
        saved = e.graph("global")
        e = trg_planner.Engine(**prm)
        e.set_sampler(5, 16)
        e.set_global_map(clouds["B"])
        e.load_json(file)
    elif then == "reset":
        e.reset_graph("global")
    return e, o, saved


@pytest.mark.parametrize("state", list(STATES))
def test_view_order(oa, clouds, points, tmp_path, state):
    has_local = STATES[state][1] == "update"
    answers, oracles, engines, built = {}, {}, {}, {}
    for order in ORDERS:
        e, o, built[order] = reach(oa, clouds, state, tmp_path, order)
        calls = ordered(consumers(e, points, tmp_path / f"saved_{order}.json"), order)
        got = {name: call() for name, call in calls}
        if has_local:  # a further update is the last consumer: it needs the pool, the grid and the order itself
            e.update_graph()
            got["update"] = e.graph("global")
        answers[order], oracles[order], engines[order] = got, o, e
    for order in ORDERS[1:]:
        for name, value in answers["forward"].items():
            assert as_bits(answers[order][name]) == as_bits(value), f"{state}: {name} differs between the orders forward and {order}"

    got, o, e = answers["forward"], oracles["forward"], engines["forward"]
    if STATES[state][1] == "reset":
        for name in ("graph_global", "graph_local"):
            assert (got[name].V, got[name].E) == (0, 0), (name, got[name].V, got[name].E)
        saved = json.loads(got["save_json"])
        assert not saved["nodes"] and not saved["edges"], saved
        for name in ("plan", "cost_field"):
            assert got[name][0] == "refused" and EMPTY_REFUSAL in got[name][1], (name, got[name])
        frontier = np.frombuffer(got["is_frontier"], np.int32)
        assert frontier.all(), f"{state}: {int((frontier == 0).sum())} of {frontier.size} points no frontier"
        # ... and a build afterwards gives the first build's graph again: its nodes and edge count, under the ids of
        # a second build (the reference's initGraph begins with the same reset, and cleanGraph numbers the nodes in
        # the iteration order of a container that remembers the first build: the oracle builds twice as well)
        first = o.graph(0)
        assert o.init_graph(us.START_B)
        again = o.graph(0)
        assert (again.V, again.E) == (first.V, first.E)
        assert sorted(map(bytes, again.xyz)) == sorted(map(bytes, first.xyz))
        for order in ORDERS:
            engines[order].init_graph(us.START_B)
            assert_oracle_graph(engines[order].graph("global"), again, f"{state}, {order}: init_graph after the reset")
        return
    # the oracle's answers before the further update (taken now: the oracle computes nothing lazily) ...
    ref_path, ref_info = o.plan(*PLAN)
    assert ref_path.shape[0] > 1
    assert got["plan"][0] == ref_path.tobytes() and got["plan"][3] == ref_info[1], f"{state}: plan against the oracle"
    assert got["is_frontier"] == o.is_frontier(points).tobytes(), f"{state}: is_frontier against the oracle"
    if state == "load_json":
        assert_loaded_graph(got["graph_global"], built["forward"], o.graph(0))
    else:
        assert_oracle_graph(got["graph_global"], o.graph(0), f"{state}: graph against the oracle")
    if has_local:  # ... and its graph after it
        o.update_graph()
        assert_oracle_graph(got["update"], o.graph(0), f"{state}: graph after the further update")
