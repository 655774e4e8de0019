"""GPU: cost fields from source sets (trg_engine_cost_field_sets, Engine.cost_fields_from / nearest_source /
assign_frontiers, routes and field_reached on a set solve; DESIGN.md section 2, "Source sets").

Every comparison is exact -- cost as bits; hops, parents, owners, `owned`, `reached` and the values at the targets
equal -- against tests/set_ref.py, the definitions in Python (checked on the CPU against the compiled host Dijkstra,
tests/test_cost_field_sets_cpu.py); bounded solves against its truncate() at the EXPECTED bound, which comes from
the reference alone.  Graphs come from tests/field_graphs.py through load_json on an engine without a map.

Shapes: the smallest at which each piece can go wrong -- V ~ 30-44 with every kind of member (duplicate, Invalid,
isolated, both components, all nodes), batches through the MULTI kernels up to the limit of 64, exact ties that
only the parent rule decides, a chain whose owner pass needs 13 doublings, a 30 000-long row, +inf costs, all-zero
costs.  Round counts are asserted on the unit chain only, where they are a function of the graph."""
import ctypes as C

import numpy as np
import pytest

import bound_ref
import field_graphs as fg
import route_ref
import set_ref
from field_support import (INVALID_ARG, SCALES, assert_rows, bits, engine, load_graph, ref,  # noqa: F401
                           reference_fields, with_isolated_node, write_graph)

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = F32(np.inf)
SF = 3.0


def _b1(v):
    return int(np.float32(v).view(np.uint32))


def _refs(x, sets):
    return [set_ref.set_field(x, SF, s) for s in sets]


def _check(e, refs, sets, at, budget=None, settle=None, targets=None, full=True):
    """One set solve against the (truncated) reference fields -> the engine's result."""
    m = len(sets)
    want = refs
    bounded = budget is not None or settle is not None
    if bounded:
        bud = np.full(m, INF, F32) if budget is None else np.broadcast_to(np.asarray(budget, F32).reshape(-1), (m,))
        want_bound = np.array([min(bud[k], bound_ref.settle_bound(refs[k].cost, refs[k].hops, targets, settle))
                               for k in range(m)], F32)
        want = [set_ref.truncate(refs[k], want_bound[k]) for k in range(m)]
    r = e.cost_fields_from(sets, targets=targets, full=full, budget=budget, settle=settle)
    if bounded:
        assert np.array_equal(bits(r["bound"]), bits(want_bound)), at + f"bound {r['bound']!r} != {want_bound!r}"
    else:
        assert "bound" not in r
    stack = [np.stack([getattr(f, name) for f in want]) for name in ("cost", "hops", "parent", "owner")]
    assert np.array_equal(r["reached"], (stack[1] >= 0).sum(axis=1)), at + f"reached {r['reached']}"
    assert r["info"].reached == int(r["reached"].sum()) and r["info"].source == int(sets[0][0]), at
    assert len(r["owned"]) == m and len(r["sets"]) == m
    for k in range(m):
        assert np.array_equal(r["owned"][k], want[k].owned), at + f"owned of set {k}: {r['owned'][k]} != {want[k].owned}"
        assert int(r["owned"][k].sum()) == int(r["reached"][k]), at
        assert np.array_equal(r["sets"][k], np.asarray(sets[k], np.int32)), at
    if full:
        assert_rows(at, "costs", r["cost"], stack[0], as_bits=True)
        assert_rows(at, "hops", r["hops"], stack[1])
        assert_rows(at, "parents", r["parent"], stack[2])
        assert_rows(at, "owners", r["owner"], stack[3])
    if targets is not None:
        t = np.asarray(targets, np.int64)
        assert np.array_equal(bits(r["cost_at"]), bits(stack[0][:, t])), at + "cost_at"
        assert np.array_equal(r["hops_at"], stack[1][:, t]), at + "hops_at"
        assert np.array_equal(r["owner_at"], stack[3][:, t]), at + "owner_at"
    return r


def _raw(e, sets, ptr=None, ids=None, m=None, budget=None, settle=0, targets=None, n_targets=None, cost_at=False,
         parent=None, owner=None, owned=None):
    """One trg_engine_cost_field_sets call with only the outputs named -> (status, TrgFieldInfo, cost_at)."""
    from trg_planner._engine import TrgFieldInfo, _f, _i
    if ptr is None:
        ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
        ids = np.concatenate([np.asarray(s) for s in sets])
    ptr, ids = np.ascontiguousarray(ptr, np.int32), np.ascontiguousarray(ids, np.int32)
    m = len(ptr) - 1 if m is None else m
    b = None if budget is None else np.ascontiguousarray(budget, np.float32)
    t = None if targets is None else np.ascontiguousarray(targets, np.int32)
    nt = (0 if t is None else t.size) if n_targets is None else n_targets
    at = np.empty(max(m, 1) * max(nt, 1), np.float32) if cost_at else None
    info = TrgFieldInfo()
    st = e.L.trg_engine_cost_field_sets(
        e.h, m, _i(ptr), _i(ids), None if b is None else _f(b), settle, None, None,
        None if parent is None else _i(parent), None if owner is None else _i(owner), None if t is None else _i(t), nt,
        None if at is None else _f(at), None, None, None if owned is None else _i(owned), None, None, C.byref(info))
    return st, info, at


def _kinds(g):
    """Member nodes of a random_small graph with an isolated last node: one of each component, an Invalid node, the
    isolated one."""
    V = len(g.state)
    half = (V - 1) // 2 + 3  # ids from here on only link among themselves
    first = int(np.flatnonzero(g.state[:half] != fg.INVALID)[0])
    second = half + int(np.flatnonzero(g.state[half:V - 1] != fg.INVALID)[0])
    invalid = int(np.flatnonzero(g.state == fg.INVALID)[0])
    return first, second, invalid, V - 1


@pytest.mark.parametrize("seed", [7, 13])
def test_random_graphs(engine, tmp_path, seed):
    """One set of each kind alone (the m == 1 kernels), then all five as one batch, at every bucket width."""
    e = engine
    g = with_isolated_node(fg.with_positions(fg.random_small(seed)))
    x = load_graph(e, g, tmp_path)
    first, second, invalid, isolated = _kinds(g)
    valid = np.flatnonzero(g.state != fg.INVALID)
    sets = {"one": [first], "two components": [first, second],
            "five with a duplicate": [int(valid[-2]), first, int(valid[len(valid) // 2]), first, second],
            "Invalid and isolated": [invalid, isolated, first], "all nodes": list(range(x.V))}
    refs = dict(zip(sets, _refs(x, list(sets.values()))))
    assert np.array_equal(refs["all nodes"].owner, np.arange(x.V)) and np.all(refs["all nodes"].hops == 0)
    assert refs["Invalid and isolated"].owned[1] == 1 and refs["five with a duplicate"].owned[3] == 0
    assert len(set(refs["two components"].owner.tolist())) == 3  # both own nodes, some node is unreached
    targets = [first, isolated, invalid, x.V // 2, first]
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        for kind, s in sets.items():
            _check(e, [refs[kind]], [s], f"seed {seed}, width {scale}, set {kind}: ", targets=targets)
        r = _check(e, list(refs.values()), list(sets.values()), f"seed {seed}, width {scale}, five sets: ",
                   targets=targets)
        assert np.array_equal(r["owner"][4], np.arange(x.V))
        _check(e, list(refs.values()), list(sets.values()), f"seed {seed}, width {scale}, at the targets: ",
               targets=targets, full=False)
    e.set_option("field_delta_scale", "4")


def test_batches(engine, tmp_path):
    """The MULTI kernels: 3 sets of 1 / 4 / 9 entries in one solve, and 64 one- and two-member sets on 44 nodes."""
    e = engine
    g = with_isolated_node(fg.with_positions(fg.random_small(13)))
    x = load_graph(e, g, tmp_path)
    assert x.V == 44
    first, second, invalid, isolated = _kinds(g)
    three = [[second], [first, invalid, second, first], [(5 * i + 2) % x.V for i in range(9)]]
    many = [[k % x.V] if k % 2 else [k % x.V, (3 * k + 1) % x.V] for k in range(64)]
    refs3, refs64 = _refs(x, three), _refs(x, many)
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        _check(e, refs3, three, f"width {scale}, sets of 1 / 4 / 9: ", targets=[0, isolated, 7])
        _check(e, refs64, many, f"width {scale}, 64 sets: ", targets=[isolated, 3])
    e.set_option("field_delta_scale", "4")


def test_lattice_ties(engine, tmp_path):
    """Every edge the same cost: whole diagonals are equally dear from two members, the parent rule decides."""
    e = engine
    x = load_graph(e, fg.lattice(20, 20), tmp_path)
    members = [399, 0, 210, 19, 380]  # the corners and the centre
    f = set_ref.set_field(x, SF, members)
    one = np.stack(reference_fields_cost(x, members))
    ties = np.sum(np.sum(one == f.cost, axis=0) > 1)
    assert ties >= 10 and np.all(f.owned > 0), (ties, f.owned)
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        _check(e, [f], [members], f"lattice, width {scale}: ", targets=[0, 199, 200, 399])
    e.set_option("field_delta_scale", "4")


def reference_fields_cost(x, members):
    """The members' single fields' costs, from the set reference with one member each."""
    return [set_ref.set_field(x, SF, [s]).cost for s in members]


@pytest.mark.parametrize("scale", ["4", "inf"])
def test_long_chain(engine, tmp_path, scale):
    """7 999 hops: the owner pass must double its way there (13 doublings and a sweep that moves nothing), in waits
    that a launch per hop would not fit in."""
    e = engine
    e.set_option("field_delta_scale", scale)
    x = load_graph(e, fg.chain(8000), tmp_path)
    f = set_ref.set_field(x, SF, [0])
    assert f.hops[7999] == 7999
    r = _check(e, [f], [[0]], f"chain, width {scale}, one member: ", targets=[7999, 0])
    print(f"chain(8000), width {scale}: {r['info'].rounds} rounds, {r['info'].host_syncs} host waits")
    # without owners, then a route: the late owner pass reports its sweeps
    st, info, _ = _raw(e, [[0]], targets=[7999], cost_at=True)
    assert st == 0
    got, rinfo = e.routes([0], [7999], xyz=False, hops_at=[7999], with_info=True)
    assert np.array_equal(got[0][0], np.arange(8000)) and got[0][2].num_nodes == 8000
    assert 14 <= rinfo.rounds <= 16, rinfo.rounds  # 2^13 >= 7 999, one sweep to see it, whole batches of 8
    assert rinfo.host_syncs <= 4, rinfo.host_syncs  # two batches of sweeps, the lengths, the routes
    both = [0, 7999]
    _check(e, _refs(x, [both]), [both], f"chain, width {scale}, both ends: ", targets=[7999, 4000])
    xs = load_graph(e, fg.chain(8000, symmetric=True), tmp_path, "sym")
    fs = set_ref.set_field(xs, SF, both)
    assert fs.owned.min() > 1000 and fs.hops.max() > 2000
    _check(e, [fs], [both], f"symmetric chain, width {scale}, both ends: ", targets=[7999, 4000])
    e.set_option("field_delta_scale", "4")


@pytest.mark.parametrize("scale", ["4", "inf"])
def test_long_row(engine, tmp_path, scale):
    e = engine
    e.set_option("field_delta_scale", scale)
    x = load_graph(e, fg.star(30000), tmp_path)
    members = [0, 1, 15000]
    f = set_ref.set_field(x, SF, members)
    assert np.all(f.owned > 0), f.owned
    _check(e, [f], [members], f"star, width {scale}: ", targets=[30000, 2, 14999])
    e.set_option("field_delta_scale", "4")


def test_saturation_and_zero_costs(engine, tmp_path):
    e = engine
    x = load_graph(e, fg.saturating_branch(), tmp_path)
    sets = [[0], [0, 7], [9, 0, 9]]
    refs = _refs(x, sets)
    at_inf = np.isposinf(refs[0].cost) & (refs[0].hops >= 0)
    assert at_inf.sum() >= 5 and np.all(refs[0].owner[at_inf] == 0)  # reached at +inf: owned like any other
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        _check(e, refs, sets, f"saturating_branch, width {scale}: ", targets=[6, 10, 11])
        for k in range(3):
            _check(e, [refs[k]], [sets[k]], f"saturating_branch, width {scale}, set {k}: ")
    x = load_graph(e, fg.all_zero(64), tmp_path, "zero")
    members = [5, 40, 5]
    f = set_ref.set_field(x, SF, members)
    assert np.all(f.cost == 0) and np.sum(f.hops == 0) == 2 and f.hops.max() >= 2
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        _check(e, [f], [members], f"all_zero, width {scale}: ", targets=[0, 63])
    e.set_option("field_delta_scale", "4")


@pytest.mark.parametrize("how", ["full", "at_targets", "late"])
def test_routes(engine, tmp_path, how):
    """Routes to every node of two set fields: full -- parents and owners came back with the solve; at_targets --
    no parent output, the owners asked for; late -- neither: the first routes call runs both sweeps."""
    e = engine
    e.set_option("field_delta_scale", "4")
    g = with_isolated_node(fg.with_positions(fg.random_small(13)))
    x = load_graph(e, g, tmp_path)
    first, second, invalid, isolated = _kinds(g)
    sets = [[second, first, 20, first], [invalid, 30]]
    refs = _refs(x, sets)
    if how == "late":
        st, info, _ = _raw(e, sets, targets=[0], cost_at=True)
        assert st == 0 and info.reached == sum(int((f.hops >= 0).sum()) for f in refs)
    else:
        _check(e, refs, sets, f"routes {how}: ", targets=[0, isolated], full=how == "full")
    pairs = [(k, t) for k in range(2) for t in range(x.V)]
    costs = route_ref.edge_costs(x.col, x.w, x.dist, x.state, SF)
    got, info = e.routes([k for k, _ in pairs], [t for _, t in pairs], hops_at=[refs[k].hops[t] for k, t in pairs],
                         with_info=True)
    assert (info.rounds > 0) == (how == "late"), info.rounds  # the owner pass ran in this call, or had run
    unreached = 0
    for (k, t), (ids, pts, one) in zip(pairs, got):
        f = refs[k]
        at = f"routes {how}, set {k}, target {t}: "
        if f.hops[t] < 0:
            unreached += 1
            assert one.num_nodes == 0 and ids.size == 0 and np.isposinf(one.cost), at
            continue
        src = sets[k][f.owner[t]]
        w = route_ref.route(x.rowptr, x.col, x.w, x.dist, x.state, SF, f.cost, f.hops, f.parent, src, t, costs)
        assert np.array_equal(ids, w.ids), at + f"ids {ids.tolist()} != {w.ids.tolist()}"
        assert ids[0] == src and ids[-1] == t and one.num_nodes == len(w.ids), at
        assert np.array_equal(bits(pts), bits(x.xyz[w.ids])), at
        for nm in ("cost", "path_length", "avg_risk"):
            assert _b1(getattr(one, nm)) == _b1(getattr(w, nm)), at + nm
    assert unreached > 2
    # the reached list of a set solve
    for k in range(2):
        want = np.flatnonzero(refs[k].hops >= 0)
        ids, cost, hops = e.field_reached(k)
        assert np.array_equal(ids, want) and np.array_equal(bits(cost), bits(refs[k].cost[want])), k
        assert np.array_equal(hops, refs[k].hops[want]), k


def test_single_sources_as_sets_of_one(engine, tmp_path):
    """The two paths share their init, gather and walk kernels: three single sources -- one valid node of each
    component and the isolated node -- solved by cost_fields and as three sets of one by cost_fields_from give the
    same fields and the same routes to every node.  Only the equivalence is asserted; either side's values are
    checked against field_ref / set_ref elsewhere."""
    e = engine
    e.set_option("field_delta_scale", "4")
    g = with_isolated_node(fg.with_positions(fg.random_small(13)))
    x = load_graph(e, g, tmp_path)
    assert x.V == 44
    first, second, _, isolated = _kinds(g)
    sources = [first, second, isolated]
    targets = [first, isolated, second, x.V // 2, 0]
    pairs = [(k, t) for k in range(3) for t in range(x.V)]

    def solve(call):
        r = call()
        routes = e.routes([k for k, _ in pairs], [t for _, t in pairs], hops_at=r["hops"].reshape(-1))
        return r, routes

    a, routes_a = solve(lambda: e.cost_fields(source_ids=sources, targets=targets, full=True))
    b, routes_b = solve(lambda: e.cost_fields_from([[s] for s in sources], targets=targets, full=True))
    assert np.array_equal(a["sources"], b["sources"]) and a["sources"].tolist() == sources
    assert_rows("sets of one: ", "costs", b["cost"], a["cost"], as_bits=True)
    for name in ("hops", "parent"):
        assert_rows("sets of one: ", name, b[name], a[name])
    assert np.array_equal(a["reached"], b["reached"]), (a["reached"], b["reached"])
    assert a["reached"][2] == 1 and np.all(a["reached"][:2] > 1)  # the isolated node reaches itself only
    assert np.array_equal(bits(a["cost_at"]), bits(b["cost_at"])) and np.array_equal(a["hops_at"], b["hops_at"])
    assert np.array_equal(b["owner"], np.where(b["hops"] >= 0, 0, -1)), b["owner"]
    assert np.array_equal(b["owner_at"], np.where(b["hops_at"] >= 0, 0, -1)), b["owner_at"]
    assert len(routes_a) == len(routes_b) == len(pairs)
    for (k, t), (ids_a, xyz_a, one_a), (ids_b, xyz_b, one_b) in zip(pairs, routes_a, routes_b):
        at = f"sets of one, field {k}, target {t}: "
        assert np.array_equal(ids_a, ids_b), at + f"ids {ids_a.tolist()} != {ids_b.tolist()}"
        assert np.array_equal(bits(xyz_a), bits(xyz_b)), at
        assert one_a.num_nodes == one_b.num_nodes == ids_a.size == a["hops"][k, t] + 1, at
        for nm in ("cost", "path_length", "avg_risk"):
            assert _b1(getattr(one_a, nm)) == _b1(getattr(one_b, nm)), at + nm


BOUND_GRAPHS = {"random_small_7": (lambda: fg.with_positions(fg.random_small(7)), None),
                "chain_3000": (lambda: fg.chain(3000), [0, 1700])}


@pytest.mark.parametrize("name", sorted(BOUND_GRAPHS))
def test_bounds(engine, tmp_path, name):
    e = engine
    make, members = BOUND_GRAPHS[name]
    x = load_graph(e, make(), tmp_path)
    if members is None:
        valid = np.flatnonzero(x.state != fg.INVALID)
        members = [int(valid[0]), int(valid[len(valid) // 3])]
    f = set_ref.set_field(x, SF, members)
    assert np.all(f.owned > 1)
    reach = np.flatnonzero((f.hops > 0) & np.isfinite(f.cost))
    reach = reach[np.argsort(f.cost[reach], kind="stable")]
    targets = [int(reach[reach.size // 2]), int(reach[reach.size // 5]), int(reach[reach.size // 2])]
    budgets = bound_ref.five_budgets(f.cost, f.hops)
    for scale in (SCALES if name != "chain_3000" else ("4", "inf")):
        e.set_option("field_delta_scale", scale)
        for budget in budgets:
            for settle in (None, "any", "all"):
                r = _check(e, [f], [members], f"{name}, width {scale}, budget {budget!r}, settle {settle}: ",
                           budget=budget, settle=settle, targets=targets)
                if budget == 0:
                    assert r["reached"][0] == int(np.sum((f.hops >= 0) & (f.cost == 0)))
        for settle in ("any", "all"):
            r = _check(e, [f], [members], f"{name}, width {scale}, settle {settle}: ", settle=settle, targets=targets,
                       full=False)
            assert np.isfinite(r["bound"][0]) and r["reached"][0] < int((f.hops >= 0).sum())
    e.set_option("field_delta_scale", "4")


def test_it_really_stops(engine, tmp_path):
    """The unit chain of 4 096 nodes, both ways, from both ends under the budget of node 40's cost: 41 nodes from each
    end, and rounds of that order.  Unbounded, nodes 2 047 and 2 048 lie 2 047 tight hops from their ends and a node
    at depth d is expanded in round d at the earliest: 2 048 working rounds per pass."""
    e = engine
    e.set_option("field_delta_scale", "4")
    a = np.arange(4095)
    g = fg.from_edges(4096, np.concatenate([a, a + 1]), np.concatenate([a + 1, a]), np.zeros(8190), np.ones(8190))
    x = load_graph(e, g, tmp_path)
    members = [0, 4095]
    f = set_ref.set_field(x, SF, members)
    assert f.cost[40] == 40 and f.hops[4055] == 40 and f.owner[2047] == 0 and f.owner[2048] == 1
    r = _check(e, [f], [members], "unit chain, budget: ", budget=f.cost[40])
    u = _check(e, [f], [members], "unit chain, unbounded: ")
    print(f"unit chain from both ends: {r['info'].rounds} rounds under the budget, {u['info'].rounds} unbounded")
    assert r["reached"][0] == 82 and r["owned"][0].tolist() == [41, 41]
    assert r["info"].rounds < 400, r["info"].rounds
    assert u["info"].rounds >= 2 * 2048, u["info"].rounds


def _hand_graph(tmp_path, e, frontier=True):
    """A line 0 .. 8 of unit-cost edges, both ways, with Frontier nodes 0, 2, 4, 6, 8, and a second component 9 - 10
    without one.  From nodes 1 and 7 node 4 is equally dear, with equal hops."""
    F = 1 if frontier else 0
    nodes = [((2.0 * i, 0.0, 0.0), F if i % 2 == 0 else 0) for i in range(9)]
    nodes += [((0.0, 10.0, 0.0), 0), ((2.0, 10.0, 0.0), 0)]
    edges = []
    for a, b in [(i, i + 1) for i in range(8)] + [(9, 10)]:
        edges += [(a, b, 0.0, 1.0), (b, a, 0.0, 1.0)]
    p = tmp_path / ("hand.json" if frontier else "hand_plain.json")
    write_graph(p, nodes, edges)
    e.load_json(str(p))
    return e.graph("global")


def test_python_helpers(engine, tmp_path):
    e = engine
    e.set_option("field_delta_scale", "4")
    x = _hand_graph(tmp_path, e)
    assert x.V == 11 and np.flatnonzero(x.state == 1).tolist() == [0, 2, 4, 6, 8]
    f = set_ref.set_field(x, SF, [1, 7, 9])
    assert f.owner.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2] and f.cost[4] == 3  # (4: parents 3 and 5 tie, 3 wins)
    cost, hops, owner, nodes = e.nearest_source([1, 7, 9])
    assert nodes.tolist() == [1, 7, 9] and np.array_equal(owner, f.owner) and np.array_equal(hops, f.hops)
    assert np.array_equal(bits(cost), bits(f.cost))
    xy = x.xyz[[1, 7, 9], :2] + F32(0.1)
    cost, hops, owner, nodes = e.nearest_source(xy, targets=[4, 10, 0])
    assert nodes.tolist() == [1, 7, 9] and owner.tolist() == [0, 2, 0] and hops.tolist() == [3, 1, 1]
    assert np.array_equal(bits(cost), bits(f.cost[[4, 10, 0]]))
    cost, hops, owner, _ = e.nearest_source([1, 7], budget=2.0)
    assert owner.tolist() == [0, 0, 0, 0, -1, 1, 1, 1, 1, -1, -1] and np.isposinf(cost[4]) and hops[4] == -1
    # three poses: the third stands in the component without a Frontier node
    got = e.assign_frontiers(xy)
    assert [o.tolist() for o, _ in got] == [[0, 2, 4], [6, 8], []]
    assert got[0][1] == (0, 1.0, [1, 0]) and got[1][1] == (6, 1.0, [7, 6]) and got[2][1] is None
    # two poses on one node: the first owns all of it
    got = e.assign_frontiers(np.concatenate([xy[:2], xy[:1] - F32(0.2), xy[2:]]))
    assert [o.tolist() for o, _ in got] == [[0, 2, 4], [6, 8], [], []]
    assert got[0][1] == (0, 1.0, [1, 0]) and got[2][1] is None and got[3][1] is None
    # a budget: node 4 is out of reach for both
    got = e.assign_frontiers(xy[:2], budget=2.0)
    assert [o.tolist() for o, _ in got] == [[0, 2], [6, 8]]
    # no Frontier node at all
    _hand_graph(tmp_path, e, frontier=False)
    got = e.assign_frontiers(xy)
    assert len(got) == 3 and all(o.size == 0 and o.dtype == np.int32 and p is None for o, p in got)


def test_errors(engine, tmp_path):
    import trg_planner
    e = engine
    x = load_graph(e, fg.with_positions(fg.random_small(1)), tmp_path)

    def refused(**kw):
        with pytest.raises(trg_planner.TrgError) as ei:
            e._chk(_raw(e, None, **kw)[0])
        assert ei.value.status == INVALID_ARG, str(ei.value)
        return str(ei.value)

    ok_ptr, ok_ids = [0, 1, 3], [0, 1, 2]
    assert "0 sets" in refused(ptr=ok_ptr, ids=ok_ids, m=0)
    assert "65 sets" in refused(ptr=list(range(66)), ids=[0] * 65)
    assert "set_ptr[0] is 1" in refused(ptr=[1, 2, 3], ids=ok_ids)
    assert "set 1 is empty" in refused(ptr=[0, 2, 2], ids=ok_ids)
    assert "set 1 is empty or set_ptr descends" in refused(ptr=[0, 2, 1], ids=ok_ids)
    msg = refused(ptr=ok_ptr, ids=[0, 1, x.V])
    assert "entry 1 of set 1" in msg and f"node {x.V}" in msg
    assert "entry 0 of set 0" in refused(ptr=ok_ptr, ids=[-1, 1, 2])
    assert "target 1" in refused(ptr=ok_ptr, ids=ok_ids, targets=[0, x.V], cost_at=True)
    assert "n_targets < 0" in refused(ptr=ok_ptr, ids=ok_ids, n_targets=-1)
    assert "field 1" in refused(ptr=ok_ptr, ids=ok_ids, budget=[1.0, -1.0])
    assert "settle mode 3" in refused(ptr=ok_ptr, ids=ok_ids, settle=3, targets=[0])
    assert "needs targets" in refused(ptr=ok_ptr, ids=ok_ids, settle=1)
    with pytest.raises(ValueError):
        e.cost_fields_from([[0]], settle="some")
    with pytest.raises(trg_planner.TrgError) as ei:
        e.cost_fields_from([[0], []])
    assert ei.value.status == INVALID_ARG and "set 1" in str(ei.value)
    # the call still works after the refusals
    _check(e, _refs(x, [[0], [1, 2]]), [[0], [1, 2]], "after the refusals: ")


def test_staleness_and_unchanged_paths(ref, engine, tmp_path):
    import trg_planner
    e = engine
    e.set_option("field_delta_scale", "4")
    g = fg.with_positions(fg.random_small(7))
    x = load_graph(e, g, tmp_path)
    valid = np.flatnonzero(x.state != fg.INVALID)
    sets = [[int(valid[0]), int(valid[-1])], [int(valid[1])]]
    _check(e, _refs(x, sets), sets, "before the batch: ")
    # a plain batch right after a set solve, on the same buffers: the reference's fields, routes to single sources
    sources = [int(valid[-1]), int(valid[0]), int(valid[2])]
    rc, rh, rp = reference_fields(ref, x, SF, sources)
    r = e.cost_fields(source_ids=sources, targets=sources)
    assert_rows("batch after sets: ", "costs", r["cost"], rc, as_bits=True)
    assert_rows("batch after sets: ", "hops", r["hops"], rh)
    assert_rows("batch after sets: ", "parents", r["parent"], rp)
    pairs = [(k, t) for k in range(3) for t in range(x.V)]
    want = route_ref.routes_of_graph(x, SF, [(sources[k], rc[k], rh[k], rp[k]) for k in range(3)], pairs)
    got, info = e.routes([k for k, _ in pairs], [t for _, t in pairs], xyz=False, hops_at=rh.reshape(-1),
                         with_info=True)
    assert info.rounds == 0
    for (k, t), (ids, _, one), w in zip(pairs, got, want):
        assert np.array_equal(ids, w.ids) and (ids.size == 0 or ids[0] == sources[k]), (k, t)
        assert _b1(one.cost) == _b1(w.cost) and _b1(one.path_length) == _b1(w.path_length), (k, t)
    # and a set solve after the batch
    _check(e, _refs(x, sets), sets, "after the batch: ", targets=sources)
    load_graph(e, g, tmp_path, "again")
    for call in (lambda: e.routes([0], [0]), lambda: e.field_reached(0)):
        with pytest.raises(trg_planner.TrgError) as ei:
            call()
        assert ei.value.status == INVALID_ARG and "earlier graph" in str(ei.value)
