"""GPU: routes of the cost field (trg_engine_field_routes, Engine.routes, Engine.plan_many): the paths behind the
keys of the last solve, walked on the device.  Every route is compared with tests/route_ref.py on the host
Dijkstra's field, exactly: node ids and offsets equal, cost / path_length / avg_risk as bits, positions as the
bits of the nodes' positions.  No tolerance anywhere.

The graphs are those of tests/field_graphs.py through load_json, at the smallest shapes where the walk can go
wrong: V ~ 30 with every (field, node) pair as a route (unreachable, Invalid, duplicate-edge and source-equals-
target routes), the degenerate shapes, one route of 3 000 nodes, a 30 000-long row to search for the route edge,
four hubs, a lattice of exact ties, folds that saturate, and 11 200 routes in one call (more than one pass of the
grid).  Then the capacity rule, the retained solve, the error cases, and plan_many on a device-built graph before
and after an updateGraph."""
import ctypes as C

import numpy as np
import pytest

import field_graphs as fg
import field_ref
import route_ref
from field_support import (INVALID_ARG, MOUNTAIN, PARAMS, bits, engine, load_graph, random_large, ref,  # noqa: F401
                           reference_fields, small_sources, with_isolated_node)
from graph_support import obs_crop

pytestmark = pytest.mark.gpu
F32 = np.float32
SF = 3.0
FIELD_DELTA_SCALE = "4"  # of this module's `engine`


def _reference_fields(ref, x, sources):
    return reference_fields(ref, x, SF, sources, stacked=False)


def _raw(e, fields, targets, cap, ids=True, xyz=False):
    """One trg_engine_field_routes call -> (offsets, ids[:cap] or None, xyz or None, infos, TrgFieldInfo)."""
    from trg_planner._engine import TrgFieldInfo, TrgRouteInfo, _f, _i
    f = np.ascontiguousarray(fields, np.int32)
    t = np.ascontiguousarray(targets, np.int32)
    n = f.shape[0]
    off = np.full(n + 1, -7, np.int32)
    out_ids = np.full(max(cap, 1), -7, np.int32) if ids else None
    out_xyz = np.full((max(cap, 1), 3), np.nan, np.float32) if xyz else None
    infos = (TrgRouteInfo * max(n, 1))()
    info = TrgFieldInfo()
    e._chk(e.L.trg_engine_field_routes(e.h, n, _i(f), _i(t), _i(off), None if out_ids is None else _i(out_ids),
                                       None if out_xyz is None else _f(out_xyz), cap, infos, C.byref(info)))
    return off, out_ids, out_xyz, [infos[r] for r in range(n)], info


def _assert_info(at, got, want):
    assert got.num_nodes == len(want.ids), at + f"num_nodes {got.num_nodes} != {len(want.ids)}"
    for name in ("cost", "path_length", "avg_risk"):
        a, b = F32(getattr(got, name)), F32(getattr(want, name))
        assert bits(a)[0] == bits(b)[0], at + f"{name} {a!r} != {b!r}"


def _check_routes(e, x, fields_ref, pairs):
    """Engine.routes for `pairs` of (field, target) on the engine's last solve against the reference."""
    pairs = [(int(f), int(t)) for f, t in pairs]
    want = route_ref.routes_of_graph(x, SF, fields_ref, pairs)
    got, info = e.routes([f for f, _ in pairs], [t for _, t in pairs], with_info=True)
    assert len(got) == len(want)
    for (f, t), (ids, pts, one), w in zip(pairs, got, want):
        at = f"field {f} (source {fields_ref[f][0]}), target {t}: "
        assert np.array_equal(ids, w.ids), at + f"ids {ids.tolist()} != {w.ids.tolist()}"
        assert pts.shape == (len(w.ids), 3) and np.array_equal(bits(pts), bits(x.xyz[w.ids])), at + "positions"
        _assert_info(at, one, w)
    assert 1 <= info.host_syncs <= 2, info.host_syncs
    return want, got


def _solve(e, sources, full=False, targets=None):
    return e.cost_fields(source_ids=[int(s) for s in sources], full=full, targets=targets)


@pytest.mark.parametrize("m", [1, 5, 64])
@pytest.mark.parametrize("seed", [0, 7, 13])
def test_random_small(ref, engine, tmp_path, seed, m):
    """Every (field, node) pair as a route."""
    g = with_isolated_node(fg.with_positions(fg.random_small(seed)))
    x = load_graph(engine, g, tmp_path)
    sources = small_sources(g, m, seed)
    fields_ref = _reference_fields(ref, x, sources)
    _solve(engine, sources)
    pairs = [(k, t) for k in range(m) for t in range(x.V)]
    assert len(pairs) <= 64 * 49
    want, _ = _check_routes(engine, x, fields_ref, pairs)
    lengths = [len(w.ids) for w in want]
    assert 0 in lengths and 1 in lengths and max(lengths) >= 3


ODDITIES = fg.oddities()


@pytest.mark.parametrize("name", sorted(ODDITIES))
def test_oddities(ref, engine, tmp_path, name):
    g, sources = ODDITIES[name]
    x = load_graph(engine, g, tmp_path)
    sources = (list(sources) * 3)[:3]
    fields_ref = _reference_fields(ref, x, sources)
    _solve(engine, sources)
    want, got = _check_routes(engine, x, fields_ref, [(k, t) for k in range(3) for t in range(x.V)])
    if name == "triple_duplicates":
        # 1 -> 2: weights 0.9, 0.1, 0.4, only the middle edge is tight; 3 -> 0: 0.2, 0.2, 0.1, only the last
        assert sources == [0, 1, 3]
        one = got[1 * x.V + 2][2]
        assert one.num_nodes == 2 and F32(one.avg_risk) == F32(F32(0.1) / F32(2.0)) and one.path_length == 1.0
        one = got[2 * x.V + 0][2]
        assert one.num_nodes == 2 and F32(one.avg_risk) == F32(F32(0.1) / F32(2.0))
    if name == "one_node":
        assert [(r[0].tolist(), r[2].num_nodes, r[2].cost) for r in got] == [([0], 1, 0.0)] * 3


@pytest.mark.parametrize("symmetric", [False, True], ids=["directed", "symmetric"])
def test_chain(ref, engine, tmp_path, symmetric):
    """One route of 3 000 nodes (field 0 to the last node), and what the other three fields reach of it."""
    V = 3000
    x = load_graph(engine, fg.chain(V, symmetric), tmp_path)
    sources = [0, V - 1, V // 2, V - 2]
    fields_ref = _reference_fields(ref, x, sources)
    _solve(engine, sources)
    want, _ = _check_routes(engine, x, fields_ref, [(0, V - 1), (1, 0), (2, V - 1), (2, 0), (3, V - 1), (0, 0)])
    assert len(want[0].ids) == V and len(want[1].ids) == (V if symmetric else 0)


def test_star_long_row(ref, engine, tmp_path):
    """Leaf -> hub -> leaf: the route edge out of the hub is searched in a row of 30 000."""
    deg = 30000
    x = load_graph(engine, fg.star(deg), tmp_path)
    sources = [1, 1 + deg // 2, 0]
    fields_ref = _reference_fields(ref, x, sources)
    _solve(engine, sources)
    _, _, hops, parent = fields_ref[0]
    via_hub = np.flatnonzero((hops == 2) & (parent == 0))  # leaf 1 -> hub -> leaf
    assert via_hub.size >= 2
    far = [int(via_hub[0]), int(via_hub[-1]), 1 + deg // 3, deg, 1 + deg // 2 + 1, 2, 0, 1]
    want, _ = _check_routes(engine, x, fields_ref, [(k, t) for k in range(3) for t in far])
    assert want[0].ids.tolist() == [1, 0, far[0]] and want[1].ids.tolist() == [1, 0, far[1]]


def test_star_four_hubs(ref, engine, tmp_path):
    x = load_graph(engine, fg.star(4096, 4), tmp_path)
    sources = [x.V - 1, 0, 4 + 4096 // 3]
    fields_ref = _reference_fields(ref, x, sources)
    _solve(engine, sources)
    targets = [0, 1, 2, 3, 4, 5, 6, 7, 4 + 4095, 4 + 2048, 4 + 1001, x.V - 1]
    _check_routes(engine, x, fields_ref, [(k, t) for k in range(3) for t in targets])


def test_lattice(ref, engine, tmp_path):
    """Exact ties everywhere: the smallest-parent rule decides every step of every route."""
    n = 200
    x = load_graph(engine, fg.lattice(n, n), tmp_path)
    centre = (n // 2) * n + n // 2
    sources = [0, n - 1, n * (n - 1), n * n - 1, centre, 0, n // 2, centre + 1]
    fields_ref = _reference_fields(ref, x, sources)
    _solve(engine, sources)
    targets = [0, n - 1, n * (n - 1), n * n - 1, centre]
    want, _ = _check_routes(engine, x, fields_ref, [(k, t) for k in range(8) for t in targets])
    assert len(want[3].ids) == 2 * (n - 1) + 1  # field 0 to the opposite corner


@pytest.mark.parametrize("name", ["saturating_chain", "saturating_branch"])
def test_saturating(ref, engine, tmp_path, name):
    """Routes to nodes reached at +inf."""
    x = load_graph(engine, getattr(fg, name)(), tmp_path)
    sources = [0, 2, 1]
    fields_ref = _reference_fields(ref, x, sources)
    _solve(engine, sources)
    want, _ = _check_routes(engine, x, fields_ref, [(k, t) for k in range(3) for t in range(x.V)])
    assert any(np.isposinf(w.cost) and len(w.ids) > 1 for w in want)


LARGE = fg.RANDOM_LARGE[2000][2]  # V = 1 950


def test_random_large(ref, engine, tmp_path):
    """16 fields x 700 random targets with duplicates: 11 200 routes, more groups than one pass of the grid."""
    x = load_graph(engine, random_large(*LARGE), tmp_path)
    V = x.V
    sources = [0, V - 1, V // 4, 0] + [int(s) for s in np.random.default_rng(16).integers(0, V, size=12)]
    fields_ref = _reference_fields(ref, x, sources)
    targets = np.random.default_rng(3).integers(0, V, size=700)
    r = _solve(engine, sources, targets=targets)
    pairs = [(k, int(t)) for k in range(16) for t in targets]
    want = route_ref.routes_of_graph(x, SF, fields_ref, pairs)
    hops_at = r["hops_at"].reshape(-1)
    assert np.array_equal(hops_at + 1, [len(w.ids) for w in want])
    got, info = engine.routes([f for f, _ in pairs], [t for _, t in pairs], hops_at=hops_at, with_info=True)
    for (f, t), (ids, pts, one), w in zip(pairs, got, want):
        at = f"field {f}, target {t}: "
        assert np.array_equal(ids, w.ids), at
        assert np.array_equal(bits(pts), bits(x.xyz[w.ids])), at
        _assert_info(at, one, w)
    assert info.host_syncs <= 2


def test_capacity(ref, engine, tmp_path):
    """cap at the total, one below it, in the middle of a route and at 0."""
    x = load_graph(engine, fg.with_positions(fg.random_small(7)), tmp_path)
    sources = [int(np.flatnonzero(x.state != fg.INVALID)[0]), x.V // 2]
    fields_ref = _reference_fields(ref, x, sources)
    solve = _solve(engine, sources)
    reach = [t for t in range(x.V) if fields_ref[0][2][t] >= 2][:4]
    unreached = [t for t in range(x.V) if fields_ref[0][2][t] < 0][:1]
    assert len(reach) == 4 and unreached
    pairs = [(0, reach[0]), (0, unreached[0]), (0, reach[1]), (1, sources[1]), (0, reach[2]), (0, reach[3])]
    want = route_ref.routes_of_graph(x, SF, fields_ref, pairs)
    lens = [len(w.ids) for w in want]
    total = sum(lens)
    full_off = np.concatenate([[0], np.cumsum(lens)])
    full_ids = np.concatenate([w.ids for w in want])
    f, t = [p[0] for p in pairs], [p[1] for p in pairs]
    for cap in (total, total - 1, int(full_off[3]) - 1, int(full_off[5]) + 1, 1, 0):
        off, ids, pts, infos, info = _raw(engine, f, t, cap, xyz=True)
        at = f"cap {cap}: "
        assert np.array_equal(off, np.minimum(full_off, cap)), at + str(off)
        assert np.array_equal(ids[:off[-1]], full_ids[:min(cap, total)]), at  # a truncated route keeps its first nodes
        assert np.all(ids[off[-1]:] == -7), at + "ids written past the last offset"
        assert np.array_equal(bits(pts[:off[-1]]), bits(x.xyz[full_ids[:off[-1]]])), at
        for r, (one, w) in enumerate(zip(infos, want)):
            _assert_info(at + f"route {r}: ", one, w)  # full num_nodes and sums whatever fits
    # lengths only, then a second call with the right cap: complete, and no new solve
    off, ids, pts, infos, info = _raw(engine, f, t, 0, ids=False)
    assert not off.any() and info.host_syncs == 1 and info.rounds == 0
    cap = sum(i.num_nodes for i in infos)
    assert cap == total
    off, ids, pts, infos, info = _raw(engine, f, t, cap)
    assert np.array_equal(off, full_off) and np.array_equal(ids[:cap], full_ids)
    assert info.host_syncs == 2 < solve["info"].host_syncs and info.rounds == 0
    # ids without positions, positions without ids
    off, ids, pts, infos, info = _raw(engine, f, t, cap, ids=False, xyz=True)
    assert np.array_equal(off, full_off) and np.array_equal(bits(pts[:cap]), bits(x.xyz[full_ids]))
    # no routes at all
    off, ids, pts, infos, info = _raw(engine, [], [], 5)
    assert off.tolist() == [0]


def test_retained_solve(ref, engine, tmp_path):
    """Routes after a solve without parents (the sweep runs late) equal those after one with; two calls in a row
    are equal; after another solve the routes follow it."""
    x = load_graph(engine, fg.with_positions(fg.random_small(13)), tmp_path)
    valid = np.flatnonzero(x.state != fg.INVALID)
    sources = [int(valid[0]), int(valid[1]), int(valid[-1])]
    fields_ref = _reference_fields(ref, x, sources)
    pairs = [(k, t) for k in range(3) for t in range(x.V)]
    f, t = [p[0] for p in pairs], [p[1] for p in pairs]

    def snapshot():
        off, ids, _, infos, _ = _raw(engine, f, t, 3 * x.V * x.V)
        return (off.tolist(), ids[:off[-1]].tolist(),
                [(i.num_nodes, bits(i.cost)[0], bits(i.path_length)[0], bits(i.avg_risk)[0]) for i in infos])

    full = _solve(engine, sources, full=True)
    _check_routes(engine, x, fields_ref, pairs)
    with_parents = snapshot()
    _solve(engine, sources, full=False)
    _check_routes(engine, x, fields_ref, pairs)
    lazy = snapshot()
    assert lazy == with_parents and snapshot() == lazy
    # the single-source entry retains its solve too, with and without its parent output
    cost, hops, parent, _ = engine.cost_field(source_id=sources[2])
    assert np.array_equal(parent, full["parent"][2])
    _check_routes(engine, x, fields_ref[2:], [(0, t) for t in range(x.V)])
    # other sources: the routes follow the new solve
    other = [sources[2], sources[0]]
    other_ref = _reference_fields(ref, x, other)
    _solve(engine, other)
    _check_routes(engine, x, other_ref, [(k, t) for k in range(2) for t in range(x.V)])
    # and a later full solve's parents are those of the reference still (the late sweep left no trace)
    again = _solve(engine, sources, full=True)
    assert np.array_equal(again["parent"], full["parent"])


def test_errors(ref, tmp_path, mountain_small):
    import trg_planner
    e = trg_planner.Engine(safety_factor=SF, **PARAMS)

    def refused(fields, targets, cap=16):
        with pytest.raises(trg_planner.TrgError) as ei:
            _raw(e, fields, targets, cap)
        assert ei.value.status == INVALID_ARG, str(ei.value)
        return str(ei.value)

    g = fg.with_positions(fg.random_small(1))
    x = load_graph(e, g, tmp_path)
    assert "no cost-field solve" in refused([0], [0])  # before any solve
    sources = [0, x.V - 1]
    fields_ref = _reference_fields(ref, x, sources)
    _solve(e, sources)
    _check_routes(e, x, fields_ref, [(0, 0), (1, 1)])
    msg = refused([0, 2, 0], [0, 0, 0])  # field index m
    assert "field 2" in msg and "route 1" in msg, msg
    msg = refused([0, 1], [0, x.V])     # target V
    assert f"target {x.V}" in msg and "route 1" in msg, msg
    assert "field -1" in refused([-1], [0]) and "target -1" in refused([0], [-1])
    refused([0], [0], cap=-1)
    with pytest.raises(trg_planner.TrgError) as ei:
        from trg_planner._engine import _i
        a = np.zeros(2, np.int32)
        e._chk(e.L.trg_engine_field_routes(e.h, -1, _i(a), _i(a), _i(a), None, None, 0, None, None))
    assert ei.value.status == INVALID_ARG
    _check_routes(e, x, fields_ref, [(k, t) for k in range(2) for t in range(x.V)])  # still works
    # the graph changes: the solve is gone until the next one
    x = load_graph(e, g, tmp_path, "again")
    assert "earlier graph" in refused([0], [0])
    _solve(e, sources)
    _check_routes(e, x, fields_ref, [(0, x.V - 1), (1, 0)])
    e.close()
    # update_graph on a built graph
    e = trg_planner.Engine(**MOUNTAIN)
    e.set_sampler(7, 16)
    e.set_global_map(mountain_small)
    e.init_graph([15.0, 15.0, 0.0])
    e.cost_fields(sources_xy=[(15.0, 15.0)], full=False)
    assert len(e.routes([0], [0])) == 1
    pose = (12.0, 12.0)
    e.set_local_map(pose, obs_crop(mountain_small, pose, 4.0, box=(pose[0] + 2.0, pose[1] + 1.0, 0.6)))
    e.update_graph()
    assert "earlier graph" in refused([0], [0])
    e.cost_fields(sources_xy=[(15.0, 15.0)], full=False)
    assert len(e.routes([0], [0])) == 1
    e.close()


def _plan_refold(e, g, costs, pose, goal_xyz, id_of):
    """Engine.plan's path as node ids and the fp32 fold of its edges' costs (per step the first relaxable edge of
    the row into the next node), or None where there is no path."""
    path, info = e.plan(pose, goal_xyz)
    if path.shape[0] == 0:
        return None
    ids = [id_of[p.tobytes()] for p in path]
    ec, ok = costs
    fold = F32(0.0)
    for a, b in zip(ids[:-1], ids[1:]):
        ks = np.arange(g.rowptr[a], g.rowptr[a + 1])
        ks = ks[(g.col[ks] == b) & ok[ks]]
        assert ks.size, f"the planned path steps {a} -> {b} without an edge"
        fold = F32(fold + ec[ks[0]])
    return ids, fold


def _resolve(e, xy):
    """The nodes the engine resolves positions to (trg_engine_cost_field_batch's resolve-only call)."""
    return e._resolve_nodes(xy)


def _check_plan_many(ref, e, g, poses, goals):
    costs = route_ref.edge_costs(g.col, g.w, g.dist, g.state, SF)
    id_of = {p.tobytes(): i for i, p in enumerate(g.xyz)}
    assert len(id_of) == g.V
    goal_nodes, starts = _resolve(e, goals), _resolve(e, poses)
    compared = reached = 0
    for pose, src in zip(poses, starts):
        st, rc, rh, rp = field_ref.field_of_graph(ref, g, SF, int(src))
        assert st == 0
        want = route_ref.routes_of_graph(g, SF, [(int(src), rc, rh, rp)], [(0, int(t)) for t in goal_nodes])
        got = e.plan_many(pose, goals)
        assert len(got) == len(goals)
        for j, ((pts, one), w) in enumerate(zip(got, want)):
            at = f"pose {pose.tolist()}, goal {j} (node {goal_nodes[j]}): "
            assert pts.shape == (len(w.ids), 3) and np.array_equal(bits(pts), bits(g.xyz[w.ids])), at
            _assert_info(at, one, w)
            reached += len(w.ids) > 0
            # A* on the same graph: its path is one walk, so its fp32 refold is no less than the field's cost at
            # the node where it ends (A* sums in double: equality is not asserted)
            planned = _plan_refold(e, g, costs, pose, [goals[j][0], goals[j][1], 0.0], id_of)
            if planned is not None:
                ids, fold = planned
                assert ids[0] == src, at
                assert fold >= rc[ids[-1]], at + f"refold {fold!r} < field cost {rc[ids[-1]]!r}"
                if ids[-1] == goal_nodes[j]:
                    assert fold >= F32(one.cost), at
                    compared += 1
    return reached, compared


def test_plan_many_device_built_graph(ref, mountain_small):
    import trg_planner
    e = trg_planner.Engine(**MOUNTAIN)
    e.set_sampler(7, 16)
    e.set_global_map(mountain_small)
    e.init_graph([15.0, 15.0, 0.0])
    assert e.stats()["used_device_bfs"] == 1, e.fallback_reason
    poses = np.array([(15.0, 15.0), (8.3, 21.7), (14.0, 16.0), (21.0, 9.5)], np.float32)
    g = e.graph("global")
    at_nodes = g.xyz[[g.V // 7, g.V // 3, g.V // 2, g.V - 1], :2]
    goals = np.concatenate([at_nodes, F32([(5.5, 6.25), (24.0, 22.0), (15.0, 15.0), (40.0, -3.0)])]).astype(np.float32)
    reached, compared = _check_plan_many(ref, e, g, poses, goals)
    print(f"device-built graph: {reached} routes with a path, {compared} compared with A* at the same goal node")
    assert reached >= 1 and compared >= 1
    pose = (12.0, 12.0)
    e.set_local_map(pose, obs_crop(mountain_small, pose, 4.0, box=(pose[0] + 2.0, pose[1] + 1.0, 0.6)))
    e.update_graph()
    g2 = e.graph("global")
    reached, compared = _check_plan_many(ref, e, g2, poses, goals)
    print(f"after updateGraph: {reached} routes with a path, {compared} compared with A* at the same goal node")
    assert reached >= 1 and compared >= 1
    e.close()
