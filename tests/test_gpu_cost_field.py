"""GPU: the cost field (trg_engine_cost_field, Engine.cost_field) against the host Dijkstra of
tests/cpp/field_reference.cpp on the same (cost, hops) key: cost (as bits), hops and parent equal, exactly.
Device-built graphs, host replay + updateGraph (the upload path and the graph_version cache), hand-written
JSON graphs with the error cases, agreement with planSafePath, the C3 graph at full size, and the pinned counts of
host waits and rounds."""
import numpy as np
import pytest

import field_graphs as fg
import field_ref
from field_support import MOUNTAIN, load_graph, ref, write_graph  # noqa: F401 (ref: a fixture)
from graph_support import obs_crop

pytestmark = pytest.mark.gpu
F32 = np.float32
def _check_against_reference(ref, e, g, src, cost, hops, parent, sf=3.0):
    st, rc, rh, rp = field_ref.field_of_graph(ref, g, sf, src)
    assert st == 0
    assert np.array_equal(cost.view(np.uint32), rc.view(np.uint32)), int((cost.view(np.uint32) != rc.view(np.uint32)).sum())
    assert np.array_equal(hops, rh), int((hops != rh).sum())
    assert np.array_equal(parent, rp), int((parent != rp).sum())
    return rc, rh, rp


def _node_of_xyz(g):
    return {tuple(p): i for i, p in enumerate(g.xyz.view(np.uint32).tolist())}


def _edge_cost(g, a, b, sf=3.0):
    """The least fp32 cost of the edges a -> b."""
    ks = np.arange(g.rowptr[a], g.rowptr[a + 1])
    ks = ks[g.col[ks] == b]
    assert ks.size, (a, b)
    return min((F32(sf) * g.w[k] + F32(1.0)) * g.dist[k] for k in ks)


def _fold(g, ids, sf=3.0):
    c = F32(0.0)
    for a, b in zip(ids[:-1], ids[1:]):
        c = F32(c + _edge_cost(g, a, b, sf))
    return c


def test_cost_field_device_built(ref, mountain_small):
    import trg_planner
    e = trg_planner.Engine(**MOUNTAIN)
    e.set_sampler(7, 16)
    e.set_global_map(mountain_small)
    e.init_graph([15.0, 15.0, 0.0])
    assert e.stats()["used_device_bfs"] == 1, e.fallback_reason
    g = e.graph("global")
    ids = _node_of_xyz(g)
    for xy in ((15.0, 15.0), (8.3, 21.7)):
        cost, hops, parent, info = e.cost_field(source_xy=xy)
        # the resolved source is planSafePath's start node for that xy
        path, _ = e.plan(xy, (20.0, 19.0, 0.0))
        assert path.shape[0] > 0
        assert info.source == ids[tuple(path[0].view(np.uint32).tolist())]
        _check_against_reference(ref, e, g, info.source, cost, hops, parent)
        assert info.reached == int((hops >= 0).sum()) and info.reached > g.V // 2
        assert 0 < info.rounds < 4 * g.V and info.ms_device > 0 and info.ms_total >= info.ms_device
    src = g.V // 3
    cost, hops, parent, info = e.cost_field(source_id=src)
    assert info.source == src
    _check_against_reference(ref, e, g, src, cost, hops, parent)


def test_cost_field_host_replay_and_updates(ref, mountain_gentle):
    import trg_planner
    prm = dict(MOUNTAIN, update_collision_threshold=0.2)
    e = trg_planner.Engine(**prm)
    e.set_sampler(5, 16)
    e.set_option("replay", "host")
    e.set_global_map(mountain_gentle)
    e.init_graph([15.0, 15.0, 0.0])
    g = e.graph("global")
    cost, hops, parent, info = e.cost_field(source_xy=(15.0, 15.0))
    _check_against_reference(ref, e, g, info.source, cost, hops, parent)
    sizes = {g.V}
    frontier_seen = False
    for pose in [(12.0, 12.0), (13.0, 12.5), (14.0, 13.0)]:
        obs = obs_crop(mountain_gentle, pose, 4.0, box=(pose[0] + 2.0, pose[1] + 1.0, 0.6))
        e.set_local_map(pose, obs)
        e.update_graph()
        g = e.graph("global")
        sizes.add(g.V)
        cost, hops, parent, info = e.cost_field(source_xy=pose)
        rc, rh, rp = _check_against_reference(ref, e, g, info.source, cost, hops, parent)
        # the cheapest Frontier node: least (cost, hops, id) of the reference's field
        fr = np.flatnonzero((g.state == 1) & np.isfinite(rc))
        best = e.cheapest_frontier(pose)
        if fr.size == 0:
            assert best is None
            continue
        frontier_seen = True
        want = int(fr[np.lexsort((fr, rh[fr], rc[fr]))[0]])
        node, c, path = best
        assert node == want and F32(c) == rc[want]
        assert path[0] == info.source and path[-1] == want and len(path) == rh[want] + 1
        assert _fold(g, path).view(np.uint32) == rc[want].view(np.uint32)
    assert len(sizes) > 1 and frontier_seen


def test_cost_field_json_graph(ref, tmp_path):
    import trg_planner
    nodes = [((0.0, 0.0, 0.0), 0), ((1.0, 0.0, 0.0), 0), ((2.0, 0.0, 0.0), 0), ((0.0, 1.0, 0.0), 0),
             ((0.0, 2.0, 0.0), -1), ((0.0, 3.0, 0.0), 0), ((9.0, 9.0, 0.0), 0), ((9.0, 8.0, 0.0), 1),
             ((-1.0, 0.0, 0.0), 1)]
    edges = [(0, 1, 0.0, 1.0),                     # directed only
             (1, 2, 0.5, 0.0), (2, 1, 0.5, 0.0),   # zero dist: cost 0
             (0, 3, 0.5, 1.0), (0, 3, 0.1, 1.0),   # duplicates, different weights
             (3, 4, 0.2, 1.0), (4, 3, 0.2, 1.0),   # 4 is Invalid: never entered ...
             (4, 5, 0.2, 1.0), (5, 4, 0.2, 1.0),   # ... so 5 is out of reach
             (6, 7, 0.3, 1.0), (7, 6, 0.3, 1.0),   # a second component
             (8, 0, 0.1, 1.0)]                     # directed only, towards the source
    p = tmp_path / "g.json"
    write_graph(p, nodes, edges)
    e = trg_planner.Engine(**MOUNTAIN)
    e.load_json(str(p))
    g = e.graph("global")
    cost, hops, parent, info = e.cost_field(source_id=0)
    c03 = (F32(3.0) * F32(0.1) + F32(1.0)) * F32(1.0)
    inf = np.inf
    assert np.array_equal(cost.view(np.uint32), np.array([0, 1, 1, c03, inf, inf, inf, inf, inf], np.float32).view(np.uint32))
    assert hops.tolist() == [0, 1, 2, 1, -1, -1, -1, -1, -1]
    assert parent.tolist() == [-1, 0, 1, 0, -1, -1, -1, -1, -1]
    assert info.source == 0 and info.reached == 4
    _check_against_reference(ref, e, g, 0, cost, hops, parent)
    # against the direction of 0 -> 1: from 2, node 1 costs 0 and node 0 is out of reach
    cost, hops, parent, info = e.cost_field(source_id=2)
    assert cost[1] == 0 and hops[1] == 1 and parent[1] == 2 and hops[0] == -1 and np.isinf(cost[0])
    _check_against_reference(ref, e, g, 2, cost, hops, parent)
    # field_path: the source alone, a path, and an unreachable node
    assert e.field_path(parent, 2) == [2]
    assert e.field_path(parent, 1) == [2, 1]
    with pytest.raises(ValueError):
        e.field_path(parent, 5)
    # a bad source id
    for bad in (g.V, -2):
        with pytest.raises(trg_planner.TrgError) as ei:
            e.cost_field(source_id=bad)
        assert ei.value.status == 1, str(ei.value)  # TRG_ERR_INVALID_ARG
    # an edge with safety_factor * weight + 1 < 0
    q = tmp_path / "neg.json"
    write_graph(q, nodes, edges + [(1, 2, -1.0, 1.0)])
    e.load_json(str(q))
    with pytest.raises(trg_planner.TrgError) as ei:
        e.cost_field(source_id=0)
    assert ei.value.status == 1, str(ei.value)
    # an empty graph
    r = tmp_path / "empty.json"
    write_graph(r, [], [])
    e.load_json(str(r))
    with pytest.raises(trg_planner.TrgError) as ei:
        e.cost_field(source_id=0)
    assert ei.value.status == 5, str(ei.value)  # TRG_ERR_NO_GRAPH
    e.close()


def test_cost_field_agrees_with_plan(ref, mountain_small):
    import trg_planner
    e = trg_planner.Engine(**MOUNTAIN)
    e.set_sampler(7, 16)
    e.set_global_map(mountain_small)
    e.init_graph([15.0, 15.0, 0.0])
    g = e.graph("global")
    ids = _node_of_xyz(g)
    start = (14.0, 16.0)
    cost, hops, parent, info = e.cost_field(source_xy=start)
    rng = np.random.default_rng(3)
    goals = rng.choice(np.flatnonzero(hops > 0), size=50, replace=False)
    checked = 0
    for gid in goals:
        path, _ = e.plan(start, g.xyz[gid])
        if path.shape[0] == 0:
            continue
        walk = [ids[tuple(p)] for p in path.view(np.uint32).tolist()]
        assert walk[0] == info.source
        goal = walk[-1]  # (setGoal may pick another node within robot_size)
        fold = _fold(g, walk)
        assert cost[goal] <= fold                      # the field is the least fold over ALL walks
        assert fold - cost[goal] <= F32(1e-4) * cost[goal]
        fp = e.field_path(parent, goal)
        assert fp[0] == info.source and len(fp) == hops[goal] + 1
        assert _fold(g, fp).view(np.uint32) == cost[goal].view(np.uint32)
        checked += 1
    assert checked >= 45


def test_cost_field_c3_fullsize(ref, synth):
    import trg_planner
    nx, ny = 3200, 3125
    cloud = synth.mountain_tile(0, nx, 0, ny, seed=20250418)
    prm = dict(MOUNTAIN, sample_num=16)
    e = trg_planner.Engine(**prm)
    e.set_sampler(7, 16)
    e.set_global_map(cloud)
    del cloud
    start = [nx * 0.05, ny * 0.05, 0.0]
    e.init_graph(start)
    assert e.stats()["used_device_bfs"] == 1, e.fallback_reason
    g = e.graph("global")
    assert g.V == 641812
    cost, hops, parent, info = e.cost_field(source_xy=start[:2])
    _check_against_reference(ref, e, g, info.source, cost, hops, parent)
    assert 0 < info.rounds < 4 * g.V
    print(f"C3 field: reached {info.reached} of {g.V}, {info.rounds} rounds, {info.host_syncs} host syncs, "
          f"{info.ms_device:.2f} ms device, {info.ms_total:.2f} ms total")


# (host_syncs, rounds) of the first solve on a freshly loaded graph and of the same solve repeated, by
# (graph, field_delta_scale, m, mode).  Measured on an MI355X at commit 77d9b5b, the last one before field_solve
# was split into phases; literal on purpose: nothing here is derived from the code under test.
WAITS = {
    ('chain100', '4', 1, 'settle_all'): ((10, 200), (9, 200)),
    ('chain100', '4', 1, 'unbounded'): ((10, 200), (9, 200)),
    ('chain100', '4', 4, 'settle_all'): ((12, 280), (11, 280)),
    ('chain100', '4', 4, 'unbounded'): ((12, 280), (11, 280)),
    ('chain100', 'inf', 1, 'settle_all'): ((10, 200), (9, 200)),
    ('chain100', 'inf', 1, 'unbounded'): ((10, 200), (9, 200)),
    ('chain100', 'inf', 4, 'settle_all'): ((10, 200), (9, 200)),
    ('chain100', 'inf', 4, 'unbounded'): ((10, 200), (9, 200)),
    ('one_node', '4', 1, 'settle_all'): ((4, 2), (3, 2)),
    ('one_node', '4', 1, 'unbounded'): ((4, 2), (3, 2)),
    ('one_node', '4', 4, 'settle_all'): ((4, 2), (3, 2)),
    ('one_node', '4', 4, 'unbounded'): ((4, 2), (3, 2)),
    ('one_node', 'inf', 1, 'settle_all'): ((4, 2), (3, 2)),
    ('one_node', 'inf', 1, 'unbounded'): ((4, 2), (3, 2)),
    ('one_node', 'inf', 4, 'settle_all'): ((4, 2), (3, 2)),
    ('one_node', 'inf', 4, 'unbounded'): ((4, 2), (3, 2)),
}


def test_host_waits_pinned(tmp_path):
    """How often a solve waits for the device, and how many rounds it runs, are pinned: the edge-cost wait (first
    solve on a graph only), one wait per batch of 32 rounds in each of the two passes, one for the outputs.  The
    one-node graph and a directed chain of 100 nodes (one node per round, so more than one batch per pass; see
    tests/test_gpu_cost_field_batch.py for why its round count is a function of the graph), at two bucket widths,
    for m = 1 and m = 4, unbounded and with settle "all" on the last node."""
    import trg_planner
    graphs = {"one_node": fg.oddities()["one_node"][0], "chain100": fg.chain(100)}
    e = trg_planner.Engine(**MOUNTAIN)
    got = {}
    for name, g in graphs.items():
        V = len(g.state)
        for scale in ("inf", "4"):
            e.set_option("field_delta_scale", scale)
            for m in (1, 4):
                for mode in ("unbounded", "settle_all"):
                    load_graph(e, g, tmp_path, name)  # a new graph_version: the next solve is the first on it
                    kw = dict(targets=[V - 1], settle="all") if mode == "settle_all" else {}
                    pair = []
                    for _ in range(2):
                        info = e.cost_fields(source_ids=[min(k, V - 1) for k in range(m)], **kw)["info"]
                        pair.append((info.host_syncs, info.rounds))
                    got[name, scale, m, mode] = tuple(pair)
    e.close()
    for key in sorted(got):
        print(f"    {key!r}: {got[key]!r},")
    assert got == WAITS
