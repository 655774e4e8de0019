"""GPU: Engine.plan_anchored on mountain_small ("Pose links" and "Start costs"): 16 start / goal
pairs whose links come from Engine.pose_links (compared with the plain loop in tests/test_gpu_pose_links.py).

The expected cost and node sequence come from tests/seed_ref.py on the graph with rho and a sink: an arc
rho -> a_i of weight 0 and dist c_i for every start link (node a_i, link cost c_i) and an arc b_j -> sink of weight 0
and dist d_j for every goal link (node b_j, link cost d_j); the path's cost is the sink's cost in the field from rho,
compared as bits.  The goal link is the earliest j whose key (fl(cost[b_j] + d_j), hops[b_j] + 1) is the sink's (the
sink's own parent would be the smallest node id among those); the node sequence walks the parents from b_j back to
the root, whose owner is the start link.  One pair starts in collision and is not found; on the reference, at least
one pair enters the graph at another node than the one `plan` snaps its start to."""
import numpy as np
import pytest

import pose_cases as pc
import seed_ref

pytestmark = pytest.mark.gpu
F32 = np.float32
SEED, N_PAIRS = 5, 16


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def built(oa, mountain_small):
    import trg_planner
    prm = dict(oa.MOUNTAIN)
    e = trg_planner.Engine(**prm)
    e.set_sampler(7, 16)
    e.set_global_map(mountain_small)
    e.init_graph([15.0, 15.0, 0.0])
    yield prm, e, e.graph("global")
    e.close()


def pairs_of(links, xy, n):
    """n (start, goal) index pairs into xy: poses with links, each start 3..8 m from its goal; the LAST pair's start is
    a pose in collision."""
    good = [k for k, one in enumerate(links) if one["n_links"] > 0]
    blocked = [k for k, one in enumerate(links) if one["status"] == 1]
    out, used = [], set()
    for a in good:
        for b in good:
            d = float(np.hypot(*(xy[a] - xy[b])))
            if a not in used and b not in used and a != b and 3.0 <= d <= 8.0:
                out.append((a, b))
                used |= {a, b}
                break
        if len(out) == n - 1:
            break
    assert len(out) == n - 1 and blocked
    return out + [(blocked[0], good[0])]


def expected(g, sf, start, goal):
    """-> (cost, node ids, start link index, goal link index) from the field of rho on the graph with a sink, or None."""
    if start["nodes"].size == 0 or goal["nodes"].size == 0:
        return None
    V = g.V
    a = seed_ref.augmented(g, start["nodes"], start["cost"], sinks=(goal["nodes"], goal["cost"]))
    cost, hops, parent = seed_ref.rho_field(a, sf, V)
    if hops[V + 1] < 0:
        return None
    with np.errstate(over="ignore"):
        through = (cost[goal["nodes"]] + goal["cost"]).astype(F32)
    j = next(j for j, b in enumerate(goal["nodes"]) if hops[b] >= 0 and _bits(through[j]) == _bits(cost[V + 1])
             and hops[b] + 1 == hops[V + 1])
    ids = [int(goal["nodes"][j])]
    while parent[ids[-1]] != V:
        ids.append(int(parent[ids[-1]]))
    ids.reverse()
    least = min(_bits(c)[0] for s, c in zip(start["nodes"], start["cost"]) if s == ids[0])
    assert _bits(cost[ids[0]])[0] == least  # the entry node is a root
    i = next(i for i, (s, c) in enumerate(zip(start["nodes"], start["cost"])) if s == ids[0] and _bits(c)[0] == least)
    return cost[V + 1], ids, i, j


def test_plans_equal_the_field_with_a_sink(built, mountain_small):
    prm, e, g = built
    rng = np.random.default_rng(SEED)
    xy = np.concatenate([rng.uniform(3.0, 27.0, size=(96, 2)).astype(F32),
                         pc.poses(mountain_small, g, 1, prm["robot_size"])[48:]])  # (the last: near steep ground)
    links = e.pose_links(xy)
    pairs = pairs_of(links, xy, N_PAIRS)
    xyz = g.xyz
    want = [expected(g, prm["safety_factor"], links[a], links[b]) for a, b in pairs]
    assert want[-1] is None and sum(w is not None for w in want) >= N_PAIRS - 2
    # on the reference: some pair enters the graph at another node than the nearest one, which `plan` starts from
    snapped = [int(np.argmin((xy[a, 0] - xyz[:, 0]) ** 2 + (xy[a, 1] - xyz[:, 1]) ** 2)) for a, _ in pairs]
    differ = [k for k, w in enumerate(want) if w is not None and w[1][0] != snapped[k]]
    assert differ, "every pair enters at its nearest node"
    for k, ((a, b), w) in enumerate(zip(pairs, want)):
        at = f"pair {k} {xy[a].tolist()} -> {xy[b].tolist()}: "
        r = e.plan_anchored(xy[a], xy[b])
        if w is None:
            assert not r["found"] and r["node_ids"].size == 0 and r["start_link"] is None, at
            continue
        cost, ids, i, j = w
        assert r["found"], at
        assert _bits(r["cost"]) == _bits(cost), at + f"cost {r['cost']!r} != {cost!r}"
        assert r["node_ids"].tolist() == ids, at + f"ids {r['node_ids'].tolist()} != {ids}"
        sl, gl = links[a], links[b]
        assert r["start_link"] == (int(sl["nodes"][i]), float(sl["weight"][i]), float(sl["dist"][i])), at + "start link"
        assert r["goal_link"] == (int(gl["nodes"][j]), float(gl["weight"][j]), float(gl["dist"][j])), at + "goal link"
        assert r["num_nodes"] == len(ids) and r["path"].shape == (len(ids) + 2, 3), at
        assert np.array_equal(_bits(r["path"][1:-1]), _bits(xyz[ids])), at + "path"
        assert np.array_equal(_bits(r["path"][0]), _bits([xy[a, 0], xy[a, 1], sl["z"]])), at + "start pose"
        assert np.array_equal(_bits(r["path"][-1]), _bits([xy[b, 0], xy[b, 1], gl["z"]])), at + "goal pose"
    # ... and that nearest node is indeed where the snapping queries start
    assert e._resolve_nodes(xy[[a for a, _ in pairs]]).tolist() == snapped
