"""Test data: update sequences and engine histories that graph_support.drive() takes an engine and the oracle
through, step by step -- clouds, parameters, sampler and steps.  Test code only; nothing here needs a GPU.

A step is one of
    ("map", cloud_name)                      set_global_map
    ("init", start3d)                        init_graph
    ("init_declined", start3d, level)        init_graph whose device build declines at `level` (the engine's
                                             debug_fallback_level, reset afterwards); a plain init_graph on the oracle
    ("replay", "device" | "host")            the engine's replay option from here on
    ("local", pose, builder)                 set_local_map(pose, builder(cloud, pose, graph, memo))
    ("update",)                              update_graph
    ("plan", start2d, goal3d)                plan
`pose` is an (x, y) or a function (graph, memo) -> (x, y); `graph` is the ORACLE's global graph at that step, so
that the engine and the oracle receive the identical array whatever the engine holds; `memo` is a dict that lives
as long as one drive, for a step that must repeat what an earlier step computed.
"""
from collections import namedtuple

import numpy as np

from graph_support import obs_crop
from step3_cases import r160

Scenario = namedtuple("Scenario", "name base overrides seed replays steps")
# base: the oracle_api parameter set by name; overrides: changes to it; seed: sampler seed (table_bits 16);
# replays: the values of the engine's replay option the scenario is run under ((None,): it sets its own)

UPDATE_OVERRIDES = dict(update_collision_threshold=0.2)
START_B = [10.0, 10.0, 0.0]
START_GENTLE = [15.0, 15.0, 0.0]


def scenario_clouds(synth, mountain_gentle, indoor_small):
    """The clouds the steps name: B, 20 m x 20 m (V=2288 from START_B under MOUNTAIN, seed 5); the two fixtures;
    rough, the 16 m x 16 m of step3_cases.py on which step 3 rescues nodes."""
    return {"B": synth.mountain_cloud(200, 200, seed=1), "gentle": mountain_gentle, "indoor": indoor_small,
            "rough": r160(synth)}


def params(oa, sc):
    return dict(getattr(oa, sc.base), **sc.overrides)


# ---- poses --------------------------------------------------------------------------------------------------------
def node_fraction(num, den, key=None, frozen=False):
    """The exact xy of node V * num // den of the graph as it is (frozen: as it was at the drive's first such
    step, that is, after the build); remembered under `key`."""
    def pose(graph, memo):
        xyz = memo.setdefault("frozen_xyz", graph.xyz.copy()) if frozen else graph.xyz
        p = xyz[xyz.shape[0] * num // den, :2]
        p = (float(p[0]), float(p[1]))
        if key is not None:
            memo[key] = p
        return p
    return pose


def remembered(key):
    return lambda graph, memo: memo[key]


# ---- local-cloud builders: (cloud, pose, graph, memo) -> (n, 3) float32 -------------------------------------------
def crop(half, box_offset=None):
    """obs_crop around the pose; box_offset (dx, dy, half): the raised block, relative to the pose."""
    def build(cloud, pose, graph, memo):
        box = None if box_offset is None else (pose[0] + box_offset[0], pose[1] + box_offset[1], box_offset[2])
        return obs_crop(cloud, pose, half, box=box)
    return build


def whole_map(cloud, pose, graph, memo):
    return cloud.copy()


def single_point(near):
    """The one cloud point nearest `near`."""
    def build(cloud, pose, graph, memo):
        d = (cloud[:, 0].astype(np.float64) - near[0]) ** 2 + (cloud[:, 1].astype(np.float64) - near[1]) ** 2
        k = int(np.argmin(d))
        return cloud[k:k + 1].copy()
    return build


def nearest_node_xy(graph, near):
    d = (graph.xyz[:, 0].astype(np.float64) - near[0]) ** 2 + (graph.xyz[:, 1].astype(np.float64) - near[1]) ** 2
    return graph.xyz[int(np.argmin(d)), :2].astype(np.float64)


def annulus(half, near, r_in, r_out, key):
    """The crop around the pose with every point p, r_in < |p - c| < r_out, raised by 1.0 on alternate points
    (obs_crop's pattern); c is the node nearest `near` when the map is first built.  Built once per drive: every
    later step under the same `key` sends the same array."""
    def build(cloud, pose, graph, memo):
        if key not in memo:
            c = nearest_node_xy(graph, near)
            obs = obs_crop(cloud, pose, half)
            d = np.hypot(obs[:, 0].astype(np.float64) - c[0], obs[:, 1].astype(np.float64) - c[1])
            ring = (d > r_in) & (d < r_out)
            obs[ring, 2] += np.float32(1.0) * (np.arange(ring.sum()) % 2).astype(np.float32)
            memo[key] = obs
            memo[key + "_centre"] = c
        return memo[key]
    return build


def stripes(half, period, width):
    """The crop around the pose with the points of `x % period < width or y % period < width` raised by 1.0."""
    def build(cloud, pose, graph, memo):
        obs = obs_crop(cloud, pose, half)
        x, y = obs[:, 0].astype(np.float64), obs[:, 1].astype(np.float64)
        m = (np.mod(x, period) < width) | (np.mod(y, period) < width)
        obs[m, 2] += np.float32(1.0)
        return obs
    return build


def beyond_bounds(centre, half, shift_x):
    """The crop around `centre` stacked with a copy of itself shifted by shift_x: half of it lies outside the
    global map."""
    def build(cloud, pose, graph, memo):
        obs = obs_crop(cloud, centre, half)
        far = obs.copy()
        far[:, 0] += np.float32(shift_x)
        return np.concatenate([obs, far], axis=0)
    return build


# ---- scenarios ----------------------------------------------------------------------------------------------------
BOTH = ("device", "host")


def _mountain(name, steps, replays=BOTH, **more):
    return Scenario(name, "MOUNTAIN", dict(UPDATE_OVERRIDES, **more), 5, replays, steps)


def _on_b(*steps):
    return [("map", "B"), ("init", START_B)] + list(steps)


_UPDATE_A = [("local", (12.0, 12.0), crop(4.0, (2.0, 1.0, 0.6))), ("update",)]
_UPDATES_B = [("local", (10.0, 10.0), crop(4.0, (2.0, 1.0, 0.6))), ("update",),
              ("local", (11.0, 10.5), crop(4.0, (2.0, 1.0, 0.6))), ("update",)]
_PLAN_B = ("plan", (8.0, 8.0), (15.0, 14.0, 0.0))
_ISOLATED = annulus(6.0, (13.0, 10.0), 0.3, 1.9, "ring")
_STRIPES = stripes(6.0, 1.2, 0.5)

SCENARIOS = [
    # step 3 of expandGraph (expand_dist - robot_size < expand_dist / 4) inside updates: the obstacle moves with
    # the pose, the fourth update sees the first place again without it
    Scenario("indoor_step3_updates", "INDOOR", {}, 5, BOTH, [
        ("map", "indoor"), ("init", [2.0, 2.0, 0.0]),
        ("local", node_fraction(1, 3, "first", frozen=True), crop(3.0, (1.0, 0.5, 0.5))), ("update",),
        ("local", node_fraction(1, 2, frozen=True), crop(3.0, (1.0, 0.5, 0.5))), ("update",),
        ("local", node_fraction(2, 3, frozen=True), crop(3.0, (1.0, 0.5, 0.5))), ("update",),
        ("local", remembered("first"), crop(3.0)), ("update",)]),
    # the same on rough ground (step3_cases.py), where step 3 decides something: parent edges fail, nodes are rescued
    # by a neighbour, weights are non-zero -- in the build and in the expansions of every update
    Scenario("terrain_step3_updates", "INDOOR", dict(UPDATE_OVERRIDES), 5, BOTH, [
        ("map", "rough"), ("init", [8.0, 8.0, 0.0]),
        ("local", node_fraction(1, 3, "first", frozen=True), crop(3.0, (1.0, 0.5, 0.5))), ("update",),
        ("local", node_fraction(1, 2, frozen=True), crop(3.0, (1.0, 0.5, 0.5))), ("update",),
        ("local", remembered("first"), crop(3.0)), ("update",)]),
    # one engine through a build, an update and a build on another map: ids follow the container's history
    _mountain("history_rebuild",
              [("map", "gentle"), ("init", START_GENTLE)] + _UPDATE_A +
              [("map", "B"), ("init", START_B)] + _UPDATES_B + [_PLAN_B]),
    # the second build declines on the device at level 6 and is redone by the host replay, which has to rebuild the
    # real container from the replica that the first build and its update left.  (A decline at a level comes before
    # the device build touches the replica, so restoring the replica afterwards changes nothing here: only a decline
    # after the level loop, which no option provokes, would show a missing restore.)
    _mountain("history_declined_build",
              [("map", "gentle"), ("init", START_GENTLE)] + _UPDATE_A +
              [("map", "B"), ("init_declined", START_B, 6)] + _UPDATES_B[:2] + [_PLAN_B], replays=("device",)),
    # the two representations of the node container hand over to each other
    _mountain("history_host_then_device",
              [("replay", "host"), ("map", "gentle"), ("init", START_GENTLE)] + _UPDATE_A +
              [("replay", "device"), ("map", "B"), ("init", START_B)] + _UPDATES_B[:2] +
              [("replay", "host"), ("map", "gentle"), ("init", START_GENTLE)] + _UPDATE_A, replays=(None,)),
    # a local map of one point: nothing is invalidated, cleanGraph still renumbers
    _mountain("renumber_only", _on_b(
        ("local", (10.0, 10.0), single_point((10.03, 10.04))), ("update",), *_UPDATES_B[:2])),
    # a node that loses every edge in one cleanGraph and is dropped by the next
    _mountain("isolated_node", _on_b(
        ("local", (10.0, 10.0), _ISOLATED), ("update",), ("local", (10.0, 10.0), _ISOLATED), ("update",),
        ("local", (10.0, 10.0), _ISOLATED), ("update",))),
    # hundreds of nodes invalidated, removed and grown back
    _mountain("stripes", _on_b(
        ("local", (10.0, 10.0), _STRIPES), ("update",), ("local", (10.0, 10.0), _STRIPES), ("update",),
        ("local", (10.0, 10.0), _STRIPES), ("update",))),
    # the pose lies exactly on a node: isFrontier's direction is (0, 0) there
    _mountain("pose_on_node", _on_b(("local", node_fraction(1, 2, "pose"), crop(3.0)), ("update",))),
    # a small local graph in the bucket array a large one left behind
    _mountain("big_then_small_local", _on_b(
        ("local", (10.0, 10.0), whole_map), ("update",), ("local", (10.0, 10.0), crop(2.0)), ("update",),
        ("local", (10.0, 10.0), whole_map), ("update",))),
    _mountain("beyond_bounds", _on_b(("local", (1.5, 1.5), beyond_bounds((1.0, 1.0), 3.0, -3.0)), ("update",))),
    # more than CHUNK_MAX = 4096 roots and more than EBATCH_MAX = 65536 deferred edges in one update: the second root
    # chunk, and one batch shipped in the middle of the expansions.  Reached: a build of 5975 nodes, 5807 of them
    # local nodes and every one a root, 100384 wireEdge calls in the update (the oracle's count and the engine's).
    # The rotation of the three batch buffers would take a fourth batch in flight, 262144 calls: not reached.
    _mountain("many_roots", [("map", "gentle"), ("init", START_GENTLE), ("local", (15.0, 15.0), whole_map),
                             ("update",)], replays=("device",), sample_num=16),
]
BY_NAME = {sc.name: sc for sc in SCENARIOS}


# ---- what each scenario must keep reaching, on the oracle's graphs ------------------------------------------------
# `hist` is drive()'s list of one record per init / update step, of the oracle's graph after it
def _updates(hist):
    return [h for h in hist if h["kind"] == "update"]


def check_indoor_step3_updates(hist):
    v = [h["V"] for h in hist][:4]  # the build and the three updates that see the obstacle
    assert all(b < a for a, b in zip(v, v[1:])), v
    assert any(h["frontier"] > 0 for h in _updates(hist)), [h["frontier"] for h in hist]


def check_terrain_step3_updates(hist):
    ups = _updates(hist)
    assert len(ups) == 3 and all(h["wire_calls"] > 1000 for h in ups), [h["wire_calls"] for h in hist]
    assert all(h["frontier"] > 0 for h in ups), [h["frontier"] for h in hist]
    assert hist[-1]["nonzero_w"] > 1000, hist[-1]["nonzero_w"]


def check_renumber_only(hist):
    build, first = hist[0], hist[1]
    assert (first["V"], first["E"]) == (build["V"], build["E"]), (build["V"], build["E"], first["V"], first["E"])
    assert not np.array_equal(first["xyz"], build["xyz"])


def check_isolated_node(hist):
    ups = _updates(hist)
    assert [h["deg0"].size for h in hist[:3]] == [0, 1, 0], [h["deg0"] for h in hist]
    # ... and it did not get its edges back: the second cleanGraph dropped it
    lone = ups[0]["xyz"][ups[0]["deg0"][0]]
    assert not (ups[1]["xyz"].view(np.uint32) == lone.view(np.uint32)).all(axis=1).any()


def check_stripes(hist):
    assert hist[0]["V"] - hist[1]["V"] > 200, [h["V"] for h in hist]


def check_many_roots(hist):
    assert hist[0]["V"] > 4096 and hist[1]["wire_calls"] > 65536, (hist[0]["V"], hist[1]["wire_calls"])
    # every node is a root: none was invalidated, so cleanGraph dropped none of the build's nodes
    before, after = (set(map(bytes, np.ascontiguousarray(h["xyz"]))) for h in hist)
    assert before <= after


PRECONDITIONS = {"many_roots": check_many_roots, "indoor_step3_updates": check_indoor_step3_updates,
                 "terrain_step3_updates": check_terrain_step3_updates,
                 "renumber_only": check_renumber_only,
                 "isolated_node": check_isolated_node, "stripes": check_stripes}
