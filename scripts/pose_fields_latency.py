#!/usr/bin/env python3
"""Run on the GPU box: what starting a cost field from a POSE costs (Engine.pose_links, cost_fields_seeded,
plan_anchored; DESIGN.md section 2, "Pose links" and "Start costs"), on the C3 graph set up as in
scripts/cost_field_sets_latency.py.  One process; after a warm-up of every shape the variants alternate, and the
medians are compared:

  (a) pose_links wall time for 1 pose and for 64 poses (free positions near the start and over the map)
  (b) a seeded solve from one pose's links, read at a ring of targets, beside cost_fields_from on the same members
      with zero start costs: the set solve is the yardstick, a seeded solve does the same rounds from the same nodes
  (c) plan_anchored from the start pose to a goal pose beside plan_many from the start to the same goal: the device
      time of the one solve each runs (plan_anchored's stops once the goal's link nodes are settled; plan_many runs
      with early_exit, which stops at the goal node)

Device time is the hipEvent time of the solve (TrgFieldInfo.ms_device), wall time the host clock around the call.

usage: python scripts/pose_fields_latency.py [--out PATH] [--reps N] [nx ny]
       -> PATH (default profiles/r21_pose_fields.json)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "trg-planner_amd"))
import trg_planner  # noqa: E402
from trg_planner import synth  # noqa: E402

argv = sys.argv[1:]
out = os.path.join(ROOT, "profiles", "r21_pose_fields.json")
reps = 15
if "--out" in argv:
    i = argv.index("--out")
    out = os.path.abspath(argv[i + 1])
    del argv[i:i + 2]
if "--reps" in argv:
    i = argv.index("--reps")
    reps = int(argv[i + 1])
    del argv[i:i + 2]
args = [a for a in argv if not a.startswith("--")]
nx, ny = (int(args[0]), int(args[1])) if len(args) >= 2 else (3200, 3125)
S = 16
prm = dict(expand_dist=0.6, robot_size=0.3, sample_num=S, height_threshold=0.16, collision_threshold=0.1,
           update_collision_threshold=0.1, safety_factor=3.0, goal_tolerance=0.8)
cloud = synth.mountain_tile(0, nx, 0, ny, seed=20250418)
cx, cy = nx * 0.05, ny * 0.05
scale = 6.0 * min(nx, ny) / 3125.0
start = (np.array([-7.22, -7.54], np.float32) * scale + np.array([cx, cy], np.float32)).astype(np.float32)

e = trg_planner.Engine(**prm)
e.set_sampler(7, 16)
e.set_global_map(cloud)
e.init_graph([cx, cy, 0.0])
V, E = e.graph_sizes("global")
n_points = int(cloud.shape[0])
del cloud

# poses with links: positions a third of an edge away from reached nodes spread over the map; the start pose first
cost0, hops0, _, info0 = e.cost_field(source_xy=start)
reachable = np.flatnonzero(hops0 >= 0)
xy = e.node_xyz("global")[:, :2]
spread = reachable[np.linspace(0, reachable.size - 1, 256).astype(np.int64)]
cand = np.concatenate([start[None], xy[spread] + np.float32(0.2)]).astype(np.float32)
linked = [k for k, one in enumerate(e.pose_links(cand)) if one["n_links"] >= 2]
poses = cand[linked[:64]]
assert poses.shape[0] == 64 and linked[0] == 0, (poses.shape, linked[:3])
d = np.hypot(xy[:, 0] - start[0], xy[:, 1] - start[1])
ring = np.flatnonzero((d >= 15.0) & (d <= 20.0) & (hops0 >= 0)).astype(np.int32)
goal = cand[[k for k in linked if 15.0 <= np.hypot(*(cand[k] - start)) <= 40.0][0]]
links0 = e.pose_links(poses[:1])[0]
demoted = int(np.count_nonzero(e.cost_fields_seeded([links0["nodes"]], [links0["cost"]], targets=links0["nodes"],
                                                    full=False)["hops_at"][0] > 0))
del cost0, hops0, xy, d


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def rec(info, wall, **more):
    return dict({"ms_device": info.ms_device, "ms_wall": wall, "rounds": info.rounds, "host_syncs": info.host_syncs},
                **more)


def links(n):
    r, wall = timed(lambda: e.pose_links(poses[:n]))
    return {"ms_wall": wall, "links": int(sum(one["n_links"] for one in r)),
            "candidates": int(sum(one["n_candidates"] for one in r))}


def seeded():
    r, wall = timed(lambda: e.cost_fields_seeded([links0["nodes"]], [links0["cost"]], targets=ring, full=False))
    return rec(r["info"], wall)


def zero_starts():
    r, wall = timed(lambda: e.cost_fields_from([links0["nodes"]], targets=ring, full=False))
    return rec(r["info"], wall)


def anchored():
    r, wall = timed(lambda: e.plan_anchored(poses[0], goal))
    assert r["found"]
    return rec(r["info"], wall, num_nodes=int(r["num_nodes"]))


def many():
    """plan_many's one solve and its routes call, timed together; the device time is the solve's."""
    goal_node = e._resolve_nodes(goal[None])

    def run():
        r = e.cost_fields(sources_xy=poses[:1], targets=goal_node, full=False, settle="all")
        return r, e.routes([0], goal_node)
    (r, routes), wall = timed(run)
    return rec(r["info"], wall, num_nodes=int(routes[0][2].num_nodes))


variants = {"a_pose_links_1": lambda: links(1), "a_pose_links_64": lambda: links(64), "b_seeded": seeded,
            "b_set_zero_starts": zero_starts, "c_plan_anchored": anchored, "c_plan_many_early_exit": many}
for fn in variants.values():  # warm-up: every shape twice
    fn()
    fn()
samples = {name: [] for name in variants}
for rep in range(reps):  # the variants alternate
    for name, fn in variants.items():
        samples[name].append(fn())
    print("rep", rep, flush=True)


def summary(recs):
    s = {}
    for key in recs[0]:
        vals = np.array([r[key] for r in recs], np.float64)
        if key.startswith("ms_"):
            s[key + "_median"] = float(np.median(vals))
            s[key + "_min"] = float(vals.min())
            s[key + "_max"] = float(vals.max())
        else:
            s[key] = int(vals[-1])
    return s


res = {"workload": f"C3-style {nx}x{ny} = {n_points} points, S={S}", "V": V, "E": E, "reps": reps,
       "field_delta_scale": 4, "ring_targets": int(ring.size), "links_of_the_start_pose": int(links0["n_links"]),
       "demoted_links_of_the_start_pose": demoted,
       "goal_distance_m": float(np.hypot(*(goal - start))),
       "variants": {name: summary(r) for name, r in samples.items()}}
v = res["variants"]
res["ratios"] = {
    "seeded_over_zero_starts_device": v["b_seeded"]["ms_device_median"] / v["b_set_zero_starts"]["ms_device_median"],
    "plan_anchored_over_plan_many_device": v["c_plan_anchored"]["ms_device_median"] /
                                           v["c_plan_many_early_exit"]["ms_device_median"],
    "pose_links_wall_per_pose_at_64": v["a_pose_links_64"]["ms_wall_median"] / 64.0,
}
res["note"] = ("ms_device = hipEvent time of the solve; ms_wall = host clock around the call (pose_links: its three "
               "batches -- collision, elevation, edges -- and the host gather and sort; plan_anchored: pose_links, the "
               "solve and the routes call).  The seeded solve and the set solve start from the same link nodes and are "
               "read at the same ring; demoted_links_of_the_start_pose counts the link nodes that a cheaper walk "
               "reaches from another link (seeds expanded once more than in the set solve).  Read the minima beside "
               "the medians: a field's time on this graph sits at one of two levels about 10 % apart -- here both occur "
               "within one process -- in every build (profiles/r17_risk_field.json), so a median of 15 can land on either.")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
