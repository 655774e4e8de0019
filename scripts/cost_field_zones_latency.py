#!/usr/bin/env python3
"""Run on the GPU box: what keep-out zones cost (Engine.cost_fields_avoiding / plan_avoiding,
trg_engine_cost_field_zones; DESIGN.md section 2, "Keep-out zones"), on the C3 graph set up as in
scripts/cost_field_models_latency.py.  One process; after a warm-up of every shape the variants alternate, and the
medians are compared:

  cold slots   a solve whose edge-cost slot is not cached against the same solve on a cached slot, both under a budget
               of 0 (the source alone is reached, so the difference is the slot: one launch and its host wait):
               a plain model (k_field_edge_cost) and zone sets of Z = 1, 16, 256 (k_field_edge_zones).  Every cold
               call names a model / a zone list no call before it named (one more ulp on the safety factor / on the
               first radius), so the cache cannot answer it.
  warm fields  one full field from the first start of scripts/plan_latency.py read at its goal, without zones and
               with 16 zones on the way; plan_avoiding for four zone sets (A, B, both, none) against the same call with
               four empty zone sets.
  plain        cost_fields of 8 fields from one start, without models and under 8 safety factors, and one full single
               field: the launches and slots that zones leave unchanged, for the comparison with the parent commit.

With --tree PATH the package is imported from PATH/trg-planner_amd (a checkout of another commit, built there); a tree
without the zone entries runs the plain part and the plain cold slot only.  Device time is the hipEvent time of the
solve (TrgFieldInfo.ms_device), wall time the host clock around a call that ends in a device synchronise.

usage: python scripts/cost_field_zones_latency.py [--out PATH] [--reps N] [--tree PATH] [nx ny]
       -> PATH (default profiles/r33_cost_field_zones.json): one run.  The committed profile holds six -- three of the
       parent commit and three of the change, alternating in one visit -- under "parent" and "change", with the
       workload's figures once at the top.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
out = os.path.join(ROOT, "profiles", "r33_cost_field_zones.json")
reps = 15
tree = ROOT
for flag in ("--out", "--reps", "--tree"):
    if flag in argv:
        i = argv.index(flag)
        value = argv[i + 1]
        del argv[i:i + 2]
        if flag == "--out":
            out = os.path.abspath(value)
        elif flag == "--reps":
            reps = int(value)
        else:
            tree = os.path.abspath(value)
sys.path.insert(0, os.path.join(tree, "trg-planner_amd"))
import trg_planner  # noqa: E402
from trg_planner import synth  # noqa: E402

args = [a for a in argv if not a.startswith("--")]
nx, ny = (int(args[0]), int(args[1])) if len(args) >= 2 else (3200, 3125)
S = 16
SF = 3.0
prm = dict(expand_dist=0.6, robot_size=0.3, sample_num=S, height_threshold=0.16, collision_threshold=0.1,
           update_collision_threshold=0.1, safety_factor=SF, goal_tolerance=0.8)
cloud = synth.mountain_tile(0, nx, 0, ny, seed=20250418)
cx, cy = nx * 0.05, ny * 0.05
ref_s = np.array([[-7.22, -7.54]], np.float32)
ref_g = np.array([[-9.97, 3.56]], np.float32)
scale = 6.0 * min(nx, ny) / 3125.0
start_xy = (ref_s * scale + np.array([cx, cy], np.float32)).astype(np.float32)[0]
goal_xy = (ref_g * scale + np.array([cx, cy], np.float32)).astype(np.float32)[0]

e = trg_planner.Engine(**prm)
e.set_sampler(7, 16)
e.set_global_map(cloud)
e.init_graph([cx, cy, 0.0])
V, E = e.graph_sizes("global")
n_points = int(cloud.shape[0])
del cloud
start, goal = (int(v) for v in e._resolve_nodes([start_xy, goal_xy]))
has_zones = hasattr(e, "cost_fields_avoiding")
pos = e.node_xyz()
lo, hi = pos[:, :2].min(axis=0), pos[:, :2].max(axis=0)
rng = np.random.default_rng(33)


def spread(n):
    """n zones spread over the graph's extent, radii 0.5 .. 2 m."""
    return np.concatenate([rng.uniform(lo, hi, size=(n, 2)), rng.uniform(0.5, 2.0, size=(n, 1))], axis=1).astype(np.float32)


mid = 0.5 * (start_xy + goal_xy)
step = (goal_xy - start_xy) / np.float32(np.hypot(*(goal_xy - start_xy)))
normal = np.array([-step[1], step[0]], np.float32)
# 16 discs of 1.5 m in a row across the straight line from start to goal, 2.5 m apart: a wall 40 m wide to go round
wall16 = np.array([[*(mid + normal * np.float32(2.5 * (k - 7.5))), 1.5] for k in range(16)], np.float32)
zone_A = wall16[:8]
zone_B = wall16[8:]
M = 8
factors = [float(k) * 8.0 / 7.0 for k in range(M)]
ulp = {"sf": np.float32(SF + 1.0), "r": {}}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def rec(r, wall):
    i = r["info"]
    return {"ms_device": i.ms_device, "ms_wall": wall, "rounds": i.rounds, "host_syncs": i.host_syncs,
            "reached": int(r["reached"].sum())}


def plain_slot(cold):
    """A budget-0 solve under a model of its own: a new one per cold call, (SF + 1, inf) otherwise."""
    if cold:
        ulp["sf"] = np.nextafter(ulp["sf"], np.float32(np.inf))
    sf = float(ulp["sf"]) if cold else SF + 1.0
    r, wall = timed(lambda: e.cost_fields_from_models([[start]], [(sf, np.inf)], targets=[goal], full=False, budget=0.0))
    return rec(r, wall)


zone_lists = {Z: spread(Z) for Z in (1, 16, 256)}


def zone_slot(Z, cold):
    """A budget-0 solve under a zone list of Z zones: with one more ulp on the first radius per cold call."""
    z = zone_lists[Z]
    if cold:
        z = z.copy()
        ulp["r"][Z] = np.nextafter(ulp["r"].get(Z, z[0, 2]), np.float32(np.inf))
        z[0, 2] = ulp["r"][Z]
    r, wall = timed(lambda: e.cost_fields_avoiding([start], z, targets=[goal], full=False, budget=0.0))
    return rec(r, wall)


def full_field(zones):
    if zones is None:
        r, wall = timed(lambda: e.cost_fields_from([[start]], targets=[goal], full=False))
    else:
        r, wall = timed(lambda: e.cost_fields_avoiding([start], zones, targets=[goal], full=False))
    out = rec(r, wall)
    out["goal_hops"] = int(r["hops_at"][0, 0])
    out["goal_cost"] = float(r["cost_at"][0, 0])
    return out


def avoiding(zone_sets):
    recs, wall = timed(lambda: e.plan_avoiding(start_xy, goal_xy, zone_sets))
    return {"ms_wall": wall, "found": sum(r["found"] for r in recs), "nodes": [int(r["ids"].size) for r in recs]}


def batch(models):
    r, wall = timed(lambda: e.cost_fields(source_ids=[start] * M, targets=[goal], full=False, models=models))
    return rec(r, wall)


def single():
    r, wall = timed(lambda: e.cost_fields(source_ids=[start], full=False))
    return rec(r, wall)


variants = {"plain_batch8": lambda: batch(None), "plain_batch8_models": lambda: batch(factors), "plain_single": single,
            "slot_plain_cold": lambda: plain_slot(True), "slot_plain_warm": lambda: plain_slot(False)}
if has_zones:
    for Z in (1, 16, 256):
        variants[f"slot_zones{Z}_cold"] = (lambda Z=Z: zone_slot(Z, True))
        variants[f"slot_zones{Z}_warm"] = (lambda Z=Z: zone_slot(Z, False))
    variants["field_plain"] = lambda: full_field(None)
    variants["field_wall16"] = lambda: full_field(wall16)
    variants["plan_avoiding_A_B_AB_none"] = lambda: avoiding([zone_A, zone_B, wall16, None])
    variants["plan_avoiding_4_empty"] = lambda: avoiding([None] * 4)

first = {name: fn() for name, fn in variants.items()}
for _ in range(70):  # fill the cache's 65 slots: from here on a cold slot takes one over, the array never grows again
    plain_slot(True)
for fn in variants.values():
    fn()
samples ={name: [] for name in variants}
for rep in range(reps):  # the variants alternate
    for name, fn in variants.items():
        samples[name].append(fn())
    print("rep", rep, flush=True)


def summary(recs):
    s = {}
    for key in recs[0]:
        if key.startswith("ms_"):
            vals = np.array([r[key] for r in recs], np.float64)
            s[key + "_median"] = float(np.median(vals))
            s[key + "_min"] = float(vals.min())
            s[key + "_max"] = float(vals.max())
        else:
            s[key] = recs[-1][key]
    return s


res = {"workload": f"C3-style {nx}x{ny} = {n_points} points, S={S}", "tree": os.path.relpath(tree, ROOT), "V": V, "E": E,
       "reps": reps, "field_delta_scale": 4, "start_node": start, "goal_node": goal, "zones": has_zones,
       "variants": {name: summary(r) for name, r in samples.items()}, "first_call": first}
v = res["variants"]


def cold_cost(name):
    return v[f"slot_{name}_cold"]["ms_device_median"] - v[f"slot_{name}_warm"]["ms_device_median"]


res["cold_slot_ms_device"] = {"plain": cold_cost("plain")}
if has_zones:
    closed = {f"zones{Z}": e.closed_edges(zone_lists[Z])["n_closed"] for Z in (1, 16, 256)}
    closed["wall16"] = e.closed_edges(wall16)["n_closed"]
    res["closed_edges"] = closed
    for Z in (1, 16, 256):
        res["cold_slot_ms_device"][f"zones{Z}"] = cold_cost(f"zones{Z}")
    res["ratios"] = {
        "field_wall16_over_plain_device": v["field_wall16"]["ms_device_median"] / v["field_plain"]["ms_device_median"],
        "plan_avoiding_over_4_empty_wall": v["plan_avoiding_A_B_AB_none"]["ms_wall_median"] /
        v["plan_avoiding_4_empty"]["ms_wall_median"]}
res["note"] = ("ms_device = hipEvent time of the solve; ms_wall = host clock around the call.  cold_slot_ms_device = "
               "median of the cold budget-0 solve minus median of the warm one: the slot's launch, its stats copy and "
               "the host wait for them.  slot_plain_* goes through the sets entry with one model.")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
