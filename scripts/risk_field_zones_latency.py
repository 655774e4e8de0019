#!/usr/bin/env python3
"""Run on the GPU box: what keep-out zones cost on risk fields (Engine.risk_fields_avoiding / safest_route_avoiding,
trg_engine_risk_field_zones; DESIGN.md section 2, "Keep-out zones on risk fields"), on the C3 graph set up as in
scripts/cost_field_zones_latency.py.  One process; after a warm-up of every shape the variants alternate, and the
medians are compared:

  cold slots   a risk solve whose slot of edge risks is not cached against the same solve on a cached slot, both under
               a ceiling of 0 from a node whose edges all carry a positive weight (the source alone is reached, so the
               difference is the slot: one launch and its host wait): the plain risk slot (k_field_edge_risk; made
               cold by eight solves under 64 new cost models, which take every slot of the cache but the engine's
               own) and zone lists of Z = 1, 16, 256 (k_field_edge_risk_zones; every cold call names a list no call
               before it named -- one more ulp on the first radius).  A warm sample is the second of two equal calls.
  warm fields  one full risk field from the first start of scripts/plan_latency.py read at its goal, without zones and
               with 16 zones on the way; four fields under four lists (the RISK MODELS kernels) against four fields
               under one list (the plain RISK kernels on one slot); safest_route_avoiding of four zone sets (A, B, both,
               none) against four safest_route calls.
  plain        risk_fields of 8 fields from one start and one full single field: the launches that zones leave
               unchanged, for the comparison with the parent commit.

With --tree PATH the package is imported from PATH/trg-planner_amd (a checkout of another commit, built there); a tree
without the zoned risk entry runs the plain part and the plain cold slot only, and so does --plain on a tree that has
it: the same calls in the same order as the parent's run, for the comparison of the two.  Device time is the hipEvent
time of the solve (TrgFieldInfo.ms_device), wall time the host clock around a call that ends in a device synchronise.

usage: python scripts/risk_field_zones_latency.py [--out PATH] [--reps N] [--tree PATH] [--plain] [nx ny]
       -> PATH (default profiles/r34_risk_field_zones.json): one run.  The committed profile holds nine -- three of the
       parent commit, three of the change with --plain and three of the change in full, alternating in one visit --
       under "parent", "change_plain" and "change", with the workload's figures once at the top.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
out = os.path.join(ROOT, "profiles", "r34_risk_field_zones.json")
reps = 15
tree = ROOT
plain_only = "--plain" in argv  # the plain part and the plain cold slot only, as a tree without the entry runs
argv = [a for a in argv if a != "--plain"]
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
has_zones = hasattr(e, "risk_fields_avoiding") and not plain_only
pos = e.node_xyz()
# The source of the cold-slot solves: a node all of whose edges carry a positive weight, so that a ceiling of 0 reaches
# it alone (nearly all weights of this graph are 0: from `start` such a solve floods most of the graph).
g = e.graph("global")
deg = np.diff(g.rowptr)
least = np.full(V, np.inf, np.float32)
rows = np.flatnonzero(deg > 0)
least[rows] = np.minimum.reduceat(g.w, g.rowptr[rows])
lone = np.flatnonzero((least > 0) & np.isfinite(least) & (g.state != -1))
lone = int(lone[lone.size // 2]) if lone.size else start
del g, deg, least, rows
lo, hi = pos[:, :2].min(axis=0), pos[:, :2].max(axis=0)
rng = np.random.default_rng(34)


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
ulp = {"sf": np.float32(SF + 1.0), "r": {}}
zone_lists = {Z: spread(Z) for Z in (1, 16, 256)}
four_lists = [zone_A, zone_B, wall16, zone_lists[16]]


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def rec(r, wall):
    i = r["info"]
    return {"ms_device": i.ms_device, "ms_wall": wall, "rounds": i.rounds, "host_syncs": i.host_syncs,
            "reached": int(r["reached"].sum())}


def evict():
    """Eight budget-0 cost solves under 64 models no call before them named: every slot of the cache but the engine's
    own is taken, least recently used first, the slot of the plain edge risks among them."""
    for _ in range(8):
        models = []
        for _ in range(8):
            ulp["sf"] = np.nextafter(ulp["sf"], np.float32(np.inf))
            models.append((float(ulp["sf"]), np.inf))
        e.cost_fields_from_models([[start]] * 8, models, targets=[goal], full=False, budget=0.0)


def plain_slot(cold):
    """A ceiling-0 risk solve on the plain slot: computed again after evict(), or cached (the second of two calls)."""
    call = lambda: e.risk_fields(source_ids=[lone], targets=[goal], full=False, budget=0.0)
    if cold:
        evict()
    else:
        call()
    r, wall = timed(call)
    return rec(r, wall)


def zone_slot(Z, cold):
    """A ceiling-0 risk solve under a list of Z zones: with one more ulp on the first radius per cold call."""
    z = zone_lists[Z]
    if cold:
        z = z.copy()
        ulp["r"][Z] = np.nextafter(ulp["r"].get(Z, z[0, 2]), np.float32(np.inf))
        z[0, 2] = ulp["r"][Z]
    call = lambda: e.risk_fields_avoiding([lone], z, targets=[goal], full=False, budget=0.0)
    if not cold:
        call()
    r, wall = timed(call)
    return rec(r, wall)


def warm(call):
    """The second of two equal calls: whatever the calls between evicted is cached again."""
    call()
    return timed(call)


def full_field(zones):
    if zones is None:
        r, wall = warm(lambda: e.risk_fields_from([[start]], targets=[goal], full=False))
    else:
        r, wall = warm(lambda: e.risk_fields_avoiding([start], zones, targets=[goal], full=False))
    out = rec(r, wall)
    out["goal_hops"] = int(r["hops_at"][0, 0])
    out["goal_risk"] = float(r["risk_at"][0, 0])
    return out


def four_fields(zone_sets):
    r, wall = warm(lambda: e.risk_fields_avoiding([start] * 4, zone_sets, targets=[goal], full=False))
    out = rec(r, wall)
    out["goal_hops"] = r["hops_at"][:, 0].tolist()
    return out


def avoiding(zone_sets):
    recs, wall = warm(lambda: e.safest_route_avoiding(start_xy, goal_xy, zone_sets))
    return {"ms_wall": wall, "found": sum(r is not None for r in recs),
            "max_risk": [None if r is None else r[0] for r in recs],
            "nodes": [0 if r is None else int(r[1]["ids"].size) for r in recs]}


def four_safest_routes():
    recs, wall = warm(lambda: [e.safest_route(start_xy, goal_xy) for _ in range(4)])
    return {"ms_wall": wall, "found": sum(r is not None for r in recs),
            "nodes": [0 if r is None else int(r[1]["ids"].size) for r in recs]}


def batch():
    r, wall = warm(lambda: e.risk_fields(source_ids=[start] * M, targets=[goal], full=False))
    return rec(r, wall)


def single():
    r, wall = warm(lambda: e.risk_fields(source_ids=[start], full=False))
    return rec(r, wall)


variants = {"plain_batch8": batch, "plain_single": single, "four_safest_routes": four_safest_routes,
            "slot_plain_cold": lambda: plain_slot(True), "slot_plain_warm": lambda: plain_slot(False)}
if has_zones:
    for Z in (1, 16, 256):
        variants[f"slot_zones{Z}_cold"] = (lambda Z=Z: zone_slot(Z, True))
        variants[f"slot_zones{Z}_warm"] = (lambda Z=Z: zone_slot(Z, False))
    variants["field_plain"] = lambda: full_field(None)
    variants["field_wall16"] = lambda: full_field(wall16)
    variants["four_fields_four_lists"] = lambda: four_fields(four_lists)
    variants["four_fields_one_list"] = lambda: four_fields(wall16)
    variants["safest_route_avoiding_A_B_AB_none"] = lambda: avoiding([zone_A, zone_B, wall16, None])

first = {name: fn() for name, fn in variants.items()}
evict()  # the cache's 65 slots are filled: from here on a cold slot takes one over, the array never grows again
for fn in variants.values():
    fn()
samples = {name: [] for name in variants}
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
       "reps": reps, "field_delta_scale": 4, "start_node": start, "goal_node": goal, "slot_node": lone, "zones": has_zones,
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
        "four_lists_over_one_list_device": v["four_fields_four_lists"]["ms_device_median"] /
        v["four_fields_one_list"]["ms_device_median"],
        "safest_route_avoiding_over_four_safest_routes_wall": v["safest_route_avoiding_A_B_AB_none"]["ms_wall_median"] /
        v["four_safest_routes"]["ms_wall_median"]}
res["note"] = ("ms_device = hipEvent time of the solve; ms_wall = host clock around the call.  cold_slot_ms_device = "
               "median of the cold ceiling-0 solve minus median of the warm one: the slot's launch, its stats copy and "
               "the host wait for them.  Every warm sample is the second of two equal calls.")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
