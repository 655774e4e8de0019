#!/usr/bin/env python3
"""Run on the GPU box: what a risk field (Engine.risk_fields, trg_engine_risk_field_sets; DESIGN.md section 2, "Risk
fields") costs, and what Engine.safest_route saves over Engine.min_risk_ceiling.  Two terrains, one after the other in
one process: the C3 graph set up as in scripts/cost_field_batch_latency.py, whose minimax answers are all 0, and a
rougher one (the terrain of the tests' mountain_small at a larger size), where some are not.  On each, after a warm-up
of every variant the variants alternate, and the medians are compared:

  (a) one risk field from each of the five scripts/plan_latency.py starts, beside one cost field from the same start
      (full fields, nothing of V entries copied back: device ms, rounds)
  (b) safest_route against min_risk_ceiling on the five start / goal pairs, by the wall clock, and their answers

Device time is the hipEvent time of the solve (TrgFieldInfo.ms_device), wall time the host clock around the call.
The first call of each variant, which computes the edge values it reads, is recorded apart as "cold".

usage: python scripts/risk_field_latency.py [--out PATH] [--reps N] [--rough N] [nx ny]
       -> PATH (default profiles/r17_risk_field.json); --rough: the rough terrain has N x N points (default 1200)
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
out = os.path.join(ROOT, "profiles", "r17_risk_field.json")
reps = 15
rough_n = 1200
if "--out" in argv:
    i = argv.index("--out")
    out = os.path.abspath(argv[i + 1])
    del argv[i:i + 2]
if "--reps" in argv:
    i = argv.index("--reps")
    reps = int(argv[i + 1])
    del argv[i:i + 2]
if "--rough" in argv:
    i = argv.index("--rough")
    rough_n = int(argv[i + 1])
    del argv[i:i + 2]
args = [a for a in argv if not a.startswith("--")]
nx, ny = (int(args[0]), int(args[1])) if len(args) >= 2 else (3200, 3125)
S = 16
SF = 3.0
prm = dict(expand_dist=0.6, robot_size=0.3, sample_num=S, height_threshold=0.16, collision_threshold=0.1,
           update_collision_threshold=0.1, safety_factor=SF, goal_tolerance=0.8)
ref_s = np.array([[-7.22, -7.54], [-2.07, -2.21], [13.04, -1.99], [17.96, 17.69], [-6.56, 4.59]], np.float32)
ref_g = np.array([[-9.97, 3.56], [7.52, 1.44], [14.43, 6.87], [9.49, 16.60], [3.11, -6.68]], np.float32)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def summary(recs):
    s = {}
    for key in recs[0]:
        vals = np.array([r[key] for r in recs], np.float64)
        if key.startswith("ms_"):
            s[key + "_median"] = float(np.median(vals))
            s[key + "_min"] = float(vals.min())
            s[key + "_max"] = float(vals.max())
        else:
            s[key] = float(vals[-1])
    return s


def measure(workload, cloud, centre, scale):
    cx, cy = centre
    starts = (ref_s * scale + np.array([cx, cy], np.float32)).astype(np.float32)
    goals = (ref_g * scale + np.array([cx, cy], np.float32)).astype(np.float32)
    e = trg_planner.Engine(**prm)
    e.set_sampler(7, 16)
    e.set_global_map(cloud)
    e.init_graph([cx, cy, 0.0])
    V, E = e.graph_sizes("global")
    g = e.graph("global")
    w_valid = g.w[g.state[g.col] != -1]
    weights = {"zero_share": float(np.mean(w_valid == 0)), "distinct": int(np.unique(w_valid).size),
               "max": float(w_valid.max())}
    del g, w_valid
    nodes = e._resolve_nodes(np.concatenate([starts, goals]))
    pairs = [(int(nodes[k]), int(nodes[5 + k])) for k in range(5)]

    def field(kind, k):
        solve = e.risk_fields if kind == "risk" else e.cost_fields
        r, wall = timed(lambda: solve(source_ids=[pairs[k][0]], targets=[pairs[k][1]], full=False))
        i = r["info"]
        at = r["risk_at" if kind == "risk" else "cost_at"][0, 0]
        return {"ms_device": i.ms_device, "ms_wall": wall, "rounds": i.rounds, "host_syncs": i.host_syncs,
                "reached": int(r["reached"][0]), "at_goal": float(at) if np.isfinite(at) else -1.0}

    def route(how, k):
        fn = e.safest_route if how == "safest_route" else e.min_risk_ceiling
        got, wall = timed(lambda: fn(starts[k], goals[k]))
        return {"ms_wall": wall, "max_risk": -1.0 if got is None else got[0],
                "nodes": 0 if got is None else int(got[1]["ids"].size),
                "cost": -1.0 if got is None else got[1]["cost"]}

    variants = {}
    for k in range(5):
        variants[f"a_risk_field_start{k}"] = (lambda k=k: field("risk", k))
        variants[f"a_cost_field_start{k}"] = (lambda k=k: field("cost", k))
    for k in range(5):
        variants[f"b_safest_route_pair{k}"] = (lambda k=k: route("safest_route", k))
        variants[f"b_min_risk_ceiling_pair{k}"] = (lambda k=k: route("min_risk_ceiling", k))
    cold = {name: fn() for name, fn in variants.items()}
    for fn in variants.values():
        fn()
    samples = {name: [] for name in variants}
    for rep in range(reps):  # the variants alternate
        for name, fn in variants.items():
            samples[name].append(fn())
        print(workload, "rep", rep, flush=True)
    e.close()
    v = {name: summary(r) for name, r in samples.items()}
    answers, ratios = [], {}
    for k in range(5):
        a, b = v[f"b_safest_route_pair{k}"], v[f"b_min_risk_ceiling_pair{k}"]
        answers.append({"pair": k, "start_node": pairs[k][0], "goal_node": pairs[k][1],
                        "safest_route_max_risk": a["max_risk"], "min_risk_ceiling_max_risk": b["max_risk"],
                        "route_nodes": a["nodes"], "same_answer": a["max_risk"] == b["max_risk"] and
                        a["nodes"] == b["nodes"] and a["cost"] == b["cost"]})
        ratios[f"pair{k}_safest_over_min_risk_ceiling_wall"] = a["ms_wall_median"] / b["ms_wall_median"]
        ratios[f"start{k}_risk_over_cost_field_device"] = (v[f"a_risk_field_start{k}"]["ms_device_median"] /
                                                           v[f"a_cost_field_start{k}"]["ms_device_median"])
    return {"workload": workload, "V": V, "E": E, "weights": weights, "answers": answers, "ratios": ratios,
            "positive_ceilings": sum(1 for a in answers if a["safest_route_max_risk"] > 0),
            "variants": v, "cold": cold}


res = {"reps": reps, "field_delta_scale": 4, "S": S, "safety_factor": SF}
cloud = synth.mountain_tile(0, nx, 0, ny, seed=20250418)
res["c3"] = measure(f"C3-style {nx}x{ny} = {cloud.shape[0]} points", cloud, (nx * 0.05, ny * 0.05),
                    6.0 * min(nx, ny) / 3125.0)
cloud = synth.mountain_cloud(rough_n, rough_n, seed=11, amplitude=5.0, wavelength=14.0)
res["rough"] = measure(f"rough terrain (seed 11, amplitude 5 m, wavelength 14 m) {rough_n}x{rough_n} = "
                       f"{cloud.shape[0]} points", cloud, (rough_n * 0.05, rough_n * 0.05), rough_n * 0.05 / 25.0)
del cloud
res["note"] = ("ms_device = hipEvent time of the solve; ms_wall = host clock around the call.  (a): one full field "
               "read at the goal on the device.  (b): wall time of the whole call -- safest_route: two solves and a "
               "routes call; min_risk_ceiling: the graph download, the search's batches and the final route.")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
