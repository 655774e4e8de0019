#!/usr/bin/env python3
"""Run on the GPU box: what a cost model per field (Engine.cost_fields(models=...), trg_engine_cost_field_models;
DESIGN.md section 2, "Cost models") costs, on the C3 graph set up as in scripts/cost_field_batch_latency.py.  One
process; after a warm-up of every shape the variants alternate, and the medians are compared:

  (a) a batch of 8 fields from one start, models=None      (b) the same with 8 explicit copies of the engine's model
  (c) 8 safety factors 0 .. 8, no ceiling                  (d) 8 ceilings: 0 and quantiles of the positive weights
  (e) plan_tradeoff of the 8 models of (c) against 8 single bounded solves (settle "any" at the goal) in sequence
  (f) min_risk_ceiling for the five start / goal pairs of scripts/plan_latency.py

(a) and (b) read one cache slot and run the plain kernels; (c) and (d) read 8 slots through the MODELS kernels.  All
batches are read at the goal on the device (no download of 8 x V).  Device time is the hipEvent time of the solve
(TrgFieldInfo.ms_device), wall time the host clock around the call.  The edge costs of every model are cached after
the warm-up; the first call of each shape, which computes them, is recorded apart as "cold".

usage: python scripts/cost_field_models_latency.py [--out PATH] [--reps N] [nx ny]
       -> PATH (default profiles/r16_cost_field_models.json)
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
out = os.path.join(ROOT, "profiles", "r16_cost_field_models.json")
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
SF = 3.0
prm = dict(expand_dist=0.6, robot_size=0.3, sample_num=S, height_threshold=0.16, collision_threshold=0.1,
           update_collision_threshold=0.1, safety_factor=SF, goal_tolerance=0.8)
cloud = synth.mountain_tile(0, nx, 0, ny, seed=20250418)
cx, cy = nx * 0.05, ny * 0.05
ref_s = np.array([[-7.22, -7.54], [-2.07, -2.21], [13.04, -1.99], [17.96, 17.69], [-6.56, 4.59]], np.float32)
ref_g = np.array([[-9.97, 3.56], [7.52, 1.44], [14.43, 6.87], [9.49, 16.60], [3.11, -6.68]], np.float32)
scale = 6.0 * min(nx, ny) / 3125.0
starts = (ref_s * scale + np.array([cx, cy], np.float32)).astype(np.float32)
goals = (ref_g * scale + np.array([cx, cy], np.float32)).astype(np.float32)

e = trg_planner.Engine(**prm)
e.set_sampler(7, 16)
e.set_global_map(cloud)
e.init_graph([cx, cy, 0.0])
V, E = e.graph_sizes("global")
n_points = int(cloud.shape[0])
del cloud

g = e.graph("global")
w_valid = np.sort(g.w[g.state[g.col] != -1])
zero_share = float(np.mean(w_valid == 0))
w_pos = w_valid[w_valid > 0] if np.any(w_valid > 0) else w_valid  # (most C3 edges weigh 0: quantiles of the rest)
quantiles = [0.0, 0.25, 0.5, 0.75, 0.9, 0.99, 0.999, 1.0]
ceilings = [0.0] + [float(w_pos[min(int(q * w_pos.size), w_pos.size - 1)]) for q in quantiles[1:]]
del g
start, goal = (int(v) for v in e._resolve_nodes([starts[0], goals[0]]))
M = 8
factors = [float(k) * 8.0 / 7.0 for k in range(M)]  # 0 .. 8
shapes = {"a_models_none": None, "b_engine_model_x8": [(SF, np.inf)] * M, "c_safety_factors": factors,
          "d_ceilings": [(SF, c) for c in ceilings]}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def batch(models):
    r, wall = timed(lambda: e.cost_fields(source_ids=[start] * M, targets=[goal], full=False, models=models))
    i = r["info"]
    return {"ms_device": i.ms_device, "ms_wall": wall, "rounds": i.rounds, "host_syncs": i.host_syncs,
            "reached": int(r["reached"].sum())}


def tradeoff():
    recs, wall = timed(lambda: e.plan_tradeoff(starts[0], goals[0], factors))
    return {"ms_wall": wall, "reachable": sum(r["reachable"] for r in recs)}


def singles():
    def run():
        n = 0
        for f in factors:
            r = e.cost_fields(source_ids=[start], targets=[goal], full=False, settle="any", models=[f])
            n += e.routes([0], [goal], hops_at=r["hops_at"][:, 0])[0][2].num_nodes > 0
        return n
    n, wall = timed(run)
    return {"ms_wall": wall, "reachable": n}


def minimax(k):
    got, wall = timed(lambda: e.min_risk_ceiling(starts[k], goals[k]))
    return {"ms_wall": wall, "max_risk": -1.0 if got is None else got[0],
            "nodes": 0 if got is None else int(got[1]["ids"].size)}


variants = {name: (lambda mo=mo: batch(mo)) for name, mo in shapes.items()}
variants["e_plan_tradeoff"] = tradeoff
variants["e_8_single_solves"] = singles
for k in range(len(starts)):
    variants[f"f_min_risk_ceiling_pair{k}"] = (lambda k=k: minimax(k))

cold = {name: fn() for name, fn in variants.items()}  # the first call of every shape computes its models' costs
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
        vals = np.array([r[key] for r in recs], np.float64)
        if key.startswith("ms_"):
            s[key + "_median"] = float(np.median(vals))
            s[key + "_min"] = float(vals.min())
            s[key + "_max"] = float(vals.max())
        else:
            s[key] = float(vals[-1])
    return s


res = {"workload": f"C3-style {nx}x{ny} = {n_points} points, S={S}", "V": V, "E": E, "reps": reps,
       "field_delta_scale": 4, "start_node": start, "goal_node": goal, "safety_factors": factors,
       "ceilings": dict(zip(map(str, quantiles), ceilings)), "zero_weight_share": zero_share,
       "variants": {name: summary(r) for name, r in samples.items()}, "cold": cold}
v = res["variants"]
res["ratios"] = {
    "b_over_a_device": v["b_engine_model_x8"]["ms_device_median"] / v["a_models_none"]["ms_device_median"],
    "c_over_a_device": v["c_safety_factors"]["ms_device_median"] / v["a_models_none"]["ms_device_median"],
    "d_over_a_device": v["d_ceilings"]["ms_device_median"] / v["a_models_none"]["ms_device_median"],
    "e_tradeoff_over_singles_wall": v["e_plan_tradeoff"]["ms_wall_median"] / v["e_8_single_solves"]["ms_wall_median"],
}
res["note"] = ("ms_device = hipEvent time of the solve; ms_wall = host clock around the call.  (a)-(d): 8 full fields "
               "from one start read at the goal on the device.  (b) goes through the sets entry (the sources are "
               "resolved by a call of their own first), (a) through the batch entry.  (f): wall time of the whole "
               "search, its solves and the final route.")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
