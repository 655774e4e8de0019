#!/usr/bin/env python3
"""Run on the GPU box: what a bounded cost field (Engine.cost_fields with budget / settle, the early_exit helpers,
Engine.reachable; DESIGN.md section 2, "Bounded fields") costs next to the full solve, on the C3 graph set up as in
scripts/cost_field_latency.py, from that script's five start points.  One process; after a warm-up of every shape
the variants alternate, and the medians of `reps` samples are compared:

  (a) per start: budgets at the 1 %, 10 % and 50 % quantile of the full field's costs against the unbounded solve
      (all four without full outputs: what differs is the solve)
  (b) cheapest_frontiers for 1, 16 and 64 poses, early_exit on and off -- and, because a terrain built in one piece
      may have no Frontier node at all (the count is recorded), the same solve with settle "any" over the nodes of a
      ring 15 .. 20 m around each pose's first start, on and off
  (c) plan_many to 8 goals within 20 m of the start, early_exit on and off
  (d) reachable(start, budget) against cost_field plus filtering on the host, at the 1 % and 10 % budgets
  (e) --single-runs PARENT.json,... CHANGE.json,...: outputs of scripts/cost_field_latency.py on the parent commit
      and on this tree, taken alternately in the same visit; the change must stay within the parent's own
      run-to-run spread (the unbounded single-source path launches what it launched before)

Device time is the hipEvent time of the solve (TrgFieldInfo.ms_device), wall time the host clock around the call.

usage: python scripts/cost_field_bounded_latency.py [--out PATH] [--reps N] [--single-runs P1,.. C1,..] [nx ny]
       -> PATH (default profiles/r09_cost_field_bounded.json)
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
out = os.path.join(ROOT, "profiles", "r09_cost_field_bounded.json")
reps = 15
single_runs = None
if "--out" in argv:
    i = argv.index("--out")
    out = os.path.abspath(argv[i + 1])
    del argv[i:i + 2]
if "--reps" in argv:
    i = argv.index("--reps")
    reps = int(argv[i + 1])
    del argv[i:i + 2]
if "--single-runs" in argv:
    i = argv.index("--single-runs")
    single_runs = (argv[i + 1].split(","), argv[i + 2].split(","))
    del argv[i:i + 3]
args = [a for a in argv if not a.startswith("--")]
nx, ny = (int(args[0]), int(args[1])) if len(args) >= 2 else (3200, 3125)
S = 16
prm = dict(expand_dist=0.6, robot_size=0.3, sample_num=S, height_threshold=0.16, collision_threshold=0.1,
           update_collision_threshold=0.1, safety_factor=3.0, goal_tolerance=0.8)
cloud = synth.mountain_tile(0, nx, 0, ny, seed=20250418)
cx, cy = nx * 0.05, ny * 0.05
ref_s = np.array([[-7.22, -7.54], [-2.07, -2.21], [13.04, -1.99], [17.96, 17.69], [-6.56, 4.59]], np.float32)
scale = 6.0 * min(nx, ny) / 3125.0
starts = (ref_s * scale + np.array([cx, cy], np.float32)).astype(np.float32)

e = trg_planner.Engine(**prm)
e.set_sampler(7, 16)
e.set_global_map(cloud)
e.init_graph([cx, cy, 0.0])
V, E = e.graph_sizes("global")
n_points = int(cloud.shape[0])
del cloud
g = e.graph("global")
xy = g.xyz[:, :2].copy()
n_frontier = int(np.sum(g.state == 1))
QUANTILES = (0.01, 0.10, 0.50)

# the full fields of the five starts: budgets at the cost quantiles of the reached nodes, what they reach, and a ring
budgets, reach_share, rings, src_nodes = [], [], [], []
for s in starts:
    cost, hops, _, info = e.cost_field(source_xy=s)
    c = np.sort(cost[(hops >= 0) & np.isfinite(cost)])
    b = [float(c[int(q * (c.size - 1))]) for q in QUANTILES]
    budgets.append(b)
    reach_share.append([float(np.sum((hops >= 0) & (cost <= x)) / V) for x in b])
    d = np.hypot(xy[:, 0] - xy[info.source, 0], xy[:, 1] - xy[info.source, 1])
    rings.append(np.flatnonzero((d >= 15.0) & (d <= 20.0) & (hops >= 0)).astype(np.int32))
    src_nodes.append(int(info.source))
cost0, hops0, _, _ = e.cost_field(source_xy=starts[0])
reachable0 = np.flatnonzero(hops0 >= 0)
poses = {m: xy[reachable0[np.linspace(0, reachable0.size - 1, m).astype(np.int64)]].astype(np.float32)
         for m in (1, 16, 64)}
poses[1] = starts[:1].copy()
ang = np.linspace(0.0, 2.0 * np.pi, 8, endpoint=False)
goals = (starts[0] + np.stack([np.cos(ang), np.sin(ang)], 1) * np.linspace(6.0, 20.0, 8)[:, None]).astype(np.float32)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def solve(**kw):
    r, wall = timed(lambda: e.cost_fields(full=False, **kw))
    i = r["info"]
    return {"ms_device": i.ms_device, "ms_wall": wall, "rounds": i.rounds, "host_syncs": i.host_syncs,
            "reached": int(r["reached"].sum())}


def wall_only(fn):
    _, wall = timed(fn)
    return {"ms_wall": wall}


def filter_on_host(k, b):
    cost, hops, _, _ = e.cost_field(source_xy=starts[k])
    ids = np.flatnonzero((hops >= 0) & (cost <= np.float32(b)))
    return ids, cost[ids], hops[ids]


variants = {}
for k in range(len(starts)):
    variants[f"a_start{k}_unbounded"] = (lambda k=k: solve(sources_xy=starts[k:k + 1]))
    for q, b in zip(QUANTILES, budgets[k]):
        variants[f"a_start{k}_budget_q{int(100 * q):02d}"] = (lambda k=k, b=b: solve(sources_xy=starts[k:k + 1], budget=b))
for m in poses:
    for on in (False, True):
        variants[f"b_cheapest_frontiers_m{m}_{'on' if on else 'off'}"] = (
            lambda m=m, on=on: wall_only(lambda: e.cheapest_frontiers(poses[m], early_exit=on)))
for k in (0, 3):
    variants[f"b_ring_start{k}_off"] = (lambda k=k: solve(source_ids=[src_nodes[k]], targets=rings[k]))
    variants[f"b_ring_start{k}_on"] = (lambda k=k: solve(source_ids=[src_nodes[k]], targets=rings[k], settle="any"))
variants["b_ring_five_starts_off"] = lambda: solve(source_ids=src_nodes, targets=rings[0])
variants["b_ring_five_starts_on"] = lambda: solve(source_ids=src_nodes, targets=rings[0], settle="any")
for on in (False, True):
    variants[f"c_plan_many_8_goals_{'on' if on else 'off'}"] = (
        lambda on=on: wall_only(lambda: e.plan_many(starts[0], goals, early_exit=on)))
for q, b in zip(QUANTILES[:2], budgets[0][:2]):
    variants[f"d_reachable_q{int(100 * q):02d}"] = (lambda b=b: wall_only(lambda: e.reachable(starts[0], b)))
    variants[f"d_cost_field_and_filter_q{int(100 * q):02d}"] = (lambda b=b: wall_only(lambda: filter_on_host(0, b)))

for name, fn in variants.items():  # warm-up: every shape once (buffers grow to the largest batch here)
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
       "field_delta_scale": 4, "frontier_nodes": n_frontier, "budgets": budgets, "budget_reach_share": reach_share,
       "ring_targets": [int(r.size) for r in rings], "variants": {name: summary(r) for name, r in samples.items()}}
v = res["variants"]
ratios = {}
for k in range(len(starts)):
    for q in QUANTILES:
        n = f"a_start{k}_budget_q{int(100 * q):02d}"
        ratios[n + "_over_unbounded_device"] = v[n]["ms_device_median"] / v[f"a_start{k}_unbounded"]["ms_device_median"]
for name in list(v):
    if name.endswith("_on"):
        key = "ms_device_median" if "ms_device_median" in v[name] else "ms_wall_median"
        ratios[name + "_over_off_" + key[3:-7]] = v[name][key] / v[name[:-3] + "_off"][key]
for q in QUANTILES[:2]:
    t = f"q{int(100 * q):02d}"
    ratios[f"d_reachable_over_filter_wall_{t}"] = (v[f"d_reachable_{t}"]["ms_wall_median"] /
                                                   v[f"d_cost_field_and_filter_{t}"]["ms_wall_median"])
res["ratios"] = ratios

if single_runs is not None:
    def medians(paths):
        runs = [json.load(open(p)) for p in paths]
        return np.array([[r["ms_device_median"] for r in run["device_csr"]] for run in runs], np.float64)
    parent, change = medians(single_runs[0]), medians(single_runs[1])
    p_med, c_med = np.median(parent, axis=0), np.median(change, axis=0)
    p_spread = parent.max(axis=0) - parent.min(axis=0)
    res["single_source_regression"] = {
        "what": "ms_device_median per start of scripts/cost_field_latency.py (device-resident CSR), runs of the "
                "parent commit and of this change alternating in one visit",
        "parent_runs": parent.tolist(), "change_runs": change.tolist(),
        "parent_median": p_med.tolist(), "change_median": c_med.tolist(),
        "parent_run_to_run_spread": p_spread.tolist(),
        "change_minus_parent": (c_med - p_med).tolist(),
        "within_parent_spread": bool(np.all(c_med - p_med <= p_spread)),
    }
res["note"] = ("ms_device = hipEvent time of the solve; ms_wall = host clock around the call. (a) and the ring solves "
               "of (b) download nothing of V entries; cheapest_frontiers, plan_many and reachable are timed as wall "
               "time of the whole helper; cost_field_and_filter downloads cost, hops and parent in full.")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
