#!/usr/bin/env python3
"""Run on the GPU box: what a batch of cost fields (Engine.cost_fields, trg_engine_cost_field_batch) costs next to
the same fields one after another, on the C3 graph set up as in scripts/cost_field_latency.py, from that script's
five start points.  One process; after a warm-up of every shape the variants alternate, and the medians are
compared:

  (a) one cost_field per start                     (b) the five starts in sequence
  (c) one batch of the five                        (d) batches of m = 2, 8, 16, 32, 64 sources spread over the map
  (e) cost_matrix of 16 nodes against 16 single fields with their full downloads

Device time is the hipEvent time of the solve (TrgFieldInfo.ms_device), wall time the host clock around the call,
downloads included.  Two conditions are evaluated and recorded, with their ratios: (c) takes less device time than
(b), and (d) at m = 8 less than 8 x the median of (a).

--single-runs PARENT.json,... CHANGE.json,...: outputs of scripts/cost_field_latency.py on the parent commit and
on this tree, taken alternately in the same visit; their medians per start and the parent's own run-to-run spread
are folded into the result (the single-source path must not regress).

usage: python scripts/cost_field_batch_latency.py [--out PATH] [--reps N] [--single-runs P1,P2,.. C1,C2,..] [nx ny]
       -> PATH (default profiles/r07_cost_field_batch.json)
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
from trg_planner._engine import TRG_FIELD_BATCH_MAX  # noqa: E402

argv = sys.argv[1:]
out = os.path.join(ROOT, "profiles", "r07_cost_field_batch.json")
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

# sources spread over the map: reached nodes of the first start's field, evenly spaced in id (creation) order
cost0, hops0, _, info0 = e.cost_field(source_xy=starts[0])
reachable = np.flatnonzero(hops0 >= 0)
spread = {m: reachable[np.linspace(0, reachable.size - 1, m).astype(np.int64)].astype(np.int32)
          for m in (2, 8, 16, 32, TRG_FIELD_BATCH_MAX)}
del cost0, hops0


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def single(k):
    (_, _, _, info), wall = timed(lambda: e.cost_field(source_xy=starts[k]))
    return {"ms_device": info.ms_device, "ms_wall": wall, "rounds": info.rounds, "host_syncs": info.host_syncs}


def sequence():
    def run():
        return [e.cost_field(source_xy=s)[3] for s in starts]
    infos, wall = timed(run)
    return {"ms_device": sum(i.ms_device for i in infos), "ms_wall": wall, "rounds": sum(i.rounds for i in infos),
            "host_syncs": sum(i.host_syncs for i in infos)}


def batch_of_starts():
    r, wall = timed(lambda: e.cost_fields(sources_xy=starts))
    i = r["info"]
    return {"ms_device": i.ms_device, "ms_wall": wall, "rounds": i.rounds, "host_syncs": i.host_syncs}


def batch_spread(m):
    # read at the sources on the device: no download of m x V, which at m = 64 would be 490 MB
    r, wall = timed(lambda: e.cost_fields(source_ids=spread[m], targets=spread[m], full=False))
    i = r["info"]
    return {"ms_device": i.ms_device, "ms_wall": wall, "rounds": i.rounds, "host_syncs": i.host_syncs}


def matrix16():
    (mc, mh, ids), wall = timed(lambda: e.cost_matrix(spread[16]))
    return {"ms_wall": wall}


def singles16():
    def run():
        return [e.cost_field(source_id=int(s))[3] for s in spread[16]]
    infos, wall = timed(run)
    return {"ms_device": sum(i.ms_device for i in infos), "ms_wall": wall}


variants = {f"a_single_start{k}": (lambda k=k: single(k)) for k in range(len(starts))}
variants["b_five_in_sequence"] = sequence
variants["c_batch_of_five"] = batch_of_starts
for m in spread:
    variants[f"d_batch_m{m}"] = (lambda m=m: batch_spread(m))
variants["e_cost_matrix_16"] = matrix16
variants["e_16_single_fields"] = singles16

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
       "field_delta_scale": 4, "variants": {name: summary(r) for name, r in samples.items()}}
v = res["variants"]
a_dev = [v[f"a_single_start{k}"]["ms_device_median"] for k in range(len(starts))]
a_med = float(np.median(a_dev))
cond = {
    "c_over_b_device": v["c_batch_of_five"]["ms_device_median"] / v["b_five_in_sequence"]["ms_device_median"],
    "c_over_b_wall": v["c_batch_of_five"]["ms_wall_median"] / v["b_five_in_sequence"]["ms_wall_median"],
    "a_median_of_starts_ms_device": a_med,
    "d_over_m_singles_device": {str(m): v[f"d_batch_m{m}"]["ms_device_median"] / (m * a_med) for m in spread},
    "e_matrix_over_16_singles_wall": v["e_cost_matrix_16"]["ms_wall_median"] / v["e_16_single_fields"]["ms_wall_median"],
}
cond["batch_of_five_pays"] = bool(cond["c_over_b_device"] < 1.0)
cond["batch_m8_pays"] = bool(cond["d_over_m_singles_device"]["8"] < 1.0)
cond["batch_loses_at_m"] = [m for m in spread if cond["d_over_m_singles_device"][str(m)] >= 1.0]
res["conditions"] = cond

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
res["note"] = ("ms_device = hipEvent time of the solve; ms_wall = host clock around the call, downloads included. "
               "(a), (b), (c) and the 16 single fields of (e) download cost, hops and parent in full; (d) and the "
               "cost matrix read the fields at the sources on the device and download m x m numbers.")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
