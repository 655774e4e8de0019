#!/usr/bin/env python3
"""Run on the GPU box: latency of the cost field (Engine.cost_field, trg_field.hip) on the C3 graph, set up as in
scripts/plan_latency.py, from that script's five start points -- on the device-resident CSR of the build and on
the uploaded CSR after one updateGraph -- with the host Dijkstra of tests/cpp/field_reference.cpp timed on one
host core on the same CSR, planSafePath per query for scale, and the bucket-width rules side by side.

usage: python scripts/cost_field_latency.py [--out PATH] [nx ny]   -> PATH (default profiles/r04_cost_field.json)
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "trg-planner_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import trg_planner  # noqa: E402
from trg_planner import synth  # noqa: E402
import field_ref  # noqa: E402  (the host reference, timed beside the engine)

argv = sys.argv[1:]
out = os.path.join(ROOT, "profiles", "r04_cost_field.json")
if "--out" in argv:
    i = argv.index("--out")
    out = os.path.abspath(argv[i + 1])
    del argv[i:i + 2]
args = [a for a in argv if not a.startswith("--")]
nx, ny = (int(args[0]), int(args[1])) if len(args) >= 2 else (3200, 3125)
S = 16
prm = dict(expand_dist=0.6, robot_size=0.3, sample_num=S, height_threshold=0.16, collision_threshold=0.1,
           update_collision_threshold=0.1, safety_factor=3.0, goal_tolerance=0.8)
cloud = synth.mountain_tile(0, nx, 0, ny, seed=20250418)
cx, cy = nx * 0.05, ny * 0.05
start_pose = [cx, cy, 0.0]
# plan_latency.py's five start / goal pairs
ref_s = np.array([[-7.22, -7.54], [-2.07, -2.21], [13.04, -1.99], [17.96, 17.69], [-6.56, 4.59]], np.float32)
ref_g = np.array([[-9.97, 3.56], [7.52, 1.44], [14.43, 6.87], [9.49, 16.60], [3.11, -6.68]], np.float32)
scale = 6.0 * min(nx, ny) / 3125.0
starts = (ref_s * scale + np.array([cx, cy], np.float32)).astype(np.float32)
goals = np.concatenate([ref_g * scale + np.array([cx, cy], np.float32), np.zeros((5, 1), np.float32)], 1).astype(np.float32)
lib = field_ref.compile_reference(tempfile.mkdtemp())

e = trg_planner.Engine(**prm)
e.set_sampler(7, 16)
e.set_global_map(cloud)
e.init_graph(start_pose)
V, E = e.graph_sizes("global")


def fields(tag, check_graph=None):
    recs = []
    for s in starts:
        for _ in range(3):
            e.cost_field(source_xy=s)
        dev, tot = [], []
        for _ in range(20):
            cost, hops, parent, info = e.cost_field(source_xy=s)
            dev.append(info.ms_device)
            tot.append(info.ms_total)
        rec = {"source": int(info.source), "reached": int(info.reached), "rounds": int(info.rounds),
               "host_syncs": int(info.host_syncs), "ms_device_median": float(np.median(dev)),
               "ms_total_median": float(np.median(tot)), "ms_device_min": float(np.min(dev))}
        if check_graph is not None:
            g = check_graph
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                st, rc, rh, rp = field_ref.field_of_graph(lib, g, prm["safety_factor"], info.source)
                ts.append(time.perf_counter() - t0)
            rec["host_reference_ms_median"] = 1e3 * float(np.median(ts))
            rec["equal_to_reference"] = bool(st == 0 and np.array_equal(cost.view(np.uint32), rc.view(np.uint32))
                                             and np.array_equal(hops, rh) and np.array_equal(parent, rp))
        recs.append(rec)
        print(tag, json.dumps(rec), flush=True)
    return recs


g = e.graph("global")
res = {"workload": f"C3-style {nx}x{ny} = {cloud.shape[0]} points, S={S}", "V": V, "E": E,
       "host_cpu": open("/proc/cpuinfo").read().split("model name")[1].split("\n")[0].strip(": \t")}
res["device_csr"] = fields("device", g)
# planSafePath per query, for scale
pl = []
for s, q in zip(starts, goals):
    e.plan(s, q)
    ts = []
    for _ in range(10):
        t0 = time.perf_counter()
        e.plan(s, q)
        ts.append(time.perf_counter() - t0)
    pl.append(1e3 * float(np.median(ts)))
res["plan_ms_per_query_median"] = pl
# bucket-width rules (field_delta_scale: delta = scale x mean edge cost; inf = Bellman-Ford), first start
rules = {}
for sc in ("1", "4", "16", "inf"):
    e.set_option("field_delta_scale", sc)
    for _ in range(3):
        e.cost_field(source_xy=starts[0])
    dev, rounds = [], 0
    for _ in range(10):
        _, _, _, info = e.cost_field(source_xy=starts[0])
        dev.append(info.ms_device)
        rounds = int(info.rounds)
    rules[sc] = {"ms_device_median": float(np.median(dev)), "rounds": rounds, "host_syncs": int(info.host_syncs)}
    print("rule", sc, rules[sc], flush=True)
e.set_option("field_delta_scale", "4")
res["delta_rules_start0"] = rules
# the uploaded CSR: after one updateGraph the device build's CSR is stale
m = (np.abs(cloud[:, 0] - cx) < 4.0) & (np.abs(cloud[:, 1] - cy) < 4.0)
e.set_local_map((cx, cy), cloud[m].copy())
e.update_graph()
g2 = e.graph("global")
res["V_after_update"] = g2.V
res["uploaded_csr"] = fields("uploaded", g2)
# first call after the update: the upload and the edge costs included
e.update_graph()
_, _, _, info = e.cost_field(source_xy=starts[0])
res["uploaded_first_call"] = {"ms_device": info.ms_device, "ms_total": info.ms_total, "host_syncs": info.host_syncs}
# algorithmic bytes of one full sweep: column + cost + target key per edge, ~16 B per node
res["bytes_per_full_sweep"] = 16 * E + 16 * V
res["note"] = ("ms_device = hipEvent time of the solve (two near-far passes, parents, outputs); ms_total = host wall "
               "time incl. the downloads of cost/hops/parent; host reference = std::priority_queue Dijkstra on one "
               "host core, same CSR, same key")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
