#!/usr/bin/env python3
"""Run on the GPU box: what the routes of the cost field (Engine.routes, trg_engine_field_routes) cost, on the C3
graph set up as in scripts/cost_field_latency.py.  One process; after a warm-up the variants alternate, and the
medians are compared:

  (a) cheapest_frontiers for 16 and for 64 poses: on routes (this tree) against the way it ran before them --
      cost_fields(..., targets=frontier, full=True), three m x V arrays to the host, Engine.field_path per pose.
      The solve is the same code on both sides; what differs is what crosses to the host and who walks.  Both
      must return the same list.  A gain is claimed only where the difference of the medians exceeds the
      earlier way's own run-to-run spread (max - min) in this visit.
  (b) one routes call: a lone route to the node of most hops of one field (device time per hop of a dependent
      walk), and 64 x (number of Frontier nodes) routes of a 64-field solve, infos only and with ids.

--single-runs PARENT.json,... CHANGE.json,...: outputs of scripts/cost_field_latency.py on the parent commit and
on this tree, taken alternately in the same visit; their medians per start and the parent's own run-to-run spread
are folded into the result (the single-source path must not regress).

usage: python scripts/cost_field_routes_latency.py [--out PATH] [--reps N] [--single-runs P1,.. C1,..] [nx ny]
       -> PATH (default profiles/r08_cost_field_routes.json)
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "trg-planner_amd"))
import trg_planner  # noqa: E402
from trg_planner import synth  # noqa: E402
from trg_planner._engine import (TRG_FIELD_BATCH_MAX, TrgFieldInfo, TrgRouteInfo, _i,  # noqa: E402
                                 choose_frontier)

argv = sys.argv[1:]
out = os.path.join(ROOT, "profiles", "r08_cost_field_routes.json")
reps = 9
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
DELTA_SCALE = "4"  # the engine's default bucket width, set here so that the record states what ran
e.set_option("field_delta_scale", DELTA_SCALE)
e.set_sampler(7, 16)
e.set_global_map(cloud)
e.init_graph([cx, cy, 0.0])
V, E = e.graph_sizes("global")
n_points = int(cloud.shape[0])
del cloud
g = e.graph("global")
frontier = np.flatnonzero(g.state == 1).astype(np.int32)
xyz = g.xyz

# poses spread over the map: positions of reached nodes of the first start's field, evenly spaced in id order
cost0, hops0, _, info0 = e.cost_field(source_xy=starts[0])
reachable = np.flatnonzero(hops0 >= 0)
spread = {m: reachable[np.linspace(0, reachable.size - 1, m).astype(np.int64)].astype(np.int32) for m in (16, 64)}
poses = {m: np.ascontiguousarray(xyz[ids, :2]) for m, ids in spread.items()}
farthest = int(np.argmax(hops0))
far_hops = int(hops0[farthest])
del g


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def frontiers_before(xy):
    """Engine.cheapest_frontiers as it ran before routes: the parent arrays on the host, one host walk per pose."""
    res = []
    for k0 in range(0, xy.shape[0], TRG_FIELD_BATCH_MAX):
        r = e.cost_fields(sources_xy=xy[k0:k0 + TRG_FIELD_BATCH_MAX], targets=frontier)
        for k in range(r["sources"].shape[0]):
            pick = choose_frontier(frontier, r["cost_at"][k], r["hops_at"][k])
            if pick is None:
                res.append(None)
                continue
            best, j = pick
            res.append((best, float(r["cost_at"][k, j]), e.field_path(r["parent"][k], best, int(r["sources"][k]))))
    return res


def raw_routes(fields, targets, with_ids):
    """One trg_engine_field_routes call; with_ids: sized by a first infos-only call, which is not timed."""
    f = np.ascontiguousarray(fields, np.int32)
    t = np.ascontiguousarray(targets, np.int32)
    n = f.shape[0]
    infos = (TrgRouteInfo * n)()
    off = np.zeros(n + 1, np.int32)
    info = TrgFieldInfo()
    e._chk(e.L.trg_engine_field_routes(e.h, n, _i(f), _i(t), _i(off), None, None, 0, infos, C.byref(info)))
    total = int(np.frombuffer(infos, np.int32).reshape(n, 4)[:, 0].astype(np.int64).sum())
    rec = {"routes": n, "nodes": total}
    if with_ids and total < 2**31 - 1:
        ids = np.empty(max(total, 1), np.int32)
        t0 = time.perf_counter()
        e._chk(e.L.trg_engine_field_routes(e.h, n, _i(f), _i(t), _i(off), _i(ids), None, total, infos, C.byref(info)))
        rec["ms_wall"] = 1e3 * (time.perf_counter() - t0)
    rec["ms_device"] = info.ms_device
    rec["host_syncs"] = info.host_syncs
    return rec


variants = {}
for m in (16, 64):
    variants[f"a_frontiers_before_m{m}"] = (lambda m=m: timed(lambda: frontiers_before(poses[m])))
    variants[f"a_frontiers_routes_m{m}"] = (lambda m=m: timed(lambda: e.cheapest_frontiers(poses[m])))

equal = {}
for m in (16, 64):  # warm-up, and the two ways must agree
    a = variants[f"a_frontiers_before_m{m}"]()[0]
    b = variants[f"a_frontiers_routes_m{m}"]()[0]
    equal[str(m)] = bool(a == b)
    variants[f"a_frontiers_before_m{m}"]()
    variants[f"a_frontiers_routes_m{m}"]()
samples = {name: [] for name in variants}
for rep in range(reps):  # the variants alternate
    for name, fn in variants.items():
        samples[name].append(fn()[1])
    print("rep", rep, flush=True)

res = {"workload": f"C3-style {nx}x{ny} = {n_points} points, S={S}", "V": V, "E": E, "reps": reps,
       "frontier_nodes": int(frontier.size), "field_delta_scale": float(DELTA_SCALE), "frontiers_equal": equal, "a": {}}
for m in (16, 64):
    before = np.array(samples[f"a_frontiers_before_m{m}"])
    routes = np.array(samples[f"a_frontiers_routes_m{m}"])
    spread_before = float(before.max() - before.min())
    diff = float(np.median(before) - np.median(routes))
    res["a"][str(m)] = {"before_ms_wall_median": float(np.median(before)), "before_ms_wall_min": float(before.min()),
                        "before_ms_wall_max": float(before.max()), "before_spread": spread_before,
                        "routes_ms_wall_median": float(np.median(routes)), "routes_ms_wall_min": float(routes.min()),
                        "routes_ms_wall_max": float(routes.max()), "before_minus_routes": diff,
                        "gain_exceeds_spread": bool(diff > spread_before),
                        "loss_exceeds_spread": bool(-diff > spread_before)}

# (b) one lone route, then 64 x Frontier routes
e.cost_fields(source_ids=[int(info0.source)], full=False)
raw_routes([0], [farthest], False)  # (the late parent sweep runs in this one)
lone = [raw_routes([0], [farthest], False) for _ in range(reps)]
lone_ids = [raw_routes([0], [farthest], True) for _ in range(reps)]
dev = float(np.median([r["ms_device"] for r in lone]))
res["b_lone_route"] = {"hops": far_hops, "nodes": lone[0]["nodes"], "ms_device_median": dev,
                       "us_per_hop": 1e3 * dev / max(far_hops, 1),
                       "with_ids_ms_wall_median": float(np.median([r["ms_wall"] for r in lone_ids]))}
r64 = e.cost_fields(source_ids=spread[64], targets=frontier, full=False)
nf = int(frontier.size)
ff = np.repeat(np.arange(64, dtype=np.int32), nf)
tt = np.tile(frontier, 64)
raw_routes(ff, tt, False)
many = [raw_routes(ff, tt, False) for _ in range(reps)]
res["b_64_x_frontier"] = {"routes": many[0]["routes"], "nodes": many[0]["nodes"],
                          "ms_device_median": float(np.median([r["ms_device"] for r in many])),
                          "solve_ms_device": float(r64["info"].ms_device)}
if many[0]["nodes"] <= 200_000_000:
    many_ids = [raw_routes(ff, tt, True) for _ in range(3)]
    res["b_64_x_frontier"]["with_ids_ms_wall_median"] = float(np.median([r["ms_wall"] for r in many_ids]))
    res["b_64_x_frontier"]["with_ids_ms_device_median"] = float(np.median([r["ms_device"] for r in many_ids]))

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
res["note"] = ("(a) 'before' is the earlier cheapest_frontiers re-implemented in this script (full m x V downloads, "
               "Engine.field_path on the host) on this tree's library, alternating with the new one in one process; it "
               "is not a build of the parent commit. ms_wall = host clock around the whole call. (b) ms_device = hipEvent time of the routes call; in an "
               "infos-only call (no ids) that is the parent sweep if it is due and the walk; with ids it spans the host's "
               "prefix sum between the length and the walk kernels.")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
