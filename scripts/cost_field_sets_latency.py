#!/usr/bin/env python3
"""Run on the GPU box: what a cost field from a source SET (Engine.cost_fields_from, trg_engine_cost_field_sets)
costs next to the same question answered with a batch of single-source fields and a host argmin, on the C3 graph
set up as in scripts/cost_field_latency.py.  One process; after a warm-up of every shape the variants alternate,
and the medians are compared:

  (a) one set of n = 1, 2, 8, 16, 64 sources spread over the map, cost / hops / owner read at a ring of targets
  (b) the existing way: a cost_fields batch of the same sources read at the same targets, argmin on the host
  (c) one set of 4 096 sources
  (d) the owner pass alone: a set solve WITHOUT owners, then one one-node route -- that routes call runs the late
      parent sweep, the owner pass and a walk of no steps; next to it the same call after a plain single-source
      solve (the late parent sweep and the walk), so that the difference is the owner pass; its sweeps come back
      in TrgFieldInfo.rounds of the routes call
  (e) the set of 64 without owners (the seeding and the passes alone)

Device time is the hipEvent time of the solve (TrgFieldInfo.ms_device), wall time the host clock around the call.
Nothing of V entries is copied back in any variant.  The C3 terrain has no Frontier node, so assign_frontiers is
not timed; (a) at the ring is the solve it would run.

--single-runs PARENT.json,... CHANGE.json,...: outputs of scripts/cost_field_latency.py on the parent commit and
on this tree, taken alternately in the same visit (the single-source path must not regress).

usage: python scripts/cost_field_sets_latency.py [--out PATH] [--reps N] [--single-runs P1,P2,.. C1,C2,..] [nx ny]
       -> PATH (default profiles/r11_cost_field_sets.json)
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
from trg_planner._engine import TrgFieldInfo, _f, _i  # noqa: E402

argv = sys.argv[1:]
out = os.path.join(ROOT, "profiles", "r11_cost_field_sets.json")
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
scale = 6.0 * min(nx, ny) / 3125.0
start = (np.array([-7.22, -7.54], np.float32) * scale + np.array([cx, cy], np.float32)).astype(np.float32)

e = trg_planner.Engine(**prm)
e.set_sampler(7, 16)
e.set_global_map(cloud)
e.init_graph([cx, cy, 0.0])
V, E = e.graph_sizes("global")
n_points = int(cloud.shape[0])
del cloud

# sources spread over the map: reached nodes of the start's field, evenly spaced in id (creation) order; the
# targets: the ring of nodes 15 - 20 m from the start
cost0, hops0, _, info0 = e.cost_field(source_xy=start)
reachable = np.flatnonzero(hops0 >= 0)
SIZES = (1, 2, 8, 16, 64)
spread = {n: reachable[np.linspace(0, reachable.size - 1, n).astype(np.int64)].astype(np.int32)
          for n in SIZES + (4096,)}
spread[1] = np.array([info0.source], np.int32)
xy = e.node_xyz("global")[:, :2]
d = np.hypot(xy[:, 0] - start[0], xy[:, 1] - start[1])
ring = np.flatnonzero((d >= 15.0) & (d <= 20.0) & (hops0 >= 0)).astype(np.int32)
frontier_nodes = int(e._frontier_ids().size)
del cost0, hops0, xy, d


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def rec(info, wall, **more):
    return dict({"ms_device": info.ms_device, "ms_wall": wall, "rounds": info.rounds, "host_syncs": info.host_syncs},
                **more)


def set_field(n):
    r, wall = timed(lambda: e.cost_fields_from([spread[n]], targets=ring, full=False))
    return rec(r["info"], wall, owners_in_use=int(np.count_nonzero(r["owned"][0])))


def batch_argmin(n):
    def run():
        r = e.cost_fields(source_ids=spread[n], targets=ring, full=False)
        return r, np.argmin(r["cost_at"], axis=0)
    (r, _), wall = timed(run)
    return rec(r["info"], wall)


def set_without_owners(n):
    """The raw entry with cost_at alone: no owner pass, no parent sweep."""
    ptr = np.array([0, spread[n].size], np.int32)
    at = np.empty(ring.size, np.float32)
    info = TrgFieldInfo()

    def run():
        e._chk(e.L.trg_engine_cost_field_sets(e.h, 1, _i(ptr), _i(spread[n]), None, 0, None, None, None, None,
                                              _i(ring), ring.size, _f(at), None, None, None, None, None,
                                              C.byref(info)))
    _, wall = timed(run)
    return rec(info, wall)


def late_route(n):
    """(d): the routes call after a solve without owners (n sources as a set), or after a plain solve (n == 0)."""
    if n:
        set_without_owners(n)
        target = int(spread[n][0])
    else:
        e.cost_fields(source_ids=spread[1], full=False)
        target = int(spread[1][0])
    (_, info), wall = timed(lambda: e.routes([0], [target], xyz=False, hops_at=[0], with_info=True))
    return {"ms_device": info.ms_device, "ms_wall": wall, "sweeps": info.rounds, "host_syncs": info.host_syncs}


variants = {}
for n in SIZES:
    variants[f"a_set_n{n}"] = (lambda n=n: set_field(n))
    variants[f"b_batch_argmin_n{n}"] = (lambda n=n: batch_argmin(n))
variants["c_set_n4096"] = lambda: set_field(4096)
variants["d_late_parents_and_walk"] = lambda: late_route(0)
variants["d_late_parents_owner_pass_and_walk_n1"] = lambda: late_route(1)
variants["d_late_parents_owner_pass_and_walk_n64"] = lambda: late_route(64)
variants["e_set_n64_without_owners"] = lambda: set_without_owners(64)

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
       "field_delta_scale": 4, "ring_targets": int(ring.size), "frontier_nodes": frontier_nodes,
       "variants": {name: summary(r) for name, r in samples.items()}}
v = res["variants"]
one = v["a_set_n1"]["ms_device_median"]
res["ratios"] = {
    "set_over_batch_argmin_device": {str(n): v[f"a_set_n{n}"]["ms_device_median"] /
                                     v[f"b_batch_argmin_n{n}"]["ms_device_median"] for n in SIZES},
    "set_over_batch_argmin_wall": {str(n): v[f"a_set_n{n}"]["ms_wall_median"] /
                                   v[f"b_batch_argmin_n{n}"]["ms_wall_median"] for n in SIZES},
    "set_of_n_over_single_source_set_device": {
        **{str(n): v[f"a_set_n{n}"]["ms_device_median"] / one for n in SIZES if n != 1},
        "4096": v["c_set_n4096"]["ms_device_median"] / one},
    "owner_pass_ms_device_n1": v["d_late_parents_owner_pass_and_walk_n1"]["ms_device_median"] -
                               v["d_late_parents_and_walk"]["ms_device_median"],
    "owner_pass_ms_device_n64": v["d_late_parents_owner_pass_and_walk_n64"]["ms_device_median"] -
                                v["d_late_parents_and_walk"]["ms_device_median"],
    "owners_in_solve_ms_device_n64": v["a_set_n64"]["ms_device_median"] -
                                     v["e_set_n64_without_owners"]["ms_device_median"],
}

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
res["note"] = ("ms_device = hipEvent time of the call; ms_wall = host clock around it. Every variant reads its "
               "fields at the ring on the device; (b) downloads n x ring numbers twice and takes the argmin on the "
               "host. (d): the owner pass includes its host waits, which the event time spans. assign_frontiers is "
               "not timed: the C3 terrain has no Frontier node (frontier_nodes above); (a) is the solve it runs.")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
