#!/usr/bin/env python3
"""Run on the GPU box: what bringing a retained RISK field through an updateGraph costs (Engine.refresh_risk_fields,
trg_engine_risk_field_refresh; DESIGN.md section 2, "Risk fields") next to solving it again.  Two terrains, one after
the other in one process: the C3 graph of scripts/cost_field_refresh_latency.py, nearly all of whose edges weigh 0, and
the rough terrain of scripts/risk_field_latency.py, whose risk fields take hundreds of rounds; on both the update
stream of scripts/cost_field_refresh_latency.py (20 m x 20 m local maps around a pose that moves 0.5 m per step, with
an injected obstacle) and the first start of scripts/plan_latency.py as the field's source.

Every update is followed by the refresh of the solve retained from before it (the engine's own node map) and then by
a fresh solve of the same sources on the same graph; the fresh solve is the yardstick.  Updates alternate between one
field, a batch of 8 (the start and 7 nodes spread over the graph) and the frontier helper -- safest_frontier from the
start's position with reuse=True, then with reuse=False; after a warm-up of each shape the medians over `reps` updates
per shape are compared.  Device time is the hipEvent time of the call (TrgFieldInfo.ms_device), wall time the host
clock around it; rounds, host waits and carried / V are recorded with them.  Nothing of V entries is copied back.

usage: python scripts/risk_field_refresh_latency.py [--out PATH] [--reps N] [--rough N] [nx ny]
       -> PATH (default profiles/r19_risk_field_refresh.json); --rough: the rough terrain has N x N points (1200)
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
out = os.path.join(ROOT, "profiles", "r19_risk_field_refresh.json")
reps = 15
rough_n = 1200
for flag in ("--out", "--reps", "--rough"):
    if flag in argv:
        i = argv.index(flag)
        if flag == "--out":
            out = os.path.abspath(argv[i + 1])
        elif flag == "--reps":
            reps = int(argv[i + 1])
        else:
            rough_n = int(argv[i + 1])
        del argv[i:i + 2]
args = [a for a in argv if not a.startswith("--")]
nx, ny = (int(args[0]), int(args[1])) if len(args) >= 2 else (3200, 3125)
S = 16
prm = dict(expand_dist=0.6, robot_size=0.3, sample_num=S, height_threshold=0.16, collision_threshold=0.1,
           update_collision_threshold=0.5, safety_factor=3.0, goal_tolerance=0.8)
WARM = 2


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def rec(r, wall, V):
    info = r["info"]
    d = {"ms_device": info.ms_device, "ms_wall": wall, "rounds": info.rounds, "host_syncs": info.host_syncs}
    if "carried" in r:
        d["carried_over_V"] = float(r["carried"].mean()) / V
    return d


def summary(recs):
    s = {}
    for key in recs[0]:
        vals = np.array([r[key] for r in recs], np.float64)
        s[key + "_median"] = float(np.median(vals))
        s[key + "_min"] = float(vals.min())
        s[key + "_max"] = float(vals.max())
    return s


def measure(workload, cloud, centre, start):
    cx, cy = centre
    e = trg_planner.Engine(**prm)
    e.set_sampler(7, 16)
    e.set_global_map(cloud)
    e.init_graph([cx, cy, 0.0])
    V0, E0 = e.graph_sizes("global")
    first = e.risk_fields(sources_xy=[start])
    reachable = np.flatnonzero(first["hops"][0] >= 0)
    levels = int(np.unique(first["risk"][0][reachable]).size)
    # the sources as positions: a node keeps its position through the updates, its id not
    xy = e.node_xyz("global")[:, :2]
    spread = reachable[np.linspace(0, reachable.size - 1, 8).astype(np.int64)]
    spread[0] = first["sources"][0]
    sources = {1: xy[spread[:1]].copy(), 8: xy[spread].copy()}
    pose0 = xy[spread[0]].copy()
    del first, xy

    def update(k):
        pose = (cx - 10.0 + 0.5 * k, cy - 6.0 + 0.2 * k)
        m = (np.abs(cloud[:, 0] - pose[0]) < 10.0) & (np.abs(cloud[:, 1] - pose[1]) < 10.0)
        obs = cloud[m].copy()
        b = (np.abs(obs[:, 0] - pose[0] - 3.0) < 0.6) & (np.abs(obs[:, 1] - pose[1] - 1.0) < 0.6)
        obs[b, 2] += np.float32(1.0) * (np.arange(b.sum()) % 2).astype(np.float32)
        e.set_local_map(pose, obs)
        _, ms = timed(e.update_graph)
        return ms

    samples = {m: {"refresh": [], "fresh": []} for m in sources}
    frontier = {"reuse": [], "fresh": []}
    update_ms, reuse_hits, n_frontier = [], 0, 0
    step = 0
    for rep in range(WARM + reps):
        for m, src_xy in sources.items():
            e.risk_fields(sources_xy=src_xy, full=False)  # the solve the update makes stale
            update_ms.append(update(step))
            step += 1
            V, _ = e.graph_sizes("global")
            r, wall_r = timed(lambda: e.refresh_risk_fields(full=False))
            f, wall_f = timed(lambda: e.risk_fields(source_ids=r["sources"], full=False))
            assert np.array_equal(r["reached"], f["reached"]), (r["reached"], f["reached"])
            if rep >= WARM:
                samples[m]["refresh"].append(rec(r, wall_r, V))
                samples[m]["fresh"].append(rec(f, wall_f, V))
        # the frontier helper from the same pose across an update
        n_frontier = int(e.frontier_ceilings(pose0)[0].size)
        update_ms.append(update(step))
        step += 1
        V, _ = e.graph_sizes("global")
        a, wall_a = timed(lambda: e.safest_frontier(pose0, reuse=True))
        hit = e.last_reuse
        b, wall_b = timed(lambda: e.safest_frontier(pose0, reuse=False))
        assert a == b, (a, b)
        if rep >= WARM:
            reuse_hits += hit is not None
            d = {"ms_wall": wall_a}
            if hit is not None:
                d.update(ms_device_refresh=hit["info"].ms_device, rounds=hit["info"].rounds,
                         carried_over_V=float(hit["carried"][0]) / V)
            frontier["reuse"].append(d)
            frontier["fresh"].append({"ms_wall": wall_b})
        print(workload, "rep", rep, flush=True)
    V1, E1 = e.graph_sizes("global")
    e.close()
    res = {"workload": workload, "V_first": V0, "E_first": E0, "V_last": V1, "E_last": E1,
           "distinct_risks_of_the_first_field": levels, "reached_of_the_first_field": int(reachable.size),
           "update_graph_ms_median": float(np.median(update_ms)),
           "fields": {str(m): {kind: summary(r) for kind, r in s.items()} for m, s in samples.items()}}
    res["refresh_over_fresh"] = {
        str(m): {key: res["fields"][str(m)]["refresh"][key + "_median"] /
                 res["fields"][str(m)]["fresh"][key + "_median"] for key in ("ms_device", "ms_wall")} for m in sources}
    keys = set.intersection(*(set(d) for d in frontier["reuse"]))
    res["safest_frontier"] = {"frontier_nodes": n_frontier, "refresh_taken": reuse_hits, "of": reps,
                              "reuse": summary([{k: d[k] for k in sorted(keys)} for d in frontier["reuse"]]),
                              "fresh": summary(frontier["fresh"])}
    res["safest_frontier"]["reuse_over_fresh_wall"] = (res["safest_frontier"]["reuse"]["ms_wall_median"] /
                                                       res["safest_frontier"]["fresh"]["ms_wall_median"])
    return res


res = {"reps": reps, "field_delta_scale": 4, "S": S}
cloud = synth.mountain_tile(0, nx, 0, ny, seed=20250418)
cx, cy = nx * 0.05, ny * 0.05
scale = 6.0 * min(nx, ny) / 3125.0
start = (np.array([-7.22, -7.54], np.float32) * scale + np.array([cx, cy], np.float32)).astype(np.float32)
res["c3"] = measure(f"C3-style {nx}x{ny} = {int(cloud.shape[0])} points", cloud, (cx, cy), start)
cloud = synth.mountain_cloud(rough_n, rough_n, seed=11, amplitude=5.0, wavelength=14.0)
c = rough_n * 0.05
start = (np.array([-7.22, -7.54], np.float32) * (c / 25.0) + np.array([c, c], np.float32)).astype(np.float32)
res["rough"] = measure(f"rough terrain (seed 11, amplitude 5 m, wavelength 14 m) {rough_n}x{rough_n} = "
                       f"{int(cloud.shape[0])} points", cloud, (c, c), start)
del cloud
res["note"] = ("ms_device = hipEvent time of the call; ms_wall = host clock around it, the upload of the updated "
               "graph's CSR included in whichever call comes first after the update -- the refresh, or safest_frontier "
               "with reuse=True; the fresh call that follows finds it uploaded and its edge risks computed.  "
               "carried_over_V: nodes whose old key was kept, per field, over the node count.  safest_frontier: the "
               "whole call (Frontier ids, the field read at them, one routes call); refresh_taken counts the updates "
               "after which reuse=True took the refresh.")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
