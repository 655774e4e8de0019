#!/usr/bin/env python3
"""Run on the GPU box: what a cost field across tiles (Engine.tiled_cost_fields, trg_engine_tiled_cost_field) costs
on the bench cloud cut 2 x 2 as `bench.py --gpus 4 --scaling strong` cuts it -- FOUR engines on ONE card over the
in-process transport, one thread per rank -- next to the only alternative there was before it: exporting the four
tiles' stitched rows to one host, concatenating them and running the compiled host Dijkstra
(tests/cpp/field_reference.cpp) there.

Reported per solve (medians of --reps after a warm-up): the wall time of the collective call (the slowest rank), the
device time per rank, exchanges, rounds and records sent per rank; the first call, which builds the solve graphs; the
host alternative's export + concatenation (once per stitch) and Dijkstra (per field); and whether both agree in cost
bits, hops and parents.  Four ranks share one GPU here: the numbers say how many exchanges a field needs and what an
exchange costs in host round trips, not what four GPUs would give.

usage: python scripts/tiled_field_latency.py [--out PATH] [--reps N] [--workload c3|c2|small]
       -> PATH (default profiles/r23_tiled_field.json)
"""
import json
import os
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "trg-planner_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first, as in tests/conftest.py: one HIP runtime for torch and the engine)
import trg_planner  # noqa: E402
from trg_planner import tiled  # noqa: E402
import bench  # noqa: E402  (terrain_tile, WORKLOADS, MOUNTAIN: the benchmark's own cloud and parameters)
import field_ref  # noqa: E402  (tests/: the compiled host Dijkstra)

argv = sys.argv[1:]


def option(name, default):
    if name in argv:
        i = argv.index(name)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return default


out = os.path.abspath(option("--out", os.path.join(ROOT, "profiles", "r23_tiled_field.json")))
reps = int(option("--reps", 15))
workload = option("--workload", "c3")
nx, ny, S, label = bench.WORKLOADS[workload]
COLS = ROWS = 2
R = COLS * ROWS
SEED = 20250418

engines, cores = [], []
n_points = 0
for t in range(R):
    core, win = tiled.split_tile(t, COLS, ROWS, nx, ny, 11)
    cloud = bench.terrain_tile(*win, seed=SEED)
    n_points += int(cloud.shape[0])
    e = trg_planner.Engine(**dict(bench.MOUNTAIN, sample_num=S))
    e.set_sampler(7, 16)
    e.set_tile(core, epoch=t)
    e.set_global_map(cloud)
    e.init_graph([0.5 * float(core[0] + core[2]), 0.5 * float(core[1] + core[3]), 0.0])
    engines.append(e)
    cores.append(core)
    del cloud
for t, e in enumerate(engines):
    e.comm_join_local(f"tiled-field-latency-{os.getpid()}", R, t)


def ranks(call):
    """call(rank, engine) on every rank, one thread each -> (results, wall ms of the slowest)"""
    res, err = [None] * R, [None] * R

    def run(r):
        try:
            res[r] = call(r, engines[r])
        except Exception as ex:  # noqa: BLE001
            err[r] = ex

    th = [threading.Thread(target=run, args=(r,)) for r in range(R)]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    for x in th:
        x.join()
    wall = 1e3 * (time.perf_counter() - t0)
    if any(err):
        raise RuntimeError([str(x) for x in err if x])
    return res, wall


(nb_nc, ms_stitch) = ranks(lambda r, e: e.stitch_exchange(cores[r], COLS, ROWS))
sizes = [e.graph_sizes("stitched") for e in engines]
off = np.concatenate([[0], np.cumsum([v for v, _ in sizes])]).astype(np.int64)

# sources: the node nearest the centre of each tile's core (global ids); field 0 alone is the m = 1 case
sources = []
for t, e in enumerate(engines):
    xyz = e.node_xyz("global")
    c = np.array([0.5 * (cores[t][0] + cores[t][2]), 0.5 * (cores[t][1] + cores[t][3])], np.float32)
    sources.append(int(off[t]) + int(np.argmin(((xyz[:, :2] - c) ** 2).sum(1))))


def record(got, wall):
    infos = [g["info"] for g in got]
    return {"ms_wall": wall, "ms_device_per_rank": [float(i.ms_device) for i in infos],
            "ms_total_per_rank": [float(i.ms_total) for i in infos], "exchanges": int(infos[0].exchanges),
            "rounds_per_rank": [int(i.rounds) for i in infos], "records_per_rank": [int(i.records_sent) for i in infos]}


def solve(src):
    got, wall = ranks(lambda r, e: e.tiled_cost_fields(src))
    return got, record(got, wall)


first_got, first = solve(sources[:1])  # builds every rank's solve graph from the rows in HBM
shapes = {"m1": sources[:1], "m4": sources}
for src in shapes.values():
    solve(src)
    solve(src)
samples = {k: [] for k in shapes}
last = {}
for rep in range(reps):
    for k, src in shapes.items():
        last[k], rec = solve(src)
        samples[k].append(rec)
    print("rep", rep, flush=True)

# the alternative: the rows to one host, one CSR, the compiled Dijkstra
t0 = time.perf_counter()
G = tiled.concat_stitched([e.graph("stitched") for e in engines])
ms_export = 1e3 * (time.perf_counter() - t0)
lib = field_ref.compile_reference(tempfile.mkdtemp())
sf = bench.MOUNTAIN["safety_factor"]
host_ms, host = [], None
for rep in range(reps):
    t0 = time.perf_counter()
    host = field_ref.field(lib, G["rowptr"], G["col"], G["w"], G["dist"], G["state"], sf, sources[0])
    host_ms.append(1e3 * (time.perf_counter() - t0))
assert host[0] == 0
f = tiled.concat_fields(last["m1"])
exact = bool(np.array_equal(f["cost"][0].view(np.uint32), host[1].view(np.uint32)) and
             np.array_equal(f["hops"][0], host[2]) and np.array_equal(f["parent"][0], host[3]))


def summary(recs):
    s = {"exchanges": recs[-1]["exchanges"], "rounds_per_rank": recs[-1]["rounds_per_rank"],
         "records_per_rank": recs[-1]["records_per_rank"],
         "ms_wall_median": float(np.median([r["ms_wall"] for r in recs])),
         "ms_wall_min": float(np.min([r["ms_wall"] for r in recs])),
         "ms_wall_max": float(np.max([r["ms_wall"] for r in recs]))}
    for key in ("ms_device_per_rank", "ms_total_per_rank"):
        s[key + "_median"] = np.median(np.array([r[key] for r in recs]), axis=0).tolist()
    s["ms_wall_per_exchange"] = s["ms_wall_median"] / max(1, s["exchanges"])
    return s


info0 = [g["info"] for g in first_got]
res = {
    "workload": f"{label}: {nx}x{ny} lattice cut {COLS}x{ROWS} (split_tile, 1.1 m halo), {n_points} points in all",
    "ranks": R, "transport": "in-process (trg_engine_comm_join_local): FOUR RANKS SHARE ONE GPU",
    "nodes_per_rank": [int(v) for v, _ in sizes], "edges_per_rank": [int(n) for _, n in sizes],
    "ghosts_per_rank": [int(i.ghosts) for i in info0], "border_nodes_per_rank": [int(i.border_nodes) for i in info0],
    "boundary_records_and_cross_edges": [int(x) for x in nb_nc[0]], "ms_stitch_exchange": ms_stitch,
    "sources": sources, "reps": reps,
    "first_call_m1_with_solve_graph_build": first,
    "solve_m1": summary(samples["m1"]), "solve_m4": summary(samples["m4"]),
    "host_alternative": {"ms_export_and_concat_once_per_stitch": ms_export,
                         "ms_dijkstra_per_field_median": float(np.median(host_ms)),
                         "ms_dijkstra_per_field_min": float(np.min(host_ms)), "V": int(G["V"]),
                         "E": int(G["col"].shape[0])},
    "device_equals_host_dijkstra": exact,
    "note": ("ms_wall = host clock around the collective call on all four threads (the slowest rank), downloads of "
             "cost, hops and parent included; ms_device = hipEvent time of a rank's own kernels between its "
             "exchanges.  The four ranks' kernels and copies share one GPU and one host here, so the wall time is "
             "an upper bound of what an exchange costs in host round trips, not a multi-GPU figure."),
}
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
for e in engines:
    e.close()
