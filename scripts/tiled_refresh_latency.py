#!/usr/bin/env python3
"""Run on the GPU box: what bringing a retained tiled solve through an update of one tile and a new stitch costs
(Engine.tiled_refresh_fields / tiled_refresh_risk_fields; DESIGN.md section 7, "Refresh across tiles") next to solving
it again, on the bench cloud cut 2 x 2 as `bench.py --gpus 4 --scaling strong` cuts it -- FOUR engines on ONE card over
the in-process transport, one thread per rank -- under the update stream of scripts/cost_field_refresh_latency.py
(20 m x 20 m local maps around a pose that moves 0.5 m per step, with an injected obstacle), applied to the tile the
pose is in.

One process.  Per shape (cost and risk, 1 field and 8): a tiled solve; then per repetition set_local_map + update_graph
on the pose's tile, the stitch exchange on all ranks, the refresh through the engines' own node maps, and a fresh tiled
solve from the refresh's set_gids on the same stitch -- the yardstick, equal to the refresh in value bits and hops every
time, and what the next repetition's refresh starts from; both download m x V values and hops.  The sources lie in the
three other tiles: the goal stays put while the map changes around the pose.  Medians with min - max over --reps after
a warm-up repetition of: the wall time of the collective call (the slowest rank), the device time per rank, the
exchanges of each kind, rounds per rank and carried / V.  Four ranks share one GPU here: the numbers say what the
exchanges cost on one shared card, not what four GPUs would give.  Over RCCL with more than one rank this has not run.

Every rank's step of a collective call runs in its own thread under a time limit (--limit seconds, default 120): one
that does not return ends the process at once, so that nothing more is started on the GPU.

usage: python scripts/tiled_refresh_latency.py [--out PATH] [--reps N] [--workload c3|c2|small] [--limit S]
       -> PATH (default profiles/r32_tiled_refresh.json)
"""
import os
import threading
import time

import numpy as np

from tiled_cut import COLS, ROWS, SEED, Cut, R, bench, option, tiled  # (first: it sets the paths and loads torch)

LIMIT = float(option("--limit", 120))
cut = Cut("refresh", "r32_tiled_refresh.json", reps=7)
engines, reps = cut.engines, cut.reps
WARM = 1
POSE_TILE = 0


def ranks(call):
    """call(rank, engine) on every rank, one thread each, under the time limit -> (results, wall ms)"""
    res, err = [None] * R, [None] * R

    def run(r):
        try:
            res[r] = call(r, engines[r])
        except Exception as ex:  # noqa: BLE001
            err[r] = ex

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(R)]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    for x in th:
        x.join(max(0.0, LIMIT - (time.perf_counter() - t0)))
    wall = 1e3 * (time.perf_counter() - t0)
    late = [r for r, x in enumerate(th) if x.is_alive()]
    if late:
        print(f"ranks {late} did not return within {LIMIT} s: ending the run", flush=True)
        os._exit(124)
    if any(err):
        raise RuntimeError([str(x) for x in err if x])
    return res, wall


def stitch():
    return ranks(lambda r, e: e.stitch_exchange(cut.cores[r], COLS, ROWS))


# the pose's tile keeps its cloud: the local maps are crops of it
core, win = tiled.split_tile(POSE_TILE, COLS, ROWS, cut.nx, cut.ny, 11)
cloud = bench.terrain_tile(*win, seed=SEED)
px, py = 0.5 * float(core[0] + core[2]), 0.5 * float(core[1] + core[3])
steps = [0]


def update():
    """one step of the update stream on the pose's tile -> ms of update_graph"""
    k = steps[0]
    steps[0] += 1
    pose = (px - 10.0 + 0.5 * k, py - 6.0 + 0.2 * k)
    m = (np.abs(cloud[:, 0] - pose[0]) < 10.0) & (np.abs(cloud[:, 1] - pose[1]) < 10.0)
    obs = cloud[m].copy()
    b = (np.abs(obs[:, 0] - pose[0] - 3.0) < 0.6) & (np.abs(obs[:, 1] - pose[1] - 1.0) < 0.6)
    obs[b, 2] += np.float32(1.0) * (np.arange(b.sum()) % 2).astype(np.float32)
    engines[POSE_TILE].set_local_map(pose, obs)
    t0 = time.perf_counter()
    engines[POSE_TILE].update_graph()
    return 1e3 * (time.perf_counter() - t0)


(nb_nc, ms_stitch) = stitch()
sizes, off = cut.sizes()
centres = cut.centres(off)
# the sources: reached nodes of the three other tiles -- the centres, then nodes spread over their id ranges
first, _ = ranks(lambda r, e: e.tiled_cost_fields([centres[3]], parent=False))
hops = tiled.concat_fields(first)["hops"][0]
others = np.flatnonzero((hops >= 0) & (np.arange(hops.shape[0]) >= off[1]))
spread = others[np.linspace(0, others.size - 1, 7).astype(np.int64)[1:-1]].tolist()
SOURCES = {1: [centres[3]], 8: [centres[3], centres[1], centres[2]] + [int(s) for s in spread]}
assert all(len(set(s)) == len(s) for s in SOURCES.values())
del first, hops


def record(got, wall, V):
    infos = [g["info"] for g in got]
    rec = {"ms_wall": wall, "ms_device_per_rank": [float(i.ms_device) for i in infos], "exchanges": int(infos[0].exchanges),
           "rounds_per_rank": [int(i.rounds) for i in infos], "records_per_rank": [int(i.records_sent) for i in infos]}
    if "carried" in got[0]:
        rec["anchor_exchanges"] = int(infos[0].anchor_exchanges)
        rec["owner_exchanges"] = int(infos[0].owner_exchanges)
        rec["anchor_records_per_rank"] = [int(i.anchor_records_sent) for i in infos]
        rec["carried_over_V"] = float(np.mean(np.sum([g["carried"] for g in got], 0))) / V
    return rec


def summary(recs):
    s = {}
    for key in recs[0]:
        vals = np.array([r[key] for r in recs], np.float64)
        s[key] = {"median": np.median(vals, axis=0).tolist(), "min": vals.min(axis=0).tolist(), "max": vals.max(axis=0).tolist()}
    return s


samples, update_ms, stitch_ms = {}, [], []
for risk in (False, True):
    for m, sources in SOURCES.items():
        shape = f"{'risk' if risk else 'cost'}_{m}"
        samples[shape] = {"refresh": [], "fresh": []}
        solve = (lambda r, e, s: e.tiled_risk_fields(s, parent=False)) if risk else (lambda r, e, s: e.tiled_cost_fields(s, parent=False))
        ranks(lambda r, e: solve(r, e, sources))  # the solve the first update makes stale
        for rep in range(WARM + reps):
            update_ms.append(update())
            stitch_ms.append(stitch()[1])
            V = int(cut.sizes()[1][-1])
            name = "risk" if risk else "cost"
            got, wall_r = ranks(lambda r, e: (e.tiled_refresh_risk_fields if risk else e.tiled_refresh_fields)(parent=False))
            sources = [int(s[0]) for s in got[0]["set_gids"]]
            fresh, wall_f = ranks(lambda r, e: solve(r, e, sources))
            for g, f in zip(got, fresh):  # bit for bit, every repetition
                assert np.array_equal(g[name].view(np.uint32), f[name].view(np.uint32)) and np.array_equal(g["hops"], f["hops"])
            if rep >= WARM:
                samples[shape]["refresh"].append(record(got, wall_r, V))
                samples[shape]["fresh"].append(record(fresh, wall_f, V))
            print(shape, "rep", rep, f"refresh {wall_r:.1f} ms, fresh {wall_f:.1f} ms", flush=True)

sizes_end, off_end = cut.sizes()
res = {
    **cut.header(),
    "nodes_per_rank_first": [int(v) for v, _ in sizes], "nodes_per_rank_last": [int(v) for v, _ in sizes_end],
    "boundary_records_and_cross_edges": [int(x) for x in nb_nc[0]], "ms_stitch_exchange_first": ms_stitch,
    "ms_restitch_median": float(np.median(stitch_ms)), "ms_update_graph_median": float(np.median(update_ms)),
    "updates": steps[0], "pose_tile": POSE_TILE, "sources_first": {str(m): s for m, s in SOURCES.items()}, "reps": reps,
    "shapes": {k: {kind: summary(v) for kind, v in by.items()} for k, by in samples.items()},
}
res["refresh_over_fresh"] = {
    k: {"ms_wall": by["refresh"]["ms_wall"]["median"] / by["fresh"]["ms_wall"]["median"],
        "ms_device_slowest_rank": max(by["refresh"]["ms_device_per_rank"]["median"]) / max(by["fresh"]["ms_device_per_rank"]["median"]),
        "exchanges_all_kinds": (by["refresh"]["exchanges"]["median"] + by["refresh"]["anchor_exchanges"]["median"] +
                                by["refresh"]["owner_exchanges"]["median"]) / by["fresh"]["exchanges"]["median"]}
    for k, by in res["shapes"].items()}
res["note"] = ("ms_wall = host clock around the collective call on all four threads (the slowest rank); the refresh is the "
               "first call after the stitch, so its wall time carries the new solve graph and its edge values, which the "
               "fresh solve after it finds built.  ms_device = hipEvent time of a rank's own kernels between its exchanges.  "
               "Refresh and fresh solve alternate within every repetition in one process.  The four ranks' kernels and "
               "copies share one GPU and one host here, so the wall time says what the exchanges cost on one shared card, "
               "not what four GPUs would give; over RCCL with more than one rank this has not run.")
cut.finish(res)
