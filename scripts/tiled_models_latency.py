#!/usr/bin/env python3
"""Run on the GPU box: what a cost model per field costs a solve across tiles (Engine.tiled_cost_fields_models,
tiled_plan_tradeoff; DESIGN.md section 7, "Cost models across tiles") on the bench cloud cut 2 x 2 as
`bench.py --gpus 4 --scaling strong` cuts it -- FOUR engines on ONE card over the in-process transport, one thread per
rank.  Every figure stands next to the plain tiled solve in the same process, the two alternating within every
repetition: there is no other baseline, the parent commit cannot run a modelled tiled solve.

Shapes (medians and minima of --reps after a warm-up):
  (a) 8 fields from one source deep inside a tile under 8 DISTINCT models (the model table in the round kernels, the
      parent sweep and the owner pass; 8 slots of edge costs), beside 8 fields from it under the engine's one model
      (the plain instantiations on one slot) through the same entry;
  (b) tiled_plan_tradeoff of the 8 models to a goal within 20 m of the start -- one solve settled "any" at the goal,
      one routes call -- beside 8 tiled_plan_many_early_exit calls in sequence, which is what 8 risk attitudes cost
      without models (and answers under one model only);
  (c) the first modelled solve after a stitch (the new solve graph, then 8 cold slots: 8 edge-cost launches and one
      wait) beside the second, and beside the first solve after a stitch under the engine's model (the new solve graph
      and one cold slot).
Reported per shape: the wall time of the collective call (the slowest rank), the device time per rank, exchanges,
rounds and records per rank.  Four ranks share one GPU here: the numbers say what the exchanges and the model table
cost, not what four GPUs would give.  Over RCCL with more than one rank this has not run.

Every rank's step of a collective call runs in its own thread under a time limit (--limit seconds, default 120): one
that does not return ends the process at once, so that nothing more is started on the GPU.

usage: python scripts/tiled_models_latency.py [--out PATH] [--reps N] [--workload c3|c2|small] [--limit S]
       -> PATH (default profiles/r31_tiled_models.json)
"""
import os
import threading
import time

import numpy as np

from tiled_cut import Cut, R, option, summary, tiled  # (first: it sets the paths and loads torch before the engine)

LIMIT = float(option("--limit", 120))
cut = Cut("models", "r31_tiled_models.json", reps=10)
engines, reps = cut.engines, cut.reps


def ranks(call):
    """Cut.ranks under the time limit: call(rank, engine) on every rank, one thread each -> (results, wall ms)"""
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
    return ranks(lambda r, e: e.stitch_exchange(cut.cores[r], 2, 2))


(nb_nc, ms_stitch) = stitch()
sizes, off = cut.sizes()
deep = cut.centres(off)[0]
# the positive weights of the global graph, from the tiles' stitched rows (the export takes them off the device:
# stitch again)
w = np.concatenate([e.graph("stitched").w for e in engines])
w = w[w > 0]
stitch()
xyz = np.concatenate([e.node_xyz("global") for e in engines], 0)
SF = float(engines[0].params.safety_factor)
q50, q75 = (float(np.float32(np.quantile(w, q))) for q in (0.5, 0.75)) if w.size else (0.0, 0.0)
MODELS = [(SF, np.inf), (0.0, np.inf), (1.0, np.inf), (2.0 * SF, np.inf), (SF, q75), (SF, q50), (1.0, q50), (0.0, q75)]
assert len(set(MODELS)) == len(MODELS), "the weight quantiles coincide: the models are not distinct"
ONE = [None] * len(MODELS)
K = len(MODELS)


def record(infos, wall, routes=None):
    rec = {"ms_wall": wall, "ms_device_per_rank": [float(i.ms_device) for i in infos],
           "exchanges": int(infos[0].exchanges), "owner_exchanges": int(infos[0].owner_exchanges),
           "rounds_per_rank": [int(i.rounds) for i in infos], "records_per_rank": [int(i.records_sent) for i in infos]}
    if routes is not None:
        rec["routes_exchanges"] = int(routes[0].exchanges)
        rec["routes_ms_device_per_rank"] = [float(i.ms_device) for i in routes]
    return rec


def fields(models):
    got, wall = ranks(lambda r, e: e.tiled_cost_fields_models([deep] * K, models, full=False, parent=False))
    return got, record([g["info"] for g in got], wall)


def tradeoff(goal):
    def both(e):  # tiled_plan_tradeoff's two calls, both infos kept
        s = e.tiled_cost_fields_models([deep] * K, MODELS, settle="any", settle_gids=[goal], full=False, parent=False)
        return dict(e.tiled_routes(np.arange(K, dtype=np.int32), np.full(K, goal, np.int32)), solve_info=s["info"])
    got, wall = ranks(lambda r, e: both(e))
    return got, record([g["solve_info"] for g in got], wall, routes=[g["info"] for g in got])


def plans_in_sequence(goal):
    """K early-exit plans to the goal, one after the other: the last one's counters, the wall time of all"""
    def all_k(e):
        out = None
        for _ in range(K):
            s = e.tiled_cost_fields_bounded([deep], settle="all", settle_gids=[goal], parent=False)
            out = dict(e.tiled_routes(np.zeros(1, np.int32), [goal]), solve_info=s["info"])
        return out
    got, wall = ranks(lambda r, e: all_k(e))
    return got, record([g["solve_info"] for g in got], wall, routes=[g["info"] for g in got])


# a goal within 20 m of the deep start that every model reaches, the farthest such
first_models, first_rec = ranks(lambda r, e: e.tiled_cost_fields_models([deep] * K, MODELS, parent=False))
f = tiled.concat_fields(first_models)
d = np.linalg.norm(xyz[:, :2] - xyz[deep, :2], axis=1)
near = np.flatnonzero((d <= 20.0) & (f["hops"] >= 0).all(0) & (np.arange(xyz.shape[0]) != deep))
goal = int(near[np.argmax(d[near])])
reached = [int(n) for n in (f["hops"] >= 0).sum(1)]

shapes = {"fields_8": (lambda: fields(MODELS), lambda: fields(ONE)),
          "tradeoff_8_to_a_goal_within_20m": (lambda: tradeoff(goal), lambda: plans_in_sequence(goal))}
names = {"fields_8": ("8_distinct_models", "the_engines_model_8_times"),
         "tradeoff_8_to_a_goal_within_20m": ("plan_tradeoff_8_models", "8_early_exit_plans_in_sequence")}
for a, b in shapes.values():  # warm-up
    for fn in (a, b, a, b):
        fn()
samples = {k: {n: [] for n in names[k]} for k in shapes}
cold = {"first_after_a_stitch_8_cold_slots": [], "second": [], "first_after_a_stitch_the_engines_model": []}
ms_restitch = []
for rep in range(reps):
    for k, fns in shapes.items():
        for name, fn in zip(names[k], fns):
            samples[k][name].append(fn()[1])
    ms_restitch.append(stitch()[1])  # a new stitch: a new solve graph, an empty cache
    for name in ("first_after_a_stitch_8_cold_slots", "second"):
        cold[name].append(fields(MODELS)[1])
    ms_restitch.append(stitch()[1])  # ... and what the first solve after a stitch costs without models: the solve graph
    cold["first_after_a_stitch_the_engines_model"].append(fields(ONE)[1])
    print("rep", rep, flush=True)

res = {
    **cut.header(),
    "nodes_per_rank": [int(v) for v, _ in sizes], "edges_per_rank": [int(n) for _, n in sizes],
    "boundary_records_and_cross_edges": [int(x) for x in nb_nc[0]], "ms_stitch_exchange": ms_stitch,
    "ms_restitch_median": float(np.median(ms_restitch)),
    "source": deep, "goal": goal, "goal_distance_m": float(d[goal]),
    "models": [[float(s), float(t)] for s, t in MODELS], "positive_weight_quantiles": {"q50": q50, "q75": q75},
    "nodes_reached_per_model": reached, "reps": reps,
    "shapes": {k: {name: summary(v, mins=True) for name, v in by.items()} for k, by in samples.items()},
    "cold_slots": {name: summary(v, mins=True) for name, v in cold.items()},
    "note": ("ms_wall = host clock around the collective call(s) on all four threads (the slowest rank), downloads "
             "included; ms_device = hipEvent time of a rank's own kernels between its exchanges (the edge-cost "
             "launches of cold slots come before the first event and show in ms_wall only).  The variants of a shape "
             "alternate within every repetition in one process.  The baseline is the plain tiled solve of the same "
             "run.  The four ranks' kernels and copies share one GPU and one host here, so the wall time says what the "
             "exchanges cost in host round trips, not what four GPUs would give; over RCCL with more than one rank this "
             "has not run.  tradeoff: the solve (settle \"any\" at the goal, without parents) and the two routes calls "
             "(lengths, then ids); the 8 plans in sequence answer under the engine's one model only."),
}
cut.finish(res)
