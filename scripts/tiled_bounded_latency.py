#!/usr/bin/env python3
"""Run on the GPU box: what a bound saves a field across tiles (Engine.tiled_cost_fields_bounded,
tiled_plan_many_early_exit; DESIGN.md section 7, "Bounded fields across tiles") on the bench cloud cut 2 x 2 as
`bench.py --gpus 4 --scaling strong` cuts it -- FOUR engines on ONE card over the in-process transport, one thread per
rank.  Every figure stands next to the unbounded tiled solve of the same source in the same process, the two
alternating within every repetition: there is no other baseline, the parent commit cannot run a bounded tiled solve.

Shapes: budgets that 1 % / 10 % / 50 % of the global graph's nodes lie within (quantiles of the full field's costs), each
for a source deep inside a tile and for one on a seam (a node with a cross edge); and tiled_plan_many to 8 goals within
20 m of the start, with and without the early exit.  Reported per shape (medians and minima of --reps after a warm-up):
the wall time of the collective call (the slowest rank), the device time per rank, exchanges, rounds, records per rank,
and for the budgets the nodes reached per rank.  Four ranks share one GPU here: the numbers say how many exchanges a
bound saves and what an exchange costs in host round trips, not what four GPUs would give.  Over RCCL with more than
one rank this has not run.

usage: python scripts/tiled_bounded_latency.py [--out PATH] [--reps N] [--workload c3|c2|small]
       -> PATH (default profiles/r30_tiled_bounded.json)
"""
import numpy as np

from tiled_cut import Cut, summary, tiled  # (first: it sets the paths and loads torch before the engine)

cut = Cut("bounded", "r30_tiled_bounded.json", reps=15)
engines, ranks, reps = cut.engines, cut.ranks, cut.reps
(nb_nc, ms_stitch) = cut.stitch()
sizes, off = cut.sizes()
deep = cut.centres(off)[0]
# a node of tile 0 with a cross edge, from its stitched rows (the export takes them off the device: stitch again)
rows = engines[0].graph("stitched")
src_of = np.repeat(np.arange(rows.V), np.diff(rows.rowptr))
cross = (rows.col < off[0]) | (rows.col >= off[1])
seam = int(off[0]) + int(src_of[cross][cross.sum() // 2])
cut.stitch()
xyz = np.concatenate([e.node_xyz("global") for e in engines], 0)


def record(infos, wall, got=None, routes=None):
    rec = {"ms_wall": wall, "ms_device_per_rank": [float(i.ms_device) for i in infos],
           "exchanges": int(infos[0].exchanges), "rounds_per_rank": [int(i.rounds) for i in infos],
           "records_per_rank": [int(i.records_sent) for i in infos]}
    if got is not None and "reached" in got[0]:
        rec["reached_per_rank"] = [int(g["reached"][0]) for g in got]
    if routes is not None:
        rec["routes_exchanges"] = int(routes[0].exchanges)
        rec["routes_ms_device_per_rank"] = [float(i.ms_device) for i in routes]
    return rec


def field(src, budget=None):
    got, wall = ranks(lambda r, e: e.tiled_cost_fields([src], parent=False) if budget is None else
                      e.tiled_cost_fields_bounded([src], budget=budget, parent=False))
    return got, record([g["info"] for g in got], wall, got)


def plan(start, goals, early):
    def both(e):  # tiled_plan_many's (tiled_plan_many_early_exit's) two calls, both infos kept
        s = e.tiled_cost_fields_bounded([start], settle="all", settle_gids=goals, parent=False) if early else \
            e.tiled_cost_fields([start], parent=False)
        return dict(e.tiled_routes(np.zeros(len(goals), np.int32), goals), solve_info=s["info"])
    got, wall = ranks(lambda r, e: both(e))
    return got, record([g["solve_info"] for g in got], wall, routes=[g["info"] for g in got])


# the budgets: quantiles of the full field's costs over ALL nodes of the global graph
fractions = (0.01, 0.10, 0.50)
budgets, first, reach = {}, {}, {}
for name, src in (("deep", deep), ("seam", seam)):
    got, first[name] = field(src)
    f = tiled.concat_fields(got)
    reach[name] = f["hops"][0] >= 0
    c = np.sort(f["cost"][0][reach[name]])
    budgets[name] = [float(c[min(c.size - 1, int(frac * xyz.shape[0]))]) for frac in fractions]
# 8 goals within 20 m of the deep start, spread over the distances
d = np.linalg.norm(xyz[:, :2] - xyz[deep, :2], axis=1)
near = np.flatnonzero((d <= 20.0) & reach["deep"] & (np.arange(xyz.shape[0]) != deep))
near = near[np.argsort(d[near])]
goals = [int(g) for g in near[np.linspace(near.size // 8, near.size - 1, 8).astype(int)]]

shapes = {}
for name, src in (("deep", deep), ("seam", seam)):
    for frac, b in zip(fractions, budgets[name]):
        shapes[f"{name}_budget_{int(100 * frac)}pct"] = (lambda src=src, b=b: field(src, b), lambda src=src: field(src))
shapes["plan_many_8_goals_20m"] = (lambda: plan(deep, goals, True), lambda: plan(deep, goals, False))
for bounded, full in shapes.values():  # warm-up
    for fn in (bounded, full, bounded, full):
        fn()
samples = {k: {"bounded": [], "unbounded": []} for k in shapes}
last = {}
for rep in range(reps):
    for k, (bounded, full) in shapes.items():
        for name, fn in (("bounded", bounded), ("unbounded", full)):
            got, rec = fn()
            samples[k][name].append(rec)
            last[k, name] = got
    print("rep", rep, flush=True)

key = lambda joined: [(ids.tolist(), i.num_nodes, np.float32(i.cost).tobytes(), np.float32(i.path_length).tobytes(),  # noqa: E731
                       np.float32(i.avg_risk).tobytes()) for ids, _, i in joined]
same_routes = key(tiled.join_routes(last["plan_many_8_goals_20m", "bounded"])) == \
    key(tiled.join_routes(last["plan_many_8_goals_20m", "unbounded"]))
res = {
    **cut.header(),
    "nodes_per_rank": [int(v) for v, _ in sizes], "edges_per_rank": [int(n) for _, n in sizes],
    "boundary_records_and_cross_edges": [int(x) for x in nb_nc[0]], "ms_stitch_exchange": ms_stitch,
    "sources": {"deep": deep, "seam": seam}, "budgets": {k: dict(zip(("1pct", "10pct", "50pct"), v)) for k, v in budgets.items()},
    "goals": goals, "goal_distances_m": [float(d[g]) for g in goals], "reps": reps,
    "first_calls_unbounded": first,
    "shapes": {k: {name: summary(v, mins=True) for name, v in by.items()} for k, by in samples.items()},
    "early_exit_routes_equal_the_full_solve's": bool(same_routes),
    "note": ("ms_wall = host clock around the collective call(s) on all four threads (the slowest rank), downloads "
             "included; ms_device = hipEvent time of a rank's own kernels between its exchanges.  bounded and unbounded "
             "alternate within every repetition in one process.  The four ranks' kernels and copies share one GPU and "
             "one host here, so the wall time is an upper bound of what an exchange costs in host round trips, not a "
             "multi-GPU figure; over RCCL with more than one rank this has not run.  plan_many: the solve (without "
             "parents) and the two routes calls (lengths, then ids)."),
}
cut.finish(res)
