#!/usr/bin/env python3
"""Run on the GPU box: what the routes of a tiled solve cost when the devices walk them (Engine.tiled_routes,
trg_engine_tiled_field_routes) on the bench cloud cut 2 x 2 as scripts/tiled_sets_latency.py cuts it -- FOUR engines on
ONE card over the in-process transport, one thread per rank -- for 1, 8 and 64 targets spread over the tiles, after one
single-source solve.  Next to it the only way there was before: every rank downloads its m x V_t parents (the solve
with parent=True against the one without), tiled.concat_fields, tiled.field_route per target, and a host fold over the
exported rows for the length and the mean risk.

Reported per case (medians of --reps after a warm-up): the wall time of the collective routes call (the slowest rank;
the capacity is known, one call), exchanges and records; for the old way the wall time of concatenation, walks and
folds, and once the extra wall time of the solve that downloads parents and of the export of the rows; and whether
both agree in ids and in the length and risk bits (they must).  Four ranks share one GPU here: the numbers say what the
exchanges cost in host round trips on one shared card, not what four GPUs would give.

usage: python scripts/tiled_routes_latency.py [--out PATH] [--reps N] [--workload c3|c2|small]
       -> PATH (default profiles/r26_tiled_routes.json)
"""
import json
import time

import numpy as np

from tiled_cut import R, Cut, bench, tiled  # (first: it sets the paths and loads torch before the engine)

F32 = np.float32
cut = Cut("routes", "r26_tiled_routes.json", reps=9)
engines, ranks, reps = cut.engines, cut.ranks, cut.reps
(nb_nc, ms_stitch) = cut.stitch()
t0 = time.perf_counter()
G = tiled.concat_stitched([e.graph("stitched") for e in engines])  # the old way's rows, for the host fold
ms_export = 1e3 * (time.perf_counter() - t0)
off = G["offsets"]
cut.stitch()  # (rows in HBM again)
rng = np.random.default_rng(26)
ok = [int(off[t]) + np.flatnonzero((G["state"][off[t]:off[t + 1]] != -1) & (np.diff(G["rowptr"])[off[t]:off[t + 1]] > 0))
      for t in range(R)]
source = int(ok[0][len(ok[0]) // 2])
sf = float(bench.MOUNTAIN["safety_factor"])
with np.errstate(over="ignore", invalid="ignore"):
    ec = ((F32(sf) * G["w"].astype(F32) + F32(1.0)) * G["dist"].astype(F32)).astype(F32)


def host_route(f, target):
    """the old way for one target: the host walk, then the fold from the target end over the least tight edges"""
    ids = tiled.field_route(f, 0, target)
    cost = f["cost"][0]
    pl, risk = F32(0.0), F32(0.0)
    for i in range(len(ids) - 1, 0, -1):
        u, v = ids[i - 1], ids[i]
        k0, k1 = int(G["rowptr"][u]), int(G["rowptr"][u + 1])
        hit = np.flatnonzero((G["col"][k0:k1] == v) & (G["state"][v] != -1) &
                             ((cost[u] + ec[k0:k1]).astype(F32).view(np.uint32) == cost[v:v + 1].view(np.uint32)))
        k = k0 + int(hit[0])
        pl, risk = F32(pl + G["dist"][k]), F32(risk + G["w"][k])
    return ids, pl, F32(risk / F32(len(ids))) if ids else F32(0.0)


# the solves: what downloading parents adds (the old way needs them on the host, the new way leaves them in HBM)
solve_ms = {True: [], False: []}
for rep in range(reps + 2):
    for parent in (True, False):
        got, wall = ranks(lambda r, e: e.tiled_cost_fields([source], parent=parent))
        if rep >= 2:
            solve_ms[parent].append(wall)
with_parents, _ = ranks(lambda r, e: e.tiled_cost_fields([source], parent=True))
hops = np.concatenate([g["hops"][0] for g in with_parents])

cases = {}
for n in (1, 8, 64):
    per = max(1, n // R)
    reached = [o[hops[o] > 0] for o in ok]
    targets = np.concatenate([rng.choice(reached[(R - 1 - t) % R], per, replace=False) for t in range(R)])[:n].astype(np.int32)
    cap = int((hops[targets] + 1).sum())
    fields = np.zeros(n, np.int32)
    new_ms, old_ms = [], []
    for rep in range(reps + 2):
        parts, wall = ranks(lambda r, e: e.tiled_routes(fields, targets, cap=cap))
        t0 = time.perf_counter()
        f = tiled.concat_fields(with_parents)
        old = [host_route(f, int(t)) for t in targets]
        ms_old = 1e3 * (time.perf_counter() - t0)
        if rep >= 2:
            new_ms.append(wall)
            old_ms.append(ms_old)
    joined = tiled.join_routes(parts)
    same = all(ids.tolist() == o[0] and np.float32(i.path_length).tobytes() == o[1].tobytes() and
               np.float32(i.avg_risk).tobytes() == o[2].tobytes() for (ids, _, i), o in zip(joined, old))
    infos = [p["info"] for p in parts]
    cases[f"targets_{n}"] = {
        "targets": int(n), "nodes_in_all": cap, "longest_route": int(infos[0].max_nodes),
        "tiled_routes": {"ms_wall_median": float(np.median(new_ms)), "ms_wall_min": float(np.min(new_ms)),
                         "ms_wall_max": float(np.max(new_ms)), "exchanges": int(infos[0].exchanges),
                         "ms_device_per_rank": [float(i.ms_device) for i in infos],
                         "records_per_rank": [int(i.records_sent) for i in infos]},
        "host_walk_and_fold": {"ms_median": float(np.median(old_ms)), "ms_min": float(np.min(old_ms)),
                               "ms_max": float(np.max(old_ms))},
        "routes_equal_bit_for_bit": bool(same),
    }
    print(f"targets_{n}", json.dumps(cases[f"targets_{n}"]), flush=True)

res = {
    **cut.header(),
    "nodes_per_rank": [int(off[t + 1] - off[t]) for t in range(R)], "parents_per_field": int(off[-1]),
    "ms_stitch_exchange": ms_stitch, "ms_export_of_the_rows_for_the_host_fold": ms_export, "reps": reps,
    "ms_solve_with_parent_download_median": float(np.median(solve_ms[True])),
    "ms_solve_without_median": float(np.median(solve_ms[False])),
    "cases": cases,
    "note": ("tiled_routes: host clock around the collective call on all four threads (the slowest rank), capacity known "
             "(one call), downloads of this rank's ids, positions and all infos included.  The old way also needs, once per "
             "solve, the parents on the host (the difference of the two solve medians) and, for length and risk, the "
             "exported rows.  The four ranks' kernels and copies share one GPU and one host here: this says what the "
             "exchanges cost on one shared card, not what four GPUs would give.  Over RCCL with more than one rank it "
             "has not run."),
}
cut.finish(res)
