#!/usr/bin/env python3
"""Run on the GPU box: what a source-set field across tiles (Engine.tiled_cost_fields_from,
trg_engine_tiled_cost_field_sets) costs on the bench cloud cut 2 x 2 as scripts/tiled_field_latency.py cuts it -- FOUR
engines on ONE card over the in-process transport, one thread per rank -- for the question "which of my members
reaches each node cheapest, at what cost": one set of 8 members spread over the tiles and one of 64, with and without
start costs.  Next to it the only way there was before: Engine.tiled_cost_fields with one field per member (8 fields in
one call, 64 in one call, start costs added on the host) and each rank's host argmin over its rows.

Reported per case (medians of --reps after a warm-up): the wall time of the collective call (the slowest rank),
exchanges, owner exchanges, records; for the old way the wall time of the solve and of the argmin; and whether both
agree in cost bits (they must) and in how many nodes the owners differ (the argmin cannot reproduce the owner rule at
ties).  Four ranks share one GPU here: the numbers say what the exchanges cost in host round trips on one shared card,
not what four GPUs would give.

usage: python scripts/tiled_sets_latency.py [--out PATH] [--reps N] [--workload c3|c2|small]
       -> PATH (default profiles/r24_tiled_sets.json)
"""
import json
import time

import numpy as np

from tiled_cut import Cut  # (first: it sets the paths and loads torch before the engine)

cut = Cut("sets", "r24_tiled_sets.json", reps=9)
engines, ranks, reps = cut.engines, cut.ranks, cut.reps
(nb_nc, ms_stitch) = cut.stitch()
sizes, off = cut.sizes()

# members: per tile, valid nodes spread over the core (global ids), taken tile after tile
rng = np.random.default_rng(24)
per_tile = []
for t, e in enumerate(engines):
    g = e.graph("global")
    ok = np.flatnonzero((g.state != -1) & (np.diff(g.rowptr) > 0))
    per_tile.append((int(off[t]) + rng.choice(ok, 16, replace=False)).astype(np.int32))
cut.stitch()  # (the exports took nothing of the stitch: rows in HBM again)
members = {8: np.concatenate([p[:2] for p in per_tile]), 64: np.concatenate(per_tile)}
starts = {k: rng.uniform(0.0, 5.0, k).astype(np.float32) for k in members}


def new_way(k, seeded):
    got, wall = ranks(lambda r, e: e.tiled_cost_fields_from([members[k]], [starts[k]] if seeded else None, parent=False))
    return got, wall


def old_way(k, seeded):
    """one field per member (at most 64 per call), then per rank the argmin over the members on the host"""
    got, wall = ranks(lambda r, e: e.tiled_cost_fields(members[k], parent=False))
    t0 = time.perf_counter()
    res = []
    for g in got:
        with np.errstate(over="ignore"):
            c = g["cost"] + starts[k][:, None] if seeded else g["cost"]
        o = np.argmin(c, 0).astype(np.int32)
        best = c[o, np.arange(c.shape[1])]
        res.append((best, np.where(np.isfinite(best), o, -1)))
    return got, res, wall, 1e3 * (time.perf_counter() - t0)


cases = {}
for k in (8, 64):
    for seeded in (False, True):
        name = f"set_of_{k}" + ("_with_start_costs" if seeded else "")
        for _ in range(2):
            new_way(k, seeded)
            old_way(k, seeded)
        new_ms, old_ms, argmin_ms = [], [], []
        for rep in range(reps):
            got, wall = new_way(k, seeded)
            new_ms.append(wall)
            old, res, wall, ms_arg = old_way(k, seeded)
            old_ms.append(wall)
            argmin_ms.append(ms_arg)
        infos = [g["info"] for g in got]
        same_cost = all(np.array_equal(g["cost"][0].view(np.uint32), b.view(np.uint32)) for g, (b, _) in zip(got, res))
        owner_diff = int(sum(int((g["owner"][0] != o).sum()) for g, (_, o) in zip(got, res)))
        cases[name] = {
            "members": int(k), "start_costs": seeded,
            "sets_call": {"ms_wall_median": float(np.median(new_ms)), "ms_wall_min": float(np.min(new_ms)),
                          "ms_wall_max": float(np.max(new_ms)), "exchanges": int(infos[0].exchanges),
                          "owner_exchanges": int(infos[0].owner_exchanges),
                          "ms_device_per_rank": [float(i.ms_device) for i in infos],
                          "records_per_rank": [int(i.records_sent) for i in infos],
                          "owner_records_per_rank": [int(i.owner_records_sent) for i in infos],
                          "roots_per_rank": [int(i.roots) for i in infos]},
            "one_field_per_member": {"ms_wall_median": float(np.median(old_ms)), "ms_wall_min": float(np.min(old_ms)),
                                     "ms_wall_max": float(np.max(old_ms)),
                                     "exchanges": int(old[0]["info"].exchanges),
                                     "ms_host_argmin_median": float(np.median(argmin_ms)),
                                     "records_per_rank": [int(g["info"].records_sent) for g in old]},
            # with start costs the host sum c + c0 is not the field's fold from the start cost: the bits may differ
            "cost_bits_equal": bool(same_cost), "owners_that_differ_from_the_argmin": owner_diff,
        }
        print(name, json.dumps(cases[name]), flush=True)

res = {
    **cut.header(),
    "nodes_per_rank": [int(v) for v, _ in sizes], "edges_per_rank": [int(n) for _, n in sizes],
    "ms_stitch_exchange": ms_stitch, "reps": reps, "cases": cases,
    "note": ("ms_wall = host clock around the collective call on all four threads (the slowest rank), downloads of "
             "cost, hops and owner (sets call) or of m x V_t costs and hops (one field per member) included.  The four "
             "ranks' kernels and copies share one GPU and one host here: this says what the exchanges cost on one "
             "shared card, not what four GPUs would give.  Over RCCL with more than one rank it has not run."),
}
cut.finish(res)
