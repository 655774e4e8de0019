#!/usr/bin/env python3
"""Run on the GPU box: what a risk field across tiles (Engine.tiled_risk_fields / tiled_risk_fields_from /
tiled_safest_routes; DESIGN.md section 7, "Risk fields across tiles") costs on the bench cloud cut 2 x 2 as
`bench.py --gpus 4 --scaling strong` cuts it -- FOUR engines on ONE card over the in-process transport, one thread per
rank -- next to the same call for the cost objective on the same cut in the same run, and next to the host way:
exporting the four tiles' stitched rows to one host, concatenating them and running the compiled host Dijkstra on the
(risk, hops) key (tests/cpp/risk_reference.cpp) there.

Three shapes, the objectives alternating within every repetition: (a) one field (m = 1); (b) one field from a set of 8
members, two per tile; (c) the safest routes from one node to 8 goals -- tiled_safest_routes' two calls (a solve
without parents, then the routes without a capacity), made one after the other here so that both infos are kept, and
tiled_plan_many's for the cost objective.  Reported per shape and objective (medians and minima of --reps after a
warm-up): the wall time of the collective call (the slowest rank), the device time per rank, exchanges, rounds and
records sent per rank.  Four ranks share one GPU here: the numbers say how many exchanges a field needs and what an
exchange costs in host round trips, not what four GPUs would give.  Over RCCL with more than one rank this has not run.

usage: python scripts/tiled_risk_latency.py [--out PATH] [--reps N] [--workload c3|c2|small]
       -> PATH (default profiles/r29_tiled_risk.json)
"""
import tempfile
import time

import numpy as np

from tiled_cut import R, Cut, summary, tiled  # (first: it sets the paths and loads torch before the engine)
import risk_ref  # (tests/: the compiled host Dijkstra on the (risk, hops) key)

cut = Cut("risk", "r29_tiled_risk.json", reps=15)
engines, ranks, reps = cut.engines, cut.ranks, cut.reps
(nb_nc, ms_stitch) = cut.stitch()
sizes, off = cut.sizes()
# per tile: the node nearest the centre of its core and the node a third of the way through its ids (global ids)
centres = cut.centres(off)
thirds = [int(off[t]) + sizes[t][0] // 3 for t in range(R)]
start = centres[0]
members = centres + thirds  # the set of 8
goals = centres[1:] + thirds + [int(off[R]) - 1]  # the 8 goals


def record(infos, wall, routes=None):
    rec = {"ms_wall": wall, "ms_device_per_rank": [float(i.ms_device) for i in infos],
           "exchanges": int(infos[0].exchanges), "rounds_per_rank": [int(i.rounds) for i in infos],
           "records_per_rank": [int(i.records_sent) for i in infos]}
    if hasattr(infos[0], "owner_exchanges"):
        rec["owner_exchanges"] = int(infos[0].owner_exchanges)
        rec["owner_records_per_rank"] = [int(i.owner_records_sent) for i in infos]
    if routes is not None:
        rec["routes_exchanges"] = int(routes[0].exchanges)
        rec["routes_records_per_rank"] = [int(i.records_sent) for i in routes]
        rec["routes_ms_device_per_rank"] = [float(i.ms_device) for i in routes]
        rec["routes_max_nodes"] = int(routes[0].max_nodes)
    return rec


def routes_of(e, solve):
    """tiled_safest_routes' / tiled_plan_many's two calls, both infos kept"""
    s = solve(e)
    r = e.tiled_routes(np.zeros(len(goals), np.int32), goals)
    return dict(r, solve_info=s["info"])


def field(risk):
    call = (lambda r, e: e.tiled_risk_fields([start])) if risk else (lambda r, e: e.tiled_cost_fields([start]))
    got, wall = ranks(call)
    return got, record([g["info"] for g in got], wall)


def sets(risk):
    call = (lambda r, e: e.tiled_risk_fields_from([members])) if risk else \
        (lambda r, e: e.tiled_cost_fields_from([members]))
    got, wall = ranks(call)
    return got, record([g["info"] for g in got], wall)


def routes(risk):
    solve = (lambda e: e.tiled_risk_fields([start], parent=False)) if risk else \
        (lambda e: e.tiled_cost_fields([start], parent=False))
    got, wall = ranks(lambda r, e: routes_of(e, solve))
    return got, record([g["solve_info"] for g in got], wall, [g["info"] for g in got])


shapes = {"field_m1": field, "set_of_8": sets, "routes_to_8": routes}
first = {}
for name, risk in (("cost", False), ("risk", True)):  # the first calls: the solve graph, then its edge risks
    first[name] = field(risk)[1]
for fn in shapes.values():  # warm-up
    for risk in (True, False, True, False):
        fn(risk)
samples = {k: {"risk": [], "cost": []} for k in shapes}
last = {}
for rep in range(reps):
    for k, fn in shapes.items():
        for name, risk in (("risk", True), ("cost", False)):
            got, rec = fn(risk)
            samples[k][name].append(rec)
            last[k, name] = got
    print("rep", rep, flush=True)

# the host way: the rows to one host, one CSR, the compiled Dijkstra on the (risk, hops) key
t0 = time.perf_counter()
G = tiled.concat_stitched([e.graph("stitched") for e in engines])
ms_export = 1e3 * (time.perf_counter() - t0)
lib = risk_ref.compile_reference(tempfile.mkdtemp())
host_ms = {"field_m1": [], "set_of_8": []}
host = {}
for rep in range(reps):
    for k, src in (("field_m1", [start]), ("set_of_8", members)):
        t0 = time.perf_counter()
        host[k] = risk_ref.risk_field(lib, G["rowptr"], G["col"], G["w"], G["state"], src)
        host_ms[k].append(1e3 * (time.perf_counter() - t0))
assert host["field_m1"][0] == 0 and host["set_of_8"][0] == 0


def same(parts, want):
    f = tiled.concat_fields(parts)
    return bool(np.array_equal(f["risk"][0].view(np.uint32), want[1].view(np.uint32)) and
                np.array_equal(f["hops"][0], want[2]) and np.array_equal(f["parent"][0], want[3]))


exact = {"field_m1": same(last["field_m1", "risk"], host["field_m1"]),
         "set_of_8": same(last["set_of_8", "risk"], host["set_of_8"])}
joined = tiled.join_routes(last["routes_to_8", "risk"])
exact["routes_to_8_cost_is_risk_at_goal"] = bool(all(
    np.float32(i.cost).view(np.uint32) == host["field_m1"][1][g:g + 1].view(np.uint32)[0] and
    i.num_nodes == host["field_m1"][2][g] + 1 for g, (_, _, i) in zip(goals, joined)))


w = G["w"]
res = {
    **cut.header(),
    "nodes_per_rank": [int(v) for v, _ in sizes], "edges_per_rank": [int(n) for _, n in sizes],
    "ghosts_per_rank": [int(g["info"].ghosts) for g in last["field_m1", "risk"]],
    "border_nodes_per_rank": [int(g["info"].border_nodes) for g in last["field_m1", "risk"]],
    "boundary_records_and_cross_edges": [int(x) for x in nb_nc[0]], "ms_stitch_exchange": ms_stitch,
    "edge_weights_exactly_zero": float((w == 0).mean()), "start": start, "members": members, "goals": goals, "reps": reps,
    "first_calls_m1": {"cost_with_solve_graph_build": first["cost"], "risk_with_edge_risk_build": first["risk"]},
    "shapes": {k: {name: summary(v, mins=True) for name, v in by.items()} for k, by in samples.items()},
    "host_way": {"ms_export_and_concat_once_per_stitch": ms_export,
                 "ms_risk_reference_median": {k: float(np.median(v)) for k, v in host_ms.items()},
                 "ms_risk_reference_min": {k: float(np.min(v)) for k, v in host_ms.items()},
                 "V": int(G["V"]), "E": int(G["col"].shape[0])},
    "device_equals_host_reference": exact,
    "note": ("ms_wall = host clock around the collective call(s) on all four threads (the slowest rank), downloads "
             "included; ms_device = hipEvent time of a rank's own kernels between its exchanges.  The four ranks' "
             "kernels and copies share one GPU and one host here, so the wall time is an upper bound of what an "
             "exchange costs in host round trips, not a multi-GPU figure; over RCCL with more than one rank this has "
             "not run.  routes_to_8: the solve (without parents) and the two routes calls (lengths, then ids)."),
}
cut.finish(res)
