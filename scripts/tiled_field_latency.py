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
import tempfile
import time

import numpy as np

from tiled_cut import Cut, bench, summary, tiled  # (first: it sets the paths and loads torch before the engine)
import field_ref  # (tests/: the compiled host Dijkstra)

cut = Cut("field", "r23_tiled_field.json", reps=15)
engines, ranks, reps = cut.engines, cut.ranks, cut.reps
(nb_nc, ms_stitch) = cut.stitch()
sizes, off = cut.sizes()
sources = cut.centres(off)  # the node nearest the centre of each tile's core; field 0 alone is the m = 1 case


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


def per_exchange(s):
    s["ms_wall_per_exchange"] = s["ms_wall_median"] / max(1, s["exchanges"])
    return s


info0 = [g["info"] for g in first_got]
res = {
    **cut.header(),
    "nodes_per_rank": [int(v) for v, _ in sizes], "edges_per_rank": [int(n) for _, n in sizes],
    "ghosts_per_rank": [int(i.ghosts) for i in info0], "border_nodes_per_rank": [int(i.border_nodes) for i in info0],
    "boundary_records_and_cross_edges": [int(x) for x in nb_nc[0]], "ms_stitch_exchange": ms_stitch,
    "sources": sources, "reps": reps,
    "first_call_m1_with_solve_graph_build": first,
    "solve_m1": per_exchange(summary(samples["m1"])), "solve_m4": per_exchange(summary(samples["m4"])),
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
cut.finish(res)
