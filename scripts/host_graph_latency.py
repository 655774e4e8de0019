#!/usr/bin/env python3
"""Run on the GPU box: latencies on a graph that was loaded from JSON, so that the engine has no device-built CSR and
the cost field and the stitch read the engine's upload of the graph (ensure_dev_graph).  An 800 x 800 mountain tile
is built and saved, a second engine loads it; then one cold solve, and 7 times each a solve, a routes call of three
routes, the 1 x 1 stitch_boundary and the 1 x 1 stitch_assemble.  Prints one line, HOSTGRAPH {json}: wall ms, the
five least of each series.  (scripts/cost_field_latency.py measures the solve on the device build's CSR.)"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "trg-planner_amd"))
import torch  # noqa: F401,E402  (before the engine: its ROCm libraries load first)
import trg_planner  # noqa: E402
from trg_planner import synth  # noqa: E402

prm = dict(expand_dist=0.6, robot_size=0.3, sample_num=16, height_threshold=0.16, collision_threshold=0.1,
           update_collision_threshold=0.5, safety_factor=3.0, goal_tolerance=0.8)
cloud = synth.mountain_cloud(800, 800, seed=3)
b = trg_planner.Engine(**prm)
b.set_sampler(7, 16)
b.set_global_map(cloud)
b.init_graph([40.0, 40.0, 0.0])
path = os.path.join(tempfile.mkdtemp(), "g.json")
b.save_json(path)
b.close()
e = trg_planner.Engine(**prm)
e.load_json(path)
V, E = e.graph_sizes("global")
core = np.array([-1e4, -1e4, 1e4, 1e4], np.float32)


def ms(f, n):
    out = []
    for _ in range(n):
        t = time.perf_counter()
        f()
        out.append((time.perf_counter() - t) * 1e3)
    return out


targets = [V - 1, V // 2, V // 3]
res = {"V": V, "E": E}
first = ms(lambda: e.cost_fields(source_ids=[0], full=False, targets=targets), 1)
res["solve_first_ms"] = round(first[0], 3)
t = ms(lambda: e.cost_fields(source_ids=[0], full=False, targets=targets), 7)
res["solve_ms"] = [round(x, 3) for x in sorted(t)[:5]]
t = ms(lambda: e.routes([0, 0, 0], targets), 7)
res["routes_ms"] = [round(x, 3) for x in sorted(t)[:5]]
t = ms(lambda: e.stitch_boundary(core, 1, 1, 0), 7)
res["stitch_boundary_ms"] = [round(x, 3) for x in sorted(t)[:5]]
t = ms(lambda: e.stitch_assemble(0, 1, [0, V], None, 0), 7)
res["stitch_assemble_ms"] = [round(x, 3) for x in sorted(t)[:5]]
print("HOSTGRAPH " + json.dumps(res), flush=True)
