"""What the tiled_*_latency.py scripts share (import it first: it sets the paths and loads torch before the engine):
their options, the bench cloud cut 2 x 2 as `bench.py --gpus 4 --scaling strong` cuts it with FOUR engines on ONE card
over the in-process transport, a call on every rank from a thread each, the stitch with its wall time, the node
nearest the centre of each tile's core, the summary of a list of per-solve records, and the result file."""
import json
import os
import sys
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

COLS = ROWS = 2
R = COLS * ROWS
SEED = 20250418
argv = sys.argv[1:]


def option(name, default):
    if name in argv:
        i = argv.index(name)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return default


class Cut:
    """--out (default profiles/`profile`), --reps and --workload read; the four engines built, each on its tile of
    the workload's cloud, and joined as the ranks of one in-process group named after `name`."""

    def __init__(self, name, profile, reps):
        self.out = os.path.abspath(option("--out", os.path.join(ROOT, "profiles", profile)))
        self.reps = int(option("--reps", reps))
        self.nx, self.ny, S, self.label = bench.WORKLOADS[option("--workload", "c3")]
        self.engines, self.cores, self.n_points = [], [], 0
        for t in range(R):
            core, win = tiled.split_tile(t, COLS, ROWS, self.nx, self.ny, 11)
            cloud = bench.terrain_tile(*win, seed=SEED)
            self.n_points += int(cloud.shape[0])
            e = trg_planner.Engine(**dict(bench.MOUNTAIN, sample_num=S))
            e.set_sampler(7, 16)
            e.set_tile(core, epoch=t)
            e.set_global_map(cloud)
            e.init_graph([0.5 * float(core[0] + core[2]), 0.5 * float(core[1] + core[3]), 0.0])
            self.engines.append(e)
            self.cores.append(core)
            del cloud
        for t, e in enumerate(self.engines):
            e.comm_join_local(f"tiled-{name}-latency-{os.getpid()}", R, t)

    def ranks(self, call):
        """call(rank, engine) on every rank, one thread each -> (results, wall ms of the slowest)"""
        res, err = [None] * R, [None] * R

        def run(r):
            try:
                res[r] = call(r, self.engines[r])
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

    def stitch(self):
        """the stitch exchange on every rank -> (per rank (boundary records, cross edges), wall ms)"""
        return self.ranks(lambda r, e: e.stitch_exchange(self.cores[r], COLS, ROWS))

    def sizes(self):
        """-> (per rank (nodes, edges) of its stitched rows, the R + 1 global id offsets)"""
        sizes = [e.graph_sizes("stitched") for e in self.engines]
        return sizes, np.concatenate([[0], np.cumsum([v for v, _ in sizes])]).astype(np.int64)

    def centres(self, off):
        """per tile the node nearest the centre of its core, as global ids"""
        out = []
        for t, e in enumerate(self.engines):
            xyz = e.node_xyz("global")
            core = self.cores[t]
            c = np.array([0.5 * (core[0] + core[2]), 0.5 * (core[1] + core[3])], np.float32)
            out.append(int(off[t]) + int(np.argmin(((xyz[:, :2] - c) ** 2).sum(1))))
        return out

    def header(self):
        """the result's first entries: workload, ranks, transport"""
        return {"workload": f"{self.label}: {self.nx}x{self.ny} lattice cut {COLS}x{ROWS} (split_tile, 1.1 m halo), "
                            f"{self.n_points} points in all",
                "ranks": R, "transport": "in-process (trg_engine_comm_join_local): FOUR RANKS SHARE ONE GPU"}

    def finish(self, res):
        """the result to --out and to the output; the engines closed"""
        os.makedirs(os.path.dirname(self.out), exist_ok=True)
        json.dump(res, open(self.out, "w"), indent=1)
        print(json.dumps(res, indent=1))
        for e in self.engines:
            e.close()


def summary(recs, mins=False):
    """Of a list of per-solve records: the last one's counters, median / min / max of ms_wall, and of every other ms_
    entry (per rank) the median (with `mins` the minimum too)."""
    s = {k: v for k, v in recs[-1].items() if "ms_" not in k}
    wall = [r["ms_wall"] for r in recs]
    s.update(ms_wall_median=float(np.median(wall)), ms_wall_min=float(np.min(wall)), ms_wall_max=float(np.max(wall)))
    for key in [k for k in recs[-1] if "ms_" in k and k != "ms_wall"]:
        s[key + "_median"] = np.median(np.array([r[key] for r in recs]), axis=0).tolist()
        if mins:
            s[key + "_min"] = np.min(np.array([r[key] for r in recs]), axis=0).tolist()
    return s
