#!/usr/bin/env python3
"""bench.py -- TRG construction throughput on MI355X (BASELINE.json metric).

A "step" is one full Traversal-Risk-Graph build over one synthetic terrain tile whose points are
already resident in HBM: map index build (setGlobalMap) + initGraph (BFS expansion + cleanGraph)
+ CSR in pinned/host memory.  value = (nodes + directed edges after cleanGraph) built per second,
summed over all ranks.

    python bench.py --gpus 1 --steps 3 --warmup 1
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

N > 1: one process per GPU, rank == spatial tile of one continuous terrain.  --scaling weak (default):
every rank holds a C3-sized core + halo (N x 10 M points); --scaling strong: the ONE C3 cloud is cut
into the N tiles (BASELINE config 4 = --gpus 4 --scaling strong: the 10 M-point cloud over 2 x 2).
Each rank builds the graph of its core on its GPU; the tile-boundary edges are then stitched with two
all-gather-v exchanges over RCCL (trg_planner/tiled.py; rule and parity oracle: DESIGN.md section 7).

A plain run sets up, warms up, times the --steps builds, writes --dump-outputs and prints the result
line (rank 0): the metric, `ms_per_step`, the workload's configuration and the per-step counters and
roofline figures that the timed builds themselves record.

--full adds, after the timed builds (rank 0's figures are reported): `ms_per_step_incl_upload` (the cloud
handed over in pageable host memory, as TRG::setGlobalMap gets it), `updates` (--updates K: K setLocalMap +
updateGraph steps of BASELINE config 5's stream on the built tile, with the CPU oracle's update beside it on
the bounded tile), and `cpu_baseline` (the oracle on a bounded tile, 3 repetitions, AND on the full
workload, one repetition in a child process on a core of its own while the GPU part runs).

--dump-outputs DIR: the graph the last timed step built, as the caller of that step receives it
(Engine.graph: node xyz / state / creation id, CSR rowptr / col, per-edge weight / dist) plus its sizes,
one DIR/<name>.npy each (rank r of N > 1: DIR/rank<r>_<name>.npy), float32 as built, integers exactly in
float64.  An array of more than DUMP_ROWS rows (DUMP_ROWS / N for N ranks) is written as the fixed, seeded
sample of rows `dump_rows(n, DUMP_ROWS)`, so that everything stays under 64 MB.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "trg-planner_amd"))

WORKLOADS = {
    # name: (nx, ny, sample_num, label)
    "c3": (3200, 3125, 16, "C3: synthetic 10M-pt Perlin terrain, mountain.yaml, sampleNum(k)=16"),
    "c2": (1000, 1000, 7, "C2: synthetic 1M-pt mountain, mountain.yaml (S=7)"),
    "small": (400, 400, 16, "smoke-size 160k-pt terrain, mountain.yaml, S=16"),
    # BASELINE config 1: the bundled indoor .pcd is not available offline -- a 40 m x 30 m
    # floor with 12 wall / box obstacles, voxel filter 0.2 (indoor.yaml), indoor.yaml parameters (step 3 of
    # expandGraph is ON for these: expand_dist - robot_size < 0.25 expand_dist)
    "c1": (0, 0, 15, "C1: synthetic indoor stand-in (40 m x 30 m floor, 12 obstacles, 0.1 m), voxel 0.2, indoor.yaml"),
}
INDOOR = dict(expand_dist=0.4, robot_size=0.3, height_threshold=0.15, collision_threshold=0.1,
              update_collision_threshold=0.1, safety_factor=3.0, goal_tolerance=0.8)
BOUNDED_N = 1200  # side of the bounded CPU-baseline tile (lattice points)
HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
MOUNTAIN = dict(expand_dist=0.6, robot_size=0.3, height_threshold=0.16, collision_threshold=0.1,
                update_collision_threshold=0.5, safety_factor=3.0, goal_tolerance=0.8)
DUMP_ROWS = 1 << 20  # --dump-outputs: longer arrays are written as a seeded sample of this many rows
DUMP_SEED = 20250418
DUMP_BYTES = 64 << 20


def terrain_tile(ix0, ix1, iy0, iy1, seed):
    """synth.mountain_tile(ix0, ix1, iy0, iy1, seed=seed), bit for bit, in a fraction of its time.

    Every point is a function of its global lattice index, so bands of lattice rows are generated
    on host threads (numpy lets go of the GIL inside its loops) straight into their place in row
    order; mountain_tile's seeded shuffle then follows as one gather through Generator.permutation,
    which draws the same swaps as Generator.shuffle (tests/test_bench_outputs.py holds the two equal)."""
    from concurrent.futures import ThreadPoolExecutor
    from trg_planner import synth
    nx = ix1 - ix0
    out = np.empty((nx * (iy1 - iy0), 3), dtype=np.float32)
    try:
        ncpu = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        ncpu = os.cpu_count() or 1
    nthreads = max(1, min(16, ncpu))
    bands = np.linspace(iy0, iy1, 4 * nthreads + 1).round().astype(np.int64)

    def band(j0, j1):
        out[(j0 - iy0) * nx:(j1 - iy0) * nx] = synth.mountain_tile(ix0, ix1, j0, j1, seed=seed, shuffle=False)

    with ThreadPoolExecutor(nthreads) as ex:
        list(ex.map(band, bands[:-1].tolist(), bands[1:].tolist()))
    rng = np.random.Generator(np.random.PCG64([seed & 0xFFFFFFFF, ix0 & 0xFFFFFFFF, iy0 & 0xFFFFFFFF]))
    return out[rng.permutation(out.shape[0])]


def dump_rows(n, max_rows):
    """The rows of an n-row array that --dump-outputs writes: all of them, or a fixed, seeded,
    sorted sample of max_rows when n is larger (the same rows for every array of n rows)."""
    if n <= max_rows:
        return None
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n, max_rows, replace=False))


def write_outputs(out_dir, arrays, max_rows=DUMP_ROWS, prefix=""):
    """arrays: name -> array.  Written as out_dir/<prefix><name>.npy: float32 stays float32, every
    other type goes to float64 (exact for the integers here); rows sampled by dump_rows.
    Returns the bytes written."""
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, a in arrays.items():
        a = np.asarray(a)
        a = a.astype(np.float32 if a.dtype == np.float32 else np.float64, copy=False)
        rows = dump_rows(a.shape[0], max_rows) if a.ndim else None
        if rows is not None:
            a = a[rows]
        a = np.ascontiguousarray(a)
        np.save(os.path.join(out_dir, f"{prefix}{name}.npy"), a)
        total += a.nbytes
    return total


def graph_outputs(g):
    """What Engine.graph() hands its caller, by name."""
    return {"sizes": np.array([g.V, g.E], np.float64), "xyz": g.xyz, "state": g.state, "cid": g.cid,
            "rowptr": g.rowptr, "col": g.col, "w": g.w, "dist": g.dist}


def kernel_source_sha():
    """sha256 over the kernel sources: a traffic record measured on other kernels must not be quoted"""
    import glob
    import hashlib
    h = hashlib.sha256()
    c = os.path.join(ROOT, "trg-planner_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(c, "*.hip")) + glob.glob(os.path.join(c, "*.inc")) +
                    [os.path.join(c, "trg_kernels.h"), os.path.join(c, "build.sh")]):  # (the flags they are built with)
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


def obs_stream(K, origin_xy, seed, lattice_hi):
    """BASELINE config 5's stream: K observation clouds = 20 m x 20 m crops (200 x 200 lattice points of
    the same terrain) around a pose moving 0.5 m per step along a polyline, with three injected obstacles
    (1.2 m boxes, every second point lifted by 1 m) that make updateGraph invalidate nodes."""
    from trg_planner import synth
    for k in range(K):
        leg, t = divmod(k, 40)
        dx, dy = ((0.5, 0.2), (0.2, 0.5), (-0.5, 0.2))[leg % 3]
        base = sum((np.array(((0.5, 0.2), (0.2, 0.5), (-0.5, 0.2))[j % 3]) * 40 for j in range(leg)), np.zeros(2))
        pose = (float(origin_xy[0] + base[0] + dx * t), float(origin_xy[1] + base[1] + dy * t))
        ix0 = int(np.clip(round(pose[0] / 0.1) - 100, 0, lattice_hi[0] - 200))
        iy0 = int(np.clip(round(pose[1] / 0.1) - 100, 0, lattice_hi[1] - 200))
        obs = synth.mountain_tile(ix0, ix0 + 200, iy0, iy0 + 200, seed=seed)
        for ox, oy in ((3.0, 1.0), (-4.0, 2.0), (1.0, -5.0)):
            b = (np.abs(obs[:, 0] - pose[0] - ox) < 0.6) & (np.abs(obs[:, 1] - pose[1] - oy) < 0.6)
            obs[b, 2] += np.float32(1.0) * (np.arange(int(b.sum())) % 2).astype(np.float32)
        yield pose, obs


def run_updates(target, K, origin_xy, seed, lattice_hi):
    """K setLocalMap + updateGraph steps on an engine or an oracle (same method names); latencies in ms"""
    t_map, t_upd, n_obs = [], [], []
    for pose, obs in obs_stream(K, origin_xy, seed, lattice_hi):
        t0 = time.perf_counter()
        target.set_local_map(pose, obs)
        t1 = time.perf_counter()
        target.update_graph()
        t2 = time.perf_counter()
        t_map.append(1e3 * (t1 - t0))
        t_upd.append(1e3 * (t2 - t1))
        n_obs.append(int(obs.shape[0]))
    if not t_upd:
        return None
    return {"updates": K, "obs_points_mean": float(np.mean(n_obs)),
            "set_local_map_ms_median": float(np.median(t_map)),
            "update_graph_ms_median": float(np.median(t_upd)),
            "update_graph_ms_p90": float(np.percentile(t_upd, 90)),
            "update_graph_ms_max": float(np.max(t_upd))}


def oracle_full_child(nx, ny, S, seed, out_path):
    """Child process (no GPU): the CPU oracle on the FULL workload, one repetition, one core."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_api as oa
    from trg_planner import synth
    try:  # a core of its own, far from the CCD the GPU-driving thread is pinned to
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[-1]})
    except (AttributeError, OSError):
        pass
    cloud = synth.mountain_tile(0, nx, 0, ny, seed=seed)
    used_ref = oa.use_reference_kd(True)
    o = oa.Oracle(**dict(MOUNTAIN, sample_num=S))
    o.set_sampler(7, 0, 16)
    t0 = time.perf_counter()
    o.set_global_map(cloud)
    t1 = time.perf_counter()
    ok = o.init_graph([nx * 0.05, ny * 0.05, 0.0])
    t2 = time.perf_counter()
    g = o.graph(0)
    json.dump({"ok": bool(ok), "V": int(g.V), "E": int(g.E), "index_s": t1 - t0, "init_graph_s": t2 - t1,
               "value": (g.V + g.E) / (t2 - t0), "points": int(cloud.shape[0]),
               "kd": "reference kdtree.c (oracle/_ref)" if used_ref else "oracle/okd.c restatement"},
              open(out_path, "w"))


def _host_cpu():
    model, cores = "unknown", os.cpu_count() or 0
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return model, cores


def cpu_baseline(sample_num, reps=3, updates=0, seed=20250418, given=None):
    """The CPU oracle (oracle/, a port of the reference algorithm; its spatial queries run through
    the reference kdtree.c when oracle/_ref is present) timed on this box's host, one core (pinned),
    on a bounded tile of the same terrain generator / parameters: `reps` repetitions, median.  With
    updates > 0 the last repetition's graph then goes through the same update stream as the engine's."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_api as oa
    from trg_planner import synth
    try:  # one core, like the reference's hot path (single thread under TRG::mtx.graph)
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
        pinned = True
    except (AttributeError, OSError):
        pinned = False
    nx = ny = BOUNDED_N  # 1.44 M points, ~94 k nodes at S=16: about 7 s of single-core work per repetition
    start = [nx * 0.05, ny * 0.05, 0.0]
    prm = dict(MOUNTAIN, sample_num=sample_num)
    if given is not None:  # (c1: the workload itself is small enough -- the very cloud, parameters and start)
        cloud, prm, start = given
        updates = 0
    else:
        cloud = synth.mountain_tile(0, nx, 0, ny, seed=seed)
    used_ref = oa.use_reference_kd(True)
    runs = []
    upd = None
    for rep in range(reps):
        o = oa.Oracle(**prm)
        o.set_sampler(7, 0, 16)
        t0 = time.perf_counter()
        o.set_global_map(cloud)
        t1 = time.perf_counter()
        ok = o.init_graph(start)
        t2 = time.perf_counter()
        g = o.graph(0)
        c = o.counters()
        runs.append(((g.V + g.E) / (t2 - t0), t1 - t0, t2 - t1, g.V, g.E, bool(ok), c["expanded"]))
        if rep == reps - 1 and updates > 0:
            upd = run_updates(o, updates, (nx * 0.05 - 20.0, ny * 0.05 - 10.0), seed, (nx, ny))
        o.close()
    oa.use_reference_kd(False)
    runs.sort()
    val, t_index, t_graph, V, E, ok, expanded = runs[len(runs) // 2]
    model, ncpu = _host_cpu()
    return {
        "value": val, "unit": "nodes+edges/s", "cores": 1, "kind": "port",
        "sample": ((f"bounded sample: {nx}x{ny}={nx * ny} pt tile of the same generator/params "
                    if given is None else f"the workload itself ({cloud.shape[0]} points) ") +
                   f"(S={sample_num}), V'={V} E'={E}; median of {reps} repetitions "
                   f"(index {t_index:.2f}s + initGraph {t_graph:.2f}s); TRG logic = oracle/trg_oracle.cpp "
                   f"(port), kd-tree = "
                   f"{'reference kdtree.c (oracle/_ref)' if used_ref else 'oracle/okd.c restatement'}; "
                   f"{'pinned to one core' if pinned else 'not pinned'}"),
        "host_cpu": model, "host_logical_cpus": ncpu,
        "all_repetitions": [r[0] for r in runs],
        "ok": ok, "us_per_expanded_node": 1e6 * t_graph / max(1, expanded),
        "updates": upd,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="after the timed builds also measure the pageable-upload step, the update stream "
                         "(--updates) and the CPU oracle baselines")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the graph of the last timed step as DIR/<name>.npy (see the module docstring)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU oracle baselines")
    ap.add_argument("--no-full-cpu-baseline", action="store_true",
                    help="--full: skip the one repetition of the CPU oracle on the full workload (a child process)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="N > 1: weak = every rank a workload-sized tile; strong = the one cloud cut into N tiles")
    ap.add_argument("--updates", type=int, default=20,
                    help="--full: K setLocalMap + updateGraph steps after the timed builds (BASELINE config 5's stream)")
    ap.add_argument("--seed", type=int, default=20250418)
    ap.add_argument("--oracle-full-child", nargs=4, metavar=("NX", "NY", "S", "OUT"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.oracle_full_child:  # (internal) the CPU oracle on the full workload; never touches the GPU
        nxc, nyc, Sc, outp = args.oracle_full_child
        oracle_full_child(int(nxc), int(nyc), int(Sc), args.seed, outp)
        return
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    rank0_env = int(os.environ.get("RANK", "0")) == 0
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    full_child, full_out = None, None
    if (args.full and rank0_env and world_env == 1 and not args.no_cpu_baseline and not args.no_full_cpu_baseline
            and args.workload != "c1"):
        # started before this process touches the GPU; runs on a core of its own while the GPU part runs
        import subprocess
        import tempfile
        nxw, nyw, Sw, _ = WORKLOADS[args.workload]
        full_out = os.path.join(tempfile.gettempdir(), f"trg_oracle_full_{os.getpid()}.json")
        full_child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--seed", str(args.seed),
                                       "--oracle-full-child", str(nxw), str(nyw), str(Sw), full_out],
                                      stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = max(1, torch.cuda.device_count())
    gpu_index = local_rank % ndev
    coll_dev = torch.device("cuda", gpu_index)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world <= ndev:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", gpu_index))
        else:
            # rehearsal with more ranks than GPUs (ranks share a card; RCCL refuses that): the
            # exchange goes over gloo with host tensors, everything else is unchanged
            dist.init_process_group(backend="gloo")
            coll_dev = torch.device("cpu")
    torch.cuda.set_device(gpu_index)
    dev = torch.device("cuda", gpu_index)
    local_rank = gpu_index

    import trg_planner
    from trg_planner import synth

    from trg_planner import tiled, tiling
    pinned = None if os.environ.get("TRG_NO_PIN") else tiling.pin_to_gpu_numa(gpu_index, slot=local_rank, nslots=min(world, ndev))
    nx, ny, S, label = WORKLOADS[args.workload]
    # One continuous terrain cut into a cols x rows grid of nx x ny tiles (C4/C5-style: 2x1, 2x2,
    # 4x2 ...); rank == tile.  Every rank holds its core plus a 1.1 m halo and
    # builds the graph of its core; for N > 1 the tile-boundary edges are stitched with two
    # all-gather-v exchanges over RCCL (trg_planner/tiled.py).  N = 1 is the plain single-root build.
    cols, rows = tiling.tile_layout(world)
    halo_pts = 11 if world > 1 else 0
    if args.scaling == "strong" and world > 1:
        # the ONE nx x ny cloud cut into cols x rows tiles (lattice columns / rows split as evenly as they go)
        core, win = tiled.split_tile(rank, cols, rows, nx, ny, halo_pts)
        lattice_hi = (nx, ny)
    else:
        core = tiled.tile_cores(cols, rows, nx, ny)[rank]
        win = tiled.tile_lattice_window(rank, cols, rows, nx, ny, halo_pts)
        lattice_hi = (cols * nx, rows * ny)
    PRM = MOUNTAIN
    voxel_info = None
    if args.workload == "c1":
        if world > 1:
            raise SystemExit("--workload c1 is a single-GPU configuration")
        PRM = INDOOR
        raw, _ = synth.indoor_cloud(seed=1, size=(40.0, 30.0))
        pre = trg_planner.Engine(**dict(INDOOR, sample_num=S), device=local_rank)
        t_v = time.perf_counter()
        cloud = pre.voxel_filter(raw, 0.2)  # pcl::VoxelGrid of loadPrebuiltMap (trg_planner.cpp:91-94), on the GPU
        voxel_info = {"points_in": int(raw.shape[0]), "points_out": int(cloud.shape[0]), "leaf": 0.2,
                      "ms_incl_transfers": 1e3 * (time.perf_counter() - t_v)}
        pre.close()
        core = np.array([0.0, 0.0, 40.0, 30.0], np.float32)
        lattice_hi = (400, 300)
    else:
        cloud = terrain_tile(*win, seed=args.seed)
    d_cloud = torch.from_numpy(cloud).to(dev)  # inputs resident in HBM before the timed region
    n_pts = cloud.shape[0]
    start = [0.5 * float(core[0] + core[2]), 0.5 * float(core[1] + core[3]), 0.0]
    if args.workload == "c1":
        start = [3.27, 4.12, 0.0]  # the first start of the reference's indoor pairs (run_trg_planner.py:27)
    h_cloud = cloud  # (pageable host memory: what TRG::setGlobalMap is handed)

    eng = trg_planner.Engine(**dict(PRM, sample_num=S), device=local_rank)
    eng.set_sampler(7, 16)
    if world > 1:
        eng.set_tile(core, epoch=rank)
    stitch_info = {"cross_edges": 0, "boundary_records": 0, "backend": "none"}

    def step():
        eng.set_global_map_device(d_cloud.data_ptr(), n_pts, 3)
        eng.init_graph(start)
        if world == 1:
            return eng.graph_sizes("global")
        # boundary extraction, pair search, cross-edge evaluation and the assembly of this tile's rows
        # of the global graph run on the GPU (trg_engine_stitch_*); the two all-gather-v exchanges
        # carry device tensors over RCCL (host tensors over gloo in the more-ranks-than-GPUs rehearsal)
        t_st = time.perf_counter()
        info = tiled.stitch_device(eng, rank, core, cols, rows, dist,
                                   None if coll_dev.type == "cuda" else coll_dev)
        stitch_info["cross_edges"] = info["n_cross"]
        stitch_info["boundary_records"] = info["n_boundary"]
        stitch_info["backend"] = info["backend"]
        stitch_info["ms_stitch_last"] = 1e3 * (time.perf_counter() - t_st)
        return eng.graph_sizes("stitched")  # this rank's rows of the assembled global graph

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    items = 0
    acc = {}
    for _ in range(args.steps):
        V, E = step()
        items += V + E
        st = eng.stats()
        for k, v in st.items():
            acc[k] = acc.get(k, 0) + v
    fence()
    dt = time.perf_counter() - t0

    if args.dump_outputs:  # the graph of the last timed step, before anything else runs on the engine
        nbytes = write_outputs(args.dump_outputs, graph_outputs(eng.graph("global" if world == 1 else "stitched")),
                               max_rows=DUMP_ROWS // world, prefix=f"rank{rank}_" if world > 1 else "")
        assert nbytes * world <= DUMP_BYTES, nbytes

    # ---- the same step with the cloud handed over in pageable host memory (setGlobalMap's real input) --------
    def step_upload():
        eng.set_global_map(h_cloud)
        ms_up = eng.stats()["ms_upload"]
        eng.init_graph(start)
        return ms_up

    fast = not args.full or bool(os.environ.get("TRG_BENCH_FAST"))  # (A/B scripts: the metric only)
    ms_incl_upload, ms_upload_only = None, [0.0]
    if not fast:
        step_upload()
        fence()
        t0u = time.perf_counter()
        n_up = max(1, min(args.steps, 5))
        ms_upload_only = [step_upload() for _ in range(n_up)]
        fence()
        ms_incl_upload = 1e3 * (time.perf_counter() - t0u) / n_up

    # ---- BASELINE config 5's update stream on the built tile (rank 0's numbers are reported) -------------------
    upd_info = None
    if args.updates > 0 and not fast and args.workload != "c1":
        upd_info = run_updates(eng, args.updates, (start[0] - 20.0, start[1] - 10.0), args.seed, lattice_hi)
        if upd_info:
            Vu, Eu = eng.graph_sizes("global")
            upd_info.update({"V_after": Vu, "E_after": Eu, "map_points": n_pts})
        fence()

    if os.environ.get("TRG_BENCH_DEBUG"):
        st_dbg = eng.stats()
        sys.stderr.write(f"[bench rank {rank}] used_device_bfs={st_dbg['used_device_bfs']} "
                         f"fallbacks={st_dbg['bfs_fallbacks']} max_spin={st_dbg['bfs_max_spin']} "
                         f"levels={st_dbg['bfs_levels']} reason={eng.fallback_reason!r}\n")
    if world > 1:
        items, dt = tiling.reduce_throughput(items, dt, dist, coll_dev)
        # nodes / directed edges of the assembled global graph = the sum of the ranks' stitched rows
        ve = torch.tensor([float(V), float(E)], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(ve, op=dist.ReduceOp.SUM)
        V, E = int(ve[0].item()), int(ve[1].item())

    if rank == 0:
        st = eng.stats()
        # the map-query kernels (the rest of the build is index/graph bookkeeping); names are those
        # rocprofv3 shows for the path that ran.  Device BFS: k_level_sample holds the sampling discs
        # (+ the elevation lookups), k_level_spec the speculative parent edges (timed together inside
        # the level loop: ms_sample_kernel), k_calls_gather the deferred wireEdge evaluations.
        dev = st["used_device_bfs"] == 1
        if dev:
            kernels = {
                "k_calls_gather": (acc["bytes_edge_kernel"], acc["ms_edge_kernel"], acc["launches_edge_kernel"]),
                "k_level_sample+k_level_spec": (acc["bytes_sample_kernel"] + acc["bytes_spec_kernel"],
                                                acc["ms_sample_kernel"], acc["launches_sample_kernel"]),
            }
        else:
            kernels = {
                "k_edges": (acc["bytes_edge_kernel"], acc["ms_edge_kernel"], acc["launches_edge_kernel"]),
                "k_spec_edges": (acc["bytes_spec_kernel"], acc["ms_spec_kernel"], acc["launches_spec_kernel"]),
                "k_sample_nodes": (acc["bytes_sample_kernel"], acc["ms_sample_kernel"],
                                   acc["launches_sample_kernel"]),
            }
        dom = max(kernels, key=lambda k: kernels[k][1])
        b, ms, launches = kernels[dom]
        achieved = (b / 1e9) / (ms / 1e3) if ms > 0 else 0.0
        # whole build: SURVEY section 8(d) B_alg = B_index + B_query + B_out over T_build
        b_out = 16 * V + 4 * (V + 1) + 12 * E
        b_alg_step = (acc["bytes_index_build"] + acc["bytes_sample_kernel"] + acc["bytes_spec_kernel"] +
                      acc["bytes_edge_kernel"]) / max(1, args.steps) + b_out
        build_gbps = (b_alg_step / 1e9) / (dt / max(1, args.steps))
        # HBM bytes per launch from the separate rocprofv3 --pmc passes of the same workload
        # (profiles/, scripts/profile_gpu.sh; FETCH_SIZE factor as established by scripts/fetch_unit.sh)
        traffic, traffic_src, traffic_note = None, None, None
        sha = kernel_source_sha()
        for tag in ("r03", "r02", "r01"):
            tpath = os.path.join(ROOT, "profiles", f"{tag}_{args.workload}_traffic.json")
            if os.path.exists(tpath):
                tj = json.load(open(tpath))
                parts = dom.split("+")  # kernels timed together: one launch of each per level
                if tj.get("kernel_source_sha256") != sha:
                    traffic_note = (f"{os.path.relpath(tpath, ROOT)} was measured on other kernel sources "
                                    f"(sha256 {str(tj.get('kernel_source_sha256'))[:12]} != {sha[:12]}): not quoted")
                else:
                    def per_launch(k):  # a kernel's variants (k, k<4>, k<8>, ...): one of them runs per level
                        v = [tj[n] for n in tj if isinstance(tj[n], dict) and (n == k or n.startswith(k + "<"))]
                        nd = sum(x["dispatches"] for x in v)
                        return sum(x["hbm_bytes_per_dispatch"] * x["dispatches"] for x in v) / nd if nd else None
                    per = [per_launch(k) for k in parts]
                    if all(x is not None for x in per):
                        traffic = sum(per)
                        traffic_src = os.path.relpath(tpath, ROOT)
                break
        out = {
            "metric": "TRG nodes+edges built/sec", "value": items / dt, "unit": "nodes+edges/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / max(1, args.steps), "higher_is_better": True,
            "scaling": args.scaling if world > 1 else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "full": args.full,
            "config": {
                "workload": label, "points_per_gpu": n_pts, "V_prime": V, "E_prime": E,
                "voxel_filter": voxel_info,
                "sampler": "counter-based table, seed 7, 16 bits",
                "host_thread": ("pinned to CPUs %d-%d of NUMA node %d (the GPU's)" % (pinned[1], pinned[2], pinned[0]))
                if pinned else "not pinned",
                "sharding": (f"{args.scaling} scaling: {cols}x{rows} tiles of one continuous terrain"
                             f"{' (the ONE workload cloud cut into tiles)' if args.scaling == 'strong' else ' (every tile workload-sized)'}"
                             f", one per rank, core + "
                             f"1.1 m halo; boundary edges stitched on the GPUs, 2 all-gather-v over "
                             f"{ {'nccl': 'RCCL (device tensors)', 'rccl-native': 'RCCL inside the engine (trg_engine_stitch_exchange)', 'gloo': 'gloo (host tensors: rehearsal)'}.get(stitch_info['backend'], stitch_info['backend'])} "
                             f"({stitch_info['cross_edges']} cross edges, "
                             f"{stitch_info['boundary_records']} boundary records); V'/E' = the assembled "
                             f"global graph")
                if world > 1 else "single tile",
            },
            "roofline": {
                "bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBPS,
                "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic,
                "traffic_source": traffic_src, "traffic_note": traffic_note, "kernel_source_sha256": sha,
                "build_GBps": build_gbps, "build_frac": build_gbps / HBM_PEAK_GBPS,
                "build_alg_bytes_per_step": b_alg_step,
                "alg_bytes_per_launch": b / max(1, launches),
                "avg_launch_ms": ms / max(1, launches), "launches": launches,
                "all_kernels_GBps": {k: ((v[0] / 1e9) / (v[1] / 1e3) if v[1] > 0 else 0.0)
                                     for k, v in kernels.items()},
            },
            "breakdown_last_step": {
                "ms_index_build_gpu": st["ms_index_build"], "ms_init_graph_total": st["ms_init_graph_total"],
                "ms_replay_host": st["ms_replay_host"], "ms_finalize_host": st["ms_finalize_host"],
                "ms_wait_gpu": st["ms_wait_gpu"], "ms_sample_kernel": st["ms_sample_kernel"],
                "ms_spec_kernel": st["ms_spec_kernel"], "ms_edge_kernel": st["ms_edge_kernel"],
                "expanded_nodes": st["expanded_nodes"], "samples": st["samples"],
                "edge_evals_gpu": st["edge_evals_gpu"], "nn_ties": st["nn_ties"], "map_nn_ties": st["map_nn_ties"],
                "gate_uncertain": st["gate_uncertain"], "bfs_levels": st["bfs_levels"],
                "used_device_bfs": st["used_device_bfs"], "bfs_fallbacks": st["bfs_fallbacks"],
                "bfs_host_levels": st["bfs_host_levels"], "bfs_ticket_reruns": st["bfs_ticket_reruns"],
                "presampled_nodes": st["presampled_nodes"],
                "bfs_max_spin": st["bfs_max_spin"], "ms_bfs_loop": st["ms_bfs_loop"],
                "ms_deferred": st["ms_deferred"], "ms_rare_events": st["ms_rare_events"],
                "ms_set_map_total": st["ms_set_map_total"],
                "map_nn_resolved": st["map_nn_resolved"], "map_nn_unresolved": st["map_nn_unresolved"],
                "ms_stitch_rank0": stitch_info.get("ms_stitch_last", 0.0),
                "fallback_reason": eng.fallback_reason,
            },
        }
        if args.full:
            out["ms_per_step_incl_upload"] = ms_incl_upload
            out["upload"] = {"ms_per_step": ms_incl_upload, "ms_upload_median": float(np.median(ms_upload_only)),
                             "bytes": int(n_pts) * 12,
                             "note": "the cloud in pageable host memory (numpy), staged through pinned chunks by 4 "
                                     "host threads + hipMemcpyAsync; `value` / `ms_per_step` keep the cloud resident "
                                     "in HBM"}
            out["updates"] = upd_info
        if args.full and not args.no_cpu_baseline and world == 1:
            cb = cpu_baseline(S, updates=min(args.updates, 10), seed=args.seed,
                              given=(h_cloud, dict(PRM, sample_num=S), start) if args.workload == "c1" else None)
            cb["bounded_sample_value"] = cb["value"]
            if full_child is not None:  # the oracle on the FULL workload (child process, one repetition)
                try:
                    full_child.wait(timeout=420)
                    fj = json.load(open(full_out))
                    os.remove(full_out)
                    cb["full_workload"] = fj
                    if fj.get("ok") and fj["V"] == V and fj["E"] == E:
                        cb["value"] = fj["value"]
                        cb["sample"] = (f"the FULL workload ({fj['points']} points, S={S}): one repetition measured in this "
                                        f"run on a host core of its own (index {fj['index_s']:.1f}s + initGraph "
                                        f"{fj['init_graph_s']:.1f}s, V'={fj['V']} E'={fj['E']} = the GPU build's); "
                                        f"kd-tree = {fj['kd']}.  Also: " + cb["sample"])
                except Exception as ex:  # noqa: BLE001  (the bounded sample stands)
                    full_child.kill()
                    cb["full_workload"] = {"ok": False, "error": repr(ex)}
            out["cpu_baseline"] = cb
            out["speedup_vs_cpu_baseline"] = out["value"] / cb["value"]
            if upd_info and cb.get("updates"):
                out["updates"]["cpu_oracle_on_bounded_tile"] = cb["updates"]
        elif full_child is not None:
            full_child.kill()
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
