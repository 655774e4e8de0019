"""Map ingest (voxel-grid filter, cell-sorted map index): plain numpy definitions and the named clouds of
tests/test_map_ingest_cpu.py and tests/test_gpu_map_ingest.py.  No GPU, no oracle: numpy and trg_planner.synth only.

Every cloud is seeded and a function of nothing else; the large ones are built once per process."""
import functools
from collections import namedtuple

import numpy as np

from trg_planner import synth

F32 = np.float32
U24 = 2.0 ** -24                      # unit roundoff of fp32
NEG_NAN = np.array([0xFFC00000], np.uint32).view(F32)[0]    # a quiet NaN with the sign bit set
BAD_COLUMNS = (np.nan, 1e30)          # what the columns past z hold: a kernel that reads them cannot pass

GRID_THREADS = 4096 * 256             # grid_for (trg_voxel.hip), k_cell_count / k_scatter_aos: 4096 blocks of 256
SECOND_TRIP_N = GRID_THREADS + 257    # ... so the grid-stride loops take a second trip (k_bounds: 1024 blocks, a fifth)
SCAN_SECOND_TRIP_N = 2048 * 257 + 1   # 258 tile sums: k_scan_tile_sums carries past its first 256
VOXEL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097)
INT32_MAX = 2 ** 31 - 1


# ---- definitions ---------------------------------------------------------------------------------------------------
def voxel_keys(xyz3, leaf):
    """(finite rows' indices, their voxel index) as pcl::VoxelGrid defines it: fp32 bounds over the finite points,
    min_b = floor(min * inv), ijk = floor(p * inv) - min_b, idx = i + j * dx + k * dx * dy -- all products in fp32."""
    xyz3 = np.asarray(xyz3, F32).reshape(-1, 3)
    keep = np.flatnonzero(np.isfinite(xyz3).all(axis=1))
    p = xyz3[keep]
    inv = F32(1.0) / F32(leaf)
    mn = np.floor(p.min(axis=0) * inv).astype(np.int64)
    mx = np.floor(p.max(axis=0) * inv).astype(np.int64)
    dims = mx - mn + 1
    ijk = np.floor(p * inv).astype(np.int64) - mn
    return keep, ijk[:, 0] + ijk[:, 1] * dims[0] + ijk[:, 2] * dims[0] * dims[1]


def voxel_index_space(xyz3, leaf):
    """dx * dy * dz as the filter computes it before it decides to hand the input through (> INT32_MAX)."""
    xyz3 = np.asarray(xyz3, F32).reshape(-1, 3)
    p = xyz3[np.isfinite(xyz3).all(axis=1)]
    inv = F32(1.0) / F32(leaf)
    d = ((p.max(axis=0) - p.min(axis=0)) * inv).astype(np.int64) + 1      # (fp32 difference, fp32 product, truncation)
    return int(d[0]) * int(d[1]) * int(d[2])


def voxel_centroids64(xyz3, leaf):
    """-> (centroids float64 (V, 3), counts (V,), largest |coordinate| per voxel and axis (V, 3)): one row per
    occupied voxel in ascending voxel index, the mean of its finite points with float64 sums (synth.voxel_centroids
    does the same for a finite cloud, rounds to fp32 and keeps no counts, which the error bound needs)."""
    xyz3 = np.asarray(xyz3, F32).reshape(-1, 3)
    keep, key = voxel_keys(xyz3, leaf)
    order = np.argsort(key, kind="stable")
    p = xyz3[keep][order].astype(np.float64)
    _, start, counts = np.unique(key[order], return_index=True, return_counts=True)
    sums = np.add.reduceat(p, start, axis=0)
    return sums / counts[:, None], counts, np.maximum.reduceat(np.abs(p), start, axis=0)


def index_wh(cloud_xyz, g):
    """(W, H) of the map grid as build_map computes them: fp32 bounds, fp32 1 / g, fp32 product, floor, + 1."""
    xy = np.asarray(cloud_xyz, F32)[:, :2]
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    inv_g = F32(1.0) / F32(g)
    wh = np.floor((hi - lo) * inv_g).astype(np.int64) + 1
    return int(wh[0]), int(wh[1])


def index_definition(cloud_xyz, x, y, z, perm, wh, org):
    """What the cell-sorted map index is, asserted: `perm` a permutation, (x, y, z) = cloud[perm] bit for bit,
    org = (min x, min y, cell size), wh from the fp32 formula of build_map, cells non-decreasing in row-major order
    with cell = clip(floor((v - v0) * inv_g), 0, dim - 1) in fp32, and perm ascending inside a cell."""
    cloud = np.asarray(cloud_xyz, F32)[:, :3]
    n = cloud.shape[0]
    perm = np.asarray(perm)
    assert perm.shape == (n,) and np.array_equal(np.sort(perm), np.arange(n))
    for k, v in enumerate((x, y, z)):
        assert v.dtype == F32 and np.array_equal(v.view(np.uint32), cloud[perm, k].view(np.uint32)), "xyz"[k]
    lo = cloud[:, :2].min(axis=0)
    assert np.array_equal(np.asarray(org[:2], F32).view(np.uint32), lo.view(np.uint32)), (org, lo)
    g = F32(org[2])
    assert g > 0
    assert (int(wh[0]), int(wh[1])) == index_wh(cloud, g), (wh, index_wh(cloud, g))
    inv_g = F32(1.0) / g
    cx = np.clip(np.floor((x - lo[0]) * inv_g), 0, wh[0] - 1).astype(np.int64)
    cy = np.clip(np.floor((y - lo[1]) * inv_g), 0, wh[1] - 1).astype(np.int64)
    cell = cy * int(wh[0]) + cx
    step = np.diff(cell)
    assert np.all(step >= 0)
    assert np.all(np.diff(perm.astype(np.int64))[step == 0] > 0)


def with_stride(xyz3, k):
    """(N, k) float32, C-contiguous: xyz3 and k - 3 columns of NaN and 1e30 in turn."""
    xyz3 = np.asarray(xyz3, F32)
    out = np.empty((xyz3.shape[0], k), F32)
    out[:, :3] = xyz3
    for c in range(3, k):
        out[:, c] = BAD_COLUMNS[(c - 3) % 2]
    return out


# ---- the clouds ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cube():
    """uniform points in a 6 m cube: at leaf 0.5 that is 12^3 voxels, several points in each from a few hundred on"""
    c = np.random.default_rng(41).uniform(0.0, 6.0, (SCAN_SECOND_TRIP_N, 3)).astype(F32)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _terrain():
    """SECOND_TRIP_N points of one terrain (the tile is shuffled, so its head is a sample of all of it)"""
    c = synth.mountain_tile(0, 1025, 0, 1024, seed=3)[:SECOND_TRIP_N]
    c.setflags(write=False)
    return c


def _terrain_nan():
    c = _terrain().copy()
    c[[0, GRID_THREADS - 1, GRID_THREADS, SECOND_TRIP_N - 1]] = np.nan
    return c


def edge_cases_5000():
    """the cloud of test_voxel_filter_edge_cases (tests/test_gpu_voxel.py)"""
    pts = np.random.default_rng(1).uniform(-5, 5, (5000, 3)).astype(F32)
    pts[::97] = np.nan
    return pts


def _nonfinite_forms():
    pts = np.random.default_rng(42).uniform(-4, 4, (2000, 3)).astype(F32)
    pts[0, 0] = np.inf                # a bad point first ...
    pts[1999, 2] = -np.inf            # ... and last (k_vox_heads treats i == 0 apart)
    pts[7::211, 0] = np.inf           # +Inf in x only
    pts[11::173, 2] = -np.inf         # -Inf in z only
    pts[13::151, 1] = np.nan          # NaN in y only
    pts[17::131, 1] = NEG_NAN         # a NaN with the sign bit set: the other end of the ordered-key range
    pts[19::307, 0] = NEG_NAN
    return pts


def _all_nonfinite():
    pts = np.random.default_rng(43).uniform(-4, 4, (300, 3)).astype(F32)
    bad = np.array([np.nan, np.inf, -np.inf, NEG_NAN], F32)
    pts[np.arange(300), np.arange(300) % 3] = bad[np.arange(300) % 4]
    return pts


def _one_voxel():
    return np.random.default_rng(44).uniform(3.01, 3.49, (5000, 3)).astype(F32)


def _one_per_voxel():
    rng = np.random.default_rng(45)
    i, j, k = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    pts = np.stack([i.ravel(), j.ravel(), k.ravel()], 1) + rng.uniform(0.1, 0.9, (4096, 3))
    return rng.permutation(pts.astype(F32))


def _far_shift():
    return _cube()[:5000] + np.array([-4096.3, 8191.7, -250.0], F32)


def _int32_edge(far):
    """corner points (0.5, 0.5, 0.5) and (far, far, far), 50 points in between, 3 more in the far corner's voxel"""
    rng = np.random.default_rng(46)
    top = np.floor(far)
    pts = np.concatenate([[[0.5, 0.5, 0.5]], rng.uniform(1.0, top - 1.0, (50, 3)), [[far, far, far]],
                          rng.uniform(top, far, (3, 3))]).astype(F32)
    return rng.permutation(pts)


def _line(axis):
    rng = np.random.default_rng(47 + axis)
    pts = np.empty((3000, 3), F32)
    pts[:, axis] = rng.uniform(-20.0, 40.0, 3000)
    pts[:, 1 - axis] = 5.25
    pts[:, 2] = rng.uniform(-0.2, 0.2, 3000)
    return pts


def _one_cell():
    rng = np.random.default_rng(49)
    return np.concatenate([rng.uniform(7.0, 7.25, (500, 2)), rng.uniform(-0.2, 0.2, (500, 1))], 1).astype(F32)


def _strip():
    """400 x 3 cells of 0.3 m: the corners are points of the cloud, so the extent is exact"""
    rng = np.random.default_rng(50)
    xy = rng.uniform((0.0, 0.0), (119.9, 0.8), (20000, 2))
    xy[:2] = (0.0, 0.0), (119.9, 0.8)
    return rng.permutation(np.concatenate([xy, rng.uniform(-0.2, 0.2, (20000, 1))], 1).astype(F32))


@functools.lru_cache(maxsize=None)
def _plan_cloud():
    c = synth.mountain_cloud(91, 91, seed=23, amplitude=2.0, wavelength=15.0)   # 8281 points
    c.setflags(write=False)
    return c


ORIGINS = {"near": (-37.3, 12.9), "far": (4096.5, -8191.25)}


@functools.lru_cache(maxsize=None)
def origin_cloud(name):
    c = synth.mountain_cloud(120, 120, seed=21, amplitude=2.0, wavelength=15.0, origin=ORIGINS[name])
    c.setflags(write=False)
    return c


def boundary_probes(cloud, m, seed, outside=3.0):
    """(m, 2) float32 positions: three quarters inside the cloud's bounding box, a quarter up to `outside` metres
    beyond it, equally on its four sides (there cell_coord clamps the cell range of the query)."""
    rng = np.random.default_rng(seed)
    lo, hi = cloud[:, :2].min(axis=0).astype(np.float64), cloud[:, :2].max(axis=0).astype(np.float64)
    k = m // 16
    parts = [rng.uniform(lo, hi, (m - 4 * k, 2))]
    for axis in (0, 1):
        for side in (0, 1):
            p = rng.uniform(lo - outside, hi + outside, (k, 2))
            off = rng.uniform(0.0, outside, k)
            p[:, axis] = lo[axis] - off if side == 0 else hi[axis] + off
            parts.append(p)
    return np.concatenate(parts).astype(F32)


# make() -> (N, 3) float32; passthrough: the filter hands the input through; multi: some voxel holds several points
VoxelCase = namedtuple("VoxelCase", "make leaf passthrough multi")
# wh: the (W, H) the issue states for the cloud at a cell size of 0.3 m, None where it states none for that axis
IndexCase = namedtuple("IndexCase", "make wh")


def ingest_cases():
    """-> {"voxel": {name: VoxelCase}, "index": {name: IndexCase}, "origin": {name: make}} (origin_cloud's clouds)"""
    vox = {f"size_{n}": VoxelCase(lambda n=n: _cube()[:n], 0.5, False, n >= 255) for n in VOXEL_SIZES}
    vox.update({
        "scan_second_trip": VoxelCase(_cube, 0.5, False, True),
        "stride_second_trip": VoxelCase(_terrain_nan, 0.2, False, True),
        "copy_second_trip": VoxelCase(_terrain_nan, 1e-4, True, False),
        "edge_cases_5000": VoxelCase(edge_cases_5000, 0.5, False, True),
        "nonfinite_forms": VoxelCase(_nonfinite_forms, 0.5, False, True),
        "all_nonfinite": VoxelCase(_all_nonfinite, 0.5, False, False),
        "one_voxel": VoxelCase(_one_voxel, 0.5, False, True),
        "one_per_voxel": VoxelCase(_one_per_voxel, 1.0, False, False),
        "far_shift": VoxelCase(_far_shift, 0.2, False, True),
        "int32_filtered": VoxelCase(lambda: _int32_edge(1289.5), 1.0, False, True),
        "int32_passthrough": VoxelCase(lambda: _int32_edge(1290.5), 1.0, True, False),
    })
    idx = {
        "line_x": IndexCase(lambda: _line(0), (None, 1)),
        "line_y": IndexCase(lambda: _line(1), (1, None)),
        "one_cell": IndexCase(_one_cell, (1, 1)),
        "one_point": IndexCase(lambda: np.array([[3.5, -2.25, 0.75]], F32), (1, 1)),
        "two_identical": IndexCase(lambda: np.array([[3.5, -2.25, 0.75]] * 2, F32), (1, 1)),
        "n_8191": IndexCase(lambda: _plan_cloud()[:8191], (None, None)),
        "n_8192": IndexCase(lambda: _plan_cloud()[:8192], (None, None)),
        "n_8193": IndexCase(lambda: _plan_cloud()[:8193], (None, None)),
        "second_trip": IndexCase(_terrain, (None, None)),
        "strip_400x3": IndexCase(_strip, (400, 3)),
    }
    return {"voxel": vox, "index": idx, "origin": {name: functools.partial(origin_cloud, name) for name in ORIGINS}}
