"""Test data: builds at the parameters the rest of the suite never moves -- robot_size (the cell of the map index and of
the node grid, the step of the segment walk, the radius of every disc), expand_dist / robot_size up to and across the
side of the node-grid window k_level_sample can stage, sample_num across the `multi` resolve variant and the level
kernels' limit, the collision and height thresholds -- and what the oracle must show on each of them before a GPU test
may rest on it (tests/test_param_cases_cpu.py).  Test code only; nothing here needs a GPU.

Every parameter a case does not name is oracle_api.MOUNTAIN's; the sampler is seed 7, table bits 16.
"""
from collections import namedtuple

import numpy as np

SEED, TABLE_BITS = 7, 16

# name -> (arguments of trg_planner.synth.mountain_cloud, start pose)
CLOUDS = {
    "dense8m": (dict(nx=160, ny=160, seed=8, spacing=0.05, jitter=0.01, amplitude=2.0, wavelength=15.0), [4.0, 4.0, 0.0]),
    "mid12m": (dict(nx=120, ny=120, seed=8, amplitude=2.0, wavelength=15.0), [6.0, 6.0, 0.0]),
    "rough12m": (dict(nx=120, ny=120, seed=11, amplitude=5.0, wavelength=14.0), [6.0, 6.0, 0.0]),
    "gentle12m": (dict(nx=120, ny=120, seed=5), [6.0, 6.0, 0.0]),
    "sparse15m": (dict(nx=60, ny=60, seed=8, spacing=0.25, jitter=0.05, amplitude=2.0, wavelength=15.0), [7.5, 7.5, 0.0]),
}

Case = namedtuple("Case", "name cloud overrides V exact")
# V: nodes on the oracle alone when the case was chosen; the witness must keep at least half of them after cleanGraph.
# exact: None, or (V before cleanGraph, V after it) that the witness must show exactly.


def _c(name, cloud, V, exact=None, **overrides):
    return Case(name, cloud, overrides, V, exact)


CASES = [
    # robot_size: discs of a handful of points ... discs over the LDS capacities of the disc query (SHCAP = 256 hits)
    _c("r015", "mid12m", 3289, robot_size=0.15, expand_dist=0.3),
    _c("r010", "mid12m", 6473, robot_size=0.1, expand_dist=0.2),
    _c("r045_dense", "dense8m", 213, robot_size=0.45, expand_dist=0.6),
    _c("r05_dense", "dense8m", 147, robot_size=0.5, expand_dist=1.0),
    _c("r06_dense", "dense8m", 93, robot_size=0.6, expand_dist=1.2),
    _c("r05_mid", "mid12m", 296, robot_size=0.5, expand_dist=1.0),
    _c("r05_sparse", "sparse15m", 418, robot_size=0.5, expand_dist=1.0),
    _c("r06_sparse", "sparse15m", 276, robot_size=0.6, expand_dist=1.2),
    # expand_dist / robot_size: the lowest that builds, below it, the last window the level kernels stage, beyond it
    _c("ratio_1", "mid12m", 1096, robot_size=0.3, expand_dist=0.3),
    _c("ratio_1_03", "mid12m", 1283, robot_size=0.3, expand_dist=0.31),
    _c("ratio_below_1", "mid12m", 1, exact=(1, 0), robot_size=0.3, expand_dist=0.25),
    _c("ratio_2_97_rough", "rough12m", 571, robot_size=0.3, expand_dist=0.89),
    _c("ratio_2_97_gentle", "gentle12m", 897, robot_size=0.3, expand_dist=0.89),
    _c("ratio_2_95_rough", "rough12m", 1886, robot_size=0.2, expand_dist=0.59),
    _c("ratio_2_95_gentle", "gentle12m", 1988, robot_size=0.2, expand_dist=0.59),
    _c("ratio_3_0", "rough12m", 640, robot_size=0.3, expand_dist=0.9),
    _c("ratio_3_05", "rough12m", 1842, robot_size=0.2, expand_dist=0.61),
    # sample_num: tiny graphs, either side of the `multi` resolve variant (> 32), beyond the level kernels' 64
    _c("s1", "rough12m", 3, exact=(3, 3), sample_num=1),
    _c("s2", "rough12m", 96, sample_num=2),
    _c("s32", "rough12m", 844, sample_num=32),
    _c("s33", "rough12m", 886, sample_num=33),
    _c("s65", "rough12m", 957, sample_num=65),
    # thresholds
    _c("ct0", "rough12m", 393, collision_threshold=0.0),
    _c("ct05", "rough12m", 712, collision_threshold=0.5),
    _c("ct1", "rough12m", 712, collision_threshold=1.0),
    _c("ht005_rough", "rough12m", 4, exact=(5, 4), height_threshold=0.05),
    _c("ht005_gentle", "gentle12m", 408, height_threshold=0.05),
    _c("ht05", "rough12m", 865, height_threshold=0.5),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]

DECLINED = ("ratio_3_0", "ratio_3_05", "s65")  # the device path must decline these; the host replay answers
DECLINE_REASON = "outside the level kernels' range"
KNOWN_START_DISC = ("r045_dense", "r015", "ratio_2_97_rough", "ratio_2_97_gentle", "s33")  # also built with the option 0 and 1
EMPTY = "ratio_below_1"  # one node before cleanGraph, none after
STEP3_BOUNDARY = {"r045_dense": False, "ratio_1": True}  # expandGraph's step 3 (trg.cpp:429), decided on a rounding edge

# disc counts (map points within robot_size of 400 random queries, DISC_SEED) a seam case is kept for
SHCAP, HCAP = 256, 1024
# the seed is part of the seam cases: on mid12m about one position in 200 has a 0.1 m disc of five points, and r010 is
# kept for queries of one to four; these 400 hold none (the build itself meets whatever the terrain holds)
DISC_SEED, DISC_QUERIES = 6, 400

# one set_local_map / update_graph step after the build: name -> (pose, (box x, box y, box half side))
UPDATES = {
    "r015": ((5.0, 5.5), (5.6, 5.9, 0.3)),
    "r05_mid": ((5.0, 5.5), (6.5, 6.5, 0.8)),
    "r045_dense": ((3.5, 3.5), (4.8, 4.6, 0.7)),
    "ratio_1": ((5.0, 5.5), (6.0, 6.2, 0.5)),
}

# plan(): two fixed pose pairs per cloud, start (x, y) -> goal (x, y, z)
PLANS = {
    "dense8m": (((1.5, 1.5), (6.5, 6.0, 0.0)), ((6.0, 2.0), (2.0, 6.5, 0.0))),
    "mid12m": (((2.0, 2.0), (10.0, 9.5, 0.0)), ((9.5, 2.5), (3.0, 10.0, 0.0))),
    "rough12m": (((4.5, 4.5), (7.5, 7.0, 0.0)), ((7.0, 5.0), (5.0, 7.5, 0.0))),
    "gentle12m": (((2.0, 2.0), (10.0, 9.5, 0.0)), ((9.5, 2.5), (3.0, 10.0, 0.0))),
    "sparse15m": (((2.0, 2.0), (13.0, 12.5, 0.0)), ((12.5, 2.5), (3.0, 13.0, 0.0))),
}

# the query-only case at HCAP = 1024: robot_size on dense8m at which the disc counts straddle the capacity
# (pi r^2 / 0.05^2 = 1024 at r = 0.903); checked on the oracle in test_param_cases_cpu.py
# (its long edges are 3 robot_size = 2.7 m, 7 walk discs: 5 robot_size do not fit into the 8 m cloud)
HCAP_CASE = dict(cloud="dense8m", overrides=dict(robot_size=0.9, expand_dist=1.2), long_edge=3.0)

# ---- the level kernels' range, written out ("What the device path accepts") ------------------
# k_level_sample stages the node-grid cells within K cells of the expanded node, a window of 2 K + 1 cells a side,
# K = ceil(expand_dist * 2.01 / robot_size) + 1 in fp32; a workgroup of LSW = 4 waves stages side^2 <= 4 * 64 cells,
# so the side is at most 16.  sample_num is at most 64 (one slot of a 64-lane wave per sample).
LSW = 4
WIN_MAX = 16  # largest s with s * s <= LSW * 64
S_MAX = 64
assert WIN_MAX * WIN_MAX <= LSW * 64 < (WIN_MAX + 1) * (WIN_MAX + 1)


def window_side(prm):
    f = np.float32
    k = int(np.ceil(f(prm["expand_dist"]) * f(2.01) / f(prm["robot_size"]))) + 1
    return 2 * k + 1


def device_supported(prm):
    return 1 <= prm["sample_num"] <= S_MAX and window_side(prm) <= WIN_MAX


def params(oa, case):
    return dict(oa.MOUNTAIN, **case.overrides)


_clouds = {}


def cloud(synth, name):
    """-> (points, start pose), made once per process."""
    if name not in _clouds:
        args, start = CLOUDS[name]
        a = dict(args)
        _clouds[name] = (synth.mountain_cloud(a.pop("nx"), a.pop("ny"), **a), start)
    return _clouds[name]


def disc_queries(points, robot_size):
    """DISC_QUERIES seeded positions whose robot_size disc lies inside the cloud."""
    lo = points[:, :2].min(axis=0) + robot_size
    hi = points[:, :2].max(axis=0) - robot_size
    return np.random.default_rng(DISC_SEED).uniform(lo, hi, size=(DISC_QUERIES, 2)).astype(np.float32)


def edge_pairs(points, prm, nearest_z, long_edge=5.0):
    """40 endpoint pairs as in test_gpu_edge_cases.test_zero_length_and_long_edges: 10 of zero length, 20 of lengths up
    to expand_dist + robot_size (the longest edge a build tries), 10 of long_edge robot_size (the general walk path).
    nearest_z: the elevation lookup of whoever is asked (engine and oracle agree bit for bit, tested beside)."""
    ed, rs = prm["expand_dist"], prm["robot_size"]
    reach = max(ed + rs, long_edge * rs)
    lo = points[:, :2].min(axis=0) + reach
    hi = points[:, :2].max(axis=0) - reach
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.uniform(lo, hi, (40, 2)), np.zeros((40, 1))], 1).astype(np.float32)
    p[:, 2] = nearest_z(p[:, :2])
    q = p.copy()
    ang = rng.uniform(0, 2 * np.pi, 30)
    length = np.concatenate([rng.uniform(0.05 * rs, ed + rs, 20), np.full(10, long_edge * rs)])
    q[10:, 0] += (length * np.cos(ang)).astype(np.float32)
    q[10:, 1] += (length * np.sin(ang)).astype(np.float32)
    q[10:, 2] = nearest_z(q[10:, :2])
    return p, q


def make_oracle(oa, prm, points, f64=True):
    o = oa.Oracle(**prm)
    o.set_sampler(SEED, 0, TABLE_BITS)
    o.set_cov_f64(f64)
    o.set_global_map(points)
    return o
