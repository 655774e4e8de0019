"""Test data: clouds on which the nearest-map-point tie-break (map_nn_exact) works past the sizes
the rest of the suite reaches -- more tied points than one page of k_map_tied_set lists, a tie on every accepted sample
of a level, insertion trees as deep as the cloud is long -- and what the oracle must show on each of them before a GPU
test may rest on it (tests/test_map_tie_cases_cpu.py).  Test code only; nothing here needs a GPU.

Every tie comes from points with identical (x, y) or from a lattice with power-of-two spacing, so that it does not
depend on how a compiler contracts dx * dx + dy * dy.
"""
import numpy as np

F = np.float32
STEP = 2.0 ** -3            # lattice spacing of the copies cases
LATTICE_N = 96              # 9216 points: the insertion tree reaches below the 8192 points the host walks
SITES = 40
K_COPIES = (2, 15, 16, 17, 18, 33, 100)   # one page of the tied set holds 16


def tied_indices(cloud, q):
    """Cloud indices at the minimal fp32 squared distance from q, computed as the kd-tree does (no contraction)."""
    dx = cloud[:, 0] - F(q[0])
    dy = cloud[:, 1] - F(q[1])
    d2 = dx * dx + dy * dy
    assert d2.dtype == np.float32
    return np.flatnonzero(d2 == d2.min())


def lowest_index_z(cloud, queries):
    """The elevation an engine that breaks no tie would give: the z of the tied point with the lowest cloud index."""
    return np.asarray([cloud[tied_indices(cloud, q)[0], 2] for q in queries], F)


def lattice(n, step, seed):
    """n x n lattice, random z, in shuffled order (the insertion tree's shape depends on the order)."""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    xyz = np.stack([ii.ravel() * step, jj.ravel() * step, rng.uniform(0, 1, n * n)], 1).astype(F)
    return xyz[rng.permutation(n * n)]


def copies_case(K, n=LATTICE_N, sites=SITES):
    """A shuffled lattice plus `sites` positions inside lattice cells that hold K points each, same (x, y), K different
    z, shuffled in.  -> (cloud, one query next to every site: exactly its K copies tie)."""
    rng = np.random.default_rng(1000 + K)
    base = lattice(n, STEP, 50 + K)
    cells = rng.choice((n - 2) * (n - 2), sites, replace=False)
    ci, cj = 1 + cells // (n - 2), 1 + cells % (n - 2)
    sx, sy = (ci + 0.25) * STEP, (cj + 0.5) * STEP          # multiples of 2^-5: exact
    extra = np.empty((sites, K, 3), F)
    extra[:, :, 0] = sx[:, None]
    extra[:, :, 1] = sy[:, None]
    for s in range(sites):
        extra[s, :, 2] = 2.0 + s + rng.permutation(K) * 2.0 ** -8   # K different elevations
    cloud = np.concatenate([base, extra.reshape(-1, 3)])
    cloud = cloud[rng.permutation(cloud.shape[0])]
    # on either side of the site in x and in y: the copies split on one of the two, whichever their depth gives
    sign = rng.choice([-1.0, 1.0], (sites, 2))
    queries = np.stack([sx + sign[:, 0] * 2.0 ** -7, sy + sign[:, 1] * 2.0 ** -8], 1).astype(F)
    return cloud, queries


MIXED_COPIES, MIXED_CELLS = 5, 12


def mixed_case(n=LATTICE_N):
    """The four corners of a lattice cell with MIXED_COPIES points each, asked at the cell's centre: 20 tied points at
    4 positions, so the walk decides left / right between positions as well as between copies.  MIXED_CELLS cells."""
    rng = np.random.default_rng(77)
    base = lattice(n, STEP, 78)
    cells = [(7 * k + 3, (11 * k + 5) % (n - 4) + 1) for k in range(MIXED_CELLS)]   # far apart from one another
    extra = []
    for i, j in cells:
        for a, b in ((i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1)):
            for c in range(MIXED_COPIES - 1):
                extra.append([a * STEP, b * STEP, 3.0 + len(extra) * 2.0 ** -6])
    cloud = np.concatenate([base, np.asarray(extra, F)])
    cloud = cloud[rng.permutation(cloud.shape[0])]
    queries = np.asarray([[(i + 0.5) * STEP, (j + 0.5) * STEP] for i, j in cells], F)
    return cloud, queries


# ---- staircases: a cloud in sorted order makes the insertion tree a chain ---------------------------------------
STAIR_STEP = 2.0 ** -7
STAIR_N = 12400
TOP = 8192                  # points of the host-side top of the tree (MAP_TOP_POINTS)
LAUNCH = 64                 # levels one launch of k_region_walk_block descends
OLD_LAUNCHES = 64           # launches the walk was limited to before it followed the tree to its end
# the depth of each twinned point, i.e. of the tied pair's lowest common ancestor, by boundary of the walk
STAIR_GROUPS = {
    "host": (100, TOP - 1),
    "first_device_step": (TOP,),
    "first_launch_boundary": (TOP + LAUNCH - 1, TOP + LAUNCH, TOP + LAUNCH + 1),
    "old_limit": (TOP + LAUNCH * OLD_LAUNCHES - 1, TOP + LAUNCH * OLD_LAUNCHES, TOP + LAUNCH * OLD_LAUNCHES + 1),
    "last_point": (STAIR_N - 1,),
}
STAIR_P = tuple(p for g in STAIR_GROUPS.values() for p in g)
STAIR_TRIPLES = (100, TOP + LAUNCH)       # twinned twice: three points tie, one of them decided on each side of TOP


def staircase(descending=False, n=STAIR_N, twins=STAIR_P, triples=STAIR_TRIPLES):
    """Points (c_i, c_i, z_i) with c_i = i * 2^-7 ascending (every point goes right of every earlier one) or descending
    (every point goes left): cloud point i is the tree's node at depth i.  A twin of every point in `twins` is appended
    (same x, y; z + 0.5), a second one (z + 1) for those in `triples`.
    -> (cloud, queries, owner): owner[k] is the twinned point query k is nearest to."""
    rng = np.random.default_rng(5 + int(descending))
    i = np.arange(n)
    c = ((n - 1 - i) if descending else i) * STAIR_STEP
    pts = np.stack([c, c, rng.uniform(0, 0.25, n)], 1).astype(F)
    extra = []
    for p in twins:
        extra.append(pts[p] + F([0, 0, 0.5]))
        if p in triples:
            extra.append(pts[p] + F([0, 0, 1.0]))
    cloud = np.concatenate([pts, np.asarray(extra, F).reshape(-1, 3)])
    queries, owner = [], []
    for p in twins:
        x, y = float(pts[p, 0]), float(pts[p, 1])
        on_split = (x, y + 2.0 ** -10) if p % 2 == 0 else (x + 2.0 ** -10, y)   # node p splits on axis p % 2
        for q in ((x + 2.0 ** -9, y + 2.0 ** -10), (x - 2.0 ** -9, y - 2.0 ** -10), on_split):
            queries.append(q)
            owner.append(p)
    return cloud, np.asarray(queries, F), np.asarray(owner)


def insertion_path(xy, k):
    """kd_insert restated (kdtree.c:179-198): the nodes point k passes on its way down the tree of the points before
    it, root first.  A node's child on one side is the first later point that takes the same turns, since points are
    inserted in cloud order into the first empty place they reach; `<` goes left, the axis alternates with the depth."""
    cand = np.arange(k)
    cols = (np.ascontiguousarray(xy[:k, 0]), np.ascontiguousarray(xy[:k, 1]))
    path, cur, axis = [], 0, 0
    while True:
        path.append(int(cur))
        split = xy[cur, axis]
        left = xy[k, axis] < split
        keep = (cols[axis][cand] < split) == left
        keep &= cand != cur
        cand = cand[keep]
        if cand.size == 0:
            return path
        cur = cand[0]
        axis ^= 1


def edge_cloud(n):
    """An ascending staircase of n - 1 points and a twin of its last point: n points, the last two tie.  n = 8191, 8192
    and 8193 lie either side of the host-side top of the tree."""
    cloud, queries, _ = staircase(n=n - 1, twins=(n - 2,), triples=())
    assert cloud.shape[0] == n
    return cloud, queries


# ---- ties the first pass of k_map_tied_set does not find ------------------------------------------------------------
def far_case():
    """A 16 x 16 lattice of spacing 1 (robot_size is 0.3).  Cell centres: 4 points tie at 0.707, found after the radius
    has doubled twice.  Points left of the map, level with the middle of a lattice edge: 2 points tie at about 40, found
    once the scan covers the whole grid."""
    cloud = lattice(16, 1.0, 9)
    inside = [[i + 0.5, j + 0.5] for i, j in ((2, 3), (7, 7), (12, 4), (5, 13))]
    outside = [[-40.0, 7.5], [-40.0, 2.5], [6.5, 60.0], [100.0, 11.5]]
    return cloud, np.asarray(inside, F), np.asarray(outside, F)


# ---- builds ---------------------------------------------------------------------------------------------------------
SEED, TABLE_BITS = 7, 16
RECORD_CAP = 256            # tie records a sampling launch kept before the lists were sized by its slots
TWIN_BUILD = dict(n=120, sample_num=16, start=[6.0, 6.0, 0.0])
COPIES_BUILD = dict(n=200, sample_num=7, start=[10.0, 10.0, 0.0], frac=0.03, copies=20)


def twinned_cloud(synth, n=TWIN_BUILD["n"]):
    """Every point has a twin at the same (x, y) with another z: every accepted sample ties."""
    base = synth.mountain_cloud(n, n, seed=3)
    rng = np.random.default_rng(3)
    twin = base.copy()
    twin[:, 2] += rng.uniform(0.01, 0.04, twin.shape[0]).astype(F)
    cloud = np.concatenate([base, twin])
    return cloud[rng.permutation(cloud.shape[0])]


def copies_cloud(synth, n=COPIES_BUILD["n"], frac=COPIES_BUILD["frac"], copies=COPIES_BUILD["copies"]):
    """3 % of the points carry 20 copies (same x, y; other z): more than a page of the tied set, inside a build.
    -> (cloud, mask of the points that have copies)"""
    base = synth.mountain_cloud(n, n, seed=5)
    rng = np.random.default_rng(5)
    pick = rng.choice(base.shape[0], int(frac * base.shape[0]), replace=False)
    dup = np.repeat(base[pick], copies - 1, axis=0)
    dup[:, 2] += rng.uniform(0.005, 0.04, dup.shape[0]).astype(F)
    cloud = np.concatenate([base, dup])
    many = np.zeros(cloud.shape[0], bool)
    many[pick] = True
    many[base.shape[0]:] = True
    order = rng.permutation(cloud.shape[0])
    return cloud[order], many[order]


def build_params(oa, which):
    return dict(oa.MOUNTAIN, sample_num=which["sample_num"])


def build_oracle(oa, which, cloud, trace=False):
    o = oa.Oracle(**build_params(oa, which))
    o.set_sampler(SEED, 0, TABLE_BITS)
    if trace:
        o.set_trace(True)
    o.set_global_map(cloud)
    assert o.init_graph(which["start"])
    return o


def expansion_levels(trace):
    """The BFS level of every created node (by creation id) from the oracle's wireEdge trace: a node is created by
    the first call that names it, one level below the node that call starts from."""
    level = {int(trace["src"][0]): 0}
    for s, d in zip(trace["src"].tolist(), trace["dst"].tolist()):
        if d not in level:
            level[d] = level[s] + 1
    return level
