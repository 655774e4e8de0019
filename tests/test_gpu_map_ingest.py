"""GPU: the two ingest steps under everything else -- the voxel-grid filter (trg_voxel.hip) and the cell-sorted map
index (build_map, trg_kernels.hip) -- at the sizes, layouts and inputs the rest of the suite never gives them:
second trips of the grid-stride loops and of the scan's carry loop, row strides other than 3, every form of non-finite
input, the int32 boundary of the voxel index space, degenerate grids, and map clouds far from the origin.

The voxel filter must give the oracle's bits (tests/test_map_ingest_cpu.py pins the oracle at these inputs against a
float64 definition); the index must satisfy its definition (ingest_ref.index_definition) and answer queries as the
oracle does.  The clouds are ingest_ref.ingest_cases()."""
import numpy as np
import pytest

import ingest_ref as ir
from conftest import assert_graph_equal, weight_report

pytestmark = pytest.mark.gpu

CASES = ir.ingest_cases()
VOX, IDX = CASES["voxel"], CASES["index"]
WEIGHT_TOL = 1e-5
INVALID_ARG = 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def eng(oa):
    """one engine for every voxel case, in the order the file runs them"""
    import trg_planner
    return trg_planner.Engine(**oa.MOUNTAIN)


def _filter_like_oracle(oa, eng, name, given=None):
    """the case's cloud through the engine (as `given`, when it is passed in another layout) and through the oracle:
    equal as uint32, all rows"""
    case = VOX[name]
    pts = case.make()
    out = eng.voxel_filter(pts if given is None else given, case.leaf)
    ref, passthrough = oa.voxel_grid(pts, case.leaf)
    assert passthrough == case.passthrough
    assert out.dtype == np.float32 and out.ndim == 2 and out.shape == ref.shape, (out.shape, ref.shape)
    assert np.array_equal(_bits(out), _bits(ref)), int((_bits(out) != _bits(ref)).any(axis=1).sum())
    if passthrough:
        assert np.array_equal(_bits(out), _bits(pts))
    return pts, out


# ---- voxel filter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ir.VOXEL_SIZES)
def test_voxel_exact_sizes(oa, eng, n):
    """block edges (64, 256), the scan's tile (2048) and two tiles (4096), each with its neighbours"""
    pts, out = _filter_like_oracle(oa, eng, f"size_{n}")
    assert pts.shape[0] == n and 1 <= out.shape[0] <= n


def test_voxel_scan_second_trip(oa, eng):
    """258 tile sums: the carry loop of k_scan_tile_sums runs twice"""
    pts, out = _filter_like_oracle(oa, eng, "scan_second_trip")
    assert pts.shape[0] == 2048 * 257 + 1 and out.shape[0] == 12 ** 3


def test_voxel_grid_stride_second_trip(oa, eng):
    """more points than the 4096 x 256 threads of the capped grid, with NaN rows at both ends and on both sides of the
    first trip's last thread: k_vox_bounds, k_vox_keys, k_vox_heads and k_vox_starts step by the grid size"""
    pts, out = _filter_like_oracle(oa, eng, "stride_second_trip")
    assert pts.shape[0] == ir.SECOND_TRIP_N and 100000 < out.shape[0] < pts.shape[0] - 4


def test_voxel_copy_second_trip(oa, eng):
    """the same cloud at a leaf that overflows the index space: handed through by k_vox_copy, NaN rows included"""
    pts, out = _filter_like_oracle(oa, eng, "copy_second_trip")
    assert out.shape[0] == ir.SECOND_TRIP_N


@pytest.mark.parametrize("k", [4, 7])
def test_voxel_row_strides(oa, eng, k):
    """(N, 4) as x y z intensity and (N, 7): the columns past z hold NaN and 1e30"""
    pts = VOX["edge_cases_5000"].make()
    wide = ir.with_stride(pts, k)
    assert wide.shape == (5000, k)
    _, out = _filter_like_oracle(oa, eng, "edge_cases_5000", given=wide)
    assert np.isfinite(out).all() and np.abs(out).max() <= 5.0
    # the flat layout of before still means packed triples
    assert np.array_equal(_bits(eng.voxel_filter(pts.ravel(), 0.5)), _bits(out))


def test_voxel_nonfinite_forms(oa, eng):
    """+Inf in x only, -Inf in z only, NaN in y only, NaN with the sign bit set, a bad point first and last"""
    pts, out = _filter_like_oracle(oa, eng, "nonfinite_forms")
    assert np.isfinite(out).all()
    # ... and by the numpy definition: one row per voxel of the finite points
    _, key = ir.voxel_keys(pts, 0.5)
    assert out.shape[0] == np.unique(key).size


def test_voxel_all_nonfinite_then_a_good_cloud(oa, eng):
    pts = VOX["all_nonfinite"].make()
    out = eng.voxel_filter(pts, 0.5)
    assert out.shape == (0, 3) and out.dtype == np.float32
    assert oa.voxel_grid(pts, 0.5)[0].shape == (0, 3)
    _filter_like_oracle(oa, eng, "size_4097")


def test_voxel_occupancy_extremes(oa, eng):
    pts, out = _filter_like_oracle(oa, eng, "one_voxel")            # one sequential sum of 5000 terms
    assert out.shape == (1, 3)
    pts, out = _filter_like_oracle(oa, eng, "one_per_voxel")        # the input, reordered by voxel index
    _, key = ir.voxel_keys(pts, 1.0)
    assert np.unique(key).size == 4096
    assert np.array_equal(_bits(out), _bits(pts[np.argsort(key, kind="stable")]))
    pts, out = _filter_like_oracle(oa, eng, "far_shift")            # floor of negatives, 1 mm fp32 spacing
    assert 4000 < out.shape[0] < 5000


def test_voxel_int32_boundary(oa, eng):
    """leaf 1.0 (1 / leaf exact): 1290^3 <= INT32_MAX is filtered, and the far corner's voxel, whose key's high word
    is 1290^3 - 1, is the last segment with four members; 1291^3 is handed through"""
    pts, out = _filter_like_oracle(oa, eng, "int32_filtered")
    _, key = ir.voxel_keys(pts, 1.0)
    assert key.max() == 1290 ** 3 - 1 and out.shape[0] == np.unique(key).size == pts.shape[0] - 3
    want, counts, _ = ir.voxel_centroids64(pts, 1.0)
    assert counts[-1] == 4 and np.all(np.floor(out[-1]) == 1289.0)
    assert np.abs(out[-1] - want[-1]).max() <= 5 * ir.U24 * 1289.5
    pts, out = _filter_like_oracle(oa, eng, "int32_passthrough")
    assert out.shape == pts.shape


# ---- map index -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def idx_eng(oa):
    """one engine for every grid shape: its index arrays and build scratch are reused from cloud to cloud"""
    import trg_planner
    return trg_planner.Engine(**oa.MOUNTAIN)


def _index_of(e, cloud):
    e.set_global_map(cloud)
    return e.map_index("global", cloud.shape[0])


def _assert_same_index(a, b):
    for u, v in zip(a[:4], b[:4]):
        assert u.dtype == v.dtype and np.array_equal(u.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(a[4], b[4]) and np.array_equal(_bits(a[5]), _bits(b[5]))


@pytest.mark.parametrize("name", list(IDX))
def test_index_grid_shapes(oa, idx_eng, monkeypatch, name):
    """the build through bins and the direct build (TRG_INDEX_DIRECT) both satisfy the definition and agree"""
    case = IDX[name]
    cloud = case.make()
    monkeypatch.delenv("TRG_INDEX_DIRECT", raising=False)
    a = _index_of(idx_eng, cloud)
    monkeypatch.setenv("TRG_INDEX_DIRECT", "1")
    b = _index_of(idx_eng, cloud)
    monkeypatch.delenv("TRG_INDEX_DIRECT", raising=False)
    for got, want in zip(a[4], case.wh):
        assert want is None or got == want, (name, a[4])
    assert a[5][2] == np.float32(oa.MOUNTAIN["robot_size"])
    ir.index_definition(cloud, *a)
    ir.index_definition(cloud, *b)
    _assert_same_index(a, b)


def _edge_pairs(cloud, oracle, m, seed, dmax):
    """as _edge_pairs of tests/test_gpu_parity.py"""
    rng = np.random.default_rng(seed)
    lo = cloud[:, :2].min(0) + 1.0
    hi = cloud[:, :2].max(0) - 1.0
    a = rng.uniform(lo, hi, size=(m, 2)).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, m)
    d = rng.uniform(0.05, dmax, m)
    b = (a + np.stack([d * np.cos(ang), d * np.sin(ang)], 1)).astype(np.float32)
    za = oracle.nearest_z(a)
    zb = oracle.nearest_z(b)
    return np.concatenate([a, za[:, None]], 1), np.concatenate([b, zb[:, None]], 1)


def _pair(oa, cloud, **over):
    import trg_planner
    prm = dict(oa.MOUNTAIN, **over)
    e = trg_planner.Engine(**prm)
    e.set_global_map(cloud)
    o = oa.Oracle(**prm)
    o.set_global_map(cloud)
    return e, o, prm


@pytest.mark.parametrize("origin", list(ir.ORIGINS))
def test_index_origins_and_strides(oa, origin):
    cloud = CASES["origin"][origin]()
    e, o, prm = _pair(oa, cloud)
    a = e.map_index("global", cloud.shape[0])
    ir.index_definition(cloud, *a)
    for k in (4, 7):
        _assert_same_index(a, _index_of(e, ir.with_stride(cloud, k)))      # (the queries below read the last build)
    xy = ir.boundary_probes(cloud, 1024, 5)
    lo, hi = cloud[:, :2].min(0), cloud[:, :2].max(0)
    assert ((xy < lo) | (xy > hi)).any(axis=1).sum() == 256
    fe, ce, ne = e.is_collision(xy, threshold=prm["collision_threshold"])
    fo, co, no = o.is_collision(xy, 0, prm["collision_threshold"])
    assert np.array_equal(ne, no) and np.array_equal(ce, co) and np.array_equal(fe, fo)
    assert (no == 0).any() and (fo == 0).any() and (fo == 1).any()  # empty discs, free, blocked
    assert np.array_equal(_bits(e.nearest_z(xy)), _bits(o.nearest_z(xy)))
    # this terrain is gentle: nearly no disc holds a point 0.16 m off its median, so the blocked discs above are the
    # empty ones.  A second pair with a height threshold of 7 cm counts points in a third of the discs (by the oracle:
    # about 240 discs blocked by their points, about 140 free with points counted).
    e2, o2, prm2 = _pair(oa, cloud, height_threshold=0.07)
    fe, ce, ne = e2.is_collision(xy, threshold=prm2["collision_threshold"])
    fo, co, no = o2.is_collision(xy, 0, prm2["collision_threshold"])
    assert np.array_equal(ne, no) and np.array_equal(ce, co) and np.array_equal(fe, fo)
    assert ((fo == 1) & (no > 0)).sum() > 50 and ((fo == 0) & (co > 0)).sum() > 50
    # edges
    p1, p2 = _edge_pairs(cloud, o, 256, 3, 2.4 * prm["expand_dist"])
    se, npe, we, de = e.edge_risk(p1, p2)
    so, npo, wo, do = o.edge_risk(p1, p2)
    assert np.array_equal(_bits(de), _bits(do)) and np.array_equal(se, so)
    ok = so == 0
    assert ok.sum() > 100 and np.array_equal(npe[ok], npo[ok])
    flips, others, mx = weight_report(we[ok], wo[ok], WEIGHT_TOL)
    assert others == 0 and flips == 0, (flips, others, mx)


@pytest.mark.parametrize("origin", list(ir.ORIGINS))
def test_init_graph_on_each_origin(oa, origin):
    """One build from the cloud's centre.  At the far origin the fp32 spacing of the coordinates is about 1 mm, so
    nearest map points can tie; every tie must be resolved on the device path.  (The origin is the one first given,
    (4096.5, -8191.25): this build of 918 nodes meets no tie there, map_nn_resolved == map_nn_unresolved == 0; ties
    themselves are the subject of test_gpu_map_ties.py and test_gpu_tie_repairs.py.)"""
    import trg_planner
    cloud = CASES["origin"][origin]()
    prm = dict(oa.MOUNTAIN, sample_num=9)
    c = (cloud[:, :2].min(0).astype(np.float64) + cloud[:, :2].max(0)) / 2
    start = [float(c[0]), float(c[1]), 0.0]
    e = trg_planner.Engine(**prm)
    e.set_sampler(7, 16)
    e.set_option("replay", "device")
    e.set_option("keep_preclean", 1)
    e.set_global_map(cloud)
    e.init_graph(start)
    o = oa.Oracle(**prm)
    o.set_sampler(7, 0, 16)
    o.set_global_map(cloud)
    assert o.init_graph(start)
    st = e.stats()
    print(origin, {k: st[k] for k in ("map_nn_resolved", "map_nn_unresolved", "used_device_bfs", "bfs_fallbacks")})
    assert o.graph(1).V > 500
    assert_graph_equal(e.graph("preclean"), o.graph(1), weight_tol=WEIGHT_TOL, max_clamp_flips=0)
    assert_graph_equal(e.graph("global"), o.graph(0), weight_tol=WEIGHT_TOL, max_clamp_flips=0)
    assert st["map_nn_unresolved"] == 0 and st["used_device_bfs"] == 1, (st, e.fallback_reason)


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_map_with_a_non_finite_x_or_y_is_refused(oa):
    """one +Inf, -Inf, NaN or sign-bit NaN in x or y, first or last point: TRG_ERR_INVALID_ARG; then a good cloud"""
    import trg_planner
    from trg_planner._engine import TrgError
    good = IDX["n_8193"].make()
    e = trg_planner.Engine(**oa.MOUNTAIN)
    for bad in (np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan), ir.NEG_NAN):
        for axis in (0, 1):
            for at in (0, good.shape[0] - 1):
                cloud = good.copy()
                cloud[at, axis] = bad
                assert cloud.view(np.uint32)[at, axis] == np.array([bad]).view(np.uint32)[0]
                with pytest.raises(TrgError) as err:
                    e.set_global_map(cloud)
                assert err.value.status == INVALID_ARG and "non-finite" in str(err.value), (bad, axis, at, err.value)
    a = _index_of(e, good)
    ir.index_definition(good, *a)
    o = oa.Oracle(**oa.MOUNTAIN)
    o.set_global_map(good)
    xy = ir.boundary_probes(good, 64, 6)
    for u, v in zip(e.is_collision(xy, threshold=0.1), o.is_collision(xy, 0, 0.1)):
        assert np.array_equal(u, v)
    assert np.array_equal(_bits(e.nearest_z(xy)), _bits(o.nearest_z(xy)))
