"""CPU: the inputs of tests/test_gpu_map_ingest.py, checked without a GPU.

The GPU tests ask the engine's voxel filter for the oracle's bits.  That means something only if the oracle is right
at those inputs, so here the oracle's voxel_grid is compared with an independent float64 definition
(ingest_ref.voxel_centroids64), and the conditions the GPU cases rely on (which clouds are handed through, which hold
several points per voxel, which grid each index cloud gives) are asserted on the clouds themselves."""
import numpy as np
import pytest

import ingest_ref as ir

CASES = ir.ingest_cases()
ROBOT_SIZE = 0.3   # oracle_api.MOUNTAIN: the cell size of the index cases


@pytest.mark.parametrize("name", list(CASES["voxel"]))
def test_oracle_voxel_grid_against_float64_centroids(oa, name):
    """Same voxels in the same order; every coordinate within (count + 1) * 2^-24 * max|coordinate in the voxel|:
    a sequential fp32 sum of `count` terms has a relative error of (count - 1) * 2^-24 against the sum of the
    magnitudes (<= count * max), the division by the count brings that to (count - 1) * 2^-24 * max and adds one
    rounding, 2^-24 * max -- count * 2^-24 * max in all, and the last unit covers the second-order terms."""
    case = CASES["voxel"][name]
    pts = case.make()
    assert pts.dtype == np.float32 and pts.ndim == 2 and pts.shape[1] == 3
    out, passthrough = oa.voxel_grid(pts, case.leaf)
    finite = np.isfinite(pts).all(axis=1)
    assert passthrough == case.passthrough
    if finite.any():
        assert (ir.voxel_index_space(pts, case.leaf) > ir.INT32_MAX) == case.passthrough
    if case.passthrough:
        assert np.array_equal(out.view(np.uint32), pts.view(np.uint32))
        return
    if not finite.any():
        assert out.shape == (0, 3)
        return
    want, counts, big = ir.voxel_centroids64(pts, case.leaf)
    assert out.shape == want.shape
    assert counts.sum() == finite.sum()
    assert counts.max() > 1 or not case.multi      # (the cases meant to sum several points per voxel do)
    err = np.abs(out.astype(np.float64) - want)
    bound = (counts[:, None] + 1) * ir.U24 * big
    print(f"{name}: {out.shape[0]} voxels, largest count {counts.max()}, worst error / bound "
          f"{float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound), (int((err > bound).sum()), float((err - bound).max()))


def test_voxel_cases_hold_what_they_are_for():
    vox = CASES["voxel"]
    assert [vox[f"size_{n}"].make().shape[0] for n in ir.VOXEL_SIZES] == list(ir.VOXEL_SIZES)
    assert vox["scan_second_trip"].make().shape[0] == 2048 * 257 + 1
    big = vox["stride_second_trip"].make()
    n = big.shape[0]
    assert n == 4096 * 256 + 257 and vox["copy_second_trip"].make().shape[0] == n
    bad = np.flatnonzero(~np.isfinite(big).all(axis=1))
    assert bad.tolist() == [0, 4096 * 256 - 1, 4096 * 256, n - 1]
    # the forms of non-finite input, each in the coordinate it is meant for
    pts = vox["nonfinite_forms"].make()
    bits = pts.view(np.uint32)
    assert pts.shape == (2000, 3)
    assert np.isposinf(pts[:, 0]).any() and not np.isposinf(pts[:, 1:]).any()
    assert np.isneginf(pts[:, 2]).any() and not np.isneginf(pts[:, :2]).any()
    assert (bits[:, 1] == 0x7FC00000).any()                       # NaN in y only ...
    assert (np.isnan(pts[:, 1]) & np.isfinite(pts[:, 0]) & np.isfinite(pts[:, 2])).any()
    assert (bits == 0xFFC00000).any(axis=0).tolist() == [True, True, False]   # ... and with the sign bit set
    assert not np.isfinite(pts[0]).all() and not np.isfinite(pts[-1]).all()
    assert 1500 < np.isfinite(pts).all(axis=1).sum() < 2000
    none = vox["all_nonfinite"].make()
    assert not np.isfinite(none).all(axis=1).any() and (none.view(np.uint32) == 0xFFC00000).any()
    # occupancy extremes
    _, counts, _ = ir.voxel_centroids64(vox["one_voxel"].make(), 0.5)
    assert counts.tolist() == [5000]
    _, counts, _ = ir.voxel_centroids64(vox["one_per_voxel"].make(), 1.0)
    assert counts.shape == (4096,) and counts.max() == 1
    far = vox["far_shift"].make()
    assert far[:, 0].max() < -4090 and far[:, 1].min() > 8191 and far[:, 2].max() < -243
    assert ir.voxel_index_space(far, 0.2) < 40 ** 3
    # the int32 boundary: 1290^3 is the largest index space still filtered, 1291^3 the first handed through
    edge = vox["int32_filtered"].make()
    assert ir.voxel_index_space(edge, 1.0) == 1290 ** 3 <= ir.INT32_MAX < 1291 ** 3
    keep, key = ir.voxel_keys(edge, 1.0)
    assert key.max() == 1290 ** 3 - 1 and (key == key.max()).sum() == 4 and key.min() == 0
    assert ir.voxel_index_space(vox["int32_passthrough"].make(), 1.0) == 1291 ** 3


@pytest.mark.parametrize("name", list(CASES["index"]))
def test_index_cases_give_the_stated_grid(name):
    case = CASES["index"][name]
    cloud = case.make()
    assert cloud.dtype == np.float32 and cloud.ndim == 2 and cloud.shape[1] == 3 and np.isfinite(cloud).all()
    W, H = ir.index_wh(cloud, ROBOT_SIZE)
    for got, want in zip((W, H), case.wh):
        assert want is None or got == want, (name, W, H)
    n = cloud.shape[0]
    if name.startswith("line"):
        assert n == 3000 and max(W, H) > 100
    if name.startswith("n_"):
        assert n == int(name[2:])
        assert (n + 8191) // 8192 == (2 if n > 8192 else 1)       # nwg of index_bins_plan
    if name == "second_trip":
        assert n == 4096 * 256 + 257 and W * H > 100000
    if name == "two_identical":
        assert n == 2 and np.array_equal(cloud[0], cloud[1])


def test_origin_clouds_and_strides():
    for name, o in ir.ORIGINS.items():
        cloud = CASES["origin"][name]()
        assert cloud.shape == (14400, 3)
        assert abs(float(cloud[:, 0].min()) - o[0]) < 0.05 and abs(float(cloud[:, 1].min()) - o[1]) < 0.05
        W, H = ir.index_wh(cloud, ROBOT_SIZE)
        assert 39 <= W <= 41 and 39 <= H <= 41
        for k in (4, 7):
            wide = ir.with_stride(cloud, k)
            assert wide.shape == (14400, k) and wide.flags.c_contiguous
            assert np.array_equal(wide[:, :3].view(np.uint32), cloud.view(np.uint32))
            assert np.isnan(wide[:, 3]).all() and (k == 4 or (wide[:, 4] == np.float32(1e30)).all())


def test_index_definition_refuses_a_wrong_index():
    """the definition itself: it accepts the index built here by a stable sort and refuses single defects"""
    cloud = CASES["index"]["n_8193"].make()
    g = np.float32(ROBOT_SIZE)
    lo = cloud[:, :2].min(axis=0)
    W, H = ir.index_wh(cloud, g)
    inv_g = np.float32(1.0) / g
    cx = np.clip(np.floor((cloud[:, 0] - lo[0]) * inv_g), 0, W - 1).astype(np.int64)
    cy = np.clip(np.floor((cloud[:, 1] - lo[1]) * inv_g), 0, H - 1).astype(np.int64)
    perm = np.argsort(cy * W + cx, kind="stable").astype(np.int32)
    x, y, z = (np.ascontiguousarray(cloud[perm, k]) for k in range(3))
    wh, org = np.array([W, H], np.int32), np.array([lo[0], lo[1], g], np.float32)
    ir.index_definition(cloud, x, y, z, perm, wh, org)
    swapped = perm.copy()
    swapped[[0, -1]] = swapped[[-1, 0]]
    defects = [
        dict(perm=swapped, x=cloud[swapped, 0], y=cloud[swapped, 1], z=cloud[swapped, 2]),  # cells out of order
        dict(z=np.nextafter(z, np.float32(np.inf))),                                        # not the cloud's bits
        dict(wh=np.array([W + 1, H], np.int32)),
        dict(org=np.array([lo[0] - 1e-3, lo[1], g], np.float32)),
        dict(perm=np.where(perm == 5, 6, perm).astype(np.int32)),                           # not a permutation
    ]
    for d in defects:
        args = dict(x=x, y=y, z=z, perm=perm, wh=wh, org=org)
        args.update(d)
        with pytest.raises(AssertionError):
            ir.index_definition(cloud, **args)


def test_voxel_filter_argument_checks():
    """(N, k) needs k >= 3 and a flat array whole triples: refused before the engine is touched (there is none)"""
    from trg_planner import Engine
    for bad in (np.zeros((5, 2), np.float32), np.zeros((6, 1), np.float32), np.zeros(7, np.float32),
                np.zeros((2, 3, 3), np.float32), np.float32(1.0)):
        with pytest.raises(ValueError):
            Engine.voxel_filter(None, bad, 0.2)
    # what is accepted gets past the checks: the engine is the first thing it needs
    for good in (np.zeros((5, 3), np.float32), np.zeros((5, 4), np.float32), np.zeros(6, np.float32)):
        with pytest.raises(AttributeError):
            Engine.voxel_filter(None, good, 0.2)
