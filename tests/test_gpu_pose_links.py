"""GPU: pose links (trg_engine_pose_links, Engine.pose_links, Engine.cost_fields_from_poses; DESIGN.md section 2,
"Pose links") on mountain_small and indoor_small, built as the parity tests build them.

64 poses per map from a seeded generator (tests/pose_cases.py): node positions themselves, edge midpoints, uniform
draws in the map's box, draws within robot_size of raised map points (indoor walls).  The reference is the plain loop
over all nodes with Engine.is_collision, nearest_z and edge_risk -- the existing probes, each pinned against the
oracle by tests/test_gpu_parity.py -- and everything is compared exactly: status, z bits, counts, link node order,
weight and dist bits.  For the first 8 poses the same loop runs over the oracle's own probes: status, z, counts, node
order and dist bits exactly, the weights within the 1e-5 at which the risk weight is pinned against the oracle.
Before any comparison the test asserts that the reference shows what the generator's seed was chosen for."""
import numpy as np
import pytest

import pose_cases as pc

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID_ARG, NO_MAP, NO_GRAPH = 1, 2, 5
WEIGHT_TOL = 1e-5


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module", params=sorted(pc.MAPS))
def built(request, oa):
    """(name, parameters, cloud, engine, oracle, the engine's graph, poses, reference) once per map."""
    import trg_planner
    name = request.param
    pname, start, seed, _ = pc.MAPS[name]
    prm = dict(getattr(oa, pname))
    cloud = request.getfixturevalue(name)
    e = trg_planner.Engine(**prm)
    e.set_sampler(7, 16)
    e.set_global_map(cloud)
    e.init_graph(start)
    o = oa.Oracle(**prm)
    o.set_sampler(7, 0, 16)
    o.set_global_map(cloud)
    assert o.init_graph(start)
    g = e.graph("global")
    xy = pc.poses(cloud, g, seed, prm["robot_size"])
    ref = pc.reference(e, g, xy, prm["expand_dist"], prm["collision_threshold"])
    yield name, prm, cloud, e, o, g, xy, ref
    e.close()


def _same(got, want, at, cap=None):
    assert got["status"] == want["status"], at + f"status {got['status']} != {want['status']}"
    assert _bits(got["z"]) == _bits(want["z"]), at + f"z {got['z']!r} != {want['z']!r}"
    assert got["n_candidates"] == want["n_candidates"] and got["n_links"] == want["n_links"], at + (
        f"counts {got['n_candidates']}, {got['n_links']} != {want['n_candidates']}, {want['n_links']}")
    n = want["n_links"] if cap is None else min(cap, want["n_links"])
    assert np.array_equal(got["nodes"], want["nodes"][:n]), at + f"nodes {got['nodes']} != {want['nodes'][:n]}"
    assert np.array_equal(_bits(got["weight"]), _bits(want["weight"][:n])), at + "weight bits"
    assert np.array_equal(_bits(got["dist"]), _bits(want["dist"][:n])), at + "dist bits"


def test_the_reference_shows_what_the_seed_was_chosen_for(built):
    name, _, _, _, _, g, xy, ref = built
    assert xy.shape == (pc.N_POSES, 2) and g.V > 200
    shown = pc.conditions(ref)
    missing = [k for k, v in shown.items() if not v]
    assert sorted(missing) == sorted(pc.MAPS[name][3]), (name, shown)


def test_links_equal_the_plain_loop(built):
    name, prm, _, e, _, g, xy, ref = built
    got = e.pose_links(xy, cap=64)
    assert len(got) == len(ref) and max(r["n_links"] for r in ref) <= 64
    for k, (a, b) in enumerate(zip(got, ref)):
        _same(a, b, f"{name}, pose {k} {xy[k].tolist()}: ")
        sf = F32(prm["safety_factor"])
        assert np.array_equal(_bits(a["cost"]), _bits((sf * b["weight"] + F32(1)) * b["dist"])), f"{name}, pose {k}: cost"
    # a radius of its own, and one pose alone
    wide = F32(2.4 * prm["expand_dist"])
    ref_wide = pc.reference(e, g, xy[:12], wide, prm["collision_threshold"])
    for k, (a, b) in enumerate(zip(e.pose_links(xy[:12], radius=wide, cap=256), ref_wide)):
        _same(a, b, f"{name}, radius {wide}, pose {k}: ")
    assert any(b["n_candidates"] > r["n_candidates"] for b, r in zip(ref_wide, ref))
    k = next(k for k, r in enumerate(ref) if r["n_links"] >= 3)
    _same(e.pose_links(xy[k:k + 1], cap=64)[0], ref[k], f"{name}, pose {k} alone: ")


def test_first_poses_against_the_oracle(built):
    name, prm, _, e, o, g, xy, _ = built
    # the first 8 poses (node positions) and two more of each other kind of the generator
    pick = np.concatenate([np.arange(8)] + [np.arange(i * (pc.N_POSES // 4), i * (pc.N_POSES // 4) + 2) for i in (1, 2, 3)])
    got = e.pose_links(xy[pick], cap=64)
    want = pc.reference(pc.OracleProbes(o), g, xy[pick], prm["expand_dist"], prm["collision_threshold"])
    for k, (a, b) in enumerate(zip(got, want)):
        at = f"{name}, pose {pick[k]} against the oracle: "
        assert a["status"] == b["status"] and _bits(a["z"]) == _bits(b["z"]), at
        assert a["n_candidates"] == b["n_candidates"] and a["n_links"] == b["n_links"], at
        assert np.array_equal(a["nodes"], b["nodes"]) and np.array_equal(_bits(a["dist"]), _bits(b["dist"])), at
        assert np.all(np.abs(a["weight"] - b["weight"]) <= WEIGHT_TOL), at + "weights"


def test_cap_and_empty_call(built):
    name, _, _, e, _, _, xy, ref = built
    k = next(k for k, r in enumerate(ref) if r["n_links"] >= 3)
    for cap in (2, 1, 0):
        got = e.pose_links(xy, cap=cap)
        for j, (a, b) in enumerate(zip(got, ref)):
            _same(a, b, f"{name}, cap {cap}, pose {j}: ", cap=cap)
        assert got[k]["nodes"].size == cap and got[k]["n_links"] == ref[k]["n_links"]
    assert e.pose_links(np.empty((0, 2), F32)) == []
    # counts alone: every link array may be NULL
    import ctypes as C
    from trg_planner._engine import TrgPoseInfo, _f
    infos = (TrgPoseInfo * len(ref))()
    st = e.L.trg_engine_pose_links(e.h, _f(xy), len(ref), C.c_float(e.params.expand_dist), 4, None, None, None, infos)
    assert st == 0 and [i.n_links for i in infos] == [r["n_links"] for r in ref]


def test_refusals(built):
    from trg_planner import TrgError
    name, prm, cloud, e, _, _, xy, _ = built
    import ctypes as C
    from trg_planner._engine import TrgPoseInfo, _f
    infos = (TrgPoseInfo * 4)()

    def raw(m, radius, cap, pts=xy):
        st = e.L.trg_engine_pose_links(e.h, _f(np.ascontiguousarray(pts, F32)), m, C.c_float(radius), cap, None, None,
                                       None, infos)
        return st, e.L.trg_engine_last_error(e.h).decode()

    ed = prm["expand_dist"]
    assert raw(-1, ed, 4)[0] == INVALID_ARG and raw(2, ed, -1)[0] == INVALID_ARG
    # wireEdge's bound is the double product 2.5 * expand_dist of the fp32 parameter: the first float32 at or above
    # it is refused, the one below it is taken
    bound = 2.5 * float(F32(ed))
    at = F32(bound) if float(F32(bound)) >= bound else np.nextafter(F32(bound), F32(np.inf))
    assert float(at) >= bound > float(np.nextafter(at, F32(0)))
    for radius in (np.nan, 0.0, -0.0, -1.0, at, np.inf):
        st, msg = raw(2, radius, 4)
        assert st == INVALID_ARG and "radius" in msg, (radius, msg)
    assert raw(2, np.nextafter(at, F32(0)), 4)[0] == 0
    assert raw(0, ed, 4)[0] == 0
    bad = xy[:4].copy()
    bad[2, 1] = np.nan
    st, msg = raw(4, ed, 4, bad)
    assert st == INVALID_ARG and "pose 2" in msg, msg
    with pytest.raises(TrgError) as err:
        e.pose_links(bad)
    assert err.value.status == INVALID_ARG
    # a position outside the map and the graph: an empty disc is a collision, so no candidates
    far = e.pose_links(cloud[:, :2].max(0)[None] + F32(20.0))[0]
    assert far["status"] == 1 and far["n_candidates"] == 0 and far["n_links"] == 0
    import trg_planner
    fresh = trg_planner.Engine(**prm)
    try:
        with pytest.raises(TrgError) as err:
            fresh.pose_links(xy[:2])
        assert err.value.status == NO_MAP
        fresh.set_global_map(cloud)
        with pytest.raises(TrgError) as err:
            fresh.pose_links(xy[:2])
        assert err.value.status == NO_GRAPH
    finally:
        fresh.close()


def test_fields_from_poses(built):
    """cost_fields_from_poses is the seeded solve of the poses' links; a pose in collision or without links is refused
    by name."""
    from trg_planner import TrgError
    name, prm, _, e, _, g, xy, ref = built
    good = [k for k, r in enumerate(ref) if r["n_links"] >= 2][:3]
    links = e.pose_links(xy[good])
    r = e.cost_fields_from_poses(xy[good], targets=[0, g.V - 1])
    s = e.cost_fields_seeded([one["nodes"] for one in links], [one["cost"] for one in links], targets=[0, g.V - 1])
    for key in ("cost", "cost_at"):
        assert np.array_equal(_bits(r[key]), _bits(s[key])), key
    for key in ("hops", "parent", "owner", "hops_at", "owner_at", "reached"):
        assert np.array_equal(r[key], s[key]), key
    assert [one["nodes"].tolist() for one in r["links"]] == [one["nodes"].tolist() for one in links]
    for i in range(len(good)):  # a link node is never dearer than its link, the nearest link need not be the entry
        assert np.all(r["cost"][i, links[i]["nodes"]] <= links[i]["cost"])
    blocked = next(k for k, one in enumerate(ref) if one["status"] == 1)
    with pytest.raises(TrgError) as err:
        e.cost_fields_from_poses(xy[[good[0], blocked]])
    assert err.value.status == INVALID_ARG and "pose 1" in str(err.value) and "collision" in str(err.value)
    lonely = [k for k, one in enumerate(ref) if one["status"] == 0 and one["n_links"] == 0]
    if "candidates but no links" not in pc.MAPS[name][3]:
        assert lonely
    if lonely:
        with pytest.raises(TrgError) as err:
            e.cost_fields_from_poses(xy[[lonely[0]]])
        assert err.value.status == INVALID_ARG and "pose 0" in str(err.value) and "no links" in str(err.value)
