"""The cases of map_tie_cases.py on the oracle alone: every cloud a GPU test of the nearest-map-point tie-break rests
on still shows what it is kept for -- the number of tied points, the depth of the tree node that decides a tie, more
ties in one level than a sampling launch once recorded -- and an engine that left every tie at the lowest cloud index
would be wrong on a fixed share of the queries, so that no case can pass by luck.  Conditions, not measurements.
No GPU."""
import numpy as np
import pytest

import map_tie_cases as mc


def _oracle_z(oa, cloud, queries):
    o = oa.Oracle(**oa.MOUNTAIN)
    o.set_global_map(cloud)
    z = o.nearest_z(queries)
    o.close()
    return z


def _lowest_index_wrong(oa, cloud, queries):
    return int((mc.lowest_index_z(cloud, queries) != _oracle_z(oa, cloud, queries)).sum())


@pytest.mark.parametrize("K", mc.K_COPIES)
def test_copies_tie_exactly_and_the_lowest_index_is_often_wrong(oa, K):
    cloud, queries = mc.copies_case(K)
    assert cloud.shape[0] == mc.LATTICE_N ** 2 + mc.SITES * K > mc.TOP
    for q in queries:
        idx = mc.tied_indices(cloud, q)
        assert idx.size == K
        assert np.unique(cloud[idx, :2], axis=0).shape[0] == 1 and np.unique(cloud[idx, 2]).size == K
    wrong = _lowest_index_wrong(oa, cloud, queries)
    print("K", K, "lowest index wrong on", wrong, "of", len(queries))
    assert 4 * wrong >= len(queries)


def test_mixed_case_ties_twenty_points_at_four_positions(oa):
    cloud, queries = mc.mixed_case()
    for q in queries:
        idx = mc.tied_indices(cloud, q)
        assert idx.size == 4 * mc.MIXED_COPIES
        assert np.unique(cloud[idx, :2], axis=0).shape[0] == 4 and np.unique(cloud[idx, 2]).size == idx.size
    wrong = _lowest_index_wrong(oa, cloud, queries)
    print("lowest index wrong on", wrong, "of", len(queries))
    assert 4 * wrong >= len(queries)


@pytest.mark.parametrize("descending", [False, True])
def test_staircase_decides_each_tie_at_the_depth_of_the_twinned_point(oa, descending):
    cloud, queries, owner = mc.staircase(descending)
    assert cloud.shape[0] == mc.STAIR_N + len(mc.STAIR_P) + len(mc.STAIR_TRIPLES)
    # where each twin went: below its original, which sits at depth p
    k = mc.STAIR_N
    for p in mc.STAIR_P:
        for _ in range(2 if p in mc.STAIR_TRIPLES else 1):
            assert np.array_equal(cloud[k, :2], cloud[p, :2]) and cloud[k, 2] != cloud[p, 2]
            path = mc.insertion_path(cloud[:, :2], k)
            assert path[:p + 1] == list(range(p + 1)), (p, k)   # the lowest common ancestor is p itself, at depth p
            k += 1
    for q, p in zip(queries, owner):
        idx = mc.tied_indices(cloud, q)
        assert idx[0] == p and idx.size == (3 if p in mc.STAIR_TRIPLES else 2)
    on_split = queries[2::3]
    assert all(q[p % 2] == cloud[p, p % 2] for q, p in zip(on_split, owner[2::3]))
    zo = _oracle_z(oa, cloud, queries)
    wrong = mc.lowest_index_z(cloud, queries) != zo
    print("descending" if descending else "ascending", "lowest index wrong on", int(wrong.sum()), "of", len(queries),
          "by group", {g: int(wrong[np.isin(owner, ps)].sum()) for g, ps in mc.STAIR_GROUPS.items()})
    # one side of every split is the far side: there the later point is visited first
    for g, ps in mc.STAIR_GROUPS.items():
        assert wrong[np.isin(owner, ps)].any(), g
    assert 4 * int(wrong.sum()) >= len(queries)


def test_group_depths_sit_on_the_walk_s_boundaries():
    g = mc.STAIR_GROUPS
    assert g["host"][1] == mc.TOP - 1 and g["first_device_step"] == (mc.TOP,)
    assert g["first_launch_boundary"] == (8255, 8256, 8257)
    assert g["old_limit"] == (12287, 12288, 12289) and g["last_point"] == (mc.STAIR_N - 1,)
    assert set(mc.STAIR_TRIPLES) <= set(mc.STAIR_P) and min(mc.STAIR_TRIPLES) < mc.TOP < max(mc.STAIR_TRIPLES)


@pytest.mark.parametrize("n", [mc.TOP - 1, mc.TOP, mc.TOP + 1])
def test_edge_clouds_tie_their_last_two_points(oa, n):
    cloud, queries = mc.edge_cloud(n)
    for q in queries:
        assert mc.tied_indices(cloud, q).tolist() == [n - 2, n - 1]
    assert _lowest_index_wrong(oa, cloud, queries) >= 1


def test_far_case_ties_beyond_the_first_radius(oa):
    cloud, inside, outside = mc.far_case()
    r = oa.MOUNTAIN["robot_size"]
    for q in inside:
        idx = mc.tied_indices(cloud, q)
        assert idx.size == 4 and np.hypot(*(cloud[idx[0], :2] - q)) > 2 * r
    lo, hi = cloud[:, :2].min(axis=0), cloud[:, :2].max(axis=0)
    for q in outside:
        idx = mc.tied_indices(cloud, q)
        assert idx.size == 2 and ((q < lo) | (q > hi)).any()
        # no radius r * 2^k reaches the pair before its box covers the whole map
        d = float(np.hypot(*(cloud[idx[0], :2] - q).astype(np.float64)))
        R = r
        while R < d:
            R *= 2
        assert (q - R < lo).all() and (q + R > hi).all()
    both = np.concatenate([inside, outside])
    zo = _oracle_z(oa, cloud, both)
    wrong = mc.lowest_index_z(cloud, both) != zo
    print("lowest index wrong on", int(wrong[:len(inside)].sum()), "of", len(inside), "inside,",
          int(wrong[len(inside):].sum()), "of", len(outside), "outside")
    assert wrong[:len(inside)].any() and wrong[len(inside):].any()


def test_twinned_build_ties_more_than_the_old_record_cap_in_one_level(oa, synth):
    cloud = mc.twinned_cloud(synth)
    # every point has its twin: whatever point is nearest to a sample, a second one is at the same distance
    xy = np.ascontiguousarray(cloud[:, :2]).view(np.dtype((np.void, 8))).ravel()
    _, counts = np.unique(xy, return_counts=True)
    assert (counts == 2).all()
    o = mc.build_oracle(oa, mc.TWIN_BUILD, cloud, trace=True)
    c, V = o.counters(), o.graph(1).V
    level = mc.expansion_levels(o.trace())
    o.close()
    levels = max(level.values()) + 1
    print("V", V, "accepted samples", c["samples"], "levels", levels, "per level", c["samples"] / levels)
    assert len(level) == c["created"] and V > 800
    # every accepted sample is a tie record, and some level holds at least the mean
    assert c["samples"] > 2 * mc.RECORD_CAP * (levels + 2)


def test_copies_build_meets_sites_of_twenty(oa, synth):
    cloud, many = mc.copies_cloud(synth)
    xy = np.ascontiguousarray(cloud[many, :2]).view(np.dtype((np.void, 8))).ravel()
    _, counts = np.unique(xy, return_counts=True)
    assert (counts == mc.COPIES_BUILD["copies"]).all() and counts.size == int(0.03 * 200 * 200)
    o = mc.build_oracle(oa, mc.COPIES_BUILD, cloud)
    g = o.graph(1)
    o.close()
    # nodes whose elevation is that of a point with 20 copies (a node's z is its nearest point's)
    at_site = 0
    for k in range(0, g.V, 256):
        p = g.xyz[k:k + 256]
        d2 = (p[:, None, 0] - cloud[None, :, 0]) ** 2 + (p[:, None, 1] - cloud[None, :, 1]) ** 2
        at_site += int(many[d2.argmin(axis=1)].sum())
    print("V", g.V, "nodes whose nearest point has 20 copies", at_site)
    assert g.V > 1000 and at_site >= 20
