"""The cases of param_cases.py on the oracle alone: every case a GPU test rests on still shows what it is kept for --
its size, the disc counts either side of an LDS capacity, walks longer than the fast path's six discs, step 3 on the
side of its rounding edge that the case names, the side of the level kernels' range that the test expects, a Frontier
state after the update step -- so that a later edit to a cloud or a parameter fails here and not silently on the GPU.
Conditions, not measurements.  No GPU."""
import numpy as np
import pytest

import param_cases as pc
import step3_cases as s3
from graph_support import _witness, first_difference, obs_crop


def _case(oa, synth, name):
    case = pc.BY_NAME[name]
    points, start = pc.cloud(synth, case.cloud)
    prm = pc.params(oa, case)
    return case, points, start, prm


def _disc_counts(oa, prm, points):
    o = pc.make_oracle(oa, prm, points)
    n = o.is_collision(pc.disc_queries(points, prm["robot_size"]), 0, prm["collision_threshold"])[2]
    o.close()
    return n


@pytest.mark.parametrize("name", pc.NAMES)
def test_case_on_the_oracle(oa, synth, name):
    case, points, start, prm = _case(oa, synth, name)
    assert points.shape[0] <= 26000
    pre, clean, c = _witness(oa, "param_" + name, prm, points, start)  # (asserts that the oracle builds a graph)
    print(name, "V before cleanGraph", pre.V, "after", clean.V, "E", clean.E)
    if case.exact is not None:
        assert (pre.V, clean.V) == case.exact
    else:
        assert 2 * clean.V >= case.V, (clean.V, case.V)
    assert c["created"] == pre.V
    # the literal fp32 oracle builds the structure of the fp64-covariance witness (its weights carry the error of an
    # fp32 covariance sum, which on the sparse clouds is larger than on the suite's 0.1 m lattice: printed, not bounded)
    o = pc.make_oracle(oa, prm, points, f64=False)
    assert o.init_graph(start)
    assert first_difference(pre, o.graph(1), weights=None) is None
    assert first_difference(clean, o.graph(0), weights=None) is None
    if clean.E:
        print(name, "largest weight difference between the two oracles", float(np.abs(clean.w - o.graph(0).w).max()))
    # plan() has an answer to compare on every case but the empty one
    if clean.V:
        for s, g in pc.PLANS[case.cloud]:
            assert o.plan(s, g)[0].shape[0] >= 2, (s, g)
    else:
        assert name == pc.EMPTY
    o.close()


def test_the_side_of_the_level_kernels_range(oa):
    """The window of k_level_sample and sample_num, from the formula written out in param_cases.py."""
    declined = tuple(c.name for c in pc.CASES if not pc.device_supported(pc.params(oa, c)))
    assert declined == pc.DECLINED
    side = {c.name: pc.window_side(pc.params(oa, c)) for c in pc.CASES}
    assert side["ratio_1"] == 9 and side["ratio_1_03"] == 9
    for name in ("ratio_2_97_rough", "ratio_2_97_gentle", "ratio_2_95_rough", "ratio_2_95_gentle"):
        assert side[name] == 15, (name, side[name])  # the last supported window (16 is even: never a side)
    assert side["ratio_3_0"] == 17 and side["ratio_3_05"] == 17
    assert pc.BY_NAME["s32"].overrides["sample_num"] == 32 and pc.BY_NAME["s33"].overrides["sample_num"] == 33
    assert pc.BY_NAME["s65"].overrides["sample_num"] == pc.S_MAX + 1
    assert set(pc.KNOWN_START_DISC) | set(pc.UPDATES) | set(pc.STEP3_BOUNDARY) <= set(pc.NAMES)
    assert not set(pc.KNOWN_START_DISC) & set(pc.DECLINED)


def test_seam_cases_straddle_the_disc_capacities(oa, synth):
    counts = {}
    for name in ("r045_dense", "r05_dense", "r010", "r015"):
        _, points, _, prm = _case(oa, synth, name)
        counts[name] = n = _disc_counts(oa, prm, points)
        print(name, "points per disc", int(n.min()), "-", int(n.max()))
    assert counts["r045_dense"].min() <= pc.SHCAP < counts["r045_dense"].max()
    assert counts["r05_dense"].min() > pc.SHCAP
    assert 1 <= counts["r010"].min() and counts["r010"].max() <= 4
    assert counts["r015"].max() < 16


def test_hcap_case_straddles_the_capacity(oa, synth):
    points, _ = pc.cloud(synth, pc.HCAP_CASE["cloud"])
    n = _disc_counts(oa, dict(oa.MOUNTAIN, **pc.HCAP_CASE["overrides"]), points)
    print("points per disc", int(n.min()), "-", int(n.max()), "over", int((n > pc.HCAP).sum()))
    assert n.min() <= pc.HCAP < n.max()


@pytest.mark.parametrize("name", ["ratio_2_97_rough", "ratio_2_97_gentle"])
def test_walks_beyond_the_fast_path(oa, synth, name):
    """Directed entries longer than KMAX = 6 steps of robot_size / 2, between nodes other than the root: each was
    evaluated, and succeeded, on the general walk path."""
    _, points, start, prm = _case(oa, synth, name)
    pre = _witness(oa, "param_" + name, prm, points, start)[0]
    src = np.repeat(np.arange(pre.V), np.diff(pre.rowptr))
    long_edges = int(((pre.dist > 6 * prm["robot_size"] / 2) & (src > 0) & (pre.col > 0)).sum())
    print(name, long_edges, "of", pre.E, "longest", float(pre.dist.max()))
    assert long_edges > 0
    assert pre.dist.max() <= prm["expand_dist"] + prm["robot_size"]


def test_step3_boundaries(oa):
    for name, on in pc.STEP3_BOUNDARY.items():
        prm = pc.params(oa, pc.BY_NAME[name])
        assert s3.step3_is_on(prm) == on, name
    # r045_dense sits on the edge: 0.6 - 0.45 against 0.25 * 0.6 differ by rounding alone
    prm = pc.params(oa, pc.BY_NAME["r045_dense"])
    assert abs((prm["expand_dist"] - prm["robot_size"]) - 0.25 * prm["expand_dist"]) < 1e-7


@pytest.mark.parametrize("name", list(pc.UPDATES))
def test_update_step_leaves_a_frontier(oa, synth, name):
    _, points, start, prm = _case(oa, synth, name)
    pose, box = pc.UPDATES[name]
    o = pc.make_oracle(oa, prm, points)
    assert o.init_graph(start)
    before = o.graph(0).V
    o.set_local_map(pose, obs_crop(points, pose, 8 * prm["robot_size"], box=box))
    o.update_graph()
    g = o.graph(0)
    o.close()
    print(name, "V", before, "->", g.V, "Frontier", int((g.state == 1).sum()))
    assert (g.state == 1).any()
