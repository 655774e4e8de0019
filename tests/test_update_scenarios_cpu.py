"""The update scenarios of update_scenarios.py on the two oracles alone (fp32 covariance and the fp64 witness): they
agree on structure at every step, and every scenario still reaches what it was written to reach -- a later edit to a
cloud or a seed cannot quietly turn one into a no-op.  No GPU."""
import numpy as np
import pytest

import update_scenarios as us
from graph_support import drive


@pytest.fixture(scope="module")
def clouds(synth, mountain_gentle, indoor_small):
    return us.scenario_clouds(synth, mountain_gentle, indoor_small)


def oracles(oa, sc):
    prm = us.params(oa, sc)
    pair = []
    for f64 in (False, True):
        o = oa.Oracle(**prm)
        o.set_sampler(sc.seed, 0, 16)
        o.set_cov_f64(f64)
        pair.append(o)
    return prm, pair[0], pair[1]


@pytest.mark.parametrize("name", [sc.name for sc in us.SCENARIOS])
def test_scenario_on_the_oracles(oa, clouds, name):
    sc = us.BY_NAME[name]
    prm, o, w = oracles(oa, sc)
    hist = drive(None, o, w, sc.steps, clouds=clouds, prm=prm)
    assert len(hist) == sum(s[0] in ("init", "init_declined", "update") for s in sc.steps)
    print(name, [(h["V"], h["E"], h["wire_calls"]) for h in hist])
    if name in us.PRECONDITIONS:
        us.PRECONDITIONS[name](hist)
    if name == "history_rebuild":
        # B built after a build and an update on another map: the V and E of a fresh build of B, another node order
        _, fresh, fresh_w = oracles(oa, sc)
        ref = drive(None, fresh, fresh_w, [("map", "B"), ("init", us.START_B)], clouds=clouds, prm=prm)[0]
        after = hist[2]
        assert sc.steps[after["i"]] == ("init", us.START_B)
        assert (after["V"], after["E"]) == (ref["V"], ref["E"]) == (2288, 16592)
        assert not np.array_equal(after["xyz"], ref["xyz"])
        assert set(map(bytes, np.ascontiguousarray(after["xyz"]))) == set(map(bytes, np.ascontiguousarray(ref["xyz"])))


def test_pose_on_node_is_not_a_frontier(oa, clouds):
    """The pose of pose_on_node is a node's exact position, and isFrontier says no there."""
    sc = us.BY_NAME["pose_on_node"]
    prm, o, w = oracles(oa, sc)
    k = [i for i, s in enumerate(sc.steps) if s[0] == "local"][0]
    drive(None, o, w, sc.steps[:k + 1], clouds=clouds, prm=prm)
    g = o.graph(0)
    pose = g.xyz[g.V // 2, :2]
    assert o.is_frontier(pose[None, :])[0] == 0
