"""GPU: the incremental path and the engine's histories against the oracle -- the scenarios of update_scenarios.py,
one engine, one oracle and the oracle's fp64 witness through the same steps (graph_support.drive): after every build
and every update the graph is the oracle's bit for bit (ids included: cleanGraph renumbers in the iteration order of
a container whose state depends on everything that went before) and its weights are the witness's bit for bit."""
import pytest

import update_scenarios as us
from graph_support import drive

pytestmark = pytest.mark.gpu

CASES = [(sc.name, replay) for sc in us.SCENARIOS for replay in sc.replays]


@pytest.fixture(scope="module")
def clouds(synth, mountain_gentle, indoor_small):
    return us.scenario_clouds(synth, mountain_gentle, indoor_small)


def run(oa, clouds, name, replay):
    import trg_planner
    sc = us.BY_NAME[name]
    prm = us.params(oa, sc)
    e = trg_planner.Engine(**prm)
    e.set_sampler(sc.seed, 16)
    if replay is not None:
        e.set_option("replay", replay)
    o, w = oa.Oracle(**prm), oa.Oracle(**prm)
    for x in (o, w):
        x.set_sampler(sc.seed, 0, 16)
    w.set_cov_f64(True)
    hist = drive(e, o, w, sc.steps, clouds=clouds, prm=prm)
    print(name, replay, [(h["V"], h["E"], h["local_V"], h["stats"]["edge_calls"]) for h in hist])
    if name in us.PRECONDITIONS:
        us.PRECONDITIONS[name](hist)
    # which replay made each build (stats are per build: the updates after it leave these alone)
    replay_now, builds = replay, []
    for i, step in enumerate(sc.steps):
        if step[0] == "replay":
            replay_now = step[1]
        if step[0] in ("init", "init_declined"):
            builds.append((step[0], replay_now, next(h for h in hist if h["i"] == i)["stats"]))
    for kind, how, st in builds:
        if kind == "init_declined":
            assert (st["used_device_bfs"], st["bfs_fallbacks"]) == (0, 1), (kind, how, st)
        else:
            assert (st["used_device_bfs"], st["bfs_fallbacks"]) == (int(how == "device"), 0), (kind, how, st)
    return hist


@pytest.mark.parametrize("name,replay", [c for c in CASES if c[0] != "many_roots"])
def test_update_sequence(oa, clouds, name, replay):
    run(oa, clouds, name, replay)


def test_many_roots(oa, clouds):
    """One update whose roots fill more than one chunk of 4096 and whose deferred edges more than one batch of
    65536: the second root chunk and the flush in the middle of an expansion.  mountain_gentle at sample_num 16
    builds 5975 nodes, 5807 of them local and every one a root, and the update makes 100384 wireEdge calls."""
    build, update = run(oa, clouds, "many_roots", "device")
    assert update["local_V"] > 4096, update["local_V"]
    assert update["stats"]["edge_calls"] - build["stats"]["edge_calls"] > 65536, \
        (build["stats"]["edge_calls"], update["stats"]["edge_calls"])
    # ... of which a full batch went out before the last expansion ended, and the rest after it
    assert update["stats"]["launches_edge_kernel"] - build["stats"]["launches_edge_kernel"] >= 2
