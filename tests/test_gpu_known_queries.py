"""GPU: map queries the build already holds the answer to (option known_start_disc).

The first disc of a wireEdge segment walk (trg.cpp:283, i = 0) sits at node1's position bit for bit, and a node
the level loop created passed exactly that isCollision call as a sample (trg.cpp:398): the engine keeps the disc's
point count per node (BfsDev::ndisc), and the speculative parent edges and the deferred evaluations start their
walk at the second disc.  With the option on and off the graph before and after cleanGraph must equal the
oracle's fp64-covariance witness bit for bit, the counters the oracle's, the byte statistics each other's --
on rough and gentle terrain, with step 3 on, at walk lengths on and off the fast path's disc limit, on every
route on which a node's count is unknown (host-replayed levels, repeated launches), in a tile and before an
update against the local map.
"""
import numpy as np
import pytest

from graph_support import _assert_same_graph, _build, _check_build, _witness, _witnesses, obs_crop

pytestmark = pytest.mark.gpu

START = [15.0, 15.0, 0.0]
COMBOS = [{"known_start_disc": 0}, {"known_start_disc": 1}]
SAME_ACROSS = ("bytes_spec_kernel", "bytes_edge_kernel", "edge_evals_gpu")


def _check_combos(oa, key, prm, cloud, start, core=None, min_nodes=200):
    witness = _witness(oa, key, prm, cloud, start, core)
    assert witness[0].V > min_nodes, (key, witness[0].V)
    seen = []
    for combo in COMBOS:
        what = f"{key} {combo}"
        e, st = _build(prm, cloud, start, combo, core)
        _check_build(e, st, witness, what)
        e.close()
        print(f"{what}: V {witness[0].V} edge_evals_gpu {st['edge_evals_gpu']} start_discs_known {st['start_discs_known']}")
        if combo["known_start_disc"]:
            # the new path really ran, and never more often than there were evaluations
            assert 0 < st["start_discs_known"] <= st["edge_evals_gpu"], (what, st["start_discs_known"])
        else:
            assert st["start_discs_known"] == 0, (what, st["start_discs_known"])
        seen.append(st)
    for name in SAME_ACROSS:
        assert len({s[name] for s in seen}) == 1, (key, name, [s[name] for s in seen])
    return seen


CLOUDS = {
    "mountain_small": ("mountain_small", "MOUNTAIN", {}, START),
    "mountain_small_s16": ("mountain_small", "MOUNTAIN", {"sample_num": 16}, START),
    "mountain_gentle": ("mountain_gentle", "MOUNTAIN", {}, START),
    "indoor_small": ("indoor_small", "INDOOR", {}, [1.5, 1.5, 0.0]),  # step 3 on
}


@pytest.mark.parametrize("name", list(CLOUDS))
def test_option_on_and_off_equal_the_witness(oa, request, name):
    fixture, base, extra, start = CLOUDS[name]
    cloud = request.getfixturevalue(fixture)
    prm = dict(getattr(oa, base), **extra)
    _check_combos(oa, name, prm, cloud, start)


# dist / ds of the parent edge on a boundary (ratio 4: five discs or four, on rounding), below it, between two,
# and deferred edges of more than KMAX = 6 discs: the general path, whose walk then starts at i = ds.  A deferred
# edge joins a node to a sample's nearest node, at most expand_dist + robot_size = 1.1 from it; ds = 0.15, so an
# edge longer than 0.9 walks i = 0, 0.15, ... 0.9: at least 7 discs.  The test below checks that the graph holds
# such edges (each was evaluated, and succeeded, on the general path), from nodes the level loop created.
WALKS = {
    "ratio4": dict(expand_dist=0.6),
    "ratio3": dict(expand_dist=0.45),
    "ratio3_33": dict(expand_dist=0.5),
    "beyond_kmax": dict(expand_dist=0.8, robot_size=0.3),
}


@pytest.mark.parametrize("name", list(WALKS))
def test_walk_lengths_at_the_seams(oa, mountain_small, name):
    prm = dict(oa.MOUNTAIN, **WALKS[name])
    _check_combos(oa, "walk_" + name, prm, mountain_small, START)
    if name == "beyond_kmax":
        pre = _witnesses["walk_" + name][0]
        src = np.repeat(np.arange(pre.V), np.diff(pre.rowptr))
        long_edges = int(((pre.dist > 0.9) & (src > 0) & (pre.col > 0)).sum())  # (node 0 is the root: no count)
        print(f"beyond_kmax: {long_edges} directed entries longer than 0.9 of {pre.E}")
        assert long_edges > 0


# routes on which a node's count is unknown or a level's kernels run more than once
UNKNOWN = {
    "host_level_replay": ({"debug_tie_every": 3}, {"bfs_host_levels_min": 5}),
    "stall_ticketed_repeat": ({"debug_stall_level": 9, "debug_wait_rerun": 0}, {}),
    "stall_host_replay": ({"debug_stall_level": 9, "debug_wait_rerun": 1}, {"bfs_host_levels_min": 1}),
    "tickets_always": ({"resolve_tickets": 1}, {}),
    "top_up_launches": ({"debug_spec_bound": 3}, {}),
    "no_overlap": ({"defer_overlap": 0}, {}),
    "sparse_call_log": ({"debug_call_stride": 1}, {}),
}


@pytest.mark.parametrize("name", list(UNKNOWN))
def test_nodes_whose_count_is_unknown(oa, mountain_small, name):
    options, expect = UNKNOWN[name]
    prm = dict(oa.MOUNTAIN)
    witness = _witness(oa, "mountain_small", prm, mountain_small, START)
    e, st = _build(prm, mountain_small, START, dict(options, known_start_disc=1))
    if "bfs_host_levels_min" in expect:
        assert st["bfs_host_levels"] >= expect["bfs_host_levels_min"], st["bfs_host_levels"]
    _check_build(e, st, witness, name)
    assert 0 < st["start_discs_known"] <= st["edge_evals_gpu"], (name, st["start_discs_known"])
    e.close()


def test_host_replayed_levels_leave_their_nodes_unknown(oa, mountain_small):
    """Every third level replayed on the host: the nodes those levels create have no count, so fewer evaluations
    skip their first disc than in the plain build."""
    prm = dict(oa.MOUNTAIN)
    e, plain = _build(prm, mountain_small, START, {"known_start_disc": 1})
    e.close()
    e, replayed = _build(prm, mountain_small, START, {"known_start_disc": 1, "debug_tie_every": 3})
    e.close()
    assert 0 < replayed["start_discs_known"] < plain["start_discs_known"], (replayed["start_discs_known"],
                                                                            plain["start_discs_known"])


def test_tile_with_a_core_smaller_than_the_cloud(oa, mountain_small):
    """Draws outside the core are rejected draws (set_tile): a rejected draw never becomes a node, an accepted one
    passed the disc test inside the core like any other."""
    core = [9.0, 9.0, 21.0, 21.0]
    prm = dict(oa.MOUNTAIN)
    seen = _check_combos(oa, "tile", prm, mountain_small, START, core=core, min_nodes=100)
    # the core really cut the build short of the cloud's 30 m x 30 m
    full = _witness(oa, "mountain_small", prm, mountain_small, START)
    assert _witnesses["tile"][0].V < full[0].V // 2
    assert seen[0]["trials"] == seen[1]["trials"]


def test_update_after_a_build_uses_no_count(oa, mountain_gentle):
    """updateGraph evaluates edges against the LOCAL map: the counts of the global build must not reach it."""
    import trg_planner
    prm = dict(oa.MOUNTAIN, update_collision_threshold=0.2)
    start = [15.0, 15.0, 0.0]
    e = trg_planner.Engine(**prm)
    e.set_sampler(5, 16)
    e.set_option("known_start_disc", 1)
    e.set_global_map(mountain_gentle)
    e.init_graph(start)
    assert e.stats()["start_discs_known"] > 0
    o = oa.Oracle(**prm)
    o.set_sampler(5, 0, 16)
    o.set_cov_f64(True)
    o.set_global_map(mountain_gentle)
    assert o.init_graph(start)
    _assert_same_graph(e.graph("global"), o.graph(0), "before the update")
    for k, pose in enumerate([(12.0, 12.0), (13.0, 12.5), (14.0, 13.0)]):
        obs = obs_crop(mountain_gentle, pose, 4.0, box=(pose[0] + 2.0, pose[1] + 1.0, 0.6))
        e.set_local_map(pose, obs)
        o.set_local_map(pose, obs)
        e.update_graph()
        o.update_graph()
        _assert_same_graph(e.graph("global"), o.graph(0), f"after update {k}")
    assert (o.graph(0).state == 1).any()  # the obstacle left frontier states behind
    e.close()
    o.close()
