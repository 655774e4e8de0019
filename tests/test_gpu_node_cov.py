"""The weights of the edges that CREATED a node, on every route a NodeCov can take.

The level loop only learns whether a candidate's parent edge holds (k_level_spec); the covariance of the gather
is computed afterwards, for the created nodes alone (k_node_cov), and k_node_weights turns it into the weight.
What k_node_cov is handed depends on the path the level took: committed by the device (beside the loop or all
after it), replayed on the host (the NodeCov is uploaded with its call alone), repeated with start tickets,
a sparse call log.  On each of them the whole graph before and after cleanGraph must equal the oracle's
fp64-covariance witness: structure equal, weights the same floats.  (The host BFS evaluates the edges whole and
is the control.)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

START = [15.0, 15.0, 0.0]
SEED = 7

# option settings per configuration, and what the build's statistics must show so that the path was taken
CONFIGS = {
    "default": ({}, {}),
    "no_overlap": ({"defer_overlap": 0}, {}),
    "host_level_replay": ({"debug_tie_every": 3}, {"bfs_host_levels_min": 5}),
    "stall_ticketed_repeat": ({"debug_stall_level": 9, "debug_wait_rerun": 0}, {"bfs_ticket_reruns": 1}),
    "stall_host_replay": ({"debug_stall_level": 9, "debug_wait_rerun": 1},
                          {"bfs_ticket_reruns": 1, "bfs_host_levels_min": 1}),
    "tickets_always": ({"resolve_tickets": 1}, {}),
    "sparse_call_log": ({"debug_call_stride": 1}, {}),
    "host_bfs": ({"replay": "host"}, {}),
}


def _assert_same_graph(g, ref, what):
    assert (g.V, g.E) == (ref.V, ref.E), (what, g.V, ref.V, g.E, ref.E)
    assert np.array_equal(g.rowptr, ref.rowptr), what
    assert np.array_equal(g.col, ref.col), what
    assert np.array_equal(g.state, ref.state), what
    assert np.array_equal(g.cid, ref.cid), what
    assert np.array_equal(g.xyz.view(np.uint32), ref.xyz.view(np.uint32)), what
    assert np.array_equal(g.dist.view(np.uint32), ref.dist.view(np.uint32)), what
    differ = int((g.w.view(np.uint32) != ref.w.view(np.uint32)).sum())
    assert differ == 0, (what, differ, float(np.abs(g.w - ref.w).max()))


def _witness(oa, prm, cloud, start):
    o = oa.Oracle(**prm)
    o.set_sampler(SEED, 0, 16)
    o.set_cov_f64(True)
    o.set_global_map(cloud)
    assert o.init_graph(start)
    graphs = (o.graph(1), o.graph(0))
    o.close()
    return graphs


@pytest.fixture(scope="module")
def mountain_witness(oa, mountain_small):
    pre, clean = _witness(oa, dict(oa.MOUNTAIN), mountain_small, START)
    # The check must not pass on zeros: in the ORACLE's graph before cleanGraph the first entry of a created
    # node's row is its parent edge (wireEdge(parent, new) is the first call that can wire the new node), and at
    # least 1 000 of those weights are non-zero (1 988 of 3 094 for this cloud).
    deg = np.diff(pre.rowptr)
    created = np.arange(1, pre.V)[deg[1:] > 0]
    first = pre.rowptr[created]
    assert (pre.col[first] < created).all()  # the parent exists before its child
    nonzero = int((pre.w[first] != 0).sum())
    print(f"witness: {created.size} created nodes with a parent edge, {nonzero} of these weights non-zero")
    assert nonzero >= 1000, (nonzero, created.size)
    return pre, clean


@pytest.mark.parametrize("name", list(CONFIGS))
def test_creating_edge_weights_equal_the_fp64_witness(oa, mountain_small, mountain_witness, name):
    import trg_planner
    options, expect = CONFIGS[name]
    e = trg_planner.Engine(**dict(oa.MOUNTAIN))
    e.set_sampler(SEED, 16)
    e.set_option("keep_preclean", 1)
    for k, v in options.items():
        e.set_option(k, v)
    e.set_global_map(mountain_small)
    e.init_graph(START)
    st = e.stats()
    assert st["bfs_fallbacks"] == 0, (st, e.fallback_reason)
    assert st["used_device_bfs"] == (0 if name == "host_bfs" else 1), e.fallback_reason
    if "bfs_ticket_reruns" in expect:
        assert st["bfs_ticket_reruns"] == expect["bfs_ticket_reruns"], st["bfs_ticket_reruns"]
    if "bfs_host_levels_min" in expect:
        assert st["bfs_host_levels"] >= expect["bfs_host_levels_min"], st["bfs_host_levels"]
    pre, clean = mountain_witness
    _assert_same_graph(e.graph("preclean"), pre, name + ": before cleanGraph")
    _assert_same_graph(e.graph("global"), clean, name + ": after cleanGraph")
    e.close()


def test_step3_build_structure_and_states(oa, indoor_small):
    """expandGraph's step 3 on (indoor.yaml) on a flat floor: this pins the tree order of the neighbour calls
    (k_kd_*, k_step3_calls) through structure and states, and nothing else.  No parent edge of this fixture fails
    (test_step3_cases_cpu.py keeps that on record) and every weight is 0, so no node is rescued and k_node_cov
    passes over none: nodes that are valid although their parent edge failed, and their weights, are
    test_gpu_step3.py's."""
    import trg_planner
    prm = dict(oa.INDOOR)
    start = [1.5, 1.5, 0.0]
    e = trg_planner.Engine(**prm)
    e.set_sampler(SEED, 16)
    e.set_option("keep_preclean", 1)
    e.set_global_map(indoor_small)
    e.init_graph(start)
    st = e.stats()
    assert st["used_device_bfs"] == 1 and st["bfs_fallbacks"] == 0, (st, e.fallback_reason)
    pre, clean = _witness(oa, prm, indoor_small, start)
    assert pre.V > 200, pre.V
    _assert_same_graph(e.graph("preclean"), pre, "indoor: before cleanGraph")
    _assert_same_graph(e.graph("global"), clean, "indoor: after cleanGraph")
    e.close()
