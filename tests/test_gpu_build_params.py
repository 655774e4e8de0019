"""GPU: builds and queries at the parameters the rest of the suite never moves (tests/param_cases.py, vetted on the
oracle alone in tests/test_param_cases_cpu.py): robot_size from 0.1 to 0.6 on clouds of 4 to 460 points per disc (the
cell of both grids, the walk's step, the LDS capacities of the disc query and the edge gather), expand_dist /
robot_size from below 1 to across the widest node-grid window k_level_sample stages, sample_num from 1 across the
`multi` resolve variant to beyond the level kernels' 64, the collision and height thresholds.

Every case: the graph before and after cleanGraph equals the oracle's fp64-covariance witness bit for bit and the
counters the oracle's, on the device path (or, beyond its range, after the decline that names the range) and with the
host replay; is_collision, nearest_z, edge_risk and plan answer as the oracle does under the case's parameters; four
cases go on through one set_local_map / update_graph step.
"""
import numpy as np
import pytest

import param_cases as pc
from graph_support import _assert_same_graph, _build, _build_any, _check_build, _witness, graph_invariants, obs_crop

pytestmark = pytest.mark.gpu


def _case(oa, synth, name):
    case = pc.BY_NAME[name]
    points, start = pc.cloud(synth, case.cloud)
    prm = pc.params(oa, case)
    return case, points, start, prm, _witness(oa, "param_" + name, prm, points, start)


def _build_as_expected(prm, points, start, options):
    """The default route: the device path where param_cases.device_supported says so, else its decline by name and
    the host replay's answer."""
    if pc.device_supported(prm):
        return _build(prm, points, start, options) + (True,)
    e, st = _build_any(prm, points, start, options)
    assert st["used_device_bfs"] == 0 and st["bfs_fallbacks"] == 1, (st["used_device_bfs"], st["bfs_fallbacks"])
    assert pc.DECLINE_REASON in e.fallback_reason, e.fallback_reason
    return e, st, False


def _check_queries(e, o32, points, prm, long_edge=5.0):
    """is_collision, nearest_z and edge_risk of engine e against the (literal, fp32-covariance) oracle o32."""
    q = pc.disc_queries(points, prm["robot_size"])
    asked = [(e.is_collision(q), o32.is_collision(q, 0, prm["collision_threshold"]), "its own threshold")]
    asked += [(e.is_collision(q, threshold=t), o32.is_collision(q, 0, t), f"threshold {t}") for t in (0.0, 0.5, 1.0)]
    for (fe, ce, ne), (fo, co, no), what in asked:
        assert np.array_equal(ne, no), (what, int((ne != no).sum()))
        assert np.array_equal(ce, co), (what, int((ce != co).sum()))
        assert np.array_equal(fe, fo), (what, int((fe != fo).sum()))
    ze, zo = e.nearest_z(q), o32.nearest_z(q)
    assert np.array_equal(ze.view(np.uint32), zo.view(np.uint32)), int((ze != zo).sum())
    # zero length, up to expand_dist + robot_size, 5 robot_size: the rule of test_zero_length_and_long_edges
    p1, p2 = pc.edge_pairs(points, prm, e.nearest_z, long_edge)
    st, npts, w, d = e.edge_risk(p1, p2)
    so, no, wo, do = o32.edge_risk(p1, p2)
    assert np.array_equal(st, so), (st.tolist(), so.tolist())
    ok = st == 0
    assert np.array_equal(npts[ok], no[ok])
    assert np.array_equal(d.view(np.uint32), do.view(np.uint32))
    print("edge_risk: statuses", np.bincount(st, minlength=1).tolist(), "largest weight difference",
          float(np.abs(w - wo).max()))
    assert float(np.abs(w - wo).max()) <= 1e-5


def _check_plans(e, o, cloud_name):
    for s, g in pc.PLANS[cloud_name]:
        po, io = o.plan(s, g)
        pe, ie = e.plan(s, g)
        assert po.shape[0] >= 2, (s, g)
        assert np.array_equal(pe.view(np.uint32), po.view(np.uint32)), (s, g, pe.shape, po.shape)
        assert ie.path_length == io[1], (s, g, ie.path_length, io[1])


@pytest.mark.parametrize("name", pc.NAMES)
def test_build_and_entry_points(oa, synth, name):
    """The default route of every case (the device path, or its decline and the host replay's answer), then the other
    entry points under the case's parameters.

    ratio_below_1 (expand_dist < robot_size): every sample lies within robot_size of the root, its nearest node,
    so expandGraph wires the root to itself (trg.cpp:414-416: no edge) and creates nothing; cleanGraph drops the
    root, which has no edge (trg.cpp:498).  The reference's initGraph goes on to an assert on node_id that a release
    build compiles out and returns with an empty graph, and the oracle reports success with one node before
    cleanGraph and none after.  So the engine must return TRG_OK and that same empty graph, on the device path; a plan
    on it is TRG_ERR_NO_GRAPH (the reference and the oracle dereference a null nearest node there: not asked)."""
    case, points, start, prm, witness = _case(oa, synth, name)
    e, st, device = _build_as_expected(prm, points, start, {})
    assert device == (name not in pc.DECLINED)
    _check_build(e, st, witness, name, device=device)
    g = e.graph("global")
    print(f"{name}: V {witness[0].V} -> {g.V}, E {g.E}, device {device}, levels {st['bfs_levels']}, "
          f"multi-pass rows {st['bfs_multipass_rows']}, edge evaluations {st['edge_evals_gpu']}")
    if name in ("s32", "s33"):
        # what the pair is kept for: at 33 a row of k_level_resolve has more earlier candidates in reach than it holds
        # at once and takes them in passes (only the `multi` variant does, and counts it); at 32 that variant is off
        assert (st["bfs_multipass_rows"] > 0) == (name == "s33"), st["bfs_multipass_rows"]
    o32 = pc.make_oracle(oa, prm, points, f64=False)
    _check_queries(e, o32, points, prm)
    o32.close()
    if name == pc.EMPTY:
        from trg_planner._engine import TrgError
        assert (g.V, g.E) == (0, 0) and g.rowptr.tolist() == [0]
        with pytest.raises(TrgError) as ei:
            e.plan(*pc.PLANS[case.cloud][0])
        assert ei.value.status == 5
    else:
        graph_invariants(g, prm["expand_dist"])
        o = pc.make_oracle(oa, prm, points)  # the witness, alive: its A* on its own graph
        assert o.init_graph(start)
        _check_plans(e, o, case.cloud)
        o.close()
    e.close()


@pytest.mark.parametrize("name", pc.NAMES)
def test_host_replay(oa, synth, name):
    _, points, start, prm, witness = _case(oa, synth, name)
    e, st = _build_any(prm, points, start, {"replay": "host"})
    assert st["used_device_bfs"] == 0 and st["bfs_fallbacks"] == 0, (st["used_device_bfs"], st["bfs_fallbacks"])
    _check_build(e, st, witness, name + " replay=host", device=False)
    e.close()


@pytest.mark.parametrize("known", [0, 1])
@pytest.mark.parametrize("name", pc.KNOWN_START_DISC)
def test_known_start_disc(oa, synth, name, known):
    _, points, start, prm, witness = _case(oa, synth, name)
    e, st = _build(prm, points, start, {"known_start_disc": known})
    _check_build(e, st, witness, f"{name} known_start_disc={known}")
    if known:
        assert 0 < st["start_discs_known"] <= st["edge_evals_gpu"], st["start_discs_known"]
    else:
        assert st["start_discs_known"] == 0
    e.close()


@pytest.mark.parametrize("name", list(pc.UPDATES))
def test_update_step(oa, synth, name):
    """One local map with an obstacle the global map lacks, 8 robot_size around the pose, then updateGraph: the graph
    equals the witness's, and isFrontier answers as the oracle's at the nodes the step left Frontier."""
    _, points, start, prm, witness = _case(oa, synth, name)
    e, st = _build(prm, points, start, {})
    _check_build(e, st, witness, name)
    o = pc.make_oracle(oa, prm, points)
    assert o.init_graph(start)
    pose, box = pc.UPDATES[name]
    obs = obs_crop(points, pose, 8 * prm["robot_size"], box=box)
    e.set_local_map(pose, obs)
    o.set_local_map(pose, obs)
    e.update_graph()
    o.update_graph()
    go = o.graph(0)
    _assert_same_graph(e.graph("global"), go, name + ": after the update")
    frontier = go.xyz[go.state == 1, :2]
    assert frontier.shape[0] > 0
    # the Frontier nodes, and the disc queries that fall into the local map's box and around it
    q = pc.disc_queries(points, prm["robot_size"])
    for xy in (frontier, q):
        fe, fo = e.is_frontier(xy), o.is_frontier(xy)
        assert np.array_equal(fe, fo), (int((fe != fo).sum()), xy.shape[0])
    thr = prm["update_collision_threshold"]
    (fe, ce, ne), (fo, co, no) = e.is_collision(q, kind="local", threshold=thr), o.is_collision(q, 1, thr)
    assert np.array_equal(ne, no) and np.array_equal(ce, co) and np.array_equal(fe, fo)
    print(f"{name}: V {witness[1].V} -> {go.V}, Frontier {frontier.shape[0]}, is_frontier true at "
          f"{int(o.is_frontier(frontier).sum())} of them")
    e.close()
    o.close()


def test_queries_at_the_hit_capacity(oa, synth):
    """No build: discs of 1009 to 1026 map points, either side of HCAP = 1024, and edges whose boxes hold thousands."""
    points, _ = pc.cloud(synth, pc.HCAP_CASE["cloud"])
    prm = dict(oa.MOUNTAIN, **pc.HCAP_CASE["overrides"])
    import trg_planner
    e = trg_planner.Engine(**prm)
    e.set_sampler(pc.SEED, pc.TABLE_BITS)
    e.set_global_map(points)
    o32 = pc.make_oracle(oa, prm, points, f64=False)
    n = e.is_collision(pc.disc_queries(points, prm["robot_size"]))[2]
    assert n.min() <= pc.HCAP < n.max(), (int(n.min()), int(n.max()))
    _check_queries(e, o32, points, prm, pc.HCAP_CASE["long_edge"])
    o32.close()
    e.close()
