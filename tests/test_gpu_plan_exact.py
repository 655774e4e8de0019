"""GPU: Engine.plan and Engine.plan_batch (planSafePath on the engine's CSR, trg_engine_plan.ipp) against the plain
restatement of the oracle's A* (tests/cpp/plan_reference.cpp, pinned to the oracle in tests/test_plan_reference.py),
exactly: the node sequence, num_points and the float words of direct_dist, path_length and avg_risk, on every query
of the families of tests/plan_graphs.py -- routes that tie as real numbers and are told apart by the rounding order
of the fp32 step cost, exact ties decided by heap order, asymmetric and parallel edges, Invalid nodes, a goal that
cannot be reached -- at three safety factors, and on a device-built terrain graph."""
import numpy as np
import pytest

import plan_graphs as pg
import plan_ref
from field_support import PARAMS, MOUNTAIN, engine, load_graph  # noqa: F401 (engine: a fixture)

pytestmark = pytest.mark.gpu
F32 = np.float32
MAX_POINTS = 4096  # above every route here (a route visits a node once; the longest graph walk is far shorter)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return plan_ref.compile_reference(tmp_path_factory.mktemp("plan_ref"))


@pytest.fixture(scope="module", params=list(pg.BRAIDS))
def braid_family(request):
    return request.param, pg.braids(request.param)


def _words(direct_dist, path_length, avg_risk):
    return np.array([direct_dist, path_length, avg_risk], np.float32).view(np.uint32).tolist()


def _mismatch(lookup, path, info, want):
    """None, or what differs between one answer of the engine and the restatement's Plan."""
    ids = plan_ref.ids_of_path(lookup, path).tolist()
    if ids != want.ids.tolist():
        return f"route {ids} != {want.ids.tolist()}"
    if info.num_points != want.num_points:
        return f"num_points {info.num_points} != {want.num_points}"
    got = _words(info.direct_dist, info.path_length, info.avg_risk)
    if got != _words(want.direct_dist, want.path_length, want.avg_risk):
        return (f"info {(info.direct_dist, info.path_length, info.avg_risk)} != "
                f"{(want.direct_dist, want.path_length, want.avg_risk)}")
    return None


def _assert_none(bad, total, what):
    assert not bad, f"{len(bad)} of {total} {what} differ from the reference, first: query {bad[0][0]}: {bad[0][1]}"


def _check_family(e, lib, fam, x, sf, batch=False):
    """Every query of the family, placed on the nodes' coordinates, through Engine.plan (and all of them through one
    plan_batch) against the restatement on the exported CSR x."""
    csr = plan_ref.Csr.of_graph(x)
    lookup = plan_ref.id_of_xyz(x.xyz)
    want = [plan_ref.plan(lib, csr, sf, s, g) for s, g in fam.queries]
    starts, goals = x.xyz[fam.queries[:, 0], :2], x.xyz[fam.queries[:, 1]]
    single = [e.plan(s, g, max_points=MAX_POINTS) for s, g in zip(starts, goals)]
    bad = [(q, m) for q, ((path, info), w) in enumerate(zip(single, want)) if (m := _mismatch(lookup, path, info, w))]
    _assert_none(bad, len(want), "Engine.plan answers")
    if batch:
        many = e.plan_batch(starts, goals)
        assert len(many) == len(want)
        bad = [(q, m) for q, ((path, info), w) in enumerate(zip(many, want)) if (m := _mismatch(lookup, path, info, w))]
        _assert_none(bad, len(want), "Engine.plan_batch answers")
    return want


def test_braids_single_and_batch(engine, lib, braid_family, tmp_path):
    """Safety factor 3: the all-fp32 step cost decides 25 of the 384 routes (tests/test_plan_reference.py): while
    plan_on_csr held the safety factor as a double, it returned another route than the reference on exactly those
    16 of 256 and 9 of 128 queries.  The threaded batch returns what the single calls return."""
    name, fam = braid_family
    x = load_graph(engine, fam.graph, tmp_path, name)
    want = _check_family(engine, lib, fam, x, MOUNTAIN["safety_factor"], batch=True)
    assert all(w.status == plan_ref.OK for w in want)


@pytest.mark.parametrize("sf", [0.0, 0.1])
def test_braids_other_safety_factors(lib, braid_family, tmp_path, sf):
    import trg_planner
    name, fam = braid_family
    e = trg_planner.Engine(**dict(PARAMS, safety_factor=sf))
    try:
        x = load_graph(e, fam.graph, tmp_path, name)
        _check_family(e, lib, fam, x, sf)
    finally:
        e.close()


def test_exact_ties(engine, lib, tmp_path):
    """Lattices where every monotone route ties in f and g: the answer hangs on the heap's order alone."""
    fam = pg.exact_ties()
    x = load_graph(engine, fam.graph, tmp_path, "ties")
    want = _check_family(engine, lib, fam, x, MOUNTAIN["safety_factor"], batch=True)
    same = [w for w, (s, g) in zip(want, fam.queries) if s == g]
    assert len(same) >= 2 and all(w.num_points == 1 and w.avg_risk == 0 for w in same)


def test_asymmetric(engine, lib, tmp_path):
    """Direction-dependent and parallel edges, missing reverse edges, Invalid nodes on the cheapest route; the
    cut-off goal gives TRG_ERR_NOT_FOUND: an empty path, num_points 0."""
    fam = pg.asymmetric()
    x = load_graph(engine, fam.graph, tmp_path, "asym")
    want = _check_family(engine, lib, fam, x, MOUNTAIN["safety_factor"], batch=True)
    assert [w.status for w in want[-2:]] == [plan_ref.NOT_FOUND] * 2
    for s, g in fam.queries[-2:]:
        path, info = engine.plan(x.xyz[s, :2], x.xyz[g], max_points=MAX_POINTS)
        assert path.shape == (0, 3) and info.num_points == 0


def test_device_built_graph(lib, mountain_small):
    """100 start and goal pairs on node coordinates of a device-built terrain graph.  Which node a query resolves to
    is tested elsewhere (setGoal may pick a neighbour within robot_size): the engine's own first and last points
    name the two nodes, the search between them is compared."""
    import trg_planner
    e = trg_planner.Engine(**MOUNTAIN)
    try:
        e.set_sampler(7, 16)
        e.set_global_map(mountain_small)
        e.init_graph([15.0, 15.0, 0.0])
        assert e.stats()["used_device_bfs"] == 1, e.fallback_reason
        x = e.graph("global")
        csr = plan_ref.Csr.of_graph(x)
        lookup = plan_ref.id_of_xyz(x.xyz)
        pairs = np.random.default_rng(17).integers(0, x.V, size=(100, 2))
        bad, longest = [], 0
        for q, (a, b) in enumerate(pairs):
            path, info = e.plan(x.xyz[a, :2], x.xyz[b])
            assert path.shape[0] > 0, q
            ends = plan_ref.ids_of_path(lookup, path[[0, -1]])
            m = _mismatch(lookup, path, info, plan_ref.plan(lib, csr, MOUNTAIN["safety_factor"], ends[0], ends[1]))
            if m:
                bad.append((q, m))
            longest = max(longest, path.shape[0])
        _assert_none(bad, len(pairs), "Engine.plan answers")
        assert longest > 20
    finally:
        e.close()
