"""GPU: the nearest-map-point tie-break past the sizes test_gpu_map_ties.py and test_gpu_tie_repairs.py reach (clouds and
their preconditions: map_tie_cases.py, test_map_tie_cases_cpu.py) -- more tied points than one page of k_map_tied_set
lists, walks down an insertion tree as deep as the cloud is long, with the decision on every boundary of the walk (the
last host step, the first device step, either side of a launch of 64 steps, either side of the 64 launches the walk
was once limited to, the last point), ties the first pass of the set kernel does not find, a second map on the same
engine, and builds in which every accepted sample of a level ties.  Everything is compared with the live oracle:
elevations bit for bit, graphs through assert_graph_equal."""
import time

import numpy as np
import pytest

import map_tie_cases as mc
from conftest import assert_graph_equal

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _engine(oa, cloud):
    import trg_planner
    e = trg_planner.Engine(**oa.MOUNTAIN)
    e.set_global_map(cloud)
    return e


def _oracle_z(oa, cloud, queries, local=False):
    o = oa.Oracle(**oa.MOUNTAIN)
    if local:
        o.set_local_map([0.0, 0.0], cloud)
    else:
        o.set_global_map(cloud)
    z = o.nearest_z(queries, 1 if local else 0)
    o.close()
    return z


def _assert_same_z(ze, zo, cloud, queries, what):
    differ = np.flatnonzero(_bits(ze) != _bits(zo))
    low = mc.lowest_index_z(cloud, queries[differ[:1]]) if differ.size else None
    assert differ.size == 0, f"{what}: z differs on {differ.size} of {len(zo)} queries, first at {queries[differ[0]]}: " \
                             f"{ze[differ[0]]!r}, oracle {zo[differ[0]]!r} (lowest cloud index: {low[0]!r})"


def _check_nearest_z(oa, cloud, queries, what):
    e = _engine(oa, cloud)
    t0 = time.perf_counter()
    ze = e.nearest_z(queries)   # (raises unless the call returns TRG_OK)
    dt = time.perf_counter() - t0
    st = e.stats()
    print(what, len(queries), "queries in", round(dt, 3), "s; resolved", st["map_nn_resolved"], "unresolved",
          st["map_nn_unresolved"])
    _assert_same_z(ze, _oracle_z(oa, cloud, queries), cloud, queries, what)
    assert st["map_nn_unresolved"] == 0 and st["map_nn_resolved"] == len(queries), st
    e.close()


@pytest.mark.parametrize("K", mc.K_COPIES)
def test_copies_beyond_one_page_of_the_tied_set(oa, K):
    cloud, queries = mc.copies_case(K)
    _check_nearest_z(oa, cloud, queries, f"{K} copies")


def test_twenty_tied_points_at_four_positions(oa):
    cloud, queries = mc.mixed_case()
    _check_nearest_z(oa, cloud, queries, "4 x 5 copies")


# ---- staircases: one engine and one oracle answer per cloud, shared by the boundary groups ---------------------------
@pytest.fixture(scope="module")
def stairs(oa):
    """descending -> (cloud, queries, owner, the oracle's z, the engine), made on first use and closed after the module's
    last test.  The engine answers per group, so that an error return or a wrong z names the boundary it belongs to."""
    made = {}

    def get(descending):
        if descending not in made:
            cloud, queries, owner = mc.staircase(descending)
            made[descending] = (cloud, queries, owner, _oracle_z(oa, cloud, queries), _engine(oa, cloud))
        return made[descending]

    yield get
    for case in made.values():
        case[4].close()


@pytest.mark.parametrize("group", list(mc.STAIR_GROUPS))
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_staircase_walks_to_the_depth_of_the_tie(stairs, descending, group):
    cloud, queries, owner, zo, e = stairs(descending)
    pick = np.isin(owner, mc.STAIR_GROUPS[group])
    before = e.stats()["map_nn_resolved"]
    t0 = time.perf_counter()
    ze = e.nearest_z(queries[pick])   # (raises unless the call returns TRG_OK)
    dt = time.perf_counter() - t0
    print(group, "depths", mc.STAIR_GROUPS[group], int(pick.sum()), "queries in", round(dt, 3), "s")
    _assert_same_z(ze, zo[pick], cloud, queries[pick], group)
    st = e.stats()
    assert st["map_nn_unresolved"] == 0 and st["map_nn_resolved"] - before == int(pick.sum()), st


@pytest.mark.parametrize("n", [mc.TOP - 1, mc.TOP, mc.TOP + 1])
def test_cloud_sizes_either_side_of_the_host_top(oa, n):
    cloud, queries = mc.edge_cloud(n)
    _check_nearest_z(oa, cloud, queries, f"{n} points")


def test_ties_found_after_the_radius_doubled_and_over_the_whole_grid(oa):
    cloud, inside, outside = mc.far_case()
    _check_nearest_z(oa, cloud, inside, "beyond robot_size")
    _check_nearest_z(oa, cloud, outside, "outside the map")


def _lattice_queries(n, seed):
    rng = np.random.default_rng(seed)
    ij = rng.integers(1, n - 2, (40, 2))
    return np.concatenate([(ij + [0.5, 0.0]) * mc.STEP, (ij + [0.0, 0.5]) * mc.STEP, (ij + 0.5) * mc.STEP]).astype(np.float32)


@pytest.mark.parametrize("kind", ["global", "local"])
def test_second_map_on_the_same_engine(oa, kind):
    """Two lattices of the same points in different orders: the tie winners follow the order, and the top of the first
    cloud's tree on the host must not answer for the second.  The second pair exceeds the top, so the device walks
    too."""
    import trg_planner
    e = trg_planner.Engine(**oa.MOUNTAIN)
    local = kind == "local"
    for n in (48, 96):
        queries = _lattice_queries(n, n)
        answers = []
        for seed in (1, 2):
            cloud = mc.lattice(n, mc.STEP, seed)
            if local:
                e.set_local_map([0.0, 0.0], cloud)
            else:
                e.set_global_map(cloud)
            ze = e.nearest_z(queries, kind=kind)
            _assert_same_z(ze, _oracle_z(oa, cloud, queries, local), cloud, queries, f"{kind} map, n {n}, order {seed}")
            answers.append(ze)
        # (the two orders do differ in their winners: the second map is not answered from the first by chance)
        assert (answers[0] != answers[1]).sum() >= len(queries) // 4
    assert e.stats()["map_nn_unresolved"] == 0
    e.close()


# ---- builds ----------------------------------------------------------------------------------------------------------
_builds = {}


def _build_case(oa, synth, name):
    if name not in _builds:
        which = mc.TWIN_BUILD if name == "twinned" else mc.COPIES_BUILD
        cloud = mc.twinned_cloud(synth) if name == "twinned" else mc.copies_cloud(synth)[0]
        o = mc.build_oracle(oa, which, cloud)
        _builds[name] = (which, cloud, o.graph(1), o.graph(0), o.counters()["samples"])
        o.close()
    return _builds[name]


@pytest.mark.parametrize("replay", ["device", "host"])
@pytest.mark.parametrize("name", ["twinned", "copies"])
def test_build_where_ties_pass_the_old_caps(oa, synth, name, replay):
    """twinned: every accepted sample ties, some 870 of them per level; copies: 3 % of the points carry 20 copies.
    The sampling launches keep a record per slot, so the device path builds both without a fallback: shown by
    used_device_bfs == 1 and, on the twinned cloud, by more records than 256 for every level -- one level at least was
    over the 256 that a launch once kept.  On the host replay of the twinned cloud every accepted sample is looked up, and
    they are more than 256 for every sampling launch: one chunk at least held more records than came back with it."""
    import trg_planner
    which, cloud, pre, glob, samples = _build_case(oa, synth, name)
    e = trg_planner.Engine(**mc.build_params(oa, which))
    e.set_sampler(mc.SEED, mc.TABLE_BITS)
    e.set_option("keep_preclean", 1)
    e.set_option("replay", replay)
    e.set_global_map(cloud)
    t0 = time.perf_counter()
    e.init_graph(which["start"])
    dt = time.perf_counter() - t0
    st = e.stats()
    print(name, replay, "init_graph", round(dt, 3), "s; V", pre.V, "levels", st["bfs_levels"], "records",
          st["map_tie_records"], "unread", st["map_tie_unread"], "resolved", st["map_nn_resolved"], "fallback",
          repr(e.fallback_reason), "sampling launches", st["launches_sample_kernel"], "oracle's samples", samples)
    assert_graph_equal(e.graph("preclean"), pre, 1e-5)
    assert_graph_equal(e.graph("global"), glob, 1e-5)
    assert st["map_nn_unresolved"] == 0, st
    assert st["used_device_bfs"] == (1 if replay == "device" else 0), e.fallback_reason
    if replay == "device":
        assert st["bfs_fallbacks"] == 0, e.fallback_reason
        if name == "twinned":
            assert st["bfs_levels"] > 0 and st["map_tie_records"] > mc.RECORD_CAP * st["bfs_levels"], st
    if replay == "host" and name == "twinned":
        assert st["map_nn_resolved"] >= samples > mc.RECORD_CAP * st["launches_sample_kernel"] > 0, st
    assert st["map_nn_resolved"] > (1000 if name == "twinned" else 20), st
    e.close()
