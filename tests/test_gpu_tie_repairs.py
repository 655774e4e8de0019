"""GPU: repairs of the level loop's rare events that the graph does not read (option lazy_tie_repair).

An accepted sample whose nearest MAP point is not unique gets the lowest cloud index on the device; the host
looks up the reference's choice (tests/test_gpu_map_ties.py).  The sample's z is read only where the sample
becomes a node, so the level loop looks up only those records -- and, once one tied candidate of a level
created a node, every tied candidate of that level, because the rerun of the commit may let another one create.
Records it left alone are repaired before anything decides the level's commit again (ticketed repeats, gate
redos, node-tie fixers, host replays).  These builds have thousands of such ties, alone and together with the
other repairs, and must equal the CPU oracle's graphs; the counters say the lookups were in fact left out.

The twin clouds restate the construction of tests/test_gpu_map_ties.py: a fraction of the points duplicated at
the same (x, y) with another z."""
import numpy as np
import pytest

from conftest import assert_graph_equal

gpu = pytest.mark.gpu


def _twin_cloud(synth, n, frac, seed=5, **cloud_kw):
    """-> cloud, xy of the twinned points"""
    base = synth.mountain_cloud(n, n, seed=seed, **cloud_kw)
    rng = np.random.default_rng(seed)
    pick = rng.choice(base.shape[0], int(frac * base.shape[0]), replace=False)
    dup = base[pick].copy()
    dup[:, 2] += rng.uniform(0.01, 0.04, dup.shape[0]).astype(np.float32)   # same x, y; other z
    cloud = np.concatenate([base, dup])
    return cloud[rng.permutation(cloud.shape[0])], base[pick, :2].copy()


CASES = {
    # name: cloud side, twinned fraction, cloud keywords, sample_num, sampler (seed, table bits), start
    "sparse": (120, 0.03, {}, 7, (7, 16), [6.0, 6.0, 0.0]),
    "dense": (150, 0.10, {}, 16, (7, 16), [7.5, 7.5, 0.0]),
    "replays": (150, 0.05, {}, 10, (21, 16), [7.5, 7.5, 0.0]),
    "node_ties": (150, 0.05, {"amplitude": 0.3}, 8, (33, 4), [7.5, 7.5, 0.0]),
}
_oracle_runs = {}


def _case(oa, synth, name):
    """The case's cloud and the oracle's build on it, computed once per session.
    -> dict(cloud, twins, prm, sampler, start, pre, glob, counters)"""
    if name not in _oracle_runs:
        n, frac, kw, sample_num, sampler, start = CASES[name]
        cloud, twins = _twin_cloud(synth, n, frac, **kw)
        prm = dict(oa.MOUNTAIN, sample_num=sample_num)
        o = oa.Oracle(**prm)
        o.set_sampler(sampler[0], 0, sampler[1])
        o.set_global_map(cloud)
        assert o.init_graph(start)
        _oracle_runs[name] = dict(cloud=cloud, twins=twins, prm=prm, sampler=sampler, start=start,
                                  pre=o.graph(1), glob=o.graph(0), counters=o.counters())
        o.close()
    return _oracle_runs[name]


def _build(case, **options):
    import trg_planner
    e = trg_planner.Engine(**case["prm"])
    e.set_sampler(*case["sampler"])
    e.set_option("keep_preclean", 1)
    for k, v in options.items():
        e.set_option(k, v)
    e.set_global_map(case["cloud"])
    e.init_graph(case["start"])
    st = e.stats()
    assert st["used_device_bfs"] == 1 and st["bfs_fallbacks"] == 0, e.fallback_reason
    assert st["map_nn_unresolved"] == 0, st
    assert_graph_equal(e.graph("preclean"), case["pre"], 1e-5)
    assert_graph_equal(e.graph("global"), case["glob"], 1e-5)
    return st


def _nodes_on_twins(case):
    """Nodes of the oracle's graph before cleanGraph whose nearest map (x, y) is a twinned one."""
    cloud = case["cloud"].astype(np.float64)
    twinned = np.zeros(cloud.shape[0], bool)
    key = {(float(x), float(y)) for x, y in case["twins"]}
    for k, p in enumerate(case["cloud"]):
        twinned[k] = (float(p[0]), float(p[1])) in key
    count = 0
    for p in case["pre"].xyz.astype(np.float64):
        d2 = (cloud[:, 0] - p[0]) ** 2 + (cloud[:, 1] - p[1]) ** 2
        count += bool(twinned[int(np.argmin(d2))])
    return count


@gpu
def test_sparse_ties_are_looked_up_only_where_a_node_reads_them(oa, synth):
    """V = 851, 5 957 accepted samples, ~180 of them tied, 22 created nodes on a twinned point."""
    case = _case(oa, synth, "sparse")
    assert case["pre"].V == 851 and case["counters"]["samples"] == 5957
    on_twins = _nodes_on_twins(case)
    assert on_twins >= 10
    st = _build(case)
    print("sparse: records", st["map_tie_records"], "unread", st["map_tie_unread"], "resolved",
          st["map_nn_resolved"], "nodes on twins", on_twins)
    assert 0 < st["map_tie_unread"] < st["map_tie_records"], st
    assert st["map_nn_resolved"] >= on_twins, (st["map_nn_resolved"], on_twins)
    assert st["map_nn_resolved"] < st["map_tie_records"], st
    eager = _build(case, lazy_tie_repair=0)  # (the same graphs: _build compares both with the oracle's)
    assert eager["map_tie_unread"] == 0 and eager["map_tie_records"] == st["map_tie_records"], eager


@gpu
def test_dense_ties_one_creator_repairs_its_level(oa, synth):
    """V = 1 558, 24 912 samples, ~2 500 tied, ~150 tied creators, 1 Invalid node: nearly every level has a tie
    on a slot that created a node, so all its candidate records are repaired and the commit is redone."""
    case = _case(oa, synth, "dense")
    c = case["counters"]
    assert case["pre"].V == 1558 and c["samples"] == 24912
    st = _build(case)
    assert st["created_nodes"] == c["created"] and st["invalid_nodes"] == c["invalid_created"], (st, c)
    assert st["map_tie_records"] > 1000 and st["map_tie_unread"] > 0, st


@gpu
def test_ties_with_host_replays_repair_skipped_records_first(oa, synth):
    """V = 1 409, E = 11 902.  Every third level is taken back and replayed on the host while tie records of
    candidates that did not create are pending: the replay decides anew who creates and must find them repaired."""
    case = _case(oa, synth, "replays")
    assert (case["pre"].V, case["glob"].E) == (1409, 11902)
    st = _build(case, debug_tie_every=3)
    assert st["bfs_host_levels"] >= 3, st
    assert st["map_tie_records"] > 0, st


@gpu
@pytest.mark.parametrize("tie_inplace", [1, 0])
def test_ties_with_natural_node_ties(oa, synth, tie_inplace):
    """V = 1 151, E = 8 020, 55 tied creators, on a 4-bit sampler table whose few directions make exact
    node-distance ties: the pinned node mirror, the batched in-place settle and the pre-level fixer, with
    skipped map-tie records on the same levels."""
    case = _case(oa, synth, "node_ties")
    assert (case["pre"].V, case["glob"].E) == (1151, 8020)
    st = _build(case, tie_inplace=tie_inplace)
    assert st["nn_ties"] > 0 and st["bfs_tie_fixups"] > 0 and st["map_tie_records"] > 0, st


def test_tie_statistics_are_appended_and_start_at_zero():
    """map_tie_records and map_tie_unread end TrgStats, in this order (the struct only grows at its end)."""
    import ctypes as C

    import trg_planner
    from trg_planner._engine import TrgParams, TrgStats
    names = [f[0] for f in TrgStats._fields_]
    assert names[-2:] == ["map_tie_records", "map_tie_unread"]
    assert names[-3] == "start_discs_known"
    fresh = TrgStats()
    assert fresh.map_tie_records == 0 and fresh.map_tie_unread == 0
    trg_planner.build_library()
    L = trg_planner.load_library()
    prm = TrgParams(0, 0.6, 0.3, 8, 0.3, 0.2, 0.5, 1.0, 0.5)
    h = C.c_void_p()
    st = L.trg_engine_create(C.byref(prm), 0, C.byref(h))
    assert h.value and st in (0, 4), (st, L.trg_engine_last_error(h))
    try:
        out = TrgStats()
        out.map_tie_records = out.map_tie_unread = 77  # (the call must write the whole struct)
        assert L.trg_engine_get_stats(h, C.byref(out)) == 0
        assert out.map_tie_records == 0 and out.map_tie_unread == 0
        for v in (b"0", b"1"):
            assert L.trg_engine_set_option(h, b"lazy_tie_repair", v) == 0
        assert L.trg_engine_set_option(h, b"lazy_tie_repair", b"2") == 1
        assert L.trg_engine_last_error(h) == b"lazy_tie_repair must be 0 or 1"
    finally:
        L.trg_engine_destroy(h)
