"""GPU: option tail_early_copy gives the graph of tail_early_copy=0, bit for bit.

With tail_early_copy=1 (the default) a plain device build (tail_overlap=1, no step 3, no keep_preclean)
  - expands the node container's iteration order on the device from its runs (no vector of V ids on the host),
  - renumbers and lays out xyz / state in front of k_fin_scatter and sends xyz, state, cid and rowptr to the host on a
    copy stream while the main stream fills and orders the rows; col / dist and w follow behind their events,
  - reduces "first successful call of a pair" over the round-2 calls only (a pair's first call is its edge when it
    succeeded), without a table-wide clear of ok_seq,
  - scatters no weights into F.w, which nothing reads there.
With 0 the tail keeps the order it had.  Every comparison below is 1 against 0 over all seven arrays
Engine.graph("global") hands out, floats as their bit patterns, and w must not be all zero.

Clouds: the benchmark's `small` workload (400 x 400 lattice points, S = 16), and ROUGH, a 200 x 200 cloud of steep
terrain under mountain.yaml parameters (S = 7) whose reference build has Invalid nodes, nodes that cleanGraph drops
and pairs whose first wireEdge call failed and a later one succeeded (asserted on the oracle, without a GPU, in
test_rough_cloud_has_what_the_tail_must_handle).  The seed was picked on the CPU from seeds 1..11: seed 3 gives 1589
nodes before cleanGraph, 141 of them Invalid and dropped, and 8 such pairs.
"""
import numpy as np
import pytest

from graph_support import obs_crop

SEED = 20250418  # bench.py's default terrain seed
PRM = dict(expand_dist=0.6, robot_size=0.3, height_threshold=0.16, collision_threshold=0.1,
           update_collision_threshold=0.5, safety_factor=3.0, goal_tolerance=0.8, sample_num=16)
ROUGH = dict(n=200, seed=3, amplitude=5.0, wavelength=14.0, start=[10.0, 10.0, 0.0])
NAMES = ("rowptr", "col", "state", "cid", "xyz", "dist", "w")


@pytest.fixture(scope="module")
def small(synth):
    cloud = synth.mountain_tile(0, 400, 0, 400, seed=SEED)
    return cloud, [20.0, 20.0, 0.0]


@pytest.fixture(scope="module")
def rough(synth):
    cloud = synth.mountain_cloud(ROUGH["n"], ROUGH["n"], seed=ROUGH["seed"], amplitude=ROUGH["amplitude"],
                                 wavelength=ROUGH["wavelength"])
    return cloud, ROUGH["start"]


@pytest.fixture(scope="module")
def rough_oracle(oa, rough):
    """The reference build of ROUGH with its wireEdge evaluations traced -> (graph before cleanGraph, after, trace)."""
    cloud, start = rough
    o = oa.Oracle(**oa.MOUNTAIN)
    o.set_sampler(7, 0, 16)
    o.set_trace(True)
    o.set_global_map(cloud)
    assert o.init_graph(start)
    out = (o.graph(1), o.graph(0), o.trace())
    o.close()
    return out


def _engine(cloud, prm=PRM, **options):
    import trg_planner
    e = trg_planner.Engine(**prm)
    e.set_sampler(7, 16)
    for k, v in options.items():
        e.set_option(k, v)
    e.set_global_map(cloud)
    return e


def _build(e, start):
    e.init_graph(start)
    st = e.stats()
    assert st["bfs_fallbacks"] == 0 and st["used_device_bfs"] == 1, e.fallback_reason
    return e.graph("global"), st


def _assert_identical(a, b, what, min_v=100):
    assert (a.V, a.E) == (b.V, b.E), (what, a.V, b.V, a.E, b.E)
    assert a.V >= min_v and a.E >= a.V, (what, a.V, a.E)
    for name in NAMES:
        x, y = getattr(a, name), getattr(b, name)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        differ = int((x != y).sum())
        assert differ == 0, (what, name, differ)
    assert int((a.w != 0).sum()) > 0, (what, "the comparison of w must not pass on zeros alone")


def _pair(cloud, start, prm=PRM, **options):
    """-> ([graph with tail_early_copy=1, graph with 0], [their stats])"""
    graphs, stats = [], []
    for early in (1, 0):
        e = _engine(cloud, prm, tail_early_copy=early, **options)
        g, st = _build(e, start)
        e.close()
        graphs.append(g)
        stats.append(st)
    return graphs, stats


@pytest.fixture(scope="module")
def small_reference(small):
    """The `small` graph with tail_early_copy=0: what cases 1, 4 (first build), 6 and 8 compare with."""
    cloud, start = small
    e = _engine(cloud, tail_early_copy=0)
    g, _ = _build(e, start)
    e.close()
    return g


def test_rough_cloud_has_what_the_tail_must_handle(rough_oracle):
    """CPU: the three properties the rough cloud was picked for, on the oracle."""
    pre, clean, tr = rough_oracle
    invalid = int((pre.state == -1).sum())
    dropped = pre.V - clean.V
    failed, late = set(), 0
    lo, hi = np.minimum(tr["src"], tr["dst"]).astype(np.int64), np.maximum(tr["src"], tr["dst"]).astype(np.int64)
    for key, status in zip((lo * (1 << 32) + hi).tolist(), tr["status"].tolist()):
        if status != 0:  # the reference evaluates a pair's calls until one succeeds (trg.cpp:255-267)
            failed.add(key)
        elif key in failed:
            late += 1
            failed.discard(key)
    print(f"rough: {pre.V} nodes, {invalid} Invalid, {dropped} dropped by cleanGraph, "
          f"{late} pairs wired by a later call after their first one failed")
    assert invalid >= 1 and dropped >= 1 and late >= 1, (invalid, dropped, late)


def test_option_values():
    """CPU: tail_early_copy takes 0 or 1 and nothing else (set_option needs no device)."""
    import ctypes as C
    import trg_planner
    from trg_planner._engine import TrgParams
    trg_planner.build_library()
    L = trg_planner.load_library()
    prm = TrgParams(0, 0.6, 0.3, 8, 0.3, 0.2, 0.5, 1.0, 0.5)
    h = C.c_void_p()
    st = L.trg_engine_create(C.byref(prm), 0, C.byref(h))
    assert h.value and st in (0, 4), st  # (4: no device here)
    try:
        for v in (b"0", b"1"):
            assert L.trg_engine_set_option(h, b"tail_early_copy", v) == 0, v
        for v in (b"2", b"", b"on"):
            assert L.trg_engine_set_option(h, b"tail_early_copy", v) == 1, v
            assert L.trg_engine_last_error(h) == b"tail_early_copy must be 0 or 1"
    finally:
        L.trg_engine_destroy(h)


@pytest.mark.gpu
def test_small_plain(small, small_reference):
    cloud, start = small
    e = _engine(cloud, tail_early_copy=1)
    g, _ = _build(e, start)
    e.close()
    print(f"small: V {g.V} E {g.E}, {int((g.w != 0).sum())} non-zero weights")
    _assert_identical(g, small_reference, "small", min_v=1000)


@pytest.mark.gpu
def test_rough_cloud_round_two(rough, rough_oracle):
    """Invalid nodes, dropped nodes and pairs whose edge is NOT their first call: the graphs are equal, equal to the
    live oracle's, and round 2 of the deferred evaluations really kept calls.  The engine has no counter for that;
    with defer_overlap=0 the whole call log (under one evaluation batch of 4 M calls) is round 1's single evaluation
    launch, and a second launch is made iff round 2 kept at least one call."""
    from conftest import assert_graph_equal
    cloud, start = rough
    (on, off), _ = _pair(cloud, start, prm=dict(PRM, sample_num=7))
    _assert_identical(on, off, "rough")
    assert_graph_equal(on, rough_oracle[1], 1e-5)
    (on2, off2), stats = _pair(cloud, start, prm=dict(PRM, sample_num=7), defer_overlap=0)
    for st in stats:
        assert st["launches_edge_kernel"] == 2, st["launches_edge_kernel"]
    _assert_identical(on2, off2, "rough, defer_overlap=0")
    _assert_identical(on2, on, "rough, defer_overlap=0 against 1")


@pytest.mark.gpu
def test_graph_of_the_root_alone(small):
    """expand_dist < robot_size: every sample merges into the root, which has no edge and is dropped (V == 1,
    E == 0 before cleanGraph, Vn == 0): no copy is enqueued, both orders hand out the empty graph."""
    cloud, start = small
    for early in (1, 0):
        e = _engine(cloud, dict(PRM, expand_dist=0.25), tail_early_copy=early)
        e.init_graph(start)
        st = e.stats()
        assert st["used_device_bfs"] == 1 and st["bfs_fallbacks"] == 0, e.fallback_reason
        assert st["created_nodes"] == 1, st["created_nodes"]
        g = e.graph("global")
        assert (g.V, g.E) == (0, 0) and g.rowptr.tolist() == [0], (early, g.V, g.E)
        e.close()


@pytest.mark.gpu
def test_three_builds_alternating_on_one_engine(small):
    """Stale buffers, shrinking then growing sizes: three roots, the option flipped between builds."""
    cloud, start = small
    starts = [start, [start[0] + 3.0, start[1] - 2.0, 0.0], [start[0] - 4.0, start[1] + 5.0, 0.0]]
    a, b = _engine(cloud), _engine(cloud)
    seen = []
    for i, st in enumerate(starts):
        a.set_option("tail_early_copy", 1 - i % 2)  # 1, 0, 1
        b.set_option("tail_early_copy", i % 2)      # 0, 1, 0
        ga, _ = _build(a, st)
        gb, _ = _build(b, st)
        _assert_identical(ga, gb, f"build {i}", min_v=1000)
        seen.append(ga)
    a.close()
    b.close()
    for i in (1, 2):  # (the three graphs differ: a stale array would show)
        assert seen[i].E != seen[0].E or not np.array_equal(seen[i].w.view(np.uint32), seen[0].w.view(np.uint32))


@pytest.mark.gpu
def test_host_replayed_levels(small):
    """debug_tie_every=3: every third level is replayed on the host, which writes those levels' call records --
    the writer the round-2-only reduction has to be safe against."""
    cloud, start = small
    (on, off), stats = _pair(cloud, start, debug_tie_every=3)
    for st in stats:
        assert st["bfs_host_levels"] >= 5, st["bfs_host_levels"]
    _assert_identical(on, off, "host-replayed levels", min_v=1000)


@pytest.mark.gpu
@pytest.mark.parametrize("options", [dict(keep_preclean=1), dict(tail_overlap=0)], ids=["keep_preclean", "tail_overlap0"])
def test_builds_that_keep_the_earlier_order(small, small_reference, options):
    """keep_preclean=1 and tail_overlap=0 take the earlier order whatever the option says: equal to each other and
    to the plain build."""
    cloud, start = small
    (on, off), _ = _pair(cloud, start, **options)
    _assert_identical(on, off, str(options), min_v=1000)
    _assert_identical(on, small_reference, str(options) + " against the plain build", min_v=1000)


@pytest.mark.gpu
def test_update_after_the_build(small):
    """The host's node state is rebuilt from the early copies: one setLocalMap + updateGraph on top of it."""
    cloud, start = small
    local = np.ascontiguousarray(obs_crop(cloud, start, 4.0, box=(start[0] + 1.5, start[1] + 1.0, 0.5)))
    graphs = []
    for early in (1, 0):
        e = _engine(cloud, tail_early_copy=early)
        _build(e, start)
        e.set_local_map(start[:2], local)
        e.update_graph()
        graphs.append(e.graph("global"))
        e.close()
    _assert_identical(graphs[0], graphs[1], "after update_graph", min_v=1000)


@pytest.mark.gpu
def test_more_runs_than_the_device_takes(small, small_reference):
    """debug_order_run_cap=1: the container's order has more runs than the cap, so the host expands and uploads it
    as before; the rest of the early-copy tail runs on it."""
    cloud, start = small
    e = _engine(cloud, tail_early_copy=1, debug_order_run_cap=1)
    g, _ = _build(e, start)
    e.close()
    _assert_identical(g, small_reference, "host expansion of the order", min_v=1000)
