"""GPU: the two orders of the build's tail give the same graph, bit for bit.

With tail_overlap=1 (the default) a plain device build lays the cleaned graph out first, sends xyz, state, cid,
rowptr, col and dist to the host and computes the weights of the edges that created the nodes (k_node_cov,
k_node_weights) on the second stream meanwhile; a pass over the cleaned rows then writes w alone and w is the
last copy.  With tail_overlap=0 the weights are computed in front of the deferred calls and travel through
k_fin_scatter and k_fin_clean_copy with everything else.  Builds with keep_preclean=1 (and with expandGraph's
step 3) take that order whatever the option says; the suites that compare with the oracle mostly set
keep_preclean and so pin it, and this file ties the new order to it.

Clouds: the benchmark's `small` workload (400 x 400 lattice points, S = 16) and a 1 000 x 1 000 cloud of the same
terrain.  Every comparison is of all seven arrays Engine.graph("global") hands out, floats as their bit patterns.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20250418  # bench.py's default terrain seed
PRM = dict(expand_dist=0.6, robot_size=0.3, height_threshold=0.16, collision_threshold=0.1,
           update_collision_threshold=0.5, safety_factor=3.0, goal_tolerance=0.8, sample_num=16)
CLOUDS = {"small": 400, "1M": 1000}


@pytest.fixture(scope="module", params=list(CLOUDS))
def workload(request, synth):
    n = CLOUDS[request.param]
    cloud = synth.mountain_tile(0, n, 0, n, seed=SEED)
    assert cloud.shape == (n * n, 3)
    centre = 0.05 * n  # 0.1 m lattice
    return request.param, cloud, [centre, centre, 0.0]


def _engine(cloud, **options):
    import trg_planner
    e = trg_planner.Engine(**PRM)
    e.set_sampler(7, 16)
    for k, v in options.items():
        e.set_option(k, v)
    e.set_global_map(cloud)
    return e


def _build(e, start, device=True):
    e.init_graph(start)
    st = e.stats()
    assert st["bfs_fallbacks"] == 0, e.fallback_reason
    assert st["used_device_bfs"] == (1 if device else 0), e.fallback_reason
    return e.graph("global"), st


def _assert_identical(a, b, what):
    assert (a.V, a.E) == (b.V, b.E), (what, a.V, b.V, a.E, b.E)
    assert a.V > 1000 and a.E > 10000, (what, a.V, a.E)
    for name in ("rowptr", "col", "state", "cid"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), (what, name)
    for name in ("xyz", "dist", "w"):
        x, y = getattr(a, name).view(np.uint32), getattr(b, name).view(np.uint32)
        differ = int((x != y).sum())
        assert differ == 0, (what, name, differ)


def _pair(cloud, start, **options):
    graphs, stats = [], []
    for overlap in (1, 0):
        e = _engine(cloud, tail_overlap=overlap, **options)
        g, st = _build(e, start)
        e.close()
        graphs.append(g)
        stats.append(st)
    return graphs, stats


def test_plain_build(workload):
    name, cloud, start = workload
    (on, off), _ = _pair(cloud, start)
    nonzero = int((on.w != 0).sum())
    print(f"{name}: V {on.V} E {on.E}, {nonzero} non-zero weights")
    assert nonzero > 0, "the comparison of w must not pass on zeros alone"
    _assert_identical(on, off, name)


def test_host_replayed_levels(workload):
    """debug_tie_every=3: every third level is replayed on the host, which supplies those nodes' NodeCov (or the
    weight itself, w_given)."""
    name, cloud, start = workload
    (on, off), stats = _pair(cloud, start, debug_tie_every=3)
    for st in stats:
        assert st["bfs_host_levels"] >= 5, st["bfs_host_levels"]
    _assert_identical(on, off, name)


def test_host_build_then_device_build_on_one_engine(workload):
    name, cloud, start = workload
    host_graphs, device_graphs = [], []
    for overlap in (1, 0):
        e = _engine(cloud, tail_overlap=overlap)
        e.set_option("replay", "host")
        host_graphs.append(_build(e, start, device=False)[0])
        e.set_option("replay", "device")
        device_graphs.append(_build(e, start)[0])
        e.close()
    _assert_identical(host_graphs[0], host_graphs[1], name + ": host builds")
    _assert_identical(device_graphs[0], device_graphs[1], name + ": device builds after a host build")


def test_three_builds_alternating_on_one_engine(workload):
    """The device buffers are reused from build to build: w2 of the previous build must not survive in the next.
    Three different roots give three different graphs."""
    name, cloud, start = workload
    starts = [start, [start[0] + 3.0, start[1] - 2.0, 0.0], [start[0] - 4.0, start[1] + 5.0, 0.0]]
    a, b = _engine(cloud), _engine(cloud)
    seen = []
    for i, st in enumerate(starts):
        a.set_option("tail_overlap", 1 - i % 2)  # 1, 0, 1
        b.set_option("tail_overlap", i % 2)      # 0, 1, 0
        ga, _ = _build(a, st)
        gb, _ = _build(b, st)
        _assert_identical(ga, gb, f"{name}: build {i}")
        seen.append(ga)
    a.close()
    b.close()
    for i in (1, 2):  # (the three graphs differ: a stale array would show)
        assert seen[i].E != seen[0].E or not np.array_equal(seen[i].w.view(np.uint32), seen[0].w.view(np.uint32))


def test_keep_preclean_takes_the_old_order_with_either_value(workload):
    name, cloud, start = workload
    graphs, pres = [], []
    for overlap in (1, 0):
        e = _engine(cloud, tail_overlap=overlap, keep_preclean=1)
        g, _ = _build(e, start)
        pre = e.graph("preclean")
        e.close()
        # cleanGraph drops nodes without edges and keeps every edge in its row's order: row k of the cleaned
        # graph is row cid[k] of the graph before it, columns renumbered, weights the same floats
        lo, hi = pre.rowptr[g.cid], pre.rowptr[g.cid + 1]
        assert np.array_equal(hi - lo, np.diff(g.rowptr)), name
        src = np.repeat(lo - g.rowptr[:-1], np.diff(g.rowptr)) + np.arange(g.E)
        assert np.array_equal(pre.col[src], g.cid[g.col]), name
        assert np.array_equal(pre.w[src].view(np.uint32), g.w.view(np.uint32)), name
        assert np.array_equal(pre.dist[src].view(np.uint32), g.dist.view(np.uint32)), name
        graphs.append(g)
        pres.append(pre)
    _assert_identical(graphs[0], graphs[1], name + ": cleaned")
    _assert_identical(pres[0], pres[1], name + ": before cleanGraph")
    # ... and the new order (no keep_preclean) gives that graph too
    e = _engine(cloud, tail_overlap=1)
    g, _ = _build(e, start)
    e.close()
    _assert_identical(g, graphs[0], name + ": tail_overlap=1 against keep_preclean=1")
