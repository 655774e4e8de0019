"""The deferred pipeline's round-1 selection in one launch (k_calls_select_append) and the expansion time from
device timestamps.

The selection appends the first call of every pair to the batch's list in whatever order the workgroups reach
the count word.  Nothing may depend on that order: record q of an evaluation is call list[q], every result is
stored under its call number, the statistics are sums.  So the graphs below must equal the CPU oracle's bit for
bit (structure) and the oracle's fp64-covariance witness bit for bit (weights), through every way a batch is
issued: several batches beside the level loop, one batch after it (a call log shorter than DEF_BATCH_MIN; the
step-3 configuration), and the sparse call log with CALL_NONE holes inside every batch.
"""
import numpy as np
import pytest

from conftest import assert_graph_equal
from test_gpu_parity import MOUNTAIN_S16, WEIGHT_TOL, _build_both, _engine

pytestmark = pytest.mark.gpu

DEF_BATCH_MIN = 6000  # trg_engine_bfs.inc: calls of finished levels are handed over beside the loop from this many on
START = [15.0, 15.0, 0.0]
CROP_START = [4.0, 4.0, 0.0]


def _crop(mountain_small):
    # the corner x, y < 8 m of the 30 m x 30 m cloud (6 484 points): the oracle creates 342 nodes on it, 312 of them
    # survive cleanGraph, and the 312 it expands make 312 x 7 = 2 184 wireEdge calls, well below DEF_BATCH_MIN
    keep = (mountain_small[:, 0] < 8.0) & (mountain_small[:, 1] < 8.0)
    return np.ascontiguousarray(mountain_small[keep])


def _case(oa, request, name):
    """cloud, parameters, start, options of the engine"""
    if name == "mountain_small_S7":
        return request.getfixturevalue("mountain_small"), dict(oa.MOUNTAIN), START, {}
    if name == "mountain_gentle_S16":
        return request.getfixturevalue("mountain_gentle"), dict(oa.MOUNTAIN, sample_num=16), START, {}
    if name == "crop_after_loop_only":
        return _crop(request.getfixturevalue("mountain_small")), dict(oa.MOUNTAIN), CROP_START, {}
    if name == "indoor_step3":
        return request.getfixturevalue("indoor_small"), dict(oa.INDOOR), [1.5, 1.5, 0.0], {}
    assert name == "sparse_call_log"
    return request.getfixturevalue("mountain_small"), dict(MOUNTAIN_S16), START, {"debug_call_stride": 1}


def _device_build(prm, cloud, start, seed=7, **options):
    e = _engine(prm)
    e.set_sampler(seed, 16)
    for k, v in options.items():
        e.set_option(k, v)
    e.set_global_map(cloud)
    e.init_graph(start)
    st = e.stats()
    assert st["used_device_bfs"] == 1 and st["bfs_fallbacks"] == 0, e.fallback_reason
    return e, st


@pytest.mark.parametrize("name", ["mountain_small_S7", "mountain_gentle_S16", "crop_after_loop_only",
                                  "indoor_step3", "sparse_call_log"])
def test_parity_with_the_live_oracle(oa, request, name):
    cloud, prm, start, options = _case(oa, request, name)
    if options:  # (_build_both sets no options)
        e, _ = _device_build(prm, cloud, start, keep_preclean=1, **options)
        o = oa.Oracle(**prm)
        o.set_sampler(7, 0, 16)
        o.set_global_map(cloud)
        assert o.init_graph(start)
    else:
        e, o = _build_both(oa, prm, cloud, start, seed=7)
    st = e.stats()
    assert st["used_device_bfs"] == 1 and st["bfs_fallbacks"] == 0, e.fallback_reason
    assert_graph_equal(e.graph("preclean"), o.graph(1), WEIGHT_TOL)
    ge, go = e.graph("global"), o.graph(0)
    assert_graph_equal(ge, go, WEIGHT_TOL)
    # the oracle's second witness (covariance accumulated in fp64, as the engine does): the same floats
    o2 = oa.Oracle(**prm)
    o2.set_sampler(7, 0, 16)
    o2.set_cov_f64(True)
    o2.set_global_map(cloud)
    assert o2.init_graph(start)
    g2 = o2.graph(0)
    assert np.array_equal(g2.col, ge.col)
    assert np.array_equal(ge.w.view(np.uint32), g2.w.view(np.uint32)), float(np.abs(ge.w - g2.w).max())
    c = o.counters()
    assert st["created_nodes"] == c["created"] and st["invalid_nodes"] == c["invalid_created"]
    calls = st["expanded_nodes"] * prm["sample_num"]
    if name in ("mountain_small_S7", "mountain_gentle_S16"):
        # slots per level are no multiple of 64 or 256 (S = 7, 16 with odd frontier sizes), several batches beside the loop
        assert st["launches_edge_kernel"] >= 3, st["launches_edge_kernel"]
    elif name == "crop_after_loop_only":
        assert go.V > 50, go.V
        assert calls < DEF_BATCH_MIN, calls
        assert 1 <= st["launches_edge_kernel"] <= 2, st["launches_edge_kernel"]  # round 1 in one batch, round 2 if any
    elif name == "indoor_step3":
        assert 1 <= st["launches_edge_kernel"] <= 2, st["launches_edge_kernel"]  # nothing beside the loop with step 3
    else:
        assert st["launches_edge_kernel"] >= 3, st["launches_edge_kernel"]


def _arrays(g):
    return (np.array([g.V, g.E]), g.xyz, g.state, g.cid, g.rowptr, g.col, g.w, g.dist)


def test_overlap_off_and_on_build_the_same_bytes(mountain_small):
    """defer_overlap=0 sends the whole call log through the selection after the loop, in the main stream; 1 hands it
    over batch by batch beside the loop.  Same graph, byte for byte, and the same sums -- in three builds each: the
    append order differs from run to run, the results must not."""
    keys = ("edge_evals_gpu", "bytes_edge_kernel", "created_nodes")
    seen = {}
    for overlap in (0, 1):
        runs = []
        for _ in range(3):
            # (a fresh engine per build: cleanGraph's renumbering follows the reference's node container, whose
            # bucket history an engine carries from one build to the next)
            e = _engine(dict(MOUNTAIN_S16))
            e.set_sampler(7, 16)
            e.set_option("defer_overlap", overlap)
            e.set_global_map(mountain_small)
            e.init_graph(START)
            st = e.stats()
            assert st["used_device_bfs"] == 1 and st["bfs_fallbacks"] == 0, e.fallback_reason
            runs.append((_arrays(e.graph("global")), tuple(st[k] for k in keys), st["launches_edge_kernel"]))
            e.close()
        seen[overlap] = runs
    assert seen[1][0][2] >= 3 and seen[0][0][2] <= 2, (seen[1][0][2], seen[0][0][2])
    ref_arrays, ref_stats, _ = seen[0][0]
    assert ref_stats[0] > 0 and ref_stats[1] > 0
    for overlap in (0, 1):
        for arrays, stats, _ in seen[overlap]:
            assert stats == ref_stats, (overlap, stats, ref_stats)
            for a, b in zip(arrays, ref_arrays):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# launches_sample_kernel of the two builds below as the parent commit reports them (read once from a build of the
# parent's library on an MI355X): one expansion per BFS level, the stalled level's repeat adds none
PARENT_LAUNCHES_SAMPLE_KERNEL = {"plain": 79, "stalled": 79}


@pytest.mark.parametrize("kind", ["plain", "stalled"])
def test_expansion_time_comes_from_the_device_clock(oa, mountain_small, kind):
    """ms_sample_kernel is the sum over all levels of (first resolve workgroup starts) - (first sampling workgroup
    starts) in ticks of the device's wall clock: positive, and inside the level loop's own wall time.  With
    debug_stall_level resolve runs twice on one level; the repeat finds the stamp cleared and adds nothing."""
    prm = dict(oa.MOUNTAIN, sample_num=10)
    options = {"debug_stall_level": 9, "debug_wait_rerun": 0} if kind == "stalled" else {}
    e, st = _device_build(prm, mountain_small, START, seed=21, **options)
    if kind == "stalled":
        assert st["bfs_ticket_reruns"] == 1, st["bfs_ticket_reruns"]
    print(f"{kind}: ms_sample_kernel {st['ms_sample_kernel']:.4f} ms_bfs_loop {st['ms_bfs_loop']:.4f} "
          f"launches_sample_kernel {st['launches_sample_kernel']} bfs_levels {st['bfs_levels']}")
    assert 0 < st["ms_sample_kernel"] <= st["ms_bfs_loop"], (st["ms_sample_kernel"], st["ms_bfs_loop"])
    assert st["launches_sample_kernel"] == PARENT_LAUNCHES_SAMPLE_KERNEL[kind], st["launches_sample_kernel"]
