"""GPU: trg_engine_stitch_exchange's own logic with 2, 3, 4 and 9 ranks -- per-rank counts and padded slots, the
node count in the count exchange, rec_off / node_off, the second exchange on the first one's buffers, the failure
announcement -- over the in-process transport (trg_engine_comm_join_local): one process, one engine and one
thread per rank, all on one device.  The kernels and their inputs are those of tiled.stitch_emulated, only the data
movement differs, so every rank's rows must equal the emulated ones bit for bit, weights included; through
test_gpu_stitch_steps.py those equal the tiled oracle's.  RCCL itself with more than one rank is not run here (it
refuses two ranks on one device)."""
import itertools
import threading
import time

import numpy as np
import pytest

import stitch_cases as sc

pytestmark = pytest.mark.gpu
INVALID_ARG, NO_MAP, DEVICE = 1, 2, 4
JOIN_SECONDS = 60
_group = itertools.count()


@pytest.fixture(scope="module")
def tiled():
    from trg_planner import tiled as t
    return t


def join_group(engines, tag):
    name = f"test-exchange-{tag}-{next(_group)}"
    for r, e in enumerate(engines):
        e.comm_join_local(name, len(engines), r)


def run_ranks(engines, cores, cols, rows):
    """eng.stitch_exchange on every rank, each from its own thread: [(nb, nc) | TrgError] per rank, wall seconds"""
    from trg_planner._engine import TrgError
    out = [None] * len(engines)

    def rank(r):
        try:
            out[r] = engines[r].stitch_exchange(cores[r], cols, rows)
        except TrgError as ex:
            out[r] = ex

    threads = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(len(engines))]
    t0 = time.monotonic()
    for th in threads:
        th.start()
    for th in threads:
        th.join(max(0.0, JOIN_SECONDS - (time.monotonic() - t0)))
    alive = [r for r, th in enumerate(threads) if th.is_alive()]
    assert not alive, f"ranks {alive} did not return within {JOIN_SECONDS} s"
    return out, time.monotonic() - t0


def assert_same_rows(g, ref):
    assert g.V == ref.V and g.E == ref.E
    for k in ("rowptr", "col", "state", "cid"):
        assert np.array_equal(getattr(g, k), getattr(ref, k)), k
    for k in ("w", "dist", "xyz"):
        assert np.array_equal(getattr(g, k).view(np.uint32), getattr(ref, k).view(np.uint32)), k


def emulated(tiled, lay, engines):
    parts, cross = tiled.stitch_emulated(engines, lay.cores, lay.cols, lay.rows)
    nb = sum(e.stitch_boundary(lay.cores[t], lay.cols, lay.rows, t) for t, e in enumerate(engines))
    return parts, nb, int(cross.shape[0])


@pytest.mark.parametrize("name", ["2x1", "3x1", "2x2", "3x3", "empty_mid", "island_mid"])
def test_exchange_equals_emulated_stitch(oa, synth, tiled, name):
    """Every rank's rows and counts, twice: the second call runs on the buffers the first one left."""
    lay, engines = sc.engines(oa, synth, tiled, name)
    want, nb, nc = emulated(tiled, lay, engines)
    for e in engines:  # (so that nothing of the emulated run is what the exchange is then seen to give)
        e.stitch_assemble(0, 1, np.array([0, e.graph_sizes("global")[0]], np.int32), None, 0)
    join_group(engines, name)
    for call in range(2):
        got, secs = run_ranks(engines, lay.cores, lay.cols, lay.rows)
        print(name, "call", call, "ranks", len(engines), "(n_boundary, n_cross)", got[0], f"{secs * 1e3:.1f} ms")
        assert got == [(nb, nc)] * len(engines), got
        for t, e in enumerate(engines):
            assert_same_rows(e.graph("stitched"), want[t])
    if name in ("empty_mid", "island_mid"):
        assert nc == 0 and want[1].E == engines[1].graph_sizes("global")[1]
    else:
        assert nc > 10
    for e in engines:
        e.comm_destroy()


def test_exchange_regrows_its_buffers(oa, synth, tiled):
    """debug_stitch_cap = 4: the record and the edge buffer start at 4 rows and grow inside the exchange."""
    import trg_planner
    lay, shared = sc.engines(oa, synth, tiled, "2x2")
    want, nb, nc = emulated(tiled, lay, shared)
    # fresh engines: the buffers of an engine that has exchanged before are large already
    engines = []
    for t, (core, win) in enumerate(zip(lay.cores, lay.windows)):
        e = trg_planner.Engine(**oa.MOUNTAIN)
        e.set_sampler(sc.SAMPLER_SEED, 16)
        e.set_tile(core, epoch=t)
        e.set_global_map(synth.mountain_tile(*win, seed=sc.SEED, **sc.TERRAIN))
        e.init_graph([0.5 * (core[0] + core[2]), 0.5 * (core[1] + core[3]), 0.0])
        e.set_option("debug_stitch_cap", 4)
        engines.append(e)
    join_group(engines, "regrow")
    got, _ = run_ranks(engines, lay.cores, lay.cols, lay.rows)
    regrows = [e.stats()["stitch_regrows"] for e in engines]
    print("2x2 regrow rounds per rank", regrows, "(n_boundary, n_cross)", got[0])
    assert got == [(nb, nc)] * 4, got
    assert all(r >= 1 for r in regrows) and max(regrows) >= 2  # (records on every rank; edges where a tile owns > 4)
    for t, e in enumerate(engines):
        assert_same_rows(e.graph("stitched"), want[t])
    for e in engines:
        e.close()


def test_failure_after_the_first_exchange_is_announced(oa, synth, tiled, tmp_path):
    """Rank 0 holds its tile graph from JSON and no map: its stitch_cross fails (TRG_ERR_NO_MAP) after exchange 1, the
    count exchange of exchange 2 carries that, and rank 1 returns instead of waiting."""
    import trg_planner
    from trg_planner._engine import TrgError
    lay, shared = sc.engines(oa, synth, tiled, "2x1")
    shared[0].save_json(tmp_path / "tile0.json")
    e0 = trg_planner.Engine(**oa.MOUNTAIN)
    e0.load_json(tmp_path / "tile0.json")
    assert e0.stitch_boundary(lay.cores[0], 2, 1, 0) > 0
    engines = [e0, shared[1]]
    join_group(engines, "failure")
    got, secs = run_ranks(engines, lay.cores, 2, 1)
    assert isinstance(got[0], TrgError) and got[0].status == NO_MAP, got[0]
    assert str(got[0]).endswith("stitch_cross: no map"), str(got[0])
    assert isinstance(got[1], TrgError) and got[1].status == DEVICE, got[1]
    assert "another rank reported a failure" in str(got[1])
    assert secs < 10.0, secs  # (the wait limit is 20 s: nobody ran into it)
    shared[1].comm_destroy()
    e0.close()


def test_grid_that_does_not_match_the_group_is_refused(oa, synth, tiled):
    from trg_planner._engine import TrgError
    lay, engines = sc.engines(oa, synth, tiled, "2x1")
    join_group(engines, "refusal")
    got, secs = run_ranks(engines, lay.cores, 3, 1)
    for g in got:
        assert isinstance(g, TrgError) and g.status == INVALID_ARG, g
        assert "cols x rows must equal the communicator's size" in str(g)
    # no collective was entered: the group is whole, and the exchange still runs
    got, _ = run_ranks(engines, lay.cores, 2, 1)
    assert got[0] == got[1] and got[0][1] > 10, got
    for e in engines:
        e.comm_destroy()


def test_join_refusals(oa):
    import trg_planner
    from trg_planner._engine import TrgError
    a, b = trg_planner.Engine(**oa.MOUNTAIN), trg_planner.Engine(**oa.MOUNTAIN)
    name = f"test-exchange-join-{next(_group)}"
    a.comm_join_local(name, 2, 0)
    for nranks, rank, text in ((2, 0, "is taken"), (3, 1, "has 2 ranks"), (2, 2, "bad arguments"), (0, 0, "bad arguments"),
                               (65, 0, "bad arguments")):
        with pytest.raises(TrgError) as ex:
            b.comm_join_local(name, nranks, rank)
        assert ex.value.status == INVALID_ARG and text in str(ex.value), str(ex.value)
    assert a.L.trg_engine_comm_join_local(a.h, None, 2, 0) == INVALID_ARG
    a.close()
    b.close()
