"""GPU: what the C boundary's one frame (csrc/abi_frame.h, entry() in trg_engine.cpp) must leave as it was: every
refusal's status and text, plan_batch on its eight threads, the staged upload on its four."""
import json

import numpy as np
import pytest

from abi_refusals import GOLDEN, MOUNTAIN, refusal_table

pytestmark = pytest.mark.gpu


def test_refusals_are_what_they_were(mountain_small):
    """(status, last_error) of every refusal in tests/abi_refusals.py against the table recorded from the commit
    before the frame: null engine, null pointers, no map, no graph, unknown options, routes without a solve; entries
    of all five files that define some."""
    with open(GOLDEN) as f:
        want = json.load(f)
    got = refusal_table(mountain_small)
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff
    assert len(want) > 100 and {v[0] for v in want.values()} >= {0, 1, 2, 5, 7}


def test_plan_batch_of_nine_equals_single_plans(mountain_small, tmp_path):
    """9 queries are 8 threads, the caller's taking queries 0 and 8: paths and infos bit-equal to 9 plan calls.  The
    fixture's graph is one piece, so one node of it is cut off (saved, its edges dropped, loaded again) and is the
    goal of the query without a path."""
    import trg_planner
    e = trg_planner.Engine(**MOUNTAIN)
    e.set_sampler(7, 16)
    e.set_global_map(mountain_small)
    e.init_graph([15.0, 15.0, 0.0])
    g = e.graph("global")
    rng = np.random.default_rng(9)
    picks = rng.choice(g.V, 19, replace=False)
    cut = int(picks[18])
    e.save_json(tmp_path / "graph.json")
    with open(tmp_path / "graph.json") as f:
        doc = json.load(f)
    doc["edges"] = [ed for ed in doc["edges"] if cut not in (ed["source"], ed["target"])]
    with open(tmp_path / "cut.json", "w") as f:
        json.dump(doc, f)
    e.load_json(tmp_path / "cut.json")
    g = e.graph("global")
    assert g.rowptr[cut + 1] == g.rowptr[cut] and g.E > 1000
    starts = g.xyz[picks[:9], :2].copy()
    goals = g.xyz[picks[9:18]].copy()
    goals[4] = g.xyz[cut]
    single = [e.plan(s, t) for s, t in zip(starts, goals)]
    batch = e.plan_batch(starts, goals)
    assert len(batch) == 9
    for k, ((ps, is_), (pb, ib)) in enumerate(zip(single, batch)):
        assert (ps.shape[0] == 0) == (k == 4), (k, ps.shape)  # (without a path: direct_dist alone is filled)
        assert np.array_equal(ps.view(np.uint32), pb.view(np.uint32)), k
        assert is_.num_points == ib.num_points == ps.shape[0] == pb.shape[0], k
        for name in ("direct_dist", "path_length", "avg_risk"):
            a, b = np.float32(getattr(is_, name)), np.float32(getattr(ib, name))
            assert a.view(np.uint32) == b.view(np.uint32), (k, name, a, b)
    assert sum(p.shape[0] > 1 for p, _ in batch) >= 6  # real searches, not nine trivial ones


def test_staged_upload_places_every_chunk():
    """A pageable cloud of 6 000 000 points is 72 MB: nine 8 MiB chunks, the last one partial, three of them on one
    of the four copy threads, which uses a pinned slot a second time.  The map index built from it equals, bit for
    bit, the one built from the same cloud already on the device."""
    import torch
    import trg_planner
    n = 6_000_000
    rng = np.random.default_rng(20)
    cloud = np.empty((n, 3), np.float32)
    cloud[:, 0] = rng.uniform(0.0, 245.0, n)
    cloud[:, 1] = rng.uniform(0.0, 245.0, n)
    cloud[:, 2] = 0.5 * np.sin(cloud[:, 0] / 7.0) + 0.5 * np.cos(cloud[:, 1] / 5.0)
    assert cloud.nbytes == 72_000_000 and -(-cloud.nbytes // (8 << 20)) == 9
    staged = trg_planner.Engine(**MOUNTAIN)
    staged.set_global_map(cloud)
    direct = trg_planner.Engine(**MOUNTAIN)
    dev = torch.from_numpy(cloud).to("cuda:0")
    torch.cuda.synchronize()
    direct.set_global_map_device(dev.data_ptr(), n, 3)
    a, b = staged.map_index("global", n), direct.map_index("global", n)
    for va, vb in zip(a, b):  # x, y, z, perm, grid size, origin and cell
        assert va.dtype == vb.dtype and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
    assert np.array_equal(np.sort(a[3]), np.arange(n, dtype=np.int32))
    assert np.array_equal(a[0], cloud[a[3], 0]) and np.array_equal(a[2], cloud[a[3], 2])
