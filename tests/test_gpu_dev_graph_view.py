"""GPU: the one device view of the global graph (ensure_dev_graph; DESIGN.md, "Host graph state and its views") under
its two consumers, the cost field and the tile stitch, in the orders that share it: a stitch between a solve and its
routes, a stitch before the first solve, a larger graph after a smaller one (the upload grows, the retained solve is
refused), and both after an update_graph has dropped the device build's CSR.  Everything is compared exactly: field
arrays as bits, routes by ids and info bits, stitched rows with the global rows.

The graphs are loaded through load_json (field_support.load_graph): a host graph, no device CSR, tens of nodes; the
larger one a few hundred."""
import numpy as np
import pytest

import field_graphs as fg
import stitch_cases as sc
from field_support import INVALID_ARG, MOUNTAIN, bits, load_graph, random_large, small_sources, with_isolated_node
from graph_support import obs_crop

pytestmark = pytest.mark.gpu
CORE = np.array([-1e3, -1e3, 1e3, 1e3], np.float32)


def _small():
    return with_isolated_node(fg.with_positions(fg.random_small(7)))


def _solve(e, sources):
    return e.cost_fields(source_ids=[int(s) for s in sources], full=True)


def _same_fields(a, b, at):
    assert np.array_equal(bits(a["cost"]), bits(b["cost"])), at + "cost"
    assert np.array_equal(a["hops"], b["hops"]), at + "hops"
    assert np.array_equal(a["parent"], b["parent"]), at + "parent"
    assert np.array_equal(a["reached"], b["reached"]), at + "reached"


def _routes(e, pairs):
    got = e.routes([k for k, _ in pairs], [t for _, t in pairs])
    return [(ids.tolist(), bits(pts).tolist(), one.num_nodes, bits(one.cost)[0], bits(one.path_length)[0],
             bits(one.avg_risk)[0]) for ids, pts, one in got]


def _reached(e, field):
    ids, cost, hops = e.field_reached(field)
    return ids.tolist(), bits(cost).tolist(), hops.tolist()


def _stitch_alone(e, x):
    """The 1 x 1 stitch of the engine's graph x: no boundary, and the stitched rows are the global rows."""
    assert e.stitch_boundary(CORE, 1, 1, 0) == 0
    e.stitch_assemble(0, 1, [0, x.V], None, 0)
    _stitched_is_global(e, x)


def _stitched_is_global(e, x):
    s = e.graph("stitched")
    assert s.V == x.V and s.E == x.E
    assert np.array_equal(s.rowptr, x.rowptr) and np.array_equal(s.col, x.col)
    assert np.array_equal(bits(s.w), bits(x.w)) and np.array_equal(bits(s.dist), bits(x.dist))
    assert np.array_equal(s.cid, np.arange(x.V))
    assert np.array_equal(s.state, x.state) and np.array_equal(bits(s.xyz), bits(x.xyz))


def _fresh():
    import trg_planner
    e = trg_planner.Engine(**MOUNTAIN)
    e.set_option("field_delta_scale", "4")
    return e


def test_stitch_between_a_solve_and_its_routes(tmp_path):
    g = _small()
    e = _fresh()
    x = load_graph(e, g, tmp_path)
    sources = small_sources(g, 2, 7)
    first = _solve(e, sources)
    pairs = [(k, t) for k in range(2) for t in (0, x.V // 2, x.V - 1, int(sources[k]))]
    routes, reached = _routes(e, pairs), [_reached(e, k) for k in range(2)]
    assert any(r[2] >= 2 for r in routes)
    _stitch_alone(e, x)
    assert _routes(e, pairs) == routes
    assert [_reached(e, k) for k in range(2)] == reached
    _same_fields(_solve(e, sources), first, "the second solve: ")
    assert _routes(e, pairs) == routes
    e.close()


def test_stitch_first(tmp_path):
    g = _small()
    sources = small_sources(g, 2, 7)
    plain = _fresh()
    load_graph(plain, g, tmp_path, "plain")
    want = _solve(plain, sources)
    plain.close()
    e = _fresh()
    x = load_graph(e, g, tmp_path)
    e.stitch_assemble(0, 1, [0, x.V], None, 0)
    _same_fields(_solve(e, sources), want, "after the stitch: ")
    _stitched_is_global(e, x)
    # ... and as stitch_cases.assemble_expected states it: the tile's rows of the assembled graph, cid the ids
    none = np.zeros((0, 6), np.int32)
    e.stitch_assemble(sc.TILE, sc.NTILES, sc.assemble_offsets(x.V), None, 0)
    import trg_planner.tiled as tiled
    gx = sc.SimpleNamespace(V=x.V, xyz=x.xyz, state=x.state, rowptr=x.rowptr.astype(np.int64),
                            col=x.col.astype(np.int64), w=x.w, dist=x.dist)
    exp = sc.assemble_expected(tiled, gx, none)
    s = e.graph("stitched")
    assert np.array_equal(s.rowptr, exp["rowptr"]) and np.array_equal(s.cid, exp["cid"])
    off = int(sc.assemble_offsets(x.V)[sc.TILE])
    assert np.array_equal(s.col.astype(np.int64), exp["col"]) and np.array_equal(s.col, x.col + off)
    assert np.array_equal(bits(s.w), bits(exp["w"])) and np.array_equal(bits(s.dist), bits(exp["dist"]))
    e.close()


def test_a_larger_graph_after_a_smaller(tmp_path):
    a, b = _small(), random_large(5, 40, 10)  # 400 nodes
    assert len(b.state) >= 4 * len(a.state) and len(b.col) >= 4 * len(a.col)
    sources_b = [1, len(b.state) // 2 + 5]  # one in each component
    plain = _fresh()
    load_graph(plain, b, tmp_path, "plain")
    want = _solve(plain, sources_b)
    plain.close()
    e = _fresh()
    load_graph(e, a, tmp_path, "a")
    _solve(e, small_sources(a, 2, 7))
    assert len(e.routes([0], [0])) == 1
    xb = load_graph(e, b, tmp_path, "b")
    _stitch_alone(e, xb)
    import trg_planner
    for call in (lambda: e.routes([0], [0]), lambda: e.field_reached(0)):
        with pytest.raises(trg_planner.TrgError) as ei:
            call()
        assert ei.value.status == INVALID_ARG and "earlier graph" in str(ei.value)
    _same_fields(_solve(e, sources_b), want, "graph B: ")
    _stitched_is_global(e, xb)
    e.close()


def test_after_the_device_csr_is_dropped(mountain_small, tmp_path):
    import trg_planner
    e = trg_planner.Engine(**MOUNTAIN)
    e.set_sampler(7, 16)
    e.set_global_map(mountain_small)
    e.init_graph([15.0, 15.0, 0.0])
    pose = (12.0, 12.0)
    e.set_local_map(pose, obs_crop(mountain_small, pose, 4.0, box=(pose[0] + 2.0, pose[1] + 1.0, 0.6)))
    e.update_graph()
    x = e.graph("global")
    e.stitch_assemble(0, 1, [0, x.V], None, 0)
    got = e.cost_fields(sources_xy=[(15.0, 15.0), (12.0, 12.0)], full=True)
    _stitched_is_global(e, x)
    path = tmp_path / "updated.json"
    e.save_json(str(path))
    other = _fresh()
    other.load_json(str(path))
    y = other.graph("global")
    assert y.V == x.V and np.array_equal(y.rowptr, x.rowptr) and np.array_equal(y.col, x.col)
    want = _solve(other, got["sources"])
    _same_fields(got, want, "after update_graph: ")
    # and in the other order on the loaded graph: the solve's upload serves the stitch
    other.stitch_assemble(0, 1, [0, y.V], None, 0)
    _stitched_is_global(other, y)
    e.close()
    other.close()
