"""CPU: the protocol of the risk field across tiles (tests/tiled_ref.py: the publish / merge loop
under the extension (max(risk, r), hops + 1)) must equal, on the UNCUT graph, both the definition
(risk_ref.py_risk_field) and the compiled host Dijkstra (tests/cpp/risk_reference.cpp) in risk bits, hops and parents
-- the exactness claim of DESIGN.md section 7, "Risk fields across tiles", pinned before any GPU run.  Also the C and
Python surface of the feature."""
import inspect
import os
import re

import numpy as np
import pytest

import risk_graphs as rg
import risk_ref
import tiled_ref as tr
from tiled_support import cuts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return risk_ref.compile_reference(tmp_path_factory.mktemp("tiled_risk_ref"))


def check(ref, G, offsets, member_sets, at=""):
    """the protocol on G cut at `offsets` against the definition and the compiled reference, per set of members"""
    infos = []
    for members in member_sets:
        want = risk_ref.py_risk_field(G["V"], G["rowptr"], G["col"], G["w"], G["state"], members)
        st, *compiled = risk_ref.risk_field(ref, G["rowptr"], G["col"], G["w"], G["state"], members)
        assert st == 0, st
        risk, hops, parent, info = tr.tiled_risk_field(G, offsets, members)
        where = f"{at} offsets {np.asarray(offsets).tolist()} members {members}: "
        for other, name in ((want, "the definition"), (compiled, "the compiled reference")):
            assert np.array_equal(risk.view(np.uint32), other[0].view(np.uint32)), where + "risk bits, " + name
            assert np.array_equal(hops, other[1]), where + "hops, " + name
            assert np.array_equal(parent, other[2]), where + "parents, " + name
        infos.append(info)
    return infos


def plateau_graph(rng, V, seed, blocks=None):
    g = tr.symmetric_graph(rng, V, blocks)
    f = rg.reweighted((g["rowptr"], g["col"], g["w"], g["dist"], g["state"]), seed)
    return dict(g, w=f.w)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("R", [2, 3, 4])
def test_protocol_equals_the_uncut_references(ref, seed, R):
    rng = np.random.default_rng(1000 * R + seed)
    V = int(rng.integers(40, 161)) if seed else 40
    G = plateau_graph(rng, V, seed)
    offsets = cuts(rng, V, R, empty=seed % 3 == 1 and R > 2)
    valid = np.flatnonzero(G["state"] != tr.INVALID)
    invalid = int(np.flatnonzero(G["state"] == tr.INVALID)[0])
    sets = [[int(valid[0])], [int(valid[len(valid) // 2])], [invalid], [int(valid[1]), int(valid[-1]), invalid]]
    infos = check(ref, G, offsets, sets)
    assert sum(infos[0]["ghosts"]) > 0 and max(min(i["exchanges"]) for i in infos) >= 2, infos
    # five weight levels: plateaus -- many nodes share a risk word
    risk = tr.tiled_risk_field(G, offsets, sets[0])[0]
    assert len(np.unique(risk[np.isfinite(risk)])) <= len(rg.LEVELS) + 1


def test_a_range_without_nodes_and_a_range_without_cross_edges(ref):
    rng = np.random.default_rng(7)
    V = 120
    G = plateau_graph(rng, V, 7, blocks=[(50, 80)])
    offsets = np.array([0, 50, 50, 80, V], np.int64)  # rank 1 has no nodes, rank 2 no cross edges
    ranks = [tr.solve_graph(G, int(offsets[t]), int(offsets[t + 1])) for t in range(4)]
    assert ranks[1].V == 0 and ranks[2].G == 0 and ranks[0].G > 0 and ranks[3].G > 0
    valid = np.flatnonzero(G["state"] != tr.INVALID)
    block = valid[(valid >= 50) & (valid < 80)]
    inside = int(block[np.argmax(np.diff(G["rowptr"])[block])])
    check(ref, G, offsets, [[int(valid[0])], [inside], [int(valid[-1]), inside]])
    hops = tr.tiled_risk_field(G, offsets, [inside])[1]
    assert (hops[:50] == -1).all() and (hops[80:] == -1).all() and (hops[50:80] >= 0).sum() > 1


def test_solve_graph_is_the_cost_protocols_on_a_symmetric_graph():
    """solve_graph against the in-edge definition written out: ghosts are the remote nodes with an edge into one of
    the rank's nodes, their rows hold exactly those edges with their values, the border is the rank's nodes with an
    edge into another rank's node."""
    rng = np.random.default_rng(11)
    G = tr.symmetric_graph(rng, 60)
    edges = [(u, int(G["col"][k]), float(G["w"][k]), float(G["dist"][k]))
             for u in range(60) for k in range(G["rowptr"][u], G["rowptr"][u + 1])]
    for lo, hi in ((0, 25), (25, 25), (25, 60)):
        a = tr.solve_graph(G, lo, hi)
        mine = lambda x: lo <= x < hi  # noqa: E731
        ghosts = sorted({u for u, v, _, _ in edges if mine(v) and not mine(u)})
        border = sorted({u - lo for u, v, _, _ in edges if mine(u) and not mine(v)})
        assert a.V == hi - lo and a.G == len(ghosts) and a.ghosts.tolist() == ghosts and a.border.tolist() == border
        assert a.gid_of.tolist() == list(range(lo, hi)) + ghosts and len(a.rowptr) == a.V + a.G + 1
        for i, g in enumerate(a.gid_of.tolist()):
            row = sorted((int(a.col[k]), float(a.w[k]), float(a.dist[k])) for k in range(a.rowptr[i], a.rowptr[i + 1]))
            assert row == sorted((v - lo, w, d) for u, v, w, d in edges if u == g and mine(v)), (lo, hi, g)
            assert i < a.V or row, (lo, hi, g)  # (a ghost has an edge into the rank)


def test_rise_and_fall_alternating_between_two_ranges(ref):
    """Every edge of the chain is a cross edge: one exchange per node, in pass 2 as well, while the risk word has
    stopped moving at the peak."""
    G, offsets, new = tr.interleaved(rg.rise_and_fall(16))
    info, = check(ref, G, offsets, [[int(new[0])]])
    assert info["exchanges"][0] >= 16 and info["exchanges"][1] >= 16, info
    risk, hops, _, _ = tr.tiled_risk_field(G, offsets, [int(new[0])])
    assert hops[new[15]] == 15 and len(np.unique(risk[new[8:]])) == 1


def test_all_zero_weights_cut_in_three(ref):
    g = rg.all_zero_weights(24)
    G = tr.as_csr(g)
    infos = check(ref, G, np.array([0, 7, 15, 24], np.int64), [[0], [23], [3, 20]])
    risk = tr.tiled_risk_field(G, np.array([0, 7, 15, 24]), [0])[0]
    assert (risk.view(np.uint32) == 0).all() and sum(infos[0]["ghosts"]) > 0


@pytest.mark.parametrize("name", sorted(rg.cases()))
def test_hand_written_cases_cut_in_two_everywhere(ref, name):
    g, sources = rg.cases()[name]
    G = tr.as_csr(g)
    for cut in range(1, G["V"]):
        check(ref, G, np.array([0, cut, G["V"]], np.int64), [[s] for s in sources] + [sources], at=name)


def stale_hops_graph():
    """Tile A = {0 (the source), 1 = P, 2}, tile B = {3, 4, 5 (a chain at 0.5 to) 6 = Q, 7, 8, 9}.  Q is reached first
    over the long walk 0-3-4-5-6 at its final risk, (0.5, 4).  P's key is (0.3, 2) over 0-7-1 when it is first
    published, and P-Q at 0.5 then gives Q (0.5, 3): a shorter walk, arriving an exchange later.  Two exchanges after
    that P drops to (0.1, 4) over the zigzag 0-8-2-9-1, which does not move Q's word: max(0.1, 0.5) is still 0.5, at
    more hops.  The Dijkstra says hops[Q] = 4 (through 5, or through P at 5); one pass keeps 3."""
    e = [(0, 3, 0.5), (3, 4, 0.5), (4, 5, 0.5), (5, 6, 0.5), (0, 7, 0.3), (7, 1, 0.3), (1, 6, 0.5), (0, 8, 0.1),
         (8, 2, 0.1), (2, 9, 0.1), (9, 1, 0.1)]
    src = [a for a, b, _ in e] + [b for a, b, _ in e]
    dst = [b for a, b, _ in e] + [a for a, b, _ in e]
    w = np.array([c for _, _, c in e] * 2, np.float32)
    order = np.lexsort((np.array(dst), np.array(src)))
    V = 10
    return dict(V=V, rowptr=np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))]).astype(np.int64),
                col=np.array(dst, np.int64)[order], w=w[order], state=np.zeros(V, np.int64))


def test_the_second_pass_is_needed_across_a_seam(ref):
    G = stale_hops_graph()
    offsets = np.array([0, 3, 10], np.int64)
    want = risk_ref.py_risk_field(G["V"], G["rowptr"], G["col"], G["w"], G["state"], [0])
    one = tr.tiled_risk_field(G, offsets, [0], passes=1)
    assert np.array_equal(one[0].view(np.uint32), want[0].view(np.uint32))  # pass 1's risk words are final
    assert want[1][6] == 4 and one[1][6] == 3, (want[1], one[1])  # the precondition: pass 1 alone keeps stale hops
    check(ref, G, offsets, [[0]])


def test_staircase_publishes_every_drop(ref):
    sizes, edges, s, t = tr.staircase(8)
    V = sum(sizes)
    src = [a for a, b, _, _ in edges] + [b for a, b, _, _ in edges]
    dst = [b for a, b, _, _ in edges] + [a for a, b, _, _ in edges]
    w = np.array([c for _, _, c, _ in edges] * 2, np.float32)
    order = np.lexsort((np.array(dst), np.array(src)))
    G = dict(V=V, rowptr=np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))]).astype(np.int64),
             col=np.array(dst, np.int64)[order], w=w[order], state=np.zeros(V, np.int64))
    offsets = np.array([0, sizes[0], V], np.int64)
    info, = check(ref, G, offsets, [[s]])
    assert info["published"][t] >= 8, info["published"][t]
    risk, hops, _, _ = tr.tiled_risk_field(G, offsets, [s])
    assert risk[t] == np.float32(0.9 - 0.1 * 7) and hops[t] == 16


def test_surface():
    """Fails without the feature: the entries, their declarations and the Python methods."""
    import trg_planner
    from trg_planner import _engine, tiled
    trg_planner.build_library()
    lib = trg_planner.load_library()
    header = open(os.path.join(ROOT, "include", "trg_engine.h")).read()
    for sym in ("trg_engine_tiled_risk_field", "trg_engine_tiled_risk_field_sets"):
        assert sym in _engine.EXPORTS, sym
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert hasattr(lib, sym), sym
    E = _engine.Engine
    assert list(inspect.signature(E.tiled_risk_fields).parameters)[1:] == ["source_gids", "parent"]
    assert list(inspect.signature(E.tiled_risk_fields_from).parameters)[1:] == ["sets", "targets", "full", "parent"]
    assert list(inspect.signature(E.tiled_safest_routes).parameters)[1:] == ["start_gid", "goal_gids"]
    assert list(inspect.signature(E.tiled_frontier_ceilings).parameters)[1:] == ["member_gids"]
    assert list(inspect.signature(tiled.safest_frontier).parameters) == ["parts"]
    assert "risk fields and refresh are not offered" not in re.sub(r"\s*\n \*\s*", " ", header)


def test_safety_factor_is_an_option():
    """The one way to move the safety factor of a live engine (the tiled risk solves must not notice it): accepted
    through the C ABI, as tests/test_options.py pins the other keys."""
    import ctypes as C
    import trg_planner
    from trg_planner._engine import TrgParams
    trg_planner.build_library()
    L = trg_planner.load_library()
    prm = TrgParams(0, 0.6, 0.3, 8, 0.3, 0.2, 0.5, 1.0, 0.5)
    h = C.c_void_p()
    L.trg_engine_create(C.byref(prm), 0, C.byref(h))
    assert h.value
    for v in (b"0.5", b"3", b"0"):
        assert L.trg_engine_set_option(h, b"safety_factor", v) == 0, v  # TRG_OK
    L.trg_engine_destroy(h)


def test_python_joins():
    from trg_planner import tiled
    a = dict(risk=np.zeros((1, 2), np.float32), hops=np.zeros((1, 2), np.int32), parent=None)
    b = dict(risk=np.ones((1, 3), np.float32), hops=np.ones((1, 3), np.int32), parent=None)
    f = tiled.concat_fields([a, b])
    assert f["risk"].shape == (1, 5) and f["parent"] is None and "cost" not in f
    inf = np.float32(np.inf)
    parts = [dict(gids=[3, 5], risk=[0.5, 0.25], hops=[2, 9], owner=[0, 0], members=2),
             dict(gids=[11, 12, 13], risk=[0.25, 0.25, inf], hops=[9, 4, -1], owner=[0, 1, 1], members=2)]
    assert tiled.safest_frontier(parts) == [(5, 0.25, 9), (12, 0.25, 4)]
    parts[1]["owner"] = [0, -1, -1]
    assert tiled.safest_frontier(parts) == [(5, 0.25, 9), None]
