"""GPU: routes of a risk solve across tiles (trg_engine_tiled_field_routes after trg_engine_tiled_risk_field / _sets;
DESIGN.md section 7, "Risk fields across tiles") over the in-process transport.  The joined routes must equal the host
definition (risk_ref.route's walk: route_ref.route under the fold max(risk, r), on the concatenation of the rows the
engines export, with the fields of the compiled host Dijkstra) bit for bit: ids, num_nodes, cost (= risk[target]),
path_length, avg_risk, root_gid and owner; and tiled_safest_routes on a built tiling."""
import numpy as np
import pytest

import field_graphs as fg
import risk_graphs as rg
import risk_ref
import route_ref
import stitch_cases as sc
import tiled_route_ref as trr
from field_keys import fold_max, relaxable, risk_values
from tiled_support import (SF, assert_routes, call_routes, close, crossing_counts, exported, join_group, level_lattice,
                           ok, pick_sources, run_ranks, stitch)
from tiled_support import risk_craft as craft, risk_reference as reference
from tiled_support import risk_solve as solve, risk_solve_sets as solve_sets
from tiled_support import risk_reference_lib, tiled  # noqa: F401  (fixtures; risk_reference_lib is `ref`)
from tiled_support import want_routes as cost_routes

pytestmark = pytest.mark.gpu
F32 = np.float32


def want_routes(G, fields, pairs):
    """the reference routes; fields: per field (risk, hops, parent) of the uncut graph; pairs: (field, target)"""
    costs = (risk_values(G["w"]), relaxable(G["col"], G["state"]))
    memos = [{} for _ in fields]
    return [route_ref.route(G["rowptr"], G["col"], G["w"], G["dist"], G["state"], None, *fields[k], None, int(t),
                            costs=costs, memo=memos[k], fold=fold_max) for k, t in pairs]


def split(want):
    return [(want[0][k], want[1][k], want[2][k]) for k in range(want[0].shape[0])]


def test_lattice_routes_to_every_node(tmp_path, tiled, ref):
    """Targets in every tile, the sources among them; routes that cross seams three times and more; a solve asked for
    no parents, so that the routes call runs the RISK parent sweep itself; clipping by cap."""
    sizes, edges, sources = level_lattice()
    edges = [(a, b, w, 0.5 + 0.01 * ((a + 2 * b) % 7)) for a, b, w, _ in edges]
    engines = craft(tmp_path, sizes, edges, tag="routes-lattice")
    G = exported(tiled, engines)
    fields = split(reference(ref, G, [[s] for s in sources]))
    pairs = [(k, v) for k in range(3) for v in range(G["V"])]
    want = want_routes(G, fields, pairs)
    assert max(trr.crossings(G["offsets"], w) for w in want) >= 3
    assert all(w.cost == fields[k][0][v] for (k, v), w in zip(pairs, want))
    f, t = [p[0] for p in pairs], [p[1] for p in pairs]
    solve(engines, sources)
    a = assert_routes("risk lattice", tiled, call_routes(engines, f, t), G, want)
    solve(engines, sources, parent=False)
    b = assert_routes("risk lattice, late parent sweep", tiled, call_routes(engines, f, t), G, want)
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(a, b))
    few = [(0, sources[1]), (1, sources[0]), (2, 7), (0, sources[0])]
    want = want_routes(G, fields, few)
    total = sum(len(w.ids) for w in want)
    for cap in (len(want[0].ids) + 2, total - 1, 1, 0):
        parts = call_routes(engines, [p[0] for p in few], [p[1] for p in few], cap=cap)
        joined = assert_routes(f"risk cap {cap}", tiled, parts, G, want, cap=cap)
        assert [j[2].num_nodes for j in joined] == [len(w.ids) for w in want]
    close(engines)


def test_unreached_target_and_set_owners(tmp_path, tiled, ref):
    """A node behind an Invalid node is unreached: the empty route.  After a set solve the routes carry owners."""
    state = np.zeros(10, np.int32)
    state[7] = fg.INVALID
    edges = [(0, 1, 0.3, 1.0), (1, 5, 0.1, 2.0), (5, 6, 0.4, 1.0), (6, 2, 0.2, 3.0), (2, 3, 0.2, 1.0), (3, 7, 0.1, 1.0),
             (7, 8, 0.1, 1.0), (3, 9, 0.5, 1.0), (9, 4, 0.0, 1.0), (0, 4, 0.6, 1.0)]
    engines = craft(tmp_path, [5, 5], edges, state=state, tag="routes-sets")
    G = exported(tiled, engines)
    fields = split(reference(ref, G, [[0]]))
    pairs = [(0, v) for v in range(10)]
    want = want_routes(G, fields, pairs)
    assert len(want[8].ids) == 0 and len(want[7].ids) == 0 and np.isposinf(want[8].cost)
    assert trr.crossings(G["offsets"], want[4]) >= 3  # 0 1 | 5 6 | 2 3 | 9 | 4 under the ceiling 0.5, not 0 - 4 at 0.6
    solve(engines, [0])
    assert_routes("risk unreached", tiled, call_routes(engines, [0] * 10, list(range(10))), G, want)
    sets = [[8, 0, 4], [7, 6]]
    got = solve_sets(engines, sets)
    w = reference(ref, G, sets)
    fields = split(w)
    pairs = [(k, v) for k in range(2) for v in range(10)]
    want = want_routes(G, fields, pairs)
    joined = assert_routes("risk sets", tiled, call_routes(engines, [p[0] for p in pairs], [p[1] for p in pairs]), G,
                           want, owners=True)
    owners = [risk_ref.owners(np.asarray(s), w[1][k], w[2][k])[0] for k, s in enumerate(sets)]
    for (k, v), (ids, _, info) in zip(pairs, joined):
        assert info.owner == owners[k][v], (k, v)
        if info.num_nodes:
            assert info.root_gid == sets[k][info.owner] == ids[0], (k, v)
    assert any(i.root_gid == 7 and i.num_nodes > 1 for _, _, i in joined)  # from the Invalid member
    close(engines)


def duplicates_across_a_seam():
    """risk_graphs.cases()["duplicates"], both ways and with the seam between 1 and 2 moved onto a node of its own: tile 0
    holds 0, 1 with the duplicates 0 - 1 at (0.5, dist 1) and (0.2, dist 2); the cross edge 1 - 2 at 0.4; tile 1 holds
    2, 3 with the duplicates 2 - 3 at (0.1, dist 7) and (0.3, dist 11).  From 0: the cost walk takes 0 - 1 at 0.5 (cost
    2.5 against 3.2), the risk walk 0 - 1 at 0.2, the only tight one under max; below the plateau of 0.4 both duplicates
    of 2 - 3 are tight under max and the first in the row decides."""
    edges = [(0, 1, 0.5, 1.0), (1, 2, 0.4, 3.0), (2, 3, 0.1, 7.0)]
    extra = [(0, 1, 0.2, 2.0), (2, 3, 0.3, 11.0)]
    return [2, 2], edges, extra


def test_cost_tight_and_risk_tight_edges_differ(tmp_path, tiled, ref):
    import field_ref
    sizes, edges, extra = duplicates_across_a_seam()
    engines = craft(tmp_path, sizes, edges, tag="routes-dup", extra=extra)
    G = exported(tiled, engines)
    fields = split(reference(ref, G, [[0]]))
    pairs = [(0, 3), (0, 1), (0, 2), (0, 0)]
    want = want_routes(G, fields, pairs)
    r = want[0]
    assert r.ids.tolist() == [0, 1, 2, 3] and G["w"][r.edges[0]] == F32(0.2) and G["dist"][r.edges[0]] == F32(2.0)
    assert G["w"][r.edges[2]] == F32(0.1) and r.cost == F32(0.4)
    # the walk under `+` over these keys finds no tight edge into 1, and over the cost solve's keys another edge
    lib = field_ref.compile_reference(tmp_path)
    st, c, h, p = field_ref.field(lib, G["rowptr"], G["col"], G["w"], G["dist"], G["state"], SF, 0)
    cost_r = cost_routes(G, [(c, h, p)], [(0, 3)])[0]
    assert cost_r.ids.tolist() == r.ids.tolist() and cost_r.edges[0] != r.edges[0]
    assert cost_r.path_length != r.path_length and cost_r.avg_risk != r.avg_risk
    solve(engines, [0])
    assert_routes("risk duplicates", tiled, call_routes(engines, [0] * 4, [t for _, t in pairs]), G, want)
    ok(run_ranks(engines, lambda r, e: e.tiled_cost_fields([0]))[0])  # the routes answer from the solve that ran last
    assert_routes("cost duplicates", tiled, call_routes(engines, [0], [3]), G, [cost_r])
    solve(engines, [0], parent=False)
    assert_routes("risk duplicates again", tiled, call_routes(engines, [0] * 4, [t for _, t in pairs]), G, want)
    close(engines)


def test_rise_and_fall_route_crosses_at_every_step(tmp_path, tiled, ref):
    g = rg.rise_and_fall(64)
    gid = lambda p: (p % 2) * 32 + p // 2  # noqa: E731
    edges = [(gid(p), gid(p + 1), float(g.w[p]), 1.0 + 0.125 * (p % 5)) for p in range(63)]
    engines = craft(tmp_path, [32, 32], edges, tag="routes-rise")
    G = exported(tiled, engines)
    fields = split(reference(ref, G, [[gid(0)]]))
    pairs = [(0, gid(63)), (0, gid(0)), (0, gid(17))]
    want = want_routes(G, fields, pairs)
    assert trr.crossings(G["offsets"], want[0]) == 63
    solve(engines, [gid(0)], parent=False)
    parts = call_routes(engines, [0, 0, 0], [t for _, t in pairs])
    assert_routes("risk rise", tiled, parts, G, want)
    assert [p["info"].exchanges for p in parts] == [66, 66]
    close(engines)


def test_tiled_safest_routes_on_a_built_tiling(oa, synth, tiled, ref):
    lay, engines = sc.engines(oa, synth, tiled, "2x2")
    join_group(engines, "risk-safest")
    stitch(engines, lay)
    G = exported(tiled, engines)
    sources, _ = pick_sources(G)
    start = sources[0]
    fields = split(reference(ref, G, [[start]]))
    n_cross = crossing_counts(G, fields[0][1], fields[0][2])
    rng = np.random.default_rng(3)
    goals = rng.integers(0, G["V"], 10).tolist() + [start, int(np.argmax(n_cross))]
    want = want_routes(G, fields, [(0, g) for g in goals])
    assert sum(trr.crossings(G["offsets"], w) > 0 for w in want) >= 2
    parts = ok(run_ranks(engines, lambda r, e: e.tiled_safest_routes(start, goals))[0])
    joined = assert_routes("safest_routes", tiled, parts, G, want)
    for g, (ids, pts, info) in zip(goals, joined):
        assert np.array_equal(pts, G["xyz"][ids]) and np.float32(info.cost).view(np.uint32) == fields[0][0][g:g + 1].view(np.uint32)[0]
    for e in engines:
        e.comm_destroy()
