"""GPU: routes across tiles (trg_engine_tiled_field_routes; DESIGN.md section 7, "Routes across tiles") over the
in-process transport: one process, one engine and one thread per rank, all on one device.  The joined routes must equal
the host definition (tests/route_ref.py on the concatenation of the rows the engines export, with the fields of the
compiled host Dijkstra or of seed_ref) bit for bit: ids, num_nodes, cost, path_length and avg_risk; every rank's part
holds its own nodes and nothing else; all ranks return the same offsets and infos; the call takes c + 3 exchanges for
the route with the most seam crossings c.  Built tilings, crafted graphs, capacity, staleness and failures, refusals,
the single-engine solve left alone, and tiled_plan_many."""
import ctypes as C

import numpy as np
import pytest

import field_graphs as fg
import stitch_cases as sc
import tiled_route_ref as trr
from field_support import MOUNTAIN, bits
from tiled_support import (INVALID_1, RING, assert_routes, call_routes, close, craft, crossing_counts, exported,
                           host_fields, join_group, most_crossings, pick_sources, reference, run_ranks, solve,
                           solve_sets, stitch, tie_lattice, want_routes)
from tiled_support import ref, tiled  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
INVALID_ARG, DEVICE = 1, 4
F32 = np.float32


# ---- 1. built tilings -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2x1", "2x2", "3x3"])
def test_built_tilings(oa, synth, tiled, ref, name):
    lay, engines = sc.engines(oa, synth, tiled, name)
    join_group(engines, "routes-" + name)
    stitch(engines, lay)
    G = exported(tiled, engines)  # (the rows leave the device: the first solve reads the fetched rows)
    R, off = len(engines), G["offsets"]
    sources, _ = pick_sources(G)
    fields = reference(ref, G, sources)
    fields = [(fields[0][k], fields[1][k], fields[2][k]) for k in range(3)]
    rng = np.random.default_rng(5 + R)
    tile_of = np.searchsorted(off, np.arange(G["V"]), side="right") - 1
    rows = np.repeat(np.arange(G["V"]), np.diff(G["rowptr"]))
    border = np.unique(rows[tile_of[rows] != tile_of[G["col"]]])
    pairs = []
    for k, (cost, hops, parent) in enumerate(fields):
        n_cross = crossing_counts(G, hops, parent)
        home = np.flatnonzero((tile_of == tile_of[sources[k]]) & (hops > 0))
        far = np.flatnonzero((tile_of == R - 1) & (hops > 0))
        t = [sources[k], int(rng.choice(home))] + rng.choice(border, 3).tolist() + rng.choice(far, 4).tolist()
        t += [int(np.argmax(n_cross))] + np.flatnonzero(G["state"] == fg.INVALID)[:1].tolist()  # (where there is one:
        t += np.flatnonzero((hops < 0) & (G["state"] != fg.INVALID))[:1].tolist()  # init_graph alone leaves none)
        pairs += [(k, int(x)) for x in t]
    want = want_routes(G, fields, pairs)
    most = most_crossings(G, want)
    assert most >= (2 if R > 2 else 1), (name, most)  # the precondition, from the reference routes
    assert sum(trr.crossings(off, w) > 0 for w in want) >= 6
    f, t = [p[0] for p in pairs], [p[1] for p in pairs]
    solve(engines, sources)
    a = assert_routes(f"{name} fetched rows", tiled, call_routes(engines, f, t), G, want)
    stitch(engines, lay)  # (again: the rows are in HBM, where the next solve reads them; no parents asked for)
    solve(engines, sources, parent=False)
    b = assert_routes(f"{name} rows in HBM, late parent sweep", tiled, call_routes(engines, f, t), G, want)
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(a, b))
    for e in engines:
        e.comm_destroy()


# ---- 2. the chain that alternates between two tiles -------------------------------------------------------------------
def test_chain_alternating_between_two_tiles(tmp_path, tiled, ref):
    gid = lambda p: (p % 2) * 32 + p // 2  # noqa: E731
    dist = np.array(fg.CHAIN_DIST, F32)
    edges = [(gid(p), gid(p + 1), 0.1 * (p % 3), float(dist[p % len(dist)])) for p in range(63)]
    engines, _ = craft(tmp_path, [32, 32], edges, tag="chain")
    G = exported(tiled, engines)
    fields = reference(ref, G, [gid(0)])
    pairs = [(0, gid(63)), (0, gid(0)), (0, gid(17))]
    want = want_routes(G, [(fields[0][0], fields[1][0], fields[2][0])], pairs)
    assert trr.crossings(G["offsets"], want[0]) == 63
    solve(engines, [gid(0)])
    parts = call_routes(engines, [0, 0, 0], [t for _, t in pairs])
    joined = assert_routes("chain", tiled, parts, G, want)
    assert [p["info"].exchanges for p in parts] == [66, 66]
    one = joined[1][2]
    assert (one.num_nodes, one.cost, one.path_length, one.avg_risk, one.root_gid) == (1, 0.0, 0.0, 0.0, gid(0))
    close(engines)


# ---- 3. / 7. exact ties across seams; 300 routes in one call -----------------------------------------------------------
def test_tie_lattice_follows_the_least_global_id_across_seams(tmp_path, tiled, ref):
    sizes, edges, sources = tie_lattice()
    engines, _ = craft(tmp_path, sizes, edges, tag="lattice")
    G = exported(tiled, engines)
    V, off = G["V"], G["offsets"]
    fields = reference(ref, G, sources)
    fields = [(fields[0][k], fields[1][k], fields[2][k]) for k in range(3)]
    tile_of = np.searchsorted(off, np.arange(V), side="right") - 1
    cost, hops, parent = fields[0]
    seam_wins = 0  # a parent in another tile although a local tight predecessor exists: the least GLOBAL id decides
    for v in range(V):
        preds = [int(u) for u in G["col"][G["rowptr"][v]:G["rowptr"][v + 1]] if cost[u] + 1.0 == cost[v]]
        seam_wins += parent[v] >= 0 and tile_of[parent[v]] != tile_of[v] and any(tile_of[u] == tile_of[v] for u in preds)
    assert seam_wins > 3, seam_wins
    solve(engines, sources)
    pairs = [(k, v) for k in range(3) for v in range(V)]
    want = want_routes(G, fields, pairs)
    assert sum(trr.reenters(off, w) for w in want) > 10
    assert_routes("lattice, every node", tiled, call_routes(engines, [p[0] for p in pairs], [p[1] for p in pairs]), G, want)
    # 300 routes with repeated targets: groups over several workgroups, record slots across waves
    rng = np.random.default_rng(9)
    pairs = [(int(rng.integers(0, 3)), int(rng.integers(0, 40))) for _ in range(300)]
    assert len(set(pairs)) < 300
    want = want_routes(G, fields, pairs)
    assert_routes("lattice, 300 routes", tiled, call_routes(engines, [p[0] for p in pairs], [p[1] for p in pairs]), G, want)
    close(engines)


def test_tie_lattice_of_a_set_solve(tmp_path, tiled):
    sizes, edges, sources = tie_lattice()
    engines, _ = craft(tmp_path, sizes, edges, tag="lattice-sets")
    G = exported(tiled, engines)
    sets, starts = [sources, [sources[1], 5, 50]], [np.array([0.0, 1.0, 2.0], F32), np.array([0.0, 3.0, 0.5], F32)]
    fields = host_fields(G, sets, starts)
    solve_sets(engines, sets, starts)
    pairs = [(k, v) for k in range(2) for v in range(G["V"])]
    want = want_routes(G, [(f.cost, f.hops, f.parent) for f in fields], pairs)
    parts = call_routes(engines, [p[0] for p in pairs], [p[1] for p in pairs])
    joined = assert_routes("lattice sets", tiled, parts, G, want, owners=True)
    for (k, v), (_, _, info) in zip(pairs, joined):
        assert info.owner == fields[k].owner[v] and info.root_gid == sets[k][info.owner], (k, v)
    assert most_crossings(G, want) >= 2
    close(engines)


# ---- 4. out of a tile and back ----------------------------------------------------------------------------------------
REENTRY = [(0, 1, 0.0, 1.0), (1, 4, 0.1, 1.0), (4, 5, 0.0, 1.0), (5, 2, 0.2, 1.0), (2, 3, 0.3, 1.0), (1, 2, 0.0, 10.0),
           (5, 6, 0.0, 1.0)]  # in [4, 3]: the cheapest path 0 .. 3 runs 0 1 | 4 5 | 2 3


def reentry(tmp_path, tiled, ref, tag):
    engines, restitch = craft(tmp_path, [4, 3], REENTRY, tag=tag)
    G = exported(tiled, engines)
    fields = reference(ref, G, [0, 6])
    return engines, restitch, G, [(fields[0][k], fields[1][k], fields[2][k]) for k in range(2)]


def test_a_route_that_leaves_a_tile_and_returns(tmp_path, tiled, ref):
    engines, _, G, fields = reentry(tmp_path, tiled, ref, "reentry")
    solve(engines, [0, 6])
    pairs = [(0, 3), (1, 0), (0, 6)]
    want = want_routes(G, fields, pairs)
    assert want[0].ids.tolist() == [0, 1, 4, 5, 2, 3] and trr.crossings(G["offsets"], want[0]) == 2
    parts = call_routes(engines, [p[0] for p in pairs], [p[1] for p in pairs])
    assert_routes("reentry", tiled, parts, G, want)
    assert parts[0]["gids"][:6].tolist() == [0, 1, -1, -1, 2, 3]  # one rank, two stretches of one route
    assert parts[1]["gids"][:6].tolist() == [-1, -1, 4, 5, -1, -1]
    close(engines)


# ---- 5. set solves with start costs -------------------------------------------------------------------------------------
def test_set_solves_with_start_costs(tmp_path, tiled):
    state = np.zeros(8, np.int32)
    state[1] = fg.INVALID  # node 1: Invalid, a border node, and a member
    engines, _ = craft(tmp_path, [4, 4], INVALID_1, state=state, tag="seeded")
    G = exported(tiled, engines)
    sets, starts = [[0, 6, 1], [7, 1, 2, 2]], [np.array([0.5, 0.25, 0.0], F32), np.array([0.0, 0.125, 3.0, 0.75], F32)]
    fields = host_fields(G, sets, starts)
    got = solve_sets(engines, sets, starts)
    owner = np.concatenate([g["owner"] for g in got], 1)
    pairs = [(k, v) for k in range(2) for v in range(8)]
    want = want_routes(G, [(f.cost, f.hops, f.parent) for f in fields], pairs)
    joined = assert_routes("seeded", tiled, call_routes(engines, [p[0] for p in pairs], [p[1] for p in pairs]), G, want,
                           owners=True)
    started = 0
    for (k, v), w, (ids, _, info) in zip(pairs, want, joined):
        assert info.owner == owner[k][v] == fields[k].owner[v], (k, v)
        if info.num_nodes:
            c0 = starts[k][info.owner]
            assert info.root_gid == sets[k][info.owner] == ids[0], (k, v)
            assert bits(info.cost)[0] == bits(fields[k].cost[v])[0] and info.cost >= c0  # the start cost is in the cost
            assert bits(info.path_length)[0] == bits(w.path_length)[0]                  # ... and not in the length
            started += c0 > 0 and info.num_nodes > 1
    assert started >= 3 and any(i.root_gid == 1 and i.num_nodes > 1 for _, _, i in joined)  # from the Invalid member
    close(engines)


# ---- 6. other shapes ----------------------------------------------------------------------------------------------------
def test_saturated_route(tmp_path, tiled, ref):
    big = 3.0e38
    edges = [(0, 1, 0.0, big), (1, 4, 0.0, big), (4, 5, 0.0, 1.0), (5, 8, 0.0, big), (8, 9, 0.0, 1.0),
             (0, 2, 0.0, 0.5), (2, 6, 0.7, 0.0), (6, 3, 0.0, 0.0), (3, 7, 0.2, 0.0)]
    engines, _ = craft(tmp_path, [4, 6], edges, tag="sat")
    G = exported(tiled, engines)
    fields = reference(ref, G, [0, 9])
    fields = [(fields[0][k], fields[1][k], fields[2][k]) for k in range(2)]
    solve(engines, [0, 9])
    pairs = [(k, v) for k in range(2) for v in range(10)]
    want = want_routes(G, fields, pairs)
    assert any(np.isposinf(w.cost) and len(w.ids) > 2 and np.isposinf(w.path_length) for w in want)
    assert_routes("sat", tiled, call_routes(engines, [p[0] for p in pairs], [p[1] for p in pairs]), G, want)
    close(engines)


def test_duplicate_edges_inside_a_tile(tmp_path, tiled, ref):
    """0 - 1 three times alike: the first counts.  1 - 2 with weights 0.9, 0.1, 0.4: only the middle one is tight.
    Behind them the seam."""
    edges = [(0, 1, 0.5, 1.0), (1, 2, 0.9, 1.0), (2, 4, 0.0, 1.0), (4, 5, 0.2, 1.0), (5, 3, 0.0, 1.0)]
    extra = [(0, 1, 0.5, 1.0), (0, 1, 0.5, 1.0), (1, 2, 0.1, 1.0), (1, 2, 0.4, 1.0)]
    engines, _ = craft(tmp_path, [4, 2], edges, tag="dup", extra=extra)
    G = exported(tiled, engines)
    assert int(np.diff(G["rowptr"])[1]) == 6
    fields = reference(ref, G, [0, 5])
    fields = [(fields[0][k], fields[1][k], fields[2][k]) for k in range(2)]
    solve(engines, [0, 5])
    pairs = [(k, v) for k in range(2) for v in range(6)]
    want = want_routes(G, fields, pairs)
    r = want[3]  # field 0 to node 3: 0 1 2 | 4 5 | 3
    assert r.ids.tolist() == [0, 1, 2, 4, 5, 3] and G["w"][r.edges[0]] == F32(0.5) and G["w"][r.edges[1]] == F32(0.1)
    assert r.edges[0] == G["rowptr"][0] and bits(r.avg_risk)[0] != bits(F32(F32(0.5 + 0.9 + 0.2) / F32(6)))[0]
    assert_routes("dup", tiled, call_routes(engines, [p[0] for p in pairs], [p[1] for p in pairs]), G, want)
    close(engines)


def test_a_tile_without_nodes_between_two_with_cross_edges(tmp_path, tiled, ref):
    engines, _ = craft(tmp_path, [6, 0, 6], RING, tag="hollow")
    G = exported(tiled, engines)
    S = [0, 8, 5]
    fields = reference(ref, G, S)
    fields = [(fields[0][k], fields[1][k], fields[2][k]) for k in range(3)]
    solve(engines, S)
    pairs = [(k, v) for k in range(3) for v in range(12)]
    want = want_routes(G, fields, pairs)
    parts = call_routes(engines, [p[0] for p in pairs], [p[1] for p in pairs])
    assert_routes("hollow", tiled, parts, G, want)
    assert (parts[1]["gids"] == -1).all() and np.isnan(parts[1]["xyz"]).all() and most_crossings(G, want) >= 1
    close(engines)


# ---- 8. capacity --------------------------------------------------------------------------------------------------------
def test_capacity(tmp_path, tiled, ref):
    engines, _, G, fields = reentry(tmp_path, tiled, ref, "cap")
    solve(engines, [0, 6])
    pairs = [(0, 3), (1, 0), (0, 6), (1, 3)]
    f, t = [p[0] for p in pairs], [p[1] for p in pairs]
    want = want_routes(G, fields, pairs)
    total = sum(len(w.ids) for w in want)
    exchanges0 = None
    for cap in (8, total - 1, 1):  # (8: the second route keeps its first two nodes, the source end; the rest are empty)
        parts = call_routes(engines, f, t, cap=cap)
        joined = assert_routes(f"cap {cap}", tiled, parts, G, want, cap=cap)
        assert int(parts[0]["offsets"][-1]) == cap and [j[2].num_nodes for j in joined] == [len(w.ids) for w in want]
        exchanges0 = parts[0]["info"].exchanges
    assert tiled.join_routes(call_routes(engines, f, t, cap=8))[1][0].tolist() == want[1].ids[:2].tolist()
    parts = call_routes(engines, f, t, cap=total + 5)  # a second call with room needs no new solve
    assert_routes("room", tiled, parts, G, want)
    assert parts[0]["info"].exchanges == exchanges0
    parts = call_routes(engines, f, t, cap=0)  # node_gids = xyz = NULL: infos only
    assert all(p["gids"] is None and p["xyz"] is None and not p["offsets"].any() for p in parts)
    assert_routes("infos only", tiled, parts, G, want, cap=0)
    infos = (type(parts[0]["infos"][0]) * 4)()
    offs = np.full(5, 7, np.int32)
    ff, tt = np.array(f, np.int32), np.array(t, np.int32)
    ip = C.POINTER(C.c_int32)
    got, _ = run_ranks(engines, lambda r, e: e.L.trg_engine_tiled_field_routes(
        e.h, 4, ff.ctypes.data_as(ip), tt.ctypes.data_as(ip), offs.ctypes.data_as(ip), None, None, 100, infos, None)
        if r == 0 else e.tiled_routes(f, t, cap=0))
    assert got[0] == 0 and not offs.any() and [i.num_nodes for i in infos] == [len(w.ids) for w in want]
    close(engines)


# ---- 9. staleness and failures ------------------------------------------------------------------------------------------
def failing(engines, fields, targets):
    from trg_planner._engine import TrgError
    got, secs = run_ranks(engines, lambda r, e: e.tiled_routes(fields, targets))
    assert all(isinstance(g, TrgError) for g in got), got
    assert secs < 10.0, secs  # (the transport's wait limit is 20 s: nobody ran into it)
    return got


def test_staleness_and_failures(tmp_path, tiled, ref):
    engines, restitch, G, fields = reentry(tmp_path, tiled, ref, "stale")
    pairs = [(0, 3), (1, 0)]
    f, t = [p[0] for p in pairs], [p[1] for p in pairs]
    want = want_routes(G, fields, pairs)
    PEER = "another rank reported a failure"

    def works():
        solve(engines, [0, 6])
        assert_routes("after a failure", tiled, call_routes(engines, f, t), G, want)

    # before any tiled solve: every rank's own message
    for g in failing(engines, f, t):
        assert g.status == INVALID_ARG and "no tiled solve is retained" in str(g), g
    works()
    # a field outside the solve's, on one rank alone: the message names the route
    from trg_planner._engine import TrgError
    got, secs = run_ranks(engines, lambda r, e: e.tiled_routes([0, 2] if r == 1 else f, t))
    assert isinstance(got[1], TrgError) and got[1].status == INVALID_ARG and "field 2 of route 1" in str(got[1]), got[1]
    assert isinstance(got[0], TrgError) and got[0].status == DEVICE and PEER in str(got[0]) and secs < 10.0
    assert_routes("after a bad field", tiled, call_routes(engines, f, t), G, want)  # (the solve is still retained)
    # one rank whose solve is missing: a fresh engine in rank 1's place
    fresh = restitch(1)
    pair = [engines[0], fresh]
    join_group(pair, "routes-stale-fresh")
    got = failing(pair, f, t)
    assert got[1].status == INVALID_ARG and "no tiled solve is retained" in str(got[1]), got[1]
    assert got[0].status == DEVICE and PEER in str(got[0]), got[0]
    fresh.close()
    join_group(engines, "routes-stale-again")
    assert_routes("the old group again", tiled, call_routes(engines, f, t), G, want)
    # one tile's graph changed: that rank's solve is stale
    engines[1].load_json(str(tmp_path / "stale1.json"))
    got = failing(engines, f, t)
    assert got[1].status == INVALID_ARG and "stale" in str(got[1]), got[1]
    assert got[0].status == DEVICE and PEER in str(got[0]), got[0]
    # a solve that fails (rank 1 has no current rows) retains nothing, on any rank
    got, _ = run_ranks(engines, lambda r, e: e.tiled_cost_fields([0, 6]))
    assert all(isinstance(g, TrgError) for g in got), got
    for g in failing(engines, f, t):
        assert g.status == INVALID_ARG and "no tiled solve is retained" in str(g), g
    restitch(1, engines[1])
    works()
    close(engines)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_group_and_the_solve_usable(tmp_path, tiled, ref):
    import trg_planner
    from trg_planner._engine import TrgError, TrgTiledRouteInfo
    engines, _, G, fields = reentry(tmp_path, tiled, ref, "refuse")
    pairs = [(0, 3), (1, 0)]
    f, t = [p[0] for p in pairs], [p[1] for p in pairs]
    want = want_routes(G, fields, pairs)
    solve(engines, [0, 6])
    ip = C.POINTER(C.c_int32)
    ff, tt, off = np.array(f, np.int32), np.array(t, np.int32), np.zeros(3, np.int32)
    p = lambda a: a.ctypes.data_as(ip)  # noqa: E731
    infos = (TrgTiledRouteInfo * 2)()
    raw = lambda e, n, a, b, c, cap: e.L.trg_engine_tiled_field_routes(e.h, n, a, b, c, None, None, cap, infos, None)  # noqa: E731
    for args, text in (((-1, p(ff), p(tt), p(off), 0), "n_routes < 0"), ((2, p(ff), p(tt), p(off), -1), "cap < 0"),
                       ((2, None, p(tt), p(off), 0), "null route_field"), ((2, p(ff), None, p(off), 0), "null route_field"),
                       ((2, p(ff), p(tt), None, 0), "null route_field")):
        got, secs = run_ranks(engines, lambda r, e: (raw(e, *args), e.L.trg_engine_last_error(e.h).decode()))
        assert all(g[0] == INVALID_ARG and text in g[1] for g in got) and secs < 5.0, (text, got)
        assert_routes("after " + text, tiled, call_routes(engines, f, t), G, want)
    for bad in (7, -1):
        got, secs = run_ranks(engines, lambda r, e: e.tiled_routes(f, [3, bad]))
        for g in got:
            assert isinstance(g, TrgError) and g.status == INVALID_ARG and "of route 1 is outside [0, 7)" in str(g), g
        assert secs < 5.0
    got, _ = run_ranks(engines, lambda r, e: e.tiled_routes([], []))  # n_routes == 0: TRG_OK without a collective
    assert all(g["infos"] == [] and g["offsets"].tolist() == [0] and g["info"].exchanges == 0 for g in got), got
    assert engines[0].tiled_routes([], [])["offsets"].tolist() == [0]  # (one rank alone: nobody is waited for)
    lone = trg_planner.Engine(**MOUNTAIN)
    lone.load_json(str(tmp_path / "refuse0.json"))
    with pytest.raises(TrgError) as ex:
        lone.tiled_routes(f, t)
    assert ex.value.status == INVALID_ARG and "no communicator" in str(ex.value)
    lone.close()
    assert_routes("after the refusals", tiled, call_routes(engines, f, t), G, want)
    close(engines)


# ---- 11. the single-engine solve is left alone ----------------------------------------------------------------------------
def test_the_single_engine_solve_still_answers(tmp_path, tiled, ref):
    engines, _, G, fields = reentry(tmp_path, tiled, ref, "single")
    e = engines[0]
    e.cost_fields(source_ids=[0, 3], full=False)
    before = e.routes([0, 1, 0], [3, 1, 2])
    solve(engines, [0, 6])
    pairs = [(0, 3), (1, 0)]
    assert_routes("single", tiled, call_routes(engines, [0, 1], [3, 0]), G, want_routes(G, fields, pairs))
    after = e.routes([0, 1, 0], [3, 1, 2])
    for (a_ids, a_xyz, a), (b_ids, b_xyz, b) in zip(before, after):
        assert np.array_equal(a_ids, b_ids) and np.array_equal(a_xyz, b_xyz)
        assert (a.num_nodes, bits(a.cost)[0], bits(a.path_length)[0], bits(a.avg_risk)[0]) == \
               (b.num_nodes, bits(b.cost)[0], bits(b.path_length)[0], bits(b.avg_risk)[0])
    assert before[0][0].tolist() == [0, 1, 2, 3]  # (the tile's own graph: the dear edge 1 - 2, not the way round)
    assert_routes("single, again", tiled, call_routes(engines, [0, 1], [3, 0]), G, want_routes(G, fields, pairs))
    close(engines)


# ---- 12. tiled_plan_many ----------------------------------------------------------------------------------------------------
def test_tiled_plan_many(oa, synth, tiled, ref):
    from trg_planner._engine import TrgError
    lay, engines = sc.engines(oa, synth, tiled, "2x1")
    join_group(engines, "routes-plan-many")
    stitch(engines, lay)
    G = exported(tiled, engines)
    sources, _ = pick_sources(G)
    start = sources[0]
    fields = reference(ref, G, [start])
    rng = np.random.default_rng(3)
    goals = rng.integers(0, G["V"], 12).tolist() + [start]
    want = want_routes(G, [(fields[0][0], fields[1][0], fields[2][0])], [(0, g) for g in goals])
    assert sum(trr.crossings(G["offsets"], w) > 0 for w in want) >= 2
    parts, _ = run_ranks(engines, lambda r, e: e.tiled_plan_many(start, goals))
    assert not [p for p in parts if isinstance(p, TrgError)], parts
    joined = assert_routes("plan_many", tiled, parts, G, want)
    assert all(np.array_equal(pts, G["xyz"][ids]) for ids, pts, _ in joined)
    for e in engines:
        e.comm_destroy()
