"""GPU: the cost field across tiles (trg_engine_tiled_cost_field; DESIGN.md section 7, "Cost fields across tiles")
over the in-process transport: one process, one engine and one thread per rank, all on one device.  Every rank's
cost bits, hops and parents (global ids) must equal the compiled host Dijkstra (tests/cpp/field_reference.cpp) on the
concatenation of the rows the engines export.  Built tilings, tilings without cross edges, crafted graphs (tile
graphs through load_json, crafted cross edges through stitch_assemble), the failure announcement, the refusals, and
the Python helpers."""
import numpy as np
import pytest

import field_graphs as fg
import stitch_cases as sc
import tiled_ref as tr
from field_support import MOUNTAIN
from tiled_support import (INVALID_1, RING, assert_fields, close, craft, exported, join_group, pick_sources, reference,
                           run_ranks, solve, stitch, tie_lattice)
from tiled_support import ref, tiled  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
INVALID_ARG, DEVICE = 1, 4
SF = MOUNTAIN["safety_factor"]
_solved = {}  # tiling -> (G, sources, fields of the m = 3 batch): shared by the tests that only read them


# ---- 1. built tilings -----------------------------------------------------------------------------------------------
def solved(oa, synth, tiled, lib, name):
    if name in _solved:
        return _solved[name]
    lay, engines = sc.engines(oa, synth, tiled, name)
    join_group(engines, name)
    stitch(engines, lay)
    G = exported(tiled, engines)
    sources, has_multi = pick_sources(G)
    assert has_multi == (lay.cols > 1 and lay.rows > 1), (name, has_multi)
    stitch(engines, lay)  # (again: the rows are in HBM, where the first solve reads them)
    want = reference(lib, G, sources)
    off = G["offsets"]
    for k, s in enumerate(sources):  # m = 1; the second and third run on the first one's solve graph and buffers
        got, secs = solve(engines, [s])
        infos = [g["info"] for g in got]
        print(name, "source", s, "exchanges", infos[0].exchanges, "rounds", [i.rounds for i in infos], "records",
              [i.records_sent for i in infos], "ghosts", [i.ghosts for i in infos], f"{secs * 1e3:.1f} ms")
        f = assert_fields(f"{name} m=1 source {s}", got, G, tuple(w[k:k + 1] for w in want))
        t_src = int(np.searchsorted(off, s, side="right") - 1)
        others = np.ones(G["V"], bool)
        others[int(off[t_src]):int(off[t_src + 1])] = False
        assert (f["hops"][0][others] >= 0).any(), "no node of another tile was reached"
        assert all(i.exchanges == infos[0].exchanges and i.exchanges >= 2 for i in infos)
        assert infos[0].exchanges >= 4  # (news crossed a seam in both passes)
    for call in range(2):  # one batch of m = 3, twice
        got, secs = solve(engines, sources)
        f = assert_fields(f"{name} m=3 call {call}", got, G, want)
    _solved[name] = (G, sources, f)
    for e in engines:
        e.comm_destroy()
    return _solved[name]


@pytest.mark.parametrize("name", ["2x1", "2x2", "3x3"])
def test_built_tilings(oa, synth, tiled, ref, name):
    G, sources, f = solved(oa, synth, tiled, ref, name)
    assert f["cost"].shape == (3, G["V"])


# ---- 2. tilings without cross edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["empty_mid", "island_mid"])
def test_no_cross_edges(oa, synth, tiled, ref, name):
    lay, engines = sc.engines(oa, synth, tiled, name)
    join_group(engines, name)
    assert stitch(engines, lay)[1] == 0
    G = exported(tiled, engines)
    off = G["offsets"]
    src = int(np.flatnonzero((G["state"][:off[1]] != fg.INVALID) & (np.diff(G["rowptr"])[:off[1]] > 0))[0])
    got, _ = solve(engines, [src])
    f = assert_fields(name, got, G, reference(ref, G, [src]))
    assert (f["hops"][0][off[1]:] == -1).all() and (f["hops"][0][:off[1]] >= 0).sum() > 10
    assert [g["info"].ghosts for g in got] == [0, 0, 0] and [g["info"].exchanges for g in got] == [2, 2, 2]
    for e in engines:
        e.comm_destroy()


# ---- 3. crafted graphs ----------------------------------------------------------------------------------------------
def crafted(tmp_path, tiled, lib, sizes, edges, sources, state=None, tag="craft", batch=True):
    """craft, export, solve (each source alone, then all in one batch), compare -> (engines, G, want, last results)"""
    engines, _ = craft(tmp_path, sizes, edges, state, tag)
    G = exported(tiled, engines)
    want = reference(lib, G, sources)
    got = None
    for k, s in enumerate(sources if batch else []):
        got, _ = solve(engines, [s])
        assert_fields(f"{tag} source {s}", got, G, tuple(w[k:k + 1] for w in want))
    got, _ = solve(engines, sources)
    assert_fields(f"{tag} batch", got, G, want)
    return engines, G, want, got


def test_chain_alternating_between_two_tiles(tmp_path, tiled, ref):
    """(a) every edge of a 64-node chain is a cross edge: the field advances one exchange per node."""
    gid = lambda p: (p % 2) * 32 + p // 2  # noqa: E731
    dist = np.array(fg.CHAIN_DIST, np.float32)
    edges = [(gid(p), gid(p + 1), 0.1 * (p % 3), float(dist[p % len(dist)])) for p in range(63)]
    engines, G, want, got = crafted(tmp_path, tiled, ref, [32, 32], edges, [gid(0), gid(40)], tag="chain")
    assert (want[1][0] >= 0).all() and want[1][0].max() == 63
    got, _ = solve(engines, [gid(0)])
    assert [g["info"].exchanges for g in got] == [got[0]["info"].exchanges] * 2
    assert got[0]["info"].exchanges >= 2 * 32, got[0]["info"].exchanges
    # each rank published every one of its nodes, one per exchange, and none twice per pass
    assert [g["info"].records_sent for g in got] == [64, 64] and [g["info"].ghosts for g in got] == [32, 32]
    close(engines)


def test_lattice_of_exact_ties_across_seams(tmp_path, tiled, ref):
    """(b) unit costs on a lattice in three tiles: nearly every node has several tight predecessors, local ones and
    ghosts of lower and of higher tiles; the parent is the least GLOBAL id among them."""
    sizes, edges, sources = tie_lattice()
    engines, G, want, got = crafted(tmp_path, tiled, ref, sizes, edges, sources, tag="lattice")
    # the precondition: both orders occur among the tight predecessors of some node
    off = G["offsets"]
    tile_of = np.searchsorted(off, np.arange(G["V"]), side="right") - 1
    cost, hops, parent = (w[0] for w in want)
    ghost_wins = local_wins = 0
    for v in range(G["V"]):
        preds = [int(u) for u in G["col"][G["rowptr"][v]:G["rowptr"][v + 1]] if cost[u] + 1.0 == cost[v]]
        ghosts = [u for u in preds if tile_of[u] != tile_of[v]]
        local = [u for u in preds if tile_of[u] == tile_of[v]]
        if ghosts and local:
            ghost_wins += min(ghosts) < min(local) and parent[v] == min(ghosts)
            local_wins += min(local) < min(ghosts) and parent[v] == min(local)
    assert ghost_wins > 3 and local_wins > 3, (ghost_wins, local_wins)
    close(engines)


def test_hops_behind_a_seam_need_the_second_pass(tmp_path, tiled, ref):
    """(c) two walks whose prefix costs differ by less than an ulp of the sum, the dearer prefix shorter in hops, the
    node they meet at behind the seam."""
    edges = [(0, 3, 0.0, 1.0000001), (0, 1, 0.0, 0.25), (1, 2, 0.0, 0.25), (2, 3, 0.0, 0.5), (3, 4, 0.0, 33554432.0),
             (4, 5, 0.0, 1.0)]
    for sizes in ([4, 2], [3, 1, 2]):
        engines, G, want, got = crafted(tmp_path, tiled, ref, sizes, edges, [0], tag=f"ulp{len(sizes)}")
        one = tr.single_pass_hops(G["V"], G["rowptr"], G["col"], G["w"], G["dist"], G["state"], SF, 0)
        assert want[1][0][4] == 4 and one[4] == 2, (want[1][0], one)  # the precondition: one pass gets node 4 wrong
        close(engines)


def test_zero_cost_cross_edges_and_saturation(tmp_path, tiled, ref):
    """(d) cross edges of cost 0, and a fold that reaches +inf on its way across the seam: such nodes are reached."""
    big = 3.0e38
    # two branches from node 0: one whose fold saturates on the cross edge 1 - 4 and stays +inf behind it, one that
    # crosses the seam three times at cost 0
    edges = [(0, 1, 0.0, big), (1, 4, 0.0, big), (4, 5, 0.0, 1.0), (5, 8, 0.0, big), (8, 9, 0.0, 1.0),
             (0, 2, 0.0, 0.5), (2, 6, 0.7, 0.0), (6, 3, 0.0, 0.0), (3, 7, 0.2, 0.0)]
    engines, G, want, got = crafted(tmp_path, tiled, ref, [4, 6], edges, [0, 9], tag="sat")
    assert np.isinf(want[0]).any() and (want[1][np.isinf(want[0])] >= 0).all()  # saturated, and reached
    assert want[0][0][3] == np.float32(0.5) and want[1][0][3] == 3  # through two zero-cost cross edges
    close(engines)


def test_invalid_border_node(tmp_path, tiled, ref):
    """(e) an Invalid node with cross edges: no walk enters it from either side."""
    state = np.zeros(8, np.int32)
    state[1] = fg.INVALID
    engines, G, want, got = crafted(tmp_path, tiled, ref, [4, 4], INVALID_1, [0, 7, 1], state=state, tag="invalid")
    assert want[1][0][1] == -1 and want[1][1][1] == -1 and (np.delete(want[1][0], 1) >= 0).all()
    close(engines)


def test_long_ghost_row_and_publish_across_blocks(tmp_path, tiled, ref):
    """(f) one node of tile 1 is the other end of 600 cross edges (a ghost row of 600 in tile 0, 600 ghosts in tile 1),
    and tile 0 has 600 border nodes: 2 400 border items at m = 4, more than a 2 048-item block of the compaction."""
    nA, nB = 600, 5
    edges = [(i, nA, 0.1 * (i % 5), 0.5 + 0.001 * (i % 17)) for i in range(nA)]
    edges += [(i, i + 1, 0.05 * (i % 3), 0.3 + 0.002 * (i % 11)) for i in range(nA - 1)]
    edges += [(nA + j, nA + j + 1, 0.0, 0.4) for j in range(nB - 1)]
    sources = [nA, 0, 300, nA + nB - 1]
    engines, G, want, got = crafted(tmp_path, tiled, ref, [nA, nB], edges, sources, tag="fan", batch=False)
    assert got[0]["info"].border_nodes == nA and got[0]["info"].ghosts == 1 and got[1]["info"].ghosts == nA
    assert 4 * got[0]["info"].border_nodes > 2048 and got[0]["info"].records_sent >= 4 * nA
    close(engines)


# ---- 4. failure and refusals ----------------------------------------------------------------------------------------
def test_a_rank_without_current_rows_is_announced(tmp_path, tiled, ref):
    from trg_planner._engine import TrgError
    engines, _ = craft(tmp_path, [6, 6], RING, tag="void")
    engines[1].load_json(str(tmp_path / "void1.json"))  # its graph changed after the stitch: its rows are void
    got, secs = run_ranks(engines, lambda r, e: e.tiled_cost_fields([0]))
    assert isinstance(got[1], TrgError) and got[1].status == INVALID_ARG, got[1]
    assert "no current stitched rows" in str(got[1])
    assert isinstance(got[0], TrgError) and got[0].status == DEVICE, got[0]
    assert "another rank reported a failure" in str(got[0])
    assert secs < 10.0, secs  # (the transport's wait limit is 20 s: nobody ran into it)
    close(engines)


def test_refusals_leave_the_group_usable(tmp_path, tiled, ref):
    import trg_planner
    from trg_planner._engine import TrgError
    engines, _ = craft(tmp_path, [6, 6], RING, tag="refuse")
    G = exported(tiled, engines)
    for sources, text in (([], "m must be in [1, 64]"), ([0] * 65, "m must be in [1, 64]"), ([12], "is outside [0, 12)"),
                          ([3, -1], "is outside [0, 12)")):
        got, secs = run_ranks(engines, lambda r, e: e.tiled_cost_fields(sources))
        for g in got:
            assert isinstance(g, TrgError) and g.status == INVALID_ARG and text in str(g), g
        assert secs < 5.0
    assert engines[0].L.trg_engine_tiled_cost_field(engines[0].h, 1, None, None, None, None, None) == INVALID_ARG
    lone = trg_planner.Engine(**MOUNTAIN)
    lone.load_json(str(tmp_path / "refuse0.json"))
    with pytest.raises(TrgError) as ex:
        lone.tiled_cost_fields([0])
    assert ex.value.status == INVALID_ARG and "no communicator" in str(ex.value)
    lone.close()
    # no collective was entered: the group is whole
    got, _ = solve(engines, [0, 7])
    assert_fields("after the refusals", got, G, reference(ref, G, [0, 7]))
    assert engines[1].global_ids() == (6, 6)
    got, _ = solve(engines, [7], parent=False)
    assert got[0]["parent"] is None and tiled.concat_fields(got)["parent"] is None
    close(engines)


# ---- 5. single sources are sets of one ------------------------------------------------------------------------------
def invalid_1_state():
    state = np.zeros(8, np.int32)
    state[1] = fg.INVALID
    return state


@pytest.mark.parametrize("case", ["ring", "lattice", "invalid"])
def test_sources_equal_sets_of_one_with_their_counters(tmp_path, case):
    """Both calls run one seeding: the same fields bit for bit and the same counters, the set call's owner 0 wherever
    the field reaches.  With a duplicate source, a source that is a border node (a ghost of the other rank) and an
    Invalid source."""
    from trg_planner._engine import TrgError
    if case == "ring":
        sizes, edges, state, S, twins = [6, 6], RING, None, [0, 0, 7, 5], (0, 1)  # (0 and 5 are border nodes)
    elif case == "lattice":
        sizes, edges, sources = tie_lattice()
        state, S, twins = None, sources + sources[:1], (0, 3)
    else:
        sizes, edges, state, S, twins = [4, 4], INVALID_1, invalid_1_state(), [0, 7, 1, 1], (2, 3)
    engines, _ = craft(tmp_path, sizes, edges, state, tag="one-" + case)
    one, _ = solve(engines, S)
    sets, _ = run_ranks(engines, lambda r, e: e.tiled_cost_fields_from([[s] for s in S]))
    assert not [g for g in sets if isinstance(g, TrgError)], [str(g) for g in sets]
    for t, (a, b) in enumerate(zip(one, sets)):
        for name in ("cost", "hops", "parent"):
            x, y = a[name].view(np.int32), b[name].view(np.int32)
            assert x.shape == (len(S), sizes[t]) and np.array_equal(x, y), (case, t, name)
            assert np.array_equal(x[twins[0]], x[twins[1]]), (case, t, name, "the duplicate source's rows differ")
        assert np.array_equal(b["owner"], np.where(a["hops"] >= 0, 0, -1)), (case, t)
        for name in ("exchanges", "rounds", "records_sent", "ghosts", "border_nodes"):
            x, y = getattr(a["info"], name), getattr(b["info"], name)
            print(case, "rank", t, name, x, y)
            assert x == y, (case, t, name, x, y)
    assert sum(int((a["hops"] >= 0).sum()) for a in one) > len(S)  # (the fields left their sources)
    if case == "invalid":  # no walk enters the Invalid node; as a source it starts there and leaves
        hops = np.concatenate([a["hops"] for a in one], 1)
        assert hops[0][1] == -1 and hops[1][1] == -1 and hops[2][1] == 0 and (hops[2] >= 0).all(), hops
    close(engines)


def test_a_tile_without_nodes_between_two_with_cross_edges(tmp_path, tiled, ref):
    """Sizes [6, 0, 6]: the middle rank has neither nodes nor entries; it only takes part in the exchanges."""
    S = [0, 8, 5]
    engines, _ = craft(tmp_path, [6, 0, 6], RING, tag="hollow")
    G = exported(tiled, engines)
    got, _ = solve(engines, S)
    assert_fields("hollow", got, G, reference(ref, G, S))  # (the empty rank's part: m x 0 arrays)
    assert got[1]["cost"].shape == (3, 0) and got[1]["hops"].shape == (3, 0) and got[1]["parent"].shape == (3, 0)
    exchanges = [g["info"].exchanges for g in got]
    assert exchanges == [exchanges[0]] * 3 and exchanges[0] >= 4, exchanges
    assert [g["info"].ghosts for g in got] == [2, 0, 2] and [g["info"].border_nodes for g in got] == [2, 0, 2]
    close(engines)


# ---- 6. the Python helpers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2x1", "2x2", "3x3"])
def test_field_route_over_concatenated_fields(oa, synth, tiled, ref, name):
    import trg_planner
    G, sources, f = solved(oa, synth, tiled, ref, name)
    want = reference(ref, G, sources)
    rng = np.random.default_rng(len(name) + G["V"])
    walker = trg_planner.Engine.field_path
    for k, s in enumerate(sources):
        reached = np.flatnonzero(want[1][k] >= 0)
        for t in rng.choice(reached, 10).tolist() + np.flatnonzero(want[1][k] < 0)[:1].tolist():
            route = tiled.field_route(f, k, t)
            if want[1][k][t] < 0:
                assert route == []
            else:
                assert route == walker(None, want[2][k], t, source=s), (name, s, t)
