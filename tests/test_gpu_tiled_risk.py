"""GPU: the risk field across tiles (trg_engine_tiled_risk_field / _sets; DESIGN.md section 7, "Risk fields across
tiles") over the in-process transport: one process, one engine and one thread per rank, all on one device.  Every
rank's risk bits, hops, parents (global ids) and owners must equal the compiled host Dijkstra on the (risk, hops) key
(tests/cpp/risk_reference.cpp) on the concatenation of the rows the engines export.  Built tilings, crafted graphs
(plateaus, width 0, exact ties, a key that drops many times, -0 weights, duplicates, an Invalid border node, a long
ghost row, a tile without nodes), sets, objectives alternating on one stitch, the failure announcement, the refusals
and the Python helpers.  Routes: tests/test_gpu_tiled_risk_routes.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import field_graphs as fg
import risk_graphs as rg
import risk_ref
import stitch_cases as sc
import tiled_ref as trr
import tiled_support
from field_support import MOUNTAIN
from tiled_support import (INVALID_1, RING, close, exported, join_group, level_lattice, ok, pick_sources, run_ranks,
                           stitch, tie_lattice)
from tiled_support import risk_craft as craft, risk_reference as reference
from tiled_support import risk_solve as solve, risk_solve_sets as solve_sets
from tiled_support import cost_ref, risk_reference_lib, tiled  # noqa: F401  (fixtures; risk_reference_lib is `ref`)

pytestmark = pytest.mark.gpu
INVALID_ARG, DEVICE = 1, 4
F32 = np.float32
FRONTIER = 1
PEER = "another rank reported a failure"
assert_fields = functools.partial(tiled_support.assert_fields, names=("risk", "hops", "parent"))


def crafted(tmp_path, tiled, lib, sizes, edges, sources, state=None, tag="craft", extra=(), batch=True):
    """craft, export, solve (each source alone, then all in one batch), compare -> (engines, G, want, last results)"""
    engines = craft(tmp_path, sizes, edges, state, tag, extra)
    G = exported(tiled, engines)
    want = reference(lib, G, [[s] for s in sources])
    for k, s in enumerate(sources if batch else []):
        assert_fields(f"{tag} source {s}", solve(engines, [s]), G, tuple(w[k:k + 1] for w in want))
    got = solve(engines, sources)
    assert_fields(f"{tag} batch", got, G, want)
    return engines, G, want, got


def exchange_cap(got, m):
    """the most exchanges of a solve's two passes: per pass 4 m B + 64 with news and one without"""
    B = sum(g["info"].border_nodes for g in got)
    return 2 * (4 * m * B + 64 + 1)


def unique_pairs(g):
    """the undirected edges of a symmetric FieldGraph, one per pair -> [(a, b, w, dist)]"""
    rows = np.repeat(np.arange(len(g.state)), np.diff(g.rowptr))
    out = {}
    for a, b, w, d in zip(rows.tolist(), g.col.tolist(), g.w.tolist(), g.dist.tolist()):
        out.setdefault((min(a, b), max(a, b)), (w, d))
    return [(a, b, w, d) for (a, b), (w, d) in out.items() if a != b]


# ---- 1. built tilings -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2x1", "2x2", "3x3"])
def test_built_tilings(oa, synth, tiled, ref, name):
    lay, engines = sc.engines(oa, synth, tiled, name)
    join_group(engines, "risk-" + name)
    stitch(engines, lay)
    G = exported(tiled, engines)  # (the rows leave the device: the first solve reads the fetched rows)
    sources, _ = pick_sources(G)
    want = reference(ref, G, [[s] for s in sources])
    off = G["offsets"]
    for where in ("fetched rows", "rows in HBM"):
        for k, s in enumerate(sources):  # m = 1
            got = solve(engines, [s])
            infos = [g["info"] for g in got]
            print(name, where, "source", s, "exchanges", infos[0].exchanges, "rounds", [i.rounds for i in infos],
                  "records", [i.records_sent for i in infos], "ms", [round(i.ms_total, 2) for i in infos])
            assert_fields(f"{name} {where} m=1 source {s}", got, G, tuple(w[k:k + 1] for w in want))
            t_src = int(np.searchsorted(off, s, side="right") - 1)
            others = np.ones(G["V"], bool)
            others[int(off[t_src]):int(off[t_src + 1])] = False
            assert (np.concatenate([g["hops"][0] for g in got])[others] >= 0).any(), "no node of another tile was reached"
            assert all(i.exchanges == infos[0].exchanges for i in infos) and infos[0].exchanges >= 4
            assert infos[0].exchanges <= exchange_cap(got, 1)
        got = solve(engines, sources)  # m = 3
        assert_fields(f"{name} {where} m=3", got, G, want)
        f = tiled.concat_fields(got)
        assert f["risk"].shape == (3, G["V"]) and np.array_equal(f["parent"], want[2])
        stitch(engines, lay)  # (again: the rows are in HBM, where the next solve reads them)
    for e in engines:
        e.comm_destroy()


# ---- 2. rise and fall, every edge a cross edge ------------------------------------------------------------------------
def test_rise_and_fall_alternating_between_two_tiles(tmp_path, tiled, ref):
    """One exchange per node in both passes; from the peak on the risk word has stopped moving and only the hops do."""
    g = rg.rise_and_fall(64)
    gid = lambda p: (p % 2) * 32 + p // 2  # noqa: E731
    edges = [(gid(p), gid(p + 1), float(g.w[p]), 1.0) for p in range(63)]
    engines, G, want, got = crafted(tmp_path, tiled, ref, [32, 32], edges, [gid(0), gid(40)], tag="rise")
    assert want[1][0][gid(63)] == 63 and len(np.unique(want[0][0][[gid(p) for p in range(32, 64)]])) == 1
    got = solve(engines, [gid(0)])
    infos = [g["info"] for g in got]
    assert [i.exchanges for i in infos] == [infos[0].exchanges] * 2
    assert 2 * 64 <= infos[0].exchanges <= exchange_cap(got, 1), infos[0].exchanges
    assert [i.records_sent for i in infos] == [64, 64] and [i.ghosts for i in infos] == [32, 32]
    close(engines)


# ---- 3. all weights zero: width 0, with merges ------------------------------------------------------------------------
def test_all_zero_weights_in_three_tiles(tmp_path, tiled, ref):
    g = rg.all_zero_weights(24)
    engines, G, want, got = crafted(tmp_path, tiled, ref, [7, 8, 9], unique_pairs(g), [0, 23, 11], tag="zero")
    assert not G["w"].any() and (want[1] >= 0).all()
    for t in got:
        assert (t["risk"].view(np.uint32) == 0).all()
    assert sum(t["info"].ghosts for t in got) > 0 and got[0]["info"].exchanges >= 4
    sets = [[0, 23], [5], [11, 17, 3]]
    got = solve_sets(engines, sets)
    assert_fields("zero sets", got, G, reference(ref, G, sets))
    close(engines)


# ---- 4. one weight everywhere: exact ties across seams ----------------------------------------------------------------
def test_lattice_of_one_weight_ties_across_seams(tmp_path, tiled, ref):
    sizes, edges, sources = tie_lattice()
    edges = [(a, b, 0.25, d) for a, b, _, d in edges]
    engines, G, want, got = crafted(tmp_path, tiled, ref, sizes, edges, sources, tag="lattice")
    off = G["offsets"]
    tile_of = np.searchsorted(off, np.arange(G["V"]), side="right") - 1
    risk, hops, parent = (w[0] for w in want)
    ghost_wins = local_wins = 0  # the precondition: both orders occur among the tight predecessors of some node
    for v in range(G["V"]):
        preds = [int(u) for u in G["col"][G["rowptr"][v]:G["rowptr"][v + 1]] if hops[u] + 1 == hops[v]]
        ghosts = [u for u in preds if tile_of[u] != tile_of[v]]
        local = [u for u in preds if tile_of[u] == tile_of[v]]
        if ghosts and local:
            ghost_wins += min(ghosts) < min(local) and parent[v] == min(ghosts)
            local_wins += min(local) < min(ghosts) and parent[v] == min(local)
    assert ghost_wins > 3 and local_wins > 3, (ghost_wins, local_wins)
    assert set(np.unique(risk).tolist()) == {0.0, 0.25}
    close(engines)


# ---- 5. a staircase: one border key drops eight times -------------------------------------------------------------------
def test_staircase_of_a_border_key_that_drops_eight_times(tmp_path, tiled, ref):
    sizes, edges, s, t = trr.staircase(8)
    engines, G, want, got = crafted(tmp_path, tiled, ref, sizes, edges, [s], tag="stairs", batch=False)
    assert want[0][0][t] == F32(0.9 - 0.1 * 7) and want[1][0][t] == 16
    # the protocol in numpy on the exported graph: the target's key is published once per walk in pass 1
    Gd = dict(V=G["V"], rowptr=G["rowptr"], col=G["col"], w=G["w"], state=G["state"])
    *_, proto = trr.tiled_risk_field(Gd, G["offsets"], [s])
    assert proto["published"][t] >= 8, proto["published"][t]
    # the ranks relax to quiescence between exchanges, as the protocol does: the same keys at every exchange
    off = G["offsets"]
    sent = [sum(n for gid, n in proto["published"].items() if off[r] <= gid < off[r + 1]) for r in range(2)]
    infos = [g["info"] for g in got]
    print("staircase exchanges", [i.exchanges for i in infos], "protocol", proto["exchanges"], "records",
          [i.records_sent for i in infos], "protocol", sent)
    assert [i.exchanges for i in infos] == [sum(proto["exchanges"])] * 2
    assert [i.records_sent for i in infos] == sent
    assert infos[0].exchanges <= exchange_cap(got, 1) and infos[0].exchanges >= 16
    close(engines)


# ---- 6. / 7. / 8. -0 on cross edges, duplicates of different weight, an Invalid border node -----------------------------
def test_negative_zero_weights_on_cross_edges(tmp_path, tiled, ref):
    edges = [(0, 1, 0.0, 1.0), (1, 3, -0.0, 1.0), (3, 4, -0.0, 1.0), (4, 2, -0.0, 1.0), (2, 5, 0.3, 1.0),
             (0, 3, 0.0, 1.0)]
    engines, G, want, got = crafted(tmp_path, tiled, ref, [3, 3], edges, [0, 5], tag="negzero")
    tile_of = np.searchsorted(G["offsets"], np.arange(6), side="right") - 1
    rows = np.repeat(np.arange(6), np.diff(G["rowptr"]))
    cross = tile_of[rows] != tile_of[G["col"]]
    assert (G["w"][cross].view(np.uint32) == 0x80000000).sum() >= 4  # the precondition: -0 reached the rows
    assert (want[0][0][:5].view(np.uint32) == 0).all() and want[0][0][5] == F32(0.3)
    assert want[1][0].tolist() == [0, 1, 3, 1, 2, 4] and want[2][0][3] == 0  # (0 - 3 at +0 ties with 0 - 1 - 3: fewer hops)
    close(engines)


def test_parallel_duplicates_of_different_weight_before_a_seam(tmp_path, tiled, ref):
    """1 - 2 three times, at 0.9, 0.1 and 0.4: only 0.1 is tight.  Behind them the seam, and behind that a plateau."""
    edges = [(0, 1, 0.05, 1.0), (1, 2, 0.9, 1.0), (2, 4, 0.1, 1.0), (4, 5, 0.2, 1.0), (5, 3, 0.0, 1.0)]
    extra = [(1, 2, 0.1, 2.0), (1, 2, 0.4, 3.0)]
    engines, G, want, got = crafted(tmp_path, tiled, ref, [4, 2], edges, [0, 5], tag="dup", extra=extra)
    assert int(np.diff(G["rowptr"])[1]) == 4
    assert want[0][0].tolist() == [F32(x) for x in (0.0, 0.05, 0.1, 0.2, 0.1, 0.2)]
    close(engines)


def test_invalid_border_node(tmp_path, tiled, ref):
    state = np.zeros(8, np.int32)
    state[1] = fg.INVALID
    engines, G, want, got = crafted(tmp_path, tiled, ref, [4, 4], INVALID_1, [0, 7, 1], state=state, tag="invalid")
    assert want[1][0][1] == -1 and want[1][1][1] == -1 and (np.delete(want[1][0], 1) >= 0).all()
    assert want[1][2][1] == 0 and (want[1][2] >= 0).all()  # a walk may start there
    close(engines)


# ---- 9. / 10. a ghost row of 600, a tile without nodes ------------------------------------------------------------------
def test_long_ghost_row_and_publish_across_blocks(tmp_path, tiled, ref):
    nA, nB = 600, 5
    edges = [(i, nA, 0.1 * (i % 5), 0.5) for i in range(nA)]
    edges += [(i, i + 1, 0.05 * (i % 3), 0.3) for i in range(nA - 1)]
    edges += [(nA + j, nA + j + 1, 0.0, 0.4) for j in range(nB - 1)]
    sources = [nA, 0, 300, nA + nB - 1]
    engines, G, want, got = crafted(tmp_path, tiled, ref, [nA, nB], edges, sources, tag="fan", batch=False)
    assert got[0]["info"].border_nodes == nA and got[0]["info"].ghosts == 1 and got[1]["info"].ghosts == nA
    assert 4 * got[0]["info"].border_nodes > 2048 and got[0]["info"].records_sent >= 4 * nA
    close(engines)


def test_a_tile_without_nodes_between_two_with_cross_edges(tmp_path, tiled, ref):
    ring = [(a, b, 0.1 * (i % 4), d) for i, (a, b, _, d) in enumerate(RING)]
    S = [0, 8, 5]
    engines, G, want, got = crafted(tmp_path, tiled, ref, [6, 0, 6], ring, S, tag="hollow", batch=False)
    assert got[1]["risk"].shape == (3, 0) and got[1]["hops"].shape == (3, 0) and got[1]["parent"].shape == (3, 0)
    exchanges = [g["info"].exchanges for g in got]
    assert exchanges == [exchanges[0]] * 3 and exchanges[0] >= 4, exchanges
    assert [g["info"].ghosts for g in got] == [2, 0, 2]
    close(engines)


# ---- 11. sets ---------------------------------------------------------------------------------------------------------
def assert_sets(at, got, G, lib, sets, targets=None):
    want = reference(lib, G, sets)
    assert_fields(at, got, G, want)
    off = G["offsets"]
    for k, members in enumerate(sets):
        owner, owned = risk_ref.owners(np.asarray(members), want[1][k], want[2][k])
        for t, g in enumerate(got):
            a, b = int(off[t]), int(off[t + 1])
            assert np.array_equal(g["owner"][k], owner[a:b]), (at, "owner", k, t)
        assert np.array_equal(np.sum([g["owned"][k] for g in got], 0), owned), (at, "owned", k)
    if targets is not None:
        for t, g in enumerate(got):
            for full, part in (("risk", "risk_at"), ("hops", "hops_at"), ("owner", "owner_at")):
                assert np.array_equal(g[part].view(np.int32), g[full][:, targets[t]].view(np.int32)), (at, part, t)
    return want


def test_sets(tmp_path, tiled, ref):
    sizes, edges, sources = level_lattice()
    engines = craft(tmp_path, sizes, edges, tag="sets")
    G = exported(tiled, engines)
    off = G["offsets"].tolist()
    tile_of = np.searchsorted(G["offsets"], np.arange(G["V"]), side="right") - 1
    rows = np.repeat(np.arange(G["V"]), np.diff(G["rowptr"]))
    border = np.unique(rows[tile_of[rows] != tile_of[G["col"]]]).tolist()
    two = [off[0] + 2, off[2] + 5]
    five = [off[1] + 1, border[0], off[2] - 1, off[1] + 1, off[3] - 1]  # a duplicate member, one on the border
    sets = [two, five, [sources[2]]]
    targets = [np.arange(0, n, 3, dtype=np.int32) for n in sizes]
    got = solve_sets(engines, sets, targets=targets)
    want = assert_sets("sets", got, G, ref, sets, targets)
    assert len(np.unique(want[0][1])) >= 3 and sum(g["info"].owner_exchanges for g in got) >= 3 * 2
    assert sum(g["info"].roots for g in got) == sum(len(set(s)) for s in sets) == 7  # every distinct member is a root
    got = solve_sets(engines, sets, targets=targets, full=False, parent=False)  # the reads alone
    for t, g in enumerate(got):
        assert "risk" not in g and np.array_equal(g["risk_at"].view(np.uint32),
                                                  np.ascontiguousarray(want[0][:, off[t] + targets[t]]).view(np.uint32))
    close(engines)


def test_sets_with_an_invalid_member(tmp_path, tiled, ref):
    state = np.zeros(8, np.int32)
    state[1] = fg.INVALID
    engines = craft(tmp_path, [4, 4], INVALID_1, state=state, tag="sets-invalid")
    G = exported(tiled, engines)
    sets = [[1, 7], [6, 1, 0, 6]]
    want = assert_sets("sets invalid", solve_sets(engines, sets), G, ref, sets)
    assert want[1][0][1] == 0 and want[1][1][1] == 0
    close(engines)


@pytest.mark.parametrize("case", ["ring", "lattice", "invalid"])
def test_sources_equal_sets_of_one_with_their_counters(tmp_path, case):
    if case == "ring":
        sizes, state, S, twins = [6, 6], None, [0, 0, 7, 5], (0, 1)
        edges = [(a, b, 0.1 * (i % 4), d) for i, (a, b, _, d) in enumerate(RING)]
    elif case == "lattice":
        sizes, edges, sources = level_lattice()
        state, S, twins = None, sources + sources[:1], (0, 3)
    else:
        state = np.zeros(8, np.int32)
        state[1] = fg.INVALID
        sizes, edges, S, twins = [4, 4], INVALID_1, [0, 7, 1, 1], (2, 3)
    engines = craft(tmp_path, sizes, edges, state, tag="one-" + case)
    one = solve(engines, S)
    sets = solve_sets(engines, [[s] for s in S])
    for t, (a, b) in enumerate(zip(one, sets)):
        for name in ("risk", "hops", "parent"):
            x, y = a[name].view(np.int32), b[name].view(np.int32)
            assert x.shape == (len(S), sizes[t]) and np.array_equal(x, y), (case, t, name)
            assert np.array_equal(x[twins[0]], x[twins[1]]), (case, t, name, "the duplicate source's rows differ")
        assert np.array_equal(b["owner"], np.where(a["hops"] >= 0, 0, -1)), (case, t)
        for name in ("exchanges", "rounds", "records_sent", "ghosts", "border_nodes"):
            x, y = getattr(a["info"], name), getattr(b["info"], name)
            assert x == y, (case, t, name, x, y)
    assert sum(int((a["hops"] >= 0).sum()) for a in one) > len(S)
    close(engines)


# ---- 13. objectives alternate on one stitch ---------------------------------------------------------------------------
def test_objectives_alternate_on_one_stitch(tmp_path, tiled, ref, cost_ref):
    import field_ref
    sizes, edges, sources = level_lattice()
    edges = [(a, b, w, 0.5 + 0.01 * ((a + 2 * b) % 7)) for a, b, w, _ in edges]
    engines = craft(tmp_path, sizes, edges, tag="alternate")
    G = exported(tiled, engines)
    S = sources[:2]
    risk_want = reference(ref, G, [[s] for s in S])

    def cost_want(sf):
        out = [field_ref.field(cost_ref, G["rowptr"], G["col"], G["w"], G["dist"], G["state"], sf, int(s)) for s in S]
        assert all(o[0] == 0 for o in out)
        return tuple(np.stack([o[i] for o in out]) for i in (1, 2, 3))

    def cost_solve(sf):
        got = ok(run_ranks(engines, lambda r, e: e.tiled_cost_fields(S))[0])
        want = cost_want(sf)
        off = G["offsets"]
        for t, g in enumerate(got):
            a, b = int(off[t]), int(off[t + 1])
            assert np.array_equal(g["cost"].view(np.uint32), np.ascontiguousarray(want[0][:, a:b]).view(np.uint32)), t
            assert np.array_equal(g["hops"], want[1][:, a:b]) and np.array_equal(g["parent"], want[2][:, a:b]), t
        return got

    sf = MOUNTAIN["safety_factor"]
    first = cost_solve(sf)
    assert_fields("risk after cost", solve(engines, S), G, risk_want)
    again = cost_solve(sf)
    for a, b in zip(first, again):
        assert np.array_equal(a["cost"].view(np.uint32), b["cost"].view(np.uint32))
    risks = solve(engines, S)
    assert_fields("risk after cost after risk", risks, G, risk_want)
    # the two objectives differ on this graph: neither call answered with the other's array
    assert not np.array_equal(np.concatenate([g["hops"] for g in again], 1), risk_want[1])
    # another safety factor: the costs change, the risks do not -- nor is the retained risk solve stale
    for e in engines:
        e.set_option("safety_factor", "0.5")
    parts = ok(run_ranks(engines, lambda r, e: e.tiled_routes([0], [sources[1]]))[0])
    assert tiled.join_routes(parts)[0][2].num_nodes == risk_want[1][0][sources[1]] + 1
    after = solve(engines, S)
    assert_fields("risk under another safety factor", after, G, risk_want)
    for a, b in zip(risks, after):
        assert a["info"].exchanges == b["info"].exchanges and a["info"].records_sent == b["info"].records_sent
    other = cost_solve(0.5)
    assert not np.array_equal(np.concatenate([g["cost"] for g in other], 1), np.concatenate([g["cost"] for g in again], 1))
    assert_fields("risk after the other cost", solve(engines, S), G, risk_want)
    close(engines)


# ---- 14. failure and refusals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bad", [("nan", np.nan), ("negative", -1.0), ("inf", np.inf)])
def test_a_bad_weight_on_one_rank_is_announced(tmp_path, tiled, ref, cost_ref, name, bad):
    """The bad weight sits on an edge no walk uses (into the Invalid node 11): the flag is taken over all edges."""
    from trg_planner._engine import TrgError
    state = np.zeros(12, np.int32)
    state[11] = fg.INVALID
    good = [(a, b, 0.1, d) for a, b, _, d in RING if 11 not in (a, b)] + [(9, 11, 0.2, 0.5)]
    engines = craft(tmp_path, [6, 6], good + [(10, 11, bad, 0.5)], state=state, tag="bad-" + name)
    got, secs = run_ranks(engines, lambda r, e: e.tiled_risk_fields([0]))
    assert isinstance(got[1], TrgError) and got[1].status == INVALID_ARG, got[1]
    assert "tiled risk field: an edge weight is negative or not finite" in str(got[1]), got[1]
    assert isinstance(got[0], TrgError) and got[0].status == DEVICE and PEER in str(got[0]), got[0]
    assert secs < 10.0, secs  # (the transport's wait limit is 20 s: nobody ran into it)
    got, secs = run_ranks(engines, lambda r, e: e.tiled_risk_fields_from([[0, 7]]))
    assert isinstance(got[1], TrgError) and got[1].status == INVALID_ARG and "an edge weight" in str(got[1]), got[1]
    assert isinstance(got[0], TrgError) and got[0].status == DEVICE and PEER in str(got[0]) and secs < 10.0, got[0]
    # the group is whole: with the weight mended on that rank it solves both objectives
    import field_ref
    mended = tiled_support.craft(tmp_path, [6, 6], good + [(10, 11, 0.3, 0.5)], state=state, tag="risk-bad-" + name)
    close(mended[0])  # (only its files are wanted: rank 1 loads the mended tile and assembles its rows again)
    mended[1](1, engines[1])
    G = exported(tiled, engines)
    got = ok(run_ranks(engines, lambda r, e: e.tiled_cost_fields([0]))[0])
    st, c, h, p = field_ref.field(cost_ref, G["rowptr"], G["col"], G["w"], G["dist"], G["state"], MOUNTAIN["safety_factor"], 0)
    assert st == 0 and np.array_equal(np.concatenate([g["cost"][0] for g in got]).view(np.uint32), c.view(np.uint32))
    assert_fields("after the failure", solve(engines, [0, 7]), G, reference(ref, G, [[0], [7]]))
    close(engines)


def test_refusals_leave_the_group_usable(tmp_path, tiled, ref):
    import trg_planner
    from trg_planner._engine import TrgError
    ring = [(a, b, 0.1 * (i % 4), d) for i, (a, b, _, d) in enumerate(RING)]
    engines = craft(tmp_path, [6, 6], ring, tag="refuse")
    G = exported(tiled, engines)
    for sources, text in (([], "m must be in [1, 64]"), ([0] * 65, "m must be in [1, 64]"), ([12], "is outside [0, 12)"),
                          ([3, -1], "is outside [0, 12)")):
        got, secs = run_ranks(engines, lambda r, e: e.tiled_risk_fields(sources))
        for g in got:
            assert isinstance(g, TrgError) and g.status == INVALID_ARG and text in str(g), g
            assert str(g).count("tiled risk field: "), g
        assert secs < 5.0
    for sets, text in (([], "m must be in [1, 64]"), ([[0], []], "set 1 is empty"), ([[0, 12]], "is outside [0, 12)")):
        got, secs = run_ranks(engines, lambda r, e: e.tiled_risk_fields_from(sets))
        for g in got:
            assert isinstance(g, TrgError) and g.status == INVALID_ARG and text in str(g), g
        assert secs < 5.0
    e0 = engines[0]
    ip = C.POINTER(C.c_int32)
    ptr, ids = np.array([0, 1], np.int32), np.array([0], np.int32)
    p = lambda a: a.ctypes.data_as(ip)  # noqa: E731
    assert e0.L.trg_engine_tiled_risk_field(e0.h, 1, None, None, None, None, None) == INVALID_ARG
    assert "null source_gids" in e0.L.trg_engine_last_error(e0.h).decode()
    sets_call = lambda a, b, tg, n: e0.L.trg_engine_tiled_risk_field_sets(  # noqa: E731
        e0.h, 1, a, b, None, None, None, None, tg, n, None, None, None, None, None)
    assert sets_call(None, p(ids), None, 0) == INVALID_ARG and sets_call(p(ptr), None, None, 0) == INVALID_ARG
    assert "null set_ptr or set_gids" in e0.L.trg_engine_last_error(e0.h).decode()
    assert sets_call(p(ptr), p(ids), None, -1) == INVALID_ARG and sets_call(p(ptr), p(ids), None, 2) == INVALID_ARG
    assert "n_targets" in e0.L.trg_engine_last_error(e0.h).decode()
    lone = trg_planner.Engine(**MOUNTAIN)
    lone.load_json(str(tmp_path / "risk-refuse0.json"))
    for call in (lambda: lone.tiled_risk_fields([0]), lambda: lone.tiled_risk_fields_from([[0]])):
        with pytest.raises(TrgError) as ex:
            call()
        assert ex.value.status == INVALID_ARG and "no communicator" in str(ex.value)
    lone.close()
    # no collective was entered: the group is whole
    assert_fields("after the refusals", solve(engines, [0, 7]), G, reference(ref, G, [[0], [7]]))
    got = solve(engines, [7], parent=False)
    assert got[0]["parent"] is None and tiled.concat_fields(got)["parent"] is None
    close(engines)


# ---- 15. the Python helpers ---------------------------------------------------------------------------------------------
def test_frontier_ceilings_and_safest_frontier(tmp_path, tiled, ref):
    sizes, edges, sources = level_lattice()
    V = sum(sizes)
    state = np.zeros(V, np.int32)
    state[np.arange(4, V, 9)] = FRONTIER
    state[[13, 50]] = fg.INVALID
    engines = craft(tmp_path, sizes, edges, state=state, tag="frontier")
    G = exported(tiled, engines)
    members = [sources[0], sources[1], sources[0]]
    parts = ok(run_ranks(engines, lambda r, e: e.tiled_frontier_ceilings(members))[0])
    st, risk, hops, parent = risk_ref.risk_field(ref, G["rowptr"], G["col"], G["w"], G["state"], members)
    owner, _ = risk_ref.owners(np.asarray(members), hops, parent)
    frontier = np.flatnonzero(G["state"] == FRONTIER)
    off = G["offsets"]
    for t, p in enumerate(parts):
        mine = frontier[(frontier >= off[t]) & (frontier < off[t + 1])]
        assert p["gids"].tolist() == mine.tolist() and mine.size > 0, t
        assert np.array_equal(p["risk"].view(np.uint32), risk[mine].view(np.uint32)), t
        assert np.array_equal(p["hops"], hops[mine]) and np.array_equal(p["owner"], owner[mine]), t
    want = []
    for k in range(len(members)):
        mine = [int(v) for v in frontier if owner[v] == k and hops[v] >= 0]
        best = min(mine, key=lambda v: (int(risk[v:v + 1].view(np.uint32)[0]), int(hops[v]), v)) if mine else None
        want.append(None if best is None else (best, float(risk[best]), int(hops[best])))
    assert tiled.safest_frontier(parts) == want and want[2] is None and want[0] is not None and want[1] is not None
    close(engines)
