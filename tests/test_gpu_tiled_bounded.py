"""GPU: bounded fields across tiles (trg_engine_tiled_cost_field_bounded / _risk_field_bounded / _field_reached;
DESIGN.md section 7, "Bounded fields across tiles") over the in-process transport: one process, one engine and one
thread per rank, all on one device.  Every rank must be bit-equal to bound_ref.truncate of the compiled host Dijkstra on
the exported rows, at the bound computed on the host from that reference -- min(budget, bound_ref.settle_bound) -- and
every rank's bound_out must be that bound."""
import numpy as np
import pytest

import bound_ref
import stitch_cases as sc
from tiled_support import (RING, assert_fields, close, craft, exported, host_fields, join_group, ok, pick_sources, reference,
                           risk_reference, run_ranks, solve, stitch, tie_lattice, want_routes)
from tiled_support import cost_ref, risk_reference_lib, tiled  # noqa: F401  (fixtures; risk_reference_lib is `ref`)

pytestmark = pytest.mark.gpu
INVALID_ARG, DEVICE = 1, 4
F32 = np.float32
INF = F32(np.inf)
COST, RISK = ("cost", "hops", "parent"), ("risk", "hops", "parent")


# ---- the calls and the reference ------------------------------------------------------------------------------------
def bounded(engines, sources, budget=None, settle=None, settle_gids=None, risk=False, parent=True):
    """the single-source form on every rank -> the ranks' dicts"""
    return ok(run_ranks(engines, lambda r, e: (e.tiled_risk_fields_bounded if risk else e.tiled_cost_fields_bounded)(
        sources, budget=budget, settle=settle, settle_gids=settle_gids, parent=parent))[0])


def truncated(want, budget, mode=None, targets=()):
    """(the reference fields truncated by the definition, the bound per field)"""
    m = want[0].shape[0]
    budget = np.broadcast_to(np.asarray(INF if budget is None else budget, F32).reshape(-1), (m,))
    bound = np.array([min(F32(budget[k]), bound_ref.settle_bound(want[0][k], want[1][k], targets, mode))
                      for k in range(m)], F32)
    return bound_ref.truncate(*want, bound), bound


def assert_bounded(at, got, G, want, budget, mode=None, targets=(), names=COST):
    """every rank against the truncated reference, its bound and its reached counts -> (the truncated reference, bound)"""
    trunc, bound = truncated(want, budget, mode, targets)
    assert_fields(at, got, G, trunc, names)
    off = G["offsets"]
    for t, g in enumerate(got):
        assert np.array_equal(g["bound"].view(np.uint32), bound.view(np.uint32)), (at, t, g["bound"], bound)
        a, b = int(off[t]), int(off[t + 1])
        assert g["reached"].tolist() == (trunc[1][:, a:b] >= 0).sum(1).tolist(), (at, t, g["reached"])
    print(at, "bound", bound.tolist(), "exchanges", got[0]["info"].exchanges, "records",
          [g["info"].records_sent for g in got], "reached", [g["reached"].tolist() for g in got])
    return trunc, bound


# ---- 1. a built tiling ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", ["cost", "risk"])
def test_built_tiling_with_a_budget_per_field(oa, synth, tiled, cost_ref, ref, objective):
    lay, engines = sc.engines(oa, synth, tiled, "2x1")
    join_group(engines, "bounded-2x1-" + objective)
    stitch(engines, lay)
    G = exported(tiled, engines)
    sources, _ = pick_sources(G)
    stitch(engines, lay)
    risk = objective == "risk"
    names = RISK if risk else COST
    want = risk_reference(ref, G, [[s] for s in sources]) if risk else reference(cost_ref, G, sources)
    reached0 = np.sort(want[0][1][want[1][1] >= 0])
    budgets = np.array([0.0, reached0[reached0.size // 2], np.inf], F32)
    got = bounded(engines, sources, budget=budgets, risk=risk)
    trunc, _ = assert_bounded(f"2x1 {objective} budgets", got, G, want, budgets, names=names)
    full = (want[1] >= 0).sum(1)
    left = (trunc[1] >= 0).sum(1)
    assert left[2] == full[2] and 0 < left[1] < full[1], (left, full)  # the median budget truncates and leaves
    assert sum(int(g["reached"][1]) for g in got) == left[1]
    # the five budgets of field 0, as five fields from its source
    five = np.array(bound_ref.five_budgets(want[0][0], want[1][0]), F32)
    got = bounded(engines, [sources[0]] * 5, budget=five, risk=risk)
    assert_bounded(f"2x1 {objective} five budgets", got, G, tuple(np.repeat(w[:1], 5, 0) for w in want), five, names=names)
    for e in engines:  # (stitch_cases keeps the engines for the module's other case)
        e.comm_destroy()


# ---- 2. the chain -----------------------------------------------------------------------------------------------------
def gid(p):
    return (p % 2) * 32 + p // 2


def chain_edges(pos=gid):
    """a 64-node chain whose nodes alternate between two tiles; every edge costs more than an ulp of any cost on it"""
    return [(pos(p), pos(p + 1), 0.1 * (p % 3), 0.4 + 0.05 * (p % 4)) for p in range(63)]


def test_chain_with_a_budget_stays_short(tmp_path, tiled, cost_ref):
    engines, _ = craft(tmp_path, [32, 32], chain_edges(), tag="bchain")
    G = exported(tiled, engines)
    want = reference(cost_ref, G, [gid(0)])
    along = np.array([want[0][0][gid(p)] for p in range(64)], F32)
    assert (np.diff(along) > 0).all()  # the precondition: the costs grow along the chain
    full, _ = solve(engines, [gid(0)])
    for budget, n in ((along[20], 21), (np.nextafter(along[20], F32(0.0)), 20)):
        got = bounded(engines, [gid(0)], budget=budget)
        trunc, _ = assert_bounded(f"chain budget {budget!r}", got, G, want, budget)
        assert sorted(np.flatnonzero(trunc[1][0] >= 0).tolist()) == sorted(gid(p) for p in range(n))
        assert [g["info"].exchanges for g in got] == [got[0]["info"].exchanges] * 2
        assert got[0]["info"].exchanges < full[0]["info"].exchanges, (got[0]["info"].exchanges, full[0]["info"].exchanges)
        for g in got:
            assert g["info"].records_sent <= 2 * int(g["reached"][0]), (g["info"].records_sent, g["reached"])
    close(engines)


# ---- 3. settle targets ------------------------------------------------------------------------------------------------
def gid2(p):
    return (p % 2) * 33 + p // 2


LONE, BAD = 32, 65  # in chain2: a node without edges, and an Invalid one


def test_settle_on_the_chain(tmp_path, tiled, cost_ref):
    """chain positions in [33, 33] nodes: node 32 has no edge, node 65 is Invalid"""
    state = np.zeros(66, np.int32)
    state[BAD] = -1
    engines, _ = craft(tmp_path, [33, 33], chain_edges(gid2), state=state, tag="bsettle")
    G = exported(tiled, engines)
    src = gid2(0)
    want = reference(cost_ref, G, [src])
    cost = lambda p: want[0][0][gid2(p)]  # noqa: E731
    assert want[1][0][LONE] == -1 and want[1][0][BAD] == -1
    full, _ = solve(engines, [src])
    cases = [("any", [gid2(10), gid2(4)], None, cost(4)), ("all", [gid2(10), gid2(4)], None, cost(10)),
             ("any", [gid2(5), gid2(11)], None, cost(5)), ("all", [gid2(5), gid2(11)], None, cost(11)),
             ("all", [gid2(6), LONE], cost(30), cost(30)),      # an unreachable target: the budget
             ("all", [gid2(6), gid2(40)], cost(20), cost(20)),  # a target beyond the budget: the budget
             ("any", [LONE, BAD], None, INF), ("any", [LONE, BAD], cost(9), cost(9)),  # no reachable target
             ("any", [gid2(7), gid2(7), BAD], None, cost(7)), ("all", [gid2(7), gid2(3), gid2(7)], None, cost(7)),
             ("all", [gid2(7), BAD], None, INF), ("any", [src, gid2(9)], None, F32(0.0))]
    for mode, targets, budget, bound in cases:
        got = bounded(engines, [src], budget=budget, settle=mode, settle_gids=targets)
        _, b = assert_bounded(f"chain {mode} {targets} budget {budget!r}", got, G, want, budget, mode, targets)
        assert b.view(np.uint32)[0] == np.array([bound], F32).view(np.uint32)[0], (mode, targets, b, bound)
        if np.isfinite(bound) and bound < cost(40):
            assert got[0]["info"].exchanges < full[0]["info"].exchanges
    close(engines)


def test_settle_on_the_lattice_of_exact_ties(tmp_path, tiled, cost_ref):
    """three tiles, unit costs: many nodes lie AT the bound and stay, each with its least-global-id parent"""
    sizes, edges, sources = tie_lattice()
    engines, _ = craft(tmp_path, sizes, edges, tag="blattice")
    G = exported(tiled, engines)
    off = G["offsets"]
    src = sources[0]
    want = reference(cost_ref, G, [src])
    tile_of = np.searchsorted(off, np.arange(G["V"]), side="right") - 1
    t_src = int(tile_of[src])
    near = [int(v) for v in np.flatnonzero((want[0][0] >= 2) & (want[0][0] <= 6))]
    here = [v for v in near if tile_of[v] == t_src][:3]
    there = [v for v in near if tile_of[v] != t_src][:3]
    each = [[v for v in near if tile_of[v] == t][-1] for t in range(3)]
    assert len(here) == 3 and len(there) == 3 and len({int(tile_of[v]) for v in there}) >= 1
    for mode in ("any", "all"):
        for targets in (here, there) + ((each,) if mode == "all" else ()):
            got = bounded(engines, [src], settle=mode, settle_gids=targets)
            trunc, b = assert_bounded(f"lattice {mode} {targets}", got, G, want, None, mode, targets)
            at_bound = int(((trunc[0][0] == b[0]) & (trunc[1][0] >= 0)).sum())
            assert at_bound >= 2 and (trunc[1][0] >= 0).sum() < G["V"], (mode, targets, at_bound)
    # all three fields at once, the median budget of each beside the settle targets
    want3 = reference(cost_ref, G, sources)
    budgets = np.array([bound_ref.five_budgets(want3[0][k], want3[1][k])[2] for k in range(3)], F32)
    got = bounded(engines, sources, budget=budgets, settle="all", settle_gids=each)
    assert_bounded("lattice m=3", got, G, want3, budgets, "all", each)
    close(engines)


# ---- 4. sets ----------------------------------------------------------------------------------------------------------
def test_sets_with_start_costs_and_owners(tmp_path, tiled):
    sizes, edges, sources = tie_lattice()
    engines, _ = craft(tmp_path, sizes, edges, tag="bsets")
    G = exported(tiled, engines)
    off = G["offsets"]
    sets = [[sources[0], sources[1], sources[2]], [sources[2], sources[2], int(off[1])]]
    starts = [np.array([0.0, 1.5, 2.0], F32), np.array([0.5, 0.25, 0.0], F32)]
    full = host_fields(G, sets, starts)
    want = tuple(np.stack([getattr(f, n) for f in full]) for n in ("cost", "hops", "parent"))
    budgets = np.array([bound_ref.five_budgets(f.cost, f.hops)[2] for f in full], F32)
    trunc, bound = truncated(want, budgets)
    owner = np.where(trunc[1] >= 0, np.stack([f.owner for f in full]), -1).astype(np.int32)
    assert ((trunc[1] < 0) & (want[1] >= 0)).any()  # something is truncated
    targets = [np.arange(0, s, 3, dtype=np.int32) for s in sizes]
    got = ok(run_ranks(engines, lambda r, e: e.tiled_cost_fields_from_bounded(sets, starts, budget=budgets,
                                                                                   targets=targets[r]))[0])
    assert_fields("bounded sets", got, G, trunc + (owner,), COST + ("owner",))
    for t, g in enumerate(got):
        a = int(off[t])
        assert np.array_equal(g["bound"].view(np.uint32), bound.view(np.uint32)), (t, g["bound"], bound)
        assert np.array_equal(g["cost_at"].view(np.uint32), trunc[0][:, a + targets[t]].view(np.uint32)), t
        assert np.array_equal(g["owner_at"], owner[:, a + targets[t]]) and np.array_equal(g["hops_at"], trunc[1][:, a + targets[t]])
    for k in range(2):
        owned = sum(g["owned"][k] for g in got)
        assert owned.tolist() == np.bincount(owner[k][owner[k] >= 0], minlength=len(sets[k])).tolist(), (k, owned)
        assert int(owned.sum()) == int((trunc[1][k] >= 0).sum()) == sum(int(g["reached"][k]) for g in got)
    close(engines)


# ---- 5. routes --------------------------------------------------------------------------------------------------------
def route_key(joined):
    return [(ids.tolist(), i.num_nodes, F32(i.cost).tobytes(), F32(i.path_length).tobytes(), F32(i.avg_risk).tobytes(),
             i.root_gid) for ids, _, i in joined]


def test_routes_from_a_bounded_solve(tmp_path, tiled, cost_ref):
    engines, _ = craft(tmp_path, [32, 32], chain_edges(), tag="broutes")
    G = exported(tiled, engines)
    want = reference(cost_ref, G, [gid(0)])
    bounded(engines, [gid(0)], budget=want[0][0][gid(20)], parent=False)
    parts = ok(run_ranks(engines, lambda r, e: e.tiled_routes([0, 0], [gid(12), gid(40)]))[0])
    joined = tiled.join_routes(parts)
    ref_routes = want_routes(G, [tuple(w[0] for w in want)], [(0, gid(12)), (0, gid(40))])
    assert joined[0][0].tolist() == ref_routes[0].ids.tolist() == [gid(p) for p in range(13)]
    assert F32(joined[0][2].cost).tobytes() == F32(ref_routes[0].cost).tobytes()
    assert F32(joined[0][2].path_length).tobytes() == F32(ref_routes[0].path_length).tobytes()
    assert joined[1][2].num_nodes == 0 and joined[1][0].size == 0 and joined[1][2].root_gid == -1  # beyond the bound
    close(engines)


def test_early_exit_gives_the_same_routes(tmp_path, tiled):
    sizes, edges, sources = tie_lattice()
    weighted = [(a, b, 0.1 * ((3 * a + 5 * b) % 4), d) for a, b, _, d in edges]
    engines, _ = craft(tmp_path, sizes, weighted, tag="bearly")
    V = sum(sizes)
    goals = [sources[2], 3, sizes[0] + 2, sizes[0] + sizes[1] + 1, sources[2]]
    assert max(goals) < V
    for call in ("tiled_plan_many", "tiled_safest_routes"):
        plain = ok(run_ranks(engines, lambda r, e: getattr(e, call)(sources[0], goals))[0])
        early = ok(run_ranks(engines, lambda r, e: getattr(e, call + "_early_exit")(sources[0], goals))[0])
        a, b = route_key(tiled.join_routes(plain)), route_key(tiled.join_routes(early))
        assert a == b and all(k[1] > 0 for k in a), call
    close(engines)


# ---- 6. the reached list ----------------------------------------------------------------------------------------------
def test_field_reached_and_reachable(tmp_path, tiled, cost_ref):
    from trg_planner._engine import TrgError
    engines, restitch = craft(tmp_path, [32, 32], chain_edges(), tag="breached")
    G = exported(tiled, engines)
    off = G["offsets"]
    want = reference(cost_ref, G, [gid(0)])
    budget = want[0][0][gid(20)]
    trunc, _ = truncated(want, budget)
    parts = ok(run_ranks(engines, lambda r, e: e.tiled_reachable(gid(0), budget))[0])
    for t, p in enumerate(parts):
        a, b = int(off[t]), int(off[t + 1])
        ids = a + np.flatnonzero(trunc[1][0][a:b] >= 0)
        assert p["gids"].tolist() == ids.tolist() and p["count"] == ids.size and ids.size > 3, (t, p["gids"])
        assert np.array_equal(p["value"].view(np.uint32), trunc[0][0][ids].view(np.uint32)), t
        assert np.array_equal(p["hops"], trunc[1][0][ids]), t
        none = engines[t].tiled_field_reached(0, cap=0)
        assert none["count"] == ids.size and none["gids"].size == 0
        first = engines[t].tiled_field_reached(0, cap=3)
        assert first["count"] == ids.size and first["gids"].tolist() == ids[:3].tolist()
        assert first["hops"].tolist() == trunc[1][0][ids[:3]].tolist()
        with pytest.raises(TrgError) as ex:
            engines[t].tiled_field_reached(1)
        assert ex.value.status == INVALID_ARG and "out of range" in str(ex.value)
    joined = tiled.concat_reached(parts)
    assert joined["gids"].tolist() == np.flatnonzero(trunc[1][0] >= 0).tolist() and joined["count"] == 21
    restitch(1, engines[1])  # tile 1's rows are assembled again: its retained solve is stale, tile 0's is not
    with pytest.raises(TrgError) as ex:
        engines[1].tiled_field_reached(0)
    assert ex.value.status == INVALID_ARG and "stale" in str(ex.value)
    assert engines[0].tiled_field_reached(0, cap=0)["count"] == parts[0]["count"]
    close(engines)


# ---- 7. a tile without nodes ------------------------------------------------------------------------------------------
def test_a_tile_without_nodes_ends_with_the_same_bound(tmp_path, tiled, cost_ref):
    engines, _ = craft(tmp_path, [6, 0, 6], RING, tag="bhollow")
    G = exported(tiled, engines)
    want = reference(cost_ref, G, [0])
    for mode, targets, budget in (("all", [2, 8], None), ("any", [3, 9], None), ("all", [2, 8], want[0][0][2]), (None, None, F32(1.0))):
        got = bounded(engines, [0], budget=budget, settle=mode, settle_gids=targets)
        _, b = assert_bounded(f"hollow {mode}", got, G, want, budget, mode, targets or ())
        assert got[1]["cost"].shape == (1, 0) and got[1]["reached"].tolist() == [0]
        assert len({g["bound"].tobytes() for g in got}) == 1 and np.isfinite(b[0])
    close(engines)


# ---- 8. without bounds the bounded entry is the unbounded call --------------------------------------------------------
def test_no_budget_and_no_settle_equal_the_unbounded_call(tmp_path, tiled):
    sizes, edges, sources = tie_lattice()
    engines, _ = craft(tmp_path, sizes, edges, tag="bsame")
    sets = [[sources[0], sources[1]], [sources[2]]]
    plain = ok(run_ranks(engines, lambda r, e: e.tiled_cost_fields_from(sets))[0])
    same = ok(run_ranks(engines, lambda r, e: e._tiled_bounded("cost", "test", sets, None, True, None, None, None, None,
                                                               True, True))[0])
    for t, (a, b) in enumerate(zip(plain, same)):
        for name in ("cost", "hops", "parent", "owner"):
            assert np.array_equal(a[name].view(np.int32), b[name].view(np.int32)), (t, name)
        assert [x.tolist() for x in a["owned"]] == [x.tolist() for x in b["owned"]]
        for name in ("exchanges", "owner_exchanges", "rounds", "records_sent", "owner_records_sent", "roots"):
            assert getattr(a["info"], name) == getattr(b["info"], name), (t, name)
        assert np.isinf(b["bound"]).all() and b["reached"].tolist() == (a["hops"] >= 0).sum(1).tolist()
    close(engines)


# ---- 9. refusals and a failing rank -------------------------------------------------------------------------------------
def test_refusals_leave_the_group_usable(tmp_path, tiled, cost_ref):
    from trg_planner import _engine
    from trg_planner._engine import TrgError
    engines, _ = craft(tmp_path, [6, 6], RING, tag="brefuse")
    G = exported(tiled, engines)
    _engine._SETTLE["no such mode"] = 7
    try:
        for kw, text in ((dict(budget=-1.0), "the budget of field 0 is negative or NaN"),
                         (dict(budget=[1.0, np.nan]), "the budget of field 1 is negative or NaN"),
                         (dict(settle="no such mode", settle_gids=[1]), "is no TRG_FIELD_SETTLE_* value"),
                         (dict(settle="any"), "a settle mode needs settle targets"),
                         (dict(settle="all", settle_gids=[]), "a settle mode needs settle targets"),
                         (dict(settle="any", settle_gids=[3, 12]), "settle target 1 (12) is outside [0, 12)"),
                         (dict(settle="all", settle_gids=[-1]), "settle target 0 (-1) is outside [0, 12)")):
            got, secs = run_ranks(engines, lambda r, e: e.tiled_cost_fields_bounded([0, 7], **kw))
            for g in got:
                assert isinstance(g, TrgError) and g.status == INVALID_ARG and text in str(g), (kw, g)
            assert secs < 5.0
    finally:
        del _engine._SETTLE["no such mode"]
    want = reference(cost_ref, G, [0, 7])
    got = bounded(engines, [0, 7], budget=[1.0, 0.6], settle="any", settle_gids=[9])
    assert_bounded("after the refusals", got, G, want, [1.0, 0.6], "any", [9])
    # a rank without current rows is announced in a bounded solve as in any other
    engines[1].load_json(str(tmp_path / "brefuse1.json"))
    got, secs = run_ranks(engines, lambda r, e: e.tiled_cost_fields_bounded([0], budget=1.0, settle="all", settle_gids=[2, 8]))
    assert isinstance(got[1], TrgError) and got[1].status == INVALID_ARG and "no current stitched rows" in str(got[1])
    assert isinstance(got[0], TrgError) and got[0].status == DEVICE and "another rank reported a failure" in str(got[0])
    assert secs < 10.0, secs
    close(engines)


# ---- 10. more than one block ------------------------------------------------------------------------------------------
def test_long_ghost_row_with_64_fields(tmp_path, tiled, cost_ref):
    """the long-ghost-row graph at m = TRG_FIELD_BATCH_MAX: 64 blocks of the bound step, every row of the table, and
    38 400 border items in the bounded publish"""
    nA, nB = 600, 5
    edges = [(i, nA, 0.1 * (i % 5), 0.5 + 0.001 * (i % 17)) for i in range(nA)]
    edges += [(i, i + 1, 0.05 * (i % 3), 0.3 + 0.002 * (i % 11)) for i in range(nA - 1)]
    edges += [(nA + j, nA + j + 1, 0.0, 0.4) for j in range(nB - 1)]
    engines, _ = craft(tmp_path, [nA, nB], edges, tag="bfan")
    G = exported(tiled, engines)
    sources = [nA, nA + nB - 1] + list(range(0, nA, 9))[:62]
    assert len(sources) == 64
    want = reference(cost_ref, G, sources)
    budgets = np.array([bound_ref.five_budgets(want[0][k], want[1][k])[k % 5] for k in range(64)], F32)
    targets = [5, 350, nA + 2, 599]
    for mode in ("all", "any"):
        got = bounded(engines, sources, budget=budgets, settle=mode, settle_gids=targets)
        trunc, b = assert_bounded(f"fan {mode}", got, G, want, budgets, mode, targets)
        assert len(set(b.tolist())) > 8 and ((trunc[1] < 0) & (want[1] >= 0)).any()
    close(engines)
