"""GPU: cost models across tiles (trg_engine_tiled_cost_field_models; DESIGN.md section 7, "Cost models across tiles")
over the in-process transport: one process, one engine and one thread per rank, all on one device.  Field k under the
model (s_k, tau_k) must be bit-equal, on every rank, to the host definition on the exported global rows: the existing
references at safety factor s_k on model_ref.prune(G, tau_k) (tests/tiled_model_ref.py) -- cost bits, hops, global-id
parents, owners, owned, bounds, reached counts and lists, and the routes with their edge sums."""
import numpy as np
import pytest

import risk_graphs as rg
import stitch_cases as sc
import tiled_model_ref as tmr
from tiled_support import (RING, SF, assert_fields, assert_routes, call_routes, close, craft, exported, join_group,
                           level_lattice, most_crossings, ok, pick_sources, run_ranks, stitch)
from tiled_support import cost_ref, tiled  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
INVALID_ARG, DEVICE = 1, 4
F32 = np.float32
INF = F32(np.inf)
COST = ("cost", "hops", "parent")
OWNED = COST + ("owner",)
PEER = "another rank reported a failure"


# ---- the calls and the reference ------------------------------------------------------------------------------------
def modelled(engines, sets, models, starts=None, targets=None, **kw):
    """the collective call on every rank (targets: per rank, or None) -> the ranks' dicts"""
    return ok(run_ranks(engines, lambda r, e: e.tiled_cost_fields_models(
        sets, models, start_costs=starts, targets=None if targets is None else targets[r], **kw))[0])


def as_sets(sets):
    return [[int(g)] for g in sets] if all(np.ndim(s) == 0 for s in sets) else [list(s) for s in sets]


def check(at, engines, G, sets, models, starts=None, **kw):
    """one modelled solve against the definition -> (the ranks' dicts, the reference's SetFields)"""
    fs = tmr.fields(G, models, as_sets(sets), starts, SF)
    got = modelled(engines, sets, models, starts, **kw)
    assert_fields(at, got, G, tmr.stacked(fs, OWNED), OWNED)
    pairs = np.array(tmr.pairs(models, SF), F32).reshape(-1, 2)
    for g in got:
        assert np.array_equal(g["models"].view(np.uint32), pairs.view(np.uint32)), (at, g["models"])
    return got, fs


def assert_bounded(at, engines, got, G, want, budget, mode=None, targets=()):
    """every rank against the truncated reference: fields, the bound, the reached counts and the reached lists"""
    trunc, bound = tmr.truncated(want, budget, mode, targets)
    assert_fields(at, got, G, trunc, COST)
    off = G["offsets"]
    for t, (g, e) in enumerate(zip(got, engines)):
        assert np.array_equal(g["bound"].view(np.uint32), bound.view(np.uint32)), (at, t, g["bound"], bound)
        a, b = int(off[t]), int(off[t + 1])
        assert g["reached"].tolist() == (trunc[1][:, a:b] >= 0).sum(1).tolist(), (at, t, g["reached"])
        for k in range(want[0].shape[0]):
            ids = a + np.flatnonzero(trunc[1][k][a:b] >= 0)
            lst = e.tiled_field_reached(k)
            assert lst["gids"].tolist() == ids.tolist() and lst["count"] == ids.size, (at, t, k, lst["gids"])
            assert np.array_equal(lst["value"].view(np.uint32), trunc[0][k][ids].view(np.uint32)), (at, t, k)
            assert np.array_equal(lst["hops"], trunc[1][k][ids]), (at, t, k)
    print(at, "bound", bound.tolist(), "exchanges", got[0]["info"].exchanges, "reached", [g["reached"].tolist() for g in got])
    return trunc, bound


# ---- 1. the ring ------------------------------------------------------------------------------------------------------
def test_ring_with_a_raised_seam_edge(tmp_path, tiled):
    ring = [(a, b, 0.5 if a == 5 else w, d) for a, b, w, d in RING]  # the seam edge 5 -- 6 at weight 0.5
    engines, _ = craft(tmp_path, [6, 6], ring, tag="mring")
    G = exported(tiled, engines)
    models = [(SF, INF), (0.0, INF), (SF, 0.2), (SF, 0.05)]
    got, fs = check("ring", engines, G, [3] * 4, models)
    # the precondition: under tau = 0.2 the far side is reached the other way round
    assert (fs[2].hops != fs[0].hops).any() and (fs[2].hops >= 0).all() and fs[0].hops[6] == 3 and fs[2].hops[6] == 9
    # (SF, 0.05) refuses every edge: only the source is reached, on both ranks
    assert [int((g["hops"][3] >= 0).sum()) for g in got] == [1, 0] and got[0]["hops"][3][3] == 0
    assert [g["reached"].tolist() for g in got] == [[6, 6, 6, 1], [6, 6, 6, 0]]
    close(engines)


# ---- 2. the only bridge refused -----------------------------------------------------------------------------------------
def gid(p):
    return (p % 2) * 32 + p // 2


def chain_edges(pos=gid, bridge=None):
    """a 64-node chain whose nodes alternate between two tiles; every edge costs more than an ulp of any cost on it;
    bridge: the position whose edge to the next is raised to weight 0.9"""
    return [(pos(p), pos(p + 1), 0.9 if p == bridge else 0.1 * (p % 3), 0.4 + 0.05 * (p % 4)) for p in range(63)]


def test_the_only_bridge_refused(tmp_path, tiled):
    engines, _ = craft(tmp_path, [32, 32], chain_edges(bridge=30), tag="mchain")
    G = exported(tiled, engines)
    got, fs = check("chain", engines, G, [gid(0)] * 2, [(SF, 0.5), None])
    assert sorted(np.flatnonzero(fs[0].hops >= 0).tolist()) == sorted(gid(p) for p in range(31))
    assert (fs[1].hops >= 0).all()
    assert sum(int(g["reached"][0]) for g in got) == 31 and all(g["reached"][0] > 0 for g in got)
    assert sum(int(g["reached"][1]) for g in got) == 64
    close(engines)


# ---- 3. the lattice of exact ties -----------------------------------------------------------------------------------------
def most_tight_predecessors(P, f):
    """of a field at s = 0 (an edge costs its length) on its pruned graph P: the most predecessors one level up whose
    extension is a node's cost"""
    u, v = np.repeat(np.arange(len(P["state"])), np.diff(P["rowptr"])), P["col"]
    with np.errstate(invalid="ignore"):
        tight = (f.hops[u] >= 0) & (f.hops[v] == f.hops[u] + 1) & ((f.cost[u] + P["dist"]).astype(F32) == f.cost[v])
    return int(np.bincount(v[tight], minlength=1).max())


def test_lattice_of_exact_ties(tmp_path, tiled):
    sizes, edges, sources = level_lattice()
    engines, _ = craft(tmp_path, sizes, edges, tag="mlattice")
    G = exported(tiled, engines)
    # five ceilings at s = 0: costs are sums of equal lengths and tie exactly
    five = [(0.0, tau) for tau in rg.LEVELS]
    sets = [s for s in sources for _ in five]
    models = five * len(sources)
    _, fs = check("lattice 3 x 5", engines, G, sets, models)
    for (_, tau), f in zip(models, fs):  # the precondition: some node has two tight admitted predecessors or more
        assert tau < rg.LEVELS[2] or most_tight_predecessors(tmr.pruned(G, tau), f) >= 2, tau
    assert len({int((f.hops >= 0).sum()) for f in fs[:5]}) == 5  # every ceiling reaches another set of nodes
    perm = np.random.default_rng(5).permutation(len(sets))
    got, _ = check("lattice permuted", engines, G, [sets[i] for i in perm], [models[i] for i in perm])
    # m = 64: more models than the cache can keep beside the engine's own
    def many(base):
        return [(base + 0.25 * k, [0.1, 0.2, 0.3, 0.4, 0.5, np.inf][k % 6]) for k in range(64)]
    src64 = [sources[k % 3] for k in range(64)]
    first, other = many(0.0), many(100.0)
    assert len(set(first)) == 64 and len(set(other)) == 64 and not set(first) & set(other)
    check("lattice 64", engines, G, src64, first)
    check("lattice 64 others", engines, G, src64, other)
    plain = ok(run_ranks(engines, lambda r, e: e.tiled_cost_fields(sources))[0])
    assert_fields("lattice plain after 128 models", plain, G, tmr.stacked(tmr.fields(G, [None] * 3, as_sets(sources), None, SF)))
    check("lattice 64 again", engines, G, src64, first)
    close(engines)


# ---- 4. duplicates inside a tile ------------------------------------------------------------------------------------------
def test_duplicates_inside_a_tile(tmp_path, tiled):
    """the pair 1 -- 2 twice in tile 0: a short risky copy first, a long safe one after it; the pair 5 -- 6 twice in tile
    1: two copies of one length, the risky one first, which tie exactly at s = 0"""
    edges = [(p, p + 1, 0.1, 0.5) for p in range(7) if p not in (1, 5)] + [(1, 2, 0.9, 0.1), (5, 6, 0.9, 0.5)]
    extra = [(1, 2, 0.1, 0.5), (5, 6, 0.1, 0.5)]
    engines, _ = craft(tmp_path, [4, 4], edges, tag="mdup", extra=extra)
    G = exported(tiled, engines)
    models = [(SF, INF), (SF, 0.5), (0.0, INF), (0.0, 0.5)]
    _, fs = check("duplicates", engines, G, [0] * 4, models)
    assert fs[1].cost[2] > fs[0].cost[2] and fs[3].cost[2] > fs[2].cost[2]  # under the ceiling: the dearer copy
    want = tmr.stacked(fs)
    pairs = [(k, 7) for k in range(4)] + [(k, 2) for k in range(4)]
    routes = tmr.routes(G, models, want, pairs, SF)
    parts = call_routes(engines, [p[0] for p in pairs], [p[1] for p in pairs])
    assert_routes("duplicates", tiled, parts, G, routes, owners=True)
    # the edge sums are those of the admitted copies: the ceiling changes the risk sum, and at s = 0 on 5 -- 6 only it
    assert routes[0].avg_risk != routes[1].avg_risk and routes[0].path_length != routes[1].path_length
    assert routes[6].avg_risk != routes[7].avg_risk
    # (SF, inf) and (0, inf) walk the same nodes and lengths to 7; at s = 0 the two copies of 5 -- 6 tie and the first,
    # risky one is the route edge, which (SF, inf) never takes
    assert routes[0].path_length == routes[2].path_length and routes[2].avg_risk > routes[0].avg_risk
    close(engines)


# ---- 5. equalities with the plain calls -----------------------------------------------------------------------------------
def test_equalities_with_the_plain_calls(tmp_path, tiled):
    sizes, edges, sources = level_lattice()
    engines, _ = craft(tmp_path, sizes, edges, tag="msame")
    G = exported(tiled, engines)
    sets = [[sources[0], sources[1]], [sources[2]]]
    for kw in (dict(), dict(budget=[4.0, 6.0]), dict(settle="all", settle_gids=[3, sizes[0] + 2])):
        plain = ok(run_ranks(engines, lambda r, e: e.tiled_cost_fields_from_bounded(sets, **kw))[0])
        for models in (None, [(SF, INF)] * 2, [None, SF]):
            same = modelled(engines, sets, models, **kw)
            for t, (a, b) in enumerate(zip(plain, same)):
                for name in ("cost", "hops", "parent", "owner", "bound", "reached"):
                    assert np.array_equal(a[name].view(np.int32), b[name].view(np.int32)), (kw, models, t, name)
                assert [x.tolist() for x in a["owned"]] == [x.tolist() for x in b["owned"]], (kw, models, t)
                for name in ("exchanges", "owner_exchanges", "rounds", "records_sent", "owner_records_sent", "roots"):
                    assert getattr(a["info"], name) == getattr(b["info"], name), (kw, models, t, name)
                assert ("models" in b) == (models is not None)
    # m = 1 under a model: the one-slot path
    check("one field, one model", engines, G, [sources[1]], [(1.0, rg.LEVELS[2])])
    check("eight fields, one model", engines, G, [sources[k % 3] for k in range(8)], [(0.5, rg.LEVELS[3])] * 8)
    close(engines)


# ---- 6. sets, start costs, owners -----------------------------------------------------------------------------------------
def test_sets_with_start_costs_and_owners(tmp_path, tiled):
    sizes, edges, sources = level_lattice()
    engines, _ = craft(tmp_path, sizes, edges, tag="msets")
    G = exported(tiled, engines)
    off = G["offsets"]
    sets = [[sources[0], sources[1], sources[2]], [sources[2], sources[2], int(off[1]), int(off[2]) + 1]]
    starts = [np.array([0.0, 1.5, 2.0], F32), np.array([0.5, 0.25, 0.0, 1.0], F32)]
    models = [(SF, rg.LEVELS[2]), (1.0, rg.LEVELS[3])]
    targets = [np.arange(0, s, 3, dtype=np.int32) for s in sizes]
    got, fs = check("sets", engines, G, sets, models, starts, targets=targets)
    cost, hops, _, owner = tmr.stacked(fs, OWNED)
    assert all(len(set(f.owner[f.owner >= 0].tolist())) >= 2 for f in fs)  # more than one member owns something
    for t, g in enumerate(got):
        at = int(off[t]) + targets[t]
        assert np.array_equal(g["cost_at"].view(np.uint32), cost[:, at].view(np.uint32)), t
        assert np.array_equal(g["hops_at"], hops[:, at]) and np.array_equal(g["owner_at"], owner[:, at]), t
    for k in range(2):
        owned = sum(g["owned"][k] for g in got)
        assert owned.tolist() == np.bincount(owner[k][owner[k] >= 0], minlength=len(sets[k])).tolist(), (k, owned)
    close(engines)


# ---- 7. bounds --------------------------------------------------------------------------------------------------------------
def test_bounds_on_the_chain(tmp_path, tiled):
    engines, _ = craft(tmp_path, [32, 32], chain_edges(bridge=30), tag="mbchain")
    G = exported(tiled, engines)
    src = gid(0)
    models = [None, (SF, 0.5)]
    want = tmr.stacked(tmr.fields(G, models, [[src]] * 2, None, SF))
    cost = lambda k, p: want[0][k][gid(p)]  # noqa: E731
    assert want[1][1][gid(41)] == -1 and want[1][0][gid(41)] == 41  # the ceiling makes position 41 unreachable
    cases = [(np.array([cost(0, 20), cost(1, 10)], F32), None, None, [cost(0, 20), cost(1, 10)]),
             (None, "any", [gid(13), gid(41)], [cost(0, 13), cost(1, 13)]),  # {reachable, unreachable}: the reachable one's
             (None, "all", [gid(13), gid(41)], [cost(0, 41), INF]),
             (None, "any", [gid(41)], [cost(0, 41), INF]),
             (np.array([INF, cost(1, 25)], F32), "all", [gid(41), gid(7)], [cost(0, 41), cost(1, 25)])]
    for budget, mode, targets, bound in cases:
        got = modelled(engines, [src] * 2, models, budget=budget, settle=mode, settle_gids=targets)
        _, b = assert_bounded(f"chain {mode} {targets}", engines, got, G, want, budget, mode, targets or ())
        assert np.array_equal(b.view(np.uint32), np.array(bound, F32).view(np.uint32)), (mode, targets, b, bound)
    close(engines)


def test_bounds_on_the_lattice(tmp_path, tiled):
    sizes, edges, sources = level_lattice()
    engines, _ = craft(tmp_path, sizes, edges, tag="mblattice")
    G = exported(tiled, engines)
    off = G["offsets"]
    models = [(0.0, rg.LEVELS[4]), (0.0, rg.LEVELS[1]), (SF, rg.LEVELS[2])]
    src = sources[0]
    want = tmr.stacked(tmr.fields(G, models, [[src]] * 3, None, SF))
    tile_of = np.searchsorted(off, np.arange(G["V"]), side="right") - 1
    both = (want[1] >= 0).all(0) & (want[1][0] >= 3)
    there = [int(v) for v in np.flatnonzero(both & (tile_of != tile_of[src]))[:2]]
    here = [int(v) for v in np.flatnonzero(both & (tile_of == tile_of[src]))[:1]]
    assert len(there) == 2 and len(here) == 1
    budgets = np.array([np.median(want[0][k][want[1][k] >= 0]) for k in range(3)], F32)
    for budget, mode, targets in ((budgets, None, None), (None, "any", there), (None, "all", there + here),
                                  (budgets, "all", there)):
        got = modelled(engines, [src] * 3, models, budget=budget, settle=mode, settle_gids=targets)
        trunc, b = assert_bounded(f"lattice {mode} {targets}", engines, got, G, want, budget, mode, targets or ())
        assert ((trunc[1] < 0) & (want[1] >= 0)).any(1).all(), (mode, targets)  # every field is truncated
        at_bound = [int(((trunc[0][k] == b[k]) & (trunc[1][k] >= 0)).sum()) for k in range(2)]
        assert mode is None or min(at_bound) >= 1, (mode, targets, at_bound)
    close(engines)


# ---- 8. routes --------------------------------------------------------------------------------------------------------------
def test_routes_under_models(tmp_path, tiled):
    sizes, edges, sources = level_lattice()
    engines, _ = craft(tmp_path, sizes, edges, tag="mroutes")
    G = exported(tiled, engines)
    models = [None, (0.0, rg.LEVELS[2]), (SF, rg.LEVELS[3]), (1.0, rg.LEVELS[1])]
    src = sources[0]
    _, fs = check("routes: the solve", engines, G, [src] * 4, models)
    want = tmr.stacked(fs)
    pairs = [(k, v) for k in range(4) for v in range(0, G["V"], 5)]
    f, t = [p[0] for p in pairs], [p[1] for p in pairs]
    routes = tmr.routes(G, models, want, pairs, SF)
    assert most_crossings(G, routes) >= 2
    behind = [i for i, (k, v) in enumerate(pairs) if k > 0 and not len(routes[i].ids) and want[1][0][v] > 0]
    assert behind  # a target behind a ceiling: reached in the plain field, the empty route under the model
    parts = call_routes(engines, f, t)
    joined = assert_routes("routes", tiled, parts, G, routes, owners=True)
    assert all(joined[i][2].num_nodes == 0 and joined[i][2].root_gid == -1 for i in behind)
    # the routes differ between the models: the walk reads each field's own admitted edges
    assert len({tuple(routes[i].ids.tolist()) for i, (k, v) in enumerate(pairs) if v == pairs[-1][1]}) > 1
    # after a solve without parents: the late parent sweep under the models
    modelled(engines, [src] * 4, models, full=False, parent=False)
    assert_routes("routes after parent=False", tiled, call_routes(engines, f, t), G, routes, owners=True)
    # one query at three risk attitudes, and at a fourth whose ceiling cuts the goal off
    goal = sources[1]
    goal_routes = tmr.routes(G, models, want, [(k, goal) for k in range(4)], SF)
    assert all(len(r.ids) for r in goal_routes[:3]) and not len(goal_routes[3].ids)
    for early in (True, False):
        parts = ok(run_ranks(engines, lambda r, e: e.tiled_plan_tradeoff(src, goal, models, early_exit=early))[0])
        assert_routes(f"tradeoff early_exit={early}", tiled, parts, G, goal_routes, owners=True)
    close(engines)


# ---- 9. a tile without nodes --------------------------------------------------------------------------------------------------
def test_a_tile_without_nodes(tmp_path, tiled):
    ring = [(a, b, 0.5 if a == 5 else w, d) for a, b, w, d in RING]
    engines, _ = craft(tmp_path, [6, 0, 6], ring, tag="mhollow")
    G = exported(tiled, engines)
    models = [(SF, 0.2), (0.0, INF)]
    got, fs = check("hollow", engines, G, [3, 8], models)
    assert got[1]["cost"].shape == (2, 0) and got[1]["reached"].tolist() == [0, 0]
    assert fs[0].hops[6] == 9 and (fs[0].hops >= 0).all()
    want = tmr.stacked(fs)
    got = modelled(engines, [3, 8], models, settle="all", settle_gids=[6, 2])
    assert_bounded("hollow settle", engines, got, G, want, None, "all", [6, 2])
    close(engines)


# ---- 10. a built tiling -----------------------------------------------------------------------------------------------------
def test_built_tiling(oa, synth, tiled, cost_ref):
    lay, engines = sc.engines(oa, synth, tiled, "2x1")
    join_group(engines, "models-2x1")
    stitch(engines, lay)
    G = exported(tiled, engines)
    sources, _ = pick_sources(G)
    stitch(engines, lay)
    w = G["w"][G["w"] > 0]
    assert w.size
    four = [(SF, INF), (0.0, INF), (SF, 0.0), (SF, F32(np.median(w)))]
    models = [mod for mod in four for _ in sources]
    src = [s for _ in four for s in sources]
    want = tmr.compiled_fields(cost_ref, G, models, src, SF)
    n = len(sources)
    differ = (want[0][:n].view(np.uint32) != want[0][2 * n:3 * n].view(np.uint32)) | ((want[1][:n] >= 0) != (want[1][2 * n:3 * n] >= 0))
    assert differ.any()  # the precondition: the ceiling 0 changes a field at one node or more
    got = modelled(engines, src, models)
    assert_fields("2x1 models", got, G, want, COST)
    print("2x1 models: exchanges", got[0]["info"].exchanges, "rounds", [g["info"].rounds for g in got], "records",
          [g["info"].records_sent for g in got], "ms", [round(g["info"].ms_total, 2) for g in got])
    for e in engines:  # (stitch_cases keeps the engines for other modules)
        e.comm_destroy()


# ---- 11. refusals and failures ------------------------------------------------------------------------------------------------
def raw_call(e, sources, pairs):
    """the C entry itself, past the wrapper's own checks: m sets of one, no outputs"""
    from trg_planner._engine import TrgFieldModel, _i
    m = len(sources)
    arr = (TrgFieldModel * m)(*[TrgFieldModel(float(a), float(b)) for a, b in pairs])
    ptr, ids = np.arange(m + 1, dtype=np.int32), np.asarray(sources, np.int32)
    e._chk(e.L.trg_engine_tiled_cost_field_models(e.h, m, arr, _i(ptr), _i(ids), None, 0, None, 0, None, 0, None, None,
                                                  None, None, None, 0, None, None, None, None, None, None, None))
    return True


def test_refusals_leave_the_group_usable(tmp_path, tiled):
    from trg_planner._engine import TrgError
    engines, _ = craft(tmp_path, [6, 6], RING, tag="mrefuse")
    G = exported(tiled, engines)
    good = [(SF, 0.2), (0.0, INF)]
    check("before the refusals", engines, G, [0, 7], good)
    for pairs, text in (([(np.nan, 0.5), good[1]], "the safety factor of field 0 is negative or not finite"),
                        ([good[0], (-1.0, 0.5)], "the safety factor of field 1 is negative or not finite"),
                        ([good[0], (np.inf, 0.5)], "the safety factor of field 1 is negative or not finite"),
                        ([(3.0, np.nan), good[1]], "the risk ceiling of field 0 is negative or not a number"),
                        ([good[0], (3.0, -0.5)], "the risk ceiling of field 1 is negative or not a number")):
        got, secs = run_ranks(engines, lambda r, e: raw_call(e, [0, 7], pairs))
        for g in got:
            assert isinstance(g, TrgError) and g.status == INVALID_ARG and text in str(g), (pairs, g)
        assert secs < 5.0
        # the retained solve is still usable, and so is the group
        parts = call_routes(engines, [0, 1], [9, 2])
        assert [i.num_nodes for i in parts[0]["infos"]] == [4, 6]
    check("after the refusals", engines, G, [0, 7], good)
    close(engines)


def test_a_model_that_overflows_on_one_rank(tmp_path, tiled):
    from trg_planner._engine import TrgError
    # only tile 0 holds an edge of positive weight: (3e38 * 2 + 1) * dist is +inf there and nowhere else
    edges = [(p, p + 1, 2.0 if p == 0 else 0.0, 0.5) for p in range(7)]
    engines, _ = craft(tmp_path, [4, 4], edges, tag="moverflow")
    G = exported(tiled, engines)
    for bad in ((3e38, INF), (3e38, 1.0)):  # (the flag is taken over all edges, those above the ceiling included)
        got, secs = run_ranks(engines, lambda r, e: e.tiled_cost_fields_models([0, 5], [None, bad]))
        assert isinstance(got[0], TrgError) and got[0].status == INVALID_ARG, got[0]
        assert "an edge cost is negative or not finite under the model of field 1" in str(got[0]), got[0]
        assert isinstance(got[1], TrgError) and got[1].status == DEVICE and PEER in str(got[1]), got[1]
        assert secs < 10.0, secs
    check("after the overflow", engines, G, [0, 5], [None, (2.0, 1.0)])
    close(engines)


def test_a_new_safety_factor_makes_a_modelled_solve_stale(tmp_path, tiled):
    from trg_planner._engine import TrgError
    engines, _ = craft(tmp_path, [6, 6], RING, tag="mstale")
    G = exported(tiled, engines)
    models = [(1.0, 0.2), (0.0, INF)]  # every field names its own s: one rule all the same
    check("before", engines, G, [0, 7], models)
    assert call_routes(engines, [0], [9])[0]["infos"][0].num_nodes == 4
    for e in engines:
        e.set_option("safety_factor", "0.5")
    got, secs = run_ranks(engines, lambda r, e: e.tiled_routes([0], [9]))
    for g in got:
        assert isinstance(g, TrgError) and g.status == INVALID_ARG and "stale" in str(g), g
    for e in engines:
        with pytest.raises(TrgError) as ex:
            e.tiled_field_reached(0)
        assert ex.value.status == INVALID_ARG and "stale" in str(ex.value)
    for e in engines:
        e.set_option("safety_factor", str(SF))
    check("after", engines, G, [0, 7], models)
    assert call_routes(engines, [0], [9])[0]["infos"][0].num_nodes == 4
    close(engines)
