"""GPU: a cost model per field (trg_engine_cost_field_models, the `models` argument of Engine.cost_fields /
Engine.cost_fields_from_models, Engine.plan_tradeoff / min_risk_ceiling; DESIGN.md section 2, "Cost models").

Every comparison is exact -- cost as bits; hops, parents, owners, `owned`, `reached`, bounds as bits, route ids and
route floats as bits -- against tests/model_ref.py: the existing host references on the graph WITHOUT the edges above
the field's ceiling, at the field's safety factor.  Nothing expected comes from the engine.

Shapes: the smallest at which each piece can go wrong -- V ~ 30-44 with every kind of source, m = 1 (the host points
the plain kernels at the model's slot), 2 and 5 (the MODELS kernels), 64 distinct models twice over (the cache gives
slots away), one graph of 2 000 nodes, a row of 40 edges (three 16-lane trips), exact ties."""
import ctypes as C

import numpy as np
import pytest

import bound_ref
import field_graphs as fg
import model_ref
import refresh_pairs
import set_ref
from field_support import (INVALID_ARG, SCALES_LARGE, assert_rows, bits, engine, load_graph,  # noqa: F401
                           random_large, small_sources, with_isolated_node, write_graph)

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = F32(np.inf)
SF = 3.0  # the engine's (field_support.MOUNTAIN)
SFS = (0.0, 0.5, 3.0, 50.0)
TAUS = (0.0, 0.1, 0.5, 1.0, np.inf)
GRID = [(s, t) for s in SFS for t in TAUS]
# 64 distinct models: the grid and 44 more; OTHER_64 shares none with them
MODELS_64 = GRID + [(0.3 + 0.13 * k, TAUS[k % 5]) for k in range(44)]
OTHER_64 = [(7.0 + 0.5 * k, (0.05, 0.3, 0.7, np.inf)[k % 4]) for k in range(64)]
SCALES = SCALES_LARGE  # near-far, a bucket per distinct cost, Bellman-Ford


def _b1(v):
    return int(np.float32(v).view(np.uint32))


def _refs(x, models, sets):
    return [model_ref.model_field(x, mo, s, SF) for mo, s in zip(models, sets)]


def _check(e, refs, models, sets, at, budget=None, settle=None, targets=None, full=True, single=False):
    """One modelled solve against the (truncated) reference fields -> the engine's result.  single: through
    cost_fields with source_ids (every set has one member), else through cost_fields_from_models."""
    m = len(sets)
    want = refs
    bounded = budget is not None or settle is not None
    if bounded:
        bud = np.full(m, INF, F32) if budget is None else np.broadcast_to(np.asarray(budget, F32).reshape(-1), (m,))
        want_bound = np.array([min(bud[k], bound_ref.settle_bound(refs[k].cost, refs[k].hops, targets, settle))
                               for k in range(m)], F32)
        want = [set_ref.truncate(refs[k], want_bound[k]) for k in range(m)]
    if single:
        r = e.cost_fields(source_ids=[s[0] for s in sets], targets=targets, full=full, budget=budget, settle=settle,
                          models=models)
        assert r["sources"].tolist() == [s[0] for s in sets], at
    else:
        r = e.cost_fields_from_models(sets, models, targets=targets, full=full, budget=budget, settle=settle)
    if bounded:
        assert np.array_equal(bits(r["bound"]), bits(want_bound)), at + f"bound {r['bound']!r} != {want_bound!r}"
    else:
        assert "bound" not in r
    pairs = np.array([model_ref.as_model(mo, SF) for mo in models], F32)
    assert np.array_equal(bits(r["models"]), bits(pairs)), at + "models"
    stack = [np.stack([getattr(f, name) for f in want]) for name in ("cost", "hops", "parent", "owner")]
    assert np.array_equal(r["reached"], (stack[1] >= 0).sum(axis=1)), at + f"reached {r['reached']}"
    assert r["info"].reached == int(r["reached"].sum()) and r["info"].source == int(sets[0][0]), at
    if not single:
        for k in range(m):
            assert np.array_equal(r["owned"][k], want[k].owned), at + f"owned of set {k}: {r['owned'][k]}"
    if full:
        assert_rows(at, "costs", r["cost"], stack[0], as_bits=True)
        assert_rows(at, "hops", r["hops"], stack[1])
        assert_rows(at, "parents", r["parent"], stack[2])
        if not single:
            assert_rows(at, "owners", r["owner"], stack[3])
    if targets is not None:
        t = np.asarray(targets, np.int64)
        assert np.array_equal(bits(r["cost_at"]), bits(stack[0][:, t])), at + "cost_at"
        assert np.array_equal(r["hops_at"], stack[1][:, t]), at + "hops_at"
        if not single:
            assert np.array_equal(r["owner_at"], stack[3][:, t]), at + "owner_at"
    return r


def _check_routes(e, x, refs, models, sets, pairs, at):
    """Routes (field, target) of the retained solve against model_ref.model_route; no route edge above a ceiling."""
    got = e.routes([k for k, _ in pairs], [t for _, t in pairs], hops_at=[refs[k].hops[t] for k, t in pairs])
    row = np.repeat(np.arange(x.V), np.diff(x.rowptr))
    unreached = 0
    for (k, t), (ids, pts, one) in zip(pairs, got):
        f = refs[k]
        where = at + f"field {k}, target {t}: "
        if f.hops[t] < 0:
            unreached += 1
            assert one.num_nodes == 0 and ids.size == 0 and np.isposinf(one.cost), where
            continue
        w = model_ref.model_route(x, models[k], f, sets[k], t, SF)
        assert np.array_equal(ids, w.ids), where + f"ids {ids.tolist()} != {w.ids.tolist()}"
        assert ids[0] == sets[k][f.owner[t]] and ids[-1] == t and one.num_nodes == len(w.ids), where
        assert np.array_equal(bits(pts), bits(x.xyz[w.ids])), where
        for nm in ("cost", "path_length", "avg_risk"):
            assert _b1(getattr(one, nm)) == _b1(getattr(w, nm)), where + nm
        tau = model_ref.as_model(models[k], SF)[1]
        assert np.all(x.w[w.edges] <= tau) and np.array_equal(row[w.edges], ids[:-1]), where
        for u, v in zip(ids[:-1], ids[1:]):  # the engine's own ids: some admitted edge joins each step
            k0, k1 = x.rowptr[u], x.rowptr[u + 1]
            assert np.any((x.col[k0:k1] == v) & (x.w[k0:k1] <= tau)), where + f"step {u} -> {v}"
    return unreached


def _raw(e, models, sets, targets=None, settle=0, cost_at=False):
    """One trg_engine_cost_field_models call with no output over the nodes -> (status, TrgFieldInfo, cost_at)."""
    from trg_planner._engine import TrgFieldInfo, TrgFieldModel, _f, _i
    m = len(sets)
    ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(s) for s in sets])]), np.int32)
    ids = np.ascontiguousarray(np.concatenate([np.asarray(s) for s in sets]), np.int32)
    arr = None
    if models is not None:
        arr = (TrgFieldModel * len(models))(*[TrgFieldModel(float(a), float(b)) for a, b in models])
    t = None if targets is None else np.ascontiguousarray(targets, np.int32)
    nt = 0 if t is None else t.size
    at = np.empty(max(m, 1) * max(nt, 1), np.float32) if cost_at else None
    info = TrgFieldInfo()
    st = e.L.trg_engine_cost_field_models(e.h, m, arr, _i(ptr), _i(ids), None, settle, None, None, None, None,
                                          None if t is None else _i(t), nt, None if at is None else _f(at), None, None,
                                          None, None, None, C.byref(info))
    return st, info, at


def _small(seed):
    return with_isolated_node(fg.with_positions(fg.random_small(seed)))


@pytest.mark.parametrize("seed", [7, 13])
def test_random_graphs(engine, tmp_path, seed):
    """m = 1 under models that are not the engine's, m = 2 from one source, m = 5 mixed, and the same five with
    their models permuted, at every bucket width."""
    e = engine
    g = _small(seed)
    x = load_graph(e, g, tmp_path)
    V = x.V
    first = small_sources(g, 1, 0)[0]
    ones = [GRID[(3 * i + seed) % 20] for i in range(6)] + [(0.0, 0.0), (50.0, np.inf)]
    two = [(SF, np.inf), (SF, 0.1)]
    five = [GRID[(7 * i + seed) % 20] for i in range(5)]
    src5 = small_sources(g, 5, seed)
    perm = [3, 0, 4, 1, 2]
    same = [(0.0, np.inf), (50.0, 1.0), (0.5, 0.5), (SF, 0.0), None]
    ref1 = {mo: _refs(x, [mo], [[first]])[0] for mo in dict.fromkeys(ones)}
    ref2 = _refs(x, two, [[first], [first]])
    assert np.any(bits(ref2[0].cost) != bits(ref2[1].cost))  # one source, two models: two fields
    ref5 = _refs(x, five, [[s] for s in src5])
    ref_same = _refs(x, same, [[first]] * 5)
    assert len({f.cost.tobytes() + f.hops.tobytes() for f in ref_same}) == 5
    targets = [first, V - 1, V // 2, 3]
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        at = f"seed {seed}, width {scale}, "
        for mo in ref1:
            _check(e, [ref1[mo]], [mo], [[first]], at + f"one field under {mo}: ", targets=targets, single=True)
        r = _check(e, ref2, two, [[first], [first]], at + "one source, two models: ", targets=targets, single=True)
        assert np.any(bits(r["cost"][0]) != bits(r["cost"][1]))
        _check(e, ref5, five, [[s] for s in src5], at + "five mixed: ", targets=targets, single=True)
        _check(e, ref5, five, [[s] for s in src5], at + "five mixed, at the targets: ", targets=targets, full=False)
        a = _check(e, ref_same, same, [[first]] * 5, at + "five models of one source: ", single=True)
        b = _check(e, [ref_same[j] for j in perm], [same[j] for j in perm], [[first]] * 5, at + "permuted: ",
                   single=True)
        for k, j in enumerate(perm):  # the fields follow their models
            assert np.array_equal(bits(b["cost"][k]), bits(a["cost"][j])) and np.array_equal(b["hops"][k], a["hops"][j])
            assert np.array_equal(b["parent"][k], a["parent"][j])
    e.set_option("field_delta_scale", "4")


def test_64_distinct_models_and_the_cache(engine, tmp_path):
    """64 fields with 64 distinct models fill the cache beside the engine's own slot; 64 other models take those
    slots over; the first 64 again; a plain solve in between and afterwards reads slot 0, which nobody took."""
    e = engine
    g = _small(13)
    x = load_graph(e, g, tmp_path)
    assert x.V == 44 and len(set(MODELS_64)) == 64 and len(set(OTHER_64)) == 64 and not set(MODELS_64) & set(OTHER_64)
    sets = [[(5 * k + 2) % x.V] for k in range(64)]
    refs_a, refs_b = _refs(x, MODELS_64, sets), _refs(x, OTHER_64, sets)
    plain = [set_ref.set_field(x, SF, s) for s in sets[:3]]
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        at = f"width {scale}, "
        _check(e, refs_a, MODELS_64, sets, at + "64 models: ", targets=[x.V - 1, 3], single=True)
        _check(e, refs_b, OTHER_64, sets, at + "64 other models: ", targets=[x.V - 1, 3], single=True)
        r = e.cost_fields(source_ids=[s[0] for s in sets[:3]])
        assert_rows(at + "plain after 128 models: ", "costs", r["cost"], np.stack([f.cost for f in plain]),
                    as_bits=True)
        assert_rows(at + "plain after 128 models: ", "hops", r["hops"], np.stack([f.hops for f in plain]))
        _check(e, refs_a, MODELS_64, sets, at + "64 models again: ", full=False, targets=[0, 7])
    e.set_option("field_delta_scale", "4")


def test_random_large(engine, tmp_path):
    e = engine
    g = random_large(*fg.RANDOM_LARGE[2000][0])
    x = load_graph(e, g, tmp_path)
    assert x.V == 2000
    models = [(0.0, 0.5), (SF, np.inf), (50.0, 1.0), (0.5, 0.1), (SF, 0.0)]
    valid = np.flatnonzero(x.state != fg.INVALID)
    sets = [[int(valid[0])], [int(valid[-1])], [int(valid[7])], [int(valid[3])], [int(valid[0])]]
    refs = _refs(x, models, sets)
    assert all((f.hops >= 0).sum() > 1 for f in refs) and len({int((f.hops >= 0).sum()) for f in refs}) >= 3
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        _check(e, refs, models, sets, f"random_large, width {scale}: ", targets=[0, 1999, 1000], single=True)
    e.set_option("field_delta_scale", "4")


def test_duplicate_edges(engine, tmp_path):
    """0 -> 1 twice: the cheaper copy (first in the row) has the greater weight.  Under a ceiling of 0.5 the dearer
    copy is used and is the route edge; so it is with m == 1, where the plain kernels read the model's slot."""
    e = engine
    e.set_option("field_delta_scale", "4")
    nodes = [((2.0 * i, 0.0, 0.0), 0) for i in range(3)]
    edges = [(0, 1, 0.8, 1.0), (0, 1, 0.1, 5.0), (0, 1, 0.1, 5.0), (1, 2, 0.0, 1.0), (1, 2, 0.9, 0.25)]
    write_graph(tmp_path / "dup.json", nodes, edges)
    e.load_json(str(tmp_path / "dup.json"))
    x = e.graph("global")
    models = [None, (SF, 0.5), (0.0, 0.85)]
    sets = [[0]] * 3
    refs = _refs(x, models, sets)
    assert refs[0].cost[1] == F32(F32(F32(3.0) * F32(0.8)) + F32(1.0)) and refs[1].cost[1] > 6
    pairs = [(k, t) for k in range(3) for t in range(3)]
    _check(e, refs, models, sets, "duplicates: ", single=True)
    _check_routes(e, x, refs, models, sets, pairs, "duplicates: ")
    got = e.routes([0, 1, 2], [2, 2, 2])
    assert [r[2].path_length for r in got] == [1.25, 6.0, 2.0], [r[2].path_length for r in got]
    assert _b1(got[1][2].avg_risk) == _b1(F32(F32(0.1) / F32(3.0)))
    for k in range(3):  # each alone: m == 1
        _check(e, [refs[k]], [models[k]], [[0]], f"duplicates, field {k} alone: ", single=True)
        _check_routes(e, x, [refs[k]], [models[k]], [[0]], [(0, t) for t in range(3)], f"duplicates, field {k} alone: ")
        assert e.routes([0], [2])[0][2].path_length == (1.25, 6.0, 2.0)[k]


def test_target_behind_a_ceiling(engine, tmp_path):
    """A chain 0 .. 39 of unit edges of weight 0, both ways, and node 40 hanging on node 3 by an edge of weight 0.9.
    Under a ceiling of 0.5 node 40 is unreached -- hops -1, an empty route -- and settle ANY on it never stops that
    field; the field without a ceiling stops at the target's cost."""
    e = engine
    e.set_option("field_delta_scale", "4")
    a = np.arange(39)
    g = fg.from_edges(41, np.concatenate([a, a + 1, [3]]), np.concatenate([a + 1, a, [40]]),
                      np.concatenate([np.zeros(78), [0.9]]), np.ones(79))
    x = load_graph(e, g, tmp_path)
    models = [(SF, 0.5), (SF, np.inf)]
    sets = [[0], [0]]
    refs = _refs(x, models, sets)
    assert refs[0].hops[40] == -1 and refs[1].hops[40] == 4
    r = _check(e, refs, models, sets, "behind a ceiling: ", settle="any", targets=[40], single=True)
    assert r["reached"].tolist() == [40, 8] and np.isposinf(r["bound"][0]) and r["bound"][1] == refs[1].cost[40]
    assert r["hops_at"][:, 0].tolist() == [-1, 4] and np.isposinf(r["cost_at"][0, 0])
    got = e.routes([0, 1], [40, 40])
    assert got[0][0].size == 0 and got[0][2].num_nodes == 0 and got[1][0].tolist() == [0, 1, 2, 3, 40]
    _check(e, refs, models, sets, "behind a ceiling, all: ", settle="all", targets=[40, 2], single=True)


def test_zero_ceiling_and_long_rows(engine, tmp_path):
    """tau = 0 admits the zero-weight edges only; star(40): the hub's row takes three 16-lane trips, under a ceiling
    that admits two edges in three, and, with the weights turned round, every third."""
    e = engine
    g = fg.star(40)
    s, d, w, dist = refresh_pairs.edges_of(g)
    hub = (s == 0) | (d == 0)
    turned = refresh_pairs.rebuilt(g, w=np.where(hub, np.where(w == F32(0.2), F32(0.05), F32(0.06)), w))
    for name, graph, tau, admitted in (("star", g, 0.0, 26), ("star turned", turned, 0.055, 14)):
        x = load_graph(e, graph, tmp_path, name.replace(" ", "_"))
        assert x.rowptr[1] - x.rowptr[0] == 40 and int(np.sum(x.w[:40] <= F32(tau))) == admitted
        models = [(SF, tau), None, (0.0, tau), (50.0, np.inf)]
        sets = [[0], [0], [5], [0, 17]]
        refs = _refs(x, models, sets)
        assert np.any(refs[0].parent != refs[1].parent)
        for scale in SCALES:
            e.set_option("field_delta_scale", scale)
            _check(e, refs, models, sets, f"{name}, width {scale}: ", targets=[0, 40, 7])
            _check(e, [refs[0]], [models[0]], [sets[0]], f"{name}, width {scale}, alone: ")
        _check_routes(e, x, [refs[0]], [models[0]], [sets[0]], [(0, t) for t in range(x.V)], name + ": ")
    e.set_option("field_delta_scale", "4")


def test_lattice_ties_across_a_band(engine, tmp_path):
    """Every edge the same cost, so only the parent rule decides -- and a band of edges above the ceiling (the
    crossings between columns 5 and 6 in rows 0 .. 8) that the ties must go round."""
    e = engine
    g = fg.lattice(12, 12)
    s, d, w, dist = refresh_pairs.edges_of(g)
    cross = (np.minimum(s % 12, d % 12) == 5) & (np.maximum(s % 12, d % 12) == 6) & (s // 12 < 9)
    assert cross.sum() == 18
    x = load_graph(e, refresh_pairs.rebuilt(g, w=np.where(cross, F32(0.9), w)), tmp_path)
    models = [(SF, 0.5), (SF, np.inf), (0.0, 0.5), (0.0, 1.0)]
    sets = [[0], [0], [143, 11], [143, 11]]
    refs = _refs(x, models, sets)
    assert refs[0].hops[11] == 11 + 2 * 9 and refs[1].hops[11] == 11
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        _check(e, refs, models, sets, f"lattice, width {scale}: ", targets=[11, 6, 77])
    _check_routes(e, x, refs, models, sets, [(k, t) for k in range(4) for t in (11, 6, 77, 132)], "lattice: ")
    e.set_option("field_delta_scale", "4")


def test_bounds(engine, tmp_path):
    """Budgets at five cost quantiles of each field and both settle modes, three fields of mixed models."""
    e = engine
    x = load_graph(e, _small(7), tmp_path)
    valid = np.flatnonzero(x.state != fg.INVALID)
    models = [(0.5, 0.5), None, (50.0, 1.0)]
    sets = [[int(valid[0])], [int(valid[0])], [int(valid[1])]]
    refs = _refs(x, models, sets)
    reach = np.flatnonzero((refs[0].hops > 0) & np.isfinite(refs[0].cost))
    reach = reach[np.argsort(refs[0].cost[reach], kind="stable")]
    targets = [int(reach[reach.size // 2]), int(reach[reach.size // 5]), int(reach[reach.size // 2])]
    budgets = np.array([bound_ref.five_budgets(f.cost, f.hops) for f in refs], F32)  # (3, 5)
    assert len(set(budgets[:, 2].tolist())) > 1  # the fields' medians differ
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        for j in range(5):
            for settle in (None, "any", "all"):
                _check(e, refs, models, sets, f"width {scale}, quantile {j}, settle {settle}: ", budget=budgets[:, j],
                       settle=settle, targets=targets, single=True)
        for settle in ("any", "all"):
            r = _check(e, refs, models, sets, f"width {scale}, settle {settle}: ", settle=settle, targets=targets,
                       full=False)
            assert np.isfinite(r["bound"][0])
    e.set_option("field_delta_scale", "4")


def test_sets(engine, tmp_path):
    """Sets of 1, 3 and 20 members, each under its own model: owners and `owned`."""
    e = engine
    x = load_graph(e, _small(13), tmp_path)
    assert x.V == 44
    valid = np.flatnonzero(x.state != fg.INVALID)
    sets = [[int(valid[0])], [int(valid[-2]), int(valid[0]), int(valid[len(valid) // 2])],
            [(2 * i + 1) % x.V for i in range(19)] + [1]]
    models = [(0.0, 0.1), (SF, 0.5), (50.0, np.inf)]
    refs = _refs(x, models, sets)
    assert refs[2].owned[19] == 0 and refs[2].owned.sum() > 20 and np.all(refs[1].owned > 0)
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        _check(e, refs, models, sets, f"sets, width {scale}: ", targets=[0, x.V - 1, 9])
        _check(e, refs, models, sets, f"sets, width {scale}, at the targets: ", targets=[0, x.V - 1, 9], full=False)
        for k in range(3):
            _check(e, [refs[k]], [models[k]], [sets[k]], f"sets, width {scale}, set {k} alone: ")
    e.set_option("field_delta_scale", "4")


@pytest.mark.parametrize("how", ["full", "at_targets", "late"])
def test_routes(engine, tmp_path, how):
    """Routes to every node of three modelled fields: full -- parents and owners came back with the solve;
    at_targets -- no parent output, the owners asked for; late -- neither: the first routes call runs both sweeps,
    with the solve's models."""
    e = engine
    e.set_option("field_delta_scale", "4")
    x = load_graph(e, _small(13), tmp_path)
    valid = np.flatnonzero(x.state != fg.INVALID)
    sets = [[int(valid[0])], [int(valid[0]), 20, int(valid[-2])], [int(valid[0])]]
    models = [(0.0, np.inf), (SF, 0.5), (50.0, 0.1)]
    refs = _refs(x, models, sets)
    if how == "late":
        st, info, _ = _raw(e, models, sets, targets=[0], cost_at=True)
        assert st == 0 and info.reached == sum(int((f.hops >= 0).sum()) for f in refs)
    else:
        _check(e, refs, models, sets, f"routes {how}: ", targets=[0, x.V - 1], full=how == "full")
    pairs = [(k, t) for k in range(3) for t in range(x.V)]
    unreached = _check_routes(e, x, refs, models, sets, pairs, f"routes {how}: ")
    assert unreached > 3
    for k in range(3):  # the reached list of a modelled solve
        want = np.flatnonzero(refs[k].hops >= 0)
        ids, cost, hops = e.field_reached(k)
        assert np.array_equal(ids, want) and np.array_equal(bits(cost), bits(refs[k].cost[want])), k
        assert np.array_equal(hops, refs[k].hops[want]), k


def test_refresh(engine, tmp_path):
    """The random update pair (nodes deleted and added, weights changed, ids permuted) under three mixed models: the
    refresh derives the models' costs again on the updated graph and equals a fresh modelled solve there; routes and
    the reached list then answer from it."""
    e = engine
    e.set_option("field_delta_scale", "4")
    p = refresh_pairs.random_pair()
    models = [(0.0, 0.5), (50.0, 0.9), None]
    load_graph(e, p.a, tmp_path, "a")
    e.cost_fields(source_ids=p.sources, models=models)
    xb = load_graph(e, p.b, tmp_path, "b")
    srcs = refresh_pairs.new_sources(p)
    sets = [[s] for s in srcs]
    refs = _refs(xb, models, sets)
    targets = [srcs[0], 5, xb.V - 1]
    r = e.refresh_fields(new2old=p.new2old, targets=targets)
    assert r["sources"].tolist() == srcs and np.all(r["carried"] > 0)
    want = [np.stack([getattr(f, name) for f in refs]) for name in ("cost", "hops", "parent")]
    assert_rows("refresh: ", "costs", r["cost"], want[0], as_bits=True)
    assert_rows("refresh: ", "hops", r["hops"], want[1])
    assert_rows("refresh: ", "parents", r["parent"], want[2])
    assert np.array_equal(bits(r["cost_at"]), bits(want[0][:, targets]))
    assert np.array_equal(r["hops_at"], want[1][:, targets])
    assert np.array_equal(r["reached"], (want[1] >= 0).sum(axis=1))
    some = [int(t) for t in np.linspace(0, xb.V - 1, 25)]
    _check_routes(e, xb, refs, models, sets, [(k, t) for k in range(3) for t in some], "refreshed: ")
    ids, cost, hops = e.field_reached(1)
    assert np.array_equal(ids, np.flatnonzero(refs[1].hops >= 0))
    assert np.array_equal(bits(cost), bits(refs[1].cost[ids])) and np.array_equal(hops, refs[1].hops[ids])
    fresh = e.cost_fields(source_ids=srcs, models=models, targets=targets)
    for name in ("cost", "cost_at"):
        assert np.array_equal(bits(fresh[name]), bits(r[name])), name
    for name in ("hops", "parent", "hops_at", "reached"):
        assert np.array_equal(fresh[name], r[name]), name


def test_unchanged_paths(engine, tmp_path):
    """models=None and explicit (engine safety factor, +inf) models give the bits of the plain calls, and a plain
    solve right after a modelled one gives the bits of a plain solve alone."""
    e = engine
    e.set_option("field_delta_scale", "4")
    g = _small(7)
    x = load_graph(e, g, tmp_path)
    srcs = small_sources(g, 4, 7)
    sets = [[srcs[0], srcs[1]], [srcs[2]], [srcs[3], srcs[0], srcs[3]]]
    targets = [0, x.V - 1, 5]

    def same(a, b, at):
        assert set(a) - {"models"} == set(b) - {"models"}, at
        for key in a:
            if key in ("info", "models", "sets"):
                continue
            if key == "owned":
                assert all(np.array_equal(u, v) for u, v in zip(a[key], b[key])), at + key
            else:
                assert np.array_equal(bits(a[key]) if a[key].dtype == np.float32 else a[key],
                                      bits(b[key]) if b[key].dtype == np.float32 else b[key]), at + key

    alone = e.cost_fields(source_ids=srcs, targets=targets)
    alone_from = e.cost_fields_from(sets, targets=targets)
    same(e.cost_fields(source_ids=srcs, targets=targets, models=None), alone, "models=None: ")
    same(e.cost_fields(source_ids=srcs, targets=targets, models=[None] * 4), alone, "None per field: ")
    same(e.cost_fields(source_ids=srcs, targets=targets, models=[(SF, np.inf)] * 4), alone, "explicit: ")
    same(e.cost_fields(source_ids=srcs, targets=targets, models=[SF, None, (SF, np.inf), 3]), alone,
         "mixed spellings: ")
    same(e.cost_fields_from_models(sets, [(SF, np.inf), None, SF], targets=targets), alone_from, "sets, explicit: ")
    same(e.cost_fields_from_models(sets, None, targets=targets), alone_from, "sets, models=None: ")
    st, info, at = _raw(e, None, sets, targets=targets, cost_at=True)
    assert st == 0 and np.array_equal(bits(at.reshape(3, 3)), bits(alone_from["cost_at"]))
    # a modelled solve in between: slot 0 of the cache is intact
    e.cost_fields(source_ids=srcs, models=[(0.0, 0.1), (50.0, 0.5), 0.5, (SF, 0.0)])
    same(e.cost_fields(source_ids=srcs, targets=targets), alone, "plain after modelled: ")
    e.cost_fields_from_models(sets, [(0.0, 0.1), (50.0, 0.5), 0.5])
    same(e.cost_fields_from(sets, targets=targets), alone_from, "plain sets after modelled: ")
    c, h, par, _ = e.cost_field(source_id=srcs[0])
    assert np.array_equal(bits(c), bits(alone["cost"][0])) and np.array_equal(h, alone["hops"][0])
    assert np.array_equal(par, alone["parent"][0])


def _tradeoff_graph(tmp_path, e):
    """0 -> 3 over node 1 (two edges of dist 1, weight 0.9) or over node 2 (dist 1.5, weight 0); 3 -> 4 by an edge
    of weight 1 only; node 5 apart.  All edges both ways."""
    nodes = [((0.0, 0.0, 0.0), 0), ((2.0, 2.0, 0.0), 0), ((2.0, -2.0, 0.0), 0), ((4.0, 0.0, 0.0), 0),
             ((6.0, 0.0, 0.0), 0), ((0.0, 8.0, 0.0), 0)]
    edges = []
    for a, b, w, d in [(0, 1, 0.9, 1.0), (1, 3, 0.9, 1.0), (0, 2, 0.0, 1.5), (2, 3, 0.0, 1.5), (3, 4, 1.0, 1.0)]:
        edges += [(a, b, w, d), (b, a, w, d)]
    write_graph(tmp_path / "tradeoff.json", nodes, edges)
    e.load_json(str(tmp_path / "tradeoff.json"))
    return e.graph("global")


def test_plan_tradeoff(engine, tmp_path):
    e = engine
    e.set_option("field_delta_scale", "4")
    x = _tradeoff_graph(tmp_path, e)
    models = [0.0, None, (0.0, 0.5), (SF, np.inf), 0.25, (50.0, 0.0)]
    start, goal = x.xyz[0, :2] + F32(0.1), x.xyz[3, :2] - F32(0.1)
    refs = _refs(x, models, [[0]] * 6)
    want_ids = [[0, 1, 3], [0, 2, 3], [0, 2, 3], [0, 2, 3], [0, 1, 3], [0, 2, 3]]
    for early in (True, False):
        got = e.plan_tradeoff(start, goal, models, early_exit=early)
        assert len(got) == 6
        for k, rec in enumerate(got):
            at = f"tradeoff, early_exit {early}, model {k}: "
            w = model_ref.model_route(x, models[k], refs[k], [0], 3, SF)
            assert rec["reachable"] and rec["ids"].tolist() == w.ids.tolist() == want_ids[k], at
            assert rec["model"] == tuple(float(v) for v in model_ref.as_model(models[k], SF)), at
            assert np.array_equal(bits(rec["xyz"]), bits(x.xyz[w.ids])), at
            for nm in ("cost", "path_length", "avg_risk"):
                assert _b1(rec[nm]) == _b1(getattr(w, nm)), at + nm
            # ... and a solve of that model alone
            one = e.cost_fields(source_ids=[0], targets=[3], full=False, models=[models[k]])
            ids, pts, info = e.routes([0], [3], hops_at=one["hops_at"][:, 0])[0]
            assert np.array_equal(ids, rec["ids"]) and _b1(info.cost) == _b1(rec["cost"]), at
            assert _b1(info.path_length) == _b1(rec["path_length"]) and _b1(info.avg_risk) == _b1(rec["avg_risk"]), at
    # a goal behind a ceiling, and one in another component
    got = e.plan_tradeoff(start, x.xyz[4, :2], [(SF, 0.95), None])
    assert not got[0]["reachable"] and got[0]["ids"].size == 0 and np.isposinf(got[0]["cost"])
    assert got[1]["ids"].tolist() == [0, 2, 3, 4]
    assert not any(rec["reachable"] for rec in e.plan_tradeoff(start, x.xyz[5, :2], [None, 0.0]))


def test_min_risk_ceiling(engine, tmp_path):
    e = engine
    e.set_option("field_delta_scale", "4")
    x = _tradeoff_graph(tmp_path, e)
    xy = lambda v: x.xyz[v, :2] + F32(0.1)  # noqa: E731
    tau, rec = e.min_risk_ceiling(xy(0), xy(3))
    assert tau == 0.0 and rec["ids"].tolist() == [0, 2, 3] and rec["model"] == (SF, 0.0)
    tau, rec = e.min_risk_ceiling(xy(0), xy(1))  # 0 -> 2 -> 3 -> 1 is safer than 0 -> 1, but not under 0.9
    assert tau == float(F32(0.9)) and rec["ids"].tolist() == [0, 1]
    tau, rec = e.min_risk_ceiling(xy(0), xy(4))  # only under the greatest weight: no ceiling at all
    assert tau == 1.0 and rec["ids"].tolist() == [0, 2, 3, 4] and rec["reachable"]
    assert e.min_risk_ceiling(xy(0), xy(5)) is None
    tau, rec = e.min_risk_ceiling(xy(2), xy(2))
    assert tau == 0.0 and rec["ids"].tolist() == [2] and rec["cost"] == 0.0
    # the random graphs against the breadth-first reference (more than 64 distinct weights: the search narrows)
    seen = {"none": 0, "zero": 0, "some": 0}
    for seed in (7, 13):
        g = _small(seed)
        xr = load_graph(e, g, tmp_path, f"r{seed}")
        assert model_ref.distinct_weights(xr).size > 64
        start = small_sources(g, 1, 0)[0]
        pos = xr.xyz[:, :2]
        nodes = e._resolve_nodes(pos)
        for v in range(0, xr.V, 2):
            s, t = int(nodes[start]), int(nodes[v])
            want = model_ref.min_ceiling(xr, s, t)
            got = e.min_risk_ceiling(pos[start], pos[v])
            at = f"seed {seed}, {s} -> {t}: "
            if want is None:
                assert got is None, at
                seen["none"] += 1
                continue
            assert got is not None and _b1(got[0]) == _b1(want), at + f"{got[0]!r} != {want!r}"
            f = model_ref.model_field(xr, (SF, want), [s], SF)
            w = model_ref.model_route(xr, (SF, want), f, [s], t, SF)
            assert got[1]["ids"].tolist() == w.ids.tolist() and _b1(got[1]["cost"]) == _b1(w.cost), at
            seen["zero" if want == 0 else "some"] += 1
    assert all(seen.values()), seen


def test_errors(engine, tmp_path):
    import trg_planner
    e = engine
    e.set_option("field_delta_scale", "4")
    g = _small(7)
    x = load_graph(e, g, tmp_path)
    first = small_sources(g, 1, 0)[0]
    models = [(0.0, 0.5), (SF, np.inf)]
    refs = _refs(x, models, [[first]] * 2)
    _check(e, refs, models, [[first]] * 2, "before the refusals: ", single=True)
    pairs = [(k, t) for k in range(2) for t in range(x.V)]

    def refused(bad, word):
        for call in (lambda: e.cost_fields(source_ids=[first, first, first], models=[None, None, bad]),
                     lambda: e.cost_fields_from_models([[first], [0, 1], [2]], [None, 1.0, bad])):
            with pytest.raises(trg_planner.TrgError) as ei:
                call()
            msg = str(ei.value)
            assert ei.value.status == INVALID_ARG and "field 2" in msg and word in msg, msg

    for sf in (np.nan, -1.0, np.inf, -np.inf):
        refused((sf, 1.0), "safety factor")
    for tau in (np.nan, -0.5, -np.inf):
        refused((SF, tau), "ceiling")
    with pytest.raises(ValueError):
        e.cost_fields(source_ids=[first, first], models=[None])
    with pytest.raises(ValueError):
        e.cost_fields_from_models([[first]], [None, None])
    st, _, _ = _raw(e, [(1.0, 1.0)] * 65, [[0]] * 65)
    assert st == INVALID_ARG and "65 sets" in e.L.trg_engine_last_error(e.h).decode()
    # none of these touched the retained solve: its routes still answer, with its models
    _check_routes(e, x, refs, models, [[first]] * 2, pairs, "after the refusals: ")
    # a model whose costs overflow: (3e38 * w + 1) * dist is +inf for some edge; the message names the field
    with np.errstate(over="ignore"):
        assert np.isinf(np.max((F32(3e38) * x.w + F32(1.0)) * x.dist))
    with pytest.raises(trg_planner.TrgError) as ei:
        e.cost_fields(source_ids=[first, first, first], models=[None, (3e38, np.inf), (3e38, np.inf)])
    assert ei.value.status == INVALID_ARG and "field 1" in str(ei.value) and "not finite" in str(ei.value)
    # ... over ALL edges of the model, those above its ceiling too
    with pytest.raises(trg_planner.TrgError) as ei:
        e.cost_fields(source_ids=[first], models=[(3e38, 0.0)])
    assert ei.value.status == INVALID_ARG and "field 0" in str(ei.value)
    # the calls still work, the cache holds no half-made slot
    _check(e, refs, models, [[first]] * 2, "after the refusals: ", single=True)
    r = e.cost_fields(source_ids=[first])
    plain = set_ref.set_field(x, SF, [first])
    assert np.array_equal(bits(r["cost"][0]), bits(plain.cost)) and np.array_equal(r["hops"][0], plain.hops)
