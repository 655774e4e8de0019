"""GPU: cost fields from source sets with start costs (trg_engine_cost_field_seeded, Engine.cost_fields_seeded,
routes / field_reached / refresh_fields on a seeded solve; DESIGN.md section 2, "Start costs").

Every comparison is exact -- cost as bits; hops, parents, owners, `owned`, `reached` and the values at the targets
equal -- against tests/seed_ref.py, the definition in Python (pinned on the CPU against the compiled host Dijkstra,
tests/test_cost_field_seeded_cpu.py); bounded solves against set_ref.truncate() at the EXPECTED bound, which comes
from the reference alone; routes against tests/route_ref.py on the seeded field, which is the route of the augmented
graph with the virtual node stripped (it walks hops[t] parents from t and must end at the owner's node).  Graphs,
sets and start costs: tests/seed_cases.py, through load_json on an engine without a map.

Shapes: V ~ 30-44 (the smallest with members of every kind: demoted, root at a non-zero start, duplicate, Invalid,
other component), 64 sets for the MULTI kernels, and one 5 000-node chain for the depth of the owner pass."""
import ctypes as C

import numpy as np
import pytest

import bound_ref
import field_graphs as fg
import model_ref
import route_ref
import seed_cases
import seed_ref
import set_ref
from field_support import INVALID_ARG, SCALES, assert_rows, bits, engine, load_graph  # noqa: F401
from seed_cases import SF

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = F32(np.inf)


def _b1(v):
    return int(np.float32(v).view(np.uint32))


def _refs(x, sets, costs):
    return [seed_ref.seeded_field(x, SF, s, c) for s, c in zip(sets, costs)]


def _compare(r, want, sets, at, targets=None, full=True, want_bound=None):
    m = len(sets)
    if want_bound is not None:
        assert np.array_equal(bits(r["bound"]), bits(want_bound)), at + f"bound {r['bound']!r} != {want_bound!r}"
    else:
        assert "bound" not in r
    stack = [np.stack([getattr(f, name) for f in want]) for name in ("cost", "hops", "parent", "owner")]
    assert np.array_equal(r["reached"], (stack[1] >= 0).sum(axis=1)), at + f"reached {r['reached']}"
    assert r["info"].reached == int(r["reached"].sum()) and r["info"].source == int(sets[0][0]), at
    for k in range(m):
        assert np.array_equal(r["owned"][k], want[k].owned), at + f"owned of set {k}: {r['owned'][k]} != {want[k].owned}"
    if full:
        assert_rows(at, "costs", r["cost"], stack[0], as_bits=True)
        assert_rows(at, "hops", r["hops"], stack[1])
        assert_rows(at, "parents", r["parent"], stack[2])
        assert_rows(at, "owners", r["owner"], stack[3])
    if targets is not None:
        t = np.asarray(targets, np.int64)
        assert np.array_equal(bits(r["cost_at"]), bits(stack[0][:, t])), at + "cost_at"
        assert np.array_equal(r["hops_at"], stack[1][:, t]), at + "hops_at"
        assert np.array_equal(r["owner_at"], stack[3][:, t]), at + "owner_at"


def _check(e, refs, sets, costs, at, budget=None, settle=None, targets=None, full=True):
    """One seeded solve against the (truncated) reference fields -> the engine's result."""
    m = len(sets)
    want, want_bound = refs, None
    if budget is not None or settle is not None:
        bud = np.full(m, INF, F32) if budget is None else np.broadcast_to(np.asarray(budget, F32).reshape(-1), (m,))
        want_bound = np.array([min(bud[k], bound_ref.settle_bound(refs[k].cost, refs[k].hops, targets, settle))
                               for k in range(m)], F32)
        want = [set_ref.truncate(refs[k], want_bound[k]) for k in range(m)]
    r = e.cost_fields_seeded(sets, costs, targets=targets, full=full, budget=budget, settle=settle)
    _compare(r, want, sets, at, targets, full, want_bound)
    return r


def _targets(x, sets):
    return sorted({0, x.V - 1, x.V // 2, *(int(s[0]) for s in sets[:3])})


@pytest.mark.parametrize("name", ["random_0", "duplicates"])
def test_zero_start_costs_are_the_set_solve(engine, tmp_path, name):
    """(a) all-zero start costs, and None, equal cost_fields_from on every output."""
    e = engine
    g, sets, _ = seed_cases.CASES[name]()
    x = load_graph(e, g, tmp_path)
    targets = _targets(x, sets)
    base = e.cost_fields_from(sets, targets=targets)
    for how, costs in (("zeros", [np.zeros(len(s), F32) for s in sets]), ("minus zeros", [np.full(len(s), -0.0, F32)
                                                                                       for s in sets]), ("None", None)):
        r = e.cost_fields_seeded(sets, costs, targets=targets)
        for key in ("cost", "cost_at"):
            assert np.array_equal(bits(r[key]), bits(base[key])), f"{name}, {how}: {key}"
        for key in ("hops", "parent", "owner", "hops_at", "owner_at", "reached"):
            assert np.array_equal(r[key], base[key]), f"{name}, {how}: {key}"
        assert all(np.array_equal(a, b) for a, b in zip(r["owned"], base["owned"])), f"{name}, {how}: owned"
    refs = [set_ref.set_field(x, SF, s) for s in sets]
    _compare(base, refs, sets, f"{name}, the set solve: ", targets)


@pytest.mark.parametrize("name", sorted(n for n in seed_cases.CASES if n.startswith("random_")))
def test_random_start_costs(engine, tmp_path, name):
    """(b) each set alone (the m == 1 kernels) and all as one batch, at every bucket width."""
    e = engine
    g, sets, costs = seed_cases.CASES[name]()
    x = load_graph(e, g, tmp_path)
    refs = _refs(x, sets, costs)
    demoted = sum(1 for f, s in zip(refs, sets) for v in set(s) if f.hops[v] > 0)
    rooted = sum(1 for f, s, c in zip(refs, sets, costs) for j, v in enumerate(s) if f.owner[v] == j and c[j] > 0)
    assert demoted >= 1 and rooted >= 1, (demoted, rooted)
    targets = _targets(x, sets)
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        for k in range(len(sets)):
            _check(e, [refs[k]], [sets[k]], [costs[k]], f"{name}, width {scale}, set {k}: ", targets=targets)
        _check(e, refs, sets, costs, f"{name}, width {scale}, the batch: ", targets=targets)
        _check(e, refs, sets, costs, f"{name}, width {scale}, at the targets: ", targets=targets, full=False)
    e.set_option("field_delta_scale", "4")


@pytest.mark.parametrize("name", ["duplicates", "exact_tie", "absorption", "saturating"])
def test_named_cases(engine, tmp_path, name):
    """(c) duplicates with different and with equal start costs and an Invalid member, (d) the exact tie on a chain,
    (e) start costs that absorb the edges, and saturating_chain() entered at a start cost."""
    e = engine
    g, sets, costs = seed_cases.CASES[name]()
    x = load_graph(e, g, tmp_path)
    refs = _refs(x, sets, costs)
    f = refs[0]
    if name == "duplicates":
        a, b, inv = sets[0][0], sets[0][1], sets[0][4]
        assert f.owner[a] == 2 and f.owner[b] == 1 and f.owner[inv] == 4 and x.state[inv] == fg.INVALID
    if name == "exact_tie":
        assert f.hops[1] == 0 and f.owner[1] == 1 and f.parent[1] == -1 and f.hops[5] == 4
    if name == "absorption":
        assert np.all(f.cost == F32(2.0 ** 25)) and f.hops[9] == 0 and f.hops[31] > 0
    if name == "saturating":
        assert np.isposinf(f.cost[2]) and f.hops[2] == 2 and np.isfinite(f.cost[1]) and f.hops[4] == 0
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        for k in range(len(sets)):
            _check(e, [refs[k]], [sets[k]], [costs[k]], f"{name}, width {scale}, set {k}: ", targets=_targets(x, sets))
    e.set_option("field_delta_scale", "4")


def test_batch_of_64(engine, tmp_path):
    """(f) 64 different sets through the MULTI kernels."""
    e = engine
    g, sets, costs = seed_cases.batch_64()
    x = load_graph(e, g, tmp_path)
    assert len(sets) == 64 and len({tuple(s) for s in sets}) == 64
    refs = _refs(x, sets, costs)
    for scale in ("4", "1e-6", "inf"):
        e.set_option("field_delta_scale", scale)
        _check(e, refs, sets, costs, f"64 sets, width {scale}: ", targets=_targets(x, sets))
    e.set_option("field_delta_scale", "4")


def test_bounded(engine, tmp_path):
    """(g) a budget below some start costs; settle ANY and ALL; budget and settle together."""
    e = engine
    g, sets, costs = seed_cases.CASES["random_1"]()
    x = load_graph(e, g, tmp_path)
    refs = _refs(x, sets, costs)
    m = len(sets)
    budget = np.array([np.sort(c)[len(c) // 2] for c in costs], F32)  # the median start cost of each set
    above = [int(np.sum(seed_ref.start_costs(c) > b)) for c, b in zip(costs, budget)]
    cut = [int(np.sum((f.hops >= 0) & (f.cost > b))) for f, b in zip(refs, budget)]
    assert min(above) >= 1 and sum(cut) >= 3, (above, cut)
    reach = [np.flatnonzero(f.hops > 0) for f in refs]
    common = sorted(set.intersection(*(set(r.tolist()) for r in reach)))
    assert len(common) >= 3
    targets = [common[0], common[len(common) // 2], common[-1]]
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        at = f"bounded, width {scale}: "
        _check(e, refs, sets, costs, at + "budget ", budget=budget, targets=targets)
        _check(e, refs, sets, costs, at + "zero budget ", budget=0.0, targets=targets)
        for settle in ("any", "all"):
            r = _check(e, refs, sets, costs, at + f"settle {settle} ", settle=settle, targets=targets)
            assert np.all(np.isfinite(r["bound"]))
            _check(e, refs, sets, costs, at + f"budget and settle {settle} ", budget=budget, settle=settle,
                   targets=targets, full=False)
            for k in range(m):
                _check(e, [refs[k]], [sets[k]], [costs[k]], at + f"settle {settle}, set {k} ", settle=settle,
                       targets=targets)
    e.set_option("field_delta_scale", "4")


def test_two_models(engine, tmp_path):
    """(h) two cost models in one seeded solve: each field is the seeded field of its model's pruned graph."""
    e = engine
    g, sets, costs = seed_cases.CASES["random_2"]()
    x = load_graph(e, g, tmp_path)
    sets, costs = sets[:2], costs[:2]
    tau = F32(np.median(x.w[x.w > 0]))
    models = [(1.0, np.inf), (5.0, float(tau))]
    refs = [seed_ref.seeded_field(model_ref.prune(x, mo[1]), mo[0], s, c) for mo, s, c in zip(models, sets, costs)]
    plain = _refs(x, sets, costs)
    assert any(not np.array_equal(bits(a.cost), bits(b.cost)) for a, b in zip(refs, plain))
    targets = _targets(x, sets)
    r = e.cost_fields_seeded(sets, costs, targets=targets, models=models)
    _compare(r, refs, sets, "two models: ", targets)
    assert np.array_equal(r["models"], np.array(models, F32))


def _route_check(e, x, sets, refs, pairs, at):
    costs = route_ref.edge_costs(x.col, x.w, x.dist, x.state, SF)
    got = e.routes([k for k, _ in pairs], [t for _, t in pairs], hops_at=[max(refs[k].hops[t], 0) for k, t in pairs])
    for (k, t), (ids, pts, one) in zip(pairs, got):
        f = refs[k]
        if f.hops[t] < 0:
            assert one.num_nodes == 0 and ids.size == 0 and np.isposinf(one.cost), at
            continue
        src = sets[k][f.owner[t]]
        w = route_ref.route(x.rowptr, x.col, x.w, x.dist, x.state, SF, f.cost, f.hops, f.parent, src, t, costs)
        assert np.array_equal(ids, w.ids), at + f"ids {ids.tolist()} != {w.ids.tolist()}"
        assert ids[0] == src and ids[-1] == t and one.num_nodes == len(w.ids) == f.hops[t] + 1, at
        assert np.array_equal(bits(pts), bits(x.xyz[w.ids])), at
        for nm in ("cost", "path_length", "avg_risk"):
            assert _b1(getattr(one, nm)) == _b1(getattr(w, nm)), at + f"{nm} of the route to {t}"


@pytest.mark.parametrize("how", ["full", "late"])
def test_routes_and_after_the_solve(engine, tmp_path, how):
    """(i) routes to every node -- roots, demoted members, nodes behind them -- and (j) field_reached, the refusal of
    refresh_fields with its message, and routes answering afterwards.  late: no parent or owner came back with the
    solve, the first routes call runs both sweeps."""
    e = engine
    e.set_option("field_delta_scale", "4")
    g, sets, costs = seed_cases.CASES["random_0"]()
    x = load_graph(e, g, tmp_path)
    refs = _refs(x, sets, costs)
    demoted = [(k, v) for k, (f, s) in enumerate(zip(refs, sets)) for v in set(s) if f.hops[v] > 0]
    through = [(k, t) for k, v in demoted for t in range(x.V) if refs[k].parent[t] == v]
    roots = [(k, int(v)) for k, f in enumerate(refs) for v in seed_ref.roots(f) if f.cost[v] > 0]
    assert demoted and through and roots, (demoted, through, roots)
    r = e.cost_fields_seeded(sets, costs, targets=[0], full=how == "full")
    pairs = [(k, t) for k in range(len(sets)) for t in range(x.V)]
    assert set(demoted + through + roots) <= set(pairs)
    _route_check(e, x, sets, refs, pairs, f"routes {how}: ")
    for k in range(len(sets)):
        want = np.flatnonzero(refs[k].hops >= 0)
        ids, cost, hops = e.field_reached(k)
        assert np.array_equal(ids, want) and np.array_equal(bits(cost), bits(refs[k].cost[want])), k
        assert np.array_equal(hops, refs[k].hops[want]), k
    from trg_planner import TrgError
    with pytest.raises(TrgError) as err:
        e.refresh_fields()
    assert err.value.status == INVALID_ARG and "start costs" in str(err.value), str(err.value)
    _route_check(e, x, sets, refs, roots + demoted + through[:4], f"routes {how}, after the refused refresh: ")
    assert r["info"].reached == sum(int((f.hops >= 0).sum()) for f in refs)


def test_refusals(engine, tmp_path):
    """(k) NaN, negative and infinite start costs, each naming set and entry; -0 is not negative."""
    e = engine
    g, sets, costs = seed_cases.CASES["random_0"]()
    load_graph(e, g, tmp_path)
    from trg_planner import TrgError
    good = e.cost_fields_seeded(sets, costs, full=False)
    for bad in (np.nan, -1e-30, np.inf, -np.inf):
        c = [a.copy() for a in costs]
        c[1][2] = bad
        with pytest.raises(TrgError) as err:
            e.cost_fields_seeded(sets, c, full=False)
        msg = str(err.value)
        assert err.value.status == INVALID_ARG and "entry 2 of set 1" in msg and "start cost" in msg, msg
    # a refusal leaves the retained solve answering
    ids, _, _ = e.field_reached(0)
    assert ids.size == good["reached"][0]
    c = [a.copy() for a in costs]
    c[1][2] = -0.0
    e.cost_fields_seeded(sets, c, full=False)


def test_two_handicapped_ends(engine, tmp_path):
    """(l) a 5 000-node chain entered at both ends, each with a handicap: thousands of hops under each owner."""
    e = engine
    e.set_option("field_delta_scale", "4")
    g, sets, costs = seed_cases.two_ends()
    x = load_graph(e, g, tmp_path)
    refs = _refs(x, sets, costs)
    assert refs[0].owned.min() > 1000 and refs[0].hops.max() > 1000
    r = _check(e, refs, sets, costs, "two ends: ", targets=[0, 2500, 4999])
    print(f"chain(5000), two handicapped ends: {r['info'].rounds} rounds, {r['info'].host_syncs} host waits")
    meet = int(np.flatnonzero(refs[0].owner == 1)[0])
    _route_check(e, x, sets, refs, [(0, meet - 1), (0, meet), (0, 0), (0, 4999)], "two ends, routes: ")
