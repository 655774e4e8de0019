"""GPU: bounded cost fields (trg_engine_cost_field_bounded, trg_engine_field_reached, Engine.cost_fields with budget
and settle, field_reached, reachable and the early_exit helpers; DESIGN.md section 2, "Bounded fields").

Every comparison is exact -- cost as bits, hops and parents equal -- against tests/bound_ref.py's truncate() of the
host Dijkstra's full field (tests/cpp/field_reference.cpp) at the EXPECTED bound, which is computed from that
reference (budgets, settle_bound of the reference's rows), never from the engine; the bound the engine returns is
compared with it as bits.  Graphs come from tests/field_graphs.py through load_json on an engine without a map.

Round counts are asserted on the unit chain only, where they are a function of the graph (one walk per node, every
node pushed once with its final key; tests/test_gpu_cost_field_batch.py, "Rounds of one batch"); measured there on
an MI355X: 82 rounds under the budget, 85 with settle "any" on the same node, 8192 unbounded."""
import ctypes as C

import numpy as np
import pytest

import bound_ref
import field_graphs as fg
import route_ref
from field_support import (INVALID_ARG, MOUNTAIN, PARAMS, SCALES, assert_rows, bits, engine, load_graph,  # noqa: F401
                           random_large, ref, reference_fields)

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = F32(np.inf)
FLT_MAX = np.finfo(np.float32).max
SF = 3.0
def _b1(v):
    """The bits of one float32."""
    return int(np.float32(v).view(np.uint32))


def _below(c):
    """The float just below the cost c (0 stays 0: no budget is negative)."""
    return F32(np.nextafter(F32(c), F32(-np.inf))) if c > 0 else F32(0.0)


def _check(e, full, sources, at, budget=None, settle=None, targets=None, want_full=True):
    """One bounded batch against truncate(full reference fields, expected bounds) -> the engine's result."""
    rc, rh, rp = full
    m = len(sources)
    bud = np.full(m, INF, F32) if budget is None else np.broadcast_to(np.asarray(budget, F32).reshape(-1), (m,))
    want_bound = np.array([min(bud[k], bound_ref.settle_bound(rc[k], rh[k], targets, settle)) for k in range(m)], F32)
    tc, th, tp = bound_ref.truncate(rc, rh, rp, want_bound)
    r = e.cost_fields(source_ids=[int(s) for s in sources], targets=targets, budget=budget, settle=settle,
                      full=want_full)
    assert np.array_equal(bits(r["bound"]), bits(want_bound)), at + f"bound {r['bound']!r} != {want_bound!r}"
    assert np.array_equal(r["reached"], (th >= 0).sum(axis=1)), at + f"reached {r['reached']}"
    assert r["info"].reached == int(r["reached"].sum()), at
    if want_full:
        assert_rows(at, "costs", r["cost"], tc, as_bits=True)
        assert_rows(at, "hops", r["hops"], th)
        assert_rows(at, "parents", r["parent"], tp)
        assert np.array_equal(r["reached"], (r["hops"] >= 0).sum(axis=1)), at
    if targets is not None:
        t = np.asarray(targets, np.int64)
        assert np.array_equal(bits(r["cost_at"]), bits(tc[:, t])), at + "cost_at"
        assert np.array_equal(r["hops_at"], th[:, t]), at + "hops_at"
    return r


def _five_sources(x):
    """Five sources: valid nodes spread over the ids (the first among them), and so over both components."""
    valid = np.flatnonzero(x.state != fg.INVALID)
    return [int(valid[i]) for i in (0, len(valid) // 4, len(valid) // 2, (3 * len(valid)) // 4, len(valid) - 1)]


def _a_cost(rc, rh):
    """A node's exact cost: the median over the reached nodes (on the chain: a cost that many nodes share)."""
    c = np.sort(rc[rh >= 0])
    return F32(c[c.size // 2])


BUDGET_GRAPHS = {
    "random_small_7": lambda: fg.with_positions(fg.random_small(7)),
    "random_small_13": lambda: fg.with_positions(fg.random_small(13)),
    "saturating_branch": fg.saturating_branch,
    "lattice_20x20_zero_band": lambda: fg.lattice(20, 20, zero_band=True),
    "chain_3000": lambda: fg.chain(3000),
}


@pytest.mark.parametrize("name", sorted(BUDGET_GRAPHS))
def test_budgets(ref, engine, tmp_path, name):
    """m = 1 and m = 5 at all five bucket widths; budgets 0, a node's exact cost (kept), the float just below it
    (dropped), a finite budget above every finite cost (on the saturating graph the +inf nodes go) and +inf (equal
    to the unbounded call); one batch of five different budgets, +inf among them, next to one budget for all."""
    e = engine
    x = load_graph(e, BUDGET_GRAPHS[name](), tmp_path)
    sources = _five_sources(x) if name != "chain_3000" else [0, 1, 700, 1500, 2990]
    full5 = reference_fields(ref, x, SF, sources)
    full1 = tuple(a[:1] for a in full5)
    rc, rh, _ = full5
    exact = [_a_cost(rc[k], rh[k]) for k in range(5)]
    assert np.sum(rc[0] == exact[0]) >= 1
    if name == "chain_3000":  # many nodes share the cost at the boundary
        assert np.sum(rc[0] == exact[0]) > 1, "the chain's median cost is no longer shared"
    if name == "saturating_branch":
        assert np.any(np.isposinf(rc[0]) & (rh[0] >= 0)), "no node is reached at +inf"
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        for budget in (F32(0.0), exact[0], _below(exact[0]), FLT_MAX, INF):
            at = f"{name}, width {scale}, m 1, budget {budget!r}: "
            r = _check(e, full1, sources[:1], at, budget=budget, targets=sources)
            if np.isposinf(budget):
                u = e.cost_fields(source_ids=sources[:1])
                assert "bound" not in u
                for key in ("cost", "hops", "parent", "reached"):
                    assert np.array_equal(r[key].view(np.int32), u[key].view(np.int32)), at + key
        mixed = np.array([0.0, exact[1], _below(exact[2]), FLT_MAX, np.inf], F32)
        r = _check(e, full5, sources, f"{name}, width {scale}, m 5, budgets {mixed!r}: ", budget=mixed, targets=sources)
        print(f"{name}, width {scale}: mixed batch reached {r['reached'].tolist()} in {r['info'].rounds} rounds")
        _check(e, full5, sources, f"{name}, width {scale}, m 5, one budget: ", budget=float(exact[0]), targets=sources)
        r = _check(e, full5, sources, f"{name}, width {scale}, m 5, budget +inf: ", budget=INF)
        u = e.cost_fields(source_ids=sources)
        for key in ("cost", "hops", "parent", "reached"):
            assert np.array_equal(r[key].view(np.int32), u[key].view(np.int32)), f"{name}, {scale}, m 5: " + key
    e.set_option("field_delta_scale", "4")


def _settle_lists(x, rc0, rh0, src):
    """Target lists by kind, from the reference's field of the first source."""
    reach = np.flatnonzero((rh0 > 0) & np.isfinite(rc0) & (rc0 > 0))
    reach = reach[np.argsort(rc0[reach], kind="stable")]  # a, b, c: the cheapest, a middle one, the dearest
    unreachable = np.flatnonzero((rh0 < 0) & (x.state != fg.INVALID))
    invalid = np.flatnonzero(x.state == fg.INVALID)
    invalid = invalid[invalid != src]
    assert reach.size >= 3 and unreachable.size and invalid.size
    a, b, c = (int(reach[i]) for i in (0, reach.size // 2, reach.size - 1))
    u, i = int(unreachable[0]), int(invalid[0])
    return {"duplicates": [a, b, a, c, c], "the source": [src], "with unreachable and Invalid": [b, u, i, a],
            "none reachable": [u, i, u]}


@pytest.mark.parametrize("mode", ["any", "all"])
def test_settle(ref, engine, tmp_path, mode):
    e = engine
    x = load_graph(e, fg.with_positions(fg.random_small(7)), tmp_path)
    valid = np.flatnonzero(x.state != fg.INVALID)
    src = int(valid[0])
    sources = [src, int(valid[1]), int(valid[-1])]  # (the last one: the other component)
    full = reference_fields(ref, x, SF, sources)
    rc, rh, _ = full
    lists = _settle_lists(x, rc[0], rh[0], src)
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        for kind, targets in lists.items():
            for m in (1, 3):
                at = f"settle {mode}, width {scale}, targets {kind} {targets}, m {m}: "
                part = tuple(a[:m] for a in full)
                r = _check(e, part, sources[:m], at, settle=mode, targets=targets)
                want0 = bound_ref.settle_bound(rc[0], rh[0], targets, mode)
                if kind == "the source":
                    assert r["bound"][0] == 0 and r["reached"][0] == int(np.sum((rh[0] >= 0) & (rc[0] == 0))), at
                if kind == "none reachable" or (kind == "with unreachable and Invalid" and mode == "all"):
                    assert np.isposinf(r["bound"][0]) and r["reached"][0] == int(np.sum(rh[0] >= 0)), at  # full field
                if kind == "with unreachable and Invalid" and mode == "any":
                    assert np.isfinite(want0) and r["bound"][0] == want0, at
        # a budget below the settle value wins; one above it does not
        targets = lists["duplicates"]
        want0 = bound_ref.settle_bound(rc[0], rh[0], targets, mode)
        assert np.isfinite(want0) and want0 > 0
        for budget in (_below(want0), F32(0.0), FLT_MAX):
            r = _check(e, tuple(a[:1] for a in full), sources[:1], f"settle {mode}, width {scale}, budget {budget!r}: ",
                       budget=budget, settle=mode, targets=targets)
            assert r["bound"][0] == min(budget, want0)
        _check(e, full, sources, f"settle {mode}, width {scale}, budgets per field: ",
               budget=[_below(want0), np.inf, 0.0], settle=mode, targets=targets)
    e.set_option("field_delta_scale", "4")


@pytest.mark.parametrize("mode", ["any", "all"])
def test_settle_batch_of_eight(ref, engine, tmp_path, mode):
    """Eight fields over one target list on the 1 950-node random graph: the fields settle buckets apart, so the
    shared threshold carries finished fields next to running ones."""
    e = engine
    x = load_graph(e, random_large(*fg.RANDOM_LARGE[2000][2]), tmp_path)
    assert x.V == 1950
    valid = np.flatnonzero(x.state != fg.INVALID)
    sources = [int(valid[(i * len(valid)) // 8]) for i in range(8)]
    full = reference_fields(ref, x, SF, sources)
    rc, rh, _ = full
    both = np.flatnonzero((rh[0] > 0) & np.isfinite(rc[0]))
    order = both[np.argsort(rc[0][both], kind="stable")]
    targets = [int(order[i]) for i in (order.size // 50, order.size // 10, order.size // 3, order.size // 10)]
    for scale in ("4", "0.5", "1e-6"):
        e.set_option("field_delta_scale", scale)
        r = _check(e, full, sources, f"eight fields, settle {mode}, width {scale}: ", settle=mode, targets=targets)
        print(f"settle {mode}, width {scale}: bounds {r['bound'].tolist()}, reached {r['reached'].tolist()}, "
              f"{r['info'].rounds} rounds")
    e.set_option("field_delta_scale", "4")
    assert np.any(np.isfinite(r["bound"])) and np.any(r["reached"] < (rh >= 0).sum(axis=1))


def test_it_really_stops(ref, engine, tmp_path):
    """A unit chain of 4096 nodes at the default width: every cost an exact integer, every node pushed once."""
    e = engine
    e.set_option("field_delta_scale", "4")
    a = np.arange(4095)
    x = load_graph(e, fg.from_edges(4096, a, a + 1, np.zeros(4095), np.ones(4095)), tmp_path)
    full = reference_fields(ref, x, SF, [0])
    rc, rh, _ = full
    assert np.array_equal(rc[0], np.arange(4096, dtype=F32)) and np.array_equal(rh[0], np.arange(4096))
    by_budget = _check(e, full, [0], "unit chain, budget: ", budget=rc[0][40])
    by_settle = _check(e, full, [0], "unit chain, settle any: ", settle="any", targets=[40])
    unbounded = e.cost_fields(source_ids=[0])
    n = (by_budget["info"].rounds, by_settle["info"].rounds, unbounded["info"].rounds)
    print(f"unit chain: {n[0]} rounds under the budget, {n[1]} with settle any, {n[2]} unbounded; host waits "
          f"{by_budget['info'].host_syncs}, {by_settle['info'].host_syncs}, {unbounded['info'].host_syncs}")
    assert by_budget["reached"][0] == 41 and by_settle["reached"][0] == 41
    # each counted round expands at least one queued item, and each pass queues exactly the reached nodes
    assert n[0] <= 2 * 41, n
    # the overshoot before detection: at most the rest of one bucket, four unit edges
    assert n[1] <= 2 * 41 + 4, n
    assert n[2] >= 2 * 4095, n


def _raw_reached(e, field, cap, ids=True, cost=True, hops=True):
    """One trg_engine_field_reached call -> (n_out, ids, cost, hops, TrgFieldInfo); the arrays keep -7 / nan where
    nothing was written."""
    from trg_planner._engine import TrgFieldInfo, _f, _i
    n = C.c_int32(-7)
    a = np.full(max(cap, 1), -7, np.int32) if ids else None
    c = np.full(max(cap, 1), np.nan, np.float32) if cost else None
    h = np.full(max(cap, 1), -7, np.int32) if hops else None
    info = TrgFieldInfo()
    e._chk(e.L.trg_engine_field_reached(e.h, field, None if a is None else _i(a), None if c is None else _f(c),
                                        None if h is None else _i(h), cap, C.byref(n), C.byref(info)))
    return n.value, a, c, h, info


def test_reached_list(ref, engine, tmp_path):
    import trg_planner
    e = engine
    e.set_option("field_delta_scale", "4")
    g = random_large(*fg.RANDOM_LARGE[2000][2])
    x = load_graph(e, g, tmp_path)
    assert x.V % 64 != 0
    valid = np.flatnonzero(x.state != fg.INVALID)
    sources = [int(valid[0]), int(valid[len(valid) // 3]), int(valid[-1])]
    full = reference_fields(ref, x, SF, sources)
    rc, rh, _ = full
    budgets = [_a_cost(rc[0], rh[0]), INF, F32(0.0)]
    r = _check(e, full, sources, "reached list: ", budget=budgets)
    for k in range(3):
        want = np.flatnonzero(r["hops"][k] >= 0)
        ids, cost, hops = e.field_reached(k)
        assert ids.dtype == np.int32 and np.array_equal(ids, want), f"field {k}: ids"
        assert np.array_equal(bits(cost), bits(r["cost"][k][want])) and np.array_equal(hops, r["hops"][k][want]), k
        assert e.field_reached(k, cap=0) == want.size  # the count only
        n, a, c, h, info = _raw_reached(e, k, 0, ids=False, cost=False, hops=False)
        assert n == want.size and info.reached == want.size and info.source == sources[k] and info.host_syncs == 1
    # a smaller cap: a prefix is written, nothing past it, and the full count comes back
    want = np.flatnonzero(r["hops"][0] >= 0)
    assert want.size > 300
    for cap in (1, 257, want.size - 1, want.size, want.size + 5):
        n, a, c, h, _ = _raw_reached(e, 0, cap)
        k = min(cap, want.size)
        assert n == want.size, cap
        assert np.array_equal(a[:k], want[:k]) and np.all(a[k:] == -7), cap
        assert np.array_equal(bits(c[:k]), bits(r["cost"][0][want[:k]])) and np.all(np.isnan(c[k:])), cap
        assert np.array_equal(h[:k], r["hops"][0][want[:k]]) and np.all(h[k:] == -7), cap
    n, a, c, h, _ = _raw_reached(e, 1, 64, cost=False)  # one array missing
    want1 = np.flatnonzero(r["hops"][1] >= 0)
    assert n == want1.size and np.array_equal(a[:64], want1[:64]) and np.array_equal(h[:64], r["hops"][1][want1[:64]])
    # reachable: one bounded solve, then the list
    ids, cost, hops = e.reachable(None, budgets[0], source_id=sources[0])
    assert np.array_equal(ids, want) and np.array_equal(bits(cost), bits(r["cost"][0][want]))
    assert np.array_equal(hops, r["hops"][0][want])

    def refused(field, cap=4):
        with pytest.raises(trg_planner.TrgError) as ei:
            _raw_reached(e, field, cap)
        assert ei.value.status == INVALID_ARG, str(ei.value)
        return str(ei.value)

    assert "field 1" in refused(1)  # (reachable's solve has one field)
    assert "field -1" in refused(-1)
    refused(0, cap=-1)
    load_graph(e, g, tmp_path, "again")
    assert "earlier graph" in refused(0)
    fresh = trg_planner.Engine(safety_factor=SF, **PARAMS)
    load_graph(fresh, fg.with_positions(fg.random_small(1)), tmp_path, "fresh")
    with pytest.raises(trg_planner.TrgError) as ei:
        fresh.field_reached(0)
    assert ei.value.status == INVALID_ARG and "no cost-field solve" in str(ei.value)
    fresh.close()


@pytest.mark.parametrize("with_parents", [True, False], ids=["parents", "late_sweep"])
def test_routes_of_a_bounded_solve(ref, engine, tmp_path, with_parents):
    """Routes to every node, inside and outside the bounds, against tests/route_ref.py on the truncated arrays."""
    e = engine
    e.set_option("field_delta_scale", "4")
    x = load_graph(e, fg.with_positions(fg.random_small(13)), tmp_path)
    valid = np.flatnonzero(x.state != fg.INVALID)
    sources = [int(valid[0]), int(valid[1]), int(valid[-1])]
    full = reference_fields(ref, x, SF, sources)
    rc, rh, _ = full
    budgets = np.array([_a_cost(rc[0], rh[0]), _below(_a_cost(rc[1], rh[1])), np.inf], F32)
    _check(e, full, sources, "routes: ", budget=budgets, want_full=with_parents)
    tc, th, tp = bound_ref.truncate(*full, budgets)
    inside, outside = int(np.sum(th[:2] >= 0)), int(np.sum((rh[:2] >= 0) & (th[:2] < 0)))
    assert inside > 2 and outside > 0, (inside, outside)
    fields_ref = [(sources[k], tc[k], th[k], tp[k]) for k in range(3)]
    pairs = [(k, t) for k in range(3) for t in range(x.V)]
    want = route_ref.routes_of_graph(x, SF, fields_ref, pairs)
    got = e.routes([f for f, _ in pairs], [t for _, t in pairs])
    for (f, t), (ids, pts, one), w in zip(pairs, got, want):
        at = f"field {f}, target {t}: "
        assert np.array_equal(ids, w.ids), at + f"ids {ids.tolist()} != {w.ids.tolist()}"
        assert pts.shape == (len(w.ids), 3) and np.array_equal(bits(pts), bits(x.xyz[w.ids])), at
        assert one.num_nodes == len(w.ids), at
        for nm in ("cost", "path_length", "avg_risk"):
            assert _b1(getattr(one, nm)) == _b1(getattr(w, nm)), at + nm
        if th[f][t] < 0:
            assert one.num_nodes == 0 and ids.size == 0, at


def _same_frontiers(e, poses):
    """cheapest_frontiers / cheapest_frontier with early_exit against without -> how many poses got a node."""
    off = e.cheapest_frontiers(poses)
    on = e.cheapest_frontiers(poses, early_exit=True)
    assert len(on) == len(off) == len(poses)
    for k, (a, b) in enumerate(zip(on, off)):
        assert (a is None) == (b is None), k
        if a is not None:
            assert a[0] == b[0] and _b1(a[1]) == _b1(b[1]) and a[2] == b[2], (k, a, b)
        one = e.cheapest_frontier(poses[k], early_exit=True)
        assert (one is None) == (b is None) and (one is None or (one[0], _b1(one[1]), one[2]) == (b[0], _b1(b[1]), b[2]))
    return sum(p is not None for p in off)


def test_frontiers_early_exit_json_graph(engine, tmp_path):
    """Frontier nodes for certain (the random family marks an eighth of its nodes Frontier), at the 1 950-node size
    and the small one, whose second component has poses without a reachable Frontier node or with few."""
    engine.set_option("field_delta_scale", "4")
    g = random_large(*fg.RANDOM_LARGE[2000][2])
    x = load_graph(engine, g, tmp_path)
    assert _same_frontiers(engine, g.pos[[0, 5, x.V // 3, x.V // 2, x.V - 1], :2].copy()) >= 2
    g = fg.with_positions(fg.random_small(3))
    x = load_graph(engine, g, tmp_path, "small")
    assert _same_frontiers(engine, g.pos[[0, 1, x.V - 1, x.V // 2, 0], :2].copy()) >= 1


def test_helpers_early_exit(mountain_small):
    """On a device-built terrain: the early_exit helpers return what they return without it."""
    import trg_planner
    e = trg_planner.Engine(**MOUNTAIN)
    e.set_sampler(7, 16)
    e.set_global_map(mountain_small)
    e.init_graph([15.0, 15.0, 0.0])
    g = e.graph("global")
    poses = np.array([(15.0, 15.0), (8.3, 21.7), (21.0, 9.5)], np.float32)
    _same_frontiers(e, poses)  # (this terrain has no Frontier node: None for every pose, either way)
    goals = g.xyz[[g.V // 7, g.V // 3, g.V // 2, g.V - 1], :2]
    off = e.plan_many(poses[0], goals)
    on = e.plan_many(poses[0], goals, early_exit=True)
    assert len(on) == 4 and any(len(p) for p, _ in off)
    for (pa, ia), (pb, ib) in zip(on, off):
        assert np.array_equal(bits(pa), bits(pb))
        assert (ia.num_nodes, _b1(ia.cost), _b1(ia.path_length), _b1(ia.avg_risk)) == \
               (ib.num_nodes, _b1(ib.cost), _b1(ib.path_length), _b1(ib.avg_risk))
    nodes = [g.V // 9, g.V // 5, g.V // 3, g.V // 2, g.V - 2]
    c0, h0, n0 = e.cost_matrix(nodes)
    c1, h1, n1 = e.cost_matrix(nodes, early_exit=True)
    assert np.array_equal(bits(c0), bits(c1)) and np.array_equal(h0, h1) and np.array_equal(n0, n1)
    # reachable agrees with filtering cost_field
    cost, hops, _, info = e.cost_field(source_xy=poses[0])
    reached = np.sort(cost[hops >= 0])
    budget = F32(reached[reached.size // 20])
    ids, c, h = e.reachable(poses[0], budget)
    want = np.flatnonzero((hops >= 0) & (cost <= budget))
    assert 0 < want.size < reached.size
    assert np.array_equal(ids, want) and np.array_equal(bits(c), bits(cost[want])) and np.array_equal(h, hops[want])
    e.close()


def test_errors(engine, tmp_path):
    import trg_planner
    from trg_planner._engine import TrgFieldInfo, _f, _i
    e = engine
    x = load_graph(e, fg.with_positions(fg.random_small(1)), tmp_path)
    src = np.array([0, x.V - 1, 0], np.int32)
    out = np.zeros(3, np.int32)

    def refused(budget=None, settle=0, targets=None, n_targets=None):
        b = None if budget is None else np.asarray(budget, np.float32)
        t = None if targets is None else np.asarray(targets, np.int32)
        nt = (0 if t is None else t.size) if n_targets is None else n_targets
        with pytest.raises(trg_planner.TrgError) as ei:
            e._chk(e.L.trg_engine_cost_field_bounded(e.h, 3, _i(src), None, None if b is None else _f(b), settle,
                                                     None, None, None, None if t is None else _i(t), nt, None, None,
                                                     None, _i(out), None, C.byref(TrgFieldInfo())))
        assert ei.value.status == INVALID_ARG, str(ei.value)
        return str(ei.value)

    assert "field 1" in refused(budget=[1.0, -1.0, 2.0])
    assert "field 2" in refused(budget=[1.0, 0.0, np.nan])
    assert "field 0" in refused(budget=[-np.inf, 0.0, 1.0])
    assert "settle mode 3" in refused(settle=3, targets=[0])
    assert "settle mode -1" in refused(settle=-1, targets=[0])
    assert "needs targets" in refused(settle=1) and "needs targets" in refused(settle=2, targets=[0], n_targets=0)
    assert "target 1" in refused(settle=1, targets=[0, x.V])  # (the batch call's check, under a settle mode too)
    with pytest.raises(ValueError):
        e.cost_fields(source_ids=[0], settle="some")
    # -0.0 is the budget 0; the call still works after the refusals
    r = e.cost_fields(source_ids=[0], budget=-0.0)
    assert r["bound"].view(np.uint32)[0] == 0 and r["reached"][0] >= 1 and np.all(r["cost"][0][r["hops"][0] >= 0] == 0)
