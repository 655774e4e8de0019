"""GPU: risk fields (trg_engine_risk_field_sets; Engine.risk_fields, risk_fields_from, safest_route, frontier_ceilings,
safest_frontier; DESIGN.md section 2, "Risk fields") -- for every node the least, over all walks, of the greatest edge
weight on the walk, with the hops of the tight subgraph and the smallest parent.

Every comparison is exact -- risk as bits, hops, parents, owners, route ids equal -- against the host Dijkstra on the
(risk, hops) key (tests/cpp/risk_reference.cpp through tests/risk_ref.py; tests/test_risk_field_cpu.py holds it against
the definition on the CPU and shows that the fixtures bite).  Bounds are the reference's full field truncated
(tests/bound_ref.py) at a bound computed from the reference, never from the engine.  Graphs come from
tests/risk_graphs.py and tests/field_graphs.py through load_json on an engine without a map; one test builds a small
terrain on the device."""
import numpy as np
import pytest

import bound_ref
import field_graphs as fg
import risk_graphs as rg
import risk_ref
from field_support import (INVALID_ARG, MOUNTAIN, SCALES, SCALES_LARGE, assert_rows, bits, engine,  # noqa: F401
                           load_graph, random_large, small_sources, with_isolated_node)
from graph_support import obs_crop

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = F32(np.inf)
SF = MOUNTAIN["safety_factor"]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """The compiled host Dijkstra of the risk field, once per module."""
    return risk_ref.compile_reference(tmp_path_factory.mktemp("risk_ref"))


def _check_full(e, ref, x, sources, at):
    """One solve from single sources, full outputs, against the reference -> the engine's result."""
    rr, rh, rp = risk_ref.reference_risks(ref, x, sources)
    r = e.risk_fields(source_ids=[int(s) for s in sources])
    assert_rows(at, "risks", r["risk"], rr, as_bits=True)
    assert_rows(at, "hops", r["hops"], rh)
    assert_rows(at, "parents", r["parent"], rp)
    assert np.array_equal(r["reached"], (rh >= 0).sum(axis=1)), at + f"reached {r['reached']}"
    assert r["info"].reached == int(r["reached"].sum()) and r["info"].source == int(sources[0]), at
    assert r["sources"].tolist() == [int(s) for s in sources], at
    return r


@pytest.mark.parametrize("seed", range(8))
def test_random_small(ref, engine, tmp_path, seed):
    """The redrawn random graphs at every bucket width; m = 1 (no item decode), 2, 5 and 64 sources, an Invalid source
    and the isolated node among them."""
    e = engine
    g = with_isolated_node(rg.redrawn(seed))
    x = load_graph(e, g, tmp_path)
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        for m in (1, 2, 5, 64):
            _check_full(e, ref, x, small_sources(g, m, seed), f"seed {seed}, width {scale}, m {m}: ")
    e.set_option("field_delta_scale", "4")


def test_random_large(ref, engine, tmp_path):
    g = rg.reweighted(random_large(*fg.RANDOM_LARGE[2000][0]), fg.RANDOM_LARGE[2000][0][0])
    x = load_graph(engine, g, tmp_path)
    valid = np.flatnonzero(x.state != fg.INVALID)
    for scale in SCALES_LARGE:
        engine.set_option("field_delta_scale", scale)
        r = _check_full(engine, ref, x, [int(valid[0])], f"2000 nodes, width {scale}, m 1: ")
        print(f"2000 nodes, width {scale}: {r['info'].rounds} rounds, reached {r['reached'].tolist()}")
        _check_full(engine, ref, x, [int(valid[0]), int(valid[-1]), int(valid[len(valid) // 2])],
                    f"2000 nodes, width {scale}, m 3: ")
    engine.set_option("field_delta_scale", "4")


SHAPES = {
    "star_70": (lambda: fg.star(70), [0, 5], ("4", "0.5", "inf")),                   # a row of 70: > 16 lanes, > a wave
    "star_70_redrawn": (lambda: rg.reweighted(fg.star(70), 70), [0, 5, 33], ("4", "0.5", "inf")),
    "chain_2000_rise_and_fall": (lambda: rg.rise_and_fall(2000), [0, 1500], ("4", "inf")),  # one node per round
    "lattice_12x12": (lambda: fg.lattice(12, 12), [0, 77], SCALES),  # every edge weighs 0.25: the parent decides
    "zero_weights": (lambda: rg.all_zero_weights(300), [0, 299], SCALES),           # bucket width 0
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_kernel_edge_shapes(ref, engine, tmp_path, name):
    make, sources, scales = SHAPES[name]
    x = load_graph(engine, make(), tmp_path)
    if name == "star_70":
        assert np.diff(x.rowptr)[0] == 70
    for scale in scales:
        engine.set_option("field_delta_scale", scale)
        for m in (1, len(sources)):
            r = _check_full(engine, ref, x, sources[:m], f"{name}, width {scale}, m {m}: ")
        if name == "chain_2000_rise_and_fall":
            peak = F32(x.w.max())
            assert np.all(r["risk"][0, 1001:] == peak) and r["risk"][0, 999] < peak
            assert r["info"].rounds >= 2 * 1999, r["info"].rounds  # one node per round, two passes
    engine.set_option("field_delta_scale", "4")


@pytest.mark.parametrize("name", sorted(rg.cases()))
def test_hand_written_cases(ref, engine, tmp_path, name):
    g, sources = rg.cases()[name]
    x = load_graph(engine, g, tmp_path)
    for scale in SCALES:
        engine.set_option("field_delta_scale", scale)
        for m in (1, len(sources)):
            r = _check_full(engine, ref, x, sources[:m], f"{name}, width {scale}, m {m}: ")
    engine.set_option("field_delta_scale", "4")
    if name == "negative_zero":  # a weight of -0 counts as +0: the risk words are +0, not the sign bit
        assert bits(r["risk"][0]).tolist()[:3] == [0, 0, 0]
    if name == "through_invalid":
        assert r["hops"][0].tolist() == [0, 1, -1, -1, -1]


def test_sets(ref, engine, tmp_path):
    """Two sets that hold duplicates and an Invalid member: risk, hops, parents, owners, owned and owner_at against the
    reference run from the set."""
    e = engine
    g = with_isolated_node(rg.redrawn(5))
    x = load_graph(e, g, tmp_path)
    V = x.V
    invalid = int(np.flatnonzero(x.state == fg.INVALID)[0])
    valid = np.flatnonzero(x.state != fg.INVALID)
    sets = [[int(valid[3]), int(valid[0]), invalid, int(valid[3]), int(valid[0])],
            [V - 1, int(valid[-2]), int(valid[1]), int(valid[-2])]]
    targets = np.arange(0, V, 3, dtype=np.int32)
    for scale in ("4", "1e-6", "inf"):
        e.set_option("field_delta_scale", scale)
        r = e.risk_fields_from(sets, targets=targets)
        for k, members in enumerate(sets):
            at = f"width {scale}, set {k}: "
            st, rr, rh, rp = risk_ref.risk_of_graph(ref, x, members)
            assert st == 0
            owner, owned = risk_ref.owners(members, rh, rp)
            assert np.array_equal(bits(r["risk"][k]), bits(rr)), at + "risk"
            assert np.array_equal(r["hops"][k], rh) and np.array_equal(r["parent"][k], rp), at + "hops, parents"
            assert np.array_equal(r["owner"][k], owner), at + "owner"
            assert np.array_equal(r["owned"][k], owned), at + f"owned {r['owned'][k]} != {owned}"
            assert np.array_equal(bits(r["risk_at"][k]), bits(rr[targets])), at + "risk_at"
            assert np.array_equal(r["hops_at"][k], rh[targets]), at + "hops_at"
            assert np.array_equal(r["owner_at"][k], owner[targets]), at + "owner_at"
            assert r["reached"][k] == int((rh >= 0).sum()) == int(owned.sum()), at
        assert r["sources"].tolist() == [s[0] for s in sets]
        # routes of a set solve end at the member that owns the target
        pairs = [(k, int(t)) for k in range(2) for t in targets]
        got = e.routes([k for k, _ in pairs], [t for _, t in pairs], xyz=False)
        for (k, t), (ids, _, one) in zip(pairs, got):
            st, rr, rh, rp = risk_ref.risk_of_graph(ref, x, sets[k])
            want = risk_ref.route(x, rr, rh, rp, t)
            assert np.array_equal(ids, want[0]), f"set {k}, target {t}: {ids} != {want[0]}"
            if ids.size:
                owner, _ = risk_ref.owners(sets[k], rh, rp)
                assert ids[0] == sets[k][owner[t]]
    e.set_option("field_delta_scale", "4")


def _check_bounded(e, full, sources, at, budget=None, settle=None, targets=None):
    rr, rh, rp = full
    m = len(sources)
    bud = np.full(m, INF, F32) if budget is None else np.broadcast_to(np.asarray(budget, F32).reshape(-1), (m,))
    want_bound = np.array([min(bud[k], bound_ref.settle_bound(rr[k], rh[k], targets, settle)) for k in range(m)], F32)
    tr, th, tp = bound_ref.truncate(rr, rh, rp, want_bound)
    r = e.risk_fields(source_ids=[int(s) for s in sources], targets=targets, budget=budget, settle=settle)
    assert np.array_equal(bits(r["bound"]), bits(want_bound)), at + f"bound {r['bound']!r} != {want_bound!r}"
    assert_rows(at, "risks", r["risk"], tr, as_bits=True)
    assert_rows(at, "hops", r["hops"], th)
    assert_rows(at, "parents", r["parent"], tp)
    assert np.array_equal(r["reached"], (th >= 0).sum(axis=1)), at + f"reached {r['reached']}"
    if targets is not None:
        t = np.asarray(targets, np.int64)
        assert np.array_equal(bits(r["risk_at"]), bits(tr[:, t])), at + "risk_at"
        assert np.array_equal(r["hops_at"], th[:, t]), at + "hops_at"
    return r


def test_bounds(ref, engine, tmp_path):
    """A budget is a ceiling: equal bits stay within it, everything riskier is unreached, the rest untouched; settle
    ANY / ALL lower it to the least / greatest risk over the targets, an unreachable target among them or not."""
    e = engine
    g = with_isolated_node(rg.redrawn(7))
    x = load_graph(e, g, tmp_path)
    V = x.V
    sources = small_sources(g, 5, 7)
    full5 = risk_ref.reference_risks(ref, x, sources)
    valid_src = [k for k, s in enumerate(sources) if (full5[1][k] >= 0).sum() > 4]
    k0 = valid_src[0]
    src = sources[k0]
    full1 = tuple(a[k0:k0 + 1] for a in full5)
    rr0, rh0 = full1[0][0], full1[1][0]
    levels = np.unique(rr0[rh0 > 0])
    assert levels.size >= 3 and levels[0] >= F32(0.1), levels
    mid = F32(levels[levels.size // 2])
    reach = np.flatnonzero(rh0 > 0)
    reach = reach[np.argsort(rr0[reach], kind="stable")]
    a, b, c = int(reach[0]), int(reach[reach.size // 2]), int(reach[-1])
    unreachable = int(np.flatnonzero((rh0 < 0) & (x.state != fg.INVALID))[0])
    for scale in SCALES:
        e.set_option("field_delta_scale", scale)
        u = e.risk_fields(source_ids=[src])
        for budget in (mid, F32(np.nextafter(mid, F32(0.0))), F32(0.05), F32(0.0), F32(levels[-1]), INF):
            at = f"width {scale}, m 1, budget {budget!r}: "
            r = _check_bounded(e, full1, [src], at, budget=budget, targets=[a, b, c, unreachable])
            if budget == mid:
                assert (r["risk"][0] == mid).any(), at + "no node at the budget itself"
            if budget == F32(0.05):  # below every positive weight: the source alone
                assert r["reached"][0] == 1, at
                assert r["info"].rounds <= u["info"].rounds, at + f"{r['info'].rounds} > {u['info'].rounds} rounds"
        mixed = np.array([0.0, mid, 0.05, levels[-1], np.inf], F32)
        _check_bounded(e, full5, sources, f"width {scale}, m 5, budgets {mixed!r}: ", budget=mixed, targets=[a, b])
        for mode in ("any", "all"):
            for name, targets in (("reachable", [b, a, b, c]), ("the source", [src]),
                                  ("with an unreachable one", [b, unreachable, a]),
                                  ("none reachable", [unreachable, V - 1])):
                at = f"width {scale}, settle {mode}, targets {name}: "
                _check_bounded(e, full1, [src], at, settle=mode, targets=targets)
                _check_bounded(e, full5, sources, at + "m 5: ", settle=mode, targets=targets)
                _check_bounded(e, full1, [src], at + "and a budget: ", budget=mid, settle=mode, targets=targets)
    e.set_option("field_delta_scale", "4")


def _check_routes(e, x, fields, pairs, at):
    """Routes of the retained solve against the host walk; fields: (risk, hops, parent) per field."""
    got = e.routes([k for k, _ in pairs], [t for _, t in pairs], xyz=True)
    for (k, t), (ids, xyz, one) in zip(pairs, got):
        rr, rh, rp = fields[k]
        want_ids, edges, cost, pl, avg = risk_ref.route(x, rr, rh, rp, t)
        where = at + f"field {k}, target {t}: "
        assert np.array_equal(ids, want_ids), where + f"{ids} != {want_ids}"
        assert one.num_nodes == want_ids.size, where
        assert bits(one.cost) == bits(cost) and bits(one.cost) == bits(rr[t]), where + f"cost {one.cost!r}"
        assert bits(one.path_length) == bits(pl), where + f"path_length {one.path_length!r} != {pl!r}"
        assert bits(one.avg_risk) == bits(avg), where + f"avg_risk {one.avg_risk!r} != {avg!r}"
        assert np.array_equal(xyz.view(np.uint32), x.xyz[want_ids].view(np.uint32)), where


@pytest.mark.parametrize("how", ["parents in the solve", "late parent sweep"])
def test_routes(ref, engine, tmp_path, how):
    e = engine
    e.set_option("field_delta_scale", "4")
    # the duplicate-edge case decides the edge: dist 2 (not 1) into node 1, 3 (not 1 or 5) into node 2, 7 into node 3
    g, _ = rg.cases()["duplicates"]
    x = load_graph(e, g, tmp_path, "dup")
    fields = [risk_ref.risk_of_graph(ref, x, s)[1:] for s in (0, 1)]
    r = e.risk_fields(source_ids=[0, 1], full=how == "parents in the solve")
    _check_routes(e, x, fields, [(k, t) for k in range(2) for t in range(4)], "duplicates: ")
    one = e.routes([0], [3], xyz=False)[0][2]
    assert one.path_length == F32(12.0) and one.cost == F32(0.4), (one.path_length, one.cost)
    assert bits(one.avg_risk) == bits(F32(F32(F32(F32(0.1) + F32(0.4)) + F32(0.2)) / F32(4.0)))
    # a random graph: every node of three fields, unreachable ones and the source among them
    g = with_isolated_node(rg.redrawn(3))
    x = load_graph(e, g, tmp_path, "rand")
    sources = small_sources(g, 3, 3)
    fields = [risk_ref.risk_of_graph(ref, x, s)[1:] for s in sources]
    r = e.risk_fields(source_ids=sources, full=how == "parents in the solve", targets=[0])
    assert ("parent" in r) == (how == "parents in the solve")
    _check_routes(e, x, fields, [(k, t) for k in range(3) for t in range(x.V)], "redrawn 3: ")
    ids, cost, hops = e.field_reached(1)
    rr, rh, _ = fields[1]
    assert np.array_equal(ids, np.flatnonzero(rh >= 0)) and np.array_equal(bits(cost), bits(rr[rh >= 0]))
    assert np.array_equal(hops, rh[rh >= 0])


def _same(a, b, keys):
    for key in keys:
        assert np.array_equal(np.asarray(a[key]).view(np.int32), np.asarray(b[key]).view(np.int32)), key


def test_beside_cost_solves(ref, engine, tmp_path):
    """A cost solve, a risk solve, the same cost solve again: the cost results are equal bit for bit, plain and with
    two models, and neither kind computes its edge values a second time (one host wait fewer)."""
    e = engine
    e.set_option("field_delta_scale", "4")
    g = with_isolated_node(rg.redrawn(2))
    x = load_graph(e, g, tmp_path)
    sources = small_sources(g, 2, 2)
    keys = ("cost", "hops", "parent", "reached")
    c1 = e.cost_fields(source_ids=sources)
    k1 = e.risk_fields(source_ids=sources)
    c2 = e.cost_fields(source_ids=sources)
    k2 = e.risk_fields(source_ids=sources)
    _same(c1, c2, keys)
    _same(k1, k2, ("risk", "hops", "parent", "reached"))
    rr, rh, rp = risk_ref.reference_risks(ref, x, sources)
    assert_rows("after a cost solve: ", "risks", k2["risk"], rr, as_bits=True)
    assert_rows("after a cost solve: ", "hops", k2["hops"], rh)
    assert c2["info"].host_syncs == c1["info"].host_syncs - 1, (c1["info"].host_syncs, c2["info"].host_syncs)
    assert k2["info"].host_syncs == k1["info"].host_syncs - 1, (k1["info"].host_syncs, k2["info"].host_syncs)
    models = [(1.5, 0.3), (SF, np.inf)]
    m1 = e.cost_fields(source_ids=sources, models=models)
    k3 = e.risk_fields(source_ids=sources)
    m2 = e.cost_fields(source_ids=sources, models=models)
    _same(m1, m2, keys)
    _same(k1, k3, ("risk", "hops", "parent", "reached"))
    assert m2["info"].host_syncs == m1["info"].host_syncs - 1 and k3["info"].host_syncs == k2["info"].host_syncs
    # a cost model of the engine's safety factor is not the risk slot, nor the other way round
    _same(c1, e.cost_fields(source_ids=sources, models=[None, None]), keys)


def _pairs(g, n):
    """n (start, goal) node pairs with goal != start over the valid nodes of both components and the isolated node."""
    valid = np.flatnonzero(g.state != fg.INVALID)
    out = []
    for i in range(n):
        a = int(valid[(3 * i) % valid.size])
        b = int(valid[(7 * i + 5) % valid.size])
        if a != b:
            out.append((a, b))
    return out


@pytest.mark.parametrize("seed", [1, 4])
def test_safest_route_equals_min_risk_ceiling(ref, engine, tmp_path, seed):
    e = engine
    e.set_option("field_delta_scale", "4")
    g = with_isolated_node(rg.redrawn(seed))
    x = load_graph(e, g, tmp_path)
    pairs = _pairs(g, 6)[:5]
    assert len(pairs) == 5
    reachable = 0
    for a, b in pairs:
        at = f"seed {seed}, {a} -> {b}: "
        start, goal = g.pos[a, :2], g.pos[b, :2]
        na, nb = (int(v) for v in e._resolve_nodes([start, goal]))
        assert na != nb, at
        want = e.min_risk_ceiling(start, goal)
        got = e.safest_route(start, goal)
        rr, rh, _ = risk_ref.risk_of_graph(ref, x, na)[1:]
        assert (got is None) == (want is None) == (rh[nb] < 0), at
        if got is None:
            continue
        reachable += 1
        assert bits(got[0]) == bits(want[0]) == bits(rr[nb]), at + f"{got[0]!r}, {want[0]!r}, {rr[nb]!r}"
        a_rec, b_rec = got[1], want[1]
        assert a_rec["model"] == b_rec["model"] and a_rec["reachable"] and b_rec["reachable"], at
        assert np.array_equal(a_rec["ids"], b_rec["ids"]) and a_rec["ids"][0] == na and a_rec["ids"][-1] == nb, at
        assert np.array_equal(a_rec["xyz"].view(np.uint32), b_rec["xyz"].view(np.uint32)), at
        for key in ("cost", "path_length", "avg_risk"):
            assert bits(a_rec[key]) == bits(b_rec[key]), at + key
    print(f"seed {seed}: {reachable} of {len(pairs)} pairs reachable")
    # goal == start: no edge has to be crossed
    a = pairs[0][0]
    na = int(e._resolve_nodes([g.pos[a, :2]])[0])
    tau, rec = e.safest_route(g.pos[a, :2], g.pos[a, :2])
    assert bits(tau) == 0 and rec["ids"].tolist() == [na] and rec["cost"] == 0.0 and rec["path_length"] == 0.0


def test_safest_route_reachable_and_not(ref, engine, tmp_path):
    """Over both test graphs the ten pairs hold reachable and unreachable goals."""
    kinds = set()
    for seed in (1, 4):
        g = with_isolated_node(rg.redrawn(seed))
        for a, b in _pairs(g, 6)[:5]:
            kinds.add(bool(risk_ref.risk_of_graph(ref, g, a)[2][b] >= 0))
    assert kinds == {True, False}
    # (and through the engine: an unreachable goal gives None)
    g = with_isolated_node(rg.redrawn(1))
    load_graph(engine, g, tmp_path)
    V = len(g.state)
    valid = np.flatnonzero(g.state != fg.INVALID)
    assert engine.safest_route(g.pos[int(valid[0]), :2], g.pos[V - 1, :2]) is None


@pytest.mark.parametrize("seed", [0, 6])
def test_frontier_helpers(ref, engine, tmp_path, seed):
    e = engine
    e.set_option("field_delta_scale", "4")
    g = with_isolated_node(rg.redrawn(seed))
    x = load_graph(e, g, tmp_path)
    frontier = np.flatnonzero(x.state == 1).astype(np.int32)
    assert frontier.size
    valid = np.flatnonzero(x.state != fg.INVALID)
    for a in (int(valid[0]), int(valid[-2]), x.V - 1):
        pose = g.pos[a, :2]
        src = int(e._resolve_nodes([pose])[0])
        _, rr, rh, rp = risk_ref.risk_of_graph(ref, x, src)
        ids, risk, hops = e.frontier_ceilings(pose)
        assert np.array_equal(ids, frontier)
        assert np.array_equal(bits(risk), bits(rr[frontier])) and np.array_equal(hops, rh[frontier])
        got = e.safest_frontier(pose)
        ok = frontier[rh[frontier] >= 0]
        if ok.size == 0:
            assert got is None
            continue
        best = int(ok[np.lexsort((ok, rh[ok], rr[ok]))[0]])
        assert got[0] == best and bits(got[1]) == bits(rr[best]), (got, best)
        assert got[2] == risk_ref.route(x, rr, rh, rp, best)[0].tolist()


@pytest.mark.parametrize("name", sorted(rg.bad_weights()))
def test_bad_weights(engine, tmp_path, name):
    """A NaN, negative or infinite weight: status 1, a message about the weight and nothing else, and the solve that
    was retained is gone, as after a bad-cost error.  No solve succeeds on the graphs with a NaN or an infinite weight
    (every cost model's edge cost is NaN there), so what is retained beforehand is a solve of the graph loaded before:
    routes call it stale ("earlier graph") until the failing risk solve begins, and unknown afterwards.  On the graph
    with the negative weight a cost solve under safety factor 0 succeeds and is retained on the graph itself."""
    import trg_planner
    e = engine

    def routes_refused(words):
        with pytest.raises(trg_planner.TrgError) as ei:
            e.routes([0], [1], xyz=False)
        assert ei.value.status == INVALID_ARG and words in str(ei.value), str(ei.value)

    load_graph(e, rg.cases()["duplicates"][0], tmp_path, "before")
    e.risk_fields(source_ids=[0])
    assert e.routes([0], [1], xyz=False)[0][2].num_nodes == 2
    g = rg.bad_weights()[name]
    p = tmp_path / "bad.json"
    fg.write_json(p, g)
    e.load_json(str(p))
    x = e.graph("global")
    assert x.E == 3 and (np.isnan(x.w[2]) if name == "nan" else x.w[2] == g.w[2])
    routes_refused("earlier graph")  # the retained solve is still there, of the graph before
    if name == "negative":
        e.cost_fields(source_ids=[0], models=[0.0])
        assert len(e.routes([0], [1], xyz=False)) == 1
    with pytest.raises(trg_planner.TrgError) as ei:
        e.risk_fields(source_ids=[0])
    msg = str(ei.value)
    assert ei.value.status == INVALID_ARG and "weight" in msg, msg
    assert "earlier graph" not in msg and "retained" not in msg, msg
    routes_refused("no cost-field solve is retained")  # ... and now it is gone
    # the engine solves again on a good graph
    load_graph(e, rg.cases()["duplicates"][0], tmp_path, "good")
    assert e.risk_fields(source_ids=[0])["hops"][0].tolist() == [0, 1, 2, 3]


def test_device_built_graph_and_refresh_refusal(ref, synth):
    """One real build: a small terrain of the mountain_small shape, built on the device; the risk fields from the root
    against the reference on the exported CSR, with a positive ceiling for some node.  Then an update_graph: a retained
    risk solve is not refreshed, and routes refuse the stale solve as they refuse a stale cost solve."""
    import trg_planner
    cloud = synth.mountain_cloud(160, 160, seed=11, amplitude=5.0, wavelength=14.0)
    e = trg_planner.Engine(**MOUNTAIN)
    try:
        e.set_sampler(7, 16)
        e.set_global_map(cloud)
        e.init_graph([8.0, 8.0, 0.0])
        x = e.graph("global")
        r = e.risk_fields(sources_xy=[(8.0, 8.0)])
        src = int(r["sources"][0])
        st, rr, rh, rp = risk_ref.risk_of_graph(ref, x, src)
        assert st == 0
        assert_rows("device build: ", "risks", r["risk"], rr[None], as_bits=True)
        assert_rows("device build: ", "hops", r["hops"], rh[None])
        assert_rows("device build: ", "parents", r["parent"], rp[None])
        positive = np.isfinite(rr) & (rr > 0)
        print(f"device build: V {x.V}, E {x.E}, reached {int(r['reached'][0])}, {int(positive.sum())} nodes with a "
              f"positive ceiling, greatest {rr[np.isfinite(rr)].max()!r}, {r['info'].rounds} rounds")
        assert positive.any()
        t = int(np.flatnonzero(positive)[-1])
        _check_routes(e, x, [(rr, rh, rp)], [(0, t), (0, src)], "device build: ")
        pose = (6.0, 6.0)
        e.set_local_map(pose, obs_crop(cloud, pose, 4.0, box=(pose[0] + 2.0, pose[1] + 1.0, 0.6)))
        e.update_graph()
        with pytest.raises(trg_planner.TrgError) as ei:
            e.refresh_fields()
        assert ei.value.status == INVALID_ARG and "risk field" in str(ei.value), str(ei.value)
        with pytest.raises(trg_planner.TrgError) as ei:
            e.routes([0], [t])
        assert ei.value.status == INVALID_ARG and "earlier graph" in str(ei.value), str(ei.value)
        # a new risk solve on the updated graph (the uploaded CSR) answers again
        x2 = e.graph("global")
        r = e.risk_fields(sources_xy=[(8.0, 8.0)])
        st, rr, rh, rp = risk_ref.risk_of_graph(ref, x2, int(r["sources"][0]))
        assert_rows("after the update: ", "risks", r["risk"], rr[None], as_bits=True)
        assert_rows("after the update: ", "hops", r["hops"], rh[None])
        assert_rows("after the update: ", "parents", r["parent"], rp[None])
    finally:
        e.close()
