"""GPU: keep-out zones (trg_engine_cost_field_zones / trg_engine_zone_edges, Engine.cost_fields_avoiding /
closed_edges / plan_avoiding; DESIGN.md section 2, "Keep-out zones").

Every comparison is exact.  The verdicts of closed_edges equal tests/zone_ref.py's byte for byte; the fields equal --
cost as bits; hops, parents, owners, `owned`, `reached`, bounds as bits, route ids and route floats as bits -- the
existing host references (tests/set_ref.py, seed_ref.py, bound_ref.py, route_ref.py) on zone_ref.pruned(): the graph
WITHOUT the edges the field's zone set closes and without those above its ceiling, at its safety factor.  Positions are
the engine's own (node_xyz()); nothing else expected comes from the engine.

Shapes: the smallest at which each piece can go wrong -- a 6 x 4 lattice whose geometry is exact in fp32, rows of 20
edges (two trips of a 16-lane group) and ragged ends, V ~ 9-48 random graphs with every kind of source, 64 distinct zone
sets and a 65th, the update pairs of the refresh tests, one map-built graph of a few thousand nodes and one random
graph of 20 000."""
import numpy as np
import pytest

import bound_ref
import field_graphs as fg
import model_ref
import refresh_pairs as rp
import route_ref
import seed_ref
import set_ref
import zone_ref as zr
from field_support import (INVALID_ARG, MOUNTAIN, assert_rows, bits, engine, load_graph,  # noqa: F401
                           random_large, small_sources, with_isolated_node)
from test_zone_ref_cpu import closed_links, lattice_cases

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = F32(np.inf)
SF = MOUNTAIN["safety_factor"]


def _b1(v):
    return int(np.float32(v).view(np.uint32))


def _median_model(x):
    return (3.0, float(np.median(x.w)))


def _zones_near(rng, pos, n, r_max=1.3):
    """n zones centred near nodes drawn at random (so that they shut something), radii 0 .. r_max."""
    at = pos[rng.integers(0, pos.shape[0], size=n), :2] + rng.uniform(-0.4, 0.4, size=(n, 2))
    return np.concatenate([at, rng.uniform(0.0, r_max, size=(n, 1))], axis=1).astype(F32)


def _verdicts(e, x, pos, zones, at):
    """closed_edges against the reference, byte for byte -> the reference's (closed, inside)."""
    got = e.closed_edges(zones)
    closed, inside = zr.closed(x, zones, pos), zr.inside(x, zones, pos)
    assert got["closed"].dtype == np.uint8 and got["closed"].shape == (x.E,) and got["inside"].shape == (x.V,), at
    bad = np.flatnonzero(got["closed"] != closed.astype(np.uint8))
    assert bad.size == 0, at + f"{bad.size} edge verdicts differ, first at CSR edge {bad[:1]}"
    assert np.array_equal(got["inside"], inside.astype(np.uint8)), at + "inside"
    assert got["n_closed"] == int(closed.sum()) and got["n_inside"] == int(inside.sum()), at
    return closed, inside


def _refs(x, pos, zone_sets, models, sets, costs=None):
    """The reference field of every (zone set, model, set[, start costs]): today's references on the pruned graph."""
    out = []
    for k, (zones, mo, members) in enumerate(zip(zone_sets, models, sets)):
        s, tau = model_ref.as_model(mo, SF)
        p = zr.pruned(x, zones, tau, pos)
        out.append(set_ref.set_field(p, s, members) if costs is None else seed_ref.seeded_field(p, s, members, costs[k]))
    return out


def _check(e, refs, zone_sets, models, sets, at, costs=None, budget=None, settle=None, targets=None, full=True):
    """One zone solve against the (truncated) reference fields -> the engine's result."""
    m = len(sets)
    want = refs
    bounded = budget is not None or settle is not None
    if bounded:
        bud = np.full(m, INF, F32) if budget is None else np.broadcast_to(np.asarray(budget, F32).reshape(-1), (m,))
        want_bound = np.array([min(bud[k], bound_ref.settle_bound(refs[k].cost, refs[k].hops, targets, settle))
                               for k in range(m)], F32)
        want = [set_ref.truncate(refs[k], want_bound[k]) for k in range(m)]
    r = e.cost_fields_avoiding(sets, zone_sets, models=None if all(mo is None for mo in models) else models,
                               start_costs=costs, targets=targets, full=full, budget=budget, settle=settle)
    if bounded:
        assert np.array_equal(bits(r["bound"]), bits(want_bound)), at + f"bound {r['bound']!r} != {want_bound!r}"
    else:
        assert "bound" not in r
    stack = [np.stack([getattr(f, name) for f in want]) for name in ("cost", "hops", "parent", "owner")]
    assert np.array_equal(r["reached"], (stack[1] >= 0).sum(axis=1)), at + f"reached {r['reached']}"
    for k in range(m):
        assert np.array_equal(r["owned"][k], want[k].owned), at + f"owned of set {k}: {r['owned'][k]}"
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
    return r


def _route_ref(x, pos, zones, mo, f, members, t):
    """route_ref's route of the field f to t on the pruned graph, its edges as CSR indices of x."""
    s, tau = model_ref.as_model(mo, SF)
    p = zr.pruned(x, zones, tau, pos)
    w = route_ref.route(p.rowptr, p.col, p.w, p.dist, p.state, s, f.cost, f.hops, f.parent, members[f.owner[t]], t)
    return w._replace(edges=p.kept[w.edges] if len(w.edges) else w.edges)


def _check_routes(e, x, pos, refs, zone_sets, models, sets, pairs, at):
    """Routes (field, target) of the retained solve against route_ref on the pruned graph; no route edge is closed."""
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
        w = _route_ref(x, pos, zone_sets[k], models[k], f, sets[k], t)
        assert np.array_equal(ids, w.ids), where + f"ids {ids.tolist()} != {w.ids.tolist()}"
        assert np.array_equal(bits(pts), bits(pos[w.ids])), where
        for nm in ("cost", "path_length", "avg_risk"):
            assert _b1(getattr(one, nm)) == _b1(getattr(w, nm)), where + nm
        assert not zr.closed(x, zone_sets[k], pos)[w.edges].any() and np.array_equal(row[w.edges], ids[:-1]), where
    return unreached


# ---- the verdicts -------------------------------------------------------------------------------------------------
def test_exact_geometry_on_the_lattice(engine, tmp_path):
    e = engine
    x = load_graph(e, fg.lattice(6, 4), tmp_path)
    pos = e.node_xyz()
    for name, (zones, want) in sorted(lattice_cases().items()):
        closed, inside = _verdicts(e, x, pos, zones, name + ": ")
        assert closed_links(x, closed) == want and closed.sum() == 2 * len(want), name
        assert inside.sum() == (1 if name == "point_on_a_node" else 0), name
    _verdicts(e, x, pos, None, "no zones: ")
    both = [lattice_cases()["point_on_a_midpoint"][0][0], lattice_cases()["tangent"][0][0]]
    assert _verdicts(e, x, pos, both, "two zones: ")[0].sum() == 4


def test_long_rows_and_ragged_ends(engine, tmp_path):
    """Rows wider than a 16-lane group (two hubs of 20 spokes, a ring), a graph without edges, an isolated last node,
    node counts that are no multiple of 64, and the full 256 zones."""
    e = engine
    g = fg.star(40, hubs=2)
    x = load_graph(e, g, tmp_path, "star")
    assert np.diff(x.rowptr).max() >= 20 and x.V % 64 != 0
    pos = e.node_xyz()
    leaves = pos[2:42, :2]
    across = [(float(leaves[5:9, 0].mean()), float(leaves[5:9, 1].mean()), 1.2)]
    closed, _ = _verdicts(e, x, pos, across, "star, a zone across some spokes: ")
    hub_rows = closed[x.rowptr[0]:x.rowptr[2]]
    assert hub_rows.any() and not hub_rows.all()
    rng = np.random.default_rng(3)
    _verdicts(e, x, pos, _zones_near(rng, pos, 256, 0.8), "star, 256 zones: ")
    refs = _refs(x, pos, [across, None], [None, None], [[x.V - 1], [x.V - 1]])
    assert refs[0].cost.tobytes() != refs[1].cost.tobytes()
    _check(e, refs, [across, None], [None, None], [[x.V - 1], [x.V - 1]], "star: ", targets=[2, 7, 41])
    g = fg.oddities()["no_edges"][0]
    x = load_graph(e, g, tmp_path, "no_edges")
    pos = e.node_xyz()
    z = [(float(pos[3, 0]), float(pos[3, 1]), 0.5)]
    closed, inside = _verdicts(e, x, pos, z, "no edges: ")
    assert x.E == 0 and closed.size == 0 and inside.tolist() == [False, False, False, True, False]
    refs = _refs(x, pos, [z, z], [None, None], [[0], [3]])
    _check(e, refs, [z, z], [None, None], [[0], [3]], "no edges: ", targets=[3])
    g = with_isolated_node(fg.with_positions(fg.random_small(7)))
    x = load_graph(e, g, tmp_path, "isolated")
    pos = e.node_xyz()
    z = [(float(pos[-1, 0]), float(pos[-1, 1]), 0.25), (float(pos[1, 0]), float(pos[1, 1]), 1.0)]
    closed, inside = _verdicts(e, x, pos, z, "an isolated node: ")
    assert inside[-1] and inside[1] and closed.any()


# ---- the fields ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [7, 13, 21])
def test_random_graphs(engine, tmp_path, seed):
    """Three fields with three zone sets (one of them empty) per model of {None, (0, inf), (3, median weight)}, full,
    at targets, under budgets and settle modes; then the same with start costs."""
    e = engine
    g = with_isolated_node(fg.with_positions(fg.random_small(seed)))
    x = load_graph(e, g, tmp_path)
    pos = e.node_xyz()
    assert (x.state == fg.INVALID).any()
    rng = np.random.default_rng(seed)
    zone_sets = [_zones_near(rng, pos, 3), None, _zones_near(rng, pos, 7, 0.9)]
    for z in zone_sets:
        _verdicts(e, x, pos, z, f"seed {seed}: ")
    src = small_sources(g, 3, seed)
    sets = [[src[0]], [src[1], src[0]], [src[2], x.V - 1, src[1]]]
    targets = [src[0], x.V - 1, x.V // 2, 3]
    differs = 0
    for mo in (None, (0.0, np.inf), _median_model(x)):
        models = [mo] * 3
        at = f"seed {seed}, model {mo}: "
        refs = _refs(x, pos, zone_sets, models, sets)
        plain = _refs(x, pos, [None] * 3, models, sets)
        differs += sum(a.cost.tobytes() != b.cost.tobytes() or a.parent.tobytes() != b.parent.tobytes()
                       for a, b in zip(refs, plain))
        _check(e, refs, zone_sets, models, sets, at, targets=targets)
        _check(e, refs, zone_sets, models, sets, at + "at the targets: ", targets=targets, full=False)
        reached = np.sort(refs[0].cost[refs[0].hops >= 0])
        for budget, settle in ((float(reached[reached.size // 2]), None), (None, "any"), (None, "all"),
                               ([0.0, float(reached[-1]), 1e30], "any")):
            _check(e, refs, zone_sets, models, sets, at + f"budget {budget}, settle {settle}: ", budget=budget,
                   settle=settle, targets=targets)
        costs = [[0.25], [0.0, 1.5], [2.0, 0.0, 0.5]]
        seeded = _refs(x, pos, zone_sets, models, sets, costs)
        _check(e, seeded, zone_sets, models, sets, at + "start costs: ", costs=costs, targets=targets)
        _check(e, seeded, zone_sets, models, sets, at + "start costs, settle any: ", costs=costs, targets=targets,
               settle="any")
    assert differs >= 2, "the zones change no field of this seed"


def test_particular_cases(engine, tmp_path):
    """On the 6 x 4 lattice: a member inside a zone keeps its key and reaches nothing; a target inside a zone is
    unreached; a wall of zones splits the graph; no zones at all is cost_fields_seeded bit for bit."""
    e = engine
    x = load_graph(e, fg.lattice(6, 4), tmp_path)
    pos = e.node_xyz()
    n = lambda ix, iy: iy * 6 + ix
    on_source = [(0.0, 0.0, 0.25)]
    on_target = [(5.0, 3.0, 0.0)]
    wall = [(2.5, float(iy), 0.1) for iy in range(4)]
    zone_sets = [on_source, on_target, wall, [(9.0, 9.0, 0.5)]]
    sets = [[n(0, 0), n(1, 1)], [n(0, 0)], [n(0, 0)], [n(0, 0)]]
    models = [None] * 4
    refs = _refs(x, pos, zone_sets, models, sets)
    assert refs[0].hops[n(0, 0)] == 0 and refs[0].owned.tolist() == [1, 23]
    assert refs[1].hops[n(5, 3)] == -1 and (refs[1].hops >= 0).sum() == 23
    assert (refs[2].hops >= 0).sum() == 12 and (refs[2].hops[[n(ix, 0) for ix in range(6)]] >= 0).tolist() == [True] * 3 + [False] * 3
    r = _check(e, refs, zone_sets, models, sets, "particular: ", targets=[n(5, 3), n(0, 0), n(3, 0)])
    assert r["hops_at"][:, 0].tolist() == [6, -1, -1, 8] and np.isposinf(r["cost_at"][1, 0])
    # settle "any" on a target the zone shuts never stops that field; the others stop at it
    r = _check(e, refs, zone_sets, models, sets, "particular, settle: ", targets=[n(5, 3)], settle="any")
    assert np.isposinf(r["bound"][1]) and np.isposinf(r["bound"][2]) and r["bound"][3] == refs[3].cost[n(5, 3)]
    # no zones: None, an empty array, empty lists per field -- cost_fields_seeded on every output
    costs = [[0.5, 0.0], [0.0], [1.0], [0.0]]
    plain = e.cost_fields_seeded(sets, costs, targets=[n(5, 3), 3], budget=[4.0, 100.0, 2.0, 100.0])
    for none in (None, np.empty((0, 3), F32), [None, np.empty((0, 3)), None, None]):
        r = e.cost_fields_avoiding(sets, none, start_costs=costs, targets=[n(5, 3), 3], budget=[4.0, 100.0, 2.0, 100.0])
        for key in ("cost", "hops", "parent", "owner", "cost_at", "hops_at", "owner_at", "reached", "bound"):
            assert np.array_equal(np.asarray(r[key]).view(np.uint32), np.asarray(plain[key]).view(np.uint32)), key
        assert all(np.array_equal(a, b) for a, b in zip(r["owned"], plain["owned"]))


# ---- slots --------------------------------------------------------------------------------------------------------
def test_64_zone_sets_a_65th_and_one_bit_of_r(engine, tmp_path):
    e = engine
    g = with_isolated_node(fg.with_positions(fg.random_small(13)))
    x = load_graph(e, g, tmp_path)
    pos = e.node_xyz()
    rng = np.random.default_rng(64)
    zone_sets = [_zones_near(rng, pos, 1 + k % 5) for k in range(65)]
    assert len({z.tobytes() for z in zone_sets}) == 65
    sets = [[(5 * k + 2) % x.V] for k in range(64)]
    models = [None] * 64
    refs = _refs(x, pos, zone_sets[:64], models, sets)
    _check(e, refs, zone_sets[:64], models, sets, "64 zone sets: ", targets=[x.V - 1, 3])
    one = _refs(x, pos, zone_sets[64:], [None], sets[:1])
    _check(e, one, zone_sets[64:], [None], sets[:1], "a 65th zone set: ")
    plain = [set_ref.set_field(x, SF, s) for s in sets[:3]]
    r = e.cost_fields(source_ids=[s[0] for s in sets[:3]])
    assert_rows("plain after 65 zone sets: ", "costs", r["cost"], np.stack([f.cost for f in plain]), as_bits=True)
    assert_rows("plain after 65 zone sets: ", "hops", r["hops"], np.stack([f.hops for f in plain]))
    _check(e, refs, zone_sets[:64], models, sets, "64 zone sets again: ", full=False, targets=[0, 7])
    # two byte-equal lists beside one that differs in a single bit of r: the tangent zone of the lattice
    x = load_graph(e, fg.lattice(6, 4), tmp_path, "lattice")
    pos = e.node_xyz()
    tangent = np.array([(2.5, 1.25, 0.25)], F32)
    short = tangent.copy()
    short[0, 2] = np.nextafter(F32(0.25), F32(0.0))
    assert (tangent.view(np.uint32) != short.view(np.uint32)).sum() == 1
    three = [tangent, short, tangent.copy()]
    refs = _refs(x, pos, three, [None] * 3, [[8]] * 3)
    assert refs[0].cost[9] > refs[1].cost[9] and refs[0].cost.tobytes() == refs[2].cost.tobytes()
    _check(e, refs, three, [None] * 3, [[8]] * 3, "one bit of r: ")


# ---- limits -------------------------------------------------------------------------------------------------------
def test_limits_and_refusals(engine, tmp_path):
    import trg_planner
    e = engine
    x = load_graph(e, fg.lattice(6, 4), tmp_path)
    pos = e.node_xyz()
    rng = np.random.default_rng(5)
    full = _zones_near(rng, pos, 256, 0.3)
    refs = _refs(x, pos, [full], [None], [[0]])
    _check(e, refs, [full], [None], [[0]], "256 zones: ")
    e.cost_fields_avoiding([[0]], [full[:3]])

    def refused(words, call):
        with pytest.raises(trg_planner.TrgError) as ei:
            call()
        assert ei.value.status == INVALID_ARG and all(w in str(ei.value) for w in words), str(ei.value)

    over = np.concatenate([full, full[:1]])
    refused(["field 1", "257 zones"], lambda: e.cost_fields_avoiding([[0], [1]], [None, over]))
    refused(["257 zones"], lambda: e.closed_edges(over))
    for member, values in (("x", (np.nan, np.inf, -np.inf)), ("y", (np.nan, np.inf, -np.inf)),
                           ("r", (np.nan, np.inf, -np.inf, -1.0))):
        for v in values:
            bad = np.array([(1.0, 1.0, 0.5), (2.0, 2.0, 0.5)], F32)
            bad[1, "xyr".index(member)] = v
            refused([f"{member} of zone 1 of field 2"], lambda: e.cost_fields_avoiding([[0], [1], [2]], [None, None, bad]))
            refused([f"{member} of zone 1"], lambda: e.closed_edges(bad))
    # the raw entry: a zone_ptr that does not start at 0, and one that descends
    from trg_planner._engine import TrgZone, _i
    import ctypes as C
    z = np.ascontiguousarray(full[:4])
    ptr, ids = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    for zptr, words in (([1, 2, 3], "zone_ptr[0] is 1"), ([0, 3, 2], "descends at field 1")):
        zp = np.array(zptr, np.int32)
        st = e.L.trg_engine_cost_field_zones(e.h, 2, None, _i(zp), z.ctypes.data_as(C.POINTER(TrgZone)), _i(ptr), _i(ids),
                                             None, None, 0, None, None, None, None, None, 0, None, None, None, None, None,
                                             None, None)
        assert st == INVALID_ARG and words in e.L.trg_engine_last_error(e.h).decode()
    # the solve before the refusals is still retained and answers
    assert e.routes([0], [0])[0][2].num_nodes == 1
    # r == 0 is a point and -0 a radius
    e.cost_fields_avoiding([[0]], [[(1.0, 1.0, 0.0), (2.0, 2.0, -0.0)]])


# ---- routes, reached lists, plan_avoiding -------------------------------------------------------------------------
def test_routes_reached_and_plan_avoiding(engine, tmp_path):
    e = engine
    g = fg.lattice(9, 7)
    x = load_graph(e, g, tmp_path)
    pos = e.node_xyz()
    n = lambda ix, iy: iy * 9 + ix
    gap_low = [(4.0, float(iy), 0.3) for iy in range(1, 7)]   # a wall with a gap at the bottom row
    gap_high = [(4.0, float(iy), 0.3) for iy in range(0, 6)]  # ... at the top row
    shut = [(4.0, float(iy), 0.3) for iy in range(0, 7)]      # no gap
    on_goal = [(8.0, 3.0, 0.1)]
    zone_sets = [gap_low, gap_high, None, shut, on_goal]
    m = len(zone_sets)
    start, goal = n(0, 3), n(8, 3)
    sets = [[start]] * m
    models = [None] * m
    refs = _refs(x, pos, zone_sets, models, sets)
    assert [int(f.hops[goal]) for f in refs] == [14, 14, 8, -1, -1]
    _check(e, refs, zone_sets, models, sets, "routes: ", targets=[goal])
    pairs = [(k, t) for k in range(m) for t in (goal, n(3, 6), n(5, 0), start)]
    assert _check_routes(e, x, pos, refs, zone_sets, models, sets, pairs, "routes: ") == 3
    for k in range(m):
        ids, c, h = e.field_reached(k)
        assert np.array_equal(ids, np.flatnonzero(refs[k].hops >= 0)), k
        assert np.array_equal(bits(c), bits(refs[k].cost[ids])) and np.array_equal(h, refs[k].hops[ids]), k
    # plan_avoiding: one record per zone set, the routes of the solve above; under a model too
    for mo in (None, (0.5, np.inf)):
        refs = _refs(x, pos, zone_sets, [mo] * m, sets)
        got = e.plan_avoiding(pos[start, :2], pos[goal, :2], zone_sets, model=mo)
        assert [rec["found"] for rec in got] == [True, True, True, False, False]
        for k, rec in enumerate(got):
            if not rec["found"]:
                assert rec["ids"].size == 0 and np.isposinf(rec["cost"])
                continue
            w = _route_ref(x, pos, zone_sets[k], mo, refs[k], sets[k], goal)
            assert np.array_equal(rec["ids"], w.ids) and np.array_equal(bits(rec["xyz"]), bits(pos[w.ids])), k
            assert _b1(rec["cost"]) == _b1(w.cost) and _b1(rec["path_length"]) == _b1(w.path_length), k
            assert _b1(rec["avg_risk"]) == _b1(w.avg_risk), k
        late = e.plan_avoiding(pos[start, :2], pos[goal, :2], zone_sets, model=mo, early_exit=False)
        assert all(np.array_equal(a["ids"], b["ids"]) and _b1(a["cost"]) == _b1(b["cost"]) for a, b in zip(got, late))
    assert n(4, 0) in got[0]["ids"].tolist() and n(4, 6) in got[1]["ids"].tolist()


# ---- refresh ------------------------------------------------------------------------------------------------------
PAIRS = ("chain_cut", "chain_join", "random", "lattice", "plateau", "star", "invalid", "saturating_chain",
         "saturating_branch", "sets")


@pytest.fixture(scope="module")
def pairs():
    out = rp.all_pairs()
    out["sets"] = rp.set_pair()
    return out


def _pair_zones(name, p, among):
    """Two zone sets for the pair, from B's positions: zones on three of the nodes `among` (those B's plain field 0
    reaches beyond its sources, so that shutting one changes the field), and, where B has nodes A did not have, one on
    a new node."""
    rng = np.random.default_rng(len(name))
    pos = p.b.pos
    new = np.flatnonzero(p.new2old < 0)
    picks = rng.choice(among, size=3, replace=False)
    first = [(float(pos[v, 0]), float(pos[v, 1]), r) for v, r in zip(picks, (0.0, 0.6, 1.1))]
    second = [(float(pos[picks[0], 0]) + 0.5, float(pos[picks[0], 1]), 0.5)]
    if new.size:
        second.append((float(pos[new[0], 0]), float(pos[new[0], 1]), 0.4))
    return [np.array(first, F32), np.array(second, F32)]


@pytest.mark.parametrize("name", PAIRS)
def test_refresh_of_a_zone_solve(engine, tmp_path, pairs, name):
    """A retained zone solve on A through the pair's node map to B: bit-equal to a fresh zone solve on B and to the
    reference on B without the edges the zones close THERE."""
    e = engine
    e.set_option("field_delta_scale", "4")
    p = pairs[name]
    old_sets = [list(s) for s in p.sets] if p.sets else [[int(s)] for s in p.sources[:2]]
    first = {}
    for v, o in enumerate(p.new2old.tolist()):
        first.setdefault(o, v)
    sets = [[first[int(s)] for s in members] for members in old_sets]
    plain = _refs(p.b, p.b.pos, [None, None], [None, None], sets)
    zone_sets = _pair_zones(name, p, np.flatnonzero(plain[0].hops > 0))
    load_graph(e, p.a, tmp_path, "a")
    e.cost_fields_avoiding(old_sets, zone_sets)
    xb = load_graph(e, p.b, tmp_path, "b")
    pos = e.node_xyz()
    r = e.refresh_fields(new2old=p.new2old)
    assert r["sources"].tolist() == [s[0] for s in sets]
    if name == "random":  # a node B made lies inside a zone: shut in the refreshed field
        new = int(np.flatnonzero(p.new2old < 0)[0])
        assert zr.inside(xb, zone_sets[1], pos)[new] and r["hops"][1, new] == -1
    refs = _refs(xb, pos, zone_sets, [None, None], sets)
    assert refs[0].hops.tobytes() != plain[0].hops.tobytes(), "the zones change nothing on B"
    for who, got in (("refresh", r), ("fresh", e.cost_fields_avoiding(sets, zone_sets))):
        at = f"{name}, {who}: "
        assert_rows(at, "costs", got["cost"], np.stack([f.cost for f in refs]), as_bits=True)
        assert_rows(at, "hops", got["hops"], np.stack([f.hops for f in refs]))
        assert_rows(at, "parents", got["parent"], np.stack([f.parent for f in refs]))
        assert_rows(at, "owners", got["owner"], np.stack([f.owner for f in refs]))
        assert np.array_equal(got["reached"], [(f.hops >= 0).sum() for f in refs]), at


def test_refresh_refuses_a_bounded_zone_solve(engine, tmp_path, pairs):
    import trg_planner
    e = engine
    p = pairs["lattice"]
    x = load_graph(e, p.a, tmp_path)
    pos = e.node_xyz()
    zones = [np.array([(3.0, 3.0, 1.1)], F32)]
    refs = _refs(x, pos, zones, [None], [[0]])
    _check(e, refs, zones, [None], [[0]], "bounded: ", budget=6.0)
    with pytest.raises(trg_planner.TrgError) as ei:
        e.refresh_fields(new2old=rp.identity(p.a))
    assert ei.value.status == INVALID_ARG and "bounded" in str(ei.value)
    near = int(np.flatnonzero((refs[0].hops >= 0) & (refs[0].cost <= 6.0))[-1])
    _check_routes(e, x, pos, refs, zones, [None], [[0]], [(0, near)], "bounded, after the refusal: ")
    # start costs: refused too, still answering
    e.cost_fields_avoiding([[0]], zones, start_costs=[[0.5]])
    with pytest.raises(trg_planner.TrgError) as ei:
        e.refresh_fields(new2old=rp.identity(p.a))
    assert ei.value.status == INVALID_ARG and "start costs" in str(ei.value)
    assert e.routes([0], [0])[0][2].num_nodes == 1


# ---- one built graph, one large graph -----------------------------------------------------------------------------
def test_one_built_graph(mountain_gentle):
    """A graph the engine built from a cloud (the device build's own arrays and positions), a zone across it."""
    import trg_planner
    e = trg_planner.Engine(**MOUNTAIN)
    try:
        e.set_sampler(5, 16)
        e.set_global_map(mountain_gentle)
        e.init_graph([15.0, 15.0, 0.0])
        x = e.graph("global")
        pos = e.node_xyz()
        assert 1000 < x.V < 20000 and np.array_equal(bits(pos), bits(x.xyz))
        rng = np.random.default_rng(1)
        zones = np.concatenate([[(15.0, float(y), 0.8) for y in np.arange(5.0, 26.0, 1.0)],
                                _zones_near(rng, pos, 20, 2.0)]).astype(F32)
        closed, inside = _verdicts(e, x, pos, zones, "built graph: ")
        assert closed.sum() > 100 and inside.sum() > 10
        src = int(np.argmin(np.hypot(pos[:, 0] - 8.0, pos[:, 1] - 15.0)))
        refs = _refs(x, pos, [zones, None], [None, None], [[src], [src]])
        assert refs[0].cost.tobytes() != refs[1].cost.tobytes()
        far = int(np.argmin(np.hypot(pos[:, 0] - 22.0, pos[:, 1] - 15.0)))
        _check(e, refs, [zones, None], [None, None], [[src], [src]], "built graph: ", targets=[far])
        _check_routes(e, x, pos, refs, [zones, None], [None, None], [[src], [src]], [(0, far), (1, far)], "built graph: ")
    finally:
        e.close()


def test_random_large(engine, tmp_path):
    e = engine
    e.set_option("field_delta_scale", "4")
    g = random_large(*fg.RANDOM_LARGE[20000][0])
    x = load_graph(e, g, tmp_path)
    assert x.V == 20000
    pos = e.node_xyz()
    rng = np.random.default_rng(20000)
    # (this family's edges join nodes all over a 142 x 142 lattice: small discs already shut one edge in six)
    zone_sets = [_zones_near(rng, pos, 60, 0.4), _zones_near(rng, pos, 16, 1.0)]
    for z in zone_sets:
        closed, _ = _verdicts(e, x, pos, z, "random_large: ")
        assert 0 < closed.sum() < x.E
    valid = np.flatnonzero(x.state != fg.INVALID)
    sets = [[int(valid[0])], [int(valid[0]), int(valid[7])]]
    models = [None, _median_model(x)]
    refs = _refs(x, pos, zone_sets, models, sets)
    assert all((f.hops >= 0).sum() > 100 for f in refs)
    _check(e, refs, zone_sets, models, sets, "random_large: ", targets=[0, 19999, 10000])
