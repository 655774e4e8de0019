"""GPU: keep-out zones on risk fields (trg_engine_risk_field_zones; Engine.risk_fields_avoiding, safest_route_avoiding,
frontier_ceilings_avoiding, safest_frontier_avoiding, refresh_risk_fields; DESIGN.md section 2, "Keep-out zones on risk
fields").

Every comparison is exact: risk as bits, hops, parents, owners, `owned`, `reached`, bounds as bits, route ids and route
floats as bits, against tests/risk_zone_ref.py -- the existing risk references on zone_ref.pruned(), the graph WITHOUT
the edges the field's zone set closes (tests/test_risk_zone_ref_cpu.py holds that reference to an independent
definition on the CPU).  Positions are the engine's own (node_xyz()); nothing else expected comes from the engine.

Shapes: the smallest at which each piece can go wrong -- a 6 x 4 lattice whose geometry is exact in fp32, rows of 20
edges (two trips of a 16-lane group), a graph without edges, the hand-written risk cases, random graphs of 40 - 200
nodes with Invalid nodes, with one list for all fields (the plain RISK kernels on one slot) and a list per field (the
RISK MODELS kernels), 64 distinct lists and a 65th, the update pairs of the risk refresh tests, one map-built graph and
one random graph of 20 000 nodes."""
import ctypes as C

import numpy as np
import pytest

import bound_ref
import field_graphs as fg
import model_ref
import refresh_pairs as rp
import risk_graphs as rg
import risk_ref
import risk_refresh_pairs as rrp
import risk_zone_ref as rz
import route_ref
import set_ref
import zone_ref as zr
from field_support import (INVALID_ARG, MOUNTAIN, assert_rows, bits, engine, load_graph,  # noqa: F401
                           random_large, with_isolated_node)
from test_zone_ref_cpu import lattice_cases

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = F32(np.inf)
SF = MOUNTAIN["safety_factor"]
FAR = [(900.0, 900.0, 0.5)]  # a zone list that closes nothing on any test graph: the zoned kernels, the plain field


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """The compiled host Dijkstra of the risk field, once per module."""
    return risk_ref.compile_reference(tmp_path_factory.mktemp("risk_ref"))


def _b1(v):
    return int(np.float32(v).view(np.uint32))


def _zones_near(rng, pos, n, r_max=1.3):
    """n zones centred near nodes drawn at random (so that they shut something), radii 0 .. r_max."""
    at = pos[rng.integers(0, pos.shape[0], size=n), :2] + rng.uniform(-0.4, 0.4, size=(n, 2))
    return np.concatenate([at, rng.uniform(0.0, r_max, size=(n, 1))], axis=1).astype(F32)


def _refs(ref, x, pos, zone_sets, sets):
    """The reference field of every (zone set, set); equal (zone set, set) pairs are computed once."""
    done = {}
    out = []
    for zones, members in zip(zone_sets, sets):
        key = (zr.zones_of(zones).tobytes(), tuple(int(v) for v in members))
        if key not in done:
            done[key] = rz.zoned_field(ref, x, zones, members, pos)
        out.append(done[key])
    return out


def _check(e, refs, zone_sets, sets, at, budget=None, settle=None, targets=None, full=True):
    """One zoned risk solve against the (truncated) reference fields -> the engine's result."""
    m = len(sets)
    want = refs
    bounded = budget is not None or settle is not None
    if bounded:
        bud = np.full(m, INF, F32) if budget is None else np.broadcast_to(np.asarray(budget, F32).reshape(-1), (m,))
        want_bound = np.array([min(bud[k], bound_ref.settle_bound(refs[k].risk, refs[k].hops, targets, settle))
                               for k in range(m)], F32)
        want = [rz.truncate(refs[k], want_bound[k]) for k in range(m)]
    r = e.risk_fields_avoiding(sets, zone_sets, targets=targets, full=full, budget=budget, settle=settle)
    if bounded:
        assert np.array_equal(bits(r["bound"]), bits(want_bound)), at + f"bound {r['bound']!r} != {want_bound!r}"
    else:
        assert "bound" not in r
    stack = [np.stack([getattr(f, name) for f in want]) for name in ("risk", "hops", "parent", "owner")]
    assert np.array_equal(r["reached"], (stack[1] >= 0).sum(axis=1)), at + f"reached {r['reached']}"
    for k in range(m):
        assert np.array_equal(r["owned"][k], want[k].owned), at + f"owned of set {k}: {r['owned'][k]}"
    if full:
        assert_rows(at, "risks", r["risk"], stack[0], as_bits=True)
        assert_rows(at, "hops", r["hops"], stack[1])
        assert_rows(at, "parents", r["parent"], stack[2])
        assert_rows(at, "owners", r["owner"], stack[3])
    if targets is not None:
        t = np.asarray(targets, np.int64)
        assert np.array_equal(bits(r["risk_at"]), bits(stack[0][:, t])), at + "risk_at"
        assert np.array_equal(r["hops_at"], stack[1][:, t]), at + "hops_at"
        assert np.array_equal(r["owner_at"], stack[3][:, t]), at + "owner_at"
    return r


def _check_routes(e, x, pos, refs, zone_sets, sets, pairs, at):
    """Routes (field, target) of the retained solve against risk_zone_ref.route; no route edge is closed, and a route
    of a set solve starts at the member that owns the target -> the number of unreached targets."""
    got = e.routes([k for k, _ in pairs], [t for _, t in pairs])
    row = np.repeat(np.arange(x.V), np.diff(x.rowptr))
    unreached = 0
    for (k, t), (ids, pts, one) in zip(pairs, got):
        f = refs[k]
        where = at + f"field {k}, target {t}: "
        if f.hops[t] < 0:
            unreached += 1
            assert one.num_nodes == 0 and ids.size == 0 and np.isposinf(one.cost), where
            continue
        want_ids, edges, cost, length, avg = rz.route(x, zone_sets[k], f, t, pos)
        assert np.array_equal(ids, want_ids), where + f"ids {ids.tolist()} != {want_ids.tolist()}"
        assert one.num_nodes == len(want_ids) and ids[0] == sets[k][f.owner[t]], where
        assert np.array_equal(bits(pts), bits(pos[want_ids])), where
        assert _b1(one.cost) == _b1(cost) == _b1(f.risk[t]), where + "cost"
        assert _b1(one.path_length) == _b1(length) and _b1(one.avg_risk) == _b1(avg), where + "path_length, avg_risk"
        assert not zr.closed(x, zone_sets[k], pos)[edges].any() and np.array_equal(row[edges], ids[:-1]), where
    return unreached


# ---- exact geometry -----------------------------------------------------------------------------------------------
def test_exact_geometry_on_the_lattice(ref, engine, tmp_path):
    """A point on a node, a point on a midpoint, a tangent disc and the same disc one ulp smaller: every weight of the
    lattice is 0.25, so a closed link shows in the hops and parents."""
    e = engine
    x = load_graph(e, fg.lattice(6, 4), tmp_path)
    pos = e.node_xyz()
    n = lambda ix, iy: iy * 6 + ix
    cases = lattice_cases()
    names = ["point_on_a_node", "point_on_a_midpoint", "tangent", "just_short_of_tangent"]
    zone_sets = [cases[name][0] for name in names]
    sets = [[n(0, 0)], [n(2, 2)], [n(2, 1)], [n(2, 1)]]
    refs = _refs(ref, x, pos, zone_sets, sets)
    plain = _refs(ref, x, pos, [None] * 4, sets)
    assert refs[0].hops[n(2, 1)] == -1 and (refs[0].hops >= 0).sum() == 23
    assert refs[1].hops[n(3, 2)] == 3 and plain[1].hops[n(3, 2)] == 1
    assert refs[2].hops[n(3, 1)] == 3 and refs[2].parent[n(3, 1)] != n(2, 1)
    assert refs[3].hops.tobytes() == plain[3].hops.tobytes() and refs[3].parent.tobytes() == plain[3].parent.tobytes()
    _check(e, refs, zone_sets, sets, "lattice, a list per field: ", targets=[n(2, 1), n(3, 1), n(3, 2)])
    for k, name in enumerate(names):
        _check(e, refs[k:k + 1], zone_sets[k:k + 1], sets[k:k + 1], name + ": ")


# ---- rows ---------------------------------------------------------------------------------------------------------
def test_long_rows_no_edges_and_an_isolated_node(ref, engine, tmp_path):
    e = engine
    g = fg.star(40, hubs=2)
    x = load_graph(e, g, tmp_path, "star")
    assert np.diff(x.rowptr).max() >= 20 and x.V % 64 != 0
    pos = e.node_xyz()
    leaves = pos[2:42, :2]
    across = [(float(leaves[5:9, 0].mean()), float(leaves[5:9, 1].mean()), 1.2)]
    hub_rows = zr.closed(x, across, pos)[x.rowptr[0]:x.rowptr[2]]
    assert hub_rows.any() and not hub_rows.all()
    zone_sets, sets = [across, None, across], [[x.V - 1], [x.V - 1], [0, 1]]
    refs = _refs(ref, x, pos, zone_sets, sets)
    assert refs[0].hops.tobytes() != refs[1].hops.tobytes()
    _check(e, refs, zone_sets, sets, "star: ", targets=[2, 7, 41])
    _check(e, refs[:1], zone_sets[:1], sets[:1], "star, m 1: ")
    x = load_graph(e, fg.oddities()["no_edges"][0], tmp_path, "no_edges")
    pos = e.node_xyz()
    z = [(float(pos[3, 0]), float(pos[3, 1]), 0.5)]
    assert x.E == 0
    refs = _refs(ref, x, pos, [z, z], [[0], [3]])
    r = _check(e, refs, [z, z], [[0], [3]], "no edges: ", targets=[3])
    assert r["hops_at"][:, 0].tolist() == [-1, 0]
    g = with_isolated_node(rg.redrawn(7))
    x = load_graph(e, g, tmp_path, "isolated")
    pos = e.node_xyz()
    z = [(float(pos[-1, 0]), float(pos[-1, 1]), 0.25), (float(pos[1, 0]), float(pos[1, 1]), 0.3)]
    sets = [[x.V - 1], [int(np.flatnonzero(g.state != fg.INVALID)[2])]]
    refs = _refs(ref, x, pos, [z, z], sets)
    assert (refs[0].hops >= 0).sum() == 1 and (refs[1].hops >= 0).sum() > 1
    _check(e, refs, [z, z], sets, "an isolated node: ", targets=[x.V - 1, 1])


# ---- zone counts, refusals ----------------------------------------------------------------------------------------
def test_limits_and_refusals(ref, engine, tmp_path):
    import trg_planner
    from trg_planner._engine import TrgZone, _i
    e = engine
    x = load_graph(e, fg.lattice(6, 4), tmp_path)
    pos = e.node_xyz()
    rng = np.random.default_rng(5)
    full = _zones_near(rng, pos, 256, 0.3)
    refs = _refs(ref, x, pos, [full], [[0]])
    _check(e, refs, [full], [[0]], "256 zones: ")

    def refused(words, call):
        with pytest.raises(trg_planner.TrgError) as ei:
            call()
        msg = str(ei.value)
        assert ei.value.status == INVALID_ARG and "risk field zones: " in msg and all(w in msg for w in words), msg

    over = np.concatenate([full, full[:1]])
    refused(["field 1", "257 zones"], lambda: e.risk_fields_avoiding([[0], [1]], [None, over]))
    for member, values in (("x", (np.nan, np.inf, -np.inf)), ("y", (np.nan, np.inf, -np.inf)),
                           ("r", (np.nan, np.inf, -np.inf, -1.0))):
        for v in values:
            bad = np.array([(1.0, 1.0, 0.5), (2.0, 2.0, 0.5)], F32)
            bad[1, "xyr".index(member)] = v
            refused([f"{member} of zone 1 of field 2"], lambda: e.risk_fields_avoiding([[0], [1], [2]], [None, None, bad]))
    # the raw entry: a zone_ptr that does not start at 0, and one that descends
    z = np.ascontiguousarray(full[:4])
    ptr, ids = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    for zptr, words in (([1, 2, 3], "zone_ptr[0] is 1"), ([0, 3, 2], "descends at field 1")):
        zp = np.array(zptr, np.int32)
        st = e.L.trg_engine_risk_field_zones(e.h, 2, _i(zp), z.ctypes.data_as(C.POINTER(TrgZone)), _i(ptr), _i(ids),
                                             None, 0, None, None, None, None, None, 0, None, None, None, None, None,
                                             None, None)
        msg = e.L.trg_engine_last_error(e.h).decode()
        assert st == INVALID_ARG and msg.startswith("risk field zones: ") and words in msg, msg
    # the solve before the refusals is still retained and answers
    assert e.routes([0], [0])[0][2].num_nodes == 1
    # r == 0 is a point and -0 a radius
    e.risk_fields_avoiding([[0]], [[(1.0, 1.0, 0.0), (2.0, 2.0, -0.0)]])


def test_a_nan_weight_on_a_closed_edge_is_still_refused(engine, tmp_path):
    """The bad-weight flag stays over ALL edges: closing the edge that carries the NaN does not hide it."""
    import trg_planner
    e = engine
    g = rg.bad_weights()["nan"]
    p = tmp_path / "bad.json"
    fg.write_json(p, g)
    e.load_json(str(p))
    x = e.graph("global")
    pos = e.node_xyz()
    on_2 = [(float(pos[2, 0]), float(pos[2, 1]), 0.1)]
    closed = zr.closed(x, on_2, pos)
    assert np.isnan(x.w[closed]).any() and not np.isnan(x.w[~closed]).any()
    for zones in (on_2, [on_2, None]):
        with pytest.raises(trg_planner.TrgError) as ei:
            e.risk_fields_avoiding([0, 0] if len(zones) == 2 else [0], zones)
        assert ei.value.status == INVALID_ARG and "weight" in str(ei.value), str(ei.value)


# ---- the fields ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rg.cases()))
def test_hand_written_cases(ref, engine, tmp_path, name):
    e = engine
    g, sources = rg.cases()[name]
    x = load_graph(e, g, tmp_path)
    pos = e.node_xyz()
    rng = np.random.default_rng(len(name))
    one = _zones_near(rng, pos, 2, 0.6)
    per_field = [one, None, _zones_near(rng, pos, 1, 0.3)][:len(sources)]
    for scale in ("4", "1e-6", "inf"):
        e.set_option("field_delta_scale", scale)
        at = f"{name}, width {scale}: "
        for m in (1, len(sources)):
            sets = [[int(s)] for s in sources[:m]]
            _check(e, _refs(ref, x, pos, [one] * m, sets), [one] * m, sets, at + f"m {m}, one list: ")
            _check(e, _refs(ref, x, pos, [FAR] * m, sets), [FAR] * m, sets, at + f"m {m}, a list that closes nothing: ")
        sets = [[int(s)] for s in sources]
        _check(e, _refs(ref, x, pos, per_field, sets), per_field, sets, at + "a list per field: ",
               targets=list(range(x.V)))
    e.set_option("field_delta_scale", "4")


def _random(seed):
    """40 .. 200 nodes, Invalid ones among them, an isolated last node; odd seeds with weights from five levels."""
    rng = np.random.default_rng(700 + seed)
    g = fg.with_positions(fg.random_graph(rng, int(rng.integers(40, 201))))
    return with_isolated_node(rg.reweighted(g, seed) if seed % 2 else g)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_graphs(ref, engine, tmp_path, seed):
    """m = 1 and m = 5; one list for all fields and a list per field, two of them empty; full, at targets, under
    budgets and both settle modes; sets of several members with owners and `owned`."""
    e = engine
    g = _random(seed)
    x = load_graph(e, g, tmp_path)
    V = x.V
    assert 40 <= V <= 201 and (x.state == fg.INVALID).any()
    pos = e.node_xyz()
    rng = np.random.default_rng(seed)
    valid = np.flatnonzero(x.state != fg.INVALID)
    invalid = int(np.flatnonzero(x.state == fg.INVALID)[0])
    half = (V - 1) // 2 + 3  # ids from here on only link among themselves
    other = int(valid[valid >= half][0])
    sets = [[int(valid[0])], [int(valid[3]), int(valid[0]), invalid, int(valid[3])], [other, V - 1],
            [invalid], [int(valid[5]), other, int(valid[1])]]
    one = _zones_near(rng, pos, 5, 1.5)
    per_field = [_zones_near(rng, pos, 3, 2.0), None, _zones_near(rng, pos, 9, 1.0), np.empty((0, 3), F32), one]
    targets = [int(valid[0]), V - 1, V // 2, 3, other]
    differs = 0
    for what, zone_sets in (("one list", [one] * 5), ("a list per field", per_field)):
        refs = _refs(ref, x, pos, zone_sets, sets)
        plain = _refs(ref, x, pos, [None] * 5, sets)
        differs += sum(a.risk.tobytes() != b.risk.tobytes() or a.parent.tobytes() != b.parent.tobytes()
                       for a, b in zip(refs, plain))
        for scale in ("4", "1e-6", "inf"):
            e.set_option("field_delta_scale", scale)
            at = f"seed {seed}, {what}, width {scale}: "
            _check(e, refs, zone_sets, sets, at, targets=targets)
            _check(e, refs[:1], zone_sets[:1], sets[:1], at + "m 1: ", targets=targets)
        e.set_option("field_delta_scale", "4")
        at = f"seed {seed}, {what}: "
        _check(e, refs, zone_sets, sets, at + "at the targets: ", targets=targets, full=False)
        levels = np.unique(refs[0].risk[refs[0].hops > 0])
        mid = float(levels[levels.size // 2]) if levels.size else 0.0
        for budget, settle in ((mid, None), (0.0, None), (None, "any"), (None, "all"),
                               ([0.0, mid, 1e30, np.inf, 0.05], "any"), (mid, "all")):
            for m in (5, 1):
                _check(e, refs[:m], zone_sets[:m], sets[:m], at + f"m {m}, budget {budget}, settle {settle}: ",
                       budget=budget if m == 5 or np.ndim(budget) == 0 else budget[:1], settle=settle, targets=targets)
    assert differs >= 3, "the zones change too few fields of this seed"


def test_particular_cases(ref, engine, tmp_path):
    """On the 6 x 4 lattice: a member inside a zone keeps its key and reaches nothing; a target inside a zone is
    unreached; a wall of zones splits the graph; zone_sets=None and empty lists are risk_fields_from bit for bit."""
    e = engine
    x = load_graph(e, fg.lattice(6, 4), tmp_path)
    pos = e.node_xyz()
    n = lambda ix, iy: iy * 6 + ix
    on_source = [(0.0, 0.0, 0.25)]
    on_target = [(5.0, 3.0, 0.0)]
    wall = [(2.5, float(iy), 0.1) for iy in range(4)]
    zone_sets = [on_source, on_target, wall, [(9.0, 9.0, 0.5)], on_source]
    sets = [[n(0, 0), n(1, 1)], [n(0, 0)], [n(0, 0)], [n(0, 0)], [n(0, 0)]]
    refs = _refs(ref, x, pos, zone_sets, sets)
    assert refs[0].hops[n(0, 0)] == 0 and _b1(refs[0].risk[n(0, 0)]) == 0 and refs[0].owned.tolist() == [1, 23]
    assert refs[1].hops[n(5, 3)] == -1 and (refs[1].hops >= 0).sum() == 23
    assert (refs[2].hops >= 0).sum() == 12 and (refs[4].hops >= 0).sum() == 1
    r = _check(e, refs, zone_sets, sets, "particular: ", targets=[n(5, 3), n(0, 0), n(3, 0)])
    assert r["hops_at"][:, 0].tolist() == [6, -1, -1, 8, -1] and np.isposinf(r["risk_at"][1, 0])
    # settle "any" on a target the zone shuts never stops that field; the others stop at it
    r = _check(e, refs, zone_sets, sets, "particular, settle: ", targets=[n(5, 3)], settle="any")
    assert np.isposinf(r["bound"][1]) and np.isposinf(r["bound"][2]) and r["bound"][3] == refs[3].risk[n(5, 3)]
    # the same wall for every field: the plain RISK kernels on the one slot
    refs = _refs(ref, x, pos, [wall] * 2, sets[:2])
    _check(e, refs, [wall] * 2, sets[:2], "particular, one wall for both: ", targets=[n(5, 3)])
    # no zones: None (a null zone_ptr), an empty array, empty lists per field -- risk_fields_from on every output
    kw = dict(targets=[n(5, 3), 3], budget=[0.25, 100.0, 0.0, 100.0, 0.1])
    plain = e.risk_fields_from(sets, **kw)
    for none in (None, np.empty((0, 3), F32), [None, np.empty((0, 3)), None, None, None]):
        r = e.risk_fields_avoiding(sets, none, **kw)
        for key in ("risk", "hops", "parent", "owner", "risk_at", "hops_at", "owner_at", "reached", "bound", "sources"):
            assert np.array_equal(np.asarray(r[key]).view(np.uint32), np.asarray(plain[key]).view(np.uint32)), key
        assert all(np.array_equal(a, b) for a, b in zip(r["owned"], plain["owned"]))
    plain = e.risk_fields_from(sets, settle="all", targets=[n(5, 3), 3])
    r = e.risk_fields_avoiding(sets, None, settle="all", targets=[n(5, 3), 3])
    for key in ("risk", "hops", "parent", "owner", "risk_at", "hops_at", "owner_at", "reached", "bound"):
        assert np.array_equal(np.asarray(r[key]).view(np.uint32), np.asarray(plain[key]).view(np.uint32)), key


def test_all_zero_weights(ref, engine, tmp_path):
    """Every weight 0: the mean over the unclosed edges and the bucket width are 0, under one list and under three."""
    e = engine
    x = load_graph(e, rg.all_zero_weights(300), tmp_path)
    pos = e.node_xyz()
    rng = np.random.default_rng(300)
    one = _zones_near(rng, pos, 8, 2.0)
    per_field = [one, None, _zones_near(rng, pos, 30, 1.0)]
    sets = [[0], [299], [150, 7]]
    for scale in ("4", "inf"):
        e.set_option("field_delta_scale", scale)
        for zone_sets in ([one] * 3, per_field):
            refs = _refs(ref, x, pos, zone_sets, sets)
            assert all(not f.risk[f.hops >= 0].any() for f in refs) and refs[0].hops.min() == -1
            _check(e, refs, zone_sets, sets, f"zero weights, width {scale}: ", targets=[0, 150, 299])
            _check(e, refs[:1], zone_sets[:1], sets[:1], f"zero weights, width {scale}, m 1: ")
    e.set_option("field_delta_scale", "4")


# ---- routes and reached lists -------------------------------------------------------------------------------------
def test_routes_and_reached(ref, engine, tmp_path):
    e = engine
    x = load_graph(e, fg.lattice(9, 7), tmp_path, "lattice")
    pos = e.node_xyz()
    n = lambda ix, iy: iy * 9 + ix
    gap_low = [(4.0, float(iy), 0.3) for iy in range(1, 7)]   # a wall with a gap at the bottom row
    gap_high = [(4.0, float(iy), 0.3) for iy in range(0, 6)]  # ... at the top row
    shut = [(4.0, float(iy), 0.3) for iy in range(0, 7)]      # no gap
    zone_sets = [gap_low, gap_high, None, shut, [(8.0, 3.0, 0.1)]]
    m = len(zone_sets)
    start, goal = n(0, 3), n(8, 3)
    sets = [[start]] * m
    refs = _refs(ref, x, pos, zone_sets, sets)
    assert [int(f.hops[goal]) for f in refs] == [14, 14, 8, -1, -1]
    for full in (True, False):  # parents in the solve, and the late parent sweep of the first routes call
        _check(e, refs, zone_sets, sets, "routes: ", targets=[goal], full=full)
        pairs = [(k, t) for k in range(m) for t in (goal, n(3, 6), n(5, 0), start)]
        assert _check_routes(e, x, pos, refs, zone_sets, sets, pairs, "routes: ") == 3
    for k in range(m):
        ids, c, h = e.field_reached(k)
        assert np.array_equal(ids, np.flatnonzero(refs[k].hops >= 0)), k
        assert np.array_equal(bits(c), bits(refs[k].risk[ids])) and np.array_equal(h, refs[k].hops[ids]), k
    # one wall for all fields (one slot, the plain RISK route walk), single sources
    sets = [[start], [n(8, 6)]]
    refs = _refs(ref, x, pos, [gap_low] * 2, sets)
    _check(e, refs, [gap_low] * 2, sets, "routes, one list: ", full=False, targets=[goal])
    _check_routes(e, x, pos, refs, [gap_low] * 2, sets, [(0, goal), (1, start), (1, n(4, 0))], "routes, one list: ")
    # sets of several members on a random graph, a list per field
    g = _random(3)
    x = load_graph(e, g, tmp_path, "random")
    pos = e.node_xyz()
    valid = np.flatnonzero(x.state != fg.INVALID)
    rng = np.random.default_rng(33)
    zone_sets = [_zones_near(rng, pos, 4, 1.5), _zones_near(rng, pos, 4, 1.5), None]
    sets = [[int(valid[0]), int(valid[7])], [int(valid[2]), int(valid[9]), int(valid[4])], [int(valid[7]), int(valid[0])]]
    refs = _refs(ref, x, pos, zone_sets, sets)
    _check(e, refs, zone_sets, sets, "routes of sets: ")
    pairs = [(k, int(t)) for k in range(3) for t in range(0, x.V, 3)]
    unreached = _check_routes(e, x, pos, refs, zone_sets, sets, pairs, "routes of sets: ")
    assert 0 < unreached < len(pairs)
    ids, c, h = e.field_reached(1)
    assert np.array_equal(ids, np.flatnonzero(refs[1].hops >= 0)) and np.array_equal(bits(c), bits(refs[1].risk[ids]))


def test_route_edge_among_duplicates(ref, engine, tmp_path):
    """Duplicate edges share their ends, so a zone closes all of them or none: under a list that closes nothing the
    route edge is still decided by tightness and CSR order -- into node 1 the higher index (weight 0.2, dist 2; the
    lower index weighs 0.5 and is not tight), into node 2 the first of the two equal ones."""
    e = engine
    g, _ = rg.cases()["duplicates"]
    x = load_graph(e, g, tmp_path)
    pos = e.node_xyz()
    for zone_sets in ([FAR, FAR], [FAR, None]):
        sets = [[0], [1]]
        assert not zr.closed(x, FAR, pos).any()
        refs = _refs(ref, x, pos, zone_sets, sets)
        _check(e, refs, zone_sets, sets, "duplicates: ", full=False, targets=[3])
        _check_routes(e, x, pos, refs, zone_sets, sets, [(k, t) for k in range(2) for t in range(4)], "duplicates: ")
        assert rz.route(x, zone_sets[0], refs[0], 3, pos)[1] == [1, 3, 5]
        one = e.routes([0], [3], xyz=False)[0][2]
        assert one.path_length == F32(12.0) and one.cost == F32(0.4), (one.path_length, one.cost)


# ---- the cache ----------------------------------------------------------------------------------------------------
def test_64_lists_a_65th_and_one_bit_of_r(ref, engine, tmp_path):
    e = engine
    g = with_isolated_node(rg.redrawn(13))
    x = load_graph(e, g, tmp_path)
    pos = e.node_xyz()
    rng = np.random.default_rng(64)
    zone_sets = [_zones_near(rng, pos, 1 + k % 5) for k in range(65)]
    assert len({z.tobytes() for z in zone_sets}) == 65
    sets = [[(5 * k + 2) % x.V] for k in range(64)]
    refs = _refs(ref, x, pos, zone_sets[:64], sets)
    _check(e, refs, zone_sets[:64], sets, "64 lists: ", targets=[x.V - 1, 3])
    one = _refs(ref, x, pos, zone_sets[64:], sets[:1])
    _check(e, one, zone_sets[64:], sets[:1], "a 65th list: ")
    # a plain risk solve and a cost solve after them
    rr, rh, rp_ = risk_ref.reference_risks(ref, x, [s[0] for s in sets[:3]])
    r = e.risk_fields(source_ids=[s[0] for s in sets[:3]])
    assert_rows("plain risk after 65 lists: ", "risks", r["risk"], rr, as_bits=True)
    assert_rows("plain risk after 65 lists: ", "hops", r["hops"], rh)
    assert_rows("plain risk after 65 lists: ", "parents", r["parent"], rp_)
    plain = [set_ref.set_field(x, SF, s) for s in sets[:3]]
    r = e.cost_fields(source_ids=[s[0] for s in sets[:3]])
    assert_rows("plain cost after 65 lists: ", "costs", r["cost"], np.stack([f.cost for f in plain]), as_bits=True)
    assert_rows("plain cost after 65 lists: ", "hops", r["hops"], np.stack([f.hops for f in plain]))
    _check(e, refs, zone_sets[:64], sets, "64 lists again: ", full=False, targets=[0, 7])
    # a cost solve and a risk solve under the SAME lists, in turn: neither reads the other's slot
    three, sets3 = zone_sets[:3], sets[:3]
    cost_refs = [set_ref.set_field(zr.pruned(x, z, np.inf, pos), SF, s) for z, s in zip(three, sets3)]
    for turn in range(2):
        r = e.cost_fields_avoiding(sets3, three)
        assert_rows(f"cost under the lists, turn {turn}: ", "costs", r["cost"], np.stack([f.cost for f in cost_refs]),
                    as_bits=True)
        assert_rows(f"cost under the lists, turn {turn}: ", "parents", r["parent"], np.stack([f.parent for f in cost_refs]))
        _check(e, refs[:3], three, sets3, f"risk under the lists, turn {turn}: ")
    # two byte-equal lists beside one that differs in a single bit of r: the tangent zone of the lattice
    x = load_graph(e, fg.lattice(6, 4), tmp_path, "lattice")
    pos = e.node_xyz()
    tangent = np.array([(2.5, 1.25, 0.25)], F32)
    short = tangent.copy()
    short[0, 2] = np.nextafter(F32(0.25), F32(0.0))
    assert (tangent.view(np.uint32) != short.view(np.uint32)).sum() == 1
    three = [tangent, short, tangent.copy()]
    refs = _refs(ref, x, pos, three, [[8]] * 3)
    assert refs[0].hops[9] > refs[1].hops[9] and refs[0].hops.tobytes() == refs[2].hops.tobytes()
    _check(e, refs, three, [[8]] * 3, "one bit of r: ")


# ---- safest_route_avoiding, the frontier helpers ------------------------------------------------------------------
def _same_route(a, b, at):
    assert (a is None) == (b is None), at
    if a is None:
        return
    assert _b1(a[0]) == _b1(b[0]), at + f"{a[0]!r} != {b[0]!r}"
    assert a[1]["model"] == b[1]["model"] and a[1]["reachable"] == b[1]["reachable"], at
    assert np.array_equal(a[1]["ids"], b[1]["ids"]) and np.array_equal(bits(a[1]["xyz"]), bits(b[1]["xyz"])), at
    for key in ("cost", "path_length", "avg_risk"):
        assert _b1(a[1][key]) == _b1(b[1][key]), at + key


@pytest.mark.parametrize("seed", [1, 4])
def test_safest_route_avoiding(ref, engine, tmp_path, seed):
    """Against model_ref.min_ceiling on the pruned graph and the cost reference on the graph pruned by zones and that
    ceiling; an empty set against safest_route; a set that contains the goal, and one that cuts it off, give None."""
    e = engine
    e.set_option("field_delta_scale", "4")
    g = with_isolated_node(rg.redrawn(seed))
    x = load_graph(e, g, tmp_path)
    pos = e.node_xyz()
    valid = np.flatnonzero(x.state != fg.INVALID)
    rng = np.random.default_rng(seed)
    found = cut = 0
    for i in range(4):
        a, b = int(valid[(3 * i) % valid.size]), int(valid[(7 * i + 5) % valid.size])
        na, nb = (int(v) for v in e._resolve_nodes([g.pos[a, :2], g.pos[b, :2]]))
        if na == nb:
            continue
        zone_sets = [None, _zones_near(rng, pos, 2, 0.8), [(float(pos[nb, 0]), float(pos[nb, 1]), 0.0)],
                     _zones_near(rng, pos, 5, 1.0)]
        got = e.safest_route_avoiding(g.pos[a, :2], g.pos[b, :2], zone_sets)
        assert len(got) == 4 and got[2] is None
        _same_route(got[0], e.safest_route(g.pos[a, :2], g.pos[b, :2]), f"seed {seed}, {na} -> {nb}, no zones: ")
        _same_route(e.safest_route_avoiding(g.pos[a, :2], g.pos[b, :2], [np.empty((0, 3), F32)])[0], got[0], "alone: ")
        for k, zones in enumerate(zone_sets):
            at = f"seed {seed}, {na} -> {nb}, zone set {k}: "
            tau = model_ref.min_ceiling(rz.pruned(x, zones, pos), na, nb)
            assert (got[k] is None) == (tau is None), at
            if tau is None:
                cut += 1
                continue
            found += 1
            assert _b1(got[k][0]) == _b1(tau + F32(0.0)), at + f"{got[k][0]!r} != {tau!r}"
            p = zr.pruned(x, zones, tau, pos)
            f = set_ref.set_field(p, F32(SF), [na])
            w = route_ref.route(p.rowptr, p.col, p.w, p.dist, p.state, F32(SF), f.cost, f.hops, f.parent, na, nb)
            rec = got[k][1]
            assert rec["reachable"] and rec["model"] == (float(F32(SF)), float(tau)), at
            assert np.array_equal(rec["ids"], w.ids) and np.array_equal(bits(rec["xyz"]), bits(pos[w.ids])), at
            for key in ("cost", "path_length", "avg_risk"):
                assert _b1(rec[key]) == _b1(getattr(w, key)), at + key
            assert not zr.closed(x, zones, pos)[p.kept[w.edges]].any() and x.w[p.kept[w.edges]].max() <= tau, at
    assert found >= 4 and cut >= 3, (found, cut)
    # a wall that cuts the goal off
    x = load_graph(e, fg.lattice(6, 4), tmp_path, "lattice")
    pos = e.node_xyz()
    wall = [(2.5, float(iy), 0.1) for iy in range(4)]
    got = e.safest_route_avoiding(pos[0, :2], pos[23, :2], [wall, None, wall[1:]])
    assert got[0] is None and got[1] is not None and got[2] is not None
    assert got[1][1]["ids"].size == 9 and got[2][1]["ids"].size == 9 and 2 in got[2][1]["ids"].tolist()
    assert e.safest_route_avoiding(pos[0, :2], pos[23, :2], [wall]) == [None]


@pytest.mark.parametrize("seed", [0, 6])
def test_frontier_helpers_avoiding(ref, engine, tmp_path, seed):
    e = engine
    e.set_option("field_delta_scale", "4")
    g = with_isolated_node(rg.redrawn(seed))
    x = load_graph(e, g, tmp_path)
    pos = e.node_xyz()
    frontier = np.flatnonzero(x.state == 1).astype(np.int32)
    assert frontier.size
    valid = np.flatnonzero(x.state != fg.INVALID)
    rng = np.random.default_rng(seed)
    picked = shut = 0
    for a in (int(valid[0]), int(valid[3]), int(valid[-2]), x.V - 1):
        pose = g.pos[a, :2]
        src = int(e._resolve_nodes([pose])[0])
        on_frontier = [(float(pos[v, 0]), float(pos[v, 1]), 0.2) for v in frontier[:2] if v != src]
        for zones in (_zones_near(rng, pos, 3, 1.0), on_frontier, None):
            f = rz.zoned_field(ref, x, zones, [src], pos)
            ids, risk, hops = e.frontier_ceilings_avoiding(pose, zones)
            assert np.array_equal(ids, frontier)
            assert np.array_equal(bits(risk), bits(f.risk[frontier])) and np.array_equal(hops, f.hops[frontier])
            shut += int((f.hops[frontier] < 0).sum())
            got = e.safest_frontier_avoiding(pose, zones)
            ok = frontier[f.hops[frontier] >= 0]
            if ok.size == 0:
                assert got is None
                continue
            picked += 1
            best = int(ok[np.lexsort((ok, f.hops[ok], f.risk[ok]))[0]])
            assert got[0] == best and _b1(got[1]) == _b1(f.risk[best]), (got, best)
            assert got[2] == rz.route(x, zones, f, best, pos)[0].tolist()
        # the unzoned helpers, asked to reuse what is retained, do not take a zoned solve for their own
        e.frontier_ceilings_avoiding(pose, on_frontier)
        plain = rz.zoned_field(ref, x, None, [src], pos)
        _, risk, hops = e.frontier_ceilings(pose, reuse=True)
        assert np.array_equal(bits(risk), bits(plain.risk[frontier])) and np.array_equal(hops, plain.hops[frontier])
    assert picked >= 2 and shut >= 2, (picked, shut)


# ---- refresh ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    out = rrp.all_pairs()
    out["risk_sets"] = rrp.risk_sets_pair()
    return out


PAIRS = ("chain_cut", "chain_join", "random", "lattice", "invalid", "star", "risk_plateau", "levels", "peak_down",
         "peak_up", "duplicates_swapped", "risk_sets")


def test_the_pairs_are_all_of_them():
    assert set(PAIRS) == set(rrp.all_pairs()) | {"risk_sets"}


def _pair_zones(name, p, among):
    """Two zone lists for the pair, from B's positions: zones on up to three of the nodes `among` (those B's plain
    field 0 reaches beyond its sources, so that shutting one changes the field), and, where B has nodes A did not
    have, one on a new node."""
    rng = np.random.default_rng(len(name))
    pos = p.b.pos
    new = np.flatnonzero(p.new2old < 0)
    picks = rng.choice(among, size=min(3, among.size), replace=False)
    first = [(float(pos[v, 0]), float(pos[v, 1]), r) for v, r in zip(picks, (0.0, 0.6, 1.1))]
    second = [(float(pos[picks[0], 0]) + 0.5, float(pos[picks[0], 1]), 0.5)]
    if new.size:
        second.append((float(pos[new[0], 0]), float(pos[new[0], 1]), 0.4))
    return [np.array(first, F32), np.array(second, F32)]


@pytest.mark.parametrize("name", PAIRS)
def test_refresh_of_a_zoned_risk_solve(ref, engine, tmp_path, pairs, name):
    """A retained zoned risk solve on A through the pair's node map to B: bit-equal to a fresh zoned solve on B and to
    the reference on B without the edges the zones close THERE -- two fields under two lists (the RISK MODELS warm seed),
    then one field under one list."""
    e = engine
    e.set_option("field_delta_scale", "4")
    p = pairs[name]
    old_sets = [list(s) for s in p.sets] if p.sets else [[int(s)] for s in p.sources[:2]]
    first = {}
    for v, o in enumerate(p.new2old.tolist()):
        first.setdefault(o, v)
    sets = [[first[int(s)] for s in members] for members in old_sets]
    plain = _refs(ref, p.b, p.b.pos, [None, None], sets)
    zone_sets = _pair_zones(name, p, np.flatnonzero(plain[0].hops > 0))
    for m in (2, 1):
        load_graph(e, p.a, tmp_path, "a")
        e.risk_fields_avoiding(old_sets[:m], zone_sets[:m])
        xb = load_graph(e, p.b, tmp_path, "b")
        pos = e.node_xyz()
        r = e.refresh_risk_fields(new2old=p.new2old)
        assert r["sources"].tolist() == [s[0] for s in sets[:m]]
        refs = _refs(ref, xb, pos, zone_sets[:m], sets[:m])
        assert refs[0].hops.tobytes() != plain[0].hops.tobytes(), "the zones change nothing on B"
        for who, got in (("refresh", r), ("fresh", e.risk_fields_avoiding(sets[:m], zone_sets[:m]))):
            at = f"{name}, m {m}, {who}: "
            assert_rows(at, "risks", got["risk"], np.stack([f.risk for f in refs]), as_bits=True)
            assert_rows(at, "hops", got["hops"], np.stack([f.hops for f in refs]))
            assert_rows(at, "parents", got["parent"], np.stack([f.parent for f in refs]))
            assert_rows(at, "owners", got["owner"], np.stack([f.owner for f in refs]))
            assert np.array_equal(got["reached"], [(f.hops >= 0).sum() for f in refs]), at


def test_refresh_when_the_update_moves_a_node_into_a_zone(ref, engine, tmp_path):
    """B is A with one node moved: into a zone that held nothing on A.  The refreshed field shuts it, as the fresh
    zoned solve on B does; routes and the reached list answer under the zones on B's positions."""
    e = engine
    a = fg.lattice(6, 4)
    n = lambda ix, iy: iy * 6 + ix
    pos_b = a.pos.copy()
    pos_b[n(3, 1)] = (20.0, 20.0, 0.0)
    b = a._replace(pos=pos_b)
    zone_sets = [[(20.0, 20.0, 0.5)], [(20.0, 20.0, 0.5), (0.0, 3.0, 0.1)]]
    sets = [[n(0, 0)], [n(5, 3), n(0, 0)]]
    xa = load_graph(e, a, tmp_path, "a")
    on_a = _refs(ref, xa, e.node_xyz(), zone_sets, sets)
    assert on_a[0].hops[n(3, 1)] == 4 and not zr.inside(xa, zone_sets[0], e.node_xyz()).any()
    _check(e, on_a, zone_sets, sets, "before the move: ")
    xb = load_graph(e, b, tmp_path, "b")
    pos = e.node_xyz()
    assert zr.inside(xb, zone_sets[0], pos).tolist() == [v == n(3, 1) for v in range(24)]
    r = e.refresh_risk_fields(new2old=rp.identity(a))
    refs = _refs(ref, xb, pos, zone_sets, sets)
    assert refs[0].hops[n(3, 1)] == -1 and refs[1].hops[n(3, 1)] == -1 and refs[1].hops[n(0, 3)] == -1
    assert r["hops"][:, n(3, 1)].tolist() == [-1, -1]
    assert_rows("after the move: ", "risks", r["risk"], np.stack([f.risk for f in refs]), as_bits=True)
    assert_rows("after the move: ", "hops", r["hops"], np.stack([f.hops for f in refs]))
    assert_rows("after the move: ", "parents", r["parent"], np.stack([f.parent for f in refs]))
    assert_rows("after the move: ", "owners", r["owner"], np.stack([f.owner for f in refs]))
    pairs_ = [(k, t) for k in range(2) for t in (n(3, 1), n(4, 1), n(5, 0), n(0, 3))]
    assert _check_routes(e, xb, pos, refs, zone_sets, sets, pairs_, "after the move: ") == 3
    ids, c, h = e.field_reached(0)
    assert np.array_equal(ids, np.flatnonzero(refs[0].hops >= 0)) and n(3, 1) not in ids.tolist()


def test_refresh_refusals_are_unchanged(ref, engine, tmp_path, pairs):
    """A bounded zoned risk solve is refused and left answering; the cost refresh refuses a zoned risk solve and the risk
    refresh a zoned cost solve."""
    import trg_planner
    e = engine
    p = pairs["lattice"]
    x = load_graph(e, p.a, tmp_path)
    pos = e.node_xyz()
    zones = [np.array([(3.0, 3.0, 1.1)], F32)]
    refs = _refs(ref, x, pos, zones, [[0]])
    _check(e, refs, zones, [[0]], "bounded: ", budget=0.25)

    def refused(call, word):
        with pytest.raises(trg_planner.TrgError) as ei:
            call(new2old=rp.identity(p.a))
        assert ei.value.status == INVALID_ARG and word in str(ei.value), str(ei.value)

    refused(e.refresh_risk_fields, "bounded")
    near = int(np.flatnonzero(refs[0].hops > 0)[-1])
    _check_routes(e, x, pos, refs, zones, [[0]], [(0, near)], "bounded, after the refusal: ")
    _check(e, refs, zones, [[0]], "unbounded: ")
    refused(e.refresh_fields, "the retained solve is a risk field")
    e.cost_fields_avoiding([[0]], zones)
    refused(e.refresh_risk_fields, "the retained solve is a cost field")
    assert e.routes([0], [0])[0][2].num_nodes == 1


# ---- one built graph, one large graph -----------------------------------------------------------------------------
def test_one_built_graph(ref, mountain_gentle):
    """A graph the engine built from a cloud (the device build's own arrays and positions), a wall of zones across it."""
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
        assert zr.closed(x, zones, pos).sum() > 100
        src = int(np.argmin(np.hypot(pos[:, 0] - 8.0, pos[:, 1] - 15.0)))
        far = int(np.argmin(np.hypot(pos[:, 0] - 22.0, pos[:, 1] - 15.0)))
        for zone_sets in ([zones, None], [zones, zones]):
            refs = _refs(ref, x, pos, zone_sets, [[src], [src]])
            _check(e, refs, zone_sets, [[src], [src]], "built graph: ", targets=[far])
            _check_routes(e, x, pos, refs, zone_sets, [[src], [src]], [(0, far), (1, far)], "built graph: ")
        plain = _refs(ref, x, pos, [None], [[src]])[0]
        assert refs[0].risk.tobytes() != plain.risk.tobytes() or refs[0].hops.tobytes() != plain.hops.tobytes()
    finally:
        e.close()


def test_random_large(ref, engine, tmp_path):
    e = engine
    e.set_option("field_delta_scale", "4")
    g = rg.reweighted(random_large(*fg.RANDOM_LARGE[20000][0]), 20000)
    x = load_graph(e, g, tmp_path)
    assert x.V == 20000
    pos = e.node_xyz()
    rng = np.random.default_rng(20000)
    # (this family's edges join nodes all over a 142 x 142 lattice: small discs already shut one edge in six)
    zone_sets = [_zones_near(rng, pos, 60, 0.4), _zones_near(rng, pos, 16, 1.0)]
    for z in zone_sets:
        assert 0 < zr.closed(x, z, pos).sum() < x.E
    valid = np.flatnonzero(x.state != fg.INVALID)
    sets = [[int(valid[0])], [int(valid[0]), int(valid[7])]]
    refs = _refs(ref, x, pos, zone_sets, sets)
    assert all((f.hops >= 0).sum() > 100 for f in refs)
    _check(e, refs, zone_sets, sets, "random_large: ", targets=[0, 19999, 10000])
    same = _refs(ref, x, pos, zone_sets[:1] * 2, sets)
    _check(e, same, zone_sets[:1] * 2, sets, "random_large, one list: ", targets=[0, 19999, 10000])
