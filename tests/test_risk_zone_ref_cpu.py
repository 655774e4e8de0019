"""CPU: the reference of the zoned risk fields (tests/risk_zone_ref.py: the existing risk references on
zone_ref.pruned()) held to a definition that shares nothing with it but the zone rule ("Keep-out
zones on risk fields"), before any GPU run; and the surface of the feature.

The independent definition: with the distinct risks r = w + 0 of the relaxable, unclosed edges in ascending order,
risk[v] is the FIRST threshold t at which v is reached from the members by a breadth-first search over relaxable,
unclosed edges with r <= t (a member's is +0); hops[v] is the breadth-first depth of v in the subgraph of tight edges --
relaxable, unclosed, max(risk[u], r) == risk[v] -- from the members.  It never builds a pruned graph: the closed edges
are a mask over g's own CSR.  Everything is exact: max never rounds."""
import inspect
import os
import re

import numpy as np
import pytest

import field_graphs as fg
import risk_graphs as rg
import risk_ref
import risk_zone_ref as rz
import zone_ref as zr
from field_keys import relaxable, risk_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SEEDS = range(12)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return risk_ref.compile_reference(tmp_path_factory.mktemp("risk_ref"))


def _bfs(V, u, v, members, risk=None):
    """Breadth-first depths from `members` over the edges (u, v) -> depth per node, -1 unreached."""
    rows = [[] for _ in range(V)]
    for a, b in zip(u.tolist(), v.tolist()):
        rows[a].append(b)
    depth = np.full(V, -1, np.int32)
    level = sorted({int(s) for s in members})
    depth[level] = 0
    d = 0
    while level:
        d += 1
        nxt = []
        for a in level:
            for b in rows[a]:
                if depth[b] < 0:
                    depth[b] = d
                    nxt.append(b)
        level = nxt
    return depth


def by_thresholds(g, zones, members):
    """The definition of the module's docstring -> (risk float32, hops int32)."""
    V = len(g.state)
    u, v = zr.edge_ends(g)
    open_ = relaxable(g.col, g.state) & ~zr.closed(g, zones)
    u, v, r = u[open_], v[open_], risk_values(g.w)[open_]
    risk = np.full(V, np.inf, F32)
    risk[list(members)] = F32(0.0)
    left = ~np.isfinite(risk)
    for t in np.unique(r).tolist():
        if not left.any():
            break
        use = r <= F32(t)
        reached = _bfs(V, u[use], v[use], members) >= 0
        risk[left & reached] = F32(t)
        left &= ~reached
    keyed = np.isfinite(risk)
    tight = keyed[u] & (np.where(r > risk[u], r, risk[u]) == risk[v])
    return risk, _bfs(V, u[tight], v[tight], members)


def _zones(rng, g, n, r_max):
    at = g.pos[rng.integers(0, len(g.state), size=n), :2] + rng.uniform(-0.4, 0.4, size=(n, 2))
    return np.concatenate([at, rng.uniform(0.0, r_max, size=(n, 1))], axis=1).astype(F32)


def _graph(seed):
    """40 .. 200 nodes with Invalid ones among them: the random family as it is (even seeds) and with its weights redrawn
    from five levels (odd seeds: plateaus of equal risk)."""
    rng = np.random.default_rng(500 + seed)
    V = int(rng.integers(40, 201))
    g = fg.with_positions(fg.random_graph(rng, V))
    return rg.reweighted(g, seed) if seed % 2 else g


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_equals_the_threshold_definition(ref, seed):
    g = _graph(seed)
    V = len(g.state)
    assert 40 <= V <= 200 and (g.state == fg.INVALID).any()
    rng = np.random.default_rng(seed)
    valid = np.flatnonzero(g.state != fg.INVALID)
    bites = 0
    for zones in (_zones(rng, g, 3, 2.0), _zones(rng, g, 12, 1.2), None):
        for members in ([int(valid[0])], [int(valid[-1]), int(valid[1]), int(valid[-1])],
                        [int(np.flatnonzero(g.state == fg.INVALID)[0]), int(valid[2])]):
            at = f"seed {seed}, {0 if zones is None else len(zones)} zones, members {members}: "
            f = rz.zoned_field(ref, g, zones, members)
            risk, hops = by_thresholds(g, zones, members)
            assert np.array_equal(f.risk.view(np.uint32), risk.view(np.uint32)), at + "risk"
            assert np.array_equal(f.hops, hops), at + "hops"
            assert np.array_equal((f.hops >= 0), np.isfinite(f.risk)), at
            if zones is not None:
                plain = rz.zoned_field(ref, g, None, members)
                bites += f.risk.tobytes() != plain.risk.tobytes()
                inside = zr.inside(g, zones)
                inside[members] = False  # (members are exempt; everything else inside a zone is shut)
                assert (f.hops[inside] == -1).all(), at + "a node inside a zone has a key"
    assert bites >= 2, f"seed {seed}: the zones change no field"


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_compiled_reference_equals_the_restated_definition_on_the_pruned_graph(ref, seed):
    """risk_ref.py_risk_field (Bellman-Ford on max, BFS over tight edges, smallest parent) on the pruned graph: parents
    too, and the owners that follow from them."""
    g = _graph(seed)
    rng = np.random.default_rng(100 + seed)
    valid = np.flatnonzero(g.state != fg.INVALID)
    zones = _zones(rng, g, 6, 1.5)
    members = [int(valid[0]), int(valid[len(valid) // 2])]
    f = rz.zoned_field(ref, g, zones, members)
    risk, hops, parent = rz.definition_field(g, zones, members)
    assert np.array_equal(f.risk.view(np.uint32), risk.view(np.uint32))
    assert np.array_equal(f.hops, hops) and np.array_equal(f.parent, parent)
    assert f.owned.sum() == (f.hops >= 0).sum() and (f.owner[f.hops >= 0] >= 0).all()
    # a route of it uses no closed edge, and its edges are g's
    closed = zr.closed(g, zones)
    row = np.repeat(np.arange(len(g.state)), np.diff(g.rowptr))
    far = int(np.argmax(f.hops))
    ids, edges, cost, _, _ = rz.route(g, zones, f, far)
    assert len(ids) == f.hops[far] + 1 and not closed[edges].any()
    assert np.array_equal(row[edges], ids[:-1]) and np.array_equal(g.col[edges], ids[1:])
    assert F32(cost).view(np.uint32) == f.risk[far].view(np.uint32)


def test_members_and_targets_inside_a_zone():
    """On the 6 x 4 lattice: a member inside a zone keeps (+0, 0) and reaches nothing; a target inside one is
    unreached; a wall splits the graph."""
    g = fg.lattice(6, 4)
    n = lambda ix, iy: iy * 6 + ix
    risk, hops = by_thresholds(g, [(0.0, 0.0, 0.25)], [n(0, 0), n(1, 1)])
    assert hops[n(0, 0)] == 0 and risk[n(0, 0)].view(np.uint32) == 0 and (hops >= 0).sum() == 24
    risk, hops = by_thresholds(g, [(0.0, 0.0, 0.25)], [n(0, 0)])
    assert (hops >= 0).sum() == 1
    risk, hops = by_thresholds(g, [(5.0, 3.0, 0.0)], [n(0, 0)])
    assert hops[n(5, 3)] == -1 and np.isposinf(risk[n(5, 3)]) and (hops >= 0).sum() == 23
    risk, hops = by_thresholds(g, [(2.5, float(iy), 0.1) for iy in range(4)], [n(0, 0)])
    assert (hops >= 0).sum() == 12


def test_surface():
    """Fails without the feature: the entry, its declaration, the export, the methods and the documents."""
    import trg_planner
    from trg_planner import _engine
    trg_planner.build_library()
    lib = trg_planner.load_library()
    with open(os.path.join(ROOT, "include", "trg_engine.h")) as f:
        header = f.read()
    sym = "trg_engine_risk_field_zones"
    assert re.search(r"\bTrgStatus\s+" + sym + r"\s*\(", header), "the header does not declare " + sym
    assert sym in _engine.EXPORTS and hasattr(lib, sym)
    assert len(lib.trg_engine_risk_field_zones.argtypes) == len(lib.trg_engine_risk_field_sets.argtypes) + 2
    E = _engine.Engine
    p = inspect.signature(E.risk_fields_avoiding).parameters
    assert list(p)[1:] == ["sets_or_sources", "zone_sets", "targets", "full", "budget", "settle"]
    assert [p[k].default for k in list(p)[3:]] == [None, True, None, None]
    assert list(inspect.signature(E.safest_route_avoiding).parameters)[1:] == ["start_xy", "goal_xy", "zone_sets"]
    assert list(inspect.signature(E.frontier_ceilings_avoiding).parameters)[1:] == ["pose_xy", "zones"]
    assert list(inspect.signature(E.safest_frontier_avoiding).parameters)[1:] == ["pose_xy", "zones"]
    assert list(inspect.signature(E.refresh_risk_fields).parameters)[1:] == ["new2old", "targets", "full"]
    for doc in ("README.md", "DESIGN.md"):
        with open(os.path.join(ROOT, doc)) as f:
            assert "safest_route_avoiding" in f.read(), doc
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "**Keep-out zones on risk fields** (`trg_engine_risk_field_zones`" in f.read()
