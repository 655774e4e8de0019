"""CPU: the keep-out zone rule as tests/zone_ref.py restates it ("Keep-out zones"), held to a
float64 point-to-segment distance before any GPU run; its symmetry and the inside-node guarantee; the exact lattice
cases the GPU test repeats on the device; the zone-list helper under the sanitizers; and the surface of the feature.

The float64 comparison leaves out the pairs whose float64 distance d lies within a relative 1e-5 of r.  Why the rule
must agree everywhere else, for the shapes drawn here: the inputs are float32, each difference (ax, ay, dx, dy) is one
rounding (relative u = 2^-24), each product one more, so cr = ax*dy - ay*dx is off by at most about 6u * |a| * L
(|a| the distance centre-to-P, L the edge length) and the perpendicular distance |cr| / L by about 6u * |a| = 3.6e-7 |a|;
the squares r*r, L2, cr*cr and r2*L2 add a few u relative.  Where the projection falls inside the edge and d is near r,
|a| <= sqrt(L^2 + r^2).  The geometric graphs have L <= 3 and r in [0.5, 3], so |a| <= 4.3 and the error is below
1.6e-6 <= 3.2e-6 r; the random_small graphs on their square lattice have |a| <= 10 and r in [1, 3], below 3.6e-6 r:
both inside 1e-5 r.  The end caps (da <= r2) are off by a few u relative, and a projection within rounding of an end
differs from that end's cap by the square of a rounding error."""
import os
import re
import subprocess

import numpy as np
import pytest

import field_graphs as fg
import zone_ref as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SEEDS = (0, 1, 2, 3, 4, 5)
LEFT_OUT_CAP = 0.01  # of the comparisons of one seed


def geometric(seed, V=300, reach=3.0, side=20.0):
    """V nodes uniform in a square, an edge (one way or both) between some of the pairs at most `reach` apart."""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([rng.uniform(0.0, side, size=(V, 2)), np.zeros((V, 1))], axis=1).astype(F32)
    d = np.hypot(pos[:, None, 0] - pos[None, :, 0], pos[:, None, 1] - pos[None, :, 1])
    a, b = np.nonzero((d <= reach) & (rng.random((V, V)) < 0.5) & ~np.eye(V, dtype=bool))
    n = a.shape[0]
    return fg.from_edges(V, a, b, rng.uniform(0.0, 1.0, n), d[a, b], pos=pos)


def zone_draw(rng, n, side, r_lo, r_hi):
    return np.stack([rng.uniform(0.0, side, n), rng.uniform(0.0, side, n), rng.uniform(r_lo, r_hi, n)],
                    axis=1).astype(F32)


def against_float64(g, zones):
    """-> (comparisons, left out): every (edge, zone) verdict of the rule against d <= r in float64."""
    u, v = zr.edge_ends(g)
    a, b = np.minimum(u, v), np.maximum(u, v)
    p = g.pos
    total = left = 0
    for x, y, r in zones:
        got = zr.closes(F32(x), F32(y), F32(r), p[a, 0], p[a, 1], p[b, 0], p[b, 1])
        d = zr.segment_distance64(x, y, p[a, 0], p[a, 1], p[b, 0], p[b, 1])
        near = np.abs(d - np.float64(r)) <= 1e-5 * np.float64(r)
        bad = np.flatnonzero(~near & (got != (d <= np.float64(r))))
        assert bad.size == 0, (float(x), float(y), float(r), int(u[bad[0]]), int(v[bad[0]]), float(d[bad[0]]))
        total += d.size
        left += int(near.sum())
    return total, left


@pytest.mark.parametrize("seed", SEEDS)
def test_rule_agrees_with_a_float64_distance(seed):
    rng = np.random.default_rng(1000 + seed)
    total, left = against_float64(geometric(seed), zone_draw(rng, 64, 20.0, 0.5, 3.0))
    g = fg.with_positions(fg.random_small(seed))
    side = float(g.pos[:, :2].max()) + 1.0
    t2, l2 = against_float64(g, zone_draw(rng, 64, side, 1.0, 3.0))
    total, left = total + t2, left + l2
    print(f"seed {seed}: {total} comparisons, {left} left out ({left / total:.2e})")
    assert total > 100000 and left <= LEFT_OUT_CAP * total, (total, left)


@pytest.mark.parametrize("seed", SEEDS)
def test_both_directions_one_verdict_and_inside_nodes_are_shut(seed):
    rng = np.random.default_rng(2000 + seed)
    for g, zones in ((geometric(seed, V=120), zone_draw(rng, 9, 20.0, 0.0, 4.0)),
                     (fg.with_positions(fg.random_small(seed)), zone_draw(rng, 5, 7.0, 0.0, 2.0))):
        closed, inside = zr.closed(g, zones), zr.inside(g, zones)
        u, v = zr.edge_ends(g)
        verdict = {}
        for a, b, c in zip(np.minimum(u, v).tolist(), np.maximum(u, v).tolist(), closed.tolist()):
            assert verdict.setdefault((a, b), c) == c, (a, b)
        assert inside.any() and closed.any() and not closed.all()
        assert closed[inside[u] | inside[v]].all()
        p = zr.pruned(g, zones)
        assert np.array_equal(p.kept, np.flatnonzero(~closed)) and p.rowptr[-1] == len(p.col) == (~closed).sum()
        assert not (inside[u[p.kept]] | inside[p.col]).any()


def lattice_cases():
    """name -> (zones, the undirected links (a, b) that must be closed): the exact cases on lattice(6, 4), whose unit
    spacing makes every value of the rule exact in fp32."""
    n = lambda ix, iy: iy * 6 + ix
    quarter = F32(0.25)
    return {
        "point_on_a_node": ([(2.0, 1.0, 0.0)], {tuple(sorted((n(2, 1), o))) for o in (n(1, 1), n(3, 1), n(2, 0), n(2, 2))}),
        "point_on_a_midpoint": ([(2.5, 2.0, 0.0)], {(n(2, 2), n(3, 2))}),
        "tangent": ([(2.5, 1.25, quarter)], {(n(2, 1), n(3, 1))}),
        "just_short_of_tangent": ([(2.5, 1.25, np.nextafter(quarter, F32(0.0)))], set()),
    }


def closed_links(g, closed):
    u, v = zr.edge_ends(g)
    return {(int(min(a, b)), int(max(a, b))) for a, b in zip(u[closed], v[closed])}


@pytest.mark.parametrize("name", sorted(lattice_cases()))
def test_exact_cases_on_the_lattice(name):
    g = fg.lattice(6, 4)
    zones, want = lattice_cases()[name]
    closed = zr.closed(g, zones)
    assert closed_links(g, closed) == want
    assert closed.sum() == 2 * len(want)  # both directions of every link
    assert zr.inside(g, zones).sum() == (1 if name == "point_on_a_node" else 0)


def test_a_nan_position_closes_nothing_and_no_zones_close_nothing():
    g = fg.lattice(3, 3)
    pos = g.pos.copy()
    pos[4, 0] = np.nan
    closed = zr.closed(g, [(1.0, 1.0, 0.75)], pos=pos)
    u, v = zr.edge_ends(g)
    assert not closed[(u == 4) | (v == 4)].any() and not zr.inside(g, [(1.0, 1.0, 0.75)], pos=pos)[4]
    assert zr.closed(g, [(1.0, 1.0, 0.75)])[(u == 4) | (v == 4)].all()
    assert not zr.closed(g, None).any() and not zr.closed(g, np.empty((0, 3))).any() and not zr.inside(g, None).any()


def test_zone_sets_helper_under_sanitizers(tmp_path):
    """trg-planner_amd/csrc/zone_sets.h -- the zone-list checks, the byte compare and the retained record -- in a
    stand-alone host program."""
    exe = tmp_path / "zone_sets_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "trg-planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "zone_sets_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "zone sets: ok" in out.stdout, out.stdout + out.stderr


def test_surface():
    """Fails without the feature: the entries, their declarations, the exports, the methods and the documents."""
    import inspect
    import trg_planner
    from trg_planner import _engine
    trg_planner.build_library()
    lib = trg_planner.load_library()
    with open(os.path.join(ROOT, "include", "trg_engine.h")) as f:
        header = f.read()
    for sym in ("trg_engine_cost_field_zones", "trg_engine_zone_edges"):
        assert hasattr(lib, sym) and sym in _engine.EXPORTS and re.search(r"\b" + sym + r"\s*\(", header), sym
    assert len(lib.trg_engine_cost_field_zones.argtypes) == len(lib.trg_engine_cost_field_seeded.argtypes) + 2
    assert "#define TRG_ZONES_MAX 256" in header and "typedef struct TrgZone" in header
    assert _engine.TRG_ZONES_MAX == zr.ZONES_MAX == 256
    assert [n for n, _ in _engine.TrgZone._fields_] == ["x", "y", "r"]
    E = _engine.Engine
    p = inspect.signature(E.cost_fields_avoiding).parameters
    assert list(p)[1:] == ["sets_or_sources", "zone_sets", "models", "start_costs", "targets", "full", "budget", "settle"]
    assert [p[k].default for k in list(p)[3:]] == [None, None, None, True, None, None]
    p = inspect.signature(E.plan_avoiding).parameters
    assert list(p)[1:] == ["start_xy", "goal_xy", "zone_sets", "model", "early_exit"]
    assert list(inspect.signature(E.closed_edges).parameters)[1:] == ["zones"]
    for doc in ("README.md", "DESIGN.md"):
        with open(os.path.join(ROOT, doc)) as f:
            assert "plan_avoiding" in f.read(), doc
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "**Keep-out zones** (`trg_engine_cost_field_zones`" in f.read()
