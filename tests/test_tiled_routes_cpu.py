"""CPU: the protocol of the routes across tiles (tests/tiled_route_ref.py: LEN records and clipped offsets, per-rank
walks over the solve graphs, HANDOFF records with carried fp32 sums, END records, the exchange count) must equal the
definition of a route on the UNCUT graph (tests/route_ref.py) bit for bit -- the claim of DESIGN.md section 7, "Routes
across tiles", pinned before any GPU run.  Also the C and Python surface of the feature, and tiled.join_routes."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import field_ref
import seed_ref
import tiled_ref as tr
import tiled_route_ref as trr
from tiled_support import cuts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SF = 3.0


def bits(x):
    return np.asarray(x, F32).reshape(-1).view(np.uint32)


def check(G, offsets, cost, hops, parent, targets, owner=None, cap=None):
    """protocol == definition for the routes of one field; -> (reference routes, protocol result)"""
    want = trr.reference_routes(G, SF, cost, hops, parent, targets)
    got = trr.tiled_routes(G, offsets, SF, cost, hops, parent, targets, owner=owner, cap=cap)
    at = f"offsets {np.asarray(offsets).tolist()}: "
    lengths = [len(w.ids) for w in want]
    assert np.array_equal(got["offsets"], trr.clipped_offsets(lengths, sum(lengths) if cap is None else cap)), at
    tile_of = lambda g: np.searchsorted(offsets, g, side="right") - 1  # noqa: E731
    for t, part in enumerate(got["parts"]):  # a rank fills its own nodes' positions and nothing else
        assert (tile_of(part[part >= 0]) == t).all(), at + f"rank {t} wrote another rank's node"
    for r, (w, ids, info) in enumerate(zip(want, trr.join(got), got["infos"])):
        room = int(got["offsets"][r + 1] - got["offsets"][r])
        assert ids.tolist() == w.ids[:room].tolist(), at + f"route {r} to {targets[r]}"
        assert info[0] == len(w.ids), at + f"route {r}: num_nodes"
        for name, x, y in (("cost", info[1], w.cost), ("path_length", info[2], w.path_length),
                           ("avg_risk", info[3], w.avg_risk)):
            assert bits(x)[0] == bits(y)[0], at + f"route {r}: {name} {x!r} != {y!r}"
        assert info[4] == (int(w.ids[0]) if len(w.ids) else -1), at + f"route {r}: root"
    most = max([trr.crossings(offsets, w) for w in want if len(w.ids)], default=None)
    assert got["exchanges"] == (2 if most is None else most + 3), (at, got["exchanges"], most)
    return want, got


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("R", [2, 3, 4])
def test_protocol_equals_the_uncut_definition(seed, R):
    rng = np.random.default_rng(3000 * R + seed)
    V = int(rng.integers(60, 241)) if seed else 40
    G = tr.symmetric_graph(rng, V)
    offsets = cuts(rng, V, R, empty=seed % 3 == 1 and R > 2)
    valid = np.flatnonzero(G["state"] != tr.INVALID)
    crossing = handoffs = 0
    for src in (int(valid[0]), int(valid[len(valid) // 2]), int(np.flatnonzero(G["state"] == tr.INVALID)[0])):
        with np.errstate(over="ignore"):
            cost, hops, parent = field_ref.py_field(V, G["rowptr"], G["col"], G["w"], G["dist"], G["state"], SF, src)
        targets = [src] + rng.integers(0, V, 24).tolist() + np.flatnonzero(hops < 0)[:2].tolist()
        want, got = check(G, offsets, cost, hops, parent, targets)
        crossing += sum(trr.crossings(offsets, w) for w in want)
        handoffs += sum(1 for ex in got["records"] for rec in ex if rec[0] == "HANDOFF")
        check(G, offsets, cost, hops, parent, targets, cap=sum(len(w.ids) for w in want) // 2)  # clipped alike
    assert crossing > 0 and handoffs == crossing, (crossing, handoffs)  # one HANDOFF per seam crossing, carried sums


def lattice(nx, ny, tile):
    """unit-length edges on an nx x ny lattice whose cells go to ranges by tile(x, y) -> (G, offsets, gid)"""
    cells = sorted((tile(x, y), y, x) for x in range(nx) for y in range(ny))
    gid = {(x, y): i for i, (_, y, x) in enumerate(cells)}
    R = max(c[0] for c in cells) + 1
    sizes = [sum(1 for c in cells if c[0] == t) for t in range(R)]
    pairs = [(gid[x, y], gid[x + 1, y]) for x in range(nx - 1) for y in range(ny)] + \
            [(gid[x, y], gid[x, y + 1]) for x in range(nx) for y in range(ny - 1)]
    src = np.array([a for a, b in pairs] + [b for a, b in pairs])
    dst = np.array([b for a, b in pairs] + [a for a, b in pairs])
    order = np.lexsort((dst, src))
    V = nx * ny
    G = dict(V=V, rowptr=np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))]).astype(np.int64),
             col=dst[order].astype(np.int64), w=np.full(len(src), 0.25, F32), dist=np.ones(len(src), F32),
             state=np.zeros(V, np.int32))
    return G, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), gid


def test_exact_ties_across_seams_and_a_route_that_reenters_a_range():
    """Unit costs on a lattice in three diagonal stripes: nearly every node has several tight predecessors, in its own
    range and in others; the route follows the least global id, in and out of a range more than once."""
    G, offsets, gid = lattice(12, 9, lambda x, y: (x // 2 + y) % 3)
    V = G["V"]
    cost, hops, parent = field_ref.py_field(V, G["rowptr"], G["col"], G["w"], G["dist"], G["state"], SF, gid[0, 0])
    tile_of = np.searchsorted(offsets, np.arange(V), side="right") - 1
    tied = sum(1 for v in range(V) if len({int(tile_of[u]) for u in G["col"][G["rowptr"][v]:G["rowptr"][v + 1]]
                                             if hops[u] + 1 == hops[v]}) > 1)
    assert tied > 20, tied  # the precondition: tight predecessors on both sides of a seam
    want, got = check(G, offsets, cost, hops, parent, list(range(V)))
    assert sum(trr.reenters(offsets, w) for w in want) > 10
    assert max(trr.crossings(offsets, w) for w in want) >= 4


def test_a_range_without_nodes_and_the_chain_that_alternates():
    """64 nodes in a chain whose neighbours lie in different ranges, the range between them empty: 63 crossings, 66
    exchanges; target == source is one node and zero sums."""
    gidf = lambda p: (p % 2) * 32 + p // 2  # noqa: E731
    pairs = [(gidf(p), gidf(p + 1), F32(0.1 * (p % 3)), F32(0.5 + 0.01 * (p % 7))) for p in range(63)]
    src = np.array([a for a, b, _, _ in pairs] + [b for a, b, _, _ in pairs])
    dst = np.array([b for a, b, _, _ in pairs] + [a for a, b, _, _ in pairs])
    w = np.array([x for _, _, x, _ in pairs] * 2, F32)
    d = np.array([x for _, _, _, x in pairs] * 2, F32)
    order = np.lexsort((dst, src))
    G = dict(V=64, rowptr=np.concatenate([[0], np.cumsum(np.bincount(src, minlength=64))]).astype(np.int64),
             col=dst[order].astype(np.int64), w=w[order], dist=d[order], state=np.zeros(64, np.int32))
    offsets = np.array([0, 32, 32, 64], np.int64)
    cost, hops, parent = field_ref.py_field(64, G["rowptr"], G["col"], G["w"], G["dist"], G["state"], SF, gidf(0))
    want, got = check(G, offsets, cost, hops, parent, [gidf(63), gidf(0), gidf(17)])
    assert trr.crossings(offsets, want[0]) == 63 and got["exchanges"] == 66
    assert got["infos"][1][:4] == (1, F32(0.0), F32(0.0), F32(0.0)) and got["infos"][1][4] == gidf(0)
    assert (got["parts"][1] == -1).all()  # the empty range fills nothing


def test_set_fields_with_start_costs():
    """A route of a set field starts at the owner's root; cost carries the start cost, path_length does not."""
    rng = np.random.default_rng(77)
    G = tr.symmetric_graph(rng, 150)
    offsets = np.array([0, 40, 95, 150], np.int64)
    valid = np.flatnonzero(G["state"] != tr.INVALID)
    mem = [int(valid[3]), int(valid[60]), int(valid[120]), int(np.flatnonzero(G["state"] == tr.INVALID)[0])]
    c0 = np.array([0.5, 0.0, 1.25, 0.75], F32)
    with np.errstate(over="ignore"):
        f = seed_ref.seeded_field(SimpleNamespace(**G), SF, mem, c0)
    targets = np.flatnonzero(f.hops >= 0)[::3].tolist() + mem
    want, got = check(G, offsets, f.cost, f.hops, f.parent, targets, owner=f.owner)
    for w, info, t in zip(want, got["infos"], targets):
        assert info[5] == f.owner[t] and mem[info[5]] == info[4] == w.ids[0]
        assert f.hops[info[4]] == 0 and bits(f.cost[info[4]])[0] == bits(c0[info[5]])[0]
    assert len({i[5] for i in got["infos"]}) >= 3  # routes from several roots, one of them behind a start cost


def test_surface():
    """Fails without the feature: the entry, its declaration, the info structs and the Python methods."""
    import trg_planner
    from trg_planner import _engine, tiled
    trg_planner.build_library()
    lib = trg_planner.load_library()
    header = open(os.path.join(ROOT, "include", "trg_engine.h")).read()
    sym = "trg_engine_tiled_field_routes"
    assert hasattr(lib, sym) and sym in _engine.EXPORTS and re.search(r"\b" + sym + r"\s*\(", header), sym
    for struct, cls in (("TrgTiledRouteInfo", _engine.TrgTiledRouteInfo), ("TrgTiledRoutesInfo", _engine.TrgTiledRoutesInfo)):
        m = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, re.S)
        assert m, f"include/trg_engine.h does not define {struct}"
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        names = [n.strip() for decl in body.split(";") if decl.strip()
                 for n in re.sub(r"\b(int32_t|int64_t|float)\b", "", decl).split(",")]
        assert names == [n for n, _ in cls._fields_], (struct, names)
    assert [n for n, _ in _engine.TrgTiledRouteInfo._fields_] == ["num_nodes", "cost", "path_length", "avg_risk",
                                                                  "root_gid", "owner"]
    assert list(inspect.signature(_engine.Engine.tiled_routes).parameters)[1:] == ["route_field", "target_gids", "cap", "xyz"]
    assert list(inspect.signature(_engine.Engine.tiled_plan_many).parameters)[1:] == ["start_gid", "goal_gids"]
    assert list(inspect.signature(tiled.join_routes).parameters) == ["parts"]
    assert callable(tiled.field_route)  # (the host walk stays, as the reference)
    for doc in ("README.md", "DESIGN.md", os.path.join("include", "trg_engine.h")):
        text = open(os.path.join(ROOT, doc)).read()
        assert not re.search(r"device-side\s+routes\s+are\s+not\s+offered", text), doc
        assert "Routes across tiles" in text, doc


def test_join_routes_on_host_parts():
    """join_routes merges the ranks' positions and raises where a position is claimed twice or by nobody, or where the
    ranks disagree."""
    from trg_planner import tiled
    from trg_planner._engine import TrgTiledRouteInfo
    infos = lambda: [TrgTiledRouteInfo(3, 1.5, 2.0, 0.25, 4, -1), TrgTiledRouteInfo(0, np.inf, 0.0, 0.0, -1, -1),  # noqa: E731
                     TrgTiledRouteInfo(2, 0.5, 1.0, 0.0, 9, -1)]
    off = np.array([0, 3, 3, 5], np.int32)
    nan = np.nan
    a = dict(offsets=off, infos=infos(), gids=np.array([4, -1, 6, -1, -1], np.int32),
             xyz=np.array([[1, 1, 1], [nan] * 3, [3, 3, 3], [nan] * 3, [nan] * 3], np.float32))
    b = dict(offsets=off.copy(), infos=infos(), gids=np.array([-1, 12, -1, 9, 10], np.int32),
             xyz=np.array([[nan] * 3, [2, 2, 2], [nan] * 3, [4, 4, 4], [5, 5, 5]], np.float32))
    got = tiled.join_routes([a, b])
    assert [g[0].tolist() for g in got] == [[4, 12, 6], [], [9, 10]]  # (route 0 leaves rank 0 and comes back)
    assert got[0][1].tolist() == [[1, 1, 1], [2, 2, 2], [3, 3, 3]] and got[2][2].root_gid == 9
    twice = dict(b, gids=np.array([4, 12, -1, 9, 10], np.int32))
    with pytest.raises(ValueError, match="claimed by two ranks"):
        tiled.join_routes([a, twice])
    nobody = dict(b, gids=np.array([-1, -1, -1, 9, 10], np.int32))
    with pytest.raises(ValueError, match="claimed by no rank"):
        tiled.join_routes([a, nobody])
    with pytest.raises(ValueError, match="different offsets or infos"):
        tiled.join_routes([a, dict(b, offsets=np.array([0, 3, 3, 4], np.int32))])
    other = infos()
    other[0].path_length = 2.5
    with pytest.raises(ValueError, match="different offsets or infos"):
        tiled.join_routes([a, dict(b, infos=other)])
    none = [dict(offsets=np.zeros(4, np.int32), infos=infos(), gids=None, xyz=None) for _ in range(2)]
    assert [g[0] for g in tiled.join_routes(none)] == [None, None, None]
