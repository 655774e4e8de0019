"""Test helper: what the tests of the fields and routes across tiles share -- the rank harness of the GPU tests (one
process, one engine and one thread per rank over the in-process transport: groups, the per-rank calls, the stitch, the
exported global graph), crafted tilings, the solves and host references of both objectives, the exact comparisons of
fields and routes, the shared graphs, the fixtures (import them by name) -- and `cuts` for the protocol tests on the
CPU.  Test code only."""
import itertools
import threading
import time
from types import SimpleNamespace

import numpy as np
import pytest

import field_graphs as fg
import field_ref
import risk_graphs as rg
import risk_ref
import seed_ref
import tiled_route_ref as trr
from field_support import MOUNTAIN, bits, ref  # noqa: F401  (ref: the fixture of the compiled cost reference)

JOIN_SECONDS = 60
SF = MOUNTAIN["safety_factor"]
F32 = np.float32
_group = itertools.count()  # one for the process: no two groups share a name


# ---- fixtures -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiled():
    from trg_planner import tiled as t
    return t


@pytest.fixture(scope="module", name="ref")
def risk_reference_lib(tmp_path_factory):
    """The compiled host Dijkstra on the (risk, hops) key (tests/cpp/risk_reference.cpp), as `ref`."""
    return risk_ref.compile_reference(tmp_path_factory.mktemp("tiled_risk"))


@pytest.fixture(scope="module")
def cost_ref(tmp_path_factory):
    """The compiled cost reference beside a `ref` that is the risk reference."""
    return field_ref.compile_reference(tmp_path_factory.mktemp("tiled_risk_cost"))


# ---- the protocol tests' cuts ---------------------------------------------------------------------------------------
def cuts(rng, V, R, empty=False):
    """R contiguous id ranges of [0, V) as R + 1 offsets; with `empty`, one range has no nodes."""
    k = R - 1 - (1 if empty else 0)
    inner = rng.choice(np.arange(1, V), size=k, replace=False).tolist()
    if empty:
        inner.append(inner[int(rng.integers(0, k))])  # a cut twice: the range between is empty
    inner = np.sort(np.array(inner, np.int64))
    return np.concatenate([[0], inner, [V]]).astype(np.int64)


# ---- ranks ----------------------------------------------------------------------------------------------------------
def join_group(engines, tag):
    name = f"test-tiled-field-{tag}-{next(_group)}"
    for r, e in enumerate(engines):
        e.comm_join_local(name, len(engines), r)


def run_ranks(engines, call):
    """call(rank, engine) on every rank, each from its own thread: [result | TrgError] per rank, wall seconds"""
    from trg_planner._engine import TrgError
    out = [None] * len(engines)

    def rank(r):
        try:
            out[r] = call(r, engines[r])
        except TrgError as ex:
            out[r] = ex

    threads = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(len(engines))]
    t0 = time.monotonic()
    for th in threads:
        th.start()
    for th in threads:
        th.join(max(0.0, JOIN_SECONDS - (time.monotonic() - t0)))
    alive = [r for r, th in enumerate(threads) if th.is_alive()]
    assert not alive, f"ranks {alive} did not return within {JOIN_SECONDS} s"
    return out, time.monotonic() - t0


def ok(got):
    """no rank returned an error"""
    from trg_planner._engine import TrgError
    bad = [g for g in got if isinstance(g, TrgError)]
    assert not bad, [str(b) for b in bad]
    return got


def stitch(engines, lay):
    got, _ = run_ranks(engines, lambda r, e: e.stitch_exchange(lay.cores[r], lay.cols, lay.rows))
    assert all(isinstance(g, tuple) for g in got), got
    return got[0]


def exported(tiled, engines):
    """The global graph from the rows the engines export (this takes the rows off the device: a solve after it builds
    its solve graph, if it has none yet, from the host rows)."""
    return tiled.concat_stitched([e.graph("stitched") for e in engines])


def close(engines):
    for e in engines:
        e.close()


def pick_sources(G, tile=0):
    """(deep inside `tile`, a border node, a node with cross edges to two other tiles or else another border node)"""
    off = G["offsets"]
    rows = np.repeat(np.arange(G["V"]), np.diff(G["rowptr"]))
    tile_of = np.searchsorted(off, np.arange(G["V"]), side="right") - 1
    cross = tile_of[rows] != tile_of[G["col"]]
    valid = G["state"] != fg.INVALID
    reach = {}
    for u, v in zip(rows[cross].tolist(), G["col"][cross].tolist()):
        reach.setdefault(u, set()).add(int(tile_of[v]))
    multi = sorted(u for u in reach if valid[u] and len(reach[u]) >= 2)
    border = sorted(u for u in reach if valid[u] and len(reach[u]) == 1)
    a, b = int(off[tile]), int(off[tile + 1])
    mine = np.arange(a, b)[valid[a:b] & (np.diff(G["rowptr"])[a:b] > 0)]
    centre = G["xyz"][a:b, :2].mean(0)
    deep = int(mine[np.argmin(((G["xyz"][mine, :2] - centre) ** 2).sum(1))])
    assert deep not in reach
    return [deep, border[0], multi[0] if multi else border[len(border) // 2]], bool(multi)


def craft(tmp_path, sizes, edges, state=None, tag="craft", extra=()):
    """Engines of len(sizes) tiles holding the symmetric global graph `edges` = [(global a, global b, w, dist)] (no
    pair twice): a tile's own edges through load_json, the others as cross-edge records through stitch_assemble,
    every engine a rank of a fresh in-process group.  extra: further (a, b, w, dist) edges INSIDE a tile that may
    repeat a pair.  -> (engines, restitch): restitch(t, engine) assembles tile t's rows again, in `engine` (a fresh
    one loads the tile's graph first)."""
    import torch
    import trg_planner
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    V = int(off[-1])
    state = np.zeros(V, np.int32) if state is None else np.asarray(state, np.int32)
    tile_of = np.searchsorted(off, np.arange(V), side="right") - 1
    assert len({(min(a, b), max(a, b)) for a, b, _, _ in edges}) == len(edges)
    assert all(tile_of[a] == tile_of[b] for a, b, _, _ in extra)
    x = [(a, b, w, d) if tile_of[a] < tile_of[b] else (b, a, w, d) for a, b, w, d in edges if tile_of[a] != tile_of[b]]
    rec = np.array([(tile_of[a], a - off[tile_of[a]], tile_of[b], b - off[tile_of[b]]) for a, b, _, _ in x],
                   np.int32).reshape(-1, 4)
    wd = np.array([(w, d) for _, _, w, d in x], F32).reshape(-1, 2)
    cross = np.ascontiguousarray(np.concatenate([rec, wd.view(np.int32)], 1))
    dev = torch.device("cuda", torch.cuda.current_device())
    cross_t = torch.from_numpy(cross).to(dev) if cross.shape[0] else None
    torch.cuda.synchronize()

    def restitch(t, e=None):
        if e is None:
            e = trg_planner.Engine(**MOUNTAIN)
        e.load_json(str(tmp_path / f"{tag}{t}.json"))
        e.stitch_assemble(t, len(sizes), off, cross_t.data_ptr() if cross_t is not None else None, int(cross.shape[0]))
        return e

    engines = []
    for t, n in enumerate(sizes):
        own = [(a - off[t], b - off[t], w, d) for a, b, w, d in list(edges) + list(extra)
               if tile_of[a] == t and tile_of[b] == t]
        src = [a for a, b, _, _ in own] + [b for a, b, _, _ in own]
        dst = [b for a, b, _, _ in own] + [a for a, b, _, _ in own]
        g = fg.from_edges(n, np.array(src, np.int64), np.array(dst, np.int64), [w for _, _, w, _ in own] * 2,
                          [d for _, _, _, d in own] * 2, state=state[off[t]:off[t + 1]])
        fg.write_json(tmp_path / f"{tag}{t}.json", g)
        engines.append(restitch(t))
    join_group(engines, tag)
    return engines, restitch


def risk_craft(tmp_path, sizes, edges, state=None, tag="craft", extra=()):
    """craft under the tag "risk-" + tag -> the engines alone"""
    return craft(tmp_path, sizes, edges, state=state, tag="risk-" + tag, extra=extra)[0]


# ---- solves and host references: cost, then risk ---------------------------------------------------------------------
def solve(engines, sources, parent=True):
    got, secs = run_ranks(engines, lambda r, e: e.tiled_cost_fields(sources, parent=parent))
    return ok(got), secs


def solve_sets(engines, sets, starts=None, targets=None, full=True, parent=True):
    """the collective call on every rank (targets: per rank, or None) -> the ranks' dicts"""
    return ok(run_ranks(engines, lambda r, e: e.tiled_cost_fields_from(
        sets, starts, targets=None if targets is None else targets[r], full=full, parent=parent))[0])


def reference(lib, G, sources):
    out = []
    for s in sources:
        st, c, h, p = field_ref.field(lib, G["rowptr"], G["col"], G["w"], G["dist"], G["state"], SF, int(s))
        assert st == 0, st
        out.append((c, h, p))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def host_fields(G, sets, starts):
    """the definition in Python: every set's SetField on the uncut graph"""
    g = SimpleNamespace(**G)
    with np.errstate(over="ignore"):
        return [seed_ref.seeded_field(g, SF, s, np.zeros(len(s), np.float32) if starts is None else starts[k])
                for k, s in enumerate(sets)]


def risk_solve(engines, sources, parent=True):
    return ok(run_ranks(engines, lambda r, e: e.tiled_risk_fields(sources, parent=parent))[0])


def risk_solve_sets(engines, sets, targets=None, full=True, parent=True):
    return ok(run_ranks(engines, lambda r, e: e.tiled_risk_fields_from(
        sets, targets=None if targets is None else targets[r], full=full, parent=parent))[0])


def risk_reference(lib, G, member_sets):
    """(risk, hops, parent), each len(member_sets) x V: the compiled reference from a node or a set of nodes"""
    out = []
    for members in member_sets:
        st, r, h, p = risk_ref.risk_field(lib, G["rowptr"], G["col"], G["w"], G["state"], members)
        assert st == 0, st
        out.append((r, h, p))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def assert_fields(at, got, G, want, names=("cost", "hops", "parent")):
    """every rank's part against the reference's rows of that rank; names: the fields of `want` in order, the first
    of them the float field, compared as bits; -> the concatenated fields"""
    from trg_planner import tiled
    off = G["offsets"]
    for t, g in enumerate(got):
        a, b = int(off[t]), int(off[t + 1])
        assert g["offset"] == a and g[names[0]].shape == (want[0].shape[0], b - a), (at, t, g[names[0]].shape)
        for name, w in zip(names, want):
            x, y = g[name], np.ascontiguousarray(w[:, a:b])
            if name == names[0]:
                x, y = x.view(np.uint32), y.view(np.uint32)
            bad = np.argwhere(x != y)
            assert bad.shape[0] == 0, (f"{at}: rank {t}: {bad.shape[0]} {name} differ, first at field {bad[0][0]}, "
                                       f"global id {a + bad[0][1]}: {g[name][tuple(bad[0])]!r} != {w[bad[0][0], a + bad[0][1]]!r}")
    return tiled.concat_fields(got)


# ---- routes ----------------------------------------------------------------------------------------------------------
def call_routes(engines, fields, targets, cap=None, xyz=True):
    return ok(run_ranks(engines, lambda r, e: e.tiled_routes(fields, targets, cap=cap, xyz=xyz))[0])


def want_routes(G, fields, pairs):
    """route_ref's routes; fields: per field (cost, hops, parent) of the uncut graph"""
    out = [None] * len(pairs)
    for k, (cost, hops, parent) in enumerate(fields):
        mine = [i for i, (f, _) in enumerate(pairs) if f == k]
        for i, r in zip(mine, trr.reference_routes(G, SF, cost, hops, parent, [pairs[i][1] for i in mine])):
            out[i] = r
    return out


def most_crossings(G, want):
    return max([trr.crossings(G["offsets"], w) for w in want if len(w.ids)], default=None)


def assert_routes(at, tiled, parts, G, want, cap=None, owners=None):
    """the ranks' parts against the reference routes -> the joined routes"""
    off = G["offsets"]
    lengths = [len(w.ids) for w in want]
    total = sum(lengths)
    offsets = trr.clipped_offsets(lengths, total if cap is None else cap)
    key = lambda i: (i.num_nodes, bits(i.cost)[0], bits(i.path_length)[0], bits(i.avg_risk)[0], i.root_gid, i.owner)  # noqa: E731
    for t, p in enumerate(parts):
        assert np.array_equal(p["offsets"], offsets), (at, t, p["offsets"], offsets)
        assert [key(i) for i in p["infos"]] == [key(i) for i in parts[0]["infos"]], (at, t)
        if p["gids"] is not None:  # exactly its own nodes, and nothing else
            mine = p["gids"] >= 0
            assert ((p["gids"][mine] >= off[t]) & (p["gids"][mine] < off[t + 1])).all(), (at, t)
            if p["xyz"] is not None:
                assert np.isnan(p["xyz"][~mine]).all() and np.array_equal(p["xyz"][mine], G["xyz"][p["gids"][mine]]), (at, t)
    joined = tiled.join_routes(parts)
    for r, (w, (ids, pts, info)) in enumerate(zip(want, joined)):
        room = int(offsets[r + 1] - offsets[r])
        if ids is not None:
            assert ids.tolist() == w.ids[:room].tolist(), f"{at}: route {r}: {ids.tolist()} != {w.ids[:room].tolist()}"
        assert info.num_nodes == len(w.ids), (at, r, info.num_nodes, len(w.ids))
        for name in ("cost", "path_length", "avg_risk"):
            x, y = getattr(info, name), getattr(w, name)
            assert bits(x)[0] == bits(y)[0], f"{at}: route {r}: {name} {x!r} != {y!r}"
        assert info.root_gid == (int(w.ids[0]) if len(w.ids) else -1), (at, r)
        if owners is None:
            assert info.owner == -1, (at, r)
    most = most_crossings(G, want)
    print(at, "routes", len(want), "most crossings", most, "exchanges", [p["info"].exchanges for p in parts], "records",
          [p["info"].records_sent for p in parts], "ms", [round(p["info"].ms_total, 2) for p in parts])
    assert [p["info"].exchanges for p in parts] == [2 if most is None else most + 3] * len(parts), at
    return joined


def crossing_counts(G, hops, parent):
    """per node: how often the route to it steps over a seam (-1: unreached)"""
    tile_of = np.searchsorted(G["offsets"], np.arange(G["V"]), side="right") - 1
    out = np.full(G["V"], -1, np.int64)
    for v in np.argsort(hops, kind="stable"):
        if hops[v] == 0:
            out[v] = 0
        elif hops[v] > 0:
            out[v] = out[parent[v]] + (tile_of[parent[v]] != tile_of[v])
    return out


# ---- the shared graphs -----------------------------------------------------------------------------------------------
INVALID_1 = [(0, 1, 0.0, 0.5), (1, 4, 0.0, 0.5), (1, 5, 0.1, 0.5), (0, 2, 0.2, 0.5), (2, 5, 0.0, 0.5), (5, 4, 0.3, 0.5),
             (4, 6, 0.0, 0.5), (6, 3, 0.0, 0.5), (3, 1, 0.0, 0.5), (6, 7, 0.0, 0.5)]  # in [4, 4]; node 1 is Invalid
RING = [(i, (i + 1) % 12, 0.1, 0.5) for i in range(12)]


def tie_lattice():
    """unit costs on a 12 x 9 lattice whose cells go to three tiles in diagonal stripes -> (sizes, edges, sources)"""
    nx, ny, R = 12, 9, 3
    tile = lambda x, y: (x // 2 + y) % R  # noqa: E731
    cells = sorted(((tile(x, y), y, x) for x in range(nx) for y in range(ny)))
    gid = {(x, y): i for i, (_, y, x) in enumerate(cells)}
    sizes = [sum(1 for c in cells if c[0] == t) for t in range(R)]
    edges = []
    for x in range(nx):
        for y in range(ny):
            if x + 1 < nx:
                edges.append((gid[x, y], gid[x + 1, y], 0.0, 1.0))
            if y + 1 < ny:
                edges.append((gid[x, y], gid[x, y + 1], 0.0, 1.0))
    return sizes, edges, [gid[0, 0], gid[nx - 1, ny - 1], gid[5, 4]]


def level_lattice():
    """tie_lattice with weights over risk_graphs.LEVELS"""
    sizes, edges, sources = tie_lattice()
    levels = rg.LEVELS.tolist()
    return sizes, [(a, b, levels[(3 * a + 5 * b) % 5], d) for a, b, _, d in edges], sources
