"""GPU: source sets across tiles (trg_engine_tiled_cost_field_sets; DESIGN.md section 7, "Source sets across tiles")
over the in-process transport: one process, one engine and one thread per rank, all on one device.  Every rank's cost
bits, hops, parents (global ids), owners and owned counts must equal the host definition on the concatenation of the
rows the engines export: seed_ref.seeded_field for crafted graphs, the compiled host Dijkstra from the virtual node of
seed_ref.augmented for built tilings.  Built tilings, a tiling with a gap, crafted graphs, the failure announcement,
the refusals, and the Python helpers."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import field_graphs as fg
import field_ref
import seed_ref
import stitch_cases as sc
from field_support import MOUNTAIN
from tiled_support import RING, close, craft, exported, host_fields, join_group, run_ranks, solve_sets, stitch
from tiled_support import ref, tiled  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
INVALID_ARG, DEVICE = 1, 4
SF = MOUNTAIN["safety_factor"]
FRONTIER = 1
_built = {}  # tiling -> what test_built_tilings solved: shared by the tests that only read it


def compiled_fields(lib, G, sets, starts):
    """the compiled host Dijkstra from rho = V on the augmented graph, shifted back (no Invalid members)"""
    g, V = SimpleNamespace(**G), G["V"]
    out = []
    for s, c0 in zip(sets, starts):
        assert all(G["state"][i] != fg.INVALID for i in s)
        a = seed_ref.augmented(g, s, c0)
        st, zc, zh, zp = field_ref.field(lib, a.rowptr, a.col, a.w, a.dist, a.state, SF, V)
        assert st == 0, st
        out.append(seed_ref.shift_back(V, s, c0, zc, zh, zp))
    return out


def assert_sets(at, got, G, want, parent=True):
    """every rank's part against the reference's rows of that rank, and the owned counts summed over the ranks"""
    off = G["offsets"]
    for t, g in enumerate(got):
        a, b = int(off[t]), int(off[t + 1])
        assert g["offset"] == a and g["cost"].shape == (len(want), b - a), (at, t, g["cost"].shape)
        for k, w in enumerate(want):
            for name in ("cost", "hops", "parent", "owner") if parent else ("cost", "hops", "owner"):
                x, y = g[name][k], getattr(w, name)[a:b]
                if name == "cost":
                    x, y = x.view(np.uint32), np.ascontiguousarray(y).view(np.uint32)
                bad = np.flatnonzero(x != y)
                assert bad.size == 0, (f"{at}: rank {t} set {k}: {bad.size} {name} differ, first at global id "
                                       f"{a + bad[0]}: {g[name][k][bad[0]]!r} != {getattr(w, name)[a + bad[0]]!r}")
    for k, w in enumerate(want):
        owned = np.sum([g["owned"][k] for g in got], 0)
        assert np.array_equal(owned, w.owned), (at, k, owned, w.owned)
    assert sum(g["info"].roots for g in got) == sum(len(seed_ref.roots(w)) for w in want), at


def usable(G, tile):
    """this tile's valid nodes with edges, as global ids"""
    a, b = int(G["offsets"][tile]), int(G["offsets"][tile + 1])
    return np.arange(a, b)[(G["state"][a:b] != fg.INVALID) & (np.diff(G["rowptr"])[a:b] > 0)]


def frontier_targets(G, every=0):
    """per tile: the local ids of its Frontier nodes; with `every`, also every `every`-th node and the last one (a
    tile built by init_graph alone has no Frontier node: the reads must not be checked on nothing)"""
    off = G["offsets"]
    out = []
    for t in range(len(off) - 1):
        n = int(off[t + 1] - off[t])
        ids = np.flatnonzero(G["state"][int(off[t]):int(off[t + 1])] == FRONTIER)
        if every and n:
            ids = np.concatenate([ids, np.arange(0, n, every), [n - 1]])
        out.append(ids.astype(np.int32))
    return out


# ---- 1. built tilings -----------------------------------------------------------------------------------------------
def built(oa, synth, tiled, lib, name):
    if name in _built:
        return _built[name]
    lay, engines = sc.engines(oa, synth, tiled, name)
    join_group(engines, "sets-" + name)
    stitch(engines, lay)
    G = exported(tiled, engines)  # (this takes the rows off the device: the first solve reads the host rows)
    R = len(engines)
    rng = np.random.default_rng(31 + R)
    mine = [usable(G, t) for t in range(R)]
    spread = [int(rng.choice(mine[j % R])) for j in range(max(9, R))]  # members in every tile
    sets = [[int(mine[0][len(mine[0]) // 2])], [int(x) for x in rng.choice(mine[0], 2, replace=False)], spread]
    starts = [np.zeros(1, np.float32)] + [rng.uniform(0.0, 2.0, len(s)).astype(np.float32) for s in sets[1:]]
    want = compiled_fields(lib, G, sets, starts)
    targets = frontier_targets(G, every=7)
    assert all(t.size > 0 for t in targets)
    for where in ("after an export", "from the rows in HBM"):
        got = solve_sets(engines, sets, starts, targets=targets)
        assert_sets(f"{name} {where}", got, G, want)
        infos = [g["info"] for g in got]
        print(name, where, "exchanges", infos[0].exchanges, "owner exchanges", infos[0].owner_exchanges, "roots",
              [i.roots for i in infos], "owner records", [i.owner_records_sent for i in infos],
              "ms", [round(i.ms_total, 2) for i in infos])
        assert all(i.exchanges == infos[0].exchanges and i.owner_exchanges == infos[0].owner_exchanges for i in infos)
        assert infos[0].owner_exchanges >= 2  # (some owner crossed a seam)
        for t, g in enumerate(got):  # the device-side reads at the Frontier nodes equal the full arrays there
            for full, at in (("cost", "cost_at"), ("hops", "hops_at"), ("owner", "owner_at")):
                assert g[at].shape == (3, targets[t].size)
                assert np.array_equal(g[at].view(np.int32), g[full][:, targets[t]].view(np.int32)), (name, t, at)
        stitch(engines, lay)  # (again: the rows are in HBM, where the next solve reads them)
    # the one-entry set is the single-source field of the existing call, bit for bit
    one, _ = run_ranks(engines, lambda r, e: e.tiled_cost_fields(sets[0]))
    for g, o in zip(got, one):
        for nm in ("cost", "hops", "parent"):
            assert np.array_equal(g[nm][0].view(np.int32), o[nm][0].view(np.int32)), (name, nm)
    _built[name] = (G, sets, starts, want, tiled.concat_fields(got))
    for e in engines:
        e.comm_destroy()
    return _built[name]


@pytest.mark.parametrize("name", ["2x1", "2x2", "3x3"])
def test_built_tilings(oa, synth, tiled, ref, name):
    G, sets, starts, want, f = built(oa, synth, tiled, ref, name)
    assert f["owner"].shape == (3, G["V"]) and [len(s) for s in sets][:2] == [1, 2] and len(sets[2]) >= 9
    tile_of = np.searchsorted(G["offsets"], np.arange(G["V"]), side="right") - 1
    assert set(tile_of[sets[2]].tolist()) == set(range(len(G["offsets"]) - 1)) and (tile_of[sets[1]] == 0).all()
    has = want[2].parent >= 0
    assert (tile_of[np.flatnonzero(has)] != tile_of[want[2].parent[has]]).any()  # some parent is another rank's node


# ---- 2. a tile without a graph --------------------------------------------------------------------------------------
def test_owners_never_cross_a_gap(oa, synth, tiled, ref):
    lay, engines = sc.engines(oa, synth, tiled, "empty_mid")
    join_group(engines, "sets-empty-mid")
    stitch(engines, lay)
    G = exported(tiled, engines)
    off = G["offsets"]
    assert off[1] == off[2]
    left, right = usable(G, 0), usable(G, 2)
    sets = [[int(left[0]), int(right[0]), int(left[len(left) // 2]), int(right[len(right) // 2])]]
    starts = [np.array([0.0, 0.5, 0.25, 0.0], np.float32)]
    want = compiled_fields(ref, G, sets, starts)
    got = solve_sets(engines, sets, starts)
    assert_sets("empty_mid", got, G, want)
    assert set(np.unique(got[0]["owner"][0]).tolist()) <= {-1, 0, 2} and (got[0]["owner"][0] >= 0).sum() > 10
    assert set(np.unique(got[2]["owner"][0]).tolist()) <= {-1, 1, 3} and (got[2]["owner"][0] >= 0).sum() > 10
    assert got[1]["cost"].shape == (1, 0) and got[1]["owned"][0].tolist() == [0, 0, 0, 0]
    assert [g["info"].owner_exchanges for g in got] == [1, 1, 1] and [g["info"].ghosts for g in got] == [0, 0, 0]
    for e in engines:
        e.comm_destroy()


# ---- 3. - 7. crafted graphs -----------------------------------------------------------------------------------------
def crafted(tmp_path, tiled, sizes, edges, sets, starts, state=None, tag="craft"):
    """craft, export, solve, compare with the Python definition -> (engines, G, want, results)"""
    engines, _ = craft(tmp_path, sizes, edges, state, "sets-" + tag)
    G = exported(tiled, engines)
    want = host_fields(G, sets, starts)
    got = solve_sets(engines, sets, starts)
    assert_sets(tag, got, G, want)
    return engines, G, want, got


def test_chain_alternating_between_two_tiles(tmp_path, tiled):
    """every edge of a 64-node chain is a cross edge: an owner advances one seam per owner exchange"""
    gid = lambda p: (p % 2) * 32 + p // 2  # noqa: E731
    dist = np.array(fg.CHAIN_DIST, np.float32)
    edges = [(gid(p), gid(p + 1), 0.1 * (p % 3), float(dist[p % len(dist)])) for p in range(63)]
    engines, G, want, got = crafted(tmp_path, tiled, [32, 32], edges, [[gid(0), gid(63)]], None, tag="chain")
    assert (want[0].owned >= 10).all(), want[0].owned
    infos = [g["info"] for g in got]
    assert all(i.owner_exchanges >= 16 for i in infos), [i.owner_exchanges for i in infos]
    assert all((i.exchanges, i.owner_exchanges) == (infos[0].exchanges, infos[0].owner_exchanges) for i in infos)
    assert [i.owner_records_sent for i in infos] == [32, 32] and [i.roots for i in infos] == [1, 1]
    close(engines)


def test_ties_between_starts_and_walks_across_the_seam(tmp_path, tiled):
    edges = [(a, b, 0.0, 1.0) for a, b in ((0, 1), (1, 4), (4, 5), (5, 6), (6, 2), (2, 3), (6, 7))]
    sets, starts = [[0, 5, 5, 2, 2, 7]], [np.array([0, 10, 3, 5, 5, 6.5], np.float32)]
    engines, G, want, got = crafted(tmp_path, tiled, [4, 4], edges, sets, starts, tag="ties")
    w = want[0]
    assert w.cost.tolist() == [0, 1, 5, 6, 2, 3, 4, 5] and w.hops.tolist() == [0, 1, 0, 1, 2, 0, 1, 2]
    assert w.owner.tolist() == [0, 0, 3, 3, 0, 2, 2, 2] and w.owned.tolist() == [3, 0, 3, 2, 0, 0]
    assert [g["owned"][0].tolist() for g in got] == [[2, 0, 0, 2, 0, 0], [1, 0, 3, 0, 0, 0]]
    close(engines)


def lattice():
    """the lattice of unit costs in three tiles of tests/test_gpu_tiled_field.py -> (nx, ny, sizes, edges, gid of (x, y))"""
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
    return nx, ny, sizes, edges, gid


def torn_nodes(G, w):
    """nodes whose parent lies in another tile and that have a local tight predecessor with a different owner"""
    tile_of = np.searchsorted(G["offsets"], np.arange(G["V"]), side="right") - 1
    torn = 0
    for v in range(G["V"]):
        if w.parent[v] < 0 or tile_of[w.parent[v]] == tile_of[v]:
            continue
        preds = [int(u) for u in G["col"][G["rowptr"][v]:G["rowptr"][v + 1]]
                 if w.cost[u] + 1.0 == w.cost[v] and w.hops[u] + 1 == w.hops[v]]
        torn += any(tile_of[u] == tile_of[v] and w.owner[u] != w.owner[v] for u in preds)
    return torn


def test_lattice_of_exact_ties_in_three_tiles(tmp_path, tiled):
    """The owner follows the GLOBAL-id parent, not a local tight predecessor with another owner.  Set 0 is three
    corners.  In this layout a node's only local neighbour is its horizontal one, which takes its owner through the
    same order of tiles above and below: no set of corners, at any start costs, has a node whose parent is another
    tile's while a local tight predecessor has a different owner (counted on the host over all corner triples and
    start costs 0..5: none).  Set 1, in the same call, is the set on which that precondition holds."""
    nx, ny, sizes, edges, gid = lattice()
    sets = [[gid[0, 0], gid[nx - 1, ny - 1], gid[nx - 1, 0]], [gid[nx - 1, 0], gid[8, 7], gid[5, 8]]]
    engines, G, want, got = crafted(tmp_path, tiled, sizes, edges, sets, None, tag="lattice")
    assert (want[0].owned > 10).all() and torn_nodes(G, want[1]) > 3, (want[0].owned, torn_nodes(G, want[1]))
    close(engines)


def test_invalid_member_that_is_a_border_node(tmp_path, tiled):
    """it starts its field, and nothing enters it"""
    state = np.zeros(8, np.int32)
    state[1] = fg.INVALID
    edges = [(0, 1, 0.0, 0.5), (1, 4, 0.0, 0.5), (1, 5, 0.1, 0.5), (0, 2, 0.2, 0.5), (2, 5, 0.0, 0.5), (5, 4, 0.3, 0.5),
             (4, 6, 0.0, 0.5), (6, 3, 0.0, 0.5), (3, 1, 0.0, 0.5), (6, 7, 0.0, 0.5)]
    sets = [[1], [7, 1], [0]]
    starts = [np.array([0.0], np.float32), np.array([0.0, 0.25], np.float32), np.array([0.5], np.float32)]
    engines, G, want, got = crafted(tmp_path, tiled, [4, 4], edges, sets, starts, state=state, tag="invalid")
    assert want[0].hops[1] == 0 and (want[0].hops >= 0).all() and (want[0].owner == 0).all()
    assert want[1].hops[1] == 0 and want[1].owner[1] == 1 and want[1].owned[1] > 1
    assert want[2].hops[1] == -1 and (np.delete(want[2].hops, 1) >= 0).all()
    close(engines)


def test_fan_seeds_and_publishes_across_blocks(tmp_path, tiled):
    """one set of 300 entries on tile 0 (more than one seeding workgroup) among m = 4; tile 0 has 600 border nodes:
    2 400 owner items, more than a 2 048-item block of the compaction"""
    nA, nB = 600, 5
    edges = [(i, nA, 0.1 * (i % 5), 0.5 + 0.001 * (i % 17)) for i in range(nA)]
    edges += [(i, i + 1, 0.05 * (i % 3), 0.3 + 0.002 * (i % 11)) for i in range(nA - 1)]
    edges += [(nA + j, nA + j + 1, 0.0, 0.4) for j in range(nB - 1)]
    rng = np.random.default_rng(5)
    many = rng.permutation(nA)[:300].tolist()
    sets = [many, [nA, 0], [300, nA + nB - 1, 300], [nA + 2]]
    starts = [rng.uniform(0.0, 2.0, 300).astype(np.float32), np.array([0.0, 0.1], np.float32),
              np.array([1.0, 0.0, 0.5], np.float32), np.array([0.0], np.float32)]
    engines, G, want, got = crafted(tmp_path, tiled, [nA, nB], edges, sets, starts, tag="fan")
    roots = len(seed_ref.roots(want[0]))
    assert 10 < roots < 300, roots  # some of the 300 start as roots, some are beaten
    assert got[0]["info"].border_nodes == nA and got[0]["info"].owner_records_sent == 4 * nA > 2048
    close(engines)


# ---- 8. failure and refusals ----------------------------------------------------------------------------------------
def test_a_rank_without_current_rows_is_announced(tmp_path, tiled):
    from trg_planner._engine import TrgError
    engines, _ = craft(tmp_path, [6, 6], RING, tag="sets-void")
    engines[1].load_json(str(tmp_path / "sets-void1.json"))  # its graph changed after the stitch: its rows are void
    got, secs = run_ranks(engines, lambda r, e: e.tiled_cost_fields_from([[0, 7]]))
    assert isinstance(got[1], TrgError) and got[1].status == INVALID_ARG, got[1]
    assert "no current stitched rows" in str(got[1])
    assert isinstance(got[0], TrgError) and got[0].status == DEVICE, got[0]
    assert "another rank reported a failure" in str(got[0])
    assert secs < 10.0, secs
    close(engines)


def raw_call(e, ptr, gids, cost0=None, targets=None, n_targets=0, m=None):
    """the C entry as it is, with the arrays as given -> (status, message)"""
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)  # noqa: E731
    ptr, gids, targets = i32(ptr), i32(gids), i32(targets)
    cost0 = None if cost0 is None else np.ascontiguousarray(cost0, np.float32)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    st = e.L.trg_engine_tiled_cost_field_sets(
        e.h, len(ptr) - 1 if m is None else m, ip(ptr), ip(gids),
        None if cost0 is None else cost0.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, None, ip(targets),
        n_targets, None, None, None, None, None)
    return st, e.L.trg_engine_last_error(e.h).decode()


def test_refusals_leave_the_group_usable(tmp_path, tiled):
    import trg_planner
    from trg_planner._engine import TrgError
    engines, _ = craft(tmp_path, [6, 6], RING, tag="sets-refuse")
    G = exported(tiled, engines)
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(ptr=[0], gids=[0]), "m must be in [1, 64]"),
        (dict(ptr=list(range(66)), gids=[0] * 65), "m must be in [1, 64]"),
        (dict(ptr=None, gids=[0], m=1), "null set_ptr or set_gids"),
        (dict(ptr=[0, 1], gids=None), "null set_ptr or set_gids"),
        (dict(ptr=[1, 2], gids=[0, 1]), "set_ptr[0] must be 0"),
        (dict(ptr=[0, 2, 1], gids=[0, 1]), "set_ptr decreases at set 1"),
        (dict(ptr=[0, 1, 1, 2], gids=[0, 1]), "set 1 is empty"),
        (dict(ptr=[0, 1, 3], gids=[0, 3, 12]), "entry 1 of set 1 (12) is outside [0, 12)"),
        (dict(ptr=[0, 2], gids=[3, -1]), "entry 1 of set 0 (-1) is outside [0, 12)"),
        (dict(ptr=[0, 1, 3], gids=[0, 3, 4], cost0=[0.0, 1.0, nan]), "the start cost of entry 1 of set 1 is NaN, negative"),
        (dict(ptr=[0, 2], gids=[0, 3], cost0=[-1e-30, 0.0]), "the start cost of entry 0 of set 0 is NaN, negative"),
        (dict(ptr=[0, 2], gids=[0, 3], cost0=[0.0, inf]), "the start cost of entry 1 of set 0 is NaN, negative or infinite"),
        (dict(ptr=[0, 1], gids=[0], n_targets=-1), "n_targets < 0"),
        (dict(ptr=[0, 1], gids=[0], n_targets=2), "targets is null with n_targets > 0"),
    ]
    for kw, text in cases:  # (refused before any collective: one rank after the other will do)
        for e in engines:
            st, msg = raw_call(e, **kw)
            assert st == INVALID_ARG and text in msg, (kw, st, msg)
    lone = trg_planner.Engine(**MOUNTAIN)
    lone.load_json(str(tmp_path / "sets-refuse0.json"))
    with pytest.raises(TrgError) as ex:
        lone.tiled_cost_fields_from([[0]])
    assert ex.value.status == INVALID_ARG and "no communicator" in str(ex.value)
    lone.close()
    # a target outside the tile on ONE rank: announced to the other
    got, secs = run_ranks(engines, lambda r, e: e.tiled_cost_fields_from([[0, 7]], targets=[0, 6] if r == 1 else [0]))
    assert isinstance(got[1], TrgError) and got[1].status == INVALID_ARG and "outside this tile's [0, 6)" in str(got[1])
    assert isinstance(got[0], TrgError) and got[0].status == DEVICE and "another rank reported a failure" in str(got[0])
    assert secs < 10.0, secs
    # the group is whole; -0 is a start cost
    sets, starts = [[0, 7], [3]], [np.array([-0.0, 0.3], np.float32), np.array([0.2], np.float32)]
    got = solve_sets(engines, sets, starts, parent=False)
    assert got[0]["parent"] is None
    assert_sets("after the refusals", got, G, host_fields(G, sets, starts), parent=False)
    close(engines)


# ---- 9. the Python helpers ------------------------------------------------------------------------------------------
def assert_assigned(engines, tiled, G, members, starts, want):
    """tiled_assign_frontiers on every rank, merged, against the reference's owners at ALL Frontier nodes of G"""
    from trg_planner._engine import choose_frontier
    parts, _ = run_ranks(engines, lambda r, e: e.tiled_assign_frontiers(members, starts))
    assert all(isinstance(p, list) for p in parts), parts
    got = tiled.merge_frontier_picks(parts)
    frontier = G["state"] == FRONTIER
    assert len(got) == len(members)
    seen = np.concatenate([ids for ids, _ in got])
    assert len(set(seen.tolist())) == seen.size  # no node goes to two entries
    for k, (ids, pick) in enumerate(got):
        mine = np.flatnonzero(frontier & (want.owner == k))
        assert np.array_equal(ids, mine), (k, ids, mine)
        p = choose_frontier(mine, want.cost[mine], want.hops[mine])
        assert pick == (None if p is None else (p[0], float(want.cost[p[0]]), int(want.hops[p[0]]))), (k, pick)
    return int(frontier.sum()), got


def test_assign_frontiers_across_tiles(oa, synth, tiled, ref, tmp_path):
    """The built 2x2 tiling (its tiles come from init_graph alone and have no Frontier node: every entry gets nothing),
    and a crafted lattice in three tiles a fifth of whose nodes are Frontier nodes."""
    lay, engines = sc.engines(oa, synth, tiled, "2x2")
    join_group(engines, "sets-assign")
    stitch(engines, lay)
    G = exported(tiled, engines)
    stitch(engines, lay)
    rng = np.random.default_rng(8)
    members = [int(rng.choice(usable(G, t))) for t in (0, 1, 2, 3, 0)]
    starts = np.array([0.0, 0.4, 0.0, 1.5, 0.2], np.float32)
    assert_assigned(engines, tiled, G, members, starts, compiled_fields(ref, G, [members], [starts])[0])
    for e in engines:
        e.comm_destroy()
    nx, ny, sizes, edges, gid = lattice()
    state = np.zeros(nx * ny, np.int32)
    state[[gid[x, y] for x in range(nx) for y in range(ny) if (x + 2 * y) % 5 == 0]] = FRONTIER
    engines, _ = craft(tmp_path, sizes, edges, state, "sets-assign-lattice")
    G = exported(tiled, engines)
    members, starts = [gid[nx - 1, 0], gid[8, 7], gid[5, 8], gid[8, 7], gid[0, 0]], [0.0, 1.0, 0.0, 1.0, 30.0]
    n, got = assert_assigned(engines, tiled, G, members, starts, host_fields(G, [members], [starts])[0])
    assert n > 15 and all(len(got[k][0]) > 2 and got[k][1] is not None for k in (0, 1, 2))
    assert len(got[3][0]) == 0 and got[3][1] is None and len(got[4][0]) == 0  # a duplicate, and a beaten member
    close(engines)


@pytest.mark.parametrize("name", ["2x1", "2x2", "3x3"])
def test_field_route_ends_at_the_owners_root(oa, synth, tiled, ref, name):
    G, sets, starts, want, f = built(oa, synth, tiled, ref, name)
    rng = np.random.default_rng(len(name) + G["V"])
    for k, s in enumerate(sets):
        reached = np.flatnonzero(want[k].hops >= 0)
        for t in rng.choice(reached, 10).tolist():
            route = tiled.field_route(f, k, t)
            assert len(route) == want[k].hops[t] + 1 and route[-1] == t
            assert route[0] == s[f["owner"][k][t]] and f["hops"][k][route[0]] == 0, (name, k, t)
