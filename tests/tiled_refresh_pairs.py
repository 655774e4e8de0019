"""Test helper: pairs of tilings for the tests of the refresh across tiles ("Refresh across tiles")
-- an earlier stitched graph A, the current one B, per tile the node map from B's LOCAL ids to A's (-1: a node the tile
did not have), and the source sets as GLOBAL ids of A -- each at the smallest size at which one piece can go wrong.
A tiling is (sizes, edges, state): the tiles' node counts, the symmetric global graph as (a, b, w, dist) with no pair
twice -- what tiled_support.craft takes -- and the node states.  Both the CPU test of tests/tiled_refresh_ref.py and the
GPU test of the engine take them from here.  Test code only."""
from collections import namedtuple

import numpy as np

import field_graphs as fg
import refresh_pairs as rp
import risk_graphs as rg
import tiled_support as ts

F32 = np.float32

Tiling = namedtuple("Tiling", "sizes edges state")
# a, b: Tiling; maps: per tile int32 over b's nodes of that tile; sets: lists of global ids of a
Pair = namedtuple("Pair", "a b maps sets")


def tiling(sizes, edges, state=None):
    return Tiling(list(sizes), [(int(a), int(b), float(F32(w)), float(F32(d))) for a, b, w, d in edges],
                  np.zeros(sum(sizes), np.int32) if state is None else np.asarray(state, np.int32).copy())


def offsets(t):
    return np.concatenate([[0], np.cumsum(t.sizes)]).astype(np.int64)


def csr(t):
    """The uncut graph of a tiling as the CSR dict of tiled_ref (rows in ascending column order) -> (G, offsets)."""
    V = sum(t.sizes)
    src = np.array([a for a, b, _, _ in t.edges] + [b for a, b, _, _ in t.edges], np.int64)
    dst = np.array([b for a, b, _, _ in t.edges] + [a for a, b, _, _ in t.edges], np.int64)
    w = np.array([w for _, _, w, _ in t.edges] * 2, F32)
    d = np.array([d for _, _, _, d in t.edges] * 2, F32)
    order = np.lexsort((dst, src))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))]).astype(np.int64)
    return dict(V=V, rowptr=rowptr, col=dst[order], w=w[order], dist=d[order], state=t.state.astype(np.int64)), offsets(t)


def of_csr(G, off):
    """A symmetric CSR dict cut at `off` as a tiling."""
    rows = np.repeat(np.arange(G["V"]), np.diff(G["rowptr"]))
    up = rows < G["col"]
    return tiling(np.diff(off).tolist(), zip(rows[up], G["col"][up], G["w"][up], G["dist"][up]), G["state"])


def of_graph(g, sizes):
    """A symmetric FieldGraph as a tiling of contiguous id ranges."""
    G = dict(V=len(g.state), rowptr=np.asarray(g.rowptr), col=np.asarray(g.col), w=g.w, dist=g.dist, state=g.state)
    return of_csr(G, np.concatenate([[0], np.cumsum(sizes)]))


def identity_maps(t):
    return [np.arange(n, dtype=np.int32) for n in t.sizes]


def old2new(a, maps):
    """old global id -> new global id under the ranks' maps (the first new node naming it), -1 where gone"""
    off_a, new_off = offsets(a), np.concatenate([[0], np.cumsum([len(m) for m in maps])])
    out = np.full(sum(a.sizes), -1, np.int64)
    for t, m in enumerate(maps):
        for v in range(len(m) - 1, -1, -1):
            if m[v] >= 0:
                out[off_a[t] + m[v]] = new_off[t] + v
    return out


def remapped(a, maps, drop=(), values=None, extra=(), state=None):
    """Tiling a under the ranks' maps: an edge survives with both its ends, but the pairs in `drop` (old ids, either
    order); values: {(old a, old b): (w, dist)} replaces an edge's values; extra: more edges in NEW global ids; state:
    {new global id: state} over the carried states (a new node is valid)."""
    o2n = old2new(a, maps)
    gone = {(min(p), max(p)) for p in drop}
    values = {(min(p), max(p)): v for p, v in (values or {}).items()}
    edges = []
    for x, y, w, d in a.edges:
        key = (min(x, y), max(x, y))
        if o2n[x] < 0 or o2n[y] < 0 or key in gone:
            continue
        w, d = values.get(key, (w, d))
        edges.append((int(o2n[x]), int(o2n[y]), w, d))
    st = np.zeros(sum(len(m) for m in maps), np.int32)
    ok = o2n >= 0
    st[o2n[ok]] = a.state[ok]
    for v, s in (state or {}).items():
        st[v] = s
    return tiling([len(m) for m in maps], edges + list(extra), st)


def new_sets(pair):
    o2n = old2new(pair.a, pair.maps)
    return [[int(o2n[g]) for g in s] for s in pair.sets]


# ---- the pairs --------------------------------------------------------------------------------------------------------

def ring_identity(m):
    """tiled_support.RING in [6, 6], stitched again unchanged"""
    a = tiling([6, 6], ts.RING)
    return Pair(a, a, identity_maps(a), [[0], [7], [3]][:m])


def seam_plateau():
    """Sub-ulp costs across a seam: B's added edge lowers node 1's cost, node 4's cost 1 000 absorbs either, so tile 1's
    graph, the seam record and tile 1's cost bits stay while all its hops rise by 2.  A single warm pass keeps them."""
    e = [(0, 1, 0.0, 1e-6), (1, 4, 0.0, 1000.0), (4, 5, 0.0, 1.0), (2, 3, 0.0, 1e-7), (3, 1, 0.0, 1e-7), (5, 6, 0.0, 2.0),
         (6, 7, 0.0, 1.0)]
    a = tiling([4, 4], e)
    return Pair(a, tiling([4, 4], e + [(0, 2, 0.0, 1e-7)]), identity_maps(a), [[0]])


def block_chain(cut):
    """refresh_pairs.chain_pair's chain of 1 000 in [500, 500]: cut between 899 and 900, or joined again"""
    p = rp.chain_pair(cut)
    a, b = of_graph(p.a, [500, 500]), of_graph(p.b, [500, 500])
    return Pair(a, b, identity_maps(a), [[s] for s in p.sources])


def alternating_chain(cut):
    """A unit chain of 64 whose consecutive nodes alternate between two tiles (every hop a seam), with the link between
    positions 57 and 58 cut, or joined again."""
    gid = lambda p: (p % 2) * 32 + p // 2  # noqa: E731
    full = [(gid(p), gid(p + 1), 0.0, 1.0) for p in range(63)]
    broken = [e for p, e in enumerate(full) if p != 57]
    a, b = (full, broken) if cut else (broken, full)
    return Pair(tiling([32, 32], a), tiling([32, 32], b), identity_maps(tiling([32, 32], a)), [[gid(0)]])


def tie_lattice(risk=False):
    """tiled_support.tie_lattice (level_lattice for risk) in three tiles; B: a block made Invalid and two weights raised
    on least walks from the first source; three sources."""
    sizes, edges, sources = ts.level_lattice() if risk else ts.tie_lattice()
    a = tiling(sizes, edges)
    deg = np.bincount(np.array([x for e in edges for x in e[:2]]), minlength=sum(sizes))
    inner = [v for v in range(sum(sizes)) if deg[v] == 4 and v not in sources]
    state = {v: fg.INVALID for v in inner[10:16]}
    first = [e for e in edges if sources[0] in e[:2]]
    values = {e[:2]: (0.9, 3.0) for e in first}
    return Pair(a, remapped(a, identity_maps(a), values=values, state=state), identity_maps(a), [[s] for s in sources])


def cross_only():
    """Only the cross records differ: a cross edge of the ring is removed and another added, no tile graph changes."""
    a = tiling([6, 6], ts.RING)
    b = remapped(a, identity_maps(a), drop=[(5, 6)], extra=[(2, 9, 0.1, 0.5)])
    return Pair(a, b, identity_maps(a), [[0], [7]])


def renumbered(seed=5, V=200, R=3, scramble=False, forget=False, empty_before=False, empty_after=False):
    """A random symmetric graph of about V nodes in R tiles.  Tile 0 loses and gains nodes, so every later global id
    shifts; the others are permuted; weights are raised and lowered.  scramble: tile 1's map is a random one (a hint
    that carries keys the anchor drops); forget: tile 1's map is all -1 but for its members.  empty_before: the last
    tile but one has no nodes, in A and in B; empty_after: it loses all its nodes in B (and holds no member)."""
    import tiled_ref as tr
    rng = np.random.default_rng(seed)
    G = tr.symmetric_graph(rng, V)
    off = np.concatenate([[0], np.sort(rng.choice(np.arange(8, V - 8), size=R - 1, replace=False)), [V]]).astype(np.int64)
    if empty_before:
        off[R - 1] = off[R - 2]  # the last tile but one is [off[R - 2], off[R - 1])
    a = of_csr(G, off)
    valid = np.flatnonzero(a.state != fg.INVALID)
    if empty_after:  # no member lies in the tile that loses its nodes
        valid = valid[(valid < off[R - 2]) | (valid >= off[R - 1])]
    sets = [[int(valid[0])], [int(valid[len(valid) // 2]), int(valid[-1]), int(valid[len(valid) // 2])], [int(valid[-2])]]
    members = {g for s in sets for g in s}
    maps, extra = [], []
    for t in range(R):
        n = a.sizes[t]
        keep = np.ones(n, bool)
        n_new = 0
        if t == 0 and n > 8:
            gone = [v for v in rng.choice(n, size=max(1, n // 8), replace=False).tolist() if int(off[t]) + v not in members]
            keep[gone] = False
            n_new = max(2, n // 10)
        if empty_after and t == R - 2:
            keep[:] = False
        m = np.concatenate([np.flatnonzero(keep), np.full(n_new, -1)]).astype(np.int32)
        maps.append(m[rng.permutation(len(m))] if len(m) else m)
    new_off = np.concatenate([[0], np.cumsum([len(m) for m in maps])])
    Vn = int(new_off[-1])
    for t, m in enumerate(maps):  # every new node gets three edges to anywhere
        for v in np.flatnonzero(m < 0).tolist():
            for o in rng.choice(Vn, size=3, replace=False).tolist():
                if o != new_off[t] + v:
                    extra.append((int(new_off[t] + v), int(o), float(rng.choice([0.0, 0.4])), float(rng.choice([0.0, 0.45, 150.0]))))
    extra = list({(min(x, y), max(x, y)): (x, y, w, d) for x, y, w, d in extra}.values())
    touched = rng.choice(len(a.edges), size=max(1, len(a.edges) // 15), replace=False)
    values = {a.edges[i][:2]: (float(F32(a.edges[i][2] * rng.choice([0.0, 0.5, 2.0, 4.0]))), a.edges[i][3]) for i in touched}
    b = remapped(a, maps, values=values, extra=extra)
    hints = [m.copy() for m in maps]
    if (scramble or forget) and R > 1 and a.sizes[1] > 0:
        o2n = old2new(a, maps)
        mine = [int(o2n[g] - new_off[1]) for g in members if int(off[1]) <= g < int(off[2])]
        h = rng.integers(-1, a.sizes[1], size=len(maps[1])).astype(np.int32) if scramble else np.full(len(maps[1]), -1, np.int32)
        # a member keeps its entry, and nothing before it may name its old node: the map decides where the members are
        for v in mine:
            old = maps[1][v]
            h[h == old] = -1
            h[v] = old
        hints[1] = h
    return Pair(a, b, hints, sets)


def saturation():
    """A +inf fold across a seam: field_graphs.saturating_chain cut in two, without its link 3 -> 4 in B."""
    p = rp.saturating_pairs()["saturating_chain"]
    V = len(p.a.state)
    sizes = [V // 2, V - V // 2]
    a = of_graph(p.a, sizes)
    return Pair(a, of_graph(p.b, sizes), identity_maps(a), [[0], [1]])


def sets_with_owners():
    """Three tiles of the tie lattice: a member on the border and a member named twice; B raises weights."""
    sizes, edges, sources = ts.tie_lattice()
    a = tiling(sizes, edges)
    off = offsets(a)
    tile_of = np.searchsorted(off, np.arange(sum(sizes)), side="right") - 1
    border = sorted({x for e in edges if tile_of[e[0]] != tile_of[e[1]] for x in e[:2]})
    sets = [[sources[0], border[3], sources[0]], [sources[1], sources[2]]]
    values = {e[:2]: (0.7, 2.5) for e in edges if border[3] in e[:2] or sources[1] in e[:2]}
    return Pair(a, remapped(a, identity_maps(a), values=values), identity_maps(a), sets)


def levels(t, seed=0):
    """tiling t with its weights over risk_graphs.LEVELS (plateaus of equal risk)"""
    lv = rg.LEVELS.tolist()
    return tiling(t.sizes, [(x, y, lv[(3 * x + 5 * y + seed) % len(lv)], d) for x, y, _, d in t.edges], t.state)
