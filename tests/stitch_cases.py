"""Test data for the tile stitch: tilings no other test builds, and crafted inputs for the
stitch's three steps.  Test code only; nothing here needs a GPU except engines().

Layouts (LAYOUTS): cores and lattice windows of every tile, so that a split_tile cut, a tile without a graph and a
tile whose cloud is an island inside its core go through the same builders (tiled_oracle.build_tiled_oracle_explicit
for the oracle, engines() for the GPU).  oracle() and engines() build a layout once per process and keep it.

Crafted records (cross_records, near_threshold_pairs, rough_records): stitch_cross takes any record array, so the
pair search, the scans and the emit kernels are fed counts that cross a 256-thread block and a 2 048-item scan tile,
and pairs whose distance test `sqrtf(dx*dx + dy*dy) < d` would come out the other way under either FMA contraction.

Crafted graphs and cross edges (ring_graph, assemble_*): stitch_assemble against tiled.assemble_global.
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

TERRAIN = dict(amplitude=2.0, wavelength=20.0)
SEED, SAMPLER_SEED, HALO = 77, 9, 11
EXPAND = 0.6  # oa.MOUNTAIN's expand_dist

Layout = namedtuple("Layout", "name cols rows cores windows no_graph")


def _grid(tiled, name, cols, rows, n, no_graph=(), island=None):
    cores = tiled.tile_cores(cols, rows, n, n)
    windows = [tiled.tile_lattice_window(t, cols, rows, n, n, HALO) for t in range(cols * rows)]
    if island is not None:  # the tile's cloud: the 2 m x 2 m of lattice in the centre of its core
        c, r = island % cols, island // cols
        windows[island] = (c * n + n // 2 - 10, c * n + n // 2 + 10, r * n + n // 2 - 10, r * n + n // 2 + 10)
    return Layout(name, cols, rows, cores, windows, tuple(no_graph))


def _split(tiled, name, cols, rows, gx, gy):
    cuts = [tiled.split_tile(t, cols, rows, gx, gy, HALO) for t in range(cols * rows)]
    return Layout(name, cols, rows, [c for c, _ in cuts], [w for _, w in cuts], ())


def layout(tiled, name):
    return {
        "2x1": lambda: _grid(tiled, name, 2, 1, 60),
        "2x2": lambda: _grid(tiled, name, 2, 2, 60),
        "3x1": lambda: _grid(tiled, name, 3, 1, 60),
        "1x3": lambda: _grid(tiled, name, 1, 3, 60),
        "3x3": lambda: _grid(tiled, name, 3, 3, 50),
        "split_3x1": lambda: _split(tiled, name, 3, 1, 130, 50),   # cores of 43 / 43 / 44 lattice columns
        "empty_mid": lambda: _grid(tiled, name, 3, 1, 60, no_graph=(1,)),
        "island_mid": lambda: _grid(tiled, name, 3, 1, 60, island=1),
    }[name]()


STEP_LAYOUTS = ["3x1", "1x3", "3x3", "split_3x1", "empty_mid", "island_mid"]

_oracles, _engines = {}, {}


def oracle(oa, synth, tiled, name):
    """(layout, tile graphs, stitched, global graph, oracles) of the tiled CPU oracle, built once."""
    if name not in _oracles:
        import tiled_oracle
        lay = layout(tiled, name)
        _oracles[name] = (lay,) + tiled_oracle.build_tiled_oracle_explicit(
            oa, synth, tiled, dict(oa.MOUNTAIN), lay.cols, lay.rows, lay.cores, lay.windows, SEED, SAMPLER_SEED,
            TERRAIN, lay.no_graph)
    return _oracles[name]


def engines(oa, synth, tiled, name):
    """(layout, engines) with every tile built on the GPU, once; a tile in no_graph has its map and no graph."""
    if name not in _engines:
        import trg_planner
        lay = layout(tiled, name)
        out = []
        for t, (core, win) in enumerate(zip(lay.cores, lay.windows)):
            e = trg_planner.Engine(**dict(oa.MOUNTAIN))
            e.set_sampler(SAMPLER_SEED, 16)
            e.set_tile(core, epoch=t)
            e.set_global_map(synth.mountain_tile(*win, seed=SEED, **TERRAIN))
            if t not in lay.no_graph:
                e.init_graph([0.5 * (core[0] + core[2]), 0.5 * (core[1] + core[3]), 0.0])
                assert e.stats()["used_device_bfs"] == 1, e.fallback_reason
            out.append(e)
        _engines[name] = (lay, out)
    return _engines[name]


def cross_census(stitched, graphs):
    """From the oracle's cross edges: their number, how many join diagonal tiles of the grid (neither the same
    column nor the same row; `cols` from the caller), rows reaching two or more other tiles."""
    ids = stitched[0]
    offs = np.concatenate([[0], np.cumsum([g.V for g in graphs])])
    reach = {}
    for ta, ia, tb, ib in ids.tolist():
        reach.setdefault(int(offs[ta]) + ia, set()).add(tb)
        reach.setdefault(int(offs[tb]) + ib, set()).add(ta)
    return dict(n_cross=int(ids.shape[0]), multi_rows=sum(1 for v in reach.values() if len(v) >= 2))


def diagonal_edges(stitched, cols):
    ids = stitched[0]
    if ids.shape[0] == 0:
        return 0
    ca, ra, cb, rb = ids[:, 0] % cols, ids[:, 0] // cols, ids[:, 2] % cols, ids[:, 2] // cols
    return int(((ca != cb) & (ra != rb)).sum())


# ---- crafted records for stitch_cross ------------------------------------------------------------------------------
FLAT_BOX = (4.0, 8.0, -1.0, 4.0)  # the flat 0.05 m map of the crafted-record cases


def flat_map():
    x0, x1, y0, y1 = FLAT_BOX
    xs = np.arange(int(round((x1 - x0) / 0.05)) + 1, dtype=np.float64) * 0.05 + x0
    ys = np.arange(int(round((y1 - y0) / 0.05)) + 1, dtype=np.float64) * 0.05 + y0
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], 1).astype(np.float32)


def _within(dx, dy, d, how):
    """The pair test on fp32 differences: "plain" = every operation rounded to fp32 (the reference's x86-64 build,
    numpy); "fma_x" = sqrtf(fma(dx, dx, dy*dy)), "fma_y" = sqrtf(fma(dy, dy, dx*dx)), the two contractions a compiler
    may make of it.  The fused sums are formed in fp64, where the product of two fp32 is exact; `exact` says that the
    sum was exact there too (TwoSum), so that the one rounding to fp32 is the fused operation's."""
    dx, dy = dx.astype(np.float32), dy.astype(np.float32)
    if how == "plain":
        s = (dx * dx + dy * dy).astype(np.float32)
        return np.sqrt(s, dtype=np.float32) < np.float32(d), np.ones(dx.shape, bool)
    a, b = (dx, dy) if how == "fma_x" else (dy, dx)
    p = a.astype(np.float64) * a.astype(np.float64)
    q = (b * b).astype(np.float32).astype(np.float64)
    s = p + q
    bb = s - p
    err = (p - (s - bb)) + (q - bb)
    return np.sqrt(s.astype(np.float32), dtype=np.float32) < np.float32(d), err == 0.0


def near_threshold_pairs(n_each=64):
    """Pairs (a left of x = 6, b right of it) at a distance within an ulp or so of expand_dist on which the plain fp32
    test and at least one of the two contractions disagree: n_each that the plain expression puts inside and a
    contraction outside, n_each the other way round.
    Returns (a[k,2], b[k,2] fp32, plain_inside[k] bool, census dict)."""
    rng = np.random.default_rng(11)
    n = 200000
    a = np.stack([rng.uniform(5.4, 6.0, n), rng.uniform(0.0, 3.0, n)], 1)
    th = rng.uniform(-1.2, 1.2, n)
    b = (a + 0.6 * np.stack([np.cos(th), np.sin(th)], 1)).astype(np.float32)
    a = a.astype(np.float32)
    seam = (a[:, 0] < 6.0) & (b[:, 0] >= 6.0)
    dx, dy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
    plain, _ = _within(dx, dy, EXPAND, "plain")
    fx, ex = _within(dx, dy, EXPAND, "fma_x")
    fy, ey = _within(dx, dy, EXPAND, "fma_y")
    any_in_out = seam & plain & (~fx | ~fy)
    any_out_in = seam & ~plain & (fx | fy)
    sure = ex & ey  # (both fused sums are the fused operations' own, see _within)
    pick = np.concatenate([np.flatnonzero(any_in_out & sure)[:n_each], np.flatnonzero(any_out_in & sure)[:n_each]])
    census = dict(in_out=int(any_in_out.sum()), out_in=int(any_out_in.sum()),
                  in_out_both=int((any_in_out & ~fx & ~fy).sum()), out_in_both=int((any_out_in & fx & fy).sum()))
    return a[pick], b[pick], plain[pick], census


def pair_tests(a, b):
    """plain / fma_x / fma_y verdicts of pairs (a[k], b[k])."""
    dx, dy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
    return {how: _within(dx, dy, EXPAND, how)[0] for how in ("plain", "fma_x", "fma_y")}


def _records(xy, z=None):
    """Boundary records of one tile from positions: local ids are a permutation-free 0..n-1 times 3 plus 1 (any ids
    do: the step only copies them)."""
    n = xy.shape[0]
    ids = (3 * np.arange(n) + 1).astype(np.int32)
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, :2] = xy
    if z is not None:
        xyz[:, 2] = z
    return ids, xyz


def cross_records():
    """Four tiles' records on the flat map, the second tile empty: tile 0 holds 700 positions left of x = 6 (500 of
    them too far from it to pair) and the 128 near-threshold a's, tile 2 holds 300 right of it and the 128 b's, tile 3
    five more on the right.  Tile 0: na = 828 > 256, U * na = 2 484 > 2 048.  Returns (ids per tile, xyz per tile)."""
    rng = np.random.default_rng(5)
    a, b, _, _ = near_threshold_pairs()
    far = np.stack([rng.uniform(4.6, 5.3, 500), rng.uniform(0.0, 3.0, 500)], 1)
    near = np.stack([rng.uniform(5.6, 6.0, 200), rng.uniform(0.0, 3.0, 200)], 1)
    right = np.stack([rng.uniform(6.0, 6.5, 300), rng.uniform(0.0, 3.0, 300)], 1)
    last = np.stack([rng.uniform(6.0, 6.4, 5), rng.uniform(0.5, 2.5, 5)], 1)
    t0 = np.concatenate([far, near, a], 0).astype(np.float32)
    t0 = t0[rng.permutation(t0.shape[0])]
    t2 = np.concatenate([right, b], 0).astype(np.float32)
    t2 = t2[rng.permutation(t2.shape[0])]
    tiles = [_records(t0), _records(np.zeros((0, 2), np.float32)), _records(t2), _records(last.astype(np.float32))]
    return [t[0] for t in tiles], [t[1] for t in tiles]


def rough_records(nearest_z, n=(400, 0, 300, 5)):
    """The same shape of input on rough ground (conftest's mountain_small, seam at x = 15): positions in a strip either
    side of the seam, z from the map through `nearest_z(xy)`, so that slope gates decide."""
    rng = np.random.default_rng(23)
    tiles = []
    for k, m in enumerate(n):
        lo, hi = (14.4, 15.0) if k == 0 else (15.0, 15.6)
        xy = np.stack([rng.uniform(lo, hi, m), rng.uniform(10.0, 16.0, m)], 1).astype(np.float32)
        tiles.append(_records(xy, nearest_z(xy) if m else None))
    return [t[0] for t in tiles], [t[1] for t in tiles]


def pack_records(ids, xyz):
    """(all records as int32 words [n, 4], rec_offsets) for trg_engine_stitch_cross."""
    rec = np.zeros((sum(i.shape[0] for i in ids), 4), np.int32)
    off = np.concatenate([[0], np.cumsum([i.shape[0] for i in ids])]).astype(np.int32)
    for t, (i, p) in enumerate(zip(ids, xyz)):
        rec[off[t]:off[t + 1], 0] = i
        rec[off[t]:off[t + 1], 1:] = np.ascontiguousarray(p, np.float32).view(np.int32)
    return rec, off


# ---- crafted graphs and cross edges for stitch_assemble -----------------------------------------------------------
def ring_graph(V):
    """A ring of V nodes 0.5 m apart along x (nodes as (pos, state), directed edges in row order) for
    field_support.write_graph, and the same as a graph object."""
    pos = np.stack([0.5 * np.arange(V), np.zeros(V), np.zeros(V)], 1).astype(np.float32)
    nodes = [([float(v) for v in p], 0) for p in pos]
    edges, col, w, d = [], [], [], []
    for i in range(V):
        for j in sorted({(i - 1) % V, (i + 1) % V} - {i}):
            ww, dd = np.float32(0.1 + 0.001 * (i % 7)), np.float32(0.5 + 0.01 * (j % 5))
            edges.append((i, j, float(ww), float(dd)))
            col.append(j)
            w.append(ww)
            d.append(dd)
    deg = [len({(i - 1) % V, (i + 1) % V} - {i}) for i in range(V)]
    g = SimpleNamespace(V=V, xyz=pos, state=np.zeros(V, np.int32),
                        rowptr=np.concatenate([[0], np.cumsum(deg)]).astype(np.int32),
                        col=np.array(col, np.int32), w=np.array(w, np.float32), dist=np.array(d, np.float32))
    return nodes, edges, g


NTILES, TILE, LOW, HIGH = 64, 5, 2, 7   # the tile under test and the two other tiles that hold nodes
N_LOW, N_HIGH = 300, 250


def assemble_offsets(V):
    """node_offsets of 64 tiles: tile 2 has 300 nodes, tile 5 (under test) V, tile 7 250; every other tile is empty,
    so tile 5 has empty tiles on both sides."""
    sizes = np.zeros(NTILES, np.int64)
    sizes[LOW], sizes[TILE], sizes[HIGH] = N_LOW, V, N_HIGH
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _edges(rows):
    """(tile_a, id_a, tile_b, id_b, w, dist) rows -> int32 words [n, 6]"""
    out = np.zeros((len(rows), 6), np.int32)
    for k, (ta, ia, tb, ib, w, d) in enumerate(rows):
        out[k, :4] = (ta, ia, tb, ib)
        out[k, 4:] = np.array([w, d], np.float32).view(np.int32)
    return out


def assemble_edge_lists(V, seed=3):
    """name -> cross edges [n, 6] for a tile of V nodes at TILE.  No two edges share (row, other end): real input
    cannot, and their order would be the atomics'."""
    rng = np.random.default_rng(seed)
    wd = lambda k: (float(np.float32(0.1 + 0.01 * (k % 13))), float(np.float32(0.3 + 0.001 * k)))  # noqa: E731
    out = {"none": _edges([])}
    out["others_only"] = _edges([(LOW, k, HIGH, k, *wd(k)) for k in range(40)])
    # one row receives 200 cross edges with distinct other ends (125 of the lower tile, 75 of the higher), shuffled
    row = V // 2
    fan = [(LOW, int(i), TILE, row, *wd(k)) for k, i in enumerate(rng.permutation(N_LOW)[:125])]
    fan += [(TILE, row, HIGH, int(i), *wd(200 + k)) for k, i in enumerate(rng.permutation(N_HIGH)[:75])]
    fan += [(LOW, 0, HIGH, 0, *wd(7))]  # and one edge that is none of this tile's
    out["fan_200"] = _edges([fan[i] for i in rng.permutation(len(fan))])
    # every row receives one edge, from either side in turn
    each = [(LOW, i % N_LOW, TILE, i, *wd(i)) if i % 2 else (TILE, i, HIGH, i % N_HIGH, *wd(i)) for i in range(V)]
    out["every_row"] = _edges([each[i] for i in rng.permutation(V)])
    return out


def assemble_expected(tiled, g, edges):
    """tiled.assemble_global on (g at TILE, nodes without edges at LOW and HIGH) restricted to TILE's rows:
    dict(rowptr, col, w, dist, cid)."""
    def bare(n):
        return SimpleNamespace(V=n, xyz=np.zeros((n, 3), np.float32), state=np.zeros(n, np.int32),
                               rowptr=np.zeros(n + 1, np.int64), col=np.zeros(0, np.int64),
                               w=np.zeros(0, np.float32), dist=np.zeros(0, np.float32))
    graphs = [bare(0) for _ in range(NTILES)]
    graphs[LOW], graphs[HIGH], graphs[TILE] = bare(N_LOW), bare(N_HIGH), g
    ids = np.ascontiguousarray(edges[:, :4]).astype(np.int64)
    w = np.ascontiguousarray(edges[:, 4]).view(np.float32)
    d = np.ascontiguousarray(edges[:, 5]).view(np.float32)
    G = tiled.assemble_global(graphs, (ids, w, d))
    r0, r1 = int(G["offsets"][TILE]), int(G["offsets"][TILE + 1])
    e0, e1 = int(G["rowptr"][r0]), int(G["rowptr"][r1])
    return dict(rowptr=G["rowptr"][r0:r1 + 1] - e0, col=G["col"][e0:e1], w=G["w"][e0:e1], dist=G["dist"][e0:e1],
                cid=np.arange(r0, r1))
