"""Test helper: graphs for the cost field's tests, as CSR arrays plus node positions -- the random family of
tests/test_field_reference.py and deterministic structured families built to reach what that family cannot:
long rows, thousands of rounds, massive exact ties, a zero or subnormal bucket width, costs over 60 decades,
folds that saturate to +inf, and degenerate shapes.  write_json stores one in the engine's graph format.
Test code only."""
import json
from collections import namedtuple

import numpy as np

from field_keys import F32, INVALID, cost_values  # noqa: F401

# rowptr, col, w, dist, state: the CSR the reference takes; pos: (V, 3) float32, at least 1 m apart
FieldGraph = namedtuple("FieldGraph", "rowptr col w dist state pos")


def random_graph(rng, V, scale=1):
    """Edges: a symmetric core, directed-only extras, duplicates with other weights, zero-dist edges and
    sub-ulp costs; two components (ids >= V // 2 + 3 only link among themselves); a few Invalid nodes.
    `scale` multiplies the node count and keeps the edge mix (scale 1: the draws of the CPU test's seeds)."""
    V = V * scale
    edges = []
    half = V // 2 + 3
    for _ in range(3 * V):
        a = int(rng.integers(0, half))
        b = int(rng.integers(0, half))
        if a == b:
            continue
        w = F32(rng.choice([0.0, rng.uniform(0.1, 1.0)]))
        d = F32(rng.choice([0.0, 1e-9, rng.uniform(0.3, 0.6), rng.uniform(100.0, 200.0)], p=[0.1, 0.1, 0.6, 0.2]))
        edges.append((a, b, w, d))
        r = rng.uniform()
        if r < 0.6:
            edges.append((b, a, w, d))  # symmetric
        elif r < 0.8:
            edges.append((a, b, F32(rng.uniform(0.1, 1.0)), d))  # duplicate, another weight
    for _ in range(V):
        a = int(rng.integers(half, V))
        b = int(rng.integers(half, V))
        if a != b:
            edges.append((a, b, F32(rng.uniform(0.1, 1.0)), F32(rng.uniform(0.3, 0.6))))
    state = np.zeros(V, np.int32)
    state[rng.choice(V, size=max(1, V // 8), replace=False)] = INVALID
    state[rng.choice(V, size=max(1, V // 8), replace=False)] = 1  # Frontier: an ordinary node here
    order = sorted(range(len(edges)), key=lambda i: edges[i][0])  # rows in push order
    rowptr = np.zeros(V + 1, np.int32)
    for i in order:
        rowptr[edges[i][0] + 1] += 1
    rowptr = np.cumsum(rowptr).astype(np.int32)
    col = np.array([edges[i][1] for i in order], np.int32)
    w = np.array([edges[i][2] for i in order], np.float32)
    d = np.array([edges[i][3] for i in order], np.float32)
    return rowptr, col, w, d, state


def random_small(seed):
    """The random family at the CPU test's sizes: V drawn from 8..47, then the graph, from one seeded stream."""
    rng = np.random.default_rng(seed)
    V = int(rng.integers(8, 48))
    return random_graph(rng, V)


# (seed, V, scale) of the large random graphs, by size class
RANDOM_LARGE = {2000: [(100, 40, 50), (101, 41, 50), (102, 39, 50), (103, 40, 50)],
                20000: [(200, 40, 500)]}


def square_positions(V):
    """Node i at (i % side, i // side, 0) metres of the smallest square lattice that holds V nodes."""
    side = max(1, int(np.ceil(np.sqrt(V))))
    i = np.arange(V)
    return np.stack([i % side, i // side, np.zeros(V)], axis=1).astype(np.float32)


def with_positions(csr):
    return FieldGraph(*csr, square_positions(len(csr[4])))


def from_edges(V, src, dst, w, dist, state=None, pos=None):
    """Rows in push order (a stable sort by source), as the engine's loader lays them out."""
    src = np.asarray(src, np.int64).reshape(-1)
    order = np.argsort(src, kind="stable")
    rowptr = np.zeros(V + 1, np.int32)
    np.add.at(rowptr, src + 1, 1)
    rowptr = np.cumsum(rowptr).astype(np.int32)
    state = np.zeros(V, np.int32) if state is None else np.asarray(state, np.int32)
    return FieldGraph(rowptr, np.asarray(dst, np.int32).reshape(-1)[order], np.asarray(w, np.float32).reshape(-1)[order],
                      np.asarray(dist, np.float32).reshape(-1)[order], state,
                      square_positions(V) if pos is None else np.asarray(pos, np.float32))


def edge_costs(g, sf):
    """(safety_factor * w + 1) * dist, every operation rounded to fp32."""
    return cost_values(g.w, g.dist, sf)


def bucket_width(g, sf, scale):
    """The engine's bucket width: scale times the mean cost (in double) of the edges into valid nodes, as fp32."""
    ok = g.state[g.col] != INVALID
    if not ok.any():
        return F32(0.0)
    mean = edge_costs(g, sf)[ok].astype(np.float64).mean()
    with np.errstate(over="ignore"):
        return F32(scale * mean) if mean > 0 else F32(0.0)


# ---- structured families ------------------------------------------------------------------------------

# a tiny step right after a huge one (swallowed whole), a zero, a half-ulp-sized step later on
CHAIN_DIST = (0.5, 1000.0, 1e-6, 0.25, 0.0, 3.0, 1e-9)
CHAIN_W = (0.0, 0.3, 0.0)


def chain(V, symmetric=False):
    """0 -> 1 -> ... -> V-1 (and back, at the same cost, if symmetric): one node per round."""
    a = np.arange(V - 1)
    d = np.array(CHAIN_DIST, np.float32)[a % len(CHAIN_DIST)]
    w = np.array(CHAIN_W, np.float32)[a % len(CHAIN_W)]
    if not symmetric:
        return from_edges(V, a, a + 1, w, d)
    # (push order: forward edge of node i, then the backward edge i + 1 -> i)
    src = np.stack([a, a + 1], axis=1)
    dst = np.stack([a + 1, a], axis=1)
    return from_edges(V, src, dst, np.repeat(w, 2), np.repeat(d, 2))


def star(deg, hubs=1):
    """`hubs` hubs (ids 0..hubs-1) and `deg` leaves; leaf j hangs on hub j % hubs, both ways, and the leaves
    form a ring of cheap edges, both ways.  With more than one hub the last node is a root joined to every hub at
    cost 0, so that all hubs are expanded in one round.  Seven leaves in eight of a hub cost 0.1..1 from it, the
    eighth 1..40: the hub's row straddles the first threshold at a bucket width of 4 and of 0.5 mean costs."""
    V = hubs + deg + (1 if hubs > 1 else 0)
    j = np.arange(deg)
    leaf = hubs + j
    hub = j % hubs
    frac = ((j * 7919) % deg) / float(deg)  # a fixed permutation-like spread over [0, 1)
    d_leaf = np.where((j // hubs) % 8 == 7, 1.0 + 39.0 * frac, 0.1 + 0.9 * frac).astype(np.float32)
    w_leaf = np.where(j % 3 == 0, 0.2, 0.0).astype(np.float32)
    nxt = hubs + (j + 1) % deg
    src = [hub, leaf, leaf, nxt]
    dst = [leaf, hub, nxt, leaf]
    w = [w_leaf, w_leaf, np.zeros(deg, np.float32), np.zeros(deg, np.float32)]
    d = [d_leaf, d_leaf, np.full(deg, 0.05, np.float32), np.full(deg, 0.05, np.float32)]
    if hubs > 1:
        root = np.full(hubs, V - 1)
        h = np.arange(hubs)
        src += [root, h]
        dst += [h, root]
        w += [np.zeros(hubs, np.float32)] * 2
        d += [np.zeros(hubs, np.float32)] * 2
    return from_edges(V, np.concatenate(src), np.concatenate(dst), np.concatenate(w), np.concatenate(d))


def lattice(nx, ny, zero_band=False):
    """4-connected nx x ny lattice, every edge the same cost: each node has up to C(h, k) least walks and only
    the smallest parent id tells answers apart.  zero_band: edges among nodes with |ix - iy| <= 1 cost 0."""
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    ix, iy = ix.reshape(-1), iy.reshape(-1)
    idx = iy * nx + ix
    src, dst = [], []
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        ok = (ix + dx >= 0) & (ix + dx < nx) & (iy + dy >= 0) & (iy + dy < ny)
        src.append(idx[ok])
        dst.append(idx[ok] + dy * nx + dx)
    src, dst = np.concatenate(src), np.concatenate(dst)
    d = np.full(src.shape[0], 0.5, np.float32)
    if zero_band:
        on = lambda n: np.abs(n % nx - n // nx) <= 1
        d[on(src) & on(dst)] = 0.0
    pos = np.stack([ix, iy, np.zeros(nx * ny)], axis=1).astype(np.float32)
    return from_edges(nx * ny, src, dst, np.full(src.shape[0], 0.25, np.float32), d, pos=pos)


def _connected_edges(rng, V, extra=3):
    """A random spanning tree (node i hangs on an earlier node) plus extra * V random edges, all both ways."""
    a = np.arange(1, V)
    b = (rng.random(V - 1) * a).astype(np.int64)  # in [0, i)
    xa = rng.integers(0, V, size=extra * V)
    xb = rng.integers(0, V, size=extra * V)
    keep = xa != xb
    s = np.concatenate([a, xa[keep]])
    t = np.concatenate([b, xb[keep]])
    return np.stack([s, t], axis=1), np.stack([t, s], axis=1)


def _connected(V, seed, dist_of):
    rng = np.random.default_rng(seed)
    src, dst = _connected_edges(rng, V)
    m = src.shape[0]
    d = np.repeat(np.asarray(dist_of(rng, m), np.float32), 2)
    w = np.repeat(rng.choice(np.array([0.0, 0.3, 1.0], np.float32), size=m), 2)
    return from_edges(V, src, dst, w, d)


def all_zero(V, seed=0):
    """A random connected graph with dist = 0 everywhere: every cost is 0, so is the mean and the bucket width."""
    return _connected(V, seed, lambda rng, m: np.zeros(m))


def denormal(V, seed=0):
    """Costs in the fp32 subnormal range: dist = (0.5 .. 2) * 1e-41."""
    return _connected(V, seed, lambda rng, m: rng.uniform(0.5, 2.0, size=m) * 1e-41)


def heavy_tail(V, seed=0):
    """dist log-uniform over 1e-30 .. 1e30: almost every add swallows its addend or is swallowed."""
    return _connected(V, seed, lambda rng, m: 10.0 ** rng.uniform(-30.0, 30.0, size=m))


def saturating_chain():
    """0 -> 1 -> ... -> 5, every edge 2e38 (finite): the fold is +inf from node 2 on, and nodes 2..5 are reached."""
    a = np.arange(5)
    return from_edges(6, a, a + 1, np.zeros(5), np.full(5, 2e38))


def saturating_branch():
    """Finite-cost nodes (0, 1, 7, 8, 9); nodes first reached at +inf one, two and three hops past the first
    saturated node 2 (3 and 10; 4 and 5; 6), 6 reachable only through them; +inf walks of different lengths into
    10 (3 and 4 hops) and 5 (4 and 5 hops), where the hops decide; an Invalid node (11) and an unreachable one
    (12); back edges from +inf nodes into finite ones."""
    e = [(0, 1, 0.0, 2e38), (1, 2, 0.0, 2e38), (2, 3, 0.0, 1.0), (3, 4, 0.5, 0.0), (4, 5, 0.0, 7.0),
         (5, 6, 0.0, 1e-9), (0, 7, 0.0, 1.0), (7, 8, 0.0, 2.0), (8, 9, 0.0, 3e38), (9, 10, 0.0, 3e38),
         (2, 10, 0.0, 1.0), (10, 5, 0.0, 1.0), (3, 0, 0.0, 1.0), (6, 7, 0.0, 0.0), (5, 9, 0.0, 1.0),
         (4, 11, 0.0, 1.0), (11, 12, 0.0, 1.0), (12, 0, 0.0, 1.0)]
    state = np.zeros(13, np.int32)
    state[11] = INVALID
    return from_edges(13, *zip(*e), state=state)


def oddities():
    """name -> (graph, sources): degenerate shapes, each small enough to read."""
    out = {}
    e = [(0, 0, 0.0, 0.0), (0, 1, 0.0, 1.0), (1, 1, 0.5, 2.0), (1, 2, 0.0, 1.0), (2, 2, 0.0, 1e-9), (2, 0, 0.0, 1.0)]
    out["self_loops"] = (from_edges(3, *zip(*e)), [0, 1, 2])
    e = [(0, 1, 0.5, 1.0), (0, 1, 0.5, 1.0), (0, 1, 0.5, 1.0),      # three equal
         (1, 2, 0.9, 1.0), (1, 2, 0.1, 1.0), (1, 2, 0.4, 1.0),      # three unequal: the middle one is least
         (0, 2, 0.0, 2.85), (2, 3, 0.0, 1.0), (2, 3, 0.0, 1.0), (3, 0, 0.2, 1.0), (3, 0, 0.2, 1.0), (3, 0, 0.1, 1.0)]
    out["triple_duplicates"] = (from_edges(4, *zip(*e)), [0, 1, 3])
    e = [(0, 1, 0.0, -0.0), (1, 2, 0.7, -0.0), (2, 3, 0.0, 1.0), (3, 4, 0.0, -0.0), (0, 4, 0.0, 1.0), (4, 0, 0.3, -0.0)]
    out["negative_zero_dist"] = (from_edges(5, *zip(*e)), [0, 2, 4])
    e = [(0, 1, 0.0, 1.0), (1, 0, 0.0, 1.0), (1, 2, 0.0, 1.0), (2, 1, 0.0, 1.0), (2, 0, 0.0, 0.5), (0, 2, 0.0, 0.5)]
    out["source_invalid"] = (from_edges(3, *zip(*e), state=[INVALID, 0, 1]), [0])
    e = [(1, 0, 0.0, 1.0), (1, 2, 0.0, 1.0), (2, 0, 0.0, 1.0), (2, 1, 0.0, 1.0)]
    out["source_without_out_edges"] = (from_edges(3, *zip(*e)), [0])
    out["one_node"] = (from_edges(1, [], [], [], []), [0])
    out["no_edges"] = (from_edges(5, [], [], [], [], state=[0, 1, INVALID, 0, 0]), [0, 2, 4])
    e = [(0, 1, 0.0, 1.0), (0, 2, 0.0, 1.0), (0, 3, 0.0, 0.0), (1, 4, 0.0, 1.0), (2, 4, 0.0, 1.0), (3, 4, 0.0, 1.0),
         (4, 0, 0.0, 1.0)]
    out["source_neighbours_invalid"] = (from_edges(5, *zip(*e), state=[0, INVALID, INVALID, INVALID, 0]), [0, 4])
    return out


# ---- what the reference's output says about a graph ----------------------------------------------------

def witnesses(g, sf, src, cost, hops):
    """(hop-tie witness, absorption witness) of the reference's field on g: is there a tight edge u -> v
    (fl(cost[u] + c) == cost[v], v valid), v not the source, with hops[u] + 1 > hops[v] -- a dearer-or-equal prefix
    a single label-correcting pass may keep -- and is there a tight edge with c > 0 and cost[u] == cost[v]."""
    V = len(g.state)
    u = np.repeat(np.arange(V), np.diff(g.rowptr))
    v = g.col
    c = edge_costs(g, sf)
    ok = (hops[u] >= 0) & (g.state[v] != INVALID)
    with np.errstate(over="ignore"):
        tight = ok & ((cost[u] + c).astype(np.float32).view(np.uint32) == cost[v].view(np.uint32))
    hop_tie = tight & (v != src) & (hops[u] + 1 > hops[v])
    absorbed = tight & (c > 0) & (cost[u] == cost[v])
    return bool(hop_tie.any()), bool(absorbed.any())


# ---- the engine's graph format ---------------------------------------------------------------------------

def write_json(path, g):
    """nodes in id order, edges row by row: load_json pushes them in file order, so the exported CSR is g.
    A float32 goes out as Python's repr of its double (shortest digits that read back to that double)."""
    V = len(g.state)
    u = np.repeat(np.arange(V), np.diff(g.rowptr)).tolist()
    doc = {"nodes": [{"id": i, "pos": p, "state": s}
                     for i, (p, s) in enumerate(zip(g.pos.astype(np.float64).tolist(), g.state.tolist()))],
           "edges": [{"source": a, "target": b, "weight": ww, "dist": dd}
                     for a, b, ww, dd in zip(u, g.col.tolist(), g.w.astype(np.float64).tolist(),
                                             g.dist.astype(np.float64).tolist())]}
    with open(path, "w") as f:
        json.dump(doc, f)
