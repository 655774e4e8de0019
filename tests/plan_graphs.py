"""Test helper: graphs on which planSafePath's answer hangs on the rounding order of its fp32 cost and on the order
of its heap -- what terrain graphs, with all weights distinct, never exercise.  Every family is ONE graph of disjoint
components set 100 m apart in a row, with the queries (start node, goal node) that go with it; nodes lie at least
1 m apart, far above robot_size, so a query placed on a node's coordinates resolves to that node alone.  Fixed seeds
throughout.  Test code only."""
import heapq
from collections import namedtuple

import numpy as np

import field_graphs as fg

F32 = np.float32
GAP = 100.0  # metres between the origins of neighbouring components

# graph: a field_graphs.FieldGraph; queries: (m, 2) int node ids (start, goal)
Family = namedtuple("Family", "graph queries")

Edge = namedtuple("Edge", "a b w dist")


def _assemble(parts):
    """parts: (pos (n, 3), edges [Edge with local ids], state (n,), queries [(start, goal) local]) per component, laid
    out along x, GAP apart.  A row holds a node's edges in the order the component lists them."""
    pos, src, dst, w, d, state, queries = [], [], [], [], [], [], []
    base = 0
    for c, (p, edges, st, qs) in enumerate(parts):
        p = np.asarray(p, np.float64) + np.array([c * GAP, 0.0, 0.0])
        pos.append(p)
        state.append(np.asarray(st, np.int32))
        src += [base + e.a for e in edges]
        dst += [base + e.b for e in edges]
        w += [e.w for e in edges]
        d += [e.dist for e in edges]
        queries += [(base + s, base + g) for s, g in qs]
        base += len(st)
    g = fg.from_edges(base, np.array(src, np.int64), np.array(dst, np.int64), np.array(w, np.float32),
                      np.array(d, np.float32), state=np.concatenate(state), pos=np.concatenate(pos))
    assert len(np.unique(g.pos.view(np.uint32).reshape(-1, 3), axis=0)) == base  # positions survive fp32, distinct
    return Family(g, np.array(queries, np.int32).reshape(-1, 2))


def _braid_nodes(K, M):
    """Layer k, strand j -> id k * M + j at (k, j, 0) metres."""
    k, j = np.meshgrid(np.arange(K), np.arange(M), indexing="ij")
    return np.stack([k.reshape(-1), j.reshape(-1), np.zeros(K * M)], axis=1)


def _length(ja, jb):
    """The fp32 Euclidean length of a step to the next layer from strand ja to strand jb."""
    return np.sqrt(F32(1.0) + F32(ja - jb) * F32(ja - jb), dtype=np.float32)


def braid(rng, K, M, n_weights):
    """K layers of M nodes on a 1 m lattice, all M x M edges between consecutive layers, both ways at the same
    weight; dist the fp32 Euclidean length; w one of n_weights values drawn for this braid.  Many routes tie as real
    numbers and differ only in the order their terms are rounded.  Query: middle strand, first to last layer."""
    palette = rng.uniform(0.1, 1.0, size=n_weights).astype(np.float32)
    edges = []
    for k in range(K - 1):
        for ja in range(M):
            for jb in range(M):
                a, b = k * M + ja, (k + 1) * M + jb
                ww = palette[int(rng.integers(0, n_weights))]
                edges.append(Edge(a, b, ww, _length(ja, jb)))
                edges.append(Edge(b, a, ww, _length(ja, jb)))
    return _braid_nodes(K, M), edges, np.zeros(K * M, np.int32), [(M // 2, (K - 1) * M + M // 2)]


# (seed, number of braids, K, M, distinct weights)
BRAIDS = {"k8m3": (3, 256, 8, 3, 2), "k16m4": (1, 128, 16, 4, 3)}


def braids(name):
    seed, n, K, M, nw = BRAIDS[name]
    rng = np.random.default_rng(seed)
    return _assemble([braid(rng, K, M, nw) for _ in range(n)])


def small_braid(seed=5201):
    """One K=5, M=2 braid with 2 weights: small enough to enumerate every simple route."""
    return _assemble([braid(np.random.default_rng(seed), 5, 2, 2)])


def _lattice(n, w):
    """n x n 4-connected lattice, 1 m pitch, dist 1 and the one weight w on every edge: every monotone route between
    two nodes ties in f and g, exactly."""
    ix, iy = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    ix, iy = ix.reshape(-1), iy.reshape(-1)
    edges = []
    for a in range(n * n):
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            x, y = ix[a] + dx, iy[a] + dy
            if 0 <= x < n and 0 <= y < n:
                edges.append(Edge(a, int(y * n + x), F32(w), F32(1.0)))
    pos = np.stack([ix, iy, np.zeros(n * n)], axis=1)
    return pos, edges, np.zeros(n * n, np.int32)


def exact_ties(n=12):
    """Two lattices, w = 0 and w = 0.3, and on each: corner to corner (both diagonals, both ways), edge midpoints
    across and along, interior pairs, neighbours, and start == goal."""
    at = lambda x, y: y * n + x
    h, e = n // 2, n - 1
    qs = [(at(0, 0), at(e, e)), (at(e, e), at(0, 0)), (at(e, 0), at(0, e)), (at(0, e), at(e, 0)),
          (at(0, 0), at(e, 0)), (at(h, 0), at(h, e)), (at(0, h), at(e, h)), (at(h, 0), at(e, h)),
          (at(3, 4), at(8, 7)), (at(8, 2), at(2, 9)), (at(5, 5), at(6, 6)), (at(4, 7), at(5, 7)),
          (at(5, 5), at(5, 5)), (at(0, 0), at(0, 0))]
    return _assemble([(*_lattice(n, 0.0), qs), (*_lattice(n, 0.3), qs)])


def _cheapest_route(V, edges, state, sf, start, goal):
    """Dijkstra in double on the component (graph construction only: where to put the Invalid nodes)."""
    rows = [[] for _ in range(V)]
    for e in edges:
        rows[e.a].append((e.b, (sf * float(e.w) + 1.0) * float(e.dist)))
    best, prev, heap = {start: 0.0}, {}, [(0.0, start)]
    while heap:
        c, u = heapq.heappop(heap)
        if c > best[u]:
            continue
        for v, ec in rows[u]:
            if state[v] != fg.INVALID and c + ec < best.get(v, np.inf):
                best[v], prev[v] = c + ec, u
                heapq.heappush(heap, (c + ec, v))
    route = [goal]
    while route[-1] != start:
        route.append(prev[route[-1]])
    return route[::-1]


def asymmetric_braid(rng, cut_off=False, K=6, M=3, sf=3.0):
    """A K=6, M=3 braid in which the two directions of an edge differ in w and dist, a fifth of the backward edges is
    missing (the path summary then finds no edge from child to parent), a sixth of the edges has a parallel twin, the
    dearer one first in the row, and one or two inner nodes of the otherwise cheapest route are Invalid.  cut_off:
    nothing joins the last layer to the rest, so the goal cannot be reached."""
    palette = rng.uniform(0.1, 1.0, size=3).astype(np.float32)
    stretch = np.array([1.0, 1.0, 1.125, 1.5], np.float32)  # dist >= the Euclidean length: the heuristic stays below

    def draw(ja, jb):
        return palette[int(rng.integers(0, 3))], F32(_length(ja, jb) * stretch[int(rng.integers(0, 4))])

    def push(edges, a, b, ja, jb):
        ww, dd = draw(ja, jb)
        if rng.uniform() < 1.0 / 6.0:
            w2, d2 = draw(ja, jb)
            cost = lambda x, y: (sf * float(x) + 1.0) * float(y)
            first, second = ((ww, dd), (w2, d2)) if cost(ww, dd) >= cost(w2, d2) else ((w2, d2), (ww, dd))
            edges.append(Edge(a, b, *first))
            edges.append(Edge(a, b, *second))
        else:
            edges.append(Edge(a, b, ww, dd))

    edges = []
    for k in range(K - 1 - (1 if cut_off else 0)):
        for ja in range(M):
            for jb in range(M):
                a, b = k * M + ja, (k + 1) * M + jb
                push(edges, a, b, ja, jb)
                if rng.uniform() >= 0.2:
                    push(edges, b, a, ja, jb)
    state = np.zeros(K * M, np.int32)
    start, goal = M // 2, (K - 1) * M + M // 2
    if not cut_off:
        for _ in range(int(rng.integers(1, 3))):
            inner = _cheapest_route(K * M, edges, state, sf, start, goal)[1:-1]
            state[inner[int(rng.integers(0, len(inner)))]] = fg.INVALID
    return _braid_nodes(K, M), edges, state, [(start, goal), (goal, start)]


N_ASYMMETRIC = 47  # and one more, cut off


def asymmetric(seed=6301):
    """N_ASYMMETRIC asymmetric braids, queried both ways (backwards there may be no route), and a last one whose
    goal layer is cut off: queries[-2:] are the ones that must find nothing."""
    rng = np.random.default_rng(seed)
    parts = [asymmetric_braid(rng) for _ in range(N_ASYMMETRIC)] + [asymmetric_braid(rng, cut_off=True)]
    return _assemble(parts)


def all_simple_routes(g, start, goal):
    """Every simple route start -> goal over valid nodes, as lists of node ids (tiny graphs only)."""
    out = []

    def walk(route, seen):
        u = route[-1]
        if u == goal:
            out.append(list(route))
            return
        for v in sorted(set(g.col[g.rowptr[u]:g.rowptr[u + 1]].tolist())):
            if v not in seen and g.state[v] != fg.INVALID:
                seen.add(v)
                route.append(v)
                walk(route, seen)
                route.pop()
                seen.discard(v)

    walk([start], {start})
    return out
