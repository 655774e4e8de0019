"""Test helper: the protocol of the risk field across tiles ("Risk fields across tiles"), restated
in numpy and plain Python apart from the engine -- tests/tiled_field_ref.py's loop (per rank: relax to quiescence,
publish the border keys that dropped, gather, merge into the ghosts, until an exchange without news; two passes;
parents as least global ids) under the extension (max(risk, r), hops + 1) over the edge risks r = w + 0.  The solve
graph is stated over IN-edges, so that a directed graph can be cut as well: a ghost is a remote node with an edge
into one of this rank's nodes, its row holds those edges, and a border node is one with an edge into another rank's
node.  On a symmetric graph that is tiled_field_ref.solve_graph's graph.  Test code only."""
from types import SimpleNamespace

import numpy as np

from field_keys import F32, INVALID, risk_values

NONE = None  # no key


def solve_graph(G, lo, hi):
    """The solve graph of the rank that owns the global rows [lo, hi) of the CSR dict G (rowptr, col, w, state)."""
    V = hi - lo
    rowptr, col = np.asarray(G["rowptr"], np.int64), np.asarray(G["col"], np.int64)
    risk = risk_values(G["w"])
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    mine_u, mine_v = (rows >= lo) & (rows < hi), (col >= lo) & (col < hi)
    ghosts = np.unique(rows[~mine_u & mine_v])
    index = lambda g: g - lo if lo <= g < hi else V + int(np.searchsorted(ghosts, g))  # noqa: E731
    edges = [[] for _ in range(V + len(ghosts))]  # per solve-graph row: (solve-graph column, risk)
    for k in np.flatnonzero(mine_v).tolist():  # (edges into a ghost are never relaxed: they are not even listed)
        edges[index(int(rows[k]))].append((int(col[k]) - lo, risk[k]))
    return SimpleNamespace(V=V, G=len(ghosts), lo=lo, ghosts=ghosts, edges=edges,
                           state=np.asarray(G["state"][lo:hi], np.int64),
                           gid_of=np.concatenate([np.arange(lo, hi), ghosts]).astype(np.int64),
                           border=np.unique(rows[mine_u & ~mine_v]) - lo)


def extend(key, r):
    return (r if r > key[0] else key[0], key[1] + 1)


def _relax(S, key, tight, queue):
    while queue:
        nxt = []
        for u in queue:
            if key[u] is NONE:
                continue
            for v, r in S.edges[u]:
                if S.state[v] == INVALID:
                    continue
                nk = extend(key[u], r)
                if tight is not None and not (tight[v] is not NONE and nk[0] == tight[v]):
                    continue
                if key[v] is NONE or nk < key[v]:
                    key[v] = nk
                    nxt.append(v)
        queue = nxt


def tiled_risk_field(G, offsets, members, passes=2):
    """One risk field of the global CSR dict G cut at `offsets` (R + 1 global ids), from every global id in `members`
    at (+0, 0), by the protocol.  passes=1: what pass 1 alone leaves (the hops of stale prefixes).
    -> (risk float32[V], hops int32[V], parent int32[V] global ids, info dict(exchanges=[per pass], ghosts,
    published={global id: times its key was published, over both passes}))."""
    R = len(offsets) - 1
    ranks = [solve_graph(G, int(offsets[t]), int(offsets[t + 1])) for t in range(R)]
    members = sorted({int(s) for s in np.atleast_1d(members)})
    tight = [None] * R
    exchanges, times = [], {}
    keys = None
    for p in range(passes):
        keys = [[NONE] * (S.V + S.G) for S in ranks]
        published = [{} for _ in ranks]
        queues = [[] for _ in ranks]
        for t, S in enumerate(ranks):
            for s in members:
                if S.lo <= s < S.lo + S.V:
                    keys[t][s - S.lo] = (F32(0.0), 0)
                    queues[t].append(s - S.lo)
        n_ex = 0
        while True:
            records = []  # (rank, global id, key)
            for t, S in enumerate(ranks):
                _relax(S, keys[t], tight[t], queues[t])
                for v in S.border.tolist():
                    k = keys[t][v]
                    if k is not NONE and (v not in published[t] or k < published[t][v]):
                        published[t][v] = k
                        records.append((t, S.lo + v, k))
                        times[S.lo + v] = times.get(S.lo + v, 0) + 1
            n_ex += 1
            if not records:
                break
            for t, S in enumerate(ranks):
                queues[t] = []
                for owner, gid, k in records:
                    if owner == t:
                        continue
                    j = int(np.searchsorted(S.ghosts, gid))
                    if j < S.G and S.ghosts[j] == gid and (keys[t][S.V + j] is NONE or k < keys[t][S.V + j]):
                        keys[t][S.V + j] = k
                        queues[t].append(S.V + j)
        exchanges.append(n_ex)
        if p == 0:
            tight = [[NONE if k is NONE else k[0] for k in keys[t]] for t in range(R)]
    V = int(offsets[-1])
    risk = np.full(V, np.inf, F32)
    hops = np.full(V, -1, np.int32)
    parent = np.full(V, -1, np.int32)
    for t, S in enumerate(ranks):
        for v in range(S.V):
            if keys[t][v] is not NONE:
                risk[S.lo + v], hops[S.lo + v] = keys[t][v]
        for u in range(S.V + S.G):  # the parent sweep, ghost rows included: the least GLOBAL id
            if keys[t][u] is NONE:
                continue
            for v, r in S.edges[u]:
                if S.state[v] == INVALID or keys[t][v] is NONE:
                    continue
                if extend(keys[t][u], r) == keys[t][v]:
                    g = int(S.gid_of[u])
                    if parent[S.lo + v] < 0 or g < parent[S.lo + v]:
                        parent[S.lo + v] = g
    return risk, hops, parent, dict(exchanges=exchanges, ghosts=[S.G for S in ranks], published=times)


def as_csr(g):
    """A FieldGraph (or anything with rowptr, col, w, state) as the CSR dict the protocol takes."""
    return dict(V=len(g.state), rowptr=np.asarray(g.rowptr, np.int64), col=np.asarray(g.col, np.int64),
                w=np.asarray(g.w, F32), state=np.asarray(g.state, np.int64))


def interleaved(g, R=2):
    """g with its nodes renumbered so that consecutive nodes alternate between R ranges: node p becomes
    (p % R) * ceil(V / R) + p // R where every range is full, packed otherwise -> (CSR dict, offsets, new id of p)."""
    V = len(g.state)
    order = sorted(range(V), key=lambda p: (p % R, p // R))  # new id -> old id
    new = np.empty(V, np.int64)
    new[order] = np.arange(V)
    rowptr, col, w = np.asarray(g.rowptr, np.int64), np.asarray(g.col, np.int64), np.asarray(g.w, F32)
    deg = np.diff(rowptr)[order]
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    take = np.concatenate([np.arange(rowptr[o], rowptr[o + 1]) for o in order]).astype(np.int64) if len(col) else col
    sizes = [len(range(r, V, R)) for r in range(R)]
    G = dict(V=V, rowptr=rp, col=new[col[take]], w=w[take], state=np.asarray(g.state, np.int64)[order])
    if hasattr(g, "dist"):
        G["dist"] = np.asarray(g.dist, F32)[take]
    return G, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), new


def staircase(steps=8, tail=3):
    """A border node reachable by `steps` disjoint walks through the other tile, of increasing seam crossings and
    strictly decreasing peak weight: walk j (0-based) runs source -> its own 2j + 1 inner nodes -> target, the inner
    nodes alternating between tile 1 and tile 0 (so 2j + 2 seam crossings, the last into the target from tile 1), every
    edge at weight 0.9 - 0.1 j.  The shorter walk arrives earlier and worse: the target's key drops once per walk, and
    every drop is published.  Behind the target a tail in tile 1 carries each drop on.
    -> (sizes, edges [(a, b, w, dist)], source gid, target gid); tile 0 holds the source and the target."""
    n0, n1 = [], []  # the walks' inner nodes per tile, as (walk, position)
    for j in range(steps):
        for i in range(2 * j + 1):
            (n1 if i % 2 == 0 else n0).append((j, i))
    gid = {("s",): 0, ("t",): 1}
    for q, key in enumerate(n0):
        gid[key] = 2 + q
    size0 = 2 + len(n0)
    for q, key in enumerate(n1):
        gid[key] = size0 + q
    base = size0 + len(n1)
    edges = []
    for j in range(steps):
        w = float(np.float32(0.9 - 0.1 * j))
        chain = [gid["s",]] + [gid[j, i] for i in range(2 * j + 1)] + [gid["t",]]
        edges += [(a, b, w, 1.0) for a, b in zip(chain, chain[1:])]
    edges += [(1 if i == 0 else base + i - 1, base + i, 0.0, 1.0) for i in range(tail)]
    return [size0, len(n1) + tail], edges, 0, 1
