"""Test helper: the protocol of the cost field across tiles ("Cost fields across tiles"),
restated in numpy and plain Python apart from the engine: per rank the solve graph (local nodes, then ghosts in
ascending global id, reverse edges in the ghost rows, edges into ghosts never relaxed), the two passes, and in each
the loop of local relaxation to quiescence, publish of the border keys that dropped, gather, merge into the ghosts,
until an exchange without news; parents as least global ids.  Test code only."""
from types import SimpleNamespace

import numpy as np

from field_keys import F32, INVALID, cost_values  # noqa: F401

NONE = None  # no key


def solve_graph(G, lo, hi):
    """The solve graph of the rank that owns the global rows [lo, hi) of the CSR dict G (rowptr, col, w, dist,
    state; global column ids)."""
    V = hi - lo
    e0, e1 = int(G["rowptr"][lo]), int(G["rowptr"][hi])
    col = np.asarray(G["col"][e0:e1], np.int64)
    remote = (col < lo) | (col >= hi)
    ghosts = np.unique(col[remote])  # sorted, distinct
    rowptr = np.asarray(G["rowptr"][lo:hi + 1], np.int64) - e0
    rows = np.repeat(np.arange(V), np.diff(rowptr))
    col2 = np.where(remote, V + np.searchsorted(ghosts, col), col - lo)
    w, d = np.asarray(G["w"][e0:e1], F32), np.asarray(G["dist"][e0:e1], F32)
    # ghost rows: the reverse of every cross edge that names the ghost, same weight and length
    gj = col2[remote] - V
    order = np.argsort(gj, kind="stable")
    deg = np.bincount(gj, minlength=len(ghosts))
    return SimpleNamespace(
        V=V, G=len(ghosts), lo=lo, ghosts=ghosts,
        rowptr=np.concatenate([rowptr, rowptr[-1] + np.cumsum(deg)]).astype(np.int64),
        col=np.concatenate([col2, rows[remote][order]]).astype(np.int64),
        w=np.concatenate([w, w[remote][order]]), dist=np.concatenate([d, d[remote][order]]),
        # a ghost is Invalid HERE: no edge into it is relaxed, its key only mirrors its owner's
        state=np.concatenate([np.asarray(G["state"][lo:hi], np.int64), np.full(len(ghosts), INVALID, np.int64)]),
        gid_of=np.concatenate([np.arange(lo, hi), ghosts]).astype(np.int64),
        border=np.unique(rows[remote]))


def _edge_costs(S, sf):
    return cost_values(S.w, S.dist, sf)


def _relax(S, ec, key, tight, queue):
    """Label-correcting relaxation of one rank from the queued items to quiescence; keys are (cost, hops)."""
    rounds = 0
    while queue:
        rounds += 1
        nxt = []
        for u in queue:
            if key[u] is NONE:
                continue
            a, h = key[u]
            for k in range(S.rowptr[u], S.rowptr[u + 1]):
                v = int(S.col[k])
                if S.state[v] == INVALID:
                    continue
                nk = (F32(a + ec[k]), h + 1)
                if tight is not None and not (tight[v] is not NONE and nk[0] == tight[v]):
                    continue
                if key[v] is NONE or nk < key[v]:
                    key[v] = nk
                    nxt.append(v)
        queue = nxt
    return rounds


def tiled_field(G, offsets, sf, src):
    """One field of the global CSR dict G cut at `offsets` (R + 1 global ids), from global id `src`, by the protocol.
    -> (cost float32[V], hops int32[V], parent int32[V] global ids, info dict(exchanges=[pass 1, pass 2], ghosts))."""
    R = len(offsets) - 1
    ranks = [solve_graph(G, int(offsets[t]), int(offsets[t + 1])) for t in range(R)]
    ecs = [_edge_costs(S, sf) for S in ranks]
    tight = [None] * R
    exchanges = []
    keys = None
    for p in range(2):
        keys = [[NONE] * (S.V + S.G) for S in ranks]
        published = [{} for _ in ranks]
        queues = [[] for _ in ranks]
        for t, S in enumerate(ranks):
            if S.lo <= src < S.lo + S.V:
                keys[t][src - S.lo] = (F32(0.0), 0)
                queues[t] = [src - S.lo]
        n_ex = 0
        while True:
            records = []  # (rank, global id, key)
            for t, S in enumerate(ranks):
                _relax(S, ecs[t], keys[t], tight[t], queues[t])
                for v in S.border:
                    k = keys[t][v]
                    if k is not NONE and (v not in published[t] or k < published[t][v]):
                        published[t][v] = k
                        records.append((t, S.lo + int(v), k))
            n_ex += 1
            if not records:  # (a rank with nothing to send stayed in the loop: it may still receive)
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
        if p == 0:  # the tight words: every item's least cost, the ghosts' from their mirrored final costs
            tight = [[NONE if k is NONE else k[0] for k in keys[t]] for t in range(R)]
    V = int(offsets[-1])
    cost = np.full(V, np.inf, F32)
    hops = np.full(V, -1, np.int32)
    parent = np.full(V, -1, np.int32)
    for t, S in enumerate(ranks):
        for v in range(S.V):
            if keys[t][v] is not NONE:
                cost[S.lo + v], hops[S.lo + v] = keys[t][v]
        # the parent sweep, ghost rows included: the least GLOBAL id among the tight predecessors
        for u in range(S.V + S.G):
            if keys[t][u] is NONE:
                continue
            a, h = keys[t][u]
            for k in range(S.rowptr[u], S.rowptr[u + 1]):
                v = int(S.col[k])
                if S.state[v] == INVALID or keys[t][v] is NONE:
                    continue
                if (F32(a + ecs[t][k]), h + 1) == keys[t][v]:
                    g = int(S.gid_of[u])
                    if parent[S.lo + v] < 0 or g < parent[S.lo + v]:
                        parent[S.lo + v] = g
    return cost, hops, parent, dict(exchanges=exchanges, ghosts=[S.G for S in ranks])


def single_pass_hops(V, rowptr, col, w, dist, state, sf, src):
    """What ONE label-correcting pass on the key (cost, hops) over all edges leaves, relaxing in FIFO order from the
    source: the hops of a stale, dearer prefix survive where fl(a + c) == fl(a' + c)."""
    ec = (F32(sf) * np.asarray(w, F32) + F32(1.0)) * np.asarray(dist, F32)
    key = [NONE] * V
    key[src] = (F32(0.0), 0)
    queue = [src]
    while queue:
        u = queue.pop(0)
        a, h = key[u]
        for k in range(rowptr[u], rowptr[u + 1]):
            v = int(col[k])
            if state[v] == INVALID:
                continue
            nk = (F32(a + ec[k]), h + 1)
            if key[v] is NONE or nk < key[v]:
                key[v] = nk
                queue.append(v)
    return np.array([-1 if k is NONE else k[1] for k in key], np.int32)


def symmetric_graph(rng, V, blocks=None):
    """A random symmetric graph as a CSR dict: every edge both ways with one weight and length, no duplicate pairs
    (the stitched graph's conditions); zero-length and sub-ulp edges, a few Invalid nodes.  blocks: id ranges
    [(lo, hi), ...] that link only among themselves (a tile without cross edges)."""
    blocks = blocks or []
    sealed = np.zeros(V, bool)
    for lo, hi in blocks:
        sealed[lo:hi] = True
    pairs = {}
    free = np.flatnonzero(~sealed)
    for _ in range(3 * V):
        a, b = (int(x) for x in rng.choice(free, 2)) if free.size > 1 else (0, 0)
        if a != b:
            pairs.setdefault((min(a, b), max(a, b)), None)
    for lo, hi in blocks:
        for _ in range(2 * (hi - lo)):
            a, b = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
            if a != b:
                pairs.setdefault((min(a, b), max(a, b)), None)
    src, dst, w, d = [], [], [], []
    for a, b in pairs:
        ww = F32(rng.choice([0.0, rng.uniform(0.1, 1.0)]))
        dd = F32(rng.choice([0.0, 1e-9, rng.uniform(0.3, 0.6), rng.uniform(100.0, 200.0)], p=[0.1, 0.1, 0.6, 0.2]))
        src += [a, b]
        dst += [b, a]
        w += [ww, ww]
        d += [dd, dd]
    state = np.zeros(V, np.int32)
    state[rng.choice(V, size=max(1, V // 10), replace=False)] = INVALID
    order = np.lexsort((np.array(dst), np.array(src)))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(np.array(src), minlength=V))]).astype(np.int64)
    return dict(V=V, rowptr=rowptr, col=np.array(dst, np.int64)[order], w=np.array(w, F32)[order],
                dist=np.array(d, F32)[order], state=state)
