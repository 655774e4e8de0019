"""Test helper: the protocol of the fields across tiles ("Cost fields", "Source sets" and "Risk
fields across tiles"), restated once in numpy and plain Python apart from the engine.

solve graph  per rank its nodes, then its ghosts in ascending global id; stated over IN-edges, so that a directed graph
             can be cut as well: a ghost is a remote node with an edge into one of this rank's nodes, its row holds
             those edges, and a border node is one with an edge into another rank's node.  Edges into ghosts are never
             relaxed: they are not even listed;
objective    the edge values (field_keys.cost_values or risk_values) and how one extends a key (value, hops):
             (fl(cost + c), hops + 1) or (max(risk, r), hops + 1);
seeding      a rank seeds only the entries whose member is its own node, at their start values; a member that is a
             ghost mirrors its owner's key.  Pass 1: the least start value per item.  Pass 2: only the entries whose
             start bits are the item's pass-1 word -- the roots, marked with their least GLOBAL entry index.  A single
             source is a set of one at +0, a risk member set a set at +0;
two passes   in each the loop of local relaxation to quiescence, publish of the border keys that dropped, gather, merge
             into the ghosts, until an exchange without news; pass 2 relaxes only into pass 1's words;
parents      the least GLOBAL id among the tight predecessors, ghost rows included; a root has none;
owner loop   per rank the first ancestors (a root and a ghost with a key are terminals), jumped to a fixed point; then
             exchanges: merge foreign owner records into the ghosts, every item takes its final ancestor's owner where
             known, publish every border item whose owner became known, ONCE; ends on an exchange without news.
Test code only."""
from types import SimpleNamespace

import numpy as np

from field_keys import F32, INVALID, cost_values, risk_values

NONE = None  # no key


def bits(x):
    return int(np.asarray(x, F32).reshape(1).view(np.uint32)[0])


def solve_graph(G, lo, hi):
    """The solve graph of the rank that owns the global rows [lo, hi) of the CSR dict G (rowptr, col, w, state and,
    for costs and routes, dist; global column ids)."""
    V = hi - lo
    rowptr, col = np.asarray(G["rowptr"], np.int64), np.asarray(G["col"], np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    mine_u, mine_v = (rows >= lo) & (rows < hi), (col >= lo) & (col < hi)
    ghosts = np.unique(rows[~mine_u & mine_v])  # sorted, distinct
    k = np.flatnonzero(mine_v)
    row = np.where(mine_u[k], rows[k] - lo, V + np.searchsorted(ghosts, rows[k]))
    k = k[np.argsort(row, kind="stable")]  # (a row keeps the order of its edges in G)
    return SimpleNamespace(
        V=V, G=len(ghosts), lo=lo, ghosts=ghosts,
        rowptr=np.concatenate([[0], np.cumsum(np.bincount(row, minlength=V + len(ghosts)))]).astype(np.int64),
        col=col[k] - lo, w=np.asarray(G["w"], F32)[k], dist=np.asarray(G["dist"], F32)[k] if "dist" in G else None,
        state=np.asarray(G["state"][lo:hi], np.int64),
        gid_of=np.concatenate([np.arange(lo, hi), ghosts]).astype(np.int64),
        border=np.unique(rows[mine_u & ~mine_v]) - lo)


def cost(sf):
    """the objective of the cost field under the safety factor sf"""
    return lambda S: cost_values(S.w, S.dist, sf), lambda key, c: (F32(key[0] + c), key[1] + 1)


RISK = lambda S: risk_values(S.w), lambda key, r: (r if r > key[0] else key[0], key[1] + 1)  # noqa: E731


def _relax(S, values, extend, key, tight, queue):
    """Label-correcting relaxation of one rank from the queued items to quiescence; keys are (value, hops)."""
    while queue:
        nxt = []
        for u in queue:
            if key[u] is NONE:
                continue
            for k in range(S.rowptr[u], S.rowptr[u + 1]):
                v = int(S.col[k])
                if S.state[v] == INVALID:
                    continue
                nk = extend(key[u], values[k])
                if tight is not None and not (tight[v] is not NONE and nk[0] == tight[v]):
                    continue
                if key[v] is NONE or nk < key[v]:
                    key[v] = nk
                    nxt.append(v)
        queue = nxt


def solve(G, offsets, objective, members, starts=None, passes=2, owners=False):
    """One field of the global CSR dict G cut at `offsets` (R + 1 global ids) under `objective` (cost(sf) or RISK), from
    the global ids `members` at the start values `starts` (None: +0 each), by the protocol.  passes=1: what pass 1
    alone leaves (the hops of stale prefixes).  owners: run the owner loop as well.
    -> (value float32[V], hops int32[V], parent int32[V] global ids, info dict(exchanges [per pass], ghosts per rank,
    published {global id: times its key was published, over the passes}, roots per rank; with owners: owner int32[V],
    owned [R, n] per rank, owner_exchanges, owner_news (records per owner exchange)))."""
    members = [int(s) for s in np.atleast_1d(members)]
    n = len(members)
    c0 = (np.zeros(n, F32) if starts is None else np.asarray(starts, F32).reshape(-1) + F32(0.0)).astype(F32)
    R = len(offsets) - 1
    ranks = [solve_graph(G, int(offsets[t]), int(offsets[t + 1])) for t in range(R)]
    values, extend = [objective[0](S) for S in ranks], objective[1]
    # per rank: the entries it seeds (global entry index, local id, start value)
    entries = [[(j, members[j] - S.lo, c0[j]) for j in range(n) if S.lo <= members[j] < S.lo + S.V] for S in ranks]
    tight = [None] * R
    exchanges, times = [], {}
    keys = mark = None
    for p in range(passes):
        keys = [[NONE] * (S.V + S.G) for S in ranks]
        mark = [{} for _ in ranks]  # local id -> least entry that seeded it (pass 2: the roots)
        published = [{} for _ in ranks]
        queues = [[] for _ in ranks]
        for t in range(R):
            for j, v, c in entries[t]:
                if p == 1 and bits(c) != bits(tight[t][v]):
                    continue
                k = (F32(c), 0)
                if keys[t][v] is NONE or k < keys[t][v]:
                    keys[t][v] = k
                if v not in mark[t]:
                    mark[t][v] = j  # (entries ascend: the first is the least)
                    queues[t].append(v)
        n_ex = 0
        while True:
            records = []  # (rank, global id, key)
            for t, S in enumerate(ranks):
                _relax(S, values[t], extend, keys[t], tight[t], queues[t])
                for v in S.border.tolist():
                    k = keys[t][v]
                    if k is not NONE and (v not in published[t] or k < published[t][v]):
                        published[t][v] = k
                        records.append((t, S.lo + v, k))
                        times[S.lo + v] = times.get(S.lo + v, 0) + 1
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
        if p == 0:  # the tight words: every item's least value, the ghosts' from their mirrored final values
            tight = [[NONE if k is NONE else k[0] for k in keys[t]] for t in range(R)]
    V = int(offsets[-1])
    value = np.full(V, np.inf, F32)
    hops = np.full(V, -1, np.int32)
    parent = np.full(V, -1, np.int32)
    for t, S in enumerate(ranks):
        for v in range(S.V):
            if keys[t][v] is not NONE:
                value[S.lo + v], hops[S.lo + v] = keys[t][v]
        # the parent sweep, ghost rows included: the least GLOBAL id among the tight predecessors
        for u in range(S.V + S.G):
            if keys[t][u] is NONE:
                continue
            for k in range(S.rowptr[u], S.rowptr[u + 1]):
                v = int(S.col[k])
                if S.state[v] == INVALID or keys[t][v] is NONE:
                    continue
                if extend(keys[t][u], values[t][k]) == keys[t][v]:
                    g = int(S.gid_of[u])
                    if parent[S.lo + v] < 0 or g < parent[S.lo + v]:
                        parent[S.lo + v] = g
    info = dict(exchanges=exchanges, ghosts=[S.G for S in ranks], published=times, roots=[len(m) for m in mark])
    if not owners:
        return value, hops, parent, info
    # a root's mark survived pass 2: its key (start, 0) equals no extension, so it has no parent
    for t, S in enumerate(ranks):
        for v in mark[t]:
            assert keys[t][v][1] == 0 and parent[S.lo + v] == -1
    # ---- the owner loop ---------------------------------------------------------------------------------------------
    anc, own = [], []
    for t, S in enumerate(ranks):
        a = np.full(S.V + S.G, -1, np.int64)
        o = np.full(S.V + S.G, -1, np.int64)
        for i in range(S.V + S.G):
            if keys[t][i] is NONE:
                continue
            if i >= S.V:
                a[i] = i  # a ghost: a terminal, only its owning rank knows its owner
            elif i in mark[t]:
                a[i] = i
                o[i] = mark[t][i]
            else:
                gp = int(parent[S.lo + i])
                if S.lo <= gp < S.lo + S.V:
                    a[i] = gp - S.lo
                else:
                    j = int(np.searchsorted(S.ghosts, gp))
                    assert j < S.G and S.ghosts[j] == gp
                    a[i] = S.V + j
        while True:  # pointer jumping until a sweep moves nothing
            b = np.where(a >= 0, a[np.maximum(a, 0)], -1)
            if np.array_equal(a, b):
                break
            a = b
        anc.append(a)
        own.append(o)
    sent = [set() for _ in ranks]
    news, incoming = [], []
    while True:
        records = []
        for t, S in enumerate(ranks):
            for src, gid, o in incoming:
                if src == t:
                    continue
                j = int(np.searchsorted(S.ghosts, gid))
                if j < S.G and S.ghosts[j] == gid:
                    own[t][S.V + j] = o
            a, o = anc[t], own[t]
            take = (o < 0) & (a >= 0)
            o[take] = o[a[take]]  # (anchors are terminals: what is read is not written here)
            for v in S.border.tolist():
                if o[v] >= 0 and v not in sent[t]:
                    sent[t].add(v)
                    records.append((t, S.lo + v, int(o[v])))
        news.append(len(records))
        if not records:
            break
        incoming = records
    owner = np.full(V, -1, np.int32)
    owned = np.zeros((R, n), np.int32)
    for t, S in enumerate(ranks):
        mine = own[t][:S.V]
        owner[S.lo:S.lo + S.V] = mine
        owned[t] = np.bincount(mine[mine >= 0], minlength=n)
    return value, hops, parent, dict(info, owner=owner, owned=owned, owner_exchanges=len(news), owner_news=news)


# ---- the entries under their earlier names --------------------------------------------------------------------------

def tiled_field(G, offsets, sf, src):
    """One cost field from the global id `src` -> (cost, hops, parent, info)."""
    return solve(G, offsets, cost(sf), [src])


def tiled_risk_field(G, offsets, members, passes=2):
    """One risk field from every global id in `members` at (+0, 0), seeded in ascending order (pass 1's hops, and with
    them its publish counts, depend on the order of relaxation) -> (risk, hops, parent, info)."""
    return solve(G, offsets, RISK, sorted({int(s) for s in np.atleast_1d(members)}), passes=passes)


def tiled_set_field(G, offsets, sf, members, c0=None):
    """One cost field from `members` at the start costs `c0`, with owners -> the info dict plus cost, hops, parent."""
    value, hops, parent, info = solve(G, offsets, cost(sf), members, c0, owners=True)
    return dict(info, cost=value, hops=hops, parent=parent)


def single_pass_hops(V, rowptr, col, w, dist, state, sf, src):
    """What ONE label-correcting pass on the key (cost, hops) over all edges leaves, relaxing in FIFO order from the
    source: the hops of a stale, dearer prefix survive where fl(a + c) == fl(a' + c)."""
    ec = cost_values(w, dist, sf)
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
