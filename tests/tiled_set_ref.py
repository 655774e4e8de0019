"""Test helper: the protocol of source sets across tiles ("Source sets across tiles"), restated
in numpy and plain Python apart from the engine, on tests/tiled_field_ref.py's solve graphs:

seeding      a rank seeds only the entries whose member is its own node, at their start costs; a member that is a
             ghost mirrors its owner's key.  Pass 1: the least start cost per item.  Pass 2: only the entries whose
             start-cost bits are the item's pass-1 cost -- the roots, marked with their least GLOBAL entry index;
two passes   tiled_field_ref's loop of relaxation, publish, gather and merge until an exchange without news;
parents      the least GLOBAL id among the tight predecessors, ghost rows included; a root has none;
owner loop   per rank the first ancestors (a root and a ghost with a key are terminals), jumped to a fixed point; then
             exchanges: merge foreign owner records into the ghosts, every item takes its final ancestor's owner where
             known, publish every border item whose owner became known, ONCE; ends on an exchange without news.
Test code only."""
import numpy as np

import tiled_field_ref as tr

F32 = np.float32
NONE = tr.NONE


def bits(x):
    return int(np.asarray(x, F32).reshape(1).view(np.uint32)[0])


def tiled_set_field(G, offsets, sf, members, c0=None):
    """One set field of the global CSR dict G cut at `offsets`, from the global ids `members` at the start costs `c0`
    (None: +0 each), by the protocol -> dict(cost float32[V], hops, parent (global ids), owner int32[V], owned [R, n]
    per rank, exchanges [pass 1, pass 2], owner_exchanges, owner_news (records per owner exchange), roots per rank)."""
    members = [int(s) for s in members]
    n = len(members)
    c0 = (np.zeros(n, F32) if c0 is None else np.asarray(c0, F32).reshape(-1) + F32(0.0)).astype(F32)
    R = len(offsets) - 1
    ranks = [tr.solve_graph(G, int(offsets[t]), int(offsets[t + 1])) for t in range(R)]
    ecs = [tr._edge_costs(S, sf) for S in ranks]
    # per rank: the entries it seeds (global entry index, local id, start cost)
    entries = [[(j, members[j] - S.lo, c0[j]) for j in range(n) if S.lo <= members[j] < S.lo + S.V] for S in ranks]
    tight = [None] * R
    exchanges = []
    keys = mark = None
    for p in range(2):
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
            records = []
            for t, S in enumerate(ranks):
                tr._relax(S, ecs[t], keys[t], tight[t], queues[t])
                for v in S.border:
                    k = keys[t][v]
                    if k is not NONE and (v not in published[t] or k < published[t][v]):
                        published[t][v] = k
                        records.append((t, S.lo + int(v), k))
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
    cost = np.full(V, np.inf, F32)
    hops = np.full(V, -1, np.int32)
    parent = np.full(V, -1, np.int32)
    for t, S in enumerate(ranks):
        for v in range(S.V):
            if keys[t][v] is not NONE:
                cost[S.lo + v], hops[S.lo + v] = keys[t][v]
        for u in range(S.V + S.G):
            if keys[t][u] is NONE:
                continue
            a, h = keys[t][u]
            for k in range(S.rowptr[u], S.rowptr[u + 1]):
                v = int(S.col[k])
                if S.state[v] == tr.INVALID or keys[t][v] is NONE:
                    continue
                if (F32(a + ecs[t][k]), h + 1) == keys[t][v]:
                    g = int(S.gid_of[u])
                    if parent[S.lo + v] < 0 or g < parent[S.lo + v]:
                        parent[S.lo + v] = g
    # a root's mark survived pass 2: its key (c0, 0) equals no extension, so it has no parent
    for t, S in enumerate(ranks):
        for v in mark[t]:
            assert keys[t][v][1] == 0 and parent[S.lo + v] == -1
    # ---- the owner loop -----------------------------------------------------------------------------------------
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
            for v in S.border:
                if o[v] >= 0 and int(v) not in sent[t]:
                    sent[t].add(int(v))
                    records.append((t, S.lo + int(v), int(o[v])))
        news.append(len(records))
        if not records:
            break
        incoming = records
    owner = np.full(V, -1, np.int32)
    owned = np.zeros((R, n), np.int32)
    for t, S in enumerate(ranks):
        owner[S.lo:S.lo + S.V] = own[t][:S.V]
        mine = own[t][:S.V]
        owned[t] = np.bincount(mine[mine >= 0], minlength=n)
    return dict(cost=cost, hops=hops, parent=parent, owner=owner, owned=owned, exchanges=exchanges,
                owner_exchanges=len(news), owner_news=news, roots=[len(m) for m in mark])
