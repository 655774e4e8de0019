"""Test helper: the protocol of the bounded fields across tiles ("Bounded fields across tiles"),
restated in plain Python on tiled_ref's solve graph, apart from the engine.

pass 1       every rank keeps its own copy of the field's bound, the budget at first.  Per exchange: the gathered bound
             records lower the bound (ANY: the least value; ALL: the rank's place in a table that starts at +inf for a
             rank that owns a settle target and at 0 for one that owns none, then the greatest entry), the gathered keys
             go into the ghosts, the rank relaxes to quiescence WITHOUT expanding an item above the bound or writing an
             extension above it, takes the least (ANY) or greatest (ALL; +inf when one has no key) value of its own
             settle targets -- ANY lowers its bound at once -- and tells it in a bound record when it is below what it
             told last; then it publishes the border keys that dropped and lie within the bound.  A bound record is news.
             The loop ends at the first exchange without news; every rank then holds the same bound.
trim         every key above the bound goes, ghosts included; what is left gives pass 2 its tight words.
pass 2 on    tiled_ref's: tight edges only, the parent sweep, the owner loop, all on the truncated keys.
Test code only."""
import numpy as np

from bound_ref import INF
from field_keys import F32, INVALID
from tiled_ref import NONE, _relax, bits, solve_graph


def _relax_bounded(S, values, extend, key, bound, queue):
    """tiled_ref._relax of pass 1 under `bound`: an item above it is not expanded, an extension above it not written."""
    while queue:
        nxt = []
        for u in queue:
            if key[u] is NONE or key[u][0] > bound:
                continue
            for k in range(S.rowptr[u], S.rowptr[u + 1]):
                v = int(S.col[k])
                if S.state[v] == INVALID:
                    continue
                nk = extend(key[u], values[k])
                if nk[0] > bound:
                    continue
                if key[v] is NONE or nk < key[v]:
                    key[v] = nk
                    nxt.append(v)
        queue = nxt


def solve(G, offsets, objective, members, starts=None, budget=INF, mode=None, targets=(), owners=False):
    """One bounded field of the global CSR dict G cut at `offsets` under `objective` (tiled_ref.cost(sf) or RISK) from
    the global ids `members` at `starts`, by the protocol: budget, and the settle `mode` (None, "any", "all") over the
    global ids `targets`.  -> (value, hops, parent, info dict(bound, exchanges [per pass], records [per rank: key
    records published], bound_records; with owners: owner, owned [R, n]))."""
    members = [int(s) for s in np.atleast_1d(members)]
    targets = [int(t) for t in np.atleast_1d(np.asarray(targets, np.int64))] if mode is not None else []
    n = len(members)
    c0 = (np.zeros(n, F32) if starts is None else np.asarray(starts, F32).reshape(-1) + F32(0.0)).astype(F32)
    R = len(offsets) - 1
    ranks = [solve_graph(G, int(offsets[t]), int(offsets[t + 1])) for t in range(R)]
    values, extend = [objective[0](S) for S in ranks], objective[1]
    entries = [[(j, members[j] - S.lo, c0[j]) for j in range(n) if S.lo <= members[j] < S.lo + S.V] for S in ranks]
    mine = [[g - S.lo for g in targets if S.lo <= g < S.lo + S.V] for S in ranks]  # the settle targets per rank
    bound = [F32(budget)] * R
    told = [INF] * R
    table = [[INF if mine[r] else F32(0.0) for r in range(R)] for _ in range(R)]  # every rank's copy
    tight = [None] * R
    exchanges, sent, bound_records = [], [0] * R, 0
    keys = mark = None
    for p in range(2):
        keys = [[NONE] * (S.V + S.G) for S in ranks]
        mark = [{} for _ in ranks]
        published = [{} for _ in ranks]
        queues = [[] for _ in ranks]
        for t in range(R):
            for j, v, c in entries[t]:
                if p == 1 and (tight[t][v] is NONE or bits(c) != bits(tight[t][v])):
                    continue
                k = (F32(c), 0)
                if keys[t][v] is NONE or k < keys[t][v]:
                    keys[t][v] = k
                if v not in mark[t]:
                    mark[t][v] = j
                    queues[t].append(v)
        n_ex = 0
        while True:
            records, news = [], []  # (rank, global id, key) and (rank, value)
            for t, S in enumerate(ranks):
                if p == 0:
                    _relax_bounded(S, values[t], extend, keys[t], bound[t], queues[t])
                    if mine[t]:
                        vals = [INF if keys[t][v] is NONE else keys[t][v][0] for v in mine[t]]
                        v = F32(min(vals) if mode == "any" else max(vals))
                        if mode == "any" and v < bound[t]:
                            bound[t] = v
                        if v < told[t]:
                            told[t] = v
                            news.append((t, v))
                else:
                    _relax(S, values[t], extend, keys[t], tight[t], queues[t])
                for v in S.border.tolist():
                    k = keys[t][v]
                    if k is NONE or not (v not in published[t] or k < published[t][v]):
                        continue
                    if p == 0 and k[0] > bound[t]:
                        continue
                    published[t][v] = k
                    records.append((t, S.lo + v, k))
                    sent[t] += 1
            n_ex += 1
            bound_records += len(news)
            if not records and not news:
                break
            for t, S in enumerate(ranks):
                for r, v in news:  # (a rank's own records included)
                    if mode == "any":
                        bound[t] = min(bound[t], v)
                    else:
                        table[t][r] = v
                if mode == "all" and news:
                    bound[t] = min(bound[t], max(table[t]))
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
            assert len({bits(b) for b in bound}) == 1, bound  # every rank holds the same bound
            for t in range(R):
                keys[t] = [NONE if k is NONE or k[0] > bound[t] else k for k in keys[t]]
            tight = [[NONE if k is NONE else k[0] for k in keys[t]] for t in range(R)]
    V = int(offsets[-1])
    value = np.full(V, np.inf, F32)
    hops = np.full(V, -1, np.int32)
    parent = np.full(V, -1, np.int32)
    for t, S in enumerate(ranks):
        for v in range(S.V):
            if keys[t][v] is not NONE:
                value[S.lo + v], hops[S.lo + v] = keys[t][v]
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
    info = dict(bound=bound[0], exchanges=exchanges, records=sent, bound_records=bound_records)
    if not owners:
        return value, hops, parent, info
    # ---- the owner loop of tiled_ref.solve, on the truncated keys -----------------------------------------------------
    anc, own = [], []
    for t, S in enumerate(ranks):
        a = np.full(S.V + S.G, -1, np.int64)
        o = np.full(S.V + S.G, -1, np.int64)
        for i in range(S.V + S.G):
            if keys[t][i] is NONE:
                continue
            if i >= S.V or i in mark[t]:
                a[i] = i
                if i < S.V:
                    o[i] = mark[t][i]
            else:
                gp = int(parent[S.lo + i])
                a[i] = gp - S.lo if S.lo <= gp < S.lo + S.V else S.V + int(np.searchsorted(S.ghosts, gp))
        while True:
            b = np.where(a >= 0, a[np.maximum(a, 0)], -1)
            if np.array_equal(a, b):
                break
            a = b
        anc.append(a)
        own.append(o)
    done = [set() for _ in ranks]
    incoming = []
    while True:
        records = []
        for t, S in enumerate(ranks):
            for src, gid, o in incoming:
                j = int(np.searchsorted(S.ghosts, gid))
                if src != t and j < S.G and S.ghosts[j] == gid:
                    own[t][S.V + j] = o
            a, o = anc[t], own[t]
            take = (o < 0) & (a >= 0)
            o[take] = o[a[take]]
            for v in S.border.tolist():
                if o[v] >= 0 and v not in done[t]:
                    done[t].add(v)
                    records.append((t, S.lo + v, int(o[v])))
        if not records:
            break
        incoming = records
    owner = np.full(V, -1, np.int32)
    owned = np.zeros((R, n), np.int32)
    for t, S in enumerate(ranks):
        part = own[t][:S.V]
        owner[S.lo:S.lo + S.V] = part
        owned[t] = np.bincount(part[part >= 0], minlength=n)
    return value, hops, parent, dict(info, owner=owner, owned=owned)
