"""Test helper: the refresh of a retained field across tiles ("Refresh across tiles"), restated in
plain Python over tiled_ref.solve_graph, apart from the engine -- section 2's "Refresh" on the stitched graph:

carry      per rank, the old keys of its LOCAL nodes through its own map new2old (new local id -> old local id, -1: a
           new node); ghost keys are not carried; the members this rank owns get (0, 0) and their least entry as mark.
           A member's node is the first new local id of its owner tile that the map names as its old local id;
ghost fill one exchange: every ghost takes its owner's carried key, by assignment;
supporters the least GLOBAL id u with an edge u -> v whose extension of key[u] is key[v], over the NEW solve graph, ghost
           rows included;
anchor     the supporter forest jumped per rank (a member is a rooted terminal, an item without a supporter is lost, a
           ghost a terminal whose verdict only its owner knows), then exchanges of "this border item hangs on a member",
           each item once, until one carries no news; what is still unknown loses its key, ghosts too;
pass 1     warm: the protocol's loop of tiled_ref.solve from the anchored keys, `published` at the anchored border keys;
anchor again, with every item cut whose key pass 1 changed (ghosts: their mirrors changed with their owners);
pass 2     warm, over the tight edges;
parents, owner loop: as tiled_ref.solve ends.
Keys are tiled_ref's (value, hops) tuples.  Test code only."""
import numpy as np

from field_keys import F32, INVALID
from tiled_ref import NONE, _relax, solve_graph


def _owner_of(offsets, g):
    return int(np.searchsorted(np.asarray(offsets), g, side="right")) - 1


def new_members(members, off_old, off_new, maps):
    """The members' new global ids by the ranks' maps (refresh_pairs.new_sources' rule, per tile), None where gone."""
    out = []
    for g in members:
        t = _owner_of(off_old, g)
        hit = np.flatnonzero(np.asarray(maps[t]) == g - int(off_old[t]))
        out.append(int(off_new[t]) + int(hit[0]) if hit.size else None)
    return out


def _ghost_item(S, gid):
    j = int(np.searchsorted(S.ghosts, gid))
    return S.V + j if j < S.G and S.ghosts[j] == gid else -1


def _supporters(S, values, extend, key):
    """per local node: the least global id among its supporters, or -1"""
    sup = np.full(S.V, -1, np.int64)
    for u in range(S.V + S.G):
        if key[u] is NONE:
            continue
        for k in range(S.rowptr[u], S.rowptr[u + 1]):
            v = int(S.col[k])
            if S.state[v] == INVALID or key[v] is NONE:
                continue
            if extend(key[u], values[k]) == key[v]:
                g = int(S.gid_of[u])
                if sup[v] < 0 or g < sup[v]:
                    sup[v] = g
    return sup


def _forest_loop(ranks, first_anc, known):
    """The owner frame: first_anc[t][i] the first ancestor of item i (itself: a terminal; -1: none), known[t][i] >= 0
    where a terminal's verdict (an owner, or "rooted") is known.  Jumps per rank, then exchanges the border items whose
    verdict became known, each once, until an exchange without news.  -> (known, records per exchange)."""
    anc = []
    for a in first_anc:
        a = np.asarray(a, np.int64).copy()
        while True:
            b = np.where(a >= 0, a[np.maximum(a, 0)], -1)
            if np.array_equal(a, b):
                break
            a = b
        anc.append(a)
    sent = [set() for _ in ranks]
    news, incoming = [], []
    while True:
        records = []
        for t, S in enumerate(ranks):
            for src, gid, o in incoming:
                if src != t:
                    i = _ghost_item(S, gid)
                    if i >= 0:
                        known[t][i] = o
            a, o = anc[t], known[t]
            take = (o < 0) & (a >= 0)
            o[take] = o[a[take]]
            for v in S.border.tolist():
                if o[v] >= 0 and v not in sent[t]:
                    sent[t].add(v)
                    records.append((t, S.lo + v, int(o[v])))
        news.append(len(records))
        if not records:
            return known, news
        incoming = records


def _anchor(ranks, keys, mark, sup, key0=None):
    """One anchor over the supporters `sup`; with key0 every item whose key is no longer key0's is cut.  Drops the keys
    that do not hang on a member -> records per exchange."""
    first_anc, known = [], []
    for t, S in enumerate(ranks):
        a = np.full(S.V + S.G, -1, np.int64)
        o = np.full(S.V + S.G, -1, np.int64)
        for i in range(S.V + S.G):
            if keys[t][i] is NONE or (key0 is not None and keys[t][i] != key0[t][i]):
                continue
            if i >= S.V:
                a[i] = i
            elif i in mark[t]:
                a[i] = i
                o[i] = 0
            elif sup[t][i] >= 0:
                gp = int(sup[t][i])
                a[i] = gp - S.lo if S.lo <= gp < S.lo + S.V else _ghost_item(S, gp)
        first_anc.append(a)
        known.append(o)
    known, news = _forest_loop(ranks, first_anc, known)
    for t, S in enumerate(ranks):
        for i in range(S.V + S.G):
            if known[t][i] < 0:
                keys[t][i] = NONE
    return news


def _warm_pass(ranks, values, extend, keys, tight):
    """tiled_ref.solve's loop of one pass from the keys as they are -> (exchanges, records)."""
    published = [{v: keys[t][v] for v in S.border.tolist() if keys[t][v] is not NONE} for t, S in enumerate(ranks)]
    queues = [[i for i in range(S.V + S.G) if keys[t][i] is not NONE] for t, S in enumerate(ranks)]
    n_ex = n_rec = 0
    while True:
        records = []
        for t, S in enumerate(ranks):
            _relax(S, values[t], extend, keys[t], None if tight is None else tight[t], queues[t])
            for v in S.border.tolist():
                k = keys[t][v]
                if k is not NONE and (v not in published[t] or k < published[t][v]):
                    published[t][v] = k
                    records.append((t, S.lo + v, k))
        n_ex += 1
        n_rec += len(records)
        if not records:
            return n_ex, n_rec
        for t, S in enumerate(ranks):
            queues[t] = []
            for owner, gid, k in records:
                i = _ghost_item(S, gid) if owner != t else -1
                if i >= 0 and (keys[t][i] is NONE or k < keys[t][i]):
                    keys[t][i] = k
                    queues[t].append(i)


def old_keys_of(value, hops, off_old):
    """per rank the (value, hops) keys of its nodes, from a field of the OLD uncut graph"""
    out = []
    for t in range(len(off_old) - 1):
        a, b = int(off_old[t]), int(off_old[t + 1])
        out.append([NONE if hops[v] < 0 else (F32(value[v]), int(hops[v])) for v in range(a, b)])
    return out


def refresh(G, off_new, objective, old_keys, off_old, maps, members, owners=False, second_pass=True):
    """One field of the NEW global CSR dict G cut at off_new, refreshed from the ranks' `old_keys` (old_keys_of) through
    the ranks' `maps`, from the OLD global ids `members`.  second_pass=False: what pass 1 leaves.
    -> (value, hops, parent, info): carried per rank, members (the new global ids), anchor_news (records per exchange
    of both anchors, the fill's first), exchanges per pass, records per pass; with owners: owner, owned, owner_news."""
    R = len(off_new) - 1
    members_new = new_members(members, off_old, off_new, maps)
    assert None not in members_new, "a member's node is gone"
    ranks = [solve_graph(G, int(off_new[t]), int(off_new[t + 1])) for t in range(R)]
    values, extend = [objective[0](S) for S in ranks], objective[1]
    keys, mark = [], []
    for t, S in enumerate(ranks):
        n2o = np.asarray(maps[t], np.int64)
        assert n2o.shape[0] == S.V
        key = [old_keys[t][o] if 0 <= o < len(old_keys[t]) else NONE for o in n2o.tolist()] + [NONE] * S.G
        mk = {}
        for j, g in enumerate(members_new):
            if S.lo <= g < S.lo + S.V:
                key[g - S.lo] = (F32(0.0), 0)
                mk.setdefault(g - S.lo, j)
        keys.append(key)
        mark.append(mk)
    # the ghost fill: one exchange of the carried border keys
    fill = [(t, S.lo + v, keys[t][v]) for t, S in enumerate(ranks) for v in S.border.tolist() if keys[t][v] is not NONE]
    for t, S in enumerate(ranks):
        for owner, gid, k in fill:
            i = _ghost_item(S, gid) if owner != t else -1
            if i >= 0:
                keys[t][i] = k
    sup = [_supporters(S, values[t], extend, keys[t]) for t, S in enumerate(ranks)]
    anchor_news = [len(fill) + len(members_new)] + _anchor(ranks, keys, mark, sup)
    carried = [sum(1 for k in keys[t][:S.V] if k is not NONE) for t, S in enumerate(ranks)]
    key0 = [list(k) for k in keys]
    exchanges, records = [], []
    n_ex, n_rec = _warm_pass(ranks, values, extend, keys, None)
    exchanges.append(n_ex)
    records.append(n_rec)
    if second_pass:
        tight = [[NONE if k is NONE else k[0] for k in keys[t]] for t in range(R)]
        anchor_news += _anchor(ranks, keys, mark, sup, key0)
        n_ex, n_rec = _warm_pass(ranks, values, extend, keys, tight)
        exchanges.append(n_ex)
        records.append(n_rec)
    V = int(off_new[-1])
    value = np.full(V, np.inf, F32)
    hops = np.full(V, -1, np.int32)
    parent = np.full(V, -1, np.int32)
    for t, S in enumerate(ranks):
        for v in range(S.V):
            if keys[t][v] is not NONE:
                value[S.lo + v], hops[S.lo + v] = keys[t][v]
        p = _supporters(S, values[t], extend, keys[t])
        p[list(mark[t])] = -1
        parent[S.lo:S.lo + S.V] = p
    info = dict(carried=carried, members=members_new, anchor_news=anchor_news, exchanges=exchanges, records=records)
    if not (owners and second_pass):
        return value, hops, parent, info
    # the owner loop over the parents: a root knows its entry, a ghost with a key is a terminal
    first_anc, own = [], []
    for t, S in enumerate(ranks):
        a = np.full(S.V + S.G, -1, np.int64)
        o = np.full(S.V + S.G, -1, np.int64)
        for i in range(S.V + S.G):
            if keys[t][i] is NONE:
                continue
            if i >= S.V:
                a[i] = i
            elif i in mark[t]:
                a[i] = i
                o[i] = mark[t][i]
            else:
                gp = int(parent[S.lo + i])
                a[i] = gp - S.lo if S.lo <= gp < S.lo + S.V else _ghost_item(S, gp)
        first_anc.append(a)
        own.append(o)
    own, news = _forest_loop(ranks, first_anc, own)
    owner = np.full(V, -1, np.int32)
    owned = np.zeros((R, len(members_new)), np.int32)
    for t, S in enumerate(ranks):
        mine = own[t][:S.V]
        owner[S.lo:S.lo + S.V] = mine
        owned[t] = np.bincount(mine[mine >= 0], minlength=len(members_new))
    return value, hops, parent, dict(info, owner=owner, owned=owned, owner_news=news)
