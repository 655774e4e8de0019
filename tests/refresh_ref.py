"""Test helper: the refresh of a retained cost field on the host ("Refresh"), step by step as
the engine runs it, in numpy and apart from the engine and from tests/cpp/field_reference.cpp:

carry    key0[v] = the old key of node new2old[v], none where the map says -1; the sources get (0, 0);
anchor   a node's supporter is the smallest u with an edge u -> v whose extension of key[u] is key[v]; a node
         whose chain of supporters does not end at a source loses its key; `carried` counts the nodes that keep it;
pass 1   label correcting on (cost, hops) from the anchored keys, until nothing improves: the cost words are final;
anchor again, with every node cut whose key pass 1 changed: the nodes still hanging on a source keep their hops;
pass 2   label correcting over the tight edges only: the hops are the BFS depths of the tight subgraph;
parents  the smallest supporter under the final keys.
Keys are uint64 words, cost bits << 32 | hops, NONE without one.  Test code only."""
import numpy as np

F32 = np.float32
INVALID = -1
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys_of(cost, hops):
    """The key words of a field given as cost (float32, +inf where unreached) and hops (-1 where unreached)."""
    bits = np.ascontiguousarray(cost, F32).view(np.uint32).astype(np.uint64)
    k = (bits << np.uint64(32)) | np.asarray(hops).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return np.where(np.asarray(hops) < 0, NONE, k)


def cost_of(key):
    c = (key >> np.uint64(32)).astype(np.uint32).view(F32).copy()
    c[key == NONE] = np.inf
    return c


def hops_of(key):
    return np.where(key == NONE, -1, (key & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)


def _edges(g, sf):
    """(u, v, cost in fp32) of the relaxable edges: into a node of the graph that is not Invalid."""
    col = np.asarray(g.col)
    V = len(g.state)
    with np.errstate(over="ignore", invalid="ignore"):
        ec = ((F32(sf) * np.asarray(g.w, F32) + F32(1.0)) * np.asarray(g.dist, F32)).astype(F32)
    eu = np.repeat(np.arange(V), np.diff(np.asarray(g.rowptr)))
    ok = (col >= 0) & (col < V)
    ok[ok] = np.asarray(g.state)[col[ok]] != INVALID
    return eu[ok], col[ok].astype(np.int64), ec[ok]


def _extend(key, c):
    """(fl(cost + c), hops + 1) of every key (none of them NONE)."""
    with np.errstate(over="ignore"):
        g = ((key >> np.uint64(32)).astype(np.uint32).view(F32) + c).astype(F32)
    return (g.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ((key + np.uint64(1)) & np.uint64(0xFFFFFFFF))


def _supporters(V, eu, ev, ec, key):
    """The smallest u with an edge u -> v and extend(key[u]) == key[v], or -1."""
    live = key[eu] != NONE
    u, v = eu[live], ev[live]
    hit = _extend(key[u], ec[live]) == key[v]
    sup = np.full(V, V, np.int64)
    np.minimum.at(sup, v[hit], u[hit])
    sup[sup == V] = -1
    return sup


def _rooted(key, sup, is_source, cut=None):
    """Which nodes hang on a source through their supporters (a cut node hangs on nothing), by pointer jumping."""
    V = key.shape[0]
    anc = np.where(is_source, np.arange(V), sup)
    anc[key == NONE] = -1
    if cut is not None:
        anc[cut] = -1
    while True:
        nxt = np.where(anc >= 0, anc[np.maximum(anc, 0)], -1)
        if np.array_equal(nxt, anc):
            return anc >= 0
        anc = nxt


def _relax(key, eu, ev, ec, tight=None):
    """Label correcting to the fixed point, over all edges or over the tight ones (tight: the final cost bits)."""
    key = key.copy()
    while True:
        live = key[eu] != NONE
        u, v = eu[live], ev[live]
        ext = _extend(key[u], ec[live])
        if tight is not None:
            on = (ext >> np.uint64(32)).astype(np.uint32) == tight[v]
            v, ext = v[on], ext[on]
        new = key.copy()
        np.minimum.at(new, v, ext)
        if np.array_equal(new, key):
            return key
        key = new


def _anchored(g, sf, old_key, new2old, sources):
    """Carry and anchor -> (edges, is_source, supporters, anchored keys)."""
    V = len(g.state)
    eu, ev, ec = _edges(g, sf)
    n2o = np.asarray(new2old, np.int64)
    key = np.where(n2o >= 0, np.asarray(old_key, np.uint64)[np.maximum(n2o, 0)], NONE)
    is_source = np.zeros(V, bool)
    is_source[np.asarray(sources, np.int64)] = True
    key[is_source] = np.uint64(0)
    sup = _supporters(V, eu, ev, ec, key)
    key[~_rooted(key, sup, is_source)] = NONE
    return (eu, ev, ec), is_source, sup, key


def carried(g, sf, old_key, new2old, sources):
    """The number of nodes that keep a key through carry and anchor (refresh's fourth result, without the passes)."""
    return int((_anchored(g, sf, old_key, new2old, sources)[3] != NONE).sum())


def refresh(g, sf, old_key, new2old, sources, second_pass=True):
    """The refreshed field of graph g (rowptr / col / w / dist / state) from the keys `old_key` of an earlier graph,
    new2old[v] the id node v had there (-1: a new node), `sources` the source nodes of g (one, or a set's members)
    -> (cost float32, hops int32, parent int32, carried).  second_pass=False stops after pass 1 and reports its
    keys, which is what the second anchor and pass 2 are there to mend."""
    V = len(g.state)
    (eu, ev, ec), is_source, sup, key = _anchored(g, sf, old_key, new2old, sources)
    n_carried = int((key != NONE).sum())
    key0 = key.copy()
    key = _relax(key, eu, ev, ec)
    if second_pass:
        tight = (key >> np.uint64(32)).astype(np.uint32)
        keep = _rooted(key, sup, is_source, cut=key != key0)
        key[~keep] = NONE
        key = _relax(key, eu, ev, ec, tight)
        cost = tight.view(F32).copy()
        cost[tight == np.uint32(0xFFFFFFFF)] = np.inf
    else:
        cost = cost_of(key)
    parent = _supporters(V, eu, ev, ec, key).astype(np.int32)
    parent[is_source] = -1
    return cost, hops_of(key), parent, n_carried
