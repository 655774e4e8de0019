"""Test helper: the refresh of a retained RISK field on the host ("Risk fields"), the steps of
tests/refresh_ref.py restated for the extension (max(risk, r), hops + 1) over the edge risks r = w + 0: carry, anchor,
pass 1, anchor again with every changed key cut, pass 2 over the tight edges, parents.  What looks at key words only
(the key packing, the jump over the supporter forest) is refresh_ref's own; the steps that extend a key take the
extension and the edge values as arguments.  In numpy, apart from the engine and from tests/cpp/risk_reference.cpp.
Test code only."""
import numpy as np

from refresh_ref import F32, INVALID, NONE, _rooted, cost_of, hops_of, keys_of  # noqa: F401

risk_of = cost_of  # (the upper word of a key, +inf without one)


def edge_risks(g):
    """(u, v, risk in fp32) of the relaxable edges: into a node of the graph that is not Invalid; r = w + 0."""
    col = np.asarray(g.col)
    V = len(g.state)
    er = (np.asarray(g.w, F32) + F32(0.0)).astype(F32)
    eu = np.repeat(np.arange(V), np.diff(np.asarray(g.rowptr)))
    ok = (col >= 0) & (col < V)
    ok[ok] = np.asarray(g.state)[col[ok]] != INVALID
    return eu[ok], col[ok].astype(np.int64), er[ok]


def extend_max(key, r):
    """(max(risk, r), hops + 1) of every key (none of them NONE); risks are >= +0 and no NaN."""
    a = (key >> np.uint64(32)).astype(np.uint32).view(F32)
    g = np.where(r > a, r, a).astype(F32)
    return (g.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ((key + np.uint64(1)) & np.uint64(0xFFFFFFFF))


def supporters(V, edges, key, extend):
    """The smallest u with an edge u -> v and extend(key[u]) == key[v], or -1."""
    eu, ev, ec = edges
    live = key[eu] != NONE
    u, v = eu[live], ev[live]
    hit = extend(key[u], ec[live]) == key[v]
    sup = np.full(V, V, np.int64)
    np.minimum.at(sup, v[hit], u[hit])
    sup[sup == V] = -1
    return sup


def relax(key, edges, extend, tight=None):
    """Label correcting to the fixed point, over all edges or over the tight ones (tight: the final upper words)."""
    eu, ev, ec = edges
    key = key.copy()
    while True:
        live = key[eu] != NONE
        u, v = eu[live], ev[live]
        ext = extend(key[u], ec[live])
        if tight is not None:
            on = (ext >> np.uint64(32)).astype(np.uint32) == tight[v]
            v, ext = v[on], ext[on]
        new = key.copy()
        np.minimum.at(new, v, ext)
        if np.array_equal(new, key):
            return key
        key = new


def anchored(V, edges, extend, old_key, new2old, sources):
    """Carry and anchor -> (is_source, supporters, anchored keys)."""
    n2o = np.asarray(new2old, np.int64)
    key = np.where(n2o >= 0, np.asarray(old_key, np.uint64)[np.maximum(n2o, 0)], NONE)
    is_source = np.zeros(V, bool)
    is_source[np.asarray(sources, np.int64)] = True
    key[is_source] = np.uint64(0)
    sup = supporters(V, edges, key, extend)
    key[~_rooted(key, sup, is_source)] = NONE
    return is_source, sup, key


def carried(g, old_key, new2old, sources):
    """The number of nodes that keep a key through carry and anchor."""
    return int((anchored(len(g.state), edge_risks(g), extend_max, old_key, new2old, sources)[2] != NONE).sum())


def refresh(g, old_key, new2old, sources, second_pass=True, edges=None, extend=extend_max):
    """The refreshed risk field of graph g from the keys `old_key` of an earlier graph, new2old[v] the id node v had
    there (-1: a new node), `sources` the source nodes of g (one, or a set's members) -> (risk float32, hops int32,
    parent int32, carried).  second_pass=False stops after pass 1 and reports its keys, which is what the second anchor
    and pass 2 are there to mend."""
    V = len(g.state)
    edges = edge_risks(g) if edges is None else edges
    is_source, sup, key = anchored(V, edges, extend, old_key, new2old, sources)
    n_carried = int((key != NONE).sum())
    key0 = key.copy()
    key = relax(key, edges, extend)
    if second_pass:
        tight = (key >> np.uint64(32)).astype(np.uint32)
        keep = _rooted(key, sup, is_source, cut=key != key0)
        key[~keep] = NONE
        key = relax(key, edges, extend, tight)
        risk = tight.view(F32).copy()
        risk[tight == np.uint32(0xFFFFFFFF)] = np.inf
    else:
        risk = risk_of(key)
    parent = supporters(V, edges, key, extend).astype(np.int32)
    parent[is_source] = -1
    return risk, hops_of(key), parent, n_carried
