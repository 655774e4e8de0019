"""Test helper: the refresh of a retained cost field on the host ("Refresh"), step by step as
the engine runs it, in numpy and apart from the engine and from tests/cpp/field_reference.cpp:

carry    key0[v] = the old key of node new2old[v], none where the map says -1; the sources get (0, 0);
anchor   a node's supporter is the smallest u with an edge u -> v whose extension of key[u] is key[v]; a node
         whose chain of supporters does not end at a source loses its key; `carried` counts the nodes that keep it;
pass 1   label correcting on (cost, hops) from the anchored keys, until nothing improves: the cost words are final;
anchor again, with every node cut whose key pass 1 changed: the nodes still hanging on a source keep their hops;
pass 2   label correcting over the tight edges only: the hops are the BFS depths of the tight subgraph;
parents  the smallest supporter under the final keys.
Keys are tests/field_keys.py's words.  The steps take the relaxable edges (u, v, value) and the extension of a key as
arguments (refresh_of, carried_of); refresh and carried bind them to the cost objective, tests/risk_refresh_ref.py to
the risk objective.  Test code only."""
import numpy as np

from field_keys import F32, INVALID, NONE, cost_of, cost_values, edge_list, extend_sum, hops_of, keys_of  # noqa: F401


def supporters(V, edges, extend, key):
    """The smallest u with an edge u -> v and extend(key[u]) == key[v], or -1."""
    eu, ev, ec = edges
    live = key[eu] != NONE
    u, v = eu[live], ev[live]
    hit = extend(key[u], ec[live]) == key[v]
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
    sup = supporters(V, edges, extend, key)
    key[~_rooted(key, sup, is_source)] = NONE
    return is_source, sup, key


def carried_of(V, edges, extend, old_key, new2old, sources):
    """The number of nodes that keep a key through carry and anchor (refresh's fourth result, without the passes)."""
    return int((anchored(V, edges, extend, old_key, new2old, sources)[2] != NONE).sum())


def refresh_of(V, edges, extend, old_key, new2old, sources, second_pass=True):
    """The refreshed field of a graph of V nodes with the relaxable `edges` from the keys `old_key` of an earlier
    graph, new2old[v] the id node v had there (-1: a new node), `sources` the source nodes (one, or a set's members)
    -> (value float32, hops int32, parent int32, carried).  second_pass=False stops after pass 1 and reports its
    keys, which is what the second anchor and pass 2 are there to mend."""
    is_source, sup, key = anchored(V, edges, extend, old_key, new2old, sources)
    n_carried = int((key != NONE).sum())
    key0 = key.copy()
    key = relax(key, edges, extend)
    if second_pass:
        tight = (key >> np.uint64(32)).astype(np.uint32)
        keep = _rooted(key, sup, is_source, cut=key != key0)
        key[~keep] = NONE
        key = relax(key, edges, extend, tight)
        value = tight.view(F32).copy()
        value[tight == np.uint32(0xFFFFFFFF)] = np.inf
    else:
        value = cost_of(key)
    parent = supporters(V, edges, extend, key).astype(np.int32)
    parent[is_source] = -1
    return value, hops_of(key), parent, n_carried


# ---- the cost objective: (fl(cost + c), hops + 1) over c = (sf * w + 1) * dist ----------------------------

def _edges(g, sf):
    return edge_list(g, cost_values(g.w, g.dist, sf))


def carried(g, sf, old_key, new2old, sources):
    return carried_of(len(g.state), _edges(g, sf), extend_sum, old_key, new2old, sources)


def refresh(g, sf, old_key, new2old, sources, second_pass=True):
    """refresh_of on graph g (rowptr / col / w / dist / state) under the safety factor sf -> (cost, hops, parent,
    carried)."""
    return refresh_of(len(g.state), _edges(g, sf), extend_sum, old_key, new2old, sources, second_pass)
