"""Test helper: the routes of a cost field on the host, from the host Dijkstra's (cost, hops, parent)
(tests/field_ref.py) -- the definition of DESIGN.md section 2, "Routes", written out without regard to speed:
the route to t is source = p_0, ..., p_h = t with p_{i-1} = parent[p_i] and h = hops[t]; the route edge into p_i is
the edge of least CSR index in row p_{i-1} whose col is p_i, which is relaxable (not into an Invalid node) and
whose extension of p_{i-1}'s key (fl(cost + c), hops + 1) is p_i's key; path_length and the risk sum are fp32 left
folds of those edges' dist and weight from the target end backwards; avg_risk = risk sum / number of nodes in
fp32.  The walk takes the objective's fold: risk_ref.route is the same walk under (max(risk, r), hops + 1).  Test
code only."""
from collections import namedtuple

import numpy as np

from field_keys import F32, INVALID, cost_values, fold_sum, relaxable  # noqa: F401

# ids: int32 node ids source..target (empty: unreachable); edges: CSR indices, edges[i] leads into ids[i + 1];
# cost, path_length, avg_risk: np.float32
Route = namedtuple("Route", "ids edges cost path_length avg_risk")


def edge_costs(col, w, dist, state, sf):
    """(cost per edge in fp32, relaxable per edge): field_keys' cost values and its rule of what is relaxed."""
    return cost_values(w, dist, sf), relaxable(col, state)


def route_edge(rowptr, col, ec, ok, cost, hops, u, v, fold=fold_sum):
    """The route edge from u into v, or -1; fold: the objective's (field_keys.fold_sum for a cost field, fold_max
    for a risk field, `ec` then being the edge risks)."""
    if int(hops[u]) + 1 != int(hops[v]):
        return -1
    k0, k1 = int(rowptr[u]), int(rowptr[u + 1])
    g = fold(cost[u:u + 1].astype(F32), ec[k0:k1])
    hit = (col[k0:k1] == v) & ok[k0:k1] & (g.view(np.uint32) == cost[v:v + 1].astype(F32).view(np.uint32))
    j = np.flatnonzero(hit)
    return k0 + int(j[0]) if j.size else -1


def route(rowptr, col, w, dist, state, sf, cost, hops, parent, src, t, costs=None, memo=None, fold=fold_sum):
    """-> Route of the field (cost, hops, parent) from src (None: from whichever source the walk ends at, as in a
    field from a set) to node t.  costs: edge_costs(...) computed once; memo: a dict per field that keeps the route
    edge found into a node; fold: route_edge's."""
    ec, ok = costs if costs is not None else edge_costs(col, w, dist, state, sf)
    col, cost = np.asarray(col), np.asarray(cost, F32)
    memo = {} if memo is None else memo
    h = int(hops[t])
    if h < 0:
        return Route(np.empty(0, np.int32), np.empty(0, np.int64), F32(np.inf), F32(0.0), F32(0.0))
    ids = [int(t)]
    edges = []
    pl, risk = F32(0.0), F32(0.0)
    for _ in range(h):
        v = ids[-1]
        u = int(parent[v])
        assert u >= 0, f"node {v} with {int(hops[v])} hops has no parent"
        k = memo.get(v)
        if k is None:
            k = memo[v] = route_edge(rowptr, col, ec, ok, cost, hops, u, v, fold)
        assert k >= 0, f"no tight edge {u} -> {v}"
        with np.errstate(over="ignore"):
            pl = F32(pl + F32(dist[k]))
            risk = F32(risk + F32(w[k]))
        edges.append(k)
        ids.append(u)
    assert src is None or ids[-1] == int(src), f"the walk from {t} ended at {ids[-1]}, not at the source {src}"
    ids.reverse()
    edges.reverse()
    return Route(np.array(ids, np.int32), np.array(edges, np.int64), F32(cost[t]), pl, F32(risk / F32(len(ids))))


def routes_of_graph(g, sf, fields, pairs):
    """g: anything with rowptr / col / w / dist / state; fields: list of (src, cost, hops, parent) per field;
    pairs: (field, target) per route -> list of Route."""
    costs = edge_costs(g.col, g.w, g.dist, g.state, sf)
    out, memos = [], {}
    for f, t in pairs:
        src, cost, hops, parent = fields[int(f)]
        out.append(route(g.rowptr, g.col, g.w, g.dist, g.state, sf, cost, hops, parent, src, int(t), costs,
                         memos.setdefault(int(f), {})))
    return out
