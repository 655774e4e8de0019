"""Test helper: cost models on the host ("Cost models").  The field of the model (safety factor
s, ceiling tau) on a graph g is DEFINED as today's field on prune(g, tau) -- g without the edges of weight > tau, in
CSR order -- at safety factor s, so every reference here is one of the existing ones (tests/set_ref.py,
tests/bound_ref.py, tests/route_ref.py) on the pruned graph; nothing of the engine is read.  min_ceiling() is the
reference of Engine.min_risk_ceiling: a breadth-first search per threshold.  Test code only."""
from collections import deque, namedtuple

import numpy as np

import route_ref
import set_ref
from field_keys import F32, INVALID, relaxable

INF = F32(np.inf)

# the pruned CSR; kept: for every edge of it the CSR index it has in the graph it was pruned from
Pruned = namedtuple("Pruned", "rowptr col w dist state kept")


def prune(g, tau):
    """g (rowptr / col / w / dist / state) without the edges with w > tau, compared in fp32; the rest in CSR order."""
    w = np.asarray(g.w, F32)
    keep = ~(w > F32(tau))
    V = len(g.state)
    eu = np.repeat(np.arange(V), np.diff(np.asarray(g.rowptr)))
    rowptr = np.zeros(V + 1, np.int64)
    np.add.at(rowptr, eu[keep] + 1, 1)
    return Pruned(np.cumsum(rowptr).astype(np.int32), np.asarray(g.col)[keep].astype(np.int32), w[keep],
                  np.asarray(g.dist, F32)[keep], np.asarray(g.state).astype(np.int32), np.flatnonzero(keep))


def as_model(model, engine_sf):
    """None, a safety factor or (safety factor, ceiling) -> (np.float32 s, np.float32 tau)."""
    if model is None:
        return F32(engine_sf), INF
    if np.ndim(model) == 0:
        return F32(model), INF
    return F32(model[0]), F32(model[1])


def model_field(g, model, members, engine_sf=3.0):
    """-> set_ref.SetField of the set `members` under `model` on g."""
    s, tau = as_model(model, engine_sf)
    return set_ref.set_field(prune(g, tau), s, members)


def model_route(g, model, f, members, t, engine_sf=3.0, costs=None):
    """The route of the field f = model_field(g, model, members) to node t -> route_ref.Route whose `edges` are CSR
    indices of g (not of the pruned graph)."""
    s, tau = as_model(model, engine_sf)
    p = prune(g, tau)
    if f.hops[t] < 0:
        src = members[0]
    else:
        src = members[f.owner[t]]
    r = route_ref.route(p.rowptr, p.col, p.w, p.dist, p.state, s, f.cost, f.hops, f.parent, src, t, costs)
    return r._replace(edges=p.kept[r.edges] if len(r.edges) else r.edges)


def distinct_weights(g):
    """The distinct weights of g's edges into valid nodes, ascending (float32)."""
    return np.unique(np.asarray(g.w, F32)[relaxable(g.col, g.state)])


def reachable_under(g, tau, start, goal):
    """Is `goal` reachable from `start` over edges of weight <= tau that enter no Invalid node (a plain BFS)."""
    if start == goal:
        return True
    seen = np.zeros(len(g.state), bool)
    seen[start] = True
    todo = deque([int(start)])
    w = np.asarray(g.w, F32)
    while todo:
        u = todo.popleft()
        for k in range(int(g.rowptr[u]), int(g.rowptr[u + 1])):
            v = int(g.col[k])
            if w[k] > F32(tau) or g.state[v] == INVALID or seen[v]:
                continue
            if v == goal:
                return True
            seen[v] = True
            todo.append(v)
    return False


def min_ceiling(g, start, goal):
    """The least of distinct_weights(g) under which `goal` is reachable from `start`, by bisection over them with one
    BFS per threshold (reachability is monotone in the threshold); None when it is unreachable under the greatest.
    A graph without such an edge has the one threshold 0."""
    ws = distinct_weights(g)
    if ws.size == 0:
        ws = np.zeros(1, F32)
    if not reachable_under(g, ws[-1], start, goal):
        return None
    lo, hi = -1, ws.size - 1  # fails, succeeds
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if reachable_under(g, ws[mid], start, goal):
            hi = mid
        else:
            lo = mid
    return F32(ws[hi])
