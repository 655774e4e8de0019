"""Test helper: the host Dijkstra of the risk field (tests/cpp/risk_reference.cpp), compiled with g++ into a shared
library and called through ctypes, and the definition restated apart from any Dijkstra.  Test code only; the product
never links it."""
import ctypes as C
import os
import subprocess

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "risk_reference.cpp")
F32 = np.float32
INVALID = -1  # a node state: never entered
BAD_WEIGHT = 1  # some edge weight is NaN, negative or infinite
BAD_SOURCE = 2


def compile_reference(out_dir):
    """-> ctypes library (built into out_dir)."""
    so = os.path.join(str(out_dir), "librisk_reference.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                           SRC, "-o", so])
    lib = C.CDLL(so)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    lib.risk_reference.argtypes = [C.c_int, ip, ip, fp, ip, ip, C.c_int, fp, ip, ip]
    lib.risk_reference.restype = C.c_int
    return lib


def risk_field(lib, rowptr, col, w, state, sources):
    """-> (status, risk, hops, parent) of the reference on a CSR, from a node or a set of nodes."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    col = np.ascontiguousarray(col, np.int32)
    w = np.ascontiguousarray(w, np.float32)
    state = np.ascontiguousarray(state, np.int32)
    src = np.ascontiguousarray(np.atleast_1d(sources), np.int32)
    V = state.shape[0]
    risk = np.empty(V, np.float32)
    hops = np.empty(V, np.int32)
    parent = np.empty(V, np.int32)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    st = lib.risk_reference(V, rowptr.ctypes.data_as(ip), col.ctypes.data_as(ip), w.ctypes.data_as(fp),
                            state.ctypes.data_as(ip), src.ctypes.data_as(ip), src.shape[0],
                            risk.ctypes.data_as(fp), hops.ctypes.data_as(ip), parent.ctypes.data_as(ip))
    return st, risk, hops, parent


def risk_of_graph(lib, g, sources):
    """The reference on anything with rowptr, col, w, state (a FieldGraph, an Engine.graph("global"))."""
    return risk_field(lib, g.rowptr, g.col, g.w, g.state, sources)


def reference_risks(lib, g, sources):
    """Full fields, one solve per distinct single source: the (m, V) arrays risk, hops, parent."""
    one = {}
    for s in dict.fromkeys(int(s) for s in sources):
        st, *rest = risk_of_graph(lib, g, s)
        assert st == 0
        one[s] = rest
    return tuple(np.stack([one[int(s)][i] for s in sources]) for i in range(3))


def owners(members, hops, parent):
    """The set call's owners restated over one field's hops and parents: a member's owner is the least entry of
    `members` that names it, any other reached node's is its parent's, an unreached node's -1 -> (owner, owned)."""
    V = len(hops)
    owner = np.full(V, -1, np.int32)
    for j in reversed(range(len(members))):
        owner[members[j]] = j
    for v in np.argsort(hops, kind="stable"):
        if hops[v] > 0:
            owner[v] = owner[parent[v]]
    owned = np.bincount(owner[owner >= 0], minlength=len(members)).astype(np.int32)
    return owner, owned


def py_risk_field(V, rowptr, col, w, state, sources):
    """The definition, restated apart from any Dijkstra: risk = the least over all walks of the greatest edge risk
    (a Bellman-Ford on max alone: max(a, r) is monotone in a); hops = the BFS depth of the tight subgraph (edges with
    max(risk[u], r) == risk[v]) from the sources; parent = the smallest tight u with hops[u] + 1 == hops[v]."""
    sources = sorted({int(s) for s in np.atleast_1d(sources)})
    er = [F32(w[k]) + F32(0.0) for k in range(len(col))]
    edges = [(u, int(col[k]), er[k]) for u in range(V) for k in range(rowptr[u], rowptr[u + 1])
             if 0 <= int(col[k]) < V and state[int(col[k])] != INVALID]
    risk = [None] * V
    for s in sources:
        risk[s] = F32(0.0)
    changed = True
    while changed:
        changed = False
        for u, v, r in edges:
            if risk[u] is not None and (risk[v] is None or max(risk[u], r) < risk[v]):
                risk[v] = max(risk[u], r)
                changed = True
    tight = [(u, v) for u, v, r in edges if risk[u] is not None and max(risk[u], r) == risk[v]]
    hops = [-1] * V
    for s in sources:
        hops[s] = 0
    level = sources
    while level:
        nxt = sorted({v for u, v in tight if u in level and hops[v] < 0})
        for v in nxt:
            hops[v] = hops[level[0]] + 1
        level = nxt
    parent = [-1] * V
    for u, v in tight:
        if hops[v] > 0 and hops[u] + 1 == hops[v] and (parent[v] < 0 or u < parent[v]):
            parent[v] = u
    risk = np.array([np.inf if r is None else r for r in risk], np.float32)
    return risk, np.array(hops, np.int32), np.array(parent, np.int32)


def route(g, risk, hops, parent, t):
    """The route of one risk field to node t on the host (include/trg_engine.h, trg_engine_risk_field_sets): the
    parent walk, the route edge into p_i the relaxable edge of least CSR index in row p_{i-1} with col p_i that is
    tight; path_length and the weight sum fp32 left folds from the target end backwards, avg_risk = sum / nodes ->
    (ids source..target, CSR indices of the route edges, cost = risk[t], path_length, avg_risk); unreachable: empty,
    +inf, zeros."""
    V = len(g.state)
    h = int(hops[t])
    if h < 0:
        return np.empty(0, np.int32), [], F32(np.inf), F32(0.0), F32(0.0)
    ids, edges = [int(t)], []
    pl, ws = F32(0.0), F32(0.0)
    for _ in range(h):
        v = ids[-1]
        u = int(parent[v])
        assert u >= 0 and hops[u] + 1 == hops[v], f"node {v} has no parent one hop nearer"
        hit = [k for k in range(int(g.rowptr[u]), int(g.rowptr[u + 1]))
               if int(g.col[k]) == v and g.state[v] != INVALID and
               np.maximum(risk[u], F32(g.w[k]) + F32(0.0)).view(np.uint32) == risk[v].view(np.uint32)]
        assert hit, f"no tight edge {u} -> {v}"
        pl = F32(pl + F32(g.dist[hit[0]]))
        ws = F32(ws + F32(g.w[hit[0]]))
        edges.append(hit[0])
        ids.append(u)
    assert hops[ids[-1]] == 0 and 0 <= ids[-1] < V
    return np.array(ids[::-1], np.int32), edges[::-1], F32(risk[t]), pl, F32(ws / F32(len(ids)))
