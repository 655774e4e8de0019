"""Test helper: the host Dijkstra of the cost field (tests/cpp/field_reference.cpp), compiled with g++ into a
shared library and called through ctypes.  Test code only; the product never links it."""
import ctypes as C
import os
import subprocess

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "field_reference.cpp")
F32 = np.float32
INVALID = -1  # a node state: never entered
NO_EDGE = 1   # some edge cost is negative or not finite
BAD_SOURCE = 2


def compile_reference(out_dir):
    """-> ctypes library (built into out_dir)."""
    so = os.path.join(str(out_dir), "libfield_reference.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                           SRC, "-o", so])
    lib = C.CDLL(so)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    lib.field_reference.argtypes = [C.c_int, ip, ip, fp, fp, ip, C.c_float, C.c_int, fp, ip, ip]
    lib.field_reference.restype = C.c_int
    return lib


def field(lib, rowptr, col, w, dist, state, sf, src):
    """-> (status, cost, hops, parent) of the reference on a CSR."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    col = np.ascontiguousarray(col, np.int32)
    w = np.ascontiguousarray(w, np.float32)
    dist = np.ascontiguousarray(dist, np.float32)
    state = np.ascontiguousarray(state, np.int32)
    V = state.shape[0]
    cost = np.empty(V, np.float32)
    hops = np.empty(V, np.int32)
    parent = np.empty(V, np.int32)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    st = lib.field_reference(V, rowptr.ctypes.data_as(ip), col.ctypes.data_as(ip), w.ctypes.data_as(fp),
                             dist.ctypes.data_as(fp), state.ctypes.data_as(ip), np.float32(sf), int(src),
                             cost.ctypes.data_as(fp), hops.ctypes.data_as(ip), parent.ctypes.data_as(ip))
    return st, cost, hops, parent


def field_of_graph(lib, g, sf, src):
    """The reference on a trg_planner CsrGraph (Engine.graph("global"))."""
    return field(lib, g.rowptr, g.col, g.w, g.dist, g.state, sf, src)


def py_field(V, rowptr, col, w, dist, state, sf, src):
    """The definition, restated apart from any Dijkstra: cost = the least fp32 fold over all walks (a
    Bellman-Ford on the cost alone: fl(a + c) is monotone in a); hops = the BFS depth of the tight subgraph
    (edges with fl(cost[u] + c) == cost[v]); parent = the smallest tight u with hops[u] + 1 == hops[v]."""
    sf = F32(sf)
    ec = [(sf * F32(w[k]) + F32(1.0)) * F32(dist[k]) for k in range(len(col))]
    edges = [(u, int(col[k]), ec[k]) for u in range(V) for k in range(rowptr[u], rowptr[u + 1])
             if state[int(col[k])] != INVALID]
    cost = [None] * V
    cost[src] = F32(0.0)
    changed = True
    while changed:
        changed = False
        for u, v, c in edges:
            if cost[u] is not None and (cost[v] is None or F32(cost[u] + c) < cost[v]):
                cost[v] = F32(cost[u] + c)
                changed = True
    tight = [(u, v) for u, v, c in edges if cost[u] is not None and F32(cost[u] + c) == cost[v]]
    hops = [-1] * V
    hops[src] = 0
    level = [src]
    while level:
        nxt = sorted({v for u, v in tight if u in level and hops[v] < 0})
        for v in nxt:
            hops[v] = hops[level[0]] + 1
        level = nxt
    parent = [-1] * V
    for u, v in tight:
        if v != src and hops[u] + 1 == hops[v] and (parent[v] < 0 or u < parent[v]):
            parent[v] = u
    cost = np.array([np.inf if c is None else c for c in cost], np.float32)
    return cost, np.array(hops, np.int32), np.array(parent, np.int32)
