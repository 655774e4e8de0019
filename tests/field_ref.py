"""Test helper: the host Dijkstra of the cost field (tests/cpp/field_reference.cpp), compiled with g++ into a
shared library and called through ctypes, the one g++ line of every host reference (compile_cpp), and the definition
of a field restated apart from any Dijkstra (definition_field; py_field binds it to the cost objective,
risk_ref.py_risk_field to the risk objective).  Test code only; the product never links it."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np

from field_keys import F32, INVALID, cost_values, edge_list  # noqa: F401

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
NO_EDGE = 1   # some edge cost is negative or not finite
BAD_SOURCE = 2


def compile_cpp(out_dir, source_name):
    """tests/cpp/<source_name>.cpp as a shared library in out_dir -> ctypes library.  Every host reference is built
    with these flags: no contraction and no fast math, so that fp32 expressions round as written."""
    so = os.path.join(str(out_dir), f"lib{source_name}.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                           os.path.join(CPP, source_name + ".cpp"), "-o", so])
    return C.CDLL(so)


def compile_reference(out_dir):
    """-> ctypes library (built into out_dir)."""
    lib = compile_cpp(out_dir, "field_reference")
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


def definition_field(V, edges, fold, sources):
    """The definition of a field, restated apart from any Dijkstra, for either objective: value = the least fold over
    all walks from a source (a Bellman-Ford on the value alone: fold(a, c) is monotone in a); hops = the BFS depth of
    the tight subgraph (edges with fold(value[u], c) == value[v]) from the sources; parent = the smallest tight u with
    hops[u] + 1 == hops[v].  edges: field_keys.edge_list's; fold: of two float32 scalars."""
    sources = sorted({int(s) for s in np.atleast_1d(sources)})
    edges = [(int(u), int(v), F32(c)) for u, v, c in zip(*edges)]
    value = [None] * V
    for s in sources:
        value[s] = F32(0.0)
    changed = True
    while changed:
        changed = False
        for u, v, c in edges:
            if value[u] is not None and (value[v] is None or fold(value[u], c) < value[v]):
                value[v] = fold(value[u], c)
                changed = True
    tight = [(u, v) for u, v, c in edges if value[u] is not None and fold(value[u], c) == value[v]]
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
    value = np.array([np.inf if c is None else c for c in value], np.float32)
    return value, np.array(hops, np.int32), np.array(parent, np.int32)


def py_field(V, rowptr, col, w, dist, state, sf, src):
    """definition_field for the cost objective: cost = the least fp32 left fold fl(a + c) of c = (sf * w + 1) * dist."""
    g = SimpleNamespace(rowptr=rowptr, col=col, state=state)
    return definition_field(V, edge_list(g, cost_values(w, dist, sf)), lambda a, c: F32(a + c), [src])
