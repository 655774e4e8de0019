"""Test helper: the host Dijkstra of the risk field (tests/cpp/risk_reference.cpp), compiled with g++ into a shared
library and called through ctypes, and the risk objective's bindings of what the cost field's helpers state once: the
definition (field_ref.definition_field), the route walk (route_ref.route) and the owner rule (set_ref.owners_of).
Test code only; the product never links it."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import field_ref
import route_ref
import set_ref
from field_keys import F32, INVALID, edge_list, fold_max, relaxable, risk_values  # noqa: F401

BAD_WEIGHT = 1  # some edge weight is NaN, negative or infinite
BAD_SOURCE = 2


def compile_reference(out_dir):
    """-> ctypes library (built into out_dir)."""
    lib = field_ref.compile_cpp(out_dir, "risk_reference")
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
    """The set call's owners restated over one field's hops and parents (set_ref.owners_of) -> (owner, owned)."""
    owner = set_ref.owners_of(members, hops, parent)
    return owner, set_ref.count_owned(owner, len(members))


def py_risk_field(V, rowptr, col, w, state, sources):
    """field_ref.definition_field for the risk objective: risk = the least over all walks of the greatest edge risk
    r = w + 0 (max(a, r) is monotone in a)."""
    g = SimpleNamespace(rowptr=rowptr, col=col, state=state)
    return field_ref.definition_field(V, edge_list(g, risk_values(w)), max, sources)


def route(g, risk, hops, parent, t):
    """The route of one risk field to node t on the host (include/trg_engine.h, trg_engine_risk_field_sets):
    route_ref.route's walk under the fold max(risk, r) over the edge risks, from whichever source it ends at ->
    (ids source..target, CSR indices of the route edges, cost = risk[t], path_length, avg_risk); unreachable: empty,
    +inf, zeros."""
    r = route_ref.route(g.rowptr, g.col, g.w, g.dist, g.state, None, risk, hops, parent, None, t,
                        costs=(risk_values(g.w), relaxable(g.col, g.state)), fold=fold_max)
    return r.ids, r.edges.tolist(), r.cost, r.path_length, r.avg_risk
