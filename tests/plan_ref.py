"""Test helper: planSafePath's A* on a CSR (tests/cpp/plan_reference.cpp), compiled with g++ into a shared library
and called through ctypes, and the fp32 cost of a route restated in numpy.  Test code only; the product never
links it."""
import ctypes as C
from collections import namedtuple

import numpy as np

import field_ref

F32 = np.float32
OK = 0
NOT_FOUND = 6  # TRG_ERR_NOT_FOUND

# ids: the route's node ids (empty when status != OK); the three floats are numpy float32 scalars
Plan = namedtuple("Plan", "status ids direct_dist path_length avg_risk num_points")


def compile_reference(out_dir):
    """-> ctypes library (built into out_dir)."""
    lib = field_ref.compile_cpp(out_dir, "plan_reference")
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    lib.plan_reference.argtypes = [C.c_int, ip, ip, fp, fp, ip, fp, C.c_float, C.c_int, C.c_int, C.c_int, ip,
                                   C.c_int32, fp, ip]
    lib.plan_reference.restype = C.c_int
    return lib


class Csr:
    """The arrays of one graph, made contiguous once: many searches run on each."""

    def __init__(self, rowptr, col, w, dist, state, pos):
        self.rowptr = np.ascontiguousarray(rowptr, np.int32)
        self.col = np.ascontiguousarray(col, np.int32)
        self.w = np.ascontiguousarray(w, np.float32)
        self.dist = np.ascontiguousarray(dist, np.float32)
        self.state = np.ascontiguousarray(state, np.int32)
        self.pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        self.V = self.state.shape[0]
        assert self.rowptr.shape[0] == self.V + 1 and self.pos.shape[0] == self.V
        self._path = np.empty(self.V + 1, np.int32)

    @classmethod
    def of_graph(cls, g):
        """Of a trg_planner CsrGraph (Engine.graph("global")) or an oracle_api Graph."""
        return cls(g.rowptr, g.col, g.w, g.dist, g.state, g.xyz)

    @classmethod
    def of_field_graph(cls, g):
        """Of a field_graphs.FieldGraph."""
        return cls(g.rowptr, g.col, g.w, g.dist, g.state, g.pos)


def plan(lib, csr, sf, start, goal, widen=0):
    """-> Plan of the reference's A* from node `start` to node `goal`."""
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    info = np.zeros(3, np.float32)
    n = C.c_int32(0)
    st = lib.plan_reference(csr.V, csr.rowptr.ctypes.data_as(ip), csr.col.ctypes.data_as(ip),
                            csr.w.ctypes.data_as(fp), csr.dist.ctypes.data_as(fp), csr.state.ctypes.data_as(ip),
                            csr.pos.ctypes.data_as(fp), np.float32(sf), int(start), int(goal), int(widen),
                            csr._path.ctypes.data_as(ip), csr._path.shape[0], info.ctypes.data_as(fp), C.byref(n))
    assert st in (OK, NOT_FOUND), st
    assert n.value <= csr._path.shape[0]  # a route visits a node once
    return Plan(st, csr._path[:n.value].copy(), info[0], info[1], info[2], int(n.value))


def id_of_xyz(xyz):
    """{float words of a position: node id}; positions must be distinct."""
    m = {tuple(p): i for i, p in enumerate(np.ascontiguousarray(xyz, np.float32).view(np.uint32).tolist())}
    assert len(m) == len(xyz)
    return m


def ids_of_path(lookup, path):
    """The node ids of returned path points, through their float words."""
    return np.array([lookup[tuple(p)] for p in np.ascontiguousarray(path, np.float32).view(np.uint32).tolist()],
                    np.int32)


def route_cost(csr, sf, ids):
    """The definition, apart from any search: the fp32 fold of (sf * w + 1) * dist along the route, taking the
    cheapest a -> b edge at each step (every operation rounded to fp32)."""
    sf = F32(sf)
    c = F32(0.0)
    for a, b in zip(ids[:-1], ids[1:]):
        ks = np.arange(csr.rowptr[a], csr.rowptr[a + 1])
        ks = ks[csr.col[ks] == b]
        assert ks.size, (a, b)
        c = F32(c + min(F32(F32(F32(sf * csr.w[k]) + F32(1.0)) * csr.dist[k]) for k in ks))
    return c
