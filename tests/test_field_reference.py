"""CPU: the host Dijkstra of the cost field (tests/cpp/field_reference.cpp, the GPU tests' yardstick) against a
tiny pure-Python restatement of the definition -- a Bellman-Ford on the cost, then a BFS over the tight edges,
every operation in numpy float32 -- on random small graphs with zero-cost and sub-ulp-cost edges, directed-only
and duplicate edges, Invalid nodes and disconnected parts.  cost (as bits), hops and parent must be equal."""
import numpy as np
import pytest

import field_ref
from field_graphs import random_graph as _random_graph

F32 = np.float32


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return field_ref.compile_reference(tmp_path_factory.mktemp("field_ref"))


@pytest.mark.parametrize("seed", range(12))
def test_reference_matches_python(ref, seed):
    rng = np.random.default_rng(seed)
    V = int(rng.integers(8, 48))
    rowptr, col, w, d, state = _random_graph(rng, V)
    sf = [3.0, 0.5, 1.0][seed % 3]
    for src in (0, int(rng.integers(0, V)), V - 1):
        st, cost, hops, parent = field_ref.field(ref, rowptr, col, w, d, state, sf, src)
        assert st == 0
        pc, ph, pp = field_ref.py_field(V, rowptr, col, w, d, state, sf, src)
        assert np.array_equal(cost.view(np.uint32), pc.view(np.uint32)), (seed, src)
        assert np.array_equal(hops, ph), (seed, src)
        assert np.array_equal(parent, pp), (seed, src)
        assert parent[src] == -1 and hops[src] == 0 and cost[src] == 0
        # along the parents: a walk whose fold is the cost, bit for bit, with hops + 1 nodes
        for v in np.flatnonzero(hops > 0):
            chain = [int(v)]
            while parent[chain[-1]] >= 0:
                chain.append(int(parent[chain[-1]]))
            assert chain[-1] == src and len(chain) == hops[v] + 1
        # the second component is out of reach from the first
        if src < V // 2 + 3:
            assert np.all(hops[V // 2 + 3:] == -1) and np.all(np.isinf(cost[V // 2 + 3:]))


def test_reference_sub_ulp_and_zero_cost():
    """A chain whose big first edge swallows a sub-ulp step (cost stays equal, hops grow) and a zero-cost
    shortcut: the hop word decides, the parent is the smallest id among equal extensions."""
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        lib = field_ref.compile_reference(td)
        # 0 -> 1 (cost 1e6), 1 -> 2 (1e-9: fl(1e6 + 1e-9) == 1e6), 0 -> 3 (1e6), 3 -> 2 (0), 2 -> 4 (1)
        rows = {0: [(1, 0.0, 1e6), (3, 0.0, 1e6)], 1: [(2, 0.0, 1e-9)], 2: [(4, 0.0, 1.0)], 3: [(2, 0.0, 0.0)], 4: []}
        rowptr, col, w, d = [0], [], [], []
        for u in range(5):
            for v, ww, dd in rows[u]:
                col.append(v)
                w.append(ww)
                d.append(dd)
            rowptr.append(len(col))
        st, cost, hops, parent = field_ref.field(lib, rowptr, col, w, d, np.zeros(5, np.int32), 3.0, 0)
        assert st == 0
        assert cost[2] == F32(1e6) and hops[2] == 2 and parent[2] == 1  # ties of (cost, hops): smallest id
        assert cost[4] == F32(1e6) + F32(1.0) and hops[4] == 3
        # a negative cost is rejected, so is a bad source
        st, *_ = field_ref.field(lib, rowptr, col, [-1.0] * len(w), d, np.zeros(5, np.int32), 3.0, 0)
        assert st == field_ref.NO_EDGE
        st, *_ = field_ref.field(lib, rowptr, col, w, d, np.zeros(5, np.int32), 3.0, 5)
        assert st == field_ref.BAD_SOURCE
