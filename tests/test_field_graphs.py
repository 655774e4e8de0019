"""CPU: the graph families of tests/field_graphs.py, which tests/test_gpu_cost_field_adversarial.py feeds to the
device.  (1) The host Dijkstra (tests/cpp/field_reference.cpp) against the pure-Python restatement of the
definition on the small members of every family, the folds that saturate to +inf included: both yardsticks say
that a node first reached at +inf is reached, with hops and a parent.  (2) The conditions that make the random
family worth running on the GPU, computed from the reference's output alone and asserted in aggregate.
(3) The JSON writer against the engine's own reader, float bits included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import field_graphs as fg
import field_ref

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return field_ref.compile_reference(tmp_path_factory.mktemp("field_ref"))


def _small_members():
    """name -> (graph, sources)"""
    out = {"chain": (fg.chain(23), [0, 11, 22]), "chain_symmetric": (fg.chain(23, symmetric=True), [0, 11, 22]),
           "star": (fg.star(40), [0, 8, 40]), "star_hubs": (fg.star(40, hubs=4), [44, 0, 9]),
           "lattice": (fg.lattice(5, 6), [0, 14, 29]), "lattice_band": (fg.lattice(6, 5, zero_band=True), [0, 5, 29]),
           "all_zero": (fg.all_zero(20), [0, 19]), "denormal": (fg.denormal(20), [0, 19]),
           "heavy_tail": (fg.heavy_tail(24), [0, 7, 23]),
           "saturating_chain": (fg.saturating_chain(), list(range(6))),
           "saturating_branch": (fg.saturating_branch(), list(range(13)))}
    out.update(fg.oddities())
    return out


SMALL = _small_members()


@pytest.mark.parametrize("name", sorted(SMALL))
def test_reference_matches_python_on_families(ref, name):
    g, sources = SMALL[name]
    V = len(g.state)
    assert g.pos.shape == (V, 3) and len({tuple(p) for p in g.pos.tolist()}) == V  # distinct lattice points
    for src in sources:
        st, cost, hops, parent = field_ref.field(ref, *g[:5], 3.0, src)
        assert st == 0
        with np.errstate(over="ignore"):
            pc, ph, pp = field_ref.py_field(V, *g[:5], 3.0, src)
        assert np.array_equal(cost.view(np.uint32), pc.view(np.uint32)), (name, src)
        assert np.array_equal(hops, ph), (name, src)
        assert np.array_equal(parent, pp), (name, src)


def test_saturated_nodes_are_reached(ref):
    """The semantics of a cost of +inf, agreed by both yardsticks (the parametrised test above) and spelled out:
    reached, with hops and a parent -- distinct from unreachable (hops -1, parent -1)."""
    st, cost, hops, parent = field_ref.field(ref, *fg.saturating_chain()[:5], 3.0, 0)
    assert st == 0
    assert cost.tolist() == [0.0, float(F32(2e38)), np.inf, np.inf, np.inf, np.inf]
    assert hops.tolist() == [0, 1, 2, 3, 4, 5] and parent.tolist() == [-1, 0, 1, 2, 3, 4]
    st, cost, hops, parent = field_ref.field(ref, *fg.saturating_branch()[:5], 3.0, 0)
    assert st == 0
    assert np.isfinite(cost[[0, 1, 7, 8, 9]]).all() and np.isinf(cost[[2, 3, 4, 5, 6, 10, 11, 12]]).all()
    assert hops.tolist() == [0, 1, 2, 3, 4, 4, 5, 1, 2, 3, 3, -1, -1]
    assert parent.tolist() == [-1, 0, 1, 2, 3, 10, 5, 0, 7, 8, 2, -1, -1]


def test_star_row_straddles_the_first_threshold():
    """At a bucket width of 4 and of 0.5 mean costs the hub's row has targets on both sides of the first
    threshold: one row pushes to the near queue and to the far pile."""
    for g in (fg.star(40), fg.star(30000), fg.star(4096, hubs=4)):
        hub_row = fg.edge_costs(g, 3.0)[g.rowptr[0]:g.rowptr[1]]
        for scale in (4.0, 0.5):
            thr = fg.bucket_width(g, 3.0, scale)
            assert (hub_row < thr).sum() >= 4 and (hub_row >= thr).sum() >= 4, (len(g.state), scale)


def _witness_shares(ref, graphs):
    tie = absorbed = 0
    for csr in graphs:
        st, cost, hops, _ = field_ref.field(ref, *csr, 3.0, 0)
        assert st == 0
        t, a = fg.witnesses(fg.with_positions(csr), 3.0, 0, cost, hops)
        tie += t
        absorbed += a
    return tie / len(graphs), absorbed / len(graphs)


@pytest.mark.parametrize("size", [30, 2000, 20000])
def test_random_family_discriminates(ref, size):
    """The GPU test is blind to a missing pass 2 unless the graphs have nodes whose hops a single label-correcting
    pass can get wrong.  From the reference's output alone: the share of graphs with a hop-tie witness (a tight
    edge u -> v, v not the source, with hops[u] + 1 > hops[v]) must be at least a half, the share with an
    absorption witness (a tight edge of cost > 0 with cost[u] == cost[v]) at least a quarter -- floors, not
    targets; at every size class the GPU test uses."""
    if size == 30:
        graphs = [fg.random_small(seed) for seed in range(60)]
    else:
        graphs = [fg.random_graph(np.random.default_rng(seed), V, scale) for seed, V, scale in fg.RANDOM_LARGE[size]]
    tie, absorbed = _witness_shares(ref, graphs)
    print(f"random family, V ~ {size}: hop-tie witness in {tie:.3f}, absorption witness in {absorbed:.3f} of "
          f"{len(graphs)} graphs")
    assert tie >= 0.5 and absorbed >= 0.25, (size, tie, absorbed)


@pytest.fixture(scope="module")
def json_reader(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("graph_json") / "libgraph_json_read.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(HERE, "cpp", "graph_json_read.cpp"), "-o", so])
    lib = C.CDLL(so)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    lib.graph_json_read.argtypes = [C.c_char_p, C.c_int, C.c_int, ip, ip, ip, fp, ip, ip, ip, fp, fp]
    lib.graph_json_read.restype = C.c_int
    return lib


def _read_json(lib, path, V, E):
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    nV, nE = C.c_int32(-1), C.c_int32(-1)
    ids, state = np.empty(V + 1, np.int32), np.empty(V + 1, np.int32)
    pos = np.empty(3 * (V + 1), np.float32)
    s, t = np.empty(E + 1, np.int32), np.empty(E + 1, np.int32)
    w, d = np.empty(E + 1, np.float32), np.empty(E + 1, np.float32)
    st = lib.graph_json_read(str(path).encode(), V + 1, E + 1, C.byref(nV), C.byref(nE), ids.ctypes.data_as(ip),
                             pos.ctypes.data_as(fp), state.ctypes.data_as(ip), s.ctypes.data_as(ip),
                             t.ctypes.data_as(ip), w.ctypes.data_as(fp), d.ctypes.data_as(fp))
    assert st == 0 and nV.value == V and nE.value == E, (st, nV.value, nE.value)
    return ids[:V], pos[:3 * V].reshape(V, 3), state[:V], s[:E], t[:E], w[:E], d[:E]


def test_json_round_trip_is_bit_exact(json_reader, tmp_path):
    """repr of a float32 widened to double, read by strtod and narrowed (graph_json.h): the same bits, for
    subnormals, -0.0, 2e38, the extremes of fp32 and every family's values."""
    special = np.array([0.0, -0.0, 1e-45, 1e-41, 1.1754942e-38, 1.1754944e-38, 2e38, 3e38, 3.4028235e38, 1e-9, 0.1,
                        1.0 / 3.0, 16777216.0, 16777217.0, 1e30, 1e-30], np.float32)
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 0x7F800000, size=4000, dtype=np.uint32).view(np.float32)  # every finite exponent
    vals = np.concatenate([special, bits])
    m = vals.shape[0]
    g = fg.from_edges(m + 1, np.arange(m), np.arange(m) + 1, vals[::-1], vals)
    graphs = {"bits": g}
    graphs.update({k: v[0] for k, v in SMALL.items()})
    for name, g in graphs.items():
        V, E = len(g.state), len(g.col)
        p = tmp_path / f"{name}.json"
        fg.write_json(p, g)
        ids, pos, state, s, t, w, d = _read_json(json_reader, p, V, E)
        assert np.array_equal(ids, np.arange(V)) and np.array_equal(state, g.state), name
        assert np.array_equal(pos.view(np.uint32), g.pos.view(np.uint32)), name
        assert np.array_equal(s, np.repeat(np.arange(V), np.diff(g.rowptr))) and np.array_equal(t, g.col), name
        assert np.array_equal(w.view(np.uint32), g.w.view(np.uint32)), name
        assert np.array_equal(d.view(np.uint32), g.dist.view(np.uint32)), name
