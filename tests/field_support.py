"""Test helper: what the GPU tests of the cost field share -- engine parameters and bucket widths, the `ref` and
`engine` fixtures (import them by name), loading a tests/field_graphs.py graph through load_json, the host
Dijkstra's fields for a list of sources, and exact comparisons.  Test code only."""
import functools
import json

import numpy as np
import pytest

import field_graphs as fg
import field_ref

F32 = np.float32
# mountain.yaml without its safety factor (the adversarial tests run three), and with it
PARAMS = dict(expand_dist=0.6, robot_size=0.3, sample_num=7, height_threshold=0.16, collision_threshold=0.1,
              update_collision_threshold=0.5, goal_tolerance=0.8)
MOUNTAIN = dict(PARAMS, safety_factor=3.0)
# field_delta_scale: near-far with a split far pile, one bucket per distinct cost through the threshold bump, and
# single-bucket Bellman-Ford
SCALES = ("4", "0.5", "1e-6", "1e3", "inf")
SCALES_LARGE = ("4", "1e-6", "inf")  # near-far, a bucket per distinct cost, Bellman-Ford
INVALID_ARG = 1  # TRG_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """The compiled host Dijkstra (tests/cpp/field_reference.cpp), once per importing module."""
    return field_ref.compile_reference(tmp_path_factory.mktemp("field_ref"))


@pytest.fixture(scope="module")
def engine(request):
    """One engine without a map for the JSON graphs of the importing module: every load_json and every batch size
    reuses the field buffers of the one before.  A module that sets FIELD_DELTA_SCALE gets that bucket width."""
    import trg_planner
    e = trg_planner.Engine(**MOUNTAIN)
    scale = getattr(request.module, "FIELD_DELTA_SCALE", None)
    if scale is not None:
        e.set_option("field_delta_scale", scale)
    yield e
    e.close()


def bits(a):
    """The float32 words of `a`, in its shape (a scalar gives one word)."""
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_rows(at, what, got, want, as_bits=False):
    a, b = (bits(got), bits(want)) if as_bits else (got, want)
    bad = np.argwhere(a != b)
    assert bad.shape[0] == 0, at + (f"{bad.shape[0]} {what} differ, first at field {bad[0][0]}, node {bad[0][1]}: "
                                    f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


@functools.lru_cache(maxsize=None)
def random_large(seed, V, scale):
    return fg.with_positions(fg.random_graph(np.random.default_rng(seed), V, scale))


def load_graph(e, g, tmp_path, name="g"):
    """g through load_json -> the exported CSR, checked against g: V, E, rows in order with float bits, states."""
    p = tmp_path / f"{name}.json"
    fg.write_json(p, g)
    e.load_json(str(p))
    x = e.graph("global")
    assert x.V == len(g.state) and x.E == len(g.col), (x.V, x.E)
    assert np.array_equal(x.rowptr, g.rowptr)
    assert np.array_equal(x.col, g.col)
    assert np.array_equal(x.w.view(np.uint32), g.w.view(np.uint32))
    assert np.array_equal(x.dist.view(np.uint32), g.dist.view(np.uint32))
    assert np.array_equal(x.state, g.state)
    assert np.array_equal(x.xyz.view(np.uint32), g.pos.view(np.uint32))
    return x


def write_graph(path, nodes, edges):
    """A hand-written graph in the engine's format: nodes as (pos, state), edges as (source, target, weight, dist)."""
    doc = {"nodes": [{"id": i, "pos": list(p), "state": s} for i, (p, s) in enumerate(nodes)],
           "edges": [{"source": a, "target": b, "weight": w, "dist": d} for a, b, w, d in edges]}
    with open(path, "w") as f:
        json.dump(doc, f)


def reference_fields(ref, x, sf, sources, stacked=True):
    """The host Dijkstra's full fields, one solve per distinct source: the (m, V) arrays cost, hops, parent, or,
    with stacked=False, a list of (source, cost, hops, parent) per field (what tests/route_ref.py takes)."""
    one = {}
    for s in dict.fromkeys(int(s) for s in sources):
        st, rc, rh, rp = field_ref.field_of_graph(ref, x, sf, s)
        assert st == 0
        one[s] = rc, rh, rp
    if not stacked:
        return [(int(s), *one[int(s)]) for s in sources]
    return tuple(np.stack([one[int(s)][i] for s in sources]) for i in range(3))


def with_isolated_node(g):
    """g plus one node without edges (the last id)."""
    pos = np.concatenate([g.pos, g.pos.max(axis=0, keepdims=True) + F32([3.0, 3.0, 0.0])])
    return fg.FieldGraph(np.append(g.rowptr, g.rowptr[-1]).astype(np.int32), g.col, g.w, g.dist,
                         np.append(g.state, 0).astype(np.int32), pos.astype(np.float32))


def small_sources(g, m, seed):
    """m sources of a random_small graph with an isolated last node: a node of each component, a duplicate, an
    Invalid node and the isolated one first (rotated by the seed, so that the short batches meet every kind),
    then nodes all over the graph."""
    V = len(g.state)
    invalid = int(np.flatnonzero(g.state == fg.INVALID)[0])
    half = (V - 1) // 2 + 3  # ids from here on only link among themselves
    first = int(np.flatnonzero(g.state[:half] != fg.INVALID)[0])
    second = half + int(np.flatnonzero(g.state[half:V - 1] != fg.INVALID)[0])
    kinds = [first, second, first, invalid, V - 1]
    kinds = kinds[seed % 5:] + kinds[:seed % 5]
    return (kinds + [(7 * i + seed) % V for i in range(m)])[:m]
