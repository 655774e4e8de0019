"""CPU: the parts of the cost field's routes that need no GPU.  The host reference of a route (tests/route_ref.py)
is checked against its own definition on the graphs the GPU tests use -- a route has hops + 1 nodes from the source
to the target, every route edge exists, is relaxable and tight, and the forward fp32 fold of the route edges' costs
reproduces the target's cost bit for bit -- and the built library, the header and the Python binding carry the
entry point."""
import os
import re

import numpy as np
import pytest

import field_graphs as fg
import field_ref
import route_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SF = 3.0


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return field_ref.compile_reference(tmp_path_factory.mktemp("field_ref_routes_cpu"))


def _bits(x):
    return np.asarray(x, F32).reshape(-1).view(np.uint32)


def _check_graph(ref, g, sources):
    """Every (source, node) pair of g as a route."""
    V = len(g.state)
    ec, ok = route_ref.edge_costs(g.col, g.w, g.dist, g.state, SF)
    row_of = np.repeat(np.arange(V), np.diff(g.rowptr))
    n_routes = 0
    for src in sources:
        st, cost, hops, parent = field_ref.field(ref, g.rowptr, g.col, g.w, g.dist, g.state, SF, src)
        assert st == 0
        routes = route_ref.routes_of_graph(g, SF, [(src, cost, hops, parent)], [(0, t) for t in range(V)])
        for t, r in enumerate(routes):
            at = f"source {src}, target {t}: "
            if hops[t] < 0:
                assert r.ids.size == 0 and r.edges.size == 0 and np.isposinf(r.cost), at
                assert r.path_length == 0 and r.avg_risk == 0, at
                continue
            n_routes += 1
            assert len(r.ids) == hops[t] + 1 and len(r.edges) == hops[t], at
            assert r.ids[0] == src and r.ids[-1] == t, at + str(r.ids)
            assert _bits(r.cost)[0] == _bits(cost[t])[0], at
            fold = F32(0.0)
            for i, k in enumerate(r.edges):
                assert row_of[k] == r.ids[i] and g.col[k] == r.ids[i + 1] and ok[k], at + f"edge {k}"
                # the least index among the row's tight edges into that node
                first = route_ref.route_edge(g.rowptr, g.col, ec, ok, cost, hops, int(r.ids[i]), int(r.ids[i + 1]))
                assert first == k, at + f"edge {k}, least tight edge {first}"
                with np.errstate(over="ignore"):
                    fold = F32(fold + ec[k])
                assert _bits(fold)[0] == _bits(cost[r.ids[i + 1]])[0], at + f"fold at node {r.ids[i + 1]}"
                assert hops[r.ids[i + 1]] == i + 1, at
            assert _bits(fold)[0] == _bits(cost[t])[0], at
            if t == src:
                assert r.path_length == 0 and r.avg_risk == 0 and len(r.ids) == 1, at
            else:  # the sums, the other way round in float64: fp32 rounding apart, the same numbers
                with np.errstate(over="ignore"):
                    want_len = g.dist[r.edges].astype(np.float64).sum()
                want_risk = g.w[r.edges].astype(np.float64).sum() / len(r.ids)
                assert np.isclose(r.path_length, want_len, rtol=1e-5) or want_len > np.finfo(F32).max, at
                assert np.isclose(r.avg_risk, want_risk, rtol=1e-5), at
    return n_routes


@pytest.mark.parametrize("seed", range(21))
def test_random_small(ref, seed):
    g = fg.with_positions(fg.random_small(seed))
    V = len(g.state)
    valid = np.flatnonzero(g.state != fg.INVALID)
    assert _check_graph(ref, g, [int(valid[0]), int(valid[-1]), V // 2]) > V // 2


@pytest.mark.parametrize("name", sorted(fg.oddities()))
def test_oddities(ref, name):
    g, sources = fg.oddities()[name]
    _check_graph(ref, g, sources)


def test_triple_duplicates_edge_rule(ref):
    """0 -> 1 has three equal edges: the first counts.  1 -> 2 has three of weights 0.9, 0.1 and 0.4: only the
    middle one is tight.  3 -> 0 has two of weight 0.2 and then one of 0.1: the last one."""
    g, _ = fg.oddities()["triple_duplicates"]
    for src, t, nth, weight in ((0, 1, 0, 0.5), (1, 2, 1, 0.1), (3, 0, 2, 0.1)):
        st, cost, hops, parent = field_ref.field(ref, g.rowptr, g.col, g.w, g.dist, g.state, SF, src)
        r = route_ref.routes_of_graph(g, SF, [(src, cost, hops, parent)], [(0, t)])[0]
        assert r.ids.tolist() == [src, t]
        assert r.edges.tolist() == [int(g.rowptr[src]) + nth]
        assert r.avg_risk == F32(F32(weight) / F32(2.0)) and r.path_length == F32(1.0)


def test_saturating_branch(ref):
    g = fg.saturating_branch()
    assert _check_graph(ref, g, [0, 2, 7]) > 10
    st, cost, hops, parent = field_ref.field(ref, g.rowptr, g.col, g.w, g.dist, g.state, SF, 0)
    r = route_ref.routes_of_graph(g, SF, [(0, cost, hops, parent)], [(0, 6), (0, 12)])
    assert np.isposinf(r[0].cost) and len(r[0].ids) == hops[6] + 1 > 1 and np.isposinf(r[0].path_length)
    assert r[1].ids.size == 0


def test_library_header_and_binding_carry_routes():
    """Fails without the feature: the entry point, its declaration and the Python methods."""
    import trg_planner
    from trg_planner import _engine
    trg_planner.build_library()
    lib = trg_planner.load_library()
    assert hasattr(lib, "trg_engine_field_routes")
    assert "trg_engine_field_routes" in _engine.EXPORTS
    header = open(os.path.join(ROOT, "include", "trg_engine.h")).read()
    assert re.search(r"\btrg_engine_field_routes\s*\(", header)
    m = re.search(r"typedef struct TrgRouteInfo \{(.*?)\} TrgRouteInfo;", header, re.S)
    assert m, "include/trg_engine.h does not define TrgRouteInfo"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip()
             for n in decl.replace("int32_t", "").replace("float", "").split(",")]
    assert names == [n for n, _ in _engine.TrgRouteInfo._fields_] == ["num_nodes", "cost", "path_length", "avg_risk"]
    assert callable(getattr(_engine.Engine, "routes", None)) and callable(getattr(_engine.Engine, "plan_many", None))
