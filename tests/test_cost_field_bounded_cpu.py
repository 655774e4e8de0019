"""CPU: bounded cost fields ("Bounded fields").

(i) Truncation is exact.  What the device does under a bound -- relax only extensions whose cost is within it --
is written out on the host (tests/bound_ref.py, restricted_field: a budget-restricted Dijkstra on the (cost, hops)
key, then the smallest-u parent rule) and compared, cost bits, hops and parents, with the definition: truncate() of
the full field of tests/cpp/field_reference.cpp.  Graphs: the random family at seeds 3, 7, 13, 21, 22, a symmetric
chain of 200, both saturating graphs, an 8 x 8 lattice with a zero band, 60-decade, subnormal and all-zero costs,
a star with two hubs; two sources each (the first and the last valid node); budgets 0, +inf, the median cost of
the reached nodes, the float just below it and the largest cost.

(ii) The entry points exist: the library exports them, the header declares them, the binding takes budget and
settle.  This part fails without the feature."""
import inspect
import os
import re

import numpy as np
import pytest

import bound_ref
import field_graphs as fg
import field_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF = 3.0

GRAPHS = {
    **{f"random_small_{s}": (lambda s=s: fg.with_positions(fg.random_small(s))) for s in (3, 7, 13, 21, 22)},
    "chain_200_symmetric": lambda: fg.chain(200, symmetric=True),
    "saturating_chain": fg.saturating_chain,
    "saturating_branch": fg.saturating_branch,
    "lattice_8x8_zero_band": lambda: fg.lattice(8, 8, zero_band=True),
    "heavy_tail_60": lambda: fg.heavy_tail(60),
    "denormal_40": lambda: fg.denormal(40),
    "all_zero_30": lambda: fg.all_zero(30),
    "star_64_2": lambda: fg.star(64, 2),
}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return field_ref.compile_reference(tmp_path_factory.mktemp("field_ref_bounded"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_restricted_dijkstra_is_the_truncated_field(ref, name):
    g = GRAPHS[name]()
    valid = np.flatnonzero(g.state != fg.INVALID)
    cases = 0
    for src in (int(valid[0]), int(valid[-1])):
        st, rc, rh, rp = field_ref.field(ref, g.rowptr, g.col, g.w, g.dist, g.state, SF, src)
        assert st == 0
        for budget in bound_ref.five_budgets(rc, rh):
            at = f"{name}, source {src}, budget {budget!r}: "
            tc, th, tp = bound_ref.truncate(rc, rh, rp, budget)
            c, h, p = bound_ref.restricted_field(g, SF, src, budget)
            assert np.array_equal(_bits(c), _bits(tc)), at + "cost bits"
            assert np.array_equal(h, th), at + "hops"
            assert np.array_equal(p, tp), at + "parents"
            # (the helper itself: a bound of +inf changes nothing, every kept node is within the bound)
            if np.isposinf(budget):
                assert np.array_equal(_bits(tc), _bits(rc)) and np.array_equal(th, rh) and np.array_equal(tp, rp), at
            assert np.all(tc[th >= 0] <= budget) and np.all(rc[(rh >= 0) & (th < 0)] > budget), at
            cases += 1
    assert cases == 10


def test_settle_bound_helper():
    cost = np.array([0.0, 2.0, 5.0, np.inf, np.inf], np.float32)
    hops = np.array([0, 1, 2, 3, -1], np.int32)  # node 3: reached at a saturated +inf; node 4: no key
    sb = bound_ref.settle_bound
    assert sb(cost, hops, [2, 1, 2], "any") == 2.0 and sb(cost, hops, [2, 1, 2], "all") == 5.0
    assert sb(cost, hops, [0], "any") == 0.0 and sb(cost, hops, [0], "all") == 0.0
    assert sb(cost, hops, [1, 4], "any") == 2.0 and np.isposinf(sb(cost, hops, [1, 4], "all"))
    assert np.isposinf(sb(cost, hops, [4], "any")) and np.isposinf(sb(cost, hops, [4], "all"))
    assert np.isposinf(sb(cost, hops, [3], "any")) and np.isposinf(sb(cost, hops, [1, 2], None))


def test_entry_points_exist():
    """Fails without the feature: the two entries, their declarations and the binding's arguments."""
    import trg_planner
    from trg_planner import _engine
    trg_planner.build_library()
    lib = trg_planner.load_library()
    header = open(os.path.join(ROOT, "include", "trg_engine.h")).read()
    for sym in ("trg_engine_cost_field_bounded", "trg_engine_field_reached"):
        assert hasattr(lib, sym), sym
        assert sym in _engine.EXPORTS, sym
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
    m = re.search(r"enum\s*\{\s*TRG_FIELD_SETTLE_NONE\s*=\s*(\d+),\s*TRG_FIELD_SETTLE_ANY\s*=\s*(\d+),\s*"
                  r"TRG_FIELD_SETTLE_ALL\s*=\s*(\d+)\s*\}", header)
    assert m, "include/trg_engine.h does not define the settle modes"
    assert [int(v) for v in m.groups()] == [_engine.SETTLE_NONE, _engine.SETTLE_ANY, _engine.SETTLE_ALL] == [0, 1, 2]
    args = inspect.signature(_engine.Engine.cost_fields).parameters
    assert "budget" in args and "settle" in args
    assert args["budget"].default is None and args["settle"].default is None
    for name in ("cheapest_frontier", "cheapest_frontiers", "plan_many", "cost_matrix"):
        p = inspect.signature(getattr(_engine.Engine, name)).parameters
        assert "early_exit" in p and p["early_exit"].default is False, name
    assert hasattr(_engine.Engine, "field_reached") and hasattr(_engine.Engine, "reachable")
