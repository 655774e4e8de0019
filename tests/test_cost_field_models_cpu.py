"""CPU: the host references of the cost models (tests/model_ref.py; DESIGN.md section 2, "Cost models") checked
against themselves before the GPU test leans on them: pruning at +inf changes nothing, a lower ceiling never makes a
node cheaper, and the bisecting reference of min_risk_ceiling agrees with a scan over every distinct weight that
decides reachability from the pruned graph's own field."""
import numpy as np
import pytest

import field_graphs as fg
import model_ref
import set_ref

F32 = np.float32
INF = F32(np.inf)
SEEDS = (3, 7, 13, 21, 22)  # the random_small graphs of tests/test_cost_field_bounded_cpu.py


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("seed", SEEDS)
def test_prune_at_inf_is_the_identity(seed):
    g = fg.with_positions(fg.random_small(seed))
    p = model_ref.prune(g, INF)
    assert np.array_equal(p.rowptr, g.rowptr) and np.array_equal(p.col, g.col) and np.array_equal(p.state, g.state)
    assert np.array_equal(_bits(p.w), _bits(g.w)) and np.array_equal(_bits(p.dist), _bits(g.dist))
    assert np.array_equal(p.kept, np.arange(len(g.col)))


@pytest.mark.parametrize("seed", SEEDS)
def test_prune_keeps_order_and_rows(seed):
    g = fg.with_positions(fg.random_small(seed))
    V = len(g.state)
    row = np.repeat(np.arange(V), np.diff(g.rowptr))
    for tau in (0.0, 0.1, 0.5, 1.0):
        p = model_ref.prune(g, tau)
        assert np.all(np.diff(p.kept) > 0) and np.all(g.w[p.kept] <= F32(tau))
        gone = np.setdiff1d(np.arange(len(g.col)), p.kept)
        assert np.all(g.w[gone] > F32(tau))
        assert np.array_equal(np.repeat(np.arange(V), np.diff(p.rowptr)), row[p.kept])
        assert np.array_equal(p.col, g.col[p.kept]) and np.array_equal(_bits(p.dist), _bits(g.dist[p.kept]))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("sf", [0.0, 3.0])
def test_a_lower_ceiling_is_never_cheaper(seed, sf):
    """Costs are >= +0, so their bits order as they do; an unreached node is +inf."""
    g = fg.with_positions(fg.random_small(seed))
    valid = np.flatnonzero(g.state != fg.INVALID)
    taus = [F32(0.0), F32(0.1), F32(0.3), F32(0.5), F32(0.8), F32(1.0), INF]
    for src in (int(valid[0]), int(valid[-1])):
        fields = [model_ref.model_field(g, (sf, t), [src]) for t in taus]
        differ = 0
        for lo, hi in zip(fields, fields[1:]):
            assert np.all(_bits(lo.cost) >= _bits(hi.cost)), (seed, sf, src)
            assert np.all((lo.hops >= 0) <= (hi.hops >= 0))
            differ += int(np.any(_bits(lo.cost) != _bits(hi.cost)))
        plain = set_ref.set_field(g, sf, [src])
        assert np.array_equal(_bits(fields[-1].cost), _bits(plain.cost)) and np.array_equal(fields[-1].hops, plain.hops)
        assert np.array_equal(fields[-1].parent, plain.parent)
        if src == int(valid[0]):
            assert differ >= 1, (seed, sf)  # the ceilings do cut something on these graphs


@pytest.mark.parametrize("seed", SEEDS)
def test_min_ceiling_against_a_scan_over_every_weight(seed):
    g = fg.with_positions(fg.random_small(seed))
    V = len(g.state)
    ws = model_ref.distinct_weights(g)
    assert ws.size > 3 and ws[0] == 0
    valid = np.flatnonzero(g.state != fg.INVALID)
    some, none = 0, 0
    for start in (int(valid[0]), int(valid[len(valid) // 2]), int(valid[-1])):
        hops = [model_ref.model_field(g, (3.0, t), [start]).hops for t in ws]
        for goal in range(V):
            want = next((F32(t) for t, h in zip(ws, hops) if h[goal] >= 0), None)
            got = model_ref.min_ceiling(g, start, goal)
            assert (got is None) == (want is None) and (got is None or got == want), (seed, start, goal, got, want)
            some += want is not None and want > 0
            none += want is None
        assert model_ref.min_ceiling(g, start, start) == ws[0]
    assert some > 0 and none > 0, (some, none)


def test_min_ceiling_on_a_hand_graph():
    # 0 -> 1 -> 3 over weights 0.9 and 0.1, 0 -> 2 -> 3 over 0.4 and 0.5, 3 -> 4 over 0.2, node 5 apart
    e = [(0, 1, 0.9, 1.0), (1, 3, 0.1, 1.0), (0, 2, 0.4, 1.0), (2, 3, 0.5, 1.0), (3, 4, 0.2, 1.0)]
    g = fg.from_edges(6, *zip(*e))
    assert model_ref.min_ceiling(g, 0, 3) == F32(0.5) and model_ref.min_ceiling(g, 0, 4) == F32(0.5)
    assert model_ref.min_ceiling(g, 0, 1) == F32(0.9) and model_ref.min_ceiling(g, 1, 4) == F32(0.2)
    assert model_ref.min_ceiling(g, 0, 5) is None and model_ref.min_ceiling(g, 5, 5) == F32(0.1)
    empty = fg.from_edges(2, [], [], [], [])
    assert model_ref.min_ceiling(empty, 0, 0) == 0 and model_ref.min_ceiling(empty, 0, 1) is None
