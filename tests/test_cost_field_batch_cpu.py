"""CPU: the parts of the batched cost field that need no GPU -- the choice of the cheapest Frontier node from
gathered arrays (trg_planner._engine.choose_frontier, what Engine.cheapest_frontiers applies per pose) and the
batch limit, which the header and the Python binding each state."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


def _choose(ids, cost, hops):
    from trg_planner._engine import choose_frontier
    return choose_frontier(np.array(ids, np.int32), np.array(cost, np.float32), np.array(hops, np.int32))


def test_choose_least_cost():
    assert _choose([4, 9, 2], [3.0, 1.5, 2.0], [1, 7, 1]) == (9, 1)


def test_choose_cost_tie_broken_by_hops():
    assert _choose([4, 9, 2], [1.5, 1.5, 2.0], [5, 3, 1]) == (9, 1)
    assert _choose([4, 9, 2], [1.5, 1.5, 1.5], [5, 3, 2]) == (2, 2)


def test_choose_cost_and_hops_tie_broken_by_id():
    assert _choose([9, 4, 7], [1.5, 1.5, 1.5], [3, 3, 3]) == (4, 1)
    # the candidates need not be sorted, and the index is into the list as given
    assert _choose([30, 20, 10], [0.0, 0.0, 0.0], [2, 2, 2]) == (10, 2)


def test_choose_skips_non_finite_costs():
    # +inf with hops >= 0 is a saturated fold: reached, but never chosen; hops == -1 is unreached; NaN never wins
    assert _choose([1, 2, 3, 4], [INF, INF, 8.0, np.nan], [2, -1, 9, 1]) == (3, 2)
    assert _choose([1, 2], [INF, INF], [2, -1]) is None
    assert _choose([1], [np.nan], [0]) is None


def test_choose_without_candidates():
    assert _choose([], [], []) is None


def test_choose_zero_cost_source_is_a_candidate():
    # a pose that stands on a Frontier node: cost 0, hops 0
    assert _choose([5, 6], [0.25, 0.0], [1, 0]) == (6, 1)


def test_batch_limit_matches_header():
    from trg_planner import _engine
    header = open(os.path.join(ROOT, "include", "trg_engine.h")).read()
    m = re.search(r"^#define\s+TRG_FIELD_BATCH_MAX\s+(\d+)\s*$", header, re.M)
    assert m, "include/trg_engine.h does not define TRG_FIELD_BATCH_MAX"
    assert int(m.group(1)) == _engine.TRG_FIELD_BATCH_MAX == 64
    assert "trg_engine_cost_field_batch" in _engine.EXPORTS
