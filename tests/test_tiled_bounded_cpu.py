"""CPU: the protocol of the bounded fields across tiles (tests/tiled_bound_ref.py: budgets, bounds lowered from above
by bound records, the bounded publish, the trim) must equal the definition -- bound_ref.truncate of the full protocol
field (tiled_ref.solve) at min(budget, bound_ref.settle_bound) -- in value bits, hops, parents, owners, owned and the
bound itself: the claim of DESIGN.md section 7, "Bounded fields across tiles", pinned before any GPU run.  Also the C and
Python surface of the feature."""
import inspect
import os
import re

import numpy as np
import pytest

import bound_ref
import tiled_bound_ref as tbr
import tiled_ref as tr
from tiled_support import cuts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF = 3.0
F32 = np.float32


def want_field(G, offsets, objective, members, starts, budget, mode, targets):
    """the definition: the full protocol field truncated at min(budget, settle_k) -> (value, hops, parent, owner,
    owned [R, n], bound, the full field's (value, hops))"""
    with np.errstate(over="ignore"):
        value, hops, parent, info = tr.solve(G, offsets, objective, members, starts, owners=True)
    bound = min(F32(budget), bound_ref.settle_bound(value, hops, targets, mode))
    v, h, p = bound_ref.truncate(value, hops, parent, bound)
    owner = np.where(h >= 0, info["owner"], -1).astype(np.int32)
    tile_of = np.searchsorted(offsets, np.arange(G["V"]), side="right") - 1
    owned = np.zeros((len(offsets) - 1, len(members)), np.int32)
    for g in np.flatnonzero(owner >= 0):
        owned[tile_of[g], owner[g]] += 1
    return v, h, p, owner, owned, F32(bound), (value, hops)


def check(G, offsets, objective, members, starts, budget, mode, targets):
    want = want_field(G, offsets, objective, members, starts, budget, mode, targets)
    with np.errstate(over="ignore"):
        value, hops, parent, info = tbr.solve(G, offsets, objective, members, starts, budget=budget, mode=mode,
                                              targets=targets, owners=True)
    at = f"offsets {offsets.tolist()} members {members} budget {budget!r} {mode} over {list(targets)}: "
    assert tr.bits(info["bound"]) == tr.bits(want[5]), at + f"bound {info['bound']!r} != {want[5]!r}"
    assert np.array_equal(value.view(np.uint32), want[0].view(np.uint32)), at + "value bits"
    assert np.array_equal(hops, want[1]), at + "hops"
    assert np.array_equal(parent, want[2]), at + "parents"
    assert np.array_equal(info["owner"], want[3]), at + "owners"
    assert np.array_equal(info["owned"], want[4]), at + "owned"
    return want, info


def target_lists(rng, G, offsets, full, src):
    """the settle target lists of one full field (value, hops) from `src`: all reached; one unreached; one Invalid; a
    duplicate; all in one range; one per range; one equal to the source"""
    value, hops = full
    V = G["V"]
    reached = np.flatnonzero(hops >= 0)
    unreached = np.flatnonzero((hops < 0) & (G["state"] != tr.INVALID))
    invalid = np.flatnonzero((G["state"] == tr.INVALID) & (hops < 0))
    pick = lambda pool, k: rng.choice(pool, size=k, replace=len(pool) < k).tolist()  # noqa: E731
    tile_of = np.searchsorted(offsets, np.arange(V), side="right") - 1
    out = [pick(reached, 3)]
    out.append(pick(reached, 2) + pick(unreached if unreached.size else invalid, 1))
    out.append(pick(reached, 2) + pick(invalid, 1))
    two = pick(reached, 2)
    out.append([two[0], two[1], two[0]])
    other = [t for t in np.unique(tile_of[reached]) if t != tile_of[src]]
    t = int(other[0]) if other else int(tile_of[src])
    out.append(pick(reached[tile_of[reached] == t], 3))
    out.append([int(rng.choice(reached[tile_of[reached] == t])) for t in np.unique(tile_of[reached])])
    out.append([int(src)] + pick(reached, 2))
    return out


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("R", [2, 3, 4])
def test_protocol_equals_the_truncated_full_field(seed, R):
    rng = np.random.default_rng(7000 * R + seed)
    V = int(rng.integers(12, 61)) if seed else 12
    # a sealed block: valid nodes that no source outside it reaches
    G = tr.symmetric_graph(rng, V, blocks=[(V - 3, V)] if seed % 2 else None)
    while True:  # a cut that leaves nodes outside the sealed block in two ranges at least
        offsets = cuts(rng, V, R, empty=seed % 2 == 1 and R > 2)
        tile_of = np.searchsorted(offsets, np.arange(V), side="right") - 1
        if len(set(tile_of[:V - 3].tolist())) >= 2:
            break
    cases = partial = far_all = fewer = 0
    for objective in (tr.cost(SF), tr.RISK):
        valid = np.flatnonzero((G["state"] != tr.INVALID) & (np.diff(G["rowptr"]) > 0) & (np.arange(V) < V - 3))
        src = int(rng.choice(valid))
        with np.errstate(over="ignore"):
            value, hops, _, full_info = tr.solve(G, offsets, objective, [src])
        lists = target_lists(rng, G, offsets, (value, hops), src)
        for budget in bound_ref.five_budgets(value, hops):
            for mode, targets in [(None, [])] + [(m, t) for m in ("any", "all") for t in lists]:
                want, info = check(G, offsets, objective, [src], None, budget, mode, targets)
                cases += 1
                left = int((want[1] >= 0).sum())
                partial += 0 < left < int((hops >= 0).sum())
                fewer += sum(info["exchanges"]) < sum(full_info["exchanges"])
                if mode == "all" and want[5] < F32(budget):  # the bound is a target's value: whose?
                    at = [t for t in targets if tr.bits(value[t]) == tr.bits(want[5])]
                    far_all += any(tile_of[t] != tile_of[src] for t in at)
    # the preconditions, which the reference alone must meet
    assert 3 * partial >= cases, (partial, cases)
    assert far_all > 0, "no ALL case took its bound from a target in a range other than the source's"
    print(f"R {R} seed {seed}: {cases} cases, {partial} truncate and leave something, {fewer} with fewer exchanges")


@pytest.mark.parametrize("seed", range(3))
def test_sets_with_start_costs_tied_with_an_arrival(seed):
    """a set of members in different ranges, one starting at exactly the cost at which another member's walk arrives"""
    rng = np.random.default_rng(90 + seed)
    V = 48
    G = tr.symmetric_graph(rng, V)
    offsets = cuts(rng, V, 3)
    valid = np.flatnonzero((G["state"] != tr.INVALID) & (np.diff(G["rowptr"]) > 0))
    a, b, c = (int(x) for x in rng.choice(valid, 3, replace=False))
    with np.errstate(over="ignore"):
        value, hops, _, _ = tr.solve(G, offsets, tr.cost(SF), [a])
    assert hops[b] > 0 and np.isfinite(value[b])
    members, starts = [a, b, c, b], np.array([0.0, value[b], 0.25, value[b] + F32(1.0)], F32)
    with np.errstate(over="ignore"):
        full = tr.solve(G, offsets, tr.cost(SF), members, starts)
    for budget in bound_ref.five_budgets(full[0], full[1]):
        for mode, targets in ((None, []), ("any", [b, c]), ("all", [a, b, c])):
            check(G, offsets, tr.cost(SF), members, starts, budget, mode, targets)


def test_a_budget_below_a_start_cost_drops_the_member():
    rng = np.random.default_rng(5)
    G = tr.symmetric_graph(rng, 30)
    offsets = np.array([0, 11, 30], np.int64)
    valid = np.flatnonzero(G["state"] != tr.INVALID)
    members, starts = [int(valid[0]), int(valid[-1])], np.array([0.0, 5.0], F32)
    want, info = check(G, offsets, tr.cost(SF), members, starts, F32(4.0), None, [])
    assert want[1][members[1]] != 0  # (not a root: above the budget, or reached cheaper from the other member)


# ---- the surface ------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "trg_engine.h")) as f:
        return f.read()


def test_header_declares_the_bounded_entries():
    flat = re.sub(r"\s*\n \*\s*", " ", _header())
    for sym in ("trg_engine_tiled_cost_field_bounded", "trg_engine_tiled_risk_field_bounded",
                "trg_engine_tiled_field_reached"):
        assert re.search(r"TrgStatus " + sym + r"\(", flat), sym
    for doc in ("README.md", "DESIGN.md", os.path.join("include", "trg_engine.h")):
        with open(os.path.join(ROOT, doc)) as f:
            text = re.sub(r"\s*\n( \*)?\s*", " ", f.read())
        assert not re.search(r"[Bb]ounds, cost models and (the )?refresh are not offered", text), doc
        assert not re.search(r"risk ceilings \(budget / settle\), cost models and refresh are not offered", text), doc
        assert "Bounded fields across tiles" in text, doc


def test_python_surface():
    """the calls that existed keep their arguments; the bounded forms are calls of their own, and without bounds they
    default to the unbounded solve"""
    from trg_planner import _engine, tiled
    E = _engine.Engine
    for name in ("tiled_cost_fields", "tiled_cost_fields_from", "tiled_risk_fields", "tiled_risk_fields_from"):
        p = inspect.signature(getattr(E, name + "_bounded")).parameters
        assert [p[k].default for k in ("budget", "settle", "settle_gids")] == [None, None, None], name
        assert "budget" not in inspect.signature(getattr(E, name)).parameters, name
    for name in ("tiled_plan_many", "tiled_safest_routes"):
        assert list(inspect.signature(getattr(E, name + "_early_exit")).parameters)[1:] == ["start_gid", "goal_gids"], name
    assert list(inspect.signature(E.tiled_assign_frontiers_within).parameters)[1:] == ["member_gids", "budget", "start_costs"]
    assert list(inspect.signature(E.tiled_frontier_ceilings_within).parameters)[1:] == ["member_gids", "budget"]
    p = inspect.signature(E.tiled_field_reached).parameters
    assert p["field"].default == 0 and p["cap"].default is None
    assert list(inspect.signature(E.tiled_reachable).parameters)[1:] == ["source_gid", "budget"]
    for sym in ("trg_engine_tiled_cost_field_bounded", "trg_engine_tiled_risk_field_bounded",
                "trg_engine_tiled_field_reached"):
        assert sym in _engine.EXPORTS, sym
    parts = [dict(gids=np.array([1, 4], np.int32), value=np.array([0.5, 1.0], F32), hops=np.array([1, 2], np.int32), count=2),
             dict(gids=np.empty(0, np.int32), value=np.empty(0, F32), hops=np.empty(0, np.int32), count=0),
             dict(gids=np.array([9], np.int32), value=np.array([2.0], F32), hops=np.array([3], np.int32), count=4)]
    joined = tiled.concat_reached(parts)
    assert joined["gids"].tolist() == [1, 4, 9] and joined["hops"].tolist() == [1, 2, 3] and joined["count"] == 6
    with pytest.raises(ValueError):
        tiled.concat_reached(parts[::-1])
