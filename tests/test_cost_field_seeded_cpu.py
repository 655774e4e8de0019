"""CPU: cost fields from source sets with start costs ("Start costs").

(i) tests/seed_ref.py, the definition in Python, against the compiled host Dijkstra (tests/cpp/field_reference.cpp)
on the augmented graph of every set of tests/seed_cases.py without an Invalid member (the compiled reference never
enters an Invalid node, so the identity does not cover those; the properties below do): the single-source field from
rho has the seeded field's cost bits, its hops + 1 and its parents, rho for the roots.  For every set: a root's cost is
bit for bit its least start cost and its owner the least such entry; every other reached node follows its parent;
every cost is the least over the entries of fl-fold(start cost + the entry's single reference field), which with all
start costs zero is tests/set_ref.py's field on every output.

(ii) The two entries, their declarations and the four Engine methods exist.  This part fails without the feature."""
import inspect
import os
import re

import numpy as np
import pytest

import field_graphs as fg
import field_ref
import seed_cases
import seed_ref
import set_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF = seed_cases.SF


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return field_ref.compile_reference(tmp_path_factory.mktemp("field_ref_seeded"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _properties(g, members, c0, f, at):
    c0 = seed_ref.start_costs(c0)
    roots = set(seed_ref.roots(f).tolist())
    assert roots and roots <= set(members), at + "roots"
    for v in roots:
        mine = [j for j, s in enumerate(members) if s == v]
        least = min(_bits(c0[j])[0] for j in mine)
        assert _bits(f.cost[v])[0] == least and f.parent[v] == -1, at + f"root {v}"
        assert f.owner[v] == min(j for j in mine if _bits(c0[j])[0] == least), at + f"owner of root {v}"
    walk = np.flatnonzero(f.hops > 0)
    assert np.all(f.parent[walk] >= 0) and np.array_equal(f.owner[walk], f.owner[f.parent[walk]]), at + "owners"
    assert np.array_equal(f.hops[walk], f.hops[f.parent[walk]] + 1), at + "hops along parents"
    for j, s in enumerate(members):  # a member is never dearer than any of its start costs
        assert f.hops[s] >= 0 and _bits(f.cost[s])[0] <= _bits(c0[j])[0], at + f"member {s}"
    assert np.all(f.owner[f.hops < 0] == -1) and int(f.owned.sum()) == int((f.hops >= 0).sum()), at + "owned"


@pytest.mark.parametrize("name", sorted(seed_cases.CASES))
def test_seed_ref_is_the_field_from_rho(ref, name):
    g, sets, costs = seed_cases.CASES[name]()
    V = len(g.state)
    pinned = 0
    for k, (members, c0) in enumerate(zip(sets, costs)):
        at = f"{name}, set {k} {members} at {c0.tolist()}: "
        f = seed_ref.seeded_field(g, SF, members, c0)
        _properties(g, members, c0, f, at)
        if all(g.state[s] != fg.INVALID for s in members):
            a = seed_ref.augmented(g, members, c0)
            st, zc, zh, zp = field_ref.field(ref, a.rowptr, a.col, a.w, a.dist, a.state, SF, V)
            assert st == 0
            assert np.array_equal(_bits(f.cost), _bits(zc[:V])), at + "cost bits"
            assert np.array_equal(np.where(f.hops >= 0, f.hops + 1, -1), zh[:V]), at + "hops"
            want = f.parent.copy()
            want[seed_ref.roots(f)] = V
            assert np.array_equal(want, zp[:V]), at + "parents"
            pinned += 1
    assert pinned >= len(sets) - len(sets) // 3 - (name == "duplicates"), f"{name}: {pinned} sets pinned"


@pytest.mark.parametrize("name", ["random_0", "random_1", "duplicates", "exact_tie"])
def test_zero_start_costs_are_the_set_field(name):
    g, sets, _ = seed_cases.CASES[name]()
    for members in sets:
        f = seed_ref.seeded_field(g, SF, members, np.zeros(len(members), np.float32))
        s = set_ref.set_field(g, SF, members)
        assert np.array_equal(_bits(f.cost), _bits(s.cost))
        assert all(np.array_equal(a, b) for a, b in zip(f[1:], s[1:])), f"{name}, {members}"


def test_the_cases_show_what_they_are_for():
    """On the reference: a demoted member and a root with a non-zero start in the random sets, the tie, the
    absorption, the duplicate rules and both ends of the long chain owning nodes."""
    g, sets, costs = seed_cases.CASES["random_0"]()
    demoted = rooted = 0
    for members, c0 in zip(sets, costs):
        f = seed_ref.seeded_field(g, SF, members, c0)
        demoted += sum(1 for s in set(members) if f.hops[s] > 0)
        rooted += sum(1 for j, s in enumerate(members) if f.hops[s] == 0 and c0[j] > 0 and f.owner[s] == j)
    assert demoted >= 1 and rooted >= 1
    g, (members,), (c0,) = seed_cases.exact_tie()
    f = seed_ref.seeded_field(g, SF, members, c0)
    assert f.hops[1] == 0 and f.owner[1] == 1 and f.parent[1] == -1 and f.cost[1] == 1.0
    assert f.hops[5] == 4 and f.parent[5] == 4 and f.cost[5] == 5.0 and f.owner[5] == 1
    g, (members,), (c0,) = seed_cases.absorption()
    f = seed_ref.seeded_field(g, SF, members, c0)
    assert np.all(f.cost == np.float32(2.0 ** 25)) and f.hops[9] == 0 and f.hops[8] == 1 and f.hops[31] > 0
    g, sets, costs = seed_cases.duplicates()
    members, c0 = sets[0], costs[0]
    f = seed_ref.seeded_field(g, SF, members, c0)
    assert f.owner[members[0]] == 2 and f.owner[members[4]] == 4 and f.hops[members[4]] == 0
    assert f.owned[0] == 0 and f.owned[5] == 0 and f.owned[3] == 0
    g, (members,), (c0,) = seed_cases.two_ends()
    f = seed_ref.seeded_field(g, SF, members, c0)
    assert f.owned[0] > 1000 and f.owned[1] > 1000 and int(f.hops.max()) > 1000


def test_entry_points_exist():
    """Fails without the feature: the entries, their declarations and the methods."""
    import trg_planner
    from trg_planner import _engine
    trg_planner.build_library()
    lib = trg_planner.load_library()
    header = open(os.path.join(ROOT, "include", "trg_engine.h")).read()
    for sym in ("trg_engine_cost_field_seeded", "trg_engine_pose_links"):
        assert hasattr(lib, sym) and sym in _engine.EXPORTS and re.search(r"\b" + sym + r"\s*\(", header), sym
    E = _engine.Engine
    assert list(inspect.signature(E.pose_links).parameters)[1:] == ["poses_xy", "radius", "cap"]
    assert inspect.signature(E.pose_links).parameters["cap"].default == 32
    assert list(inspect.signature(E.cost_fields_seeded).parameters)[1:4] == ["sets", "start_costs", "targets"]
    assert list(inspect.signature(E.cost_fields_from_poses).parameters)[1:] == [
        "poses_xy", "radius", "targets", "full", "budget", "settle"]
    assert list(inspect.signature(E.plan_anchored).parameters)[1:] == ["start_xy", "goal_xy", "radius"]
