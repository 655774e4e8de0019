"""CPU: cost fields from source sets ("Source sets").

(i) tests/set_ref.py, the definitions in Python, against the compiled host Dijkstra (tests/cpp/field_reference.cpp)
through the super-source identity: G plus one node z with an edge z -> s of weight 0 and dist 0 for each distinct
non-Invalid member s; the single-source field from z has the set field's cost bits, its hops + 1 and its parents,
except that the members' parent is z.  Graphs: the thirteen of test_cost_field_bounded_cpu.py; sets of 1, 2 and 5
entries and one with a duplicate.  Also: cost == min_k cost_k and cost_{owner[v]}[v] == cost[v] as bits over the
members' single reference fields; a one-member set is that source's reference field with owner 0 where reached; an
Invalid member is itself a source (against that node's single reference field: the identity does not cover it).

(ii) The entry point and the three Engine methods exist.  This part fails without the feature."""
import inspect
import os
import re

import numpy as np
import pytest

import field_graphs as fg
import field_ref
import set_ref
from test_cost_field_bounded_cpu import GRAPHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF = 3.0


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return field_ref.compile_reference(tmp_path_factory.mktemp("field_ref_sets"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sets(g):
    valid = np.flatnonzero(g.state != fg.INVALID)
    n = len(valid)
    five = [int(valid[(i * (n - 1)) // 4]) for i in range(5)]
    return {"one": [five[2]], "two": [five[0], five[4]], "five": five, "duplicate": five[:3] + [five[1], five[0]]}


def _single(ref, g, s):
    st, c, h, p = field_ref.field(ref, g.rowptr, g.col, g.w, g.dist, g.state, SF, s)
    assert st == 0
    return c, h, p


def _check_against_members(ref, g, members, f, at):
    """cost == min_k cost_k, cost_{owner[v]}[v] == cost[v] (bits), owners consistent along parents, owned sums."""
    one = {s: _single(ref, g, s) for s in dict.fromkeys(members)}
    stack = np.stack([one[s][0] for s in members])
    assert np.array_equal(_bits(f.cost), _bits(stack.min(axis=0))), at + "cost is not the minimum over the members"
    assert np.array_equal(f.hops >= 0, np.any(np.stack([one[s][1] for s in members]) >= 0, axis=0)), at + "reached"
    r = np.flatnonzero(f.hops >= 0)
    assert np.array_equal(_bits(stack[f.owner[r], r]), _bits(f.cost[r])), at + "the owner's field is dearer"
    for j, s in enumerate(members):
        assert f.owner[s] == members.index(s) and f.hops[s] == 0 and f.parent[s] == -1 and f.cost[s] == 0, at
    walk = r[f.hops[r] > 0]
    assert np.array_equal(f.owner[walk], f.owner[f.parent[walk]]), at + "owners change along a route"
    assert np.all(f.owner[f.hops < 0] == -1) and int(f.owned.sum()) == r.size, at
    assert all(f.owned[j] == 0 for j, s in enumerate(members) if members.index(s) != j), at + "a shadowed entry owns"


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_set_ref_is_the_super_source_field(ref, name):
    g = GRAPHS[name]()
    V = len(g.state)
    for kind, members in _sets(g).items():
        at = f"{name}, set {kind} {members}: "
        f = set_ref.set_field(g, SF, members)
        st, zc, zh, zp = field_ref.field(ref, *set_ref.with_super_source(g, members), SF, V)
        assert st == 0
        assert np.array_equal(_bits(f.cost), _bits(zc[:V])), at + "cost bits"
        assert np.array_equal(np.where(f.hops >= 0, f.hops + 1, -1), zh[:V]), at + "hops"
        want_parent = f.parent.copy()
        want_parent[members] = V
        assert np.array_equal(want_parent, zp[:V]), at + "parents"
        _check_against_members(ref, g, members, f, at)
        if kind == "one":
            c, h, p = _single(ref, g, members[0])
            assert np.array_equal(_bits(f.cost), _bits(c)) and np.array_equal(f.hops, h) and np.array_equal(f.parent, p)
            assert np.array_equal(f.owner, np.where(h >= 0, 0, -1)) and f.owned.tolist() == [int((h >= 0).sum())], at


@pytest.mark.parametrize("seed", [3, 7, 13, 21, 22])
def test_an_invalid_member_is_a_source(ref, seed):
    g = fg.with_positions(fg.random_small(seed))
    invalid = int(np.flatnonzero(g.state == fg.INVALID)[0])
    valid = int(np.flatnonzero(g.state != fg.INVALID)[0])
    f = set_ref.set_field(g, SF, [invalid])
    c, h, p = _single(ref, g, invalid)
    assert np.array_equal(_bits(f.cost), _bits(c)) and np.array_equal(f.hops, h) and np.array_equal(f.parent, p)
    assert np.array_equal(f.owner, np.where(h >= 0, 0, -1))
    members = [valid, invalid, valid]
    _check_against_members(ref, g, members, set_ref.set_field(g, SF, members), f"random_small_{seed}, {members}: ")


def test_truncate_helper():
    g = fg.chain(12, symmetric=True)
    f = set_ref.set_field(g, SF, [0, 11])
    bound = np.sort(f.cost)[6]
    t = set_ref.truncate(f, bound)
    out = f.cost > bound
    assert out.any() and np.all(t.owner[out] == -1) and np.all(t.hops[out] == -1) and np.all(t.parent[out] == -1)
    assert np.array_equal(t.owner[~out], f.owner[~out]) and int(t.owned.sum()) == int((~out).sum())
    same = set_ref.truncate(f, np.inf)
    assert all(np.array_equal(a, b) for a, b in zip(same, f))


def test_entry_points_exist():
    """Fails without the feature: the entry, its declaration and the three methods."""
    import trg_planner
    from trg_planner import _engine
    trg_planner.build_library()
    lib = trg_planner.load_library()
    header = open(os.path.join(ROOT, "include", "trg_engine.h")).read()
    sym = "trg_engine_cost_field_sets"
    assert hasattr(lib, sym) and sym in _engine.EXPORTS and re.search(r"\b" + sym + r"\s*\(", header)
    args = inspect.signature(_engine.Engine.cost_fields_from).parameters
    assert list(args)[1:] == ["sets", "targets", "full", "budget", "settle"]
    assert args["targets"].default is None and args["full"].default is True
    assert list(inspect.signature(_engine.Engine.nearest_source).parameters)[1:] == ["nodes_or_xy", "targets", "budget"]
    assert list(inspect.signature(_engine.Engine.assign_frontiers).parameters)[1:] == ["poses", "budget"]
