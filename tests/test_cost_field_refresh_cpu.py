"""CPU: the refresh of a retained cost field as tests/refresh_ref.py states it ("Refresh") --
carry, anchor, two warm passes -- against the compiled host Dijkstra (tests/cpp/field_reference.cpp) on the graph
pairs of tests/refresh_pairs.py, the ones the GPU test runs the engine on; with identity, scrambled and empty node
maps; and that the pairs bite: the plateau pair needs the second anchor and pass 2."""
import numpy as np
import pytest

import field_ref
import refresh_pairs as rp
import refresh_ref as rr
import set_ref

SF = 3.0


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return field_ref.compile_reference(tmp_path_factory.mktemp("field_ref"))


@pytest.fixture(scope="module")
def pairs():
    return rp.all_pairs()


def host_field(ref, g, src):
    st, cost, hops, parent = field_ref.field(ref, g.rowptr, g.col, g.w, g.dist, g.state, SF, src)
    assert st == 0
    return cost, hops, parent


def assert_field(at, got, want):
    for name, a, b in zip(("cost", "hops", "parent"), got, want):
        a, b = (a.view(np.uint32), b.view(np.uint32)) if name == "cost" else (a, b)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{at}: {bad.size} {name} differ, first at node {bad[0]}: {a[bad[0]]} != {b[bad[0]]}"


@pytest.mark.parametrize("name", ["chain_cut", "chain_join", "random", "lattice", "plateau", "star", "invalid",
                                  "saturating_chain", "saturating_branch"])
def test_refresh_equals_a_fresh_field(ref, pairs, name):
    p = pairs[name]
    V = len(p.b.state)
    for s_old, s_new in zip(p.sources, rp.new_sources(p)):
        cost, hops, _ = host_field(ref, p.a, s_old)
        got = rr.refresh(p.b, SF, rr.keys_of(cost, hops), p.new2old, [s_new])
        assert_field(f"{name}, source {s_old}", got[:3], host_field(ref, p.b, s_new))
        assert 1 <= got[3] <= V


def test_chain_carries_what_the_cut_leaves(ref, pairs):
    """The cut chain keeps the 900 keys before the cut and nothing behind it; joined again, the 900 keys it had."""
    for name in ("chain_cut", "chain_join"):
        p = pairs[name]
        cost, hops, _ = host_field(ref, p.a, 0)
        got = rr.refresh(p.b, SF, rr.keys_of(cost, hops), p.new2old, [0])
        assert got[3] == 900, name
        assert (got[1][900:] >= 0).all() == (name == "chain_join")


@pytest.mark.parametrize("kind", ["identity", "scrambled", "none"])
def test_the_map_is_only_a_hint(ref, pairs, kind):
    """Whatever the map says beside where the source is, the result is the fresh field; an identity map on an
    unchanged graph carries every reached node, a map of -1 the source alone."""
    g = pairs["random"].a
    V = len(g.state)
    src = 11
    cost, hops, parent = host_field(ref, g, src)
    n2o = np.arange(V, dtype=np.int32)
    if kind == "scrambled":
        n2o = np.random.default_rng(3).permutation(V).astype(np.int32)
    if kind == "none":
        n2o[:] = -1
    if kind != "identity":
        n2o[src] = src
    got = rr.refresh(g, SF, rr.keys_of(cost, hops), n2o, [src])
    assert_field(kind, got[:3], (cost, hops, parent))
    if kind == "identity":
        assert got[3] == int((hops >= 0).sum())
    if kind == "none":
        assert got[3] == 1


def test_plateau_pair_needs_the_second_pass(ref, pairs):
    """The property the pair is built for, on the host reference: node 1 gets cheaper, node 2 keeps its cost bits and
    changes its hops.  Without the second anchor and pass 2 the refresh keeps node 2's old hops."""
    p = pairs["plateau"]
    ca, ha, _ = host_field(ref, p.a, 0)
    cb, hb, pb = host_field(ref, p.b, 0)
    assert cb[1] < ca[1]
    assert cb[2].view(np.uint32) == ca[2].view(np.uint32) and hb[2] != ha[2]
    one_pass = rr.refresh(p.b, SF, rr.keys_of(ca, ha), p.new2old, [0], second_pass=False)
    assert np.array_equal(one_pass[0].view(np.uint32), cb.view(np.uint32))  # the costs are final after pass 1
    assert not np.array_equal(one_pass[1], hb)
    assert_field("plateau", rr.refresh(p.b, SF, rr.keys_of(ca, ha), p.new2old, [0])[:3], (cb, hb, pb))


def test_sets_refresh_equals_a_fresh_set_field():
    p = rp.set_pair()
    for members, now in zip(p.sets, rp.new_sets(p)):
        old = set_ref.set_field(p.a, SF, members)
        got = rr.refresh(p.b, SF, rr.keys_of(old.cost, old.hops), p.new2old, now)
        want = set_ref.set_field(p.b, SF, now)
        assert_field(f"set {members}", got[:3], (want.cost, want.hops, want.parent))
