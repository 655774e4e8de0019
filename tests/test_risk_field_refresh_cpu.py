"""CPU: the refresh of a retained risk field as tests/risk_refresh_ref.py states it ("Risk
fields") -- carry, anchor, two warm passes under the extension (max(risk, r), hops + 1) -- against the compiled host
Dijkstra of the risk field (tests/cpp/risk_reference.cpp) on the graph pairs of tests/risk_refresh_pairs.py, the ones
the GPU test runs the engine on, and against the definition restated (risk_ref.py_risk_field) on the small ones; that
the pairs bite -- one warm pass leaves wrong hops, the levels pair carries and changes many keys, the peak pairs change
every risk word behind the peak -- and that the entry point and the Python calls are there."""
import inspect
import os
import re

import numpy as np
import pytest

import refresh_pairs as rp
import risk_ref
import risk_refresh_pairs as rrp
import risk_refresh_ref as rrr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the star's 30 001 nodes are the GPU test's; the numpy restatement skips them)
NAMES = ("chain_cut", "chain_join", "random", "lattice", "invalid", "risk_plateau", "levels", "peak_down", "peak_up",
         "duplicates_swapped")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return risk_ref.compile_reference(tmp_path_factory.mktemp("risk_ref"))


@pytest.fixture(scope="module")
def pairs():
    return rrp.all_pairs(star=False)


def host_field(ref, g, sources):
    st, risk, hops, parent = risk_ref.risk_of_graph(ref, g, sources)
    assert st == 0
    return risk, hops, parent


def assert_field(at, got, want):
    for name, a, b in zip(("risk", "hops", "parent"), got, want):
        a, b = (a.view(np.uint32), b.view(np.uint32)) if name == "risk" else (a, b)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{at}: {bad.size} {name} differ, first at node {bad[0]}: {a[bad[0]]} != {b[bad[0]]}"


def test_the_pairs_are_all_there(pairs):
    assert sorted(pairs) == sorted(NAMES)
    assert sorted(rrp.all_pairs()) == sorted(NAMES + ("star",))


@pytest.mark.parametrize("name", NAMES)
def test_refresh_equals_a_fresh_field(ref, pairs, name):
    p = pairs[name]
    V = len(p.b.state)
    for s_old, s_new in zip(p.sources, rp.new_sources(p)):
        risk, hops, _ = host_field(ref, p.a, s_old)
        got = rrr.refresh(p.b, rrr.keys_of(risk, hops), p.new2old, [s_new])
        want = host_field(ref, p.b, s_new)
        assert_field(f"{name}, source {s_old}", got[:3], want)
        assert 1 <= got[3] <= V
        assert got[3] == rrr.carried(p.b, rrr.keys_of(risk, hops), p.new2old, [s_new])
        if V <= 200:
            g = p.b
            assert_field(f"{name}, source {s_old}, the definition", got[:3],
                         risk_ref.py_risk_field(V, g.rowptr, g.col, g.w, g.state, [s_new]))


def test_chain_carries_what_the_cut_leaves(ref, pairs):
    """All-zero weights: only hops change.  The cut chain keeps the 900 keys before the cut and nothing behind it;
    joined again, the 900 keys it had."""
    for name in ("chain_cut", "chain_join"):
        p = pairs[name]
        assert not p.a.w.any() and not p.b.w.any()
        risk, hops, _ = host_field(ref, p.a, 0)
        got = rrr.refresh(p.b, rrr.keys_of(risk, hops), p.new2old, [0])
        assert got[3] == 900, name
        assert (got[1][900:] >= 0).all() == (name == "chain_join")


@pytest.mark.parametrize("name", ["risk_plateau", "levels", "random"])
def test_one_warm_pass_is_not_enough(ref, pairs, name):
    """Without the second anchor and pass 2 the risk words are final and some hops are those of a stale, riskier
    prefix."""
    p = pairs[name]
    s_old, s_new = p.sources[0], rp.new_sources(p)[0]
    ra, ha, _ = host_field(ref, p.a, s_old)
    rb, hb, pb = host_field(ref, p.b, s_new)
    one_pass = rrr.refresh(p.b, rrr.keys_of(ra, ha), p.new2old, [s_new], second_pass=False)
    assert np.array_equal(one_pass[0].view(np.uint32), rb.view(np.uint32))  # the risks are final after pass 1
    assert not np.array_equal(one_pass[1], hb)
    assert_field(name, rrr.refresh(p.b, rrr.keys_of(ra, ha), p.new2old, [s_new])[:3], (rb, hb, pb))


def test_risk_plateau_is_what_it_says(ref, pairs):
    p = pairs["risk_plateau"]
    ra, ha, _ = host_field(ref, p.a, 0)
    rb, hb, _ = host_field(ref, p.b, 0)
    assert (ra[1], ha[1]) == (np.float32(0.3), 1) and (rb[1], hb[1]) == (np.float32(0.1), 3)
    assert ra[2] == rb[2] == np.float32(0.5) and (ha[2], hb[2]) == (2, 4) and (ha[3], hb[3]) == (3, 5)
    one_pass = rrr.refresh(p.b, rrr.keys_of(ra, ha), p.new2old, [0], second_pass=False)
    assert (one_pass[0][2], one_pass[1][2]) == (np.float32(0.5), 2)


def test_levels_carries_and_changes_many_keys(ref, pairs):
    p = pairs["levels"]
    now = rp.new_sources(p)
    n2o = p.new2old.astype(np.int64)
    seen = []
    for k in range(2):
        ra, ha, _ = host_field(ref, p.a, p.sources[k])
        rb, hb, _ = host_field(ref, p.b, now[k])
        ka, kb = rrr.keys_of(ra, ha), rrr.keys_of(rb, hb)
        carried = rrr.carried(p.b, ka, p.new2old, [now[k]])
        old = np.where(n2o >= 0, ka[np.maximum(n2o, 0)], rrr.NONE)
        changed = int(((kb != old) & (kb != rrr.NONE)).sum())
        seen.append((carried, changed, int(np.unique(rb[hb >= 0]).size)))
    print(f"levels: V {len(p.b.state)}, (carried, changed, distinct risks) per field {seen}")
    assert all(c >= 200 and ch >= 500 for c, ch, _ in seen), seen
    # the third source reaches only itself, before and after
    assert (host_field(ref, p.b, now[2])[1] >= 0).sum() == 1 and (host_field(ref, p.a, p.sources[2])[1] >= 0).sum() == 1


@pytest.mark.parametrize("name", ["peak_down", "peak_up"])
def test_peak_pairs_change_every_risk_behind_the_peak(ref, pairs, name):
    p = pairs[name]
    behind = np.arange(rrp.PEAK_EDGE + 1, rrp.PEAK_V)
    for s in p.sources:
        assert s <= rrp.PEAK_EDGE
        ra, ha, _ = host_field(ref, p.a, s)
        rb, hb, _ = host_field(ref, p.b, s)
        assert (ra[behind] != rb[behind]).all() and np.array_equal(ha, hb)
        assert np.array_equal(ra[:rrp.PEAK_EDGE + 1].view(np.uint32), rb[:rrp.PEAK_EDGE + 1].view(np.uint32))
        assert (rb[behind] > ra[behind]).all() == (name == "peak_up")


def test_duplicates_swapped_keeps_every_key_and_moves_the_route_edge(ref, pairs):
    p = pairs["duplicates_swapped"]
    fa, fb = host_field(ref, p.a, 0), host_field(ref, p.b, 0)
    assert_field("duplicates_swapped", fa, fb)
    assert risk_ref.route(p.a, *fa, 1)[1] == [1] and risk_ref.route(p.b, *fb, 1)[1] == [0]


def test_sets_refresh_equals_a_fresh_set_field(ref):
    p = rrp.risk_sets_pair()
    assert len(p.sets[0]) != len(set(p.sets[0]))  # a member named twice
    for members, now in zip(p.sets, rp.new_sets(p)):
        risk, hops, _ = host_field(ref, p.a, members)
        got = rrr.refresh(p.b, rrr.keys_of(risk, hops), p.new2old, now)
        assert_field(f"set {members}", got[:3], host_field(ref, p.b, now))


def test_bad_b_is_refused_by_the_reference(ref):
    p = rrp.bad_b_pair()
    assert int(np.isnan(p.b.w).sum()) == 1 and not np.isnan(p.a.w).any()
    assert risk_ref.risk_of_graph(ref, p.a, 0)[0] == 0
    assert risk_ref.risk_of_graph(ref, p.b, 0)[0] == risk_ref.BAD_WEIGHT


@pytest.mark.parametrize("kind", ["identity", "scrambled", "none"])
def test_the_map_is_only_a_hint(ref, pairs, kind):
    g = pairs["levels"].a
    V = len(g.state)
    src = 11
    risk, hops, parent = host_field(ref, g, src)
    n2o = np.arange(V, dtype=np.int32)
    if kind == "scrambled":
        n2o = np.random.default_rng(3).permutation(V).astype(np.int32)
    if kind == "none":
        n2o[:] = -1
    if kind != "identity":
        n2o[src] = src
    got = rrr.refresh(g, rrr.keys_of(risk, hops), n2o, [src])
    assert_field(kind, got[:3], (risk, hops, parent))
    if kind == "identity":
        assert got[3] == int((hops >= 0).sum())
    if kind == "none":
        assert got[3] == 1


def test_entry_point_exported_declared_and_listed():
    import trg_planner
    from trg_planner import _engine
    sym = "trg_engine_risk_field_refresh"
    lib = trg_planner.load_library()
    with open(os.path.join(ROOT, "include", "trg_engine.h")) as f:
        header = f.read()
    assert hasattr(lib, sym) and sym in _engine.EXPORTS and re.search(r"\b" + sym + r"\s*\(", header)
    assert lib.trg_engine_risk_field_refresh.argtypes == lib.trg_engine_cost_field_refresh.argtypes


def test_python_surface():
    from trg_planner import _engine
    sig = inspect.signature(_engine.Engine.refresh_risk_fields)
    assert list(sig.parameters)[1:] == ["new2old", "targets", "full"]
    assert sig.parameters["new2old"].default is None and sig.parameters["full"].default is True
    for name in ("frontier_ceilings", "safest_frontier"):
        par = inspect.signature(getattr(_engine.Engine, name)).parameters
        assert "reuse" in par and par["reuse"].default is False, name
