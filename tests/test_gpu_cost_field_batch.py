"""GPU: cost fields from many sources in one solve (trg_engine_cost_field_batch, Engine.cost_fields, cost_matrix,
cheapest_frontiers).  m fields are one field of the disjoint union of m copies of the graph: one threshold, one
"work left" word and one round counter for all, work items (field, node).  Every row of a batch is compared,
exactly -- cost as bits, hops and parents equal, no tolerance -- with the host Dijkstra of
tests/cpp/field_reference.cpp for that row's source and with Engine.cost_field for the same source.

The graphs are those of tests/field_graphs.py, through load_json, at the smallest shapes where the item indexing
can go wrong: V ~ 30 with m up to the limit of 64 (duplicate, Invalid, isolated sources, both components), one
node with three fields, a 3 000-node chain whose four fields converge thousands of rounds apart, a 30 000-long
row in one field while the others idle, four hubs in one wave, a 200 x 200 lattice of exact ties with eight
fields, saturating folds, zero and subnormal bucket widths, and a 1 950-node random graph with 16 fields
(V is no multiple of 4, m * V none of 64).  Then the gathered targets, buffer reuse over one engine, a
device-built graph before and after an updateGraph, and the error cases.

Rounds of one batch.  Above, every batch stays under the host's cap of 2 * (4 * m * V + 64) rounds, and
reached_out[k] is the count of hops[k] >= 0; both are asserted for every batch.  Below, "a batch takes at least the
rounds of the slowest single solve of its sources" is asserted where a round count is a function of the graph: on
the directed chain, where every node has one walk and is pushed once, with its final key.  Elsewhere a round count
is not reproducible, with or without batches, so two counts cannot be ordered: a queued node is expanded with the
key it has when its lanes read it, which another lane of the same launch may just have lowered, so a key can travel
two hops in one round or not, by timing; and the union's bucket boundaries (least live far cost over ALL fields)
are not a field's own, which changes how often nodes are expanded again, either way.  Measured on an MI355X, all
results equal to the reference each time: random_small seed 13, m = 5, width 0.5: 19 rounds for the batch against
20 for the slowest single solve in one run, 18 against 20 in another; the same graph with ONE bucket (width inf,
where the fields do not interact): 20 against 20 in one run, 19 against 20 in the next.  The counts of every
batch are printed."""
import numpy as np
import pytest

import field_graphs as fg
from field_support import (INVALID_ARG, MOUNTAIN, PARAMS, SCALES, assert_rows, bits, engine, load_graph,  # noqa: F401
                           random_large, ref, reference_fields, small_sources, with_isolated_node, write_graph)
from graph_support import obs_crop

pytestmark = pytest.mark.gpu
F32 = np.float32
def _check_batch(ref, e, x, sources, scales=SCALES, targets=None, sf=3.0, one_walk_per_node=False):
    """One batch per bucket width against the reference and against the single solves of its sources."""
    V, m = x.V, len(sources)
    sources = [int(s) for s in sources]
    rc, rh, rp = reference_fields(ref, x, sf, sources)
    r = None
    for scale in scales:
        e.set_option("field_delta_scale", scale)
        at = f"field_delta_scale {scale}, m {m}: "
        r = e.cost_fields(source_ids=sources, targets=targets)
        assert r["cost"].shape == r["hops"].shape == r["parent"].shape == (m, V), at
        assert_rows(at, "costs", r["cost"], rc, as_bits=True)
        assert_rows(at, "hops", r["hops"], rh)
        assert_rows(at, "parents", r["parent"], rp)
        info = r["info"]
        assert r["sources"].tolist() == sources and info.source == sources[0], at
        assert np.array_equal(r["reached"], (r["hops"] >= 0).sum(axis=1)), at + str(r["reached"])
        assert info.reached == int(r["reached"].sum()), at
        assert info.rounds <= 2 * (4 * m * V + 64), at + f"{info.rounds} rounds"  # the host's cap, over two passes
        single_rounds = 0
        for k, s in enumerate(sources):
            if s in sources[:k]:
                continue
            cost, hops, parent, one = e.cost_field(source_id=s)
            sat = at + f"single field of source {s}: "
            assert np.array_equal(bits(cost), bits(r["cost"][k])), sat + "costs differ"
            assert np.array_equal(hops, r["hops"][k]) and np.array_equal(parent, r["parent"][k]), sat
            assert one.reached == r["reached"][k], sat
            single_rounds = max(single_rounds, one.rounds)
        print(at + f"{info.rounds} rounds, {info.host_syncs} host waits; largest single solve {single_rounds} rounds")
        if one_walk_per_node:  # (module docstring, "Rounds of one batch")
            assert info.rounds >= single_rounds, at + f"{info.rounds} rounds < {single_rounds} of a single solve"
            assert info.rounds >= 2 * int(rh.max()), at + f"{info.rounds} rounds for keys of {int(rh.max())} hops"
        if targets is not None:
            t = np.asarray(targets, np.int64)
            assert r["cost_at"].shape == r["hops_at"].shape == (m, t.size), at
            assert np.array_equal(bits(r["cost_at"]), bits(r["cost"][:, t])), at + "cost_at"
            assert np.array_equal(r["hops_at"], r["hops"][:, t]), at + "hops_at"
    return r


@pytest.mark.parametrize("m", [1, 2, 5, 64])
@pytest.mark.parametrize("seed", [0, 7, 13])
def test_random_small(ref, engine, tmp_path, seed, m):
    g = with_isolated_node(fg.with_positions(fg.random_small(seed)))
    x = load_graph(engine, g, tmp_path)
    sources = small_sources(g, m, seed)
    if m >= 5:
        assert len(set(sources[:5])) == 4 and x.state[sources].min() == fg.INVALID and x.V - 1 in sources
    _check_batch(ref, engine, x, sources, targets=[x.V - 1, 0, 0, x.V // 2])


ODDITIES = fg.oddities()


@pytest.mark.parametrize("name", sorted(ODDITIES))
def test_oddities(ref, engine, tmp_path, name):
    """Three fields on every degenerate shape; V == 1 is three items on one node."""
    g, sources = ODDITIES[name]
    x = load_graph(engine, g, tmp_path)
    r = _check_batch(ref, engine, x, (list(sources) * 3)[:3])
    if name == "one_node":
        assert x.V == 1 and r["cost"].tolist() == [[0.0]] * 3 and r["hops"].tolist() == [[0]] * 3
        assert r["parent"].tolist() == [[-1]] * 3 and r["reached"].tolist() == [1, 1, 1]


@pytest.mark.parametrize("symmetric", [False, True], ids=["directed", "symmetric"])
def test_chain(ref, engine, tmp_path, symmetric):
    """Four fields that converge thousands of rounds apart under one threshold and one "work left" word: from
    node 0 the whole chain, from the middle half of it (both halves at once if symmetric), from the last node
    of a directed chain one round, from the one before it two."""
    V = 3000
    x = load_graph(engine, fg.chain(V, symmetric), tmp_path)
    r = _check_batch(ref, engine, x, [0, V - 1, V // 2, V - 2], scales=("4", "1e-6", "inf"),
                     one_walk_per_node=not symmetric)
    assert r["reached"].tolist() == ([V, V, V, V] if symmetric else [V, 1, V - V // 2, 2])
    assert r["info"].rounds >= 2 * (V - 1)


def test_star_long_row(ref, engine, tmp_path):
    """The hub's row of 30 000 (1 875 sixteen-lane trips) in one field while the two leaves' fields have one
    short row each in the same launch."""
    x = load_graph(engine, fg.star(30000), tmp_path)
    _check_batch(ref, engine, x, [0, 1, 1 + 30000 // 2], scales=("4", "0.5", "inf"))


def test_star_four_hubs(ref, engine, tmp_path):
    x = load_graph(engine, fg.star(4096, 4), tmp_path)
    _check_batch(ref, engine, x, [x.V - 1, 0, 4 + 4096 // 3])


def test_lattice(ref, engine, tmp_path):
    """Massive exact ties in eight fields at once: the parent rule (smallest id) holds per field."""
    n = 200
    x = load_graph(engine, fg.lattice(n, n), tmp_path)
    centre = (n // 2) * n + n // 2
    sources = [0, n - 1, n * (n - 1), n * n - 1, centre, 0, n // 2, centre + 1]
    r = _check_batch(ref, engine, x, sources, scales=("4", "inf"))
    ids = np.arange(n * n)
    iy, ix = np.divmod(ids, n)
    assert np.array_equal(r["hops"][0], ix + iy)
    assert np.array_equal(r["hops"][3], (n - 1 - ix) + (n - 1 - iy))
    assert np.array_equal(r["parent"][0][1:], np.where(iy > 0, ids - n, ids - 1)[1:])


@pytest.mark.parametrize("name", ["saturating_chain", "saturating_branch"])
def test_saturating(ref, engine, tmp_path, name):
    g = getattr(fg, name)()
    x = load_graph(engine, g, tmp_path)
    r = _check_batch(ref, engine, x, [0, 2, 1])
    assert np.isinf(r["cost"][0][r["hops"][0] >= 0]).any()  # reached at +inf


@pytest.mark.parametrize("V", [30, 2000])
@pytest.mark.parametrize("family", ["all_zero", "denormal"])
def test_cost_ranges(ref, engine, tmp_path, family, V):
    """A bucket width of zero (the threshold moves by the one-ulp bump alone) and a subnormal one, shared."""
    x = load_graph(engine, getattr(fg, family)(V, seed=V), tmp_path)
    _check_batch(ref, engine, x, [0, V - 1, V // 3])


LARGE = fg.RANDOM_LARGE[2000][2]  # V = 1 950


def _large_sources(V, m=16):
    return [0, V - 1, V // 4, 0] + [int(s) for s in np.random.default_rng(16).integers(0, V, size=m - 4)]


def test_random_large(ref, engine, tmp_path):
    x = load_graph(engine, random_large(*LARGE), tmp_path)
    assert x.V % 4 and (16 * x.V) % 64
    targets = np.random.default_rng(3).integers(0, x.V, size=700)  # more than one block, duplicates
    _check_batch(ref, engine, x, _large_sources(x.V), targets=targets)


def test_targets(ref, engine, tmp_path):
    """The gathered arrays are the full arrays at the targets: duplicates, an unreached node, an Invalid one and
    a saturated one; no targets at all; and only the gathered arrays with full=False."""
    x = load_graph(engine, fg.saturating_branch(), tmp_path)
    sources = [0, 7, 2]
    targets = [3, 3, 12, 5, 0, 11, 7, 3]
    r = _check_batch(ref, engine, x, sources, targets=targets)
    assert np.isposinf(r["cost_at"][0, 3]) and r["hops_at"][0, 3] == 4      # saturated: reached at +inf
    assert np.isposinf(r["cost_at"][0, 2]) and r["hops_at"][0, 2] == -1     # unreached
    assert r["cost_at"][1, 6] == 0 and r["hops_at"][1, 6] == 0              # a source among the targets
    g = engine.cost_fields(source_ids=sources, targets=targets, full=False)
    assert sorted(g) == ["cost_at", "hops_at", "info", "reached", "sources"]
    assert np.array_equal(bits(g["cost_at"]), bits(r["cost_at"])) and np.array_equal(g["hops_at"], r["hops_at"])
    assert g["reached"].tolist() == r["reached"].tolist() and g["sources"].tolist() == sources
    z = engine.cost_fields(source_ids=sources, targets=[], full=False)
    assert z["cost_at"].shape == z["hops_at"].shape == (3, 0) and z["reached"].tolist() == r["reached"].tolist()
    h = engine.cost_fields(source_ids=sources)
    assert sorted(h) == ["cost", "hops", "info", "parent", "reached", "sources"]


def test_engine_state_sequence(ref, tmp_path):
    """One engine: a batch of 16 on a large graph, a single field, a batch of 3 on a small graph, the first batch
    again -- buffers sized for m * V serve V and a smaller m * V, and every solve initialises its own stamps."""
    import trg_planner
    e = trg_planner.Engine(safety_factor=3.0, **PARAMS)
    big = random_large(*LARGE)
    xb = load_graph(e, big, tmp_path, "big")
    src_big = _large_sources(xb.V)
    first = _check_batch(ref, e, xb, src_big, scales=("4",))
    cost, hops, parent, info = e.cost_field(source_id=src_big[2])
    assert np.array_equal(bits(cost), bits(first["cost"][2])) and np.array_equal(hops, first["hops"][2])
    assert np.array_equal(parent, first["parent"][2]) and info.reached == first["reached"][2]
    xs = load_graph(e, with_isolated_node(fg.with_positions(fg.random_small(5))), tmp_path, "small")
    assert xs.V * 40 < xb.V
    _check_batch(ref, e, xs, [0, xs.V - 1, 0], scales=("4",))
    xb = load_graph(e, big, tmp_path, "big_again")
    again = _check_batch(ref, e, xb, src_big, scales=("4",))
    for key in ("cost", "hops", "parent"):
        assert np.array_equal(bits(again[key]), bits(first[key])), key
    e.close()


def _frontier_choice(g, rc, rh):
    fr = np.flatnonzero((g.state == 1) & np.isfinite(rc) & (rh >= 0))
    return None if fr.size == 0 else int(fr[np.lexsort((fr, rh[fr], rc[fr]))[0]])


def _check_poses(ref, e, g, poses):
    """cost_fields(sources_xy), cheapest_frontiers and cost_matrix for `poses` on the engine's current graph."""
    singles = [e.cost_field(source_xy=p) for p in poses]
    want_src = [int(s[3].source) for s in singles]
    r = e.cost_fields(sources_xy=poses)
    assert r["sources"].tolist() == want_src
    rc, rh, rp = reference_fields(ref, g, 3.0, want_src)
    assert_rows("sources_xy: ", "costs", r["cost"], rc, as_bits=True)
    assert_rows("sources_xy: ", "hops", r["hops"], rh)
    assert_rows("sources_xy: ", "parents", r["parent"], rp)
    for k, (cost, hops, parent, info) in enumerate(singles):
        assert np.array_equal(bits(cost), bits(r["cost"][k])) and np.array_equal(hops, r["hops"][k])
        assert np.array_equal(parent, r["parent"][k]) and info.reached == r["reached"][k]
    # a mix of ids and positions: -1 takes the position
    mixed = e.cost_fields(sources_xy=poses, source_ids=[-1, want_src[1]] + [-1] * (len(poses) - 2), full=False)
    assert mixed["sources"].tolist() == want_src and mixed["reached"].tolist() == r["reached"].tolist()
    # the cheapest Frontier node per pose
    both = e.cheapest_frontiers(poses)
    assert len(both) == len(poses)
    chosen = 0
    for k, p in enumerate(poses):
        one = e.cheapest_frontier(p)
        assert both[k] == one, (k, both[k], one)
        want = _frontier_choice(g, rc[k], rh[k])
        assert (one is None) == (want is None)
        if one is not None:
            chosen += 1
            assert one[0] == want and F32(one[1]) == rc[k][want] and one[2][0] == want_src[k] and one[2][-1] == want
    # the cost matrix between the poses' nodes, by position and by id
    for arg in (poses, np.array(want_src, np.int32)):
        mc, mh, nodes = e.cost_matrix(arg)
        assert nodes.tolist() == want_src
        assert np.array_equal(bits(mc), bits(rc[:, want_src])) and np.array_equal(mh, rh[:, want_src])
        assert not mc.diagonal().any() and not mh.diagonal().any()
    return chosen


def test_device_built_graph(ref, mountain_small):
    """Sources from positions on the CSR the device build left in HBM, then on the uploaded CSR after an
    updateGraph."""
    import trg_planner
    e = trg_planner.Engine(**MOUNTAIN)
    e.set_sampler(7, 16)
    e.set_global_map(mountain_small)
    e.init_graph([15.0, 15.0, 0.0])
    assert e.stats()["used_device_bfs"] == 1, e.fallback_reason
    poses = np.array([(15.0, 15.0), (8.3, 21.7), (14.0, 16.0), (21.0, 9.5)], np.float32)
    g = e.graph("global")
    _check_poses(ref, e, g, poses)
    pose = (12.0, 12.0)
    e.set_local_map(pose, obs_crop(mountain_small, pose, 4.0, box=(pose[0] + 2.0, pose[1] + 1.0, 0.6)))
    e.update_graph()
    g2 = e.graph("global")
    _check_poses(ref, e, g2, poses)
    e.close()


def test_cheapest_frontiers_json_graph(ref, engine, tmp_path):
    """Frontier nodes for certain: the random family marks an eighth of its nodes Frontier."""
    g = fg.with_positions(fg.random_small(3))
    x = load_graph(engine, g, tmp_path)
    engine.set_option("field_delta_scale", "4")
    poses = g.pos[[0, 1, x.V - 1, x.V // 2, 0], :2].copy()
    assert _check_poses(ref, engine, x, poses) >= 1


def test_matrix_in_chunks(ref, engine, tmp_path):
    """More waypoints than one batch holds: chunks of sources against the full target list."""
    x = load_graph(engine, fg.lattice(24, 24), tmp_path)
    engine.set_option("field_delta_scale", "4")
    nodes = (np.arange(70) * 8) % x.V
    mc, mh, ids = engine.cost_matrix(nodes.astype(np.int32))
    rc, rh, _ = reference_fields(ref, x, 3.0, nodes)
    assert ids.tolist() == nodes.tolist() and mc.shape == mh.shape == (70, 70)
    assert np.array_equal(bits(mc), bits(rc[:, nodes])) and np.array_equal(mh, rh[:, nodes])


def test_errors(ref, engine, tmp_path):
    import trg_planner

    def status_of(**kw):
        with pytest.raises(trg_planner.TrgError) as ei:
            engine.cost_fields(**kw)
        return ei.value.status, str(ei.value)

    x = load_graph(engine, fg.with_positions(fg.random_small(1)), tmp_path)
    V = x.V
    NO_GRAPH = 5
    assert status_of(source_ids=[])[0] == INVALID_ARG                     # m = 0
    assert status_of(source_ids=[0] * 65)[0] == INVALID_ARG               # m = 65
    st, msg = status_of(source_ids=[0, 1, -2])
    assert st == INVALID_ARG and "source 2" in msg, msg
    st, msg = status_of(source_ids=[0, V, 1])
    assert st == INVALID_ARG and "source 1" in msg, msg
    st, msg = status_of(source_ids=[0, 1], targets=[0, 1, 2, V])
    assert st == INVALID_ARG and "target 3" in msg, msg
    st, msg = status_of(source_ids=[0, 1], targets=[-1])
    assert st == INVALID_ARG and "target 0" in msg, msg
    st, msg = status_of(source_ids=[0, -1])                                # -1 needs a position
    assert st == INVALID_ARG and "source 1" in msg, msg
    # the engine still solves after the refusals
    _check_batch(ref, engine, x, [0, V - 1], scales=("4",))
    nodes = [((0.0, 0.0, 0.0), 0), ((1.0, 0.0, 0.0), 0), ((2.0, 0.0, 0.0), 0)]
    p = tmp_path / "neg.json"
    write_graph(p, nodes, [(0, 1, 0.0, 1.0), (1, 2, -1.0, 1.0)])         # safety_factor * weight + 1 < 0
    engine.load_json(str(p))
    assert status_of(source_ids=[0, 1])[0] == INVALID_ARG
    p = tmp_path / "empty.json"
    write_graph(p, [], [])
    engine.load_json(str(p))
    assert status_of(source_ids=[0, 0])[0] == NO_GRAPH
