"""GPU: trg_engine_risk_field_refresh / Engine.refresh_risk_fields ("Risk fields") -- the retained
risk solve of graph A brought to graph B through a node map equals, bit for bit, a fresh risk solve on B: risk bits,
hops, parents, reached counts against the host Dijkstra on the (risk, hops) key (tests/cpp/risk_reference.cpp), owners
against risk_ref.owners, `carried` against the refresh written out on the host (tests/risk_refresh_ref.py).  The pairs
are those of tests/risk_refresh_pairs.py (tests/test_risk_field_refresh_cpu.py shows on the CPU that they bite), each
with one field (the kernels without the item decode) and three, at a bucket width of 4 mean risks and at one bucket
per distinct risk; then the same graph under three maps, sets, routes, the refusals, a bad weight, cost and risk
refreshes in turn, the real path through update_graph's own node map, and the frontier helpers with reuse=True."""
import numpy as np
import pytest

import field_graphs as fg
import field_ref
import refresh_pairs as rp
import risk_ref
import risk_refresh_pairs as rrp
import risk_refresh_ref as rrr
from field_support import INVALID_ARG, MOUNTAIN, assert_rows, bits, engine, load_graph, reference_fields  # noqa: F401
from graph_support import obs_crop

pytestmark = pytest.mark.gpu
SF = MOUNTAIN["safety_factor"]
SCALES = ("4", "1e-6")
# (chain_cut / chain_join have all-zero weights: bucket width 0, only hops change.  The star's removed edge weighs 0.2
# and is tight for no key, so under max the pair changes nothing: 30 001 keys carried over a row of 30 000 edges, 0
# rounds -- the "touched nothing" case at the largest size.)
PAIRS = ("chain_cut", "chain_join", "random", "lattice", "invalid", "star", "risk_plateau", "levels", "peak_down",
         "peak_up", "duplicates_swapped")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """The compiled host Dijkstra of the risk field, once per module."""
    return risk_ref.compile_reference(tmp_path_factory.mktemp("risk_ref"))


@pytest.fixture(scope="module")
def cost_ref(tmp_path_factory):
    """The compiled host Dijkstra of the cost field, for the test that refreshes both kinds in turn."""
    return field_ref.compile_reference(tmp_path_factory.mktemp("field_ref"))


class Graphs:
    """The pairs, their JSON files (written and checked through load_graph once, loaded from the file afterwards)
    and the host fields, each computed once per module."""

    def __init__(self, tmp):
        self.tmp = tmp
        self.pairs = rrp.all_pairs()
        self.pairs["risk_sets"] = rrp.risk_sets_pair()
        self.files = {}
        self.fields = {}

    def load(self, e, name, side):
        g = getattr(self.pairs[name], side)
        key = f"{name}_{side}"
        if key not in self.files:
            load_graph(e, g, self.tmp, key)
            self.files[key] = str(self.tmp / f"{key}.json")
        else:
            e.load_json(self.files[key])
        return g

    def host(self, lib, name, side, sources):
        """The reference's (m, V) risk, hops, parent of the pair's graph, one Dijkstra per (graph, source) and module."""
        g = getattr(self.pairs[name], side)
        for s in sources:
            if (name, side, int(s)) not in self.fields:
                st, *rest = risk_ref.risk_of_graph(lib, g, int(s))
                assert st == 0
                self.fields[name, side, int(s)] = rest
        return tuple(np.stack([self.fields[name, side, int(s)][i] for s in sources]) for i in range(3))


@pytest.fixture(scope="module")
def graphs(tmp_path_factory):
    return Graphs(tmp_path_factory.mktemp("risk_refresh"))


def assert_fields(at, r, want):
    risk, hops, parent = want
    assert_rows(at, "risks", r["risk"], risk, as_bits=True)
    assert_rows(at, "hops", r["hops"], hops)
    assert_rows(at, "parents", r["parent"], parent)
    assert np.array_equal(r["reached"], (hops >= 0).sum(axis=1)), at


def refreshed(e, lib, graphs, name, m, scale, new2old=None, **kw):
    """Solve on A, load B, refresh with the pair's map (or new2old) -> (pair, result), after comparing the result
    with the host Dijkstra on B from sources_out and `carried` with the host refresh."""
    p = graphs.pairs[name]
    n2o = p.new2old if new2old is None else new2old
    at = f"{name}, m = {m}, scale {scale}: "
    e.set_option("field_delta_scale", scale)
    graphs.load(e, name, "a")
    src = p.sources[:m]
    e.risk_fields(source_ids=src)
    graphs.load(e, name, "b")
    r = e.refresh_risk_fields(new2old=n2o, **kw)
    first = {}
    for v, o in enumerate(n2o.tolist()):
        first.setdefault(o, v)
    assert r["sources"].tolist() == [first[int(s)] for s in src], at
    assert "owner" not in r and "owner_at" not in r, at  # (risk_fields: sets of one, no owners)
    if kw.get("full", True):
        assert_fields(at, r, graphs.host(lib, name, "b", r["sources"]))
    ra, ha, _ = graphs.host(lib, name, "a", src)
    carried = [rrr.carried(p.b, rrr.keys_of(ra[k], ha[k]), n2o, [int(r["sources"][k])]) for k in range(m)]
    assert r["carried"].tolist() == carried, at + f"carried {r['carried'].tolist()} != {carried}"
    return p, r


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("name", PAIRS)
def test_refresh_equals_a_fresh_solve(engine, ref, graphs, name, m, scale):
    e = engine
    if name == "risk_plateau":
        # what the pair is for, on the host reference, before the engine is asked: node 1 gets safer, node 2 keeps
        # its risk bits and changes its hops
        (ra, ha, _), (rb, hb, _) = graphs.host(ref, name, "a", [0]), graphs.host(ref, name, "b", [0])
        assert rb[0, 1] < ra[0, 1] and bits(rb[0, 2]) == bits(ra[0, 2]) and (ha[0, 2], hb[0, 2]) == (2, 4)
    p, r = refreshed(e, ref, graphs, name, m, scale)
    print(f"{name}, m = {m}, scale {scale}: V {len(p.b.state)}, carried {r['carried'].tolist()}, reached "
          f"{r['reached'].tolist()}, {r['info'].rounds} rounds, {r['info'].host_syncs} host waits")
    if name == "chain_cut":  # everything behind the cut is unreached, and nothing of it was carried
        assert (r["hops"][:, 900:] == -1).all() and r["carried"].tolist() == [900] * m
    if name == "chain_join":
        # 100 nodes to relabel against 1 000, a node per round in both passes: a margin of 2.5
        fresh = e.risk_fields(source_ids=r["sources"])
        print(f"chain_join: {r['info'].rounds} refresh rounds, {fresh['info'].rounds} fresh rounds")
        assert 0 < 4 * r["info"].rounds <= fresh["info"].rounds, (r["info"].rounds, fresh["info"].rounds)
        assert_fields(f"{name}, fresh: ", fresh, graphs.host(ref, name, "b", r["sources"]))
    if name in ("peak_down", "peak_up"):  # every risk word behind the peak is another, and every hop count stays
        ra, ha, _ = graphs.host(ref, name, "a", p.sources[:m])
        assert (r["risk"][:, rrp.PEAK_EDGE + 1:] != ra[:, rrp.PEAK_EDGE + 1:]).all() and np.array_equal(r["hops"], ha)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("kind", ["identity", "scrambled", "none"])
def test_same_graph_whatever_the_map(engine, ref, graphs, kind, m, scale):
    """A to A: with the identity map nothing is relaxed (0 rounds) and every reached node is carried; a scrambled
    map moves the sources and still gives the exact fields from where they are now; a map of -1 but for the sources
    carries the sources alone."""
    e = engine
    name = "levels"
    p = graphs.pairs[name]
    V = len(p.a.state)
    src = p.sources[:m]
    e.set_option("field_delta_scale", scale)
    graphs.load(e, name, "a")
    e.risk_fields(source_ids=src)
    graphs.load(e, name, "a")
    n2o = np.arange(V, dtype=np.int32)
    if kind == "scrambled":
        n2o = np.random.default_rng(5).permutation(V).astype(np.int32)
    if kind == "none":
        n2o[:] = -1
        n2o[src] = src
    r = e.refresh_risk_fields(new2old=n2o)
    at = f"{kind}, m = {m}, scale {scale}: "
    assert_fields(at, r, graphs.host(ref, name, "a", r["sources"]))
    ra, ha, _ = graphs.host(ref, name, "a", src)
    carried = [rrr.carried(p.a, rrr.keys_of(ra[k], ha[k]), n2o, [int(r["sources"][k])]) for k in range(m)]
    assert r["carried"].tolist() == carried, at
    if kind == "identity":
        assert r["info"].rounds == 0 and r["sources"].tolist() == list(src)
        assert np.array_equal(r["carried"], r["reached"])
    if kind == "none":
        assert r["carried"].tolist() == [1] * m and r["sources"].tolist() == list(src)


@pytest.mark.parametrize("scale", SCALES)
def test_refresh_of_a_set_solve(engine, ref, graphs, scale):
    """Two sets, one with a member named twice: risk, hops, parents, owners at every node and at targets and the owned
    counts after the refresh are the reference's on B from the members where they are now; routes start at the
    owners."""
    e = engine
    p = graphs.pairs["risk_sets"]
    e.set_option("field_delta_scale", scale)
    graphs.load(e, "risk_sets", "a")
    e.risk_fields_from(p.sets)
    graphs.load(e, "risk_sets", "b")
    now = rp.new_sets(p)
    targets = np.arange(0, len(p.b.state), 37, dtype=np.int32)
    r = e.refresh_risk_fields(new2old=p.new2old, targets=targets)
    assert r["sources"].tolist() == [s[0] for s in now]
    for k, members in enumerate(now):
        st, rr, rh, rpar = risk_ref.risk_of_graph(ref, p.b, members)
        assert st == 0
        owner, owned = risk_ref.owners(members, rh, rpar)
        at = f"set {k}, scale {scale}: "
        assert_rows(at, "risks", r["risk"][k:k + 1], rr[None], as_bits=True)
        assert_rows(at, "hops", r["hops"][k:k + 1], rh[None])
        assert_rows(at, "parents", r["parent"][k:k + 1], rpar[None])
        assert_rows(at, "owners", r["owner"][k:k + 1], owner[None])
        assert np.array_equal(r["owner_at"][k], owner[targets]) and np.array_equal(r["hops_at"][k], rh[targets]), at
        assert np.array_equal(bits(r["risk_at"][k]), bits(rr[targets])), at
        assert np.array_equal(np.bincount(r["owner"][k][r["owner"][k] >= 0], minlength=len(members)), owned), at
        assert r["reached"][k] == int((rh >= 0).sum()) == int(owned.sum()), at
        st, oa_, oh, _ = risk_ref.risk_of_graph(ref, p.a, p.sets[k])
        assert r["carried"][k] == rrr.carried(p.b, rrr.keys_of(oa_, oh), p.new2old, members), at
        far = int(np.argmax(rh))
        ids, _, info = e.routes([k], [far], xyz=False)[0]
        assert info.num_nodes == rh[far] + 1 and ids[0] == members[owner[far]] and ids[-1] == far, at
        assert np.array_equal(ids, risk_ref.route(p.b, rr, rh, rpar, far)[0]), at


def check_routes(e, g, fields, pairs, at):
    """Routes of the retained solve against the host walk; fields: (risk, hops, parent) per field."""
    got = e.routes([k for k, _ in pairs], [t for _, t in pairs], xyz=False)
    for (k, t), (ids, _, one) in zip(pairs, got):
        rr, rh, rpar = fields[k]
        want_ids, edges, cost, pl, avg = risk_ref.route(g, rr, rh, rpar, t)
        where = at + f"field {k}, target {t}: "
        assert np.array_equal(ids, want_ids), where + f"{ids} != {want_ids}"
        assert one.num_nodes == want_ids.size, where
        assert bits(one.cost) == bits(cost), where + f"cost {one.cost!r}"
        assert bits(one.path_length) == bits(pl), where + f"path_length {one.path_length!r} != {pl!r}"
        assert bits(one.avg_risk) == bits(avg), where + f"avg_risk {one.avg_risk!r} != {avg!r}"


def test_routes_and_reached_answer_from_the_refreshed_solve(engine, ref, graphs):
    e = engine
    # the exchanged duplicates: no key changes, and the route edge into node 1 is the other one (dist 1, not 2)
    p, r = refreshed(e, ref, graphs, "duplicates_swapped", 2, "4")
    fields = [tuple(a[k] for a in graphs.host(ref, "duplicates_swapped", "b", r["sources"])) for k in range(2)]
    check_routes(e, p.b, fields, [(k, t) for k in range(2) for t in range(4)], "duplicates_swapped: ")
    one = e.routes([0], [1], xyz=False)[0][2]
    assert one.path_length == np.float32(1.0) and one.cost == np.float32(0.2), (one.path_length, one.cost)
    # levels, nothing of V entries copied back: the parent sweep runs with the first routes call
    p, r = refreshed(e, ref, graphs, "levels", 3, "4", full=False)
    assert "parent" not in r and "risk" not in r
    risk, hops, parent = graphs.host(ref, "levels", "b", r["sources"])
    V = len(p.b.state)
    check_routes(e, p.b, [(risk[k], hops[k], parent[k]) for k in range(3)],
                 [(k, t) for k in range(3) for t in range(k, V, 97)], "levels, late parent sweep: ")
    for k in range(3):
        ids, c, h = e.field_reached(k)
        assert np.array_equal(ids, np.flatnonzero(hops[k] >= 0))
        assert np.array_equal(bits(c), bits(risk[k][ids])) and np.array_equal(h, hops[k][ids])


def test_refusals_leave_the_solve_as_it_was(engine, ref, graphs):
    import trg_planner
    e = engine
    name = "invalid"
    p = graphs.pairs[name]
    V = len(p.b.state)
    ident = rp.identity(p.b)
    e.set_option("field_delta_scale", "4")

    def refused(words, call=None, **kw):
        with pytest.raises(trg_planner.TrgError) as ei:
            (call or e.refresh_risk_fields)(**kw)
        assert ei.value.status == INVALID_ARG and all(w in str(ei.value) for w in words), str(ei.value)

    def still_stale():
        with pytest.raises(trg_planner.TrgError) as ei:
            e.routes([0], [0])
        assert ei.value.status == INVALID_ARG and "earlier graph" in str(ei.value)

    e.reset_graph("global")  # (drops the field buffers with the graph)
    graphs.load(e, name, "a")
    refused(["no cost-field solve is retained"], new2old=ident)
    # a cost solve is the other call's, and a risk solve not the cost call's
    e.cost_fields(source_ids=p.sources)
    graphs.load(e, name, "b")
    refused(["risk field refresh", "retained solve is a cost field", "trg_engine_cost_field_refresh"], new2old=ident)
    still_stale()
    graphs.load(e, name, "a")
    e.risk_fields(source_ids=p.sources)
    graphs.load(e, name, "b")
    refused(["cost field refresh", "retained solve is a risk field", "trg_engine_risk_field_refresh"],
            call=e.refresh_fields, new2old=ident)
    still_stale()
    graphs.load(e, name, "a")
    e.risk_fields(source_ids=p.sources, budget=0.3)
    graphs.load(e, name, "b")
    refused(["bounded"], new2old=ident)
    still_stale()
    graphs.load(e, name, "a")
    e.risk_fields(source_ids=p.sources)
    refused(["already of the current graph"], new2old=ident)
    assert e.routes([0], [p.sources[0]])[0][2].num_nodes == 1  # ... and still current
    graphs.load(e, name, "b")
    refused(["no node map", "solve again"])  # load_json leaves the engine no map
    still_stale()
    refused(["node map has", str(V - 1)], new2old=ident[:V - 1])
    bad = ident.copy()
    bad[5] = V
    refused(["entry 5", str(V)], new2old=bad)
    bad[5] = -2
    refused(["entry 5"], new2old=bad)
    gone = ident.copy()
    gone[p.sources[1]] = -1
    # (risk_fields runs every source as a set of one: the message names the set and its one member)
    refused(["member 0 of set 1", f"node {p.sources[1]}", "has no node in the current graph"], new2old=gone)
    with pytest.raises(trg_planner.TrgError) as ei:
        e.refresh_risk_fields(new2old=ident, targets=[V])
    assert ei.value.status == INVALID_ARG and "target 0" in str(ei.value)
    still_stale()
    r = e.refresh_risk_fields(new2old=ident)  # after all of them the stale solve is still there to be refreshed
    assert_fields("after the refusals: ", r, graphs.host(ref, name, "b", r["sources"]))
    assert e.routes([0], [int(r["sources"][0])])[0][2].num_nodes == 1


def test_bad_weight_on_the_new_graph(engine, tmp_path):
    """A NaN weight in B: the refresh fails as a fresh risk solve of B does, naming the weight, after the retained
    solve is gone."""
    import trg_planner
    e = engine
    e.set_option("field_delta_scale", "4")
    p = rrp.bad_b_pair()
    load_graph(e, p.a, tmp_path, "bad_a")
    e.risk_fields(source_ids=[0])
    assert e.routes([0], [1], xyz=False)[0][2].num_nodes == 2
    path = tmp_path / "bad_b.json"
    fg.write_json(path, p.b)
    e.load_json(str(path))
    assert int(np.isnan(e.graph("global").w).sum()) == 1
    with pytest.raises(trg_planner.TrgError) as ei:
        e.refresh_risk_fields(new2old=p.new2old)
    msg = str(ei.value)
    assert ei.value.status == INVALID_ARG and "weight" in msg and "retained" not in msg, msg
    for call in (lambda: e.routes([0], [1], xyz=False), lambda: e.refresh_risk_fields(new2old=p.new2old)):
        with pytest.raises(trg_planner.TrgError) as ei:
            call()
        assert ei.value.status == INVALID_ARG and "no cost-field solve is retained" in str(ei.value), str(ei.value)


def test_cost_and_risk_refreshes_in_turn(engine, ref, cost_ref, graphs):
    """Cost solve, update, refresh_fields, risk solve, update, refresh_risk_fields, twice: each equal to its
    reference on the graph it ends on (the edge costs and the edge risks lie in slots of one cache)."""
    e = engine
    e.set_option("field_delta_scale", "4")
    p = graphs.pairs["levels"]
    src = p.sources[:2]
    for _ in range(2):
        graphs.load(e, "levels", "a")
        e.cost_fields(source_ids=src)
        graphs.load(e, "levels", "b")
        r = e.refresh_fields(new2old=p.new2old)
        cost, hops, parent = reference_fields(cost_ref, p.b, SF, r["sources"])
        assert_rows("cost refresh: ", "costs", r["cost"], cost, as_bits=True)
        assert_rows("cost refresh: ", "hops", r["hops"], hops)
        assert_rows("cost refresh: ", "parents", r["parent"], parent)
        e.risk_fields(source_ids=r["sources"])  # on B
        graphs.load(e, "levels", "a")
        back = np.full(len(p.a.state), -1, np.int32)  # A's ids from B's: the map the other way
        back[p.new2old[p.new2old >= 0]] = np.flatnonzero(p.new2old >= 0)
        r = e.refresh_risk_fields(new2old=back)
        assert r["sources"].tolist() == list(src)
        assert_fields("risk refresh: ", r, graphs.host(ref, "levels", "a", src))


def terrain(synth):
    """The 160 x 160 terrain of tests/test_gpu_risk_field.py's device-build test, built on the device -> (engine,
    cloud)."""
    import trg_planner
    cloud = synth.mountain_cloud(160, 160, seed=11, amplitude=5.0, wavelength=14.0)
    e = trg_planner.Engine(**MOUNTAIN)
    e.set_sampler(7, 16)
    e.set_global_map(cloud)
    e.init_graph([8.0, 8.0, 0.0])
    return e, cloud


def update(e, cloud, pose, box=None):
    box = (pose[0] + 2.0, pose[1] + 1.0, 0.6) if box is None else box
    e.set_local_map(pose, obs_crop(cloud, pose, 4.0, box=box))
    e.update_graph()


def map_by_position(xa, xb):
    """new2old from node positions: the id in graph xa of the node at each position of graph xb, -1 for none (the
    engine's own map is not exported; an update keeps a node's position bit for bit)."""
    where = {row.tobytes(): i for i, row in enumerate(np.ascontiguousarray(xa.xyz))}
    return np.array([where.get(row.tobytes(), -1) for row in np.ascontiguousarray(xb.xyz)], np.int32)


UPDATE_POSES = [(6.0, 6.0), (7.0, 6.5), (8.0, 7.0)]


def test_refresh_through_update_graph(ref, synth):
    """The real path: a map-built graph, the risk field from the root, an update with an obstacle; refresh_risk_fields()
    with the engine's own map equals the reference on the exported CSR and a fresh solve; then two updates before one
    refresh.  On the reference's fields the first update changes a key of a node that both graphs have, and the keys
    that survive the anchor are fewer than the nodes: the refresh had something to do."""
    e, cloud = terrain(synth)
    try:
        xa = e.graph("global")
        first = e.risk_fields(sources_xy=[(8.0, 8.0)])
        src = int(first["sources"][0])
        st, ra, ha, _ = risk_ref.risk_of_graph(ref, xa, src)
        assert st == 0
        update(e, cloud, UPDATE_POSES[0])
        r = e.refresh_risk_fields()
        xb = e.graph("global")
        now = int(r["sources"][0])
        assert np.array_equal(bits(xb.xyz[now]), bits(xa.xyz[src]))  # the source is the node it was
        st, rb, hb, pb = risk_ref.risk_of_graph(ref, xb, now)
        assert st == 0
        assert_fields("update 0: ", r, (rb[None], hb[None], pb[None]))
        n2o = map_by_position(xa, xb)
        assert n2o[now] == src
        ka, kb = rrr.keys_of(ra, ha), rrr.keys_of(rb, hb)
        changed = int(((n2o >= 0) & (kb != ka[np.maximum(n2o, 0)])).sum())
        host_carried = rrr.carried(xb, ka, n2o, [now])
        print(f"update 0: V {xa.V} -> {xb.V}, {int((n2o < 0).sum())} new nodes, {changed} keys changed through the map, "
              f"carried {r['carried'].tolist()} (host, by position: {host_carried}), reached {r['reached'].tolist()}, "
              f"{r['info'].rounds} rounds")
        assert changed >= 1 and host_carried < xb.V
        assert 0 < r["carried"][0] < xb.V and r["info"].rounds > 0
        positive = np.flatnonzero(np.isfinite(rb) & (rb > 0))
        check_routes(e, xb, [(rb, hb, pb)], [(0, int(positive[-1])), (0, now)], "update 0: ")
        fresh = e.risk_fields(source_ids=[now])
        for key in ("risk", "hops", "parent", "reached"):
            assert np.array_equal(r[key].view(np.uint32), fresh[key].view(np.uint32)), key
        # two updates, the map composed over both, one refresh
        for pose in UPDATE_POSES[1:3]:
            update(e, cloud, pose)
        r = e.refresh_risk_fields()
        xc = e.graph("global")
        assert np.array_equal(bits(xc.xyz[r["sources"][0]]), bits(xa.xyz[src]))
        st, rc, hc, pc = risk_ref.risk_of_graph(ref, xc, int(r["sources"][0]))
        assert_fields("two updates: ", r, (rc[None], hc[None], pc[None]))
        print(f"two updates: V {xc.V}, carried {r['carried'].tolist()}, {r['info'].rounds} rounds")
    finally:
        e.close()


def test_frontier_helpers_reuse_the_retained_solve(ref, mountain_gentle):
    """frontier_ceilings / safest_frontier with reuse=True across updates: from the same pose the retained solve is
    refreshed (last_reuse holds the refresh's `carried` and info) and the answer is reuse=False's and the reference's;
    from a pose that resolves to another node the refresh is not taken and the answer is again the fresh one.  The
    gentle terrain and the update stream of tests/test_gpu_cost_field_refresh.py's real path, whose updates leave
    Frontier nodes; the first update comes before the first solve, so that there are some from the start."""
    import trg_planner
    cloud = mountain_gentle
    e = trg_planner.Engine(**dict(MOUNTAIN, update_collision_threshold=0.2))
    try:
        e.set_sampler(5, 16)
        e.set_global_map(cloud)
        e.init_graph([15.0, 15.0, 0.0])
        pose = (10.0, 10.0)
        stream = [(12.0, 12.0), (13.0, 12.5), (14.0, 13.0), (15.0, 13.5), (16.0, 14.0)]
        sizes = []  # Frontier nodes at every comparison

        def want(p):
            x = e.graph("global")
            node = int(e._resolve_nodes([p])[0])
            frontier = np.flatnonzero(x.state == 1).astype(np.int32)
            st, rr, rh, rpar = risk_ref.risk_of_graph(ref, x, node)
            assert st == 0
            return x, frontier, rr, rh, rpar

        def same(got, p):
            x, frontier, rr, rh, _ = want(p)
            sizes.append(int(frontier.size))
            assert np.array_equal(got[0], frontier)
            assert np.array_equal(bits(got[1]), bits(rr[frontier])) and np.array_equal(got[2], rh[frontier])

        update(e, cloud, stream[0])
        got = e.frontier_ceilings(pose, reuse=True)  # nothing retained: solved afresh
        assert e.last_reuse is None
        same(got, pose)
        update(e, cloud, stream[1])
        got = e.frontier_ceilings(pose, reuse=True)
        assert e.last_reuse is not None and 0 < e.last_reuse["carried"][0] and e.last_reuse["info"].source >= 0
        print(f"frontier_ceilings, reuse: carried {e.last_reuse['carried'].tolist()}, "
              f"{e.last_reuse['info'].rounds} rounds, {got[0].size} frontier nodes")
        same(got, pose)
        again = e.frontier_ceilings(pose, reuse=False)
        assert e.last_reuse is None
        for a, b in zip(got, again):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        got = e.frontier_ceilings(pose, reuse=True)  # already current: refused, solved afresh
        assert e.last_reuse is None
        same(got, pose)
        update(e, cloud, stream[2])
        pick = e.safest_frontier(pose, reuse=True)
        assert e.last_reuse is not None and "carried" in e.last_reuse
        x, frontier, rr, rh, rpar = want(pose)
        ok = frontier[rh[frontier] >= 0]
        sizes.append(int(ok.size))
        if ok.size == 0:
            assert pick is None
        else:
            best = int(ok[np.lexsort((ok, rh[ok], rr[ok]))[0]])
            assert pick[0] == best and bits(pick[1]) == bits(rr[best]), (pick, best)
            assert pick[2] == risk_ref.route(x, rr, rh, rpar, best)[0].tolist()
        assert e.safest_frontier(pose, reuse=False) == pick and e.last_reuse is None
        # another node: the refresh is not the pose's field
        update(e, cloud, stream[3])
        other = (20.0, 19.0)
        assert int(e._resolve_nodes([other])[0]) != int(e._resolve_nodes([pose])[0])
        got = e.frontier_ceilings(other, reuse=True)
        assert e.last_reuse is None
        same(got, other)
        pick = e.safest_frontier(other, reuse=True)  # (already current)
        assert e.last_reuse is None and pick == e.safest_frontier(other, reuse=False)
        # a cost solve retained: the refresh refuses, the helper solves afresh
        e.cost_fields(sources_xy=[pose])
        update(e, cloud, stream[4])
        got = e.frontier_ceilings(pose, reuse=True)
        assert e.last_reuse is None
        same(got, pose)
        print(f"Frontier nodes at the comparisons: {sizes}")
        assert sizes[1] > 0 and sizes[3] > 0, sizes  # both that took the refresh read it at Frontier nodes (46, 48)
    finally:
        e.close()
