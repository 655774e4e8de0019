"""GPU: trg_engine_cost_field_refresh / Engine.refresh_fields ("Refresh") -- the retained solve
of graph A brought to graph B through a node map equals, bit for bit, a fresh solve on B: cost bits, hops, parents,
reached counts against the host Dijkstra (tests/cpp/field_reference.cpp), owners against tests/set_ref.py, `carried`
against the refresh written out on the host (tests/refresh_ref.py).  The pairs are those of tests/refresh_pairs.py
(tests/test_cost_field_refresh_cpu.py shows on the CPU that they bite), each with one field (the kernels without the
item decode) and three, at a bucket width of 4 mean costs and at one bucket per distinct cost; then the refusals, the
routes of a refreshed solve, and the real path: update_graph's own node map on a map-built graph."""
import ctypes as C

import numpy as np
import pytest

import field_graphs as fg
import refresh_pairs as rp
import refresh_ref as rr
import route_ref
import set_ref
from field_support import INVALID_ARG, MOUNTAIN, assert_rows, engine, load_graph, ref, reference_fields  # noqa: F401
from graph_support import obs_crop

pytestmark = pytest.mark.gpu
SF = MOUNTAIN["safety_factor"]
SCALES = ("4", "1e-6")
PAIRS = ("chain_cut", "chain_join", "random", "lattice", "plateau", "star", "invalid", "saturating_chain",
         "saturating_branch")


class Graphs:
    """The pairs, their JSON files (written and checked through load_graph once, loaded from the file afterwards)
    and the host fields, each computed once per module."""

    def __init__(self, tmp):
        self.tmp = tmp
        self.pairs = rp.all_pairs()
        self.pairs["sets"] = rp.set_pair()
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
        """reference_fields of the pair's graph, one Dijkstra per (graph, source) and module."""
        g = getattr(self.pairs[name], side)
        for s in sources:
            if (name, side, int(s)) not in self.fields:
                c, h, p = reference_fields(lib, g, SF, [int(s)])
                self.fields[name, side, int(s)] = c[0], h[0], p[0]
        return tuple(np.stack([self.fields[name, side, int(s)][i] for s in sources]) for i in range(3))


@pytest.fixture(scope="module")
def graphs(tmp_path_factory):
    return Graphs(tmp_path_factory.mktemp("refresh"))


def assert_fields(at, r, want):
    cost, hops, parent = want
    assert_rows(at, "costs", r["cost"], cost, as_bits=True)
    assert_rows(at, "hops", r["hops"], hops)
    assert_rows(at, "parents", r["parent"], parent)
    assert np.array_equal(r["reached"], (hops >= 0).sum(axis=1)), at


def refreshed(e, lib, graphs, name, m, scale, new2old=None):
    """Solve on A, load B, refresh with the pair's map (or new2old) -> (pair, result), after comparing the result
    with the host Dijkstra on B from sources_out and `carried` with the host refresh."""
    p = graphs.pairs[name]
    n2o = p.new2old if new2old is None else new2old
    at = f"{name}, m = {m}, scale {scale}: "
    e.set_option("field_delta_scale", scale)
    graphs.load(e, name, "a")
    src = p.sources[:m]
    e.cost_fields(source_ids=src)
    graphs.load(e, name, "b")
    r = e.refresh_fields(new2old=n2o)
    first = {}
    for v, o in enumerate(n2o.tolist()):
        first.setdefault(o, v)
    assert r["sources"].tolist() == [first[int(s)] for s in src], at
    assert_fields(at, r, graphs.host(lib, name, "b", r["sources"]))
    ca, ha, _ = graphs.host(lib, name, "a", src)
    carried = [rr.carried(p.b, SF, rr.keys_of(ca[k], ha[k]), n2o, [int(r["sources"][k])]) for k in range(m)]
    assert r["carried"].tolist() == carried, at
    return p, r


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("name", PAIRS)
def test_refresh_equals_a_fresh_solve(engine, ref, graphs, name, m, scale):
    e = engine
    if name == "plateau":
        # what the pair is for, on the host reference, before the engine is asked: node 1 gets cheaper, node 2 keeps
        # its cost bits and changes its hops
        (ca, ha, _), (cb, hb, _) = graphs.host(ref, name, "a", [0]), graphs.host(ref, name, "b", [0])
        assert cb[0, 1] < ca[0, 1] and cb[0, 2].view(np.uint32) == ca[0, 2].view(np.uint32) and hb[0, 2] != ha[0, 2]
    p, r = refreshed(e, ref, graphs, name, m, scale)
    if name == "chain_cut":  # everything behind the cut is unreached, and nothing of it was carried
        assert (r["hops"][:, 900:] == -1).all() and r["carried"].tolist() == [900] * m
    if name == "chain_join":
        # 100 nodes to relabel against 1 000, with a margin of 2.5 for keys that travel two hops in a round
        fresh = e.cost_fields(source_ids=r["sources"])
        assert 0 < 4 * r["info"].rounds <= fresh["info"].rounds, (r["info"].rounds, fresh["info"].rounds)
        assert_fields(f"{name}, fresh: ", fresh, graphs.host(ref, name, "b", r["sources"]))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("kind", ["identity", "scrambled", "none"])
def test_same_graph_whatever_the_map(engine, ref, graphs, kind, m, scale):
    """A to A: with the identity map nothing is relaxed (0 rounds) and every reached node is carried; a scrambled
    map moves the sources and still gives the exact fields from where they are now; a map of -1 but for the sources
    carries the sources alone."""
    e = engine
    name = "random"
    p = graphs.pairs[name]
    V = len(p.a.state)
    src = p.sources[:m]
    e.set_option("field_delta_scale", scale)
    graphs.load(e, name, "a")
    e.cost_fields(source_ids=src)
    graphs.load(e, name, "a")
    n2o = np.arange(V, dtype=np.int32)
    if kind == "scrambled":
        n2o = np.random.default_rng(5).permutation(V).astype(np.int32)
    if kind == "none":
        n2o[:] = -1
        n2o[src] = src
    r = e.refresh_fields(new2old=n2o)
    at = f"{kind}, m = {m}, scale {scale}: "
    want = graphs.host(ref, name, "a", r["sources"])
    assert_fields(at, r, want)
    ca, ha, _ = graphs.host(ref, name, "a", src)
    carried = [rr.carried(p.a, SF, rr.keys_of(ca[k], ha[k]), n2o, [int(r["sources"][k])]) for k in range(m)]
    assert r["carried"].tolist() == carried, at
    if kind == "identity":
        assert r["info"].rounds == 0 and r["sources"].tolist() == list(src)
        assert np.array_equal(r["carried"], r["reached"])
    if kind == "none":
        assert r["carried"].tolist() == [1] * m and r["sources"].tolist() == list(src)


@pytest.mark.parametrize("scale", SCALES)
def test_refresh_of_a_set_solve(engine, graphs, scale):
    """Two sets, one with a member named twice: cost, hops, parents, owners at every node and at targets after the
    refresh are tests/set_ref.py's on B; routes then start at the owners."""
    e = engine
    p = graphs.pairs["sets"]
    e.set_option("field_delta_scale", scale)
    graphs.load(e, "sets", "a")
    e.cost_fields_from(p.sets)
    graphs.load(e, "sets", "b")
    now = rp.new_sets(p)
    targets = np.arange(0, len(p.b.state), 37, dtype=np.int32)
    r = e.refresh_fields(new2old=p.new2old, targets=targets)
    assert r["sources"].tolist() == [s[0] for s in now]
    for k, members in enumerate(now):
        want = set_ref.set_field(p.b, SF, members)
        at = f"set {k}, scale {scale}: "
        assert_rows(at, "costs", r["cost"][k:k + 1], want.cost[None], as_bits=True)
        assert_rows(at, "hops", r["hops"][k:k + 1], want.hops[None])
        assert_rows(at, "parents", r["parent"][k:k + 1], want.parent[None])
        assert_rows(at, "owners", r["owner"][k:k + 1], want.owner[None])
        assert np.array_equal(r["owner_at"][k], want.owner[targets]) and np.array_equal(r["hops_at"][k], want.hops[targets])
        assert np.array_equal(np.bincount(r["owner"][k][r["owner"][k] >= 0], minlength=len(members)), want.owned)
        old = set_ref.set_field(p.a, SF, p.sets[k])
        assert r["carried"][k] == rr.carried(p.b, SF, rr.keys_of(old.cost, old.hops), p.new2old, members)
        far = int(np.argmax(want.hops))
        ids, _, info = e.routes([k], [far], xyz=False)[0]
        assert info.num_nodes == want.hops[far] + 1 and ids[0] == members[want.owner[far]] and ids[-1] == far


def test_routes_and_reached_answer_from_the_refreshed_solve(engine, ref, graphs):
    e = engine
    p, r = refreshed(e, ref, graphs, "random", 3, "4")
    cost, hops, parent = graphs.host(ref, "random", "b", r["sources"])
    fields = [(int(r["sources"][k]), cost[k], hops[k], parent[k]) for k in range(3)]
    V = len(p.b.state)
    pairs = [(k, t) for k in range(3) for t in range(k, V, 97)]
    got = e.routes([f for f, _ in pairs], [t for _, t in pairs], xyz=False)
    for (f, t), (ids, _, info), want in zip(pairs, got, route_ref.routes_of_graph(p.b, SF, fields, pairs)):
        assert np.array_equal(ids, want.ids), (f, t)
        assert info.num_nodes == len(want.ids)
        if len(want.ids):
            assert np.float32(info.cost).view(np.uint32) == want.cost.view(np.uint32)
            assert np.float32(info.path_length).view(np.uint32) == want.path_length.view(np.uint32)
    for k in range(3):
        ids, c, h = e.field_reached(k)
        assert np.array_equal(ids, np.flatnonzero(hops[k] >= 0))
        assert np.array_equal(c.view(np.uint32), cost[k][ids].view(np.uint32)) and np.array_equal(h, hops[k][ids])


def raw_refresh(e, n2o, owner=None):
    """The C entry with nothing but a map (and an owner output) -> status."""
    ip = C.POINTER(C.c_int32)
    return e.L.trg_engine_cost_field_refresh(
        e.h, None if n2o is None else n2o.ctypes.data_as(ip), 0 if n2o is None else n2o.shape[0], None, None, None,
        None, 0, None, None, None if owner is None else owner.ctypes.data_as(ip), None, None, None, None, None)


def test_refusals_leave_the_solve_as_it_was(engine, ref, graphs):
    import trg_planner
    e = engine
    name = "invalid"
    p = graphs.pairs[name]
    V = len(p.b.state)
    ident = rp.identity(p.b)
    e.set_option("field_delta_scale", "4")

    def refused(words, **kw):
        with pytest.raises(trg_planner.TrgError) as ei:
            e.refresh_fields(**kw)
        assert ei.value.status == INVALID_ARG and all(w in str(ei.value) for w in words), str(ei.value)

    def still_stale():
        with pytest.raises(trg_planner.TrgError) as ei:
            e.routes([0], [0])
        assert ei.value.status == INVALID_ARG and "earlier graph" in str(ei.value)

    e.reset_graph("global")  # (drops the field buffers with the graph)
    graphs.load(e, name, "a")
    refused(["no cost-field solve is retained"], new2old=ident)
    e.cost_fields(source_ids=p.sources, budget=1.0)
    graphs.load(e, name, "b")
    refused(["bounded"], new2old=ident)
    graphs.load(e, name, "a")
    e.cost_fields(source_ids=p.sources)
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
    refused(["source of field 1", f"node {p.sources[1]}"], new2old=gone)
    owner = np.empty((3, V), np.int32)
    assert raw_refresh(e, ident, owner) == INVALID_ARG
    assert "without sets" in e.L.trg_engine_last_error(e.h).decode()
    with pytest.raises(trg_planner.TrgError) as ei:
        e.refresh_fields(new2old=ident, targets=[V])
    assert ei.value.status == INVALID_ARG and "target 0" in str(ei.value)
    still_stale()
    r = e.refresh_fields(new2old=ident)  # after all of them the stale solve is still there to be refreshed
    assert_fields("after the refusals: ", r, graphs.host(ref, name, "b", r["sources"]))
    # a set whose member has no node: the message names the set and the member
    ps = graphs.pairs["sets"]
    graphs.load(e, "sets", "a")
    e.cost_fields_from(ps.sets)
    graphs.load(e, "sets", "b")
    gone = ps.new2old.copy()
    gone[gone == ps.sets[0][3]] = -1
    refused(["member 3 of set 0", f"node {ps.sets[0][3]}"], new2old=gone)
    still_stale()


def test_refresh_through_update_graph(oa, mountain_gentle, ref):
    """The real path: a map-built graph, two sources with parents, the three updates of tests/test_gpu_update.py;
    after each, refresh_fields() with the engine's own map equals a fresh cost_fields from the same nodes and the
    host Dijkstra on the exported CSR."""
    import trg_planner
    prm = dict(oa.MOUNTAIN, update_collision_threshold=0.2)
    e = trg_planner.Engine(**prm)
    try:
        e.set_sampler(5, 16)
        e.set_global_map(mountain_gentle)
        e.init_graph([15.0, 15.0, 0.0])
        first = e.cost_fields(sources_xy=[(10.0, 10.0), (20.0, 19.0)])
        xyz = e.graph("global").xyz[first["sources"]].copy()
        seen = []
        for k, pose in enumerate([(12.0, 12.0), (13.0, 12.5), (14.0, 13.0)]):
            obs = obs_crop(mountain_gentle, pose, 4.0, box=(pose[0] + 2.0, pose[1] + 1.0, 0.6))
            e.set_local_map(pose, obs)
            e.update_graph()
            r = e.refresh_fields()
            g = e.graph("global")
            V = g.V
            at = f"update {k}: "
            # the sources are the nodes they were: the same positions
            assert np.array_equal(g.xyz[r["sources"]].view(np.uint32), xyz.view(np.uint32)), at
            assert_fields(at, r, reference_fields(ref, g, prm["safety_factor"], r["sources"]))
            seen.append((r["carried"].tolist(), V))
            fresh = e.cost_fields(source_ids=r["sources"])
            for key in ("cost", "hops", "parent"):
                assert np.array_equal(r[key].view(np.uint32), fresh[key].view(np.uint32)), at + key
            assert np.array_equal(r["reached"], fresh["reached"]), at
        assert all(0 < c < seen[0][1] for c in seen[0][0]), f"carried, V per update: {seen}"
        # each refresh above crossed one update (the fresh solve starts the map again); now two updates, the map
        # composed over both, and one refresh
        for pose in [(15.0, 13.5), (16.0, 14.0)]:
            e.set_local_map(pose, obs_crop(mountain_gentle, pose, 4.0, box=(pose[0] + 2.0, pose[1] + 1.0, 0.6)))
            e.update_graph()
        r = e.refresh_fields()
        g = e.graph("global")
        assert np.array_equal(g.xyz[r["sources"]].view(np.uint32), xyz.view(np.uint32))
        assert_fields("two updates: ", r, reference_fields(ref, g, prm["safety_factor"], r["sources"]))
    finally:
        e.close()


def chain_without_last_link(V):
    """fg.chain(V) with the link V-2 -> V-1 removed: the last node is cut off."""
    g = fg.chain(V)
    a = np.arange(V - 2)
    return fg.from_edges(V, a, a + 1, g.w[:V - 2], g.dist[:V - 2])


# (host waits, rounds) of the solve, then (host waits, rounds, carried per field) of its refresh, as the parent of
# the commit that folded the refresh into the one solver gave them in two separate processes
# (profiles/r14_field_refresh_fold.md).  Keys: graphs, bucket width, fields or "sets".
REFRESH_WAITS = {
    ('chain_cut', '4', 'sets'): ((11, 250), (7, 0, (99, 89))),
    ('chain_cut', '4', 1): ((10, 200), (6, 0, (99,))),
    ('chain_cut', '4', 4): ((12, 280), (6, 0, (99, 98, 97, 96))),
    ('chain_cut', 'inf', 'sets'): ((11, 200), (7, 0, (99, 89))),
    ('chain_cut', 'inf', 1): ((10, 200), (6, 0, (99,))),
    ('chain_cut', 'inf', 4): ((10, 200), (6, 0, (99, 98, 97, 96))),
    ('chain_restored', '4', 'sets'): ((11, 246), (7, 8, (99, 89))),
    ('chain_restored', '4', 1): ((10, 198), (6, 4, (99,))),
    ('chain_restored', '4', 4): ((12, 276), (6, 8, (99, 98, 97, 96))),
    ('chain_restored', 'inf', 'sets'): ((11, 198), (7, 4, (99, 89))),
    ('chain_restored', 'inf', 1): ((10, 198), (6, 4, (99,))),
    ('chain_restored', 'inf', 4): ((10, 198), (6, 4, (99, 98, 97, 96))),
    ('one_node', '4', 1): ((4, 2), (6, 0, (1,))),
    ('one_node', '4', 4): ((4, 2), (6, 0, (1, 1, 1, 1))),
    ('one_node', 'inf', 1): ((4, 2), (6, 0, (1,))),
    ('one_node', 'inf', 4): ((4, 2), (6, 0, (1, 1, 1, 1))),
}


def refresh_waits(tmp_path):
    """The table that test_refresh_host_waits_pinned pins, measured."""
    import trg_planner
    chain, cut = fg.chain(100), chain_without_last_link(100)
    one = fg.oddities()["one_node"][0]
    pairs = {"chain_cut": (chain, cut), "chain_restored": (cut, chain), "one_node": (one, one)}
    sets = [[0], [10, 50]]
    e = trg_planner.Engine(**MOUNTAIN)
    got = {}
    for name, (a, b) in pairs.items():
        V = len(a.state)
        for scale in ("inf", "4"):
            e.set_option("field_delta_scale", scale)
            for m in (1, 4) + (("sets",) if V > 1 else ()):
                load_graph(e, a, tmp_path, name + "_a")  # a new graph_version: the next solve is the first on it
                if m == "sets":
                    info = e.cost_fields_from(sets)["info"]
                else:
                    info = e.cost_fields(source_ids=[min(k, V - 1) for k in range(m)])["info"]
                load_graph(e, b, tmp_path, name + "_b")
                r = e.refresh_fields(new2old=np.arange(V, dtype=np.int32))
                assert m != "sets" or r["owner"].shape == (2, V)
                got[name, scale, m] = ((info.host_syncs, info.rounds),
                                       (r["info"].host_syncs, r["info"].rounds, tuple(r["carried"].tolist())))
    e.close()
    return got


def test_refresh_host_waits_pinned(tmp_path):
    """The refresh's counterpart of tests/test_gpu_cost_field.py::test_host_waits_pinned: how often a refresh waits
    for the device (the edge costs of the new graph, one wait per 8 jumping sweeps of each of the two anchors and of
    the owner pass, one per batch of 32 rounds in each pass, one for the outputs), how many rounds it runs and how
    many keys it carries are pinned, next to the waits and rounds of the solve before it.  The directed chain of 100
    nodes to the same chain without its last link and back, through the identity map (round counts on a directed
    chain are a function of the graph), and the one-node graph onto a reload of itself; bucket widths inf and 4;
    one field and four from single sources, and two sets of one and two members refreshed with the owners."""
    got = refresh_waits(tmp_path)
    for key in sorted(got, key=repr):
        print(f"    {key!r}: {got[key]!r},")
    assert got == REFRESH_WAITS
