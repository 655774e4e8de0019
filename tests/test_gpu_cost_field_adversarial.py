"""GPU: the cost field on graphs built to break it (tests/field_graphs.py), loaded through load_json into an
engine without a map, at five bucket widths (field_delta_scale 4, 0.5, 1e-6, 1e3, inf: near-far with a split far
pile, one bucket per distinct cost through the threshold bump, and single-bucket Bellman-Ford).  Everything is
compared with the host Dijkstra of tests/cpp/field_reference.cpp on the exported CSR, exactly: cost bits, hops
and parents, no tolerance.  The exported CSR is first compared with what was written, so a later mismatch is the
field's and not the loader's.

Families: the CPU test's random graphs (zero and sub-ulp costs, heavy tails, duplicates, Invalid nodes, two
components; tests/test_field_graphs.py asserts that they have nodes a single pass gets wrong) at V ~ 30, 2 000 and
20 000; chains of 3 000 and 8 000 nodes (one node per round: hundreds of 32-round batches); a star of degree
30 000 (a row of 1 875 sixteen-lane trips that feeds the near queue and the far pile) and one of four hubs that
are expanded in one wave;
200 x 200 lattices of equal costs (massive exact ties); all-zero, subnormal and 60-decade costs; folds that
saturate to +inf (reached, with hops and parent, distinct from unreachable); self-loops, triple duplicates,
-0.0, an Invalid or isolated source, V == 1, E == 0; and one engine that solves a large graph, a small one and
the large one again.

Wall time on an MI355X: 10.8 s for this file, next to 8.2 s for tests/test_gpu_cost_field.py with its full-size
case in the same run (24.8 s before the longest chain went from 20 000 to 8 000 nodes and the graphs of 8 000
nodes and more to three of the five widths and fewer sources; every family still runs all five widths at some
size).  What is left is mostly host work -- the generators, JSON, the reference -- and a chain's launches."""
import numpy as np
import pytest

import field_graphs as fg
import field_ref
from field_support import PARAMS, SCALES, SCALES_LARGE, load_graph, random_large, ref  # noqa: F401 (ref: a fixture)

pytestmark = pytest.mark.gpu
F32 = np.float32
@pytest.fixture(scope="module")
def engine_of():
    """safety_factor -> one engine (no map), shared by the tests of this module: every load_json replaces the
    graph of an engine whose field buffers served another one."""
    import trg_planner
    made = {}

    def get(sf=3.0):
        if sf not in made:
            made[sf] = trg_planner.Engine(safety_factor=sf, **PARAMS)
        return made[sf]

    yield get
    for e in made.values():
        e.close()


def _check_walks(x, sf, src, cost, hops, parent, rng):
    """Independent of the reference: the fp32 left fold along `parent` from the source is cost[v], bit for bit,
    over hops[v] + 1 nodes.  Every node, one step each (v's last edge: the least-cost edge parent[v] -> v extends
    parent's cost to v's and its hops by one -- by induction the whole walk folds to cost[v]); and whole walks,
    node by node, for every reached node of a small graph and a seeded sample of a large one."""
    V = x.V
    u = np.repeat(np.arange(V), np.diff(x.rowptr))
    ec = (F32(sf) * x.w + F32(1.0)) * x.dist
    last = np.flatnonzero((parent[x.col] == u) & (x.state[x.col] != fg.INVALID))
    last = last[np.lexsort((ec[last], x.col[last]))]  # by target, the cheapest first
    v, first = np.unique(x.col[last], return_index=True)
    step = np.full(V, np.inf, np.float32)  # least cost of the edges parent[v] -> v
    step[v] = ec[last[first]]
    reached = hops >= 0
    assert reached[src] and cost[src] == 0 and hops[src] == 0 and parent[src] == -1
    assert np.all(parent[~reached] == -1) and np.all(np.isposinf(cost[~reached]))
    inner = np.flatnonzero(reached & (np.arange(V) != src))
    p = parent[inner]
    assert np.all(p >= 0) and np.all(reached[p]) and np.all(np.isfinite(step[inner]))
    assert np.array_equal(hops[p] + 1, hops[inner])
    with np.errstate(over="ignore"):
        assert np.array_equal((cost[p] + step[inner]).astype(np.float32).view(np.uint32), cost[inner].view(np.uint32))
    for v in (inner if V <= 64 else rng.choice(inner, size=min(6, inner.size), replace=False)):
        walk = [int(v)]
        while walk[-1] != src:
            assert len(walk) <= V
            walk.append(int(parent[walk[-1]]))
        assert len(walk) == hops[v] + 1
        c = F32(0.0)
        with np.errstate(over="ignore"):
            for n in walk[-2::-1]:
                c = F32(c + step[n])
        assert c.view(np.uint32) == cost[v].view(np.uint32), (src, int(v))


def _check_field(ref, e, x, sf, sources, scales=SCALES, seed=0):
    V = x.V
    rng = np.random.default_rng(seed)
    want = {}
    for scale in scales:
        e.set_option("field_delta_scale", scale)
        for src in dict.fromkeys(int(s) for s in sources):
            if src not in want:
                st, rc, rh, rp = field_ref.field_of_graph(ref, x, sf, src)
                assert st == 0
                want[src] = rc, rh, rp
            rc, rh, rp = want[src]
            cost, hops, parent, info = e.cost_field(source_id=src)
            at = f"field_delta_scale {scale}, source {src}: "
            bad = np.flatnonzero(cost.view(np.uint32) != rc.view(np.uint32))
            assert bad.size == 0, at + f"{bad.size} costs differ, first at node {bad[0]}: {cost[bad[0]]!r} != {rc[bad[0]]!r}"
            bad = np.flatnonzero(hops != rh)
            assert bad.size == 0, at + f"{bad.size} hops differ, first at node {bad[0]}: {hops[bad[0]]} != {rh[bad[0]]}"
            bad = np.flatnonzero(parent != rp)
            assert bad.size == 0, at + f"{bad.size} parents differ, first at node {bad[0]}: {parent[bad[0]]} != {rp[bad[0]]}"
            assert info.source == src and info.reached == int((hops >= 0).sum()), at
            assert info.rounds <= 2 * (4 * V + 64), at + f"{info.rounds} rounds"  # the host's cap, over two passes
            _check_walks(x, sf, src, cost, hops, parent, rng)
    return want


def _sources(V, seed, *more):
    """node 0, the last node, a seeded random one, and the family's own (hub, corner, middle)"""
    return [0, V - 1, int(np.random.default_rng(seed).integers(0, V)), *more]


@pytest.mark.parametrize("seed", range(24))
def test_random_small(ref, engine_of, tmp_path, seed):
    sf = [3.0, 0.5, 1.0][seed % 3]
    g = fg.with_positions(fg.random_small(seed))
    e = engine_of(sf)
    x = load_graph(e, g, tmp_path)
    _check_field(ref, e, x, sf, _sources(x.V, seed), seed=seed)


@pytest.mark.parametrize("seed,V,scale", [c for size in sorted(fg.RANDOM_LARGE) for c in fg.RANDOM_LARGE[size]])
def test_random_large(ref, engine_of, tmp_path, seed, V, scale):
    g = random_large(seed, V, scale)
    e = engine_of()
    x = load_graph(e, g, tmp_path)
    if x.V <= 3000:
        _check_field(ref, e, x, 3.0, _sources(x.V, seed, x.V // 4), seed=seed)
    else:
        _check_field(ref, e, x, 3.0, _sources(x.V, seed)[::2], scales=SCALES_LARGE, seed=seed)


@pytest.mark.parametrize("symmetric", [False, True], ids=["directed", "symmetric"])
@pytest.mark.parametrize("V", [3000, 8000])
def test_chain(ref, engine_of, tmp_path, V, symmetric):
    """One node (two, from the middle of a symmetric chain) per round: V rounds a pass, V / 32 batches.  From the
    last node of a directed chain nothing is reachable.  The longest chain runs three of the five widths from two
    sources (the launches of one of its solves cost as much as a whole other family)."""
    g = fg.chain(V, symmetric)
    e = engine_of()
    x = load_graph(e, g, tmp_path)
    if V <= 3000:
        want = _check_field(ref, e, x, 3.0, [0, V - 1, V // 2])
    else:
        want = _check_field(ref, e, x, 3.0, _sources(V, V)[::2], scales=SCALES_LARGE)
    assert int((want[0][1] >= 0).sum()) == V and want[0][1][V - 1] == V - 1
    if V <= 3000 and not symmetric:
        assert int((want[V - 1][1] >= 0).sum()) == 1


@pytest.mark.parametrize("deg,hubs", [(30000, 1), (4096, 4)])
def test_star(ref, engine_of, tmp_path, deg, hubs):
    """A row of 30 000 (four of 1 024, all four in one wave of the round after the root's) whose targets lie on
    both sides of the first threshold; the leaves' edges back make every leaf improve its hub."""
    g = fg.star(deg, hubs)
    e = engine_of()
    x = load_graph(e, g, tmp_path)
    assert x.rowptr[1] - x.rowptr[0] == deg // hubs + (hubs > 1)
    if deg <= 4096:
        _check_field(ref, e, x, 3.0, _sources(x.V, hubs, hubs + deg // 3))
    else:
        _check_field(ref, e, x, 3.0, _sources(x.V, hubs), scales=("4", "0.5", "inf"))


@pytest.mark.parametrize("zero_band", [False, True], ids=["uniform", "zero_band"])
@pytest.mark.parametrize("n", [24, 200])
def test_lattice(ref, engine_of, tmp_path, n, zero_band):
    """Equal costs: every node off the source's row and column has many least walks of equal hops, and the parent
    is the smallest id among them."""
    g = fg.lattice(n, n, zero_band)
    e = engine_of()
    x = load_graph(e, g, tmp_path)
    if n <= 24:
        want = _check_field(ref, e, x, 3.0, _sources(x.V, n, (n // 2) * n + n // 2, n - 1))
    else:
        want = _check_field(ref, e, x, 3.0, [0, x.V - 1, (n // 2) * n + n // 2], scales=SCALES_LARGE)
    rc, rh, rp = want[0]
    if not zero_band:
        ids = np.arange(n * n)
        iy, ix = np.divmod(ids, n)
        assert np.array_equal(rh, ix + iy)
        assert np.array_equal(rp[1:], np.where(iy > 0, ids - n, ids - 1)[1:])  # of (x - 1, y) and (x, y - 1): the row below


@pytest.mark.parametrize("V", [30, 2000])
@pytest.mark.parametrize("family", ["all_zero", "denormal", "heavy_tail"])
def test_cost_ranges(ref, engine_of, tmp_path, family, V):
    """all_zero: the mean cost and so the bucket width are 0, the threshold moves by the one-ulp bump alone;
    denormal: subnormal costs, a subnormal or zero width; heavy_tail: costs over 60 decades."""
    g = getattr(fg, family)(V, seed=V)
    e = engine_of()
    x = load_graph(e, g, tmp_path)
    want = _check_field(ref, e, x, 3.0, _sources(V, V))
    rc, rh, _ = want[0]
    assert np.all(rh >= 0)  # connected
    if family == "all_zero":
        assert not rc.any()
    if family == "denormal":
        assert np.all(rc[1:] > 0) and np.all(rc < F32(1.1754944e-38))


@pytest.mark.parametrize("name", ["saturating_chain", "saturating_branch"])
def test_saturating(ref, engine_of, tmp_path, name):
    """A fold that saturates: a node first reached at +inf is reached, with hops and a parent, and is expanded."""
    g = getattr(fg, name)()
    e = engine_of()
    x = load_graph(e, g, tmp_path)
    want = _check_field(ref, e, x, 3.0, range(x.V))
    rc, rh, rp = want[0]
    if name == "saturating_chain":
        assert rh.tolist() == [0, 1, 2, 3, 4, 5] and rp.tolist() == [-1, 0, 1, 2, 3, 4]
        assert np.isinf(rc[2:]).all() and np.isfinite(rc[:2]).all()
    else:
        assert rh.tolist() == [0, 1, 2, 3, 4, 4, 5, 1, 2, 3, 3, -1, -1]


ODDITIES = fg.oddities()


@pytest.mark.parametrize("name", sorted(ODDITIES))
def test_oddities(ref, engine_of, tmp_path, name):
    g, sources = ODDITIES[name]
    e = engine_of()
    x = load_graph(e, g, tmp_path)
    _check_field(ref, e, x, 3.0, sources)


def test_engine_state_sequence(ref, tmp_path):
    """One engine: a large graph, another bucket width, a much smaller graph with another edge count, the large
    graph again -- the graph_version and column-pointer caches of the edge costs and the reuse of oversized
    buffers.  Every result equals a fresh engine's (and the reference's)."""
    import trg_planner
    big = random_large(*fg.RANDOM_LARGE[2000][0])
    small = fg.with_positions(fg.random_small(5))
    e = trg_planner.Engine(safety_factor=3.0, **PARAMS)

    def solve(eng, x, scale, sources):
        eng.set_option("field_delta_scale", scale)
        return [eng.cost_field(source_id=s)[:3] for s in sources]

    def fresh(g, scale, sources, name):
        f = trg_planner.Engine(safety_factor=3.0, **PARAMS)
        out = solve(f, load_graph(f, g, tmp_path, name), scale, sources)
        f.close()
        return out

    def same(a, b):
        return all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for ra, rb in zip(a, b) for p, q in zip(ra, rb))

    Vb, Vs = len(big.state), len(small.state)
    src_big, src_small = [0, Vb // 4], [0, Vs - 1]
    xb = load_graph(e, big, tmp_path, "big")
    first = solve(e, xb, "4", src_big)
    assert same(first, fresh(big, "4", src_big, "big_fresh"))
    assert same(solve(e, xb, "0.5", src_big), first)
    xs = load_graph(e, small, tmp_path, "small")
    assert xs.E != xb.E and Vs * 40 < Vb
    assert same(solve(e, xs, "0.5", src_small), fresh(small, "0.5", src_small, "small_fresh"))
    _check_field(ref, e, xs, 3.0, src_small)
    xb = load_graph(e, big, tmp_path, "big_again")
    assert same(solve(e, xb, "1e3", src_big), first)
    _check_field(ref, e, xb, 3.0, src_big, scales=("1e3", "4"))
    e.close()
