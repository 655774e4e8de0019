"""CPU: the plain restatement of planSafePath's A* (tests/cpp/plan_reference.cpp) that tests/test_gpu_plan_exact.py
holds the engine to -- pinned to the oracle's planSafePath bit for bit, pinned to the definition of a route's cost
apart from any heap, run over the graph families of tests/plan_graphs.py, and shown to tell the oracle's all-fp32
step cost from one evaluated in double on those families."""
import numpy as np
import pytest

import field_ref
import plan_graphs as pg
import plan_ref

F32 = np.float32
SF = 3.0
U = 2.0 ** -24  # unit roundoff of fp32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return plan_ref.compile_reference(tmp_path_factory.mktemp("plan_ref"))


@pytest.fixture(scope="module")
def field_lib(tmp_path_factory):
    return field_ref.compile_reference(tmp_path_factory.mktemp("field_ref"))


@pytest.fixture(scope="module")
def oracle_runs(oa, synth, lib):
    """Per oracle graph (mountain, indoor: the small clouds of tests/test_oracle_trg.py): the CSR, and for 50 queries
    the oracle's path as node ids, its info floats and the restatement's Plan between the same two nodes.  Odd
    queries lie on node coordinates, even ones anywhere in the graph's bounding box."""
    import os
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "trg_golden.npz"))
    nx, ny, seed = [int(v) for v in gold["m_seed"]]
    m = oa.Oracle(**oa.MOUNTAIN)
    m.set_sampler(7, 0, 16)
    m.set_global_map(synth.mountain_cloud(nx, ny, seed=seed, amplitude=5.0, wavelength=14.0))
    assert m.init_graph([8.0, 8.0, 0.0])
    i = oa.Oracle(**oa.INDOOR)
    i.set_sampler(5, 0, 16)
    i.set_global_map(gold["i_cloud"])
    assert i.init_graph([1.5, 1.5, 0.0])
    out = {}
    for name, o, sf in (("mountain", m, oa.MOUNTAIN["safety_factor"]), ("indoor", i, oa.INDOOR["safety_factor"])):
        g = o.graph(0)
        csr = plan_ref.Csr.of_graph(g)
        lookup = plan_ref.id_of_xyz(g.xyz)
        rng = np.random.default_rng(1)
        lo, hi = g.xyz[:, :2].min(axis=0), g.xyz[:, :2].max(axis=0)
        runs = []
        for q in range(50):
            if q % 2:
                a, b = rng.integers(0, g.V, size=2)
                start, goal = g.xyz[a, :2], g.xyz[b]
            else:
                start, goal = rng.uniform(lo, hi), np.append(rng.uniform(lo, hi), 0.0)
            path, info = o.plan(start, goal)
            assert path.shape[0] > 0, (name, q)
            ids = plan_ref.ids_of_path(lookup, path)
            runs.append((ids, info.copy(), plan_ref.plan(lib, csr, sf, ids[0], ids[-1])))
        out[name] = (g, csr, sf, runs)
        o.close()
    return out


def _info_bits(p):
    return np.array([p.direct_dist, p.path_length, p.avg_risk], np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ["mountain", "indoor"])
def test_restatement_equals_oracle(oracle_runs, name):
    """The oracle's exported rows are its nodes' edge lists in push order, so the restatement on that CSR must
    return the oracle's points and its three info floats, bit for bit, on every query."""
    g, csr, sf, runs = oracle_runs[name]
    assert max(len(ids) for ids, _, _ in runs) > 20  # long routes are among them
    for q, (ids, info, p) in enumerate(runs):
        assert p.status == plan_ref.OK and p.num_points == len(ids), (name, q)
        assert np.array_equal(p.ids, ids), (name, q)
        assert np.array_equal(_info_bits(p), info.view(np.uint32)), (name, q, p, info)


def _assert_near_least(fold, least, n_points, at):
    """A route A* returns costs no less than the least fp32 fold over all walks (a minimum), and no more than that
    times 1 + 2 (n + 4) u: a stored g carries at most n adds and three roundings of its last edge cost, f one more
    add and the store, so A* can prefer a dearer record to a cheaper one only if they lie within (n + 4) u of each
    other, relative, as real numbers; the same once more for what the fold of the chosen route adds in roundings."""
    assert np.isfinite(least), at
    assert fold >= least, (at, fold, least)
    assert float(fold) <= float(least) * (1.0 + 2.0 * (n_points + 4) * U), (at, fold, least)


@pytest.mark.parametrize("name", ["mountain", "indoor"])
def test_oracle_routes_cost_the_least_fold(oracle_runs, field_lib, name):
    """The definition, apart from any heap: the numpy fp32 fold of (sf * w + 1) * dist along each returned route
    (the cheapest a -> b edge at each step) against the least fold over all walks (tests/cpp/field_reference.cpp)."""
    g, csr, sf, runs = oracle_runs[name]
    for q, (ids, _, _) in enumerate(runs):
        st, least, _, _ = field_ref.field(field_lib, g.rowptr, g.col, g.w, g.dist, g.state, sf, ids[0])
        assert st == 0
        _assert_near_least(plan_ref.route_cost(csr, sf, ids), least[ids[-1]], len(ids), (name, q))


@pytest.mark.parametrize("sf", [3.0, 0.1, 0.0])
def test_small_braid_against_every_route(lib, field_lib, sf):
    """K=5, M=2: the fold of every simple route, enumerated.  Its minimum is the least fold the host Dijkstra reports
    (exactly: fl(a + c) is monotone in a, so no walk with a cycle is cheaper), and the restatement's route is one of
    the enumerated ones and costs that minimum within the rounding bound."""
    fam = pg.small_braid()
    g = fam.graph
    csr = plan_ref.Csr.of_field_graph(g)
    for start, goal in (fam.queries[0], fam.queries[0][::-1], (0, 7), (3, 2)):
        routes = pg.all_simple_routes(g, int(start), int(goal))
        assert len(routes) >= 16
        folds = np.array([plan_ref.route_cost(csr, sf, r) for r in routes], np.float32)
        st, least, _, _ = field_ref.field(field_lib, g.rowptr, g.col, g.w, g.dist, g.state, sf, int(start))
        assert st == 0 and folds.min().view(np.uint32) == least[goal].view(np.uint32)
        p = plan_ref.plan(lib, csr, sf, start, goal)
        assert p.status == plan_ref.OK and p.ids.tolist() in routes
        _assert_near_least(plan_ref.route_cost(csr, sf, p.ids), folds.min(), p.num_points, (sf, start, goal))


WITNESS = {"k8m3": 16, "k16m4": 9}


def _differing(lib, fam, sf):
    csr = plan_ref.Csr.of_field_graph(fam.graph)
    n = 0
    for s, g in fam.queries:
        a, b = plan_ref.plan(lib, csr, sf, s, g, widen=0), plan_ref.plan(lib, csr, sf, s, g, widen=1)
        assert a.status == plan_ref.OK and b.status == plan_ref.OK
        n += not np.array_equal(a.ids, b.ids)
    return n


def test_braids_tell_fp32_from_double(lib):
    """The discrimination witness: over the 384 braid queries at safety factor 3, the all-fp32 step cost and the one
    evaluated in double (sf widened, one rounding on the store) return different node sequences on at least 10.
    Measured: 16 of the 256 K=8, M=3 braids and 9 of the 128 K=16, M=4 braids, 25 in all (WITNESS below; the seeds
    are fixed, so the count is too).  At safety factor 0 the step cost is dist, exact either way, and the two must
    differ on none."""
    fams = {name: pg.braids(name) for name in pg.BRAIDS}
    assert sum(len(f.queries) for f in fams.values()) == 384
    assert [len(f.graph.state) for f in fams.values()] == [256 * 8 * 3, 128 * 16 * 4]
    differ = {name: _differing(lib, f, SF) for name, f in fams.items()}
    print("witness:", differ)
    assert sum(differ.values()) >= 10, differ
    assert differ == WITNESS, differ
    for name, f in fams.items():
        assert _differing(lib, f, 0.0) == 0, name


def test_exact_tie_family(lib):
    """Every monotone lattice route ties: the restatement returns one of them, start == goal is one point."""
    fam = pg.exact_ties()
    g = fam.graph
    csr = plan_ref.Csr.of_field_graph(g)
    assert len(fam.queries) >= 20
    for s, t in fam.queries:
        p = plan_ref.plan(lib, csr, SF, s, t)
        manhattan = int(np.abs(g.pos[s] - g.pos[t]).sum())
        assert p.status == plan_ref.OK and p.num_points == manhattan + 1
        assert p.ids[0] == s and p.ids[-1] == t
        assert p.direct_dist == F32(np.sqrt(F32(((g.pos[s] - g.pos[t]) ** 2).sum())))
        assert p.path_length == F32(manhattan)
        w = g.w[g.rowptr[s]]
        assert abs(float(p.avg_risk) - float(w) * manhattan / (manhattan + 1)) <= 1e-6
        if s == t:
            assert p.ids.tolist() == [s] and p.avg_risk == 0 and p.path_length == 0 and p.direct_dist == 0


def test_asymmetric_family_is_what_it_says(lib):
    """The family holds what it was built for, on the routes the restatement takes: steps over parallel edges with
    the dearer one first, steps without a reverse edge (the summary adds nothing there), Invalid nodes that change the
    route, and a cut-off goal that gives NOT_FOUND and no path."""
    fam = pg.asymmetric()
    g = fam.graph
    csr = plan_ref.Csr.of_field_graph(g)
    open_csr = plan_ref.Csr(g.rowptr, g.col, g.w, g.dist, np.zeros_like(g.state), g.pos)
    cost = (F32(SF) * g.w + F32(1.0)) * g.dist
    parallel = no_reverse = detour = found = 0
    for s, t in fam.queries[:-2]:
        p = plan_ref.plan(lib, csr, SF, s, t)
        if p.status != plan_ref.OK:
            continue
        found += 1
        assert (g.state[p.ids] != -1).all()
        detour += not np.array_equal(plan_ref.plan(lib, open_csr, SF, s, t).ids, p.ids)
        length = F32(0.0)
        for a, b in zip(p.ids[:-1], p.ids[1:]):
            ks = np.arange(g.rowptr[a], g.rowptr[a + 1])
            ks = ks[g.col[ks] == b]
            assert ks.size
            parallel += ks.size > 1 and cost[ks[0]] > cost[ks[1]]
        for a, b in zip(p.ids[::-1][1:], p.ids[::-1][:-1]):  # walking back from the goal: child b, parent a
            ks = np.arange(g.rowptr[b], g.rowptr[b + 1])
            ks = ks[g.col[ks] == a]
            no_reverse += ks.size == 0
            if ks.size:
                length = F32(length + g.dist[ks[0]])
        assert p.path_length == length
    assert found >= pg.N_ASYMMETRIC and parallel >= 5 and no_reverse >= 5 and detour >= 5, \
        (found, parallel, no_reverse, detour)
    for s, t in fam.queries[-2:]:
        p = plan_ref.plan(lib, csr, SF, s, t)
        assert p.status == plan_ref.NOT_FOUND and p.num_points == 0 and p.ids.size == 0
        assert p.path_length == 0 and p.avg_risk == 0 and p.direct_dist == F32(5.0)
