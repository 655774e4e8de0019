"""The risk field's host reference (tests/cpp/risk_reference.cpp, a Dijkstra on the (risk, hops) key) against the
definition restated apart from any Dijkstra (tests/risk_ref.py, py_risk_field: Bellman-Ford on max, BFS over the tight
edges, smallest parent), on the fixtures the GPU tests use; and that those fixtures bite.  No GPU."""
import numpy as np
import pytest

import field_graphs as fg
import risk_graphs as rg
import risk_ref

SEEDS = range(20)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return risk_ref.compile_reference(tmp_path_factory.mktemp("risk_ref"))


def _agree(ref, g, sources, at):
    V = len(g.state)
    st, risk, hops, parent = risk_ref.risk_of_graph(ref, g, sources)
    assert st == 0, at
    pr, ph, pp = risk_ref.py_risk_field(V, g.rowptr, g.col, g.w, g.state, sources)
    assert np.array_equal(risk.view(np.uint32), pr.view(np.uint32)), at
    assert np.array_equal(hops, ph), at
    assert np.array_equal(parent, pp), at
    return risk, hops, parent


def _bfs_depth(g, src):
    """Plain BFS depth over relaxable edges."""
    V = len(g.state)
    depth = np.full(V, -1, np.int32)
    depth[src] = 0
    level = [src]
    while level:
        nxt = []
        for u in level:
            for k in range(g.rowptr[u], g.rowptr[u + 1]):
                v = int(g.col[k])
                if g.state[v] != fg.INVALID and depth[v] < 0:
                    depth[v] = depth[u] + 1
                    nxt.append(v)
        level = nxt
    return depth


@pytest.mark.parametrize("family", ["plain", "redrawn"])
def test_random_small(ref, family):
    for seed in SEEDS:
        g = getattr(rg, family)(seed)
        V = len(g.state)
        invalid = int(np.flatnonzero(g.state == fg.INVALID)[0])
        for src in (rg.first_valid(g), invalid, V - 1, [0, V // 2, V - 1, 0]):
            _agree(ref, g, src, f"{family} seed {seed}, from {src}: ")


def test_structured(ref):
    for name, g, sources in (("lattice", fg.lattice(5, 4), [0, 7]), ("lattice 12x12", fg.lattice(12, 12), [0]),
                             ("star", fg.star(70), [0, 5]), ("stars", fg.star(40, hubs=3), [43, 1]),
                             ("chain", fg.chain(40), [0, 20]), ("symmetric chain", fg.chain(25, symmetric=True), [12]),
                             ("rise and fall", rg.rise_and_fall(60), [0, 40]),
                             ("zero weights", rg.all_zero_weights(30), [0])):
        for src in sources:
            _agree(ref, g, src, f"{name} from {src}: ")
        _agree(ref, g, sources, f"{name} from the set {sources}: ")
    for name, (g, sources) in {**fg.oddities(), **rg.cases()}.items():
        for src in sources:
            _agree(ref, g, src, f"{name} from {src}: ")
        _agree(ref, g, sources, f"{name} from the set {sources}: ")


def test_hand_written_cases(ref):
    """What each hand-written case is there for, read off the reference."""
    c = rg.cases()
    g, _ = c["negative_zero"]
    _, risk, hops, parent = risk_ref.risk_of_graph(ref, g, 0)
    assert risk.view(np.uint32).tolist()[:3] == [0, 0, 0] and hops.tolist() == [0, 1, 1, 2] and parent[2] == 0
    g, _ = c["duplicates"]
    _, risk, hops, parent = risk_ref.risk_of_graph(ref, g, 0)
    assert risk.tolist() == [0.0, np.float32(0.2), np.float32(0.4), np.float32(0.4)] and hops.tolist() == [0, 1, 2, 3]
    g, _ = c["plateau_cycle"]
    _, risk, hops, parent = risk_ref.risk_of_graph(ref, g, 0)
    assert np.all(risk[1:6] == np.float32(0.3)) and risk[6] == np.float32(0.2)
    assert hops.tolist() == [0, 1, 2, 1, 2, 3, 1] and parent.tolist() == [-1, 0, 1, 0, 3, 4, 0]
    g, _ = c["through_invalid"]
    _, risk, hops, parent = risk_ref.risk_of_graph(ref, g, 0)
    assert hops.tolist() == [0, 1, -1, -1, -1] and np.isposinf(risk[2:]).all()
    _, risk, hops, parent = risk_ref.risk_of_graph(ref, g, 2)  # (a walk may start from an Invalid node)
    assert hops.tolist() == [2, 3, 0, 1, -1]
    for name, g in rg.bad_weights().items():
        assert risk_ref.risk_of_graph(ref, g, 0)[0] == risk_ref.BAD_WEIGHT, name
    assert risk_ref.risk_of_graph(ref, c["duplicates"][0], 4)[0] == risk_ref.BAD_SOURCE


def test_fixtures_bite(ref):
    """The redrawn graphs hold several plateaus, and hops that only the tight subgraph explains."""
    several, differ = 0, 0
    for seed in SEEDS:
        g = rg.redrawn(seed)
        src = rg.first_valid(g)
        _, risk, hops, _ = risk_ref.risk_of_graph(ref, g, src)
        several += np.unique(risk[np.isfinite(risk)]).size >= 3
        depth = _bfs_depth(g, src)
        assert np.array_equal(depth >= 0, hops >= 0)
        differ += int(((hops >= 0) & (hops != depth)).sum())
    print(f"{several} of {len(SEEDS)} redrawn graphs with three or more distinct risks; {differ} reached nodes whose "
          "tight-subgraph hops differ from the plain BFS depth")
    assert several >= 15
    assert differ >= 100
