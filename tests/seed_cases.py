"""Test helper: the graphs, sets and start costs that the CPU and the GPU test of seeded cost fields (DESIGN.md
section 2, "Start costs") share -- name -> (graph, sets, start costs), sets[k] a list of node ids, costs[k] a float32
array of that length.  Graphs of 30..44 nodes from tests/field_graphs.py, except where a case says otherwise.
Test code only."""
import functools

import numpy as np

import field_graphs as fg

F32 = np.float32
SF = 3.0
SMALL_SEEDS = tuple(s for s in range(1, 80) if 30 <= int(np.random.default_rng(s).integers(8, 48)) <= 44)[:4]


@functools.lru_cache(maxsize=None)
def small(i):
    """The i-th random_small graph with 30..44 nodes."""
    return fg.with_positions(fg.random_small(SMALL_SEEDS[i]))


def first_component(g):
    """The valid nodes of the component of the low ids (ids >= V // 2 + 3 only link among themselves)."""
    V = len(g.state)
    return [v for v in range(V // 2 + 3) if g.state[v] != fg.INVALID]


def typical_cost(g):
    c = fg.edge_costs(g, SF)[g.state[g.col] != fg.INVALID]
    return float(np.median(c[c > 0]))


def random_sets(g, seed, m, entries=5):
    """m sets of `entries` entries over ALL nodes (both components, Invalid ones included; duplicates may occur), start
    costs 0 for some entries and up to four typical edge costs for the others."""
    rng = np.random.default_rng(seed)
    V = len(g.state)
    scale = typical_cost(g)
    sets, costs = [], []
    valid = np.flatnonzero(g.state != fg.INVALID)
    for k in range(m):  # (every third set may name Invalid nodes; the others are what the compiled reference takes)
        sets.append([int(v) for v in (rng.integers(0, V, size=entries) if k % 3 == 2 else rng.choice(valid, entries))])
        c = rng.uniform(0.0, 4.0 * scale, size=entries)
        c[rng.random(entries) < 0.25] = 0.0
        costs.append(c.astype(F32))
    return sets, costs


def unit_chain(V):
    """0 <-> 1 <-> ... <-> V-1, weight 0 and dist 1: every edge costs exactly 1 under any safety factor."""
    a = np.arange(V - 1)
    return fg.from_edges(V, np.stack([a, a + 1], axis=1), np.stack([a + 1, a], axis=1), np.zeros(2 * (V - 1)),
                         np.ones(2 * (V - 1)))


def duplicates():
    """Node a named three times with different start costs (the least twice: the earlier of those entries owns), node b
    twice with equal ones (the first owns), and an Invalid member."""
    g = small(0)
    comp = first_component(g)
    a, b = comp[0], comp[-1]
    inv = int(np.flatnonzero(g.state == fg.INVALID)[0])
    t = F32(typical_cost(g))
    c0 = np.array([t, t / 2, t / 4, t / 2, 8 * t, t / 4], F32)
    return g, [[a, b, a, b, inv, a], [a, b, a, b, a]], [c0, np.delete(c0, 4)]  # (the second: no Invalid member)


def exact_tie():
    """Node 0 at +0, unit edges, node 1 at 1.0: the walk 0 -> 1 costs exactly node 1's start cost and does not beat
    it; node 5 at 7.0 loses to the walk's 5.0 and is demoted."""
    return unit_chain(32), [[0, 1, 5]], [np.array([0.0, 1.0, 7.0], F32)]


def absorption():
    """Start costs of 2^25 beside unit edges: fl(2^25 + 1) == 2^25, so every node costs 2^25 and only the hops and the
    member marks tell roots from walks (node 9 is a root at hops 0 between nodes reached at 8 and 10 hops)."""
    big = F32(2.0 ** 25)
    return unit_chain(32), [[0, 9, 31]], [np.array([big, big, big + F32(4.0)], F32)]


def saturating():
    """saturating_chain() (every edge 2e38) entered at 1e38: 3e38 is finite, the next fold is +inf."""
    return fg.saturating_chain(), [[0, 4]], [np.array([1e38, 3e38], F32)]


def batch_64():
    g = small(1)
    return (g, *random_sets(g, 64, 64, entries=4))


def two_ends():
    """A 5 000-node chain entered at both ends, each with a handicap: the owner pass jumps over thousands of hops."""
    return fg.chain(5000, symmetric=True), [[0, 4999]], [np.array([1000.0, 250000.0], F32)]


CASES = {
    **{f"random_{i}": (lambda i=i: (small(i), *random_sets(small(i), 10 + i, 3))) for i in range(len(SMALL_SEEDS))},
    "duplicates": duplicates,
    "exact_tie": exact_tie,
    "absorption": absorption,
    "saturating": saturating,
    "batch_64": batch_64,
    "two_ends": two_ends,
}
