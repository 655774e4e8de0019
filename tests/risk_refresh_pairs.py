"""Test helper: pairs of graphs for the tests of the risk-field refresh ("Risk fields") -- the
pairs of tests/refresh_pairs.py that say something under the risk objective, as they are, and pairs of their own: each
an earlier graph A, the current graph B, the node map from B's ids to A's and the sources as ids of A (refresh_pairs.
Pair).  Both the CPU test of tests/risk_refresh_ref.py and the GPU test of the engine take them from here.  Test code
only."""
import numpy as np

import field_graphs as fg
import refresh_pairs as rp
import risk_graphs as rg
from refresh_pairs import Pair

F32 = np.float32

# tests/refresh_pairs.py's pairs under the risk objective; chain_* and star have all-zero weights: the bucket width is
# 0 and only hops change
FROM_COST = ("random", "lattice", "invalid", "chain_cut", "chain_join", "star")
LEVELS_SETS = [[0, 11, 0, 57], [1005, 1009]]


def risk_plateau_pair():
    """In B the added edge 0 -> 4 lowers node 1's risk from 0.3 (one hop) to 0.1 (three hops); node 2's risk 0.5
    absorbs either, and its hops go from 2 to 4, as do the hops of node 3 behind it.  A single warm pass on
    (risk, hops) keeps (0.5, 2) at node 2: no extension of node 1's new key improves it."""
    e = [(0, 1, 0.3, 1.0), (1, 2, 0.5, 1.0), (2, 3, 0.1, 1.0), (4, 5, 0.1, 1.0), (5, 1, 0.1, 1.0), (3, 0, 0.1, 1.0)]
    a = fg.from_edges(6, *zip(*e))
    b = rp.rebuilt(a, extra=[(0, 4, 0.1, 1.0)])
    return Pair(a, b, rp.identity(a), [0, 4, 0])


def levels_pair(seed=7, protect=()):
    """refresh_pairs.random_pair's construction -- 5 % of the nodes deleted, 5 % new ones with edges, weights raised and
    lowered, ids permuted -- on its base graph with every weight first redrawn from risk_graphs.LEVELS: plateaus of
    equal risk several hops wide on both sides of the update.  The third source reaches only itself."""
    rng = np.random.default_rng(seed)
    a = rg.reweighted(fg.random_graph(np.random.default_rng(100), 40, 50), seed)
    V = len(a.state)
    sources = [0, 11, V // 2 + 5]
    keep = np.ones(V, bool)
    gone = rng.choice(V, size=V // 20, replace=False)
    keep[gone] = False
    keep[sources] = True
    keep[list(protect)] = True
    s, d, w, dist = rp.edges_of(a)
    touched = rng.choice(s.shape[0], size=s.shape[0] // 20, replace=False)
    w = w.copy()
    w[touched] = (w[touched] * rng.choice(np.array([0.0, 0.5, 2.0, 4.0], F32), size=touched.shape[0])).astype(F32)
    a2 = rp.rebuilt(a, w=w)
    n_keep, n_new = int(keep.sum()), V // 20
    new_edges = []
    for j in range(n_new):
        for _ in range(3):
            o = int(rng.integers(0, n_keep + n_new))
            wd = (F32(rng.choice([0.0, 0.4])), F32(rng.choice([0.0, 1e-9, 0.45, 150.0])))
            new_edges.append((n_keep + j, o, *wd))
            new_edges.append((o, n_keep + j, *wd))
    b, new2old = rp.renumbered(a2, keep, n_new, new_edges, rng)
    return Pair(a, b, new2old, sources)


PEAK_V = 400
PEAK_EDGE = (PEAK_V - 1) // 2  # the edge PEAK_EDGE -> PEAK_EDGE + 1 of risk_graphs.rise_and_fall(PEAK_V)


def peak_pair(up):
    """The directed chain whose weights rise to a peak and fall again, with the peak edge's weight lowered to the next
    lower weight of the chain, or raised by 0.5: every key behind the peak changes its risk word, none its hops."""
    a = rg.rise_and_fall(PEAK_V)
    w = a.w.copy()
    assert w[PEAK_EDGE] == w.max() and w[PEAK_EDGE - 1] < w[PEAK_EDGE]
    w[PEAK_EDGE] = w[PEAK_EDGE] + F32(0.5) if up else w[PEAK_EDGE - 1]
    return Pair(a, rp.rebuilt(a, w=w), rp.identity(a), [0, 100, 150])


def duplicates_swapped_pair():
    """risk_graphs.cases()["duplicates"] with the weights of the two edges 0 -> 1 exchanged: every key stays, and the
    route edge into node 1 is CSR index 0 (dist 1) where it was index 1 (dist 2)."""
    a, _ = rg.cases()["duplicates"]
    w = a.w.copy()
    assert a.col[0] == a.col[1] == 1 and a.rowptr[1] >= 2
    w[0], w[1] = a.w[1], a.w[0]
    return Pair(a, rp.rebuilt(a, w=w), rp.identity(a), [0, 1, 0])


def risk_sets_pair():
    """Two source sets on the levels pair, one with a member named twice; the members are protected from deletion."""
    p = levels_pair(protect=LEVELS_SETS[0] + LEVELS_SETS[1])
    return Pair(p.a, p.b, p.new2old, [s[0] for s in LEVELS_SETS], sets=LEVELS_SETS)


def bad_b_pair():
    """risk_plateau with one NaN weight in B (the edge 5 -> 1): a risk solve of B refuses the graph."""
    p = risk_plateau_pair()
    w = p.b.w.copy()
    s, d, _, _ = rp.edges_of(p.b)
    w[(s == 5) & (d == 1)] = np.nan
    return Pair(p.a, rp.rebuilt(p.b, w=w), p.new2old, p.sources)


def all_pairs(star=True):
    """name -> Pair, every pair of the risk refresh tests that ends in a solve from single sources."""
    cost = rp.all_pairs()
    out = {name: cost[name] for name in FROM_COST if star or name != "star"}
    out.update({"risk_plateau": risk_plateau_pair(), "levels": levels_pair(), "peak_down": peak_pair(False),
                "peak_up": peak_pair(True), "duplicates_swapped": duplicates_swapped_pair()})
    return out
