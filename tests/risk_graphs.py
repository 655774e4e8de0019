"""Test helper: graphs for the risk field's tests ("Risk fields") -- the random family of
tests/field_graphs.py with its weights redrawn from five values, so that a graph holds plateaus of equal risk several
hops wide, and small hand-written cases, each small enough to read.  Test code only."""
import numpy as np

import field_graphs as fg

LEVELS = np.array([0.1, 0.2, 0.3, 0.4, 0.5], np.float32)


def reweighted(g, seed):
    """g (anything with the FieldGraph members, or the CSR tuple) with every weight redrawn from LEVELS."""
    if not isinstance(g, fg.FieldGraph):
        g = fg.with_positions(g)
    w = np.random.default_rng(1000 + seed).choice(LEVELS, size=len(g.col)).astype(np.float32)
    return g._replace(w=w)


def redrawn(seed):
    """field_graphs.random_small(seed) with w redrawn from {0.1, 0.2, 0.3, 0.4, 0.5} by default_rng(1000 + seed)."""
    return reweighted(fg.random_small(seed), seed)


def plain(seed):
    """field_graphs.random_small(seed) as it is."""
    return fg.with_positions(fg.random_small(seed))


def first_valid(g):
    return int(np.flatnonzero(g.state != fg.INVALID)[0])


def rise_and_fall(V):
    """0 -> 1 -> ... -> V-1, the weights rising to a peak in the middle and falling again: one node per round, and
    from the peak on the risk stays at the peak."""
    a = np.arange(V - 1)
    peak = (V - 1) // 2
    w = (1.0 - np.abs(a - peak) / float(V)).astype(np.float32)
    return fg.from_edges(V, a, a + 1, w, np.ones(V - 1, np.float32))


def all_zero_weights(V, seed=0):
    """A random connected graph whose weights are all 0: every risk is 0, so is the mean and the bucket width."""
    g = fg.all_zero(V, seed)
    return g._replace(w=np.zeros(len(g.col), np.float32), dist=np.ones(len(g.col), np.float32))


def cases():
    """name -> (graph, sources): edges are (source, target, weight, dist)."""
    out = {}
    # a weight of -0 counts as +0: 1 and 2 are at risk +0 (bits 0), and the edge 0 -> 2 of weight +0 ties with it
    e = [(0, 1, -0.0, 1.0), (1, 2, -0.0, 1.0), (0, 2, 0.0, 1.0), (2, 3, 0.3, 1.0), (3, 0, -0.0, 1.0)]
    out["negative_zero"] = (fg.from_edges(4, *zip(*e)), [0, 2])
    # duplicate edges of different weight: only the lower one is tight (0 -> 1: index 1; 1 -> 2: index 2 of row 1,
    # where the first of the two equal ones decides); 2 -> 3 below the plateau: both duplicates are tight
    e = [(0, 1, 0.5, 1.0), (0, 1, 0.2, 2.0), (1, 2, 0.9, 1.0), (1, 2, 0.4, 3.0), (1, 2, 0.4, 5.0), (2, 3, 0.1, 7.0),
         (2, 3, 0.3, 11.0), (3, 0, 0.2, 1.0)]
    out["duplicates"] = (fg.from_edges(4, *zip(*e)), [0, 1])
    # a plateau of equal weights with a cycle of tight edges (1 -> 2 -> 3 -> 1), entered twice, and a cheaper long
    # way round to 5 whose interior is riskier than its end
    e = [(0, 1, 0.3, 1.0), (1, 2, 0.3, 1.0), (2, 3, 0.3, 1.0), (3, 1, 0.3, 1.0), (0, 3, 0.3, 1.0), (3, 4, 0.1, 1.0),
         (4, 5, 0.3, 1.0), (2, 5, 0.5, 1.0), (5, 0, 0.3, 1.0), (0, 6, 0.2, 1.0), (6, 4, 0.4, 1.0)]
    out["plateau_cycle"] = (fg.from_edges(7, *zip(*e)), [0, 2, 6])
    # 3's only way in is through the Invalid node 2 (which a walk may start from, never enter); 4 is isolated
    e = [(0, 1, 0.2, 1.0), (1, 2, 0.1, 1.0), (2, 3, 0.1, 1.0), (3, 0, 0.1, 1.0)]
    out["through_invalid"] = (fg.from_edges(5, *zip(*e), state=[0, 0, fg.INVALID, 1, 0]), [0, 2, 4])
    return out


def bad_weights():
    """name -> graph with one weight that a risk solve refuses (on an edge no walk from node 0 uses)."""
    out = {}
    for name, bad in (("nan", np.nan), ("negative", -1.0), ("inf", np.inf)):
        e = [(0, 1, 0.2, 1.0), (1, 0, 0.1, 1.0), (2, 1, bad, 1.0)]
        out[name] = fg.from_edges(3, *zip(*e))
    return out
