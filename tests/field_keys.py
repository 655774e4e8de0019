"""Test helper: the key algebra every host reference of a field shares, whatever its formulation (DESIGN.md section 2,
"Cost field" and "Risk fields") -- the key words, the fp32 value of an edge under either objective, which edges are
relaxed at all, and how an edge extends a key.  A key is a uint64 word, value bits << 32 | hops, NONE without one;
the objectives differ only in the edge value and in the fold: cost (fl(cost + c), hops + 1) over c = (sf * w + 1) *
dist, risk (max(risk, r), hops + 1) over r = w + 0.  Test code only."""
import numpy as np

F32 = np.float32
INVALID = -1  # a node state: never entered
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys_of(cost, hops):
    """The key words of a field given as cost (float32, +inf where unreached) and hops (-1 where unreached)."""
    bits = np.ascontiguousarray(cost, F32).view(np.uint32).astype(np.uint64)
    k = (bits << np.uint64(32)) | np.asarray(hops).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return np.where(np.asarray(hops) < 0, NONE, k)


def cost_of(key):
    """The upper word of every key as float32, +inf without one."""
    c = (key >> np.uint64(32)).astype(np.uint32).view(F32).copy()
    c[key == NONE] = np.inf
    return c


def hops_of(key):
    return np.where(key == NONE, -1, (key & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)


# ---- edge values: one per CSR edge, every operation rounded to fp32 ---------------------------------------

def cost_values(w, dist, sf):
    """(sf * w + 1) * dist."""
    with np.errstate(over="ignore", invalid="ignore"):
        return ((F32(sf) * np.asarray(w, F32) + F32(1.0)) * np.asarray(dist, F32)).astype(F32)


def risk_values(w):
    """w + 0 (a weight of -0 counts as +0)."""
    return (np.asarray(w, F32) + F32(0.0)).astype(F32)


# ---- which edges are relaxed ------------------------------------------------------------------------------

def relaxable(col, state):
    """Per CSR edge: its column is a node of the graph, and that node is not Invalid."""
    col = np.asarray(col)
    ok = (col >= 0) & (col < len(state))
    ok[ok] = np.asarray(state)[col[ok]] != INVALID
    return ok


def edge_list(g, values):
    """(u, v, value) of the relaxable edges of g (rowptr / col / state), `values` being one per CSR edge."""
    ok = relaxable(g.col, g.state)
    eu = np.repeat(np.arange(len(g.state)), np.diff(np.asarray(g.rowptr)))
    return eu[ok], np.asarray(g.col)[ok].astype(np.int64), values[ok]


# ---- how an edge extends a key ----------------------------------------------------------------------------

def fold_sum(a, c):
    """fl(a + c)."""
    with np.errstate(over="ignore"):
        return (a + c).astype(F32)


def fold_max(a, r):
    """max(a, r); risks are >= +0 and no NaN."""
    return np.where(r > a, r, a).astype(F32)


def _extension(fold):
    def extend(key, c):
        g = fold((key >> np.uint64(32)).astype(np.uint32).view(F32), c)
        return (g.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ((key + np.uint64(1)) & np.uint64(0xFFFFFFFF))
    return extend


extend_sum = _extension(fold_sum)  # (fl(cost + c), hops + 1) of every key (none of them NONE)
extend_max = _extension(fold_max)  # (max(risk, r), hops + 1)
