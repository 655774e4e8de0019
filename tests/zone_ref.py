"""Test helper: keep-out zones on the host ("Keep-out zones") -- the rule in numpy float32, one
operation per line as DESIGN.md and the device function have it, giving closed(g, zones) per CSR edge and
inside(g, zones) per node.  The field of (model, zone set) on a graph g is DEFINED as today's field on
pruned(g, zones, tau): g without the edges above the ceiling and without the closed edges, in CSR order -- so every
reference is one of the existing ones (tests/set_ref.py, bound_ref.py, route_ref.py, seed_ref.py, refresh_ref.py) on
the pruned graph.  Nothing of the engine is read.  Test code only."""
import numpy as np

import model_ref
from field_keys import F32

ZONES_MAX = 256  # TRG_ZONES_MAX


def zones_of(zones):
    """None or anything that reads as rows (x, y, r) -> (Z, 3) float32."""
    if zones is None:
        return np.empty((0, 3), F32)
    z = np.asarray(zones, F32)
    return z.reshape(-1, 3) if z.size else np.empty((0, 3), F32)


def positions(g, pos=None):
    """(V, 3) or (V, 2) float32 positions: `pos`, else the graph's own (FieldGraph.pos, CsrGraph.xyz)."""
    if pos is None:
        pos = g.pos if hasattr(g, "pos") else g.xyz
    return np.asarray(pos, F32)


def closes(x, y, r, Px, Py, Qx, Qy):
    """The rule: does the zone (x, y, r), np.float32 scalars, close the edges between P and Q (float32 arrays), P the
    position of the end with the smaller node id.  Every line is one rounded fp32 operation (or two products and their
    sum, each rounded); the comparisons are taken as written, so a NaN closes nothing."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        r2 = r * r
        ax = x - Px
        ay = y - Py
        da = ax * ax + ay * ay
        bx = x - Qx
        by = y - Qy
        db = bx * bx + by * by
        dx = Qx - Px
        dy = Qy - Py
        L2 = dx * dx + dy * dy
        t = ax * dx + ay * dy
        cr = ax * dy - ay * dx
        assert all(v.dtype == F32 for v in (r2, da, db, L2, t, cr))
        return (da <= r2) | (db <= r2) | ((t > 0) & (t < L2) & (cr * cr <= r2 * L2))


def holds(x, y, r, Px, Py):
    """The rule's da <= r2: are the nodes at P inside the zone."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        r2 = r * r
        ax = x - Px
        ay = y - Py
        da = ax * ax + ay * ay
        return da <= r2


def edge_ends(g):
    """(u, v) per CSR edge: its row and its column."""
    V = len(g.state)
    return np.repeat(np.arange(V), np.diff(np.asarray(g.rowptr))), np.asarray(g.col).astype(np.int64)


def closed(g, zones, pos=None):
    """bool per CSR edge of g: some zone closes it.  An edge whose column is no node is never closed."""
    z = zones_of(zones)
    p = positions(g, pos)
    u, v = edge_ends(g)
    ok = (v >= 0) & (v < len(g.state))
    a, b = np.minimum(u, v)[ok], np.maximum(u, v)[ok]
    Px, Py, Qx, Qy = p[a, 0], p[a, 1], p[b, 0], p[b, 1]
    out = np.zeros(len(u), bool)
    hit = np.zeros(int(ok.sum()), bool)
    for x, y, r in z:
        hit |= closes(F32(x), F32(y), F32(r), Px, Py, Qx, Qy)
    out[ok] = hit
    return out


def inside(g, zones, pos=None):
    """bool per node of g: inside some zone."""
    z = zones_of(zones)
    p = positions(g, pos)
    out = np.zeros(len(g.state), bool)
    for x, y, r in z:
        out |= holds(F32(x), F32(y), F32(r), p[:, 0], p[:, 1])
    return out


def pruned(g, zones, tau=np.inf, pos=None):
    """model_ref.prune with the extra mask: g without the edges of weight > tau and without the edges the zone set
    closes, the rest in CSR order -> model_ref.Pruned (`kept`: the CSR index in g of every edge of it)."""
    w = np.asarray(g.w, F32)
    keep = ~(w > F32(tau)) & ~closed(g, zones, pos)
    V = len(g.state)
    eu, _ = edge_ends(g)
    rowptr = np.zeros(V + 1, np.int64)
    np.add.at(rowptr, eu[keep] + 1, 1)
    return model_ref.Pruned(np.cumsum(rowptr).astype(np.int32), np.asarray(g.col)[keep].astype(np.int32), w[keep],
                            np.asarray(g.dist, F32)[keep], np.asarray(g.state).astype(np.int32), np.flatnonzero(keep))


def segment_distance64(cx, cy, Px, Py, Qx, Qy):
    """The float64 distance from the point (cx, cy) to the segments P-Q: what the rule decides `<= r` of."""
    cx, cy, Px, Py, Qx, Qy = (np.asarray(v, np.float64) for v in (cx, cy, Px, Py, Qx, Qy))
    dx, dy = Qx - Px, Qy - Py
    L2 = dx * dx + dy * dy
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(L2 > 0, ((cx - Px) * dx + (cy - Py) * dy) / L2, 0.0)
    s = np.clip(s, 0.0, 1.0)
    return np.hypot(cx - (Px + s * dx), cy - (Py + s * dy))
