"""Test helper: the protocol of the routes across tiles ("Routes across tiles"), restated in numpy
and plain Python apart from the engine.  Every rank holds what a tiled solve leaves it: its solve graph
(tiled_ref.solve_graph), the keys of its nodes and of its ghosts, the global parents of its nodes.  Exchange 0: the
owner of each target publishes LEN {route, hops or -1, cost bits, owner}; every rank computes the same clipped offsets.
From exchange 1 on each rank walks what stands on its nodes -- the route edge is the tight edge of least index into the
node in the parent's row of ITS solve graph, a ghost's row when the parent is another rank's node -- and publishes
HANDOFF {route, parent gid, sum_dist, sum_w} at a seam or END {route, -1 - root gid, sums} at a root; the loop ends at
the first exchange without news.  reference_routes is the definition (tests/route_ref.py) on the uncut graph.  Test
code only."""
from types import SimpleNamespace

import numpy as np

import route_ref
import tiled_ref as tr
from field_keys import INVALID, cost_values

F32 = np.float32


def reference_routes(G, sf, cost, hops, parent, targets):
    """route_ref's routes of one field of the uncut graph to `targets`; a route starts at the root its parents lead to"""
    g = SimpleNamespace(**G)
    costs = route_ref.edge_costs(g.col, g.w, g.dist, g.state, sf)
    out, memo = [], {}
    for t in targets:
        root = int(t)
        while hops[root] > 0:
            root = int(parent[root])
        with np.errstate(over="ignore"):
            out.append(route_ref.route(g.rowptr, g.col, g.w, g.dist, g.state, sf, cost, hops, parent, root, int(t), costs,
                                       memo))
    return out


def crossings(offsets, route):
    """how often a reference route steps from one range into another"""
    tile = np.searchsorted(offsets, route.ids, side="right") - 1
    return int((tile[1:] != tile[:-1]).sum())


def reenters(offsets, route):
    """does the route leave a range and come back to it?"""
    tile = (np.searchsorted(offsets, route.ids, side="right") - 1).tolist()
    runs = [t for i, t in enumerate(tile) if i == 0 or tile[i - 1] != t]
    return len(set(runs)) < len(runs)


def clipped_offsets(lengths, cap):
    off = np.zeros(len(lengths) + 1, np.int64)
    for r, n in enumerate(lengths):
        off[r + 1] = min(off[r] + n, cap)
    return off


def tiled_routes(G, offsets, sf, cost, hops, parent, targets, owner=None, cap=None):
    """The protocol for the routes of one field (cost, hops, parent: the field of the uncut graph, which a tiled solve
    equals) to the global ids `targets`.  -> dict(offsets, infos: per route (num_nodes, cost, path_length, avg_risk,
    root_gid, owner), parts: per rank the global ids at its own positions and -1 elsewhere, exchanges, records: per
    exchange the (kind, fields) tuples gathered in it)."""
    R = len(offsets) - 1
    ranks = [tr.solve_graph(G, int(offsets[t]), int(offsets[t + 1])) for t in range(R)]
    cost = np.asarray(cost, F32)
    for S in ranks:
        S.ec = cost_values(S.w, S.dist, sf)
        S.ok = S.state[S.col] != INVALID
        S.cost, S.hops = cost[S.gid_of], np.asarray(hops)[S.gid_of]  # the ghosts mirror their owners' keys
        S.index = {int(g): i for i, g in enumerate(S.gid_of)}
    rank_of = lambda g: int(np.searchsorted(offsets, g, side="right") - 1)  # noqa: E731
    n = len(targets)
    # exchange 0: LEN
    gathered = [("LEN", r, int(hops[t]), cost[t] if hops[t] >= 0 else F32(np.inf),
                 -1 if owner is None or hops[t] < 0 else int(owner[t])) for r, t in enumerate(targets)]
    records = [gathered]
    lengths = [rec[2] + 1 for rec in gathered]
    off = clipped_offsets(lengths, sum(lengths) if cap is None else cap)
    infos = [[lengths[r], gathered[r][3], F32(0.0), F32(0.0), -1, gathered[r][4]] for r in range(n)]
    parts = [np.full(int(off[-1]), -1, np.int64) for _ in range(R)]

    def walk(t, r, v, sd, sw):
        S = ranks[t]
        while True:
            h = int(S.hops[v])
            assert h >= 0
            if h < off[r + 1] - off[r]:
                parts[t][off[r] + h] = S.lo + v
            if h == 0:
                return ("END", r, -1 - (S.lo + v), sd, sw)
            p = int(parent[S.lo + v])
            u = S.index[p]  # (a KeyError: a parent that is neither a node nor a ghost of this rank)
            k0, k1 = int(S.rowptr[u]), int(S.rowptr[u + 1])
            with np.errstate(over="ignore"):
                ext = (S.cost[u] + S.ec[k0:k1]).astype(F32)
            hit = (S.col[k0:k1] == v) & S.ok[k0:k1] & (ext.view(np.uint32) == S.cost[v:v + 1].view(np.uint32)) & \
                (S.hops[u] + 1 == h)
            k = k0 + int(np.flatnonzero(hit)[0])
            with np.errstate(over="ignore"):
                sd, sw = F32(sd + S.dist[k]), F32(sw + S.w[k])
            if u >= S.V:
                return ("HANDOFF", r, p, sd, sw)
            v = u

    exchanges = 1
    while True:
        out = []
        if exchanges == 1:
            for r, t in enumerate(targets):
                if hops[t] >= 0:
                    k = rank_of(t)
                    out.append(walk(k, r, int(t) - ranks[k].lo, F32(0.0), F32(0.0)))
        else:
            for kind, r, b, sd, sw in gathered:
                if kind == "HANDOFF":
                    k = rank_of(b)
                    out.append(walk(k, r, b - ranks[k].lo, sd, sw))
                elif kind == "END":
                    infos[r][2], infos[r][3], infos[r][4] = sd, F32(sw / F32(infos[r][0])), -1 - b
        exchanges += 1
        gathered = out
        if not out:
            break
        records.append(out)
    return dict(offsets=off, infos=[tuple(i) for i in infos], parts=parts, exchanges=exchanges, records=records)


def join(got):
    """the ranks' parts -> the routes' global ids; every position claimed exactly once"""
    claims = np.sum([p >= 0 for p in got["parts"]], 0)
    assert (claims == 1).all(), claims
    ids = np.max(got["parts"], 0)
    off = got["offsets"]
    return [ids[off[r]:off[r + 1]] for r in range(len(off) - 1)]
