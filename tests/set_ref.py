"""Test helper: the cost field of a source SET on the host ("Source sets"), the definitions
written out apart from the engine and from tests/cpp/field_reference.cpp:

cost    the least fp32 left fold over all walks from any member (a Dijkstra on the cost alone: fl(a + c) is monotone
        in a and never below a); walks never enter an Invalid node, every member costs +0;
hops    the BFS depth in the tight subgraph (edges with fl(cost[u] + c) == cost[v]) from all members at depth 0;
parent  the smallest u with a tight edge u -> v and hops[u] + 1 == hops[v]; none for a member or an unreached node;
owner   for a member the least index into the set that names it, for any other reached node owner[parent[v]];
owned   nodes per index of the set.
truncate() is tests/bound_ref.py's with owner -1 and `owned` recounted.  Test code only."""
import heapq
from collections import namedtuple

import numpy as np

import bound_ref
from field_keys import F32, INVALID, cost_values, relaxable  # noqa: F401

# cost float32, hops / parent / owner int32 over the nodes; owned int32 over the set's entries
SetField = namedtuple("SetField", "cost hops parent owner owned")


def _edges(g, sf):
    """(source node, cost in fp32, relaxable) per CSR edge."""
    eu = np.repeat(np.arange(len(g.state)), np.diff(np.asarray(g.rowptr)))
    return eu, cost_values(g.w, g.dist, sf), relaxable(g.col, g.state)


def owners_of(members, hops, parent):
    """The owner rule, for either objective: a member's owner is the least index into `members` that names it, any
    other reached node's is its parent's (taken along the parents in the order of the depths), an unreached node's
    -1."""
    owner = np.full(len(hops), -1, np.int32)
    for j in range(len(members) - 1, -1, -1):
        owner[members[j]] = j
    for v in np.argsort(hops, kind="stable").tolist():
        if hops[v] > 0:
            owner[v] = owner[parent[v]]
    return owner


def set_field(g, sf, members):
    """-> SetField of the set `members` (node ids, duplicates and Invalid nodes allowed) on g (rowptr / col / w /
    dist / state)."""
    members = [int(s) for s in members]
    assert members
    V = len(g.state)
    rowptr, col = np.asarray(g.rowptr), np.asarray(g.col)
    eu, ec, ok = _edges(g, sf)
    # costs
    cost = [None] * V
    heap = []
    for s in dict.fromkeys(members):
        cost[s] = F32(0.0)
        heap.append((0.0, s))
    heapq.heapify(heap)
    done = [False] * V
    with np.errstate(over="ignore"):
        while heap:
            a, u = heapq.heappop(heap)
            if done[u]:
                continue
            done[u] = True
            for k in range(int(rowptr[u]), int(rowptr[u + 1])):
                if not ok[k]:
                    continue
                v = int(col[k])
                b = F32(cost[u] + ec[k])
                if cost[v] is None or b < cost[v]:
                    cost[v] = b
                    heapq.heappush(heap, (float(b), v))
    reached = np.array([c is not None for c in cost])
    cost = np.array([np.inf if c is None else c for c in cost], F32)
    # tight edges, BFS depths from all members
    with np.errstate(over="ignore"):
        ext = (cost[eu] + ec).astype(F32)
    colc = np.where(ok, col, 0)
    tight = ok & reached[eu] & (ext.view(np.uint32) == cost[colc].view(np.uint32))
    hops = np.full(V, -1, np.int32)
    level = sorted(set(members))
    hops[level] = 0
    tk = np.flatnonzero(tight)
    start = np.searchsorted(eu[tk], np.arange(V + 1))  # (eu is ascending: the tight edges of row u)
    depth = 0
    while level:
        depth += 1
        nxt = []
        for u in level:
            for v in col[tk[start[u]:start[u + 1]]].tolist():
                if hops[v] < 0:
                    hops[v] = depth
                    nxt.append(v)
        level = nxt
    assert np.array_equal(hops >= 0, reached)
    # parents, then owners along them in the order of the depths
    cand = tight & (hops[eu] + 1 == hops[colc])
    parent = np.full(V, V, np.int64)
    np.minimum.at(parent, col[cand], eu[cand])
    parent[parent == V] = -1
    parent = parent.astype(np.int32)
    owner = owners_of(members, hops, parent)
    assert np.all((owner >= 0) == reached)
    return SetField(cost, hops, parent, owner, count_owned(owner, len(members)))


def count_owned(owner, n):
    return np.bincount(owner[owner >= 0], minlength=n).astype(np.int32)


def truncate(f, bound):
    """The set field f truncated at `bound`: bound_ref.truncate, and a truncated node has no owner."""
    cost, hops, parent = bound_ref.truncate(f.cost, f.hops, f.parent, bound)
    owner = np.where(hops >= 0, f.owner, -1).astype(np.int32)
    return SetField(cost, hops, parent, owner, count_owned(owner, len(f.owned)))


def with_super_source(g, members):
    """g plus one node z (id V) with an edge z -> s of weight 0 and dist 0 for each distinct non-Invalid member s
    -> (rowptr, col, w, dist, state).  The single-source field from z has the set field's cost bits, its hops + 1
    and its parents, except that every member's parent is z."""
    V = len(g.state)
    to = [s for s in dict.fromkeys(int(s) for s in members) if g.state[s] != INVALID]
    rowptr = np.append(np.asarray(g.rowptr), g.rowptr[-1] + len(to)).astype(np.int32)
    col = np.concatenate([np.asarray(g.col), np.array(to, np.int32)]).astype(np.int32)
    w = np.concatenate([np.asarray(g.w, F32), np.zeros(len(to), F32)])
    dist = np.concatenate([np.asarray(g.dist, F32), np.zeros(len(to), F32)])
    state = np.append(np.asarray(g.state), 0).astype(np.int32)
    return rowptr, col, w, dist, state
