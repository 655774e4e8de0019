"""Test helper: the cost field of a source set whose entries have START COSTS, on the host (DESIGN.md section 2,
"Start costs") -- the definition written out apart from the engine, tests/set_ref.with_super_source generalised:

augmented()     g plus one node rho (id V) with, for EVERY entry j of the set, one arc rho -> members[j] of weight 0
                and dist c0[j] + 0, which costs exactly c0[j] under any finite safety factor ((sf * 0 + 1) * c0);
                nothing enters rho;
seeded_field()  the single-source field from rho on that graph -- costs by a Dijkstra on the cost alone, hops as the
                BFS depth of the tight subgraph, parent the smallest tight u one level up -- with the arcs out of rho
                exempt from the Invalid rule (a set member may be Invalid), shifted back: hops - 1, rho reported as
                parent -1, node rho dropped.  A node whose parent is rho is a ROOT; the owner of a root is the least
                entry naming it whose c0 bits are its cost bits, of any other reached node its parent's owner.
The compiled host Dijkstra (tests/cpp/field_reference.cpp) takes the augmented graph as it is wherever no member is
Invalid: tests/test_cost_field_seeded_cpu.py pins this file against it.  Test code only."""
import heapq
from collections import namedtuple

import numpy as np

import set_ref

F32 = np.float32
INVALID = -1

Augmented = namedtuple("Augmented", "rowptr col w dist state")


def start_costs(c0):
    """The start costs as the engine takes them: float32, -0 as +0."""
    return (np.asarray(c0, F32).reshape(-1) + F32(0.0)).astype(F32)


def augmented(g, members, c0, sinks=None):
    """-> Augmented: g, node rho = V with the arcs of the docstring and, with `sinks` = (nodes, costs), one more node
    V + 1 entered by an arc b -> V + 1 of weight 0 and dist d for every pair -- rows stay in CSR order, a node's new
    arc after its own edges."""
    V = len(g.state)
    members = [int(s) for s in members]
    c0 = start_costs(c0)
    assert len(members) == len(c0) and members
    src = np.repeat(np.arange(V), np.diff(np.asarray(g.rowptr))).tolist()
    dst, w, dist = np.asarray(g.col).tolist(), np.asarray(g.w, F32).tolist(), np.asarray(g.dist, F32).tolist()
    n = V + 1
    if sinks is not None:
        for b, d in zip(*sinks):
            src.append(int(b))
            dst.append(V + 1)
            w.append(0.0)
            dist.append(F32(d))
        n = V + 2
    for s, c in zip(members, c0):
        src.append(V)
        dst.append(s)
        w.append(0.0)
        dist.append(c)
    order = np.argsort(np.asarray(src), kind="stable")
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(np.asarray(src), minlength=n), out=rowptr[1:])
    state = np.concatenate([np.asarray(g.state), np.zeros(n - V, np.int64)]).astype(np.int32)
    return Augmented(rowptr, np.asarray(dst, np.int32)[order], np.asarray(w, F32)[order], np.asarray(dist, F32)[order],
                     state)


def rho_field(a, sf, rho):
    """(cost float32, hops, parent int32) of the single-source field from `rho` on the augmented graph `a`, the arcs
    out of rho exempt from the Invalid rule."""
    n = len(a.state)
    rowptr, col = np.asarray(a.rowptr), np.asarray(a.col)
    eu, ec, ok = set_ref._edges(a, sf)
    ok = ok | (eu == rho)
    cost = [None] * n
    cost[rho] = F32(0.0)
    heap = [(0.0, rho)]
    done = [False] * n
    with np.errstate(over="ignore"):
        while heap:
            _, u = heapq.heappop(heap)
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
    with np.errstate(over="ignore"):
        ext = (cost[eu] + ec).astype(F32)
    tight = ok & reached[eu] & (ext.view(np.uint32) == cost[col].view(np.uint32))
    hops = np.full(n, -1, np.int32)
    hops[rho] = 0
    level, depth = [rho], 0
    tk = np.flatnonzero(tight)
    start = np.searchsorted(eu[tk], np.arange(n + 1))
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
    cand = tight & (hops[eu] + 1 == hops[col])
    parent = np.full(n, n, np.int64)
    np.minimum.at(parent, col[cand], eu[cand])
    parent[parent == n] = -1
    return cost, hops, parent.astype(np.int32)


def shift_back(V, members, c0, cost, hops, parent):
    """The field from rho = V over the nodes 0..V-1 as the seeded call reports it -> set_ref.SetField."""
    members = [int(s) for s in members]
    c0 = start_costs(c0)
    cost, hops, parent = cost[:V].copy(), hops[:V].copy(), parent[:V].copy()
    root = parent == V
    assert np.all(hops[root] == 1) and np.all(hops[hops >= 0] >= 1)
    hops = np.where(hops >= 0, hops - 1, -1).astype(np.int32)
    parent[root] = -1
    owner = np.full(V, -1, np.int32)
    for j in range(len(members) - 1, -1, -1):
        s = members[j]
        if root[s] and c0[j:j + 1].view(np.uint32)[0] == cost[s:s + 1].view(np.uint32)[0]:
            owner[s] = j
    assert np.all(owner[root] >= 0)
    for v in np.argsort(hops, kind="stable").tolist():
        if hops[v] >= 0 and not root[v]:
            owner[v] = owner[parent[v]]
    assert np.all((owner >= 0) == (hops >= 0))
    return set_ref.SetField(cost, hops, parent, owner, set_ref.count_owned(owner, len(members)))


def seeded_field(g, sf, members, c0):
    """-> set_ref.SetField of the set `members` with the start costs `c0` on g."""
    V = len(g.state)
    return shift_back(V, members, c0, *rho_field(augmented(g, members, c0), sf, V))


def roots(f):
    """The roots of a seeded field: reached, hops 0."""
    return np.flatnonzero(f.hops == 0)
