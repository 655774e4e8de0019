"""Test helper: bounded cost fields on the host ("Bounded fields").

truncate         the definition: the full field with every node dearer than the bound reported as unreached.
settle_bound     the settle value of one field over a target list: the least ("any") or greatest ("all") full-field
                 cost over the targets, +inf where that value would come from a target without a key.
restricted_field what the device computes, written out without regard to speed and WITHOUT truncate: a Dijkstra
                 on the (cost, hops) key that relaxes only extensions whose cost is within the budget, then the
                 smallest-u parent rule over the keys it found.
Test code only."""
import heapq

import numpy as np

import field_graphs as fg

F32 = np.float32
INF = F32(np.inf)


def truncate(cost, hops, parent, bound):
    """The field(s) (cost, hops, parent), (V,) or (m, V), truncated at `bound`, a cost or one per field -> new
    arrays.  Costs are >= +0 and never NaN, so the float order is the order of their bits; +inf > +inf is false: a
    node reached at a saturated +inf stays under a bound of +inf."""
    cost = np.array(cost, F32)
    hops = np.array(hops, np.int32)
    parent = np.array(parent, np.int32)
    b = np.asarray(bound, F32)
    if cost.ndim == 2:
        b = np.broadcast_to(b.reshape(-1, 1) if b.ndim else b, cost.shape)
    out = (hops >= 0) & (cost > b)
    cost[out] = INF
    hops[out] = -1
    parent[out] = -1
    return cost, hops, parent


def settle_bound(cost_row, hops_row, targets, mode):
    """settle_k of one full field over `targets` (node ids, duplicates allowed); mode None, "any" or "all"."""
    if mode is None:
        return INF
    t = np.asarray(targets, np.int64).reshape(-1)
    keyed = np.asarray(hops_row)[t] >= 0
    c = np.asarray(cost_row, F32)[t]
    if mode == "any":
        return F32(c[keyed].min()) if keyed.any() else INF
    if mode == "all":
        return F32(c.max()) if t.size and keyed.all() else INF
    raise ValueError(mode)


def restricted_field(g, sf, src, budget):
    """(cost, hops, parent) of the budget-restricted Dijkstra on g (rowptr / col / w / dist / state) from src."""
    V = len(g.state)
    ec = fg.edge_costs(g, sf)
    budget = F32(budget)
    NONE = (1 << 64) - 1

    def extend(k, c):
        with np.errstate(over="ignore"):
            a = F32(np.array(k >> 32, np.uint32).view(F32) + c)
        return (int(a.view(np.uint32)) << 32) | ((k + 1) & 0xFFFFFFFF), a

    def relaxable(v):
        return 0 <= v < V and g.state[v] != fg.INVALID

    key = [NONE] * V
    done = [False] * V
    key[src] = 0
    heap = [(0, src)]
    while heap:
        k, u = heapq.heappop(heap)
        if done[u] or k != key[u]:
            continue
        done[u] = True
        for e in range(int(g.rowptr[u]), int(g.rowptr[u + 1])):
            v = int(g.col[e])
            if not relaxable(v):
                continue
            nk, a = extend(k, ec[e])
            if a <= budget and nk < key[v]:
                key[v] = nk
                heapq.heappush(heap, (nk, v))
    parent = np.full(V, -1, np.int32)
    for u in range(V):
        if key[u] == NONE:
            continue
        for e in range(int(g.rowptr[u]), int(g.rowptr[u + 1])):
            v = int(g.col[e])
            if relaxable(v) and extend(key[u], ec[e])[0] == key[v] and (parent[v] < 0 or u < parent[v]):
                parent[v] = u
    cost = np.full(V, INF, F32)
    hops = np.full(V, -1, np.int32)
    for v in range(V):
        if key[v] != NONE:
            cost[v] = np.array(key[v] >> 32, np.uint32).view(F32)
            hops[v] = key[v] & 0xFFFFFFFF
    return cost, hops, parent


def five_budgets(cost, hops):
    """The budgets every bounded check runs one full field at: 0, +inf, the median cost of the reached nodes, the
    float just below it (0 where the median is 0: no budget is negative) and the largest cost."""
    c = np.sort(np.asarray(cost, F32)[np.asarray(hops) >= 0])
    med = F32(c[c.size // 2])
    below = F32(np.nextafter(med, F32(-np.inf))) if med > 0 else F32(0.0)
    return [F32(0.0), INF, med, below, F32(c[-1])]
