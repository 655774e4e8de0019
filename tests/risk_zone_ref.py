"""Test helper: keep-out zones on risk fields on the host ("Keep-out zones on risk fields").  The
risk field of a zone set on a graph g is DEFINED as today's risk field on zone_ref.pruned(g, zones): g without the
edges the set closes, in CSR order -- so every reference here is one of the existing ones on the pruned graph: the
compiled Dijkstra on the (risk, hops) key (tests/cpp/risk_reference.cpp through risk_ref), the definition restated
apart from it (risk_ref.py_risk_field), the owner rule (risk_ref.owners), the truncation (bound_ref) and the route walk
(risk_ref.route), whose edge indices are mapped back to g's through Pruned.kept.  Nothing of the engine is read.  Test
code only."""
from collections import namedtuple

import numpy as np

import bound_ref
import risk_ref
import set_ref
import zone_ref as zr

# one field of a set of members: risk / hops / parent / owner per node, owned per member
RiskField = namedtuple("RiskField", "risk hops parent owner owned")


def pruned(g, zones, pos=None):
    """g without the edges that `zones` closes (no ceiling: a risk field has none) -> model_ref.Pruned."""
    return zr.pruned(g, zones, np.inf, pos)


def zoned_field(lib, g, zones, members, pos=None):
    """The risk field of the set `members` under `zones` on g, by the compiled reference -> RiskField."""
    p = pruned(g, zones, pos)
    st, risk, hops, parent = risk_ref.risk_of_graph(lib, p, members)
    assert st == 0, st
    owner, owned = risk_ref.owners(list(members), hops, parent)
    return RiskField(risk, hops, parent, owner, owned)


def definition_field(g, zones, members, pos=None):
    """The same field by the definition (risk_ref.py_risk_field) on the pruned graph -> (risk, hops, parent)."""
    p = pruned(g, zones, pos)
    return risk_ref.py_risk_field(len(p.state), p.rowptr, p.col, p.w, p.state, members)


def truncate(f, bound):
    """f truncated at the ceiling `bound`: bound_ref.truncate, and a truncated node has no owner."""
    risk, hops, parent = bound_ref.truncate(f.risk, f.hops, f.parent, bound)
    owner = np.where(hops >= 0, f.owner, -1).astype(np.int32)
    return RiskField(risk, hops, parent, owner, set_ref.count_owned(owner, len(f.owned)))


def route(g, zones, f, t, pos=None):
    """The route of the field f = zoned_field(.., g, zones, ..) to node t: risk_ref.route on the pruned graph ->
    (ids, the route edges as CSR indices of g, cost = risk[t], path_length, avg_risk)."""
    p = pruned(g, zones, pos)
    ids, edges, cost, length, avg = risk_ref.route(p, f.risk, f.hops, f.parent, t)
    return ids, [int(p.kept[k]) for k in edges], cost, length, avg
