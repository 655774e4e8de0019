"""Test helper: the refresh of a retained RISK field on the host ("Risk fields"): the steps of
tests/refresh_ref.py -- carry, anchor, pass 1, anchor again with every changed key cut, pass 2 over the tight edges,
parents -- bound to the extension (max(risk, r), hops + 1) over the edge risks r = w + 0.  In numpy, apart from the
engine and from tests/cpp/risk_reference.cpp.  Test code only."""
from field_keys import NONE, cost_of, edge_list, extend_max, hops_of, keys_of, risk_values  # noqa: F401
from refresh_ref import carried_of, refresh_of

risk_of = cost_of  # (the upper word of a key, +inf without one)


def edge_risks(g):
    """(u, v, risk in fp32) of the relaxable edges."""
    return edge_list(g, risk_values(g.w))


def carried(g, old_key, new2old, sources):
    return carried_of(len(g.state), edge_risks(g), extend_max, old_key, new2old, sources)


def refresh(g, old_key, new2old, sources, second_pass=True):
    """refresh_of on graph g (rowptr / col / w / state) -> (risk, hops, parent, carried)."""
    return refresh_of(len(g.state), edge_risks(g), extend_max, old_key, new2old, sources, second_pass)
