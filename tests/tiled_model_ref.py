"""Test helper: cost models across tiles on the host ("Cost models across tiles").  The tiled field
of the model (s, tau) on the global stitched graph G is DEFINED as the tiled field at safety factor s on G without the
edges of weight > tau, CSR order kept -- so every reference here is an existing one (tests/model_ref.py's prune, then
tests/seed_ref.py, tests/field_ref.py, tests/bound_ref.py, tests/tiled_route_ref.py) on the pruned global rows; nothing
of the engine is read.  Test code only."""
from types import SimpleNamespace

import numpy as np

import bound_ref
import field_ref
import model_ref
import seed_ref
import tiled_route_ref as trr

F32 = np.float32
INF = F32(np.inf)


def pairs(models, engine_sf):
    """None, a safety factor or (safety factor, ceiling) per field -> [(np.float32 s, np.float32 tau)]"""
    return [model_ref.as_model(one, engine_sf) for one in models]


def pruned(G, tau):
    """the exported global graph (a dict) without the edges of weight > tau; everything else of G stays"""
    p = model_ref.prune(SimpleNamespace(**G), tau)
    return dict(G, rowptr=p.rowptr, col=p.col, w=p.w, dist=p.dist, state=p.state)


def fields(G, models, sets, starts=None, engine_sf=3.0):
    """per field k: the seeded field of sets[k] (start costs starts[k], None: +0 each) under models[k] ->
    [set_ref.SetField]"""
    out = []
    for k, ((s, tau), members) in enumerate(zip(pairs(models, engine_sf), sets)):
        c0 = np.zeros(len(members), F32) if starts is None else np.asarray(starts[k], F32)
        with np.errstate(over="ignore"):
            out.append(seed_ref.seeded_field(SimpleNamespace(**pruned(G, tau)), s, [int(g) for g in members], c0))
    return out


def stacked(fs, names=("cost", "hops", "parent")):
    """[SetField] -> the (m, V) arrays of `names`"""
    return tuple(np.stack([getattr(f, n) for f in fs]) for n in names)


def compiled_fields(lib, G, models, sources, engine_sf=3.0):
    """the compiled cost reference (field_ref) from one source per field on the pruned graphs -> (cost, hops, parent)"""
    out = []
    for (s, tau), src in zip(pairs(models, engine_sf), sources):
        P = pruned(G, tau)
        st, c, h, p = field_ref.field(lib, P["rowptr"], P["col"], P["w"], P["dist"], P["state"], float(s), int(src))
        assert st == 0, st
        out.append((c, h, p))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def truncated(want, budget=None, mode=None, targets=()):
    """(cost, hops, parent) truncated at min(budget, the settle value over `targets`) per field -> (the truncated
    fields, the bounds)"""
    m = want[0].shape[0]
    budget = np.broadcast_to(np.asarray(INF if budget is None else budget, F32).reshape(-1), (m,))
    bound = np.array([min(F32(budget[k]), bound_ref.settle_bound(want[0][k], want[1][k], targets, mode))
                      for k in range(m)], F32)
    return bound_ref.truncate(*want, bound), bound


def routes(G, models, want, route_pairs, engine_sf=3.0):
    """route_ref's routes (through tiled_route_ref.reference_routes) of the (field, target) pairs; want: the (m, V)
    arrays (cost, hops, parent) of the fields under `models`.  Field k's routes are walked on ITS pruned graph at ITS
    safety factor: the route edge is the admitted tight edge of least CSR index."""
    out = [None] * len(route_pairs)
    for k, (s, tau) in enumerate(pairs(models, engine_sf)):
        mine = [i for i, (f, _) in enumerate(route_pairs) if f == k]
        if not mine:
            continue
        P = pruned(G, tau)
        for i, r in zip(mine, trr.reference_routes(P, float(s), want[0][k], want[1][k], want[2][k],
                                                   [route_pairs[i][1] for i in mine])):
            out[i] = r
    return out
