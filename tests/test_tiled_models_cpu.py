"""CPU: cost models across tiles ("Cost models across tiles").  The definition -- the model (s, tau)
on G is the field at safety factor s on G without the edges of weight > tau -- against the protocol: tiled_ref.solve on
the pruned graph, cut into ranges, must equal model_ref.model_field on the uncut graph in value bits, hops, global
parents and owners.  This holds the reference to itself before the GPU is held to it.  Also the C and Python surface of
the feature and the wrapper's refusals, which need no device."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import model_ref
import risk_graphs as rg
import tiled_model_ref as tmr
import tiled_ref as tr
from tiled_support import cuts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
# tau at each of the five levels, s in {0, 1, 3}
MODELS = [(F32(3.0), rg.LEVELS[0]), (F32(0.0), rg.LEVELS[1]), (F32(1.0), rg.LEVELS[2]), (F32(3.0), rg.LEVELS[3]),
          (F32(0.0), rg.LEVELS[4])]


def level_graph(rng, V):
    """tiled_ref.symmetric_graph with every weight redrawn from the five levels, one draw per pair"""
    G = tr.symmetric_graph(rng, V)
    rows = np.repeat(np.arange(V), np.diff(G["rowptr"]))
    lo, hi = np.minimum(rows, G["col"]), np.maximum(rows, G["col"])
    _, pair = np.unique(lo * V + hi, return_inverse=True)
    G["w"] = rng.choice(rg.LEVELS, size=int(pair.max()) + 1 if pair.size else 0)[pair].astype(F32)
    return G


def check(G, offsets, members):
    g = SimpleNamespace(**G)
    reached = []
    for s, tau in MODELS:
        with np.errstate(over="ignore"):
            want = model_ref.model_field(g, (s, tau), members)
            P = tmr.pruned(G, tau)
            value, hops, parent, info = tr.solve(P, offsets, tr.cost(s), members, owners=True)
        at = f"V {G['V']} offsets {offsets.tolist()} members {members} model ({s!r}, {tau!r}): "
        assert np.array_equal(value.view(np.uint32), np.asarray(want.cost, F32).view(np.uint32)), at + "value bits"
        assert np.array_equal(hops, want.hops), at + "hops"
        assert np.array_equal(parent, want.parent), at + "parents"
        assert np.array_equal(info["owner"], want.owner), at + "owners"
        reached.append(int((hops >= 0).sum()))
    return reached


@pytest.mark.parametrize("R", [2, 3, 4])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_protocol_on_the_pruned_graph_equals_the_definition(seed, R):
    rng = np.random.default_rng(3100 + 10 * R + seed)
    V = int(rng.integers(40, 201))
    G = level_graph(rng, V)
    offsets = cuts(rng, V, R)
    valid = np.flatnonzero(G["state"] != tr.INVALID)
    members = [int(v) for v in rng.choice(valid, size=3, replace=False)]
    reached = check(G, offsets, members)
    assert reached[-1] > reached[0], reached  # the ceilings bite: the lowest reaches fewer nodes than the highest


def test_protocol_with_a_range_without_nodes():
    rng = np.random.default_rng(3177)
    G = level_graph(rng, 90)
    offsets = cuts(rng, 90, 4, empty=True)
    assert (np.diff(offsets) == 0).any()
    valid = np.flatnonzero(G["state"] != tr.INVALID)
    check(G, offsets, [int(valid[0]), int(valid[-1])])


# ---- the surface ------------------------------------------------------------------------------------------------------
def test_surface():
    """Fails without the feature: the entry, its declaration, the export and the two methods."""
    import trg_planner
    from trg_planner import _engine
    trg_planner.build_library()
    lib = trg_planner.load_library()
    with open(os.path.join(ROOT, "include", "trg_engine.h")) as f:
        header = f.read()
    sym = "trg_engine_tiled_cost_field_models"
    assert sym in _engine.EXPORTS
    assert re.search(r"TrgStatus " + sym + r"\(TrgEngine \*e, int32_t m,\s*const TrgFieldModel \*models,", header)
    assert hasattr(lib, sym)
    bounded = lib.trg_engine_tiled_cost_field_bounded.argtypes
    assert list(getattr(lib, sym).argtypes) == list(bounded[:2]) + [_engine.C.POINTER(_engine.TrgFieldModel)] + list(bounded[2:])
    E = _engine.Engine
    assert list(inspect.signature(E.tiled_cost_fields_models).parameters)[1:] == [
        "sets_or_sources", "models", "start_costs", "budget", "settle", "settle_gids", "targets", "full", "parent"]
    p = inspect.signature(E.tiled_cost_fields_models).parameters
    assert [p[k].default for k in ("start_costs", "budget", "settle", "settle_gids", "targets", "full", "parent")] == \
        [None, None, None, None, None, True, True]
    p = inspect.signature(E.tiled_plan_tradeoff).parameters
    assert list(p)[1:] == ["start_gid", "goal_gid", "models", "early_exit"] and p["early_exit"].default is True
    assert "tiled_safest_routes" in E.tiled_plan_tradeoff.__doc__ and not hasattr(E, "tiled_min_risk_ceiling")
    for doc in ("README.md", "DESIGN.md", os.path.join("include", "trg_engine.h")):
        with open(os.path.join(ROOT, doc)) as f:
            text = re.sub(r"\s*\n( \*)?\s*", " ", f.read())
        assert not re.search(r"[Cc]ost models and (the )?refresh are not offered", text), doc
        assert "Cost models across tiles" in text and re.search(r"[Rr]efresh is not offered across tiles", text), doc


def bare_engine():
    """an Engine object without a device or a handle: what the wrapper refuses, it refuses before any call"""
    from trg_planner import _engine
    e = object.__new__(_engine.Engine)
    e.params = SimpleNamespace(safety_factor=3.0)
    return e


@pytest.mark.parametrize("models, text", [
    ([(np.nan, 0.5), None], "the safety factor of field 0 is negative or not finite"),
    ([None, (-1.0, 0.5)], "the safety factor of field 1 is negative or not finite"),
    ([None, np.inf], "the safety factor of field 1 is negative or not finite"),
    ([(3.0, np.nan), None], "the risk ceiling of field 0 is negative or not a number"),
    ([3.0, (3.0, -0.5)], "the risk ceiling of field 1 is negative or not a number"),
    ([None], "1 models for 2 fields"),
    ([None, None, 1.0], "3 models for 2 fields"),
])
def test_wrapper_refuses_bad_models_without_a_device(models, text):
    e = bare_engine()
    for sets in ([4, 9], [[4, 5], [9]]):
        with pytest.raises(ValueError) as ex:
            e.tiled_cost_fields_models(sets, models)
        assert text in str(ex.value) and "tiled_cost_fields_models" in str(ex.value)
    if len(models) == 2:
        with pytest.raises(ValueError) as ex:
            e.tiled_plan_tradeoff(4, 9, models)
        assert text in str(ex.value)
