"""CPU: the refresh across tiles as tests/tiled_refresh_ref.py restates it ("Refresh across tiles")
must equal, on the NEW graph, the fresh protocol (tiled_ref.solve) and the definition on the uncut graph
(field_ref.definition_field) in value bits, hops, parents and owners, and its carried counts must sum to what the
single-engine refresh carries on the uncut graph (refresh_ref.carried_of) -- the exactness claim pinned before any GPU
run.  Also the seam plateau that needs the second anchor, the node map helper, and the surface of the feature."""
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import field_ref
import refresh_ref
import tiled_ref as tr
import tiled_refresh_pairs as tp
import tiled_refresh_ref as rr
from field_keys import F32, edge_list, extend_max, extend_sum, fold_max, fold_sum, keys_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJECTIVES = {"cost0": (tr.cost(0.0), extend_sum, fold_sum, 0.0), "cost3": (tr.cost(3.0), extend_sum, fold_sum, 3.0),
              "risk": (tr.RISK, extend_max, fold_max, None)}


def uncut_edges(G, sf):
    g = SimpleNamespace(rowptr=G["rowptr"], col=G["col"], state=G["state"])
    values = tr.risk_values(G["w"]) if sf is None else tr.cost_values(G["w"], G["dist"], sf)
    return edge_list(g, values)


def check(pair, name, owners=True):
    """every set of the pair as one field: the reference against the fresh protocol, the definition and carried_of"""
    objective, extend, fold, sf = OBJECTIVES[name]
    Ga, off_a = tp.csr(pair.a)
    Gb, off_b = tp.csr(pair.b)
    n2o = np.concatenate([np.where(m >= 0, m + off_a[t], -1) for t, m in enumerate(pair.maps)]).astype(np.int64)
    infos = []
    with np.errstate(over="ignore"):
        for members in pair.sets:
            value, hops, _, _ = tr.solve(Ga, off_a, objective, members)
            got = rr.refresh(Gb, off_b, objective, rr.old_keys_of(value, hops, off_a), off_a, pair.maps, members, owners=owners)
            new = got[3]["members"]
            assert new == tp.new_sets(pair._replace(sets=[members]))[0]
            fresh = tr.solve(Gb, off_b, objective, new, owners=owners)
            definition = field_ref.definition_field(Gb["V"], uncut_edges(Gb, sf), lambda a, c: fold(F32(a), F32(c)), new)
            at = f"{name} members {members}: "
            for other, what in ((fresh, "the fresh protocol"), (definition, "the definition")):
                assert np.array_equal(got[0].view(np.uint32), other[0].view(np.uint32)), at + "value bits, " + what
                assert np.array_equal(got[1], other[1]), at + "hops, " + what
                assert np.array_equal(got[2], other[2]), at + "parents, " + what
            if owners:
                assert np.array_equal(got[3]["owner"], fresh[3]["owner"]), at + "owners"
                assert np.array_equal(got[3]["owned"], fresh[3]["owned"]), at + "owned"
            want = refresh_ref.carried_of(Gb["V"], uncut_edges(Gb, sf), extend, keys_of(value, hops), n2o, new)
            assert sum(got[3]["carried"]) == want, (at, got[3]["carried"], want)
            infos.append(got[3])
    return infos


@pytest.mark.parametrize("name", sorted(OBJECTIVES))
@pytest.mark.parametrize("R", [2, 3, 4])
@pytest.mark.parametrize("seed", [0, 1])
def test_random_tilings_deleted_added_renumbered(seed, R, name):
    V = [40, 120, 200][(seed + R) % 3]
    infos = check(tp.renumbered(seed=10 * R + seed, V=V, R=R, scramble=seed == 1 and R == 3), name)
    assert any(sum(i["carried"]) > 0 for i in infos) and all(len(i["exchanges"]) == 2 for i in infos)


@pytest.mark.parametrize("name", ["cost3", "risk"])
def test_a_range_empty_before_and_a_range_empty_after(name):
    before = tp.renumbered(seed=3, V=90, R=3, empty_before=True)
    assert before.a.sizes[1] == 0 and before.b.sizes[1] == 0
    check(before, name)
    after = tp.renumbered(seed=4, V=90, R=4, empty_after=True)
    assert after.a.sizes[2] > 0 and after.b.sizes[2] == 0
    check(after, name)
    check(tp.renumbered(seed=6, V=60, R=3, forget=True), name)


@pytest.mark.parametrize("name", ["cost0", "cost3"])
def test_crafted_pairs(name):
    for pair in (tp.ring_identity(3), tp.cross_only(), tp.alternating_chain(True), tp.alternating_chain(False),
                 tp.tie_lattice(), tp.saturation(), tp.sets_with_owners()):
        check(pair, name)


def test_crafted_pairs_risk():
    for pair in (tp.tie_lattice(risk=True), tp.sets_with_owners()._replace(b=tp.levels(tp.sets_with_owners().b)),
                 tp.cross_only()):
        check(pair, "risk")


def test_unchanged_graph_publishes_nothing():
    """identity: every key is carried and anchored, each pass ends in its first exchange, no key record travels"""
    for m in (1, 3):
        for info in check(tp.ring_identity(m), "cost3"):
            assert sum(info["carried"]) == 12 and info["exchanges"] == [1, 1] and info["records"] == [0, 0], info


def test_seam_plateau_needs_the_second_anchor():
    """Tile 1's cost bits stay and all its hops rise by 2; pass 1 alone keeps its hops."""
    pair = tp.seam_plateau()
    check(pair, "cost0")
    Ga, off = tp.csr(pair.a)
    Gb, _ = tp.csr(pair.b)
    old = tr.solve(Ga, off, tr.cost(0.0), [0])
    new = tr.solve(Gb, off, tr.cost(0.0), [0])
    assert np.array_equal(old[0][4:].view(np.uint32), new[0][4:].view(np.uint32))
    assert np.array_equal(new[1][4:], old[1][4:] + 2) and np.array_equal(new[1], [0, 3, 1, 2, 4, 5, 6, 7])
    keys = rr.old_keys_of(old[0], old[1], off)
    one = rr.refresh(Gb, off, tr.cost(0.0), keys, off, pair.maps, [0], second_pass=False)
    assert np.array_equal(one[0].view(np.uint32), new[0].view(np.uint32))
    assert np.array_equal(one[1][4:], old[1][4:]) and not np.array_equal(one[1], new[1])
    assert np.array_equal(rr.refresh(Gb, off, tr.cost(0.0), keys, off, pair.maps, [0])[1], new[1])


def test_block_chain_joined_needs_fewer_exchanges_than_fresh():
    pair = tp.block_chain(False)
    Ga, off = tp.csr(pair.a)
    Gb, _ = tp.csr(pair.b)
    old = tr.solve(Ga, off, tr.cost(3.0), [0])
    got = rr.refresh(Gb, off, tr.cost(3.0), rr.old_keys_of(old[0], old[1], off), off, pair.maps, [0])
    fresh = tr.solve(Gb, off, tr.cost(3.0), [0])
    assert np.array_equal(got[1], fresh[1]) and np.array_equal(got[2], fresh[2])
    assert got[3]["carried"] == [500, 400]


# ---- the node map helper under sanitizers -----------------------------------------------------------------------------
def test_node_map_helper_under_sanitizers(tmp_path):
    """trg-planner_amd/csrc/node_map.h, the one composing loop of both node maps, in a stand-alone host program."""
    exe = tmp_path / "node_map_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "trg-planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "node_map_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "node map: ok" in out.stdout, out.stdout + out.stderr


# ---- the surface ------------------------------------------------------------------------------------------------------
def test_surface():
    """Fails without the feature: the entries, their declarations, the exports, the methods and the documents."""
    import trg_planner
    from trg_planner import _engine
    trg_planner.build_library()
    lib = trg_planner.load_library()
    with open(os.path.join(ROOT, "include", "trg_engine.h")) as f:
        header = f.read()
    for sym in ("trg_engine_tiled_cost_field_refresh", "trg_engine_tiled_risk_field_refresh"):
        assert sym in _engine.EXPORTS and hasattr(lib, sym)
        assert re.search(r"TrgStatus " + sym + r"\(TrgEngine \*e, const int32_t \*new2old, int32_t n_map,", header), sym
        assert len(getattr(lib, sym).argtypes) == 16
    assert "typedef struct TrgTiledRefreshInfo" in header
    assert [n for n, _ in _engine.TrgTiledRefreshInfo._fields_][:4] == ["exchanges", "anchor_exchanges", "owner_exchanges", "rounds"]
    E = _engine.Engine
    for method in (E.tiled_refresh_fields, E.tiled_refresh_risk_fields):
        p = inspect.signature(method).parameters
        assert list(p)[1:] == ["new2old", "targets", "full", "parent"]
        assert [p[k].default for k in list(p)[1:]] == [None, None, True, True]
    for doc in ("README.md", "DESIGN.md", os.path.join("include", "trg_engine.h"), os.path.join("scripts", "README.md")):
        with open(os.path.join(ROOT, doc)) as f:
            text = re.sub(r"\s*\n( \*)?\s*", " ", f.read())
        assert "tiled_refresh" in text or "tiled_cost_field_refresh" in text, doc
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "### Refresh across tiles" in f.read()
