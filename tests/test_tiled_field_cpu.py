"""CPU: the protocol of the cost field across tiles (tests/tiled_ref.py: solve graphs with ghost mirrors,
publish / merge until no news, two passes, parents as least global ids) must equal the definition on the UNCUT
graph (field_ref.py_field) in cost bits, hops and parents -- the exactness claim of DESIGN.md section 7 and the
pass-2 ghost rule, pinned before any GPU run.  Also the C and Python surface of the feature."""
import inspect
import os
import re

import numpy as np
import pytest

import field_ref
import tiled_ref as tr
from tiled_support import cuts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF = 3.0


def check(G, offsets, sources):
    infos = []
    with np.errstate(over="ignore"):
        for src in sources:
            want = field_ref.py_field(G["V"], G["rowptr"], G["col"], G["w"], G["dist"], G["state"], SF, src)
            cost, hops, parent, info = tr.tiled_field(G, offsets, SF, src)
            at = f"offsets {offsets.tolist()} source {src}: "
            assert np.array_equal(cost.view(np.uint32), want[0].view(np.uint32)), at + "cost bits"
            assert np.array_equal(hops, want[1]), at + "hops"
            assert np.array_equal(parent, want[2]), at + "parents"
            infos.append(info)
    return infos


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("R", [2, 3, 4])
def test_protocol_equals_the_uncut_definition(seed, R):
    rng = np.random.default_rng(1000 * R + seed)
    V = int(rng.integers(40, 301)) if seed else 40
    G = tr.symmetric_graph(rng, V)
    offsets = cuts(rng, V, R, empty=seed % 3 == 1 and R > 2)
    valid = np.flatnonzero(G["state"] != tr.INVALID)
    sources = [int(valid[0]), int(valid[len(valid) // 2]), int(np.flatnonzero(G["state"] == tr.INVALID)[0])]
    infos = check(G, offsets, sources)
    # (some field crossed a seam in both passes: a protocol that never exchanged cannot pass)
    assert sum(infos[0]["ghosts"]) > 0 and max(min(i["exchanges"]) for i in infos) >= 2, infos


def test_a_range_without_nodes_and_a_range_without_cross_edges():
    rng = np.random.default_rng(7)
    V = 120
    G = tr.symmetric_graph(rng, V, blocks=[(50, 80)])
    offsets = np.array([0, 50, 50, 80, V], np.int64)  # rank 1 has no nodes, rank 2 no cross edges
    ranks = [tr.solve_graph(G, int(offsets[t]), int(offsets[t + 1])) for t in range(4)]
    assert ranks[1].V == 0 and ranks[2].G == 0 and ranks[0].G > 0 and ranks[3].G > 0
    valid = np.flatnonzero(G["state"] != tr.INVALID)
    block = valid[(valid >= 50) & (valid < 80)]
    inside = int(block[np.argmax(np.diff(G["rowptr"])[block])])  # the block's node with the most edges
    check(G, offsets, [int(valid[0]), inside, int(valid[-1])])
    with np.errstate(over="ignore"):
        cost, hops, _, _ = tr.tiled_field(G, offsets, SF, inside)
    assert (hops[:50] == -1).all() and (hops[80:] == -1).all() and (hops[50:80] >= 0).sum() > 1


def test_the_second_pass_is_needed_across_a_seam():
    """Two walks into a node behind the seam whose prefix costs differ by less than an ulp of the sum, the dearer
    prefix shorter in hops: one label-correcting pass keeps the stale hops, the protocol does not."""
    # 0 -> 3 directly (cost 1 + 2^-23: dearer, 1 hop) and 0 -> 1 -> 2 -> 3 (cost 1: 3 hops), then 3 -> 4 with a cost of
    # 2^25, whose ulp of 4 swallows the difference: hops[4] is 4, and a pass that saw the direct walk first says 2
    edges = [(0, 3, 1.0000001), (0, 1, 0.25), (1, 2, 0.25), (2, 3, 0.5), (3, 4, 33554432.0), (4, 5, 1.0)]
    src = [a for a, b, _ in edges] + [b for a, b, _ in edges]
    dst = [b for a, b, _ in edges] + [a for a, b, _ in edges]
    d = np.array([c for _, _, c in edges] * 2, np.float32)
    order = np.lexsort((np.array(dst), np.array(src)))
    V = 6
    G = dict(V=V, rowptr=np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))]).astype(np.int64),
             col=np.array(dst, np.int64)[order], w=np.zeros(len(src), np.float32), dist=d[order],
             state=np.zeros(V, np.int32))
    want = field_ref.py_field(V, G["rowptr"], G["col"], G["w"], G["dist"], G["state"], SF, 0)
    one = tr.single_pass_hops(V, G["rowptr"], G["col"], G["w"], G["dist"], G["state"], SF, 0)
    assert one[4] != want[1][4], (one, want[1])  # the precondition: a single pass gets the hops behind the seam wrong
    for offsets in ([0, 4, 6], [0, 3, 4, 6], [0, 1, 6]):
        check(G, np.array(offsets, np.int64), [0])


def test_surface():
    """Fails without the feature: the entries, their declarations and the Python methods."""
    import trg_planner
    from trg_planner import _engine, tiled
    trg_planner.build_library()
    lib = trg_planner.load_library()
    header = open(os.path.join(ROOT, "include", "trg_engine.h")).read()
    for sym in ("trg_engine_tiled_cost_field", "trg_engine_stitch_ids"):
        assert hasattr(lib, sym) and sym in _engine.EXPORTS and re.search(r"\b" + sym + r"\s*\(", header), sym
    m = re.search(r"typedef struct TrgTiledFieldInfo \{(.*?)\} TrgTiledFieldInfo;", header, re.S)
    assert m, "include/trg_engine.h does not define TrgTiledFieldInfo"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [decl.split()[-1] for decl in body.split(";") if decl.strip()]
    assert names == [n for n, _ in _engine.TrgTiledFieldInfo._fields_]
    assert names == ["exchanges", "rounds", "ghosts", "border_nodes", "records_sent", "ms_device", "ms_total"]
    assert list(inspect.signature(_engine.Engine.tiled_cost_fields).parameters)[1:] == ["source_gids", "parent"]
    assert list(inspect.signature(_engine.Engine.global_ids).parameters) == ["self"]
    assert list(inspect.signature(tiled.concat_fields).parameters) == ["parts"]
    assert list(inspect.signature(tiled.field_route).parameters) == ["fields", "k", "target_gid"]


def test_field_route_walks_concatenated_parents():
    from trg_planner import tiled
    rng = np.random.default_rng(3)
    G = tr.symmetric_graph(rng, 60)
    src = int(np.flatnonzero(G["state"] != tr.INVALID)[0])
    with np.errstate(over="ignore"):
        cost, hops, parent, _ = tr.tiled_field(G, np.array([0, 20, 45, 60]), SF, src)
    parts = [dict(cost=cost[None, a:b], hops=hops[None, a:b], parent=parent[None, a:b])
             for a, b in ((0, 20), (20, 45), (45, 60))]
    fields = tiled.concat_fields(parts)
    assert np.array_equal(fields["parent"][0], parent) and fields["cost"].shape == (1, 60)
    for t in range(60):
        route = tiled.field_route(fields, 0, t)
        if hops[t] < 0:
            assert route == []
            continue
        assert route[0] == src and route[-1] == t and len(route) == hops[t] + 1
        assert all(parent[b] == a for a, b in zip(route, route[1:]))
