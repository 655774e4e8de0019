"""CPU: the protocol of source sets across tiles (tests/tiled_ref.py: per-rank seeding, two passes, parents as
least global ids, the owner loop with ghost terminals and publish-once) must equal the definition on the UNCUT graph
(seed_ref.seeded_field) in cost bits, hops, parents, owners and owned -- the claim of DESIGN.md section 7, "Source sets
across tiles", pinned before any GPU run.  Also the C and Python surface of the feature."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import seed_ref
import tiled_ref as tr
from tiled_support import cuts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF = 3.0


def member_sets(rng, G):
    """Sets of 1 to 12 members with duplicates and Invalid members; start costs: none, zeros, random, and random with
    some copied from another member's arrival cost (exact ties between a start and a walk)."""
    V = G["V"]
    g = SimpleNamespace(**G)
    invalid = np.flatnonzero(G["state"] == tr.INVALID)
    out = []
    for size, kind in ((1, "none"), (2, "zero"), (5, "random"), (9, "ties"), (12, "ties")):
        mem = rng.integers(0, V, size).tolist()
        if size >= 5:
            mem[1] = mem[0]  # a duplicate
            mem[2] = int(invalid[int(rng.integers(0, len(invalid)))])  # an Invalid member
        if kind == "none":
            c0 = None
        elif kind == "zero":
            c0 = np.zeros(size, np.float32)
        else:
            c0 = rng.uniform(0.0, 2.0, size).astype(np.float32)
            c0[1] = c0[0] + np.float32(0.5)  # the duplicate starts dearer: it never owns
            if kind == "ties":
                with np.errstate(over="ignore"):
                    f = seed_ref.seeded_field(g, SF, mem, c0)
                for j in range(3, size):  # a member reached from elsewhere starts at exactly its arrival cost
                    if f.hops[mem[j]] > 0 and np.isfinite(f.cost[mem[j]]) and j % 2:
                        c0[j] = f.cost[mem[j]]
        out.append((mem, c0))
    return out


def check(G, offsets, mem, c0):
    g = SimpleNamespace(**G)
    with np.errstate(over="ignore"):
        want = seed_ref.seeded_field(g, SF, mem, np.zeros(len(mem), np.float32) if c0 is None else c0)
        got = tr.tiled_set_field(G, offsets, SF, mem, c0)
    at = f"offsets {offsets.tolist()} members {mem}: "
    assert np.array_equal(got["cost"].view(np.uint32), want.cost.view(np.uint32)), at + "cost bits"
    assert np.array_equal(got["hops"], want.hops), at + "hops"
    assert np.array_equal(got["parent"], want.parent), at + "parents"
    assert np.array_equal(got["owner"], want.owner), at + "owners"
    assert np.array_equal(got["owned"].sum(0), want.owned), at + "owned"
    assert sum(got["roots"]) == len(seed_ref.roots(want)), at + "roots"
    return want, got


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("R", [2, 3, 4])
def test_protocol_equals_the_uncut_definition(seed, R):
    rng = np.random.default_rng(2000 * R + seed)
    V = int(rng.integers(40, 301)) if seed else 40
    G = tr.symmetric_graph(rng, V)
    offsets = cuts(rng, V, R, empty=seed % 3 == 1 and R > 2)
    tile_of = np.searchsorted(offsets, np.arange(V), side="right") - 1
    crossing = beaten = late_news = 0
    for mem, c0 in member_sets(rng, G):
        want, got = check(G, offsets, mem, c0)
        has = want.parent >= 0
        crossing += int((tile_of[np.flatnonzero(has)] != tile_of[want.parent[has]]).sum())
        beaten += sum(1 for s in set(mem) if want.hops[s] > 0)
        late_news += sum(got["owner_news"][1:])
    # the preconditions: a parent in another range, a member that is no root, owner news beyond the first exchange
    assert crossing > 0 and beaten > 0 and late_news > 0, (crossing, beaten, late_news)


def test_one_entry_sets_equal_the_single_source_protocol():
    rng = np.random.default_rng(11)
    G = tr.symmetric_graph(rng, 90)
    offsets = np.array([0, 30, 55, 90], np.int64)
    for src in (3, 40, int(np.flatnonzero(G["state"] == tr.INVALID)[0])):
        with np.errstate(over="ignore"):
            cost, hops, parent, info = tr.tiled_field(G, offsets, SF, src)
            got = tr.tiled_set_field(G, offsets, SF, [src])
        assert np.array_equal(got["cost"].view(np.uint32), cost.view(np.uint32))
        assert np.array_equal(got["hops"], hops) and np.array_equal(got["parent"], parent)
        assert got["exchanges"] == info["exchanges"]
        assert np.array_equal(got["owner"], np.where(hops >= 0, 0, -1))


def test_crafted_ties():
    """The issue's tie graph in [4, 4] nodes: a member tied with a walk arriving across the seam stays a root, a dearer
    duplicate never owns, of two equal entries the first owns, a beaten member is an ordinary node."""
    edges = [(0, 1), (1, 4), (4, 5), (5, 6), (6, 2), (2, 3), (6, 7)]
    src = [a for a, b in edges] + [b for a, b in edges]
    dst = [b for a, b in edges] + [a for a, b in edges]
    order = np.lexsort((np.array(dst), np.array(src)))
    V = 8
    G = dict(V=V, rowptr=np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))]).astype(np.int64),
             col=np.array(dst, np.int64)[order], w=np.zeros(len(src), np.float32),
             dist=np.ones(len(src), np.float32), state=np.zeros(V, np.int32))
    mem, c0 = [0, 5, 5, 2, 2, 7], np.array([0, 10, 3, 5, 5, 6.5], np.float32)
    want, got = check(G, np.array([0, 4, 8], np.int64), mem, c0)
    assert want.cost.tolist() == [0, 1, 5, 6, 2, 3, 4, 5] and want.hops.tolist() == [0, 1, 0, 1, 2, 0, 1, 2]
    assert want.owner.tolist() == [0, 0, 3, 3, 0, 2, 2, 2] and want.owned.tolist() == [3, 0, 3, 2, 0, 0]
    assert got["owned"].tolist() == [[2, 0, 0, 2, 0, 0], [1, 0, 3, 0, 0, 0]]


def test_surface():
    """Fails without the feature: the entry, its declaration, the info struct and the Python methods."""
    import trg_planner
    from trg_planner import _engine, tiled
    trg_planner.build_library()
    lib = trg_planner.load_library()
    header = open(os.path.join(ROOT, "include", "trg_engine.h")).read()
    sym = "trg_engine_tiled_cost_field_sets"
    assert hasattr(lib, sym) and sym in _engine.EXPORTS and re.search(r"\b" + sym + r"\s*\(", header), sym
    m = re.search(r"typedef struct TrgTiledSetInfo \{(.*?)\} TrgTiledSetInfo;", header, re.S)
    assert m, "include/trg_engine.h does not define TrgTiledSetInfo"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [decl.split()[-1] for decl in body.split(";") if decl.strip()]
    assert names == [n for n, _ in _engine.TrgTiledSetInfo._fields_]
    assert names == ["exchanges", "owner_exchanges", "rounds", "ghosts", "border_nodes", "roots", "records_sent",
                     "owner_records_sent", "ms_device", "ms_total"]
    assert list(inspect.signature(_engine.Engine.tiled_cost_fields_from).parameters)[1:] == [
        "sets", "start_costs", "targets", "full", "parent"]
    assert list(inspect.signature(_engine.Engine.tiled_assign_frontiers).parameters)[1:] == ["member_gids", "start_costs"]
    assert list(inspect.signature(tiled.merge_frontier_picks).parameters) == ["parts"]
    assert list(inspect.signature(tiled.concat_fields).parameters) == ["parts"]


def test_python_helpers_on_host_parts():
    """concat_fields carries the owners when every part has them; merge_frontier_picks joins the ranks' answers."""
    from trg_planner import tiled
    a = dict(cost=np.zeros((1, 2), np.float32), hops=np.zeros((1, 2), np.int32), parent=np.full((1, 2), -1, np.int32),
             owner=np.array([[0, 1]], np.int32))
    b = dict(a, owner=np.array([[1, 1]], np.int32))
    assert tiled.concat_fields([a, b])["owner"].tolist() == [[0, 1, 1, 1]]
    assert "owner" not in tiled.concat_fields([a, {k: v for k, v in b.items() if k != "owner"}])
    none = np.empty(0, np.int32)
    parts = [[(np.array([7, 3], np.int32), (3, 2.0, 4)), (none, None)],
             [(np.array([5], np.int32), (5, 2.0, 3)), (none, None)],
             [(none, None), (np.array([9], np.int32), (9, 1.0, 1))]]
    got = tiled.merge_frontier_picks(parts)
    assert got[0][0].tolist() == [3, 5, 7] and got[0][1] == (5, 2.0, 3)
    assert got[1][0].tolist() == [9] and got[1][1] == (9, 1.0, 1)
