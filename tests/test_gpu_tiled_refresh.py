"""GPU: the refresh across tiles (trg_engine_tiled_cost_field_refresh / trg_engine_tiled_risk_field_refresh; DESIGN.md
section 7, "Refresh across tiles") over the in-process transport: one process, one engine and one thread per rank, all
on one device.  A tiled solve on tiling A, every tile's graph replaced or updated, a new stitch on the live group, then
the refresh: every rank's value bits, hops, global parents, owners and owned must equal the protocol reference
(tests/tiled_ref.py) and the compiled host references on the rows the engines export, and a fresh tiled solve from
set_gids_out; the carried counts must sum to the single-engine definition's (refresh_ref.carried_of) on the uncut graph.
The pairs are tests/tiled_refresh_pairs.py's."""
from types import SimpleNamespace

import numpy as np
import pytest

import field_graphs as fg
import refresh_ref
import tiled_ref as tr
import tiled_refresh_pairs as tp
from field_keys import edge_list, extend_max, extend_sum, keys_of
from field_support import MOUNTAIN
from tiled_support import (JOIN_SECONDS, assert_fields, call_routes, close, cost_ref, craft, exported, join_group, ok,  # noqa: F401
                           reference, risk_reference, run_ranks, stitch)
from tiled_support import risk_reference_lib, tiled  # noqa: F401  (fixtures: `ref` is the compiled risk reference)

pytestmark = pytest.mark.gpu
INVALID_ARG, DEVICE = 1, 4
SF = MOUNTAIN["safety_factor"]
F32 = np.float32


# ---- the harness ------------------------------------------------------------------------------------------------------
def retile(engines, tmp_path, b, tag):
    """Tiling b on the engines of a live group: every tile's graph through load_json, the cross edges through
    stitch_assemble (tiled_support.craft's steps, on engines that already hold a tiling and a retained solve)."""
    import torch
    off = tp.offsets(b).astype(np.int32)
    V = int(off[-1])
    tile_of = np.searchsorted(off, np.arange(V), side="right") - 1
    x = [(p, q, w, d) if tile_of[p] < tile_of[q] else (q, p, w, d) for p, q, w, d in b.edges if tile_of[p] != tile_of[q]]
    rec = np.array([(tile_of[p], p - off[tile_of[p]], tile_of[q], q - off[tile_of[q]]) for p, q, _, _ in x],
                   np.int32).reshape(-1, 4)
    wd = np.array([(w, d) for _, _, w, d in x], F32).reshape(-1, 2)
    cross = np.ascontiguousarray(np.concatenate([rec, wd.view(np.int32)], 1))
    cross_t = torch.from_numpy(cross).to(torch.device("cuda", torch.cuda.current_device())) if cross.shape[0] else None
    torch.cuda.synchronize()
    for t, e in enumerate(engines):
        own = [(p - off[t], q - off[t], w, d) for p, q, w, d in b.edges if tile_of[p] == t and tile_of[q] == t]
        src = [p for p, q, _, _ in own] + [q for p, q, _, _ in own]
        dst = [q for p, q, _, _ in own] + [p for p, q, _, _ in own]
        g = fg.from_edges(b.sizes[t], np.array(src, np.int64), np.array(dst, np.int64), [w for _, _, w, _ in own] * 2,
                          [d for _, _, _, d in own] * 2, state=b.state[off[t]:off[t + 1]])
        fg.write_json(tmp_path / f"{tag}{t}.json", g)
        e.load_json(str(tmp_path / f"{tag}{t}.json"))
        e.stitch_assemble(t, len(engines), off, cross_t.data_ptr() if cross_t is not None else None, int(cross.shape[0]))
    torch.cuda.synchronize()


def solve_a(engines, sets, risk, owners, targets=None):
    """the retained solve: the set call (owners) or the single-source call over the sets' first members"""
    if owners:
        if risk:
            call = lambda r, e: e.tiled_risk_fields_from(sets, targets=None if targets is None else targets[r])  # noqa: E731
        else:
            call = lambda r, e: e.tiled_cost_fields_from(sets, targets=None if targets is None else targets[r])  # noqa: E731
    else:
        assert all(len(s) == 1 for s in sets)
        src = [s[0] for s in sets]
        call = (lambda r, e: e.tiled_risk_fields(src)) if risk else (lambda r, e: e.tiled_cost_fields(src))
    return ok(run_ranks(engines, call)[0])


def refresh(engines, maps, risk, targets=None):
    def call(r, e):
        f = e.tiled_refresh_risk_fields if risk else e.tiled_refresh_fields
        return f(None if maps is None else maps[r], targets=None if targets is None else targets[r])
    return run_ranks(engines, call)


def uncut_edges(G, risk):
    g = SimpleNamespace(rowptr=G["rowptr"], col=G["col"], state=G["state"])
    return edge_list(g, tr.risk_values(G["w"]) if risk else tr.cost_values(G["w"], G["dist"], SF))


def check(at, tiled, libs, engines, got, risk, owners, old=None, off_a=None, maps=None, targets=None, fresh=True):
    """The ranks' refreshed dicts against the references on the exported rows; then (fresh) against a fresh tiled solve
    from set_gids, which replaces the retained solve.  old: the concatenated fields of the retained solve on A, for the
    carried counts.  -> (G, the protocol reference per field)"""
    name = "risk" if risk else "cost"
    G = exported(tiled, engines)
    sets = [s.tolist() for s in got[0]["set_gids"]]
    for g in got:
        assert [s.tolist() for s in g["set_gids"]] == sets, at
        assert (g["info"].m, g["info"].owners) == (len(sets), int(owners)), at
    with np.errstate(over="ignore"):
        want = [tr.solve(G, G["offsets"], tr.RISK if risk else tr.cost(SF), s, owners=True) for s in sets]
    fields = [np.stack([w[i] for w in want]) for i in range(3)] + [np.stack([w[3]["owner"] for w in want])]
    names = (name, "hops", "parent", "owner")
    assert_fields(at + " protocol", got, G, fields if owners else fields[:3], names if owners else names[:3])
    if risk:
        assert_fields(at + " compiled", got, G, risk_reference(libs["risk"], G, sets), names[:3])
    elif all(len(set(s)) == 1 for s in sets):
        assert_fields(at + " compiled", got, G, reference(libs["cost"], G, [s[0] for s in sets]), names[:3])
    if owners:
        for t, g in enumerate(got):
            for k, w in enumerate(want):
                assert np.array_equal(g["owned"][k], w[3]["owned"][t]), (at, t, k, g["owned"][k], w[3]["owned"][t])
    if old is not None:
        n2o = np.concatenate([np.where(np.asarray(m) >= 0, np.asarray(m) + off_a[t], -1) for t, m in enumerate(maps)])
        for k, s in enumerate(sets):
            carried = refresh_ref.carried_of(G["V"], uncut_edges(G, risk), extend_max if risk else extend_sum,
                                             keys_of(old[name][k], old["hops"][k]), n2o.astype(np.int64), s)
            assert sum(int(g["carried"][k]) for g in got) == carried, (at, k, [g["carried"] for g in got], carried)
    if fresh:
        again = solve_a(engines, sets, risk, owners, targets)
        for t, (g, f) in enumerate(zip(got, again)):
            for key in [name, "hops", "parent"] + (["owner"] if owners else []) + \
                    ([name + "_at", "hops_at", "owner_at"] if owners and targets is not None else []):
                x, y = np.asarray(g[key]), np.asarray(f[key])
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (at, "fresh", t, key)
            if owners:
                assert all(np.array_equal(x, y) for x, y in zip(g["owned"], f["owned"])), (at, "fresh owned", t)
                assert g["info"].roots == f["info"].roots, (at, "roots", t)
    return G, want


def run_pair(tmp_path, tiled, libs, pair, tag, risk=False, owners=False, targets=None, fresh=True, keep=False):
    """solve on pair.a, pair.b on the live group, refresh, check -> (engines, the ranks' dicts, G, the solve's dicts)"""
    engines, _ = craft(tmp_path, pair.a.sizes, pair.a.edges, state=pair.a.state, tag=tag + "-a")
    before = solve_a(engines, pair.sets, risk, owners, targets)
    old = tiled.concat_fields(before)
    retile(engines, tmp_path, pair.b, tag + "-b")
    got, secs = refresh(engines, pair.maps, risk, targets)
    got = ok(got)
    assert [[s.tolist() for s in g["set_gids"]] for g in got] == [tp.new_sets(pair)] * len(engines), tag
    G, _ = check(tag, tiled, libs, engines, got, risk, owners, old, tp.offsets(pair.a), pair.maps, targets, fresh)
    infos = [g["info"] for g in got]
    print(tag, "refresh: exchanges", infos[0].exchanges, "anchor", infos[0].anchor_exchanges, "owner", infos[0].owner_exchanges,
          "rounds", [i.rounds for i in infos], "records", [i.records_sent for i in infos], "anchor records",
          [i.anchor_records_sent for i in infos], "carried", [g["carried"].tolist() for g in got],
          "| solve: exchanges", before[0]["info"].exchanges, "rounds", [b["info"].rounds for b in before], f"{secs * 1e3:.1f} ms")
    if not keep:
        close(engines)
    return engines, got, G, before


@pytest.fixture(scope="module")
def libs(ref, cost_ref):  # noqa: F811
    return {"risk": ref, "cost": cost_ref}


# ---- the cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3])
def test_identity(tmp_path, tiled, libs, m):  # noqa: F811
    """RING in [6, 6], stitched again unchanged: 0 rounds, no key record in the passes, each pass ends in its first
    exchange, and everything reached is carried."""
    _, got, G, before = run_pair(tmp_path, tiled, libs, tp.ring_identity(m), f"identity{m}")
    for t, g in enumerate(got):
        i = g["info"]
        assert (i.rounds, i.records_sent, i.exchanges) == (0, 0, 2), (t, i.rounds, i.records_sent, i.exchanges)
        assert g["carried"].tolist() == (g["hops"] >= 0).sum(1).tolist() == [6] * m


def test_seam_plateau(tmp_path, tiled, libs):  # noqa: F811
    """Tile 1's graph, the seam record and its cost bits stay; all its hops rise by 2 (pass 1 alone would keep them:
    tests/test_tiled_refresh_cpu.py)."""
    _, got, G, before = run_pair(tmp_path, tiled, libs, tp.seam_plateau(), "plateau")
    assert np.array_equal(got[1]["cost"].view(np.uint32), before[1]["cost"].view(np.uint32))
    assert np.array_equal(got[1]["hops"], before[1]["hops"] + 2)
    assert got[0]["hops"].tolist() == [[0, 3, 1, 2]] and got[1]["hops"].tolist() == [[4, 5, 6, 7]]


def test_block_chain_cut_and_joined(tmp_path, tiled, libs):  # noqa: F811
    """chain_pair's 1 000-node chain in [500, 500], cut at 899/900 and joined again: fewer rounds than a fresh solve."""
    for cut in (True, False):
        pair = tp.block_chain(cut)
        engines, got, G, _ = run_pair(tmp_path, tiled, libs, pair, f"chain-{'cut' if cut else 'join'}", fresh=False, keep=True)
        fresh = solve_a(engines, tp.new_sets(pair), False, False)
        close(engines)
        for key in ("cost", "hops", "parent"):
            assert all(np.array_equal(g[key].view(np.uint32), f[key].view(np.uint32)) for g, f in zip(got, fresh)), key
        rounds = sum(g["info"].rounds for g in got), sum(f["info"].rounds for f in fresh)
        print("block chain", "cut" if cut else "joined", "rounds refresh / fresh", rounds, f"ratio {rounds[0] / rounds[1]:.3f}",
              "exchanges", got[0]["info"].exchanges, "+", got[0]["info"].anchor_exchanges, "/", fresh[0]["info"].exchanges)
        assert rounds[0] < rounds[1], rounds


@pytest.mark.parametrize("cut", [True, False])
def test_alternating_chain(tmp_path, tiled, libs, cut):  # noqa: F811
    """64 nodes, every hop a seam, a link near the far end cut / joined again: results and carried only (its anchors
    take about an exchange per crossing, more than a fresh solve's exchanges)."""
    _, got, _, _ = run_pair(tmp_path, tiled, libs, tp.alternating_chain(cut), f"alt-{int(cut)}")
    assert sum(int(g["carried"][0]) for g in got) == 58


@pytest.mark.parametrize("risk", [False, True])
def test_tie_lattice(tmp_path, tiled, libs, risk):  # noqa: F811
    run_pair(tmp_path, tiled, libs, tp.tie_lattice(risk), f"lattice-{int(risk)}", risk=risk)


def test_cross_records_only(tmp_path, tiled, libs):  # noqa: F811
    pair = tp.cross_only()
    assert all(np.array_equal(m, np.arange(6)) for m in pair.maps)
    run_pair(tmp_path, tiled, libs, pair, "cross-only")
    run_pair(tmp_path, tiled, libs, pair, "cross-only-risk", risk=True)


@pytest.mark.parametrize("how", ["maps", "scramble", "forget"])
def test_renumbered(tmp_path, tiled, libs, how):  # noqa: F811
    """About 200 nodes in three tiles; tile 0 loses and gains nodes, so every later gid shifts; a scrambled map and a
    map of all -1 on tile 1 (hints: the anchor drops what they carry wrongly)."""
    pair = tp.renumbered(seed=5, V=200, R=3, scramble=how == "scramble", forget=how == "forget")
    assert pair.b.sizes[0] != pair.a.sizes[0]
    run_pair(tmp_path, tiled, libs, pair, "renum-" + how, owners=True)
    run_pair(tmp_path, tiled, libs, pair._replace(sets=[s[:1] for s in pair.sets]), "renum-risk-" + how, risk=True)


def test_empty_tiles(tmp_path, tiled, libs):  # noqa: F811
    """a tile that becomes empty, and one that is empty throughout ([6, 0, 6])"""
    after = tp.renumbered(seed=4, V=90, R=3, empty_after=True)
    assert after.a.sizes[1] > 0 and after.b.sizes[1] == 0
    run_pair(tmp_path, tiled, libs, after, "empty-after", owners=True)
    ring = tp.tiling([6, 0, 6], tp.ts.RING)
    pair = tp.Pair(ring, tp.remapped(ring, tp.identity_maps(ring), drop=[(2, 3)], values={(8, 9): (0.6, 0.5)}),
                   tp.identity_maps(ring), [[0], [7]])
    _, got, _, _ = run_pair(tmp_path, tiled, libs, pair, "empty-throughout")
    assert got[1]["carried"].tolist() == [0, 0] and got[1]["cost"].shape == (2, 0)


def test_saturation(tmp_path, tiled, libs):  # noqa: F811
    run_pair(tmp_path, tiled, libs, tp.saturation(), "saturation")


@pytest.mark.parametrize("risk", [False, True])
def test_sets_with_owners(tmp_path, tiled, libs, risk):  # noqa: F811
    """three tiles, a member on the border and a member named twice: owners, owned and the target reads"""
    pair = tp.sets_with_owners()
    if risk:
        pair = pair._replace(a=tp.levels(pair.a), b=tp.levels(pair.b, seed=1))
    targets = [np.array([0, n - 1, n // 2], np.int32) for n in pair.b.sizes]
    _, got, G, _ = run_pair(tmp_path, tiled, libs, pair, f"owners-{int(risk)}", risk=risk, owners=True, targets=targets)
    name = "risk" if risk else "cost"
    for t, g in enumerate(got):
        assert np.array_equal(g[name + "_at"].view(np.uint32), g[name][:, targets[t]].view(np.uint32))
        assert np.array_equal(g["hops_at"], g["hops"][:, targets[t]]) and np.array_equal(g["owner_at"], g["owner"][:, targets[t]])


def test_after_the_refresh(tmp_path, tiled, libs):  # noqa: F811
    """tiled_routes across two seams and tiled_field_reached from the refreshed solve; A -> B -> C with a refresh per
    step; then cost and risk refreshes in turn on one group."""
    pair = tp.tie_lattice()
    engines, got, G, _ = run_pair(tmp_path, tiled, libs, pair, "after", fresh=False, keep=True)
    f = tiled.concat_fields(got)
    from tiled_support import assert_routes, crossing_counts, want_routes
    crossings = crossing_counts(G, f["hops"][0], f["parent"][0])
    far = int(np.argmax(crossings))
    assert crossings[far] >= 2
    pairs = [(0, far), (1, int(np.argmax(f["hops"][1]))), (2, tp.new_sets(pair)[2][0])]
    want = want_routes(G, [(f["cost"][k], f["hops"][k], f["parent"][k]) for k in range(3)], pairs)
    assert_routes("after the refresh", tiled, call_routes(engines, [p[0] for p in pairs], [p[1] for p in pairs]), G, want)
    for t, e in enumerate(engines):
        r = e.tiled_field_reached(1)
        mine = np.flatnonzero(got[t]["hops"][1] >= 0) + got[t]["offset"]
        assert r["count"] == mine.shape[0] and np.array_equal(r["gids"], mine)
    # B -> C: the lattice with two more weights raised, refreshed again from the refreshed solve
    c = tp.remapped(pair.b, tp.identity_maps(pair.b), values={pair.b.edges[40][:2]: (0.8, 2.0), pair.b.edges[90][:2]: (0.8, 2.0)})
    old = tiled.concat_fields(got)
    retile(engines, tmp_path, c, "after-c")
    got = ok(refresh(engines, tp.identity_maps(c), False)[0])
    check("B -> C", tiled, libs, engines, got, False, False, old, tp.offsets(pair.b), tp.identity_maps(c), fresh=False)
    # cost and risk in turn on the one group: each entry refreshes its own objective's solve only
    sets = tp.new_sets(pair)
    solve_a(engines, sets, True, False)
    bad = refresh(engines, tp.identity_maps(c), False)[0]
    assert all(getattr(b, "status", None) == INVALID_ARG and "risk field" in str(b) for b in bad), bad
    retile(engines, tmp_path, pair.b, "after-b2")
    got = ok(refresh(engines, tp.identity_maps(c), True)[0])
    check("risk after cost", tiled, libs, engines, got, True, False, fresh=False)
    solve_a(engines, sets, False, False)
    retile(engines, tmp_path, c, "after-c2")
    got = ok(refresh(engines, tp.identity_maps(c), False)[0])
    check("cost after risk", tiled, libs, engines, got, False, False)
    close(engines)


def test_the_real_path(oa, synth, tiled, libs):  # noqa: F811
    """A built 2 x 1 tiling: stitch_exchange, a tiled solve, set_local_map + update_graph on tile 0 1.5 m from the seam,
    stitch_exchange again on the same group, a refresh through the engine's own map; then two updates before one
    refresh."""
    import trg_planner
    cols, rows, n, halo = 2, 1, 130, 11
    prm = dict(oa.MOUNTAIN, update_collision_threshold=0.2)
    cores = tiled.tile_cores(cols, rows, n, n)
    engines, clouds = [], []
    for t, core in enumerate(cores):
        cloud = synth.mountain_tile(*tiled.tile_lattice_window(t, cols, rows, n, n, halo), seed=77, amplitude=2.0, wavelength=20.0)
        e = trg_planner.Engine(**prm)
        e.set_sampler(9, 16)
        e.set_tile(core, epoch=t)
        e.set_global_map(cloud)
        e.init_graph([0.5 * (core[0] + core[2]), 0.5 * (core[1] + core[3]), 0.0])
        engines.append(e)
        clouds.append(cloud)
    lay = SimpleNamespace(cores=cores, cols=cols, rows=rows)
    join_group(engines, "real-path")
    stitch(engines, lay)
    G = exported(tiled, engines)
    stitch(engines, lay)
    valid = np.flatnonzero((G["state"] != fg.INVALID) & (np.diff(G["rowptr"]) > 0))
    sources = [int(valid[len(valid) // 3]), int(valid[-5])]
    solve_a(engines, [[s] for s in sources], False, False)

    def update(pose):
        cl = clouds[0]
        m = (np.abs(cl[:, 0] - pose[0]) < 3.0) & (np.abs(cl[:, 1] - pose[1]) < 3.0)
        obs = cl[m].copy()
        b = (np.abs(obs[:, 0] - (pose[0] + 1.0)) < 0.5) & (np.abs(obs[:, 1] - (pose[1] + 1.2)) < 0.5)
        obs[b, 2] += np.float32(1.0) * (np.arange(b.sum()) % 2).astype(np.float32)
        engines[0].set_local_map(pose, obs)
        engines[0].update_graph()

    for step, poses in enumerate([[(11.5, 5.0)], [(11.5, 5.5), (11.5, 6.0)]]):
        for pose in poses:
            update(pose)
        stitch(engines, lay)  # the second stitch_exchange of a live group
        got, secs = refresh(engines, None, False)
        got = ok(got)
        print("real path step", step, "rounds", [g["info"].rounds for g in got], "exchanges", got[0]["info"].exchanges,
              got[0]["info"].anchor_exchanges, "carried", [g["carried"].tolist() for g in got], f"{secs * 1e3:.1f} ms")
        G = exported(tiled, engines)
        stitch(engines, lay)
        sets = [s.tolist() for s in got[0]["set_gids"]]
        assert_fields(f"real path {step}", got, G, reference(libs["cost"], G, [s[0] for s in sets]))
        fresh = solve_a(engines, sets, False, False)
        for g, f in zip(got, fresh):
            assert all(np.array_equal(g[k].view(np.uint32), f[k].view(np.uint32)) for k in ("cost", "hops", "parent"))
        assert sum(int(g["carried"].sum()) for g in got) > G["V"]  # (two fields: most keys are carried)
    close(engines)


def test_refusals_and_announced_failures(tmp_path, tiled, libs):  # noqa: F811
    from trg_planner._engine import TrgError
    import trg_planner
    pair = tp.cross_only()
    ids = tp.identity_maps(pair.a)
    status = lambda got: [getattr(g, "status", 0) for g in got]  # noqa: E731
    # no communicator; no retained tiled solve
    lone = trg_planner.Engine(**MOUNTAIN)
    with pytest.raises(TrgError, match="no communicator|no tiled solve"):
        lone.tiled_refresh_fields()
    lone.close()
    engines, _ = craft(tmp_path, pair.a.sizes, pair.a.edges, tag="refuse")
    got = refresh(engines, ids, False)[0]
    assert status(got) == [INVALID_ARG] * 2 and "no tiled solve is retained" in str(got[0]), got
    # a bounded, a modelled and a start-cost solve; the other objective's entry: refused, the solve still answers
    for what, call in (("bounded", lambda r, e: e.tiled_cost_fields_bounded([0], budget=0.7)),
                       ("cost models", lambda r, e: e.tiled_cost_fields_models([0], [(1.0, np.inf)])),
                       ("start costs", lambda r, e: e.tiled_cost_fields_from([[0]], [[0.5]]))):
        ok(run_ranks(engines, call)[0])
        got = refresh(engines, ids, False)[0]
        assert status(got) == [INVALID_ARG] * 2 and what in str(got[0]), (what, got)
        ok(call_routes(engines, [0], [7]))
    solve_a(engines, pair.sets, False, False)
    got = refresh(engines, ids, True)[0]
    assert status(got) == [INVALID_ARG] * 2 and "cost field" in str(got[0]), got
    ok(call_routes(engines, [0], [7]))
    # a wrong map length on one rank: that rank's error, the peer's "another rank", well inside the guard
    got, secs = refresh(engines, [ids[0], ids[1][:-1]], False)
    assert status(got) == [DEVICE, INVALID_ARG] and "another rank reported a failure" in str(got[0]), got
    assert "node map has 5 entries" in str(got[1]) and secs < JOIN_SECONDS / 4, (got, secs)
    got = refresh(engines, ids, False)[0]  # nothing is retained afterwards
    assert status(got) == [INVALID_ARG] * 2 and "no tiled solve is retained" in str(got[0]), got
    # an entry that is no old node; no map at all (load_json leaves none)
    for maps, text in (([np.array([0, 1, 2, 3, 4, 6], np.int32), ids[1]], "is no node of this tile"), ([None, ids[1]], "no node map")):
        solve_a(engines, pair.sets, False, False)
        retile(engines, tmp_path, pair.b, "refuse-b")
        got, secs = refresh(engines, maps, False)
        assert status(got) == [INVALID_ARG, DEVICE] and text in str(got[0]) and secs < JOIN_SECONDS / 4, (got, secs)
    # a deleted member: the map of the rank that owns it does not name it
    solve_a(engines, pair.sets, False, False)
    gone = ids[1].copy()
    gone[1] = -1  # global id 7, the source of field 1
    got, secs = refresh(engines, [ids[0], gone], False)
    assert status(got) == [DEVICE, INVALID_ARG] and "has no node in this tile" in str(got[1]) and secs < JOIN_SECONDS / 4, (got, secs)
    # no current stitch on one rank: its graph changed and was not stitched again
    solve_a(engines, pair.sets, False, False)
    engines[0].load_json(str(tmp_path / "refuse0.json"))
    got, secs = refresh(engines, ids, False)
    assert status(got) == [INVALID_ARG, DEVICE] and "stitch" in str(got[0]) and secs < JOIN_SECONDS / 4, (got, secs)
    # the group is still usable, and a full cycle works after all that
    retile(engines, tmp_path, pair.a, "refuse-a2")
    solve_a(engines, pair.sets, False, False)
    retile(engines, tmp_path, pair.b, "refuse-b2")
    got = ok(refresh(engines, ids, False)[0])
    check("after the refusals", tiled, libs, engines, got, False, False)
    close(engines)
    # a different rank count: a solve in a group of two, the refresh asked of a group of one
    engines, _ = craft(tmp_path, [12], tp.ts.RING, tag="ranks")
    one = engines[0]
    solve_a([one], [[0]], False, False)
    one.comm_join_local("test-tiled-refresh-two", 2, 0)
    with pytest.raises(TrgError, match="2 ranks, the retained solve had 1"):
        one.tiled_refresh_fields(np.arange(12, dtype=np.int32))
    close(engines)
