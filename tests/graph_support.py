"""Test helper: what the tests of built graphs share -- a local-map crop of a cloud with an obstacle that the global
map lacks, the driver that takes an engine and the oracle through the steps of update_scenarios.py, the oracle's
fp64-covariance witness of a build with the engine build and the bit-for-bit comparison that go with it (_witness,
_build, _check_build), and the reference's invariants of a built graph.  Test code only."""
import numpy as np


def obs_crop(cloud, centre, half, box=None):
    m = (np.abs(cloud[:, 0] - centre[0]) < half) & (np.abs(cloud[:, 1] - centre[1]) < half)
    obs = cloud[m].copy()
    if box is not None:  # raise a block of points: an obstacle that was not in the global map
        b = (np.abs(obs[:, 0] - box[0]) < box[2]) & (np.abs(obs[:, 1] - box[1]) < box[2])
        obs[b, 2] += np.float32(1.0) * (np.arange(b.sum()) % 2).astype(np.float32)
    return obs


GRAPH_FIELDS = ("rowptr", "col", "state", "xyz", "dist", "cid")


def first_difference(g, ref, weights="bits"):
    """The first field in which graph g differs from ref, as a sentence, or None.  V, E, then GRAPH_FIELDS bit for
    bit; weights="bits": w bit for bit as well (None: w is left to the caller)."""
    if g.V != ref.V or g.E != ref.E:
        return f"V, E = {g.V}, {g.E}; expected {ref.V}, {ref.E}"
    for name in GRAPH_FIELDS + (("w",) if weights == "bits" else ()):
        a, b = getattr(g, name), getattr(ref, name)
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if not np.array_equal(a, b):
            k = np.argwhere(a != b)[0]
            at = tuple(int(v) for v in k)
            return f"{name}{list(at)} = {getattr(g, name)[at]!r}; expected {getattr(ref, name)[at]!r} " \
                   f"({int((a != b).sum())} entries differ)"
    return None


def _probe_local(engine, oracle, witness, pose, local_xyz, prm, where):
    """isFrontier / isCollision(local) agree at the local nodes, at the pose and at 200 seeded points of a box 1 m
    larger than the local map's (some lie outside it)."""
    rng = np.random.default_rng(1234)
    lo, hi = local_xyz[:, :2].min(axis=0) - 1.0, local_xyz[:, :2].max(axis=0) + 1.0
    sets = {"random points": rng.uniform(lo, hi, size=(200, 2)).astype(np.float32),
            "pose": np.asarray([pose], np.float32)}
    if engine is not None:
        sets["local nodes"] = engine.graph("local").xyz[:, :2]
    thr = prm["update_collision_threshold"]
    for name, xy in sets.items():
        if xy.shape[0] == 0:
            continue
        fo = oracle.is_frontier(xy)
        co, _, no = oracle.is_collision(xy, 1, thr)
        others = [("witness", witness.is_frontier(xy), witness.is_collision(xy, 1, thr))]
        if engine is not None:
            others.append(("engine", engine.is_frontier(xy), engine.is_collision(xy, kind="local", threshold=thr)))
        for who, f, (c, _, n) in others:
            assert np.array_equal(f, fo), f"{where}: is_frontier of the {who} at the {name}: " \
                                          f"{int((f != fo).sum())} of {xy.shape[0]} differ"
            assert np.array_equal(c, co) and np.array_equal(n, no), \
                f"{where}: is_collision(local) of the {who} at the {name}: {int((c != co).sum())} flags, " \
                f"{int((n != no).sum())} counts of {xy.shape[0]} differ"


def drive(engine, oracle, witness, steps, check=None, *, clouds, prm):
    """Take a trg_planner.Engine, an oracle and the oracle's fp64-covariance witness through `steps`
    (update_scenarios.py) and compare after every one that changes something:
      init*, update: the engine's global graph with the oracle's by conftest.assert_graph_equal (structure bit for
                     bit, weights within 1e-5, no clamp flip), and its weights and col bit for bit with the witness's;
      local:         isFrontier and isCollision(local) against the oracle, see _probe_local;
      plan:          the path bit for bit and path_length.
    engine=None: the two oracles alone, compared with each other (structure bit for bit, weights as above).
    A failure names the step and the first differing field.  check(i, step, record) runs after every init / update.
    -> the records: dict(i, kind, V, E, xyz, deg0 (the rows without an edge), frontier (the number of Frontier nodes),
    nonzero_w (the number of non-zero weights), wire_calls (wireEdge calls of an update), local_V, stats) of the
    ORACLE's graph after the step (local_V, stats: the engine's local-graph size before an update and its stats()
    after the step, else None)."""
    from concurrent.futures import ThreadPoolExecutor
    # the two oracles work beside the engine, each on a thread of its own (their calls hold no Python lock)
    with ThreadPoolExecutor(2) as pool:
        return _drive(pool, engine, oracle, witness, steps, check, clouds, prm)


def _drive(pool, engine, oracle, witness, steps, check, clouds, prm):
    from conftest import assert_graph_equal
    cloud, memo, hist, local_V, calls_before = None, {}, [], None, 0
    for i, step in enumerate(steps):
        kind = step[0]
        where = f"step {i} {step[0]}"
        if kind == "map":
            cloud = clouds[step[1]]
            for who in (engine, oracle, witness):
                if who is not None:
                    who.set_global_map(cloud)
        elif kind == "replay":
            if engine is not None:
                engine.set_option("replay", step[1])
        elif kind in ("init", "init_declined"):
            built = [pool.submit(who.init_graph, step[1]) for who in (oracle, witness)]
            if engine is not None:
                if kind == "init_declined":
                    engine.set_option("debug_fallback_level", step[2])
                try:
                    engine.init_graph(step[1])
                finally:
                    engine.set_option("debug_fallback_level", -1)
            assert all(f.result() for f in built), where
        elif kind == "local":
            graph = oracle.graph(0)
            pose = step[1](graph, memo) if callable(step[1]) else step[1]
            local = np.ascontiguousarray(step[2](cloud, pose, graph, memo), dtype=np.float32)
            for who in (engine, oracle, witness):
                if who is not None:
                    who.set_local_map(pose, local)
            _probe_local(engine, oracle, witness, pose, local, prm, where)
            local_V = None if engine is None else engine.graph("local").V
        elif kind == "update":
            calls_before = oracle.counters()["wire_calls"]
            updated = [pool.submit(who.update_graph) for who in (oracle, witness)]
            if engine is not None:
                engine.update_graph()
            for f in updated:
                f.result()
        elif kind == "plan":
            po, io = oracle.plan(step[1], step[2])
            assert po.shape[0] > 1, f"{where}: the oracle finds no path"
            if engine is not None:
                pe, ie = engine.plan(step[1], step[2])
                assert np.array_equal(pe.view(np.uint32), po.view(np.uint32)), f"{where}: the paths differ"
                assert ie.path_length == io[1], f"{where}: path_length {ie.path_length} != {io[1]}"
        else:
            raise ValueError(f"unknown step {step!r}")
        if kind not in ("init", "init_declined", "update"):
            continue
        go, gw = oracle.graph(0), witness.graph(0)
        ge = gw if engine is None else engine.graph("global")
        diff = first_difference(ge, go, weights=None)
        assert diff is None, f"{where}: {'witness' if engine is None else 'engine'} against the oracle: {diff}"
        try:
            assert_graph_equal(ge, go, 1e-5)
        except AssertionError as err:
            raise AssertionError(f"{where}: weights against the oracle (others over 1e-5, max) or clamp flips "
                                 f"(found, allowed): {err}") from None
        if engine is not None:
            assert np.array_equal(ge.col, gw.col), f"{where}: col differs from the witness's"
            same = ge.w.view(np.uint32) == gw.w.view(np.uint32)
            assert same.all(), f"{where}: w differs from the witness's on {int((~same).sum())} of {ge.E} edges, " \
                               f"by {float(np.abs(ge.w - gw.w).max())} at the most"
        rec = dict(i=i, kind="update" if kind == "update" else "init", V=go.V, E=go.E, xyz=go.xyz,
                   deg0=np.flatnonzero(np.diff(go.rowptr) == 0), frontier=int((go.state == 1).sum()),
                   nonzero_w=int((go.w != 0).sum()),
                   wire_calls=oracle.counters()["wire_calls"] - calls_before if kind == "update" else None,
                   local_V=local_V if kind == "update" else None, stats=None if engine is None else engine.stats())
        hist.append(rec)
        if check is not None:
            check(i, step, rec)
    return hist


SEED = 7  # sampler seed of _witness and _build (table bits 16)


def _assert_same_graph(g, ref, what):
    assert (g.V, g.E) == (ref.V, ref.E), (what, g.V, ref.V, g.E, ref.E)
    assert np.array_equal(g.rowptr, ref.rowptr), what
    assert np.array_equal(g.col, ref.col), what
    assert np.array_equal(g.state, ref.state), what
    assert np.array_equal(g.cid, ref.cid), what
    assert np.array_equal(g.xyz.view(np.uint32), ref.xyz.view(np.uint32)), what
    assert np.array_equal(g.dist.view(np.uint32), ref.dist.view(np.uint32)), what
    differ = int((g.w.view(np.uint32) != ref.w.view(np.uint32)).sum())
    assert differ == 0, (what, differ, float(np.abs(g.w - ref.w).max()))


_witnesses = {}


def _witness(oa, key, prm, cloud, start, core=None):
    """(graph before cleanGraph, after it, the oracle's counters) of the fp64-covariance witness, computed once."""
    if key not in _witnesses:
        o = oa.Oracle(**prm)
        o.set_sampler(SEED, 0, 16)
        o.set_cov_f64(True)
        if core is not None:
            o.set_tile(core, epoch=0)
        o.set_global_map(cloud)
        assert o.init_graph(start)
        _witnesses[key] = (o.graph(1), o.graph(0), o.counters())
        o.close()
    return _witnesses[key]


def _build_any(prm, cloud, start, options, core=None):
    """An engine built with keep_preclean and `options`, whichever path built it -> (engine, its stats)."""
    import trg_planner
    e = trg_planner.Engine(**prm)
    e.set_sampler(SEED, 16)
    e.set_option("keep_preclean", 1)
    for k, v in options.items():
        e.set_option(k, v)
    if core is not None:
        e.set_tile(core, epoch=0)
    e.set_global_map(cloud)
    e.init_graph(start)
    return e, e.stats()


def _build(prm, cloud, start, options, core=None):
    e, st = _build_any(prm, cloud, start, options, core)
    assert st["used_device_bfs"] == 1 and st["bfs_fallbacks"] == 0, (options, e.fallback_reason)
    return e, st


def _check_build(e, st, witness, what, device=True):
    """device=False: a build the host replay made, which has no speculative parent edges to count."""
    pre, clean, c = witness
    _assert_same_graph(e.graph("preclean"), pre, what + ": before cleanGraph")
    _assert_same_graph(e.graph("global"), clean, what + ": after cleanGraph")
    assert st["trials"] == c["trials"], what
    assert st["samples"] == c["samples"], what
    assert st["created_nodes"] == c["created"], what
    assert st["invalid_nodes"] == c["invalid_created"], what
    assert st["bytes_sample_kernel"] == 12 * c["sample_hits"], (what, st["bytes_sample_kernel"], c["sample_hits"])
    if device:
        assert st["bytes_spec_created"] == 12 * c["wire_hits_new"], (what, st["bytes_spec_created"], c["wire_hits_new"])


def graph_invariants(g, expand_dist):
    assert (g.state != -1).all() and (np.diff(g.rowptr) >= 1).all()       # cleanGraph post-condition
    assert (g.dist < 2.5 * expand_dist).all()                              # trg.cpp:279
    nz = g.w[g.w != 0]
    assert ((nz >= 0.1) & (nz <= 0.4761)).all()                            # trg.cpp:359-363
    src = np.repeat(np.arange(g.V, dtype=np.int64), np.diff(g.rowptr))
    key = src * g.V + g.col
    rev = g.col.astype(np.int64) * g.V + src
    assert np.array_equal(np.sort(key), np.sort(rev))                      # edges are symmetric
    assert np.unique(key).size == key.size                                 # wireEdge's dedupe
    # nodes are at least robot_size apart only in a statistical sense (merge test is against the
    # NEAREST node); what must hold exactly: every edge length equals the fp32 node distance
    d = np.sqrt(((g.xyz[src, 0] - g.xyz[g.col, 0]) ** 2 + (g.xyz[src, 1] - g.xyz[g.col, 1]) ** 2))
    assert np.abs(d - g.dist).max() < 1e-5
