"""GPU: the stitch kernels (trg_stitch.inc) and their host steps (stitch_boundary, stitch_cross, stitch_assemble) at
the layouts, capacities and record counts of tests/stitch_cases.py, against the plain restatement: the tiled oracle
for whole builds, tiled.stitch_local with the oracle's edge_risk for crafted records, tiled.assemble_global for crafted
cross edges.  Ids, order, rowptr, col, state, xyz and dist bit for bit; weights within 1e-5, no clamp flips.
test_stitch_cases_cpu.py shows that every case has the property it is here for."""
import ctypes as C

import numpy as np
import pytest

import stitch_cases as sc
from conftest import weight_report

pytestmark = pytest.mark.gpu
WEIGHT_TOL = 1e-5
OK, INVALID_ARG, NO_MAP, CAPACITY = 0, 1, 2, 8
CANARY = 0x5A5A5A5A


@pytest.fixture(scope="module")
def tiled():
    from trg_planner import tiled as t
    return t


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def assert_weights(w, w_ref):
    if len(w):
        flips, others, mx = weight_report(w, w_ref, WEIGHT_TOL)
        assert others == 0 and flips == 0, (flips, others, mx)


def assert_global_equal(G, OG):
    assert G["V"] == OG["V"] and np.array_equal(G["rowptr"], OG["rowptr"])
    assert np.array_equal(G["col"], OG["col"]) and np.array_equal(G["state"], OG["state"])
    assert np.array_equal(G["xyz"].view(np.uint32), OG["xyz"].view(np.uint32))
    assert np.array_equal(G["dist"].view(np.uint32), OG["dist"].view(np.uint32))
    assert_weights(G["w"], OG["w"])


# ---- a. layouts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.STEP_LAYOUTS)
def test_layout_matches_tiled_oracle(oa, synth, tiled, name):
    lay, o_graphs, o_stitched, OG, _ = sc.oracle(oa, synth, tiled, name)
    _, engines = sc.engines(oa, synth, tiled, name)
    graphs = [e.graph("global") for e in engines]
    parts, cross = tiled.stitch_emulated(engines, lay.cores, lay.cols, lay.rows)
    G = tiled.concat_stitched(parts)
    for t, (g, og) in enumerate(zip(graphs, o_graphs)):
        c = lay.cores[t]
        assert ((g.xyz[:, 0] >= c[0]) & (g.xyz[:, 0] < c[2]) & (g.xyz[:, 1] >= c[1]) & (g.xyz[:, 1] < c[3])).all()
        assert g.V == og.V and np.array_equal(g.col, og.col) and np.array_equal(g.xyz, og.xyz)
        assert (t in lay.no_graph) == (g.V == 0)
    print(name, "V per tile", [g.V for g in graphs], "cross edges", cross.shape[0])
    assert np.array_equal(cross[:, :4], o_stitched[0])  # the same cross edges in the same order
    assert np.array_equal(np.ascontiguousarray(cross[:, 5]).view(np.uint32), o_stitched[2].view(np.uint32))
    assert_weights(np.ascontiguousarray(cross[:, 4]).view(np.float32), o_stitched[1])
    assert np.array_equal(np.concatenate([p.cid for p in parts]), np.arange(G["V"]))  # rows = global ids
    assert_global_equal(G, OG)
    src = np.repeat(np.arange(G["V"]), np.diff(G["rowptr"]))
    fwd = set(zip(src.tolist(), G["col"].tolist()))
    assert all((b, a) in fwd for a, b in fwd)  # symmetric
    tile_of = np.searchsorted(G["offsets"], np.arange(G["V"]), side="right") - 1
    assert (tile_of[src] != tile_of[G["col"]]).sum() == 2 * o_stitched[0].shape[0]


# ---- b. stitch_cross on crafted records ---------------------------------------------------------------------------
def _call_cross(e, tile, ntiles, rec_t, off, buf, cap):
    """the C call itself: (status, n) -- the wrapper raises before it returns n"""
    n = C.c_int32(-1)
    st = e.L.trg_engine_stitch_cross(e.h, tile, ntiles, C.c_void_p(rec_t.data_ptr()),
                                     off.ctypes.data_as(C.POINTER(C.c_int32)),
                                     C.c_void_p(buf.data_ptr() if buf is not None else 0), cap, C.byref(n))
    return st, n.value


def _expected_rows(tiled, o, tile, ids, xyz):
    rows, w, d = tiled.stitch_local(tile, ids, xyz, sc.EXPAND, lambda p1, p2: o.edge_risk(p1, p2))
    return rows, w, d


def _assert_rows(got, want):
    rows, w, d = want
    assert got.shape[0] == rows.shape[0], (got.shape, rows.shape)
    assert np.array_equal(got[:, :4], rows)
    assert np.array_equal(np.ascontiguousarray(got[:, 5]).view(np.uint32), d.view(np.uint32))
    assert_weights(np.ascontiguousarray(got[:, 4]).view(np.float32), w)


@pytest.fixture(scope="module")
def flat(oa, dev):
    """engine and oracle on the flat map, the crafted records on the device, tile 0's full result"""
    import torch
    import trg_planner
    cloud = sc.flat_map()
    e = trg_planner.Engine(**oa.MOUNTAIN)
    e.set_global_map(cloud)
    o = oa.Oracle(**oa.MOUNTAIN)
    o.set_global_map(cloud)
    ids, xyz = sc.cross_records()
    rec, off = sc.pack_records(ids, xyz)
    rec_t = torch.from_numpy(rec).to(dev)
    torch.cuda.synchronize()
    return dict(e=e, o=o, ids=ids, xyz=xyz, rec_t=rec_t, off=off)


def _full(flat, dev, tile):
    import torch
    st, n = _call_cross(flat["e"], tile, 4, flat["rec_t"], flat["off"], None, 0)
    assert st == OK
    buf = torch.full((max(n, 1) + 1, 6), CANARY, dtype=torch.int32, device=dev)
    st, n2 = _call_cross(flat["e"], tile, 4, flat["rec_t"], flat["off"], buf, n)
    assert st == OK and n2 == n
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[n:] == CANARY).all()
    return out[:n]


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
def test_cross_on_crafted_records(flat, tiled, dev, tile):
    got = _full(flat, dev, tile)
    want = _expected_rows(tiled, flat["o"], tile, flat["ids"], flat["xyz"])
    print("tile", tile, "records", np.diff(flat["off"]).tolist(), "rows", got.shape[0])
    _assert_rows(got, want)
    assert (got.shape[0] > 2048) if tile == 0 else (got.shape[0] > 0) == (tile == 2)


def test_cross_decides_near_threshold_pairs_without_contraction(flat, dev):
    """The 128 pairs a contraction of dx*dx + dy*dy would move across expand_dist: the emitted rows hold exactly the 64
    the plain fp32 expression puts inside."""
    a, b, plain_inside, _ = sc.near_threshold_pairs()
    got = _full(flat, dev, 0)
    ids, xyz = flat["ids"], flat["xyz"]
    emitted = {(ia, ib) for ia, tb, ib in zip(got[:, 1].tolist(), got[:, 2].tolist(), got[:, 3].tolist()) if tb == 2}
    seen = 0
    for k in range(128):
        ka = np.flatnonzero((xyz[0][:, 0] == a[k, 0]) & (xyz[0][:, 1] == a[k, 1]))
        kb = np.flatnonzero((xyz[2][:, 0] == b[k, 0]) & (xyz[2][:, 1] == b[k, 1]))
        assert ka.size == 1 and kb.size == 1, k
        inside = (int(ids[0][ka[0]]), int(ids[2][kb[0]])) in emitted
        assert inside == bool(plain_inside[k]), (k, inside)
        seen += inside
    assert seen == 64


def test_cross_capacity(flat, dev):
    """cap = 0 (count only and with a buffer), 1, n - 1, n, n + 7: the status, the prefix, the canary behind cap."""
    import torch
    e = flat["e"]
    full = _full(flat, dev, 0)
    n = full.shape[0]
    for cap in (0, 1, n - 1, n, n + 7):
        buf = torch.full((cap + 3, 6), CANARY, dtype=torch.int32, device=dev)
        st, got_n = _call_cross(e, 0, 4, flat["rec_t"], flat["off"], buf, cap)
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert got_n == n, (cap, got_n)
        assert st == (CAPACITY if cap < n else OK), (cap, st)
        if cap < n:
            assert e.L.trg_engine_last_error(e.h) == b"stitch_cross: edge buffer too small"
        k = min(cap, n)
        assert np.array_equal(out[:k], full[:k]), cap
        assert (out[k:] == CANARY).all(), cap


def test_cross_bad_arguments_and_no_map(flat, oa, dev):
    import trg_planner
    e = flat["e"]
    n = C.c_int32(0)
    for tile, ntiles in ((0, 0), (0, 65), (-1, 4), (4, 4)):
        st, _ = _call_cross(e, tile, ntiles, flat["rec_t"], flat["off"] if ntiles <= 4 else np.zeros(66, np.int32), None, 0)
        assert st == INVALID_ARG, (tile, ntiles)
    bare = trg_planner.Engine(**oa.MOUNTAIN)
    st, _ = _call_cross(bare, 0, 4, flat["rec_t"], flat["off"], None, 0)
    assert st == NO_MAP
    bare.close()


def test_boundary_capacity(oa, synth, tiled, dev):
    """stitch_boundary on one built tile (the middle one of the 3 x 3): count only, then caps around n."""
    import torch
    lay, engines = sc.engines(oa, synth, tiled, "3x3")
    _, o_graphs, _, _, _ = sc.oracle(oa, synth, tiled, "3x3")
    t = 4
    e = engines[t]
    want = tiled.boundary_nodes(o_graphs[t].xyz, lay.cores[t], lay.cols, lay.rows, t, sc.EXPAND)
    core = np.ascontiguousarray(lay.cores[t], np.float32)

    def call(buf, cap):
        n = C.c_int32(-1)
        st = e.L.trg_engine_stitch_boundary(e.h, core.ctypes.data_as(C.POINTER(C.c_float)), lay.cols, lay.rows, t,
                                            C.c_void_p(buf.data_ptr() if buf is not None else 0), cap, C.byref(n))
        return st, n.value

    st, n = call(None, 0)
    assert st == OK and n == want.size and n > 20
    rec = np.empty((n, 4), np.int32)
    rec[:, 0] = want
    rec[:, 1:] = np.ascontiguousarray(o_graphs[t].xyz[want], np.float32).view(np.int32)
    for cap in (0, 1, n - 1, n, n + 7):
        buf = torch.full((cap + 3, 4), CANARY, dtype=torch.int32, device=dev)
        st, got_n = call(buf, cap)
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert got_n == n and st == (CAPACITY if cap < n else OK), (cap, st, got_n)
        k = min(cap, n)
        assert np.array_equal(out[:k], rec[:k]), cap   # ascending local id, positions bit for bit
        assert (out[k:] == CANARY).all(), cap
    n32 = C.c_int32(0)
    assert e.L.trg_engine_stitch_boundary(e.h, core.ctypes.data_as(C.POINTER(C.c_float)), lay.cols, lay.rows, t, None,
                                          -1, C.byref(n32)) == INVALID_ARG


def test_cross_uncertain_gates_take_the_second_attempt(oa, mountain_small, tiled, dev):
    """debug_gate_margin = 0.15 on rough ground: the device leaves slope gates to the host's libm, stitch_cross runs
    its selection a second time, and the rows are those of the run without the option, bit for bit, and the oracle's."""
    import torch
    import trg_planner
    o = oa.Oracle(**oa.MOUNTAIN)
    o.set_global_map(mountain_small)
    ids, xyz = sc.rough_records(o.nearest_z)
    rec, off = sc.pack_records(ids, xyz)
    rec_t = torch.from_numpy(rec).to(dev)
    torch.cuda.synchronize()
    e = trg_planner.Engine(**oa.MOUNTAIN)
    e.set_global_map(mountain_small)
    runs = []
    for margin in (None, 0.15):
        if margin is not None:
            e.set_option("debug_gate_margin", margin)
        before = e.stats()
        st, n = _call_cross(e, 0, 4, rec_t, off, None, 0)
        assert st == OK and n > 50
        buf = torch.full((n + 1, 6), CANARY, dtype=torch.int32, device=dev)
        st, n2 = _call_cross(e, 0, 4, rec_t, off, buf, n)
        torch.cuda.synchronize()
        assert st == OK and n2 == n
        after = e.stats()
        runs.append((buf.cpu().numpy()[:n], after["stitch_gate_retries"] - before["stitch_gate_retries"],
                     after["gate_uncertain"] - before["gate_uncertain"]))
    (plain, retries0, unc0), (wide, retries1, unc1) = runs
    print("rows", plain.shape[0], "second attempts", retries0, "->", retries1, "gates left to the host", unc0, "->", unc1)
    assert retries1 == 2 and unc1 > 10 and unc1 > unc0  # (both calls of the wide run: the count and the emit)
    assert np.array_equal(plain, wide)
    _assert_rows(plain, _expected_rows(tiled, o, 0, ids, xyz))
    e.close()


# ---- c. stitch_assemble on crafted edges --------------------------------------------------------------------------
def _assemble(e, tile, ntiles, off, edges, dev):
    import torch
    ed = torch.from_numpy(np.ascontiguousarray(edges)).to(dev) if edges.shape[0] else None
    torch.cuda.synchronize()
    st = e.L.trg_engine_stitch_assemble(e.h, tile, ntiles, off.ctypes.data_as(C.POINTER(C.c_int32)),
                                        C.c_void_p(ed.data_ptr() if ed is not None else 0), int(edges.shape[0]))
    return st


def _assert_assembled(e, g, want):
    s = e.graph("stitched")
    assert s.V == g.V and np.array_equal(s.rowptr, want["rowptr"])
    assert np.array_equal(s.col, want["col"]) and np.array_equal(s.cid, want["cid"])
    assert np.array_equal(s.w.view(np.uint32), want["w"].view(np.uint32))       # (copied, never computed)
    assert np.array_equal(s.dist.view(np.uint32), want["dist"].view(np.uint32))
    assert np.array_equal(s.state, g.state) and np.array_equal(s.xyz.view(np.uint32), g.xyz.view(np.uint32))
    assert e.graph_sizes("stitched") == (g.V, int(want["rowptr"][-1]))


def _ring_engine(oa, V, tmp_path):
    import trg_planner
    from field_support import write_graph
    nodes, edges, g = sc.ring_graph(V)
    p = tmp_path / f"ring{V}.json"
    write_graph(p, nodes, edges)
    e = trg_planner.Engine(**oa.MOUNTAIN)
    e.load_json(p)
    x = e.graph("global")
    assert x.V == V and np.array_equal(x.rowptr, g.rowptr) and np.array_equal(x.col, g.col)
    assert np.array_equal(x.w.view(np.uint32), g.w.view(np.uint32))
    assert np.array_equal(x.dist.view(np.uint32), g.dist.view(np.uint32))
    return e, g


@pytest.mark.parametrize("V", [255, 256, 257, 2049])
def test_assemble_rings_across_block_and_scan_tile(oa, tiled, dev, tmp_path, V):
    """Graphs loaded from JSON (the upload branch of stitch_dev_graph) with V at the block and scan-tile edges."""
    e, g = _ring_engine(oa, V, tmp_path)
    off = sc.assemble_offsets(V)
    for name, edges in sc.assemble_edge_lists(V).items():
        assert _assemble(e, sc.TILE, sc.NTILES, off, edges, dev) == OK, (name, e.L.trg_engine_last_error(e.h))
        _assert_assembled(e, g, sc.assemble_expected(tiled, g, edges))
    e.close()


@pytest.mark.parametrize("branch", ["resident", "uploaded"])
def test_assemble_built_tile(oa, synth, tiled, dev, tmp_path, branch):
    """A built tile's graph, still resident on the device after its build, and the same graph after save_json /
    load_json into a fresh engine, where it is uploaded from the host copy."""
    import trg_planner
    _, engines = sc.engines(oa, synth, tiled, "3x1")
    e = engines[0]
    g = e.graph("global")
    if branch == "uploaded":
        e.save_json(tmp_path / "tile.json")
        e = trg_planner.Engine(**oa.MOUNTAIN)
        e.load_json(tmp_path / "tile.json")
        x = e.graph("global")
        assert x.V == g.V and np.array_equal(x.col, g.col) and np.array_equal(x.xyz.view(np.uint32), g.xyz.view(np.uint32))
        assert np.array_equal(x.w.view(np.uint32), g.w.view(np.uint32))
    gg = sc.SimpleNamespace(V=g.V, xyz=g.xyz, state=g.state, rowptr=g.rowptr, col=g.col, w=g.w, dist=g.dist)
    off = sc.assemble_offsets(g.V)
    for name, edges in sc.assemble_edge_lists(g.V).items():
        assert _assemble(e, sc.TILE, sc.NTILES, off, edges, dev) == OK, (name, e.L.trg_engine_last_error(e.h))
        _assert_assembled(e, gg, sc.assemble_expected(tiled, gg, edges))


def test_assemble_refusals(oa, tiled, dev, tmp_path):
    V = 257
    e, g = _ring_engine(oa, V, tmp_path)
    off = sc.assemble_offsets(V)
    good = sc.assemble_edge_lists(V)["every_row"]

    def stitched_is_gone():
        assert e.graph_sizes("stitched") == (0, 0)
        s = e.graph("stitched")
        assert s.V == 0 and s.E == 0 and np.array_equal(s.rowptr, [0])

    assert _assemble(e, sc.TILE, sc.NTILES, off, good, dev) == OK
    assert e.graph_sizes("stitched")[1] == g.col.shape[0] + V
    # 65 tiles: refused before anything is touched
    assert _assemble(e, sc.TILE, 65, np.concatenate([off, off[-1:]]), good, dev) == INVALID_ARG
    assert e.L.trg_engine_last_error(e.h) == b"stitch_assemble: bad arguments"
    # edges that name a tile or a node outside node_offsets: counted, refused, and the view before them is gone
    w, d = 0.5, 0.25
    bad_rows = [(-1, 0, sc.TILE, 0, w, d), (sc.TILE, 1, sc.NTILES, 0, w, d), (sc.LOW, 0, sc.TILE, V, w, d)]
    for k in range(1, 4):
        assert _assemble(e, sc.TILE, sc.NTILES, off, good, dev) == OK
        edges = np.concatenate([good[:100], sc._edges(bad_rows[:k]), good[100:]], 0)
        assert _assemble(e, sc.TILE, sc.NTILES, off, edges, dev) == INVALID_ARG
        msg = e.L.trg_engine_last_error(e.h).decode()
        assert msg == f"stitch_assemble: {k} cross edges name a tile or a node outside node_offsets", msg
        stitched_is_gone()
    # ... and a good call afterwards gives the whole result again
    assert _assemble(e, sc.TILE, sc.NTILES, off, good, dev) == OK
    _assert_assembled(e, g, sc.assemble_expected(tiled, g, good))
    e.close()
