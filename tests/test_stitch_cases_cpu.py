"""CPU: every case of tests/stitch_cases.py has the property it was made for, shown with the oracle and numpy alone
(the GPU tests, test_gpu_stitch_steps.py and test_gpu_exchange_ranks.py, rest on these)."""
import numpy as np
import pytest

import stitch_cases as sc


@pytest.fixture(scope="module")
def tiled():
    from trg_planner import tiled as t
    return t


def test_grid_3x3_has_diagonal_and_multi_tile_rows(oa, synth, tiled):
    lay, graphs, stitched, G, _ = sc.oracle(oa, synth, tiled, "3x3")
    census = sc.cross_census(stitched, graphs)
    diag = sc.diagonal_edges(stitched, lay.cols)
    print("3x3:", [g.V for g in graphs], census, "diagonal", diag)
    assert census["n_cross"] >= 200 and diag >= 1 and census["multi_rows"] >= 5
    # the centre tile shares all four sides, and every one of them carries edges
    others = set(stitched[0][stitched[0][:, 0] == 4][:, 2].tolist()) | set(stitched[0][stitched[0][:, 2] == 4][:, 0].tolist())
    assert {1, 3, 5, 7} <= others, others


@pytest.mark.parametrize("name", ["3x1", "1x3", "split_3x1"])
def test_strips_have_cross_edges_on_both_seams(oa, synth, tiled, name):
    lay, graphs, stitched, G, _ = sc.oracle(oa, synth, tiled, name)
    ids = stitched[0]
    print(name, [g.V for g in graphs], sc.cross_census(stitched, graphs))
    assert ids.shape[0] >= 40
    assert ((ids[:, 0] == 0) & (ids[:, 2] == 1)).any() and ((ids[:, 0] == 1) & (ids[:, 2] == 2)).any()
    # the middle tile's records come from its two shared sides alone: in a column these are sides 4 and 8
    mid = tiled.boundary_nodes(graphs[1].xyz, lay.cores[1], lay.cols, lay.rows, 1, sc.EXPAND)
    assert 0 < mid.size < graphs[1].V


def test_split_tile_cores_are_unequal(tiled):
    lay = sc.layout(tiled, "split_3x1")
    widths = [int(round(float(c[2] - c[0]) / 0.1)) for c in lay.cores]
    assert widths == [43, 43, 44], widths


@pytest.mark.parametrize("name", ["empty_mid", "island_mid"])
def test_middle_tile_without_records(oa, synth, tiled, name):
    lay, graphs, stitched, G, _ = sc.oracle(oa, synth, tiled, name)
    nb = [tiled.boundary_nodes(g.xyz, lay.cores[t], lay.cols, lay.rows, t, sc.EXPAND).size for t, g in enumerate(graphs)]
    print(name, [g.V for g in graphs], nb, stitched[0].shape[0])
    if name == "empty_mid":
        assert graphs[1].V == 0
    else:
        assert graphs[1].V > 0
    assert nb[1] == 0 and nb[0] > 0 and nb[2] > 0
    assert stitched[0].shape[0] == 0  # the outer tiles have boundary nodes and nothing to pair them with
    assert G["V"] == sum(g.V for g in graphs)


def test_near_threshold_selection_is_full_and_flips():
    a, b, plain_inside, census = sc.near_threshold_pairs()
    print("near-threshold census:", census)
    assert a.shape == (128, 2) and b.shape == (128, 2)
    assert plain_inside[:64].all() and not plain_inside[64:].any()
    assert (a[:, 0] < 6.0).all() and (b[:, 0] >= 6.0).all()
    v = sc.pair_tests(a, b)
    assert np.array_equal(v["plain"], plain_inside)
    assert ((v["fma_x"] != v["plain"]) | (v["fma_y"] != v["plain"])).all()  # a contraction moves every one of them
    assert (v["fma_x"] != v["plain"]).any() and (v["fma_y"] != v["plain"]).any()  # and each contraction some
    # numpy's own statement of the rule (tiled.cross_pairs) is the plain one
    from trg_planner import tiled
    for k in range(128):
        ia, _, _ = tiled.cross_pairs(0, [a[k:k + 1], b[k:k + 1]], sc.EXPAND)
        assert (ia.size == 1) == bool(plain_inside[k]), k


def test_cross_records_cross_block_and_scan_tile(oa, tiled):
    ids, xyz = sc.cross_records()
    na = [i.shape[0] for i in ids]
    assert na == [828, 0, 428, 5]
    assert na[0] > 256 and (len(na) - 1) * na[0] > 2048
    ia, iu, ib = tiled.cross_pairs(0, xyz, sc.EXPAND)
    ia2, _, _ = tiled.cross_pairs(2, xyz, sc.EXPAND)
    print("pairs of tile 0:", ia.size, "by other tile", {int(u): int((iu == u).sum()) for u in np.unique(iu)},
          "of tile 2:", ia2.size)
    assert ia.size > 2048 and set(np.unique(iu).tolist()) == {2, 3} and ia2.size > 0
    # on the flat map the oracle accepts every pair: the emitted rows are the pairs
    o = oa.Oracle(**oa.MOUNTAIN)
    o.set_global_map(sc.flat_map())
    rows, w, d = tiled.stitch_local(0, ids, xyz, sc.EXPAND, lambda p1, p2: o.edge_risk(p1, p2))
    assert rows.shape[0] == ia.size and w.shape[0] == ia.size


def test_rough_records_meet_slope_gates(oa, mountain_small, tiled):
    o = oa.Oracle(**oa.MOUNTAIN)
    o.set_global_map(mountain_small)
    ids, xyz = sc.rough_records(o.nearest_z)
    ia, iu, ib = tiled.cross_pairs(0, xyz, sc.EXPAND)
    p1, p2 = xyz[0][ia], np.where((iu == 2)[:, None], xyz[2][np.minimum(ib, xyz[2].shape[0] - 1)],
                                  xyz[3][np.minimum(ib, xyz[3].shape[0] - 1)])
    st, _, w, d = o.edge_risk(p1, p2)
    # the gate: |dz| * robot_size / (height_threshold * dist) against 1 (trg.cpp:269-274); within 15 % of it the
    # engine under debug_gate_margin = 0.15 leaves the decision to the host
    dz = np.abs(p1[:, 2] - p2[:, 2]).astype(np.float64)
    ratio = dz * oa.MOUNTAIN["robot_size"] / (oa.MOUNTAIN["height_threshold"] * np.maximum(d.astype(np.float64), 1e-9))
    band = int((np.abs(ratio - 1.0) < 0.1).sum())
    print("rough pairs:", ia.size, "status counts", np.bincount(st, minlength=5).tolist(), "near the gate", band)
    assert ia.size > 300 and (st == 0).sum() > 50 and (st == 1).sum() > 50 and band > 5


@pytest.mark.parametrize("V", [255, 256, 257, 2049])
def test_assemble_cases_against_a_row_by_row_statement(tiled, V):
    """assemble_expected (tiled.assemble_global on 64 tiles) against the rule said row by row."""
    _, _, g = sc.ring_graph(V)
    off = sc.assemble_offsets(V)
    assert off[sc.TILE] == sc.N_LOW and off[sc.TILE + 1] - off[sc.TILE] == V and off[-1] == sc.N_LOW + V + sc.N_HIGH
    for name, edges in sc.assemble_edge_lists(V).items():
        want = sc.assemble_expected(tiled, g, edges)
        extra = {i: [] for i in range(V)}
        for ta, ia, tb, ib, w, d in edges.tolist():
            if ta == sc.TILE:
                extra[ia].append((int(off[tb]) + ib, w, d))
            if tb == sc.TILE:
                extra[ib].append((int(off[ta]) + ia, w, d))
        col, wbits, dbits, rowptr = [], [], [], [0]
        for i in range(V):
            for k in range(g.rowptr[i], g.rowptr[i + 1]):
                col.append(int(g.col[k]) + int(off[sc.TILE]))
                wbits.append(int(g.w[k:k + 1].view(np.int32)[0]))
                dbits.append(int(g.dist[k:k + 1].view(np.int32)[0]))
            for c, w, d in sorted(extra[i]):
                col.append(c)
                wbits.append(w)
                dbits.append(d)
            rowptr.append(len(col))
        assert np.array_equal(want["rowptr"], rowptr), name
        assert np.array_equal(want["col"], col), name
        assert np.array_equal(want["w"].view(np.int32), wbits) and np.array_equal(want["dist"].view(np.int32), dbits)
        if name == "fan_200":
            assert max(len(v) for v in extra.values()) == 200
        if name == "every_row":
            assert all(len(v) == 1 for v in extra.values())
