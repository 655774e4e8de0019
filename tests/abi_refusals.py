"""The C ABI's refusals as a table: a fixed list of calls whose arguments the engine refuses, each with the
(status, last_error) it answers.  tests/test_gpu_abi_frame.py compares the table with tests/golden/abi_refusals.json;

    python tests/abi_refusals.py

records that file from the library of the tree it runs in (needs the GPU: an engine without a device refuses
everything alike).  The calls run in the order below on one engine, so the text a bare status leaves in place is
the text of the call before it.
"""
import ctypes as C
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_refusals.json")
MOUNTAIN = dict(expand_dist=0.6, robot_size=0.3, height_threshold=0.16, collision_threshold=0.1,
                update_collision_threshold=0.5, safety_factor=3.0, goal_tolerance=0.8, sample_num=7)


def refusal_table(cloud):
    """name -> [status, last_error] of every refusal; `cloud` is the map of the cases that need a graph."""
    import trg_planner
    from trg_planner import _engine as E

    L = trg_planner.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    f3 = (C.c_float * 6)(1.0, 2.0, 0.0, 4.0, 5.0, 0.0)
    f4 = (C.c_float * 4)(0.0, 0.0, 10.0, 10.0)
    i4 = (C.c_int32 * 4)(0, 0, 0, 0)
    n32 = C.c_int32(0)
    nsz = C.c_size_t(0)
    ident = (C.c_uint8 * 128)()
    pinfo = E.TrgPathInfo()
    view = E.TrgCsrView()
    xyz, xy, ints = C.cast(f3, fp), C.cast(f3, fp), C.cast(i4, ip)
    out = {}

    def row(name, h, st):
        assert name not in out, name
        out[name] = [int(st), L.trg_engine_last_error(h).decode()]

    def cases(tag, h):
        """the argument refusals: with h = None every one is the null-engine refusal"""
        r = lambda name, st: row(f"{tag}:{name}", h, st)  # noqa: E731
        # trg_engine.cpp
        r("set_global_map null cloud", L.trg_engine_set_global_map(h, None, 5, 3))
        r("set_global_map stride", L.trg_engine_set_global_map(h, xyz, 2, 2))
        r("set_global_map_device null cloud", L.trg_engine_set_global_map_device(h, None, 5, 3))
        r("set_local_map null start", L.trg_engine_set_local_map(h, None, xyz, 2, 3))
        r("init_graph null start", L.trg_engine_init_graph(h, None, None))
        r("init_graph no map", L.trg_engine_init_graph(h, xyz, None))
        r("update_graph no map", L.trg_engine_update_graph(h))
        r("set_option unknown", L.trg_engine_set_option(h, b"no_such_option", b"1"))
        r("set_option null key", L.trg_engine_set_option(h, None, b"1"))
        r("set_option zero or one", L.trg_engine_set_option(h, b"defer_overlap", b"2"))
        r("set_option host or device", L.trg_engine_set_option(h, b"replay", b"gpu"))
        r("set_option positive", L.trg_engine_set_option(h, b"field_delta_scale", b"-1"))
        r("export_csr null view", L.trg_engine_export_csr(h, E.KIND_GLOBAL, None))
        r("save_json null path", L.trg_engine_save_json(h, None))
        r("save_json no directory", L.trg_engine_save_json(h, b"/no-such-directory/graph"))
        r("load_json null path", L.trg_engine_load_json(h, None))
        r("load_json no file", L.trg_engine_load_json(h, b"/no-such-directory/graph.json"))
        r("is_collision_batch null positions",
          L.trg_engine_is_collision_batch(h, E.KIND_GLOBAL, 0.1, None, 3, None, None, None))
        r("nearest_z_batch null", L.trg_engine_nearest_z_batch(h, E.KIND_GLOBAL, None, 3, None))
        r("edge_risk_batch null", L.trg_engine_edge_risk_batch(h, E.KIND_GLOBAL, None, None, 3, None, None, None, None))
        r("voxel_filter null n_out", L.trg_engine_voxel_filter(h, xyz, 2, 3, 0.1, xyz, None, None))
        r("voxel_filter stride", L.trg_engine_voxel_filter(h, xyz, 2, 2, 0.1, xyz, C.byref(nsz), None))
        r("voxel_filter leaf", L.trg_engine_voxel_filter(h, xyz, 2, 3, 0.0, xyz, C.byref(nsz), None))
        r("is_frontier_batch null", L.trg_engine_is_frontier_batch(h, None, 3, None))
        r("get_stats null", L.trg_engine_get_stats(h, None))
        r("debug_map_index no map",
          L.trg_engine_debug_map_index(h, E.KIND_GLOBAL, None, None, None, None, None, None))
        # trg_engine_plan.ipp
        r("plan null info", L.trg_engine_plan(h, xy, xyz, None, 0, None))
        r("plan empty graph", L.trg_engine_plan(h, xy, xyz, None, 0, C.byref(pinfo)))
        r("plan_batch null offsets", L.trg_engine_plan_batch(h, xy, xyz, 1, None, 0, None, C.byref(pinfo)))
        r("plan_batch path buffer", L.trg_engine_plan_batch(h, xy, xyz, 1, None, 5, ints, C.byref(pinfo)))
        r("plan_batch empty graph", L.trg_engine_plan_batch(h, xy, xyz, 1, None, 0, ints, C.byref(pinfo)))
        # trg_engine_field.ipp
        r("cost_field source", L.trg_engine_cost_field(h, -2, None, None, None, None, None))
        r("cost_field empty graph", L.trg_engine_cost_field(h, 0, None, None, None, None, None))
        r("cost_field_batch no fields", L.trg_engine_cost_field_batch(h, 0, ints, None, None, None, None, None, 0,
                                                                      None, None, None, None, None))
        r("cost_field_bounded no sources", L.trg_engine_cost_field_bounded(h, 1, None, None, None, 0, None, None, None,
                                                                           None, 0, None, None, None, None, None, None))
        r("cost_field_bounded settle", L.trg_engine_cost_field_bounded(h, 1, ints, None, None, 7, None, None, None,
                                                                       None, 0, None, None, None, None, None, None))
        r("cost_field_sets null sets", L.trg_engine_cost_field_sets(h, 1, None, None, None, 0, None, None, None, None,
                                                                    None, 0, None, None, None, None, None, None, None))
        r("risk_field_sets null sets", L.trg_engine_risk_field_sets(h, 1, None, None, None, 0, None, None, None, None,
                                                                    None, 0, None, None, None, None, None, None, None))
        r("field_routes negative", L.trg_engine_field_routes(h, -1, None, None, None, None, None, 0, None, None))
        r("field_reached negative cap", L.trg_engine_field_reached(h, 0, None, None, None, -1, C.byref(n32), None))
        # trg_engine_stitch.inc
        r("stitch_boundary null core", L.trg_engine_stitch_boundary(h, None, 1, 1, 0, None, 0, C.byref(n32)))
        r("stitch_boundary tile", L.trg_engine_stitch_boundary(h, f4, 2, 2, 4, None, 0, C.byref(n32)))
        r("stitch_cross no tiles", L.trg_engine_stitch_cross(h, 0, 0, None, ints, None, 0, C.byref(n32)))
        r("stitch_cross no map", L.trg_engine_stitch_cross(h, 0, 1, None, ints, None, 0, C.byref(n32)))
        r("stitch_assemble null offsets", L.trg_engine_stitch_assemble(h, 0, 1, None, None, 0))
        r("graph_sizes null", L.trg_engine_graph_sizes(h, E.KIND_GLOBAL, None, None))
        # trg_engine_exchange.inc
        r("comm_unique_id null", L.trg_engine_comm_unique_id(h, None))
        r("comm_init null id", L.trg_engine_comm_init(h, None, 1, 0))
        r("comm_init rank", L.trg_engine_comm_init(h, ident, 2, 2))
        r("comm_adopt null", L.trg_engine_comm_adopt(h, None))
        r("stitch_exchange no communicator", L.trg_engine_stitch_exchange(h, f4, 1, 1, None, None))
        r("comm_join_local null name", L.trg_engine_comm_join_local(h, None, 2, 0))
        r("comm_join_local rank", L.trg_engine_comm_join_local(h, b"refusals", 2, 2))

    cases("null engine", None)
    row("null engine:comm_destroy", None, L.trg_engine_comm_destroy(None))
    row("null engine:set_tile", None, L.trg_engine_set_tile(None, None, 0))
    row("create null params", None, L.trg_engine_create(None, 0, None))

    eng = trg_planner.Engine(**MOUNTAIN)
    cases("fresh engine", eng.h)

    # an engine with a graph and no solve
    eng.set_sampler(7, 16)
    eng.set_global_map(cloud)
    eng.init_graph([15.0, 15.0, 0.0])
    V, _ = eng.graph_sizes("global")
    assert V > 100, V
    h = eng.h
    r = lambda name, st: row(f"graph:{name}", h, st)  # noqa: E731
    one = (C.c_int32 * 2)(0, 1)
    r("field_routes without a solve", L.trg_engine_field_routes(h, 1, ints, ints, C.cast(one, ip), None, None, 0, None,
                                                               None))
    r("field_reached without a solve", L.trg_engine_field_reached(h, 0, None, None, None, 0, C.byref(n32), None))
    r("cost_field_refresh without a solve", L.trg_engine_cost_field_refresh(h, None, 0, None, None, None, None, 0, None,
                                                                           None, None, None, None, None, None, None))
    r("risk_field_refresh without a solve", L.trg_engine_risk_field_refresh(h, None, 0, None, None, None, None, 0, None,
                                                                           None, None, None, None, None, None, None))
    far = (C.c_int32 * 1)(2 ** 30)
    r("cost_field source past the graph", L.trg_engine_cost_field(h, 2 ** 30, None, None, None, None, None))
    r("cost_field_batch source past the graph",
      L.trg_engine_cost_field_batch(h, 1, C.cast(far, ip), None, None, None, None, None, 0, None, None, None, None, None))
    r("cost_field_batch target past the graph",
      L.trg_engine_cost_field_batch(h, 1, ints, None, None, None, None, C.cast(far, ip), 1, None, None, None, None,
                                    None))
    r("stitch_assemble other graph", L.trg_engine_stitch_assemble(h, 0, 1, C.cast(one, ip), None, 0))
    r("stitch_exchange no communicator", L.trg_engine_stitch_exchange(h, f4, 1, 1, None, None))
    r("view of the graph still exports", L.trg_engine_export_csr(h, E.KIND_GLOBAL, C.byref(view)))
    assert view.num_nodes == V
    eng.close()
    return out


if __name__ == "__main__":
    import sys
    import torch  # noqa: F401  (first, as in conftest.py)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "trg-planner_amd"))
    from trg_planner import synth
    table = refusal_table(synth.mountain_cloud(300, 300, seed=11, amplitude=5.0, wavelength=14.0))
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(table)} refusals")
