"""ctypes binding of csrc/libtrg_engine.so (C ABI: include/trg_engine.h).

The library is the product; this module adds nothing but argument marshalling.  There is no
fallback: if the shared library is missing, or no gfx950 device is usable, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.normpath(os.path.join(_HERE, "..", "csrc"))
# TRG_ENGINE_LIB: another build of the same library (A/B measurements of kernel variants on one box)
LIB_PATH = os.environ.get("TRG_ENGINE_LIB") or os.path.join(CSRC, "libtrg_engine.so")

KIND_GLOBAL, KIND_LOCAL, KIND_PRECLEAN, KIND_STITCHED = 0, 1, 2, 3
_KINDS = {"global": KIND_GLOBAL, "local": KIND_LOCAL, "preclean": KIND_PRECLEAN,
          "stitched": KIND_STITCHED}

STATUS_NAMES = {0: "TRG_OK", 1: "TRG_ERR_INVALID_ARG", 2: "TRG_ERR_NO_MAP", 3: "TRG_ERR_NO_ROOT",
                4: "TRG_ERR_DEVICE", 5: "TRG_ERR_NO_GRAPH", 6: "TRG_ERR_NOT_FOUND",
                7: "TRG_ERR_IO", 8: "TRG_ERR_CAPACITY"}


class TrgError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


class TrgParams(C.Structure):
    _fields_ = [("is_verbose", C.c_int32), ("expand_dist", C.c_float), ("robot_size", C.c_float),
                ("sample_num", C.c_int32), ("height_threshold", C.c_float),
                ("collision_threshold", C.c_float), ("update_collision_threshold", C.c_float),
                ("safety_factor", C.c_float), ("goal_tolerance", C.c_float)]


class TrgSampler(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("table_bits", C.c_int32)]


class TrgCsrView(C.Structure):
    _fields_ = [("num_nodes", C.c_int32), ("num_edges", C.c_int32),
                ("node_xyz", C.POINTER(C.c_float)), ("node_state", C.POINTER(C.c_int32)),
                ("rowptr", C.POINTER(C.c_int32)), ("col", C.POINTER(C.c_int32)),
                ("weight", C.POINTER(C.c_float)), ("dist", C.POINTER(C.c_float)),
                ("creation_id", C.POINTER(C.c_int32))]


class TrgPathInfo(C.Structure):
    _fields_ = [("direct_dist", C.c_float), ("path_length", C.c_float), ("avg_risk", C.c_float),
                ("num_points", C.c_int32)]


class TrgFieldInfo(C.Structure):
    _fields_ = [("source", C.c_int32), ("reached", C.c_int32), ("rounds", C.c_int32),
                ("host_syncs", C.c_int32), ("ms_device", C.c_double), ("ms_total", C.c_double)]


class TrgTiledFieldInfo(C.Structure):
    _fields_ = [("exchanges", C.c_int32), ("rounds", C.c_int32), ("ghosts", C.c_int32), ("border_nodes", C.c_int32),
                ("records_sent", C.c_int64), ("ms_device", C.c_float), ("ms_total", C.c_float)]


class TrgTiledSetInfo(C.Structure):
    _fields_ = [("exchanges", C.c_int32), ("owner_exchanges", C.c_int32), ("rounds", C.c_int32), ("ghosts", C.c_int32),
                ("border_nodes", C.c_int32), ("roots", C.c_int32), ("records_sent", C.c_int64),
                ("owner_records_sent", C.c_int64), ("ms_device", C.c_float), ("ms_total", C.c_float)]


class TrgTiledRefreshInfo(C.Structure):
    _fields_ = [("exchanges", C.c_int32), ("anchor_exchanges", C.c_int32), ("owner_exchanges", C.c_int32),
                ("rounds", C.c_int32), ("ghosts", C.c_int32), ("border_nodes", C.c_int32), ("roots", C.c_int32),
                ("m", C.c_int32), ("owners", C.c_int32), ("reserved", C.c_int32), ("records_sent", C.c_int64),
                ("anchor_records_sent", C.c_int64), ("owner_records_sent", C.c_int64), ("ms_device", C.c_float),
                ("ms_total", C.c_float)]


class TrgRouteInfo(C.Structure):
    _fields_ = [("num_nodes", C.c_int32), ("cost", C.c_float), ("path_length", C.c_float),
                ("avg_risk", C.c_float)]


class TrgTiledRouteInfo(C.Structure):
    _fields_ = [("num_nodes", C.c_int32), ("cost", C.c_float), ("path_length", C.c_float), ("avg_risk", C.c_float),
                ("root_gid", C.c_int32), ("owner", C.c_int32)]


class TrgTiledRoutesInfo(C.Structure):
    _fields_ = [("exchanges", C.c_int32), ("max_nodes", C.c_int32), ("records_sent", C.c_int64),
                ("ms_device", C.c_float), ("ms_total", C.c_float)]


class TrgFieldModel(C.Structure):
    _fields_ = [("safety_factor", C.c_float), ("max_weight", C.c_float)]


class TrgZone(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("r", C.c_float)]


class TrgPoseInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_candidates", C.c_int32), ("n_links", C.c_int32), ("z", C.c_float)]


class TrgStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "map_points", "expanded_nodes", "trials", "samples", "created_nodes", "invalid_nodes",
        "edge_calls", "edge_evals_gpu", "nn_ties", "gate_uncertain", "sync_batches",
        "bytes_sample_kernel", "bytes_spec_kernel", "bytes_edge_kernel", "bytes_index_build")] + [
        ("ms_index_build", C.c_double), ("ms_sample_kernel", C.c_double),
        ("ms_spec_kernel", C.c_double), ("ms_edge_kernel", C.c_double),
        ("launches_sample_kernel", C.c_uint64), ("launches_spec_kernel", C.c_uint64),
        ("launches_edge_kernel", C.c_uint64), ("ms_set_map_total", C.c_double),
        ("ms_init_graph_total", C.c_double), ("ms_replay_host", C.c_double),
        ("ms_finalize_host", C.c_double), ("ms_wait_gpu", C.c_double),
        ("bfs_levels", C.c_uint64), ("used_device_bfs", C.c_uint64), ("bfs_fallbacks", C.c_uint64),
        ("bfs_max_spin", C.c_uint64), ("bfs_host_levels", C.c_uint64),
        ("map_nn_ties", C.c_uint64),
        ("ms_bfs_loop", C.c_double), ("ms_deferred", C.c_double),
        ("map_nn_resolved", C.c_uint64), ("map_nn_unresolved", C.c_uint64),
        ("bfs_tie_fixups", C.c_uint64), ("bytes_spec_created", C.c_uint64),
        ("ms_rare_events", C.c_double), ("bfs_ticket_reruns", C.c_uint64),
        ("bfs_multipass_rows", C.c_uint64), ("ms_upload", C.c_double), ("presampled_nodes", C.c_uint64),
        ("stitch_gate_retries", C.c_uint64), ("stitch_regrows", C.c_uint64),
        ("start_discs_known", C.c_uint64), ("map_tie_records", C.c_uint64), ("map_tie_unread", C.c_uint64)]


# every symbol include/trg_engine.h declares (tests check that the library exports all of them)
EXPORTS = [
    "trg_engine_create", "trg_engine_destroy", "trg_engine_last_error", "trg_engine_device_arch",
    "trg_engine_set_global_map", "trg_engine_set_global_map_device", "trg_engine_set_local_map",
    "trg_engine_reset_map", "trg_engine_reset_graph", "trg_engine_init_graph",
    "trg_engine_update_graph", "trg_engine_export_csr", "trg_engine_save_json",
    "trg_engine_load_json", "trg_engine_plan", "trg_engine_refine_path",
    "trg_engine_is_collision_batch", "trg_engine_nearest_z_batch", "trg_engine_edge_risk_batch",
    "trg_engine_is_frontier_batch", "trg_engine_get_stats", "trg_engine_get_sampler_table",
    "trg_engine_debug_map_index", "trg_engine_set_option", "trg_engine_fallback_reason",
    "trg_engine_check_reached", "trg_engine_check_replan", "trg_engine_set_tile",
    "trg_engine_voxel_filter", "trg_engine_plan_batch",
    "trg_engine_stitch_boundary", "trg_engine_stitch_cross", "trg_engine_stitch_assemble",
    "trg_engine_graph_sizes",
    "trg_engine_comm_unique_id", "trg_engine_comm_init", "trg_engine_comm_adopt", "trg_engine_comm_destroy",
    "trg_engine_comm_join_local",
    "trg_engine_stitch_exchange", "trg_engine_cost_field", "trg_engine_cost_field_batch",
    "trg_engine_field_routes", "trg_engine_cost_field_bounded", "trg_engine_field_reached",
    "trg_engine_cost_field_sets", "trg_engine_cost_field_refresh", "trg_engine_cost_field_models",
    "trg_engine_risk_field_sets", "trg_engine_risk_field_refresh",
    "trg_engine_pose_links", "trg_engine_cost_field_seeded",
    "trg_engine_cost_field_zones", "trg_engine_zone_edges", "trg_engine_risk_field_zones",
    "trg_engine_tiled_cost_field", "trg_engine_stitch_ids", "trg_engine_tiled_cost_field_sets",
    "trg_engine_tiled_field_routes", "trg_engine_tiled_risk_field", "trg_engine_tiled_risk_field_sets",
    "trg_engine_tiled_cost_field_bounded", "trg_engine_tiled_risk_field_bounded", "trg_engine_tiled_field_reached",
    "trg_engine_tiled_cost_field_models", "trg_engine_tiled_cost_field_refresh", "trg_engine_tiled_risk_field_refresh",
]

TRG_FIELD_BATCH_MAX = 64  # include/trg_engine.h: fields of one trg_engine_cost_field_batch call
TRG_ZONES_MAX = 256       # include/trg_engine.h: zones of one field of trg_engine_cost_field_zones
# include/trg_engine.h: TRG_FIELD_SETTLE_*
SETTLE_NONE, SETTLE_ANY, SETTLE_ALL = 0, 1, 2
_SETTLE = {None: SETTLE_NONE, "any": SETTLE_ANY, "all": SETTLE_ALL}


def build_library(force=False):
    """Compile csrc/*.hip for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    import glob
    # every source the build reads: a stale library must never pass for the tree's code
    srcs = []
    for pat in ("*.hip", "*.inc", "*.ipp", "*.h", "*.cpp", "*.sh"):
        srcs += glob.glob(os.path.join(CSRC, pat))
    srcs += glob.glob(os.path.normpath(os.path.join(CSRC, "..", "..", "include", "*")))
    stale = force or not os.path.exists(LIB_PATH) or not glob.glob(os.path.join(_HERE, "_trg_pybind*.so"))
    if not stale:
        t = os.path.getmtime(LIB_PATH)
        stale = any(os.path.exists(s) and os.path.getmtime(s) > t for s in srcs)
    if stale:
        subprocess.check_call(["bash", os.path.join(CSRC, "build.sh")])
    return LIB_PATH


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run trg-planner_amd/csrc/build.sh "
                          "(__graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    vp = C.c_void_p
    L.trg_engine_create.argtypes = [C.POINTER(TrgParams), C.c_int, C.POINTER(vp)]
    L.trg_engine_destroy.argtypes = [vp]
    L.trg_engine_destroy.restype = None
    L.trg_engine_last_error.argtypes = [vp]
    L.trg_engine_last_error.restype = C.c_char_p
    L.trg_engine_device_arch.argtypes = [vp]
    L.trg_engine_device_arch.restype = C.c_char_p
    L.trg_engine_set_global_map.argtypes = [vp, fp, C.c_size_t, C.c_size_t]
    L.trg_engine_set_global_map_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    L.trg_engine_set_local_map.argtypes = [vp, fp, fp, C.c_size_t, C.c_size_t]
    L.trg_engine_reset_map.argtypes = [vp, C.c_int]
    L.trg_engine_reset_graph.argtypes = [vp, C.c_int]
    L.trg_engine_init_graph.argtypes = [vp, fp, C.POINTER(TrgSampler)]
    L.trg_engine_update_graph.argtypes = [vp]
    L.trg_engine_export_csr.argtypes = [vp, C.c_int, C.POINTER(TrgCsrView)]
    L.trg_engine_save_json.argtypes = [vp, C.c_char_p]
    L.trg_engine_load_json.argtypes = [vp, C.c_char_p]
    L.trg_engine_plan.argtypes = [vp, fp, fp, fp, C.c_int32, C.POINTER(TrgPathInfo)]
    L.trg_engine_refine_path.argtypes = [fp, C.c_int32, fp, C.c_int32]
    L.trg_engine_refine_path.restype = C.c_int32
    L.trg_engine_plan_batch.argtypes = [vp, fp, fp, C.c_size_t, fp, C.c_int32,
                                        C.POINTER(C.c_int32), C.POINTER(TrgPathInfo)]
    L.trg_engine_voxel_filter.argtypes = [vp, fp, C.c_size_t, C.c_size_t, C.c_float, fp,
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    L.trg_engine_is_collision_batch.argtypes = [vp, C.c_int, C.c_float, fp, C.c_size_t, ip, ip, ip]
    L.trg_engine_nearest_z_batch.argtypes = [vp, C.c_int, fp, C.c_size_t, fp]
    L.trg_engine_edge_risk_batch.argtypes = [vp, C.c_int, fp, fp, C.c_size_t, ip, ip, fp, fp]
    L.trg_engine_is_frontier_batch.argtypes = [vp, fp, C.c_size_t, ip]
    L.trg_engine_get_stats.argtypes = [vp, C.POINTER(TrgStats)]
    L.trg_engine_get_sampler_table.argtypes = [vp, fp, fp]
    L.trg_engine_debug_map_index.argtypes = [vp, C.c_int, fp, fp, fp, ip, ip, fp]
    L.trg_engine_check_reached.argtypes = [vp, fp]
    L.trg_engine_check_reached.restype = C.c_int32
    L.trg_engine_check_replan.argtypes = [vp, fp, fp, C.c_int32]
    L.trg_engine_check_replan.restype = C.c_int32
    L.trg_engine_set_tile.argtypes = [vp, fp, C.c_uint32]
    L.trg_engine_stitch_boundary.argtypes = [vp, fp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, ip]
    L.trg_engine_stitch_cross.argtypes = [vp, C.c_int32, C.c_int32, vp, ip, vp, C.c_int32, ip]
    L.trg_engine_stitch_assemble.argtypes = [vp, C.c_int32, C.c_int32, ip, vp, C.c_int32]
    L.trg_engine_graph_sizes.argtypes = [vp, C.c_int, ip, ip]
    u8p = C.POINTER(C.c_uint8)
    L.trg_engine_comm_unique_id.argtypes = [vp, u8p]
    L.trg_engine_comm_init.argtypes = [vp, u8p, C.c_int32, C.c_int32]
    L.trg_engine_comm_adopt.argtypes = [vp, vp]
    L.trg_engine_comm_destroy.argtypes = [vp]
    L.trg_engine_comm_join_local.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32]
    L.trg_engine_stitch_exchange.argtypes = [vp, fp, C.c_int32, C.c_int32, ip, ip]
    L.trg_engine_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.trg_engine_cost_field.argtypes = [vp, C.c_int32, fp, fp, ip, ip, C.POINTER(TrgFieldInfo)]
    L.trg_engine_cost_field_batch.argtypes = [vp, C.c_int32, ip, fp, fp, ip, ip, ip, C.c_int32, fp, ip, ip, ip,
                                              C.POINTER(TrgFieldInfo)]
    L.trg_engine_field_routes.argtypes = [vp, C.c_int32, ip, ip, ip, ip, fp, C.c_int32, C.POINTER(TrgRouteInfo),
                                          C.POINTER(TrgFieldInfo)]
    L.trg_engine_cost_field_bounded.argtypes = [vp, C.c_int32, ip, fp, fp, C.c_int32, fp, ip, ip, ip, C.c_int32, fp, ip,
                                                ip, ip, fp, C.POINTER(TrgFieldInfo)]
    L.trg_engine_field_reached.argtypes = [vp, C.c_int32, ip, fp, ip, C.c_int32, ip, C.POINTER(TrgFieldInfo)]
    L.trg_engine_cost_field_sets.argtypes = [vp, C.c_int32, ip, ip, fp, C.c_int32, fp, ip, ip, ip, ip, C.c_int32, fp, ip,
                                             ip, ip, ip, fp, C.POINTER(TrgFieldInfo)]
    L.trg_engine_cost_field_models.argtypes = [vp, C.c_int32, C.POINTER(TrgFieldModel), ip, ip, fp, C.c_int32, fp, ip,
                                               ip, ip, ip, C.c_int32, fp, ip, ip, ip, ip, fp, C.POINTER(TrgFieldInfo)]
    L.trg_engine_cost_field_seeded.argtypes = [vp, C.c_int32, C.POINTER(TrgFieldModel), ip, ip, fp, fp, C.c_int32, fp,
                                               ip, ip, ip, ip, C.c_int32, fp, ip, ip, ip, ip, fp,
                                               C.POINTER(TrgFieldInfo)]
    L.trg_engine_cost_field_zones.argtypes = [vp, C.c_int32, C.POINTER(TrgFieldModel), ip, C.POINTER(TrgZone)] + \
        L.trg_engine_cost_field_seeded.argtypes[3:]
    L.trg_engine_zone_edges.argtypes = [vp, C.POINTER(TrgZone), C.c_int32, u8p, u8p, ip, ip]
    L.trg_engine_pose_links.argtypes = [vp, fp, C.c_int32, C.c_float, C.c_int32, ip, fp, fp, C.POINTER(TrgPoseInfo)]
    L.trg_engine_risk_field_sets.argtypes = L.trg_engine_cost_field_sets.argtypes
    L.trg_engine_risk_field_zones.argtypes = [vp, C.c_int32, ip, C.POINTER(TrgZone)] + \
        L.trg_engine_risk_field_sets.argtypes[2:]
    L.trg_engine_cost_field_refresh.argtypes = [vp, ip, C.c_int32, fp, ip, ip, ip, C.c_int32, fp, ip, ip, ip, ip, ip, ip,
                                                C.POINTER(TrgFieldInfo)]
    L.trg_engine_risk_field_refresh.argtypes = L.trg_engine_cost_field_refresh.argtypes
    L.trg_engine_tiled_cost_field.argtypes = [vp, C.c_int32, ip, fp, ip, ip, C.POINTER(TrgTiledFieldInfo)]
    L.trg_engine_stitch_ids.argtypes = [vp, ip, ip, ip]
    L.trg_engine_tiled_cost_field_sets.argtypes = [vp, C.c_int32, ip, ip, fp, fp, ip, ip, ip, ip, C.c_int32, fp, ip, ip,
                                                   ip, C.POINTER(TrgTiledSetInfo)]
    L.trg_engine_tiled_risk_field.argtypes = L.trg_engine_tiled_cost_field.argtypes
    L.trg_engine_tiled_risk_field_sets.argtypes = [vp, C.c_int32, ip, ip, fp, ip, ip, ip, ip, C.c_int32, fp, ip, ip, ip,
                                                   C.POINTER(TrgTiledSetInfo)]
    L.trg_engine_tiled_cost_field_bounded.argtypes = [vp, C.c_int32, ip, ip, fp, C.c_int32, fp, C.c_int32, ip, C.c_int32,
                                                      fp, ip, ip, ip, ip, C.c_int32, fp, ip, ip, ip, fp, ip,
                                                      C.POINTER(TrgTiledSetInfo)]
    L.trg_engine_tiled_risk_field_bounded.argtypes = [vp, C.c_int32, ip, ip, C.c_int32, fp, C.c_int32, ip, C.c_int32,
                                                      fp, ip, ip, ip, ip, C.c_int32, fp, ip, ip, ip, fp, ip,
                                                      C.POINTER(TrgTiledSetInfo)]
    L.trg_engine_tiled_cost_field_models.argtypes = [vp, C.c_int32, C.POINTER(TrgFieldModel)] + \
        L.trg_engine_tiled_cost_field_bounded.argtypes[2:]
    L.trg_engine_tiled_field_reached.argtypes = [vp, C.c_int32, ip, fp, ip, C.c_int32, ip]
    L.trg_engine_tiled_cost_field_refresh.argtypes = [vp, ip, C.c_int32, fp, ip, ip, ip, ip, C.c_int32, fp, ip, ip, ip, ip,
                                                      ip, C.POINTER(TrgTiledRefreshInfo)]
    L.trg_engine_tiled_risk_field_refresh.argtypes = L.trg_engine_tiled_cost_field_refresh.argtypes
    L.trg_engine_tiled_field_routes.argtypes = [vp, C.c_int32, ip, ip, ip, ip, fp, C.c_int32,
                                                C.POINTER(TrgTiledRouteInfo), C.POINTER(TrgTiledRoutesInfo)]
    L.trg_engine_fallback_reason.argtypes = [vp]
    L.trg_engine_fallback_reason.restype = C.c_char_p
    _lib = L
    return L


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def choose_frontier(ids, cost, hops):
    """Of the candidate nodes `ids` with their `cost` and `hops` (arrays of one length): the node of the least
    (cost, hops, id) among those with a finite cost and hops >= 0 -> (node, index into ids), or None if
    there is none."""
    ids = np.asarray(ids)
    cost = np.asarray(cost)
    hops = np.asarray(hops)
    ok = np.flatnonzero(np.isfinite(cost) & (hops >= 0))
    if ok.size == 0:
        return None
    j = int(ok[np.lexsort((ids[ok], hops[ok], cost[ok]))[0]])
    return int(ids[j]), j


def pack_sets(who, sets, start_costs=None, who_starts=None):
    """Source sets as the set entries take them -> (the m int32 arrays, ptr int32 (m + 1), the concatenated int32 ids,
    the m float32 start-cost arrays or None, their concatenation or None).  The ValueErrors name the caller, `who`
    (`who_starts` for the start costs' shape, where another call answers for them)."""
    sets = [np.ascontiguousarray(s, dtype=np.int32).reshape(-1) for s in sets]
    m = len(sets)
    starts, c0 = None, None
    if start_costs is not None:
        starts = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in start_costs]
        if len(starts) != m or any(c.shape != s.shape for c, s in zip(starts, sets)):
            raise ValueError(f"{who_starts or who}: start_costs and sets differ in shape")
        c0 = np.ascontiguousarray(np.concatenate(starts) if m else np.empty(0, np.float32), dtype=np.float32)
    ptr = np.zeros(m + 1, np.int64)
    np.cumsum([s.shape[0] for s in sets], out=ptr[1:])
    if ptr[-1] > 2**31 - 1:
        raise ValueError(f"{who}: {int(ptr[-1])} source entries do not fit 32 bits")
    ids = np.ascontiguousarray(np.concatenate(sets) if m else np.empty(0, np.int32), dtype=np.int32)
    return sets, ptr.astype(np.int32), ids, starts, c0


def _owned_buffer(ptr):
    """A set solve's `owned` over pack_sets' `ptr` -> (the buffer the entry fills, a call that splits it per set)."""
    owned = np.zeros(max(int(ptr[-1]), 1), np.int32)
    return owned, lambda: [owned[ptr[k]:ptr[k + 1]].copy() for k in range(ptr.shape[0] - 1)]


def _as_risk(out):
    """A result dict under the risk fields' names: "risk" / "risk_at" for "cost" / "cost_at"."""
    for old, new in (("cost", "risk"), ("cost_at", "risk_at")):
        if old in out:
            out[new] = out.pop(old)
    return out


def _check_settle(who, settle):
    if settle not in _SETTLE:
        raise ValueError(f"{who}: settle {settle!r} (\"any\", \"all\" or None)")


# The solve the engine retains, as Engine._retain records it: risk -- the objective; fields -- m; sets -- solved through
# a set entry; owners -- a refresh returns "owner" / "owner_at"; single -- one field from a set of one (frontier_ceilings'
# `reuse`); source -- of the last cost_field, for field_path (kept across other solves: the caller holds its parents).
Retained = namedtuple("Retained", "risk fields sets owners single source", defaults=(False, 1, False, False, False, -1))


class CsrGraph:
    """Host copy of a TrgCsrView."""

    def __init__(self, xyz, state, rowptr, col, weight, dist, cid):
        self.xyz, self.state, self.rowptr, self.col = xyz, state, rowptr, col
        self.w, self.dist, self.cid = weight, dist, cid

    @property
    def V(self):
        return int(self.state.shape[0])

    @property
    def E(self):
        return int(self.col.shape[0])


class Engine:
    """One TrgEngine handle."""

    def __init__(self, expand_dist=0.6, robot_size=0.3, sample_num=7, height_threshold=0.16,
                 collision_threshold=0.1, update_collision_threshold=0.5, safety_factor=3.0,
                 goal_tolerance=0.8, is_verbose=False, device=0):
        self.L = load_library()
        self.params = TrgParams(int(is_verbose), expand_dist, robot_size, sample_num,
                                height_threshold, collision_threshold, update_collision_threshold,
                                safety_factor, goal_tolerance)
        self.h = C.c_void_p()
        st = self.L.trg_engine_create(C.byref(self.params), device, C.byref(self.h))
        if st != 0:
            msg = self.L.trg_engine_last_error(self.h).decode() if self.h else "create failed"
            if self.h:
                self.L.trg_engine_destroy(self.h)
                self.h = C.c_void_p()
            raise TrgError(st, msg)
        self.sampler = TrgSampler(1, 16)
        self.last_reuse = None  # frontier_ceilings(reuse=True): the refresh's dict when it was taken
        self._retained = Retained()  # (nothing solved through this object yet: one field, no sets, source -1)
        self._tiled_retained = None  # the last tiled solve made here: (its sets' offsets, whether its owner pass ran)

    def close(self):
        if getattr(self, "h", None):
            self.L.trg_engine_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st):
        if st != 0:
            raise TrgError(st, self.L.trg_engine_last_error(self.h).decode())

    @property
    def arch(self):
        return self.L.trg_engine_device_arch(self.h).decode()

    def set_tile(self, core_xyxy=None, epoch=0):
        """Tiled builds: node creation restricted to [x0,x1) x [y0,y1); sampler epoch of the tile."""
        if core_xyxy is None:
            self._chk(self.L.trg_engine_set_tile(self.h, None, int(epoch)))
        else:
            c = np.ascontiguousarray(core_xyxy, dtype=np.float32)
            self._chk(self.L.trg_engine_set_tile(self.h, _f(c), int(epoch)))

    # ---- tiled builds: boundary stitch (device buffers = torch tensors' data_ptr()) -------------------
    def stitch_boundary(self, core_xyxy, cols, rows, tile, rec_ptr=None, cap=0):
        """Number of boundary nodes; with rec_ptr (device, cap x 16 bytes) also their records."""
        c = np.ascontiguousarray(core_xyxy, dtype=np.float32)
        n = C.c_int32(0)
        self._chk(self.L.trg_engine_stitch_boundary(self.h, _f(c), cols, rows, tile,
                                                    C.c_void_p(rec_ptr or 0), cap, C.byref(n)))
        return n.value

    def stitch_cross(self, tile, ntiles, all_rec_ptr, rec_offsets, edges_ptr=None, cap=0):
        off = np.ascontiguousarray(rec_offsets, dtype=np.int32)
        n = C.c_int32(0)
        self._chk(self.L.trg_engine_stitch_cross(self.h, tile, ntiles, C.c_void_p(all_rec_ptr or 0), _i(off),
                                                 C.c_void_p(edges_ptr or 0), cap, C.byref(n)))
        return n.value

    def stitch_assemble(self, tile, ntiles, node_offsets, all_edges_ptr, n_edges):
        off = np.ascontiguousarray(node_offsets, dtype=np.int32)
        self._chk(self.L.trg_engine_stitch_assemble(self.h, tile, ntiles, _i(off),
                                                    C.c_void_p(all_edges_ptr or 0), n_edges))

    # ---- the native exchange: one call = the whole stitch of this rank's tile over RCCL -------------------
    def comm_unique_id(self):
        """128 bytes one rank draws and hands to every rank (e.g. torch.distributed broadcast)."""
        buf = (C.c_uint8 * 128)()
        self._chk(self.L.trg_engine_comm_unique_id(self.h, buf))
        return bytes(buf)

    def comm_init(self, unique_id, nranks, rank):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self.L.trg_engine_comm_init(self.h, buf, nranks, rank))
        self._comm_ranks = nranks

    def comm_join_local(self, group_name, nranks, rank):
        """Rank `rank` of an in-process group of engines on one device, one thread per engine (tests of the exchange
        with more than one rank; RCCL refuses two ranks on one device)."""
        self._chk(self.L.trg_engine_comm_join_local(self.h, str(group_name).encode(), nranks, rank))
        self._comm_ranks = nranks

    def comm_destroy(self):
        self.L.trg_engine_comm_destroy(self.h)
        self._comm_ranks = 0

    def stitch_exchange(self, core_xyxy, cols, rows):
        """(boundary records of all tiles, cross edges of all tiles); rows: graph('stitched')."""
        c = np.ascontiguousarray(core_xyxy, dtype=np.float32)
        nb, nc = C.c_int32(0), C.c_int32(0)
        self._chk(self.L.trg_engine_stitch_exchange(self.h, _f(c), cols, rows, C.byref(nb), C.byref(nc)))
        return nb.value, nc.value

    # ---- cost fields across tiles ("Cost fields across tiles") ---------------------------
    def global_ids(self):
        """(this tile's first global id, its node count) of the current stitch."""
        first, n, total = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._chk(self.L.trg_engine_stitch_ids(self.h, C.byref(first), C.byref(n), C.byref(total)))
        return int(first.value), int(n.value)

    # (what the cost and the risk calls below share, each keyed by the objective's value name and its C entry or solve)
    def _tiled_ids(self):
        """global_ids(), or (0, 0) where that refuses: the solve itself reports, and announces, that there are no
        current rows."""
        try:
            return self.global_ids()
        except TrgError:
            return 0, 0

    def _tiled_fields(self, value, entry, source_gids, parent):
        """tiled_cost_fields and tiled_risk_fields: `value` names the objective's array ("cost" or "risk"), `entry` is
        its C entry."""
        src = np.ascontiguousarray(source_gids, dtype=np.int32).reshape(-1)
        m = int(src.shape[0])
        offset, V = self._tiled_ids()
        rows = max(m, 1)
        val = np.empty((rows, V), np.float32)
        hops = np.empty((rows, V), np.int32)
        par = np.empty((rows, V), np.int32) if parent else None
        info = TrgTiledFieldInfo()
        self._chk(entry(self.h, m, _i(src), _f(val), _i(hops), None if par is None else _i(par), C.byref(info)))
        self._tiled_retained = (np.arange(m + 1, dtype=np.int32), False)
        return {value: val, "hops": hops, "parent": par, "offset": offset, "info": info}

    def _tiled_fields_from(self, value, entry, who, sets, start_costs, targets, full, parent):
        """tiled_cost_fields_from and tiled_risk_fields_from (`who`): `value` names the objective's arrays (`value` and
        `value`_at), `entry` is its C entry; only the cost entry takes start costs, and only its dict has them."""
        sets, ptr, ids, starts, c0 = pack_sets(who, sets, start_costs)
        m = len(sets)
        offset, V = self._tiled_ids()
        rows = max(m, 1)
        at = value + "_at"
        out = dict(offset=offset, sets=sets)
        if value == "cost":
            out["start_costs"] = starts
        if full:
            out.update({value: np.empty((rows, V), np.float32), "hops": np.empty((rows, V), np.int32),
                        "parent": np.empty((rows, V), np.int32) if parent else None,
                        "owner": np.empty((rows, V), np.int32)})
        tg, n_t = None, 0
        if targets is not None:
            tg = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
            n_t = int(tg.shape[0])
            out.update({at: np.empty((rows, n_t), np.float32), "hops_at": np.empty((rows, n_t), np.int32),
                        "owner_at": np.empty((rows, n_t), np.int32)})
        owned, split_owned = _owned_buffer(ptr)
        info = TrgTiledSetInfo()
        arr = lambda name, conv: None if out.get(name) is None else conv(out[name])  # noqa: E731
        self._chk(entry(
            self.h, m, _i(ptr), _i(ids), *((None if c0 is None else _f(c0),) if value == "cost" else ()),
            arr(value, _f), arr("hops", _i), arr("parent", _i), arr("owner", _i),
            None if tg is None or n_t == 0 else _i(tg), n_t, arr(at, _f), arr("hops_at", _i), arr("owner_at", _i),
            _i(owned), C.byref(info)))
        self._tiled_retained = (ptr, True)
        out["owned"] = split_owned()
        out["info"] = info
        return out

    def _tiled_bounded(self, value, who, sets, start_costs, owners, budget, settle, settle_gids, targets, full, parent,
                       models=None):
        """The bounded tiled entries of either objective (`value`: "cost" or "risk"; DESIGN.md section 7, "Bounded fields
        across tiles"): sets of GLOBAL ids, `owners` as every rank passes it, budget (a value or one per field, None:
        +inf), settle ("any" / "all" / None) over the GLOBAL ids settle_gids.  -> _tiled_fields_from's dict (without
        owners: "owner", "owned" and the targets' reads are absent) plus "bound" (m float32, the same on every rank)
        and "reached" (m int32: THIS tile's nodes within the bound).  With `models` (cost only; as cost_fields takes
        them) the call is trg_engine_tiled_cost_field_models and the dict has "models", the (m, 2) pairs as solved."""
        _check_settle(who, settle)
        sets, ptr, ids, starts, c0 = pack_sets(who, sets, start_costs)
        m = len(sets)
        marr, pairs = (None, None) if models is None else self._models(who, models, m)
        offset, V = self._tiled_ids()
        rows = max(m, 1)
        at = value + "_at"
        out = dict(offset=offset, sets=sets)
        if value == "cost":
            out["start_costs"] = starts
        if full:
            out.update({value: np.empty((rows, V), np.float32), "hops": np.empty((rows, V), np.int32),
                        "parent": np.empty((rows, V), np.int32) if parent else None})
            if owners:
                out["owner"] = np.empty((rows, V), np.int32)
        tg, n_t = None, 0
        if targets is not None and owners:
            tg = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
            n_t = int(tg.shape[0])
            out.update({at: np.empty((rows, n_t), np.float32), "hops_at": np.empty((rows, n_t), np.int32),
                        "owner_at": np.empty((rows, n_t), np.int32)})
        bud = None
        if budget is not None:
            bud = np.ascontiguousarray(np.broadcast_to(np.asarray(budget, dtype=np.float32).reshape(-1), (rows,)))
        sg = np.ascontiguousarray([] if settle_gids is None else settle_gids, dtype=np.int32).reshape(-1)
        out["bound"] = np.empty(rows, np.float32)
        out["reached"] = np.zeros(rows, np.int32)
        owned, split_owned = _owned_buffer(ptr)
        info = TrgTiledSetInfo()
        arr = lambda name, conv: None if out.get(name) is None else conv(out[name])  # noqa: E731
        entry = self.L.trg_engine_tiled_cost_field_bounded if value == "cost" else self.L.trg_engine_tiled_risk_field_bounded
        if models is not None:
            entry = self.L.trg_engine_tiled_cost_field_models
        self._chk(entry(
            self.h, m, *(() if models is None else (marr,)), _i(ptr), _i(ids),
            *((None if c0 is None else _f(c0),) if value == "cost" else ()),
            1 if owners else 0, None if bud is None else _f(bud), _SETTLE[settle], _i(sg) if sg.shape[0] else None,
            int(sg.shape[0]), arr(value, _f), arr("hops", _i), arr("parent", _i), arr("owner", _i),
            None if tg is None or n_t == 0 else _i(tg), n_t, arr(at, _f), arr("hops_at", _i), arr("owner_at", _i),
            _i(owned) if owners else None, _f(out["bound"]), _i(out["reached"]), C.byref(info)))
        self._tiled_retained = (ptr, bool(owners))
        if owners:
            out["owned"] = split_owned()
        if models is not None:
            out["models"] = pairs
        out["info"] = info
        return out

    def _tiled_fields_bounded(self, value, who, source_gids, parent, budget, settle, settle_gids, full=True):
        """The single-source forms under bounds: m sets of one entry through the bounded entry, owners off ->
        _tiled_fields' dict plus "bound" and "reached"."""
        src = np.ascontiguousarray(source_gids, dtype=np.int32).reshape(-1)
        r = self._tiled_bounded(value, who, [[int(g)] for g in src], None, False, budget, settle, settle_gids, None, full,
                                parent)
        out = {"offset": r["offset"], "info": r["info"], "bound": r["bound"], "reached": r["reached"]}
        if full:
            out.update({value: r[value], "hops": r["hops"], "parent": r["parent"]})
        return out

    def _tiled_refresh(self, value, entry, new2old, targets, full, parent):
        """tiled_refresh_fields and tiled_refresh_risk_fields: `value` names the objective's arrays, `entry` is its C
        entry.  The shapes are those of the last tiled solve made through this object (its sets' offsets and whether
        its owner pass ran); without one the entry is called without outputs and answers with its refusal."""
        ptr, owners = self._tiled_retained or (None, False)
        n2o = None if new2old is None else np.ascontiguousarray(new2old, dtype=np.int32).reshape(-1)
        info = TrgTiledRefreshInfo()
        head = (self.h, None if n2o is None else _i(n2o), 0 if n2o is None else int(n2o.shape[0]))
        if ptr is None:
            self._chk(entry(*head, *([None] * 4), None, 0, *([None] * 6), C.byref(info)))
            raise TrgError(1, "tiled refresh: the engine retains a tiled solve that this object did not make")
        m = int(ptr.shape[0]) - 1
        offset, V = self._tiled_ids()
        at = value + "_at"
        out = dict(offset=offset)
        if full:
            out.update({value: np.empty((m, V), np.float32), "hops": np.empty((m, V), np.int32),
                        "parent": np.empty((m, V), np.int32) if parent else None})
            if owners:
                out["owner"] = np.empty((m, V), np.int32)
        tg, n_t = None, 0
        if targets is not None and owners:
            tg = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
            n_t = int(tg.shape[0])
            out.update({at: np.empty((m, n_t), np.float32), "hops_at": np.empty((m, n_t), np.int32),
                        "owner_at": np.empty((m, n_t), np.int32)})
        owned, split_owned = _owned_buffer(ptr)
        gids = np.full(max(int(ptr[-1]), 1), -1, np.int32)
        carried = np.zeros(m, np.int32)
        arr = lambda name, conv: None if out.get(name) is None else conv(out[name])  # noqa: E731
        self._chk(entry(
            *head, arr(value, _f), arr("hops", _i), arr("parent", _i), arr("owner", _i),
            None if tg is None or n_t == 0 else _i(tg), n_t, arr(at, _f), arr("hops_at", _i), arr("owner_at", _i),
            _i(owned) if owners else None, _i(gids), _i(carried), C.byref(info)))
        self._tiled_retained = (ptr, owners)
        if owners:
            out["owned"] = split_owned()
        out["set_gids"] = [gids[ptr[k]:ptr[k + 1]].copy() for k in range(m)]
        out["sets"] = out["set_gids"]
        out["carried"] = carried
        out["info"] = info
        return out

    def tiled_refresh_fields(self, new2old=None, targets=None, full=True, parent=True):
        """Refresh across tiles (trg_engine_tiled_cost_field_refresh; DESIGN.md section 7, "Refresh across tiles"): the
        retained tiled cost solve brought to the current stitch.  A collective call: every rank makes it after any
        number of them changed their tile graph and ALL stitched again, with the ranks and tiles of the solve.
        new2old: for every node of THIS tile's graph now its LOCAL id at the retained solve, -1 for a new node; None
        takes the engine's own map through its update_graph calls.  targets / full / parent: tiled_cost_fields_from's
        (targets, "owner" and "owned" only where the retained solve was a set solve).  -> that call's dict, bit for bit
        what a fresh tiled solve from "set_gids" on the current stitch returns, plus "set_gids" (per set, the members'
        NEW global ids, the same on every rank; also under "sets"), "carried" (m: this tile's nodes that kept a key
        through carry and anchor) and "info" (TrgTiledRefreshInfo).  Bounded, modelled and start-cost solves are not
        refreshed."""
        return self._tiled_refresh("cost", self.L.trg_engine_tiled_cost_field_refresh, new2old, targets, full, parent)

    def tiled_refresh_risk_fields(self, new2old=None, targets=None, full=True, parent=True):
        """tiled_refresh_fields for a retained tiled RISK solve (trg_engine_tiled_risk_field_refresh): its dict with
        "risk" / "risk_at" where that has "cost" / "cost_at"."""
        return self._tiled_refresh("risk", self.L.trg_engine_tiled_risk_field_refresh, new2old, targets, full, parent)

    def tiled_field_reached(self, field=0, cap=None):
        """THIS tile's reached nodes of field `field` of the last tiled solve (trg_engine_tiled_field_reached), compacted
        on the device: local work, no collective.  cap: room for that many nodes (None: a first call for the count,
        then one with exactly enough room; 0: the count alone) -> dict with "gids" (ascending global ids), the
        values under "value", "hops" -- the first min(cap, count) each -- and "count".  tiled.concat_reached joins the
        ranks' lists."""
        n = C.c_int32(0)
        if cap is None or int(cap) == 0:
            self._chk(self.L.trg_engine_tiled_field_reached(self.h, int(field), None, None, None, 0, C.byref(n)))
            if cap is not None or n.value == 0:
                return dict(gids=np.empty(0, np.int32), value=np.empty(0, np.float32), hops=np.empty(0, np.int32),
                            count=int(n.value))
            cap = n.value
        cap = int(cap)
        gids = np.empty(max(cap, 1), np.int32)
        val = np.empty(max(cap, 1), np.float32)
        hops = np.empty(max(cap, 1), np.int32)
        self._chk(self.L.trg_engine_tiled_field_reached(self.h, int(field), _i(gids), _f(val), _i(hops), cap, C.byref(n)))
        k = min(cap, int(n.value))
        return dict(gids=gids[:k], value=val[:k], hops=hops[:k], count=int(n.value))

    def tiled_reachable(self, source_gid, budget):
        """THIS tile's nodes of the global stitched graph within the cost `budget` of the global id `source_gid`: one
        bounded tiled solve without full outputs (a collective call, all ranks alike), then tiled_field_reached's list
        -> its dict; tiled.concat_reached joins the ranks' lists."""
        self._tiled_fields_bounded("cost", "tiled_reachable", [int(source_gid)], False, budget, None, None, full=False)
        return self.tiled_field_reached(0)

    def _tiled_at_frontier(self, member_gids, solve):
        """tiled_assign_frontiers and tiled_frontier_ceilings: solve(sets, targets), the set solve of either objective,
        from the one set `member_gids` read at this tile's Frontier nodes -> (the members, those nodes' global ids,
        the solve's dict)."""
        members = np.ascontiguousarray(member_gids, dtype=np.int32).reshape(-1)
        try:
            frontier = self._frontier_ids()
        except TrgError:
            frontier = np.empty(0, np.int32)  # (the solve reports what is wrong with this tile)
        r = solve([members], frontier)
        return members, (frontier.astype(np.int64) + r["offset"]).astype(np.int32), r

    def _tiled_one_to_many(self, solve, start_gid, goal_gids, early_exit=False):
        """tiled_plan_many and tiled_safest_routes (solve: the single-source solve of either objective) and their
        early-exit forms (solve: its bounded form, which settles "all" over the goals -- nothing beyond the dearest goal
        is relaxed or traded, the routes are the same)."""
        goals = np.ascontiguousarray(goal_gids, dtype=np.int32).reshape(-1)
        if early_exit and goals.shape[0]:
            solve([int(start_gid)], parent=False, settle="all", settle_gids=goals)
        else:
            solve([int(start_gid)], parent=False)
        return self.tiled_routes(np.zeros(goals.shape[0], np.int32), goals)

    def tiled_cost_fields(self, source_gids, parent=True):
        """The cost fields of the global stitched graph from the global ids `source_gids`, for this tile's nodes: a
        collective call, made by every rank of the communicator with the same sources after a stitch.  -> dict with
        cost, hops (m x V_t), parent (global ids; None without `parent`), offset (this tile's first global id) and
        info (TrgTiledFieldInfo).  tiled.concat_fields joins the ranks' results.  Under a budget or settle targets:
        tiled_cost_fields_bounded."""
        return self._tiled_fields("cost", self.L.trg_engine_tiled_cost_field, source_gids, parent)

    def tiled_cost_fields_bounded(self, source_gids, budget=None, settle=None, settle_gids=None, parent=True):
        """tiled_cost_fields under bounds (trg_engine_tiled_cost_field_bounded; DESIGN.md section 7, "Bounded fields
        across tiles"): budget (a cost, or one per field; None: +inf), settle ("any" / "all" / None) over the GLOBAL ids
        settle_gids, every rank alike.  Field k is the full field truncated at min(budget[k], settle_k).  ->
        tiled_cost_fields' dict with "bound" (m, the same on every rank) and "reached" (m: this tile's nodes within the
        bound) as well; its info is a TrgTiledSetInfo.  Without budget and settle the solve is tiled_cost_fields'."""
        return self._tiled_fields_bounded("cost", "tiled_cost_fields_bounded", source_gids, parent, budget, settle,
                                          settle_gids)

    def tiled_cost_fields_from(self, sets, start_costs=None, targets=None, full=True, parent=True):
        """Source sets across tiles (trg_engine_tiled_cost_field_sets; DESIGN.md section 7, "Source sets across tiles"):
        m fields of the global stitched graph in one collective solve, field k from EVERY entry of sets[k] (GLOBAL ids;
        duplicates and Invalid nodes allowed), entry j at start_costs[k][j] (finite, >= 0; None: +0 each).  Every rank
        calls it with the same sets and start costs after a stitch; `targets` (LOCAL ids of this tile), `full` and
        `parent` are this rank's own.  -> dict with "cost", "hops", "parent" (global ids; None without `parent`),
        "owner" (m x V_t) with `full`; "cost_at", "hops_at", "owner_at" (m x n_t) with `targets`; "owned" (a list of m
        int32 arrays: THIS tile's nodes per entry of sets[k]); "offset" (this tile's first global id), "info"
        (TrgTiledSetInfo), "sets" and "start_costs" (the arrays as solved, None without start costs).  An owner is the
        index into sets[k] of the member a node's route starts from, -1 where unreached.  tiled.concat_fields joins
        the ranks' results.  Under a budget or settle targets: tiled_cost_fields_from_bounded."""
        return self._tiled_fields_from("cost", self.L.trg_engine_tiled_cost_field_sets, "tiled_cost_fields_from", sets,
                                       start_costs, targets, full, parent)

    def tiled_cost_fields_from_bounded(self, sets, start_costs=None, budget=None, settle=None, settle_gids=None,
                                       targets=None, full=True, parent=True):
        """tiled_cost_fields_from under bounds: budget / settle / settle_gids as tiled_cost_fields_bounded takes them ->
        tiled_cost_fields_from's dict with "bound" and "reached" as well; a truncated node has owner -1."""
        return self._tiled_bounded("cost", "tiled_cost_fields_from_bounded", sets, start_costs, True, budget, settle,
                                   settle_gids, targets, full, parent)

    def tiled_cost_fields_models(self, sets_or_sources, models, start_costs=None, budget=None, settle=None,
                                 settle_gids=None, targets=None, full=True, parent=True):
        """Cost models across tiles (trg_engine_tiled_cost_field_models; DESIGN.md section 7, "Cost models across
        tiles"): tiled_cost_fields_from_bounded with a cost model per field.  `sets_or_sources`: m sets of GLOBAL ids,
        or a flat list of global ids -- m sets of one.  `models` as cost_fields(models=) takes them, m entries: each
        None (the engine's model), a safety factor (no ceiling) or (safety_factor, max_risk); field k admits the edges
        of G with weight <= max_risk and prices them with its safety factor.  models=None is
        tiled_cost_fields_from_bounded.  Every rank passes the same sets, start costs, bounds and models.  ->
        tiled_cost_fields_from_bounded's dict plus "models", the (m, 2) float32 pairs as solved (absent with
        models=None).  The solve is retained with its models: tiled_routes and tiled_field_reached answer under them."""
        sets = list(sets_or_sources)
        if all(np.ndim(one) == 0 for one in sets):
            sets = [[int(g)] for g in sets]
        if models is not None:  # what the entry refuses on every rank alike, said here before any call
            for k, (s, tau) in enumerate(self._models("tiled_cost_fields_models", models, len(sets))[1]):
                if not s >= 0.0 or np.isinf(s):
                    raise ValueError(f"tiled_cost_fields_models: the safety factor of field {k} is negative or not finite")
                if not tau >= 0.0:
                    raise ValueError(f"tiled_cost_fields_models: the risk ceiling of field {k} is negative or not a number")
        return self._tiled_bounded("cost", "tiled_cost_fields_models", sets, start_costs, True, budget, settle,
                                   settle_gids, targets, full, parent, models=models)

    def tiled_plan_tradeoff(self, start_gid, goal_gid, models, early_exit=True):
        """The same start-to-goal query of the global stitched graph under k cost models (plan_tradeoff across tiles):
        ONE collective solve of k fields from `start_gid`, field k under models[k] -- with `early_exit` settled "any"
        at the goal, so that no field goes on past it -- then one tiled_routes call, all ranks alike -> tiled_routes'
        dict; tiled.join_routes gives route k under model k (empty where model k's ceiling cuts the goal off).  There
        is no tiled min_risk_ceiling: tiled_safest_routes already answers it from one risk solve -- the least ceiling
        under which the goal is reachable is that route's `cost`."""
        models = list(models)
        k = len(models)
        goal = int(goal_gid)
        self.tiled_cost_fields_models([int(start_gid)] * k, models, settle="any" if early_exit else None,
                                      settle_gids=[goal] if early_exit else None, full=False, parent=False)
        return self.tiled_routes(np.arange(k, dtype=np.int32), np.full(k, goal, np.int32))

    def tiled_assign_frontiers(self, member_gids, start_costs=None):
        """Every Frontier node of the global stitched graph to the entry of `member_gids` (GLOBAL ids, e.g. the robots'
        nodes) that reaches it cheapest: a collective call -- one set field across tiles, read at THIS tile's own
        Frontier nodes on the device.  -> per entry (the global ids of this tile's Frontier nodes it owns, ascending;
        pick), pick being choose_frontier's among them as (gid, cost, hops), or None when it owns none here.
        tiled.merge_frontier_picks joins the ranks' answers.  Within a budget: tiled_assign_frontiers_within."""
        return self.tiled_assign_frontiers_within(member_gids, None, start_costs)

    def tiled_assign_frontiers_within(self, member_gids, budget, start_costs=None):
        """tiled_assign_frontiers within the cost `budget` (None: +inf): no Frontier node dearer than it is assigned,
        and nothing beyond it is relaxed or traded."""
        solve = self.tiled_cost_fields_from if budget is None else \
            (lambda sets, starts, **kw: self.tiled_cost_fields_from_bounded(sets, starts, budget=budget, **kw))
        members, gids, r = self._tiled_at_frontier(member_gids, lambda sets, at: solve(
            sets, None if start_costs is None else [start_costs], targets=at, full=False, parent=False))
        cost, hops, owner = r["cost_at"][0], r["hops_at"][0], r["owner_at"][0]
        out = []
        for k in range(members.shape[0]):
            mine = np.flatnonzero(owner == k)
            pick = choose_frontier(gids[mine], cost[mine], hops[mine])
            out.append((gids[mine], None if pick is None else
                        (pick[0], float(cost[mine[pick[1]]]), int(hops[mine[pick[1]]]))))
        return out

    def tiled_routes(self, route_field, target_gids, cap=None, xyz=True):
        """Routes across tiles (trg_engine_tiled_field_routes; DESIGN.md section 7, "Routes across tiles"): route r of the
        last tiled solve runs from the root of field route_field[r] to the node with GLOBAL id target_gids[r], any
        rank's node.  A collective call: every rank makes it with the same arguments.  cap: the room for node ids in
        all (None: a first collective call for the lengths, then one with exactly enough room; 0: infos only).
        -> dict with "offsets" (n + 1) and "infos" (a list of TrgTiledRouteInfo), the same on every rank; "gids" (the
        global ids at THIS rank's own positions, -1 elsewhere; None with cap == 0), "xyz" (positions there, NaN
        elsewhere; None without `xyz` or with cap == 0) and "info" (TrgTiledRoutesInfo of the last call).
        tiled.join_routes merges the ranks' dicts."""
        f = np.ascontiguousarray(route_field, dtype=np.int32).reshape(-1)
        t = np.ascontiguousarray(target_gids, dtype=np.int32).reshape(-1)
        if f.shape[0] != t.shape[0]:
            raise ValueError("tiled_routes: route_field and target_gids differ in length")
        n = f.shape[0]
        infos = (TrgTiledRouteInfo * max(n, 1))()
        off = np.zeros(n + 1, np.int32)
        info = TrgTiledRoutesInfo()
        if cap is None:
            self._chk(self.L.trg_engine_tiled_field_routes(self.h, n, _i(f), _i(t), _i(off), None, None, 0, infos,
                                                           C.byref(info)))
            cap = sum(infos[r].num_nodes for r in range(n))
            if cap > 2**31 - 1:
                raise ValueError(f"tiled_routes: {cap} nodes in all do not fit one call's 32-bit capacity")
        cap = int(cap)
        gids = np.full(max(cap, 1), -1, np.int32) if cap > 0 else None
        pts = np.full((max(cap, 1), 3), np.nan, np.float32) if xyz and cap > 0 else None
        self._chk(self.L.trg_engine_tiled_field_routes(
            self.h, n, _i(f), _i(t), _i(off), None if gids is None else _i(gids), None if pts is None else _f(pts), cap,
            infos, C.byref(info)))
        total = int(off[n])
        one = [TrgTiledRouteInfo(i.num_nodes, i.cost, i.path_length, i.avg_risk, i.root_gid, i.owner)
               for i in infos[:n]]
        return dict(offsets=off, infos=one, gids=None if gids is None else gids[:total],
                    xyz=None if pts is None else pts[:total], info=info)

    def tiled_plan_many(self, start_gid, goal_gids):
        """Paths from one node of the global stitched graph to many: ONE tiled solve from `start_gid` (no parents are
        downloaded) and one tiled_routes call without a capacity -- the lengths first, then the ids -- all
        ranks alike (a collective call) -> tiled_routes' dict; tiled.join_routes gives the routes.  Each path is the
        least fp32 fold of edge costs to its goal (tiled_cost_fields' semantics)."""
        return self._tiled_one_to_many(self.tiled_cost_fields, start_gid, goal_gids)

    def tiled_plan_many_early_exit(self, start_gid, goal_gids):
        """tiled_plan_many whose solve stops at the dearest goal (settle "all" over the goals): the same routes, nothing
        beyond that goal relaxed or traded."""
        return self._tiled_one_to_many(self.tiled_cost_fields_bounded, start_gid, goal_gids, early_exit=True)

    # ---- risk fields across tiles ("Risk fields across tiles") ---------------------------
    def tiled_risk_fields(self, source_gids, parent=True):
        """The risk fields of the global stitched graph from the global ids `source_gids`, for this tile's nodes
        (trg_engine_tiled_risk_field): the least, over all walks, of the greatest edge weight on the walk.  A collective
        call like tiled_cost_fields -> its dict with "risk" where that has "cost".  Under a risk ceiling or settle
        targets: tiled_risk_fields_bounded."""
        return self._tiled_fields("risk", self.L.trg_engine_tiled_risk_field, source_gids, parent)

    def tiled_risk_fields_bounded(self, source_gids, budget=None, settle=None, settle_gids=None, parent=True):
        """tiled_risk_fields under bounds (trg_engine_tiled_risk_field_bounded): tiled_cost_fields_bounded with a risk
        ceiling as the budget -> its dict with "risk" where that has "cost"."""
        return self._tiled_fields_bounded("risk", "tiled_risk_fields_bounded", source_gids, parent, budget, settle,
                                          settle_gids)

    def tiled_risk_fields_from(self, sets, targets=None, full=True, parent=True):
        """Risk fields from source sets across tiles (trg_engine_tiled_risk_field_sets): field k from EVERY entry of
        sets[k] (GLOBAL ids) at risk 0 -- risk solves take no start values.  A collective call like
        tiled_cost_fields_from -> its dict with "risk" / "risk_at" where that has "cost" / "cost_at" and without
        "start_costs".  Under a risk ceiling or settle targets: tiled_risk_fields_from_bounded."""
        return self._tiled_fields_from("risk", self.L.trg_engine_tiled_risk_field_sets, "tiled_risk_fields_from", sets,
                                       None, targets, full, parent)

    def tiled_risk_fields_from_bounded(self, sets, budget=None, settle=None, settle_gids=None, targets=None, full=True,
                                       parent=True):
        """tiled_risk_fields_from under bounds: tiled_cost_fields_from_bounded with a risk ceiling as the budget and
        without start costs."""
        return self._tiled_bounded("risk", "tiled_risk_fields_from_bounded", sets, None, True, budget, settle,
                                   settle_gids, targets, full, parent)

    def tiled_safest_routes(self, start_gid, goal_gids):
        """The safest paths from one node of the global stitched graph to many: ONE tiled risk solve from `start_gid`
        (no parents are downloaded) and one tiled_routes call without a capacity, all ranks alike (a collective call)
        -> tiled_routes' dict; tiled.join_routes gives the routes.  Each route's `cost` is the least worst-edge risk to
        its goal (tiled_risk_fields' semantics)."""
        return self._tiled_one_to_many(self.tiled_risk_fields, start_gid, goal_gids)

    def tiled_safest_routes_early_exit(self, start_gid, goal_gids):
        """tiled_safest_routes whose solve stops at the riskiest goal (settle "all" over the goals): the same routes."""
        return self._tiled_one_to_many(self.tiled_risk_fields_bounded, start_gid, goal_gids, early_exit=True)

    def tiled_frontier_ceilings(self, member_gids):
        """For every Frontier node of THIS tile the least risk ceiling under which the nearest entry of `member_gids`
        (GLOBAL ids, e.g. the robots' nodes) reaches it: a collective call -- one set risk field across tiles, read at
        this tile's Frontier nodes on the device; no array of V_t entries is downloaded.  -> dict with "gids" (this
        tile's Frontier nodes, global ids ascending), "risk" (+inf: unreachable), "hops" (-1), "owner" (the entry of
        member_gids whose tree the node hangs in, -1) and "members" (their number).  tiled.safest_frontier joins the
        ranks' answers.  Under a risk ceiling: tiled_frontier_ceilings_within."""
        return self.tiled_frontier_ceilings_within(member_gids, None)

    def tiled_frontier_ceilings_within(self, member_gids, budget):
        """tiled_frontier_ceilings under the risk ceiling `budget` (None: +inf): a Frontier node above it comes out
        unreachable, and nothing above it is relaxed or traded."""
        solve = self.tiled_risk_fields_from if budget is None else \
            (lambda sets, **kw: self.tiled_risk_fields_from_bounded(sets, budget=budget, **kw))
        members, gids, r = self._tiled_at_frontier(member_gids, lambda sets, at: solve(
            sets, targets=at, full=False, parent=False))
        return dict(gids=gids, risk=r["risk_at"][0], hops=r["hops_at"][0], owner=r["owner_at"][0],
                    members=int(members.shape[0]), info=r["info"])

    def set_option(self, key, value):
        self._chk(self.L.trg_engine_set_option(self.h, str(key).encode(), str(value).encode()))

    @property
    def fallback_reason(self):
        return self.L.trg_engine_fallback_reason(self.h).decode()

    def set_sampler(self, seed=1, table_bits=16):
        self.sampler = TrgSampler(seed, table_bits)

    def set_global_map(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        self._chk(self.L.trg_engine_set_global_map(self.h, _f(xyz), xyz.shape[0], xyz.shape[1]))

    def set_global_map_device(self, data_ptr, n, stride=3):
        """Points already in HBM (e.g. a torch tensor's data_ptr())."""
        self._chk(self.L.trg_engine_set_global_map_device(self.h, C.c_void_p(data_ptr), n, stride))

    def set_local_map(self, start2d, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        s = np.ascontiguousarray(start2d, dtype=np.float32)
        self._chk(self.L.trg_engine_set_local_map(self.h, _f(s), _f(xyz), xyz.shape[0], 3))

    def reset_map(self, kind="global"):
        self._chk(self.L.trg_engine_reset_map(self.h, _KINDS[kind]))

    def reset_graph(self, kind="global"):
        self._chk(self.L.trg_engine_reset_graph(self.h, _KINDS[kind]))

    def init_graph(self, start3d):
        s = np.ascontiguousarray(start3d, dtype=np.float32)
        self._chk(self.L.trg_engine_init_graph(self.h, _f(s), C.byref(self.sampler)))

    def update_graph(self):
        self._chk(self.L.trg_engine_update_graph(self.h))

    def graph(self, kind="global"):
        v = TrgCsrView()
        self._chk(self.L.trg_engine_export_csr(self.h, _KINDS[kind], C.byref(v)))
        V, E = v.num_nodes, v.num_edges

        def arr(ptr, n, dt):
            if n == 0:
                return np.empty(0, dt)
            return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True)

        return CsrGraph(arr(v.node_xyz, 3 * V, np.float32).reshape(V, 3),
                        arr(v.node_state, V, np.int32), arr(v.rowptr, V + 1, np.int32),
                        arr(v.col, E, np.int32), arr(v.weight, E, np.float32),
                        arr(v.dist, E, np.float32), arr(v.creation_id, V, np.int32))

    def graph_sizes(self, kind="global"):
        """(num_nodes, num_edges) without copying the arrays."""
        V, E = C.c_int32(0), C.c_int32(0)
        self._chk(self.L.trg_engine_graph_sizes(self.h, _KINDS[kind], C.byref(V), C.byref(E)))
        return int(V.value), int(E.value)

    def node_xyz(self, kind="global"):
        """(V, 3) float32 node positions only (no edge arrays copied)."""
        v = TrgCsrView()
        self._chk(self.L.trg_engine_export_csr(self.h, _KINDS[kind], C.byref(v)))
        if v.num_nodes == 0:
            return np.zeros((0, 3), np.float32)
        return np.ctypeslib.as_array(v.node_xyz, shape=(3 * v.num_nodes,)).astype(
            np.float32, copy=True).reshape(v.num_nodes, 3)

    def save_json(self, path):
        self._chk(self.L.trg_engine_save_json(self.h, str(path).encode()))

    def load_json(self, path):
        self._chk(self.L.trg_engine_load_json(self.h, str(path).encode()))

    def plan(self, start2d, goal3d, max_points=100000):
        s = np.ascontiguousarray(start2d, dtype=np.float32)
        g = np.ascontiguousarray(goal3d, dtype=np.float32)
        path = np.empty((max_points, 3), np.float32)
        info = TrgPathInfo()
        st = self.L.trg_engine_plan(self.h, _f(s), _f(g), _f(path), max_points, C.byref(info))
        if st == 6:  # TRG_ERR_NOT_FOUND: planSafePath returned false
            return np.empty((0, 3), np.float32), info
        self._chk(st)
        return path[:info.num_points].copy(), info

    def plan_batch(self, starts2d, goals3d, path_cap=200000):
        """m consecutive planSafePath calls in one boundary crossing -> list of (path, info)."""
        s = np.ascontiguousarray(starts2d, dtype=np.float32).reshape(-1, 2)
        g = np.ascontiguousarray(goals3d, dtype=np.float32).reshape(-1, 3)
        m = s.shape[0]
        path = np.empty((path_cap, 3), np.float32)
        off = np.zeros(m + 1, np.int32)
        infos = (TrgPathInfo * max(m, 1))()
        self._chk(self.L.trg_engine_plan_batch(self.h, _f(s), _f(g), m, _f(path), path_cap,
                                               off.ctypes.data_as(C.POINTER(C.c_int32)), infos))
        return [(path[off[k]:off[k + 1]].copy(), infos[k]) for k in range(m)]

    def cost_field(self, source_xy=None, source_id=-1):
        """Least risk cost from one node to every node of the global graph, on the GPU (DESIGN.md
        section 2, "Cost field").  The source is node `source_id`, or, with source_id == -1, the node
        planSafePath starts from for `source_xy`.  -> (cost float32 (+inf: unreachable, or a fold that
        saturated), hops int32 (-1: unreachable), parent int32 (-1 for the source and unreachable nodes),
        TrgFieldInfo)."""
        if source_id == -1 and source_xy is None:
            raise ValueError("cost_field needs source_xy or source_id")
        xy = None if source_xy is None else np.ascontiguousarray(source_xy, dtype=np.float32).reshape(2)
        V, _ = self.graph_sizes("global")
        cost = np.empty(V, np.float32)
        hops = np.empty(V, np.int32)
        parent = np.empty(V, np.int32)
        info = TrgFieldInfo()
        self._chk(self.L.trg_engine_cost_field(self.h, int(source_id), None if xy is None else _f(xy), _f(cost),
                                               _i(hops), _i(parent), C.byref(info)))
        self._retain(risk=False, fields=1, source=int(info.source))
        return cost, hops, parent, info

    def field_path(self, parent, node, source=None):
        """Node ids from the field's source to `node` along `parent` (of cost_field; `source` defaults to the
        source of this engine's last cost_field).  Raises ValueError if `node` is unreachable."""
        if source is None:
            source = self._retained.source
        node = int(node)
        path = [node]
        while path[-1] != source:
            p = int(parent[path[-1]])
            if p < 0 or len(path) > len(parent):
                raise ValueError(f"node {node} is not reachable from the field's source {source}")
            path.append(p)
        return path[::-1]

    def cheapest_frontier(self, source_xy, early_exit=False):
        """The Frontier node that is cheapest to reach from `source_xy`: the least (cost, hops, id) among
        Frontier nodes with a finite cost -> (node, cost, path ids) or None.  early_exit: the same answer from a
        solve that stops once the cheapest Frontier node is settled (cheapest_frontiers' path with one pose)."""
        if early_exit:
            return self.cheapest_frontiers(np.ascontiguousarray(source_xy, dtype=np.float32).reshape(1, 2),
                                           early_exit=True)[0]
        cost, hops, parent, info = self.cost_field(source_xy=source_xy)
        frontier = self._frontier_ids()
        pick = choose_frontier(frontier, cost[frontier], hops[frontier])
        if pick is None:
            return None
        return pick[0], float(cost[pick[0]]), self.field_path(parent, pick[0], int(info.source))

    def _frontier_ids(self):
        """The ids of the global graph's Frontier nodes, ascending (none for an empty graph)."""
        v = TrgCsrView()
        self._chk(self.L.trg_engine_export_csr(self.h, KIND_GLOBAL, C.byref(v)))
        if v.num_nodes == 0:
            return np.empty(0, np.int32)
        return np.flatnonzero(np.ctypeslib.as_array(v.node_state, shape=(v.num_nodes,)) == 1).astype(np.int32)

    def _field_outputs(self, who, m, targets, full, budget, settle, owners=False):
        """What cost_fields, refresh_fields and cost_fields_from (`who`) share: `settle` checked, then the result dict
        with its output arrays -- "cost", "hops", "parent" (and "owner") (m, V) with `full`; "cost_at", "hops_at" (and
        "owner_at") (m, n_t) with `targets`; "reached"; "bound" under budget / settle -- and the C entries' argument
        groups for them, ready to splat, None where an array is not there -> (dict, groups): "full" (cost, hops,
        parent), "at" (targets, n_t, cost_at, hops_at), and the single arguments "owner", "owner_at", "reached",
        "budget" (broadcast to m float32) and "bound"."""
        _check_settle(who, settle)
        V, _ = self.graph_sizes("global")
        out = {}
        if full:
            out["cost"] = np.empty((m, V), np.float32)
            for key in ("hops", "parent") + (("owner",) if owners else ()):
                out[key] = np.empty((m, V), np.int32)
        tg, nt = None, 0
        if targets is not None:
            tg = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
            nt = tg.shape[0]
            out["cost_at"] = np.empty((m, nt), np.float32)
            for key in ("hops_at",) + (("owner_at",) if owners else ()):
                out[key] = np.empty((m, nt), np.int32)
        out["reached"] = np.zeros(max(m, 1), np.int32)  # (m == 0 is refused by the call: no result has that size)
        bud = None
        if budget is not None:
            bud = np.ascontiguousarray(np.broadcast_to(np.asarray(budget, dtype=np.float32).reshape(-1), (m,)))
        if budget is not None or settle is not None:
            out["bound"] = np.empty(max(m, 1), np.float32)

        def arg(key, conv=_i):
            return conv(out[key]) if key in out else None
        groups = {"full": [arg("cost", _f), arg("hops"), arg("parent")],
                  "at": [None if tg is None else _i(tg), nt, arg("cost_at", _f), arg("hops_at")],
                  "owner": arg("owner"), "owner_at": arg("owner_at"), "reached": arg("reached"),
                  "budget": None if bud is None else _f(bud), "bound": arg("bound", _f)}
        return out, groups

    def _retain(self, risk, fields, **more):
        """The record of the retained solve: every solve calls this once its C call has succeeded."""
        self._retained = Retained(risk, fields, source=self._retained.source)._replace(**more)

    def _sources(self, who, sources_xy, source_ids, settle=None):
        """The sources of cost_fields / risk_fields (`who`) checked -> (m, ids int32 or None, xy (m, 2) float32 or
        None).  settle: cost_fields' own, which it has always checked between the two checks made here."""
        if sources_xy is None and source_ids is None:
            raise ValueError(f"{who} needs sources_xy or source_ids")
        _check_settle(who, settle)
        ids = None if source_ids is None else np.ascontiguousarray(source_ids, dtype=np.int32).reshape(-1)
        xy = None if sources_xy is None else np.ascontiguousarray(sources_xy, dtype=np.float32).reshape(-1, 2)
        m = ids.shape[0] if ids is not None else xy.shape[0]
        if ids is not None and xy is not None and xy.shape[0] != m:
            raise ValueError(f"{who}: sources_xy and source_ids differ in length")
        return m, ids, xy

    def _resolve(self, m, ids, xy, nodes):
        """The batch entry's resolve-only call (no solve, see the header): source k's node into nodes[k]."""
        self._chk(self.L.trg_engine_cost_field_batch(self.h, m, None if ids is None else _i(ids),
                                                     None if xy is None else _f(xy), None, None, None, None, 0,
                                                     None, None, _i(nodes), None, None))
        return nodes

    def _models(self, who, models, m):
        """`models` of cost_fields / cost_fields_from as the C entry's array: m entries, each None (the engine's
        model), a safety factor (no ceiling) or (safety_factor, max_risk) -> (TrgFieldModel * m, the (m, 2) float32
        pairs)."""
        models = list(models)
        if len(models) != m:
            raise ValueError(f"{who}: {len(models)} models for {m} fields")
        pairs = np.empty((m, 2), np.float32)
        for k, one in enumerate(models):
            if one is None:
                pairs[k] = self.params.safety_factor, np.inf
            elif np.ndim(one) == 0:
                pairs[k] = one, np.inf
            else:
                pairs[k] = one
        arr = (TrgFieldModel * max(m, 1))()
        for k in range(m):
            arr[k] = TrgFieldModel(float(pairs[k, 0]), float(pairs[k, 1]))
        return arr, pairs

    def cost_fields(self, sources_xy=None, source_ids=None, targets=None, full=True, budget=None, settle=None,
                    models=None):
        """m cost fields in one solve on the GPU (trg_engine_cost_field_batch; each field as cost_field's).
        Field k starts at source_ids[k], or, where source_ids is None or source_ids[k] == -1, at the node
        planSafePath starts from for sources_xy[k].  -> dict: with `full`, the (m, V) arrays "cost", "hops",
        "parent"; with `targets` (node ids), the (m, n_t) arrays "cost_at", "hops_at", read on the device
        (with full=False nothing of V entries is copied back); always "sources" (m resolved nodes), "reached"
        (m counts) and "info" (TrgFieldInfo of the whole solve).
        Bounded fields (trg_engine_cost_field_bounded; DESIGN.md section 2, "Bounded fields"): `budget`, a cost or
        m costs, and `settle`, "any" or "all" over `targets`, truncate field k at bound[k] = min(budget[k], the least
        ("any") or greatest ("all") cost of field k over the targets): every node dearer than the bound comes back
        as unreached, every other node exactly as in the full field, and the solve stops early.  With either
        given the result also has "bound" (m float32).
        Cost models (trg_engine_cost_field_models; DESIGN.md section 2, "Cost models"): `models`, m entries, each
        None (the engine's model), a safety factor, or (safety_factor, max_risk) -- field k prices an edge with its
        own safety factor and uses no edge of weight above max_risk.  The sources are resolved first (no solve), then
        every field runs as a set of one; the result also has "models", the (m, 2) float32 pairs as solved."""
        m, ids, xy = self._sources("cost_fields", sources_xy, source_ids, settle)
        out, a = self._field_outputs("cost_fields", m, targets, full, budget, settle)
        out["sources"] = np.full(m, -1, np.int32)
        out["info"] = info = TrgFieldInfo()
        # the bounded entry's arguments; the batch entry's are these without budget, settle and bound_out
        sources = [self.h, m, None if ids is None else _i(ids), None if xy is None else _f(xy)]
        outputs = [*a["full"], *a["at"], _i(out["sources"]), a["reached"]]
        if models is not None:
            marr, out["models"] = self._models("cost_fields", models, m)
            self._resolve(m, ids, xy, out["sources"])
            ptr = np.arange(m + 1, dtype=np.int32)
            self._chk(self.L.trg_engine_cost_field_models(
                self.h, m, marr, _i(ptr), _i(out["sources"]), a["budget"], _SETTLE[settle], *a["full"], None, *a["at"],
                None, None, a["reached"], a["bound"], C.byref(info)))
        elif "bound" in out:
            self._chk(self.L.trg_engine_cost_field_bounded(*sources, a["budget"], _SETTLE[settle], *outputs, a["bound"],
                                                           C.byref(info)))
        else:
            self._chk(self.L.trg_engine_cost_field_batch(*sources, *outputs, C.byref(info)))
        self._retain(risk=False, fields=m)
        return out

    def refresh_fields(self, new2old=None, targets=None, full=True):
        """The retained solve of an EARLIER graph (cost_field, cost_fields or cost_fields_from before the last
        update_graph calls) brought to the current graph: trg_engine_cost_field_refresh, DESIGN.md section 2,
        "Refresh".  The result is that of a fresh solve from the same sources on the current graph, for work that
        follows what the graph change touched.  new2old: for every node of the current graph its id in the
        retained solve's graph, -1 for a new node; None: the map the engine recorded over its update_graph calls.
        -> cost_fields' dict ("cost", "hops", "parent" (m, V) with `full`; "cost_at", "hops_at" (m, n_t) with
        `targets`; "sources" as ids of the current graph, "reached", "info") plus "carried" (m counts of nodes whose
        old key could be kept as a starting point), and for a retained set solve "owner" / "owner_at".  Afterwards
        routes and field_reached answer from the refreshed solve.  A retained risk solve is refused:
        refresh_risk_fields is its call."""
        return self._refresh(self.L.trg_engine_cost_field_refresh, "refresh_fields", new2old, targets, full)

    def _refresh(self, entry, who, new2old, targets, full):
        """refresh_fields / refresh_risk_fields (`who`) through their C `entry`, the outputs sized from the record of
        the retained solve; without one, or for one of the other objective, the call refuses before it writes."""
        m, owners = self._retained.fields, self._retained.owners
        n2o = None if new2old is None else np.ascontiguousarray(new2old, dtype=np.int32).reshape(-1)
        out, a = self._field_outputs(who, m, targets, full, None, None, owners=owners)
        out["sources"] = np.full(m, -1, np.int32)
        out["carried"] = np.zeros(m, np.int32)
        out["info"] = info = TrgFieldInfo()
        self._chk(entry(self.h, None if n2o is None else _i(n2o), 0 if n2o is None else n2o.shape[0], *a["full"],
                        *a["at"], a["owner"], a["owner_at"], _i(out["sources"]), a["reached"], _i(out["carried"]),
                        C.byref(info)))
        return out

    def field_reached(self, field=0, cap=None, with_info=False):
        """The nodes that field `field` of the last cost_field / cost_fields solve reached, compacted on the GPU
        (trg_engine_field_reached) -> (ids int32 ascending, cost float32, hops int32); nothing of V entries is
        copied back.  cap: at most that many entries (the first, by id); cap == 0 -> the count only, as an int.
        with_info: -> (that, TrgFieldInfo of the call, whose `reached` is the full count)."""
        n = C.c_int32(0)
        info = TrgFieldInfo()
        if cap is None:
            self._chk(self.L.trg_engine_field_reached(self.h, int(field), None, None, None, 0, C.byref(n), None))
            cap = n.value
        elif cap == 0:
            self._chk(self.L.trg_engine_field_reached(self.h, int(field), None, None, None, 0, C.byref(n),
                                                      C.byref(info)))
            return (n.value, info) if with_info else n.value
        ids = np.empty(max(cap, 1), np.int32)
        cost = np.empty(max(cap, 1), np.float32)
        hops = np.empty(max(cap, 1), np.int32)
        self._chk(self.L.trg_engine_field_reached(self.h, int(field), _i(ids), _f(cost), _i(hops), int(cap),
                                                  C.byref(n), C.byref(info)))
        k = min(n.value, int(cap))
        out = (ids[:k].copy(), cost[:k].copy(), hops[:k].copy())
        return (out, info) if with_info else out

    def reachable(self, source_xy, budget, source_id=-1):
        """What can be reached from `source_xy` (or node `source_id`) for at most `budget`: one bounded solve without
        full outputs, then the reached list -> (ids int32 ascending, cost float32, hops int32)."""
        r = self.cost_fields(sources_xy=None if source_xy is None else np.asarray(source_xy, np.float32).reshape(1, 2),
                             source_ids=None if source_id == -1 else [int(source_id)], full=False, budget=budget)
        return self.field_reached(0, cap=max(int(r["reached"][0]), 1))

    def _resolve_nodes(self, xy):
        """The node of every position of `xy` (n, 2), each resolved as cost_field resolves a source: the batch entry's
        resolve-only call (no solve, see the header), in chunks of TRG_FIELD_BATCH_MAX."""
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        nodes = np.empty(xy.shape[0], np.int32)
        for k0 in range(0, xy.shape[0], TRG_FIELD_BATCH_MAX):
            part = xy[k0:k0 + TRG_FIELD_BATCH_MAX]  # (rows of a contiguous array: contiguous themselves)
            self._resolve(part.shape[0], None, part, nodes[k0:k0 + TRG_FIELD_BATCH_MAX])
        return nodes

    def cost_fields_from(self, sets, targets=None, full=True, budget=None, settle=None):
        """m cost fields in one solve, field k from EVERY node of sets[k] (a non-empty list of node ids; duplicates
        and Invalid nodes allowed) at cost 0: trg_engine_cost_field_sets, DESIGN.md section 2, "Source sets".
        -> cost_fields' dict ("cost", "hops", "parent" (m, V) with `full`; "cost_at", "hops_at" (m, n_t) with
        `targets`; "reached", "info", "bound" under budget / settle) plus "owner" (m, V) with `full` and "owner_at"
        with `targets` -- the index into sets[k] of the member a node's route starts from, -1 where unreached --
        "owned" (a list of m int32 arrays: nodes per entry of sets[k]) and "sets" (the m int32 arrays as solved);
        "sources" is every set's first id."""
        return self._cost_fields_from(sets, None, targets, full, budget, settle)

    def cost_fields_from_models(self, sets, models, targets=None, full=True, budget=None, settle=None):
        """cost_fields_from with a cost model per field (trg_engine_cost_field_models; DESIGN.md section 2, "Cost
        models"): `models` as cost_fields', m entries or None.  The result also has "models", the (m, 2) float32 pairs
        as solved."""
        return self._cost_fields_from(sets, models, targets, full, budget, settle)

    def cost_fields_seeded(self, sets, start_costs, targets=None, full=True, budget=None, settle=None, models=None):
        """cost_fields_from with a start cost per set entry (trg_engine_cost_field_seeded; DESIGN.md section 2, "Start
        costs"): start_costs[k][j] is the cost at which entry j of sets[k] starts, a finite number >= 0; None is
        cost_fields_from (every entry at +0).  A member reached cheaper from another one is an ordinary node of the
        field; "owner" names, for a node, the entry its route starts from.  -> cost_fields_from's dict, plus
        "start_costs" (the m float32 arrays as solved) and, with `models`, "models"."""
        return self._cost_fields_from(sets, models, targets, full, budget, settle, start_costs=start_costs)

    @staticmethod
    def _zone_array(who, zones):
        """One zone set -- None, or anything that reads as (Z, 3) float32 rows (x, y, r) -- as a contiguous (Z, 3)
        float32 array."""
        if zones is None:
            return np.empty((0, 3), np.float32)
        a = np.ascontiguousarray(zones, dtype=np.float32)
        if a.size == 0:
            return np.empty((0, 3), np.float32)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{who}: a zone set is a (Z, 3) array of (x, y, r), not of shape {a.shape}")
        return a

    def _zone_sets(self, who, zone_sets, m):
        """`zone_sets` of cost_fields_avoiding -- one (Z, 3) array for all m fields, or a list with one per field (None
        or (0, 3): no zones) -> (the m float32 (Z_k, 3) arrays, ptr int32 (m + 1), their concatenation (n, 3))."""
        per_field = isinstance(zone_sets, (list, tuple)) and len(zone_sets) > 0 and \
            any(z is None or np.ndim(z) == 2 for z in zone_sets)
        if per_field:
            if len(zone_sets) != m:
                raise ValueError(f"{who}: {len(zone_sets)} zone sets for {m} fields")
            each = [self._zone_array(who, z) for z in zone_sets]
        else:
            each = [self._zone_array(who, zone_sets)] * m
        ptr = np.zeros(m + 1, np.int32)
        np.cumsum([z.shape[0] for z in each], out=ptr[1:])
        flat = np.ascontiguousarray(np.concatenate(each) if m else np.empty((0, 3), np.float32), dtype=np.float32)
        return each, ptr, flat

    def closed_edges(self, zones):
        """What a keep-out zone set shuts on the current global graph (trg_engine_zone_edges; DESIGN.md section 2,
        "Keep-out zones"), by the device function the solves use.  `zones`: (Z, 3) rows (x, y, r), Z <= 256; None or
        (0, 3): no zones.  -> dict: "closed" (E,) uint8 per CSR edge, "inside" (V,) uint8 per node, "n_closed",
        "n_inside"."""
        z = self._zone_array("closed_edges", zones)
        V, E = self.graph_sizes("global")
        closed = np.zeros(max(E, 1), np.uint8)
        inside = np.zeros(max(V, 1), np.uint8)
        nc, ni = C.c_int32(0), C.c_int32(0)
        u8 = C.POINTER(C.c_uint8)
        self._chk(self.L.trg_engine_zone_edges(self.h, z.ctypes.data_as(C.POINTER(TrgZone)), z.shape[0],
                                               closed.ctypes.data_as(u8), inside.ctypes.data_as(u8), C.byref(nc),
                                               C.byref(ni)))
        return {"closed": closed[:E], "inside": inside[:V], "n_closed": int(nc.value), "n_inside": int(ni.value)}

    def cost_fields_avoiding(self, sets_or_sources, zone_sets, models=None, start_costs=None, targets=None, full=True,
                             budget=None, settle=None):
        """Cost fields that avoid keep-out zones (trg_engine_cost_field_zones; DESIGN.md section 2, "Keep-out zones"):
        cost_fields_seeded on the graph without the edges that field k's zone set closes -- an edge is closed when a
        disc (x, y, r) of the set touches it, so no walk enters or crosses a zone; the graph itself is left as it is.
        `sets_or_sources`: m sets of node ids, or a flat list of node ids -- m sets of one.  `zone_sets`: one (Z, 3)
        array of (x, y, r) rows for all fields, or a list with one per field; None or (0, 3) means no zones, Z <= 256.
        `models` as cost_fields', `start_costs` as cost_fields_seeded's.  A member inside a zone keeps its key and
        reaches nothing; a target inside a zone is unreached.  -> cost_fields_seeded's dict plus "zones" (the m
        float32 (Z_k, 3) arrays as solved).  The solve is retained with its zones: routes, field_reached and
        refresh_fields answer under them."""
        sets = list(sets_or_sources)
        if all(np.ndim(one) == 0 for one in sets):
            sets = [[int(v)] for v in sets]
        each, zptr, flat = self._zone_sets("cost_fields_avoiding", zone_sets, len(sets))
        out = self._cost_fields_from(sets, models, targets, full, budget, settle, start_costs=start_costs,
                                     zones=(zptr, flat))
        out["zones"] = each
        return out

    def plan_avoiding(self, start_xy, goal_xy, zone_sets, model=None, early_exit=True):
        """The same start-to-goal query under several keep-out zone sets -- the route if A is closed, if B is closed,
        if both are: one field per zone set of `zone_sets` (a list of (Z, 3) arrays; None or (0, 3): no zones) from
        the node planSafePath starts from for `start_xy`, in ONE solve under `model` (None, a safety factor or
        (safety_factor, max_risk)), the goal resolved to a node as plan_many resolves it, the routes walked on the
        device.  early_exit: every field stops once the goal is settled in it (settle "any"); the result is the same.
        More than TRG_FIELD_BATCH_MAX zone sets run in chunks.  -> one dict per zone set: "zones" (Z, 3), "found"
        (False where the zone set cuts the goal off or contains it), "ids" (int32 node ids start .. goal, empty when
        not found), "xyz" (n, 3), "cost" (+inf when not found), "path_length", "avg_risk"."""
        zone_sets = [self._zone_array("plan_avoiding", z) for z in zone_sets]
        start, goal = (int(v) for v in self._resolve_nodes([np.asarray(start_xy, np.float32).reshape(2),
                                                            np.asarray(goal_xy, np.float32).reshape(2)]))
        out = []
        for k0 in range(0, len(zone_sets), TRG_FIELD_BATCH_MAX):
            part = zone_sets[k0:k0 + TRG_FIELD_BATCH_MAX]
            r = self.cost_fields_avoiding([start] * len(part), part, models=None if model is None else [model] * len(part),
                                          targets=[goal], full=False, settle="any" if early_exit else None)
            routes = self.routes(np.arange(len(part)), [goal] * len(part), hops_at=r["hops_at"][:, 0])
            for z, (ids, xyz, one) in zip(part, routes):
                out.append({"zones": z, "found": one.num_nodes > 0, "ids": ids, "xyz": xyz, "cost": float(one.cost),
                            "path_length": float(one.path_length), "avg_risk": float(one.avg_risk)})
        return out

    def _cost_fields_from(self, sets, models, targets, full, budget, settle, start_costs=None, zones=None):
        sets, ptr, ids, starts, c0 = pack_sets("cost_fields_from", sets, start_costs, who_starts="cost_fields_seeded")
        m = len(sets)
        marr, pairs = (None, None) if models is None else self._models("cost_fields_from_models", models, m)
        out, a = self._field_outputs("cost_fields_from", m, targets, full, budget, settle, owners=True)
        owned, split_owned = _owned_buffer(ptr)
        info = TrgFieldInfo()
        tail = [_i(ptr), _i(ids), a["budget"], _SETTLE[settle], *a["full"], a["owner"], *a["at"], a["owner_at"],
                _i(owned), a["reached"], a["bound"], C.byref(info)]
        if zones is not None:  # (zptr int32 (m + 1), the (n, 3) float32 rows)
            self._chk(self.L.trg_engine_cost_field_zones(
                self.h, m, marr, _i(zones[0]), zones[1].ctypes.data_as(C.POINTER(TrgZone)), *tail[:2],
                None if c0 is None else _f(c0), *tail[2:]))
            if c0 is not None:
                out["start_costs"] = starts
            if marr is not None:
                out["models"] = pairs
        elif c0 is not None:
            self._chk(self.L.trg_engine_cost_field_seeded(self.h, m, marr, *tail[:2], _f(c0), *tail[2:]))
            out["start_costs"] = starts
            if marr is not None:
                out["models"] = pairs
        elif marr is None:
            self._chk(self.L.trg_engine_cost_field_sets(self.h, m, *tail))
        else:
            self._chk(self.L.trg_engine_cost_field_models(self.h, m, marr, *tail))
            out["models"] = pairs
        self._retain(risk=False, fields=m, sets=True, owners=True)
        out["owned"] = split_owned()
        out["sets"] = sets
        out["sources"] = np.array([s[0] for s in sets], np.int32)
        out["info"] = info
        return out

    def nearest_source(self, nodes_or_xy, targets=None, budget=None):
        """For every node, the nearest of the given nodes by risk cost: ONE set field from all of them.
        `nodes_or_xy` is a list of node ids or an (n, 2) array of positions (each resolved as cost_field resolves a
        source).  -> (cost float32, hops int32, owner int32, nodes int32): owner[v] is the index into `nodes` of the
        node v's route starts from (the first of equal nodes), -1 where v is unreached or dearer than `budget`; over
        the graph, or, with `targets` (node ids), at the targets only -- nothing of V entries is copied back."""
        a = np.asarray(nodes_or_xy)
        if a.ndim == 1 and np.issubdtype(a.dtype, np.integer):
            nodes = np.ascontiguousarray(a, dtype=np.int32)
        else:
            nodes = self._resolve_nodes(a)
        r = self.cost_fields_from([nodes], targets=targets, full=targets is None, budget=budget)
        if targets is None:
            return r["cost"][0], r["hops"][0], r["owner"][0], nodes
        return r["cost_at"][0], r["hops_at"][0], r["owner_at"][0], nodes

    def assign_frontiers(self, poses, budget=None):
        """Every Frontier node to the pose of `poses` (m, 2) that reaches it cheapest: one set field from the poses'
        nodes read at the Frontier nodes, and one routes call.  -> per pose (Frontier node ids it owns, ascending;
        pick), where pick is choose_frontier over the pose's own Frontier nodes as (node, cost, path ids), or None
        when it owns none.  No two poses get the same node; of two poses that resolve to one node the first owns
        everything.  Without a Frontier node every pose gets (empty, None)."""
        xy = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 2)
        frontier = self._frontier_ids()
        none = np.empty(0, np.int32)
        if frontier.size == 0 or xy.shape[0] == 0:
            return [(none, None) for _ in range(xy.shape[0])]
        r = self.cost_fields_from([self._resolve_nodes(xy)], targets=frontier, full=False, budget=budget)
        cost, hops, owner = r["cost_at"][0], r["hops_at"][0], r["owner_at"][0]
        mine = [np.flatnonzero(owner == k) for k in range(xy.shape[0])]
        picks = [choose_frontier(frontier[j], cost[j], hops[j]) for j in mine]
        chosen = [(k, mine[k][p[1]]) for k, p in enumerate(picks) if p is not None]  # (pose, index into frontier)
        routes = self.routes([0] * len(chosen), [frontier[j] for _, j in chosen], xyz=False,
                             hops_at=[hops[j] for _, j in chosen]) if chosen else []
        paths = {k: ids.tolist() for (k, _), (ids, _, _) in zip(chosen, routes)}
        at = dict(chosen)
        return [(frontier[mine[k]], None if k not in at else (int(frontier[at[k]]), float(cost[at[k]]), paths[k]))
                for k in range(xy.shape[0])]

    def cost_matrix(self, nodes_or_xy, early_exit=False):
        """Least costs between m waypoints -> (cost (m, m) float32, hops (m, m) int32, node ids (m,)): entry
        [a, b] is from waypoint a to waypoint b.  `nodes_or_xy` is a list of node ids or an (m, 2) array of
        positions (each resolved as cost_field resolves a source).  The fields are read at the waypoints on
        the device; more than TRG_FIELD_BATCH_MAX waypoints run in chunks of sources.  early_exit: every field stops
        once all waypoints are settled in it (settle "all"); the result is the same."""
        a = np.asarray(nodes_or_xy)
        if a.ndim == 1 and np.issubdtype(a.dtype, np.integer):
            nodes = np.ascontiguousarray(a, dtype=np.int32)
        else:
            # every chunk's targets are ALL waypoints: resolve the positions first (no solve, see the header)
            nodes = self._resolve_nodes(a)
        m = nodes.shape[0]
        cost = np.empty((m, m), np.float32)
        hops = np.empty((m, m), np.int32)
        for k0 in range(0, m, TRG_FIELD_BATCH_MAX):
            r = self.cost_fields(source_ids=nodes[k0:k0 + TRG_FIELD_BATCH_MAX], targets=nodes, full=False,
                                 settle="all" if early_exit and m else None)
            cost[k0:k0 + TRG_FIELD_BATCH_MAX] = r["cost_at"]
            hops[k0:k0 + TRG_FIELD_BATCH_MAX] = r["hops_at"]
        return cost, hops, nodes

    def cheapest_frontiers(self, poses, early_exit=False):
        """cheapest_frontier for every pose of `poses` (m, 2), from one batch of fields read at the Frontier
        nodes and one routes call for the chosen nodes (nothing of V entries is copied back) -> list of
        (node, cost, path ids) or None, per pose.  early_exit: every field stops once its cheapest Frontier node is
        settled (settle "any": the Frontier nodes of that cost keep their keys, every dearer one reads as
        unreached, and choose_frontier picks among the same least ones); the result is the same."""
        xy = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 2)
        frontier = self._frontier_ids()  # (an empty graph: the batch call says so, as cheapest_frontier's does)
        out = []
        for k0 in range(0, xy.shape[0], TRG_FIELD_BATCH_MAX):
            r = self.cost_fields(sources_xy=xy[k0:k0 + TRG_FIELD_BATCH_MAX], targets=frontier, full=False,
                                 settle="any" if early_exit and frontier.size else None)
            picks = [choose_frontier(frontier, r["cost_at"][k], r["hops_at"][k]) for k in range(r["sources"].shape[0])]
            chosen = [(k, p) for k, p in enumerate(picks) if p is not None]
            routes = self.routes([k for k, _ in chosen], [p[0] for _, p in chosen], xyz=False,
                                 hops_at=[r["hops_at"][k, p[1]] for k, p in chosen]) if chosen else []
            paths = {k: ids.tolist() for (k, _), (ids, _, _) in zip(chosen, routes)}
            for k, pick in enumerate(picks):
                out.append(None if pick is None else (pick[0], float(r["cost_at"][k, pick[1]]), paths[k]))
        return out

    def routes(self, fields, targets, xyz=True, hops_at=None, with_info=False):
        """Paths of the last cost_field / cost_fields solve, walked on the GPU (trg_engine_field_routes; DESIGN.md
        section 2, "Routes"): route r runs from the source of field fields[r] of that solve to node targets[r].
        -> list of (ids int32 (n,), xyz float32 (n, 3) or None, TrgRouteInfo) per route; an unreachable target
        gives empty arrays and num_nodes == 0.  The buffers are sized from `hops_at` (hops of the routes'
        targets, as cost_fields gathers them) when given, else from a first call that returns the lengths only;
        no new solve either way.  with_info: -> (that list, TrgFieldInfo of the last call)."""
        f = np.ascontiguousarray(fields, dtype=np.int32).reshape(-1)
        t = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
        if f.shape[0] != t.shape[0]:
            raise ValueError("routes: fields and targets differ in length")
        n = f.shape[0]
        infos = (TrgRouteInfo * max(n, 1))()
        off = np.zeros(n + 1, np.int32)
        info = TrgFieldInfo()
        if hops_at is not None:
            cap = int((np.asarray(hops_at, np.int64).reshape(-1) + 1).sum())
        else:
            self._chk(self.L.trg_engine_field_routes(self.h, n, _i(f), _i(t), _i(off), None, None, 0, infos,
                                                     C.byref(info)))
            cap = sum(infos[r].num_nodes for r in range(n))
        if cap > 2**31 - 1:
            raise ValueError(f"routes: {cap} nodes in all do not fit one call's 32-bit capacity; ask for fewer routes")
        ids = np.empty(max(cap, 1), np.int32)
        pts = np.empty((max(cap, 1), 3), np.float32) if xyz else None
        self._chk(self.L.trg_engine_field_routes(self.h, n, _i(f), _i(t), _i(off), _i(ids),
                                                 None if pts is None else _f(pts), cap, infos, C.byref(info)))
        out = []
        for r in range(n):
            a, b = int(off[r]), int(off[r + 1])
            one = TrgRouteInfo(infos[r].num_nodes, infos[r].cost, infos[r].path_length, infos[r].avg_risk)
            out.append((ids[a:b].copy(), None if pts is None else pts[a:b].copy(), one))
        return (out, info) if with_info else out

    def plan_many(self, start_xy, goals_xy, early_exit=False):
        """Paths from one start to many goals from ONE cost field: the field from the node planSafePath starts
        from for `start_xy`, every goal of `goals_xy` (n, 2) resolved to a node the same way, one routes call
        -> list of (path xyz float32 (k, 3), TrgRouteInfo) per goal; an unreachable goal gives an empty path and
        num_nodes == 0.  Each path is the least fp32 fold of edge costs to its goal node (cost_field's
        semantics), not planSafePath's A* result.  early_exit: the field stops once every goal node is settled
        (settle "all"); the result is the same."""
        goals = np.ascontiguousarray(goals_xy, dtype=np.float32).reshape(-1, 2)
        start = np.ascontiguousarray(start_xy, dtype=np.float32).reshape(1, 2)
        if not (early_exit and goals.shape[0]):
            self.cost_fields(sources_xy=start, full=False)
        nodes = self._resolve_nodes(goals)
        if early_exit and goals.shape[0]:  # (the goals are the settle targets: resolved first)
            self.cost_fields(sources_xy=start, targets=nodes, full=False, settle="all")
        return [(pts, one) for _, pts, one in self.routes(np.zeros(nodes.shape[0], np.int32), nodes)]

    def _route_record(self, model, ids, xyz, one):
        """One route of plan_tradeoff / min_risk_ceiling as a dict."""
        return {"model": (float(model[0]), float(model[1])), "reachable": one.num_nodes > 0, "ids": ids, "xyz": xyz,
                "cost": float(one.cost), "path_length": float(one.path_length), "avg_risk": float(one.avg_risk)}

    def plan_tradeoff(self, start_xy, goal_xy, models, early_exit=True):
        """The same start-to-goal query under several cost models (each None, a safety factor, or (safety_factor,
        max_risk), as cost_fields'): one field per model from the node planSafePath starts from for `start_xy`, in ONE
        solve, the goal resolved to a node as plan_many resolves it, the routes walked on the device.  early_exit:
        every field stops once the goal is settled in it (settle "any"); the result is the same.  More than
        TRG_FIELD_BATCH_MAX models run in chunks.  -> one dict per model: "model" (safety_factor, max_risk),
        "reachable", "ids" (int32 node ids start .. goal, empty when unreachable), "xyz" (n, 3), "cost" (+inf when
        unreachable), "path_length", "avg_risk"."""
        models = list(models)
        start, goal = (int(v) for v in self._resolve_nodes([np.asarray(start_xy, np.float32).reshape(2),
                                                            np.asarray(goal_xy, np.float32).reshape(2)]))
        out = []
        for k0 in range(0, len(models), TRG_FIELD_BATCH_MAX):
            part = models[k0:k0 + TRG_FIELD_BATCH_MAX]
            r = self.cost_fields(source_ids=[start] * len(part), targets=[goal], full=False,
                                 settle="any" if early_exit else None, models=part)
            routes = self.routes(np.arange(len(part)), [goal] * len(part), hops_at=r["hops_at"][:, 0])
            out += [self._route_record(r["models"][k], *routes[k]) for k in range(len(part))]
        return out

    def min_risk_ceiling(self, start_xy, goal_xy):
        """The minimax ("safest possible") route: the least ceiling among the graph's distinct edge weights (of edges
        into valid nodes) under which the goal is reachable from the start, and the route at that ceiling under the
        engine's safety factor -> (max_risk, route dict as plan_tradeoff's), or None when the goal is unreachable
        without any ceiling.  Reachability is monotone in the ceiling, so the search is exact: every solve tries up to
        TRG_FIELD_BATCH_MAX evenly spaced candidates in one batch (settle "any" at the goal), and the interval between
        the last that fails and the first that succeeds is searched again until it holds one weight.  With goal ==
        start every ceiling succeeds: the least weight (0 for a graph without such an edge)."""
        start, goal = (int(v) for v in self._resolve_nodes([np.asarray(start_xy, np.float32).reshape(2),
                                                            np.asarray(goal_xy, np.float32).reshape(2)]))
        g = self.graph("global")
        ok = (g.col >= 0) & (g.col < g.V)
        ok[ok] = g.state[g.col[ok]] != -1  # TRG_NODE_INVALID
        ws = np.unique(g.w[ok & ~np.isnan(g.w)])
        if ws.size == 0:
            ws = np.zeros(1, np.float32)
        sf = self.params.safety_factor
        lo, hi = -1, None  # the greatest index known to fail, the least known to succeed
        while hi is None or hi - lo > 1:
            top = ws.size - 1 if hi is None else hi - 1
            idx = np.unique(np.rint(np.linspace(lo + 1, top, min(TRG_FIELD_BATCH_MAX, top - lo))).astype(np.int64))
            r = self.cost_fields(source_ids=[start] * idx.size, targets=[goal], full=False, settle="any",
                                 models=[(sf, ws[i]) for i in idx])
            good = np.flatnonzero(r["hops_at"][:, 0] >= 0)
            if good.size == 0:
                if hi is None:
                    return None
                lo = int(idx[-1])
            else:
                j = int(good[0])
                hi = int(idx[j])
                if j > 0:
                    lo = int(idx[j - 1])
        tau = float(ws[hi])
        r = self.cost_fields(source_ids=[start], targets=[goal], full=False, settle="any", models=[(sf, tau)])
        route = self.routes([0], [goal], hops_at=r["hops_at"][:, 0])[0]
        return tau, self._route_record(r["models"][0], *route)

    def risk_fields(self, sources_xy=None, source_ids=None, targets=None, full=True, budget=None, settle=None):
        """m risk fields in one solve on the GPU (trg_engine_risk_field_sets; DESIGN.md section 2, "Risk fields"): for
        every node the least, over all walks from the source, of the greatest edge weight on the walk -- the least risk
        ceiling under which the node can be reached at all -- exactly.  Sources as cost_fields' (resolved first, no
        solve; every field then runs as a set of one).  -> cost_fields' dict with "risk" / "risk_at" where that has
        "cost" / "cost_at": "risk" float32 (+inf: unreachable), "hops" (the BFS depth over tight edges, -1:
        unreachable), "parent" (m, V) with `full`; "risk_at", "hops_at" (m, n_t) with `targets`; "sources", "reached",
        "info".  `budget` is a risk ceiling (a node of greater risk comes back unreached, every other one as in the full
        field), `settle` "any" / "all" lowers it to the least / greatest risk over `targets`; with either the result
        has "bound".  The solve is retained: routes and field_reached answer from it (a route's cost is its target's
        risk); after update_graph calls refresh_risk_fields brings it to the current graph (refresh_fields, the cost
        fields' call, refuses it)."""
        m, ids, xy = self._sources("risk_fields", sources_xy, source_ids)
        nodes = self._resolve(m, ids, xy, np.full(max(m, 1), -1, np.int32))
        # (a set of one owns all it reaches: no owner pass)
        return self._risk_fields_from("risk_fields", [nodes[k:k + 1] for k in range(m)], targets, full, budget, settle,
                                      owners=False)

    def risk_fields_from(self, sets, targets=None, full=True, budget=None, settle=None):
        """m risk fields in one solve, field k from EVERY node of sets[k] at risk 0 (trg_engine_risk_field_sets):
        cost_fields_from's dict with "risk" / "risk_at" where that has "cost" / "cost_at" -- "owner", "owner_at",
        "owned" and "sets" as there, over the (risk, hops) keys."""
        return self._risk_fields_from("risk_fields_from", sets, targets, full, budget, settle, owners=True)

    def _risk_fields_from(self, who, sets, targets, full, budget, settle, owners, zones=None):
        sets, ptr, ids, _, _ = pack_sets(who, sets)
        m = len(sets)
        out, a = self._field_outputs(who, m, targets, full, budget, settle, owners=owners)
        owned, split_owned = _owned_buffer(ptr)
        info = TrgFieldInfo()
        tail = [_i(ptr), _i(ids), a["budget"], _SETTLE[settle], *a["full"], a["owner"], *a["at"], a["owner_at"],
                _i(owned) if owners else None, a["reached"], a["bound"], C.byref(info)]
        if zones is not None:  # (zptr int32 (m + 1) or None: a null zone_ptr, the (n, 3) float32 rows)
            self._chk(self.L.trg_engine_risk_field_zones(self.h, m, None if zones[0] is None else _i(zones[0]),
                                                         zones[1].ctypes.data_as(C.POINTER(TrgZone)), *tail))
        else:
            self._chk(self.L.trg_engine_risk_field_sets(self.h, m, *tail))
        # (`single` is what frontier_ceilings' reuse asks for: a zoned solve, whose refresh stays zoned, is not that)
        self._retain(risk=True, fields=m, sets=True, owners=owners,
                     single=m == 1 and sets[0].shape[0] == 1 and (zones is None or zones[1].shape[0] == 0))
        _as_risk(out)
        if owners:
            out["owned"] = split_owned()
            out["sets"] = sets
        out["sources"] = np.array([s[0] for s in sets], np.int32)
        out["info"] = info
        return out

    def safest_route(self, start_xy, goal_xy):
        """min_risk_ceiling's answer from two solves: one risk field from the start, stopped once the goal is settled
        (its risk there IS the least ceiling under which the goal is reachable), then one cost field under (the
        engine's safety factor, that ceiling) with a routes call -> (max_risk, route dict as plan_tradeoff's), or None
        when the goal is unreachable.  For a goal node other than the start node the result equals
        min_risk_ceiling's bit for bit.  For goal == start the ceiling is 0.0 (no edge has to be crossed;
        min_risk_ceiling names the graph's least weight there) and the route is the one node.  Two more differences:
        on a graph with a NaN, negative or infinite weight this raises TrgError (the risk solve refuses the graph)
        where min_risk_ceiling leaves NaN out and may answer, and a ceiling of zero is always +0.0 here, where
        min_risk_ceiling may name a weight of -0.0 (equal, not the same bits)."""
        start, goal = (int(v) for v in self._resolve_nodes([np.asarray(start_xy, np.float32).reshape(2),
                                                            np.asarray(goal_xy, np.float32).reshape(2)]))
        r = self.risk_fields(source_ids=[start], targets=[goal], full=False, settle="any")
        if r["hops_at"][0, 0] < 0:
            return None
        tau = float(r["risk_at"][0, 0])
        r = self.cost_fields(source_ids=[start], targets=[goal], full=False, settle="any",
                             models=[(self.params.safety_factor, tau)])
        route = self.routes([0], [goal], hops_at=r["hops_at"][:, 0])[0]
        return tau, self._route_record(r["models"][0], *route)

    def risk_fields_avoiding(self, sets_or_sources, zone_sets, targets=None, full=True, budget=None, settle=None):
        """Risk fields that avoid keep-out zones (trg_engine_risk_field_zones; DESIGN.md section 2, "Keep-out zones on
        risk fields"): risk_fields_from on the graph without the edges that field k's zone set closes -- the least
        worst-edge risk of the walks that stay out of the zones; the graph itself is left as it is.  `sets_or_sources`
        and `zone_sets` as cost_fields_avoiding's: m sets of node ids or a flat list of ids; one (Z, 3) array of
        (x, y, r) rows for all fields (they then share one slot of edge risks, the cheap case) or a list with one per
        field; None or (0, 3) means no zones, Z <= 256.  A member inside a zone keeps risk 0 and reaches nothing; a
        target inside a zone is unreached.  -> risk_fields_from's dict plus "zones" (the m float32 (Z_k, 3) arrays as
        solved).  The solve is retained with its zones: routes, field_reached and refresh_risk_fields answer under
        them."""
        return self._risk_fields_avoiding("risk_fields_avoiding", sets_or_sources, zone_sets, targets, full, budget,
                                          settle, owners=True)

    def _risk_fields_avoiding(self, who, sets_or_sources, zone_sets, targets, full, budget, settle, owners):
        """risk_fields_avoiding for `who`; owners=False (sets of one, which own all they reach): no owner pass and no
        owner keys in the dict, as risk_fields has it."""
        sets = list(sets_or_sources)
        if all(np.ndim(one) == 0 for one in sets):
            sets = [[int(v)] for v in sets]
        each, zptr, flat = self._zone_sets(who, zone_sets, len(sets))
        out = self._risk_fields_from(who, sets, targets, full, budget, settle, owners=owners,
                                     zones=(None if zone_sets is None else zptr, flat))
        out["zones"] = each
        return out

    def safest_route_avoiding(self, start_xy, goal_xy, zone_sets):
        """safest_route under several keep-out zone sets -- the safest route if A is closed, if B is closed, if both
        are (`zone_sets`: a list of (Z, 3) arrays; None or (0, 3): no zones): ONE zoned risk solve of one field per zone
        set from the start node, settled at the goal (field k's risk there is its least ceiling), then ONE
        cost_fields_avoiding solve under (the engine's safety factor, that ceiling) and the same zone sets, and one
        routes call.  More than TRG_FIELD_BATCH_MAX zone sets run in chunks.  -> one entry per zone set: (max_risk,
        route dict as plan_tradeoff's), or None where the zone set cuts the goal off or contains it.  With one empty
        zone set the entry equals safest_route's result."""
        zone_sets = [self._zone_array("safest_route_avoiding", z) for z in zone_sets]
        start, goal = (int(v) for v in self._resolve_nodes([np.asarray(start_xy, np.float32).reshape(2),
                                                            np.asarray(goal_xy, np.float32).reshape(2)]))
        out = []
        for k0 in range(0, len(zone_sets), TRG_FIELD_BATCH_MAX):
            part = zone_sets[k0:k0 + TRG_FIELD_BATCH_MAX]
            r = self._risk_fields_avoiding("safest_route_avoiding", [start] * len(part), part, [goal], False, None,
                                           "any", owners=False)
            found = r["hops_at"][:, 0] >= 0
            if not found.any():
                out += [None] * len(part)
                continue
            # (a field that does not reach the goal gets no ceiling: it does not reach it under any)
            taus = [float(t) if ok else np.inf for t, ok in zip(r["risk_at"][:, 0], found)]
            r = self.cost_fields_avoiding([start] * len(part), part, targets=[goal], full=False, settle="any",
                                          models=[(self.params.safety_factor, tau) for tau in taus])
            routes = self.routes(np.arange(len(part)), [goal] * len(part), hops_at=r["hops_at"][:, 0])
            out += [(taus[k], self._route_record(r["models"][k], *routes[k])) if found[k] else None
                    for k in range(len(part))]
        return out

    def frontier_ceilings_avoiding(self, pose_xy, zones):
        """frontier_ceilings under one keep-out zone set (`zones`: (Z, 3) rows (x, y, r); None or (0, 3): no zones): one
        zoned risk field from `pose_xy`, read at the Frontier nodes on the device -> (frontier ids int32 ascending,
        risk float32 (+inf: unreachable or inside a zone), hops int32 (-1 there))."""
        frontier = self._frontier_ids()
        node = int(self._resolve_nodes(np.asarray(pose_xy, np.float32).reshape(1, 2))[0])
        r = self._risk_fields_avoiding("frontier_ceilings_avoiding", [node],
                                       self._zone_array("frontier_ceilings_avoiding", zones), frontier, False, None,
                                       None, owners=False)
        return frontier, r["risk_at"][0], r["hops_at"][0]

    def safest_frontier_avoiding(self, pose_xy, zones):
        """safest_frontier under one keep-out zone set: the least (risk, hops, id) among the Frontier nodes reachable
        without entering a zone, with its route -> (node, risk, path ids), or None without a reachable one."""
        frontier, risk, hops = self.frontier_ceilings_avoiding(pose_xy, zones)
        pick = choose_frontier(frontier, risk, hops)
        if pick is None:
            return None
        ids, _, _ = self.routes([0], [pick[0]], xyz=False, hops_at=[hops[pick[1]]])[0]
        return pick[0], float(risk[pick[1]]), ids.tolist()

    def refresh_risk_fields(self, new2old=None, targets=None, full=True):
        """refresh_fields for a retained RISK solve (risk_fields or risk_fields_from before the last update_graph
        calls): trg_engine_risk_field_refresh, DESIGN.md section 2, "Risk fields".  The result is that of a fresh risk
        solve from the same sources or sets on the current graph, bit for bit.  new2old as refresh_fields'.
        -> refresh_fields' dict with "risk" / "risk_at" where that has "cost" / "cost_at" ("hops", "parent" (m, V) with
        `full`; "hops_at" with `targets`; "sources", "reached", "carried", "info"), and "owner" / "owner_at" only when
        the retained solve came from risk_fields_from.  A retained cost solve is refused (refresh_fields is its call),
        as are a bounded risk solve and one that is already current; a refused call leaves the retained solve answering.
        A NaN, negative or infinite weight on the current graph raises as in risk_fields, and nothing is retained
        afterwards.  Afterwards routes and field_reached answer from the refreshed solve.  A solve of
        risk_fields_avoiding carries its zone sets: the result is the fresh zoned solve's on the current graph, a node
        that the update moved into a zone shut."""
        return _as_risk(self._refresh(self.L.trg_engine_risk_field_refresh, "refresh_risk_fields", new2old, targets,
                                      full))

    def _risk_field_reused(self, node, frontier):
        """frontier_ceilings' `reuse`: the retained risk solve refreshed and read at `frontier`, if it is one field from
        the one node `node` (an id of the current graph) -> refresh_risk_fields' dict, or None: solve afresh.  Whatever
        the refresh refuses (nothing retained, a cost solve, a bounded one, already current, no map) ends here too."""
        if not (self._retained.risk and self._retained.single):
            return None
        try:
            r = self.refresh_risk_fields(targets=frontier, full=False)
        except TrgError:
            return None
        return r if int(r["sources"][0]) == node else None

    def frontier_ceilings(self, pose_xy, reuse=False):
        """For every Frontier node the least risk ceiling under which it can be reached from `pose_xy`: one risk field
        read at the Frontier nodes on the device -> (frontier ids int32 ascending, risk float32 (+inf: unreachable),
        hops int32 (-1: unreachable)); nothing of V entries is copied back.
        reuse: first try to refresh the retained risk solve (refresh_risk_fields) instead of solving -- taken only when
        that solve is one field from one node, that node is the one `pose_xy` resolves to on the current graph, and the
        refresh does not refuse; else the field is solved afresh.  The result is the same bit for bit either way.  It
        pays when the pose still resolves to the same node as at the last call, with update_graph calls in between.
        `last_reuse` is then the refresh's dict ("carried", "info"), None when the field was solved afresh."""
        frontier = self._frontier_ids()
        xy = np.asarray(pose_xy, np.float32).reshape(1, 2)
        self.last_reuse = None
        if reuse:
            self.last_reuse = self._risk_field_reused(int(self._resolve_nodes(xy)[0]), frontier)
        r = self.last_reuse
        if r is None:
            r = self.risk_fields(sources_xy=xy, targets=frontier, full=False)
        return frontier, r["risk_at"][0], r["hops_at"][0]

    def safest_frontier(self, pose_xy, reuse=False):
        """The Frontier node that is safest to reach from `pose_xy`: the least (risk, hops, id) among the reachable
        Frontier nodes, with its route in the minimax tree from one routes call -> (node, risk, path ids), or None
        without a reachable one.  reuse: as frontier_ceilings'."""
        frontier, risk, hops = self.frontier_ceilings(pose_xy, reuse=reuse)
        pick = choose_frontier(frontier, risk, hops)
        if pick is None:
            return None
        ids, _, _ = self.routes([0], [pick[0]], xyz=False, hops_at=[hops[pick[1]]])[0]
        return pick[0], float(risk[pick[1]]), ids.tolist()

    def check_reached(self, pos2d):
        p = np.ascontiguousarray(pos2d, dtype=np.float32)
        return bool(self.L.trg_engine_check_reached(self.h, _f(p)))

    def check_replan(self, pos2d, path):
        p = np.ascontiguousarray(pos2d, dtype=np.float32)
        path = np.ascontiguousarray(path, dtype=np.float32).reshape(-1, 3)
        return bool(self.L.trg_engine_check_replan(self.h, _f(p), _f(path), path.shape[0]))

    def refine_path(self, path):
        path = np.ascontiguousarray(path, dtype=np.float32).reshape(-1, 3)
        out = np.empty((2 * path.shape[0] + 2, 3), np.float32)
        n = self.L.trg_engine_refine_path(_f(path), path.shape[0], _f(out), out.shape[0])
        return out[:n].copy()

    def is_collision(self, xy, kind="global", threshold=None):
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        m = xy.shape[0]
        if threshold is None:
            threshold = self.params.collision_threshold
        flag = np.empty(m, np.int32)
        cnt = np.empty(m, np.int32)
        n = np.empty(m, np.int32)
        self._chk(self.L.trg_engine_is_collision_batch(self.h, _KINDS[kind], threshold, _f(xy), m,
                                                       _i(flag), _i(cnt), _i(n)))
        return flag, cnt, n

    def nearest_z(self, xy, kind="global"):
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        z = np.empty(xy.shape[0], np.float32)
        self._chk(self.L.trg_engine_nearest_z_batch(self.h, _KINDS[kind], _f(xy), xy.shape[0], _f(z)))
        return z

    def edge_risk(self, p1, p2, kind="global"):
        p1 = np.ascontiguousarray(p1, dtype=np.float32).reshape(-1, 3)
        p2 = np.ascontiguousarray(p2, dtype=np.float32).reshape(-1, 3)
        m = p1.shape[0]
        status = np.empty(m, np.int32)
        n_pts = np.empty(m, np.int32)
        w = np.empty(m, np.float32)
        d = np.empty(m, np.float32)
        self._chk(self.L.trg_engine_edge_risk_batch(self.h, _KINDS[kind], _f(p1), _f(p2), m,
                                                    _i(status), _i(n_pts), _f(w), _f(d)))
        return status, n_pts, w, d

    # ---- poses: verified links onto the graph, fields and plans that start from them ------------------------
    def pose_links(self, poses_xy, radius=None, cap=32):
        """The verified links from every position of `poses_xy` (m, 2) to the global graph (trg_engine_pose_links;
        DESIGN.md section 2, "Pose links"): the non-Invalid nodes within `radius` (None: expand_dist, the range of
        expandGraph's step 3) that an edge from a node at the pose would reach -- slope gate, segment collision walk and
        risk weight as wireEdge's.  -> one dict per pose: "status" (1: the pose is in collision and has no links),
        "z" (the elevation addNode would give it), "n_candidates", "n_links" (the full counts) and, for the first `cap`
        links by (dist, node), "nodes" int32, "weight", "dist" and "cost" float32 -- cost is the engine's own edge
        cost, (safety_factor * weight + 1) * dist in fp32."""
        xy = np.ascontiguousarray(poses_xy, dtype=np.float32).reshape(-1, 2)
        m, cap = xy.shape[0], int(cap)
        if radius is None:
            radius = self.params.expand_dist
        room = max(m * max(cap, 0), 1)
        nodes = np.full(room, -1, np.int32)
        w = np.zeros(room, np.float32)
        d = np.zeros(room, np.float32)
        infos = (TrgPoseInfo * max(m, 1))()
        self._chk(self.L.trg_engine_pose_links(self.h, _f(xy), m, C.c_float(radius), cap, _i(nodes), _f(w), _f(d),
                                               infos))
        sf = np.float32(self.params.safety_factor)
        out = []
        for k in range(m):
            n = min(infos[k].n_links, cap)
            a = k * cap
            wk, dk = w[a:a + n].copy(), d[a:a + n].copy()
            out.append({"status": infos[k].status, "z": np.float32(infos[k].z), "n_candidates": infos[k].n_candidates,
                        "n_links": infos[k].n_links, "nodes": nodes[a:a + n].copy(), "weight": wk, "dist": dk,
                        "cost": (sf * wk + np.float32(1)) * dk})
        return out

    def cost_fields_from_poses(self, poses_xy, radius=None, targets=None, full=True, budget=None, settle=None):
        """m cost fields in one solve, field k from the pose poses_xy[k] itself: its link nodes (pose_links) are the
        set, the link costs the start costs, so the field is the exact cost from the pose over the verified links and
        the graph.  -> cost_fields_seeded's dict plus "links" (pose_links' records); "owner" is the index of the link
        a node's route enters the graph by.  A pose in collision or without links raises TrgError(INVALID_ARG) naming
        it: the caller decides whether to fall back to the snapped node (cost_fields)."""
        links = self.pose_links(poses_xy, radius)
        for k, one in enumerate(links):
            if one["status"] != 0:
                raise TrgError(1, f"cost_fields_from_poses: pose {k} is in collision")
            if one["nodes"].size == 0:
                raise TrgError(1, f"cost_fields_from_poses: pose {k} has no links to the graph")
        r = self.cost_fields_seeded([one["nodes"] for one in links], [one["cost"] for one in links], targets=targets,
                                    full=full, budget=budget, settle=settle)
        r["links"] = links
        return r

    def plan_anchored(self, start_xy, goal_xy, radius=None):
        """A least-cost path between two POSITIONS over verified links: both poses' links from one pose_links call, one
        seeded solve from the start's links that stops once every goal link node is settled, the field read at those
        nodes on the device, and one routes call.  Goal link j, from the goal pose to node b_j at link cost c_j (a goal
        link is evaluated from the goal pose, like any other), ends a path of key (fl(cost[b_j] + c_j), hops[b_j] + 1);
        the least key wins, the earlier link on a tie.  -> dict: "found"; "cost", the winning key's cost; "node_ids";
        "path" float32 (n + 2, 3): the start pose's xyz, the route's, the goal pose's; "start_link" and "goal_link" as
        (node, weight, dist); "num_nodes", "path_length" and "avg_risk" of the route (graph nodes and edges only);
        "info", the solve's TrgFieldInfo.
        found is False when either pose has no links or no goal link node is reached.  There is no direct
        pose-to-pose segment: two poses that see each other still go through a node."""
        xy = np.ascontiguousarray([start_xy, goal_xy], dtype=np.float32).reshape(2, 2)
        start, goal = self.pose_links(xy, radius)
        none = {"found": False, "cost": float("inf"), "node_ids": np.empty(0, np.int32),
                "path": np.empty((0, 3), np.float32), "start_link": None, "goal_link": None, "num_nodes": 0,
                "path_length": 0.0, "avg_risk": 0.0}
        if start["nodes"].size == 0 or goal["nodes"].size == 0:
            return none
        r = self.cost_fields_seeded([start["nodes"]], [start["cost"]], targets=goal["nodes"], full=False, settle="all")
        cost, hops = r["cost_at"][0], r["hops_at"][0]
        ok = np.flatnonzero(hops >= 0)
        if ok.size == 0:
            return none
        total = cost[ok] + goal["cost"][ok]  # (float32 + float32: one rounded add)
        j = int(ok[np.lexsort((ok, hops[ok], total))[0]])
        b = int(goal["nodes"][j])
        (ids, pts, one), = self.routes([0], [b], hops_at=[hops[j]])
        i = int(r["owner_at"][0][j])  # (the start link the route enters the graph by)
        path = np.concatenate([[[xy[0, 0], xy[0, 1], start["z"]]], pts, [[xy[1, 0], xy[1, 1], goal["z"]]]])
        return {"found": True, "cost": float(cost[j] + goal["cost"][j]), "node_ids": ids,
                "path": path.astype(np.float32),
                "start_link": (int(start["nodes"][i]), float(start["weight"][i]), float(start["dist"][i])),
                "goal_link": (b, float(goal["weight"][j]), float(goal["dist"][j])),
                "num_nodes": one.num_nodes, "path_length": float(one.path_length), "avg_risk": float(one.avg_risk),
                "info": r["info"]}

    def voxel_filter(self, xyz, leaf):
        """pcl::VoxelGrid of TRGPlanner::loadPrebuiltMap (trg_planner.cpp:91-94) on the GPU.  `xyz` is (N, k) with
        k >= 3 (columns past z, such as a PCD intensity, are skipped: the row stride is k floats) or a flat array of
        3 N floats; -> float32 (n_out, 3)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        if xyz.ndim == 1:
            if xyz.size % 3:
                raise ValueError(f"voxel_filter: a flat cloud holds x y z triples, not {xyz.size} floats")
            xyz = xyz.reshape(-1, 3)
        if xyz.ndim != 2 or xyz.shape[1] < 3:
            raise ValueError(f"voxel_filter: the cloud must be (N, k) with k >= 3, not {xyz.shape}")
        n, stride = xyz.shape
        out = np.empty((n, 3), np.float32)
        n_out = C.c_size_t(0)
        passthrough = C.c_int32(0)
        self._chk(self.L.trg_engine_voxel_filter(self.h, _f(xyz), n, stride, C.c_float(leaf),
                                                 _f(out), C.byref(n_out), C.byref(passthrough)))
        return out[:n_out.value].copy()

    def is_frontier(self, xy):
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        flag = np.empty(xy.shape[0], np.int32)
        self._chk(self.L.trg_engine_is_frontier_batch(self.h, _f(xy), xy.shape[0], _i(flag)))
        return flag

    def stats(self):
        s = TrgStats()
        self._chk(self.L.trg_engine_get_stats(self.h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in TrgStats._fields_}

    def sampler_table(self):
        n = 1 << self.sampler.table_bits
        c = np.empty(n, np.float32)
        s = np.empty(n, np.float32)
        self._chk(self.L.trg_engine_get_sampler_table(self.h, _f(c), _f(s)))
        return c, s

    def map_index(self, kind="global", n=None):
        wh = np.zeros(2, np.int32)
        org = np.zeros(3, np.float32)
        self._chk(self.L.trg_engine_debug_map_index(self.h, _KINDS[kind], None, None, None, None,
                                                    _i(wh), _f(org)))
        if n is None:
            return wh, org
        x = np.empty(n, np.float32)
        y = np.empty(n, np.float32)
        z = np.empty(n, np.float32)
        p = np.empty(n, np.int32)
        self._chk(self.L.trg_engine_debug_map_index(self.h, _KINDS[kind], _f(x), _f(y), _f(z),
                                                    _i(p), _i(wh), _f(org)))
        return x, y, z, p, wh, org
