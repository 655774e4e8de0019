/*
 * include/trg_engine.h -- C ABI of the MI355X-native Traversal-Risk-Graph construction engine.
 *
 * This is the drop-in boundary for the one hot path this repository accelerates: everything the
 * reference's `class TRG` does between "here is a point-cloud map" and "here is the graph"
 * (reference: cpp/trg_planner/core/trg_planner/include/graph/trg.h:50-98 and
 * src/graph/trg.cpp).  Plain pointers and sizes only; no C++/torch types; no exceptions cross
 * the boundary; every call returns a TrgStatus and trg_engine_last_error() explains failures.
 * A failure inside the library itself (host memory exhausted, a thread or a stream that cannot be
 * made) comes back the same way: TRG_ERR_CAPACITY "<call>: out of host memory", or TRG_ERR_DEVICE
 * with the cause.  After such a status, as after any failed HIP call in the middle of a build or an
 * update, trg_engine_last_error explains it and trg_engine_destroy, trg_engine_reset_graph and
 * trg_engine_init_graph are safe; the graph of the call that failed mid-way is unspecified until
 * one of those.  (The three entries that answer with a number -- check_reached, check_replan,
 * refine_path -- answer 0.)
 *
 * Each entry point cites the reference interface it replaces.  The C++ `TRG`/`TRGPlanner`
 * shims, the Python mirror (trg-planner_amd/trg_planner) and the reference-side binding shown
 * in INTEGRATION.md are thin layers over exactly these symbols.
 *
 * Threading: like the reference (every entry is taken under TRG::mtx.graph, trg.cpp:37,196,458,610)
 * an engine must be entered from one thread at a time; one HIP stream set per engine.
 */
#ifndef TRG_ENGINE_H_
#define TRG_ENGINE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct TrgEngine TrgEngine;

typedef enum TrgStatus {
  TRG_OK = 0,
  TRG_ERR_INVALID_ARG = 1,
  TRG_ERR_NO_MAP = 2,        /* reference: assert "Map is empty", trg.cpp:42 */
  TRG_ERR_NO_ROOT = 3,       /* reference: "Failed to generate root node" + exit(1), trg.cpp:49-52 */
  TRG_ERR_DEVICE = 4,        /* HIP runtime error, no GPU, wrong architecture */
  TRG_ERR_NO_GRAPH = 5,
  TRG_ERR_NOT_FOUND = 6,     /* planSafePath returned false, trg.cpp:689 */
  TRG_ERR_IO = 7,
  TRG_ERR_CAPACITY = 8
} TrgStatus;

/* Graph / map selector: reference trgMap_ keys "global" / "local" (trg.h:113-119).
 * TRG_KIND_PRECLEAN is build-side instrumentation: the global graph as it stood right before
 * the last cleanGraph(), ids == creation order (used by the parity tests). */
typedef enum TrgKind {
  TRG_KIND_GLOBAL = 0,
  TRG_KIND_LOCAL = 1,
  TRG_KIND_PRECLEAN = 2,
  TRG_KIND_STITCHED = 3 /* tiled builds: this tile's rows of the stitched global graph (global ids) */
} TrgKind;

/* Node states: reference TRG::NodeState, trg.h:27-31 */
enum { TRG_NODE_VALID = 0, TRG_NODE_INVALID = -1, TRG_NODE_FRONTIER = 1 };

/* Constructor arguments of reference TRG::TRG, trg.h:51-59 / trg.cpp:11-34 (same order). */
typedef struct TrgParams {
  int32_t is_verbose;
  float expand_dist;
  float robot_size;
  int32_t sample_num;
  float height_threshold;
  float collision_threshold;
  float update_collision_threshold;
  float safety_factor;
  float goal_tolerance;
} TrgParams;

/* The reference seeds std::mt19937 from std::random_device (trg.cpp:20), so it has no canonical
 * sample stream; here the sampler is an explicit input.  Direction of trial t of the expansion
 * of node id in build epoch e = table[hash(seed, e, id, t) >> (32 - table_bits)], table[k] =
 * (cosf, sinf)((float)(k / 2^bits * 2 * M_PI)) computed once with the host libm (same values the
 * reference's `distr_(gen_) * 2 * M_PI` -> cos/sin would give for that draw, trg.cpp:395-397). */
typedef struct TrgSampler {
  uint32_t seed;
  int32_t table_bits; /* 2..20 (out of range: 16); few bits = few directions: degenerate, tie-rich graphs for tests */
} TrgSampler;

/* Read-only view of a built graph in CSR form (host memory owned by the engine, valid until the
 * next call that mutates that graph).  Replaces the std::unordered_map<int, Node*> the reference
 * hands out (TRG::getGraph / getGraphCopy, trg.cpp:805-824): row i is the node with id_ == i,
 * col/weight/dist are that node's edges_ in order (Edge{dst_id_, weight_, dist_}, trg.h:20-25). */
typedef struct TrgCsrView {
  int32_t num_nodes;
  int32_t num_edges;        /* directed edges = CSR nnz */
  const float *node_xyz;    /* num_nodes x 3, Node::pos_ */
  const int32_t *node_state;/* num_nodes, Node::state_ */
  const int32_t *rowptr;    /* num_nodes + 1 */
  const int32_t *col;       /* num_edges, Edge::dst_id_ */
  const float *weight;      /* num_edges, Edge::weight_ */
  const float *dist;        /* num_edges, Edge::dist_ */
  const int32_t *creation_id; /* num_nodes: index of the node among all nodes created since the last build began
                               * (the nodes updates create count on; the index of a dropped node is not reused) */
} TrgCsrView;

/* Output of trg_engine_plan: reference TRG::planSafePath out-params (trg.cpp:603-608). */
typedef struct TrgPathInfo {
  float direct_dist;
  float path_length;
  float avg_risk;
  int32_t num_points;
} TrgPathInfo;

/* Counters and timers of the last build (instrumentation; bench.py's roofline uses them). */
typedef struct TrgStats {
  uint64_t map_points;
  uint64_t expanded_nodes;     /* nodes popped from the BFS queue */
  uint64_t trials;             /* sample draws */
  uint64_t samples;            /* accepted samples */
  uint64_t created_nodes;
  uint64_t invalid_nodes;
  uint64_t edge_calls;         /* wireEdge() calls replayed */
  uint64_t edge_evals_gpu;     /* edge evaluations executed on the GPU (speculative ones included) */
  uint64_t nn_ties;            /* exact fp32 distance ties between nearest-NODE candidates; resolved
                                  exactly (reference kd-tree traversal order, host_index.h) */
  uint64_t gate_uncertain;     /* slope gates decided by host libm atan2f */
  uint64_t sync_batches;       /* synchronous GPU round trips forced by the replay */
  /* bytes of map points inside query radii that the GPU kernels touched (12 B per hit) */
  uint64_t bytes_sample_kernel;   /* sampling discs: k_level_sample (device BFS) / k_sample_nodes */
  uint64_t bytes_spec_kernel;     /* speculative parent edges: k_level_spec / k_spec_edges */
  uint64_t bytes_edge_kernel;     /* deferred wireEdge evaluations: k_calls_gather / k_edges */
  uint64_t bytes_index_build;
  /* device time per kernel, milliseconds, measured with hipEvents on the launch stream.  Inside the
   * device-resident BFS k_level_sample + k_level_spec are timed TOGETHER on every 8th level only (an
   * event pair costs ~12 us of stream time per level), reported as ms_sample_kernel /
   * launches_sample_kernel (ms_spec_kernel stays 0) and scaled by launches / timed launches; the
   * deferred edge evaluations are timed in full. */
  double ms_index_build;
  double ms_sample_kernel;
  double ms_spec_kernel;
  double ms_edge_kernel;
  uint64_t launches_sample_kernel;
  uint64_t launches_spec_kernel;
  uint64_t launches_edge_kernel;
  /* host wall time, milliseconds */
  double ms_set_map_total;
  double ms_init_graph_total;
  double ms_replay_host;
  double ms_finalize_host;
  double ms_wait_gpu;
  uint64_t bfs_levels;         /* BFS depth of the last build (device-resident path) */
  uint64_t used_device_bfs;    /* 1: BFS + CSR ran on the GPU; 0: host replay */
  uint64_t bfs_fallbacks;      /* device path declined and the host replay redid the build */
  uint64_t bfs_max_spin;       /* longest dependency wait (poll iterations) in k_level_resolve */
  uint64_t bfs_host_levels;    /* BFS levels replayed on the host because of an exact distance tie */
  uint64_t map_nn_ties;        /* nearest-map-point queries (trial discs and elevation lookups,
                                  trg.cpp:244-247) that met two MAP points at exactly the same fp32
                                  distance (~2e-7 per query) */
  double ms_bfs_loop;          /* device path: wall time of the level loop */
  double ms_deferred;          /* device path: wall time of the deferred edge evaluations */
  uint64_t map_nn_resolved;    /* of those, the ones an accepted sample / addNode depended on: decided
                                  in the reference's map-tree visiting order (kdtree.c:303-362) */
  uint64_t map_nn_unresolved;  /* always 0: every tie is decided, however many points tie and however many
                                  samples of a launch do (the field keeps its place in the struct) */
  uint64_t bfs_tie_fixups;     /* BFS levels whose only trouble was a distance tie among nodes that existed
                                  before the level: the reference's winner was handed to the device and
                                  resolve + commit ran again (no host replay) */
  uint64_t bytes_spec_created; /* device path: the part of bytes_spec_kernel spent on the parent edges of
                                  the nodes that were created -- the wireEdge(node, new_node) calls the
                                  reference itself evaluates (trg.cpp:425); the rest of
                                  bytes_spec_kernel is speculation on candidates that merged */
  double ms_rare_events;       /* device path: wall time inside the level loop spent repairing rare events
                                  (map-point ties, uncertain slope gates, node ties, host level replays) */
  uint64_t bfs_ticket_reruns;  /* device path: resolve launches repeated with start tickets as workgroup indices
                                  after a bounded inter-workgroup wait ran out */
  uint64_t bfs_multipass_rows; /* device path: sample slots whose blockers did not fit one row (taken in passes) */
  double ms_upload;            /* host cloud -> HBM of the last setGlobalMap / setLocalMap from a host pointer */
  uint64_t presampled_nodes;   /* always 0: the variant that drew samples inside the previous level's resolve
                                  launch was removed; the field keeps the struct's layout */
  uint64_t stitch_gate_retries; /* trg_engine_stitch_cross calls that ran their edge selection a second time, after the
                                  host's libm decided slope gates the device could not call */
  uint64_t stitch_regrows;     /* trg_engine_stitch_exchange: times a record or edge buffer was too small and grew */
  uint64_t start_discs_known;  /* device path: edge evaluations (of edge_evals_gpu) that did not evaluate the first disc
                                  of their segment walk: it is the start node's own acceptance disc, whose outcome
                                  and point count the sampling kept (option "known_start_disc") */
  uint64_t map_tie_records;    /* device path: map-point tie records of accepted samples the level loop looked at */
  uint64_t map_tie_unread;     /* of those, the ones left at "lowest cloud index" without a lookup because nothing
                                  reads the sample's elevation: the sample created no node (option "lazy_tie_repair") */
} TrgStats;

/* ---- lifetime ------------------------------------------------------------------------------- */
/* reference: TRG::TRG(...) trg.cpp:11-34.  device = HIP device ordinal.  On failure *out is an engine that
 * explains it (trg_engine_last_error) and is to be destroyed, or NULL where not even that could be made
 * (TRG_ERR_CAPACITY). */
TrgStatus trg_engine_create(const TrgParams *params, int device, TrgEngine **out);
void trg_engine_destroy(TrgEngine *e);
const char *trg_engine_last_error(const TrgEngine *e);
/* "gfx950" etc. of the device the engine runs on */
const char *trg_engine_device_arch(const TrgEngine *e);

/* ---- map ingest ------------------------------------------------------------------------------ */
/* reference: TRG::setGlobalMap(PointCloudPtr&) trg.cpp:179-193 (the kd_insert2 loop becomes the
 * cell-sorted SoA index build on the GPU).  xyz: n points, `stride` floats apart (3 for packed
 * xyz, 4 for pcl::PointXYZ). */
TrgStatus trg_engine_set_global_map(TrgEngine *e, const float *xyz, size_t n, size_t stride);
/* same, points already resident in device memory (HBM) */
TrgStatus trg_engine_set_global_map_device(TrgEngine *e, const float *d_xyz, size_t n, size_t stride);
/* reference: TRG::setLocalMap(Vector2f start2d, PointCloudPtr&) trg.cpp:195-209 (also refreshes
 * the local graph membership, trg.cpp:211-231) */
TrgStatus trg_engine_set_local_map(TrgEngine *e, const float start_xy[2], const float *xyz, size_t n,
                                   size_t stride);
/* reference: TRG::resetMap / TRG::resetGraph, trg.cpp:732-744 */
TrgStatus trg_engine_reset_map(TrgEngine *e, TrgKind kind);
TrgStatus trg_engine_reset_graph(TrgEngine *e, TrgKind kind);

/* ---- graph build ----------------------------------------------------------------------------- */
/* reference: TRG::initGraph(bool isPreMap, Vector3f start3d) trg.cpp:36-64
 * (root seeding -> expandGraph :372-454 -> cleanGraph(false) :491-535). */
TrgStatus trg_engine_init_graph(TrgEngine *e, const float start_xyz[3], const TrgSampler *sampler);
/* reference: TRG::updateGraph() trg.cpp:456-489 */
TrgStatus trg_engine_update_graph(TrgEngine *e);

/* ---- export ---------------------------------------------------------------------------------- */
/* reference: TRG::getGraph / getGraphCopy trg.cpp:805-824 */
TrgStatus trg_engine_export_csr(TrgEngine *e, TrgKind kind, TrgCsrView *out);
/* node / directed-edge counts of a graph without touching (or, for TRG_KIND_STITCHED, fetching) its arrays */
TrgStatus trg_engine_graph_sizes(TrgEngine *e, TrgKind kind, int32_t *num_nodes, int32_t *num_edges);
/* reference: TRG::saveGraph / loadPrebuiltGraph trg.cpp:66-177 (same JSON schema) */
TrgStatus trg_engine_save_json(TrgEngine *e, const char *path);
TrgStatus trg_engine_load_json(TrgEngine *e, const char *path);

/* ---- query (host A*, consumes the CSR) ------------------------------------------------------- */
/* reference: TRG::planSafePath trg.cpp:603-690 (+ setGoal :537-565).  path_xyz receives up to
 * max_points x 3 floats; info->num_points is the full length. */
TrgStatus trg_engine_plan(TrgEngine *e, const float start_xy[2], const float goal_xyz[3],
                          float *path_xyz, int32_t max_points, TrgPathInfo *info);
/* m consecutive planSafePath calls in one boundary crossing (reference: the loop over start/goal
 * pairs of python/examples/run_trg_planner.py:35-43).  Exactly the results
 * of calling trg_engine_plan m times in order (the goal state left behind is that of the last
 * query).  path_xyz: room for path_cap points in total; query k's points are
 * [offsets[k], offsets[k+1]) (offsets has m + 1 entries); a query without a path has an empty
 * range and infos[k].num_points == 0; a path that no longer fits is truncated (num_points keeps
 * its full length). */
TrgStatus trg_engine_plan_batch(TrgEngine *e, const float *starts_xy, const float *goals_xyz,
                                size_t m, float *path_xyz, int32_t path_cap, int32_t *offsets,
                                TrgPathInfo *infos);
/* reference: TRG::checkReadched (sic) trg.cpp:567-574 / TRG::checkReplan trg.cpp:576-601; 1 = true */
int32_t trg_engine_check_reached(TrgEngine *e, const float pos_xy[2]);
int32_t trg_engine_check_replan(TrgEngine *e, const float pos_xy[2], const float *path_xyz,
                                int32_t n_path);
/* reference: TRG::refinePath trg.cpp:692-730.  Returns the number of output points. */
int32_t trg_engine_refine_path(const float *in_xyz, int32_t n_in, float *out_xyz, int32_t max_out);

/* ---- batched probes of the pure map functions (debug / parity tests) ------------------------- */
/* reference: TRG::isCollision(pos, type, threshold) trg.cpp:746-778.  Any output may be NULL.
 * flag: 1 = collision; cnt: points with |z - z_med| > height_threshold; n: points in the disc. */
TrgStatus trg_engine_is_collision_batch(TrgEngine *e, TrgKind map, float threshold, const float *xy,
                                        size_t m, int32_t *flag, int32_t *cnt, int32_t *n);
/* reference: the kd_nearest2 elevation lookup of TRG::addNode trg.cpp:244-247 */
TrgStatus trg_engine_nearest_z_batch(TrgEngine *e, TrgKind map, const float *xy, size_t m, float *z);
/* reference: the position-only part of TRG::wireEdge trg.cpp:269-363.
 * status: 0 ok, 1 slope gate, 2 segment collision, 3 empty gather, 4 fewer than 3 points. */
TrgStatus trg_engine_edge_risk_batch(TrgEngine *e, TrgKind map, const float *p1_xyz,
                                     const float *p2_xyz, size_t m, int32_t *status, int32_t *n_pts,
                                     float *weight, float *dist);
/* reference: TRG::isFrontier trg.cpp:780-803 */
TrgStatus trg_engine_is_frontier_batch(TrgEngine *e, const float *xy, size_t m, int32_t *flag);
/* Pose links ("Pose links"; an extension): the verified links from a position to the global
 * graph, each judged on the GLOBAL map as the reference would judge an edge from a node at that position.
 * For pose k at p = (x, y):
 *   z             the elevation addNode would give a node at p (trg_engine_nearest_z_batch, map ties included)
 *   status        1 when isCollision(p, collision_threshold) holds -- the reference refuses a root there,
 *                 trg.cpp:236-241 -- and the pose then has no candidates and no links; else 0
 *   n_candidates  the nodes v with state != Invalid and d <= radius, d = sqrtf(dx * dx + dy * dy) in fp32 without
 *                 contraction (wireEdge's dist, trg.cpp:276)
 *   n_links       a candidate at d == 0 is a link of weight 0 and dist 0 without evaluation (the pose is that node);
 *                 every other candidate is evaluated as trg_engine_edge_risk_batch(GLOBAL, p1 = (x, y, z),
 *                 p2 = the node's xyz) and is a link, with that weight and dist, when its status is 0
 * Links are sorted by (dist bits, node id) ascending and the first min(cap, n_links) are written to row k of
 * link_node / link_weight / link_dist (m x cap each, any may be NULL); both counts are always the full ones.
 * All poses of a call share one collision batch, one elevation batch and one edge batch.
 * TRG_ERR_NO_MAP without a global map, TRG_ERR_NO_GRAPH for an empty graph, TRG_ERR_INVALID_ARG (naming the pose
 * where there is one) for m < 0, cap < 0, a NaN position, or a radius that is NaN, <= 0 or >= 2.5 * expand_dist
 * (wireEdge's own assert, trg.cpp:279).  m == 0 is TRG_OK. */
typedef struct TrgPoseInfo {
  int32_t status, n_candidates, n_links;
  float z;
} TrgPoseInfo;
TrgStatus trg_engine_pose_links(TrgEngine *e, const float *poses_xy, int32_t m, float radius, int32_t cap,
                                int32_t *link_node, float *link_weight, float *link_dist, TrgPoseInfo *infos);

/* ---- map ingest: voxel-grid filter --------------------------------------------------------------- */
/* reference: the pcl::VoxelGrid step of TRGPlanner::loadPrebuiltMap, trg_planner.cpp:91-94
 * (setLeafSize(voxelSize x3), filter): one point per occupied voxel = centroid of its points,
 * voxels in ascending voxel index (PCL filters/impl/voxel_grid.hpp applyFilter; PCL is not vendored
 * by the reference -> parity unpinned, the in-voxel fp32 summation order is ascending point index).
 * xyz: n host points with `stride` floats each; out_xyz: room for 3*n floats; *n_out = points
 * written.  *passthrough (optional) = 1 when the leaf is too small for 32-bit voxel indices and the
 * input was handed through unchanged, as PCL does. */
TrgStatus trg_engine_voxel_filter(TrgEngine *e, const float *xyz, size_t n, size_t stride, float leaf,
                                  float *out_xyz, size_t *n_out, int32_t *passthrough);

/* ---- options ----------------------------------------------------------------------------------- */
/* "replay" = "device" (default: BFS, dedupe and CSR on the GPU) | "host" (sequential replay on the host);
 * "keep_preclean" = "0" | "1" (keep the TRG_KIND_PRECLEAN snapshot); "defer_overlap" = "1" | "0"
 * (device BFS: deferred wireEdge evaluations pipelined behind the level loop on a second stream, one
 * batch per level -- default; 0: after the loop);
 * "tie_inplace" = "1" | "0" (device BFS: a nearest-node distance tie is settled for the affected slot alone on
 * the committed level -- off: the whole level is replayed on the host);
 * "known_start_disc" = "1" | "0" (device BFS: the first disc of a segment walk that starts at a node the level
 * loop created -- trg.cpp:283 at i = 0, the node's position bit for bit -- is the disc that accepted the node as
 * a sample, trg.cpp:398: same position, radius, threshold and map.  It cannot collide and its point count is
 * kept per node, so the speculative parent edges and the deferred evaluations add that count and start their
 * walk at the second disc -- default; 0: every disc is evaluated.  The root, nodes of host-replayed levels, and
 * every evaluation outside the global build -- updates against the local map among them -- never use a kept
 * count);
 * "lazy_tie_repair" = "1" | "0" (device BFS: an accepted sample whose nearest map point was not unique gets the
 * reference's elevation only if the level's commit made a node of it, or of another tied candidate of its level --
 * a sample's z is read by nothing but the node it creates and that node's parent edge -- default; 0: every such
 * sample is looked up and its level's commit redone when a z changed).  All modes give identical
 * graphs; the env var TRG_REPLAY=host sets the default.  Test hooks (never change results):
 * "debug_tie_every" = n (treat every n-th BFS level as tie-affected -> host level replay),
 * "debug_gate_margin" = x (widen the band of slope gates left to the host's libm),
 * "debug_spec_bound" = n (cap the speculative next-level sampling launch at n nodes -> top-up
 * launches), "debug_fallback_level" = n (the device BFS declines at level n -> whole-build host
 * replay), "debug_stall_level" = n (k_level_resolve leaves one candidate of level n undecided ->
 * BFS_ERR_STALL -> the level is taken back and replayed on the host), "debug_lookback_level" = n (one
 * workgroup's commit look-back gives up at level n -> BFS_ERR_LOOKBACK -> whole-build host replay),
 * "resolve_tickets" = "1" (every resolve launch takes its workgroup indices from start tickets -- by
 * default only the repeat of a launch whose bounded wait ran out), "debug_stitch_cap" = n (first capacity, in rows,
 * of trg_engine_stitch_exchange's record and edge buffers, so that small tilings reach its regrow loops; 0: the
 * default).  "comm_wait_seconds" = x > 0 (default 20): the longest an engine of an in-process group
 * (trg_engine_comm_join_local) waits for the other ranks -- a cap, the exchanges take milliseconds.
 * "safety_factor" = x: TrgParams.safety_factor from the next call on -- plans and cost fields price an edge with it, a
 * retained tiled cost solve becomes stale; risk fields do not know it. */
TrgStatus trg_engine_set_option(TrgEngine *e, const char *key, const char *value);
/* Tiled builds (multi-GPU; an extension, not a reference interface): restrict
 * node creation to the core region [x0,x1) x [y0,y1) -- a sample outside it counts as a rejected
 * draw -- and give the tile its own sampler epoch.  core_xyxy == NULL restores the whole plane. */
TrgStatus trg_engine_set_tile(TrgEngine *e, const float core_xyxy[4], uint32_t epoch);
/* ---- tiled builds: the boundary stitch (an extension; rule: trg_planner/tiled.py) --
 * Three steps with one exchange between each (all-gather-v of DEVICE buffers over RCCL, done by the
 * caller; tile index == rank).  d_* arguments are device pointers owned by the caller. */
typedef struct TrgBoundaryRec { int32_t local_id; float x, y, z; } TrgBoundaryRec;          /* 16 bytes */
typedef struct TrgCrossEdge { int32_t tile_a, id_a, tile_b, id_b; float weight, dist; } TrgCrossEdge; /* 24 */
/* 1: the nodes of this tile closer than expand_dist to a core side shared with another tile of the
 * cols x rows grid, ascending local id.  d_rec may be NULL to ask for the count only. */
TrgStatus trg_engine_stitch_boundary(TrgEngine *e, const float core_xyxy[4], int32_t cols, int32_t rows,
                                     int32_t tile, TrgBoundaryRec *d_rec, int32_t cap, int32_t *n_out);
/* 2: the cross edges this tile owns: every pair (a of this tile, b of a HIGHER tile) of the gathered
 * records (all tiles concatenated in tile order, rec_offsets[ntiles + 1] on the host) with fp32 planar
 * distance < expand_dist (the test of trg.cpp:414) whose wireEdge position-only part (trg.cpp:269-363)
 * succeeds on this tile's map; order (other tile, a, b). */
TrgStatus trg_engine_stitch_cross(TrgEngine *e, int32_t tile, int32_t ntiles, const TrgBoundaryRec *d_all_rec,
                                  const int32_t *rec_offsets, TrgCrossEdge *d_edges, int32_t cap,
                                  int32_t *n_out);
/* 3: this tile's rows of the global graph from ALL tiles' cross edges (any order): local edges with
 * global ids (node_offsets[tile] + local id; node_offsets[ntiles + 1] = exclusive prefix of the tiles'
 * node counts), then the row's cross edges ordered by the global id of their other end.  Read the
 * result with trg_engine_export_csr(TRG_KIND_STITCHED); creation_id holds the rows' global ids. */
TrgStatus trg_engine_stitch_assemble(TrgEngine *e, int32_t tile, int32_t ntiles, const int32_t *node_offsets,
                                     const TrgCrossEdge *d_all_edges, int32_t n_edges);
/* The whole stitch of this rank's tile with both exchanges done natively over RCCL (librccl is resolved at
 * run time): steps 1-3 above with an all-gather of counts + an all-gather of padded payloads between them.
 * rank = tile, ranks = cols * rows.  The communicator is either made here from a unique id that ONE rank
 * draws and the application hands to every rank (MPI_Bcast, a file, torch.distributed ...), or adopted
 * from the caller (an ncclComm_t of the SAME librccl instance; one that is refused, for more ranks than the
 * stitch has tiles, is not kept, and the engine is then without a communicator).  A rank whose own step fails announces it
 * in the next count exchange, so its peers return an error instead of waiting.  Read the result with
 * trg_engine_export_csr(TRG_KIND_STITCHED).  (Replaces nothing in the reference: TRG has no multi-device
 * build) */
#define TRG_COMM_ID_BYTES 128
TrgStatus trg_engine_comm_unique_id(TrgEngine *e, uint8_t id[TRG_COMM_ID_BYTES]);
TrgStatus trg_engine_comm_init(TrgEngine *e, const uint8_t id[TRG_COMM_ID_BYTES], int32_t nranks, int32_t rank);
TrgStatus trg_engine_comm_adopt(TrgEngine *e, void *nccl_comm);
/* The in-process transport, for tests of the exchange's own logic with more than one rank where RCCL cannot run
 * (it refuses two ranks on one device): the engine becomes rank `rank` of the group `group_name`, which the first
 * engine to name it makes, with `nranks` ranks, in a process-wide table.  The members are engines on the SAME device
 * in the same process, each entered from its own thread.  An all-gather of such a group is device-to-device copies on
 * the engine's own stream between two host barriers; every wait is on the host, in a condition variable, and ends
 * after "comm_wait_seconds" at the latest with TRG_ERR_DEVICE and a message naming a rank that did not arrive.
 * After that, or once a member left (trg_engine_comm_destroy, trg_engine_destroy, another join), the group fails
 * every all-gather at once; a new one needs a new name or all members gone.  TRG_ERR_INVALID_ARG for nranks < 1 or
 * > 64, a rank outside [0, nranks), a group of another size, a rank that is taken.  Never chosen unless asked for. */
TrgStatus trg_engine_comm_join_local(TrgEngine *e, const char *group_name, int32_t nranks, int32_t rank);
TrgStatus trg_engine_comm_destroy(TrgEngine *e);
TrgStatus trg_engine_stitch_exchange(TrgEngine *e, const float core_xyxy[4], int32_t cols, int32_t rows,
                                     int32_t *n_boundary, int32_t *n_cross);
/* why the last build fell back from the device path to the host replay ("" if it did not) */
const char *trg_engine_fallback_reason(const TrgEngine *e);

/* ---- cost field (an extension, DESIGN.md section 2 "Cost field"; the reference has no such call) ------
 * The least risk cost from one node to EVERY node of the global graph, on the device.  An edge u->v costs
 * (safety_factor * weight + 1) * dist, each operation rounded to fp32 (the A* step of trg.cpp:674); a walk's
 * cost is the left fold g' = g + c in fp32; walks never enter an Invalid node (trg.cpp:670).  A node's key
 * is (cost, hops), compared lexicographically; the result equals a host Dijkstra on that key bit for bit.
 *   cost[v]    least cost, +inf if unreachable
 *   hops[v]    hop count of that key, -1 if unreachable
 *   parent[v]  smallest u with an edge u->v whose extension of u's key is v's key; -1 for the source and
 *              for unreachable nodes
 * A fold may saturate: a node whose least cost is +inf is reached, with hops >= 0 and a parent, and is
 * expanded like any other; unreachable is hops == -1, not cost == +inf.
 * Source: source_id >= 0, or, with source_id == -1, the node planSafePath starts from for source_xy.
 * The output arrays are host memory of num_nodes entries; any of them may be NULL.
 * TRG_ERR_NO_GRAPH on an empty graph; TRG_ERR_INVALID_ARG for a source out of range or when an edge cost
 * is negative or not finite; TRG_ERR_DEVICE if the relaxation does not converge. */
typedef struct TrgFieldInfo {
  int32_t source;     /* the resolved source node */
  int32_t reached;    /* nodes with a key (hops >= 0), a cost of +inf included */
  int32_t rounds;     /* relaxation rounds that did work */
  int32_t host_syncs; /* times the host waited for the device */
  double ms_device;   /* hipEvent time of the solve */
  double ms_total;    /* host wall time, upload of a stale CSR and downloads included */
} TrgFieldInfo;
TrgStatus trg_engine_cost_field(TrgEngine *e, int32_t source_id, const float source_xy[2],
                                float *cost, int32_t *hops, int32_t *parent, TrgFieldInfo *info);
/* m fields in ONE solve (trg_engine_cost_field is its m == 1 call): m fields of a graph are one field of the
 * disjoint union of m copies of it, so they share the relaxation rounds, the bucket threshold and the host
 * waits instead of repeating them.  Field k follows the semantics above, from source_ids[k], or, where
 * source_ids is NULL or source_ids[k] == -1, from the node planSafePath starts from for source_xy[2k, 2k+1].
 * Duplicate sources are allowed and give identical fields.
 *   cost, hops, parent     m x num_nodes each (row k = field k), host memory; any may be NULL
 *   targets, n_targets     optional node ids (duplicates allowed) at which the fields are read on the device:
 *   cost_at, hops_at       m x n_targets each, [k * n_targets + j] = field k at targets[j]; any may be NULL.
 *                          With only these requested, nothing of num_nodes entries is copied to the host.
 *   sources_out            m resolved sources, may be NULL
 *   reached_out            m counts of nodes with a key, may be NULL
 *   info                   source = field 0's, reached = the sum over the fields, rounds / host_syncs / ms_* of
 *                          the whole solve; may be NULL
 * With every output NULL but sources_out the call resolves the sources and solves nothing.
 * TRG_ERR_INVALID_ARG (the message names the offending index where there is one) for m < 1 or
 * m > TRG_FIELD_BATCH_MAX, a source or target out of range, n_targets < 0, a missing source_xy where one is
 * needed, a negative or non-finite edge cost; TRG_ERR_CAPACITY when the m * num_nodes items do not fit a 32-bit
 * index or device memory runs out; TRG_ERR_NO_GRAPH and TRG_ERR_DEVICE as for the single call. */
#define TRG_FIELD_BATCH_MAX 64
TrgStatus trg_engine_cost_field_batch(
    TrgEngine *e, int32_t m,
    const int32_t *source_ids,   /* m entries, or NULL: all from source_xy            */
    const float *source_xy,      /* m x 2, used where source_ids is NULL or [k] == -1 */
    float *cost, int32_t *hops, int32_t *parent,   /* m x num_nodes each, any may be NULL */
    const int32_t *targets, int32_t n_targets,     /* optional                        */
    float *cost_at, int32_t *hops_at,              /* m x n_targets, any may be NULL  */
    int32_t *sources_out,        /* m resolved sources, may be NULL                   */
    int32_t *reached_out,        /* m, may be NULL                                    */
    TrgFieldInfo *info);
/* Bounded fields ("Bounded fields"): trg_engine_cost_field_batch with a bound per field.
 * The field truncated at bound b (an fp32 cost >= 0, +inf allowed) is the full field with every node whose least
 * cost is greater than b reported as unreached: cost +inf, hops -1, parent -1, not counted in reached.  Every
 * node with cost <= b -- equal bits included -- keeps its cost bits, hops and parent; b = +inf is the full field
 * (nodes reached at a saturated +inf stay reached).  The result is exact: fl(a + c) >= a, so a node within b has a
 * least walk within b, and so has every candidate parent of it.
 * Field k is truncated at bound[k] = min(budget[k], settle_k):
 *   budget     m costs, NULL: +inf each
 *   settle     over the entries of `targets`:
 *                TRG_FIELD_SETTLE_NONE  settle_k = +inf
 *                TRG_FIELD_SETTLE_ANY   the least full-field cost of field k over the targets
 *                TRG_FIELD_SETTLE_ALL   the greatest such cost
 *              a mode whose value would come from a target without a key gives +inf: ANY with no reachable
 *              target, ALL with an unreachable or Invalid one, solve the full field.
 *   bound_out  m: bound[k], a function of the graph, the sources and the arguments alone; may be NULL
 * The solve stops expanding a field once its bound is known, so a bound that few nodes lie within costs few
 * rounds.  Everything else is trg_engine_cost_field_batch's: the sources, the outputs (cost_at / hops_at read the
 * truncated field), the resolve-only call (bound_out NULL as well), the errors, and the solve retained for
 * trg_engine_field_routes (a target beyond its field's bound has the empty route, one within it the route it
 * has in the full field) and trg_engine_field_reached.  trg_engine_cost_field_batch is this call with budget
 * NULL, TRG_FIELD_SETTLE_NONE and bound_out NULL.
 * TRG_ERR_INVALID_ARG also for a budget that is negative or NaN (the message names the field), a settle value
 * outside the enum, a settle mode other than NONE with n_targets == 0 or targets NULL. */
enum { TRG_FIELD_SETTLE_NONE = 0, TRG_FIELD_SETTLE_ANY = 1, TRG_FIELD_SETTLE_ALL = 2 };
TrgStatus trg_engine_cost_field_bounded(
    TrgEngine *e, int32_t m, const int32_t *source_ids, const float *source_xy,
    const float *budget,         /* m, or NULL: +inf each */
    int32_t settle,              /* TRG_FIELD_SETTLE_*, over `targets` */
    float *cost, int32_t *hops, int32_t *parent,
    const int32_t *targets, int32_t n_targets, float *cost_at, int32_t *hops_at,
    int32_t *sources_out, int32_t *reached_out,
    float *bound_out,            /* m: the bound each field ended with, may be NULL */
    TrgFieldInfo *info);
/* Source sets ("Source sets"): field k starts from EVERY member of a set of nodes,
 * set k = set_ids[set_ptr[k] .. set_ptr[k+1]), each member at cost +0 and hops 0 -- for every node, the nearest member
 * by risk cost, that cost, and through trg_engine_field_routes the route from it.  A set is non-empty and may hold
 * any number of ids, duplicates and Invalid nodes (a source like any other) among them.  One field of num_nodes
 * items per set, whatever its size: a set field costs about what a field from one source costs.
 *   cost[v]    the least fp32 left fold over all walks from any member to v: bit for bit the minimum over the
 *              members' single fields
 *   hops[v]    BFS depth of v in the tight subgraph from all members at depth 0 (NOT in general the minimum of the
 *              members' hops); -1 when unreachable
 *   parent[v]  as trg_engine_cost_field's; -1 for every member and every unreachable node
 *   owner[v]   an entry of set k, counted from set_ptr[k]: for a member the least entry that names it, for any
 *              other reached node owner[parent[v]] -- where v's route starts; -1 when unreachable
 *   owned      set_ptr[m] counts: owned[set_ptr[k] + j] = nodes of field k whose owner is j (0 for an entry that a
 *              smaller entry of the same node shadows); their sum over a set is that field's reached count
 *   cost_at, hops_at, owner_at   m x n_targets, the fields read at `targets` on the device
 * budget, settle, bound_out, reached_out, info and the truncation are trg_engine_cost_field_bounded's (a truncated
 * node has owner -1); info->source is set 0's first id.  The owners cost one more pass (pointer jumping over the
 * parents, sweeps logarithmic in the greatest hop count) that runs only when owner, owner_at or owned is asked for.
 * The solve is retained like any other: trg_engine_field_reached works on it unchanged, and a route of
 * trg_engine_field_routes runs from the member that owns its target (ids[0] == set_ids[set_ptr[k] + owner]); the
 * first routes call after a solve without owners runs the owner pass (its sweeps come back in info->rounds).
 * trg_engine_cost_field_batch and _bounded are untouched by this call and keep their limit of one source per field.
 * TRG_ERR_INVALID_ARG (the message names the set, and the entry where there is one) for m < 1 or
 * m > TRG_FIELD_BATCH_MAX, set_ptr[0] != 0, an empty set or a descending set_ptr, an id out of range, and the
 * target, budget and settle errors of the bounded call; the other codes as there. */
TrgStatus trg_engine_cost_field_sets(
    TrgEngine *e, int32_t m,
    const int32_t *set_ptr,      /* m + 1, set_ptr[0] == 0, strictly ascending */
    const int32_t *set_ids,      /* set_ptr[m] node ids */
    const float *budget, int32_t settle,                           /* as trg_engine_cost_field_bounded */
    float *cost, int32_t *hops, int32_t *parent, int32_t *owner,   /* m x num_nodes each, any may be NULL */
    const int32_t *targets, int32_t n_targets,
    float *cost_at, int32_t *hops_at, int32_t *owner_at,           /* m x n_targets, any may be NULL */
    int32_t *owned,              /* set_ptr[m], may be NULL */
    int32_t *reached_out, float *bound_out, TrgFieldInfo *info);
/* Cost models ("Cost models"): trg_engine_cost_field_sets with a cost model per field, so that one
 * solve answers the same query at several risk attitudes.  A model is (safety_factor s, max_weight tau), both fp32.
 * In a field with that model an edge is admitted iff it is relaxable (its target a node, and not Invalid) and its
 * weight is <= tau, compared in fp32 (tau = +inf admits every weight); an admitted edge costs
 * (s * weight + 1) * dist, every operation rounded to fp32.  Keys, hops, parents, owners, the saturation rule, the
 * truncation at a bound and the routes are the set call's, over the field's own admitted edges and costs: the field
 * is bit for bit the one an engine created with safety_factor s computes on the graph without the edges of weight
 * > tau, and a route edge is the admitted edge of least CSR index with the matching extension (so a ceiling also
 * decides among duplicate edges).  models == NULL, or (the engine's safety_factor, +inf) for a field, is
 * trg_engine_cost_field_sets' behaviour; a single source is a set of one.
 * The solve is retained with its models: trg_engine_field_routes, trg_engine_field_reached and
 * trg_engine_cost_field_refresh (which derives the models' costs again on the updated graph) answer from it with
 * them.  Edge costs are cached per distinct model and graph; the engine's own model is never dropped from the cache.
 * TRG_ERR_INVALID_ARG, naming the field, for a safety_factor that is NaN, negative or infinite, a max_weight that is
 * NaN or negative, and for a model under which some edge cost is negative or not finite; TRG_ERR_CAPACITY when the
 * edge costs of the models do not fit the device; everything else as trg_engine_cost_field_sets. */
typedef struct TrgFieldModel {
  float safety_factor;  /* finite, >= 0 */
  float max_weight;     /* the risk ceiling: >= 0, +inf for none */
} TrgFieldModel;
TrgStatus trg_engine_cost_field_models(
    TrgEngine *e, int32_t m,
    const TrgFieldModel *models, /* m, or NULL: the engine's model for every field */
    const int32_t *set_ptr, const int32_t *set_ids,
    const float *budget, int32_t settle,
    float *cost, int32_t *hops, int32_t *parent, int32_t *owner,
    const int32_t *targets, int32_t n_targets,
    float *cost_at, int32_t *hops_at, int32_t *owner_at,
    int32_t *owned, int32_t *reached_out, float *bound_out, TrgFieldInfo *info);
/* Start costs ("Start costs"): trg_engine_cost_field_models with a start cost per set entry, so
 * that a robot with a head start, a handicapped source or a pose joined to the graph by verified links
 * (trg_engine_pose_links) starts a field.  Field k is the single-source field from a virtual node rho_k added to the
 * graph: for every entry j of set k one arc rho_k -> set_ids[j] of cost c0 = set_cost0[j] + 0.0f, nothing enters
 * rho_k, and the arcs are exempt from the Invalid rule as set members are.  Hops are counted from the members' level:
 *   cost[v]    that field's cost bits
 *   hops[v]    its hops - 1
 *   parent[v]  its parent, rho_k reported as -1
 * A node whose parent is rho_k is a ROOT: a member whose final cost is, bit for bit, its least start cost.  A cheaper
 * walk from another root strictly beats a start cost, an equal-cost walk does not ((c0, 0) is the smaller key); a
 * member that is not a root is an ordinary node with a parent and an owner.
 *   owner[v]   for a root, the least entry naming it whose c0 bits equal its cost; else owner[parent[v]]
 * owned, reached_out, owner_at, budget / settle / bound_out and the truncation are the set call's, over these keys: a
 * member whose start cost lies above the bound is unreached.  models pass through unchanged.
 * The solve is retained: trg_engine_field_reached works on it; trg_engine_field_routes ends a route at a root, with
 * TrgRouteInfo.cost the key's cost, start cost included, and path_length, avg_risk and num_nodes over graph edges and
 * nodes only; trg_engine_cost_field_refresh refuses it (TRG_ERR_INVALID_ARG, the message says why) and leaves it
 * answering, as it does a bounded one.  set_cost0 == NULL is trg_engine_cost_field_models, bit for bit on every
 * output.  Risk solves take no start values.
 * TRG_ERR_INVALID_ARG, naming set and entry, for a start cost that is NaN, negative (-0 is not) or infinite;
 * everything else as trg_engine_cost_field_models. */
TrgStatus trg_engine_cost_field_seeded(
    TrgEngine *e, int32_t m,
    const TrgFieldModel *models,
    const int32_t *set_ptr, const int32_t *set_ids,
    const float *set_cost0,      /* set_ptr[m] start costs, or NULL: +0 each */
    const float *budget, int32_t settle,
    float *cost, int32_t *hops, int32_t *parent, int32_t *owner,
    const int32_t *targets, int32_t n_targets,
    float *cost_at, int32_t *hops_at, int32_t *owner_at,
    int32_t *owned, int32_t *reached_out, float *bound_out, TrgFieldInfo *info);
/* Keep-out zones ("Keep-out zones"): trg_engine_cost_field_seeded with, per field, a list of discs
 * that the field's walks avoid -- "avoid this" said per query, the graph left as it is.  A zone is a vertical
 * cylinder (x, y, r); a zone set is a list of 0 .. TRG_ZONES_MAX zones; field k's is zones[zone_ptr[k] ..
 * zone_ptr[k + 1]).  For the CSR edge in row u with column v let a = min(u, v), b = max(u, v) by node id (both
 * directions of an edge get one verdict), P = pos[a].xy, Q = pos[b].xy.  Every operation below is one fp32 operation,
 * rounded, with no contraction:
 *   r2 = r*r
 *   ax = x - Px;  ay = y - Py;  da = ax*ax + ay*ay
 *   bx = x - Qx;  by = y - Qy;  db = bx*bx + by*by
 *   dx = Qx - Px; dy = Qy - Py; L2 = dx*dx + dy*dy
 *   t  = ax*dx + ay*dy
 *   cr = ax*dy - ay*dx
 *   closes = da <= r2 || db <= r2 || (t > 0 && t < L2 && cr*cr <= r2*L2)
 * An edge is CLOSED by a zone set iff some zone of it closes it; a node v is INSIDE iff da <= r2 with P = pos[v] for
 * some zone, so every edge at an inside node is closed by definition.  Comparisons are taken as written: a NaN position
 * closes nothing.
 * Field k under models[k] and zone set k is, bit for bit, the field trg_engine_cost_field_seeded computes under
 * models[k] on the graph without the closed edges, CSR order otherwise kept: cost bits, hops, parents, owners, owned,
 * the target reads, the bounds, reached_out, the saturation rule, the truncation and the start costs.  Set members
 * are exempt as they are from the Invalid rule: a member inside a zone keeps its key and reaches nothing; a target
 * inside a zone is unreached.  The bucket width's edge statistics are over admitted, unclosed edges; the bad-cost flag
 * is over all edges.  zone_ptr == NULL, or an empty set for a field, is trg_engine_cost_field_seeded on every output
 * bit; a single source is a set of one.
 * The solve is retained with its zone sets: trg_engine_field_routes (a route edge is the admitted, unclosed, tight
 * edge of least CSR index) and trg_engine_field_reached answer from it, and trg_engine_cost_field_refresh derives the
 * closures again on the updated graph and its positions -- bit for bit the fresh zone solve there; bounded and
 * start-cost solves stay refused by it.  Edge costs are cached per distinct (model, zone list as bytes) and graph.
 * TRG_ERR_INVALID_ARG, naming field and zone, for a zone whose x or y is NaN or infinite or whose r is NaN, negative
 * or infinite (r == 0 is a point and accepted), for more than TRG_ZONES_MAX zones in a field, and for a zone_ptr
 * that does not start at 0 or descends; everything else as trg_engine_cost_field_seeded. */
#define TRG_ZONES_MAX 256
typedef struct TrgZone {
  float x, y;  /* the centre, finite */
  float r;     /* the radius: finite, >= 0 */
} TrgZone;
TrgStatus trg_engine_cost_field_zones(
    TrgEngine *e, int32_t m,
    const TrgFieldModel *models,
    const int32_t *zone_ptr,     /* m + 1 offsets into zones, or NULL: no zones */
    const TrgZone *zones,        /* zone_ptr[m] */
    const int32_t *set_ptr, const int32_t *set_ids,
    const float *set_cost0,
    const float *budget, int32_t settle,
    float *cost, int32_t *hops, int32_t *parent, int32_t *owner,
    const int32_t *targets, int32_t n_targets,
    float *cost_at, int32_t *hops_at, int32_t *owner_at,
    int32_t *owned, int32_t *reached_out, float *bound_out, TrgFieldInfo *info);
/* What a zone set shuts on the current global graph, by the device function the solve uses: closed[e] = 1 iff the
 * zone set closes CSR edge e (else 0; an edge whose column is no node is never closed), inside[v] = 1 iff node v is
 * inside.  closed (num_edges bytes) and inside (num_nodes bytes) may each be NULL; *n_closed and *n_inside (may be
 * NULL) always get the counts.  n_zones == 0 closes nothing.  The retained solve is left as it is.
 * TRG_ERR_INVALID_ARG for n_zones outside 0 .. TRG_ZONES_MAX, a null zones with n_zones > 0 and a bad zone (as
 * above, as field 0); TRG_ERR_NO_GRAPH without a graph; TRG_ERR_CAPACITY when device memory runs out. */
TrgStatus trg_engine_zone_edges(TrgEngine *e, const TrgZone *zones, int32_t n_zones,
    uint8_t *closed, uint8_t *inside, int32_t *n_closed, int32_t *n_inside);
/* Risk fields ("Risk fields"): for every node, how risky is the worst edge that must be crossed
 * to get there -- trg_engine_cost_field_sets with max in the place of +, exact, for every node in one solve.
 * An edge of CSR index e is relaxable exactly as in a cost field (its col a node, and not Invalid); its risk is
 * r[e] = weight[e] + 0.0f in fp32, so that a weight of -0 counts as +0.  Node v's key is (risk, hops):
 *   risk[v]    the least, over all walks of relaxable edges from a member of the set (key (+0, 0)) to v, of the
 *              greatest r[e] on the walk: +0 for a member, +inf (hops -1) when unreachable, always the weight of
 *              some edge or +0.  max never rounds, so there is no saturation rule.
 *   hops[v]    with an edge u -> v TIGHT iff it is relaxable, u has a key and max(risk[u], r[e]) == risk[v] as bits:
 *              the BFS depth of v in the subgraph of tight edges from the members at depth 0 -- what a host Dijkstra on
 *              the key (risk, hops) with the extension (max(risk, r), hops + 1) computes.  NOT in general the fewest
 *              hops among all walks that attain risk[v]: such a walk may detour, in its interior, over edges riskier
 *              than the risk of the node it leaves, and those edges are not tight.
 *   parent[v]  the smallest u with a tight edge into v and hops[u] + 1 == hops[v]; -1 for members and unreached nodes
 *   owner, owned, owner_at, reached_out   trg_engine_cost_field_sets' definitions, over these keys
 *   risk_at, hops_at   m x n_targets, the fields read at `targets` on the device
 * budget[k] is a CEILING: field k truncated at bound b is the full risk field with every node of risk > b reported
 * as unreached and the rest untouched; settle ANY / ALL over `targets` lowers the bound as for costs, bound_out gets
 * it, and the solve stops early as a bounded cost solve does.  A solve is a cost solve or a risk solve, never both in
 * one batch (their thresholds are in different units), and cost models do not apply: a ceiling here is the budget.
 * A single source is a set of one; positions are resolved through trg_engine_cost_field_batch's resolve-only call.
 * The solve is retained like any other.  trg_engine_field_reached answers from it (its cost output is the risk).
 * trg_engine_field_routes walks the parents; the route edge into p_i is the relaxable edge of least CSR index in row
 * p_{i-1} with col p_i that is tight and steps the hops by one; TrgRouteInfo.cost is risk[target], path_length and
 * avg_risk are as for a cost solve.  trg_engine_cost_field_refresh refuses a retained risk solve
 * (TRG_ERR_INVALID_ARG, the message says so) and leaves it answering routes, as it does for a bounded one;
 * trg_engine_risk_field_refresh (below) is the call that refreshes it.
 * TRG_ERR_INVALID_ARG when some edge weight is NaN, negative (-0 is not) or infinite -- taken over ALL edges, as the
 * bad-cost flag of a cost solve is, and like it after the previously retained solve is gone; the other argument,
 * capacity and device errors are trg_engine_cost_field_sets'. */
TrgStatus trg_engine_risk_field_sets(
    TrgEngine *e, int32_t m,
    const int32_t *set_ptr, const int32_t *set_ids,
    const float *budget, int32_t settle,
    float *risk, int32_t *hops, int32_t *parent, int32_t *owner,   /* m x num_nodes each, any may be NULL */
    const int32_t *targets, int32_t n_targets,
    float *risk_at, int32_t *hops_at, int32_t *owner_at,           /* m x n_targets, any may be NULL */
    int32_t *owned, int32_t *reached_out, float *bound_out, TrgFieldInfo *info);
/* Keep-out zones on risk fields ("Keep-out zones on risk fields"): trg_engine_risk_field_sets
 * with, per field, a list of discs that the field's walks avoid -- the safest way round a closure.  The zone lists
 * and the rule that closes an edge are trg_engine_cost_field_zones' (above), unchanged: an edge is RELAXABLE FOR FIELD
 * k iff it is relaxable in a risk field (its col a node, and not Invalid) and zone set k does not close it; its risk
 * is r[e] = weight[e] + 0.0f as ever.
 * Field k is, bit for bit, the field trg_engine_risk_field_sets computes on the graph without the edges that zone set
 * k closes, CSR order otherwise kept: risk bits, hops, parents, owners, owned, the target reads, budgets and both
 * settle modes, bound_out and reached_out.  Set members are exempt as they are from the Invalid rule: a member inside
 * a zone keeps its key (+0, 0) and reaches nothing; a target inside a zone is unreached.  zone_ptr == NULL, or an
 * empty list for a field, is trg_engine_risk_field_sets on every output bit.  The bad-weight flag stays over ALL
 * edges: a closed edge with a NaN weight still refuses the solve.  The bucket width's edge statistics are over
 * relaxable, unclosed edges.
 * The solve is retained with its zone lists: trg_engine_field_routes (a route edge is the relaxable, unclosed, tight
 * edge of least CSR index) and trg_engine_field_reached answer from it, and trg_engine_risk_field_refresh derives the
 * closures again on the updated graph and its positions -- bit for bit the fresh zoned risk solve there, a node that
 * the update moved into a zone shut; bounded solves stay refused by it.  Edge risks are cached per distinct zone list
 * (as bytes) and graph, beside the edge costs.
 * TRG_ERR_INVALID_ARG, the message starting "risk field zones:", for what trg_engine_cost_field_zones refuses in a
 * zone or a zone_ptr; everything else as trg_engine_risk_field_sets. */
TrgStatus trg_engine_risk_field_zones(
    TrgEngine *e, int32_t m,
    const int32_t *zone_ptr,     /* m + 1 offsets into zones, or NULL: no zones */
    const TrgZone *zones,        /* zone_ptr[m] */
    const int32_t *set_ptr, const int32_t *set_ids,
    const float *budget, int32_t settle,
    float *risk, int32_t *hops, int32_t *parent, int32_t *owner,
    const int32_t *targets, int32_t n_targets,
    float *risk_at, int32_t *hops_at, int32_t *owner_at,
    int32_t *owned, int32_t *reached_out, float *bound_out, TrgFieldInfo *info);
/* The nodes of field `field` (0 .. m-1) of the retained solve that have a key, compacted on the device: their
 * ids in ascending order with cost and hops, so that a bounded field that reaches few nodes is read without
 * copying anything of num_nodes entries.  *n_out is always the full count; node_ids, cost and hops (room for cap
 * entries each, any may be NULL) get the first min(cap, count) entries; with all three NULL the call returns the
 * count only.  info: source = the field's, reached = the count, ms_* / host_syncs of this call; may be NULL.
 * The retained solve and its staleness are trg_engine_field_routes' (below), with the same two messages.
 * TRG_ERR_INVALID_ARG also for a field out of range and cap < 0. */
TrgStatus trg_engine_field_reached(TrgEngine *e, int32_t field,
    int32_t *node_ids, float *cost, int32_t *hops,   /* room for cap each, any may be NULL */
    int32_t cap, int32_t *n_out, TrgFieldInfo *info);
/* Routes: the paths behind the keys of the LAST cost-field solve, walked on the device (DESIGN.md section 2,
 * "Routes").  A successful trg_engine_cost_field / _batch solve stays on the device; a new solve replaces it,
 * and init_graph, update_graph (from its start, also when it fails), load_json, a reset of the global graph
 * end it.
 * Route r is field route_field[r] (0 .. m-1 of that solve) to node route_target[r].  With h = hops there:
 *   h == -1   the empty route: num_nodes 0, cost +inf, path_length and avg_risk 0;
 *   else      the h + 1 nodes source = p_0, ..., p_h = target with p_{i-1} = parent[p_i].  The route edge into
 *             p_i is the edge of least CSR index in row p_{i-1} whose col is p_i, which is relaxable (not into
 *             an Invalid node) and whose extension of p_{i-1}'s key is p_i's key -- this decides among
 *             duplicate edges.  path_length is the fp32 left fold of the route edges' dist, taken from the
 *             target end backwards (the order in which planSafePath's backtrack sums); avg_risk the same
 *             fold of their weight, divided by num_nodes in fp32; cost the key's cost word (+inf for a node
 *             reached by a saturated fold, which has a route like any other).  A target equal to the source:
 *             one node, zeros.
 * Capacity as trg_engine_plan_batch: route r's nodes are [offsets[r], offsets[r+1]) of node_ids (and of xyz,
 * x 3); a route that no longer fits in cap is truncated (its first nodes are kept), later routes are empty
 * ranges; infos[r].num_nodes always keeps the full length, so a second call with enough room -- which needs
 * no new solve -- gets all of it.  With node_ids and xyz both NULL (or cap == 0) the call returns infos only
 * and every offset is 0.  If the solve was asked for no parent output, the first routes call runs the parent
 * sweep; the routes are those of a solve that was.
 * TRG_ERR_INVALID_ARG when no solve of the current graph is retained (the message says whether there is none
 * or the graph changed), for n_routes < 0, cap < 0, a field or target out of range (the message names it and
 * the route); n_routes == 0 is TRG_OK.  TRG_ERR_CAPACITY when device memory runs out; TRG_ERR_DEVICE if a
 * walk does not end at its field's source (the retained arrays are damaged; nothing is returned as a route). */
typedef struct TrgRouteInfo {
  int32_t num_nodes;  /* full length of the route, 0 if the target is unreachable */
  float cost, path_length, avg_risk;
} TrgRouteInfo;
TrgStatus trg_engine_field_routes(TrgEngine *e, int32_t n_routes,
    const int32_t *route_field, const int32_t *route_target,
    int32_t *offsets,      /* n_routes + 1 */
    int32_t *node_ids,     /* room for cap ids, may be NULL */
    float *xyz,            /* room for cap x 3, may be NULL (filled on the host from the ids) */
    int32_t cap,
    TrgRouteInfo *infos,   /* n_routes, may be NULL */
    TrgFieldInfo *info);   /* ms_device / ms_total / host_syncs of this call, may be NULL */
/* Refresh ("Refresh"): the retained solve of an EARLIER graph brought to the current graph.
 * The result -- cost bits, hops, parents, owners -- is that of a fresh solve from the same sources on the current
 * graph; the work follows what changed between the graphs, not the graph's size.  The sources are the nodes the
 * retained solve started from, wherever they are now; the number of fields is that solve's.
 *   new2old, n_map   n_map == num_nodes entries: new2old[v] is the id node v had in the retained solve's graph, -1
 *                    for a node that graph did not have.  NULL, 0: the map the engine recorded over the
 *                    update_graph calls since that solve (init_graph, load_json, a reset and a failed update leave
 *                    none).  The map only says where old keys are tried: a wrong entry costs work, never exactness;
 *                    what it decides is where the sources are -- field k starts at the first node whose entry is
 *                    its old source, a set at the first such node of every member.
 *   cost .. reached_out   as trg_engine_cost_field_batch's; owner, owner_at as trg_engine_cost_field_sets', and
 *                    only for a retained set solve; sources_out: the sources as ids of the current graph (a set's
 *                    first member)
 *   carried_out      m counts: the nodes whose old key was still that of a walk of the current graph and was
 *                    kept as a starting point -- the sources alone when nothing could be used; may be NULL
 *   info             as the batch call's; rounds counts the relaxation rounds of both warm passes, 0 when the
 *                    graph change touched nothing the fields depend on
 * Afterwards the retained solve is the refreshed one, of the current graph: trg_engine_field_routes and
 * trg_engine_field_reached answer from it.
 * TRG_ERR_INVALID_ARG, with the retained solve left as it was, when none is retained, when it is a bounded one,
 * when it is already of the current graph, when new2old is NULL and the engine has no map (pass one, or solve
 * again), when n_map != num_nodes or an entry is below -1 or not below the old node count, when a source has no
 * node in the current graph (the message names the field, and for a set the member), when owner or owner_at is
 * asked of a solve without sets, and for the target errors of the batch call.  The other codes as there. */
TrgStatus trg_engine_cost_field_refresh(TrgEngine *e,
    const int32_t *new2old, int32_t n_map,   /* NULL, 0: the map the engine recorded over its update_graph calls */
    float *cost, int32_t *hops, int32_t *parent,            /* m x num_nodes each, any may be NULL */
    const int32_t *targets, int32_t n_targets, float *cost_at, int32_t *hops_at,
    int32_t *owner, int32_t *owner_at,                      /* set solves only */
    int32_t *sources_out, int32_t *reached_out, int32_t *carried_out,   /* m */
    TrgFieldInfo *info);
/* trg_engine_cost_field_refresh for a retained RISK solve ("Risk fields"): the same steps with
 * the edge risks in the place of the edge costs and max in the place of +, and the result -- risk bits, hops,
 * parents, owners, reached -- that of a fresh trg_engine_risk_field_sets call from the same sets on the current
 * graph.  The differences: risk / risk_at are risks; a retained COST solve is refused (TRG_ERR_INVALID_ARG, the
 * message names trg_engine_cost_field_refresh) and left answering, as that call refuses a risk solve; and an edge
 * weight of the current graph that is NaN, negative or infinite is TRG_ERR_INVALID_ARG as in a fresh risk solve --
 * found after the retained solve is gone, so nothing is retained afterwards.  A solve of
 * trg_engine_risk_field_zones is refreshed under its zone lists, which the retained solve carries. */
TrgStatus trg_engine_risk_field_refresh(TrgEngine *e,
    const int32_t *new2old, int32_t n_map,
    float *risk, int32_t *hops, int32_t *parent,
    const int32_t *targets, int32_t n_targets, float *risk_at, int32_t *hops_at,
    int32_t *owner, int32_t *owner_at,
    int32_t *sources_out, int32_t *reached_out, int32_t *carried_out,
    TrgFieldInfo *info);

/* ---- cost fields across tiles ("Cost fields across tiles") -------------------------------
 * The cost field of the GLOBAL stitched graph, solved by all ranks together: a collective call, made by every rank
 * of the engine's communicator (trg_engine_comm_init / comm_adopt / comm_join_local) with the same m and sources,
 * after a stitch (trg_engine_stitch_exchange, or trg_engine_stitch_assemble with the ranks' own exchanges) that is
 * still current -- the tile's graph has not changed since.  The global graph G is the concatenation of the tiles'
 * stitched rows; node `local id` of tile t has the global id node_offsets[t] + local id, with the node_offsets of
 * that stitch, which the engine keeps (trg_engine_stitch_ids).  Field k is what trg_engine_cost_field defines, on G,
 * from global id source_gids[k]: cost bits, hops and parents equal a host Dijkstra on G.  A rank receives its own
 * nodes' part:
 *   cost, hops, parent   m x (this tile's nodes) each, host memory, any may be NULL; parents are GLOBAL ids, the
 *                        smallest global id u with an edge u->v whose extension of u's key is v's key; -1 for the
 *                        source and for unreached nodes (hops == -1)
 * The ranks relax their own rows and trade the keys of their border nodes (16-byte records through the stitch's
 * all-gather-v) until an exchange in which no rank has news, once per pass of the solve.
 * TRG_ERR_INVALID_ARG, before any collective and with the group still usable, for what every rank judges alike: no
 * communicator, m < 1 or m > TRG_FIELD_BATCH_MAX, a NULL source_gids, a source outside [0, nodes of G).  A failure
 * of one rank's own -- no current stitched rows (TRG_ERR_INVALID_ARG), an edge cost that is negative or not finite
 * (TRG_ERR_INVALID_ARG), m x (nodes + ghosts) beyond the solver's 32-bit item index or no device memory
 * (TRG_ERR_CAPACITY), a queue overflow (TRG_ERR_DEVICE) -- is announced in the next count exchange: that rank returns
 * its error, every other rank TRG_ERR_DEVICE "another rank reported a failure", none waits.  TRG_ERR_DEVICE on every
 * rank at once when the exchanges do not converge.  Source sets and start costs are the call below, routes
 * trg_engine_tiled_field_routes, risk fields trg_engine_tiled_risk_field, budgets and settle targets
 * trg_engine_tiled_cost_field_bounded; the refresh of a retained solve is trg_engine_tiled_cost_field_refresh; cost
 * models are trg_engine_tiled_cost_field_models.  None of these calls touches the retained single-engine solve. */
typedef struct TrgTiledFieldInfo {
  int32_t exchanges;     /* all-gather-v exchanges of both passes, the two that found no news included */
  int32_t rounds;        /* relaxation rounds of this rank that did work */
  int32_t ghosts;        /* distinct other ends of this tile's cross edges */
  int32_t border_nodes;  /* this tile's nodes with a cross edge */
  int64_t records_sent;  /* records this rank published */
  float ms_device;       /* hipEvent time from the start of this rank's local work to its publish, summed over the
                          * exchanges, plus the parent sweep and outputs: the waits for other ranks are not in it */
  float ms_total;        /* host wall time */
} TrgTiledFieldInfo;
TrgStatus trg_engine_tiled_cost_field(TrgEngine *e, int32_t m, const int32_t *source_gids,
    float *cost, int32_t *hops, int32_t *parent,   /* m x (this tile's nodes), any may be NULL */
    TrgTiledFieldInfo *info);                      /* may be NULL */
/* Source sets across tiles ("Source sets across tiles"): m fields of the global stitched graph G
 * in one collective solve, field k from EVERY entry of set k = set_gids[set_ptr[k] .. set_ptr[k + 1]) (GLOBAL ids;
 * duplicates and Invalid nodes allowed), entry j at the start cost set_cost0[j] + 0.0f (set_cost0 == NULL: +0 each).
 * Every rank calls it with the same arguments after a stitch that is still current.  Field k is exactly what
 * trg_engine_cost_field_seeded defines, on G: the single-source field from a virtual node joined to every entry j of
 * set k by an arc of that cost, these arcs exempt from the Invalid rule, hops counted from the members' level.  A ROOT
 * is a member whose final cost is, bit for bit, its least start cost.  A rank receives its own V_t nodes' part (host
 * memory, any may be NULL):
 *   cost, hops, parent   m x V_t; parents are GLOBAL ids, the least global id among the tight predecessors one level
 *                        up, -1 for roots and unreached nodes -- trg_engine_tiled_cost_field's rule
 *   owner                m x V_t; of a root the least entry of set k naming it whose start-cost bits equal its cost,
 *                        counted from set_ptr[k]; of every other reached node owner[parent], where the parent may be
 *                        another rank's node; -1 where unreached
 *   targets, n_targets   LOCAL ids of this tile, read on the device: cost_at, hops_at, owner_at are m x n_targets,
 *                        so that a rank that needs its Frontier nodes only downloads nothing of V_t entries
 *   owned                set_ptr[m] ints: how many of THIS tile's nodes each entry owns (the ranks' arrays sum to the
 *                        global counts)
 * With m sets of one entry each and no start costs, cost / hops / parent equal trg_engine_tiled_cost_field's from the
 * same ids bit for bit.  The owners need the parents of every rank: the parent sweep runs whether `parent` is asked
 * for or not, and then the ranks trade the owners of their border nodes -- each published once, when it is known --
 * until an exchange without news; the result is a function of the global parent forest, not of the order.
 * TRG_ERR_INVALID_ARG before any collective, the group still usable, for what every rank judges alike: no
 * communicator; m outside [1, TRG_FIELD_BATCH_MAX]; NULL set_ptr or set_gids; set_ptr[0] != 0, a decreasing set_ptr
 * or an empty set (the message names the set); a gid outside [0, nodes of G) (set and entry; where the stitch's
 * offsets are known); a start cost that is NaN, negative (-0 is not) or infinite (set and entry); n_targets < 0, or
 * n_targets > 0 with NULL targets.  A rank's own failure -- no current stitched rows, a target outside its tile
 * (TRG_ERR_INVALID_ARG), an allocation (TRG_ERR_CAPACITY), a bad edge cost, a queue overflow -- is announced in the
 * next count exchange, of the owner exchanges as well: that rank returns its error, its peers TRG_ERR_DEVICE "another
 * rank reported a failure", nobody waits.  An owner loop that outlasts m x (border nodes of all ranks) + 2 exchanges
 * ends with TRG_ERR_DEVICE on every rank at once.  Routes are trg_engine_tiled_field_routes, risk fields from sets
 * trg_engine_tiled_risk_field_sets, budgets and settle targets trg_engine_tiled_cost_field_bounded; the refresh of a
 * retained solve is trg_engine_tiled_cost_field_refresh; cost models are trg_engine_tiled_cost_field_models; the
 * retained single-engine solve is left alone. */
typedef struct TrgTiledSetInfo {
  int32_t exchanges;           /* all-gather-v exchanges of passes 1 and 2, the two without news included */
  int32_t owner_exchanges;     /* ... of the owner pass, the one without news included */
  int32_t rounds;              /* relaxation rounds of this rank that did work */
  int32_t ghosts;              /* distinct other ends of this tile's cross edges */
  int32_t border_nodes;        /* this tile's nodes with a cross edge */
  int32_t roots;               /* roots among this tile's nodes, over all fields */
  int64_t records_sent;        /* key records this rank published */
  int64_t owner_records_sent;  /* owner records this rank published */
  float ms_device;             /* as TrgTiledFieldInfo's, the owner pass's own kernels included */
  float ms_total;              /* host wall time */
} TrgTiledSetInfo;
TrgStatus trg_engine_tiled_cost_field_sets(TrgEngine *e, int32_t m,
    const int32_t *set_ptr, const int32_t *set_gids, const float *set_cost0,   /* set_cost0 may be NULL */
    float *cost, int32_t *hops, int32_t *parent, int32_t *owner,   /* m x (this tile's nodes), any may be NULL */
    const int32_t *targets, int32_t n_targets, float *cost_at, int32_t *hops_at, int32_t *owner_at,
    int32_t *owned,                                                /* set_ptr[m], may be NULL */
    TrgTiledSetInfo *info);                                        /* may be NULL */
/* Risk fields across tiles ("Risk fields across tiles"): the least, over all walks of the global
 * stitched graph G, of the GREATEST edge weight on the walk -- exactly what trg_engine_risk_field_sets defines, on G.
 * An edge's risk is w + 0.0f (-0 counts as +0), a walk never enters an Invalid node, and risk, hops and parents equal a
 * host Dijkstra on the key (risk, hops) with the extension (max(risk, r), hops + 1), bit for bit: the maximum never
 * rounds.  Collective calls like the two above, with the same exchanges, caps and outputs; `risk` stands where `cost`
 * stood.  Risk solves take no start values: every member of a set is seeded at (+0, 0), so every member is a root, whose
 * owner is the least entry of its set naming it; every other reached node takes owner[parent].  Parents are GLOBAL ids,
 * the least global id among the tight predecessors one level up, -1 for members and unreached nodes.  The
 * single-source call is m sets of one, bit for bit, with the same exchanges, rounds and records.  targets (LOCAL ids),
 * risk_at / hops_at / owner_at and owned are trg_engine_tiled_cost_field_sets'.
 * The solve graph's edge risks are computed by the first risk solve after a stitch and kept beside its edge costs: a
 * change of the safety factor leaves them and the answers as they are, and cost and risk solves may alternate on one
 * stitch.
 * TRG_ERR_INVALID_ARG before any collective, the group still usable: the refusals of the cost calls without those of
 * the start costs.  A rank's own failure, announced in the next count exchange like every other (that rank returns its
 * error, its peers TRG_ERR_DEVICE "another rank reported a failure", nobody waits): those of the cost calls, and in
 * the place of the bad edge cost "tiled risk field: an edge weight is negative or not finite" (TRG_ERR_INVALID_ARG),
 * taken over ALL edges of that rank's solve graph, relaxable or not, as in the single-engine call.
 * Routes are trg_engine_tiled_field_routes, risk ceilings (budget / settle) trg_engine_tiled_risk_field_bounded;
 * the refresh of a retained solve is trg_engine_tiled_risk_field_refresh; cost models are
 * trg_engine_tiled_cost_field_models (of the cost objective: a risk field has no cost model). */
TrgStatus trg_engine_tiled_risk_field(TrgEngine *e, int32_t m, const int32_t *source_gids,
    float *risk, int32_t *hops, int32_t *parent,   /* m x (this tile's nodes), any may be NULL */
    TrgTiledFieldInfo *info);                      /* may be NULL */
TrgStatus trg_engine_tiled_risk_field_sets(TrgEngine *e, int32_t m,
    const int32_t *set_ptr, const int32_t *set_gids,
    float *risk, int32_t *hops, int32_t *parent, int32_t *owner,   /* m x (this tile's nodes), any may be NULL */
    const int32_t *targets, int32_t n_targets, float *risk_at, int32_t *hops_at, int32_t *owner_at,
    int32_t *owned,                                                /* set_ptr[m], may be NULL */
    TrgTiledSetInfo *info);                                        /* may be NULL */
/* Bounded fields across tiles ("Bounded fields across tiles"): trg_engine_cost_field_bounded's
 * definition ("Bounded fields") on the global stitched graph G.  Field k is the full tiled field k
 * -- of trg_engine_tiled_cost_field_sets from the same sets and start costs -- truncated at
 *   bound[k] = min(budget[k], settle_k):
 * every node whose cost is greater than the bound comes out unreached (+inf, hops -1, parent -1, owner -1), every node
 * at or below it, equal bits included, keeps its cost bits, hops, global-id parent and owner.
 *   budget        m costs >= 0 (+inf allowed), or NULL: +inf each.  Under the risk objective a budget is a risk ceiling.
 *   settle        TRG_FIELD_SETTLE_NONE: settle_k = +inf.  _ANY: the least full-field value of field k over the settle
 *                 targets.  _ALL: the greatest.  +inf whenever that value would come from a target without a key.
 *   settle_gids   n_settle GLOBAL ids, the same list on every rank; duplicates and Invalid nodes allowed
 *   owners        != 0: the owner pass runs and owner, targets / cost_at / hops_at / owner_at and owned are the set
 *                 call's, on the truncated field (a truncated node has owner -1).  Every rank passes the same value: the
 *                 owner pass is a collective.  0: those arguments are neither read nor written, as in the
 *                 single-source calls (m sets of one entry give their fields).
 *   bound_out     m, may be NULL: bound[k], the same bits on every rank, a tile without nodes included -- a function of
 *                 G, the sets, the start costs and these arguments alone
 *   reached_out   m, may be NULL: how many of THIS tile's nodes lie within field k's bound (the ranks' counts sum to
 *                 the truncated field's reached nodes)
 * With budget NULL and TRG_FIELD_SETTLE_NONE the solve is the unbounded calls' bit for bit, with their exchanges, rounds
 * and records.  Else pass 1 of the solve relaxes nothing above a field's current bound and publishes no key above it;
 * the ranks lower the bound between the exchanges from the keys their settle targets hold -- upper bounds on the
 * targets' final values -- told to each other in the same 16-byte records, until an exchange without news, where the
 * bound is the definition's on every rank.  A wavefront that a bound keeps inside one tile ends with the fewest
 * exchanges there are.  The solve is retained like any tiled solve: trg_engine_tiled_field_routes answers from it, a
 * target beyond its field's bound has the empty route, one within it the route it has in the full field.
 * TRG_ERR_INVALID_ARG before any collective, the group still usable, beside the set call's refusals: a budget that is
 * negative or NaN (the message names the field); a settle value outside the enum; a settle mode other than NONE with
 * n_settle <= 0 or NULL settle_gids; a settle target outside [0, nodes of G) (the message names the target).  A rank's
 * own failure is announced in the next count exchange like every other. */
TrgStatus trg_engine_tiled_cost_field_bounded(TrgEngine *e, int32_t m,
    const int32_t *set_ptr, const int32_t *set_gids, const float *set_cost0,   /* set_cost0 may be NULL */
    int32_t owners,
    const float *budget,                                           /* m, or NULL */
    int32_t settle, const int32_t *settle_gids, int32_t n_settle,  /* TRG_FIELD_SETTLE_*, over GLOBAL ids */
    float *cost, int32_t *hops, int32_t *parent, int32_t *owner,   /* m x (this tile's nodes), any may be NULL */
    const int32_t *targets, int32_t n_targets, float *cost_at, int32_t *hops_at, int32_t *owner_at,
    int32_t *owned,                                                /* set_ptr[m], may be NULL */
    float *bound_out, int32_t *reached_out,                        /* m each, may be NULL */
    TrgTiledSetInfo *info);                                        /* may be NULL */
/* Cost models across tiles ("Cost models across tiles"): trg_engine_tiled_cost_field_bounded with
 * a cost model (safety_factor s_k, max_weight tau_k) per field.  On the global stitched graph G, field k is exactly what
 * trg_engine_cost_field_seeded with models defines on one engine:
 *   - an edge of G is admitted iff it is relaxable and w <= tau_k, compared in fp32 (tau = +inf admits every weight);
 *   - an admitted edge costs (s_k * w + 1) * dist, each operation rounded to fp32;
 *   - everything else keeps its definition over the field's own admitted edges and costs: keys, hops, global-id parents
 *     (the least global id among the tight predecessors one level up), the saturation rule, roots, owners, owned, the
 *     truncation at min(budget, settle value), bound_out, reached_out, the reached lists and the routes;
 *   - a route edge is the ADMITTED tight edge of least CSR index in the parent's row.
 * As an equation between programs: the tiled field of (s, tau) on G is, bit for bit, the tiled field that engines
 * created with safety_factor s compute on G without the edges of weight > tau, CSR order kept.  One stitch record
 * serves both directions of a cross edge, so both ranks judge its admission and its cost from the same w and dist bits.
 * models == NULL is trg_engine_tiled_cost_field_bounded bit for bit on every output; a solve whose models all equal
 * (the engine's safety_factor, +inf) gives the plain call's fields and the same exchanges, rounds and records_sent.
 * The arguments after `models` are trg_engine_tiled_cost_field_bounded's, in its order; every rank passes the same
 * models.  The edge costs are cached per distinct model on the rank's solve graph, for one tile graph and stitch: room
 * for TRG_FIELD_BATCH_MAX + 1 models, the engine's own never dropped, the least recently used that the solve does not
 * read given away first; the single-engine cache is neither read nor evicted.  The solve is retained with its models:
 * trg_engine_tiled_field_routes (the walk, and the late parent sweep after a solve without parents) and
 * trg_engine_tiled_field_reached answer under them.  Staleness is one rule: a new graph, a new stitch or a change of the
 * engine's safety factor makes any cost solve stale, even where every field names its own s.
 * TRG_ERR_INVALID_ARG before any collective, the group and the retained tiled solve still usable, naming the field:
 * a safety_factor that is NaN, negative or infinite, a max_weight that is NaN or negative; beside them the bounded
 * call's refusals.  A rank's own failure, announced in the next count exchange like every other (that rank returns its
 * error, its peers TRG_ERR_DEVICE "another rank reported a failure", nobody waits): a model under which some edge cost of
 * THIS rank's solve graph is negative or not finite (TRG_ERR_INVALID_ARG naming the first such field; taken over all
 * edges, those above the ceiling included), and edge costs that do not fit the device (TRG_ERR_CAPACITY).
 * Refresh is not offered across tiles for a solve under models, nor for one under bounds or with start costs:
 * trg_engine_tiled_cost_field_refresh refuses them as trg_engine_cost_field_refresh refuses their single-engine kin. */
TrgStatus trg_engine_tiled_cost_field_models(TrgEngine *e, int32_t m,
    const TrgFieldModel *models,   /* m, or NULL: the engine's model for every field */
    const int32_t *set_ptr, const int32_t *set_gids, const float *set_cost0,   /* set_cost0 may be NULL */
    int32_t owners,
    const float *budget,                                           /* m, or NULL */
    int32_t settle, const int32_t *settle_gids, int32_t n_settle,  /* TRG_FIELD_SETTLE_*, over GLOBAL ids */
    float *cost, int32_t *hops, int32_t *parent, int32_t *owner,   /* m x (this tile's nodes), any may be NULL */
    const int32_t *targets, int32_t n_targets, float *cost_at, int32_t *hops_at, int32_t *owner_at,
    int32_t *owned,                                                /* set_ptr[m], may be NULL */
    float *bound_out, int32_t *reached_out,                        /* m each, may be NULL */
    TrgTiledSetInfo *info);                                        /* may be NULL */
/* trg_engine_tiled_cost_field_bounded under the risk objective (trg_engine_tiled_risk_field_sets' fields; no start
 * values, no cost models). */
TrgStatus trg_engine_tiled_risk_field_bounded(TrgEngine *e, int32_t m,
    const int32_t *set_ptr, const int32_t *set_gids,
    int32_t owners,
    const float *budget,                                           /* m risk ceilings, or NULL */
    int32_t settle, const int32_t *settle_gids, int32_t n_settle,
    float *risk, int32_t *hops, int32_t *parent, int32_t *owner,   /* m x (this tile's nodes), any may be NULL */
    const int32_t *targets, int32_t n_targets, float *risk_at, int32_t *hops_at, int32_t *owner_at,
    int32_t *owned,                                                /* set_ptr[m], may be NULL */
    float *bound_out, int32_t *reached_out,                        /* m each, may be NULL */
    TrgTiledSetInfo *info);                                        /* may be NULL */
/* Refresh across tiles ("Refresh across tiles"): the retained tiled solve brought to the current
 * stitch -- trg_engine_cost_field_refresh's steps (carry, anchor, warm pass 1, anchor again, warm pass 2) on the global
 * stitched graph.  A collective call: every rank makes it when (a) the last tiled solve succeeded and is retained, (b)
 * any number of ranks have changed their tile graph since (update_graph any number of times, or a replaced graph), and
 * (c) a new stitch is current on every rank, with the rank count and the tile layout of the solve: nodes never change
 * tile.  new2old (n_map entries = this tile's nodes now): entry v is the LOCAL id this tile's node v had at the retained
 * solve, -1 for a new node; NULL takes the engine's own map -- the identity after a tiled solve or refresh, composed
 * through every update_graph since, none after init_graph, load_json, a reset or a failed update.  The map is a hint: a
 * wrong entry carries a key that the anchor drops.  It decides only where the members are: a member's node is the first
 * new local id of its owner tile that the map names as its old local id.
 * The result is bit for bit what trg_engine_tiled_cost_field_sets / trg_engine_tiled_risk_field_sets computes from
 * set_gids_out on the current stitch (a retained single-source solve: without the owner pass, and owner, the targets'
 * reads and owned are neither read nor written): value bits, hops, global parents, owners, owned, the target reads and
 * the roots.  The refreshed solve is then the retained one: it answers trg_engine_tiled_field_routes and
 * trg_engine_tiled_field_reached, and can be refreshed again.  set_gids_out (set_ptr[m] of the retained request, the
 * same on every rank): the NEW global id of every member.  carried_out (m): THIS tile's nodes per field that kept a key
 * through carry and anchor.  A retained solve that is current on every rank refreshes with 0 rounds.
 * TRG_ERR_INVALID_ARG before any collective, the retained solve still answering, for what every rank judges alike: no
 * communicator; no retained tiled solve; a bounded, modelled or start-cost solve (removed keys bound nothing, and members
 * would need their start costs as anchors); a solve of the other objective; another rank count than the solve's.  A
 * rank's own failure -- no map, a wrong n_map or an entry that is no old node and not -1, no current stitch, a member
 * whose node is gone (TRG_ERR_INVALID_ARG), an allocation (TRG_ERR_CAPACITY) -- is announced in the first count exchange:
 * that rank returns its error, its peers TRG_ERR_DEVICE "another rank reported a failure", nobody waits, and nothing is
 * retained afterwards. */
typedef struct TrgTiledRefreshInfo {
  int32_t exchanges;            /* all-gather-v exchanges of the two warm passes, the two without news included */
  int32_t anchor_exchanges;     /* ... of the fill and both anchors */
  int32_t owner_exchanges;      /* ... of the owner pass (0 without owners) */
  int32_t rounds;               /* relaxation rounds of this rank that did work */
  int32_t ghosts;
  int32_t border_nodes;
  int32_t roots;
  int32_t m;                    /* fields of the refreshed solve */
  int32_t owners;               /* 1: the retained solve was a set solve, the owner pass ran */
  int32_t reserved;
  int64_t records_sent;         /* key records this rank published in the passes */
  int64_t anchor_records_sent;  /* carried keys, member records and anchor verdicts */
  int64_t owner_records_sent;
  float ms_device;
  float ms_total;
} TrgTiledRefreshInfo;
TrgStatus trg_engine_tiled_cost_field_refresh(TrgEngine *e, const int32_t *new2old, int32_t n_map,
    float *cost, int32_t *hops, int32_t *parent, int32_t *owner,   /* m x (this tile's nodes), any may be NULL */
    const int32_t *targets, int32_t n_targets, float *cost_at, int32_t *hops_at, int32_t *owner_at,
    int32_t *owned,                                                /* set_ptr[m], may be NULL */
    int32_t *set_gids_out,                                         /* set_ptr[m], may be NULL */
    int32_t *carried_out,                                          /* m, may be NULL */
    TrgTiledRefreshInfo *info);                                    /* may be NULL */
TrgStatus trg_engine_tiled_risk_field_refresh(TrgEngine *e, const int32_t *new2old, int32_t n_map,
    float *risk, int32_t *hops, int32_t *parent, int32_t *owner,
    const int32_t *targets, int32_t n_targets, float *risk_at, int32_t *hops_at, int32_t *owner_at,
    int32_t *owned, int32_t *set_gids_out, int32_t *carried_out, TrgTiledRefreshInfo *info);
/* THIS tile's reached nodes of field `field` of the retained tiled solve (any tiled field call, bounded or not), in
 * ascending global id, compacted on the device: gids / value (cost or risk) / hops get the first `cap` of them (any may
 * be NULL), *n_out their total; cap == 0 returns the count alone.  Local work, no collective: the ranks' lists,
 * concatenated in tile order, are the field's reached nodes in ascending global id.  TRG_ERR_INVALID_ARG for cap < 0,
 * without a retained tiled solve, with a stale one (the tile's graph, the stitch or, for a cost solve, the safety
 * factor changed since), or for a field outside [0, m). */
TrgStatus trg_engine_tiled_field_reached(TrgEngine *e, int32_t field,
    int32_t *gids, float *value, int32_t *hops,   /* room for cap each, any may be NULL */
    int32_t cap, int32_t *n_out);                 /* n_out may be NULL */
/* Routes across tiles ("Routes across tiles"): the paths behind the keys of the LAST tiled solve
 * (any of the tiled field calls above, whichever objective), walked on the devices.  A successful tiled solve stays on every rank's device; a new tiled solve
 * replaces it from its start (one that fails leaves none), and a change of the tile's graph, a new stitch or another
 * safety factor makes it stale (a risk solve does not know the safety factor and outlives its change).  A collective
 * call: every rank makes it with the same arguments.
 * Route r is field route_field[r] (0 .. m-1 of that solve) to the node with GLOBAL id route_target_gid[r], any rank's
 * node.  It is exactly what trg_engine_field_routes defines, on the global stitched graph G with the solve's global
 * parents: the hops + 1 nodes from the root to the target; the route edge into p_i is the tight, relaxable edge of least
 * CSR index in row p_{i-1} of G; path_length and the risk sum are fp32 left folds from the target end backwards, avg_risk
 * the risk sum / num_nodes in fp32, cost the key's cost word (a start cost included); an unreached target has the empty
 * route.  After a risk solve the routes are trg_engine_field_routes' after a risk solve: tight is tight under the
 * maximum -- max(risk[p_{i-1}], r) == risk[p_i] with the hops stepping by one -- and cost is risk[target]; the sums are the
 * same folds of dist and w.  The rank that owns a node walks the route while it stands on its nodes and hands it, with the sums so far, to
 * the owner of the parent at a seam: the fold is one fold across any number of seams.
 * Every rank receives the same offsets and the same infos for ALL routes: offsets from the full lengths and cap, clipped
 * as trg_engine_field_routes clips them (the source end is kept, later routes are empty ranges, infos[r].num_nodes keeps
 * the full length, and a second call with room needs no new solve).  In node_gids / xyz a rank receives only the
 * positions of ITS OWN nodes -- the global id, and the position from its node mirror; every other position holds -1 /
 * NaN.  Position offsets[r] + i holds the node with hops == i, so a route that leaves a tile and comes back fills two
 * stretches; trg_planner.tiled.join_routes merges the ranks' arrays.  With node_gids and xyz both NULL (or cap == 0)
 * the call returns infos only and every offset is 0.  If the solve was asked for no parents (the single-source call with
 * parent == NULL), the call runs the parent sweep first, local work.
 * The exchanges: one for the lengths (the only records a host downloads: n_routes x 16 bytes), one per stretch of the
 * route with the most seam crossings, one without news: exactly c + 3 for c crossings, beyond the largest num_nodes + 3
 * TRG_ERR_DEVICE on every rank at once.
 * The stitch emits one cross edge per unordered pair of nodes, so the seam edge of a step is unambiguous; for
 * hand-assembled rows (trg_engine_stitch_assemble) that repeat a pair, which of the tight duplicates the sums take is
 * unspecified.  Duplicate edges inside a tile are decided by the least CSR index, as on one engine.
 * TRG_ERR_INVALID_ARG before any collective, the group and the retained solve still usable, for what every rank judges
 * alike: no communicator; n_routes < 0; cap < 0; NULL route_field, route_target_gid or offsets with n_routes > 0; a
 * target outside [0, nodes of G) (where the stitch's offsets are known).  n_routes == 0 is TRG_OK without a collective.
 * A rank's own failure -- no retained tiled solve or a stale one (TRG_ERR_INVALID_ARG; the message says which), a field
 * outside [0, m) (TRG_ERR_INVALID_ARG; the message names the route), an allocation (TRG_ERR_CAPACITY), a walk that lost
 * its way (TRG_ERR_DEVICE: damaged arrays) -- is announced in the next count exchange: that rank returns its error, its
 * peers TRG_ERR_DEVICE "another rank reported a failure", nobody waits.  The retained single-engine solve
 * (trg_engine_field_routes) is neither read nor touched. */
typedef struct TrgTiledRouteInfo {
  int32_t num_nodes;  /* full length of the route, 0 if the target is unreachable */
  float cost, path_length, avg_risk;
  int32_t root_gid;   /* the global id of the node the route starts at, -1 for the empty route */
  int32_t owner;      /* a set solve: the entry of the route's set that root is, counted from set_ptr[k]; else -1 */
} TrgTiledRouteInfo;
typedef struct TrgTiledRoutesInfo {
  int32_t exchanges;     /* all-gather-v exchanges of this call, the one without news included */
  int32_t max_nodes;     /* the longest route's num_nodes */
  int64_t records_sent;  /* LEN, HANDOFF and END records this rank published */
  float ms_device;       /* as TrgTiledFieldInfo's */
  float ms_total;        /* host wall time */
} TrgTiledRoutesInfo;
TrgStatus trg_engine_tiled_field_routes(TrgEngine *e, int32_t n_routes,
    const int32_t *route_field, const int32_t *route_target_gid,
    int32_t *offsets,      /* n_routes + 1 */
    int32_t *node_gids,    /* room for cap global ids, may be NULL */
    float *xyz,            /* room for cap x 3, may be NULL */
    int32_t cap,
    TrgTiledRouteInfo *infos,    /* n_routes, may be NULL */
    TrgTiledRoutesInfo *info);   /* may be NULL */
/* The global ids of the current stitch: this tile's first global id, its node count and the global graph's.
 * TRG_ERR_INVALID_ARG without current stitched rows. */
TrgStatus trg_engine_stitch_ids(TrgEngine *e, int32_t *first_gid, int32_t *num_nodes, int32_t *total_nodes);

/* ---- instrumentation ------------------------------------------------------------------------- */
TrgStatus trg_engine_get_stats(const TrgEngine *e, TrgStats *out);
/* the direction table the engine uses (2^table_bits entries each) */
TrgStatus trg_engine_get_sampler_table(TrgEngine *e, float *cos_out, float *sin_out);
/* cell-sorted map arrays (n each), for index-build tests; any pointer may be NULL */
TrgStatus trg_engine_debug_map_index(TrgEngine *e, TrgKind map, float *x, float *y, float *z,
                                     int32_t *perm, int32_t *grid_wh, float *origin_cell);

#ifdef __cplusplus
}
#endif
#endif /* TRG_ENGINE_H_ */
