// trg_kernels.h -- host-visible launch interface of the gfx950 kernels (trg_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "map_order_runs.h"

namespace trg {

// Cell-sorted structure-of-arrays map index (replaces the reference's 2-D kd-tree of map points,
// trg.cpp:185-188 / kdtree.c).  Cells are row-major (cy * W + cx); the points of the cells
// [cx0..cx1] of one row are one contiguous, coalesced range of x[], y[], z[].
struct MapView {
  const float *x;
  const float *y;
  const float *z;
  const int *perm;        // original index of each sorted point (nearest-neighbour tie-break)
  const float4 *pt;       // the same points as 16-byte records (x, y, z, perm): what the tile staging reads --
                          // one load per point, and a row segment's ragged ends cost one partial line, not four
  const int *cell_start;  // W*H + 1 exclusive prefix of points per cell
  float x0, y0;           // grid origin (min x, min y of the cloud)
  float inv_g;            // 1 / cell size
  int W, H;
  int n;
};

// An accepted sample whose nearest map point was not unique (kd_nearest's visiting order decides
// which one the reference takes, trg.cpp:226-233 -> kdtree.c:303-362); the host resolves these.
// A sampling launch keeps every record (a slot ties at most once, the lists hold one record per slot).
constexpr int MAPTIE_CAP = 256;      // records the host replay copies back with a chunk's results; more are fetched after
constexpr int MAPTIE_SET_CAP = 16;   // points of a tie listed per page (k_map_tied_set's `skip`)
struct MapTieRec {
  int slot;        // sample slot of the launch (node * S + j)
  float qx, qy;    // the sample position
  float d2;        // the tied fp32 squared distance
};
struct MapTieSet {
  int count;                  // all tied points, whichever page was asked for
  float d2;
  int sidx[MAPTIE_SET_CAP];   // index in the cell-sorted arrays
  int perm[MAPTIE_SET_CAP];   // original (insertion) index
  float x[MAPTIE_SET_CAP], y[MAPTIE_SET_CAP], z[MAPTIE_SET_CAP];
};

struct QueryParams {
  float robot_size;
  float height_threshold;
  float collision_threshold;
  float expand_dist;
  int sample_num;
  // tiled builds: samples outside [core_x0, core_x1) x [core_y0, core_y1) are rejected draws
  // (default: the whole plane, i.e. the reference behaviour)
  float core_x0, core_y0, core_x1, core_y1;
  // relative half-width of the band in which the device does not call the slope gate itself
  // (1e-4 by default; tests widen it to exercise the host decision path)
  float gate_margin;
};

// result codes of the position-only part of wireEdge (trg.cpp:269-363)
enum : int {
  EDGE_OK = 0,
  EDGE_GATE = 1,
  EDGE_SEG = 2,
  EDGE_EMPTY = 3,
  EDGE_FEW = 4,
  EDGE_STATUS_MASK = 7,
  EDGE_GATE_UNCERTAIN = 8,  // rational slope test too close to call: host decides with libm atan2f
  EDGE_CLAMPED = 16,        // weight < 0.1 -> 0 (trg.cpp:361-363)
};

// Instrumentation counters, sharded so that concurrent blocks do not serialise on one address:
// shard = blockIdx.x % COUNTER_SHARDS, one 128-byte line per shard, summed by the host.
constexpr int COUNTER_SHARDS = 64;
struct alignas(128) DeviceCounters {
  unsigned long long sample_hits;  // map points inside sample-collision discs
  unsigned long long edge_hits;    // map points inside segment discs + ellipse gathers (k_edges)
  unsigned long long spec_hits;    // same, speculative parent edges (k_spec_edges)
  unsigned long long nn_ties;
  unsigned long long overflow;     // disc queries that used the large-disc fallback
  unsigned long long start_known;  // deferred evaluations that took their walk's first disc as known (BfsDev::ndisc)
  unsigned long long pad[10];
};

// ---- index build -------------------------------------------------------------------------------
// bounds[4] = {min_x, min_y, max_x, max_y} as order-preserving uint32 keys; init with init_bounds
void launch_init_bounds(unsigned *d_bounds, hipStream_t s);
void launch_bounds(const float *d_xyz, size_t n, size_t stride, unsigned *d_bounds, hipStream_t s);
void launch_cell_count(const float *d_xyz, size_t n, size_t stride, float x0, float y0, float inv_g,
                       int W, int H, int *d_cell_of, int *d_rank, int *d_counts, hipStream_t s);
// exclusive scan of counts[0..m) into out[0..m], out[m] = total; tmp needs ceil(m/1024)+1 ints
// voxel-grid downsampling (trg_voxel.hip); *status 1 = leaf too small, input copied through
hipError_t voxel_grid_filter(const float *d_xyz, size_t n, size_t stride, float leaf, float *d_out,
                             size_t *n_out, int *status, hipStream_t s);
void launch_exclusive_scan(const int *d_counts, int *d_out, int m, int *d_tmp, hipStream_t s);
// index build through bins (trg_kernels.hip): plan = false when the grid has too many cells for it (the direct
// count / scatter path then); d_hist and d_base hold nbins * nwg + 1 ints, d_tmp (nbins * nwg) / 2048 + 4,
// the two scratch arrays n records each (scratch_a may be the map's own record array)
bool index_bins_plan(size_t n, size_t ncell, int *bin_shift, int *nbins, int *nwg);
void launch_index_bins(const float *d_xyz, size_t n, size_t stride, float x0, float y0, float inv_g, int W, int H,
                       int ncell, int bin_shift, int nbins, int nwg, int *d_hist, int *d_base, int *d_tmp,
                       float4 *d_scratch_a, float4 *d_scratch_b, int *d_cell_start, float *x, float *y, float *z,
                       int *perm, float4 *pt, hipStream_t s);
// scatter + per-cell sort through a scratch array of n 16-byte records (one store per point)
// (pt: the sorted points once more as 16-byte records, MapView::pt)
void launch_scatter_sort_aos(const float *d_xyz, size_t n, size_t stride, const int *d_cell_of,
                             const int *d_rank, int ncell, const int *d_cell_start, void *d_aos, float *x,
                             float *y, float *z, int *perm, float4 *pt, hipStream_t s);

// ---- queries -----------------------------------------------------------------------------------
void launch_probe_collision(const MapView &m, QueryParams p, float threshold, const float *d_xy,
                            int count, int *flag, int *cnt, int *n, DeviceCounters *ctr,
                            hipStream_t s);
void launch_probe_nearest_z(const MapView &m, QueryParams p, const float *d_xy, int count, float *z,
                            int *found, DeviceCounters *ctr, hipStream_t s);
// p1/p2: count x 3 floats
// mid: device scratch of edge_mid_floats(count) floats (phase-1 records consumed by phase 2)
void launch_edges(const MapView &m, QueryParams p, const float *d_p1, const float *d_p2, int count,
                  float *mid, int *status, int *n_pts, float *weight, float *dist,
                  DeviceCounters *ctr, hipStream_t s);
size_t edge_mid_floats(size_t edges);

// Expansion of `count` queued nodes (trg.cpp:384-403 sampling + the elevation lookup :244-247):
//   node_xy[count*2], node_id[count] (sampler key), outputs per node: n_acc, n_draws and
//   per slot (node*S + j): sample x, y, z
void launch_sample_nodes(const MapView &m, QueryParams p, const float *cos_t, const float *sin_t,
                         int table_bits, uint32_t seed, uint32_t epoch, const float *node_xy,
                         const int *node_id, int count, int *n_acc, int *n_draws, float *sx,
                         float *sy, float *sz, DeviceCounters *ctr, int *mt_count,
                         MapTieRec *mt_rec, hipStream_t s);
// exact nearest-point tie-break helpers (rare path, see map_nn_exact in trg_engine.cpp)
// the tied points number skip .. skip + MAPTIE_SET_CAP - 1 in the order of the cell-sorted arrays, and the count of all
void launch_map_tied_set(const MapView &m, float qx, float qy, float r0, int skip, MapTieSet *d_out,
                         hipStream_t s);
// State of one walk down the map's insertion tree (which of two tied points kd_nearest visits first):
// the steps run on the device back to back, the host only looks at the final state.
struct MapTieWalk {
  float lo[2], hi[2];      // half-open region of the current subtree
  int cur_perm;            // its ancestor (points inserted later than this one are in the subtree)
  int axis;
  float qx, qy;
  int aperm, bperm;
  float ax, ay, bx, by;
  int done;                // 0 walking, 1 decided (first = 0: A, 1: B), 2 lost its candidates
  int first;
  int steps;               // tree levels descended so far, the host's part included
};
void launch_map_tie_walk(const MapView &m, MapTieWalk *d_state, int block_steps, hipStream_t s);
// out_xy[2 * k], [2 * k + 1] = position of the point with original index k, for k < M
void launch_collect_first(const MapView &m, int M, float *d_out_xy, hipStream_t s);
// Speculative parent edges node -> sample for every accepted sample of a chunk:
//   node_xyz[count*3]; slot = node*S + j evaluated iff j < n_acc[node]
void launch_spec_edges(const MapView &m, QueryParams p, const float *node_xyz, int count,
                       const int *n_acc, const float *sx, const float *sy, const float *sz,
                       float *mid, int *status, int *n_pts, float *weight, float *dist,
                       DeviceCounters *ctr, hipStream_t s);

// ---- device-resident BFS (trg_bfs.inc, trg_level.inc) -------------------------------------------------
constexpr int GRID_SLOTS = 4;      // nodes per grid cell (cell = robot_size, nodes are >= robot_size apart)
constexpr int BFS_TIE_CAP = 64;    // tied slots of one level handed to the host one by one (more: the level is replayed)
constexpr int BFS_UNC_CAP = 4096;  // uncertain slope gates handed to the host per sync point
enum : int {
  BFS_CTR_V = 0, BFS_CTR_MNEXT = 1, BFS_CTR_NCAND = 2, BFS_CTR_NUNC = 3, BFS_CTR_ERR = 4,
  BFS_CTR_DONE = 5,   // in the host copy: the stamp of the level (as word 15)
  BFS_CTR_NTIE = 5,   // on the device: entries of tie_list (slots whose nearest node was not unique)
  BFS_CTR_NMAPTIE = 6 /* and 7: one list per level parity */,
  BFS_CTR_NUNC1 = 8,  // uncertain gates of odd levels (the next level is expanded while the host
                      // still looks at this one)
  // (9..13 spare)
  BFS_CTR_NUNC2 = 14,      // uncertain gates of the deferred evaluations (third list)
  BFS_CTR_COUNT = 16
};
enum : int {
  BFS_ERR_GRID_OVERFLOW = 1, BFS_ERR_NB_OVERFLOW = 2, BFS_ERR_VCAP = 4, BFS_ERR_TIE = 8,
  BFS_ERR_HASH = 16, BFS_ERR_LEVEL_TOO_BIG = 32, BFS_ERR_CLEAN = 64,
  BFS_ERR_STALL = 128,  // k_level_resolve's bounded wait ran out: the level is replayed on the host
  BFS_ERR_LOOKBACK = 512,  // the commit's look-back scan ran out of polls (another process on the card): the
                           // level's numbering is void, the whole build is redone by the host replay
  BFS_ERR_STEP3 = 1024,  // step 3: more neighbours than a list / the call log's stride holds, or a slope gate of a
                         // rescue edge the device could not call: the build goes to the host replay
  BFS_ERR_TIE_CLS = 256 // a sample's nearest PRE-LEVEL node was not unique (k_level_sample; the slot
                        // carries SLOT_TIE): the host picks the reference's winner, resolve + commit rerun
};
enum : int { CALL_NONE = -2, CALL_PENDING = -1 };

// One cell of the node hash grid (cell = robot_size): everything a probe needs in one 64-byte line.
struct alignas(64) GridCell {
  int cnt;
  int id[GRID_SLOTS];
  float x[GRID_SLOTS], y[GRID_SLOTS];
  int pad[3];
};
// Everything the level kernels keep per sample slot (slot = queue position * S + j), 64 bytes.
struct alignas(16) SlotRec {
  float x, y, z;   // accepted sample: position and elevation of the nearest map point
  float d0sq;      // squared distance to the nearest node that existed before the level
  int nn0;         // that node (-1: none in reach)
  int cls;         // low byte: 0 unused slot, 1 a pre-level node within robot_size, 2 candidate for a
                   // new node; SLOT_TIE: the nearest pre-level node was not unique
  int status;      // speculative parent edge (candidates): EDGE_* code and flags
  float dist;      //   its length
  float cov[5];    //   cov[0] = weight when w_given (set by the host), else unused: k_node_cov computes the covariance
  int ndisc;       // map points inside the sample's acceptance disc (k_level_sample): the commit's BfsDev::ndisc.
                   // Written for class-2 slots ONLY (stale in every other slot) and read by the commit for slots that
                   // create a node, which are class 2.  Invariant this rests on: a slot's class (low byte of cls) is
                   // set once by k_level_sample and no repair changes it -- the fixers change z, nn0, the edge words and the
                   // SLOT_TIE flag.  A repair that ever promotes a slot to a candidate must set this word (or -1).
  int w_given;    //   1: the weight itself is stored (host re-evaluation after a map tie)
  int hits;        //   map points inside the edge's query radii (instrumentation)
};
enum : int { SLOT_CLS_MASK = 0xFF, SLOT_TIE = 0x100 };
struct alignas(16) NodeRec {  // per queued node of a level, 48 bytes
  int n_acc, n_draws;         // accepted samples, draws made
  int hits_sample, hits_spec; // map points inside its sampling discs / speculative-edge queries
  unsigned cand_lo, cand_hi;  // bit j: accepted sample j is a candidate
  int spec_known;             // its speculative edges that took their first disc as known (k_level_spec)
  int pad1;
  float px, py, pz;           // the node itself (k_level_spec: its speculative edges start here)
  int pdisc;                  // ... and the map points inside its own acceptance disc (BfsDev::ndisc; -1: unknown)
};
static_assert(sizeof(SlotRec) == 64 && sizeof(NodeRec) == 48, "the level kernels address these records by 16-byte words");
struct alignas(16) HashEnt {  // candidate hash of a level: node-grid cell -> candidate
  unsigned long long tagcell; // level tag << 32 | cell; entries of other levels count as empty
  int slot;
  int pad;
  float x, y;
  int pad2[2];
};
// expandGraph's step 3 inside a level (trg_step3.inc): who can make a candidate whose parent edge failed a
// valid node after all.  Per sample slot; written for such candidates only.
constexpr int RESC_MAX = 14;
struct alignas(16) RescueRec {
  int pre;             // 1: an edge to a node that existed before the level succeeds
  int n;               // earlier candidates of the level whose edge from this sample succeeds ...
  int slot[RESC_MAX];  // ... their slots
};
struct alignas(16) NodeCov {  // what the edge to a node created by the BFS still needs: its weight
  float cov[6];               // is computed after the level loop (k_node_weights) from the covariance of the gather
                              // (xx xy xz yy yz zz, k_node_cov), or cov[0] is the weight when w_given
  int w_given;
  int call;                   // the wireEdge call that created the node
};

struct BfsDev {
  // node store (creation order) and its hash grid
  float *nx, *ny, *nz;
  int *nstate;
  int *ndisc;  // per node: map points of the GLOBAL map inside the robot_size disc around it, when the node is a sample
               // this build's level loop accepted (that disc did not collide: edge_gather's n0); -1 = unknown (the
               // root, nodes a host-replayed level created); null: option known_start_disc=0
  NodeCov *ncov;
  int vcap;
  GridCell *gcell;
  float gx0, gy0, ginv, gcell_size;
  int GW, GH;
  // frontier ping-pong
  int *front_cur, *front_next;
  float2 *fxy_cur, *fxy_next;  // their positions (the sampling workgroup starts from here)
  int fcap;
  // level records (two sets, by level parity)
  NodeRec *node_rec;
  SlotRec *slot_rec;
  int *c_outcome;   // per slot: resolve outcome (polled across workgroups)
  unsigned long long *c_cell;  // per slot of the level being resolved, resolve -> commit workgroups: launch epoch << 44 |
                               // creates a node (0 no, 1 Invalid, 2 valid) << 42 | node-grid cell * GRID_SLOTS + its place
  HashEnt *lv_hash;
  int ht_size;
  RescueRec *resc;   // step-3 builds only (else null)
  unsigned long long *wg_state;  // per resolve workgroup: epoch | state | created | valid (look-back scan of the commit)
  unsigned *ticket;  // start-order tickets of the resolve workgroups (runs on across launches)
  int4 *nexp;       // per expanded node: accepted | candidates << 8, draws, disc hits, speculative-edge hits
  int *nhits;       // per created node: map points inside its parent edge's queries
  // deferred edge evaluation scratch
  float *mid;
  // uncertain slope gates for the host (2 x BFS_UNC_CAP, by level parity)
  int *unc_list;
  float *unc_rec;
  int *tie_list;      // BFS_TIE_CAP slots of the current level that met an exact distance tie in k_level_resolve
  MapTieRec *mt_rec;  // 2 x mt_cap records (level parity), counts in ctrs[BFS_CTR_NMAPTIE + parity]
  int mt_cap;         // = the slots of a level (fcap * sample_num): a slot ties at most once, no record is dropped
  // call log (one record per sample slot, in program order)
  int *call_n1, *call_n2, *call_status;
  float *call_w, *call_dist;
  int *newid_of_call;  // node id created by call number i (set by the commit in k_level_resolve)
  int cstride;         // call-log entries per sample slot: 1, or LEVEL_STEP3_STRIDE when expandGraph's step 3 is on
  // counters
  int *ctrs;
  int *host_ctrs;      // pinned host copy of ctrs + stamp, written by the next level's k_level_sample (may be null)
  unsigned long long *stats64;  // [6]: longest resolve wait; [7]: multi-pass rows; [14], [15]: expansion timing (below)
  unsigned long long *tl;       // wall-clock marks of a few levels (-DLV_TIMELINE builds with TRG_TIMELINE set; else null)
};
// Words of stats64 that time the expansion of every level on the device: k_level_sample's first workgroup
// stamps the wall clock, the first resolve workgroup of the k_level_resolve behind it adds the ticks since.
constexpr int STATS64_EXPAND_START = 14, STATS64_EXPAND_TICKS = 15;
constexpr int STATS64_SPEC_KNOWN = 4;  // speculative parent edges that took their first disc as known (k_bfs_stats)

struct FinDev {
  unsigned long long *ht_key;
  int *ht_seq;
  int *ok_seq;  // per table entry: the smallest call number among the pair's SUCCESSFUL calls (its edge); after
                // launch_fin_insert_count_listed: valid for the pairs of the round-2 calls only, the others' edge
                // is their first call (ht_seq)
  unsigned ht_size;
  int *call_slot;
  int *deg, *fill, *rowptr;
  int *col, *seq;
  float *w, *dist;  // w: call_w as k_fin_scatter found it.  In a build that computes the creating edges' weights
                    // after the scatter (Build::tail_split) those entries are stale and w has no reader: the
                    // cleaned graph takes its weights from call_w (launch_fin_clean_weights); with
                    // launch_fin_scatter(with_w = false) it is not written at all
};

void launch_bfs_insert_nodes(const BfsDev &B, int first, int count, hipStream_t s);
void launch_bfs_clear_tie(const BfsDev &B, hipStream_t s);
// takes the grid reservations of a level's created nodes back (from the slots' outcomes)
void launch_bfs_undo_slots(const BfsDev &B, int slots, hipStream_t s);
// ---- one BFS level in three kernels (trg_level.inc) ---------------------------------------------
constexpr int LEVEL_MAX_SAMPLES = 64;  // sample_num the level kernels support
constexpr int LEVEL_STEP3_STRIDE = 16; // call-log entries per slot with step 3 on: the slot's own call + up to 15 neighbour calls
// expansion of the frontier nodes [node_base, count) (count_dev != nullptr: count is an upper
// bound, the kernel takes min(count, *count_dev)); tag: hash tag of this level attempt (>= 1);
// pub_stamp != 0: the launch first hands B.ctrs (the counters of the level committed just before
// it in the stream) to the host: B.host_ctrs[0..15], words 5 and 15 = pub_stamp
void launch_level_expand(const MapView &m, QueryParams p, const float *cos_t, const float *sin_t,
                         int table_bits, uint32_t seed, uint32_t epoch, const BfsDev &B, int count,
                         const int *count_dev, int node_base, int parity, int tag, int pub_stamp,
                         DeviceCounters *ctr, hipStream_t s, int which = 3);
// whether the level kernels can serve these parameters (window of the node grid, sample count)
bool level_kernels_support(const QueryParams &p, float grid_cell);
// ticketed: the workgroups take their logical index from a start ticket (*B.ticket; ticket_base = tickets
// drawn by earlier launches, advanced here) instead of blockIdx.x -- the repeat of a launch whose wait ran out
void launch_level_resolve_commit(const BfsDev &B, QueryParams p, int count, int new_state,
                                 long long call_base, int V0, int tag, int epoch, hipStream_t s,
                                 int stall_test,  // 0; test hooks: 1 a candidate stays undecided, 2 a look-back gives up
                                 bool ticketed, unsigned *ticket_base);
// sums of the per-node expansion statistics into out[0..5] (added to what is there)
typedef int TrgStatus_t;  // 0 ok
// step 3 after the level loop: the reference's node tree rebuilt on the device (creation order), then the
// neighbour calls of every valid node into the call log behind its creating call; scratch: 6 V + 8 ints
TrgStatus_t launch_step3_calls(const BfsDev &B, int V, float range, int *scratch, int *h_left, hipStream_t s);
void launch_bfs_stats(const BfsDev &B, int V, unsigned long long *out, hipStream_t s);
// covariances of the gathers of the edges that created the valid nodes [v_lo, v_hi) (their levels are final)
void launch_node_cov(const MapView &m, QueryParams p, const BfsDev &B, int v_lo, int v_hi, hipStream_t s);
// weights of the edges to the nodes [1, V) the BFS created (covariance -> SVD -> weight); after launch_node_cov
// has covered every node
void launch_node_weights(const BfsDev &B, int V, hipStream_t s);
// deferred wireEdge evaluations of the calls list[0..count) (count_dev != nullptr: count is an upper
// bound, the kernels take min(count, *count_dev))
void launch_calls_eval(const MapView &m, QueryParams p, const BfsDev &B, const int *list, int count,
                       const int *count_dev, DeviceCounters *ctr, hipStream_t s);
// pair table of the calls [c0, c1); zeroes *sel_count for the selection that follows in the same stream
void launch_first_insert(const FinDev &F, const BfsDev &B, long long c0, long long c1, int *sel_count,
                         hipStream_t s);
// round 1 of the calls [c0, c1) in one launch: the first call of every pair appended to list in any order,
// *count = how many (zero on entry: launch_first_insert), *total += that number
void launch_calls_select_append(const FinDev &F, const BfsDev &B, long long c0, long long c1, int *list,
                                int *count, unsigned long long *total, hipStream_t s);
// round 2 over the whole log in one pass (*count must be zero): calls whose pair's first call failed
void launch_calls_select2_append(const FinDev &F, const BfsDev &B, long long ncalls, int *list, int *count,
                                 unsigned long long *total, hipStream_t s);
void launch_fin_insert_count(const FinDev &F, const BfsDev &B, long long ncalls, hipStream_t s);
// builds without step 3: ok_seq over the round-2 calls list[0..count) alone, F.ok_seq needs no clear (trg_bfs.inc)
void launch_fin_insert_count_listed(const FinDev &F, const BfsDev &B, long long ncalls, const int *list, int count,
                                    hipStream_t s);
// with_w = false: F.w is left alone (a build whose cleaned graph takes its weights from call_w: launch_fin_clean_weights)
void launch_fin_scatter(const FinDev &F, const BfsDev &B, long long ncalls, bool with_w, hipStream_t s);
void launch_fin_rowsort(const FinDev &F, int V, hipStream_t s);
// map_order[0..V) expanded on the device from the node container's runs (map_order_runs.h)
void launch_map_order_fill(const MapOrderRuns &R, int V, int *map_order, hipStream_t s);
// launch_fin_clean in three steps, for a build that sends the node arrays to the host while the rows are still
// being filled: the renumbering (needs F.rowptr, not the rows), xyz / state, and col / dist after launch_fin_scatter
void launch_fin_renumber(const FinDev &F, const BfsDev &B, const int *map_order, int V, int *keep_flag,
                         int *keep_pos, int *new2old, int *old2new, int *deg_new, int *rowptr_new,
                         int *scan_tmp, hipStream_t s);
void launch_fin_clean_nodes(const FinDev &F, const BfsDev &B, int V, const int *keep_pos, const int *new2old,
                            float *xyz, int *state, hipStream_t s);
void launch_fin_clean_edges(const FinDev &F, const BfsDev &B, int V, const int *keep_pos, const int *new2old,
                            const int *old2new, const int *rowptr_new, int *col, float *dist, hipStream_t s);
void launch_fin_clean(const FinDev &F, const BfsDev &B, const int *map_order, int V, int *keep_flag,
                      int *keep_pos, int *new2old, int *old2new, int *deg_new, int *rowptr_new,
                      int *scan_tmp, int *col, float *w, float *dist, float *xyz, int *state,
                      hipStream_t s);
// the weights launch_fin_clean left out (w == nullptr there): w[...] = call_w of the call that made the entry, for
// the rows launch_fin_clean laid out; after launch_node_weights
void launch_fin_clean_weights(const FinDev &F, const BfsDev &B, int V, const int *keep_pos, const int *new2old,
                              const int *rowptr_new, float *w, hipStream_t s);

// ---- tile-boundary stitch of the tiled build (trg_stitch.inc) ----------------------------------------
struct StitchRec {  // a boundary node: local id and position (16 bytes; layout of TrgBoundaryRec)
  int id;
  float x, y, z;
};
struct StitchEdge {  // a cross edge (24 bytes; layout of TrgCrossEdge)
  int tile_a, id_a, tile_b, id_b;
  float weight, dist;
};
constexpr int STITCH_MAX_TILES = 64;
// sides: bit 0 left, 1 right, 2 bottom, 3 top side of the core has a neighbouring tile
void launch_stitch_boundary(const float *d_xyz, int V, const float core[4], int sides, float d, int *flag,
                            int *off, int *scan_tmp, StitchRec *rec, int cap, hipStream_t s);
void launch_stitch_pairs(const StitchRec *all, const int *rec_offsets, int tile, int ntiles, float d,
                         int pass, int *cnt, const int *off, int *pair_a, int *pair_b, hipStream_t s);
void launch_stitch_pair_points(const StitchRec *all, const int *pair_a, const int *pair_b, int n,
                               float *p1, float *p2, hipStream_t s);
void launch_stitch_edge_select(const StitchRec *all, const int *rec_offsets, int tile, int ntiles,
                               const int *pair_a, const int *pair_b, const int *status,
                               const float *weight, const float *dist, int n, int *flag, int *off,
                               int *scan_tmp, int *n_unc, StitchEdge *out, int cap, hipStream_t s);
void launch_stitch_assemble(const StitchEdge *edges, int n_edges, int tile, int ntiles,
                            const int *node_offsets, const int *rowptr, const int *col, const float *w,
                            const float *dist, int V, int *extra, int *deg, int *rowptr_new,
                            int *scan_tmp, int *fill, int *col_new, float *w_new, float *dist_new,
                            int phase, hipStream_t s);

// ---- cost field of the global graph (trg_field.hip; an extension) ----------------
// m fields (m sources) are solved at once as ONE field of the disjoint union of m copies of the graph.  A
// work item is the pair (field k, node v), indexed k * V + v; an edge (k, u) -> (k, col) stays in its field.
// Every per-node array is per item (N = m * V entries); rowptr, col and the edge costs are one shared copy.
// An item's key is (fp32 cost bits << 32 | hops); unreached = FIELD_KEY_NONE.  Edge costs are
// (safety_factor * w + 1) * dist in fp32; FIELD_EDGE_SKIP marks an edge never relaxed (into an Invalid
// node, or a column out of range).
constexpr unsigned long long FIELD_KEY_NONE = ~0ull;
constexpr unsigned FIELD_EDGE_SKIP = 0xFFFFFFFFu;
constexpr int FIELD_NODE_INVALID = -1;  // TRG_NODE_INVALID
constexpr int FIELD_MAX_SOURCES = 64;   // TRG_FIELD_BATCH_MAX
// per graph: the edge costs' sum and count over relaxable edges (the bucket width) and the bad-cost flag
struct alignas(128) FieldEdgeStats {
  double sum;
  int count;
  int bad;   // some edge cost is negative or not finite
};
// Round control, one set for all fields (it describes the union graph).  Words updated by atomics inside a
// launch and words written by the one-thread round end live on separate 128-byte lines.
struct alignas(128) FieldCounters {
  int n[2];        // near-queue sizes, by round parity
  int nfar[2];     // far-pile sizes, by far_sel
  unsigned fmin;   // least live far cost (bits) when a round relaxed nothing into the near queue; ~0 = none
  int overflow;    // a push past a queue's capacity (the stamps make it impossible; checked anyway)
};
struct alignas(128) FieldState {
  int work;        // near-queue entries after the last round: 0 = converged
  int rounds;      // rounds that did work
  int overflow;
  unsigned thr;    // near bucket: cost bits < thr (bits, so that the bucket above a least cost of +inf exists)
  float delta;     // bucket width
  unsigned phase;  // far-pile stamp of the current bucket
  int far_sel;
};
struct FieldCtrl {
  FieldCounters c;
  FieldState s;
  alignas(128) int reached[FIELD_MAX_SOURCES];  // per field: items with a key
  // Bounded solves only ("Bounded fields"): field k's bound as cost bits -- the caller's
  // budget at first, lowered by the settle step; nothing above it is relaxed, and pass 1 ends with the keys
  // above it removed.
  alignas(128) unsigned bound[FIELD_MAX_SOURCES];
};
struct FieldBounds {
  unsigned bits[FIELD_MAX_SOURCES];
};
constexpr int FIELD_SETTLE_NONE = 0;  // TRG_FIELD_SETTLE_*
constexpr int FIELD_SETTLE_ANY = 1;
constexpr int FIELD_SETTLE_ALL = 2;
struct FieldSources {
  int id[FIELD_MAX_SOURCES];
};
// Cost models ("Cost models"): the edge costs of a solve whose fields do not all price an edge
// alike lie in one array of slots, slot * stride + e, one slot per distinct model; field k reads slot[k].  F.ec is
// slot 0's first entry.  A solve whose fields share one slot gets no table: its F.ec points at that slot.
struct FieldModels {
  long long stride;  // entries from one slot to the next
  int slot[FIELD_MAX_SOURCES];
};
// Source sets ("Source sets"), which a solve may take in place of single sources: field k
// starts from every member of set k = ids[ptr[k] .. ptr[k + 1]) at key (0, 0) instead of from one node.
// An entry is an index into ids; the owner of an item is an entry of its field's set, counted from ptr[k].
// Which entry stands for a member item is kept in the item's stamp_near word: FIELD_MEMBER | its least entry.
// A round stamp is >= 1 and k_field_init leaves 0, so the word is negative for members only, and it stays so:
// a member's key (0, 0) is never improved, hence the relaxation never pushes, and never stamps, a member.
// With start costs ("Start costs") that holds for pass 2 only, which marks the roots alone -- the
// members whose key is their least start cost; pass 1 may overwrite a mark, and nothing reads one before pass 2.
struct FieldSets {
  const int *ptr;   // m + 1 entry offsets, ptr[0] == 0 (device)
  const int *ids;   // ptr[m] node ids (device)
  int n;            // ptr[m]
  int *owner;       // per item: the owning entry of its field's set, -1 without a key; nullptr until asked for
};
constexpr int FIELD_MEMBER = INT32_MIN;
struct FieldDev {
  const int *rowptr, *col;
  const float *ec;             // edge costs
  int V;                       // nodes
  int m;                       // fields
  int N;                       // items: m * V
  unsigned long long *key;
  int *q[2];                   // near queues of items (N entries each), by round parity
  int *far[2];                 // far piles of items (N entries each), by far_sel
  int *stamp_near;             // round that last pushed the item to a near queue
  unsigned *stamp_far;         // phase that last pushed the item to a far pile
  int *parent;                 // node ids, per item
  FieldCtrl *ctrl;
  const unsigned *tight;       // pass 2: the least costs of pass 1 (bits), per item; only edges with
                               // fl(cost[u] + c) == cost[v] are relaxed.  nullptr in pass 1.
};
// ec[e] = (safety_factor * w[e] + 1) * dist[e], FIELD_EDGE_SKIP for an edge that is not relaxable or whose weight
// is above max_weight (+inf: none is); *st (zeroed here) over the edges that got a cost, its bad flag over all.
void launch_field_edge_cost(const int *col, const float *w, const float *dist, const int *state, int V, int E,
                            float safety_factor, float max_weight, float *ec, FieldEdgeStats *st, hipStream_t s);
// Risk fields ("Risk fields"): er[e] = w[e] + 0, FIELD_EDGE_SKIP for an edge that is not
// relaxable; *st (zeroed here) over the relaxable edges, its bad flag over all (a weight that is NaN, negative or
// infinite).  `er` is a slot of the edge-cost array: a risk solve's F.ec points at it.
void launch_field_edge_risk(const int *col, const float *w, const int *state, int V, int E, float *er,
                            FieldEdgeStats *st, hipStream_t s);
// Keep-out zones ("Keep-out zones"): a disc that closes every edge it touches; the layout of the
// header's TrgZone.  A zone set is at most FIELD_ZONES_MAX of them.
struct FieldZone {
  float x, y, r;
};
constexpr int FIELD_ZONES_MAX = 256;  // TRG_ZONES_MAX
// launch_field_edge_cost for a slot with a zone set: ec[e] is what that launch writes, or FIELD_EDGE_SKIP where the set
// (nz zones on the device, 1 .. FIELD_ZONES_MAX) closes edge e by the rule of DESIGN.md; *st (zeroed here) over the
// edges that got a cost, its bad flag over all.  xyz: the node positions, 3 floats a node; one 16-lane group per row.
void launch_field_edge_zones(const int *rowptr, const int *col, const float *w, const float *dist, const int *state,
                             const float *xyz, int V, int E, float safety_factor, float max_weight,
                             const FieldZone *zones, int nz, float *ec, FieldEdgeStats *st, hipStream_t s);
// launch_field_edge_risk for a slot with a zone set ("Keep-out zones on risk fields"): er[e] is
// what that launch writes, or FIELD_EDGE_SKIP where the set (nz zones on the device, 1 .. FIELD_ZONES_MAX) closes edge
// e; *st (zeroed here) over the relaxable, unclosed edges, its bad flag over all.  The row walk of the launch above.
void launch_field_edge_risk_zones(const int *rowptr, const int *col, const float *w, const int *state,
                                  const float *xyz, int V, int E, const FieldZone *zones, int nz, float *er,
                                  FieldEdgeStats *st, hipStream_t s);
// The verdicts themselves, by the same device function: closed[e] (E bytes, may be nullptr) 1 where the set closes edge
// e, inside[v] (V bytes, may be nullptr) 1 where node v is inside a zone; counts[0] / counts[1] (zeroed here) the
// closed edges and the inside nodes.  nz == 0: nothing is closed.
void launch_field_zone_verdicts(const int *rowptr, const int *col, const float *xyz, int V, int E,
                                const FieldZone *zones, int nz, unsigned char *closed, unsigned char *inside,
                                int *counts, hipStream_t s);
// Field k starts at node sources.id[k], k < F.m (duplicates give identical fields).  With `sets` (a set solve; else
// nullptr) sources is not read: every item is left without a key, then a second launch seeds every distinct member
// item and pushes it once to near queue 0; F.ctrl's queue size and work are the count of distinct member items.
// With `cost0` (a seeded solve, DESIGN.md section 2, "Start costs"; sets->n cost words on the device, else nullptr)
// entry e seeds its item at key (cost0[e], 0): in pass 1 the least of an item's entries, in pass 2 (F.tight set) only
// the entries whose start cost is the item's least cost, so that the member marks then name exactly the roots.
// With `carried` (a refresh's launch_field_carry output, per item; else nullptr) every item that is no source starts
// with its carried key instead of none; the queue is then not used: the warm start empties it.
void launch_field_init(const FieldDev &F, const FieldSources &sources, const FieldSets *sets, const unsigned *cost0,
                       const unsigned long long *carried, float delta, hipStream_t s);
// the settle step of a bounded round: n_t target nodes (device ids) and the mode, FIELD_SETTLE_*
struct FieldSettle {
  const int *targets;
  int n_t;
  int mode;
};
// One relaxation round (round >= 0, consecutive from 0): relax the near queue, and when that pushed nothing near
// in ANY field, open the next bucket from the least live far cost over all fields; every launch reads its sizes
// from F.ctrl.  under_bounds == nullptr: a round that knows nothing of bounds (every pass 2 is such: a removed
// key's tight word matches no extension).  Else pass 1 of a bounded solve: an item above its field's bound is not
// expanded, an extension above it neither written nor pushed, a far-pile entry above it not live; and with mode
// ANY / ALL, a round that opens a bucket or converges lowers the bound of every field whose targets are settled --
// some (ANY) or all (ALL) of them have a key below the least live far cost -- to the least (greatest) of those
// costs.
// models (here and below; nullptr: every field reads F.ec): the slot table of a solve with more than one cost model.
// risk (here and below; never with models): a risk solve -- F.ec holds edge risks and a walk's key is extended by
// (max(risk, r), hops + 1) instead of (fl(cost + c), hops + 1).
void launch_field_round(const FieldDev &F, int round, hipStream_t s, const FieldSettle *under_bounds = nullptr,
                        const FieldModels *models = nullptr, bool risk = false);
// F.ctrl->bound[k] = budgets.bits[k], before the first round of a bounded solve
void launch_field_bounds(const FieldDev &F, const FieldBounds &budgets, hipStream_t s);
// after the last round of pass 1: keys above their field's bound become FIELD_KEY_NONE
void launch_field_trim(const FieldDev &F, hipStream_t s);
// The nodes of one field of a finished solve that have a key, in ascending id: ids / cost / hops (any may be
// nullptr) get the first `cap` of them, offsets[(V + 255) / 256] their total.  counts: (V + 255) / 256 ints,
// offsets one more, tmp (V / 256) / 2048 + 8.
void launch_field_reached_list(const FieldDev &F, int field, int *counts, int *offsets, int *tmp, int cap, int *ids,
                               float *cost, int *hops, hipStream_t s);
// pass 1 -> pass 2: bits[item] = cost word of key[item]
void launch_field_cost_bits(const FieldDev &F, unsigned *bits, hipStream_t s);
// parents (smallest id among the edges that realise an item's key; only if `parents`) and the outputs, m x V
// each: cost (+inf), hops (-1) and parent (-1) of unreached items; F.ctrl->reached[k] counts field k's reached
// nodes
void launch_field_finish(const FieldDev &F, float *cost, int *hops, bool parents, hipStream_t s,
                         const FieldModels *models = nullptr, bool risk = false);
// the finished keys at n_t target nodes: cost_at / hops_at[k * n_t + j] of (field k, targets[j]), +inf and
// -1 where unreached; of a set solve whose owner pass ran (`sets`, else nullptr) owner_at likewise, sets->owner of
// (field k, targets[j]).  Any output may be nullptr.
void launch_field_gather(const FieldDev &F, const FieldSets *sets, const int *targets, int n_t, float *cost_at,
                         int *hops_at, int *owner_at, hipStream_t s);
// Routes of a finished solve ("Routes").  Layout of TrgRouteInfo (include/trg_engine.h).
struct FieldRouteInfo {
  int num_nodes;
  float cost, path_length, avg_risk;
};
constexpr int FIELD_ROUTE_BROKEN = -1;  // num_nodes of a walk that did not end at its field's source
// the parent sweep of a finished solve whose launch_field_finish ran without `parents`: F.parent as with it
void launch_field_parents_late(const FieldDev &F, hipStream_t s, const FieldModels *models = nullptr,
                               bool risk = false);
// len[r] = hops + 1 of (field route_field[r], node route_target[r]), 0 where unreached
void launch_field_route_len(const FieldDev &F, const int *route_field, const int *route_target, int n_routes,
                            int *len, hipStream_t s);
// Walks route r from its target back along F.parent: node ids at [offsets[r], offsets[r + 1]) (the first ids of
// a route that is longer), infos[r] over the whole route; w / dist are the CSR's edge arrays, sources the
// solve's (a walk must end at its field's, else infos[r].num_nodes = FIELD_ROUTE_BROKEN).  Of a set solve, `sets`
// are its sets with the owners filled (else nullptr): a walk must end at the member that owns its target, and
// sources is not read.  node_ids may be nullptr (offsets is then not read), infos may be nullptr.
void launch_field_route_walk(const FieldDev &F, const float *w, const float *dist, const int *route_field,
                             const int *route_target, int n_routes, const int *offsets, int *node_ids,
                             FieldRouteInfo *infos, const FieldSources &sources, const FieldSets *sets,
                             hipStream_t s, const FieldModels *models = nullptr, bool risk = false);

// ---- the owner pass of a set solve ("Source sets") -------------------------------------
constexpr int FIELD_OWNER_SWEEPS_MAX = 40;  // pointer jumping doubles: 2^31 hops need 31 sweeps and one that finds nothing
// Owners of a finished set solve whose parent sweep ran, by pointer jumping over the parents.  begin
// (launch_field_forest_begin without single sources or key0): the first ancestors into F.q[0] (a member itself,
// another reached item its parent, -1 without a key); sweep i reads F.q[i & 1], writes F.q[~i & 1] = anc[anc[.]] and
// sets changed[i] when some entry moved (changed: zeroed by begin, FIELD_OWNER_SWEEPS_MAX words); end: S.owner from
// F.q[sweeps & 1] once a sweep moved nothing.
// The begin of every jump over the forest in F.parent, the owner pass's and a refresh's anchors': a source is its
// own first ancestor -- node single->id[k] of field k, or with single == nullptr (a set solve) every member, told by
// its mark -- and with key0 (may be nullptr) an item whose key differs from key0's is cut.
void launch_field_forest_begin(const FieldDev &F, const FieldSources *single, const unsigned long long *key0,
                               int *changed, hipStream_t s);
void launch_field_owner_sweep(const FieldDev &F, int sweep, int *changed, hipStream_t s);
void launch_field_owner_end(const FieldDev &F, const FieldSets &S, int sweeps, hipStream_t s);
// owned[entry] = items whose owner is that entry (S.n counts, zeroed here)
void launch_field_owned(const FieldDev &F, const FieldSets &S, int *owned, hipStream_t s);

// ---- refresh: the retained solve of an earlier graph brought to the current one ("Refresh") --
// out[k * V + v] = old_key[k * V_old + new2old[v]], FIELD_KEY_NONE where new2old[v] is no node of the old graph; m
// fields.  `out` is a buffer of its own (m * V keys): the old solve's arrays may be regrown once this is enqueued.
void launch_field_carry(const unsigned long long *old_key, int V_old, const int *new2old, int V, int m,
                        unsigned long long *out, hipStream_t s);
// F.parent[item] = the item's supporter under the keys as they are: the smallest u with an edge u -> v and
// key_extend(key[u], c) == key[v], INT_MAX without one: the parent sweep, which launch_field_finish and
// launch_field_parents_late run through this
void launch_field_supporters(const FieldDev &F, hipStream_t s, const FieldModels *models = nullptr,
                             bool risk = false);
// The anchor: an item keeps its key if its chain of supporters (F.parent) ends at a source.  begin:
// launch_field_forest_begin; then launch_field_owner_sweep until a sweep moves nothing; end: every item whose last
// ancestor is no source loses its key, key0 (may be nullptr) gets the keys after that and carried[k] (may be nullptr;
// m ints) the number of field k's items that kept one.
void launch_field_anchor_end(const FieldDev &F, int sweeps, unsigned long long *key0, int *carried, hipStream_t s);
// A warm pass starts from the keys as they are: stamps cleared (a member's mark stays), threshold 0, both queues
// empty, and in far pile 0 every item with a key one of whose edges (F.tight set: tight edges) improves its target.
// launch_field_round from round 0 on then runs to the same fixed point as a pass from launch_field_init, provided
// every key is one that a walk of the graph has.  reset_parents: F.parent = INT_MAX, for the last parent sweep.
void launch_field_warm_start(const FieldDev &F, float delta, bool reset_parents, hipStream_t s,
                             const FieldModels *models = nullptr, bool risk = false);

// ---- cost fields across tiles (trg_field_tiled.inc; DESIGN.md section 7, "Cost fields across tiles") ----------------
// A rank's solve graph: its V local nodes (solve-graph index = local id) and then its G ghosts, the distinct other
// ends of its cross edges in ascending global id.  ghost_flag / ghost_off (Vg + 1 words each) are a flag per global
// node and its exclusive scan: the ghost index of global id g.  The solve runs the round kernels above on a FieldDev
// whose V is V + G.
struct FieldTiled {
  int V, G, B;            // local nodes, ghosts, border rows (local nodes with a cross edge)
  int lo, Vg;             // the global id of local node 0; nodes of the global graph
  const int *ghost_flag, *ghost_off;
  int *gid_of;            // V + G: solve-graph index -> global id
  int *state;             // V + G: the local nodes' states, FIELD_NODE_INVALID for every ghost
  int *border;            // B: the border rows' local ids, ascending
};
constexpr int FIELD_TILED_REC_BYTES = 16;  // (field, global id, key): what the ranks exchange
// the stitched rows (global column ids) -> ghost_flag (zeroed here) and border_flag (V words)
void launch_tiled_mark(const int *rowptr, const int *col, int V, int lo, int Vg, int *ghost_flag, int *border_flag,
                       hipStream_t s);
// after the scans of both flags (T.G, T.B known): T.gid_of, T.state, T.border, and ghost_deg (G + 1 words, zeroed here)
void launch_tiled_tables(const FieldTiled &T, const int *state, const int *border_flag, const int *border_off,
                         const int *rowptr, const int *col, int *ghost_deg, hipStream_t s);
// after the scan of ghost_deg (ghost_row, G + 1 words): the solve graph's CSR, V + G + 1 row pointers and E2 = E_local +
// ghost_row[G] edges
void launch_tiled_fill(const FieldTiled &T, const int *rowptr, const int *col, const float *w, const float *dist,
                       int E_local, int E2, const int *ghost_row, int *ghost_fill, int *rowptr2, int *col2,
                       float *w2, float *dist2, hipStream_t s);
// One entry of a source set whose member is this rank's node, as the host splits them off per call (DESIGN.md
// section 7, "Source sets across tiles"; a single source is a set of one).  `entry` is the GLOBAL index into the call's
// set_gids, which the member marks carry, so that the least entry of a node is the same on every rank.
struct TiledEntry {
  int field, node;   // the set, and the member's local id
  int entry;         // index into set_gids
  unsigned cost0;    // the start cost, bits of set_cost0[entry] + 0
};
static_assert(sizeof(TiledEntry) == 16, "entry layout");
// A pass begins: no item has a key but the members that are this rank's nodes -- its n_entries entries, queued as
// launch_field_init's seeded sets: in pass 1 each at its start cost, in pass 2 (F.tight set) the roots only, whose
// member marks then stay.  Nothing is published (m * B + 1 words).
void launch_tiled_begin(const FieldDev &F, const FieldTiled &T, const TiledEntry *entries, int n_entries, float delta,
                        unsigned long long *published, hipStream_t s);
// records (m * B of FIELD_TILED_REC_BYTES at most; *n_rec, zeroed here, counts them) of the border items with news.
// owner == nullptr, a pass: the key dropped below the published one.  Else the owner pass: the item's owner is known
// and unpublished; it travels in the record's key word.
void launch_tiled_publish(const FieldDev &F, const FieldTiled &T, const int *owner, unsigned long long *published,
                          void *rec, int *n_rec, hipStream_t s);
// the gathered records of all ranks into this rank's ghosts; what improved is queued for launch_field_round
void launch_tiled_merge(const FieldDev &F, const FieldTiled &T, const void *rec, int n_rec, hipStream_t s);
// Bounded fields across tiles ("Bounded fields across tiles"): pass 1 of a bounded tiled solve runs
// launch_field_round under bounds with the settle mode NONE, and lowers the bounds between the exchanges from the keys
// the settle targets hold.  targets: the settle targets that are THIS rank's nodes, local ids (device).  told: per field
// the value this rank last put into a bound record, +inf bits at first.  table (ALL): m rows of STITCH_MAX_TILES words,
// the ranks' last values -- at first +inf bits for a rank that owns a settle target, 0 for one that owns none.
struct TiledSettle {
  int mode;  // FIELD_SETTLE_*
  const int *targets;
  int n_t;
  int rank, n_ranks;
  unsigned *told, *table;
};
// launch_tiled_publish's pass form for pass 1 of a bounded solve: *n_rec is zeroed, the bound step writes this rank's
// bound records (field, -1 - rank, value << 32; ANY lowers F.ctrl->bound at once), then the border keys with news that
// lie within their field's bound follow.  m * B + m records at most.
void launch_tiled_publish_bounded(const FieldDev &F, const FieldTiled &T, const TiledSettle &S,
                                  unsigned long long *published, void *rec, int *n_rec, hipStream_t s);
// the bound records among the gathered records of all ranks into F.ctrl->bound; runs on a rank without nodes as well
void launch_tiled_bound_merge(const FieldDev &F, const TiledSettle &S, const void *rec, int n_rec, hipStream_t s);
// counts[k] (m ints, zeroed here) = this rank's OWN nodes with a key in field k
void launch_tiled_reached(const FieldDev &F, const FieldTiled &T, int *counts, hipStream_t s);
// launch_field_reached_list over this rank's own nodes (T.V > 0), emitting GLOBAL ids: counts (T.V + 255) / 256 ints,
// offsets one more (the last is the total), tmp (T.V / 256) / 2048 + 8
void launch_tiled_reached_list(const FieldDev &F, const FieldTiled &T, int field, int *counts, int *offsets, int *tmp,
                               int cap, int *gids, float *value, int *hops, hipStream_t s);
// parents as least global ids (when asked for), then cost / hops / parent of the local nodes, m x T.V, and with
// owner_out (else nullptr) their owners from `owner`, the owner pass's m x (V + G) words
void launch_tiled_finish(const FieldDev &F, const FieldTiled &T, float *cost, int *hops, int *parent, bool parents,
                         const int *owner, int *owner_out, hipStream_t s, bool risk = false,
                         const FieldModels *models = nullptr);
// the parent sweep alone (the set call runs it before its owner pass; launch_tiled_finish then goes without); `risk`: F.ec
// holds edge risks (launch_field_edge_risk over the solve graph) and a key is extended by the maximum; `models` (never
// with risk; "Cost models across tiles"): the fields read more than one slot of F.ec, each its own
void launch_tiled_parents(const FieldDev &F, const FieldTiled &T, hipStream_t s, bool risk = false,
                          const FieldModels *models = nullptr);
// The owner pass of the set call, after the parent sweep.  begin: F.q[0] = every item's first ancestor (a local root
// and a ghost with a key: itself; another item with a key: its parent's solve-graph item), owner (m x (V + G)) = the
// roots' entries counted from set_ptr[field], -1 elsewhere, *n_roots their count; changed (FIELD_OWNER_SWEEPS_MAX
// words) and published (m * B + 1 words) are reset.  Then launch_field_owner_sweep until a sweep moves nothing.
void launch_tiled_forest_begin(const FieldDev &F, const FieldTiled &T, const int *set_ptr, int *owner, int *changed,
                               int *n_roots, unsigned long long *published, hipStream_t s);
// One step of the owner exchange: the gathered owner records of all ranks (rec_in, n_in) into this rank's ghost
// items, every item without an owner takes its final ancestor's (anc) where known, then launch_tiled_publish's owners.
void launch_tiled_owner_step(const FieldDev &F, const FieldTiled &T, const void *rec_in, int n_in, const int *anc,
                             int *owner, unsigned long long *published, void *rec, int *n_rec, hipStream_t s);
// owned (n_entries, zeroed here) = the local nodes per entry
void launch_tiled_owned(const FieldDev &F, const FieldTiled &T, const int *set_ptr, const int *owner, int n_entries,
                        int *owned, hipStream_t s);
// Refresh across tiles ("Refresh across tiles"): the retained tiled solve brought to a new stitch.
// carry: out[k * V + v] = old_key[k * old_stride + new2old[v]] over this rank's local nodes, FIELD_KEY_NONE where
// new2old[v] is no local node of the old tile graph (V_old of them); `out` is no array of the old solve.
void launch_tiled_carry(const unsigned long long *old_key, long long old_stride, int V_old, const int *new2old, int V,
                        int m, unsigned long long *out, hipStream_t s);
// launch_field_init's place in a refresh: the local nodes take their carried keys (m x T.V), the ghosts none; then
// this rank's members are forced to (0, 0) and marked, as launch_tiled_begin seeds them (entries at cost 0).
void launch_tiled_refresh_begin(const FieldDev &F, const FieldTiled &T, const unsigned long long *carried,
                                const TiledEntry *entries, int n_entries, float delta, hipStream_t s);
// The fill exchange's publish: every border item with a key (published: m * B + 1 words, reset here), then one member
// record (entry, -1, new global id) per entry of this rank.  m * B + n_entries records at most.
void launch_tiled_fill_publish(const FieldDev &F, const FieldTiled &T, const TiledEntry *entries, int n_entries,
                               unsigned long long *published, void *rec, int *n_rec, hipStream_t s);
// the gathered records of the fill exchange: every ghost takes its owner's carried key by assignment, every member
// record writes members[entry] (n_members words)
void launch_tiled_fill_ghosts(const FieldDev &F, const FieldTiled &T, const void *rec, int n_rec, int *members,
                              int n_members, hipStream_t s);
// An anchor over the owner frame, after launch_tiled_parents found the supporters.  begin: F.q[0] = every item's first
// ancestor in the supporter forest, rooted (m x (V + G)) >= 0 for the marked members and -1 elsewhere; with key0 every
// item whose key is not key0's is cut; changed and published are reset as launch_tiled_forest_begin resets them.  Then
// launch_field_owner_sweep and launch_tiled_owner_step over `rooted`, as the owner pass runs them over its owners.
void launch_tiled_anchor_begin(const FieldDev &F, const FieldTiled &T, const unsigned long long *key0, int *rooted,
                               int *changed, unsigned long long *published, hipStream_t s);
// end: every item with rooted < 0 loses its key; key0 / carried (the first anchor; else nullptr): the keys as they are
// now and, per field, this rank's own nodes that kept theirs; published = the border keys as they are now.
void launch_tiled_anchor_end(const FieldDev &F, const FieldTiled &T, const int *rooted, unsigned long long *key0,
                             int *carried, unsigned long long *published, hipStream_t s);
// Routes across tiles ("Routes across tiles"): the routes of a finished tiled solve whose parent
// sweep ran, each walked by the rank that owns the node it stands on and handed over at a seam through the exchange's
// 16-byte records.  Layout of TrgTiledRouteInfo (include/trg_engine.h).
struct TiledRouteInfo {
  int num_nodes;
  float cost, path_length, avg_risk;
  int root_gid, owner;
};
struct TiledRoutes {
  const int *field, *target;  // n each (device): the field, and the target's GLOBAL id
  int n;
  const int *offsets;         // n + 1: the clipped segments; not read while node_gids == nullptr
  int *node_gids;             // offsets[n] global ids, or nullptr
  const float *w, *dist;      // the solve graph's edge arrays
  const int *owner;           // the owner pass's m x (V + G) words, or nullptr (a single-source solve)
  void *rec;                  // room for rec_cap records of FIELD_TILED_REC_BYTES
  int rec_cap;
  int *n_rec;                 // [0] the record count (zeroed by every launch here), [2] route + 1 of a broken walk
};
// exchange 0: a LEN record {route, hops or -1, cost bits, owner or -1} per route whose target is this rank's node
void launch_tiled_route_len(const FieldDev &F, const FieldTiled &T, const TiledRoutes &R, hipStream_t s);
// Exchange 1 (rec_in == nullptr): the walks of the routes whose target is this rank's node begin.  Later exchanges: the
// gathered HANDOFF records that name this rank's nodes are walked on, and the gathered END records are written into
// infos (n entries, device; num_nodes set from the LEN records).  A walk publishes HANDOFF {route, parent gid, sums}
// where its parent is a ghost and END {route, -1 - root gid, sums} at a root.
void launch_tiled_route_step(const FieldDev &F, const FieldTiled &T, const TiledRoutes &R, const void *rec_in, int n_in,
                             TiledRouteInfo *infos, hipStream_t s, bool risk = false,
                             const FieldModels *models = nullptr);

}  // namespace trg
