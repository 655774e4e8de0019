// trg_bfs.inc -- device-resident replay of TRG::expandGraph (trg.cpp:372-454) for configurations
// whose step 3 is disabled (mountain.yaml), included into trg_kernels.hip's anonymous namespace:
// shared helpers, the node grid, the deferred wireEdge evaluations and the call log -> CSR passes.
// The level kernels themselves are in trg_level.inc.
//
// The reference BFS is one FIFO.  Its order is preserved here by giving every accepted sample the
// sequence number (queue position of its parent) * S + j: a level (= all nodes queued at the same
// BFS depth) is processed as a batch whose slots are in exactly that order.  What a sample does in
// the reference depends only on the nodes that existed before it:
//     nn = nearest existing node; Invalid -> skip; ||nn - s|| < r -> wireEdge(parent, nn);
//     else create a node at s (Invalid iff its parent edge fails), wireEdge(parent, new).
// Nodes existing before the level (N0) sit in a device hash grid.  Nodes created inside the level
// can only come from samples with no N0 node within r ("candidates"); a candidate is decided as
// soon as no UNDECIDED earlier candidate lies closer than its current nearest node, which reproduces
// the sequential outcome exactly (the earliest undecided candidate is always decidable).
// Exact fp32 distance ties, where the reference's kd-tree traversal order would decide, raise
// BFS_ERR_TIE and the engine replays that one level on the host.

__device__ __forceinline__ int bfs_cell_x(const BfsDev &B, float x) {
  float t = floorf((x - B.gx0) * B.ginv);
  t = fminf(fmaxf(t, 0.0f), (float)(B.GW - 1));
  return (int)t;
}
__device__ __forceinline__ int bfs_cell_y(const BfsDev &B, float y) {
  float t = floorf((y - B.gy0) * B.ginv);
  t = fminf(fmaxf(t, 0.0f), (float)(B.GH - 1));
  return (int)t;
}
__device__ __forceinline__ float bfs_d2(float nx, float ny, float qx, float qy) {
  // the reference's accumulation order: SQ(node.x - q.x) then + SQ(node.y - q.y)  (kdtree.c:339-342)
  float acc = 0.0f;
  acc += (nx - qx) * (nx - qx);
  acc += (ny - qy) * (ny - qy);
  return acc;
}
__device__ __forceinline__ uint32_t bfs_hash(int key) { return fmix32((uint32_t)key * 0x9E3779B1u); }

// insert nodes [first, first+count) into the node grid
__global__ __launch_bounds__(256) void k_bfs_insert_nodes(BfsDev B, int first, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int id = first + i;
  GridCell &c = B.gcell[bfs_cell_y(B, B.ny[id]) * B.GW + bfs_cell_x(B, B.nx[id])];
  const int pos = atomicAdd(&c.cnt, 1);
  if (pos < GRID_SLOTS) {
    c.id[pos] = id;
    c.x[pos] = B.nx[id];
    c.y[pos] = B.ny[id];
  } else {
    atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_GRID_OVERFLOW);
  }
}

__device__ __forceinline__ int outcome_load(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void outcome_store(int *p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// waves per SIMD the speculative-edge kernel is compiled for: 6 (80 registers, 3 spilled) measured best once the
// per-disc ratio division became a branch (4: +0.7 ms, 5: +0.4, 7: see DESIGN, 8: +2.9 -- the LDS tiles allow 30 per CU).
// Measured again with the status-only edge evaluation (GATHER_STATUS: the 18 registers of the moments are gone, but
// the disc sweep is where the registers are short): 6 (80 registers, 5 spilled) is still best -- 7 (72 registers,
// 26 spilled): +0.9 ms per C3 build, 8 (64 registers, 27 spilled): +3.1 ms (profiles/r05_spec_status_ab.txt)
#ifndef SPEC_WAVES_PER_SIMD
#define SPEC_WAVES_PER_SIMD 6
#endif
#ifndef SPEC3_WAVES_PER_SIMD
#define SPEC3_WAVES_PER_SIMD 5  // k_level_spec3 (step-3 builds): more registers in flight
#endif
#ifndef RESOLVE_EARLY_CREATE
#define RESOLVE_EARLY_CREATE 1
#endif
#ifndef TRG_RWV
#define TRG_RWV 8
#endif
constexpr int RW = TRG_RWV * 4;  // sample slots per resolve workgroup (one look-back word per workgroup)
static_assert(256 % RW == 0, "a commit workgroup covers whole resolve groups");

// take the nodes [V0, V1) out of the grid again (they were appended last in their cells)
__global__ void k_bfs_clear_tie(BfsDev B) {
  if (threadIdx.x == 0) {
    atomicAnd(&B.ctrs[BFS_CTR_ERR], ~BFS_ERR_TIE);
    B.ctrs[BFS_CTR_NTIE] = 0;
  }
}

// take a level's commit back: every slot that created a node reserved a place in its grid cell (the
// newest entries of the cell).  Works from the slots' outcomes, so it also serves a launch whose
// numbering never completed (look-back run-out).
__global__ __launch_bounds__(256) void k_bfs_undo_slots(BfsDev B, int slots) {
  // (the next level's expansion ran in between and is void: the repeat of resolve must not take its stamp)
  if (blockIdx.x == 0 && threadIdx.x == 0) B.stats64[STATS64_EXPAND_START] = 0ull;
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= slots) return;
  const int o = B.c_outcome[slot];
  if (o != 3 && o != 4) return;
  const SlotRec &sr = B.slot_rec[slot];
  if ((sr.cls & SLOT_CLS_MASK) != 2) return;
  atomicSub(&B.gcell[bfs_cell_y(B, sr.y) * B.GW + bfs_cell_x(B, sr.x)].cnt, 1);
}

// ---- deferred wireEdge evaluations: node -> already existing node --------------------------------
// list: the call indices to evaluate (record q of the launch is call list[q])
// count_dev != nullptr: count is an upper bound (the launch was issued before the host knew how many
// calls the selection kept), the kernel takes min(count, *count_dev)
__global__ __launch_bounds__(QW *WAVE, EDGE_WAVES_PER_SIMD) void k_calls_gather(MapView m, QueryParams p, BfsDev B,
                                                           const int *list, int count,
                                                           const int *count_dev, DeviceCounters *ctr) {
  __shared__ EdgeLds lds;
  const int w = threadIdx.x >> 6;
  const int q = blockIdx.x * QW + w;
  if (count_dev) count = min(count, *count_dev);
  if (q >= count) return;
  const size_t at = (size_t)list[q];
  if (B.call_status[at] != CALL_PENDING) return;
  const int a = B.call_n1[at], b = B.call_n2[at];
  float *rec = B.mid + (size_t)q * MID_STRIDE;
  // the walk starts at node a: its acceptance disc is the walk's first one (B.ndisc; wave-uniform, kept scalar)
  const int n0 = __builtin_amdgcn_readfirstlane(B.ndisc ? B.ndisc[a] : -1);
  const EdgeMidOut o = edge_gather(m, p, B.nx[a], B.ny[a], B.nz[a], B.nx[b], B.ny[b], B.nz[b],
                                   lds.w[w], rec, ctr, n0);
  store_mid(rec, o, n0);
}

__global__ __launch_bounds__(256) void k_calls_finish(BfsDev B, const int *list, int count,
                                                      const int *count_dev, DeviceCounters *ctr) {
  __shared__ int wave_hits[4], wave_known[4];
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (count_dev) count = min(count, *count_dev);
  const size_t at = (size_t)list[q < count ? q : 0];
  const bool live = q < count && B.call_status[at] == CALL_PENDING;
  const float *r = B.mid + (size_t)(live ? q : 0) * MID_STRIDE;
  const int st_word = live ? __float_as_int(r[0]) : 0;
  const int h = wave_sum(live ? __float_as_int(r[MID_HITS]) : 0);
  const int kn = __popcll(ballot((st_word & MID_START_KNOWN) != 0));  // evaluations that took their first disc as known
  if (lane_id() == 0) {
    wave_hits[threadIdx.x >> 6] = h;
    wave_known[threadIdx.x >> 6] = kn;
  }
  __syncthreads();
  if (threadIdx.x == 0 && ctr) {
    const unsigned long long tot =
        (unsigned long long)(wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3]);
    if (tot) atomicAdd(&ctr[blockIdx.x % COUNTER_SHARDS].edge_hits, tot);
    const unsigned long long tk =
        (unsigned long long)(wave_known[0] + wave_known[1] + wave_known[2] + wave_known[3]);
    if (tk) atomicAdd(&ctr[blockIdx.x % COUNTER_SHARDS].start_known, tk);
  }
  if (!live) return;
  int st = st_word & ~MID_START_KNOWN;
  float w = 0.0f;
  if ((st & EDGE_STATUS_MASK) == EDGE_OK) {
    float cov[3][3];
    mid_covariance(r, cov);
    int clamped = 0;
    w = risk_weight(cov, clamped);
    st |= clamped;
  }
  if (st & EDGE_GATE_UNCERTAIN) {
    const int k = atomicAdd(&B.ctrs[BFS_CTR_NUNC2], 1);
    if (k < BFS_UNC_CAP) {
      const int u = 2 * BFS_UNC_CAP + k;  // third list: the level kernels own the first two
      B.unc_list[u] = (int)at;  // absolute call index
      B.unc_rec[3 * u] = B.nz[B.call_n1[at]];
      B.unc_rec[3 * u + 1] = B.nz[B.call_n2[at]];
      B.unc_rec[3 * u + 2] = r[2];
    }
  }
  B.call_status[at] = st & (EDGE_STATUS_MASK | EDGE_CLAMPED | EDGE_GATE_UNCERTAIN);
  B.call_w[at] = w;
  B.call_dist[at] = r[2];
}

// ---- wireEdge's dedupe + push_back (trg.cpp:255-267, 365-368) as a parallel reduction ----------
// The edge of an unordered pair is created by the FIRST successful call on it in program order, and
// a node's edge list is ordered by the sequence numbers of the calls that created its edges.
__device__ __forceinline__ unsigned long long pair_key(int a, int b) {
  const unsigned lo = (unsigned)min(a, b), hi = (unsigned)max(a, b);
  return ((unsigned long long)lo << 32) | hi;
}
__device__ __forceinline__ uint32_t hash64(unsigned long long k) {
  return fmix32((uint32_t)(k >> 32) * 0x85EBCA6Bu ^ fmix32((uint32_t)k));
}

// Which deferred calls need evaluating at all.  wireEdge returns at once when the pair is already
// wired (trg.cpp:255-267), and a pair's edge comes from its FIRST successful call, so:
//   round 1 evaluates, per unordered pair, only the first call on it in program order;
//   round 2 evaluates every other call of the (few) pairs whose first call failed or could not be
//   called by the device (uncertain slope gate) -- more than the reference strictly evaluates, which
//   is harmless: the finalize pass below keeps the first SUCCESSFUL call of each pair.
// k_first_insert: table pair -> smallest call number over ALL calls of the pair.  Its first thread also zeroes
// *sel_count, the count word of the selection that follows it in the stream (the evaluations of the batch
// before, which read the word, are complete by then: same stream).
__global__ __launch_bounds__(256) void k_first_insert(FinDev F, BfsDev B, long long c0, long long ncalls,
                                                      int *sel_count) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *sel_count = 0;
  const long long i = c0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncalls) return;
  F.call_slot[i] = -1;
  if (B.call_status[i] == CALL_NONE) return;
  // a target created in the same level was recorded as a reference to the creating call
  // (trg_level.inc): from here on the log holds node ids only
  int n2 = B.call_n2[i];
  if (n2 <= -2) {
    n2 = B.newid_of_call[-(long long)n2 - 2];
    B.call_n2[i] = n2;
  }
  const unsigned long long key = pair_key(B.call_n1[i], n2);
  const uint32_t mask = F.ht_size - 1u;
  uint32_t s = hash64(key) & mask;
  for (uint32_t probe = 0; probe < F.ht_size; ++probe) {
    const unsigned long long prev = atomicCAS(&F.ht_key[s], ~0ull, key);
    if (prev == ~0ull || prev == key) {
      atomicMin(&F.ht_seq[s], (int)i);
      F.call_slot[i] = (int)s;
      return;
    }
    s = (s + 1) & mask;
  }
  atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_HASH);
}

// Round-1 selection of the calls [c0, ncalls): per unordered pair the first call on it in program order,
// appended to list in any order (record q of the evaluation is call list[q], and every result is stored under
// its call number); *count = how many (zeroed by k_first_insert).  One atomic per workgroup that selected
// anything: a batch beside the level loop is ~74 workgroups, the whole log after the loop ~30 k.  The same
// thread adds the workgroup's number to *total (instrumentation).
__global__ __launch_bounds__(256) void k_calls_select_append(FinDev F, BfsDev B, long long c0, long long ncalls,
                                                             int *list, int *count, unsigned long long *total) {
  __shared__ int wave_cnt[4];
  __shared__ int wg_base;
  const long long i = c0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool sel = false;
  if (i < ncalls && B.call_status[i] == CALL_PENDING) {
    const int slot = F.call_slot[i];  // (-1: the pair table was full, BFS_ERR_HASH is raised)
    sel = slot >= 0 && F.ht_seq[slot] == (int)i;
  }
  const unsigned long long m = ballot(sel);
  const int w = threadIdx.x >> 6;
  if (lane_id() == 0) wave_cnt[w] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    if (tot) {
      wg_base = atomicAdd(count, tot);
      if (total) atomicAdd(total, (unsigned long long)tot);
    }
  }
  __syncthreads();
  if (!sel) return;
  int rank = __popcll(m & lanemask_lt());
  for (int k = 0; k < w; ++k) rank += wave_cnt[k];
  list[wg_base + rank] = (int)i;
}

// Round-2 selection over the whole call log in one pass: the calls that are NOT the first of their
// pair while that first call failed (or hangs on an uncertain gate) -- a few thousand of ten million --
// appended to list in any order (every result is stored under its call number); *count = how many.
__global__ __launch_bounds__(256) void k_calls_select2_append(FinDev F, BfsDev B, long long ncalls, int *list,
                                                              int *count, unsigned long long *total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool sel = false;
  if (i < ncalls && B.call_status[i] == CALL_PENDING) {
    const int first = F.ht_seq[F.call_slot[i]];
    if (first != (int)i) {
      const int fst = B.call_status[first];  // evaluated in round 1 or speculatively during the BFS
      sel = (fst & EDGE_STATUS_MASK) != EDGE_OK || (fst & EDGE_GATE_UNCERTAIN);
    }
  }
  const unsigned long long m = ballot(sel);
  if (m == 0ull) return;
  int base = 0;
  if (lane_id() == 0) {
    base = atomicAdd(count, __popcll(m));
    if (total) atomicAdd(total, (unsigned long long)__popcll(m));
  }
  base = __shfl(base, 0);
  if (sel) list[base + __popcll(m & lanemask_lt())] = (int)i;
}

// A pair's edge comes from its first SUCCESSFUL call.  Every call already knows its pair's entry of the
// table (k_first_insert), so this needs no second table: one atomicMin per successful call.
__global__ __launch_bounds__(256) void k_fin_insert(FinDev F, BfsDev B, long long ncalls) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncalls) return;
  const int st = B.call_status[i];
  if (st < 0 || (st & EDGE_STATUS_MASK) != EDGE_OK) return;
  const int s = F.call_slot[i];
  if (s < 0) {  // (every call that was evaluated went through k_first_insert)
    atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_HASH);
    return;
  }
  atomicMin(&F.ok_seq[s], (int)i);
}

// The same over the round-2 list alone (plain builds: no step 3).  When a pair's first call succeeded, the edge
// is that call, F.ht_seq[slot], and nothing has to be reduced; ok_seq is needed only for the pairs whose first
// call did not succeed, and then holds the smallest of their OTHER successful calls.  Those are all on the
// round-2 list, because a call that is not the first of its pair can carry EDGE_OK only if round 2 evaluated it.
// Every writer of call_status:
//   k_level_resolve (and its repeat after an undo): CALL_NONE, CALL_PENDING for a merge, and a speculative status
//     for the call that CREATES a node -- the first call of its pair, since the pair's other node did not exist
//     before that slot's turn and every later call has a larger number;
//   the host replay of a level (Build::replay_level): the same three cases, from the same records;
//   the tie patches (Build::settle_ties_in_place): CALL_PENDING / CALL_NONE only; all three write a level's
//     records before its calls are handed to the deferred pipeline;
//   k_calls_finish: the calls of its list -- a round-1 list holds first calls only (k_calls_select_append:
//     F.ht_seq[slot] == i, and later batches only add larger numbers), the other list is round 2's;
//   the gate patches (Build::resolve_uncertain on B.call_status): calls k_calls_finish listed, i.e. evaluated ones;
//   k_node_weights: creating calls, bits outside EDGE_STATUS_MASK (and it runs after these kernels).
// (Step 3 adds calls to the log after the loop; those builds take k_fin_insert over the whole log.)
// INIT: the entries of the listed calls' pairs = INT_MAX (a pass of its own: two listed calls may share a pair);
// then the minimum over the listed calls that succeeded.  No table-wide clear of ok_seq is needed.
template <bool INIT>
__global__ __launch_bounds__(256) void k_fin_insert_listed(FinDev F, BfsDev B, const int *list, int count) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= count) return;
  const int i = list[q];
  const int s = F.call_slot[i];
  if (s < 0) {  // (every listed call went through k_first_insert)
    atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_HASH);
    return;
  }
  if (INIT) {
    F.ok_seq[s] = 0x7FFFFFFF;
    return;
  }
  const int st = B.call_status[i];
  if (st < 0 || (st & EDGE_STATUS_MASK) != EDGE_OK) return;
  atomicMin(&F.ok_seq[s], i);
}

// The calls of one expanded node follow each other in the log and share n1: among the wave's edge lanes, runs
// of neighbours with the same first node take ONE atomic on that node's counter (the run's first lane), and
// their entries land side by side in its row.  rank / cnt: this lane's place in its run and the run's length;
// first: the lane that does the atomic.
struct EdgeRun {
  int rank, cnt, first;
};
__device__ __forceinline__ EdgeRun edge_runs(bool is_edge, int a) {
  const int lane = lane_id();
  const unsigned long long em = ballot(is_edge);
  const unsigned long long below = lanemask_lt();
  const unsigned long long eb = em & below;
  const int prev = eb ? 63 - __clzll((long long)eb) : -1;  // the previous edge lane
  const int pa = __shfl(a, prev < 0 ? lane : prev);
  const unsigned long long heads = ballot(is_edge && (prev < 0 || pa != a));
  const unsigned long long upto = below | (1ull << lane);
  const unsigned long long hb = heads & upto;
  EdgeRun r;
  r.first = hb ? 63 - __clzll((long long)hb) : lane;
  const unsigned long long ha = heads & ~upto;
  const int next = ha ? __ffsll((long long)ha) - 1 : 64;
  const unsigned long long from = ~((1ull << r.first) - 1ull);
  const unsigned long long run = em & from & (next >= 64 ? ~0ull : ((1ull << next) - 1ull));
  r.rank = __popcll(run & below);
  r.cnt = __popcll(run);
  return r;
}

// FIRST_KNOWN (after k_fin_insert_listed): a successful call is its pair's edge iff it is the pair's first call,
// or that first call did not succeed and it is the smallest of the others (ok_seq, valid for exactly those pairs).
template <bool FIRST_KNOWN>
__device__ __forceinline__ bool fin_is_edge(const FinDev &F, const BfsDev &B, int s, int i) {
  if (!FIRST_KNOWN) return F.ok_seq[s] == i;
  const int first = F.ht_seq[s];
  if (first == i) return true;
  const int fst = B.call_status[first];
  return (fst < 0 || (fst & EDGE_STATUS_MASK) != EDGE_OK) && F.ok_seq[s] == i;
}
template <bool FIRST_KNOWN>
__global__ __launch_bounds__(256) void k_fin_count(FinDev F, BfsDev B, long long ncalls) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool edge = false;
  int a = -1, b = -1;
  if (i < ncalls) {
    const int s = F.call_slot[i];
    if (s >= 0) {
      const int st = B.call_status[i];
      if (st < 0 || (st & EDGE_STATUS_MASK) != EDGE_OK || !fin_is_edge<FIRST_KNOWN>(F, B, s, (int)i)) {
        F.call_slot[i] = -1;  // failed, or a later duplicate: no edge
      } else {
        edge = true;
        a = B.call_n1[i];
        b = B.call_n2[i];
      }
    }
  }
  const EdgeRun r = edge_runs(edge, a);
  if (!edge) return;
  if (r.first == lane_id()) atomicAdd(&F.deg[a], r.cnt);
  atomicAdd(&F.deg[b], 1);
}

// WITH_W = false: a build whose cleaned graph takes its weights from call_w afterwards (Build::tail_split,
// FIN_WEIGHTS below) has no reader of F.w: call_w is not read and the two scattered stores per edge are not made.
template <bool WITH_W>
__global__ __launch_bounds__(256) void k_fin_scatter(FinDev F, BfsDev B, long long ncalls) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool edge = i < ncalls && F.call_slot[i] >= 0;
  int a = -1, b = -1;
  float w = 0.0f, d = 0.0f;
  if (edge) {
    a = B.call_n1[i];
    b = B.call_n2[i];
    if (WITH_W) w = B.call_w[i];
    d = B.call_dist[i];
  }
  const EdgeRun r = edge_runs(edge, a);
  int base = 0;
  if (edge && r.first == lane_id()) base = F.rowptr[a] + atomicAdd(&F.fill[a], r.cnt);
  base = __shfl(base, r.first);
  if (!edge) return;
  const int pa = base + r.rank;
  F.col[pa] = b;
  if (WITH_W) F.w[pa] = w;
  F.dist[pa] = d;
  F.seq[pa] = (int)i;
  const int pb = F.rowptr[b] + atomicAdd(&F.fill[b], 1);
  F.col[pb] = a;
  if (WITH_W) F.w[pb] = w;
  F.dist[pb] = d;
  F.seq[pb] = (int)i;
}

__global__ __launch_bounds__(256) void k_fin_rowsort(FinDev F, int V) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const int s = F.rowptr[v], e = F.rowptr[v + 1];
  for (int i = s + 1; i < e; ++i) {
    const int ks = F.seq[i], kc = F.col[i];
    const float kw = F.w[i], kd = F.dist[i];
    int j = i - 1;
    while (j >= s && F.seq[j] > ks) {
      F.seq[j + 1] = F.seq[j];
      F.col[j + 1] = F.col[j];
      F.w[j + 1] = F.w[j];
      F.dist[j + 1] = F.dist[j];
      --j;
    }
    F.seq[j + 1] = ks;
    F.col[j + 1] = kc;
    F.w[j + 1] = kw;
    F.dist[j + 1] = kd;
  }
}

// cleanGraph (trg.cpp:491-535): the new ids follow the iteration order of the reference's node
// container (map_order, known from the node count alone while the GPU still evaluates edges: expanded from
// the container's runs by k_map_order_fill, or by the host and uploaded); a node survives iff it is not
// Invalid and has at least one edge.
// map_order from the container's runs (map_order_runs.h; the list is a kernel argument): the O(V) expansion of
// a few (lo, length, direction) entries, which the host otherwise writes and uploads while the GPU waits for it
__global__ __launch_bounds__(256) void k_map_order_fill(MapOrderRuns R, int V, int *map_order) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= V || k >= R.start[R.n]) return;
  map_order[k] = map_order_at(R, k);
}
__global__ __launch_bounds__(256) void k_fin_keep_flag(FinDev F, BfsDev B, const int *map_order, int V,
                                                       int *flag) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= V) return;
  const int id = map_order[k];
  flag[k] = (B.nstate[id] != -1 && F.rowptr[id + 1] - F.rowptr[id] >= 1) ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_fin_renumber(const int *map_order, const int *flag, const int *pos,
                                                      int V, int *new2old, int *old2new) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= V) return;
  const int id = map_order[k];
  if (flag[k]) {
    new2old[pos[k]] = id;
    old2new[id] = pos[k];
  } else {
    old2new[id] = -1;
  }
}
// row k of the cleaned graph is old node new2old[k] (*vn of them); columns are remapped through old2new
__global__ __launch_bounds__(256) void k_fin_clean_deg(FinDev F, const int *new2old, const int *vn, int V,
                                                       int *deg_new) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= V) return;
  int d = 0;
  if (k < *vn) {
    const int o = new2old[k];
    d = F.rowptr[o + 1] - F.rowptr[o];
  }
  deg_new[k] = d;
}
// The row's edges go out in the order the reference pushed them (the call number, F.seq): the scatter
// left them in arrival order, and each entry's place is the number of entries of its row with a
// smaller call number (rows are ~10 entries; no sorting pass over the whole edge list is needed).
// One 16-lane group per node, one entry per lane and pass: every entry is loaded once (a thread per node
// that walked its row once per entry fetched 1.5-3 GB from HBM for 0.1 GB of entries -- the rows of a wave
// are scattered and do not survive in the L2 between two walks).
// PARTS: what a launch writes.  FIN_ALL is the whole cleaned graph.  A build whose creating-edge weights are
// computed beside the copy of the cleaned graph to the host (Build::clean_and_fetch) launches FIN_STRUCTURE
// first -- everything but w, none of which depends on a weight -- and FIN_WEIGHTS once k_node_weights has run:
// the same traversal and ranks, w alone, taken from the call that made the entry (F.seq; F.w holds what
// k_fin_scatter saw, which is older than k_node_weights there).
// FIN_STRUCTURE is two parts of its own: FIN_NODES (xyz, state: they need the renumbering only, not the rows, so a
// build that sends the node arrays to the host early launches them alone, a thread per node, in front of
// k_fin_scatter) and FIN_EDGES (col, dist).
enum : int { FIN_WEIGHTS = 1, FIN_EDGES = 2, FIN_NODES = 4, FIN_STRUCTURE = FIN_EDGES | FIN_NODES, FIN_ALL = 7 };
constexpr int FIN_ROW = 16;
template <int PARTS>
__global__ __launch_bounds__(256) void k_fin_clean_copy(FinDev F, BfsDev B, const int *new2old,
                                                        const int *old2new, const int *vn,
                                                        const int *rowptr_new, int *col, float *w,
                                                        float *dist, float *xyz, int *state) {
  constexpr int LANES = PARTS == FIN_NODES ? 1 : FIN_ROW;  // lanes per node
  const int k = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) / LANES);
  const int l = threadIdx.x % LANES;
  if (k >= *vn) return;  // (whole groups leave together)
  const int o = new2old[k];
  if ((PARTS & FIN_NODES) && l == 0) {
    xyz[3 * k] = B.nx[o];
    xyz[3 * k + 1] = B.ny[o];
    xyz[3 * k + 2] = B.nz[o];
    state[k] = B.nstate[o];
  }
  if (PARTS == FIN_NODES) return;
  const int dst0 = rowptr_new[k];
  const int e0 = F.rowptr[o], e1 = F.rowptr[o + 1];
  for (int base = e0; base < e1; base += FIN_ROW) {
    const int e = base + l;
    const bool have = e < e1;
    const int ks = have ? F.seq[e] : 0x7FFFFFFF;
    int rank = 0;
    for (int b2 = e0; b2 < e1; b2 += FIN_ROW) {
      const int other = (b2 + l < e1) ? (b2 == base ? ks : F.seq[b2 + l]) : 0x7FFFFFFF;
#pragma unroll
      for (int j = 0; j < FIN_ROW; ++j) rank += __shfl(other, j, FIN_ROW) < ks;
    }
    if (have && (PARTS & FIN_EDGES)) {
      const int nc = old2new[F.col[e]];
      if (nc < 0) atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_CLEAN);
      col[dst0 + rank] = nc;
      dist[dst0 + rank] = F.dist[e];
    }
    if (have && PARTS == FIN_ALL) w[dst0 + rank] = F.w[e];
    if (have && PARTS == FIN_WEIGHTS) w[dst0 + rank] = B.call_w[ks];
  }
}
