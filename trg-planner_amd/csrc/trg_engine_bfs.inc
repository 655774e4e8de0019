// trg_engine_bfs.inc -- host driver of the device-resident TRG build (included by trg_engine.cpp).
//
// initGraph for configurations whose expandGraph step 3 is disabled (mountain.yaml): the whole BFS
// (trg.cpp:372-454), every wireEdge evaluation, wireEdge's dedupe/push order and cleanGraph's
// compaction run on the GPU; the host launches one batch of kernels per BFS level, reads back a
// handful of counters, decides the (rare) slope gates the device flagged as too close to call with
// the reference's own libm, and computes cleanGraph's renumbering with the same
// std::unordered_map the reference iterates.

namespace {

// Everything the expansion (k_level_sample + k_level_spec) writes exists twice (level parity): the next level is expanded while the
// host still looks at the counters of this one, and a level whose second half has to be redone must
// find its first half untouched.
struct LevelSet {
  DevArr node_rec;   // NodeRec per frontier node
  DevArr slot_rec;   // SlotRec per sample slot
  DevArr c_outcome;  // int per sample slot
  DevArr lv_hash;    // HashEnt table
  DevArr resc;       // RescueRec per sample slot (builds with expandGraph's step 3 only)
  void apply(BfsDev &B) const {
    B.node_rec = (NodeRec *)node_rec.p;
    B.slot_rec = (SlotRec *)slot_rec.p;
    B.c_outcome = (int *)c_outcome.p;
    B.lv_hash = (HashEnt *)lv_hash.p;
    B.resc = use_resc ? (RescueRec *)resc.p : nullptr;
  }
  bool use_resc = false;
};

// pinned words of h_ctrs behind the level counters (BFS_CTR_*) in the same 64-int block
constexpr int H_CLEAN_TOTALS = 32;  // 2 words: nodes and edges that survive cleanGraph
constexpr int H_ROUND2_CALLS = 34;  // calls round 2 of the deferred evaluations selected
constexpr int H_STEP3_LEFT = 40;    // step 3's device node tree: nodes not yet placed
constexpr int H_STATS64 = 64;       // 16 x 64 bit: the first words of B.stats64 (report_stats)
constexpr int H_CTRS_WORDS = 96;
static_assert(BFS_CTR_COUNT <= H_CLEAN_TOTALS && H_CLEAN_TOTALS + 2 <= H_ROUND2_CALLS &&
                  H_ROUND2_CALLS < H_STEP3_LEFT && H_STEP3_LEFT < H_STATS64 && H_STATS64 % 2 == 0 &&
                  H_STATS64 + 32 <= H_CTRS_WORDS,
              "pinned words overlap");

// words of B.stats64 the host reads: calls the deferred selections kept, longest resolve wait, rows that went
// multi-pass; then launch_bfs_stats's draws, samples, map points inside sampling discs and inside
// speculative-edge queries, speculative parent edges (candidates) and the map points of the parent edges of
// created nodes; the start stamp of the expansion in flight and the wall-clock ticks of all expansions so far
// (k_level_sample / k_level_resolve); from S64_PHASES 1024 shards x 8 phases of cycles (profiling builds)
enum : int {
  S64_SPEC_KNOWN = STATS64_SPEC_KNOWN /* 4: the word in front of the block below, filled by launch_bfs_stats too */,
  S64_DEF_KEPT = 5, S64_MAX_SPIN, S64_MULTIPASS, S64_DRAWS, S64_SAMPLES, S64_DISC_HITS, S64_SPEC_HITS,
  S64_CANDIDATES, S64_PARENT_HITS, S64_EXPAND_START = STATS64_EXPAND_START, S64_EXPAND_TICKS = STATS64_EXPAND_TICKS,
  S64_PHASES = 16, S64_WORDS = 16 + 1024 * 8
};
static_assert(S64_SPEC_KNOWN < S64_DEF_KEPT && S64_PARENT_HITS < S64_EXPAND_START && S64_EXPAND_START < S64_EXPAND_TICKS && S64_EXPAND_TICKS < S64_PHASES,
              "report_stats fetches the words in front of S64_PHASES");

struct BfsBuffers {
  BfsDev B{};
  FinDev F{};
  LevelSet lv[2];
  // the arrays behind B's views (the frontier pair swaps its views level by level)
  DevArr nx, ny, nz, nstate, ndisc, gcell, ncov, nexp, nhits, front0, front1, fxy0, fxy1;
  DevArr mid, unc_list, unc_rec, mt_rec, ctrs, stats64, wg_state, c_cell, tl, scan_tmp, s3_scratch;
  DevArr call_n1, call_n2, call_status, call_w, call_dist, newid_of_call, call_slot;  // the call log
  // selection of the deferred calls that need evaluating: the index list; def_counts: round 2's count, then the
  // count of the round-1 batch in flight
  DevArr sel_list, def_counts;
  // finalize: pair table, CSR in creation order, cleanGraph's renumbering and the cleaned graph
  DevArr ht_key, ht_seq, ok_seq, deg, fill, rowptr, col, seq, w, dist;
  DevArr map_order, keep_flag, keep_pos, new2old, old2new, deg_new, rowptr_new, col2, w2, dist2, xyz2, state2;
  Pinned<int> h_ctrs;  // pinned, device-visible: the counters of a level, its stamp in words 5 and 15
  int stamp_serial = 0;
  // host mirror of the nodes [0, hm_state.size()): states and positions, fetched from the device when a
  // rare event needs them; it only holds nodes of levels that are final or being examined.  Pinned (late in a
  // build a fetch is megabytes) and kept from build to build: clear() leaves the capacity.
  PVec<int> hm_state;
  PVec<float> hm_x, hm_y;
  // pinned staging of the tie repairs: records fetched from / patches sent to the device in one batch of
  // asynchronous copies with a single wait
  PVec<SlotRec> st_slot;
  PVec<int> st_int;
  std::vector<int> rp_stamp, rp_head;  // replay_level: cell -> newest node this replay created
  int rp_serial = 0;
  unsigned long long nodes_created = 0, nodes_invalid = 0;  // by the levels that became final
};

// The stream of the tie repairs' batched copies.  Like the synchronous copies they replace they are not ordered
// behind the main stream, which may hold the next level's expansion: what they read is final since the level's
// stamp arrived, what they write is read by launches the host issues after the wait.
inline hipStream_t repair_stream(TrgEngine *e) { return e->s_aux; }

// the host mirror grown to the nodes [0, n): three copies into pinned memory, one wait
TrgStatus mirror_nodes(TrgEngine *e, BfsBuffers &bb, int n) {
  const size_t at = bb.hm_state.size();
  if ((size_t)n <= at) return TRG_OK;
  const size_t k = (size_t)n - at;
  bb.hm_state.resize(n);
  bb.hm_x.resize(n);
  bb.hm_y.resize(n);
  const hipStream_t st = repair_stream(e);
  HIPCHK(e, hipMemcpyAsync(bb.hm_state.data() + at, bb.B.nstate + at, k * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(e, hipMemcpyAsync(bb.hm_x.data() + at, bb.B.nx + at, k * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(e, hipMemcpyAsync(bb.hm_y.data() + at, bb.B.ny + at, k * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(e, hipStreamSynchronize(st));
  return TRG_OK;
}

// squared distance in the reference's accumulation order (kdtree.c:339-342)
inline float ref_d2(float x, float y, float qx, float qy) {
  float acc = 0;
  acc += (x - qx) * (x - qx);
  acc += (y - qy) * (y - qy);
  return acc;
}

// The host's nearest node to a slot's sample as the reference finds it: the pre-level node
// k_level_sample found (all pre-level nodes that far when it carries SLOT_TIE), then the nodes the level
// created before the slot's turn, offered one by one.  Exact ties go to the kd-tree's visiting order
// (kd_tie_winner, host_index.h).  Positions come from the host mirror.
struct Nearest {
  int nn = -1;
  float best = INFINITY;
  std::vector<int> tied;
  void start(const BfsBuffers &bb, const SlotRec &sr, int V0) {
    nn = sr.nn0;
    best = nn >= 0 ? sr.d0sq : INFINITY;
    tied.clear();
    if (nn >= 0 && (sr.cls & SLOT_TIE)) {
      for (int i = 0; i < V0; ++i)
        if (ref_d2(bb.hm_x[i], bb.hm_y[i], sr.x, sr.y) == best) tied.push_back(i);
    } else if (nn >= 0) {
      tied.push_back(nn);
    }
  }
  void offer(const BfsBuffers &bb, int id, float qx, float qy) {
    const float dd = ref_d2(bb.hm_x[id], bb.hm_y[id], qx, qy);
    if (dd < best) {
      best = dd;
      nn = id;
      tied.assign(1, id);
    } else if (dd == best) {
      tied.push_back(id);
    }
  }
  bool tie() const { return tied.size() > 1; }
  // the reference's answer among the nodes [0, V_at)
  int winner(const BfsBuffers &bb, int V_at, float qx, float qy) {
    if (!tie()) return nn;
    std::sort(tied.begin(), tied.end());
    return kd_tie_winner(bb.hm_x.data(), bb.hm_y.data(), V_at, qx, qy, tied);
  }
};

constexpr int BFS_FCAP = 1 << 16;       // nodes per BFS level the device path accepts
constexpr int CALL_EVAL_BATCH = 1 << 22;  // calls per selection / evaluation chunk (sizes the edge scratch)
// repaired by replaying ONE level on the host (or, for a tie among pre-level nodes only, by handing
// k_level_resolve the reference's winner)
constexpr int BFS_ERR_SOFT = BFS_ERR_TIE | BFS_ERR_STALL | BFS_ERR_TIE_CLS;
// calls per batch (at least): about one batch per BFS level -- many small batches disturb the level
// kernels least (measured: 3.2 M -> 54.6 ms per C3 build, 100 k -> 53.2, 6 k -> 51.6; no overlap 54.5)
constexpr long long DEF_BATCH_MIN = 6000;

std::string err_text(int code) {
  std::string t;
  if (code & BFS_ERR_GRID_OVERFLOW) t += "grid-cell overflow;";
  if (code & BFS_ERR_NB_OVERFLOW) t += "neighbour list overflow;";
  if (code & BFS_ERR_VCAP) t += "node capacity;";
  if (code & BFS_ERR_TIE) t += "exact fp32 distance tie (kd-tree order decides);";
  if (code & BFS_ERR_TIE_CLS) t += "exact fp32 distance tie among pre-level nodes;";
  if (code & BFS_ERR_HASH) t += "hash table full;";
  if (code & BFS_ERR_LEVEL_TOO_BIG) t += "BFS level too large;";
  if (code & BFS_ERR_CLEAN) t += "clean remap;";
  if (code & BFS_ERR_STALL) t += "resolve stalled;";
  if (code & BFS_ERR_LOOKBACK) t += "commit look-back ran out (another process on the GPU?);";
  if (code & BFS_ERR_STEP3) t += "step 3: neighbour list / call stride overflow or an uncertain slope gate;";
  return t;
}

// test hook: pretend a tie was seen so that the undo + host-level replay are exercised on data that has
// no real tie
bool debug_tie_level(const TrgEngine *e, int level) {
  return e->debug_tie_every > 0 && level > 0 && level % e->debug_tie_every == 0;
}

int hash_size(size_t nodes, int S) {
  int ht = 1024;
  while ((size_t)ht < 2 * nodes * (size_t)S) ht <<= 1;
  return ht;
}

// one BFS level as the host sees it
struct Level {
  int index, parity, mcur, V0;
  size_t slots;
  long long call_base;
  int tag, unc_ctr;  // the hash tag of the level's expansion, the counter of this parity's uncertain gates
  // from the counters
  int err = 0, err_from_sample = 0, mnext = 0, v_after = 0, n_unc = 0, n_mt = 0;
  bool reexpand = false;  // the level's commit was redone: the next level's expansion is void
  bool undone = false;    // the commit is taken back and not yet redone
  bool replayed = false;  // replayed on the host (which counted its own nodes)
  // map-point tie records of candidates that the commit that stands did not make nodes: their elevation is read
  // by nobody and was left as the device picked it.  A rerun of resolve + commit or a host replay of the level
  // may create other nodes, so either repairs them first (repair_skipped_map_ties).
  std::vector<MapTieRec> mt_skipped;
  std::string repairs;  // what repair_level did, for its trace line
};

// One device build: what its phases share, the phases and the steps of a level.
struct Build {
  TrgEngine *e;
  BfsBuffers &bb;
  BfsDev &B;
  FinDev &F;
  DevMap &m;
  const QueryParams qp;
  const hipStream_t s;
  const int S;
  // call-log entries per sample slot: with expandGraph's step 3 on, every slot's own call is followed by room
  // for the neighbour calls of the node it creates (debug_call_stride: the sparse log on any configuration)
  const int CS;
  size_t calls_bound = 0;
  unsigned fht = 0;       // pair-table size
  bool overlap = false;   // deferred evaluations beside the level loop, on s_def
  hipStream_t s_def = nullptr;
  unsigned ticket_base = 0;  // the host's count of the resolve start tickets drawn so far
  bool unc_changed = false;  // resolve_uncertain: a provisional "not gated" turned out to be gated
  int res_epoch = 0;         // one per k_level_resolve launch: the look-back words of other launches do not count
  int levels = 0, V = 1;  // results of the level loop
  long long ncalls = 0;
  // deferred wireEdge evaluations
  long long def_lo = 0;  // first call not yet handed to the deferred pipeline
  int nsel2 = 0;         // calls round 2 kept: sel_list[0, nsel2) until the build ends
  size_t n_eval_batches = 0;
  std::vector<std::pair<Event, Event>> def_events;
  Event ev_order, ev_nodes, ev_structure, ev_weights;
  // The tail as two resources.  The weights of the edges that created the nodes (k_node_cov, k_node_weights)
  // feed ONE array of the result, w: with tail_split they run on the second stream beside the copies of the
  // other six arrays to the host, and w follows as the last copy (clean_and_fetch).  Without it (builds with
  // step 3, whose neighbour calls go between the weights and the deferred pipeline; keep_preclean, which
  // downloads F.w; option tail_overlap=0) they run in the main stream in front of the deferred calls.
  bool tail_split = false;
  // ... and three with early_copy (option tail_early_copy, tail_split builds): the link is the tail's floor, so
  // the copies start as early as their sources exist.  xyz, state, cid and rowptr need the degrees and the
  // renumbering only: they are laid out in front of k_fin_scatter and travel on a copy stream of their own
  // (copy_stream()) while the main stream fills and orders the rows; col / dist follow behind ev_structure and
  // w behind ev_weights.  The host learns the sizes from ev_totals, not from a drained stream.
  bool early_copy = false;
  Event ev_node_arrays, ev_totals;
  hipStream_t copy_stream() const { return e->s_aux; }  // (idle in the tail: the level loop's rare events own it)
  bool edge_stream_busy = false;  // the second stream (and the copy stream) was given work of the tail that nothing has waited for yet
  Clock::time_point t_fin;  // finalize: its start, TRG_TIMING set
  bool trace_fin = false;

  explicit Build(TrgEngine *e_)
      : e(e_), bb(*e_->bfs), B(bb.B), F(bb.F), m(e_->gmap), qp(qparams(e_)), s(e_->s_main),
        S(e_->prm.sample_num), CS((e_->step3 || e_->debug_call_stride) ? LEVEL_STEP3_STRIDE : 1),
        tail_split(e_->tail_overlap && !e_->step3 && !e_->keep_preclean),
        early_copy(tail_split && e_->tail_early_copy) {}
  // Whichever way a build ends, nothing of its tail stays in flight: a return between the hand-over to the
  // second stream and the last synchronisation (an error, a fallback to the host replay, which reuses these
  // buffers) leaves both streams drained.
  ~Build() {
    if (!edge_stream_busy) return;
    (void)hipStreamSynchronize(e->s_edge);
    (void)hipStreamSynchronize(s);
    if (early_copy) (void)hipStreamSynchronize(copy_stream());
  }
  Build(const Build &) = delete;
  Build &operator=(const Build &) = delete;
  TrgStatus fallback(const std::string &why) {
    e->bfs_fallback_reason = why;
    return TRG_ERR_CAPACITY;
  }
  void lap(const char *what) {
    if (!trace_fin) return;
    (void)hipStreamSynchronize(s);
    if (edge_stream_busy) (void)hipStreamSynchronize(e->s_edge);
    if (edge_stream_busy && early_copy) (void)hipStreamSynchronize(copy_stream());
    fprintf(stderr, "[trg finalize] %-28s %8.3f ms\n", what, ms_since(t_fin));
  }
  void mark(const char *what) {  // host time only: the stream keeps running
    if (trace_fin) fprintf(stderr, "[trg finalize]   (host) %-20s %8.3f ms\n", what, ms_since(t_fin));
  }
  // phases
  TrgStatus allocate();
  TrgStatus seed_root(float root_x, float root_y, float root_z);
  TrgStatus level_loop();
  TrgStatus finish_deferred();
  TrgStatus assemble_csr();
  TrgStatus clean_and_fetch();
  TrgStatus report_stats();
  // steps of a level and of the deferred pipeline
  TrgStatus read_ctrs();
  TrgStatus wait_stamp(int stamp);
  void read_level(Level &lv, bool first);
  TrgStatus repair_level(Level &lv);
  TrgStatus undo_level(Level &lv);
  TrgStatus redo_commit(Level &lv, bool decide_gates = false, bool ticketed = false, int hook = 0);
  TrgStatus fix_map_ties(Level &lv);
  TrgStatus repair_map_tie(const MapTieRec &r, SlotRec &sr, bool *z_changed);
  TrgStatus repair_skipped_map_ties(Level &lv);
  TrgStatus fix_pre_level_ties(Level &lv);
  TrgStatus settle_ties_in_place(Level &lv);
  TrgStatus replay_level(Level &lv);
  TrgStatus resolve_uncertain(int n_unc, void *status_base, size_t stride, int list_parity, int ctr_index,
                              bool slot_records = false);
  TrgStatus grow_call_log(size_t need);
  TrgStatus launch_deferred(long long c1, bool in_loop);
  void launch_creating_edge_weights(hipStream_t st);
};

TrgStatus Build::read_ctrs() {
  HIPCHK(e, hipMemcpyAsync(bb.h_ctrs, B.ctrs, BFS_CTR_COUNT * sizeof(int), hipMemcpyDeviceToHost, s));
  auto t0 = Clock::now();
  HIPCHK(e, hipStreamSynchronize(s));
  e->stats.ms_wait_gpu += ms_since(t0);
  return TRG_OK;
}

// The level's counters reach the host without a copy in the stream: the first workgroup of the next
// level's k_level_sample writes them into pinned host memory with the level's stamp; the host polls the
// stamp.
TrgStatus Build::wait_stamp(int stamp) {
  constexpr long poll_query_mask = 0xFFFFFL;
  auto t0 = Clock::now();
  volatile int *hv = bb.h_ctrs;
  long spins = 0;
  while (hv[BFS_CTR_DONE] != stamp || hv[BFS_CTR_COUNT - 1] != stamp) {
    if ((++spins & poll_query_mask) == 0) {
      // the kernels may have failed to launch or the queue may be gone: do not spin forever.  (Rarely:
      // a stream query makes the runtime put a marker behind the last kernel, and the next level's
      // first kernel then starts ~6 us late.)
      const hipError_t q = hipStreamQuery(s);
      if (q != hipErrorNotReady && q != hipSuccess)
        return e->fail(TRG_ERR_DEVICE, std::string("level kernels: ") + hipGetErrorString(q));
      if (q == hipSuccess && hv[BFS_CTR_DONE] != stamp && spins > (1L << 24))
        return e->fail(TRG_ERR_DEVICE, "level counters were not published");
    }
    __builtin_ia32_pause();
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  e->stats.ms_wait_gpu += ms_since(t0);
  return TRG_OK;
}

// The level's result from the counter block, on the first read after wait_stamp and after every rerun of
// resolve + commit.  What k_level_sample reported stays true (that kernel does not run again); so do the
// expansion's counts of uncertain gates and map-point ties, which an undo clears.
void Build::read_level(Level &lv, bool first) {
  const int *h = bb.h_ctrs;
  lv.err = h[BFS_CTR_ERR] | lv.err_from_sample;
  if (debug_tie_level(e, lv.index)) lv.err |= BFS_ERR_TIE;
  lv.mnext = h[BFS_CTR_MNEXT];
  lv.v_after = h[BFS_CTR_V];
  if (!first) return;
  lv.err_from_sample = lv.err & BFS_ERR_TIE_CLS;
  lv.n_unc = h[lv.unc_ctr];
  lv.n_mt = h[BFS_CTR_NMAPTIE + lv.parity];
}

// host decision of the slope gates the device could not call (reference libm, trg.cpp:269-274);
// list: the parity's half of unc_list / unc_rec, entries index status_array.  slot_records: the entries are
// SlotRecs, whose hits word counts the queries of the evaluation the device ran in case the gate is open; behind a
// closed gate the reference makes none (trg.cpp:269-276), and the node such a slot creates must count none.
TrgStatus Build::resolve_uncertain(int n_unc, void *status_base, size_t stride, int list_parity, int ctr_index,
                                   bool slot_records) {
  unc_changed = false;
  if (n_unc > BFS_UNC_CAP) return fallback("too many uncertain slope gates in one batch");
  std::vector<int> unc_idx(n_unc);
  std::vector<float> unc_rec(3 * (size_t)n_unc);
  HIPCHK(e, hipMemcpy(unc_idx.data(), B.unc_list + (size_t)list_parity * BFS_UNC_CAP, n_unc * sizeof(int),
                      hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(unc_rec.data(), B.unc_rec + (size_t)list_parity * 3 * BFS_UNC_CAP,
                      3 * (size_t)n_unc * sizeof(float), hipMemcpyDeviceToHost));
  for (int k = 0; k < n_unc; ++k) {
    int stt = 0;
    char *addr = (char *)status_base + (size_t)unc_idx[k] * stride;
    HIPCHK(e, hipMemcpy(&stt, addr, sizeof(int), hipMemcpyDeviceToHost));
    e->stats.gate_uncertain++;
    if (host_slope_gate(e, unc_rec[3 * k], unc_rec[3 * k + 1], unc_rec[3 * k + 2])) {
      stt = EDGE_GATE;
      unc_changed = true;
      if (slot_records) {
        const int none = 0;
        HIPCHK(e, hipMemcpy(addr - offsetof(SlotRec, status) + offsetof(SlotRec, hits), &none, sizeof(int),
                            hipMemcpyHostToDevice));
      }
    } else {
      stt &= ~EDGE_GATE_UNCERTAIN;
    }
    HIPCHK(e, hipMemcpy(addr, &stt, sizeof(int), hipMemcpyHostToDevice));
  }
  const int zero = 0;
  HIPCHK(e, hipMemcpy(B.ctrs + ctr_index, &zero, sizeof(int), hipMemcpyHostToDevice));
  return TRG_OK;
}

// the level's commit taken back: its nodes leave the grid, its outcomes are undecided again
TrgStatus Build::undo_level(Level &lv) {
  lv.reexpand = true;
  lv.undone = true;
  HIPCHK(e, hipStreamSynchronize(s));  // the next level's expansion (now void) must be out of the way
  // whatever follows an undo -- resolve + commit again, the host's replay -- decides anew who creates a node
  const TrgStatus st_mt = repair_skipped_map_ties(lv);
  if (st_mt != TRG_OK) return st_mt;
  launch_bfs_undo_slots(B, (int)lv.slots, s);
  // k_level_resolve polls outcomes: a rerun must find them undecided again
  HIPCHK(e, hipMemsetAsync(B.c_outcome, 0, lv.slots * sizeof(int), s));
  int ctr_host[BFS_CTR_COUNT] = {0};
  ctr_host[BFS_CTR_V] = lv.V0;
  HIPCHK(e, hipMemcpy(B.ctrs, ctr_host, BFS_CTR_NUNC2 * sizeof(int), hipMemcpyHostToDevice));  // (the deferred pipeline owns NUNC2)
  if ((int)bb.hm_state.size() > lv.V0) {  // the host mirror keeps the nodes of earlier levels only
    bb.hm_state.resize(lv.V0);
    bb.hm_x.resize(lv.V0);
    bb.hm_y.resize(lv.V0);
  }
  return TRG_OK;
}

// Undo, resolve + commit again, fall back on a hard error.  decide_gates: the level's uncertain gates are
// decided in between; ticketed: the resolve workgroups take start tickets (hook: the repeat's test hook).
TrgStatus Build::redo_commit(Level &lv, bool decide_gates, bool ticketed, int hook) {
  TrgStatus st;
  if ((st = undo_level(lv)) != TRG_OK) return st;  // (also clears the tie / gate counters)
  if (decide_gates && lv.n_unc > 0) {
    void *status = (char *)B.slot_rec + offsetof(SlotRec, status);
    if ((st = resolve_uncertain(std::min(lv.n_unc, BFS_UNC_CAP), status, sizeof(SlotRec), lv.parity, lv.unc_ctr,
                                true)) != TRG_OK)
      return st;
    lv.n_unc = 0;
  }
  launch_level_resolve_commit(B, qp, lv.mcur, TRG_NODE_VALID, lv.call_base, lv.V0, lv.tag, ++res_epoch,
                              s, hook, ticketed || e->resolve_tickets != 0, &ticket_base);
  if ((st = read_ctrs()) != TRG_OK) return st;  // (rare path: a plain copy)
  read_level(lv, false);
  lv.undone = false;
  if (lv.err & ~BFS_ERR_SOFT) return fallback(err_text(lv.err));
  return TRG_OK;
}

// accepted samples whose elevation hung on a nearest-map-point tie: the device took the lowest cloud
// index; fetch the reference's choice and, if a z changed, re-evaluate that sample's speculative edge and
// redo resolve + commit (sample positions and classes do not depend on z)
//
// Only where that elevation is read (option lazy_tie_repair, the default).  A sample's z is the z of the node
// it creates and the end of that node's parent edge -- nothing else.  A class-1 slot has a pre-level node
// within robot_size: it merges or is skipped, never creates.  A candidate that the commit decided as 1 or 2
// did not create either, and its speculative edge reached other slots only as "would be Invalid if created".
// Such records get no lookup.  One candidate record whose slot created a node repairs every candidate record
// of the level, since the rerun may let another of them create.
TrgStatus Build::fix_map_ties(Level &lv) {
  TrgStatus st;
  if ((size_t)lv.n_mt > lv.slots) return e->fail(TRG_ERR_DEVICE, "more map-tie records than the level has slots");
  std::vector<MapTieRec> recs((size_t)lv.n_mt);
  HIPCHK(e, hipMemcpy(recs.data(), B.mt_rec + (size_t)lv.parity * B.mt_cap, recs.size() * sizeof(MapTieRec),
                      hipMemcpyDeviceToHost));
  e->stats.map_tie_records += recs.size();
  std::vector<SlotRec> srs(recs.size());
  for (size_t k = 0; k < recs.size(); ++k)
    if (recs[k].slot < 0 || (size_t)recs[k].slot >= lv.slots)
      return e->fail(TRG_ERR_DEVICE, "map-tie record of a slot outside the level");
  if (recs.size() * 8 >= lv.slots) {
    // a level where ties are the rule (a twinned cloud): the level's slot records in one copy, not one copy a record
    std::vector<SlotRec> all(lv.slots);
    HIPCHK(e, hipMemcpy(all.data(), B.slot_rec, lv.slots * sizeof(SlotRec), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < recs.size(); ++k) srs[k] = all[recs[k].slot];
  } else {
    for (size_t k = 0; k < recs.size(); ++k)
      HIPCHK(e, hipMemcpy(&srs[k], B.slot_rec + recs[k].slot, sizeof(SlotRec), hipMemcpyDeviceToHost));
  }
  std::vector<char> repair(recs.size(), 1);
  if (e->lazy_tie_repair) {
    // the outcomes of the candidates among them, from the commit that stands: one batch of copies, one wait
    std::vector<size_t> cand;
    for (size_t k = 0; k < recs.size(); ++k)
      if ((srs[k].cls & SLOT_CLS_MASK) == 1) repair[k] = 0;
      else cand.push_back(k);
    bb.st_int.resize(cand.size());
    const hipStream_t sr_ = repair_stream(e);
    for (size_t q = 0; q < cand.size(); ++q)
      HIPCHK(e, hipMemcpyAsync(bb.st_int.data() + q, B.c_outcome + recs[cand[q]].slot, sizeof(int),
                               hipMemcpyDeviceToHost, sr_));
    if (!cand.empty()) HIPCHK(e, hipStreamSynchronize(sr_));
    bool any_reads_z = false;  // (an outcome that is not final -- a stalled resolve -- counts as one that may create)
    for (size_t q = 0; q < cand.size(); ++q) any_reads_z |= bb.st_int[q] != 1 && bb.st_int[q] != 2;
    if (!any_reads_z)
      for (size_t k : cand) {
        repair[k] = 0;
        lv.mt_skipped.push_back(recs[k]);
      }
  }
  bool z_changed = false;
  size_t unread = 0;
  for (size_t k = 0; k < recs.size(); ++k) {
    if (!repair[k])
      unread++;
    else if ((st = repair_map_tie(recs[k], srs[k], &z_changed)) != TRG_OK)
      return st;
  }
  e->stats.map_tie_unread += unread;
  lv.repairs += " fix_map_ties(" + std::to_string(recs.size() - unread) + " of " + std::to_string(recs.size()) +
                (z_changed ? " looked up, z_changed)" : " looked up)");
  if (z_changed)
    // the level's uncertain gates are decided before the second half runs again (the entry of a
    // re-evaluated slot is stale but harmless: its status no longer carries the flag)
    return redo_commit(lv, true);
  const int zero = 0;
  HIPCHK(e, hipMemcpy(B.ctrs + BFS_CTR_NMAPTIE + lv.parity, &zero, sizeof(int), hipMemcpyHostToDevice));
  return TRG_OK;
}

// one record: the reference's elevation and, for a candidate, its parent edge with it; sr is the slot's record
TrgStatus Build::repair_map_tie(const MapTieRec &r, SlotRec &sr, bool *z_changed) {
  TrgStatus st;
  float z_exact = 0;
  bool found = false;
  if ((st = map_nn_exact(e, m, r.qx, r.qy, &z_exact, &found)) != TRG_OK) return st;
  if (!found || z_exact == sr.z) return TRG_OK;
  sr.z = z_exact;
  *z_changed = true;
  if ((sr.cls & SLOT_CLS_MASK) == 2) {
    // the candidate's parent edge with the corrected elevation (position-only part of wireEdge)
    int parent = 0;
    float p1[3], p2[3] = {r.qx, r.qy, z_exact}, wgt = 0, dd = 0;
    HIPCHK(e, hipMemcpy(&parent, B.front_cur + r.slot / S, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(&p1[0], B.nx + parent, sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(&p1[1], B.ny + parent, sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(&p1[2], B.nz + parent, sizeof(float), hipMemcpyDeviceToHost));
    int32_t raw = 0;
    if ((st = edges_sync(e, e->gmap, p1, p2, 1, &raw, nullptr, &wgt, &dd, false)) != TRG_OK) return st;
    if (raw & EDGE_GATE_UNCERTAIN) {
      e->stats.gate_uncertain++;
      raw = host_slope_gate(e, p1[2], p2[2], dd) ? EDGE_GATE : (raw & ~EDGE_GATE_UNCERTAIN);
    }
    if ((raw & EDGE_STATUS_MASK) != EDGE_OK) wgt = 0.0f;
    if ((raw & EDGE_STATUS_MASK) == EDGE_GATE) sr.hits = 0;  // (behind a closed gate the reference makes no query)
    sr.status = raw;
    sr.dist = dd;
    sr.cov[0] = wgt;  // the weight itself (already clamped): k_node_weights takes it as given
    sr.w_given = 1;
  }
  HIPCHK(e, hipMemcpy(B.slot_rec + r.slot, &sr, sizeof(SlotRec), hipMemcpyHostToDevice));
  return TRG_OK;
}

// the records fix_map_ties left alone, repaired after all: the level's commit is about to be decided again.
// The caller has drained the main stream (edges_sync runs there).
TrgStatus Build::repair_skipped_map_ties(Level &lv) {
  if (lv.mt_skipped.empty()) return TRG_OK;
  TrgStatus st;
  bool z_changed = false;
  for (const MapTieRec &r : lv.mt_skipped) {
    SlotRec sr;
    HIPCHK(e, hipMemcpy(&sr, B.slot_rec + r.slot, sizeof(SlotRec), hipMemcpyDeviceToHost));
    if ((st = repair_map_tie(r, sr, &z_changed)) != TRG_OK) return st;
  }
  e->stats.map_tie_unread -= lv.mt_skipped.size();  // (read after all)
  lv.repairs += " skipped_map_ties(" + std::to_string(lv.mt_skipped.size()) + (z_changed ? ", z_changed)" : ")");
  lv.mt_skipped.clear();
  return TRG_OK;
}

// Only ties among nodes that existed before the level: nothing else of the level is in doubt.  The
// reference's winner (kd-tree visiting order, host_index.h) replaces the device's pick in the slot records
// and resolve + commit run again -- no host replay of the whole level.
TrgStatus Build::fix_pre_level_ties(Level &lv) {
  TrgStatus st;
  std::vector<SlotRec> srec(lv.slots);
  HIPCHK(e, hipMemcpy(srec.data(), B.slot_rec, lv.slots * sizeof(SlotRec), hipMemcpyDeviceToHost));
  Nearest near;
  std::vector<size_t> patched;  // slots whose records changed: bb.st_slot holds them, in this order
  bb.st_slot.clear();
  for (size_t sl = 0; sl < lv.slots; ++sl) {
    SlotRec &sr = srec[sl];
    if (!(sr.cls & SLOT_TIE) || (sr.cls & SLOT_CLS_MASK) == 0 || sr.nn0 < 0) continue;
    if ((st = mirror_nodes(e, bb, lv.V0)) != TRG_OK) return st;
    near.start(bb, sr, lv.V0);
    e->stats.nn_ties++;
    sr.nn0 = near.winner(bb, lv.V0, sr.x, sr.y);
    sr.cls &= ~SLOT_TIE;
    bb.st_slot.push_back(sr);
    patched.push_back(sl);
  }
  for (size_t k = 0; k < patched.size(); ++k)
    HIPCHK(e, hipMemcpyAsync(B.slot_rec + patched[k], bb.st_slot.data() + k, sizeof(SlotRec), hipMemcpyHostToDevice,
                             repair_stream(e)));
  if (!patched.empty()) HIPCHK(e, hipStreamSynchronize(repair_stream(e)));
  lv.repairs += " fix_pre_level_ties(" + std::to_string(patched.size()) + ")";
  lv.err_from_sample = 0;  // settled
  if ((st = redo_commit(lv)) != TRG_OK) return st;
  e->stats.bfs_tie_fixups++;
  return TRG_OK;
}

// A tie between two nearest-node candidates touches only the slots that met it: whichever of the tied
// nodes wins, the distance -- hence "creates a node or not" -- is the same unless their states differ, and
// nobody waits for a sample that does not create.  The committed level stands; the host decides the
// listed slots as the reference would and rewrites their call records.  (States differ and one outcome
// creates: the tie stays in lv.err and the level is replayed.)
TrgStatus Build::settle_ties_in_place(Level &lv) {
  TrgStatus st;
  int ntie = 0;
  HIPCHK(e, hipMemcpy(&ntie, B.ctrs + BFS_CTR_NTIE, sizeof(int), hipMemcpyDeviceToHost));
  if (ntie <= 0 || ntie > BFS_TIE_CAP) return TRG_OK;
  std::vector<int> tslots(ntie);
  HIPCHK(e, hipMemcpy(tslots.data(), B.tie_list, (size_t)ntie * sizeof(int), hipMemcpyDeviceToHost));
  std::sort(tslots.begin(), tslots.end());
  tslots.erase(std::unique(tslots.begin(), tslots.end()), tslots.end());
  if (tslots.front() < 0 || (size_t)tslots.back() >= lv.slots) return TRG_OK;
  // which slots created a node (outcomes 3 / 4): the nodes that existed at a slot's turn are
  // V0 + the creations of the slots before it
  std::vector<int> oc((size_t)tslots.back() + 1);
  HIPCHK(e, hipMemcpy(oc.data(), B.c_outcome, oc.size() * sizeof(int), hipMemcpyDeviceToHost));
  const auto t_mirror = Clock::now();
  const size_t mirrored = bb.hm_state.size();
  if ((st = mirror_nodes(e, bb, lv.v_after)) != TRG_OK) return st;  // (the level's nodes included)
  const double ms_mirror = ms_since(t_mirror);
  struct Patch {
    size_t at;
    int n2, st;
  };
  std::vector<Patch> patches;
  // the tied slots' records and parents: one batch of copies, one wait.  st_int: a parent per slot, then room
  // for the two patch words of each.
  const size_t nt = tslots.size();
  const hipStream_t sr_ = repair_stream(e);
  bb.st_slot.resize(nt);
  bb.st_int.resize(3 * nt);
  for (size_t k = 0; k < nt; ++k) {
    HIPCHK(e, hipMemcpyAsync(bb.st_slot.data() + k, B.slot_rec + tslots[k], sizeof(SlotRec), hipMemcpyDeviceToHost,
                             sr_));
    HIPCHK(e, hipMemcpyAsync(bb.st_int.data() + k, B.front_cur + tslots[k] / S, sizeof(int), hipMemcpyDeviceToHost,
                             sr_));
  }
  HIPCHK(e, hipStreamSynchronize(sr_));
  Nearest near;
  size_t scanned = 0;
  int created_before = 0;
  for (size_t k = 0; k < nt; ++k) {
    const int sl = tslots[k];
    for (; scanned < (size_t)sl; ++scanned) created_before += (oc[scanned] == 3 || oc[scanned] == 4);
    const int V_at = lv.V0 + created_before;
    const SlotRec &sr = bb.st_slot[k];
    const int u = bb.st_int[k];
    if ((sr.cls & SLOT_CLS_MASK) == 0) continue;
    near.start(bb, sr, lv.V0);
    for (int i = lv.V0; i < V_at; ++i) near.offer(bb, i, sr.x, sr.y);
    if (near.nn < 0) return TRG_OK;
    if (near.tie()) e->stats.nn_ties++;
    const int nn = near.winner(bb, V_at, sr.x, sr.y);
    const int kind =
        bb.hm_state[nn] == TRG_NODE_INVALID ? 1 : (std::sqrt(near.best) < e->prm.robot_size ? 2 : 3);
    const bool dev_creates = oc[sl] == 3 || oc[sl] == 4;
    if ((kind == 3) != dev_creates) return TRG_OK;  // the level's node set is in doubt: replay it
    if (kind == 3) continue;                          // creates either way: its record stands
    patches.push_back({(size_t)lv.call_base + (size_t)sl, kind == 2 ? nn : -1,
                       (kind == 2 && nn != u) ? CALL_PENDING : CALL_NONE});
  }
  for (size_t k = 0; k < patches.size(); ++k) {  // (at most one per tied slot)
    int *words = bb.st_int.data() + nt + 2 * k;
    words[0] = patches[k].n2;
    words[1] = patches[k].st;
    HIPCHK(e, hipMemcpyAsync(B.call_n2 + patches[k].at, words, sizeof(int), hipMemcpyHostToDevice, sr_));
    HIPCHK(e, hipMemcpyAsync(B.call_status + patches[k].at, words + 1, sizeof(int), hipMemcpyHostToDevice, sr_));
  }
  if (!patches.empty()) HIPCHK(e, hipStreamSynchronize(sr_));
  {
    char txt[160];
    snprintf(txt, sizeof txt, " settle_ties_in_place(%zu slots, %zu patched, %zu nodes mirrored in %.3f ms)", nt,
             patches.size(), bb.hm_state.size() - mirrored, ms_mirror);
    lv.repairs += txt;
  }
  launch_bfs_clear_tie(B, s);
  lv.err &= ~BFS_ERR_TIE;
  e->stats.bfs_tie_fixups++;
  return TRG_OK;
}

// One BFS level replayed sequentially on the host (exactly the reference's loop, trg.cpp:406-452),
// consuming what the device already computed for the level: the samples, every sample's nearest
// PRE-LEVEL node (k_level_sample; a slot whose nearest pre-level node was not unique carries
// SLOT_TIE) and the speculative parent edges.  Used when the device met an exact fp32 distance tie
// between two nearest-node candidates -- the reference's answer then depends on its kd-tree's
// traversal order, which kd_tie_winner() (host_index.h) reproduces without building the tree -- or
// when a resolve wait ran out.  The nodes this level creates are indexed in a small cell map and
// appended to the host mirror.  Afterwards the device BFS continues.
TrgStatus Build::replay_level(Level &lv) {
  const int V0 = lv.V0;
  const size_t slots = lv.slots;
  TrgStatus st;
  // states and positions of the nodes that exist before this level (kept across replays)
  if ((st = mirror_nodes(e, bb, V0)) != TRG_OK) return st;  // (the undo before the replay cut it back to V0)
  // level inputs: the records k_level_sample / k_level_spec left (candidates are indexed by slot)
  std::vector<int> front(lv.mcur);
  std::vector<NodeRec> nrec(lv.mcur);
  std::vector<SlotRec> srec(slots);
  HIPCHK(e, hipMemcpy(front.data(), B.front_cur, (size_t)lv.mcur * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(nrec.data(), B.node_rec, (size_t)lv.mcur * sizeof(NodeRec), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(srec.data(), B.slot_rec, slots * sizeof(SlotRec), hipMemcpyDeviceToHost));
  std::vector<NodeCov> new_cov;  // of the nodes created here, in creation order
  std::vector<float> new_z;
  std::vector<int> new_hits;
  // the nodes this level has created so far, by cell of the node grid (cell = robot_size): flat
  // head / next chains; a cell's head is valid only if its stamp is this replay's serial number, so
  // the arrays are never cleared
  const size_t ncell = (size_t)B.GW * B.GH;
  if (bb.rp_stamp.size() != ncell) {
    bb.rp_stamp.assign(ncell, 0);
    bb.rp_head.assign(ncell, -1);
    bb.rp_serial = 0;
  }
  const int serial = ++bb.rp_serial;
  std::vector<int> rp_next;  // chain link of node V0 + k
  auto cell_xy = [&](float v, float v0, int n) {
    float t = std::floor((v - v0) * B.ginv);
    t = std::min(std::max(t, 0.0f), (float)(n - 1));
    return (int)t;
  };
  // sequential replay
  std::vector<int> call_n1(slots), call_n2(slots, -1), call_st(slots, CALL_NONE), next_front;
  std::vector<float> call_w(slots, 0.0f), call_d(slots, 0.0f);
  Nearest near;
  int Vcur = V0;
  unsigned long long invalid = 0;
  for (int qpos = 0; qpos < lv.mcur; ++qpos) {
    const int u = front[qpos];
    for (int j = 0; j < S; ++j) {
      const size_t slot = (size_t)qpos * S + j;
      call_n1[slot] = u;
      if (j >= nrec[qpos].n_acc) continue;
      const SlotRec &sr = srec[slot];
      const float qx = sr.x, qy = sr.y;
      // nearest node: the pre-level one(s) the device found, against the nodes created earlier in this level
      near.start(bb, sr, V0);
      {
        const float rad = (near.nn >= 0 ? std::sqrt(near.best) : e->prm.expand_dist * 1.01f) * 1.001f + 1e-6f;
        const int cx0 = cell_xy(qx - rad, B.gx0, B.GW), cx1 = cell_xy(qx + rad, B.gx0, B.GW);
        const int cy0 = cell_xy(qy - rad, B.gy0, B.GH), cy1 = cell_xy(qy + rad, B.gy0, B.GH);
        for (int cy = cy0; cy <= cy1; ++cy)
          for (int cx = cx0; cx <= cx1; ++cx) {
            const size_t cell = (size_t)cy * B.GW + cx;
            if (bb.rp_stamp[cell] != serial) continue;
            for (int id = bb.rp_head[cell]; id >= 0; id = rp_next[id - V0]) near.offer(bb, id, qx, qy);
          }
      }
      if (near.nn < 0) return e->fail(TRG_ERR_DEVICE, "host level replay: a sample without a nearest node");
      if (near.tie()) e->stats.nn_ties++;
      const int nn = near.winner(bb, Vcur, qx, qy);
      if (bb.hm_state[nn] == TRG_NODE_INVALID) continue;                         // trg.cpp:411-413
      // (existing - sample).norm() < robot_size: the distance is `best` whichever node it is
      if (std::sqrt(near.best) < e->prm.robot_size) {                                              // trg.cpp:414-417
        if (nn != u) {
          call_n2[slot] = nn;
          call_st[slot] = CALL_PENDING;
        }
        continue;
      }
      if ((sr.cls & SLOT_CLS_MASK) != 2)
        return e->fail(TRG_ERR_DEVICE, "host level replay: missing speculative edge");
      const bool ok = (sr.status & EDGE_STATUS_MASK) == EDGE_OK;
      const int id = Vcur++;
      new_hits.push_back(sr.hits);  // map points of the parent edge the reference evaluates (trg.cpp:425)
      bb.hm_x.push_back(qx);
      bb.hm_y.push_back(qy);
      bb.hm_state.push_back(ok ? TRG_NODE_VALID : TRG_NODE_INVALID);
      new_z.push_back(sr.z);
      {
        const size_t cell = (size_t)cell_xy(qy, B.gy0, B.GH) * B.GW + cell_xy(qx, B.gx0, B.GW);
        rp_next.push_back(bb.rp_stamp[cell] == serial ? bb.rp_head[cell] : -1);
        bb.rp_stamp[cell] = serial;
        bb.rp_head[cell] = id;
      }
      NodeCov nc{};
      if (ok) {
        call_n2[slot] = id;
        call_st[slot] = sr.status & EDGE_STATUS_MASK;  // the weight follows after the loop (k_node_weights)
        call_d[slot] = sr.dist;
        next_front.push_back(id);
        // the covariance follows on the device (k_node_cov, after the loop) unless the host re-evaluated the
        // edge and left its weight
        if (sr.w_given) nc.cov[0] = sr.cov[0];
        nc.w_given = sr.w_given;
        nc.call = (int)(lv.call_base + (long long)slot);
      } else {
        invalid++;
      }
      new_cov.push_back(nc);
    }
  }
  const int created = Vcur - V0;
  bb.nodes_created += (unsigned long long)created;
  bb.nodes_invalid += invalid;
  // (draws / samples / candidates / hit counts: per-node records, summed after the loop)
  if (Vcur > B.vcap || (int)next_front.size() > B.fcap)
    return e->fail(TRG_ERR_CAPACITY, "host level replay: capacity");
  // hand the level's results to the device
  if (created > 0) {
    const size_t at = (size_t)V0, n = (size_t)created;
    HIPCHK(e, hipMemcpy(B.nx + at, bb.hm_x.data() + at, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(B.ny + at, bb.hm_y.data() + at, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(B.nz + at, new_z.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(B.nstate + at, bb.hm_state.data() + at, n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(B.ncov + at, new_cov.data(), n * sizeof(NodeCov), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(B.nhits + at, new_hits.data(), n * sizeof(int), hipMemcpyHostToDevice));
    // (their disc counts stay unknown: the void device commit numbered other samples with these ids)
    if (B.ndisc) {
      const std::vector<int> unknown(n, -1);
      HIPCHK(e, hipMemcpy(B.ndisc + at, unknown.data(), n * sizeof(int), hipMemcpyHostToDevice));
    }
    launch_bfs_insert_nodes(B, V0, created, s);
  }
  if (!next_front.empty()) {
    HIPCHK(e, hipMemcpy(B.front_next, next_front.data(), next_front.size() * sizeof(int),
                        hipMemcpyHostToDevice));
    std::vector<float> fxy(2 * next_front.size());
    for (size_t k = 0; k < next_front.size(); ++k) {
      fxy[2 * k] = bb.hm_x[next_front[k]];
      fxy[2 * k + 1] = bb.hm_y[next_front[k]];
    }
    HIPCHK(e, hipMemcpy(B.fxy_next, fxy.data(), fxy.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  const size_t cb = (size_t)lv.call_base;
  HIPCHK(e, hipMemcpy(B.call_n1 + cb, call_n1.data(), slots * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(B.call_n2 + cb, call_n2.data(), slots * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(B.call_status + cb, call_st.data(), slots * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(B.call_w + cb, call_w.data(), slots * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(B.call_dist + cb, call_d.data(), slots * sizeof(float), hipMemcpyHostToDevice));
  int ctr_host[BFS_CTR_COUNT] = {0};
  ctr_host[BFS_CTR_V] = Vcur;
  ctr_host[BFS_CTR_MNEXT] = (int)next_front.size();
  HIPCHK(e, hipMemcpy(B.ctrs, ctr_host, BFS_CTR_NUNC2 * sizeof(int), hipMemcpyHostToDevice));  // (the deferred pipeline owns NUNC2)
  HIPCHK(e, hipStreamSynchronize(s));
  lv.v_after = Vcur;
  lv.mnext = (int)next_front.size();
  lv.replayed = true;
  e->stats.bfs_host_levels++;
  return TRG_OK;
}

// The rare events of a level, repaired in this order.  The device treats a slope gate it could not call
// as "not gated" and a nearest-node tie as "lowest id"; when either happened the level's commit is taken
// back, the host supplies the exact answer, and resolve + commit run again / the level is replayed on the
// host.
//
// Invariant of the map-point ties (step 4): no rerun of resolve + commit and no host replay of a level ever runs
// with an unrepaired candidate (class-2) tie record of that level.  fix_map_ties may leave such records alone
// (Level::mt_skipped) only while the commit it looked at stands; redo_commit, the undo_level calls of steps 5
// and 8, fix_pre_level_ties (through redo_commit) and replay_level (always behind an undo) all pass through
// undo_level, which repairs them first.  Step 2 runs before any record is skipped, and the filter of step 4
// reads the outcomes of the commit step 2 left.  Step 7 keeps the commit and changes no creator.
TrgStatus Build::repair_level(Level &lv) {
  TrgStatus st;
  // 1. step-3 guards
  if (e->step3 && lv.n_unc > 0)
    // (the rescue search of k_level_spec3 ran on the provisional verdict of that gate)
    return fallback("a slope gate left to the host's libm in a build with expandGraph's step 3");
  if (CS > 1 && ((lv.err & BFS_ERR_SOFT & ~BFS_ERR_STALL) || lv.n_mt > 0))
    // (the host repairs of nearest-node ties and map-point ties are written for the dense call log and
    // know nothing of step 3: such a build goes to the host replay as a whole)
    return fallback("exact fp32 distance tie in a build with expandGraph's step 3");
  const auto t_rare = Clock::now();
  const bool any_rare = lv.n_mt > 0 || lv.n_unc > 0 || (lv.err & (BFS_ERR_SOFT | BFS_ERR_LOOKBACK));
  // 2. ticketed repeat: a bounded wait of the resolve launch ran out, the hardware did not start its
  // workgroups in index order (another process's kernels on the card).  The launch is repeated with start
  // tickets as logical indices: every wait is then for a workgroup that is already running, whatever the
  // dispatch order.  (Test hook debug_wait_rerun: the repeat fails as well.)
  constexpr int ERR_WAIT = BFS_ERR_STALL | BFS_ERR_LOOKBACK;
  if ((lv.err & ERR_WAIT) && !(lv.err & ~(BFS_ERR_SOFT | ERR_WAIT))) {
    const int hook = e->debug_wait_rerun ? ((lv.err & BFS_ERR_LOOKBACK) ? 2 : 1) : 0;
    e->stats.bfs_ticket_reruns++;
    st = redo_commit(lv, false, true, hook);
    if (st == TRG_ERR_CAPACITY) e->stats.ms_rare_events += ms_since(t_rare);  // (a hard error, as below)
    if (st != TRG_OK) return st;
  }
  // 3. hard errors
  if (lv.err & ~BFS_ERR_SOFT) {
    if (any_rare) e->stats.ms_rare_events += ms_since(t_rare);
    return fallback(err_text(lv.err));
  }
  // 4. map-point ties (the level's gates are decided before their rerun)
  if (lv.n_mt > 0 && (st = fix_map_ties(lv)) != TRG_OK) return st;
  // 5. uncertain gates: a speculative edge the level relied on that is in fact gated redoes the second half
  if (lv.n_unc > 0) {
    void *status = (char *)B.slot_rec + offsetof(SlotRec, status);
    if ((st = resolve_uncertain(lv.n_unc, status, sizeof(SlotRec), lv.parity, lv.unc_ctr, true)) != TRG_OK) return st;
    if (unc_changed && (st = (lv.err & BFS_ERR_SOFT) ? undo_level(lv) : redo_commit(lv)) != TRG_OK) return st;
  }
  // 6. ties among pre-level nodes only
  if ((lv.err & BFS_ERR_SOFT) == BFS_ERR_TIE_CLS && !lv.undone && (st = fix_pre_level_ties(lv)) != TRG_OK)
    return st;
  // 7. ties with the level's own nodes, settled on the committed level
  if ((lv.err & BFS_ERR_SOFT) == BFS_ERR_TIE && !lv.undone && e->tie_inplace && !debug_tie_level(e, lv.index)) {
    if ((st = settle_ties_in_place(lv)) != TRG_OK) return st;
  }
  // 8. exact fp32 distance tie (or a resolve whose bounded wait ran out): this one level is replayed on the
  // host, then the device goes on
  if (lv.err & BFS_ERR_SOFT) {
    if (CS > 1) return fallback("a level of a build with expandGraph's step 3 needs the host replay");
    if (!lv.undone && (st = undo_level(lv)) != TRG_OK) return st;
    if ((st = replay_level(lv)) != TRG_OK) return st;
  }
  if (any_rare) {
    e->stats.ms_rare_events += ms_since(t_rare);
    if (getenv("TRG_TRACE_LEVELS"))
      fprintf(stderr,
              "[trg bfs] level %d: rare events (map ties %d, uncertain gates %d, err %d%s) took %.3f ms; ran:%s%s, "
              "commit %s\n",
              lv.index, lv.n_mt, lv.n_unc, lv.err, lv.replayed ? ", host replay" : "", ms_since(t_rare),
              lv.repairs.empty() ? " -" : lv.repairs.c_str(), lv.replayed ? " replay_level" : "",
              lv.reexpand ? "redone" : "kept");
  }
  return TRG_OK;
}

// ---- phase 1: geometry of the node grid, capacities, device buffers -----------------------------------
TrgStatus Build::allocate() {
  const float pad = e->prm.expand_dist * 2 + e->prm.robot_size;
  float cell = e->prm.robot_size;
  if (!(cell > 0)) return fallback("robot_size <= 0");
  const double ex = (double)(m.bounds[2] - m.bounds[0]) + 2 * pad + 4 * cell;
  const double ey = (double)(m.bounds[3] - m.bounds[1]) + 2 * pad + 4 * cell;
  if ((ex / cell + 2) * (ey / cell + 2) > 256e6) return fallback("node grid too large");
  B.gx0 = m.bounds[0] - pad - 2 * cell;
  B.gy0 = m.bounds[1] - pad - 2 * cell;
  B.gcell_size = cell;
  B.ginv = 1.0f / cell;
  B.GW = (int)floor(ex / cell) + 2;
  B.GH = (int)floor(ey / cell) + 2;
  const size_t ncell = (size_t)B.GW * B.GH;
  // nodes are pairwise >= robot_size apart: hexagonal packing bounds their number
  const double vbound = ex * ey / (0.8660254 * cell * cell) * 1.05 + 4096;
  if (vbound > 400e6) return fallback("node capacity bound too large");
  const size_t vcap = (size_t)vbound;
  const size_t fcap = BFS_FCAP;
  const size_t slots = fcap * (size_t)std::max(S, 1);

  if (!level_kernels_support(qp, cell))
    return fallback("sample_num or expand_dist / robot_size outside the level kernels' range");
  TrgStatus st;
  const size_t wg_words = slots / 16 + 64 + 8;  // (>= one word per resolve workgroup, then the start tickets)
  const size_t I = sizeof(int), FL = sizeof(float);
  if ((st = ensure_all(e, {{&bb.nx, vcap * FL}, {&bb.ny, vcap * FL}, {&bb.nz, vcap * FL}, {&bb.nstate, vcap * I},
                           {&bb.gcell, ncell * sizeof(GridCell)}, {&bb.ncov, vcap * sizeof(NodeCov)},
                           {&bb.front0, fcap * I}, {&bb.front1, fcap * I}, {&bb.fxy0, fcap * sizeof(float2)},
                           {&bb.fxy1, fcap * sizeof(float2)}})) != TRG_OK)
    return st;
  B.nx = (float *)bb.nx.p;
  B.ny = (float *)bb.ny.p;
  B.nz = (float *)bb.nz.p;
  B.nstate = (int *)bb.nstate.p;
  // per node: the map points inside its acceptance disc, the first disc of every walk that starts at it
  // (edge_gather's n0).  -1 = unknown wherever the level loop's commit has not written: the root, and the nodes of
  // a level the host replayed (replay_level sets them again, a void device commit may have written there)
  B.ndisc = nullptr;
  if (e->known_start_disc) {
    if ((st = ensure_bytes(e, bb.ndisc, vcap * I)) != TRG_OK) return st;
    B.ndisc = (int *)bb.ndisc.p;
    HIPCHK(e, hipMemsetAsync(B.ndisc, 0xFF, vcap * I, s));
  }
  B.vcap = (int)std::min<size_t>(vcap, 0x7FFFFFF0);
  B.gcell = (GridCell *)bb.gcell.p;
  B.ncov = (NodeCov *)bb.ncov.p;
  B.front_cur = (int *)bb.front0.p;
  B.front_next = (int *)bb.front1.p;
  B.fxy_cur = (float2 *)bb.fxy0.p;
  B.fxy_next = (float2 *)bb.fxy1.p;
  B.fcap = (int)fcap;
  const size_t ht_need = hash_size(fcap, std::max(S, 1));
  for (LevelSet &l : bb.lv) {
    if ((st = ensure_all(e, {{&l.node_rec, fcap * sizeof(NodeRec)}, {&l.slot_rec, slots * sizeof(SlotRec)},
                             {&l.c_outcome, slots * I}, {&l.lv_hash, ht_need * sizeof(HashEnt)}})) != TRG_OK)
      return st;
    l.use_resc = e->step3;
    if (e->step3 && (st = ensure_bytes(e, l.resc, slots * sizeof(RescueRec))) != TRG_OK) return st;
    // tags start at 1 in every build: entries of earlier builds must not look current
    HIPCHK(e, hipMemsetAsync(l.lv_hash.p, 0, ht_need * sizeof(HashEnt), s));
  }
  // unc_list: even levels, odd levels, deferred evaluations; tied slots
  if ((st = ensure_all(e, {{&bb.mid, edge_mid_floats(CALL_EVAL_BATCH) * FL},
                           {&bb.unc_list, (3 * BFS_UNC_CAP + BFS_TIE_CAP) * I},
                           {&bb.unc_rec, 3 * 3 * BFS_UNC_CAP * FL}, {&bb.mt_rec, 2 * slots * sizeof(MapTieRec)},
                           {&bb.ctrs, BFS_CTR_COUNT * I}, {&bb.stats64, S64_WORDS * sizeof(unsigned long long)},
                           {&bb.wg_state, wg_words * sizeof(unsigned long long)},
                           {&bb.c_cell, slots * sizeof(unsigned long long)}, {&bb.nexp, vcap * sizeof(int4)},
                           {&bb.nhits, vcap * I}, {&bb.scan_tmp, (std::max(slots, vcap) / 2048 + 8) * I}})) != TRG_OK)
    return st;
  B.mid = (float *)bb.mid.p;
  B.unc_list = (int *)bb.unc_list.p;
  B.tie_list = B.unc_list + 3 * BFS_UNC_CAP;
  B.unc_rec = (float *)bb.unc_rec.p;
  B.mt_rec = (MapTieRec *)bb.mt_rec.p;
  B.mt_cap = (int)slots;  // (a record per slot of a level, for either parity: k_level_sample drops none)
  B.ctrs = (int *)bb.ctrs.p;
  B.stats64 = (unsigned long long *)bb.stats64.p;
  B.wg_state = (unsigned long long *)bb.wg_state.p;
  HIPCHK(e, hipMemsetAsync(B.wg_state, 0, wg_words * sizeof(unsigned long long), s));  // epochs start at 1
  B.ticket = (unsigned *)(B.wg_state + (slots / 16 + 64));  // start tickets of the resolve workgroups: zero, like
  ticket_base = 0;                                          // the host's count of the tickets drawn so far
  B.tl = nullptr;
  if (getenv("TRG_TIMELINE")) {
    const size_t tl_bytes = (size_t)(1 << 16) * 12 * 6 * sizeof(unsigned long long);
    if ((st = ensure_bytes(e, bb.tl, tl_bytes)) != TRG_OK) return st;
    B.tl = (unsigned long long *)bb.tl.p;
    HIPCHK(e, hipMemsetAsync(B.tl, 0, tl_bytes, s));
  }
  B.c_cell = (unsigned long long *)bb.c_cell.p;
  HIPCHK(e, hipMemsetAsync(B.c_cell, 0, slots * sizeof(unsigned long long), s));  // (launch epochs start at 1 in every build)
  B.nexp = (int4 *)bb.nexp.p;
  B.nhits = (int *)bb.nhits.p;
  if (!bb.h_ctrs) {
    HIPCHK(e, bb.h_ctrs.ensure(H_CTRS_WORDS, hipHostMallocMapped | hipHostMallocCoherent));
    memset(bb.h_ctrs, 0, H_CTRS_WORDS * sizeof(int));
  }
  {
    void *dp = nullptr;
    HIPCHK(e, hipHostGetDevicePointer(&dp, bb.h_ctrs, 0));
    B.host_ctrs = (int *)dp;
  }

  bb.hm_state.clear();
  bb.hm_x.clear();
  bb.hm_y.clear();
  bb.nodes_created = bb.nodes_invalid = 0;
  HIPCHK(e, hipMemsetAsync(B.gcell, 0, ncell * sizeof(GridCell), s));
  HIPCHK(e, hipMemsetAsync(B.ctrs, 0, BFS_CTR_COUNT * sizeof(int), s));
  HIPCHK(e, hipMemsetAsync(B.stats64, 0, S64_WORDS * sizeof(unsigned long long), s));

  // Deferred wireEdge evaluations (node -> existing node), pipelined behind the level loop.  wireEdge
  // returns at once when a pair is already wired (trg.cpp:255-267), so per unordered pair only its FIRST
  // call is evaluated, then (after the loop) the remaining calls of the few pairs whose first call did not
  // succeed.  "First call of its pair" is final as soon as the call's level is: the calls of finished levels
  // are therefore handed over in batches to a second, low priority stream, where they fill the issue slots
  // the latency-bound level kernels leave idle.  The pair table is sized from the node capacity bound
  // (every node is expanded at most once).
  calls_bound = std::min<size_t>(vcap * (size_t)std::max(S, 1) * (size_t)CS, 0x7FFFFFF0u);
  fht = 1024;
  while ((unsigned long long)fht < (unsigned long long)calls_bound && fht < (1u << 31)) fht <<= 1;
  if ((st = ensure_all(e, {{&bb.ht_key, fht * sizeof(unsigned long long)}, {&bb.ht_seq, fht * I},
                           {&bb.ok_seq, fht * I}, {&bb.def_counts, 2 * I}})) != TRG_OK)
    return st;
  F.ht_key = (unsigned long long *)bb.ht_key.p;
  F.ht_seq = (int *)bb.ht_seq.p;
  F.ok_seq = (int *)bb.ok_seq.p;
  F.ht_size = fht;
  // With step 3 the neighbour calls of a node sit BEFORE later calls in the log but are only known after the
  // loop (trg_step3.inc): "first call of its pair" is not final level by level, so nothing is evaluated beside
  // the loop.
  overlap = !e->step3 && e->defer_overlap;
  s_def = overlap ? e->s_edge : s;
  if (overlap) {  // (otherwise the table is cleared after the loop, right before its first use)
    // (In the main stream.  Measured and dropped: these two clears on the deferred stream, in front of its first
    // batch -- the level loop of a C3 build 0.05-0.15 ms SLOWER in four of four series, profiles/r27_tail_early_copy_ab.txt)
    HIPCHK(e, hipMemsetAsync(F.ht_key, 0xFF, (size_t)fht * sizeof(unsigned long long), s));
    HIPCHK(e, hipMemsetAsync(F.ht_seq, 0x7F, (size_t)fht * sizeof(int), s));
  }
  // (first used after the loop; early_copy: k_fin_insert_listed sets the few entries that are read)
  if (!early_copy) HIPCHK(e, hipMemsetAsync(F.ok_seq, 0x7F, (size_t)fht * sizeof(int), s));
  return TRG_OK;
}

// ---- phase 2: the root node ------------------------------------------------------------------------
TrgStatus Build::seed_root(float root_x, float root_y, float root_z) {
  const int one = 1, zero = 0, valid = TRG_NODE_VALID;
  HIPCHK(e, hipMemcpyAsync(B.nx, &root_x, 4, hipMemcpyHostToDevice, s));
  HIPCHK(e, hipMemcpyAsync(B.ny, &root_y, 4, hipMemcpyHostToDevice, s));
  HIPCHK(e, hipMemcpyAsync(B.nz, &root_z, 4, hipMemcpyHostToDevice, s));
  HIPCHK(e, hipMemcpyAsync(B.nstate, &valid, 4, hipMemcpyHostToDevice, s));
  HIPCHK(e, hipMemcpyAsync(B.ctrs + BFS_CTR_V, &one, 4, hipMemcpyHostToDevice, s));
  HIPCHK(e, hipMemcpyAsync(B.front_cur, &zero, 4, hipMemcpyHostToDevice, s));
  const float root_xy[2] = {root_x, root_y};
  HIPCHK(e, hipMemcpyAsync(B.fxy_cur, root_xy, sizeof(root_xy), hipMemcpyHostToDevice, s));
  HIPCHK(e, hipStreamSynchronize(s));  // the sources above are stack variables
  launch_bfs_insert_nodes(B, 0, 1, s);
  return TRG_OK;
}

// ---- deferred wireEdge evaluations -------------------------------------------------------------------------
// calls [def_lo, c1) of finished levels -> pair table, first-of-pair selection, evaluation: four launches per
// batch.  The batches share one count word (and the edge scratch B.mid): each is ordered behind the one before
// it, by the stream, and the first batch on the main stream by finish_deferred's wait for the deferred stream.
TrgStatus Build::launch_deferred(long long c1, bool in_loop) {
  int *sel_count = (int *)bb.def_counts.p + 1;
  while (def_lo < c1) {
    const long long c_hi = std::min<long long>(c1, def_lo + CALL_EVAL_BATCH);
    const long long n = c_hi - def_lo;
    hipStream_t st_ = in_loop ? s_def : s;
    launch_first_insert(F, B, def_lo, c_hi, sel_count, st_);
    launch_calls_select_append(F, B, def_lo, c_hi, (int *)bb.sel_list.p + def_lo, sel_count,
                               B.stats64 + S64_DEF_KEPT, st_);
    // the evaluations, timed like the level kernels: every 8th batch, scaled up afterwards (an event pair per
    // batch was a fifth of the host's launch work per level)
    Event t0, t1;
    if ((n_eval_batches++ % 8) == 0 && def_events.size() < 8192) {
      HIPCHK(e, t0.create());
      HIPCHK(e, t1.create());
      HIPCHK(e, hipEventRecord(t0.ev, st_));
    }
    // the number of selected calls lives on the device: the grid is an upper bound
    launch_calls_eval(m.view, qp, B, (int *)bb.sel_list.p + def_lo, (int)n, sel_count, e->d_ctr, st_);
    e->stats.launches_edge_kernel++;
    if (t0.ev) {
      HIPCHK(e, hipEventRecord(t1.ev, st_));
      def_events.emplace_back(std::move(t0), std::move(t1));
    }
    def_lo = c_hi;
  }
  return TRG_OK;
}

// the call log grown to `need` calls, its contents kept
TrgStatus Build::grow_call_log(size_t need) {
  const size_t I = sizeof(int);
  const size_t want = std::max(need, std::max<size_t>(bb.call_n1.bytes / I * 2, (size_t)4 << 20));
  // the grow copies run on the NULL stream, which does not wait for the (non-blocking) level and
  // deferred streams: everything that still writes the call log must have finished first
  HIPCHK(e, hipStreamSynchronize(s));
  if (s_def != s) HIPCHK(e, hipStreamSynchronize(s_def));
  TrgStatus st;
  for (DevArr *a : {&bb.call_n1, &bb.call_n2, &bb.call_status, &bb.call_w, &bb.call_dist, &bb.newid_of_call,
                    &bb.call_slot})
    if ((st = ensure_bytes(e, *a, want * I, true)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, bb.sel_list, (want + 1) * I, true)) != TRG_OK) return st;
  B.call_n1 = (int *)bb.call_n1.p;
  B.call_n2 = (int *)bb.call_n2.p;
  B.call_status = (int *)bb.call_status.p;
  B.call_w = (float *)bb.call_w.p;
  B.call_dist = (float *)bb.call_dist.p;
  B.newid_of_call = (int *)bb.newid_of_call.p;
  F.call_slot = (int *)bb.call_slot.p;
  return TRG_OK;
}

// ---- phase 3: the level loop ---------------------------------------------------------------------------
TrgStatus Build::level_loop() {
  TrgStatus st;
  for (Event *ev : {&ev_order, &ev_nodes, &ev_structure, &ev_weights, &ev_node_arrays, &ev_totals})
    HIPCHK(e, ev->create(false));
  bool have_expand = false;  // this level's expansion was issued by the previous iteration
  // The level kernels time every expansion themselves (B.stats64[S64_EXPAND_TICKS], report_stats): no event
  // is recorded in this stream (a pair around a kernel costs ~12 us of stream time).
  uint64_t n_expand_all = 0;
  int mcur = 1;
  int v_now = 1;  // nodes that exist before the current level (the root)
  long long call_base = 0;
  int tag_serial = 0;  // one hash tag per level attempt
  int cur_tag = 0;
  int cur_ht = 0;  // hash size the current level's expand used
  auto t_loop = Clock::now();
  while (mcur > 0) {
    const size_t level_slots = (size_t)mcur * S;
    const size_t need_calls = (size_t)call_base + level_slots * (size_t)CS;
    if (bb.call_n1.bytes < need_calls * sizeof(int) && (st = grow_call_log(need_calls)) != TRG_OK) return st;
    const int parity = levels & 1;
    bb.lv[parity].apply(B);
    if (levels == e->debug_fallback_level) {
      HIPCHK(e, hipStreamSynchronize(s));
      return fallback("declined on request (debug_fallback_level)");
    }
    if (!have_expand) {
      cur_tag = ++tag_serial;
      cur_ht = hash_size((size_t)mcur, S);
      B.ht_size = cur_ht;
      launch_level_expand(m.view, qp, e->d_cos, e->d_sin, e->sampler.table_bits, e->sampler.seed,
                          e->epoch, B, mcur, nullptr, 0, parity, cur_tag, 0, e->d_ctr, s);
    }
    B.ht_size = cur_ht;
    // The rest of the level is launched at once and the host looks at the counters once, at the end.
    Level lv{levels, parity, mcur, v_now, level_slots, call_base, cur_tag,
             parity ? BFS_CTR_NUNC1 : BFS_CTR_NUNC};
    // The next level's record set, hash size and tag: its expansion is launched right behind this
    // level's resolve, before the host has seen this level's counters (the frontier size is read from
    // the device, the grid is an upper bound).
    BfsDev Bn = B;
    std::swap(Bn.front_cur, Bn.front_next);
    std::swap(Bn.fxy_cur, Bn.fxy_next);
    bb.lv[parity ^ 1].apply(Bn);
    const size_t next_cap_nodes =
        std::min<size_t>((size_t)B.fcap, std::max<size_t>(2 * (size_t)mcur, (size_t)mcur + 1024));
    const int next_ht = hash_size(next_cap_nodes, S);
    Bn.ht_size = next_ht;
    int spec_bound = (int)std::min<size_t>(
        (size_t)B.fcap, std::min<size_t>(level_slots, (size_t)(mcur + std::max(128, mcur / 4))));
    if (e->debug_spec_bound > 0) spec_bound = std::min(spec_bound, e->debug_spec_bound);
    int next_tag = ++tag_serial;
    const int stall_hook = levels == e->debug_stall_level ? 1 : (levels == e->debug_lookback_level ? 2 : 0);
    launch_level_resolve_commit(B, qp, mcur, TRG_NODE_VALID, call_base, lv.V0, cur_tag, ++res_epoch, s,
                                stall_hook, e->resolve_tickets != 0, &ticket_base);
    const int stamp = ++bb.stamp_serial;  // published by the next level's expansion, launched right below
    launch_level_expand(m.view, qp, e->d_cos, e->d_sin, e->sampler.table_bits, e->sampler.seed,
                        e->epoch, Bn, spec_bound, B.ctrs + BFS_CTR_MNEXT, 0, parity ^ 1, next_tag, stamp,
                        e->d_ctr, s);
    // The calls of the levels before this one are final: into the deferred pipeline, a batch at a time.  Behind
    // the level's own launches, not in front of them: the main stream holds only the running expansion while the
    // host issues these four or more launches, and on a level of a few hundred nodes that is 25-30 us of work.
    // (The calls of the last levels stay for finish_deferred.)
    if (overlap && call_base - def_lo >= DEF_BATCH_MIN && call_base < 0x7FFFFFF0LL)
      if ((st = launch_deferred(call_base, true)) != TRG_OK) return st;
    if ((st = wait_stamp(stamp)) != TRG_OK) return st;
    n_expand_all++;
    read_level(lv, true);
    if (lv.err && getenv("TRG_TRACE_LEVELS"))
      fprintf(stderr, "[trg bfs] level %d: err=%d (%s) mcur=%d v=%d mnext=%d\n", levels, lv.err,
              err_text(lv.err).c_str(), mcur, lv.v_after, lv.mnext);
    if ((st = repair_level(lv)) != TRG_OK) return st;
    // the level is final: its statistics (a replayed level counted its nodes itself)
    if (!lv.replayed) {
      bb.nodes_created += (unsigned long long)(lv.v_after - lv.V0);
      bb.nodes_invalid += (unsigned long long)(lv.v_after - lv.V0 - lv.mnext);
    }
    // the next level's expansion: redo it after a redone commit or when its hash was sized too
    // small, top it up past the launch bound
    if (lv.reexpand || (size_t)lv.mnext > next_cap_nodes) {
      if (!lv.reexpand) HIPCHK(e, hipStreamSynchronize(s));
      int ctr_fix[3] = {0, 0, 0};
      HIPCHK(e, hipMemcpy(B.ctrs + BFS_CTR_NMAPTIE, ctr_fix, 2 * sizeof(int), hipMemcpyHostToDevice));
      HIPCHK(e, hipMemcpy(B.ctrs + ((parity ^ 1) ? BFS_CTR_NUNC1 : BFS_CTR_NUNC), ctr_fix, sizeof(int),
                          hipMemcpyHostToDevice));
      have_expand = false;  // issued at the top of the next iteration with a fresh tag
    } else {
      if (lv.mnext > spec_bound)
        launch_level_expand(m.view, qp, e->d_cos, e->d_sin, e->sampler.table_bits, e->sampler.seed,
                            e->epoch, Bn, lv.mnext, nullptr, spec_bound, parity ^ 1, next_tag, 0, e->d_ctr, s);
      have_expand = true;
      cur_tag = next_tag;
      cur_ht = next_ht;
    }
    v_now = lv.v_after;
    std::swap(B.front_cur, B.front_next);
    std::swap(B.fxy_cur, B.fxy_next);
    call_base += (long long)level_slots * CS;
    mcur = lv.mnext;
    levels++;
  }
  HIPCHK(e, hipStreamSynchronize(s));
  e->stats.ms_bfs_loop = ms_since(t_loop);
  e->stats.launches_sample_kernel += n_expand_all;  // (their time: report_stats)
  V = v_now;
  ncalls = call_base;
  e->stats.sync_batches += (uint64_t)levels;
  return TRG_OK;
}

// The covariances of the edges that created the nodes (the level loop only decided whether those edges hold) and
// the weights from them (same stream: ordered), all nodes in ONE launch each, after the loop, where every level
// is final.  (Handed over level by level beside the loop, like the call batches, the same work comes as ~370
// small launches that take vector issue from the level kernels: DESIGN.md section 4.)  k_node_weights touches
// only the calls that created a node: their call_w, and call_status outside EDGE_STATUS_MASK.
void Build::launch_creating_edge_weights(hipStream_t st) {
  launch_node_cov(m.view, qp, B, 1, V, st);
  launch_node_weights(B, V, st);
}

// ---- phase 4: the rest of the deferred wireEdge evaluations (round 1), then round 2 ----------------------
TrgStatus Build::finish_deferred() {
  TrgStatus st;
  auto t_def = Clock::now();
  if (ncalls >= 0x7FFFFFF0LL) return fallback("call log too long");
  if ((size_t)ncalls > calls_bound) return fallback("more wireEdge calls than the node capacity bound allows");
  if (!overlap) {
    HIPCHK(e, hipMemsetAsync(F.ht_key, 0xFF, (size_t)fht * sizeof(unsigned long long), s));
    HIPCHK(e, hipMemsetAsync(F.ht_seq, 0x7F, (size_t)fht * sizeof(int), s));
  }
  if (!tail_split) launch_creating_edge_weights(s);  // (tail_split: beside the copies of clean_and_fetch)
  if (e->step3) {
    // step 3 (trg.cpp:429-444): the node tree rebuilt on the device, every valid node's neighbour calls into
    // the entries behind its creating call; the deferred pipeline below takes them like all other calls
    if ((st = ensure_bytes(e, bb.s3_scratch, (6 * (size_t)V + 8) * sizeof(int))) != TRG_OK) return st;
    if (launch_step3_calls(B, V, e->prm.expand_dist, (int *)bb.s3_scratch.p, bb.h_ctrs + H_STEP3_LEFT, s) != 0)
      return e->fail(TRG_ERR_DEVICE, "step-3 call generation failed");
    HIPCHK(e, hipGetLastError());
  }
  if (overlap) {  // what ran beside the loop must be complete before the main stream goes on with it
    HIPCHK(e, hipEventRecord(ev_order.ev, e->s_edge));
    HIPCHK(e, hipStreamWaitEvent(s, ev_order.ev, 0));
  }
  if ((st = launch_deferred(ncalls, false)) != TRG_OK) return st;  // round 1 of the calls not yet handed over
  // while the GPU evaluates: the reference's graph.nodes[node_id] = node for ids 0..V-1 in creation
  // order (trg.cpp:248); cleanGraph iterates this container below
  const auto t_order = Clock::now();
  e->nodes_sim.clear();  // resetGraph("global") -> nodes.clear(): buckets and policy persist
  e->nodes_sim.fill((size_t)V);
  e->next_cid = V;  // (cleanGraph drops some of them; the nodes of later updates count on from all that were created)
  // ... whose order goes to the device on the (idle) second stream, for the renumbering kernels of cleanGraph.
  // A plain build sends the container's runs (a few dozen words, as a kernel argument) and a kernel expands
  // them: no vector of V ids is written and uploaded while the GPU has only the last batches left.
  if ((st = ensure_bytes(e, bb.map_order, ((size_t)V + 1) * sizeof(int))) != TRG_OK) return st;
  MapOrderRuns runs;
  std::vector<int> map_order;  // (host expansion only)
  const int run_cap = e->debug_order_run_cap > 0 ? std::min(e->debug_order_run_cap, MAP_ORDER_MAX_RUNS)
                                                 : MAP_ORDER_MAX_RUNS;
  if (tail_split && e->nodes_sim.runs_into(runs, run_cap)) {
    launch_map_order_fill(runs, V, (int *)bb.map_order.p, e->s_edge);
  } else if (V > 0) {  // (more runs than the argument holds, or a build that keeps the earlier order of its tail)
    e->nodes_sim.iteration_order(map_order);
    HIPCHK(e, hipMemcpyAsync(bb.map_order.p, map_order.data(), (size_t)V * sizeof(int), hipMemcpyHostToDevice,
                             e->s_edge));
  }
  // ... and behind it the sums of the expansion's statistics (their inputs are final since the loop ended): a
  // small kernel beside the evaluations instead of one at the very end of the build
  launch_bfs_stats(B, V, B.stats64 + S64_DRAWS, e->s_edge);  // draws, samples, disc hits, speculative-edge hits, candidates, parent-edge hits
  HIPCHK(e, hipEventRecord(ev_order.ev, e->s_edge));
  const double ms_order_host = ms_since(t_order);
  HIPCHK(e, hipStreamSynchronize(s_def));
  if (s_def != s) HIPCHK(e, hipStreamSynchronize(s));  // (the evaluations after the loop run in the main stream)
  if (getenv("TRG_TIMING"))  // who ends this phase last: the host's part against its wait for the last batches
    fprintf(stderr, "[trg deferred]   (host) container order  %8.3f ms, then waited %8.3f ms for the GPU\n",
            ms_order_host, ms_since(t_order) - ms_order_host);
  double ms_edges = 0;
  for (auto &ev : def_events) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev.first.ev, ev.second.ev) == hipSuccess) ms_edges += ms;
  }
  if (!def_events.empty()) ms_edges *= (double)n_eval_batches / (double)def_events.size();
  def_events.clear();
  // round 2: every remaining call of the (few) pairs whose first call failed or was left to the host
  int *d_n2 = (int *)bb.def_counts.p;
  int *h_n2 = bb.h_ctrs + H_ROUND2_CALLS;
  HIPCHK(e, hipMemsetAsync(d_n2, 0, sizeof(int), s));
  launch_calls_select2_append(F, B, ncalls, (int *)bb.sel_list.p, d_n2, B.stats64 + S64_DEF_KEPT, s);
  HIPCHK(e, hipMemcpyAsync(h_n2, d_n2, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  const int nsel = *h_n2;
  nsel2 = nsel;
  // (a batch of evaluations shares the edge scratch: at most CALL_EVAL_BATCH at a time)
  Event t0, t1;
  for (long long q0 = 0; q0 < nsel; q0 += CALL_EVAL_BATCH) {
    const int nq = (int)std::min<long long>(CALL_EVAL_BATCH, nsel - q0);
    HIPCHK(e, t0.create());
    HIPCHK(e, t1.create());
    HIPCHK(e, hipEventRecord(t0.ev, s));
    launch_calls_eval(m.view, qp, B, (int *)bb.sel_list.p + q0, nq, nullptr, e->d_ctr, s);
    e->stats.launches_edge_kernel++;
    HIPCHK(e, hipEventRecord(t1.ev, s));
    HIPCHK(e, hipEventSynchronize(t1.ev));
    float ms = 0;
    if (hipEventElapsedTime(&ms, t0.ev, t1.ev) == hipSuccess) ms_edges += ms;
  }
  e->stats.ms_edge_kernel += ms_edges;
  if ((st = read_ctrs()) != TRG_OK) return st;
  if (bb.h_ctrs[BFS_CTR_ERR]) return fallback(err_text(bb.h_ctrs[BFS_CTR_ERR]));
  const int n_unc2 = bb.h_ctrs[BFS_CTR_NUNC2];
  if (n_unc2 > 0 && (st = resolve_uncertain(n_unc2, B.call_status, sizeof(int), 2, BFS_CTR_NUNC2)) != TRG_OK)
    return st;
  e->stats.ms_deferred = ms_since(t_def);
  return TRG_OK;
}

// ---- phase 5: dedupe + CSR in creation order (and the graph before cleanGraph, on request) ----------
TrgStatus Build::assemble_csr() {
  TrgStatus st;
  t_fin = Clock::now();
  trace_fin = getenv("TRG_TIMING") != nullptr;
  // the edge count is not known to the host before the scatter runs: the arrays are sized by the
  // bound (every call wires at most one pair, two directed entries)
  const size_t e_bound = 2 * (size_t)ncalls, I = sizeof(int), FL = sizeof(float), v1 = (size_t)V + 1;
  if ((st = ensure_all(e, {{&bb.deg, v1 * I}, {&bb.fill, v1 * I}, {&bb.rowptr, (v1 + 1) * I},
                           {&bb.col, (e_bound + 1) * I}, {&bb.seq, (e_bound + 1) * I}, {&bb.w, (e_bound + 1) * FL},
                           {&bb.dist, (e_bound + 1) * FL}, {&bb.new2old, v1 * I}, {&bb.old2new, v1 * I},
                           {&bb.deg_new, v1 * I}, {&bb.rowptr_new, (v1 + 1) * I}, {&bb.keep_flag, v1 * I},
                           {&bb.keep_pos, (v1 + 1) * I}, {&bb.col2, (e_bound + 1) * I}, {&bb.w2, (e_bound + 1) * FL},
                           {&bb.dist2, (e_bound + 1) * FL}, {&bb.xyz2, 3 * v1 * FL}, {&bb.state2, v1 * I}})) != TRG_OK)
    return st;
  F.deg = (int *)bb.deg.p;
  F.fill = (int *)bb.fill.p;
  F.rowptr = (int *)bb.rowptr.p;
  F.col = (int *)bb.col.p;
  F.seq = (int *)bb.seq.p;
  F.w = (float *)bb.w.p;
  F.dist = (float *)bb.dist.p;
  HIPCHK(e, hipMemsetAsync(F.deg, 0, v1 * sizeof(int), s));
  HIPCHK(e, hipMemsetAsync(F.fill, 0, v1 * sizeof(int), s));
  // which call is its pair's edge, and the degrees.  early_copy (no step 3): a pair's first call when it
  // succeeded, so only the pairs of the round-2 calls are reduced
  if (early_copy) launch_fin_insert_count_listed(F, B, ncalls, (int *)bb.sel_list.p, nsel2, s);
  else launch_fin_insert_count(F, B, ncalls, s);
  launch_exclusive_scan(F.deg, F.rowptr, V, (int *)bb.scan_tmp.p, s);
  if (early_copy) {  // the rows are filled behind the renumbering and the node arrays: clean_and_fetch
    lap("insert+count+scan");
    return TRG_OK;
  }
  launch_fin_scatter(F, B, ncalls, true, s);
  lap("insert+count+scan+scatter");
  if (!e->keep_preclean) return TRG_OK;
  // the graph before cleanGraph, edges in push order (tests compare it with the oracle's)
  launch_fin_rowsort(F, V, s);
  if ((st = read_ctrs()) != TRG_OK) return st;
  if (bb.h_ctrs[BFS_CTR_ERR]) return fallback(err_text(bb.h_ctrs[BFS_CTR_ERR]));
  int E = 0;
  HIPCHK(e, hipMemcpy(&E, F.rowptr + V, sizeof(int), hipMemcpyDeviceToHost));
  std::vector<float> h_x(V), h_y(V), h_z(V);
  Csr &c = e->csr_pre;
  c.clear();
  c.xyz.resize(3 * (size_t)V);
  c.state.resize(V);
  c.rowptr.resize((size_t)V + 1);
  c.cid.resize(V);
  c.col.resize(E);
  c.w.resize(E);
  c.dist.resize(E);
  HIPCHK(e, hipMemcpy(c.state.data(), B.nstate, (size_t)V * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(c.rowptr.data(), F.rowptr, ((size_t)V + 1) * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(h_x.data(), B.nx, (size_t)V * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(h_y.data(), B.ny, (size_t)V * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(h_z.data(), B.nz, (size_t)V * sizeof(float), hipMemcpyDeviceToHost));
  for (int i = 0; i < V; ++i) {
    c.xyz[3 * (size_t)i] = h_x[i];
    c.xyz[3 * (size_t)i + 1] = h_y[i];
    c.xyz[3 * (size_t)i + 2] = h_z[i];
    c.cid[i] = i;
  }
  if (E) {
    HIPCHK(e, hipMemcpy(c.col.data(), F.col, (size_t)E * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(c.w.data(), F.w, (size_t)E * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(c.dist.data(), F.dist, (size_t)E * sizeof(float), hipMemcpyDeviceToHost));
  }
  return TRG_OK;
}

// ---- phase 6: cleanGraph (trg.cpp:491-535), renumbering in the reference container's iteration order, and
// the cleaned graph to the host ----
TrgStatus Build::clean_and_fetch() {
  TrgStatus st;
  // (the order went to the device while the deferred evaluations ran, the statistics were summed behind it)
  HIPCHK(e, hipStreamWaitEvent(s, ev_order.ev, 0));
  int *h_tot = bb.h_ctrs + H_CLEAN_TOTALS;
  const hipStream_t cs = early_copy ? copy_stream() : s;  // the stream of the copies to the host
  if (early_copy) {
    // The renumbering and the node arrays need the degrees only (k_fin_keep_flag and k_fin_clean_deg read
    // differences of F.rowptr), and both sizes are known after the scans: Vn = keep_pos[V], E = F.rowptr[V] (every
    // edge survives cleanGraph, checked below).  So they come first, the copy stream takes the sizes and then the
    // node arrays from there, and the main stream fills and orders the rows meanwhile.
    launch_fin_renumber(F, B, (int *)bb.map_order.p, V, (int *)bb.keep_flag.p, (int *)bb.keep_pos.p,
                        (int *)bb.new2old.p, (int *)bb.old2new.p, (int *)bb.deg_new.p, (int *)bb.rowptr_new.p,
                        (int *)bb.scan_tmp.p, s);
    launch_fin_clean_nodes(F, B, V, (int *)bb.keep_pos.p, (int *)bb.new2old.p, (float *)bb.xyz2.p,
                           (int *)bb.state2.p, s);
    HIPCHK(e, hipEventRecord(ev_node_arrays.ev, s));
    edge_stream_busy = true;  // (from here on the main stream and the copy stream hold work nobody waited for)
    HIPCHK(e, hipStreamWaitEvent(cs, ev_node_arrays.ev, 0));
  } else {
    // tail_split: the structure only.  Nothing in it depends on a weight: the kernels up to here and these read
    // call_status & EDGE_STATUS_MASK, call_n1 / _n2, call_dist and the node arrays.
    launch_fin_clean(F, B, (int *)bb.map_order.p, V, (int *)bb.keep_flag.p, (int *)bb.keep_pos.p,
                     (int *)bb.new2old.p, (int *)bb.old2new.p, (int *)bb.deg_new.p, (int *)bb.rowptr_new.p,
                     (int *)bb.scan_tmp.p, (int *)bb.col2.p, tail_split ? nullptr : (float *)bb.w2.p,
                     (float *)bb.dist2.p, (float *)bb.xyz2.p, (int *)bb.state2.p, s);
    // The second stream starts behind the structure kernels, never beside them (k_node_weights rewrites words of
    // call_status / call_w that k_fin_* read).
    if (tail_split) HIPCHK(e, hipEventRecord(ev_structure.ev, s));
  }
  HIPCHK(e, hipMemcpyAsync(h_tot, (int *)bb.keep_pos.p + V, sizeof(int), hipMemcpyDeviceToHost, cs));
  HIPCHK(e, hipMemcpyAsync(h_tot + 1, F.rowptr + V, sizeof(int), hipMemcpyDeviceToHost, cs));
  // the statistics, for report_stats (S64_DEF_KEPT is final since round 2)
  HIPCHK(e, hipMemcpyAsync(bb.h_ctrs + H_STATS64, B.stats64, S64_PHASES * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, cs));
  if (early_copy) {
    HIPCHK(e, hipEventRecord(ev_totals.ev, cs));
    // the rows: entries in arrival order (no weights: the cleaned graph takes them from call_w, FIN_WEIGHTS),
    // then col / dist of the cleaned graph in push order
    launch_fin_scatter(F, B, ncalls, false, s);
    launch_fin_clean_edges(F, B, V, (int *)bb.keep_pos.p, (int *)bb.new2old.p, (int *)bb.old2new.p,
                           (int *)bb.rowptr_new.p, (int *)bb.col2.p, (float *)bb.dist2.p, s);
    HIPCHK(e, hipEventRecord(ev_structure.ev, s));
    HIPCHK(e, hipEventSynchronize(ev_totals.ev));  // the sizes alone: the main stream keeps running
  } else {
    HIPCHK(e, hipStreamSynchronize(s));
  }
  const int Vn = h_tot[0], E = h_tot[1];
  lap("clean kernels");
  Csr &g = e->csr_global;
  g.clear();
  g.rowptr.assign(1, 0);
  if (Vn > 0) {
    // every edge survives: nodes dropped here are Invalid or edgeless and neither has edges
    const int En = E;
    g.rowptr.resize((size_t)Vn + 1);
    g.xyz.resize(3 * (size_t)Vn);
    g.state.resize(Vn);
    g.cid.resize(Vn);
    g.col.resize(En);
    g.w.resize(En);
    g.dist.resize(En);
    // node arrays first: the host rebuilds its node state from them while the edge arrays travel
    // (early_copy: cs is behind ev_node_arrays already, and rowptr, which needs no more than they do, goes with them)
    HIPCHK(e, hipMemcpyAsync(g.xyz.data(), bb.xyz2.p, 3 * (size_t)Vn * sizeof(float), hipMemcpyDeviceToHost, cs));
    if (tail_split && En) {
      // The compute units have nothing to do during these copies: the covariances, the SVDs and the weights of
      // the cleaned graph (a pass over its rows that writes w2 alone) run now, on the second stream, and w2
      // goes last.  (Enqueued behind the first copy so that the copy is under way when the chip fills up.)
      hipStream_t s2 = e->s_edge;
      // (Measured and dropped: k_node_cov, which only reads call_status, in front of this wait, beside
      // k_fin_scatter -- no gain, 37.78 ms per C3 build either way: w does not wait for its weights.)
      HIPCHK(e, hipStreamWaitEvent(s2, ev_structure.ev, 0));
      edge_stream_busy = true;
      launch_creating_edge_weights(s2);
      launch_fin_clean_weights(F, B, V, (int *)bb.keep_pos.p, (int *)bb.new2old.p, (int *)bb.rowptr_new.p,
                               (float *)bb.w2.p, s2);
      HIPCHK(e, hipEventRecord(ev_weights.ev, s2));
    }
    HIPCHK(e, hipMemcpyAsync(g.state.data(), bb.state2.p, (size_t)Vn * sizeof(int), hipMemcpyDeviceToHost, cs));
    HIPCHK(e, hipMemcpyAsync(g.cid.data(), bb.new2old.p, (size_t)Vn * sizeof(int), hipMemcpyDeviceToHost, cs));
    HIPCHK(e, hipEventRecord(ev_nodes.ev, cs));
    HIPCHK(e, hipMemcpyAsync(g.rowptr.data(), bb.rowptr_new.p, ((size_t)Vn + 1) * sizeof(int), hipMemcpyDeviceToHost, cs));
    if (En) {
      if (early_copy) HIPCHK(e, hipStreamWaitEvent(cs, ev_structure.ev, 0));  // (the other orders: same stream)
      HIPCHK(e, hipMemcpyAsync(g.col.data(), bb.col2.p, (size_t)En * sizeof(int), hipMemcpyDeviceToHost, cs));
      HIPCHK(e, hipMemcpyAsync(g.dist.data(), bb.dist2.p, (size_t)En * sizeof(float), hipMemcpyDeviceToHost, cs));
      if (tail_split) HIPCHK(e, hipStreamWaitEvent(cs, ev_weights.ev, 0));
      HIPCHK(e, hipMemcpyAsync(g.w.data(), bb.w2.p, (size_t)En * sizeof(float), hipMemcpyDeviceToHost, cs));
    }
    mark("copies enqueued");
    // while the copies run: global_graph.nodes = new_nodes (trg.cpp:526) -- the copy takes over the
    // source's bucket count, policy state and element order, which is exactly what moving the source
    // in leaves behind
    {
      MapOrderSim new_nodes;  // a fresh container: new_nodes[new_id] = node (trg.cpp:502)
      new_nodes.fill((size_t)Vn);
      e->nodes_sim.assign_from(new_nodes);
    }
    mark("container replica");
    // ... and the host-side graph state (slot == id) as soon as the node arrays are here
    HIPCHK(e, hipEventSynchronize(ev_nodes.ev));
    mark("node arrays here");
    e->nx.resize(Vn);
    e->ny.resize(Vn);
    e->nz.resize(Vn);
    e->nstate.resize(Vn);
    e->ncid.assign(g.cid.data(), g.cid.data() + Vn);
    for (int k = 0; k < Vn; ++k) {
      e->nx[k] = g.xyz[3 * (size_t)k];
      e->ny[k] = g.xyz[3 * (size_t)k + 1];
      e->nz[k] = g.xyz[3 * (size_t)k + 2];
      e->nstate[k] = g.state[k];
    }
    mark("host node state");
    // (the stream of the copies waited for the second one; early_copy: the main stream ended long before them)
    if ((st = read_ctrs()) != TRG_OK) return st;
    if (early_copy) HIPCHK(e, hipStreamSynchronize(cs));
    edge_stream_busy = false;  // all three are drained
    if (bb.h_ctrs[BFS_CTR_ERR]) return fallback(err_text(bb.h_ctrs[BFS_CTR_ERR]));
    if (g.rowptr[Vn] != En) return e->fail(TRG_ERR_DEVICE, "cleanGraph edge count mismatch");
  } else {
    MapOrderSim new_nodes;
    e->nodes_sim.assign_from(new_nodes);
    if ((st = read_ctrs()) != TRG_OK) return st;  // (no copy was enqueued; early_copy: the rows' kernels end here)
    if (early_copy) HIPCHK(e, hipStreamSynchronize(cs));
    edge_stream_busy = false;
    if (bb.h_ctrs[BFS_CTR_ERR]) return fallback(err_text(bb.h_ctrs[BFS_CTR_ERR]));
    e->nx.clear();
    e->ny.clear();
    e->nz.clear();
    e->nstate.clear();
    e->ncid.clear();
  }
  lap("clean kernels + CSR to host");
  e->node_id = Vn;
  lap("host graph state");
  e->history_in_sim = true;  // the real std::unordered_map is rebuilt only if a host path needs it
  // csr_global is here, and xyz2 / rowptr_new / col2 / w2 / dist2 / state2 hold the cleaned graph in HBM; the edge
  // pool, the node grid and the node tree's refill order (trg.cpp:528-530) are derived on demand
  if (Vn > 0) graph_changed(e, {TrgEngine::VIEW_CSR, TrgEngine::VIEW_DEV_CSR});
  else graph_changed(e, {TrgEngine::VIEW_CSR});  // (nothing was cleaned into HBM)
  return TRG_OK;
}

// ---- phase 7: statistics and instrumentation reports -------------------------------------------------
TrgStatus Build::report_stats() {
  // (summed in finish_deferred, fetched into pinned memory in front of clean_and_fetch's first synchronisation)
  unsigned long long s64[S64_PHASES];
  memcpy(s64, bb.h_ctrs + H_STATS64, sizeof(s64));
  if (getenv("TRG_DEBUG_STATS")) {  // the reduction against a host sum of the same arrays
    std::vector<int> hs(V), hx(4 * (size_t)V);
    HIPCHK(e, hipMemcpy(hs.data(), B.nstate, (size_t)V * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(hx.data(), B.nexp, (size_t)V * 16, hipMemcpyDeviceToHost));
    unsigned long long d = 0, a = 0;
    size_t zero = 0;
    for (int i = 0; i < V; ++i)
      if (hs[i] != -1) {
        d += (unsigned long long)hx[4 * (size_t)i + 1];
        a += (unsigned long long)(hx[4 * (size_t)i] & 0xFF);
        zero += hx[4 * (size_t)i + 1] == 0;
      }
    fprintf(stderr, "[trg stats] device draws %llu samples %llu | host sum draws %llu samples %llu | valid nodes with 0 draws %zu\n",
            s64[S64_DRAWS], s64[S64_SAMPLES], d, a, zero);
  }
  if (B.tl) {  // -DLV_TIMELINE=<tag> builds: wall-clock marks of the level kernels (100 MHz), six level attempts
    constexpr int UNITS = 1 << 16, KINDS = 12, TAGS = 6;
    std::vector<unsigned long long> tl((size_t)UNITS * KINDS * TAGS);
    HIPCHK(e, hipMemcpy(tl.data(), B.tl, tl.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    static const char *names[KINDS] = {"sample start", "sample end", "spec start", "spec end", "resolve start",
                                       "resolve collected", "resolve decided(w0)", "resolve published",
                                       "(unused)", "(unused)", "commit start", "commit sums known"};
    for (int t = 0; t < TAGS; ++t) {
      const unsigned long long *base = &tl[(size_t)t * UNITS * KINDS];
      unsigned long long t0 = ~0ull;
      for (int i = 0; i < UNITS; ++i)
        if (base[i]) t0 = std::min(t0, base[i]);
      if (t0 == ~0ull) continue;
      fprintf(stderr, "[trg timeline] level attempt +%d (us after its first sampling workgroup started; n, min, p10, median, p90, max):\n", t);
      for (int k = 0; k < KINDS; ++k) {
        std::vector<double> v;
        for (int i = 0; i < UNITS; ++i)
          if (base[(size_t)k * UNITS + i]) v.push_back(((double)base[(size_t)k * UNITS + i] - (double)t0) / 100.0);
        if (v.empty()) continue;
        std::sort(v.begin(), v.end());
        auto q = [&](double f) { return v[(size_t)(f * (v.size() - 1))]; };
        fprintf(stderr, "[trg timeline]   %-22s n=%6zu  %8.1f %8.1f %8.1f %8.1f %8.1f%s\n", names[k], v.size(), q(0), q(0.1), q(0.5),
                q(0.9), q(1), k >= 4 ? "   (of the PREVIOUS level's resolve launch)" : "");
      }
    }
  }
  if (getenv("TRG_PHASE_TIMING") && ncalls > 0) {
    std::vector<unsigned long long> ph(1024 * 8);
    HIPCHK(e, hipMemcpy(ph.data(), B.stats64 + S64_PHASES, ph.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double t[8] = {0};
    for (size_t i = 0; i < ph.size(); ++i) t[i & 7] += (double)ph[i];
    const double nodes = (double)(ncalls / std::max(S * CS, 1));
    if (getenv("TRG_PHASE_TIMING")[0] == 'r')
      fprintf(stderr, "[trg resolve phases, cycles per workgroup] collect %.0f  decide(wave 0) %.0f  records+stash %.0f  other waves %.0f  look-back %.0f\n",
              t[0] / nodes * (32.0 / S), t[1] / nodes * (32.0 / S), t[2] / nodes * (32.0 / S), t[3] / nodes * (32.0 / S), t[4] / nodes * (32.0 / S));  // (32 slots per resolve workgroup)
    else
    fprintf(stderr, "[trg expand phases, cycles per node] sample: tile %.0f  nodegrid %.0f  sampling %.0f  classify %.0f  hash %.0f  record %.0f | spec (per node): tile %.0f  edges %.0f\n",
            t[0] / nodes, t[1] / nodes, t[2] / nodes, t[3] / nodes, t[4] / nodes, t[5] / nodes, t[6] / nodes, t[7] / nodes);
  }
  e->stats.expanded_nodes = (uint64_t)(ncalls / std::max(S * CS, 1));
  e->stats.trials = s64[S64_DRAWS];
  e->stats.samples = s64[S64_SAMPLES];
  e->stats.created_nodes = bb.nodes_created + 1;  // + root
  e->stats.invalid_nodes = bb.nodes_invalid;
  e->stats.edge_calls = s64[S64_SAMPLES];
  e->stats.edge_evals_gpu = s64[S64_CANDIDATES] + s64[S64_DEF_KEPT];  // speculative parent edges + deferred
  e->lv_hits_sample = s64[S64_DISC_HITS];
  e->lv_hits_spec = s64[S64_SPEC_HITS];
  e->lv_start_known = s64[S64_SPEC_KNOWN];
  e->stats.bytes_spec_created = 12ull * s64[S64_PARENT_HITS];
  e->stats.ms_finalize_host = ms_since(t_fin);
  e->stats.bfs_levels = (uint64_t)levels;
  e->stats.bfs_max_spin = s64[S64_MAX_SPIN];
  // the expansion holds the sampling AND the speculative parent edges of a level: its time is reported as the
  // "sample kernel" (every level's, in ticks of the device's wall clock), its algorithmic bytes are
  // bytes_sample + bytes_spec
  e->stats.ms_sample_kernel += (double)s64[S64_EXPAND_TICKS] / (double)e->wall_clock_khz;
  e->stats.bfs_multipass_rows = s64[S64_MULTIPASS];
  return TRG_OK;
}

// returns TRG_OK, a hard error, or TRG_ERR_CAPACITY with e->bfs_fallback_reason set when the
// caller should redo the build with the host replay
TrgStatus build_graph_device(TrgEngine *e, float root_x, float root_y, float root_z) {
  e->bfs_fallback_reason.clear();
  Build b(e);
  b.B.cstride = b.CS;
  TrgStatus st;
  if ((st = b.allocate()) != TRG_OK) return st;
  if ((st = b.seed_root(root_x, root_y, root_z)) != TRG_OK) return st;
  if ((st = b.level_loop()) != TRG_OK) return st;
  if ((st = b.finish_deferred()) != TRG_OK) return st;
  if ((st = b.assemble_csr()) != TRG_OK) return st;
  if ((st = b.clean_and_fetch()) != TRG_OK) return st;
  return b.report_stats();  // (the events of the build are destroyed with it)
}

}  // namespace
