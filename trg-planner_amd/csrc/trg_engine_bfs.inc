// trg_engine_bfs.inc -- host driver of the device-resident TRG build (included by trg_engine.cpp).
//
// initGraph for configurations whose expandGraph step 3 is disabled (mountain.yaml): the whole BFS
// (trg.cpp:372-454), every wireEdge evaluation, wireEdge's dedupe/push order and cleanGraph's
// compaction run on the GPU; the host launches one batch of kernels per BFS level, reads back a
// handful of counters, decides the (rare) slope gates the device flagged as too close to call with
// the reference's own libm, and computes cleanGraph's renumbering with the same
// std::unordered_map the reference iterates.

namespace {

template <typename T>
TrgStatus dev_ensure(TrgEngine *e, T *&p, size_t &cap, size_t need, bool keep = false) {
  if (cap >= need && p) return TRG_OK;
  size_t ncap = std::max(need, cap + cap / 2);
  T *np = nullptr;
  HIPCHK(e, hipMalloc((void **)&np, ncap * sizeof(T)));
  if (keep && p && cap) {
    hipError_t he = hipMemcpy(np, p, cap * sizeof(T), hipMemcpyDeviceToDevice);
    if (he != hipSuccess) {
      (void)hipFree(np);
      return e->fail(TRG_ERR_DEVICE, std::string("grow copy: ") + hipGetErrorString(he));
    }
  }
  if (p) (void)hipFree(p);
  p = np;
  cap = ncap;
  return TRG_OK;
}

// a device array with its capacity in bytes
struct DevArr {
  void *p = nullptr;
  size_t bytes = 0;
};
TrgStatus ensure_bytes(TrgEngine *e, DevArr &a, size_t need, bool keep = false) {
  if (a.p && a.bytes >= need) return TRG_OK;
  const size_t nb = std::max(need, a.bytes + a.bytes / 2);
  void *np = nullptr;
  HIPCHK(e, hipMalloc(&np, nb));
  if (keep && a.p && a.bytes) {
    hipError_t he = hipMemcpy(np, a.p, a.bytes, hipMemcpyDeviceToDevice);
    if (he != hipSuccess) {
      (void)hipFree(np);
      return e->fail(TRG_ERR_DEVICE, std::string("grow copy: ") + hipGetErrorString(he));
    }
  }
  if (a.p) (void)hipFree(a.p);
  a.p = np;
  a.bytes = nb;
  return TRG_OK;
}

// scratch of the tile-boundary stitch (trg_engine_stitch.inc)
struct StitchBufs {
  DevArr flag, off, cnt, pair_a, pair_b, p1, p2, mid, status, npts, weight, dist, n_unc;
  DevArr extra, deg, rowptr_new, fill, col_new, w_new, dist_new;
  DevArr up_xyz, up_rowptr, up_col, up_w, up_dist;  // uploads when the device copy of the graph is stale
  DevArr scan_tmp;
  std::array<DevArr *, 26> all() {
    return {&flag, &off, &cnt, &pair_a, &pair_b, &p1, &p2, &mid, &status, &npts, &weight, &dist, &n_unc,
            &extra, &deg, &rowptr_new, &fill, &col_new, &w_new, &dist_new, &up_xyz, &up_rowptr, &up_col,
            &up_w, &up_dist, &scan_tmp};
  }
  void release() {
    for (DevArr *a : all())
      if (a->p) (void)hipFree(a->p);
    *this = StitchBufs();
  }
};

// Everything the expansion (k_level_sample + k_level_spec) writes exists twice (level parity): the next level is expanded while the
// host still looks at the counters of this one, and a level whose second half has to be redone must
// find its first half untouched.
struct LevelSet {
  DevArr node_rec;   // NodeRec per frontier node
  DevArr slot_rec;   // SlotRec per sample slot
  DevArr c_outcome;  // int per sample slot
  DevArr lv_hash;    // HashEnt table
  DevArr resc;       // RescueRec per sample slot (builds with expandGraph's step 3 only)
  std::array<DevArr *, 5> all() { return {&node_rec, &slot_rec, &c_outcome, &lv_hash, &resc}; }
  void apply(BfsDev &B) const {
    B.node_rec = (NodeRec *)node_rec.p;
    B.slot_rec = (SlotRec *)slot_rec.p;
    B.c_outcome = (int *)c_outcome.p;
    B.lv_hash = (HashEnt *)lv_hash.p;
    B.resc = use_resc ? (RescueRec *)resc.p : nullptr;
  }
  bool use_resc = false;
};

struct BfsBuffers {
  BfsDev B{};
  FinDev F{};
  LevelSet lv[2];
  DevArr newid_of_call;
  DevArr gcell, ncov, wg_state, nexp, nhits, fxy0, fxy1, def_counts, tl, c_cell, s3_scratch;
  size_t cap_nx = 0, cap_ny = 0, cap_nz = 0, cap_nstate = 0;
  size_t cap_front0 = 0, cap_front1 = 0;
  size_t cap_mid = 0;
  size_t cap_unclist = 0, cap_uncrec = 0, cap_mtrec = 0;
  size_t cap_c1 = 0, cap_c2 = 0, cap_cs = 0, cap_cw = 0, cap_cd = 0;
  size_t cap_ctrs = 0, cap_stats = 0;
  int *flag = nullptr, *scan_tmp = nullptr;
  size_t cap_flag = 0, cap_scantmp = 0;
  // selection of the deferred calls that need evaluating (flags, their scan, the index list)
  int *sel_flag = nullptr, *sel_off = nullptr, *sel_list = nullptr, *sel_tmp = nullptr;
  size_t cap_selflag = 0, cap_seloff = 0, cap_sellist = 0, cap_seltmp = 0;
  // finalize
  size_t cap_fkey = 0, cap_fseq = 0, cap_fslot = 0, cap_fdeg = 0, cap_ffill = 0, cap_frow = 0,
         cap_fok = 0, cap_fcol = 0, cap_fseqe = 0, cap_fw = 0, cap_fdist = 0;
  int *d_new2old = nullptr, *d_old2new = nullptr, *d_deg_new = nullptr, *d_rowptr_new = nullptr,
      *d_col2 = nullptr, *d_state2 = nullptr, *d_map_order = nullptr, *d_keep_flag = nullptr,
      *d_keep_pos = nullptr;
  size_t cap_maporder = 0, cap_keepf = 0, cap_keepp = 0;
  float *d_w2 = nullptr, *d_dist2 = nullptr, *d_xyz2 = nullptr;
  size_t cap_n2o = 0, cap_o2n = 0, cap_degn = 0, cap_rown = 0, cap_col2 = 0, cap_state2 = 0,
         cap_w2 = 0, cap_dist2 = 0, cap_xyz2 = 0;
  int *h_ctrs = nullptr;  // pinned, device-visible: the counters of a level, its stamp in words 5 and 15
  int stamp_serial = 0;
  // host mirror of the node states, filled only when a BFS level has to be replayed on the host
  std::vector<int> hm_state;
  int hm_upto = 0;
  std::vector<float> hm_x, hm_y;  // host mirror of the node positions, extended when a tie has to be broken
  std::vector<int> rp_stamp, rp_head;  // replay_level_on_host: cell -> newest node this replay created
  int rp_serial = 0;
  // statistics of the levels that became final: draws, samples, created, invalid, speculative edges,
  // map points inside sampling discs, map points inside speculative-edge queries
  unsigned long long host_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // [7]: of [6], parent edges of created nodes
  void release() {
    void *ptrs[] = {gcell.p, ncov.p, B.nx, B.ny, B.nz, B.nstate, B.front_cur,
                    B.front_next, B.mid, B.unc_list, B.unc_rec, B.mt_rec, B.call_n1, B.call_n2,
                    B.call_status, B.call_w, B.call_dist, B.ctrs, B.stats64, flag, sel_flag, sel_off,
                    sel_list, sel_tmp, scan_tmp, F.ht_key, F.ht_seq, F.ok_seq, F.call_slot, F.deg, F.fill,
                    F.rowptr, F.col, F.seq, F.w, F.dist, d_new2old, d_old2new, d_deg_new,
                    d_rowptr_new, d_col2, d_state2, d_w2, d_dist2, d_xyz2, newid_of_call.p, wg_state.p, nexp.p, nhits.p, fxy0.p, fxy1.p, def_counts.p, tl.p, c_cell.p, s3_scratch.p,
                    d_map_order, d_keep_flag, d_keep_pos};
    for (void *p : ptrs)
      if (p) (void)hipFree(p);
    for (LevelSet &l : lv)
      for (DevArr *a : l.all())
        if (a->p) (void)hipFree(a->p);
    if (h_ctrs) (void)hipHostFree(h_ctrs);
    *this = BfsBuffers();
  }
};

// One BFS level replayed sequentially on the host (exactly the reference's loop, trg.cpp:406-452),
// consuming what the device already computed for the level: the samples, every sample's nearest
// PRE-LEVEL node (k_level_sample; a slot whose nearest pre-level node was not unique carries
// SLOT_TIE) and the speculative parent edges.  Used when the device met an exact fp32 distance tie
// between two nearest-node candidates -- the reference's answer then depends on its kd-tree's
// traversal order, which kd_tie_winner() (host_index.h) reproduces without building the tree -- or
// when a resolve wait ran out.  Only the nodes this level creates are indexed here (a small cell
// map); the positions of all earlier nodes are fetched only if a tie really has to be broken.
// Afterwards the device BFS continues.
TrgStatus replay_level_on_host(TrgEngine *e, BfsBuffers &bb, int mcur, int V0, long long call_base,
                               int *v_out, int *mnext_out) {
  BfsDev &B = bb.B;
  const int S = e->prm.sample_num;
  const size_t slots = (size_t)mcur * S;
  const float r = e->prm.robot_size;
  hipStream_t s = e->s_main;
  // states of the nodes that exist before this level (kept across replays)
  if (bb.hm_upto < V0) {
    const size_t n = (size_t)(V0 - bb.hm_upto), at = (size_t)bb.hm_upto;
    bb.hm_state.resize(V0);
    HIPCHK(e, hipMemcpy(bb.hm_state.data() + at, B.nstate + at, n * sizeof(int), hipMemcpyDeviceToHost));
    bb.hm_upto = V0;
  }
  bb.hm_state.resize(V0);  // (nodes of a level replayed earlier and then taken back)
  // level inputs: the records k_level_sample / k_level_spec left (candidates are indexed by slot)
  std::vector<int> front(mcur);
  std::vector<NodeRec> nrec(mcur);
  std::vector<SlotRec> srec(slots);
  HIPCHK(e, hipMemcpy(front.data(), B.front_cur, (size_t)mcur * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(nrec.data(), B.node_rec, (size_t)mcur * sizeof(NodeRec), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(srec.data(), B.slot_rec, slots * sizeof(SlotRec), hipMemcpyDeviceToHost));
  unsigned long long C = 0;
  for (size_t i = 0; i < slots; ++i) C += (srec[i].cls & SLOT_CLS_MASK) == 2;
  std::vector<NodeCov> new_cov;  // of the nodes created here, in creation order
  std::vector<float> new_x, new_y, new_z;
  std::vector<int> new_state, new_hits;
  // positions of ALL nodes [0, Vcur), fetched lazily for kd_tie_winner
  std::vector<float> all_x, all_y;
  auto ensure_all_positions = [&](int Vcur) -> TrgStatus {
    if (all_x.empty()) {
      all_x.resize(V0);
      all_y.resize(V0);
      HIPCHK(e, hipMemcpy(all_x.data(), B.nx, (size_t)V0 * sizeof(float), hipMemcpyDeviceToHost));
      HIPCHK(e, hipMemcpy(all_y.data(), B.ny, (size_t)V0 * sizeof(float), hipMemcpyDeviceToHost));
    }
    for (size_t k = all_x.size() - (size_t)V0; (int)(V0 + k) < Vcur; ++k) {
      all_x.push_back(new_x[k]);
      all_y.push_back(new_y[k]);
    }
    return TRG_OK;
  };
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
  auto d2_of = [](float nx_, float ny_, float qx, float qy) {
    float acc = 0;  // the reference's accumulation order (kdtree.c:339-342)
    acc += (nx_ - qx) * (nx_ - qx);
    acc += (ny_ - qy) * (ny_ - qy);
    return acc;
  };
  // sequential replay
  std::vector<int> call_n1(slots), call_n2(slots, -1), call_st(slots, CALL_NONE), next_front, tied;
  std::vector<float> call_w(slots, 0.0f), call_d(slots, 0.0f);
  int Vcur = V0;
  unsigned long long invalid = 0;
  TrgStatus st;
  for (int qpos = 0; qpos < mcur; ++qpos) {
    const int u = front[qpos];
    for (int j = 0; j < S; ++j) {
      const size_t slot = (size_t)qpos * S + j;
      call_n1[slot] = u;
      if (j >= nrec[qpos].n_acc) continue;
      const SlotRec &sr = srec[slot];
      const float qx = sr.x, qy = sr.y;
      // nearest node: the pre-level one the device found ...
      int nn = sr.nn0;
      float best = nn >= 0 ? sr.d0sq : INFINITY;
      tied.clear();
      bool tie = false;
      if (nn >= 0 && (sr.cls & SLOT_TIE)) {  // ... which was not unique: all pre-level nodes that far
        if ((st = ensure_all_positions(Vcur)) != TRG_OK) return st;
        for (int i = 0; i < V0; ++i)
          if (d2_of(all_x[i], all_y[i], qx, qy) == best) tied.push_back(i);
        tie = tied.size() > 1;
      } else if (nn >= 0) {
        tied.push_back(nn);
      }
      // ... against the nodes created earlier in this level
      {
        const float rad = (nn >= 0 ? std::sqrt(best) : e->prm.expand_dist * 1.01f) * 1.001f + 1e-6f;
        const int cx0 = cell_xy(qx - rad, B.gx0, B.GW), cx1 = cell_xy(qx + rad, B.gx0, B.GW);
        const int cy0 = cell_xy(qy - rad, B.gy0, B.GH), cy1 = cell_xy(qy + rad, B.gy0, B.GH);
        for (int cy = cy0; cy <= cy1; ++cy)
          for (int cx = cx0; cx <= cx1; ++cx) {
            const size_t cell = (size_t)cy * B.GW + cx;
            if (bb.rp_stamp[cell] != serial) continue;
            for (int id = bb.rp_head[cell]; id >= 0; id = rp_next[id - V0]) {
              const float dd = d2_of(new_x[id - V0], new_y[id - V0], qx, qy);
              if (dd < best) {
                best = dd;
                nn = id;
                tied.assign(1, id);
                tie = false;
              } else if (dd == best) {
                tied.push_back(id);
                tie = true;
              }
            }
          }
      }
      if (nn < 0) return e->fail(TRG_ERR_DEVICE, "host level replay: a sample without a nearest node");
      if (tie) {
        e->stats.nn_ties++;
        if ((st = ensure_all_positions(Vcur)) != TRG_OK) return st;
        std::sort(tied.begin(), tied.end());
        nn = kd_tie_winner(all_x.data(), all_y.data(), Vcur, qx, qy, tied);
      }
      const int nn_state = nn < V0 ? bb.hm_state[nn] : new_state[nn - V0];
      const float nnx = nn < V0 ? 0.0f : new_x[nn - V0], nny = nn < V0 ? 0.0f : new_y[nn - V0];
      if (nn_state == TRG_NODE_INVALID) continue;                                // trg.cpp:411-413
      // (existing - sample).norm() < robot_size: the distance is `best` whichever node it is
      (void)nnx;
      (void)nny;
      if (std::sqrt(best) < r) {                                                   // trg.cpp:414-417
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
      new_x.push_back(qx);
      new_y.push_back(qy);
      new_z.push_back(sr.z);
      new_state.push_back(ok ? TRG_NODE_VALID : TRG_NODE_INVALID);
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
        for (int q = 0; q < 6; ++q) nc.cov[q] = sr.cov[q];
        nc.w_given = sr.w_given;
        nc.call = (int)(call_base + (long long)slot);
      } else {
        invalid++;
      }
      new_cov.push_back(nc);
    }
  }
  const int created = Vcur - V0;
  bb.hm_state.insert(bb.hm_state.end(), new_state.begin(), new_state.end());
  bb.hm_upto = Vcur;
  bb.host_stats[2] += (unsigned long long)created;
  bb.host_stats[3] += invalid;
  (void)C;  // (draws / samples / candidates / hit counts: per-node records, summed after the loop)
  if (Vcur > B.vcap || (int)next_front.size() > B.fcap)
    return e->fail(TRG_ERR_CAPACITY, "host level replay: capacity");
  // hand the level's results to the device
  if (created > 0) {
    const size_t at = (size_t)V0, n = (size_t)created;
    HIPCHK(e, hipMemcpy(B.nx + at, new_x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(B.ny + at, new_y.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(B.nz + at, new_z.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(B.nstate + at, new_state.data(), n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(B.ncov + at, new_cov.data(), n * sizeof(NodeCov), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(B.nhits + at, new_hits.data(), n * sizeof(int), hipMemcpyHostToDevice));
    launch_bfs_insert_nodes(B, V0, created, s);
  }
  if (!next_front.empty()) {
    HIPCHK(e, hipMemcpy(B.front_next, next_front.data(), next_front.size() * sizeof(int),
                        hipMemcpyHostToDevice));
    std::vector<float> fxy(2 * next_front.size());
    for (size_t k = 0; k < next_front.size(); ++k) {
      fxy[2 * k] = new_x[next_front[k] - V0];
      fxy[2 * k + 1] = new_y[next_front[k] - V0];
    }
    HIPCHK(e, hipMemcpy(B.fxy_next, fxy.data(), fxy.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  const size_t cb = (size_t)call_base;
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
  *v_out = Vcur;
  *mnext_out = (int)next_front.size();
  e->stats.bfs_host_levels++;
  return TRG_OK;
}

constexpr int BFS_FCAP = 1 << 16;       // nodes per BFS level the device path accepts
constexpr int CALL_EVAL_BATCH = 1 << 22;  // calls per selection / evaluation chunk (sizes the edge scratch)
// repaired by replaying ONE level on the host (or, for a tie among pre-level nodes only, by handing
// k_level_resolve the reference's winner)
constexpr int BFS_ERR_SOFT = BFS_ERR_TIE | BFS_ERR_STALL | BFS_ERR_TIE_CLS;

// returns TRG_OK, a hard error, or TRG_ERR_CAPACITY with e->bfs_fallback_reason set when the
// caller should redo the build with the host replay
TrgStatus build_graph_device(TrgEngine *e, float root_x, float root_y, float root_z) {
  BfsBuffers &bb = *e->bfs;
  BfsDev &B = bb.B;
  FinDev &F = bb.F;
  const int S = e->prm.sample_num;
  // call-log entries per sample slot: with expandGraph's step 3 on, every slot's own call is followed by room
  // for the neighbour calls of the node it creates (debug_call_stride: the sparse log on any configuration)
  const int CS = (e->step3 || e->debug_call_stride) ? LEVEL_STEP3_STRIDE : 1;
  B.cstride = CS;
  const QueryParams qp = qparams(e);
  hipStream_t s = e->s_main;
  e->bfs_fallback_reason.clear();
  auto fallback = [&](const std::string &why) {
    e->bfs_fallback_reason = why;
    return TRG_ERR_CAPACITY;
  };

  // ---- geometry of the node grid and capacities ------------------------------------------------
  DevMap &m = e->gmap;
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
#define ENS(ptr, capf, need) \
  if ((st = dev_ensure(e, ptr, bb.capf, (size_t)(need))) != TRG_OK) return st
#define ENSB(arr, bytes) \
  if ((st = ensure_bytes(e, arr, (size_t)(bytes))) != TRG_OK) return st
  ENS(B.nx, cap_nx, vcap);
  ENS(B.ny, cap_ny, vcap);
  ENS(B.nz, cap_nz, vcap);
  ENS(B.nstate, cap_nstate, vcap);
  B.vcap = (int)std::min<size_t>(vcap, 0x7FFFFFF0);
  ENSB(bb.gcell, ncell * sizeof(GridCell));
  B.gcell = (GridCell *)bb.gcell.p;
  ENSB(bb.ncov, vcap * sizeof(NodeCov));
  B.ncov = (NodeCov *)bb.ncov.p;
  ENS(B.front_cur, cap_front0, fcap);
  ENS(B.front_next, cap_front1, fcap);
  ENSB(bb.fxy0, fcap * sizeof(float2));
  ENSB(bb.fxy1, fcap * sizeof(float2));
  B.fxy_cur = (float2 *)bb.fxy0.p;
  B.fxy_next = (float2 *)bb.fxy1.p;
  B.fcap = (int)fcap;
  size_t ht_need = 1024;
  while (ht_need < 2 * slots) ht_need <<= 1;
  for (LevelSet &l : bb.lv) {
    ENSB(l.node_rec, fcap * sizeof(NodeRec));
    ENSB(l.slot_rec, slots * sizeof(SlotRec));
    ENSB(l.c_outcome, slots * sizeof(int));
    ENSB(l.lv_hash, ht_need * sizeof(HashEnt));
    l.use_resc = e->step3;
    if (e->step3) ENSB(l.resc, slots * sizeof(RescueRec));
    // tags start at 1 in every build: entries of earlier builds must not look current
    HIPCHK(e, hipMemsetAsync(l.lv_hash.p, 0, ht_need * sizeof(HashEnt), s));
  }
  ENS(B.mid, cap_mid, edge_mid_floats(CALL_EVAL_BATCH));
  ENS(B.unc_list, cap_unclist, 3 * BFS_UNC_CAP + BFS_TIE_CAP);  // even levels, odd levels, deferred evaluations; tied slots
  B.tie_list = B.unc_list + 3 * BFS_UNC_CAP;
  ENS(B.unc_rec, cap_uncrec, 3 * 3 * BFS_UNC_CAP);
  ENS(B.mt_rec, cap_mtrec, 2 * MAPTIE_CAP);
  ENS(B.ctrs, cap_ctrs, BFS_CTR_COUNT);
  ENS(B.stats64, cap_stats, 16 + 1024 * 8);
  ENS(bb.flag, cap_flag, slots + 1);
  ENSB(bb.wg_state, (slots / 16 + 64 + 8) * sizeof(unsigned long long));  // (>= one word per resolve workgroup)
  B.wg_state = (unsigned long long *)bb.wg_state.p;
  HIPCHK(e, hipMemsetAsync(B.wg_state, 0, (slots / 16 + 64 + 8) * sizeof(unsigned long long), s));  // epochs start at 1
  B.ticket = (unsigned *)(B.wg_state + (slots / 16 + 64));  // start tickets of the resolve workgroups: zero, like
  unsigned ticket_base = 0;                                   // the host's count of the tickets drawn so far
  B.tl = nullptr;
  if (getenv("TRG_TIMELINE")) {
    const size_t tl_bytes = (size_t)(1 << 16) * 12 * 6 * sizeof(unsigned long long);
    ENSB(bb.tl, tl_bytes);
    B.tl = (unsigned long long *)bb.tl.p;
    HIPCHK(e, hipMemsetAsync(B.tl, 0, tl_bytes, s));
  }
  ENSB(bb.c_cell, slots * sizeof(unsigned long long));
  B.c_cell = (unsigned long long *)bb.c_cell.p;
  HIPCHK(e, hipMemsetAsync(B.c_cell, 0, slots * sizeof(unsigned long long), s));  // (launch epochs start at 1 in every build)
  ENSB(bb.nexp, vcap * sizeof(int4));
  B.nexp = (int4 *)bb.nexp.p;
  ENSB(bb.nhits, vcap * sizeof(int));
  B.nhits = (int *)bb.nhits.p;
  ENS(bb.scan_tmp, cap_scantmp, std::max(slots, vcap) / 2048 + 8);
  if (!bb.h_ctrs) {
    HIPCHK(e, hipHostMalloc((void **)&bb.h_ctrs, 64 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
    memset(bb.h_ctrs, 0, 64 * sizeof(int));
  }
  {
    void *dp = nullptr;
    HIPCHK(e, hipHostGetDevicePointer(&dp, bb.h_ctrs, 0));
    B.host_ctrs = (int *)dp;
  }

  bb.hm_state.clear();
  bb.hm_upto = 0;
  bb.hm_x.clear();
  bb.hm_y.clear();
  for (auto &v : bb.host_stats) v = 0;
  HIPCHK(e, hipMemsetAsync(B.gcell, 0, ncell * sizeof(GridCell), s));
  HIPCHK(e, hipMemsetAsync(B.ctrs, 0, BFS_CTR_COUNT * sizeof(int), s));
  HIPCHK(e, hipMemsetAsync(B.stats64, 0, (16 + 1024 * 8) * sizeof(unsigned long long), s));

  // ---- root node ---------------------------------------------------------------------------------
  {
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
  }

  auto read_ctrs = [&]() -> TrgStatus {
    HIPCHK(e, hipMemcpyAsync(bb.h_ctrs, B.ctrs, BFS_CTR_COUNT * sizeof(int), hipMemcpyDeviceToHost, s));
    auto t0 = Clock::now();
    HIPCHK(e, hipStreamSynchronize(s));
    e->stats.ms_wait_gpu += ms_since(t0);
    return TRG_OK;
  };
  // The level's counters reach the host without a copy in the stream: the last workgroup of
  // the next level's k_level_sample writes them into pinned host memory with the level's stamp; the host polls
  // the stamp.
  int &stamp_serial = bb.stamp_serial;  // monotonic over the engine's life: a stale block never matches
  constexpr long poll_query_mask = 0xFFFFFL;
  auto wait_stamp = [&](int stamp) -> TrgStatus {
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
  };
  auto err_text = [](int code) {
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
  };
  // host decision of the slope gates the device could not call (reference libm, trg.cpp:269-274);
  // list: the parity's half of unc_list / unc_rec, entries index status_array
  std::vector<int> unc_idx;
  std::vector<float> unc_rec;
  bool unc_changed = false;  // set when a provisional "not gated" turned out to be gated
  auto resolve_uncertain = [&](int n_unc, void *status_base, size_t stride, int list_parity,
                               int ctr_index) -> TrgStatus {
    unc_changed = false;
    if (n_unc > BFS_UNC_CAP) return fallback("too many uncertain slope gates in one batch");
    unc_idx.resize(n_unc);
    unc_rec.resize(3 * (size_t)n_unc);
    HIPCHK(e, hipMemcpy(unc_idx.data(), B.unc_list + (size_t)list_parity * BFS_UNC_CAP,
                        n_unc * sizeof(int), hipMemcpyDeviceToHost));
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
      } else {
        stt &= ~EDGE_GATE_UNCERTAIN;
      }
      HIPCHK(e, hipMemcpy(addr, &stt, sizeof(int), hipMemcpyHostToDevice));
    }
    const int zero = 0;
    HIPCHK(e, hipMemcpy(B.ctrs + ctr_index, &zero, sizeof(int), hipMemcpyHostToDevice));
    return TRG_OK;
  };
  auto slot_status = [&]() { return (void *)((char *)B.slot_rec + offsetof(SlotRec, status)); };

  // ---- deferred wireEdge evaluations (node -> existing node), pipelined behind the level loop -------
  // wireEdge returns at once when a pair is already wired (trg.cpp:255-267), so per unordered pair
  // only its FIRST call is evaluated, then (after the loop) the remaining calls of the few pairs
  // whose first call did not succeed.  "First call of its pair" is final as soon as the call's
  // level is: the calls of finished levels are therefore handed over in batches to a second, low
  // priority stream, where they fill the issue slots the latency-bound level kernels leave idle.
  // The pair table is sized from the node capacity bound (every node is expanded at most once).
  const size_t calls_bound = std::min<size_t>(vcap * (size_t)std::max(S, 1) * (size_t)CS, 0x7FFFFFF0u);
  unsigned fht = 1024;
  while ((unsigned long long)fht < (unsigned long long)calls_bound && fht < (1u << 31)) fht <<= 1;
  ENS(F.ht_key, cap_fkey, fht);
  ENS(F.ht_seq, cap_fseq, fht);
  ENS(F.ok_seq, cap_fok, fht);
  F.ht_size = fht;
  // calls per batch (at least): about one batch per BFS level -- many small batches disturb the level
  // kernels least (measured: 3.2 M -> 54.6 ms per C3 build, 100 k -> 53.2, 6 k -> 51.6; no overlap 54.5)
  constexpr long long DEF_BATCH_MIN = 6000;
  const size_t sel_cap = (size_t)CALL_EVAL_BATCH + 2;
  ENS(bb.sel_flag, cap_selflag, sel_cap);
  ENS(bb.sel_off, cap_seloff, sel_cap + 1);
  ENS(bb.sel_tmp, cap_seltmp, sel_cap / 2048 + 16);
  // With step 3 the neighbour calls of a node sit BEFORE later calls in the log but are only known after the
  // loop (trg_step3.inc): "first call of its pair" is not final level by level, so nothing is evaluated beside
  // the loop.
  const bool overlap = !e->step3 && e->defer_overlap;
  if (overlap) {  // (otherwise the table is cleared after the loop, right before its first use)
    HIPCHK(e, hipMemsetAsync(F.ht_key, 0xFF, (size_t)fht * sizeof(unsigned long long), s));
    HIPCHK(e, hipMemsetAsync(F.ht_seq, 0x7F, (size_t)fht * sizeof(int), s));
  }
  HIPCHK(e, hipMemsetAsync(F.ok_seq, 0x7F, (size_t)fht * sizeof(int), s));  // (first used after the loop)
  hipStream_t s_def = overlap ? e->s_edge : s;
  long long def_lo = 0;  // first call not yet handed to the deferred pipeline
  std::vector<std::pair<hipEvent_t, hipEvent_t>> def_events;
  constexpr int TIMED_BATCH_EVERY = 8;
  size_t n_eval_batches = 0;
  unsigned long long *d_def_total = B.stats64 + 5;  // calls the selections kept (device counter)
  ENSB(bb.def_counts, sizeof(int));  // round 2's count of selected calls
  auto eval_batch = [&](long long lo, long long n, const int *count_dev, hipStream_t st_) -> TrgStatus {
    hipEvent_t a = nullptr, b = nullptr;
    // (timed like the level kernels: every 8th batch, scaled up afterwards -- an event pair per batch was
    // a fifth of the host's launch work per level)
    if ((n_eval_batches++ % TIMED_BATCH_EVERY) == 0 && def_events.size() < 8192) {
      HIPCHK(e, hipEventCreate(&a));
      HIPCHK(e, hipEventCreate(&b));
      HIPCHK(e, hipEventRecord(a, st_));
    }
    // the number of selected calls lives on the device: the grid is an upper bound
    launch_calls_eval(m.view, qp, B, bb.sel_list + lo, (int)n, count_dev, e->d_ctr, st_);
    e->stats.launches_edge_kernel++;
    if (a) {
      HIPCHK(e, hipEventRecord(b, st_));
      def_events.emplace_back(a, b);
    }
    return TRG_OK;
  };
  // calls [def_lo, c1) of finished levels -> pair table, first-of-pair selection, evaluation
  auto launch_deferred = [&](long long c1, bool in_loop) -> TrgStatus {
    while (def_lo < c1) {
      const long long c_hi = std::min<long long>(c1, def_lo + CALL_EVAL_BATCH);
      const long long n = c_hi - def_lo;
      hipStream_t st_ = in_loop ? s_def : s;
      launch_first_insert(F, B, def_lo, c_hi, st_);
      launch_calls_select(F, B, def_lo, c_hi, 1, bb.sel_flag, bb.sel_off, bb.sel_tmp, bb.sel_list + def_lo,
                          d_def_total, st_);
      TrgStatus r = eval_batch(def_lo, n, bb.sel_off + n, st_);
      if (r != TRG_OK) return r;
      def_lo = c_hi;
    }
    return TRG_OK;
  };

  // ---- level loop ----------------------------------------------------------------------------------
  hipEvent_t ev0, ev1, evn0, evn1, ev_order, ev_nodes;
  HIPCHK(e, hipEventCreate(&ev0));
  HIPCHK(e, hipEventCreate(&ev1));
  HIPCHK(e, hipEventCreate(&evn0));
  HIPCHK(e, hipEventCreate(&evn1));
  HIPCHK(e, hipEventCreateWithFlags(&ev_order, hipEventDisableTiming));
  HIPCHK(e, hipEventCreateWithFlags(&ev_nodes, hipEventDisableTiming));
  bool have_expand = false;  // this level's expansion was issued by the previous iteration
  // Kernel timing inside the level loop is SAMPLED: an event pair around a kernel costs ~12 us of
  // stream time.  Every TIMED_EVERY-th level is timed and the totals are scaled by
  // launches / timed launches at the end (levels change slowly, so the subsample is unbiased).
  constexpr int TIMED_EVERY = 8;
  auto timed_level = [&](int level) { return level % TIMED_EVERY == 0; };
  double ms_expand_timed = 0;
  uint64_t n_expand_timed = 0, n_expand_all = 0;
  bool expand_events_valid = false;  // ev0/ev1 bracket the expand launch of the current level
  int mcur = 1;
  int v_now = 1;  // nodes that exist before the current level (the root)
  long long call_base = 0;
  int levels = 0;
  int tag_serial = 0;        // one hash tag per level attempt
  int cur_tag = 0;
  int cur_ht = 0;            // hash size the current level's expand used
  auto ht_for = [&](size_t nodes) {
    int ht = 1024;
    while ((size_t)ht < 2 * nodes * (size_t)S) ht <<= 1;
    return ht;
  };
  int res_epoch = 0;  // one per k_level_resolve launch: the look-back words of other launches do not count
  auto t_loop = Clock::now();
  while (mcur > 0) {
    const size_t level_slots = (size_t)mcur * S;
    const size_t need_calls = (size_t)call_base + level_slots * (size_t)CS;
    if (bb.cap_c1 < need_calls) {
      const size_t want = std::max(need_calls, std::max<size_t>(bb.cap_c1 * 2, (size_t)4 << 20));
      // the grow copies run on the NULL stream, which does not wait for the (non-blocking) level and
      // deferred streams: everything that still writes the call log must have finished first
      HIPCHK(e, hipStreamSynchronize(s));
      if (s_def != s) HIPCHK(e, hipStreamSynchronize(s_def));
      if ((st = dev_ensure(e, B.call_n1, bb.cap_c1, want, true)) != TRG_OK) return st;
      if ((st = dev_ensure(e, B.call_n2, bb.cap_c2, want, true)) != TRG_OK) return st;
      if ((st = dev_ensure(e, B.call_status, bb.cap_cs, want, true)) != TRG_OK) return st;
      if ((st = dev_ensure(e, B.call_w, bb.cap_cw, want, true)) != TRG_OK) return st;
      if ((st = dev_ensure(e, B.call_dist, bb.cap_cd, want, true)) != TRG_OK) return st;
      if ((st = ensure_bytes(e, bb.newid_of_call, want * sizeof(int), true)) != TRG_OK) return st;
      B.newid_of_call = (int *)bb.newid_of_call.p;
      if ((st = dev_ensure(e, F.call_slot, bb.cap_fslot, want, true)) != TRG_OK) return st;
      if ((st = dev_ensure(e, bb.sel_list, bb.cap_sellist, want + 1, true)) != TRG_OK) return st;
    }
    const int parity = levels & 1;
    bb.lv[parity].apply(B);
    if (levels == e->debug_fallback_level) {
      HIPCHK(e, hipStreamSynchronize(s));
      return fallback("declined on request (debug_fallback_level)");
    }
    if (!have_expand) {
      cur_tag = ++tag_serial;
      cur_ht = ht_for((size_t)mcur);
      B.ht_size = cur_ht;
      HIPCHK(e, hipEventRecord(ev0, s));
      launch_level_expand(m.view, qp, e->d_cos, e->d_sin, e->sampler.table_bits, e->sampler.seed,
                          e->epoch, B, mcur, nullptr, 0, parity, cur_tag, 0, e->d_ctr, s);
      HIPCHK(e, hipEventRecord(ev1, s));
      expand_events_valid = true;
    }
    B.ht_size = cur_ht;
    // The rest of the level is launched at once and the host looks at the counters once, at the end.
    // The device treats a slope gate it could not call as "not gated" and a nearest-node tie as
    // "lowest id"; when either happened (rare) the level's commit is taken back, the host supplies
    // the exact answer, and resolve + commit run again / the level is replayed on the host.
    const int V0 = v_now;
    // The next level's record set, hash size and tag: its expansion is launched right behind this
    // level's resolve, before the host has seen this level's counters (the frontier size is read from
    // the device, the grid is an upper bound).
    BfsDev Bn = B;
    std::swap(Bn.front_cur, Bn.front_next);
    std::swap(Bn.fxy_cur, Bn.fxy_next);
    bb.lv[parity ^ 1].apply(Bn);
    const size_t next_cap_nodes =
        std::min<size_t>((size_t)B.fcap, std::max<size_t>(2 * (size_t)mcur, (size_t)mcur + 1024));
    const int next_ht = ht_for(next_cap_nodes);
    Bn.ht_size = next_ht;
    int spec_bound = (int)std::min<size_t>(
        (size_t)B.fcap, std::min<size_t>(level_slots, (size_t)(mcur + std::max(128, mcur / 4))));
    if (e->debug_spec_bound > 0) spec_bound = std::min(spec_bound, e->debug_spec_bound);
    const bool next_timed = timed_level(levels + 1);
    int next_tag = ++tag_serial;
    const int stall_hook = levels == e->debug_stall_level ? 1 : (levels == e->debug_lookback_level ? 2 : 0);
    launch_level_resolve_commit(B, qp, mcur, TRG_NODE_VALID, call_base, V0, cur_tag, ++res_epoch, s, stall_hook,
                                e->resolve_tickets != 0, &ticket_base);
    const int stamp = ++stamp_serial;  // published by the next level's expansion, launched right below
    if (next_timed) HIPCHK(e, hipEventRecord(evn0, s));
    launch_level_expand(m.view, qp, e->d_cos, e->d_sin, e->sampler.table_bits, e->sampler.seed,
                        e->epoch, Bn, spec_bound, B.ctrs + BFS_CTR_MNEXT, 0, parity ^ 1, next_tag, stamp,
                        e->d_ctr, s);
    if (next_timed) HIPCHK(e, hipEventRecord(evn1, s));
    bool next_events_valid = next_timed;
    bool reexpand = false;  // set when the level's commit was redone: the frontier may differ
    if ((st = wait_stamp(stamp)) != TRG_OK) return st;
    {
      float ms = 0;
      if (expand_events_valid && hipEventQuery(ev1) == hipSuccess &&
          hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) {
        ms_expand_timed += ms;
        n_expand_timed++;
      }
      n_expand_all++;
    }
    int err = bb.h_ctrs[BFS_CTR_ERR];
    // test hook: pretend a tie was seen so that the undo + host-level replay are exercised on
    // data that has no real tie
    if (e->debug_tie_every > 0 && levels > 0 && levels % e->debug_tie_every == 0) err |= BFS_ERR_TIE;
    if (err && getenv("TRG_TRACE_LEVELS"))
      fprintf(stderr, "[trg bfs] level %d: err=%d (%s) mcur=%d v=%d mnext=%d\n", levels, err,
              err_text(err).c_str(), mcur, bb.h_ctrs[BFS_CTR_V], bb.h_ctrs[BFS_CTR_MNEXT]);
    int mnext = bb.h_ctrs[BFS_CTR_MNEXT];
    int v_after = bb.h_ctrs[BFS_CTR_V];
    const int unc_ctr = parity ? BFS_CTR_NUNC1 : BFS_CTR_NUNC;
    int n_unc = bb.h_ctrs[unc_ctr];
    const int n_mt = bb.h_ctrs[BFS_CTR_NMAPTIE + parity];
    // nodes this level created / created Invalid (a level replayed on the host counts its own)
    unsigned long long lvl_stats[2] = {(unsigned long long)(v_after - V0),
                                       (unsigned long long)(v_after - V0 - mnext)};
    int err_from_sample = err & BFS_ERR_TIE_CLS;
    auto undo_level = [&]() -> TrgStatus {
      reexpand = true;
      HIPCHK(e, hipStreamSynchronize(s));  // the next level's expansion (now void) must be out of the way
      launch_bfs_undo_slots(B, (int)level_slots, s);
      // k_level_resolve polls outcomes: a rerun must find them undecided again
      HIPCHK(e, hipMemsetAsync(B.c_outcome, 0, level_slots * sizeof(int), s));
      int ctr_host[BFS_CTR_COUNT] = {0};
      ctr_host[BFS_CTR_V] = V0;
      HIPCHK(e, hipMemcpy(B.ctrs, ctr_host, BFS_CTR_NUNC2 * sizeof(int), hipMemcpyHostToDevice));  // (the deferred pipeline owns NUNC2)
      return TRG_OK;
    };
    auto rerun_second_half = [&](bool ticketed = false, int hook = 0) -> TrgStatus {
      launch_level_resolve_commit(B, qp, mcur, TRG_NODE_VALID, call_base, V0, cur_tag, ++res_epoch, s, hook,
                                  ticketed || e->resolve_tickets != 0, &ticket_base);
      TrgStatus r = read_ctrs();  // (rare path: a plain copy)
      if (r != TRG_OK) return r;
      // (what k_level_sample reported about the level stays true: that kernel does not run again)
      err = bb.h_ctrs[BFS_CTR_ERR] | err_from_sample;
      if (e->debug_tie_every > 0 && levels > 0 && levels % e->debug_tie_every == 0) err |= BFS_ERR_TIE;
      mnext = bb.h_ctrs[BFS_CTR_MNEXT];
      v_after = bb.h_ctrs[BFS_CTR_V];
      lvl_stats[0] = (unsigned long long)(v_after - V0);
      lvl_stats[1] = (unsigned long long)(v_after - V0 - mnext);
      return TRG_OK;
    };
    auto settle_ties_in_place = [&](bool *settled) -> TrgStatus {
      *settled = false;
      int ntie = 0;
      HIPCHK(e, hipMemcpy(&ntie, B.ctrs + BFS_CTR_NTIE, sizeof(int), hipMemcpyDeviceToHost));
      if (ntie <= 0 || ntie > BFS_TIE_CAP) return TRG_OK;
      std::vector<int> tslots(ntie);
      HIPCHK(e, hipMemcpy(tslots.data(), B.tie_list, (size_t)ntie * sizeof(int), hipMemcpyDeviceToHost));
      std::sort(tslots.begin(), tslots.end());
      tslots.erase(std::unique(tslots.begin(), tslots.end()), tslots.end());
      if (tslots.front() < 0 || (size_t)tslots.back() >= level_slots) return TRG_OK;
      // which slots created a node (outcomes 3 / 4): the nodes that existed at a slot's turn are
      // V0 + the creations of the slots before it
      std::vector<int> oc((size_t)tslots.back() + 1);
      HIPCHK(e, hipMemcpy(oc.data(), B.c_outcome, oc.size() * sizeof(int), hipMemcpyDeviceToHost));
      if ((int)bb.hm_x.size() < v_after) {  // positions: kd_tie_winner walks them in insertion order
        const size_t at = bb.hm_x.size(), n = (size_t)v_after - at;
        bb.hm_x.resize(v_after);
        bb.hm_y.resize(v_after);
        HIPCHK(e, hipMemcpy(bb.hm_x.data() + at, B.nx + at, n * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(bb.hm_y.data() + at, B.ny + at, n * sizeof(float), hipMemcpyDeviceToHost));
      }
      const float *ax = bb.hm_x.data(), *ay = bb.hm_y.data();
      auto d2_of = [](float nx_, float ny_, float qx, float qy) {
        float acc = 0;  // the reference's accumulation order (kdtree.c:339-342)
        acc += (nx_ - qx) * (nx_ - qx);
        acc += (ny_ - qy) * (ny_ - qy);
        return acc;
      };
      struct Patch {
        size_t at;
        int n2, st;
      };
      std::vector<Patch> patches;
      std::vector<int> tied;
      size_t scanned = 0;
      int created_before = 0;
      for (int sl : tslots) {
        for (; scanned < (size_t)sl; ++scanned) created_before += (oc[scanned] == 3 || oc[scanned] == 4);
        const int V_at = V0 + created_before;
        SlotRec sr;
        int u = -1;
        HIPCHK(e, hipMemcpy(&sr, B.slot_rec + sl, sizeof(SlotRec), hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(&u, B.front_cur + sl / S, sizeof(int), hipMemcpyDeviceToHost));
        if ((sr.cls & SLOT_CLS_MASK) == 0) continue;
        // nearest node: the pre-level one the device found (all of them if that was not unique) ...
        float best = sr.nn0 >= 0 ? sr.d0sq : INFINITY;
        tied.clear();
        if (sr.nn0 >= 0 && (sr.cls & SLOT_TIE)) {
          for (int i = 0; i < V0; ++i)
            if (d2_of(ax[i], ay[i], sr.x, sr.y) == best) tied.push_back(i);
        } else if (sr.nn0 >= 0) {
          tied.push_back(sr.nn0);
        }
        // ... against the nodes this level created before the slot's turn
        for (int i = V0; i < V_at; ++i) {
          const float dd = d2_of(ax[i], ay[i], sr.x, sr.y);
          if (dd < best) {
            best = dd;
            tied.assign(1, i);
          } else if (dd == best) {
            tied.push_back(i);
          }
        }
        if (tied.empty()) return TRG_OK;
        int nn = tied[0];
        if (tied.size() > 1) {
          e->stats.nn_ties++;
          std::sort(tied.begin(), tied.end());
          nn = kd_tie_winner(ax, ay, V_at, sr.x, sr.y, tied);
        }
        int nn_state = 0;
        HIPCHK(e, hipMemcpy(&nn_state, B.nstate + nn, sizeof(int), hipMemcpyDeviceToHost));
        const int kind = nn_state == TRG_NODE_INVALID ? 1 : (std::sqrt(best) < e->prm.robot_size ? 2 : 3);
        const bool dev_creates = oc[sl] == 3 || oc[sl] == 4;
        if ((kind == 3) != dev_creates) return TRG_OK;  // the level's node set is in doubt: replay it
        if (kind == 3) continue;                          // creates either way: its record stands
        patches.push_back({(size_t)call_base + (size_t)sl, kind == 2 ? nn : -1,
                           (kind == 2 && nn != u) ? CALL_PENDING : CALL_NONE});
      }
      for (const Patch &pt : patches) {
        HIPCHK(e, hipMemcpy(B.call_n2 + pt.at, &pt.n2, sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(B.call_status + pt.at, &pt.st, sizeof(int), hipMemcpyHostToDevice));
      }
      launch_bfs_clear_tie(B, s);
      *settled = true;
      return TRG_OK;
    };
    if (e->step3 && n_unc > 0)
      // (the rescue search of k_level_spec3 ran on the provisional verdict of that gate)
      return fallback("a slope gate left to the host's libm in a build with expandGraph's step 3");
    if (CS > 1 && ((err & BFS_ERR_SOFT & ~BFS_ERR_STALL) || n_mt > 0))
      // (the host repairs of nearest-node ties and map-point ties are written for the dense call log and
      // know nothing of step 3: such a build goes to the host replay as a whole)
      return fallback("exact fp32 distance tie in a build with expandGraph's step 3");
    bool undone = false;
    const auto t_rare = Clock::now();
    const bool any_rare = n_mt > 0 || n_unc > 0 || (err & (BFS_ERR_SOFT | BFS_ERR_LOOKBACK));
    constexpr int ERR_WAIT = BFS_ERR_STALL | BFS_ERR_LOOKBACK;
    if ((err & ERR_WAIT) && !(err & ~(BFS_ERR_SOFT | ERR_WAIT))) {
      // A bounded wait of the resolve launch ran out: the hardware did not start its workgroups in index
      // order (another process's kernels on the card).  The level is taken back and the launch repeated
      // with start tickets as logical indices: every wait is then for a workgroup that is already
      // running, whatever the dispatch order.  (Test hook debug_wait_rerun: the repeat fails as well.)
      if ((st = undo_level()) != TRG_OK) return st;
      const int hook = e->debug_wait_rerun ? ((err & BFS_ERR_LOOKBACK) ? 2 : 1) : 0;
      if ((st = rerun_second_half(true, hook)) != TRG_OK) return st;
      e->stats.bfs_ticket_reruns++;
    }
    if (err & ~BFS_ERR_SOFT) {
      if (any_rare) e->stats.ms_rare_events += ms_since(t_rare);
      return fallback(err_text(err));
    }
    if (n_mt > 0) {
      // accepted samples whose elevation hung on a nearest-map-point tie: the device took the lowest
      // cloud index; fetch the reference's choice and, if a z changed, re-evaluate that sample's
      // speculative edge and redo resolve + commit (sample positions and classes do not depend on z)
      std::vector<MapTieRec> recs((size_t)std::min(n_mt, MAPTIE_CAP));
      HIPCHK(e, hipMemcpy(recs.data(), B.mt_rec + parity * MAPTIE_CAP, recs.size() * sizeof(MapTieRec),
                          hipMemcpyDeviceToHost));
      if (n_mt > MAPTIE_CAP) e->stats.map_nn_unresolved += (uint64_t)(n_mt - MAPTIE_CAP);
      bool z_changed = false;
      for (const MapTieRec &r : recs) {
        float z_exact = 0, z_dev = 0;
        bool found = false;
        if ((st = map_nn_exact(e, m, r.qx, r.qy, &z_exact, &found)) != TRG_OK) return st;
        SlotRec sr;
        HIPCHK(e, hipMemcpy(&sr, B.slot_rec + r.slot, sizeof(SlotRec), hipMemcpyDeviceToHost));
        z_dev = sr.z;
        if (!found || z_exact == z_dev) continue;
        sr.z = z_exact;
        z_changed = true;
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
          sr.status = raw;
          sr.dist = dd;
          sr.cov[0] = wgt;  // the weight itself (already clamped): k_node_weights takes it as given
          sr.w_given = 1;
        }
        HIPCHK(e, hipMemcpy(B.slot_rec + r.slot, &sr, sizeof(SlotRec), hipMemcpyHostToDevice));
      }
      if (z_changed) {
        if ((st = undo_level()) != TRG_OK) return st;  // also clears the tie / gate counters
        if (n_unc > 0) {
          // the level's uncertain gates are decided before the second half runs again (the entry of
          // a re-evaluated slot is stale but harmless: its status no longer carries the flag)
          if ((st = resolve_uncertain(std::min(n_unc, BFS_UNC_CAP), slot_status(), sizeof(SlotRec), parity,
                                      unc_ctr)) != TRG_OK)
            return st;
          n_unc = 0;
        }
        if ((st = rerun_second_half()) != TRG_OK) return st;
        if (err & ~BFS_ERR_SOFT) return fallback(err_text(err));
      } else {
        const int zero = 0;
        HIPCHK(e, hipMemcpy(B.ctrs + BFS_CTR_NMAPTIE + parity, &zero, sizeof(int), hipMemcpyHostToDevice));
      }
    }
    if (n_unc > 0) {
      if ((st = resolve_uncertain(n_unc, slot_status(), sizeof(SlotRec), parity, unc_ctr)) != TRG_OK) return st;
      if (unc_changed) {
        // a speculative edge the level relied on is in fact gated: redo the second half
        if ((st = undo_level()) != TRG_OK) return st;
        undone = true;
        if (!(err & BFS_ERR_SOFT)) {
          if ((st = rerun_second_half()) != TRG_OK) return st;
          if (err & ~BFS_ERR_SOFT) return fallback(err_text(err));
          undone = false;
        }
      }
    }
    if ((err & BFS_ERR_SOFT) == BFS_ERR_TIE_CLS && !undone) {
      // Only ties among nodes that existed before the level: nothing else of the level is in doubt.
      // The reference's winner (kd-tree visiting order, host_index.h) replaces the device's pick in the
      // slot records and resolve + commit run again -- no host replay of the whole level.
      std::vector<SlotRec> srec(level_slots);
      HIPCHK(e, hipMemcpy(srec.data(), B.slot_rec, level_slots * sizeof(SlotRec), hipMemcpyDeviceToHost));
      std::vector<float> all_x, all_y;
      std::vector<int> tied;
      for (size_t sl = 0; sl < level_slots; ++sl) {
        SlotRec &sr = srec[sl];
        if (!(sr.cls & SLOT_TIE) || (sr.cls & SLOT_CLS_MASK) == 0 || sr.nn0 < 0) continue;
        if (all_x.empty()) {
          all_x.resize(V0);
          all_y.resize(V0);
          HIPCHK(e, hipMemcpy(all_x.data(), B.nx, (size_t)V0 * sizeof(float), hipMemcpyDeviceToHost));
          HIPCHK(e, hipMemcpy(all_y.data(), B.ny, (size_t)V0 * sizeof(float), hipMemcpyDeviceToHost));
        }
        tied.clear();
        for (int i = 0; i < V0; ++i) {
          float acc = 0;  // the reference's accumulation order (kdtree.c:339-342)
          acc += (all_x[i] - sr.x) * (all_x[i] - sr.x);
          acc += (all_y[i] - sr.y) * (all_y[i] - sr.y);
          if (acc == sr.d0sq) tied.push_back(i);
        }
        e->stats.nn_ties++;
        if (tied.size() > 1) sr.nn0 = kd_tie_winner(all_x.data(), all_y.data(), V0, sr.x, sr.y, tied);
        sr.cls &= ~SLOT_TIE;
        HIPCHK(e, hipMemcpy(B.slot_rec + sl, &sr, sizeof(SlotRec), hipMemcpyHostToDevice));
      }
      err_from_sample = 0;  // settled
      if ((st = undo_level()) != TRG_OK) return st;
      if ((st = rerun_second_half()) != TRG_OK) return st;
      if (err & ~BFS_ERR_SOFT) return fallback(err_text(err));
      e->stats.bfs_tie_fixups++;
    }
    if ((err & BFS_ERR_SOFT) == BFS_ERR_TIE && !undone && e->tie_inplace &&
        !(e->debug_tie_every > 0 && levels > 0 && levels % e->debug_tie_every == 0)) {
      // A tie between two nearest-node candidates touches only the slots that met it: whichever of
      // the tied nodes wins, the distance -- hence "creates a node or not" -- is the same unless their
      // states differ, and nobody waits for a sample that does not create.  The committed level
      // stands; the host decides the listed slots as the reference would (kd-tree visiting order,
      // host_index.h) and rewrites their call records.  (States differ and one outcome creates: the
      // level is replayed below.)
      bool settled = false;
      if ((st = settle_ties_in_place(&settled)) != TRG_OK) return st;
      if (settled) {
        err &= ~BFS_ERR_TIE;
        e->stats.bfs_tie_fixups++;
      }
    }
    bool replayed = false;
    if (err & BFS_ERR_SOFT) {
      // exact fp32 distance tie (or a resolve whose bounded wait ran out): this one level is replayed
      // on the host, then the device goes on
      if (CS > 1) return fallback("a level of a build with expandGraph's step 3 needs the host replay");
      if (!undone && (st = undo_level()) != TRG_OK) return st;
      int vnew = V0;
      if ((st = replay_level_on_host(e, bb, mcur, V0, call_base, &vnew, &mnext)) != TRG_OK) return st;
      v_after = vnew;
      replayed = true;
    }
    if (any_rare) {
      e->stats.ms_rare_events += ms_since(t_rare);
      if (getenv("TRG_TRACE_LEVELS"))
        fprintf(stderr, "[trg bfs] level %d: rare events (map ties %d, uncertain gates %d, err %d%s) took %.3f ms\n",
                levels, n_mt, n_unc, err, replayed ? ", host replay" : "", ms_since(t_rare));
    }
    // the level is final: its statistics (a replayed level counted draws / samples / nodes itself)
    if (!replayed) {
      bb.host_stats[2] += lvl_stats[0];
      bb.host_stats[3] += lvl_stats[1];
    }
    // the next level's expansion: redo it after a redone commit or when its hash was sized too
    // small, top it up past the launch bound
    if (reexpand || (size_t)mnext > next_cap_nodes) {
      if (!reexpand) HIPCHK(e, hipStreamSynchronize(s));
      int ctr_fix[3] = {0, 0, 0};
      HIPCHK(e, hipMemcpy(B.ctrs + BFS_CTR_NMAPTIE, ctr_fix, 2 * sizeof(int), hipMemcpyHostToDevice));
      HIPCHK(e, hipMemcpy(B.ctrs + ((parity ^ 1) ? BFS_CTR_NUNC1 : BFS_CTR_NUNC), ctr_fix, sizeof(int),
                          hipMemcpyHostToDevice));
      have_expand = false;  // issued at the top of the next iteration with a fresh tag
      next_events_valid = false;
    } else {
      if (mnext > spec_bound)
        launch_level_expand(m.view, qp, e->d_cos, e->d_sin, e->sampler.table_bits, e->sampler.seed,
                            e->epoch, Bn, mnext, nullptr, spec_bound, parity ^ 1, next_tag, 0, e->d_ctr, s);
      have_expand = true;
      cur_tag = next_tag;
      cur_ht = next_ht;
    }
    std::swap(ev0, evn0);
    std::swap(ev1, evn1);
    expand_events_valid = next_events_valid;
    v_now = v_after;
    std::swap(B.front_cur, B.front_next);
    std::swap(B.fxy_cur, B.fxy_next);
    std::swap(bb.cap_front0, bb.cap_front1);
    call_base += (long long)level_slots * CS;
    mcur = mnext;
    levels++;
    // the calls of the levels that are final by now: into the deferred pipeline, a batch at a time
    if (overlap && call_base - def_lo >= DEF_BATCH_MIN && call_base < 0x7FFFFFF0LL)
      if ((st = launch_deferred(call_base, true)) != TRG_OK) return st;
  }
  HIPCHK(e, hipStreamSynchronize(s));
  e->stats.ms_bfs_loop = ms_since(t_loop);
  // the expansion holds the sampling AND the speculative parent edges of a level: its time is
  // reported as the "sample kernel", its algorithmic bytes are bytes_sample + bytes_spec
  if (n_expand_timed)
    e->stats.ms_sample_kernel += ms_expand_timed * (double)n_expand_all / (double)n_expand_timed;
  e->stats.launches_sample_kernel += n_expand_all;
  auto t_def = Clock::now();
  const int V = v_now;
  const long long ncalls = call_base;
  e->stats.sync_batches += (uint64_t)levels;

  // ---- rest of the deferred wireEdge evaluations ------------------------------------------------------
  if (ncalls >= 0x7FFFFFF0LL) return fallback("call log too long");
  if ((size_t)ncalls > calls_bound) return fallback("more wireEdge calls than the node capacity bound allows");
  if (!overlap) {
    HIPCHK(e, hipMemsetAsync(F.ht_key, 0xFF, (size_t)fht * sizeof(unsigned long long), s));
    HIPCHK(e, hipMemsetAsync(F.ht_seq, 0x7F, (size_t)fht * sizeof(int), s));
  }
  launch_node_weights(B, V, s);  // weights of the edges to the nodes the BFS created (the commit kept
                                 // their covariances); touches only the calls that created a node
  if (e->step3) {
    // step 3 (trg.cpp:429-444): the node tree rebuilt on the device, every valid node's neighbour calls into
    // the entries behind its creating call; the deferred pipeline below takes them like all other calls
    ENSB(bb.s3_scratch, (6 * (size_t)V + 8) * sizeof(int));
    if (launch_step3_calls(B, V, e->prm.expand_dist, (int *)bb.s3_scratch.p, bb.h_ctrs + 40, s) != 0)
      return e->fail(TRG_ERR_DEVICE, "step-3 call generation failed");
    HIPCHK(e, hipGetLastError());
  }
  if (overlap) {  // what ran beside the loop must be complete before the main stream goes on with it
    HIPCHK(e, hipEventRecord(ev_order, e->s_edge));
    HIPCHK(e, hipStreamWaitEvent(s, ev_order, 0));
  }
  if ((st = launch_deferred(ncalls, false)) != TRG_OK) return st;  // round 1 of the calls not yet handed over
  // while the GPU evaluates: the reference's graph.nodes[node_id] = node for ids 0..V-1 in creation
  // order (trg.cpp:248); cleanGraph iterates this container below
  e->nodes_sim.clear();  // resetGraph("global") -> nodes.clear(): buckets and policy persist
  e->nodes_sim.fill((size_t)V);
  std::vector<int> map_order;
  e->nodes_sim.iteration_order(map_order);
  // ... and goes to the device on the (idle) second stream, for the renumbering kernels of cleanGraph
  ENS(bb.d_map_order, cap_maporder, (size_t)V + 1);
  if (V > 0)
    HIPCHK(e, hipMemcpyAsync(bb.d_map_order, map_order.data(), (size_t)V * sizeof(int), hipMemcpyHostToDevice,
                             e->s_edge));
  HIPCHK(e, hipEventRecord(ev_order, e->s_edge));
  HIPCHK(e, hipStreamSynchronize(s_def));
  if (s_def != s) HIPCHK(e, hipStreamSynchronize(s));  // (the evaluations after the loop run in the main stream)
  double ms_edges = 0;
  for (auto &ev : def_events) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) ms_edges += ms;
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  if (!def_events.empty()) ms_edges *= (double)n_eval_batches / (double)def_events.size();
  def_events.clear();
  // round 2: every remaining call of the (few) pairs whose first call failed or was left to the host
  uint64_t round2_evals = 0;
  {
    int *d_n2 = (int *)bb.def_counts.p;
    int *h_n2 = bb.h_ctrs + 34;  // pinned
    HIPCHK(e, hipMemsetAsync(d_n2, 0, sizeof(int), s));
    launch_calls_select2_append(F, B, ncalls, bb.sel_list, d_n2, d_def_total, s);
    HIPCHK(e, hipMemcpyAsync(h_n2, d_n2, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    const int nsel = *h_n2;
    // (a batch of evaluations shares the edge scratch: at most CALL_EVAL_BATCH at a time)
    for (long long q0 = 0; q0 < nsel; q0 += CALL_EVAL_BATCH) {
      const int nq = (int)std::min<long long>(CALL_EVAL_BATCH, nsel - q0);
      HIPCHK(e, hipEventRecord(ev0, s));
      launch_calls_eval(m.view, qp, B, bb.sel_list + q0, nq, nullptr, e->d_ctr, s);
      e->stats.launches_edge_kernel++;
      HIPCHK(e, hipEventRecord(ev1, s));
      HIPCHK(e, hipEventSynchronize(ev1));
      float ms = 0;
      if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) ms_edges += ms;
      round2_evals += (uint64_t)nq;
    }
  }
  e->stats.ms_edge_kernel += ms_edges;
  if ((st = read_ctrs()) != TRG_OK) return st;
  if (bb.h_ctrs[BFS_CTR_ERR]) return fallback(err_text(bb.h_ctrs[BFS_CTR_ERR]));
  if (bb.h_ctrs[BFS_CTR_NUNC2] > 0) {
    if ((st = resolve_uncertain(bb.h_ctrs[BFS_CTR_NUNC2], B.call_status, sizeof(int), 2, BFS_CTR_NUNC2)) != TRG_OK)
      return st;
  }
  (void)round2_evals;

  e->stats.ms_deferred = ms_since(t_def);
  // ---- dedupe + CSR in creation order --------------------------------------------------------------
  auto t_fin = Clock::now();
  const bool trace_fin = getenv("TRG_TIMING") != nullptr;
  auto lap = [&](const char *what) {
    if (!trace_fin) return;
    (void)hipStreamSynchronize(s);
    fprintf(stderr, "[trg finalize] %-28s %8.3f ms\n", what, ms_since(t_fin));
  };
  auto mark = [&](const char *what) {  // host time only: the stream keeps running
    if (trace_fin) fprintf(stderr, "[trg finalize]   (host) %-20s %8.3f ms\n", what, ms_since(t_fin));
  };
  ENS(F.deg, cap_fdeg, (size_t)V + 1);
  ENS(F.fill, cap_ffill, (size_t)V + 1);
  ENS(F.rowptr, cap_frow, (size_t)V + 2);
  // the edge count is not known to the host before the scatter runs: the arrays are sized by the
  // bound (every call wires at most one pair, two directed entries)
  const size_t e_bound = 2 * (size_t)ncalls;
  ENS(F.col, cap_fcol, e_bound + 1);
  ENS(F.seq, cap_fseqe, e_bound + 1);
  ENS(F.w, cap_fw, e_bound + 1);
  ENS(F.dist, cap_fdist, e_bound + 1);
  ENS(bb.d_new2old, cap_n2o, (size_t)V + 1);
  ENS(bb.d_old2new, cap_o2n, (size_t)V + 1);
  ENS(bb.d_deg_new, cap_degn, (size_t)V + 1);
  ENS(bb.d_rowptr_new, cap_rown, (size_t)V + 2);
  ENS(bb.d_keep_flag, cap_keepf, (size_t)V + 1);
  ENS(bb.d_keep_pos, cap_keepp, (size_t)V + 2);
  ENS(bb.d_col2, cap_col2, e_bound + 1);
  ENS(bb.d_w2, cap_w2, e_bound + 1);
  ENS(bb.d_dist2, cap_dist2, e_bound + 1);
  ENS(bb.d_xyz2, cap_xyz2, 3 * (size_t)V + 3);
  ENS(bb.d_state2, cap_state2, (size_t)V + 1);
  HIPCHK(e, hipMemsetAsync(F.deg, 0, ((size_t)V + 1) * sizeof(int), s));
  HIPCHK(e, hipMemsetAsync(F.fill, 0, ((size_t)V + 1) * sizeof(int), s));
  launch_fin_insert_count(F, B, ncalls, s);
  launch_exclusive_scan(F.deg, F.rowptr, V, bb.scan_tmp, s);
  launch_fin_scatter(F, B, ncalls, s);
  lap("insert+count+scan+scatter");

  if (e->keep_preclean) {
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
  }

  // ---- cleanGraph (trg.cpp:491-535): renumbering in the reference container's iteration order ----
  // (the order went to the device while the deferred evaluations ran)
  HIPCHK(e, hipStreamWaitEvent(s, ev_order, 0));
  launch_fin_clean(F, B, bb.d_map_order, V, bb.d_keep_flag, bb.d_keep_pos, bb.d_new2old, bb.d_old2new,
                   bb.d_deg_new, bb.d_rowptr_new, bb.scan_tmp, bb.d_col2, bb.d_w2, bb.d_dist2, bb.d_xyz2,
                   bb.d_state2, s);
  int *h_tot = bb.h_ctrs + 32;  // pinned: surviving nodes, edges
  HIPCHK(e, hipMemcpyAsync(h_tot, bb.d_keep_pos + V, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipMemcpyAsync(h_tot + 1, F.rowptr + V, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
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
    HIPCHK(e, hipMemcpyAsync(g.xyz.data(), bb.d_xyz2, 3 * (size_t)Vn * sizeof(float),
                             hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(g.state.data(), bb.d_state2, (size_t)Vn * sizeof(int),
                             hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(g.cid.data(), bb.d_new2old, (size_t)Vn * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipEventRecord(ev_nodes, s));
    HIPCHK(e, hipMemcpyAsync(g.rowptr.data(), bb.d_rowptr_new, ((size_t)Vn + 1) * sizeof(int),
                             hipMemcpyDeviceToHost, s));
    if (En) {
      HIPCHK(e, hipMemcpyAsync(g.col.data(), bb.d_col2, (size_t)En * sizeof(int), hipMemcpyDeviceToHost, s));
      HIPCHK(e, hipMemcpyAsync(g.w.data(), bb.d_w2, (size_t)En * sizeof(float), hipMemcpyDeviceToHost, s));
      HIPCHK(e, hipMemcpyAsync(g.dist.data(), bb.d_dist2, (size_t)En * sizeof(float),
                               hipMemcpyDeviceToHost, s));
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
    HIPCHK(e, hipEventSynchronize(ev_nodes));
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
    if ((st = read_ctrs()) != TRG_OK) return st;
    if (bb.h_ctrs[BFS_CTR_ERR]) return fallback(err_text(bb.h_ctrs[BFS_CTR_ERR]));
    if (g.rowptr[Vn] != En) return e->fail(TRG_ERR_DEVICE, "cleanGraph edge count mismatch");
  } else {
    MapOrderSim new_nodes;
    e->nodes_sim.assign_from(new_nodes);
    if ((st = read_ctrs()) != TRG_OK) return st;
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
  e->dev_csr_valid = Vn > 0;  // d_xyz2 / d_rowptr_new / d_col2 / d_w2 / d_dist2 hold the cleaned graph
  e->real_map_stale = true;  // the real std::unordered_map is rebuilt only if a host path needs it
  e->kd_order_dirty = true;  // node-tree refill order (trg.cpp:528-530) derived on demand
  e->kd_valid = false;
  e->graph_version++;
  e->stitched_on_device = false;  // (the stitched rows belonged to the previous graph)
  e->stitched_edges = 0;
  e->csr_stitched.clear();
  e->pool_valid = false;      // the host edge pool / node grid are rebuilt from the CSR on demand
  e->host_grid_valid = false;

  // ---- statistics ------------------------------------------------------------------------------------
  unsigned long long s64[16] = {0};
  launch_bfs_stats(B, V, B.stats64 + 8, s);  // draws, samples, disc hits, speculative-edge hits, candidates, parent-edge hits
  HIPCHK(e, hipStreamSynchronize(s));  // (s does not synchronise with the plain copy below)
  HIPCHK(e, hipMemcpy(s64, B.stats64, sizeof(s64), hipMemcpyDeviceToHost));
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
            s64[8], s64[9], d, a, zero);
  }
  bb.host_stats[0] = s64[8];
  bb.host_stats[1] = s64[9];
  bb.host_stats[5] = s64[10];
  bb.host_stats[6] = s64[11];
  bb.host_stats[4] = s64[12];
  bb.host_stats[7] = s64[13];
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
    HIPCHK(e, hipMemcpy(ph.data(), B.stats64 + 16, ph.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
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
  e->stats.trials = bb.host_stats[0];
  e->stats.samples = bb.host_stats[1];
  e->stats.created_nodes = bb.host_stats[2] + 1;  // + root
  e->stats.invalid_nodes = bb.host_stats[3];
  e->stats.edge_calls = bb.host_stats[1];
  e->stats.edge_evals_gpu = bb.host_stats[4] + s64[5];  // speculative parent edges + deferred
  e->lv_hits_sample = bb.host_stats[5];
  e->lv_hits_spec = bb.host_stats[6];
  e->stats.bytes_spec_created = 12ull * bb.host_stats[7];
  e->stats.ms_finalize_host = ms_since(t_fin);
  e->stats.bfs_levels = (uint64_t)levels;
  e->stats.bfs_max_spin = s64[6];
  e->stats.bfs_multipass_rows = s64[7];
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  (void)hipEventDestroy(evn0);
  (void)hipEventDestroy(evn1);
  (void)hipEventDestroy(ev_order);
  (void)hipEventDestroy(ev_nodes);
#undef ENS
  return TRG_OK;
}

}  // namespace
