// trg_engine_field_tiled.inc -- host side of the cost field across tiles (included by trg_engine.cpp after the
// exchange; DESIGN.md section 7, "Cost fields across tiles"; kernels: trg_field_tiled.inc).  A collective call: every
// rank of the engine's communicator relaxes the fields over its own rows of the stitched graph plus mirrors
// ("ghosts") of the other ends of its cross edges, and the ranks trade the keys of their border nodes through
// exchange_allgatherv until an exchange carries no news from anybody.  The least fp32 fold over all walks is one
// least fixed point that every relaxation order reaches (DESIGN.md section 2), and this is one more order; the two
// passes of the single-engine solve (all edges, then tight edges only) are kept, each with its own exchange loop.

namespace {

// rounds enqueued between two looks at the "work left" word (fewer than a single-engine solve's: a rank is
// re-started once per exchange, mostly for a handful of rounds)
constexpr int TILED_BATCH = 8;

struct TiledFieldBufs {
  // the solve graph, built once per stitch: stamped with the graph version, the stitch and the cost model
  uint64_t version = 0, serial = 0;
  uint32_t sf_bits = 0;
  FieldTiled T{};
  int E2 = 0;              // its edges
  double mean_cost = 0.0;  // ... and the mean of their costs (the bucket width)
  bool bad_cost = false;
  DevArr up_rowptr, up_col, up_w, up_dist;  // the stitched rows, uploaded when an export had taken them off the device
  DevArr ghost_flag, ghost_off, border_flag, border_off, ghost_deg, ghost_row, ghost_fill, scan_tmp;
  DevArr gid_of, state, border, rowptr, col, w, dist, ec, stats;
  // work arrays, per item (m x (V + G)), and per border item (m x B)
  DevArr key, q[2], far[2], stamp_near, stamp_far, parent, tight, ctrl;
  DevArr published, rec, n_rec, cost, hops, parent_out;
  Pinned<FieldState> h_state;
  Pinned<FieldEdgeStats> h_stats;
  Pinned<int> h_n;  // [0] ghosts or records, [1] border rows
  Event t0, t1;
};

// One solve on its way: the request, the kernels' view, and what ends up in `info`.
struct TiledRun {
  int32_t m;
  const int32_t *source_gids;
  float *cost;
  int32_t *hops, *parent;
  TrgTiledFieldInfo *info;
  FieldDev F{};
  FieldSources local{};  // per field: the source as a local id where it is this rank's node, else -1
  int round = 0;         // of the current pass
  int rounds = 0, exchanges = 0;
  long long records = 0;
  double ms_device = 0.0;
};

TrgStatus tiled_grow(TrgEngine *e, DevArr &a, size_t bytes) {
  if (ensure_bytes(e, a, bytes + 16) == TRG_OK) return TRG_OK;
  (void)hipGetLastError();
  return e->fail(TRG_ERR_CAPACITY, "tiled cost field: no device memory for " + std::to_string(bytes) + " bytes (" + e->err + ")");
}

// the device time between the two events, once the stream has been waited for
TrgStatus tiled_lap(TrgEngine *e, TiledRun &run) {
  TiledFieldBufs &tb = *e->tiled;
  float ms = 0.0f;
  HIPCHK(e, hipEventElapsedTime(&ms, tb.t0, tb.t1));
  run.ms_device += ms;
  return TRG_OK;
}

// The solve graph of this rank for the current stitch (trg_field_tiled.inc), its edge costs included; built when the
// graph, the stitch or the safety factor moved since the last one.  The stitched rows are read where they are: in
// HBM while stitch_assemble's arrays are current, else from the host rows an export fetched.
TrgStatus tiled_graph(TrgEngine *e, const ExchangeState &x) {
  TiledFieldBufs &tb = *e->tiled;
  hipStream_t s = e->s_main;
  const Csr &rows = e->csr_stitched;
  const int V = (int)rows.state.size();
  const bool on_device = e->current(TrgEngine::VIEW_STITCH_DEV);
  if (rows.rowptr.empty() || e->stitch_node_off.empty() || (V > 0 && !on_device && rows.rowptr.size() != (size_t)V + 1))
    return e->fail(TRG_ERR_INVALID_ARG, "tiled cost field: no current stitched rows (stitch after the tile's graph last changed)");
  const std::vector<int32_t> &off = e->stitch_node_off;
  const int R = (int)off.size() - 1, tile = e->stitch_tile;
  if (R != x.nranks || tile != x.rank)
    return e->fail(TRG_ERR_INVALID_ARG, "tiled cost field: the stitch's tile is not this rank of the communicator");
  if (off[tile + 1] - off[tile] != V)
    return e->fail(TRG_ERR_INVALID_ARG, "tiled cost field: the stitch's node offsets do not match its rows");
  const uint32_t sf_bits = float_bits(e->prm.safety_factor);
  if (tb.version == e->graph_version && tb.serial == e->stitch_serial && tb.sf_bits == sf_bits) return TRG_OK;
  tb.version = 0;  // (until the build is through)
  FieldTiled &T = tb.T;
  T = FieldTiled{};
  T.V = V;
  T.lo = off[tile];
  T.Vg = off[R];
  tb.E2 = 0;
  tb.mean_cost = 0.0;
  tb.bad_cost = false;
  if (V > 0) {
    TrgStatus st;
    const int En = on_device ? e->stitched_edges : (int)rows.col.size();
    const int *rowptr, *col;
    const float *w, *dist;
    if (on_device) {
      const StitchBufs &sb = *e->stitch;
      rowptr = sb.rowptr_new.as<int>();
      col = sb.col_new.as<int>();
      w = sb.w_new.as<float>();
      dist = sb.dist_new.as<float>();
    } else {
      const size_t eb = (size_t)En * 4;
      if ((st = tiled_grow(e, tb.up_rowptr, ((size_t)V + 1) * 4)) != TRG_OK) return st;
      for (DevArr *a : {&tb.up_col, &tb.up_w, &tb.up_dist})
        if ((st = tiled_grow(e, *a, eb)) != TRG_OK) return st;
      HIPCHK(e, hipMemcpyAsync(tb.up_rowptr.p, rows.rowptr.data(), ((size_t)V + 1) * 4, hipMemcpyHostToDevice, s));
      if (En) {
        HIPCHK(e, hipMemcpyAsync(tb.up_col.p, rows.col.data(), eb, hipMemcpyHostToDevice, s));
        HIPCHK(e, hipMemcpyAsync(tb.up_w.p, rows.w.data(), eb, hipMemcpyHostToDevice, s));
        HIPCHK(e, hipMemcpyAsync(tb.up_dist.p, rows.dist.data(), eb, hipMemcpyHostToDevice, s));
      }
      rowptr = tb.up_rowptr.as<int>();
      col = tb.up_col.as<int>();
      w = tb.up_w.as<float>();
      dist = tb.up_dist.as<float>();
    }
    DevGraph g;
    if ((st = ensure_dev_graph(e, DEV_NODES, &g)) != TRG_OK) return st;
    if (g.V != V || !g.state) return e->fail(TRG_ERR_INVALID_ARG, "tiled cost field: the stitched rows are not of this tile's graph");
    // ghosts and border rows: flags, scans, counts
    const size_t nVg = (size_t)T.Vg + 2, nV = (size_t)V + 2;
    if ((st = tiled_grow(e, tb.ghost_flag, nVg * 4)) != TRG_OK || (st = tiled_grow(e, tb.ghost_off, nVg * 4)) != TRG_OK ||
        (st = tiled_grow(e, tb.border_flag, nV * 4)) != TRG_OK || (st = tiled_grow(e, tb.border_off, nV * 4)) != TRG_OK ||
        (st = tiled_grow(e, tb.scan_tmp, (std::max(nVg, nV) / 2048 + 16) * 4)) != TRG_OK)
      return st;
    launch_tiled_mark(rowptr, col, V, T.lo, T.Vg, tb.ghost_flag.as<int>(), tb.border_flag.as<int>(), s);
    launch_exclusive_scan(tb.ghost_flag.as<int>(), tb.ghost_off.as<int>(), T.Vg, tb.scan_tmp.as<int>(), s);
    launch_exclusive_scan(tb.border_flag.as<int>(), tb.border_off.as<int>(), V, tb.scan_tmp.as<int>(), s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(&tb.h_n[0], tb.ghost_off.as<int>() + T.Vg, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(&tb.h_n[1], tb.border_off.as<int>() + V, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    T.G = tb.h_n[0];
    T.B = tb.h_n[1];
    if (T.G < 0 || T.G > T.Vg || T.B < 0 || T.B > V) return e->fail(TRG_ERR_DEVICE, "tiled cost field: bad ghost or border count");
    if ((long long)V + T.G + 8 > INT_MAX) return e->fail(TRG_ERR_CAPACITY, "tiled cost field: too many nodes and ghosts");
    const size_t n = (size_t)V + T.G, nG = (size_t)T.G + 2;
    if ((st = tiled_grow(e, tb.gid_of, (n + 1) * 4)) != TRG_OK || (st = tiled_grow(e, tb.state, (n + 1) * 4)) != TRG_OK ||
        (st = tiled_grow(e, tb.border, ((size_t)T.B + 1) * 4)) != TRG_OK || (st = tiled_grow(e, tb.ghost_deg, nG * 4)) != TRG_OK ||
        (st = tiled_grow(e, tb.ghost_row, nG * 4)) != TRG_OK || (st = tiled_grow(e, tb.ghost_fill, nG * 4)) != TRG_OK ||
        (st = tiled_grow(e, tb.scan_tmp, (nG / 2048 + 16) * 4)) != TRG_OK)
      return st;
    T.ghost_flag = tb.ghost_flag.as<int>();
    T.ghost_off = tb.ghost_off.as<int>();
    T.gid_of = tb.gid_of.as<int>();
    T.state = tb.state.as<int>();
    T.border = tb.border.as<int>();
    launch_tiled_tables(T, g.state, tb.border_flag.as<int>(), tb.border_off.as<int>(), rowptr, col, tb.ghost_deg.as<int>(), s);
    HIPCHK(e, hipMemsetAsync(tb.ghost_row.p, 0, nG * 4, s));  // (a tile without cross edges: nothing to scan)
    if (T.G > 0) launch_exclusive_scan(tb.ghost_deg.as<int>(), tb.ghost_row.as<int>(), T.G, tb.scan_tmp.as<int>(), s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(&tb.h_n[0], tb.ghost_row.as<int>() + T.G, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    const int X = tb.h_n[0];  // cross edges of this tile's rows
    if (X < 0 || X > En) return e->fail(TRG_ERR_DEVICE, "tiled cost field: bad cross-edge count");
    if ((long long)En + X + 8 > INT_MAX) return e->fail(TRG_ERR_CAPACITY, "tiled cost field: too many edges");
    tb.E2 = En + X;
    const size_t e2 = (size_t)tb.E2 + 4;
    if ((st = tiled_grow(e, tb.rowptr, (n + 2) * 4)) != TRG_OK) return st;
    for (DevArr *a : {&tb.col, &tb.w, &tb.dist, &tb.ec})
      if ((st = tiled_grow(e, *a, e2 * 4)) != TRG_OK) return st;
    if ((st = tiled_grow(e, tb.stats, sizeof(FieldEdgeStats))) != TRG_OK) return st;
    launch_tiled_fill(T, rowptr, col, w, dist, En, tb.E2, tb.ghost_row.as<int>(), tb.ghost_fill.as<int>(),
                      tb.rowptr.as<int>(), tb.col.as<int>(), tb.w.as<float>(), tb.dist.as<float>(), s);
    // edge costs of its own (the single-engine cache is neither read nor evicted); every edge into a ghost is skipped
    launch_field_edge_cost(tb.col.as<int>(), tb.w.as<float>(), tb.dist.as<float>(), T.state, (int)n, tb.E2,
                           e->prm.safety_factor, bits_float(FIELD_INF_BITS), tb.ec.as<float>(),
                           tb.stats.as<FieldEdgeStats>(), s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(tb.h_stats, tb.stats.p, sizeof(FieldEdgeStats), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    tb.mean_cost = tb.h_stats->count ? tb.h_stats->sum / (double)tb.h_stats->count : 0.0;
    tb.bad_cost = tb.h_stats->bad != 0;
  }
  tb.version = e->graph_version;
  tb.serial = e->stitch_serial;
  tb.sf_bits = sf_bits;
  return TRG_OK;
}

// the work arrays for m fields and the kernels' view of them
TrgStatus tiled_work_arrays(TrgEngine *e, TiledRun &run) {
  TiledFieldBufs &tb = *e->tiled;
  const FieldTiled &T = tb.T;
  if (tb.bad_cost) return e->fail(TRG_ERR_INVALID_ARG, "tiled cost field: an edge cost is negative or not finite");
  const long long n = (long long)T.V + T.G;
  if ((long long)run.m * n + 8 > INT_MAX)
    return e->fail(TRG_ERR_CAPACITY, "tiled cost field: m x (nodes + ghosts) does not fit the solver's 32-bit item index");
  FieldDev &F = run.F;
  F.V = (int)n;
  F.m = run.m;
  F.N = (int)(run.m * n);
  const size_t nN = (size_t)F.N + 4, nB = (size_t)run.m * T.B + 4, nO = (size_t)run.m * T.V + 4;
  TrgStatus st;
  if ((st = tiled_grow(e, tb.key, nN * 8)) != TRG_OK) return st;
  for (DevArr *a : {&tb.q[0], &tb.q[1], &tb.far[0], &tb.far[1], &tb.stamp_near, &tb.stamp_far, &tb.parent, &tb.tight})
    if ((st = tiled_grow(e, *a, nN * 4)) != TRG_OK) return st;
  for (DevArr *a : {&tb.cost, &tb.hops, &tb.parent_out})
    if ((st = tiled_grow(e, *a, nO * 4)) != TRG_OK) return st;
  if ((st = tiled_grow(e, tb.published, nB * 8)) != TRG_OK || (st = tiled_grow(e, tb.rec, nB * FIELD_TILED_REC_BYTES)) != TRG_OK ||
      (st = tiled_grow(e, tb.n_rec, 16)) != TRG_OK || (st = tiled_grow(e, tb.ctrl, sizeof(FieldCtrl))) != TRG_OK)
    return st;
  F.rowptr = tb.rowptr.as<int>();
  F.col = tb.col.as<int>();
  F.ec = tb.ec.as<float>();
  F.key = tb.key.as<unsigned long long>();
  for (int i = 0; i < 2; ++i) {
    F.q[i] = tb.q[i].as<int>();
    F.far[i] = tb.far[i].as<int>();
  }
  F.stamp_near = tb.stamp_near.as<int>();
  F.stamp_far = tb.stamp_far.as<unsigned>();
  F.parent = tb.parent.as<int>();
  F.ctrl = tb.ctrl.as<FieldCtrl>();
  F.tight = nullptr;
  for (int k = 0; k < run.m; ++k) {
    const long long l = (long long)run.source_gids[k] - T.lo;
    run.local.id[k] = l >= 0 && l < T.V ? (int)l : -1;
  }
  return TRG_OK;
}

// everything of this rank that comes before the first exchange
TrgStatus tiled_prepare(TrgEngine *e, const ExchangeState &x, TiledRun &run) {
  if (!e->tiled) e->tiled.reset(new TiledFieldBufs());
  TiledFieldBufs &tb = *e->tiled;
  HIPCHK(e, tb.h_state.ensure(1));
  HIPCHK(e, tb.h_stats.ensure(1));
  HIPCHK(e, tb.h_n.ensure(2));
  HIPCHK(e, tb.t0.create());
  HIPCHK(e, tb.t1.create());
  TrgStatus st = tiled_graph(e, x);
  if (st == TRG_OK) st = tiled_work_arrays(e, run);
  return st;
}

// the rounds of this rank from where the pass stands, until it has no work left
TrgStatus tiled_rounds(TrgEngine *e, TiledRun &run) {
  TiledFieldBufs &tb = *e->tiled;
  const FieldDev &F = run.F;
  hipStream_t s = e->s_main;
  const long long cap = 4LL * F.N + 64;
  int first = -1;
  for (;;) {
    for (int i = 0; i < TILED_BATCH; ++i, ++run.round) launch_field_round(F, run.round, s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(tb.h_state, &F.ctrl->s, sizeof(FieldState), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    if (tb.h_state->overflow) return e->fail(TRG_ERR_DEVICE, "tiled cost field: queue overflow");
    if (tb.h_state->work == 0) break;
    if (first < 0) first = tb.h_state->rounds;
    if (tb.h_state->rounds - first >= cap) return e->fail(TRG_ERR_DEVICE, "tiled cost field: the rounds of a rank did not converge");
  }
  return TRG_OK;
}

// One pass: the outer loop of local rounds, publish, exchange, merge, until an exchange in which no rank has news.
// `local` is this rank's status so far; a failure of its own is announced in the next count exchange, and every
// rank leaves the loop in the same exchange.
TrgStatus tiled_pass(TrgEngine *e, ExchangeState &x, TiledRun &run, TrgStatus local, int pass) {
  TiledFieldBufs &tb = *e->tiled;
  const FieldTiled &T = tb.T;
  FieldDev &F = run.F;
  hipStream_t s = e->s_main;
  const bool work = F.N > 0;  // (a tile without nodes only takes part in the exchanges)
  const float delta = tb.mean_cost > 0.0 ? (float)(e->field_delta_scale * tb.mean_cost) : 0.0f;
  std::string local_msg = e->err;
  // a step of this rank: skipped once one has failed, whose status and message are kept for the announcement
  const auto step = [&](auto body) {
    if (local != TRG_OK) return;
    local = [&]() -> TrgStatus {
      const TrgStatus st = body();
      if (st != TRG_OK) return st;
      HIPCHK(e, hipGetLastError());
      return TRG_OK;
    }();
    if (local != TRG_OK) local_msg = e->err;
  };
  step([&]() -> TrgStatus {
    if (!work) return TRG_OK;
    F.tight = pass ? tb.tight.as<unsigned>() : nullptr;
    run.round = 0;
    HIPCHK(e, hipEventRecord(tb.t0, s));
    launch_tiled_begin(F, T, run.local, delta, tb.published.as<unsigned long long>(), s);
    return TRG_OK;
  });
  std::vector<long long> counts, words;
  const void *d_all = nullptr;
  long long gathered = 0;
  for (int exchanges = 0;; ++exchanges) {
    long long n = 0;
    step([&]() -> TrgStatus {
      if (!work) return TRG_OK;
      if (exchanges) HIPCHK(e, hipEventRecord(tb.t0, s));
      launch_tiled_merge(F, T, d_all, (int)gathered, s);
      if (const TrgStatus st = tiled_rounds(e, run); st != TRG_OK) return st;
      launch_tiled_publish(F, T, tb.published.as<unsigned long long>(), tb.rec.p, tb.n_rec.as<int>(), s);
      HIPCHK(e, hipEventRecord(tb.t1, s));
      HIPCHK(e, hipMemcpyAsync(&tb.h_n[0], tb.n_rec.p, sizeof(int), hipMemcpyDeviceToHost, s));
      HIPCHK(e, hipStreamSynchronize(s));
      n = tb.h_n[0];
      if (n < 0 || n > (long long)F.m * T.B) return e->fail(TRG_ERR_DEVICE, "tiled cost field: bad record count");
      return tiled_lap(e, run);
    });
    e->err = local_msg;
    void *all = nullptr;
    const TrgStatus st = exchange_after(e, x, local, tb.rec.p, n, T.B, FIELD_TILED_REC_BYTES, counts, words, &all);
    if (st != TRG_OK) return st;
    d_all = all;
    ++run.exchanges;
    run.records += n;
    long long border = 0;
    gathered = 0;
    for (int k = 0; k < x.nranks; ++k) {
      gathered += counts[k];
      border += words[k];
    }
    if (gathered == 0) break;  // nobody has news: every rank reads the same counts and leaves here
    // a key of a border item drops at most a few times per item in practice; the cap is the round cap's shape
    if (exchanges >= 4 * (long long)F.m * border + 64)
      return e->fail(TRG_ERR_DEVICE, "tiled cost field: the exchanges did not converge");
    if (gathered > INT_MAX) return e->fail(TRG_ERR_CAPACITY, "tiled cost field: too many records in one exchange");
  }
  if (work) {
    run.rounds += tb.h_state->rounds;
    if (pass == 0) launch_field_cost_bits(F, tb.tight.as<unsigned>(), s);
    HIPCHK(e, hipGetLastError());
  }
  return TRG_OK;
}

TrgStatus tiled_outputs(TrgEngine *e, TiledRun &run) {
  TiledFieldBufs &tb = *e->tiled;
  const FieldTiled &T = tb.T;
  hipStream_t s = e->s_main;
  if (run.F.N > 0 && T.V > 0) {
    const size_t nO = (size_t)run.m * T.V;
    HIPCHK(e, hipEventRecord(tb.t0, s));
    launch_tiled_finish(run.F, T, tb.cost.as<float>(), tb.hops.as<int>(), tb.parent_out.as<int>(), run.parent != nullptr, s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(tb.t1, s));
    if (run.cost) HIPCHK(e, hipMemcpyAsync(run.cost, tb.cost.p, nO * sizeof(float), hipMemcpyDeviceToHost, s));
    if (run.hops) HIPCHK(e, hipMemcpyAsync(run.hops, tb.hops.p, nO * sizeof(int), hipMemcpyDeviceToHost, s));
    if (run.parent) HIPCHK(e, hipMemcpyAsync(run.parent, tb.parent_out.p, nO * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    if (const TrgStatus st = tiled_lap(e, run); st != TRG_OK) return st;
  }
  return TRG_OK;
}

TrgStatus tiled_cost_field(TrgEngine *e, int32_t m, const int32_t *source_gids, float *cost, int32_t *hops,
                           int32_t *parent, TrgTiledFieldInfo *info) {
  const Clock::time_point t_total = Clock::now();
  // what every rank judges alike is refused before any collective
  if (!e->exchange || !e->exchange->transport)
    return e->fail(TRG_ERR_INVALID_ARG, "tiled cost field: no communicator (trg_engine_comm_init)");
  if (m < 1 || m > TRG_FIELD_BATCH_MAX)
    return e->fail(TRG_ERR_INVALID_ARG, "tiled cost field: m must be in [1, " + std::to_string(TRG_FIELD_BATCH_MAX) + "]");
  if (!source_gids) return e->fail(TRG_ERR_INVALID_ARG, "tiled cost field: null source_gids");
  if (!e->stitch_node_off.empty())
    for (int k = 0; k < m; ++k)
      if (source_gids[k] < 0 || source_gids[k] >= e->stitch_node_off.back())
        return e->fail(TRG_ERR_INVALID_ARG, "tiled cost field: the source of field " + std::to_string(k) +
                                                " is outside [0, " + std::to_string(e->stitch_node_off.back()) + ")");
  ExchangeState &x = *e->exchange;
  TiledRun run{m, source_gids, cost, hops, parent, info};
  TrgStatus local = tiled_prepare(e, x, run);
  for (int pass = 0; pass < 2; ++pass) {
    const TrgStatus st = tiled_pass(e, x, run, local, pass);
    if (st != TRG_OK) return st;
    local = TRG_OK;  // (a pass that returns TRG_OK had no failure of this rank left to announce)
  }
  if (const TrgStatus st = tiled_outputs(e, run); st != TRG_OK) return st;
  const FieldTiled &T = e->tiled->T;
  info->exchanges = run.exchanges;
  info->rounds = run.rounds;
  info->ghosts = T.G;
  info->border_nodes = T.B;
  info->records_sent = run.records;
  info->ms_device = (float)run.ms_device;
  info->ms_total = (float)ms_since(t_total);
  return TRG_OK;
}

TrgStatus stitch_ids(TrgEngine *e, int32_t *first_gid, int32_t *num_nodes, int32_t *total_nodes) {
  if (e->csr_stitched.rowptr.empty() || e->stitch_node_off.empty() || e->stitch_tile < 0)
    return e->fail(TRG_ERR_INVALID_ARG, "stitch_ids: no current stitched rows");
  const std::vector<int32_t> &off = e->stitch_node_off;
  *first_gid = off[e->stitch_tile];
  *num_nodes = off[e->stitch_tile + 1] - off[e->stitch_tile];
  *total_nodes = off.back();
  return TRG_OK;
}

}  // namespace

extern "C" {

TrgStatus trg_engine_tiled_cost_field(TrgEngine *e, int32_t m, const int32_t *source_gids, float *cost, int32_t *hops,
                                      int32_t *parent, TrgTiledFieldInfo *info) {
  return entry(e, "tiled_cost_field", DEVICE, [&] {
    TrgTiledFieldInfo local{};
    TrgTiledFieldInfo *out = info ? info : &local;
    *out = TrgTiledFieldInfo{};
    return tiled_cost_field(e, m, source_gids, cost, hops, parent, out);
  });
}

TrgStatus trg_engine_stitch_ids(TrgEngine *e, int32_t *first_gid, int32_t *num_nodes, int32_t *total_nodes) {
  if (!first_gid || !num_nodes || !total_nodes) return TRG_ERR_INVALID_ARG;
  return entry(e, "stitch_ids", ENGINE, [&] { return stitch_ids(e, first_gid, num_nodes, total_nodes); });
}

}  // extern "C"
