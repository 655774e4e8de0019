// trg_engine_field_tiled.inc -- host side of the cost field and the risk field across tiles (included by trg_engine.cpp
// after the exchange; DESIGN.md section 7, "Cost fields across tiles" and "Risk fields across tiles"; kernels:
// trg_field_tiled.inc).  What follows is said of the cost objective; a risk solve is the same run on the edge risks of
// the solve graph, its keys extended by the maximum, which never rounds.  A collective call: every
// rank of the engine's communicator relaxes the fields over its own rows of the stitched graph plus mirrors
// ("ghosts") of the other ends of its cross edges, and the ranks trade the keys of their border nodes through
// exchange_allgatherv until an exchange carries no news from anybody.  The least fp32 fold over all walks is one
// least fixed point that every relaxation order reaches (DESIGN.md section 2), and this is one more order; the two
// passes of the single-engine solve (all edges, then tight edges only) are kept, each with its own exchange loop.
// A solve starts from source sets with start costs ("Source sets across tiles"), one source per field being m sets of
// one entry: the members are seeded by the ranks that own them, and for the set call a third loop of the same frame
// trades, after the two passes, the owners of the border nodes over the forest of the global parents.
// A successful solve stays in the work arrays; the routes call ("Routes across tiles") walks its routes on the devices,
// the fourth use of the frame.  Under a budget or a settle mode ("Bounded fields across tiles") pass 1 runs under
// bounds that the ranks lower between the exchanges through bound records in the same stream, and ends with a trim;
// the reached list of a retained solve is local work.
// A cost solve may name a cost model per field ("Cost models across tiles"): the edge costs of every distinct model lie
// in a slot of `ec`, cached per solve graph, the round kernels, the parent sweep and the walk take the slot table where
// the fields read more than one slot, and the retained solve answers under its models.
// The refresh ("Refresh across tiles") brings the retained solve to a new stitch: the carry before the work arrays are
// regrown, a fifth use of the frame for the ghost fill and the anchors, the passes started warm, and the solve's tail.

namespace {

// rounds enqueued between two looks at the "work left" word (fewer than a single-engine solve's: a rank is
// re-started once per exchange, mostly for a handful of rounds)
constexpr int TILED_BATCH = 8;

struct TiledFieldBufs {
  // the solve graph, built once per stitch: stamped with the graph version and the stitch
  uint64_t version = 0, serial = 0;
  FieldTiled T{};
  int E2 = 0;  // its edges
  // One value per edge of the solve graph and objective.  The risks (`er`; "Risk fields across tiles") are built by the
  // first risk solve after a stitch, stamped on their own: `mean` gives the bucket width, `bad` refuses the solve.
  struct EdgeValues {
    uint64_t version = 0, serial = 0;
    double mean = 0.0;
    bool bad = false;
  } risks;
  // The costs ("Cost models across tiles"): `ec` holds slot i at i * ec_stride, one slot per cost model met on this
  // solve graph -- the cache is of one (version, serial) above and a new solve graph empties it.  Slot 0 is the
  // engine's own model (its safety factor, no ceiling) and is never given away; the others go to the model a solve
  // needs and does not find, the least recently used first.  The single-engine cache (FieldBufs::slots) is another.
  struct CostSlot {
    uint32_t sf_bits, tau_bits;  // the model, as bits
    bool valid;                  // the costs and the three words below are computed
    double sum;                  // over admitted edges
    long long count;
    bool bad;                    // some edge cost is negative or not finite (over all edges, those above the ceiling too)
    uint64_t used;               // ec_tick of the last solve that read it
  };
  std::vector<CostSlot> slots;
  size_t ec_stride = 0;  // entries from one slot to the next
  uint64_t ec_tick = 0;
  DevArr up_rowptr, up_col, up_w, up_dist;  // the stitched rows, uploaded when an export had taken them off the device
  DevArr ghost_flag, ghost_off, border_flag, border_off, ghost_deg, ghost_row, ghost_fill, scan_tmp;
  DevArr gid_of, state, border, rowptr, col, w, dist, ec, er, stats;
  // work arrays, per item (m x (V + G)), and per border item (m x B)
  DevArr key, q[2], far[2], stamp_near, stamp_far, parent, tight, ctrl;
  DevArr published, rec, n_rec, cost, hops, parent_out;
  // this rank's entries, which the copy to `entries` reads after the call that enqueued it has gone on
  std::vector<TiledEntry> h_entries;
  DevArr entries;
  // with owners: the sets' offsets, owners per item, and the outputs at the targets
  DevArr set_ptr, owner, own_changed, owner_out, owned, targets, cost_at, hops_at, owner_at;
  Pinned<FieldState> h_state;
  Pinned<FieldEdgeStats> h_stats;
  Pinned<int> h_n;  // [0] ghosts, records or a sweep's "moved" word, [1] border rows or roots, [2] a broken walk
  Event t0, t1;
  // What the last successful solve left in the work arrays, for the routes ("Routes across tiles").  It is of the
  // graph and the stitch of the stamps above and, a cost solve, of the safety factor it ran with; any new solve clears
  // it at its start.
  struct Solved {
    bool valid = false;
    int m = 0;
    bool owners = false;   // the owner pass ran: `owner` holds m x (V + G) words
    bool parents = false;  // the parent sweep ran
    bool risk = false;     // the objective: F.ec is the edge risks, the walk and a late parent sweep take their RISK form
    uint32_t sf_bits = 0;  // (a cost solve)
    FieldDev F{};
    // a cost solve's models ("Cost models across tiles"): the pairs as solved (empty: the request named none), the slot
    // table, and whether the fields read more than one slot -- then the walk and a late parent sweep take the table,
    // else F.ec is the one slot.  No solve comes between this one and its routes, so its slots are not given away.
    std::vector<TrgFieldModel> pairs;
    FieldModels models{};
    bool many = false;
    const FieldModels *model_table() const { return many ? &models : nullptr; }
    // What a refresh needs of it ("Refresh across tiles"): the request as solved, the stitch's node offsets then (the
    // ranks' old id ranges: V_old of this tile and, with F.V, the stride its keys lie at), and whether it is one that
    // cannot be refreshed -- under bounds its removed keys bound nothing, with start costs its members are no anchors.
    std::vector<int32_t> set_ptr, set_gids, node_off;
    bool bounded = false, seeded = false;
  } solved;
  // A refresh: the carried keys (m x V), the anchored ones (m x (V + G)), the node map, the counts per field, the
  // members' new global ids and the anchors' verdicts (m x (V + G)).
  DevArr carry, key0, node_map, carried, members, rooted;
  DevArr route_field, route_target, route_off, route_gids, route_info;
  // Bounded solves ("Bounded fields across tiles"): this rank's settle targets (local ids), the words of TiledSettle --
  // `told` (FIELD_MAX_SOURCES words), then the table -- with the host copies their uploads read, and the bounds that
  // pass 1 ended with.  The reached counts per field and the list of trg_engine_tiled_field_reached.
  DevArr settle, bound_words, reached, list_counts, list_off, list_tmp, list_gids, list_value, list_hops;
  std::vector<int32_t> h_settle;
  std::vector<uint32_t> h_bound_words, h_bound;
};

// What a solve is asked for.  Both calls come as source sets in global ids: one source per field is m sets of one
// entry (set_ptr = 0 .. m) without start costs.
struct TiledRequest {
  int32_t m;
  const int32_t *set_ptr, *set_gids;
  const float *set_cost0;  // or nullptr: every entry starts at 0
  float *cost;
  int32_t *hops, *parent;
  // The set call: the owner pass runs, and what follows may be asked for.  Fixed by the entry that was called, so
  // every rank decides alike whether the owner pass, a collective, runs (tiled_solve).
  bool owners;
  // The objective: the least worst-edge risk ("Risk fields across tiles") in the place of the least cost fold.  Fixed by
  // the entry as well: the ranks' round kernels must extend alike.
  bool risk;
  const char *what;         // the error prefix of the call
  const char *null_ids;     // the refusal of a null set_ptr or set_gids
  const char *source_noun;  // of an id out of range: "<noun> k", or with nullptr "entry j of set k (id)"
  int32_t *owner = nullptr;
  const int32_t *targets = nullptr;
  int32_t n_targets = 0;
  float *cost_at = nullptr;
  int32_t *hops_at = nullptr, *owner_at = nullptr, *owned = nullptr;
  // The bounded entries ("Bounded fields across tiles"): a budget per field (nullptr: +inf each), the settle mode over
  // the settle targets -- GLOBAL ids, the same list on every rank -- and the outputs: the bound every field ended with
  // (m, the same on every rank) and how many of THIS tile's nodes lie within it (m).
  const float *budget = nullptr;
  int32_t settle = TRG_FIELD_SETTLE_NONE;
  const int32_t *settle_gids = nullptr;
  int32_t n_settle = 0;
  float *bound_out = nullptr;
  int32_t *reached_out = nullptr;
  // a cost model per field ("Cost models across tiles"; never with risk), or nullptr: the engine's for every field
  const TrgFieldModel *models = nullptr;
};

// One solve on its way: the request, the kernels' view, and what ends up in the caller's info.
struct TiledRun {
  const TiledRequest &rq;
  FieldDev F{};
  int n_entries = 0;  // the entries whose member is this rank's node (tb.entries)
  bool always = false;  // the routes, pass 1 under a settle mode: a tile without nodes still runs its step of every exchange
  // Some budget below +inf, or a settle mode: pass 1 runs under bounds.  Without either the launches, exchanges and
  // records are those of a solve that knows no bounds.
  bool bounded = false;
  FieldBounds budgets{};
  TiledSettle S{};
  // the edge costs of this solve (tiled_edge_costs): the slot table, whether the fields read more than one slot (else
  // F.ec is the one they share and no kernel takes the table), and the mean over its distinct slots
  FieldModels models{};
  bool many_models = false;
  double mean_cost = 0.0;
  const FieldModels *model_table() const { return many_models ? &models : nullptr; }
  int round = 0;      // of the current pass
  int rounds = 0, exchanges = 0, owner_exchanges = 0, roots = 0;
  long long records = 0, owner_records = 0;
  // a refresh ("Refresh across tiles"): the passes start warm, from what the anchor before them left
  bool warm = false;
  int anchor_exchanges = 0;
  long long anchor_records = 0;
  std::vector<int32_t> h_members, h_carried;  // what the first anchor brought back: every member's new gid, the counts
  double ms_device = 0.0;
};

// This rank's status through a loop of exchanges.  A step is skipped once one has failed; the failure's status and
// message are kept for the announcement in the next count exchange (exchange_after).
struct TiledLocal {
  TrgEngine *e;
  TrgStatus st;
  std::string msg;
  TiledLocal(TrgEngine *e_, TrgStatus st_) : e(e_), st(st_), msg(e_->err) {}
  template <typename Body>
  void step(Body body) {
    if (st != TRG_OK) return;
    st = [&]() -> TrgStatus {
      const TrgStatus r = body();
      if (r != TRG_OK) return r;
      HIPCHK(e, hipGetLastError());
      return TRG_OK;
    }();
    if (st != TRG_OK) msg = e->err;
  }
};

// the error prefix of what both objectives share
const char *tiled_what(bool risk) { return risk ? "tiled risk field: " : "tiled cost field: "; }

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

// The edge risks of the current solve graph ("Risk fields across tiles"), computed when the graph moved since they
// were.  Every edge into a ghost is skipped.
TrgStatus tiled_edge_risks(TrgEngine *e) {
  TiledFieldBufs &tb = *e->tiled;
  const FieldTiled &T = tb.T;
  hipStream_t s = e->s_main;
  TiledFieldBufs::EdgeValues &ev = tb.risks;
  if (ev.version == tb.version && ev.serial == tb.serial) return TRG_OK;
  ev = TiledFieldBufs::EdgeValues{};
  if (T.V > 0) {
    const int n = T.V + T.G;
    TrgStatus st;
    if ((st = tiled_grow(e, tb.er, ((size_t)tb.E2 + 4) * 4)) != TRG_OK ||
        (st = tiled_grow(e, tb.stats, sizeof(FieldEdgeStats))) != TRG_OK)
      return st;
    launch_field_edge_risk(tb.col.as<int>(), tb.w.as<float>(), T.state, n, tb.E2, tb.er.as<float>(),
                           tb.stats.as<FieldEdgeStats>(), s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(tb.h_stats, tb.stats.p, sizeof(FieldEdgeStats), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    ev.mean = tb.h_stats->count ? tb.h_stats->sum / (double)tb.h_stats->count : 0.0;
    ev.bad = tb.h_stats->bad != 0;
  }
  ev.version = tb.version;
  ev.serial = tb.serial;
  return TRG_OK;
}

// The edge costs of a cost solve on the current solve graph ("Cost models across tiles"): every field's model gets a
// slot of the cache, found or taken; only the slots that are missing are computed, one launch each on the solve
// graph's arrays -- ghosts are Invalid there, so every edge into a ghost stays skipped under every model -- and ONE host
// wait for all their stats.  The bucket width's mean is over the solve's distinct slots: without models that is the one
// slot of the engine's model.  The single-engine cache is neither read nor evicted.
TrgStatus tiled_edge_costs(TrgEngine *e, TiledRun &run) {
  TiledFieldBufs &tb = *e->tiled;
  const FieldTiled &T = tb.T;
  const TiledRequest &rq = run.rq;
  hipStream_t s = e->s_main;
  const int m = rq.m;
  const uint32_t sf0 = float_bits(e->prm.safety_factor);
  const size_t stride = ((size_t)tb.E2 + 4 + 3) & ~(size_t)3;  // (slots start 16-byte aligned, 16 bytes of slack each)
  run.models = FieldModels{};
  run.models.stride = (long long)stride;
  run.many_models = false;
  run.mean_cost = 0.0;
  if (T.V <= 0) return TRG_OK;  // (a tile without nodes has no edges: nothing reads a cost)
  if (tb.slots.empty() || tb.ec_stride != stride || tb.slots[0].sf_bits != sf0)
    tb.slots.assign(1, TiledFieldBufs::CostSlot{sf0, FIELD_INF_BITS, false, 0.0, 0, false, 0});
  tb.ec_stride = 0;  // (until this phase is through: a failure half-way leaves no cache)
  const uint64_t tick = ++tb.ec_tick;
  std::vector<int> fresh;  // the slots to compute
  for (int k = 0; k < m; ++k) {
    const uint32_t sfb = rq.models ? float_bits(rq.models[k].safety_factor) : sf0;
    const uint32_t taub = rq.models ? float_bits(rq.models[k].max_weight) : FIELD_INF_BITS;
    int slot = -1;
    for (size_t i = 0; i < tb.slots.size() && slot < 0; ++i)
      if (tb.slots[i].sf_bits == sfb && tb.slots[i].tau_bits == taub) slot = (int)i;
    if (slot < 0) {
      if ((int)tb.slots.size() < FIELD_SLOTS_MAX) {
        slot = (int)tb.slots.size();
        tb.slots.push_back({});
      } else {  // (a solve reads at most FIELD_MAX_SOURCES slots: one beside slot 0 is not this solve's)
        for (size_t i = 1; i < tb.slots.size(); ++i)
          if (tb.slots[i].used != tick && (slot < 0 || tb.slots[i].used < tb.slots[slot].used)) slot = (int)i;
      }
      if (slot < 0)
        return e->fail(TRG_ERR_CAPACITY, std::string(rq.what) + "no cache slot left for the model of field " + std::to_string(k));
      tb.slots[slot] = TiledFieldBufs::CostSlot{sfb, taub, false, 0.0, 0, false, tick};
    }
    TiledFieldBufs::CostSlot &cs = tb.slots[slot];
    if (!cs.valid && std::find(fresh.begin(), fresh.end(), slot) == fresh.end()) fresh.push_back(slot);
    cs.used = tick;
    run.models.slot[k] = slot;
  }
  if (!fresh.empty() || !tb.ec.p) {  // whole slots, contents kept
    const size_t bytes = tb.slots.size() * stride * sizeof(float) + 16;
    if (ensure_bytes(e, tb.ec, bytes, true) != TRG_OK ||
        ensure_bytes(e, tb.stats, FIELD_SLOTS_MAX * sizeof(FieldEdgeStats)) != TRG_OK) {
      (void)hipGetLastError();
      return e->fail(TRG_ERR_CAPACITY, std::string(rq.what) + "no device memory for the edge costs of " +
                                           std::to_string(tb.slots.size()) + " cost models (" + e->err + ")");
    }
  }
  if (!fresh.empty()) {
    FieldEdgeStats *d_stats = tb.stats.as<FieldEdgeStats>();
    const int n = T.V + T.G;
    for (size_t j = 0; j < fresh.size(); ++j) {
      const TiledFieldBufs::CostSlot &cs = tb.slots[fresh[j]];
      launch_field_edge_cost(tb.col.as<int>(), tb.w.as<float>(), tb.dist.as<float>(), T.state, n, tb.E2,
                             bits_float(cs.sf_bits), bits_float(cs.tau_bits), tb.ec.as<float>() + (size_t)fresh[j] * stride,
                             d_stats + j, s);
    }
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(tb.h_stats, d_stats, fresh.size() * sizeof(FieldEdgeStats), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    for (size_t j = 0; j < fresh.size(); ++j) {
      TiledFieldBufs::CostSlot &cs = tb.slots[fresh[j]];
      cs.sum = tb.h_stats[j].sum;
      cs.count = tb.h_stats[j].count;
      cs.bad = tb.h_stats[j].bad != 0;
      cs.valid = true;
    }
  }
  tb.ec_stride = stride;
  double sum = 0.0;
  long long count = 0;
  for (int k = 0; k < m; ++k) {
    const int slot = run.models.slot[k];
    const TiledFieldBufs::CostSlot &cs = tb.slots[slot];
    if (cs.bad)
      return e->fail(TRG_ERR_INVALID_ARG, rq.models ? std::string(rq.what) + "an edge cost is negative or not finite under the model of field " +
                                                          std::to_string(k)
                                                    : std::string("tiled cost field: an edge cost is negative or not finite"));
    bool seen = false;
    for (int j = 0; j < k && !seen; ++j) seen = run.models.slot[j] == slot;
    if (!seen) {
      sum += cs.sum;
      count += cs.count;
    }
    run.many_models = run.many_models || slot != run.models.slot[0];
  }
  run.mean_cost = count ? sum / (double)count : 0.0;
  return TRG_OK;
}

// The solve graph of this rank for the current stitch (trg_field_tiled.inc), built when the graph or the stitch moved
// since the last one; a new one empties the caches of its edge values.  The stitched rows are read where they
// are: in HBM while stitch_assemble's arrays are current, else from the host rows an export fetched.
TrgStatus tiled_graph(TrgEngine *e, const ExchangeState &x, bool risk) {
  TiledFieldBufs &tb = *e->tiled;
  hipStream_t s = e->s_main;
  const Csr &rows = e->csr_stitched;
  const int V = (int)rows.state.size();
  const bool on_device = e->current(TrgEngine::VIEW_STITCH_DEV);
  const std::string what = tiled_what(risk);
  if (rows.rowptr.empty() || e->stitch_node_off.empty() || (V > 0 && !on_device && rows.rowptr.size() != (size_t)V + 1))
    return e->fail(TRG_ERR_INVALID_ARG, what + "no current stitched rows (stitch after the tile's graph last changed)");
  const std::vector<int32_t> &off = e->stitch_node_off;
  const int R = (int)off.size() - 1, tile = e->stitch_tile;
  if (R != x.nranks || tile != x.rank)
    return e->fail(TRG_ERR_INVALID_ARG, what + "the stitch's tile is not this rank of the communicator");
  if (off[tile + 1] - off[tile] != V)
    return e->fail(TRG_ERR_INVALID_ARG, what + "the stitch's node offsets do not match its rows");
  if (tb.version == e->graph_version && tb.serial == e->stitch_serial) return TRG_OK;
  tb.version = 0;  // (until the build is through)
  tb.risks = TiledFieldBufs::EdgeValues{};
  tb.slots.clear();
  tb.ec_stride = 0;
  FieldTiled &T = tb.T;
  T = FieldTiled{};
  T.V = V;
  T.lo = off[tile];
  T.Vg = off[R];
  tb.E2 = 0;
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
    if (g.V != V || !g.state) return e->fail(TRG_ERR_INVALID_ARG, what + "the stitched rows are not of this tile's graph");
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
    if (T.G < 0 || T.G > T.Vg || T.B < 0 || T.B > V) return e->fail(TRG_ERR_DEVICE, what + "bad ghost or border count");
    if ((long long)V + T.G + 8 > INT_MAX) return e->fail(TRG_ERR_CAPACITY, what + "too many nodes and ghosts");
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
    if (X < 0 || X > En) return e->fail(TRG_ERR_DEVICE, what + "bad cross-edge count");
    if ((long long)En + X + 8 > INT_MAX) return e->fail(TRG_ERR_CAPACITY, what + "too many edges");
    tb.E2 = En + X;
    const size_t e2 = (size_t)tb.E2 + 4;
    if ((st = tiled_grow(e, tb.rowptr, (n + 2) * 4)) != TRG_OK) return st;
    for (DevArr *a : {&tb.col, &tb.w, &tb.dist})
      if ((st = tiled_grow(e, *a, e2 * 4)) != TRG_OK) return st;
    launch_tiled_fill(T, rowptr, col, w, dist, En, tb.E2, tb.ghost_row.as<int>(), tb.ghost_fill.as<int>(),
                      tb.rowptr.as<int>(), tb.col.as<int>(), tb.w.as<float>(), tb.dist.as<float>(), s);
    HIPCHK(e, hipGetLastError());
  }
  tb.version = e->graph_version;
  tb.serial = e->stitch_serial;
  return TRG_OK;
}

// A bounded solve's own arrays: of the settle targets this rank keeps those that are its nodes, as it does the entries;
// `told` starts at +inf bits; the table of the ALL rule starts at +inf bits for a rank that owns a settle target and at
// 0 for one that owns none, which every rank derives alike from the stitch's node offsets.
TrgStatus tiled_settle_arrays(TrgEngine *e, TiledRun &run) {
  TiledFieldBufs &tb = *e->tiled;
  const FieldTiled &T = tb.T;
  const TiledRequest &rq = run.rq;
  const ExchangeState &x = *e->exchange;
  const std::vector<int32_t> &off = e->stitch_node_off;
  hipStream_t s = e->s_main;
  const bool settles = rq.settle != TRG_FIELD_SETTLE_NONE;
  std::vector<int32_t> &mine = tb.h_settle;
  mine.clear();
  std::vector<uint32_t> &words = tb.h_bound_words;
  words.assign((size_t)FIELD_MAX_SOURCES + (size_t)rq.m * STITCH_MAX_TILES, 0u);
  std::fill(words.begin(), words.begin() + FIELD_MAX_SOURCES, FIELD_INF_BITS);
  for (int j = 0; settles && j < rq.n_settle; ++j) {
    const int32_t g = rq.settle_gids[j];
    const int owner = (int)(std::upper_bound(off.begin(), off.end(), g) - off.begin()) - 1;  // (the last of equal offsets)
    if (owner < 0 || owner >= x.nranks) continue;  // (never: tiled_check_request)
    for (int k = 0; k < rq.m; ++k) words[(size_t)FIELD_MAX_SOURCES + (size_t)k * STITCH_MAX_TILES + owner] = FIELD_INF_BITS;
    if (owner == x.rank) mine.push_back(g - T.lo);
  }
  TrgStatus st;
  if ((st = tiled_grow(e, tb.settle, (mine.size() + 1) * 4)) != TRG_OK ||
      (st = tiled_grow(e, tb.bound_words, words.size() * 4)) != TRG_OK)
    return st;
  if (!mine.empty()) HIPCHK(e, hipMemcpyAsync(tb.settle.p, mine.data(), mine.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(e, hipMemcpyAsync(tb.bound_words.p, words.data(), words.size() * 4, hipMemcpyHostToDevice, s));
  run.S = TiledSettle{rq.settle, tb.settle.as<int>(), (int)mine.size(), x.rank, x.nranks, tb.bound_words.as<unsigned>(),
                      tb.bound_words.as<unsigned>() + FIELD_MAX_SOURCES};
  return TRG_OK;
}

// the work arrays for m fields and the kernels' view of them
TrgStatus tiled_work_arrays(TrgEngine *e, TiledRun &run) {
  TiledFieldBufs &tb = *e->tiled;
  const FieldTiled &T = tb.T;
  const TiledRequest &rq = run.rq;
  if (rq.risk && tb.risks.bad) return e->fail(TRG_ERR_INVALID_ARG, "tiled risk field: an edge weight is negative or not finite");
  const long long n = (long long)T.V + T.G;
  if ((long long)rq.m * n + 8 > INT_MAX)
    return e->fail(TRG_ERR_CAPACITY, std::string(tiled_what(rq.risk)) + "m x (nodes + ghosts) does not fit the solver's 32-bit item index");
  FieldDev &F = run.F;
  F.V = (int)n;
  F.m = rq.m;
  F.N = (int)(rq.m * n);
  const size_t nN = (size_t)F.N + 4, nB = (size_t)rq.m * T.B + 4, nO = (size_t)rq.m * T.V + 4;
  TrgStatus st;
  if ((st = tiled_grow(e, tb.key, nN * 8)) != TRG_OK) return st;
  for (DevArr *a : {&tb.q[0], &tb.q[1], &tb.far[0], &tb.far[1], &tb.stamp_near, &tb.stamp_far, &tb.parent, &tb.tight})
    if ((st = tiled_grow(e, *a, nN * 4)) != TRG_OK) return st;
  for (DevArr *a : {&tb.cost, &tb.hops, &tb.parent_out})
    if ((st = tiled_grow(e, *a, nO * 4)) != TRG_OK) return st;
  const size_t n_bound_rec = run.bounded ? (size_t)rq.m : 0;  // (the bound records of one exchange)
  if ((st = tiled_grow(e, tb.published, nB * 8)) != TRG_OK ||
      (st = tiled_grow(e, tb.rec, (nB + n_bound_rec) * FIELD_TILED_REC_BYTES)) != TRG_OK ||
      (st = tiled_grow(e, tb.n_rec, 16)) != TRG_OK || (st = tiled_grow(e, tb.ctrl, sizeof(FieldCtrl))) != TRG_OK)
    return st;
  F.rowptr = tb.rowptr.as<int>();
  F.col = tb.col.as<int>();
  // (a cost solve whose fields share one slot reads that slot through F.ec, and no kernel takes the table)
  F.ec = rq.risk ? tb.er.as<float>()
                 : tb.ec.as<float>() + (run.many_models ? 0 : (size_t)run.models.slot[0] * (size_t)run.models.stride);
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
  HIPCHK(e, hipMemsetAsync(tb.n_rec.p, 0, 16, e->s_main));  // (the word that only a broken walk of the routes sets)
  // The targets are this tile's nodes; of the entries this rank seeds those whose member is its own node (work per
  // entry and per target, none per node).
  hipStream_t s = e->s_main;
  for (int j = 0; j < rq.n_targets; ++j)
    if (rq.targets[j] < 0 || rq.targets[j] >= T.V)
      return e->fail(TRG_ERR_INVALID_ARG, std::string(rq.what) + "target " + std::to_string(j) + " (" + std::to_string(rq.targets[j]) +
                                              ") is outside this tile's [0, " + std::to_string(T.V) + ")");
  std::vector<TiledEntry> &mine = tb.h_entries;
  mine.clear();
  for (int k = 0; k < rq.m; ++k)
    for (int j = rq.set_ptr[k]; j < rq.set_ptr[k + 1]; ++j) {
      const long long l = (long long)rq.set_gids[j] - T.lo;
      if (l < 0 || l >= T.V) continue;
      const float c0 = rq.set_cost0 ? rq.set_cost0[j] + 0.0f : 0.0f;
      mine.push_back(TiledEntry{k, (int)l, j, float_bits(c0)});
    }
  run.n_entries = (int)mine.size();
  if ((st = tiled_grow(e, tb.entries, (mine.size() + 1) * sizeof(TiledEntry))) != TRG_OK) return st;
  if (!mine.empty())
    HIPCHK(e, hipMemcpyAsync(tb.entries.p, mine.data(), mine.size() * sizeof(TiledEntry), hipMemcpyHostToDevice, s));
  if (run.bounded)
    if ((st = tiled_settle_arrays(e, run)) != TRG_OK) return st;
  if (!rq.owners) return TRG_OK;
  const size_t nT = (size_t)rq.m * (size_t)rq.n_targets + 4;
  if ((st = tiled_grow(e, tb.set_ptr, ((size_t)rq.m + 2) * 4)) != TRG_OK || (st = tiled_grow(e, tb.owner, nN * 4)) != TRG_OK ||
      (st = tiled_grow(e, tb.own_changed, FIELD_OWNER_SWEEPS_MAX * sizeof(int))) != TRG_OK ||
      (st = tiled_grow(e, tb.owner_out, nO * 4)) != TRG_OK ||
      (st = tiled_grow(e, tb.owned, ((size_t)rq.set_ptr[rq.m] + 4) * 4)) != TRG_OK ||
      (st = tiled_grow(e, tb.targets, ((size_t)rq.n_targets + 4) * 4)) != TRG_OK)
    return st;
  for (DevArr *a : {&tb.cost_at, &tb.hops_at, &tb.owner_at})
    if ((st = tiled_grow(e, *a, nT * 4)) != TRG_OK) return st;
  HIPCHK(e, hipMemcpyAsync(tb.set_ptr.p, rq.set_ptr, ((size_t)rq.m + 1) * 4, hipMemcpyHostToDevice, s));
  if (rq.n_targets > 0)
    HIPCHK(e, hipMemcpyAsync(tb.targets.p, rq.targets, (size_t)rq.n_targets * 4, hipMemcpyHostToDevice, s));
  HIPCHK(e, hipStreamSynchronize(s));  // (the caller's arrays; a tile without nodes waits for the stream nowhere else)
  return TRG_OK;
}

// everything of this rank that comes before the first exchange; `between` is a refresh's carry, which needs the new
// solve graph's node count and must be enqueued before the work arrays are regrown (a solve: nothing)
template <typename Between>
TrgStatus tiled_prepare(TrgEngine *e, const ExchangeState &x, TiledRun &run, Between between) {
  if (!e->tiled) e->tiled.reset(new TiledFieldBufs());
  TiledFieldBufs &tb = *e->tiled;
  HIPCHK(e, tb.h_state.ensure(1));
  HIPCHK(e, tb.h_stats.ensure(FIELD_SLOTS_MAX));
  HIPCHK(e, tb.h_n.ensure(4));
  HIPCHK(e, tb.t0.create());
  HIPCHK(e, tb.t1.create());
  TrgStatus st = tiled_graph(e, x, run.rq.risk);
  if (st == TRG_OK) st = between();
  if (st == TRG_OK) st = run.rq.risk ? tiled_edge_risks(e) : tiled_edge_costs(e, run);
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
  // Pass 1 of a bounded solve runs under bounds without the settle step of a single engine, whose rule needs one
  // global bucket order: the bounds drop between the exchanges instead ("Bounded fields across tiles").
  const FieldSettle no_settle{nullptr, 0, FIELD_SETTLE_NONE};
  const FieldSettle *under_bounds = run.bounded && !F.tight ? &no_settle : nullptr;
  for (;;) {
    for (int i = 0; i < TILED_BATCH; ++i, ++run.round) launch_field_round(F, run.round, s, under_bounds, run.model_table(), run.rq.risk);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(tb.h_state, &F.ctrl->s, sizeof(FieldState), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    if (tb.h_state->overflow) return e->fail(TRG_ERR_DEVICE, std::string(tiled_what(run.rq.risk)) + "queue overflow");
    if (tb.h_state->work == 0) break;
    if (first < 0) first = tb.h_state->rounds;
    if (tb.h_state->rounds - first >= cap) return e->fail(TRG_ERR_DEVICE, std::string(tiled_what(run.rq.risk)) + "the rounds of a rank did not converge");
  }
  return TRG_OK;
}

// The frame of every loop of exchanges, a pass's and the owner pass's.  Per exchange: `launches(exchanges, d_all,
// gathered)` enqueues this rank's work -- what it does with the records gathered in the exchange before, then its
// publish into tb.rec / tb.n_rec -- as a step of `mine`, timed from tb.t0 (recorded by the caller before the first)
// to tb.t1; a failure of this rank is announced in the count exchange; the loop ends at the first exchange in which
// no rank has news, where every rank reads the same counts and leaves.  `rec_bound` is the most records this rank may
// publish in one exchange (the room of tb.rec).  One that has exchanged cap(B) times with news (B the global border
// count from the auxiliary words; the passes and the owner pass: per item x (m x B) + slack) ends with TRG_ERR_DEVICE
// on every rank at once.  The copy of the record count takes the two words beside it along; the third is set by a walk
// of the routes that lost its way, to its route + 1.  n_exchanges and n_records count what went through.
template <typename Cap, typename Launches>
TrgStatus tiled_exchanges(TrgEngine *e, ExchangeState &x, TiledRun &run, TiledLocal &mine, const std::string &what,
                          long long rec_bound, Cap cap, int &n_exchanges, long long &n_records, Launches launches) {
  TiledFieldBufs &tb = *e->tiled;
  const FieldTiled &T = tb.T;
  hipStream_t s = e->s_main;
  const bool work = run.F.N > 0 || run.always;  // (a tile without nodes only takes part in the exchanges)
  std::vector<long long> counts, words;
  const void *d_all = nullptr;
  long long gathered = 0;
  for (int exchanges = 0;; ++exchanges) {
    long long n = 0;
    mine.step([&]() -> TrgStatus {
      if (!work) return TRG_OK;
      if (exchanges) HIPCHK(e, hipEventRecord(tb.t0, s));
      if (const TrgStatus st = launches(exchanges, d_all, (int)gathered); st != TRG_OK) return st;
      HIPCHK(e, hipEventRecord(tb.t1, s));
      HIPCHK(e, hipMemcpyAsync(&tb.h_n[0], tb.n_rec.p, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
      HIPCHK(e, hipStreamSynchronize(s));
      n = tb.h_n[0];
      if (n < 0 || n > rec_bound) return e->fail(TRG_ERR_DEVICE, what + "bad record count");
      if (tb.h_n[2] != 0)
        return e->fail(TRG_ERR_DEVICE, what + "the walk of route " + std::to_string(tb.h_n[2] - 1) +
                                           " lost its way (the retained arrays are damaged)");
      return tiled_lap(e, run);
    });
    e->err = mine.msg;
    void *all = nullptr;
    const TrgStatus st = exchange_after(e, x, mine.st, tb.rec.p, n, T.B, FIELD_TILED_REC_BYTES, counts, words, &all);
    if (st != TRG_OK) return st;
    d_all = all;
    ++n_exchanges;
    n_records += n;
    long long border = 0;
    gathered = 0;
    for (int k = 0; k < x.nranks; ++k) {
      gathered += counts[k];
      border += words[k];
    }
    if (gathered == 0) break;
    if (exchanges >= cap(border)) return e->fail(TRG_ERR_DEVICE, what + "the exchanges did not converge");
    if (gathered > INT_MAX) return e->fail(TRG_ERR_CAPACITY, what + "too many records in one exchange");
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
  const bool work = F.N > 0;
  // the bucket width from the mean edge value of the objective; all risks zero: width 0 ("Risk fields across tiles")
  const double mean = run.rq.risk ? tb.risks.mean : run.mean_cost;
  const float delta = mean > 0.0 ? (float)(e->field_delta_scale * mean) : 0.0f;
  // Pass 1 of a bounded solve ("Bounded fields across tiles"): the budgets, then per exchange the bound records of all
  // ranks into the bounds, the rounds under bounds, the bound step and the bounded publish.  Under a settle mode a tile
  // without nodes runs the merge of the bound records all the same: it must end with the bounds of the others.
  const bool bounded = run.bounded && pass == 0;
  const long long n_settle = bounded && run.rq.settle != TRG_FIELD_SETTLE_NONE ? run.rq.n_settle : 0;
  run.always = bounded && run.rq.settle != TRG_FIELD_SETTLE_NONE;
  TiledLocal mine(e, local);
  mine.step([&]() -> TrgStatus {
    if (!work && !bounded) return TRG_OK;
    F.tight = pass ? tb.tight.as<unsigned>() : nullptr;
    run.round = 0;
    HIPCHK(e, hipEventRecord(tb.t0, s));
    if (work && run.warm)  // (`published` is the anchor's: the border keys it left)
      launch_field_warm_start(F, delta, pass == 1, s, run.model_table(), run.rq.risk);
    else if (work)
      launch_tiled_begin(F, T, tb.entries.as<TiledEntry>(), run.n_entries, delta, tb.published.as<unsigned long long>(), s);
    if (bounded) launch_field_bounds(F, run.budgets, s);
    return TRG_OK;
  });
  // a key of a border item drops at most a few times per item in practice; the cap is the round cap's shape (under a
  // settle mode a bound record is news as well: the settle targets count beside the border nodes)
  const TrgStatus st = tiled_exchanges(
      e, x, run, mine, tiled_what(run.rq.risk), (long long)F.m * T.B + (bounded ? F.m : 0),
      [&](long long border) { return 4 * F.m * (border + n_settle) + 64; }, run.exchanges, run.records,
      [&](int, const void *d_all, int gathered) -> TrgStatus {
        if (bounded) launch_tiled_bound_merge(F, run.S, d_all, gathered, s);
        if (!work) return TRG_OK;  // (a tile without nodes under a settle mode: tb.n_rec stays 0)
        launch_tiled_merge(F, T, d_all, gathered, s);
        if (const TrgStatus r = tiled_rounds(e, run); r != TRG_OK) return r;
        if (bounded)
          launch_tiled_publish_bounded(F, T, run.S, tb.published.as<unsigned long long>(), tb.rec.p, tb.n_rec.as<int>(), s);
        else
          launch_tiled_publish(F, T, nullptr, tb.published.as<unsigned long long>(), tb.rec.p, tb.n_rec.as<int>(), s);
        return TRG_OK;
      });
  run.always = false;
  if (st != TRG_OK) return st;
  if (work) {
    run.rounds += tb.h_state->rounds;
    // the keys between the final bound and an earlier one go, ghosts included, before they become tight words
    if (bounded) launch_field_trim(F, s);
    if (pass == 0) launch_field_cost_bits(F, tb.tight.as<unsigned>(), s);
    HIPCHK(e, hipGetLastError());
  }
  if (bounded) {  // the same words on every rank: the budgets, lowered by the same bound records
    tb.h_bound.assign(FIELD_MAX_SOURCES, FIELD_INF_BITS);
    HIPCHK(e, hipMemcpyAsync(tb.h_bound.data(), F.ctrl->bound, (size_t)F.m * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
  }
  return TRG_OK;
}

// The owner pass of the set call, after its two passes (DESIGN.md section 7, "Source sets across tiles"): the third
// use of the frame.  This rank: the parent sweep, the forest of the global parents with the local roots and the
// ghosts as terminals, jumping sweeps until one moves nothing.  Then the loop: merge the gathered owner records into
// the ghost items, every item takes its final ancestor's owner where that is known, publish the border items whose
// owner became known -- each once, so m x B exchanges carry news at most, and one more ends the loop.
TrgStatus tiled_owner_pass(TrgEngine *e, ExchangeState &x, TiledRun &run) {
  TiledFieldBufs &tb = *e->tiled;
  const FieldTiled &T = tb.T;
  const FieldDev &F = run.F;
  hipStream_t s = e->s_main;
  int *owner = tb.owner.as<int>();
  const int *anc = nullptr;
  TiledLocal mine(e, TRG_OK);
  mine.step([&]() -> TrgStatus {
    if (F.N <= 0) return TRG_OK;
    int *changed = tb.own_changed.as<int>();
    HIPCHK(e, hipEventRecord(tb.t0, s));
    launch_tiled_parents(F, T, s, run.rq.risk, run.model_table());
    launch_tiled_forest_begin(F, T, tb.set_ptr.as<int>(), owner, changed, tb.n_rec.as<int>() + 1,
                              tb.published.as<unsigned long long>(), s);
    HIPCHK(e, hipMemcpyAsync(&tb.h_n[1], tb.n_rec.as<int>() + 1, sizeof(int), hipMemcpyDeviceToHost, s));
    int sweeps = 0;
    if (const TrgStatus st = field_forest_sweeps(e, F, changed, &tb.h_n[0],
                                                    run.rq.risk ? "tiled risk field sets: the owner pass's sweeps"
                                                                : "tiled cost field sets: the owner pass's sweeps",
                                                    sweeps);
        st != TRG_OK)
      return st;
    anc = F.q[sweeps & 1];
    run.roots = tb.h_n[1];  // (the first wait of the sweeps was for this copy too)
    return TRG_OK;
  });
  return tiled_exchanges(e, x, run, mine, std::string(run.rq.what) + "owner pass: ", (long long)F.m * T.B,
                         [&](long long border) { return F.m * border + 2; }, run.owner_exchanges, run.owner_records,
                         [&](int, const void *d_all, int gathered) -> TrgStatus {
                           launch_tiled_owner_step(F, T, d_all, gathered, anc, owner, tb.published.as<unsigned long long>(),
                                                   tb.rec.p, tb.n_rec.as<int>(), s);
                           return TRG_OK;
                         });
}

TrgStatus tiled_outputs(TrgEngine *e, TiledRun &run) {
  TiledFieldBufs &tb = *e->tiled;
  const FieldTiled &T = tb.T;
  const TiledRequest &rq = run.rq;
  hipStream_t s = e->s_main;
  const int n_entries = rq.set_ptr[rq.m];
  if (rq.owned) std::fill(rq.owned, rq.owned + n_entries, 0);  // (a tile without nodes owns none)
  if (rq.reached_out) std::fill(rq.reached_out, rq.reached_out + rq.m, 0);
  if (rq.bound_out)
    for (int k = 0; k < rq.m; ++k) rq.bound_out[k] = bits_float(run.bounded ? tb.h_bound[k] : FIELD_INF_BITS);
  if (rq.reached_out && run.F.N > 0 && T.V > 0)
    if (const TrgStatus st = tiled_grow(e, tb.reached, ((size_t)rq.m + 1) * sizeof(int)); st != TRG_OK) return st;
  if (run.F.N > 0 && T.V > 0) {
    const size_t nO = (size_t)rq.m * T.V, nT = (size_t)rq.m * (size_t)rq.n_targets;
    HIPCHK(e, hipEventRecord(tb.t0, s));
    // (with owners the parent sweep ran before the owner pass)
    launch_tiled_finish(run.F, T, tb.cost.as<float>(), tb.hops.as<int>(), tb.parent_out.as<int>(),
                        rq.parent != nullptr && !rq.owners, tb.owner.as<int>(), rq.owner ? tb.owner_out.as<int>() : nullptr, s,
                        rq.risk, run.model_table());
    if (rq.owners) {
      if (rq.owned) launch_tiled_owned(run.F, T, tb.set_ptr.as<int>(), tb.owner.as<int>(), n_entries, tb.owned.as<int>(), s);
      FieldSets S{};
      S.owner = tb.owner.as<int>();
      launch_field_gather(run.F, &S, tb.targets.as<int>(), rq.n_targets, rq.cost_at ? tb.cost_at.as<float>() : nullptr,
                          rq.hops_at ? tb.hops_at.as<int>() : nullptr, rq.owner_at ? tb.owner_at.as<int>() : nullptr, s);
    }
    if (rq.reached_out) launch_tiled_reached(run.F, T, tb.reached.as<int>(), s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(tb.t1, s));
    if (rq.reached_out)
      HIPCHK(e, hipMemcpyAsync(rq.reached_out, tb.reached.p, (size_t)rq.m * sizeof(int), hipMemcpyDeviceToHost, s));
    if (rq.cost) HIPCHK(e, hipMemcpyAsync(rq.cost, tb.cost.p, nO * sizeof(float), hipMemcpyDeviceToHost, s));
    if (rq.hops) HIPCHK(e, hipMemcpyAsync(rq.hops, tb.hops.p, nO * sizeof(int), hipMemcpyDeviceToHost, s));
    if (rq.parent) HIPCHK(e, hipMemcpyAsync(rq.parent, tb.parent_out.p, nO * sizeof(int), hipMemcpyDeviceToHost, s));
    if (rq.owner) HIPCHK(e, hipMemcpyAsync(rq.owner, tb.owner_out.p, nO * sizeof(int), hipMemcpyDeviceToHost, s));
    if (rq.owned) HIPCHK(e, hipMemcpyAsync(rq.owned, tb.owned.p, (size_t)n_entries * sizeof(int), hipMemcpyDeviceToHost, s));
    if (nT) {
      if (rq.cost_at) HIPCHK(e, hipMemcpyAsync(rq.cost_at, tb.cost_at.p, nT * sizeof(float), hipMemcpyDeviceToHost, s));
      if (rq.hops_at) HIPCHK(e, hipMemcpyAsync(rq.hops_at, tb.hops_at.p, nT * sizeof(int), hipMemcpyDeviceToHost, s));
      if (rq.owner_at) HIPCHK(e, hipMemcpyAsync(rq.owner_at, tb.owner_at.p, nT * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(e, hipStreamSynchronize(s));
    if (const TrgStatus st = tiled_lap(e, run); st != TRG_OK) return st;
  }
  return TRG_OK;
}

// What a solve and a refresh end with, after pass 2: with owners the owner pass (which runs the parent sweep), the
// outputs, and the record of the retained solve, from which the routes, the reached list and the next refresh start.
TrgStatus tiled_tail(TrgEngine *e, ExchangeState &x, TiledRun &run) {
  if (run.rq.owners)
    if (const TrgStatus st = tiled_owner_pass(e, x, run); st != TRG_OK) return st;
  if (const TrgStatus st = tiled_outputs(e, run); st != TRG_OK) return st;
  // retained for the routes: the keys, marks and parents lie in the work arrays as the kernels left them
  TiledFieldBufs::Solved &kept = e->tiled->solved;
  kept = TiledFieldBufs::Solved{true, run.rq.m, run.rq.owners, run.rq.owners || run.rq.parent != nullptr,
                                run.rq.risk, float_bits(e->prm.safety_factor), run.F};
  if (run.rq.models) kept.pairs.assign(run.rq.models, run.rq.models + run.rq.m);
  kept.models = run.models;
  kept.many = run.many_models;
  kept.set_ptr.assign(run.rq.set_ptr, run.rq.set_ptr + run.rq.m + 1);
  kept.set_gids.assign(run.rq.set_gids, run.rq.set_gids + run.rq.set_ptr[run.rq.m]);
  kept.node_off = e->stitch_node_off;
  kept.bounded = run.bounded;
  kept.seeded = run.rq.set_cost0 != nullptr;
  e->tiled_map.state = NodeMap::IDENTITY;  // update_graph takes the node map on from here
  return TRG_OK;
}

// The collective part of a solve whose request passed tiled_check_request: the two passes, with owners the owner pass,
// the outputs.  The owner pass is a collective: whether it runs hangs on the entry that was called, which every rank
// decides alike, never on which outputs one rank asks for.
TrgStatus tiled_solve(TrgEngine *e, TiledRun &run) {
  ExchangeState &x = *e->exchange;
  if (e->tiled) e->tiled->solved = TiledFieldBufs::Solved{};  // (a solve that fails retains nothing)
  e->tiled_map.state = NodeMap::NONE;                           // (the node map was of the retained solve's tile graph)
  // the budgets as cost bits; every rank decides alike whether the solve is a bounded one
  for (int k = 0; k < run.rq.m; ++k) {
    const float b = run.rq.budget ? run.rq.budget[k] : std::numeric_limits<float>::infinity();
    run.budgets.bits[k] = b == 0.0f ? 0u : float_bits(b);  // (-0.0 orders as +0.0)
    run.bounded = run.bounded || run.budgets.bits[k] != FIELD_INF_BITS;
  }
  run.bounded = run.bounded || run.rq.settle != TRG_FIELD_SETTLE_NONE;
  TrgStatus local = tiled_prepare(e, x, run, [] { return TRG_OK; });
  for (int pass = 0; pass < 2; ++pass) {
    const TrgStatus st = tiled_pass(e, x, run, local, pass);
    if (st != TRG_OK) return st;
    local = TRG_OK;  // (a pass that returns TRG_OK had no failure of this rank left to announce)
  }
  return tiled_tail(e, x, run);
}

// What every rank judges alike, refused before any collective.
TrgStatus tiled_check_request(TrgEngine *e, const TiledRequest &rq) {
  const std::string what = rq.what;
  const auto refuse = [&](const std::string &why) { return e->fail(TRG_ERR_INVALID_ARG, what + why); };
  if (!e->exchange || !e->exchange->transport) return refuse("no communicator (trg_engine_comm_init)");
  if (rq.m < 1 || rq.m > TRG_FIELD_BATCH_MAX) return refuse("m must be in [1, " + std::to_string(TRG_FIELD_BATCH_MAX) + "]");
  if (!rq.set_ptr || !rq.set_gids) return refuse(rq.null_ids);
  if (rq.set_ptr[0] != 0) return refuse("set_ptr[0] must be 0");
  for (int k = 0; k < rq.m; ++k) {
    if (rq.set_ptr[k + 1] < rq.set_ptr[k]) return refuse("set_ptr decreases at set " + std::to_string(k));
    if (rq.set_ptr[k + 1] == rq.set_ptr[k]) return refuse("set " + std::to_string(k) + " is empty");
  }
  const long long n_ids = e->stitch_node_off.empty() ? LLONG_MAX : e->stitch_node_off.back();  // (no stitch: tiled_graph refuses)
  for (int k = 0; k < rq.m; ++k)
    for (int j = rq.set_ptr[k]; j < rq.set_ptr[k + 1]; ++j) {
      const std::string where = "entry " + std::to_string(j - rq.set_ptr[k]) + " of set " + std::to_string(k);
      if (rq.set_gids[j] < 0 || rq.set_gids[j] >= n_ids)
        return refuse((rq.source_noun ? rq.source_noun + std::to_string(k) : where + " (" + std::to_string(rq.set_gids[j]) + ")") +
                      " is outside [0, " + std::to_string(n_ids) + ")");
      if (rq.set_cost0) {
        const float c = rq.set_cost0[j];
        if (c != c || c < 0.0f || c == __builtin_huge_valf())
          return refuse("the start cost of " + where + " is NaN, negative or infinite");
      }
    }
  // a model is a finite safety factor >= 0 and a ceiling >= 0 (+inf: none), as on one engine
  for (int k = 0; rq.models && k < rq.m; ++k) {
    if (!(rq.models[k].safety_factor >= 0.0f) || std::isinf(rq.models[k].safety_factor))
      return refuse("the safety factor of field " + std::to_string(k) + " is negative or not finite");
    if (!(rq.models[k].max_weight >= 0.0f))
      return refuse("the risk ceiling of field " + std::to_string(k) + " is negative or not a number");
  }
  if (rq.n_targets < 0 || (rq.n_targets > 0 && !rq.targets))
    return refuse("n_targets < 0, or targets is null with n_targets > 0");
  // the bounded entries' own arguments (the others leave them at their defaults)
  if (rq.budget)
    for (int k = 0; k < rq.m; ++k)
      if (!(rq.budget[k] >= 0.0f)) return refuse("the budget of field " + std::to_string(k) + " is negative or NaN");
  if (rq.settle != TRG_FIELD_SETTLE_NONE && rq.settle != TRG_FIELD_SETTLE_ANY && rq.settle != TRG_FIELD_SETTLE_ALL)
    return refuse("settle " + std::to_string(rq.settle) + " is no TRG_FIELD_SETTLE_* value");
  if (rq.settle != TRG_FIELD_SETTLE_NONE) {
    if (rq.n_settle <= 0 || !rq.settle_gids) return refuse("a settle mode needs settle targets (n_settle > 0 and settle_gids)");
    for (int j = 0; j < rq.n_settle; ++j)
      if (rq.settle_gids[j] < 0 || rq.settle_gids[j] >= n_ids)
        return refuse("settle target " + std::to_string(j) + " (" + std::to_string(rq.settle_gids[j]) + ") is outside [0, " +
                      std::to_string(n_ids) + ")");
  }
  return TRG_OK;
}

// ---- refresh across tiles (DESIGN.md section 7, "Refresh across tiles") ---------------------------------------------

// One anchor of a refresh, a fifth use of the frame: the owner pass's loop over the forest of the SUPPORTERS, with
// "this border item hangs on a member" where the owner pass trades owners.  The first anchor opens with the fill
// exchange -- every border item's carried key and this rank's member records -- and finds the supporters when the
// ghosts hold their owners' keys; it leaves the anchored keys in key0 and counts them.  The second cuts every item
// whose key is no longer key0's and jumps the same supporters.  Both end with every item that is not known to hang on a
// member losing its key, ghosts too, and `published` at the border keys that are left.  A tile without nodes takes
// part in the first anchor's exchanges all the same: it must end with the members' new ids of the others.
TrgStatus tiled_anchor(TrgEngine *e, ExchangeState &x, TiledRun &run, TrgStatus local, bool first) {
  TiledFieldBufs &tb = *e->tiled;
  const FieldTiled &T = tb.T;
  const FieldDev &F = run.F;
  hipStream_t s = e->s_main;
  const bool work = F.N > 0;
  const int fill = first ? 1 : 0;
  const int n_members = run.rq.set_ptr[run.rq.m];
  int *rooted = tb.rooted.as<int>();
  unsigned long long *key0 = tb.key0.as<unsigned long long>();
  unsigned long long *published = tb.published.as<unsigned long long>();
  const std::string what = std::string(run.rq.what) + "anchor: ";
  const int *anc = nullptr;
  const int before = run.anchor_exchanges;
  run.always = first;
  TiledLocal mine(e, local);
  mine.step([&]() -> TrgStatus {
    HIPCHK(e, hipEventRecord(tb.t0, s));
    return TRG_OK;
  });
  const TrgStatus st = tiled_exchanges(
      e, x, run, mine, what, (long long)F.m * T.B + (first ? run.n_entries : 0),
      [&](long long border) { return F.m * border + 2 + fill; }, run.anchor_exchanges, run.anchor_records,
      [&](int exchange, const void *d_all, int gathered) -> TrgStatus {
        if (exchange < fill) {
          if (work)
            launch_tiled_fill_publish(F, T, tb.entries.as<TiledEntry>(), run.n_entries, published, tb.rec.p, tb.n_rec.as<int>(), s);
          return TRG_OK;
        }
        if (exchange == fill) {
          if (first) launch_tiled_fill_ghosts(F, T, d_all, gathered, tb.members.as<int>(), n_members, s);
          if (!work) return TRG_OK;
          int *changed = tb.own_changed.as<int>();
          if (first) launch_tiled_parents(F, T, s, run.rq.risk, run.model_table());  // (pass 1 writes no parent)
          launch_tiled_anchor_begin(F, T, first ? nullptr : key0, rooted, changed, published, s);
          int sweeps = 0;
          if (const TrgStatus r = field_forest_sweeps(e, F, changed, &tb.h_n[0], "tiled field refresh: an anchor's sweeps", sweeps);
              r != TRG_OK)
            return r;
          anc = F.q[sweeps & 1];
          d_all = nullptr;  // (the fill's records are no verdicts)
          gathered = 0;
        }
        if (work) launch_tiled_owner_step(F, T, d_all, gathered, anc, rooted, published, tb.rec.p, tb.n_rec.as<int>(), s);
        return TRG_OK;
      });
  run.always = false;
  if (st != TRG_OK) return st;
  if (run.anchor_exchanges - before <= fill)  // (never: some rank owns a member and published its record)
    return e->fail(TRG_ERR_DEVICE, what + "the fill exchange carried no record");
  if (work) {
    HIPCHK(e, hipEventRecord(tb.t0, s));
    launch_tiled_anchor_end(F, T, rooted, first ? key0 : nullptr, first ? tb.carried.as<int>() : nullptr, published, s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(tb.t1, s));
  }
  if (first) {
    run.h_members.assign((size_t)n_members, -1);
    run.h_carried.assign((size_t)F.m, 0);
    HIPCHK(e, hipMemcpyAsync(run.h_members.data(), tb.members.p, (size_t)n_members * sizeof(int), hipMemcpyDeviceToHost, s));
    if (work) HIPCHK(e, hipMemcpyAsync(run.h_carried.data(), tb.carried.p, (size_t)F.m * sizeof(int), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(e, hipStreamSynchronize(s));
  return work ? tiled_lap(e, run) : TRG_OK;
}

// What a refresh is given beside the set call's outputs.
struct TiledRefreshRequest {
  bool risk;  // the objective of the entry that was called
  const int32_t *new2old;
  int32_t n_map;
  float *value;
  int32_t *hops, *parent, *owner;
  const int32_t *targets;
  int32_t n_targets;
  float *value_at;
  int32_t *hops_at, *owner_at, *owned, *set_gids_out, *carried_out;
};

// The refresh of the retained tiled solve: DESIGN.md section 2's steps on the stitched graph.  What every rank judges
// alike is refused first and leaves the retained solve as it was; from there on nothing is retained until the tail.
TrgStatus tiled_refresh(TrgEngine *e, const TiledRefreshRequest &a, TrgTiledRefreshInfo *info) {
  const Clock::time_point t_total = Clock::now();
  TrgTiledRefreshInfo local_info{};
  TrgTiledRefreshInfo &out = info ? *info : local_info;
  out = TrgTiledRefreshInfo{};
  const std::string what = a.risk ? "tiled risk field refresh: " : "tiled cost field refresh: ";
  const auto refuse = [&](const std::string &why) { return e->fail(TRG_ERR_INVALID_ARG, what + why); };
  if (!e->exchange || !e->exchange->transport) return refuse("no communicator (trg_engine_comm_init)");
  if (!e->tiled || !e->tiled->solved.valid) return refuse("no tiled solve is retained (a tiled field call first)");
  ExchangeState &x = *e->exchange;
  TiledFieldBufs &tb = *e->tiled;
  if (tb.solved.bounded) return refuse("the retained solve is bounded (a bounded solve cannot be refreshed: its removed keys bound nothing)");
  if (!tb.solved.pairs.empty()) return refuse("the retained solve has cost models (a modelled solve cannot be refreshed)");
  if (tb.solved.seeded)
    return refuse("the retained solve has start costs (a seeded solve cannot be refreshed: its members' keys are not carried)");
  if (tb.solved.risk != a.risk)
    return refuse(a.risk ? "the retained solve is a cost field (use trg_engine_tiled_cost_field_refresh)"
                         : "the retained solve is a risk field (use trg_engine_tiled_risk_field_refresh)");
  if ((int)tb.solved.node_off.size() - 1 != x.nranks)
    return refuse("the communicator has " + std::to_string(x.nranks) + " ranks, the retained solve had " +
                  std::to_string((int)tb.solved.node_off.size() - 1));
  if (a.n_targets < 0 || (a.n_targets > 0 && !a.targets)) return refuse("n_targets < 0, or targets is null with n_targets > 0");
  // ---- collective from here on: nothing is retained until the tail has run ----
  TiledFieldBufs::Solved old = std::move(tb.solved);
  tb.solved = TiledFieldBufs::Solved{};
  const NodeMap::State map_state = e->tiled_map.state;
  e->tiled_map.state = NodeMap::NONE;
  const int m = old.m, n_members = old.set_ptr[m];
  std::vector<int32_t> gids((size_t)n_members, -1);  // the members' new global ids: this rank's own, then all
  TiledRequest rq{m, old.set_ptr.data(), gids.data(), nullptr, a.value, a.hops, a.parent, old.owners, a.risk, what.c_str(),
                  "", nullptr};
  if (old.owners) {
    rq.owner = a.owner;
    rq.targets = a.targets;
    rq.n_targets = a.n_targets;
    rq.cost_at = a.value_at;
    rq.hops_at = a.hops_at;
    rq.owner_at = a.owner_at;
    rq.owned = a.owned;
  }
  TiledRun run{rq};
  run.warm = true;
  for (int k = 0; k < m; ++k) run.budgets.bits[k] = FIELD_INF_BITS;
  hipStream_t s = e->s_main;
  // Step 1, the carry, between the new solve graph and the regrown work arrays: the map, this rank's members, the keys.
  const auto carry = [&]() -> TrgStatus {
    const FieldTiled &T = tb.T;
    const int rank = x.rank, V = T.V;
    const int V_old = old.node_off[rank + 1] - old.node_off[rank];
    const int32_t *map = a.new2old;
    int32_t n_map = a.n_map;
    std::vector<int32_t> identity;
    if (!map) {
      if (map_state == NodeMap::NONE)
        return refuse("no node map is given and the engine has none for this tile's graph (pass new2old, or solve again)");
      if (map_state == NodeMap::IDENTITY) {
        identity.resize((size_t)V_old);
        for (int v = 0; v < V_old; ++v) identity[v] = v;
        map = identity.data();
        n_map = V_old;
      } else {
        map = e->tiled_map.ids.data();
        n_map = (int32_t)e->tiled_map.ids.size();
      }
    }
    if (n_map != V)
      return refuse("the node map has " + std::to_string(n_map) + " entries, the tile " + std::to_string(V) + " nodes");
    std::vector<int32_t> first((size_t)V_old, -1);  // the first node of the tile's graph now that names an old one
    for (int v = 0; v < V; ++v) {
      const int o = map[v];
      if (o < -1 || o >= V_old)
        return refuse("node map entry " + std::to_string(v) + " (" + std::to_string(o) + ") is no node of this tile at the retained solve (" +
                      std::to_string(V_old) + " nodes) and not -1");
      if (o >= 0 && first[o] < 0) first[o] = v;
    }
    for (int k = 0; k < m; ++k)
      for (int j = old.set_ptr[k]; j < old.set_ptr[k + 1]; ++j) {
        const int32_t g = old.set_gids[j];
        const int owner = (int)(std::upper_bound(old.node_off.begin(), old.node_off.end(), g) - old.node_off.begin()) - 1;
        if (owner != rank) continue;
        const int l = g - old.node_off[rank];
        if (l < 0 || l >= V_old || first[l] < 0)
          return refuse("member " + std::to_string(j - old.set_ptr[k]) + " of set " + std::to_string(k) + " (global id " +
                        std::to_string(g) + " of the retained solve) has no node in this tile's graph");
        gids[j] = T.lo + first[l];
      }
    if (V <= 0) return TRG_OK;
    TrgStatus st;
    if ((st = tiled_grow(e, tb.carry, ((size_t)m * V + 4) * sizeof(unsigned long long))) != TRG_OK ||
        (st = tiled_grow(e, tb.node_map, ((size_t)V + 4) * sizeof(int))) != TRG_OK)
      return st;
    HIPCHK(e, hipMemcpyAsync(tb.node_map.p, map, (size_t)V * sizeof(int), hipMemcpyHostToDevice, s));
    launch_tiled_carry(old.F.key, old.F.V, V_old, tb.node_map.as<int>(), V, m, tb.carry.as<unsigned long long>(), s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(s));  // (the map may be this call's own vector; the old keys are read before they move)
    return TRG_OK;
  };
  TrgStatus local = tiled_prepare(e, x, run, carry);
  if (local == TRG_OK)
    local = [&]() -> TrgStatus {
      const FieldTiled &T = tb.T;
      const FieldDev &F = run.F;
      const size_t nN = (size_t)F.N + 4;
      TrgStatus st;
      if ((st = tiled_grow(e, tb.key0, nN * sizeof(unsigned long long))) != TRG_OK ||
          (st = tiled_grow(e, tb.rooted, nN * sizeof(int))) != TRG_OK ||
          (st = tiled_grow(e, tb.own_changed, FIELD_OWNER_SWEEPS_MAX * sizeof(int))) != TRG_OK ||
          (st = tiled_grow(e, tb.carried, (TRG_FIELD_BATCH_MAX + 1) * sizeof(int))) != TRG_OK ||
          (st = tiled_grow(e, tb.members, ((size_t)n_members + 1) * sizeof(int))) != TRG_OK ||
          (st = tiled_grow(e, tb.rec, ((size_t)m * T.B + 4 + (size_t)run.n_entries) * FIELD_TILED_REC_BYTES)) != TRG_OK)
        return st;
      HIPCHK(e, hipMemsetAsync(tb.members.p, 0xFF, ((size_t)n_members + 1) * sizeof(int), s));
      if (F.N > 0) {
        launch_tiled_refresh_begin(F, T, tb.carry.as<unsigned long long>(), tb.entries.as<TiledEntry>(), run.n_entries, 0.0f, s);
        HIPCHK(e, hipGetLastError());
      }
      return TRG_OK;
    }();
  // Steps 2 and 3: the ghost fill and the anchor.  Then every rank knows every member's node.
  TrgStatus st = tiled_anchor(e, x, run, local, true);
  if (st != TRG_OK) return st;
  for (int j = 0; j < n_members; ++j) {
    if (run.h_members[j] < 0 || (gids[j] >= 0 && gids[j] != run.h_members[j]))
      return e->fail(TRG_ERR_DEVICE, what + "the ranks disagree on where member entry " + std::to_string(j) + " lies");
    gids[j] = run.h_members[j];
  }
  // Steps 4 to 6: pass 1 warm, the second anchor, pass 2 warm; then a solve's tail.
  if ((st = tiled_pass(e, x, run, TRG_OK, 0)) != TRG_OK || (st = tiled_anchor(e, x, run, TRG_OK, false)) != TRG_OK ||
      (st = tiled_pass(e, x, run, TRG_OK, 1)) != TRG_OK || (st = tiled_tail(e, x, run)) != TRG_OK)
    return st;
  if (a.set_gids_out) std::copy(gids.begin(), gids.end(), a.set_gids_out);
  if (a.carried_out) std::copy(run.h_carried.begin(), run.h_carried.end(), a.carried_out);
  out.exchanges = run.exchanges;
  out.anchor_exchanges = run.anchor_exchanges;
  out.owner_exchanges = run.owner_exchanges;
  out.rounds = run.rounds;
  out.ghosts = tb.T.G;
  out.border_nodes = tb.T.B;
  out.roots = run.roots;
  out.m = m;
  out.owners = old.owners ? 1 : 0;
  out.records_sent = run.records;
  out.anchor_records_sent = run.anchor_records;
  out.owner_records_sent = run.owner_records;
  out.ms_device = (float)run.ms_device;
  out.ms_total = (float)ms_since(t_total);
  return TRG_OK;
}

// The reached list of one field of the retained tiled solve over THIS tile's nodes ("Bounded fields across tiles"):
// count, scan and emit on the device, global ids ascending.  Local work, no collective.
TrgStatus tiled_field_reached(TrgEngine *e, int32_t field, int32_t *gids, float *value, int32_t *hops, int32_t cap,
                              int32_t *n_out) {
  const std::string what = "tiled field reached: ";
  const auto refuse = [&](const std::string &why) { return e->fail(TRG_ERR_INVALID_ARG, what + why); };
  if (cap < 0) return refuse("cap < 0");
  if (!e->tiled || !e->tiled->solved.valid) return refuse("no tiled solve is retained (a tiled field call first)");
  TiledFieldBufs &tb = *e->tiled;
  if (tb.version != e->graph_version || tb.serial != e->stitch_serial ||
      (!tb.solved.risk && tb.solved.sf_bits != float_bits(e->prm.safety_factor)))
    return refuse("the retained tiled solve is stale (the tile's graph, the stitch or the safety factor changed since)");
  const FieldDev &F = tb.solved.F;
  const FieldTiled &T = tb.T;
  if (field < 0 || field >= tb.solved.m)
    return refuse("field " + std::to_string(field) + " out of range (the solve has " + std::to_string(tb.solved.m) + ")");
  if (n_out) *n_out = 0;
  if (T.V <= 0 || F.N <= 0) return TRG_OK;  // (a tile without nodes)
  const bool want = cap > 0 && (gids || value || hops);
  const int room = want ? std::min<int>(cap, T.V) : 0;
  const size_t nb = ((size_t)T.V + 255) / 256;
  TrgStatus st;
  if ((st = tiled_grow(e, tb.list_counts, (nb + 1) * sizeof(int))) != TRG_OK ||
      (st = tiled_grow(e, tb.list_off, (nb + 1) * sizeof(int))) != TRG_OK ||
      (st = tiled_grow(e, tb.list_tmp, (nb / 2048 + 8) * sizeof(int))) != TRG_OK)
    return st;
  if (gids && (st = tiled_grow(e, tb.list_gids, ((size_t)room + 4) * sizeof(int))) != TRG_OK) return st;
  if (value && (st = tiled_grow(e, tb.list_value, ((size_t)room + 4) * sizeof(float))) != TRG_OK) return st;
  if (hops && (st = tiled_grow(e, tb.list_hops, ((size_t)room + 4) * sizeof(int))) != TRG_OK) return st;
  hipStream_t s = e->s_main;
  launch_tiled_reached_list(F, T, field, tb.list_counts.as<int>(), tb.list_off.as<int>(), tb.list_tmp.as<int>(), room,
                            gids ? tb.list_gids.as<int>() : nullptr, value ? tb.list_value.as<float>() : nullptr,
                            hops ? tb.list_hops.as<int>() : nullptr, s);
  HIPCHK(e, hipGetLastError());
  int total = 0;
  HIPCHK(e, hipMemcpyAsync(&total, tb.list_off.as<int>() + nb, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  if (total < 0 || total > T.V) return e->fail(TRG_ERR_DEVICE, what + "bad count");
  const size_t n = (size_t)std::min(total, room);
  if (n > 0) {
    if (gids) HIPCHK(e, hipMemcpyAsync(gids, tb.list_gids.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    if (value) HIPCHK(e, hipMemcpyAsync(value, tb.list_value.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (hops) HIPCHK(e, hipMemcpyAsync(hops, tb.list_hops.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
  }
  if (n_out) *n_out = total;
  return TRG_OK;
}

// One call: the refusals, the solve, the fields that both info structs have, then the call's own through `more`.
template <typename Info, typename More>
TrgStatus tiled_call(TrgEngine *e, const TiledRequest &rq, Info *info, More more) {
  const Clock::time_point t_total = Clock::now();
  Info local{};
  Info &out = info ? *info : local;
  out = Info{};
  if (const TrgStatus st = tiled_check_request(e, rq); st != TRG_OK) return st;
  TiledRun run{rq};
  if (const TrgStatus st = tiled_solve(e, run); st != TRG_OK) return st;
  out.exchanges = run.exchanges;
  out.rounds = run.rounds;
  out.ghosts = e->tiled->T.G;
  out.border_nodes = e->tiled->T.B;
  out.records_sent = run.records;
  more(out, run);
  out.ms_device = (float)run.ms_device;
  out.ms_total = (float)ms_since(t_total);
  return TRG_OK;
}

// The bounded entries of both objectives ("Bounded fields across tiles"): the set call's request with the `owners` flag
// that every rank passes alike -- the owner pass is a collective -- and the bounds.  Without owners the outputs that
// hang on the owner pass (owner, the targets' reads, owned) are neither read nor written: the single-source form.
TrgStatus tiled_bounded_call(TrgEngine *e, int32_t m, const int32_t *set_ptr, const int32_t *set_gids,
                             const float *set_cost0, bool owners, bool risk, const char *what, const float *budget,
                             int32_t settle, const int32_t *settle_gids, int32_t n_settle, float *value, int32_t *hops,
                             int32_t *parent, int32_t *owner, const int32_t *targets, int32_t n_targets, float *value_at,
                             int32_t *hops_at, int32_t *owner_at, int32_t *owned, float *bound_out, int32_t *reached_out,
                             TrgTiledSetInfo *info, const TrgFieldModel *models = nullptr) {
  TiledRequest rq{m, set_ptr, set_gids, set_cost0, value, hops, parent, owners, risk, what, "null set_ptr or set_gids", nullptr};
  if (owners) {
    rq.owner = owner;
    rq.targets = targets;
    rq.n_targets = n_targets;
    rq.cost_at = value_at;
    rq.hops_at = hops_at;
    rq.owner_at = owner_at;
    rq.owned = owned;
  }
  rq.budget = budget;
  rq.settle = settle;
  rq.settle_gids = settle_gids;
  rq.n_settle = n_settle;
  rq.bound_out = bound_out;
  rq.reached_out = reached_out;
  rq.models = models;
  return tiled_call(e, rq, info, [](TrgTiledSetInfo &out, const TiledRun &run) {
    out.owner_exchanges = run.owner_exchanges;
    out.roots = run.roots;
    out.owner_records_sent = run.owner_records;
  });
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

// ---- routes across tiles (DESIGN.md section 7, "Routes across tiles") ------------------------------------------------

static_assert(sizeof(TrgTiledRouteInfo) == sizeof(TiledRouteInfo) && offsetof(TrgTiledRouteInfo, num_nodes) == 0 &&
                  offsetof(TrgTiledRouteInfo, cost) == offsetof(TiledRouteInfo, cost) &&
                  offsetof(TrgTiledRouteInfo, path_length) == offsetof(TiledRouteInfo, path_length) &&
                  offsetof(TrgTiledRouteInfo, avg_risk) == offsetof(TiledRouteInfo, avg_risk) &&
                  offsetof(TrgTiledRouteInfo, root_gid) == offsetof(TiledRouteInfo, root_gid) &&
                  offsetof(TrgTiledRouteInfo, owner) == offsetof(TiledRouteInfo, owner),
              "the kernels' and the header's tiled route info differ");

struct TiledRoutesRequest {
  int32_t n;
  const int32_t *field, *target;  // n each; the targets are global ids
  int32_t *offsets;               // n + 1
  int32_t *node_gids;             // cap, may be nullptr
  float *xyz;                     // cap x 3, may be nullptr
  int32_t cap;
  TrgTiledRouteInfo *infos;       // n, may be nullptr
};

// what a LEN record looks like on the host
struct TiledLenRec {
  int32_t route, hops;
  uint32_t cost_bits;
  int32_t owner;
};
static_assert(sizeof(TiledLenRec) == FIELD_TILED_REC_BYTES, "record layout");

// The routes of the retained tiled solve: the fourth use of the frame.  Exchange 0 gathers the LEN records, from
// which every rank computes the same clipped offsets and the same cap on the exchanges; from exchange 1 on every
// rank walks what stands on its nodes, until an exchange in which no walk handed over or ended.
TrgStatus tiled_routes(TrgEngine *e, const TiledRoutesRequest &rq, TrgTiledRoutesInfo *out) {
  const Clock::time_point t_total = Clock::now();
  const std::string what = "tiled routes: ";
  const auto refuse = [&](const std::string &why) { return e->fail(TRG_ERR_INVALID_ARG, what + why); };
  // what every rank judges alike, before any collective
  if (!e->exchange || !e->exchange->transport) return refuse("no communicator (trg_engine_comm_init)");
  if (rq.n < 0) return refuse("n_routes < 0");
  if (rq.cap < 0) return refuse("cap < 0");
  if (rq.n > 0 && (!rq.field || !rq.target || !rq.offsets)) return refuse("null route_field, route_target_gid or offsets");
  if (!e->stitch_node_off.empty()) {
    const long long n_ids = e->stitch_node_off.back();
    for (int r = 0; r < rq.n; ++r)
      if (rq.target[r] < 0 || rq.target[r] >= n_ids)
        return refuse("target " + std::to_string(rq.target[r]) + " of route " + std::to_string(r) + " is outside [0, " +
                      std::to_string(n_ids) + ")");
  }
  if (rq.n == 0) {
    if (rq.offsets) rq.offsets[0] = 0;
    out->ms_total = (float)ms_since(t_total);
    return TRG_OK;
  }
  ExchangeState &x = *e->exchange;
  if (!e->tiled) e->tiled.reset(new TiledFieldBufs());
  TiledFieldBufs &tb = *e->tiled;
  const FieldTiled &T = tb.T;
  hipStream_t s = e->s_main;
  const size_t n = (size_t)rq.n;
  const bool want_ids = (rq.node_gids || rq.xyz) && rq.cap > 0;
  static const TiledRequest no_request{};
  TiledRun run{no_request};
  run.always = true;
  TiledRoutes R{};
  std::vector<int32_t> off(n + 1, 0);
  std::vector<TiledRouteInfo> infos(n);
  std::vector<TiledLenRec> lens(n);
  long long max_nodes = -1;  // known after exchange 0
  // this rank's own part before the first exchange; what fails here is announced in it
  TiledLocal mine(e, TRG_OK);
  mine.step([&]() -> TrgStatus {
    if (!tb.solved.valid) return refuse("no tiled solve is retained (trg_engine_tiled_cost_field or _sets first)");
    if (tb.version != e->graph_version || tb.serial != e->stitch_serial ||
        (!tb.solved.risk && tb.solved.sf_bits != float_bits(e->prm.safety_factor)))
      return refuse("the retained tiled solve is stale (the tile's graph, the stitch or the safety factor changed since)");
    for (int r = 0; r < rq.n; ++r)
      if (rq.field[r] < 0 || rq.field[r] >= tb.solved.m)
        return refuse("field " + std::to_string(rq.field[r]) + " of route " + std::to_string(r) +
                      " out of range (the solve has " + std::to_string(tb.solved.m) + ")");
    run.F = tb.solved.F;
    TrgStatus st;
    if ((st = tiled_grow(e, tb.route_field, n * 4)) != TRG_OK || (st = tiled_grow(e, tb.route_target, n * 4)) != TRG_OK ||
        (st = tiled_grow(e, tb.route_off, (n + 1) * 4)) != TRG_OK ||
        (st = tiled_grow(e, tb.route_info, n * sizeof(TiledRouteInfo))) != TRG_OK ||
        (st = tiled_grow(e, tb.rec, 2 * n * FIELD_TILED_REC_BYTES)) != TRG_OK || (st = tiled_grow(e, tb.n_rec, 16)) != TRG_OK)
      return st;
    HIPCHK(e, hipMemcpyAsync(tb.route_field.p, rq.field, n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(tb.route_target.p, rq.target, n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemsetAsync(tb.n_rec.p, 0, 16, s));
    HIPCHK(e, hipEventRecord(tb.t0, s));
    if (!tb.solved.parents) {  // the solve was asked for no parents: local work, no collective
      if (run.F.N > 0) launch_tiled_parents(run.F, T, s, tb.solved.risk, tb.solved.model_table());
      tb.solved.parents = true;
    }
    R.field = tb.route_field.as<int>();
    R.target = tb.route_target.as<int>();
    R.n = rq.n;
    R.w = tb.w.as<float>();
    R.dist = tb.dist.as<float>();
    R.owner = tb.solved.owners ? tb.owner.as<int>() : nullptr;
    R.rec = tb.rec.p;
    R.rec_cap = (int)std::min<size_t>(2 * n, INT_MAX);
    R.n_rec = tb.n_rec.as<int>();
    return TRG_OK;
  });
  int exchanges = 0, total = 0;
  long long records = 0;
  const TrgStatus st = tiled_exchanges(
      e, x, run, mine, what, 2 * (long long)n, [&](long long) { return max_nodes < 0 ? LLONG_MAX : max_nodes + 3; },
      exchanges, records, [&](int exchange, const void *d_all, int gathered) -> TrgStatus {
        if (exchange == 0) {
          launch_tiled_route_len(run.F, T, R, s);
          return TRG_OK;
        }
        TiledRouteInfo *d_infos = tb.route_info.as<TiledRouteInfo>();
        if (exchange > 1) {
          launch_tiled_route_step(run.F, T, R, d_all, gathered, d_infos, s, tb.solved.risk, tb.solved.model_table());
          return TRG_OK;
        }
        // exchange 1: the lengths of all routes -- the one download of records -- then the walks begin
        if ((size_t)gathered != n) return e->fail(TRG_ERR_DEVICE, what + "the ranks published " + std::to_string(gathered) +
                                                                      " lengths for " + std::to_string(n) + " routes");
        HIPCHK(e, hipMemcpyAsync(lens.data(), d_all, n * sizeof(TiledLenRec), hipMemcpyDeviceToHost, s));
        HIPCHK(e, hipStreamSynchronize(s));
        for (TiledRouteInfo &o : infos) o = TiledRouteInfo{-1, 0.0f, 0.0f, 0.0f, -1, -1};
        for (const TiledLenRec &l : lens) {
          if (l.route < 0 || (size_t)l.route >= n || infos[l.route].num_nodes != -1 || l.hops < -1)
            return e->fail(TRG_ERR_DEVICE, what + "bad length record");
          infos[l.route] = TiledRouteInfo{l.hops + 1, bits_float(l.cost_bits), 0.0f, 0.0f, -1, l.owner};
          max_nodes = std::max<long long>(max_nodes, (long long)l.hops + 1);
        }
        max_nodes = std::max<long long>(max_nodes, 0);
        if (want_ids)  // a route that no longer fits is truncated, later routes are empty ranges
          for (size_t r = 0; r < n; ++r)
            off[r + 1] = (int32_t)std::min<long long>((long long)off[r] + infos[r].num_nodes, rq.cap);
        total = off[n];
        HIPCHK(e, hipMemcpyAsync(tb.route_info.p, infos.data(), n * sizeof(TiledRouteInfo), hipMemcpyHostToDevice, s));
        if (want_ids) {
          if (const TrgStatus g = tiled_grow(e, tb.route_gids, ((size_t)total + 4) * 4); g != TRG_OK) return g;
          HIPCHK(e, hipMemcpyAsync(tb.route_off.p, off.data(), (n + 1) * 4, hipMemcpyHostToDevice, s));
          HIPCHK(e, hipMemsetAsync(tb.route_gids.p, 0xFF, ((size_t)total + 4) * 4, s));  // -1: another rank's node
          R.offsets = tb.route_off.as<int>();
          R.node_gids = tb.route_gids.as<int>();
        }
        launch_tiled_route_step(run.F, T, R, nullptr, 0, d_infos, s, tb.solved.risk, tb.solved.model_table());
        return TRG_OK;
      });
  if (st != TRG_OK) return st;
  // every rank holds the same infos; the ids are this rank's own
  std::vector<int32_t> ids;
  int32_t *ids_out = rq.node_gids;
  if (total > 0) {
    if (!ids_out) {
      ids.resize((size_t)total);
      ids_out = ids.data();
    }
    HIPCHK(e, hipMemcpyAsync(ids_out, tb.route_gids.p, (size_t)total * 4, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(e, hipMemcpyAsync(infos.data(), tb.route_info.p, n * sizeof(TiledRouteInfo), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  for (size_t r = 0; r < n; ++r)
    if (infos[r].num_nodes > 0 && infos[r].root_gid < 0)
      return e->fail(TRG_ERR_DEVICE, what + "the walk of route " + std::to_string(r) + " did not end at a root");
  std::copy(off.begin(), off.end(), rq.offsets);
  if (rq.infos)
    for (size_t r = 0; r < n; ++r)
      rq.infos[r] = TrgTiledRouteInfo{infos[r].num_nodes, infos[r].cost, infos[r].path_length, infos[r].avg_risk,
                                      infos[r].root_gid, infos[r].owner};
  if (rq.xyz) {
    const float nan = __builtin_nanf("");
    for (int i = 0; i < total; ++i) {
      const long long l = (long long)ids_out[i] - T.lo;
      if (ids_out[i] >= 0 && (l < 0 || l >= T.V || (size_t)l >= e->nx.size()))
        return e->fail(TRG_ERR_DEVICE, what + "a walk left this tile's nodes");
      const bool own = ids_out[i] >= 0;
      rq.xyz[3 * i] = own ? e->nx[l] : nan;
      rq.xyz[3 * i + 1] = own ? e->ny[l] : nan;
      rq.xyz[3 * i + 2] = own ? e->nz[l] : nan;
    }
  }
  out->exchanges = exchanges;
  out->max_nodes = (int32_t)max_nodes;
  out->records_sent = records;
  out->ms_device = (float)run.ms_device;
  out->ms_total = (float)ms_since(t_total);
  return TRG_OK;
}

}  // namespace

extern "C" {

TrgStatus trg_engine_tiled_cost_field(TrgEngine *e, int32_t m, const int32_t *source_gids, float *cost, int32_t *hops,
                                      int32_t *parent, TrgTiledFieldInfo *info) {
  return entry(e, "tiled_cost_field", DEVICE, [&] {
    int32_t one_each[TRG_FIELD_BATCH_MAX + 1];  // m sets of one entry
    for (int k = 0; k <= TRG_FIELD_BATCH_MAX; ++k) one_each[k] = k;
    const TiledRequest rq{m, one_each, source_gids, nullptr, cost, hops, parent, false, false, "tiled cost field: ",
                          "null source_gids", "the source of field "};
    return tiled_call(e, rq, info, [](TrgTiledFieldInfo &, const TiledRun &) {});
  });
}

TrgStatus trg_engine_tiled_cost_field_sets(TrgEngine *e, int32_t m, const int32_t *set_ptr, const int32_t *set_gids,
                                           const float *set_cost0, float *cost, int32_t *hops, int32_t *parent,
                                           int32_t *owner, const int32_t *targets, int32_t n_targets, float *cost_at,
                                           int32_t *hops_at, int32_t *owner_at, int32_t *owned, TrgTiledSetInfo *info) {
  return entry(e, "tiled_cost_field_sets", DEVICE, [&] {
    const TiledRequest rq{m, set_ptr, set_gids, set_cost0, cost, hops, parent, true, false, "tiled cost field sets: ",
                          "null set_ptr or set_gids", nullptr, owner, targets, n_targets, cost_at, hops_at, owner_at, owned};
    return tiled_call(e, rq, info, [](TrgTiledSetInfo &out, const TiledRun &run) {
      out.owner_exchanges = run.owner_exchanges;
      out.roots = run.roots;
      out.owner_records_sent = run.owner_records;
    });
  });
}

TrgStatus trg_engine_tiled_risk_field(TrgEngine *e, int32_t m, const int32_t *source_gids, float *risk, int32_t *hops,
                                      int32_t *parent, TrgTiledFieldInfo *info) {
  return entry(e, "tiled_risk_field", DEVICE, [&] {
    int32_t one_each[TRG_FIELD_BATCH_MAX + 1];  // m sets of one entry
    for (int k = 0; k <= TRG_FIELD_BATCH_MAX; ++k) one_each[k] = k;
    const TiledRequest rq{m, one_each, source_gids, nullptr, risk, hops, parent, false, true, "tiled risk field: ",
                          "null source_gids", "the source of field "};
    return tiled_call(e, rq, info, [](TrgTiledFieldInfo &, const TiledRun &) {});
  });
}

TrgStatus trg_engine_tiled_risk_field_sets(TrgEngine *e, int32_t m, const int32_t *set_ptr, const int32_t *set_gids,
                                           float *risk, int32_t *hops, int32_t *parent, int32_t *owner,
                                           const int32_t *targets, int32_t n_targets, float *risk_at, int32_t *hops_at,
                                           int32_t *owner_at, int32_t *owned, TrgTiledSetInfo *info) {
  return entry(e, "tiled_risk_field_sets", DEVICE, [&] {
    const TiledRequest rq{m, set_ptr, set_gids, nullptr, risk, hops, parent, true, true, "tiled risk field sets: ",
                          "null set_ptr or set_gids", nullptr, owner, targets, n_targets, risk_at, hops_at, owner_at, owned};
    return tiled_call(e, rq, info, [](TrgTiledSetInfo &out, const TiledRun &run) {
      out.owner_exchanges = run.owner_exchanges;
      out.roots = run.roots;
      out.owner_records_sent = run.owner_records;
    });
  });
}

TrgStatus trg_engine_tiled_cost_field_bounded(TrgEngine *e, int32_t m, const int32_t *set_ptr, const int32_t *set_gids,
                                              const float *set_cost0, int32_t owners, const float *budget, int32_t settle,
                                              const int32_t *settle_gids, int32_t n_settle, float *cost, int32_t *hops,
                                              int32_t *parent, int32_t *owner, const int32_t *targets, int32_t n_targets,
                                              float *cost_at, int32_t *hops_at, int32_t *owner_at, int32_t *owned,
                                              float *bound_out, int32_t *reached_out, TrgTiledSetInfo *info) {
  return entry(e, "tiled_cost_field_bounded", DEVICE, [&] {
    return tiled_bounded_call(e, m, set_ptr, set_gids, set_cost0, owners != 0, false, "tiled cost field bounded: ", budget,
                              settle, settle_gids, n_settle, cost, hops, parent, owner, targets, n_targets, cost_at,
                              hops_at, owner_at, owned, bound_out, reached_out, info);
  });
}

TrgStatus trg_engine_tiled_cost_field_models(TrgEngine *e, int32_t m, const TrgFieldModel *models, const int32_t *set_ptr,
                                             const int32_t *set_gids, const float *set_cost0, int32_t owners,
                                             const float *budget, int32_t settle, const int32_t *settle_gids,
                                             int32_t n_settle, float *cost, int32_t *hops, int32_t *parent, int32_t *owner,
                                             const int32_t *targets, int32_t n_targets, float *cost_at, int32_t *hops_at,
                                             int32_t *owner_at, int32_t *owned, float *bound_out, int32_t *reached_out,
                                             TrgTiledSetInfo *info) {
  return entry(e, "tiled_cost_field_models", DEVICE, [&] {
    return tiled_bounded_call(e, m, set_ptr, set_gids, set_cost0, owners != 0, false, "tiled cost field models: ", budget,
                              settle, settle_gids, n_settle, cost, hops, parent, owner, targets, n_targets, cost_at,
                              hops_at, owner_at, owned, bound_out, reached_out, info, models);
  });
}

TrgStatus trg_engine_tiled_risk_field_bounded(TrgEngine *e, int32_t m, const int32_t *set_ptr, const int32_t *set_gids,
                                              int32_t owners, const float *budget, int32_t settle,
                                              const int32_t *settle_gids, int32_t n_settle, float *risk, int32_t *hops,
                                              int32_t *parent, int32_t *owner, const int32_t *targets, int32_t n_targets,
                                              float *risk_at, int32_t *hops_at, int32_t *owner_at, int32_t *owned,
                                              float *bound_out, int32_t *reached_out, TrgTiledSetInfo *info) {
  return entry(e, "tiled_risk_field_bounded", DEVICE, [&] {
    return tiled_bounded_call(e, m, set_ptr, set_gids, nullptr, owners != 0, true, "tiled risk field bounded: ", budget,
                              settle, settle_gids, n_settle, risk, hops, parent, owner, targets, n_targets, risk_at,
                              hops_at, owner_at, owned, bound_out, reached_out, info);
  });
}

TrgStatus trg_engine_tiled_cost_field_refresh(TrgEngine *e, const int32_t *new2old, int32_t n_map, float *cost,
                                              int32_t *hops, int32_t *parent, int32_t *owner, const int32_t *targets,
                                              int32_t n_targets, float *cost_at, int32_t *hops_at, int32_t *owner_at,
                                              int32_t *owned, int32_t *set_gids_out, int32_t *carried_out,
                                              TrgTiledRefreshInfo *info) {
  return entry(e, "tiled_cost_field_refresh", DEVICE, [&] {
    return tiled_refresh(e, TiledRefreshRequest{false, new2old, n_map, cost, hops, parent, owner, targets, n_targets, cost_at,
                                                hops_at, owner_at, owned, set_gids_out, carried_out},
                         info);
  });
}

TrgStatus trg_engine_tiled_risk_field_refresh(TrgEngine *e, const int32_t *new2old, int32_t n_map, float *risk,
                                              int32_t *hops, int32_t *parent, int32_t *owner, const int32_t *targets,
                                              int32_t n_targets, float *risk_at, int32_t *hops_at, int32_t *owner_at,
                                              int32_t *owned, int32_t *set_gids_out, int32_t *carried_out,
                                              TrgTiledRefreshInfo *info) {
  return entry(e, "tiled_risk_field_refresh", DEVICE, [&] {
    return tiled_refresh(e, TiledRefreshRequest{true, new2old, n_map, risk, hops, parent, owner, targets, n_targets, risk_at,
                                                hops_at, owner_at, owned, set_gids_out, carried_out},
                         info);
  });
}

TrgStatus trg_engine_tiled_field_reached(TrgEngine *e, int32_t field, int32_t *gids, float *value, int32_t *hops,
                                         int32_t cap, int32_t *n_out) {
  return entry(e, "tiled_field_reached", DEVICE,
               [&] { return tiled_field_reached(e, field, gids, value, hops, cap, n_out); });
}

TrgStatus trg_engine_tiled_field_routes(TrgEngine *e, int32_t n_routes, const int32_t *route_field,
                                        const int32_t *route_target_gid, int32_t *offsets, int32_t *node_gids,
                                        float *xyz, int32_t cap, TrgTiledRouteInfo *infos, TrgTiledRoutesInfo *info) {
  return entry(e, "tiled_field_routes", DEVICE, [&] {
    TrgTiledRoutesInfo local{};
    TrgTiledRoutesInfo &out = info ? *info : local;
    out = TrgTiledRoutesInfo{};
    return tiled_routes(e, TiledRoutesRequest{n_routes, route_field, route_target_gid, offsets, node_gids, xyz, cap, infos},
                        &out);
  });
}

TrgStatus trg_engine_stitch_ids(TrgEngine *e, int32_t *first_gid, int32_t *num_nodes, int32_t *total_nodes) {
  if (!first_gid || !num_nodes || !total_nodes) return TRG_ERR_INVALID_ARG;
  return entry(e, "stitch_ids", ENGINE, [&] { return stitch_ids(e, first_gid, num_nodes, total_nodes); });
}

}  // extern "C"
