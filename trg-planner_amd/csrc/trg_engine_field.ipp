// Part of trg_engine.cpp (included at file scope): the cost field of the global graph -- the least (cost, hops)
// key from one node to every node, on the device, for up to TRG_FIELD_BATCH_MAX sources in one solve (kernels:
// trg_field.hip; an extension, the reference has no such call) -- and its C ABI entries.  One solver: the
// single-source entry is its m == 1 call, the batch entry the bounded one's call without budgets or a settle mode;
// the refresh (trg_engine_cost_field_refresh) is a request of its own kind to the same field_solve: a check phase
// before the others, the retained keys carried in before the work arrays, and passes that start warm.  A risk field
// (trg_engine_risk_field_sets; DESIGN.md section 2, "Risk fields") is the set entry's request with one flag: the
// edge risks in the place of the edge costs, and kernels that extend a key by max instead of +; its refresh
// (trg_engine_risk_field_refresh) is the refresh request with that flag.

namespace {

// rounds enqueued between two looks at the pinned "work left" word
constexpr int FIELD_BATCH = 32;

inline uint32_t float_bits(float f) {
  uint32_t b;
  memcpy(&b, &f, sizeof b);
  return b;
}
inline float bits_float(uint32_t b) {
  float f;
  memcpy(&f, &b, sizeof f);
  return f;
}

// device buffers of the cost field, owned by the engine
struct FieldBufs {
  DevArr ec, stats, ctrl;
  DevArr key, q[2], far[2], stamp_near, stamp_far, parent, cost, hops;  // per item: m x V entries
  DevArr targets, cost_at, hops_at;                                           // n_targets, m x n_targets
  // The edge-cost cache ("Cost models"): `ec` holds slot i at i * ec_stride, one slot per
  // cost model met, for one graph_version and column array.  Slot 0 is the engine's own model and is never given
  // away; the others go to the model a solve needs and does not find, the least recently used first.
  struct CostSlot {
    uint32_t sf_bits, tau_bits;  // the model, as bits; (FIELD_RISK_SLOT, FIELD_RISK_SLOT): the edge risks
    bool valid;                  // the costs and the three words below are computed
    double sum;                  // over admitted edges
    long long count;
    bool bad;                    // some edge cost is negative or not finite
    uint64_t used;               // ec_tick of the last solve that read it
    // the keep-out zones of the slot ("Keep-out zones"), part of its identity, compared as bytes;
    // empty: a slot of the model, or of the edge risks, alone (slot 0 always is)
    std::vector<TrgZone> zones;
  };
  std::vector<CostSlot> slots;
  size_t ec_stride = 0;      // entries from one slot to the next
  uint64_t ec_tick = 0;
  uint64_t ec_version = 0;   // graph_version of the edge costs (0: none)
  const void *ec_col = nullptr;  // ... and the column array they were computed from
  // The last solve, kept on the device for trg_engine_field_routes: set by a successful solve, cleared when a
  // solve begins its device work; a graph_version other than the engine's (init_graph, update_graph, load_json,
  // a reset) makes it stale, so does a device graph (ensure_dev_graph) that is no longer the one it ran on (the
  // device build's, once an update_graph began, whether or not it finished), and field_release drops it with the
  // buffers.
  struct Last {
    uint64_t version = 0;    // graph_version of the solve (0: none)
    FieldDev F{};            // keys, parents and the CSR it ran on (ensure_dev_graph's, as are w and dist)
    const float *w = nullptr, *dist = nullptr;  // that CSR's edge arrays
    FieldSources sources{};  // a walk must end at its field's
    bool parents = false;    // the parent sweep ran
    std::optional<FieldSets> sets;  // of a set solve ("Source sets"), on the device
    bool owners = false;     // ... and the owner pass ran: sets->owner is filled
    bool bounded = false;    // keys above a bound were removed: nothing a refresh can start from
    bool risk = false;       // a risk solve ("Risk fields"): F.ec holds the edge risks
    bool seeded = false;     // its members had start costs ("Start costs"): no refresh either
    // its cost models ("Cost models"): per field, empty when the request named none; F.ec is
    // the slot all fields share, or with `many` slot 0 and `models` the table the kernels take
    std::vector<TrgFieldModel> pairs;
    FieldModels models{};
    bool many = false;
    ZoneSets zones;  // its keep-out zone lists ("Keep-out zones"); empty(): it had none
    // (F.V and F.m are the node count of its graph and its fields: what a refresh reads the old keys by)
  } last;
  DevArr set_ptr, set_ids, owner, owner_at, owned, own_changed;  // set solves; owner: m x V, only when asked for
  DevArr set_cost0;          // ... with start costs: one cost word per entry
  // keep-out zones: the lists of the slots being computed (FIELD_ZONES_MAX zones a slot, in the order of `fresh`), and
  // the verdicts and counts of trg_engine_zone_edges
  DevArr zones, zone_closed, zone_inside, zone_counts;
  std::vector<int32_t> h_set_ptr, h_set_ids;  // the sets as uploaded, for a refresh to carry to the next graph
  DevArr key0, node_map, carried;  // refresh: the carried, then the anchored keys (m x V); new2old (V); counts (m)
  Pinned<int> h_carried;     // per field
  Pinned<int> h_changed;     // the owner pass's "a sweep moved something" word
  DevArr route_field, route_target, route_len, route_off, route_ids, route_info;
  DevArr list_counts, list_off, list_tmp, list_ids, list_cost, list_hops;  // trg_engine_field_reached
  Pinned<unsigned> h_bound;  // per field, as cost bits (bounded solves)
  Pinned<FieldState> h_state;
  Pinned<FieldEdgeStats> h_stats;
  Pinned<int> h_reached;  // per field
  Event t0, t1;
};

void field_release(TrgEngine *e) {
  if (!e->field) return;
  if (e->device_ok) {
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->s_main);
  }
  e->field.reset();
}

static_assert(FIELD_MAX_SOURCES == TRG_FIELD_BATCH_MAX, "the kernels' and the header's batch limit differ");
static_assert(FIELD_ZONES_MAX == TRG_ZONES_MAX && sizeof(FieldZone) == sizeof(TrgZone) &&
                  offsetof(FieldZone, r) == offsetof(TrgZone, r),
              "the kernels' and the header's zones differ");
// the engine's own slot and one per field of the largest batch
constexpr int FIELD_SLOTS_MAX = FIELD_MAX_SOURCES + 1;
// The key of the slot that holds the edge risks ("Risk fields"): a NaN pattern in both words,
// which no model has (field_check_models refuses a NaN).  It is never slot 0, lives and dies with the cache like any
// other slot (graph_version, column array), and is taken or given away by the same least-recently-used rule.
constexpr uint32_t FIELD_RISK_SLOT = 0xFFFFFFFFu;

// What an entry asks of field_solve.  Every entry value-initialises one and names what it sets: all else is null, 0,
// false, TRG_FIELD_SETTLE_NONE.
struct FieldRequest {
  int32_t m;
  const int32_t *source_ids;  // m, or nullptr: all from source_xy
  const float *source_xy;     // m x 2
  float *cost;                // m x V each, any may be nullptr
  int32_t *hops, *parent;
  const int32_t *targets;     // n_targets node ids
  int32_t n_targets;
  float *cost_at;             // m x n_targets each, any may be nullptr
  int32_t *hops_at;
  int32_t *sources_out, *reached_out;  // m
  bool resolve_only;          // nothing but sources_out is wanted: no solve
  const float *budget;        // m, or nullptr: +inf each
  int32_t settle;             // TRG_FIELD_SETTLE_*, over `targets`
  float *bound_out;           // m, may be nullptr
  // a set solve (trg_engine_cost_field_sets): field k starts from set_ids[set_ptr[k] .. set_ptr[k + 1])
  const int32_t *set_ptr, *set_ids;
  const float *set_cost0;  // set_ptr[m] start costs (trg_engine_cost_field_seeded), or nullptr: +0 each
  int32_t *owner;     // m x V
  int32_t *owner_at;  // m x n_targets
  int32_t *owned;     // set_ptr[m]
  // a cost model per field (trg_engine_cost_field_models), or nullptr: the engine's for every field
  const TrgFieldModel *models;  // m
  // a keep-out zone list per field (trg_engine_cost_field_zones, trg_engine_risk_field_zones): field k's is
  // zones[zone_ptr[k] .. zone_ptr[k + 1]), or nullptr: none
  const int32_t *zone_ptr;  // m + 1
  const TrgZone *zones;
  // a refresh (trg_engine_cost_field_refresh): m and the sources or sets are the retained solve's, filled in by
  // field_check_refresh, and its keys are carried through new2old instead of a cold start
  bool refresh;
  const int32_t *new2old;  // n_map entries, or nullptr: the engine's map
  int32_t n_map;
  int32_t *carried_out;    // m
  // a risk solve (trg_engine_risk_field_sets): cost / cost_at / budget / bound_out are risks; never with models.
  // With `refresh` (trg_engine_risk_field_refresh): the objective the entry refreshes, which the retained solve's
  // must match.
  bool risk;
};
static_assert(TRG_FIELD_SETTLE_NONE == 0, "a value-initialised request has no settle mode");

// an allocation that fails is a matter of capacity
TrgStatus field_grow(TrgEngine *e, DevArr &a, size_t bytes) {
  if (ensure_bytes(e, a, bytes) == TRG_OK) return TRG_OK;
  (void)hipGetLastError();
  return e->fail(TRG_ERR_CAPACITY, "cost field: no device memory for " + std::to_string(bytes) + " bytes (" + e->err + ")");
}

// One solve on its way through the phases below: the request, what the checks derived from it, the graph and the
// work arrays on the device, and the counts that end up in `info`.
struct FieldRun {
  FieldRequest rq;          // the entry's; of a refresh, completed by field_check_refresh
  TrgFieldInfo *info;
  Clock::time_point t_total;
  FieldDev F{};             // the kernels' view; V, m and N from the checks on
  FieldSources sources{};
  FieldBounds budgets{};
  bool bounded = false;     // some budget below +inf, or a settle mode ("Bounded fields")
  bool gather = false;      // cost_at / hops_at (/ owner_at) are wanted
  FieldSets sets{};         // a set solve: n from the checks on, the device arrays from the passes on
  bool owners = false;      // owner, owner_at or owned is wanted: the owner pass runs
  DevGraph G{};             // the graph the solve runs on (ensure_dev_graph)
  int syncs = 0, rounds = 0;
  // a refresh: the retained solve's view, whose keys field_carry reads, and what field_check_refresh built for rq
  // to point at -- the identity map, the sources or the sets as ids of the current graph
  FieldDev old{};
  std::vector<int32_t> identity, src, set_ptr, set_ids;
  std::vector<TrgFieldModel> pairs;  // ... and its models
  ZoneSets zones;                    // ... and its keep-out zone lists
  std::vector<uint32_t> cost0;       // a seeded solve: the start costs as cost bits (-0 as +0), per entry
  // the edge costs of this solve (field_edge_costs): the slot table, whether the fields read more than one slot
  // (else F.ec is the one they share and no kernel takes the table), and the mean over its distinct slots
  FieldModels models{};
  bool many_models = false;
  const float *ec = nullptr;
  double mean_cost = 0.0;
  const FieldModels *model_table() const { return many_models ? &models : nullptr; }
};

constexpr uint32_t FIELD_INF_BITS = 0x7f800000u;

// is the retained solve one of the engine's graph as it is now, the device graph it ran on still current
bool field_last_current(TrgEngine *e, const FieldBufs::Last &last) {
  DevGraph now;
  return last.version == e->graph_version && ensure_dev_graph(e, 0, &now) == TRG_OK && now.rowptr == last.F.rowptr;
}

// the retained solve for `call` ("cost field routes", ...), or that call's refusal; `current`: a stale one is refused
TrgStatus field_retained(TrgEngine *e, const std::string &call, FieldBufs::Last *&last, bool current = true) {
  if (!e->field || e->field->last.version == 0)
    return e->fail(TRG_ERR_INVALID_ARG, call + ": no cost-field solve is retained (solve first)");
  last = &e->field->last;
  if (current && !field_last_current(e, *last))
    return e->fail(TRG_ERR_INVALID_ARG, call + ": the retained solve is of an earlier graph (solve again)");
  return TRG_OK;
}

// The check phase of a refresh ("Refresh"), before field_check_request's: the retained solve
// must be there, unbounded and stale; the node map is the given one, the engine's, or the identity; and m and the
// sources or sets of the request become the retained solve's, as ids of the current graph.  Like every refusal
// before field_begin, these leave the retained solve as it was.  rq.risk is the objective of the entry that was
// called: each entry refreshes the solves of its own objective only, and a match takes the flag from the retained solve.
TrgStatus field_check_refresh(TrgEngine *e, FieldRun &run) {
  FieldRequest &rq = run.rq;
  const std::string call = rq.risk ? "risk field refresh" : "cost field refresh";
  FieldBufs::Last *last;
  if (const TrgStatus st = field_retained(e, call, last, false); st != TRG_OK) return st;
  const FieldBufs::Last &old = *last;
  if (old.risk && !rq.risk)
    return e->fail(TRG_ERR_INVALID_ARG, call + ": the retained solve is a risk field (this call refreshes a cost "
                                               "field; use trg_engine_risk_field_refresh)");
  if (!old.risk && rq.risk)
    return e->fail(TRG_ERR_INVALID_ARG, call + ": the retained solve is a cost field (this call refreshes a risk "
                                               "field; use trg_engine_cost_field_refresh)");
  rq.risk = old.risk;
  if (old.bounded)
    return e->fail(TRG_ERR_INVALID_ARG, call + ": the retained solve is bounded (a bounded solve cannot be refreshed)");
  if (old.seeded)
    return e->fail(TRG_ERR_INVALID_ARG, call + ": the retained solve has start costs (a seeded solve cannot be "
                                               "refreshed: its members' keys are not carried)");
  if (field_last_current(e, old))
    return e->fail(TRG_ERR_INVALID_ARG, call + ": the retained solve is already of the current graph");
  const int V = (int)e->nx.size(), V_old = old.F.V, m = old.F.m;
  if (!rq.new2old) {
    if (e->field_map.state == NodeMap::NONE)
      return e->fail(TRG_ERR_INVALID_ARG, call + ": no node map is given and the engine has none for this graph "
                                                 "(pass new2old, or solve again)");
    if (e->field_map.state == NodeMap::IDENTITY) {
      run.identity.resize((size_t)V_old);
      for (int v = 0; v < V_old; ++v) run.identity[v] = v;
      rq.new2old = run.identity.data();
      rq.n_map = V_old;
    } else {  // (the engine's own stays in place through the phases: field_begin only marks it ended)
      rq.new2old = e->field_map.ids.data();
      rq.n_map = (int32_t)e->field_map.ids.size();
    }
  }
  if (rq.n_map != V)
    return e->fail(TRG_ERR_INVALID_ARG, call + ": the node map has " + std::to_string(rq.n_map) +
                                            " entries, the graph " + std::to_string(V) + " nodes");
  std::vector<int32_t> first((size_t)V_old, -1);  // the first node of the current graph that names an old one
  for (int v = 0; v < V; ++v) {
    const int o = rq.new2old[v];
    if (o < -1 || o >= V_old)
      return e->fail(TRG_ERR_INVALID_ARG, call + ": node map entry " + std::to_string(v) + " (" + std::to_string(o) +
                                              ") is no node of the retained solve's graph (" + std::to_string(V_old) +
                                              " nodes) and not -1");
    if (o >= 0 && first[o] < 0) first[o] = v;
  }
  if ((rq.owner || rq.owner_at) && !old.sets)
    return e->fail(TRG_ERR_INVALID_ARG, call + ": owner / owner_at asked of a solve without sets");
  if (rq.n_targets < 0) return e->fail(TRG_ERR_INVALID_ARG, call + ": n_targets < 0");
  const FieldBufs &fb = *e->field;
  if (old.sets) {
    run.set_ptr = fb.h_set_ptr;  // (a copy: field_uploads writes the host record again)
    run.set_ids.resize(fb.h_set_ids.size());
    for (int k = 0; k < m; ++k)
      for (int j = fb.h_set_ptr[k]; j < fb.h_set_ptr[k + 1]; ++j)
        if ((run.set_ids[j] = first[fb.h_set_ids[j]]) < 0)
          return e->fail(TRG_ERR_INVALID_ARG, call + ": member " + std::to_string(j - fb.h_set_ptr[k]) + " of set " +
                                                  std::to_string(k) + " (node " + std::to_string(fb.h_set_ids[j]) +
                                                  " of the retained solve's graph) has no node in the current graph");
    rq.set_ptr = run.set_ptr.data();
    rq.set_ids = run.set_ids.data();
  } else {
    run.src.resize((size_t)m);
    for (int k = 0; k < m; ++k)
      if ((run.src[k] = first[old.sources.id[k]]) < 0)
        return e->fail(TRG_ERR_INVALID_ARG, call + ": the source of field " + std::to_string(k) + " (node " +
                                                std::to_string(old.sources.id[k]) +
                                                " of the retained solve's graph) has no node in the current graph");
    rq.source_ids = run.src.data();
  }
  rq.m = m;
  run.old = old.F;
  if (!old.pairs.empty()) {  // the retained models, whose costs field_edge_costs derives again on this graph
    run.pairs = old.pairs;
    rq.models = run.pairs.data();
  }
  if (!old.zones.empty()) {  // ... and the retained zone lists, whose closures it derives again from this graph's positions
    run.zones = old.zones;
    rq.zone_ptr = run.zones.ptr.data();
    rq.zones = run.zones.zones.data();
  }
  return TRG_OK;
}

// The sets of a set solve (trg_engine_cost_field_sets): set_ptr from 0 and strictly ascending, every id a node; a
// start cost (trg_engine_cost_field_seeded) is a finite number >= 0, kept as cost bits with -0 as +0.
// Field k's source, for `info` and the reached list, is its set's first id.
TrgStatus field_check_sets(TrgEngine *e, FieldRun &run) {
  const FieldRequest &rq = run.rq;
  const int V = run.F.V, m = run.F.m;
  if (rq.set_ptr[0] != 0)
    return e->fail(TRG_ERR_INVALID_ARG, "cost field sets: set_ptr[0] is " + std::to_string(rq.set_ptr[0]) + ", not 0");
  for (int k = 0; k < m; ++k) {
    if (rq.set_ptr[k + 1] <= rq.set_ptr[k])
      return e->fail(TRG_ERR_INVALID_ARG, "cost field sets: set " + std::to_string(k) + " is empty or set_ptr descends (" +
                                              std::to_string(rq.set_ptr[k]) + ", then " +
                                              std::to_string(rq.set_ptr[k + 1]) + ")");
    for (int j = rq.set_ptr[k]; j < rq.set_ptr[k + 1]; ++j)
      if (rq.set_ids[j] < 0 || rq.set_ids[j] >= V)
        return e->fail(TRG_ERR_INVALID_ARG, "cost field sets: entry " + std::to_string(j - rq.set_ptr[k]) + " of set " +
                                                std::to_string(k) + " (node " + std::to_string(rq.set_ids[j]) +
                                                ") out of range");
    run.sources.id[k] = rq.set_ids[rq.set_ptr[k]];
  }
  run.sets.n = rq.set_ptr[m];
  if (rq.set_cost0) {
    run.cost0.resize((size_t)run.sets.n);
    for (int k = 0; k < m; ++k)
      for (int j = rq.set_ptr[k]; j < rq.set_ptr[k + 1]; ++j) {
        const float c0 = rq.set_cost0[j];
        if (!(c0 >= 0.0f) || std::isinf(c0))
          return e->fail(TRG_ERR_INVALID_ARG, "cost field sets: the start cost of entry " +
                                                  std::to_string(j - rq.set_ptr[k]) + " of set " + std::to_string(k) +
                                                  " is negative or not finite");
        run.cost0[j] = float_bits(c0 + 0.0f);
      }
  }
  run.owners = rq.owner || rq.owned || (rq.owner_at && rq.n_targets > 0);
  return TRG_OK;
}

// Request checks, in the order a caller sees them: the sources (a resolve-only call ends after them), the targets,
// the 32-bit item index, and the budgets as cost bits.
TrgStatus field_check_request(TrgEngine *e, FieldRun &run) {
  const FieldRequest &rq = run.rq;
  const int V = run.F.V = (int)e->nx.size();
  const int m = run.F.m = rq.m;
  if (rq.set_ptr)
    if (const TrgStatus st = field_check_sets(e, run); st != TRG_OK) return st;
  for (int k = 0; !rq.set_ptr && k < m; ++k) {  // (a set solve has its sources)
    int src = rq.source_ids ? rq.source_ids[k] : -1;
    if (src == -1) {
      if (!rq.source_xy)
        return e->fail(TRG_ERR_INVALID_ARG, m == 1 ? "cost field: no source"
                                                   : "cost field: source " + std::to_string(k) + " needs source_xy");
      // planSafePath's start node
      src = plan_nearest_node(e, rq.source_xy[2 * k], rq.source_xy[2 * k + 1], e->plan_scratch.tied);
    }
    if (src < 0 || src >= V)
      return e->fail(TRG_ERR_INVALID_ARG, m == 1 ? "cost field: source out of range"
                                                 : "cost field: source " + std::to_string(k) + " out of range");
    run.sources.id[k] = src;
  }
  if (rq.resolve_only) {
    for (int k = 0; k < m; ++k) rq.sources_out[k] = run.sources.id[k];
    run.info->source = run.sources.id[0];
    run.info->ms_total = ms_since(run.t_total);
    return TRG_OK;
  }
  run.gather = rq.n_targets > 0 && (rq.cost_at || rq.hops_at || rq.owner_at);
  if (rq.n_targets > 0 && !rq.targets) return e->fail(TRG_ERR_INVALID_ARG, "cost field: no targets");
  for (int j = 0; j < rq.n_targets; ++j)
    if (rq.targets[j] < 0 || rq.targets[j] >= V)
      return e->fail(TRG_ERR_INVALID_ARG, "cost field: target " + std::to_string(j) + " out of range");
  // items are indexed in 32 bits (and the grid-stride loops step past the last one)
  const long long N64 = (long long)m * V;
  if (N64 > (long long)INT_MAX - (1 << 20))
    return e->fail(TRG_ERR_CAPACITY, "cost field: " + std::to_string(m) + " fields of " + std::to_string(V) +
                                         " nodes do not fit a 32-bit item index");
  if (run.gather && (long long)m * rq.n_targets > (long long)INT_MAX - (1 << 20))
    return e->fail(TRG_ERR_CAPACITY, "cost field: too many targets");
  run.F.N = (int)N64;
  // A bounded solve: some budget below +inf, or a settle mode.  Without either, the launches are those of a solve
  // that knows nothing of bounds.
  run.bounded = rq.settle != TRG_FIELD_SETTLE_NONE;
  for (int k = 0; k < m; ++k) {
    const float b = rq.budget ? rq.budget[k] : std::numeric_limits<float>::infinity();
    run.budgets.bits[k] = b == 0.0f ? 0u : float_bits(b);  // (-0.0 orders as +0.0)
    run.bounded = run.bounded || run.budgets.bits[k] != FIELD_INF_BITS;
  }
  return TRG_OK;
}

// the engine's field buffers; from here on the retained solve is gone
TrgStatus field_begin(TrgEngine *e, FieldRun &) {
  if (!e->field) e->field.reset(new FieldBufs());
  FieldBufs &fb = *e->field;
  fb.last = FieldBufs::Last{};  // from here on the work arrays change
  e->field_map.state = NodeMap::NONE;  // (the node map is of the retained solve's graph)
  HIPCHK(e, fb.h_state.ensure(1));
  HIPCHK(e, fb.h_stats.ensure(FIELD_SLOTS_MAX));
  HIPCHK(e, fb.h_reached.ensure(TRG_FIELD_BATCH_MAX));
  HIPCHK(e, fb.h_bound.ensure(TRG_FIELD_BATCH_MAX));
  HIPCHK(e, fb.t0.create());
  HIPCHK(e, fb.t1.create());
  return TRG_OK;
}

// the graph on the device (ensure_dev_graph: plan_prepare has made csr_global current); t0 follows its uploads
TrgStatus field_graph(TrgEngine *e, FieldRun &run) {
  if (const TrgStatus st = ensure_dev_graph(e, DEV_NODES | DEV_EDGES, &run.G); st != TRG_OK) return st;
  HIPCHK(e, hipEventRecord(e->field->t0, e->s_main));
  return TRG_OK;
}

// Edge costs ("Cost models"): every field's model gets a slot of the cache, found or taken;
// only the slots that are missing are computed, one launch each and ONE host wait for all their stats.  The bucket
// width's mean is over the solve's distinct slots.
TrgStatus field_edge_costs(TrgEngine *e, FieldRun &run) {
  FieldBufs &fb = *e->field;
  hipStream_t s = e->s_main;
  const DevGraph &G = run.G;
  const int m = run.F.m;
  const uint32_t sf0 = float_bits(e->prm.safety_factor);
  const size_t stride = ((size_t)G.E + 4 + 3) & ~(size_t)3;  // (slots start 16-byte aligned, 16 bytes of slack each)
  if (fb.ec_version != e->graph_version || fb.ec_col != (const void *)G.col || fb.ec_stride != stride ||
      fb.slots.empty() || fb.slots[0].sf_bits != sf0)
    fb.slots.assign(1, FieldBufs::CostSlot{sf0, FIELD_INF_BITS, false, 0.0, 0, false, 0});
  fb.ec_version = 0;  // (until this phase is through: a failure half-way leaves no cache)
  const uint64_t tick = ++fb.ec_tick;
  std::vector<int> fresh;  // the slots to compute
  for (int k = 0; k < m; ++k) {
    uint32_t sfb = run.rq.models ? float_bits(run.rq.models[k].safety_factor) : sf0;
    uint32_t taub = run.rq.models ? float_bits(run.rq.models[k].max_weight) : FIELD_INF_BITS;
    // (every field of a risk solve reads edge risks: those of its zone list, trg_engine_risk_field_zones)
    if (run.rq.risk) sfb = taub = FIELD_RISK_SLOT;
    const TrgZone *zk = run.rq.zone_ptr ? run.rq.zones + run.rq.zone_ptr[k] : nullptr;
    const size_t nzk = run.rq.zone_ptr ? (size_t)(run.rq.zone_ptr[k + 1] - run.rq.zone_ptr[k]) : 0;
    int slot = -1;
    for (size_t i = 0; i < fb.slots.size() && slot < 0; ++i)
      if (fb.slots[i].sf_bits == sfb && fb.slots[i].tau_bits == taub &&
          zone_list_equal(fb.slots[i].zones.data(), fb.slots[i].zones.size(), zk, nzk))
        slot = (int)i;
    if (slot < 0) {
      if ((int)fb.slots.size() < FIELD_SLOTS_MAX) {
        slot = (int)fb.slots.size();
        fb.slots.push_back({});
      } else {  // (a solve reads at most FIELD_MAX_SOURCES slots: one beside slot 0 is not this solve's)
        for (size_t i = 1; i < fb.slots.size(); ++i)
          if (fb.slots[i].used != tick && (slot < 0 || fb.slots[i].used < fb.slots[slot].used)) slot = (int)i;
      }
      if (slot < 0)
        return e->fail(TRG_ERR_CAPACITY, "cost field: no cache slot left for the model of field " + std::to_string(k));
      fb.slots[slot] = FieldBufs::CostSlot{sfb, taub, false, 0.0, 0, false, tick};
      if (nzk) fb.slots[slot].zones.assign(zk, zk + nzk);
    }
    FieldBufs::CostSlot &cs = fb.slots[slot];
    if (!cs.valid && std::find(fresh.begin(), fresh.end(), slot) == fresh.end()) fresh.push_back(slot);
    cs.used = tick;
    run.models.slot[k] = slot;
  }
  if (!fresh.empty() || !fb.ec.p) {
    const size_t bytes = fb.slots.size() * stride * sizeof(float);
    if (ensure_bytes(e, fb.ec, bytes, true) != TRG_OK ||
        ensure_bytes(e, fb.stats, FIELD_SLOTS_MAX * sizeof(FieldEdgeStats)) != TRG_OK) {
      (void)hipGetLastError();
      return e->fail(TRG_ERR_CAPACITY, "cost field: no device memory for the edge costs of " +
                                           std::to_string(fb.slots.size()) + " cost models (" + e->err + ")");
    }
  }
  if (!fresh.empty()) {
    FieldEdgeStats *d_stats = fb.stats.as<FieldEdgeStats>();
    bool zoned = false;
    for (const int i : fresh) zoned = zoned || !fb.slots[i].zones.empty();
    if (zoned)  // (the lists stay in place until this phase's host wait)
      if (const TrgStatus st = field_grow(e, fb.zones, fresh.size() * FIELD_ZONES_MAX * sizeof(FieldZone)); st != TRG_OK)
        return st;
    for (size_t j = 0; j < fresh.size(); ++j) {
      const FieldBufs::CostSlot &cs = fb.slots[fresh[j]];
      float *slot = fb.ec.as<float>() + (size_t)fresh[j] * stride;
      const bool risk_slot = cs.sf_bits == FIELD_RISK_SLOT && cs.tau_bits == FIELD_RISK_SLOT;
      FieldZone *d_zones = nullptr;
      if (!cs.zones.empty()) {
        d_zones = fb.zones.as<FieldZone>() + j * FIELD_ZONES_MAX;
        HIPCHK(e, hipMemcpyAsync(d_zones, cs.zones.data(), cs.zones.size() * sizeof(FieldZone), hipMemcpyHostToDevice, s));
      }
      if (risk_slot && d_zones) {
        launch_field_edge_risk_zones(G.rowptr, G.col, G.w, G.state, G.xyz, run.F.V, G.E, d_zones, (int)cs.zones.size(),
                                     slot, d_stats + j, s);
      } else if (risk_slot) {
        launch_field_edge_risk(G.col, G.w, G.state, run.F.V, G.E, slot, d_stats + j, s);
      } else if (d_zones) {
        launch_field_edge_zones(G.rowptr, G.col, G.w, G.dist, G.state, G.xyz, run.F.V, G.E, bits_float(cs.sf_bits),
                                bits_float(cs.tau_bits), d_zones, (int)cs.zones.size(), slot, d_stats + j, s);
      } else
        launch_field_edge_cost(G.col, G.w, G.dist, G.state, run.F.V, G.E, bits_float(cs.sf_bits),
                               bits_float(cs.tau_bits), slot, d_stats + j, s);
    }
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(fb.h_stats, d_stats, fresh.size() * sizeof(FieldEdgeStats), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    run.syncs++;
    for (size_t j = 0; j < fresh.size(); ++j) {
      FieldBufs::CostSlot &cs = fb.slots[fresh[j]];
      cs.sum = fb.h_stats[j].sum;
      cs.count = fb.h_stats[j].count;
      cs.bad = fb.h_stats[j].bad != 0;
      cs.valid = true;
    }
  }
  fb.ec_version = e->graph_version;
  fb.ec_col = G.col;
  fb.ec_stride = stride;
  double sum = 0.0;
  long long count = 0;
  for (int k = 0; k < m; ++k) {
    const int slot = run.models.slot[k];
    const FieldBufs::CostSlot &cs = fb.slots[slot];
    if (cs.bad && run.rq.risk)
      return e->fail(TRG_ERR_INVALID_ARG, "risk field: an edge weight is negative or not finite");
    if (cs.bad)
      return e->fail(TRG_ERR_INVALID_ARG,
                     "cost field: an edge cost is negative or not finite under the model of field " + std::to_string(k));
    bool seen = false;
    for (int j = 0; j < k && !seen; ++j) seen = run.models.slot[j] == slot;
    if (!seen) {
      sum += cs.sum;
      count += cs.count;
    }
    run.many_models = run.many_models || slot != run.models.slot[0];
  }
  run.mean_cost = count ? sum / (double)count : 0.0;
  run.models.stride = (long long)stride;
  run.ec = fb.ec.as<float>() + (run.many_models ? 0 : (size_t)run.models.slot[0] * stride);
  return TRG_OK;
}

// A refresh only: the old keys, still in the retained solve's array (run.old, as field_begin found it), gathered
// through the node map into a buffer of their own -- before field_work_arrays regrows anything.
TrgStatus field_carry(TrgEngine *e, FieldRun &run) {
  if (!run.rq.refresh) return TRG_OK;
  FieldBufs &fb = *e->field;
  hipStream_t s = e->s_main;
  const FieldDev &F = run.F;
  TrgStatus st;
  if ((st = field_grow(e, fb.key0, ((size_t)F.N + 4) * sizeof(unsigned long long))) != TRG_OK) return st;
  if ((st = field_grow(e, fb.node_map, (size_t)F.V * sizeof(int))) != TRG_OK) return st;
  if ((st = field_grow(e, fb.carried, TRG_FIELD_BATCH_MAX * sizeof(int))) != TRG_OK) return st;
  HIPCHK(e, fb.h_carried.ensure(TRG_FIELD_BATCH_MAX));
  HIPCHK(e, hipMemcpyAsync(fb.node_map.p, run.rq.new2old, (size_t)F.V * sizeof(int), hipMemcpyHostToDevice, s));
  launch_field_carry(run.old.key, run.old.V, fb.node_map.as<int>(), F.V, F.m, fb.key0.as<unsigned long long>(), s);
  HIPCHK(e, hipGetLastError());
  return TRG_OK;
}

// work arrays, per item, and the kernels' view of them
TrgStatus field_work_arrays(TrgEngine *e, FieldRun &run) {
  FieldBufs &fb = *e->field;
  const size_t nV = (size_t)run.F.N + 4;
  TrgStatus st;
  if ((st = field_grow(e, fb.key, nV * sizeof(unsigned long long))) != TRG_OK) return st;
  for (DevArr *a : {&fb.q[0], &fb.q[1], &fb.far[0], &fb.far[1], &fb.stamp_near, &fb.stamp_far, &fb.parent, &fb.cost,
                    &fb.hops})
    if ((st = field_grow(e, *a, nV * sizeof(int))) != TRG_OK) return st;
  if ((st = ensure_bytes(e, fb.ctrl, sizeof(FieldCtrl))) != TRG_OK) return st;
  FieldDev &F = run.F;
  F.rowptr = run.G.rowptr;
  F.col = run.G.col;
  F.ec = run.ec;
  F.key = fb.key.as<unsigned long long>();
  for (int i = 0; i < 2; ++i) {
    F.q[i] = fb.q[i].as<int>();
    F.far[i] = fb.far[i].as<int>();
  }
  F.stamp_near = fb.stamp_near.as<int>();
  F.stamp_far = fb.stamp_far.as<unsigned>();
  F.parent = fb.parent.as<int>();
  F.ctrl = fb.ctrl.as<FieldCtrl>();
  return TRG_OK;
}

// what the passes read beside the graph: the target list and the sets
TrgStatus field_uploads(TrgEngine *e, FieldRun &run) {
  FieldBufs &fb = *e->field;
  const FieldRequest &rq = run.rq;
  FieldDev &F = run.F;
  hipStream_t s = e->s_main;
  if (rq.settle != TRG_FIELD_SETTLE_NONE || run.gather) {  // the target list: read by the settle step, the gather
    const TrgStatus st = field_grow(e, fb.targets, (size_t)rq.n_targets * sizeof(int));
    if (st != TRG_OK) return st;
    HIPCHK(e, hipMemcpyAsync(fb.targets.p, rq.targets, (size_t)rq.n_targets * sizeof(int), hipMemcpyHostToDevice, s));
  }
  if (rq.set_ptr) {  // the sets, uploaded once per solve
    FieldSets &S = run.sets;
    TrgStatus st;
    if ((st = field_grow(e, fb.set_ptr, ((size_t)F.m + 1) * sizeof(int))) != TRG_OK) return st;
    if ((st = field_grow(e, fb.set_ids, (size_t)S.n * sizeof(int))) != TRG_OK) return st;
    HIPCHK(e, hipMemcpyAsync(fb.set_ptr.p, rq.set_ptr, ((size_t)F.m + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(fb.set_ids.p, rq.set_ids, (size_t)S.n * sizeof(int), hipMemcpyHostToDevice, s));
    S.ptr = fb.set_ptr.as<int>();
    S.ids = fb.set_ids.as<int>();
    fb.h_set_ptr.assign(rq.set_ptr, rq.set_ptr + F.m + 1);
    fb.h_set_ids.assign(rq.set_ids, rq.set_ids + S.n);
    if (rq.set_cost0) {
      if ((st = field_grow(e, fb.set_cost0, (size_t)S.n * sizeof(unsigned))) != TRG_OK) return st;
      HIPCHK(e, hipMemcpyAsync(fb.set_cost0.p, run.cost0.data(), (size_t)S.n * sizeof(unsigned),
                               hipMemcpyHostToDevice, s));
    }
  }
  return TRG_OK;
}

// the bucket width: a fixed multiple of the mean edge cost
float field_delta(const TrgEngine *e, const FieldRun &run) {
  return run.mean_cost > 0.0 ? (float)(e->field_delta_scale * run.mean_cost) : 0.0f;
}

// the rounds of one pass from round 0 on, enqueued in batches, until no work is left
TrgStatus field_rounds(TrgEngine *e, FieldRun &run, const FieldSettle *under) {
  FieldBufs &fb = *e->field;
  const FieldDev &F = run.F;
  hipStream_t s = e->s_main;
  const long long cap = 4LL * F.N + 64;
  for (int round = 0;;) {
    for (int i = 0; i < FIELD_BATCH; ++i, ++round)
      launch_field_round(F, round, s, under, run.model_table(), run.rq.risk);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(fb.h_state, &F.ctrl->s, sizeof(FieldState), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    run.syncs++;
    if (fb.h_state->overflow) return e->fail(TRG_ERR_DEVICE, "cost field: queue overflow");
    if (fb.h_state->work == 0) break;
    if (fb.h_state->rounds >= cap) return e->fail(TRG_ERR_DEVICE, "cost field did not converge");
  }
  run.rounds += fb.h_state->rounds;
  return TRG_OK;
}

// sweeps enqueued between two looks at a forest pass's pinned "moved" word
constexpr int FIELD_OWNER_BATCH = 8;
static_assert(FIELD_OWNER_SWEEPS_MAX % FIELD_OWNER_BATCH == 0, "a forest pass looks after whole batches");

// The jumping sweeps after a forest's begin launch (which zeroed `changed`), in batches, until one moves nothing:
// one host wait per batch, on the pinned word `h_moved`.  -> the sweep count, which says where the ancestors lie
// (F.q[sweeps & 1]).  `what` names the pass in the error of one that does not end.
TrgStatus field_forest_sweeps(TrgEngine *e, const FieldDev &F, int *changed, int *h_moved, const char *what,
                              int &sweeps) {
  hipStream_t s = e->s_main;
  for (sweeps = 0;;) {
    for (int i = 0; i < FIELD_OWNER_BATCH; ++i, ++sweeps) launch_field_owner_sweep(F, sweeps, changed, s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(h_moved, changed + sweeps - 1, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    if (*h_moved == 0) return TRG_OK;
    if (sweeps >= FIELD_OWNER_SWEEPS_MAX) return e->fail(TRG_ERR_DEVICE, std::string(what) + " did not end");
  }
}

// One jump over the forest in F.parent (the owner pass, a refresh's anchors; trg_field.hip): the begin launch for
// `single` sources or marked members and `key0`, the jumping sweeps in the idle near queues until a sweep moves
// nothing -- about log2 of the longest chain of them, one host wait per FIELD_OWNER_BATCH sweeps -- then `end`'s
// launch, given the sweep count.
template <typename End>
TrgStatus field_forest_pass(TrgEngine *e, const FieldDev &F, const FieldSources *single,
                            const unsigned long long *key0, const char *what, int &syncs, int &sweeps, End end) {
  FieldBufs &fb = *e->field;
  if (const TrgStatus st = field_grow(e, fb.own_changed, FIELD_OWNER_SWEEPS_MAX * sizeof(int)); st != TRG_OK) return st;
  HIPCHK(e, fb.h_changed.ensure(1));
  int *changed = fb.own_changed.as<int>();
  launch_field_forest_begin(F, single, key0, changed, e->s_main);
  const TrgStatus st = field_forest_sweeps(e, F, changed, fb.h_changed, what, sweeps);
  syncs += sweeps / FIELD_OWNER_BATCH;  // (one wait per batch)
  if (st != TRG_OK) return st;
  end(sweeps);
  HIPCHK(e, hipGetLastError());
  return TRG_OK;
}

// The owner pass of a set solve whose parent sweep ran ("Source sets"): the forest of the
// parents, then S.owner, whose m x V words are allocated here.
TrgStatus field_owner_pass(TrgEngine *e, const FieldDev &F, FieldSets &S, int &syncs, int &sweeps) {
  FieldBufs &fb = *e->field;
  if (const TrgStatus st = field_grow(e, fb.owner, ((size_t)F.N + 4) * sizeof(int)); st != TRG_OK) return st;
  S.owner = fb.owner.as<int>();
  return field_forest_pass(e, F, nullptr, nullptr, "cost field sets: the owner pass", syncs, sweeps,
                           [&](int n) { launch_field_owner_end(F, S, n, e->s_main); });
}

// One anchor of a refresh ("Refresh"): the forest of the supporters; the first leaves the
// anchored keys in key0 and counts them, the second cuts every key that is no longer key0's.
TrgStatus field_anchor(TrgEngine *e, FieldRun &run, bool first) {
  FieldBufs &fb = *e->field;
  const FieldDev &F = run.F;
  unsigned long long *key0 = fb.key0.as<unsigned long long>();
  int sweeps = 0;
  return field_forest_pass(e, F, run.rq.set_ptr ? nullptr : &run.sources, first ? nullptr : key0,
                           "cost field refresh: an anchor", run.syncs, sweeps, [&](int n) {
                             launch_field_anchor_end(F, n, first ? key0 : nullptr,
                                                     first ? fb.carried.as<int>() : nullptr, e->s_main);
                           });
}

// Near-far rounds; pass 1 finds the least costs, pass 2 the hops over the tight edges (trg_field.hip).  A solve
// starts each pass cold, from the sources.  A refresh starts pass 1 from the carried keys, anchored to the new graph,
// and pass 2 from the keys that pass 1 left alone, anchored again: warm starts both.  The rounds are the same.
TrgStatus field_passes(TrgEngine *e, FieldRun &run) {
  FieldBufs &fb = *e->field;
  const FieldRequest &rq = run.rq;
  FieldDev &F = run.F;
  hipStream_t s = e->s_main;
  const float delta = field_delta(e, run);
  const FieldModels *models = run.model_table();
  const FieldSettle under{fb.targets.as<int>(), rq.n_targets, rq.settle};
  const FieldSets *sets = rq.set_ptr ? &run.sets : nullptr;
  const unsigned *cost0 = rq.set_cost0 ? fb.set_cost0.as<unsigned>() : nullptr;
  TrgStatus st;
  if (run.bounded) launch_field_bounds(F, run.budgets, s);
  for (int pass = 0; pass < 2; ++pass) {
    // the bounds act in pass 1 only: it ends with the keys above them removed, and no pass-2 extension matches
    // the tight word of a node without a key
    const bool under_bounds = run.bounded && pass == 0;
    F.tight = pass ? fb.cost.as<unsigned>() : nullptr;
    if (!rq.refresh) {
      launch_field_init(F, run.sources, sets, cost0, nullptr, delta, s);
    } else {
      if (pass == 0) {
        launch_field_init(F, run.sources, sets, nullptr, fb.key0.as<unsigned long long>(), delta, s);
        launch_field_supporters(F, s, models, rq.risk);
      }
      if ((st = field_anchor(e, run, pass == 0)) != TRG_OK) return st;
      if (pass == 0)
        HIPCHK(e, hipMemcpyAsync(fb.h_carried, fb.carried.p, (size_t)F.m * sizeof(int), hipMemcpyDeviceToHost, s));
      launch_field_warm_start(F, delta, pass == 1, s, models, rq.risk);
    }
    if ((st = field_rounds(e, run, under_bounds ? &under : nullptr)) != TRG_OK) return st;
    if (under_bounds) {
      launch_field_trim(F, s);
      HIPCHK(e, hipMemcpyAsync(fb.h_bound, F.ctrl->bound, (size_t)F.m * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    }
    if (pass == 0) launch_field_cost_bits(F, fb.cost.as<unsigned>(), s);
  }
  return TRG_OK;
}

// The end of every call that timed device work between the engine's two events (created by field_begin, so there
// for every retained solve): the event time, the host waits and the wall time into `info`.
TrgStatus field_timing(TrgEngine *e, TrgFieldInfo *info, int syncs, Clock::time_point t_total) {
  FieldBufs &fb = *e->field;
  float ms_dev = 0.0f;
  HIPCHK(e, hipEventElapsedTime(&ms_dev, fb.t0, fb.t1));
  info->host_syncs = syncs;
  info->ms_device = ms_dev;
  info->ms_total = ms_since(t_total);
  return TRG_OK;
}

// finish, gather, the copies of only what was asked for, `info`, and the retained-solve record
TrgStatus field_outputs(TrgEngine *e, FieldRun &run) {
  FieldBufs &fb = *e->field;
  const FieldRequest &rq = run.rq;
  const FieldDev &F = run.F;
  hipStream_t s = e->s_main;
  const int m = F.m;
  const size_t nN = (size_t)F.N, nat = (size_t)m * rq.n_targets;
  const bool parents = rq.parent != nullptr || run.owners;  // (owners follow parents)
  launch_field_finish(F, fb.cost.as<float>(), fb.hops.as<int>(), parents, s, run.model_table(), rq.risk);
  TrgStatus st;
  int sweeps = 0;
  if (run.owners && (st = field_owner_pass(e, F, run.sets, run.syncs, sweeps)) != TRG_OK) return st;
  if (run.gather) {
    if ((st = field_grow(e, fb.cost_at, nat * sizeof(float))) != TRG_OK) return st;
    if ((st = field_grow(e, fb.hops_at, nat * sizeof(int))) != TRG_OK) return st;
    if (rq.owner_at && (st = field_grow(e, fb.owner_at, nat * sizeof(int))) != TRG_OK) return st;
    float *d_cost_at = rq.cost_at ? fb.cost_at.as<float>() : nullptr;
    int *d_hops_at = rq.hops_at ? fb.hops_at.as<int>() : nullptr;
    launch_field_gather(F, rq.set_ptr ? &run.sets : nullptr, fb.targets.as<int>(), rq.n_targets, d_cost_at,
                        d_hops_at, rq.owner_at ? fb.owner_at.as<int>() : nullptr, s);
  }
  if (rq.owned) {
    if ((st = field_grow(e, fb.owned, (size_t)run.sets.n * sizeof(int))) != TRG_OK) return st;
    launch_field_owned(F, run.sets, fb.owned.as<int>(), s);
  }
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipEventRecord(fb.t1, s));
  HIPCHK(e, hipMemcpyAsync(fb.h_reached, F.ctrl->reached, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, s));
  if (rq.cost) HIPCHK(e, hipMemcpyAsync(rq.cost, fb.cost.p, nN * sizeof(float), hipMemcpyDeviceToHost, s));
  if (rq.hops) HIPCHK(e, hipMemcpyAsync(rq.hops, fb.hops.p, nN * sizeof(int), hipMemcpyDeviceToHost, s));
  if (rq.parent) HIPCHK(e, hipMemcpyAsync(rq.parent, fb.parent.p, nN * sizeof(int), hipMemcpyDeviceToHost, s));
  if (run.gather && rq.cost_at)
    HIPCHK(e, hipMemcpyAsync(rq.cost_at, fb.cost_at.p, nat * sizeof(float), hipMemcpyDeviceToHost, s));
  if (run.gather && rq.hops_at)
    HIPCHK(e, hipMemcpyAsync(rq.hops_at, fb.hops_at.p, nat * sizeof(int), hipMemcpyDeviceToHost, s));
  if (rq.owner) HIPCHK(e, hipMemcpyAsync(rq.owner, fb.owner.p, nN * sizeof(int), hipMemcpyDeviceToHost, s));
  if (run.gather && rq.owner_at)
    HIPCHK(e, hipMemcpyAsync(rq.owner_at, fb.owner_at.p, nat * sizeof(int), hipMemcpyDeviceToHost, s));
  if (rq.owned)
    HIPCHK(e, hipMemcpyAsync(rq.owned, fb.owned.p, (size_t)run.sets.n * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  run.syncs++;
  long long reached = 0;
  for (int k = 0; k < m; ++k) {
    reached += fb.h_reached[k];
    if (rq.sources_out) rq.sources_out[k] = run.sources.id[k];
    if (rq.reached_out) rq.reached_out[k] = fb.h_reached[k];
    if (rq.bound_out) rq.bound_out[k] = bits_float(run.bounded ? fb.h_bound[k] : FIELD_INF_BITS);
    if (rq.carried_out) rq.carried_out[k] = fb.h_carried[k];
  }
  run.info->source = run.sources.id[0];
  run.info->reached = (int32_t)reached;
  run.info->rounds = run.rounds;
  fb.last = FieldBufs::Last{e->graph_version, F, run.G.w, run.G.dist, run.sources, parents,
                            rq.set_ptr ? std::optional<FieldSets>(run.sets) : std::nullopt, run.owners};
  fb.last.F.tight = nullptr;  // (its array holds the cost output now)
  fb.last.bounded = run.bounded;
  fb.last.risk = rq.risk;
  fb.last.seeded = rq.set_cost0 != nullptr;
  if (rq.models) fb.last.pairs.assign(rq.models, rq.models + m);
  fb.last.models = run.models;
  fb.last.many = run.many_models;
  if (rq.zone_ptr) fb.last.zones.assign(m, rq.zone_ptr, rq.zones);
  e->field_map.state = NodeMap::IDENTITY;  // update_graph takes the node map on from here
  return field_timing(e, run.info, run.syncs, run.t_total);
}

TrgStatus field_solve(TrgEngine *e, const FieldRequest &rq, TrgFieldInfo *info) {
  FieldRun run{rq, info, Clock::now()};
  TrgStatus st = plan_prepare(e);  // graph present, CSR rows and node grid current
  if (st != TRG_OK) return st;
  if (rq.refresh && (st = field_check_refresh(e, run)) != TRG_OK) return st;
  if ((st = field_check_request(e, run)) != TRG_OK || rq.resolve_only) return st;
  for (const auto phase : {field_begin, field_graph, field_edge_costs, field_carry, field_work_arrays, field_uploads,
                           field_passes, field_outputs})
    if ((st = phase(e, run)) != TRG_OK) return st;
  return TRG_OK;
}

// The field entries' common frame: entry() with `info` defaulted, zeroed and without a source for `body(info)`;
// `call` is the entry's message prefix.
template <typename Body>
TrgStatus field_entry(TrgEngine *e, TrgFieldInfo *info, const char *call, Body body) {
  return entry(e, call, DEVICE, [&] {
    TrgFieldInfo local{};
    TrgFieldInfo *out = info ? info : &local;
    *out = TrgFieldInfo{};
    out->source = -1;
    return body(out);
  });
}

static_assert(sizeof(TrgRouteInfo) == sizeof(FieldRouteInfo) && offsetof(TrgRouteInfo, num_nodes) == 0 &&
                  offsetof(TrgRouteInfo, cost) == offsetof(FieldRouteInfo, cost) &&
                  offsetof(TrgRouteInfo, path_length) == offsetof(FieldRouteInfo, path_length) &&
                  offsetof(TrgRouteInfo, avg_risk) == offsetof(FieldRouteInfo, avg_risk),
              "the kernels' and the header's route info differ");

struct RouteRequest {
  int32_t n;
  const int32_t *field, *target;  // n each
  int32_t *offsets;               // n + 1
  int32_t *node_ids;              // cap, may be nullptr
  float *xyz;                     // cap x 3, may be nullptr
  int32_t cap;
  TrgRouteInfo *infos;            // n, may be nullptr
};

// Routes of the retained solve ("Routes"): lengths on the device, their clipped prefix sum
// on the host, then the walk.  Two host waits with ids or positions, one without.
TrgStatus field_routes(TrgEngine *e, const RouteRequest &rq, TrgFieldInfo *info) {
  const auto t_total = Clock::now();
  if (rq.n < 0) return e->fail(TRG_ERR_INVALID_ARG, "cost field routes: n_routes < 0");
  if (rq.cap < 0) return e->fail(TRG_ERR_INVALID_ARG, "cost field routes: cap < 0");
  FieldBufs::Last *last;
  TrgStatus st = field_retained(e, "cost field routes", last);
  if (st != TRG_OK) return st;
  FieldBufs &fb = *e->field;
  const FieldDev &F = last->F;
  if (rq.n > 0 && (!rq.field || !rq.target || !rq.offsets))
    return e->fail(TRG_ERR_INVALID_ARG, "cost field routes: null route_field, route_target or offsets");
  for (int r = 0; r < rq.n; ++r) {
    if (rq.field[r] < 0 || rq.field[r] >= F.m)
      return e->fail(TRG_ERR_INVALID_ARG, "cost field routes: field " + std::to_string(rq.field[r]) + " of route " +
                                              std::to_string(r) + " out of range (the solve has " +
                                              std::to_string(F.m) + ")");
    if (rq.target[r] < 0 || rq.target[r] >= F.V)
      return e->fail(TRG_ERR_INVALID_ARG, "cost field routes: target " + std::to_string(rq.target[r]) + " of route " +
                                              std::to_string(r) + " out of range");
  }
  if (rq.n == 0) {
    if (rq.offsets) rq.offsets[0] = 0;
    info->ms_total = ms_since(t_total);
    return TRG_OK;
  }
  const bool want_ids = (rq.node_ids || rq.xyz) && rq.cap > 0;
  const size_t n = (size_t)rq.n;
  if ((st = field_grow(e, fb.route_field, n * sizeof(int))) != TRG_OK) return st;
  if ((st = field_grow(e, fb.route_target, n * sizeof(int))) != TRG_OK) return st;
  if ((st = field_grow(e, fb.route_info, n * sizeof(FieldRouteInfo))) != TRG_OK) return st;
  hipStream_t s = e->s_main;
  int syncs = 0;
  HIPCHK(e, hipMemcpyAsync(fb.route_field.p, rq.field, n * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(e, hipMemcpyAsync(fb.route_target.p, rq.target, n * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(e, hipEventRecord(fb.t0, s));
  if (!last->parents) {
    launch_field_parents_late(F, s, last->many ? &last->models : nullptr, last->risk);
    HIPCHK(e, hipGetLastError());
    last->parents = true;
  }
  if (last->sets && !last->owners) {  // a walk of a set solve ends at its target's owner
    int sweeps = 0;
    if ((st = field_owner_pass(e, F, *last->sets, syncs, sweeps)) != TRG_OK) return st;
    last->owners = true;
    info->rounds = sweeps;
  }
  const int *d_field = fb.route_field.as<int>(), *d_target = fb.route_target.as<int>();
  std::vector<int32_t> ids;
  int total = 0;
  std::fill(rq.offsets, rq.offsets + n + 1, 0);
  if (want_ids) {
    if ((st = field_grow(e, fb.route_len, n * sizeof(int))) != TRG_OK) return st;
    if ((st = field_grow(e, fb.route_off, (n + 1) * sizeof(int))) != TRG_OK) return st;
    launch_field_route_len(F, d_field, d_target, rq.n, fb.route_len.as<int>(), s);
    HIPCHK(e, hipGetLastError());
    std::vector<int32_t> len(n);
    HIPCHK(e, hipMemcpyAsync(len.data(), fb.route_len.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    syncs++;
    // a route that no longer fits is truncated, later routes are empty ranges
    for (size_t r = 0; r < n; ++r)
      rq.offsets[r + 1] = (int32_t)std::min<long long>((long long)rq.offsets[r] + len[r], rq.cap);
    total = rq.offsets[n];
    if ((st = field_grow(e, fb.route_ids, ((size_t)total + 4) * sizeof(int))) != TRG_OK) return st;
    HIPCHK(e, hipMemcpyAsync(fb.route_off.p, rq.offsets, (n + 1) * sizeof(int), hipMemcpyHostToDevice, s));
  }
  std::vector<FieldRouteInfo> infos(n);
  const int *d_off = want_ids ? fb.route_off.as<int>() : nullptr;
  int *d_ids = want_ids ? fb.route_ids.as<int>() : nullptr;
  launch_field_route_walk(F, last->w, last->dist, d_field, d_target, rq.n, d_off, d_ids,
                          fb.route_info.as<FieldRouteInfo>(), last->sources, last->sets ? &*last->sets : nullptr, s,
                          last->many ? &last->models : nullptr, last->risk);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipEventRecord(fb.t1, s));
  int32_t *ids_out = rq.node_ids;
  if (total > 0) {
    if (!ids_out) {
      ids.resize((size_t)total);
      ids_out = ids.data();
    }
    HIPCHK(e, hipMemcpyAsync(ids_out, fb.route_ids.p, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(e, hipMemcpyAsync(infos.data(), fb.route_info.p, n * sizeof(FieldRouteInfo), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  syncs++;
  for (size_t r = 0; r < n; ++r)
    if (infos[r].num_nodes == FIELD_ROUTE_BROKEN)
      return e->fail(TRG_ERR_DEVICE, "cost field routes: the walk of route " + std::to_string(r) +
                                         " did not end at its field's source");
  if (rq.infos)
    for (size_t r = 0; r < n; ++r)
      rq.infos[r] = TrgRouteInfo{infos[r].num_nodes, infos[r].cost, infos[r].path_length, infos[r].avg_risk};
  if (rq.xyz)
    for (int i = 0; i < total; ++i) {
      const int id = ids_out[i];
      if (id < 0 || id >= F.V) return e->fail(TRG_ERR_DEVICE, "cost field routes: a walk left the graph");
      rq.xyz[3 * i] = e->nx[id];
      rq.xyz[3 * i + 1] = e->ny[id];
      rq.xyz[3 * i + 2] = e->nz[id];
    }
  return field_timing(e, info, syncs, t_total);
}

// The reached list of one field of the retained solve: count, scan, emit on the device; the count comes back
// first, then as many entries as were written.
TrgStatus field_reached(TrgEngine *e, int32_t field, int32_t *node_ids, float *cost, int32_t *hops, int32_t cap,
                        int32_t *n_out, TrgFieldInfo *info) {
  const auto t_total = Clock::now();
  if (cap < 0) return e->fail(TRG_ERR_INVALID_ARG, "cost field reached: cap < 0");
  FieldBufs::Last *last;
  TrgStatus st = field_retained(e, "cost field reached", last);
  if (st != TRG_OK) return st;
  FieldBufs &fb = *e->field;
  const FieldDev &F = last->F;
  if (field < 0 || field >= F.m)
    return e->fail(TRG_ERR_INVALID_ARG, "cost field reached: field " + std::to_string(field) +
                                            " out of range (the solve has " + std::to_string(F.m) + ")");
  const bool want = cap > 0 && (node_ids || cost || hops);
  const int room = want ? std::min<int>(cap, F.V) : 0;
  const size_t nb = ((size_t)F.V + 255) / 256;
  if ((st = field_grow(e, fb.list_counts, (nb + 1) * sizeof(int))) != TRG_OK) return st;
  if ((st = field_grow(e, fb.list_off, (nb + 1) * sizeof(int))) != TRG_OK) return st;
  if ((st = field_grow(e, fb.list_tmp, (nb / 2048 + 8) * sizeof(int))) != TRG_OK) return st;
  if (node_ids && (st = field_grow(e, fb.list_ids, ((size_t)room + 4) * sizeof(int))) != TRG_OK) return st;
  if (cost && (st = field_grow(e, fb.list_cost, ((size_t)room + 4) * sizeof(float))) != TRG_OK) return st;
  if (hops && (st = field_grow(e, fb.list_hops, ((size_t)room + 4) * sizeof(int))) != TRG_OK) return st;
  hipStream_t s = e->s_main;
  int syncs = 0;
  HIPCHK(e, hipEventRecord(fb.t0, s));
  launch_field_reached_list(F, field, fb.list_counts.as<int>(), fb.list_off.as<int>(), fb.list_tmp.as<int>(), room,
                            node_ids ? fb.list_ids.as<int>() : nullptr, cost ? fb.list_cost.as<float>() : nullptr,
                            hops ? fb.list_hops.as<int>() : nullptr, s);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipEventRecord(fb.t1, s));
  int total = 0;
  HIPCHK(e, hipMemcpyAsync(&total, fb.list_off.as<int>() + nb, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  syncs++;
  const size_t n = (size_t)std::min(total, room);
  if (n > 0) {
    if (node_ids) HIPCHK(e, hipMemcpyAsync(node_ids, fb.list_ids.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    if (cost) HIPCHK(e, hipMemcpyAsync(cost, fb.list_cost.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (hops) HIPCHK(e, hipMemcpyAsync(hops, fb.list_hops.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    syncs++;
  }
  if (n_out) *n_out = total;
  info->source = last->sources.id[field];
  info->reached = total;
  return field_timing(e, info, syncs, t_total);
}

// The shape checks that the bounded and the set entry share: the entry's message prefix, its noun for a field, and
// `also`, the refusal of its own that stands between the two (nullptr: none).
TrgStatus field_check_shape(TrgEngine *e, const std::string &call, const char *noun, int32_t m, int32_t n_targets,
                            const char *also = nullptr) {
  if (m < 1 || m > TRG_FIELD_BATCH_MAX)
    return e->fail(TRG_ERR_INVALID_ARG, call + ": a batch of " + std::to_string(m) + " " + noun + " (1.." +
                                            std::to_string(TRG_FIELD_BATCH_MAX) + ")");
  if (also) return e->fail(TRG_ERR_INVALID_ARG, call + ": " + also);
  if (n_targets < 0) return e->fail(TRG_ERR_INVALID_ARG, call + ": n_targets < 0");
  return TRG_OK;
}

// the budget and settle checks that the bounded and the set entry share
TrgStatus field_check_bounds(TrgEngine *e, int32_t m, const float *budget, int32_t settle, const int32_t *targets,
                             int32_t n_targets) {
  if (budget)
    for (int k = 0; k < m; ++k)
      if (!(budget[k] >= 0.0f))
        return e->fail(TRG_ERR_INVALID_ARG, "cost field: the budget of field " + std::to_string(k) +
                                                " is negative or not a number");
  if (settle != TRG_FIELD_SETTLE_NONE && settle != TRG_FIELD_SETTLE_ANY && settle != TRG_FIELD_SETTLE_ALL)
    return e->fail(TRG_ERR_INVALID_ARG, "cost field: settle mode " + std::to_string(settle) + " (0..2)");
  if (settle != TRG_FIELD_SETTLE_NONE && (n_targets == 0 || !targets))
    return e->fail(TRG_ERR_INVALID_ARG, "cost field: settle mode " + std::to_string(settle) + " needs targets");
  return TRG_OK;
}

// the model checks of trg_engine_cost_field_models: a safety factor is a finite number >= 0, a ceiling a number >= 0
TrgStatus field_check_models(TrgEngine *e, int32_t m, const TrgFieldModel *models) {
  for (int k = 0; models && k < m; ++k) {
    if (!(models[k].safety_factor >= 0.0f) || std::isinf(models[k].safety_factor))
      return e->fail(TRG_ERR_INVALID_ARG, "cost field: the safety factor of field " + std::to_string(k) +
                                              " is negative or not finite");
    if (!(models[k].max_weight >= 0.0f))
      return e->fail(TRG_ERR_INVALID_ARG, "cost field: the risk ceiling of field " + std::to_string(k) +
                                              " is negative or not a number");
  }
  return TRG_OK;
}

// the request members that every entry with targets sets, by name
FieldRequest field_request(int32_t m, float *cost, int32_t *hops, int32_t *parent, const int32_t *targets,
                           int32_t n_targets, float *cost_at, int32_t *hops_at, int32_t *reached_out) {
  FieldRequest rq{};
  rq.m = m;
  rq.cost = cost;
  rq.hops = hops;
  rq.parent = parent;
  rq.targets = targets;
  rq.n_targets = n_targets;
  rq.cost_at = cost_at;
  rq.hops_at = hops_at;
  rq.reached_out = reached_out;
  return rq;
}

// the solve behind trg_engine_cost_field_bounded and, without bounds, trg_engine_cost_field_batch (no_info: the caller
// gave no TrgFieldInfo)
TrgStatus cost_field_bounded(TrgEngine *e, int32_t m, const int32_t *source_ids, const float *source_xy,
                             const float *budget, int32_t settle, float *cost, int32_t *hops, int32_t *parent,
                             const int32_t *targets, int32_t n_targets, float *cost_at, int32_t *hops_at,
                             int32_t *sources_out, int32_t *reached_out, float *bound_out, bool no_info,
                             TrgFieldInfo *out) {
  // every output NULL but sources_out: the caller wants the sources resolved, nothing solved
  const bool resolve_only =
      sources_out && !cost && !hops && !parent && !cost_at && !hops_at && !reached_out && !bound_out && no_info;
  if (const TrgStatus st = field_check_shape(e, "cost field", "fields", m, n_targets); st != TRG_OK) return st;
  if (!source_ids && !source_xy) return e->fail(TRG_ERR_INVALID_ARG, "cost field: no sources");
  if (source_ids)
    for (int k = 0; k < m; ++k)
      if (source_ids[k] < -1)
        return e->fail(TRG_ERR_INVALID_ARG, "cost field: source " + std::to_string(k) + " out of range");
  if (const TrgStatus st = field_check_bounds(e, m, budget, settle, targets, n_targets); st != TRG_OK) return st;
  FieldRequest rq = field_request(m, cost, hops, parent, targets, n_targets, cost_at, hops_at, reached_out);
  rq.source_ids = source_ids;
  rq.source_xy = source_xy;
  rq.sources_out = sources_out;
  rq.resolve_only = resolve_only;
  rq.budget = budget;
  rq.settle = settle;
  rq.bound_out = bound_out;
  return field_solve(e, rq, out);
}

// the zone-list checks of trg_engine_cost_field_zones and trg_engine_risk_field_zones (zone_sets.h), under the name
// of the caller; a null zone_ptr: no lists
TrgStatus field_check_zones(TrgEngine *e, const char *who, int32_t m, const int32_t *zone_ptr, const TrgZone *zones) {
  std::string why;
  if (zone_ptr && !zone_sets_check(m, zone_ptr, zones, why))
    return e->fail(TRG_ERR_INVALID_ARG, std::string(who) + ": " + why);
  return TRG_OK;
}

// ... and the one behind trg_engine_cost_field_zones, without zone lists trg_engine_cost_field_seeded, without start
// costs either trg_engine_cost_field_models and, without models, trg_engine_cost_field_sets
TrgStatus cost_field_models(TrgEngine *e, int32_t m, const TrgFieldModel *models, const int32_t *set_ptr,
                            const int32_t *set_ids, const float *set_cost0, const float *budget, int32_t settle, float *cost, int32_t *hops,
                            int32_t *parent, int32_t *owner, const int32_t *targets, int32_t n_targets, float *cost_at,
                            int32_t *hops_at, int32_t *owner_at, int32_t *owned, int32_t *reached_out, float *bound_out,
                            TrgFieldInfo *out, const int32_t *zone_ptr = nullptr, const TrgZone *zones = nullptr) {
  const char *no_sets = !set_ptr || !set_ids ? "null set_ptr or set_ids" : nullptr;
  if (const TrgStatus st = field_check_shape(e, "cost field sets", "sets", m, n_targets, no_sets); st != TRG_OK)
    return st;
  if (const TrgStatus st = field_check_models(e, m, models); st != TRG_OK) return st;
  if (const TrgStatus st = field_check_zones(e, "cost field zones", m, zone_ptr, zones); st != TRG_OK) return st;
  if (const TrgStatus st = field_check_bounds(e, m, budget, settle, targets, n_targets); st != TRG_OK) return st;
  FieldRequest rq = field_request(m, cost, hops, parent, targets, n_targets, cost_at, hops_at, reached_out);
  rq.budget = budget;
  rq.settle = settle;
  rq.bound_out = bound_out;
  rq.set_ptr = set_ptr;
  rq.set_ids = set_ids;
  rq.set_cost0 = set_cost0;
  rq.owner = owner;
  rq.owner_at = owner_at;
  rq.owned = owned;
  rq.models = models;
  rq.zone_ptr = zone_ptr;
  rq.zones = zones;
  return field_solve(e, rq, out);
}

// The solve behind trg_engine_risk_field_zones and, without zone lists, trg_engine_risk_field_sets.
TrgStatus risk_field_sets(TrgEngine *e, int32_t m, const int32_t *zone_ptr, const TrgZone *zones,
                          const int32_t *set_ptr, const int32_t *set_ids, const float *budget, int32_t settle,
                          float *risk, int32_t *hops, int32_t *parent, int32_t *owner, const int32_t *targets,
                          int32_t n_targets, float *risk_at, int32_t *hops_at, int32_t *owner_at, int32_t *owned,
                          int32_t *reached_out, float *bound_out, TrgFieldInfo *out) {
  const char *no_sets = !set_ptr || !set_ids ? "null set_ptr or set_ids" : nullptr;
  if (const TrgStatus st = field_check_shape(e, "risk field sets", "sets", m, n_targets, no_sets); st != TRG_OK)
    return st;
  if (const TrgStatus st = field_check_zones(e, "risk field zones", m, zone_ptr, zones); st != TRG_OK) return st;
  if (const TrgStatus st = field_check_bounds(e, m, budget, settle, targets, n_targets); st != TRG_OK) return st;
  FieldRequest rq = field_request(m, risk, hops, parent, targets, n_targets, risk_at, hops_at, reached_out);
  rq.budget = budget;
  rq.settle = settle;
  rq.bound_out = bound_out;
  rq.set_ptr = set_ptr;
  rq.set_ids = set_ids;
  rq.owner = owner;
  rq.owner_at = owner_at;
  rq.owned = owned;
  rq.zone_ptr = zone_ptr;
  rq.zones = zones;
  rq.risk = true;
  return field_solve(e, rq, out);
}

// The verdicts of a zone set on the current global graph (trg_engine_zone_edges), by the kernels' own rule; the
// retained solve and the edge-cost cache are left alone.
TrgStatus zone_edges(TrgEngine *e, const TrgZone *zones, int32_t n_zones, uint8_t *closed, uint8_t *inside,
                     int32_t *n_closed, int32_t *n_inside) {
  if (n_zones < 0 || n_zones > TRG_ZONES_MAX)
    return e->fail(TRG_ERR_INVALID_ARG, "zone edges: " + std::to_string(n_zones) + " zones (0.." +
                                            std::to_string(TRG_ZONES_MAX) + ")");
  const int32_t ptr[2] = {0, n_zones};
  std::string why;
  if (!zone_sets_check(1, ptr, zones, why)) return e->fail(TRG_ERR_INVALID_ARG, "zone edges: " + why);
  TrgStatus st = plan_prepare(e);  // graph present, CSR rows current
  if (st != TRG_OK) return st;
  DevGraph G;
  if ((st = ensure_dev_graph(e, DEV_NODES | DEV_EDGES, &G)) != TRG_OK) return st;
  if (!e->field) e->field.reset(new FieldBufs());
  FieldBufs &fb = *e->field;
  hipStream_t s = e->s_main;
  if ((st = field_grow(e, fb.zones, (size_t)FIELD_ZONES_MAX * sizeof(FieldZone))) != TRG_OK) return st;
  if ((st = field_grow(e, fb.zone_counts, 2 * sizeof(int))) != TRG_OK) return st;
  if (closed && (st = field_grow(e, fb.zone_closed, (size_t)G.E + 4)) != TRG_OK) return st;
  if (inside && (st = field_grow(e, fb.zone_inside, (size_t)G.V + 4)) != TRG_OK) return st;
  if (n_zones > 0)
    HIPCHK(e, hipMemcpyAsync(fb.zones.p, zones, (size_t)n_zones * sizeof(FieldZone), hipMemcpyHostToDevice, s));
  launch_field_zone_verdicts(G.rowptr, G.col, G.xyz, G.V, G.E, fb.zones.as<FieldZone>(), n_zones,
                             closed ? fb.zone_closed.as<unsigned char>() : nullptr,
                             inside ? fb.zone_inside.as<unsigned char>() : nullptr, fb.zone_counts.as<int>(), s);
  HIPCHK(e, hipGetLastError());
  int counts[2] = {0, 0};
  HIPCHK(e, hipMemcpyAsync(counts, fb.zone_counts.p, sizeof counts, hipMemcpyDeviceToHost, s));
  if (closed && G.E > 0) HIPCHK(e, hipMemcpyAsync(closed, fb.zone_closed.p, (size_t)G.E, hipMemcpyDeviceToHost, s));
  if (inside && G.V > 0) HIPCHK(e, hipMemcpyAsync(inside, fb.zone_inside.p, (size_t)G.V, hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  if (n_closed) *n_closed = counts[0];
  if (n_inside) *n_inside = counts[1];
  return TRG_OK;
}

}  // namespace

extern "C" {

TrgStatus trg_engine_cost_field(TrgEngine *e, int32_t source_id, const float source_xy[2], float *cost,
                                int32_t *hops, int32_t *parent, TrgFieldInfo *info) {
  return field_entry(e, info, "cost field", [&](TrgFieldInfo *out) {
    if (source_id < -1) return e->fail(TRG_ERR_INVALID_ARG, "cost field: source out of range");
    FieldRequest rq{};  // no targets, budgets or settle mode
    rq.m = 1;
    rq.source_ids = &source_id;
    rq.source_xy = source_xy;
    rq.cost = cost;
    rq.hops = hops;
    rq.parent = parent;
    return field_solve(e, rq, out);
  });
}

TrgStatus trg_engine_cost_field_batch(TrgEngine *e, int32_t m, const int32_t *source_ids, const float *source_xy,
                                      float *cost, int32_t *hops, int32_t *parent, const int32_t *targets,
                                      int32_t n_targets, float *cost_at, int32_t *hops_at, int32_t *sources_out,
                                      int32_t *reached_out, TrgFieldInfo *info) {
  return field_entry(e, info, "cost field", [&](TrgFieldInfo *out) {  // the bounded solve without bounds
    return cost_field_bounded(e, m, source_ids, source_xy, nullptr, TRG_FIELD_SETTLE_NONE, cost, hops, parent, targets,
                              n_targets, cost_at, hops_at, sources_out, reached_out, nullptr, !info, out);
  });
}

TrgStatus trg_engine_cost_field_bounded(TrgEngine *e, int32_t m, const int32_t *source_ids, const float *source_xy,
                                        const float *budget, int32_t settle, float *cost, int32_t *hops,
                                        int32_t *parent, const int32_t *targets, int32_t n_targets, float *cost_at,
                                        int32_t *hops_at, int32_t *sources_out, int32_t *reached_out,
                                        float *bound_out, TrgFieldInfo *info) {
  return field_entry(e, info, "cost field", [&](TrgFieldInfo *out) {
    return cost_field_bounded(e, m, source_ids, source_xy, budget, settle, cost, hops, parent, targets, n_targets,
                              cost_at, hops_at, sources_out, reached_out, bound_out, !info, out);
  });
}

TrgStatus trg_engine_cost_field_sets(TrgEngine *e, int32_t m, const int32_t *set_ptr, const int32_t *set_ids,
                                     const float *budget, int32_t settle, float *cost, int32_t *hops, int32_t *parent,
                                     int32_t *owner, const int32_t *targets, int32_t n_targets, float *cost_at,
                                     int32_t *hops_at, int32_t *owner_at, int32_t *owned, int32_t *reached_out,
                                     float *bound_out, TrgFieldInfo *info) {
  return field_entry(e, info, "cost field sets", [&](TrgFieldInfo *out) {
    return cost_field_models(e, m, nullptr, set_ptr, set_ids, nullptr, budget, settle, cost, hops, parent, owner, targets,
                             n_targets, cost_at, hops_at, owner_at, owned, reached_out, bound_out, out);
  });
}

TrgStatus trg_engine_cost_field_models(TrgEngine *e, int32_t m, const TrgFieldModel *models, const int32_t *set_ptr,
                                       const int32_t *set_ids, const float *budget, int32_t settle, float *cost,
                                       int32_t *hops, int32_t *parent, int32_t *owner, const int32_t *targets,
                                       int32_t n_targets, float *cost_at, int32_t *hops_at, int32_t *owner_at,
                                       int32_t *owned, int32_t *reached_out, float *bound_out, TrgFieldInfo *info) {
  return field_entry(e, info, "cost field sets", [&](TrgFieldInfo *out) {
    return cost_field_models(e, m, models, set_ptr, set_ids, nullptr, budget, settle, cost, hops, parent, owner,
                             targets, n_targets, cost_at, hops_at, owner_at, owned, reached_out, bound_out, out);
  });
}

TrgStatus trg_engine_cost_field_seeded(TrgEngine *e, int32_t m, const TrgFieldModel *models, const int32_t *set_ptr,
                                       const int32_t *set_ids, const float *set_cost0, const float *budget,
                                       int32_t settle, float *cost, int32_t *hops, int32_t *parent, int32_t *owner,
                                       const int32_t *targets, int32_t n_targets, float *cost_at, int32_t *hops_at,
                                       int32_t *owner_at, int32_t *owned, int32_t *reached_out, float *bound_out,
                                       TrgFieldInfo *info) {
  return field_entry(e, info, "cost field sets", [&](TrgFieldInfo *out) {
    return cost_field_models(e, m, models, set_ptr, set_ids, set_cost0, budget, settle, cost, hops, parent, owner,
                             targets, n_targets, cost_at, hops_at, owner_at, owned, reached_out, bound_out, out);
  });
}

TrgStatus trg_engine_cost_field_zones(TrgEngine *e, int32_t m, const TrgFieldModel *models, const int32_t *zone_ptr,
                                      const TrgZone *zones, const int32_t *set_ptr, const int32_t *set_ids,
                                      const float *set_cost0, const float *budget, int32_t settle, float *cost,
                                      int32_t *hops, int32_t *parent, int32_t *owner, const int32_t *targets,
                                      int32_t n_targets, float *cost_at, int32_t *hops_at, int32_t *owner_at,
                                      int32_t *owned, int32_t *reached_out, float *bound_out, TrgFieldInfo *info) {
  return field_entry(e, info, "cost field zones", [&](TrgFieldInfo *out) {
    return cost_field_models(e, m, models, set_ptr, set_ids, set_cost0, budget, settle, cost, hops, parent, owner,
                             targets, n_targets, cost_at, hops_at, owner_at, owned, reached_out, bound_out, out,
                             zone_ptr, zones);
  });
}

TrgStatus trg_engine_zone_edges(TrgEngine *e, const TrgZone *zones, int32_t n_zones, uint8_t *closed, uint8_t *inside,
                                int32_t *n_closed, int32_t *n_inside) {
  return entry(e, "zone edges", DEVICE,
               [&] { return zone_edges(e, zones, n_zones, closed, inside, n_closed, n_inside); });
}

TrgStatus trg_engine_risk_field_sets(TrgEngine *e, int32_t m, const int32_t *set_ptr, const int32_t *set_ids,
                                     const float *budget, int32_t settle, float *risk, int32_t *hops, int32_t *parent,
                                     int32_t *owner, const int32_t *targets, int32_t n_targets, float *risk_at,
                                     int32_t *hops_at, int32_t *owner_at, int32_t *owned, int32_t *reached_out,
                                     float *bound_out, TrgFieldInfo *info) {
  return field_entry(e, info, "risk field sets", [&](TrgFieldInfo *out) {
    return risk_field_sets(e, m, nullptr, nullptr, set_ptr, set_ids, budget, settle, risk, hops, parent, owner, targets,
                           n_targets, risk_at, hops_at, owner_at, owned, reached_out, bound_out, out);
  });
}

TrgStatus trg_engine_risk_field_zones(TrgEngine *e, int32_t m, const int32_t *zone_ptr, const TrgZone *zones,
                                      const int32_t *set_ptr, const int32_t *set_ids, const float *budget,
                                      int32_t settle, float *risk, int32_t *hops, int32_t *parent, int32_t *owner,
                                      const int32_t *targets, int32_t n_targets, float *risk_at, int32_t *hops_at,
                                      int32_t *owner_at, int32_t *owned, int32_t *reached_out, float *bound_out,
                                      TrgFieldInfo *info) {
  return field_entry(e, info, "risk field zones", [&](TrgFieldInfo *out) {
    return risk_field_sets(e, m, zone_ptr, zones, set_ptr, set_ids, budget, settle, risk, hops, parent, owner, targets,
                           n_targets, risk_at, hops_at, owner_at, owned, reached_out, bound_out, out);
  });
}

TrgStatus trg_engine_cost_field_refresh(TrgEngine *e, const int32_t *new2old, int32_t n_map, float *cost,
                                        int32_t *hops, int32_t *parent, const int32_t *targets, int32_t n_targets,
                                        float *cost_at, int32_t *hops_at, int32_t *owner, int32_t *owner_at,
                                        int32_t *sources_out, int32_t *reached_out, int32_t *carried_out,
                                        TrgFieldInfo *info) {
  return field_entry(e, info, "cost field refresh", [&](TrgFieldInfo *out) {
    // (m and the sources or sets are the retained solve's: field_check_refresh)
    FieldRequest rq = field_request(0, cost, hops, parent, targets, n_targets, cost_at, hops_at, reached_out);
    rq.refresh = true;
    rq.new2old = new2old;
    rq.n_map = n_map;
    rq.owner = owner;
    rq.owner_at = owner_at;
    rq.sources_out = sources_out;
    rq.carried_out = carried_out;
    return field_solve(e, rq, out);
  });
}

TrgStatus trg_engine_risk_field_refresh(TrgEngine *e, const int32_t *new2old, int32_t n_map, float *risk,
                                        int32_t *hops, int32_t *parent, const int32_t *targets, int32_t n_targets,
                                        float *risk_at, int32_t *hops_at, int32_t *owner, int32_t *owner_at,
                                        int32_t *sources_out, int32_t *reached_out, int32_t *carried_out,
                                        TrgFieldInfo *info) {
  return field_entry(e, info, "risk field refresh", [&](TrgFieldInfo *out) {
    FieldRequest rq = field_request(0, risk, hops, parent, targets, n_targets, risk_at, hops_at, reached_out);
    rq.refresh = true;
    rq.new2old = new2old;
    rq.n_map = n_map;
    rq.owner = owner;
    rq.owner_at = owner_at;
    rq.sources_out = sources_out;
    rq.carried_out = carried_out;
    rq.risk = true;  // (the objective this entry refreshes: field_check_refresh)
    return field_solve(e, rq, out);
  });
}

TrgStatus trg_engine_field_reached(TrgEngine *e, int32_t field, int32_t *node_ids, float *cost, int32_t *hops,
                                   int32_t cap, int32_t *n_out, TrgFieldInfo *info) {
  return field_entry(e, info, "cost field reached", [&](TrgFieldInfo *out) {
    return field_reached(e, field, node_ids, cost, hops, cap, n_out, out);
  });
}

TrgStatus trg_engine_field_routes(TrgEngine *e, int32_t n_routes, const int32_t *route_field,
                                  const int32_t *route_target, int32_t *offsets, int32_t *node_ids, float *xyz,
                                  int32_t cap, TrgRouteInfo *infos, TrgFieldInfo *info) {
  return field_entry(e, info, "cost field routes", [&](TrgFieldInfo *out) {
    const RouteRequest rq{n_routes, route_field, route_target, offsets, node_ids, xyz, cap, infos};
    return field_routes(e, rq, out);
  });
}

}  // extern "C"
