// trg_field_tiled.inc -- kernels of the cost field across tiles (DESIGN.md section 7, "Cost fields across tiles") and of
// the risk field across tiles ("Risk fields across tiles": the same kernels on the edge risks of the solve graph, the
// parent sweep and the route walk in their RISK form); part of trg_field.hip, whose round kernels run on the solve
// graph built here as they are.
//
// The solve graph of a rank: its V local nodes, then its G ghosts -- the distinct other ends of this tile's cross
// edges, in ascending global id.  The ghost table is a flag per GLOBAL node and the exclusive scan of the flags
// (ghost_off), which sorts, uniques and looks up in one: the ghost index of global id g is ghost_off[g] where
// ghost_flag[g] is set.  Local rows keep their order with columns as solve-graph indices; ghost j's row holds the
// reverse of every cross edge that names it, with that edge's weight and length (one record serves both directions,
// so the costs are the owner's bit for bit).  Ghosts carry the Invalid state in the solve graph's state array, so
// k_field_edge_cost gives every edge INTO a ghost the skip marker: no relaxation here ever writes a ghost's key, it
// only mirrors its owner's (k_tiled_merge).
//
// Every solve starts from source sets ("Source sets across tiles"; a single source is a set of one): k_tiled_seed runs
// over this rank's own entries.  The set call adds, after the parent sweep, the owner pass: k_tiled_forest_begin, the
// jumping sweeps of trg_field.hip, then per exchange k_tiled_owner_merge / _resolve and the publish kernel again;
// k_tiled_output writes the owners beside the fields and k_tiled_owned the counts per entry.  The routes of a finished
// solve ("Routes across tiles"): k_tiled_route_len, k_tiled_route_step and k_tiled_route_end.  Pass 1 of a bounded
// solve ("Bounded fields across tiles"): k_tiled_bound, the bounded form of k_tiled_publish, k_tiled_bound_merge and
// k_tiled_bound_fold around trg_field.hip's BOUNDED round kernels; k_tiled_reached and k_tiled_list_count / _emit list
// a rank's own reached nodes.  A cost model per field ("Cost models across tiles"): the only kernels here that read an
// edge cost, k_tiled_parent and k_tiled_route_step, have a MODELS form that takes the slot of the block's or the route's
// field from a FieldModels table, as trg_field.hip's round kernels do.  The refresh of a retained solve ("Refresh across
// tiles"): k_tiled_carry and k_tiled_refresh_begin bring this rank's keys to the new solve graph, k_tiled_member_recs and
// k_tiled_fill_ghosts are the fill exchange's two ends, k_tiled_anchor_begin / _end an anchor around the owner pass's
// sweeps and step, k_tiled_published_init what a warm pass starts from as published; the passes themselves are
// trg_field.hip's warm start and round kernels.
//
// All kernels: wave64, bounds taken from the arguments, no scalar memory writes, nothing waits on another workgroup.

namespace {

// 16 bytes: what a rank tells the others about a border node whose key dropped
struct TiledRec {
  int field, gid;
  unsigned long long key;
};
static_assert(sizeof(TiledRec) == 16 && sizeof(TiledRec) == FIELD_TILED_REC_BYTES, "record layout");

// Is global id g a node of another tile?  The first half of the ghost lookup, and all that k_tiled_mark can ask: it
// runs before the ghost table exists.
__device__ __forceinline__ bool tiled_foreign(int lo, int V, int Vg, int g) {
  return g >= 0 && g < Vg && (g < lo || g >= lo + V);
}

// The ghost index of global id g on this rank, or -1: an own node, an id out of range, or a node that is no ghost here.
__device__ __forceinline__ int tiled_ghost(const FieldTiled &T, int g) {
  if (!tiled_foreign(T.lo, T.V, T.Vg, g) || !T.ghost_flag[g]) return -1;
  const int j = T.ghost_off[g];
  return j < T.G ? j : -1;
}

// the ghost item that a gathered record names, or -1: a record of this rank's own, or one that names no ghost of it
__device__ __forceinline__ int tiled_rec_item(const FieldDev &F, const FieldTiled &T, const TiledRec &r) {
  const int j = r.field >= 0 && r.field < F.m ? tiled_ghost(T, r.gid) : -1;
  return j < 0 ? -1 : r.field * F.V + T.V + j;
}

// One thread per local row: flags the remote ends of its cross edges in the global table and the row as a border
// row.  (Several rows may flag one ghost: every store writes the same word.)
__global__ __launch_bounds__(THREADS) void k_tiled_mark(const int *__restrict__ rowptr, const int *__restrict__ col,
                                                        int V, int lo, int Vg, int *ghost_flag, int *border_flag) {
  for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < V; u += gridDim.x * blockDim.x) {
    int border = 0;
    for (int k = rowptr[u], kend = rowptr[u + 1]; k < kend; ++k) {
      const int c = col[k];
      if (tiled_foreign(lo, V, Vg, c)) {
        ghost_flag[c] = 1;
        border = 1;
      }
    }
    border_flag[u] = border;
  }
}

// After the scans of both flag arrays: the ghosts' global ids and the border rows' local ids, in ascending order,
// and the solve-graph-index -> global-id table with the solve graph's node states (a ghost: Invalid, see above).
__global__ __launch_bounds__(THREADS) void k_tiled_tables(FieldTiled T, const int *__restrict__ state,
                                                          const int *__restrict__ border_flag,
                                                          const int *__restrict__ border_off) {
  const int n_all = max(T.Vg, T.V);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += gridDim.x * blockDim.x) {
    if (i < T.Vg && T.ghost_flag[i]) {
      const int j = T.ghost_off[i];
      if (j < T.G) {
        T.gid_of[T.V + j] = i;
        T.state[T.V + j] = FIELD_NODE_INVALID;
      }
    }
    if (i < T.V) {
      T.gid_of[i] = T.lo + i;
      T.state[i] = state[i];
      if (border_flag[i]) {
        const int b = border_off[i];
        if (b < T.B) T.border[b] = i;
      }
    }
  }
}

// one thread per local row: the degree of every ghost = the cross edges that name it
__global__ __launch_bounds__(THREADS) void k_tiled_ghost_deg(FieldTiled T, const int *__restrict__ rowptr,
                                                             const int *__restrict__ col, int *ghost_deg) {
  for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < T.V; u += gridDim.x * blockDim.x)
    for (int k = rowptr[u], kend = rowptr[u + 1]; k < kend; ++k) {
      const int j = tiled_ghost(T, col[k]);
      if (j >= 0) atomicAdd(&ghost_deg[j], 1);
    }
}

// One thread per local row writes the row with solve-graph columns and, for each of its cross edges, the reverse
// edge into the ghost's row (slots within a ghost's row by an atomic: their order decides nothing, the parent sweep
// takes a minimum; E2 is the solve graph's edge count, the arrays' size).  Threads past the rows write the ghosts'
// row pointers: rowptr[V + j] = E_local + ghost_row[j].
__global__ __launch_bounds__(THREADS) void k_tiled_fill(FieldTiled T, const int *__restrict__ rowptr,
                                                        const int *__restrict__ col, const float *__restrict__ w,
                                                        const float *__restrict__ dist, int E_local, int E2,
                                                        const int *__restrict__ ghost_row, int *ghost_fill,
                                                        int *rowptr2, int *col2, float *w2, float *dist2) {
  const int n_all = T.V + T.G + 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += gridDim.x * blockDim.x) {
    if (i >= T.V) {
      rowptr2[i] = E_local + ghost_row[i - T.V];
      continue;
    }
    rowptr2[i] = rowptr[i];
    for (int k = rowptr[i], kend = rowptr[i + 1]; k < kend; ++k) {
      const int c = col[k];
      w2[k] = w[k];
      dist2[k] = dist[k];
      const int j = tiled_ghost(T, c);
      if (c >= T.lo && c < T.lo + T.V) {
        col2[k] = c - T.lo;
      } else if (j >= 0) {
        col2[k] = T.V + j;
        const int slot = E_local + ghost_row[j] + atomicAdd(&ghost_fill[j], 1);
        if (slot < E2) {
          col2[slot] = i;
          w2[slot] = w[k];
          dist2[slot] = dist[k];
        }
      } else {
        col2[k] = -1;  // (never: stitch_assemble range-checks its edges; k_field_edge_cost skips such a column)
      }
    }
  }
}

// The seeding of every solve (DESIGN.md section 7, "Source sets across tiles"): one thread per entry of this rank's entry
// table -- the entries of all sets whose member is this rank's node, which the host splits off per call (a single
// source: a set of one entry at cost 0); a member that is a ghost here is seeded by its owner and mirrored like any key.  k_field_seed<true>'s rule with the GLOBAL entry
// index in the member mark, so that "the least entry" is the same on every rank.  Pass 1: the item's key is the least
// of its entries' start costs (atomicMin), queued once.  Pass 2 (F.tight, pass 1's cost bits): only an entry whose
// start cost is the item's least cost seeds it -- a root, whose key (c0, 0) is below every tight extension (hops >= 1),
// so no relaxation pushes or stamps it and its mark stays.
__global__ __launch_bounds__(THREADS) void k_tiled_seed(FieldDev F, const TiledEntry *__restrict__ ent, int n) {
  const int n_iter = (n + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, i = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, i += gridDim.x * blockDim.x) {
    bool first = false;
    int item = 0;
    if (i < n) {
      const TiledEntry t = ent[i];
      if (t.field >= 0 && t.field < F.m && t.node >= 0 && t.node < F.V && t.entry >= 0) {
        item = t.field * F.V + t.node;
        const unsigned long long k0 = (unsigned long long)t.cost0 << 32;
        if (!F.tight) {
          atomicMin(&F.key[item], k0);
          first = atomicMin(&F.stamp_near[item], FIELD_MEMBER | t.entry) >= 0;
        } else if (t.cost0 == F.tight[item]) {
          F.key[item] = k0;  // (every entry that gets here writes this word)
          first = atomicMin(&F.stamp_near[item], FIELD_MEMBER | t.entry) >= 0;
        }
      }
    }
    const unsigned long long mk = ballot(first);
    const int slot = wave_reserve(first, &F.ctrl->c.n[0]);
    if (mk && lane_id() == __ffsll(mk) - 1) atomicAdd(&F.ctrl->s.work, __popcll(mk));
    if (first) {
      if (slot < F.N) F.q[0][slot] = item;
      else atomicOr(&F.ctrl->c.overflow, 1);
    }
  }
}

// Publish: over (field, border row) pairs, those with news become records, compacted with one atomic per wave.
// `published` has m * B words, `rec` room for as many records.  A pass (`owner` is not read): the key is news where it
// is below what this rank last published, and travels.  OWNERS, the owner pass: the owner is news once it is known, and
// travels in the key word; the published word is all ones until then, so that an item is published once.
// BOUNDED, pass 1 of a bounded solve ("Bounded fields across tiles"): a key above its field's current bound is not news
// -- the bound only drops, so it never becomes news -- and the records follow the bound records that k_tiled_bound
// wrote, so the stream has room for m more.
template <bool OWNERS, bool BOUNDED = false>
__global__ __launch_bounds__(THREADS) void k_tiled_publish(FieldDev F, FieldTiled T, const int *__restrict__ owner,
                                                           unsigned long long *published, TiledRec *rec, int *n_rec) {
  static_assert(!(OWNERS && BOUNDED), "the owner pass knows no bounds");
  const int items = F.m * T.B;
  const int room = BOUNDED ? items + F.m : items;
  const int n_iter = (items + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, i = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, i += gridDim.x * blockDim.x) {
    bool news = false;
    TiledRec r{};
    if (i < items) {
      const int f = i / T.B;
      const int v = T.border[i - f * T.B];
      const int item = f * F.V + v;
      if constexpr (OWNERS) {
        const int o = owner[item];
        news = o >= 0 && published[i] != 0ull;
        r.key = (unsigned long long)(unsigned)o;
      } else {
        r.key = F.key[item];
        news = r.key < published[i];
        if constexpr (BOUNDED) news = news && key_cost_bits(r.key) <= F.ctrl->bound[f];
      }
      if (news) {
        published[i] = OWNERS ? 0ull : r.key;
        r.field = f;
        r.gid = T.lo + v;
      }
    }
    const int slot = wave_reserve(news, n_rec);
    if (news && slot < room) rec[slot] = r;
  }
}

// ---- bounded fields across tiles (DESIGN.md section 7, "Bounded fields across tiles") --------------------------------

constexpr unsigned TILED_INF_BITS = 0x7f800000u;  // the cost word that stands for "no key" among settle values

// The bound step of one rank, one block per field, after its rounds went quiet and before its publish.  Over the settle
// targets that are THIS rank's nodes (local ids, n_t > 0): the least (ANY) or greatest (ALL) cost word of their keys,
// +inf bits for a target without one.  Every key is the fold of a real walk, so the value is an upper bound on what the
// definition's settle value takes from these targets, and it only drops.  ANY lowers the field's bound at once (only
// this block writes the word, and no other kernel runs beside it).  A value below what this rank last told the others
// becomes a bound record (field, -1 - rank, value in the key's high word) at the head of the record stream, which the
// host emptied before this launch.
template <bool ALL>
__global__ __launch_bounds__(THREADS) void k_tiled_bound(FieldDev F, const int *__restrict__ targets, int n_t, int rank,
                                                         unsigned *told, TiledRec *rec, int *n_rec, int room) {
  __shared__ unsigned s_v[THREADS / WAVE];
  const int f = blockIdx.x;
  const int fbase = f * F.V;
  unsigned v = ALL ? 0u : TILED_INF_BITS;
  for (int j = threadIdx.x; j < n_t; j += blockDim.x) {
    const int t = targets[j];
    unsigned c = TILED_INF_BITS;
    if (t >= 0 && t < F.V) {
      const unsigned long long k = F.key[fbase + t];
      if (k != FIELD_KEY_NONE) c = key_cost_bits(k);
    }
    v = ALL ? max(v, c) : min(v, c);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)v, m);
    v = ALL ? max(v, o) : min(v, o);
  }
  if (lane_id() == 0) s_v[threadIdx.x / WAVE] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < THREADS / WAVE; ++w) v = ALL ? max(v, s_v[w]) : min(v, s_v[w]);
    if (!ALL && v < F.ctrl->bound[f]) F.ctrl->bound[f] = v;
    if (v < told[f]) {
      told[f] = v;
      const int slot = atomicAdd(n_rec, 1);
      if (slot < room) rec[slot] = TiledRec{f, -1 - rank, (unsigned long long)v << 32};
    }
  }
}

// One thread per gathered record, on every rank and over the records of all ranks, its own included: a bound record
// (gid < 0) lowers its field's bound (ANY), or takes its rank's place in the field's row of the table (ALL; a rank
// tells a field's value once per exchange, so one thread writes the word).  The key merge ignores these records: their
// gid names no node.
template <bool ALL>
__global__ __launch_bounds__(THREADS) void k_tiled_bound_merge(FieldDev F, const TiledRec *__restrict__ rec, int n_rec,
                                                               int n_ranks, unsigned *table) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += gridDim.x * blockDim.x) {
    const TiledRec r = rec[i];
    const int rank = -1 - r.gid;
    if (r.gid >= 0 || rank >= n_ranks || r.field < 0 || r.field >= F.m) continue;
    const unsigned v = (unsigned)(r.key >> 32);
    if constexpr (ALL) table[r.field * STITCH_MAX_TILES + rank] = v;
    else atomicMin(&F.ctrl->bound[r.field], v);
  }
}

// ALL, after the merge: one thread per field folds its row of the table -- +inf bits for a rank that owns a settle
// target and has told nothing yet, 0 for a rank that owns none -- and lowers the field's bound to the greatest entry.
__global__ void k_tiled_bound_fold(FieldDev F, int n_ranks, const unsigned *__restrict__ table) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F.m) return;
  unsigned v = 0u;
  for (int r = 0; r < n_ranks; ++r) v = max(v, table[f * STITCH_MAX_TILES + r]);
  if (v < F.ctrl->bound[f]) F.ctrl->bound[f] = v;
}

// grid.y = field: how many of this rank's OWN nodes have a key (the single-engine count would take the ghosts in), one
// atomicAdd per wave
__global__ __launch_bounds__(THREADS) void k_tiled_reached(FieldDev F, FieldTiled T, int *counts) {
  const int fbase = blockIdx.y * F.V;
  const int n_iter = (T.V + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, v = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, v += gridDim.x * blockDim.x) {
    const unsigned long long mk = ballot(v < T.V && F.key[fbase + v] != FIELD_KEY_NONE);
    if (mk && lane_id() == __ffsll(mk) - 1) atomicAdd(&counts[blockIdx.y], __popcll(mk));
  }
}

// The reached list of one field over this rank's own nodes: k_field_list_count / k_field_list_emit restricted to
// v < T.V, emitting global ids.  Block b covers the nodes [b * THREADS, (b + 1) * THREADS).
__global__ __launch_bounds__(THREADS) void k_tiled_list_count(FieldDev F, FieldTiled T, int field, int *counts) {
  __shared__ int s_n[THREADS / WAVE];
  const int v = blockIdx.x * THREADS + threadIdx.x;
  const bool has = v < T.V && F.key[field * F.V + v] != FIELD_KEY_NONE;
  const unsigned long long m = ballot(has);
  if (lane_id() == 0) s_n[threadIdx.x / WAVE] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int w = 0; w < THREADS / WAVE; ++w) n += s_n[w];
    counts[blockIdx.x] = n;
  }
}

__global__ __launch_bounds__(THREADS) void k_tiled_list_emit(FieldDev F, FieldTiled T, int field,
                                                             const int *__restrict__ offsets, int cap, int *gids,
                                                             float *value, int *hops) {
  __shared__ int s_n[THREADS / WAVE];
  const int v = blockIdx.x * THREADS + threadIdx.x;
  unsigned long long k = FIELD_KEY_NONE;
  if (v < T.V) k = F.key[field * F.V + v];
  const bool has = k != FIELD_KEY_NONE;
  const unsigned long long m = ballot(has);
  if (lane_id() == 0) s_n[threadIdx.x / WAVE] = __popcll(m);
  __syncthreads();
  int pos = offsets[blockIdx.x] + __popcll(m & ((1ull << lane_id()) - 1ull));
  for (int w = 0; w < (int)threadIdx.x / WAVE; ++w) pos += s_n[w];
  if (has && pos < cap) {
    if (gids) gids[pos] = T.lo + v;
    if (value) value[pos] = key_cost(k);
    if (hops) hops[pos] = (int)(unsigned)k;
  }
}

// Merge: one thread per gathered record.  A record of another rank that names one of this rank's ghosts lowers the
// ghost's key to its owner's (only this thread writes the word: an owner publishes a node once per exchange) and
// queues the ghost item in the live far pile at the current phase.  The threshold drops to 0, so that the next round
// opens a bucket at the least merged cost: the rounds then run on as after a warm start.
__global__ __launch_bounds__(THREADS) void k_tiled_merge(FieldDev F, FieldTiled T, const TiledRec *__restrict__ rec,
                                                         int n_rec) {
  const int fs = F.ctrl->s.far_sel;
  const unsigned phase = F.ctrl->s.phase;
  const int n_iter = (n_rec + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, i = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, i += gridDim.x * blockDim.x) {
    bool push = false;
    int item = 0;
    if (i < n_rec) {
      const TiledRec r = rec[i];
      item = tiled_rec_item(F, T, r);
      if (item >= 0 && r.key < F.key[item]) {
        F.key[item] = r.key;
        F.stamp_far[item] = phase;
        push = true;
      }
    }
    const int slot = wave_reserve(push, &F.ctrl->c.nfar[fs]);
    if (push) {
      if (slot < F.N) F.far[fs][slot] = item;
      else atomicOr(&F.ctrl->c.overflow, 1);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) F.ctrl->s.thr = 0u;
}

// The parent sweep over the solve graph, ghost rows included: the least GLOBAL id u with an edge u -> v whose
// extension of key[u] is key[v] (ghosts are not in id order among the solve-graph indices, hence the table).  RISK: F.ec
// holds the edge risks and the extension is the maximum ("Risk fields across tiles").  MODELS (never with RISK): the
// edge costs are those of the block's field ("Cost models across tiles"), one table read per (block, field).
template <bool RISK, bool MODELS>
__global__ __launch_bounds__(THREADS) void k_tiled_parent(FieldDev F, FieldTiled T, FieldModelsArg<MODELS> M) {
  static_assert(!(RISK && MODELS), "a risk field has no cost model");
  const float *__restrict__ ec = field_costs<MODELS>(F, M, blockIdx.y);
  const int sub = threadIdx.x & (GROUP - 1);
  const int g0 = (blockIdx.x * blockDim.x + threadIdx.x) / GROUP;
  const int ng = gridDim.x * blockDim.x / GROUP;
  const int fbase = blockIdx.y * F.V;
  for (int u = g0; u < F.V; u += ng) {
    const unsigned long long ku = F.key[fbase + u];
    if (ku == FIELD_KEY_NONE) continue;
    const int gu = T.gid_of[u];
    for (int k = F.rowptr[u] + sub, kend = F.rowptr[u + 1]; k < kend; k += GROUP) {
      const float c = ec[k];
      if (__float_as_uint(c) == FIELD_EDGE_SKIP) continue;
      const int v = fbase + F.col[k];
      if (key_extend<RISK>(ku, c) == F.key[v]) atomicMin(&F.parent[v], gu);
    }
  }
}

// grid.y = field: this rank's own nodes only, m x V_local; with owner_out (else nullptr) their owners too
__global__ __launch_bounds__(THREADS) void k_tiled_output(FieldDev F, FieldTiled T, float *cost, int *hops,
                                                          int *parent, const int *__restrict__ owner,
                                                          int *owner_out) {
  const int fbase = blockIdx.y * F.V, obase = blockIdx.y * T.V;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < T.V; v += gridDim.x * blockDim.x) {
    const unsigned long long k = F.key[fbase + v];
    const bool reached = k != FIELD_KEY_NONE;
    cost[obase + v] = reached ? key_cost(k) : __builtin_huge_valf();
    hops[obase + v] = reached ? (int)(unsigned)k : -1;
    const int p = F.parent[fbase + v];
    parent[obase + v] = p == INT_MAX ? -1 : p;
    if (owner_out) owner_out[obase + v] = owner[fbase + v];
  }
}

// ---- the owner pass across seams (DESIGN.md section 7, "Source sets across tiles") ---------------------------------

// grid.y = field, over the solve graph's items: the first ancestor of every item in the forest of k_tiled_parent's
// GLOBAL parents, into F.q[0], and the owners known before any exchange.  A local root (by its mark) is its own
// ancestor and knows its owner, the mark's entry counted from its set's first; a ghost with a key is its own ancestor
// too -- a terminal, whose owner only the rank that owns the node knows; every other item with a key points at the
// solve-graph item of its parent, a local node or a ghost.  *n_roots counts the roots, one atomic per wave.
__global__ __launch_bounds__(THREADS) void k_tiled_forest_begin(FieldDev F, FieldTiled T,
                                                                const int *__restrict__ set_ptr, int *owner,
                                                                int *n_roots) {
  const int fbase = blockIdx.y * F.V;
  const int e0 = set_ptr[blockIdx.y];
  int *anc = F.q[0];
  const int n_iter = (F.V + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, v = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, v += gridDim.x * blockDim.x) {
    bool root = false;
    if (v < F.V) {
      const int i = fbase + v;
      int a = -1, o = -1;
      if (F.key[i] != FIELD_KEY_NONE) {
        const int mark = F.stamp_near[i];
        if (v >= T.V) {
          a = i;
        } else if (mark < 0) {
          a = i;
          o = (mark & INT_MAX) - e0;
          root = true;
        } else {
          const int p = F.parent[i];
          const int j = tiled_ghost(T, p);
          if (p >= T.lo && p < T.lo + T.V) a = fbase + (p - T.lo);
          else if (j >= 0) a = fbase + T.V + j;
        }
      }
      anc[i] = a;
      owner[i] = o;
    }
    const unsigned long long mk = ballot(root);
    if (mk && lane_id() == __ffsll(mk) - 1) atomicAdd(n_roots, __popcll(mk));
  }
}

// One thread per gathered owner record (field, global id, owner in the key word): a record of another rank that names
// one of this rank's ghosts gives the ghost item its owner.  An owner publishes an item once, so one thread writes
// the word; only ghost items are written, as in k_tiled_merge.
__global__ __launch_bounds__(THREADS) void k_tiled_owner_merge(FieldDev F, FieldTiled T,
                                                               const TiledRec *__restrict__ rec, int n_rec, int *owner) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += gridDim.x * blockDim.x) {
    const TiledRec r = rec[i];
    const int item = tiled_rec_item(F, T, r);
    if (item >= 0) owner[item] = (int)(unsigned)r.key;
  }
}

// One gather over the items: an item without an owner takes its last ancestor's once that is known.  `anc` is final
// (the sweeps ended), an item that is read here is its own ancestor and is not written here.
__global__ __launch_bounds__(THREADS) void k_tiled_owner_resolve(const int *__restrict__ anc, int *owner, int N) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const int a = anc[i];
    if (a < 0 || a >= N || a == i || owner[i] >= 0) continue;
    const int o = owner[a];
    if (o >= 0) owner[i] = o;
  }
}

// grid.y = field: a histogram of the owners of this rank's own nodes (k_field_owned's shape, the ghosts left out: the
// rank that owns a node counts it), one atomicAdd per wave and distinct owner among its lanes
__global__ __launch_bounds__(THREADS) void k_tiled_owned(FieldDev F, FieldTiled T, const int *__restrict__ set_ptr,
                                                         const int *__restrict__ owner, int n_entries, int *owned) {
  const int fbase = blockIdx.y * F.V;
  const int e0 = set_ptr[blockIdx.y];
  const int room = min(set_ptr[blockIdx.y + 1], n_entries) - e0;
  const int n_iter = (T.V + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, v = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, v += gridDim.x * blockDim.x) {
    int o = v < T.V ? owner[fbase + v] : -1;
    if (o >= room) o = -1;  // (never: an owner is an entry of its field's set)
    unsigned long long rest = ballot(o >= 0);
    while (rest) {  // (wave-uniform)
      const int leader = __ffsll(rest) - 1;
      const int lo = __shfl(o, leader);
      const unsigned long long same = ballot(o == lo);
      if (lane_id() == leader) atomicAdd(&owned[e0 + lo], __popcll(same));
      rest &= ~same;
    }
  }
}

// ---- routes across tiles (DESIGN.md section 7, "Routes across tiles") -----------------------------------------------

// 16 bytes, the exchange's record again.  LEN (exchange 0 only): {route, hops or -1, cost bits, owner}.  HANDOFF:
// {route, the parent's global id (>= 0), sum_dist bits, sum_w bits}.  END: {route, -1 - root gid, the sums}.
struct TiledRouteRec {
  int route, b;
  unsigned c, d;
};
static_assert(sizeof(TiledRouteRec) == FIELD_TILED_REC_BYTES, "record layout");
static_assert(sizeof(TiledRouteInfo) == 24, "route info layout");

// One thread per route: the rank that owns the target publishes its LEN record.
__global__ __launch_bounds__(THREADS) void k_tiled_route_len(FieldDev F, FieldTiled T, TiledRoutes R) {
  TiledRouteRec *rec = (TiledRouteRec *)R.rec;
  const int n_iter = (R.n + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, r = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, r += gridDim.x * blockDim.x) {
    bool mine = false;
    TiledRouteRec out{};
    if (r < R.n) {
      const int f = R.field[r];
      const long long l = (long long)R.target[r] - T.lo;
      if (l >= 0 && l < T.V && f >= 0 && f < F.m) {
        const int item = f * F.V + (int)l;
        const unsigned long long k = F.key[item];
        const bool reached = k != FIELD_KEY_NONE;
        mine = true;
        out.route = r;
        out.b = reached ? (int)(unsigned)k : -1;
        out.c = reached ? key_cost_bits(k) : __float_as_uint(__builtin_huge_valf());
        out.d = (unsigned)(reached && R.owner ? R.owner[item] : -1);
      }
    }
    const int slot = wave_reserve(mine, R.n_rec);
    if (mine) {
      if (slot < R.rec_cap) rec[slot] = out;
      else atomicMax(R.n_rec + 2, r + 1);
    }
  }
}

// The walks of one exchange: one 16-lane group per item, as k_field_route_walk.  BEGIN (exchange 1): an item is a
// route, walked from its target by the rank that owns it.  Else an item is a gathered record; a HANDOFF that names
// one of this rank's nodes is walked on from there with the sums it carries.  A walk writes its node's global id at
// offsets[r] + hops where that lies inside the clipped segment, finds the tight edge of least index into its node in
// the parent's row of the solve graph -- a local row keeps G's order, a ghost's row holds each cross edge once, with
// the owner's bits -- adds its dist and w, and steps to the parent; at a ghost it publishes HANDOFF, at hops == 0,
// where its node must carry a member mark, END.  Every route has one walker at any time: nothing here is atomic but
// the record slots (wave_reserve, every lane of the wave gets there: the trip counts are uniform) and the word beside
// the record count that a walk which lost its way sets to its route + 1.  RISK: the tight-edge test extends by the
// maximum over the edge risks in F.ec; the sums are the folds of dist and w all the same.  MODELS (never with RISK):
// the edge costs are those of the route's field, one table read per item -- an edge above the field's ceiling is
// skipped there, so the route edge is the ADMITTED tight edge of least index.
template <bool BEGIN, bool RISK, bool MODELS>
__global__ __launch_bounds__(THREADS) void k_tiled_route_step(FieldDev F, FieldTiled T, TiledRoutes R,
                                                              const TiledRouteRec *__restrict__ in, int n_in,
                                                              FieldModelsArg<MODELS> M) {
  static_assert(!(RISK && MODELS), "a risk field has no cost model");
  TiledRouteRec *rec = (TiledRouteRec *)R.rec;
  const int sub = threadIdx.x & (GROUP - 1);
  const int gshift = lane_id() & ~(GROUP - 1);
  const int g0 = (blockIdx.x * blockDim.x + threadIdx.x) / GROUP;
  const int ng = gridDim.x * blockDim.x / GROUP;
  const int items = BEGIN ? R.n : n_in;
  const int n_iter = (items + ng - 1) / ng;
  for (int it = 0, i = g0; it < n_iter; ++it, i += ng) {
    bool go = false, broken = false, publish = false;
    int r = 0, v = 0;
    float sum_dist = 0.0f, sum_w = 0.0f;
    if (i < items) {
      long long l = -1;
      if constexpr (BEGIN) {
        r = i;
        l = (long long)R.target[r] - T.lo;
      } else {
        const TiledRouteRec h = in[i];
        r = h.route;
        if (r >= 0 && r < R.n && h.b >= 0) l = (long long)h.b - T.lo;
        sum_dist = __uint_as_float(h.c);
        sum_w = __uint_as_float(h.d);
      }
      if (l >= 0 && l < T.V) {
        v = (int)l;
        const int f = R.field[r];
        go = f >= 0 && f < F.m && (!BEGIN || F.key[f * F.V + v] != FIELD_KEY_NONE);
      }
    }
    TiledRouteRec out{};
    if (go) {
      const int fbase = R.field[r] * F.V;
      const float *__restrict__ ec = field_costs<MODELS>(F, M, R.field[r]);
      const int off = R.node_gids ? R.offsets[r] : 0;
      const int room = R.node_gids ? R.offsets[r + 1] - off : 0;
      unsigned long long kv = F.key[fbase + v];
      broken = kv == FIELD_KEY_NONE;
      while (!broken) {
        const int h = (int)(unsigned)kv;
        if (sub == 0 && h < room) R.node_gids[off + h] = T.lo + v;
        if (h == 0) {  // a root, by its mark
          if (F.stamp_near[fbase + v] >= 0) broken = true;
          out.b = -1 - (T.lo + v);
          publish = true;
          break;
        }
        const int p = F.parent[fbase + v];  // a global id
        const int j = tiled_ghost(T, p);
        const int u = p >= T.lo && p < T.lo + T.V ? p - T.lo : j >= 0 ? T.V + j : -1;
        if (u < 0) {
          broken = true;
          break;
        }
        const unsigned long long ku = F.key[fbase + u];
        int edge = -1;
        for (int k0 = F.rowptr[u], kend = F.rowptr[u + 1]; k0 < kend; k0 += GROUP) {
          const int k = k0 + sub;
          bool hit = false;
          if (k < kend && F.col[k] == v) {
            const float c = ec[k];
            hit = __float_as_uint(c) != FIELD_EDGE_SKIP && key_extend<RISK>(ku, c) == kv;
          }
          const unsigned hits = (unsigned)(ballot(hit) >> gshift) & ((1u << GROUP) - 1u);
          if (hits) {
            edge = k0 + __ffs(hits) - 1;
            break;
          }
        }
        if (edge < 0) {
          broken = true;
          break;
        }
        sum_dist += R.dist[edge];
        sum_w += R.w[edge];
        if (u >= T.V) {  // the parent is another rank's node: the route goes on there
          out.b = p;
          publish = true;
          break;
        }
        v = u;
        kv = ku;
      }
      out.route = r;
      out.c = __float_as_uint(sum_dist);
      out.d = __float_as_uint(sum_w);
      if (broken && sub == 0) atomicMax(R.n_rec + 2, r + 1);
    }
    const bool mine = publish && !broken && sub == 0;
    const int slot = wave_reserve(mine, R.n_rec);
    if (mine) {
      if (slot < R.rec_cap) rec[slot] = out;
      else atomicMax(R.n_rec + 2, r + 1);
    }
  }
}

// One thread per gathered record: an END record gives its route the sums and the root.  Every rank gathers the same
// records, so every rank's info array ends up the same; a route ends once, so one thread writes its entry.
__global__ __launch_bounds__(THREADS) void k_tiled_route_end(const TiledRouteRec *__restrict__ in, int n_in,
                                                             TiledRouteInfo *infos, int n_routes) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += gridDim.x * blockDim.x) {
    const TiledRouteRec h = in[i];
    if (h.b >= 0 || h.route < 0 || h.route >= n_routes) continue;
    TiledRouteInfo &o = infos[h.route];
    if (o.num_nodes <= 0) continue;  // (never: only a reached target is walked)
    o.path_length = __uint_as_float(h.c);
    o.avg_risk = __uint_as_float(h.d) / (float)o.num_nodes;
    o.root_gid = -1 - h.b;
  }
}

// ---- refresh across tiles (DESIGN.md section 7, "Refresh across tiles") ---------------------------------------------

// grid.y = field: this rank's keys of the retained solve (V_old local nodes per field, at `old_stride` = V_old + G_old
// items per field; ghost keys are not carried) at the local nodes of the new tile graph, none where the map names no
// old node.  `out` (m x V, no ghosts: their number is not known yet) is no array of the old solve.
__global__ __launch_bounds__(THREADS) void k_tiled_carry(const unsigned long long *__restrict__ old_key,
                                                         long long old_stride, int V_old,
                                                         const int *__restrict__ new2old, int V,
                                                         unsigned long long *__restrict__ out) {
  const long long obase = (long long)blockIdx.y * old_stride;
  const int fbase = blockIdx.y * V;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
    const int o = new2old[v];
    out[fbase + v] = o >= 0 && o < V_old ? old_key[obase + o] : FIELD_KEY_NONE;
  }
}

// grid.y = field, over the solve graph's items: k_field_init for a refresh.  A local node takes its carried key, a
// ghost none (the fill gives it its owner's); parents, stamps and the control block as a cold pass starts them, so
// that k_tiled_seed can force and mark this rank's members.
__global__ __launch_bounds__(THREADS) void k_tiled_refresh_begin(FieldDev F, FieldTiled T,
                                                                 const unsigned long long *__restrict__ carried,
                                                                 float delta) {
  const int f = blockIdx.y;
  const int fbase = f * F.V, cbase = f * T.V;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < F.V; v += gridDim.x * blockDim.x) {
    F.key[fbase + v] = v < T.V ? carried[cbase + v] : FIELD_KEY_NONE;
    F.parent[fbase + v] = INT_MAX;
    F.stamp_near[fbase + v] = 0;
    F.stamp_far[fbase + v] = 0u;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) F.ctrl->reached[f] = 0;
  if (blockIdx.x == 0 && f == 0 && threadIdx.x == 0) field_ctrl_reset(F, __float_as_uint(delta), delta, 0);
}

// One thread per entry of this rank's entry table: a member record (entry, -1, the member's NEW global id) behind the
// key records of the fill exchange, so that every rank learns where every member of the retained request lies now.
// The key merges ignore it: its gid names no node.
__global__ __launch_bounds__(THREADS) void k_tiled_member_recs(FieldTiled T, const TiledEntry *__restrict__ ent, int n,
                                                               TiledRec *rec, int *n_rec, int room) {
  const int n_iter = (n + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, i = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, i += gridDim.x * blockDim.x) {
    const bool mine = i < n;
    TiledRec r{};
    if (mine) {
      const TiledEntry t = ent[i];
      r.field = t.entry;
      r.gid = -1;
      r.key = (unsigned long long)(unsigned)(T.lo + t.node);
    }
    const int slot = wave_reserve(mine, n_rec);
    if (mine && slot < room) rec[slot] = r;
  }
}

// The ghost fill, the "set" form of k_tiled_merge: one thread per gathered record of the fill exchange.  A key record
// of another rank that names one of this rank's ghosts gives the ghost its owner's carried key, by assignment (an owner
// publishes a node once: one thread writes the word; nothing is queued).  A member record writes its entry's word of
// `members` (n_members words; an entry has one owner, so one record).
__global__ __launch_bounds__(THREADS) void k_tiled_fill_ghosts(FieldDev F, FieldTiled T,
                                                               const TiledRec *__restrict__ rec, int n_rec,
                                                               int *members, int n_members) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += gridDim.x * blockDim.x) {
    const TiledRec r = rec[i];
    if (r.gid < 0) {
      if (r.gid == -1 && r.field >= 0 && r.field < n_members) members[r.field] = (int)(unsigned)r.key;
      continue;
    }
    const int item = T.G > 0 ? tiled_rec_item(F, T, r) : -1;  // (a tile without nodes has no ghost table)
    if (item >= 0) F.key[item] = r.key;
  }
}

// grid.y = field, over the solve graph's items: the forest of an anchor, k_tiled_forest_begin over the SUPPORTERS that
// k_tiled_parent found under the carried keys.  `rooted` takes the owner pass's place: >= 0 where an item is known to
// hang on a member (a marked member at once), -1 where not yet.  A ghost with a key is a terminal whose verdict its
// owner publishes; an item without a supporter points nowhere and is lost.  With key0 (the second anchor) an item
// whose key is no longer key0's is cut.
__global__ __launch_bounds__(THREADS) void k_tiled_anchor_begin(FieldDev F, FieldTiled T,
                                                                const unsigned long long *__restrict__ key0,
                                                                int *rooted) {
  const int fbase = blockIdx.y * F.V;
  int *anc = F.q[0];
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < F.V; v += gridDim.x * blockDim.x) {
    const int i = fbase + v;
    const unsigned long long k = F.key[i];
    int a = -1, o = -1;
    if (k != FIELD_KEY_NONE && (!key0 || k == key0[i])) {
      if (v >= T.V) {
        a = i;
      } else if (F.stamp_near[i] < 0) {
        a = i;
        o = 0;
      } else {
        const int p = F.parent[i];
        const int j = tiled_ghost(T, p);
        if (p >= T.lo && p < T.lo + T.V) a = fbase + (p - T.lo);
        else if (j >= 0) a = fbase + T.V + j;
      }
    }
    anc[i] = a;
    rooted[i] = o;
  }
}

// grid.y = field, over the solve graph's items, after the anchor's exchanges: an item that is not known to hang on a
// member loses its key, a ghost too.  key0 / carried (the first anchor): the keys as they are now (m x (V + G)), and
// per field the count of this rank's OWN nodes that kept theirs, one atomic per wave.
__global__ __launch_bounds__(THREADS) void k_tiled_anchor_end(FieldDev F, FieldTiled T, const int *__restrict__ rooted,
                                                              unsigned long long *__restrict__ key0, int *carried) {
  const int fbase = blockIdx.y * F.V;
  const int n_iter = (F.V + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, v = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, v += gridDim.x * blockDim.x) {
    bool kept = false;
    if (v < F.V) {
      unsigned long long k = F.key[fbase + v];
      if (rooted[fbase + v] < 0 && k != FIELD_KEY_NONE) F.key[fbase + v] = k = FIELD_KEY_NONE;
      if (key0) key0[fbase + v] = k;
      kept = v < T.V && k != FIELD_KEY_NONE;
    }
    const unsigned long long mk = ballot(kept);
    if (carried && mk && lane_id() == __ffsll(mk) - 1) atomicAdd(&carried[blockIdx.y], __popcll(mk));
  }
}

// Over (field, border row) pairs: what a warm pass starts from as published -- the border keys as the anchor left
// them, which every ghost of them mirrors.  A pass then publishes only what its rounds lowered.
__global__ __launch_bounds__(THREADS) void k_tiled_published_init(FieldDev F, FieldTiled T,
                                                                  unsigned long long *published) {
  const int items = F.m * T.B;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < items; i += gridDim.x * blockDim.x) {
    const int f = i / T.B;
    published[i] = F.key[f * F.V + T.border[i - f * T.B]];
  }
}

}  // namespace

void launch_tiled_carry(const unsigned long long *old_key, long long old_stride, int V_old, const int *new2old, int V,
                        int m, unsigned long long *out, hipStream_t s) {
  if (V > 0 && m > 0)
    hipLaunchKernelGGL(k_tiled_carry, dim3(field_blocks(V, THREADS), m), dim3(THREADS), 0, s, old_key, old_stride, V_old,
                       new2old, V, out);
}

void launch_tiled_refresh_begin(const FieldDev &F, const FieldTiled &T, const unsigned long long *carried,
                                const TiledEntry *entries, int n_entries, float delta, hipStream_t s) {
  hipLaunchKernelGGL(k_tiled_refresh_begin, dim3(field_blocks(F.V, THREADS), F.m), dim3(THREADS), 0, s, F, T, carried,
                     delta);
  if (n_entries > 0)
    hipLaunchKernelGGL(k_tiled_seed, dim3(field_blocks(n_entries, THREADS)), dim3(THREADS), 0, s, F, entries, n_entries);
}

void launch_tiled_fill_publish(const FieldDev &F, const FieldTiled &T, const TiledEntry *entries, int n_entries,
                               unsigned long long *published, void *rec, int *n_rec, hipStream_t s) {
  (void)hipMemsetAsync(published, 0xFF, ((size_t)F.m * T.B + 1) * sizeof(unsigned long long), s);
  launch_tiled_publish(F, T, nullptr, published, rec, n_rec, s);
  if (n_entries > 0)
    hipLaunchKernelGGL(k_tiled_member_recs, dim3(field_blocks(n_entries, THREADS)), dim3(THREADS), 0, s, T, entries,
                       n_entries, (TiledRec *)rec, n_rec, F.m * T.B + n_entries);
}

void launch_tiled_fill_ghosts(const FieldDev &F, const FieldTiled &T, const void *rec, int n_rec, int *members,
                              int n_members, hipStream_t s) {
  if (n_rec > 0)
    hipLaunchKernelGGL(k_tiled_fill_ghosts, dim3(field_blocks(n_rec, THREADS)), dim3(THREADS), 0, s, F, T,
                       (const TiledRec *)rec, n_rec, members, n_members);
}

void launch_tiled_anchor_begin(const FieldDev &F, const FieldTiled &T, const unsigned long long *key0, int *rooted,
                               int *changed, unsigned long long *published, hipStream_t s) {
  (void)hipMemsetAsync(changed, 0, FIELD_OWNER_SWEEPS_MAX * sizeof(int), s);
  (void)hipMemsetAsync(published, 0xFF, ((size_t)F.m * T.B + 1) * sizeof(unsigned long long), s);
  hipLaunchKernelGGL(k_tiled_anchor_begin, dim3(field_blocks(F.V, THREADS), F.m), dim3(THREADS), 0, s, F, T, key0,
                     rooted);
}

void launch_tiled_anchor_end(const FieldDev &F, const FieldTiled &T, const int *rooted, unsigned long long *key0,
                             int *carried, unsigned long long *published, hipStream_t s) {
  if (carried) (void)hipMemsetAsync(carried, 0, (size_t)F.m * sizeof(int), s);
  hipLaunchKernelGGL(k_tiled_anchor_end, dim3(field_blocks(F.V, THREADS), F.m), dim3(THREADS), 0, s, F, T, rooted, key0,
                     carried);
  if (T.B > 0)
    hipLaunchKernelGGL(k_tiled_published_init, dim3(field_blocks((long long)F.m * T.B, THREADS)), dim3(THREADS), 0, s, F,
                       T, published);
}

void launch_tiled_route_len(const FieldDev &F, const FieldTiled &T, const TiledRoutes &R, hipStream_t s) {
  (void)hipMemsetAsync(R.n_rec, 0, sizeof(int), s);
  if (R.n > 0 && T.V > 0)
    hipLaunchKernelGGL(k_tiled_route_len, dim3(field_blocks(R.n, THREADS)), dim3(THREADS), 0, s, F, T, R);
}

void launch_tiled_route_step(const FieldDev &F, const FieldTiled &T, const TiledRoutes &R, const void *rec_in, int n_in,
                             TiledRouteInfo *infos, hipStream_t s, bool risk, const FieldModels *models) {
  const FieldNoModels none{};
  (void)hipMemsetAsync(R.n_rec, 0, sizeof(int), s);
  const TiledRouteRec *in = (const TiledRouteRec *)rec_in;
  if (!in) {
    if (R.n > 0 && T.V > 0) {
      const dim3 grid(field_blocks((long long)R.n * GROUP, THREADS));
      if (risk) hipLaunchKernelGGL((k_tiled_route_step<true, true, false>), grid, dim3(THREADS), 0, s, F, T, R, in, 0, none);
      else if (models)
        hipLaunchKernelGGL((k_tiled_route_step<true, false, true>), grid, dim3(THREADS), 0, s, F, T, R, in, 0, *models);
      else hipLaunchKernelGGL((k_tiled_route_step<true, false, false>), grid, dim3(THREADS), 0, s, F, T, R, in, 0, none);
    }
    return;
  }
  if (n_in <= 0) return;
  if (T.V > 0) {
    const dim3 grid(field_blocks((long long)n_in * GROUP, THREADS));
    if (risk) hipLaunchKernelGGL((k_tiled_route_step<false, true, false>), grid, dim3(THREADS), 0, s, F, T, R, in, n_in, none);
    else if (models)
      hipLaunchKernelGGL((k_tiled_route_step<false, false, true>), grid, dim3(THREADS), 0, s, F, T, R, in, n_in, *models);
    else hipLaunchKernelGGL((k_tiled_route_step<false, false, false>), grid, dim3(THREADS), 0, s, F, T, R, in, n_in, none);
  }
  hipLaunchKernelGGL(k_tiled_route_end, dim3(field_blocks(n_in, THREADS)), dim3(THREADS), 0, s, in, n_in, infos, R.n);
}

void launch_tiled_mark(const int *rowptr, const int *col, int V, int lo, int Vg, int *ghost_flag, int *border_flag,
                       hipStream_t s) {
  (void)hipMemsetAsync(ghost_flag, 0, ((size_t)Vg + 1) * sizeof(int), s);
  if (V > 0)
    hipLaunchKernelGGL(k_tiled_mark, dim3(field_blocks(V, THREADS)), dim3(THREADS), 0, s, rowptr, col, V, lo, Vg,
                       ghost_flag, border_flag);
}

void launch_tiled_tables(const FieldTiled &T, const int *state, const int *border_flag, const int *border_off,
                         const int *rowptr, const int *col, int *ghost_deg, hipStream_t s) {
  hipLaunchKernelGGL(k_tiled_tables, dim3(field_blocks(std::max(T.Vg, T.V), THREADS)), dim3(THREADS), 0, s, T, state,
                     border_flag, border_off);
  (void)hipMemsetAsync(ghost_deg, 0, ((size_t)T.G + 1) * sizeof(int), s);
  hipLaunchKernelGGL(k_tiled_ghost_deg, dim3(field_blocks(T.V, THREADS)), dim3(THREADS), 0, s, T, rowptr, col,
                     ghost_deg);
}

void launch_tiled_fill(const FieldTiled &T, const int *rowptr, const int *col, const float *w, const float *dist,
                       int E_local, int E2, const int *ghost_row, int *ghost_fill, int *rowptr2, int *col2,
                       float *w2, float *dist2, hipStream_t s) {
  (void)hipMemsetAsync(ghost_fill, 0, ((size_t)T.G + 1) * sizeof(int), s);
  hipLaunchKernelGGL(k_tiled_fill, dim3(field_blocks(T.V + T.G + 1, THREADS)), dim3(THREADS), 0, s, T, rowptr, col, w,
                     dist, E_local, E2, ghost_row, ghost_fill, rowptr2, col2, w2, dist2);
}

void launch_tiled_begin(const FieldDev &F, const FieldTiled &T, const TiledEntry *entries, int n_entries, float delta,
                        unsigned long long *published, hipStream_t s) {
  hipLaunchKernelGGL(k_field_init, dim3(field_blocks(F.V, THREADS), F.m), dim3(THREADS), 0, s, F, FieldSources{}, delta,
                     false, (const unsigned long long *)nullptr);
  if (n_entries > 0)
    hipLaunchKernelGGL(k_tiled_seed, dim3(field_blocks(n_entries, THREADS)), dim3(THREADS), 0, s, F, entries, n_entries);
  (void)hipMemsetAsync(published, 0xFF, ((size_t)F.m * T.B + 1) * sizeof(unsigned long long), s);
}

void launch_tiled_publish(const FieldDev &F, const FieldTiled &T, const int *owner, unsigned long long *published,
                          void *rec, int *n_rec, hipStream_t s) {
  (void)hipMemsetAsync(n_rec, 0, sizeof(int), s);
  if (T.B <= 0) return;
  const dim3 grid(field_blocks((long long)F.m * T.B, THREADS));
  TiledRec *out = (TiledRec *)rec;
  if (owner) hipLaunchKernelGGL(k_tiled_publish<true>, grid, dim3(THREADS), 0, s, F, T, owner, published, out, n_rec);
  else hipLaunchKernelGGL(k_tiled_publish<false>, grid, dim3(THREADS), 0, s, F, T, owner, published, out, n_rec);
}

void launch_tiled_publish_bounded(const FieldDev &F, const FieldTiled &T, const TiledSettle &S,
                                  unsigned long long *published, void *rec, int *n_rec, hipStream_t s) {
  (void)hipMemsetAsync(n_rec, 0, sizeof(int), s);
  if (F.N <= 0) return;
  TiledRec *out = (TiledRec *)rec;
  const int room = F.m * T.B + F.m;
  if (S.mode == FIELD_SETTLE_ANY && S.n_t > 0)
    hipLaunchKernelGGL(k_tiled_bound<false>, dim3(F.m), dim3(THREADS), 0, s, F, S.targets, S.n_t, S.rank, S.told, out,
                       n_rec, room);
  else if (S.mode == FIELD_SETTLE_ALL && S.n_t > 0)
    hipLaunchKernelGGL(k_tiled_bound<true>, dim3(F.m), dim3(THREADS), 0, s, F, S.targets, S.n_t, S.rank, S.told, out,
                       n_rec, room);
  if (T.B > 0)
    hipLaunchKernelGGL((k_tiled_publish<false, true>), dim3(field_blocks((long long)F.m * T.B, THREADS)), dim3(THREADS),
                       0, s, F, T, (const int *)nullptr, published, out, n_rec);
}

void launch_tiled_bound_merge(const FieldDev &F, const TiledSettle &S, const void *rec, int n_rec, hipStream_t s) {
  if (n_rec <= 0 || S.mode == FIELD_SETTLE_NONE) return;
  const dim3 grid(field_blocks(n_rec, THREADS));
  if (S.mode == FIELD_SETTLE_ANY) {
    hipLaunchKernelGGL(k_tiled_bound_merge<false>, grid, dim3(THREADS), 0, s, F, (const TiledRec *)rec, n_rec,
                       S.n_ranks, S.table);
    return;
  }
  hipLaunchKernelGGL(k_tiled_bound_merge<true>, grid, dim3(THREADS), 0, s, F, (const TiledRec *)rec, n_rec, S.n_ranks,
                     S.table);
  hipLaunchKernelGGL(k_tiled_bound_fold, dim3(1), dim3(FIELD_MAX_SOURCES), 0, s, F, S.n_ranks, S.table);
}

void launch_tiled_reached(const FieldDev &F, const FieldTiled &T, int *counts, hipStream_t s) {
  (void)hipMemsetAsync(counts, 0, (size_t)F.m * sizeof(int), s);
  if (T.V > 0 && F.N > 0)
    hipLaunchKernelGGL(k_tiled_reached, dim3(field_blocks(T.V, THREADS), F.m), dim3(THREADS), 0, s, F, T, counts);
}

void launch_tiled_reached_list(const FieldDev &F, const FieldTiled &T, int field, int *counts, int *offsets, int *tmp,
                               int cap, int *gids, float *value, int *hops, hipStream_t s) {
  const int nb = (T.V + THREADS - 1) / THREADS;
  hipLaunchKernelGGL(k_tiled_list_count, dim3(nb), dim3(THREADS), 0, s, F, T, field, counts);
  launch_exclusive_scan(counts, offsets, nb, tmp, s);
  if (cap > 0 && (gids || value || hops))
    hipLaunchKernelGGL(k_tiled_list_emit, dim3(nb), dim3(THREADS), 0, s, F, T, field, offsets, cap, gids, value, hops);
}

void launch_tiled_merge(const FieldDev &F, const FieldTiled &T, const void *rec, int n_rec, hipStream_t s) {
  if (n_rec > 0 && T.G > 0)
    hipLaunchKernelGGL(k_tiled_merge, dim3(field_blocks(n_rec, THREADS)), dim3(THREADS), 0, s, F, T,
                       (const TiledRec *)rec, n_rec);
}

void launch_tiled_parents(const FieldDev &F, const FieldTiled &T, hipStream_t s, bool risk, const FieldModels *models) {
  const dim3 grid(field_blocks((long long)F.V * GROUP, THREADS), F.m);
  if (risk) hipLaunchKernelGGL((k_tiled_parent<true, false>), grid, dim3(THREADS), 0, s, F, T, FieldNoModels{});
  else if (models) hipLaunchKernelGGL((k_tiled_parent<false, true>), grid, dim3(THREADS), 0, s, F, T, *models);
  else hipLaunchKernelGGL((k_tiled_parent<false, false>), grid, dim3(THREADS), 0, s, F, T, FieldNoModels{});
}

void launch_tiled_finish(const FieldDev &F, const FieldTiled &T, float *cost, int *hops, int *parent, bool parents,
                         const int *owner, int *owner_out, hipStream_t s, bool risk, const FieldModels *models) {
  if (parents) launch_tiled_parents(F, T, s, risk, models);
  if (T.V > 0)
    hipLaunchKernelGGL(k_tiled_output, dim3(field_blocks(T.V, THREADS), F.m), dim3(THREADS), 0, s, F, T, cost, hops,
                       parent, owner, owner_out);
}

void launch_tiled_forest_begin(const FieldDev &F, const FieldTiled &T, const int *set_ptr, int *owner, int *changed,
                               int *n_roots, unsigned long long *published, hipStream_t s) {
  (void)hipMemsetAsync(changed, 0, FIELD_OWNER_SWEEPS_MAX * sizeof(int), s);
  (void)hipMemsetAsync(n_roots, 0, sizeof(int), s);
  (void)hipMemsetAsync(published, 0xFF, ((size_t)F.m * T.B + 1) * sizeof(unsigned long long), s);
  hipLaunchKernelGGL(k_tiled_forest_begin, dim3(field_blocks(F.V, THREADS), F.m), dim3(THREADS), 0, s, F, T, set_ptr,
                     owner, n_roots);
}

void launch_tiled_owner_step(const FieldDev &F, const FieldTiled &T, const void *rec_in, int n_in, const int *anc,
                             int *owner, unsigned long long *published, void *rec, int *n_rec, hipStream_t s) {
  if (n_in > 0 && T.G > 0)
    hipLaunchKernelGGL(k_tiled_owner_merge, dim3(field_blocks(n_in, THREADS)), dim3(THREADS), 0, s, F, T,
                       (const TiledRec *)rec_in, n_in, owner);
  hipLaunchKernelGGL(k_tiled_owner_resolve, dim3(field_blocks(F.N, THREADS)), dim3(THREADS), 0, s, anc, owner, F.N);
  launch_tiled_publish(F, T, owner, published, rec, n_rec, s);
}

void launch_tiled_owned(const FieldDev &F, const FieldTiled &T, const int *set_ptr, const int *owner, int n_entries,
                        int *owned, hipStream_t s) {
  (void)hipMemsetAsync(owned, 0, (size_t)n_entries * sizeof(int), s);
  if (T.V > 0)
    hipLaunchKernelGGL(k_tiled_owned, dim3(field_blocks(T.V, THREADS), F.m), dim3(THREADS), 0, s, F, T, set_ptr, owner,
                       n_entries, owned);
}
