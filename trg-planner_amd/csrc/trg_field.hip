// trg_field.hip -- gfx950 kernels of the cost field: the least (cost, hops) key from one node to every node of
// the global graph (an extension; the reference answers only single-pair queries, planSafePath trg.cpp:603-690),
// for m sources in one solve.
//
// Semantics ("Cost field"): an edge costs (safety_factor * w + 1) * dist, every operation
// rounded to fp32 (the A* step of trg.cpp:674 on OptimizeNode's float g_); a walk's cost is the left fold
// g' = g + c in fp32; walks never enter an Invalid node (trg.cpp:670).  fl(a + c) is monotone in a and never
// below a, so the least fold over all walks is one least fixed point that every relaxation order reaches.
// The hop word is NOT monotone under rounding (a < a' can give fl(a + c) == fl(a' + c) with more hops on the
// cheaper side), so a single label-correcting pass on (cost, hops) could keep the hops of a stale, dearer
// prefix.  Hence two passes of the same relaxation:
//   pass 1  keys (cost, hops) over all edges: the cost words are the least folds;
//   pass 2  keys again, over "tight" edges only (fl(cost[u] + c) == cost[v]): every key now has its final cost,
//           the hop extension h -> h + 1 is monotone, and the hops are the BFS depths of the tight subgraph --
//           which is exactly what a host Dijkstra on the (cost, hops) key computes.
//
// Relaxation: near-far, label-correcting.  A round expands the near queue with one 16-lane group per node
// (rows longer than 16 loop); an improved target goes to the next near queue when its cost is below the
// bucket's threshold, else to the far pile.  A round that pushes nothing near opens the next bucket
// [least live far cost, + delta) from the far pile.  Pushes are deduplicated by per-round / per-bucket
// stamps and reserved with one atomicAdd per wave (ballot + prefix).  No launch waits for another
// workgroup: sizes are read from device memory, the host enqueues rounds in batches.
//
// Batches: m fields are one field of the disjoint union of m copies of the graph with m sources -- still one
// least fixed point, so the same relaxation, with ONE threshold, phase, far-pile selector and round counter for
// the union, reaches it.  A work item is (field k, node v) = k * V + v; queues, piles, stamps, keys and parents
// are per item, the CSR and the edge costs are shared.  The relax loop decodes an item once (one 32-bit
// division, MULTI only) and adds the field's first item to every column it reads; with m == 1 the template
// drops both.  The other kernels either never look inside an item (far min, far split, cost bits) or take the
// field from blockIdx.y.
//
// Bounded solves ("Bounded fields"): field k is truncated at a bound, its budget lowered
// by the settle step once its targets are settled -- every node dearer than the bound comes out unreached, every
// other node as in the full field.  Pass 1 runs the BOUNDED instantiations of the round kernels with the settle
// step between far min and far split, and ends with the keys above the bounds removed; pass 2 and everything after
// it are the plain kernels.  A solve without bounds launches none of this.
//
// Source sets ("Source sets"): a field may start from a set of nodes, every member at key
// (0, 0) -- the same least fixed point with more seeds, so the round kernels are the plain ones; only the seeding
// differs.  After the parent sweep every reached node hangs on exactly one member through its parents; the owner
// pass finds that member by pointer jumping, in sweeps logarithmic in the greatest hop count.  A single source is a
// set of one whose owner is known without that pass: both kinds share k_field_init (which seeds single sources
// itself and leaves sets to k_field_seed), k_field_gather (the owners at the targets where there are any) and the
// route walk (which differs in where a walk must end); k_field_seed and the owner pass a solve from single
// sources never launches.
//
// Start costs ("Start costs"): a set entry may start at a cost of its own -- the field from a
// virtual node joined to the members by arcs of those costs, still one least fixed point.  Only k_field_seed knows:
// its COST0 instantiation seeds entry e at (cost0[e], 0), in pass 2 only where that is the item's least cost, so that
// the member marks name the roots; the relaxation, the owner pass and the route walk are the set solve's.
//
// Refresh ("Refresh"): the keys of a solve on an earlier graph, carried through a node map,
// are starting points on the current one once the anchor has dropped every key that is not a walk's of the current
// graph: the supporter forest of k_field_parent, pointer-jumped as the owner pass jumps the parents (one begin kernel,
// k_field_forest_begin, and one sweep for both), keeps what hangs on a source.  The carried keys enter through
// k_field_init, in the place of "no key".  Both passes then start warm -- k_field_warm_seed queues every item one
// of whose edges improves its target, the round kernels run as they are -- with a second anchor between them that
// cuts every key pass 1 changed, so that the hops pass 2 starts from are those of tight walks.  The relaxation
// kernels know nothing of this.
//
// Cost models ("Cost models"): the fields of a solve need not price an edge alike -- nothing in
// the argument above asks the copies of the union to carry the same costs.  The costs of a solve's distinct models
// lie in slots of one array; the four kernels that read an edge cost (relax, parent sweep, route walk, warm seed)
// have a MODELS instantiation that takes the slot from the item's field, one table read per queued item or route.
// A solve whose fields share one model runs the plain instantiations on that slot.
//
// Keep-out zones ("Keep-out zones"): a field may also refuse edges by place -- every edge that a
// disc of its zone set touches.  That is one more reason for the skip marker in a slot, decided by k_field_edge_zones
// (near the end of this file) where k_field_edge_cost decides by weight, and by k_field_edge_risk_zones for a slot of
// edge risks; every kernel that reads a slot is unchanged.
//
// Risk fields ("Risk fields"): the least, over all walks, of the GREATEST edge weight on the walk.
// The extension is (max(risk, r), hops + 1) with r = w + 0 -- monotone in the risk word and never below it, which is
// all the argument above asks of fl(a + c), and it never rounds.  The hop word is no more monotone than under
// rounding (a < a' gives max(a, r) == max(a', r) for every r >= a'), so the two passes stay.  The kernels that read an
// edge value (relax, parent sweep, route walk, warm seed) have a RISK instantiation whose only difference is that
// extension.  The edge risks lie in a slot of the edge-cost array (k_field_edge_risk); every kernel that looks at cost
// bits only is used as it is.  RISK combines with MODELS where the fields of a risk solve read different slots: a risk
// solve has no cost model, but its fields may avoid different keep-out zones ("Keep-out zones on
// risk fields"; k_field_edge_risk_zones fills such a slot), and the slot table is the same.  A risk solve is
// refreshed by the steps of the cost refresh ("Risk fields"): carry, anchors, warm init, rounds
// and finish look at key bits only or have their RISK form, and the RISK warm seed queues by the maximum.  A bucket
// width of 0 (all-zero weights) takes the warm control block, which starts at threshold 0, down the path of a cold one:
// every push goes far, and next_threshold opens the bucket one word above the least live risk.
//
// Across tiles ("Cost fields across tiles"; trg_field_tiled.inc, included at the end): the field
// of the stitched global graph, each rank relaxing its own rows plus mirrors of the other ends of its cross edges and
// trading border keys between runs of the round kernels -- one more relaxation order to the same fixed point.  The
// round kernels run on that rank's solve graph as they are; the tiled kernels build the graph, seed, publish, merge
// and take the parents as least GLOBAL ids.  A risk field across tiles ("Risk fields across tiles") is the same run with
// launch_field_round(.., risk = true) on the edge risks of that graph.
//
// Compiled with -ffp-contract=off (build.sh): a cost is one fp32 multiply, add, multiply; a fold one add.
#include "trg_kernels.h"

#include <limits.h>

#include <algorithm>
#include <type_traits>

namespace trg {

namespace {

constexpr int WAVE = 64;
constexpr int GROUP = 16;    // lanes per queued node
constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 512;

__device__ __forceinline__ int lane_id() { return threadIdx.x & (WAVE - 1); }

__device__ __forceinline__ unsigned long long ballot(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }

// the key of a walk extended by an edge of cost c: (fl(cost + c), hops + 1); RISK: by an edge of risk c (>= +0, no
// NaN: a select gives the greater word as it is), (max(risk, c), hops + 1)
template <bool RISK = false>
__device__ __forceinline__ unsigned long long key_extend(unsigned long long k, float c) {
  const float a = __uint_as_float((unsigned)(k >> 32));
  const float g = RISK ? (c > a ? c : a) : a + c;
  return ((unsigned long long)__float_as_uint(g) << 32) | (unsigned)((unsigned)k + 1u);
}

__device__ __forceinline__ float key_cost(unsigned long long k) { return __uint_as_float((unsigned)(k >> 32)); }

// The slot of this lane in a queue whose tail is *tail: one atomicAdd per wave for all its pushing lanes.
// Called by every lane of the wave (convergent); the result is meaningful where pred.
__device__ __forceinline__ int wave_reserve(bool pred, int *tail) {
  const unsigned long long m = ballot(pred);
  if (m == 0) return 0;
  const int leader = __ffsll((unsigned long long)m) - 1;
  int base = 0;
  if (lane_id() == leader) base = atomicAdd(tail, __popcll(m));
  base = __shfl(base, leader);
  return base + __popcll(m & ((1ull << lane_id()) - 1ull));
}

__device__ __forceinline__ unsigned key_cost_bits(unsigned long long k) { return (unsigned)(k >> 32); }

// The next bucket's threshold above the least live far cost (strictly above it, whatever delta is).  Thresholds
// are kept and compared as bits: costs are >= +0, so their bits order as they do, and the word after a least
// cost of +inf (no float: a NaN pattern) is still a threshold that +inf lies below.
__device__ __forceinline__ unsigned next_threshold(unsigned fminb, float delta) {
  const float fmin = __uint_as_float(fminb);
  const float t = fmin + delta;
  return t > fmin ? __float_as_uint(t) : fminb + 1u;
}

// (bounded solves) the bound of the field that item i belongs to, as cost bits
__device__ __forceinline__ unsigned field_bound(const FieldDev &F, int i) {
  return F.ctrl->bound[(unsigned)i / (unsigned)F.V];
}

// what a kernel with a MODELS parameter takes last: the slot table, or nothing
struct FieldNoModels {};
template <bool MODELS>
using FieldModelsArg = std::conditional_t<MODELS, FieldModels, FieldNoModels>;

// the edge costs that field f reads
template <bool MODELS>
__device__ __forceinline__ const float *field_costs(const FieldDev &F, const FieldModelsArg<MODELS> &M, int f) {
  if constexpr (MODELS) return F.ec + (long long)M.slot[f] * M.stride;
  else return F.ec;
}

__global__ __launch_bounds__(THREADS) void k_field_edge_cost(const int *__restrict__ col, const float *__restrict__ w,
                                                             const float *__restrict__ dist,
                                                             const int *__restrict__ state, int V, int E, float sf,
                                                             float tau, float *__restrict__ ec, FieldEdgeStats *st) {
  double sum = 0.0;
  int cnt = 0, bad = 0;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < E; k += gridDim.x * blockDim.x) {
    const float c = (sf * w[k] + 1.0f) * dist[k];
    if (!(c >= 0.0f) || c == __builtin_huge_valf()) bad = 1;
    const int v = col[k];
    bool skip = v < 0 || v >= V;
    if (!skip) skip = state[v] == FIELD_NODE_INVALID;
    skip = skip || w[k] > tau;  // (the ceiling; +inf: no weight is above it)
    ec[k] = skip ? __uint_as_float(FIELD_EDGE_SKIP) : c;
    if (!skip) {
      sum += (double)c;
      cnt++;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sum += __shfl_xor(sum, m);
    cnt += __shfl_xor(cnt, m);
    bad |= __shfl_xor(bad, m);
  }
  if (lane_id() == 0) {
    if (cnt) {
      atomicAdd(&st->sum, sum);
      atomicAdd(&st->count, cnt);
    }
    if (bad) atomicOr(&st->bad, 1);
  }
}

// Risk fields: r[e] = w[e] + 0 (a weight of -0 counts as +0), FIELD_EDGE_SKIP for an edge that is not relaxable; the
// sum and count over relaxable edges, and `bad` over ALL edges for a weight that is NaN, negative or infinite.
__global__ __launch_bounds__(THREADS) void k_field_edge_risk(const int *__restrict__ col, const float *__restrict__ w,
                                                             const int *__restrict__ state, int V, int E,
                                                             float *__restrict__ er, FieldEdgeStats *st) {
  double sum = 0.0;
  int cnt = 0, bad = 0;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < E; k += gridDim.x * blockDim.x) {
    const float r = w[k] + 0.0f;
    if (!(r >= 0.0f) || r == __builtin_huge_valf()) bad = 1;
    const int v = col[k];
    bool skip = v < 0 || v >= V;
    if (!skip) skip = state[v] == FIELD_NODE_INVALID;
    er[k] = skip ? __uint_as_float(FIELD_EDGE_SKIP) : r;
    if (!skip) {
      sum += (double)r;
      cnt++;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sum += __shfl_xor(sum, m);
    cnt += __shfl_xor(cnt, m);
    bad |= __shfl_xor(bad, m);
  }
  if (lane_id() == 0) {
    if (cnt) {
      atomicAdd(&st->sum, sum);
      atomicAdd(&st->count, cnt);
    }
    if (bad) atomicOr(&st->bad, 1);
  }
}

// The control block before the first round of a pass (one thread): `queued` items in near queue 0, as much work,
// nothing else queued or piled, the near bucket below `thr`, phase 1.
__device__ __forceinline__ void field_ctrl_reset(const FieldDev &F, unsigned thr, float delta, int queued) {
  FieldCounters &c = F.ctrl->c;
  c.n[0] = queued;
  c.n[1] = 0;
  c.nfar[0] = c.nfar[1] = 0;
  c.fmin = ~0u;
  c.overflow = 0;
  FieldState &s = F.ctrl->s;
  s.work = queued;
  s.rounds = 0;
  s.overflow = 0;
  s.thr = thr;
  s.delta = delta;
  s.phase = 1;
  s.far_sel = 0;
}

// grid.y = field.  `single`: field f starts at node S.id[f], keyed (0, 0) and queued here; else (a set solve) no
// item is a source and the near queue is empty, for k_field_seed.  Every other item gets no key, or, with `carried`
// (a refresh; per item), its carried one.  The control block of a carried init is the cold one all the same: no
// launch reads it before k_field_warm_init writes every word of it again (k_field_seed only adds to the queue size
// and the work), and the first anchor overwrites q[0].
__global__ __launch_bounds__(THREADS) void k_field_init(FieldDev F, FieldSources S, float delta, bool single,
                                                        const unsigned long long *__restrict__ carried) {
  const int V = F.V;
  const int f = blockIdx.y;
  const int src = single ? S.id[f] : -1;
  const int fbase = f * V;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
    F.key[fbase + v] = v == src ? 0ull : carried ? carried[fbase + v] : FIELD_KEY_NONE;
    F.parent[fbase + v] = INT_MAX;
    F.stamp_near[fbase + v] = 0;
    F.stamp_far[fbase + v] = 0u;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (single) F.q[0][f] = fbase + src;
    F.ctrl->reached[f] = 0;
  }
  if (blockIdx.x == 0 && f == 0 && threadIdx.x == 0)
    field_ctrl_reset(F, __float_as_uint(delta), delta, single ? F.m : 0);
}

// Expand the near queue of this round: one 16-lane group per queued item, four per wave.
// MULTI: more than one field (an item is decoded into its field's first item and its node); else item == node.
// BOUNDED: pass 1 of a bounded solve -- an item above its field's bound is not expanded (it was queued before the
// settle step lowered the bound), an extension above the bound is neither written nor pushed.
// MODELS (with MULTI): the edge costs are those of the item's field.
// RISK: a risk field -- the slot holds edge risks, the extension is the maximum; with MODELS, fields under different
// keep-out zone lists.
template <bool MULTI, bool BOUNDED, bool MODELS, bool RISK = false>
__global__ __launch_bounds__(THREADS) void k_field_relax(FieldDev F, int par, int stamp, FieldModelsArg<MODELS> M) {
  static_assert(MULTI || !MODELS, "one field has one model: the host points F.ec at its slot");
  const int N = MULTI ? F.N : F.V;
  const int n = min(F.ctrl->c.n[par], N);  // (past N only after an overflow, which the host then reports)
  if (n == 0) return;
  const unsigned thr = F.ctrl->s.thr;
  const unsigned phase = F.ctrl->s.phase;
  const int fs = F.ctrl->s.far_sel;
  const int *__restrict__ q_cur = F.q[par];
  int *q_next = F.q[par ^ 1];
  int *far = F.far[fs];
  int *next_tail = &F.ctrl->c.n[par ^ 1];
  int *far_tail = &F.ctrl->c.nfar[fs];
  const int sub = threadIdx.x & (GROUP - 1);
  const int gw = lane_id() / GROUP;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int nwaves = gridDim.x * blockDim.x / WAVE;
  constexpr int PER_WAVE = WAVE / GROUP;
  for (int base = wave * PER_WAVE; base < n; base += nwaves * PER_WAVE) {  // (wave-uniform)
    const int item = base + gw;
    unsigned long long ku = 0;
    int k = 0, kend = 0;
    int fbase = 0;  // the first item of the queued item's field
    unsigned bnd = 0;  // (BOUNDED) that field's bound
    const float *__restrict__ ec = F.ec;
    if (item < n) {
      const int iu = q_cur[item];
      ku = F.key[iu];
      int u = iu;
      int f = 0;
      if constexpr (MULTI) {
        f = (int)((unsigned)iu / (unsigned)F.V);
        fbase = f * F.V;
        u = iu - fbase;
      }
      ec = field_costs<MODELS>(F, M, f);
      if constexpr (BOUNDED) bnd = F.ctrl->bound[f];
      if (!BOUNDED || key_cost_bits(ku) <= bnd) {
        k = F.rowptr[u] + sub;
        kend = F.rowptr[u + 1];
      }
    }
    for (;; k += GROUP) {
      const bool act = k < kend;
      if (ballot(act) == 0) break;  // (wave-uniform: the longest row of the wave's four)
      bool to_near = false, to_far = false;
      int v = 0;
      if (act) {
        const float c = ec[k];
        if (__float_as_uint(c) != FIELD_EDGE_SKIP) {
          v = F.col[k];
          if constexpr (MULTI) v += fbase;  // the target item: an edge never leaves its field
          const unsigned long long nk = key_extend<RISK>(ku, c);
          const bool tight = !F.tight || (unsigned)(nk >> 32) == F.tight[v];  // (pass 2: tight edges only)
          const bool within = !BOUNDED || key_cost_bits(nk) <= bnd;
          if (tight && within && nk < F.key[v]) {  // plain load first: the atomic only on an improvement
            const unsigned long long old = atomicMin(&F.key[v], nk);
            if (nk < old) {
              if (key_cost_bits(nk) < thr)
                to_near = atomicExch(&F.stamp_near[v], stamp) != stamp;
              else
                to_far = atomicExch(&F.stamp_far[v], phase) != phase;
            }
          }
        }
      }
      const int sn = wave_reserve(to_near, next_tail);
      if (to_near) {
        if (sn < N) q_next[sn] = v;
        else atomicOr(&F.ctrl->c.overflow, 1);
      }
      const int sf = wave_reserve(to_far, far_tail);
      if (to_far) {
        if (sf < N) far[sf] = v;
        else atomicOr(&F.ctrl->c.overflow, 1);
      }
    }
  }
}

// The least live cost of the far pile, over all fields (live: not below the threshold; an entry below it was
// pushed near and expanded since) -- only when this round's relaxation pushed nothing near in any field.
// BOUNDED: an entry above its field's bound is not live either -- else a field that the settle step stopped would
// keep opening buckets of nothing until its pile drained.
template <bool BOUNDED>
__global__ __launch_bounds__(THREADS) void k_field_far_min(FieldDev F, int par) {
  if (F.ctrl->c.n[par ^ 1] != 0) return;
  const int fs = F.ctrl->s.far_sel;
  const int nf = min(F.ctrl->c.nfar[fs], F.N);
  const unsigned thr = F.ctrl->s.thr;
  const int *__restrict__ far = F.far[fs];
  unsigned best = ~0u;
  const int n_iter = (nf + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, i = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, i += gridDim.x * blockDim.x) {
    if (i < nf) {
      const int v = far[i];
      const unsigned c = key_cost_bits(F.key[v]);
      if (c >= thr && (!BOUNDED || c <= field_bound(F, v))) best = min(best, c);
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, m));
  if (lane_id() == 0 && best != ~0u) atomicMin(&F.ctrl->c.fmin, best);
}

// Open the next bucket: live far entries below the new threshold go to the (empty) next near queue, the
// rest to the other far pile, stamped with the next phase.
// (Whether to split is told by fmin, which only k_field_far_min sets: the near-queue size changes here.)
template <bool BOUNDED>
__global__ __launch_bounds__(THREADS) void k_field_far_split(FieldDev F, int par) {
  const unsigned fminb = F.ctrl->c.fmin;
  if (fminb == ~0u) return;
  const int fs = F.ctrl->s.far_sel;
  const int nf = min(F.ctrl->c.nfar[fs], F.N);
  const unsigned thr = F.ctrl->s.thr;
  const unsigned thr_new = next_threshold(fminb, F.ctrl->s.delta);
  const unsigned phase_new = F.ctrl->s.phase + 1u;
  const int N = F.N;
  const int *__restrict__ far = F.far[fs];
  int *far_new = F.far[fs ^ 1];
  int *q_next = F.q[par ^ 1];
  const int n_iter = (nf + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, i = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, i += gridDim.x * blockDim.x) {
    bool to_near = false, to_far = false;
    int v = 0;
    if (i < nf) {
      v = far[i];
      const unsigned c = key_cost_bits(F.key[v]);
      if (c >= thr && (!BOUNDED || c <= field_bound(F, v))) {
        to_near = c < thr_new;  // (thr_new > fmin: the least live cost always makes progress, +inf too)
        to_far = !to_near;
      }
    }
    const int sn = wave_reserve(to_near, &F.ctrl->c.n[par ^ 1]);
    if (to_near) {
      if (sn < N) q_next[sn] = v;
      else atomicOr(&F.ctrl->c.overflow, 1);
    }
    const int sf = wave_reserve(to_far, &F.ctrl->c.nfar[fs ^ 1]);
    if (to_far) {
      F.stamp_far[v] = phase_new;
      if (sf < N) far_new[sf] = v;
      else atomicOr(&F.ctrl->c.overflow, 1);
    }
  }
}

// One thread: the next near queue becomes the current one; a split switches the far pile and the bucket.
// BOUNDED: the least live far cost was found before the settle step ran, so a split may have moved nothing near
// (that cost's field was stopped) and yet have left live entries of other fields in the far pile: they are work.
template <bool BOUNDED>
__global__ void k_field_round_end(FieldDev F, int par) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  FieldCounters &c = F.ctrl->c;
  FieldState &s = F.ctrl->s;
  const bool worked = c.n[par] != 0;
  c.n[par] = 0;
  if (c.fmin != ~0u) {  // the bucket was opened from the far pile
    c.nfar[s.far_sel] = 0;
    s.far_sel ^= 1;
    s.phase += 1u;
    s.thr = next_threshold(c.fmin, s.delta);
    c.fmin = ~0u;
  } else if (c.n[par ^ 1] == 0) {
    c.nfar[s.far_sel] = 0;  // converged: what is left in the far pile is stale
  }
  if (worked) s.rounds++;
  s.work = c.n[par ^ 1];
  if constexpr (BOUNDED) s.work += c.nfar[s.far_sel];
  s.overflow = c.overflow;
}

// ---- bounded fields ("Bounded fields") ---------------------------------------------------

__global__ void k_field_bounds(FieldDev F, FieldBounds B) {
  if (blockIdx.x == 0 && threadIdx.x < F.m) F.ctrl->bound[threadIdx.x] = B.bits[threadIdx.x];
}

// The settle step, one block per field, between k_field_far_min and k_field_far_split of a round that pushed
// nothing near: the near queue is empty, so every key below the least live far cost fmin (every key, when nothing
// is live: convergence) is final, and every other key of the union lies at or above fmin.  A target is settled
// when it has a key below fmin.  ANY: the least cost of the settled targets is the least over all targets.  ALL,
// when every target is settled: their greatest cost.  The field's bound drops to that cost; only this block
// writes the word, and no other kernel runs beside it.
__global__ __launch_bounds__(THREADS) void k_field_settle(FieldDev F, int par, const int *__restrict__ targets,
                                                          int n_t, int mode) {
  if (F.ctrl->c.n[par ^ 1] != 0) return;
  __shared__ unsigned s_lo[THREADS / WAVE], s_hi[THREADS / WAVE];
  __shared__ int s_unmet[THREADS / WAVE];
  const unsigned fmin = F.ctrl->c.fmin;
  const int fbase = blockIdx.x * F.V;
  unsigned lo = ~0u, hi = 0u;
  int unmet = 0;
  for (int j = threadIdx.x; j < n_t; j += blockDim.x) {
    const unsigned long long k = F.key[fbase + targets[j]];
    const unsigned c = key_cost_bits(k);
    if (k != FIELD_KEY_NONE && c < fmin) {
      lo = min(lo, c);
      hi = max(hi, c);
    } else {
      unmet = 1;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lo = min(lo, (unsigned)__shfl_xor((int)lo, m));
    hi = max(hi, (unsigned)__shfl_xor((int)hi, m));
    unmet |= __shfl_xor(unmet, m);
  }
  if (lane_id() == 0) {
    s_lo[threadIdx.x / WAVE] = lo;
    s_hi[threadIdx.x / WAVE] = hi;
    s_unmet[threadIdx.x / WAVE] = unmet;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < THREADS / WAVE; ++w) {
      lo = min(lo, s_lo[w]);
      hi = max(hi, s_hi[w]);
      unmet |= s_unmet[w];
    }
    unsigned b = ~0u;
    if (mode == FIELD_SETTLE_ANY && lo != ~0u) b = lo;
    if (mode == FIELD_SETTLE_ALL && !unmet && n_t > 0) b = hi;
    if (b < F.ctrl->bound[blockIdx.x]) F.ctrl->bound[blockIdx.x] = b;
  }
}

// grid.y = field: after pass 1, a key above its field's bound is no key
__global__ __launch_bounds__(THREADS) void k_field_trim(FieldDev F) {
  const int fbase = blockIdx.y * F.V;
  const unsigned bnd = F.ctrl->bound[blockIdx.y];
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < F.V; v += gridDim.x * blockDim.x) {
    const unsigned long long k = F.key[fbase + v];
    if (k != FIELD_KEY_NONE && key_cost_bits(k) > bnd) F.key[fbase + v] = FIELD_KEY_NONE;
  }
}

// The reached list of one field: block b covers the nodes [b * THREADS, (b + 1) * THREADS).  Count per block, an
// exclusive scan of the counts (launch_exclusive_scan), then every block writes its nodes from its offset on, in
// id order: a wave's lanes by the ballot's prefix, the block's waves by the sums of the waves before.
__global__ __launch_bounds__(THREADS) void k_field_list_count(FieldDev F, int field, int *counts) {
  __shared__ int s_n[THREADS / WAVE];
  const int v = blockIdx.x * THREADS + threadIdx.x;
  const bool has = v < F.V && F.key[field * F.V + v] != FIELD_KEY_NONE;
  const unsigned long long m = ballot(has);
  if (lane_id() == 0) s_n[threadIdx.x / WAVE] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int w = 0; w < THREADS / WAVE; ++w) n += s_n[w];
    counts[blockIdx.x] = n;
  }
}

__global__ __launch_bounds__(THREADS) void k_field_list_emit(FieldDev F, int field, const int *__restrict__ offsets,
                                                             int cap, int *ids, float *cost, int *hops) {
  __shared__ int s_n[THREADS / WAVE];
  const int v = blockIdx.x * THREADS + threadIdx.x;
  unsigned long long k = FIELD_KEY_NONE;
  if (v < F.V) k = F.key[field * F.V + v];
  const bool has = k != FIELD_KEY_NONE;
  const unsigned long long m = ballot(has);
  if (lane_id() == 0) s_n[threadIdx.x / WAVE] = __popcll(m);
  __syncthreads();
  int pos = offsets[blockIdx.x] + __popcll(m & ((1ull << lane_id()) - 1ull));
  for (int w = 0; w < (int)threadIdx.x / WAVE; ++w) pos += s_n[w];
  if (has && pos < cap) {
    if (ids) ids[pos] = v;
    if (cost) cost[pos] = key_cost(k);
    if (hops) hops[pos] = (int)(unsigned)k;
  }
}

// Parents: the smallest u with an edge u -> v whose extension of key[u] is key[v], in each field (grid.y).
template <bool MODELS, bool RISK = false>
__global__ __launch_bounds__(THREADS) void k_field_parent(FieldDev F, FieldModelsArg<MODELS> M) {
  const float *__restrict__ ec = field_costs<MODELS>(F, M, blockIdx.y);
  const int sub = threadIdx.x & (GROUP - 1);
  const int g0 = (blockIdx.x * blockDim.x + threadIdx.x) / GROUP;
  const int ng = gridDim.x * blockDim.x / GROUP;
  const int fbase = blockIdx.y * F.V;
  for (int u = g0; u < F.V; u += ng) {
    const unsigned long long ku = F.key[fbase + u];
    if (ku == FIELD_KEY_NONE) continue;
    for (int k = F.rowptr[u] + sub, kend = F.rowptr[u + 1]; k < kend; k += GROUP) {
      const float c = ec[k];
      if (__float_as_uint(c) == FIELD_EDGE_SKIP) continue;
      const int v = fbase + F.col[k];
      if (key_extend<RISK>(ku, c) == F.key[v]) atomicMin(&F.parent[v], u);
    }
  }
}

// grid.y = field: a wave's items are of one field, one atomicAdd per wave into its count
__global__ __launch_bounds__(THREADS) void k_field_output(FieldDev F, float *cost, int *hops) {
  const int V = F.V;
  const int fbase = blockIdx.y * V;
  const int n_iter = (V + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, v = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, v += gridDim.x * blockDim.x) {
    bool reached = false;
    if (v < V) {
      const unsigned long long k = F.key[fbase + v];
      reached = k != FIELD_KEY_NONE;
      cost[fbase + v] = reached ? key_cost(k) : __builtin_huge_valf();
      hops[fbase + v] = reached ? (int)(unsigned)k : -1;
      if (F.parent[fbase + v] == INT_MAX) F.parent[fbase + v] = -1;
    }
    const unsigned long long m = ballot(reached);
    if (lane_id() == 0 && m) atomicAdd(&F.ctrl->reached[blockIdx.y], __popcll(m));
  }
}

// pass 1 -> pass 2: the least costs as bits (unreached: ~0)
__global__ __launch_bounds__(THREADS) void k_field_cost_bits(FieldDev F, unsigned *bits) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < F.N; i += gridDim.x * blockDim.x)
    bits[i] = (unsigned)(F.key[i] >> 32);
}

// The finished keys at the target nodes, in each field (grid.y); with `owner` (a set solve's, per item) the
// targets' owners as well.
__global__ __launch_bounds__(THREADS) void k_field_gather(FieldDev F, const int *__restrict__ targets, int n_t,
                                                          float *cost_at, int *hops_at,
                                                          const int *__restrict__ owner, int *owner_at) {
  const int fbase = blockIdx.y * F.V;
  const long long obase = (long long)blockIdx.y * n_t;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n_t; j += gridDim.x * blockDim.x) {
    const unsigned long long k = F.key[fbase + targets[j]];
    const bool reached = k != FIELD_KEY_NONE;
    if (cost_at) cost_at[obase + j] = reached ? key_cost(k) : __builtin_huge_valf();
    if (hops_at) hops_at[obase + j] = reached ? (int)(unsigned)k : -1;
    if (owner_at) owner_at[obase + j] = owner[fbase + targets[j]];
  }
}

// The lazy parent sweep of a solve that skipped it: every parent word equal to `from` becomes `to`
// (-1 -> INT_MAX before k_field_parent, INT_MAX -> -1 after it, as k_field_init / k_field_output leave them).
__global__ __launch_bounds__(THREADS) void k_field_parent_mark(FieldDev F, int from, int to) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < F.N; i += gridDim.x * blockDim.x)
    if (F.parent[i] == from) F.parent[i] = to;
}

// Route lengths: hops + 1 at (field, target), 0 where the target has no key.
__global__ __launch_bounds__(THREADS) void k_field_route_len(FieldDev F, const int *__restrict__ route_field,
                                                             const int *__restrict__ route_target, int n_routes,
                                                             int *len) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_routes; r += gridDim.x * blockDim.x) {
    const unsigned long long k = F.key[route_field[r] * F.V + route_target[r]];
    len[r] = k == FIELD_KEY_NONE ? 0 : (int)(unsigned)k + 1;
  }
}

// Routes ("Routes"): one 16-lane group per route, grid-stride.  The group walks the parents
// from the target back to the source -- hops[target] steps, the hops drop by one per step -- and writes the node
// ids at descending positions of the route's segment [offsets[r], offsets[r + 1]) (a truncated segment keeps the
// source end; the sums cover the whole route).  The route edge into v from its parent u is the least CSR index
// of row u with col == v, a cost that is not the skip marker and key_extend(key[u], ec) == key[v]: the lanes
// read 16 consecutive entries per trip, so the lowest matching lane of the first trip with a match is that
// edge.  Everything the loops branch on is uniform over the group; the ballot is masked to the group's lanes.
// A walk that loses its way -- a parent out of range, no route edge, an end that is not where it must end; none
// can happen on the keys and parents of a finished solve -- reports num_nodes = FIELD_ROUTE_BROKEN, which the
// host turns into an error, instead of a route that looks right.
// Where it must end is all that SETS changes: at the field's source S.id[field], or, for a set solve (S its sets,
// the owner pass has run), at the member that owns the target, ids[ptr[field] + owner[target]].  The single-source
// instantiation has no owner array to read.  MODELS: the edge costs are those of the route's field.  RISK (with
// MODELS: under a zone list per field): the retained solve is a risk solve -- the matching extension is the maximum,
// `cost` the risk word.
template <bool SETS, bool MODELS, bool RISK = false>
__global__ __launch_bounds__(THREADS) void k_field_route_walk(FieldDev F, const float *__restrict__ w,
                                                              const float *__restrict__ dist,
                                                              const int *__restrict__ route_field,
                                                              const int *__restrict__ route_target, int n_routes,
                                                              const int *__restrict__ offsets, int *node_ids,
                                                              FieldRouteInfo *infos,
                                                              std::conditional_t<SETS, FieldSets, FieldSources> S,
                                                              FieldModelsArg<MODELS> M) {
  const int V = F.V;
  const int sub = threadIdx.x & (GROUP - 1);
  const int gshift = lane_id() & ~(GROUP - 1);  // the group's first lane within the wave
  const int g0 = (blockIdx.x * blockDim.x + threadIdx.x) / GROUP;
  const int ng = gridDim.x * blockDim.x / GROUP;
  for (int r = g0; r < n_routes; r += ng) {
    const int fbase = route_field[r] * V;
    const float *__restrict__ ec = field_costs<MODELS>(F, M, route_field[r]);
    int v = route_target[r];
    unsigned long long kv = F.key[fbase + v];
    FieldRouteInfo out;
    out.num_nodes = 0;
    out.cost = __builtin_huge_valf();
    out.path_length = 0.0f;
    out.avg_risk = 0.0f;
    if (kv != FIELD_KEY_NONE) {
      const int h = (int)(unsigned)kv;
      const int off = node_ids ? offsets[r] : 0;
      const int room = node_ids ? offsets[r + 1] - off : 0;
      float sum_dist = 0.0f, sum_w = 0.0f;
      bool broken = false;
      for (int i = h;; --i) {
        if (sub == 0 && i < room) node_ids[off + i] = v;
        if (i == 0) break;
        const int u = F.parent[fbase + v];
        if (u < 0 || u >= V) {  // (never for a node with a key and hops > 0: the parent sweep ran)
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
        if (edge < 0) {  // (never: the parent is a node with such an edge)
          broken = true;
          break;
        }
        sum_dist += dist[edge];
        sum_w += w[edge];
        v = u;
        kv = ku;
      }
      if constexpr (SETS) {  // h steps back from the target end at the member that owns it
        const int o = S.owner[fbase + route_target[r]];
        const int e = S.ptr[route_field[r]] + o;
        if (o < 0 || e >= S.n || v != S.ids[e]) broken = true;
      } else {  // ... at the source
        if (v != S.id[route_field[r]]) broken = true;
      }
      out.num_nodes = broken ? FIELD_ROUTE_BROKEN : h + 1;
      out.cost = key_cost(F.key[fbase + route_target[r]]);
      out.path_length = sum_dist;
      out.avg_risk = sum_w / (float)(h + 1);
    }
    if (sub == 0 && infos) infos[r] = out;
  }
}

// ---- source sets ("Source sets") ----------------------------------------------------------

// what k_field_seed takes last: the start costs of a seeded solve, or nothing
struct FieldNoCost0 {};
template <bool COST0>
using FieldCost0Arg = std::conditional_t<COST0, const unsigned *, FieldNoCost0>;

// One thread per entry of all sets: its item gets key (0, 0) and the least entry that names it (atomicMin on the
// member word, see FieldSets); the entry that finds the word unmarked pushes the item, so a duplicate is queued
// once.  The queue size and `work` grow by one atomicAdd per wave each.
// COST0 ("Start costs"): entry e starts at key (cost0[e], 0), cost bits.  Pass 1: the item's
// key is the least of its entries' (atomicMin), and it is queued in near queue 0 whatever its cost; the relaxation
// may improve it and then overwrites its mark, which nobody reads before pass 2 seeds again.  Pass 2 (F.tight):
// only an entry whose start cost is the item's least cost seeds it -- the item is a root, no tight extension is
// below (cost, 0), so its mark stays and names the least such entry; every other member is an ordinary node.
template <bool COST0>
__global__ __launch_bounds__(THREADS) void k_field_seed(FieldDev F, FieldSets S, FieldCost0Arg<COST0> cost0) {
  const int n_iter = (S.n + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, e = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, e += gridDim.x * blockDim.x) {
    bool first = false;
    int item = 0;
    if (e < S.n) {
      int lo = 0, hi = F.m;  // the set of entry e: the last k with ptr[k] <= e
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (S.ptr[mid] <= e) lo = mid;
        else hi = mid;
      }
      item = lo * F.V + S.ids[e];
      if constexpr (COST0) {
        const unsigned c0 = cost0[e];
        const unsigned long long k0 = (unsigned long long)c0 << 32;
        if (!F.tight) {
          atomicMin(&F.key[item], k0);
          first = atomicMin(&F.stamp_near[item], FIELD_MEMBER | e) >= 0;
        } else if (c0 == F.tight[item]) {
          F.key[item] = k0;  // (every entry that gets here writes this word)
          first = atomicMin(&F.stamp_near[item], FIELD_MEMBER | e) >= 0;
        }
      } else {
        F.key[item] = 0ull;
        first = atomicMin(&F.stamp_near[item], FIELD_MEMBER | e) >= 0;
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

// is item i (node v of field f) a source: a member of its set by its mark (FieldSets), else its field's one source
__device__ __forceinline__ bool field_is_source(const FieldDev &F, const FieldSources &S, bool single, int f, int v) {
  return single ? v == S.id[f] : F.stamp_near[f * F.V + v] < 0;
}

// grid.y = field: the first ancestor of every item in the forest that k_field_parent left in F.parent -- itself for
// a source, its parent's (supporter's) item for another item with a key, -1 without one or without a supporter.
// The owner pass of a set solve and both anchors of a refresh begin here.  With key0 (the second anchor) an item
// whose key is no longer key0's is cut: -1.
__global__ __launch_bounds__(THREADS) void k_field_forest_begin(FieldDev F, FieldSources S, bool single,
                                                                const unsigned long long *__restrict__ key0) {
  const int fbase = blockIdx.y * F.V;
  int *anc = F.q[0];
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < F.V; v += gridDim.x * blockDim.x) {
    const int i = fbase + v;
    const unsigned long long k = F.key[i];
    int a = -1;
    if (k != FIELD_KEY_NONE && (!key0 || k == key0[i])) {
      const int p = F.parent[i];
      a = field_is_source(F, S, single, blockIdx.y, v) ? i : (p >= 0 && p < F.V ? fbase + p : -1);
    }
    anc[i] = a;
  }
}

// One pointer-jumping sweep: out[i] = in[in[i]].  `in` is only read and `out` only written in this launch, so no
// workgroup reads a word another one writes; *changed is set (to the one value anybody stores) when an entry moved.
__global__ __launch_bounds__(THREADS) void k_field_owner_sweep(const int *__restrict__ in, int *__restrict__ out,
                                                               int N, int *changed) {
  bool moved = false;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const int a = in[i];
    int b = a;
    if (a >= 0) {
      b = in[a];
      moved |= b != a;
    }
    out[i] = b;
  }
  if (moved) *changed = 1;
}

// grid.y = field: the owner of an item is the entry its last ancestor, a member, is marked with
__global__ __launch_bounds__(THREADS) void k_field_owner_end(FieldDev F, FieldSets S, const int *__restrict__ anc) {
  const int fbase = blockIdx.y * F.V;
  const int e0 = S.ptr[blockIdx.y];
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < F.V; v += gridDim.x * blockDim.x) {
    const int a = anc[fbase + v];
    int o = -1;
    if (a >= 0) {
      const int mark = F.stamp_near[a];
      if (mark < 0) o = (mark & INT_MAX) - e0;
    }
    S.owner[fbase + v] = o;
  }
}

// grid.y = field: a histogram of the owners, one atomicAdd per wave and distinct owner among its lanes
__global__ __launch_bounds__(THREADS) void k_field_owned(FieldDev F, FieldSets S, int *owned) {
  const int V = F.V;
  const int fbase = blockIdx.y * V;
  int *mine = owned + S.ptr[blockIdx.y];
  const int n_iter = (V + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, v = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, v += gridDim.x * blockDim.x) {
    const int o = v < V ? S.owner[fbase + v] : -1;
    unsigned long long rest = ballot(o >= 0);
    while (rest) {  // (wave-uniform)
      const int leader = __ffsll(rest) - 1;
      const int lo = __shfl(o, leader);
      const unsigned long long same = ballot(o == lo);
      if (lane_id() == leader) atomicAdd(&mine[lo], __popcll(same));
      rest &= ~same;
    }
  }
}

// ---- refresh ("Refresh") --------------------------------------------------------------------

// grid.y = field: the keys of the retained solve (V_old nodes per field) at the nodes of the new graph, none where
// the map names no old node.  `out` is not one of the old solve's arrays: they are regrown only after this ran.
__global__ __launch_bounds__(THREADS) void k_field_carry(const unsigned long long *__restrict__ old_key, int V_old,
                                                         const int *__restrict__ new2old, int V,
                                                         unsigned long long *__restrict__ out) {
  const long long obase = (long long)blockIdx.y * V_old;
  const int fbase = blockIdx.y * V;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
    const int o = new2old[v];
    out[fbase + v] = o >= 0 && o < V_old ? old_key[obase + o] : FIELD_KEY_NONE;
  }
}

// grid.y = field: an item whose last ancestor is no source (-1: only a source points to itself) loses its key.
// key0 / carried (the first anchor): the keys as they are now, and per field the count of items that kept theirs.
__global__ __launch_bounds__(THREADS) void k_field_anchor_end(FieldDev F, const int *__restrict__ anc,
                                                              unsigned long long *__restrict__ key0, int *carried) {
  const int V = F.V;
  const int fbase = blockIdx.y * V;
  const int n_iter = (V + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0, v = blockIdx.x * blockDim.x + threadIdx.x; it < n_iter; ++it, v += gridDim.x * blockDim.x) {
    bool kept = false;
    if (v < V) {
      unsigned long long k = F.key[fbase + v];
      if (anc[fbase + v] < 0 && k != FIELD_KEY_NONE) F.key[fbase + v] = k = FIELD_KEY_NONE;
      if (key0) key0[fbase + v] = k;
      kept = k != FIELD_KEY_NONE;
    }
    const unsigned long long m = ballot(kept);
    if (carried && lane_id() == 0 && m) atomicAdd(&carried[blockIdx.y], __popcll(m));
  }
}

// The control block and the stamps of a warm pass: threshold 0 (every push goes far, every far entry is live), both
// queues and both piles empty, for k_field_warm_seed to fill far pile 0 at phase 1.  A member's mark stays
// (FieldSets).  reset_parents: before the last parent sweep, the forest of the anchors is no longer needed.
__global__ __launch_bounds__(THREADS) void k_field_warm_init(FieldDev F, float delta, bool reset_parents) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < F.N; i += gridDim.x * blockDim.x) {
    if (F.stamp_near[i] > 0) F.stamp_near[i] = 0;
    F.stamp_far[i] = 0u;
    if (reset_parents) F.parent[i] = INT_MAX;
  }
  if (blockIdx.x == 0 && threadIdx.x < F.m) F.ctrl->reached[threadIdx.x] = 0;  // (k_field_output counts into it)
  if (blockIdx.x == 0 && threadIdx.x == 0) field_ctrl_reset(F, 0u, delta, 0);
}

// The seeding sweep of a warm pass: one 16-lane group per item, four per wave, as k_field_relax -- but over every
// item with a key, writing no key: an item one of whose edges would improve its target is pushed, once, to far
// pile 0, stamped with phase 1.  TIGHT: pass 2, tight edges only.  MODELS, RISK: as k_field_relax's.
template <bool MULTI, bool TIGHT, bool MODELS, bool RISK = false>
__global__ __launch_bounds__(THREADS) void k_field_warm_seed(FieldDev F, FieldModelsArg<MODELS> M) {
  static_assert(MULTI || !MODELS, "one field has one model: the host points F.ec at its slot");
  const int N = MULTI ? F.N : F.V;
  const int sub = threadIdx.x & (GROUP - 1);
  const int gw = lane_id() / GROUP;
  const int gshift = lane_id() & ~(GROUP - 1);
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int nwaves = gridDim.x * blockDim.x / WAVE;
  constexpr int PER_WAVE = WAVE / GROUP;
  for (int base = wave * PER_WAVE; base < N; base += nwaves * PER_WAVE) {  // (wave-uniform)
    const int iu = base + gw;
    unsigned long long ku = 0;
    int k = 0, kend = 0;
    int fbase = 0;
    const float *__restrict__ ec = F.ec;
    if (iu < N) {
      ku = F.key[iu];
      int u = iu;
      if constexpr (MULTI) {
        const int f = (int)((unsigned)iu / (unsigned)F.V);
        fbase = f * F.V;
        u = iu - fbase;
        ec = field_costs<MODELS>(F, M, f);
      }
      if (ku != FIELD_KEY_NONE) {
        k = F.rowptr[u] + sub;
        kend = F.rowptr[u + 1];
      }
    }
    bool any = false;
    for (;; k += GROUP) {
      const bool act = k < kend;
      if (ballot(act) == 0) break;  // (wave-uniform: the longest row of the wave's four)
      if (act) {
        const float c = ec[k];
        if (__float_as_uint(c) != FIELD_EDGE_SKIP) {
          int v = F.col[k];
          if constexpr (MULTI) v += fbase;
          const unsigned long long nk = key_extend<RISK>(ku, c);
          const bool tight = !TIGHT || (unsigned)(nk >> 32) == F.tight[v];
          any |= tight && nk < F.key[v];
        }
      }
    }
    const unsigned hits = (unsigned)(ballot(any) >> gshift) & ((1u << GROUP) - 1u);
    const bool push = sub == 0 && hits != 0;
    const int slot = wave_reserve(push, &F.ctrl->c.nfar[0]);
    if (push) {
      F.stamp_far[iu] = 1u;
      if (slot < F.N) F.far[0][slot] = iu;
      else atomicOr(&F.ctrl->c.overflow, 1);
    }
  }
}

int field_blocks(long long items, int per_block) {
  const long long b = (items + per_block - 1) / per_block;
  return (int)std::max(1ll, std::min<long long>(b, MAX_BLOCKS));
}

// one round's launches; the settle step only under bounds with a settle mode
template <bool BOUNDED>
void field_round(const FieldDev &F, int round, const FieldSettle *settle, const FieldModels *models, bool risk,
                 hipStream_t s) {
  const int par = round & 1;
  const dim3 relax_grid(field_blocks((long long)F.N * GROUP, THREADS));
  if (risk && F.m == 1)
    hipLaunchKernelGGL((k_field_relax<false, BOUNDED, false, true>), relax_grid, dim3(THREADS), 0, s, F, par, round + 1,
                       FieldNoModels{});
  else if (risk && models)
    hipLaunchKernelGGL((k_field_relax<true, BOUNDED, true, true>), relax_grid, dim3(THREADS), 0, s, F, par, round + 1,
                       *models);
  else if (risk)
    hipLaunchKernelGGL((k_field_relax<true, BOUNDED, false, true>), relax_grid, dim3(THREADS), 0, s, F, par, round + 1,
                       FieldNoModels{});
  else if (F.m == 1)
    hipLaunchKernelGGL((k_field_relax<false, BOUNDED, false>), relax_grid, dim3(THREADS), 0, s, F, par, round + 1,
                       FieldNoModels{});
  else if (!models)
    hipLaunchKernelGGL((k_field_relax<true, BOUNDED, false>), relax_grid, dim3(THREADS), 0, s, F, par, round + 1,
                       FieldNoModels{});
  else
    hipLaunchKernelGGL((k_field_relax<true, BOUNDED, true>), relax_grid, dim3(THREADS), 0, s, F, par, round + 1,
                       *models);
  hipLaunchKernelGGL(k_field_far_min<BOUNDED>, dim3(field_blocks(F.N, THREADS)), dim3(THREADS), 0, s, F, par);
  if (BOUNDED && settle->mode != FIELD_SETTLE_NONE)
    hipLaunchKernelGGL(k_field_settle, dim3(F.m), dim3(THREADS), 0, s, F, par, settle->targets, settle->n_t,
                       settle->mode);
  hipLaunchKernelGGL(k_field_far_split<BOUNDED>, dim3(field_blocks(F.N, THREADS)), dim3(THREADS), 0, s, F, par);
  hipLaunchKernelGGL(k_field_round_end<BOUNDED>, dim3(1), dim3(64), 0, s, F, par);
}

// ---- keep-out zones ("Keep-out zones") ------------------------------------------------------------
// A zone set closes edges by geometry: k_field_edge_zones fills a slot of the edge-cost array with what
// k_field_edge_cost writes, or the skip marker where the set closes the edge, so every kernel above runs unchanged on
// such a slot.  The verdict needs the positions of BOTH ends, hence the row of an edge: one 16-lane group per row, as the
// relaxation has it (no search in rowptr; the row's position is one load for the group, and consecutive groups read
// consecutive stretches of col / w / dist / ec).  The zone set is staged in LDS once per workgroup as (x, y, r*r).

// The rule, restated line for line from DESIGN.md: does the zone (x, y, r2 = r*r) close the edge between P and Q, P the
// position of the end with the smaller node id.  Every operation is one fp32 operation (-ffp-contract=off); the
// comparisons are taken as written, so a NaN position closes nothing.
__device__ __forceinline__ bool zone_closes(float x, float y, float r2, float Px, float Py, float Qx, float Qy) {
  const float ax = x - Px;
  const float ay = y - Py;
  const float da = ax * ax + ay * ay;
  const float bx = x - Qx;
  const float by = y - Qy;
  const float db = bx * bx + by * by;
  const float dx = Qx - Px;
  const float dy = Qy - Py;
  const float L2 = dx * dx + dy * dy;
  const float t = ax * dx + ay * dy;
  const float cr = ax * dy - ay * dx;
  return da <= r2 || db <= r2 || (t > 0.0f && t < L2 && cr * cr <= r2 * L2);
}

// is the node at P inside the zone: the rule's da <= r2
__device__ __forceinline__ bool zone_holds(float x, float y, float r2, float Px, float Py) {
  const float ax = x - Px;
  const float ay = y - Py;
  const float da = ax * ax + ay * ay;
  return da <= r2;
}

// the zone set into LDS, (x, y, r*r, unused) per zone; every thread of the workgroup calls it -> the zones staged
__device__ __forceinline__ int zones_stage(float4 *zs, const FieldZone *__restrict__ zones, int nz) {
  nz = min(max(nz, 0), FIELD_ZONES_MAX);
  for (int i = threadIdx.x; i < nz; i += blockDim.x) {
    const FieldZone z = zones[i];
    zs[i] = make_float4(z.x, z.y, z.r * z.r, 0.0f);
  }
  __syncthreads();
  return nz;
}

// does some staged zone close the edge between nodes u and v (both in [0, V)); P is the end of the smaller id
__device__ __forceinline__ bool zones_close_edge(const float4 *zs, int nz, const float *__restrict__ xyz, int u, int v) {
  const int a = min(u, v), b = max(u, v);
  const float Px = xyz[3 * (size_t)a], Py = xyz[3 * (size_t)a + 1];
  const float Qx = xyz[3 * (size_t)b], Qy = xyz[3 * (size_t)b + 1];
  bool closed = false;
  for (int i = 0; i < nz && !closed; ++i) {
    const float4 z = zs[i];
    closed = zone_closes(z.x, z.y, z.z, Px, Py, Qx, Qy);
  }
  return closed;
}

// the rows of the 16-lane group this thread belongs to: u = first, first + step, ... below V
__device__ __forceinline__ void zone_group_rows(int &first, int &step, int &lane) {
  first = (blockIdx.x * blockDim.x + threadIdx.x) / GROUP;
  step = gridDim.x * blockDim.x / GROUP;
  lane = threadIdx.x & (GROUP - 1);
}

__global__ __launch_bounds__(THREADS) void k_field_edge_zones(
    const int *__restrict__ rowptr, const int *__restrict__ col, const float *__restrict__ w,
    const float *__restrict__ dist, const int *__restrict__ state, const float *__restrict__ xyz, int V, int E, float sf,
    float tau, const FieldZone *__restrict__ zones, int nz, float *__restrict__ ec, FieldEdgeStats *st) {
  __shared__ float4 zs[FIELD_ZONES_MAX];
  nz = zones_stage(zs, zones, nz);
  double sum = 0.0;
  int cnt = 0, bad = 0;
  int first, step, lane;
  zone_group_rows(first, step, lane);
  for (int u = first; u < V; u += step) {
    const int beg = max(rowptr[u], 0), end = min(rowptr[u + 1], E);
    for (int k = beg + lane; k < end; k += GROUP) {
      const float c = (sf * w[k] + 1.0f) * dist[k];
      if (!(c >= 0.0f) || c == __builtin_huge_valf()) bad = 1;
      const int v = col[k];
      bool skip = v < 0 || v >= V;
      if (!skip) skip = state[v] == FIELD_NODE_INVALID;
      skip = skip || w[k] > tau;  // (the ceiling; +inf: no weight is above it)
      if (!skip) skip = zones_close_edge(zs, nz, xyz, u, v);
      ec[k] = skip ? __uint_as_float(FIELD_EDGE_SKIP) : c;
      if (!skip) {
        sum += (double)c;
        cnt++;
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sum += __shfl_xor(sum, m);
    cnt += __shfl_xor(cnt, m);
    bad |= __shfl_xor(bad, m);
  }
  if (lane_id() == 0) {
    if (cnt) {
      atomicAdd(&st->sum, sum);
      atomicAdd(&st->count, cnt);
    }
    if (bad) atomicOr(&st->bad, 1);
  }
}

// k_field_edge_risk for a slot with a zone set ("Keep-out zones on risk fields"): er[k] is what
// that kernel writes, or the skip marker where the set closes the edge; the sum and count over relaxable, unclosed
// edges, `bad` over ALL edges.  The row walk of k_field_edge_zones.
__global__ __launch_bounds__(THREADS) void k_field_edge_risk_zones(
    const int *__restrict__ rowptr, const int *__restrict__ col, const float *__restrict__ w,
    const int *__restrict__ state, const float *__restrict__ xyz, int V, int E, const FieldZone *__restrict__ zones,
    int nz, float *__restrict__ er, FieldEdgeStats *st) {
  __shared__ float4 zs[FIELD_ZONES_MAX];
  nz = zones_stage(zs, zones, nz);
  double sum = 0.0;
  int cnt = 0, bad = 0;
  int first, step, lane;
  zone_group_rows(first, step, lane);
  for (int u = first; u < V; u += step) {
    const int beg = max(rowptr[u], 0), end = min(rowptr[u + 1], E);
    for (int k = beg + lane; k < end; k += GROUP) {
      const float r = w[k] + 0.0f;
      if (!(r >= 0.0f) || r == __builtin_huge_valf()) bad = 1;
      const int v = col[k];
      bool skip = v < 0 || v >= V;
      if (!skip) skip = state[v] == FIELD_NODE_INVALID;
      if (!skip) skip = zones_close_edge(zs, nz, xyz, u, v);
      er[k] = skip ? __uint_as_float(FIELD_EDGE_SKIP) : r;
      if (!skip) {
        sum += (double)r;
        cnt++;
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sum += __shfl_xor(sum, m);
    cnt += __shfl_xor(cnt, m);
    bad |= __shfl_xor(bad, m);
  }
  if (lane_id() == 0) {
    if (cnt) {
      atomicAdd(&st->sum, sum);
      atomicAdd(&st->count, cnt);
    }
    if (bad) atomicOr(&st->bad, 1);
  }
}

// The verdicts of a zone set by the device function of the solve: closed per CSR edge, inside per node (either may be
// nullptr), and their counts.  An edge whose column is no node is not closed.
__global__ __launch_bounds__(THREADS) void k_field_zone_verdicts(
    const int *__restrict__ rowptr, const int *__restrict__ col, const float *__restrict__ xyz, int V, int E,
    const FieldZone *__restrict__ zones, int nz, unsigned char *__restrict__ closed, unsigned char *__restrict__ inside,
    int *counts) {
  __shared__ float4 zs[FIELD_ZONES_MAX];
  nz = zones_stage(zs, zones, nz);
  int n_closed = 0, n_inside = 0;
  int first, step, lane;
  zone_group_rows(first, step, lane);
  for (int u = first; u < V; u += step) {
    if (lane == 0) {
      const float Px = xyz[3 * (size_t)u], Py = xyz[3 * (size_t)u + 1];
      bool in = false;
      for (int i = 0; i < nz && !in; ++i) in = zone_holds(zs[i].x, zs[i].y, zs[i].z, Px, Py);
      if (inside) inside[u] = in ? 1 : 0;
      n_inside += in ? 1 : 0;
    }
    const int beg = max(rowptr[u], 0), end = min(rowptr[u + 1], E);
    for (int k = beg + lane; k < end; k += GROUP) {
      const int v = col[k];
      const bool shut = v >= 0 && v < V && zones_close_edge(zs, nz, xyz, u, v);
      if (closed) closed[k] = shut ? 1 : 0;
      n_closed += shut ? 1 : 0;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    n_closed += __shfl_xor(n_closed, m);
    n_inside += __shfl_xor(n_inside, m);
  }
  if (lane_id() == 0) {
    if (n_closed) atomicAdd(&counts[0], n_closed);
    if (n_inside) atomicAdd(&counts[1], n_inside);
  }
}

}  // namespace

void launch_field_edge_cost(const int *col, const float *w, const float *dist, const int *state, int V, int E,
                            float safety_factor, float max_weight, float *ec, FieldEdgeStats *st, hipStream_t s) {
  (void)hipMemsetAsync(st, 0, sizeof(FieldEdgeStats), s);
  if (E == 0) return;
  hipLaunchKernelGGL(k_field_edge_cost, dim3(field_blocks(E, THREADS * 8)), dim3(THREADS), 0, s, col, w, dist,
                     state, V, E, safety_factor, max_weight, ec, st);
}

void launch_field_edge_risk(const int *col, const float *w, const int *state, int V, int E, float *er,
                            FieldEdgeStats *st, hipStream_t s) {
  (void)hipMemsetAsync(st, 0, sizeof(FieldEdgeStats), s);
  if (E == 0) return;
  hipLaunchKernelGGL(k_field_edge_risk, dim3(field_blocks(E, THREADS * 8)), dim3(THREADS), 0, s, col, w, state, V, E,
                     er, st);
}

void launch_field_edge_zones(const int *rowptr, const int *col, const float *w, const float *dist, const int *state,
                             const float *xyz, int V, int E, float safety_factor, float max_weight,
                             const FieldZone *zones, int nz, float *ec, FieldEdgeStats *st, hipStream_t s) {
  (void)hipMemsetAsync(st, 0, sizeof(FieldEdgeStats), s);
  if (E == 0) return;
  hipLaunchKernelGGL(k_field_edge_zones, dim3(field_blocks((long long)V * GROUP, THREADS)), dim3(THREADS), 0, s, rowptr,
                     col, w, dist, state, xyz, V, E, safety_factor, max_weight, zones, nz, ec, st);
}

void launch_field_edge_risk_zones(const int *rowptr, const int *col, const float *w, const int *state,
                                  const float *xyz, int V, int E, const FieldZone *zones, int nz, float *er,
                                  FieldEdgeStats *st, hipStream_t s) {
  (void)hipMemsetAsync(st, 0, sizeof(FieldEdgeStats), s);
  if (E == 0) return;
  hipLaunchKernelGGL(k_field_edge_risk_zones, dim3(field_blocks((long long)V * GROUP, THREADS)), dim3(THREADS), 0, s,
                     rowptr, col, w, state, xyz, V, E, zones, nz, er, st);
}

void launch_field_zone_verdicts(const int *rowptr, const int *col, const float *xyz, int V, int E,
                                const FieldZone *zones, int nz, unsigned char *closed, unsigned char *inside,
                                int *counts, hipStream_t s) {
  (void)hipMemsetAsync(counts, 0, 2 * sizeof(int), s);
  if (V == 0) return;
  hipLaunchKernelGGL(k_field_zone_verdicts, dim3(field_blocks((long long)V * GROUP, THREADS)), dim3(THREADS), 0, s,
                     rowptr, col, xyz, V, E, zones, nz, closed, inside, counts);
}

void launch_field_init(const FieldDev &F, const FieldSources &sources, const FieldSets *sets, const unsigned *cost0,
                       const unsigned long long *carried, float delta, hipStream_t s) {
  hipLaunchKernelGGL(k_field_init, dim3(field_blocks(F.V, THREADS), F.m), dim3(THREADS), 0, s, F, sources, delta,
                     sets == nullptr, carried);
  if (!sets) return;
  const dim3 grid(field_blocks(sets->n, THREADS));
  if (cost0) hipLaunchKernelGGL(k_field_seed<true>, grid, dim3(THREADS), 0, s, F, *sets, cost0);
  else hipLaunchKernelGGL(k_field_seed<false>, grid, dim3(THREADS), 0, s, F, *sets, FieldNoCost0{});
}

void launch_field_round(const FieldDev &F, int round, hipStream_t s, const FieldSettle *under_bounds,
                        const FieldModels *models, bool risk) {
  if (under_bounds)
    field_round<true>(F, round, under_bounds, models, risk, s);
  else
    field_round<false>(F, round, nullptr, models, risk, s);
}

void launch_field_bounds(const FieldDev &F, const FieldBounds &budgets, hipStream_t s) {
  hipLaunchKernelGGL(k_field_bounds, dim3(1), dim3(FIELD_MAX_SOURCES), 0, s, F, budgets);
}

void launch_field_trim(const FieldDev &F, hipStream_t s) {
  hipLaunchKernelGGL(k_field_trim, dim3(field_blocks(F.V, THREADS), F.m), dim3(THREADS), 0, s, F);
}

void launch_field_reached_list(const FieldDev &F, int field, int *counts, int *offsets, int *tmp, int cap, int *ids,
                               float *cost, int *hops, hipStream_t s) {
  const int nb = (F.V + THREADS - 1) / THREADS;
  hipLaunchKernelGGL(k_field_list_count, dim3(nb), dim3(THREADS), 0, s, F, field, counts);
  launch_exclusive_scan(counts, offsets, nb, tmp, s);
  if (cap > 0 && (ids || cost || hops))
    hipLaunchKernelGGL(k_field_list_emit, dim3(nb), dim3(THREADS), 0, s, F, field, offsets, cap, ids, cost, hops);
}

void launch_field_cost_bits(const FieldDev &F, unsigned *bits, hipStream_t s) {
  hipLaunchKernelGGL(k_field_cost_bits, dim3(field_blocks(F.N, THREADS)), dim3(THREADS), 0, s, F, bits);
}

void launch_field_finish(const FieldDev &F, float *cost, int *hops, bool parents, hipStream_t s,
                         const FieldModels *models, bool risk) {
  if (parents) launch_field_supporters(F, s, models, risk);
  hipLaunchKernelGGL(k_field_output, dim3(field_blocks(F.V, THREADS), F.m), dim3(THREADS), 0, s, F, cost, hops);
}

void launch_field_gather(const FieldDev &F, const FieldSets *sets, const int *targets, int n_t, float *cost_at,
                         int *hops_at, int *owner_at, hipStream_t s) {
  if (n_t <= 0) return;
  const int *owner = sets ? sets->owner : nullptr;
  hipLaunchKernelGGL(k_field_gather, dim3(field_blocks(n_t, THREADS), F.m), dim3(THREADS), 0, s, F, targets, n_t,
                     cost_at, hops_at, owner, owner ? owner_at : nullptr);
}

void launch_field_parents_late(const FieldDev &F, hipStream_t s, const FieldModels *models, bool risk) {
  const dim3 grid(field_blocks(F.N, THREADS));
  hipLaunchKernelGGL(k_field_parent_mark, grid, dim3(THREADS), 0, s, F, -1, INT_MAX);
  launch_field_supporters(F, s, models, risk);
  hipLaunchKernelGGL(k_field_parent_mark, grid, dim3(THREADS), 0, s, F, INT_MAX, -1);
}

void launch_field_route_len(const FieldDev &F, const int *route_field, const int *route_target, int n_routes,
                            int *len, hipStream_t s) {
  if (n_routes <= 0) return;
  hipLaunchKernelGGL(k_field_route_len, dim3(field_blocks(n_routes, THREADS)), dim3(THREADS), 0, s, F, route_field,
                     route_target, n_routes, len);
}

void launch_field_route_walk(const FieldDev &F, const float *w, const float *dist, const int *route_field,
                             const int *route_target, int n_routes, const int *offsets, int *node_ids,
                             FieldRouteInfo *infos, const FieldSources &sources, const FieldSets *sets,
                             hipStream_t s, const FieldModels *models, bool risk) {
  if (n_routes <= 0) return;
  const dim3 grid(field_blocks((long long)n_routes * GROUP, THREADS));
  if (risk && sets && models)
    hipLaunchKernelGGL((k_field_route_walk<true, true, true>), grid, dim3(THREADS), 0, s, F, w, dist, route_field,
                       route_target, n_routes, offsets, node_ids, infos, *sets, *models);
  else if (risk && models)
    hipLaunchKernelGGL((k_field_route_walk<false, true, true>), grid, dim3(THREADS), 0, s, F, w, dist, route_field,
                       route_target, n_routes, offsets, node_ids, infos, sources, *models);
  else if (risk && sets)
    hipLaunchKernelGGL((k_field_route_walk<true, false, true>), grid, dim3(THREADS), 0, s, F, w, dist, route_field,
                       route_target, n_routes, offsets, node_ids, infos, *sets, FieldNoModels{});
  else if (risk)
    hipLaunchKernelGGL((k_field_route_walk<false, false, true>), grid, dim3(THREADS), 0, s, F, w, dist, route_field,
                       route_target, n_routes, offsets, node_ids, infos, sources, FieldNoModels{});
  else if (sets && models)
    hipLaunchKernelGGL((k_field_route_walk<true, true>), grid, dim3(THREADS), 0, s, F, w, dist, route_field,
                       route_target, n_routes, offsets, node_ids, infos, *sets, *models);
  else if (sets)
    hipLaunchKernelGGL((k_field_route_walk<true, false>), grid, dim3(THREADS), 0, s, F, w, dist, route_field,
                       route_target, n_routes, offsets, node_ids, infos, *sets, FieldNoModels{});
  else if (models)
    hipLaunchKernelGGL((k_field_route_walk<false, true>), grid, dim3(THREADS), 0, s, F, w, dist, route_field,
                       route_target, n_routes, offsets, node_ids, infos, sources, *models);
  else
    hipLaunchKernelGGL((k_field_route_walk<false, false>), grid, dim3(THREADS), 0, s, F, w, dist, route_field,
                       route_target, n_routes, offsets, node_ids, infos, sources, FieldNoModels{});
}

void launch_field_owner_sweep(const FieldDev &F, int sweep, int *changed, hipStream_t s) {
  hipLaunchKernelGGL(k_field_owner_sweep, dim3(field_blocks(F.N, THREADS)), dim3(THREADS), 0, s, F.q[sweep & 1],
                     F.q[~sweep & 1], F.N, changed + sweep);
}

void launch_field_owner_end(const FieldDev &F, const FieldSets &S, int sweeps, hipStream_t s) {
  hipLaunchKernelGGL(k_field_owner_end, dim3(field_blocks(F.V, THREADS), F.m), dim3(THREADS), 0, s, F, S,
                     F.q[sweeps & 1]);
}

void launch_field_carry(const unsigned long long *old_key, int V_old, const int *new2old, int V, int m,
                        unsigned long long *out, hipStream_t s) {
  hipLaunchKernelGGL(k_field_carry, dim3(field_blocks(V, THREADS), m), dim3(THREADS), 0, s, old_key, V_old, new2old, V,
                     out);
}

void launch_field_supporters(const FieldDev &F, hipStream_t s, const FieldModels *models, bool risk) {
  const dim3 grid(field_blocks((long long)F.V * GROUP, THREADS), F.m);
  if (risk && models) hipLaunchKernelGGL((k_field_parent<true, true>), grid, dim3(THREADS), 0, s, F, *models);
  else if (risk) hipLaunchKernelGGL((k_field_parent<false, true>), grid, dim3(THREADS), 0, s, F, FieldNoModels{});
  else if (models) hipLaunchKernelGGL(k_field_parent<true>, grid, dim3(THREADS), 0, s, F, *models);
  else hipLaunchKernelGGL(k_field_parent<false>, grid, dim3(THREADS), 0, s, F, FieldNoModels{});
}

void launch_field_forest_begin(const FieldDev &F, const FieldSources *single, const unsigned long long *key0,
                               int *changed, hipStream_t s) {
  (void)hipMemsetAsync(changed, 0, FIELD_OWNER_SWEEPS_MAX * sizeof(int), s);
  hipLaunchKernelGGL(k_field_forest_begin, dim3(field_blocks(F.V, THREADS), F.m), dim3(THREADS), 0, s, F,
                     single ? *single : FieldSources{}, single != nullptr, key0);
}

void launch_field_anchor_end(const FieldDev &F, int sweeps, unsigned long long *key0, int *carried, hipStream_t s) {
  if (carried) (void)hipMemsetAsync(carried, 0, (size_t)F.m * sizeof(int), s);
  hipLaunchKernelGGL(k_field_anchor_end, dim3(field_blocks(F.V, THREADS), F.m), dim3(THREADS), 0, s, F,
                     F.q[sweeps & 1], key0, carried);
}

void launch_field_warm_start(const FieldDev &F, float delta, bool reset_parents, hipStream_t s,
                             const FieldModels *models, bool risk) {
  hipLaunchKernelGGL(k_field_warm_init, dim3(field_blocks(F.N, THREADS)), dim3(THREADS), 0, s, F, delta,
                     reset_parents);
  const dim3 grid(field_blocks((long long)F.N * GROUP, THREADS));
  const FieldNoModels none{};
  if (risk && F.m == 1) {
    if (F.tight) hipLaunchKernelGGL((k_field_warm_seed<false, true, false, true>), grid, dim3(THREADS), 0, s, F, none);
    else hipLaunchKernelGGL((k_field_warm_seed<false, false, false, true>), grid, dim3(THREADS), 0, s, F, none);
  } else if (risk && models) {
    if (F.tight) hipLaunchKernelGGL((k_field_warm_seed<true, true, true, true>), grid, dim3(THREADS), 0, s, F, *models);
    else hipLaunchKernelGGL((k_field_warm_seed<true, false, true, true>), grid, dim3(THREADS), 0, s, F, *models);
  } else if (risk) {
    if (F.tight) hipLaunchKernelGGL((k_field_warm_seed<true, true, false, true>), grid, dim3(THREADS), 0, s, F, none);
    else hipLaunchKernelGGL((k_field_warm_seed<true, false, false, true>), grid, dim3(THREADS), 0, s, F, none);
  } else if (F.m == 1) {
    if (F.tight) hipLaunchKernelGGL((k_field_warm_seed<false, true, false>), grid, dim3(THREADS), 0, s, F, none);
    else hipLaunchKernelGGL((k_field_warm_seed<false, false, false>), grid, dim3(THREADS), 0, s, F, none);
  } else if (!models) {
    if (F.tight) hipLaunchKernelGGL((k_field_warm_seed<true, true, false>), grid, dim3(THREADS), 0, s, F, none);
    else hipLaunchKernelGGL((k_field_warm_seed<true, false, false>), grid, dim3(THREADS), 0, s, F, none);
  } else {
    if (F.tight) hipLaunchKernelGGL((k_field_warm_seed<true, true, true>), grid, dim3(THREADS), 0, s, F, *models);
    else hipLaunchKernelGGL((k_field_warm_seed<true, false, true>), grid, dim3(THREADS), 0, s, F, *models);
  }
}

void launch_field_owned(const FieldDev &F, const FieldSets &S, int *owned, hipStream_t s) {
  (void)hipMemsetAsync(owned, 0, (size_t)S.n * sizeof(int), s);
  hipLaunchKernelGGL(k_field_owned, dim3(field_blocks(F.V, THREADS), F.m), dim3(THREADS), 0, s, F, S, owned);
}

#include "trg_field_tiled.inc"

}  // namespace trg
