// trg_level.inc -- the three kernels of one BFS level of the device-resident TRG build
// (TRG::expandGraph, trg.cpp:372-454, for configurations whose step 3 is off), included into
// trg_kernels.hip's anonymous namespace after trg_bfs.inc.
//
//   k_level_sample   one workgroup per queued node: stages the map points its trial discs can reach
//                    in LDS once and uses that tile for the rejection sampling (trg.cpp:384-403) and
//                    the elevation lookup of addNode (:244-247); then the nearest pre-level node of
//                    every accepted sample (:408-413, from an LDS copy of the node grid around the
//                    parent).  Samples with no pre-level node within robot_size may create a node
//                    ("candidates"); they are entered into the level's hash (cell -> sample slot).
//   k_level_spec     one wave per candidate: whether its speculative parent edge holds (wireEdge :269-338 up to
//                    the decision; the covariance of the gather is left to k_node_cov).
//   k_level_resolve  one wave per sample slot: what the sequential loop would have done with this
//                    sample given everything EARLIER in the level (trg.cpp:406-452) -- skip, merge with
//                    an existing or a newly created node, or create a node -- by waiting only for the
//                    earlier candidates that can matter; writes the wireEdge call record of the slot.
//                    Then the commit: the new nodes are numbered in sequence order (= creation order;
//                    a single-pass scan with look-back over the workgroups' totals), appended to the
//                    node store and the node grid, and the next frontier and the level totals go out.
//
// A call record that points at a node created in the same level cannot know its id yet (ids follow
// from a prefix over the whole level): it stores a reference to the creating call instead
// (call_ref), the commit leaves the id in newid_of_call[], and the first pass over the call log
// (k_first_insert) replaces references by ids.  The weight of the edge to a created node is not
// needed inside the loop either (only whether the edge exists): three candidates out of four never create
// a node, so the covariance of the gather is computed for the created nodes alone (k_node_cov) and
// k_node_weights runs the SVDs (trg.cpp:339-363), both for all nodes after the loop.

__device__ __forceinline__ int call_ref(long long at) { return -(int)(at + 2); }       // <= -2
// The call log holds B.cstride entries per sample slot: entry 0 is the slot's own wireEdge call (trg.cpp:416,
// 425), entries 1.. are the calls of expandGraph's step 3 for the node the slot created (trg.cpp:429-444;
// cstride = 1 when that step is compiled out by the parameters), so that log order = program order.
__device__ __forceinline__ long long call_at(const BfsDev &B, long long call_base, int slot) {
  return call_base + (long long)slot * B.cstride;
}
__device__ __forceinline__ long long ref_call(int n2) { return -(long long)n2 - 2; }

// entry e (xx xy xz yy yz zz) of covariance = centred^T * centred / (n - 1) from the fp64 moments,
// rounded once -- the same expressions as mid_covariance
__device__ __forceinline__ float cov_entry(const double (&sm)[9], int kept, int e) {
  const double n = (double)kept;
  const double inv = 1.0 / (double)(kept - 1);
  // (a, b) = (0,0) (0,1) (0,2) (1,1) (1,2) (2,2); explicit selects keep the totals in registers
  const double sa = e < 3 ? sm[0] : (e < 5 ? sm[1] : sm[2]);
  const double sb = e == 0 ? sm[0] : ((e == 1 || e == 3) ? sm[1] : sm[2]);
  const double sab = e == 0 ? sm[3] : e == 1 ? sm[4] : e == 2 ? sm[5] : e == 3 ? sm[6] : e == 4 ? sm[7] : sm[8];
  const double ma = sa / n, mb = sb / n;
  return (float)((sab - n * ma * mb) * inv);
}

// waves per SIMD k_level_sample is compiled for: 5 (86 registers; five workgroups per CU) measured 0.2 ms
// faster than 6 (80 registers, six per CU -- which is also all the LDS allows): the kernel does not live on
// occupancy, and the tighter register budget costs more than the sixth workgroup brings
#ifndef LV_WAVES_PER_SIMD
#define LV_WAVES_PER_SIMD 5
#endif
constexpr int LV_SMAX = 64;       // sample_num the level kernels support (larger: host replay)
constexpr int LV_NODE_CAP = 256;  // pre-level nodes within reach of one node's samples (packing bound ~170)
#ifndef TRG_LSW
#define TRG_LSW 4
#endif
constexpr int LSW = TRG_LSW;       // waves of a k_level_sample workgroup (2 draws per wave and round): 4 measured best --
                                  // 8 finish a node in fewer rounds but only half as many nodes are resident
static_assert(LSW <= SW, "the sampling LDS (SampleLds) is sized for SW waves");
constexpr int LV_WIN_MAX = LSW >= 8 ? 22 : (LSW >= 4 ? 16 : 11);  // side of the node-grid window a workgroup can stage (side^2 <= LSW*64)

// -DLV_PHASE_TIMING: thread 0 of every expand workgroup adds the cycles each phase took into
// stats64[16 + shard * 8 + phase] (1024 shards; profiling builds only; scripts/phase_timing.sh)
#ifdef LV_PHASE_TIMING_RESOLVE  // the same slots, filled by k_level_resolve instead (phases: see the kernel)
#define RV_PHASE(n)                                                                               \
  if (threadIdx.x == 0) {                                                                         \
    const long long now_ = clock64();                                                             \
    atomicAdd(&B.stats64[16 + (blockIdx.x & 1023) * 8 + (n)], (unsigned long long)(now_ - phase_t_)); \
    phase_t_ = clock64();                                                                         \
  }
#define RV_PHASE_BEGIN long long phase_t_ = clock64();
#else
#define RV_PHASE(n)
#define RV_PHASE_BEGIN
#endif
#if defined(LV_PHASE_TIMING) && !defined(LV_PHASE_TIMING_RESOLVE)
#define LV_PHASE(n)                                                                               \
  if (threadIdx.x == 0) {                                                                         \
    const long long now_ = clock64();                                                             \
    atomicAdd(&B.stats64[16 + (blockIdx.x & 1023) * 8 + (n)], (unsigned long long)(now_ - phase_t_)); \
    phase_t_ = clock64();                                                                         \
  }
#define LV_PHASE_BEGIN long long phase_t_ = clock64();
#else
#define LV_PHASE(n)
#define LV_PHASE_BEGIN
#endif

// -DLV_TIMELINE=<tag>: wall-clock marks (100 MHz) of the level attempts tag .. tag + 5, one plain store per
// workgroup / slot and mark into B.tl (no atomics: a shared mark would serialise the level); the host
// prints minima / maxima / medians when TRG_TIMELINE is set (scripts/level_marks.sh).
// Layout per tag: TL_STRIDE words; kind k of unit i at [k * TL_UNITS + i].
constexpr int TL_UNITS = 1 << 16, TL_KINDS = 12, TL_TAGS = 6;
constexpr size_t TL_STRIDE = (size_t)TL_UNITS * TL_KINDS;
#ifdef LV_TIMELINE
#define TL_MARK(tag, kind, unit)                                                                      \
  do {                                                                                                \
    const unsigned tlt_ = (unsigned)((tag) - (LV_TIMELINE));                                          \
    if (B.tl && tlt_ < (unsigned)TL_TAGS && (unsigned)(unit) < (unsigned)TL_UNITS)                    \
      B.tl[(size_t)tlt_ * TL_STRIDE + (size_t)(kind) * TL_UNITS + (unit)] = (unsigned long long)wall_clock64(); \
  } while (0)
#else
#define TL_MARK(tag, kind, unit)
#endif
// kinds: 0 sample start, 1 sample end (per node); 2 spec start, 3 spec end (per slot); 4 resolve start,
// 5 blockers collected, 6 first wave decided, 7 counts published (per resolve workgroup, filed under the NEXT
// level's tag); 8, 9 unused; 10 commit start, 11 commit sums known (per commit workgroup, next level's tag)
struct LevelLds {
  float nd_x[LV_NODE_CAP], nd_y[LV_NODE_CAP];
  int nd_id[LV_NODE_CAP];
  int nd_n;
  int pdisc;          // BfsDev::ndisc of the node being expanded
  int cand[LV_SMAX];  // class of every sample
};

// level tag of a hash entry: entries of other levels (or builds: the table is cleared per build)
// count as empty, so the table is never cleared inside the level loop
__device__ __forceinline__ unsigned long long lv_entry(int tag, int cell) {
  return ((unsigned long long)(unsigned)tag << 32) | (unsigned)cell;
}

// ---- two trial discs per wave (32 lanes each) ----------------------------------------------------------
// A robot_size disc holds ~28 of the ~60 points of the three or four cell-row segments it touches:
// one 64-lane wave per disc leaves more than half of the lanes idle in every row sweep and pays the
// wave-wide reductions once per disc.  Here each HALF of a wave evaluates its own draw; the
// reductions are DPP row operations whose last step joins rows 0-1 and rows 2-3 separately, and the
// median bookkeeping runs on the scalar unit for both halves at once.

// minimum / maximum of an order-preserving key over the 32 lanes of each half; every lane gets the
// result of its own half
template <bool IS_MIN>
__device__ __forceinline__ unsigned half_reduce_key(unsigned v) {
  const unsigned ident = IS_MIN ? 0xFFFFFFFFu : 0u;
#define HKEY_STEP(ctrl, rowmask)                                                                 \
  {                                                                                              \
    const unsigned o = (unsigned)__builtin_amdgcn_update_dpp((int)ident, (int)v, ctrl, rowmask,  \
                                                             0xf, false);                        \
    v = IS_MIN ? (o < v ? o : v) : (o > v ? o : v);                                              \
  }
  HKEY_STEP(0x111, 0xf)  // row_shr:1
  HKEY_STEP(0x112, 0xf)  // row_shr:2
  HKEY_STEP(0x114, 0xf)  // row_shr:4
  HKEY_STEP(0x118, 0xf)  // row_shr:8  -> lane 15 of every row holds the row's result
  HKEY_STEP(0x142, 0xa)  // row_bcast:15 into rows 1 and 3 -> lanes 31 and 63 hold the halves' results
#undef HKEY_STEP
  const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)v, 31);
  const unsigned r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 63);
  return (lane_id() & 32) ? r1 : r0;
}

// this half's 32 bits of a wave ballot
__device__ __forceinline__ unsigned half_bits(unsigned long long mask) {
  return (lane_id() & 32) ? (unsigned)(mask >> 32) : (unsigned)mask;
}

struct Disc2 {  // per lane: the values of the lane's half
  int n, cnt;
  float nn_z, nn_d2;
  int nn_tie;
};

// lanes that keep the smaller value in step (K, J) of the ascending bitonic network over each 32-lane half
constexpr unsigned long long hsort_keep_min_mask(int K, int J) {
  unsigned long long m = 0;
  for (int l = 0; l < 64; ++l) {
    const int l32 = l & 31;
    if (((l32 & K) == 0) == ((l32 & J) == 0)) m |= 1ull << l;
  }
  return m;
}

// isCollision + nearest map point of TWO discs (one per half wave), candidates read from the block
// tile; zb: this wave's hit buffer, SHCAP / 2 floats per half.  cnt = -1: this half's disc does not
// fit the fast path (more than SHCAP / 2 hits), the caller evaluates it with the whole wave.
// (The nearest-point tracking stays fused into every trial disc although only one draw in five -- a candidate --
// needs it.  Taking it out and looking candidates up in a second pass after the classification was measured:
// k_level_sample<4> 29.6 -> 32.9 us per launch, the build 0.33 ms slower; profiles/r20_known_queries_ab.txt.)
__device__ Disc2 sample_tile_disc2(const MapView &m, const SampleLds &L, float *zb, float qx, float qy,
                                   float r, float h) {
  const int lane = lane_id();
  const int hh = lane >> 5, l32 = lane & 31;
  float *zbh = zb + hh * (SHCAP / 2);
  const float r2 = r * r;
  const CellRange c = cells_for(m, qx, qy, r);
  // the disc's cells in box coordinates (the box covers them by construction; clamp for safety)
  const int cx0 = max(c.cx0 - L.bx0, 0), cx1 = min(c.cx1 - L.bx0, L.ncols - 1);
  const int cy0 = max(c.cy0 - L.by0, 0), cy1 = min(c.cy1 - L.by0, L.nrows - 1);
  const int nrows = cy1 - cy0 + 1;
  const int nrows_max = max(__builtin_amdgcn_readlane(nrows, 0), __builtin_amdgcn_readlane(nrows, 32));
  int n = 0;
  float best_d2 = FLT_MAX, best_z = 0.0f;
  int best_perm = INT_MAX;
  bool lane_tie = false;
  for (int ri = 0; ri < nrows_max; ++ri) {
    const bool rvalid = ri < nrows && cx1 >= cx0;
    const int row = rvalid ? cy0 + ri : 0;
    const int s = rvalid ? L.cs[row][cx0] : 0, e = rvalid ? L.cs[row][cx1 + 1] : 0;
    const int len = e - s;
    const int len_max = max(__builtin_amdgcn_readlane(len, 0), __builtin_amdgcn_readlane(len, 32));
    for (int base = 0; base < len_max; base += 32) {
      const int i = s + base + l32;
      const bool act = base + l32 < len;
      bool hit = false;
      float z = 0.0f, d2 = 0.0f;
      if (act) {
        const f2 pt = L.xy[i];
        const float dx = pt.x - qx;
        const float dy = pt.y - qy;
        z = L.z[i];
        d2 = dx * dx + dy * dy;
        hit = d2 <= r2;
      }
      const unsigned hm = half_bits(ballot(hit));
      if (hit) {
        const int pos = n + __popc(hm & ((1u << l32) - 1u));
        if (pos < SHCAP / 2) zbh[pos] = z;
        const int pm = L.perm[i];
        if (d2 == best_d2) lane_tie = true;
        if (d2 < best_d2) lane_tie = false;
        if (d2 < best_d2 || (d2 == best_d2 && pm < best_perm)) {
          best_d2 = d2;
          best_z = z;
          best_perm = pm;
        }
      }
      n += __popc(hm);
    }
  }
  Disc2 out;
  out.n = n;
  out.cnt = 0;
  out.nn_z = 0.0f;
  out.nn_d2 = 0.0f;
  out.nn_tie = 0;
  // nearest point: smallest distance (d2 >= 0, so its bit pattern orders like the value), then the
  // smallest original index among the lanes that hold it
  const unsigned dkey = __float_as_uint(best_d2);
  const unsigned wdk = half_reduce_key<true>(dkey);
  const bool holds = best_perm != INT_MAX && dkey == wdk;
  const unsigned wp = half_reduce_key<true>(holds ? (unsigned)best_perm : 0xFFFFFFFFu);
  const unsigned who = half_bits(ballot(holds && (unsigned)best_perm == wp));
  const int src = (lane & 32) + (who ? __ffs((int)who) - 1 : 0);
  out.nn_z = __shfl(best_z, src);
  out.nn_d2 = __uint_as_float(wdk);
  out.nn_tie = half_bits(ballot(holds && ((unsigned)best_perm != wp || lane_tie))) != 0u;
  if (n > SHCAP / 2) out.cnt = -1;
  // z range of the hits, from the compacted hit buffer
  wave_lds_sync();
  const int nq = min(n, SHCAP / 2);
  const float zl = zbh[l32 < nq ? l32 : 0];
  unsigned kmn = 0xFFFFFFFFu, kmx = 0u;
  for (int i = l32; i < nq; i += 32) {
    const unsigned zk = float_key(i == l32 ? zl : zbh[i]);
    kmn = zk < kmn ? zk : kmn;
    kmx = zk > kmx ? zk : kmx;
  }
  const unsigned klo = half_reduce_key<true>(kmn), khi = half_reduce_key<false>(kmx);
  // every |z - z_med| <= zmax - zmin (rounding is monotone), so a flat disc needs no median
  const bool need = n > 0 && out.cnt == 0 && !(key_float(khi) - key_float(klo) <= h);
  const unsigned long long need_m = ballot(need);
  if (need_m) {
    const bool need0 = (need_m & 1ull) != 0ull, need1 = (need_m >> 32) != 0ull;
    const int n0 = __builtin_amdgcn_readlane(n, 0), n1 = __builtin_amdgcn_readlane(n, 32);
    if ((need0 && n0 > 32) || (need1 && n1 > 32)) {
      // more hits than lanes in a half: rank selection over the hit buffer, the whole wave per half
      int c0 = 0, c1 = 0;
      if (need0) c0 = median_count(zb, n0, h);
      if (need1) c1 = median_count(zb + SHCAP / 2, n1, h);
      out.cnt = need ? ((lane & 32) ? c1 : c0) : out.cnt;
    } else {
      // Both medians at once: lane i of a half holds hit i (+inf past the half's count); a bitonic network
      // over the 32 lanes of each half sorts them ascending -- 15 compare-exchange steps, the partner lane
      // (lane ^ j) read through the LDS crossbar without touching memory (ds_swizzle, bit mode) -- and the
      // upper median (trg.cpp:763-764, pts[pts.size() / 2]) sits in lane n / 2.  (Counting every hit's
      // rank against all others, one LDS broadcast and five vector instructions per hit, was twice the
      // vector instructions; a radix selection over the key bits three times that.)
      float v = (l32 < n) ? zl : FLT_MAX;
#define HSORT_STEP(K, J)                                                                               \
  {                                                                                                    \
    const float o = __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1F | ((J) << 10))); \
    float mn, mx;                                                                                      \
    asm("v_min_f32 %0, %1, %2" : "=v"(mn) : "v"(v), "v"(o));                                           \
    asm("v_max_f32 %0, %1, %2" : "=v"(mx) : "v"(v), "v"(o));                                           \
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(v) : "v"(mx), "v"(mn), "s"(hsort_keep_min_mask(K, J)));  \
  }
      HSORT_STEP(2, 1)
      HSORT_STEP(4, 2) HSORT_STEP(4, 1)
      HSORT_STEP(8, 4) HSORT_STEP(8, 2) HSORT_STEP(8, 1)
      HSORT_STEP(16, 8) HSORT_STEP(16, 4) HSORT_STEP(16, 2) HSORT_STEP(16, 1)
      HSORT_STEP(32, 16) HSORT_STEP(32, 8) HSORT_STEP(32, 4) HSORT_STEP(32, 2) HSORT_STEP(32, 1)
#undef HSORT_STEP
      const float zmed = __shfl(v, (lane & 32) + (n >> 1));
      const unsigned bad = half_bits(ballot(need && l32 < n && fabsf(zl - zmed) > h));
      out.cnt = need ? __popc(bad) : out.cnt;
    }
  }
  wave_lds_sync();  // the hit buffer is reused by the next round
  return out;
}

// ---- the PURE part of a node's expansion -----------------------------------------------------------------
// Rejection sampling (trg.cpp:384-403) and the elevation of every accepted sample (addNode, :244-247) are
// a function of (node position, node id, map) alone: nothing another node of the level does can change
// them.  sample_pure runs them with a workgroup of NW waves; k_level_sample calls it inline.
template <int NW>
struct PureLds {
  float sx[LV_SMAX], sy[LV_SMAX], sz[LV_SMAX];
  int sn[LV_SMAX];  // map points inside the accepted sample's disc (Disc2::n)
  int r_col[2][2 * NW];
  unsigned long long r_hits[NW];
  int r_ties[NW];
};

// all threads of the workgroup: the tile of map points every draw of the node can reach (barriers inside)
template <int NW>
__device__ __forceinline__ bool sample_pure_stage(const MapView &m, const QueryParams &p, float px, float py,
                                                  SampleLds &L, PureLds<NW> &P) {
  static_assert(NW <= SW, "the sampling LDS (SampleLds) is sized for SW waves");
  if (threadIdx.x < NW) P.r_ties[threadIdx.x] = 0;
  return stage_sample_tile(m, p, px, py, L);
}

// all threads of the workgroup, after sample_pure_stage; on return (after a barrier) P.sx/sy/sz[0..n_acc)
// hold the accepted samples in draw order, P.r_hits / P.r_ties the per-wave counters; mt_slot_base: slot
// number of the node's first sample in the level the samples belong to (map-tie records)
template <int NW>
__device__ __forceinline__ void sample_pure_draws(const MapView &m, const QueryParams &p, const float *cos_t,
                                                  const float *sin_t, int table_bits, uint32_t seed, uint32_t epoch,
                                                  const BfsDev &B, int mt_parity, int mt_slot_base,
                                                  DeviceCounters *ctr, uint32_t id, float px, float py, bool use_tile,
                                                  SampleLds &L, PureLds<NW> &P, int &n_acc_out, int &draws_out) {
  const int tid = threadIdx.x;
  const int w = tid >> 6;
  const int lane = lane_id();
  const int S = p.sample_num;
  // 2 * NW draws per round (one per HALF wave), acceptance in draw order on the scalar unit, so the
  // result equals the sequential loop's.  (Evaluating only ~1.5 x the missing samples in later rounds
  // was measured: 4 % fewer vector instructions, but the extra rounds cost more than they save.)
  constexpr int drr = 2 * NW;  // draws per round
  const int max_trial_sample = 1000;
  int n_acc = 0, rejects = 0, draws = 0, round = 0;
  unsigned long long hits = 0;
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const int hh = lane >> 5;
  float c_next, s_next;
  {
    const uint32_t k = sample_hash(seed, epoch, id, (uint32_t)(2 * w + hh)) >> (32 - table_bits);
    c_next = cos_t[k];
    s_next = sin_t[k];
  }
  while (n_acc < S && rejects <= max_trial_sample) {
    const float qx = px + p.expand_dist * c_next;
    const float qy = py + p.expand_dist * s_next;
    {  // the table entries of the next round (a round that is not the last consumes all its draws)
      const uint32_t k = sample_hash(seed, epoch, id, (uint32_t)(draws + drr + 2 * w + hh)) >> (32 - table_bits);
      c_next = cos_t[k];
      s_next = sin_t[k];
    }
    Disc2 d;
    d.n = 0;
    d.cnt = -1;
    d.nn_z = d.nn_d2 = 0.0f;
    d.nn_tie = 0;
    const bool wave_active = 2 * wu < drr;
    if (wave_active && use_tile) d = sample_tile_disc2(m, L, L.zb[w], qx, qy, p.robot_size, p.height_threshold);
    // dense disc or oversized box: the general query with the whole wave, one half after the other
    // (its hit buffer is this wave's LDS slice; a disc with more hits selects the median by
    // re-reading the map)
    const unsigned long long slow = wave_active ? ballot(d.cnt < 0) : 0ull;
    if (slow) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        if (!((slow >> (32 * g)) & 1ull)) continue;
        const float gx = __shfl(qx, 32 * g), gy = __shfl(qy, 32 * g);
        const Disc dg = disc_query<true>(m, gx, gy, p.robot_size, p.height_threshold, L.zb[w], ctr, SHCAP);
        if (hh == g) {
          d.n = dg.n;
          d.cnt = dg.cnt;
          d.nn_z = dg.nn_z;
          d.nn_d2 = dg.nn_d2;
          d.nn_tie = dg.nn_tie;
        }
      }
    }
    const bool in_core = qx >= p.core_x0 && qx < p.core_x1 && qy >= p.core_y0 && qy < p.core_y1;
    bool collides = true;                        // empty disc: trg.cpp:749-752
    if (ballot(d.n > 0 && d.cnt != 0) != 0ull) {  // (wave-uniform: two flat discs need no division, 0 / n = +0 exactly)
      if (d.n > 0) collides = (float)d.cnt / (float)d.n > p.collision_threshold;  // trg.cpp:773
    } else if (d.n > 0) {
      collides = 0.0f > p.collision_threshold;
    }
    collides = collides || !in_core;
    int *colbuf = P.r_col[round & 1];  // double-buffered: one barrier per round
    if ((lane & 31) == 0 && 2 * w + hh < drr) colbuf[2 * w + hh] = collides ? 1 : 0;
    __syncthreads();
    const unsigned long long colmask = ballot(lane < drr && colbuf[lane < drr ? lane : 0] != 0);
    int my_slot0 = -1, my_slot1 = -1;
    int consumed = 0;
    for (int i = 0; i < drr; ++i) {
      if (n_acc >= S || rejects > max_trial_sample) break;
      draws++;
      consumed++;
      if ((colmask >> i) & 1ull) {
        rejects++;
      } else {
        if (i == 2 * wu) my_slot0 = n_acc;
        if (i == 2 * wu + 1) my_slot1 = n_acc;
        n_acc++;
      }
    }
    // instrumentation counts the reference's queries only (draws past the stopping point are not its)
    {
      const int n0 = __builtin_amdgcn_readlane(d.n, 0), n1 = __builtin_amdgcn_readlane(d.n, 32);
      if (2 * wu < consumed) hits += (unsigned long long)n0;
      if (2 * wu + 1 < consumed) hits += (unsigned long long)n1;
    }
    const int my_slot = hh ? my_slot1 : my_slot0;
    if (my_slot >= 0 && (lane & 31) == 0) {
      P.sx[my_slot] = qx;
      P.sy[my_slot] = qy;
      P.sz[my_slot] = d.nn_z;
      P.sn[my_slot] = d.n;
      if (d.nn_tie) {
        atomicAdd(&P.r_ties[w], 1);
        const int k = atomicAdd(&B.ctrs[BFS_CTR_NMAPTIE + mt_parity], 1);
        if (k < B.mt_cap) {  // (a slot ties at most once, and the list holds a record per slot: always)
          MapTieRec rec;
          rec.slot = mt_slot_base + my_slot;
          rec.qx = qx;
          rec.qy = qy;
          rec.d2 = d.nn_d2;
          B.mt_rec[(size_t)mt_parity * B.mt_cap + k] = rec;
        }
      }
    }
    round++;
  }
  if (lane == 0) P.r_hits[w] = hits;
  __syncthreads();  // samples and the per-wave counters are complete
  n_acc_out = n_acc;
  draws_out = draws;
}

// What the sampling workgroup's lanes share (one node per workgroup)
template <int NW>
struct SampleSide {
  SampleLds L;
  LevelLds V;
  PureLds<NW> P;
};

// wg: index of the workgroup among the sampling workgroups of the launch; NW: its waves (2 draws per wave and round)
template <int NW>
__device__ __forceinline__ void sample_body(SampleSide<NW> &SS, const MapView &m, const QueryParams &p, const float *cos_t,
                                            const float *sin_t, int table_bits, uint32_t seed, uint32_t epoch,
                                            const BfsDev &B, int count, const int *count_dev, int node_base,
                                            int parity, int tag, int pub_stamp, DeviceCounters *ctr, int wg) {
  SampleLds &L = SS.L;
  LevelLds &V = SS.V;
  PureLds<NW> &P = SS.P;
  const int node = wg + node_base;
  // The counters of the level that has just been committed reach the host without a copy in the
  // stream: this kernel runs right behind that level's k_level_resolve, and its first workgroup
  // hands them over in ONE 64-byte store instruction of 16 lanes that carries the level's stamp at
  // both ends (words 5 and 15 are spare), so the host never takes a torn block for a valid one.
  if (pub_stamp && wg == 0 && threadIdx.x < BFS_CTR_COUNT && B.host_ctrs) {
    int v = __hip_atomic_load(&B.ctrs[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == BFS_CTR_DONE || threadIdx.x == BFS_CTR_COUNT - 1) v = pub_stamp;
    __hip_atomic_store(&B.host_ctrs[threadIdx.x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // the expansion's start, for the k_level_resolve behind it (a top-up launch, node_base > 0, is inside the bracket)
  if (node == 0 && threadIdx.x == 0) B.stats64[STATS64_EXPAND_START] = (unsigned long long)wall_clock64();
  if (count_dev) count = min(count, *count_dev);
  if (node >= count) return;
  const int tid = threadIdx.x;
  const int w = tid >> 6;
  const int lane = lane_id();
  const int S = p.sample_num;
  if (tid == 0) TL_MARK(tag, 0, node);
  const int gid = B.front_cur[node];
  const float2 pxy = B.fxy_cur[node];  // (= nx[gid], ny[gid]: no second round trip before the tile)
  const float px = pxy.x, py = pxy.y, pz = B.nz[gid];
  // the node's own acceptance disc, the first disc of its edges' walks: loaded beside nz, parked in LDS for the
  // node record at the end (no register through the sampling)
  if (tid == 0) V.pdisc = B.ndisc ? B.ndisc[gid] : -1;
  const uint32_t id = (uint32_t)gid;
  if (tid == 0) {
    V.nd_n = 0;
  }
  LV_PHASE_BEGIN
  // ---- the node grid around the parent: every node that can be the nearest of one of its samples --
  // (a sample is expand_dist from the parent and its nearest node at most 1.01 expand_dist from it).
  // One thread per cell, the cell's whole 64-byte record in one go; the loads are in flight while
  // the map tile is staged.
  int4 gc0 = {0, 0, 0, 0}, gc1 = gc0, gc2 = gc0;
  int gc_y0 = 0;
  {
    const int K = (int)ceilf(p.expand_dist * 2.01f * B.ginv) + 1;
    const int side = 2 * K + 1;
    const int cx = bfs_cell_x(B, px), cy = bfs_cell_y(B, py);
    if (tid < side * side) {
      const int yy = cy - K + tid / side, xx = cx - K + tid % side;
      // only the cells the disc of radius 2.01 expand_dist around the parent reaches (the corners of the
      // window are a third of its 64-byte records)
      const float bx = B.gx0 + (float)xx * B.gcell_size, by = B.gy0 + (float)yy * B.gcell_size;
      const float ddx = fmaxf(fmaxf(bx - px, px - (bx + B.gcell_size)), 0.0f);
      const float ddy = fmaxf(fmaxf(by - py, py - (by + B.gcell_size)), 0.0f);
      const float reach = p.expand_dist * 2.02f + 1e-3f;
      if (yy >= 0 && yy < B.GH && xx >= 0 && xx < B.GW && ddx * ddx + ddy * ddy <= reach * reach) {
        const int4 *c = (const int4 *)&B.gcell[yy * B.GW + xx];
        gc0 = c[0];  // cnt, id0..2
        gc1 = c[1];  // id3, x0..2
        gc2 = c[2];  // x3, y0..2
        gc_y0 = ((const int *)c)[12];  // y3
      }
    }
  }
  int n_acc = 0, draws = 0;
  unsigned long long hits_node = 0;
  int ties_node = 0;
  const bool use_tile = sample_pure_stage<NW>(m, p, px, py, L, P);
  if (!use_tile) __syncthreads();  // (a box that does not fit the tile is staged without barriers)
  LV_PHASE(0)
  {
    const int cnt = min(gc0.x, GRID_SLOTS);
    if (cnt > 0) {
      const int base = atomicAdd(&V.nd_n, cnt);
      const int ids[4] = {gc0.y, gc0.z, gc0.w, gc1.x};
      const int xs[4] = {gc1.y, gc1.z, gc1.w, gc2.x};
      const int ys[4] = {gc2.y, gc2.z, gc2.w, gc_y0};
#pragma unroll
      for (int qi = 0; qi < GRID_SLOTS; ++qi)
        if (qi < cnt && base + qi < LV_NODE_CAP) {
          V.nd_id[base + qi] = ids[qi];
          V.nd_x[base + qi] = __int_as_float(xs[qi]);
          V.nd_y[base + qi] = __int_as_float(ys[qi]);
        }
    }
  }
  LV_PHASE(1)
  sample_pure_draws<NW>(m, p, cos_t, sin_t, table_bits, seed, epoch, B, parity, node * S, ctr, id, px, py, use_tile,
                         L, P, n_acc, draws);
  if (tid == 0)
    for (int i = 0; i < NW; ++i) {
      hits_node += P.r_hits[i];
      ties_node += P.r_ties[i];
    }
  if (tid == 0 && V.nd_n > LV_NODE_CAP) atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_GRID_OVERFLOW);
  const int hh = lane >> 5;
  LV_PHASE(2)
  // ---- nearest pre-level node and class of every accepted sample (trg.cpp:408-417) ---------------
  // (two samples per wave at a time, one per half: the node list is ~100 entries, a whole wave per
  // sample left most lanes idle through the reductions)
  const int nd_n = min(V.nd_n, LV_NODE_CAP);
  {
    const int l32 = lane & 31;
    for (int j0 = w; j0 < S; j0 += 2 * NW) {
      const int j = j0 + hh * NW;  // this half's sample
      const bool have_slot = j < S;
      const bool acc = have_slot && j < n_acc;
      const int slot = node * S + j;
      float qx = 0.0f, qy = 0.0f;
      unsigned bkey = 0xFFFFFFFFu;
      int bid = -1;
      bool lane_tie = false;
      if (acc) {
        qx = P.sx[j];
        qy = P.sy[j];
        for (int i = l32; i < nd_n; i += 32) {
          const unsigned k = __float_as_uint(bfs_d2(V.nd_x[i], V.nd_y[i], qx, qy));
          const int nid = V.nd_id[i];
          if (k < bkey) {
            bkey = k;
            bid = nid;
            lane_tie = false;
          } else if (k == bkey && nid != bid) {
            lane_tie = true;
          }
        }
      }
      const unsigned mk = half_reduce_key<true>(bkey);
      const unsigned who = half_bits(ballot(bkey == mk));
      const unsigned tl = half_bits(ballot(bkey == mk && lane_tie));
      int cls = 0, nn = -1;
      float d2 = FLT_MAX;
      const int src = (lane & 32) + (who ? __ffs((int)who) - 1 : 0);
      const int nn_s = __shfl(bid, src);
      if (acc) {
        bool tie = false;
        if (mk != 0xFFFFFFFFu) {
          nn = nn_s;
          d2 = __uint_as_float(mk);
          tie = __popc(who) > 1 || tl != 0u;
          if (tie && l32 == 0) atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_TIE_CLS);
        }
        cls = ((nn >= 0 && sqrtf(d2) < p.robot_size) ? 1 : 2) | (tie ? SLOT_TIE : 0);
      }
      if (l32 == 0 && have_slot) {
        float4 *rec = (float4 *)&B.slot_rec[slot];
        rec[0] = make_float4(qx, qy, acc ? P.sz[j] : 0.0f, d2);
        rec[1] = make_float4(__int_as_float(nn), __int_as_float(cls), __int_as_float(EDGE_GATE), 0.0f);
        if ((cls & SLOT_CLS_MASK) == 2) B.slot_rec[slot].ndisc = P.sn[j];  // (only a candidate can become a node)
        B.c_outcome[slot] = 0;  // undecided (k_level_resolve polls the candidates' outcomes)
        V.cand[j] = cls & SLOT_CLS_MASK;
      }
    }
  }
  // (the candidates' hash entries for k_level_resolve are written by k_level_spec, by each candidate's own wave:
  // three dependent round trips that were the last 3-4 us of every workgroup here)
  __syncthreads();
  LV_PHASE(3)
  // which samples are candidates (their speculative parent edges follow in k_level_spec.  Evaluating
  // them here, candidate k on wave k mod LSW, was measured: the workgroups stay resident two to three
  // times as long and the build is 8 ms slower)
  const unsigned long long cand_mask = ballot(lane < S && V.cand[lane < S ? lane : 0] == 2);  // (every wave)
  LV_PHASE(4)
  // per-node record; the counts become final when k_level_resolve commits the level, so a launch that is later
  // discarded (the speculative next level) counts nothing
  if (tid == 0) {
    int4 *nr = (int4 *)&B.node_rec[node];
    nr[0] = make_int4(n_acc, draws, (int)hits_node, 0);
    nr[1] = make_int4((int)(unsigned)cand_mask, (int)(unsigned)(cand_mask >> 32), 0, 0);
    ((float4 *)nr)[2] = make_float4(px, py, pz, __int_as_float(V.pdisc));
    if (ties_node && ctr) atomicAdd(&ctr[wg % COUNTER_SHARDS].nn_ties, (unsigned long long)ties_node);
    TL_MARK(tag, 1, node);
  }
  LV_PHASE(5)
}

// NW = LSW (4) for levels that fill the chip; NW = 8 for small levels (launch_level_expand): twice the draws per
// round, and a small level waits for its slowest node -- next to walls that is hundreds of rejected draws
// (indoor.yaml: 62 -> 4x us per level) -- while residency does not matter when every workgroup is resident anyway.
template <int NW>
__global__ __launch_bounds__(NW *WAVE, NW == LSW ? LV_WAVES_PER_SIMD : 4) void k_level_sample(
    MapView m, QueryParams p, const float *cos_t, const float *sin_t, int table_bits, uint32_t seed,
    uint32_t epoch, BfsDev B, int count, const int *count_dev, int node_base, int parity, int tag,
    int pub_stamp, DeviceCounters *ctr) {
  __shared__ SampleSide<NW> SS;
  sample_body<NW>(SS, m, p, cos_t, sin_t, table_bits, seed, epoch, B, count, count_dev, node_base, parity, tag,
                  pub_stamp, ctr, (int)blockIdx.x);
}


// The speculative parent edge of every candidate (a new node is Invalid iff that edge fails,
// trg.cpp:425, 447-449): one wave per sample slot, the waves of non-candidates leave at once.  The
// edge is evaluated like every other one (edge_gather: the capsule around the segment and the
// gather disc staged into a per-wave LDS tile from the L2-resident map), up to its decision (trg.cpp:269-331):
// the level loop reads the status and the length of a slot's edge and nothing else, so the ellipse sweep only
// counts (GATHER_STATUS: no fp64 moments, no reduction, no covariance).  The covariance of the edges that did
// create a node follows in k_node_cov, the SVD after the level loop.
#ifndef TRG_LQW
#define TRG_LQW 1
#endif
constexpr int LQW = TRG_LQW;  // waves per k_level_spec workgroup: small, so that the LDS of a workgroup
                              // whose slots are not candidates is free again at once
// The candidate's entry in the level's hash (cell of the sample -> slot, read by k_level_resolve and
// k_level_spec3 in later launches), written by lane 0 of the candidate's wave once its edge is evaluated.
// Level tags only grow inside a build (the tables are cleared when a build starts) and an entry of another
// level counts as empty, so ONE atomicMax of the tag word claims an entry: an older tag comes back -> it is
// ours; this level's tag comes back -> taken, next entry (linear probing; rare at load factor <= 1/2).
// (At the end of every SAMPLING workgroup a load + CAS + store chain was its last 3-4 us.  Spreading
// the steps over the edge evaluation -- load before it, CAS between the tile's loads and the sweeps, the rest
// after it -- was measured too: the state kept alive across the evaluation costs 15 spilled registers and
// 0.75 ms more than the round trips it hides.)
__device__ __forceinline__ bool level_hash_insert(const BfsDev &B, int tag, int slot, float qx, float qy) {
  static_assert(sizeof(HashEnt) == 32, "the table is addressed as 8 words per entry: cell, tag, slot, -, x, y, -, -");
  bool placed = true;
  if (lane_id() == 0) {
    int *tab = (int *)B.lv_hash;
    const uint32_t mask = (uint32_t)B.ht_size - 1u;
    const int key = bfs_cell_y(B, qy) * B.GW + bfs_cell_x(B, qx);
    uint32_t e = bfs_hash(key) & mask;
    placed = false;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
      int *w = tab + 8 * (size_t)e;
      if (atomicMax(&w[1], tag) < tag) {
        w[0] = key;
        w[2] = slot;
        w[4] = __float_as_int(qx);
        w[5] = __float_as_int(qy);
        placed = true;
        break;
      }
      e = (e + 1) & mask;
    }
  }
  return placed;
}

// one candidate's speculative parent edge (one wave): edge_gather up to the decision, results into the slot's
// record (its cov words are not written here: the host sets them together with w_given, nobody else reads them)
__device__ __forceinline__ void spec_one(const MapView &m, const QueryParams &p, const BfsDev &B, int slot, int node,
                                         int unit, float4 par, float qx, float qy, float qz, WaveTile &tile,
                                         int parity, DeviceCounters *ctr, int tl_tag) {
  const int lane = lane_id();
  if (lane == 0) TL_MARK(tl_tag, 2, unit);
  // (par.w: the parent's own disc count or -1, wave-uniform: a scalar register through the evaluation)
  const int n0 = __builtin_amdgcn_readfirstlane(__float_as_int(par.w));
  const EdgeMidOut o = edge_gather<GATHER_STATUS>(m, p, par.x, par.y, par.z, qx, qy, qz, tile, nullptr, ctr, n0);
  float *out = (float *)&B.slot_rec[slot];
  if (lane == 0) {
    if (edge_start_known(o, n0)) atomicAdd(&B.node_rec[node].spec_known, 1);
    out[6] = __int_as_float(o.status);
    out[7] = o.dist;
    out[14] = __int_as_float(0);  // w_given
    out[15] = __int_as_float(o.hits);
    TL_MARK(tl_tag, 3, unit);
    if (o.hits) atomicAdd(&B.node_rec[node].hits_spec, o.hits);
    if (o.status & EDGE_GATE_UNCERTAIN) {
      const int q = atomicAdd(&B.ctrs[parity ? BFS_CTR_NUNC1 : BFS_CTR_NUNC], 1);
      if (q < BFS_UNC_CAP) {
        const int at = parity * BFS_UNC_CAP + q;
        B.unc_list[at] = slot;
        B.unc_rec[3 * at] = par.z;
        B.unc_rec[3 * at + 1] = qz;
        B.unc_rec[3 * at + 2] = o.dist;
      }
    }
  }
}

// One wave per sample slot, the waves of non-candidates leave at once.  (TRG_KC single-wave workgroups per
// NODE, workgroup k taking the node's k-th candidate from a compact record, were measured: 8 per node
// +5 ms per build, 4 per node +18 ms -- the sequential tail of nodes with many candidates.  A COMPACT CANDIDATE
// LIST -- k_level_sample appending each node's candidates to one of 64 lists with one atomic per node, this
// kernel launched with as many waves as are resident at once, each walking its list -- was measured as well:
// +1 ms at best (4 waves per SIMD, no spills), +4 ms at 5.  The waves that leave at once are not what bounds
// this kernel: a candidate's wave issues ~1150 vector instructions, 4 cycles each, and 5 such waves per SIMD
// ARE the ~9 us a wave lives -- the kernel is bound by vector-instruction issue (12.8 us per level at the
// full issue rate, 25 measured with ramp and tail).  A single list counter, one same-address atomic per
// node, costs 25 us per level.)
__global__ __launch_bounds__(LQW *WAVE, SPEC_WAVES_PER_SIMD) void k_level_spec(MapView m, QueryParams p, BfsDev B,
                                                                            int count, const int *count_dev,
                                                                            int node_base, int parity,
                                                                            DeviceCounters *ctr, int tl_tag) {
  __shared__ WaveTile tiles[LQW];
  const int w = threadIdx.x >> 6;
  const int S = p.sample_num;
  if (count_dev) count = min(count, *count_dev);
  const int slot = node_base * S + blockIdx.x * LQW + w;
  if (slot >= count * S) return;
  // One round trip: the node's candidate mask, the slot's position and the parent's position.  Three
  // slots out of four are no candidates: their waves wait for the FIRST load only (loads return in
  // order) -- the masks of a level are a few KB that every L2 holds after the first touch, the 64-byte
  // slot records come from another XCD's writes.
  const int node = slot / S;
  const int2 cm = *(const int2 *)&B.node_rec[node].cand_lo;
  const float4 r0 = ((const float4 *)&B.slot_rec[slot])[0];  // x y z d0sq
  const float4 par = ((const float4 *)&B.node_rec[node])[2];  // px py pz
  const int j = slot - node * S;
  if (!(((j < 32 ? (unsigned)cm.x : (unsigned)cm.y) >> (j & 31)) & 1u)) return;
  // (the sample's position is wave-uniform: kept in scalar registers across the edge evaluation, which has no
  // vector register to spare)
  const float sqx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(r0.x)));
  const float sqy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(r0.y)));
  spec_one(m, p, B, slot, node, slot - node_base * S, par, r0.x, r0.y, r0.z, tiles[w], parity, ctr, tl_tag);
  if (!level_hash_insert(B, tl_tag, slot, sqx, sqy)) atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_HASH);
}

// (Sampling and speculative edges in ONE launch -- the edge waves dispatched behind the sampling workgroups,
// each polling its node's flag, slot records handed over write-through -- was built and measured: the build
// is 3.4 ms SLOWER.  A launch has one workgroup shape: the edge waves then come four to a 25-KB workgroup
// that stays resident until its slowest wave is through, instead of as single-wave workgroups that free
// their place at once; that costs more than the removed kernel boundary and the overlapped tail give.)

// Decide every sample slot of the level and write its wireEdge call record.  One wave serves RG = 4
// consecutive slots, ONE 16-LANE ROW PER SLOT, RWV waves (= RW slots) per workgroup, so that a whole
// level is resident at once and every reduction is a DPP row operation.
//   Light pass: a sample that has a pre-level node within robot_size ("merge" sample) only needs to
//   know whether an EARLIER candidate of this level lies at least as near; its row probes the few
//   hash cells that could hold one.  Usually there is none and the call record is written at once.
//   Full pass (candidates, and merge samples with such a candidate nearby; the rows of a wave work
//   in parallel):
//     Phase 1: the EARLIER candidates that could become this sample's nearest node -- those closer
//     than its nearest pre-level node -- are collected from the level's hash (lanes take one cell
//     each) into a per-row LDS list; every lane then owns at most NBL of these "blockers".
//     Phase 2: the row polls its undecided blockers (outcomes are agent-scope relaxed atomics in
//     global memory, mirrored in LDS inside a workgroup) and folds the decided ones with row-wide
//     reductions until the sample can be decided.  Dependencies point to LOWER slots only and a
//     workgroup's slots follow from the ticket it draws when it starts, so the lowest undecided slot
//     always belongs to a running workgroup and can decide.
//   Outcomes: 1 skip (nearest node Invalid), 2 wireEdge to the nearest node, 3 create a valid node,
//   4 create an Invalid node, 7 "will not create" (announced early by a candidate that already has
//   a decided node within robot_size, so that later candidates need not wait for it).
// stall_test == 1 (test hook): the first candidate at or after the middle slot stays undecided and
// waits are bounded by max_spin polls; stall_test == 2: the middle workgroup's look-back gives up.
#ifndef TRG_POLL_FREE
#define TRG_POLL_FREE 2   // polls before a waiting wave starts to sleep between polls
#endif
#ifndef TRG_POLL_SLEEP
#define TRG_POLL_SLEEP 2  // s_sleep argument (64 cycles each)
#endif
constexpr int RG = 4;         // slots (= 16-lane rows) per wave
constexpr int RWV = TRG_RWV;  // waves per resolve workgroup
static_assert(RWV * RG == RW, "slots per resolve workgroup");
constexpr int NBL = 4;             // blockers a lane tracks
constexpr int NB_ROW = 16 * NBL;   // blockers a slot can have

struct ResolveLds {
  int so[RW];
  int nb_n[RWV][RG];
  int nb_c[RWV][RG][NB_ROW];
  float nb_d[RWV][RG][NB_ROW];
  int spin_max[RWV];
  int c_flag[RW];  // 0 no node, 1 creates an Invalid node, 2 creates a valid node
  int c_cell[RW];  // grid cell * GRID_SLOTS + reserved place (-1: cell full)
};
static_assert(RW <= WAVE, "the first wave commits one slot per lane");

// minimum of an order-preserving key over the 16 lanes of each row; every lane gets its row's result
__device__ __forceinline__ unsigned row_min_key(unsigned v) {
#define RKEY_STEP(ctrl)                                                                            \
  {                                                                                                \
    const unsigned o = (unsigned)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, ctrl, 0xf, 0xf, \
                                                             false);                               \
    v = o < v ? o : v;                                                                             \
  }
  RKEY_STEP(0x111)  // row_shr:1
  RKEY_STEP(0x112)  // row_shr:2
  RKEY_STEP(0x114)  // row_shr:4
  RKEY_STEP(0x118)  // row_shr:8 -> lane 15 of every row holds the row's minimum
#undef RKEY_STEP
  return (unsigned)__shfl((int)v, (lane_id() & 48) | 15);
}

#ifndef RESOLVE_WAVES_PER_SIMD
#define RESOLVE_WAVES_PER_SIMD 6
#endif
// the plain variant (sample_num <= 32, step 3 off): with the blockers' state packed (three registers per
// blocker instead of six) it fits 64 registers + 10 spilled, i.e. FOUR 8-wave workgroups per CU instead of
// three -- 1 024 resident workgroups, so that a level of up to 2 048 nodes resolves in one residency round:
// -0.35 ms per C3 build (7 waves per SIMD: no spills but still three workgroups per CU, +-0)
#ifndef RESOLVE_WAVES_PER_SIMD_PLAIN
#define RESOLVE_WAVES_PER_SIMD_PLAIN 8
#endif
// an exact fp32 distance tie between two nearest-node candidates of this slot: the reference's answer
// hangs on its kd-tree's visiting order, which the host supplies for the listed slots
__device__ __forceinline__ void report_tie(const BfsDev &B, int slot) {
  atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_TIE);
  const int k = atomicAdd(&B.ctrs[BFS_CTR_NTIE], 1);
  if (k < BFS_TIE_CAP) B.tie_list[k] = slot;
}
// the packed state of a blocker in resolve_body (see there)
constexpr int BL_OPEN = 1, BL_BAD = 2, BL_OC_SHIFT = 2;
// distance key of a blocker once it is decided as a created node (d2 >= 0: the bit pattern orders like the value)
__device__ __forceinline__ unsigned bl_key(int st, float dd) {
  return (st >> BL_OC_SHIFT) ? __float_as_uint(dd) : 0xFFFFFFFFu;
}
// bid / nwg: logical index of this workgroup among the nwg resolve workgroups of the launch
// MULTI: rows with more than NB_ROW blockers take them in several passes (launched for sample_num > 32)
// STEP3: expandGraph's step 3 is on -- a candidate whose parent edge failed may still become a valid node
// through an edge to a neighbour (RescueRec, trg_step3.inc)
template <bool MULTI, bool STEP3>
__device__ __forceinline__ void resolve_body(ResolveLds &R, const BfsDev &B, int m, int S, float d, float r, int tag,
                                             long long call_base, int stall_test, int max_spin, int V0,
                                             int new_state, int epoch, int bid, int nwg) {
  RV_PHASE_BEGIN
  volatile int *vso = R.so;
  const int w = threadIdx.x >> 6, lane = lane_id();
  const int slots = m * S;
  if (threadIdx.x == 0) TL_MARK(tag + 1, 4, bid);
  const int wg_base = bid * RW;
  const int g = lane >> 4, l16 = lane & 15;
  const int rshift = 16 * g;  // this row's bits in a wave ballot
  const int slot = wg_base + w * RG + g;
  float4 r0 = {0, 0, 0, 0}, r1 = {0, 0, 0, 0};
  int u = -1;
  if (slot < slots) {
    const float4 *rec = (const float4 *)&B.slot_rec[slot];
    r0 = rec[0];  // x y z d0sq
    r1 = rec[1];  // nn0 cls status dist
    u = B.front_cur[slot / S];
  }
  if (threadIdx.x < RW) {
    R.so[threadIdx.x] = 0;
    R.c_flag[threadIdx.x] = 0;
  }
  if (threadIdx.x < RWV * RG) R.nb_n[threadIdx.x / RG][threadIdx.x % RG] = 0;
  __syncthreads();
  int cls = 0, nn = -1;
  float qx = 0.0f, qy = 0.0f, lim = FLT_MAX;
  bool nn_valid = true;
  int own_st = 0;
  float own_dist = 0.0f;
  if (slot < slots) {
    cls = __float_as_int(r1.y) & SLOT_CLS_MASK;
    if (cls != 0) {
      qx = r0.x;
      qy = r0.y;
      nn = __float_as_int(r1.x);
      own_st = __float_as_int(r1.z);
      own_dist = r1.w;
      if (nn >= 0) {
        lim = r0.w;
        nn_valid = B.nstate[nn] != -1;
      }
    }
  }
  const bool have = nn >= 0;
  const bool is_cand = cls == 2;
  // ---- phases 1 and 2.  Phase 1: the earlier candidates nearer than the nearest pre-level node ("blockers",
  // a merge sample also takes a candidate exactly as far as that node: the tie is then reported) go from the
  // level's hash into the row's LDS list.  Phase 2 polls and decides.  A row with more than NB_ROW blockers
  // (sample_num >= 48 on open ground) takes them in K passes: pass p holds the blockers whose slot number is
  // p modulo K (the hash is probed again with that filter; K is chosen for ~32 per pass), the nearest
  // created blocker found so far is carried from pass to pass, and the row decides in its last pass.
  const bool own_ok = is_cand && (own_st & EDGE_STATUS_MASK) == EDGE_OK;
  // step 3: the candidate's parent edge failed -- an edge to an older node rescues it outright (pre); the
  // earlier candidates of the level it has an edge to are waited for like blockers (below), and one that
  // became a valid node rescues it too
  bool pre_rescue = false;
  int n_resc = 0;
  if (STEP3 && is_cand && !own_ok) {
    const int2 pn2 = *(const int2 *)&B.resc[slot];
    pre_rescue = pn2.x != 0;
    n_resc = pre_rescue ? 0 : min(pn2.y, RESC_MAX);
  }
  bool rescued = false;  // (this lane saw a rescuer become a valid node)
  // test hook: the first candidate at or after the middle slot of the level stays undecided
  bool hold = false;
  if (stall_test == 1 && is_cand && slot >= slots / 2) {
    bool earlier = false;
    for (int i = slots / 2 + l16; i < slot; i += 16) earlier |= (B.slot_rec[i].cls & SLOT_CLS_MASK) == 2;
    hold = ((ballot(earlier) >> rshift) & 0xFFFFull) == 0ull;
  }
  bool announced = !is_cand;  // nobody waits for a non-candidate
  bool done = cls == 0 || hold;
  int outcome = 0, target = -1, spin = 0;
  int K = 1, pass = 0;                  // (row-uniform)
  unsigned car_key = 0xFFFFFFFFu;       // nearest created blocker of the passes already finished ...
  int car_c = -1, car_o = 0;            // ... its slot and outcome
  bool car_tie = false;
  bool first_probe = true;
  bool need_probe = cls != 0;
  for (;;) {
    if (ballot(need_probe) != 0ull) {
      if (!first_probe) {
        if (need_probe && l16 == 0) R.nb_n[w][g] = 0;
        wave_lds_sync();
      }
      if (need_probe) {
        const float rad = have ? sqrtf(lim) : d * 1.01f;
        const float rp = rad * 1.001f + 1e-6f;
        const int cx0 = bfs_cell_x(B, qx - rp), cx1 = bfs_cell_x(B, qx + rp);
        const int cy0 = bfs_cell_y(B, qy - rp), cy1 = bfs_cell_y(B, qy + rp);
        const int nxc = cx1 - cx0 + 1;
        const int ncell = nxc * (cy1 - cy0 + 1);
        const uint32_t mask = (uint32_t)B.ht_size - 1u;
        const bool filtered = MULTI && K > 1;
        // one entry of a cell's probe sequence; false: the sequence ends here (an entry of another level)
        auto consume = [&](const int4 h0, const float4 h1, int key) -> bool {
          if (h0.y != tag) return false;
          if (h0.x == key) {
            const int s2 = h0.z;
            if (s2 < slot && (!filtered || s2 % K == pass)) {
              const float d2 = bfs_d2(h1.x, h1.y, qx, qy);
              if (d2 < lim) {
                const int pos = atomicAdd(&R.nb_n[w][g], 1);
                if (pos < NB_ROW) {
                  R.nb_c[w][g][pos] = s2;
                  R.nb_d[w][g][pos] = d2;
                }
              } else if (d2 == lim && have && first_probe) {
                report_tie(B, slot);
              }
            }
          }
          return true;
        };
        // Two cells per lane and two entries per cell are fetched at once (the table is at most half
        // full: a probe sequence rarely goes further), so the usual case is ONE memory round trip.
        for (int l = l16; l < ncell; l += 32) {
          const int la = l, lb = l + 16;
          const bool has_b = lb < ncell;
          const int key_a = (cy0 + la / nxc) * B.GW + (cx0 + la % nxc);
          const int key_b = has_b ? (cy0 + lb / nxc) * B.GW + (cx0 + lb % nxc) : key_a;
          const uint32_t ia = bfs_hash(key_a) & mask, ib = bfs_hash(key_b) & mask;
          const int4 *ea0 = (const int4 *)&B.lv_hash[ia], *ea1 = (const int4 *)&B.lv_hash[(ia + 1) & mask];
          const int4 *eb0 = (const int4 *)&B.lv_hash[ib], *eb1 = (const int4 *)&B.lv_hash[(ib + 1) & mask];
          const int4 a0 = ea0[0], a1 = ea1[0], b0 = eb0[0], b1 = eb1[0];
          const float4 a0h = *(const float4 *)&ea0[1], a1h = *(const float4 *)&ea1[1];
          const float4 b0h = *(const float4 *)&eb0[1], b1h = *(const float4 *)&eb1[1];
          bool more_a = consume(a0, a0h, key_a) && consume(a1, a1h, key_a);
          bool more_b = has_b && consume(b0, b0h, key_b) && consume(b1, b1h, key_b);
          uint32_t i = (ia + 2) & mask;
          for (int probe = 2; more_a && probe < B.ht_size; ++probe) {
            const int4 *en = (const int4 *)&B.lv_hash[i];
            more_a = consume(en[0], *(const float4 *)&en[1], key_a);
            i = (i + 1) & mask;
          }
          i = (ib + 2) & mask;
          for (int probe = 2; more_b && probe < B.ht_size; ++probe) {
            const int4 *en = (const int4 *)&B.lv_hash[i];
            more_b = consume(en[0], *(const float4 *)&en[1], key_b);
            i = (i + 1) & mask;
          }
        }
      }
      wave_lds_sync();
    }
    int n = (cls != 0 && !done) ? R.nb_n[w][g] : 0;
    if (first_probe) {
      first_probe = false;
      RV_PHASE(0)  // records + blockers collected from the hash
      if (threadIdx.x == 0) TL_MARK(tag + 1, 5, bid);
      if (MULTI) {
        if (n > NB_ROW) {
          K = (n + 31) / 32;
          if (l16 == 0) atomicAdd(&B.stats64[7], 1ull);  // (instrumentation: rows that went multi-pass)
        }
        need_probe = K > 1;
        if (ballot(need_probe) != 0ull) continue;  // those rows collect again: pass 0 of K
      }
    }
    if (STEP3 && pass == 0) {  // the rescuers join pass 0's list (distance -1 marks them)
      if (l16 < n_resc && !done) {
        const int pos = atomicAdd(&R.nb_n[w][g], 1);
        if (pos < NB_ROW) {
          R.nb_c[w][g][pos] = B.resc[slot].slot[l16];
          R.nb_d[w][g][pos] = -1.0f;
        }
      }
      wave_lds_sync();
      if (n_resc > 0 && !done) n = R.nb_n[w][g];
    }
    if (n > NB_ROW) {  // (a pass of a filtered row still too long: give up as before)
      if (l16 == 0) atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_NB_OVERFLOW);
      n = NB_ROW;
    }
    const bool last_pass = !MULTI || pass >= K - 1;
    // blockers per lane any row of this wave really needs (wave-uniform: the loops below skip the rest)
    int nq = 0;
#pragma unroll
    for (int q = 1; q <= NBL; ++q) nq += ballot(n > 16 * (q - 1)) != 0ull;
    // per blocker: its slot, its squared distance, and one packed word (three arrays of NBL registers instead
    // of six): bit 0 = still undecided and still able to matter, bit 1 = would be an INVALID node if created,
    // bits 2.. = its outcome once it is decided as a created node (3 or 4)
    int c2[NBL], st[NBL];
    float dd[NBL];
#pragma unroll
    for (int q = 0; q < NBL; ++q) {
      const int idx = l16 + 16 * q;
      c2[q] = -1;
      st[q] = 0;
      dd[q] = FLT_MAX;
      if (idx < n) {
        c2[q] = R.nb_c[w][g][idx];
        dd[q] = R.nb_d[w][g][idx];
        st[q] = (((B.slot_rec[c2[q]].status & EDGE_STATUS_MASK) == EDGE_OK) ? 0 : BL_BAD) | BL_OPEN;
      }
    }

    // ---- phase 2: poll and decide (all rows of the wave at once) -------------------------------------
    bool pdone = done;  // this pass is over for the row (decided, or its blockers of this pass are through)
    while (ballot(!pdone) != 0ull && spin < max_spin) {  // usual maximum: a few dozen polls
      // a waiting wave steps aside (the hardware issues older waves first)
      if (spin > TRG_POLL_FREE) __builtin_amdgcn_s_sleep(TRG_POLL_SLEEP);
      ++spin;
      if (!pdone) {
#pragma unroll
        for (int q = 0; q < NBL; ++q) {
          if (q < nq && (st[q] & BL_OPEN)) {
            const int cq = c2[q];
            const int o2 = cq >= wg_base ? vso[cq - wg_base] : outcome_load(&B.c_outcome[cq]);
            if (STEP3 && dd[q] < 0.0f) {  // a rescuer: only whether it became a valid node matters
              if (o2 == 3) rescued = true;
            } else if (o2 == 3 || o2 == 4) {
              st[q] |= o2 << BL_OC_SHIFT;
            }
            if (o2 != 0) st[q] &= ~BL_OPEN;
          }
        }
        // nearest DECIDED node: among the created blockers and the pre-level node (every blocker is
        // strictly nearer than the pre-level node by construction)
        unsigned kmin = bl_key(st[0], dd[0]);
        int qmin = 0;
        int local_ties = 1;
        if (nq > 1) {
#pragma unroll
          for (int q = 1; q < NBL; ++q) {
            const unsigned kq = bl_key(st[q], dd[q]);
            if (kq < kmin) {
              kmin = kq;
              qmin = q;
            }
          }
          local_ties = 0;
#pragma unroll
          for (int q = 0; q < NBL; ++q) local_ties += (bl_key(st[q], dd[q]) == kmin);
        }
        unsigned mkey = row_min_key(kmin);
        float best = FLT_MAX;
        int bestc = -1, best_outcome = 0;
        bool tie = false, exists = false;
        if (mkey != 0xFFFFFFFFu) {
          const unsigned rowbits = (unsigned)(ballot(kmin == mkey) >> rshift) & 0xFFFFu;
          const int src = rshift + __ffs((int)rowbits) - 1;
          int cmin = c2[0], omin = st[0] >> BL_OC_SHIFT;
          if (nq > 1) {
#pragma unroll
            for (int q = 1; q < NBL; ++q)
              if (q == qmin) {
                cmin = c2[q];
                omin = st[q] >> BL_OC_SHIFT;
              }
          }
          bestc = __shfl(cmin, src);
          best_outcome = __shfl(omin, src);
          tie = __popc(rowbits) > 1 || ((ballot(kmin == mkey && local_ties > 1) >> rshift) & 0xFFFFull) != 0ull;
        }
        if (MULTI) {  // ... and the nearest created blocker of the passes before this one
          if (car_key < mkey) {
            mkey = car_key;
            bestc = car_c;
            best_outcome = car_o;
            tie = car_tie;
          } else if (car_key == mkey && mkey != 0xFFFFFFFFu) {
            tie = true;
          }
        }
        if (mkey != 0xFFFFFFFFu) {
          best = __uint_as_float(mkey);
          exists = true;
        } else if (have) {
          best = lim;
          exists = true;
        }
        // an undecided blocker farther than the nearest decided node can no longer matter
        bool any_open = false, any_risky = false;
#pragma unroll
        for (int q = 0; q < NBL; ++q) {
          if (q < nq) {
            if ((st[q] & BL_OPEN) && dd[q] > best) st[q] &= ~BL_OPEN;
            any_open |= (st[q] & BL_OPEN) != 0;
            any_risky |= (st[q] & BL_OPEN) != 0 && (!(sqrtf(dd[q]) >= r) || (st[q] & BL_BAD) != 0);
          }
        }
        const bool wait_exact = ((ballot(any_open) >> rshift) & 0xFFFFull) != 0ull;
        const bool wait_create = ((ballot(any_risky) >> rshift) & 0xFFFFull) != 0ull;
        const bool near = exists && sqrtf(best) < r;
        const bool best_valid = bestc >= 0 ? best_outcome == 3 : nn_valid;
        // a created node is valid if its parent edge holds -- or, with step 3, an edge to a neighbour
        const bool new_ok = own_ok || (STEP3 && (pre_rescue || ((ballot(rescued) >> rshift) & 0xFFFFull) != 0ull));
        // (1) a decided node within robot_size: no node will be created here -- tell the others
        if (!announced && near) {
          if (l16 == 0) {
            vso[slot - wg_base] = 7;
            outcome_store(&B.c_outcome[slot], 7);
          }
          announced = true;
        }
        if (!wait_exact && !last_pass) {
          // this pass's blockers are through: what they left goes on to the next pass
          car_key = mkey;
          car_c = bestc;
          car_o = best_outcome;
          car_tie = tie;
          pdone = true;
        } else if (!wait_exact) {
          if (tie && l16 == 0) report_tie(B, slot);
          if (exists && !best_valid) {
            outcome = 1;
          } else if (near) {
            outcome = 2;
            target = bestc >= 0 ? call_ref(call_at(B, call_base, bestc)) : nn;
          } else {
            outcome = new_ok ? 3 : 4;
          }
        } else if (RESOLVE_EARLY_CREATE && K == 1 && is_cand && !wait_create && !near && (!exists || best_valid) &&
                   !tie) {
          // (2) every undecided blocker is >= robot_size away and would be a valid node: whatever
          // they do, the nearest node stays valid and >= robot_size away -> this one creates
          // (an undecided rescuer counts as such a blocker, so here they are all decided)
          outcome = new_ok ? 3 : 4;
        }
        if (outcome) {
          if (is_cand && l16 == 0) {
            vso[slot - wg_base] = outcome;
            outcome_store(&B.c_outcome[slot], outcome);
          }
          done = true;
          pdone = true;
        }
      }
    }
    if (!MULTI) break;
    ++pass;
    need_probe = !done && cls != 0 && pass < K;
    if (ballot(need_probe) == 0ull || spin >= max_spin) break;
  }
  RV_PHASE(1)  // the first wave's slots decided
  if (threadIdx.x == 0) TL_MARK(tag + 1, 6, bid);
  if (cls != 0 && outcome == 0 && l16 == 0) atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_STALL);  // bounded wait ran out
  // ---- the call record of this slot (trg.cpp:414-417, 425) -------------------------------------------
  if (slot < slots && l16 == 0) {
    int n2 = -1, st = CALL_NONE;
    float wgt = 0.0f, dist = 0.0f;
    if (outcome == 2) {
      n2 = target;
      st = CALL_PENDING;
    } else if (outcome == 3) {  // the weight follows after the loop (k_node_weights)
      n2 = call_ref(call_at(B, call_base, slot));
      st = own_st & EDGE_STATUS_MASK;
      dist = own_dist;
    }
    const size_t at = (size_t)call_at(B, call_base, slot);
    B.call_n1[at] = u;
    B.call_n2[at] = n2;
    B.call_status[at] = (n2 == u) ? CALL_NONE : st;
    B.call_w[at] = wgt;
    B.call_dist[at] = dist;
  } else if (slot < slots && l16 < B.cstride) {  // the slot's step-3 entries start out empty
    B.call_status[(size_t)call_at(B, call_base, slot) + l16] = CALL_NONE;
  }
  // ---- what the commit needs of this workgroup (trg.cpp:233-252 addNode in sequence order; the queue push :450)
  // A new node's id is V0 + the nodes created by lower slots, known only when every lower slot is
  // decided.  Everything that does not need the id happens here, in the slot's own wave: its place in
  // the node grid is reserved (c_cell), the workgroup's counts are published (wg_state) -- and the
  // workgroup LEAVES: its registers, wave slots and LDS go to the resolve workgroups still waiting to
  // start.  The numbering itself is done by the commit workgroups at the end of the launch
  // (commit_role).  (Keeping the first wave of every workgroup resident through a look-back scan made a
  // level of 1 226 workgroups take two residency rounds of ~21 us each on the 768 places of the chip.)
  const bool created = is_cand && (outcome == 3 || outcome == 4) && l16 == 0;
  const bool valid = is_cand && outcome == 3 && l16 == 0;
  if (slot < slots && l16 == 0) {
    const int ls = w * RG + g;
    if (slot % S == 0) {  // per-node statistics of the expansion, summed after the loop (k_bfs_stats)
      const int4 nr = *(const int4 *)&B.node_rec[slot / S];  // n_acc draws hits_sample hits_spec
      const NodeRec &full = B.node_rec[slot / S];
      const int ncand = __popc(full.cand_lo) + __popc(full.cand_hi);
      // (n_acc and the candidates are at most LV_SMAX = 64, and so are the known start discs among them)
      *(int4 *)&B.nexp[u] = make_int4(nr.x | (ncand << 8) | (full.spec_known << 16), nr.y, nr.z, nr.w);
    }
    if (created) {
      const int cell = bfs_cell_y(B, qy) * B.GW + bfs_cell_x(B, qx);
      GridCell &c = B.gcell[cell];
      const int pos = atomicAdd(&c.cnt, 1);
      if (pos < GRID_SLOTS) {
        c.x[pos] = qx;
        c.y[pos] = qy;
      } else {
        atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_GRID_OVERFLOW);
      }
      R.c_cell[ls] = pos < GRID_SLOTS ? cell * GRID_SLOTS + pos : -1;
    }
    R.c_flag[ls] = created ? (valid ? 2 : 1) : 0;
  }
  if (lane == 0) R.spin_max[w] = spin;
  RV_PHASE(2)  // call records, grid reservation
  __syncthreads();
  if (w != 0) return;
  RV_PHASE(3)  // the other waves' slots decided
  const int flag = lane < RW ? R.c_flag[lane] : 0;  // local slot == lane
  const unsigned long long cb = ballot(flag != 0), vb = ballot(flag == 2);
  int sm = 0;
  for (int i = 0; i < RWV; ++i) sm = max(sm, R.spin_max[i]);
  // what the commit workgroup needs of every slot -- creates a node? where in the grid? -- goes out from
  // this one wave; every word carries the launch's epoch, so the reader needs no ordering between these
  // stores and the workgroup's word (a release fence here would write back everything the workgroup
  // left in the L2: 7 us)
  const unsigned long long ep = (unsigned long long)(unsigned)epoch & 0xFFFFFull;  // words: epoch:20 state:2 ...
  if (lane < RW && wg_base + lane < slots)
    __hip_atomic_store(&B.c_cell[wg_base + lane],
                       (ep << 44) | ((unsigned long long)(unsigned)flag << 42) | (unsigned)(flag ? R.c_cell[lane] : 0),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (lane == 0) {
    const unsigned long long own_c = (unsigned long long)__popcll(cb), own_v = (unsigned long long)__popcll(vb);
    __hip_atomic_store(&B.wg_state[bid], (ep << 44) | (1ull << 42) | (own_c << 21) | own_v, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);  // epoch:20 state:2 created:21 valid:21
    if (sm > 0) atomicMax(&B.stats64[6], (unsigned long long)sm);
    TL_MARK(tag + 1, 7, bid);
  }
  RV_PHASE(4)
}

// Commit workgroup c of a resolve launch: numbers the nodes created by the slots of the resolve workgroups
// [c * CRW, (c + 1) * CRW) -- a new node's id is V0 + the nodes created by lower slots (creation order) --
// and appends them to the node store, the node grid (the reserved place gets its id) and the next
// frontier.  Every thread sums the published counts of a share of ALL lower
// resolve workgroups (a few loads each; they are published long before, when those workgroups left), so
// no commit workgroup waits for another one.  The last one writes the level's totals.
constexpr int CRW = RWV * WAVE / RW;  // resolve workgroups per commit workgroup (one thread per slot)
struct CommitLds {
  int red_c[RWV], red_v[RWV];
  int pre_c[CRW + 1], pre_v[CRW + 1];
  int failed;
};
__device__ __forceinline__ void commit_role(CommitLds &C, const BfsDev &B, int m, int S, long long call_base,
                                            int stall_test, int max_spin, int V0, int new_state, int epoch, int c,
                                            int nR, int nC, int tl_tag) {
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const int slots = m * S;
  if (tid == 0) TL_MARK(tl_tag, 10, c);
  const int first = c * CRW, last = min(first + CRW, nR);
  const unsigned long long ep = (unsigned long long)(unsigned)epoch & 0xFFFFFull;
  if (tid <= CRW) {
    C.pre_c[tid] = 0;
    C.pre_v[tid] = 0;
  }
  if (tid == 0) C.failed = (stall_test == 2 && c == nC / 2) ? 1 : 0;  // test hook: this workgroup gives up
  __syncthreads();
  // the slot's own words first, so that their round trips overlap the sums over the lower workgroups
  const int slot = first * RW + tid;
  int flag = 0, cp = -1;
  if (slot < slots) {  // the slot's own word (stamped with the launch's epoch; its workgroup has left)
    long long polls = 0;
    for (;;) {
      const unsigned long long fc = __hip_atomic_load(&B.c_cell[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((fc >> 44) == ep) {
        flag = (int)((fc >> 42) & 3ull);
        cp = (int)(unsigned)fc;
        break;
      }
      if (++polls > 64ll * max_spin) {
        atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_LOOKBACK);
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
  }
  float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f);  // x y z -
  int4 s2 = make_int4(0, 0, 0, 0), s3 = s2;      // cov0..3 | cov4 cov5 w_given hits
  if (flag != 0) {
    const int4 *src = (const int4 *)&B.slot_rec[slot];
    r0 = ((const float4 *)src)[0];
    s2 = src[2];
    s3 = src[3];
  }
  int sum_c = 0, sum_v = 0;
  for (int i = tid; i < last; i += RWV * WAVE) {
    unsigned long long v = 0;
    long long polls = 0;
    for (;;) {
      v = __hip_atomic_load(&B.wg_state[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((v >> 44) == ep && ((v >> 42) & 3ull) != 0ull) break;
      if (++polls > 64ll * max_spin || *(volatile int *)&C.failed) {  // bounded: the resolve workgroup never published
        C.failed = 1;
        v = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(4);
    }
    const int cc = (int)((v >> 21) & 0x1FFFFFull), vv = (int)(v & 0x1FFFFFull);
    if (i < first) {
      sum_c += cc;
      sum_v += vv;
    } else {
      C.pre_c[i - first + 1] = cc;
      C.pre_v[i - first + 1] = vv;
    }
  }
  sum_c = wave_sum(sum_c);
  sum_v = wave_sum(sum_v);
  if (lane == 0) {
    C.red_c[w] = sum_c;
    C.red_v[w] = sum_v;
  }
  __syncthreads();
  if (C.failed) {
    if (tid == 0) atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_LOOKBACK);
    return;
  }
  if (tid == 0) {  // exclusive prefixes: pre[k] = created by everything before resolve workgroup first + k
    int ac = 0, av = 0;
    for (int i = 0; i < RWV; ++i) {
      ac += C.red_c[i];
      av += C.red_v[i];
    }
    for (int k = 0; k <= CRW; ++k) {
      ac += C.pre_c[k];
      av += C.pre_v[k];
      C.pre_c[k] = ac;
      C.pre_v[k] = av;
    }
    if (c == nC - 1) {  // the level's totals
      B.ctrs[BFS_CTR_V] = V0 + C.pre_c[last - first];
      B.ctrs[BFS_CTR_MNEXT] = C.pre_v[last - first];
    }
  }
  __syncthreads();
  if (tid == 0) TL_MARK(tl_tag, 11, c);
  // ---- one thread per slot: the node store, the grid entry's id, the next frontier ------------------------
  static_assert(WAVE % RW == 0, "a wave of the commit covers whole resolve workgroups");
  const unsigned long long cb = ballot(flag != 0), vb = ballot(flag == 2);
  if (flag == 0) return;
  // the lanes of this slot's resolve workgroup that come before it
  const unsigned long long gmask = (RW == 64 ? ~0ull : ((1ull << (RW % 64)) - 1ull)) << ((lane / RW) * RW);
  const unsigned long long below = lanemask_lt() & gmask;
  const int k = tid / RW;  // resolve workgroup first + k
  const int before_c = C.pre_c[k] + __popcll(cb & below);
  const int before_v = C.pre_v[k] + __popcll(vb & below);
  const int id = V0 + before_c;
  B.newid_of_call[call_at(B, call_base, slot)] = id;
  if (id < B.vcap) {
    B.nx[id] = r0.x;
    B.ny[id] = r0.y;
    B.nz[id] = r0.z;
    B.nstate[id] = flag == 2 ? new_state : -1;
    B.nhits[id] = s3.w;  // map points inside the parent-edge queries (trg.cpp:425)
    if (B.ndisc) B.ndisc[id] = s3.y;  // SlotRec::ndisc: the node is this sample, its acceptance disc held that many
    if (flag == 2) {  // what the weight of the creating edge still needs: w_given (then cov[0] is the weight) and
                      // the call.  The cov words of a slot without w_given are stale (k_level_spec does not write
                      // them) and are copied all the same -- one 16-byte store, no branch: k_node_cov overwrites
                      // all six before k_node_weights reads them
      int4 *dst = (int4 *)&B.ncov[id];
      dst[0] = s2;
      dst[1] = make_int4(s3.x, s3.y, s3.z, (int)call_at(B, call_base, slot));
    }
    if (cp >= 0) B.gcell[cp / GRID_SLOTS].id[cp % GRID_SLOTS] = id;
  } else {
    atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_VCAP);
  }
  if (flag == 2) {
    if (before_v < B.fcap) {
      B.front_next[before_v] = id;
      B.fxy_next[before_v] = make_float2(r0.x, r0.y);
    } else {
      atomicOr(&B.ctrs[BFS_CTR_ERR], BFS_ERR_LEVEL_TOO_BIG);
    }
  }
}

// The launch: nR resolve workgroups, then nC commit workgroups.  TICKET = false: a workgroup's logical index is blockIdx.x -- the waits (for
// lower indices only) then rely on the hardware starting workgroups in index order, which it does but
// does not promise; all waits are bounded, and a launch whose wait ran out is repeated with TICKET = true:
// the logical index is a ticket drawn at the start, so a lower index belongs to a workgroup that is
// already running by construction (always-on tickets cost 1.5 ms per C3 build: one contended atomic
// per workgroup at the head of every launch's dependency chain).
template <bool TICKET, bool MULTI, bool STEP3>
__global__ __launch_bounds__(RWV *WAVE, (MULTI || STEP3) ? RESOLVE_WAVES_PER_SIMD : RESOLVE_WAVES_PER_SIMD_PLAIN) void k_level_resolve(
    BfsDev B, int m, int S, float d, float r, int tag, long long call_base, int stall_test, int max_spin, int V0,
    int new_state, int epoch, int nR, int nC, unsigned ticket_base) {
  __shared__ union {
    ResolveLds R;
    CommitLds C;
  } sh;
  __shared__ int wg_ticket;
  int bid = (int)blockIdx.x;
  if (TICKET) {
    if (threadIdx.x == 0) wg_ticket = (int)(atomicAdd(B.ticket, 1u) - ticket_base);
    __syncthreads();
    bid = wg_ticket;
  }
  if (bid >= nR + nC) return;
  // The expansion in front of this launch (sampling, speculative edges, a top-up launch, the kernel boundaries up
  // to here) has drained: its wall-clock ticks into the sum, and the stamp cleared, so that a rerun of this
  // launch adds nothing.  One thread, plain loads and stores: the kernels of one stream order them.
  if (bid == 0 && threadIdx.x == 0) {
    const unsigned long long t0 = B.stats64[STATS64_EXPAND_START];
    if (t0) {
      B.stats64[STATS64_EXPAND_TICKS] += (unsigned long long)wall_clock64() - t0;
      B.stats64[STATS64_EXPAND_START] = 0ull;
    }
  }
  if (bid >= nR) {
    commit_role(sh.C, B, m, S, call_base, stall_test, max_spin, V0, new_state, epoch, bid - nR, nR, nC, tag + 1);
  } else {
    resolve_body<MULTI, STEP3>(sh.R, B, m, S, d, r, tag, call_base, stall_test, max_spin, V0, new_state, epoch, bid, nR);
  }
}

// Statistics of the whole expansion, once after the level loop: every valid node was expanded exactly
// once and left its draw / sample / hit counts in nexp; every created node the map points its parent
// edge touched.  out[0..5] = draws, samples, hits of sampling discs, hits of speculative edges,
// candidates, hits of the created nodes' parent edges; stats64[STATS64_SPEC_KNOWN] += speculative edges whose first disc was known.
constexpr int BFS_STATS_N = 7;
__global__ __launch_bounds__(256) void k_bfs_stats(BfsDev B, int V, unsigned long long *out) {
  __shared__ unsigned long long red[BFS_STATS_N][4];
  unsigned long long a[BFS_STATS_N] = {0, 0, 0, 0, 0, 0, 0};
  for (int id = blockIdx.x * 256 + threadIdx.x; id < V; id += gridDim.x * 256) {
    if (B.nstate[id] != -1) {
      const int4 n = *(const int4 *)&B.nexp[id];
      a[0] += (unsigned long long)n.y;
      a[1] += (unsigned long long)(n.x & 0xFF);
      a[2] += (unsigned long long)n.z;
      a[3] += (unsigned long long)n.w;
      a[4] += (unsigned long long)((n.x >> 8) & 0xFF);
      a[6] += (unsigned long long)((n.x >> 16) & 0xFF);
    }
    if (id > 0) a[5] += (unsigned long long)B.nhits[id];
  }
#pragma unroll
  for (int q = 0; q < BFS_STATS_N; ++q) {
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) a[q] += __shfl_xor(a[q], msk);
    if (lane_id() == 0) red[q][threadIdx.x >> 6] = a[q];
  }
  __syncthreads();
  if (threadIdx.x < BFS_STATS_N) {
    const unsigned long long t = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    // where sum q goes: the six contiguous words the caller names, and the word of its own behind them
    unsigned long long *const dst[BFS_STATS_N] = {&out[0], &out[1], &out[2], &out[3], &out[4], &out[5],
                                                  &B.stats64[STATS64_SPEC_KNOWN]};
    if (t) atomicAdd(dst[threadIdx.x], t);
  }
}

// The covariance of the gather (trg.cpp:304-338) of the edge parent -> created node, for the nodes [v_lo, v_hi)
// of levels that are final (the driver: all of them in one launch after the loop): one wave per node.
// k_level_spec found the edge EDGE_OK with the same two positions (the parent's nx / ny / nz, and the sample's
// x, y, z the commit stored as the node's), so GATHER_MOMENTS stages the same tile and leaves the same moments a
// full evaluation would have.  Skips Invalid nodes, nodes whose weight the host supplied (w_given) and nodes
// whose creating edge failed (step 3 rescued them).  Counts nothing: the edge's map hits were counted when
// k_level_spec evaluated it.
// Invariant: every NodeCov that k_node_weights reads without w_given was written here in this build.
constexpr int NCW = 4;  // waves (= nodes) per workgroup, like the other edge kernels (measured at C3: single-wave
                        // workgroups +0.05 ms per build, 8 waves +0.2)
__global__ __launch_bounds__(NCW *WAVE, EDGE_WAVES_PER_SIMD) void k_node_cov(MapView m, QueryParams p, BfsDev B, int v_lo,
                                                                          int v_hi) {
  __shared__ WaveTile tiles[NCW];
  __shared__ alignas(16) float mids[NCW][MID_STRIDE];
  const int w = threadIdx.x >> 6, lane = lane_id();
  const int id = v_lo + blockIdx.x * NCW + w;
  if (id < 1 || id >= min(v_hi, B.vcap) || B.nstate[id] == -1) return;  // (wave-uniform, like every exit below)
  const int2 gc = *(const int2 *)&B.ncov[id].w_given;  // w_given, call
  if (gc.x) return;
  const size_t at = (size_t)gc.y;
  const int st = B.call_status[at];
  if (st < 0 || (st & EDGE_STATUS_MASK) != EDGE_OK) return;
  const int par = B.call_n1[at];
  float *rec = mids[w];
  const EdgeMidOut o = edge_gather<GATHER_MOMENTS>(m, p, B.nx[par], B.ny[par], B.nz[par], B.nx[id], B.ny[id],
                                                   B.nz[id], tiles[w], rec, nullptr);
  wave_lds_sync();  // the moments edge_gather left in rec
  if (lane < 6) {   // the six entries on six lanes
    double sm[9];
    const double *src = (const double *)(rec + MID_MOMENTS);
#pragma unroll
    for (int i = 0; i < 9; ++i) sm[i] = src[i];
    B.ncov[id].cov[lane] = cov_entry(sm, o.n_pts, lane);
  }
}

// The weights of the edges parent -> created node (trg.cpp:339-363: JacobiSVD of the covariance ->
// |z| of the two leading singular vectors -> 0.8 / 0.2 blend -> < 0.1 clamp), for all nodes the BFS
// created, after the level loop: nothing inside the loop depends on them.
__global__ __launch_bounds__(256) void k_node_weights(BfsDev B, int V) {
  const int id = 1 + blockIdx.x * blockDim.x + threadIdx.x;  // node 0 is the root
  if (id >= V || B.nstate[id] == -1) return;
  const NodeCov nc = B.ncov[id];
  const size_t at = (size_t)nc.call;
  int st = B.call_status[at];
  if (st < 0 || (st & EDGE_STATUS_MASK) != EDGE_OK) return;
  float w;
  if (nc.w_given) {
    w = nc.cov[0];
  } else {
    float cov[3][3];
    cov[0][0] = nc.cov[0];
    cov[0][1] = cov[1][0] = nc.cov[1];
    cov[0][2] = cov[2][0] = nc.cov[2];
    cov[1][1] = nc.cov[3];
    cov[1][2] = cov[2][1] = nc.cov[4];
    cov[2][2] = nc.cov[5];
    int clamped = 0;
    w = risk_weight(cov, clamped);
    st |= clamped;
  }
  B.call_w[at] = w;
  B.call_status[at] = st;
}
