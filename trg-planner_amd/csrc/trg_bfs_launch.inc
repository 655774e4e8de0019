// trg_bfs_launch.inc -- host launchers of the device-resident BFS kernels (included into
// trg_kernels.hip, namespace trg).

void launch_bfs_insert_nodes(const BfsDev &B, int first, int count, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_bfs_insert_nodes, dim3((count + 255) / 256), dim3(256), 0, s, B, first, count);
}

bool level_kernels_support(const QueryParams &p, float grid_cell) {
  if (p.sample_num < 1 || p.sample_num > LV_SMAX || !(grid_cell > 0.0f)) return false;
  const int K = (int)ceilf(p.expand_dist * 2.01f / grid_cell) + 1;
  return 2 * K + 1 <= LV_WIN_MAX;
}

void launch_level_expand(const MapView &m, QueryParams p, const float *cos_t, const float *sin_t,
                         int table_bits, uint32_t seed, uint32_t epoch, const BfsDev &B, int count,
                         const int *count_dev, int node_base, int parity, int tag, int pub_stamp,
                         DeviceCounters *ctr, hipStream_t s, int which) {
  if (count - node_base <= 0) return;
  const int spec_slots = (count - node_base) * p.sample_num;
  if (which & 1) {
    // a level whose workgroups are all resident at once anyway takes 8-wave workgroups (twice the draws per round)
    constexpr int wide_max = 512;
    if (count - node_base <= wide_max && 8 <= SW)
      hipLaunchKernelGGL(k_level_sample<8>, dim3(count - node_base), dim3(8 * WAVE), 0, s, m, p, cos_t, sin_t,
                         table_bits, seed, epoch, B, count, count_dev, node_base, parity, tag, pub_stamp, ctr);
    else
      hipLaunchKernelGGL(k_level_sample<LSW>, dim3(count - node_base), dim3(LSW * WAVE), 0, s, m, p, cos_t, sin_t,
                         table_bits, seed, epoch, B, count, count_dev, node_base, parity, tag, pub_stamp, ctr);
  }
  if (which & 2)
    hipLaunchKernelGGL(k_level_spec, dim3((spec_slots + LQW - 1) / LQW), dim3(LQW * WAVE), 0, s, m, p, B, count,
                       count_dev, node_base, parity, ctr, tag);
  if ((which & 2) && B.resc)  // step 3: who could rescue the candidates whose parent edge just failed
    hipLaunchKernelGGL(k_level_spec3, dim3(spec_slots), dim3(WAVE), 0, s, m, p, B, count, count_dev, node_base, tag,
                       B.resc);
}

void launch_level_resolve_commit(const BfsDev &B, QueryParams p, int count, int new_state,
                                 long long call_base, int V0, int tag, int epoch, hipStream_t s,
                                 int stall_test, bool ticketed, unsigned *ticket_base) {
  if (count <= 0) return;
  const int slots = count * p.sample_num;
  // one 16-lane row per sample slot; a workgroup waits for lower-numbered slots / workgroups only
  const unsigned nR = (unsigned)((slots + RW - 1) / RW);
  const int max_spin = stall_test ? (1 << 10) : (1 << 16);
  const unsigned nC = (nR + CRW - 1) / CRW;  // commit workgroups: one thread per slot
  // sample_num > 32: a slot can have more blockers than its row holds at once (multi-pass variant)
  const bool multi = p.sample_num > 32;
  const dim3 grid(nR + nC), block(RWV * WAVE);
#define TRG_LAUNCH_RESOLVE(T, M, S3)                                                                          \
  hipLaunchKernelGGL((k_level_resolve<T, M, S3>), grid, block, 0, s, B, count, p.sample_num, p.expand_dist,   \
                     p.robot_size, tag, call_base, stall_test, max_spin, V0, new_state, epoch, (int)nR,       \
                     (int)nC, ticketed ? *ticket_base : 0u)
  const bool s3 = B.resc != nullptr;  // expandGraph's step 3 is on
  const int variant = (ticketed ? 4 : 0) | (multi ? 2 : 0) | (s3 ? 1 : 0);
  switch (variant) {
    case 0: TRG_LAUNCH_RESOLVE(false, false, false); break;
    case 1: TRG_LAUNCH_RESOLVE(false, false, true); break;
    case 2: TRG_LAUNCH_RESOLVE(false, true, false); break;
    case 3: TRG_LAUNCH_RESOLVE(false, true, true); break;
    case 4: TRG_LAUNCH_RESOLVE(true, false, false); break;
    case 5: TRG_LAUNCH_RESOLVE(true, false, true); break;
    case 6: TRG_LAUNCH_RESOLVE(true, true, false); break;
    default: TRG_LAUNCH_RESOLVE(true, true, true); break;
  }
#undef TRG_LAUNCH_RESOLVE
  if (ticketed) *ticket_base += nR + nC;
}

// the reference's node tree over the nodes [0, V) in creation order, then the step-3 calls of every valid
// node into the call log (trg_step3.inc).  scratch: 6 V + 8 ints.  h_left: pinned word for the round check.
TrgStatus_t launch_step3_calls(const BfsDev &B, int V, float range, int *scratch, int *h_left, hipStream_t s) {
  if (V <= 1) return 0;
  KdDev kd;
  kd.child = scratch;
  kd.claim = scratch + 2 * (size_t)V;
  kd.axis = scratch + 4 * (size_t)V;
  kd.cur = scratch + 5 * (size_t)V;
  kd.left = scratch + 6 * (size_t)V;
  const int nb = (V + 255) / 256;
  hipLaunchKernelGGL(k_kd_init, dim3(nb), dim3(256), 0, s, kd, V);
  for (int round = 0; round < V; ++round) {
    // a few rounds per look at the counter: every round places one more tree level
    for (int k = 0; k < 8; ++k) {
      hipLaunchKernelGGL(k_kd_walk, dim3(nb), dim3(256), 0, s, B, kd, V);
      hipLaunchKernelGGL(k_kd_place, dim3(nb), dim3(256), 0, s, B, kd, V);
    }
    if (hipMemcpyAsync(h_left, kd.left, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return 1;
    if (hipStreamSynchronize(s) != hipSuccess) return 1;
    if (*h_left == 0) break;
  }
  hipLaunchKernelGGL(k_step3_calls, dim3((V - 1 + 63) / 64), dim3(64), 0, s, B, kd, V, range);
  return 0;
}

void launch_bfs_stats(const BfsDev &B, int V, unsigned long long *out, hipStream_t s) {
  if (V <= 0) return;
  const int nb = std::min((V + 255) / 256, 512);
  hipLaunchKernelGGL(k_bfs_stats, dim3(nb), dim3(256), 0, s, B, V, out);
}

void launch_node_cov(const MapView &m, QueryParams p, const BfsDev &B, int v_lo, int v_hi, hipStream_t s) {
  v_lo = std::max(v_lo, 1);  // node 0 is the root
  if (v_hi <= v_lo) return;
  hipLaunchKernelGGL(k_node_cov, dim3((v_hi - v_lo + NCW - 1) / NCW), dim3(NCW * WAVE), 0, s, m, p, B, v_lo, v_hi);
}

void launch_node_weights(const BfsDev &B, int V, hipStream_t s) {
  if (V <= 1) return;
  hipLaunchKernelGGL(k_node_weights, dim3((V - 1 + 255) / 256), dim3(256), 0, s, B, V);
}

void launch_bfs_clear_tie(const BfsDev &B, hipStream_t s) {
  hipLaunchKernelGGL(k_bfs_clear_tie, dim3(1), dim3(64), 0, s, B);
}

void launch_bfs_undo_slots(const BfsDev &B, int slots, hipStream_t s) {
  if (slots <= 0) return;
  hipLaunchKernelGGL(k_bfs_undo_slots, dim3((slots + 255) / 256), dim3(256), 0, s, B, slots);
}

void launch_calls_eval(const MapView &m, QueryParams p, const BfsDev &B, const int *list, int count,
                       const int *count_dev, DeviceCounters *ctr, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_calls_gather, dim3((count + QW - 1) / QW), dim3(QW * WAVE), 0, s, m, p, B,
                     list, count, count_dev, ctr);
  hipLaunchKernelGGL(k_calls_finish, dim3((count + 255) / 256), dim3(256), 0, s, B, list, count,
                     count_dev, ctr);
}

void launch_first_insert(const FinDev &F, const BfsDev &B, long long c0, long long c1, int *sel_count,
                         hipStream_t s) {
  if (c1 <= c0) return;
  hipLaunchKernelGGL(k_first_insert, dim3((unsigned)((c1 - c0 + 255) / 256)), dim3(256), 0, s, F, B, c0, c1,
                     sel_count);
}

// round 1 of the calls [c0, c1): list = the first call of every pair, in any order; *count = how many
void launch_calls_select_append(const FinDev &F, const BfsDev &B, long long c0, long long c1, int *list,
                                int *count, unsigned long long *total, hipStream_t s) {
  if (c1 <= c0) return;
  hipLaunchKernelGGL(k_calls_select_append, dim3((unsigned)((c1 - c0 + 255) / 256)), dim3(256), 0, s, F, B, c0,
                     c1, list, count, total);
}

void launch_calls_select2_append(const FinDev &F, const BfsDev &B, long long ncalls, int *list, int *count,
                                 unsigned long long *total, hipStream_t s) {
  if (ncalls <= 0) return;
  hipLaunchKernelGGL(k_calls_select2_append, dim3((unsigned)((ncalls + 255) / 256)), dim3(256), 0, s, F, B,
                     ncalls, list, count, total);
}

void launch_fin_insert_count(const FinDev &F, const BfsDev &B, long long ncalls, hipStream_t s) {
  if (ncalls <= 0) return;
  const unsigned nb = (unsigned)((ncalls + 255) / 256);
  hipLaunchKernelGGL(k_fin_insert, dim3(nb), dim3(256), 0, s, F, B, ncalls);
  hipLaunchKernelGGL(k_fin_count<false>, dim3(nb), dim3(256), 0, s, F, B, ncalls);
}
// the same for a build without step 3: ok_seq for the pairs of the round-2 calls list[0..count) only (no
// table-wide clear of ok_seq is needed), and the count takes a pair's first call when that one succeeded
void launch_fin_insert_count_listed(const FinDev &F, const BfsDev &B, long long ncalls, const int *list, int count,
                                    hipStream_t s) {
  if (ncalls <= 0) return;
  if (count > 0) {
    const unsigned nl = (unsigned)((count + 255) / 256);
    hipLaunchKernelGGL(k_fin_insert_listed<true>, dim3(nl), dim3(256), 0, s, F, B, list, count);
    hipLaunchKernelGGL(k_fin_insert_listed<false>, dim3(nl), dim3(256), 0, s, F, B, list, count);
  }
  hipLaunchKernelGGL(k_fin_count<true>, dim3((unsigned)((ncalls + 255) / 256)), dim3(256), 0, s, F, B, ncalls);
}

void launch_fin_scatter(const FinDev &F, const BfsDev &B, long long ncalls, bool with_w, hipStream_t s) {
  if (ncalls <= 0) return;
  const unsigned nb = (unsigned)((ncalls + 255) / 256);
  if (with_w) hipLaunchKernelGGL(k_fin_scatter<true>, dim3(nb), dim3(256), 0, s, F, B, ncalls);
  else hipLaunchKernelGGL(k_fin_scatter<false>, dim3(nb), dim3(256), 0, s, F, B, ncalls);
}
void launch_map_order_fill(const MapOrderRuns &R, int V, int *map_order, hipStream_t s) {
  if (V > 0) hipLaunchKernelGGL(k_map_order_fill, dim3((V + 255) / 256), dim3(256), 0, s, R, V, map_order);
}
void launch_fin_rowsort(const FinDev &F, int V, hipStream_t s) {
  if (V > 0) hipLaunchKernelGGL(k_fin_rowsort, dim3((V + 255) / 256), dim3(256), 0, s, F, V);
}

// cleanGraph on the device: keep flags in container order -> new ids -> compacted, remapped, ordered
// rows.  keep_pos[V] (= rowptr of the flags) is the number of surviving nodes, rowptr_new[V] the edge
// count; the host reads both afterwards.  w == nullptr: everything but the weights, which
// launch_fin_clean_weights writes later.
// the renumbering alone: it reads the rows' lengths (F.rowptr), not their entries, so it can run before
// k_fin_scatter has filled them
void launch_fin_renumber(const FinDev &F, const BfsDev &B, const int *map_order, int V, int *keep_flag,
                         int *keep_pos, int *new2old, int *old2new, int *deg_new, int *rowptr_new,
                         int *scan_tmp, hipStream_t s) {
  if (V <= 0) return;
  const int nb = (V + 255) / 256;
  hipLaunchKernelGGL(k_fin_keep_flag, dim3(nb), dim3(256), 0, s, F, B, map_order, V, keep_flag);
  launch_exclusive_scan(keep_flag, keep_pos, V, scan_tmp, s);
  hipLaunchKernelGGL(k_fin_renumber, dim3(nb), dim3(256), 0, s, map_order, (const int *)keep_flag,
                     (const int *)keep_pos, V, new2old, old2new);
  const int *vn = keep_pos + V;
  hipLaunchKernelGGL(k_fin_clean_deg, dim3(nb), dim3(256), 0, s, F, (const int *)new2old, vn, V, deg_new);
  launch_exclusive_scan(deg_new, rowptr_new, V, scan_tmp, s);
}
// xyz and state of the cleaned graph (after launch_fin_renumber)
void launch_fin_clean_nodes(const FinDev &F, const BfsDev &B, int V, const int *keep_pos, const int *new2old,
                            float *xyz, int *state, hipStream_t s) {
  if (V <= 0) return;
  hipLaunchKernelGGL(k_fin_clean_copy<FIN_NODES>, dim3((V + 255) / 256), dim3(256), 0, s, F, B, new2old,
                     (const int *)nullptr, keep_pos + V, (const int *)nullptr, (int *)nullptr, (float *)nullptr,
                     (float *)nullptr, xyz, state);
}
// col and dist of the cleaned graph (after launch_fin_renumber and launch_fin_scatter)
void launch_fin_clean_edges(const FinDev &F, const BfsDev &B, int V, const int *keep_pos, const int *new2old,
                            const int *old2new, const int *rowptr_new, int *col, float *dist, hipStream_t s) {
  if (V <= 0) return;
  hipLaunchKernelGGL(k_fin_clean_copy<FIN_EDGES>, dim3((unsigned)(((long long)V * FIN_ROW + 255) / 256)), dim3(256),
                     0, s, F, B, new2old, old2new, keep_pos + V, rowptr_new, col, (float *)nullptr, dist,
                     (float *)nullptr, (int *)nullptr);
}

void launch_fin_clean(const FinDev &F, const BfsDev &B, const int *map_order, int V, int *keep_flag,
                      int *keep_pos, int *new2old, int *old2new, int *deg_new, int *rowptr_new,
                      int *scan_tmp, int *col, float *w, float *dist, float *xyz, int *state,
                      hipStream_t s) {
  if (V <= 0) return;
  launch_fin_renumber(F, B, map_order, V, keep_flag, keep_pos, new2old, old2new, deg_new, rowptr_new, scan_tmp, s);
  const int *vn = keep_pos + V;
  const dim3 grid((unsigned)(((long long)V * FIN_ROW + 255) / 256));
  if (w)
    hipLaunchKernelGGL(k_fin_clean_copy<FIN_ALL>, grid, dim3(256), 0, s, F, B, (const int *)new2old,
                       (const int *)old2new, vn, (const int *)rowptr_new, col, w, dist, xyz, state);
  else
    hipLaunchKernelGGL(k_fin_clean_copy<FIN_STRUCTURE>, grid, dim3(256), 0, s, F, B, (const int *)new2old,
                       (const int *)old2new, vn, (const int *)rowptr_new, col, w, dist, xyz, state);
}

void launch_fin_clean_weights(const FinDev &F, const BfsDev &B, int V, const int *keep_pos, const int *new2old,
                              const int *rowptr_new, float *w, hipStream_t s) {
  if (V <= 0) return;
  hipLaunchKernelGGL(k_fin_clean_copy<FIN_WEIGHTS>, dim3((unsigned)(((long long)V * FIN_ROW + 255) / 256)), dim3(256),
                     0, s, F, B, new2old, (const int *)nullptr, keep_pos + V, rowptr_new, (int *)nullptr, w,
                     (float *)nullptr, (float *)nullptr, (int *)nullptr);
}
