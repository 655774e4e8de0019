// trg_engine_stitch.inc -- host side of the tile-boundary stitch (included by trg_engine.cpp): the
// three C-ABI steps of DESIGN.md section 7 over the kernels of trg_stitch.inc.  The two exchanges
// between the steps are the caller's (all-gather-v of device buffers over RCCL).

namespace {

// the cleaned global graph of this engine on the device: still resident after a device build, else
// uploaded from the host copy
struct DevGraph {
  const float *xyz = nullptr;
  const int *rowptr = nullptr, *col = nullptr;
  const float *w = nullptr, *dist = nullptr;
  int V = 0, E = 0;
};

TrgStatus stitch_dev_graph(TrgEngine *e, bool need_edges, DevGraph *g) {
  StitchBufs &sb = *e->stitch;
  Csr &c = e->csr_global;
  (void)ensure_csr_global(e);  // (false: neither the CSR nor the pool is current, the old rows stay in place)
  g->V = (int)c.state.size();
  g->E = (int)c.col.size();
  if (const BfsBuffers *bb = dev_csr(e)) {
    g->xyz = (const float *)bb->xyz2.p;
    g->rowptr = (const int *)bb->rowptr_new.p;
    g->col = (const int *)bb->col2.p;
    g->w = (const float *)bb->w2.p;
    g->dist = (const float *)bb->dist2.p;
    return TRG_OK;
  }
  TrgStatus st;
  hipStream_t s = e->s_main;
  if ((st = ensure_bytes(e, sb.up_xyz, (size_t)g->V * 12 + 16)) != TRG_OK) return st;
  if (g->V) HIPCHK(e, hipMemcpyAsync(sb.up_xyz.p, c.xyz.data(), (size_t)g->V * 12, hipMemcpyHostToDevice, s));
  g->xyz = (const float *)sb.up_xyz.p;
  if (need_edges) {
    if ((st = ensure_bytes(e, sb.up_rowptr, ((size_t)g->V + 1) * 4)) != TRG_OK) return st;
    if ((st = ensure_bytes(e, sb.up_col, (size_t)g->E * 4 + 16)) != TRG_OK) return st;
    if ((st = ensure_bytes(e, sb.up_w, (size_t)g->E * 4 + 16)) != TRG_OK) return st;
    if ((st = ensure_bytes(e, sb.up_dist, (size_t)g->E * 4 + 16)) != TRG_OK) return st;
    std::vector<int> rp(1, 0);
    const int *rowptr_h = c.rowptr.empty() ? rp.data() : c.rowptr.data();
    HIPCHK(e, hipMemcpyAsync(sb.up_rowptr.p, rowptr_h, ((size_t)g->V + 1) * 4, hipMemcpyHostToDevice, s));
    if (g->E) {
      HIPCHK(e, hipMemcpyAsync(sb.up_col.p, c.col.data(), (size_t)g->E * 4, hipMemcpyHostToDevice, s));
      HIPCHK(e, hipMemcpyAsync(sb.up_w.p, c.w.data(), (size_t)g->E * 4, hipMemcpyHostToDevice, s));
      HIPCHK(e, hipMemcpyAsync(sb.up_dist.p, c.dist.data(), (size_t)g->E * 4, hipMemcpyHostToDevice, s));
    }
    HIPCHK(e, hipStreamSynchronize(s));  // (rp is a stack object)
    g->rowptr = (const int *)sb.up_rowptr.p;
    g->col = (const int *)sb.up_col.p;
    g->w = (const float *)sb.up_w.p;
    g->dist = (const float *)sb.up_dist.p;
  }
  return TRG_OK;
}

// the stitched rows from HBM into the host CSR (lazily, on the first export after an assemble)
TrgStatus stitch_fetch(TrgEngine *e) {
  if (!e->current(TrgEngine::VIEW_STITCH_DEV)) return TRG_OK;
  StitchBufs &sb = *e->stitch;
  Csr &out = e->csr_stitched;
  hipStream_t s = e->s_main;
  const size_t V = out.state.size();
  const int En = e->stitched_edges;
  out.rowptr.resize(V + 1);
  out.col.resize(En);
  out.w.resize(En);
  out.dist.resize(En);
  HIPCHK(e, hipMemcpyAsync(out.rowptr.data(), sb.rowptr_new.p, (V + 1) * 4, hipMemcpyDeviceToHost, s));
  if (En) {
    HIPCHK(e, hipMemcpyAsync(out.col.data(), sb.col_new.p, (size_t)En * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(out.w.data(), sb.w_new.p, (size_t)En * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(out.dist.data(), sb.dist_new.p, (size_t)En * 4, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(e, hipStreamSynchronize(s));
  e->view_stamp[TrgEngine::VIEW_STITCH_DEV] = 0;
  return TRG_OK;
}

TrgStatus stitch_boundary(TrgEngine *e, const float core_xyxy[4], int32_t cols, int32_t rows, int32_t tile,
                          TrgBoundaryRec *d_rec, int32_t cap, int32_t *n_out) {
  if (!core_xyxy || !n_out || cols < 1 || rows < 1 || tile < 0 || tile >= cols * rows || cap < 0)
    return e->fail(TRG_ERR_INVALID_ARG, "stitch_boundary: bad arguments");
  StitchBufs &sb = *e->stitch;
  DevGraph g;
  TrgStatus st = stitch_dev_graph(e, false, &g);
  if (st != TRG_OK) return st;
  *n_out = 0;
  if (g.V == 0) return TRG_OK;
  const int c = tile % cols, r = tile / cols;
  const int sides = (c > 0 ? 1 : 0) | (c < cols - 1 ? 2 : 0) | (r > 0 ? 4 : 0) | (r < rows - 1 ? 8 : 0);
  if ((st = ensure_bytes(e, sb.flag, ((size_t)g.V + 1) * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.off, ((size_t)g.V + 2) * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.scan_tmp, ((size_t)g.V / 2048 + 16) * 4)) != TRG_OK) return st;
  hipStream_t s = e->s_main;
  launch_stitch_boundary(g.xyz, g.V, core_xyxy, sides, e->prm.expand_dist, (int *)sb.flag.p, (int *)sb.off.p,
                         (int *)sb.scan_tmp.p, (StitchRec *)d_rec, d_rec ? cap : 0, s);
  int n = 0;
  HIPCHK(e, hipMemcpyAsync(&n, (int *)sb.off.p + g.V, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  *n_out = n;
  if (d_rec && n > cap) return e->fail(TRG_ERR_CAPACITY, "stitch_boundary: record buffer too small");
  return TRG_OK;
}

TrgStatus stitch_cross(TrgEngine *e, int32_t tile, int32_t ntiles, const TrgBoundaryRec *d_all_rec,
                       const int32_t *rec_offsets, TrgCrossEdge *d_edges, int32_t cap, int32_t *n_out) {
  if (!rec_offsets || !n_out || ntiles < 1 || ntiles > STITCH_MAX_TILES || tile < 0 || tile >= ntiles)
    return e->fail(TRG_ERR_INVALID_ARG, "stitch_cross: bad arguments");
  if (!e->gmap.valid) return e->fail(TRG_ERR_NO_MAP, "stitch_cross: no map");
  *n_out = 0;
  StitchBufs &sb = *e->stitch;
  hipStream_t s = e->s_main;
  const int na = rec_offsets[tile + 1] - rec_offsets[tile];
  const int U = ntiles - tile - 1;
  if (na <= 0 || U <= 0 || rec_offsets[ntiles] - rec_offsets[tile + 1] <= 0) return TRG_OK;
  const StitchRec *all = (const StitchRec *)d_all_rec;
  TrgStatus st;
  const size_t cells = (size_t)U * na;
  if ((st = ensure_bytes(e, sb.cnt, (cells + 1) * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.off, (cells + 2) * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.scan_tmp, (cells / 2048 + 16) * 4)) != TRG_OK) return st;
  launch_stitch_pairs(all, rec_offsets, tile, ntiles, e->prm.expand_dist, 0, (int *)sb.cnt.p, nullptr, nullptr,
                      nullptr, s);
  launch_exclusive_scan((const int *)sb.cnt.p, (int *)sb.off.p, (int)cells, (int *)sb.scan_tmp.p, s);
  int npairs = 0;
  HIPCHK(e, hipMemcpyAsync(&npairs, (int *)sb.off.p + cells, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  if (npairs <= 0) return TRG_OK;
  const size_t np_ = (size_t)npairs;
  if ((st = ensure_bytes(e, sb.pair_a, np_ * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.pair_b, np_ * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.p1, np_ * 12)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.p2, np_ * 12)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.mid, edge_mid_floats(np_) * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.status, np_ * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.npts, np_ * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.weight, np_ * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.dist, np_ * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.flag, (np_ + 1) * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.n_unc, 16)) != TRG_OK) return st;
  launch_stitch_pairs(all, rec_offsets, tile, ntiles, e->prm.expand_dist, 1, nullptr, (const int *)sb.off.p,
                      (int *)sb.pair_a.p, (int *)sb.pair_b.p, s);
  launch_stitch_pair_points(all, (const int *)sb.pair_a.p, (const int *)sb.pair_b.p, npairs, (float *)sb.p1.p,
                            (float *)sb.p2.p, s);
  // wireEdge's position-only part for (a, b) on this tile's map (trg.cpp:269-363)
  launch_edges(e->gmap.view, qparams(e), (const float *)sb.p1.p, (const float *)sb.p2.p, npairs,
               (float *)sb.mid.p, (int *)sb.status.p, (int *)sb.npts.p, (float *)sb.weight.p,
               (float *)sb.dist.p, e->d_ctr, s);
  e->stats.edge_evals_gpu += (uint64_t)npairs;
  // pair offsets are no longer needed: off is reused for the scan of the success flags
  if ((st = ensure_bytes(e, sb.off, (np_ + 2) * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.scan_tmp, (np_ / 2048 + 16) * 4)) != TRG_OK) return st;
  for (int attempt = 0; attempt < 2; ++attempt) {
    HIPCHK(e, hipMemsetAsync(sb.n_unc.p, 0, 4, s));
    launch_stitch_edge_select(all, rec_offsets, tile, ntiles, (const int *)sb.pair_a.p, (const int *)sb.pair_b.p,
                              (const int *)sb.status.p, (const float *)sb.weight.p, (const float *)sb.dist.p,
                              npairs, (int *)sb.flag.p, (int *)sb.off.p, (int *)sb.scan_tmp.p, (int *)sb.n_unc.p,
                              (StitchEdge *)d_edges, d_edges ? cap : 0, s);
    int tail[2] = {0, 0};
    HIPCHK(e, hipMemcpyAsync(&tail[0], (int *)sb.off.p + npairs, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(&tail[1], sb.n_unc.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    if (tail[1] == 0 || attempt == 1) {
      *n_out = tail[0];
      break;
    }
    // slope gates the device could not call: the reference's own libm decides (trg.cpp:269-274)
    ++e->stats.stitch_gate_retries;
    std::vector<int> hs(np_);
    std::vector<float> hd(np_), h1(3 * np_), h2(3 * np_);
    HIPCHK(e, hipMemcpy(hs.data(), sb.status.p, np_ * 4, hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(hd.data(), sb.dist.p, np_ * 4, hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(h1.data(), sb.p1.p, np_ * 12, hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(h2.data(), sb.p2.p, np_ * 12, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < np_; ++k)
      if (hs[k] & EDGE_GATE_UNCERTAIN) hs[k] = resolve_status(e, hs[k], h1[3 * k + 2], h2[3 * k + 2], hd[k]);
    HIPCHK(e, hipMemcpy(sb.status.p, hs.data(), np_ * 4, hipMemcpyHostToDevice));
  }
  if (d_edges && *n_out > cap) return e->fail(TRG_ERR_CAPACITY, "stitch_cross: edge buffer too small");
  return TRG_OK;
}

TrgStatus stitch_assemble(TrgEngine *e, int32_t tile, int32_t ntiles, const int32_t *node_offsets,
                          const TrgCrossEdge *d_all_edges, int32_t n_edges) {
  if (!node_offsets || ntiles < 1 || ntiles > STITCH_MAX_TILES || tile < 0 || tile >= ntiles || n_edges < 0)
    return e->fail(TRG_ERR_INVALID_ARG, "stitch_assemble: bad arguments");
  StitchBufs &sb = *e->stitch;
  hipStream_t s = e->s_main;
  DevGraph g;
  TrgStatus st = stitch_dev_graph(e, true, &g);
  if (st != TRG_OK) return st;
  if (node_offsets[tile + 1] - node_offsets[tile] != g.V)
    return e->fail(TRG_ERR_INVALID_ARG, "stitch_assemble: node_offsets do not match this tile's graph");
  Csr &out = e->csr_stitched;
  out.clear();
  e->view_stamp[TrgEngine::VIEW_STITCH_DEV] = 0;
  e->stitched_edges = 0;
  const Csr &c = e->csr_global;
  out.xyz = c.xyz;
  out.state = c.state;
  out.cid.resize(g.V);
  for (int i = 0; i < g.V; ++i) out.cid[i] = node_offsets[tile] + i;  // global id of the row
  out.rowptr.assign(1, 0);
  if (g.V == 0) return TRG_OK;
  const size_t V = (size_t)g.V;
  if ((st = ensure_bytes(e, sb.extra, (V + 1) * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.fill, (V + 1) * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.deg, (V + 1) * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.rowptr_new, (V + 2) * 4)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.scan_tmp, (V / 2048 + 16) * 4)) != TRG_OK) return st;
  HIPCHK(e, hipMemsetAsync(sb.extra.p, 0, (V + 1) * 4, s));
  HIPCHK(e, hipMemsetAsync(sb.fill.p, 0, (V + 1) * 4, s));
  const StitchEdge *edges = (const StitchEdge *)d_all_edges;
  launch_stitch_assemble(edges, n_edges, tile, ntiles, node_offsets, g.rowptr, g.col, g.w, g.dist, g.V,
                         (int *)sb.extra.p, (int *)sb.deg.p, (int *)sb.rowptr_new.p, (int *)sb.scan_tmp.p,
                         (int *)sb.fill.p, nullptr, nullptr, nullptr, 0, s);
  int En = 0, n_bad = 0;
  HIPCHK(e, hipMemcpyAsync(&En, (int *)sb.rowptr_new.p + g.V, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipMemcpyAsync(&n_bad, (int *)sb.extra.p + g.V, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  if (n_bad) {
    out.clear();  // (no rows at all: a view of V nodes without their V + 1 row pointers must not be exported)
    return e->fail(TRG_ERR_INVALID_ARG, "stitch_assemble: " + std::to_string(n_bad) +
                                            " cross edges name a tile or a node outside node_offsets");
  }
  if ((st = ensure_bytes(e, sb.col_new, (size_t)En * 4 + 16)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.w_new, (size_t)En * 4 + 16)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, sb.dist_new, (size_t)En * 4 + 16)) != TRG_OK) return st;
  launch_stitch_assemble(edges, n_edges, tile, ntiles, node_offsets, g.rowptr, g.col, g.w, g.dist, g.V,
                         (int *)sb.extra.p, (int *)sb.deg.p, (int *)sb.rowptr_new.p, (int *)sb.scan_tmp.p,
                         (int *)sb.fill.p, (int *)sb.col_new.p, (float *)sb.w_new.p, (float *)sb.dist_new.p, 1, s);
  // the rows stay in HBM; an export of TRG_KIND_STITCHED fetches them when asked
  e->stitched_edges = En;
  e->view_stamp[TrgEngine::VIEW_STITCH_DEV] = e->graph_version;
  HIPCHK(e, hipGetLastError());
  return TRG_OK;
}

TrgStatus graph_sizes(TrgEngine *e, TrgKind kind, int32_t *num_nodes, int32_t *num_edges) {
  if (kind == TRG_KIND_STITCHED) {  // (without fetching rows that are still in HBM)
    *num_nodes = (int32_t)e->csr_stitched.state.size();
    *num_edges = e->stitched_edges;
    return TRG_OK;
  }
  TrgCsrView v;
  const TrgStatus st = export_csr(e, kind, &v);
  if (st != TRG_OK) return st;
  *num_nodes = v.num_nodes;
  *num_edges = v.num_edges;
  return TRG_OK;
}

}  // namespace

extern "C" {

TrgStatus trg_engine_stitch_boundary(TrgEngine *e, const float core_xyxy[4], int32_t cols, int32_t rows,
                                     int32_t tile, TrgBoundaryRec *d_rec, int32_t cap, int32_t *n_out) {
  return entry(e, "stitch_boundary", DEVICE,
               [&] { return stitch_boundary(e, core_xyxy, cols, rows, tile, d_rec, cap, n_out); });
}

TrgStatus trg_engine_stitch_cross(TrgEngine *e, int32_t tile, int32_t ntiles, const TrgBoundaryRec *d_all_rec,
                                  const int32_t *rec_offsets, TrgCrossEdge *d_edges, int32_t cap, int32_t *n_out) {
  return entry(e, "stitch_cross", DEVICE,
               [&] { return stitch_cross(e, tile, ntiles, d_all_rec, rec_offsets, d_edges, cap, n_out); });
}

TrgStatus trg_engine_stitch_assemble(TrgEngine *e, int32_t tile, int32_t ntiles, const int32_t *node_offsets,
                                     const TrgCrossEdge *d_all_edges, int32_t n_edges) {
  return entry(e, "stitch_assemble", DEVICE,
               [&] { return stitch_assemble(e, tile, ntiles, node_offsets, d_all_edges, n_edges); });
}

TrgStatus trg_engine_graph_sizes(TrgEngine *e, TrgKind kind, int32_t *num_nodes, int32_t *num_edges) {
  if (!num_nodes || !num_edges) return TRG_ERR_INVALID_ARG;
  return entry(e, "graph_sizes", ENGINE, [&] { return graph_sizes(e, kind, num_nodes, num_edges); });
}

}  // extern "C"
