// trg_engine_stitch.inc -- host side of the tile-boundary stitch (included by trg_engine.cpp): the
// three C-ABI steps of DESIGN.md section 7 over the kernels of trg_stitch.inc.  The two exchanges
// between the steps are the caller's (all-gather-v of device buffers over RCCL).

namespace {

// scratch of the three steps, and the stitched rows until an export fetches them; made on first use
struct StitchBufs {
  DevArr flag, off, cnt, pair_a, pair_b, p1, p2, mid, status, npts, weight, dist, n_unc;
  DevArr extra, deg, rowptr_new, fill, col_new, w_new, dist_new;
  DevArr scan_tmp;
};

StitchBufs &stitch_bufs(TrgEngine *e) {
  if (!e->stitch) e->stitch.reset(new StitchBufs());
  return *e->stitch;
}

// the stitched rows from HBM into the host CSR (lazily, on the first export after an assemble)
TrgStatus stitch_fetch(TrgEngine *e) {
  if (!e->current(TrgEngine::VIEW_STITCH_DEV)) return TRG_OK;
  StitchBufs &sb = *e->stitch;  // (stitch_assemble made it)
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
  StitchBufs &sb = stitch_bufs(e);
  DevGraph g;
  TrgStatus st = ensure_dev_graph(e, DEV_NODES, &g);
  if (st != TRG_OK) return st;
  *n_out = 0;
  if (g.V == 0) return TRG_OK;
  const int c = tile % cols, r = tile / cols;
  const int sides = (c > 0 ? 1 : 0) | (c < cols - 1 ? 2 : 0) | (r > 0 ? 4 : 0) | (r < rows - 1 ? 8 : 0);
  const size_t V = (size_t)g.V;
  if ((st = ensure_all(e, {{&sb.flag, (V + 1) * 4}, {&sb.off, (V + 2) * 4}, {&sb.scan_tmp, (V / 2048 + 16) * 4}})) != TRG_OK)
    return st;
  hipStream_t s = e->s_main;
  launch_stitch_boundary(g.xyz, g.V, core_xyxy, sides, e->prm.expand_dist, sb.flag.as<int>(), sb.off.as<int>(),
                         sb.scan_tmp.as<int>(), (StitchRec *)d_rec, d_rec ? cap : 0, s);
  int n = 0;
  HIPCHK(e, hipMemcpyAsync(&n, sb.off.as<int>() + g.V, sizeof(int), hipMemcpyDeviceToHost, s));
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
  StitchBufs &sb = stitch_bufs(e);
  hipStream_t s = e->s_main;
  const int na = rec_offsets[tile + 1] - rec_offsets[tile];
  const int U = ntiles - tile - 1;
  if (na <= 0 || U <= 0 || rec_offsets[ntiles] - rec_offsets[tile + 1] <= 0) return TRG_OK;
  const StitchRec *all = (const StitchRec *)d_all_rec;
  TrgStatus st;
  const size_t cells = (size_t)U * na;
  if ((st = ensure_all(e, {{&sb.cnt, (cells + 1) * 4}, {&sb.off, (cells + 2) * 4},
                           {&sb.scan_tmp, (cells / 2048 + 16) * 4}})) != TRG_OK)
    return st;
  launch_stitch_pairs(all, rec_offsets, tile, ntiles, e->prm.expand_dist, 0, sb.cnt.as<int>(), nullptr, nullptr, nullptr, s);
  launch_exclusive_scan(sb.cnt.as<int>(), sb.off.as<int>(), (int)cells, sb.scan_tmp.as<int>(), s);
  int npairs = 0;
  HIPCHK(e, hipMemcpyAsync(&npairs, sb.off.as<int>() + cells, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  if (npairs <= 0) return TRG_OK;
  const size_t np_ = (size_t)npairs;
  if ((st = ensure_all(e, {{&sb.pair_a, np_ * 4}, {&sb.pair_b, np_ * 4}, {&sb.p1, np_ * 12}, {&sb.p2, np_ * 12},
                           {&sb.mid, edge_mid_floats(np_) * 4}, {&sb.status, np_ * 4}, {&sb.npts, np_ * 4},
                           {&sb.weight, np_ * 4}, {&sb.dist, np_ * 4}, {&sb.flag, (np_ + 1) * 4}, {&sb.n_unc, 16}})) !=
      TRG_OK)
    return st;
  int *pair_a = sb.pair_a.as<int>(), *pair_b = sb.pair_b.as<int>(), *status = sb.status.as<int>();
  float *p1 = sb.p1.as<float>(), *p2 = sb.p2.as<float>(), *weight = sb.weight.as<float>(), *dist = sb.dist.as<float>();
  launch_stitch_pairs(all, rec_offsets, tile, ntiles, e->prm.expand_dist, 1, nullptr, sb.off.as<int>(), pair_a, pair_b, s);
  launch_stitch_pair_points(all, pair_a, pair_b, npairs, p1, p2, s);
  // wireEdge's position-only part for (a, b) on this tile's map (trg.cpp:269-363)
  launch_edges(e->gmap.view, qparams(e), p1, p2, npairs, sb.mid.as<float>(), status, sb.npts.as<int>(), weight, dist,
               e->d_ctr, s);
  e->stats.edge_evals_gpu += (uint64_t)npairs;
  // pair offsets are no longer needed: off is reused for the scan of the success flags
  if ((st = ensure_all(e, {{&sb.off, (np_ + 2) * 4}, {&sb.scan_tmp, (np_ / 2048 + 16) * 4}})) != TRG_OK) return st;
  for (int attempt = 0; attempt < 2; ++attempt) {
    HIPCHK(e, hipMemsetAsync(sb.n_unc.p, 0, 4, s));
    launch_stitch_edge_select(all, rec_offsets, tile, ntiles, pair_a, pair_b, status, weight, dist, npairs,
                              sb.flag.as<int>(), sb.off.as<int>(), sb.scan_tmp.as<int>(), sb.n_unc.as<int>(),
                              (StitchEdge *)d_edges, d_edges ? cap : 0, s);
    int tail[2] = {0, 0};
    HIPCHK(e, hipMemcpyAsync(&tail[0], sb.off.as<int>() + npairs, sizeof(int), hipMemcpyDeviceToHost, s));
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
  StitchBufs &sb = stitch_bufs(e);
  hipStream_t s = e->s_main;
  DevGraph g;
  TrgStatus st = ensure_dev_graph(e, DEV_EDGES, &g);
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
  const auto stitched = [&] {  // this tile has rows of the global graph, with these offsets
    e->stitch_node_off.assign(node_offsets, node_offsets + ntiles + 1);
    e->stitch_tile = tile;
    ++e->stitch_serial;
  };
  if (g.V == 0) {
    stitched();
    return TRG_OK;
  }
  const size_t V = (size_t)g.V;
  if ((st = ensure_all(e, {{&sb.extra, (V + 1) * 4}, {&sb.fill, (V + 1) * 4}, {&sb.deg, (V + 1) * 4},
                           {&sb.rowptr_new, (V + 2) * 4}, {&sb.scan_tmp, (V / 2048 + 16) * 4}})) != TRG_OK)
    return st;
  HIPCHK(e, hipMemsetAsync(sb.extra.p, 0, (V + 1) * 4, s));
  HIPCHK(e, hipMemsetAsync(sb.fill.p, 0, (V + 1) * 4, s));
  const StitchEdge *edges = (const StitchEdge *)d_all_edges;
  // pass 0 counts the rows, pass 1 (with the edge arrays) fills them
  const auto pass = [&](int fill) {
    launch_stitch_assemble(edges, n_edges, tile, ntiles, node_offsets, g.rowptr, g.col, g.w, g.dist, g.V,
                           sb.extra.as<int>(), sb.deg.as<int>(), sb.rowptr_new.as<int>(), sb.scan_tmp.as<int>(),
                           sb.fill.as<int>(), fill ? sb.col_new.as<int>() : nullptr,
                           fill ? sb.w_new.as<float>() : nullptr, fill ? sb.dist_new.as<float>() : nullptr, fill, s);
  };
  pass(0);
  int En = 0, n_bad = 0;
  HIPCHK(e, hipMemcpyAsync(&En, sb.rowptr_new.as<int>() + g.V, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipMemcpyAsync(&n_bad, sb.extra.as<int>() + g.V, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  if (n_bad) {
    out.clear();  // (no rows at all: a view of V nodes without their V + 1 row pointers must not be exported)
    return e->fail(TRG_ERR_INVALID_ARG, "stitch_assemble: " + std::to_string(n_bad) +
                                            " cross edges name a tile or a node outside node_offsets");
  }
  const size_t eb = (size_t)En * 4 + 16;
  if ((st = ensure_all(e, {{&sb.col_new, eb}, {&sb.w_new, eb}, {&sb.dist_new, eb}})) != TRG_OK) return st;
  pass(1);
  // the rows stay in HBM; an export of TRG_KIND_STITCHED fetches them when asked
  e->stitched_edges = En;
  e->view_stamp[TrgEngine::VIEW_STITCH_DEV] = e->graph_version;
  HIPCHK(e, hipGetLastError());
  stitched();
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
