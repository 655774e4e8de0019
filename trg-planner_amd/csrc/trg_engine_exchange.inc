// trg_engine_exchange.inc -- the tile-boundary stitch with its two exchanges done natively over RCCL
// (included by trg_engine.cpp).  One call runs DESIGN.md section 7 for this rank's tile: boundary records
// -> all-gather-v -> cross edges -> all-gather-v -> this tile's rows of the global graph.  RCCL has no
// all-gather-v: each exchange is an all-gather of one count per rank (the only host round trip), then an
// all-gather of payloads padded to the largest count, compacted on the device.  xGMI is point-to-point
// and these payloads are a few 10 KB, so latency decides: two small collectives per exchange, nothing
// bucketed.  A C / C++ consumer (the ROS nodes inherit TRGPlanner) needs no Python for N > 1;
// trg_planner/tiled.py::stitch_device calls the same entry point through ctypes.
//
// librccl is resolved at run time (dlopen): the engine has no link-time dependency on it, and a process
// that already loaded an RCCL (torch's) shares that instance when the soname matches.
//
// The all-gathers go through a Transport.  RCCL is the one a product uses.  The in-process transport
// (trg_engine_comm_join_local, never chosen unless asked for) lets R engines on one device in one process,
// each entered from its own thread, run the exchange's own logic -- counts, padded slots, the tail row,
// compaction, buffer reuse, the failure announcement -- where RCCL refuses two ranks on one device.

#include <dlfcn.h>
#include <rccl/rccl.h>

#include "local_group.h"

namespace {

struct RcclApi {
  void *lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclCommCount) CommCount = nullptr;
  decltype(&ncclCommUserRank) CommUserRank = nullptr;
  std::string err;
  bool load() {
    if (lib) return true;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib) break;
    }
    if (!lib) {
      err = std::string("dlopen librccl: ") + dlerror();
      return false;
    }
#define RCCL_SYM(field, sym)                         \
  field = (decltype(field))dlsym(lib, sym);          \
  if (!field) {                                      \
    err = std::string("librccl lacks ") + sym;       \
    lib = nullptr;                                   \
    return false;                                    \
  }
    RCCL_SYM(GetUniqueId, "ncclGetUniqueId")
    RCCL_SYM(CommInitRank, "ncclCommInitRank")
    RCCL_SYM(CommDestroy, "ncclCommDestroy")
    RCCL_SYM(AllGather, "ncclAllGather")
    RCCL_SYM(GetErrorString, "ncclGetErrorString")
    RCCL_SYM(CommCount, "ncclCommCount")
    RCCL_SYM(CommUserRank, "ncclCommUserRank")
#undef RCCL_SYM
    return true;
  }
};
RcclApi g_rccl;

#define RCCLCHK(e, call)                                                                            \
  do {                                                                                              \
    const ncclResult_t r_ = (call);                                                                 \
    if (r_ != ncclSuccess) return (e)->fail(TRG_ERR_DEVICE, std::string(#call ": ") + g_rccl.GetErrorString(r_)); \
  } while (0)

// what carries the exchange's two all-gathers: every rank gives `count` elements of `elem_bytes` (8: the
// counts, 1: the padded payload) and receives the ranks' blocks in rank order
struct Transport {
  virtual ~Transport() = default;
  virtual TrgStatus all_gather(TrgEngine *e, const void *d_send, void *d_recv, size_t count, size_t elem_bytes,
                               hipStream_t s) = 0;
};

struct RcclTransport : Transport {
  ncclComm_t comm = nullptr;
  bool owned = false;  // created by trg_engine_comm_init (destroyed with the engine)
  ~RcclTransport() override {
    if (comm && owned && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(comm);
  }
  TrgStatus all_gather(TrgEngine *e, const void *d_send, void *d_recv, size_t count, size_t elem_bytes,
                       hipStream_t s) override {
    RCCLCHK(e, g_rccl.AllGather(d_send, d_recv, count, elem_bytes == 8 ? ncclInt64 : ncclChar, comm, s));
    return TRG_OK;
  }
};

// The in-process transport: the group's host side (barriers bounded by the engine's comm_wait_seconds, the send
// pointers) is local_group.h; the all-gather is device-to-device copies on the own stream between two barriers.
// Nothing waits on the device.
struct LocalTransport : Transport {
  std::shared_ptr<LocalGroup> group;
  int rank = 0;
  const double *wait_seconds = nullptr;  // the engine's option, read at every wait
  ~LocalTransport() override {
    if (group) group->leave(rank);
  }
  TrgStatus barrier(TrgEngine *e) {
    const std::string why = group->barrier(rank, *wait_seconds);
    return why.empty() ? TRG_OK : e->fail(TRG_ERR_DEVICE, "local exchange: " + why);
  }
  TrgStatus all_gather(TrgEngine *e, const void *d_send, void *d_recv, size_t count, size_t elem_bytes,
                       hipStream_t s) override {
    const size_t bytes = count * elem_bytes;
    HIPCHK(e, hipStreamSynchronize(s));  // what the peers will read is written
    group->show(rank, d_send);
    TrgStatus st = barrier(e);
    if (st != TRG_OK) return st;
    const std::vector<const void *> from = group->shown();
    hipError_t he = hipSuccess;
    for (int k = 0; k < group->nranks() && he == hipSuccess; ++k)
      he = hipMemcpyAsync((char *)d_recv + (size_t)k * bytes, from[k], bytes, hipMemcpyDeviceToDevice, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    st = barrier(e);  // (entered on every path: the peers' send buffers are theirs again after it)
    if (he != hipSuccess) return e->fail(TRG_ERR_DEVICE, std::string("local exchange copy: ") + hipGetErrorString(he));
    return st;
  }
};

struct ExchangeState {
  std::unique_ptr<Transport> transport;
  int nranks = 0, rank = 0;
  DevArr rec, edges, send, recv, all, cnt;
  Pinned<long long> h_cnt;  // nranks + 1 words
};

// all-gather-v of `n` records of `rec_bytes` each, on the device: out = the ranks' records in rank order,
// counts[k] = rank k's number (n < 0 announces "this rank failed": every rank then returns an error
// instead of waiting in the payload collective).  One host round trip (the counts).
TrgStatus exchange_allgatherv(TrgEngine *e, ExchangeState &x, const void *d_mine, long long n, size_t rec_bytes,
                              std::vector<long long> &counts, void **d_all_out) {
  hipStream_t s = e->s_main;
  TrgStatus st;
  const int R = x.nranks;
  if ((st = ensure_bytes(e, x.cnt, (size_t)(R + 1) * sizeof(long long))) != TRG_OK) return st;
  long long *d_cnt = (long long *)x.cnt.p;
  HIPCHK(e, x.h_cnt.ensure(STITCH_MAX_TILES + 1));
  x.h_cnt[R] = n;
  HIPCHK(e, hipMemcpyAsync(d_cnt + R, x.h_cnt + R, sizeof(long long), hipMemcpyHostToDevice, s));
  if ((st = x.transport->all_gather(e, d_cnt + R, d_cnt, 1, sizeof(long long), s)) != TRG_OK) return st;
  HIPCHK(e, hipMemcpyAsync(x.h_cnt, d_cnt, (size_t)R * sizeof(long long), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  counts.assign(x.h_cnt.p, x.h_cnt.p + R);
  long long pad = 1, total = 0;
  for (long long c : counts) {
    if (c < 0) return e->fail(TRG_ERR_DEVICE, "stitch exchange: another rank reported a failure");
    pad = std::max(pad, c);
    total += c;
  }
  const size_t slot = (size_t)pad * rec_bytes;
  if ((st = ensure_bytes(e, x.send, slot)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, x.recv, slot * (size_t)R)) != TRG_OK) return st;
  if ((st = ensure_bytes(e, x.all, (size_t)std::max<long long>(total, 1) * rec_bytes)) != TRG_OK) return st;
  HIPCHK(e, hipMemsetAsync(x.send.p, 0, slot, s));
  if (n > 0) HIPCHK(e, hipMemcpyAsync(x.send.p, d_mine, (size_t)n * rec_bytes, hipMemcpyDeviceToDevice, s));
  if ((st = x.transport->all_gather(e, x.send.p, x.recv.p, slot, 1, s)) != TRG_OK) return st;
  size_t off = 0;
  for (int k = 0; k < R; ++k) {
    const size_t nb = (size_t)counts[k] * rec_bytes;
    if (nb) HIPCHK(e, hipMemcpyAsync((char *)x.all.p + off, (char *)x.recv.p + (size_t)k * slot, nb, hipMemcpyDeviceToDevice, s));
    off += nb;
  }
  *d_all_out = x.all.p;
  return TRG_OK;
}

TrgStatus comm_unique_id(TrgEngine *e, uint8_t id[TRG_COMM_ID_BYTES]) {
  if (!g_rccl.load()) return e->fail(TRG_ERR_DEVICE, g_rccl.err);
  static_assert(TRG_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
  ncclUniqueId u;
  RCCLCHK(e, g_rccl.GetUniqueId(&u));
  memcpy(id, u.internal, TRG_COMM_ID_BYTES);
  return TRG_OK;
}

TrgStatus comm_init(TrgEngine *e, const uint8_t id[TRG_COMM_ID_BYTES], int32_t nranks, int32_t rank) {
  if (!id || nranks < 1 || nranks > STITCH_MAX_TILES || rank < 0 || rank >= nranks)
    return e->fail(TRG_ERR_INVALID_ARG, "comm_init: bad arguments");
  if (!g_rccl.load()) return e->fail(TRG_ERR_DEVICE, g_rccl.err);
  if (!e->exchange) e->exchange.reset(new ExchangeState());
  ExchangeState &x = *e->exchange;
  x.transport.reset();
  ncclUniqueId u;
  memcpy(u.internal, id, TRG_COMM_ID_BYTES);
  std::unique_ptr<RcclTransport> t(new RcclTransport());
  RCCLCHK(e, g_rccl.CommInitRank(&t->comm, nranks, u, rank));
  t->owned = true;
  x.transport = std::move(t);
  x.nranks = nranks;
  x.rank = rank;
  return TRG_OK;
}

// A communicator the engine refuses is not kept: the one it had is gone (as after a comm_init that failed), and a
// later stitch_exchange finds none instead of indexing its count buffers with the refused communicator's size.
TrgStatus comm_adopt(TrgEngine *e, void *nccl_comm) {
  if (!nccl_comm) return e->fail(TRG_ERR_INVALID_ARG, "comm_adopt: null communicator");
  if (!g_rccl.load()) return e->fail(TRG_ERR_DEVICE, g_rccl.err);
  if (!e->exchange) e->exchange.reset(new ExchangeState());
  ExchangeState &x = *e->exchange;
  x.transport.reset();
  const ncclComm_t comm = (ncclComm_t)nccl_comm;
  int nranks = 0, rank = 0;
  RCCLCHK(e, g_rccl.CommCount(comm, &nranks));
  RCCLCHK(e, g_rccl.CommUserRank(comm, &rank));
  if (nranks > STITCH_MAX_TILES) return e->fail(TRG_ERR_INVALID_ARG, "comm_adopt: too many ranks");
  std::unique_ptr<RcclTransport> t(new RcclTransport());
  t->comm = comm;
  x.transport = std::move(t);
  x.nranks = nranks;
  x.rank = rank;
  return TRG_OK;
}

// Rank `rank` of the in-process group `name` (made by whoever joins first; gone with its last member).  Joining does
// not wait for the others: the first all-gather does.
TrgStatus comm_join_local(TrgEngine *e, const char *name, int32_t nranks, int32_t rank) {
  if (nranks < 1 || nranks > STITCH_MAX_TILES || rank < 0 || rank >= nranks)
    return e->fail(TRG_ERR_INVALID_ARG, "comm_join_local: bad arguments");
  if (!e->exchange) e->exchange.reset(new ExchangeState());
  ExchangeState &x = *e->exchange;
  x.transport.reset();  // (leaves the group it was in)
  std::unique_ptr<LocalTransport> t(new LocalTransport());
  std::string why;
  t->group = LocalGroup::join(name, nranks, rank, why);
  if (!t->group) return e->fail(TRG_ERR_INVALID_ARG, "comm_join_local: " + why);
  t->rank = rank;
  t->wait_seconds = &e->comm_wait_seconds;
  x.transport = std::move(t);
  x.nranks = nranks;
  x.rank = rank;
  return TRG_OK;
}

TrgStatus comm_destroy(TrgEngine *e) {
  (void)hipSetDevice(e->device);
  e->exchange.reset();
  return TRG_OK;
}

TrgStatus stitch_exchange(TrgEngine *e, const float core_xyxy[4], int32_t cols, int32_t rows, int32_t *n_boundary,
                          int32_t *n_cross) {
  if (!e->exchange || !e->exchange->transport) return e->fail(TRG_ERR_INVALID_ARG, "stitch_exchange: no communicator (trg_engine_comm_init)");
  ExchangeState &x = *e->exchange;
  const int R = x.nranks, tile = x.rank;
  if (!core_xyxy || cols < 1 || rows < 1 || cols * rows != R)
    return e->fail(TRG_ERR_INVALID_ARG, "stitch_exchange: cols x rows must equal the communicator's size");
  hipStream_t s = e->s_main;
  TrgStatus st, deferred = TRG_OK;
  std::string deferred_msg;
  // ---- 1: this tile's boundary records; the tile's node count rides behind them ---------------------------
  int32_t nb = 0;
  // (debug_stitch_cap: the first capacity in rows of rec and edges, so that tests reach the regrow loops)
  const size_t rec_rows = e->debug_stitch_cap > 0 ? (size_t)e->debug_stitch_cap + 1 : (size_t)1 << 14;
  const size_t edge_rows = e->debug_stitch_cap > 0 ? (size_t)e->debug_stitch_cap : (size_t)1 << 15;
  if ((st = ensure_bytes(e, x.rec, rec_rows * sizeof(TrgBoundaryRec))) != TRG_OK) return st;
  for (;;) {
    const int32_t cap = (int32_t)(x.rec.bytes / sizeof(TrgBoundaryRec)) - 1;
    st = stitch_boundary(e, core_xyxy, cols, rows, tile, (TrgBoundaryRec *)x.rec.p, cap, &nb);
    if (st != TRG_ERR_CAPACITY) break;
    ++e->stats.stitch_regrows;
    if ((st = ensure_bytes(e, x.rec, (size_t)(2 * nb + 2) * sizeof(TrgBoundaryRec))) != TRG_OK) break;
  }
  int32_t V = 0, E_ = 0;
  if (st == TRG_OK) st = graph_sizes(e, TRG_KIND_GLOBAL, &V, &E_);
  if (st == TRG_OK) {
    const TrgBoundaryRec tail = {V, 0.0f, 0.0f, 0.0f};
    hipError_t he = hipMemcpyAsync((TrgBoundaryRec *)x.rec.p + nb, &tail, sizeof(tail), hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);  // (tail is a stack object)
    if (he != hipSuccess) st = e->fail(TRG_ERR_DEVICE, std::string("stitch exchange tail row: ") + hipGetErrorString(he));
  }
  if (st != TRG_OK) {  // tell the others instead of leaving them in the collective
    deferred = st;
    deferred_msg = e->err;
  }
  std::vector<long long> counts;
  void *d_all = nullptr;
  st = exchange_allgatherv(e, x, x.rec.p, deferred == TRG_OK ? (long long)nb + 1 : -1, sizeof(TrgBoundaryRec), counts, &d_all);
  if (deferred != TRG_OK) return e->fail(deferred, deferred_msg);
  if (st != TRG_OK) return st;
  // the gathered block holds, per rank, its records and then the count row: split the two
  std::vector<int32_t> rec_off(R + 1, 0), node_off(R + 1, 0);
  {
    long long off = 0;
    std::vector<TrgBoundaryRec> tails(R);
    for (int k = 0; k < R; ++k) {
      off += counts[k];
      HIPCHK(e, hipMemcpyAsync(&tails[k], (TrgBoundaryRec *)d_all + (off - 1), sizeof(TrgBoundaryRec), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(e, hipStreamSynchronize(s));
    for (int k = 0; k < R; ++k) {
      rec_off[k + 1] = rec_off[k] + (int32_t)(counts[k] - 1);
      node_off[k + 1] = node_off[k] + tails[k].local_id;
    }
    // compact in place, front to back (rank k's records move down by k rows: memmove semantics per block)
    long long src = 0;
    for (int k = 0; k < R; ++k) {
      const size_t nbk = (size_t)(counts[k] - 1) * sizeof(TrgBoundaryRec);
      if (k > 0 && nbk)
        HIPCHK(e, hipMemcpyAsync((TrgBoundaryRec *)x.recv.p + rec_off[k], (TrgBoundaryRec *)d_all + src, nbk, hipMemcpyDeviceToDevice, s));
      else if (nbk)
        HIPCHK(e, hipMemcpyAsync(x.recv.p, d_all, nbk, hipMemcpyDeviceToDevice, s));
      src += counts[k];
    }
  }
  const TrgBoundaryRec *d_recs = (const TrgBoundaryRec *)x.recv.p;  // (recv is free again: the payload was copied out)
  // ---- 2: the cross edges this tile owns ------------------------------------------------------------------------
  int32_t nc = 0;
  if ((st = ensure_bytes(e, x.edges, edge_rows * sizeof(TrgCrossEdge))) != TRG_OK) return st;
  for (;;) {
    const int32_t cap = (int32_t)(x.edges.bytes / sizeof(TrgCrossEdge));
    st = stitch_cross(e, tile, R, d_recs, rec_off.data(), (TrgCrossEdge *)x.edges.p, cap, &nc);
    if (st != TRG_ERR_CAPACITY) break;
    ++e->stats.stitch_regrows;
    if ((st = ensure_bytes(e, x.edges, (size_t)(2 * nc + 2) * sizeof(TrgCrossEdge))) != TRG_OK) break;
  }
  if (st != TRG_OK) {
    deferred = st;
    deferred_msg = e->err;
  }
  // (the gathered records in recv are dead from here on: the exchange below reuses send / recv / all)
  std::vector<long long> ecounts;
  void *d_all_edges = nullptr;
  st = exchange_allgatherv(e, x, x.edges.p, deferred == TRG_OK ? (long long)nc : -1, sizeof(TrgCrossEdge), ecounts, &d_all_edges);
  if (deferred != TRG_OK) return e->fail(deferred, deferred_msg);
  if (st != TRG_OK) return st;
  long long ne = 0;
  for (long long c : ecounts) ne += c;
  // ---- 3: this tile's rows of the global graph ---------------------------------------------------------------------
  st = stitch_assemble(e, tile, R, node_off.data(), (const TrgCrossEdge *)d_all_edges, (int32_t)ne);
  if (st != TRG_OK) return st;
  if (n_boundary) *n_boundary = rec_off[R];
  if (n_cross) *n_cross = (int32_t)ne;
  return TRG_OK;
}

}  // namespace

extern "C" {

TrgStatus trg_engine_comm_unique_id(TrgEngine *e, uint8_t id[TRG_COMM_ID_BYTES]) {
  if (!id) return TRG_ERR_INVALID_ARG;
  return entry(e, "comm_unique_id", ENGINE, [&] { return comm_unique_id(e, id); });
}

TrgStatus trg_engine_comm_init(TrgEngine *e, const uint8_t id[TRG_COMM_ID_BYTES], int32_t nranks, int32_t rank) {
  return entry(e, "comm_init", DEVICE, [&] { return comm_init(e, id, nranks, rank); });
}

TrgStatus trg_engine_comm_adopt(TrgEngine *e, void *nccl_comm) {
  return entry(e, "comm_adopt", DEVICE, [&] { return comm_adopt(e, nccl_comm); });
}

TrgStatus trg_engine_comm_join_local(TrgEngine *e, const char *group_name, int32_t nranks, int32_t rank) {
  if (!group_name) return TRG_ERR_INVALID_ARG;
  return entry(e, "comm_join_local", DEVICE, [&] { return comm_join_local(e, group_name, nranks, rank); });
}

TrgStatus trg_engine_comm_destroy(TrgEngine *e) {
  return entry(e, "comm_destroy", ENGINE, [&] { return comm_destroy(e); });
}

TrgStatus trg_engine_stitch_exchange(TrgEngine *e, const float core_xyxy[4], int32_t cols, int32_t rows,
                                     int32_t *n_boundary, int32_t *n_cross) {
  return entry(e, "stitch_exchange", DEVICE,
               [&] { return stitch_exchange(e, core_xyxy, cols, rows, n_boundary, n_cross); });
}

}  // extern "C"
