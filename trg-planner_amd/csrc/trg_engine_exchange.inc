// trg_engine_exchange.inc -- the tile-boundary stitch with its two exchanges done natively over RCCL
// (included by trg_engine.cpp).  One call runs DESIGN.md section 7 for this rank's tile: boundary records
// -> all-gather-v -> cross edges -> all-gather-v -> this tile's rows of the global graph.  RCCL has no
// all-gather-v: each exchange is an all-gather of one count and one auxiliary word per rank (the only host round
// trip; the first exchange's word is the tile's node count), then an all-gather of payloads padded to the largest
// count, compacted on the device.  xGMI is point-to-point
// and these payloads are a few 10 KB, so latency decides: two small collectives per exchange, nothing
// bucketed.  A C / C++ consumer (the ROS nodes inherit TRGPlanner) needs no Python for N > 1;
// trg_planner/tiled.py::stitch_device calls the same entry point through ctypes.
//
// librccl is resolved at run time (dlopen): the engine has no link-time dependency on it, and a process
// that already loaded an RCCL (torch's) shares that instance when the soname matches.
//
// The all-gathers go through a Transport.  RCCL is the one a product uses.  The in-process transport
// (trg_engine_comm_join_local, never chosen unless asked for) lets R engines on one device in one process,
// each entered from its own thread, run the exchange's own logic -- counts and node counts, padded slots,
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
// count and the word, 1: the padded payload) and receives the ranks' blocks in rank order
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
  Pinned<long long> h_cnt;  // 2 (nranks + 1) words
};

// all-gather-v of `n` records of `rec_bytes` each, on the device, with one word `aux` per rank beside the count:
// out = the ranks' records in rank order, counts[k] = rank k's number, words[k] = its word (n < 0 announces "this
// rank failed": every rank then returns an error instead of waiting in the payload collective).  One host round
// trip: the counts and the words travel together.  The only function that enters collectives.
TrgStatus exchange_allgatherv(TrgEngine *e, ExchangeState &x, const void *d_mine, long long n, long long aux,
                              size_t rec_bytes, std::vector<long long> &counts, std::vector<long long> &words,
                              void **d_all_out) {
  hipStream_t s = e->s_main;
  TrgStatus st;
  const int R = x.nranks;
  if ((st = ensure_bytes(e, x.cnt, (size_t)(R + 1) * 2 * sizeof(long long))) != TRG_OK) return st;
  long long *d_cnt = x.cnt.as<long long>(), *d_own = d_cnt + 2 * R;
  HIPCHK(e, x.h_cnt.ensure(2 * (STITCH_MAX_TILES + 1)));
  long long *h_own = x.h_cnt + 2 * R;
  h_own[0] = n;
  h_own[1] = aux;
  HIPCHK(e, hipMemcpyAsync(d_own, h_own, 2 * sizeof(long long), hipMemcpyHostToDevice, s));
  if ((st = x.transport->all_gather(e, d_own, d_cnt, 2, sizeof(long long), s)) != TRG_OK) return st;
  HIPCHK(e, hipMemcpyAsync(x.h_cnt, d_cnt, (size_t)R * 2 * sizeof(long long), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  counts.resize(R);
  words.resize(R);
  long long pad = 1, total = 0;
  for (int k = 0; k < R; ++k) {
    counts[k] = x.h_cnt[2 * k];
    words[k] = x.h_cnt[2 * k + 1];
    if (counts[k] < 0) return e->fail(TRG_ERR_DEVICE, "stitch exchange: another rank reported a failure");
    pad = std::max(pad, counts[k]);
    total += counts[k];
  }
  const size_t slot = (size_t)pad * rec_bytes;
  if ((st = ensure_all(e, {{&x.send, slot}, {&x.recv, slot * (size_t)R},
                           {&x.all, (size_t)std::max<long long>(total, 1) * rec_bytes}})) != TRG_OK)
    return st;
  HIPCHK(e, hipMemsetAsync(x.send.p, 0, slot, s));
  if (n > 0) HIPCHK(e, hipMemcpyAsync(x.send.p, d_mine, (size_t)n * rec_bytes, hipMemcpyDeviceToDevice, s));
  if ((st = x.transport->all_gather(e, x.send.p, x.recv.p, slot, 1, s)) != TRG_OK) return st;
  size_t off = 0;
  for (int k = 0; k < R; ++k) {
    const size_t nb = (size_t)counts[k] * rec_bytes;
    if (nb) HIPCHK(e, hipMemcpyAsync(x.all.as<char>() + off, x.recv.as<char>() + (size_t)k * slot, nb, hipMemcpyDeviceToDevice, s));
    off += nb;
  }
  *d_all_out = x.all.p;
  return TRG_OK;
}

// One exchange of stitch_exchange after the step that made its payload: a failure of that step (`local`, its message
// in e->err) is announced in the count exchange, so that no rank waits for this one, and then returned as it was.
TrgStatus exchange_after(TrgEngine *e, ExchangeState &x, TrgStatus local, const void *d_mine, long long n, long long aux,
                         size_t rec_bytes, std::vector<long long> &counts, std::vector<long long> &words,
                         void **d_all_out) {
  const std::string local_msg = e->err;
  const TrgStatus st = exchange_allgatherv(e, x, d_mine, local == TRG_OK ? n : -1, aux, rec_bytes, counts, words, d_all_out);
  return local == TRG_OK ? st : e->fail(local, local_msg);
}

// A step that writes up to `cap` rows into `buf` and reports in *n how many it has, run until they fit: a step that
// ends with TRG_ERR_CAPACITY gets twice the rows it asked for (stats.stitch_regrows counts these).
template <typename Step>
TrgStatus stitch_grown(TrgEngine *e, DevArr &buf, size_t row_bytes, const int32_t *n, Step step) {
  TrgStatus st;
  while ((st = step((int32_t)(buf.bytes / row_bytes))) == TRG_ERR_CAPACITY) {
    ++e->stats.stitch_regrows;
    if ((st = ensure_bytes(e, buf, (size_t)(2 * *n + 2) * row_bytes)) != TRG_OK) break;
  }
  return st;
}

TrgStatus comm_unique_id(TrgEngine *e, uint8_t id[TRG_COMM_ID_BYTES]) {
  if (!g_rccl.load()) return e->fail(TRG_ERR_DEVICE, g_rccl.err);
  static_assert(TRG_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
  ncclUniqueId u;
  RCCLCHK(e, g_rccl.GetUniqueId(&u));
  memcpy(id, u.internal, TRG_COMM_ID_BYTES);
  return TRG_OK;
}

// Installs the transport that `make` builds.  The one the engine had goes first (an owned communicator is destroyed, a
// local one leaves its group), and when `make` refuses, none is kept: a later stitch_exchange finds no communicator
// instead of indexing its count buffers with the size of one that was refused.
template <typename Make>
TrgStatus comm_install(TrgEngine *e, Make make) {
  if (!e->exchange) e->exchange.reset(new ExchangeState());
  ExchangeState &x = *e->exchange;
  x.transport.reset();
  std::unique_ptr<Transport> t;
  int nranks = 0, rank = 0;
  const TrgStatus st = make(t, nranks, rank);
  if (st != TRG_OK) return st;
  x.transport = std::move(t);
  x.nranks = nranks;
  x.rank = rank;
  return TRG_OK;
}

TrgStatus comm_init(TrgEngine *e, const uint8_t id[TRG_COMM_ID_BYTES], int32_t nranks, int32_t rank) {
  if (!id || nranks < 1 || nranks > STITCH_MAX_TILES || rank < 0 || rank >= nranks)
    return e->fail(TRG_ERR_INVALID_ARG, "comm_init: bad arguments");
  if (!g_rccl.load()) return e->fail(TRG_ERR_DEVICE, g_rccl.err);
  return comm_install(e, [&](std::unique_ptr<Transport> &out, int &n, int &r) {
    ncclUniqueId u;
    memcpy(u.internal, id, TRG_COMM_ID_BYTES);
    std::unique_ptr<RcclTransport> t(new RcclTransport());
    RCCLCHK(e, g_rccl.CommInitRank(&t->comm, nranks, u, rank));
    t->owned = true;
    out = std::move(t);
    n = nranks;
    r = rank;
    return TRG_OK;
  });
}

TrgStatus comm_adopt(TrgEngine *e, void *nccl_comm) {
  if (!nccl_comm) return e->fail(TRG_ERR_INVALID_ARG, "comm_adopt: null communicator");
  if (!g_rccl.load()) return e->fail(TRG_ERR_DEVICE, g_rccl.err);
  return comm_install(e, [&](std::unique_ptr<Transport> &out, int &n, int &r) {
    std::unique_ptr<RcclTransport> t(new RcclTransport());
    t->comm = (ncclComm_t)nccl_comm;  // (not owned: the caller destroys it)
    RCCLCHK(e, g_rccl.CommCount(t->comm, &n));
    RCCLCHK(e, g_rccl.CommUserRank(t->comm, &r));
    if (n > STITCH_MAX_TILES) return e->fail(TRG_ERR_INVALID_ARG, "comm_adopt: too many ranks");
    out = std::move(t);
    return TRG_OK;
  });
}

// Rank `rank` of the in-process group `name` (made by whoever joins first; gone with its last member).  Joining does
// not wait for the others: the first all-gather does.
TrgStatus comm_join_local(TrgEngine *e, const char *name, int32_t nranks, int32_t rank) {
  if (nranks < 1 || nranks > STITCH_MAX_TILES || rank < 0 || rank >= nranks)
    return e->fail(TRG_ERR_INVALID_ARG, "comm_join_local: bad arguments");
  return comm_install(e, [&](std::unique_ptr<Transport> &out, int &n, int &r) {
    std::unique_ptr<LocalTransport> t(new LocalTransport());
    std::string why;
    t->group = LocalGroup::join(name, nranks, rank, why);
    if (!t->group) return e->fail(TRG_ERR_INVALID_ARG, "comm_join_local: " + why);
    t->rank = rank;
    t->wait_seconds = &e->comm_wait_seconds;
    out = std::move(t);
    n = nranks;
    r = rank;
    return TRG_OK;
  });
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
  // (debug_stitch_cap: the first capacity in rows of rec and edges, so that tests reach the regrows)
  const size_t rec_rows = e->debug_stitch_cap > 0 ? (size_t)e->debug_stitch_cap : (size_t)1 << 14;
  const size_t edge_rows = e->debug_stitch_cap > 0 ? (size_t)e->debug_stitch_cap : (size_t)1 << 15;
  TrgStatus st;
  std::vector<long long> counts, words;
  void *d_all = nullptr;
  // ---- 1: this tile's boundary records; the tile's node count rides in the count exchange ----------------------
  int32_t nb = 0, V = 0, E_ = 0;
  if ((st = ensure_bytes(e, x.rec, rec_rows * sizeof(TrgBoundaryRec))) != TRG_OK) return st;
  st = stitch_grown(e, x.rec, sizeof(TrgBoundaryRec), &nb, [&](int32_t cap) {
    return stitch_boundary(e, core_xyxy, cols, rows, tile, x.rec.as<TrgBoundaryRec>(), cap, &nb);
  });
  if (st == TRG_OK) st = graph_sizes(e, TRG_KIND_GLOBAL, &V, &E_);
  st = exchange_after(e, x, st, x.rec.p, nb, V, sizeof(TrgBoundaryRec), counts, words, &d_all);
  if (st != TRG_OK) return st;
  const TrgBoundaryRec *d_recs = (const TrgBoundaryRec *)d_all;  // (the gathered block as it is)
  std::vector<int32_t> rec_off(R + 1, 0), node_off(R + 1, 0);
  for (int k = 0; k < R; ++k) {
    rec_off[k + 1] = rec_off[k] + (int32_t)counts[k];
    node_off[k + 1] = node_off[k] + (int32_t)words[k];
  }
  // ---- 2: the cross edges this tile owns ------------------------------------------------------------------------
  int32_t nc = 0;
  if ((st = ensure_bytes(e, x.edges, edge_rows * sizeof(TrgCrossEdge))) != TRG_OK) return st;
  st = stitch_grown(e, x.edges, sizeof(TrgCrossEdge), &nc, [&](int32_t cap) {
    return stitch_cross(e, tile, R, d_recs, rec_off.data(), x.edges.as<TrgCrossEdge>(), cap, &nc);
  });
  // (the gathered records are dead from here on: the exchange below reuses send / recv / all)
  void *d_all_edges = nullptr;
  st = exchange_after(e, x, st, x.edges.p, nc, 0, sizeof(TrgCrossEdge), counts, words, &d_all_edges);
  if (st != TRG_OK) return st;
  long long ne = 0;
  for (long long c : counts) ne += c;
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
