// trg_engine.cpp -- host side of the MI355X TRG construction engine and its C ABI
// (include/trg_engine.h).
//
// Division of labour:
//   GPU  : every function of (positions, map) -- map index build, isCollision, elevation lookup,
//          rejection sampling, edge risk (segment walk + ellipse gather + PCA).  trg_kernels.hip
//   host : everything that depends on graph STATE and is inherently sequential in the reference --
//          the FIFO of expandGraph (trg.cpp:376-381), nearest existing node / merge test
//          (trg.cpp:408-417), wireEdge's dedupe (trg.cpp:255-267), cleanGraph's renumbering
//          (trg.cpp:491-535), A* (trg.cpp:603-690).  The host never evaluates a map query itself:
//          without a working HIP device every entry point fails with TRG_ERR_DEVICE.
//
// The BFS is replayed in exactly the reference's order; GPU work is issued ahead of the replay in
// chunks of queued nodes (the samples of a node depend only on its position and id), so device
// latency hides behind the host loop.
#include <hip/hip_runtime.h>
#include <math.h>  // float overloads of atan2 etc. in the global namespace, as the reference has

#include <algorithm>
#include <array>
#include <atomic>
#include <cstddef>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <functional>
#include <memory>
#include <optional>
#include <queue>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/trg_engine.h"
#include "abi_frame.h"
#include "graph_json.h"
#include "host_index.h"
#include "map_order_sim.h"
#include "node_map.h"
#include "trg_kernels.h"
#include "zone_sets.h"

namespace {

using namespace trg;
using Clock = std::chrono::steady_clock;

inline double ms_since(Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}
inline float norm2f(float dx, float dy) { return sqrtf(dx * dx + dy * dy); }

// fn(begin, end) over [0, n) on up to 8 host threads (bulk host passes over the graph: cleanGraph, CSR <-> edge pool)
template <typename F>
void parallel_ranges(size_t n, F fn) {
  const size_t hw = std::max(1u, std::thread::hardware_concurrency());
  const size_t T = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(8, hw), (n + 65535) / 65536));
  fork_join(T, [&](size_t t) { fn(n * t / T, n * (t + 1) / T); });
}

// ---- owners of GPU resources ---------------------------------------------------------------------
// Whatever this translation unit holds on the device, in pinned host memory or as a HIP handle lives in one of
// these: move-only, released by the destructor, and the capacity sits inside the owner and changes only with
// the block itself.  An empty owner makes no HIP call, so an engine that never saw a device is destroyed
// without one.  The owners of an engine are released with its device current (trg_engine_destroy).

// device memory with its capacity in bytes
struct DevArr {
  void *p = nullptr;
  size_t bytes = 0;
  DevArr() = default;
  DevArr(DevArr &&o) noexcept { *this = std::move(o); }
  DevArr &operator=(DevArr &&o) noexcept {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    return *this;
  }
  ~DevArr() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  // at least `need` bytes, at exactly that size when it has to grow; the contents are not kept, and the old
  // block goes first (the arrays of a 10 M-point map are too large to hold twice or to give head-room).
  // ensure_bytes below is the growth with head-room for arrays that creep up.
  hipError_t reserve(size_t need) {
    if (p && bytes >= need) return hipSuccess;
    release();
    const hipError_t err = hipMalloc(&p, need);
    if (err != hipSuccess) p = nullptr;
    else bytes = need;
    return err;
  }
  template <typename T>
  T *as() const {
    return (T *)p;
  }
};

// a DevArr of T, sized in elements: it goes into a launch as the T* it holds
template <typename T>
struct DevBuf : DevArr {
  hipError_t ensure(size_t n) { return reserve(n * sizeof(T)); }
  operator T *() const { return (T *)p; }
};

// pinned host memory of T, the same way (h_ctrs of the device BFS is Mapped | Coherent: the flags are a parameter)
template <typename T>
struct Pinned {
  T *p = nullptr;
  size_t count = 0;
  Pinned() = default;
  Pinned(Pinned &&o) noexcept { *this = std::move(o); }
  Pinned &operator=(Pinned &&o) noexcept {
    std::swap(p, o.p);
    std::swap(count, o.count);
    return *this;
  }
  ~Pinned() { release(); }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    count = 0;
  }
  hipError_t ensure(size_t n, unsigned flags = hipHostMallocDefault) {
    if (p && count >= n) return hipSuccess;
    release();
    const hipError_t err = hipHostMalloc((void **)&p, n * sizeof(T), flags);
    if (err != hipSuccess) p = nullptr;
    else count = n;
    return err;
  }
  operator T *() const { return p; }
  T *operator->() const { return p; }
  template <typename U>
  U *as() const {
    return (U *)p;
  }
};

// `cap` elements in pinned host memory and as many on the device: the two ends of a staged copy
template <typename T>
struct PinnedBuf {
  Pinned<T> h;
  DevBuf<T> d;
  hipError_t ensure(size_t cap) {
    const hipError_t err = h.ensure(cap);
    return err != hipSuccess ? err : d.ensure(cap);
  }
};

struct Event {
  hipEvent_t ev = nullptr;
  Event() = default;
  Event(Event &&o) noexcept { std::swap(ev, o.ev); }
  Event &operator=(Event &&o) noexcept {
    std::swap(ev, o.ev);
    return *this;
  }
  ~Event() { if (ev) (void)hipEventDestroy(ev); }
  hipError_t create(bool timing = true) {  // (one that exists is kept)
    return ev ? hipSuccess : hipEventCreateWithFlags(&ev, timing ? hipEventDefault : hipEventDisableTiming);
  }
  operator hipEvent_t() const { return ev; }
};

struct Stream {  // non-blocking
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream &&o) noexcept { std::swap(s, o.s); }
  Stream &operator=(Stream &&o) noexcept {
    std::swap(s, o.s);
    return *this;
  }
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  hipError_t create_with_priority(int priority) {
    return s ? hipSuccess : hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority);
  }
  operator hipStream_t() const { return s; }
};

struct IndexScratch {  // temporaries of build_index, grown on demand
  DevBuf<int> cell_of, rank, counts, tmp;  // the direct path (huge grids only)
  DevBuf<int> hist, base, bin_tmp;         // the path through bins
  DevBuf<float4> aos;
};

struct DevMap {
  size_t n = 0;
  DevBuf<float> x, y, z;
  DevBuf<int> perm, cell_start;
  DevBuf<float4> pt;  // the sorted points as 16-byte records (MapView::pt)
  MapView view{};
  float g = 0;
  float bounds[4] = {0, 0, 0, 0};
  bool valid = false;
  // the top of the reference's insertion-built kd-tree over this map: its first points (original index
  // < top_m), built lazily when a nearest-point tie has to be broken (map_first_of_two)
  int top_m = 0;
  std::vector<float> top_xy;
  std::vector<int> top_left, top_right;
  // For the global map the top is prepared beside the build (start_map_top): its points are fetched on the aux
  // stream and a helper thread inserts them; whoever needs the top (or replaces / frees the map) joins it first.
  // (The helper reads the map's arrays and the engine's top_xy_h / top_ev: those outlive it, see TrgEngine.)
  std::thread top_thread;
  void top_wait() {
    if (top_thread.joinable()) top_thread.join();
  }
  ~DevMap() { top_wait(); }
};

// results of one speculative / deferred edge evaluation as the replay consumes them
struct CallRec {
  int n1, n2;
  int status;  // EDGE_* | flags, -1 = pending
  float weight, dist;
};

// std::vector whose resize() leaves trivially constructible elements uninitialised (the bulk builders overwrite
// every element; value-initialising four 6.7 M-entry arrays cost 10 ms per cleanGraph at C3)
template <typename T>
struct NoInitAlloc : std::allocator<T> {
  template <typename U>
  struct rebind {
    using other = NoInitAlloc<U>;
  };
  NoInitAlloc() = default;
  template <typename U>
  NoInitAlloc(const NoInitAlloc<U> &) {}
  template <typename U>
  void construct(U *p) noexcept {
    ::new ((void *)p) U;
  }
  template <typename U, typename... A>
  void construct(U *p, A &&...a) {
    ::new ((void *)p) U(std::forward<A>(a)...);
  }
};
template <typename T>
using RawVec = std::vector<T, NoInitAlloc<T>>;

struct EdgePool {
  RawVec<int> dst, next;
  RawVec<float> w, dist;
  std::vector<int> head, tail, deg;
  void reset(size_t nodes) {
    dst.clear();
    next.clear();
    w.clear();
    dist.clear();
    head.assign(nodes, -1);
    tail.assign(nodes, -1);
    deg.assign(nodes, 0);
  }
  void grow_nodes(size_t nodes) {
    if (head.size() < nodes) {
      head.resize(nodes, -1);
      tail.resize(nodes, -1);
      deg.resize(nodes, 0);
    }
  }
  bool has(int a, int b) const {
    for (int e = head[a]; e >= 0; e = next[e])
      if (dst[e] == b) return true;
    return false;
  }
  // rows laid out one after the other (offs[nodes + 1]); the caller fills dst / w / dist of every row and calls
  // link_rows: the lists then read like pushes in that order, and later pushes append behind them
  void alloc_rows(const std::vector<int> &offs) {
    const size_t nodes = offs.size() - 1, E = (size_t)offs[nodes];
    const size_t room = E + E / 8 + 65536;  // (the pushes that follow must not reallocate 100 MB)
    dst.reserve(room);
    next.reserve(room);
    w.reserve(room);
    dist.reserve(room);
    dst.resize(E);
    next.resize(E);
    w.resize(E);
    dist.resize(E);
    head.resize(nodes);
    tail.resize(nodes);
    deg.resize(nodes);
  }
  void link_rows(const std::vector<int> &offs, size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; ++i) {
      const int a = offs[i], b = offs[i + 1];
      deg[i] = b - a;
      head[i] = b > a ? a : -1;
      tail[i] = b > a ? b - 1 : -1;
      for (int k = a; k < b; ++k) next[k] = k + 1 < b ? k + 1 : -1;
    }
  }
  void push(int a, int b, float ww, float dd) {
    const int e = (int)dst.size();
    dst.push_back(b);
    w.push_back(ww);
    dist.push_back(dd);
    next.push_back(-1);
    if (tail[a] >= 0) {
      next[tail[a]] = e;
    } else {
      head[a] = e;
    }
    tail[a] = e;
    deg[a]++;
  }
};

// Minimal vector over pinned host memory (hipHostMalloc): the CSR the engine hands out is the
// destination of the final device-to-host copies, which run at full PCIe rate only into pinned
// pages; no value-initialisation on resize (an 80 MB memset would cost as much as the copy).
template <typename T>
struct PVec {
  T *p = nullptr;
  size_t n = 0, cap = 0;
  bool pinned = false;
  PVec() = default;
  PVec(const PVec &) = delete;
  PVec &operator=(const PVec &o) {
    resize(o.n);
    if (o.n) memcpy(p, o.p, o.n * sizeof(T));
    return *this;
  }
  PVec &operator=(const std::vector<T> &o) {
    resize(o.size());
    if (!o.empty()) memcpy(p, o.data(), o.size() * sizeof(T));
    return *this;
  }
  ~PVec() { release(); }
  void release() {
    if (p) {
      if (pinned) (void)hipHostFree(p);
      else free(p);
    }
    p = nullptr;
    n = cap = 0;
  }
  void reserve(size_t m) {
    if (m <= cap) return;
    size_t nc = std::max(m, cap + cap / 2);
    T *np = nullptr;
    bool pin = hipHostMalloc((void **)&np, nc * sizeof(T), hipHostMallocDefault) == hipSuccess;
    if (!pin) np = (T *)malloc(nc * sizeof(T));
    if (n) memcpy(np, p, n * sizeof(T));
    if (p) {
      if (pinned) (void)hipHostFree(p);
      else free(p);
    }
    p = np;
    cap = nc;
    pinned = pin;
  }
  void resize(size_t m) {
    reserve(m);
    n = m;
  }
  void assign(size_t m, const T &v) {
    resize(m);
    for (size_t i = 0; i < m; ++i) p[i] = v;
  }
  void clear() { n = 0; }
  bool empty() const { return n == 0; }
  size_t size() const { return n; }
  T *data() { return p; }
  const T *data() const { return p; }
  T &operator[](size_t i) { return p[i]; }
  const T &operator[](size_t i) const { return p[i]; }
  T *begin() { return p; }
  T *end() { return p + n; }
  const T *begin() const { return p; }
  const T *end() const { return p + n; }
  void push_back(const T &v) {
    if (n == cap) reserve(std::max<size_t>(16, cap * 2));
    p[n++] = v;
  }
  template <typename It>
  void append(It first, It last) {
    const size_t m = (size_t)(last - first);
    reserve(n + m);
    for (size_t i = 0; i < m; ++i) p[n + i] = first[i];
    n += m;
  }
};

struct Csr {
  PVec<float> xyz;
  PVec<int32_t> state, rowptr, col, cid;
  PVec<float> w, dist;
  void clear() {
    xyz.clear();
    state.clear();
    rowptr.clear();
    col.clear();
    cid.clear();
    w.clear();
    dist.clear();
  }
};

template <typename T>
struct View {  // host / device views into a chunk's packed blobs
  T *h = nullptr;
  T *d = nullptr;
};

struct Chunk {
  int first = 0, count = 0;  // queue positions [first, first+count)
  bool in_flight = false;
  Event done;
  Event t0, t1, t2;  // sample start / sample end / edges end
  // one packed input blob (H2D) and one packed output blob (D2H) per chunk: a single copy each way
  PinnedBuf<uint32_t> in_blob, out_blob;
  DevBuf<float> mid;  // phase-1 edge records (device only)
  View<float> node_xy, node_xyz, sx, sy, sz, weight, dist;
  View<int> node_id, n_acc, n_draws, status;
  // nearest-map-point ties of accepted samples: [0] = count, records from word 4 (MapTieRec)
  PinnedBuf<int> mt;
  size_t in_words = 0, out_words = 0;
  void carve(int cnt, int S) {
    const size_t c = (size_t)cnt, cs = c * (size_t)S;
    auto iv = [&](size_t off) { return View<int>{in_blob.h.as<int>() + off, in_blob.d.as<int>() + off}; };
    auto fv = [&](size_t off) { return View<float>{in_blob.h.as<float>() + off, in_blob.d.as<float>() + off}; };
    node_xy = fv(0);
    node_xyz = fv(2 * c);
    node_id = iv(5 * c);
    in_words = 6 * c;
    auto io = [&](size_t off) { return View<int>{out_blob.h.as<int>() + off, out_blob.d.as<int>() + off}; };
    auto fo = [&](size_t off) { return View<float>{out_blob.h.as<float>() + off, out_blob.d.as<float>() + off}; };
    n_acc = io(0);
    n_draws = io(c);
    sx = fo(2 * c);
    sy = fo(2 * c + cs);
    sz = fo(2 * c + 2 * cs);
    status = io(2 * c + 3 * cs);
    weight = fo(2 * c + 4 * cs);
    dist = fo(2 * c + 5 * cs);
    out_words = 2 * c + 6 * cs;
  }
};

struct EdgeBatch {
  bool in_flight = false;
  int count = 0;
  Event done, t0, t1;
  std::vector<int> call_idx;  // which CallRec each row fills
  PinnedBuf<float> p1, p2, weight, dist;
  PinnedBuf<int> status;
  DevBuf<float> mid;
};

struct BfsBuffers;  // device-resident BFS state (trg_engine_bfs.inc)
struct StitchBufs;  // scratch of the tile-boundary stitch (trg_engine_stitch.inc)
struct Uploader;    // host cloud -> HBM staging (trg_engine_map.ipp)
struct ExchangeState;  // transport (RCCL communicator or in-process group) + buffers of the native stitch exchange (trg_engine_exchange.inc)
struct FieldBufs;      // device buffers of the cost field (trg_engine_field.ipp)
struct TiledFieldBufs; // solve graph and work arrays of the cost field across tiles (trg_engine_field_tiled.inc)

// the engine's own copy of the cleaned global graph in HBM, for when the device build's is not current
// (ensure_dev_graph): its two parts, and the sizes they were copied at
struct DevGraphUpload {
  DevArr xyz, state;             // VIEW_UP_NODES
  DevArr rowptr, col, w, dist;   // VIEW_UP_EDGES
  long long nodes_of = -1, edges_of = -1;  // V, and V << 32 | E
};

}  // namespace

struct TrgEngine;
namespace {
TrgStatus stitch_fetch(TrgEngine *e);  // trg_engine_stitch.inc
void field_release(TrgEngine *e);      // trg_engine_field.ipp
}
// Scratch of one A* search over the CSR.  open_check / close_list of the reference (trg.cpp:619-620,
// unordered_maps keyed by node id) are flat arrays whose entries count only when their stamp equals the
// search's generation, so nothing of size V is cleared per query.
struct PlanScratch {
  struct Opt {  // OptimizeNode (TRG.h:42-48): f_cost and g_cost are floats
    int id;
    int parent;  // index into pool, -1 for the start
    float f, g;
  };
  std::vector<Opt> pool;
  std::vector<int> heap;
  std::vector<uint32_t> open_gen, close_gen;
  std::vector<int> open_idx;
  uint32_t gen = 0;
  std::vector<int> chain, hits, tied;
  void begin(size_t V) {
    if (open_gen.size() != V) {
      open_gen.assign(V, 0);
      close_gen.assign(V, 0);
      open_idx.assign(V, -1);
      gen = 0;
    }
    if (++gen == 0) {  // wrapped: start over
      std::fill(open_gen.begin(), open_gen.end(), 0u);
      std::fill(close_gen.begin(), close_gen.end(), 0u);
      gen = 1;
    }
    pool.clear();
    heap.clear();
  }
};

// Members are destroyed last to first, and the order below is the order of teardown that matters: the three
// streams come first, so they go after everything that may hold work in them, after the uploader's own streams
// and after the RCCL communicator (ExchangeState); top_xy_h / top_ev stand before the maps, whose destructor
// joins the helper thread that reads them (and the map's arrays).  trg_engine_destroy makes the engine's
// device current and synchronises it before any of this runs.
struct TrgEngine {
  TrgEngine();   // (both defined at the end of this file, where the types behind the unique_ptrs are complete)
  ~TrgEngine();
  TrgParams prm{};
  int device = 0;
  int wall_clock_khz = 0;  // rate of the device's constant wall clock (wall_clock64)
  std::string err;
  std::string arch;
  bool device_ok = false;  // create went through: the entry points run (entry(), DEVICE)

  Stream s_main, s_edge;
  Stream s_aux;  // rare-event work (nearest-point tie walks) beside whatever the main stream holds
  DevBuf<float> top_xy_d;  // staging of start_map_top: device,
  Pinned<float> top_xy_h;  // pinned host,
  Event top_ev;            // and "fetched"
  DevMap gmap, lmap;
  IndexScratch idx_scratch;
  DevBuf<DeviceCounters> d_ctr;
  DevBuf<unsigned> d_bounds;

  // sampler
  TrgSampler sampler{1, 16};
  std::vector<float> cos_t, sin_t;
  DevBuf<float> d_cos, d_sin;
  int table_bits_dev = 0;
  uint32_t epoch = 0;
  uint32_t epoch_base = 0;  // tiled builds: sampler epoch of this tile
  float core[4] = {-INFINITY, -INFINITY, INFINITY, INFINITY};  // tiled builds: node creation region

  // ---- host graph state ("Host graph state and its views") -----------------------------------------
  // The global graph is the node arrays (slot == id, ids dense at all times) and the container history; all else is a
  // view, stamped with the graph_version it is current for.  Only its ensure_* reads the stamp; graph_changed() commits.
  //   view             data                         brought up to date by                        asked for by
  //   VIEW_POOL        edges                        host build, update, load; ensure_pool        update, save_json, graph("local")
  //   VIEW_GRID        grid                         the same; ensure_host_grid                   update, plan, cost field, is_frontier
  //   VIEW_KD_ORDER    kd_insert_order              the same; ensure_kd_order                    kd_sync, ensure_kd_order_arrays, update
  //   VIEW_KD          kd, a prefix of the order    kd_sync                                      distance ties, hits near a radius
  //   VIEW_KDO         kdo_x / kdo_y / kdo_index    ensure_kd_order_arrays                       plan, cost field: order questions
  //   VIEW_CSR         csr_global                   every build, update, load; ensure_csr_global plan, cost field, graph("global"), stitch
  //   VIEW_DEV_CSR     the cleaned CSR in HBM       device build; update drops it (dev_csr)      cost field, stitch: spares an upload
  //   VIEW_UP_NODES    dev_up: xyz, state           ensure_dev_graph, when no VIEW_DEV_CSR       cost field, stitch
  //   VIEW_UP_EDGES    dev_up: rowptr, col, w, dist ensure_dev_graph, when no VIEW_DEV_CSR       cost field, stitch_assemble
  //   VIEW_STITCH_DEV  csr_stitched's edges in HBM  stitch_assemble; stitch_fetch un-stamps      graph("stitched")
  // (the cost field's edge costs carry their own stamp in FieldBufs, the tiled cost field's solve graph in TiledFieldBufs)
  enum GraphView { VIEW_POOL, VIEW_GRID, VIEW_KD_ORDER, VIEW_KD, VIEW_KDO, VIEW_CSR, VIEW_DEV_CSR, VIEW_UP_NODES,
                   VIEW_UP_EDGES, VIEW_STITCH_DEV, VIEW_COUNT };
  uint64_t graph_version = 1;            // bumped by graph_changed() alone
  uint64_t view_stamp[VIEW_COUNT] = {};  // graph_version each view is current for (0: none)
  bool current(GraphView v) const { return view_stamp[v] == graph_version; }
  std::vector<float> nx, ny, nz;
  std::vector<int> nstate;
  std::vector<int> ncid;  // creation index since the last build began
  int next_cid = 0;       // ... of the next node: counts every node created, the dropped ones too, through the updates
  int node_id = 0;
  std::unordered_map<int, int> order_map;  // mirrors trgStruct::nodes (iteration order only)
  // After a device build the container history is carried by an O(n) replica of the hashtable's
  // iteration order (map_order_sim.h); the real map is rebuilt from it only if a host path needs it.
  MapOrderSim nodes_sim;
  // Which of the two carries the container history: nodes_sim (true, from a device build on) or order_map (false,
  // from ensure_real_map on).  Not a view and no validity flag: graph_changed() never touches it.
  bool history_in_sim = false;
  std::vector<int> last_new2old;  // of the last host cleanGraph: old id of every surviving node
  EdgePool edges;
  NodeGrid grid;
  std::vector<int> kd_insert_order;  // ids in the order the reference inserted them
  NodeKd kd;                         // reference-shaped index of the current node set
  std::vector<float> kdo_x, kdo_y;   // positions in the node tree's insertion order, for the planner's rare order
  std::vector<int> kdo_index;        // questions (nearest-node ties, several goal hits): node id -> position
  Csr csr_global;
  DevGraphUpload dev_up;   // csr_global and nstate in HBM (VIEW_UP_NODES, VIEW_UP_EDGES)
  Csr csr_stitched;        // tiled builds: this tile's rows of the stitched global graph
  int stitched_edges = 0;  // ... and their edge count (the edge arrays may still be in HBM only)
  // the node offsets and the tile of the last stitch_assemble that went through (kept when the rows are voided: the
  // tiled cost field judges its sources by them), and a count of such stitches, the stamp of what is built from the rows
  std::vector<int32_t> stitch_node_off;
  int stitch_tile = -1;
  uint64_t stitch_serial = 0;
  float root_pos[2] = {0, 0};
  float local_root[2] = {0, 0};
  std::unordered_map<int, int> local_map;  // mirrors local trgStruct::nodes (iteration order)
  std::vector<int> local_nodes;  // ids in local_map's iteration order
  bool step3 = false;

  // build scratch
  std::vector<int> queue;
  std::vector<CallRec> calls;
  static constexpr int NCHUNK = 3;
  static constexpr int CHUNK_MAX = 4096;
  Chunk chunks[NCHUNK];
  Chunk root_chunk;  // samples + speculative edges of updateGraph's expansion roots, fetched in bulk
  static constexpr int NEBATCH = 3;
  static constexpr int EBATCH_MAX = 1 << 16;
  EdgeBatch ebatches[NEBATCH];
  std::vector<int> pending_calls;

  // small synchronous scratch
  PinnedBuf<float> sy_in, sy_in2, sy_f0, sy_f1;
  PinnedBuf<int> sy_i0, sy_i1, sy_i2;
  DevBuf<float> sy_mid;
  // exact nearest-map-point tie-break scratch (map_nn_exact)
  PinnedBuf<MapTieSet> mt_set;
  PinnedBuf<MapTieWalk> mt_walk;

  Csr csr_pre, csr_local;
  std::unique_ptr<StitchBufs> stitch;
  bool keep_preclean = false;    // instrumentation: snapshot the graph before cleanGraph
  bool use_device_bfs = true;    // device-resident BFS (off: host replay)
  bool defer_overlap = true;     // deferred edge evaluations pipelined behind the level loop on a 2nd stream
  bool known_start_disc = true;  // edge walks that start at a node the level loop created skip their first disc (BfsDev::ndisc)
  bool lazy_tie_repair = true;   // a map-point tie is looked up only where the sample's elevation is read (fix_map_ties)
  bool tail_overlap = true;      // after the loop: the creating edges' covariances beside the cleaned graph's copy to the host
  bool tail_early_copy = true;   // ... and the node arrays on their way to the host before the rows are filled (plain builds with tail_overlap)
  int debug_order_run_cap = 0;   // test hook: at most n runs of the container order go to the device (above: host expansion)
  PlanScratch plan_scratch;  // the planner's search scratch (A* runs straight on csr_global, see plan_on_csr)
  std::unique_ptr<Uploader> uploader;  // host cloud -> HBM staging (upload_and_build): pinned slots, streams and events
                                       // of its copy threads, made on the first cloud that needs them
  std::unique_ptr<ExchangeState> exchange;  // tiled builds: RCCL communicator and buffers of the native stitch
                                            // exchange, made by trg_engine_comm_init / comm_adopt
  std::unique_ptr<FieldBufs> field;  // cost field: work arrays and edge costs (cached per graph_version)
  std::unique_ptr<TiledFieldBufs> tiled;  // cost field across tiles: the solve graph (per stitch) and its work arrays
  double field_delta_scale = 4.0;  // cost field: bucket width in mean edge costs (a measurement knob, see set_option)
  // The node map of trg_engine_cost_field_refresh: for every node of the current graph its id in the graph of the
  // retained cost-field solve, -1 for a node made since.  A solve starts it as the identity, update_graph composes
  // it with its cleanGraph's renumbering; a new solve's start, every graph_changed() (init_graph, load_json, a
  // reset, an update's own before it composes) and an update that fails leave none.
  NodeMap field_map;
  // The same for the retained solve across tiles (trg_engine_tiled_cost_field_refresh): LOCAL ids of this tile's graph
  // at the tiled solve.  A tiled solve or refresh that succeeds starts it as the identity; the rest is field_map's.
  NodeMap tiled_map;
  int debug_tie_every = 0;       // test hook: treat every n-th BFS level as tie-affected
  int debug_spec_bound = 0;      // test hook: cap the speculative sampling launch at n nodes
  int debug_fallback_level = -1; // test hook: the device BFS declines at this level
  bool tie_inplace = true;       // node-distance ties settled slot by slot on the committed level (off: host level replay)
  int debug_lookback_level = -1; // test hook: one workgroup's commit look-back gives up at this level
  int debug_stall_level = -1;    // test hook: k_level_resolve leaves one candidate of this level undecided
  bool debug_wait_rerun = false; // test hook: the ticketed repeat of that launch runs into the same hook
  bool debug_call_stride = false; // test hook: the sparse call log of step-3 builds on any configuration
  int resolve_tickets = 0;       // 1: every resolve launch takes its workgroup indices from start tickets (default: only
                                 // the repeat of a launch whose bounded wait ran out)
  float gate_margin = 1e-4f;     // band in which the slope gate is left to the host's libm
  int debug_stitch_cap = 0;      // test hook: first row capacity of the exchange's record and edge buffers (0: the default)
  double comm_wait_seconds = 20.0;  // in-process exchange transport: the longest wait for the other ranks (a cap)
  std::unique_ptr<BfsBuffers> bfs;
  std::string bfs_fallback_reason;
  // map points inside the queries of the level kernels of the last device build (instrumentation;
  // counted per committed level, so discarded launches count nothing)
  uint64_t lv_hits_sample = 0, lv_hits_spec = 0;
  uint64_t lv_start_known = 0;  // speculative parent edges of the last device build that took their first disc as known
  TrgStats stats{};

  // goal state (trg.h:121-126)
  int goal_node = -1;
  bool goal_known = false;
  float goal_pose2d[2] = {0, 0};

  TrgStatus fail(TrgStatus s, const std::string &m) {
    err = m;
    return s;
  }
};

namespace {

#define HIPCHK(e, expr)                                                                   \
  do {                                                                                    \
    hipError_t _err = (expr);                                                             \
    if (_err != hipSuccess) {                                                             \
      return (e)->fail(TRG_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_err)); \
    }                                                                                     \
  } while (0)

// The frame of every C entry that takes an engine: the engine is there (ENGINE), it has a device and that device is
// current (DEVICE), and body() runs behind the exception ladder of abi_frame.h with `call` as the message's prefix.
enum EntryNeed { ENGINE, DEVICE };
template <typename Body>
TrgStatus entry(TrgEngine *e, const char *call, EntryNeed need, Body body) {
  if (!e) return TRG_ERR_INVALID_ARG;
  return abi_guard(call, [e](TrgStatus s, const std::string &m) { return e->fail(s, m); }, [&]() -> TrgStatus {
    if (need == DEVICE) {
      if (!e->device_ok) return e->fail(TRG_ERR_DEVICE, "engine has no usable device");
      if (hipSetDevice(e->device) != hipSuccess) return e->fail(TRG_ERR_DEVICE, "hipSetDevice failed");
    }
    return body();
  });
}

// growth with head-room for arrays that creep up from build to build (keep: the contents move along)
TrgStatus ensure_bytes(TrgEngine *e, DevArr &a, size_t need, bool keep = false) {
  if (a.p && a.bytes >= need) return TRG_OK;
  DevArr grown;
  HIPCHK(e, grown.reserve(std::max(need, a.bytes + a.bytes / 2)));
  if (keep && a.p && a.bytes) {
    hipError_t he = hipMemcpy(grown.p, a.p, a.bytes, hipMemcpyDeviceToDevice);
    if (he != hipSuccess) return e->fail(TRG_ERR_DEVICE, std::string("grow copy: ") + hipGetErrorString(he));
  }
  std::swap(a, grown);  // (the old block goes with `grown`)
  return TRG_OK;
}
TrgStatus ensure_all(TrgEngine *e, std::initializer_list<std::pair<DevArr *, size_t>> need) {
  for (const auto &n : need) {
    const TrgStatus st = ensure_bytes(e, *n.first, n.second);
    if (st != TRG_OK) return st;
  }
  return TRG_OK;
}

QueryParams qparams(const TrgEngine *e) {
  QueryParams q;
  q.robot_size = e->prm.robot_size;
  q.height_threshold = e->prm.height_threshold;
  q.collision_threshold = e->prm.collision_threshold;
  q.expand_dist = e->prm.expand_dist;
  q.sample_num = e->prm.sample_num;
  q.core_x0 = e->core[0];
  q.core_y0 = e->core[1];
  q.core_x1 = e->core[2];
  q.core_y1 = e->core[3];
  q.gate_margin = e->gate_margin;
  return q;
}

inline float key_to_float(unsigned k) {
  unsigned b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float f;
  memcpy(&f, &b, 4);
  return f;
}

#include "trg_engine_map.ipp"

// ---- sampler table -----------------------------------------------------------------------------
TrgStatus ensure_sampler(TrgEngine *e, const TrgSampler *smp) {
  TrgSampler want = smp ? *smp : e->sampler;
  if (want.table_bits < 2 || want.table_bits > 20) want.table_bits = 16;
  e->sampler = want;
  if (e->table_bits_dev == want.table_bits && e->d_cos) return TRG_OK;
  const size_t n = (size_t)1 << want.table_bits;
  e->cos_t.resize(n);
  e->sin_t.resize(n);
  for (size_t k = 0; k < n; ++k) {
    // the reference's `float angle = distr_(gen_) * 2 * M_PI; cos(angle), sin(angle)` (trg.cpp:395-397)
    float u = (float)k / (float)n;
    float angle = u * 2 * M_PI;
    e->cos_t[k] = cos(angle);
    e->sin_t[k] = sin(angle);
  }
  e->table_bits_dev = 0;
  e->d_cos.release();  // (a table of another size is allocated afresh, a smaller one too)
  e->d_sin.release();
  HIPCHK(e, e->d_cos.ensure(n));
  HIPCHK(e, e->d_sin.ensure(n));
  HIPCHK(e, hipMemcpy(e->d_cos, e->cos_t.data(), n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(e->d_sin, e->sin_t.data(), n * sizeof(float), hipMemcpyHostToDevice));
  e->table_bits_dev = want.table_bits;
  return TRG_OK;
}

inline uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
inline uint32_t sample_hash(uint32_t seed, uint32_t epoch, uint32_t id, uint32_t trial) {
  uint32_t h = fmix32(seed ^ 0x9E3779B9u);
  h = fmix32(h + epoch * 0x9E3779B9u + 0x7F4A7C15u);
  h = fmix32(h + id * 0x85EBCA6Bu + 0x165667B1u);
  h = fmix32(h + trial * 0xC2B2AE35u + 0x27D4EB2Fu);
  return h;
}
inline float sampler_uniform(const TrgEngine *e, uint32_t k) {
  uint32_t h = sample_hash(e->sampler.seed, e->epoch, 0xFFFFFFFFu, k);
  return (float)(h >> 8) * (1.0f / 16777216.0f);
}

#include "trg_engine_probe.ipp"

// ---- graph state helpers -----------------------------------------------------------------------
// The one commit point: every change of the global graph ends here.  `fresh` names the views the caller has just
// brought up to date; every other view is stale from here on, until its ensure_* is next asked for it.  The stitched
// rows and the cost field's node map belong to the graph that was (update_graph composes a new map afterwards).
void graph_changed(TrgEngine *e, std::initializer_list<TrgEngine::GraphView> fresh) {
  e->graph_version++;
  for (const auto v : fresh) e->view_stamp[v] = e->graph_version;
  e->stitched_edges = 0;
  e->csr_stitched.clear();
  e->field_map.state = NodeMap::NONE;
  e->tiled_map.state = NodeMap::NONE;
}

void reset_graph_global(TrgEngine *e) {
  e->nx.clear();
  e->ny.clear();
  e->nz.clear();
  e->nstate.clear();
  e->ncid.clear();
  e->next_cid = 0;
  e->order_map.clear();
  e->edges.reset(0);
  e->node_id = 0;
  e->kd.clear();
  e->kd_insert_order.clear();
  e->goal_node = -1;
  // (the empty pool, order and tree are those of the empty graph; the grid and the CSR still hold the old one)
  graph_changed(e, {TrgEngine::VIEW_POOL, TrgEngine::VIEW_KD_ORDER, TrgEngine::VIEW_KD});
}

// the node map's keys in iteration order, whichever representation is current
void node_map_order(const TrgEngine *e, std::vector<int> &out) {
  if (e->history_in_sim) {
    e->nodes_sim.iteration_order(out);
  } else {
    out.clear();
    out.reserve(e->order_map.size());
    for (auto &kv : e->order_map) out.push_back(kv.first);
  }
}
// rebuild the real container exactly as cleanGraph left it: new_nodes[new_id] for the dense new ids,
// then nodes = new_nodes (trg.cpp:502, 526)
void ensure_real_map(TrgEngine *e) {
  if (!e->history_in_sim) return;
  std::unordered_map<int, int> fresh;
  const int n = (int)e->nodes_sim.size();
  for (int k = 0; k < n; ++k) fresh[k] = k;
  e->order_map = std::move(fresh);
  e->history_in_sim = false;
}

void grid_rebuild(TrgEngine *e) {
  const DevMap &m = e->gmap;
  float x0 = m.bounds[0], y0 = m.bounds[1], x1 = m.bounds[2], y1 = m.bounds[3];
  for (size_t i = 0; i < e->nx.size(); ++i) {
    x0 = std::min(x0, e->nx[i]);
    x1 = std::max(x1, e->nx[i]);
    y0 = std::min(y0, e->ny[i]);
    y1 = std::max(y1, e->ny[i]);
  }
  const float pad = e->prm.expand_dist * 2 + e->prm.robot_size;
  float cell = e->prm.robot_size > 0 ? e->prm.robot_size : 0.3f;
  while (((double)(x1 - x0 + 2 * pad) / cell + 5) * ((double)(y1 - y0 + 2 * pad) / cell + 5) > 128e6)
    cell *= 2;
  e->grid.reset(x0 - pad, y0 - pad, x1 + pad, y1 + pad, cell);
  for (size_t i = 0; i < e->nx.size(); ++i) e->grid.insert(e->nx[i], e->ny[i]);
}

// bring the reference-shaped kd replica in sync with the node set (lazy: the replay only needs it
// for ties and for step 3; queries need it for hit order)
// after a device build the node-tree refill order (the node map's iteration order, trg.cpp:528-530)
// is derived on demand
void ensure_kd_order(TrgEngine *e) {
  if (e->current(TrgEngine::VIEW_KD_ORDER)) return;
  node_map_order(e, e->kd_insert_order);
  e->view_stamp[TrgEngine::VIEW_KD_ORDER] = e->graph_version;
}

void kd_sync(TrgEngine *e) {
  ensure_kd_order(e);
  if (!e->current(TrgEngine::VIEW_KD)) {
    e->kd.clear();
    e->view_stamp[TrgEngine::VIEW_KD] = e->graph_version;
  }
  while (e->kd.size() < e->kd_insert_order.size()) {
    const int id = e->kd_insert_order[e->kd.size()];
    e->kd.insert(e->nx[id], e->ny[id], id);
  }
}

int add_node_host(TrgEngine *e, float x, float y, float z, int state) {
  const int id = e->node_id;
  e->nx.push_back(x);
  e->ny.push_back(y);
  e->nz.push_back(z);
  e->nstate.push_back(state);
  e->ncid.push_back(e->next_cid++);
  // graph.nodes[node_id] = node (trg.cpp:248): into whichever representation of the container is current
  // (after a device build or a cleanGraph the keys are dense and ascending: the O(1) replica serves)
  if (e->history_in_sim) {
    e->nodes_sim.insert_next();
  } else {
    e->order_map[id] = id;
  }
  e->kd_insert_order.push_back(id);
  e->grid.insert(x, y);
  e->edges.grow_nodes(e->nx.size());
  e->node_id++;
  e->stats.created_nodes++;
  return id;
}

// nearest existing node exactly as kd_nearest2 on node_tree would answer (trg.cpp:408-409)
int nearest_node(TrgEngine *e, float qx, float qy) {
  bool tie = false;
  int s = e->grid.nearest(qx, qy, &tie);
  if (tie) {
    e->stats.nn_ties++;
    kd_sync(e);
    s = e->kd.nearest(qx, qy);
  }
  return s;
}

#include "trg_engine_replay.ipp"

#include "trg_engine_clean.ipp"

}  // namespace

#include "trg_engine_bfs.inc"

namespace {
// host-side edge pool / node grid rebuilt from the CSR after a device build (lazy)
void ensure_pool(TrgEngine *e) {
  if (e->current(TrgEngine::VIEW_POOL)) return;
  const Csr &g = e->csr_global;
  const size_t V = g.state.size();
  std::vector<int> offs(g.rowptr.data(), g.rowptr.data() + V + 1);
  e->edges.reset(0);
  e->edges.alloc_rows(offs);
  parallel_ranges(V, [&](size_t i0, size_t i1) {
    const size_t a = (size_t)offs[i0], b = (size_t)offs[i1];
    if (b > a) {
      memcpy(e->edges.dst.data() + a, g.col.data() + a, (b - a) * sizeof(int));
      memcpy(e->edges.w.data() + a, g.w.data() + a, (b - a) * sizeof(float));
      memcpy(e->edges.dist.data() + a, g.dist.data() + a, (b - a) * sizeof(float));
    }
    e->edges.link_rows(offs, i0, i1);
  });
  e->view_stamp[TrgEngine::VIEW_POOL] = e->graph_version;
}
void ensure_host_grid(TrgEngine *e) {
  if (e->current(TrgEngine::VIEW_GRID)) return;
  grid_rebuild(e);
  e->view_stamp[TrgEngine::VIEW_GRID] = e->graph_version;
}
// the commit of the host paths (host build, update_graph, load_json): pool, grid and insertion order are the
// caller's work, the CSR is taken from the pool here
void host_graph_changed(TrgEngine *e) {
  snapshot_csr(e, e->csr_global);
  graph_changed(e, {TrgEngine::VIEW_POOL, TrgEngine::VIEW_GRID, TrgEngine::VIEW_KD_ORDER, TrgEngine::VIEW_CSR});
}
// csr_global from the pool; false: neither is of the current graph.  (The size test covers an update_graph that
// failed midway: it has added nodes under an unchanged version.)
bool ensure_csr_global(TrgEngine *e) {
  if (e->current(TrgEngine::VIEW_CSR) && e->csr_global.state.size() == e->nx.size()) return true;
  if (!e->current(TrgEngine::VIEW_POOL)) return false;
  snapshot_csr(e, e->csr_global);
  e->view_stamp[TrgEngine::VIEW_CSR] = e->graph_version;
  return true;
}
// the cleaned CSR of the last device build while it is the current graph's
const BfsBuffers *dev_csr(const TrgEngine *e) {
  const BfsBuffers *bb = e->bfs.get();
  return e->current(TrgEngine::VIEW_DEV_CSR) && bb && bb->xyz2.p && bb->rowptr_new.p ? bb : nullptr;
}

// The cleaned global graph of this engine on the device, for the cost field and the stitch: the device build's
// arrays in place while they are the current graph's, else the engine's upload of csr_global and nstate.
struct DevGraph {
  const int *rowptr = nullptr, *col = nullptr;
  const float *w = nullptr, *dist = nullptr;
  const int *state = nullptr;
  const float *xyz = nullptr;
  int V = 0, E = 0;
  bool dev_build = false;
};
enum { DEV_NODES = 1, DEV_EDGES = 2 };

// `need`: the parts (DEV_NODES | DEV_EDGES) the caller will read.  A part of the upload is copied when it is asked for
// and is not of this graph_version (the size test is ensure_csr_global's: an update_graph that failed midway).  One
// that is current is neither copied nor regrown, so what was handed out stays good for as long as the version does.
// need == 0 copies nothing and hands out what is current, null for the rest: "are these still the graph's arrays".
TrgStatus ensure_dev_graph(TrgEngine *e, int need, DevGraph *g) {
  *g = DevGraph{};
  if (need) (void)ensure_csr_global(e);  // (false: neither the CSR nor the pool is current, the old rows stay in place)
  const Csr &c = e->csr_global;
  const int V = g->V = (int)c.state.size(), E = g->E = (int)c.col.size();
  if (const BfsBuffers *bb = dev_csr(e)) {
    *g = {bb->rowptr_new.as<int>(), bb->col2.as<int>(), bb->w2.as<float>(), bb->dist2.as<float>(),
          bb->state2.as<int>(), bb->xyz2.as<float>(), V, E, true};
    return TRG_OK;
  }
  DevGraphUpload &up = e->dev_up;
  struct Copy { DevArr &a; const void *src; size_t bytes; };
  // one part: current, or copied now when `need` names it (stale and not asked for: left alone, *current false)
  const auto part = [&](TrgEngine::GraphView view, int flag, long long &have, long long want,
                        std::initializer_list<Copy> copies, bool *current) -> TrgStatus {
    *current = e->view_stamp[view] == e->graph_version && have == want;
    if (*current || !(need & flag)) return TRG_OK;
    e->view_stamp[view] = 0;
    for (const Copy &k : copies)
      if (const TrgStatus st = ensure_bytes(e, k.a, k.bytes + 16); st != TRG_OK) return st;
    for (const Copy &k : copies)
      if (k.bytes) HIPCHK(e, hipMemcpyAsync(k.a.p, k.src, k.bytes, hipMemcpyHostToDevice, e->s_main));
    have = want;
    e->view_stamp[view] = e->graph_version;
    *current = true;
    return TRG_OK;
  };
  static const int no_rows[1] = {0};  // the row pointers of the empty graph
  const size_t nv = (size_t)V, ne = (size_t)E;
  bool nodes = false, edges = false;
  TrgStatus st = part(TrgEngine::VIEW_UP_NODES, DEV_NODES, up.nodes_of, V,
                      {{up.xyz, c.xyz.data(), nv * 12}, {up.state, e->nstate.data(), std::min(nv, e->nstate.size()) * 4}},
                      &nodes);
  if (st == TRG_OK)
    st = part(TrgEngine::VIEW_UP_EDGES, DEV_EDGES, up.edges_of, (long long)V << 32 | E,
              {{up.rowptr, c.rowptr.empty() ? no_rows : c.rowptr.data(), (nv + 1) * 4},
               {up.col, c.col.data(), ne * 4}, {up.w, c.w.data(), ne * 4}, {up.dist, c.dist.data(), ne * 4}},
              &edges);
  if (st != TRG_OK) return st;
  if (nodes) {
    g->xyz = up.xyz.as<float>();
    g->state = up.state.as<int>();
  }
  if (edges) {
    g->rowptr = up.rowptr.as<int>();
    g->col = up.col.as<int>();
    g->w = up.w.as<float>();
    g->dist = up.dist.as<float>();
  }
  return TRG_OK;
}
}  // namespace

// =================================== C ABI ======================================================
// Every entry reads the same way: the argument checks that need no engine, then entry() around a named function of
// this namespace (the probes, the planner, the fields, the stitch and the exchange follow in their own files).  No
// code calls a trg_engine_* symbol: what two entries share is a function here.
namespace {

TrgStatus create_engine(const TrgParams *params, int device, TrgEngine **out) {
  TrgEngine *e = new TrgEngine();
  e->prm = *params;
  e->device = device;
  *out = e;  // handed out even on failure so the caller can read last_error
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    return e->fail(TRG_ERR_DEVICE, "no HIP device visible: the TRG engine has no CPU fallback");
  }
  if (device < 0 || device >= ndev) return e->fail(TRG_ERR_INVALID_ARG, "bad device ordinal");
  HIPCHK(e, hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(e, hipGetDeviceProperties(&prop, device));
  e->arch = prop.gcnArchName;
  if (e->arch.rfind("gfx950", 0) != 0) {
    return e->fail(TRG_ERR_DEVICE, "kernels are built for gfx950 only, device is " + e->arch);
  }
  HIPCHK(e, hipDeviceGetAttribute(&e->wall_clock_khz, hipDeviceAttributeWallClockRate, device));
  if (e->wall_clock_khz <= 0) return e->fail(TRG_ERR_DEVICE, "the device reports no wall-clock rate");
  // (whatever exists when one of these fails is released by trg_engine_destroy)
  HIPCHK(e, e->s_main.create());
  // the deferred stream at the main stream's priority (the lowest leaves a longer tail after the loop:
  // measured 0.5 ms slower)
  HIPCHK(e, e->s_edge.create_with_priority(0));
  HIPCHK(e, e->s_aux.create());
  HIPCHK(e, e->d_ctr.ensure(COUNTER_SHARDS));
  HIPCHK(e, hipMemset(e->d_ctr, 0, COUNTER_SHARDS * sizeof(DeviceCounters)));
  HIPCHK(e, e->d_bounds.ensure(4));
  // step 3 of expandGraph is compiled in or out by this fp comparison (trg.cpp:429)
  e->step3 = (e->prm.expand_dist - e->prm.robot_size) < 0.25 * e->prm.expand_dist;
  e->bfs.reset(new BfsBuffers());
  e->uploader.reset(new Uploader());
  e->device_ok = true;
  if (const char *env = getenv("TRG_REPLAY")) e->use_device_bfs = std::string(env) != "host";
  reset_graph_global(e);
  return TRG_OK;
}

TrgStatus set_global_map(TrgEngine *e, const float *xyz, size_t n, size_t stride) {
  if ((n && !xyz) || stride < 3) return e->fail(TRG_ERR_INVALID_ARG, "bad map arguments");
  auto t0 = Clock::now();
  TrgStatus st = upload_and_build(e, e->gmap, xyz, n, stride);
  e->stats.ms_set_map_total = ms_since(t0);
  return st;
}

TrgStatus set_global_map_device(TrgEngine *e, const float *d_xyz, size_t n, size_t stride) {
  if ((n && !d_xyz) || stride < 3) return e->fail(TRG_ERR_INVALID_ARG, "bad map arguments");
  if (n == 0) {
    e->gmap.n = 0;
    e->gmap.valid = false;
    return TRG_OK;
  }
  return build_map(e, e->gmap, d_xyz, n, stride);
}

TrgStatus set_local_map(TrgEngine *e, const float start_xy[2], const float *xyz, size_t n, size_t stride) {
  if (!start_xy || (n && !xyz) || stride < 3) return e->fail(TRG_ERR_INVALID_ARG, "bad arguments");
  e->local_root[0] = start_xy[0];
  e->local_root[1] = start_xy[1];
  TrgStatus st = upload_and_build(e, e->lmap, xyz, n, stride);
  if (st != TRG_OK) return st;
  return set_local_graph(e);
}

TrgStatus reset_map(TrgEngine *e, TrgKind kind) {
  DevMap *m = pick_map(e, kind);
  m->top_wait();  // (a helper preparing the map's tie-break structures still reads it)
  m->n = 0;
  m->valid = false;
  return TRG_OK;
}

TrgStatus reset_graph(TrgEngine *e, TrgKind kind) {
  if (kind == TRG_KIND_LOCAL) {
    e->local_nodes.clear();
    e->local_map.clear();
  } else {
    ensure_real_map(e);
    reset_graph_global(e);
    e->csr_global.clear();
    field_release(e);
  }
  return TRG_OK;
}

TrgStatus init_graph(TrgEngine *e, const float start_xyz[3], const TrgSampler *sampler) {
  if (!start_xyz) return e->fail(TRG_ERR_INVALID_ARG, "null start");
  if (!e->gmap.valid || e->gmap.n == 0) return e->fail(TRG_ERR_NO_MAP, "Map is empty");
  auto t_total = Clock::now();
  TrgStatus st = ensure_sampler(e, sampler);
  if (st != TRG_OK) return st;
  // per-build stats (map-index figures are kept)
  {
    TrgStats keep = e->stats;
    e->stats = TrgStats();
    e->stats.map_points = keep.map_points;
    e->stats.ms_index_build = keep.ms_index_build;
    e->stats.bytes_index_build = keep.bytes_index_build;
    e->stats.ms_set_map_total = keep.ms_set_map_total;
  }
  // (in the main stream: it is non-blocking, a plain memset would not be ordered with the kernels)
  HIPCHK(e, hipMemsetAsync(e->d_ctr, 0, COUNTER_SHARDS * sizeof(DeviceCounters), e->s_main));
  e->lv_hits_sample = e->lv_hits_spec = e->lv_start_known = 0;
  if (!e->use_device_bfs) ensure_real_map(e);
  MapOrderSim sim_before;  // container history as of before this build (for the fallback)
  if (e->use_device_bfs) {
    if (!e->history_in_sim) e->nodes_sim.adopt_bucket_state(e->order_map);
    sim_before = e->nodes_sim;
  }
  reset_graph_global(e);
  e->epoch = e->epoch_base;
  e->calls.clear();
  e->pending_calls.clear();
  e->csr_pre.clear();

  // root seeding, trg.cpp:44-56
  e->root_pos[0] = start_xyz[0];
  e->root_pos[1] = start_xyz[1];
  float rx = e->root_pos[0], ry = e->root_pos[1], rz = 0.0f;
  rx = rx + e->prm.expand_dist;
  int cnt = 0;
  for (;;) {
    float xy[2] = {rx, ry};
    int32_t flag = 1;
    st = collision_sync(e, e->gmap, e->prm.collision_threshold, xy, 1, &flag, nullptr, nullptr);
    if (st != TRG_OK) return st;
    if (!(rx >= e->core[0] && rx < e->core[2] && ry >= e->core[1] && ry < e->core[3])) flag = 1;
    if (!flag) {
      int32_t found = 0;
      st = nearest_z_sync(e, e->gmap, xy, 1, &rz, &found);
      if (st != TRG_OK) return st;
      break;
    }
    if (cnt > 100) return e->fail(TRG_ERR_NO_ROOT, "Failed to generate root node");
    const float u0 = sampler_uniform(e, 2 * cnt), u1 = sampler_uniform(e, 2 * cnt + 1);
    rx = rx + e->prm.expand_dist * u0;
    ry = ry + e->prm.expand_dist * u1;
    cnt++;
  }

  if (e->use_device_bfs) {
    st = build_graph_device(e, rx, ry, rz);
    if (st == TRG_OK) {
      read_counters(e);
      e->stats.used_device_bfs = 1;
      e->stats.ms_init_graph_total = ms_since(t_total);
      return TRG_OK;
    }
    if (e->bfs_fallback_reason.empty()) return st;
    // the device path declined (capacity, or an exact fp32 tie whose winner depends on the
    // reference kd-tree's shape): redo the build with the host replay, which handles those
    e->stats.bfs_fallbacks++;
    // (kernels of the abandoned attempt may still be in flight: the streams do not synchronise with
    // plain copies / memsets)
    HIPCHK(e, hipStreamSynchronize(e->s_main));
    HIPCHK(e, hipStreamSynchronize(e->s_edge));
    HIPCHK(e, hipMemset(e->d_ctr, 0, COUNTER_SHARDS * sizeof(DeviceCounters)));
    e->lv_hits_sample = e->lv_hits_spec = e->lv_start_known = 0;
    e->nodes_sim = sim_before;
    ensure_real_map(e);
    reset_graph_global(e);  // (the abandoned attempt may have written the node arrays: clean_and_fetch)
  }

  grid_rebuild(e);  // (empty, over the map's extent: add_node_host fills it, host_graph_changed names it)
  add_node_host(e, rx, ry, rz, TRG_NODE_VALID);
  st = expand_bfs(e, e->node_id - 1);
  if (st != TRG_OK) return st;
  auto t_fin = Clock::now();
  st = flush_pending(e, true);
  if (st != TRG_OK) return st;
  apply_calls(e, 0);
  if (e->keep_preclean) snapshot_csr(e, e->csr_pre);
  clean_graph(e);
  host_graph_changed(e);
  e->stats.ms_finalize_host = ms_since(t_fin);
  read_counters(e);
  e->stats.ms_init_graph_total = ms_since(t_total);
  return TRG_OK;
}

TrgStatus set_option(TrgEngine *e, const char *key, const char *value) {
  enum Kind {
    INT,             // atoi
    BOOL,            // anything but "0" is true
    ZERO_OR_ONE,     // -> bool, nothing else accepted
    HOST_OR_DEVICE,  // -> bool "device", nothing else accepted
    FLOAT,           // atof
    POSITIVE_DOUBLE  // strtod, > 0 ("inf" included)
  };
  const struct {
    const char *name;
    Kind kind;
    void *target;
  } options[] = {
      {"replay", HOST_OR_DEVICE, &e->use_device_bfs},
      {"defer_overlap", ZERO_OR_ONE, &e->defer_overlap},
      {"tail_overlap", ZERO_OR_ONE, &e->tail_overlap},
      {"tail_early_copy", ZERO_OR_ONE, &e->tail_early_copy},
      {"known_start_disc", ZERO_OR_ONE, &e->known_start_disc},
      {"lazy_tie_repair", ZERO_OR_ONE, &e->lazy_tie_repair},
      {"tie_inplace", BOOL, &e->tie_inplace},
      {"keep_preclean", BOOL, &e->keep_preclean},
      {"resolve_tickets", INT, &e->resolve_tickets},
      // measurement knob: cost-field bucket width in mean edge costs ("inf": Bellman-Ford)
      {"field_delta_scale", POSITIVE_DOUBLE, &e->field_delta_scale},
      // the safety factor of the planner and of the cost fields from the next call on (every cache of edge costs is
      // stamped with its bits; the risk fields do not know it)
      {"safety_factor", FLOAT, &e->prm.safety_factor},
      {"debug_gate_margin", FLOAT, &e->gate_margin},
      {"debug_tie_every", INT, &e->debug_tie_every},
      {"debug_spec_bound", INT, &e->debug_spec_bound},
      {"debug_stall_level", INT, &e->debug_stall_level},
      {"debug_lookback_level", INT, &e->debug_lookback_level},
      {"debug_fallback_level", INT, &e->debug_fallback_level},
      {"debug_call_stride", BOOL, &e->debug_call_stride},
      {"debug_order_run_cap", INT, &e->debug_order_run_cap},
      {"debug_wait_rerun", BOOL, &e->debug_wait_rerun},
      {"debug_stitch_cap", INT, &e->debug_stitch_cap},
      {"comm_wait_seconds", POSITIVE_DOUBLE, &e->comm_wait_seconds},
  };
  const std::string k(key), v(value);
  for (const auto &o : options) {
    if (k != o.name) continue;
    switch (o.kind) {
      case INT:
        *(int *)o.target = atoi(value);
        break;
      case BOOL:
        *(bool *)o.target = v != "0";
        break;
      case ZERO_OR_ONE:
        if (v != "0" && v != "1") return e->fail(TRG_ERR_INVALID_ARG, k + " must be 0 or 1");
        *(bool *)o.target = v == "1";
        break;
      case HOST_OR_DEVICE:
        if (v != "host" && v != "device") return e->fail(TRG_ERR_INVALID_ARG, k + " must be host or device");
        *(bool *)o.target = v == "device";
        break;
      case FLOAT:
        *(float *)o.target = (float)atof(value);
        break;
      case POSITIVE_DOUBLE: {
        const double d = strtod(value, nullptr);
        if (!(d > 0.0)) return e->fail(TRG_ERR_INVALID_ARG, k + " must be > 0");
        *(double *)o.target = d;
        break;
      }
    }
    return TRG_OK;
  }
  return e->fail(TRG_ERR_INVALID_ARG, "unknown option " + k);
}

TrgStatus set_tile(TrgEngine *e, const float core_xyxy[4], uint32_t epoch) {
  if (core_xyxy) {
    for (int i = 0; i < 4; ++i) e->core[i] = core_xyxy[i];
  } else {
    e->core[0] = e->core[1] = -INFINITY;
    e->core[2] = e->core[3] = INFINITY;
  }
  e->epoch_base = epoch;
  return TRG_OK;
}

TrgStatus is_frontier_batch(TrgEngine *e, const float *xy, size_t m, int32_t *flag);  // (with the probes, below)

TrgStatus update_graph(TrgEngine *e) {
  if (!e->gmap.valid) return e->fail(TRG_ERR_NO_MAP, "Map is empty");
  TrgStatus st = ensure_sampler(e, nullptr);
  if (st != TRG_OK) return st;
  e->epoch++;
  e->view_stamp[TrgEngine::VIEW_DEV_CSR] = 0;  // dropped before anything can fail (the cost field's retained solve)
  const size_t nodes_before = e->nx.size();
  const NodeMap::State map_before = e->field_map.state, tiled_map_before = e->tiled_map.state;
  e->field_map.state = e->tiled_map.state = NodeMap::NONE;  // (an update that fails leaves no map)
  const bool trace_up = getenv("TRG_TIMING") != nullptr;
  auto t_up = Clock::now();
  auto lap_up = [&](const char *what) {
    if (trace_up) fprintf(stderr, "[trg update] %-28s %8.3f ms\n", what, ms_since(t_up));
  };
  ensure_pool(e);
  ensure_host_grid(e);
  ensure_kd_order(e);  // nodes created below are appended to the existing insertion order
  e->calls.clear();
  e->pending_calls.clear();
  lap_up("host structures ready");

  // per local node: invalidate / keep frontier / revalidate (trg.cpp:464-481)
  const size_t L = e->local_nodes.size();
  std::vector<float> xy(2 * L);
  for (size_t i = 0; i < L; ++i) {
    xy[2 * i] = e->nx[e->local_nodes[i]];
    xy[2 * i + 1] = e->ny[e->local_nodes[i]];
  }
  std::vector<int32_t> col(L, 0), fro(L, 0);
  if (L) {
    st = collision_sync(e, e->lmap, e->prm.update_collision_threshold, xy.data(), L, col.data(),
                        nullptr, nullptr);
    if (st != TRG_OK) return st;
    st = is_frontier_batch(e, xy.data(), L, fro.data());
    if (st != TRG_OK) return st;
  }
  std::vector<int> expand_queue;
  for (size_t i = 0; i < L; ++i) {
    const int id = e->local_nodes[i];
    const float px = e->nx[id], py = e->ny[id];
    if (norm2f(px - e->local_root[0], py - e->local_root[1]) > 2.0 * e->prm.expand_dist) {
      if (col[i] || e->edges.deg[id] < 1) {
        e->nstate[id] = TRG_NODE_INVALID;
        continue;
      }
    }
    if (fro[i] && e->nstate[id] == TRG_NODE_FRONTIER) {
      e->nstate[id] = TRG_NODE_FRONTIER;
      expand_queue.push_back(id);
      continue;
    }
    expand_queue.push_back(id);
    e->nstate[id] = TRG_NODE_VALID;
  }
  // isFrontier looked at the node set as it stood; expansions below mutate it, and the reference
  // evaluates isFrontier lazily inside the same loop BEFORE any expansion, so this order is exact.
  // The GPU results of a root (its samples and their speculative parent edges) depend on the map
  // and on (seed, epoch, id) only, so they are fetched for all roots in bulk; the expansions
  // themselves are replayed one root after the other, as the reference runs them.  wireEdge's
  // dedupe does not influence any node decision, so the logged calls are evaluated and applied once
  // at the end, in program order (first successful call per pair wins).
  lap_up("local nodes classified");
  st = ensure_chunks(e);
  if (st != TRG_OK) return st;
  for (size_t g0 = 0; g0 < expand_queue.size(); g0 += TrgEngine::CHUNK_MAX) {
    const int cnt = (int)std::min<size_t>(TrgEngine::CHUNK_MAX, expand_queue.size() - g0);
    st = submit_nodes(e, e->root_chunk, expand_queue.data() + g0, cnt);
    if (st != TRG_OK) return st;
    st = wait_chunk(e, e->root_chunk);
    if (st != TRG_OK) return st;
    for (int i = 0; i < cnt; ++i) {
      st = expand_bfs(e, expand_queue[g0 + i], &e->root_chunk, i);
      if (st != TRG_OK) return st;
    }
  }
  lap_up("roots expanded");
  st = flush_pending(e, true);
  if (st != TRG_OK) return st;
  lap_up("deferred edges evaluated");
  std::vector<int32_t> member_old;  // local-graph membership of the nodes as they are now (positions do not change)
  st = local_membership(e, member_old);
  if (st != TRG_OK) return st;
  apply_calls(e, 0);
  lap_up("calls applied");
  if (e->keep_preclean) snapshot_csr(e, e->csr_pre);
  clean_graph(e);
  lap_up("cleanGraph");
  host_graph_changed(e);
  lap_up("CSR snapshot");
  read_counters(e);
  std::vector<int32_t> member_new(e->nx.size(), 0);
  for (size_t k = 0; k < member_new.size() && k < e->last_new2old.size(); ++k)
    member_new[k] = member_old[e->last_new2old[k]];
  st = set_local_graph(e, &member_new);
  lap_up("setLocalGraph");
  // the node maps of the retained solves through this update (node_map.h)
  for (const auto &[map, before] : {std::pair<NodeMap *, NodeMap::State>{&e->field_map, map_before},
                                    std::pair<NodeMap *, NodeMap::State>{&e->tiled_map, tiled_map_before}})
    if (st == TRG_OK && before != NodeMap::NONE) {
      map->state = before;
      node_map_compose(*map, e->last_new2old, nodes_before);
    }
  return st;  // cleanGraph(true) -> setLocalGraph (trg.cpp:532-534)
}

TrgStatus export_csr(TrgEngine *e, TrgKind kind, TrgCsrView *out) {
  Csr *c = nullptr;
  if (kind == TRG_KIND_GLOBAL) {
    c = &e->csr_global;
    (void)ensure_csr_global(e);  // (false: neither the CSR nor the pool is current, the old rows stay in place)
  } else if (kind == TRG_KIND_PRECLEAN) {
    c = &e->csr_pre;
  } else if (kind == TRG_KIND_STITCHED) {
    c = &e->csr_stitched;
    const TrgStatus fs = stitch_fetch(e);
    if (fs != TRG_OK) return fs;
  } else {
    // local graph: the global rows of the local member nodes
    c = &e->csr_local;
    ensure_pool(e);
    Csr full;
    snapshot_csr(e, full);
    c->clear();
    c->rowptr.push_back(0);
    for (int id : e->local_nodes) {
      c->xyz.append(full.xyz.begin() + 3 * id, full.xyz.begin() + 3 * id + 3);
      c->state.push_back(full.state[id]);
      c->cid.push_back(id);  // for the local view: the node's global id
      for (int k = full.rowptr[id]; k < full.rowptr[id + 1]; ++k) {
        c->col.push_back(full.col[k]);
        c->w.push_back(full.w[k]);
        c->dist.push_back(full.dist[k]);
      }
      c->rowptr.push_back((int)c->col.size());
    }
  }
  if (c->rowptr.empty()) c->rowptr.push_back(0);
  out->num_nodes = (int32_t)c->state.size();
  out->num_edges = (int32_t)c->col.size();
  out->node_xyz = c->xyz.data();
  out->node_state = c->state.data();
  out->rowptr = c->rowptr.data();
  out->col = c->col.data();
  out->weight = c->w.data();
  out->dist = c->dist.data();
  out->creation_id = c->cid.data();
  return TRG_OK;
}

// ---- JSON persistence (schema of trg.cpp:130-177) ---------------------------------------------
TrgStatus save_json(TrgEngine *e, const char *path) {
  std::string p(path);
  // save_path.extension().empty() -> append ".json" (trg.cpp:135-137)
  {
    size_t slash = p.find_last_of('/');
    size_t dot = p.find_last_of('.');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) p += ".json";
  }
  std::ofstream f(p);
  if (!f) return e->fail(TRG_ERR_IO, "cannot open " + p);
  ensure_pool(e);
  // nodes/edges are listed in the node map's iteration order, like the reference
  std::vector<int> map_order;
  node_map_order(e, map_order);
  GraphJson g;
  g.nodes.reserve(map_order.size());
  for (int id : map_order) {
    g.nodes.push_back({id, {e->nx[id], e->ny[id], e->nz[id]}, e->nstate[id]});
    for (int ed = e->edges.head[id]; ed >= 0; ed = e->edges.next[ed])
      g.edges.push_back({id, e->edges.dst[ed], e->edges.w[ed], e->edges.dist[ed]});
  }
  write_graph_json(f, g);
  f.close();
  if (!f) return e->fail(TRG_ERR_IO, "write failed: " + p);
  return TRG_OK;
}

TrgStatus load_json(TrgEngine *e, const char *path) {
  if (!path) return TRG_ERR_INVALID_ARG;
  std::ifstream f(path);
  if (!f) return e->fail(TRG_ERR_IO, std::string("File not found: ") + path);
  std::stringstream ss;
  ss << f.rdbuf();
  const std::string txt = ss.str();
  GraphJson gj;
  std::string perr;
  if (!parse_graph_json(txt, gj, perr) || !validate_graph_json(gj, perr)) return e->fail(TRG_ERR_IO, perr);
  const std::vector<GraphJson::N> &nodes = gj.nodes;
  const std::vector<GraphJson::Ed> &eds = gj.edges;
  const size_t V = nodes.size();
  ensure_real_map(e);
  reset_graph_global(e);
  e->nx.assign(V, 0);
  e->ny.assign(V, 0);
  e->nz.assign(V, 0);
  e->nstate.assign(V, 0);
  e->ncid.assign(V, 0);
  e->edges.reset(V);
  for (auto &n : nodes) {
    e->nx[n.id] = n.p[0];
    e->ny[n.id] = n.p[1];
    e->nz[n.id] = n.p[2];
    e->nstate[n.id] = n.state;
    e->ncid[n.id] = n.id;
    e->order_map[n.id] = n.id;          // global_graph.nodes[id] = node_ptr, file order
    e->kd_insert_order.push_back(n.id);  // kd_insert2 in file order (trg.cpp:103)
  }
  e->node_id = (int)V;
  e->next_cid = (int)V;
  for (auto &ed : eds) e->edges.push(ed.s, ed.t, ed.w, ed.d);
  grid_rebuild(e);
  host_graph_changed(e);
  return TRG_OK;
}

// ---- probes --------------------------------------------------------------------------------------
TrgStatus is_collision_batch(TrgEngine *e, TrgKind map, float threshold, const float *xy, size_t m, int32_t *flag,
                             int32_t *cnt, int32_t *n) {
  if (m && !xy) return e->fail(TRG_ERR_INVALID_ARG, "null positions");
  return collision_sync(e, *pick_map(e, map), threshold, xy, m, flag, cnt, n);
}

TrgStatus nearest_z_batch(TrgEngine *e, TrgKind map, const float *xy, size_t m, float *z) {
  if (m && (!xy || !z)) return e->fail(TRG_ERR_INVALID_ARG, "null arguments");
  return nearest_z_sync(e, *pick_map(e, map), xy, m, z, nullptr);
}

TrgStatus edge_risk_batch(TrgEngine *e, TrgKind map, const float *p1_xyz, const float *p2_xyz, size_t m,
                          int32_t *status, int32_t *n_pts, float *weight, float *dist) {
  if (m && (!p1_xyz || !p2_xyz)) return e->fail(TRG_ERR_INVALID_ARG, "null arguments");
  return edges_sync(e, *pick_map(e, map), p1_xyz, p2_xyz, m, status, n_pts, weight, dist, true);
}

TrgStatus voxel_filter(TrgEngine *e, const float *xyz, size_t n, size_t stride, float leaf, float *out_xyz,
                       size_t *n_out, int32_t *passthrough) {
  if (!n_out || (n && (!xyz || !out_xyz))) return e->fail(TRG_ERR_INVALID_ARG, "null arguments");
  if (stride < 3) return e->fail(TRG_ERR_INVALID_ARG, "stride must be >= 3 floats");
  if (!(leaf > 0.0f)) return e->fail(TRG_ERR_INVALID_ARG, "leaf size must be positive");
  *n_out = 0;
  if (passthrough) *passthrough = 0;
  if (n == 0) return TRG_OK;
  DevBuf<float> d_in, d_out;  // (freed on every way out)
  HIPCHK(e, d_in.ensure(n * stride));
  hipError_t he = d_out.ensure(n * 3);
  if (he == hipSuccess)
    he = hipMemcpyAsync(d_in, xyz, n * stride * sizeof(float), hipMemcpyHostToDevice, e->s_main);
  int status = 0;
  size_t m = 0;
  if (he == hipSuccess) he = voxel_grid_filter(d_in, n, stride, leaf, d_out, &m, &status, e->s_main);
  if (he == hipSuccess && m)
    he = hipMemcpy(out_xyz, d_out, m * 3 * sizeof(float), hipMemcpyDeviceToHost);
  if (he != hipSuccess)
    return e->fail(TRG_ERR_DEVICE, std::string("voxel filter: ") + hipGetErrorString(he));
  *n_out = m;
  if (passthrough) *passthrough = status;
  return TRG_OK;
}

TrgStatus is_frontier_batch(TrgEngine *e, const float *xy, size_t m, int32_t *flag) {
  if (m && (!xy || !flag)) return e->fail(TRG_ERR_INVALID_ARG, "null arguments");
  // trg.cpp:780-803: check = pos + 2*robot_size*normalize(pos - local root); frontier iff no global
  // node within robot_size of check AND no local-map point within robot_size/2 of it
  // "no global node within robot_size" only asks whether the range query is empty: the node grid answers
  // that without the tree replica (building it costs O(V log V) per update); the replica is consulted
  // only for a node within rounding of the radius, where the tree's pruning decides
  ensure_host_grid(e);
  std::vector<float> chk(2 * m);
  std::vector<int> hits;
  std::vector<char> blocked(m, 0);
  for (size_t i = 0; i < m; ++i) {
    float dx = xy[2 * i] - e->local_root[0], dy = xy[2 * i + 1] - e->local_root[1];
    const float sq = dx * dx + dy * dy;
    if (sq > 0.0f) {
      const float nrm = sqrtf(sq);
      dx = dx / nrm;
      dy = dy / nrm;
    }
    const float k = 2 * e->prm.robot_size;
    chk[2 * i] = xy[2 * i] + k * dx;
    chk[2 * i + 1] = xy[2 * i + 1] + k * dy;
    int w = e->grid.ready() ? e->grid.within(chk[2 * i], chk[2 * i + 1], e->prm.robot_size) : -1;
    if (w < 0) {
      kd_sync(e);
      e->kd.range(chk[2 * i], chk[2 * i + 1], e->prm.robot_size, hits);
      w = hits.empty() ? 0 : 1;
    }
    blocked[i] = w != 0;
  }
  std::vector<int32_t> n(m, 0);
  if (e->lmap.valid && m) {
    TrgStatus st = collision_sync(e, e->lmap, 0.0f, chk.data(), m, nullptr, nullptr, n.data(), nullptr,
                                  (float)(0.5 * e->prm.robot_size));
    if (st != TRG_OK) return st;
  }
  for (size_t i = 0; i < m; ++i) flag[i] = (!blocked[i] && n[i] == 0) ? 1 : 0;
  return TRG_OK;
}

// Pose links ("Pose links"): the candidates of every pose from the node grid, then ONE collision
// batch, ONE elevation batch and ONE edge batch for all poses, and the sort per pose on the host.
TrgStatus pose_links(TrgEngine *e, const float *xy, int32_t m, float radius, int32_t cap, int32_t *link_node,
                     float *link_weight, float *link_dist, TrgPoseInfo *infos) {
  if (m < 0) return e->fail(TRG_ERR_INVALID_ARG, "m < 0");
  if (cap < 0) return e->fail(TRG_ERR_INVALID_ARG, "cap < 0");
  // wireEdge asserts dist < 2.5 * expand_dist (trg.cpp:279), the product taken in double
  if (!(radius > 0.0f) || !((double)radius < 2.5 * (double)e->prm.expand_dist))
    return e->fail(TRG_ERR_INVALID_ARG, "radius " + std::to_string(radius) + " is not a number in (0, 2.5 * expand_dist = " +
                                            std::to_string(2.5 * (double)e->prm.expand_dist) + ")");
  if (m == 0) return TRG_OK;
  if (!xy || !infos) return e->fail(TRG_ERR_INVALID_ARG, "null poses_xy or infos");
  for (int k = 0; k < m; ++k)
    if (std::isnan(xy[2 * k]) || std::isnan(xy[2 * k + 1]))
      return e->fail(TRG_ERR_INVALID_ARG, "the position of pose " + std::to_string(k) + " is not a number");
  if (!e->gmap.valid) return e->fail(TRG_ERR_NO_MAP, "no global map");
  if (e->nx.empty()) return e->fail(TRG_ERR_NO_GRAPH, "graph is empty");
  ensure_host_grid(e);
  const size_t M = (size_t)m;
  std::vector<int32_t> hit(M);
  std::vector<float> z(M);
  TrgStatus st = collision_sync(e, e->gmap, e->prm.collision_threshold, xy, M, hit.data(), nullptr, nullptr);
  if (st != TRG_OK) return st;
  if ((st = nearest_z_sync(e, e->gmap, xy, M, z.data(), nullptr)) != TRG_OK) return st;
  // a link before the sort; `eval`: its place in the edge batch, -1 for the node the pose stands on
  struct Link {
    int node, eval;
    float w, d;
  };
  std::vector<std::vector<Link>> links(M);
  std::vector<float> p1, p2;
  std::vector<int> slots;
  const int V = (int)e->nx.size();
  for (size_t k = 0; k < M; ++k) {
    infos[k] = TrgPoseInfo{hit[k] ? 1 : 0, 0, 0, z[k]};
    if (hit[k]) continue;
    const float px = xy[2 * k], py = xy[2 * k + 1];
    const auto candidate = [&](int v) {
      if (e->nstate[v] == TRG_NODE_INVALID) return;
      const float dx = px - e->nx[v], dy = py - e->ny[v];
      const float xx = dx * dx, yy = dy * dy;  // (each product rounded on its own: no contraction)
      const float d = sqrtf(xx + yy);
      if (!(d <= radius)) return;
      infos[k].n_candidates++;
      if (d == 0.0f) {
        links[k].push_back({v, -1, 0.0f, 0.0f});
        return;
      }
      links[k].push_back({v, (int)(p1.size() / 3), 0.0f, 0.0f});
      p1.insert(p1.end(), {px, py, z[k]});
      p2.insert(p2.end(), {e->nx[v], e->ny[v], e->nz[v]});
    };
    if (e->grid.ready() && e->grid.size() == (size_t)V) {
      e->grid.disc_cells(px, py, radius, slots);
      for (int v : slots) candidate(v);
    } else {
      for (int v = 0; v < V; ++v) candidate(v);
    }
  }
  const size_t n_eval = p1.size() / 3;
  std::vector<int32_t> status(n_eval);
  std::vector<float> w(n_eval), d(n_eval);
  if (n_eval && (st = edges_sync(e, e->gmap, p1.data(), p2.data(), n_eval, status.data(), nullptr, w.data(), d.data(),
                                 true)) != TRG_OK)
    return st;
  for (size_t k = 0; k < M; ++k) {
    std::vector<Link> &L = links[k];
    size_t n = 0;
    for (const Link &c : L) {
      if (c.eval >= 0 && status[c.eval] != EDGE_OK) continue;
      L[n++] = c.eval < 0 ? c : Link{c.node, c.eval, w[c.eval], d[c.eval]};
    }
    L.resize(n);
    const auto bits = [](float f) {
      uint32_t b;
      memcpy(&b, &f, sizeof b);
      return b;
    };
    std::sort(L.begin(), L.end(), [&](const Link &a, const Link &b) {
      return bits(a.d) != bits(b.d) ? bits(a.d) < bits(b.d) : a.node < b.node;
    });
    infos[k].n_links = (int32_t)n;
    for (size_t i = 0; i < std::min<size_t>(n, (size_t)cap); ++i) {
      if (link_node) link_node[k * cap + i] = L[i].node;
      if (link_weight) link_weight[k * cap + i] = L[i].w;
      if (link_dist) link_dist[k * cap + i] = L[i].d;
    }
  }
  return TRG_OK;
}

TrgStatus get_sampler_table(TrgEngine *e, float *cos_out, float *sin_out) {
  TrgStatus st = ensure_sampler(e, nullptr);
  if (st != TRG_OK) return st;
  if (cos_out) memcpy(cos_out, e->cos_t.data(), e->cos_t.size() * sizeof(float));
  if (sin_out) memcpy(sin_out, e->sin_t.data(), e->sin_t.size() * sizeof(float));
  return TRG_OK;
}

TrgStatus debug_map_index(TrgEngine *e, TrgKind map, float *x, float *y, float *z, int32_t *perm, int32_t *grid_wh,
                          float *origin_cell) {
  DevMap &m = *pick_map(e, map);
  if (!m.valid) return e->fail(TRG_ERR_NO_MAP, "no map");
  if (x) HIPCHK(e, hipMemcpy(x, m.x, m.n * sizeof(float), hipMemcpyDeviceToHost));
  if (y) HIPCHK(e, hipMemcpy(y, m.y, m.n * sizeof(float), hipMemcpyDeviceToHost));
  if (z) HIPCHK(e, hipMemcpy(z, m.z, m.n * sizeof(float), hipMemcpyDeviceToHost));
  if (perm) HIPCHK(e, hipMemcpy(perm, m.perm, m.n * sizeof(int), hipMemcpyDeviceToHost));
  if (grid_wh) {
    grid_wh[0] = m.view.W;
    grid_wh[1] = m.view.H;
  }
  if (origin_cell) {
    origin_cell[0] = m.view.x0;
    origin_cell[1] = m.view.y0;
    origin_cell[2] = m.g;
  }
  return TRG_OK;
}

}  // namespace

#include "trg_engine_plan.ipp"
#include "trg_engine_field.ipp"

extern "C" {

TrgStatus trg_engine_create(const TrgParams *params, int device, TrgEngine **out) {
  if (!params || !out) return TRG_ERR_INVALID_ARG;
  *out = nullptr;  // (stays so where the engine itself cannot be made: TRG_ERR_CAPACITY)
  return abi_guard("create", [out](TrgStatus s, const std::string &m) { return *out ? (*out)->fail(s, m) : s; },
                   [&] { return create_engine(params, device, out); });
}

void trg_engine_destroy(TrgEngine *e) {
  if (!e) return;
  // the main stream is the first thing create makes on the device: without it every owner is empty, and
  // nothing below needs a device (there may be none)
  if (e->s_main) {
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
  }
  delete e;  // the order of release is the members' order, see TrgEngine
}

const char *trg_engine_last_error(const TrgEngine *e) { return e ? e->err.c_str() : "null engine"; }
const char *trg_engine_device_arch(const TrgEngine *e) { return e ? e->arch.c_str() : ""; }
const char *trg_engine_fallback_reason(const TrgEngine *e) { return e ? e->bfs_fallback_reason.c_str() : ""; }

TrgStatus trg_engine_set_global_map(TrgEngine *e, const float *xyz, size_t n, size_t stride) {
  return entry(e, "set_global_map", DEVICE, [&] { return set_global_map(e, xyz, n, stride); });
}

TrgStatus trg_engine_set_global_map_device(TrgEngine *e, const float *d_xyz, size_t n, size_t stride) {
  return entry(e, "set_global_map_device", DEVICE, [&] { return set_global_map_device(e, d_xyz, n, stride); });
}

TrgStatus trg_engine_set_local_map(TrgEngine *e, const float start_xy[2], const float *xyz, size_t n,
                                   size_t stride) {
  return entry(e, "set_local_map", DEVICE, [&] { return set_local_map(e, start_xy, xyz, n, stride); });
}

TrgStatus trg_engine_reset_map(TrgEngine *e, TrgKind kind) {
  return entry(e, "reset_map", DEVICE, [&] { return reset_map(e, kind); });
}

TrgStatus trg_engine_reset_graph(TrgEngine *e, TrgKind kind) {
  return entry(e, "reset_graph", DEVICE, [&] { return reset_graph(e, kind); });
}

TrgStatus trg_engine_init_graph(TrgEngine *e, const float start_xyz[3], const TrgSampler *sampler) {
  return entry(e, "init_graph", DEVICE, [&] { return init_graph(e, start_xyz, sampler); });
}

TrgStatus trg_engine_update_graph(TrgEngine *e) {
  return entry(e, "update_graph", DEVICE, [&] { return update_graph(e); });
}

TrgStatus trg_engine_set_option(TrgEngine *e, const char *key, const char *value) {
  if (!key || !value) return TRG_ERR_INVALID_ARG;
  return entry(e, "set_option", ENGINE, [&] { return set_option(e, key, value); });
}

TrgStatus trg_engine_set_tile(TrgEngine *e, const float core_xyxy[4], uint32_t epoch) {
  return entry(e, "set_tile", ENGINE, [&] { return set_tile(e, core_xyxy, epoch); });
}

TrgStatus trg_engine_export_csr(TrgEngine *e, TrgKind kind, TrgCsrView *out) {
  if (!out) return TRG_ERR_INVALID_ARG;
  return entry(e, "export_csr", ENGINE, [&] { return export_csr(e, kind, out); });
}

TrgStatus trg_engine_save_json(TrgEngine *e, const char *path) {
  if (!path) return TRG_ERR_INVALID_ARG;
  return entry(e, "save_json", ENGINE, [&] { return save_json(e, path); });
}

TrgStatus trg_engine_load_json(TrgEngine *e, const char *path) {
  return entry(e, "load_json", DEVICE, [&] { return load_json(e, path); });
}

TrgStatus trg_engine_is_collision_batch(TrgEngine *e, TrgKind map, float threshold, const float *xy, size_t m,
                                        int32_t *flag, int32_t *cnt, int32_t *n) {
  return entry(e, "is_collision_batch", DEVICE,
               [&] { return is_collision_batch(e, map, threshold, xy, m, flag, cnt, n); });
}

TrgStatus trg_engine_nearest_z_batch(TrgEngine *e, TrgKind map, const float *xy, size_t m, float *z) {
  return entry(e, "nearest_z_batch", DEVICE, [&] { return nearest_z_batch(e, map, xy, m, z); });
}

TrgStatus trg_engine_edge_risk_batch(TrgEngine *e, TrgKind map, const float *p1_xyz, const float *p2_xyz, size_t m,
                                     int32_t *status, int32_t *n_pts, float *weight, float *dist) {
  return entry(e, "edge_risk_batch", DEVICE,
               [&] { return edge_risk_batch(e, map, p1_xyz, p2_xyz, m, status, n_pts, weight, dist); });
}

TrgStatus trg_engine_voxel_filter(TrgEngine *e, const float *xyz, size_t n, size_t stride, float leaf, float *out_xyz,
                                  size_t *n_out, int32_t *passthrough) {
  return entry(e, "voxel_filter", DEVICE,
               [&] { return voxel_filter(e, xyz, n, stride, leaf, out_xyz, n_out, passthrough); });
}

TrgStatus trg_engine_is_frontier_batch(TrgEngine *e, const float *xy, size_t m, int32_t *flag) {
  return entry(e, "is_frontier_batch", DEVICE, [&] { return is_frontier_batch(e, xy, m, flag); });
}

TrgStatus trg_engine_get_stats(const TrgEngine *e, TrgStats *out) {
  if (!out) return TRG_ERR_INVALID_ARG;
  return entry(const_cast<TrgEngine *>(e), "get_stats", ENGINE, [&] {
    *out = e->stats;
    return TRG_OK;
  });
}

TrgStatus trg_engine_pose_links(TrgEngine *e, const float *poses_xy, int32_t m, float radius, int32_t cap,
                                int32_t *link_node, float *link_weight, float *link_dist, TrgPoseInfo *infos) {
  return entry(e, "pose_links", DEVICE,
               [&] { return pose_links(e, poses_xy, m, radius, cap, link_node, link_weight, link_dist, infos); });
}

TrgStatus trg_engine_get_sampler_table(TrgEngine *e, float *cos_out, float *sin_out) {
  return entry(e, "get_sampler_table", DEVICE, [&] { return get_sampler_table(e, cos_out, sin_out); });
}

TrgStatus trg_engine_debug_map_index(TrgEngine *e, TrgKind map, float *x, float *y, float *z, int32_t *perm,
                                     int32_t *grid_wh, float *origin_cell) {
  return entry(e, "debug_map_index", DEVICE, [&] { return debug_map_index(e, map, x, y, z, perm, grid_wh, origin_cell); });
}

}  // extern "C"

#include "trg_engine_stitch.inc"
#include "trg_engine_exchange.inc"
#include "trg_engine_field_tiled.inc"

// (here BfsBuffers, StitchBufs, Uploader, ExchangeState, FieldBufs and TiledFieldBufs are complete types)
TrgEngine::TrgEngine() = default;
TrgEngine::~TrgEngine() = default;
