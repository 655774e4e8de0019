// Test code, never linked into the product: a host Dijkstra of the cost field (include/trg_engine.h,
// trg_engine_cost_field) on the same (cost, hops) key.  Compile with -ffp-contract=off: on x86-64 float
// arithmetic is SSE, so every operation below rounds exactly to fp32, as on the device.
//
//   edge cost  c = (sf * w + 1) * dist                     (fp32, three roundings)
//   key        (bits(cost) << 32) | hops, unsigned order  (costs are >= +0)
//   extension  (a, h) -> (fl(a + c), h + 1)
//   parents    smallest u with an edge u->v whose extension of key[u] is key[v]
//   walks never enter an Invalid node (state -1); a column out of range is skipped
//
// returns 0, 1 if some edge cost is negative or not finite, 2 for a bad source
#include <stdint.h>
#include <string.h>

#include <functional>
#include <limits>
#include <queue>
#include <utility>
#include <vector>

namespace {
inline uint64_t extend(uint64_t k, float c) {
  float a;
  const uint32_t hi = (uint32_t)(k >> 32);
  memcpy(&a, &hi, 4);
  const float g = a + c;
  uint32_t gb;
  memcpy(&gb, &g, 4);
  return ((uint64_t)gb << 32) | (uint32_t)((uint32_t)k + 1u);
}
}  // namespace

extern "C" int field_reference(int V, const int32_t *rowptr, const int32_t *col, const float *w, const float *dist,
                               const int32_t *state, float sf, int src, float *cost, int32_t *hops,
                               int32_t *parent) {
  const uint64_t NONE = ~0ull;
  const int E = V > 0 ? rowptr[V] : 0;
  std::vector<float> ec(E);
  for (int k = 0; k < E; ++k) {
    const float c = (sf * w[k] + 1.0f) * dist[k];
    if (!(c >= 0.0f) || c == std::numeric_limits<float>::infinity()) return 1;
    ec[k] = c;
  }
  if (src < 0 || src >= V) return 2;
  auto relaxable = [&](int v) { return v >= 0 && v < V && state[v] != -1; };
  std::vector<uint64_t> key(V, NONE);
  std::vector<char> done(V, 0);
  typedef std::pair<uint64_t, int> Item;
  std::priority_queue<Item, std::vector<Item>, std::greater<Item>> pq;
  key[src] = 0;
  pq.push(Item(0, src));
  while (!pq.empty()) {
    const Item it = pq.top();
    pq.pop();
    const int u = it.second;
    if (done[u] || it.first != key[u]) continue;
    done[u] = 1;
    for (int k = rowptr[u]; k < rowptr[u + 1]; ++k) {
      const int v = col[k];
      if (!relaxable(v)) continue;
      const uint64_t nk = extend(key[u], ec[k]);
      if (nk < key[v]) {
        key[v] = nk;
        pq.push(Item(nk, v));
      }
    }
  }
  for (int v = 0; v < V; ++v) parent[v] = -1;
  for (int u = 0; u < V; ++u) {
    if (key[u] == NONE) continue;
    for (int k = rowptr[u]; k < rowptr[u + 1]; ++k) {
      const int v = col[k];
      if (!relaxable(v)) continue;
      if (extend(key[u], ec[k]) == key[v] && (parent[v] < 0 || u < parent[v])) parent[v] = u;
    }
  }
  for (int v = 0; v < V; ++v) {
    if (key[v] == NONE) {
      cost[v] = std::numeric_limits<float>::infinity();
      hops[v] = -1;
    } else {
      const uint32_t hi = (uint32_t)(key[v] >> 32);
      memcpy(&cost[v], &hi, 4);
      hops[v] = (int32_t)(uint32_t)key[v];
    }
  }
  return 0;
}
