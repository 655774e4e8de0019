// Test code, never linked into the product: a host Dijkstra of the risk field (include/trg_engine.h,
// trg_engine_risk_field_sets) on the same (risk, hops) key.
//
//   edge risk  r = w + 0                                   (fp32; a weight of -0 counts as +0)
//   key        (bits(risk) << 32) | hops, unsigned order   (risks are >= +0)
//   extension  (a, h) -> (max(a, r), h + 1)
//   parents    smallest u with an edge u->v whose extension of key[u] is key[v]
//   walks never enter an Invalid node (state -1); a column out of range is skipped
//   sources    n_src node ids, every one at key (+0, 0)
//
// returns 0, 1 if some edge weight is NaN, negative or infinite, 2 for a bad source
#include <stdint.h>
#include <string.h>

#include <functional>
#include <limits>
#include <queue>
#include <utility>
#include <vector>

namespace {
inline uint64_t extend(uint64_t k, float r) {
  float a;
  const uint32_t hi = (uint32_t)(k >> 32);
  memcpy(&a, &hi, 4);
  const float g = r > a ? r : a;
  uint32_t gb;
  memcpy(&gb, &g, 4);
  return ((uint64_t)gb << 32) | (uint32_t)((uint32_t)k + 1u);
}
}  // namespace

extern "C" int risk_reference(int V, const int32_t *rowptr, const int32_t *col, const float *w, const int32_t *state,
                              const int32_t *src, int n_src, float *risk, int32_t *hops, int32_t *parent) {
  const uint64_t NONE = ~0ull;
  const int E = V > 0 ? rowptr[V] : 0;
  std::vector<float> er(E);
  for (int k = 0; k < E; ++k) {
    const float r = w[k] + 0.0f;
    if (!(r >= 0.0f) || r == std::numeric_limits<float>::infinity()) return 1;
    er[k] = r;
  }
  for (int j = 0; j < n_src; ++j)
    if (src[j] < 0 || src[j] >= V) return 2;
  auto relaxable = [&](int v) { return v >= 0 && v < V && state[v] != -1; };
  std::vector<uint64_t> key(V, NONE);
  std::vector<char> done(V, 0);
  typedef std::pair<uint64_t, int> Item;
  std::priority_queue<Item, std::vector<Item>, std::greater<Item>> pq;
  for (int j = 0; j < n_src; ++j) {
    if (key[src[j]] == 0) continue;
    key[src[j]] = 0;
    pq.push(Item(0, src[j]));
  }
  while (!pq.empty()) {
    const Item it = pq.top();
    pq.pop();
    const int u = it.second;
    if (done[u] || it.first != key[u]) continue;
    done[u] = 1;
    for (int k = rowptr[u]; k < rowptr[u + 1]; ++k) {
      const int v = col[k];
      if (!relaxable(v)) continue;
      const uint64_t nk = extend(key[u], er[k]);
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
      if (extend(key[u], er[k]) == key[v] && (parent[v] < 0 || u < parent[v])) parent[v] = u;
    }
  }
  for (int v = 0; v < V; ++v) {
    if (key[v] == NONE) {
      risk[v] = std::numeric_limits<float>::infinity();
      hops[v] = -1;
    } else {
      const uint32_t hi = (uint32_t)(key[v] >> 32);
      memcpy(&risk[v], &hi, 4);
      hops[v] = (int32_t)(uint32_t)key[v];
    }
  }
  return 0;
}
