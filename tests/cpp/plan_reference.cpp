// Test code, never linked into the product: planSafePath's A* (oracle/trg_oracle.cpp, Oracle::planSafePath) after
// start and goal are resolved, restated on a CSR whose rows hold each node's edges in push order.  Compile with
// -ffp-contract=off: on x86-64 float arithmetic is SSE, so every float operation below rounds exactly to fp32.
//
//   open list   std::priority_queue of search records, comparator a.f > b.f  (records hold float f, g)
//   step cost   g' = g + (sf * w + 1) * dist, every operand a float (four roundings), widened to double afterwards;
//               f' = g' + |goal - dst| (the fp32 planar norm), in double; both stored as float
//   open_check  a record is pushed when its node has no open record or its g is smaller than that record's g;
//               the popped record's node leaves open_check, a popped node is closed for good
//   skipped     closed destinations, Invalid destinations (state -1)
//   summary     walking back from the goal, each node with a parent adds dist and w of the FIRST edge of ITS OWN row
//               that leads to the parent (the reverse edge, not the edge taken), nothing if there is none;
//               avg_risk = sum_w / number of path points
//
// widen != 0: the step cost with sf held as a double (one rounding on the store), which is not the oracle's
// arithmetic; it only serves to show that a set of graphs tells the two apart.
//
// returns 0 (path found), 6 (no path: num_points 0), 1 (bad argument)
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <queue>
#include <vector>

namespace {
struct Rec {
  int id, parent;  // parent: index of a record, -1 for the start
  float f, g;
};
inline float planar(float dx, float dy) { return std::sqrt(dx * dx + dy * dy); }
}  // namespace

extern "C" int plan_reference(int V, const int32_t *rowptr, const int32_t *col, const float *w, const float *dist,
                              const int32_t *state, const float *pos, float safety_factor, int start, int goal,
                              int widen, int32_t *path, int32_t path_cap, float *info3, int32_t *num_points) {
  info3[0] = info3[1] = info3[2] = 0.0f;
  *num_points = 0;
  if (start < 0 || start >= V || goal < 0 || goal >= V) return 1;
  std::vector<Rec> recs;
  std::function<bool(int, int)> later = [&recs](int a, int b) { return recs[a].f > recs[b].f; };
  std::priority_queue<int, std::vector<int>, std::function<bool(int, int)>> open_list(later);
  std::vector<int> open_check(V, -1);
  std::vector<char> closed(V, 0);
  const float gx = pos[3 * goal], gy = pos[3 * goal + 1];
  const double sf_wide = safety_factor;

  const float direct = planar(gx - pos[3 * start], gy - pos[3 * start + 1]);
  info3[0] = direct;
  {
    const double g_cost = 0.0;
    const double f_cost = g_cost + direct;
    recs.push_back(Rec{start, -1, (float)f_cost, (float)g_cost});
    open_list.push(0);
    open_check[start] = 0;
  }
  while (!open_list.empty()) {
    const int ci = open_list.top();
    open_list.pop();
    const Rec cur = recs[ci];
    open_check[cur.id] = -1;

    if (cur.id == goal) {
      std::vector<int> back;
      float sum_dist = 0.0f, sum_weight = 0.0f;
      for (int r = ci; r >= 0; r = recs[r].parent) {
        const int n = recs[r].id;
        if (recs[r].parent >= 0) {
          const int p = recs[recs[r].parent].id;
          for (int k = rowptr[n]; k < rowptr[n + 1]; ++k)
            if (col[k] == p) {
              sum_dist += dist[k];
              sum_weight += w[k];
              break;
            }
        }
        back.push_back(n);
      }
      info3[1] = sum_dist;
      info3[2] = sum_weight / back.size();
      *num_points = (int32_t)back.size();
      for (size_t i = 0; i < back.size() && (int32_t)i < path_cap; ++i) path[i] = back[back.size() - 1 - i];
      return 0;
    }

    closed[cur.id] = 1;
    for (int k = rowptr[cur.id]; k < rowptr[cur.id + 1]; ++k) {
      const int dst = col[k];
      if (dst < 0 || dst >= V) continue;
      if (closed[dst] || state[dst] == -1) continue;
      double next_g;
      if (widen) {
        next_g = cur.g + (sf_wide * w[k] + 1) * dist[k];
      } else {
        const float step = cur.g + (safety_factor * w[k] + 1) * dist[k];
        next_g = step;
      }
      const double next_f = next_g + planar(gx - pos[3 * dst], gy - pos[3 * dst + 1]);
      recs.push_back(Rec{dst, ci, (float)next_f, (float)next_g});
      const int ni = (int)recs.size() - 1;
      if (open_check[dst] < 0 || recs[ni].g < recs[open_check[dst]].g) {
        open_list.push(ni);
        open_check[dst] = ni;
      }
    }
  }
  return 6;
}
