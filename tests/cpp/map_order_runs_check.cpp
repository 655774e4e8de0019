// CPU check: the container order as runs (MapOrderSim::runs / runs_into) and its expansion map_order_at
// (map_order_runs.h, the function the device kernel uses) against MapOrderSim::iteration_order and against the
// real std::unordered_map<int,int>: sizes 0, 1, 2, at and around every rehash up to a million keys, 642 000; after
// clear() + refill with fewer and with more keys; after assign_from; and the run count at four million keys.
#include <cstdio>
#include <unordered_map>
#include <vector>

#include "../../trg-planner_amd/csrc/map_order_sim.h"

static int max_runs = 0;

// the three descriptions of one order agree
static bool check(const std::unordered_map<int, int> &m, const trg::MapOrderSim &s, const char *what, long n) {
  std::vector<int> want, got;
  want.reserve(m.size());
  for (auto &kv : m) want.push_back(kv.first);
  s.iteration_order(got);
  if (want != got || m.bucket_count() != s.bucket_count()) {
    printf("%s n=%ld: iteration_order differs from the container\n", what, n);
    return false;
  }
  const std::vector<trg::MapOrderSim::OrderRun> rs = s.runs();
  if ((int)rs.size() > max_runs) max_runs = (int)rs.size();
  size_t k = 0;
  for (const auto &r : rs) {  // the accessor itself: (lo, hi, descending) in iteration order
    if (r.hi <= r.lo) {
      printf("%s n=%ld: empty run\n", what, n);
      return false;
    }
    for (int j = 0; j < r.hi - r.lo; ++j, ++k)
      if (k >= want.size() || want[k] != (r.descending ? r.hi - 1 - j : r.lo + j)) {
        printf("%s n=%ld: runs() differs at position %zu\n", what, n, k);
        return false;
      }
  }
  if (k != want.size()) {
    printf("%s n=%ld: runs() covers %zu of %zu keys\n", what, n, k, want.size());
    return false;
  }
  trg::MapOrderRuns R;
  if (!s.runs_into(R)) {
    printf("%s n=%ld: more than %d runs\n", what, n, trg::MAP_ORDER_MAX_RUNS);
    return false;
  }
  if (R.n > 0 ? R.start[R.n] != (int)want.size() : !want.empty()) {
    printf("%s n=%ld: packed runs cover the wrong number of keys\n", what, n);
    return false;
  }
  for (size_t p = 0; p < want.size(); ++p)
    if (trg::map_order_at(R, (int)p) != want[p]) {
      printf("%s n=%ld: map_order_at differs at position %zu\n", what, n, p);
      return false;
    }
  // a cap below the run count is refused (the engine expands on the host then)
  if (rs.size() > 1 && s.runs_into(R, (int)rs.size() - 1)) {
    printf("%s n=%ld: cap not honoured\n", what, n);
    return false;
  }
  return true;
}

static void fill_to(std::unordered_map<int, int> &m, trg::MapOrderSim &s, long n) {
  for (long i = (long)m.size(); i < n; ++i) m[(int)i] = (int)i;
  s.fill((size_t)n - s.size());
}

int main() {
  // the sizes at which a fresh container rehashes, up to a million keys
  std::vector<long> sizes = {0, 1, 2, 642000};
  {
    trg::MapOrderSim probe;
    size_t b = probe.bucket_count();
    for (long n = 1; n <= 1000000; ++n) {
      probe.insert_next();
      if (probe.bucket_count() != b) {  // the n-th key caused a rehash: sizes n - 1 (at the limit) and n (one past)
        b = probe.bucket_count();
        sizes.push_back(n - 1);
        sizes.push_back(n);
      }
    }
  }
  for (long n : sizes) {
    std::unordered_map<int, int> m;
    trg::MapOrderSim s;
    fill_to(m, s, n);
    if (!check(m, s, "fresh fill", n)) return 1;
    // clear() keeps the buckets: refill with fewer, then with more keys than before
    const long fewer = n / 3, more = n + n / 2 + 5;
    for (long r : {fewer, more}) {
      m.clear();
      s.clear();
      fill_to(m, s, r);
      if (!check(m, s, "refill", r)) return 1;
    }
    // cleanGraph: a fresh container of the survivors takes the place of the old one, then the graph grows
    std::unordered_map<int, int> m2;
    trg::MapOrderSim s2;
    fill_to(m2, s2, n - n / 16);
    m = m2;
    s.assign_from(s2);
    if (!check(m, s, "assign_from", n)) return 1;
    fill_to(m, s, n + 7);
    if (!check(m, s, "assign_from + growth", n)) return 1;
  }
  // four million nodes: fresh, and after the clear + refill cycles above (the replica alone)
  {
    trg::MapOrderSim s;
    s.fill(4000000);
    int worst = (int)s.runs().size();
    s.clear();
    s.fill(1000);
    s.clear();
    s.fill(4000000 + 2000000);
    if ((int)s.runs().size() > worst) worst = (int)s.runs().size();
    trg::MapOrderRuns R;
    if (worst > trg::MAP_ORDER_MAX_RUNS || !s.runs_into(R)) {
      printf("4 M nodes: %d runs, cap %d\n", worst, trg::MAP_ORDER_MAX_RUNS);
      return 1;
    }
    if (worst > max_runs) max_runs = worst;
  }
  printf("ok (%zu sizes, at most %d runs)\n", sizes.size(), max_runs);
  return 0;
}
