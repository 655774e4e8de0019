// map_order_runs.h -- the iteration order of MapOrderSim (map_order_sim.h) as a short list of runs, and the
// expansion "position k of the order -> node id" over it, for the host and for device code alike.
//
// Between two rehashes the dense keys land side by side in the element list, so the order of V nodes is a few
// runs of consecutive ids (one per rehash at most, ~20 for a million nodes), each read upwards or downwards.
// The list is small enough to travel as a kernel argument: the O(V) expansion then runs on the device, where
// cleanGraph's renumbering kernels read it, not on the host while the GPU waits.
// tests/cpp/map_order_runs_check.cpp compares the expansion with iteration_order and the real container.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TRG_RUNS_HD __host__ __device__
#else
#define TRG_RUNS_HD
#endif

namespace trg {

constexpr int MAP_ORDER_MAX_RUNS = 64;

// runs [0, n) in iteration order: run r covers the positions [start[r], start[r + 1]) and holds the ids
// [lo[r], lo[r] + start[r + 1] - start[r]), read from the top down when bit r of descending is set
struct MapOrderRuns {
  int n;
  int start[MAP_ORDER_MAX_RUNS + 1];
  int lo[MAP_ORDER_MAX_RUNS];
  unsigned long long descending;
};

// the run that holds position k (0 <= k < R.start[R.n]): the last r with start[r] <= k
TRG_RUNS_HD inline int map_order_run_of(const MapOrderRuns &R, int k) {
  int a = 0, b = R.n - 1;
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (R.start[mid] <= k) a = mid;
    else b = mid - 1;
  }
  return a;
}

// the node id at position k of the order
TRG_RUNS_HD inline int map_order_at(const MapOrderRuns &R, int k) {
  const int r = map_order_run_of(R, k);
  const int off = k - R.start[r];
  const int len = R.start[r + 1] - R.start[r];
  return ((R.descending >> r) & 1ull) ? R.lo[r] + len - 1 - off : R.lo[r] + off;
}

}  // namespace trg
