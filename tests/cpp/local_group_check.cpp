// local_group_check.cpp -- csrc/local_group.h on its own (host only): R threads run the all-gather's host side
// (show a pointer, barrier, read everybody's, barrier) many times and must always read what the others showed for
// that very round; joins that must be refused; a member that leaves breaks the group at once, also for a member
// waiting in a barrier; a name is free again when all members are gone.  Prints "ok".  tests/test_local_group.py
// builds it plain and under the thread sanitizer.  No case waits for the limit to run out.
#include <atomic>
#include <cstdio>
#include <thread>

#include "../../trg-planner_amd/csrc/local_group.h"

using trg::LocalGroup;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static const double WAIT = 30.0;  // a cap no case runs into

static int rounds(int R, int n_rounds) {
  std::string err;
  std::vector<std::shared_ptr<LocalGroup>> g(R);
  for (int r = 0; r < R; ++r) {
    g[r] = LocalGroup::join("rounds" + std::to_string(R), R, r, err);
    CHECK(g[r] && g[r] == g[0]);
  }
  std::vector<long> value(R, -1);  // rank r's "send buffer"
  std::atomic<int> bad{0};
  std::vector<std::thread> th;
  for (int r = 0; r < R; ++r)
    th.emplace_back([&, r] {
      for (long k = 0; k < n_rounds; ++k) {
        value[r] = 1000 * k + r;  // written before the barrier, read by the others after it
        g[r]->show(r, &value[r]);
        if (!g[r]->barrier(r, WAIT).empty()) ++bad;
        const std::vector<const void *> from = g[r]->shown();
        for (int j = 0; j < R; ++j)
          if (from[j] != &value[j] || *(const long *)from[j] != 1000 * k + j) ++bad;
        if (!g[r]->barrier(r, WAIT).empty()) ++bad;  // (nobody writes its next value before all have read)
      }
    });
  for (auto &t : th) t.join();
  CHECK(bad == 0);
  for (int r = 0; r < R; ++r) g[r]->leave(r);
  return 0;
}

static int refusals() {
  std::string err;
  auto a = LocalGroup::join("refusals", 2, 0, err);
  CHECK(a && a->nranks() == 2);
  CHECK(!LocalGroup::join("refusals", 2, 0, err) && err == "rank 0 of group refusals is taken");
  CHECK(!LocalGroup::join("refusals", 3, 1, err) && err == "group refusals has 2 ranks");
  auto b = LocalGroup::join("refusals", 2, 1, err);
  CHECK(b == a);
  // a member that leaves breaks the group: at once for a later barrier, and for one that is waiting
  std::string waited;
  std::thread t([&] { waited = a->barrier(0, WAIT); });
  b->leave(1);
  t.join();
  CHECK(waited == "rank 1 left the group");
  CHECK(a->barrier(0, WAIT) == "rank 1 left the group");
  CHECK(!LocalGroup::join("refusals", 2, 1, err) && err == "group refusals is broken: rank 1 left the group");
  a->leave(0);
  a.reset();
  b.reset();
  // all members gone: the name makes a new group
  auto c = LocalGroup::join("refusals", 1, 0, err);
  CHECK(c && c->nranks() == 1 && c->barrier(0, WAIT).empty() && c->barrier(0, WAIT).empty());
  c->leave(0);
  return 0;
}

int main() {
  if (rounds(2, 2000) || rounds(9, 500) || rounds(1, 10) || refusals()) return 1;
  std::puts("ok");
  return 0;
}
