// Stand-alone check of trg-planner_amd/csrc/abi_frame.h: the exception ladder of the C entries and the
// engine's fork-join, with the failures injected here (throwing bodies, a thread type whose constructor
// throws).  Prints "ok" and exits 0; tests/test_abi_frame.py builds it plain and under the sanitizers.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../trg-planner_amd/csrc/abi_frame.h"

using trg::abi_guard;
using trg::fork_join;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

// ---- abi_guard ---------------------------------------------------------------------------------------
struct Sink {  // what TrgEngine::fail is to the engine
  std::string msg = "untouched";
  int calls = 0;
  TrgStatus operator()(TrgStatus s, const std::string &m) {
    msg = m;
    calls++;
    return s;
  }
};

template <typename Body>
void guard_case(Body body, TrgStatus want, const char *want_msg, int want_calls) {
  Sink sink;
  const TrgStatus st = abi_guard("the call", [&](TrgStatus s, const std::string &m) { return sink(s, m); }, body);
  CHECK(st == want);
  CHECK(sink.msg == want_msg);
  CHECK(sink.calls == want_calls);
}

void check_guard() {
  guard_case([]() -> TrgStatus { throw std::bad_alloc(); }, TRG_ERR_CAPACITY, "the call: out of host memory", 1);
  guard_case([]() -> TrgStatus { throw std::length_error("vector::reserve"); }, TRG_ERR_CAPACITY,
             "the call: out of host memory", 1);
  guard_case([]() -> TrgStatus { throw std::runtime_error("x"); }, TRG_ERR_DEVICE, "the call: x", 1);
  guard_case([]() -> TrgStatus { throw 7; }, TRG_ERR_DEVICE, "the call: unknown exception", 1);
  guard_case([]() -> TrgStatus { return TRG_OK; }, TRG_OK, "untouched", 0);
  guard_case([]() -> TrgStatus { return TRG_ERR_NO_MAP; }, TRG_ERR_NO_MAP, "untouched", 0);
  // a `fail` that throws itself: the bare status comes back
  const TrgStatus st = abi_guard(
      "the call", [](TrgStatus, const std::string &) -> TrgStatus { throw std::bad_alloc(); },
      []() -> TrgStatus { throw std::runtime_error("x"); });
  CHECK(st == TRG_ERR_DEVICE);
}

// ---- fork_join -----------------------------------------------------------------------------------------
// std::thread whose `fail_at`-th construction (counted from 1, per plan) throws what a failed spawn throws;
// counts what was started and what was joined
struct FlakyThread {
  static int fail_at, made, started, joined;
  static void plan(int at) {
    fail_at = at;
    made = started = joined = 0;
  }
  std::thread th;
  template <typename F, typename... A>
  explicit FlakyThread(F &&f, A &&...a) {
    if (++made == fail_at) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
    th = std::thread(std::forward<F>(f), std::forward<A>(a)...);
    started++;
  }
  FlakyThread(FlakyThread &&) = default;
  void join() {
    th.join();
    joined++;
  }
};
int FlakyThread::fail_at = 0, FlakyThread::made = 0, FlakyThread::started = 0, FlakyThread::joined = 0;

struct Tally {  // which index ran how often, and on which thread in which order
  std::mutex mu;
  std::vector<int> runs;
  std::vector<size_t> on_caller;
  std::thread::id caller = std::this_thread::get_id();
  explicit Tally(size_t T) : runs(T, 0) {}
  void note(size_t t) {
    std::lock_guard<std::mutex> g(mu);
    runs[t]++;
    if (std::this_thread::get_id() == caller) on_caller.push_back(t);
  }
  void check_each_once() const {
    for (int r : runs) CHECK(r == 1);
  }
  void check_caller_ascending() const {
    CHECK(!on_caller.empty() && on_caller[0] == 0);
    for (size_t i = 1; i < on_caller.size(); ++i) CHECK(on_caller[i] > on_caller[i - 1]);
  }
};

void check_fork_join() {
  for (size_t T : {(size_t)1, (size_t)2, (size_t)8}) {
    Tally tally(T);
    fork_join(T, [&](size_t t) { tally.note(t); });
    tally.check_each_once();
    CHECK(tally.on_caller.size() == 1 && tally.on_caller[0] == 0);
  }
  fork_join(0, [&](size_t) { CHECK(false); });

  // a spawn fails: the first, the fourth, the last of the seven
  for (int at : {1, 4, 7}) {
    const size_t T = 8;
    Tally tally(T);
    FlakyThread::plan(at);
    fork_join<FlakyThread>(T, [&](size_t t) { tally.note(t); });
    tally.check_each_once();
    tally.check_caller_ascending();
    CHECK(FlakyThread::started == at - 1 && FlakyThread::joined == at - 1);
    CHECK(tally.on_caller.size() == 1 + (T - (size_t)at));  // index 0 and every index without a thread
    CHECK(tally.on_caller.back() == T - 1);
  }

  // fn(3) throws on its own thread: it arrives here, after every other index has finished
  {
    const size_t T = 8;
    std::atomic<int> finished{0};
    bool caught = false;
    FlakyThread::plan(0);
    try {
      fork_join<FlakyThread>(T, [&](size_t t) {
        if (t == 3) throw std::runtime_error("three");
        finished++;
      });
    } catch (const std::runtime_error &x) {
      caught = std::string(x.what()) == "three";
      CHECK(finished == (int)T - 1);
    }
    CHECK(caught);
    CHECK(FlakyThread::started == 7 && FlakyThread::joined == 7);
  }

  // two indices throw: one exception arrives, and it is one of the two
  {
    int arrivals = 0;
    std::atomic<int> finished{0};
    try {
      fork_join(8, [&](size_t t) {
        if (t == 2 || t == 5) throw std::runtime_error(t == 2 ? "two" : "five");
        finished++;
      });
    } catch (const std::runtime_error &x) {
      arrivals++;
      CHECK(std::string(x.what()) == "two" || std::string(x.what()) == "five");
    }
    CHECK(arrivals == 1 && finished == 6);
  }

  // fn(0) throws on the caller: the others are joined first
  {
    std::atomic<int> finished{0};
    bool caught = false;
    FlakyThread::plan(0);
    try {
      fork_join<FlakyThread>(8, [&](size_t t) {
        if (t == 0) throw std::length_error("zero");
        finished++;
      });
    } catch (const std::length_error &) {
      caught = true;
      CHECK(finished == 7);
      CHECK(FlakyThread::started == 7 && FlakyThread::joined == 7);
    }
    CHECK(caught);
  }

  // the two together, as an entry has them: a worker's exception becomes the entry's status
  {
    Sink sink;
    const TrgStatus st = abi_guard("plan_batch", [&](TrgStatus s, const std::string &m) { return sink(s, m); }, [&] {
      fork_join(4, [&](size_t t) {
        if (t == 1) throw std::bad_alloc();
      });
      return TRG_OK;
    });
    CHECK(st == TRG_ERR_CAPACITY && sink.msg == "plan_batch: out of host memory");
  }
}

int main() {
  check_guard();
  check_fork_join();
  printf("ok\n");
  return 0;
}
