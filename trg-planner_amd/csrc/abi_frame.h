// abi_frame.h -- the two frames every C entry of the engine stands on (host only, no HIP):
//
//   abi_guard   runs an entry's body behind the one exception ladder, so that "no exceptions cross the
//               boundary; every call returns a TrgStatus" (include/trg_engine.h) holds for allocation
//               failures and whatever else the standard library throws;
//   fork_join   the engine's one fork-join over host threads: every started thread is joined on every
//               path, a thread that cannot be started costs speed and nothing else, and an exception
//               of a worker reaches the caller, where abi_guard can catch it.
//
// tests/cpp/abi_frame_check.cpp checks both on their own, also under the sanitizers.
#pragma once
#include <atomic>
#include <cstddef>
#include <exception>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/trg_engine.h"

namespace trg {

// body() -> TrgStatus behind the ladder; `fail` is any callable (TrgStatus, std::string) -> TrgStatus that
// records the message (TrgEngine::fail).  Nothing leaves: where even the message cannot be built, the
// bare status is the answer.
template <typename Fail, typename Body>
TrgStatus abi_guard(const char *call, Fail fail, Body body) noexcept {
  auto refuse = [&](TrgStatus s, const char *what) noexcept {
    try {
      return fail(s, std::string(call) + ": " + what);
    } catch (...) {
      return s;
    }
  };
  try {
    return body();
  } catch (const std::bad_alloc &) {
    return refuse(TRG_ERR_CAPACITY, "out of host memory");
  } catch (const std::length_error &) {
    return refuse(TRG_ERR_CAPACITY, "out of host memory");
  } catch (const std::exception &x) {
    return refuse(TRG_ERR_DEVICE, x.what());
  } catch (...) {
    return refuse(TRG_ERR_DEVICE, "unknown exception");
  }
}

// fn(t) for every t in [0, T): index 0 on the caller, the others on a thread each.  A thread that cannot be
// started (std::system_error, or no memory for the handles) leaves its index and those after it to the
// caller, which runs them after fn(0) in ascending order: callers partition their work by index, so the
// result is the same.  Every fn(t) runs to its end or to its exception; the first exception caught is
// rethrown here once all threads are joined.  (`Thread` is a parameter for the check alone: it injects a
// type whose constructor throws.)
template <typename Thread = std::thread, typename F>
void fork_join(size_t T, F fn) {
  std::atomic_flag thrown = ATOMIC_FLAG_INIT;
  std::exception_ptr first;  // written by whoever set `thrown`, read after the join
  auto run = [&](size_t t) noexcept {
    try {
      fn(t);
    } catch (...) {
      if (!thrown.test_and_set()) first = std::current_exception();
    }
  };
  std::vector<Thread> thr;
  size_t started = 1;  // indices below this one have a runner
  try {
    if (T > 1) thr.reserve(T - 1);
    for (; started < T; ++started) thr.emplace_back(run, started);
  } catch (...) {  // (the caller takes over below)
  }
  if (T > 0) run(0);
  for (size_t t = started; t < T; ++t) run(t);
  for (Thread &th : thr) th.join();
  if (first) std::rethrow_exception(first);
}

}  // namespace trg
