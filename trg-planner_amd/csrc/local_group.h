// local_group.h -- the host side of the stitch exchange's in-process transport (host only, no HIP): a named
// group of R members in one process, each on its own thread, that meet in barriers and show each other one
// pointer (trg_engine_exchange.inc builds its all-gather from that; trg_engine_comm_join_local).
//
// Every wait is in the group's condition variable and ends after `wait_seconds` at the latest.  A wait that
// ran out, or a member that left, breaks the group for good: the members' barrier counts no longer agree, so
// every later barrier of it fails at once, with the reason.  A group lives while a member holds it; its name
// is free again once all of them are gone.
//
// tests/cpp/local_group_check.cpp checks it on its own, also under the thread sanitizer.
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace trg {

class LocalGroup {
 public:
  explicit LocalGroup(int nranks) : nranks_(nranks), member_(nranks, 0), arrived_(nranks, 0), shown_(nranks, nullptr) {}
  int nranks() const { return nranks_; }

  // Rank `rank` of the group `name`, which the first to name it makes with `nranks` ranks.  Joining waits for
  // nobody.  nullptr with the reason in `err` for a group of another size, a rank that is taken, a broken group.
  static std::shared_ptr<LocalGroup> join(const std::string &name, int nranks, int rank, std::string &err) {
    std::lock_guard<std::mutex> table(table_mutex());
    auto &groups = table_groups();
    for (auto it = groups.begin(); it != groups.end();)  // (groups whose members are all gone)
      it = it->second.expired() ? groups.erase(it) : std::next(it);
    std::weak_ptr<LocalGroup> &slot = groups[name];
    std::shared_ptr<LocalGroup> g = slot.lock();
    if (!g) {
      g = std::make_shared<LocalGroup>(nranks);
      slot = g;
    }
    std::lock_guard<std::mutex> lock(g->m_);
    if (g->nranks_ != nranks) {
      err = "group " + name + " has " + std::to_string(g->nranks_) + " ranks";
      return nullptr;
    }
    if (g->member_[rank]) {
      err = "rank " + std::to_string(rank) + " of group " + name + " is taken";
      return nullptr;
    }
    if (!g->broken_.empty()) {
      err = "group " + name + " is broken: " + g->broken_;
      return nullptr;
    }
    g->member_[rank] = 1;
    return g;
  }

  void leave(int rank) {
    std::lock_guard<std::mutex> lock(m_);
    member_[rank] = 0;
    if (broken_.empty()) broken_ = "rank " + std::to_string(rank) + " left the group";
    cv_.notify_all();
  }

  // the pointer the others read between this member's next two barriers
  void show(int rank, const void *p) {
    std::lock_guard<std::mutex> lock(m_);
    shown_[rank] = p;
  }
  std::vector<const void *> shown() {
    std::lock_guard<std::mutex> lock(m_);
    return shown_;
  }

  // Every member enters its k-th barrier before any leaves it.  "" when all came; else why not (the group is
  // then broken): a rank that did not arrive within wait_seconds is named.
  std::string barrier(int rank, double wait_seconds) {
    std::unique_lock<std::mutex> lock(m_);
    if (!broken_.empty()) return broken_;
    const uint64_t mine = ++arrived_[rank];
    cv_.notify_all();
    int late = -1;
    auto all_here = [&] {
      late = -1;
      for (int k = 0; k < nranks_ && late < 0; ++k)
        if (arrived_[k] < mine) late = k;
      return late < 0 || !broken_.empty();
    };
    // The limit is the steady clock's.  The waits themselves are slices on the system clock, that is
    // pthread_cond_timedwait, which every thread sanitizer in use knows to release the mutex (it does not know the
    // steady clock's pthread_cond_clockwait everywhere); a clock that is set meanwhile costs one slice at most.
    using steady = std::chrono::steady_clock;
    const steady::time_point limit = steady::now() + std::chrono::duration_cast<steady::duration>(std::chrono::duration<double>(
                                                         std::min(std::max(wait_seconds, 0.0), 1e6)));
    bool done = all_here();
    while (!done) {
      const steady::time_point now = steady::now();
      if (now >= limit) break;
      const steady::duration slice = std::min<steady::duration>(limit - now, std::chrono::milliseconds(200));
      cv_.wait_until(lock, std::chrono::system_clock::now() + slice);
      done = all_here();
    }
    if (late < 0) return "";  // (everyone came, whatever happened to the group since)
    if (!done) {
      broken_ = "rank " + std::to_string(late) + " did not arrive within " + std::to_string(wait_seconds) + " s";
      cv_.notify_all();
    }
    return broken_;
  }

 private:
  static std::mutex &table_mutex() {
    static std::mutex m;
    return m;
  }
  static std::map<std::string, std::weak_ptr<LocalGroup>> &table_groups() {
    static std::map<std::string, std::weak_ptr<LocalGroup>> groups;
    return groups;
  }
  std::mutex m_;
  std::condition_variable cv_;
  const int nranks_;
  std::vector<char> member_;          // rank r has joined and not left
  std::vector<uint64_t> arrived_;     // barriers rank r has entered
  std::vector<const void *> shown_;   // rank r's pointer
  std::string broken_;                // why the group is of no use any more ("" while it is)
};

}  // namespace trg
