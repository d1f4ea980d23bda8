// The side-operation mailbox: one operation at a time travels from the thread that posts it
// (the cold-store thread) to the stepper, which launches it beside the steps, and its result
// back.  Host-only -- no HIP, no Python: what an operation launches and how its completion
// is polled stay in the engine; tests/native/engine_host_test.cpp runs the box alone.
//
// States: empty -> posted (post) -> launched (begin_launch .. launched, the stepper) -> empty
// (clear, by the poster once it has taken the result).  One poster thread, one launcher.
#pragma once
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <optional>
#include <stdexcept>

#include "step_abi.h"

// kind: what to run (0: nothing; the engine's SIDE_* values); a, b, c, max_n, max_bytes: its
// scalar arguments; n: records that came with it
struct SideOp { int kind; u32 a; u64 b, c; u32 max_n; u64 max_bytes; u32 n; };

class SideBox {
 public:
  // fill runs under the lock once the box is known to be empty and before the operation can
  // be launched (the engine copies the operation's records into their host-mapped buffer)
  template <class Fill>
  void post(const SideOp& op, Fill&& fill) {
    std::lock_guard<std::mutex> g(mu_);
    if (op_.kind) throw std::runtime_error("side operation pending (side_wait first)");
    fill();
    op_ = op;
    launched_ = false;
  }
  void post(const SideOp& op) { post(op, [] {}); }
  bool pending() {
    std::lock_guard<std::mutex> g(mu_);
    return op_.kind != 0;
  }
  // posted and not launched yet
  bool queued() {
    std::lock_guard<std::mutex> g(mu_);
    return op_.kind && !launched_;
  }
  // the launcher: the operation to launch now, if one is queued; launched() once it is on
  // its stream (an operation whose launch threw stays queued)
  std::optional<SideOp> begin_launch() {
    std::lock_guard<std::mutex> g(mu_);
    if (!op_.kind || launched_) return std::nullopt;
    return op_;
  }
  void launched() {
    std::lock_guard<std::mutex> g(mu_);
    launched_ = true;
    cv_.notify_all();
  }
  // the poster: the posted operation's kind once it was launched, 0 when it was not by the
  // deadline; throws when nothing is posted
  int wait_launched(std::chrono::steady_clock::time_point until) {
    std::unique_lock<std::mutex> g(mu_);
    if (!op_.kind) throw std::runtime_error("side_wait: nothing posted");
    return cv_.wait_until(g, until, [&] { return launched_; }) ? op_.kind : 0;
  }
  // the result was taken: empty again (only a launched operation can be cleared)
  void clear() {
    std::lock_guard<std::mutex> g(mu_);
    if (!op_.kind || !launched_) throw std::logic_error("side box: clear() of an operation that was not launched");
    op_.kind = 0;
    launched_ = false;
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  SideOp op_{0, 0, 0, 0, 0, 0, 0};
  bool launched_ = false;
};
