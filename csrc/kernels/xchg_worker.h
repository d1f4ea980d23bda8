// The asynchronous exchange's worker (xchg_setup async=true): a one-job mailbox with its own
// thread.  The stepper posts a step's exchange and collects its result one step later; the
// work itself comes in as a callable, so nothing here knows of HIP, RCCL or the step slots --
// host-only, tested stand-alone by tests/native/engine_host_test.cpp.
//
// The contract (the engine and phase B's device-side wait rely on every line of it):
//  - A job's sequence number is never 0 (0 in StepSlot::b_wait means "no job to wait for"):
//    the 32-bit counter skips it when it wraps.  The counter outlives stop() / start().
//  - run(q, flags, seq) does everything the job publishes, in this order: on failure (rc != 0)
//    the zeroing of the receive counts, then the release-store of seq into the flag word the
//    device polls.  It returns only after both, and never throws (it reports an exception as
//    rc -1 with its text).
//  - The result becomes collectable only after run() returned: the flag store happens before
//    any collect() hands the job's result out.
//  - One job at a time: post() is called only after collect().  collect() waits until no job
//    is queued or running, returns (0, 0) when no result is uncollected and hands each result
//    out once; rc -1 throws "exchange thread: <text>" (the result counts as handed out).
//  - stop(abort) sets stop under the lock and wakes the thread; abort is called (under the
//    lock) only when a job is queued or running.  A job queued at stop() still runs to its
//    end: the thread leaves only when woken with no job.  After the join, job, busy and result
//    are cleared, so a later start() begins clean.
//  - post / collect / wait_idle / stop / start come from one thread (the stepper); busy() and
//    last_seq() from any.
#pragma once
#include <condition_variable>
#include <functional>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>

#include "step_abi.h"

class XchgWorker {
 public:
  struct Result { int rc = 0; u32 orf = 0; std::string err; };
  using Run = std::function<Result(int q, u32 flags, u32 seq)>;

  explicit XchgWorker(u32 last_seq = 0) : seq_(last_seq) {}
  ~XchgWorker() { stop(); }

  // init (optional) runs first on the new thread
  void start(Run run, std::function<void()> init = nullptr) {
    run_ = std::move(run);
    th_ = std::thread([this, init] {
      if (init) init();
      loop();
    });
  }
  // the sequence number of the last job posted (0: none yet)
  u32 last_seq() {
    std::lock_guard<std::mutex> g(mu_);
    return seq_;
  }
  u32 post(int q, u32 flags) {
    std::lock_guard<std::mutex> g(mu_);
    q_ = q;
    flags_ = flags;
    if (++seq_ == 0) ++seq_;   // (0: no wait)
    job_ = true;
    cv_.notify_all();
    return seq_;
  }
  bool busy() {
    std::lock_guard<std::mutex> g(mu_);
    return job_ || busy_;
  }
  void wait_idle() {
    std::unique_lock<std::mutex> g(mu_);
    cv_.wait(g, [&] { return !job_ && !busy_; });
  }
  // the last job's result (waits for it); (0, 0) when none is uncollected
  void collect(int* rc, u32* orf) {
    std::unique_lock<std::mutex> g(mu_);
    cv_.wait(g, [&] { return !job_ && !busy_; });
    *rc = 0;
    *orf = 0;
    if (!has_res_) return;
    has_res_ = false;
    *rc = res_.rc;
    *orf = res_.orf;
    if (res_.rc == -1) throw std::runtime_error("exchange thread: " + res_.err);
  }
  // abort (optional): makes a job that waits for a peer give up at once
  void stop(const std::function<void()>& abort = nullptr) {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
      cv_.notify_all();
      if (abort && (job_ || busy_)) abort();
    }
    if (th_.joinable()) th_.join();
    std::lock_guard<std::mutex> g(mu_);
    stop_ = job_ = busy_ = has_res_ = false;
  }

 private:
  void loop() {
    std::unique_lock<std::mutex> g(mu_);
    while (true) {
      cv_.wait(g, [&] { return stop_ || job_; });
      if (!job_) return;
      const int q = q_;
      const u32 fl = flags_, seq = seq_;
      job_ = false;
      busy_ = true;
      g.unlock();
      Result r = run_(q, fl, seq);
      g.lock();
      busy_ = false;
      has_res_ = true;
      res_ = std::move(r);
      cv_.notify_all();
    }
  }

  std::thread th_;
  std::mutex mu_;
  std::condition_variable cv_;
  Run run_;
  bool stop_ = false, job_ = false, busy_ = false, has_res_ = false;
  int q_ = 0;
  u32 flags_ = 0, seq_ = 0;
  Result res_;
};
