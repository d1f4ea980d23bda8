// Stand-alone checks of the engine's host-only pieces: the SDMA copy plan and cuts
// (csrc/kernels/sdma_plan.h), the asynchronous-exchange worker (xchg_worker.h) and the
// side-operation mailbox (side_box.h).  Built twice by tests/test_delta_stage.py -- with
// -fsanitize=address,undefined and with -fsanitize=thread -- and run as a child process;
// exit 0 and "ok" = every check held.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "sdma_plan.h"
#include "side_box.h"
#include "xchg_worker.h"

#define CHECK(c, ...)                                            \
  do {                                                           \
    if (!(c)) {                                                  \
      std::fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #c); \
      std::fprintf(stderr, __VA_ARGS__);                         \
      std::fprintf(stderr, "\n");                                \
      std::exit(1);                                              \
    }                                                            \
  } while (0)

// ------------------------------------------------------------------ sdma_plan.h
static bool same(const SdmaPlan& p, u32 e, u32 e2, u32 t, u32 i, u32 i2) {
  return p.egress == e && p.egress2 == e2 && p.tail == t && p.ingress == i && p.ingress2 == i2;
}

static void test_plan() {
  struct Row { u32 mask; int pref, split; bool h2d; u32 want[5]; };
  const Row rows[] = {
      {0xF, -1, 1, true, {2, 0, 4, 1, 8}},    // the defaults on MI355X: egress 1, tail 2, ingress 0 and 3
      {0xF, -1, 2, true, {2, 4, 8, 1, 8}},    // (the second half shares the tail engine)
      {0xF, -1, 1, false, {2, 0, 4, 1, 0}},
      {0xF, 2, 1, true, {4, 0, 8, 1, 8}},
      {0xF, 9, 1, true, {2, 0, 4, 1, 8}},     // (a preferred engine that is not offered)
      {0x7, -1, 1, true, {2, 0, 4, 1, 4}},
      {0x7, -1, 2, true, {2, 4, 1, 1, 0}},
      {0x3, -1, 1, true, {2, 0, 1, 1, 0}},
      {0x2, -1, 1, true, {2, 0, 2, 2, 0}},
      {0x1, -1, 1, true, {1, 0, 1, 1, 0}},
      {0x8100, -1, 1, true, {0x100, 0, 0x100, 0x100, 0}},   // only slow engines: no split, nothing shared into 0..3
  };
  for (const Row& r : rows) {
    const SdmaPlan p = plan_sdma(r.mask, r.pref, r.split, r.h2d);
    CHECK(same(p, r.want[0], r.want[1], r.want[2], r.want[3], r.want[4]),
          "mask %#x pref %d split %d h2d %d: (%#x, %#x, %#x, %#x, %#x)", r.mask, r.pref, r.split, (int)r.h2d, p.egress,
          p.egress2, p.tail, p.ingress, p.ingress2);
  }
  // every availability mask x preference x option: engines come from the mask; an ingress half
  // never queues behind a gated egress copy or the other half; no second engine unless asked
  auto one_of = [](u32 e, u32 mask) { return e == 0 || ((e & mask) && !(e & (e - 1))); };
  for (u32 mask = 1; mask <= 0xFFFF; ++mask)
    for (int pref = -1; pref <= 15; ++pref)
      for (int split = 1; split <= 2; ++split)
        for (int h2d = 0; h2d <= 1; ++h2d) {
          const SdmaPlan p = plan_sdma(mask, pref, split, h2d != 0);
          const bool ok = p.egress && p.tail && p.ingress && one_of(p.egress, mask) && one_of(p.egress2, mask) &&
                          one_of(p.tail, mask) && one_of(p.ingress, mask) && one_of(p.ingress2, mask) &&
                          (!p.ingress2 || (p.ingress2 != p.egress && p.ingress2 != p.egress2 && p.ingress2 != p.ingress)) &&
                          (h2d || !p.ingress2) && (split > 1 || !p.egress2);
          CHECK(ok, "mask %#x pref %d split %d h2d %d: (%#x, %#x, %#x, %#x, %#x)", mask, pref, split, h2d, p.egress,
                p.egress2, p.tail, p.ingress, p.ingress2);
        }
}

static void test_cuts() {
  const u64 MB4 = 4ull << 20;
  CHECK(ingress_cut(8192, 1, true) == 8192, "8192 stays whole");
  CHECK(ingress_cut(8193, 1, true) == 4096, "8193 = 4096 + 4097");
  CHECK(ingress_cut(12296, 1, true) == 8192, "12296: half rounded up to 4 KB");
  CHECK(ingress_cut(MB4, MB4, true) == MB4 / 2, "4 MB in two equal halves");
  CHECK(ingress_cut(MB4 - 1, MB4, true) == MB4 - 1, "one byte below split_min stays whole");
  CHECK(ingress_cut(MB4, MB4, false) == MB4, "no second engine: whole");
  CHECK(ingress_cut(0, 0, true) == 0, "empty");
  for (u64 len : std::vector<u64>{8193, 12296, 65537, MB4 + 4097, (64ull << 20) - 1}) {
    const u64 h = ingress_cut(len, 1, true);
    CHECK(h % 4096 == 0 && h > 0 && h < len && 2 * h + 1 >= len && 2 * h < len + 8192, "cut of %llu at %llu",
          (unsigned long long)len, (unsigned long long)h);
  }
  CHECK(egress_cut(2u << 20, 2) == 1u << 20, "2 MB on two engines");
  CHECK(egress_cut(2u << 20, 1) == 2u << 20, "2 MB on one engine");
  CHECK(egress_cut((2u << 20) + 4097, 2) == 1u << 20, "odd length: half rounded down to 4 KB");
  CHECK(egress_cut((2u << 20) + 12345, 2) == (1u << 20) + 4096, "odd length: half rounded down to 4 KB");
  CHECK(egress_cut(8191, 2) == 0, "below 8 KB the first part is empty");
  const u64 none[4] = {0, 0, 0, 0}, one[4] = {0, 1, 0, 0}, big[4] = {5, 100ull << 20, 7, 9}, exact[4] = {0, 0, 0, 983040};
  CHECK(spec_bytes(none, 1ull << 30) == 0, "no egress in the last four steps");
  CHECK(spec_bytes(one, 1ull << 30) == 131072, "1 byte: + 64 KB, rounded up to 64 KB");
  CHECK(spec_bytes(big, 96ull << 20) == 96ull << 20, "capped at the allocation");
  CHECK(spec_bytes(big, 1ull << 30) == ((100ull << 20) + (100ull << 20) / 16 + 65536 + 65535) / 65536 * 65536, "largest + 1/16 + 64 KB");
  // 983040 = 15 * 64 KB, + 1/16 = 61440, + 64 KB = 1110016 -> 17 * 64 KB
  CHECK(spec_bytes(exact, 1ull << 30) == 17ull * 65536, "a multiple of 64 KB");
  const u64 m64[4] = {1048576, 0, 0, 0};   // 16 * 64 KB + 64 KB (1/16) + 64 KB: no rounding left
  CHECK(spec_bytes(m64, 1ull << 30) == 18ull * 65536, "an exact sum is not rounded further");
}

// ------------------------------------------------------------------ xchg_worker.h
// What the engine's job does (Engine::x_run), on plain memory: the work, on failure the zeroing
// of the receive counts, then the release-store of the job's number into the flag word
struct Exchange {
  std::mutex mu;
  std::vector<std::string> log;         // the order of the job's side effects
  std::atomic<u32> flag{0};             // what phase B's device-side wait polls
  u32 counts = 0;                       // the receive counts phase B imports (ordered by flag)
  std::function<int(u32 flags)> work = [](u32) { return 0; };
  std::atomic<int> ran{0};

  void note(const char* what) {
    std::lock_guard<std::mutex> g(mu);
    log.push_back(what);
  }
  XchgWorker::Result run(int, u32 flags, u32 seq) {
    XchgWorker::Result r;
    try {
      r.rc = work(flags);
      r.orf = flags | 0x100;
      if (!r.rc) counts = 5;
    } catch (const std::exception& e) {
      r.rc = -1;
      r.err = e.what();
    }
    if (r.rc) {
      counts = 0;
      note("zero");
    }
    flag.store(seq, std::memory_order_release);
    note("flag");
    ++ran;
    return r;
  }
  XchgWorker::Run fn() {
    return [this](int q, u32 fl, u32 seq) { return run(q, fl, seq); };
  }
};

static void test_worker_order() {
  Exchange x;
  XchgWorker w;
  int rc = 9;
  u32 orf = 9;
  w.collect(&rc, &orf);   // nothing posted, no thread: at once
  CHECK(rc == 0 && orf == 0, "collect with nothing posted");
  w.start(x.fn());
  w.collect(&rc, &orf);
  CHECK(rc == 0 && orf == 0 && !w.busy(), "collect with nothing posted (thread running)");
  // success: while the job runs it is not collectable; the flag is stored before it is
  std::atomic<bool> entered{false}, go{false};
  x.work = [&](u32) {
    entered = true;
    while (!go) std::this_thread::yield();
    return 0;
  };
  const u32 s1 = w.post(0, 3);
  CHECK(s1 == 1 && w.last_seq() == 1, "first job number %u", s1);
  while (!entered) std::this_thread::yield();
  CHECK(w.busy() && x.flag.load() == 0, "a running job is busy and has not published");
  go = true;
  w.collect(&rc, &orf);
  x.note("collected");
  CHECK(rc == 0 && orf == 0x103, "result (%d, %#x)", rc, orf);
  CHECK(x.flag.load(std::memory_order_acquire) == s1 && x.counts == 5, "flag %u counts %u", x.flag.load(), x.counts);
  CHECK((x.log == std::vector<std::string>{"flag", "collected"}), "order on success");
  w.collect(&rc, &orf);
  CHECK(rc == 0 && orf == 0, "a result is handed out once");
  // failure (rc -2): zeroing, flag store, then collectable; a poller of the flag (phase B's
  // wait) finds the counts zeroed
  x.log.clear();
  x.counts = 77;
  x.work = [](u32) { return -2; };
  u32 seen_counts = 99;
  const u32 s2 = w.post(1, 0);
  std::thread dev([&] {
    while (x.flag.load(std::memory_order_acquire) != s2) std::this_thread::yield();
    seen_counts = x.counts;
  });
  w.collect(&rc, &orf);
  x.note("collected");
  dev.join();
  CHECK(rc == -2 && s2 == 2, "result %d of job %u", rc, s2);
  CHECK(seen_counts == 0, "phase B would import %u", seen_counts);
  CHECK((x.log == std::vector<std::string>{"zero", "flag", "collected"}), "order on failure");
  // a throwing job: rc -1, collect throws with its text, once
  x.log.clear();
  x.work = [](u32) -> int { throw std::runtime_error("peer lost"); };
  const u32 s3 = w.post(0, 0);
  std::string what;
  try { w.collect(&rc, &orf); } catch (const std::runtime_error& e) { what = e.what(); }
  CHECK(what == "exchange thread: peer lost", "collect threw '%s'", what.c_str());
  CHECK(x.flag.load() == s3 && (x.log == std::vector<std::string>{"zero", "flag"}), "a throwing job still publishes");
  w.collect(&rc, &orf);
  CHECK(rc == 0 && orf == 0, "the thrown result is not handed out again");
  w.stop();
}

static void test_worker_rounds() {
  Exchange x;
  XchgWorker w;
  w.start(x.fn());
  u32 last = 0;
  for (u32 k = 0; k < 2000; ++k) {
    const u32 seq = w.post((int)(k & 1), k);
    CHECK(seq == last + 1, "job numbers count up: %u after %u", seq, last);
    last = seq;
    int rc = -9;
    u32 orf = 0;
    w.collect(&rc, &orf);
    CHECK(rc == 0 && orf == (k | 0x100) && x.flag.load(std::memory_order_acquire) == seq && !w.busy(), "round %u", k);
  }
  CHECK(x.ran == 2000, "%d jobs ran", x.ran.load());
  w.stop();
}

static void test_worker_wrap() {
  Exchange x;
  XchgWorker w(0xFFFFFFFEu);
  w.start(x.fn());
  const u32 want[4] = {0xFFFFFFFFu, 1, 2, 3};
  for (u32 k = 0; k < 4; ++k) {
    const u32 seq = w.post(0, 0);
    int rc;
    u32 orf;
    w.collect(&rc, &orf);
    CHECK(seq != 0 && seq == want[k] && x.flag.load() == seq && w.last_seq() == seq, "job %u numbered %u", k, seq);
  }
  w.stop();
}

static void test_worker_stop() {
  Exchange x;
  XchgWorker w;
  int aborts = 0, rc = 0;
  u32 orf = 0;
  const std::function<void()> abort_fn = [&] { ++aborts; };
  w.stop(abort_fn);   // never started
  CHECK(aborts == 0, "abort with no thread");
  w.start(x.fn());
  w.stop(abort_fn);   // nothing in flight
  CHECK(aborts == 0, "abort with nothing in flight");
  // a job that blocks until the abort function releases it
  std::atomic<bool> entered{false}, gave_up{false};
  x.work = [&](u32) {
    entered = true;
    while (!gave_up) std::this_thread::yield();
    return -2;
  };
  w.start(x.fn());
  w.post(0, 0);
  while (!entered) std::this_thread::yield();
  w.stop([&] { ++aborts; gave_up = true; });
  CHECK(aborts == 1 && x.ran == 1, "abort called %d times, %d jobs ended", aborts, x.ran.load());
  CHECK(!w.busy(), "idle after stop");
  w.collect(&rc, &orf);
  CHECK(rc == 0 && orf == 0, "stop left a stale result (%d)", rc);
  // start after stop: works, the numbering goes on
  x.work = [](u32) { return 0; };
  w.start(x.fn());
  const u32 seq = w.post(1, 4);
  w.collect(&rc, &orf);
  CHECK(seq == 2 && rc == 0 && orf == 0x104, "job %u after a restart: (%d, %#x)", seq, rc, orf);
  // stop without abort right behind a post: the job runs to its end
  w.post(0, 0);
  w.stop();
  CHECK(x.ran == 3, "a job posted before stop() did not run (%d)", x.ran.load());
  w.collect(&rc, &orf);
  CHECK(rc == 0 && orf == 0, "stop left a stale result");
  // the same with the job certainly still queued when stop is set: the thread is held in its
  // init until the abort function (called under the lock, stop already set) lets it go
  std::atomic<bool> go{false};
  w.start(x.fn(), [&] { while (!go) std::this_thread::yield(); });
  w.post(0, 0);
  w.stop([&] { ++aborts; go = true; });
  CHECK(aborts == 2 && x.ran == 4, "a job queued at stop() did not run (%d jobs, %d aborts)", x.ran.load(), aborts);
}

// ------------------------------------------------------------------ side_box.h
static void test_box_states() {
  using clock = std::chrono::steady_clock;
  SideBox b;
  bool threw = false;
  CHECK(!b.pending() && !b.queued() && !b.begin_launch(), "an empty box");
  try { b.wait_launched(clock::now()); } catch (const std::runtime_error& e) { threw = std::string(e.what()) == "side_wait: nothing posted"; }
  CHECK(threw, "wait_launched on an empty box");
  int fills = 0;
  b.post(SideOp{2, 1, 2, 3, 4, 5, 6}, [&] { ++fills; });
  CHECK(fills == 1 && b.pending() && b.queued(), "posted");
  threw = false;
  try { b.post(SideOp{3, 0, 0, 0, 0, 0, 0}, [&] { ++fills; }); } catch (const std::runtime_error& e) {
    threw = std::string(e.what()) == "side operation pending (side_wait first)";
  }
  CHECK(threw && fills == 1, "a second post must throw before it fills");
  CHECK(b.wait_launched(clock::now() + std::chrono::milliseconds(2)) == 0, "not launched: times out");
  threw = false;
  try { b.clear(); } catch (const std::logic_error&) { threw = true; }
  CHECK(threw && b.pending(), "clear before the launch");
  const std::optional<SideOp> op = b.begin_launch();
  CHECK(op && op->kind == 2 && op->a == 1 && op->b == 2 && op->c == 3 && op->max_n == 4 && op->max_bytes == 5 && op->n == 6,
        "the posted operation comes out as it went in");
  CHECK(b.queued(), "queued until launched()");
  b.launched();
  CHECK(b.pending() && !b.queued() && !b.begin_launch(), "launched");
  CHECK(b.wait_launched(clock::now()) == 2, "launched: its kind, even at the deadline");
  threw = false;
  try { b.post(SideOp{3, 0, 0, 0, 0, 0, 0}); } catch (const std::runtime_error&) { threw = true; }
  CHECK(threw, "a post before the result was taken");
  b.clear();
  CHECK(!b.pending() && !b.queued() && !b.begin_launch(), "empty again");
  threw = false;
  try { b.clear(); } catch (const std::logic_error&) { threw = true; }
  CHECK(threw, "clear of an empty box");
  b.post(SideOp{5, 0, 0, 0, 0, 0, 0});
  CHECK(b.queued(), "posted again");
}

static void test_box_rounds() {
  SideBox b;
  u64 records = 0, result = 0;   // plain memory the box's states order (the engine's side_h_)
  std::atomic<bool> done{false};
  std::thread launcher([&] {
    while (!done) {
      const std::optional<SideOp> op = b.begin_launch();
      if (!op) { std::this_thread::yield(); continue; }
      result = records * 2 + op->a;
      b.launched();
    }
  });
  for (u32 k = 1; k <= 2000; ++k) {
    b.post(SideOp{1 + (int)(k % 5), k, 0, 0, 0, 0, 0}, [&] { records = 3ull * k; });
    int kind = 0;
    while (!kind) kind = b.wait_launched(std::chrono::steady_clock::now() + std::chrono::seconds(1));
    CHECK(kind == 1 + (int)(k % 5) && result == 7ull * k, "round %u: kind %d result %llu", k, kind, (unsigned long long)result);
    b.clear();
  }
  done = true;
  launcher.join();
  CHECK(!b.pending(), "empty at the end");
}

int main() {
  test_plan();
  test_cuts();
  test_worker_order();
  test_worker_rounds();
  test_worker_wrap();
  test_worker_stop();
  test_box_states();
  test_box_rounds();
  std::puts("ok");
  return 0;
}
