// Stand-alone check of the deferred control-write stager (csrc/kernels/delta_stage.h): a
// seeded random mix of stage_write / stage_begin / stage_end / stage_unpause /
// stage_mark_dirty / pack_deltas against a byte array standing in for device memory, next to
// a model that mirrors the batches.  Built with -fsanitize=address,undefined by
// tests/test_delta_stage.py and run as a child process; exit 0 and "ok" = every check held.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <map>
#include <random>
#include <vector>

#include "delta_stage.h"
#include "step_abi.h"

static constexpr u32 MEM = 64u << 10;             // the stand-in for device memory
static constexpr u64 BASE = 0x7f0000000000ull;    // its "device address"
static constexpr u32 N_CONN = 64, N_CH = 512;

#define CHECK(c, ...)                                            \
  do {                                                           \
    if (!(c)) {                                                  \
      std::fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #c); \
      std::fprintf(stderr, __VA_ARGS__);                         \
      std::fprintf(stderr, "\n");                                \
      std::exit(1);                                              \
    }                                                            \
  } while (0)

// what one batch of the stager must still hold: per byte the last value staged into it
struct ModelBatch {
  u64 id = 0;
  bool open = false;
  std::map<u32, u8> bytes;
  std::vector<u32> dirty, unp;
  bool empty() const { return bytes.empty() && dirty.empty(); }
};

struct Harness {
  DeltaStage ds;
  std::vector<u8> dev = std::vector<u8>(MEM, 0);     // records applied as k_stage would
  std::vector<u8> naive = std::vector<u8>(MEM, 0);   // every write in call order, last wins
  std::deque<ModelBatch> mb;
  std::vector<u32> ready;      // unpauses of batches a flush applied (the next step's)
  u32 open_cnt = 0;
  u64 next_id = 1, taken = 0;  // taken: last dl_state(1)
  u32 max_nrec = 0;
  std::vector<u64> outbuf = std::vector<u64>(DELTA_CAP / 8);   // (16-byte aligned by operator new)
  std::vector<u32> unpbuf = std::vector<u32>(UNPAUSE_STEP_MAX);
  std::mt19937 rng;

  explicit Harness(u32 seed) : rng(seed) {}
  u32 rnd(u32 n) { return (u32)(rng() % n); }

  void new_batch() {
    mb.emplace_back();
    mb.back().open = open_cnt > 0;
    mb.back().id = next_id++;
  }
  // the batch staging goes into: never a closed batch with nothing in it (it counts as taken)
  ModelBatch& staging() {
    if (!mb.empty() && !mb.back().open && mb.back().empty() && mb.back().unp.empty()) mb.pop_back();
    if (mb.empty()) new_batch();
    return mb.back();
  }
  static bool has(const std::vector<u32>& v, u32 x) { return std::find(v.begin(), v.end(), x) != v.end(); }

  // the stager's own view agrees with the mirror; dl_state(1) never decreases (6)
  void check_state() {
    CHECK(ds.dl_state(3) == mb.size(), "batches %llu vs %zu", (unsigned long long)ds.dl_state(3), mb.size());
    CHECK(ds.dl_state(2) == open_cnt, "open sections");
    const u64 cur = (!mb.empty() && mb.back().open) ? mb.back().id : 0;
    CHECK(ds.dl_state(0) == cur, "staging batch id %llu vs %llu", (unsigned long long)ds.dl_state(0), (unsigned long long)cur);
    const u64 t = ds.dl_state(1);
    CHECK(t >= taken, "dl_state(1) went back: %llu after %llu", (unsigned long long)t, (unsigned long long)taken);
    taken = t;
    size_t nrec = 0, nd = 0, want_b = 0, want_d = 0;
    u64 nb = 0;
    ds.deltas_pending(&nrec, &nb, &nd);
    for (auto& b : mb) { want_b += b.bytes.size(); want_d += b.dirty.size(); }
    CHECK(nb == want_b && nd == want_d, "deltas_pending (%llu B, %zu ch) vs model (%zu B, %zu ch)", (unsigned long long)nb, nd,
          want_b, want_d);
    CHECK((nrec == 0) == (want_b == 0), "records pending");
  }

  void write(u32 off, u32 n) {
    std::vector<u8> data(n);
    for (u32 i = 0; i < n; ++i) data[i] = (u8)rng();
    ds.stage_write(BASE + off, data.data(), n);
    ModelBatch& b = staging();
    for (u32 i = 0; i < n; ++i) {
      b.bytes[off + i] = data[i];
      naive[off + i] = data[i];
    }
  }
  void begin() {
    ds.stage_begin();
    ++open_cnt;
    if (mb.empty() || !mb.back().open) new_batch();
  }
  void end() {
    ds.stage_end();
    if (open_cnt) --open_cnt;
    if (!open_cnt)
      for (auto& b : mb) b.open = false;
  }
  void unpause(u32 conn) {
    ds.stage_unpause(conn);
    ModelBatch& b = staging();
    if (!has(b.unp, conn)) b.unp.push_back(conn);
  }
  void mark_dirty(u32 ch) {
    ds.stage_mark_dirty(ch);
    ModelBatch& b = staging();
    if (!has(b.dirty, ch)) b.dirty.push_back(ch);
  }

  // step: the form a submitted step uses (unpause list out); else flush_deltas' form
  u32 pack(bool step) {
    u8* out = (u8*)outbuf.data();
    u32 nunp = 0;
    const u32 used = ds.pack_deltas(out, step ? unpbuf.data() : nullptr, step ? &nunp : nullptr);
    CHECK(used <= DELTA_CAP, "bytes used %u", used);   // (3)
    if (used) {
      const DeltaHead h = *(const DeltaHead*)out;
      CHECK(h.nrec <= DELTA_REC_MAX, "nrec %u", h.nrec);   // (3)
      max_nrec = std::max(max_nrec, h.nrec);
      const DeltaRec* recs = (const DeltaRec*)(out + sizeof(DeltaHead));
      const u32* dirty = (const u32*)(recs + h.nrec);
      const u8* data = (const u8*)dirty + ((4u * h.ndirty + 15u) & ~15u);
      CHECK((u64)(data - out) + 16ull * h.nchunk == used, "layout ends at %llu, used %u",
            (unsigned long long)((data - out) + 16ull * h.nchunk), used);
      CHECK(h.nrec || h.ndirty, "a packed buffer with nothing in it");
      // records: chunks in order, inside the memory, no two overlapping (2)
      std::vector<u8> seen(MEM, 0);
      u32 c = 0;
      for (u32 r = 0; r < h.nrec; ++r) {
        CHECK(recs[r].chunk0 == c && recs[r].len > 0, "record %u chunk0 %u (expected %u) len %u", r, recs[r].chunk0, c,
              recs[r].len);
        c += (recs[r].len + 15) / 16;
        CHECK(recs[r].dst >= BASE && recs[r].dst + recs[r].len <= BASE + MEM, "record %u outside the memory", r);
        for (u32 i = 0; i < recs[r].len; ++i) {
          u8& s = seen[recs[r].dst - BASE + i];
          CHECK(!s, "records overlap at byte %llu", (unsigned long long)(recs[r].dst - BASE + i));
          s = 1;
        }
      }
      CHECK(c == h.nchunk, "nchunk %u, records cover %u", h.nchunk, c);
      // apply the way apply_deltas does: chunk i belongs to the last record with chunk0 <= i,
      // clipped to its length
      for (u32 i = 0; i < h.nchunk; ++i) {
        u32 lo = 0, hi = h.nrec;
        while (hi - lo > 1) {
          const u32 mid = (lo + hi) >> 1;
          if (recs[mid].chunk0 <= i) lo = mid; else hi = mid;
        }
        const DeltaRec& r = recs[lo];
        const u32 off = (i - r.chunk0) * 16u;
        const u32 n = r.len - off < 16u ? r.len - off : 16u;
        for (u32 k = 0; k < n; ++k) {
          const u32 a = (u32)(r.dst - BASE) + off + k;
          dev[a] = data[16ull * i + k];
          take_byte(a, dev[a], step);
        }
      }
      for (u32 k = 0; k < h.ndirty; ++k) take_dirty(dirty[k], step);
    }
    for (u32 k = 0; k < nunp; ++k) take_unpause(unpbuf[k]);
    // batches the stager dropped: leading ones, whole
    const u64 left = ds.dl_state(3);
    CHECK(left <= mb.size(), "more batches than staged");
    while (mb.size() > left) {
      ModelBatch& b = mb.front();
      CHECK(b.empty(), "batch %llu dropped with %zu bytes / %zu channels unpacked", (unsigned long long)b.id, b.bytes.size(),
            b.dirty.size());
      CHECK(!step || b.unp.empty(), "batch %llu dropped by a step that left %zu of its unpauses behind",
            (unsigned long long)b.id, b.unp.size());
      ready.insert(ready.end(), b.unp.begin(), b.unp.end());   // (flush form: the next step's)
      mb.pop_front();
    }
    check_state();
    return used;
  }
  // a byte that came out: the oldest batch holding that address staged exactly this value,
  // and a step never takes it from an open batch (4)
  void take_byte(u32 a, u8 v, bool step) {
    for (auto& b : mb) {
      auto it = b.bytes.find(a);
      if (it == b.bytes.end()) continue;
      CHECK(!(step && b.open), "a step took byte %u from open batch %llu", a, (unsigned long long)b.id);
      CHECK(it->second == v, "byte %u: %u packed, %u staged in batch %llu", a, v, it->second, (unsigned long long)b.id);
      b.bytes.erase(it);
      return;
    }
    CHECK(false, "byte %u packed but staged nowhere", a);
  }
  void take_dirty(u32 ch, bool step) {
    for (auto& b : mb) {
      auto it = std::find(b.dirty.begin(), b.dirty.end(), ch);
      if (it == b.dirty.end()) continue;
      CHECK(!(step && b.open), "a step took channel %u from open batch %llu", ch, (unsigned long long)b.id);
      b.dirty.erase(it);
      return;
    }
    CHECK(false, "channel %u packed but staged nowhere", ch);
  }
  // an unpause that came out with a step: from a flushed batch, or from the oldest batch
  // staging it -- closed (4) and with its last record out already (5)
  void take_unpause(u32 conn) {
    auto rt = std::find(ready.begin(), ready.end(), conn);
    if (rt != ready.end()) { ready.erase(rt); return; }
    for (auto& b : mb) {
      auto it = std::find(b.unp.begin(), b.unp.end(), conn);
      if (it == b.unp.end()) continue;
      CHECK(!b.open, "a step took the unpause of %u from open batch %llu", conn, (unsigned long long)b.id);
      CHECK(b.empty(), "unpause of %u out before batch %llu's last record (%zu bytes, %zu channels left)", conn,
            (unsigned long long)b.id, b.bytes.size(), b.dirty.size());
      b.unp.erase(it);
      return;
    }
    CHECK(false, "connection %u unpaused but staged nowhere", conn);
  }

  void random_ops(u32 n_ops) {
    for (u32 k = 0; k < n_ops; ++k) {
      const u32 op = rnd(100);
      if (op < 55) {
        const u32 n = 1 + rnd(rnd(8) ? 300 : 4);
        const u32 off = rnd(4) ? rnd(MEM - n + 1) : std::min<u32>(rnd(2048), MEM - n);   // (a crowded corner: overlaps)
        write(off, n);
      } else if (op < 62) {
        if (open_cnt < 3) begin();
      } else if (op < 70) {
        end();   // (also with no section open: ignored)
      } else if (op < 78) {
        unpause(rnd(N_CONN));
      } else if (op < 84) {
        mark_dirty(rnd(N_CH));
      } else if (op < 97) {
        pack(true);
      } else {
        pack(false);
      }
      check_state();
    }
  }

  // close every section, let steps carry the rest: memory == naive model (1)
  void drain() {
    while (open_cnt) end();
    for (u32 k = 0; ds.host_work() || ds.has_deltas(); ++k) {
      CHECK(k < 100000, "the drain does not end");
      pack(true);
    }
    CHECK(mb.empty() || (mb.size() == 1 && mb.front().empty() && mb.front().unp.empty()), "%zu batches left", mb.size());
    CHECK(ready.empty(), "%zu flushed unpauses never came out", ready.size());
    CHECK(dev == naive, "memory differs from the naive model");
  }
};

int main() {
  {   // (7) one record must fit a step's buffer with its header
    DeltaStage ds;
    std::vector<u8> big(DELTA_CAP - 63, 1);
    bool threw = false;
    try { ds.stage_write(BASE, big.data(), big.size()); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw, "a write of DELTA_CAP - 63 bytes was accepted");
    CHECK(!ds.has_deltas() && !ds.host_work(), "the refused write left something staged");
  }
  {   // more records than one step takes, in one batch and in a section's: cut at DELTA_REC_MAX
    Harness h(7);
    for (u32 i = 0; i < 3000; ++i) h.write(2 * i, 1);
    h.unpause(3);
    h.begin();
    for (u32 i = 0; i < 1500; ++i) h.write(8192 + 3 * i, 2);
    h.unpause(4);
    h.pack(true);
    h.end();
    h.drain();
    CHECK(h.max_nrec == DELTA_REC_MAX, "the record limit was never reached (%u)", h.max_nrec);
  }
  for (u32 seed = 1; seed <= 6; ++seed) {
    Harness h(seed);
    h.random_ops(4000);
    h.drain();
  }
  std::puts("ok");
  return 0;
}
