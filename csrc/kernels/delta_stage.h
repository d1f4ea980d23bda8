// Deferred control writes (no pipeline drain): the control plane stages table writes while
// steps run; the next submitted step carries them (k_stage applies them first).  Pure host
// logic over the step ABI's delta records -- no HIP, no Python: the engine packs into a
// parity's host-mapped delta buffer, tests/native/delta_stage_test.cpp into plain memory.
// Any thread.  Writes to the same bytes: the last one wins (records never overlap).
#pragma once
#include <algorithm>
#include <cstring>
#include <deque>
#include <iterator>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "step_abi.h"

static constexpr u64 DELTA_CAP = 4ull << 20;   // one step's delta buffer (head, records, channels, data)

class DeltaStage {
 public:
  // guards everything below and the engine's spill request words (Engine::stage_spill)
  std::mutex mu;

  // dst: device address; an earlier staged write to the same bytes is cut to what remains
  void stage_write(u64 dst, const u8* data, u64 n) {
    if (!n) return;
    // one record must fit a step's delta buffer with its header (a larger one
    // was never packed and kept the stepper spinning on host_work)
    if (n + 64 > DELTA_CAP) throw std::runtime_error("stage_write: a write larger than one step's delta buffer");
    std::lock_guard<std::mutex> g(mu);
    Batch& bt = staging();
    const u64 a = dst, e = dst + n;
    auto it = bt.w.lower_bound(a);
    if (it != bt.w.begin()) --it;
    std::vector<std::pair<u64, std::string>> keep;
    while (it != bt.w.end() && it->first < e) {
      const u64 s0 = it->first, s1 = s0 + it->second.size();
      if (s1 <= a) { ++it; continue; }
      if (s0 < a) keep.emplace_back(s0, it->second.substr(0, a - s0));
      if (s1 > e) keep.emplace_back(e, it->second.substr(e - s0));
      bytes_ -= it->second.size();
      it = bt.w.erase(it);
    }
    for (auto& kv : keep) {
      bytes_ += kv.second.size();
      bt.w.emplace(kv.first, std::move(kv.second));
    }
    bt.w.emplace(a, std::string((const char*)data, n));
    bytes_ += n;
  }
  void stage_mark_dirty(u32 ch) {
    std::lock_guard<std::mutex> g(mu);
    add_once(staging().dirty, ch);
  }
  // a paused connection (its control command answered) resumes with the next submitted
  // step: k_stage clears its flag before the frame scan reads it, so the host never writes
  // device state while steps are in flight
  void stage_unpause(u32 conn) {
    std::lock_guard<std::mutex> g(mu);
    add_once(staging().unp, conn);   // with the writes staged before it
  }
  // a light control section's staging: everything staged until stage_end() forms one batch
  // that no step takes before the section closed it (a step packing in the middle of a
  // section split a command's consumer rows and q_cons lists over two steps)
  void stage_begin() {
    std::lock_guard<std::mutex> g(mu);
    ++open_;
    if (dl_.empty() || !dl_.back().open) new_batch();
  }
  void stage_end() {
    std::lock_guard<std::mutex> g(mu);
    if (open_) --open_;
    if (!open_)
      for (auto& bt : dl_) bt.open = false;
  }
  // batch ids (light sections tie their replies to them, Frontend::send_after): 0 = the
  // batch staging goes into now (the next one to be created when none is open), 1 = every
  // batch up to this id was taken by a submitted step (or applied by flush_deltas)
  u64 dl_state(int which) {
    std::lock_guard<std::mutex> g(mu);
    if (which == 2) return open_;      // (diagnostics: open light sections, batches queued)
    if (which == 3) return dl_.size();
    if (which == 1) {   // (closed batches with nothing in them count as taken: no step needs to carry them)
      for (auto& bt : dl_)
        if (bt.open || !bt.w.empty() || !bt.dirty.empty() || !bt.unp.empty()) return bt.id - 1;
      return next_id_ - 1;
    }
    // outside a light section nothing is staged for the caller: no batch to wait for
    return (!dl_.empty() && dl_.back().open) ? dl_.back().id : 0;
  }
  // (records, data bytes, channels to mark) staged and not yet taken by a step
  void deltas_pending(size_t* nrec, u64* nbytes, size_t* ndirty) {
    std::lock_guard<std::mutex> g(mu);
    *nrec = *ndirty = 0;
    for (auto& bt : dl_) { *nrec += bt.w.size(); *ndirty += bt.dirty.size(); }
    *nbytes = bytes_;
  }
  // something a step should carry even without client bytes: applied batches' unpauses or a
  // closed batch with content
  bool host_work() {
    std::lock_guard<std::mutex> g(mu);
    if (!unp_ready_.empty()) return true;
    for (auto& bt : dl_) {
      if (bt.open) break;   // (staged by a section still running: stage_end wakes the stepper)
      if (!bt.w.empty() || !bt.dirty.empty() || !bt.unp.empty()) return true;
    }
    return false;
  }
  bool has_deltas() {
    std::lock_guard<std::mutex> g(mu);
    for (auto& bt : dl_)
      if (!bt.w.empty() || !bt.dirty.empty()) return true;
    return false;
  }
  // staged batches, oldest first, into one step's delta buffer `out` (DELTA_CAP bytes): bytes
  // used (0 = none).  The oldest batch may go in part (what does not fit -- records or bytes
  // -- stays for a later step; records are independent bytes, and the control plane keeps a
  // change set within one step by cutting its batches at deltas_pending() limits); later
  // closed batches ride the same step whole, as long as they fit and write no byte an earlier
  // record of the step writes (k_apply_deltas applies a step's records in parallel).  One
  // batch per step capped the light sections at the step rate: under connection / RPC
  // churn on a slower (durable) broker they queued up until a full pause flushed them.
  // A batch's unpauses go with its last records to unp (at most UNPAUSE_STEP_MAX, *nunp) or,
  // with unp null (flush_deltas: no step), to unp_ready_ for the next submitted step.
  u32 pack_deltas(u8* out, u32* unp, u32* nunp) {
    std::lock_guard<std::mutex> g(mu);
    u32 nu = 0;
    auto take_unp = [&](std::vector<u32>& v) {
      size_t k = 0;
      for (; k < v.size(); ++k) {
        if (!unp) { unp_ready_.push_back(v[k]); continue; }
        if (nu == UNPAUSE_STEP_MAX) break;
        unp[nu++] = v[k];
      }
      v.erase(v.begin(), v.begin() + k);
    };
    auto done = [&](u32 r) { if (nunp) *nunp = nu; return r; };
    if (unp) take_unp(unp_ready_);
    // a step (unp set) never takes a batch a light section is still staging into;
    // flush_deltas (between steps, the control plane holds the engine) takes everything
    auto usable = [&](const Batch& bt) { return !(unp && bt.open); };
    // leading batches with no writes: their unpauses only
    while (!dl_.empty() && usable(dl_.front()) && dl_.front().w.empty() && dl_.front().dirty.empty()) {
      take_unp(dl_.front().unp);
      if (!dl_.front().unp.empty()) return done(0);   // (the step's unpause list is full)
      if (dl_.size() == 1 && dl_.front().open) { dl_.pop_front(); break; }
      dl_.pop_front();
    }
    if (dl_.empty() || !usable(dl_.front()) || (dl_.front().w.empty() && dl_.front().dirty.empty())) return done(0);
    // ---- plan: how many records of the first batch, then which whole batches follow
    u64 nrec = 0, nchunk = 0, ndirty = 0;
    std::map<u64, u64> iv;   // byte ranges [dst, end) written by the records planned so far
    auto overlaps = [&](u64 d0, u64 d1) {
      auto it = iv.lower_bound(d0);
      if (it != iv.end() && it->first < d1) return true;
      if (it != iv.begin() && std::prev(it)->second > d0) return true;
      return false;
    };
    auto need = [&](u64 r, u64 dn, u64 ch) { return 16 + 16 * r + ((4 * dn + 15) & ~15ull) + 16 * ch; };
    Batch& b0 = dl_.front();
    const u64 nd0 = std::min<u64>(b0.dirty.size(), 4096);
    u64 n0 = 0;
    for (auto& kv : b0.w) {
      const u64 ch = (kv.second.size() + 15) / 16;
      if (nrec == DELTA_REC_MAX || need(nrec + 1, nd0, nchunk + ch) > DELTA_CAP) break;
      ++nrec;
      nchunk += ch;
      iv[kv.first] = kv.first + kv.second.size();
      ++n0;
    }
    ndirty = nd0;
    size_t nwhole = 0;   // later batches taken whole
    if (n0 == b0.w.size() && nd0 == b0.dirty.size() && b0.unp.size() + nu <= UNPAUSE_STEP_MAX) {
      u32 nu_plan = nu + (u32)b0.unp.size();
      for (size_t k = 1; k < dl_.size(); ++k) {
        Batch& bt = dl_[k];
        if (!usable(bt)) break;
        u64 r = nrec, ch = nchunk;
        const u64 dn = ndirty + bt.dirty.size();
        bool ok = dn <= 4096 && nu_plan + bt.unp.size() <= UNPAUSE_STEP_MAX;
        for (auto it = bt.w.begin(); ok && it != bt.w.end(); ++it) {
          ++r;
          ch += (it->second.size() + 15) / 16;
          ok = r <= DELTA_REC_MAX && need(r, dn, ch) <= DELTA_CAP &&
               !overlaps(it->first, it->first + it->second.size());
        }
        if (!ok) break;
        for (auto& kv : bt.w) iv[kv.first] = kv.first + kv.second.size();
        nrec = r;
        nchunk = ch;
        ndirty = dn;
        nu_plan += (u32)bt.unp.size();
        ++nwhole;
      }
    }
    // ---- write: head, records, dirty channels, data
    DeltaHead* h = (DeltaHead*)out;
    h->nrec = (u32)nrec; h->ndirty = (u32)ndirty; h->nchunk = (u32)nchunk; h->pad = 0;
    DeltaRec* recs = (DeltaRec*)(out + sizeof(DeltaHead));
    u32* dirty = (u32*)(recs + nrec);
    u8* data = (u8*)dirty + ((4ull * ndirty + 15) & ~15ull);
    u64 r = 0, c = 0, di = 0;
    auto put = [&](Batch& bt, u64 nr, u64 ndr) {
      u64 k = 0;
      for (auto it = bt.w.begin(); it != bt.w.end() && k < nr; ++k) {
        recs[r].dst = it->first;
        recs[r].len = (u32)it->second.size();
        recs[r].chunk0 = (u32)c;
        memcpy(data + 16 * c, it->second.data(), it->second.size());
        c += (it->second.size() + 15) / 16;
        bytes_ -= it->second.size();
        it = bt.w.erase(it);
        ++r;
      }
      for (u64 k2 = 0; k2 < ndr; ++k2) dirty[di++] = bt.dirty[k2];
      bt.dirty.erase(bt.dirty.begin(), bt.dirty.begin() + ndr);
    };
    put(b0, n0, nd0);
    size_t gone = 0;   // leading batches fully taken (unpauses included)
    for (size_t k = 0; k <= nwhole; ++k) {
      Batch& bt = dl_[k];
      if (k) put(bt, bt.w.size(), bt.dirty.size());
      if (!bt.w.empty() || !bt.dirty.empty()) break;   // (the first batch went in part)
      take_unp(bt.unp);   // the whole batch went: its unpauses ride along
      if (!bt.unp.empty()) break;
      ++gone;
    }
    for (size_t k = 0; k < gone; ++k) dl_.pop_front();
    return done((u32)((data - out) + 16 * c));
  }

 private:
  // staged writes (device address -> bytes, non-overlapping) and channels to mark, with the
  // unpauses staged after them; a batch that overflows one step's delta buffer keeps its
  // unpauses until its last write is packed.  open: a light control section is still staging
  // into it (stage_begin .. stage_end); a step never takes an open batch, so one section's
  // change set rides one step whole
  struct Batch { std::map<u64, std::string> w; std::vector<u32> dirty, unp; bool open = false; u64 id = 0; };
  void new_batch() {   // (mu held)
    dl_.emplace_back();
    dl_.back().open = open_ > 0;
    dl_.back().id = next_id_++;
  }
  // the batch staging goes into (mu held).  Never a closed batch with nothing in it: dl_state(1)
  // counts that one as taken already, and it must not go back on that for what is staged now
  Batch& staging() {
    if (!dl_.empty()) {
      const Batch& b = dl_.back();
      if (!b.open && b.w.empty() && b.dirty.empty() && b.unp.empty()) dl_.pop_back();
    }
    if (dl_.empty()) new_batch();
    return dl_.back();
  }
  static void add_once(std::vector<u32>& v, u32 x) {
    if (std::find(v.begin(), v.end(), x) == v.end()) v.push_back(x);
  }
  std::deque<Batch> dl_;          // oldest first
  std::vector<u32> unp_ready_;    // unpauses of batches flush_deltas applied (next step)
  u32 open_ = 0;                  // light sections staging now (stage_begin / stage_end)
  u64 next_id_ = 1;               // id of the next batch (Batch.id)
  u64 bytes_ = 0;                 // data bytes staged (deltas_pending)
};
