// Data plane: helpers shared by every stage (wave / block primitives, copies, hashes,
// message release) and the topic-word splitter.
#pragma once
#include "dp_state.h"

#define INVALID 0xffffffffu
#define FNV64_BASIS 0xcbf29ce484222325ULL
#define FNV64_PRIME 0x100000001b3ULL

// ============================================================================ helpers
DEV u32 lane_id() { return __lane_id(); }
DEV u64 lanemask_lt() {
  u32 l = __lane_id();
  return l ? ((~0ull) >> (64 - l)) : 0ull;
}
DEV u32 be16(const u8* p) { return (u32(p[0]) << 8) | u32(p[1]); }
DEV u32 be32(const u8* p) {
  return (u32(p[0]) << 24) | (u32(p[1]) << 16) | (u32(p[2]) << 8) | u32(p[3]);
}
DEV u64 be64(const u8* p) { return (u64(be32(p)) << 32) | u64(be32(p + 4)); }
DEV void wr16(u8* p, u32 v) { p[0] = u8(v >> 8); p[1] = u8(v); }
DEV void wr32(u8* p, u32 v) { p[0] = u8(v >> 24); p[1] = u8(v >> 16); p[2] = u8(v >> 8); p[3] = u8(v); }
DEV void wr64(u8* p, u64 v) { wr32(p, u32(v >> 32)); wr32(p + 4, u32(v)); }
DEV u32 align16(u32 x) { return (x + 15u) & ~15u; }

DEV u64 exch_hash(u32 vhost, const u8* name, u32 n) {
  u64 h = FNV64_BASIS ^ (u64(vhost) * 0x9E3779B97F4A7C15ULL);
  for (u32 i = 0; i < n; ++i) { h ^= name[i]; h *= FNV64_PRIME; }
  return h;
}
DEV u32 fnv1a32(const u8* p, u32 n) {
  u32 h = 0x811c9dc5u;
  for (u32 i = 0; i < n; ++i) { h ^= p[i]; h *= 0x01000193u; }
  return h;
}

struct __attribute__((packed, aligned(1))) U4 { u32 x, y, z, w; };

// unaligned-source, unaligned-dest byte copy by the 64 lanes of one wave (kept minimal:
// it is inlined into the store / render / pack kernels, and a batched variant with 8
// loads in flight raised their VGPR count and cost them ~20% at 1 KB messages, measured)
DEV void wave_copy(u8* dst, const u8* src, u32 n) {
  u32 lane = lane_id();
  u32 nv = n >> 4;
  for (u32 i = lane; i < nv; i += 64) {
    U4 v = *(const U4*)(src + (u64)i * 16);
    *(U4*)(dst + (u64)i * 16) = v;
  }
  for (u32 i = (nv << 4) + lane; i < n; i += 64) dst[i] = src[i];
}

// same, by the G lanes (lane = 0..G-1) of a lane group
template <u32 G>
DEV void group_copy(u8* dst, const u8* src, u32 n, u32 lane) {
  u32 nv = n >> 4;
  for (u32 i = lane; i < nv; i += G) {
    U4 v = *(const U4*)(src + (u64)i * 16);
    *(U4*)(dst + (u64)i * 16) = v;
  }
  for (u32 i = (nv << 4) + lane; i < n; i += G) dst[i] = src[i];
}

// same, by all threads of a block
DEV void block_copy(u8* dst, const u8* src, u32 n, u32 tid, u32 nt) {
  u32 nv = n >> 4;
  for (u32 i = tid; i < nv; i += nt) {
    U4 v = *(const U4*)(src + (u64)i * 16);
    *(U4*)(dst + (u64)i * 16) = v;
  }
  for (u32 i = (nv << 4) + tid; i < n; i += nt) dst[i] = src[i];
}

// Saturating reservation for counters that restart at 0 every step (control bytes,
// delivery slots, egress budget): one atomicAdd and no give-back.  The caller owns
// [cur, cur + want) and is granted its part below cap, so granted ranges never overlap
// and the total granted is exactly min(sum of requests, cap) whatever the arrival order.
// The counter itself may end above cap: every reader clamps.  (A CAS loop serialises
// ~1000 queue blocks on one L2 line — 2.9 ms per step at 1024 fan-out queues — and an
// add-then-give-back fast path lets a transient overshoot inflate other threads' bases.)
DEV u32 reserve_sat(u32* p, u32 want, u32 cap, u32* base) {
  u32 cur = want ? atomicAdd(p, want) : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  *base = cur;
  if (cur >= cap) return 0;
  return want < cap - cur ? want : cap - cur;
}
DEV u64 reserve_sat64(u64* p, u64 want, u64 cap) {
  u64 cur = atomicAdd((unsigned long long*)p, (unsigned long long)want);
  if (cur >= cap) return 0;
  return want < cap - cur ? want : cap - cur;
}

// exact CAS reservation for counters that persist across steps and are also decremented
// (per-channel delivery windows): grant min(want, cap - *p).  Contention is per channel.
DEV u32 reserve_upto(u32* p, u32 want, u32 cap, u32* base) {
  u32 cur = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (true) {
    u32 avail = cur < cap ? cap - cur : 0;
    u32 g = want < avail ? want : avail;
    if (g == 0) { *base = cur; return 0; }
    u32 prev = atomicCAS(p, cur, cur + g);
    if (prev == cur) { *base = cur; return g; }
    cur = prev;
  }
}

// exclusive block scan (NT threads), returns this thread's offset; total via ref
template <int NT>
DEV u32 block_scan(u32 v, u32* lds, u32& total) {
  u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u32 x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    u32 y = __shfl_up(x, o, 64);
    if (lane >= (u32)o) x += y;
  }
  if (lane == 63) lds[w] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 run = 0;
    for (int i = 0; i < NT / 64; ++i) { u32 t = lds[i]; lds[i] = run; run += t; }
    lds[NT / 64] = run;
  }
  __syncthreads();
  u32 res = lds[w] + x - v;
  total = lds[NT / 64];
  __syncthreads();
  return res;
}

DEV u64 shfl_xor64(u64 v, int m) {
  return ((u64)(u32)__shfl_xor((int)(v >> 32), m, 64) << 32) | (u32)__shfl_xor((int)(u32)v, m, 64);
}
DEV u64 shfl64(u64 v, u32 src) {
  u32 lo = __shfl((u32)v, src, 64), hi = __shfl((u32)(v >> 32), src, 64);
  return (u64(hi) << 32) | lo;
}
DEV i64 wave_sum64(i64 v) {
  u64 x = (u64)v;
  for (int o = 32; o > 0; o >>= 1) {
    u32 lo = __shfl_xor((u32)x, o, 64), hi = __shfl_xor((u32)(x >> 32), o, 64);
    x += (u64(hi) << 32) | lo;
  }
  return (i64)x;
}
// inclusive prefix sum over the wave's lanes (all 64 lanes call it)
DEV u64 wave_incl_scan64(u64 v) {
  const u32 lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 lo = __shfl_up((u32)v, o, 64), hi = __shfl_up((u32)(v >> 32), o, 64);
    if (lane >= (u32)o) v += (u64(hi) << 32) | lo;
  }
  return v;
}
// all 64 lanes must call these (wave-uniform control flow); one atomic per distinct index
DEV void wave_add_u32(u32* arr, u32 idx, u32 v, bool valid) {
  u64 pend = __ballot(valid);
  while (pend) {
    u32 leader = __ffsll((unsigned long long)pend) - 1;
    u32 b = __shfl(idx, leader, 64);
    bool mine = valid && idx == b && ((pend >> lane_id()) & 1);
    u32 x = mine ? v : 0;
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if (lane_id() == leader) atomicAdd(&arr[b], x);
    pend &= ~__ballot(mine);
  }
}
DEV void wave_sub_u32(u32* arr, u32 idx, u32 v, bool valid) {
  u64 pend = __ballot(valid);
  while (pend) {
    u32 leader = __ffsll((unsigned long long)pend) - 1;
    u32 b = __shfl(idx, leader, 64);
    bool mine = valid && idx == b && ((pend >> lane_id()) & 1);
    u32 x = mine ? v : 0;
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if (lane_id() == leader) atomicSub(&arr[b], x);
    pend &= ~__ballot(mine);
  }
}
DEV void wave_add_i64(i64* arr, u64 idx, i64 v, bool valid) {
  u64 pend = __ballot(valid);
  while (pend) {
    u32 leader = __ffsll((unsigned long long)pend) - 1;
    u64 b = shfl64(idx, leader);
    bool mine = valid && idx == b && ((pend >> lane_id()) & 1);
    i64 x = wave_sum64(mine ? v : 0);
    if (lane_id() == leader) atomicAdd((unsigned long long*)&arr[b], (unsigned long long)x);
    pend &= ~__ballot(mine);
  }
}
// wave-uniform reservation of `cnt` (per lane) slots from one counter: returns lane's base
DEV u32 wave_reserve(u32* ctr, bool want, u32* total_out = nullptr) {
  u64 m = __ballot(want);
  u32 n = __popcll(m);
  u32 base = 0;
  if (n) {
    u32 leader = __ffsll((unsigned long long)m) - 1;
    if (lane_id() == leader) base = atomicAdd(ctr, n);
    base = __shfl(base, leader, 64);
  }
  if (total_out) *total_out = n;
  return base + __popcll(m & lanemask_lt());
}

// a message's slot: the HBM body log, or the host spill ring for a spilled cold body
DEV const u8* msg_slot(const DS& d, u64 log_off) {
  return (log_off & SPILL_BIT) ? d.spill + ((log_off & ~SPILL_BIT) % d.spill_bytes) : d.log + (log_off % d.log_bytes);
}

// live-bytes accounting of a freed slot in the spill ring
DEV void spill_free(const DS& d, u64 log_off, u32 slot_bytes) {
  const u64 blk = ((log_off & ~SPILL_BIT) / d.log_block) % d.n_spill_blocks;
  atomicAdd((unsigned long long*)&d.spill_live[blk], (unsigned long long)(-(i64)slot_bytes));
}

// ---- message release (K11): refcount -1, free slot + table index at zero
DEV void release_msg(const DS& d, u32 msg) {
  if (msg == INVALID) return;
  i32 old = atomicSub(&d.msgs[msg].refcnt, 1);
  if (old == 1) {
    MsgEnt& m = d.msgs[msg];
    if (m.log_off & COLD_BIT) {
      atomicAdd((unsigned long long*)&d.cold_live[((m.log_off & ~COLD_BIT) >> COLD_SEG_SHIFT) % COLD_SEGS],
                (unsigned long long)(-(i64)m.slot_bytes));
    } else if (m.log_off & SPILL_BIT) {
      spill_free(d, m.log_off, m.slot_bytes);
    } else {
      u64 blk = (m.log_off / d.log_block) % d.n_log_blocks;
      atomicAdd((unsigned long long*)&d.log_live[blk], (unsigned long long)(-(i64)m.slot_bytes));
      atomicAdd((unsigned long long*)d.live_bytes, (unsigned long long)(-(i64)m.slot_bytes));
    }
    u32 slot = atomicAdd(d.msg_free_top, 1u);
    d.msg_free[slot] = msg;
    atomicAdd(&d.ctr->n_freed, 1u);
  }
}

// wave-uniform release: refcount atomics per lane, one free-list reservation and one
// live-bytes atomic per distinct log block per wave (avoids serialising on hot words)
DEV void wave_release(const DS& d, u32 msg, bool valid) {
  bool freed = false, spilled = false;
  u64 blk = 0;
  i64 sb = 0;
  if (valid && msg != INVALID) {
    i32 old = atomicSub(&d.msgs[msg].refcnt, 1);
    if (old == 1) {
      freed = true;
      const u64 lo = d.msgs[msg].log_off;
      sb = d.msgs[msg].slot_bytes;
      spilled = (lo & (SPILL_BIT | COLD_BIT)) != 0;
      if (lo & COLD_BIT)   // (rare: bodies in the cold store)
        atomicAdd((unsigned long long*)&d.cold_live[((lo & ~COLD_BIT) >> COLD_SEG_SHIFT) % COLD_SEGS],
                  (unsigned long long)(-sb));
      else if (spilled) spill_free(d, lo, (u32)sb);   // (rare: cold bodies)
      else blk = (lo / d.log_block) % d.n_log_blocks;
    }
  }
  u64 fm = __ballot(freed);
  if (!fm) return;
  u32 nf;
  u32 pos = wave_reserve(d.msg_free_top, freed, &nf);
  if (freed) d.msg_free[pos] = msg;
  i64 tot = wave_sum64(freed && !spilled ? sb : 0);
  if (lane_id() == __ffsll((unsigned long long)fm) - 1) {
    atomicAdd(&d.ctr->n_freed, nf);
    if (tot) atomicAdd((unsigned long long*)d.live_bytes, (unsigned long long)(-tot));
  }
  wave_add_i64(d.log_live, blk, -sb, freed && !spilled);
}

// ---- K13 snowflake ids: id = ms << 22 | worker << 12 | seq (IdGenerator.scala:14-34).
// The reference's generator allows 4096 ids per ms per node and waits for the next ms
// (IdGenerator.scala:55-83); one MI355X publishes ~10x that.  A GPU therefore owns
// ID_WORKERS worker ids (group g = StepIn.worker owns g*64 .. g*64+63): 2^18 ids per ms
// (262 M msgs/s), so the virtual position (ms << 18 | slot) never outruns the wall clock
// and ids stay unique across restarts (the host seeds id_next above recovered ids).
DEV u64 snowflake_id(u64 pos, u32 group) {
  const u64 ms = pos >> ID_SLOT_BITS;
  const u64 worker = (u64)(group & (1023 / ID_WORKERS)) * ID_WORKERS + ((pos >> 12) & (ID_WORKERS - 1));
  return (ms << 22) | (worker << 12) | (pos & 4095);
}

// ============================================================================ topic words
// Java String.split("\\.") semantics (QueueMatcher.scala:69-71): trailing empty
// words dropped, "" -> [""], "..." -> [].
struct Words { u32 eff; u32 count; };
DEV Words words_of(const u8* s, u32 n) {
  Words w;
  if (n == 0) { w.eff = 0; w.count = 1; return w; }
  u32 e = n;
  while (e > 0 && s[e - 1] == '.') --e;
  w.eff = e;
  if (e == 0) { w.count = 0; return w; }
  u32 c = 1;
  for (u32 i = 0; i < e; ++i) c += (s[i] == '.');
  w.count = c;
  return w;
}
DEV u32 word_len(const u8* s, u32 off, u32 eff) {
  u32 i = off;
  while (i < eff && s[i] != '.') ++i;
  return i - off;
}
DEV bool word_eq(const u8* a, u32 al, const u8* b, u32 bl) {
  if (al != bl) return false;
  for (u32 i = 0; i < al; ++i)
    if (a[i] != b[i]) return false;
  return true;
}
// exact topic match: '*' = one word, '#' = zero or more words (when hash_wild),
// greedy backtracking (glob algorithm over words). Golden: models/matcher.py words_match.
DEV bool topic_match(const u8* pat, u32 plen, const u8* key, u32 klen, bool hash_wild) {
  Words pw = words_of(pat, plen), kw = words_of(key, klen);
  u32 pend = pw.eff + 1, kend = kw.eff + 1;  // cursor == end -> exhausted
  u32 p = pw.count ? 0 : pend, k = kw.count ? 0 : kend;
  u32 sp = INVALID, sk = 0;
  while (k < kend) {
    u32 kl = word_len(key, k, kw.eff);
    if (p < pend) {
      u32 pl = word_len(pat, p, pw.eff);
      bool is_hash = hash_wild && pl == 1 && pat[p] == '#';
      bool is_star = pl == 1 && pat[p] == '*';
      if (is_hash) { p += pl + 1; sp = p; sk = k; continue; }
      if (is_star || word_eq(pat + p, pl, key + k, kl)) { p += pl + 1; k += kl + 1; continue; }
    }
    if (sp != INVALID) {
      sk += word_len(key, sk, kw.eff) + 1;
      k = sk;
      p = sp;
      continue;
    }
    return false;
  }
  while (p < pend) {
    u32 pl = word_len(pat, p, pw.eff);
    if (hash_wild && pl == 1 && pat[p] == '#') { p += pl + 1; continue; }
    return false;
  }
  return true;
}
