// MI355X (gfx950) AMQP 0-9-1 data plane: the broker hot path as a fixed-shape,
// hipGraph-capturable kernel pipeline.
//
//   K0 stage        carry + new TCP bytes -> contiguous per-connection work segment
//   K1 frame_scan   speculative frame-boundary scan + chain resolution (LDS), command
//                   assembly (method -> header -> bodies), control barrier, carry-out
//                   (FrameParser.scala:86-157, CommandAssembler.scala:56-130)
//   K3/K4 decode    Basic.Publish / Ack / Nack / Reject args + content-header
//                   properties (Basic.scala:36-59, BasicProperties.scala:42-96)
//   K6 route        direct (device hash), fanout (CSR), topic (int8 MFMA word-hash
//                   prefilter + exact word matcher)  (QueueMatcher.scala, ExchangeEntity.scala:287-331)
//   K13 ids         snowflake ids (IdGenerator.scala:55-83)
//   K7 enqueue      stable radix sort by queue -> per-queue HBM ring append (QueueEntity.scala:271-316)
//   K9 acks         per-channel unacked windows, ack/nack/reject (AMQChannel.scala:109-174)
//   K8/K12 dequeue  credit-limited round-robin pull with TTL skip (QueueEntity.scala:318-393)
//   K9 tags         stable sort by channel -> delivery tags
//   K5 render       Deliver / Return / confirm-Ack frames written straight into
//                   host-mapped egress memory (AMQCommand.scala:30-59)
//   K10 confirms    one coalesced Basic.Ack per channel per step (FrameStage.scala:571-596)
//   K11 refcount    body refcount + free-list / log reclamation (MessageEntity.scala:134-166)
//
// Every kernel reads its dynamic sizes from device counters, so grids are fixed by
// EngineCfg and the whole step is captured once into a hipGraph (engine.hip).
//
// The stages are being moved into headers dp_*.h of their own, included in pipeline order;
// each includes the earlier headers whose functions it calls.  Moved so far: the shared
// helpers and the frame scan; the other stages are still in this file.
#include "dp_state.h"
#include "dp_util.h"

// ============================================================================ deferred control writes
// The control plane's table writes (connection / channel / consumer state) staged while
// steps run, packed per step by the host (DeltaStage::pack_deltas): applied by k_stage before
// the step reads anything, so no pipeline drain is needed for them.  Layout (step_abi.h):
//   DeltaHead | DeltaRec[nrec] | u32 dirty channel slots[ndirty] (16-B padded) | data chunks
// Records never overlap (the host keeps the last write of every byte), so they are applied
// in parallel: 16-byte chunk i belongs to record r with chunk0[r] <= i < chunk0[r + 1].
DEV void apply_deltas(const DS& d, const u8* buf, u32 tid, u32 nt, DeltaRec* lrec) {
  const DeltaHead h = *(const DeltaHead*)buf;
  const DeltaRec* recs = (const DeltaRec*)(buf + sizeof(DeltaHead));
  const u32* dirty = (const u32*)(recs + h.nrec);
  const uint4* data = (const uint4*)((const u8*)dirty + ((4u * h.ndirty + 15u) & ~15u));
  for (u32 r = tid; r < h.nrec; r += nt) lrec[r] = recs[r];
  __syncthreads();
  for (u32 i = tid; i < h.nchunk; i += nt) {
    u32 lo = 0, hi = h.nrec;   // last record with chunk0 <= i
    while (hi - lo > 1) {
      const u32 mid = (lo + hi) >> 1;
      if (lrec[mid].chunk0 <= i) lo = mid; else hi = mid;
    }
    const DeltaRec r = lrec[lo];
    const u32 off = (i - r.chunk0) * 16u;
    const u32 n = r.len - off < 16u ? r.len - off : 16u;
    const uint4 v = data[i];
    u8* dst = (u8*)(uintptr_t)(r.dst + off);
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    if (((uintptr_t)dst & 3) == 0 && (n & 3) == 0) {
      for (u32 k = 0; k < n / 4; ++k) ((u32*)dst)[k] = w[k];
    } else {
      for (u32 k = 0; k < n; ++k) dst[k] = (u8)(w[k >> 2] >> (8 * (k & 3)));
    }
  }
  __syncthreads();
  // closing channels: on the dirty list (k_chan_advance requeues their unacked deliveries)
  for (u32 k = tid; k < h.ndirty; k += nt) {
    const u32 ch = dirty[k];
    if (atomicExch(&d.ch_dirty[ch], 1u) == 0) d.dirty_list[atomicAdd(d.n_dirty, 1u)] = ch;
  }
  __threadfence();   // (rare: steps with control writes) every later read of the block sees them
  __syncthreads();
}
// between steps (the control plane holds the engine): the staged writes now
__global__ __launch_bounds__(1024) void k_apply_deltas(DS d, const u8* buf) {
  __shared__ DeltaRec lrec[DELTA_REC_MAX];
  apply_deltas(d, buf, threadIdx.x, 1024, lrec);
}

// ============================================================================ K0 step init
// one block: resets the step counters and lays the step's segments out in the work buffer
// (segment k at the prefix of the 16-aligned sizes carry + new bytes + 32 of the segments
// before it).  The copy itself is done by k_frame_scan's block for the segment, which
// stages the bytes through its LDS anyway (was: a grid-wide copy kernel, 12 us per 16.7 MB
// step, whose output the frame scan then read back)
__global__ __launch_bounds__(1024) void k_stage(DS d) {
  __shared__ u32 lds[1024 / 64 + 1];
  __shared__ StepIn s_in;
  __shared__ DeltaRec lrec[DELTA_REC_MAX];
  const u32 tid = threadIdx.x;
  // the step's descriptors from the host's mapped staging (one PCIe round), written to
  // their device copies for every later kernel of the step
  if (tid == 0) {
    s_in = *d.in_h;
    *d.in = s_in;
  }
  __syncthreads();
  if (s_in.delta_bytes) apply_deltas(d, d.delta_h, tid, 1024, lrec);   // control writes first
  const u32 nseg = s_in.nseg;
  {
    u32* c = (u32*)d.ctr;
    for (u32 k = tid; k < sizeof(Counters) / 4; k += 1024)
      if (k * 4 < offsetof(Counters, log_head)) c[k] = 0;
    if (tid == 0) {   // (per-parity scratch only: the link-ack counts and the id floor are
                      // reset by marks_range, in the step's routing half)
      d.ctr->n_grow = 0; d.tot[TS_NMOVE] = 0; d.tot[TS_NDEFER] = 0; d.tot[TS_TTL_BUDGET] = 0;
      d.tot[TS_NDGET] = 0;
      d.tot[TS_SPILL_USED] = 0;
      d.tot[TS_HOP_N] = 0;
      d.ctr->spill_moved = 0;
      d.ctr->n_ref = 0; d.ctr->gath_off = 0; d.ctr->ref_bytes = 0;
      d.ctr->n_maxlen_dropped = 0; d.ctr->n_maxlen_rejected = 0;
      *d.egress_budget = 0;
    }
    // connections whose control command the host has answered resume with this step (the
    // frame scan, the only reader and writer of the flag, runs after this kernel)
    const u32 nunp = s_in.nunp;
    for (u32 k = tid; k < nunp; k += 1024) {
      const u32 c = d.unpause_req[k];
      if (c < d.c_max) d.conn_paused[c] = 0;
    }
  }
  u32 total = 0;
  u32 cl0 = 0, len0 = 0;   // this thread's first segment (the usual step has <= 1024): the
                           // layout pass below reuses it instead of a second PCIe read
  for (u32 k = tid; k < nseg; k += 1024) {
    const SegIn sg = d.segs_h[k];
    ((SegIn*)d.segs)[k] = sg;
    const u32 cl = d.carry_len[sg.conn];
    if (k == tid) { cl0 = cl; len0 = sg.len; }
    total += align16(cl + sg.len + 32);
  }
  u32 all_t;
  block_scan<1024>(total, lds, all_t);
  if (tid == 0) d.tot[TS_WORK_USED] = all_t;
  if (all_t > d.work_cap) return;   // host sizes steps so this never triggers
  u32 run = 0;
  for (u32 b0 = 0; b0 < nseg; b0 += 1024) {
    const u32 k = b0 + tid;
    u32 cl = 0, len = 0, v = 0;
    if (k < nseg) {
      if (b0 == 0) {
        cl = cl0;
        len = len0;
      } else {
        const SegIn sg = d.segs_h[k];
        cl = d.carry_len[sg.conn];
        len = sg.len;
      }
      v = align16(cl + len + 32);
    }
    u32 all;
    __syncthreads();   // lds of the previous scan
    const u32 o = block_scan<1024>(v, lds, all);
    if (k < nseg) { d.seg_total[k] = cl + len; d.seg_start[k] = run + o; }
    run += all;
  }
}

#include "dp_frame_scan.h"
#include "dp_headers.h"
#include "dp_xdeath.h"

// ============================================================================ K3 classify / decode
DEV void set_counts(const DS& d, u32 np, u32 na) {
  d.ctr->n_pubs = np < d.pub_max ? np : d.pub_max;
  d.ctr->n_acks = na < d.ack_max ? na : d.ack_max;
  // routing phase 0: the step's own publishes
  d.tot[TS_RANGE_LO] = 0;
  d.tot[TS_RANGE_HI] = d.ctr->n_pubs;
  d.tot[TS_PAIR_BASE] = 0;
  d.tot[TS_PAIR_N] = 0;
  d.tot[TS_NIMPORT] = 0;
}

DEV bool skip_shortstr(const u8* p, u32& o, u32 end) {
  if (o + 1 > end) return false;
  o += 1 + p[o];
  return o <= end;
}

// topic key vector (8 words x 32 bits, +-1), built only if topic bindings exist
DEV u32 build_keyvec(const DS& d, const u8* key, u32 len, u32 pi) {
  Words kw = words_of(key, len);
  if (d.tb_max) {
    // 32 int8 lanes per word (+1 / -1 per hash bit), written as two 16-B stores
    uint4* kv = (uint4*)(d.pub_keyvec + (u64)pi * TOPIC_K);
    u16* kwo = d.pub_kwoff + (u64)pi * TOPIC_WORDS;   // (offset << 8 | length) per word
    u32 off = 0;
    u32 wi = 0;
    if (kw.count) {
      while (wi < TOPIC_WORDS && off <= kw.eff) {
        u32 wl = word_len(key, off, kw.eff);
        u32 h = fnv1a32(key + off, wl);
        kwo[wi] = (u16)((off << 8) | (wl & 255));
        u32 pk[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) {
          u32 v = 0;
#pragma unroll
          for (int bb = 0; bb < 4; ++bb) v |= (((h >> (g * 4 + bb)) & 1) ? 0x01u : 0xffu) << (8 * bb);
          pk[g] = v;
        }
        kv[wi * 2] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        kv[wi * 2 + 1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
        off += wl + 1;
        ++wi;
      }
    }
    for (; wi < TOPIC_WORDS; ++wi) {
      kv[wi * 2] = make_uint4(0, 0, 0, 0);
      kv[wi * 2 + 1] = make_uint4(0, 0, 0, 0);
    }
  }
  return kw.count;
}

// ---- 32-byte register windows of a publish's method arguments and routing key.  The
// byte loops above cost one memory round trip per byte wherever a loop's exit depends on
// the byte (word_len, the trailing-'.' strip), ~20 dependent trips per publish at one
// thread per command; here two 16-byte loads bring the bytes in and every loop below is
// unrolled over compile-time positions (register selects, no scratch).  Callers guarantee
// 32 readable bytes at the window start (the work buffer has 4 KB of slack past work_cap).
// named words, not an array: no dynamic index can pin the window to scratch memory
struct Win32 { u32 w0, w1, w2, w3, w4, w5, w6, w7; };
DEV Win32 load_win(const u8* p) {
  const U4 a = *(const U4*)p, b = *(const U4*)(p + 16);
  return Win32{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}
// word k < 8: folds to one register for a compile-time k, a select chain otherwise
DEV u32 win_word(const Win32& s, u32 k) {
  // selects over values (a ?: over the members themselves selects their addresses)
  const u32 a0 = s.w0, a1 = s.w1, a2 = s.w2, a3 = s.w3, a4 = s.w4, a5 = s.w5, a6 = s.w6, a7 = s.w7;
  const u32 lo = k < 2 ? (k == 0 ? a0 : a1) : (k == 2 ? a2 : a3);
  const u32 hi = k < 6 ? (k == 4 ? a4 : a5) : (k == 6 ? a6 : a7);
  return k < 4 ? lo : hi;
}
// byte i < 32 of the window
DEV u32 win_byte(const Win32& s, u32 i) { return (win_word(s, i >> 2) >> (8 * (i & 3))) & 255u; }
DEV u32 win_get(const Win32& s, u32 i) { return win_byte(s, i); }
// FNV-1a 64 of bytes [S, S + n) of the window (S + n <= 32)
template <u32 S>
DEV u64 win_fnv64(const Win32& s, u32 n, u64 h) {
#pragma unroll
  for (u32 i = 0; i + S < 32; ++i) {
    if (i < n) {   // predicated, not a break: the loop stays fully unrolled (constant indices)
      h ^= win_byte(s, i + S);
      h *= FNV64_PRIME;
    }
  }
  return h;
}

// build_keyvec for a routing key of n <= 32 bytes held in a window: same rows, same count
DEV u32 build_keyvec_win(const DS& d, const Win32& s, u32 n, u32 pi) {
  const u32 lenmask = n >= 32 ? ~0u : ((1u << n) - 1u);
  u32 dots = 0;
#pragma unroll
  for (u32 i = 0; i < 32; ++i) dots |= (win_byte(s, i) == '.' ? 1u : 0u) << i;
  dots &= lenmask;
  const u32 nd = ~dots & lenmask;                 // trailing '.' stripped (words_of)
  const u32 eff = nd ? 32u - __clz(nd) : 0u;
  const u32 effmask = eff >= 32 ? ~0u : ((1u << eff) - 1u);
  const u32 de = dots & effmask;
  const u32 count = n == 0 ? 1u : (eff == 0 ? 0u : 1u + __popc(de));
  if (!d.tb_max) return count;
  // per-word FNV-1a 32 in one pass: a '.' commits the running hash to its word slot
  u32 hw[TOPIC_WORDS];
#pragma unroll
  for (u32 k = 0; k < TOPIC_WORDS; ++k) hw[k] = 0x811c9dc5u;
  u32 h = 0x811c9dc5u, wi = 0;
#pragma unroll
  for (u32 i = 0; i < 32; ++i) {
    const u32 c = win_byte(s, i);
    const bool in = i < eff, dot = in && c == '.';
#pragma unroll
    for (u32 k = 0; k < TOPIC_WORDS; ++k) hw[k] = (dot && wi == k) ? h : hw[k];
    wi += dot ? 1u : 0u;
    h = dot ? 0x811c9dc5u : (in ? (h ^ c) * 0x01000193u : h);
  }
#pragma unroll
  for (u32 k = 0; k < TOPIC_WORDS; ++k) hw[k] = wi == k ? h : hw[k];
  const u32 nw = count < TOPIC_WORDS ? count : TOPIC_WORDS;
  uint4* kv = (uint4*)(d.pub_keyvec + (u64)pi * TOPIC_K);
  u16* kwo = d.pub_kwoff + (u64)pi * TOPIC_WORDS;
  u32 off = 0;
#pragma unroll
  for (u32 k = 0; k < TOPIC_WORDS; ++k) {
    if (k < nw) {
      const u32 rest = off >= 32 ? 0u : (de & ~((1u << off) - 1u));   // separators at or after off
      u32 e = rest ? (u32)(__ffs(rest) - 1) : eff;
      if (e > eff) e = eff;
      const u32 wl = e - off;
      kwo[k] = (u16)((off << 8) | (wl & 255));
      u32 pk[8];
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        u32 v = 0;
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) v |= (((hw[k] >> (g * 4 + bb)) & 1) ? 0x01u : 0xffu) << (8 * bb);
        pk[g] = v;
      }
      kv[k * 2] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
      kv[k * 2 + 1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
      off = e + 1;
    } else {
      kv[k * 2] = make_uint4(0, 0, 0, 0);
      kv[k * 2 + 1] = make_uint4(0, 0, 0, 0);
    }
  }
  return count;
}

// K9 ack mark (AMQChannel.scala:128-174): single tag -> its window slot; multiple -> the
// record (tag resolved) stays in d.acks and the channel's [first, last] ack index range
// grows, so k_chan_advance resolves the step's multiple settles in wire order (ack index
// = command order): a tag's fate is the first settle covering it, e.g. Nack(4, requeue)
// then Ack(8) requeues 1-4.  Marks only depend on earlier steps' deliveries.
template <bool DLX>   // DS.dlx as a compile-time constant: the flag-off kernel holds none of the dead-letter code
DEV void apply_ack(const DS& d, Ack a, u32 ai) {
  const u32 ch = a.chslot;
  if (ch == INVALID) { d.acks[ai] = a; return; }
  const u64 nt = d.ch_next_tag[ch];
  u64 tag = a.tag;
  if (tag == 0 && a.multiple) tag = nt - 1;  // ack everything outstanding
  a.tag = tag;
  d.acks[ai] = a;
  const bool requeue = (a.kind != CK_ACK) && a.requeue;
  // DS.dlx: a Reject / Nack without requeue is its own mark (dead-lettered where the queue has
  // a dead-letter exchange, else an ack: chan_advance_one); off, it is an ack as always
  const bool dead = DLX && (a.kind != CK_ACK) && !a.requeue;
  if (a.multiple) {
    atomicMin(&d.ch_mlo[ch], ai);
    atomicMax(&d.ch_mhi[ch], ai);
  } else if (tag >= d.ch_uhead[ch] && tag < nt) {
    USlot& u = d.uwin[(u64)ch * (d.ucap_mask + 1) + ((tag - 1) & d.ucap_mask)];
    atomicCAS(&u.state, (u32)US_PENDING, requeue ? (u32)US_REQUEUE : (dead ? (u32)US_DEAD : (u32)US_ACKED));
  }
  if (atomicExch(&d.ch_dirty[ch], 1u) == 0) {
    u32 k = atomicAdd(d.n_dirty, 1u);
    d.dirty_list[k] = ch;
  }
  atomicAdd(&d.ctr->n_acked, 1u);
}

// publishes are numbered in segment order (segment s's publishes follow those of the
// segments before it), not in the order the frame-scan blocks reserved their commands:
// queue order across connections is then deterministic (the golden model's order)
__global__ __launch_bounds__(256) void k_decode(DS d) {
  __shared__ u32 spref[DEC_SEG_LDS];
  __shared__ u32 sprefa[DEC_SEG_LDS];
  __shared__ u32 lds[256 / 64 + 1];
  const u32 nseg = d.in->nseg;
  const bool seg_order = nseg <= DEC_SEG_LDS;
  u32 n0 = d.ctr->n_cmds;
  n0 = n0 < d.cmd_max ? n0 : d.cmd_max;
  if (!d.rank_scan) {
    // segment-major numbering from the frame scan's per-segment ordinals: every busy block
    // (and block 0, which sets the step's counts) scans the segments' publish / ack counts
    if (blockIdx.x != 0 && blockIdx.x * 256 >= n0) return;   // whole block idle
    u32 run = 0, runa = 0;
    for (u32 b0 = 0; b0 < nseg; b0 += 256) {
      const u32 k = b0 + threadIdx.x;
      const u32 v = k < nseg ? d.seg_npub[k] : 0, va = k < nseg ? d.seg_nack[k] : 0;
      u32 all, alla;
      const u32 o = block_scan<256>(v, lds, all);
      const u32 oa = block_scan<256>(va, lds, alla);
      if (k < nseg) { spref[k] = run + o; sprefa[k] = runa + oa; }
      run += all;
      runa += alla;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) set_counts(d, run, runa);   // fused: counts + phase-0 range
    __syncthreads();
    if (blockIdx.x * 256 >= n0) return;
  } else {
    if (blockIdx.x == 0 && threadIdx.x == 0) set_counts(d, d.tot[TS_CMD_PUBS], d.tot[TS_CMD_ACKS]);
    if (blockIdx.x * 256 >= n0) return;   // whole block idle
    if (seg_order) {
      u32 run = 0;
      for (u32 b0 = 0; b0 < nseg; b0 += 256) {
        const u32 k = b0 + threadIdx.x;
        const u32 v = k < nseg ? d.seg_npub[k] : 0;
        u32 all;
        const u32 o = block_scan<256>(v, lds, all);
        if (k < nseg) spref[k] = run + o;
        run += all;
      }
      __syncthreads();
    }
  }
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  u32 n = d.ctr->n_cmds;
  if (n > d.cmd_max) n = d.cmd_max;
  if (i >= n) return;
  const Cmd c = d.cmds[i];
  const u8* w = d.work;
  if (c.kind == CK_PUBLISH) {
    u32 pi;
    if (!d.rank_scan) {
      pi = spref[c.seg] + c.pad[1];
    } else {
      pi = d.cmd_pub_rank[i];
      if (seg_order && c.seg < nseg && d.seg_cmd_base[c.seg] != INVALID)
        pi = spref[c.seg] + (pi - d.cmd_pub_rank[d.seg_cmd_base[c.seg]]);
    }
    if (pi >= d.pub_max) return;
    Pub pb;
    pb.conn = c.conn;
    pb.chslot = c.pad[0];
    pb.frag0 = c.frag0;
    pb.nfrag = c.nfrag;
    pb.body_size = c.body_size;
    pb.flags = 0;
    pb.expire_ms = 0;
    pb.ts_ms = 0;
    pb.nq = 0; pb.slot_bytes = 0; pb.msg = INVALID; pb.pad = 0; pb.xid = 0;
    // method args: class u16, method u16, ticket u16, exchange ss, rk ss, bits
    // (skip_shortstr inlined over register windows: [ex_len][exchange][rk_len] in one,
    // exchange names up to 30 bytes; the routing key and the bits octet in a second)
    u32 o = c.m_off + 6, end = c.m_off + c.m_len;
    const u32 o0 = o;
    const Win32 ma = load_win(w + o0);
    bool ok = o <= end;
    pb.ex_off = o + 1;
    const u32 b0 = ok && o < end ? win_byte(ma, 0) : 0u;
    pb.ex_len = b0;
    if (ok) { if (o + 1 > end) ok = false; else { o += 1 + b0; ok = o <= end; } }
    pb.rk_off = o + 1;
    const u32 b1 = ok && o < end ? (o - o0 < 32 ? win_get(ma, o - o0) : (u32)w[o]) : 0u;
    pb.rk_len = b1;
    if (ok) { if (o + 1 > end) ok = false; else { o += 1 + b1; ok = o <= end; } }
    const Win32 rkw = load_win(w + pb.rk_off);
    u32 bits = (ok && o < end) ? (o - pb.rk_off < 32 ? win_get(rkw, o - pb.rk_off) : (u32)w[o]) : 0u;
    if (bits & 1) pb.flags |= MF_MANDATORY;
    if (bits & 2) pb.flags |= MF_IMMEDIATE;
    // exchange
    i32 xs = -1;
    if (ok) {
      const u32 vh = d.conn_vhost[c.conn];
      u64 hk = pb.ex_len <= 31 ? win_fnv64<1>(ma, pb.ex_len, FNV64_BASIS ^ (u64(vh) * 0x9E3779B97F4A7C15ULL))
                               : exch_hash(vh, w + pb.ex_off, pb.ex_len);
      u32 mask = d.xhash_mask;
      for (u32 j = 0; j <= mask; ++j) {
        u32 slot = (u32)(hk + j) & mask;
        i32 v = d.x_hval[slot];
        if (v < 0) break;
        if (d.x_hkey[slot] == hk) { xs = v; break; }
      }
    }
    pb.exch = ok ? xs : -2;
    pb.keyhash = pb.rk_len <= 32 ? win_fnv64<0>(rkw, pb.rk_len, FNV64_BASIS) : fnv1a64_dev(w + pb.rk_off, pb.rk_len);
    // properties (flags chain then values), read through a 32-byte register window of the
    // header payload (one pair of loads instead of one dependent load per field)
    u32 ho = c.h_off + 12, hend = c.h_off + c.h_len;
    pb.props_off = ho;
    pb.props_len = hend > ho ? hend - ho : 0;
    const Win32 pw = load_win(w + ho);
    auto pbyte = [&](u32 q) -> u32 { const u32 o = q - ho; return o < 32 ? win_byte(pw, o) : (u32)w[q]; };
    u32 fl = 0;   // the first property-flags word (continuation words are skipped)
    u32 nfl = 0;
    u32 q = ho;
    bool fend = false;   // the flags chain ended on a word without the continuation bit
    while (q + 2 <= hend) {
      u32 fw = (pbyte(q) << 8) | pbyte(q + 1);
      q += 2;
      if (nfl == 0) fl = fw;
      ++nfl;
      if (!(fw & 1)) { fend = true; break; }
    }
    if (!fend) fl = 0;   // cut short inside the flags: no properties (as below)
    bool pok = true;
    // field order: 15 ctype ss, 14 cenc ss, 13 headers tbl, 12 dmode oct, 11 prio oct,
    // 10 corr ss, 9 replyto ss, 8 expiration ss, 7 msgid ss, 6 timestamp u64, 5 type,
    // 4 userid, 3 appid, 2 clusterid
    for (int bit = 15; bit >= 2 && pok; --bit) {
      if (!(fl & (1u << bit))) continue;
      switch (bit) {
        case 13: {
          if (q + 4 > hend) { pok = false; break; }
          u32 tl = (pbyte(q) << 24) | (pbyte(q + 1) << 16) | (pbyte(q + 2) << 8) | pbyte(q + 3);
          q += 4 + tl;
          pok = q <= hend;
          break;
        }
        case 12:
          if (q + 1 > hend) { pok = false; break; }
          if (pbyte(q) == 2) pb.flags |= MF_PERSIST;
          q += 1;
          break;
        case 11: q += 1; pok = q <= hend; break;
        case 8: {
          if (q + 1 > hend) { pok = false; break; }
          u32 sl = pbyte(q);
          if (q + 1 + sl > hend) { pok = false; break; }
          i64 v = 0;
          bool digits = sl > 0 && sl <= 18;
          for (u32 k = 0; k < sl && digits; ++k) {
            u32 ch = pbyte(q + 1 + k);
            if (ch < '0' || ch > '9') digits = false;
            else v = v * 10 + (ch - '0');
          }
          if (digits) pb.expire_ms = d.in->now_ms + v;
          q += 1 + sl;
          break;
        }
        case 6: {
          if (q + 8 > hend) { pok = false; break; }
          u64 ts = 0;
#pragma unroll
          for (u32 k = 0; k < 8; ++k) ts = (ts << 8) | pbyte(q + k);
          pb.ts_ms = (i64)ts * 1000;
          pb.flags |= MF_HAS_TS;
          q += 8;
          break;
        }
        default:
          if (q + 1 > hend) { pok = false; break; }
          q += 1 + pbyte(q);
          pok = q <= hend;
      }
    }
    // a list cut short inside a field has no properties at all (the golden model's reading:
    // the reference's decoder throws on one), whatever was read ahead of the cut
    if (!pok) { pb.flags &= ~(MF_PERSIST | MF_HAS_TS); pb.expire_ms = 0; pb.ts_ms = 0; }
    pb.nwords = pb.rk_len <= 32 ? build_keyvec_win(d, rkw, pb.rk_len, pi) : build_keyvec(d, w + pb.rk_off, pb.rk_len, pi);
    // egress by reference: a body that is one run of this step's new ingress bytes (not in
    // the connection's carry) keeps its host address -- its deliveries can be sent from
    // there instead of crossing PCIe back (render_deliv)
    if (c.nfrag == 1 && d.in->ingress_host && d.in->ref_back != 0xffffffffu && c.body_size >= d.in->ref_min &&
        c.seg < nseg) {
      const Frag fg = d.frags[c.frag0];
      const u32 w0 = d.seg_start[c.seg], cl = d.seg_total[c.seg] - d.segs[c.seg].len;
      const u64 ing_rel = (u64)d.in->ingress - (u64)d.work;
      if (fg.len == c.body_size && d.scan_inplace && (u64)d.in->ingress > (u64)d.work && fg.off >= ing_rel) {
        pb.flags |= MF_HREF;   // (read in place from the ingress slot: its payload offset)
        pb.pad = (u32)(fg.off - ing_rel);
      } else if (fg.len == c.body_size && fg.off >= w0 + cl && fg.off < w0 + d.seg_total[c.seg]) {
        pb.flags |= MF_HREF;
        pb.pad = (u32)(d.segs[c.seg].src + (fg.off - w0 - cl));
      }
    }
    d.pubs[pi] = pb;   // (its channel's confirm count: marks_range)
  } else if (c.kind == CK_ACK || c.kind == CK_NACK || c.kind == CK_REJECT) {
    const u32 ai = d.rank_scan ? d.cmd_ack_rank[i] : sprefa[c.seg] + c.pad[2];
    if (ai >= d.ack_max) return;
    Ack a;
    a.chslot = c.pad[0];
    a.kind = c.kind;
    u32 o = c.m_off + 4;
    bool ok = c.m_len >= 13;
    a.tag = ok ? be64(w + o) : 0;
    u32 bits = ok ? w[o + 8] : 0;
    if (c.kind == CK_ACK) { a.multiple = bits & 1; a.requeue = 0; }
    else if (c.kind == CK_REJECT) { a.multiple = 0; a.requeue = bits & 1; }
    else { a.multiple = bits & 1; a.requeue = (bits >> 1) & 1; }
    d.acks[ai] = a;   // marked in the channel's window by marks_range (k_chan_advance resolves it)
  }
}

// K9 marks + K10 confirm counts of the step's commands: the first kernel of the step's
// routing half.  k_decode only records acks and publishes, so the ingest half never
// touches delivery-side state and can run next to the previous step's k_chan_advance /
// k_render (engine overlap).  Also the routing half's per-step resets.
// (fused into k_route_store, phase 0: the marks only have to precede k_chan_advance, and
// the snowflake id floor moved into log_reserve, its one reader -- a launch less per step)
template <bool DLX>
DEV void marks_range(const DS& d, u32 i0, u32 stride) {
  if (i0 == 0 && d.links)
    for (u32 r = 0; r < WORLD_MAX; ++r) d.lk_cnt[r] = 0;
  const u32 na = d.ctr->n_acks, np = d.ctr->n_pubs;
  const u32 n = na > np ? na : np;
  for (u32 i = i0; i < n; i += stride) {
    if (i < na) apply_ack<DLX>(d, d.acks[i], i);
    if (i < np) {
      const u32 ch = d.pubs[i].chslot;
      if (ch != INVALID && d.ch_confirm[ch]) atomicAdd(&d.ch_pub_cnt[ch], 1u);
    }
  }
}

// ============================================================================ scans
// single-block multi-array exclusive scan; n read from device; totals -> tot[slot+k]
// lo != null: scan elements [*lo, *n) (absolute indices), else [0, *n)
// NA <= 4: arrays in[k] / out[k].  NA = 8 (per-rank pairs): array k is in[k & 1] +
// (k >> 1) * stride
struct ScanArgs { const u32* in[4]; u32* out[4]; const u32* n; const u32* lo; u32 narr; u32 nmax; u32 tot_slot; u64 stride; };
// Single-pass exclusive scan over up to NA arrays, 4 elements per thread, 4096-element
// tiles (NA = 8: the per-rank counts of the cross-GPU pack, 4 ranks per launch; 16 arrays
// spill registers; 1024-element tiles lengthen the look-back chain), tiles chained by
// decoupled look-back: each tile publishes its aggregate, then its inclusive prefix, in a
// per-(array, tile) status word tagged with the launch epoch, so the status array never
// needs clearing.  Tickets (not blockIdx) order the tiles, so a tile only ever waits on
// tiles whose blocks are already running.
//   status word = epoch << 34 | flag << 32 | value   (flag 1 = aggregate, 2 = inclusive)
#define SCAN_TILE 4096
// one tile of the scan (1024 threads); true (block-uniform) in the block that holds the
// last data tile, after its totals are written
template <int NA, int EPT>
DEV bool scan_tile(const ScanArgs& a, u32* tot, u64* status, u32* ctl, u32 smax) {
  constexpr u32 TILE = 1024 * EPT;
  __shared__ u32 s_tile, s_epoch;
  __shared__ u32 s_excl[NA];
  __shared__ u32 wsum[NA][1024 / 64 + 1];
  const u32 tid = threadIdx.x;
  if (tid == 0) {
    s_epoch = atomicAdd(&ctl[1], 0u);
    s_tile = atomicAdd(&ctl[0], 1u);
  }
  __syncthreads();
  const u32 tile = s_tile, epoch = s_epoch & 0x3fffffffu;
  const bool last_block = tile == gridDim.x - 1;
  u32 n = a.n ? *a.n : a.nmax;
  if (n > a.nmax) n = a.nmax;
  // lo: elements [lo, lo + n) -- applied at each access (rewriting the argument struct's
  // pointers would copy it to scratch memory)
  const u32 lo = a.lo ? *a.lo : 0u;
  n = n > lo ? n - lo : 0;
  const u32 base = tile * TILE;
  const bool data = base < n || tile == 0;
  if (data) {
    const u32 i = base + tid * EPT;
    u32 v[NA][EPT], off[NA], sm[NA];
    // every array's loads in flight at once, then one block scan of the sums together
#pragma clang loop unroll(full)
    for (int k = 0; k < NA; ++k) {
#pragma clang loop unroll(full)
      for (int e = 0; e < EPT; ++e) v[k][e] = 0;
      if ((u32)k >= a.narr) continue;
      const u32* in = (NA <= 4 ? a.in[k & 3] : a.in[k & 1] + (u64)(k >> 1) * a.stride) + lo;
      if (EPT == 4 && i + 3 < n && !(((uintptr_t)(in + i)) & 15)) {
        uint4 x = *(const uint4*)(in + i);
        v[k][0] = x.x; v[k][EPT > 1 ? 1 : 0] = x.y; v[k][EPT > 2 ? 2 : 0] = x.z; v[k][EPT > 3 ? 3 : 0] = x.w;
      } else {
#pragma clang loop unroll(full)
        for (int e = 0; e < EPT; ++e)
          if (i + e < n) v[k][e] = in[i + e];
      }
    }
    const u32 ln = tid & 63, w = tid >> 6;
    u32 x[NA];
#pragma clang loop unroll(full)
    for (int k = 0; k < NA; ++k) {
      u32 t = 0;
#pragma clang loop unroll(full)
      for (int e = 0; e < EPT; ++e) t += v[k][e];
      sm[k] = t;
      x[k] = t;
    }
#pragma clang loop unroll(full)
    for (int o = 1; o < 64; o <<= 1) {
#pragma clang loop unroll(full)
      for (int k = 0; k < NA; ++k) {
        u32 y = __shfl_up(x[k], o, 64);
        if (ln >= (u32)o) x[k] += y;
      }
    }
    if (ln == 63) {
#pragma clang loop unroll(full)
      for (int k = 0; k < NA; ++k) wsum[k][w] = x[k];
    }
    __syncthreads();
    if (tid < NA) {
      u32 run = 0;
      for (u32 j = 0; j < 1024 / 64; ++j) { u32 t = wsum[tid][j]; wsum[tid][j] = run; run += t; }
      wsum[tid][1024 / 64] = run;
    }
    __syncthreads();
#pragma clang loop unroll(full)
    for (int k = 0; k < NA; ++k) off[k] = wsum[k][w] + x[k] - sm[k];
    // look-back, one wave per array: the wave's 64 lanes read the 64 preceding tiles'
    // status words at once, so a tile waits one round trip for all its (concurrently
    // running) predecessors instead of a chain of them
    const u32 wv = tid >> 6, lane = tid & 63;
    if (wv < a.narr && wv < (u32)NA) {
      const u32 k = wv;
      const u32 A = wsum[k][1024 / 64];   // the tile's aggregate of array k
      // agent-scope (coherent across the XCDs' L2s) relaxed status words: a word carries
      // its own value, nothing else has to become visible with it, so no release fence
      // (an agent-scope release writes back the whole L2: ~1 us per tile, measured)
      u64* st = status + (u64)k * smax;
      const u64 tag = (u64)epoch << 34;
      u32 excl = 0;
      if (tile > 0) {
        if (lane == 0)
          __hip_atomic_store(&st[tile], tag | (1ull << 32) | A, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        u32 top = tile;   // predecessors [0, top) not yet summed
        while (top > 0) {
          const bool has = lane < top;
          const u32 j = has ? top - 1 - lane : 0;   // lane 0 = nearest predecessor
          u64 w = 0;
          if (has) {
            do {
              w = __hip_atomic_load(&st[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } while ((w >> 34) != epoch || ((w >> 32) & 3) == 0);
          }
          const u64 incl = __ballot(has && ((w >> 32) & 3) == 2);
          // sum lanes up to (and including) the nearest inclusive prefix, or the window
          const u32 last = incl ? (u32)(__ffsll((unsigned long long)incl) - 1) : 63u;
          u32 v = (has && lane <= last) ? (u32)w : 0u;
          for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
          excl += v;
          if (incl) break;
          top = top > 64 ? top - 64 : 0;
        }
      }
      if (lane == 0) {
        __hip_atomic_store(&st[tile], tag | (2ull << 32) | (excl + A), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_excl[k] = excl;
        if (base + TILE >= n) tot[a.tot_slot + k] = excl + A;   // the last data tile
      }
    }
    __syncthreads();
#pragma clang loop unroll(full)
    for (int k = 0; k < NA; ++k) {
      if ((u32)k >= a.narr) continue;   // (continue, not break: a single-exit loop unrolls)
      u32 o0 = s_excl[k] + off[k];
      u32* out = (NA <= 4 ? a.out[k & 3] : a.out[k & 1] + (u64)(k >> 1) * a.stride) + lo;
      if (EPT == 4) {
        uint4 o;
        o.x = o0; o.y = o0 + v[k][0]; o.z = o.y + v[k][EPT > 1 ? 1 : 0]; o.w = o.z + v[k][EPT > 2 ? 2 : 0];
        if (i + 3 < n && !(((uintptr_t)(out + i)) & 15)) *(uint4*)(out + i) = o;
        else {
          if (i < n) out[i] = o.x;
          if (i + 1 < n) out[i + 1] = o.y;
          if (i + 2 < n) out[i + 2] = o.z;
          if (i + 3 < n) out[i + 3] = o.w;
        }
      } else {
#pragma clang loop unroll(full)
        for (int e = 0; e < EPT; ++e) {
          if (i + e < n) out[i + e] = o0;
          o0 += v[k][e];
        }
      }
    }
  }
  if (last_block && tid == 0) {   // every block has its ticket: reset for the next launch
    atomicExch(&ctl[0], 0u);
    atomicExch(&ctl[1], epoch + 1);
  }
  return data && base + TILE >= n;
}

template <int NA, int EPT>
__global__ __launch_bounds__(1024) void k_scan(ScanArgs a, u32* tot, u64* status, u32* ctl, u32 smax) {
  (void)scan_tile<NA, EPT>(a, tot, status, ctl, smax);
}

// the route phase's scan (pub_nq, pub_slot, pub_routed, pub_ret_sz) with the phase's
// body-log / message-table reservation done by the block of the last data tile once its
// totals are out (fused: k_route<1> used to reserve, so k_route<1> + k_store can be one)
DEV void log_reserve(const DS& d);
__global__ __launch_bounds__(1024) void k_scan_route(ScanArgs a, u32* tot, u64* status, u32* ctl, u32 smax, DS d) {
  const bool last = scan_tile<4, 4>(a, tot, status, ctl, smax);
  if (last) {
    __syncthreads();   // the totals (tot[TS_ROUTE..]) were written by lane 0 of waves 0..3
    if (threadIdx.x == 0) log_reserve(d);
  }
}

// ============================================================================ radix sort
// stable LSD radix sort of (key, val) u32 pairs, DB bits per pass (8, or 9..11 for keys
// of 9..11 bits in one pass instead of two);
// n from device.  Per-tile digit histograms; the last occupied tile to finish turns them
// into the offsets of the occupied tiles (fused k_rs_offsets).  hist and hscan are both
// tile-major (hist[t * D + digit], hscan[t * D + digit]): the tiles write and the offsets
// pass reads / writes contiguous words, and the queue starts (k_ring_plan / k_enqueue) are
// row 0.  The offsets block keeps up to RS_RT tiles' counts in registers: one round of
// loads, one block scan, one round of stores.
constexpr u32 RS_RT = 16;
constexpr u32 RS_RB = 8;   // past RS_RT tiles: tiles per round of the first pass over the histograms
template <int DB> struct RsNt { static constexpr u32 v = DB > 10 ? 1024u : (DB > 9 ? 512u : 256u); };
template <int DB>
DEV void rs_offsets(const u32* hist, u32* hscan, u32 T, u32* lds) {
  constexpr u32 NT = RsNt<DB>::v, D = 1u << DB, PER = D / NT;   // consecutive digits per thread
  const u32 d0 = threadIdx.x * PER;
  u32 tot[PER];
#pragma unroll
  for (u32 j = 0; j < PER; ++j) tot[j] = 0;
  if (T <= RS_RT) {
    u32 h[RS_RT][PER];
#pragma unroll
    for (u32 a = 0; a < RS_RT; ++a)
#pragma unroll
      for (u32 j = 0; j < PER; ++j) h[a][j] = a < T ? hist[a * D + d0 + j] : 0u;
#pragma unroll
    for (u32 a = 0; a < RS_RT; ++a)
#pragma unroll
      for (u32 j = 0; j < PER; ++j) tot[j] += h[a][j];
    u32 sum = 0;
#pragma unroll
    for (u32 j = 0; j < PER; ++j) sum += tot[j];
    u32 all;
    u32 run = block_scan<NT>(sum, lds, all);
#pragma unroll
    for (u32 j = 0; j < PER; ++j) { const u32 x = tot[j]; tot[j] = run; run += x; }   // digit starts
#pragma unroll
    for (u32 a = 0; a < RS_RT; ++a) {
      if (a >= T) break;
#pragma unroll
      for (u32 j = 0; j < PER; ++j) { hscan[a * D + d0 + j] = tot[j]; tot[j] += h[a][j]; }
    }
    return;
  }
  // many tiles: two passes over the histograms, RB tiles at a time
  constexpr u32 RB = RS_RB;
  u32 t = 0;
  for (; t + RB <= T; t += RB) {
    u32 h[RB][PER];
#pragma unroll
    for (u32 a = 0; a < RB; ++a)
#pragma unroll
      for (u32 j = 0; j < PER; ++j) h[a][j] = hist[(t + a) * D + d0 + j];
#pragma unroll
    for (u32 a = 0; a < RB; ++a)
#pragma unroll
      for (u32 j = 0; j < PER; ++j) tot[j] += h[a][j];
  }
  for (; t < T; ++t) {
#pragma unroll
    for (u32 j = 0; j < PER; ++j) tot[j] += hist[t * D + d0 + j];
  }
  u32 sum = 0;
#pragma unroll
  for (u32 j = 0; j < PER; ++j) sum += tot[j];
  u32 all;
  u32 run = block_scan<NT>(sum, lds, all);
#pragma unroll
  for (u32 j = 0; j < PER; ++j) { const u32 x = tot[j]; tot[j] = run; run += x; }   // digit starts
  for (t = 0; t < T; ++t) {
    u32 h[PER];
#pragma unroll
    for (u32 j = 0; j < PER; ++j) h[j] = hist[t * D + d0 + j];
#pragma unroll
    for (u32 j = 0; j < PER; ++j) { hscan[t * D + d0 + j] = tot[j]; tot[j] += h[j]; }
  }
}

// The occupied tiles' digit histograms of one pass (tile-stride over the blocks), then, in
// the last block to finish (ticket), the tiles' offsets; true (block-uniform) in that block
template <int DB>
DEV bool rs_hist_tiles(const u32* keys, u32 n, u32 shift, u32* hist, u32* hscan, u32* ticket, u32 ntiles) {
  constexpr u32 NT = RsNt<DB>::v, D = 1u << DB;
  __shared__ u32 cnt[D];
  __shared__ u32 lds[NT / 64 + 1];
  __shared__ u32 s_last;
  u32 tid = threadIdx.x, t = blockIdx.x;
  u32 T = (n + SORT_TILE - 1) / SORT_TILE;
  if (T > ntiles) T = ntiles;
  if (t >= T) return false;   // only occupied tiles take part (and take a ticket)
  bool last = false;
  for (; t < T; t += gridDim.x) {   // tile-stride: the grid is capped below ntiles
    for (u32 k = tid; k < D; k += NT) cnt[k] = 0;
    __syncthreads();
    u32 base = t * SORT_TILE;
    for (u32 j = 0; j < SORT_TILE / NT; ++j) {
      u32 i = base + j * NT + tid;
      if (i < n) atomicAdd(&cnt[(keys[i] >> shift) & (D - 1)], 1u);
    }
    __syncthreads();
    // agent-coherent stores + a workgroup-scope release (wait for them) before the
    // ticket: no L2 writeback per tile (__threadfence: +11 us at 15 tiles, measured)
    for (u32 k = tid; k < D; k += NT)
      __hip_atomic_store(&hist[t * D + k], cnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(ticket, 1u) == T - 1;
    __syncthreads();
    last = last || s_last;
  }
  if (!last) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (tid == 0) *ticket = 0;
  rs_offsets<DB>(hist, hscan, T, lds);
  return true;
}

template <int DB>
__global__ __launch_bounds__(RsNt<DB>::v) void k_rs_hist(const u32* keys, const u32* np, u32 shift, u32* hist,
                                                        u32* hscan, u32* ticket, u32 ntiles) {
  (void)rs_hist_tiles<DB>(keys, *np, shift, hist, hscan, ticket, ntiles);
}

// the lanes of this wave whose digit is dg (of the valid ones): one ballot per digit bit
template <int DB>
DEV u64 digit_peers(u32 dg, bool valid) {
  u64 peers = __ballot(valid);
#pragma unroll
  for (u32 bb = 0; bb < DB; ++bb) {
    const u64 m = __ballot((dg >> bb) & 1);
    peers &= ((dg >> bb) & 1) ? m : ~m;
  }
  return peers;
}

template <int DB>
__global__ __launch_bounds__(256) void k_rs_scatter(const u32* kin, const u32* vin, u32* kout, u32* vout,
                                                    const u32* np, u32 shift, const u32* hscan,
                                                    u32 ntiles) {
  constexpr u32 D = 1u << DB;
  __shared__ u32 wc[4][D];
  const u32 tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const u32 n = *np;
  for (u32 t = blockIdx.x; t * SORT_TILE < n; t += gridDim.x) {   // tile-stride (capped grid)
    const u32 base = t * SORT_TILE;
    __syncthreads();   // wc of the previous tile
    for (u32 i = tid; i < 4 * D; i += 256) ((u32*)wc)[i] = 0;
    __syncthreads();
    u32 wbase = base + w * (SORT_TILE / 4);
    // pass 1: per-wave digit counts
    for (u32 c = 0; c < SORT_TILE / 256; ++c) {
      u32 i = wbase + c * 64 + lane;
      bool valid = i < n;
      u32 dg = valid ? (kin[i] >> shift) & (D - 1) : 0;
      u64 peers = digit_peers<DB>(dg, valid);
      bool leader = valid && ((peers & lanemask_lt()) == 0);
      if (leader) wc[w][dg] += __popcll(peers);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    for (u32 dg = tid; dg < D; dg += 256) {
      u32 run = hscan[t * D + dg];
      for (u32 ww = 0; ww < 4; ++ww) { u32 x = wc[ww][dg]; wc[ww][dg] = run; run += x; }
    }
    __syncthreads();
    for (u32 c = 0; c < SORT_TILE / 256; ++c) {
      u32 i = wbase + c * 64 + lane;
      bool valid = i < n;
      u32 key = valid ? kin[i] : 0;
      u32 dg = (key >> shift) & (D - 1);
      u64 peers = digit_peers<DB>(dg, valid);
      u32 basepos = ((volatile u32*)wc[w])[dg];
      u32 rank = __popcll(peers & lanemask_lt());
      if (valid) {
        kout[basepos + rank] = key;
        vout[basepos + rank] = vin[i];
      }
      __builtin_amdgcn_wave_barrier();
      bool leader = valid && ((peers & lanemask_lt()) == 0);
      if (leader) ((volatile u32*)wc[w])[dg] = basepos + __popcll(peers);
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ============================================================================ K6 route
// topic prefilter on MFMA: score[p][b] = keyvec[p] . patvec[b] over 256 int8 lanes;
// a pattern word contributes +32 iff its 32-bit word hash equals the key's.
typedef int v4i __attribute__((ext_vector_type(4)));
DEV void topic_tile(const DS& d, u32 i0, u32 j0, u32 jt, u32 ntb, u32 npub, u32 lane) {
  v4i acc = {0, 0, 0, 0};
  const i8* A = d.pub_keyvec + (u64)(i0 + (lane & 15)) * TOPIC_K + (lane >> 4) * 16;
  const i8* B = d.t_mat + (u64)(j0 + (lane & 15)) * TOPIC_K + (lane >> 4) * 16;
#pragma unroll
  for (int kk = 0; kk < TOPIC_K / 64; ++kk) {
    v4i a = *(const v4i*)(A + kk * 64);
    v4i bv = *(const v4i*)(B + kk * 64);
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bv, acc, 0, 0, 0);
  }
  i32 ex = d.t_expect[j0 + (lane & 15)];
  u64 m0 = __ballot(acc[0] == ex), m1 = __ballot(acc[1] == ex);
  u64 m2 = __ballot(acc[2] == ex), m3 = __ballot(acc[3] == ex);
  if (lane < 16) {  // row = i0 + 4*g + r with g = lane/4, r = lane%4
    u32 g = lane >> 2, r = lane & 3;
    u64 mm = r == 0 ? m0 : r == 1 ? m1 : r == 2 ? m2 : m3;
    u32 rr = i0 + g * 4 + r;
    if (rr < npub) d.pub_match[(u64)rr * ntb + jt] = (u16)((mm >> (16 * g)) & 0xffff);
  }
}

// the topic prefilter tiles of one group of 16 publishes [g0, g0 + 16) (all binding tiles,
// spread over the block's 16 waves); tiles whose publishes all arrived routed (MF_ONEQ /
// MF_RESTORE) or are not topic-routed have nothing to match.  The rows are written to
// pub_match (global: k_route_store re-reads them for publishes with > 8 queues) and made
// visible to the block's waves before they route.
DEV void topic_group(const DS& d, u32 g0, u32 n, u32 w, u32 lane) {
  // the prefilter tiles of the bindings in use only (the tables are packed from row 0): a
  // step of a few publishes on a 4096-row table cost ~68 us here (profiles/r5_coldprof/)
  const u32 nused = d.t_count[0] < d.tb_pad ? d.t_count[0] : d.tb_pad;
  const u32 ntb = d.tb_max ? d.tb_pad >> 4 : 0u;   // (pub_match row stride: every tile)
  const u32 nt = d.tb_max ? (nused + 15) >> 4 : 0u;
  if (nt == 0) return;
  const u32 pi = g0 + lane;
  const bool need = lane < 16 && pi < n && !(d.pubs[pi].flags & (MF_ONEQ | MF_RESTORE));
  if (!__ballot(need)) return;
  for (u32 jt = w; jt < nt; jt += 16) topic_tile(d, g0, jt * 16, jt, ntb, n, lane);
}


// exact check behind an MFMA prefilter hit: same word count (checked) and every non-'*'
// pattern word byte-equal to the key word at its position.  Word offsets are precomputed
// (host: t_woff, decode: pub_kwoff), so the compares of all words issue together instead
// of walking both strings byte by byte.
// bytes of a publish: the step's work buffer, or for a record imported from another
// rank the all-to-all receive buffer itself (k_import_route copies nothing)
DEV const u8* pub_src(const DS& d, const Pub& pb) { return (pb.flags & MF_IMPORTED) ? d.recv_pay : d.work; }

// word i (offset << 8 | length) of a row of TOPIC_WORDS u16 held in one 16-byte load
DEV u32 woff_at(const uint4& v, u32 i) {
  const u32 w = i < 2 ? v.x : i < 4 ? v.y : i < 6 ? v.z : v.w;
  return (w >> (16 * (i & 1))) & 0xffffu;
}

// a binding is a candidate for a publish when its pattern needs the full matcher (flags
// bit 0: '#', long keys) or the word counts agree and the MFMA prefilter bit is set: two
// small loads per binding lane (flags, prefilter row), nothing else for the non-candidates
DEV bool topic_cand(const DS& d, const Pub& pb, u32 pidx, u32 t, u32& fl) {
  fl = d.t_flags[t];
  const u16 mw = d.pub_match[(u64)pidx * (d.tb_pad >> 4) + (t >> 4)];
  return (fl & 1) || ((((fl >> 8) & 0xffu) == pb.nwords) && ((mw >> (t & 15)) & 1));
}

// exact check of a candidate: both word-offset rows (one 16-byte load each) and the
// pattern offset in one round, the word lengths checked without memory, then every byte
// compare issued together (was: word offsets one by one, each a round trip)
DEV bool topic_verify(const DS& d, const Pub& pb, u32 pidx, u32 t, u32 fl) {
  const uint4 pw = *(const uint4*)(d.t_woff + (u64)t * TOPIC_WORDS);
  const uint4 kw = *(const uint4*)(d.pub_kwoff + (u64)pidx * TOPIC_WORDS);
  const u32 kb = d.t_kb_off[t];
  if (fl & 1)   // pattern the prefilter cannot express: full matcher
    return topic_match(d.kpool + kb, d.t_kb_len[t], pub_src(d, pb) + pb.rk_off, pb.rk_len, d.hash_wildcard != 0);
  const u32 nw = pb.nwords < TOPIC_WORDS ? pb.nwords : TOPIC_WORDS;
  const u32 star = (fl >> 16) & 0xffu;
  bool lens_ok = true;
#pragma unroll
  for (u32 i = 0; i < TOPIC_WORDS; ++i)
    if (i < nw && !((star >> i) & 1)) lens_ok &= (woff_at(pw, i) & 255) == (woff_at(kw, i) & 255);
  if (!lens_ok) return false;
  const u8* pat = d.kpool + kb;
  const u8* key = pub_src(d, pb) + pb.rk_off;
  u32 diff = 0;
#pragma unroll
  for (u32 i = 0; i < TOPIC_WORDS; ++i) {
    if (i >= nw || ((star >> i) & 1)) continue;
    const u32 pe = woff_at(pw, i), ke = woff_at(kw, i);
    const u32 len = pe & 255;
    const u8* a = pat + (pe >> 8);
    const u8* b = key + (ke >> 8);
    for (u32 k0 = 0; k0 < len; k0 += 8) {
#pragma unroll
      for (u32 j = 0; j < 8; ++j)
        if (k0 + j < len) diff |= (u32)(a[k0 + j] ^ b[k0 + j]);
    }
  }
  return diff == 0;
}

DEV i32 direct_find(const DS& d, const Pub& pb, i32 exch) {
  u64 k = pb.keyhash ^ (u64(exch) * 0x9E3779B97F4A7C15ULL);
  u32 mask = d.dhash_mask;
  for (u32 j = 0; j <= mask; ++j) {
    u32 s = (u32)(k + j) & mask;
    i32 ex = d.d_exch[s];
    if (ex < 0) return -1;
    if (ex == exch && d.d_key[s] == k &&
        word_eq(d.kpool + d.d_kb_off[s], d.d_kb_len[s], pub_src(d, pb) + pb.rk_off, pb.rk_len))
      return (i32)s;
  }
  return -1;
}

// pass 0: count queues; pass 1: write pairs
// Publishes [tot[RANGE_LO], tot[RANGE_HI]): phase 0 = the step's own, phase 1 = records
// imported from other ranks (sharded queues; only locally owned queues are emitted).
// One wave per publish: the lanes walk the exchange's candidate list (direct queue list,
// fanout list, or topic bindings with their MFMA prefilter bits) 64 entries at a time, so
// a publish costs a few dependent loads instead of one serial chain per binding.
DEV u32 wave_or(u32 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
  return v;
}

template <int PASS>
struct RouteAcc {
  u32 nq = 0, nq_all = 0, rmask = 0;
  u32 nrem = 0, rq = INVALID;   // remote queues matched, the first of them
  bool has_cons = false;
};

// emit one candidate queue per lane (valid lanes), preserving lane order.  qo / qc: the
// queue's owner and consumer count when the caller loaded them already (INVALID: load)
// BAN (the dead view's routing with x-death on): a queue the record's history bans is no
// candidate at all -- counted (n_dl_cycle, pass 0) and otherwise as if its binding were not there.
// The dead pass's record of publish p: its records follow the step's own publishes.  Pass 0 runs
// inside k_import_route, whose block 0 writes tot[TS_RANGE_LO] while the other blocks already
// route: there the base is n_pubs, as for import_one; pass 1 is a later kernel
template <int PASS>
DEV u32 ban_record(const DS& d, u32 p) { return p - (PASS == 0 ? d.ctr->n_pubs : d.tot[TS_RANGE_LO]); }
template <int PASS, bool BAN = false>
DEV void route_emit(const DS& d, RouteAcc<PASS>& a, u32 p, u32 wbase, u32 srank, u32 q, bool valid, u32 lane,
                    u32 qo = INVALID, u32 qc = INVALID) {
  if (BAN) {
    const bool b = valid && xd_banned(d, ban_record<PASS>(d, p), q);
    const u64 bm = __ballot(b);
    if (PASS == 0 && lane == 0 && bm) atomicAdd(&d.ctr->n_dl_cycle, (u32)__popcll(bm));
    valid = valid && !b;
  }
  const u32 me = d.my_rank;
  u32 owner = (valid && d.world > 1) ? (qo != INVALID ? qo : d.q_owner[q]) : me;
  bool remote = valid && owner != me;
  bool local = valid && !remote;
  a.rmask |= wave_or(remote ? (1u << owner) : 0u);
  const u64 rm = __ballot(remote);
  if (rm) {
    if (a.rq == INVALID) a.rq = (u32)__shfl((int)q, (int)(__ffsll((unsigned long long)rm) - 1));
    a.nrem += (u32)__popcll(rm);
  }
  u64 lm = __ballot(local);
  bool cons = local && (qc != INVALID ? qc : d.q_cons_n[q]) != 0;
  if (__ballot(cons || remote)) a.has_cons = true;
  u32 pos = a.nq + (u32)__popcll(lm & lanemask_lt());
  if (local) {
    if (PASS) {
      // every lane counts (a.nq stays uniform over the chunks); only a lane whose pair lies
      // within the pair table stores it, so a full table keeps the pairs of the lowest queues
      // (store_one trims refcnt to those)
      if (wbase + pos < d.pair_max) {
        d.pair_k[0][wbase + pos] = (q << d.rank_bits) | srank;
        d.pair_v[0][wbase + pos] = p;
      }
    } else if (pos < PUB_QC) {
      d.pub_qc[(u64)p * PUB_QC + pos] = q;
    }
  }
  a.nq += (u32)__popcll(lm);
  a.nq_all += (u32)__popcll(__ballot(valid));
}

// ---- exchange-to-exchange bindings: a publish whose entry exchange has outgoing edges
// (x_type & XF_HOP) walks the closure in route pass 0, one wave per publish, through the
// same matchers as every other publish (route_one's loop runs once per visited exchange).
// Visited and pending exchanges are one register each across the wave (lane l: slots
// 32l .. 32l+31); the pending exchange with the lowest slot is matched next and every
// exchange once, so cycles end.  Matching queues collect in a per-wave LDS list (distinct;
// the host keeps every walk's reach within HOP_QMAX at bind time) and go through route_emit
// when the walk is over, so everything downstream of the queue set is the plain path's.
// With more than 8 local queues the local list is also kept in hop_q for pass 1.
struct HopWalk {
  u32* L;            // the wave's queue list
  u32 nl = 0;        // queues in it
  u32 visited = 0, pending = 0;
};

// the walk of an ALT instantiation (alternate exchanges): whether the exchange being matched had a
// destination of its own -- wave-uniform, taken from values the matchers hold anyway (a list's
// length, the last hit) -- and the alternates the walk has taken.  A type of its own, so that the
// other instantiations' walk, and with it their code, is what it was
struct HopWalkAlt : HopWalk {
  bool dest = false;
  u32 nalt = 0;
};

// one candidate per lane: a queue (appended unless listed) or XT_EDGE | destination exchange
DEV void hop_add(HopWalk& h, u32 item, bool valid, u32 lane) {
  const bool isx = valid && (item & XT_EDGE);
  bool isq = valid && !isx;
  if (isq)
    for (u32 i = 0; i < h.nl; ++i)
      if (h.L[i] == item) { isq = false; break; }
  const u64 qm = __ballot(isq);
  const u32 pos = h.nl + (u32)__popcll(qm & lanemask_lt());
  if (isq && pos < HOP_QMAX) h.L[pos] = item;
  h.nl += (u32)__popcll(qm);
  if (h.nl > HOP_QMAX) h.nl = HOP_QMAX;
  __builtin_amdgcn_wave_barrier();
  for (u64 xm = __ballot(isx); xm; xm &= xm - 1) {
    const u32 dst = (u32)__shfl((int)item, (int)(__ffsll((unsigned long long)xm) - 1)) & ~XT_EDGE;
    if (lane == (dst >> 5) && !((h.visited >> (dst & 31)) & 1)) h.pending |= 1u << (dst & 31);
  }
}

// the pending exchange with the lowest slot becomes visited; false when none is left
DEV bool hop_next(HopWalk& h, u32& x, u32 lane) {
  const u64 pm = __ballot(h.pending != 0);
  if (!pm) return false;
  const u32 l0 = (u32)__ffsll((unsigned long long)pm) - 1;
  const u32 bit = (u32)__ffs((int)__shfl((int)h.pending, (int)l0)) - 1;
  if (lane == l0) { h.pending &= ~(1u << bit); h.visited |= 1u << bit; }
  x = l0 * 32 + bit;
  return true;
}

// the walk is over: its queues through route_emit, the local ones kept for pass 1
template <bool BAN = false>
DEV void hop_finish(const DS& d, RouteAcc<0>& a, const HopWalk& h, const Pub& pb, u32 p, u32 srank, u32 lane) {
  __builtin_amdgcn_wave_barrier();
  for (u32 k0 = 0; k0 < h.nl; k0 += 64) {
    const bool v = k0 + lane < h.nl;
    route_emit<0, BAN>(d, a, p, 0, srank, v ? h.L[k0 + lane] : 0u, v, lane);
  }
  // more than 8 local queues: a run of hop_q for pass 1.  Only a publish that is enqueued
  // reserves (an immediate publish without a consumer is returned with 313: no pairs), so
  // the reservations never add up to more than the step's pairs
  if (a.nq <= PUB_QC || ((pb.flags & (MF_IMMEDIATE | MF_IMPORTED)) == MF_IMMEDIATE && !a.has_cons)) return;
  u32 off = lane == 0 ? atomicAdd(&d.tot[TS_HOP_N], a.nq) : 0u;
  off = (u32)__shfl((int)off, 0);
  if (off + a.nq > d.pair_max) {
    // no room: the step's pair table overflows as well; as there, not enqueued and the
    // publisher gets Basic.Nack
    if (lane == 0) {
      atomicAdd(&d.ctr->n_ring_full, a.nq);
      if (pb.chslot != INVALID) d.ch_pub_fail[pb.chslot] = 1u;
    }
    a.nq = 0;
    return;
  }
  u32 n = 0;
  for (u32 k0 = 0; k0 < h.nl; k0 += 64) {
    const bool v = k0 + lane < h.nl;
    const u32 q = v ? h.L[k0 + lane] : 0u;
    bool local = v && (d.world > 1 ? d.q_owner[q] : d.my_rank) == d.my_rank;
    if (BAN) local = local && !xd_banned(d, ban_record<0>(d, p), q);   // (as route_emit refused it above)
    const u64 lm = __ballot(local);
    if (local) d.hop_q[off + n + (u32)__popcll(lm & lanemask_lt())] = q;
    n += (u32)__popcll(lm);
  }
  // pub_qc[0] was stored by route_emit, possibly from another lane: release / acquire at
  // wavefront scope orders lane 0's store after it
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane == 0) d.pub_qc[(u64)p * PUB_QC] = XT_EDGE | off;
}

// ALT (alternate exchanges, pass 0 with the option on): an exchange the walk matched without any
// destination -- no queue and no edge hit, counted before the walk's list and its visited set
// drop what they hold already, and before BAN refuses a queue -- hands the publish to the
// exchange x_alt names, one more pending member of the walk (the rule: control.py route_closure).
// The host gives an exchange with an alternate XF_HOP, so its publishes are walked
template <int PASS, bool BAN = false, bool ALT = false>
DEV void route_one(const DS& d, u32 p, u32 lane) {
  Pub& pb = d.pubs[p];
  // pass 0 of an imported record that arrived with its queue ran in import_one
  if (PASS == 0 && (pb.flags & MF_IMPORTED) && (pb.flags & (MF_ONEQ | MF_RESTORE))) return;
  const u32 wbase = PASS ? d.tot[TS_PAIR_BASE] + d.pub_pair_off[p] : 0;
  // pair key = queue << rank_bits | (source rank >= this rank) (engine.hip): with the
  // stable sort and the generation order (own publishes, then imports by source rank) a
  // queue's messages are ordered by (source rank, connection, publish order) whichever
  // rank owns it
  const u32 srank = d.rank_bits ? (((pb.flags & MF_IMPORTED) ? pb.pad : d.my_rank) >= d.my_rank ? 1u : 0u) : 0u;
  if (PASS == 1) {
    if (lane == 0 && d.pub_ret_sz[p]) atomicMin(&d.conn_ret_min[pb.conn], d.pub_ret_off[p]);
    u32 nq0 = d.pub_nq[p];
    if (nq0 == 0) return;
    if (wbase >= d.pair_max) return;  // capacity: log_reserve clamps the pair count
    const u32 fit = d.pair_max - wbase < nq0 ? d.pair_max - wbase : nq0;
    // routing result cached by pass 0: up to 8 queues in pub_qc; the longer list of a walk
    // (exchange-to-exchange edges) in a run of hop_q, its offset under XT_EDGE in pub_qc[0]
    const u32 q0 = d.pub_qc[(u64)p * PUB_QC];
    if (nq0 <= PUB_QC || (q0 & XT_EDGE)) {
      const u32* run = nq0 <= PUB_QC ? d.pub_qc + (u64)p * PUB_QC : d.hop_q + (q0 & ~XT_EDGE);
      for (u32 k = lane; k < fit; k += 64) {
        d.pair_k[0][wbase + k] = (run[k] << d.rank_bits) | srank;
        d.pair_v[0][wbase + k] = p;
      }
      return;
    }
  }
  RouteAcc<PASS> a;
  const i32 ex = pb.exch;
  if (pb.flags & (MF_RESTORE | MF_ONEQ)) {   // recovered / origin-routed: exactly its queue
    route_emit<PASS, BAN>(d, a, p, wbase, srank, (u32)pb.keyhash, lane == 0, lane);
  } else if (ex >= 0) {
    u32 xt = d.x_type[ex];
    // a walk over exchange-to-exchange edges (pass 0; pass 1 was served from pub_qc / hop_q
    // above): the loop below runs once per visited exchange, candidates go to the walk's list
    const bool hop = PASS == 0 && __builtin_expect((xt & XF_HOP) != 0, 0);
    std::conditional_t<ALT, HopWalkAlt, HopWalk> h;
    u32 x = (u32)ex;
    if (hop) {
      __shared__ u32 hop_list[16][HOP_QMAX];   // (route pass 0 runs at most 16 waves per block)
      h.L = hop_list[threadIdx.x >> 6];
      h.visited = (x >> 5) == lane ? 1u << (x & 31) : 0u;
      xt &= XF_TYPE | XF_HMATCH;
    }
    for (;;) {
      if (xt == EX_DIRECT || xt == EX_FANOUT) {
        u32 o = 0, c = 0, xo = 0, xc = 0;
        const u32* list;
        if (xt == EX_DIRECT) {
          i32 s = lane == 0 ? direct_find(d, pb, (i32)x) : 0;
          s = __shfl(s, 0);
          if (s >= 0) {
            o = d.d_q_off[s]; c = d.d_q_n[s];
            if (hop) { xo = d.d_x_off[s]; xc = d.d_x_n[s]; }
          }
          list = d.d_q;
        } else {
          o = d.x_fan_off[x]; c = d.x_fan_n[x];
          if (hop) { xo = d.x_fanx_off[x]; xc = d.x_fanx_n[x]; }
          list = d.fan_q;
        }
        for (u32 k0 = 0; k0 < c; k0 += 64) {
          bool v = k0 + lane < c;
          u32 q = v ? list[o + k0 + lane] : 0;
          if (__builtin_expect(hop, 0)) hop_add(h, q, v, lane);
          else route_emit<PASS, BAN>(d, a, p, wbase, srank, q, v, lane);
        }
        if (hop) {
          const u32* xl = xt == EX_DIRECT ? d.d_x : d.fan_x;
          for (u32 k0 = 0; k0 < xc; k0 += 64) {
            const bool v = k0 + lane < xc;
            hop_add(h, v ? (xl[xo + k0 + lane] | XT_EDGE) : 0u, v, lane);
          }
          if constexpr (ALT) h.dest = c + xc != 0;
        }
      } else if (PASS == 0 && __builtin_expect(hop && (xt & XF_HMATCH) != 0, 0)) {
        // headers, matched on the bindings' arguments against the publish's own property bytes
        // (an imported record's lie in recv_pay): a row per lane, a queue taken once by its
        // first hit as with the topic rows.  Always as a walk (the host sets XF_HOP with
        // XF_HMATCH, edges or none): the queues go through the walk's list, and above PUB_QC
        // of them into hop_q, so pass 1 never matches again and k_route_store holds no
        // headers code.  (The table is opened and checked again for every 64 rows: opened once
        // in front of this loop, its bounds stay live across hop_add and k_route spills 11
        // VGPRs to scratch -- profiles/headers_match/resource_usage.md)
        if constexpr (PASS == 0) {
          const u32 o = d.x_h_off[x], c = d.x_h_n[x];
          const u8* props = pub_src(d, pb) + hdr_s(pb.props_off);
          const u32 plen = hdr_s(pb.props_len);
          u32 lastq = INVALID;
          for (u32 k0 = 0; k0 < c; k0 += 64) {
            const bool v = k0 + lane < c;
            const u32 r = o + k0 + lane;
            const u32 q = v ? d.h_queue[r] : INVALID;
            const bool hit = headers_hit(props, plen, d.h_meta, d.h_pair, d.hp, d.kpool, r, v, lane);
            const u64 hm = __ballot(hit);
            const u64 below = hm & lanemask_lt();
            const u32 qb = (u32)__shfl((int)q, below ? 63 - __clzll(below) : 0);
            const u32 qtop = (u32)__shfl((int)q, hm ? 63 - __clzll(hm) : 0);
            hop_add(h, q, hit && (below ? qb : lastq) != q, lane);
            if (hm) lastq = qtop;
          }
          if constexpr (ALT) h.dest = lastq != INVALID;   // (a hit row's queue or edge word is never INVALID)
        }
      } else {
        u32 o = d.x_t_off[x], c = d.x_t_n[x];
        u32 lastq = INVALID;
        for (u32 k0 = 0; k0 < c; k0 += 64) {
          bool v = k0 + lane < c;
          u32 t = o + k0 + lane;
          u32 q = INVALID, fl = 0, qo = INVALID, qc = INVALID;
          bool hit = false;
          if (v) {
            q = d.t_queue[t];   // (a walk: or XT_EDGE | destination, the rows after the queues')
            if (topic_cand(d, pb, p, t, fl)) {
              // the queue's owner / consumer count load alongside the exact check's loads
              // (a walk's row may be an edge, and route_emit loads them later: queue 0 here)
              const u32 qi = hop ? 0u : q;
              qo = d.world > 1 ? d.q_owner[qi] : d.my_rank;
              qc = d.q_cons_n[qi];
              hit = topic_verify(d, pb, p, t, fl);
            }
          }
          // bindings are sorted by queue: a queue is emitted once, by its first hit
          u64 hm = __ballot(hit);
          u64 below = hm & lanemask_lt();
          u32 qb = (u32)__shfl((int)q, below ? 63 - __clzll(below) : 0);  // nearest lower hit
          u32 qtop = (u32)__shfl((int)q, hm ? 63 - __clzll(hm) : 0);     // highest hit
          bool emit = hit && (below ? qb : lastq) != q;
          if (__builtin_expect(hop, 0)) hop_add(h, q, emit, lane);
          else route_emit<PASS, BAN>(d, a, p, wbase, srank, q, emit, lane, qo, qc);
          if (hm) lastq = qtop;
        }
        if constexpr (ALT) h.dest = lastq != INVALID;
      }
      if constexpr (ALT && PASS == 0) {
        if (hop && !h.dest) {
          // taken (and counted) unless it was visited already; the host keeps both slots below HOP_XSLOTS
          const i32 al = d.x_alt[x];
          if (al >= 0 && (u32)al < HOP_XSLOTS) {
            const u32 vis = (u32)__shfl((int)h.visited, al >> 5);
            if (!((vis >> (al & 31)) & 1)) {
              hop_add(h, (u32)al | XT_EDGE, lane == 0, lane);
              ++h.nalt;
            }
          }
        }
      }
      if (__builtin_expect(!hop, 1) || !hop_next(h, x, lane)) break;
      xt = d.x_type[x] & (XF_TYPE | XF_HMATCH);
    }
    if constexpr (PASS == 0) {
      if (hop) hop_finish<BAN>(d, a, h, pb, p, srank, lane);
    }
    if constexpr (ALT && PASS == 0) {
      // lane 0 adds the walk's count once.  Counted by the walk of the publish's own rank: an owner's
      // re-match of a record follows the same alternates without counting them again (the dead
      // pass's records are world 1's)
      if (hop && lane == 0 && h.nalt && (d.world == 1 || !(pb.flags & MF_IMPORTED))) atomicAdd(&d.ctr->n_alt, h.nalt);
    }
  }
  if (PASS == 0 && lane == 0) {
    u32 nq = a.nq, rmask = a.rmask;
    u32 ret = 0;
    if (!(pb.flags & MF_IMPORTED))   // a single remote queue travels with the record (MF_ONEQ)
      pb.xid = a.nrem == 1 ? (u64)a.rq : ~0ull;
    if (pb.flags & MF_IMPORTED) {
      rmask = 0;  // imported records are never forwarded again
    } else if (ex < 0 && !(pb.flags & MF_RESTORE)) {
      atomicAdd(&d.ctr->n_unknown_exchange, 1u);
      u32 ri = atomicAdd(&d.ctr->n_ctrl, 1u);
      CtrlRec rec;
      rec.conn = pb.conn; rec.off = INVALID; rec.len = 404; rec.seg = pb.chslot;
      if (ri < d.seg_max * 2) d.ctrl_rec[ri] = rec;
    } else if (a.nq_all == 0) {
      atomicAdd(&d.ctr->n_unroutable, 1u);
      if (pb.flags & MF_MANDATORY) ret = 312;
    } else if ((pb.flags & MF_IMMEDIATE) && !a.has_cons) {
      ret = 313;
      nq = 0;  // spec behaviour: not enqueued (SURVEY A.Q16/CHANGES.md)
    }
    d.pub_ret[p] = ret;
    if (d.world > 1) d.pub_rmask[p] = ret ? 0 : rmask;
    u32 meta = align16(pb.ex_len + pb.rk_len + pb.props_len);
    u32 slot = nq ? align16(meta + pb.body_size) : 0;
    d.pub_nq[p] = nq;
    d.pub_slot[p] = slot;
    d.pub_routed[p] = nq ? 1 : 0;
    pb.nq = nq;
    pb.slot_bytes = slot;
    u32 rsz = 0;
    if (ret) {
      // bytes in the connection's return region; the offset comes from the publish-order
      // scan of pub_ret_sz (returns keep publish order within a connection)
      u32 tl = ret == 312 ? 49u : 72u;  // reply texts (ErrorCodes.scala:23-31)
      u32 sz = (8 + 4 + 2 + 1 + tl + 1 + pb.ex_len + 1 + pb.rk_len) /*method*/ +
               (8 + 12 + pb.props_len) /*header*/;
      u32 fm = d.conn_frame_max[pb.conn];
      u32 fmb = fm ? fm - 8 : 0xffffffffu;
      u32 nb = pb.body_size ? (pb.body_size - 1) / fmb + 1 : 0;   // (no sum: fmb is 2^32 - 1 for frame-max 0)
      sz += pb.body_size + 8 * nb;
      atomicAdd(&d.conn_ret_bytes[pb.conn], sz);
      rsz = sz;
      u32 ri = atomicAdd(&d.ctr->n_returns, 1u);
      if (ri < d.pub_max) d.ret_list[ri] = p;
    }
    d.pub_ret_sz[p] = rsz;
  }
}

// routing pass 0 of the group of 16 publishes [g0, g0 + 16) below n by a 1024-thread block:
// the group's topic prefilter tiles, then wave w routes publish g0 + w
template <bool BAN = false, bool ALT = false>
DEV void route_group(const DS& d, u32 g0, u32 n, u32 w, u32 lane) {
  topic_group(d, g0, n, w, lane);
  __threadfence_block();
  __syncthreads();
  if (g0 + w < n) route_one<0, BAN, ALT>(d, g0 + w, lane);
  __syncthreads();   // the next group's tiles overwrite nothing this group reads, but keep waves together
}

// routing pass 0 (count queues, destination ranks) of the step's own publishes, 16 per
// 1024-thread block: the group's topic prefilter tiles on MFMA (fused k_topic_mfma), then
// one wave per publish.  Pass 1 runs fused with the store (k_route_store) after
// k_scan_route reserved the phase's log region.  The imports' pass 0 is k_import_route.
#ifndef ROUTE_WPE   // k_route occupancy target: 8 (two blocks per CU, 64 VGPRs, 12 VGPRs spilled)
#define ROUTE_WPE 8     // or 4 (one block per CU, no spill): A/B through CHANAMQ_DP_SO
#endif
template <bool ALT>   // (with alternate exchanges on: route_one's rule for an exchange without a destination)
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(ROUTE_WPE))) void k_route(DS d) {
  // the wave index as a scalar: each wave's publish index, and every pointer derived from
  // it, then lives in SGPRs (as a VGPR value it pushed the wave router past 64 VGPRs and
  // into scratch)
  const u32 lane = lane_id(), w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32 lo = d.tot[TS_RANGE_LO];
  u32 n = d.tot[TS_RANGE_HI];
  if (n > d.pub_cap) n = d.pub_cap;
  // a block past the step's publishes leaves before any per-wave set-up: the grid is sized
  // for capacity (2048 blocks), and the register allocator spills loop-invariant state to
  // scratch in the prologue -- 1 KB of HBM writes per idle wave otherwise (PMC WRITE_SIZE)
  if (lo + blockIdx.x * 16 >= n) return;
  for (u32 g0 = lo + blockIdx.x * 16; g0 < n; g0 += gridDim.x * 16) route_group<false, ALT>(d, g0, n, w, lane);
}

// reserve the step's contiguous body-log region and message-table indices
DEV void log_reserve(const DS& d) {
  u32 total = d.tot[TS_ROUTE_SLOT_BYTES];
  u32 routed = d.tot[TS_ROUTE_MSGS];
  u32 np = d.tot[TS_PAIR_BASE] + d.tot[TS_ROUTE_PAIRS];
  d.tot[TS_PAIR_N] = np < d.pair_max ? np : d.pair_max;
  d.ctr->n_pairs = d.tot[TS_PAIR_N];
  // snowflake virtual position base for this step (ID_SLOT_BITS slots per wall-clock ms):
  // never below the step's clock (was k_marks; idempotent for a second routing phase)
  const u64 floor_pos = d.in->id_ms << ID_SLOT_BITS;
  const u64 cur = *d.id_next > floor_pos ? *d.id_next : floor_pos;
  *d.id_base = cur;
  *d.id_next = cur + routed;
  u64 head = *d.log_head, tail = *d.log_tail;
  u64 phys = head % d.log_bytes;
  if (phys + total > d.log_bytes) head += d.log_bytes - phys;
  bool ok = (head + total - tail <= d.log_bytes) && routed <= *d.msg_free_top;
  if (!ok || total == 0) {
    *d.log_step_base = ok ? head : INVALID;
    if (!ok) d.ctr->n_dropped_nomem += routed;
    return;
  }
  *d.log_step_base = head;
  *d.log_head = head + total;
  d.tot[TS_FREE_TOP] = *d.msg_free_top;
  *d.msg_free_top = d.tot[TS_FREE_TOP] - routed;
  d.ctr->n_routed_msgs += routed;
  atomicAdd((unsigned long long*)d.live_bytes, (unsigned long long)total);
}

// live bytes per log block (fused k_live_add), by one wave: the phase's slots are
// contiguous from the step base (slot p at base + pub_slot_off[p]) and a slot counts in
// the block where it starts, as release_msg subtracts it.  Lane l owns log block b0 + l:
// its bytes = S(end of the block) - S(start), S(x) = pub_slot_off of the first slot
// starting at or after x (a prefix sum; binary search, all lanes in parallel).
DEV void live_add_blocks(const DS& d, u32 lane) {
  const u64 head = *d.log_step_base;
  const u32 total = d.tot[TS_ROUTE_SLOT_BYTES];
  if (head == INVALID || total == 0) return;
  const u32 lo = d.tot[TS_RANGE_LO];
  u32 hi = d.tot[TS_RANGE_HI];
  if (hi > d.pub_cap) hi = d.pub_cap;
  const u64 b0 = head / d.log_block, b1 = (head + total - 1) / d.log_block;
  for (u64 g = b0; g <= b1; g += 64) {
    const u64 bk = g + lane;
    u64 s_end = 0, s_beg = 0;
    if (bk <= b1) {
      auto S = [&](u64 x) -> u64 {
        u32 a = lo, b = hi;
        while (a < b) { u32 mid = (a + b) >> 1; if ((u64)d.pub_slot_off[mid] < x) a = mid + 1; else b = mid; }
        return a < hi ? (u64)d.pub_slot_off[a] : (u64)total;
      };
      s_end = bk == b1 ? (u64)total : S((bk + 1) * d.log_block - head);
      s_beg = bk == b0 ? 0 : S(bk * d.log_block - head);
      if (s_end > s_beg)
        atomicAdd((unsigned long long*)&d.log_live[bk % d.n_log_blocks], (unsigned long long)(s_end - s_beg));
    }
  }
}

// a publish in slot layout at dst, by one wave: exchange, routing key, props, then (16-
// aligned) its body fragments; w = the base its offsets are relative to
DEV void write_slot(u8* dst, const u8* w, const Pub& pb, const Frag* frags) {
  wave_copy(dst, w + pb.ex_off, pb.ex_len);
  wave_copy(dst + pb.ex_len, w + pb.rk_off, pb.rk_len);
  wave_copy(dst + pb.ex_len + pb.rk_len, w + pb.props_off, pb.props_len);
  u32 bo = align16(pb.ex_len + pb.rk_len + pb.props_len);
  for (u32 k = 0; k < pb.nfrag; ++k) {
    Frag fg = frags[pb.frag0 + k];
    wave_copy(dst + bo, w + fg.off, fg.len);
    bo += fg.len;
  }
}

// one wave per publish: write its queue pairs (route pass 1), then allocate the message,
// fill its MsgEnt and copy exchange / rk / props / body into the log (fused k_route<1> +
// k_store: one pass over the phase's publishes)
DEV void store_one_pre(const DS& d, u32 p, u32 lane, const Pub& pb, u32 nq, u32 rr, u32 soff, u32 wbase);
template <bool DLX, bool BAN = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void k_route_store(DS d, u32 marks) {
  u32 lane = lane_id();
  if (blockIdx.x == 0 && threadIdx.x < 64) live_add_blocks(d, lane);
  // phase 0 (the step's own commands): K9 ack marks + K10 confirm counts (fused k_marks)
  if (marks) marks_range<DLX>(d, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  u32 n = d.tot[TS_RANGE_HI];
  if (n > d.pub_cap) n = d.pub_cap;
  const u32 nw = (gridDim.x * blockDim.x) >> 6;
  // (wave-uniform, made scalar: the publish's loads and pointers stay in SGPRs)
  const u32 wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  for (u32 p = d.tot[TS_RANGE_LO] + wave; p < n; p += nw) {
    // the store's loads go out before pass 1's pair stores (which the compiler cannot
    // move them past: every table is a global pointer of DS), one round instead of two
    const Pub pb = d.pubs[p];
    const u32 nq = d.pub_nq[p];
    const u32 rr = d.pub_routed_rank[p];
    const u32 soff = d.pub_slot_off[p];
    const u32 wbase = d.tot[TS_PAIR_BASE] + d.pub_pair_off[p];
    route_one<1, BAN>(d, p, lane);
    store_one_pre(d, p, lane, pb, nq, rr, soff, wbase);
  }
}

DEV void store_one_pre(const DS& d, u32 p, u32 lane, const Pub& pb, u32 nq, u32 rr, u32 soff, u32 wbase) {
  if (nq == 0) return;
  u64 base = *d.log_step_base;
  if (base == INVALID) {   // body log / message table full: dropped, confirmed with Basic.Nack
    if (lane == 0) {
      d.pubs[p].msg = INVALID;
      if (pb.chslot != INVALID) d.ch_pub_fail[pb.chslot] = 1u;
    }
    return;
  }
  u32 msg = d.msg_free[d.tot[TS_FREE_TOP] - 1 - rr];
  u64 off = base + soff;
  u8* slot = d.log + (off % d.log_bytes);
  const u8* w = pub_src(d, pb);
  u32 meta = align16(pb.ex_len + pb.rk_len + pb.props_len);
  if ((pb.flags & (MF_IMPORTED | MF_SLOTFMT)) == (MF_IMPORTED | MF_SLOTFMT)) {
    // a record already in slot layout, 16-aligned on both sides: one vector copy
    const uint4* src = (const uint4*)(w + pb.ex_off);
    uint4* dst = (uint4*)slot;
    for (u32 i = lane; i < (pb.slot_bytes >> 4); i += 64) dst[i] = src[i];
  } else {
    write_slot(slot, w, pb, d.frags);
  }
  if (lane == 0) {
    MsgEnt m;
    m.log_off = off;
    u64 pos = (*d.id_base) + rr;
    m.msg_id = (pb.flags & MF_RESTORE) ? pb.xid : snowflake_id(pos, d.in->worker);
    m.ts_ms = pb.ts_ms;
    m.slot_bytes = pb.slot_bytes;
    m.body_len = pb.body_size;
    m.body_off = meta;
    m.props_len = (u16)pb.props_len;
    m.ex_len = (u8)pb.ex_len;
    m.rk_len = (u8)pb.rk_len;
    // pairs past the pair table were not written (route_one): those queues never get
    // the message, so it holds only the references that were enqueued, and the
    // publisher gets Basic.Nack
    const u32 fit = wbase >= d.pair_max ? 0u : (d.pair_max - wbase < pb.nq ? d.pair_max - wbase : pb.nq);
    m.refcnt = (i32)(fit ? fit : 1u);
    m.flags = pb.flags;
    m.pub_step = (u32)d.in->step;
    m.pad = 0;
    m.href = (pb.flags & (MF_HREF | MF_IMPORTED)) == MF_HREF ? d.in->ingress_host + pb.pad : 0ull;
    d.msgs[msg] = m;
    u32 pmsg = msg;
    if (fit < pb.nq) {
      atomicAdd(&d.ctr->n_ring_full, pb.nq - fit);
      if (pb.chslot != INVALID) d.ch_pub_fail[pb.chslot] = 1u;
    }
    if (!fit) {   // freed by k_post: this kernel's waves are still popping the free list
      pmsg = INVALID;
      d.defer_free[atomicAdd(&d.tot[TS_NDEFER], 1u)] = msg;
    }
    d.pubs[p].msg = pmsg;
  }
}

// ============================================================================ sharded queues
// Cross-rank exchange of publishes (SURVEY §3.4 / BASELINE config 3).  Each queue has one
// owning rank; bindings are replicated.  Phase A (the step's own publishes) emits pairs for
// local queues and marks remote owners in pub_rmask; the packers below serialise each such
// publish once per destination rank into [RDesc][payload] send buffers, laid out
// destination-major so one RCCL all_to_all_single moves them.  Phase B imports the
// received records as publishes and routes them against local queues only.

// Inclusive scans, in place, of per-rank values over the wave's first WORLD_MAX lanes.
// Variadic on purpose: a caller scans two or three values, and one call issues the shuffles
// of all of them in each round before any of the adds, as the hand-written loops did; a
// one-value helper called once per value made each value's chain of shuffles wait for the
// one before (three times the dependent LDS round trips).
template <class... U>
DEV void world_scan(u32 lane, U&... x) {
#pragma unroll
  for (u32 o = 1; o < WORLD_MAX; o <<= 1) {
    const u32 y[] = {__shfl_up(x, o, 64)...};
    u32 k = 0;
    if (lane >= o) ((x += y[k++]), ...);
  }
}

// Per-destination record / byte offsets of the step's own publishes (phase A), without
// any inter-block waiting: a block per 1024-publish tile ranks its records per wave and
// destination (ballot: records, shuffle scan: payload bytes), scans the 16 waves' totals
// in LDS and writes tile-relative offsets for the destinations each publish goes to, plus
// the tile's 2W aggregates.  The last tile to finish (ticket) turns the aggregates into
// per-tile prefixes (one wave per value, 64 tiles per round) and the totals
// (tot[TS_XSCAN + 2r], tot[TS_XSCAN + 2r + 1]); k_pack adds the prefix of its tile.
// The tile aggregates are agent-coherent relaxed stores ordered before the ticket by a
// workgroup-scope release: no L2 writeback per tile.
constexpr u32 PK_TILE = 1024;
__global__ __launch_bounds__(1024) void k_pack_scan(DS d, u32* agg, u32* ticket) {
  __shared__ u32 wtot[16][2 * WORLD_MAX];
  __shared__ u32 s_last;
  const u32 tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  u32 n = d.ctr->n_pubs;
  if (n > d.pub_max) n = d.pub_max;
  const u32 W = d.world, V = 2 * W;
  const u32 T = n ? (n + PK_TILE - 1) / PK_TILE : 1;   // tile 0 always runs (publishes totals)
  const u32 tile = blockIdx.x;
  if (tile >= T) return;
  const u32 p = tile * PK_TILE + tid;
  u32 m = 0, sz = 0;
  if (p < n) {
    m = d.pub_rmask[p];
    if (m) {
      const Pub& pb = d.pubs[p];
      sz = align16(align16(pb.ex_len + pb.rk_len + pb.props_len) + pb.body_size);   // slot layout
    }
  }
  u32 myc[WORLD_MAX], myb[WORLD_MAX];
#pragma unroll
  for (u32 r = 0; r < WORLD_MAX; ++r) {
    myc[r] = myb[r] = 0;
    if (r >= W) continue;
    const u32 bit = (m >> r) & 1u;
    const u64 bal = __ballot(bit);
    myc[r] = (u32)__popcll(bal & lanemask_lt());
    const u32 v = bit ? sz : 0u;
    u32 x = v;
#pragma unroll
    for (u32 o = 1; o < 64; o <<= 1) {
      const u32 y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    myb[r] = x - v;
    const u32 bt = (u32)__shfl((int)x, 63);
    if (lane == 0) { wtot[w][2 * r] = (u32)__popcll(bal); wtot[w][2 * r + 1] = bt; }
  }
  __syncthreads();
  if (tid < V) {   // value tid: exclusive offsets of the 16 waves, the tile aggregate
    u32 run = 0;
    for (u32 ww = 0; ww < 16; ++ww) { const u32 t = wtot[ww][tid]; wtot[ww][tid] = run; run += t; }
    __hip_atomic_store(&agg[(u64)tile * 2 * WORLD_MAX + tid], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
#pragma unroll
  for (u32 r = 0; r < WORLD_MAX; ++r) {
    if (r >= W || !((m >> r) & 1u)) continue;
    d.xp_cnt_off[(u64)r * d.pub_cap + p] = wtot[w][2 * r] + myc[r];
    d.xp_byt_off[(u64)r * d.pub_cap + p] = wtot[w][2 * r + 1] + myb[r];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the agent-coherent agg stores are done
  __syncthreads();
  if (tid == 0) s_last = atomicAdd(ticket, 1u) == T - 1;
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (tid == 0) *ticket = 0;
  // aggregates -> per-tile exclusive prefixes, in place; totals
  for (u32 v = w; v < V; v += 16) {
    u32 carry = 0;
    for (u32 t0 = 0; t0 < T; t0 += 64) {
      const u32 t = t0 + lane;
      const u32 a = t < T ? __hip_atomic_load(&agg[(u64)t * 2 * WORLD_MAX + v], __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT) : 0u;
      u32 x = a;
#pragma unroll
      for (u32 o = 1; o < 64; o <<= 1) {
        const u32 y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
      }
      if (t < T) agg[(u64)t * 2 * WORLD_MAX + v] = carry + x - a;
      carry += (u32)__shfl((int)x, 63);
    }
    if (lane == 0) d.tot[TS_XSCAN + v] = carry;
  }
}

// one wave per local publish with remote owners: write one record per destination.
// Fused k_pack_bases: every block turns the per-rank totals of k_pack_scan into destination bases
// itself (one wave, lane r = rank r, one load round trip and a shuffle scan); block 0
// also publishes the send counts to the host-visible words
DEV void pack_one(const DS& d, u32 p, u32 lane, const u32* s_base);
__global__ __launch_bounds__(256) void k_pack(DS d) {
  __shared__ u32 s_base[2 * WORLD_MAX];
  const u32 tid = threadIdx.x, lane = lane_id();
  if (tid < 64) {
    const bool v = lane < d.world;
    const u32 c = v ? d.tot[TS_XSCAN + 2 * lane] : 0u, b = v ? d.tot[TS_XSCAN + 2 * lane + 1] : 0u;
    u32 sc = c, sb = b;
    world_scan(lane, sc, sb);   // (lane r = rank r)
    if (v) { s_base[lane] = sc - c; s_base[WORLD_MAX + lane] = sb - b; }
    if (blockIdx.x == 0) {
      if (v) { d.xs_base[lane] = sc - c; d.xs_base[WORLD_MAX + lane] = sb - b; d.xchg[lane] = c; d.xchg[WORLD_MAX + lane] = b; }
      const u32 dsum = (u32)__shfl((int)sc, (int)d.world - 1), psum = (u32)__shfl((int)sb, (int)d.world - 1);
      if (lane == 0) d.xchg[4 * WORLD_MAX] = (dsum > d.xfer_desc_max || psum > d.xfer_bytes) ? 1u : 0u;
    }
  }
  __syncthreads();
  const u32 n = d.ctr->n_pubs, nw = (gridDim.x * blockDim.x) >> 6;
  for (u32 p = (blockIdx.x * blockDim.x + tid) >> 6; p < n; p += nw) pack_one(d, p, lane, s_base);
}

DEV void pack_one(const DS& d, u32 p, u32 lane, const u32* s_base) {
  u32 m = d.pub_rmask[p];
  if (!m) return;
  const Pub pb = d.pubs[p];
  const u8* w = d.work;
  while (m) {
    u32 r = __builtin_ctz(m);
    m &= m - 1;
    // tile prefix (k_pack_scan) + offset within the tile
    const u32* tp = d.pk_agg + (u64)(p / PK_TILE) * 2 * WORLD_MAX;
    u32 di = s_base[r] + tp[2 * r] + d.xp_cnt_off[(u64)r * d.pub_cap + p];
    u32 rel = tp[2 * r + 1] + d.xp_byt_off[(u64)r * d.pub_cap + p];
    u64 po = (u64)s_base[WORLD_MAX + r] + rel;
    // the record is laid out as the owner's body-log slot (MF_SLOTFMT)
    const u32 meta = align16(pb.ex_len + pb.rk_len + pb.props_len);
    u32 sz = align16(meta + pb.body_size);
    if (di >= d.xfer_desc_max || po + sz > d.xfer_bytes) continue;  // overflow flagged by k_pack_bases
    write_slot(d.send_pay + po, w, pb, d.frags);
    if (lane == 0) {
      RDesc rd{};
      rd.pay_off = rel;
      rd.body_len = pb.body_size;
      rd.props_len = pb.props_len;
      rd.exch = pb.exch;
      rd.flags = (pb.flags & (MF_PERSIST | MF_HAS_TS)) | MF_SLOTFMT;
      if (pb.xid != ~0ull) {   // the owner skips re-routing: its one queue is known
        rd.flags |= MF_ONEQ;
        rd.tq = (u32)pb.xid;
      }
      rd.ex_len = (u8)pb.ex_len;
      rd.rk_len = (u8)pb.rk_len;
      rd.expire_ms = pb.expire_ms;
      rd.ts_ms = pb.ts_ms;
      d.send_desc[di] = rd;
    }
  }
}

// Phase B head: one kernel imports the received records and applies the received link
// acks (fused k_import_prep + k_link_acks).  Every block derives the per-source bases from
// the received counts (host-mapped xchg) itself -- one wave, lane r = source r, one load
// round trip and a shuffle scan -- and block 0 also publishes the import range for the
// kernels after it.  xr: [0,W) record bases, [W,2W) byte bases, [2W,3W) publish records
// of each source (the link deliveries after them have payload offsets past the publish
// bytes, [3W,4W): native exchange, engine.hip exchange()).  The same kernel runs routing
// pass 0 of the imports (fused k_topic_mfma + k_route): 16 records per 1024-thread block
// -- 16 threads import them, the block computes their topic tiles, one wave per record
// routes it (records that arrived with their queue were routed by import_one and return
// at once)
DEV void import_one(const DS& d, u32 i, const u32* xr);
DEV void link_ack_one(const DS& d, u32 i);
// (BAN: the dead view's launch with x-death on, route_emit's ban check; ALT: with alternate exchanges on)
template <bool BAN, bool ALT = false>
__global__ __launch_bounds__(1024) void k_import_route(DS d) {
  __shared__ u32 xr[4 * WORLD_MAX];
  __shared__ u32 s_n, s_k;
  const u32 tid = threadIdx.x;
  if (tid < 64) {
    const u32 lane = tid;
    const bool v = lane < d.world;
    const u32 cn = v ? d.xchg[XC_RECV_N + lane] : 0u, cb = v ? d.xchg[XC_RECV_B + lane] : 0u;
    const u32 an = v ? d.xchg[XC_RECV_AN + lane] : 0u, ab = v ? d.xchg[XC_RECV_AB + lane] : 0u;
    const u32 rk = (v && d.links) ? d.xchg[XC_RACK_N + lane] : 0u;
    u32 sn = cn, sb = cb, sk = rk;
    world_scan(lane, sn, sb, sk);   // (lane r = source r)
    if (v) { xr[lane] = sn - cn; xr[WORLD_MAX + lane] = sb - cb; xr[2 * WORLD_MAX + lane] = an; xr[3 * WORLD_MAX + lane] = ab; }
    const u32 last = d.world - 1;
    const u32 dsum = (u32)__shfl((int)sn, (int)last), psum = (u32)__shfl((int)sb, (int)last);
    const u32 nk = (u32)__shfl((int)sk, (int)last);
    const bool fits = dsum <= d.import_max && psum <= d.import_bytes;
    const u32 ni = fits ? dsum : 0u;
    const u32 kcap = (d.world - 1) * d.lk_cap;
    const u32 nr = d.links ? (nk < kcap ? nk : kcap) : 0u;
    if (lane == 0) { s_n = ni; s_k = nr; }
    if (blockIdx.x == 0) {
      if (v)
        for (u32 k = 0; k < 4; ++k) d.xr_base[k * WORLD_MAX + lane] = xr[k * WORLD_MAX + lane];
      if (lane == 0) {
        if (!fits) d.ctr->n_dropped_nomem += dsum;
        d.tot[TS_NRACK] = nr;
        d.tot[TS_NIMPORT] = ni;
        d.tot[TS_IMPORT_BASE] = 0;   // imported bytes stay in the receive buffer (pub_src)
        d.tot[TS_RANGE_LO] = d.ctr->n_pubs;
        d.tot[TS_RANGE_HI] = d.ctr->n_pubs + ni;
        d.tot[TS_PAIR_BASE] = d.tot[TS_PAIR_N];
      }
    }
  }
  __syncthreads();
  const u32 n = s_n, nk = s_k;
  const u32 g = blockIdx.x * blockDim.x + tid, gs = gridDim.x * blockDim.x;
  for (u32 i = g; i < nk; i += gs) link_ack_one(d, i);
  const u32 base = d.ctr->n_pubs, lane = tid & 63, w = tid >> 6;
  for (u32 g0 = blockIdx.x * 16; g0 < n; g0 += gridDim.x * 16) {
    if (tid < 16 && g0 + tid < n) import_one(d, g0 + tid, xr);
    __threadfence_block();
    __syncthreads();
    route_group<BAN, ALT>(d, base + g0, base + n, w, lane);
  }
}

// one thread per received record -> imported Publish whose bytes stay in recv_pay (no
// copy: a thread builds the record's key hash / key vector, as k_decode does per publish)
DEV void import_one(const DS& d, u32 i, const u32* xr) {
  u32 src = 0;
  for (u32 r = 1; r < d.world; ++r)
    if (xr[r] <= i) src = r;
  const RDesc rd = d.recv_desc[i];
  const u32 lpart = i - xr[src] >= xr[2 * WORLD_MAX + src] ? xr[3 * WORLD_MAX + src] : 0u;
  const u32 roff = xr[WORLD_MAX + src] + lpart + rd.pay_off;
  const u32 wo = roff;   // offsets relative to recv_pay (MF_IMPORTED, pub_src)
  u32 pi = d.ctr->n_pubs + i;
  Pub pb;
  pb.conn = INVALID;
  pb.chslot = INVALID;
  pb.exch = rd.exch;
  pb.ex_off = wo;
  pb.ex_len = rd.ex_len;
  pb.rk_off = wo + rd.ex_len;
  pb.rk_len = rd.rk_len;
  pb.props_off = pb.rk_off + rd.rk_len;
  pb.props_len = rd.props_len;
  u32 fi = d.frag_max + i;  // imported bodies live past the step's own fragments
  d.frags[fi] = Frag{(rd.flags & MF_SLOTFMT) ? wo + align16(rd.ex_len + rd.rk_len + rd.props_len)
                                            : pb.props_off + rd.props_len, rd.body_len};
  pb.frag0 = fi;
  pb.nfrag = rd.body_len ? 1 : 0;
  pb.body_size = rd.body_len;
  pb.flags = rd.flags | MF_IMPORTED;
  pb.expire_ms = rd.expire_ms;
  pb.ts_ms = rd.ts_ms;
  const u8* key = d.recv_pay + roff + rd.ex_len;
  const bool routed = rd.flags & (MF_RESTORE | MF_ONEQ);   // target queue in tq, no matching
  pb.keyhash = routed ? (u64)rd.tq : fnv1a64_dev(key, rd.rk_len);
  pb.nwords = routed ? 0u : build_keyvec(d, key, rd.rk_len, pi);
  pb.nq = 0; pb.slot_bytes = 0; pb.msg = INVALID; pb.xid = rd.xid;
  pb.pad = src;  // source rank (pair ordering)
  if (rd.flags & MF_HOSTPUB) {   // the publisher's channel: confirm counting, Nack on a drop
    pb.chslot = rd.pad[0];
    pb.conn = rd.pad[1];
    if (pb.chslot < d.c_max * d.chpc && d.ch_confirm[pb.chslot]) atomicAdd(&d.ch_pub_cnt[pb.chslot], 1u);
  }
  if (routed) {
    // routing pass 0 for a record that arrived with its queue (what route_one<0> computes
    // for it: one local queue, no return, never forwarded); route_one<0> skips it
    const u32 q = rd.tq;
    const u32 nq = (d.world == 1 || d.q_owner[q] == d.my_rank) ? 1u : 0u;
    const u32 slot = nq ? align16(align16(pb.ex_len + pb.rk_len + pb.props_len) + pb.body_size) : 0u;
    pb.nq = nq;
    pb.slot_bytes = slot;
    d.pub_qc[(u64)pi * PUB_QC] = q;
    d.pub_nq[pi] = nq;
    d.pub_slot[pi] = slot;
    d.pub_routed[pi] = nq;
    d.pub_ret[pi] = 0;
    d.pub_ret_sz[pi] = 0;
    if (d.world > 1) d.pub_rmask[pi] = 0;
  }
  d.pubs[pi] = pb;
}

// ============================================================================ dead pass (DS.dlx)
// The entries on the dead list become publishes to their queues' dead-letter exchanges, in
// the step after the one they died in: k_dead_pack renders them as import records (RDesc +
// [exchange name][routing key][props][body] in slot layout) into the dead-letter buffers, and
// k_import_route / k_scan_route / k_route_store, given a DS view whose receive side is those
// buffers, route and store them behind the step's own publishes -- the order phase B of a
// sharded step uses -- for the step's one sort and enqueue.
//
// Phase 0, one 1024-thread block: the pending items ordered by (step died, queue slot, queue
// position, reason, channel slot, tag) -- a total order, whatever order the blocks of
// k_dequeue and k_chan_advance appended them in -- by counting ranks over the keys in LDS
// (32 KB; each thread compares its key with every other, an LDS broadcast per read); the
// longest prefix that fits the pass's records (`room`) and payload (dead_bytes) is taken, the
// rest moves to the list's front.  An item whose record is larger than the whole payload
// buffer, or whose body went to the cold store, is taken without a record (n_dl_dropped); a
// hole (msg INVALID) is taken silently.  Phase 1, one wave per taken item: its record and
// payload, then the list's reference is dropped.  Phase 2, after the pass's routing: the records
// that reached no queue are counted (n_dl_unrouted).
DEV bool dead_key_less(const u64* a, const u64* b) {
  if (a[0] != b[0]) return a[0] < b[0];
  if (a[1] != b[1]) return a[1] < b[1];
  if (a[2] != b[2]) return a[2] < b[2];
  return a[3] < b[3];
}
// record bytes of item `it` in slot layout (0: a hole); *lens = exchange name | key << 8 bytes
// (plen: the property bytes the record gets -- x-death's new length; INVALID: the message's own)
DEV u32 dead_rec_size(const DS& d, const DeadItem& it, u32* lens, bool* cold, u32 plen = INVALID) {
  *lens = 0;
  *cold = false;
  if (it.msg == INVALID) return 0;
  const MsgEnt& m = d.msgs[it.msg];
  const u32 ql = d.dl->q_dl_len[it.q];
  const u32 exl = ql & 255u, rkl = (ql & DLQ_HAS_KEY) ? ((ql >> 8) & 255u) : (u32)m.rk_len;
  *lens = exl | (rkl << 8);
  *cold = (m.log_off & COLD_BIT) != 0;
  return align16(align16(exl + rkl + (plen != INVALID ? plen : (u32)m.props_len)) + m.body_len);
}
// XD (DlState.xdeath): the sizes are k_dead_size's, phase 1 rewrites the property bytes and fills
// the record's ban row (dp_xdeath.h); without it the kernel is the one it was
// PRIO (DS.prio, with XD): the ban row's entry for the source queue is its base slot
template <bool XD, bool PRIO = false>
__global__ __launch_bounds__(1024) void k_dead_pack(DS d, u32 phase, u32 room) {
  const u32 tid = threadIdx.x, lane = lane_id();
  if (phase == 0) {
    __shared__ u64 key[DEAD_LIST_MAX][4];
    __shared__ u32 perm[DEAD_LIST_MAX];
    __shared__ u32 lds[1024 / 64 + 1];
    __shared__ u32 s_take;
    if (blockIdx.x) return;
    u32 n = d.dl->dead_n[0];
    if (n > d.dl->dead_max) n = d.dl->dead_max;
    if (n == 0) {   // block-uniform: nothing pending, the pass imports nothing
      if (tid == 0) {
        d.dl->dead_n[1] = 0;
        d.dl->dead_xchg[XC_RECV_N] = d.dl->dead_xchg[XC_RECV_B] = d.dl->dead_xchg[XC_RECV_AN] = d.dl->dead_xchg[XC_RECV_AB] = 0;
      }
      return;
    }
    if (tid < n) {
      const DeadItem it = d.dl->dead[tid];
      key[tid][0] = ((u64)it.step << 32) | it.q;
      key[tid][1] = it.qpos;
      key[tid][2] = ((u64)it.reason << 32) | it.ch;
      key[tid][3] = it.tag;
    }
    if (tid == 0) s_take = n;
    __syncthreads();
    if (tid < n) {
      u32 r = 0;
      for (u32 j = 0; j < n; ++j) r += (dead_key_less(key[j], key[tid]) || (j < tid && !dead_key_less(key[tid], key[j]))) ? 1u : 0u;
      perm[r] = tid;
    }
    __syncthreads();
    // thread t: the item at ordered position t (read before anything is written back)
    DeadItem it;
    it.msg = INVALID; it.q = 0; it.qpos = 0; it.step = 0; it.reason = 0; it.ch = 0; it.xs = 0; it.tag = 0;
    u32 sz = 0, lens = 0, plen = INVALID;
    bool cold = false, over = false;
    if (tid < n) {
      it = d.dl->dead[perm[tid]];
      if (XD) {   // (INVALID: the rewrite is over a limit -- dropped like a record larger than the buffer)
        plen = d.dl->dead_plen[perm[tid]];
        over = plen == INVALID;
      }
      sz = dead_rec_size(d, it, &lens, &cold, plen);
    }
    const bool hole = tid < n && it.msg == INVALID;
    const bool drop = tid < n && !hole && (cold || over || (u64)sz > d.dl->dead_bytes);
    const bool rec = tid < n && !hole && !drop;
    u32 tot_b, tot_r;
    const u32 off = block_scan<1024>(rec ? sz : 0u, lds, tot_b);
    const u32 ri = block_scan<1024>(rec ? 1u : 0u, lds, tot_r);
    // (offsets grow with the position: the first item that does not fit ends the prefix)
    if (rec && (ri >= room || (u64)off + sz > d.dl->dead_bytes)) atomicMin(&s_take, tid);
    __syncthreads();
    const u32 take = s_take;
    if (tid < take) {
      d.dl->dead_take[tid] = it;
      d.dl->dead_off[2 * tid] = rec ? ri : INVALID;
      d.dl->dead_off[2 * tid + 1] = off;
      if (XD) d.dl->dead_plen[tid] = plen;   // (every read of the list-order values lies before the barrier above)
      if (drop) atomicAdd(&d.ctr->n_dl_dropped, 1u);
    } else if (tid < n) {
      d.dl->dead[tid - take] = it;
    }
    if (tid == (take ? take - 1 : 0u)) {   // the pass's totals: those of the last taken item
      const u32 nr = take ? ri + (rec ? 1u : 0u) : 0u, nb = take ? off + (rec ? sz : 0u) : 0u;
      d.dl->dead_n[0] = n - take;
      d.dl->dead_n[1] = take;
      d.dl->dead_xchg[XC_RECV_N] = d.dl->dead_xchg[XC_RECV_AN] = nr;
      d.dl->dead_xchg[XC_RECV_B] = d.dl->dead_xchg[XC_RECV_AB] = nb;
    }
    return;
  }
  if (phase == 2) {
    // behind the pass's routing: a dead letter its exchange routed to no queue is lost, and counted
    // (here, not in route_one: the routing kernels are the ones every publish of every step runs)
    u32 hi = d.tot[TS_RANGE_HI];
    if (hi > d.pub_cap) hi = d.pub_cap;
    const u32 gs = gridDim.x * blockDim.x;
    for (u32 p0 = d.tot[TS_RANGE_LO] + blockIdx.x * blockDim.x; p0 < hi; p0 += gs) {   // (wave-uniform trips)
      const u32 p = p0 + tid;
      const u64 m = __ballot(p < hi && d.pub_nq[p] == 0);
      if (lane == 0 && m) atomicAdd(&d.ctr->n_dl_unrouted, (u32)__popcll(m));
    }
    return;
  }
  // phase 1: one wave per taken item
  const u32 take = d.dl->dead_n[1] < d.dl->dead_max ? d.dl->dead_n[1] : d.dl->dead_max;
  const u32 nw = (gridDim.x * blockDim.x) >> 6;
  for (u32 t = (blockIdx.x * blockDim.x + tid) >> 6; t < take; t += nw) {
    const DeadItem it = d.dl->dead_take[t];
    const u32 ri = d.dl->dead_off[2 * t], off = d.dl->dead_off[2 * t + 1];
    if (ri != INVALID && it.msg != INVALID) {
      const MsgEnt m = d.msgs[it.msg];
      const u32 ql = d.dl->q_dl_len[it.q];
      const u32 exl = ql & 255u;
      const bool own = !(ql & DLQ_HAS_KEY);
      const u32 rkl = own ? (u32)m.rk_len : ((ql >> 8) & 255u);
      const u8* slot = msg_slot(d, m.log_off);
      const u8* names = d.dl->q_dl_name + (u64)it.q * (2 * DLQ_STR);
      u8* dst = d.dl->dead_pay + off;
      wave_copy(dst, names, exl);
      wave_copy(dst + exl, own ? slot + m.ex_len : names + DLQ_STR, rkl);
      u32 plen = m.props_len;
      bool bad = false;
      if (XD) {
        u32* ban_n = d.dl->dead_ban_n + ri;
        plen = xd_render(d, it, m, slot, dst + exl + rkl, d.dl->dead_plen[t], d.dl->dead_ban + (u64)ri * XD_ELEMS_MAX, ban_n, lane);
        bad = plen == INVALID;   // (the two passes disagree: never; the record then names no exchange and carries nothing)
        // a dead letter of a priority queue's lane: routing emits base slots and the history's names
        // resolve to base slots, so the source queue's own entry (xd_render: row[0]) is the base slot too
        if (PRIO && !bad && it.reason != DL_REJECTED && lane == 0)
          d.dl->dead_ban[(u64)ri * XD_ELEMS_MAX] = d.q_lane_base[it.q];
        if (bad) {
          plen = 0;
          if (lane == 0) *ban_n = 0;
        }
      } else {
        wave_copy(dst + exl + rkl, slot + m.ex_len + m.rk_len, m.props_len);
      }
      if (!bad) wave_copy(dst + align16(exl + rkl + plen), slot + m.body_off, m.body_len);
      if (lane == 0) {
        RDesc rd{};
        rd.pay_off = off;
        rd.body_len = bad ? 0u : m.body_len;
        rd.props_len = plen;
        rd.exch = bad ? -1 : (i32)it.xs;
        // a new message without a publisher: never mandatory or immediate, never expiring again
        // by its own property (the target queue's x-message-ttl still applies at its enqueue)
        rd.flags = (m.flags & (MF_PERSIST | MF_HAS_TS)) | MF_SLOTFMT;
        rd.ex_len = (u8)exl;
        rd.rk_len = (u8)rkl;
        rd.expire_ms = 0;
        rd.ts_ms = m.ts_ms;
        rd.pad[0] = it.q;        // (source queue and reason: read by nothing; x-death works from the item itself)
        rd.pad[1] = it.reason;
        d.dl->dead_desc[ri] = rd;
      }
    }
    wave_release(d, it.msg, lane == 0);   // the list's reference (a hole: nothing)
  }
}

// ============================================================================ K7 enqueue
__global__ void k_qfirst(DS d, u32 src) {
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  u32 n = d.tot[TS_PAIR_N];
  if (i >= n) return;
  const u32* k = d.pair_k[src];
  const u32 rb = d.rank_bits;
  if (i == 0 || (k[i - 1] >> rb) != (k[i] >> rb)) d.q_first[k[i] >> rb] = i;
}

// publish p's entry at position `rank` of this step's entries for queue q (`last`: the
// queue's last pair, which moves q_tail); returns the message to release if the ring is full
// a pair's enqueue in two halves: every load (the publish, the queue's ring state), then
// the stores -- so a kernel can have the loads of several pairs in flight at once
struct EnqLoad {
  u32 msg = INVALID, flags = 0, chslot = INVALID;
  u64 head = 0, tail = 0, mask = 0, ring_off = 0;
  i64 expire_ms = 0, ttl = 0;
  bool durable = false;
  u32 ql = 0;   // the queue's length limit (q_limit; 0 with DS.limits off)
  u32 kq = INVALID;   // BL: K_q of a reject-publish queue with a byte limit (q_broom; INVALID: no such limit)
};
template <bool BL = false>   // DS.blimits as a compile-time constant, like DLX: the flag-off kernels hold none of it
DEV EnqLoad enq_load(const DS& d, u32 q, u32 p) {
  const Pub& pb = d.pubs[p];
  EnqLoad e;
  e.msg = pb.msg;
  e.flags = pb.flags;
  e.chslot = pb.chslot;
  e.expire_ms = pb.expire_ms;
  // the queue's last pair moves q_tail in this kernel: every pair reads the tail that
  // k_ring_plan recorded before the enqueue, never q_tail itself
  e.head = d.q_head[q];
  e.tail = d.q_enq_tail[q];
  e.mask = d.q_ring_mask[q];
  e.ring_off = d.q_ring_off[q];
  e.ttl = d.q_ttl[q];
  e.durable = d.persist && d.q_durable[q];
  if (d.limits) e.ql = d.q_limit[q];   // kernel-uniform
  if (BL) {
    if (ql_reject(e.ql) && d.q_blimit[q]) e.kq = d.q_broom[q];
  }
  return e;
}
// `limited`: the dropped pair was refused by the queue's x-max-length (reject-publish), not by its ring
DEV u32 enq_store(const DS& d, const EnqLoad& l, u32 q, u32 rank, bool last, PersistRec* pr, bool* limited) {
  const u64 cap = l.mask + 1;
  u64 freec = cap - (l.tail - l.head);
  u32 drop = INVALID;
  if (l.msg == INVALID) return INVALID;
  if (ql_reject(l.ql)) {
    // reject-publish: room for L ready entries, the step's earlier pairs of the queue counted by
    // their rank; requeues may have put the depth above L (room zero, never negative).  The
    // limit is asked before the ring: where both end at the same pair (a ring of exactly L
    // slots, or one a requeue filled) the refusal is the limit's
    const u64 depth = l.tail - l.head, len = ql_len(l.ql);
    const u64 room = len > depth ? len - depth : 0;
    if (room <= freec) { freec = room; *limited = true; }
  }
  // x-max-length-bytes, reject-publish: the first K_q pairs of the queue pass the byte rule
  // (k_byte_room); asked before the ring like the count limit, and the smaller of the two decides
  if (l.kq != INVALID && l.kq <= freec) { freec = l.kq; *limited = true; }
  if (rank < freec) {
    u64 pos = l.tail + rank;
    Desc ds;
    ds.msg = l.msg;
    ds.flags = (l.flags & MF_REDELIVERED) ? 1u : 0u;
    i64 e = l.expire_ms;
    if (l.ttl > 0) { i64 qe = d.in->now_ms + l.ttl; e = (e == 0 || qe < e) ? qe : e; }
    ds.expire_ms = e;
    d.ring[l.ring_off + (pos & l.mask)] = ds;
    if (l.durable && (l.flags & MF_PERSIST) && !(l.flags & MF_RESTORE)) {
      pr->msg = l.msg; pr->q = q; pr->qpos = pos; pr->expire_ms = e;
    }
  } else {
    drop = l.msg;
    if (l.chslot != INVALID) d.ch_pub_fail[l.chslot] = 1u;   // confirmed with Basic.Nack
  }
  if (last) {
    u64 cnt = rank + 1;
    u64 nt = l.tail + (cnt < freec ? cnt : freec);
    d.q_tail[q] = nt;
  }
  return drop;
}
template <bool BL>
DEV u32 enqueue_one(const DS& d, u32 src, u32 i, u32 n, PersistRec* pr, bool* limited) {
  const u32* kk = d.pair_k[src];
  const u32 rb = d.rank_bits;
  u32 q = kk[i] >> rb;
  u32 p = d.pair_v[src][i];
  u32 first = d.q_first[q];   // the queue's first pair (k_qfirst)
  return enq_store(d, enq_load<BL>(d, q, p), q, i - first, (i + 1 == n) || (kk[i + 1] >> rb) != q, pr, limited);
}
// after a pair's enqueue (whole waves: wave collectives): release the message a full ring
// (or a reject-publish queue at its limit) dropped and count it by the reason; record a
// persistent message's enqueue for the store
DEV void enqueue_done(const DS& d, u32 drop, bool limited, const PersistRec& pr) {
  wave_release(d, drop, drop != INVALID);
  if (drop != INVALID) atomicAdd(limited ? &d.ctr->n_maxlen_rejected : &d.ctr->n_ring_full, 1u);
  if (d.persist) {
    const bool want = pr.msg != INVALID;
    const u32 k = wave_reserve(&d.ctr->n_persist, want);
    if (want && k < d.persist_max) d.prec[k] = pr;
  }
}

// ---- unbounded queues (QueueEntity.scala:271-316 keeps a growing Vector): before the
// step's enqueue, the last pair of every queue checks that the queue's ring holds this
// step's entries; if not, the ring moves to one of >= 2x the needed size taken from the
// ring pool (one bump pointer shared with the host's allocator), within the queue's
// max_capacity.  Positions stay absolute (entry pos lives at off + (pos & mask)), so
// unacked windows, requeues and store rows keep their queue offsets.
template <bool BL = false>
DEV void plan_queue(const DS& d, u32 q, u64 cnt);
// copy every moved (grown) ring's live entries to its new place, by the nt threads of a block
DEV void copy_moved_rings(const DS& d, u32 nm, u32 tid, u32 nt) {
  for (u32 m = 0; m < nm; ++m) {
    const RingMove mv = d.moves[m];
    for (u64 pos = mv.head + tid; pos < mv.tail; pos += nt)
      d.ring[mv.new_off + (pos & mv.new_mask)] = d.ring[mv.old_off + (pos & mv.old_mask)];
  }
}

template <bool BL>
DEV void ring_plan_one(const DS& d, u32 src, u32 i, u32 n) {
  const u32* kk = d.pair_k[src];
  const u32 rb = d.rank_bits;
  const u32 q = kk[i] >> rb;
  if (i + 1 < n && (kk[i + 1] >> rb) == q) return;   // not the queue's last pair
  plan_queue<BL>(d, q, (u64)(i - d.q_first[q]) + 1);
}
// queue q takes cnt entries this step: record its tail before the enqueue, grow its ring
template <bool BL>
DEV void plan_queue(const DS& d, u32 q, u64 cnt) {
  const u64 head = d.q_head[q], tail = d.q_tail[q];
  d.q_enq_tail[q] = tail;
  if (d.limits) {   // kernel-uniform: a reject-publish queue takes no more than its room (enq_store)
    const u32 ql = d.q_limit[q];
    if (ql_reject(ql)) {
      const u64 depth = tail - head, len = ql_len(ql);
      const u64 room = len > depth ? len - depth : 0;
      if (cnt > room) cnt = room;
      if (BL) {   // and no more than pass its byte rule (K_q): no ring grows for pairs it will refuse
        if (d.q_blimit[q] && cnt > d.q_broom[q]) cnt = d.q_broom[q];
      }
    }
  }
  const u64 mask = d.q_ring_mask[q], cap = mask + 1;
  const u64 need = tail - head + cnt;
  if (need <= cap) return;
  const u64 limit = d.q_max_cap[q] ? d.q_max_cap[q] : d.ring_pool;
  u64 want = cap;
  while (want < 2 * need && want * 2 <= limit) want *= 2;
  if (want <= cap) return;                            // at max_capacity: the overflow drops (nack)
  unsigned long long* top = (unsigned long long*)d.ring_top;
  u64 off = __hip_atomic_load(top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (true) {
    if (off + want > d.ring_pool) return;            // pool exhausted: drops (nack)
    u64 prev = atomicCAS(top, off, off + want);
    if (prev == off) break;
    off = prev;
  }
  RingMove mv;
  mv.q = q; mv.pad = 0;
  mv.old_off = d.q_ring_off[q]; mv.old_mask = mask;
  mv.new_off = off; mv.new_mask = want - 1;
  mv.head = head; mv.tail = tail;
  const u32 mi = atomicAdd(&d.tot[TS_NMOVE], 1u);
  d.moves[mi] = mv;                                  // mi < q_max: one move per queue
  d.q_ring_off[q] = off;
  d.q_ring_mask[q] = want - 1;
  const u32 gi = atomicAdd(&d.ctr->n_grow, 1u);      // the host reclaims the old ring
  if (gi < GROW_MAX) d.grow_h[gi] = mv;
  __threadfence();   // the move is visible to the last block of k_ring_plan (which copies)
}

// the last (occupied) block to finish copies every moved ring's live entries (fused
// k_ring_moves: growth is rare, so one block does it and the common step saves a launch)
// Grid-stride over the pairs with a capped grid (the graph's grid is sized for pair_max;
// a block per 256 pairs of the capacity would mostly launch waves with nothing to do)
template <bool BL>
__global__ __launch_bounds__(256) void k_ring_plan(DS d, u32 src) {
  __shared__ u32 s_last;
  const u32 n = d.tot[TS_PAIR_N];
  u32 nb = (n + 255) / 256;
  if (nb > gridDim.x) nb = gridDim.x;   // blocks taking part
  if (blockIdx.x >= nb) return;
  for (u32 i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) ring_plan_one<BL>(d, src, i, n);
  // a thread that planned a ring move fenced it itself (rare); the common step only waits
  // for its own stores before the ticket (no L2 writeback per block)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(&d.tot[TS_RP_TICKET], 1u) == nb - 1;
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (threadIdx.x == 0) d.tot[TS_RP_TICKET] = 0;
  copy_moved_rings(d, d.tot[TS_NMOVE], threadIdx.x, 256);
}

// x-max-length-bytes, reject-publish (DS.blimits): K_q of the step for every queue that has pairs
// and such a limit -- how many of its pairs, in sort order, pass "ready bytes + the body sizes of
// the queue's earlier pairs of the step < B".  The rule is monotone, so the count is a prefix.
// Waves stride over the sorted pairs; a lane that holds the first pair of such a queue names it,
// and the whole wave then walks that queue's pairs 64 at a time with a prefix scan of their
// body sizes, up to the first pair that fails.  Runs behind the sort, ahead of k_ring_plan and
// k_enqueue, which read K_q (q_broom); q_bytes is what the last step's k_dequeue (and a
// Basic.Get between steps) left.
__global__ __launch_bounds__(256) void k_byte_room(DS d, u32 src) {
  const u32 n = d.tot[TS_PAIR_N];
  const u32* kk = d.pair_k[src];
  const u32* vv = d.pair_v[src];
  const u32 rb = d.rank_bits, lane = lane_id();
  const u32 wv = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  for (u32 b = wv * 64; b < n; b += nw * 64) {   // (wave-uniform)
    const u32 i = b + lane;
    u32 q = INVALID;
    bool first = false;
    if (i < n) {
      q = kk[i] >> rb;
      first = i == 0 || (kk[i - 1] >> rb) != q;
    }
    bool mine = false;
    if (first && q < d.q_max) mine = ql_reject(d.q_limit[q]) && d.q_blimit[q] != 0;
    u64 todo = __ballot(mine);
    while (todo) {
      const u32 l0 = (u32)__ffsll((unsigned long long)todo) - 1u;
      todo &= todo - 1;
      const u32 qq = (u32)__shfl((int)q, l0, 64);
      const u32 i0 = b + l0;
      const u64 B = d.q_blimit[qq] - 1;
      u64 y = d.q_bytes[qq];   // Y + the sizes of the pairs walked so far
      u32 k = 0;
      for (u32 j0 = i0; j0 < n; j0 += 64) {
        const u32 j = j0 + lane;
        const bool in = j < n && (kk[j] >> rb) == qq;
        const u64 sz = in ? d.pubs[vv[j]].body_size : 0u;
        const u64 incl = wave_incl_scan64(sz);
        const u64 inm = __ballot(in);
        // the queue's pairs are contiguous: `in` is a prefix of the lanes, and so is `pass` within it
        const u32 nin = (u32)__popcll(inm);
        const u32 np = (u32)__popcll(__ballot(in && y + (incl - sz) < B));
        k += np;
        if (np < 64u || nin < 64u) break;
        y += shfl64(incl, 63);
      }
      if (lane == 0) d.q_broom[qq] = k;
    }
  }
}

// BL: the bytes of the accepted pairs join q_bytes, one atomic per (wave, queue) run -- the pairs
// are sorted by queue, so a queue's lanes are contiguous
template <bool BL>
__global__ void k_enqueue(DS d, u32 src) {
  const u32 n = d.tot[TS_PAIR_N];
  const u32 stride = gridDim.x * blockDim.x;
  // whole waves iterate together (the wave collectives below need every lane)
  for (u32 b = blockIdx.x * blockDim.x; b < n; b += stride) {
    const u32 i = b + threadIdx.x;
    PersistRec pr;
    pr.msg = INVALID;
    bool limited = false;
    u32 drop = i < n ? enqueue_one<BL>(d, src, i, n, &pr, &limited) : INVALID;
    if (BL) {
      const u32 lane = lane_id();
      u32 q = INVALID;
      u64 sz = 0;
      if (i < n) {
        q = d.pair_k[src][i] >> d.rank_bits;
        const u32 msg = d.pubs[d.pair_v[src][i]].msg;
        if (drop == INVALID && msg != INVALID) sz = d.msgs[msg].body_len;   // stored (exact under any cut)
      }
      const u64 incl = wave_incl_scan64(sz);
      const u32 qprev = (u32)__shfl_up((int)q, 1, 64), qnext = (u32)__shfl_down((int)q, 1, 64);
      const bool head = lane == 0 || qprev != q, last = lane == 63 || qnext != q;
      const u64 heads = __ballot(head);
      // the run's first lane: the highest head at or below this lane
      const u32 l0 = 63u - (u32)__clzll((unsigned long long)(heads & (lanemask_lt() | (1ull << lane))));
      const u64 before = shfl64(incl - sz, l0);
      if (last && q != INVALID && incl != before)
        atomicAdd((unsigned long long*)&d.q_bytes[q], (unsigned long long)(incl - before));
    }
    enqueue_done(d, drop, limited, pr);
  }
}

// ---- single-pass sort (queue | rank key <= 11 bits) with the enqueue fused: k_ring_plan
// and k_enqueue fold into the sort's two kernels.  The histogram's last block knows every
// queue's pair count (its digit range) and plans the rings; the scatter knows every pair's
// sorted position -- its rank in its queue -- and writes the ring entry itself, so the
// sorted pair arrays are never materialised.  Two launches a step instead of four.
DEV void plan_rings_block(const DS& d, const u32* hscan, u32 n, u32 D, u32 tid, u32 nt) {
  const u32 rb = d.rank_bits;
  for (u32 q = tid; q < d.q_max && (q << rb) < D; q += nt) {
    // the digit starts (row 0 of hscan) were stored by this block: agent-scope loads
    const u32 first = __hip_atomic_load(&hscan[q << rb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u32 nx = ((q + 1) << rb) < D
                       ? __hip_atomic_load(&hscan[(q + 1) << rb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                       : n;
    if (nx > first) plan_queue(d, q, nx - first);
  }
  __syncthreads();
  const u32 nm = __hip_atomic_load(&d.tot[TS_NMOVE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!nm) return;   // (block-uniform) rings that grew: copy their live entries over
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  copy_moved_rings(d, nm, tid, nt);
}

template <int DB>
__global__ __launch_bounds__(RsNt<DB>::v) void k_rs_hist_plan(DS d, const u32* keys, const u32* np, u32* hist,
                                                             u32* hscan, u32* ticket, u32 ntiles) {
  const u32 n = *np;
  if (n == 0) return;   // no pairs (T == 0): nothing to plan (the queues' tails stay)
  if (!rs_hist_tiles<DB>(keys, n, 0u, hist, hscan, ticket, ntiles)) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  plan_rings_block(d, hscan, n, 1u << DB, threadIdx.x, RsNt<DB>::v);
}

template <int DB>
__global__ __launch_bounds__(256) void k_rs_scatter_enq(DS d, const u32* kin, const u32* vin, const u32* np,
                                                       const u32* hscan) {
  constexpr u32 D = 1u << DB, CH = SORT_TILE / 256;   // CH items per lane
  __shared__ u32 wc[4][D];
  const u32 tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const u32 n = *np, rb = d.rank_bits;
  const u64 lt = lanemask_lt();
  for (u32 t = blockIdx.x; t * SORT_TILE < n; t += gridDim.x) {   // tile-stride (capped grid)
    const u32 base = t * SORT_TILE;
    __syncthreads();
    for (u32 i = tid; i < 4 * D; i += 256) ((u32*)wc)[i] = 0;
    __syncthreads();
    const u32 wbase = base + w * (SORT_TILE / 4);
    // the lane's CH pairs loaded at once, and kept: the rank pass and the enqueue reuse them
    // (was: each of the CH rounds re-read its pair, then walked its queue's state -- ~3
    // dependent memory trips a round, CH rounds in series: the kernel's 12-13 us floor)
    u32 key[CH], val[CH];
    u64 pe[CH];
#pragma unroll
    for (u32 c = 0; c < CH; ++c) {
      const u32 i = wbase + c * 64 + lane;
      key[c] = i < n ? kin[i] : 0u;
      val[c] = i < n ? vin[i] : 0u;
    }
#pragma unroll
    for (u32 c = 0; c < CH; ++c) {   // per-wave digit counts
      const bool valid = wbase + c * 64 + lane < n;
      const u32 dg = key[c] & (D - 1);
      const u64 peers = pe[c] = digit_peers<DB>(dg, valid);
      if (valid && ((peers & lt) == 0)) wc[w][dg] += __popcll(peers);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    for (u32 dg = tid; dg < D; dg += 256) {
      u32 run = hscan[t * D + dg];
      for (u32 ww = 0; ww < 4; ++ww) { const u32 x = wc[ww][dg]; wc[ww][dg] = run; run += x; }
    }
    __syncthreads();
    // every pair's position in digit order (LDS only), then every load the enqueue needs --
    // its queue's first pair / next digit start, the publish, the queue's ring state -- issued
    // together for the lane's CH pairs, then the ring stores
    u32 pos[CH];
#pragma unroll
    for (u32 c = 0; c < CH; ++c) {
      const bool valid = wbase + c * 64 + lane < n;
      const u32 dg = key[c] & (D - 1);
      const u32 basepos = ((volatile u32*)wc[w])[dg];
      pos[c] = basepos + __popcll(pe[c] & lt);
      __builtin_amdgcn_wave_barrier();
      if (valid && ((pe[c] & lt) == 0)) ((volatile u32*)wc[w])[dg] = basepos + __popcll(pe[c]);
      __builtin_amdgcn_wave_barrier();
    }
    EnqLoad el[CH];
    u32 first[CH], nx[CH];
#pragma unroll
    for (u32 c = 0; c < CH; ++c) {
      const bool valid = wbase + c * 64 + lane < n;
      const u32 q = key[c] >> rb;
      first[c] = valid ? hscan[q << rb] : 0u;
      nx[c] = valid ? (((q + 1) << rb) < D ? hscan[(q + 1) << rb] : n) : 0u;
      el[c] = valid ? enq_load(d, q, val[c]) : EnqLoad{};
    }
#pragma unroll
    for (u32 c = 0; c < CH; ++c) {
      const bool valid = wbase + c * 64 + lane < n;
      PersistRec pr;
      pr.msg = INVALID;
      u32 drop = INVALID;
      bool limited = false;
      if (valid) drop = enq_store(d, el[c], key[c] >> rb, pos[c] - first[c], pos[c] + 1 == nx[c], &pr, &limited);
      enqueue_done(d, drop, limited, pr);
    }
  }
}

// a persistent message changed state in a durable queue: record it for the store
// (kind 0 consumed/acked, 1 expired, 2 dropped, 3 delivered awaiting ack, 4 requeued)
DEV bool wants_record(const DS& d, u32 msg, u32 q, bool valid) {
  return d.persist && valid && msg != INVALID && d.q_durable[q] && (d.msgs[msg].flags & MF_PERSIST);
}
DEV void consumed_rec_at(const DS& d, u32 msg, u32 q, u64 qpos, u32 kind, u32 k) {
  ConsumedRec r;
  r.msg_id = (i64)d.msgs[msg].msg_id;
  r.qpos = qpos;
  r.q = q;
  r.kind = kind;
  r.pad[0] = r.pad[1] = 0;
  d.crec[k] = r;
}
// X3: a shadow message left its queue (consumed, expired, dropped): ack it at the owner
DEV void link_consumed(const DS& d, u32 msg, u32 q, u32 kind, bool valid) {
  if (d.links && valid && msg != INVALID && kind <= 2u) {
    const u32 ow = d.q_link_owner[q];
    if (ow) {
      const u32 k = atomicAdd(&d.lk_cnt[ow - 1], 1u);
      if (k < d.lk_cap) {
        AckRec a;
        a.tq = q;
        a.pad = 0;
        a.xid = d.msgs[msg].msg_id;
        d.lk_send[(u64)(ow - 1) * d.lk_cap + k] = a;
      }
    }
  }
}
DEV void wave_consumed(const DS& d, u32 msg, u32 q, u64 qpos, u32 kind, bool valid) {
  link_consumed(d, msg, q, kind, valid);
  if (!d.persist) return;
  bool want = wants_record(d, msg, q, valid);
  u32 k = wave_reserve(&d.ctr->n_consumed, want);
  if (want && k < d.persist_max) consumed_rec_at(d, msg, q, qpos, kind, k);
}

// ---- dead-lettering (DS.dlx): the dead list.  k_dequeue's walks reserve what they can get
// (reserve_upto: exact, one wave per queue contends); k_chan_advance reserves a 256-tag chunk's
// rejects all or nothing.  The count never passes dead_max and granted ranges never overlap.
// k_dead_pack, the only reader, runs in the next step, behind every writer on the routing stream
DEV u32 dead_reserve_all(const DS& d, u32 n) {
  u32 cur = __hip_atomic_load(&d.dl->dead_n[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (true) {
    if (cur + n > d.dl->dead_max) return INVALID;
    const u32 prev = atomicCAS(&d.dl->dead_n[0], cur, cur + n);
    if (prev == cur) return cur;
    cur = prev;
  }
}
DEV void dead_put(const DS& d, u32 k, u32 step, u32 msg, u32 q, u64 qpos, u32 reason, u32 xs, u32 ch, u64 tag) {
  // (field by field: a 40-byte store would hold ten registers at once in k_chan_advance)
  volatile DeadItem* it = d.dl->dead + k;
  it->msg = msg; it->q = q; it->qpos = qpos; it->step = step; it->reason = reason;
  it->ch = ch; it->xs = xs; it->tag = tag;
}
// One wave, at the head of queue q whose q_dlx word is dx (not 0): the wave's first n lanes hold
// entries (msg at position idx, ring expiry exp) that leave the queue expired or trimmed.
// Purged entries (expiry 1, Queue.Purge's mark) are released and never dead-lettered; the
// others join the dead list in place of their release, as far as it has room.  Returns how
// many of the n entries left (all of them, or those before the first the list had no room
// for: the walk stops there and the next steps go on); the caller writes their consumed
// records and moves the head
DEV u32 dead_leave(const DS& d, u32 dx, u32 step, u32 msg, i64 exp, u32 q, u64 idx, u32 reason, u32 n) {
  const u32 lane = lane_id();
  const bool dead = lane < n && exp != 1 && msg != INVALID;
  const u64 dm = __ballot(dead);
  const u32 want = (u32)__popcll(dm);
  if (dx == 1u) {   // the exchange does not exist (now): lost, like a publish to no queue
    wave_release(d, msg, lane < n);
    if (lane == 0 && want) atomicAdd(&d.ctr->n_dl_unrouted, want);
    return n;
  }
  u32 g = 0, b = 0;
  if (lane == 0 && want) g = reserve_upto(&d.dl->dead_n[0], want, d.dl->dead_max, &b);
  g = (u32)__shfl((int)g, 0, 64);
  b = (u32)__shfl((int)b, 0, 64);
  const u32 rank = (u32)__popcll(dm & lanemask_lt());
  if (dead && rank < g) dead_put(d, b + rank, step, msg, q, idx, reason, dx - 2u, 0u, 0ull);
  if (g < want) {   // the lane of the first entry without room: nothing from it on leaves
    const u64 first = __ballot(dead && rank == g);
    n = (u32)__ffsll((unsigned long long)first) - 1u;
  }
  wave_release(d, msg, lane < n && !dead);
  if (lane == 0 && g) atomicAdd(reason == DL_EXPIRED ? &d.ctr->n_dl_expired : &d.ctr->n_dl_maxlen, g);
  return n;
}


// ============================================================================ K9 window advance
// one block (4 waves) per dirty channel: resolve marks, release/requeue, advance the
// window head over the contiguous run of finished slots, 256 slots per iteration
#define MS_MAX 256   // multiple settles per channel per step resolved exactly (more: folded)
struct MsLds {
  u64 up[MS_MAX + 1];   // (+ 1: the fold of the settles past MS_MAX)
  u32 rq[MS_MAX + 1];
  u32 wc[4];
  u32 rc[4];     // store records per wave of the current chunk
  u32 rbase;     // their block reservation (INVALID: budget exhausted)
  u32 dc[4];     // (DS.dlx) dead-list items per wave of the current chunk
  u32 dbase;     // their block reservation (INVALID: the list is full)
  u32 n, nb;
  unsigned long long ovf_a, ovf_r, ovf_d;
};
template <bool DLX>
DEV void chan_advance_one(const DS& d, u32 ch, u32 tid, u32 lane, u32 w, u32* s_first, u32* s_done, MsLds& ms);
template <bool DLX>
__global__ __launch_bounds__(256) void k_chan_advance(DS d) {
  __shared__ u32 s_first[4];
  __shared__ u32 s_done[4];
  __shared__ MsLds ms;
  const u32 tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const u32 nd = *d.n_dirty;
  for (u32 wv = blockIdx.x; wv < nd; wv += gridDim.x) chan_advance_one<DLX>(d, d.dirty_list[wv], tid, lane, w, s_first,
                                                                        s_done, ms);
}

// the channel's multiple settles of this step (ack indices [lo, hi]) in wire order, reduced
// to record-breaking uptos: ms.up[0..nb) increasing, the first one >= t decides tag t
// (ms.rq: 0 ack, 1 requeue, 2 -- DS.dlx only -- rejected without requeue)
template <bool DLX>
DEV void collect_settles(const DS& d, u32 ch, u32 tid, u32 lane, u32 w, MsLds& ms) {
  const u32 lo = d.ch_mlo[ch], hi = d.ch_mhi[ch];
  if (tid == 0) { ms.n = 0; ms.nb = 0; ms.ovf_a = 0; ms.ovf_r = 0; ms.ovf_d = 0; }
  __syncthreads();
  if (lo == INVALID) return;   // block-uniform
  for (u32 base = lo; base <= hi; base += 256) {
    const u32 i = base + tid;
    bool take = false;
    Ack a;
    a.tag = 0; a.kind = 0; a.requeue = 0;
    if (i <= hi) {
      a = d.acks[i];
      take = a.chslot == ch && a.multiple;
    }
    const u32 rq = a.kind != CK_ACK ? (a.requeue ? 1u : (DLX ? 2u : 0u)) : 0u;
    const u64 m = __ballot(take);
    if (lane == 0) ms.wc[w] = (u32)__popcll(m);
    __syncthreads();
    u32 pos = ms.n + (u32)__popcll(m & lanemask_lt());
    for (u32 k = 0; k < w; ++k) pos += ms.wc[k];
    if (take) {
      if (pos < MS_MAX) { ms.up[pos] = a.tag; ms.rq[pos] = rq; }
      else atomicMax(rq == 1u ? &ms.ovf_r : ((DLX && rq) ? &ms.ovf_d : &ms.ovf_a), (unsigned long long)a.tag);
    }
    __syncthreads();
    if (tid == 0) ms.n += ms.wc[0] + ms.wc[1] + ms.wc[2] + ms.wc[3];
    __syncthreads();
  }
  if (tid == 0) {
    const u32 n = ms.n < MS_MAX ? ms.n : MS_MAX;
    u64 top = 0;
    u32 nb = 0;
    for (u32 k = 0; k < n; ++k)
      if (ms.up[k] > top) { ms.up[nb] = ms.up[k]; ms.rq[nb] = ms.rq[k]; ++nb; top = ms.up[k]; }
    // past MS_MAX: the largest cover with its kind, appended (equal covers: ack, then requeue)
    const u64 oa = ms.ovf_a, orq = ms.ovf_r, od = DLX ? ms.ovf_d : 0ull;
    const u64 om = oa > orq ? (oa > od ? oa : od) : (orq > od ? orq : od);
    if (om > top) { ms.up[nb] = om; ms.rq[nb] = oa == om ? 0u : (orq == om ? 1u : 2u); ++nb; }
    ms.nb = nb;
    d.ch_mlo[ch] = INVALID;
    d.ch_mhi[ch] = 0;
  }
  __syncthreads();
}

// k_chan_advance's share of a step's consumed-store records: persist_max minus what the
// later producers can take (deliveries <= deliv_max in k_dv_write / k_post, the durable
// TTL skip <= persist_max / 4 in k_dequeue); the engine sizes persist_max so this is
// >= deliv_max / 2.  Reserved per 256-slot chunk, never past the budget (CAS).
DEV u32 ca_reserve(const DS& d, u32 n) {
  const u32 lim = d.persist_max - d.deliv_max - (d.persist_max >> 2) - 64u;
  u32 cur = *(volatile u32*)&d.ctr->n_consumed;
  while (true) {
    if (cur + n > lim) return INVALID;
    const u32 prev = atomicCAS(&d.ctr->n_consumed, cur, cur + n);
    if (prev == cur) return cur;
    cur = prev;
  }
}

template <bool DLX>
DEV void chan_advance_one(const DS& d, u32 ch, u32 tid, u32 lane, u32 w, u32* s_first, u32* s_done, MsLds& ms) {
  collect_settles<DLX>(d, ch, tid, lane, w, ms);
  const u32 nb = ms.nb;
  const u64 head = d.ch_uhead[ch], nt = d.ch_next_tag[ch];
  const u64 aup = d.ch_ack_upto[ch], rup = d.ch_req_upto[ch];
  const u64 dup = DLX ? d.dl->ch_dead_upto[ch] : 0ull;
  USlot* win = d.uwin + (u64)ch * (d.ucap_mask + 1);
  bool contiguous = true;
  bool deferred = false;   // block-uniform: the record budget ran out at some chunk
  u64 newhead = head;
  u32 manual_done = 0;
  for (u64 t0 = head; t0 < nt; t0 += 256) {
    const u64 t = t0 + tid;
    const bool valid = t < nt;
    u32 st = US_FREE;
    USlot u;
    u.state = US_FREE; u.msg = INVALID; u.q = 0; u.cons = 0; u.qpos = 0; u.expire_ms = 0;
    if (valid) {
      u = win[(t - 1) & d.ucap_mask];
      st = u.state;
      if (st == US_PENDING) {   // host marks (between steps) first, then this step's settles
        if (t <= aup) st = US_ACKED;
        else if (t <= rup) st = US_REQUEUE;
        else if (DLX && t <= dup) st = US_DEAD;
        else
          for (u32 k = 0; k < nb; ++k)
            if (t <= ms.up[k]) { st = ms.rq[k] == 1u ? US_REQUEUE : ((DLX && ms.rq[k]) ? US_DEAD : US_ACKED); break; }
      }
    }
    bool acked = valid && st == US_ACKED;
    const bool req = valid && st == US_REQUEUE;
    // DS.dlx: a rejected entry whose queue has a dead-letter exchange joins the dead list in
    // place of its release (its record is the ack's); on any other queue it is an ack
    bool dead = false, unrouted = false;
    if (DLX) {
      if (valid && st == US_DEAD) {
        const u32 dxs = u.q < d.q_max ? d.dl->q_dlx[u.q] : 0u;
        dead = dxs >= 2u;
        unrouted = dxs == 1u;
        acked = !dead;
      }
      const u64 dmk = __ballot(dead);
      if (lane == 0) ms.dc[w] = (u32)__popcll(dmk);
      __syncthreads();
      if (tid == 0) {
        const u32 tot = ms.dc[0] + ms.dc[1] + ms.dc[2] + ms.dc[3];
        ms.dbase = deferred ? INVALID : (tot ? dead_reserve_all(d, tot) : 0u);
      }
      __syncthreads();
      if (ms.dbase == INVALID) deferred = true;   // the list is full: the marks stay, like past the record budget
    }
    // store records of this chunk, reserved for the whole block within the step's budget.
    // Past the budget the channel keeps its decided marks (ACKED / REQUEUE slot states,
    // which the next step resolves first) and stays dirty (a burst of settles
    // of durable persistent messages must not overflow persist_max and stop the broker)
    u32 rec_k = INVALID;
    const bool want_rec = wants_record(d, u.msg, u.q, acked || req || dead);
    if (d.persist) {   // kernel-uniform
      const u64 rm = __ballot(want_rec);
      if (lane == 0) ms.rc[w] = (u32)__popcll(rm);
      __syncthreads();
      if (tid == 0) {
        const u32 tot = ms.rc[0] + ms.rc[1] + ms.rc[2] + ms.rc[3];
        ms.rbase = deferred ? INVALID : (tot ? ca_reserve(d, tot) : 0u);
      }
      __syncthreads();
      if (ms.rbase == INVALID && !deferred) {
        deferred = true;
        if (DLX) {   // the chunk's dead-list reservation stays behind as holes (k_dead_pack skips them)
          const u64 dmk = __ballot(dead);
          u32 k = ms.dbase + (u32)__popcll(dmk & lanemask_lt());
          for (u32 j = 0; j < w; ++j) k += ms.dc[j];
          if (dead) dead_put(d, k, (u32)d.in->step, INVALID, u.q, u.qpos, DL_REJECTED, 0u, ch, t);
        }
      }
      if (!deferred) {
        rec_k = ms.rbase + (u32)__popcll(rm & lanemask_lt());
        for (u32 k = 0; k < w; ++k) rec_k += ms.rc[k];
      }
    }
    if (deferred) {   // block-uniform
      if (valid && (st == US_ACKED || st == US_REQUEUE || st == US_DEAD) && st != u.state) win[(t - 1) & d.ucap_mask].state = st;
      contiguous = false;
      continue;
    }
    if (DLX) {
      const u64 dmk = __ballot(dead);
      u32 k = ms.dbase + (u32)__popcll(dmk & lanemask_lt());
      for (u32 j = 0; j < w; ++j) k += ms.dc[j];
      if (dead) dead_put(d, k, (u32)d.in->step, u.msg, u.q, u.qpos, DL_REJECTED, d.dl->q_dlx[u.q] - 2u, ch, t);
      const u32 nun = (u32)__popcll(__ballot(unrouted));
      if (lane == 0 && dmk) atomicAdd(&d.ctr->n_dl_rejected, (u32)__popcll(dmk));
      if (lane == 0 && nun) atomicAdd(&d.ctr->n_dl_unrouted, nun);
    }
    // requeue list (one reservation per wave)
    u32 rtot;
    u32 ri = wave_reserve(d.req_n, req, &rtot);
    bool req_ok = req && ri < d.req_max;
    if (req_ok) {
      ReqItem r;
      r.q = u.q; r.msg = u.msg; r.qpos = u.qpos; r.expire_ms = u.expire_ms;
      d.req[ri] = r;
    }
    wave_add_u32(d.req_q_n, u.q, 1u, req_ok);
    link_consumed(d, u.msg, u.q, (acked || dead) ? 0u : (req_ok ? 4u : 2u), acked || req || dead);
    if (want_rec) consumed_rec_at(d, u.msg, u.q, u.qpos, (acked || dead) ? 0u : (req_ok ? 4u : 2u), rec_k);
    wave_release(d, u.msg, acked || (req && !req_ok));
    wave_sub_u32(d.cons_unacked, u.cons, 1u, acked || req || dead);
    manual_done += __popcll(__ballot(acked || req || dead));
    if (lane == 0 && rtot) atomicAdd(&d.ctr->n_requeue, rtot);
    if (acked || req || dead) st = US_DONE;
    if (valid && st != u.state) win[(t - 1) & d.ucap_mask].state = st;
    if (contiguous) {   // block-uniform
      // both ballots wave-wide (a ballot inside the lane-0 branch would see one lane)
      const u64 notdone = __ballot(valid && st != US_DONE);
      const u32 nvalid = (u32)__popcll(__ballot(valid));
      if (lane == 0) {
        s_first[w] = notdone ? (u32)(__ffsll((unsigned long long)notdone) - 1) : 64u;
        s_done[w] = nvalid;
      }
      __syncthreads();
      u32 adv = 0;
      bool stop = false;
      for (u32 k = 0; k < 4 && !stop; ++k) {
        if (s_first[k] < 64) { adv += s_first[k]; stop = true; }
        else adv += s_done[k];
      }
      newhead += adv;
      if (stop) contiguous = false;
      __syncthreads();
    }
  }
  if (lane == 0 && manual_done) atomicSub(&d.ch_unacked[ch], manual_done);
  if (tid == 0) {
    atomicSub(&d.ch_win[ch], (u32)(newhead - head));
    d.ch_uhead[ch] = newhead;
    if (deferred) d.def_list[atomicAdd(&d.tot[TS_NCADEF], 1u)] = ch;   // stays dirty: k_dequeue re-lists it
    else d.ch_dirty[ch] = 0;
  }
}

// ============================================================================ K8 dequeue
DEV u32 deliver_size(const DS& d, u32 cons, const MsgEnt& m, u32 conn) {
  // a link pseudo-connection ships [ex][rk][props][body] as a restore record (render_deliv)
  if (d.links && d.conn_link[conn]) return align16(m.ex_len + m.rk_len + m.props_len + m.body_len);
  // cons_max = a Basic.GetOk: no consumer tag, a 4-byte message-count instead
  u32 mp = (cons == d.cons_max ? 4 + 4 : 4 + 1 + d.cons_tag_len[cons]) + 8 + 1 + 1 + m.ex_len + 1 + m.rk_len;
  u32 sz = 8 + mp + 8 + 12 + m.props_len;
  u32 fm = d.conn_frame_max[conn];
  u32 fmb = fm ? fm - 8 : 0xffffffffu;
  u32 nb = m.body_len ? (m.body_len - 1) / fmb + 1 : 0;   // (no sum: fmb is 2^32 - 1 for frame-max 0)
  return sz + m.body_len + 8 * nb;
}

// egress by reference: the delivery of message m to connection conn is rendered without its
// body (the host sends those bytes from the publishing step's ingress payload): a body the
// publish decode marked (MsgEnt.href), published at most ref_back steps ago, no shorter than
// ref_min and within one body frame of the connection.  Link pseudo-connections ship
// restore records, never references.  k_dv_write and render_deliv must agree: same inputs
// Returns the body's host address, or 0 (rendered whole).  A body in the host spill ring
// is referenced there whatever its age: a freed ring byte is reused only SPILL_LAG steps
// later (spill_reserve), after every egress that can reference it was written out
DEV u64 deliv_href(const DS& d, const MsgEnt& m, u32 conn) {
  if (d.in->ref_back == 0xffffffffu || m.body_len < d.in->ref_min) return 0;
  if (d.links && d.conn_link[conn]) return 0;
  const u32 fm = d.conn_frame_max[conn];
  if (fm != 0 && m.body_len > fm - 8) return 0;
  if ((m.log_off & (SPILL_BIT | COLD_BIT)) == SPILL_BIT && d.spill_host)
    return d.spill_host + ((m.log_off & ~SPILL_BIT) % d.spill_bytes) + m.body_off;
  if (d.in->ref_back & REF_SPILL_ONLY) return 0;   // (ingress bodies inline this step)
  if (!m.href || (u32)d.in->step - m.pub_step > d.in->ref_back) return 0;
  return m.href;
}

// give back channel reservations for `take` messages not delivered after all
DEV void unreserve(const DS& d, u32 c, u32 take) {
  u32 ch = d.cons_ch[c];
  atomicSub(&d.ch_win[ch], take);
  if (!d.cons_noack[c]) { atomicSub(&d.ch_unacked[ch], take); d.cons_unacked[c] -= take; }
}

// one block per queue: TTL skip (K12, wave 0), credit-limited round-robin split over the
// consumers (thread 0, deterministic consumer order), egress byte budget (block-parallel
// sizes), then one delivery run per granted consumer.  runs_body orders the runs by channel
// and k_dv_write expands them into Deliv records at their final positions, so no sort
// over individual deliveries is needed (QueueEntity.scala:318-393, FrameStage.scala:380-406).
#define REQ_BLK 1024
DEV void requeue_compact(const DS& d);
template <bool BL>
DEV void requeue_queue(const DS& d, u32 q, u64* kpos, u32* kidx, u32* cnt_p);
// one queue's share of a spill (4 waves): every queued message past the first `hot` entries
// (of a queue with consumers) whose slot lies below log position `lim` -- its body to the
// host spill ring, the message switched to it; at most `budget` bytes per launch across
// all queues (budget 0: no limit)
DEV bool spill_reserve(const DS& d, u32 sz, u64* pos);
DEV void spill_queue(const DS& d, u32 q, u64 lim, u32 hot, u32 budget, u64* moved) {
  const u32 lane = lane_id(), w = threadIdx.x >> 6;
  if (!d.q_active[q]) return;
  // (agent scope: in k_dequeue this block's requeue may just have moved the head)
  const u64 head = __hip_atomic_load(&d.q_head[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const u64 tail = d.q_tail[q], mask = d.q_ring_mask[q];
  const Desc* ring = d.ring + d.q_ring_off[q];
  const u64 skip = d.q_cons_n[q] ? hot : 0;
  // Resume at the queue's cursor: every entry before it is tiered already, so a deep
  // backlog is not walked again each step (it was: ~10 ms per step for a 90 K-entry queue
  // of spilled and cold bodies, profiles/r5_coldprof/).  A queue's log offsets grow along
  // the queue (requeues only go lower), so the first entry at or past `lim` ends the walk.
  __shared__ unsigned long long s_open;
  if (threadIdx.x == 0) s_open = ~0ull;
  __syncthreads();
  const u64 start0 = head + skip;
  u64 cur = d.q_spill_cur[q];
  if (cur < start0 || cur > tail) cur = start0;   // (the head passed it, or the slot was reset)
  u64 open = ~0ull;   // this wave's first entry left in the log
  for (u64 i = cur + w; i < tail; i += 4) {
    const u32 msg = ring[i & mask].msg;
    if (msg == INVALID || msg >= d.msg_max) continue;
    MsgEnt& m = d.msgs[msg];
    const u64 lo = __hip_atomic_load(&m.log_off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lo & (SPILL_BIT | COLD_BIT)) continue;
    if (lo >= lim) { open = i; break; }
    const u32 sz = m.slot_bytes;
    u64 pos = 0;
    u32 ok = 0;
    if (lane == 0) {
      ok = (!budget || atomicAdd(&d.tot[TS_SPILL_USED], sz) + sz <= budget) ? 1u : 0u;
      if (ok) ok = spill_reserve(d, sz, &pos) ? 1u : 0u;
    }
    ok = (u32)__shfl((int)ok, 0);
    if (!ok) { open = i; break; }   // the spill ring is full, or this step's budget is spent
    pos = shfl64(pos, 0);
    wave_copy(d.spill + (pos % d.spill_bytes), d.log + (lo % d.log_bytes), sz);
    __threadfence_system();   // the copy reached host memory before the slot is switched
    if (lane == 0 &&
        atomicCAS((unsigned long long*)&m.log_off, (unsigned long long)lo, (unsigned long long)(SPILL_BIT | pos)) == lo) {
      atomicAdd((unsigned long long*)&d.log_live[(lo / d.log_block) % d.n_log_blocks], (unsigned long long)(-(i64)sz));
      atomicAdd((unsigned long long*)&d.spill_live[(pos / d.log_block) % d.n_spill_blocks], (unsigned long long)sz);
      atomicAdd((unsigned long long*)d.live_bytes, (unsigned long long)(-(i64)sz));
      atomicAdd((unsigned long long*)moved, (unsigned long long)sz);
    }
  }
  if (lane == 0 && open != ~0ull) atomicMin(&s_open, (unsigned long long)open);
  __syncthreads();
  if (threadIdx.x == 0) d.q_spill_cur[q] = s_open == ~0ull ? tail : (u64)s_open;
}

// true: the block wrote runs with plain stores (the ticket before runs_body needs an
// agent-scope release); false: at most q_nruns[q] = 0, stored agent-coherent
// a consumer's dispatch inputs, loaded by the block's other waves while wave 0 walks the
// TTL head (thread 0's credit loop then reads them from LDS: only its atomics stay serial)
struct DqCons { u32 c, ch, ok, noack, pc, glob, unacked; };
// x-max-length, drop-head (DS.limits; wave 0, on every exit of dequeue_queue that stores q_head,
// once the step's final head is fixed): the ready entries above the queue's limit leave from
// the head, oldest first, 64 an iteration like the TTL walk -- after the step's enqueue, requeues,
// TTL walk, Basic.Gets and dispatch, so a consumer with credit still gets what the step brought
// and only what would stay queued is bounded.  A trimmed entry goes the way of an expired one
// (store record kind 1, release); a durable queue on a persisting plane draws on the TTL walk's
// record budget, and the next steps trim what that did not cover.  The entries of the runs
// written this step lie below `head` and are not touched.  q_spill_cur copes with a
// head that passes it (spill_queue restarts at the head); for q_cold_lim the rule is the one at
// DS.q_cold_lim (dp_state.h): a trim without a dead-letter exchange may leave head > q_cold_lim
// until the next step's cold_lim_rescan puts the limit at the first cold entry again, or at ~0.
// Stores q_head[q] if it moved; a dead-letter exchange would take the trimmed entries here.
// BL (x-max-length-bytes): `bytes` are the queue's ready bytes at `head`; the trim also runs while
// they exceed the byte limit B.  An iteration looks at the (up to) 64 entries at the head, their
// body sizes loaded together: with E_i the exclusive prefix of the sizes, entry i leaves iff
// i < depth - L or bytes - E_i > B -- both monotone in i, so the drop count is one ballot.  One
// body larger than B leaves an empty queue.  Stores q_bytes[q], for every queue, limited or not
// (this is where the queue's step ends).
template <bool DLX, bool BL>
DEV void trim_head(const DS& d, u32 q, u64 head, u64 tail, u64 mask, const Desc* ring, u64 bytes) {
  const u32 ql = d.q_limit[q];
  const u32 lane = lane_id();
  if (!ql_set(ql) || ql_reject(ql)) {   // wave-uniform
    if (BL && lane == 0) d.q_bytes[q] = bytes;
    return;
  }
  const u64 len = ql_len(ql);
  u64 bl = 0;   // BL: 0, or B + 1
  if (BL) bl = d.q_blimit[q];
  if (tail - head <= len && !(BL && bl && bytes >= bl)) {
    if (BL && lane == 0) d.q_bytes[q] = bytes;
    return;
  }
  const bool budget = d.persist && d.q_durable[q];
  // DS.dlx, a queue with a dead-letter exchange: as in the TTL walk, the trimmed entries join
  // the dead list as far as it has room, and the trim ends where bodies may be cold
  const u32 dx = DLX ? d.dl->q_dlx[q] : 0u;   // wave-uniform
  const u64 clim = dx ? d.q_cold_lim[q] : ~0ull;
  while ((tail - head > len || (BL && bl && bytes >= bl)) && head < clim) {
    if (budget) {
      u32 ok = 1;
      if (lane == 0) ok = atomicAdd(&d.tot[TS_TTL_BUDGET], 64u) + 64u <= (d.persist_max >> 2);
      if (!__shfl(ok, 0, 64)) break;
    }
    const u64 idx = head + lane;
    Desc ds;
    ds.msg = INVALID; ds.expire_ms = 0; ds.flags = 0;
    u32 n;
    u32 esz = 0;   // BL: the entry's body bytes
    if (!BL) {
      u64 over = tail - head - len;
      if (over > clim - head) over = clim - head;
      n = over < 64 ? (u32)over : 64u;
      if (lane < n) ds = ring[idx & mask];
    } else {
      const u64 over = tail - head > len ? tail - head - len : 0;
      u64 span = tail - head;
      if (span > clim - head) span = clim - head;
      const u32 w = span < 64 ? (u32)span : 64u;   // the entries looked at
      if (w == 0) break;   // (an empty queue holds no bytes)
      if (lane < w) ds = ring[idx & mask];
      if (lane < w && ds.msg != INVALID) esz = d.msgs[ds.msg].body_len;
      const u64 excl = wave_incl_scan64(esz) - esz;
      n = (u32)__popcll(__ballot(lane < w && (lane < over || (bl && bytes - excl >= bl))));
      if (lane >= n) { ds.msg = INVALID; ds.expire_ms = 0; ds.flags = 0; }
    }
    bool full = false;
    if (dx) {
      const u32 left = dead_leave(d, dx, (u32)d.in->step, ds.msg, ds.expire_ms, q, idx, DL_MAXLEN, n);
      full = left < n;
      n = left;
    }
    const bool v = lane < n;
    wave_consumed(d, ds.msg, q, idx, 1u, v);
    if (!dx) wave_release(d, ds.msg, v);
    if (lane == 0 && n) atomicAdd(&d.ctr->n_maxlen_dropped, n);
    if (BL) bytes -= (u64)wave_sum64(v ? (i64)esz : 0);
    head += n;
    if (full) break;
  }
  if (lane == 0) d.q_head[q] = head;
  if (BL && lane == 0) d.q_bytes[q] = bytes;
}
// q_cold_lim once the head has reached it (wave 0 of the queue's block): the first cold entry
// from the head on, ~0 when there is none -- the rule stated at DS.q_cold_lim.  A head that
// stands at the first cold entry costs one look at that entry; a head that passed the limit
// (TTL walk, purge, Basic.Get, trim) or a limit k_cold_in left in front of resident
// entries is found here instead of holding the queue until some later k_cold_scan.
// Returns the limit that holds now.
DEV u64 cold_lim_rescan(const DS& d, u32 q, u64 head, u64 tail, u64 mask, const Desc* ring) {
  const u64 lim = d.q_cold_lim[q];
  if (lim == ~0ull || head < lim) return lim;   // wave-uniform
  const u32 lane = lane_id();
  u64 first = ~0ull;
  for (u64 b = head; b < tail; b += 64) {
    const u64 i = b + lane;
    bool cold = false;
    if (i < tail) {
      const u32 msg = ring[i & mask].msg;
      cold = msg != INVALID && msg < d.msg_max && (d.msgs[msg].log_off & COLD_BIT) != 0;
    }
    const u64 cm = __ballot(cold);
    if (cm) { first = b + (u64)(__ffsll((unsigned long long)cm) - 1); break; }
  }
  if (lane == 0 && first != lim) d.q_cold_lim[q] = first;
  return first;
}
// PRIO (DS.prio): a base slot of a priority queue (q_prio != 0) goes through as a queue without
// consumers or Gets -- requeue, spill, TTL walk as for every lane -- and k_prio_dispatch serves it
template <bool DLX, bool BL, bool PRIO>
DEV bool dequeue_queue(const DS& d) {
  __shared__ u32 g_cons[RUNS_PER_Q];
  __shared__ u32 g_n[RUNS_PER_Q];
  __shared__ DqCons g_ci[RUNS_PER_Q];
  __shared__ u64 s_head;
  __shared__ u32 s_ngr;
  __shared__ unsigned long long s_bytes;
  __shared__ u64 s_qb;   // BL: the queue's ready bytes as the step's walks leave them (wave 0 / thread 0)
  __shared__ u64 kpos[REQ_BLK];
  __shared__ u32 kidx[REQ_BLK];
  __shared__ u32 rq_cnt, rq_last;
  const u32 q = blockIdx.x, tid = threadIdx.x, lane = lane_id();
  if (q == 0 && tid == 0) {   // fused k_reset_dirty (k_chan_advance consumed the list)
    // channels it deferred (store-record budget) start the next step's list
    const u32 nd = d.tot[TS_NCADEF];
    for (u32 k = 0; k < nd; ++k) d.dirty_list[k] = d.def_list[k];
    *d.n_dirty = nd;
    d.tot[TS_NCADEF] = 0;
  }
  // fused k_requeue: requeued deliveries go back in front of their queues' heads before this
  // step's dispatch, in queue-offset order.  Every block takes the ticket (req_n only
  // changes in the compaction, which runs after every block has read it); the last one
  // compacts the unconsumed items
  if (*d.req_n != 0) {
    if (q < d.q_max && d.req_q_n[q] != 0) requeue_queue<BL>(d, q, kpos, kidx, &rq_cnt);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (tid == 0) rq_last = atomicAdd(&d.tot[TS_REQ_TICKET], 1u) == gridDim.x - 1;
    __syncthreads();
    if (rq_last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      if (tid == 0) d.tot[TS_REQ_TICKET] = 0;
      requeue_compact(d);
      __syncthreads();
    }
  }
  if (q >= d.q_max) return false;
  const u32 ndg = d.tot[TS_NDGET] < DGET_MAX ? d.tot[TS_NDGET] : DGET_MAX;   // Basic.Gets decoded this step
  if (!d.q_active[q]) {
    if (tid == 0) {
      __hip_atomic_store(&d.q_nruns[q], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // a Basic.Get staged for a queue deleted since: answered GONE (never left RETRY, which
      // the host would resubmit forever -- or serve from whatever queue reuses the slot)
      const u32 ng = d.in->nget < GET_STEP_MAX ? d.in->nget : GET_STEP_MAX;
      for (u32 i = 0; i < ng; ++i)
        if (d.get_req[i].q == q) d.get_out_h[i] = GetOut{GS_GONE, 0u};
      for (u32 k = 0; k < ndg; ++k)
        if (d.dget[k].q == q) dget_to_host(d, k);
    }
    return false;
  }
  const bool nodisp = (d.in->flags & SF_NODISPATCH) != 0;
  bool pbase = false;   // block-uniform
  if (PRIO) pbase = d.q_prio[q] != 0;
  if (d.in->spill_frac && d.spill_bytes) {   // (kernel-uniform) the step's share of body tiering
    const u64 lim = *d.log_tail + (((u64)d.log_bytes * d.in->spill_frac) >> 16);
    spill_queue(d, q, lim, d.in->spill_hot, d.in->spill_budget, &d.ctr->spill_moved);
    __syncthreads();
  }
  if (nodisp && d.links && d.q_link_owner[q]) {   // a live link shadow: its acks could not travel
    if (tid == 0) {
      __hip_atomic_store(&d.q_nruns[q], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (u32 k = 0; k < ndg; ++k)
        if (d.dget[k].q == q) dget_to_host(d, k);
    }
    return false;
  }
  // agent-scope load: the requeue above (this block's thread 0) may have moved the head
  // after this wave read the line
  u64 head = __hip_atomic_load(&d.q_head[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const u64 tail = d.q_tail[q];
  const u64 mask = d.q_ring_mask[q];
  const Desc* ring = d.ring + d.q_ring_off[q];
  const i64 now = d.in->now_ms;
  if (tid < 64) {   // TTL skip at the head (K12)
    // durable queues: every skipped persistent entry is a store record (ConsumedRec); a
    // purge of a deep queue marks its whole backlog expired, so the skip takes at most a
    // quarter of the step's record buffer (reserved 64 at a time) and the next steps
    // continue it -- the record buffer never overflows (the store would miss deletions)
    const bool budget = d.persist && d.q_durable[q];
    // DS.dlx, a queue with a dead-letter exchange: the expired entries join the dead list
    // (dead_leave) as far as it has room, and the walk ends at the first position whose body
    // may be cold (k_dead_pack could not copy it; k_cold_scan pages the head window back in)
    const u32 dx = DLX ? d.dl->q_dlx[q] : 0u;   // wave-uniform
    const u64 clim0 = d.spill_bytes ? cold_lim_rescan(d, q, head, tail, mask, ring) : ~0ull;
    u64 wend = tail;
    if (dx && clim0 < wend) wend = clim0;
    // BL: the ready bytes before the walk (agent scope, like the head: the requeue above added to them)
    u64 qb = 0;
    if (BL) qb = __hip_atomic_load(&d.q_bytes[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (head < wend) {
      if (budget) {
        u32 ok = 1;
        if (lane == 0) ok = atomicAdd(&d.tot[TS_TTL_BUDGET], 64u) + 64u <= (d.persist_max >> 2);
        if (!__shfl(ok, 0, 64)) break;
      }
      u64 idx = head + lane;
      bool valid = idx < wend;
      Desc ds;
      ds.msg = INVALID; ds.expire_ms = 0; ds.flags = 0;
      if (valid) ds = ring[idx & mask];
      bool exp = valid && ds.expire_ms != 0 && ds.expire_ms <= now;
      u64 live = __ballot(valid && !exp);
      u32 nexp = live ? (__ffsll((unsigned long long)live) - 1) : __popcll(__ballot(valid));
      u32 esz = 0;   // BL: the leaving entry's body bytes (read before its release)
      if (BL) {
        if (lane < nexp && ds.msg != INVALID) esz = d.msgs[ds.msg].body_len;
      }
      bool full = false;
      if (dx) {
        const u32 left = dead_leave(d, dx, (u32)d.in->step, ds.msg, ds.expire_ms, q, idx, DL_EXPIRED, nexp);
        full = left < nexp;
        nexp = left;
      }
      wave_consumed(d, ds.msg, q, idx, 1u, lane < nexp);
      if (!dx) wave_release(d, ds.msg, lane < nexp);
      if (lane == 0 && nexp) atomicAdd(&d.ctr->n_expired, nexp);
      if (BL) qb -= (u64)wave_sum64(lane < nexp ? (i64)esz : 0);
      head += nexp;
      if (live || full) break;
    }
    if (d.spill_bytes) cold_lim_rescan(d, q, head, tail, mask, ring);   // (the walk may have passed it)
    if (lane == 0) { s_head = head; s_bytes = 0; }
    if (BL && lane == 0) s_qb = qb;
  } else if (!nodisp && tid - 64 < RUNS_PER_Q) {   // the consumers' inputs, beside the TTL walk
    const u32 j = tid - 64, mall0 = pbase ? 0u : d.q_cons_n[q];
    if (j < mall0) {
      const u32 c = d.q_cons[d.q_cons_off[q] + (d.q_rr[q] % mall0 + j) % mall0];
      const u32 ch = d.cons_ch[c];
      DqCons ci;
      ci.c = c;
      ci.ch = ch;
      // wblock: the front end's socket backlog for this connection is above its high
      // watermark (host-mapped, written by the IO threads): its messages stay queued in HBM
      // (cons_active 2: staged by a light control section this step -- it takes deliveries
      // from the next step on, behind its Basic.ConsumeOk)
      ci.ok = d.cons_active[c] == 1u && d.ch_flow[ch] && !d.conn_wblock[ch / d.chpc];
      ci.noack = d.cons_noack[c];
      ci.pc = d.ch_prefetch[ch];
      ci.glob = d.ch_global[ch];
      ci.unacked = d.cons_unacked[c];
      g_ci[j] = ci;
    }
  }
  __syncthreads();
  head = s_head;
  // Basic.Get requests of this queue, in request order, ahead of its consumers (the
  // reference's Pull(1) with the channel's next delivery tag, FrameStage.scala:1199-1229):
  // each answer is one run of cnt 1 on the requester's channel (consumer slot cons_max),
  // rendered as GetOk + header + body by k_render; EMPTY / RETRY / WINDOW_FULL go back
  // to the host through the step's host-mapped GetOut (the host initialised them RETRY)
  u32 ngr = 0;
  if ((d.in->nget || ndg) && !pbase) {   // kernel-uniform (pbase: block-uniform)
    if (tid == 0) {
      const u32 ng = d.in->nget < GET_STEP_MAX ? d.in->nget : GET_STEP_MAX;
      const u64 clim = d.q_cold_lim[q];   // a cold head waits for the host's page-in (RETRY)
      u64 h = head;
      u64 gbytes = 0;   // BL: body bytes of the entries the answers take
      // the host-staged requests (their connections were paused: nothing of theirs was
      // decoded this step), then the step's own Basic.Gets in wire order
      for (u32 i = 0; i < ng + ndg; ++i) {
        const bool dev = i >= ng;
        const u32 dk = dev ? i - ng : 0u;
        GetReq rq;
        if (dev) {
          rq.conn = d.dget[dk].conn; rq.chslot = d.dget[dk].chslot; rq.q = d.dget[dk].q; rq.noack = d.dget[dk].noack;
        } else {
          rq = d.get_req[i];
        }
        if (rq.q != q) continue;
        GetOut o;
        o.status = GS_RETRY;
        o.msg_count = 0;
        if (!nodisp && h == tail) {
          o.status = GS_EMPTY;
        } else if (!nodisp && h < clim && ngr < RUNS_PER_Q / 2 && rq.chslot < d.c_max * d.chpc) {
          const u32 ch = rq.chslot;
          const u32 sz = deliver_size(d, d.cons_max, d.msgs[ring[h & mask].msg], ch / d.chpc);
          u32 wb, db;
          if (sz > d.egress_cap / 2) {
            o.status = GS_NO_SPACE;
          } else if (!reserve_upto(&d.ch_win[ch], 1u, d.ucap_mask + 1, &wb)) {
            o.status = GS_WINDOW_FULL;
          } else if (reserve_sat64(d.egress_budget, sz, d.egress_cap) < sz ||
                     !reserve_sat(&d.ctr->n_deliv, 1u, d.deliv_max, &db)) {
            atomicSub(&d.ch_win[ch], 1u);   // step full: the host retries with a later step
          } else {
            if (!rq.noack) { atomicAdd(&d.ch_unacked[ch], 1u); atomicAdd(&d.cons_unacked[d.cons_max], 1u); }
            const u64 left = tail - h - 1;
            Run rn;
            rn.ch = ch;
            rn.cons = left < 0xffffffffull ? (u32)left : 0xffffffffu;
            rn.cnt = 1;
            rn.q = q;
            rn.qpos = h;
            rn.noack = rq.noack ? 1u : 0u;
            rn.flags = RUN_GET;
            d.runs[(u64)q * RUNS_PER_Q + ngr] = rn;
            if (BL) gbytes += d.msgs[ring[h & mask].msg].body_len;
            ++ngr;
            ++h;
            o.status = GS_OK;
            o.msg_count = rn.cons;
          }
        }
        if (!dev) {
          d.get_out_h[i] = o;
        } else if (o.status == GS_EMPTY && reserve_sat64(d.egress_budget, 13, d.egress_cap) == 13) {
          atomicAdd(&d.conn_gempty[rq.conn], 1u);   // Basic.GetEmpty, rendered by render_confirms
          d.conn_gempty_ch[rq.conn] = d.ch_num[rq.chslot];
        } else if (o.status != GS_OK) {
          dget_to_host(d, dk);
        }
      }
      s_head = h;
      s_ngr = ngr;
      if (BL) s_qb -= gbytes;
    }
    __syncthreads();
    head = s_head;
    ngr = s_ngr;
  }
  const u32 mall = pbase ? 0u : d.q_cons_n[q];
  // bodies from q_cold_lim on may be in the cold store: delivered once paged back in
  const u64 dlim = d.q_cold_lim[q] < tail ? d.q_cold_lim[q] : tail;
  const u64 avail = dlim > head ? dlim - head : 0;
  if (mall == 0 || avail == 0 || nodisp) {
    if (tid == 0) { d.q_head[q] = head; d.q_nruns[q] = ngr; }
    // (wave 0: thread 0's store of q_head above is ordered before lane 0's in trim_head)
    if (d.limits && tid < 64) trim_head<DLX, BL>(d, q, head, tail, mask, ring, BL ? s_qb : 0ull);
    return true;
  }
  const u32 m = mall > RUNS_PER_Q - ngr ? RUNS_PER_Q - ngr : mall;
  const u32 r = d.q_rr[q] % mall;
  // (1) counts by credit (the consumers' inputs came in beside the TTL walk: g_ci)
  if (tid == 0) {
    u64 remaining = avail;
    for (u32 j = 0; j < m; ++j) {
      const DqCons ci = g_ci[j];
      u32 c = ci.c;
      g_cons[j] = c;
      g_n[j] = 0;
      if (remaining == 0) continue;
      u32 ch = ci.ch;
      if (!ci.ok) continue;
      u64 share = (remaining + (m - j) - 1) / (m - j);
      u32 want = (u32)(share < d.deliver_cap ? share : d.deliver_cap);
      const u32 dcb = d.in->dcap_bytes;
      if (dcb && want > 1 && !(d.links && d.conn_link[ch / d.chpc])) {   // byte cap (StepIn.dcap_bytes)
        const u32 s0 = deliver_size(d, c, d.msgs[ring[(head + (avail - remaining)) & mask].msg], ch / d.chpc);
        const u32 lim = s0 >= dcb ? 1u : dcb / s0;
        want = want < lim ? want : lim;
      }
      bool noack = ci.noack;
      u32 pc = ci.pc;
      if (!noack && pc && !ci.glob) {
        u32 used = ci.unacked;
        u32 cr = used < pc ? pc - used : 0;
        want = want < cr ? want : cr;
      }
      u32 wb;
      u32 g = reserve_upto(&d.ch_win[ch], want, d.ucap_mask + 1, &wb);
      if (!noack && pc && ci.glob && g) {
        u32 ub;
        u32 g2 = reserve_upto(&d.ch_unacked[ch], g, pc, &ub);
        if (g2 < g) atomicSub(&d.ch_win[ch], g - g2);
        g = g2;
      } else if (!noack && g) {
        atomicAdd(&d.ch_unacked[ch], g);
      }
      if (!noack && g) d.cons_unacked[c] += g;
      g_n[j] = g;
      remaining -= g;
    }
  }
  __syncthreads();
  // (2) egress bytes of every granted entry, block-parallel per consumer run
  {
    u32 mine = 0;
    u64 qp = head;
    for (u32 j = 0; j < m; ++j) {
      const u32 cnt = g_n[j];
      if (!cnt) continue;
      const u32 c = g_cons[j];
      const u32 conn = g_ci[j].ch / d.chpc;
      // four entries a thread per round, their ring loads then their message loads in flight
      // together (a round trip each per entry in series before)
      constexpr u32 U = 4;
      for (u32 k0 = tid; k0 < cnt; k0 += 256 * U) {
        u32 mg[U];
#pragma unroll
        for (u32 u = 0; u < U; ++u) {
          const u32 k = k0 + u * 256;
          mg[u] = k < cnt ? ring[(qp + k) & mask].msg : INVALID;
        }
#pragma unroll
        for (u32 u = 0; u < U; ++u)
          if (mg[u] != INVALID) mine += deliver_size(d, c, d.msgs[mg[u]], conn);
      }
      qp += cnt;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0 && mine) atomicAdd(&s_bytes, (unsigned long long)mine);
  }
  __syncthreads();
  if (tid == 0) {
    const u64 bytes = s_bytes;
    const u64 gb = reserve_sat64(d.egress_budget, bytes, d.egress_cap);
    if (gb < bytes) {
      // egress budget nearly spent: keep the longest prefix of the queue's granted
      // entries (in run order) whose frames fit in what this queue was granted
      u64 left = gb;
      u64 qp = head;
      bool full = false;
      for (u32 j = 0; j < m; ++j) {
        u32 cnt = g_n[j];
        if (!cnt) continue;
        u32 c = g_cons[j];
        u32 conn = d.cons_ch[c] / d.chpc;
        u32 keep = 0;
        while (!full && keep < cnt) {
          u32 sz = deliver_size(d, c, d.msgs[ring[(qp + keep) & mask].msg], conn);
          if (sz > left) { full = true; break; }
          left -= sz;
          ++keep;
        }
        if (keep < cnt) unreserve(d, c, cnt - keep);
        g_n[j] = keep;
        qp += keep;
      }
    }
    // (3) delivery slots (capacity), trimmed from the last run backwards; runs_body
    // rewrites n_deliv with the exact total of the kept runs
    u32 total = 0;
    for (u32 j = 0; j < m; ++j) total += g_n[j];
    u32 db;
    u32 gt = reserve_sat(&d.ctr->n_deliv, total, d.deliv_max, &db);
    u32 excess = total - gt;
    for (int j = (int)m - 1; j >= 0 && excess; --j) {
      u32 take = g_n[j] < excess ? g_n[j] : excess;
      if (!take) continue;
      unreserve(d, g_cons[j], take);
      g_n[j] -= take;
      excess -= take;
    }
    // (4) runs, in round-robin order (after this step's Basic.Get answers)
    u32 nr = ngr;
    u64 qp = head;
    for (u32 j = 0; j < m; ++j) {
      u32 cnt = g_n[j];
      if (!cnt) continue;
      u32 c = g_cons[j];
      Run rn;
      rn.ch = d.cons_ch[c];
      rn.cons = c;
      rn.cnt = cnt;
      rn.q = q;
      rn.qpos = qp;
      rn.noack = d.cons_noack[c];
      rn.flags = 0;
      d.runs[(u64)q * RUNS_PER_Q + nr] = rn;
      ++nr;
      qp += cnt;
    }
    d.q_nruns[q] = nr;
    d.q_head[q] = qp;
    d.q_rr[q] = (r + 1) % mall;
    if (d.limits) s_head = qp;
    if (BL) s_bytes = 0;   // (read above; the block sums the dispatched entries' body bytes into it next)
  }
  if (d.limits) {   // kernel-uniform: the step's final head through LDS to wave 0
    __syncthreads();
    if (BL) {
      // the body bytes of what the dispatch took, [head, s_head): summed once the budget and slot
      // cuts of (3) have fixed the runs, so the count is exact under any cut; four entries a
      // thread per round, their ring loads then their message loads in flight together
      const u64 hend = s_head;
      constexpr u32 U = 4;
      u64 took = 0;
      for (u64 k0 = head + tid; k0 < hend; k0 += 256 * U) {
        u32 mg[U];
#pragma unroll
        for (u32 u = 0; u < U; ++u) {
          const u64 k = k0 + (u64)u * 256;
          mg[u] = k < hend ? ring[k & mask].msg : INVALID;
        }
#pragma unroll
        for (u32 u = 0; u < U; ++u)
          if (mg[u] != INVALID) took += d.msgs[mg[u]].body_len;
      }
      took = (u64)wave_sum64((i64)took);
      if (lane == 0 && took) atomicAdd(&s_bytes, (unsigned long long)took);
      __syncthreads();
    }
    if (tid < 64) trim_head<DLX, BL>(d, q, s_head, tail, mask, ring, BL ? s_qb - s_bytes : 0ull);
  }
  return true;
}

// K8 dequeue, one block per queue; the last block to finish (ticket) then lays out the
// step's delivery runs (runs_body, once the kernel k_runs: a launch less per step)
template <u32 NT> DEV void runs_body(const DS& d, u64* key_lds, u32 key_cap, u32* lds);
#define DQ_RUN_LDS 2048   // runs that runs_body sorts in LDS (more: the global-memory sort)
// PRIO: no ticket and no runs_body here -- k_prio_dispatch, launched next, adds the priority queues'
// runs and its last block lays out the step's
template <bool DLX, bool BL = false, bool PRIO = false>
__global__ __launch_bounds__(256) void k_dequeue(DS d) {
  __shared__ u64 key_lds[DQ_RUN_LDS];
  __shared__ u32 lds[256 / 64 + 1];
  __shared__ u32 s_last;
  const bool wrote = dequeue_queue<DLX, BL, PRIO>(d);
  if (PRIO) return;
  // every block's runs and counts reach the device-wide coherence point before its ticket
  // (agent scope: the last block may run on another XCD, whose L2 does not see this one's);
  // a block that wrote no runs stored its zero count agent-coherent and skips the L2
  // write-back that release costs
  if (wrote) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(&d.tot[TS_DQ_TICKET], 1u) == gridDim.x - 1;
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (threadIdx.x == 0) d.tot[TS_DQ_TICKET] = 0;
  runs_body<256>(d, key_lds, DQ_RUN_LDS, lds);
}

// ============================================================================ runs -> deliveries
// One block: gather the step's runs (queue order, then round-robin order), sort them by
// channel (bitonic on (channel << 32 | run slot): ties keep queue order, the stable order
// of the reference's per-channel delivery), lay out their deliveries contiguously, and
// record the first delivery of every channel / first and last of every connection.
DEV void bitonic_sort_u64(u64* k, u32 np2, u32 tid, u32 nt) {
  for (u32 sz = 2; sz <= np2; sz <<= 1) {
    for (u32 j = sz >> 1; j > 0; j >>= 1) {
      for (u32 i = tid; i < np2; i += nt) {
        u32 ij = i ^ j;
        if (ij > i) {
          bool up = (i & sz) == 0;
          u64 a = k[i], b = k[ij];
          if ((a > b) == up) { k[i] = b; k[ij] = a; }
        }
      }
      __syncthreads();
    }
  }
}

template <u32 NT>
DEV void runs_body(const DS& d, u64* key_lds, u32 key_cap, u32* lds) {
  const u32 tid = threadIdx.x;
  // pass 1: total runs
  u32 R = 0;
  for (u32 b0 = 0; b0 < d.q_max; b0 += NT) {
    u32 qq = b0 + tid;
    u32 v = qq < d.q_max ? d.q_nruns[qq] : 0;
    u32 all;
    u32 off = block_scan<NT>(v, lds, all);
    for (u32 j = 0; j < v; ++j) {
      const u32 slot = qq * RUNS_PER_Q + j;
      const u32 pos = R + off + j;
      const u64 k = ((u64)d.runs[slot].ch << 32) | slot;
      if (pos < key_cap) key_lds[pos] = k;
      d.run_key[pos] = k;
    }
    R += all;
  }
  __syncthreads();
  u32 np2 = 1;
  while (np2 < R) np2 <<= 1;
  const bool in_lds = np2 <= key_cap;
  u64* key = in_lds ? key_lds : d.run_key;
  for (u32 i = R + tid; i < np2; i += NT) key[i] = ~0ull;
  __syncthreads();
  if (R > 1) bitonic_sort_u64(key, np2, tid, NT);
  // pass 2: delivery offsets in run order
  u32 run = 0;
  for (u32 b0 = 0; b0 < R; b0 += NT) {
    const u32 s = b0 + tid;
    u32 cnt = 0, slot = 0;
    if (s < R) { slot = (u32)key[s]; cnt = d.runs[slot].cnt; }
    u32 all;
    u32 off = block_scan<NT>(cnt, lds, all);
    if (s < R) {
      const u32 start = run + off;
      d.run_order[s] = slot;
      d.run_start[s] = start;
      const u32 ch = (u32)(key[s] >> 32);
      const u32 conn = ch / d.chpc;
      const u32 pch = s > 0 ? (u32)(key[s - 1] >> 32) : INVALID;
      const u32 nch = s + 1 < R ? (u32)(key[s + 1] >> 32) : INVALID;
      if (pch != ch) d.ch_first[ch] = start;
      if (pch == INVALID || pch / d.chpc != conn) d.conn_dfirst[conn] = start;
      if (nch == INVALID || nch / d.chpc != conn) d.conn_dlast[conn] = start + cnt - 1;
    }
    run += all;
  }
  if (tid == 0) {
    d.tot[TS_NRUNS] = R;
    d.ctr->n_deliv = run;   // the saturating slot counter may have ended above deliv_max
  }
}

#include "dp_prio.h"   // k_prio_lane, k_prio_dispatch (DS.prio)

// thread per delivery: expand its run (binary search), assign the channel's next delivery
// tag, fill the unacked window slot, size the rendered frames
#define DVW_LDS 512   // runs staged in LDS per block (more: searched in global memory)
__global__ __launch_bounds__(256) void k_dv_write(DS d) {
  __shared__ u32 s_start[DVW_LDS];
  __shared__ Run s_run[DVW_LDS];
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 n = d.ctr->n_deliv;
  const bool valid = i < n;
  u32 lat = 0, nref = 0, rbytes = 0;
  Deliv dv;
  dv.msg = INVALID; dv.q = 0; dv.qpos = 0; dv.flags = 2;
  const u32 R = d.tot[TS_NRUNS];
  // the step's runs (run order) staged in LDS by the block: one coalesced load of the
  // starts and the runs instead of a chain of dependent global loads per delivery (the
  // binary search's probes, then run_order -> runs)
  const bool lds_runs = R <= DVW_LDS;
  if (lds_runs && blockIdx.x * blockDim.x < n) {   // (block-uniform)
    for (u32 s = threadIdx.x; s < R; s += blockDim.x) {
      s_start[s] = d.run_start[s];
      s_run[s] = d.runs[d.run_order[s]];
    }
    __syncthreads();
  }
  if (valid) {
    u32 lo = 0, hi = R;   // last s with run_start[s] <= i
    while (hi - lo > 1) {
      u32 mid = (lo + hi) >> 1;
      if ((lds_runs ? s_start[mid] : d.run_start[mid]) <= i) lo = mid; else hi = mid;
    }
    const Run rn = lds_runs ? s_run[lo] : d.runs[d.run_order[lo]];
    const u32 k = i - (lds_runs ? s_start[lo] : d.run_start[lo]);
    const Desc ds = d.ring[d.q_ring_off[rn.q] + ((rn.qpos + k) & d.q_ring_mask[rn.q])];
    const u32 ch = rn.ch;
    const u64 tag = d.ch_next_tag[ch] + (i - d.ch_first[ch]);
    const bool get = rn.flags & RUN_GET;
    const u32 cons = get ? d.cons_max : rn.cons;   // Basic.Get: the reserved slot cons_max
    dv.chslot = ch;
    dv.cons = rn.cons;   // Basic.Get: the message-count of the GetOk
    dv.msg = ds.msg;
    dv.q = rn.q;
    dv.qpos = rn.qpos + k;
    dv.expire_ms = ds.expire_ms;
    dv.tag = tag;
    dv.flags = (ds.flags & 1) | (rn.noack ? 2u : 0u) | (get ? DV_GET : 0u);
    USlot u;
    u.state = rn.noack ? US_DONE : US_PENDING;
    u.msg = ds.msg;
    u.q = rn.q;
    u.cons = cons;
    u.qpos = dv.qpos;
    u.expire_ms = ds.expire_ms;
    d.uwin[(u64)ch * (d.ucap_mask + 1) + ((tag - 1) & d.ucap_mask)] = u;
    const MsgEnt& m = d.msgs[ds.msg];
    const bool ref = deliv_href(d, m, ch / d.chpc) != 0;
    const u32 sz = deliver_size(d, cons, m, ch / d.chpc) - (ref ? m.body_len : 0u);
    dv.size = sz;
    d.dv_size[i] = sz;
    if (ref) { nref = 1; rbytes = m.body_len; }
    d.deliv[i] = dv;
    lat = (u32)d.in->step - m.pub_step;
    // the channel's last delivery this step: the window needs a k_chan_advance pass
    bool last = i + 1 == n ||
                (k + 1 == rn.cnt && (lo + 1 >= R || (lds_runs ? s_run[lo + 1].ch : d.runs[d.run_order[lo + 1]].ch) != ch));
    if (last) {
      // auto-ack channel with nothing pending (no manual delivery awaiting a settle, no
      // deferred marks): every slot up to this tag is done, so the window head moves here
      // and k_chan_advance has nothing to walk for it
      if (rn.noack && d.ch_unacked[ch] == 0 && d.ch_dirty[ch] == 0) {
        const u64 head = d.ch_uhead[ch];
        atomicSub(&d.ch_win[ch], (u32)(tag + 1 - head));
        d.ch_uhead[ch] = tag + 1;
      } else if (atomicExch(&d.ch_dirty[ch], 1u) == 0) {
        u32 kk = atomicAdd(d.n_dirty, 1u);
        d.dirty_list[kk] = ch;
      }
    }
  } else if (i < d.deliv_max) {
    d.dv_size[i] = 0;
  }
  if (d.persist)   // manual-ack delivery of a persistent message: its row becomes an unack
    wave_consumed(d, dv.msg, dv.q, dv.qpos, 3u, valid && !(dv.flags & 2));
  wave_add_u32(d.ctr->lat_hist, lat < LAT_BINS ? lat : LAT_BINS - 1, 1u, valid);
  {   // referenced deliveries / body bytes of the step (one atomic per wave)
    u32 nr = nref;
    u64 rb = rbytes;
    for (int o = 32; o > 0; o >>= 1) { nr += __shfl_xor(nr, o, 64); rb += shfl_xor64(rb, o); }
    if (lane_id() == 0 && nr) {
      atomicAdd(&d.ctr->n_ref, nr);
      atomicAdd((unsigned long long*)&d.ctr->ref_bytes, (unsigned long long)rb);
    }
  }
}

// per connection: egress size = returns + confirms + deliveries
__global__ void k_conn_sizes(DS d) {
  u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d.c_max) return;
  u32 conf = 0;
  for (u32 l = 0; l < d.chpc; ++l) {
    u32 ch = c * d.chpc + l;
    if (d.ch_pub_cnt[ch] && d.ch_confirm[ch]) conf += 21;
  }
  d.conn_conf_bytes[c] = conf;
  u32 dl = 0;
  u32 f = d.conn_dfirst[c];
  if (f != INVALID) {
    u32 l = d.conn_dlast[c];
    dl = d.dv_off[l] + d.dv_size[l] - d.dv_off[f];
  }
  d.conn_total[c] = d.conn_ret_bytes[c] + conf + dl + 13u * d.conn_gempty[c];
}

// the step's D2H size: its rendered bytes, then -- when any delivery references a host
// body -- the gather table (one EgressRef per delivery), so one copy carries both
DEV void set_egress_bytes(const DS& d, u32 eb) {
  if (d.ctr->n_ref) {
    u32 nd = d.ctr->n_deliv;
    if (nd > d.deliv_max) nd = d.deliv_max;
    const u32 go = align16(eb);
    d.ctr->gath_off = go;
    eb = go + 16u * nd;
  }
  d.ctr->egress_bytes = eb;
}

// single block (c_max <= CONN_LAYOUT_MAX): k_conn_sizes + scan of conn_total + k_conn_out
#define CONN_LAYOUT_MAX 8192
__global__ __launch_bounds__(1024) void k_conn_layout(DS d) {
  __shared__ u32 lds[1024 / 64 + 1];
  // exclusive scan of the deliveries' rendered sizes (fused k_scan: one block walks the
  // step's deliveries 16K at a time -- 16 per thread, all loads of a pass in flight at
  // once, one block scan per pass: a step's deliveries usually take one pass)
  {
    u32 n = d.ctr->n_deliv;
    if (n > d.deliv_max) n = d.deliv_max;
    u32 acc = 0;
    constexpr u32 EPT = 16;
    for (u32 b0 = 0; b0 < n; b0 += 1024 * EPT) {
      const u32 i0 = b0 + threadIdx.x * EPT;
      u32 v[EPT];
      if (i0 + EPT <= n) {   // dv_size is 16-byte aligned and i0 a multiple of 16
        const uint4* src = (const uint4*)(d.dv_size + i0);
#pragma unroll
        for (u32 k = 0; k < EPT / 4; ++k) {
          const uint4 x = src[k];
          v[4 * k] = x.x; v[4 * k + 1] = x.y; v[4 * k + 2] = x.z; v[4 * k + 3] = x.w;
        }
      } else {
#pragma unroll
        for (u32 k = 0; k < EPT; ++k) v[k] = i0 + k < n ? d.dv_size[i0 + k] : 0u;
      }
      u32 sum = 0;
#pragma unroll
      for (u32 k = 0; k < EPT; ++k) sum += v[k];
      u32 all;
      u32 o = acc + block_scan<1024>(sum, lds, all);
      if (i0 + EPT <= n) {
        uint4* dst = (uint4*)(d.dv_off + i0);
#pragma unroll
        for (u32 k = 0; k < EPT / 4; ++k) {
          uint4 x;
          x.x = o; o += v[4 * k];
          x.y = o; o += v[4 * k + 1];
          x.z = o; o += v[4 * k + 2];
          x.w = o; o += v[4 * k + 3];
          dst[k] = x;
        }
      } else {
#pragma unroll
        for (u32 k = 0; k < EPT; ++k) {
          if (i0 + k < n) d.dv_off[i0 + k] = o;
          o += v[k];
        }
      }
      acc += all;
      __syncthreads();   // lds of the next pass's scan
    }
    if (threadIdx.x == 0) d.tot[TS_DELIV_BYTES] = acc;
    __syncthreads();
  }
  u32 run = 0;
  for (u32 b0 = 0; b0 < d.c_max; b0 += 1024) {
    const u32 c = b0 + threadIdx.x;
    u32 total = 0;
    if (c < d.c_max) {
      u32 conf = 0;
      for (u32 l = 0; l < d.chpc; ++l) {
        u32 ch = c * d.chpc + l;
        if (d.ch_pub_cnt[ch] && d.ch_confirm[ch]) conf += 21;
      }
      d.conn_conf_bytes[c] = conf;
      u32 dl = 0;
      u32 f = d.conn_dfirst[c];
      if (f != INVALID) {
        u32 l = d.conn_dlast[c];
        dl = d.dv_off[l] + d.dv_size[l] - d.dv_off[f];
      }
      total = d.conn_ret_bytes[c] + conf + dl + 13u * d.conn_gempty[c];
      d.conn_total[c] = total;
    }
    u32 all;
    const u32 off = block_scan<1024>(total, lds, all);
    if (c < d.c_max) {
      ConnOut o;
      o.off = run + off;
      o.len = d.links && d.conn_link[c] ? 0u : total;   // links: their bytes go to lsend_*
      d.conn_base[c] = o.off;
      d.conn_out[c] = o;
      if (c == d.c_max - 1) set_egress_bytes(d, o.off + total);
    }
    run += all;
  }
}

__global__ void k_conn_out(DS d) {
  u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d.c_max) return;
  ConnOut o;
  o.off = d.conn_base[c];
  o.len = d.links && d.conn_link[c] ? 0u : d.conn_total[c];
  d.conn_out[c] = o;
  if (c == d.c_max - 1) set_egress_bytes(d, o.off + d.conn_total[c]);
}

// ============================================================================ links (X2/X3)
// one wave: record / payload bases of every link pseudo-connection's deliveries in this
// parity's link send buffers, destination-major (the host reads the per-destination
// totals from xchg and sends each destination's region to it in the next exchange)
__global__ __launch_bounds__(64) void k_link_bases(DS d) {
  const u32 lane = threadIdx.x;
  const u32 nl = *d.n_link_conns;
  u32 c = INVALID, dest = INVALID, n = 0, b = 0;
  if (lane < nl && lane < 64) {
    c = d.link_conns[lane];
    const u32 lk = d.conn_link[c];
    const u32 f = d.conn_dfirst[c];
    if (lk) {
      dest = lk - 1;
      if (f != INVALID) { n = d.conn_dlast[c] - f + 1; b = d.conn_total[c]; }
    }
  }
  u32 npre = 0, bpre = 0, tn = 0, tb = 0;
  for (u32 j = 0; j < 64; ++j) {
    const u32 dj = __shfl(dest, j, 64), nj = __shfl(n, j, 64), bj = __shfl(b, j, 64);
    if (j < lane && dj == dest) { npre += nj; bpre += bj; }
    if (dj == lane) { tn += nj; tb += bj; }
  }
  u32 basen = 0, baseb = 0;
  for (u32 r = 0; r < 64; ++r) {
    const u32 x = __shfl(tn, r, 64), y = __shfl(tb, r, 64);
    if (r < lane) { basen += x; baseb += y; }
  }
  if (lane < d.world) {
    d.link_dbase[lane] = baseb;
    d.xchg[XC_LINK_N + lane] = tn;
    d.xchg[XC_LINK_B + lane] = tb;
  }
  const u32 sl = dest < 64 ? dest : 0;
  const u32 dbn = __shfl(basen, sl, 64);
  if (c != INVALID) {
    d.link_nbase[c] = dbn + npre;
    d.link_bbase[c] = bpre;
  }
}

// owner side, phase B (k_import_route): an ack a connection side sent for a link pseudo channel
// (the device form of Basic.Ack on the owner's pseudo channel; k_chan_advance settles)
DEV void link_ack_one(const DS& d, u32 i) {
  const AckRec a = d.rack[i];
  if (a.tq >= d.q_max) return;
  const u32 ch = d.q_link_ch[a.tq];
  if (ch == INVALID || (u32)(a.xid >> 40) != d.q_link_epoch[a.tq]) return;
  const u64 tag = a.xid & ((1ull << 40) - 1);
  if (tag < d.ch_uhead[ch] || tag >= d.ch_next_tag[ch]) return;
  USlot* u = &d.uwin[(u64)ch * (d.ucap_mask + 1) + ((tag - 1) & d.ucap_mask)];
  if (atomicCAS(&u->state, (u32)US_PENDING, (u32)US_ACKED) == US_PENDING &&
      atomicExch(&d.ch_dirty[ch], 1u) == 0)
    d.dirty_list[atomicAdd(d.n_dirty, 1u)] = ch;
}

// ============================================================================ K5 render
DEV u32 put_frame_hdr(u8* o, u32 type, u32 ch, u32 size) {
  o[0] = (u8)type;
  wr16(o + 1, ch);
  wr32(o + 3, size);
  return 7;
}

// one group of RD_G lanes per delivery i (< n_deliv), lane = 0..RD_G-1: with egress by
// reference a delivery is ~100 bytes of frames, so a whole wave per delivery left 3/4 of
// its lanes idle (four deliveries per wave now)
#define RD_G 16
DEV void render_deliv(const DS& d, u32 i, u32 lane) {
  const Deliv dv = d.deliv[i];
  const u32 ch = dv.chslot;
  const MsgEnt m = d.msgs[dv.msg];
  u32 conn = ch / d.chpc;
  u32 f = d.conn_dfirst[conn];
  const u8* slot = msg_slot(d, m.log_off);
  // gather entry of this delivery (the table exists when some delivery of the step
  // references its body; dst of an unreferenced one = its end, so dst never decreases)
  const u64 href = deliv_href(d, m, conn);
  const bool ref = href != 0;
  EgressRef* gt = d.ctr->n_ref ? (EgressRef*)((u8*)d.in->egress + d.ctr->gath_off) : nullptr;
  if (d.links && d.conn_link[conn]) {   // X2: a restore record for the shadow queue
    if (gt && lane == 0) gt[i] = EgressRef{0ull, d.conn_base[conn], 0u};
    const u32 dest = d.conn_link[conn] - 1;
    const u32 po = d.link_bbase[conn] + (d.dv_off[i] - d.dv_off[f]);
    u8* lo = d.lsend_pay + (u64)d.link_dbase[dest] + po;
    const u32 meta = m.ex_len + m.rk_len + m.props_len;
    group_copy<RD_G>(lo, slot, meta, lane);
    group_copy<RD_G>(lo + meta, slot + m.body_off, m.body_len, lane);
    if (lane == 0) {
      RDesc rd{};
      rd.pay_off = po;
      rd.body_len = m.body_len;
      rd.props_len = m.props_len;
      rd.exch = -1;
      rd.flags = MF_RESTORE | ((dv.flags & 1) ? MF_REDELIVERED : 0u);
      rd.ex_len = m.ex_len;
      rd.rk_len = m.rk_len;
      rd.expire_ms = dv.expire_ms;
      rd.ts_ms = m.ts_ms;
      rd.xid = ((u64)d.conn_link_epoch[conn] << 40) | (dv.tag & ((1ull << 40) - 1));
      rd.tq = d.conn_link_tq[conn];
      d.lsend_desc[d.link_nbase[conn] + (i - f)] = rd;
    }
    return;
  }
  u64 off = (u64)d.conn_base[conn] + d.conn_ret_bytes[conn] + d.conn_conf_bytes[conn] + d.dv_off[i] -
            d.dv_off[f];
  if (gt && lane == 0)   // (a referenced body goes after its body frame's 7-byte header)
    gt[i] = ref ? EgressRef{href, (u32)(off + dv.size - 1u), m.body_len} : EgressRef{0ull, (u32)(off + dv.size), 0u};
  // never: dequeue reserves an egress byte budget.  (Against the buffer, not egress_cap: that
  // bounds the step's deliveries, and off also counts the returns and confirms in front)
  if (off + dv.size > d.egress_alloc) return;
  u8* o = (u8*)d.in->egress + off;
  u32 chno = d.ch_num[ch];
  const bool get = dv.flags & DV_GET;   // Basic.GetOk (60/71): no consumer tag, message-count last
  u32 taglen = get ? 0u : d.cons_tag_len[dv.cons];
  u32 mp = (get ? 4 + 4 : 4 + 1 + taglen) + 8 + 1 + 1 + m.ex_len + 1 + m.rk_len;
  u64 dtag = dv.tag;
  // method frame: scalar fields by lane 0, the variable-length strings (consumer tag,
  // exchange, routing key) by all lanes in parallel (no serial byte-load chains)
  const u32 p_tag = 7 + 4 + (get ? 0 : 1), p_ex = p_tag + taglen + 8 + 1 + 1, p_rk = p_ex + m.ex_len + 1;
  if (lane == 0) {
    put_frame_hdr(o, 1, chno, mp);
    wr16(o + 7, 60); wr16(o + 9, get ? 71 : 60);
    if (!get) o[11] = (u8)taglen;
    wr64(o + p_tag + taglen, dtag);
    o[p_tag + taglen + 8] = (dv.flags & 1) ? 1 : 0;
    o[p_ex - 1] = m.ex_len;
    o[p_rk - 1] = m.rk_len;
    u32 p = p_rk + m.rk_len;
    if (get) { wr32(o + p, dv.cons); p += 4; }
    o[p++] = 0xCE;
    p += put_frame_hdr(o + p, 2, chno, 12 + m.props_len);
    wr16(o + p, 60); wr16(o + p + 2, 0); wr64(o + p + 4, m.body_len);
  }
  if (!get) {
    const u8* tg = d.tpool + d.cons_tag_off[dv.cons];
    for (u32 k = lane; k < taglen; k += RD_G) o[p_tag + k] = tg[k];
  }
  for (u32 k = lane; k < m.ex_len; k += RD_G) o[p_ex + k] = slot[k];
  for (u32 k = lane; k < m.rk_len; k += RD_G) o[p_rk + k] = slot[m.ex_len + k];
  u32 hp = 8 + mp + 7 + 12;
  group_copy<RD_G>(o + hp, slot + m.ex_len + m.rk_len, m.props_len, lane);
  if (lane == 0) o[hp + m.props_len] = 0xCE;
  u32 bp = hp + m.props_len + 1;
  u32 fm = d.conn_frame_max[conn];
  u32 fmb = fm ? fm - 8 : 0xffffffffu;
  if (ref) {   // one body frame whose payload the host inserts: header, then the frame end
    if (lane == 0) {
      put_frame_hdr(o + bp, 3, chno, m.body_len);
      o[bp + 7] = 0xCE;
    }
    return;
  }
  const u8* body = slot + m.body_off;
  for (u32 b0 = 0; b0 < m.body_len; b0 += fmb) {
    u32 bl = m.body_len - b0 < fmb ? m.body_len - b0 : fmb;
    if (lane == 0) put_frame_hdr(o + bp, 3, chno, bl);
    group_copy<RD_G>(o + bp + 7, body + b0, bl, lane);
    if (lane == 0) o[bp + 7 + bl] = 0xCE;
    bp += bl + 8;
  }
}

// confirms: one thread per connection writes its channels' coalesced confirm frames:
// Basic.Ack(last, multiple) when every publish of the channel in this step was stored,
// else Basic.Nack(last, multiple, requeue=0) over the step's whole range — a publisher
// may resend a nacked message, it never loses an acked one (FrameStage.scala:571-596
// confirms everything it asked the entities to store; drops are ours: ring full, no memory)
DEV void render_confirms(const DS& d, u32 c) {
  const u32 ng = d.conn_gempty[c];
  if (ng) {   // Basic.GetEmpty (60/72, empty cluster-id) frames close the connection's region
    u8* e = (u8*)d.in->egress + (u64)d.conn_base[c] + d.conn_total[c] - 13u * ng;
    const u32 chno = d.conn_gempty_ch[c];
    for (u32 k = 0; k < ng; ++k, e += 13) {
      put_frame_hdr(e, 1, chno, 5);
      wr16(e + 7, 60); wr16(e + 9, 72);
      e[11] = 0;
      e[12] = 0xCE;
    }
  }
  u32 conf = d.conn_conf_bytes[c];
  u8* o = (u8*)d.in->egress + (u64)d.conn_base[c] + d.conn_ret_bytes[c];
  u32 p = 0;
  for (u32 l = 0; l < d.chpc; ++l) {
    u32 ch = c * d.chpc + l;
    u32 cnt = d.ch_pub_cnt[ch];
    const bool fail = d.ch_pub_fail[ch] != 0;
    if (fail) d.ch_pub_fail[ch] = 0;
    if (!cnt) continue;
    d.ch_pub_cnt[ch] = 0;
    if (!d.ch_confirm[ch]) continue;
    u64 last = d.ch_confirm_next[ch] + cnt - 1;
    d.ch_confirm_next[ch] = last + 1;
    u32 chno = d.ch_num[ch];
    if (p + 21 > conf) break;
    put_frame_hdr(o + p, 1, chno, 13);
    wr16(o + p + 7, 60); wr16(o + p + 9, fail ? 120 : 80);
    wr64(o + p + 11, last);
    o[p + 19] = cnt > 1 ? 1 : 0;
    o[p + 20] = 0xCE;
    p += 21;
    atomicAdd(&d.ctr->n_confirm_frames, 1u);
  }
}

// returns: one wave per returned publish (Basic.Return 312/313 + header + body)
DEV void render_return(const DS& d, u32 i, u32 lane) {
  u32 p = d.ret_list[i];
  const Pub pb = d.pubs[p];
  u32 code = d.pub_ret[p];
  u8* o = (u8*)d.in->egress + (u64)d.conn_base[pb.conn] + (d.pub_ret_off[p] - d.conn_ret_min[pb.conn]);
  const u8* w = d.work;
  // channel number from the publish command's frame
  u32 chno = d.ch_num[pb.chslot];
  const char* txt = code == 312 ? "The exchange cannot route the result of a Publish"
                                : "The exchange cannot deliver to a consumer when the immediate flag is set";
  u32 tl = 0;
  while (txt[tl]) ++tl;
  u32 mp = 4 + 2 + 1 + tl + 1 + pb.ex_len + 1 + pb.rk_len;
  if (lane == 0) {
    u32 q = 0;
    q += put_frame_hdr(o, 1, chno, mp);
    wr16(o + q, 60); wr16(o + q + 2, 50); q += 4;
    wr16(o + q, code); q += 2;
    o[q++] = (u8)tl;
    for (u32 k = 0; k < tl; ++k) o[q + k] = (u8)txt[k];
    q += tl;
    o[q++] = (u8)pb.ex_len;
    for (u32 k = 0; k < pb.ex_len; ++k) o[q + k] = w[pb.ex_off + k];
    q += pb.ex_len;
    o[q++] = (u8)pb.rk_len;
    for (u32 k = 0; k < pb.rk_len; ++k) o[q + k] = w[pb.rk_off + k];
    q += pb.rk_len;
    o[q++] = 0xCE;
    q += put_frame_hdr(o + q, 2, chno, 12 + pb.props_len);
    wr16(o + q, 60); wr16(o + q + 2, 0); wr64(o + q + 4, pb.body_size);
  }
  u32 hp = 8 + mp + 7 + 12;
  wave_copy(o + hp, w + pb.props_off, pb.props_len);
  if (lane == 0) o[hp + pb.props_len] = 0xCE;
  u32 bp = hp + pb.props_len + 1;
  u32 fm = d.conn_frame_max[pb.conn];
  u32 fmb = fm ? fm - 8 : 0xffffffffu;
  // body from ingress fragments, re-split at the connection's frame size
  u32 fi = 0, fo = 0;
  for (u32 b0 = 0; b0 < pb.body_size; b0 += fmb) {
    u32 bl = pb.body_size - b0 < fmb ? pb.body_size - b0 : fmb;
    if (lane == 0) put_frame_hdr(o + bp, 3, chno, bl);
    u32 done = 0;
    while (done < bl) {
      Frag fg = d.frags[pb.frag0 + fi];
      u32 take = fg.len - fo < bl - done ? fg.len - fo : bl - done;
      wave_copy(o + bp + 7 + done, w + fg.off + fo, take);
      done += take;
      fo += take;
      if (fo == fg.len) { ++fi; fo = 0; }
    }
    if (lane == 0) o[bp + 7 + bl] = 0xCE;
    bp += bl + 8;
  }
}

// blocks [0, RC_RET_BLOCKS): returns, grid-stride, one wave each; the rest: confirms,
// one thread per connection
#define RC_RET_BLOCKS 512
DEV void render_rc(const DS& d, u32 blk);
// one launch for all egress rendering: returns / confirms blocks first, then one wave per
// delivery (the two write disjoint byte ranges of each connection's egress)
__global__ __launch_bounds__(256) void k_render(DS d, u32 n_rc) {
  if (blockIdx.x < n_rc) { render_rc(d, blockIdx.x); return; }
  const u32 n = d.ctr->n_deliv;
  const u32 ng = ((gridDim.x - n_rc) * blockDim.x) / RD_G;
  const u32 g = ((blockIdx.x - n_rc) * blockDim.x + threadIdx.x) / RD_G;
  const u32 lane = threadIdx.x % RD_G;
  for (u32 i = g; i < n; i += ng) render_deliv(d, i, lane);
}
DEV void render_rc(const DS& d, u32 blk) {
  if (blk >= RC_RET_BLOCKS) {
    u32 c = (blk - RC_RET_BLOCKS) * blockDim.x + threadIdx.x;
    if (c < d.c_max) render_confirms(d, c);
    return;
  }
  u32 n = d.ctr->n_returns;
  if (n > d.pub_max) n = d.pub_max;
  const u32 lane = lane_id();
  for (u32 i = (blk * blockDim.x + threadIdx.x) >> 6; i < n; i += RC_RET_BLOCKS * 4) render_return(d, i, lane);
}

// ============================================================================ post / final
// (a last-block ticket here to fold k_host_out in costs more than the launch it saves:
// hundreds of blocks serialise on the ticket word)
DEV void final_step(const DS& d);
DEV void host_out_copies(const DS& d, u64 gtid, u64 gsz);
// fin (no persistence: nothing runs after it): the host-visible copies and, by the last
// block to finish (ticket), the log tail + counters (fused k_host_out)
__global__ __launch_bounds__(256) void k_post(DS d, u32 fin) {
  __shared__ u32 s_last;
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  u32 n = d.ctr->n_deliv;
  u32 msg = INVALID, q = 0;
  u64 qpos = 0;
  bool aa = false;
  if (i < n) {
    const Deliv& dv = d.deliv[i];
    aa = dv.flags & 2;
    msg = dv.msg;
    q = dv.q;
    qpos = dv.qpos;
    const u32 ch = dv.chslot;
    if (i + 1 == n || d.deliv[i + 1].chslot != ch) d.ch_next_tag[ch] = dv.tag + 1;
  }
  wave_consumed(d, msg, q, qpos, 0u, aa);
  wave_release(d, msg, aa);
  const u32 nd = d.tot[TS_NDEFER], gs = gridDim.x * blockDim.x;
  for (u32 b = 0; b < nd; b += gs)   // grid-uniform trip count (wave_release ballots)
    wave_release(d, b + i < nd ? d.defer_free[b + i] : INVALID, b + i < nd);
  // consumers a light control section activated (cons_active 2, applied by this or an
  // earlier step's k_stage) take deliveries from the next step on: this step's dequeue (it
  // ran before this kernel) rendered none for them, so its egress -- behind which the front
  // end releases the Basic.ConsumeOk (Frontend::send_after) -- never holds a Basic.Deliver
  // that overtakes the ConsumeOk.  (Here and not in the next step's k_stage: with the
  // overlapped engine that k_stage may run beside this step's k_dequeue; a step that stages
  // writes waits for the previous step's routing half, so no 2 written after this point is
  // flipped by it)
  for (u32 c = i; c < d.cons_max; c += gridDim.x * blockDim.x)
    if (d.cons_active[c] == 2u) d.cons_active[c] = 1u;
  // reset per-connection scratch (fused k_post2)
  if (i < d.c_max) {
    d.conn_dfirst[i] = INVALID;
    d.conn_dlast[i] = INVALID;
    d.conn_ret_bytes[i] = 0;
    d.conn_ret_min[i] = INVALID;
    d.conn_gempty[i] = 0;
  }
  if (!fin) return;
  host_out_copies(d, i, (u64)gridDim.x * blockDim.x);
  // every block's releases are done (their atomics returned) before its ticket
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(&d.tot[TS_POST_TICKET], 1u) == gridDim.x - 1;
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (threadIdx.x == 0) {
    d.tot[TS_POST_TICKET] = 0;
    final_step(d);
  }
}


DEV void final_step(const DS& d) {
  // advance the log tail over fully released blocks (K11)
  u64 head = *d.log_head, tail = *d.log_tail;
  while (tail < head) {
    u64 blk_idx = tail / d.log_block;
    if (blk_idx == head / d.log_block) break;
    if (d.log_live[blk_idx % d.n_log_blocks] > 0) break;
    tail = (blk_idx + 1) * d.log_block;
  }
  if (tail > head) tail = head;
  *d.log_tail = tail;
  if (d.spill_bytes) {   // the spill ring's tail, the same way
    const u64 sh = *d.spill_head;
    u64 st = *d.spill_tail;
    while (st < sh) {
      const u64 bi = st / d.log_block;
      if (bi == sh / d.log_block) break;
      if (d.spill_live[bi % d.n_spill_blocks] > 0) break;
      st = (bi + 1) * d.log_block;
    }
    *d.spill_tail = st > sh ? sh : st;
    d.spill_tail_lag[d.in->step % SPILL_LAG] = *d.spill_tail;
  }
  Counters* c = d.ctr;
  c->log_head = head;
  c->log_tail = tail;
  c->msg_free_top = *d.msg_free_top;
  c->n_live_msgs = d.msg_max - *d.msg_free_top;
  c->live_bytes = *d.live_bytes;
  c->n_dget = d.tot[TS_NDGET];
  if (d.dlx) c->n_dl_pending = d.dl->dead_n[0] < d.dl->dead_max ? d.dl->dead_n[0] : d.dl->dead_max;
  if (d.links)
    for (u32 r = 0; r < d.world; ++r) d.xchg[XC_ACK_N + r] = d.lk_cnt[r] < d.lk_cap ? d.lk_cnt[r] : d.lk_cap;
  *d.ctr_host = *c;
  // open the step's egress gate: the SDMA engine, polling it, starts the D2H of this
  // step's egress now.  The rendered bytes left their L2s at the earlier kernels' ends;
  // the system-scope release covers this kernel's own stores (vector store, system scope)
  const u64 gate = d.in->gate;
  if (gate) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store((i64*)gate, (i64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// persistence: size + pack the step's persist records (header + message bytes) into the
// host-mapped persist buffer; the host writes them to the store before it releases the
// step's publisher confirms (write-behind with confirm gating)
__global__ void k_persist_size(DS d) {
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  u32 n = d.ctr->n_persist;
  if (n > d.persist_max) n = d.persist_max;
  if (i >= n) return;
  // a message's bytes travel once per step: with its first record (claimed through the
  // otherwise unused MsgEnt.pad, zeroed when the message is stored); its other queues'
  // records are headers only (PersistHdr.size == sizeof(PersistHdr))
  MsgEnt& m = d.msgs[d.prec[i].msg];
  const u32 bytes = (m.ex_len + m.rk_len + m.props_len + m.body_len + 7u) & ~7u;
  const bool first = atomicCAS(&m.pad, 0u, 1u) == 0u;
  d.ps_size[i] = (u32)sizeof(PersistHdr) + (first ? bytes : 0u);
}

__global__ __launch_bounds__(256) void k_persist_pack(DS d) {
  u32 lane = lane_id();
  u32 n = d.ctr->n_persist;
  if (n > d.persist_max) n = d.persist_max;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    u64 used = d.tot[TS_PERSIST];
    d.ctr->persist_used = (u32)(used < d.persist_bytes ? used : d.persist_bytes);
  }
  const u32 nw = (gridDim.x * blockDim.x) >> 6;
  for (u32 i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nw) {
    const PersistRec r = d.prec[i];
    const MsgEnt m = d.msgs[r.msg];
    u64 off = d.ps_off[i];
    u32 sz = d.ps_size[i];
    if (off + sz > d.persist_bytes) {
      if (lane == 0) atomicAdd(&d.ctr->n_persist_overflow, 1u);
      continue;
    }
    u8* o = d.ps_persist[d.in->pslot] + off;
    const u8* slot = msg_slot(d, m.log_off);
    if (lane == 0) {
      PersistHdr h;
      h.msg_id = (i64)m.msg_id; h.ts_ms = m.ts_ms; h.qpos = r.qpos; h.expire_ms = r.expire_ms;
      h.q = r.q; h.body_len = m.body_len; h.props_len = m.props_len; h.ex_len = m.ex_len; h.rk_len = m.rk_len;
      h.size = sz;
      *(PersistHdr*)o = h;
    }
    if (sz == sizeof(PersistHdr)) continue;   // header only: the bytes ride the message's first record
    u32 meta = m.ex_len + m.rk_len + m.props_len;
    wave_copy(o + sizeof(PersistHdr), slot, meta);
    wave_copy(o + sizeof(PersistHdr) + meta, slot + m.body_off, m.body_len);
  }
}

// egress D2H on a few workgroups (copy_engine=2): 16-B loads from HBM, 16-B stores into
// mapped pinned memory; PCIe is the limit, so a handful of CUs saturate it
__global__ __launch_bounds__(256) void k_copy_out(u8* dst, const u8* src, u64 n) {
  const u64 gtid = blockIdx.x * blockDim.x + threadIdx.x, gsz = (u64)gridDim.x * blockDim.x;
  const u64 nv = n >> 4;
  typedef unsigned int v4u __attribute__((ext_vector_type(4)));
  for (u64 i = gtid; i < nv; i += gsz) ((v4u*)dst)[i] = __builtin_nontemporal_load(((const v4u*)src) + i);
  for (u64 i = (nv << 4) + gtid; i < n; i += gsz) dst[i] = src[i];
}

// the same, sized on the device (the step's egress byte count): launched right behind the
// step's kernels, with no host round trip between render and copy (copy_engine=2, overlap)
__global__ __launch_bounds__(256) void k_copy_out_dev(u8* dst, const u8* src, const Counters* c) {
  const u64 n = c->egress_bytes;
  const u64 gtid = blockIdx.x * blockDim.x + threadIdx.x, gsz = (u64)gridDim.x * blockDim.x;
  const u64 nv = n >> 4;
  typedef unsigned int v4u __attribute__((ext_vector_type(4)));
  for (u64 i = gtid; i < nv; i += gsz) ((v4u*)dst)[i] = __builtin_nontemporal_load(((const v4u*)src) + i);
  for (u64 i = (nv << 4) + gtid; i < n; i += gsz) dst[i] = src[i];
}

// copy the step's small host-visible results to their host-mapped mirrors in one pass
// (16-B stores, grid-stride) once the whole step has run
DEV void copy16(u8* dst, const u8* src, u64 n, u64 gtid, u64 gsz) {
  u64 nv = n >> 4;
  for (u64 i = gtid; i < nv; i += gsz) ((uint4*)dst)[i] = ((const uint4*)src)[i];
  for (u64 i = (nv << 4) + gtid; i < n; i += gsz) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void k_host_out(DS d) {
  if (blockIdx.x == 0 && threadIdx.x == 0) final_step(d);   // log tail, counters -> host
  host_out_copies(d, blockIdx.x * blockDim.x + threadIdx.x, (u64)gridDim.x * blockDim.x);
}

DEV void host_out_copies(const DS& d, u64 gtid, u64 gsz) {
  u32 nseg = d.in->nseg;
  copy16((u8*)d.seg_out_h, (const u8*)d.seg_out, (u64)nseg * sizeof(SegOut), gtid, gsz);
  copy16((u8*)d.conn_out_h, (const u8*)d.conn_out, (u64)d.c_max * sizeof(ConnOut), gtid, gsz);
  copy16((u8*)d.conn_conf_h, (const u8*)d.conn_conf_bytes, (u64)d.c_max * 4, gtid, gsz);
  u32 nc = d.ctr->n_ctrl;
  if (nc > d.seg_max * 2) nc = d.seg_max * 2;
  copy16((u8*)d.ctrl_rec_h, (const u8*)d.ctrl_rec, (u64)nc * sizeof(CtrlRec), gtid, gsz);
  u64 cb = d.ctr->ctrl_bytes;
  if (cb > d.ctrl_cap) cb = d.ctrl_cap;
  copy16(d.ctrl_h, d.ctrl, cb, gtid, gsz);
  if (d.persist) {
    u32 nr = d.ctr->n_consumed;
    if (nr > d.persist_max) nr = d.persist_max;
    copy16((u8*)d.ps_crec[d.in->pslot], (const u8*)d.crec, (u64)nr * sizeof(ConsumedRec), gtid, gsz);
  }
}

// ============================================================================ Basic.Get
// Basic.Get (60/70) between steps, while the connection is paused behind the command
// (FrameStage.scala:1199-1229: Pull(1) -> GetOk / GetEmpty; QueueEntity.scala:318-393).
// One wave: TTL skip of up to 64 head entries (K12), then the head message gets the
// channel's next delivery tag.  Manual ack: a pending window slot that Basic.Ack/Nack/
// Reject/Recover/channel close resolve exactly like a consumer delivery (k_chan_advance);
// no-ack: a done slot, the message is released now.  GetOk + content header + body frames
// (split at the connection's frame-max) are rendered into `out` (host-mapped).
// Consumer bookkeeping uses the spare consumer slot cons_max.
// DS.dlx, a queue with a dead-letter exchange: the expired entries join the dead list, stamped
// with `step` (the last step submitted), and the next step's dead pass takes them; where the
// list has no room the answer is GetEmpty (the entries behind wait for a step to drain it)
// BL (DS.blimits): the skipped entries and the one handed out leave q_bytes
template <bool BL>
__global__ __launch_bounds__(64) void k_basic_get(DS d, u32 q, u32 ch, u32 noack, i64 now, u8* out, u64 out_cap,
                                                  GetRes* res, u32 step) {
  u32 lane = lane_id();
  u64 head = d.q_head[q], tail = d.q_tail[q];
  const u64 mask = d.q_ring_mask[q];
  const Desc* ring = d.ring + d.q_ring_off[q];
  u32 nexp = 0;
  bool more_expired = false, full = false;
  u64 qb = 0;   // BL: the queue's ready bytes
  if (BL) qb = d.q_bytes[q];
  const u32 dx = d.dlx ? d.dl->q_dlx[q] : 0u;
  if (head < tail) {
    u64 idx = head + lane;
    bool valid = idx < tail;
    Desc ds;
    ds.msg = INVALID; ds.expire_ms = 0; ds.flags = 0;
    if (valid) ds = ring[idx & mask];
    bool exp = valid && ds.expire_ms != 0 && ds.expire_ms <= now;
    u64 live = __ballot(valid && !exp);
    nexp = live ? (__ffsll((unsigned long long)live) - 1) : __popcll(__ballot(valid));
    more_expired = !live && head + nexp < tail;
    u32 esz = 0;
    if (BL) {
      if (lane < nexp && ds.msg != INVALID) esz = d.msgs[ds.msg].body_len;   // (before the release)
    }
    if (dx) {
      const u32 left = dead_leave(d, dx, step, ds.msg, ds.expire_ms, q, idx, DL_EXPIRED, nexp);
      full = left < nexp;
      nexp = left;
    }
    bool mine = lane < nexp;
    bool rec = mine && d.q_durable[q] && (d.msgs[ds.msg].flags & MF_PERSIST);
    u64 rm = __ballot(rec);
    if (rec) {
      ConsumedRec r;
      r.msg_id = (i64)d.msgs[ds.msg].msg_id;
      r.qpos = idx;
      r.q = q;
      r.kind = 1;
      r.pad[0] = r.pad[1] = 0;
      res->exp[__popcll(rm & lanemask_lt())] = r;
    }
    if (!dx) wave_release(d, ds.msg, mine);
    if (lane == 0) res->n_exp = __popcll(rm);
    if (BL) qb -= (u64)wave_sum64(mine ? (i64)esz : 0);
    head += nexp;
  } else if (lane == 0) {
    res->n_exp = 0;
  }
  if (head >= tail || more_expired || full) {
    if (lane == 0) {
      d.q_head[q] = head;
      if (BL) d.q_bytes[q] = qb;
      res->status = (more_expired && !full) ? GET_RETRY : GET_EMPTY;
      res->msg_count = (u32)(tail - head);
      res->out_len = 0;
    }
    return;
  }
  if (head >= d.q_cold_lim[q] && (d.msgs[ring[head & mask].msg].log_off & COLD_BIT)) {
    if (lane == 0) {   // the host pages the queue's head back in, then asks again
      d.q_head[q] = head;
      if (BL) d.q_bytes[q] = qb;
      res->status = GET_COLD;
      res->msg_count = (u32)(tail - head);
      res->out_len = 0;
    }
    return;
  }
  const Desc ds = ring[head & mask];
  const MsgEnt m = d.msgs[ds.msg];
  const u32 conn = ch / d.chpc;
  const u32 ucap = d.ucap_mask + 1;
  const u32 msg_count = (u32)(tail - head - 1);
  u32 mp = 4 + 8 + 1 + 1 + m.ex_len + 1 + m.rk_len + 4;
  u32 fm = d.conn_frame_max[conn];
  u32 fmb = fm ? fm - 8 : 0xffffffffu;
  u32 nb = m.body_len ? (m.body_len - 1) / fmb + 1 : 0;   // (no sum: fmb is 2^32 - 1 for frame-max 0)
  u64 need = 8ull + mp + 8 + 12 + m.props_len + m.body_len + 8ull * nb;
  u32 st = need > out_cap ? GET_NO_SPACE : (d.ch_win[ch] >= ucap ? GET_WINDOW_FULL : GET_OK);
  if (st != GET_OK) {
    if (lane == 0) {
      d.q_head[q] = head;
      if (BL) d.q_bytes[q] = qb;
      res->status = st;
      res->msg_count = (u32)(tail - head);
      res->out_len = 0;
    }
    return;
  }
  const u64 tag = d.ch_next_tag[ch];
  const bool redelivered = ds.flags & 1;
  if (lane == 0) {
    d.ch_next_tag[ch] = tag + 1;
    d.ch_win[ch] += 1;
    USlot u;
    u.state = noack ? US_DONE : US_PENDING;
    u.msg = ds.msg;
    u.q = q;
    u.cons = d.cons_max;
    u.qpos = head;
    u.expire_ms = ds.expire_ms;
    d.uwin[(u64)ch * ucap + ((tag - 1) & d.ucap_mask)] = u;
    if (!noack) { d.ch_unacked[ch] += 1; d.cons_unacked[d.cons_max] += 1; }
    if (d.ch_dirty[ch] == 0) {   // k_chan_advance walks the window at the next step
      d.ch_dirty[ch] = 1;
      u32 k = *d.n_dirty;
      d.dirty_list[k] = ch;
      *d.n_dirty = k + 1;
    }
    d.q_head[q] = head + 1;
    if (BL) d.q_bytes[q] = qb - m.body_len;
    res->status = GET_OK;
    res->msg_count = msg_count;
    res->out_len = (u32)need;
    res->tag = tag;
    res->msg_id = (i64)m.msg_id;
    res->qpos = head;
    res->persist = d.q_durable[q] && (m.flags & MF_PERSIST) ? 1u : 0u;
  }
  // render: GetOk(tag, redelivered, exchange, routing-key, message-count) + header + body
  const u8* slot = msg_slot(d, m.log_off);
  const u32 chno = d.ch_num[ch];
  if (lane == 0) {
    u32 p = 0;
    p += put_frame_hdr(out + p, 1, chno, mp);
    wr16(out + p, 60); wr16(out + p + 2, 71); p += 4;
    wr64(out + p, tag); p += 8;
    out[p++] = redelivered ? 1 : 0;
    out[p++] = m.ex_len;
    for (u32 k = 0; k < m.ex_len; ++k) out[p + k] = slot[k];
    p += m.ex_len;
    out[p++] = m.rk_len;
    for (u32 k = 0; k < m.rk_len; ++k) out[p + k] = slot[m.ex_len + k];
    p += m.rk_len;
    wr32(out + p, msg_count); p += 4;
    out[p++] = 0xCE;
    p += put_frame_hdr(out + p, 2, chno, 12 + m.props_len);
    wr16(out + p, 60); wr16(out + p + 2, 0); wr64(out + p + 4, m.body_len);
  }
  u32 hp = 8 + mp + 7 + 12;
  wave_copy(out + hp, slot + m.ex_len + m.rk_len, m.props_len);
  if (lane == 0) out[hp + m.props_len] = 0xCE;
  u32 bp = hp + m.props_len + 1;
  const u8* body = slot + m.body_off;
  for (u32 b0 = 0; b0 < m.body_len; b0 += fmb) {
    u32 bl = m.body_len - b0 < fmb ? m.body_len - b0 : fmb;
    if (lane == 0) put_frame_hdr(out + bp, 3, chno, bl);
    wave_copy(out + bp + 7, body + b0, bl);
    if (lane == 0) out[bp + 7 + bl] = 0xCE;
    bp += bl + 8;
  }
  wave_release(d, ds.msg, noack && lane == 0);
}

// ============================================================================ spill (between steps)
// reserve `sz` bytes in the spill ring (never across its wrap), false when it is full
DEV bool spill_reserve(const DS& d, u32 sz, u64* pos) {
  unsigned long long cur = __hip_atomic_load(d.spill_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // the tail of SPILL_LAG steps ago (the oldest of the history): bytes freed since may still
  // be referenced by an egress not yet written out (spilled bodies are sent from the ring)
  u64 tail = *d.spill_tail;
  for (u32 k = 0; k < SPILL_LAG; ++k) tail = d.spill_tail_lag[k] < tail ? d.spill_tail_lag[k] : tail;
  while (true) {
    u64 h = cur;
    const u64 phys = h % d.spill_bytes;
    if (phys + sz > d.spill_bytes) h += d.spill_bytes - phys;
    if (h + sz - tail > d.spill_bytes) return false;
    const unsigned long long prev = atomicCAS((unsigned long long*)d.spill_head, cur, (unsigned long long)(h + sz));
    if (prev == cur) { *pos = h; return true; }
    cur = prev;
  }
}

// the tail spill_reserve is full against, and whether `sz` bytes fit a ring whose head is `head`
// (k_cold_scan sizes a wave's reservation with them before it makes it)
DEV u64 spill_lagged_tail(const DS& d) {
  u64 tail = *d.spill_tail;
  for (u32 k = 0; k < SPILL_LAG; ++k) tail = d.spill_tail_lag[k] < tail ? d.spill_tail_lag[k] : tail;
  return tail;
}
DEV bool spill_fits(const DS& d, u64 head, u64 tail, u32 sz) {
  const u64 phys = head % d.spill_bytes;
  if (phys + sz > d.spill_bytes) head += d.spill_bytes - phys;
  return head + sz - tail <= d.spill_bytes;
}

// Cold bodies to host memory (host-driven, between steps, when the HBM log fills): one
// block per queue, one wave per ring entry whose body sits in the log below position
// `lim` -- the oldest part, which pins the log tail: the log is a ring, only its tail
// frees space -- skipping the first `hot` entries of a queue that has consumers (about to
// be delivered; a backlog without consumers moves from its head).
// The slot is copied into the spill ring (pinned host memory), then MsgEnt.log_off is
// switched with a CAS (a message in several queues moves once; a lost race leaves a
// never-live gap the spill tail passes).  Its log block loses the bytes, so the next
// step's final_step can advance the log tail.  Unacked deliveries stay in the log.
__global__ __launch_bounds__(256) void k_spill(DS d, u64 lim, u32 hot, unsigned long long* moved) {
  const u32 q = blockIdx.x;
  if (q >= d.q_max || d.spill_bytes == 0) return;
  spill_queue(d, q, lim, hot, 0, (u64*)moved);
}

// ============================================================================ cold store (between steps)
// Third body tier (MessageEntity.scala:174-186: idle bodies go to the store and are
// read back on demand).  Out: k_cold_pick lists spilled bodies of single-queue,
// non-persistent messages at least `hot` entries behind their queue's head; the host
// writes them from the pinned ring to the cold store; k_cold_commit switches each
// MsgEnt to COLD_BIT | store offset, frees its ring bytes and lowers q_cold_lim.
// Candidates are taken from the oldest part of the ring (slot position below `lim`, like
// k_spill's log limit): the ring is a FIFO, so only freeing its tail end makes room; a
// queue with consumers keeps its first `hot` entries resident.
// `lim` counts from the ring's tail; nothing is picked while the ring holds less than
// `min_used` bytes (the cold thread asks every 10 ms without reading the ring state)
__global__ __launch_bounds__(256) void k_cold_pick(DS d, u32 hot, u64 lim_rel, u64 min_used, ColdRec* out, u32 max_n,
                                                   u32* n_out, unsigned long long* bytes, u64 max_bytes) {
  const u32 q = blockIdx.x, lane = lane_id(), w = threadIdx.x >> 6;
  if (q >= d.q_max || !d.q_active[q] || d.spill_bytes == 0) return;
  if (*d.spill_head - *d.spill_tail < min_used) return;
  const u64 lim = *d.spill_tail + lim_rel;
  const u64 head = d.q_head[q], tail = d.q_tail[q], mask = d.q_ring_mask[q];
  const Desc* ring = d.ring + d.q_ring_off[q];
  const u64 skip = d.q_cons_n[q] ? hot : 0;
  // resume past the queue's cold prefix (cursor): a deep cold backlog is not walked again
  // at every call (it was: up to ~370 us between two steps, profiles/r5_coldprof/)
  __shared__ unsigned long long s_open;
  if (threadIdx.x == 0) s_open = ~0ull;
  __syncthreads();
  const u64 start0 = head + skip;
  u64 cur = d.q_cold_cur[q];
  if (cur < start0 || cur > tail) cur = start0;   // (the head passed it, or the slot was reset)
  u64 open = ~0ull;   // this wave's first entry that is not cold (or where it stopped)
  for (u64 b = cur + (u64)w * 64; b < tail; b += 256) {
    const u64 i = b + lane;
    bool want = false, cold = false;
    u32 msg = INVALID, sz = 0;
    u64 lo = 0;
    if (i < tail) {
      msg = ring[i & mask].msg;
      cold = msg == INVALID || msg >= d.msg_max;
      if (!cold) {
        const MsgEnt& m = d.msgs[msg];
        lo = m.log_off;
        sz = m.slot_bytes;
        cold = (lo & COLD_BIT) != 0;
        want = (lo & SPILL_BIT) && !(lo & COLD_BIT) && (lo & ~SPILL_BIT) < lim && m.refcnt == 1 &&
               !(m.flags & MF_PERSIST);
      }
    }
    const u64 nc = __ballot(i < tail && !cold);
    if (nc && open == ~0ull) open = b + (u64)(__ffsll((unsigned long long)nc) - 1);
    const u32 k = wave_reserve(n_out, want);
    bool ok = want && k < max_n;
    if (ok) ok = atomicAdd(bytes, (unsigned long long)sz) + sz <= max_bytes;
    if (want && k < max_n) {   // (a record of bytes 0 is skipped by the host)
      ColdRec r;
      r.msg = ok ? msg : INVALID; r.q = q; r.qpos = i; r.pos = lo & ~SPILL_BIT; r.cold = 0;
      r.bytes = ok ? sz : 0; r.pad = 0;
      out[k] = r;
    }
    if (__ballot(want && !ok)) {   // the batch is full
      if (b < open) open = b;
      break;
    }
  }
  if (lane == 0 && open != ~0ull) atomicMin(&s_open, (unsigned long long)open);
  __syncthreads();
  if (threadIdx.x == 0) d.q_cold_cur[q] = s_open == ~0ull ? tail : (u64)s_open;
}

__global__ void k_cold_commit(DS d, const ColdRec* recs, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ColdRec r = recs[i];
  if (!r.bytes || r.msg >= d.msg_max) return;
  // (picked a few steps ago by the cold thread: an entry delivered since then stays spilled)
  if (d.q_head[r.q] > r.qpos) return;
  MsgEnt& m = d.msgs[r.msg];
  const u64 expect = SPILL_BIT | r.pos;
  if (atomicCAS((unsigned long long*)&m.log_off, (unsigned long long)expect, (unsigned long long)(COLD_BIT | r.cold)) !=
      expect)
    return;
  spill_free(d, expect, r.bytes);
  atomicAdd((unsigned long long*)&d.cold_live[(r.cold >> COLD_SEG_SHIFT) % COLD_SEGS], (unsigned long long)r.bytes);
  atomicMin((unsigned long long*)&d.q_cold_lim[r.q], (unsigned long long)r.qpos);
}

// In: for every queue held at q_cold_lim, the cold entries among its next `window`
// positions get a slot in the spill ring (in queue order; the scan stops where the ring
// is full) and are listed for the host, which reads their bodies into those slots;
// k_cold_in then switches them back to SPILL_BIT and moves q_cold_lim past the scan
// (to ~0 when it reached the tail: entries behind the tail are never cold)
__global__ __launch_bounds__(64) void k_cold_scan(DS d, u32 window, ColdRec* out, u32 max_n, u32* n_out,
                                                  u64* scan_end) {
  const u32 q = blockIdx.x, lane = lane_id();
  if (q >= d.q_max) return;
  const u64 lim = d.q_cold_lim[q];
  if (lim == ~0ull) return;
  const u64 head = d.q_head[q], tail = d.q_tail[q], mask = d.q_ring_mask[q];
  const Desc* ring = d.ring + d.q_ring_off[q];
  const u64 start = lim > head ? lim : head;
  const u64 stop = tail < head + window ? tail : head + window;
  __shared__ u32 s_incl[64];
  u64 end = start;
  for (u64 b = start; b < stop; b += 64) {
    const u64 i = b + lane;
    u32 msg = INVALID, sz = 0;
    u64 lo = 0;
    bool cold = false;
    if (i < stop) {
      msg = ring[i & mask].msg;
      if (msg != INVALID && msg < d.msg_max) {
        lo = d.msgs[msg].log_off;
        sz = d.msgs[msg].slot_bytes;
        cold = (lo & COLD_BIT) != 0;
      }
    }
    // one ring reservation for the wave's cold bodies, in lane order: all of them, or the
    // longest prefix that the ring and the batch have room for (all-or-nothing could never
    // page in 64 cold bodies that together exceed the ring's free room: the queue stood still)
    u32 off = cold ? sz : 0;
    for (int o = 1; o < 64; o <<= 1) {
      const u32 y = __shfl_up(off, o, 64);
      if (lane >= (u32)o) off += y;
    }
    const u64 cm = __ballot(cold);
    const u32 nc = (u32)__popcll(cm);
    const u32 rank = (u32)__popcll(cm & lanemask_lt());   // this lane's place among the cold ones
    if (cold) s_incl[rank] = off;   // bytes of the first rank + 1 cold bodies
    off -= cold ? sz : 0;
    __syncthreads();   // (the block is this one wave; b and stop are uniform)
    u64 pos = 0;
    u32 nok = 0, k0 = 0;
    if (lane == 0 && nc) {
      k0 = atomicAdd(n_out, nc);
      nok = k0 < max_n ? (max_n - k0 < nc ? max_n - k0 : nc) : 0u;
      // the longest prefix the ring has room for now: room only shrinks with the size (the pad to
      // the wrap included), so a bisection over the prefix sums with the ring read once; another
      // queue's block may take room meanwhile, then the reservation steps down
      const u64 h0 = __hip_atomic_load(d.spill_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const u64 t0 = spill_lagged_tail(d);
      u32 fit = 0, over = nok + 1;   // fit bodies fit, over do not
      while (over - fit > 1) {
        const u32 mid = fit + (over - fit) / 2;
        if (spill_fits(d, h0, t0, s_incl[mid - 1])) fit = mid; else over = mid;
      }
      nok = fit;
      while (nok && !spill_reserve(d, s_incl[nok - 1], &pos)) --nok;
    }
    nok = (u32)__shfl((int)nok, 0);
    pos = shfl64(pos, 0);
    k0 = (u32)__shfl((int)k0, 0);
    const u32 k = k0 + rank;
    const bool ok = cold && rank < nok;
    // the reserved bytes count as live from here: steps that run before k_cold_in (the
    // cold thread reads the store meanwhile) must not move the ring's tail over them
    if (ok) atomicAdd((unsigned long long*)&d.spill_live[((pos + off) / d.log_block) % d.n_spill_blocks],
                      (unsigned long long)sz);
    if (cold && k < max_n) {   // (not ok: a record of bytes 0, skipped by the host)
      ColdRec r;
      r.msg = ok ? msg : INVALID; r.q = q; r.qpos = i; r.pos = ok ? pos + off : 0; r.cold = lo & ~COLD_BIT;
      r.bytes = ok ? sz : 0; r.pad = 0;
      out[k] = r;
    }
    if (nok < nc) {   // ring (or the batch) full: the scan ends at the first entry left out
      end = b + (u64)(__ffsll((unsigned long long)(cm & ~__ballot(ok))) - 1);
      break;
    }
    end = b + 64 < stop ? b + 64 : stop;
    __syncthreads();   // lane 0 has read s_incl before the next wave of entries overwrites it
  }
  if (lane == 0) scan_end[q] = end == tail ? ~0ull : end;
}

__global__ void k_cold_in(DS d, const ColdRec* recs, u32 n, const u64* scan_end) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const ColdRec r = recs[i];
    if (r.bytes && r.msg < d.msg_max) {
      // still the cold message the scan listed (not purged since): back to its ring slot;
      // else the slot's reservation is returned
      const unsigned long long expect = COLD_BIT | r.cold;
      if (atomicCAS((unsigned long long*)&d.msgs[r.msg].log_off, expect, (unsigned long long)(SPILL_BIT | r.pos)) ==
          expect)
        atomicAdd((unsigned long long*)&d.cold_live[(r.cold >> COLD_SEG_SHIFT) % COLD_SEGS],
                  (unsigned long long)(-(i64)r.bytes));
      else
        spill_free(d, SPILL_BIT | r.pos, r.bytes);
    }
  }
  if (i < d.q_max && scan_end[i] != 0) d.q_cold_lim[i] = scan_end[i];   // (0: not scanned)
}

// ============================================================================ asynchronous exchange
// Phase B of a sharded step waits here (one wave, ahead of its graph) until the exchange
// thread finished the exchange it imports: the thread writes the received counts, then the
// job's sequence number into host-mapped flag[0].  Bounded: after ~20 s the wave gives up
// and sets flag[1] (the exchange thread always releases its job, so only a lost thread
// would get there; the host reports it), so a stuck host can never wedge the queue.
// lim: s_memrealtime ticks (100 MHz) after which the job counts as lost (the host derives
// it from the exchange timeout); phase B then imports nothing -- its receive counts are
// zeroed here too (the host zeroed them before handing the job over; a job that finishes
// after the give-up must not have them imported), and the next exchange() call throws
__global__ __launch_bounds__(64) void k_xwait(const u32* flag, u32 seq, u32* gave_up, u64 lim, u32* xchg, u32 world) {
  const u64 t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
  while (true) {
    const u32 v = __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
    if ((int)(v - seq) >= 0) return;
    if (__builtin_amdgcn_s_memrealtime() - t0 > lim) {
      const u32 r = threadIdx.x;
      if (r < world && r < WORLD_MAX) {
        __hip_atomic_store(&xchg[XC_RECV_N + r], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&xchg[XC_RECV_B + r], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&xchg[XC_RECV_AN + r], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&xchg[XC_RECV_AB + r], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&xchg[XC_RACK_N + r], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      if (threadIdx.x == 0) __hip_atomic_store(gave_up, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __threadfence_system();
      return;
    }
    __builtin_amdgcn_s_sleep(32);
  }
}

// the cold thread's copy of a pick / scan: the listed records into host-mapped memory
__global__ void k_side_out(const ColdRec* recs, const u32* cnt, u32 max_n, u32* out, u32* out_cnt) {
  u32 n = *cnt;
  if (n > max_n) n = max_n;
  const u32 words = n * (u32)(sizeof(ColdRec) / 4);
  const u32* src = (const u32*)recs;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) out[i] = src[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) out_cnt[0] = n;
}

// ============================================================================ requeue (pre-step)
// run by k_dequeue (fused k_requeue): the block of a queue with requeued items gathers
// them, bitonic-sorts by queue position and pushes them back in front of the head with
// the redelivered flag (QueueEntity.scala:415-446); the last block compacts the rest.
// The sort holds REQ_BLK items: a queue with more of them in one step is pushed in passes
// over ranges of queue position, the highest range first (next to the head), so the
// queue's order holds for any count up to req_max.

// this queue's listed items with lo <= qpos < hi, counted; with `keep` the first REQ_BLK
// of them (in arrival order) are gathered into kpos / kidx
DEV u32 requeue_gather(const DS& d, u32 q, u32 n, u64 lo, u64 hi, bool keep, u64* kpos, u32* kidx, u32* cnt_p) {
  const u32 tid = threadIdx.x;
  if (tid == 0) *cnt_p = 0;
  __syncthreads();
  for (u32 i = tid; i < n; i += 256) {
    if (d.req[i].q != q) continue;
    const u64 p = d.req[i].qpos;
    if (p < lo || p >= hi) continue;
    const u32 k = atomicAdd(cnt_p, 1u);
    if (keep && k < REQ_BLK) { kpos[k] = p; kidx[k] = i; }
  }
  __syncthreads();
  const u32 c = *cnt_p;
  __syncthreads();
  return c;
}

// the m gathered items sorted by queue position; the first k of them written to ring
// positions base, base + 1, .. and taken off the list
// BL: the pushed entries' bytes go back into q_bytes (atomics: the block's waves; the queue's block
// reads the sum agent-scope once its requeue is done)
template <bool BL>
DEV void requeue_sort_push(const DS& d, u32 q, u64* kpos, u32* kidx, u32 m, u32 k, u64 base, u64 mask) {
  const u32 tid = threadIdx.x;
  u32 np2 = 1;
  while (np2 < m) np2 <<= 1;
  for (u32 i = m + tid; i < np2; i += 256) { kpos[i] = ~0ull; kidx[i] = INVALID; }
  __syncthreads();
  for (u32 sz = 2; sz <= np2; sz <<= 1) {
    for (u32 j = sz >> 1; j > 0; j >>= 1) {
      for (u32 i = tid; i < np2; i += 256) {
        u32 ij = i ^ j;
        if (ij > i) {
          bool up = (i & sz) == 0;
          if ((kpos[i] > kpos[ij]) == up) {
            u64 t = kpos[i]; kpos[i] = kpos[ij]; kpos[ij] = t;
            u32 x = kidx[i]; kidx[i] = kidx[ij]; kidx[ij] = x;
          }
        }
      }
      __syncthreads();
    }
  }
  u64 back = 0;
  for (u32 i = tid; i < k; i += 256) {
    const ReqItem r = d.req[kidx[i]];
    Desc ds;
    ds.msg = r.msg;
    ds.flags = 1;
    ds.expire_ms = r.expire_ms;
    d.ring[d.q_ring_off[q] + ((base + i) & mask)] = ds;
    // consumed (agent-coherent: the compacting block of another XCD reads it after the ticket)
    __hip_atomic_store(&d.req[kidx[i]].q, INVALID, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (BL) back += d.msgs[r.msg].body_len;
  }
  if (BL) {
    back = (u64)wave_sum64((i64)back);
    if (lane_id() == 0 && back) atomicAdd((unsigned long long*)&d.q_bytes[q], (unsigned long long)back);
  }
  __syncthreads();
}

template <bool BL>
DEV void requeue_queue(const DS& d, u32 q, u64* kpos, u32* kidx, u32* cnt_p) {
  const u32 tid = threadIdx.x;
  u32 n = *d.req_n;
  if (n > d.req_max) n = d.req_max;
  const u64 head = d.q_head[q], tail = d.q_tail[q];
  const u64 mask = d.q_ring_mask[q];
  const u64 freec = mask + 1 - (tail - head);
  const u32 total = requeue_gather(d, q, n, 0, ~0ull, true, kpos, kidx, cnt_p);
  u32 done = 0;
  if (total <= REQ_BLK) {
    done = total < freec ? total : (u32)freec;   // (no room for all: the lowest positions)
    requeue_sort_push<BL>(d, q, kpos, kidx, total, done, head - done, mask);
  } else {
    // the positions' bounds (kpos[0..1] as scratch: the gathers below rewrite them)
    if (tid == 0) { kpos[0] = ~0ull; kpos[1] = 0; }
    __syncthreads();
    for (u32 i = tid; i < n; i += 256) {
      if (d.req[i].q != q) continue;
      atomicMin((unsigned long long*)&kpos[0], (unsigned long long)d.req[i].qpos);
      atomicMax((unsigned long long*)&kpos[1], (unsigned long long)d.req[i].qpos);
    }
    __syncthreads();
    const u64 lo0 = kpos[0];
    u64 hi = kpos[1] + 1;
    __syncthreads();
    if (total > freec) {   // no room for all: the items below the largest bound that fits
      u64 g = lo0, b = hi;   // count[lo0, g) <= freec < count[lo0, b)
      while (b - g > 1) {
        const u64 mid = g + (b - g) / 2;
        if (requeue_gather(d, q, n, lo0, mid, false, kpos, kidx, cnt_p) <= freec) g = mid;
        else b = mid;
      }
      hi = g;
    }
    // passes from the head downwards: the widest range [lo, hi) of at most REQ_BLK items
    // (bisected by count); every loop condition is block-uniform
    while (hi > lo0) {
      u64 lo = lo0;
      if (requeue_gather(d, q, n, lo, hi, false, kpos, kidx, cnt_p) > REQ_BLK) {
        u64 b = lo0, g = hi;   // count[g, hi) <= REQ_BLK < count[b, hi)
        while (g - b > 1) {
          const u64 mid = b + (g - b) / 2;
          if (requeue_gather(d, q, n, mid, hi, false, kpos, kidx, cnt_p) <= REQ_BLK) g = mid;
          else b = mid;
        }
        lo = g;
      }
      if (lo == hi) break;   // more than REQ_BLK items at one position: they stay listed
      const u32 m = requeue_gather(d, q, n, lo, hi, true, kpos, kidx, cnt_p);
      requeue_sort_push<BL>(d, q, kpos, kidx, m, m, head - done - m, mask);
      done += m;
      hi = lo;
    }
  }
  if (tid == 0) {
    d.q_head[q] = head - done;
    d.req_q_n[q] -= done;
    // the tier cursors say "everything before me is tiered": the entries that came back in
    // front of them are not (unacked deliveries stay where they are), so the walks restart there
    if (done && d.spill_bytes) {
      if (d.q_spill_cur[q] > head - done) d.q_spill_cur[q] = head - done;
      if (d.q_cold_cur[q] > head - done) d.q_cold_cur[q] = head - done;
    }
  }
}

DEV void requeue_compact(const DS& d) {
  // one block of 256: compact the remaining (unconsumed) requeue items
  __shared__ u32 lds[256 / 64 + 1];
  u32 n = *d.req_n;
  if (n == 0) return;
  if (n > d.req_max) n = d.req_max;
  u32 run = 0;
  for (u32 b0 = 0; b0 < n; b0 += 256) {
    u32 i = b0 + threadIdx.x;
    // (fields as scalars: an aggregate copy across the scan's barriers was lowered to scratch)
    u32 rq = INVALID, rm = 0;
    u64 rp = 0;
    i64 re = 0;
    if (i < n) { rq = d.req[i].q; rm = d.req[i].msg; rp = d.req[i].qpos; re = d.req[i].expire_ms; }
    u32 keep = (i < n && rq != INVALID) ? 1 : 0;
    u32 all;
    u32 off = block_scan<256>(keep, lds, all);
    __syncthreads();
    if (keep) {   // run + off <= i: safe forward compaction
      ReqItem& o = d.req[run + off];
      o.q = rq; o.msg = rm; o.qpos = rp; o.expire_ms = re;
    }
    __syncthreads();
    run += all;
  }
  if (threadIdx.x == 0) *d.req_n = run;
}
