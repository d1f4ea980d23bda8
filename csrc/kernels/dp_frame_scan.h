// Data plane: K1 frame scan.
#pragma once
#include "dp_state.h"
#include "dp_util.h"

// ============================================================================ K1 frame scan
struct FInfo { u32 type, ch, size; bool complete, valid_hdr; };

DEV FInfo frame_at(const u8* b, u32 p, u32 L, u32 fmax) {
  FInfo f;
  f.complete = false;
  f.valid_hdr = false;
  f.type = 0; f.ch = 0; f.size = 0;
  if (p + 7 > L) return f;  // partial header
  f.type = b[p];
  f.ch = be16(b + p + 1);
  f.size = be32(b + p + 3);
  bool tok = f.type == 1 || f.type == 2 || f.type == 3 || f.type == 8;
  bool sok = fmax == 0 || f.size + 8 <= fmax;
  f.valid_hdr = tok && sok;
  if (f.valid_hdr && (u64)p + 8 + f.size <= L) f.complete = (b[p + 7 + f.size] == 0xCE);
  return f;
}

DEV i32 chan_lookup(const DS& d, u32 conn, u32 ch) {
  const u32* m = d.chmap + (u64)conn * d.chmap_size;
  u32 mask = d.chmap_size - 1;
  u32 h = (ch * 0x9E3779B1u) >> 7;
  for (u32 i = 0; i < d.chmap_size; ++i) {
    u32 e = m[(h + i) & mask];
    if (e == 0) return -1;
    if ((e >> 16) == ch && (e & 0x8000u)) return (i32)(conn * d.chpc + (e & 0x7fffu));
  }
  return -1;
}

// candidate screen: one u16 mask per 16 work bytes; bit j set when byte j looks like a
// frame header (type 1/2/3/8, size within the broker frame-max).  Reads 32 bytes (the
// header of a frame starting at byte 15 ends in the next word); segments are padded
// by >= 32 bytes in the work buffer
// SWAR: 0x80 in every byte of v that is zero (exact per byte: no borrow between bytes)
DEV u32 zero_bytes(u32 v) { return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu); }
// bits 0..3 = bytes 0..3 of v hold a frame type (1, 2, 3 or 8); the multiply gathers the
// four 0x80 flags (bits 0, 8, 16, 24 after the shift) into bits 21..24 without carries
DEV u32 type_nibble(u32 v) {
  const u32 h = (zero_bytes(v & 0xFCFCFCFCu) & ~zero_bytes(v)) | zero_bytes(v ^ 0x08080808u);
  return (((h >> 7) * 0x00204081u) >> 21) & 0xFu;
}
DEV u32 cand_bits(uint4 A, uint4 B, u32 fm) {
  const u32 w[6] = {A.x, A.y, A.z, A.w, B.x, B.y};
  u32 m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u32 h = type_nibble(w[i]);
    // the rare type hits: big-endian size from bytes k+3..k+6 of the 4i-byte window
    while (h) {
      const u32 k = __ffs(h) - 1;
      h &= h - 1;
      const u32 v = k == 0 ? __builtin_amdgcn_alignbyte(w[i + 1], w[i], 3)
                           : __builtin_amdgcn_alignbyte(w[i + 2], w[i + 1], k - 1);
      const u32 sz = __builtin_bswap32(v);
      if (fm == 0 || sz <= fm - 8) m |= 1u << (4 * i + k);
    }
  }
  return m;
}
DEV u32 cand_word(const u8* w16, u32 fm) {
  const uint4* q = (const uint4*)w16;
  return cand_bits(q[0], q[1], fm);
}

#define FS_MARK(k) \
  do { if (tid == 0 && d.dbg) d.dbg[(u64)s * 16 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
constexpr u32 FS_AM_MAX = 8192;  // 128 KB segment; 16 KB of LDS
// Segments up to FS_STAGE bytes (the screen's 32-byte read-ahead included) are copied
// into LDS by the screen pass itself, and every later phase reads the segment's bytes
// from LDS instead of HBM (frame headers, method ids, body sizes, control bytes: ~15
// dependent global round trips per segment before).  The block's LDS is one pool carved
// per segment: staged segments hold up to FS_CAND_STAGED candidates next to the 72 KB
// stage, other segments CAND_MAX candidates (a 128 KB segment of 1-byte messages)
constexpr u32 FS_STAGE = 72u << 10;
constexpr u32 FS_CAND_STAGED = 6144;
constexpr u32 FS_RUNS = 1024;   // run records of the chain (phase c), kept at the top of wend
static_assert(CAND_MAX < (1u << 16) && FS_CAND_STAGED > 2 * FS_RUNS, "k_frame_scan candidate limits");
// candidate arrays: wend + cpos (u32), chain / screen mask (u16), csucc (i16), claim (u8)
constexpr u32 fs_cand_bytes(u32 cmax, u32 amw) { return cmax * 4 * 2 + (cmax > amw ? cmax : amw) * 2 + cmax * 2 + cmax; }
constexpr u32 FS_POOL_STAGED = FS_STAGE + fs_cand_bytes(FS_CAND_STAGED, FS_STAGE / 16);
constexpr u32 FS_POOL_FULL = fs_cand_bytes(CAND_MAX, FS_AM_MAX);
constexpr u32 FS_POOL = ((FS_POOL_STAGED > FS_POOL_FULL ? FS_POOL_STAGED : FS_POOL_FULL) + 15) & ~15u;
static_assert(FS_POOL <= 156u << 10, "k_frame_scan LDS pool");
// one block of FS_NT threads per segment: 16 waves (4 per SIMD) hide the screen's
// dependent integer chains, which one wave per SIMD could not
#define FS_NT 1024
// a content publish whose whole command (method + header + body frames) cannot fit the
// connection's carry: the host assembles it (FE_CTRL of its method + header frames; the
// body is read on the host and enqueued as an MF_HOSTPUB record)
DEV bool big_publish(const DS& d, u32 msize, u32 hsize, u64 bsz, u32 fmax) {
  const u64 fb = fmax > 8 ? fmax - 8 : 0;
  const u64 nb = bsz == 0 ? 0 : (fb ? (bsz + fb - 1) / fb : 1);
  return (u64)msize + 8 + hsize + 8 + bsz + 8 * nb > d.carry_cap;
}

// bytes [sh, sh + 16) of the 32 bytes a:b (sh 0..15): a two-level word barrel shift (by 2
// words, then 1 -- named registers and selects: an indexed word array here was lowered to
// a scratch-memory table, 48 bytes per lane), then four dword funnel shifts
DEV uint4 shift_pair(uint4 a, uint4 b, u32 sh) {
  const u32 q = sh >> 2, r = sh & 3;
  const bool q2 = (q & 2) != 0, q1 = (q & 1) != 0;
  const u32 s0 = q2 ? a.z : a.x, s1 = q2 ? a.w : a.y, s2 = q2 ? b.x : a.z;
  const u32 s3 = q2 ? b.y : a.w, s4 = q2 ? b.z : b.x, s5 = q2 ? b.w : b.y;
  const u32 w0 = q1 ? s1 : s0, w1 = q1 ? s2 : s1, w2 = q1 ? s3 : s2, w3 = q1 ? s4 : s3, w4 = q1 ? s5 : s4;
  if (!r) return make_uint4(w0, w1, w2, w3);
  return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, r), __builtin_amdgcn_alignbyte(w2, w1, r),
                    __builtin_amdgcn_alignbyte(w3, w2, r), __builtin_amdgcn_alignbyte(w4, w3, r));
}
// word c (bytes [16c, 16c + 16)) of a segment = the connection's carry (cl bytes, C
// 16-aligned) then its new ingress bytes (N 16-aligned; reading up to 32 bytes past them
// stays inside the ingress slot's slack); bytes past the segment are don't-care
DEV uint4 seg_word(const u8* C, u32 cl, const u8* N, u32 c) {
  const u32 b0 = c * 16;
  if (b0 + 16 <= cl) return *(const uint4*)(C + b0);
  if (b0 >= cl) {
    const u32 o = b0 - cl, k = o >> 4, sh = o & 15;
    const uint4 a = ((const uint4*)N)[k];
    return sh ? shift_pair(a, ((const uint4*)N)[k + 1], sh) : a;
  }
  u32 v[4] = {0, 0, 0, 0};   // the word holding the carry's end and the new bytes' start
#pragma unroll
  for (u32 j = 0; j < 16; ++j) {
    const u32 i = b0 + j;
    const u32 x = i < cl ? C[i] : N[i - cl];
    v[j >> 2] |= x << (8 * (j & 3));
  }
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// Basic.Get the step can serve itself: a named queue of the connection's vhost (the default
// exchange's direct binding of that name), owned by this rank, not another connection's
// exclusive queue.  An empty name (the channel's last declared queue) and every error case
// go to the host.  Method args at b + p + 7: class, method, ticket, queue shortstr, bits.
DEV bool dget_resolve(const DS& d, u32 conn, const u8* b, u32 p, u32 size, u32& q, u32& noack) {
  if (size < 8) return false;
  const u32 a = p + 7 + 6, n = b[a], end = p + 7 + size;
  if (n == 0 || a + 1 + n + 1 > end) return false;
  const u8* name = b + a + 1;
  const u32 vh = d.conn_vhost[conn];
  const u64 hk = exch_hash(vh, name, 0);   // the vhost's default exchange ("")
  i32 xs = -1;
  for (u32 j = 0; j <= d.xhash_mask; ++j) {
    const u32 slot = (u32)(hk + j) & d.xhash_mask;
    const i32 v = d.x_hval[slot];
    if (v < 0) break;
    if (d.x_hkey[slot] == hk) { xs = v; break; }
  }
  if (xs < 0 || d.x_type[xs] != EX_DIRECT) return false;
  const u64 k = fnv1a64_dev(name, n) ^ (u64(xs) * 0x9E3779B97F4A7C15ULL);
  for (u32 j = 0; j <= d.dhash_mask; ++j) {
    const u32 s = (u32)(k + j) & d.dhash_mask;
    const i32 ex = d.d_exch[s];
    if (ex < 0) return false;
    if (ex == xs && d.d_key[s] == k && word_eq(d.kpool + d.d_kb_off[s], d.d_kb_len[s], name, n)) {
      if (d.d_q_n[s] != 1) return false;
      const u32 qq = d.d_q[d.d_q_off[s]];
      const u32 ex_owner = d.q_excl[qq];
      if (!d.q_active[qq] || d.q_owner[qq] != d.my_rank || (ex_owner && ex_owner != conn + 1)) return false;
      q = qq;
      noack = b[a + 1 + n] & 1u;
      return true;
    }
  }
  return false;
}

// a segment's descriptor and the connection state its scan starts from: nothing of the
// ingress slot, so a block loads its first segment's before it waits for the payload copy
struct FsHead { u32 conn, L, seg_len, src, fmax; };
DEV FsHead fs_head(const DS& d, const u32 s) {
  FsHead h;
  h.conn = d.segs[s].conn;
  h.L = d.seg_total[s];
  h.seg_len = d.segs[s].len;
  h.src = d.segs[s].src;
  h.fmax = d.conn_frame_max[h.conn];
  return h;
}

DEV void frame_scan_seg(const DS& d, const u32 s, const FsHead hd) {
  __shared__ uint4 fs_pool[FS_POOL / 16];
  __shared__ u32 sc[FS_NT / 64 + 1];
  __shared__ u32 sh_m, sh_over, sh_ok, sh_nf, sh_stop, sh_brk;
  __shared__ u32 sh_cmd_base, sh_frag_base, sh_ncmd;
  __shared__ u32 sh_get0, sh_gch, sh_gq, sh_gna, sh_gbase;   // Basic.Get: the segment's first, its key
  __shared__ u32 sh_split;   // split mode: bytes [0, sh_split) are in the work buffer

  const u32 tid = threadIdx.x;
  const u32 conn = hd.conn;
  const u32 L = hd.L;
  const u32 seg_len = hd.seg_len, seg_cl = L - seg_len, src = hd.src;
  // the step's new bytes are read where their H2D put them: the ingress slots follow the
  // work buffers in one allocation, so a u32 offset from d.work reaches them, and every
  // later reader (decode, route-store, returns, gets) takes a frame's bytes from there.  A
  // segment with no carry is scanned in place (nothing goes to the work buffer); one with a
  // carry is staged in LDS by the screen and only its head -- the carry and the frame that
  // straddles into the new bytes -- is written to the work buffer (split mode, OFF below):
  // the work copy of the step's bytes is gone.  Single GPU (sharded steps read imports
  // beside the work buffer).
  const u64 ing_rel = (u64)d.in->ingress - (u64)d.work;
  const bool ing_ok = d.scan_inplace && d.world == 1 && (u64)d.in->ingress > (u64)d.work && ing_rel + src + L + 64 < (1ull << 32) &&
                      d.tot[TS_WORK_USED] <= d.work_cap;
  const bool inplace = ing_ok && seg_cl == 0 && L > 0;
  const u32 wbase = inplace ? (u32)(ing_rel + src) : d.seg_start[s];
  const u8* const bg = d.work + wbase;   // the segment in HBM: the work buffer or its ingress slot
  const u8* b = bg;                      // switched to the LDS stage after the screen
  // the pool for this segment: [stage] wend cpos chain/amask csucc claim
  const u32 nm16 = (L + 15) >> 4;
  const bool staged = nm16 * 16 + 32 <= FS_STAGE;
  const u32 cmax = staged ? FS_CAND_STAGED : CAND_MAX;
  u8* const pool = (u8*)fs_pool;
  uint4* const fs_stage = fs_pool;
  // per accepted candidate: its frame end | complete << 31 (phase b reuses it instead of
  // re-reading the header); ~0u = recompute
  u32* const wend = (u32*)(pool + (staged ? FS_STAGE : 0u));
  u32* const cpos = wend + cmax;
  // chain (first written in phase c) aliases amask (used only in phase a, which ends on a
  // __syncthreads)
  u16* const chain_am = (u16*)(cpos + cmax);
  u16* const chain = chain_am;
  u16* const amask = chain_am;
  int16_t* const csucc = (int16_t*)(chain_am + (staged ? FS_CAND_STAGED : (CAND_MAX > FS_AM_MAX ? CAND_MAX : FS_AM_MAX)));
  u8* const claim = (u8*)(csucc + cmax);
  const u32 fmax = hd.fmax;
  FS_MARK(15);
  const u8* const seg_C = d.carry + (u64)conn * d.carry_cap;
  const u8* const seg_N = (const u8*)d.in->ingress + src;
  // the common segment is copied into the work buffer by the screen pass itself: one read
  // of the sources, the work copy, the LDS stage and the candidate mask from the same
  // registers (was: a copy pass, then the screen re-reading the copy)
  const bool fit = d.tot[TS_WORK_USED] <= d.work_cap;
  const bool fuse = fit && !inplace && L > 0 && ((L + 15) >> 4) <= FS_AM_MAX && !d.conn_paused[conn];
  const bool split = fuse && staged && ing_ok;   // (the screen then leaves the work buffer alone)
  if (fit && !fuse && !inplace) {
    // the segment into the work buffer (fused k_stage copy): the connection's carry, then
    // its new ingress bytes.  k_decode / k_route_store read publishes from there
    u8* const dst = d.work + wbase;
    if (seg_cl) block_copy(dst, seg_C, seg_cl, tid, FS_NT);
    if (seg_len) block_copy(dst + seg_cl, seg_N, seg_len, tid, FS_NT);
  }
  __threadfence_block();
  __syncthreads();
  SegOut so;
  so.conn = conn; so.status = 0; so.consumed = 0; so.carry = L; so.ncmds = 0; so.err_off = 0;
  so.pad[0] = so.pad[1] = 0;

  if (d.conn_paused[conn]) {
    // hold everything; write carry back (k_stage already appended new bytes)
    if (L > d.carry_cap) { so.status = SS_TOO_LARGE; so.carry = 0; }
    else block_copy(d.carry + (u64)conn * d.carry_cap, b, L, tid, FS_NT);
    if (tid == 0) {
      so.status |= SS_PAUSED;
      d.carry_len[conn] = so.carry;
      d.seg_out[s] = so;
      d.seg_cmd_base[s] = INVALID;
      d.seg_npub[s] = 0;
      d.seg_nack[s] = 0;
    }
    return;
  }
  if (L == 0) {
    if (tid == 0) {
      d.carry_len[conn] = 0; d.seg_out[s] = so; d.seg_cmd_base[s] = INVALID; d.seg_npub[s] = 0; d.seg_nack[s] = 0;
    }
    return;
  }
  if (tid == 0) { sh_m = 0; sh_over = 0; }
  __syncthreads();

  FS_MARK(0);
  // ---- (a) candidates: screen the segment (one mask bit per byte that looks like a frame
  // header), validate them against the connection's frame-max / end marker, append the
  // trailing positions that can only hold a partial header.  cpos = accepted positions in
  // order; wend[i] = candidate i's frame end | complete << 31 (~0u: phase b re-reads it)
  {
    const u32 nm = (L + 15) >> 4;
    const u32 per = (nm + FS_NT - 1) / FS_NT;
    const u32 c0 = tid * per;
    const u32 c1 = c0 + per < nm ? c0 + per : nm;
    const u32 lim = L >= 7 ? L - 6 : 0;   // full-header positions are p < lim
    const bool use_am = nm <= FS_AM_MAX;
    const u32 fmg = d.frame_max_global;
    if (use_am) {   // candidate screen of the segment into LDS (fused k_cand), coalesced reads
      const uint4* W = (const uint4*)bg;   // 16-aligned; >= 32 bytes of padding after the segment
      uint4* const WD = (uint4*)(d.work + wbase);
      // every word is read from memory once: a lane's next word (the screen looks 16 bytes
      // ahead) is its neighbour lane's word, the wave's last lane reads it itself -- all 256
      // segment blocks screen at once, so the double read made this phase HBM-bound
      const u32 ln = lane_id();
      // (wave-uniform trip count: every lane of a wave takes part in the shuffles)
      for (u32 cb = tid - ln; cb < nm; cb += FS_NT * 4) {
        const u32 cc = cb + ln;
        uint4 x[4], y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // every load of the batch in flight before any use
          const u32 c = cc + k * FS_NT;   // (c == nm: the word after the segment, read as slack)
          x[k] = make_uint4(0, 0, 0, 0);
          y[k] = make_uint4(0, 0, 0, 0);
          if (c <= nm) x[k] = fuse ? seg_word(seg_C, seg_cl, seg_N, c) : W[c];
          if (ln == 63 && c < nm) y[k] = fuse ? seg_word(seg_C, seg_cl, seg_N, c + 1) : W[c + 1];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint4 nx = make_uint4(__shfl_down(x[k].x, 1), __shfl_down(x[k].y, 1), __shfl_down(x[k].z, 1),
                                      __shfl_down(x[k].w, 1));
          if (ln != 63) y[k] = nx;
          const u32 c = cc + k * FS_NT;
          if (c < nm) {
            amask[c] = (u16)cand_bits(x[k], y[k], fmg);
            if (staged) fs_stage[c] = x[k];
            if (fuse && !split) WD[c] = x[k];
          }
        }
      }
      if (fuse && !staged) __threadfence_block();   // the later phases read the work copy
      if (staged && tid < 2) fs_stage[nm + tid] = make_uint4(0, 0, 0, 0);   // the screen's read-ahead
      __syncthreads();
      if (staged) b = (const u8*)fs_stage;
    }
    FS_MARK(12);
    // raw candidates per thread (its words are contiguous: the scan keeps position order)
    u32 rc = 0;
    if (use_am)
      for (u32 c = c0; c < c1; ++c) {
        u32 mk = amask[c];
        if (c * 16 + 16 > lim) mk &= lim > c * 16 ? (1u << (lim - c * 16)) - 1u : 0u;
        rc += __popc(mk);
      }
    u32 rtot;
    u32 roff = block_scan<FS_NT>(rc, sc, rtot);
    FS_MARK(13);
    u32 tot = 0;
    if (use_am && rtot <= cmax) {
      // every raw candidate validated in parallel (one thread each), then compacted in
      // place chunk by chunk: accepted entries only move left, after the chunk was read
      for (u32 c = c0; c < c1; ++c) {
        u32 mk = amask[c];
        while (mk) {
          const u32 j = __ffs(mk) - 1;
          mk &= mk - 1;
          const u32 p = c * 16 + j;
          if (p >= lim) break;
          cpos[roff++] = p;
        }
      }
      __syncthreads();
      FS_MARK(14);
      for (u32 k0 = 0; k0 < rtot; k0 += FS_NT) {
        const u32 i = k0 + tid;
        bool ok = false;
        u32 p = 0, we = ~0u;
        if (i < rtot) {
          p = cpos[i];
          const FInfo f = frame_at(b, p, L, fmax);
          ok = f.valid_hdr && (f.complete || (u64)p + 8 + f.size > L);
          const u64 e64 = (u64)p + 8 + f.size;
          we = e64 < 0x7fffffffull ? ((f.complete ? 0x80000000u : 0u) | (u32)e64) : ~0u;
        }
        u32 all;
        const u32 o = block_scan<FS_NT>(ok ? 1u : 0u, sc, all);
        if (ok) { cpos[tot + o] = p; wend[tot + o] = we; }
        tot += all;
      }
    } else {
      // very long segment (no LDS mask) or more raw candidates than cmax: each
      // thread validates its own words, twice (count, then emit)
      u32 cnt = 0;
      for (u32 c = c0; c < c1; ++c) {
        u32 mk = use_am ? (u32)amask[c] : cand_word(b + c * 16, fmg);
        u32 acc = 0;
        while (mk) {
          u32 j = __ffs(mk) - 1;
          mk &= mk - 1;
          u32 p = c * 16 + j;
          if (p >= lim) break;
          FInfo f = frame_at(b, p, L, fmax);
          if (f.valid_hdr && (f.complete || (u64)p + 8 + f.size > L)) { ++cnt; acc |= 1u << j; }
        }
        if (use_am) amask[c] = (u16)acc;
      }
      u32 off = block_scan<FS_NT>(cnt, sc, tot);
      for (u32 c = c0; c < c1; ++c) {
        u32 mk = use_am ? (u32)amask[c] : cand_word(b + c * 16, fmg);
        while (mk) {
          u32 j = __ffs(mk) - 1;
          mk &= mk - 1;
          u32 p = c * 16 + j;
          if (p >= lim) break;
          bool acc = use_am;
          if (!use_am) {
            FInfo f = frame_at(b, p, L, fmax);
            acc = f.valid_hdr && (f.complete || (u64)p + 8 + f.size > L);
          }
          if (acc) {
            if (off < cmax) { cpos[off] = p; wend[off] = ~0u; }
            ++off;
          }
        }
      }
    }
    __syncthreads();
    if (tid == 0) {
      u32 nmc = tot;
      for (u32 p = lim; p < L; ++p) {
        if (nmc < cmax) { cpos[nmc] = p; wend[nmc] = ~0u; }
        ++nmc;
      }
      if (nmc > cmax) {
        // more accepted candidates than slots: header lookalikes inside bodies, or that many
        // frames.  A list cut at cmax may end between a frame and its successor, and the chain
        // with it, however little of the segment was real frames.  The list becomes the frames
        // themselves, walked from byte 0 (at most cmax steps, each past a checked header);
        // phases (b) and (c) then find every successor next in line.  over = the walk itself
        // ran out of slots: whole frames follow the last one listed
        u32 n = 0;
        u64 p = 0;
        bool cut = false;
        while (p < L) {
          if (n == cmax) { cut = true; break; }
          const FInfo f = frame_at(b, (u32)p, L, fmax);
          const bool ok = p + 7 > L || (f.valid_hdr && (f.complete || p + 8 + f.size > L));
          if (!ok) break;   // a broken frame: phase (b) finds no successor for the one before it
          cpos[n] = (u32)p;
          wend[n] = ~0u;
          ++n;
          if (!f.complete) break;
          p += 8 + (u64)f.size;
        }
        sh_over = cut ? 1u : 0u;
        nmc = n;
      }
      sh_m = nmc;
    }
    __syncthreads();
  }
  FS_MARK(1);
  const u32 m = sh_m;
  const bool over = sh_over != 0;

  // ---- (b) successor of every candidate (-1 exact end, -2 partial/unknown, -3 broken)
  for (u32 i = tid; i < m; i += FS_NT) {
    u32 p = cpos[i];
    bool complete;
    u32 e;
    const u32 we = wend[i];
    if (we != ~0u) {
      complete = (we >> 31) != 0;
      e = we & 0x7fffffffu;
    } else {
      FInfo f = frame_at(b, p, L, fmax);
      complete = f.complete;
      e = p + 8 + f.size;
    }
    i32 sx;
    if (!complete) sx = -2;
    else {
      if (e == L) sx = -1;
      else {
        u32 lo = i + 1, hi = m;  // successor lies strictly after i
        while (lo < hi) { u32 mid = (lo + hi) >> 1; if (cpos[mid] < e) lo = mid + 1; else hi = mid; }
        if (lo < m && cpos[lo] == e) sx = (i32)lo;
        else sx = (over && e > cpos[m - 1]) ? -2 : -3;
      }
    }
    csucc[i] = (int16_t)sx;
  }
  FS_MARK(2);
  // ---- (c) chain.  A failure is a candidate whose successor is not the next candidate;
  // between failures the chain runs through consecutive candidates.  The failures are
  // compacted in order (into wend, dead after (b)), then one thread walks failure to
  // failure -- one step per jump over false candidates (e.g. timestamp bytes inside a
  // header that look like a frame running past the segment end), not one per frame --
  // recording runs, which all threads expand into chain[].  A single run starting at 0
  // is the implicit chain (frame f = candidate f)
  const u32 FS_FAIL_MAX = cmax - 2 * FS_RUNS;
  __syncthreads();   // csucc / wend of (b) complete
  FS_MARK(9);
  {
    const u32 per = (m + FS_NT - 1) / FS_NT;
    const u32 i0 = tid * per < m ? tid * per : m;
    const u32 i1 = i0 + per < m ? i0 + per : m;
    u32 nfl = 0;
    for (u32 i = i0; i < i1; ++i) nfl += csucc[i] != (i32)(i + 1);
    u32 tfl;
    u32 o = block_scan<FS_NT>(nfl, sc, tfl);
    for (u32 i = i0; i < i1; ++i)
      if (csucc[i] != (i32)(i + 1) && o < FS_FAIL_MAX) wend[o++] = i;
    __syncthreads();
    // per failure x (candidate F[x] = wend[x]) with a successor: the first failure at or
    // after that successor, in parallel (binary search over F); kept in chain[] (free
    // until the expansion below), 0xFFFF = the chain ends at this failure
    if (tfl <= FS_FAIL_MAX)
      for (u32 x = tid; x < tfl; x += FS_NT) {
        const i32 sx = csucc[wend[x]];
        u32 nx = 0xFFFFu;
        if (sx >= 0) {
          u32 lo = x + 1, hi = tfl;   // successors lie after the failure
          while (lo < hi) { u32 mid = (lo + hi) >> 1; if (wend[mid] < (u32)sx) lo = mid + 1; else hi = mid; }
          nx = lo;   // < tfl: the last candidate is a failure
        }
        chain[x] = (u16)nx;
      }
    __syncthreads();
    FS_MARK(10);
    if (tid == 0) {
      u32 nf = 0, brk = 0, nrun = 0;
      if (m == 0 || cpos[0] != 0) {
        brk = 1;  // first bytes are not a frame header
      } else if (tfl <= FS_FAIL_MAX) {
        // failure to failure: the run [i, F[x]], then the run from F[x]'s successor
        u32 i = 0, x = 0;
        while (true) {
          const u32 k = wend[x], nx = chain[x];
          if (nrun < FS_RUNS) { wend[FS_FAIL_MAX + 2 * nrun] = i; wend[FS_FAIL_MAX + 2 * nrun + 1] = nf; }
          ++nrun;
          nf += k - i + 1;
          if (nx == 0xFFFFu) { brk = csucc[k] == -3; break; }
          i = (u32)csucc[k];
          x = nx;
        }
      }
      if (m != 0 && cpos[0] == 0 && (tfl > FS_FAIL_MAX || nrun > FS_RUNS)) {
        nf = 0; brk = 0; nrun = FS_RUNS + 1;   // pathological: serial walk
        i32 i = 0;
        while (true) {
          chain[nf++] = (u16)i;
          i32 sx = csucc[i];
          if (sx >= 0) { i = sx; continue; }
          if (sx == -3) brk = 1;
          break;
        }
      }
      sh_nf = nf;
      sh_brk = brk;
      sh_ok = nrun;
    }
    __syncthreads();
    FS_MARK(11);
    const u32 nrun = sh_ok;
    if (nrun > 1 && nrun <= FS_RUNS) {
      for (u32 r = tid; r < nrun; r += FS_NT) {
        const u32 ci = wend[FS_FAIL_MAX + 2 * r], f0 = wend[FS_FAIL_MAX + 2 * r + 1];
        const u32 f1 = r + 1 < nrun ? wend[FS_FAIL_MAX + 2 * r + 3] : sh_nf;
        for (u32 f = f0; f < f1; ++f) chain[f] = (u16)(ci + (f - f0));
      }
    }
    __syncthreads();
  }
  FS_MARK(3);
  const u32 nf = sh_nf;
  const bool implicit_chain = sh_ok == 1;
#define CPOS(f) (cpos[implicit_chain ? (f) : chain[f]])

  // ---- (d) commands: each method frame walks its content frames
  for (u32 f = tid; f < nf; f += FS_NT) claim[f] = 0;
  if (tid == 0) { sh_stop = (nf << 3) | 7; sh_get0 = INVALID; }  // (frame << 3) | reason; 7 = none
  __syncthreads();
  // stop reasons: 0 = after control, 1 = incomplete, 2 = unexpected frame, 3 = frame error,
  // 4 = before a command that may not follow the segment's Basic.Gets in one step
  for (u32 f = tid; f < nf; f += FS_NT) {
    u32 p = CPOS(f);
    FInfo fi = frame_at(b, p, L, fmax);
    if (!fi.complete) {
      if (fi.type == 1 || fi.type == 8 || !fi.valid_hdr) atomicMin(&sh_stop, (f << 3) | 1);
      continue;
    }
    if (fi.type == 8) { claim[f] = 1; continue; }
    if (fi.type != 1) continue;
    claim[f] = 1;
    if (fi.size < 4) { atomicMin(&sh_stop, (f << 3) | 3); continue; }
    u32 cls = be16(b + p + 7), mid = be16(b + p + 9);
    bool content = (cls == 60 && mid == 40);
    bool data = (cls == 60 && (mid == 40 || mid == 80 || mid == 90 || mid == 120)) && fi.ch != 0 &&
                chan_lookup(d, conn, fi.ch) >= 0;
    if (cls == 60 && mid == 70 && fi.ch != 0 && chan_lookup(d, conn, fi.ch) >= 0) {
      u32 gq, gna;
      if (dget_resolve(d, conn, b, p, fi.size, gq, gna)) { atomicMin(&sh_get0, f); continue; }
    }
    if (!content) {
      if (!data) atomicMin(&sh_stop, ((f + 1) << 3) | 0);
      continue;
    }
    // header then bodies on the same channel
    u32 g = f + 1;
    if (g >= nf) { atomicMin(&sh_stop, (f << 3) | 1); continue; }
    u32 hp = CPOS(g);
    FInfo hi = frame_at(b, hp, L, fmax);
    if (!hi.complete) { atomicMin(&sh_stop, (f << 3) | 1); continue; }
    if (hi.type != 2 || hi.ch != fi.ch || hi.size < 14) { atomicMin(&sh_stop, (f << 3) | 2); continue; }
    claim[g] = 1;
    u64 bsz = be64(b + hp + 7 + 4);
    if (data && big_publish(d, fi.size, hi.size, bsz, fmax)) {   // host-assembled: stop after its header
      atomicMin(&sh_stop, ((g + 1) << 3) | 0);
      continue;
    }
    u64 got = 0;
    u32 e = g;
    bool bad = false, incomplete = false;
    while (got < bsz) {
      ++e;
      if (e >= nf) { incomplete = true; break; }
      u32 bp = CPOS(e);
      FInfo bi = frame_at(b, bp, L, fmax);
      if (!bi.complete) { incomplete = true; break; }
      if (bi.type != 3 || bi.ch != fi.ch) { atomicMin(&sh_stop, (f << 3) | 2); bad = true; break; }
      claim[e] = 1;
      got += bi.size;
      if (got > bsz) { atomicMin(&sh_stop, (f << 3) | 3); bad = true; break; }
    }
    if (incomplete) atomicMin(&sh_stop, (f << 3) | 1);
    (void)bad;
    if (!data) atomicMin(&sh_stop, ((e + 1) << 3) | 0);
  }
  __syncthreads();
  for (u32 f = tid; f < nf; f += FS_NT) {
    if (claim[f]) continue;
    FInfo fi = frame_at(b, CPOS(f), L, fmax);
    if (fi.complete) atomicMin(&sh_stop, (f << 3) | 2);
  }
  __syncthreads();
  if (sh_get0 != INVALID) {   // (block-uniform) the segment serves Basic.Gets in this step
    // they all ask the same (channel, queue, no-ack) -- any two then answer alike, whichever
    // is served first -- and nothing but such Gets follows the first in this step (an ack
    // after a Get may name its delivery tag, which the step assigns later); the rest of the
    // segment waits in the carry for the next step
    const u32 g0 = sh_get0;
    if (tid == g0 % FS_NT) {
      const u32 p = CPOS(g0);
      FInfo fi = frame_at(b, p, L, fmax);
      u32 gq = 0, gna = 0;
      dget_resolve(d, conn, b, p, fi.size, gq, gna);
      sh_gch = fi.ch; sh_gq = gq; sh_gna = gna;
    }
    __syncthreads();
    for (u32 f = g0 + 1 + tid; f < nf; f += FS_NT) {
      const u32 p = CPOS(f);
      if (b[p] != 1) continue;   // content and heartbeat frames go with their method / nothing
      FInfo fi = frame_at(b, p, L, fmax);
      bool same = false;
      if (fi.complete && fi.size >= 4 && be16(b + p + 7) == 60 && be16(b + p + 9) == 70 && fi.ch == sh_gch) {
        u32 gq, gna;
        same = dget_resolve(d, conn, b, p, fi.size, gq, gna) && gq == sh_gq && gna == sh_gna;
      }
      if (!same) atomicMin(&sh_stop, (f << 3) | 4);
    }
    __syncthreads();
  }
  FS_MARK(4);
  u32 stop = sh_stop;
  u32 kf = stop >> 3, reason = stop & 7;
  if (kf > nf) kf = nf;
  if (reason == 7 && sh_brk) { reason = 3; }  // chain ended on a broken frame

  // consumed bytes: up to frame kf (or the end of the chain)
  u32 consumed;
  if (kf < nf) consumed = CPOS(kf);
  else if (nf == 0) consumed = 0;
  else {
    u32 lp = CPOS(nf - 1);
    FInfo lf = frame_at(b, lp, L, fmax);
    consumed = lf.complete ? lp + 8 + lf.size : lp;
  }
  if (reason == 3 || reason == 2) {
    so.status |= (reason == 3) ? SS_FRAME_ERROR : SS_UNEXPECTED;
    so.err_off = consumed;
  }
  // the list ran out of slots and the scan stopped for want of frames, at the chain's end or
  // at a command whose frames run past it: the carry holds whole frames the next step must
  // see without waiting for new bytes (kf == 0: one command of more frames than slots)
  if (over && ((reason != 0 && kf == nf) || (reason == 1 && kf > 0))) so.status |= SS_OVERFLOW;
  if (reason == 4) so.status |= SS_OVERFLOW;   // the carry is re-presented to the next step

  // split mode: the work buffer gets the carry and the frame that runs from it into the new
  // bytes (frames start inside the carry only before that point); later frames are read from
  // the ingress slot
  if (split) {
    if (tid == 0) sh_split = seg_cl;
    __syncthreads();
    for (u32 f = tid; f < nf; f += FS_NT) {
      const u32 p = CPOS(f);
      if (p >= seg_cl) continue;
      const FInfo fi = frame_at(b, p, L, fmax);
      const u64 e = fi.complete ? (u64)p + 8 + fi.size : (u64)L;
      atomicMax(&sh_split, (u32)(e < L ? e : L));
    }
    __syncthreads();
    uint4* const WD = (uint4*)(d.work + wbase);
    const u32 nw = (sh_split + 15) >> 4;
    for (u32 w = tid; w < nw; w += FS_NT) WD[w] = fs_stage[w];
    __syncthreads();
  }
  const u32 sp = split ? sh_split : inplace ? 0u : L + 1u;
  // a frame's offset from d.work (frames lie wholly below sp or at / above it)
  auto OFF = [&](u32 pos) -> u32 { return pos < sp ? wbase + pos : (u32)(ing_rel + src + pos - seg_cl); };
  FS_MARK(5);
  // ---- (e) emit commands for method frames < kf
  u32 run = 0, frun = 0;
  if (tid == 0) { sh_cmd_base = INVALID; sh_ncmd = 0; }
  __syncthreads();
  // count first -- unless the commands fit one emit chunk (the common case): then the emit
  // pass reserves them itself, from the scans it runs anyway
  const bool one = kf <= FS_NT;   // (block-uniform)
  u32 my_cmds = 0, my_frags = 0;
  for (u32 f = tid; f < kf && !one; f += FS_NT) {
    u32 p = CPOS(f);
    if (b[p] != 1) continue;
    ++my_cmds;
    if (be16(b + p + 7) == 60 && be16(b + p + 9) == 40) {
      // frags: frames after header until the next method
      u32 e = f + 2;
      while (e < kf && b[CPOS(e)] == 3) { ++my_frags; ++e; }
    }
  }
  u32 tc = 0, tfr = 0;
  if (!one) {
    block_scan<FS_NT>(my_cmds, sc, tc);
    block_scan<FS_NT>(my_frags, sc, tfr);
  }
  // one uncontended atomicAdd per block (a CAS loop here serialises all blocks);
  // on overflow the reserved in-range slots are filled with CK_NONE and the whole
  // segment is carried to the next step
  if (!one && tid == 0) {
    u32 cb = tc ? atomicAdd(&d.ctr->n_cmds, tc) : 0;
    u32 fb = tfr ? atomicAdd(&d.ctr->n_frags, tfr) : 0;
    sh_frag_base = fb;
    sh_cmd_base = cb;
    sh_ncmd = (cb + tc > d.cmd_max || fb + tfr > d.frag_max) ? 1u : 0u;
  }
  __syncthreads();
  if (sh_ncmd && tc > 0) {
    u32 cb = sh_cmd_base;
    for (u32 i = cb + tid; i < cb + tc && i < d.cmd_max; i += FS_NT) {
      d.cmds[i].kind = CK_NONE;
      d.cmd_is_pub[i] = 0;
      d.cmd_is_ack[i] = 0;
    }
    if (tid == 0) sh_cmd_base = INVALID;
    __syncthreads();
  }
  if (sh_cmd_base == INVALID && tc > 0) {
    so.status |= SS_OVERFLOW;
    so.status &= ~(SS_FRAME_ERROR | SS_UNEXPECTED);
    consumed = 0;
    kf = 0;
    reason = 7;
  }
  FS_MARK(6);
  const i64 now = d.in->now_ms;
  u32 npub_run = 0, nack_run = 0;   // the segment's publishes / acks so far (their ordinals)
  for (u32 f0 = 0; f0 < kf; f0 += FS_NT) {
    u32 f = f0 + tid;
    u32 is_cmd = 0, nfr = 0;
    u32 p = 0;
    // every command's kind first: the publish / ack ordinals within the segment come out of
    // the same block scan as the command index (no grid-wide rank scan over the commands)
    Cmd c;
    FInfo fi;
    u32 cls = 0, mid = 0, hp = 0, gq = 0, gna = 0;
    FInfo hi;
    if (f < kf) {
      p = CPOS(f);
      if (b[p] == 1) {
        is_cmd = 1;
        if (be16(b + p + 7) == 60 && be16(b + p + 9) == 40) {
          u32 e = f + 2;
          while (e < kf && b[CPOS(e)] == 3) { ++nfr; ++e; }
        }
      }
    }
    if (is_cmd) {
      fi = frame_at(b, p, L, fmax);
      cls = be16(b + p + 7);
      mid = be16(b + p + 9);
      const i32 chs = fi.ch ? chan_lookup(d, conn, fi.ch) : -1;
      c.pad[0] = (u32)chs;
      if (cls == 60 && mid == 40 && chs >= 0) c.kind = CK_PUBLISH;
      else if (cls == 60 && mid == 70 && chs >= 0 && dget_resolve(d, conn, b, p, fi.size, gq, gna)) c.kind = CK_GET;
      else if (cls == 60 && mid == 80 && chs >= 0) c.kind = CK_ACK;
      else if (cls == 60 && mid == 90 && chs >= 0) c.kind = CK_REJECT;
      else if (cls == 60 && mid == 120 && chs >= 0) c.kind = CK_NACK;
      else c.kind = CK_CONTROL;
      if (c.kind != CK_CONTROL && c.kind != CK_GET && d.ch_tx[chs]) c.kind = CK_TXBUF;   // held until Tx.Commit
      if (cls == 60 && mid == 40) {
        hp = CPOS(f + 1);
        hi = frame_at(b, hp, L, fmax);
        // a publish too large for the carry is a control command: the host assembles it
        if ((c.kind == CK_PUBLISH || c.kind == CK_TXBUF) && big_publish(d, fi.size, hi.size, be64(b + hp + 7 + 4), fmax))
          c.kind = CK_CONTROL;
      }
    }
    const u32 is_pub = is_cmd && c.kind == CK_PUBLISH;
    const u32 is_ack = is_cmd && (c.kind == CK_ACK || c.kind == CK_NACK || c.kind == CK_REJECT);
    // two scans of packed counters: commands | pubs (11 bits each, <= FS_NT per chunk), and
    // fragments | acks (16 bits each: a chunk's fragments are frames of the segment, < 2^16
    // by CAND_MAX; a chunk that is all acks counts FS_NT of them, 11 bits)
    u32 tpk, tfa;
    const u32 rpk = block_scan<FS_NT>(is_cmd | (is_pub << 11), sc, tpk);
    const u32 rfa = block_scan<FS_NT>(nfr | (is_ack << 16), sc, tfa);
    const u32 fr = rfa & 0xffffu, tf = tfa & 0xffffu;
    const u32 r = rpk & 0x7ffu, tcnt = tpk & 0x7ffu;
    if (one) {   // the segment's only chunk: reserve its commands / fragments now (as above)
      if (tid == 0) {
        const u32 cb = tcnt ? atomicAdd(&d.ctr->n_cmds, tcnt) : 0;
        const u32 fb = tf ? atomicAdd(&d.ctr->n_frags, tf) : 0;
        sh_frag_base = fb;
        sh_cmd_base = cb;
        sh_ncmd = (cb + tcnt > d.cmd_max || fb + tf > d.frag_max) ? 1u : 0u;
      }
      __syncthreads();
      if (sh_ncmd && tcnt > 0) {   // (block-uniform) overflow: nothing is emitted, all carried
        const u32 cb = sh_cmd_base;
        for (u32 i = cb + tid; i < cb + tcnt && i < d.cmd_max; i += FS_NT) {
          d.cmds[i].kind = CK_NONE;
          d.cmd_is_pub[i] = 0;
          d.cmd_is_ack[i] = 0;
        }
        __syncthreads();
        if (tid == 0) sh_cmd_base = INVALID;
        so.status |= SS_OVERFLOW;
        so.status &= ~(SS_FRAME_ERROR | SS_UNEXPECTED);
        consumed = 0;
        kf = 0;
        reason = 7;
        break;
      }
      if (tcnt == 0 && tid == 0) sh_cmd_base = INVALID;
    }
    // the segment's Basic.Gets: a contiguous DGet range per chunk, in wire order
    u32 gi = INVALID;
    if (sh_get0 != INVALID) {   // (block-uniform)
      const u32 is_get = is_cmd && c.kind == CK_GET;
      u32 tg;
      const u32 rg = block_scan<FS_NT>(is_get, sc, tg);
      if (tid == 0) sh_gbase = tg ? atomicAdd(&d.tot[TS_NDGET], tg) : 0;
      __syncthreads();
      if (is_get) gi = sh_gbase + rg;
    }
    if (is_cmd) {
      c.conn = conn;
      c.ch = fi.ch;
      c.m_off = OFF(p) + 7;
      c.m_len = fi.size;
      c.h_off = 0; c.h_len = 0; c.frag0 = 0; c.nfrag = 0; c.body_size = 0;
      c.seg = s;
      c.raw_off = OFF(p);
      // ordinals within the segment: k_decode numbers publishes / acks segment-major
      c.pad[1] = npub_run + (rpk >> 11);
      c.pad[2] = nack_run + (rfa >> 16);
      u32 endp = p + 8 + fi.size;
      if (cls == 60 && mid == 40) {
        c.h_off = OFF(hp) + 7;
        c.h_len = hi.size;
        c.body_size = (u32)be64(b + hp + 7 + 4);
        c.frag0 = sh_frag_base + frun + fr;
        c.nfrag = nfr;
        endp = hp + 8 + hi.size;
        for (u32 k = 0; k < nfr; ++k) {
          u32 bp = CPOS(f + 2 + k);
          FInfo bi = frame_at(b, bp, L, fmax);
          Frag fg;
          fg.off = OFF(bp) + 7;
          fg.len = bi.size;
          d.frags[c.frag0 + k] = fg;
          endp = bp + 8 + bi.size;
        }
      }
      c.raw_len = endp - p;
      const u32 ci = sh_cmd_base + run + r;
      if (gi != INVALID) {
        if (gi < DGET_MAX) {
          DGet g;
          g.conn = conn; g.chslot = c.pad[0]; g.q = gq; g.noack = gna;
          g.raw_off = c.raw_off; g.raw_len = c.raw_len; g.seg = s; g.pad = 0;
          d.dget[gi] = g;
        } else {
          c.kind = CK_CONTROL;   // the step's DGet list is full: the host serves it (not paused)
        }
      }
      d.cmds[ci] = c;
      // classification for the rank scan of the large-segment-count path (k_decode)
      d.cmd_is_pub[ci] = is_pub;
      d.cmd_is_ack[ci] = is_ack;
      if (c.kind == CK_CONTROL || c.kind == CK_TXBUF) {
        u32 cbase;
        u32 g = reserve_sat(&d.ctr->ctrl_bytes, c.raw_len, (u32)d.ctrl_cap, &cbase);
        u32 ri = atomicAdd(&d.ctr->n_ctrl, 1u);
        CtrlRec rec;
        rec.conn = conn;
        if (g == c.raw_len) {
          for (u32 k = 0; k < c.raw_len; ++k) d.ctrl[cbase + k] = b[p + k];
          rec.off = cbase; rec.len = c.raw_len;
          rec.seg = c.kind == CK_TXBUF ? (CTRL_TXBUF | p) : gi != INVALID ? (CTRL_DGET | s) : s;
        } else {   // control buffer full: an event, the host closes the connection (506)
          rec.off = INVALID; rec.len = 506; rec.seg = 0;
        }
        if (ri < d.seg_max * 2) d.ctrl_rec[ri] = rec;
      }
    }
    run += tcnt;
    frun += tf;
    npub_run += tpk >> 11;
    nack_run += tfa >> 16;
  }
  if (tid == 0 && kf > 0) d.conn_last_rx[conn] = now;
  if (reason == 0) so.status |= SS_CTRL;
  if (tid == 0) {   // the segment's publish / ack counts: k_decode numbers them segment-major
    d.seg_cmd_base[s] = (run && sh_cmd_base != INVALID) ? sh_cmd_base : INVALID;
    d.seg_npub[s] = d.seg_cmd_base[s] == INVALID ? 0u : npub_run;
    d.seg_nack[s] = d.seg_cmd_base[s] == INVALID ? 0u : nack_run;
  }

  FS_MARK(7);
  // ---- (f) carry out: bytes [consumed, L)
  u32 rest = L - consumed;
  if (rest > d.carry_cap) { so.status |= SS_TOO_LARGE; rest = 0; }
  else if (split) {   // [consumed, sp) from the work copy, the rest from the ingress slot (sp >= carry)
    u8* const cd = d.carry + (u64)conn * d.carry_cap;
    if (consumed < sp) block_copy(cd, d.work + wbase + consumed, sp - consumed, tid, FS_NT);
    const u32 from = consumed > sp ? consumed : sp;
    if (from < L) block_copy(cd + (from - consumed), seg_N + (from - seg_cl), L - from, tid, FS_NT);
  } else block_copy(d.carry + (u64)conn * d.carry_cap, bg + consumed, rest, tid, FS_NT);   // 16-B moves from HBM
  FS_MARK(8);
  if (tid == 0) {
    so.consumed = consumed;
    so.carry = rest;
    so.ncmds = run;
    d.carry_len[conn] = rest;
    if (reason == 0) d.conn_paused[conn] = 1;
    d.seg_out[s] = so;
  }
#undef CPOS
}

// the step's ingress payload copy, queued by the host on one or two SDMA engines through HSA
// (Engine h2d_hsa): waited for here, on the device, by the kernel that first reads the slot.
// No marker on a HIP stream and no cross-queue barrier sits between two steps' copies, so
// they run back to back on their engine (bench/micro/h2d_chain_probe.hip, profiles/r6_z).
// Block 0 alone polls the completion signals -- they live in host memory, every poll is a
// read over the link the copy is using -- and passes the news on through a device word
// (tot[TS_H2D_SEEN] = step + 1) the other blocks poll at agent scope.  The SDMA engine
// writes HBM behind the L2s: every block of the grid, with a segment or without, ends its
// wait with a system-scope acquire before it reads the slot or returns, so every XCD the
// dispatcher gave a block has dropped its stale lines of the slot before k_decode,
// k_route_store and the later readers run -- as the 16 blocks of the earlier k_h2d_wait did,
// with a block per CU instead of two per XCD.
// Bounded: a copy that never completes lets the step run on (block 0 passes the word on
// when its budget is spent, and every other block has the same budget), and the host's
// check of the signal at collection (Engine::wait_results) reports it
DEV void h2d_wait(const DS& d) {
  const u64 sig = d.in->h2d_sig, sig2 = d.in->h2d_sig2;   // (sig2: a payload split over two engines)
  if (!sig) return;
  const u32 lim = d.in->h2d_polls ? d.in->h2d_polls : (1u << 24);
  const u32 seen = (u32)d.in->step + 1u;
  // (one wave polls and acquires: the block's waves share the CU's L1 and the XCD's L2, and
  // the barrier keeps their reads of the slot behind it)
  if (threadIdx.x < 64) {
    if (threadIdx.x != 0) {
    } else if (blockIdx.x == 0) {
      for (u32 it = 0; it < lim; ++it) {
        if (__hip_atomic_load((const i64*)sig, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0 &&
            (!sig2 || __hip_atomic_load((const i64*)sig2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0))
          break;
        __builtin_amdgcn_s_sleep(4);
      }
      __hip_atomic_store(&d.tot[TS_H2D_SEEN], seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      for (u32 it = 0; it < lim; ++it) {
        if (__hip_atomic_load(&d.tot[TS_H2D_SEEN], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == seen) break;
        __builtin_amdgcn_s_sleep(4);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  }
  __syncthreads();
}

// the same wait as a launch of its own, 16 blocks in front of the frame scan: for a frame
// scan grid of fewer blocks than that (a small seg_max), which could not reach every XCD
__global__ __launch_bounds__(64) void k_h2d_wait(DS d) { h2d_wait(d); }

// block-stride over the segments: the grid is capped below seg_max (a 1024-thread block
// per segment slot of the capacity would mostly launch idle waves).  wait: every block waits
// for the step's payload (h2d_wait) -- one with a segment loads its first descriptor before
// it does -- so a step never ends before its copy, whatever its segments
__global__ __launch_bounds__(FS_NT) void k_frame_scan(DS d, u32 wait) {
  const u32 nseg = d.in->nseg;
  if (!wait && blockIdx.x >= nseg) return;
  FsHead hd{};
  if (blockIdx.x < nseg) hd = fs_head(d, blockIdx.x);
  if (wait) h2d_wait(d);
  for (u32 s = blockIdx.x; s < nseg; s += gridDim.x) {
    frame_scan_seg(d, s, s == blockIdx.x ? hd : fs_head(d, s));
    __syncthreads();   // the next segment reuses the LDS
  }
}

// a Basic.Get the frame scan decoded that its step cannot serve (delivery window full, cold
// queue head, step full, queue gone): its bytes go to the host as a control record flagged
// CTRL_DGET -- the connection is not paused -- and the host serves it with a later step
DEV void dget_to_host(const DS& d, u32 k) {
  const DGet g = d.dget[k];
  u32 cbase;
  const u32 got = reserve_sat(&d.ctr->ctrl_bytes, g.raw_len, (u32)d.ctrl_cap, &cbase);
  const u32 ri = atomicAdd(&d.ctr->n_ctrl, 1u);
  CtrlRec rec;
  rec.conn = g.conn;
  if (got == g.raw_len) {
    for (u32 k = 0; k < g.raw_len; ++k) d.ctrl[cbase + k] = d.work[g.raw_off + k];
    rec.off = cbase; rec.len = g.raw_len; rec.seg = CTRL_DGET | g.seg;
  } else {   // control buffer full: an event, the host closes the connection (506)
    rec.off = INVALID; rec.len = 506; rec.seg = 0;
  }
  if (ri < d.seg_max * 2) d.ctrl_rec[ri] = rec;
}
