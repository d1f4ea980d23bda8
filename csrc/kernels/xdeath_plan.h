// x-death (chana.mq.gpu.dead-letter-x-death): how a dead letter's property bytes are rewritten.
// One plan function and one writer, both plain C++ without wave intrinsics, so that the dead
// pass's size pass and its write pass cannot disagree about a length (a disagreement there is a
// buffer overrun on the device) and so that tests/native/xdeath_plan_test.cpp can drive them on
// the CPU.  The device side is dp_xdeath.h; the rule is CHANGES.md "x-death headers"; the golden
// model's form of it is chanamq_amd/engine/xdeath.py.
//
// xd_plan turns a property list into offsets, the matched x-death element, the new length and
// the verdict; xd_emit writes the new bytes through an emitter (the test's appends to a bounded
// buffer, the device's copies with the whole wave).  Every value read from the bytes goes
// through S::s(): the identity here, readfirstlane on the device, where the list is the same
// for every lane of the wave and the walk then runs in scalar registers (dp_headers.h's idiom).
#pragma once
#include "step_abi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XD_FN __device__ __host__ inline
#else
#define XD_FN inline
#endif

enum : u32 {
  XD_VERBATIM = 0,   // no rewrite: the property list is cut short, or its headers table does not parse
  XD_REWRITE = 1,
  XD_OVER = 2,       // over a limit: the dead letter is dropped (n_dl_dropped)
  XD_NONE = 0xffffffffu,
  XD_ELEMS_MAX = 64,          // elements of the merged x-death array
  XD_PROPS_MAX = 65535        // new property bytes (MsgEnt.props_len is 16 bits; the import path has no lower bound)
};
enum : u32 { XD_EXPIRED = 0, XD_MAXLEN = 1, XD_REJECTED = 2 };

struct XdScalarId { static XD_FN u32 s(u32 v) { return v; } };

// what dies: the source queue's name, the reason, the exchange and routing key the message
// carried in the queue, the seconds of the step that renders the dead letter
struct XdCtx {
  const u8* qn; u32 qnl;
  u32 reason;
  const u8* ex; u32 exl;
  const u8* rk; u32 rkl;
  u64 time_s;
};

struct XdPlan {
  u32 status, new_len;
  u32 fl_end;             // end of the flag words
  u32 hpos;               // where the headers table's length word stands, or is inserted
  u32 tb, te;             // the old table's body (tb == te: none, or empty)
  u32 hend;               // first byte behind the old table (hpos when there is none)
  u32 has_tab;
  u32 exp_off, exp_len;   // the expiration's length byte and text length (exp_off 0: none)
  u32 tab_len;            // the new table's body
  u32 first;              // the three x-first-death entries are added
  u32 arr_b, arr_e;       // the old x-death array's body (0, 0: none, or malformed and replaced)
  u32 arr_len;            // the new array's body
  u32 nel;                // elements of the old array
  u32 m_off, m_end;       // the matched element, from its 'F' (m_off XD_NONE: none, a new one goes in front)
  u32 c_off, c_end;       // its count's value, tag included (c_off 0: no count entry, one is inserted first)
  u32 front_len;          // the front element's bytes, 'F' and length included
  u64 count;              // the matched element's new count
};

XD_FN u32 xd_be16(const u8* p) { return ((u32)p[0] << 8) | (u32)p[1]; }
XD_FN u32 xd_be32(const u8* p) { return ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | (u32)p[3]; }

XD_FN const char* xd_reason(u32 r, u32* n) {
  if (r == XD_EXPIRED) { *n = 7; return "expired"; }
  if (r == XD_MAXLEN) { *n = 6; return "maxlen"; }
  *n = 8;
  return "rejected";
}

// wire bytes of a fixed-size tag; -1: a 4-byte length follows; -2: unknown (dp_headers.h hdr_fixed)
XD_FN int xd_fixed(u32 tag) {
  switch (tag) {
    case 'V': return 0;
    case 't': case 'b': case 'B': return 1;
    case 's': case 'u': return 2;
    case 'I': case 'i': case 'f': return 4;
    case 'D': return 5;
    case 'l': case 'T': case 'd': return 8;
    case 'S': case 'x': case 'A': case 'F': return -1;
    default: return -2;
  }
}
XD_FN bool xd_is_int(u32 tag) {
  return tag == 'b' || tag == 'B' || tag == 's' || tag == 'u' || tag == 'I' || tag == 'i' || tag == 'l';
}

struct XdEnt { u32 noff, nlen, tag, voff, vend; };   // name bytes, tag, the value's bytes behind the tag

// the table entry at pos of the table ending at end, pos moved behind it; false: malformed.
// (xd_fixed / xd_next are a host-compilable copy of dp_headers.h's hdr_fixed / hdr_next, which call
// readfirstlane directly: a change of the table format goes into both)
template <class S>
XD_FN bool xd_next(const u8* p, u32& pos, u32 end, XdEnt& e) {
  if (end - pos < 2) return false;
  const u32 nl = S::s(p[pos]);
  if (nl + 2 > end - pos) return false;
  const u32 tag = S::s(p[pos + 1 + nl]);
  e.noff = pos + 1;
  e.nlen = nl;
  e.tag = tag;
  pos += 2 + nl;
  e.voff = pos;
  const int fx = xd_fixed(tag);
  if (fx == -2) return false;
  u32 n = (u32)fx;
  if (fx < 0) {
    if (end - pos < 4) return false;
    const u32 len = S::s(xd_be32(p + pos));
    if (len > end - pos - 4) return false;
    n = 4 + len;
  }
  if (n > end - pos) return false;
  pos += n;
  e.vend = pos;
  return true;
}

template <class S>
XD_FN bool xd_eq(const u8* a, const u8* b, u32 n) {
  u32 diff = 0;
  for (u32 i = 0; i < n; ++i) diff |= (u32)(a[i] ^ b[i]);
  return S::s(diff) == 0;
}
template <class S>
XD_FN bool xd_name_is(const u8* p, const XdEnt& e, const char* name, u32 n) {
  return e.nlen == n && xd_eq<S>(p + e.noff, (const u8*)name, n);
}

// an integer tag's value, with the width and signedness csrc/core/codec.cpp reads it
template <class S>
XD_FN i64 xd_int(const u8* v, u32 tag) {
  switch (tag) {
    case 'b': return (i64)(int8_t)S::s(v[0]);
    case 'B': return (i64)S::s(v[0]);
    case 's': return (i64)(int16_t)S::s(xd_be16(v));
    case 'u': return (i64)S::s(xd_be16(v));
    case 'I': return (i64)(i32)S::s(xd_be32(v));
    case 'i': return (i64)S::s(xd_be32(v));
    default: return (i64)(((u64)S::s(xd_be32(v)) << 32) | S::s(xd_be32(v + 4)));
  }
}

// one element of an x-death array: a table ('F') at pos of the array body ending at end
struct XdElem {
  u32 off, end;           // from its 'F' to behind its body
  u32 q_off, q_len;       // its first `queue` entry's string (q_len XD_NONE: none, or no string)
  u32 r_off, r_len;       // its first `reason` entry's string
  u32 c_off, c_end, c_tag;   // its first `count` entry's value, tag included (c_off 0: none)
};
// false: not a table, or it runs past the array.  An element whose own table does not parse is
// kept as it is and has neither queue nor reason
template <class S>
XD_FN bool xd_elem(const u8* p, u32 pos, u32 end, XdElem& el) {
  if (end - pos < 5 || S::s(p[pos]) != 'F') return false;
  const u32 len = S::s(xd_be32(p + pos + 1));
  if (len > end - pos - 5) return false;
  el.off = pos;
  el.end = pos + 5 + len;
  el.q_len = el.r_len = XD_NONE;
  el.q_off = el.r_off = el.c_off = el.c_end = el.c_tag = 0;
  bool seen_q = false, seen_r = false, seen_c = false;
  u32 q = pos + 5;
  while (q < el.end) {
    XdEnt e;
    if (!xd_next<S>(p, q, el.end, e)) { el.q_len = el.r_len = XD_NONE; el.c_off = 0; return true; }
    if (!seen_q && xd_name_is<S>(p, e, "queue", 5)) {
      seen_q = true;
      if (e.tag == 'S') { el.q_off = e.voff + 4; el.q_len = e.vend - e.voff - 4; }
    } else if (!seen_r && xd_name_is<S>(p, e, "reason", 6)) {
      seen_r = true;
      if (e.tag == 'S') { el.r_off = e.voff + 4; el.r_len = e.vend - e.voff - 4; }
    } else if (!seen_c && xd_name_is<S>(p, e, "count", 5)) {
      seen_c = true;
      el.c_off = e.voff - 1; el.c_end = e.vend; el.c_tag = e.tag;
    }
  }
  return true;
}
XD_FN bool xd_elem_complete(const XdElem& el) { return el.q_len != XD_NONE && el.r_len != XD_NONE; }

// The plan of the rewrite of property bytes p[0, plen) for the death c.  ban.add(off, len) gets
// the queue names (in p) of the old elements that ban their queue for this dead letter: those
// in front of the first element whose reason is `rejected`, the matched element left out (it
// is the front element, whose queue is the source queue itself: the caller bans that one,
// unless the reason is a reject -- then nothing is banned and ban.add is never called).
template <class S, class B>
XD_FN void xd_plan(const u8* p, u32 plen, const XdCtx& c, XdPlan& pl, B& ban) {
  pl = XdPlan{};
  pl.status = XD_VERBATIM;
  pl.new_len = plen;
  pl.m_off = XD_NONE;
  // ---- the flag words and the values behind them (dp_headers.h hdr_table's walk)
  u32 q = 0, fl = 0, nfl = 0;
  bool fend = false;
  while (q + 2 <= plen) {
    const u32 fw = S::s(xd_be16(p + q));
    q += 2;
    if (nfl == 0) fl = fw;
    ++nfl;
    if (!(fw & 1)) { fend = true; break; }
  }
  if (!fend) return;
  pl.fl_end = q;
  for (int bit = 15; bit >= 2; --bit) {
    if (bit == 13) pl.hpos = pl.hend = pl.tb = pl.te = q;
    if (!(fl & (1u << bit))) continue;
    u32 n;
    if (bit == 13) {
      if (plen - q < 4) return;
      const u32 tl = S::s(xd_be32(p + q));
      if (tl > plen - q - 4) return;
      pl.has_tab = 1;
      pl.tb = q + 4; pl.te = pl.tb + tl;
      pl.hend = pl.te;
      n = 4 + tl;
    } else if (bit == 12 || bit == 11) {
      n = 1;
    } else if (bit == 6) {
      n = 8;
    } else {
      if (plen - q < 1) return;
      n = 1 + S::s(p[q]);
      if (bit == 8) { pl.exp_off = q; pl.exp_len = n - 1; }
    }
    if (n > plen - q) return;
    q += n;
  }
  // ---- the old table: checked from end to end; the x-death entries and x-first-death-queue
  u32 xd_rm = 0, xd_tag = 0, xd_voff = 0, xd_vend = 0;
  bool have_xd = false, have_first = false;
  u32 pos = pl.tb;
  while (pos < pl.te) {
    XdEnt e;
    const u32 e0 = pos;
    if (!xd_next<S>(p, pos, pl.te, e)) return;
    if (xd_name_is<S>(p, e, "x-death", 7)) {
      xd_rm += pos - e0;
      if (!have_xd) { have_xd = true; xd_tag = e.tag; xd_voff = e.voff; xd_vend = e.vend; }
    } else if (xd_name_is<S>(p, e, "x-first-death-queue", 19)) {
      have_first = true;
    }
  }
  pl.status = XD_REWRITE;
  pl.first = have_first ? 0u : 1u;
  u32 rl;
  const char* rs = xd_reason(c.reason, &rl);
  // ---- the old array: every element a table, or it is replaced
  if (have_xd && xd_tag == 'A') {
    pl.arr_b = xd_voff + 4; pl.arr_e = xd_vend;
    u32 a = pl.arr_b, n = 0;
    bool banning = c.reason != XD_REJECTED;
    while (a < pl.arr_e) {
      XdElem el;
      if (!xd_elem<S>(p, a, pl.arr_e, el)) { n = XD_NONE; break; }
      a = el.end;
      ++n;
      if (!xd_elem_complete(el)) continue;
      const bool match = pl.m_off == XD_NONE && el.q_len == c.qnl && el.r_len == rl &&
                         xd_eq<S>(p + el.q_off, c.qn, c.qnl) && xd_eq<S>(p + el.r_off, (const u8*)rs, rl);
      if (match) {
        pl.m_off = el.off; pl.m_end = el.end;
        pl.c_off = el.c_off; pl.c_end = el.c_end;
        pl.count = (el.c_off && xd_is_int(el.c_tag)) ? (u64)xd_int<S>(p + el.c_off + 1, el.c_tag) + 1 : 1;
        continue;
      }
      if (!banning) continue;
      if (el.r_len == 8 && xd_eq<S>(p + el.r_off, (const u8*)"rejected", 8)) banning = false;
      else ban.add(el.q_off, el.q_len);
    }
    if (n == XD_NONE) {   // malformed: an array holding the new element alone (whatever was banned is void)
      pl.arr_b = pl.arr_e = 0;
      pl.m_off = XD_NONE;
      pl.nel = 0;
      ban.reset();
    } else {
      pl.nel = n;
    }
  }
  // ---- sizes
  if (pl.m_off == XD_NONE) {
    u32 body = 15 + (12 + rl) + (11 + c.qnl) + 14 + (14 + c.exl) + (18 + 5 + c.rkl);
    if (pl.exp_off) body += 25 + pl.exp_len;
    pl.front_len = 5 + body;
    pl.arr_len = pl.front_len + (pl.arr_e - pl.arr_b);
  } else {
    const u32 ml = pl.m_end - pl.m_off;
    pl.front_len = pl.c_off ? ml - (pl.c_end - pl.c_off) + 9 : ml + 15;
    pl.arr_len = pl.front_len + (pl.arr_e - pl.arr_b) - ml;
  }
  u32 first_len = 0;
  if (pl.first) first_len = (26 + rl) + (25 + c.qnl) + (28 + c.exl);
  pl.tab_len = (pl.te - pl.tb) - xd_rm + first_len + 13 + pl.arr_len;
  pl.new_len = plen + (pl.has_tab ? 0u : 4u) - (pl.te - pl.tb) + pl.tab_len - (pl.exp_off ? 1 + pl.exp_len : 0u);
  if (pl.nel + (pl.m_off == XD_NONE ? 1u : 0u) > XD_ELEMS_MAX || pl.new_len > XD_PROPS_MAX) pl.status = XD_OVER;
}

// The new property bytes of a plan with status XD_REWRITE, through emitter em: em.raw(src, n)
// copies bytes, em.byte / em.be32 / em.be64 write values, each appending.  pl.new_len bytes.
template <class S, class E>
XD_FN void xd_field(E& em, const char* name, u32 nl, const u8* v, u32 vl) {
  em.byte(nl);
  em.raw((const u8*)name, nl);
  em.byte('S');
  em.be32(vl);
  em.raw(v, vl);
}
template <class S, class E>
XD_FN void xd_emit(E& em, const u8* p, u32 plen, const XdCtx& c, const XdPlan& pl) {
  u32 rl;
  const char* rs = xd_reason(c.reason, &rl);
  // flag words, the values in front of the table, the table's new length
  const u32 fl = (S::s(xd_be16(p)) | (1u << 13)) & ~(1u << 8);
  em.byte(fl >> 8);
  em.byte(fl & 255u);
  em.raw(p + 2, pl.fl_end - 2);
  em.raw(p + pl.fl_end, pl.hpos - pl.fl_end);
  em.be32(pl.tab_len);
  // the old entries in their old order, minus every x-death (runs between them copied whole)
  u32 pos = pl.tb, run = pl.tb;
  while (pos < pl.te) {
    XdEnt e;
    const u32 e0 = pos;
    if (!xd_next<S>(p, pos, pl.te, e)) break;   // (checked by the plan: never)
    if (xd_name_is<S>(p, e, "x-death", 7)) {
      em.raw(p + run, e0 - run);
      run = pos;
    }
  }
  em.raw(p + run, pl.te - run);
  if (pl.first) {
    xd_field<S>(em, "x-first-death-reason", 20, (const u8*)rs, rl);
    xd_field<S>(em, "x-first-death-queue", 19, c.qn, c.qnl);
    xd_field<S>(em, "x-first-death-exchange", 22, c.ex, c.exl);
  }
  em.byte(7);
  em.raw((const u8*)"x-death", 7);
  em.byte('A');
  em.be32(pl.arr_len);
  // the front element: new, or the matched one with its count rewritten
  em.byte('F');
  em.be32(pl.front_len - 5);
  if (pl.m_off == XD_NONE) {
    em.byte(5); em.raw((const u8*)"count", 5); em.byte('l'); em.be64(1);
    xd_field<S>(em, "reason", 6, (const u8*)rs, rl);
    xd_field<S>(em, "queue", 5, c.qn, c.qnl);
    em.byte(4); em.raw((const u8*)"time", 4); em.byte('T'); em.be64(c.time_s);
    xd_field<S>(em, "exchange", 8, c.ex, c.exl);
    em.byte(12); em.raw((const u8*)"routing-keys", 12); em.byte('A'); em.be32(5 + c.rkl);
    em.byte('S'); em.be32(c.rkl); em.raw(c.rk, c.rkl);
    if (pl.exp_off) xd_field<S>(em, "original-expiration", 19, p + pl.exp_off + 1, pl.exp_len);
    em.raw(p + pl.arr_b, pl.arr_e - pl.arr_b);
  } else {
    const u32 b0 = pl.m_off + 5;
    if (pl.c_off) {
      em.raw(p + b0, pl.c_off - b0);
      em.byte('l'); em.be64(pl.count);
      em.raw(p + pl.c_end, pl.m_end - pl.c_end);
    } else {
      em.byte(5); em.raw((const u8*)"count", 5); em.byte('l'); em.be64(pl.count);
      em.raw(p + b0, pl.m_end - b0);
    }
    em.raw(p + pl.arr_b, pl.m_off - pl.arr_b);
    em.raw(p + pl.m_end, pl.arr_e - pl.m_end);
  }
  // the values behind the table, minus the expiration
  if (pl.exp_off) {
    em.raw(p + pl.hend, pl.exp_off - pl.hend);
    em.raw(p + pl.exp_off + 1 + pl.exp_len, plen - (pl.exp_off + 1 + pl.exp_len));
  } else {
    em.raw(p + pl.hend, plen - pl.hend);
  }
}
