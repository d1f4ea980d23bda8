// Data plane: headers exchanges matched on their bindings' arguments (route_one's headers
// branch, taken for an exchange whose x_type carries XF_HMATCH: chana.mq.gpu.headers-match).
// The rule and the canonical value form are models/matcher.py headers_match's.
//
// Tables (host: dataplane.py routing_changed): per exchange x_h_off / x_h_n into the rows;
// per row h_queue (the queue, or XT_EDGE | destination; sorted like the topic rows), h_meta
// (pairs | HM_ANY) and h_pair (first pair); per pair HP_WORDS words (below).  Names and
// values lie in kpool; a raw-class value (f d D A F) there is its tag byte and wire bytes.
//
// One wave per publish, one lane per row (64 rows a call).  The message side is the same for
// every lane, so it is kept in scalar registers: the wave walks the table entry by entry
// together (every value read from the message goes through readfirstlane), hashes an entry's
// name 64 bytes a load (lane i loads byte i, the hash runs over readlane), and each row lane
// looks the entry up in its own pairs.  Equal 32-bit hashes are a prefilter only, the bytes
// decide.  A pair counts the first entry of its name (seen); later ones are ignored.  The
// value's hash is worked out only for an entry whose name some row asks for.
//
// The branch shares k_route's 64 VGPRs with the live state of the other exchange types: per
// lane it keeps the row's pair pointer, count, mode and the seen / hit masks, and its loops
// stay rolled (profiles/headers_match/resource_usage.md).
#pragma once
#include "dp_state.h"
#include "dp_util.h"

enum : u32 {
  HP_NHASH = 0, HP_VHASH = 1,   // FNV-1a 32 of the name / of the canonical value bytes
  HP_NOFF = 2, HP_VOFF = 3,     // kpool offsets
  HP_VLEN = 4,
  HP_NLEN = 5,                  // name length | flags << 24
  HPF_PRESENT = 1,              // void binding value: the name's presence is the hit
  HPF_RAW = 2,                  // raw-class value
  HM_ANY = 0x100                // h_meta: x-match any
};
#define HDR_BASIS 0x811c9dc5u
#define HDR_PRIME 0x01000193u
#define HDR_TRUE 0x65757274ull      // "true", "false": first byte lowest
#define HDR_FALSE 0x65736c6166ull

// a value every lane holds alike, in a scalar register
DEV u32 hdr_s(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }

struct HdrEnt { u32 noff, nlen, tag, voff, vlen; };   // (scalar) offsets from the property bytes

// wire bytes of a fixed-size tag; -1: a 4-byte length follows; -2: unknown tag
DEV int hdr_fixed(u32 tag) {
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
DEV bool hdr_is_raw(u32 tag) { return tag == 'f' || tag == 'd' || tag == 'D' || tag == 'A' || tag == 'F'; }
DEV bool hdr_is_str(u32 tag) { return tag == 'S' || tag == 'x'; }

// (xdeath_plan.h keeps a host-compilable copy of hdr_fixed / hdr_next, xd_fixed / xd_next: a change
// of the table format goes into both)
// the entry at pos of the table ending at end, pos moved behind it; false: malformed (an
// unknown tag, or the entry runs past the table).  voff / vlen: the bytes the canonical
// value is made of (a string's bytes; an array's or table's length and bytes)
DEV bool hdr_next(const u8* p, u32& pos, u32 end, HdrEnt& e) {
  const u32 nl = hdr_s(p[pos]);
  if (nl + 2 > end - pos) return false;
  const u32 tag = hdr_s(p[pos + 1 + nl]);
  e.noff = pos + 1;
  e.nlen = nl;
  e.tag = tag;
  pos += 2 + nl;
  const int fx = hdr_fixed(tag);
  if (fx == -2) return false;
  if (fx >= 0) {
    if ((u32)fx > end - pos) return false;
    e.voff = pos; e.vlen = (u32)fx;
    pos += (u32)fx;
    return true;
  }
  if (end - pos < 4) return false;
  const u32 len = hdr_s(be32(p + pos));
  if (len > end - pos - 4) return false;
  if (hdr_is_str(tag)) { e.voff = pos + 4; e.vlen = len; }
  else { e.voff = pos; e.vlen = len + 4; }
  pos += 4 + len;
  return true;
}

// the headers table's body [tb, te) in the property bytes (flags chain, then the values);
// false: none -- or the list is cut short anywhere, the fields behind the headers included
// (k_decode reads such a list as no properties at all)
DEV bool hdr_table(const u8* p, u32 plen, u32& tb, u32& te) {
  u32 q = 0, fl = 0, nfl = 0;
  bool fend = false;
#pragma clang loop unroll(disable)
  while (q + 2 <= plen) {
    const u32 fw = hdr_s(be16(p + q));
    q += 2;
    if (nfl == 0) fl = fw;
    ++nfl;
    if (!(fw & 1)) { fend = true; break; }
  }
  if (!fend) return false;
  bool have = false;
#pragma clang loop unroll(disable)
  for (int bit = 15; bit >= 2; --bit) {
    if (!(fl & (1u << bit))) continue;
    u32 n;
    if (bit == 13) {
      if (plen - q < 4) return false;
      const u32 tl = hdr_s(be32(p + q));
      if (tl > plen - q - 4) return false;
      tb = q + 4; te = tb + tl;
      have = true;
      n = 4 + tl;
    } else if (bit == 12 || bit == 11) {
      n = 1;
    } else if (bit == 6) {
      n = 8;
    } else {
      if (plen - q < 1) return false;
      n = 1 + hdr_s(p[q]);
    }
    if (n > plen - q) return false;
    q += n;
  }
  return have;
}

// FNV-1a 32 over n bytes at b (both the same for every lane), continued from h: lane i loads
// byte i of each 64, the hash runs over them in a scalar register
DEV u32 hdr_fnv(u32 h, const u8* b, u32 n, u32 lane) {
#pragma clang loop unroll(disable)
  for (u32 c0 = 0; c0 < n; c0 += 64) {
    const u32 m = n - c0 < 64 ? n - c0 : 64;
    const u32 v = lane < m ? (u32)b[c0 + lane] : 0u;
#pragma clang loop unroll(disable)
    for (u32 i = 0; i < m; ++i) { h ^= (u32)__builtin_amdgcn_readlane((int)v, (int)i); h *= HDR_PRIME; }
  }
  return h;
}

// an integer tag's value, with the width and signedness csrc/core/codec.cpp reads it
DEV i64 hdr_int(const u8* v, u32 tag) {
  switch (tag) {
    case 'b': return (i64)(int8_t)hdr_s(v[0]);
    case 'B': return (i64)hdr_s(v[0]);
    case 's': return (i64)(int16_t)hdr_s(be16(v));
    case 'u': return (i64)hdr_s(be16(v));
    case 'I': return (i64)(i32)hdr_s(be32(v));
    case 'i': return (i64)hdr_s(be32(v));
    default: return (i64)(((u64)hdr_s(be32(v)) << 32) | hdr_s(be32(v + 4)));   // 'l', 'T'
  }
}

// FNV-1a 32 of an entry's canonical value bytes
DEV u32 hdr_value_hash(const u8* p, const HdrEnt& e, u32 lane) {
  u32 h = HDR_BASIS;
  if (hdr_is_str(e.tag)) return hdr_fnv(h, p + e.voff, e.vlen, lane);
  if (hdr_is_raw(e.tag)) {
    h ^= e.tag; h *= HDR_PRIME;
    return hdr_fnv(h, p + e.voff, e.vlen, lane);
  }
  if (e.tag == 'V') return h;
  if (e.tag == 't') {
    const bool b = hdr_s(p[e.voff]) != 0;
    const u64 s = b ? HDR_TRUE : HDR_FALSE;
#pragma clang loop unroll(disable)
    for (u32 i = 0; i < (b ? 4u : 5u); ++i) { h ^= (u32)(s >> (8 * i)) & 0xffu; h *= HDR_PRIME; }
    return h;
  }
  // the decimal text: digits taken from the end (divisions by a constant only) into nibbles,
  // at most 19 of them, then hashed from the front
  const i64 v = hdr_int(p + e.voff, e.tag);
  u64 m = v < 0 ? 0 - (u64)v : (u64)v;
  if (v < 0) { h ^= '-'; h *= HDR_PRIME; }
  u64 lo = 0;
  u32 hi = 0, nd = 0;
#pragma clang loop unroll(disable)
  do {
    const u32 dg = (u32)(m % 10);
    m /= 10;
    if (nd < 16) lo |= (u64)dg << (4 * nd);
    else hi |= dg << (4 * (nd - 16));
    ++nd;
  } while (m);
#pragma clang loop unroll(disable)
  for (u32 k = nd; k-- > 0;) {
    const u32 dg = k < 16 ? (u32)(lo >> (4 * k)) & 15u : (hi >> (4 * (k - 16))) & 15u;
    h ^= '0' + dg; h *= HDR_PRIME;
  }
  return h;
}

DEV bool hdr_bytes_eq(const u8* a, const u8* b, u32 n) {
  u32 diff = 0;
#pragma clang loop unroll(disable)
  for (u32 i = 0; i < n; ++i) diff |= (u32)(a[i] ^ b[i]);
  return diff == 0;
}

// an entry's canonical value against a binding's (kv: kl bytes of kpool; raw: its class).
// Strings and the raw class compare in place; integers and booleans are rendered again,
// digit by digit from the end, against the binding's text
DEV bool hdr_value_eq(const u8* p, const HdrEnt& e, const u8* kv, u32 kl, bool raw) {
  if (hdr_is_str(e.tag)) return !raw && kl == e.vlen && hdr_bytes_eq(kv, p + e.voff, e.vlen);
  if (hdr_is_raw(e.tag)) return raw && kl == e.vlen + 1 && kv[0] == e.tag && hdr_bytes_eq(kv + 1, p + e.voff, e.vlen);
  if (raw) return false;
  if (e.tag == 'V') return kl == 0;
  if (e.tag == 't') {
    const bool b = hdr_s(p[e.voff]) != 0;
    const u64 s = b ? HDR_TRUE : HDR_FALSE;
    if (kl != (b ? 4u : 5u)) return false;
    u32 diff = 0;
#pragma clang loop unroll(disable)
    for (u32 i = 0; i < kl; ++i) diff |= (u32)kv[i] ^ ((u32)(s >> (8 * i)) & 0xffu);
    return diff == 0;
  }
  const i64 v = hdr_int(p + e.voff, e.tag);
  u64 m = v < 0 ? 0 - (u64)v : (u64)v;
  u32 i = kl;
#pragma clang loop unroll(disable)
  do {
    if (i == 0 || kv[--i] != '0' + (u32)(m % 10)) return false;
    m /= 10;
  } while (m);
  if (v < 0 && (i == 0 || kv[--i] != '-')) return false;
  return i == 0;
}

// The headers table [tb, te) of the publish whose property bytes are p[0, plen), checked
// from end to end: false when there is none or it is malformed (no headers at all, whatever
// came before the fault).  By the whole wave.
DEV bool hdr_open(const u8* p, u32 plen, u32& tb, u32& te) {
  if (!hdr_table(p, plen, tb, te)) return false;
  u32 pos = tb;
  HdrEnt e;
#pragma clang loop unroll(disable)
  while (pos < te) {
    if (!hdr_next(p, pos, te, e)) return false;
  }
  return true;
}

// Does row `row` (valid lanes; one row per lane) match the publish whose property bytes are
// p[0, plen) (the same for every lane)?  Called by all 64 lanes of a wave together.
DEV bool headers_hit(const u8* p, u32 plen, const u32* h_meta, const u32* h_pair, const u32* hp, const u8* kpool,
                     u32 row, bool valid, u32 lane) {
  u32 np = 0, any = 0;
  const u32* pr = hp;
  if (valid) {
    const u32 m = h_meta[row];
    np = m & 0xffu;
    any = m & HM_ANY;
    pr = hp + (u64)h_pair[row] * HP_WORDS;
  }
  if (!__ballot(np != 0)) return valid;   // rows without pairs match everything, in both modes
  u32 tb = 0, te = 0;
  if (!hdr_open(p, plen, tb, te)) tb = te = 0;   // no headers
  u32 seen = 0, hit = 0;
  u32 pos = tb;
#pragma clang loop unroll(disable)
  while (pos < te) {
    HdrEnt e;
    hdr_next(p, pos, te, e);
    const u32 nh = hdr_fnv(HDR_BASIS, p + e.noff, e.nlen, lane);
    // the lane's first pair not yet seen that has this name
    u32 jm = HB_PAIRS;
#pragma clang loop unroll(disable)
    for (u32 j = 0; j < np; ++j) {
      if ((seen >> j) & 1) continue;
      const u32* w = pr + j * HP_WORDS;
      if (w[HP_NHASH] != nh || (w[HP_NLEN] & 0xffffffu) != e.nlen) continue;
      if (!hdr_bytes_eq(kpool + w[HP_NOFF], p + e.noff, e.nlen)) continue;
      jm = j;
      break;
    }
    if (!__ballot(jm < HB_PAIRS)) continue;
    const u32 vh = hdr_value_hash(p, e, lane);
    if (jm < HB_PAIRS) {
      const u32* w = pr + jm * HP_WORDS;
      const u32 fl = w[HP_NLEN] >> 24;
      seen |= 1u << jm;
      if ((fl & HPF_PRESENT) ||
          (w[HP_VHASH] == vh && hdr_value_eq(p, e, kpool + w[HP_VOFF], w[HP_VLEN], (fl & HPF_RAW) != 0)))
        hit |= 1u << jm;
    }
  }
  const u32 nhit = (u32)__popc(hit);
  return valid && (any ? (np == 0 || nhit > 0) : nhit == np);
}
