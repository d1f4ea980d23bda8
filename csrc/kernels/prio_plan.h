// Priority queues (chana.mq.gpu.priority-queues): the two pieces of plain arithmetic the device
// and the golden model must agree on, in C++ without wave intrinsics so that
// tests/native/prio_plan_test.cpp can drive them on the CPU.  The device side is k_prio_lane and
// k_prio_dispatch (dataplane.hip); the rule is CHANGES.md "Priority queues on the GPU path".
//
// prio_of_props: the `priority` octet of a Basic property list (flags + values).  The whole list
// is walked, as k_decode walks it: a list cut short inside any field has no properties at all
// (the golden model's reading: the codec throws on one), so its priority is 0 whatever was read
// ahead of the cut.
//
// prio_split: a priority queue's lanes hold n[0], n[1], ... ready entries; V is their
// concatenation, lane 0 (the highest priority) first.  A piece [off, off + cnt) of V is cut into
// one part per lane it touches.
#pragma once
#include "step_abi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PRIO_FN __device__ __host__ inline
#else
#define PRIO_FN inline
#endif

#define PRIO_MAX 15u               // the largest x-max-priority served: a queue takes at most 16 slots
#define PRIO_LANES (PRIO_MAX + 1u)

// field order of the first flags word: 15 content-type, 14 content-encoding (short strings),
// 13 headers (table: 32-bit length), 12 delivery-mode, 11 priority (octets), 10..7 short strings,
// 6 timestamp (64 bits), 5..2 short strings.  Continuation words (bit 0) carry no field served
// here and are skipped
PRIO_FN u32 prio_of_props(const u8* p, u32 len) {
  u32 q = 0, fl = 0, nfl = 0;
  bool fend = false;
  while (q + 2 <= len) {
    const u32 fw = ((u32)p[q] << 8) | p[q + 1];
    q += 2;
    if (nfl == 0) fl = fw;
    ++nfl;
    if (!(fw & 1u)) { fend = true; break; }
  }
  if (!fend) return 0;   // cut short inside the flags
  u32 prio = 0;
  for (int bit = 15; bit >= 2; --bit) {
    if (!(fl & (1u << bit))) continue;
    if (bit == 13) {
      if (q + 4 > len) return 0;
      const u32 tl = ((u32)p[q] << 24) | ((u32)p[q + 1] << 16) | ((u32)p[q + 2] << 8) | p[q + 3];
      if (tl > len - q - 4) return 0;
      q += 4 + tl;
    } else if (bit == 12 || bit == 11) {
      if (q + 1 > len) return 0;
      if (bit == 11) prio = p[q];
      q += 1;
    } else if (bit == 6) {
      if (q + 8 > len) return 0;
      q += 8;
    } else {
      if (q + 1 > len) return 0;
      const u32 sl = p[q];
      if (sl > len - q - 1) return 0;
      q += 1 + sl;
    }
  }
  return prio;
}

// the lane slot offset (0 = the base slot, priority P) a message of priority `prio` goes to
PRIO_FN u32 prio_lane(u32 prio, u32 P) { return P - (prio < P ? prio : P); }

struct PrioPart { u32 lane; u64 pos; u32 cnt; };   // `cnt` entries of lane `lane` from its ready entry `pos` on

// the parts of [off, off + cnt) of V, in lane order, into out[] (room for `lanes` parts); returns
// how many.  What lies behind the end of V is left out (the caller grants no more than |V|)
PRIO_FN u32 prio_split(const u64* n, u32 lanes, u64 off, u32 cnt, PrioPart* out) {
  u32 k = 0;
  u64 base = 0;
  for (u32 l = 0; l < lanes && cnt; ++l) {
    const u64 end = base + n[l];
    if (off < end) {
      const u64 room = end - off;
      const u32 take = room < cnt ? (u32)room : cnt;
      out[k].lane = l;
      out[k].pos = off - base;
      out[k].cnt = take;
      ++k;
      off += take;
      cnt -= take;
    }
    base = end;
  }
  return k;
}

// the lane and the position in it of V's entry `off` (off < |V|); false behind the end
PRIO_FN bool prio_locate(const u64* n, u32 lanes, u64 off, u32* lane, u64* pos) {
  u64 base = 0;
  for (u32 l = 0; l < lanes; ++l) {
    if (off < base + n[l]) { *lane = l; *pos = off - base; return true; }
    base += n[l];
  }
  return false;
}
