// Which SDMA engine carries which of the step's copies (copy_engine 3), where a copy is cut
// in two, and how much egress is copied speculatively behind the gate.  Pure functions of
// their arguments -- no HIP, no HSA, no Python: the engine casts the plan into its HSA engine
// ids, tests/native/engine_host_test.cpp checks it for every availability mask.
#pragma once
#include <initializer_list>

#include "step_abi.h"

// engine bit masks (1 << engine number); 0: none
struct SdmaPlan { u32 egress, egress2, tail, ingress, ingress2; };

// the first engine of `order` that is in `mask` and not among `taken`; 0: none
inline u32 sdma_first(std::initializer_list<u32> order, u32 mask, u32 taken) {
  for (u32 c : order)
    if (((mask & ~taken) >> c) & 1u) return 1u << c;
  return 0;
}

// mask: the engines the runtime offers for device -> host copies (not 0); pref: cfg
// sdma_engine (-1 none); sdma_split: cfg sdma_split (2: split egress copies); h2d_split: cfg
// h2d_split.  Measured on MI355X: engines 0-3 reach PCIe rate, 8 and 15 a third of it.
inline SdmaPlan plan_sdma(u32 mask, int pref, int sdma_split, bool h2d_split) {
  SdmaPlan p{0, 0, 0, 0, 0};
  if (!mask) return p;
  // egress: not the engine of the runtime's own H2D copies -- one SDMA engine serialises
  // both directions (measured 54 GB/s total vs 94 GB/s on two engines, bench/pcie_probe.hip)
  if (pref >= 0 && pref < 32 && ((mask >> pref) & 1u)) p.egress = 1u << pref;
  else if ((mask >> 1) & 1u) p.egress = 1u << 1;
  else p.egress = mask & (~mask + 1);   // (the lowest one offered)
  // a second engine for split egress copies: another full-rate one (0-3), not engine 0
  // (the runtime's H2D engine) when there is a choice
  if (sdma_split > 1) p.egress2 = sdma_first({2u, 3u, 0u}, mask, p.egress);
  // the tail engine (gated egress): another full-rate engine than the gated copies' --
  // which can sit behind the next step's gate -- and than the runtime's H2D engine 0
  // (nor the split copies' second engine: an engine's queue is in order, and a gated copy
  // waiting there for the next step's gate would hold the tail back by a step)
  p.tail = sdma_first({2u, 3u, 0u}, mask, p.egress | p.egress2);
  if (!p.tail) p.tail = p.egress;
  // the ingress engine (cfg h2d_hsa): engine 0, the runtime's own H2D engine -- the egress
  // engines stay free of it (measured: egress on engine 0 next to the ingress copies halves
  // the throughput, profiles/r6_x); else any full-rate engine the egress does not use
  p.ingress = sdma_first({0u, 3u, 2u, 1u}, mask, p.egress | p.egress2 | p.tail);
  if (!p.ingress) p.ingress = p.tail;
  // a split payload's second engine: another full-rate one (0-3) that no egress copy uses --
  // on MI355X with the defaults engine 3, next to egress 1, tail 2, ingress 0.  When none is
  // free next to the tail engine, the second half shares the tail engine's queue: the tail is
  // an un-gated copy the host issues after the step (egress_copy) and an ingress half depends
  // on nothing, so each can only wait for the other's bytes to move (at most half a payload),
  // never for a gate.  The gated engines (egress, egress2) are never taken: a copy queued
  // there sits behind a gated copy until the step in flight ends, and the step would wait for
  // its own payload
  if (h2d_split) {
    p.ingress2 = sdma_first({3u, 2u, 0u}, mask, p.ingress | p.egress | p.egress2 | p.tail);
    if (!p.ingress2 && p.tail != p.egress && p.tail != p.egress2 && p.tail != p.ingress && p.tail < (1u << 4))
      p.ingress2 = p.tail;
  }
  return p;
}

// an ingress payload of len bytes: the bytes of its first half, len when it stays whole.  A
// large payload goes in two halves on two engines at once: 56.8 vs 54.9 GB/s on one (the
// PCIe link is the bound, bench/micro/h2d_chain_probe.hip, profiles/r6_z/h2d_chain3.txt)
inline u64 ingress_cut(u64 len, u64 split_min, bool have_engine2) {
  const bool split = have_engine2 && len >= split_min && len > 8192;
  return split ? ((len / 2 + 4095) & ~(u64)4095) : len;
}

// an egress copy of n bytes on k engines: the bytes of the first part
inline u64 egress_cut(u64 n, int k) { return k == 2 ? ((n / 2) & ~(u64)4095) : n; }

// gated egress: bytes to copy speculatively for the next step -- the largest of the last
// four steps' egress + 1/16 + 64 KB, in 64 KB units, at most the slot's allocation (0 after
// four steps without egress)
inline u64 spec_bytes(const u64 hist[4], u64 alloc) {
  u64 mx = 0;
  for (int i = 0; i < 4; ++i) mx = hist[i] > mx ? hist[i] : mx;
  if (!mx) return 0;
  const u64 sz = (mx + mx / 16 + (64u << 10) + 65535) & ~(u64)65535;
  return sz < alloc ? sz : alloc;
}
