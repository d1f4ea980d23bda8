// Priority queues (DS.prio; x-max-priority): the two kernels the engine adds to a step with the
// option on.  Included by dataplane.hip behind k_dequeue and runs_body, whose helpers they call;
// the arithmetic both share with the golden model's test is prio_plan.h.  DS.q_prio (dp_state.h)
// has the layout: a priority queue with x-max-priority P is P + 1 consecutive slots, its lanes,
// the base slot b (priority P) first.
#pragma once
#include "prio_plan.h"

// ============================================================================ pairs -> lanes
// At the start of launch_tail, ahead of either sort path: one thread per pair of the step's pair
// table (the step's own publishes, the dead pass's and the host-assembled ones all stand in
// pair_k[0] / pair_v[0] below tot[TS_PAIR_N] by then).  Routing emitted the base slot; a pair whose
// queue is a priority queue moves to the lane of its publish's priority, read from the property
// bytes Pub.props_off points at -- in the work buffer, or, for an imported publish, in `imp`, the
// payload the import of this launch read (the dead pass's buffer in a step, DS.recv_pay otherwise).
__global__ __launch_bounds__(256) void k_prio_lane(DS d, const u8* imp) {
  u32 n = d.tot[TS_PAIR_N];
  if (n > d.pair_max) n = d.pair_max;
  const u32 rb = d.rank_bits, gs = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) {
    const u32 key = d.pair_k[0][i];
    const u32 q = key >> rb;
    if (q >= d.q_max) continue;
    const u32 P = d.q_prio[q];
    if (!P) continue;
    const u32 p = d.pair_v[0][i];
    if (p >= d.pub_cap) continue;
    const Pub& pb = d.pubs[p];
    const u8* src = (pb.flags & MF_IMPORTED) ? imp : d.work;
    const u32 pr = prio_of_props(src + pb.props_off, pb.props_len);
    d.pair_k[0][i] = ((q + prio_lane(pr, P)) << rb) | (key & ((1u << rb) - 1u));
  }
}

// ============================================================================ dispatch over the lanes
// Behind k_dequeue<.., PRIO>, which took every lane -- the base slot too -- through requeue, spill
// and the TTL walk as a queue without consumers and left the base slots' Gets unanswered.  One
// block per slot; the blocks of slots that are no base slot only take the ticket.  For its queue
// the block does what dequeue_queue does behind the TTL walk, over the virtual sequence V: lane
// 0's ready entries (from its head up to its q_cold_lim or tail), then lane 1's, and so on.
//   Gets first, from the front of V, with dequeue_queue's statuses; message-count is what all
//   lanes hold behind the answer.  Then the credit loop with remaining = |V|, the egress-byte sum,
//   the budget cut (longest prefix in run order) and the delivery-slot cut (from the last run
//   backwards), all by dequeue_queue's rules.  Consumer j's grant is a contiguous piece of V and
//   becomes one Run per lane it touches, in that lane's run array with Run.q the lane slot and
//   qpos in the lane's ring, so k_dv_write, acks, requeue and the dead list see ordinary queues.
//   runs_body orders a channel's runs by run slot: lanes stand highest priority first, so one
//   channel's deliveries from several lanes come out in priority order.
// Run-array bound: a lane's array takes at most one run per Get (ngr < RUNS_PER_Q / 2 over all
// lanes) and one per consumer of the window (m <= RUNS_PER_Q - ngr), so at most RUNS_PER_Q.
// Writes q_head and q_nruns of each lane and q_rr[b].  True: runs may have been written.
DEV bool prio_dispatch_queue(const DS& d) {
  __shared__ u32 g_cons[RUNS_PER_Q];
  __shared__ u32 g_n[RUNS_PER_Q];
  __shared__ DqCons g_ci[RUNS_PER_Q];
  __shared__ u64 l_head[PRIO_LANES];   // the lane's head as k_dequeue left it
  __shared__ u64 l_n[PRIO_LANES];      // its entries in V
  __shared__ u64 l_left[PRIO_LANES];   // its ready entries (up to the tail)
  __shared__ u64 l_mask[PRIO_LANES];
  __shared__ u64 l_roff[PRIO_LANES];
  __shared__ u32 l_nr[PRIO_LANES];     // runs written into the lane's array
  __shared__ u64 s_voff;               // V entries the Gets took
  __shared__ u32 s_ngr;
  __shared__ unsigned long long s_bytes;
  const u32 b = blockIdx.x, tid = threadIdx.x, lane = lane_id();
  if (b >= d.q_max) return false;
  const u32 P = d.q_prio[b];   // block-uniform
  if (!P || P > PRIO_MAX || b + P >= d.q_max || !d.q_active[b]) return false;
  const u32 L = P + 1;
  const bool nodisp = (d.in->flags & SF_NODISPATCH) != 0;
  const u32 ndg = d.tot[TS_NDGET] < DGET_MAX ? d.tot[TS_NDGET] : DGET_MAX;
  if (tid < L) {
    const u32 s = b + tid;
    const u64 head = d.q_head[s], tail = d.q_tail[s], clim = d.q_cold_lim[s];
    const u64 lim = clim < tail ? clim : tail;
    l_head[tid] = head;
    l_n[tid] = lim > head ? lim - head : 0;
    l_left[tid] = tail > head ? tail - head : 0;
    l_mask[tid] = d.q_ring_mask[s];
    l_roff[tid] = d.q_ring_off[s];
    l_nr[tid] = 0;
    if (tid == 0) { s_voff = 0; s_ngr = 0; s_bytes = 0; }
  } else if (!nodisp && tid >= 64 && tid - 64 < RUNS_PER_Q) {   // the consumers' inputs, as dequeue_queue loads them
    const u32 j = tid - 64, mall0 = d.q_cons_n[b];
    if (j < mall0) {
      const u32 c = d.q_cons[d.q_cons_off[b] + (d.q_rr[b] % mall0 + j) % mall0];
      const u32 ch = d.cons_ch[c];
      DqCons ci;
      ci.c = c;
      ci.ch = ch;
      ci.ok = d.cons_active[c] == 1u && d.ch_flow[ch] && !d.conn_wblock[ch / d.chpc];
      ci.noack = d.cons_noack[c];
      ci.pc = d.ch_prefetch[ch];
      ci.glob = d.ch_global[ch];
      ci.unacked = d.cons_unacked[c];
      g_ci[j] = ci;
    }
  }
  __syncthreads();
  u64 vsum = 0, ready = 0;
  for (u32 l = 0; l < L; ++l) { vsum += l_n[l]; ready += l_left[l]; }
  // V's entry `off` (off < vsum): its message
  auto msg_at = [&](u64 off) -> u32 {
    u32 ln = 0;
    u64 pos = 0;
    if (!prio_locate(l_n, L, off, &ln, &pos)) return INVALID;
    return d.ring[l_roff[ln] + ((l_head[ln] + pos) & l_mask[ln])].msg;
  };
  if (d.in->nget || ndg) {   // kernel-uniform
    if (tid == 0) {
      const u32 ng = d.in->nget < GET_STEP_MAX ? d.in->nget : GET_STEP_MAX;
      u64 voff = 0;
      u32 ngr = 0;
      for (u32 i = 0; i < ng + ndg; ++i) {
        const bool dev = i >= ng;
        const u32 dk = dev ? i - ng : 0u;
        GetReq rq;
        if (dev) {
          rq.conn = d.dget[dk].conn; rq.chslot = d.dget[dk].chslot; rq.q = d.dget[dk].q; rq.noack = d.dget[dk].noack;
        } else {
          rq = d.get_req[i];
        }
        if (rq.q != b) continue;
        GetOut o;
        o.status = GS_RETRY;
        o.msg_count = 0;
        if (!nodisp && voff == ready) {
          o.status = GS_EMPTY;
        } else if (!nodisp && voff < vsum && ngr < RUNS_PER_Q / 2 && rq.chslot < d.c_max * d.chpc) {
          const u32 ch = rq.chslot;
          u32 ln = 0;
          u64 pos = 0;
          prio_locate(l_n, L, voff, &ln, &pos);
          const u32 mg = d.ring[l_roff[ln] + ((l_head[ln] + pos) & l_mask[ln])].msg;
          const u32 sz = deliver_size(d, d.cons_max, d.msgs[mg], ch / d.chpc);
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
            const u64 left = ready - voff - 1;   // over all lanes
            Run rn;
            rn.ch = ch;
            rn.cons = left < 0xffffffffull ? (u32)left : 0xffffffffu;
            rn.cnt = 1;
            rn.q = b + ln;
            rn.qpos = l_head[ln] + pos;
            rn.noack = rq.noack ? 1u : 0u;
            rn.flags = RUN_GET;
            d.runs[(u64)(b + ln) * RUNS_PER_Q + l_nr[ln]] = rn;
            ++l_nr[ln];
            ++ngr;
            ++voff;
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
      s_voff = voff;
      s_ngr = ngr;
    }
    __syncthreads();
  }
  const u64 voff = s_voff;
  const u32 ngr = s_ngr;
  // each lane's new head and run count, once V's first `taken` entries are handed out (thread 0)
  auto finish = [&](u64 taken) {
    u64 base = 0;
    for (u32 l = 0; l < L; ++l) {
      const u64 t = taken > base ? (taken - base < l_n[l] ? taken - base : l_n[l]) : 0;
      if (t) d.q_head[b + l] = l_head[l] + t;
      d.q_nruns[b + l] = l_nr[l];
      base += l_n[l];
    }
  };
  const u32 mall = d.q_cons_n[b];
  const u64 avail = vsum - voff;
  if (mall == 0 || avail == 0 || nodisp) {
    if (tid == 0 && ngr) finish(voff);   // (no Get answered: k_dequeue's heads and zero counts stand)
    return ngr != 0;
  }
  const u32 m = mall > RUNS_PER_Q - ngr ? RUNS_PER_Q - ngr : mall;
  const u32 r = d.q_rr[b] % mall;
  // (1) counts by credit: dequeue_queue's loop, the queue's ready entries being V's
  if (tid == 0) {
    u64 remaining = avail;
    for (u32 j = 0; j < m; ++j) {
      const DqCons ci = g_ci[j];
      const u32 c = ci.c;
      g_cons[j] = c;
      g_n[j] = 0;
      if (remaining == 0) continue;
      const u32 ch = ci.ch;
      if (!ci.ok) continue;
      const u64 share = (remaining + (m - j) - 1) / (m - j);
      u32 want = (u32)(share < d.deliver_cap ? share : d.deliver_cap);
      const u32 dcb = d.in->dcap_bytes;
      if (dcb && want > 1 && !(d.links && d.conn_link[ch / d.chpc])) {   // byte cap (StepIn.dcap_bytes)
        const u32 s0 = deliver_size(d, c, d.msgs[msg_at(voff + (avail - remaining))], ch / d.chpc);
        const u32 lim = s0 >= dcb ? 1u : dcb / s0;
        want = want < lim ? want : lim;
      }
      const bool noack = ci.noack;
      const u32 pc = ci.pc;
      if (!noack && pc && !ci.glob) {
        const u32 used = ci.unacked;
        const u32 cr = used < pc ? pc - used : 0;
        want = want < cr ? want : cr;
      }
      u32 wb;
      u32 g = reserve_upto(&d.ch_win[ch], want, d.ucap_mask + 1, &wb);
      if (!noack && pc && ci.glob && g) {
        u32 ub;
        const u32 g2 = reserve_upto(&d.ch_unacked[ch], g, pc, &ub);
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
  // (2) egress bytes of every granted entry, block-parallel per consumer piece
  {
    u32 mine = 0;
    u64 vq = voff;
    for (u32 j = 0; j < m; ++j) {
      const u32 cnt = g_n[j];
      if (!cnt) continue;
      const u32 c = g_cons[j];
      const u32 conn = g_ci[j].ch / d.chpc;
      // the piece is split once into its lanes; within a part the entries are one ring's, four a
      // thread per round with their ring loads, then their message loads, in flight together
      PrioPart part[PRIO_LANES];
      const u32 np = prio_split(l_n, L, vq, cnt, part);
      for (u32 pi = 0; pi < np; ++pi) {
        const u32 ln = part[pi].lane, pc = part[pi].cnt;
        const Desc* ring = d.ring + l_roff[ln];
        const u64 qp = l_head[ln] + part[pi].pos, mask = l_mask[ln];
        constexpr u32 U = 4;
        for (u32 k0 = tid; k0 < pc; k0 += 256 * U) {
          u32 mg[U];
#pragma unroll
          for (u32 u = 0; u < U; ++u) {
            const u32 k = k0 + u * 256;
            mg[u] = k < pc ? ring[(qp + k) & mask].msg : INVALID;
          }
#pragma unroll
          for (u32 u = 0; u < U; ++u)
            if (mg[u] != INVALID) mine += deliver_size(d, c, d.msgs[mg[u]], conn);
        }
      }
      vq += cnt;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0 && mine) atomicAdd(&s_bytes, (unsigned long long)mine);
  }
  __syncthreads();
  if (tid == 0) {
    const u64 bytes = s_bytes;
    const u64 gb = reserve_sat64(d.egress_budget, bytes, d.egress_cap);
    if (gb < bytes) {   // the longest prefix of V's granted entries (in run order) whose frames fit
      u64 left = gb;
      u64 vq = voff;
      bool full = false;
      for (u32 j = 0; j < m; ++j) {
        const u32 cnt = g_n[j];
        if (!cnt) continue;
        const u32 c = g_cons[j];
        const u32 conn = d.cons_ch[c] / d.chpc;
        u32 keep = 0;
        while (!full && keep < cnt) {
          const u32 sz = deliver_size(d, c, d.msgs[msg_at(vq + keep)], conn);
          if (sz > left) { full = true; break; }
          left -= sz;
          ++keep;
        }
        if (keep < cnt) unreserve(d, c, cnt - keep);
        g_n[j] = keep;
        vq += keep;
      }
    }
    // (3) delivery slots, trimmed from the last run backwards (across lanes: V's tail goes first)
    u32 total = 0;
    for (u32 j = 0; j < m; ++j) total += g_n[j];
    u32 db;
    const u32 gt = reserve_sat(&d.ctr->n_deliv, total, d.deliv_max, &db);
    u32 excess = total - gt;
    for (int j = (int)m - 1; j >= 0 && excess; --j) {
      const u32 take = g_n[j] < excess ? g_n[j] : excess;
      if (!take) continue;
      unreserve(d, g_cons[j], take);
      g_n[j] -= take;
      excess -= take;
    }
    // (4) runs, in round-robin order behind the Get answers: one per lane a consumer's piece touches
    u64 vq = voff;
    for (u32 j = 0; j < m; ++j) {
      const u32 cnt = g_n[j];
      if (!cnt) continue;
      const u32 c = g_cons[j];
      PrioPart part[PRIO_LANES];
      const u32 np = prio_split(l_n, L, vq, cnt, part);
      for (u32 k = 0; k < np; ++k) {
        const u32 ln = part[k].lane;
        Run rn;
        rn.ch = d.cons_ch[c];
        rn.cons = c;
        rn.cnt = part[k].cnt;
        rn.q = b + ln;
        rn.qpos = l_head[ln] + part[k].pos;
        rn.noack = d.cons_noack[c];
        rn.flags = 0;
        if (l_nr[ln] < RUNS_PER_Q) {   // (always: the bound above)
          d.runs[(u64)(b + ln) * RUNS_PER_Q + l_nr[ln]] = rn;
          ++l_nr[ln];
        }
      }
      vq += cnt;
    }
    finish(vq);
    d.q_rr[b] = (r + 1) % mall;
  }
  return true;
}

__global__ __launch_bounds__(256) void k_prio_dispatch(DS d) {
  __shared__ u64 key_lds[DQ_RUN_LDS];
  __shared__ u32 lds[256 / 64 + 1];
  __shared__ u32 s_last;
  const bool wrote = prio_dispatch_queue(d);
  // k_dequeue's ticket, taken here in its place (its PRIO instantiation ends before it): the runs
  // k_dequeue wrote are visible since its kernel ended, this kernel's through the release below
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
