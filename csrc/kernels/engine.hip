// Native host runtime for the MI355X data plane: owns every device/host-mapped
// buffer, launches the step pipeline on a caller-supplied HIP stream and captures
// it once into a hipGraph (steady-state deliver loop = one hipGraphLaunch).
//
// Python sees a pybind11 module `_dataplane` with class Engine (chanamq_amd/ops).
#include <pybind11/pybind11.h>
#include <pybind11/numpy.h>
#include <pybind11/stl.h>

#include <chrono>
#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <thread>
#include <type_traits>
#include <stdexcept>
#include <string>
#include <vector>

#include <hsa/amd_hsa_signal.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include "dataplane.hip"
#include "delta_stage.h"
#include "sdma_plan.h"
#include "side_box.h"
#include "xchg_host.h"
#include "xchg_rccl.h"
#include "xchg_worker.h"

namespace py = pybind11;

#define HIPCHECK(x)                                                                  \
  do {                                                                               \
    hipError_t _e = (x);                                                             \
    if (_e != hipSuccess)                                                            \
      throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(_e));      \
  } while (0)

static u32 ceil_div(u64 a, u64 b) { return (u32)((a + b - 1) / b); }
static u32 next_pow2(u32 x) { u32 p = 1; while (p < x) p <<= 1; return p; }
static u32 bits_for(u64 maxval) { u32 b = 0; while ((1ull << b) <= maxval) ++b; return b; }

// host-side time accounting of the step loop (seconds, per named phase)
struct HostTimer {
  double* acc;
  std::chrono::steady_clock::time_point t0;
  explicit HostTimer(double* a) : acc(a), t0(std::chrono::steady_clock::now()) {}
  ~HostTimer() { *acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

// roctx range over a host scope (rocprofv3 --marker-trace): step phases, copies, Get
struct Range {
  explicit Range(const char* name) { roctxRangePushA(name); }
  ~Range() { roctxRangePop(); }
};

struct Buf {
  void* ptr = nullptr;
  size_t bytes = 0;
  bool host = false;
  bool view = false;   // a named range of another allocation (not freed on its own)
};

// per-step IO sets ("parities"): step t uses set t % npar_.  Two (double buffering) by
// default; three for a single-GPU engine without the overlapped ingest (cfg "parities"): the
// host then submits step t+1 once step t-2 -- not t-1 -- is collected, so the next step's
// ingress H2D never waits for the host to notice the previous step's kernels ending
static constexpr int NPAR_MAX = 3;

// a parity's device view (what its kernels get) + host addresses of its mapped outputs
struct HostIO : DS {
  const Counters* ctr_host_h = nullptr;
  const SegOut* seg_out_hh = nullptr;
  const ConnOut* conn_out_hh = nullptr;
  const CtrlRec* ctrl_rec_hh = nullptr;
  const u8* ctrl_hh = nullptr;
  const RingMove* grow_hh = nullptr;
  const u32* conn_conf_hh = nullptr;
  GetOut* get_out_hh = nullptr;
  u32* xchg_h = nullptr;   // the exchange words (XC_*): send counts out, receive counts in
};

// one parity: the step IO set, the staging buffers its submit fills, where its step stands
struct StepSlot {
  HostIO io;
  // host-mapped staging read by k_stage / copied H2D with the step
  StepIn* stage_in = nullptr;
  SegIn* stage_segs = nullptr;
  GetReq* stage_gets = nullptr;
  u32* stage_unp = nullptr;
  u8* dl_h = nullptr;              // delta buffer (DeltaStage::pack_deltas)
  // the submitted step
  bool inflight = false;           // submitted, results not collected
  bool staged = false;             // submitted with defer, kernels not launched yet
  u64 launch_seq = 0;              // its step number
  int slot = 0, pslot = 0;         // its egress slot / store-record slot
  u32 nget = 0, nunp = 0;          // Basic.Gets / unpauses it carried
  u32 dl_step = 0;                 // delta bytes it carried
  bool h2d_hip = true;             // its stream waits for ev_h2d
  u64 h2d_addr = 0, h2d_addr2 = 0; // the words its frame scan's wait polled (0: none; second half of a split payload)
  bool eager_d2h = false;          // its egress copy was queued at launch (copy_mode 2)
  // a payload queued ahead of its submit (prefetch)
  bool pre = false;
  u64 pre_seq = 0, pre_ptr = 0, pre_len = 0;
  // overlapped halves recorded at least once
  bool rest_issued = false;
  // sharded steps
  bool phase_a = false;            // phase A launched, submit_b due
  bool counts_ready = false;       // phase A launched, send counts not yet taken
  bool b_due = false;              // phase A launched, launch_b due (native exchange)
  u32 b_wait = 0;                  // the exchange job its phase B waits for (0: none)
  u8 *xs_desc = nullptr, *xs_pay = nullptr, *xr_desc = nullptr, *xr_pay = nullptr;   // native exchange
  u8 *ls_desc = nullptr, *ls_pay = nullptr, *lk_send = nullptr, *rack = nullptr;     // links
  // graphs, captured on first use: whole step / phase A, phase B, overlapped ingest + rest
  hipGraphExec_t graph_exec = nullptr, graph_b = nullptr, graph_ing = nullptr, graph_rest = nullptr;
  // H2D queued, step finished, phase A finished, external exchange stream, ingest half,
  // payload stream, routing half
  hipEvent_t ev_h2d, ev_done, ev_a, ev_ext, ev_ing, ev_pre, ev_rest;
};

// egress slots rotate per step (step t renders into slot t % EGRESS_SLOTS)
struct EgressSlot {
  u8* dev = nullptr;               // rendered on the device
  u8* host = nullptr;              // D2H target
  u8* host_dev = nullptr;          // its device address (copy_mode 2: the copy kernel stores into it)
  hipEvent_t ev_d2h;
  bool d2h_issued = false;
  // HSA SDMA egress: completion of the bulk copy and of the host-issued tail, the gate the
  // step's last kernel opens, bytes copied speculatively behind the gate (0: not gated)
  hsa_signal_t sdma_sig{}, tail_sig{}, gate_sig{};
  bool sdma_pending = false, tail_pending = false;
  u64 spec = 0;
};

// ingress payload slots rotate per step (StepIn.ingress)
struct IngressSlot {
  u8* buf = nullptr;
  hipEvent_t ev_read;              // its last reader (the step's routing half)
  bool read_issued = false;
  // HSA ingress (cfg h2d_hsa): completion of the payload copy, of a split payload's second half
  hsa_signal_t sig{}, sig2{};
  bool hsa = false, split = false; // the slot's last payload went through HSA / in two halves
};

class Engine {
 public:
  explicit Engine(py::dict cfg) {
    auto get = [&](const char* k, u64 dflt) -> u64 {
      return cfg.contains(k) ? cfg[k].cast<u64>() : dflt;
    };
    device_ = (int)get("device", 0);
    HIPCHECK(hipSetDevice(device_));
    {
      int ncu = 0;
      if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device_) == hipSuccess && ncu > 0)
        n_cu_ = (u32)ncu;
    }
    d_ = DS{};
    d_.c_max = (u32)get("c_max", 1024);
    d_.chpc = next_pow2((u32)get("chpc", 16));
    d_.q_max = (u32)get("q_max", 4096);
    d_.x_max = (u32)get("x_max", 1024);
    d_.cons_max = (u32)get("cons_max", 16384);
    d_.seg_max = (u32)get("seg_max", 1024);
    d_.carry_cap = (u32)get("carry_cap", 1u << 20);
    d_.cmd_max = (u32)get("cmd_max", 65536);
    d_.frag_max = (u32)get("frag_max", d_.cmd_max * 2);
    d_.pub_max = d_.cmd_max;
    d_.ack_max = d_.cmd_max;
    // sharded queues (world > 1): records imported from other ranks per step
    d_.world = (u32)get("world", 1);
    d_.my_rank = (u32)get("rank", 0);
    if (d_.world < 1 || d_.world > WORLD_MAX || d_.my_rank >= d_.world)
      throw std::runtime_error("world must be 1..16 and rank < world");
    // Each publish is shipped at most once per other rank and its record payload never
    // exceeds its wire bytes, so these defaults cannot overflow (records / bytes per step).
    d_.import_max = d_.world > 1 ? (u32)get("import_max", (d_.world - 1) * d_.pub_max) : 0;
    // exchange_lag = 1: step t's phase B imports the records of step t-1's all-to-all, so
    // phases A and B launch back to back and the collective overlaps the next step's
    // kernels (cross-GPU publishes are delivered one step later)
    lag_ = d_.world > 1 && get("exchange_lag", 0) != 0;
    d_.pub_cap = ((d_.pub_max + d_.import_max + 63) / 64) * 64;
    d_.xfer_desc_max = d_.world > 1 ? (u32)get("xfer_desc_max", (d_.world - 1) * d_.pub_max) : 0;
    // persistence + recovery: restore batches reuse the import path (world == 1: own buffers)
    d_.persist = (u32)get("persist", 0);
    d_.limits = get("queue_limits", 0) ? 1u : 0u;   // x-max-length / x-overflow honoured (q_limit)
    // x-max-length-bytes honoured (q_blimit, q_bytes, q_broom; the BL instantiations and k_byte_room)
    d_.blimits = get("queue_limit_bytes", 0) ? 1u : 0u;
    if (d_.blimits && !d_.limits) throw std::runtime_error("queue_limit_bytes needs queue_limits");
    // x-max-priority honoured (q_prio, q_lane_base; k_prio_lane, k_prio_dispatch and the PRIO instantiations)
    d_.prio = get("priority_queues", 0) ? 1u : 0u;
    if (d_.prio && d_.world > 1) throw std::runtime_error("priority_queues is not served on a sharded plane (world > 1)");
    d_.persist_max = d_.persist ? (u32)get("persist_max", d_.cmd_max) : 0;
    d_.persist_bytes = d_.persist ? get("persist_bytes", 64ull << 20) : 0;
    // restore / host-publish records at world 1: recovery batches (persist) and messages
    // larger than a connection's carry, assembled by the host (MF_HOSTPUB)
    restore_max_ = (u32)get("restore_max", d_.persist ? (1u << 14) : 64);
    if (d_.world == 1 && restore_max_) {
      d_.import_max = restore_max_;
      d_.pub_cap = ((d_.pub_max + d_.import_max + 63) / 64) * 64;
    }
    d_.pair_max = (u32)get("pair_max", d_.cmd_max * 4);
    // dead-lettering (x-dead-letter-exchange honoured): the dead list and the dead pass's own
    // import buffers.  The pass's records run through the import path of a world-1 engine
    // (publish slots and fragments past the step's own: pub_cap, frag_max + i), so it takes
    // at most import_max of them a step
    if (get("x_death", 0) && !get("dead_letter", 0)) throw std::runtime_error("x_death needs dead_letter");
    d_.dlx = get("dead_letter", 0) ? 1u : 0u;
    alt_ = get("alternate_exchange", 0) != 0;
    if (d_.dlx) {
      if (d_.world != 1)
        throw std::runtime_error("dead_letter: single-rank planes only (a dead-letter exchange's queues may live on "
                                 "another rank, which needs the cross-rank pack path)");
      dl_h_.xdeath = get("x_death", 0) ? 1u : 0u;
      dl_h_.dead_max = (u32)get("dead_max", 1024);
      dl_h_.dead_bytes = get("dead_bytes", 8ull << 20);
      if (dl_h_.dead_max < 1 || dl_h_.dead_max > DEAD_LIST_MAX)
        throw std::runtime_error("dead_max must be 1.." + std::to_string(DEAD_LIST_MAX) + " (k_dead_pack orders the list in one block)");
      if (dl_h_.dead_bytes < 16 || dl_h_.dead_bytes + 8192 > (4ull << 30))
        throw std::runtime_error("dead_bytes must be 16 B .. 4 GiB (u32 offsets)");
      if (!d_.import_max)
        throw std::runtime_error("dead_letter needs the import path's publish slots: restore_max must not be 0");
      dead_room_ = std::min(d_.import_max, dl_h_.dead_max);
      // every record of the pass is at least one pair behind the step's own publishes' pairs
      if ((u64)d_.pair_max < (u64)d_.pub_max + dead_room_)
        throw std::runtime_error("dead_letter: pair_max must cover a step's publishes plus the dead pass (pub_max + min(restore_max, dead_max))");
    }
    d_.deliv_max = (u32)get("deliv_max", 65536);
    if (d_.persist) {
      // a step's consumed-store records: deliveries (<= deliv_max), the durable TTL skip
      // (<= persist_max / 4) and k_chan_advance's settles, budgeted to what is left and
      // carried to the next step past it -- so the record buffer can never overflow
      const u64 need = 2ull * d_.deliv_max + 4096;
      if (d_.persist_max < need) d_.persist_max = (u32)std::min<u64>(need, 1u << 30);
    }
    // remote-consumer links (X2/X3) on the native exchange: a peer's link deliveries (at
    // most its deliv_max per step) arrive with its publishes and are imported with them
    links_ = d_.world > 1 && get("native_xchg", 0) != 0 && get("links", 0) != 0;
    if (links_) {
      d_.import_max += (d_.world - 1) * d_.deliv_max;
      d_.pub_cap = ((d_.pub_max + d_.import_max + 63) / 64) * 64;
    }
    d_.msg_max = (u32)get("msg_max", 1u << 22);
    u32 ucap = next_pow2((u32)get("ucap", 8192));
    d_.ucap_mask = ucap - 1;
    d_.deliver_cap = (u32)get("deliver_cap", 4096);
    dcap_bytes_ = (u32)get("deliver_cap_bytes", 0);
    d_.chmap_size = next_pow2(d_.chpc * 2);
    u32 xhash = next_pow2(d_.x_max * 2);
    d_.xhash_mask = xhash - 1;
    u32 dhash = next_pow2((u32)get("dhash", 65536));
    d_.dhash_mask = dhash - 1;
    d_.tb_max = (u32)get("tb_max", 4096);
    d_.tb_pad = ((d_.tb_max + 15) / 16) * 16;
    hb_max_ = std::max<u32>(1, (u32)get("hb_max", 1024));          // headers binding rows (chana.mq.gpu.headers-bindings)
    hp_max_ = std::max<u32>(1, (u32)get("hp_max", 4ull * hb_max_));  // pairs of all of them
    d_.req_max = (u32)get("req_max", 65536);
    d_.hash_wildcard = (u32)get("hash_wildcard", 1);
    d_.frame_max_global = (u32)get("frame_max", 131072);
    d_.log_bytes = get("log_bytes", 1ull << 32);
    d_.log_block = get("log_block", 4ull << 20);
    d_.log_bytes = (d_.log_bytes / d_.log_block) * d_.log_block;
    d_.n_log_blocks = d_.log_bytes / d_.log_block;
    d_.ingress_cap = get("ingress_cap", 64ull << 20);
    d_.xfer_bytes = d_.world > 1 ? get("xfer_bytes", (d_.world - 1) * (d_.ingress_cap + 64))
                                 : (restore_max_ ? get("restore_bytes", 80ull << 20) : 0);
    // work buffer = this step's new bytes + the carries of the connections in the step.
    // carry_cap bounds one connection's (= the largest command assembled on the device,
    // e.g. a multi-MB message); carry_budget bounds their sum per step (the front end
    // gathers within it), so large carries do not multiply by seg_max
    carry_budget_ = std::min<u64>((u64)d_.seg_max * (d_.carry_cap + 64), get("carry_budget", 512ull << 20));
    d_.work_cap = d_.ingress_cap + carry_budget_;
    d_.work_cap = d_.work_cap > (3ull << 30) ? (3ull << 30) : d_.work_cap;  // u32 offsets
    if (d_.work_cap + d_.xfer_bytes + 8192 > (4ull << 30))
      throw std::runtime_error("work buffer + imported bytes must stay below 4 GiB (u32 offsets): lower ingress_cap");
    d_.egress_cap = get("egress_cap", 96ull << 20);
    // receive payload: the peers' publishes + (links) their link deliveries, each bounded
    // by the sender's egress budget
    d_.import_bytes = d_.xfer_bytes + (links_ ? (u64)(d_.world - 1) * d_.egress_cap : 0);
    if (d_.persist) {
      // a step's persist records: one 48-B header per enqueue (<= pair_max) and each
      // message's bytes once (<= the step's work buffer + what it imported), so the
      // packed buffer can never overflow (no fail-closed stop on a burst)
      const u64 need = d_.work_cap + d_.xfer_bytes + dl_h_.dead_bytes + 56ull * d_.pair_max + 4096;   // (+ the dead pass's messages)
      if (d_.persist_bytes < need) d_.persist_bytes = need;
      if (d_.persist_max < d_.pair_max) d_.persist_max = d_.pair_max;
    }
    if (d_.import_bytes + 8192 > (4ull << 30))
      throw std::runtime_error("import buffer must stay below 4 GiB (u32 offsets): lower ingress_cap / egress_cap");
    d_.ctrl_cap = get("ctrl_cap", 4ull << 20);
    d_.ring_pool = get("ring_pool", 1ull << 26);
    u32 fan_max = (u32)get("fan_max", 1u << 20);
    u32 dq_max = (u32)get("dq_max", 1u << 20);
    hopx_max_ = (u32)get("hopx_max", 1u << 16);   // exchange-to-exchange edges per source type (like fan_max)
    const u32 hopx_max = hopx_max_;
    u64 kpool = get("kpool", 16ull << 20);
    kpool_ = kpool;
    u32 nch = d_.c_max * d_.chpc;
    // pair key = queue << 1 | (source rank >= this rank) at world > 1: the pairs are
    // generated as (this rank's publishes, then imports in source-rank order) and the sort
    // is stable, so one key bit restores (source rank, connection, publish) order per queue
    // (imports from lower ranks, own publishes, higher ranks) -- 9 key bits at q_max 256
    // instead of q_bits + log2(world)
    d_.rank_bits = d_.world > 1 ? 1 : 0;
    d_.q_bits = bits_for(d_.q_max);
    if (d_.q_bits + d_.rank_bits > 32) throw std::runtime_error("q_max too large for sharded pair keys");
    d_.ch_bits = bits_for(nch);
    graph_enabled_ = get("graph", 1) != 0;
    // step IO copies.  copy_engine: 0 = runtime default (a blit kernel that spreads over
    // the whole GPU and, for the egress D2H, holds its CUs for the entire PCIe transfer,
    // stalling the next step's kernels), 1 = hipMemcpyDeviceToDeviceNoCU request,
    // 2 = our own egress copy kernel on copy_wgs workgroups only (stores straight into
    // mapped pinned memory), leaving the rest of the CUs to the step kernels
    // 3 = the egress D2H on an SDMA engine through HSA directly (no CUs involved)
    copy_mode_ = (int)get("copy_engine", 0);   // measured: blit 24.0 M msgs/s, kernel(16 WG) 19.1 M
    sdma_ = copy_mode_ == 1;
    copy_wgs_ = (u32)get("copy_wgs", 16);
    sdma_pref_ = cfg.contains("sdma_engine") ? cfg["sdma_engine"].cast<int>() : -1;
    // (measured: no step-period gain in bench.py, 45.9 / 46.4 vs 45.9 / 46.3 M msgs/s,
    // profiles/r6_sp/ -- the egress D2H shares the link; opt-in)
    h2d_split_cfg_ = get("h2d_split", 1) != 0;         // (on unless explicitly 0: with h2d_hsa, payloads >= h2d_split_min)
    h2d_split_min_ = get("h2d_split_min", 4u << 20);   // (tests lower it: every payload splits)
    wait_ms_ = (u32)get("wait_timeout_ms", 10000);
    sdma_split_ = cfg.contains("sdma_split") ? std::max(1, std::min(2, cfg["sdma_split"].cast<int>())) : 1;

    // a step's egress: deliveries and Basic.GetEmpty frames (k_dequeue's byte budget:
    // egress_cap), returns (each its publish's bytes from the work buffer with the reply
    // text, at most 72 bytes, in place of the ticket and flags: work_cap + 72 per publish),
    // one 21-byte confirm per channel, then the gather table of egress by reference (16-byte
    // aligned, one EgressRef per delivery)
    egress_alloc_ = d_.egress_cap + d_.work_cap + 72ull * d_.pub_max + (u64)nch * 21 + 4096 + 16ull * d_.deliv_max;
    d_.egress_alloc = egress_alloc_;
    if (egress_alloc_ + 8192 > (4ull << 30))
      throw std::runtime_error("egress buffer must stay below 4 GiB (u32 offsets): lower egress_cap / ingress_cap");

    // ---- allocations
    auto dev = [&](const char* name, size_t bytes) { return alloc(name, bytes, false); };
    auto hst = [&](const char* name, size_t bytes) { return alloc(name, bytes, true); };
    d_.ctr = (Counters*)dev("ctr", sizeof(Counters));
    // the two parities' work buffers and the ingress slots in one allocation, the slots
    // last: a u32 offset from either work buffer reaches them, so a segment without a
    // carry is scanned and read where its H2D put it (k_frame_scan in place: no work copy)
    {
      const u64 wb = (d_.work_cap + 4096 + 255) & ~255ull, ib = (d_.ingress_cap + 64 + 255) & ~255ull;
      u8* base = (u8*)dev("work_all", 2 * wb + INGRESS_SLOTS * ib);
      d_.work = (u8*)view("work", base, d_.work_cap + 4096);   // imports are read in place (k_import_route)
      work_p1_ = (u8*)view("work_p1", base + wb, d_.work_cap + 4096);
      for (int k = 0; k < INGRESS_SLOTS; ++k)
        ing_[k].buf = (u8*)view(("ingress_s" + std::to_string(k)).c_str(), base + 2 * wb + k * ib, d_.ingress_cap + 64);
    }
    // per-parity step IO: step t uses set t % npar_, so step t+1's H2D and step t-1's D2H
    // overlap step t's kernels (the graph of each parity is captured once)
    npar_ = (d_.world == 1 && get("overlap", 1) == 0 && get("parities", 2) >= 3) ? 3 : 2;
    // egress slots rotate per step independently of the IO parity: step t renders into
    // slot t % EGRESS_SLOTS, so its kernels only wait for the D2H of step t-3 (long done)
    // instead of step t-2's, which is still on the copy engine
    for (int e = 0; e < EGRESS_SLOTS; ++e) {
      std::string sfx = std::to_string(e);
      EgressSlot& es = eg_[e];
      es.dev = (u8*)dev(("egress" + sfx).c_str(), egress_alloc_);
      if (copy_mode_ == 2) {
        es.host = (u8*)mapped(&es.host_dev, "egress_host" + sfx, egress_alloc_);
      } else {
        es.host = (u8*)pinned(("egress_host" + sfx).c_str(), egress_alloc_);
      }
    }
    d_.carry = (u8*)dev("carry", (u64)d_.c_max * d_.carry_cap + 64);
    d_.carry_len = (u32*)dev("carry_len", 4ull * d_.c_max);
    d_.conn_paused = (u32*)dev("conn_paused", 4ull * d_.c_max);
    d_.conn_frame_max = (u32*)dev("conn_frame_max", 4ull * d_.c_max);
    d_.conn_vhost = (u32*)dev("conn_vhost", 4ull * d_.c_max);
    d_.conn_last_rx = (i64*)dev("conn_last_rx", 8ull * d_.c_max);
    d_.chmap = (u32*)dev("chmap", 4ull * d_.c_max * d_.chmap_size);
    d_.conn_ret_bytes = (u32*)dev("conn_ret_bytes", 4ull * d_.c_max);
    d_.conn_conf_bytes = (u32*)dev("conn_conf_bytes", 4ull * d_.c_max);
    d_.conn_dfirst = (u32*)dev("conn_dfirst", 4ull * d_.c_max);
    d_.conn_dlast = (u32*)dev("conn_dlast", 4ull * d_.c_max);
    wblock_h_ = (u32*)mapped(&d_.conn_wblock, "conn_wblock", 4ull * d_.c_max);
    d_.conn_total = (u32*)dev("conn_total", 4ull * d_.c_max);
    d_.conn_base = (u32*)dev("conn_base", 4ull * d_.c_max);

    d_.seg_start = (u32*)dev("seg_start", 4ull * d_.seg_max);
    d_.seg_total = (u32*)dev("seg_total", 4ull * d_.seg_max);
    d_.seg_cmd_base = (u32*)dev("seg_cmd_base", 4ull * d_.seg_max);
    d_.seg_npub = (u32*)dev("seg_npub", 4ull * d_.seg_max);
    d_.seg_nack = (u32*)dev("seg_nack", 4ull * d_.seg_max);
    // up to DEC_SEG_LDS segments k_decode numbers publishes / acks from the frame scan's
    // per-segment ordinals (segment prefix in LDS): no rank scan over the commands
    d_.rank_scan = d_.seg_max > DEC_SEG_LDS ? 1u : 0u;
    d_.scan_inplace = get("scan_in_place", 1) ? 1u : 0u;

    d_.cmds = (Cmd*)dev("cmds", sizeof(Cmd) * (u64)d_.cmd_max);
    d_.frags = (Frag*)dev("frags", sizeof(Frag) * ((u64)d_.frag_max + d_.import_max));
    d_.cmd_is_pub = (u32*)dev("cmd_is_pub", 4ull * d_.cmd_max);
    d_.cmd_is_ack = (u32*)dev("cmd_is_ack", 4ull * d_.cmd_max);
    d_.cmd_pub_rank = (u32*)dev("cmd_pub_rank", 4ull * d_.cmd_max);
    d_.cmd_ack_rank = (u32*)dev("cmd_ack_rank", 4ull * d_.cmd_max);

    d_.pubs = (Pub*)dev("pubs", sizeof(Pub) * (u64)d_.pub_cap);
    d_.pub_keyvec = (i8*)dev("pub_keyvec", (u64)d_.pub_cap * TOPIC_K + 64);
    d_.pub_kwoff = (u16*)dev("pub_kwoff", 2ull * TOPIC_WORDS * d_.pub_cap + 64);
    d_.pub_match = (u16*)dev("pub_match", 2ull * d_.pub_cap * (d_.tb_pad / 16) + 64);
    d_.pub_nq = (u32*)dev("pub_nq", 4ull * d_.pub_cap);
    d_.pub_qc = (u32*)dev("pub_qc", 4ull * PUB_QC * d_.pub_cap);
    d_.pub_slot = (u32*)dev("pub_slot", 4ull * d_.pub_cap);
    d_.pub_routed = (u32*)dev("pub_routed", 4ull * d_.pub_cap);
    d_.pub_pair_off = (u32*)dev("pub_pair_off", 4ull * d_.pub_cap);
    d_.pub_slot_off = (u32*)dev("pub_slot_off", 4ull * d_.pub_cap);
    d_.hop_q = (u32*)dev("hop_q", 4ull * d_.pair_max);
    d_.pub_routed_rank = (u32*)dev("pub_routed_rank", 4ull * d_.pub_cap);
    d_.pub_ret = (u32*)dev("pub_ret", 4ull * d_.pub_cap);
    d_.ret_list = (u32*)dev("ret_list", 4ull * d_.pub_cap);
    d_.pub_ret_sz = (u32*)dev("pub_ret_sz", 4ull * d_.pub_cap);
    d_.pub_ret_off = (u32*)dev("pub_ret_off", 4ull * d_.pub_cap);
    d_.conn_ret_min = (u32*)dev("conn_ret_min", 4ull * d_.c_max);
    u64 xw = d_.world > 1 ? (u64)d_.world * d_.pub_cap : 64;
    d_.q_owner = (u32*)dev("q_owner", 4ull * d_.q_max);
    d_.q_excl = (u32*)dev("q_excl", 4ull * d_.q_max);
    d_.dget = (DGet*)dev("dget", sizeof(DGet) * (u64)DGET_MAX);
    d_.conn_gempty = (u32*)dev("conn_gempty", 4ull * d_.c_max);
    d_.conn_gempty_ch = (u32*)dev("conn_gempty_ch", 4ull * d_.c_max);
    d_.pub_rmask = (u32*)dev("pub_rmask", 4ull * d_.pub_cap);
    d_.xp_cnt_off = (u32*)dev("xp_cnt_off", 4 * xw);
    d_.xp_byt_off = (u32*)dev("xp_byt_off", 4 * xw);
    // k_pack_scan: per-tile aggregates / prefixes (2 * WORLD_MAX values per 1024 publishes)
    d_.pk_agg = (u32*)dev("pk_agg", 4ull * 2 * WORLD_MAX * (ceil_div(d_.pub_max ? d_.pub_max : 1, 1024) + 1));
    d_.xs_base = (u32*)dev("xs_base", 8ull * WORLD_MAX);
    d_.xr_base = (u32*)dev("xr_base", 16ull * WORLD_MAX);
    d_.id_base = (u64*)dev("id_base", 8);
    d_.q_durable = (u32*)dev("q_durable", 4ull * d_.q_max);
    if (d_.persist) {
      d_.prec = (PersistRec*)dev("prec", sizeof(PersistRec) * (u64)d_.persist_max);
      d_.crec = (ConsumedRec*)dev("crec", sizeof(ConsumedRec) * (u64)d_.persist_max);
      d_.ps_size = (u32*)dev("ps_size", 4ull * d_.persist_max);
      d_.ps_off = (u32*)dev("ps_off", 4ull * d_.persist_max);
    }
    if (d_.world == 1 && restore_max_) {
      d_.recv_desc = (const RDesc*)dev("restore_desc", sizeof(RDesc) * (u64)restore_max_);
      d_.recv_pay = (const u8*)dev("restore_pay", d_.xfer_bytes + 64);
    }
    d_.acks = (Ack*)dev("acks", sizeof(Ack) * (u64)d_.ack_max);

    for (int k = 0; k < 2; ++k) {
      d_.pair_k[k] = (u32*)dev(k ? "pair_k1" : "pair_k0", 4ull * d_.pair_max);
      d_.pair_v[k] = (u32*)dev(k ? "pair_v1" : "pair_v0", 4ull * d_.pair_max);
    }
    d_.q_first = (u32*)dev("q_first", 4ull * d_.q_max);

    d_.x_hkey = (u64*)dev("x_hkey", 8ull * xhash);
    d_.x_hval = (i32*)dev("x_hval", 4ull * xhash);
    d_.x_type = (u32*)dev("x_type", 4ull * d_.x_max);
    d_.x_fan_off = (u32*)dev("x_fan_off", 4ull * d_.x_max);
    d_.x_fan_n = (u32*)dev("x_fan_n", 4ull * d_.x_max);
    d_.x_t_off = (u32*)dev("x_t_off", 4ull * d_.x_max);
    d_.x_t_n = (u32*)dev("x_t_n", 4ull * d_.x_max);
    d_.fan_q = (u32*)dev("fan_q", 4ull * fan_max);
    d_.x_fanx_off = (u32*)dev("x_fanx_off", 4ull * d_.x_max);
    d_.x_fanx_n = (u32*)dev("x_fanx_n", 4ull * d_.x_max);
    d_.fan_x = (u32*)dev("fan_x", 4ull * hopx_max);
    d_.d_x_off = (u32*)dev("d_x_off", 4ull * dhash);
    d_.d_x_n = (u32*)dev("d_x_n", 4ull * dhash);
    d_.d_x = (u32*)dev("d_x", 4ull * hopx_max);
    d_.d_key = (u64*)dev("d_key", 8ull * dhash);
    d_.d_exch = (i32*)dev("d_exch", 4ull * dhash);
    d_.d_kb_off = (u32*)dev("d_kb_off", 4ull * dhash);
    d_.d_kb_len = (u32*)dev("d_kb_len", 4ull * dhash);
    d_.d_q_off = (u32*)dev("d_q_off", 4ull * dhash);
    d_.d_q_n = (u32*)dev("d_q_n", 4ull * dhash);
    d_.d_q = (u32*)dev("d_q", 4ull * dq_max);
    d_.kpool = (u8*)dev("kpool", kpool);
    d_.t_queue = (u32*)dev("t_queue", 4ull * d_.tb_pad);
    d_.t_exch = (u32*)dev("t_exch", 4ull * d_.tb_pad);
    d_.t_kb_off = (u32*)dev("t_kb_off", 4ull * d_.tb_pad);
    d_.t_kb_len = (u32*)dev("t_kb_len", 4ull * d_.tb_pad);
    d_.t_flags = (u32*)dev("t_flags", 4ull * d_.tb_pad);
    d_.t_count = (u32*)dev("t_count", 16);
    {   // (until the first topology upload: every row, as before the count existed)
      const u32 all[4] = {d_.tb_pad, 0, 0, 0};
      HIPCHECK(hipMemcpy(d_.t_count, all, 16, hipMemcpyHostToDevice));
    }
    d_.t_expect = (i32*)dev("t_expect", 4ull * d_.tb_pad);
    d_.t_mat = (i8*)dev("t_mat", (u64)d_.tb_pad * TOPIC_K + 64);
    d_.t_woff = (u16*)dev("t_woff", 2ull * TOPIC_WORDS * d_.tb_pad + 64);
    d_.x_h_off = (u32*)dev("x_h_off", 4ull * d_.x_max);
    d_.x_h_n = (u32*)dev("x_h_n", 4ull * d_.x_max);
    d_.x_alt = (i32*)dev("x_alt", 4ull * d_.x_max);
    HIPCHECK(hipMemset(d_.x_alt, 0xff, 4ull * d_.x_max));   // (until the first topology upload: no alternates)
    d_.h_queue = (u32*)dev("h_queue", 4ull * hb_max_);
    d_.h_meta = (u32*)dev("h_meta", 4ull * hb_max_);
    d_.h_pair = (u32*)dev("h_pair", 4ull * hb_max_);
    d_.hp = (u32*)dev("hp", 4ull * HP_WORDS * hp_max_);

    d_.q_ring_off = (u64*)dev("q_ring_off", 8ull * d_.q_max);
    d_.q_ring_mask = (u64*)dev("q_ring_mask", 8ull * d_.q_max);
    d_.q_head = (u64*)dev("q_head", 8ull * d_.q_max);
    d_.q_tail = (u64*)dev("q_tail", 8ull * d_.q_max);
    d_.q_ttl = (i64*)dev("q_ttl", 8ull * d_.q_max);
    d_.q_cons_off = (u32*)dev("q_cons_off", 4ull * d_.q_max);
    d_.q_cons_n = (u32*)dev("q_cons_n", 4ull * d_.q_max);
    d_.q_rr = (u32*)dev("q_rr", 4ull * d_.q_max);
    d_.q_active = (u32*)dev("q_active", 4ull * d_.q_max);
    d_.q_cons = (u32*)dev("q_cons", 4ull * d_.cons_max);
    d_.ring = (Desc*)dev("ring", sizeof(Desc) * d_.ring_pool);
    d_.ring_top = (u64*)dev("ring_top", 8);
    d_.q_max_cap = (u64*)dev("q_max_cap", 8ull * d_.q_max);
    d_.q_limit = (u32*)dev("q_limit", 4ull * d_.q_max);
    if (d_.blimits) {
      d_.q_blimit = (u64*)dev("q_blimit", 8ull * d_.q_max);
      d_.q_bytes = (u64*)dev("q_bytes", 8ull * d_.q_max);
      d_.q_broom = (u32*)dev("q_broom", 4ull * d_.q_max);
    }
    if (d_.prio) {
      d_.q_prio = (u32*)dev("q_prio", 4ull * d_.q_max);
      d_.q_lane_base = (u32*)dev("q_lane_base", 4ull * d_.q_max);
    }
    if (d_.dlx) {
      dl_h_.q_dlx = (u32*)dev("q_dlx", 4ull * d_.q_max);
      dl_h_.q_dl_len = (u32*)dev("q_dl_len", 4ull * d_.q_max);
      dl_h_.q_dl_name = (u8*)dev("q_dl_name", 2ull * DLQ_STR * d_.q_max);
      dl_h_.ch_dead_upto = (u64*)dev("ch_dead_upto", 8ull * d_.c_max * d_.chpc);
      dl_h_.dead = (DeadItem*)dev("dead", sizeof(DeadItem) * (u64)dl_h_.dead_max);
      dl_h_.dead_n = (u32*)dev("dead_n", 16);
      dl_h_.dead_take = (DeadItem*)dev("dead_take", sizeof(DeadItem) * (u64)dl_h_.dead_max);
      dl_h_.dead_off = (u32*)dev("dead_off", 8ull * dl_h_.dead_max);
      dl_h_.dead_desc = (RDesc*)dev("dead_desc", sizeof(RDesc) * (u64)dl_h_.dead_max);
      dl_h_.dead_pay = (u8*)dev("dead_pay", dl_h_.dead_bytes + 64);
      dl_h_.dead_xchg = (u32*)dev("dead_xchg", 4ull * XC_WORDS);
      if (dl_h_.xdeath) {
        dl_h_.q_name = (u8*)dev("q_name", (u64)DLQ_STR * d_.q_max);
        dl_h_.q_name_len = (u32*)dev("q_name_len", 4ull * d_.q_max);
        dl_h_.dead_plen = (u32*)dev("dead_plen", 4ull * dl_h_.dead_max);
        dl_h_.dead_ban = (u32*)dev("dead_ban", 4ull * XD_ELEMS_MAX * dead_room_);
        dl_h_.dead_ban_n = (u32*)dev("dead_ban_n", 4ull * dead_room_);
      }
      DlState* dl = (DlState*)dev("dl_state", sizeof(DlState));
      HIPCHECK(hipMemcpy(dl, &dl_h_, sizeof(DlState), hipMemcpyHostToDevice));
      d_.dl = dl;
    }
    d_.q_enq_tail = (u64*)dev("q_enq_tail", 8ull * d_.q_max);
    d_.moves = (RingMove*)dev("moves", sizeof(RingMove) * (u64)d_.q_max);
    d_.defer_free = (u32*)dev("defer_free", 4ull * d_.pub_cap);

    d_.ch_confirm = (u32*)dev("ch_confirm", 4ull * nch);
    d_.ch_pub_cnt = (u32*)dev("ch_pub_cnt", 4ull * nch);
    d_.ch_pub_fail = (u32*)dev("ch_pub_fail", 4ull * nch);
    d_.ch_confirm_next = (u64*)dev("ch_confirm_next", 8ull * nch);
    d_.ch_next_tag = (u64*)dev("ch_next_tag", 8ull * nch);
    d_.ch_uhead = (u64*)dev("ch_uhead", 8ull * nch);
    d_.ch_ack_upto = (u64*)dev("ch_ack_upto", 8ull * nch);
    d_.ch_req_upto = (u64*)dev("ch_req_upto", 8ull * nch);
    d_.ch_mlo = (u32*)dev("ch_mlo", 4ull * nch);
    d_.ch_mhi = (u32*)dev("ch_mhi", 4ull * nch);
    d_.ch_prefetch = (u32*)dev("ch_prefetch", 4ull * nch);
    d_.ch_global = (u32*)dev("ch_global", 4ull * nch);
    d_.ch_flow = (u32*)dev("ch_flow", 4ull * nch);
    d_.ch_tx = (u32*)dev("ch_tx", 4ull * nch);
    d_.ch_num = (u32*)dev("ch_num", 4ull * nch);
    d_.ch_unacked = (u32*)dev("ch_unacked", 4ull * nch);
    d_.ch_win = (u32*)dev("ch_win", 4ull * nch);
    d_.ch_dirty = (u32*)dev("ch_dirty", 4ull * nch);
    d_.dirty_list = (u32*)dev("dirty_list", 4ull * nch);
    d_.n_dirty = (u32*)dev("n_dirty", 4);
    d_.def_list = (u32*)dev("def_list", 4ull * nch);
    d_.uwin = (USlot*)dev("uwin", sizeof(USlot) * (u64)nch * ucap);

    d_.cons_q = (u32*)dev("cons_q", 4ull * d_.cons_max);
    d_.cons_ch = (u32*)dev("cons_ch", 4ull * d_.cons_max);
    d_.cons_noack = (u32*)dev("cons_noack", 4ull * d_.cons_max);
    d_.cons_active = (u32*)dev("cons_active", 4ull * d_.cons_max);
    d_.cons_unacked = (u32*)dev("cons_unacked", 4ull * (d_.cons_max + 1));   // [cons_max]: Basic.Get
    d_.cons_tag_off = (u32*)dev("cons_tag_off", 4ull * d_.cons_max);
    d_.cons_tag_len = (u32*)dev("cons_tag_len", 4ull * d_.cons_max);
    d_.tpool = (u8*)dev("tpool", 256ull * d_.cons_max);

    d_.msgs = (MsgEnt*)dev("msgs", sizeof(MsgEnt) * (u64)d_.msg_max);
    d_.msg_free = (u32*)dev("msg_free", 4ull * d_.msg_max);
    d_.msg_free_top = (u32*)dev("msg_free_top", 4);
    d_.log = (u8*)dev("log", d_.log_bytes + 4096);
    d_.log_head = (u64*)dev("log_head", 8);
    d_.log_tail = (u64*)dev("log_tail", 8);
    d_.log_step_base = (u64*)dev("log_step_base", 8);
    d_.log_live = (i64*)dev("log_live", 8ull * d_.n_log_blocks);
    d_.live_bytes = (i64*)dev("live_bytes", 8);
    d_.id_next = (u64*)dev("id_next", 8);
    // cold-body spill ring in pinned host memory (mapped: kernels read / write it over PCIe)
    d_.spill_bytes = (get("spill_bytes", 0) / d_.log_block) * d_.log_block;
    d_.n_spill_blocks = d_.spill_bytes / d_.log_block;
    d_.spill_head = (u64*)dev("spill_head", 8);
    d_.spill_tail = (u64*)dev("spill_tail", 8);
    d_.spill_live = (i64*)dev("spill_live", 8ull * (d_.n_spill_blocks ? d_.n_spill_blocks : 1));
    d_.spill = d_.spill_bytes ? (u8*)hst("spill", d_.spill_bytes + 4096) : nullptr;
    d_.spill_host = d_.spill_bytes ? (u64)buf("spill").ptr : 0;
    d_.spill_tail_lag = (u64*)dev("spill_tail_lag", 8ull * SPILL_LAG);
    spill_moved_ = (unsigned long long*)dev("spill_moved", 8);
    d_.cold_live = (i64*)dev("cold_live", 8ull * COLD_SEGS);
    cold_recs_ = (ColdRec*)dev("cold_recs", sizeof(ColdRec) * COLD_BATCH);
    cold_cnt_ = (u32*)dev("cold_cnt", 16);
    cold_bytes_ = (unsigned long long*)dev("cold_bytes", 8);
    cold_end_ = (u64*)dev("cold_end", 8ull * d_.q_max);
    if (d_.spill_bytes && d_.world == 1) {   // (side operations)
      side_d_ = alloc("cold_side", sizeof(ColdRec) * COLD_BATCH + 64, true);
      side_h_ = buf("cold_side").ptr;
      side_live_h_ = (i64*)pinned("cold_side_live", 8ull * COLD_SEGS);
      HIPCHECK(hipEventCreateWithFlags(&ev_side_, hipEventDisableTiming));
    }
    d_.q_cold_lim = (u64*)dev("q_cold_lim", 8ull * d_.q_max);
    HIPCHECK(hipMemset(d_.q_cold_lim, 0xff, 8ull * d_.q_max));
    d_.q_spill_cur = (u64*)dev("q_spill_cur", 8ull * d_.q_max);
    d_.q_cold_cur = (u64*)dev("q_cold_cur", 8ull * d_.q_max);

    d_.deliv = (Deliv*)dev("deliv", sizeof(Deliv) * (u64)d_.deliv_max);
    {
      const u64 nrun = (u64)d_.q_max * RUNS_PER_Q;
      d_.runs = (Run*)dev("runs", sizeof(Run) * nrun);
      d_.q_nruns = (u32*)dev("q_nruns", 4ull * d_.q_max);
      d_.run_order = (u32*)dev("run_order", 4ull * nrun);
      d_.run_start = (u32*)dev("run_start", 4ull * nrun);
      u64 np2 = 1;
      while (np2 < nrun) np2 <<= 1;
      d_.run_key = (u64*)dev("run_key", 8ull * np2);
    }
    d_.dv_size = (u32*)dev("dv_size", 4ull * d_.deliv_max);
    d_.dv_off = (u32*)dev("dv_off", 4ull * d_.deliv_max);
    d_.ch_first = (u32*)dev("ch_first", 4ull * nch);

    d_.req = (ReqItem*)dev("req", sizeof(ReqItem) * (u64)d_.req_max);
    d_.req_n = (u32*)dev("req_n", 4);
    d_.req_q_n = (u32*)dev("req_q_n", 4ull * d_.q_max);

    ntiles_max_ = ceil_div(d_.pair_max, SORT_TILE);
    d_.hist = (u32*)dev("hist", 4ull * 2048 * ntiles_max_);        // up to 11-bit digits
    d_.hist_scan = (u32*)dev("hist_scan", 4ull * 2048 * ntiles_max_);
    {   // look-back scan state: status words for the largest scan, ticket/epoch
      u64 big = d_.pub_cap > d_.cmd_max ? d_.pub_cap : d_.cmd_max;
      big = big > d_.deliv_max ? big : d_.deliv_max;
      big = big > d_.c_max ? big : d_.c_max;
      scan_smax_ = ceil_div(big, SCAN_TILE) + 1;
      // 4 arrays x smax 4096-tiles, or 16 arrays x 4*smax 1024-tiles
      scan_status_ = (u64*)dev("scan_status", 8ull * 16 * (SCAN_TILE / 1024) * scan_smax_);
      scan_ctl_ = (u32*)dev("scan_ctl", 64);
      // the ingest half's command scan has its own look-back state (it may run next to a
      // scan of the previous step's routing half)
      scan_status_ing_ = (u64*)dev("scan_status_ing", 8ull * 16 * (SCAN_TILE / 1024) * scan_smax_);
      scan_ctl_ing_ = (u32*)dev("scan_ctl_ing", 64);
    }
    d_.tot = (u32*)dev("tot", 4ull * 128);
    d_.egress_budget = (u64*)dev("egress_budget", 8);
    gate_dummy_ = dev("gate_dummy", 64);
    h2d_dummy_ = pinned("h2d_dummy", 64);
    // Basic.Get: rendered frames + result, host-mapped (a stored body never exceeds the
    // carry, which bounds an assembled command)
    get_cap_ = (u64)d_.carry_cap + d_.carry_cap / 64 + 4096;
    get_out_h_ = (u8*)mapped(&get_out_dev_, "get_out", get_cap_);
    get_res_h_ = (GetRes*)mapped(&get_res_dev_, "get_res", sizeof(GetRes));
    // k_frame_scan phase timestamps (scripts/frame_scan_phases.py): off unless asked for --
    // each mark is a clock read plus a store on the block's critical path
    d_.dbg = get("fs_marks", 0) ? (u64*)dev("dbg", 8ull * 16 * d_.seg_max) : nullptr;

    // the step's ingest buffers exist once per parity: with overlap (world 1), parity
    // t+1's ingest half (k_stage .. k_decode) runs while parity t's routing / delivery half
    // still reads its own commands, publishes, bodies, counters and scratch totals
    dup(&DS::ctr, "ctr", sizeof(Counters));
    dup(&DS::tot, "tot", 4ull * 128);
    dup(&DS::egress_budget, "egress_budget", 8);
    dup(&DS::seg_start, "seg_start", 4ull * d_.seg_max);
    dup(&DS::seg_total, "seg_total", 4ull * d_.seg_max);
    dup(&DS::seg_cmd_base, "seg_cmd_base", 4ull * d_.seg_max);
    dup(&DS::seg_npub, "seg_npub", 4ull * d_.seg_max);
    dup(&DS::seg_nack, "seg_nack", 4ull * d_.seg_max);
    par1_.push_back([this](DS& io) { io.work = work_p1_; });   // (allocated with the ingress slots)
    dup(&DS::cmds, "cmds", sizeof(Cmd) * (u64)d_.cmd_max);
    dup(&DS::frags, "frags", sizeof(Frag) * ((u64)d_.frag_max + d_.import_max));
    dup(&DS::cmd_is_pub, "cmd_is_pub", 4ull * d_.cmd_max);
    dup(&DS::cmd_is_ack, "cmd_is_ack", 4ull * d_.cmd_max);
    dup(&DS::cmd_pub_rank, "cmd_pub_rank", 4ull * d_.cmd_max);
    dup(&DS::cmd_ack_rank, "cmd_ack_rank", 4ull * d_.cmd_max);
    dup(&DS::pubs, "pubs", sizeof(Pub) * (u64)d_.pub_cap);
    dup(&DS::pub_keyvec, "pub_keyvec", (u64)d_.pub_cap * TOPIC_K + 64);
    dup(&DS::pub_kwoff, "pub_kwoff", 2ull * TOPIC_WORDS * d_.pub_cap + 64);
    dup(&DS::acks, "acks", sizeof(Ack) * (u64)d_.ack_max);
    dup(&DS::dget, "dget", sizeof(DGet) * (u64)DGET_MAX);
    // native exchange (sharded steps driven by the native front end, csrc/core/frontend.cpp):
    // the engine owns the per-parity send / receive buffers and moves them itself (RCCL or
    // the host shared-memory backend); implies the pipelined (lagged) exchange
    native_x_ = d_.world > 1 && get("native_xchg", 0) != 0;
    if (native_x_) lag_ = xfer_set_ = true;
    if (links_) {
      d_.links = 1;
      d_.lk_cap = (u32)get("link_acks", 2ull * d_.deliv_max);
      d_.conn_link = (u32*)dev("conn_link", 4ull * d_.c_max);
      d_.conn_link_tq = (u32*)dev("conn_link_tq", 4ull * d_.c_max);
      d_.conn_link_epoch = (u32*)dev("conn_link_epoch", 4ull * d_.c_max);
      d_.link_conns = (u32*)dev("link_conns", 4ull * 64);
      d_.n_link_conns = (u32*)dev("n_link_conns", 4);
      d_.link_nbase = (u32*)dev("link_nbase", 4ull * d_.c_max);
      d_.link_bbase = (u32*)dev("link_bbase", 4ull * d_.c_max);
      d_.link_dbase = (u32*)dev("link_dbase", 4ull * WORLD_MAX);
      d_.q_link_owner = (u32*)dev("q_link_owner", 4ull * d_.q_max);
      d_.q_link_ch = (u32*)dev("q_link_ch", 4ull * d_.q_max);
      d_.q_link_epoch = (u32*)dev("q_link_epoch", 4ull * d_.q_max);
      d_.lk_cnt = (u32*)dev("lk_cnt", 4ull * WORLD_MAX);
      fill("q_link_ch", 0xff);
    }
    if (d_.persist)
      for (int k = 0; k < PSLOTS; ++k) {   // store-record slots, shared by the parities (rotating per step)
        const std::string ks = std::to_string(k);
        persist_h_[k] = (const u8*)mapped(&d_.ps_persist[k], "persist" + ks, d_.persist_bytes + 64);
        consumed_h_[k] = (const ConsumedRec*)mapped(&d_.ps_crec[k], "consumed" + ks,
                                                    sizeof(ConsumedRec) * (u64)d_.persist_max + 64);
      }
    // per-parity step IO on top of the shared state: step t uses set t % npar_, so step t+1's
    // H2D and step t-1's D2H overlap step t's kernels (the graph of each parity is captured once)
    for (int p = 0; p < npar_; ++p) {
      const std::string sfx = std::to_string(p);
      StepSlot& sp = par_[p];
      HostIO& io = sp.io;
      static_cast<DS&>(io) = d_;
      if (p == 1)
        for (auto& f : par1_) f(io);
      io.in = (StepIn*)dev(("in" + sfx).c_str(), sizeof(StepIn));
      io.segs = (const SegIn*)dev(("segs" + sfx).c_str(), sizeof(SegIn) * d_.seg_max);
      // ingress payloads rotate over INGRESS_SLOTS buffers by step (StepIn.ingress): the
      // next step's payload goes into a slot whose last reader (three steps back) is known
      // done, so an early H2D never waits on the GPU
      io.ingress = ing_[p].buf;
      // outputs: device buffers the kernels fill, host-mapped ones the host reads (their host
      // addresses resolved here, once: nothing on the step path looks a name up)
      io.seg_out = (SegOut*)dev(("seg_out_d" + sfx).c_str(), sizeof(SegOut) * d_.seg_max);
      io.seg_out_hh = (const SegOut*)mapped(&io.seg_out_h, "seg_out" + sfx, sizeof(SegOut) * d_.seg_max);
      io.ctr_host_h = (const Counters*)mapped(&io.ctr_host, "ctr_host" + sfx, sizeof(Counters));
      io.conn_out = (ConnOut*)dev(("conn_out_d" + sfx).c_str(), sizeof(ConnOut) * d_.c_max);
      io.conn_out_hh = (const ConnOut*)mapped(&io.conn_out_h, "conn_out" + sfx, sizeof(ConnOut) * d_.c_max);
      io.ctrl = (u8*)dev(("ctrl_d" + sfx).c_str(), d_.ctrl_cap);
      io.ctrl_hh = (const u8*)mapped(&io.ctrl_h, "ctrl" + sfx, d_.ctrl_cap);
      io.ctrl_rec = (CtrlRec*)dev(("ctrl_rec_d" + sfx).c_str(), sizeof(CtrlRec) * d_.seg_max * 2);
      io.ctrl_rec_hh = (const CtrlRec*)mapped(&io.ctrl_rec_h, "ctrl_rec" + sfx, sizeof(CtrlRec) * d_.seg_max * 2);
      io.grow_hh = (const RingMove*)mapped(&io.grow_h, "grow" + sfx, sizeof(RingMove) * GROW_MAX);
      io.conn_conf_hh = (const u32*)mapped(&io.conn_conf_h, "conn_conf" + sfx, 4ull * d_.c_max);
      io.xchg_h = (u32*)mapped(&io.xchg, "xchg" + sfx, 4ull * XC_WORDS);
      // the step's descriptors stay in host-mapped memory: k_stage reads them over PCIe
      // and writes the device copies (io.in / io.segs) the later kernels read.  Two H2D
      // copies per step were runtime blit kernels on a third hardware queue, ordered behind
      // the prefetched payload: ~50 us between the payload's arrival and the ingest
      sp.stage_in = (StepIn*)mapped(&io.in_h, "stage_in" + sfx, sizeof(StepIn));
      sp.stage_segs = (SegIn*)mapped(&io.segs_h, "stage_segs" + sfx, sizeof(SegIn) * d_.seg_max + 64);
      // deferred control writes ridden by this parity's steps (pack_deltas)
      sp.dl_h = (u8*)mapped(&io.delta_h, "delta" + sfx, DELTA_CAP);
      // Basic.Get on the step: the requests (H2D with the step) and their answers
      io.get_req = (const GetReq*)dev(("get_req" + sfx).c_str(), sizeof(GetReq) * GET_STEP_MAX);
      io.get_out_hh = (GetOut*)mapped(&io.get_out_h, "get_out" + sfx, sizeof(GetOut) * GET_STEP_MAX);
      sp.stage_gets = (GetReq*)pinned(("stage_gets" + sfx).c_str(), sizeof(GetReq) * GET_STEP_MAX);
      io.unpause_req = (const u32*)dev(("unpause_req" + sfx).c_str(), 4ull * UNPAUSE_STEP_MAX);
      sp.stage_unp = (u32*)pinned(("stage_unp" + sfx).c_str(), 4ull * UNPAUSE_STEP_MAX);
      if (native_x_) {
        sp.xs_desc = (u8*)dev(("xs_desc" + sfx).c_str(), 64ull * d_.xfer_desc_max + 64);
        sp.xs_pay = (u8*)dev(("xs_pay" + sfx).c_str(), d_.xfer_bytes + 64);
        sp.xr_desc = (u8*)dev(("xr_desc" + sfx).c_str(), 64ull * d_.import_max + 64);
        sp.xr_pay = (u8*)dev(("xr_pay" + sfx).c_str(), d_.import_bytes + 64);
      }
      if (links_) {
        sp.ls_desc = (u8*)dev(("ls_desc" + sfx).c_str(), 64ull * d_.deliv_max + 64);
        sp.ls_pay = (u8*)dev(("ls_pay" + sfx).c_str(), d_.egress_cap + 64);
        sp.lk_send = (u8*)dev(("lk_send" + sfx).c_str(), 16ull * d_.world * d_.lk_cap + 64);
        sp.rack = (u8*)dev(("rack" + sfx).c_str(), 16ull * d_.world * d_.lk_cap + 64);
      }
    }
    for (int p = 0; p < npar_; ++p) {   // (sharded engines have two parities) p packs into S[p], imports R[p^1]
      StepSlot& sp = par_[p];
      const StepSlot& other = par_[p ^ 1];
      if (native_x_) {
        sp.io.send_desc = (RDesc*)sp.xs_desc; sp.io.send_pay = sp.xs_pay;
        sp.io.recv_desc = (const RDesc*)other.xr_desc; sp.io.recv_pay = other.xr_pay;
      }
      if (links_) {
        sp.io.lsend_desc = (RDesc*)sp.ls_desc; sp.io.lsend_pay = sp.ls_pay; sp.io.lk_send = (AckRec*)sp.lk_send;
        sp.io.rack = (const AckRec*)other.rack;   // the acks of the exchange this parity imports
      }
    }
    if (copy_mode_ == 3) init_sdma();
    HIPCHECK(hipStreamCreateWithFlags(&s_comp_, hipStreamNonBlocking));
    HIPCHECK(hipStreamCreateWithFlags(&s_h2d_, hipStreamNonBlocking));
    // (non-overlapped single GPU, cfg h2d_alt) odd steps' ingress copies on a second stream:
    // consecutive steps' payloads need not wait for one stream's previous copy to retire
    if (d_.world == 1 && get("overlap", 1) == 0 && get("h2d_alt", 0) != 0)
      HIPCHECK(hipStreamCreateWithFlags(&s_h2d_alt_, hipStreamNonBlocking));
    // (non-overlapped single GPU, HSA egress, cfg h2d_hsa) ingress payloads queued on an SDMA
    // engine through HSA and waited for on the device (k_frame_scan's h2d_wait): consecutive steps' copies
    // run back to back, with no HIP marker / cross-queue barrier between them
    h2d_hsa_ = copy_mode_ == 3 && !sdma_ && d_.world == 1 && get("overlap", 1) == 0 && get("h2d_hsa", 0) != 0;
    if (h2d_hsa_)
      for (int k = 0; k < INGRESS_SLOTS; ++k)
        if (hsa_signal_create(0, 0, nullptr, &ing_[k].sig) != HSA_STATUS_SUCCESS ||
            hsa_signal_create(0, 0, nullptr, &ing_[k].sig2) != HSA_STATUS_SUCCESS)
          throw std::runtime_error("hsa_signal_create failed");
    // ingress payloads share the H2D stream: a stream of their own stalled the host for ~6 ms
    // in an early prefetch on some boxes (12+ MB copies; profiles/r4_summary.md)
    s_pre_ = s_h2d_;
    HIPCHECK(hipStreamCreateWithFlags(&s_d2h_, hipStreamNonBlocking));
    {   // the ingest half gets its own (high-priority) hardware queue: next to the routing
        // half of the previous step, not queued behind it
      int lo = 0, hi = 0;
      HIPCHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
      HIPCHECK(hipStreamCreateWithPriority(&s_ing_, hipStreamNonBlocking, hi));
    }
    for (int p = 0; p < npar_; ++p) {
      StepSlot& sp = par_[p];
      for (hipEvent_t* ev : {&sp.ev_ing, &sp.ev_pre, &sp.ev_rest, &sp.ev_h2d, &sp.ev_done, &sp.ev_a, &sp.ev_ext})
        HIPCHECK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    }
    for (IngressSlot& ig : ing_) HIPCHECK(hipEventCreateWithFlags(&ig.ev_read, hipEventDisableTiming));
    for (EgressSlot& es : eg_) HIPCHECK(hipEventCreateWithFlags(&es.ev_d2h, hipEventDisableTiming));
    // overlap (world 1): the step's ingest half runs on its own stream, next to the
    // previous step's routing / delivery half
    overlap_ = d_.world == 1 && get("overlap", 1) != 0;
    // egress by reference (StepIn.ref_back / ref_min): off unless the driver keeps its
    // ingress payloads for it (set_egress_ref)
    ref_back_ = cfg.contains("egress_ref_back") ? cfg["egress_ref_back"].cast<int>() : -1;
    if (ref_back_ > 64) throw std::runtime_error("egress_ref_back: at most 64 steps back");
    ref_min_ = (u32)get("egress_ref_min", 256);
    // egress_gate (HSA SDMA egress, overlapped steps): the step's D2H is queued on the SDMA
    // engine at launch, behind a gate signal the step's last kernel opens (final_step), sized
    // from the recent steps' egress (a host-issued tail copies the rest when a step renders
    // more) -- the host is off the render -> D2H path.  0: the D2H is issued by the host
    // after it saw the step finish (egress_copy)
    // (sharded ranks too: the step's last kernel -- phase B's -- opens the gate the same way)
    gated_ = copy_mode_ == 3 && get("egress_gate", 1) != 0;
    // ---- initial state
    fill("conn_dfirst", 0xff);
    fill("conn_ret_min", 0xff);
    fill("conn_dlast", 0xff);
    fill("x_hval", 0xff);
    fill("ch_mlo", 0xff);
    fill("d_exch", 0xff);
    std::vector<u32> fl(d_.msg_max);
    for (u32 i = 0; i < d_.msg_max; ++i) fl[i] = d_.msg_max - 1 - i;
    HIPCHECK(hipMemcpy(d_.msg_free, fl.data(), 4ull * d_.msg_max, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_.msg_free_top, &d_.msg_max, 4, hipMemcpyHostToDevice));
    HIPCHECK(hipDeviceSynchronize());
  }

  ~Engine() {
    x_stop(true);
    // a gated copy never outlives its gate: open every gate, so no SDMA queue waits forever
    // (a step that faulted before its last kernel), then let the copies finish
    if (copy_mode_ == 3)
      for (int e = 0; e < EGRESS_SLOTS; ++e) {
        EgressSlot& es = eg_[e];
        if (es.gate_sig.handle) hsa_signal_store_screlease(es.gate_sig, 0);
        if (es.sdma_pending || es.tail_pending) {
          try { sdma_wait(e); } catch (const std::exception&) {}   // (reported already)
        }
      }
    for (IngressSlot& ig : ing_)
      if (ig.sig.handle) {
        if (ig.hsa) (void)hsa_signal_wait_scacquire(ig.sig, HSA_SIGNAL_CONDITION_EQ, 0, 2000 * block_ticks_,
                                                    HSA_WAIT_STATE_BLOCKED);
        if (ig.split) (void)hsa_signal_wait_scacquire(ig.sig2, HSA_SIGNAL_CONDITION_EQ, 0, 2000 * block_ticks_,
                                                      HSA_WAIT_STATE_BLOCKED);
      }
    (void)hipStreamSynchronize(s_comp_);
    (void)hipStreamSynchronize(s_h2d_);
    if (s_h2d_alt_) (void)hipStreamSynchronize(s_h2d_alt_);
    (void)hipStreamSynchronize(s_pre_);
    for (IngressSlot& ig : ing_)
      if (ig.sig.handle) { hsa_signal_destroy(ig.sig); hsa_signal_destroy(ig.sig2); }
    (void)hipStreamSynchronize(s_d2h_);
    for (int p = 0; p < npar_; ++p) {
      StepSlot& sp = par_[p];
      if (sp.graph_exec) (void)hipGraphExecDestroy(sp.graph_exec);
      if (sp.graph_b) (void)hipGraphExecDestroy(sp.graph_b);
      (void)hipEventDestroy(sp.ev_a);
      (void)hipEventDestroy(sp.ev_ext);
      (void)hipEventDestroy(sp.ev_h2d);
      (void)hipEventDestroy(sp.ev_done);
    }
    for (EgressSlot& es : eg_) (void)hipEventDestroy(es.ev_d2h);
    if (ev_side_) (void)hipEventDestroy(ev_side_);
    if (s_x_) (void)hipStreamDestroy(s_x_);
    if (s_io_) (void)hipStreamDestroy(s_io_);
    (void)hipStreamDestroy(s_comp_);
    (void)hipStreamDestroy(s_h2d_);
    if (s_h2d_alt_) (void)hipStreamDestroy(s_h2d_alt_);
    (void)hipStreamDestroy(s_d2h_);
    for (auto& kv : bufs_) {
      if (kv.second.view) continue;
      if (kv.second.host) (void)hipHostFree(kv.second.ptr);
      else (void)hipFree(kv.second.ptr);
    }
  }

  // page-locked (not mapped into kernels) host buffer: DMA target/source
  void* pinned(const char* name, size_t bytes) {
    Buf b;
    b.bytes = bytes;
    b.host = true;
    HIPCHECK(hipHostMalloc(&b.ptr, bytes, hipHostMallocPortable));
    memset(b.ptr, 0, bytes);
    total_bytes_ += bytes;
    bufs_[name] = b;
    return b.ptr;
  }

  // ------------------------------------------------------------- buffers
  void* alloc(const char* name, size_t bytes, bool host) {
    Buf b;
    b.bytes = bytes;
    b.host = host;
    if (host) {
      HIPCHECK(hipHostMalloc(&b.ptr, bytes, hipHostMallocMapped | hipHostMallocPortable));
      memset(b.ptr, 0, bytes);
    } else {
      HIPCHECK(hipMalloc(&b.ptr, bytes));
      HIPCHECK(hipMemset(b.ptr, 0, bytes));
    }
    total_bytes_ += bytes;
    bufs_[name] = b;
    if (host) {
      void* dp = nullptr;
      HIPCHECK(hipHostGetDevicePointer(&dp, b.ptr, 0));
      return dp;
    }
    return b.ptr;
  }

  // a host-mapped buffer: its device address into *dptr, its host address back
  template <class D>
  void* mapped(D** dptr, const std::string& name, size_t bytes) {
    *dptr = (D*)alloc(name.c_str(), bytes, true);
    return bufs_[name].ptr;
  }

  // a named device range inside an allocation made with alloc()
  void* view(const char* name, void* ptr, size_t bytes) {
    Buf b;
    b.ptr = ptr;
    b.bytes = bytes;
    b.view = true;
    bufs_[name] = b;
    return ptr;
  }

  const Buf& buf(const std::string& name) const {
    auto it = bufs_.find(name);
    if (it == bufs_.end()) throw std::runtime_error("no buffer " + name);
    return it->second;
  }

  void fill(const std::string& name, int byte) {
    const Buf& b = buf(name);
    if (b.host) memset(b.ptr, byte, b.bytes);
    else HIPCHECK(hipMemset(b.ptr, byte, b.bytes));
  }

  void upload(const std::string& name, py::buffer data, size_t offset) {
    py::buffer_info info = data.request();
    size_t n = (size_t)info.size * info.itemsize;
    const Buf& b = buf(name);
    if (offset + n > b.bytes) throw std::runtime_error("upload overflows " + name);
    if (b.host) memcpy((u8*)b.ptr + offset, info.ptr, n);
    else io_copy((u8*)b.ptr + offset, info.ptr, n, hipMemcpyHostToDevice);
  }

  // table reads / writes from any host thread: on their own non-blocking stream (a
  // legacy-stream copy would conflict with a graph capture running on the stepper thread)
  void io_copy(void* dst, const void* src, size_t n, hipMemcpyKind k) {
    std::lock_guard<std::mutex> g(io_mu_);
    if (!s_io_) HIPCHECK(hipStreamCreateWithFlags(&s_io_, hipStreamNonBlocking));
    HIPCHECK(hipMemcpyAsync(dst, src, n, k, s_io_));
    HIPCHECK(hipStreamSynchronize(s_io_));
  }

  py::bytes download(const std::string& name, size_t offset, size_t n) {
    const Buf& b = buf(name);
    if (n == 0) n = b.bytes - offset;
    if (offset + n > b.bytes) throw std::runtime_error("download overflows " + name);
    std::string out(n, '\0');
    if (b.host) memcpy(&out[0], (u8*)b.ptr + offset, n);
    else io_copy(&out[0], (u8*)b.ptr + offset, n, hipMemcpyDeviceToHost);
    return py::bytes(out);
  }

  // zero-copy numpy view of a host-mapped buffer
  py::array host_view(const std::string& name) {
    const Buf& b = buf(name);
    if (!b.host) throw std::runtime_error(name + " is not host-mapped");
    return py::array(py::dtype("uint8"), {(py::ssize_t)b.bytes}, {(py::ssize_t)1}, b.ptr,
                     py::capsule(b.ptr, [](void*) {}));
  }

  py::dict info() const {
    py::dict o;
    o["c_max"] = d_.c_max; o["chpc"] = d_.chpc; o["q_max"] = d_.q_max; o["x_max"] = d_.x_max;
    o["cons_max"] = d_.cons_max; o["seg_max"] = d_.seg_max; o["carry_cap"] = d_.carry_cap;
    o["cmd_max"] = d_.cmd_max; o["pair_max"] = d_.pair_max; o["deliv_max"] = d_.deliv_max;
    o["msg_max"] = d_.msg_max; o["ucap"] = d_.ucap_mask + 1; o["deliver_cap"] = d_.deliver_cap;
    o["chmap_size"] = d_.chmap_size; o["xhash"] = d_.xhash_mask + 1; o["dhash"] = d_.dhash_mask + 1;
    o["tb_max"] = d_.tb_max; o["tb_pad"] = d_.tb_pad; o["log_bytes"] = d_.log_bytes;
    o["spill_bytes"] = d_.spill_bytes;
    o["hb_max"] = hb_max_; o["hp_max"] = hp_max_; o["hb_pairs"] = (u32)HB_PAIRS; o["kpool"] = kpool_;
    o["hop_qmax"] = (u32)HOP_QMAX; o["hop_xslots"] = (u32)HOP_XSLOTS; o["hopx_max"] = hopx_max_;
    o["ingress_cap"] = d_.ingress_cap; o["egress_cap"] = d_.egress_cap; o["ring_pool"] = d_.ring_pool;
    o["work_cap"] = d_.work_cap; o["total_bytes"] = total_bytes_; o["req_max"] = d_.req_max;
    o["carry_budget"] = carry_budget_;
    o["egress_alloc"] = egress_alloc_; o["pub_max"] = d_.pub_max;
    o["exchange_lag"] = lag_ ? 1 : 0;
    o["native_xchg"] = native_x_ ? 1 : 0;
    o["rccl_standin"] = (rccl_ && cmqx::RcclLib::get().standin) ? 1 : 0;   // (tests/rccl_standin: not RCCL)
    o["links"] = links_ ? 1 : 0;
    o["import_bytes"] = d_.import_bytes;
    o["world"] = d_.world; o["rank"] = d_.my_rank; o["import_max"] = d_.import_max; o["pub_cap"] = d_.pub_cap;
    o["copy_engine"] = copy_mode_ == 3 ? "hsa-sdma" : copy_mode_ == 2 ? "kernel" : (sdma_ ? "nocu" : "blit");
    o["copy_wgs"] = copy_wgs_;
    o["egress_gate"] = gated_ ? 1 : 0;
    o["egress_ref_back"] = ref_back_;
    o["egress_ref_min"] = ref_min_;
    o["egress_slots"] = EGRESS_SLOTS;
    o["parities"] = npar_;
    auto engine_no = [](bool used, u32 mask) { return used && mask ? __builtin_ctz(mask) : -1; };   // (one-bit masks)
    o["sdma_engine"] = engine_no(copy_mode_ == 3, (u32)sdma_engine_);
    o["sdma_engine2"] = engine_no(true, (u32)sdma_engine2_);
    o["h2d_hsa_engine"] = engine_no(h2d_hsa_, (u32)ing_engine_);
    o["h2d_hsa_engine2"] = engine_no(h2d_hsa_, (u32)ing_engine2_);
    o["egress_tail_engine"] = engine_no(copy_mode_ == 3, (u32)tail_engine_);
    o["h2d_split_min"] = h2d_split_min_;
    o["queue_limits"] = d_.limits;
    o["queue_limit_bytes"] = d_.blimits;
    o["priority_queues"] = d_.prio;
    o["dead_letter"] = d_.dlx; o["dead_max"] = dl_h_.dead_max; o["dead_bytes"] = dl_h_.dead_bytes; o["dead_room"] = dead_room_; o["x_death"] = dl_h_.xdeath;
    o["alternate_exchange"] = alt_ ? 1 : 0;
    o["persist"] = d_.persist; o["persist_max"] = d_.persist_max; o["persist_bytes"] = d_.persist_bytes;
    o["restore_max"] = restore_max_;
    o["xfer_desc_max"] = d_.xfer_desc_max; o["xfer_bytes"] = d_.xfer_bytes; o["world_max"] = WORLD_MAX;
    o["pk_tile"] = PK_TILE;   // publishes per k_pack_scan tile
    o["sizeof"] = py::dict(py::arg("StepIn") = sizeof(StepIn), py::arg("SegIn") = sizeof(SegIn),
                           py::arg("SegOut") = sizeof(SegOut), py::arg("Counters") = sizeof(Counters),
                           py::arg("CtrlRec") = sizeof(CtrlRec), py::arg("ConnOut") = sizeof(ConnOut),
                           py::arg("MsgEnt") = sizeof(MsgEnt), py::arg("Desc") = sizeof(Desc),
                           py::arg("USlot") = sizeof(USlot), py::arg("Deliv") = sizeof(Deliv),
                           py::arg("Pub") = sizeof(Pub), py::arg("Cmd") = sizeof(Cmd),
                           py::arg("RDesc") = sizeof(RDesc));
    return o;
  }

 private:
  // ---- configuration (fixed by the constructor)
  int device_ = 0;
  u32 n_cu_ = 256;   // compute units of the device (grid caps of the block-per-segment / group kernels)
  DS d_;
  bool graph_enabled_ = true;
  bool overlap_ = false;   // world 1: the ingest half on its own stream next to the previous routing half
  int npar_ = 2;           // per-step IO sets in use (of NPAR_MAX)
  bool lag_ = false, native_x_ = false, links_ = false;
  u32 restore_max_ = 0;
  u32 dead_room_ = 0;      // records one dead pass takes: min(import_max, dead_max)
  bool alt_ = false;       // alternate exchanges (cfg alternate_exchange): routing pass 0 runs its ALT instantiations
  DlState dl_h_{};         // host copy of DS.dl
  u64 carry_budget_ = 0;
  int copy_mode_ = 0;      // cfg copy_engine
  bool sdma_ = true;       // copy_engine 1: NoCU copy requests
  u32 copy_wgs_ = 16;
  u32 hopx_max_ = 1u << 16;   // capacity of fan_x / d_x (cfg hopx_max)
  u32 hb_max_ = 1024, hp_max_ = 4096;   // headers rows / pair pool (cfg hb_max, hp_max)
  u64 kpool_ = 0;             // key pool bytes (cfg kpool)
  int sdma_pref_ = -1, sdma_split_ = 1;
  bool gated_ = false;     // egress D2H queued at launch behind a gate (HSA SDMA)
  bool h2d_hsa_ = false;   // ingress payloads in GPU-mapped host memory go to an SDMA engine through HSA
  bool h2d_split_cfg_ = true;
  u64 h2d_split_min_ = 4u << 20;
  // payload copies so far: in two halves on two engines, whole on the ingress engine, by the
  // runtime (pageable memory / h2d_hsa off) -- a split that silently does not happen shows here
  u64 h2d_n_[3] = {0, 0, 0};
  u32 wait_ms_ = 10000;    // bounded_wait deadline
  int ref_back_ = -1;      // egress by reference: steps back a body may be referenced (-1 off)
  u32 ref_min_ = 256;      // smallest referenced body (smaller ones are cheaper inline)
 public:
  u32 dcap_bytes_ = 0;     // StepIn.dcap_bytes of the next submitted steps (deliver_cap_bytes)
 private:
  // ---- buffers
  std::map<std::string, Buf> bufs_;
  u64 total_bytes_ = 0;
  u64 egress_alloc_ = 0;
  u32 ntiles_max_ = 0;
  u64* scan_status_ = nullptr;
  u32* scan_ctl_ = nullptr;
  u64* scan_status_ing_ = nullptr;   // the ingest half's own look-back state
  u32* scan_ctl_ing_ = nullptr;
  u32 scan_smax_ = 0;
  u8* work_p1_ = nullptr;
  // parity 1's copies of the per-step buffers (parity 0 keeps d_'s)
  std::vector<std::function<void(DS&)>> par1_;
  template <class T>
  void dup(T* DS::*m, const char* name, size_t bytes) {
    T* p1 = (T*)alloc((std::string(name) + "_p1").c_str(), bytes, false);
    par1_.push_back([m, p1](DS& io) { io.*m = p1; });
  }
  u64 get_cap_ = 0;                  // Basic.Get between steps
  u8 *get_out_dev_ = nullptr, *get_out_h_ = nullptr;
  GetRes *get_res_dev_ = nullptr, *get_res_h_ = nullptr;
  const u8* persist_h_[PSLOTS] = {};            // store-record slots (persist)
  const ConsumedRec* consumed_h_[PSLOTS] = {};
  u32* wblock_h_ = nullptr;
  // ---- slots
  StepSlot par_[NPAR_MAX];
  EgressSlot eg_[EGRESS_SLOTS];
  IngressSlot ing_[INGRESS_SLOTS];
  StepSlot& par(int p) {
    if (p < 0 || p >= npar_) throw std::runtime_error("no such parity: " + std::to_string(p));
    return par_[p];
  }
  bool any_inflight() const {
    for (int p = 0; p < npar_; ++p)
      if (par_[p].inflight) return true;
    return false;
  }
  // ---- step path
  u64 seq_ = 0;
  hipStream_t s_comp_ = nullptr, s_h2d_ = nullptr, s_d2h_ = nullptr, s_ing_ = nullptr;
  hipStream_t s_pre_ = nullptr;       // payloads (= s_h2d_)
  hipStream_t s_h2d_alt_ = nullptr;   // odd steps' H2D (cfg h2d_alt)
  hipStream_t h2d_of(u64 step) const { return (s_h2d_alt_ && (step & 1)) ? s_h2d_alt_ : s_h2d_; }
  std::vector<GetReq> pend_gets_;     // Basic.Get requests for the next submit
  DeltaStage dl_;                     // deferred control writes for the next submit
  u32 spill_req_[3] = {0, 0, 0};      // stage_spill for the next submitted step (dl_.mu)
  bool h2d_fault_ = false, gate_fault_ = false, wait_failed_ = false;
  void* h2d_dummy_ = nullptr;         // pinned host word of inject_h2d_fault
  void* gate_dummy_ = nullptr;        // device word a faulted step's gate store lands in
  double ht_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // host_times() phases
  // ---- HSA copies (copy_engine 3)
  hsa_agent_t gpu_agent_{}, cpu_agent_{};
  hsa_amd_sdma_engine_id_t sdma_engine_{}, sdma_engine2_{}, tail_engine_{};
  hsa_amd_sdma_engine_id_t ing_engine_{}, ing_engine2_{};   // ingress; a split payload's second engine (0: no split)
  u64 spin_ticks_ = 0, block_ticks_ = 0;   // bounded_wait: active spin / blocked slice (timestamp ticks)
  u64 eg_hist_[4] = {0, 0, 0, 0};          // the last steps' egress bytes (spec_bytes)
  u32 eg_hist_i_ = 0;
  u64 eg_stats_[4] = {0, 0, 0, 0};
  // ---- exchange
  std::vector<u32> lag_recv_;
  u64 lag_stream_ = 0;
  bool xfer_set_ = false;
  std::unique_ptr<cmqx::RcclXchg> rccl_;
  std::unique_ptr<cmqx::ShmXchg> shm_;
  std::unique_ptr<cmqx::ShmXchg> cshm_;   // rccl + host shared-memory count exchange
  std::vector<int> xmembers_;
  int xtimeout_ms_ = 10000;
  bool xfailover_ = false;
  bool x_wait_ = false;              // phase B waits on the RCCL bulk transfer
  u64 xseq_ = 0;
  // asynchronous exchange (xchg_setup async=true): one job at a time on the exchange thread
  bool async_x_ = false;
  XchgWorker xw_;
  u32* xflag_h_ = nullptr;           // host-mapped [0] last finished job, [1] a device wait gave up
  u32* xflag_d_ = nullptr;
  std::mutex cap_mu_;                // graph captures vs the exchange thread's HIP calls
  hipStream_t s_x_ = nullptr;        // the shared-memory exchange's copies
  // ---- side operations, table IO
  static constexpr u32 COLD_BATCH = 1u << 16;   // cold records per pick / scan call
  SideBox side_;
  hipEvent_t ev_side_ = nullptr;
  void* side_h_ = nullptr;      // host-mapped: [count @0][ColdRec[] @64]
  void* side_d_ = nullptr;
  i64* side_live_h_ = nullptr;
  ColdRec* cold_recs_ = nullptr;
  u32* cold_cnt_ = nullptr;
  unsigned long long* cold_bytes_ = nullptr;
  unsigned long long* spill_moved_ = nullptr;
  u64* cold_end_ = nullptr;
  std::mutex io_mu_;
  hipStream_t s_io_ = nullptr;       // upload / download
  // ---- C API
  CmqEngineApi api_{};
  std::string err_;
 public:
  // ------------------------------------------------------------- step (pipelined)
  // submit(): stage step t's ingress on the H2D stream and launch parity t&1's graph on
  // the compute stream behind it.  wait_results(p) -> host-mapped SegOut/Counters/ConnOut
  // are valid; egress_copy(p) DMAs exactly the rendered bytes on the D2H stream;
  // egress_wait(p) -> egress_host(p) is valid.
  // defer: queue only the ingress H2D and return; launch(p) starts the step's kernels.  A
  // sharded driver uses the gap to run the previous step's exchange while this step's
  // bytes cross PCIe (the host waits on phase A of t-1, not on H2D(t) + phase A(t))
  int submit(py::buffer segs, u64 payload_ptr, u64 payload_len, i64 now_ms, u64 step, u64 id_ms,
             u32 worker, bool defer, u32 flags) {
    py::buffer_info si = segs.request();
    size_t sb = (size_t)si.size * si.itemsize;
    return submit_raw((const SegIn*)si.ptr, (u32)(sb / sizeof(SegIn)), payload_ptr, payload_len, now_ms, id_ms,
                      worker, defer, flags);
  }

  // step numbers are the engine's own submit sequence (latency histogram, message
  // publish step): identical whether Python or the native front end drives the steps
  int submit_raw(const SegIn* segp, u32 nseg, u64 payload_ptr, u64 payload_len, i64 now_ms, u64 id_ms,
                 u32 worker, bool defer = false, u32 sflags = 0) {
    HostTimer ht(&ht_[0]);
    Range rg("chanamq.step.submit");
    const size_t sb = (size_t)nseg * sizeof(SegIn);
    const u64 step = seq_;
    if (nseg > d_.seg_max) throw std::runtime_error("too many segments");
    if (payload_len > d_.ingress_cap) throw std::runtime_error("ingress payload exceeds ingress_cap");
    const int p = (int)(seq_ % (u64)npar_);
    StepSlot& sp = par_[p];
    if (sp.inflight) throw std::runtime_error("submit: results of the previous step of this parity not collected");
    HIPCHECK(hipEventSynchronize(sp.ev_h2d));  // staging buffers of step t-2 are free
    // the payload first: the H2D is the step's longest stage and nothing below changes what
    // it copies (the slot's last reader, step t - INGRESS_SLOTS, is finished: its results were
    // collected before step t-2's).  It may already be on its way (prefetch): then only the
    // step's descriptors follow it on the H2D stream
    const int is = (int)(seq_ % INGRESS_SLOTS);
    IngressSlot& ig = ing_[is];
    const bool pre = sp.pre;
    if (pre && (sp.pre_seq != step || sp.pre_ptr != payload_ptr || sp.pre_len != payload_len))
      throw std::runtime_error("submit: payload differs from the one prefetched for this step");
    sp.pre = false;
    {   // overlapped engines move payloads on their own stream (prefetches run ahead of the
        // small per-step copies there; the ingest half waits for both)
      hipStream_t ps = overlap_ ? s_pre_ : h2d_of(step);
      if (payload_len && !pre) ingress_copy(step, is, payload_ptr, payload_len, ps);
      else if (!payload_len) ig.hsa = false;
    }
    StepIn* in = sp.stage_in;
    *in = StepIn{};
    in->h2d_sig = ig.hsa ? (u64)&((amd_signal_t*)ig.sig.handle)->value : 0;
    in->h2d_sig2 = ig.hsa && ig.split ? (u64)&((amd_signal_t*)ig.sig2.handle)->value : 0;
    if (in->h2d_sig && h2d_fault_) {   // (tests) the step waits on a word no copy completes
      h2d_fault_ = false;
      *(volatile i64*)h2d_dummy_ = 1;
      in->h2d_sig = (u64)h2d_dummy_;
      in->h2d_sig2 = 0;
      in->h2d_polls = 4096;
    }
    sp.h2d_addr = in->h2d_sig;
    sp.h2d_addr2 = in->h2d_sig2;
    // the step's stream waits for the H2D stream only when a runtime copy of this step is on it
    sp.h2d_hip = !h2d_hsa_ || (payload_len && !ig.hsa) || !pend_gets_.empty();
    in->nseg = nseg;
    in->ref_back = ref_back_ >= 0 ? (u32)ref_back_ : ref_back_ == -2 ? REF_SPILL_ONLY : 0xffffffffu;
    in->ref_min = ref_min_;
    in->ingress_host = ref_back_ >= 0 && payload_len ? payload_ptr : 0;
    in->dcap_bytes = dcap_bytes_;
    in->flags = sflags;
    in->now_ms = now_ms;
    in->step = step;
    in->id_ms = id_ms;
    in->worker = worker;
    const int e = (int)(seq_ % EGRESS_SLOTS);
    EgressSlot& es = eg_[e];
    in->egress = (u64)es.dev;
    // the slot's previous D2H (step t - EGRESS_SLOTS, long finished) must be complete before
    // its gate is re-armed and its buffer rendered into again
    if (copy_mode_ == 3 && (es.sdma_pending || es.tail_pending)) { HostTimer t(&ht_[1]); sdma_wait(e); }
    es.spec = gated_ ? spec_bytes(eg_hist_, egress_alloc_) : 0;
    in->gate = 0;
    if (es.spec) {
      hsa_signal_store_screlease(es.gate_sig, 1);
      in->gate = (u64)&((amd_signal_t*)es.gate_sig.handle)->value;
      if (gate_fault_) {   // (tests) the last kernel opens a scratch word instead: the copy never starts
        gate_fault_ = false;
        in->gate = (u64)gate_dummy_;
      }
    }
    in->ingress = (u64)ig.buf;
    in->pslot = (u32)(seq_ % PSLOTS);
    sp.pslot = (int)in->pslot;
    sp.slot = e;
    sp.launch_seq = step;
    if (sb) memcpy(sp.stage_segs, segp, sb);
    // staged Basic.Get requests ride this step; their answers start out RETRY (a queue the
    // device cannot serve now leaves it so)
    in->nget = (u32)pend_gets_.size();
    if (in->nget) {
      memcpy(sp.stage_gets, pend_gets_.data(), sizeof(GetReq) * in->nget);
      for (u32 i = 0; i < in->nget; ++i) sp.io.get_out_hh[i] = GetOut{GS_RETRY, 0};
      HIPCHECK(hipMemcpyAsync((void*)sp.io.get_req, sp.stage_gets, sizeof(GetReq) * in->nget,
                              hipMemcpyHostToDevice, h2d_of(step)));
      pend_gets_.clear();
    }
    sp.nget = in->nget;
    {   // body tiering asked for by the control plane rides this step (k_dequeue)
      std::lock_guard<std::mutex> g(dl_.mu);
      in->spill_frac = spill_req_[0];
      in->spill_hot = spill_req_[1];
      in->spill_budget = spill_req_[2];
    }
    // the control writes staged so far (what fits one step) and the connections
    // unpaused with them: a connection resumed in this step finds every write staged
    // before its unpause applied (k_stage applies the writes first)
    u32 nunp = 0;
    in->delta_bytes = dl_.pack_deltas(sp.dl_h, sp.stage_unp, &nunp);
    in->nunp = nunp;
    sp.nunp = nunp;
    if (in->nunp)
      HIPCHECK(hipMemcpyAsync((void*)sp.io.unpause_req, sp.stage_unp, 4ull * in->nunp, hipMemcpyHostToDevice,
                              h2d_of(step)));
    sp.dl_step = in->delta_bytes;
    if (in->nunp) sp.h2d_hip = true;
    if (overlap_) HIPCHECK(hipEventRecord(sp.ev_pre, s_pre_));
    HIPCHECK(hipEventRecord(sp.ev_h2d, overlap_ ? s_h2d_ : h2d_of(step)));
    sp.inflight = true;
    sp.staged = true;
    ++seq_;
    if (!defer) launch(p);
    return p;
  }

  // Early ingress of the NEXT step (overlapped single-GPU steps): its payload crosses PCIe
  // while the current steps run -- the H2D stream only waits (on the GPU) for the ingest
  // half of the step two back, the last reader of this parity's ingress buffer -- so the
  // copy engine never idles between steps.  The step is then submit()ed with the same
  // payload.  false: not applicable (no overlap), nothing queued.
  // Up to two steps ahead: each call queues the payload of the next step not yet queued
  // (the next submit, then the one after it).
  bool prefetch(u64 payload_ptr, u64 payload_len) {
    if (d_.world != 1 || !payload_len) return false;   // (s_pre_ is s_h2d_: the step waits for it)
    Range rg("chanamq.step.prefetch");
    u64 tgt = seq_;
    if (par_[tgt % (u64)npar_].pre) {   // the next submit's payload is queued already: the one after it
      tgt = seq_ + 1;
      if (par_[tgt % (u64)npar_].pre) return false;
    }
    StepSlot& sp = par_[tgt % (u64)npar_];
    if (sp.staged) throw std::runtime_error("prefetch: this step's payload is already queued");
    if (payload_len > d_.ingress_cap) throw std::runtime_error("ingress payload exceeds ingress_cap");
    // the slot's last reader: the ingest of step tgt - INGRESS_SLOTS, collected by now in
    // the drivers' order (bench / front end prefetch t+1 once t-2 is finished); if not,
    // the copy waits for it on the GPU
    const int is = (int)(tgt % INGRESS_SLOTS);
    hipStream_t ps = overlap_ ? s_pre_ : h2d_of(tgt);
    ingress_copy(tgt, is, payload_ptr, payload_len, ps);
    sp.pre = true;
    sp.pre_seq = tgt;
    sp.pre_ptr = payload_ptr;
    sp.pre_len = payload_len;
    return true;
  }

  // the agent address of a payload in page-locked host memory (hipHostMalloc /
  // hipHostRegister), 0 for pageable memory (the runtime's copy stages that)
  static u64 ingress_src(u64 ptr) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, (const void*)ptr) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    return a.type == hipMemoryTypeHost && a.devicePointer ? (u64)a.devicePointer : 0;
  }

  // a step's payload into ingress slot is: on the HSA path (k_frame_scan waits for it on the
  // device) or as a runtime copy on stream ps (the step's stream waits for ev_h2d_)
  void ingress_copy(u64 step, int is, u64 ptr, u64 len, hipStream_t ps) {
    IngressSlot& ig = ing_[is];
    const u64 src = h2d_hsa_ ? ingress_src(ptr) : 0;
    if (src) {
      // the slot's last reader (step - INGRESS_SLOTS, collected long ago in the drivers'
      // order) and its copy are done before the signal is re-armed
      if (step >= INGRESS_SLOTS && ig.read_issued && hipEventQuery(ig.ev_read) != hipSuccess)
        HIPCHECK(hipEventSynchronize(ig.ev_read));
      if (ig.hsa) bounded_wait(ig.sig, -1, "ingress H2D");
      if (ig.split) bounded_wait(ig.sig2, -1, "ingress H2D");
      const u64 h1 = ingress_cut(len, h2d_split_min_, ing_engine2_ != 0);
      const bool split = h1 < len;
      hsa_signal_store_relaxed(ig.sig, 1);
      if (hsa_amd_memory_async_copy_on_engine(ig.buf, gpu_agent_, (const void*)src, cpu_agent_, h1, 0,
                                              nullptr, ig.sig, ing_engine_, true) != HSA_STATUS_SUCCESS)
        throw std::runtime_error("hsa_amd_memory_async_copy_on_engine (ingress) failed");
      if (split) {
        hsa_signal_store_relaxed(ig.sig2, 1);
        if (hsa_amd_memory_async_copy_on_engine(ig.buf + h1, gpu_agent_, (const void*)(src + h1), cpu_agent_,
                                                len - h1, 0, nullptr, ig.sig2, ing_engine2_,
                                                true) != HSA_STATUS_SUCCESS)
          throw std::runtime_error("hsa_amd_memory_async_copy_on_engine (ingress, second half) failed");
      }
      ig.hsa = true;
      ig.split = split;
      ++h2d_n_[split ? 0 : 1];
      return;
    }
    ++h2d_n_[2];
    if (step >= INGRESS_SLOTS && ig.read_issued && hipEventQuery(ig.ev_read) != hipSuccess)
      HIPCHECK(hipStreamWaitEvent(ps, ig.ev_read, 0));
    HIPCHECK(hipMemcpyAsync((void*)ig.buf, (const void*)ptr, len,
                            sdma_ ? hipMemcpyDeviceToDeviceNoCU : hipMemcpyHostToDevice, ps));
    ig.hsa = false;
    ig.split = false;
  }

  // Basic.Get requests for the next submitted step (validated by the caller: a local queue
  // of this rank, a channel slot of an open channel)
  void stage_gets(const GetReq* r, u32 n) {
    if (pend_gets_.size() + n > GET_STEP_MAX) throw std::runtime_error("stage_gets: more than GET_STEP_MAX per step");
    for (u32 i = 0; i < n; ++i) {
      if (r[i].q >= d_.q_max || r[i].chslot >= d_.c_max * d_.chpc) throw std::runtime_error("stage_gets: bad queue / channel");
      pend_gets_.push_back(r[i]);
    }
  }
  py::list get_out_py(int p) {
    const StepSlot& sp = par(p);
    const GetOut* go = sp.io.get_out_hh;
    py::list l;
    for (u32 i = 0; i < sp.nget; ++i) l.append(py::make_tuple(go[i].status, go[i].msg_count));
    return l;
  }

  // ---- deferred control writes (delta_stage.h): staged from any thread while steps run,
  // carried by the next submitted step.  Here only what needs the engine: names and limits
  void stage_write_buf(const std::string& name, py::buffer data, size_t offset) {
    py::buffer_info info = data.request();
    const size_t n = (size_t)info.size * info.itemsize;
    const Buf& b = buf(name);
    if (offset + n > b.bytes) throw std::runtime_error("stage_write overflows " + name);
    if (b.host) { memcpy((u8*)b.ptr + offset, info.ptr, n); return; }   // host-mapped: direct
    dl_.stage_write((u64)b.ptr + offset, (const u8*)info.ptr, n);
  }
  void stage_mark_dirty(u32 ch) {
    if (ch >= d_.c_max * d_.chpc) throw std::runtime_error("stage_mark_dirty: bad channel slot");
    dl_.stage_mark_dirty(ch);
  }
  void stage_unpause(u32 conn) {
    if (conn >= d_.c_max) throw std::runtime_error("stage_unpause: bad connection");
    dl_.stage_unpause(conn);
  }
  void stage_begin() { dl_.stage_begin(); }
  void stage_end() { dl_.stage_end(); }
  u64 dl_state(int which) { return dl_.dl_state(which); }
  py::tuple deltas_pending() {
    size_t nrec, nd;
    u64 nbytes;
    dl_.deltas_pending(&nrec, &nbytes, &nd);
    return py::make_tuple(nrec, nbytes, nd);
  }
  bool host_work() { return dl_.host_work() || side_.queued(); }
  // from the next submitted step on, every step moves queued bodies in the oldest frac/65536
  // of the HBM log (past the first `hot` entries of a queue with consumers) to the host
  // spill ring, at most `budget` bytes a step -- spill() without the pipeline drain; frac 0
  // stops it.  Any thread.
  void stage_spill(u32 frac, u32 hot, u32 budget) {
    if (!d_.spill_bytes) return;
    std::lock_guard<std::mutex> g(dl_.mu);
    spill_req_[0] = frac; spill_req_[1] = hot; spill_req_[2] = budget;
  }
  // between steps (the control plane holds the engine): apply what is staged now
  void flush_deltas() {
    if (!dl_.has_deltas()) return;
    if (any_inflight()) throw std::runtime_error("flush_deltas() between steps only");
    sync();
    while (dl_.has_deltas()) {
      if (!dl_.pack_deltas(par_[0].dl_h, nullptr, nullptr)) break;
      hipLaunchKernelGGL(k_apply_deltas, dim3(1), dim3(1024), 0, s_comp_, par_[0].io, par_[0].io.delta_h);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipStreamSynchronize(s_comp_));
    }
  }

  // second half of submit(): the kernels of the staged step of parity p
  void launch(int p) {
    StepSlot& sp = par(p);
    if (!sp.staged) throw std::runtime_error("launch: no staged step of this parity");
    sp.staged = false;
    const int e = sp.slot;
    EgressSlot& es = eg_[e];
    IngressSlot& ig = ing_[sp.launch_seq % INGRESS_SLOTS];
    // egress slot e (last used by step t-EGRESS_SLOTS) drained before this step's kernels
    // overwrite it; waited for only after this step's ingress H2D is queued, so the H2D
    // and the in-flight D2H overlap on their two SDMA engines
    if (copy_mode_ == 3 && es.sdma_pending) { HostTimer t(&ht_[1]); sdma_wait(e); }
    if (overlap_) {
      // ingest half on s_ing_: after this step's H2D and once parity p's buffers are free
      // (the routing half of step t-2); the routing half on s_comp_ behind it and behind
      // the previous step's routing half (stream order), as a single step would run
      // a side operation between the previous step's routing half and this step's ingest
      if (side_.queued()) {
        run_side(s_comp_);
        HIPCHECK(hipStreamWaitEvent(s_ing_, ev_side_, 0));
      }
      HIPCHECK(hipStreamWaitEvent(s_ing_, sp.ev_h2d, 0));
      HIPCHECK(hipStreamWaitEvent(s_ing_, sp.ev_pre, 0));
      if (sp.rest_issued) HIPCHECK(hipStreamWaitEvent(s_ing_, sp.ev_rest, 0));
      // control writes: applied between steps -- after the previous step's routing half
      if (sp.dl_step && par_[p ^ 1].rest_issued) HIPCHECK(hipStreamWaitEvent(s_ing_, par_[p ^ 1].ev_rest, 0));
      {
        HostTimer t(&ht_[2]);
        if (!sp.graph_ing) capture(s_ing_, &sp.graph_ing, [&] { launch_ingest(s_ing_, sp.io); });
        HIPCHECK(hipGraphLaunch(sp.graph_ing, s_ing_));
      }
      HIPCHECK(hipEventRecord(sp.ev_ing, s_ing_));
      HIPCHECK(hipStreamWaitEvent(s_comp_, sp.ev_ing, 0));
      if (es.d2h_issued) HIPCHECK(hipStreamWaitEvent(s_comp_, es.ev_d2h, 0));
      {
        HostTimer t(&ht_[2]);
        if (!sp.graph_rest) capture(s_comp_, &sp.graph_rest, [&] { launch_rest(s_comp_, sp.io); });
        HIPCHECK(hipGraphLaunch(sp.graph_rest, s_comp_));
      }
      HIPCHECK(hipEventRecord(sp.ev_rest, s_comp_));
      sp.rest_issued = true;
      // the ingress slot's last reader: the routing half (segments scanned in place)
      HIPCHECK(hipEventRecord(ig.ev_read, s_comp_));
      ig.read_issued = true;
      HIPCHECK(hipEventRecord(sp.ev_done, s_comp_));
      gated_copy(e);
      if (copy_mode_ == 2) {   // egress D2H right behind the step, sized on the device
        // (measured slower than the host-issued SDMA copy -- CU stores over PCIe stall
        // behind the next step's kernels: 8.7 vs 32.9 M msgs/s, profiles/r4_bench/pre_*)
        HIPCHECK(hipStreamWaitEvent(s_d2h_, sp.ev_rest, 0));
        hipLaunchKernelGGL(k_copy_out_dev, dim3(copy_wgs_), dim3(256), 0, s_d2h_, es.host_dev,
                           (const u8*)es.dev, (const Counters*)sp.io.ctr);
        HIPCHECK(hipEventRecord(es.ev_d2h, s_d2h_));
        es.d2h_issued = true;
        sp.eager_d2h = true;
      }
      return;
    }
    if (side_h_) run_side(s_comp_);
    if (sp.h2d_hip) HIPCHECK(hipStreamWaitEvent(s_comp_, sp.ev_h2d, 0));
    if (es.d2h_issued) HIPCHECK(hipStreamWaitEvent(s_comp_, es.ev_d2h, 0));
    if (d_.world > 1 && !xfer_set_) throw std::runtime_error("set_xfer_buffers() before the first sharded step");
    if (graph_enabled_) {
      if (!sp.graph_exec) capture(s_comp_, &sp.graph_exec, [&] { launch_main(s_comp_, sp.io); });
      HostTimer t(&ht_[2]);
      HIPCHECK(hipGraphLaunch(sp.graph_exec, s_comp_));
    } else {
      launch_main(s_comp_, sp.io);
    }
    if (d_.world == 1) {   // the ingress slot's last reader (a later prefetch into it waits for it)
      HIPCHECK(hipEventRecord(ig.ev_read, s_comp_));
      ig.read_issued = true;
    }
    if (d_.world > 1 && lag_) {
      HIPCHECK(hipEventRecord(sp.ev_a, s_comp_));
      sp.counts_ready = true;
      if (native_x_) {   // the front end runs the previous step's exchange, then launch_b(p)
        sp.b_due = true;
        return;
      }
      // phase B right behind phase A: imports the previous step's exchange
      recv_counts(sp, lag_recv_.size() == 2 * d_.world ? lag_recv_.data() : nullptr);
      lag_recv_.clear();
      if (lag_stream_) {
        HIPCHECK(hipEventRecord(sp.ev_ext, (hipStream_t)lag_stream_));
        HIPCHECK(hipStreamWaitEvent(s_comp_, sp.ev_ext, 0));
        lag_stream_ = 0;
      }
      run_phase_b(p);
    } else if (d_.world > 1) {
      HIPCHECK(hipEventRecord(sp.ev_a, s_comp_));
      sp.phase_a = true;
      sp.counts_ready = true;
    } else {
      HIPCHECK(hipEventRecord(sp.ev_done, s_comp_));
      gated_copy(e);   // (world 1, one stream: the whole step is one graph)
    }
  }

  // non-blocking: the launched step of parity p has finished (its results are readable)
  bool step_done(int p) {
    const StepSlot& sp = par(p);
    if (!sp.inflight || sp.staged || sp.phase_a || sp.b_due) return !sp.inflight;
    return hipEventQuery(sp.ev_done) == hipSuccess;
  }

  void wait_results(int p) {
    HostTimer ht(&ht_[3]);
    Range rg("chanamq.step.wait_results");
    StepSlot& sp = par(p);
    if (sp.phase_a || sp.b_due) throw std::runtime_error("wait_results: phase B of this sharded step not submitted");
    if (sp.staged) throw std::runtime_error("wait_results: step staged but never launched");
    HIPCHECK(hipEventSynchronize(sp.ev_done));
    sp.inflight = false;
    if (sp.h2d_addr) {   // (the device-side wait gives up after its poll budget: the step then ran on a stale slot)
      if (*(volatile const i64*)sp.h2d_addr != 0 || (sp.h2d_addr2 && *(volatile const i64*)sp.h2d_addr2 != 0)) {
        wait_failed_ = true;
        throw std::runtime_error("ingress copy of step " + std::to_string(sp.launch_seq) +
                                 " did not complete before its step ran (HSA SDMA copy lost)");
      }
    }
    // egress history of the gated copies' sizing (every finished step, idle ones too)
    const u64 n = sp.io.ctr_host_h->egress_bytes;
    eg_hist_[eg_hist_i_++ & 3] = n;
    eg_stats_[3] += n;
  }

  void sync() {
    HIPCHECK(hipStreamSynchronize(s_h2d_));
    if (s_h2d_alt_) HIPCHECK(hipStreamSynchronize(s_h2d_alt_));
    HIPCHECK(hipStreamSynchronize(s_pre_));
    HIPCHECK(hipStreamSynchronize(s_ing_));
    HIPCHECK(hipStreamSynchronize(s_comp_));
    HIPCHECK(hipStreamSynchronize(s_d2h_));
  }

  // seconds spent in each host phase since the last reset
  py::dict host_times(bool reset) {
    // (asynchronous exchange: "exchange" is the stepper's wait for the previous job,
    // "exchange_thread" and "exchange_counts" the exchange thread's time)
    static const char* names[9] = {"submit", "submit_sdma_wait", "submit_graph_launch", "wait_results",
                                   "egress_copy", "egress_wait", "exchange", "exchange_counts", "exchange_thread"};
    py::dict o;
    for (int i = 0; i < 9; ++i) { o[names[i]] = ht_[i]; if (reset) ht_[i] = 0; }
    return o;
  }

  // payload copies since construction, by path (a payload that should split and does not is
  // counted unsplit), and the engines the HSA path uses (-1: none)
  py::dict h2d_stats() const {
    py::dict o;
    o["split"] = h2d_n_[0]; o["unsplit"] = h2d_n_[1]; o["runtime"] = h2d_n_[2];
    o["engine"] = h2d_hsa_ && ing_engine_ ? __builtin_ctz((u32)ing_engine_) : -1;
    o["engine2"] = h2d_hsa_ && ing_engine2_ ? __builtin_ctz((u32)ing_engine2_) : -1;
    return o;
  }

  // delivery runs of the finished step of parity p (TS_NRUNS: k_dequeue's count, what
  // k_dv_write chooses its path by); a device read, for tests
  u32 step_runs(int p) {
    u32 v = 0;
    io_copy(&v, par(p).io.tot + TS_NRUNS, sizeof(v), hipMemcpyDeviceToHost);
    return v;
  }

  py::dict counters(int p) {
    const Counters& c = *par(p).io.ctr_host_h;
    py::dict o;
#define F(x) o[#x] = c.x
    F(n_cmds); F(n_frags); F(n_pubs); F(n_acks); F(n_ctrl); F(ctrl_bytes); F(n_pairs); F(n_deliv);
    F(egress_bytes); F(n_returns); F(n_confirm_frames); F(n_freed); F(n_requeue); F(n_unroutable);
    F(n_dropped_nomem); F(n_expired); F(n_routed_msgs); F(n_unknown_exchange); F(n_ring_full);
    F(n_acked); F(log_head); F(log_tail); F(msg_free_top); F(n_live_msgs);
    F(n_persist); F(n_consumed); F(persist_used); F(n_persist_overflow);
    F(live_bytes); F(n_grow); F(n_dget); F(spill_moved); F(n_ref); F(gath_off); F(ref_bytes);
    F(n_maxlen_dropped); F(n_maxlen_rejected);
    // (only with dead_letter on: off, a step's counters are the dict they were -- each entry is a
    // string and a hash on the host's per-step path, which the headline benchmark drives)
    if (d_.dlx) { F(n_dl_expired); F(n_dl_maxlen); F(n_dl_rejected); F(n_dl_unrouted); F(n_dl_dropped); F(n_dl_pending); }
    if (dl_h_.xdeath) F(n_dl_cycle);
    if (alt_) F(n_alt);
#undef F
    std::vector<u32> lat(c.lat_hist, c.lat_hist + LAT_BINS);
    o["lat_hist"] = lat;
    return o;
  }

  // ------------------------------------------------------------- egress
  u64 egress_copy(int p) {
    HostTimer ht(&ht_[4]);
    Range rg("chanamq.K5.egress_d2h");
    StepSlot& sp = par(p);
    const u64 n = sp.io.ctr_host_h->egress_bytes;
    const int e = sp.slot;
    EgressSlot& es = eg_[e];
    if (es.spec) {   // gated: the bulk is on its way already; the host only adds a tail
      if (n > es.spec) {
        const u64 off = es.spec;
        hsa_signal_store_screlease(es.tail_sig, 1);
        hsa_status_t st = hsa_amd_memory_async_copy_on_engine((u8*)es.host + off, cpu_agent_,
                                                              (u8*)es.dev + off, gpu_agent_, n - off, 0, nullptr,
                                                              es.tail_sig, tail_engine_, true);
        if (st != HSA_STATUS_SUCCESS) {
          hsa_signal_store_screlease(es.tail_sig, 0);
          throw std::runtime_error("hsa_amd_memory_async_copy_on_engine (egress tail) failed");
        }
        es.tail_pending = true;
        ++eg_stats_[1];
      }
      return n;
    }
    if (sp.eager_d2h) {   // already queued behind the step (launch)
      sp.eager_d2h = false;
      return n;
    }
    HIPCHECK(hipStreamWaitEvent(s_d2h_, sp.ev_done, 0));
    if (n && copy_mode_ == 3) {
      HIPCHECK(hipEventSynchronize(sp.ev_done));
      // sdma_split 2: large egress split over two SDMA engines, each part decrementing the
      // slot's signal once (measured slower on MI355X: 28.9 vs 38.6 M msgs/s, p99 6.6 ms,
      // profiles/r4_sdma_split.md -- off by default)
      const int k = (n >= (2u << 20) && sdma_engine2_) ? 2 : 1;
      if (!sdma_d2h(es, n, k, false)) throw std::runtime_error("hsa_amd_memory_async_copy_on_engine failed");
      es.sdma_pending = true;
      return n;
    }
    if (n && copy_mode_ == 2)
      hipLaunchKernelGGL(k_copy_out, dim3(copy_wgs_), dim3(256), 0, s_d2h_, es.host_dev,
                         (const u8*)es.dev, n);
    else if (n)
      HIPCHECK(hipMemcpyAsync(es.host, es.dev, n,
                              sdma_ ? hipMemcpyDeviceToDeviceNoCU : hipMemcpyDeviceToHost, s_d2h_));
    HIPCHECK(hipEventRecord(es.ev_d2h, s_d2h_));
    es.d2h_issued = true;
    return n;
  }

  void egress_wait(int p) { egress_wait_slot(par(p).slot); }

  // the slot's SDMA D2H (+ its tail) landed.  Reads the pending flags and leaves them as they
  // are: egress_ready runs on another thread than the stepper and must not write them; the
  // stepper's waits (sdma_wait, egress_wait_slot) clear them afterwards
  void sdma_landed(int e) {
    EgressSlot& es = eg_[e];
    if (es.sdma_pending) bounded_wait(es.sdma_sig, e, "egress D2H");
    if (es.tail_pending) bounded_wait(es.tail_sig, e, "egress tail D2H");
  }
  void sdma_wait(int e) {
    sdma_landed(e);
    eg_[e].sdma_pending = eg_[e].tail_pending = false;
  }

  // n bytes of egress slot es to the host on k SDMA engines, each part decrementing the slot's
  // completion signal once; gated: every part starts when the slot's gate opens.  false: the
  // runtime refused a part
  bool sdma_d2h(EgressSlot& es, u64 n, int k, bool gated) {
    hsa_signal_store_screlease(es.sdma_sig, k);
    const u64 half = egress_cut(n, k);
    for (int i = 0; i < k; ++i) {
      const u64 off = i ? half : 0, len = i ? n - half : half;
      if (hsa_amd_memory_async_copy_on_engine((u8*)es.host + off, cpu_agent_, (u8*)es.dev + off, gpu_agent_, len,
                                              gated ? 1 : 0, gated ? &es.gate_sig : nullptr, es.sdma_sig,
                                              i ? sdma_engine2_ : sdma_engine_, true) != HSA_STATUS_SUCCESS)
        return false;
    }
    return true;
  }

  // a copy's completion signal reaching 0: an active spin first (a step's egress lands
  // within its period; a blocked wait would add the interrupt wake-up to every delivery's
  // latency), then blocked waits up to the engine's wait deadline -- past it the copy is
  // declared lost: the slot's gate is opened (a gated copy that never saw its step's last
  // kernel would otherwise hold its SDMA queue forever) and the engine reports an error
  // (the front end's healthy() turns false, a sharded node fails over).  Was: an unbounded
  // active wait, a core spinning forever on a lost gate
  void bounded_wait(hsa_signal_t sig, int e, const char* what) {
    if (hsa_signal_wait_scacquire(sig, HSA_SIGNAL_CONDITION_EQ, 0, spin_ticks_, HSA_WAIT_STATE_ACTIVE) == 0) return;
    const auto t0 = std::chrono::steady_clock::now();
    while (hsa_signal_wait_scacquire(sig, HSA_SIGNAL_CONDITION_EQ, 0, block_ticks_, HSA_WAIT_STATE_BLOCKED) != 0) {
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(wait_ms_)) {
        if (e >= 0 && eg_[e].gate_sig.handle) hsa_signal_store_screlease(eg_[e].gate_sig, 0);
        wait_failed_ = true;
        throw std::runtime_error(std::string(what) + " of egress slot " + std::to_string(e) + " did not complete within " +
                                 std::to_string(wait_ms_) + " ms (gate never opened / copy lost)");
      }
    }
  }
  // fault injection (tests): the next submitted step's egress gate is never opened by its
  // last kernel (it stores to a scratch word instead), as after a step that died before it
  void inject_gate_fault() { gate_fault_ = true; }
  // (tests) the next step's ingress wait polls a word that never reaches 0 (HSA ingress only)
  void inject_h2d_fault() { h2d_fault_ = true; }
  bool wait_failed() const { return wait_failed_; }

  // gated egress counters: [gated copies, tail copies, bytes copied speculatively, bytes rendered]
  py::dict egress_stats() const {
    py::dict o;
    o["gated"] = gated_;
    o["gated_copies"] = eg_stats_[0];
    o["tail_copies"] = eg_stats_[1];
    o["spec_bytes"] = eg_stats_[2];
    o["egress_bytes"] = eg_stats_[3];
    return o;
  }

  // egress slot (host view "egress_host<slot>") of the step last submitted with parity p
  int egress_slot(int p) { return par(p).slot; }
  // egress by reference from the next submitted step on (StepIn.ref_back): bodies of the
  // last `back` steps' ingress payloads (-1: off; -2: only bodies in the host spill ring) of
  // at least min_bytes are not rendered;
  // the caller keeps those payloads unchanged until the delivering step's egress is sent
  void set_egress_ref(int back, u32 min_bytes) {
    if (back > 64) throw std::runtime_error("set_egress_ref: at most 64 steps back");
    ref_back_ = back == -2 ? -2 : back < 0 ? -1 : back;
    ref_min_ = min_bytes < 16 ? 16 : min_bytes;
  }
  // store-record slot (host views "persist<slot>" / "consumed<slot>") of that step
  int persist_slot(int p) { return par(p).pslot; }
  const u8* pslot_host(int p) { return persist_h_[par(p).pslot]; }   // (null without persistence)
  const ConsumedRec* cslot_host(int p) { return consumed_h_[par(p).pslot]; }

  // egress_wait_slot without touching engine state (any thread; the slot's D2H was
  // issued before the caller learnt of the slot)
  void egress_ready(int e) {
    if (copy_mode_ == 3) { sdma_landed(e); return; }
    if (eg_[e].d2h_issued) HIPCHECK(hipEventSynchronize(eg_[e].ev_d2h));
  }

  void egress_wait_slot(int e) {
    HostTimer ht(&ht_[5]);
    egress_ready(e);
    if (copy_mode_ == 3) eg_[e].sdma_pending = eg_[e].tail_pending = false;
  }

  // the egress D2H of slot e, queued now: starts when the step's last kernel opens the gate
  void gated_copy(int e) {
    EgressSlot& es = eg_[e];
    if (!es.spec) return;
    Range rg("chanamq.K5.egress_gated");
    // sdma_split 2: the speculative copy in two halves on two SDMA engines, both released by
    // the same gate, each decrementing the slot's completion signal once
    const u64 n = es.spec;
    const int k = (sdma_split_ > 1 && sdma_engine2_ && n >= (4u << 20)) ? 2 : 1;
    if (!sdma_d2h(es, n, k, true)) {
      hsa_signal_store_screlease(es.sdma_sig, 0);
      throw std::runtime_error("hsa_amd_memory_async_copy_on_engine (gated egress) failed");
    }
    es.sdma_pending = true;
    ++eg_stats_[0];
    eg_stats_[2] += es.spec;
  }

  // non-blocking: egress slot e's D2H (and tail) landed in host memory
  bool egress_done_slot(int e) {
    EgressSlot& es = eg_[e];
    if (copy_mode_ == 3) {
      if (es.sdma_pending && hsa_signal_load_scacquire(es.sdma_sig) != 0) return false;
      if (es.tail_pending && hsa_signal_load_scacquire(es.tail_sig) != 0) return false;
      es.sdma_pending = es.tail_pending = false;
      return true;
    }
    return !es.d2h_issued || hipEventQuery(es.ev_d2h) == hipSuccess;
  }

  // HSA agents of this device and of the host, an SDMA engine for GPU -> host copies
  void init_sdma() {
    if (hsa_init() != HSA_STATUS_SUCCESS) throw std::runtime_error("hsa_init failed");
    struct Ctx { std::vector<hsa_agent_t> gpus, cpus; } ctx;
    hsa_iterate_agents([](hsa_agent_t a, void* data) {
      hsa_device_type_t t;
      hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t);
      auto* c = (Ctx*)data;
      if (t == HSA_DEVICE_TYPE_GPU) c->gpus.push_back(a);
      else if (t == HSA_DEVICE_TYPE_CPU) c->cpus.push_back(a);
      return HSA_STATUS_SUCCESS;
    }, &ctx);
    if ((int)ctx.gpus.size() <= device_ || ctx.cpus.empty()) throw std::runtime_error("HSA agents not found");
    {   // bounded_wait: spin 2 ms actively, then block in 1 ms slices
      u64 f = 0;
      if (hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY, &f) != HSA_STATUS_SUCCESS || !f) f = 100000000ull;
      spin_ticks_ = f / 500;
      block_ticks_ = f / 1000;
    }
    gpu_agent_ = ctx.gpus[device_];
    cpu_agent_ = ctx.cpus[0];
    uint32_t mask = 0;
    if (hsa_amd_memory_copy_engine_status(cpu_agent_, gpu_agent_, &mask) != HSA_STATUS_SUCCESS || !mask)
      throw std::runtime_error("no SDMA engine available for device -> host copies");
    // which engine carries what: sdma_plan.h (with the defaults on MI355X: egress 1, tail 2,
    // ingress 0 and 3)
    const SdmaPlan pl = plan_sdma(mask, sdma_pref_, sdma_split_, h2d_split_cfg_);
    sdma_engine_ = (hsa_amd_sdma_engine_id_t)pl.egress;
    sdma_engine2_ = (hsa_amd_sdma_engine_id_t)pl.egress2;
    tail_engine_ = (hsa_amd_sdma_engine_id_t)pl.tail;
    ing_engine_ = (hsa_amd_sdma_engine_id_t)pl.ingress;
    ing_engine2_ = (hsa_amd_sdma_engine_id_t)pl.ingress2;
    for (EgressSlot& es : eg_)
      if (hsa_signal_create(0, 0, nullptr, &es.sdma_sig) != HSA_STATUS_SUCCESS ||
          hsa_signal_create(0, 0, nullptr, &es.tail_sig) != HSA_STATUS_SUCCESS ||
          hsa_signal_create(0, 0, nullptr, &es.gate_sig) != HSA_STATUS_SUCCESS)
        throw std::runtime_error("hsa_signal_create failed");
  }

  void drain_egress() {
    for (int e = 0; e < EGRESS_SLOTS; ++e) {
      sdma_wait(e);
      if (eg_[e].d2h_issued) HIPCHECK(hipEventSynchronize(eg_[e].ev_d2h));
    }
  }

  // ------------------------------------------------------------- exchange driven by the host (Python): send_counts / submit_b / set_import
  // sharded step, after submit(): wait for phase A and return the per-destination send
  // counts [records x world, bytes x world, overflow]
  std::vector<u32> send_counts(int p) {
    StepSlot& sp = par(p);
    if (!sp.counts_ready) throw std::runtime_error("send_counts: no phase-A step in flight for this parity");
    sp.counts_ready = false;
    HIPCHECK(hipEventSynchronize(sp.ev_a));
    const u32* x = sp.io.xchg_h;
    std::vector<u32> o;
    for (u32 r = 0; r < d_.world; ++r) o.push_back(x[r]);
    for (u32 r = 0; r < d_.world; ++r) o.push_back(x[WORLD_MAX + r]);
    o.push_back(x[4 * WORLD_MAX]);
    return o;
  }

  // sharded step: received [records x world, bytes x world]; the exchange ran on
  // `stream` (0 = already complete); launches phase B behind it
  void submit_b(int p, std::vector<u32> recv, u64 stream) {
    StepSlot& sp = par(p);
    if (!sp.phase_a) throw std::runtime_error("submit_b: no phase-A step in flight for this parity");
    if (recv.size() != 2 * d_.world) throw std::runtime_error("submit_b: need 2*world counts");
    recv_counts(sp, recv.data());
    if (stream) {
      HIPCHECK(hipEventRecord(sp.ev_ext, (hipStream_t)stream));
      HIPCHECK(hipStreamWaitEvent(s_comp_, sp.ev_ext, 0));
    }
    run_phase_b(p);
    sp.phase_a = false;
  }

  // received counts [records x world, bytes x world] (v null: nothing) into the words phase B
  // of a host-driven exchange reads (submit_b, exchange_lag's set_import)
  void recv_counts(StepSlot& sp, const u32* v) {
    u32* x = sp.io.xchg_h;
    for (u32 r = 0; r < d_.world; ++r) {
      x[2 * WORLD_MAX + r] = x[XC_RECV_AN + r] = v ? v[r] : 0;
      x[3 * WORLD_MAX + r] = x[XC_RECV_AB + r] = v ? v[d_.world + r] : 0;
    }
  }

  // phase B of parity p's step, behind whatever s_comp_ was made to wait for: its last kernel
  // finishes the step and opens the egress gate (sharded ranks gate too)
  void run_phase_b(int p) {
    StepSlot& sp = par_[p];
    if (graph_enabled_) {
      if (!sp.graph_b) capture(s_comp_, &sp.graph_b, [&] { launch_phase_b(s_comp_, sp.io); });
      HIPCHECK(hipGraphLaunch(sp.graph_b, s_comp_));
    } else {
      launch_phase_b(s_comp_, sp.io);
    }
    HIPCHECK(hipEventRecord(sp.ev_done, s_comp_));
    gated_copy(sp.slot);
  }

  // exchange_lag mode: the all-to-all of step t finished on `stream` (0 = complete) with
  // these received counts; the next submit()'s phase B imports it
  void set_import(std::vector<u32> recv, u64 stream) {
    if (recv.size() != 2 * d_.world) throw std::runtime_error("set_import: need 2*world counts");
    lag_recv_ = recv;
    lag_stream_ = stream;
  }

  // per-parity exchange operands (exchange_lag: parity p sends from S[p] and imports R[p^1])
  void set_xfer_parity(int p, u64 send_desc, u64 send_pay, u64 recv_desc, u64 recv_pay) {
    StepSlot& sp = par(p);
    sp.io.send_desc = (RDesc*)send_desc; sp.io.send_pay = (u8*)send_pay;
    sp.io.recv_desc = (const RDesc*)recv_desc; sp.io.recv_pay = (const u8*)recv_pay;
    drop_graphs(sp);
    xfer_set_ = true;
  }
  // (the captured graphs hold the old operands)
  void drop_graphs(StepSlot& sp) {
    if (sp.graph_exec) { HIPCHECK(hipGraphExecDestroy(sp.graph_exec)); sp.graph_exec = nullptr; }
    if (sp.graph_b) { HIPCHECK(hipGraphExecDestroy(sp.graph_b)); sp.graph_b = nullptr; }
  }

  // caller-owned exchange operands (device pointers, e.g. torch tensors used by RCCL)
  void set_xfer_buffers(u64 send_desc, u64 send_pay, u64 recv_desc, u64 recv_pay) {
    d_.send_desc = (RDesc*)send_desc; d_.send_pay = (u8*)send_pay;
    d_.recv_desc = (const RDesc*)recv_desc; d_.recv_pay = (const u8*)recv_pay;
    for (int p = 0; p < npar_; ++p) {
      StepSlot& sp = par_[p];
      sp.io.send_desc = d_.send_desc; sp.io.send_pay = d_.send_pay;
      sp.io.recv_desc = d_.recv_desc; sp.io.recv_pay = d_.recv_pay;
      drop_graphs(sp);
    }
    xfer_set_ = true;
  }

  // ------------------------------------------------------------- native exchange
  // Sharded steps driven by the native front end: submit(t) stages step t and launches its
  // phase A; exchange(parity of t-1) moves step t-1's cross-rank records (and the link
  // traffic of the step before) between the live ranks; launch_b(t) imports them.  The
  // count exchange carries a flags word per rank (control-sync request, busy), so
  // replicated control ops need no per-tick collective of their own.

  // kind "rccl": arg = 128-byte RCCL unique id; "shm": arg = shared-memory name.
  // members: the live logical ranks (sorted); timeout_ms bounds every host wait;
  // failover: the host also waits (bounded) for the bulk transfer before phase B
  // counts_shm (rccl only): a shared-memory name common to the group -- the per-step count
  // exchange then runs through host shared memory (a spin barrier, ~µs) instead of an
  // RCCL round trip with two PCIe copies; the bulk records stay on RCCL over xGMI.  All
  // ranks of one node (the bench, the sharded server on one host) can use it.
  void xchg_setup(const std::string& kind, const std::string& arg, std::vector<int> members, int timeout_ms,
                  bool failover, const std::string& counts_shm, bool async) {
    if (!native_x_) throw std::runtime_error("xchg_setup: engine built without native_xchg");
    for (int& m : members)
      if (m < 0 || m >= (int)d_.world) throw std::runtime_error("xchg_setup: bad member");
    std::sort(members.begin(), members.end());
    x_stop();   // (a job of the old group finished or failed: its phase B was released)
    if (!s_x_) {
      // high priority: the runtime takes a high-priority stream's hardware queue from a pool
      // of its own, so the exchange never shares a queue with s_comp_ -- where, with the
      // asynchronous exchange, phase B's k_xwait spins until this stream's transfer is done
      // (4 hardware queues per process: a sixth normal stream wraps onto s_comp_'s queue)
      int lo = 0, hi = 0;
      HIPCHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
      HIPCHECK(hipStreamCreateWithPriority(&s_x_, hipStreamNonBlocking, hi));
    }
    rccl_.reset();
    shm_.reset();
    cshm_.reset();
    xtimeout_ms_ = timeout_ms;
    xfailover_ = failover;
    if (kind == "rccl") {
      rccl_.reset(new cmqx::RcclXchg(arg, members, (int)d_.my_rank, timeout_ms));
      if (!counts_shm.empty()) cshm_.reset(new cmqx::ShmXchg(counts_shm, members, (int)d_.my_rank, 4096, timeout_ms));
    } else if (kind == "shm") {
      // a mailbox holds one rank's sends to every peer: records + payload
      // (+ with remote-consumer links: link delivery records, their payload and link acks,
      // as the receive side's import sizing already allows)
      size_t box = 64ull * d_.xfer_desc_max + d_.xfer_bytes + 16ull * (WORLD_MAX + 4) * 16;
      if (links_) box += 64ull * d_.deliv_max + d_.egress_cap + 16ull * d_.world * d_.lk_cap;
      shm_.reset(new cmqx::ShmXchg(arg, members, (int)d_.my_rank, box, timeout_ms));
    } else {
      throw std::runtime_error("xchg_setup: kind must be rccl or shm");
    }
    xmembers_ = members;
    xseq_ = 0;
    x_wait_ = false;
    lag_recv_.clear();
    async_x_ = async;
    if (async_x_) {
      if (!xflag_h_) {
        xflag_d_ = (u32*)alloc("xflag", 64, true);
        xflag_h_ = (u32*)buf("xflag").ptr;
      }
      __atomic_store_n(&xflag_h_[0], xw_.last_seq(), __ATOMIC_RELEASE);
      xw_.start([this](int q, u32 fl, u32 seq) { return x_run(q, fl, seq); },
                [this] { HIPCHECK(hipSetDevice(device_)); });
    }
  }

  static py::bytes xchg_unique_id() { return py::bytes(cmqx::rccl_unique_id()); }

  // the exchange of the launched step of parity q.  0: done (launch_b imports it);
  // -2: a peer did not answer within the timeout (nothing imported, retry impossible:
  // the caller drops it and fails over).  or_flags: OR of every member's flags.
  //
  // Asynchronous (xchg_setup async=true): the step's exchange is handed
  // to the exchange thread and the call returns the PREVIOUS exchange's result (rc, flags
  // OR) -- one step later, the same on every rank, so lockstep decisions stay identical --
  // after waiting for that job, which normally finished while the last step ran.  launch_b
  // queues phase B behind a device-side wait for its job (k_xwait), so the stepper submits
  // step t+1 while step t's counts and bulk transfer are in flight.  -2 from a finished job:
  // this step is not exchanged (the caller drops it); a failed job releases its phase B
  // with nothing to import.
  int exchange(int q, u32 flags, u32* or_flags) {
    if (!native_x_ || (!rccl_ && !shm_)) throw std::runtime_error("exchange: no native exchange set up");
    StepSlot& sq = par(q);
    if (!sq.counts_ready) throw std::runtime_error("exchange: no phase-A step of this parity");
    if (!async_x_) {
      const int rc = exchange_now(q, flags, or_flags, -1);
      if (rc == 0) sq.counts_ready = false;
      return rc;
    }
    HostTimer ht(&ht_[6]);
    int rc = 0;
    u32 orf = 0;
    x_collect(&rc, &orf);
    *or_flags = orf;
    if (rc) return rc;
    sq.counts_ready = false;
    // what the next phase B (parity q^1) imports starts out as nothing: the job writes the
    // counts when it succeeds; a phase B whose wait gives up imports nothing instead of the
    // counts parity q^1 held two steps ago.  (Its last reader, step t-2, has
    // finished: its results were collected before this step's submit)
    x_recv_counts(q ^ 1, nullptr);
    par_[q ^ 1].b_wait = xw_.post(q, flags);
    return 0;
  }

  // the last job's result (waits for it); (0, 0) when none is uncollected.  A phase B that
  // gave up is reported once the job in flight ended and ahead of its result (which stays)
  void x_collect(int* rc, u32* orf) {
    xw_.wait_idle();
    if (xflag_h_ && __atomic_load_n(&xflag_h_[1], __ATOMIC_ACQUIRE))
      throw std::runtime_error("a phase B gave up waiting for its exchange (exchange thread lost)");
    xw_.collect(rc, orf);
  }

  // one job of the exchange thread (xchg_worker.h: the order of what it publishes is the
  // contract): the exchange of parity q's step into parity q^1's import words
  XchgWorker::Result x_run(int q, u32 fl, u32 seq) {
    XchgWorker::Result r;
    try {
      std::lock_guard<std::mutex> cg(cap_mu_);
      r.rc = exchange_now(q, fl, &r.orf, q ^ 1);
    } catch (const std::exception& e) {
      r.rc = -1;
      r.err = e.what();
    }
    if (r.rc) x_recv_counts(q ^ 1, nullptr);   // phase B imports nothing
    __atomic_store_n(&xflag_h_[0], seq, __ATOMIC_RELEASE);
    return r;
  }

  // shutdown (abort true): a job still waiting for a peer gives up at once
  void x_stop(bool abort = false) {
    if (abort) xw_.stop([this] {
      if (shm_) shm_->abort();
      if (cshm_) cshm_->abort();
    });
    else xw_.stop();
    for (StepSlot& sp : par_) sp.b_wait = 0;
  }

  // what phase B of parity p imports: per rank [records, bytes, publish records, publish
  // bytes, link acks]; v null: nothing
  void x_recv_counts(int p, const u32* v) {
    u32* x = par_[p].io.xchg_h;
    for (u32 r = 0; r < d_.world; ++r) {
      x[XC_RECV_N + r] = v ? v[r] : 0;
      x[XC_RECV_B + r] = v ? v[d_.world + r] : 0;
      x[XC_RECV_AN + r] = v ? v[2 * d_.world + r] : 0;
      x[XC_RECV_AB + r] = v ? v[3 * d_.world + r] : 0;
      x[XC_RACK_N + r] = v ? v[4 * d_.world + r] : 0;
    }
  }

  // dst >= 0 (exchange thread): the received counts go straight into parity dst's xchg
  // words and the RCCL bulk transfer is waited for here, not by phase B's stream
  int exchange_now(int q, u32 flags, u32* or_flags, int dst) {
    Range rg("chanamq.X1.exchange");
    HostTimer ht(&ht_[dst >= 0 ? 8 : 6]);   // (async: the exchange thread's time)
    HIPCHECK(hipEventSynchronize(par_[q].ev_a));
    const u32* x = par_[q].io.xchg_h;
    if (x[XC_OVF]) throw std::runtime_error("cross-rank send buffers overflowed (xfer_desc_max / xfer_bytes)");
    const int n = (int)xmembers_.size();
    int me = 0;
    for (int i = 0; i < n; ++i)
      if (xmembers_[i] == (int)d_.my_rank) me = i;
    // send regions per destination rank: destination-major prefix over all ranks (k_pack_bases)
    u64 sbn[WORLD_MAX], sbb[WORLD_MAX];
    {
      u64 a = 0, b = 0;
      for (u32 r = 0; r < d_.world; ++r) { sbn[r] = a; sbb[r] = b; a += x[XC_SEND_N + r]; b += x[XC_SEND_B + r]; }
    }
    // link deliveries / acks of the step before (its phase B preceded this phase A): the
    // other parity's link buffers, destination-major (k_link_bases)
    const u32* xl = par_[q ^ 1].io.xchg_h;
    u64 lbn[WORLD_MAX], lbb[WORLD_MAX];
    u32 lnn[WORLD_MAX], lnb[WORLD_MAX], lnk[WORLD_MAX];
    {
      u64 a = 0, b = 0;
      for (u32 r = 0; r < d_.world; ++r) {
        lnn[r] = links_ ? xl[XC_LINK_N + r] : 0;
        lnb[r] = links_ ? xl[XC_LINK_B + r] : 0;
        lnk[r] = links_ ? std::min<u32>(xl[XC_ACK_N + r], d_.lk_cap) : 0;
        lbn[r] = a; lbb[r] = b;
        a += lnn[r]; b += lnb[r];
      }
    }
    std::vector<u32> hs((size_t)n * cmqx::XH_WORDS, 0), hr((size_t)n * cmqx::XH_WORDS, 0);
    for (int i = 0; i < n; ++i) {
      u32* h = &hs[(size_t)i * cmqx::XH_WORDS];
      const int r = xmembers_[i];
      if (i != me) {
        h[0] = x[XC_SEND_N + r]; h[1] = x[XC_SEND_B + r];
        h[2] = lnn[r]; h[3] = lnb[r]; h[4] = lnk[r];
      }
      h[5] = flags;
      h[6] = (u32)xseq_;
    }
    int rc;
    {
      Range rc_("chanamq.X1.counts");
      HostTimer hc(&ht_[7]);   // the host's blocking part: waiting for every peer's counts
      rc = cshm_ ? cshm_->counts(hs.data(), hr.data())
                 : rccl_ ? rccl_->counts(hs.data(), hr.data(), cmqx::XH_WORDS) : shm_->counts(hs.data(), hr.data());
    }
    if (rc) return rc;
    u32 orf = 0;
    for (int i = 0; i < n; ++i) {
      const u32* h = &hr[(size_t)i * cmqx::XH_WORDS];
      orf |= h[5];
      if (i != me && h[6] != (u32)xseq_)
        throw std::runtime_error("exchange out of lockstep with rank " + std::to_string(xmembers_[i]));
    }
    *or_flags = orf;
    // receive layout: sources in rank order, each [publish records | link records] and
    // [publish bytes | link bytes]
    u64 rn = 0, rb = 0, rk = 0;
    std::vector<u64> rbn(n), rbb(n), rbk(n);
    for (int i = 0; i < n; ++i) {
      const u32* h = &hr[(size_t)i * cmqx::XH_WORDS];
      rbn[i] = rn; rbb[i] = rb; rbk[i] = rk;
      if (i == me) continue;
      rn += (u64)h[0] + h[2];
      rb += (u64)h[1] + h[3];
      rk += h[4];
    }
    if (rn > d_.import_max || rb > d_.import_bytes || (rk && (!links_ || rk > (u64)(d_.world - 1) * d_.lk_cap)))
      throw std::runtime_error("exchange: received records exceed the import buffers");
    u8* R_d = par_[q].xr_desc;
    u8* R_p = par_[q].xr_pay;
    const u8* S_d = par_[q].xs_desc;
    const u8* S_p = par_[q].xs_pay;
    // link buffers: sent from the other parity (step t-1), received with this exchange
    const u8* L_d = links_ ? par_[q ^ 1].ls_desc : nullptr;
    const u8* L_p = links_ ? par_[q ^ 1].ls_pay : nullptr;
    const u8* K_s = links_ ? par_[q ^ 1].lk_send : nullptr;
    u8* RK = links_ ? par_[q].rack : nullptr;
    if (rccl_) {
      std::vector<std::vector<cmqx::XPart>> snd(n), rcv(n);
      for (int i = 0; i < n; ++i) {
        if (i == me) continue;
        const int r = xmembers_[i];
        const u32* h = &hr[(size_t)i * cmqx::XH_WORDS];
        // per peer, both sides in this order: publish records, link records, publish
        // payload, link payload, link acks
        snd[i].push_back({(void*)(S_d + 64 * sbn[r]), 64ull * x[XC_SEND_N + r]});
        if (links_) snd[i].push_back({(void*)(L_d + 64 * lbn[r]), 64ull * lnn[r]});
        snd[i].push_back({(void*)(S_p + sbb[r]), (u64)x[XC_SEND_B + r]});
        if (links_) {
          snd[i].push_back({(void*)(L_p + lbb[r]), (u64)lnb[r]});
          snd[i].push_back({(void*)(K_s + 16ull * d_.lk_cap * r), 16ull * lnk[r]});
        }
        rcv[i].push_back({(void*)(R_d + 64 * rbn[i]), 64ull * h[0]});
        if (links_) rcv[i].push_back({(void*)(R_d + 64 * (rbn[i] + h[0])), 64ull * h[2]});
        rcv[i].push_back({(void*)(R_p + rbb[i]), (u64)h[1]});
        if (links_) {
          rcv[i].push_back({(void*)(R_p + rbb[i] + h[1]), (u64)h[3]});
          rcv[i].push_back({(void*)(RK + 16 * rbk[i]), 16ull * h[4]});
        }
      }
      {
        Range rb_("chanamq.X1.bulk");
        rc = rccl_->bulk(snd, rcv);
      }
      if (rc) return rc;
      if (dst < 0) x_wait_ = true;   // (stepper thread only: the exchange thread never touches it)
      if (xfailover_ || dst >= 0) {   // bounded: a peer lost mid-transfer must not wedge the compute stream
        rc = rccl_->wait(rccl_->event());
        if (rc) return rc;
      }
    } else {
      // host backend: my sends into my mailbox (destination blocks), barrier, the blocks
      // addressed to me from every source's mailbox into the receive buffers
      Range rb_("chanamq.X1.bulk_shm");
      u8* box = shm_->box(me);
      uint64_t* dir = shm_->dir(me);
      u64 off = 0;
      for (int i = 0; i < n; ++i) {
        if (i == me) continue;
        const int r = xmembers_[i];
        dir[i] = off;
        const u64 nd = 64ull * x[XC_SEND_N + r], nb = x[XC_SEND_B + r];
        const u64 ld = 64ull * lnn[r], lb = lnb[r], kb = 16ull * lnk[r];
        if (off + nd + ld + nb + 16 + lb + kb > shm_->box_bytes())
          throw std::runtime_error("exchange: shm mailbox too small");
        if (nd) HIPCHECK(hipMemcpyAsync(box + off, S_d + 64 * sbn[r], nd, hipMemcpyDeviceToHost, s_x_));
        off += nd;
        if (ld) HIPCHECK(hipMemcpyAsync(box + off, L_d + 64 * lbn[r], ld, hipMemcpyDeviceToHost, s_x_));
        off += ld;
        if (nb) HIPCHECK(hipMemcpyAsync(box + off, S_p + sbb[r], nb, hipMemcpyDeviceToHost, s_x_));
        off += (nb + 15) & ~15ull;
        if (lb) HIPCHECK(hipMemcpyAsync(box + off, L_p + lbb[r], lb, hipMemcpyDeviceToHost, s_x_));
        off += (lb + 15) & ~15ull;
        if (kb) HIPCHECK(hipMemcpyAsync(box + off, K_s + 16ull * d_.lk_cap * r, kb, hipMemcpyDeviceToHost, s_x_));
        off += kb;
      }
      HIPCHECK(hipStreamSynchronize(s_x_));
      rc = shm_->barrier();
      if (rc) return rc;
      for (int i = 0; i < n; ++i) {
        if (i == me) continue;
        const u32* h = &hr[(size_t)i * cmqx::XH_WORDS];
        const u8* src = shm_->box(i) + shm_->dir(i)[me];
        const u64 nd = 64ull * h[0], nb = h[1], ld = 64ull * h[2], lb = h[3], kb = 16ull * h[4];
        if (nd + ld) HIPCHECK(hipMemcpyAsync(R_d + 64 * rbn[i], src, nd + ld, hipMemcpyHostToDevice, s_x_));
        src += nd + ld;
        if (nb) HIPCHECK(hipMemcpyAsync(R_p + rbb[i], src, nb, hipMemcpyHostToDevice, s_x_));
        src += (nb + 15) & ~15ull;
        if (lb) HIPCHECK(hipMemcpyAsync(R_p + rbb[i] + nb, src, lb, hipMemcpyHostToDevice, s_x_));
        src += (lb + 15) & ~15ull;
        if (kb) HIPCHECK(hipMemcpyAsync(RK + 16 * rbk[i], src, kb, hipMemcpyHostToDevice, s_x_));
      }
      HIPCHECK(hipStreamSynchronize(s_x_));
    }
    // what launch_b writes into the importing step's xchg: per rank [records, bytes,
    // publish records, publish bytes].  A local vector: on the exchange thread (dst >= 0)
    // the stepper's lag_recv_ must not be touched (unsynchronised vector writes)
    std::vector<u32> recv(5 * d_.world, 0);
    for (int i = 0; i < n; ++i) {
      if (i == me) continue;
      const int r = xmembers_[i];
      const u32* h = &hr[(size_t)i * cmqx::XH_WORDS];
      recv[r] = h[0] + h[2];
      recv[d_.world + r] = h[1] + h[3];
      recv[2 * d_.world + r] = h[0];
      recv[3 * d_.world + r] = h[1];
      recv[4 * d_.world + r] = h[4];
    }
    if (dst >= 0) x_recv_counts(dst, recv.data());
    else lag_recv_.swap(recv);
    ++xseq_;
    return 0;
  }

  // the launched step of parity q will not be exchanged (it packed nothing, or a peer
  // failed): the next phase B imports nothing
  // Asynchronous, collect (the stepper): also waits for the job in flight; -2 when it
  // failed (its phase B imported nothing), which the caller handles like a failed exchange.
  // A host-run step of the control plane (collect false) leaves the stepper's uncollected
  // result alone: it carries the flags every rank acts on at the same step.
  int drop_exchange(int q, bool collect = true) {
    par(q).counts_ready = false;
    if (!async_x_) {   // (asynchronous: the exchange thread's job owns no stepper state)
      lag_recv_.clear();
      x_wait_ = false;
    }
    if (!async_x_ || !collect) return 0;
    int rc = 0;
    u32 orf = 0;
    x_collect(&rc, &orf);
    return rc;
  }

  // phase B of the launched step of parity p, importing the last exchange (if any)
  void launch_b(int p) {
    StepSlot& sp = par(p);
    if (!sp.b_due) throw std::runtime_error("launch_b: no phase-A step of this parity");
    sp.b_due = false;
    if (async_x_) {   // behind its exchange job (the exchange thread writes the counts)
      const u32 w = sp.b_wait;
      sp.b_wait = 0;
      // give up only well past every bound the job itself has (counts barrier + bulk
      // barrier + the bulk's own wait, each xtimeout_ms) plus settle: then the job is lost
      const u64 lim = ((u64)xtimeout_ms_ * 3 + 5000) * 100000ull;   // s_memrealtime: 100 MHz
      if (w) hipLaunchKernelGGL(k_xwait, dim3(1), dim3(64), 0, s_comp_, (const u32*)xflag_d_, w, xflag_d_ + 1, lim,
                                sp.io.xchg, d_.world);
      else x_recv_counts(p, nullptr);
    } else {
      x_recv_counts(p, lag_recv_.size() == 5 * d_.world ? lag_recv_.data() : nullptr);
      lag_recv_.clear();
      if (x_wait_ && rccl_) HIPCHECK(hipStreamWaitEvent(s_comp_, rccl_->event(), 0));
      x_wait_ = false;
    }
    run_phase_b(p);
  }

  // ------------------------------------------------------------- side operations (between steps, or beside them)
  // cold bodies to the host spill ring, between steps: every queued message past the first
  // `hot` entries of its queue whose slot lies below log position `lim` (k_spill); returns
  // the bytes moved (the log tail advances over the emptied blocks at the next step)
  u64 spill(u64 lim, u32 hot) {
    if (!d_.spill_bytes) return 0;
    Range rg("chanamq.spill");
    between_steps("spill");
    HIPCHECK(hipMemsetAsync(spill_moved_, 0, 8, s_comp_));
    hipLaunchKernelGGL(k_spill, dim3(d_.q_max), dim3(256), 0, s_comp_, par_[0].io, lim, hot, spill_moved_);
    HIPCHECK(hipGetLastError());
    unsigned long long moved = 0;
    HIPCHECK(hipMemcpyAsync(&moved, spill_moved_, 8, hipMemcpyDeviceToHost, s_comp_));
    HIPCHECK(hipStreamSynchronize(s_comp_));
    return moved;
  }

  // ---- cold store (third body tier); the host moves the bytes.  Four operations, each either
  // between steps (cold_*: pipeline drained, on s_comp_) or beside them (side_cold_*, below)
  enum : int { SIDE_NONE = 0, SIDE_PICK, SIDE_COMMIT, SIDE_SCAN, SIDE_IN, SIDE_LIVE };
  // the kernel of one of them on stream s, with the memsets it needs; commit / in: op.n
  // records are in cold_recs_ already
  void launch_cold(const SideOp& op, hipStream_t s) {
    const HostIO& io = par_[0].io;
    switch (op.kind) {
      case SIDE_PICK:
        HIPCHECK(hipMemsetAsync(cold_cnt_, 0, 16, s));
        HIPCHECK(hipMemsetAsync(cold_bytes_, 0, 8, s));
        hipLaunchKernelGGL(k_cold_pick, dim3(d_.q_max), dim3(256), 0, s, io, op.a, op.b, op.c, cold_recs_, op.max_n,
                           cold_cnt_, cold_bytes_, op.max_bytes);
        break;
      case SIDE_SCAN:
        HIPCHECK(hipMemsetAsync(cold_cnt_, 0, 16, s));
        HIPCHECK(hipMemsetAsync(cold_end_, 0, 8ull * d_.q_max, s));
        hipLaunchKernelGGL(k_cold_scan, dim3(d_.q_max), dim3(64), 0, s, io, op.a, cold_recs_, op.max_n, cold_cnt_,
                           cold_end_);
        break;
      case SIDE_COMMIT:
        if (op.n) hipLaunchKernelGGL(k_cold_commit, blocks(op.n, 256), dim3(256), 0, s, io, cold_recs_, op.n);
        break;
      case SIDE_IN: {
        const u64 g = op.n > d_.q_max ? op.n : d_.q_max;
        hipLaunchKernelGGL(k_cold_in, blocks(g, 256), dim3(256), 0, s, io, cold_recs_, op.n, cold_end_);
        break;
      }
    }
  }
  // out: candidate records (ColdRec[], bytes 0 = skip) for the host to write to the store
  // (slots below spill tail + lim)
  py::bytes cold_pick(u32 hot, u64 lim, u32 max_n, u64 max_bytes) {
    if (!d_.spill_bytes) return py::bytes("");
    between_steps("cold_pick");
    if (max_n > COLD_BATCH) max_n = COLD_BATCH;
    launch_cold(SideOp{SIDE_PICK, hot, lim, 0, max_n, max_bytes, 0}, s_comp_);
    return cold_fetch(max_n);
  }
  // ... the host stored them (ColdRec.cold = store offsets): switch the messages over
  void cold_commit(py::buffer recs) {
    launch_cold(SideOp{SIDE_COMMIT, 0, 0, 0, 0, 0, cold_upload(recs)}, s_comp_);
    HIPCHECK(hipStreamSynchronize(s_comp_));
  }
  // in: the cold entries near the heads of the held queues, each with a spill-ring slot
  py::bytes cold_scan(u32 window, u32 max_n) {
    if (!d_.spill_bytes) return py::bytes("");
    between_steps("cold_scan");
    if (max_n > COLD_BATCH) max_n = COLD_BATCH;
    launch_cold(SideOp{SIDE_SCAN, window, 0, 0, max_n, 0, 0}, s_comp_);
    return cold_fetch(max_n);
  }
  // ... the host read their bodies into those slots: back to SPILL_BIT, q_cold_lim moved on
  void cold_in(py::buffer recs) {
    launch_cold(SideOp{SIDE_IN, 0, 0, 0, 0, 0, cold_upload(recs)}, s_comp_);
    HIPCHECK(hipStreamSynchronize(s_comp_));
  }
  // ---- the same four operations beside the steps (no pipeline drain, single GPU): the
  // cold thread posts one (side_*), the next launch() runs it on the compute stream between
  // two steps, side_wait() hands back its records; the steps keep flowing while the host
  // moves bodies between the ring and the store (the mailbox: side_box.h).  A pick is picked
  // up again by the commit only where its entry is still queued (k_cold_commit); k_cold_scan's
  // ring slots count as live until k_cold_in.  SIDE_LIVE copies cold_live (store segment GC).
  void side_post(int kind, u32 a, u64 b, u64 c, u32 max_n, u64 max_bytes, const ColdRec* recs, u32 n) {
    if (d_.world != 1) throw std::runtime_error("side operations: single-GPU engines only");
    if (!side_h_) throw std::runtime_error("side operations: no spill ring");
    side_.post(SideOp{kind, a, b, c, max_n > COLD_BATCH ? COLD_BATCH : max_n, max_bytes, n},
               [&] { if (n) memcpy((u8*)side_h_ + 64, recs, sizeof(ColdRec) * n); });
  }
  void side_cold_pick(u32 hot, u64 lim_rel, u64 min_used, u32 max_n, u64 max_bytes) {
    side_post(SIDE_PICK, hot, lim_rel, min_used, max_n, max_bytes, nullptr, 0);
  }
  void side_cold_scan(u32 window, u32 max_n) { side_post(SIDE_SCAN, window, 0, 0, max_n, 0, nullptr, 0); }
  void side_cold_commit(py::buffer recs) { side_recs(SIDE_COMMIT, recs); }
  void side_cold_in(py::buffer recs) { side_recs(SIDE_IN, recs); }
  void side_cold_live() { side_post(SIDE_LIVE, 0, 0, 0, 0, 0, nullptr, 0); }
  void side_recs(int kind, py::buffer recs) {
    py::buffer_info bi = recs.request();
    side_post(kind, 0, 0, 0, 0, 0, (const ColdRec*)bi.ptr, cold_batch(bi));
  }
  bool side_pending() { return side_.pending(); }
  // launch(): the posted operation on stream s, ahead of the step's kernels
  void run_side(hipStream_t s) {
    const std::optional<SideOp> op = side_.begin_launch();
    if (!op) return;
    ColdRec* hrecs = (ColdRec*)((u8*)side_h_ + 64);
    ColdRec* drecs = (ColdRec*)((u8*)side_d_ + 64);
    switch (op->kind) {
      case SIDE_PICK:
      case SIDE_SCAN:
        launch_cold(*op, s);
        hipLaunchKernelGGL(k_side_out, dim3(64), dim3(256), 0, s, (const ColdRec*)cold_recs_, (const u32*)cold_cnt_,
                           op->max_n, (u32*)drecs, (u32*)side_d_);
        break;
      case SIDE_COMMIT:
      case SIDE_IN:
        if (op->n) HIPCHECK(hipMemcpyAsync(cold_recs_, hrecs, sizeof(ColdRec) * op->n, hipMemcpyHostToDevice, s));
        launch_cold(*op, s);
        break;
      case SIDE_LIVE:
        HIPCHECK(hipMemcpyAsync(side_live_h_, d_.cold_live, 8ull * COLD_SEGS, hipMemcpyDeviceToHost, s));
        break;
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(ev_side_, s));
    side_.launched();
  }
  // the posted operation's result once it ran: ColdRec[] (pick / scan), cold_live bytes
  // (live), b"" (commit / in); None while it has not finished within timeout_s
  py::object side_wait(double timeout_s) {
    int kind = SIDE_NONE;
    hipError_t err = hipSuccess;
    bool done = false;
    {
      py::gil_scoped_release nogil;   // (no Python objects in here)
      const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds((i64)(timeout_s * 1e6));
      kind = side_.wait_launched(until);
      while (kind) {
        err = hipEventQuery(ev_side_);
        if (err == hipSuccess) { done = true; break; }
        if (err != hipErrorNotReady || std::chrono::steady_clock::now() > until) break;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
      }
    }
    if (err != hipSuccess && err != hipErrorNotReady) HIPCHECK(err);
    if (!done) return py::none();
    side_.clear();
    if (kind == SIDE_PICK || kind == SIDE_SCAN) {
      const u32 n = *(volatile u32*)side_h_;
      return py::bytes((const char*)side_h_ + 64, sizeof(ColdRec) * (size_t)n);
    }
    if (kind == SIDE_LIVE) return py::bytes((const char*)side_live_h_, 8ull * COLD_SEGS);
    return py::bytes("");
  }

  // the operations that need the pipeline drained: no step in flight, no exchange pending
  void between_steps(const char* what) {
    if (any_inflight()) throw std::runtime_error(std::string(what) + "() between steps only");
    for (int p = 0; native_x_ && p < npar_; ++p)
      if (par_[p].counts_ready) throw std::runtime_error(std::string(what) + "() with an exchange pending");
    sync();
  }
  py::bytes cold_fetch(u32 max_n) {
    u32 n = 0;
    HIPCHECK(hipMemcpyAsync(&n, cold_cnt_, 4, hipMemcpyDeviceToHost, s_comp_));
    HIPCHECK(hipStreamSynchronize(s_comp_));
    if (n > max_n) n = max_n;
    std::string out(sizeof(ColdRec) * (size_t)n, '\0');
    if (n) HIPCHECK(hipMemcpy(&out[0], cold_recs_, out.size(), hipMemcpyDeviceToHost));
    return py::bytes(out);
  }
  // a ColdRec[] batch from Python: its record count
  static u32 cold_batch(const py::buffer_info& bi) {
    const size_t nb = (size_t)bi.size * bi.itemsize;
    if (nb % sizeof(ColdRec) || nb / sizeof(ColdRec) > COLD_BATCH) throw std::runtime_error("cold: bad ColdRec batch");
    return (u32)(nb / sizeof(ColdRec));
  }
  u32 cold_upload(py::buffer recs) {
    py::buffer_info bi = recs.request();
    const u32 n = cold_batch(bi);
    if (n) HIPCHECK(hipMemcpy(cold_recs_, bi.ptr, sizeof(ColdRec) * (size_t)n, hipMemcpyHostToDevice));
    return n;
  }

  // recovery: enqueue store records (RDesc with MF_RESTORE, payload [ex][rk][props][body])
  // through the import path, between steps; returns the number of messages enqueued
  u32 restore(py::buffer desc, py::buffer pay, i64 now_ms) {
    py::buffer_info di = desc.request(), pi = pay.request();
    u64 db = (u64)di.size * di.itemsize, pb = (u64)pi.size * pi.itemsize;
    if (db % sizeof(RDesc)) throw std::runtime_error("restore: descriptors are no whole records");
    u32 n = (u32)(db / sizeof(RDesc));
    // native exchange: restores run at a synchronisation point (no import pending) through
    // parity 0's receive buffers
    const RDesc* rdesc = d_.recv_desc ? d_.recv_desc : (native_x_ ? par_[0].io.recv_desc : nullptr);
    const u8* rpay = d_.recv_pay ? d_.recv_pay : (native_x_ ? par_[0].io.recv_pay : nullptr);
    if (!rdesc || n > d_.import_max || pb > d_.xfer_bytes)
      throw std::runtime_error("restore batch exceeds the import buffers (restore_max / restore_bytes)");
    // import_one indexes q_owner with a routed record's tq and ch_pub_fail with a host
    // publish's channel slot, route_one the exchange tables with exch (below 0: no exchange),
    // and the payload is read at pay_off, all as given
    const RDesc* hd = (const RDesc*)di.ptr;
    for (u32 i = 0; i < n; ++i) {
      const RDesc& r = hd[i];
      if ((r.flags & (MF_RESTORE | MF_ONEQ)) && r.tq >= d_.q_max)
        throw std::runtime_error("restore: record " + std::to_string(i) + " names queue slot " + std::to_string(r.tq));
      if ((r.flags & MF_HOSTPUB) && (r.pad[0] >= d_.c_max * d_.chpc || r.pad[1] >= d_.c_max))
        throw std::runtime_error("restore: record " + std::to_string(i) + " names a channel out of range");
      if (r.exch >= (i32)d_.x_max)
        throw std::runtime_error("restore: record " + std::to_string(i) + " names exchange slot " + std::to_string(r.exch));
      if ((u64)r.pay_off + r.ex_len + r.rk_len + r.props_len + r.body_len > pb)
        throw std::runtime_error("restore: record " + std::to_string(i) + " ends past its payload");
    }
    between_steps("restore");
    drain_egress();
    if (db) HIPCHECK(hipMemcpy((void*)rdesc, di.ptr, db, hipMemcpyHostToDevice));
    if (pb) HIPCHECK(hipMemcpy((void*)rpay, pi.ptr, pb, hipMemcpyHostToDevice));
    DS& io = par_[0].io;
    StepIn& in = *par_[0].stage_in;   // (k_stage copies it to the device; no step in flight)
    in = StepIn{};
    in.ref_back = 0xffffffffu;   // (no dispatch: nothing rendered)
    in.nseg = 0;
    in.now_ms = now_ms;
    in.step = seq_;
    in.id_ms = now_ms;
    in.worker = 0;
    in.egress = (u64)eg_[0].dev;
    in.ingress = (u64)ing_[0].buf;
    u32* x = par_[0].io.xchg_h;
    for (u32 r = 0; r < 2 * WORLD_MAX; ++r) x[2 * WORLD_MAX + r] = x[XC_RECV_AN + r] = 0;
    for (u32 r = 0; r < WORLD_MAX; ++r) x[XC_RACK_N + r] = 0;
    x[2 * WORLD_MAX + d_.my_rank] = x[XC_RECV_AN + d_.my_rank] = n;
    x[3 * WORLD_MAX + d_.my_rank] = x[XC_RECV_AB + d_.my_rank] = (u32)pb;
    launch_ingest(s_comp_, io);
    launch_route(s_comp_, io, d_.pub_max);
    launch_phase_b(s_comp_, io, /*dispatch=*/false);
    HIPCHECK(hipStreamSynchronize(s_comp_));
    return par_[0].io.ctr_host_h->n_routed_msgs;
  }

  // Basic.Get between steps: (status, message_count, frames, tag, msg_id, qpos, persist,
  // expired [(msg_id, q, qpos)] of durable x persistent messages dropped by the TTL skip)
  py::tuple basic_get(u32 q, u32 chslot, u32 noack, i64 now_ms) {
    if (any_inflight()) throw std::runtime_error("basic_get() between steps only");
    if (q >= d_.q_max || chslot >= d_.c_max * d_.chpc) throw std::runtime_error("basic_get: bad queue / channel");
    Range rg("chanamq.basic_get");
    sync();
    const u32 last = (u32)(seq_ ? seq_ - 1 : 0);   // (the last step submitted; before the first: 0)
    with_flags([&](auto BL) {
      hipLaunchKernelGGL(k_basic_get<BL()>, dim3(1), dim3(64), 0, s_comp_, par_[0].io, q, chslot, noack, now_ms,
                         get_out_dev_, get_cap_, get_res_dev_, last);
    }, d_.blimits != 0);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s_comp_));
    const GetRes& r = *get_res_h_;
    py::list exp;
    for (u32 i = 0; i < r.n_exp && i < GET_EXP_MAX; ++i)
      exp.append(py::make_tuple(r.exp[i].msg_id, r.exp[i].q, r.exp[i].qpos));
    py::bytes frames(r.status == GET_OK ? (const char*)get_out_h_ : "", r.status == GET_OK ? r.out_len : 0);
    return py::make_tuple(r.status, r.msg_count, frames, r.tag, r.msg_id, r.qpos, r.persist, exp);
  }

  // ------------------------------------------------------------- native front end
  // C entry points (step_abi.h) for csrc/core/frontend.cpp: the front end's stepper
  // thread drives submit / wait_results / egress copies directly, without the GIL.  The
  // table lives as long as the Engine; the front end is stopped before the Engine dies.
  u64 c_api() {
    CmqEngineApi& a = api_;
    a.abi = CMQ_STEP_ABI;
    a.c_max = d_.c_max; a.seg_max = d_.seg_max; a.carry_cap = d_.carry_cap;
    a.persist = d_.persist; a.persist_max = d_.persist_max;
    a.ingress_cap = d_.ingress_cap; a.ctrl_cap = d_.ctrl_cap; a.carry_budget = carry_budget_;
    a.log_bytes = d_.log_bytes;
    a.eng = this;
    a.submit = [](void* e, const SegIn* sg, u32 n, const u8* pay, u64 len, i64 now, u32 worker) -> int {
      return ((Engine*)e)->guard([&] { return ((Engine*)e)->submit_raw(sg, n, (u64)pay, len, now, (u64)now, worker); });
    };
    a.prefetch = [](void* e, const u8* pay, u64 len) -> int {
      return ((Engine*)e)->guard([&] { return ((Engine*)e)->prefetch((u64)pay, len) ? 1 : 0; });
    };
    a.wait_results = [](void* e, int p) -> int {
      return ((Engine*)e)->guard([&] { ((Engine*)e)->wait_results(p); return 0; });
    };
    a.egress_slot = [](void* e, int p) -> int { return ((Engine*)e)->egress_slot(p); };
    a.egress_copy = [](void* e, int p) -> int {
      return ((Engine*)e)->guard([&] { ((Engine*)e)->egress_copy(p); return 0; });
    };
    a.egress_wait_slot = [](void* e, int slot) -> int {
      return ((Engine*)e)->guard([&] { ((Engine*)e)->egress_wait_slot(slot); return 0; });
    };
    a.error = [](void* e) -> const char* { return ((Engine*)e)->err_.c_str(); };
    a.counters = [](void* e, int p) -> const Counters* { return ((Engine*)e)->par_[p].io.ctr_host_h; };
    a.seg_out = [](void* e, int p) -> const SegOut* { return ((Engine*)e)->par_[p].io.seg_out_hh; };
    a.conn_out = [](void* e, int p) -> const ConnOut* { return ((Engine*)e)->par_[p].io.conn_out_hh; };
    a.ctrl_rec = [](void* e, int p) -> const CtrlRec* { return ((Engine*)e)->par_[p].io.ctrl_rec_hh; };
    a.ctrl = [](void* e, int p) -> const u8* { return ((Engine*)e)->par_[p].io.ctrl_hh; };
    a.egress_host = [](void* e, int slot) -> const u8* { return ((Engine*)e)->eg_[slot].host; };
    a.persist_host = [](void* e, int p) -> const u8* { return ((Engine*)e)->pslot_host(p); };
    a.consumed_host = [](void* e, int p) -> const ConsumedRec* { return ((Engine*)e)->cslot_host(p); };
    a.wblock = wblock_h_;
    a.grow_host = [](void* e, int p) -> const RingMove* { return ((Engine*)e)->par_[p].io.grow_hh; };
    a.conn_conf = [](void* e, int p) -> const u32* { return ((Engine*)e)->par_[p].io.conn_conf_hh; };
    a.world = d_.world;
    a.rank = d_.my_rank;
    a.native_xchg = native_x_ ? 1u : 0u;
    a.exchange = [](void* e, int q, u32 flags, u32* orf) -> int {   // (0 / -2; -1: threw)
      return ((Engine*)e)->guard([&] { return ((Engine*)e)->exchange(q, flags, orf); });
    };
    a.drop_exchange = [](void* e, int q) -> int {
      return ((Engine*)e)->guard([&] { return ((Engine*)e)->drop_exchange(q); });
    };
    a.launch_b = [](void* e, int p) -> int {
      return ((Engine*)e)->guard([&] { ((Engine*)e)->launch_b(p); return 0; });
    };
    a.links = links_ ? 1u : 0u;
    a.flush_submit = [](void* e, i64 now, u32 worker) -> int {
      return ((Engine*)e)->guard([&] {
        return ((Engine*)e)->submit_raw(nullptr, 0, 0, 0, now, (u64)now, worker, false, SF_NODISPATCH);
      });
    };
    a.host_register = [](void* e, void* ptr, u64 bytes) -> int {
      return ((Engine*)e)->guard([&] { HIPCHECK(hipHostRegister(ptr, bytes, hipHostRegisterDefault)); return 0; });
    };
    a.host_unregister = [](void* e, void* ptr) -> int {
      return ((Engine*)e)->guard([&] { HIPCHECK(hipHostUnregister(ptr)); return 0; });
    };
    a.egress_ready = [](void* e, int slot) -> int {
      return ((Engine*)e)->guard([&] { ((Engine*)e)->egress_ready(slot); return 0; });
    };
    a.stage_gets = [](void* e, const GetReq* r, u32 n) -> int {
      return ((Engine*)e)->guard([&] { ((Engine*)e)->stage_gets(r, n); return 0; });
    };
    a.get_out = [](void* e, int p) -> const GetOut* { return ((Engine*)e)->par_[p].io.get_out_hh; };
    a.host_work = [](void* e) -> int { return ((Engine*)e)->host_work() ? 1 : 0; };
    a.dl_state = [](void* e, int which) -> u64 { return ((Engine*)e)->dl_state(which); };
    a.unpaused = [](void* e, int p, const u32** out) -> u32 {
      Engine* en = (Engine*)e;
      if (p < 0 || p >= en->npar_) return 0;
      *out = en->par_[p].stage_unp;
      return en->par_[p].nunp;
    };
    a.set_egress_ref = [](void* e, int back, u32 min_bytes) -> int {
      return ((Engine*)e)->guard([&] { ((Engine*)e)->set_egress_ref(back, min_bytes); return 0; });
    };
    return (u64)&api_;
  }

  template <class F>
  int guard(F&& f) {
    try {
      HIPCHECK(hipSetDevice(device_));   // the caller may be any host thread
      return f();
    } catch (std::exception& ex) {
      err_ = ex.what();
      return -1;
    }
  }

 private:
  static ScanArgs scan_args(std::initializer_list<std::pair<const u32*, u32*>> arrs, const u32* n, u32 nmax,
                            u32 slot, const u32* lo) {
    if (arrs.size() > 4) throw std::runtime_error("launch_scan: at most 4 arrays");
    ScanArgs a{};
    a.lo = lo;
    u32 k = 0;
    for (auto& p : arrs) { a.in[k] = p.first; a.out[k] = p.second; ++k; }
    a.narr = k;
    a.n = n;
    a.nmax = nmax;
    a.tot_slot = slot;
    return a;
  }
  void launch_scan(hipStream_t s, const DS& d, std::initializer_list<std::pair<const u32*, u32*>> arrs, const u32* n,
                   u32 nmax, u32 slot, const u32* lo = nullptr, bool ingest = false) {
    const ScanArgs a = scan_args(arrs, n, nmax, slot, lo);
    u32 nb = ceil_div(nmax ? nmax : 1, SCAN_TILE);
    hipLaunchKernelGGL((k_scan<4, 4>), dim3(nb), dim3(1024), 0, s, a, d.tot, ingest ? scan_status_ing_ : scan_status_,
                       ingest ? scan_ctl_ing_ : scan_ctl_, scan_smax_);
  }
  // f(std::integral_constant<u32, B>{}) for the digit width B of a sort pass over `bits` key
  // bits: 8 (or fewer) .. 11, the widths the sort kernels are instantiated for
  template <class F>
  static void with_key_bits(u32 bits, F&& f) {
    if (bits <= 8) f(std::integral_constant<u32, 8>{});
    else if (bits == 9) f(std::integral_constant<u32, 9>{});
    else if (bits == 10) f(std::integral_constant<u32, 10>{});
    else f(std::integral_constant<u32, 11>{});
  }
  // f(std::bool_constant<B0>{}, std::bool_constant<B1>{}, ...) for the runtime booleans b0, b1, ...:
  // the launch of the kernel instantiation a combination of options selects, written once
  template <class F>
  static void with_flags(F&& f) { f(); }
  template <class F, class... B>
  static void with_flags(F&& f, bool b, B... rest) {
    if (b) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
  }
  // returns index (0/1) of the buffer holding the sorted output
  u32 radix_sort(hipStream_t s, const DS& d, u32** keys, u32** vals, const u32* n, u32 nmax, u32 bits) {
    const u32 ntiles = ceil_div(nmax, SORT_TILE);
    const u32 digit = bits > 8 && bits <= SORT_ONEPASS_BITS ? bits : 8;   // one 9..11-bit pass instead of two 8-bit ones
    u32 src = 0;
    for (u32 shift = 0; shift < bits; shift += digit) {
      with_key_bits(digit, [&](auto b) {
        constexpr u32 B = decltype(b)::value;
        hipLaunchKernelGGL(k_rs_hist<B>, capped(ntiles, 256), dim3(RsNt<B>::v), 0, s, keys[src], n, shift, d_.hist,
                           d_.hist_scan, &d.tot[TS_RS_TICKET], ntiles);
        hipLaunchKernelGGL(k_rs_scatter<B>, capped(ntiles, 256), dim3(256), 0, s, keys[src], vals[src], keys[src ^ 1],
                           vals[src ^ 1], n, shift, d_.hist_scan, ntiles);
      });
      src ^= 1;
    }
    return src;
  }

  static dim3 blocks(u64 n, u32 per) { return dim3(n ? ceil_div(n, per) : 1); }
  // wave-per-item grid-stride kernels: 4 waves per block, at most 8192 blocks.  Grids are
  // fixed at graph capture, sized for capacity; the cap keeps a step with a fraction of
  // the capacity from launching (and retiring) 100K+ idle waves, while still giving the
  // latency-bound per-item chains (route, store, render) one wave per item at the usual
  // step sizes (measured: a 2048-block cap made k_route / k_route_store / k_render slower)
  static dim3 wave_blocks(u64 n) { u64 b = n ? ceil_div(n, 4) : 1; return dim3(b > 8192 ? 8192 : (u32)b); }
  static dim3 capped(u64 b, u32 cap) { return dim3(b == 0 ? 1u : (b > cap ? cap : (u32)b)); }

  // frame scan, command assembly, decode (K1-K5)
  void launch_ingest(hipStream_t s, const DS& d) {
    Range rg("chanamq.K1-K4.ingest");
    hipLaunchKernelGGL(k_stage, dim3(1), dim3(1024), 0, s, d);
    // the wait for the payload copy rides the frame scan's own blocks (every block of the
    // grid waits and acquires, so every XCD a block lands on has dropped its stale lines of
    // the slot); a grid too small to reach every XCD gets the wait as 16 blocks of its own
    const dim3 fs_grid = capped(d.seg_max, n_cu_);
    const bool fold = h2d_hsa_ && fs_grid.x >= 16;
    if (h2d_hsa_ && !fold) hipLaunchKernelGGL(k_h2d_wait, dim3(16), dim3(64), 0, s, d);
    // one block per CU fits (154 KB of LDS): more blocks than CUs only queue behind the
    // busy ones, and blocks past the step's segments would still be dispatched one by one
    // after them (the grid is sized for capacity at capture)
    hipLaunchKernelGGL(k_frame_scan, fs_grid, dim3(FS_NT), 0, s, d, fold ? 1u : 0u);
    if (d.rank_scan)
      launch_scan(s, d, {{d.cmd_is_pub, d.cmd_pub_rank}, {d.cmd_is_ack, d.cmd_ack_rank}}, &d.ctr->n_cmds,
                  d.cmd_max, TS_CMD_PUBS, nullptr, /*ingest=*/true);
    hipLaunchKernelGGL(k_decode, blocks(d.cmd_max, 256), dim3(256), 0, s, d);
  }

  // route + store the publishes of the current phase range (K6); nmax = range capacity.
  // imports: phase B's import + routing pass 0 kernel (k_import_route) instead of k_route
  // ban: the dead view's routing with x-death on (the instantiations with route_emit's ban check)
  void launch_route(hipStream_t s, const DS& d, u32 nmax, bool imports = false, bool ban = false) {
    Range rg("chanamq.K6-K13.route_store");
    // 16 publishes per block, grid-stride; the grid is the blocks that can be resident
    // (k_route: 2 per CU at 64 VGPRs; k_import_route: 1), not the capacity's groups --
    // the idle blocks of a capacity-sized grid were still dispatched after the busy ones
    const u64 ngroups = ceil_div(nmax ? nmax : 1, 16);
    // (alt_: the instantiations with the alternate-exchange rule, launched only with the option on)
    with_flags([&](auto BAN, auto ALT) {
      if (imports) hipLaunchKernelGGL((k_import_route<BAN(), ALT()>), capped(ngroups, n_cu_), dim3(1024), 0, s, d);   // + prep, link acks
      else hipLaunchKernelGGL(k_route<ALT()>, capped(ngroups, 2 * n_cu_), dim3(1024), 0, s, d);
    }, ban, alt_);
    // scan of the routing counts + the phase's log reservation, then pairs + store
    const ScanArgs a = scan_args({{d.pub_nq, d.pub_pair_off}, {d.pub_slot, d.pub_slot_off},
                                  {d.pub_routed, d.pub_routed_rank}, {d.pub_ret_sz, d.pub_ret_off}},
                                 &d.tot[TS_RANGE_HI], d.pub_cap, TS_ROUTE, &d.tot[TS_RANGE_LO]);
    hipLaunchKernelGGL(k_scan_route, dim3(ceil_div(d.pub_cap ? d.pub_cap : 1, SCAN_TILE)), dim3(1024), 0, s, a, d.tot,
                       scan_status_, scan_ctl_, scan_smax_, d);
    // (the kernels that hold dead-letter code exist twice: with the flag off the step runs the
    // instantiation without any of it)
    if (ban) hipLaunchKernelGGL((k_route_store<true, true>), wave_blocks(nmax), dim3(256), 0, s, d, 0u);
    else if (d.dlx) hipLaunchKernelGGL(k_route_store<true>, wave_blocks(nmax), dim3(256), 0, s, d, imports ? 0u : 1u);
    else hipLaunchKernelGGL(k_route_store<false>, wave_blocks(nmax), dim3(256), 0, s, d, imports ? 0u : 1u);
  }

  // serialise publishes with remote owners into the per-destination send buffers
  void launch_pack(hipStream_t s, const DS& d) {
    Range rg("chanamq.X1.pack");
    // per destination rank: record and byte offsets of every publish (one pass, all
    // ranks); k_pack derives the destination bases itself and serialises
    hipLaunchKernelGGL(k_pack_scan, blocks(d.pub_max, PK_TILE), dim3(1024), 0, s, d, d.pk_agg, &d.tot[TS_PK_TICKET]);
    hipLaunchKernelGGL(k_pack, wave_blocks(d.pub_max), dim3(256), 0, s, d);
  }

  // enqueue, acks, dispatch, render (K7-K11)
  // dispatch = false (restore): enqueue only; nothing is delivered or rendered between
  // steps (the restored messages go out with the next step's dispatch)
  // imp: the payload the imported publishes of this launch were read from (DS.prio: k_prio_lane reads
  // their property bytes there; nullptr: DS.recv_pay)
  void launch_tail(hipStream_t s, const DS& d, bool dispatch = true, const u8* imp = nullptr) {
    Range rg("chanamq.K7-K11.tail");
    u32 nch = d.c_max * d.chpc;
    const u32 pbits = d.q_bits + d.rank_bits;
    // priority queues on (DS.prio): the pairs of priority queues move to their lanes ahead of the sort
    if (d.prio)
      hipLaunchKernelGGL(k_prio_lane, capped(ceil_div(d.pair_max, 256), 1024), dim3(256), 0, s, d, imp ? imp : d.recv_pay);
    if (pbits <= SORT_ONEPASS_BITS && !d.blimits) {
      // single-pass sort with the ring plan folded into the histogram's last block and the
      // enqueue into the scatter (k_rs_hist_plan / k_rs_scatter_enq): two launches
      const u32 nt = ceil_div(d.pair_max, SORT_TILE);
      const u32* n = &d.tot[TS_PAIR_N];
      u32* tk = &d.tot[TS_RS_TICKET];
      with_key_bits(pbits, [&](auto b) {
        constexpr u32 B = decltype(b)::value;
        hipLaunchKernelGGL(k_rs_hist_plan<B>, capped(nt, 256), dim3(RsNt<B>::v), 0, s, d, d.pair_k[0], n, d_.hist, d_.hist_scan, tk, nt);
        hipLaunchKernelGGL(k_rs_scatter_enq<B>, capped(nt, 256), dim3(256), 0, s, d, d.pair_k[0], d.pair_v[0], n, d_.hist_scan);
      });
    } else {
      u32* pk[2] = {d.pair_k[0], d.pair_k[1]};
      u32* pv[2] = {d.pair_v[0], d.pair_v[1]};
      const u32 psrc = radix_sort(s, d, pk, pv, &d.tot[TS_PAIR_N], d.pair_max, pbits);
      hipLaunchKernelGGL(k_qfirst, blocks(d.pair_max, 256), dim3(256), 0, s, d, psrc);
      // byte limits on (DS.blimits): this path at every key width -- k_byte_room needs the sorted pair
      // arrays, which the fused path never materialises -- with K_q computed ahead of the ring plan
      // and the BL instantiations of the plan and the enqueue
      const dim3 pg = capped(ceil_div(d.pair_max, 256), 1024);
      if (d.blimits) hipLaunchKernelGGL(k_byte_room, pg, dim3(256), 0, s, d, psrc);
      with_flags([&](auto BL) {
        hipLaunchKernelGGL(k_ring_plan<BL()>, pg, dim3(256), 0, s, d, psrc);
        hipLaunchKernelGGL(k_enqueue<BL()>, pg, dim3(256), 0, s, d, psrc);
      }, d.blimits != 0);
    }
    // without persistence nothing runs after k_post: it also writes the host-visible
    // outputs and its last block the counters (fused k_host_out)
    const u32 fin = d.persist ? 0u : 1u;
    if (!dispatch) {
      const u64 pn = d.deliv_max > d.c_max ? d.deliv_max : d.c_max;
      hipLaunchKernelGGL(k_post, blocks(pn, 256), dim3(256), 0, s, d, fin);   // n_deliv = 0: frees only
      if (!fin) hipLaunchKernelGGL(k_host_out, dim3(64), dim3(256), 0, s, d);
      return;
    }
    // k_dequeue first puts requeued deliveries back in front of their queues' heads, in
    // queue-offset order (QueueEntity.scala:415-446), then dispatches; its last block lays out the runs
    // (DS.prio: the PRIO instantiations leave the base slots of priority queues and the step's run
    // layout to k_prio_dispatch, launched behind them)
    with_flags([&](auto DLX, auto BL, auto PRIO) {
      hipLaunchKernelGGL(k_chan_advance<DLX()>, capped(nch, 1024), dim3(256), 0, s, d);
      hipLaunchKernelGGL((k_dequeue<DLX(), BL(), PRIO()>), dim3(d.q_max), dim3(256), 0, s, d);
    }, d.dlx != 0, d.blimits != 0, d.prio != 0);
    if (d.prio) hipLaunchKernelGGL(k_prio_dispatch, dim3(d.q_max), dim3(256), 0, s, d);
    hipLaunchKernelGGL(k_dv_write, blocks(d.deliv_max, 256), dim3(256), 0, s, d);
    if (d.c_max <= CONN_LAYOUT_MAX) {
      hipLaunchKernelGGL(k_conn_layout, dim3(1), dim3(1024), 0, s, d);   // + the delivery-size scan
    } else {
      launch_scan(s, d, {{d.dv_size, d.dv_off}}, &d.ctr->n_deliv, d.deliv_max, TS_DELIV_BYTES);
      hipLaunchKernelGGL(k_conn_sizes, blocks(d.c_max, 256), dim3(256), 0, s, d);
      launch_scan(s, d, {{d.conn_total, d.conn_base}}, nullptr, d.c_max, TS_CONN_BYTES);
      hipLaunchKernelGGL(k_conn_out, blocks(d.c_max, 256), dim3(256), 0, s, d);
    }
    if (d.links) hipLaunchKernelGGL(k_link_bases, dim3(1), dim3(64), 0, s, d);
    {
      const u32 n_rc = RC_RET_BLOCKS + ceil_div(d.c_max, 256);
      hipLaunchKernelGGL(k_render, dim3(n_rc + wave_blocks(d.deliv_max).x), dim3(256), 0, s, d, n_rc);
    }
    u64 pn = d.deliv_max > d.c_max ? d.deliv_max : d.c_max;
    hipLaunchKernelGGL(k_post, blocks(pn, 256), dim3(256), 0, s, d, fin);
    if (d.persist) {
      hipLaunchKernelGGL(k_persist_size, blocks(d.persist_max, 256), dim3(256), 0, s, d);
      launch_scan(s, d, {{d.ps_size, d.ps_off}}, &d.ctr->n_persist, d.persist_max, TS_PERSIST);
      hipLaunchKernelGGL(k_persist_pack, wave_blocks(d.persist_max), dim3(256), 0, s, d);
      hipLaunchKernelGGL(k_host_out, dim3(64), dim3(256), 0, s, d);
    }
  }

  // dead-lettering (DS.dlx, world 1): the entries that died in earlier steps, rendered as
  // import records by k_dead_pack, routed and stored behind the step's own publishes -- the
  // import range behind the local range, its pairs appended at TS_PAIR_BASE, one sort and
  // enqueue for both, as phase B of a sharded step.  The pass sees `d` with its receive side
  // pointing at the dead-letter buffers (restore() and publish_host keep theirs); the counts
  // are k_dead_pack's.  One list and one pair of buffers serve the steps in flight: the
  // routing halves of consecutive steps are ordered on one stream, and the ingest half
  // touches none of it
  void launch_dead(hipStream_t s, const DS& d) {
    Range rg("chanamq.DL.dead_pass");
    // x-death: one launch more, the pending items' new property lengths, before phase 0 takes its
    // prefix by them; phase 1 then rewrites the bytes and fills the ban rows the routing reads
    const bool xd = dl_h_.xdeath != 0;
    if (xd) hipLaunchKernelGGL(k_dead_size, wave_blocks(dl_h_.dead_max), dim3(256), 0, s, d);
    with_flags([&](auto XD, auto PRIO) {
      hipLaunchKernelGGL(k_dead_pack<XD()>, dim3(1), dim3(1024), 0, s, d, 0u, dead_room_);
      // (x-death with DS.prio: the instantiation whose ban rows name a lane's base slot)
      hipLaunchKernelGGL((k_dead_pack<XD(), XD() && PRIO()>), wave_blocks(dead_room_), dim3(256), 0, s, d, 1u, dead_room_);
    }, xd, d.prio != 0);
    DS v = d;
    v.dlx = 2;
    v.recv_desc = dl_h_.dead_desc;
    v.recv_pay = dl_h_.dead_pay;
    v.xchg = dl_h_.dead_xchg;
    v.import_max = dead_room_;
    v.import_bytes = dl_h_.dead_bytes;
    launch_route(s, v, dead_room_, /*imports=*/true, /*ban=*/xd);
    hipLaunchKernelGGL(k_dead_pack<false>, capped(ceil_div(dead_room_, 256), 64), dim3(256), 0, s, d, 2u, dead_room_);
  }

  // world == 1: the whole step; world > 1: phase A (ingest, local route, pack)
  void launch_main(hipStream_t s, const DS& d) {
    launch_ingest(s, d);
    launch_route(s, d, d.pub_max);   // (+ the K9 marks / K10 confirm counts: k_route_store)
    if (d.world > 1) {
      launch_pack(s, d);
    } else {
      if (d.dlx) launch_dead(s, d);
      launch_tail(s, d, true, d.dlx ? dl_h_.dead_pay : nullptr);
    }
  }

  // world == 1 with overlap: the routing / delivery half of the step (the step's acks /
  // nacks / rejects are marked and its confirms counted in it -- k_route_store, phase 0 --
  // never in the ingest half, so an overlapped ingest never touches delivery-side state)
  void launch_rest(hipStream_t s, const DS& d) {
    launch_route(s, d, d.pub_max);
    if (d.dlx) launch_dead(s, d);
    launch_tail(s, d, true, d.dlx ? dl_h_.dead_pay : nullptr);
  }
  // the launches f makes on stream st, captured once into *ge
  void capture(hipStream_t st, hipGraphExec_t* ge, const std::function<void()>& f) {
    hipGraph_t g;
    std::lock_guard<std::mutex> cg(cap_mu_);   // (no exchange-thread HIP call inside a capture)
    HIPCHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    f();
    HIPCHECK(hipStreamEndCapture(st, &g));
    HIPCHECK(hipGraphInstantiate(ge, g, nullptr, nullptr, 0));
    HIPCHECK(hipGraphDestroy(g));
  }

  // world > 1, after the all-to-all: import, route against local queues, rest of the step
  void launch_phase_b(hipStream_t s, const DS& d, bool dispatch = true) {
    Range rg("chanamq.X1.import");
    launch_route(s, d, d.import_max, /*imports=*/true);
    launch_tail(s, d, dispatch);
  }
};

static py::array alloc_pinned(size_t bytes) {
  void* p = nullptr;
  HIPCHECK(hipHostMalloc(&p, bytes, hipHostMallocPortable));
  return py::array(py::dtype("uint8"), {(py::ssize_t)bytes}, {(py::ssize_t)1}, p,
                   py::capsule(p, [](void* q) { (void)hipHostFree(q); }));
}

static u64 create_stream(int device) {
  HIPCHECK(hipSetDevice(device));
  hipStream_t st;
  HIPCHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  return (u64)st;
}

static int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

PYBIND11_MODULE(_dataplane, m) {
  m.doc() = "MI355X (gfx950) AMQP data-plane kernels + native step runtime";
  m.def("alloc_pinned", &alloc_pinned, "page-locked host buffer (numpy uint8)");
  m.def("roctx_push", [](const std::string& n) { roctxRangePushA(n.c_str()); });
  m.def("roctx_pop", []() { roctxRangePop(); });
  m.def("roctx_mark", [](const std::string& n) { roctxMarkA(n.c_str()); });
  m.def("device_count", &device_count);
  m.def("create_stream", &create_stream, py::arg("device") = 0);
  m.attr("CAND_MAX") = CAND_MAX;
  m.attr("FS_CAND_STAGED") = FS_CAND_STAGED;   // the frame scan's limits (dp_frame_scan.h)
  m.attr("FS_STAGE") = FS_STAGE;
  m.attr("FS_AM_MAX") = FS_AM_MAX;
  m.attr("FS_RUNS") = FS_RUNS;
  m.attr("TOPIC_K") = TOPIC_K;
  m.attr("TOPIC_WORDS") = TOPIC_WORDS;
  m.attr("SORT_TILE") = SORT_TILE;   // the sort / enqueue limits (dataplane.hip)
  m.attr("RS_RT") = RS_RT;
  m.attr("RS_RB") = RS_RB;
  m.attr("PUB_QC") = PUB_QC;
  m.attr("HB_PAIRS") = (u32)HB_PAIRS;   // pairs of one headers binding (dp_headers.h)
  m.attr("SORT_ONEPASS_BITS") = SORT_ONEPASS_BITS;
  m.attr("LAT_BINS") = LAT_BINS;
  m.attr("DVW_LDS") = DVW_LDS;   // the delivery layout / render limits (dataplane.hip)
  m.attr("CONN_LAYOUT_MAX") = CONN_LAYOUT_MAX;
  m.attr("RC_RET_BLOCKS") = RC_RET_BLOCKS;
  m.attr("RD_G") = RD_G;
  m.attr("PK_TILE") = PK_TILE;   // the cross-rank pack's limits (info() has them too)
  m.attr("WORLD_MAX") = (u32)WORLD_MAX;
  py::class_<Engine>(m, "Engine")
      .def(py::init<py::dict>())
      .def("info", &Engine::info)
      .def("fill", &Engine::fill)
      .def("upload", &Engine::upload, py::arg("name"), py::arg("data"), py::arg("offset") = 0)
      .def("download", &Engine::download, py::arg("name"), py::arg("offset") = 0, py::arg("n") = 0)
      .def("host_view", &Engine::host_view)
      .def("submit", &Engine::submit, py::arg("segs"), py::arg("payload_ptr"), py::arg("payload_len"),
           py::arg("now_ms"), py::arg("step"), py::arg("id_ms"), py::arg("worker"), py::arg("defer") = false,
           py::arg("flags") = 0)
      .def("launch", &Engine::launch)
      .def("prefetch", &Engine::prefetch, py::arg("payload_ptr"), py::arg("payload_len"))
      .def("persist_slot", &Engine::persist_slot)
      .def("step_runs", &Engine::step_runs)
      .def("stage_unpause", &Engine::stage_unpause)
      .def("stage_gets", [](Engine& e, py::buffer b) {
             py::buffer_info bi = b.request();
             const size_t nb = (size_t)bi.size * bi.itemsize;
             if (nb % sizeof(GetReq)) throw std::runtime_error("stage_gets: GetReq[] (u32 conn, chslot, q, noack)");
             e.stage_gets((const GetReq*)bi.ptr, (u32)(nb / sizeof(GetReq)));
           })
      .def("get_out", &Engine::get_out_py)
      .def("send_counts", &Engine::send_counts)
      .def("submit_b", &Engine::submit_b, py::arg("parity"), py::arg("recv"), py::arg("stream") = 0)
      .def("set_xfer_buffers", &Engine::set_xfer_buffers)
      .def("set_xfer_parity", &Engine::set_xfer_parity)
      .def("set_import", &Engine::set_import, py::arg("recv"), py::arg("stream") = 0)
      .def("restore", &Engine::restore, py::arg("desc"), py::arg("payload"), py::arg("now_ms"))
      .def("spill", &Engine::spill, py::arg("lim"), py::arg("hot"), py::call_guard<py::gil_scoped_release>())
      .def("cold_pick", &Engine::cold_pick, py::arg("hot"), py::arg("lim"), py::arg("max_n"), py::arg("max_bytes"))
      .def("cold_commit", &Engine::cold_commit)
      .def("cold_scan", &Engine::cold_scan, py::arg("window"), py::arg("max_n"))
      .def("cold_in", &Engine::cold_in)
      .def("side_cold_pick", &Engine::side_cold_pick, py::arg("hot"), py::arg("lim"), py::arg("min_used"),
           py::arg("max_n"), py::arg("max_bytes"))
      .def("side_cold_commit", &Engine::side_cold_commit)
      .def("side_cold_scan", &Engine::side_cold_scan, py::arg("window"), py::arg("max_n"))
      .def("side_cold_in", &Engine::side_cold_in)
      .def("side_cold_live", &Engine::side_cold_live)
      .def("side_wait", &Engine::side_wait, py::arg("timeout_s"))
      .def("side_pending", &Engine::side_pending)
      .def("basic_get", &Engine::basic_get, py::arg("q"), py::arg("chslot"), py::arg("noack"), py::arg("now_ms"))
      .def("wait_results", &Engine::wait_results)
      .def("h2d_stats", &Engine::h2d_stats)
      .def("egress_copy", &Engine::egress_copy)
      .def("egress_wait", &Engine::egress_wait)
      .def("egress_slot", &Engine::egress_slot)
      .def("set_egress_ref", &Engine::set_egress_ref)
      .def("set_deliver_cap_bytes", [](Engine& e, u32 n) { e.dcap_bytes_ = n; })
      .def("egress_wait_slot", &Engine::egress_wait_slot)
      .def("egress_done_slot", &Engine::egress_done_slot)
      .def("step_done", &Engine::step_done)
      .def("sync", &Engine::sync)
      .def("c_api", &Engine::c_api)
      .def("xchg_setup", &Engine::xchg_setup, py::arg("kind"), py::arg("arg"), py::arg("members"),
           py::arg("timeout_ms") = 10000, py::arg("failover") = false, py::arg("counts_shm") = "",
           py::arg("async_x") = false,
           py::call_guard<py::gil_scoped_release>())
      .def_static("xchg_unique_id", &Engine::xchg_unique_id)
      .def("exchange", [](Engine& e, int q, u32 flags) {
             u32 orf = 0;
             int rc;
             {
               py::gil_scoped_release nogil;
               rc = e.exchange(q, flags, &orf);
             }
             return py::make_tuple(rc, orf);
           }, py::arg("parity"), py::arg("flags") = 0)
      .def("drop_exchange", &Engine::drop_exchange, py::arg("q"), py::arg("collect") = false)
      .def("launch_b", &Engine::launch_b)
      .def("counters", &Engine::counters)
      .def("host_times", &Engine::host_times, py::arg("reset") = false)
      .def("egress_stats", &Engine::egress_stats)
      .def("inject_gate_fault", &Engine::inject_gate_fault)
      .def("inject_h2d_fault", &Engine::inject_h2d_fault)
      .def("wait_failed", &Engine::wait_failed)
      .def("stage_write", &Engine::stage_write_buf, py::arg("name"), py::arg("data"), py::arg("offset") = 0)
      .def("stage_mark_dirty", &Engine::stage_mark_dirty)
      .def("stage_begin", &Engine::stage_begin)
      .def("dl_state", &Engine::dl_state)
      .def("stage_end", &Engine::stage_end)
      .def("stage_spill", &Engine::stage_spill)
      .def("deltas_pending", &Engine::deltas_pending)
      .def("flush_deltas", &Engine::flush_deltas, py::call_guard<py::gil_scoped_release>());
}
