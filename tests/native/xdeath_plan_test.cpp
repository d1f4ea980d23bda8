// Stand-alone driver of csrc/kernels/xdeath_plan.h (no GPU, no Python extension), built with
// -fsanitize=address,undefined by tests/test_xdeath_plan.py.
//
//   no arguments   hand-made property lists and a few thousand mutated ones from a fixed seed:
//                  every plan stays inside its input (each input lives in a heap block of exactly
//                  its size, so a read past it is an ASan report), its new length equals the bytes
//                  the scalar writer produces from the same plan, and its output parses again
//                  with the merged array's element count.  Prints "ok".
//   "pipe"         lines "reason qname ex rk time props" (hex; "-" for empty) on stdin; for each
//                  "status out ban,ban,.." on stdout -- the Python test compares them with the
//                  golden model's rewrite.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "xdeath_plan.h"

typedef std::vector<u8> Bytes;

struct BanList {
  std::vector<std::pair<u32, u32>> v;
  void add(u32 off, u32 len) { v.push_back({off, len}); }
  void reset() { v.clear(); }
};

struct Emit {
  Bytes out;
  size_t cap;
  bool over = false;
  void raw(const u8* s, u32 n) {
    if (out.size() + n > cap) { over = true; return; }
    out.insert(out.end(), s, s + n);
  }
  void byte(u32 v) { const u8 b = (u8)v; raw(&b, 1); }
  void be32(u32 v) { const u8 b[4] = {(u8)(v >> 24), (u8)(v >> 16), (u8)(v >> 8), (u8)v}; raw(b, 4); }
  void be64(u64 v) { be32((u32)(v >> 32)); be32((u32)v); }
};

static void fail(const char* what, const Bytes& in) {
  std::fprintf(stderr, "FAIL %s: input", what);
  for (u8 b : in) std::fprintf(stderr, " %02x", b);
  std::fprintf(stderr, "\n");
  std::exit(1);
}

struct Death { Bytes qn, ex, rk; u32 reason; u64 t; };

// plan + write over an exact-size heap copy of `in`; returns the status
static u32 run(const Bytes& in, const Death& d, Bytes* out, BanList* bans, XdPlan* plan) {
  std::unique_ptr<u8[]> p(new u8[in.size() ? in.size() : 1]);
  if (!in.empty()) std::memcpy(p.get(), in.data(), in.size());
  XdCtx c{d.qn.data(), (u32)d.qn.size(), d.reason, d.ex.data(), (u32)d.ex.size(), d.rk.data(), (u32)d.rk.size(), d.t};
  XdPlan pl;
  BanList bl;
  xd_plan<XdScalarId>(p.get(), (u32)in.size(), c, pl, bl);
  if (plan) *plan = pl;
  if (bans) *bans = bl;
  if (pl.status == XD_REWRITE) {
    Emit em;
    em.cap = pl.new_len;
    xd_emit<XdScalarId>(em, p.get(), (u32)in.size(), c, pl);
    if (em.over || em.out.size() != pl.new_len) fail("the writer's bytes differ from the plan's length", in);
    if (out) *out = em.out;
  } else {
    if (pl.status == XD_VERBATIM && pl.new_len != in.size()) fail("verbatim length", in);
    if (out) *out = in;
  }
  for (auto& b : bl.v)
    if ((u64)b.first + b.second > in.size()) fail("a banned name outside the input", in);
  return pl.status;
}

// ---- building property lists
static void put32(Bytes& b, u32 v) { for (int s = 24; s >= 0; s -= 8) b.push_back((u8)(v >> s)); }
static void put_name(Bytes& b, const std::string& n) { b.push_back((u8)n.size()); b.insert(b.end(), n.begin(), n.end()); }
static void put_S(Bytes& b, const std::string& n, const std::string& v) {
  put_name(b, n); b.push_back('S'); put32(b, (u32)v.size()); b.insert(b.end(), v.begin(), v.end());
}
static void put_l(Bytes& b, const std::string& n, u64 v) { put_name(b, n); b.push_back('l'); put32(b, (u32)(v >> 32)); put32(b, (u32)v); }
static Bytes elem(const std::string& q, const std::string& r, int count_tag) {
  Bytes body;
  if (count_tag == 'l') put_l(body, "count", 3);
  if (count_tag == 'I') { put_name(body, "count"); body.push_back('I'); put32(body, 7); }
  if (count_tag == 'S') put_S(body, "count", "many");
  if (!r.empty()) put_S(body, "reason", r);
  if (!q.empty()) put_S(body, "queue", q);
  Bytes e{'F'};
  put32(e, (u32)body.size());
  e.insert(e.end(), body.begin(), body.end());
  return e;
}
static Bytes props(u32 flags, const Bytes& table, bool has_table, const std::string& exp) {
  Bytes p{(u8)(flags >> 8), (u8)flags};
  if (flags & (1u << 15)) put_name(p, "text/plain");
  if (flags & (1u << 14)) put_name(p, "gzip");
  if (has_table) { put32(p, (u32)table.size()); p.insert(p.end(), table.begin(), table.end()); }
  if (flags & (1u << 12)) p.push_back(2);
  if (flags & (1u << 10)) put_name(p, "corr");
  if (flags & (1u << 8)) put_name(p, exp);
  if (flags & (1u << 6)) for (int i = 0; i < 8; ++i) p.push_back((u8)i);
  if (flags & (1u << 3)) put_name(p, "app");
  return p;
}
static Bytes xdeath_entry(const std::vector<Bytes>& els) {
  Bytes arr;
  for (auto& e : els) arr.insert(arr.end(), e.begin(), e.end());
  Bytes t;
  put_name(t, "x-death");
  t.push_back('A');
  put32(t, (u32)arr.size());
  t.insert(t.end(), arr.begin(), arr.end());
  return t;
}

static const Death DEATH{{'w', 'o', 'r', 'k'}, {'i', 'n'}, {'k', '.', '1'}, XD_EXPIRED, 1700000000ull};

// the output parses again: a rewrite of it for the same death matches the front element
static void reparse(const Bytes& in, const Bytes& out, const XdPlan& pl) {
  XdPlan p2;
  Bytes o2;
  const u32 st = run(out, DEATH, &o2, nullptr, &p2);
  const u32 merged = pl.nel + (pl.m_off == XD_NONE ? 1u : 0u);
  if (st == XD_VERBATIM) fail("the output does not parse", in);
  if (p2.nel != merged) fail("the output's array has another element count", in);
  if (p2.m_off == XD_NONE) fail("the output's front element does not match its own death", in);
  if (p2.first) fail("the output lost x-first-death-queue", in);
  if (p2.exp_off) fail("the output still has an expiration", in);
}

static u32 checked(const Bytes& in, const Death& d = DEATH) {
  Bytes out;
  XdPlan pl;
  const u32 st = run(in, d, &out, nullptr, &pl);
  if (st == XD_REWRITE && d.reason == DEATH.reason && d.qn == DEATH.qn) reparse(in, out, pl);
  return st;
}

static int self_test() {
  // hand-made: no properties, no table, a table, properties on both sides, continuation flags
  Bytes t1;
  put_S(t1, "kind", "late");
  const u32 BOTH = (1u << 15) | (1u << 14) | (1u << 12) | (1u << 10) | (1u << 8) | (1u << 6) | (1u << 3);
  std::vector<Bytes> hand = {
      props(0, {}, false, ""), props(1u << 8, {}, false, "1000"), props(1u << 13, t1, true, ""),
      props(BOTH, {}, false, "60000"), props(BOTH | (1u << 13), t1, true, "5"), props(1u << 13, {}, true, "")};
  for (auto& h : hand)
    if (checked(h) != XD_REWRITE) fail("a well-formed list is not rewritten", h);
  {  // cut short: verbatim
    Bytes c = props(BOTH | (1u << 13), t1, true, "5");
    for (size_t n = 0; n < c.size(); ++n) {
      Bytes cut(c.begin(), c.begin() + n);
      if (checked(cut) != XD_VERBATIM) fail("a list cut short is rewritten", cut);
    }
    Bytes one{0x00};
    if (checked(one) != XD_VERBATIM || checked(Bytes{}) != XD_VERBATIM) fail("empty", one);
  }
  // arrays: match with each count form, no match, lookalike names, duplicates, malformed
  for (int tag : {(int)'l', (int)'I', (int)'S', 0}) {
    Bytes t = t1;
    Bytes x = xdeath_entry({elem("other", "expired", 'l'), elem("work", "expired", tag), elem("work", "rejected", 'l')});
    t.insert(t.end(), x.begin(), x.end());
    put_S(t, "x-deat", "1");
    put_S(t, "x-death2", "2");
    put_S(t, "X-Death", "3");
    Bytes x2 = xdeath_entry({elem("dup", "expired", 'l')});
    t.insert(t.end(), x2.begin(), x2.end());
    const Bytes p = props(BOTH | (1u << 13), t, true, "77");
    Bytes out;
    XdPlan pl;
    BanList bl;
    if (run(p, DEATH, &out, &bl, &pl) != XD_REWRITE || pl.m_off == XD_NONE || pl.nel != 3) fail("match", p);
    const u64 want = tag == 'l' ? 4 : (tag == 'I' ? 8 : 1);
    if (pl.count != want) fail("count", p);
    if (bl.v.size() != 1) fail("bans: `other`, then the reject ends them", p);
    reparse(p, out, pl);
  }
  {  // 63 + 1 fit, 64 + 1 are over, 64 with a match stay
    for (int n : {62, 63, 64}) {
      std::vector<Bytes> els;
      for (int i = 0; i < n; ++i) els.push_back(elem("old" + std::to_string(i), "expired", 'l'));
      const Bytes p = props(1u << 13, xdeath_entry(els), true, "");
      if (checked(p) != (n == 64 ? XD_OVER : XD_REWRITE)) fail("element limit", p);
      els.back() = elem("work", "expired", 'l');
      if (checked(props(1u << 13, xdeath_entry(els), true, "")) != XD_REWRITE) fail("element limit with a match", p);
    }
    // malformed values are replaced
    Bytes t;
    put_S(t, "x-death", "once");
    if (checked(props(1u << 13, t, true, "")) != XD_REWRITE) fail("string x-death", t);
    Bytes bad = xdeath_entry({elem("a", "expired", 'l')});
    bad.push_back('I');   // (outside the array: the table is malformed -> verbatim)
    if (checked(props(1u << 13, bad, true, "")) != XD_VERBATIM) fail("garbage behind the array", bad);
    Bytes arr = elem("a", "expired", 'l');
    arr.push_back('t'); arr.push_back(1);
    Bytes t2;
    put_name(t2, "x-death"); t2.push_back('A'); put32(t2, (u32)arr.size()); t2.insert(t2.end(), arr.begin(), arr.end());
    XdPlan pl;
    const Bytes p2 = props(1u << 13, t2, true, "");
    if (run(p2, DEATH, nullptr, nullptr, &pl) != XD_REWRITE || pl.nel != 0 || pl.arr_e != 0) fail("array with a boolean", p2);
  }
  {  // the byte limit: exactly XD_PROPS_MAX fits, one more is over
    for (u32 extra : {0u, 1u}) {
      Bytes probe;
      put_S(probe, "pad", "");
      XdPlan pl;
      run(props(1u << 13, probe, true, ""), DEATH, nullptr, nullptr, &pl);
      Bytes t;
      put_S(t, "pad", std::string(XD_PROPS_MAX - pl.new_len + extra, 'p'));
      const Bytes p = props(1u << 13, t, true, "");
      if (checked(p) != (extra ? XD_OVER : XD_REWRITE)) fail("byte limit", p);
    }
  }
  // mutated lists from a fixed seed: bytes flipped, lengths bent, lists cut
  std::vector<Bytes> seeds = hand;
  {
    Bytes t = t1;
    Bytes x = xdeath_entry({elem("other", "expired", 'l'), elem("work", "expired", 'I'), elem("", "rejected", 'l'),
                            elem("work", "", 0)});
    t.insert(t.end(), x.begin(), x.end());
    put_S(t, "x-first-death-queue", "first");
    seeds.push_back(props(BOTH | (1u << 13), t, true, "1000"));
    seeds.push_back(props((1u << 13) | 1u, t, true, ""));   // (a continuation flag word is missing: cut short)
  }
  u64 rng = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
  u32 n_rw = 0, n_vb = 0, n_ov = 0;
  for (int it = 0; it < 6000; ++it) {
    Bytes m = seeds[next() % seeds.size()];
    const int nmut = 1 + (int)(next() % 3);
    for (int k = 0; k < nmut && !m.empty(); ++k) {
      const size_t at = next() % m.size();
      switch (next() % 4) {
        case 0: m[at] = (u8)next(); break;
        case 1: m[at] ^= (u8)(1u << (next() % 8)); break;
        case 2: m.resize(at); break;
        default: m.insert(m.begin() + at, (u8)next()); break;
      }
    }
    Death d = DEATH;
    d.reason = (u32)(next() % 3);
    const u32 st = checked(m, d);
    (st == XD_REWRITE ? n_rw : (st == XD_VERBATIM ? n_vb : n_ov))++;
  }
  if (n_rw < 500 || n_vb < 500) { std::fprintf(stderr, "FAIL mutation mix %u %u %u\n", n_rw, n_vb, n_ov); return 1; }
  std::printf("ok\n");
  return 0;
}

static Bytes unhex(const std::string& s) {
  Bytes b;
  if (s == "-") return b;
  for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((u8)std::stoul(s.substr(i, 2), nullptr, 16));
  return b;
}
static std::string hex(const u8* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) { s.push_back(d[p[i] >> 4]); s.push_back(d[p[i] & 15]); }
  return s.empty() ? "-" : s;
}

int main(int argc, char** argv) {
  if (argc < 2) return self_test();
  std::string reason, qn, ex, rk, t, pr;
  while (std::cin >> reason >> qn >> ex >> rk >> t >> pr) {
    const Death d{unhex(qn), unhex(ex), unhex(rk), (u32)std::stoul(reason), std::stoull(t)};
    const Bytes in = unhex(pr);
    Bytes out;
    BanList bl;
    const u32 st = run(in, d, &out, &bl, nullptr);
    std::string bans;
    if (st == XD_REWRITE)
      for (auto& b : bl.v) bans += (bans.empty() ? "" : ",") + hex(in.data() + b.first, b.second);
    std::printf("%u %s %s\n", st, st == XD_REWRITE ? hex(out.data(), out.size()).c_str() : "-", bans.empty() ? "-" : bans.c_str());
  }
  return 0;
}
