// csrc/kernels/prio_plan.h on the CPU, under the address and undefined-behaviour sanitizers.
//   no argument: the split of a piece of V against a brute-force one, prio_locate and prio_lane
//                over every small case; the property walk on lists held in exact-size heap blocks,
//                so a read past the end is an error here
//   "pipe":      one property list per line (hex, "-" for the empty list); prints its priority
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "prio_plan.h"

static int fails = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
  } while (0)

static u32 walk_exact(const std::vector<u8>& v) {
  u8* p = (u8*)std::malloc(v.size() ? v.size() : 1);   // exact size: the sanitizer sees any overread
  if (!v.empty()) std::memcpy(p, v.data(), v.size());
  const u32 r = prio_of_props(p, (u32)v.size());
  std::free(p);
  return r;
}

static void test_split() {
  // every lane filling of up to 4 lanes with 0..3 entries, every piece
  for (u32 lanes = 1; lanes <= 4; ++lanes) {
    u32 combos = 1;
    for (u32 l = 0; l < lanes; ++l) combos *= 4;
    for (u32 c = 0; c < combos; ++c) {
      u64 n[PRIO_LANES] = {};
      u32 x = c;
      u64 total = 0;
      std::vector<std::pair<u32, u64>> v;   // V, entry by entry: (lane, position)
      for (u32 l = 0; l < lanes; ++l) {
        n[l] = x % 4;
        x /= 4;
        for (u64 k = 0; k < n[l]; ++k) v.push_back({l, k});
        total += n[l];
      }
      for (u64 off = 0; off <= total; ++off) {
        u32 ln = 99;
        u64 pos = 99;
        const bool in = prio_locate(n, lanes, off, &ln, &pos);
        CHECK(in == (off < total));
        if (in) CHECK(ln == v[off].first && pos == v[off].second);
        for (u32 cnt = 0; off + cnt <= total; ++cnt) {
          PrioPart out[PRIO_LANES];
          const u32 k = prio_split(n, lanes, off, cnt, out);
          std::vector<std::pair<u32, u64>> got;
          for (u32 i = 0; i < k; ++i) {
            CHECK(out[i].cnt > 0);
            if (i) CHECK(out[i].lane > out[i - 1].lane);
            for (u32 e = 0; e < out[i].cnt; ++e) got.push_back({out[i].lane, out[i].pos + e});
          }
          CHECK(got.size() == cnt);
          for (u32 e = 0; e < cnt && e < got.size(); ++e) CHECK(got[e] == v[off + e]);
        }
        // a piece that runs past the end of V is cut at it
        PrioPart out[PRIO_LANES];
        u64 sum = 0;
        const u32 k = prio_split(n, lanes, off, 1000, out);
        for (u32 i = 0; i < k; ++i) sum += out[i].cnt;
        CHECK(sum == total - off);
      }
    }
  }
  // 16 lanes of large counts: no 32-bit wrap in the offsets
  u64 big[PRIO_LANES];
  for (u32 l = 0; l < PRIO_LANES; ++l) big[l] = (1ull << 33) + l;
  PrioPart out[PRIO_LANES];
  const u64 off = 3 * (1ull << 33) + 3 - 2;   // two entries before the end of lane 2
  const u32 k = prio_split(big, PRIO_LANES, off, 5, out);
  CHECK(k == 2 && out[0].lane == 2 && out[0].cnt == 2 && out[0].pos == big[2] - 2);
  CHECK(out[1].lane == 3 && out[1].pos == 0 && out[1].cnt == 3);
}

static void test_lane() {
  for (u32 P = 1; P <= PRIO_MAX; ++P)
    for (u32 pr = 0; pr < 256; ++pr) {
      const u32 l = prio_lane(pr, P);
      CHECK(l <= P && l == P - (pr < P ? pr : P));
    }
}

static void test_walk() {
  CHECK(walk_exact({}) == 0);
  CHECK(walk_exact({0x08}) == 0);
  CHECK(walk_exact({0x08, 0x00}) == 0);                  // the octet is missing
  CHECK(walk_exact({0x08, 0x00, 7}) == 7);
  CHECK(walk_exact({0x18, 0x00, 2, 9}) == 9);            // behind delivery-mode
  CHECK(walk_exact({0x08, 0x01, 0x00, 0x00, 5}) == 5);   // a continuation word
  CHECK(walk_exact({0x08, 0x01, 5}) == 0);               // the continuation word is cut
  CHECK(walk_exact({0x28, 0x00, 0, 0, 0, 1, 0xaa, 4}) == 4);            // behind a table of one byte
  CHECK(walk_exact({0x28, 0x00, 0xff, 0xff, 0xff, 0xff, 0xaa, 4}) == 0);  // a table length past the end
  CHECK(walk_exact({0x88, 0x00, 2, 'a', 'b', 3}) == 3);  // behind content-type
  CHECK(walk_exact({0x88, 0x00, 200, 'a', 'b', 3}) == 0);
  CHECK(walk_exact({0x08, 0x80, 6, 1, 'x'}) == 6);       // message-id behind it, whole
  CHECK(walk_exact({0x08, 0x80, 6, 2, 'x'}) == 0);       // message-id cut: no properties at all
  CHECK(walk_exact({0x08, 0x40, 6, 0, 0, 0, 0, 0, 0, 0}) == 0);   // timestamp cut
}

static int pipe_mode() {
  char* line = nullptr;
  size_t cap = 0;
  ssize_t len;
  while ((len = getline(&line, &cap, stdin)) > 0) {
    std::vector<u8> v;
    if (line[0] != '-') {
      for (ssize_t i = 0; i + 1 < len && line[i] != '\n'; i += 2) {
        unsigned b = 0;
        if (std::sscanf(line + i, "%2x", &b) != 1) return 2;
        v.push_back((u8)b);
      }
    }
    std::printf("%u\n", walk_exact(v));
  }
  std::free(line);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "pipe") return pipe_mode();
  test_split();
  test_lane();
  test_walk();
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
