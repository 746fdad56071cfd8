// Checks what nwc_sanitize_messages_view adds to narwhal_amd/csrc/msg_plan.h on the CPU: the call
// arena with the view records, the body and the body allocator's counter for m = 1, 63, 64, 65 and
// 4,097 -- every field on a 256-byte boundary, large enough for its array, no two overlapping, the
// total as written out here -- and that call_arena without views returns exactly the offsets it
// returned before the views existed, for all four (own_state, votes) combinations.  Built by
// tests/test_msg_plan_view_host.py with the address and undefined-behaviour sanitizers and run as a
// child process.  Exit status 0 and a last line "ok" mean every check held.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "msg_plan.h"

namespace {

using namespace nwc::plan;

uint64_t g_failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      if (++g_failures <= 50) std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    }                                                                    \
  } while (0)

struct Field { size_t at, size; };
size_t al(size_t x) { return (x + 255) / 256 * 256; }

void check_fields(std::vector<Field> f, size_t bytes) {
  size_t sum = 0;
  for (const Field& x : f) {
    CHECK(x.at % 256 == 0);
    CHECK(x.at + x.size <= bytes);
    sum += al(x.size);
  }
  CHECK(sum == bytes);
  std::sort(f.begin(), f.end(), [](const Field& a, const Field& b) { return a.at < b.at; });
  for (size_t i = 0; i + 1 < f.size(); ++i) CHECK(f[i].at + f[i].size <= f[i + 1].at);
  // a scribble test under the address sanitizer: every byte of every field is inside one allocation
  // of `bytes` bytes and is written by exactly one field
  std::vector<unsigned char> arena(bytes, 0);
  for (const Field& x : f)
    for (size_t k = 0; k < x.size; ++k) arena[x.at + k]++;
  for (size_t k = 0; k < bytes; ++k) CHECK(arena[k] <= 1);
}

const size_t MS[] = {1, 63, 64, 65, 4097};
const uint64_t TOTALS[] = {0, 1, 255, 4096, 1234567};

// the layout of a call without views, written out as it was before the views existed
struct Before { size_t data, offsets, codes, rec, digests, gc_rounds, targets, vote_sigs, voted, bytes; };
Before before(size_t m, uint64_t total, bool own, bool votes) {
  Before b{};
  size_t at = 0;
  auto take = [&](size_t n) { const size_t r = at; at += al(n); return r; };
  b.data = take(total + 16);
  b.offsets = take(8 * (m + 1));
  b.codes = take(4 * m);
  b.rec = take(16 * m);
  b.digests = take(32 * m);
  if (own) {
    b.gc_rounds = take(8 * m);
    b.targets = take(80 * m);
  }
  if (votes) {
    b.vote_sigs = take(64 * m);
    b.voted = take(m);
  }
  b.bytes = at;
  return b;
}

void test_body_bound() {
  CHECK(MSG_VIEW_BYTES == 160);
  CHECK(view_body_bound(1000, 3) == 1192);
  CHECK(view_body_bound(0, 0) == 0 && view_body_bound(0, 1) == 64);
  // the largest body a message can need stays below its wire length + 64: a header of P payload
  // entries and Q parents under a 44-symbol key, a certificate with V votes of 116 bytes
  for (uint64_t P : {0ull, 1ull, 64ull, 1000ull})
    for (uint64_t Q : {0ull, 1ull, 67ull, 1000ull})
      for (uint64_t V : {0ull, 1ull, 67ull, 1000ull}) {
        const uint64_t wire = 4 + 52 + 8 + 8 + 36 * P + 8 + 32 * Q + 32 + 64 + (V ? 8 + 116 * V : 0);
        const uint64_t body = ((36 * P + 15) & ~15ull) + ((32 * Q + 15) & ~15ull) + ((8 * V + 15) & ~15ull);
        CHECK(body < view_body_bound(wire, 1));
      }
}

void test_call_arena() {
  for (size_t m : MS) {
    for (uint64_t total : TOTALS) {
      for (int own = 0; own < 2; ++own) {
        for (int votes = 0; votes < 2; ++votes) {
          const Before b = before(m, total, own != 0, votes != 0);
          // without views: today's offsets, with the flag left out and with it false
          for (const CallArena& p : {call_arena(m, total, own != 0, votes != 0), call_arena(m, total, own != 0, votes != 0, false)}) {
            CHECK(p.data == b.data && p.offsets == b.offsets && p.codes == b.codes && p.rec == b.rec && p.digests == b.digests);
            CHECK(p.gc_rounds == b.gc_rounds && p.targets == b.targets && p.vote_sigs == b.vote_sigs && p.voted == b.voted);
            CHECK(p.bytes == b.bytes);
            CHECK(p.views == 0 && p.body == 0 && p.body_used == 0);
          }
          // with views: nothing before them moves; the three fields behind everything else
          const CallArena c = call_arena(m, total, own != 0, votes != 0, true);
          CHECK(c.data == b.data && c.offsets == b.offsets && c.codes == b.codes && c.rec == b.rec && c.digests == b.digests);
          CHECK(c.gc_rounds == b.gc_rounds && c.targets == b.targets && c.vote_sigs == b.vote_sigs && c.voted == b.voted);
          const size_t body = (size_t)total + 64 * m;
          CHECK(c.views == b.bytes && c.body == c.views + al(160 * m) && c.body_used == c.body + al(body));
          CHECK(c.views % 8 == 0 && c.body % 16 == 0 && c.body_used % 8 == 0);
          CHECK(c.bytes == b.bytes + al(160 * m) + al(body) + 256);
          std::vector<Field> f{{c.data, (size_t)total + 16}, {c.offsets, 8 * (m + 1)}, {c.codes, 4 * m}, {c.rec, 16 * m},
                               {c.digests, 32 * m}, {c.views, 160 * m}, {c.body, body}, {c.body_used, 8}};
          if (own) {
            f.push_back({c.gc_rounds, 8 * m});
            f.push_back({c.targets, 80 * m});
          }
          if (votes) {
            f.push_back({c.vote_sigs, 64 * m});
            f.push_back({c.voted, m});
          }
          check_fields(f, c.bytes);
        }
      }
    }
  }
}

}  // namespace

int main() {
  test_body_bound();
  std::printf("body bound\n");
  test_call_arena();
  std::printf("call arena\n");
  if (g_failures) {
    std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)g_failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
