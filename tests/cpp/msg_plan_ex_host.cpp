// Checks what nwc_sanitize_messages_ex adds to narwhal_amd/csrc/msg_plan.h on the CPU: the call
// arena with the per-message gc_rounds, vote targets, vote signatures and "voted" bytes, and the
// message arena with its own digest array, for m = 1, 63, 64, 65 and 4,097 -- every field on a
// 256-byte boundary, large enough for its array, no two overlapping, the total as written out here
// -- and that a call without per-message state and without a signer has the layout it had before
// these arrays existed.  Built by tests/test_msg_plan_ex_host.py with the address and
// undefined-behaviour sanitizers and run as a child process.  Exit status 0 and a last line "ok"
// mean every check held.
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

// Every field 256-byte aligned, inside [0, bytes), and no two overlapping; the fields as a whole
// fill the arena up to the padding of each.
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

void test_call_arena() {
  CHECK(MSG_TARGET_STRIDE == 80);
  for (size_t m : MS) {
    for (uint64_t total : TOTALS) {
      const size_t parent = al(total + 16) + al(8 * (m + 1)) + al(4 * m) + al(16 * m) + al(32 * m);
      // without per-message state and without a signer: the layout from before the new arrays
      const CallArena p = call_arena(m, total), q = call_arena(m, total, false, false);
      CHECK(p.bytes == parent && q.bytes == parent);
      CHECK(p.data == 0 && p.offsets == al(total + 16) && p.codes == p.offsets + al(8 * (m + 1)));
      CHECK(p.rec == p.codes + al(4 * m) && p.digests == p.rec + al(16 * m));
      CHECK(p.data == q.data && p.offsets == q.offsets && p.codes == q.codes && p.rec == q.rec && p.digests == q.digests);
      for (int own = 0; own < 2; ++own) {
        for (int votes = 0; votes < 2; ++votes) {
          const CallArena c = call_arena(m, total, own != 0, votes != 0);
          // the parent's fields stay where they were, whatever is added behind them
          CHECK(c.data == p.data && c.offsets == p.offsets && c.codes == p.codes && c.rec == p.rec && c.digests == p.digests);
          std::vector<Field> f{{c.data, (size_t)total + 16}, {c.offsets, 8 * (m + 1)}, {c.codes, 4 * m}, {c.rec, 16 * m},
                               {c.digests, 32 * m}};
          size_t need = parent;
          if (own) {
            f.push_back({c.gc_rounds, 8 * m});
            f.push_back({c.targets, 80 * m});
            CHECK(c.gc_rounds >= parent && c.gc_rounds % 8 == 0 && c.targets % 4 == 0);
            need += al(8 * m) + al(80 * m);
          }
          if (votes) {
            f.push_back({c.vote_sigs, 64 * m});
            f.push_back({c.voted, m});
            CHECK(c.vote_sigs >= parent && c.vote_sigs % 4 == 0);
            need += al(64 * m) + al(m);
          }
          CHECK(c.bytes == need);
          check_fields(f, c.bytes);
        }
      }
    }
  }
}

void test_msg_arena() {
  for (size_t m : MS) {
    for (uint64_t total : TOTALS) {
      for (size_t nch : {(size_t)1, (size_t)5}) {
        const uint64_t vt = vote_slots(total, nch);
        for (int ysplit = 0; ysplit < 2; ++ysplit) {
          for (int own_rec = 0; own_rec < 2; ++own_rec) {
            const MsgArena p = msg_arena(m, total, vt, ysplit != 0, own_rec != 0);
            const MsgArena q = msg_arena(m, total, vt, ysplit != 0, own_rec != 0, false);
            const MsgArena a = msg_arena(m, total, vt, ysplit != 0, own_rec != 0, true);
            CHECK(p.bytes == q.bytes && p.lbits == q.lbits && p.srs_meta == q.srs_meta);
            // the digest array behind everything else; nothing before it moves
            CHECK(a.bytes == p.bytes + al(32 * m));
            CHECK(a.hashbuf == p.hashbuf && a.eq_pk == p.eq_pk && a.v_total == p.v_total && a.rec == p.rec && a.rec_n == p.rec_n);
            CHECK(a.sbits == p.sbits && a.lbits == p.lbits && a.srs_meta == p.srs_meta);
            CHECK(a.digests % 256 == 0 && a.digests + 32 * m <= a.bytes);
            const size_t last = ysplit ? a.srs_meta + 4 * m : a.lbits + 8 * ((vt + 63) / 64);
            CHECK(a.digests >= last);
            CHECK(a.digests + al(32 * m) + (own_rec ? 0 : al(16 * m)) == a.bytes);
          }
        }
      }
    }
  }
}

}  // namespace

int main() {
  test_call_arena();
  std::printf("call arena\n");
  test_msg_arena();
  std::printf("message arena\n");
  if (g_failures) {
    std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)g_failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
