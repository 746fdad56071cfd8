// Checks narwhal_amd/csrc/msg_plan.h on the CPU: the message pipeline's chunk cuts against worked
// values and their post-condition over a sweep of batches, the vote-slot count and its limit, the
// two arena layouts against the sizes written out here, the pinned stage's layout, and the
// schedule's truth table.  Built by tests/test_msg_plan_host.py with the address and
// undefined-behaviour sanitizers and run as a child process.  Exit status 0 and a last line "ok"
// mean every check held.
#include <cstdio>
#include <random>
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

using Cuts = std::vector<size_t>;
constexpr uint64_t MiB = 1ull << 20;

Settings with_chunk(uint64_t msg_chunk) {
  Settings s;
  s.msg_chunk = msg_chunk;
  return s;
}
std::vector<uint64_t> offsets_of(const std::vector<uint64_t>& sizes) {
  std::vector<uint64_t> hoff(sizes.size() + 1, 0);
  for (size_t i = 0; i < sizes.size(); ++i) hoff[i + 1] = hoff[i] + sizes[i];
  return hoff;
}
Cuts cuts_of(size_t m, uint64_t size, uint64_t msg_chunk) {
  const std::vector<uint64_t> hoff = offsets_of(std::vector<uint64_t>(m, size));
  return message_cuts(hoff.data(), m, with_chunk(msg_chunk));
}

void test_cuts_worked() {
  CHECK(Settings().msg_chunk == 24 * MiB);
  CHECK((cuts_of(20000, 10100, 24 * MiB) == Cuts{0, 1600, 4032, 6464, 8896, 11328, 13760, 16192, 18048, 19008, 20000}));
  const Cuts c = cuts_of(20000, 10100, 1 * MiB);
  CHECK(c.size() == 312 && c.front() == 0 && c.back() == 20000);
  for (size_t k = 1; k + 1 < c.size(); ++k) CHECK(c[k] == 64 * k);
  CHECK((cuts_of(20000, 10100, 0) == Cuts{0, 20000}));
  CHECK((cuts_of(129, 70000, 1 * MiB) == Cuts{0, 64, 128, 129}));
  CHECK((cuts_of(256, 33000, 1 * MiB) == Cuts{0, 64, 128, 192, 256}));
  // any batch under 4 MiB travels in one copy: one chunk, whatever the chunk size
  const uint64_t chunks[] = {0, 1, 4096, 1 * MiB, 24 * MiB};
  for (uint64_t chunk : chunks) {
    CHECK((cuts_of(4000, 1048, chunk) == Cuts{0, 4000}));   // 4 MiB - 2,304 B
    CHECK((cuts_of(1000, 4194, chunk) == Cuts{0, 1000}));
    CHECK((cuts_of(1, 4 * MiB - 1, chunk) == Cuts{0, 1}));
    CHECK((cuts_of(300, 0, chunk) == Cuts{0, 300}));
  }
  CHECK(cuts_of(4096, 1024, 1 * MiB).size() > 2);   // 4 MiB exactly: staged and cut
}

void test_cuts_sweep() {
  std::mt19937_64 rng(20240607);
  const size_t ms[] = {1, 63, 64, 65, 127, 128, 129, 1000, 20000, 70000};
  const uint64_t chunks[] = {0, 1, 1 * MiB, 3 * MiB, 8 * MiB, 16 * MiB, 24 * MiB, 48 * MiB, 1ull << 40};
  for (size_t m : ms) {
    std::vector<std::vector<uint64_t>> batches;
    batches.emplace_back(m, 10100);   // constant
    batches.emplace_back(m, 70000);
    batches.emplace_back(m);          // random in 0..40000
    for (uint64_t& b : batches.back()) b = rng() % 40001;
    batches.emplace_back(m, 0);       // mostly empty with a few 3 MB messages
    for (int j = 0; j < 12; ++j) batches.back()[rng() % m] = 3000000;
    for (const auto& sizes : batches) {
      const std::vector<uint64_t> hoff = offsets_of(sizes);
      const uint64_t total = hoff[m];
      for (uint64_t chunk : chunks) {
        const Cuts cuts = message_cuts(hoff.data(), m, with_chunk(chunk));
        // the post-condition msg_plan.h states
        CHECK(cuts.size() >= 2 && cuts.front() == 0 && cuts.back() == m);
        for (size_t k = 0; k + 1 < cuts.size(); ++k) {
          CHECK(cuts[k] < cuts[k + 1]);
          if (k > 0) CHECK(cuts[k] % 64 == 0);
        }
        const uint64_t lo = std::min<uint64_t>(8 * MiB, chunk);
        if (chunk == 0 || total < 4 * MiB || total < 4 * lo) CHECK(cuts.size() == 2);
      }
    }
  }
}

void test_vote_slots() {
  CHECK(vote_slots(0, 1) == 1 && vote_slots(71, 1) == 1 && vote_slots(72, 1) == 2);
  CHECK(vote_slots(202000000, 1) == 202000000 / 72 + 1);
  CHECK(vote_slots(202000000, 2) == 202000000 / 72 + 1 + 128);
  CHECK(vote_slots(202000000, 10) == 202000000 / 72 + 1 + 640);
  // slot indices travel as uint32
  CHECK(vote_slots(72ull * 0xFFFFFFFEull, 1) == 0xFFFFFFFFull);
  CHECK(vote_slots(72ull * 0xFFFFFFFFull, 1) == 0);
  CHECK(vote_slots(72ull * 0xFFFFFFFEull, 2) == 0);
}

bool aligned(size_t x) { return x % 256 == 0; }

// fields in order with their sizes: each on a 256-byte boundary, none reaching into the next
struct Field { size_t at, size; };
void check_fields(const std::vector<Field>& f, size_t bytes) {
  CHECK(!f.empty() && f.front().at == 0);
  for (size_t i = 0; i < f.size(); ++i) {
    CHECK(aligned(f[i].at));
    const size_t end = i + 1 < f.size() ? f[i + 1].at : bytes;
    CHECK(f[i].at + f[i].size <= end && end - (f[i].at + f[i].size) < 256);
  }
}

void test_layouts() {
  CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512);
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  for (size_t m : {(size_t)1, (size_t)64, (size_t)65, (size_t)20000}) {
    const uint64_t totals[] = {0, 1, 239, 240, 10100 * (uint64_t)m, 5 * MiB + 17, 1ull << 31};
    for (uint64_t total : totals) {
      // the call arena: the sizes as the host call needs them
      const CallArena c = call_arena(m, total);
      CHECK(c.bytes == al(total + 16) + al(8 * (m + 1)) + al(4 * m) + al(16 * m) + al(32 * m));
      check_fields({{c.data, total + 16}, {c.offsets, 8 * (m + 1)}, {c.codes, 4 * m}, {c.rec, 16 * m}, {c.digests, 32 * m}}, c.bytes);

      const uint64_t vts[] = {1, 64, 65, vote_slots(total, 1), vote_slots(total, 8), 12345};
      for (uint64_t vt : vts) {
        for (int ysplit = 0; ysplit < 2; ++ysplit) {
          // the message arena's size, stated independently: the same whoever owns the records
          const size_t need = al(total + 128 * (m + 2)) + al(32 * m) * 3 + al(64 * m) + al(32 * vt) + al(64 * vt) + al(4 * vt) +
                              al(4) + al(4 * m) + al(16 * m) + al(4 * m) + al(8 * ((m + 63) / 64)) + al(8 * ((vt + 63) / 64)) +
                              (ysplit ? 3 * al(32 * vt) + al(4 * vt) + 3 * al(32 * m) + al(4 * m) : 0);
          for (int own_rec = 0; own_rec < 2; ++own_rec) {
            const MsgArena a = msg_arena(m, total, vt, ysplit != 0, own_rec != 0);
            CHECK(a.bytes == need);
            std::vector<Field> f = {{a.hashbuf, total + 128 * (m + 2)}, {a.eq_msg, 32 * m}, {a.eq_pk, 32 * m}, {a.eq_sig, 64 * m},
                                    {a.cdig, 32 * m}, {a.v_pk, 32 * vt}, {a.v_sig, 64 * vt}, {a.v_msg, 4 * vt}, {a.v_total, 4},
                                    {a.hmatch, 4 * m}};
            if (own_rec) f.push_back({a.rec, 16 * m});
            f.push_back({a.rec_n, 4 * m});
            f.push_back({a.sbits, 8 * ((m + 63) / 64)});
            f.push_back({a.lbits, 8 * ((vt + 63) / 64)});
            if (ysplit) {
              for (size_t at : {a.sr_x, a.sr_z, a.sr_p}) f.push_back({at, 32 * vt});
              f.push_back({a.sr_meta, 4 * vt});
              for (size_t at : {a.srs_x, a.srs_z, a.srs_p}) f.push_back({at, 32 * m});
              f.push_back({a.srs_meta, 4 * m});
            }
            // a caller's own records leave their share of the arena unused at its end
            check_fields(f, own_rec ? a.bytes : a.bytes - al(16 * m));
          }
        }
      }
    }
  }
}

void test_stage() {
  // the chunk counts (one uint32 per chunk) end where the host offsets begin, at the chunk limit too
  CHECK(STAGE_COUNTS_AT == 0 && STAGE_OFFSETS_AT == 65536 && stage_chunk_limit() == 16384);
  CHECK(STAGE_COUNTS_AT + 4 * stage_chunk_limit() <= STAGE_OFFSETS_AT);
  CHECK(STAGE_OFFSETS_AT % 8 == 0);
  const size_t stage = 1u << 20;
  CHECK(stage_holds_offsets(1, stage) && stage_holds_offsets(20000, stage));
  CHECK(stage_holds_offsets(122879, stage) && !stage_holds_offsets(122880, stage));
  CHECK(STAGE_OFFSETS_AT + 8 * (122879 + 1) <= stage);
}

void test_schedule() {
  const Settings dflt;
  const size_t nchs[] = {1, 2, 3, 4, 6, 10, 311};
  const size_t at[] = {0, 0, 1, 1, 2, 3, 103};
  for (int i = 0; i < 7; ++i) CHECK(schedule(nchs[i], true, true, dflt).strict_at == at[i]);
  for (size_t nch : nchs)
    for (int bits = 0; bits < 16; ++bits) {
      const bool deferrable = bits & 1, config = bits & 2;
      Settings s;
      s.sign_defer = bits & 4;
      s.strict_y = bits & 8;
      const MsgSchedule p = schedule(nch, deferrable, config, s);
      CHECK(p.chunked == (nch > 1));
      CHECK(p.defer == (nch > 1 && deferrable));
      CHECK(p.ysplit == (nch > 1 && deferrable && s.sign_defer));
      CHECK(p.strict_y == (nch > 1 && deferrable && s.sign_defer && config && s.strict_y));
      CHECK(p.strict_at == (nch >= 3 ? nch / 3 : 0) && p.strict_at < nch);
      if (nch == 1) CHECK(!p.defer && !p.ysplit && !p.strict_y);
    }
  // the production pipeline, and each A/B switch on its own
  const MsgSchedule prod = schedule(10, true, true, dflt);
  CHECK(prod.chunked && prod.defer && prod.ysplit && prod.strict_y);
  Settings s = dflt;
  s.sign_defer = false;
  CHECK(schedule(10, true, true, s).defer && !schedule(10, true, true, s).ysplit && !schedule(10, true, true, s).strict_y);
  s = dflt;
  s.strict_y = false;
  CHECK(schedule(10, true, true, s).ysplit && !schedule(10, true, true, s).strict_y);
  CHECK(schedule(10, true, false, dflt).ysplit && !schedule(10, true, false, dflt).strict_y);
}

}  // namespace

int main() {
  test_cuts_worked();
  std::printf("message_cuts worked\n");
  test_cuts_sweep();
  std::printf("message_cuts sweep\n");
  test_vote_slots();
  std::printf("vote_slots\n");
  test_layouts();
  std::printf("layouts\n");
  test_stage();
  std::printf("pinned stage\n");
  test_schedule();
  std::printf("schedule\n");
  if (g_failures) {
    std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)g_failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
