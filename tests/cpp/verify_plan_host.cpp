// Checks narwhal_amd/csrc/verify_plan.h on the CPU: the environment settings against fake
// environments, the host pipelines' chunk cuts, launch_verify's routing table and its invariants
// over every combination of the device view's facts, and the poll of the "written" bytes.  Built by
// tests/test_verify_plan_host.py with the address and undefined-behaviour sanitizers and run as a
// child process.  Exit status 0 and a last line "ok" mean every check held.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "verify_plan.h"

namespace {

using namespace nwc::plan;

uint64_t g_failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      if (++g_failures <= 50) std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    }                                                                    \
  } while (0)

using Env = std::map<std::string, std::string>;
Settings parse(const Env& env) {
  return Settings::parse([&](const char* name) -> const char* {
    auto it = env.find(name);
    return it == env.end() ? nullptr : it->second.c_str();
  });
}

void test_settings() {
  const Settings d = parse({});
  // README "Switches"
  CHECK(d.auto_keys == 256 && d.comb16 && d.verify_path == VPath::Default);
  CHECK(d.verify_max_launch == (16ull << 20) && d.verify_keep_bytes == (256ull << 20));
  CHECK(d.cold && d.cold_max == 3072 && !d.host_timing && d.host_staging_threads == 8 && d.force_fallback_every == 0);
  CHECK(d.sign_defer && d.strict_y && d.digest_sched == -1 && d.zero_copy && d.spin_wait);
  CHECK(d.host_pair && d.host_pair_first == 65536 && d.host_pair_growth == 2 && d.host_pair_max == 1048576);
  CHECK(d.host_chunk == 131072 && d.host_chunk_growth == 3 && d.host_chunk_max == 1048576 && d.msg_chunk == (24ull << 20));
  CHECK(d.sign_wide_max == 256 && d.verifier_group_eq == 4096);
  CHECK(d.launch_keys == 1 && d.straus_nq == 12 && d.force_windows == 0 && d.msm_group == 0 && d.msm_adapt == 1);

  // roundings and clamps
  CHECK(parse({{"NWC_HOST_PAIR_FIRST", "100"}}).host_pair_first == 64);
  CHECK(parse({{"NWC_HOST_PAIR_FIRST", "10"}}).host_pair_first == 64);
  CHECK(parse({{"NWC_HOST_PAIR_MAX", "10000"}}).host_pair_max == 9984);
  CHECK(parse({{"NWC_HOST_PAIR_GROWTH", "0"}}).host_pair_growth == 1);
  CHECK(parse({{"NWC_HOST_CHUNK", "200"}}).host_chunk == 192);
  CHECK(parse({{"NWC_HOST_CHUNK", "0"}}).host_chunk == 0);
  CHECK(parse({{"NWC_HOST_CHUNK", "63"}}).host_chunk == 0);
  CHECK(parse({{"NWC_HOST_CHUNK_GROWTH", "0"}}).host_chunk_growth == 1);
  CHECK(parse({{"NWC_HOST_CHUNK_MAX", "10000"}}).host_chunk_max == 9984);
  CHECK(parse({{"NWC_HOST_CHUNK_MAX", "1"}}).host_chunk_max == 64);
  CHECK(parse({{"NWC_VERIFY_MAX_LAUNCH", "1"}}).verify_max_launch == 65536);
  CHECK(parse({{"NWC_VERIFY_MAX_LAUNCH", "100001"}}).verify_max_launch == 99968);
  CHECK(parse({{"NWC_VERIFIER_GROUP_EQ", "0"}}).verifier_group_eq == 1);
  CHECK(parse({{"NWC_VERIFIER_GROUP_EQ", "1000000"}}).verifier_group_eq == 65536);
  CHECK(parse({{"NWC_HOST_STAGING_THREADS", "0"}}).host_staging_threads == 1);
  CHECK(parse({{"NWC_HOST_STAGING_THREADS", "3"}}).host_staging_threads == 3);
  CHECK(parse({{"NWC_AUTO_KEYS", "0"}}).auto_keys == 0);
  CHECK(parse({{"NWC_COLD_MAX", "17"}}).cold_max == 17);
  CHECK(parse({{"NWC_VERIFY_KEEP_BYTES", "0"}}).verify_keep_bytes == 0);
  CHECK(parse({{"NWC_MSG_CHUNK", "0"}}).msg_chunk == 0);
  CHECK(parse({{"NWC_SIGN_WIDE_MAX", "0"}}).sign_wide_max == 0);
  CHECK(parse({{"NWC_FORCE_FALLBACK_EVERY", "7"}}).force_fallback_every == 7);
  CHECK(parse({{"NWC_DIGEST_SCHED", "1"}}).digest_sched == 1 && parse({{"NWC_DIGEST_SCHED", "0"}}).digest_sched == 0);
  CHECK(parse({{"NWC_HOST_TIMING", ""}}).host_timing && parse({{"NWC_HOST_TIMING", "0"}}).host_timing);
  CHECK(parse({{"NWC_LAUNCH_KEYS", "0"}}).launch_keys == 0 && parse({{"NWC_STRAUS_NQ", "9"}}).straus_nq == 9);
  CHECK(parse({{"NWC_FORCE_WINDOWS", "5"}}).force_windows == 5 && parse({{"NWC_MSM_GROUP", "128"}}).msm_group == 128);

  // on/off switches: only the literal "0" is off ...
  struct Sw { const char* name; bool Settings::*field; };
  const Sw sws[] = {{"NWC_COMB16", &Settings::comb16},         {"NWC_COLD", &Settings::cold},
                    {"NWC_SIGN_DEFER", &Settings::sign_defer}, {"NWC_STRICT_Y", &Settings::strict_y},
                    {"NWC_ZERO_COPY", &Settings::zero_copy},   {"NWC_SPIN_WAIT", &Settings::spin_wait},
                    {"NWC_HOST_PAIR", &Settings::host_pair}};
  for (const Sw& sw : sws) {
    CHECK(!(parse({{sw.name, "0"}}).*sw.field));
    CHECK(parse({{sw.name, "00"}}).*sw.field);
    CHECK(parse({{sw.name, ""}}).*sw.field);
    CHECK(parse({{sw.name, "1"}}).*sw.field);
    CHECK(parse({{sw.name, "off"}}).*sw.field);
  }
  // ... except NWC_MSM_ADAPT, which is a number
  CHECK(parse({{"NWC_MSM_ADAPT", "0"}}).msm_adapt == 0 && parse({{"NWC_MSM_ADAPT", "00"}}).msm_adapt == 0);
  CHECK(parse({{"NWC_MSM_ADAPT", ""}}).msm_adapt == 0 && parse({{"NWC_MSM_ADAPT", "2"}}).msm_adapt == 1);
  CHECK(parse({{"NWC_VERIFY_PATH", "half"}}).verify_path == VPath::Half);
  CHECK(parse({{"NWC_VERIFY_PATH", "full"}}).verify_path == VPath::Full);
  for (const char* other : {"", "Half", "FULL", "default", "half ", "1"})
    CHECK(parse({{"NWC_VERIFY_PATH", other}}).verify_path == VPath::Default);
  // the cold kernel's s B is a sum over the basepoint comb
  CHECK(!parse({{"NWC_COMB16", "0"}}).cold);
  CHECK(!parse({{"NWC_COMB16", "0"}, {"NWC_COLD", "1"}}).cold);
  CHECK(parse({{"NWC_COMB16", "1"}}).cold);
}

void test_chunk_cuts() {
  using V = std::vector<uint64_t>;
  CHECK((chunk_cuts(262144, 131072, 3, 1 << 20) == V{0, 131072, 262144}));
  CHECK((chunk_cuts(525288, 131072, 3, 1 << 20) == V{0, 131072, 525288}));   // the 1,000-equation sliver folded in
  CHECK((chunk_cuts(131072, 65536, 2, 1 << 20) == V{0, 65536, 131072}));
  const V c = chunk_cuts(150001, 4096, 2, 9984);
  CHECK(c.size() > 4 && c[0] == 0 && c[1] == 4096 && c[2] == 12288 && c[3] == 22272 && c[4] == 32256 && c.back() == 150001);
  CHECK(longest_chunk(c) <= 9984 + 4096 / 2 && longest_chunk(V{0, 5, 20, 30}) == 15);
  // (first, growth, max) as Settings produces them: first and max multiples of 64, growth >= 1
  const uint64_t triples[][3] = {{131072, 3, 1 << 20}, {65536, 2, 1 << 20}, {4096, 2, 9984}, {64, 1, 64},
                                 {192, 5, 64},         {4096, 1, 1 << 20},  {128, 7, 100032}};
  for (const auto& t : triples) {
    const uint64_t first = t[0];
    for (uint64_t n = 1; n < 400000; n += 997) {
      const V cuts = chunk_cuts(n, first, t[1], t[2]);
      CHECK(cuts.size() >= 2 && cuts.front() == 0 && cuts.back() == n);
      const size_t nch = cuts.size() - 1;
      for (size_t k = 0; k < nch; ++k) {
        CHECK(cuts[k] < cuts[k + 1]);
        if (k > 0) CHECK(cuts[k] % 64 == 0);
        if (k + 1 < nch) CHECK(cuts[k + 1] - cuts[k] >= first);
      }
      if (nch > 1) CHECK(cuts[nch] - cuts[nch - 1] >= first / 2);
    }
  }
}

bool same(const Route& a, const Route& b) {
  return ((a.error == nullptr && b.error == nullptr) || (a.error && b.error && std::strcmp(a.error, b.error) == 0)) &&
         a.kernel == b.kernel && a.comb == b.comb && a.lk_build == b.lk_build &&
         a.list_pass == b.list_pass && a.fallback == b.fallback && a.torsion == b.torsion && a.zero_words == b.zero_words &&
         a.zero_fb_count == b.zero_fb_count && a.scratch == b.scratch && a.scratch_order == b.scratch_order;
}
// a route over the table slots and lists
Route listed(Kernel k, bool comb, bool lk, bool list, bool fb, Torsion t, uint64_t zero, bool zero_fb, bool order = true) {
  Route r;
  r.kernel = k; r.comb = comb; r.lk_build = lk; r.list_pass = list; r.fallback = fb; r.torsion = t;
  r.zero_words = zero; r.zero_fb_count = zero_fb; r.scratch = true; r.scratch_order = order;
  return r;
}
Route single(Kernel k, bool comb, uint64_t zero) {
  Route r;
  r.kernel = k; r.comb = comb; r.zero_words = zero;
  return r;
}
Route error(const char* msg, bool late = false, bool comb = false, bool lk = false) {
  Route r;
  r.error = msg; r.scratch = late; r.comb = comb; r.lk_build = lk;
  return r;
}
Request req(uint64_t n, bool strict, int flags = 0) {
  Request q;
  q.n = n; q.strict = strict; q.flags = flags;
  return q;
}

void test_route_table() {
  DeviceView none;   // no cache of any kind; the basepoint comb, the cold kernel and launch keys on
  none.comb16 = true;
  none.fb_cap = 1 << 20;
  DeviceView cm = none;   // a committee cache with combs
  cm.cm_n = 100;
  cm.cm_comb = true;
  DeviceView ak = none;   // an auto cache
  ak.ak_n = 5;
  ak.ak_comb = true;
  Request q;
  const Torsion NoT = Torsion::None;

  // 1. auto-cache latency launch
  q = req(3, false, LV_ALL_CACHED | LV_AUTO | LV_OUT_ZEROED); q.vbytes = true;
  CHECK(same(route_verify(ak, q), single(Kernel::AutoWide, false, 0)));
  q = req(3, true, LV_ALL_CACHED | LV_AUTO);
  CHECK(same(route_verify(ak, q), single(Kernel::AutoWide, false, 2)));   // its word and the missing-key word
  // 2. committee latency launch, with and without verdict bytes
  q = req(67, false, LV_ALL_CACHED | LV_OUT_ZEROED); q.vbytes = true;
  CHECK(same(route_verify(cm, q), single(Kernel::CommitteeWide, true, 0)));
  q = req(67, false, LV_ALL_CACHED);
  CHECK(same(route_verify(cm, q), single(Kernel::CommitteeWide, true, 3)));
  q = req(67, false, LV_ALL_CACHED | LV_OUT_ZEROED);
  CHECK(same(route_verify(cm, q), single(Kernel::CommitteeWide, true, 0)));
  // 3. zero-copy cold
  q = req(10, false, LV_OUT_ZEROED); q.vbytes = true;
  CHECK(same(route_verify(none, q), single(Kernel::ZeroCopyCold, false, 0)));
  // 4. staged cold at 3072, the one-lane ladder at 3073
  CHECK(same(route_verify(none, req(3072, false, LV_OUT_ZEROED)), listed(Kernel::Cold, false, false, false, true, NoT, 0, true)));
  CHECK(same(route_verify(none, req(3072, false)), listed(Kernel::Cold, false, false, false, true, NoT, 48, true)));
  CHECK(same(route_verify(none, req(3073, false, LV_OUT_ZEROED)),
             listed(Kernel::Half, false, false, false, true, Torsion::AfterAll, 0, true)));
  CHECK(same(route_verify(none, req(3072, true)), listed(Kernel::Cold, false, false, false, true, NoT, 48, true)));
  DeviceView warm = none;   // NWC_COLD=0: the torsion test beside the one-lane ladder
  warm.cold = false;
  CHECK(same(route_verify(warm, req(1024, false)), listed(Kernel::Half, false, false, false, true, Torsion::Beside, 0, true)));
  CHECK(same(route_verify(warm, req(1025, false)), listed(Kernel::Half, false, false, false, true, Torsion::AfterAll, 0, true)));
  // 5. 1024 against 1025 on the committee comb path
  CHECK(same(route_verify(cm, req(1024, false)), listed(Kernel::CombWide, true, false, true, true, Torsion::AfterList, 16, true)));
  CHECK(same(route_verify(cm, req(1025, false)), listed(Kernel::Comb, true, false, true, true, Torsion::AfterList, 0, true)));
  CHECK(same(route_verify(cm, req(1025, true)), listed(Kernel::Comb, true, false, true, true, NoT, 0, true)));
  DeviceView cm_nocomb16 = cm;   // NWC_COMB16=0: the latency kernel still, the cached ladder above it
  cm_nocomb16.comb16 = false;
  cm_nocomb16.cold = false;
  CHECK(same(route_verify(cm_nocomb16, req(1024, false)),
             listed(Kernel::CombWide, true, false, true, true, Torsion::AfterList, 16, true)));
  CHECK(same(route_verify(cm_nocomb16, req(1025, false)),
             listed(Kernel::HalfCached, false, false, false, true, Torsion::AfterAll, 0, true)));
  // 6. launch keys at 65536 against 65535, no committee, not strict
  CHECK(same(route_verify(none, req(65536, false)), listed(Kernel::Comb, true, true, true, true, Torsion::AfterList, 0, true)));
  CHECK(same(route_verify(none, req(65535, false)), listed(Kernel::Half, false, false, false, true, Torsion::AfterAll, 0, true)));
  DeviceView nolk = none;
  nolk.launch_keys = false;
  CHECK(same(route_verify(nolk, req(65536, false)), listed(Kernel::Half, false, false, false, true, Torsion::AfterAll, 0, true)));
  // 7. strict at 65536 takes no launch keys
  CHECK(same(route_verify(none, req(65536, true)), listed(Kernel::Half, false, false, false, true, NoT, 0, true)));
  // 8. half and full paths
  DeviceView cm_half = cm, cm_full = cm, none_full = none;
  cm_half.path = VPath::Half;
  cm_full.path = none_full.path = VPath::Full;
  CHECK(same(route_verify(cm_half, req(2000, false)), listed(Kernel::HalfCached, false, false, false, true, Torsion::AfterAll, 0, true)));
  CHECK(same(route_verify(cm_half, req(100, false, LV_ALL_CACHED)),
             listed(Kernel::HalfCached, false, false, false, true, Torsion::Beside, 0, true)));
  CHECK(same(route_verify(cm_full, req(2000, false)), listed(Kernel::Full, false, false, false, false, Torsion::AfterAll, 0, false)));
  CHECK(same(route_verify(none_full, req(100, false)), listed(Kernel::Full, false, false, false, false, Torsion::Beside, 0, false)));
  CHECK(same(route_verify(none_full, req(65536, true)), listed(Kernel::Full, false, false, false, false, NoT, 0, false)));
  // 9. paired strict: its own half of the slots, no fallback pass of its own, no ordering by scratch_free
  q = req(65536, true); q.pair = true;
  CHECK(same(route_verify(none, q), listed(Kernel::Half, false, false, false, false, NoT, 0, true, false)));
  // 10. deferred list, with and without SignRecs
  q = req(5000, false, LV_DEFER_LIST); q.list_base = 64;
  CHECK(same(route_verify(cm, q), listed(Kernel::Comb, true, false, false, false, NoT, 0, false)));
  q.sign_recs = true;
  CHECK(same(route_verify(cm, q), listed(Kernel::CombY, true, false, false, false, NoT, 0, false)));
  q.sign_pass = true;
  CHECK(same(route_verify(cm, q), listed(Kernel::CombYSign, true, false, false, false, NoT, 0, false)));
  q = req(100, false, LV_DEFER_LIST); q.list_base = 7;
  CHECK(same(route_verify(cm, q), listed(Kernel::CombWide, true, false, false, false, NoT, 2, false)));
  // ... and the chunked host call's launches: the sign deferred, the lists per launch
  q = req(131072, false); q.sign_recs = true;
  CHECK(same(route_verify(cm, q), listed(Kernel::CombY, true, false, true, true, Torsion::AfterList, 2048, true)));
  q.sign_pass = true;
  CHECK(same(route_verify(none, q), listed(Kernel::CombYSign, true, true, true, true, Torsion::AfterList, 2048, true)));
  // 11. the stamp build
  CHECK(same(route_verify(none, req(4096, true, LV_STAMP)), listed(Kernel::HalfStamp, false, false, false, true, NoT, 0, true)));
  // 12. the argument errors
  q = req(1ull << 32, false); q.vbytes = true;
  CHECK(same(route_verify(none, q), error("more than 2^32 - 1 equations in one launch")));
  const char* const e_defer = "deferred list launch off the committee-cache comb path";
  CHECK(same(route_verify(none, req(5000, false, LV_DEFER_LIST)), error(e_defer)));
  CHECK(same(route_verify(cm_nocomb16, req(100, false, LV_DEFER_LIST)), error(e_defer)));
  q = req(5000, false, LV_DEFER_LIST); q.list_base = cm.fb_cap - 4999;
  CHECK(same(route_verify(cm, q), error(e_defer)));
  const char* const e_sign = "sign-deferred launch off the comb path or off a verdict word";
  q = req(5000, false); q.sign_recs = true;
  CHECK(same(route_verify(none, q), error(e_sign)));
  q = req(5000, false, LV_DEFER_LIST); q.sign_recs = true; q.list_base = 65;
  CHECK(same(route_verify(cm, q), error(e_sign)));
  const char* const e_pair = "paired launch off the strict half-size path";
  q = req(70000, false); q.pair = true;   // (not strict: launch keys, ensured before the error as ever)
  CHECK(same(route_verify(none, q), error(e_pair, true, true, true)));
  q = req(70000, true); q.pair = true;
  CHECK(same(route_verify(cm, q), error(e_pair, true, true, false)));
  CHECK(same(route_verify(none_full, q), error(e_pair, true)));
  CHECK(splits(none, req(none.verify_max_launch + 1, false)) && !splits(none, req(none.verify_max_launch, false)));
  q = req(none.verify_max_launch + 1, false); q.vbytes = true;
  CHECK(!splits(none, q));
}

void test_route_invariants() {
  const uint64_t ns[] = {1, 1024, 1025, 3072, 3073, 65535, 65536};
  uint64_t routes = 0;
  for (int vb = 0; vb < 128 * 3; ++vb) {
    DeviceView v;
    v.cm_n = vb & 1 ? 100 : 0;
    v.cm_comb = vb & 2;
    v.comb16 = vb & 4;
    v.ak_n = vb & 8 ? 5 : 0;
    v.ak_comb = vb & 16;
    v.launch_keys = vb & 32;
    v.cold = vb & 64;
    v.path = (VPath)(vb / 128);
    v.fb_cap = 1 << 20;
    for (int qb = 0; qb < 2 * 32 * 2 * 2 * 3; ++qb) {
      Request q;
      q.strict = qb & 1;
      q.flags = (qb >> 1) & 31;
      q.vbytes = (qb >> 6) & 1;
      q.pair = (qb >> 7) & 1;
      q.sign_recs = (qb >> 8) >= 1;
      q.sign_pass = (qb >> 8) == 2;
      for (uint64_t n : ns) {
        q.n = n;
        const Route r = route_verify(v, q);
        const bool defer = q.flags & LV_DEFER_LIST;
        if (r.error) {
          CHECK(defer || q.sign_recs || q.pair);
          // only the paired error comes late: launch_verify sends a route to the scratch path (which
          // returns a late error once the scratch is ensured) iff `scratch`, and returns any other
          // error before it enqueues
          const bool late = std::strstr(r.error, "paired") != nullptr;
          CHECK(r.scratch == late && early_error(r) == !late);
          if (late) CHECK(q.pair);
          if (!late) CHECK(!r.comb && !r.lk_build);
          CHECK(!r.list_pass && !r.fallback && !r.scratch_order && r.torsion == Torsion::None && r.zero_words == 0);
          continue;
        }
        ++routes;
        CHECK(!early_error(r));
        const bool latency = r.kernel == Kernel::AutoWide || r.kernel == Kernel::CommitteeWide || r.kernel == Kernel::ZeroCopyCold;
        const bool cold = r.kernel == Kernel::Cold || r.kernel == Kernel::ZeroCopyCold;
        CHECK(latency == !r.scratch);
        CHECK(r.fallback == (v.path != VPath::Full && !q.pair && !defer && !latency));
        CHECK((r.torsion == Torsion::None) == (q.strict || cold || latency || defer));
        CHECK((r.torsion == Torsion::Beside) == (!q.strict && !r.comb && n <= 1024 && !cold && !latency && !defer));
        if (r.torsion != Torsion::None) CHECK((r.torsion == Torsion::AfterList) == r.comb);
        if (q.pair) CHECK(!r.scratch_order && !r.fallback);
        if (!q.pair) CHECK(r.scratch_order == r.scratch);
        // the comb decision is takes_comb_path's (comb_path without flags) wherever it is taken
        if (r.scratch || r.kernel == Kernel::CommitteeWide) {
          CHECK(r.comb == comb_path(v, n, q.strict, q.flags).comb);
          if (!(q.flags & LV_AUTO)) CHECK(r.comb == comb_path(v, n, q.strict).comb);
          CHECK(r.lk_build == comb_path(v, n, q.strict, q.flags).lk);
        }
        CHECK(r.list_pass == (r.comb && !defer && !latency));
        if (r.lk_build) CHECK(r.comb && !v.cm_n && n >= 65536);
        if (defer && !latency) CHECK(r.comb && deferrable_list(v) && !r.zero_fb_count);
        if (q.sign_recs && !latency) CHECK(r.kernel == (q.sign_pass ? Kernel::CombYSign : Kernel::CombY));
        if (r.kernel == Kernel::Cold) CHECK(n <= v.cold_max && v.cold && !v.cm_n);
        CHECK(r.zero_words == 0 || r.zero_words == (n + 63) / 64 + (latency ? 1 : 0));
      }
    }
  }
  CHECK(routes > 100000);
}

void test_small_call_route() {
  DeviceView none, cm, ak;
  none.comb16 = cm.comb16 = ak.comb16 = true;
  cm.cm_n = 100; cm.cm_comb = true;
  ak.ak_n = 5; ak.ak_comb = true;
  const Settings s = parse({});
  const uint64_t stage = 1 << 20;
  SmallRoute r = small_call_route(cm, s, 67, true, false, 10000, stage);
  CHECK(r.flags == (LV_OUT_ZEROED | LV_ALL_CACHED) && r.mode == SmallMode::ZeroCopyCached);
  r = small_call_route(cm, s, 67, false, false, 10000, stage);   // a committee, a key outside it: staged
  CHECK(r.flags == LV_OUT_ZEROED && r.mode == SmallMode::Staged);
  r = small_call_route(ak, s, 3, false, true, 1000, stage);
  CHECK(r.flags == (LV_OUT_ZEROED | LV_ALL_CACHED | LV_AUTO) && r.mode == SmallMode::ZeroCopyCached);
  r = small_call_route(ak, s, 1025, false, true, 200000, stage);   // the auto cache serves latency launches only
  CHECK(r.flags == LV_OUT_ZEROED && r.mode == SmallMode::Staged);
  r = small_call_route(none, s, 10, false, false, 2000, stage);
  CHECK(r.flags == LV_OUT_ZEROED && r.mode == SmallMode::ZeroCopyCold);
  r = small_call_route(none, s, 1025, false, false, 200000, stage);
  CHECK(r.mode == SmallMode::Staged);
  r = small_call_route(none, s, 10, false, false, stage - 5, stage);   // no room for the verdict bytes
  CHECK(r.mode == SmallMode::Staged);
  DeviceView warm = none;
  warm.cold = false;
  CHECK(small_call_route(warm, s, 10, false, false, 2000, stage).mode == SmallMode::Staged);
  DeviceView half = cm;
  half.path = VPath::Half;
  r = small_call_route(half, s, 67, true, false, 10000, stage);
  CHECK(r.flags == (LV_OUT_ZEROED | LV_ALL_CACHED) && r.mode == SmallMode::Staged);
  DeviceView nocomb = cm;
  nocomb.cm_comb = false;
  CHECK(small_call_route(nocomb, s, 67, true, false, 10000, stage).mode == SmallMode::Staged);
  const Settings staged = parse({{"NWC_ZERO_COPY", "0"}});
  CHECK(small_call_route(cm, staged, 67, true, false, 10000, stage).mode == SmallMode::Staged);
  CHECK(small_call_route(none, staged, 10, false, false, 2000, stage).mode == SmallMode::Staged);
}

void test_poll_written() {
  std::vector<uint8_t> bytes(300, 0);
  std::thread writer([&] {
    std::this_thread::sleep_for(std::chrono::milliseconds(2));
    for (size_t i = 0; i < bytes.size(); ++i) {
      __atomic_store_n(&bytes[i], (uint8_t)(0x80 | (i & 1)), __ATOMIC_RELEASE);
    }
  });
  CHECK(poll_written(bytes.data(), bytes.size(), std::chrono::seconds(10)));
  writer.join();
  CHECK(poll_written(bytes.data(), bytes.size(), std::chrono::microseconds(0)));
  CHECK(poll_written(bytes.data(), 0, std::chrono::microseconds(0)));
  bytes[299] = 1;   // never written
  const auto t0 = std::chrono::steady_clock::now();
  CHECK(!poll_written(bytes.data(), bytes.size(), std::chrono::milliseconds(5)));
  const auto dt = std::chrono::steady_clock::now() - t0;
  CHECK(dt >= std::chrono::milliseconds(5) && dt < std::chrono::seconds(2));
  CHECK(poll_written(bytes.data(), 299, std::chrono::milliseconds(5)));
}

}  // namespace

int main() {
  test_settings();
  std::printf("settings\n");
  test_chunk_cuts();
  std::printf("chunk_cuts\n");
  test_route_table();
  std::printf("route table\n");
  test_route_invariants();
  std::printf("route invariants\n");
  test_small_call_route();
  std::printf("small_call_route\n");
  test_poll_written();
  std::printf("poll_written\n");
  if (g_failures) {
    std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)g_failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
