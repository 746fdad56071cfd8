// The host verify path's decisions, with no HIP in them: the environment switches (Settings), the
// chunk cuts of the host pipelines (chunk_cuts), which kernels one launch_verify launch enqueues
// (route_verify), how a small host call travels (small_call_route) and the poll of the "written"
// bytes of a zero-copy launch (poll_written).  nwc_api.hip, signer.h and verifier.h read these and
// enqueue; tests/cpp/verify_plan_host.cpp runs them on the CPU under the host sanitizers.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

// Compile-time defaults of the switches below (each also an environment variable of the same name).
#ifndef NWC_VERIFY_MAX_LAUNCH
#define NWC_VERIFY_MAX_LAUNCH (16ull << 20)
#endif
// largest launch the cold kernel takes (one 4-wave block per equation); above it the one-lane
// ladder's throughput wins (tools/cold_sizes.py)
#ifndef NWC_COLD_MAX
#define NWC_COLD_MAX 3072
#endif
// Host calls of at least 2 chunks are pipelined: chunk i+1's inputs cross PCIe while chunk i
// verifies.  A chunk is one full round of resident lanes (2 blocks of 256 per CU x 256 CUs).
#ifndef NWC_HOST_CHUNK
#define NWC_HOST_CHUNK (1u << 17)
#endif
#ifndef NWC_HOST_CHUNK_MAX
#define NWC_HOST_CHUNK_MAX (1u << 20)
#endif
#ifndef NWC_HOST_CHUNK_GROWTH
#define NWC_HOST_CHUNK_GROWTH 3
#endif
#ifndef NWC_MSG_CHUNK
#define NWC_MSG_CHUNK (24u << 20)   // largest pipelined chunk of nwc_sanitize_messages, bytes of wire messages (A/B: profiles/r05/wire_host.md)
#endif
// batches up to this size take the latency kernel (k_verify_comb_wide) on the comb path
#ifndef NWC_WIDE_MAX
#define NWC_WIDE_MAX 1024
#endif
#ifndef NWC_VERIFIER_GROUP_EQ
#define NWC_VERIFIER_GROUP_EQ 4096
#endif

namespace nwc {
namespace plan {

// Verification path (NWC_VERIFY_PATH): default = the doubling-free comb kernel for equations whose
// key is in the committee cache (when the committee has combs) and half-size equations with
// full-length fallback for the rest; "half" = no comb kernel; "full" = the full-length ladder for
// every lane.  The alternatives exist to cross-check the paths against each other.
enum class VPath { Default, Half, Full };

// Every environment variable the host verify, sign and verifier paths read once per process, with
// its own default, clamp, rounding and notion of "off" (README "Switches").
struct Settings {
  uint32_t auto_keys = 256;           // NWC_AUTO_KEYS: capacity of the per-device auto key cache, 0 = off
  bool comb16 = true;                 // NWC_COMB16=0: no radix-2^22 basepoint comb (saves 3.2 GB of HBM per device)
  VPath verify_path = VPath::Default;
  uint64_t verify_max_launch = NWC_VERIFY_MAX_LAUNCH;   // equations per launch: a multiple of 64, >= 65,536
  uint64_t verify_keep_bytes = 256ull << 20;            // per-launch buffers above this are shrunk or freed when idle
  bool cold = true;                   // NWC_COLD=0 (or no comb16, its s B is a comb16 sum): no k_verify_cold
  uint64_t cold_max = NWC_COLD_MAX;
  bool host_timing = false;           // NWC_HOST_TIMING set: per-phase times of large host calls on stderr
  unsigned host_staging_threads = 8;
  uint32_t force_fallback_every = 0;  // test hook: every k-th equation of the half-size kernels takes the fallback
  bool sign_defer = true;             // NWC_SIGN_DEFER=0: the comb path decides the sign in k_verify_comb everywhere
  bool strict_y = true;               // NWC_STRICT_Y=0: the message pipeline's strict equations through launch_verify
  int digest_sched = -1;              // NWC_DIGEST_SCHED=0/1 forces the one-lane / scheduled digest kernel
  bool zero_copy = true;
  bool spin_wait = true;              // NWC_SPIN_WAIT=0: zero-copy calls wait for the stream
  bool host_pair = true;
  uint64_t host_pair_first = 65536, host_pair_growth = 2, host_pair_max = 1ull << 20;
  uint64_t host_chunk = NWC_HOST_CHUNK;   // 0 = no pipelining
  uint64_t host_chunk_growth = NWC_HOST_CHUNK_GROWTH;
  // a multiple of 64 like host_pair_max: every chunk's launch writes whole verdict words
  uint64_t host_chunk_max = NWC_HOST_CHUNK_MAX;
  uint64_t msg_chunk = NWC_MSG_CHUNK;     // 0 = one copy, then one pass
  uint64_t sign_wide_max = 256;
  uint32_t verifier_group_eq = NWC_VERIFIER_GROUP_EQ;
  // nwc_sanitizer_create: wire bytes (4 KiB to 64 MiB, a multiple of 256) and messages (1 to 65,536)
  // one group holds
  uint64_t sanitizer_group_bytes = 1u << 20;
  uint32_t sanitizer_group_msgs = 256;
  // initial values of the run-time knobs (nwc_diag_set)
  uint32_t launch_keys = 1, straus_nq = 12, force_windows = 0, msm_group = 0, msm_adapt = 1;

  // lookup: const char* (const char* name), nullptr = unset
  template <class Lookup>
  static Settings parse(Lookup&& lookup) {
    Settings s;
    auto off = [&](const char* name) {   // only the literal "0" switches off
      const char* e = lookup(name);
      return e && std::strcmp(e, "0") == 0;
    };
    auto u64 = [&](const char* name, uint64_t dflt) {
      const char* e = lookup(name);
      return e ? (uint64_t)std::strtoull(e, nullptr, 10) : dflt;
    };
    auto u32 = [&](const char* name, uint32_t dflt) {
      const char* e = lookup(name);
      return e ? (uint32_t)std::strtoul(e, nullptr, 10) : dflt;
    };
    auto words64 = [](uint64_t v) { return std::max<uint64_t>(64, v / 64 * 64); };
    s.auto_keys = u32("NWC_AUTO_KEYS", s.auto_keys);
    s.comb16 = !off("NWC_COMB16");
    if (const char* e = lookup("NWC_VERIFY_PATH")) {
      if (std::strcmp(e, "full") == 0) s.verify_path = VPath::Full;
      if (std::strcmp(e, "half") == 0) s.verify_path = VPath::Half;
    }
    s.verify_max_launch = std::max<uint64_t>(1u << 16, u64("NWC_VERIFY_MAX_LAUNCH", s.verify_max_launch) / 64 * 64);
    s.verify_keep_bytes = u64("NWC_VERIFY_KEEP_BYTES", s.verify_keep_bytes);
    s.cold = !off("NWC_COLD") && s.comb16;
    s.cold_max = u64("NWC_COLD_MAX", s.cold_max);
    s.host_timing = lookup("NWC_HOST_TIMING") != nullptr;
    if (const char* e = lookup("NWC_HOST_STAGING_THREADS")) s.host_staging_threads = (unsigned)std::max(1, std::atoi(e));
    s.force_fallback_every = u32("NWC_FORCE_FALLBACK_EVERY", 0);
    s.sign_defer = !off("NWC_SIGN_DEFER");
    s.strict_y = !off("NWC_STRICT_Y");
    if (const char* e = lookup("NWC_DIGEST_SCHED")) s.digest_sched = std::atoi(e);
    s.zero_copy = !off("NWC_ZERO_COPY");
    s.spin_wait = !off("NWC_SPIN_WAIT");
    s.host_pair = !off("NWC_HOST_PAIR");
    s.host_pair_first = words64(u64("NWC_HOST_PAIR_FIRST", s.host_pair_first));
    s.host_pair_growth = std::max<uint64_t>(1, u64("NWC_HOST_PAIR_GROWTH", s.host_pair_growth));
    s.host_pair_max = words64(u64("NWC_HOST_PAIR_MAX", s.host_pair_max));
    if (const char* e = lookup("NWC_HOST_CHUNK")) s.host_chunk = (uint64_t)std::strtoull(e, nullptr, 10) / 64 * 64;
    s.host_chunk_growth = std::max<uint64_t>(1, u64("NWC_HOST_CHUNK_GROWTH", s.host_chunk_growth));
    s.host_chunk_max = words64(u64("NWC_HOST_CHUNK_MAX", s.host_chunk_max));
    s.msg_chunk = u64("NWC_MSG_CHUNK", s.msg_chunk);
    s.sign_wide_max = u64("NWC_SIGN_WIDE_MAX", s.sign_wide_max);
    if (const char* e = lookup("NWC_VERIFIER_GROUP_EQ"))
      s.verifier_group_eq = (uint32_t)std::min<unsigned long>(std::max<unsigned long>(std::strtoul(e, nullptr, 10), 1), 1ul << 16);
    s.sanitizer_group_bytes =
        std::min<uint64_t>(std::max<uint64_t>(u64("NWC_SANITIZER_GROUP_BYTES", s.sanitizer_group_bytes), 4096), 64u << 20) / 256 * 256;
    s.sanitizer_group_msgs = std::min<uint32_t>(std::max<uint32_t>(u32("NWC_SANITIZER_GROUP_MSGS", s.sanitizer_group_msgs), 1), 1u << 16);
    s.launch_keys = u32("NWC_LAUNCH_KEYS", s.launch_keys);
    s.straus_nq = u32("NWC_STRAUS_NQ", s.straus_nq);
    s.force_windows = u32("NWC_FORCE_WINDOWS", s.force_windows);
    s.msm_group = u32("NWC_MSM_GROUP", s.msm_group);
    if (const char* e = lookup("NWC_MSM_ADAPT")) s.msm_adapt = std::atoi(e) != 0;
    return s;
  }
};

// The process's settings, parsed from the environment by the first caller.
inline const Settings& settings() {
  static const Settings s = Settings::parse([](const char* name) -> const char* { return std::getenv(name); });
  return s;
}

// Chunks of a pipelined host call over n equations: [cuts[k], cuts[k + 1]).  The first is `first`
// long, each further one `growth` times the previous up to max(first, max), and a remainder below
// first / 2 joins the last chunk (no sliver of a last chunk).  first and max are multiples of 64
// (Settings), so every chunk but the last starts and ends on a verdict word.
inline std::vector<uint64_t> chunk_cuts(uint64_t n, uint64_t first, uint64_t growth, uint64_t max) {
  std::vector<uint64_t> cuts{0};
  for (uint64_t len = first; cuts.back() < n; len = std::min(len * growth, std::max(first, max))) {
    uint64_t next = std::min<uint64_t>(n, cuts.back() + len);
    if (n - next < first / 2) next = n;
    cuts.push_back(next);
  }
  return cuts;
}
inline uint64_t longest_chunk(const std::vector<uint64_t>& cuts) {
  uint64_t m = 0;
  for (size_t k = 0; k + 1 < cuts.size(); ++k) m = std::max(m, cuts[k + 1] - cuts[k]);
  return m;
}

// launch_verify flags: the caller checked on the host that every key is in the committee cache,
// and/or out_words is already zero (both let the latency path run as a single kernel)
// LV_AUTO: the keys are in the auto cache; LV_STAMP: the headline kernel's clock-stamp build
// (k_verify<.., STAMP>, nwc_diag_verify_clock)
// LV_DEFER_LIST: a launch on the committee-cache comb path (deferrable_list()) that only appends
// its uncached equations, as list_base + i, to the call-wide list; the caller zeroed the list's
// count and sized the lists (ensure_scratch) for the whole call before the first such launch, and
// runs the list, fallback and torsion passes once over all of them (finish_deferred_list).  The
// chunked sanitize pipeline: one set of those small launches per call instead of per chunk.
constexpr int LV_ALL_CACHED = 1, LV_OUT_ZEROED = 2, LV_AUTO = 4, LV_STAMP = 8, LV_DEFER_LIST = 16;

constexpr uint64_t WIDE_MAX = NWC_WIDE_MAX;
constexpr uint64_t LK_MIN_EQUATIONS = 65536;   // launch_keys.h (nwc_api.hip asserts they agree)

// What launch_verify reads of its device context, the settings and the knobs.
struct DeviceView {
  VPath path = VPath::Default;
  uint32_t cm_n = 0;         // keys in the committee cache
  bool cm_comb = false;      // ... with per-key combs
  bool comb16 = false;       // the basepoint comb exists
  uint32_t ak_n = 0;         // keys in the auto cache
  bool ak_comb = false;
  bool launch_keys = true;   // the run-time knob
  bool cold = true;
  uint64_t cold_max = NWC_COLD_MAX;
  uint64_t fb_cap = 0;       // capacity of the per-launch lists
  uint64_t verify_max_launch = NWC_VERIFY_MAX_LAUNCH;
};

struct Request {
  uint64_t n = 0;
  bool strict = false;
  int flags = 0;
  uint64_t list_base = 0;
  bool vbytes = false;      // verdict bytes in host memory (zero-copy)
  bool pair = false;        // a PairLaunch
  bool sign_recs = false;   // SignRecs: the sign test deferred
  bool sign_pass = false;   // ... and a previous launch's sign pass to run in front (SignPass with n > 0)
};

// One value per kernel (or template instantiation) launch_verify launches as its main kernel.
enum class Kernel {
  AutoWide,        // k_verify_comb_wide over the auto cache, alone (latency)
  ZeroCopyCold,    // k_verify_cold, verdict bytes straight to the host
  CommitteeWide,   // k_verify_comb_wide over the committee cache, alone (latency)
  CombYSign,       // k_verify_comb_y_sign
  CombY,           // k_verify_comb_y
  CombWide,        // k_verify_comb_wide with the uncached list
  Comb,            // k_verify_comb
  Cold,            // k_verify_cold, staged
  HalfCached,      // k_verify<true, true>
  HalfStamp,       // k_verify<true, false, false, true>
  Half,            // k_verify<true, false>
  Full,            // k_verify<false, false>
};
// the keys' torsion test of a batch-leaf launch: beside the verification on the side stream, or
// after it over all equations or over the comb path's uncached list
enum class Torsion { None, Beside, AfterAll, AfterList };

struct Route {
  // an argument error (NWC_ERR_ARG) with this message.  With `scratch` set it is returned only after
  // the scratch and the launch keys (comb, lk_build) are ensured, as ever; the rest is unset.
  const char* error = nullptr;
  Kernel kernel = Kernel::Half;
  bool comb = false;             // the comb path (launch keys or the committee cache)
  bool lk_build = false;         // the launch-key build runs in front
  bool list_pass = false;        // k_verify<true, false, true> over the uncached list follows
  bool fallback = false;         // k_verify_fallback follows
  Torsion torsion = Torsion::None;
  uint64_t zero_words = 0;       // verdict words zeroed first (0 = none)
  bool zero_fb_count = false;    // the fallback count zeroed first
  bool scratch = false;          // uses the table slots and lists (ensure_scratch)
  bool scratch_order = false;    // waits for scratch_free first and records it last
};

struct CombPath { bool lk, comb; };
// Whether a launch of n equations takes the comb path: with launch keys of its own (lk: a large
// batch-leaf launch without a committee cache brings its own committee, launch_keys.h) or over
// the committee cache (the throughput comb kernel needs the basepoint comb16; the latency kernel
// does not).
inline CombPath comb_path(const DeviceView& v, uint64_t n, bool strict, int flags = 0) {
  if (v.path != VPath::Default) return {false, false};
  const bool lk = !strict && !v.cm_n && v.comb16 && n >= LK_MIN_EQUATIONS && v.launch_keys && !(flags & LV_AUTO);
  return {lk, lk || (v.cm_n && v.cm_comb && (n <= WIDE_MAX || v.comb16))};
}
// launch_verify's comb path over the committee cache for any n (what LV_DEFER_LIST needs)
inline bool deferrable_list(const DeviceView& v) { return v.path == VPath::Default && v.cm_n && v.cm_comb && v.comb16; }
// launch_verify runs a request of more than verify_max_launch equations as consecutive launches
inline bool splits(const DeviceView& v, const Request& q) { return q.n > v.verify_max_launch && !q.vbytes; }

// Whether launch_verify returns r's error at once; otherwise the route goes to the single-kernel
// launches or, with `scratch`, to the listed ones, which return a late error once the scratch stands.
inline bool early_error(const Route& r) { return r.error && !r.scratch; }

// What one launch (q.n <= verify_max_launch, or verdict bytes) enqueues.
inline Route route_verify(const DeviceView& v, const Request& q) {
  Route r;
  const uint64_t n = q.n, words = (n + 63) / 64;
  auto fail = [&](const char* msg, bool late = false) {
    Route e;
    e.error = msg;
    e.scratch = late;
    e.lk_build = late && r.lk_build;
    e.comb = late && r.comb;
    return e;
  };
  // equation indices travel as uint32 (fallback / uncached / torsion lists)
  if (n > 0xFFFFFFFFull) return fail("more than 2^32 - 1 equations in one launch");
  const bool all_cached = (q.flags & LV_ALL_CACHED) != 0;
  const uint64_t latency_zero = !q.vbytes && !(q.flags & LV_OUT_ZEROED) ? words + 1 : 0;
  if ((q.flags & LV_AUTO) && all_cached && v.path == VPath::Default && n <= WIDE_MAX && v.ak_n) {
    // latency path over the auto key cache (same kernel, the auto cache as its committee)
    r.kernel = Kernel::AutoWide;
    r.zero_words = latency_zero;
    return r;
  }
  if (q.vbytes && !all_cached) {
    // zero-copy cold launch (the caller checked: no committee cache, n <= NWC_WIDE_MAX, default
    // path, cold kernel on): no scratch, no fallback launch, verdict bytes straight to the host
    r.kernel = Kernel::ZeroCopyCold;
    return r;
  }
  const CombPath cp = comb_path(v, n, q.strict, q.flags);
  const bool lk = cp.lk, comb = cp.comb;
  const bool defer = (q.flags & LV_DEFER_LIST) != 0;
  if (defer && (lk || !comb || q.list_base + n > v.fb_cap || !deferrable_list(v)))
    return fail("deferred list launch off the committee-cache comb path");
  if (q.sign_recs && (!comb || (defer && (q.list_base & 63))))
    return fail("sign-deferred launch off the comb path or off a verdict word");
  if (comb && n <= WIDE_MAX && all_cached) {
    // latency path, one launch: no scratch, no uncached list, no fallback (the comb path has none).
    // The host checked every key against its view of the cache; should a key still be missing on
    // the device, the kernel sets the word after the verdict words instead of listing it, and the
    // caller re-runs the general path.
    r.kernel = Kernel::CommitteeWide;
    r.comb = true;
    r.zero_words = latency_zero;
    return r;
  }
  r.comb = comb;
  r.lk_build = lk;
  r.scratch = true;
  r.scratch_order = !q.pair;
  if (q.pair && (!q.strict || comb || v.path == VPath::Full || v.cm_n))
    return fail("paired launch off the strict half-size path", true);
  const Kernel comb_y = q.sign_pass ? Kernel::CombYSign : Kernel::CombY;
  if (defer) {
    // only the comb kernel, listing its uncached equations; the sign of x(R') later in k_comb_sign
    // over many votes when the caller passed SignRecs
    r.kernel = q.sign_recs ? comb_y : n <= WIDE_MAX ? Kernel::CombWide : Kernel::Comb;
    r.zero_words = !q.sign_recs && n <= WIDE_MAX ? words : 0;
    return r;
  }
  const bool half = v.path != VPath::Full;
  // a small batch no cache covers (first-sight keys): one limb-sliced block per equation, the
  // batch leaf's torsion test inside it
  const bool cold = half && !comb && !v.cm_n && n <= v.cold_max && v.cold && !q.pair;
  r.zero_fb_count = half;
  r.fallback = half && !q.pair;   // a paired launch's fallback passes run once its pipeline has joined
  if (comb) {
    // sign test deferred (the chunked host path): the words zeroed for the list passes and the
    // later sign pass to OR into; small batches: one block per equation, zeroed likewise
    r.kernel = q.sign_recs ? comb_y : n <= WIDE_MAX ? Kernel::CombWide : Kernel::Comb;
    r.zero_words = q.sign_recs || n <= WIDE_MAX ? words : 0;
    r.list_pass = true;
  } else if (cold) {
    r.kernel = Kernel::Cold;
    r.zero_words = q.flags & LV_OUT_ZEROED ? 0 : words;
  } else if (!half) {
    r.kernel = Kernel::Full;
  } else {
    r.kernel = v.cm_n ? Kernel::HalfCached : (q.flags & LV_STAMP) ? Kernel::HalfStamp : Kernel::Half;
  }
  // batch leaves: keys with torsion (cached keys were checked in the comb kernels; the comb path's
  // other equations are its uncached list).  Small launches outside the comb path: the test (one
  // long serial lane per new key) runs on the side stream beside the verification.
  if (!q.strict && !cold)
    r.torsion = comb ? Torsion::AfterList : n <= WIDE_MAX ? Torsion::Beside : Torsion::AfterAll;
  return r;
}

// How a small host call (its staged inputs fit the pinned stage) travels.
enum class SmallMode { ZeroCopyCached, ZeroCopyCold, Staged };
struct SmallRoute {
  int flags;   // LV_* of its launch
  SmallMode mode;
};
// cm_all_cached / ak_all_found: every key of the call is in the host's view of the committee cache
// / the auto cache (the caller looks only where the view can use the answer).  stage_bytes: the
// staged inputs and verdict words, after which a zero-copy launch's n verdict bytes go (256-byte
// aligned); stage_max: the pinned stage's size.
inline SmallRoute small_call_route(const DeviceView& v, const Settings& s, uint64_t n, bool cm_all_cached, bool ak_all_found,
                                   uint64_t stage_bytes, uint64_t stage_max) {
  int fl = LV_OUT_ZEROED;
  if (v.cm_n && cm_all_cached) fl |= LV_ALL_CACHED;
  else if (v.ak_n && n <= WIDE_MAX && ak_all_found) fl |= LV_ALL_CACHED | LV_AUTO;
  const uint64_t vb_off = (stage_bytes + 255) & ~(uint64_t)255;
  const bool zc_ok = s.zero_copy && n <= WIDE_MAX && vb_off + n <= stage_max && v.path == VPath::Default;
  const bool cached = (fl & LV_ALL_CACHED) != 0;
  if (zc_ok && cached && (fl & LV_AUTO ? v.ak_comb : v.cm_comb)) return {fl, SmallMode::ZeroCopyCached};
  if (zc_ok && !cached && !v.cm_n && v.cold) return {fl, SmallMode::ZeroCopyCold};
  return {fl, SmallMode::Staged};
}

// Polls the "written" bytes (bit 7) a zero-copy launch stores to host memory: whether all n were
// written within `limit`.  A launch that never writes them (a device error) is the caller's to
// report after its stream wait.
inline bool poll_written(const volatile uint8_t* vb, uint64_t n, std::chrono::microseconds limit) {
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t done = 0;
  for (;;) {
    while (done < n && (vb[done] & 0x80u)) ++done;
    if (done == n) break;
    if (std::chrono::steady_clock::now() - t0 > limit) return false;
    __builtin_ia32_pause();
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return true;
}

}  // namespace plan
}  // namespace nwc
