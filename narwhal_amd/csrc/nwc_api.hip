// Host side of libnwc.so: the C ABI declared in include/nwc.h.
//
// One context per HIP device: its own stream, the basepoint table, and a growable staging
// arena.  A per-device mutex makes every entry point thread-safe (the reference calls the
// crypto crate from concurrent tokio tasks: primary/src/core.rs:88-114,
// worker/src/worker.rs:182,227).  Host batch entry points shard independent units
// (signatures, certificates, messages) over all initialised devices with one host thread per
// device; nothing here ever falls back to a CPU path -- a device failure is
// an error code (< 0), never a verdict.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "nwc.h"
#include "copy_pool.h"
#include "dev_buf.h"
#include "kernels.hip"
#include "launch_keys.h"
#include "messages.h"
#include "msg_plan.h"
#include "verify_plan.h"

namespace {

using nwc::plan::settings;
using nwc::plan::VPath;
using nwc::plan::LV_ALL_CACHED;
using nwc::plan::LV_OUT_ZEROED;
using nwc::plan::LV_AUTO;
using nwc::plan::LV_STAMP;
using nwc::plan::LV_DEFER_LIST;
static_assert(nwc::plan::LK_MIN_EQUATIONS == nwc::LK_MIN_EQUATIONS, "verify_plan.h routes by launch_keys.h's threshold");

thread_local std::string t_err;
thread_local int t_dev = 0;
thread_local int t_code = 0;   // code of the calling thread's last error (nwc_last_error_code)

int set_err(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  t_err = buf;
  t_code = code;
  return code;
}

#define HIP_TRY(expr)                                                                           \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return set_err(NWC_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),     \
                     __FILE__, __LINE__);                                                       \
  } while (0)

// Exact 32-byte key lookup with the device's hash and probing (committee_lookup): the host copy
// of a device key cache, so that small host calls can tell before launching whether every key
// is cached.
struct KeyIndex {
  std::vector<nwc::u32> keys;   // 8 words per key
  std::vector<int32_t> slots;   // slot -> key index, -1 empty
  uint32_t mask = 0;
  bool find(const uint8_t* pk) const {
    if (slots.empty()) return false;
    nwc::u32 w[8];
    std::memcpy(w, pk, 32);
    const nwc::u32 h = nwc::committee_hash(w[0], w[1]);
    for (int p = 0; p < nwc::COMMITTEE_MAX_PROBE; ++p) {
      const int32_t idx = slots[(h + p) & mask];
      if (idx < 0) return false;
      if (std::memcmp(&keys[8 * (size_t)idx], w, 32) == 0) return true;
    }
    return false;
  }
  bool all_found(const uint8_t* pks, uint64_t n) const {
    for (uint64_t i = 0; i < n; ++i)
      if (!find(pks + 32 * i)) return false;
    return true;
  }
};

// Open-addressing slot table over the first n keys (load factor <= 1/4, probe length bounded by
// COMMITTEE_MAX_PROBE; a duplicate key keeps its first index).
uint32_t build_slots(const std::vector<nwc::u32>& keys, size_t n, std::vector<int32_t>& table) {
  uint32_t slots = 16;
  while (slots < 4 * n) slots <<= 1;
  for (;;) {
    table.assign(slots, -1);
    bool fits = true;
    for (size_t i = 0; i < n && fits; ++i) {
      const nwc::u32 h = nwc::committee_hash(keys[8 * i], keys[8 * i + 1]);
      int p = 0;
      for (; p < nwc::COMMITTEE_MAX_PROBE; ++p) {
        int32_t& slot = table[(h + p) & (slots - 1)];
        if (slot < 0) { slot = (int32_t)i; break; }
        if (std::memcmp(&keys[8 * slot], &keys[8 * i], 32) == 0) break;   // duplicate key
      }
      fits = p < nwc::COMMITTEE_MAX_PROBE;
    }
    if (fits) return slots;
    slots <<= 1;
  }
}

// The runtime's allocation calls, for dev_buf.h: the only place in this file that frees.
struct HipAlloc {
  using Error = hipError_t;
  using Stream = hipStream_t;
  static constexpr Error ok = hipSuccess;
  static Error alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static Error alloc_async(void** p, size_t bytes, Stream s) { return hipMallocAsync(p, bytes, s); }
  static Error alloc_pinned(void** host, void** dev, size_t bytes) {
    // coherent: a kernel's stores reach the host while it polls them
    if (Error e = hipHostMalloc(host, bytes, hipHostMallocCoherent)) return e;
    const Error e = hipHostGetDevicePointer(dev, *host, 0);
    if (e != hipSuccess) (void)hipHostFree(*host);
    return e;
  }
  static Error free(void* p) { return hipFree(p); }
  static Error free_async(void* p, Stream s) { return hipFreeAsync(p, s); }
  static Error free_pinned(void* p) { return hipHostFree(p); }
};
template <class T> using Buf = nwc::buf::Buf<T, HipAlloc>;
using RawBuf = nwc::buf::RawBuf<HipAlloc>;
using nwc::buf::Account;
using nwc::buf::Keep;
using nwc::buf::Trimmable;
// Plain release of each buffer; the first error, after all of them are empty.
hipError_t release_each(std::initializer_list<RawBuf*> bufs) {
  hipError_t first = hipSuccess;
  for (RawBuf* b : bufs)
    if (hipError_t e = b->release(); first == hipSuccess) first = e;
  return first;
}

// Every device and pinned buffer is a Buf registered with `bufs` (dev_buf.h) under the account
// nwc_memory_info reports it in, Trimmable if nwc_trim drops it.
struct DevCtx {
  int hip_id = 0;
  int cus = 0;
  int verify_blocks_per_cu = 1;
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;      // small batch-leaf calls: the keys' torsion test beside the verification
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_msg = nullptr;   // sanitize: k_header_digests done on the side stream
  hipEvent_t ev_count = nullptr; // sanitize: the vote count has reached the host
  // large host calls: input chunks are copied on `xfer` while the previous chunk verifies on
  // `stream` (one event per chunk in flight, created on first use)
  hipStream_t xfer = nullptr;
  std::vector<hipEvent_t> ev_chunk;
  std::vector<hipEvent_t> ev_cnt;      // sanitize: chunk k's vote count copied to the host
  nwc::buf::BufSet<HipAlloc> bufs;     // owns every Buf below
  Buf<nwc::ge_niels> base_table{bufs, Account::Tables, Keep};
  Buf<nwc::ge_niels> sign_table{bufs, Account::Tables, Keep};   // the signers' basepoint table (60 KB, sign.h), built by the first signer
  Buf<nwc::ge_niels_pad> base24{bufs, Account::Tables, Keep};   // radix-2^24 basepoint tables (2.1 GB)
  Buf<nwc::ge_p3> base24_points{bufs, Account::Tables, Keep};   // B and 2^141 B
  Buf<nwc::ge_niels_pad> comb_base{bufs, Account::Tables, Keep};   // radix-256 basepoint comb (528 KB): latency kernel
  Buf<nwc::ge_niels_pad> comb16{bufs, Account::Tables, Keep};      // basepoint comb (radix 2^NWC_BCOMB_BITS, 67 MB at 2^16): k_verify_comb
  Buf<nwc::ge_p3> comb16_bases{bufs, Account::Tables, Keep};       // its window bases 2^(bits w) B (built at init)
  Buf<nwc::ge_p3> kb_bases{bufs, Account::AutoCache, Keep};        // key comb window bases (scratch of build_key_combs)
  size_t kb_cap = 0;
  int comb_blocks_per_cu = 1;
  Buf<uint8_t> straus_scratch{bufs, Account::Scratch, Trimmable};   // k_verify_straus per-lane tables (nwc_dev_verify_batch_straus)
  Buf<uint8_t> msm_scratch{bufs, Account::Scratch, Trimmable};      // k_verify_msm per-wave points and digits (nwc_dev_verify_batch_msm)
  Buf<uint32_t> msm_stats{bufs, Account::Uncounted, Keep};          // groups passed / failed / key overflow (nwc_msm_stats)
  Buf<uint8_t> rs_buf{bufs, Account::Scratch, Trimmable};           // dalek's equation per certificate (resolve.h): failing-vote list, certificate states
  Buf<uint32_t> uc_list{bufs, Account::Scratch, Trimmable};     // k_verify_comb: equations whose key is not cached
  Buf<uint32_t> uc_count{bufs, Account::Uncounted, Keep};
  bool hold_lists = false;         // a call with a deferred list pending: ensure_scratch does not shrink the lists
  bool tables_ready = false;       // ensure_verify_tables has built the basepoint tables, memo and auto cache
  // k_verify per-lane table slots; reused by every launch, so launches that use it are
  // serialised across streams with `scratch_free` (recorded after each such launch).
  Buf<uint8_t> scratch{bufs, Account::Scratch, Trimmable};
  Buf<uint32_t> fb_list{bufs, Account::Scratch, Trimmable};     // lanes whose half-size reduction failed (k_verify_fallback)
  Buf<uint32_t> fb_count{bufs, Account::Uncounted, Keep};
  Buf<uint8_t> pair_buf{bufs, Account::Scratch, Trimmable};     // the paired strict host pipeline: per-chunk fallback counts + lists
  Buf<uint8_t> sign_buf{bufs, Account::Scratch, Trimmable};     // large host calls on the comb path: two chunks' SignRecs
  const uint8_t* busy_buf = nullptr;   // a buffer a host pipeline's launches use: never released under it
  Buf<uint64_t> stamps{bufs, Account::Uncounted, Keep};   // k_verify<.., STAMP>: 4 words per wave of the resident grid (nwc_diag_verify_clock)
  size_t fb_cap = 0;               // entries of fb_list, uc_list and ts_uniq
  hipEvent_t scratch_free = nullptr;
  // batch-leaf torsion post-pass (k_tors_*): key hash set sized for fb_cap equations
  Buf<int32_t> ts_slots{bufs, Account::Scratch, Trimmable};
  Buf<uint32_t> ts_flag{bufs, Account::Scratch, Trimmable};
  Buf<uint32_t> ts_uniq{bufs, Account::Scratch, Trimmable};
  Buf<uint32_t> ts_nuniq{bufs, Account::Uncounted, Keep};
  uint32_t ts_slot_count = 0;
  Buf<nwc::u32> km_keys{bufs, Account::Tables, Keep};   // torsion memo of uncached keys (KeyMemo), kept for the context's life
  Buf<nwc::u32> km_flag{bufs, Account::Tables, Keep};
  // committee key cache (nwc_set_committee); buffers replaced only after scratch_free
  Buf<nwc::u32> cm_keys{bufs, Account::Committee, Keep};
  Buf<nwc::u32> cm_flags{bufs, Account::Committee, Keep};
  Buf<nwc::ge_niels> cm_tables{bufs, Account::Committee, Keep};
  Buf<nwc::ge_niels_pad> cm_comb{bufs, Account::Committee, Keep};   // per-key combs (committees of <= COMB_MAX_KEYS keys)
  Buf<int32_t> cm_slots{bufs, Account::Committee, Keep};
  uint32_t cm_n = 0, cm_slot_mask = 0;
  Buf<uint8_t> arena{bufs, Account::Scratch, Trimmable};
  // config::Committee stake / worker tables (nwc_set_committee_config)
  Buf<uint64_t> cc_stakes{bufs, Account::Uncounted, Keep};
  Buf<uint32_t> cc_worker_off{bufs, Account::Uncounted, Keep};
  Buf<uint32_t> cc_worker_ids{bufs, Account::Uncounted, Keep};
  uint64_t cc_quorum = 0;
  uint32_t cc_n = 0;
  Buf<uint8_t> msg_arena{bufs, Account::Scratch, Trimmable};   // nwc_sanitize_messages buffers
  // host staging for small calls: one H2D and one D2H per call, or read in place by the latency
  // kernel through its device alias (dev())
  Buf<uint8_t> pinned{bufs, Account::Uncounted, Keep, nwc::buf::Kind::Pinned};
  // auto key cache (NWC_AUTO_KEYS): keys of small host calls outside the committee cache, added
  // with their flags, 129-entry tables and combs the second time they are seen, so that repeated
  // first-sight certificates take the latency kernel; append-only, guarded by mu like the rest
  Buf<nwc::u32> ak_keys{bufs, Account::AutoCache, Keep};
  Buf<nwc::u32> ak_flags{bufs, Account::AutoCache, Keep};
  Buf<nwc::ge_niels> ak_tables{bufs, Account::AutoCache, Keep};
  Buf<nwc::ge_niels_pad> ak_comb{bufs, Account::AutoCache, Keep};
  Buf<int32_t> ak_slots{bufs, Account::AutoCache, Keep};
  uint32_t ak_n = 0, ak_cap = 0, ak_slot_cap = 0;
  uint32_t ak_evict = 0;                  // next FIFO position once the cache is full
  uint64_t ak_builds = 0, ak_hits = 0;    // insert batches built / calls served from the auto cache
  KeyIndex ak_host;                       // host copy of the auto cache's lookup table
  std::unordered_set<std::string> ak_seen;   // keys seen once (32-byte strings), bounded
  // copy sources of the last auto-cache build, alive until the stream has passed it
  std::vector<nwc::u32> ak_pend_keys;
  std::vector<int32_t> ak_pend_slots;
  bool ak_pending = false;
  // launch keys (launch_keys.h): allocated by the first large batch-leaf launch without a
  // committee.  `lk` is what kernels take by value; its pointers are filled from the buffers.
  nwc::LaunchKeys lk{};
  Buf<nwc::u32> lk_keys{bufs, Account::AutoCache, Trimmable};
  Buf<nwc::u32> lk_flags{bufs, Account::AutoCache, Trimmable};
  Buf<int32_t> lk_slots{bufs, Account::AutoCache, Trimmable};
  Buf<nwc::ge_p3> lk_bases{bufs, Account::AutoCache, Trimmable};
  Buf<uint32_t> lk_state{bufs, Account::AutoCache, Trimmable};
  Buf<nwc::ge_niels_pad> lk_comb{bufs, Account::AutoCache, Trimmable};
  bool lk_alloc = false;
  bool lk_censused = false;           // the first launch-key launch has measured its keys' demand
  Buf<uint32_t> lk_demand{bufs, Account::Uncounted, Keep, nwc::buf::Kind::Pinned};   // host-mapped demand word (lk.host_demand's host side)
  // large host calls: pageable inputs through pinned stages on `xfer` (created on first use)
  std::unique_ptr<HostStager> stager;
  std::mutex mu;

  int ensure_pinned(size_t bytes) { HIP_TRY(pinned.ensure(bytes)); return 0; }
  int ensure_arena(size_t bytes) { HIP_TRY(arena.ensure(bytes, bytes / 4 + (1 << 20))); return 0; }
};

// slots of the per-device torsion memo of uncached keys (power of two)
#ifndef NWC_MEMO_SLOTS
#define NWC_MEMO_SLOTS (1u << 16)
#endif
// committees up to this size get per-key combs (20 MB each at radix 2^14); larger ones use the cached ladder
#ifndef NWC_COMB_MAX_KEYS
#define NWC_COMB_MAX_KEYS 1024
#endif

// (the switches' compile-time defaults, NWC_WIDE_MAX among them, are in verify_plan.h)
#ifndef NWC_PINNED_STAGE_MAX
#define NWC_PINNED_STAGE_MAX (1u << 20)
#endif
// persistent verify grid: this many blocks per resident block slot
#ifndef NWC_VERIFY_GRID_MULT
#define NWC_VERIFY_GRID_MULT 8
#endif

std::mutex g_mu;
std::vector<std::unique_ptr<DevCtx>> g_devs;

struct HostCommittee {
  std::mutex mu;
  KeyIndex idx;
  bool all_cached(const uint8_t* pks, uint64_t n) {
    std::lock_guard<std::mutex> lk(mu);
    return idx.all_found(pks, n);
  }
};
HostCommittee g_hcm;

using nwc::plan::align256;

struct Carve {
  uint8_t* base;
  size_t off = 0;
  explicit Carve(uint8_t* b) : base(b) {}
  template <class T> T* take(size_t bytes) { T* p = reinterpret_cast<T*>(base + off); off += align256(bytes); return p; }
};

void signers_shutdown();
void verifiers_shutdown();
void sanitizers_shutdown();
int auto_grow(DevCtx& d, uint32_t ncap);

// Test and A/B knobs settable at run time (nwc_diag_set), defaults from the environment (settings()):
// NWC_STRAUS_NQ (votes per Straus sub-batch, 12) and NWC_FORCE_WINDOWS (half-ladder window count
// forced on every wave, 0 = off).  Atomics: a setter racing a launch gives that launch either value.
struct Knobs {
  std::atomic<uint32_t> straus_nq{12};
  std::atomic<uint32_t> force_windows{0};
  std::atomic<uint32_t> launch_keys{1};   // NWC_LAUNCH_KEYS: 0 = large batch-leaf launches never build launch keys
  std::atomic<uint32_t> msm_group{0};     // NWC_MSM_GROUP: votes per Pippenger group of k_verify_msm (0 = sized per launch)
  std::atomic<uint32_t> msm_adapt{1};     // NWC_MSM_ADAPT: 0 = the equation on every group (no skip policy)
  std::atomic<uint32_t> sign_path{0};     // tests: 0 = by size (NWC_SIGN_WIDE_MAX), 1 = k_sign, 2 = k_sign_wide
  std::atomic<uint32_t> sanitizer_redo_every{0};   // tests: k_finalize_group marks message slots i % k == 0 "decide me again" (0 = off)
  std::atomic<uint64_t> dalek_seed{0};    // tests: fixed seed of the per-certificate equation's z_i (0 = host CSPRNG)
  Knobs() {
    const nwc::plan::Settings& s = settings();
    launch_keys = s.launch_keys;
    straus_nq = s.straus_nq;
    force_windows = s.force_windows;
    msm_group = s.msm_group;
    msm_adapt = s.msm_adapt;
  }
};
Knobs& knobs() {
  static Knobs k;
  return k;
}

int init_device(DevCtx& d) {
  HIP_TRY(hipSetDevice(d.hip_id));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, d.hip_id));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_err(NWC_ERR_NO_DEVICE, "device %d is %s; libnwc is built for gfx950 only", d.hip_id, prop.gcnArchName);
  HIP_TRY(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&d.scratch_free, hipEventDisableTiming));
  HIP_TRY(hipStreamCreateWithFlags(&d.side, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&d.ev_fork, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&d.ev_join, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&d.ev_msg, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&d.ev_count, hipEventDisableTiming));
  d.cus = prop.multiProcessorCount;
  int bpc = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, reinterpret_cast<const void*>(nwc::k_verify<true, false>), 256, 0));
  d.verify_blocks_per_cu = bpc > 0 ? bpc : 1;
  if (std::getenv("NWC_SHOW_OCCUPANCY")) std::fprintf(stderr, "nwc: k_verify resident blocks per CU %d\n", bpc);
  bpc = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, reinterpret_cast<const void*>(nwc::k_verify_comb), 256, 0));
  d.comb_blocks_per_cu = bpc > 0 ? bpc : 1;
  HIP_TRY(d.uc_count.alloc(sizeof(uint32_t)));
  HIP_TRY(d.fb_count.alloc(sizeof(uint32_t)));
  HIP_TRY(hipStreamSynchronize(d.stream));
  return 0;
}

// The verification tables, built by the first call that verifies (or signs) on the device, not at
// nwc_init: a worker process that only digests batches holds none of them (worker/src/worker.rs:
// 182-188 -- workers and a primary share the host's GPUs).  Built on d.stream and waited for once,
// so launches on any stream after it see them.  Caller holds d.mu and has set the device.
int build_verify_tables(DevCtx& d) {
  HIP_TRY(d.comb_base.alloc(nwc::BaseComb::per * sizeof(nwc::ge_niels_pad)));
  hipLaunchKernelGGL(nwc::k_build_comb<nwc::BaseComb>, dim3((unsigned)((nwc::BaseComb::per + 255) / 256)), dim3(256), 0, d.stream,
                     (const nwc::u32*)nullptr, 1u, d.comb_base.get());
  HIP_TRY(hipGetLastError());
  if (settings().comb16) {
    // radix-2^22 basepoint comb (3.2 GB): the committee comb kernel and the cold kernel's s B
    HIP_TRY(d.comb16.alloc(nwc::COMB16_TOTAL * sizeof(nwc::ge_niels_pad)));
    HIP_TRY(d.comb16_bases.alloc(nwc::COMB16_WINDOWS * sizeof(nwc::ge_p3)));
    hipLaunchKernelGGL(nwc::k_bcomb_bases, dim3(1), dim3(64), 0, d.stream, d.comb16_bases.get());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(nwc::k_build_comb16, dim3((unsigned)((nwc::COMB16_TOTAL + 255) / 256)), dim3(256), 0, d.stream,
                       d.comb16.get(), (const nwc::ge_p3*)d.comb16_bases);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(d.base_table.alloc(2 * 129 * sizeof(nwc::ge_niels)));
  hipLaunchKernelGGL(nwc::k_build_base_table, dim3(5), dim3(64), 0, d.stream, d.base_table.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(d.base24.alloc(2 * (size_t)nwc::B24_ENTRIES * sizeof(nwc::ge_niels_pad)));
  HIP_TRY(d.base24_points.alloc(2 * sizeof(nwc::ge_p3)));
  hipLaunchKernelGGL(nwc::k_base_pow2, dim3(1), dim3(64), 0, d.stream, d.base24_points.get());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(nwc::k_build_base_table24, dim3((unsigned)((2 * (size_t)nwc::B24_ENTRIES + 255) / 256)), dim3(256), 0,
                     d.stream, d.base24.get(), (const nwc::ge_p3*)d.base24_points);
  HIP_TRY(hipGetLastError());
  // torsion memo: 64K keys (2.3 MB), all slots empty
  HIP_TRY(d.km_keys.alloc(32 * (size_t)NWC_MEMO_SLOTS));
  HIP_TRY(d.km_flag.alloc(4 * (size_t)NWC_MEMO_SLOTS));
  HIP_TRY(hipMemsetAsync(d.km_flag, 0xFF, 4 * (size_t)NWC_MEMO_SLOTS, d.stream));
  // auto key cache: the first AUTO_INIT_KEYS keys' arrays (~330 MB), their slot table and the key
  // comb builder's scratch are allocated here, so the call that first fills the cache only
  // queues its build (growth beyond this is stream-ordered, auto_grow)
  if (const uint32_t acap = settings().auto_keys) {
    if (int rc = auto_grow(d, std::min<uint32_t>(acap, 16u))) return rc;
    d.ak_slot_cap = 64;
    while (d.ak_slot_cap < 8 * std::min<uint32_t>(acap, 16u)) d.ak_slot_cap <<= 1;
    HIP_TRY(d.ak_slots.alloc(4 * (size_t)d.ak_slot_cap));
    if (!d.kb_bases) {
      d.kb_cap = 64 * (size_t)nwc::KeyComb::windows;
      HIP_TRY(d.kb_bases.alloc(d.kb_cap * sizeof(nwc::ge_p3)));
    }
  }
  HIP_TRY(hipStreamSynchronize(d.stream));
  return 0;
}
int ensure_verify_tables(DevCtx& d) {
  if (d.tables_ready) return 0;
  const int rc = build_verify_tables(d);
  d.tables_ready = rc == 0;
  if (rc == 0) return 0;
  // A failed build holds nothing (out of memory on a GPU shared with other processes is the
  // expected failure): the builders queued on d.stream are drained, and the next verifying call
  // starts again from an empty context.
  (void)hipStreamSynchronize(d.stream);
  (void)release_each({&d.comb_base, &d.comb16, &d.comb16_bases, &d.base_table, &d.base24, &d.base24_points, &d.km_keys,
                      &d.km_flag, &d.ak_keys, &d.ak_flags, &d.ak_tables, &d.ak_comb, &d.ak_slots, &d.kb_bases});
  d.ak_cap = d.ak_slot_cap = 0;
  d.kb_cap = 0;
  return rc;
}

DevCtx* ctx(int i) {
  if (i < 0 || i >= (int)g_devs.size()) return nullptr;
  return g_devs[i].get();
}

int require_init() {
  if (g_devs.empty()) return set_err(NWC_ERR_NOT_INIT, "nwc_init has not been called (or found no device)");
  return 0;
}

// Per-key combs of m keys (KeyComb) into out: window bases first, then one lane per entry.  The
// bases are re-allocated stream-ordered when a larger build needs more.
int build_key_combs(DevCtx& d, const nwc::u32* keys, uint32_t m, nwc::ge_niels_pad* out) {
  if (m == 0) return 0;
  const size_t need = (size_t)m * nwc::KeyComb::windows;
  if (need > d.kb_cap) {
    // stream-ordered: the old bases are freed behind the launches that read them
    d.kb_cap = 0;
    HIP_TRY(d.kb_bases.release_async(d.stream));
    HIP_TRY(d.kb_bases.alloc_async(need * sizeof(nwc::ge_p3), d.stream));
    d.kb_cap = need;
  }
  hipLaunchKernelGGL(nwc::k_comb_key_bases<nwc::KeyComb>, dim3((m + 63) / 64), dim3(64), 0, d.stream, keys, m, d.kb_bases.get());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(nwc::k_build_comb_from_bases<nwc::KeyComb>, dim3((unsigned)(d.cus * 8)), dim3(256), 0, d.stream,
                     (const nwc::ge_p3*)d.kb_bases, 0u, m, (const uint32_t*)nullptr, out);
  HIP_TRY(hipGetLastError());
  return 0;
}

constexpr size_t AUTO_SEEN_MAX = 4096;   // keys remembered as seen once (cleared when full)
constexpr uint32_t AUTO_INIT_KEYS = 16;   // auto-cache capacity allocated at nwc_init (doubled on demand)

// Stream-ordered (re)allocation of the auto cache's arrays to ncap keys: the new arrays come from
// the stream's pool (hipMallocAsync), what is built is copied over, and the old arrays are freed
// behind every launch already queued -- the host never waits.  Caller holds d.mu.
int auto_grow(DevCtx& d, uint32_t ncap) {
  RawBuf* const held[4] = {&d.ak_keys, &d.ak_flags, &d.ak_tables, &d.ak_comb};
  const size_t per_key[4] = {32, 4, 129 * sizeof(nwc::ge_niels), nwc::COMB_PER_KEY * sizeof(nwc::ge_niels_pad)};
  RawBuf fresh[4];
  hipError_t e = hipSuccess;
  for (int i = 0; i < 4 && e == hipSuccess; ++i) e = fresh[i].alloc_async(per_key[i] * ncap, d.stream);
  for (int i = 0; i < 4 && e == hipSuccess && d.ak_n; ++i)
    e = hipMemcpyAsync(fresh[i].raw(), held[i]->raw(), per_key[i] * d.ak_n, hipMemcpyDeviceToDevice, d.stream);
  if (e != hipSuccess) {   // the cache keeps its arrays; the new ones go back to the pool
    for (RawBuf& b : fresh) (void)b.release_async(d.stream);
    return set_err(NWC_ERR_DEVICE, "growing the auto key cache to %u keys: %s", ncap, hipGetErrorString(e));
  }
  for (int i = 0; i < 4; ++i) {   // the old arrays are freed behind the copies
    if (hipError_t f = held[i]->release_async(d.stream); e == hipSuccess) e = f;
    (void)held[i]->adopt(std::move(fresh[i]));
  }
  d.ak_cap = ncap;
  HIP_TRY(e);
  return 0;
}

// Empties the auto cache (nwc_set_committee: a new committee makes the remembered keys stale).
// The arrays are kept for reuse.  Caller holds d.mu and has drained d.stream.
void auto_reset(DevCtx& d) {
  d.ak_n = 0;
  d.ak_evict = 0;
  d.ak_pending = false;
  d.ak_host = KeyIndex{};
  d.ak_seen.clear();
}

// Keys of a small host call that missed every cache: a key seen before is added to the auto
// cache (flags, 129-entry table and comb built on d.stream after this call's work; the next call
// on this device is ordered after the build), a new one is remembered as seen.  Once the cache
// holds NWC_AUTO_KEYS keys, new ones replace the oldest (FIFO ring): a launch queued before the
// replacement has finished with the old entry when the build runs (one stream), and the host
// index drops the old key at once, so its next call takes the uncached path.  The host copy is
// updated once the build is enqueued; the call does not wait for it (its copy sources stay in
// d.ak_pend_* until the next build has synchronised).  Caller holds d.mu and has set the device.
int auto_insert(DevCtx& d, const uint8_t* pks, uint64_t n) {
  const uint32_t cap = settings().auto_keys;
  if (cap == 0) return 0;
  std::vector<nwc::u32> add;
  std::unordered_set<std::string> added;
  for (uint64_t i = 0; i < n && add.size() / 8 < cap; ++i) {
    const uint8_t* k = pks + 32 * i;
    if (d.ak_host.find(k)) continue;
    std::string ks(reinterpret_cast<const char*>(k), 32);
    if (added.count(ks)) continue;
    if (!d.ak_seen.count(ks)) {
      if (d.ak_seen.size() >= AUTO_SEEN_MAX) d.ak_seen.clear();
      d.ak_seen.insert(std::move(ks));
      continue;
    }
    d.ak_seen.erase(ks);
    added.insert(ks);
    add.insert(add.end(), reinterpret_cast<const nwc::u32*>(k), reinterpret_cast<const nwc::u32*>(k) + 8);
  }
  const uint32_t m = (uint32_t)(add.size() / 8);
  if (m == 0) return 0;
  if (d.ak_pending) {
    HIP_TRY(hipStreamSynchronize(d.stream));   // the previous build's copy sources are free again
    d.ak_pending = false;
  }
  // positions: append while there is room, then the FIFO ring over [0, cap)
  std::vector<uint32_t> pos(m);
  uint32_t n1 = d.ak_n;
  for (uint32_t j = 0; j < m; ++j) {
    if (n1 < cap) {
      pos[j] = n1++;
    } else {
      pos[j] = d.ak_evict;
      d.ak_evict = (d.ak_evict + 1) % cap;
    }
  }
  if (n1 > d.ak_cap)
    if (int rc = auto_grow(d, std::min(cap, std::max<uint32_t>(AUTO_INIT_KEYS, 2 * n1)))) return rc;
  KeyIndex next = d.ak_host;
  next.keys.resize(8 * (size_t)n1);
  for (uint32_t j = 0; j < m; ++j) std::memcpy(&next.keys[8 * (size_t)pos[j]], &add[8 * (size_t)j], 32);
  std::vector<int32_t> table;
  const uint32_t slots = build_slots(next.keys, n1, table);
  if (slots > d.ak_slot_cap) {
    d.ak_slot_cap = 0;
    HIP_TRY(d.ak_slots.release_async(d.stream));   // after every launch that reads it
    HIP_TRY(d.ak_slots.alloc_async(4 * (size_t)slots, d.stream));
    d.ak_slot_cap = slots;
  }
  d.ak_pend_keys = std::move(add);
  d.ak_pend_slots = table;
  // contiguous runs of positions (at most two: the appended tail and the ring's start)
  for (uint32_t j0 = 0; j0 < m;) {
    uint32_t j1 = j0 + 1;
    while (j1 < m && pos[j1] == pos[j1 - 1] + 1) ++j1;
    const uint32_t p0 = pos[j0], r = j1 - j0;
    HIP_TRY(hipMemcpyAsync(d.ak_keys + 8 * (size_t)p0, d.ak_pend_keys.data() + 8 * (size_t)j0, 32 * (size_t)r,
                           hipMemcpyHostToDevice, d.stream));
    hipLaunchKernelGGL(nwc::k_build_key_tables, dim3((unsigned)((r * 129 + 255) / 256)), dim3(256), 0, d.stream,
                       d.ak_keys + 8 * (size_t)p0, r, d.ak_tables + (size_t)p0 * 129, d.ak_flags + p0);
    HIP_TRY(hipGetLastError());
    if (int rc = build_key_combs(d, d.ak_keys + 8 * (size_t)p0, r, d.ak_comb + (size_t)p0 * nwc::COMB_PER_KEY)) return rc;
    j0 = j1;
  }
  HIP_TRY(hipMemcpyAsync(d.ak_slots, d.ak_pend_slots.data(), 4 * (size_t)slots, hipMemcpyHostToDevice, d.stream));
  d.ak_pending = true;
  next.slots = std::move(table);
  next.mask = slots - 1;
  d.ak_host = std::move(next);
  d.ak_n = n1;
  ++d.ak_builds;
  return 0;
}

// ---- launch helpers (caller holds the device mutex and has set the device) -----------------
// Device memory of the verification path (a primary and workers share the GPU:
// worker/src/worker.rs:182,227).  One launch takes at most NWC_VERIFY_MAX_LAUNCH equations (larger
// calls run as consecutive launches of that size, launch_verify), so the per-launch lists below are
// bounded; and lists larger than NWC_VERIFY_KEEP_BYTES are shrunk to a smaller launch's size
// when one comes (after the device has finished with them).  The per-lane table slots are sized
// for the resident grid, not for n.
// bytes of the per-launch lists: fb_list, uc_list, ts_uniq (4 B per entry) and the torsion hash set
size_t list_bytes(uint64_t cap, uint64_t slots) { return 12 * (size_t)cap + 8 * (size_t)slots; }
int free_lists(DevCtx& d) {
  d.fb_cap = 0;
  d.ts_slot_count = 0;
  HIP_TRY(release_each({&d.fb_list, &d.uc_list, &d.ts_slots, &d.ts_flag, &d.ts_uniq}));
  return 0;
}

int ensure_scratch(DevCtx& d, size_t bytes, uint64_t n) {
  const uint64_t want = n + n / 2 + 4096;
  const bool shrink = !d.hold_lists && d.fb_cap > 4 * want && list_bytes(d.fb_cap, d.ts_slot_count) > settings().verify_keep_bytes;
  if (d.scratch.fits(bytes) && n <= d.fb_cap && !shrink) return 0;
  HIP_TRY(hipEventSynchronize(d.scratch_free));
  HIP_TRY(d.scratch.ensure(bytes));
  if (shrink || n > d.fb_cap) {
    if (int rc = free_lists(d)) return rc;
    const size_t c = want;
    HIP_TRY(d.fb_list.alloc(4 * c));
    HIP_TRY(d.uc_list.alloc(4 * c));
    // the hash set stays at most half full: >= 2 slots per equation
    uint32_t slots = 1024;
    while (slots < 2 * c) slots <<= 1;
    HIP_TRY(d.ts_slots.alloc(4 * (size_t)slots));
    HIP_TRY(d.ts_flag.alloc(4 * (size_t)slots));
    HIP_TRY(d.ts_uniq.alloc(4 * c));
    d.ts_slot_count = slots;
    d.fb_cap = c;
  }
  if (!d.ts_nuniq) HIP_TRY(d.ts_nuniq.alloc(sizeof(uint32_t)));
  return 0;
}

// ev grown to n events (one per chunk in flight, created on first use)
int ensure_events(std::vector<hipEvent_t>& ev, size_t n) {
  while (ev.size() < n) {
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ev.push_back(e);
  }
  return 0;
}

// b grown to need + headroom bytes -- or, with `keep`, replaced by a block of `need` when it holds
// more than keep bytes and under a quarter is needed (Buf::ensure) -- once its users have
// finished: every launch that uses these buffers records scratch_free after its last kernel, so
// waiting for it (and for *drain, a stream whose queued work may use b as well; nullptr = none)
// drains them on any stream.
int ensure_idle(DevCtx& d, RawBuf& b, size_t need, const hipStream_t* drain, size_t headroom = 0,
                size_t keep = nwc::buf::NO_SHRINK) {
  if (b.fits(need, keep)) return 0;
  HIP_TRY(hipEventSynchronize(d.scratch_free));
  if (drain) HIP_TRY(hipStreamSynchronize(*drain));
  HIP_TRY(b.ensure(need, headroom, keep));
  return 0;
}

// Batch-leaf launches: clear the verdict bits of equations whose key has an 8-torsion component
// (dalek verify_batch's randomized domain, answered Err; kernels.hip k_tors_*).  list/count
// (device) restrict the pass to the comb path's uncached equations; nullptr = all n.  The hash set
// is sized for the number of candidate equations, which never exceeds n <= fb_cap.
// phase 1 = mark + eval, 2 = apply, 3 = both.  pre: phase 1 runs before or beside the
// verification (every equation a candidate; the verdict words untouched until apply).
int launch_torsion(DevCtx& d, const uint8_t* pks, uint64_t* out_words, uint64_t n, const uint32_t* list,
                   const uint32_t* count, const nwc::Committee& cm, hipStream_t s, int phase = 3, int pre = 0) {
  if (n == 0) return 0;
  if (2 * n > d.ts_slot_count) return set_err(NWC_ERR_ARG, "torsion set too small for %llu equations", (unsigned long long)n);
  const nwc::KeyMemo memo{d.km_keys, d.km_flag, NWC_MEMO_SLOTS - 1};
  const nwc::TorsArgs t{pks, out_words, list, count, n, d.ts_slots, d.ts_slot_count - 1, d.ts_uniq, d.ts_nuniq, d.ts_flag, cm,
                        memo, pre};
  const uint64_t cap = (uint64_t)d.cus * 8;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, cap);
  if (phase & 1) {
    HIP_TRY(hipMemsetAsync(d.ts_slots, 0xFF, 4 * (size_t)d.ts_slot_count, s));
    HIP_TRY(hipMemsetAsync(d.ts_nuniq, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(nwc::k_tors_mark, dim3(grid), dim3(256), 0, s, t);
    HIP_TRY(hipGetLastError());
    if (n <= NWC_WIDE_MAX) {
      // a certificate's worth of keys: one limb-sliced wave per distinct key (latency)
      hipLaunchKernelGGL(nwc::k_tors_eval_sliced, dim3((unsigned)n), dim3(64), 0, s, t);
    } else {
      hipLaunchKernelGGL(nwc::k_tors_eval, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)d.cus * 2)), dim3(256), 0, s, t);
    }
    HIP_TRY(hipGetLastError());
  }
  if (phase & 2) {
    hipLaunchKernelGGL(nwc::k_tors_apply, dim3(grid), dim3(256), 0, s, t);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

// Device buffers of the launch keys (launch_keys.h), allocated once per device except the combs
// (20 MB per key), which grow as keys ask to join; the set starts empty.  Caller holds d.mu.
int lk_ensure(DevCtx& d, hipStream_t s) {
  if (d.lk_alloc) return 0;
  HIP_TRY(d.lk_keys.alloc(32 * (size_t)nwc::LK_MAX_KEYS));
  HIP_TRY(d.lk_flags.alloc(4 * (size_t)nwc::LK_MAX_KEYS));
  HIP_TRY(d.lk_slots.alloc(4 * (size_t)nwc::LK_SLOTS));
  HIP_TRY(d.lk_bases.alloc((size_t)nwc::LK_MAX_KEYS * nwc::KeyComb::windows * sizeof(nwc::ge_p3)));
  HIP_TRY(d.lk_state.alloc(16));
  if (!d.lk_demand) HIP_TRY(d.lk_demand.alloc(sizeof(uint32_t)));   // (nwc_trim keeps this word)
  *reinterpret_cast<volatile uint32_t*>(d.lk_demand.get()) = 0;
  d.lk = nwc::LaunchKeys{d.lk_keys, d.lk_flags, d.lk_slots, nullptr, d.lk_bases, d.lk_state, d.lk_demand.dev(), 0};
  HIP_TRY(hipMemsetAsync(d.lk.slots, 0xFF, 4 * (size_t)nwc::LK_SLOTS, s));
  HIP_TRY(hipMemsetAsync(d.lk.state, 0, 16, s));
  d.lk_alloc = true;
  d.lk_censused = false;
  return 0;
}

// Room for the keys that asked to join: the first launch-key launch (and the first after
// nwc_set_committee emptied the set) runs the census once and waits for its demand; later launches
// read the demand the previous ones left in host memory (no sync) and grow the combs
// stream-ordered on s (held combs copied), so a key that did not fit joins at the next launch.
// Called after s waits for scratch_free (no launch still reads the set).
int lk_reserve(DevCtx& d, const uint8_t* pks, uint64_t n, hipStream_t s) {
  nwc::LaunchKeys& k = d.lk;
  if (k.cap >= nwc::LK_MAX_KEYS) return 0;
  if (!d.lk_censused) {
    // nothing held: with the room for no key the select only counts, then the host reads its demand
    nwc::LaunchKeys count_only = k;
    count_only.cap = 0;
    hipLaunchKernelGGL(nwc::k_lk_select, dim3(1), dim3(1024), 0, s, pks, n, count_only);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    d.lk_censused = true;
  }
  const uint32_t demand = *reinterpret_cast<volatile uint32_t*>(d.lk_demand.get());
  if (demand <= k.cap) return 0;
  const uint32_t cap = std::min<uint32_t>(nwc::LK_MAX_KEYS, (demand + 7) / 8 * 8);
  Buf<nwc::ge_niels_pad> comb;
  const size_t per = nwc::COMB_PER_KEY * sizeof(nwc::ge_niels_pad);
  HIP_TRY(comb.alloc_async((size_t)cap * per, s));
  if (d.lk_comb) {
    if (hipError_t e = hipMemcpyAsync(comb, d.lk_comb, (size_t)k.cap * per, hipMemcpyDeviceToDevice, s)) {
      (void)comb.release_async(s);
      HIP_TRY(e);
    }
  }
  const hipError_t freed = d.lk_comb.release_async(s);   // behind the copy
  (void)d.lk_comb.adopt(std::move(comb));
  k.comb = d.lk_comb;
  k.cap = cap;
  HIP_TRY(freed);
  return 0;
}

// Large host calls copy their pageable inputs through the device's pinned stages, filled by
// NWC_HOST_STAGING_THREADS (8) host threads (straight from pageable memory measured 7-10 % slower,
// profiles/r05/wire_host.md; that switch was removed in round 6).
// The device's transfer stream and its pinned stages.  Caller holds d.mu.
int ensure_stager(DevCtx& d) {
  if (!d.xfer) HIP_TRY(hipStreamCreateWithFlags(&d.xfer, hipStreamNonBlocking));
  if (!d.stager) {
    auto st = std::make_unique<HostStager>();
    const hipError_t e = st->init(d.xfer, settings().host_staging_threads);
    if (e != hipSuccess) {
      st->release();
      return set_err(NWC_ERR_DEVICE, "host stager: %s", hipGetErrorString(e));
    }
    d.stager = std::move(st);
  }
  return 0;
}

// The batch entries' buffers (Straus tables, MSM groups, the per-certificate resolution) above
// NWC_VERIFY_KEEP_BYTES that the current launch does not use are freed -- after every launch that
// used them, each of which records scratch_free -- so a process that ran the Straus or MSM entry
// once holds at most the keep threshold of them while it verifies by other paths.
int release_idle_buffers(DevCtx& d, const uint8_t* in_use) {
  const size_t keep = settings().verify_keep_bytes;
  RawBuf* const bufs[] = {&d.straus_scratch, &d.msm_scratch, &d.rs_buf, &d.pair_buf, &d.sign_buf};
  auto idle = [&](const RawBuf* b) { return b->raw() && b->raw() != in_use && b->raw() != d.busy_buf && b->bytes() > keep; };
  if (std::none_of(std::begin(bufs), std::end(bufs), idle)) return 0;
  HIP_TRY(hipEventSynchronize(d.scratch_free));
  for (RawBuf* b : bufs)
    if (idle(b)) HIP_TRY(b->release());
  return 0;
}

// One launch of the paired strict host pipeline (verify_paired): launches on two streams may run at
// the same time, so each takes half of the table slots (`half`; grid capped at half the persistent
// grid) and lists its failed reductions in its own region of the fallback list with its own count;
// the caller orders the slots against other launches (scratch_free), sized the list beforehand and
// runs the fallback passes once the pipeline has joined (a fallback launch queued behind a chunk
// would wait for free slots while the other stream's chunk holds them, stalling its stream).
struct PairLaunch {
  int half;
  uint32_t* fb_list;
  uint32_t* fb_count;
};

// The committee cache, the auto cache and the launch keys as a kernel's key set.
nwc::Committee committee_of(const DevCtx& d) {
  return nwc::Committee{d.cm_keys, d.cm_flags, d.cm_tables, d.cm_comb, d.cm_slots, d.cm_slot_mask, d.cm_n};
}
nwc::Committee auto_committee_of(const DevCtx& d) {
  return nwc::Committee{d.ak_keys, d.ak_flags, d.ak_tables, d.ak_comb, d.ak_slots, d.ak_host.mask, d.ak_n};
}
nwc::Committee launch_committee_of(const DevCtx& d) {
  return nwc::Committee{d.lk.keys, d.lk.flags, nullptr, d.lk.comb, d.lk.slots, nwc::LK_SLOTS - 1, nwc::LK_MAX_KEYS};
}

// What verify_plan.h's decisions read of the device, the settings and the knobs.
nwc::plan::DeviceView device_view(const DevCtx& d) {
  const nwc::plan::Settings& st = settings();
  nwc::plan::DeviceView v;
  v.path = st.verify_path;
  v.cm_n = d.cm_n;
  v.cm_comb = d.cm_comb != nullptr;
  v.comb16 = d.comb16 != nullptr;
  v.ak_n = d.ak_n;
  v.ak_comb = d.ak_comb != nullptr;
  v.launch_keys = knobs().launch_keys.load() != 0;
  v.cold = st.cold;
  v.cold_max = st.cold_max;
  v.fb_cap = d.fb_cap;
  v.verify_max_launch = st.verify_max_launch;
  return v;
}
bool deferrable_list(const DevCtx& d) { return nwc::plan::deferrable_list(device_view(d)); }
// Whether launch_verify takes the comb path (k_verify_comb) for a plain launch of n equations.
bool takes_comb_path(const DevCtx& d, uint64_t n, int strict) {
  return nwc::plan::comb_path(device_view(d), n, strict != 0).comb;
}

// One verification launch: equation i checks msgs (msg_index[i] or i * msg_stride), pks and sigs on
// the device and sets bit i of out_words, on `stream`.
struct VerifyLaunch {
  const uint8_t* msgs = nullptr;
  const uint32_t* msg_index = nullptr;
  uint64_t msg_stride = 0;
  const uint8_t* pks = nullptr;
  const uint8_t* sigs = nullptr;
  uint64_t n = 0;
  int strict = 0;
  uint64_t* out_words = nullptr;
  hipStream_t stream = nullptr;
  int flags = 0;                            // LV_*
  uint8_t* vbytes = nullptr;                // zero-copy: a verdict byte per equation in host memory
  uint64_t list_base = 0;                   // LV_DEFER_LIST: equation i is listed as list_base + i
  const PairLaunch* pair = nullptr;
  const nwc::SignRecs* sign_recs = nullptr;   // the sign tests deferred: their records
  const nwc::SignPass* sign_pass = nullptr;   // ... and the previous launch's votes, tested in this launch's first blocks
};

// The single-kernel launches (latency kernels, zero-copy cold): no table slots, no lists.
int enqueue_single(DevCtx& d, const VerifyLaunch& q, const nwc::plan::Route& r) {
  using nwc::plan::Kernel;
  const uint64_t n = q.n;
  const bool cold = r.kernel == Kernel::ZeroCopyCold;
  if (r.kernel == Kernel::AutoWide) ++d.ak_hits;
  const nwc::Committee cm = cold ? nwc::Committee{} : r.kernel == Kernel::AutoWide ? auto_committee_of(d) : committee_of(d);
  const nwc::VerifyArgs a{q.msgs, q.msg_index, q.msg_stride, q.pks, q.sigs, q.out_words, n, q.strict, d.base_table, d.base24,
                          d.scratch, d.fb_list, d.fb_count, cold ? settings().force_fallback_every : 0u, cm};
  if (r.zero_words) HIP_TRY(hipMemsetAsync(q.out_words, 0, 8 * r.zero_words, q.stream));
  if (cold) {
    hipLaunchKernelGGL(nwc::k_verify_cold, dim3((unsigned)n), dim3(256), 0, q.stream, a, (const nwc::ge_niels_pad*)d.comb16,
                       q.vbytes);
  } else {
    // a key missing on the device after all sets the word after the verdict words
    const nwc::CombArgs ca{nullptr, reinterpret_cast<uint32_t*>(q.out_words + (n + 63) / 64), d.comb_base, d.comb16,
                           q.vbytes};
    hipLaunchKernelGGL(nwc::k_verify_comb_wide, dim3((unsigned)n), dim3(128), 0, q.stream, a, ca);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// The launches over the table slots and lists, as the route says: the launch-key build, the
// torsion test beside, the main kernel, the uncached list's pass, the fallback, the torsion pass.
int enqueue_listed(DevCtx& d, const VerifyLaunch& q, const nwc::plan::Route& r) {
  using nwc::plan::Kernel;
  using nwc::plan::Torsion;
  const uint64_t n = q.n;
  const hipStream_t s = q.stream;
  const bool defer = (q.flags & LV_DEFER_LIST) != 0;
  const uint64_t tiles = (n + 255) / 256;
  // persistent grid: a few blocks per resident slot so the tail is short
  const uint64_t cap = (uint64_t)d.cus * d.verify_blocks_per_cu * NWC_VERIFY_GRID_MULT;
  size_t need = (size_t)cap * 256 * 2 * nwc::TAB_BYTES_PER_LANE;
  const uint64_t gcap = q.pair ? cap / 2 : cap;
  const unsigned grid = (unsigned)(tiles < gcap ? tiles : gcap);
  // comb grid: at most the resident blocks; tile t goes to block t mod grid, so every lane gets
  // ceil or floor of n / lanes equations (in chunks of COMB_BATCH sharing one inversion), and
  // a small n spreads one equation per lane
  unsigned gridc = 0;
  if (r.comb) {
    const uint64_t resident = (uint64_t)d.cus * d.comb_blocks_per_cu;
    gridc = (unsigned)std::min<uint64_t>(tiles, resident);
    need = std::max(need, (size_t)resident * 256 * nwc::COMB_BYTES_PER_LANE);
  }
  // (deferred: n = the lists' capacity, so they are neither grown nor shrunk under the pending list)
  if (int rc = ensure_scratch(d, need, defer ? d.fb_cap : n)) return rc;
  if (r.lk_build)
    if (int rc = lk_ensure(d, s)) return rc;
  if (r.error) return set_err(NWC_ERR_ARG, "%s", r.error);
  if (r.scratch_order) HIP_TRY(hipStreamWaitEvent(s, d.scratch_free, 0));
  if (r.lk_build) {
    // the set's update is ordered after every launch that read it (scratch_free) and before this
    // launch's comb kernel; the builds exit at once when no key joined
    if (int rc = lk_reserve(d, q.pks, n, s)) return rc;
    hipLaunchKernelGGL(nwc::k_lk_select, dim3(1), dim3(1024), 0, s, q.pks, n, d.lk);
    hipLaunchKernelGGL(nwc::k_lk_keys, dim3((nwc::LK_MAX_KEYS + 63) / 64), dim3(64), 0, s, d.lk);
    hipLaunchKernelGGL(nwc::k_build_comb_from_bases<nwc::KeyComb>, dim3((unsigned)(d.cus * 8)), dim3(256), 0, s,
                       (const nwc::ge_p3*)d.lk.bases, 0u, 0u, (const uint32_t*)d.lk.state, d.lk.comb);
    HIP_TRY(hipGetLastError());
  }
  const nwc::Committee cm = r.lk_build ? launch_committee_of(d) : committee_of(d);
  nwc::VerifyArgs a{q.msgs, q.msg_index, q.msg_stride, q.pks, q.sigs, q.out_words, n, q.strict, d.base_table, d.base24,
                    d.scratch, d.fb_list, d.fb_count, settings().force_fallback_every, cm};
  if (q.pair) {
    a.scratch = d.scratch + (size_t)(q.pair->half ? cap / 2 : 0) * 256 * 2 * nwc::TAB_BYTES_PER_LANE;
    a.fb_list = q.pair->fb_list;
    a.fb_count = q.pair->fb_count;
  }
  a.force_windows = knobs().force_windows.load();
  a.stamps = d.stamps;
  const nwc::CombArgs ca{d.uc_list, d.uc_count, d.comb_base, d.comb16, nullptr, (uint32_t)(defer ? q.list_base : 0)};
  if (r.torsion == Torsion::Beside) {
    HIP_TRY(hipEventRecord(d.ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(d.side, d.ev_fork, 0));
    if (int rc = launch_torsion(d, q.pks, q.out_words, n, nullptr, nullptr, cm, d.side, 1, 1)) return rc;
    HIP_TRY(hipEventRecord(d.ev_join, d.side));
  }
  if (r.zero_fb_count) HIP_TRY(hipMemsetAsync(a.fb_count, 0, sizeof(uint32_t), s));
  if (r.list_pass) HIP_TRY(hipMemsetAsync(d.uc_count, 0, sizeof(uint32_t), s));
  if (r.zero_words) HIP_TRY(hipMemsetAsync(q.out_words, 0, 8 * r.zero_words, s));
  // R' and the projective y test now, the sign of x(R') later in k_comb_sign over many votes (or
  // in the first blocks of the next such launch: sign_pass, the previous launch's votes)
  const unsigned gy = (unsigned)std::min<uint64_t>(tiles, 60000);
  switch (r.kernel) {
    case Kernel::CombYSign:
      hipLaunchKernelGGL(nwc::k_verify_comb_y_sign, dim3(gy + q.sign_pass->blocks), dim3(256), 0, s, a, ca, *q.sign_recs,
                         *q.sign_pass);
      break;
    case Kernel::CombY:
      hipLaunchKernelGGL(nwc::k_verify_comb_y, dim3(gy), dim3(256), 0, s, a, ca, *q.sign_recs);
      break;
    case Kernel::CombWide:   // small batches: one block per equation, critical path = one square root
      hipLaunchKernelGGL(nwc::k_verify_comb_wide, dim3((unsigned)n), dim3(128), 0, s, a, ca);
      break;
    case Kernel::Comb:
      hipLaunchKernelGGL(nwc::k_verify_comb, dim3(gridc), dim3(256), 0, s, a, ca);
      break;
    case Kernel::Cold:
      hipLaunchKernelGGL(nwc::k_verify_cold, dim3((unsigned)n), dim3(256), 0, s, a, (const nwc::ge_niels_pad*)d.comb16,
                         (uint8_t*)nullptr);
      break;
    case Kernel::HalfCached:
      hipLaunchKernelGGL((nwc::k_verify<true, true>), dim3(grid), dim3(256), 0, s, a, ca);
      break;
    case Kernel::HalfStamp:
      hipLaunchKernelGGL((nwc::k_verify<true, false, false, true>), dim3(grid), dim3(256), 0, s, a, ca);
      break;
    case Kernel::Half:
      hipLaunchKernelGGL((nwc::k_verify<true, false>), dim3(grid), dim3(256), 0, s, a, ca);
      break;
    case Kernel::Full:
      hipLaunchKernelGGL((nwc::k_verify<false, false>), dim3(grid), dim3(256), 0, s, a, ca);
      break;
    default:
      return set_err(NWC_ERR_ARG, "a single-kernel route among the listed launches");
  }
  HIP_TRY(hipGetLastError());
  if (r.list_pass) {
    // uncached keys: half-size equations in list mode (waves exit at once when the list is empty)
    nwc::VerifyArgs l = a;
    l.committee.n = 0;
    hipLaunchKernelGGL((nwc::k_verify<true, false, true>), dim3(grid), dim3(256), 0, s, l, ca);
    HIP_TRY(hipGetLastError());
  }
  if (r.fallback) {
    // lanes whose reduction failed are rare (|c| or d >= 2^147); a few blocks suffice
    const unsigned fgrid = grid < 16u ? grid : 16u;
    hipLaunchKernelGGL(nwc::k_verify_fallback, dim3(fgrid), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
  }
  if (r.torsion == Torsion::Beside) {
    HIP_TRY(hipStreamWaitEvent(s, d.ev_join, 0));
    if (int rc = launch_torsion(d, q.pks, q.out_words, n, nullptr, nullptr, cm, s, 2, 1)) return rc;
  } else if (r.torsion != Torsion::None) {
    const bool list = r.torsion == Torsion::AfterList;
    if (int rc = launch_torsion(d, q.pks, q.out_words, n, list ? d.uc_list : nullptr, list ? d.uc_count : nullptr, cm, s))
      return rc;
  }
  if (r.scratch_order) HIP_TRY(hipEventRecord(d.scratch_free, s));
  return 0;
}

int launch_verify(DevCtx& d, const VerifyLaunch& q) {
  if (q.n == 0) return 0;
  if (int rc = ensure_verify_tables(d)) return rc;
  if (int rc = release_idle_buffers(d, nullptr)) return rc;
  const nwc::plan::DeviceView view = device_view(d);
  const nwc::plan::Request req{q.n, q.strict != 0, q.flags, q.list_base, q.vbytes != nullptr, q.pair != nullptr,
                               q.sign_recs != nullptr, q.sign_pass && q.sign_pass->n};
  if (nwc::plan::splits(view, req)) {
    // consecutive launches of at most NWC_VERIFY_MAX_LAUNCH equations (a multiple of 64: whole
    // verdict words), so the per-launch lists stay bounded; every equation is independent, so the
    // verdicts are those of one launch (launch keys and the torsion set are per launch anyway)
    const uint64_t step = view.verify_max_launch;
    for (uint64_t lo = 0; lo < q.n; lo += step) {
      VerifyLaunch part = q;
      if (!q.msg_index) part.msgs = q.msgs + 32 * lo * q.msg_stride;
      if (q.msg_index) part.msg_index = q.msg_index + lo;
      part.pks = q.pks + 32 * lo;
      part.sigs = q.sigs + 64 * lo;
      part.n = std::min(step, q.n - lo);
      part.out_words = q.out_words + lo / 64;
      part.list_base = q.list_base + lo;
      part.pair = nullptr;
      part.sign_recs = nullptr;
      part.sign_pass = nullptr;
      if (int rc = launch_verify(d, part)) return rc;
    }
    return 0;
  }
  const nwc::plan::Route r = nwc::plan::route_verify(view, req);
  if (nwc::plan::early_error(r)) return set_err(NWC_ERR_ARG, "%s", r.error);
  return r.scratch ? enqueue_listed(d, q, r) : enqueue_single(d, q, r);   // (enqueue_listed returns a late error)
}

// The passes LV_DEFER_LIST launches left out, once over equations [0, n) of the arrays they were
// launched on (their list holds indices into these): the uncached equations' half-size list
// launch, its fallback and (batch leaves) the torsion pass over the same list.
int finish_deferred_list(DevCtx& d, const uint8_t* msgs, const uint32_t* msg_index, uint64_t msg_stride,
                         const uint8_t* pks, const uint8_t* sigs, uint64_t n, int strict, uint64_t* out_words,
                         hipStream_t s) {
  if (n == 0) return 0;
  if (!deferrable_list(d) || n > d.fb_cap) return set_err(NWC_ERR_ARG, "deferred list finish off the comb path");
  const uint64_t tiles = (n + 255) / 256;
  const uint64_t cap = (uint64_t)d.cus * d.verify_blocks_per_cu * NWC_VERIFY_GRID_MULT;
  const unsigned grid = (unsigned)(tiles < cap ? tiles : cap);
  if (int rc = ensure_scratch(d, (size_t)cap * 256 * 2 * nwc::TAB_BYTES_PER_LANE, d.fb_cap)) return rc;
  HIP_TRY(hipStreamWaitEvent(s, d.scratch_free, 0));
  const nwc::Committee cm = committee_of(d);
  nwc::VerifyArgs a{msgs, msg_index, msg_stride, pks, sigs, out_words, n, strict, d.base_table, d.base24, d.scratch,
                    d.fb_list, d.fb_count, settings().force_fallback_every, cm};
  a.force_windows = knobs().force_windows.load();
  a.stamps = d.stamps;
  const nwc::CombArgs ca{d.uc_list, d.uc_count, d.comb_base, d.comb16};
  HIP_TRY(hipMemsetAsync(d.fb_count, 0, sizeof(uint32_t), s));
  nwc::VerifyArgs l = a;
  l.committee.n = 0;
  hipLaunchKernelGGL((nwc::k_verify<true, false, true>), dim3(grid), dim3(256), 0, s, l, ca);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(nwc::k_verify_fallback, dim3(grid < 16u ? grid : 16u), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  if (!strict)
    if (int rc = launch_torsion(d, pks, out_words, n, d.uc_list, d.uc_count, cm, s)) return rc;
  HIP_TRY(hipEventRecord(d.scratch_free, s));
  return 0;
}

// sr with its arrays moved by `off` records (record i of the result is record i + off of sr)
nwc::SignRecs sign_recs_at(const nwc::SignRecs& r, int64_t off) {
  return nwc::SignRecs{r.x + 8 * off, r.z + 8 * off, r.p + 8 * off, r.meta + off};
}
// k_comb_sign over votes [v0, v0 + n) of sr (v0 a multiple of 64): about 8 votes per lane, so the
// lane's one inversion is shared, and at most the resident comb lanes
uint32_t comb_sign_blocks(const DevCtx& d, uint64_t n) {
  constexpr uint64_t per = 8;   // votes per lane
  const uint64_t resident = (uint64_t)d.cus * d.comb_blocks_per_cu;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(resident, (n + 256 * per - 1) / (256 * per)));
}
int launch_comb_sign(DevCtx& d, const nwc::SignRecs& sr, uint64_t v0, uint64_t n, uint64_t* out_bits, hipStream_t s) {
  if (n == 0) return 0;
  if (v0 & 63) return set_err(NWC_ERR_ARG, "sign pass off a verdict word");
  const uint32_t blocks = comb_sign_blocks(d, n);
  hipLaunchKernelGGL(nwc::k_comb_sign, dim3(blocks), dim3(256), 0, s, sr, v0, n, out_bits);
  HIP_TRY(hipGetLastError());
  return 0;
}

int launch_digest(const uint8_t* data, const uint64_t* offsets, const uint64_t* ends, uint64_t n, uint8_t* out32,
                  hipStream_t s) {
  if (n == 0) return 0;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  int cus = 0;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  // more than one wave per SIMD of one-lane-per-message work: schedule blocks instead
  const int mode = settings().digest_sched;   // NWC_DIGEST_SCHED=0/1 forces a kernel (A/B and tests)
  const bool sched = mode >= 0 ? mode == 1 : n > 64ull * 4 * (uint64_t)cus;
  if (sched) {
    hipLaunchKernelGGL(nwc::k_sha512_digest32_sched, dim3((unsigned)cus), dim3(256), 0, s, data, offsets, ends, n,
                       out32);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(nwc::k_sha512_digest32, dim3(grid), dim3(256), 0, s, data, offsets, ends, n, out32);
  HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cert_reduce(const uint64_t* leaf, const uint32_t* offs, uint64_t m, uint64_t nvotes, uint64_t* cert,
                       uint64_t* bad, hipStream_t s) {
  const uint64_t words = (nvotes + 63) / 64;
  const uint64_t threads = m > words ? m : words;
  if (threads == 0) return 0;
  const unsigned grid = (unsigned)((threads + 255) / 256);
  hipLaunchKernelGGL(nwc::k_cert_reduce, dim3(grid), dim3(256), 0, s, leaf, offs, m, nvotes, cert, bad);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Run fn(device_index, lo, hi) over [0, n) split across all devices, one host thread each.  The
// ranges come from nwc_shard_bounds: every range but the last starts on a multiple of 64 units.
template <class F>
int shard(uint64_t n, F fn) {
  const int nd = (int)g_devs.size();
  if (nd == 1 || n < 4096) return fn(0, (uint64_t)0, n);
  std::vector<int> rc(nd, 0);
  std::vector<std::thread> th;
  for (int i = 0; i < nd; ++i) {
    uint64_t lo = 0, hi = 0;
    nwc_shard_bounds(n, (uint32_t)nd, (uint32_t)i, &lo, &hi);
    th.emplace_back([&, i, lo, hi] {
      rc[i] = fn(i, lo, hi);
    });
  }
  for (auto& t : th) t.join();
  for (int r : rc) if (r < 0) return r;
  return 0;
}

// Copy `nbits` bits of device verdict words to a host bitmap starting at bit `bit0`.
void merge_bits(uint8_t* dst, uint64_t bit0, const std::vector<uint64_t>& words, uint64_t nbits) {
  // dst bits [bit0, bit0 + nbits) = source bits [0, nbits); bits of dst outside the range kept
  auto put1 = [&](uint64_t b) {
    const uint64_t o = bit0 + b;
    const bool v = (words[b >> 6] >> (b & 63)) & 1;
    dst[o >> 3] = (uint8_t)((dst[o >> 3] & ~(1u << (o & 7))) | ((unsigned)v << (o & 7)));
  };
  uint64_t b = 0;
  if ((bit0 & 7) == 0) {
    const uint64_t full = nbits / 8;
    std::memcpy(dst + bit0 / 8, words.data(), full);
    b = full * 8;
  } else {
    // head bits up to a destination byte boundary, then 8 source bits per destination byte
    for (; b < nbits && ((bit0 + b) & 7); ++b) put1(b);
    for (; b + 8 <= nbits; b += 8) {
      const uint64_t w = b >> 6, sh = b & 63;
      uint64_t v = words[w] >> sh;
      if (sh > 56 && w + 1 < words.size()) v |= words[w + 1] << (64 - sh);
      dst[(bit0 + b) >> 3] = (uint8_t)v;
    }
  }
  for (; b < nbits; ++b) put1(b);
}

// Certificates [c_lo, c_end) of offsets (m + 1 entries) whose votes meet [lo, hi), lo < hi <= offsets[m].
void cert_span(const uint32_t* offsets, uint64_t m, uint64_t lo, uint64_t hi, uint64_t& c_lo, uint64_t& c_end) {
  c_lo = (uint64_t)(std::upper_bound(offsets, offsets + m + 1, (uint32_t)lo) - offsets) - 1;   // offsets[c_lo] <= lo
  c_end = (uint64_t)(std::lower_bound(offsets, offsets + m + 1, (uint32_t)hi) - offsets);     // first offsets[c] >= hi
}

// vote -> certificate index of votes [lo, hi) on the host (small calls; k_cert_index on the device)
void fill_cert_index(uint32_t* dst, const uint32_t* offsets, uint64_t c_lo, uint64_t c_end, uint64_t lo, uint64_t hi) {
  for (uint64_t c = c_lo; c < c_end; ++c) {
    const uint64_t a = std::max<uint64_t>(offsets[c], lo), b = std::min<uint64_t>(offsets[c + 1], hi);
    if (b > a) std::fill(dst + (a - lo), dst + (b - lo), (uint32_t)c);
  }
}

// vote -> certificate index of votes [lo, hi) on stream s, from the offsets already at doffs
// (certificates c_lo .. c_end)
void launch_cert_index(const uint32_t* doffs, uint64_t c_lo, uint64_t c_end, uint64_t lo, uint64_t hi, uint32_t* dmi,
                       hipStream_t s) {
  const uint64_t ncert = c_end - c_lo;
  const unsigned grid = (unsigned)std::min<uint64_t>((ncert * 64 + 255) / 256, 16384);
  hipLaunchKernelGGL(nwc::k_cert_index, dim3(grid), dim3(256), 0, s, doffs, (uint32_t)c_lo, (uint32_t)ncert, lo, hi, dmi);
}

// One host-memory verification call on a device: the caller's arrays, its equations [lo, lo + n)
// and their places in the device arena.  Batch mode (cert_offsets, the m + 1 vote offsets of the
// call's certificates; msgs = their m digests): equation v checks digest c with
// offsets[c] <= v < offsets[c + 1], c in [c_lo, c_end).
struct HostCall {
  const uint8_t* msgs;
  uint64_t msg_stride;
  const uint32_t* cert_offsets;
  const uint8_t* pks;
  const uint8_t* sigs;
  uint64_t lo, n, words, nmsgs;
  int strict;
  uint64_t c_lo = 0, c_end = 0;
  uint64_t msg_bytes = 0;
  size_t need = 0, offs_bytes = 0;   // arena bytes up to the verdict words' end; of the offsets after them
  uint8_t* dm = nullptr;
  uint32_t* dmi = nullptr;     // batch: vote -> certificate index
  uint8_t* dp = nullptr;
  uint8_t* ds = nullptr;
  uint64_t* dout = nullptr;    // words + the latency kernel's missing-key word
  uint32_t* doffs = nullptr;   // batch, large ranges: k_cert_index's input
  bool batch() const { return cert_offsets != nullptr; }
  // the launch of equations [c0, c0 + len) of the device arrays on s
  VerifyLaunch launch(uint64_t c0, uint64_t len, hipStream_t s) const {
    return {.msgs = msg_stride ? dm + 32 * c0 : dm, .msg_index = batch() ? dmi + c0 : nullptr, .msg_stride = msg_stride ? 1u : 0u,
            .pks = dp + 32 * c0, .sigs = ds + 64 * c0, .n = len, .strict = strict, .out_words = dout + c0 / 64, .stream = s};
  }
};

// Inputs of equations [c0, c0 + len) through the pinned stages on the transfer stream; ev is
// recorded behind them.
int stage_chunk(DevCtx& d, const HostCall& c, uint64_t c0, uint64_t len, hipEvent_t ev) {
  HostStager& hs = *d.stager;
  if (c.msg_stride) HIP_TRY(hs.put(c.dm + 32 * c0, c.msgs + 32 * (c.lo + c0), 32 * len));
  HIP_TRY(hs.put(c.dp + 32 * c0, c.pks + 32 * (c.lo + c0), 32 * len));
  HIP_TRY(hs.put(c.ds + 64 * c0, c.sigs + 64 * (c.lo + c0), 64 * len));
  HIP_TRY(hs.flush());
  HIP_TRY(hipEventRecord(ev, d.xfer));
  return 0;
}

// The verdict words to the host once the device stream is done (NWC_HOST_TIMING: the phases' times).
int collect_words(DevCtx& d, const HostCall& c, std::vector<uint64_t>& out_words, const char* kind, uint64_t nch,
                  std::chrono::steady_clock::time_point tv0) {
  const auto tq = std::chrono::steady_clock::now();
  HIP_TRY(hipMemcpyAsync(out_words.data(), c.dout, 8 * c.words, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(hipStreamSynchronize(d.stream));
  if (settings().host_timing)
    std::fprintf(stderr, "nwc host call%s: %llu equations in %llu chunks: copies queued after %.2f ms, done %.2f ms later\n", kind,
                 (unsigned long long)c.n, (unsigned long long)nch, std::chrono::duration<double>(tq - tv0).count() * 1e3,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - tq).count() * 1e3);
  return 0;
}

// Small call (a certificate, a header): packed into pinned memory, then one H2D and one D2H -- or,
// with every key cached or none (first sight), read in place by one kernel that stores a verdict
// byte per equation there (zero copy).
int verify_small(DevCtx& d, const HostCall& c, std::vector<uint64_t>& out_words) {
  using nwc::plan::SmallMode;
  const uint64_t n = c.n, words = c.words;
  if (int rc = d.ensure_pinned(NWC_PINNED_STAGE_MAX)) return rc;
  uint8_t* h = d.pinned;
  const uint8_t* keys = c.pks + 32 * c.lo;
  std::memcpy(h + (c.dm - d.arena), c.batch() ? c.msgs : c.msgs + (c.msg_stride ? 32 * c.lo : 0), c.msg_bytes);
  if (c.batch())
    fill_cert_index(reinterpret_cast<uint32_t*>(h + ((uint8_t*)c.dmi - d.arena)), c.cert_offsets, c.c_lo, c.c_end, c.lo, c.lo + n);
  std::memcpy(h + (c.dp - d.arena), keys, 32 * n);
  std::memcpy(h + (c.ds - d.arena), c.sigs + 64 * c.lo, 64 * n);
  std::memset(h + ((uint8_t*)c.dout - d.arena), 0, 8 * (words + 1));
  const bool cm_hit = d.cm_n && g_hcm.all_cached(keys, n);
  const bool ak_hit = !cm_hit && d.ak_n && n <= NWC_WIDE_MAX && d.ak_host.all_found(keys, n);
  const nwc::plan::SmallRoute sr =
      nwc::plan::small_call_route(device_view(d), settings(), n, cm_hit, ak_hit, c.need, NWC_PINNED_STAGE_MAX);
  int fl = sr.flags;
  const size_t staged_bytes = (size_t)((uint8_t*)c.dout - d.arena) + 8 * (words + 1);
  if (sr.mode != SmallMode::Staged) {
    uint8_t* hb = h + align256(c.need);   // byte verdicts of a zero-copy launch, after the staged inputs
    std::memset(hb, 0, n);
    auto dev = [&](const void* p) { return p ? d.pinned.dev() + ((const uint8_t*)p - d.arena) : nullptr; };
    VerifyLaunch zc = c.launch(0, n, d.stream);
    zc.msgs = dev(c.dm);
    zc.msg_index = reinterpret_cast<const uint32_t*>(dev(c.dmi));
    zc.pks = dev(c.dp);
    zc.sigs = dev(c.ds);
    zc.flags = fl;
    zc.vbytes = d.pinned.dev() + (hb - h);
    if (int rc = launch_verify(d, zc)) return rc;
    // poll the verdict bytes (bit 7 = written); a launch that never writes them (a device error)
    // falls back to the stream wait after 200 ms, which reports the error
    const bool spin = settings().spin_wait;   // 0 = wait for the stream (A/B)
    if (!spin || !nwc::plan::poll_written(hb, n, std::chrono::milliseconds(200))) {
      HIP_TRY(hipStreamSynchronize(d.stream));
      if (spin && !nwc::plan::poll_written(hb, n, std::chrono::microseconds(0)))
        return set_err(NWC_ERR_DEVICE, "latency kernel left verdicts unwritten");
    }
    bool missing = false;
    for (uint64_t i = 0; i < n; ++i) {
      if (hb[i] & 1) out_words[i >> 6] |= 1ull << (i & 63);
      missing = missing || (hb[i] & 2);
    }
    if (!missing) return sr.mode == SmallMode::ZeroCopyCold ? auto_insert(d, keys, n) : 0;
    // a key was missing on the device after all (cold: a reduction failed): stage the inputs
    // and run the general path
    std::fill(out_words.begin(), out_words.end(), 0);
    fl &= ~(LV_ALL_CACHED | LV_AUTO);
  }
  HIP_TRY(hipMemcpyAsync(d.arena, h, staged_bytes, hipMemcpyHostToDevice, d.stream));
  VerifyLaunch q = c.launch(0, n, d.stream);
  q.flags = fl;
  if (int rc = launch_verify(d, q)) return rc;
  HIP_TRY(hipMemcpyAsync(h, c.dout, 8 * (words + 1), hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(hipStreamSynchronize(d.stream));
  if ((fl & LV_ALL_CACHED) && h[8 * words] != 0) {
    // a key was missing on the device after all: the general path decides every equation
    if (int rc = launch_verify(d, c.launch(0, n, d.stream))) return rc;
    HIP_TRY(hipMemcpyAsync(h, c.dout, 8 * words, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
  }
  std::memcpy(out_words.data(), h, 8 * words);
  if (!(fl & LV_ALL_CACHED) && n <= NWC_WIDE_MAX && settings().verify_path == VPath::Default)
    if (int rc = auto_insert(d, keys, n)) return rc;
  return 0;
}

// Strict calls without a committee cache: the paired pipeline.  Chunks alternate between the
// device stream and the side stream, each launch on its own half of the table slots with its own
// fallback count and list region (PairLaunch), so chunk k + 1's blocks take the slots chunk k's
// drain frees instead of waiting for its last block, and the first chunk can be small
// (NWC_HOST_PAIR_FIRST, 65,536 equations = 8 MB of inputs, then x NWC_HOST_PAIR_GROWTH = 2).
// The fallback passes run once the streams have joined.  NWC_HOST_PAIR=0: the single-stream
// chunks (verify_chunked, A/B).
int verify_paired(DevCtx& d, const HostCall& c, std::vector<uint64_t>& out_words) {
  const nwc::plan::Settings& st = settings();
  const uint64_t n = c.n;
  if (int rc = ensure_stager(d)) return rc;
  if (int rc = ensure_verify_tables(d)) return rc;
  if (int rc = release_idle_buffers(d, d.pair_buf)) return rc;
  d.stager->reset();
  const auto tv0 = std::chrono::steady_clock::now();
  const std::vector<uint64_t> cuts = nwc::plan::chunk_cuts(n, st.host_pair_first, st.host_pair_growth, st.host_pair_max);
  const uint64_t nch = cuts.size() - 1;
  if (int rc = ensure_events(d.ev_chunk, nch)) return rc;
  // slots, lists and the per-chunk counts and list regions sized once, before any launch: inside
  // the pipeline nothing is reallocated under a running chunk (hold_lists: no shrink either)
  const uint64_t gcap = (uint64_t)d.cus * d.verify_blocks_per_cu * NWC_VERIFY_GRID_MULT;
  if (int rc = ensure_scratch(d, (size_t)gcap * 256 * 2 * nwc::TAB_BYTES_PER_LANE, nwc::plan::longest_chunk(cuts))) return rc;
  const size_t counts_bytes = align256(4 * nch), pair_need = counts_bytes + 4 * n;
  if (int rc = ensure_idle(d, d.pair_buf, pair_need, nullptr)) return rc;
  uint32_t* const counts = reinterpret_cast<uint32_t*>(d.pair_buf.get());
  uint32_t* const lists = reinterpret_cast<uint32_t*>(d.pair_buf + counts_bytes);
  struct Hold {
    DevCtx& d;
    ~Hold() {
      d.hold_lists = false;
      d.busy_buf = nullptr;
    }
  } hold{d};
  d.hold_lists = true;
  d.busy_buf = d.pair_buf;
  // the previous call's kernels may still read the arena and the slots: the copies wait for the
  // device stream, both compute streams for scratch_free
  HIP_TRY(hipEventRecord(d.ev_fork, d.stream));
  HIP_TRY(hipStreamWaitEvent(d.xfer, d.ev_fork, 0));
  HIP_TRY(hipStreamWaitEvent(d.side, d.ev_fork, 0));
  HIP_TRY(hipStreamWaitEvent(d.stream, d.scratch_free, 0));
  HIP_TRY(hipStreamWaitEvent(d.side, d.scratch_free, 0));
  if (!c.msg_stride) HIP_TRY(d.stager->put(c.dm, c.msgs, 32));
  for (uint64_t k = 0; k < nch; ++k) {
    const uint64_t c0 = cuts[k], len = cuts[k + 1] - cuts[k];
    if (int rc = stage_chunk(d, c, c0, len, d.ev_chunk[k])) return rc;
    const hipStream_t sk = (k & 1) ? d.side : d.stream;
    HIP_TRY(hipStreamWaitEvent(sk, d.ev_chunk[k], 0));
    const PairLaunch pl{(int)(k & 1), lists + c0, counts + k};
    VerifyLaunch q = c.launch(c0, len, sk);
    q.pair = &pl;
    if (int rc = launch_verify(d, q)) return rc;
  }
  HIP_TRY(hipEventRecord(d.ev_join, d.side));
  HIP_TRY(hipStreamWaitEvent(d.stream, d.ev_join, 0));
  // every chunk's failed reductions (rare: waves exit at once on an empty list)
  for (uint64_t k = 0; k < nch; ++k) {
    const uint64_t c0 = cuts[k], len = cuts[k + 1] - cuts[k];
    const nwc::VerifyArgs a{c.msg_stride ? c.dm + 32 * c0 : c.dm, nullptr, c.msg_stride ? 1u : 0u, c.dp + 32 * c0, c.ds + 64 * c0,
                            c.dout + c0 / 64, len, c.strict, d.base_table, d.base24, d.scratch, lists + c0, counts + k,
                            0u, nwc::Committee{}};
    hipLaunchKernelGGL(nwc::k_verify_fallback, dim3(16), dim3(256), 0, d.stream, a);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(d.scratch_free, d.stream));
  return collect_words(d, c, out_words, " (paired)", nch, tv0);
}

// Pipelined: inputs of chunk k on the transfer stream, its verification on the device stream
// after the chunk's event; every chunk has its own region of the arena (no reuse hazards).
// Chunk k + 1 is up to NWC_HOST_CHUNK_GROWTH x chunk k: its 128 B per equation cross PCIe
// (~50 GB/s) while chunk k verifies (~100 M/s), so it arrives in time while growing up to ~3.7x;
// fewer, larger launches leave fewer kernel tails (the first chunk is one round of resident
// lanes).  Chunks stop growing at NWC_HOST_CHUNK_MAX equations: when the kernels keep pace with
// the copies (the comb kernel: ~640 M votes/s against ~600 M votes/s of inputs through the stages)
// a huge last chunk would start only once all its inputs are in and run alone at the end.
int verify_chunked(DevCtx& d, const HostCall& c, std::vector<uint64_t>& out_words) {
  const nwc::plan::Settings& st = settings();
  if (int rc = ensure_stager(d)) return rc;
  HostStager* const hs = d.stager.get();
  hs->reset();
  const auto tv0 = std::chrono::steady_clock::now();
  const std::vector<uint64_t> cuts = nwc::plan::chunk_cuts(c.n, st.host_chunk, st.host_chunk_growth, st.host_chunk_max);
  const uint64_t nch = cuts.size() - 1;
  if (int rc = ensure_events(d.ev_chunk, nch)) return rc;
  // Chunks on the comb path (launch keys or the committee cache) defer their sign tests: a
  // lane gets ~8 votes of a 1M-vote chunk, and its one inversion would be ~9 % of each vote's
  // work (k_verify_comb_y; the sign pass of chunk k runs in the first blocks of chunk k + 1's
  // launch, the last one alone; SignRecs of two chunks alternate in sign_buf)
  const uint64_t maxlen = nwc::plan::longest_chunk(cuts);
  const bool ysplit = !c.strict && st.sign_defer;
  nwc::SignRecs reg[2] = {};
  if (ysplit) {
    if (int rc = release_idle_buffers(d, d.sign_buf)) return rc;
    const size_t need_s = 2 * (3 * align256(32 * maxlen) + align256(4 * maxlen));
    if (int rc = ensure_idle(d, d.sign_buf, need_s, nullptr)) return rc;
    Carve cs(d.sign_buf);
    for (auto& r : reg) {
      r.x = cs.take<uint32_t>(32 * maxlen);
      r.z = cs.take<uint32_t>(32 * maxlen);
      r.p = cs.take<uint32_t>(32 * maxlen);
      r.meta = cs.take<uint32_t>(4 * maxlen);
    }
  }
  uint64_t owed_c0 = 0, owed_len = 0;   // the chunk whose sign tests are still to run
  int owed_reg = 0;
  struct Busy {
    DevCtx& d;
    ~Busy() { d.busy_buf = nullptr; }
  } busy{d};
  d.busy_buf = d.sign_buf;
  // the previous call's kernels may still read the arena: the transfers wait for the stream
  HIP_TRY(hipEventRecord(d.ev_fork, d.stream));
  HIP_TRY(hipStreamWaitEvent(d.xfer, d.ev_fork, 0));
  if (c.batch()) {
    // digests and offsets first; the vote index is built on the device behind them, so chunk 0's
    // event (recorded later on the same stream) covers it
    HIP_TRY(hs->put(c.dm, c.msgs, c.msg_bytes));
    HIP_TRY(hs->put(reinterpret_cast<uint8_t*>(c.doffs), reinterpret_cast<const uint8_t*>(c.cert_offsets + c.c_lo), c.offs_bytes));
    HIP_TRY(hs->flush());
    launch_cert_index(c.doffs, c.c_lo, c.c_end, c.lo, c.lo + c.n, c.dmi, d.xfer);
    HIP_TRY(hipGetLastError());
  } else if (!c.msg_stride) {
    HIP_TRY(hs->put(c.dm, c.msgs, 32));
  }
  for (uint64_t k = 0; k < nch; ++k) {
    const uint64_t c0 = cuts[k], len = cuts[k + 1] - cuts[k];
    if (int rc = stage_chunk(d, c, c0, len, d.ev_chunk[k])) return rc;
    HIP_TRY(hipStreamWaitEvent(d.stream, d.ev_chunk[k], 0));
    const nwc::SignPass sp{sign_recs_at(reg[owed_reg], -(int64_t)owed_c0), owed_c0, owed_len, c.dout,
                           comb_sign_blocks(d, owed_len)};
    const bool y = ysplit && takes_comb_path(d, len, c.strict);
    if (!y && owed_len) {
      if (int rc = launch_comb_sign(d, sp.rec, owed_c0, owed_len, c.dout, d.stream)) return rc;
      owed_len = 0;
    }
    const int r = (int)(k & 1);
    VerifyLaunch q = c.launch(c0, len, d.stream);
    q.sign_recs = y ? &reg[r] : nullptr;
    q.sign_pass = y && owed_len ? &sp : nullptr;
    if (int rc = launch_verify(d, q)) return rc;
    if (y) {
      owed_c0 = c0;
      owed_len = len;
      owed_reg = r;
    }
  }
  if (owed_len)
    if (int rc = launch_comb_sign(d, sign_recs_at(reg[owed_reg], -(int64_t)owed_c0), owed_c0, owed_len, c.dout, d.stream))
      return rc;
  return collect_words(d, c, out_words, "", nch, tv0);
}

// One copy of everything, one launch, one copy back.
int verify_direct(DevCtx& d, const HostCall& c, std::vector<uint64_t>& out_words) {
  if (c.batch()) {
    HIP_TRY(hipMemcpyAsync(c.dm, c.msgs, c.msg_bytes, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(c.doffs, c.cert_offsets + c.c_lo, c.offs_bytes, hipMemcpyHostToDevice, d.stream));
    launch_cert_index(c.doffs, c.c_lo, c.c_end, c.lo, c.lo + c.n, c.dmi, d.stream);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemcpyAsync(c.dm, c.msgs + (c.msg_stride ? 32 * c.lo : 0), c.msg_bytes, hipMemcpyHostToDevice, d.stream));
  }
  HIP_TRY(hipMemcpyAsync(c.dp, c.pks + 32 * c.lo, 32 * c.n, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(hipMemcpyAsync(c.ds, c.sigs + 64 * c.lo, 64 * c.n, hipMemcpyHostToDevice, d.stream));
  if (int rc = launch_verify(d, c.launch(0, c.n, d.stream))) return rc;
  HIP_TRY(hipMemcpyAsync(out_words.data(), c.dout, 8 * c.words, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(hipStreamSynchronize(d.stream));
  return 0;
}

// Host-memory verification of equations [lo, hi) on device di: the arena carved for them, then the
// pipeline their size and kind call for.
int verify_range(int di, const uint8_t* msgs, uint64_t msg_stride, const uint32_t* cert_offsets,
                 const uint8_t* pks, const uint8_t* sigs, uint64_t lo, uint64_t hi, int strict,
                 std::vector<uint64_t>& out_words, uint64_t nmsgs) {
  DevCtx& d = *ctx(di);
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  const uint64_t n = hi - lo;
  const uint64_t words = (n + 63) / 64;
  out_words.assign(words, 0);
  if (n == 0) return 0;
  HostCall c{msgs, msg_stride, cert_offsets, pks, sigs, lo, n, words, nmsgs, strict};
  const bool batch = c.batch();
  if (batch) cert_span(cert_offsets, nmsgs, lo, hi, c.c_lo, c.c_end);
  c.msg_bytes = batch ? 32 * nmsgs : (msg_stride ? 32 * n : 32);
  c.need = align256(c.msg_bytes) + align256(batch ? 4 * n : 0) + align256(32 * n) + align256(64 * n) + align256(8 * (words + 1));
  c.offs_bytes = batch ? 4 * (c.c_end - c.c_lo + 1) : 0;
  if (int rc = d.ensure_arena(c.need + align256(c.offs_bytes))) return rc;
  Carve cv(d.arena);
  c.dm = cv.take<uint8_t>(c.msg_bytes);
  c.dmi = batch ? cv.take<uint32_t>(4 * n) : nullptr;
  c.dp = cv.take<uint8_t>(32 * n);
  c.ds = cv.take<uint8_t>(64 * n);
  c.dout = cv.take<uint64_t>(8 * (words + 1));
  c.doffs = batch ? cv.take<uint32_t>(c.offs_bytes) : nullptr;
  const nwc::plan::Settings& st = settings();
  if (c.need <= NWC_PINNED_STAGE_MAX) return verify_small(d, c, out_words);
  if (st.host_pair && strict && !batch && st.verify_path == VPath::Default && !d.cm_n && n >= 2 * st.host_pair_first &&
      n <= st.verify_max_launch)
    return verify_paired(d, c, out_words);
  if (st.host_chunk && n >= 2 * st.host_chunk) return verify_chunked(d, c, out_words);
  return verify_direct(d, c, out_words);
}

// A per-launch device buffer of the batch entries (MSM, Straus, resolve), grown on demand and
// shrunk back when it holds more than NWC_VERIFY_KEEP_BYTES and a launch needs under a quarter of
// it (a primary and workers share the GPU: worker/src/worker.rs:182,227), after the other idle
// ones above that threshold have gone.
int ensure_batch_buf(DevCtx& d, Buf<uint8_t>& b, size_t need, hipStream_t s) {
  if (int rc = release_idle_buffers(d, b)) return rc;
  return ensure_idle(d, b, need, &s, 0, settings().verify_keep_bytes);
}

// The per-launch z_i seed: 32 bytes from the host's CSPRNG (dalek: merlin transcript + thread_rng),
// or the test knob's fixed value (nwc_diag_set("dalek_seed")).
void draw_seed(uint32_t seed[8]) {
  const uint64_t fixed = knobs().dalek_seed.load();
  if (fixed) {
    for (int i = 0; i < 8; ++i) seed[i] = i == 0 ? (uint32_t)fixed : 0u;
    return;
  }
  static thread_local std::random_device rd;
  for (int i = 0; i < 8; ++i) seed[i] = rd();
}

// dalek's batch equation over sub-batches (k_verify_straus) + the exact leaves for the failing
// sub-batches, on d's stream s: leaf words (a bit per vote) for cert_reduce.  Caller holds d.mu
// and has set the device.
int launch_straus(DevCtx& d, const uint8_t* dig, const uint32_t* mi, const uint8_t* pks, const uint8_t* sigs,
                  uint64_t nvotes, uint64_t* leaf, hipStream_t s) {
  if (nvotes == 0) return 0;
  if (int rc = ensure_verify_tables(d)) return rc;
  if (nvotes > settings().verify_max_launch) {
    // consecutive launches of at most NWC_VERIFY_MAX_LAUNCH votes, as launch_verify: sub-batches
    // are any consecutive votes (each reads its own certificate's digest through mi)
    const uint64_t step = settings().verify_max_launch;
    for (uint64_t lo = 0; lo < nvotes; lo += step)
      if (int rc = launch_straus(d, dig, mi + lo, pks + 32 * lo, sigs + 64 * lo, std::min(step, nvotes - lo), leaf + lo / 64, s))
        return rc;
    return 0;
  }
  if (!d.comb16)   // no basepoint comb (NWC_COMB16=0): the exact leaves
    return launch_verify(d, {.msgs = dig, .msg_index = mi, .pks = pks, .sigs = sigs, .n = nvotes, .out_words = leaf, .stream = s});
  // sub-batches of ~12 votes (knobs().straus_nq), every lane slot the same number of rounds
  const uint32_t target = knobs().straus_nq.load();
  const uint64_t resident = (uint64_t)d.cus * nwc::STRAUS_WAVES_PER_SIMD * 256;
  const uint64_t runs = nwc::straus_runs(nvotes, resident, target);
  const uint64_t lanes = std::min<uint64_t>((runs + 255) / 256 * 256, resident);
  const uint64_t maxq = (nvotes + runs - 1) / runs;
  const uint64_t stride = maxq * nwc::STRAUS_VOTE_BYTES;
  if (int rc = ensure_batch_buf(d, d.straus_scratch, lanes * stride, s)) return rc;
  // the failing sub-batches' leaves: the list-mode leaf kernel's scratch and lists
  const uint64_t lgrid = (uint64_t)d.cus * d.verify_blocks_per_cu;
  if (int rc = ensure_scratch(d, (size_t)lgrid * 256 * 2 * nwc::TAB_BYTES_PER_LANE, nvotes)) return rc;
  HIP_TRY(hipStreamWaitEvent(s, d.scratch_free, 0));
  nwc::StrausArgs sa{};
  sa.digests = dig; sa.msg_index = mi; sa.pks = pks; sa.sigs = sigs; sa.nv = nvotes; sa.runs = runs;
  draw_seed(sa.seed);
  sa.comb16 = d.comb16; sa.scratch = d.straus_scratch; sa.lane_stride = stride;
  sa.leaf_words = leaf; sa.list = d.uc_list; sa.count = d.uc_count;
  HIP_TRY(hipMemsetAsync(leaf, 0, 8 * ((nvotes + 63) / 64), s));
  HIP_TRY(hipMemsetAsync(d.uc_count, 0, sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(d.fb_count, 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(nwc::k_verify_straus<false>, dim3((unsigned)(lanes / 256)), dim3(256), 0, s, sa);
  HIP_TRY(hipGetLastError());
  nwc::VerifyArgs a{dig, mi, 0, pks, sigs, leaf, nvotes, 0, d.base_table, d.base24, d.scratch, d.fb_list,
                    d.fb_count, 0u, nwc::Committee{}};
  const nwc::CombArgs ca{d.uc_list, d.uc_count, d.comb_base, d.comb16};
  hipLaunchKernelGGL((nwc::k_verify<true, false, true>), dim3((unsigned)lgrid), dim3(256), 0, s, a, ca);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(nwc::k_verify_fallback, dim3(16), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  if (int rc = launch_torsion(d, pks, leaf, nvotes, d.uc_list, d.uc_count, nwc::Committee{}, s)) return rc;
  HIP_TRY(hipEventRecord(d.scratch_free, s));
  return 0;
}


// dalek's batch equation over groups of consecutive votes as a Pippenger MSM with a wavefront-level
// bucket reduction (k_verify_msm, msm.h) + the exact leaves for the groups it rejects, on d's
// stream s: leaf words (a bit per vote) for cert_reduce, like launch_straus.  Caller holds d.mu and
// has set the device.
int launch_msm(DevCtx& d, const uint8_t* dig, const uint32_t* mi, const uint8_t* pks, const uint8_t* sigs,
               uint64_t nvotes, uint64_t* leaf, hipStream_t s) {
  if (nvotes == 0) return 0;
  if (int rc = ensure_verify_tables(d)) return rc;
  if (nvotes > settings().verify_max_launch) {
    const uint64_t step = settings().verify_max_launch;
    for (uint64_t lo = 0; lo < nvotes; lo += step)
      if (int rc = launch_msm(d, dig, mi + lo, pks + 32 * lo, sigs + 64 * lo, std::min(step, nvotes - lo), leaf + lo / 64, s))
        return rc;
    return 0;
  }
  if (!d.comb16)   // no basepoint comb (NWC_COMB16=0): the exact leaves
    return launch_verify(d, {.msgs = dig, .msg_index = mi, .pks = pks, .sigs = sigs, .n = nvotes, .out_words = leaf, .stream = s});
  static int bpc = [] {
    int b = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, reinterpret_cast<const void*>(nwc::k_verify_msm), 64, 0);
    return b > 0 ? b : 1;
  }();
  const uint64_t slots = (uint64_t)d.cus * bpc;   // resident waves (one group each at a time)
  uint32_t group = knobs().msm_group.load();
  if (group == 0) {
    // as few rounds of the resident waves as groups of <= MSM_GMAX allow, every round full: the
    // per-window costs of a group (scan, doublings, key points) amortise over larger groups, and a
    // partial last round would leave waves idle
    const uint64_t rounds = (nvotes + slots * nwc::MSM_GMAX - 1) / (slots * nwc::MSM_GMAX);
    group = (uint32_t)((nvotes + slots * rounds - 1) / (slots * rounds));
  }
  group = std::min<uint32_t>(nwc::MSM_GMAX, std::max<uint32_t>(64, (group + 63) / 64 * 64));
  const uint64_t groups = (nvotes + group - 1) / group;
  const uint64_t grid = std::min<uint64_t>(groups, slots);
  // per-wave points and digits, then the failing groups' vote list (count word, entries)
  const size_t list_off = align256((size_t)grid * nwc::MSM_WAVE_BYTES);
  const size_t need = list_off + 256 + 4 * nvotes;
  if (int rc = ensure_batch_buf(d, d.msm_scratch, need, s)) return rc;
  if (!d.msm_stats) {
    HIP_TRY(d.msm_stats.alloc(4 * nwc::MSM_ST_WORDS));
    HIP_TRY(hipMemsetAsync(d.msm_stats, 0, 4 * nwc::MSM_ST_WORDS, s));
  }
  uint32_t* const mcount = reinterpret_cast<uint32_t*>(d.msm_scratch + list_off);
  uint32_t* const mlist = mcount + 64;
  // the failing groups' votes go straight to the exact leaves (list mode): a vote meets at most one
  // random equation, its group's
  const uint64_t lgrid = (uint64_t)d.cus * d.verify_blocks_per_cu;
  if (int rc = ensure_scratch(d, (size_t)lgrid * 256 * 2 * nwc::TAB_BYTES_PER_LANE, nvotes)) return rc;
  HIP_TRY(hipStreamWaitEvent(s, d.scratch_free, 0));
  nwc::MsmArgs ma{};
  ma.digests = dig; ma.msg_index = mi; ma.pks = pks; ma.sigs = sigs; ma.nv = nvotes; ma.group = group;
  draw_seed(ma.seed);
  ma.comb16 = d.comb16; ma.scratch = d.msm_scratch;
  ma.leaf_words = leaf; ma.list = mlist; ma.count = mcount; ma.stats = d.msm_stats;
  // the policy off holds for this launch too: a mode an earlier launch armed is not obeyed, and
  // k_msm_policy clears it below
  const uint32_t adapt = knobs().msm_adapt.load();
  ma.adapt = adapt;
  HIP_TRY(hipMemsetAsync(leaf, 0, 8 * ((nvotes + 63) / 64), s));
  HIP_TRY(hipMemsetAsync(mcount, 0, sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(d.fb_count, 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(nwc::k_verify_msm, dim3((unsigned)grid), dim3(64), 0, s, ma);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(nwc::k_msm_policy, dim3(1), dim3(64), 0, s, d.msm_stats, adapt);
  HIP_TRY(hipGetLastError());
  const nwc::VerifyArgs a{dig, mi, 0, pks, sigs, leaf, nvotes, 0, d.base_table, d.base24, d.scratch, d.fb_list,
                          d.fb_count, 0u, nwc::Committee{}};
  const nwc::CombArgs ca{mlist, mcount, d.comb_base, d.comb16};
  hipLaunchKernelGGL((nwc::k_verify<true, false, true>), dim3((unsigned)lgrid), dim3(256), 0, s, a, ca);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(nwc::k_verify_fallback, dim3(16), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  if (int rc = launch_torsion(d, pks, leaf, nvotes, mlist, mcount, nwc::Committee{}, s)) return rc;
  HIP_TRY(hipEventRecord(d.scratch_free, s));
  return 0;
}

// dalek's batch equation per certificate over the votes the leaves rejected (resolve.h), on s after
// the leaves wrote `leaf` (bit per vote of m certificates): cm = the key set whose combs the leaves
// used (nullptr combs: the ladder).  Sets the bits of the failing votes of certificates the equation
// accepts.  Caller holds d.mu and has set the device.
int launch_resolve(DevCtx& d, const uint8_t* dig, const uint32_t* mi, uint64_t m, const uint8_t* pks,
                   const uint8_t* sigs, uint64_t nv, uint64_t* leaf, const nwc::Committee& cm, hipStream_t s) {
  if (nv == 0) return 0;
  if (nv > 0xFFFFFFFFull || m > 0xFFFFFFFFull) return set_err(NWC_ERR_ARG, "more than 2^32 - 1 votes or certificates");
  const size_t state_off = align256(256 + 4 * (size_t)nv);
  if (int rc = ensure_batch_buf(d, d.rs_buf, state_off + align256(4 * (size_t)m), s)) return rc;
  // one lane per failing vote; a lane slot's ladder table lives in the verification scratch
  const uint64_t grid = (uint64_t)d.cus * d.verify_blocks_per_cu;
  if (int rc = ensure_scratch(d, (size_t)grid * 256 * 2 * nwc::TAB_BYTES_PER_LANE, std::min(nv, settings().verify_max_launch)))
    return rc;
  HIP_TRY(hipStreamWaitEvent(s, d.scratch_free, 0));
  uint32_t* const count = reinterpret_cast<uint32_t*>(d.rs_buf.get());
  uint32_t* const list = count + 64;
  uint32_t* const state = reinterpret_cast<uint32_t*>(d.rs_buf + state_off);
  HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(state, 0, 4 * (size_t)m, s));
  const uint64_t words = (nv + 63) / 64;
  hipLaunchKernelGGL(nwc::k_list_failing, dim3((unsigned)std::min<uint64_t>((words + 255) / 256, (uint64_t)d.cus * 8)),
                     dim3(256), 0, s, leaf, nv, list, count);
  HIP_TRY(hipGetLastError());
  nwc::ResolveArgs ra{};
  ra.digests = dig; ra.msg_index = mi; ra.pks = pks; ra.sigs = sigs; ra.list = list; ra.count = count;
  draw_seed(ra.seed);
  ra.cm = cm; ra.comb16 = d.comb16; ra.base_table = d.base_table; ra.scratch = d.scratch;
  ra.cert_state = state; ra.leaf_words = leaf;
  hipLaunchKernelGGL(nwc::k_vote_resolve, dim3((unsigned)grid), dim3(256), 0, s, ra);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(nwc::k_resolve_apply, dim3((unsigned)(d.cus * 2)), dim3(256), 0, s, ra);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(d.scratch_free, s));
  return 0;
}

// Signature::verify_batch over m certificates with dalek's batch semantics (crypto/src/lib.rs:218).
// Where key combs apply (a committee cache with combs, or a launch large enough for launch keys):
// the exact per-vote leaves on the comb path, then dalek's equation once per certificate over the
// votes they rejected (launch_resolve) -- every vote meets one random equation, its certificate's.
// Otherwise the Pippenger groups first (launch_msm).  Caller holds d.mu and has set the device.
int launch_batch_dalek(DevCtx& d, const uint8_t* dig, const uint32_t* mi, uint64_t m, const uint8_t* pks,
                       const uint8_t* sigs, uint64_t nv, uint64_t* leaf, hipStream_t s) {
  if (nv == 0) return 0;
  if (int rc = ensure_verify_tables(d)) return rc;
  const bool committee = d.cm_n && d.cm_comb;
  const bool lkeys = !d.cm_n && nv >= nwc::LK_MIN_EQUATIONS && knobs().launch_keys.load();
  if (settings().verify_path != VPath::Default || !d.comb16 || !(committee || lkeys))
    return launch_msm(d, dig, mi, pks, sigs, nv, leaf, s);
  if (int rc = launch_verify(d, {.msgs = dig, .msg_index = mi, .pks = pks, .sigs = sigs, .n = nv, .out_words = leaf, .stream = s}))
    return rc;
  return launch_resolve(d, dig, mi, m, pks, sigs, nv, leaf, committee ? committee_of(d) : launch_committee_of(d), s);
}

// Per-vote leaf bits of every device's share (whole certificates) -> certificate verdicts and the
// bad-vote bitmap (a certificate passes iff every vote's bit is set; an empty one passes).
int batch_verdicts(const uint32_t* offsets, size_t m, const std::vector<uint64_t>& cuts,
                   const std::vector<std::vector<uint64_t>>& parts, uint8_t* cert_ok_bitmap, uint8_t* bad_vote_bitmap) {
  // word-level: a certificate is ok iff every bit of its vote range is set (two masked words for a
  // 67-vote certificate), and the bad-vote bitmap is the complement of the leaf bits
  const uint64_t nv = offsets[m];
  std::vector<uint64_t> leafw((nv + 63) / 64 + 1, 0);
  uint8_t* const leafbytes = reinterpret_cast<uint8_t*>(leafw.data());
  for (size_t i = 0; i + 1 < cuts.size(); ++i) merge_bits(leafbytes, cuts[i], parts[i], cuts[i + 1] - cuts[i]);
  std::memset(cert_ok_bitmap, 0, (m + 7) / 8);
  for (size_t c = 0; c < m; ++c) {
    const uint64_t a = offsets[c], e = offsets[c + 1];
    bool ok = true;
    if (e > a) {
      const uint64_t w0 = a >> 6, w1 = (e - 1) >> 6;
      for (uint64_t w = w0; w <= w1 && ok; ++w) {
        uint64_t mask = ~0ull;
        if (w == w0) mask &= ~0ull << (a & 63);
        if (w == w1) mask &= ~0ull >> (63 - ((e - 1) & 63));
        ok = (leafw[w] & mask) == mask;
      }
    }
    if (ok) cert_ok_bitmap[c >> 3] |= (uint8_t)(1u << (c & 7));
  }
  if (bad_vote_bitmap && nv) {
    const uint64_t full = nv / 8;
    for (uint64_t i = 0; i < full; ++i) bad_vote_bitmap[i] = (uint8_t)~leafbytes[i];
    for (uint64_t v = full * 8; v < nv; ++v) {
      const bool bad = !((leafbytes[v >> 3] >> (v & 7)) & 1);
      bad_vote_bitmap[v >> 3] = (uint8_t)((bad_vote_bitmap[v >> 3] & ~(1u << (v & 7))) | ((unsigned)bad << (v & 7)));
    }
  }
  return 0;
}

// One device's share of nwc_verify_batch_straus_many: votes [lo, hi) (whole certificates) staged
// into the arena with one H2D each, the Straus launch, one D2H of the leaf words.
int straus_range(int di, const uint8_t* digests, size_t m, const uint32_t* offsets, const uint8_t* pks,
                 const uint8_t* sigs, uint64_t lo, uint64_t hi, std::vector<uint64_t>& out_words, bool msm = false) {
  DevCtx& d = *ctx(di);
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  const uint64_t n = hi - lo;
  const uint64_t words = (n + 63) / 64;
  out_words.assign(words, 0);
  if (n == 0) return 0;
  uint64_t c_lo, c_end;
  cert_span(offsets, m, lo, hi, c_lo, c_end);
  const size_t offs_bytes = 4 * (c_end - c_lo + 1);
  const size_t need = align256(32 * m) + align256(4 * n) + align256(32 * n) + align256(64 * n) + align256(8 * words) +
                      align256(offs_bytes);
  if (int rc = d.ensure_arena(need)) return rc;
  Carve c(d.arena);
  uint8_t* dm = c.take<uint8_t>(32 * m);
  uint32_t* dmi = c.take<uint32_t>(4 * n);
  uint8_t* dp = c.take<uint8_t>(32 * n);
  uint8_t* ds = c.take<uint8_t>(64 * n);
  uint64_t* dout = c.take<uint64_t>(8 * words);
  uint32_t* doffs = c.take<uint32_t>(offs_bytes);
  HIP_TRY(hipMemcpyAsync(dm, digests, 32 * m, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(hipMemcpyAsync(doffs, offsets + c_lo, offs_bytes, hipMemcpyHostToDevice, d.stream));
  launch_cert_index(doffs, c_lo, c_end, lo, hi, dmi, d.stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(dp, pks + 32 * lo, 32 * n, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(hipMemcpyAsync(ds, sigs + 64 * lo, 64 * n, hipMemcpyHostToDevice, d.stream));
  if (int rc = msm ? launch_batch_dalek(d, dm, dmi, m, dp, ds, n, dout, d.stream)
                   : launch_straus(d, dm, dmi, dp, ds, n, dout, d.stream))
    return rc;
  HIP_TRY(hipMemcpyAsync(out_words.data(), dout, 8 * words, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(hipStreamSynchronize(d.stream));
  return 0;
}

}  // namespace

extern "C" {

int nwc_shard_bounds(uint64_t n, uint32_t world, uint32_t rank, uint64_t* lo, uint64_t* hi) {
  if (!lo || !hi || world == 0 || rank >= world) return set_err(NWC_ERR_ARG, "bad shard arguments");
  const uint64_t words = (n + 63) / 64, per = (words + world - 1) / world;
  *lo = std::min<uint64_t>(n, (uint64_t)rank * per * 64);
  *hi = std::min<uint64_t>(n, ((uint64_t)rank + 1) * per * 64);
  return 0;
}

int nwc_cert_cuts(const uint32_t* offsets, size_t m, uint32_t world, uint64_t* cuts) {
  if (!offsets || !cuts || world == 0) return set_err(NWC_ERR_ARG, "bad cut arguments");
  const uint64_t nv = offsets[m];
  cuts[0] = 0;
  size_t c = 0;
  for (uint32_t r = 1; r < world; ++r) {
    const uint64_t target = nv * r / world;
    while (c < m && offsets[c] < target) ++c;   // first boundary at or past the target
    cuts[r] = offsets[c];
  }
  cuts[world] = nv;
  return 0;
}

int nwc_version(void) { return (1 << 16) | 2; }

#ifndef NWC_BUILD_ID
#define NWC_BUILD_ID "unknown"
#endif
// "NWC_BUILD_ID:" + the hash narwhal_amd/build.py takes over the sources and flags; build.py finds
// it in the .so's bytes to decide whether the library is HEAD's.
static const char k_build_id[] = "NWC_BUILD_ID:" NWC_BUILD_ID;
const char* nwc_build_id(void) { return k_build_id + 13; }

int nwc_diag_set(const char* name, int64_t value) {
  if (!name) return set_err(NWC_ERR_ARG, "null knob name");
  if (value < 0 || value > 0xFFFFFFFFll) return set_err(NWC_ERR_ARG, "knob value out of range");
  if (std::strcmp(name, "straus_nq") == 0) {
    if (value < 1 || value > nwc::STRAUS_MAX_PER_LANE) return set_err(NWC_ERR_ARG, "straus_nq must be in [1, %d]", nwc::STRAUS_MAX_PER_LANE);
    knobs().straus_nq = (uint32_t)value;
  } else if (std::strcmp(name, "msm_group") == 0) {
    if (value != 0 && (value < 64 || value > nwc::MSM_GMAX || value % 64))
      return set_err(NWC_ERR_ARG, "msm_group must be 0 (sized per launch) or a multiple of 64 in [64, %d]", nwc::MSM_GMAX);
    knobs().msm_group = (uint32_t)value;
  } else if (std::strcmp(name, "msm_adapt") == 0) {
    if (value > 1) return set_err(NWC_ERR_ARG, "msm_adapt must be 0 or 1");
    knobs().msm_adapt = (uint32_t)value;
  } else if (std::strcmp(name, "dalek_seed") == 0) {
    knobs().dalek_seed = (uint64_t)value;
  } else if (std::strcmp(name, "sanitizer_redo_every") == 0) {
    knobs().sanitizer_redo_every = (uint32_t)value;
  } else if (std::strcmp(name, "sign_path") == 0) {
    if (value > 2) return set_err(NWC_ERR_ARG, "sign_path must be 0 (by size), 1 (k_sign) or 2 (k_sign_wide)");
    knobs().sign_path = (uint32_t)value;
  } else if (std::strcmp(name, "launch_keys") == 0) {
    if (value > 1) return set_err(NWC_ERR_ARG, "launch_keys must be 0 or 1");
    knobs().launch_keys = (uint32_t)value;
  } else if (std::strcmp(name, "force_windows") == 0) {
    if (value != 0 && (value < nwc::HALF_WINDOWS_MIN || value > nwc::HALF_WINDOWS_MAX))
      return set_err(NWC_ERR_ARG, "force_windows must be 0 or in [%d, %d]", nwc::HALF_WINDOWS_MIN, nwc::HALF_WINDOWS_MAX);
    knobs().force_windows = (uint32_t)value;
  } else {
    return set_err(NWC_ERR_ARG, "unknown knob '%s'", name);
  }
  return 0;
}

const char* nwc_last_error(void) { return t_err.c_str(); }

int nwc_init(uint32_t device_mask) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_devs.empty()) return 0;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0)
    return set_err(NWC_ERR_NO_DEVICE, "no HIP device visible (%s)", hipGetErrorString(e));
  if (device_mask == 0) device_mask = 1;
  for (int i = 0; i < count && i < 32; ++i) {
    if (!((device_mask >> i) & 1)) continue;
    auto d = std::make_unique<DevCtx>();
    d->hip_id = i;
    if (int rc = init_device(*d)) { g_devs.clear(); return rc; }
    g_devs.push_back(std::move(d));
  }
  if (g_devs.empty()) return set_err(NWC_ERR_NO_DEVICE, "device mask 0x%x selects no visible device", device_mask);
  // A process that exits without nwc_shutdown (a Python caller, a node killed by its runtime)
  // still releases every device object of the library -- streams synchronised, copies finished,
  // pinned stages and HBM freed -- before the HIP runtime's own exit-time teardown: atexit
  // handlers run in reverse order of registration, and this one is registered after the runtime
  // was initialised above.  nwc_shutdown is idempotent (the second call finds no context).
  static const bool at_exit = std::atexit([] { nwc_shutdown(); }) == 0;
  (void)at_exit;
  // Test hook: NWC_VIRTUAL_DEVICES=k opens k contexts (own stream, tables, buffers) on a single
  // selected GPU, so the multi-device host paths -- shard threads, certificate cuts, bitmap
  // merges -- run for real on a one-GPU box (tests/test_gpu_multidev.py).
  const char* ve = std::getenv("NWC_VIRTUAL_DEVICES");
  const int virt = ve ? std::atoi(ve) : 0;
  const bool single = g_devs.size() == 1;
  for (int k = 1; single && k < virt && k < 32; ++k) {
    auto d = std::make_unique<DevCtx>();
    d->hip_id = g_devs[0]->hip_id;
    if (int rc = init_device(*d)) { g_devs.clear(); return rc; }
    g_devs.push_back(std::move(d));
  }
  return 0;
}

void nwc_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  signers_shutdown();   // live signers' key records are zeroed and freed first
  verifiers_shutdown();  // live verifiers finish what is queued; their pinned group buffers go
  sanitizers_shutdown(); // and live sanitizers: their pinned group buffers and their HBM scratch
  for (auto& d : g_devs) {
    std::lock_guard<std::mutex> dl(d->mu);
    (void)hipSetDevice(d->hip_id);
    // every stream drained, then every buffer (plain frees, the stream-ordered blocks included),
    // then the events and streams
    for (hipStream_t st : {d->stream, d->side, d->xfer})
      if (st) (void)hipStreamSynchronize(st);
    (void)d->bufs.release_all();
    if (d->scratch_free) (void)hipEventDestroy(d->scratch_free);
    if (d->ev_fork) (void)hipEventDestroy(d->ev_fork);
    if (d->ev_join) (void)hipEventDestroy(d->ev_join);
    if (d->ev_msg) (void)hipEventDestroy(d->ev_msg);
    if (d->ev_count) (void)hipEventDestroy(d->ev_count);
    if (d->side) (void)hipStreamDestroy(d->side);
    if (d->stager) d->stager->release();
    d->stager.reset();
    for (hipEvent_t e : d->ev_chunk) (void)hipEventDestroy(e);
    for (hipEvent_t e : d->ev_cnt) (void)hipEventDestroy(e);
    if (d->xfer) (void)hipStreamDestroy(d->xfer);
    if (d->stream) (void)hipStreamDestroy(d->stream);
  }
  g_devs.clear();
}

int nwc_device_count(void) { return (int)g_devs.size(); }

int nwc_verify_strict_many(const uint8_t* msgs32, const uint8_t* pks, const uint8_t* sigs, size_t n,
                           uint8_t* verdict_bitmap) {
  if (int rc = require_init()) return rc;
  if (n && (!msgs32 || !pks || !sigs || !verdict_bitmap)) return set_err(NWC_ERR_ARG, "null buffer");
  // per-device verdict words are merged into the caller's bitmap on this thread, after the join
  std::vector<std::vector<uint64_t>> parts(g_devs.size());
  std::vector<std::pair<uint64_t, uint64_t>> range(g_devs.size(), {0, 0});
  if (int rc = shard(n, [&](int di, uint64_t lo, uint64_t hi) -> int {
        range[di] = {lo, hi};
        return verify_range(di, msgs32, 1, nullptr, pks, sigs, lo, hi, 1, parts[di], 0);
      }))
    return rc;
  for (size_t di = 0; di < parts.size(); ++di)
    if (range[di].second > range[di].first) merge_bits(verdict_bitmap, range[di].first, parts[di], range[di].second - range[di].first);
  return 0;
}

int nwc_verify_strict(const uint8_t msg32[32], const uint8_t pk[32], const uint8_t sig[64]) {
  uint8_t bit = 0;
  int rc = nwc_verify_strict_many(msg32, pk, sig, 1, &bit);
  if (rc < 0) return rc;
  return (bit & 1) ? NWC_OK : NWC_INVALID;
}

int nwc_verify_batch(const uint8_t msg32[32], const uint8_t* pks, const uint8_t* sigs, size_t n,
                     uint8_t* bad_bitmap) {
  if (int rc = require_init()) return rc;
  if (n == 0) return NWC_OK;  // empty iterator: dalek verify_batch of nothing is Ok
  if (!msg32 || !pks || !sigs) return set_err(NWC_ERR_ARG, "null buffer");
  std::vector<uint64_t> words;
  if (int rc = verify_range(t_dev < (int)g_devs.size() ? t_dev : 0, msg32, 0, nullptr, pks, sigs, 0, n, 0, words, 0))
    return rc;
  bool all = true;
  for (size_t i = 0; i < n; ++i) all = all && ((words[i >> 6] >> (i & 63)) & 1);
  if (bad_bitmap) {
    std::vector<uint64_t> bad(words.size());
    for (size_t w = 0; w < words.size(); ++w) bad[w] = ~words[w];
    merge_bits(bad_bitmap, 0, bad, n);
  }
  return all ? NWC_OK : NWC_INVALID;
}

int nwc_verify_batch_many(const uint8_t* digests, const uint32_t* offsets, const uint8_t* pks, const uint8_t* sigs,
                          size_t m, uint8_t* cert_ok_bitmap, uint8_t* bad_vote_bitmap) {
  if (int rc = require_init()) return rc;
  if (m == 0) return 0;
  if (!digests || !offsets || !cert_ok_bitmap) return set_err(NWC_ERR_ARG, "null buffer");
  if (offsets[0] != 0) return set_err(NWC_ERR_ARG, "offsets[0] must be 0");
  for (size_t c = 0; c < m; ++c)
    if (offsets[c + 1] < offsets[c]) return set_err(NWC_ERR_ARG, "offsets not monotone at %zu", c);
  const uint64_t nv = offsets[m];
  if (nv && (!pks || !sigs)) return set_err(NWC_ERR_ARG, "null vote buffer");
  // the vote -> certificate index is built per device range (k_cert_index; on the host for small calls)
  using clk = std::chrono::steady_clock;
  const auto t1 = clk::now();
  // shard votes on certificate boundaries
  const int nd = (int)g_devs.size();
  std::vector<uint64_t> cuts(nd + 1);
  nwc_cert_cuts(offsets, m, (uint32_t)nd, cuts.data());
  std::vector<int> rc(nd, 0);
  std::vector<std::vector<uint64_t>> parts(nd);
  std::vector<std::thread> th;
  for (int i = 0; i < nd; ++i) {
    th.emplace_back([&, i] {
      rc[i] = verify_range(i, digests, 0, offsets, pks, sigs, cuts[i], cuts[i + 1], 0, parts[i], m);
    });
  }
  for (auto& t : th) t.join();
  for (int r : rc) if (r < 0) return r;
  const auto t2 = clk::now();
  const int r = batch_verdicts(offsets, m, cuts, parts, cert_ok_bitmap, bad_vote_bitmap);
  if (settings().host_timing) {
    auto ms = [](clk::duration d) { return std::chrono::duration<double>(d).count() * 1e3; };
    std::fprintf(stderr, "nwc_verify_batch_many: %zu certificates, %llu votes: devices %.2f ms, verdicts %.2f ms\n",
                 m, (unsigned long long)nv, ms(t2 - t1), ms(clk::now() - t2));
  }
  return r;
}

static int batch_equation_many(const uint8_t* digests, const uint32_t* offsets, const uint8_t* pks, const uint8_t* sigs,
                               size_t m, uint8_t* cert_ok_bitmap, uint8_t* bad_vote_bitmap, bool msm);

int nwc_verify_batch_straus_many(const uint8_t* digests, const uint32_t* offsets, const uint8_t* pks,
                                 const uint8_t* sigs, size_t m, uint8_t* cert_ok_bitmap, uint8_t* bad_vote_bitmap) {
  return batch_equation_many(digests, offsets, pks, sigs, m, cert_ok_bitmap, bad_vote_bitmap, false);
}

int nwc_verify_batch_msm_many(const uint8_t* digests, const uint32_t* offsets, const uint8_t* pks,
                              const uint8_t* sigs, size_t m, uint8_t* cert_ok_bitmap, uint8_t* bad_vote_bitmap) {
  return batch_equation_many(digests, offsets, pks, sigs, m, cert_ok_bitmap, bad_vote_bitmap, true);
}

static int batch_equation_many(const uint8_t* digests, const uint32_t* offsets, const uint8_t* pks, const uint8_t* sigs,
                               size_t m, uint8_t* cert_ok_bitmap, uint8_t* bad_vote_bitmap, bool msm) {
  if (int rc = require_init()) return rc;
  if (m == 0) return 0;
  if (!digests || !offsets || !cert_ok_bitmap) return set_err(NWC_ERR_ARG, "null buffer");
  if (offsets[0] != 0) return set_err(NWC_ERR_ARG, "offsets[0] must be 0");
  for (size_t c = 0; c < m; ++c)
    if (offsets[c + 1] < offsets[c]) return set_err(NWC_ERR_ARG, "offsets not monotone at %zu", c);
  const uint64_t nv = offsets[m];
  if (nv && (!pks || !sigs)) return set_err(NWC_ERR_ARG, "null vote buffer");
  const int nd = (int)g_devs.size();
  std::vector<uint64_t> cuts(nd + 1);
  nwc_cert_cuts(offsets, m, (uint32_t)nd, cuts.data());
  std::vector<int> rc(nd, 0);
  std::vector<std::vector<uint64_t>> parts(nd);
  std::vector<std::thread> th;
  for (int i = 0; i < nd; ++i)
    th.emplace_back([&, i] { rc[i] = straus_range(i, digests, m, offsets, pks, sigs, cuts[i], cuts[i + 1], parts[i], msm); });
  for (auto& t : th) t.join();
  for (int r : rc) if (r < 0) return r;
  return batch_verdicts(offsets, m, cuts, parts, cert_ok_bitmap, bad_vote_bitmap);
}

// Committee updates are serialised: the devices' caches and the host's view of them (g_hcm, which
// the latency path trusts) change together, one committee at a time.
std::mutex g_cm_mu;
static int set_committee_locked(const uint8_t* pks, size_t n);

// The committee cache holds exactly nwc_set_committee_config's committee (set there, cleared by
// nwc_set_committee): the message pipeline may then leave the strict equations of uncached keys
// undecided -- their authors are outside the committee, and UnknownAuthority precedes
// InvalidSignature for every message kind (primary/src/core.rs, messages.rs).
std::atomic<bool> g_cm_is_config{false};
// Every device's committee cache holds keys with their per-key combs (the latency kernels'
// precondition; read without a context's mu by sanitizer_handle.h).
std::atomic<bool> g_cm_combs{false};

int nwc_set_committee(const uint8_t* pks, size_t n) {
  std::lock_guard<std::mutex> lk(g_cm_mu);
  g_cm_is_config = false;
  return set_committee_locked(pks, n);
}

static int set_committee_locked(const uint8_t* pks, size_t n) {
  if (int rc = require_init()) return rc;
  if (n && !pks) return set_err(NWC_ERR_ARG, "null buffer");
  if (n > (1u << 20)) return set_err(NWC_ERR_ARG, "committee of %zu keys is too large", n);
  // open-addressing table (exact 32-byte keys), load factor <= 1/4, probe length bounded
  std::vector<nwc::u32> keys(8 * n);
  std::memcpy(keys.data(), pks, 32 * n);
  std::vector<int32_t> table;
  const uint32_t slots = build_slots(keys, n, table);
  g_cm_combs = false;
  {
    // host view cleared while the devices change (a call in between takes the general path),
    // set again once every device holds the new cache (end of this function)
    std::lock_guard<std::mutex> lk(g_hcm.mu);
    g_hcm.idx.slots.clear();
  }
  for (auto& dp : g_devs) {
    DevCtx& d = *dp;
    std::lock_guard<std::mutex> lk(d.mu);
    HIP_TRY(hipSetDevice(d.hip_id));
    HIP_TRY(hipEventSynchronize(d.scratch_free));   // no verify launch still reads the old cache
    HIP_TRY(hipStreamSynchronize(d.stream));
    auto_reset(d);   // keys remembered under the old committee are stale
    if (d.lk_alloc) {   // so are the launch keys (the next launch-key launch measures its demand anew)
      HIP_TRY(hipMemsetAsync(d.lk.slots, 0xFF, 4 * (size_t)nwc::LK_SLOTS, d.stream));
      HIP_TRY(hipMemsetAsync(d.lk.state, 0, 16, d.stream));
      d.lk_censused = false;
    }
    // the old cache, and the stake / worker tables indexed like it (nwc_set_committee_config sets
    // those again right after)
    d.cm_n = 0; d.cm_slot_mask = 0; d.cc_n = 0;
    HIP_TRY(release_each({&d.cm_keys, &d.cm_flags, &d.cm_tables, &d.cm_slots, &d.cm_comb, &d.cc_stakes, &d.cc_worker_off,
                          &d.cc_worker_ids}));
    if (n == 0) continue;
    HIP_TRY(d.cm_keys.alloc(32 * n));
    HIP_TRY(d.cm_flags.alloc(4 * n));
    HIP_TRY(d.cm_tables.alloc(n * 129 * sizeof(nwc::ge_niels)));
    HIP_TRY(d.cm_slots.alloc(4 * (size_t)slots));
    HIP_TRY(hipMemcpyAsync(d.cm_keys, keys.data(), 32 * n, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d.cm_slots, table.data(), 4 * (size_t)slots, hipMemcpyHostToDevice, d.stream));
    const unsigned grid = (unsigned)((n * 129 + 255) / 256);
    hipLaunchKernelGGL(nwc::k_build_key_tables, dim3(grid), dim3(256), 0, d.stream, d.cm_keys.get(), (nwc::u32)n,
                       d.cm_tables.get(), d.cm_flags.get());
    HIP_TRY(hipGetLastError());
    if (n <= NWC_COMB_MAX_KEYS) {
      // per-key combs for the doubling-free path (radix 2^14: 20 MB per key)
      const size_t entries = n * nwc::COMB_PER_KEY;
      HIP_TRY(d.cm_comb.alloc(entries * sizeof(nwc::ge_niels_pad)));
      if (int rc = build_key_combs(d, d.cm_keys, (uint32_t)n, d.cm_comb)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(d.stream));
    d.cm_n = (uint32_t)n;
    d.cm_slot_mask = slots - 1;
  }
  if (n) {
    std::lock_guard<std::mutex> lk(g_hcm.mu);
    g_hcm.idx.keys = keys;
    g_hcm.idx.slots = table;
    g_hcm.idx.mask = slots - 1;
  }
  g_cm_combs = n > 0 && n <= NWC_COMB_MAX_KEYS;
  return 0;
}

int nwc_cache_stats(uint32_t* committee_keys, uint32_t* auto_keys) {
  if (int rc = require_init()) return rc;
  DevCtx& d = *ctx(t_dev < (int)g_devs.size() ? t_dev : 0);
  std::lock_guard<std::mutex> lk(d.mu);
  if (committee_keys) *committee_keys = d.cm_n;
  if (auto_keys) *auto_keys = d.ak_n;
  return 0;
}

int nwc_launch_keys_info(uint32_t* held, uint32_t* capacity) {
  if (int rc = require_init()) return rc;
  DevCtx& d = *ctx(t_dev < (int)g_devs.size() ? t_dev : 0);
  std::lock_guard<std::mutex> g(d.mu);
  uint32_t st[4] = {0, 0, 0, 0};
  if (d.lk_alloc) {
    HIP_TRY(hipSetDevice(d.hip_id));
    HIP_TRY(hipDeviceSynchronize());   // the set is updated on callers' streams
    HIP_TRY(hipMemcpy(st, d.lk.state, 16, hipMemcpyDeviceToHost));
  }
  if (held) *held = st[0];
  if (capacity) *capacity = nwc::LK_MAX_KEYS;
  return 0;
}

// Where a precomputed table lives on the calling thread's device (tests/test_gpu_tables.py reads the
// entries through its probe library).  Read-only: never allocates or builds.
int nwc_diag_table(const char* name, uint64_t* address, uint32_t* elem_bytes, uint64_t* elements, uint32_t* keys) {
  // the name is judged first, so a wrong one is an argument error with or without a device
  static const char* const NAMES[] = {"base_table", "sign_table", "base24", "comb_base", "comb16", "committee_keys",
                                      "committee_flags", "committee_tables", "committee_comb", "auto_keys", "auto_flags",
                                      "auto_tables", "auto_comb", "launch_keys", "launch_flags", "launch_comb"};
  if (!name) return set_err(NWC_ERR_ARG, "null table name");
  if (std::none_of(std::begin(NAMES), std::end(NAMES), [&](const char* s) { return std::strcmp(name, s) == 0; }))
    return set_err(NWC_ERR_ARG, "unknown table '%.40s'", name);
  if (int rc = require_init()) return rc;
  DevCtx& d = *ctx(t_dev < (int)g_devs.size() ? t_dev : 0);
  std::lock_guard<std::mutex> g(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  HIP_TRY(hipDeviceSynchronize());   // builds and regrows run on the device's and on callers' streams
  uint32_t lk_held = 0;
  if (d.lk_alloc) HIP_TRY(hipMemcpy(&lk_held, d.lk.state, 4, hipMemcpyDeviceToHost));
  constexpr uint32_t NIELS = sizeof(nwc::ge_niels), PAD = sizeof(nwc::ge_niels_pad);
  constexpr uint64_t COMB = nwc::COMB_PER_KEY;
  struct Row { const char* name; const void* p; uint32_t elem; uint64_t per; int64_t nkeys; };   // nkeys < 0: not per key
  const Row rows[] = {
      {"base_table", d.base_table.raw(), NIELS, 2 * 129, -1},
      {"sign_table", d.sign_table.raw(), NIELS, nwc::SIGN_TABLE_ENTRIES, -1},
      {"base24", d.base24.raw(), PAD, 2 * (uint64_t)nwc::B24_ENTRIES, -1},
      {"comb_base", d.comb_base.raw(), PAD, nwc::BaseComb::per, -1},
      {"comb16", d.comb16.raw(), PAD, nwc::COMB16_TOTAL, -1},
      {"committee_keys", d.cm_keys.raw(), 32, 1, d.cm_n},
      {"committee_flags", d.cm_flags.raw(), 4, 1, d.cm_n},
      {"committee_tables", d.cm_tables.raw(), NIELS, 129, d.cm_n},
      {"committee_comb", d.cm_comb.raw(), PAD, COMB, d.cm_n},
      {"auto_keys", d.ak_keys.raw(), 32, 1, d.ak_n},
      {"auto_flags", d.ak_flags.raw(), 4, 1, d.ak_n},
      {"auto_tables", d.ak_tables.raw(), NIELS, 129, d.ak_n},
      {"auto_comb", d.ak_comb.raw(), PAD, COMB, d.ak_n},
      {"launch_keys", d.lk_alloc ? d.lk_keys.raw() : nullptr, 32, 1, lk_held},
      {"launch_flags", d.lk_alloc ? d.lk_flags.raw() : nullptr, 4, 1, lk_held},
      {"launch_comb", d.lk_alloc ? d.lk_comb.raw() : nullptr, PAD, COMB, lk_held},
  };
  for (const Row& r : rows) {
    if (std::strcmp(name, r.name) != 0) continue;
    const uint64_t n = r.p ? (r.nkeys < 0 ? r.per : r.per * (uint64_t)r.nkeys) : 0;
    if (address) *address = (uint64_t)reinterpret_cast<uintptr_t>(r.p);
    if (elem_bytes) *elem_bytes = r.elem;
    if (elements) *elements = n;
    if (keys) *keys = r.p && r.nkeys > 0 ? (uint32_t)r.nkeys : 0;
    return 0;
  }
  return set_err(NWC_ERR_ARG, "table '%.40s' has no row", name);   // NAMES and rows[] list the same names
}

int nwc_auto_cache_info(uint32_t* capacity, uint64_t* builds, uint64_t* hits) {
  if (int rc = require_init()) return rc;
  DevCtx& d = *ctx(t_dev < (int)g_devs.size() ? t_dev : 0);
  std::lock_guard<std::mutex> lk(d.mu);
  if (capacity) *capacity = settings().auto_keys;
  if (builds) *builds = d.ak_builds;
  if (hits) *hits = d.ak_hits;
  return 0;
}

int nwc_sha512_trunc32_many(const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out32) {
  if (int rc = require_init()) return rc;
  if (n == 0) return 0;
  if (!offsets || !out32) return set_err(NWC_ERR_ARG, "null buffer");
  for (size_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return set_err(NWC_ERR_ARG, "offsets not monotone at %zu", i);
  if (offsets[n] > offsets[0] && !data) return set_err(NWC_ERR_ARG, "null data");
  return shard(n, [&](int di, uint64_t lo, uint64_t hi) -> int {
    DevCtx& d = *ctx(di);
    std::lock_guard<std::mutex> lk(d.mu);
    HIP_TRY(hipSetDevice(d.hip_id));
    const uint64_t k = hi - lo;
    if (k == 0) return 0;
    // Device layout: every message starts 16-byte aligned (the kernel's dwordx4 path).
    std::vector<uint64_t> starts(k), ends(k);
    uint64_t total = 0;
    for (uint64_t i = 0; i < k; ++i) {
      const uint64_t len = offsets[lo + i + 1] - offsets[lo + i];
      starts[i] = total;
      ends[i] = total + len;
      total += (len + 15) & ~15ull;
    }
    const size_t need = align256(total + 16) + 2 * align256(8 * k) + align256(32 * k);
    if (int rc = d.ensure_arena(need)) return rc;
    Carve c(d.arena);
    uint8_t* dd = c.take<uint8_t>(total + 16);
    uint64_t* dstarts = c.take<uint64_t>(8 * k);
    uint64_t* dends = c.take<uint64_t>(8 * k);
    uint8_t* dout = c.take<uint8_t>(32 * k);
    const bool aligned = (offsets[lo] % 16 == 0) && [&] {
      for (uint64_t i = 0; i < k; ++i) if (offsets[lo + i] - offsets[lo] != starts[i]) return false;
      return true;
    }();
    if (aligned) {
      if (total) HIP_TRY(hipMemcpyAsync(dd, data + offsets[lo], offsets[hi] - offsets[lo], hipMemcpyHostToDevice, d.stream));
    } else {
      std::vector<uint8_t> stage(total);
      for (uint64_t i = 0; i < k; ++i)
        if (ends[i] > starts[i]) std::memcpy(stage.data() + starts[i], data + offsets[lo + i], ends[i] - starts[i]);
      if (total) HIP_TRY(hipMemcpyAsync(dd, stage.data(), total, hipMemcpyHostToDevice, d.stream));
      HIP_TRY(hipStreamSynchronize(d.stream));  // `stage` is pageable and about to go out of scope
    }
    HIP_TRY(hipMemcpyAsync(dstarts, starts.data(), 8 * k, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(dends, ends.data(), 8 * k, hipMemcpyHostToDevice, d.stream));
    if (int rc = launch_digest(dd, dstarts, dends, k, dout, d.stream)) return rc;
    HIP_TRY(hipMemcpyAsync(out32 + 32 * lo, dout, 32 * k, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    return 0;
  });
}

int nwc_digest32(const uint8_t* data, size_t len, uint8_t out32[32]) {
  uint64_t offs[2] = {0, (uint64_t)len};
  return nwc_sha512_trunc32_many(data, offs, 1, out32);
}

// ---- device-resident ---------------------------------------------------------------------
int nwc_dev_set_device(int device) {
  if (int rc = require_init()) return rc;
  if (device < 0 || device >= (int)g_devs.size()) return set_err(NWC_ERR_ARG, "device %d not initialised", device);
  t_dev = device;
  return 0;
}

#define DEV_PROLOGUE                                                        \
  if (int rc_ = require_init()) return rc_;                                 \
  DevCtx& d = *ctx(t_dev < (int)g_devs.size() ? t_dev : 0);                 \
  std::lock_guard<std::mutex> lk(d.mu);                                     \
  HIP_TRY(hipSetDevice(d.hip_id));                                          \
  hipStream_t s = reinterpret_cast<hipStream_t>(stream); /* NULL = HIP default stream */

int nwc_dev_verify(const void* d_msgs, const void* d_msg_index, uint64_t msg_stride, const void* d_pks,
                   const void* d_sigs, uint64_t n, int strict, void* d_verdict_words, void* stream) {
  DEV_PROLOGUE
  if (n && (!d_msgs || !d_pks || !d_sigs || !d_verdict_words)) return set_err(NWC_ERR_ARG, "null buffer");
  return launch_verify(d, {.msgs = (const uint8_t*)d_msgs, .msg_index = (const uint32_t*)d_msg_index, .msg_stride = msg_stride,
                           .pks = (const uint8_t*)d_pks, .sigs = (const uint8_t*)d_sigs, .n = n, .strict = strict,
                           .out_words = (uint64_t*)d_verdict_words, .stream = s});
}

int nwc_diag_verify_clock(const void* d_msgs, uint64_t msg_stride, const void* d_pks, const void* d_sigs, uint64_t n,
                          void* d_verdict_words, void* stream, double* clock_ghz, uint32_t* waves) {
  DEV_PROLOGUE
  if (!d_msgs || !d_pks || !d_sigs || !d_verdict_words || !clock_ghz) return set_err(NWC_ERR_ARG, "null buffer");
  if (n < 4096) return set_err(NWC_ERR_ARG, "the clock stamp needs a full launch (n >= 4096)");
  // the stamps come from the plain k_verify launch: a committee cache would send these strict
  // equations to the comb kernel (no stamps), and a split launch would overwrite them
  if (d.cm_n) return set_err(NWC_ERR_ARG, "the clock stamp needs the plain k_verify path: clear the committee cache first");
  if (n > settings().verify_max_launch)
    return set_err(NWC_ERR_ARG, "the clock stamp needs a single launch (n <= %llu)", (unsigned long long)settings().verify_max_launch);
  // one stamp slot per wave of the largest grid launch_verify gives k_verify
  const uint64_t nwaves = (uint64_t)d.cus * d.verify_blocks_per_cu * NWC_VERIFY_GRID_MULT * 4;
  if (!d.stamps) HIP_TRY(d.stamps.alloc(32 * nwaves));
  HIP_TRY(hipMemsetAsync(d.stamps, 0, 32 * nwaves, s));
  if (int rc = launch_verify(d, {.msgs = (const uint8_t*)d_msgs, .msg_stride = msg_stride, .pks = (const uint8_t*)d_pks,
                                 .sigs = (const uint8_t*)d_sigs, .n = n, .strict = 1, .out_words = (uint64_t*)d_verdict_words,
                                 .stream = s, .flags = LV_STAMP}))
    return rc;
  std::vector<uint64_t> st(4 * nwaves);
  HIP_TRY(hipMemcpyAsync(st.data(), d.stamps, 32 * nwaves, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  std::vector<double> ghz;
  for (uint64_t w = 0; w < nwaves; ++w) {
    const uint64_t* x = &st[4 * w];
    // a wave that ran at least ~10 us of real time (100 MHz ticks)
    if (x[3] > x[2] + 1000 && x[1] > x[0]) ghz.push_back((double)(x[1] - x[0]) / (double)(x[3] - x[2]) * 0.1);
  }
  if (ghz.empty()) return set_err(NWC_ERR_DEVICE, "no wave stamped its clock");
  std::nth_element(ghz.begin(), ghz.begin() + ghz.size() / 2, ghz.end());
  *clock_ghz = ghz[ghz.size() / 2];
  if (waves) *waves = (uint32_t)ghz.size();
  return 0;
}

int nwc_dev_cert_reduce(const void* d_leaf_words, const void* d_offsets, uint64_t m, uint64_t nvotes,
                        void* d_cert_words, void* d_bad_words, void* stream) {
  DEV_PROLOGUE
  return launch_cert_reduce((const uint64_t*)d_leaf_words, (const uint32_t*)d_offsets, m, nvotes,
                            (uint64_t*)d_cert_words, (uint64_t*)d_bad_words, s);
}

int nwc_dev_verify_batch_straus(const void* d_digests, const void* d_offsets, const void* d_msg_index, uint64_t m,
                                uint64_t nvotes, const void* d_pks, const void* d_sigs, void* d_leaf_words,
                                void* stream) {
  DEV_PROLOGUE
  if (m == 0 || nvotes == 0) return 0;
  if (!d_digests || !d_offsets || !d_msg_index || !d_pks || !d_sigs || !d_leaf_words)
    return set_err(NWC_ERR_ARG, "null buffer");
  return launch_straus(d, static_cast<const uint8_t*>(d_digests), static_cast<const uint32_t*>(d_msg_index),
                       static_cast<const uint8_t*>(d_pks), static_cast<const uint8_t*>(d_sigs), nvotes,
                       static_cast<uint64_t*>(d_leaf_words), s);
}

int nwc_dev_verify_batch_msm(const void* d_digests, const void* d_offsets, const void* d_msg_index, uint64_t m,
                             uint64_t nvotes, const void* d_pks, const void* d_sigs, void* d_leaf_words, void* stream) {
  DEV_PROLOGUE
  if (m == 0 || nvotes == 0) return 0;
  if (!d_digests || !d_offsets || !d_msg_index || !d_pks || !d_sigs || !d_leaf_words)
    return set_err(NWC_ERR_ARG, "null buffer");
  return launch_batch_dalek(d, static_cast<const uint8_t*>(d_digests), static_cast<const uint32_t*>(d_msg_index), m,
                            static_cast<const uint8_t*>(d_pks), static_cast<const uint8_t*>(d_sigs), nvotes,
                            static_cast<uint64_t*>(d_leaf_words), s);
}

int nwc_msm_stats(uint64_t* groups_passed, uint64_t* groups_failed, uint64_t* key_overflows, uint64_t* groups_skipped) {
  if (int rc = require_init()) return rc;
  DevCtx* dp = ctx(t_dev);
  if (!dp) return set_err(NWC_ERR_ARG, "device index %d not initialised", t_dev);
  DevCtx& d = *dp;
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  uint32_t st[nwc::MSM_ST_WORDS] = {};
  if (d.msm_stats) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(st, d.msm_stats, sizeof st, hipMemcpyDeviceToHost));
  }
  if (groups_passed) *groups_passed = st[nwc::MSM_ST_PASSED];
  if (groups_failed) *groups_failed = st[nwc::MSM_ST_FAILED];
  if (key_overflows) *key_overflows = st[nwc::MSM_ST_OVERFLOW];
  if (groups_skipped) *groups_skipped = st[nwc::MSM_ST_SKIPPED];
  return 0;
}

int nwc_dev_sha512_trunc32(const void* d_data, const void* d_offsets, uint64_t n, void* d_out32, void* stream) {
  DEV_PROLOGUE
  return launch_digest((const uint8_t*)d_data, (const uint64_t*)d_offsets, nullptr, n, (uint8_t*)d_out32, s);
}

int nwc_dev_sha512_trunc32_ranges(const void* d_data, const void* d_starts, const void* d_ends, uint64_t n,
                                  void* d_out32, void* stream) {
  DEV_PROLOGUE
  if (n && (!d_starts || !d_ends || !d_out32)) return set_err(NWC_ERR_ARG, "null buffer");
  return launch_digest((const uint8_t*)d_data, (const uint64_t*)d_starts, (const uint64_t*)d_ends, n,
                       (uint8_t*)d_out32, s);
}

int nwc_dev_derive32(const uint8_t* tag, int taglen, uint64_t first, uint64_t n, void* d_out, void* stream) {
  DEV_PROLOGUE
  if (taglen < 0 || taglen > 96) return set_err(NWC_ERR_ARG, "tag longer than 96 bytes");
  if (n == 0) return 0;
  nwc::Tag64 t;
  std::memset(&t, 0, sizeof t);
  if (taglen > 64) return set_err(NWC_ERR_ARG, "tag longer than 64 bytes");
  std::memcpy(t.b, tag, (size_t)taglen);
  hipLaunchKernelGGL(nwc::k_derive32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t, taglen, first, n,
                     (uint8_t*)d_out);
  HIP_TRY(hipGetLastError());
  return 0;
}

int nwc_dev_keygen_sign(const void* d_seeds, const void* d_msgs, uint64_t n, void* d_pks, void* d_sigs,
                        void* stream) {
  DEV_PROLOGUE
  if (n == 0) return 0;
  if (int rc = ensure_verify_tables(d)) return rc;
  hipLaunchKernelGGL(nwc::k_keygen_sign, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint8_t*)d_seeds,
                     (const uint8_t*)d_msgs, n, (uint8_t*)d_pks, (uint8_t*)d_sigs, d.base_table);
  HIP_TRY(hipGetLastError());
  return 0;
}


int nwc_set_committee_config(const uint8_t* pks, const uint64_t* stakes, size_t n, const uint32_t* worker_offsets,
                             const uint32_t* worker_ids) {
  if (int rc = require_init()) return rc;
  if (n && (!pks || !stakes || !worker_offsets)) return set_err(NWC_ERR_ARG, "null buffer");
  if (n && worker_offsets[0] != 0) return set_err(NWC_ERR_ARG, "worker_offsets[0] must be 0");
  if (n > nwc::MSG_MAX_COMMITTEE)
    return set_err(NWC_ERR_ARG, "committee of %zu authorities exceeds %u", n, nwc::MSG_MAX_COMMITTEE);
  for (size_t k = 0; k < n; ++k)
    if (worker_offsets[k + 1] < worker_offsets[k]) return set_err(NWC_ERR_ARG, "worker_offsets not monotone");
  const uint32_t nw = n ? worker_offsets[n] : 0;
  if (nw && !worker_ids) return set_err(NWC_ERR_ARG, "null worker ids");
  // config::Committee holds a BTreeMap<PublicKey, Authority>: a key listed twice is one authority
  // with the LAST entry's stake and workers (a map insert replaces the value).  Deduplicate so the
  // cache index, the stake table and the quorum (config/src/lib.rs:181-186) all see that map.
  std::vector<uint8_t> ukeys;
  std::vector<uint64_t> ustakes;
  std::vector<uint32_t> uoff{0}, uids;
  {
    std::vector<size_t> last;   // entry index of the last occurrence, in first-appearance order
    for (size_t k = 0; k < n; ++k) {
      size_t j = 0;
      while (j < last.size() && std::memcmp(pks + 32 * last[j], pks + 32 * k, 32) != 0) ++j;
      if (j == last.size()) last.push_back(k);
      else last[j] = k;
    }
    for (size_t k : last) {
      ukeys.insert(ukeys.end(), pks + 32 * k, pks + 32 * k + 32);
      ustakes.push_back(stakes[k]);
      if (worker_offsets[k + 1] > worker_offsets[k])
        uids.insert(uids.end(), worker_ids + worker_offsets[k], worker_ids + worker_offsets[k + 1]);
      uoff.push_back((uint32_t)uids.size());
    }
  }
  n = ustakes.size();
  pks = ukeys.data();
  stakes = ustakes.data();
  worker_offsets = uoff.data();
  worker_ids = uids.data();
  std::lock_guard<std::mutex> cm_lk(g_cm_mu);
  g_cm_is_config = false;
  if (int rc = set_committee_locked(pks, n)) return rc;
  g_cm_is_config = true;
  uint64_t total = 0;
  for (size_t k = 0; k < n; ++k) total += stakes[k];
  for (auto& dp : g_devs) {
    DevCtx& d = *dp;
    std::lock_guard<std::mutex> lk(d.mu);
    HIP_TRY(hipSetDevice(d.hip_id));
    HIP_TRY(hipStreamSynchronize(d.stream));
    d.cc_n = 0;
    d.cc_quorum = 2 * total / 3 + 1;   // Committee::quorum_threshold (config/src/lib.rs:168-173)
    HIP_TRY(d.cc_stakes.alloc(8 * (n + 1)));   // (set_committee_locked released the old tables)
    HIP_TRY(d.cc_worker_off.alloc(4 * (n + 1)));
    HIP_TRY(d.cc_worker_ids.alloc(4 * (size_t)(nw + 1)));
    if (n) {
      HIP_TRY(hipMemcpy(d.cc_stakes, stakes, 8 * n, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(d.cc_worker_off, worker_offsets, 4 * (n + 1), hipMemcpyHostToDevice));
      if (!uids.empty()) HIP_TRY(hipMemcpy(d.cc_worker_ids, worker_ids, 4 * uids.size(), hipMemcpyHostToDevice));
    }
    d.cc_n = (uint32_t)n;
  }
  return 0;
}

}  // extern "C"

#include "digester.h"
#include "signer.h"
#include "sanitizer.h"
#include "verifier.h"
#include "sanitizer_handle.h"

extern "C" {

int nwc_memory_info(nwc_memory* out) {
  if (int rc = require_init()) return rc;
  if (!out) return set_err(NWC_ERR_ARG, "null argument");
  DevCtx* dp = ctx(t_dev);
  if (!dp) return set_err(NWC_ERR_ARG, "device index %d not initialised", t_dev);
  DevCtx& d = *dp;
  *out = nwc_memory{};
  {
    std::lock_guard<std::mutex> lk(d.mu);
    // tables: built by the first call that verifies (ensure_verify_tables) or signs (sign_table); 0 before
    out->tables = d.bufs.bytes(Account::Tables);
    out->committee = d.bufs.bytes(Account::Committee);
    out->auto_cache = d.bufs.bytes(Account::AutoCache);
    out->scratch = d.bufs.bytes(Account::Scratch);
  }
  out->digesters = digester_device_bytes(d.hip_id);
  size_t fr = 0, tot = 0;
  HIP_TRY(hipSetDevice(d.hip_id));
  HIP_TRY(hipMemGetInfo(&fr, &tot));
  out->device_free = fr;
  out->device_total = tot;
  return 0;
}

int nwc_trim(void) {
  if (int rc = require_init()) return rc;
  DevCtx* dp = ctx(t_dev);
  if (!dp) return set_err(NWC_ERR_ARG, "device index %d not initialised", t_dev);
  DevCtx& d = *dp;
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  // every stream: nwc_dev_* launches on callers' streams read these buffers too
  HIP_TRY(hipDeviceSynchronize());
  // the table slots, arenas and batch buffers, the per-launch lists (fallback, uncached, torsion
  // hash set) and the launch-key set (2.6 GB of combs): the next launch that needs them allocates
  // them again, the launch keys empty
  const hipError_t freed = d.bufs.release_trimmable();
  d.fb_cap = 0;
  d.ts_slot_count = 0;
  d.lk = nwc::LaunchKeys{};
  d.lk_alloc = false;
  HIP_TRY(freed);
  return 0;
}

}  // extern "C"
