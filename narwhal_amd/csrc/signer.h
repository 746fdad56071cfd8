// Host side of signing with a registered key (include/nwc.h "signing"; kernels in sign.h).
// Included by nwc_api.hip after the device contexts: uses DevCtx, set_err, HIP_TRY, knobs().
//
// A signer owns one 96-byte key record (a mod l, prefix, A) in device memory; the host keeps the
// public half only.  The seed crosses the device's pinned stage once, in nwc_signer_create, and the
// stage is zeroed before create returns.  Host calls stage digests in the same pinned memory; the
// kernels read them in place and store signatures and one "written" byte per signature there (the
// zero-copy path of the small verification calls, with its NWC_SPIN_WAIT convention).
#pragma once

namespace {

struct Signer {
  DevCtx* d = nullptr;
  nwc::SignKey* key = nullptr;   // device memory; nullptr once nwc_shutdown has released it
  uint8_t pk[32] = {};
};

std::mutex g_sign_mu;                  // guards g_signers; taken before a context's mu
std::unordered_set<Signer*> g_signers;

// digests per pinned chunk of a host call: 32 B in, 64 B out and a flag byte each, inside
// NWC_PINNED_STAGE_MAX
constexpr uint64_t SIGN_HOST_CHUNK = 8192;
static_assert((32 * SIGN_HOST_CHUNK) % 256 == 0 && 97 * SIGN_HOST_CHUNK <= NWC_PINNED_STAGE_MAX,
              "a chunk's digests, signatures and flags fit the pinned stage");

// votes per pinned chunk of a host call (nwc_signer_vote_many): id, round and origin (72 B) in,
// 64 B out and a flag byte each
constexpr uint64_t VOTE_HOST_CHUNK = 4096;
static_assert((32 * VOTE_HOST_CHUNK) % 256 == 0 && (8 * VOTE_HOST_CHUNK) % 256 == 0 &&
                  (72 + 64 + 1) * VOTE_HOST_CHUNK <= NWC_PINNED_STAGE_MAX,
              "a chunk's ids, rounds, origins, signatures and flags fit the pinned stage");

void wipe(volatile uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) p[i] = 0;
}

// The signer's basepoint table (60 KB), built by the device's first signer.  Caller holds d.mu.
int ensure_sign_table(DevCtx& d) {
  if (d.sign_table) return 0;
  HIP_TRY(d.sign_table.alloc(nwc::SIGN_TABLE_BYTES));
  hipLaunchKernelGGL(nwc::k_build_sign_table, dim3(nwc::SIGN_TABLE_ENTRIES / 64), dim3(64), 0, d.stream, d.sign_table.get());
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
  if (e != hipSuccess) {
    (void)d.sign_table.release();
    return set_err(NWC_ERR_DEVICE, "building the signer table failed: %s", hipGetErrorString(e));
  }
  return 0;
}

// h = SHA-512(seed), a, prefix, A = aB on the device.  pub (nullable): the claimed public half,
// *match = it equals A.  key (nullable): receives the record when it matches.  The seed's bytes in
// the pinned stage are zeroed before returning.  Caller holds d.mu and has set the device.
int expand_key(DevCtx& d, const uint8_t* seed, const uint8_t* pub, nwc::SignKey* key, uint8_t A[32], bool* match) {
  if (int rc = ensure_sign_table(d)) return rc;
  if (int rc = d.ensure_pinned(NWC_PINNED_STAGE_MAX)) return rc;
  uint8_t* h = d.pinned;
  std::memcpy(h, seed, 32);
  if (pub) std::memcpy(h + 32, pub, 32);
  else std::memset(h + 32, 0, 32);
  std::memset(h + 64, 0, 36);
  hipLaunchKernelGGL(nwc::k_sign_expand, dim3(1), dim3(64), 0, d.stream, (const uint8_t*)d.pinned.dev(), pub ? 1 : 0,
                     (const nwc::ge_niels*)d.sign_table, key, d.pinned.dev() + 64, reinterpret_cast<uint32_t*>(d.pinned.dev() + 96));
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
  wipe(h, 32);
  if (e != hipSuccess) return set_err(NWC_ERR_DEVICE, "key expansion failed: %s", hipGetErrorString(e));
  uint32_t status;
  std::memcpy(&status, h + 96, 4);
  if (status != 1 && status != 2) return set_err(NWC_ERR_DEVICE, "key expansion left no status");
  std::memcpy(A, h + 64, 32);
  *match = status == 1;
  return 0;
}

// n <= NWC_SIGN_WIDE_MAX takes k_sign_wide under "sign_path" 0 (by size).  Default 256, from measurement on an
// MI355X (tools/sign_rate.py, profiles/sign/sign_rate.json, DESIGN.md "Signing"): the wide kernel's
// host-call p50 is below the lane kernel's by more than the run-to-run spread at every measured
// n <= 256 (90 us against 408 us at n = 1, 281 us against 379 us at n = 256) and above it at 1,024
// (440 us against 396 us).
bool sign_takes_wide(uint64_t n) {
  const uint32_t path = knobs().sign_path;
  return path == 2 || (path == 0 && n <= settings().sign_wide_max);
}

int launch_sign(DevCtx& d, const nwc::SignKey* key, const uint8_t* msgs, uint64_t stride, uint64_t n, uint8_t* sigs,
                uint8_t* flags, bool wide, hipStream_t s) {
  if (n == 0) return 0;
  if (n >= (1ull << 31)) return set_err(NWC_ERR_ARG, "n must be below 2^31 per call");
  if (wide)
    hipLaunchKernelGGL(nwc::k_sign_wide, dim3((unsigned)n), dim3(64), 0, s, key, (const nwc::ge_niels*)d.sign_table, msgs,
                       stride, n, sigs, flags);
  else
    hipLaunchKernelGGL(nwc::k_sign, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, key, (const nwc::ge_niels*)d.sign_table,
                       msgs, stride, n, sigs, flags);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Vote::new for n (id, round, origin) triples: k_vote_wide or k_vote (vote.h), chosen as launch_sign's caller does.
int launch_vote(DevCtx& d, const nwc::SignKey* key, const uint8_t* ids, const uint64_t* rounds, const uint8_t* origins, uint64_t n,
                uint8_t* sigs, uint8_t* flags, bool wide, hipStream_t s) {
  if (n == 0) return 0;
  if (n >= (1ull << 31)) return set_err(NWC_ERR_ARG, "n must be below 2^31 per call");
  if (wide)
    hipLaunchKernelGGL(nwc::k_vote_wide, dim3((unsigned)n), dim3(64), 0, s, key, (const nwc::ge_niels*)d.sign_table, ids, rounds,
                       origins, n, sigs, flags);
  else
    hipLaunchKernelGGL(nwc::k_vote, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, key, (const nwc::ge_niels*)d.sign_table,
                       ids, rounds, origins, n, sigs, flags);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Releases a signer's key record: zeros written on the context's stream and waited for, then the
// free.  Caller holds d.mu and has set the device.
void release_key(DevCtx& d, Signer& sg) {
  if (!sg.key) return;
  (void)hipDeviceSynchronize();   // launches of nwc_dev_sign on callers' streams read the record
  (void)hipMemsetAsync(sg.key, 0, sizeof(nwc::SignKey), d.stream);
  (void)hipStreamSynchronize(d.stream);
  (void)hipFree(sg.key);
  sg.key = nullptr;
}

// nwc_shutdown: the contexts are about to go; live signers lose their key records (zeroed first)
// and answer NWC_ERR_NOT_INIT from then on.  Caller holds g_mu.
void signers_shutdown() {
  std::lock_guard<std::mutex> sl(g_sign_mu);
  for (Signer* sg : g_signers) {
    DevCtx& d = *sg->d;
    std::lock_guard<std::mutex> dl(d.mu);
    (void)hipSetDevice(d.hip_id);
    release_key(d, *sg);
    sg->d = nullptr;
  }
}

#define SIGNER_PROLOGUE(ptr)                                                                      \
  if (!(ptr)) return set_err(NWC_ERR_ARG, "null signer");                                         \
  if (int rc_ = require_init()) return rc_;                                                       \
  Signer& sg = *static_cast<Signer*>(const_cast<void*>(static_cast<const void*>(ptr)));           \
  if (!sg.d || !sg.key) return set_err(NWC_ERR_NOT_INIT, "the signer's device context was shut down")

}  // namespace

extern "C" {

int nwc_last_error_code(void) { return t_code; }

int nwc_keypair_from_seed(const uint8_t seed[32], uint8_t secret64[64]) {
  if (!seed || !secret64) return set_err(NWC_ERR_ARG, "null buffer");
  if (int rc = require_init()) return rc;
  DevCtx* dp = ctx(t_dev);
  if (!dp) return set_err(NWC_ERR_ARG, "device index %d not initialised", t_dev);
  DevCtx& d = *dp;
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  uint8_t A[32];
  bool match = false;
  if (int rc = expand_key(d, seed, nullptr, nullptr, A, &match)) return rc;
  std::memmove(secret64, seed, 32);
  std::memcpy(secret64 + 32, A, 32);
  return 0;
}

void* nwc_signer_create(const uint8_t secret64[64]) {
  if (!secret64) { set_err(NWC_ERR_ARG, "null secret key"); return nullptr; }
  if (require_init()) return nullptr;
  DevCtx* dp = ctx(t_dev);
  if (!dp) { set_err(NWC_ERR_ARG, "device index %d not initialised", t_dev); return nullptr; }
  DevCtx& d = *dp;
  auto sg = std::make_unique<Signer>();
  sg->d = &d;
  {
    std::lock_guard<std::mutex> lk(d.mu);
    if (hipSetDevice(d.hip_id) != hipSuccess) { set_err(NWC_ERR_DEVICE, "hipSetDevice failed"); return nullptr; }
    if (hipMalloc(&sg->key, sizeof(nwc::SignKey)) != hipSuccess) { set_err(NWC_ERR_DEVICE, "hipMalloc of the key record failed"); return nullptr; }
    bool match = false;
    int rc = hipMemsetAsync(sg->key, 0, sizeof(nwc::SignKey), d.stream) == hipSuccess ? 0 : set_err(NWC_ERR_DEVICE, "hipMemsetAsync failed");
    if (!rc) rc = expand_key(d, secret64, secret64 + 32, sg->key, sg->pk, &match);
    if (!rc && !match)
      rc = set_err(NWC_ERR_ARG, "secret key mismatch: bytes 32..64 are not the public key of the seed in bytes 0..32");
    if (rc) { (void)hipFree(sg->key); return nullptr; }   // a mismatch leaves the record all zero
  }
  std::lock_guard<std::mutex> sl(g_sign_mu);
  g_signers.insert(sg.get());
  return sg.release();
}

int nwc_signer_public_key(const void* signer, uint8_t pk[32]) {
  if (!signer || !pk) return set_err(NWC_ERR_ARG, "null argument");
  std::memcpy(pk, static_cast<const Signer*>(signer)->pk, 32);
  return 0;
}

int nwc_signer_sign_many(void* signer, const uint8_t* msgs32, size_t n, uint8_t* sigs) {
  if (n && (!msgs32 || !sigs)) return set_err(NWC_ERR_ARG, "null buffer");
  SIGNER_PROLOGUE(signer);
  if (n == 0) return 0;
  DevCtx& d = *sg.d;
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  if (int rc = d.ensure_pinned(NWC_PINNED_STAGE_MAX)) return rc;
  const bool spin = settings().spin_wait;   // 0 = wait for the stream (A/B)
  const bool wide = sign_takes_wide(n);
  for (uint64_t lo = 0; lo < n; lo += SIGN_HOST_CHUNK) {
    const uint64_t c = std::min<uint64_t>(SIGN_HOST_CHUNK, n - lo);
    const size_t so = align256(32 * c), fo = so + align256(64 * c);
    uint8_t* h = d.pinned;
    std::memcpy(h, msgs32 + 32 * lo, 32 * c);
    std::memset(h + fo, 0, c);
    if (int rc = launch_sign(d, sg.key, d.pinned.dev(), 32, c, d.pinned.dev() + so, d.pinned.dev() + fo, wide, d.stream)) return rc;
    // poll the "written" bytes (stored after the signature's words and a system fence); a launch
    // that never writes them (a device error) falls back to the stream wait after 200 ms
    const bool poll = spin && c <= NWC_WIDE_MAX;
    if (!poll || !nwc::plan::poll_written(h + fo, c, std::chrono::milliseconds(200))) {
      HIP_TRY(hipStreamSynchronize(d.stream));
      if (poll && !nwc::plan::poll_written(h + fo, c, std::chrono::microseconds(0)))
        return set_err(NWC_ERR_DEVICE, "sign kernel left signatures unwritten");
    }
    std::memcpy(sigs + 64 * lo, h + so, 64 * c);
  }
  return 0;
}

int nwc_signer_sign(void* signer, const uint8_t msg32[32], uint8_t sig[64]) {
  if (!msg32 || !sig) return set_err(NWC_ERR_ARG, "null buffer");
  return nwc_signer_sign_many(signer, msg32, 1, sig);
}

int nwc_dev_sign(void* signer, const void* d_msgs, uint64_t msg_stride, uint64_t n, void* d_sigs, void* stream) {
  if (n && (!d_msgs || !d_sigs)) return set_err(NWC_ERR_ARG, "null buffer");
  SIGNER_PROLOGUE(signer);
  if (msg_stride != 0 && msg_stride != 32) return set_err(NWC_ERR_ARG, "msg_stride must be 32 or 0");
  if (((uintptr_t)d_msgs & 15) || ((uintptr_t)d_sigs & 3)) return set_err(NWC_ERR_ARG, "d_msgs must be 16-byte and d_sigs 4-byte aligned");
  if (n == 0) return 0;
  DevCtx& d = *sg.d;
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  return launch_sign(d, sg.key, static_cast<const uint8_t*>(d_msgs), msg_stride, n, static_cast<uint8_t*>(d_sigs), nullptr,
                     sign_takes_wide(n), reinterpret_cast<hipStream_t>(stream));
}

int nwc_signer_vote_many(void* signer, const uint8_t* ids32, const uint64_t* rounds, const uint8_t* origins32, size_t n,
                         uint8_t* sigs) {
  if (n && (!ids32 || !rounds || !origins32 || !sigs)) return set_err(NWC_ERR_ARG, "null buffer");
  SIGNER_PROLOGUE(signer);
  if (n == 0) return 0;
  DevCtx& d = *sg.d;
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  if (int rc = d.ensure_pinned(NWC_PINNED_STAGE_MAX)) return rc;
  const bool spin = settings().spin_wait;
  const bool wide = sign_takes_wide(n);
  for (uint64_t lo = 0; lo < n; lo += VOTE_HOST_CHUNK) {
    const uint64_t c = std::min<uint64_t>(VOTE_HOST_CHUNK, n - lo);
    // ids | rounds | origins | signatures | flags, each from a 256-byte boundary
    const size_t ro = align256(32 * c), oo = ro + align256(8 * c), so = oo + align256(32 * c), fo = so + align256(64 * c);
    uint8_t* h = d.pinned;
    uint8_t* g = d.pinned.dev();
    std::memcpy(h, ids32 + 32 * lo, 32 * c);
    std::memcpy(h + ro, rounds + lo, 8 * c);
    std::memcpy(h + oo, origins32 + 32 * lo, 32 * c);
    std::memset(h + fo, 0, c);
    if (int rc = launch_vote(d, sg.key, g, reinterpret_cast<const uint64_t*>(g + ro), g + oo, c, g + so, g + fo, wide, d.stream))
      return rc;
    const bool poll = spin && c <= NWC_WIDE_MAX;
    if (!poll || !nwc::plan::poll_written(h + fo, c, std::chrono::milliseconds(200))) {
      HIP_TRY(hipStreamSynchronize(d.stream));
      if (poll && !nwc::plan::poll_written(h + fo, c, std::chrono::microseconds(0)))
        return set_err(NWC_ERR_DEVICE, "vote kernel left signatures unwritten");
    }
    std::memcpy(sigs + 64 * lo, h + so, 64 * c);
  }
  return 0;
}

int nwc_signer_vote(void* signer, const uint8_t id32[32], uint64_t round, const uint8_t origin32[32], uint8_t sig[64]) {
  if (!id32 || !origin32 || !sig) return set_err(NWC_ERR_ARG, "null buffer");
  return nwc_signer_vote_many(signer, id32, &round, origin32, 1, sig);
}

int nwc_dev_vote(void* signer, const void* d_ids, const void* d_rounds, const void* d_origins, uint64_t n, void* d_sigs,
                 void* stream) {
  if (n && (!d_ids || !d_rounds || !d_origins || !d_sigs)) return set_err(NWC_ERR_ARG, "null buffer");
  SIGNER_PROLOGUE(signer);
  if (((uintptr_t)d_ids & 15) || ((uintptr_t)d_origins & 15) || ((uintptr_t)d_rounds & 7) || ((uintptr_t)d_sigs & 3))
    return set_err(NWC_ERR_ARG, "d_ids and d_origins must be 16-byte, d_rounds 8-byte and d_sigs 4-byte aligned");
  if (n == 0) return 0;
  DevCtx& d = *sg.d;
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  return launch_vote(d, sg.key, static_cast<const uint8_t*>(d_ids), static_cast<const uint64_t*>(d_rounds),
                     static_cast<const uint8_t*>(d_origins), n, static_cast<uint8_t*>(d_sigs), nullptr, sign_takes_wide(n),
                     reinterpret_cast<hipStream_t>(stream));
}

int nwc_signer_destroy(void* signer) {
  if (!signer) return set_err(NWC_ERR_ARG, "null signer");
  Signer* sg = static_cast<Signer*>(signer);
  {
    // g_mu: a concurrent nwc_shutdown either releases the key before this or finds the signer gone
    std::lock_guard<std::mutex> gl(g_mu);
    {
      std::lock_guard<std::mutex> sl(g_sign_mu);
      g_signers.erase(sg);
    }
    if (sg->d) {
      DevCtx& d = *sg->d;
      std::lock_guard<std::mutex> lk(d.mu);
      (void)hipSetDevice(d.hip_id);
      release_key(d, *sg);
    }
  }
  wipe(sg->pk, 32);
  delete sg;
  return 0;
}

}  // extern "C"
