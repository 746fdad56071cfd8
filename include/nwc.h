/*
 * nwc.h -- C ABI of the MI355X-native Narwhal signature-and-digest hot path (libnwc.so).
 *
 * This is the drop-in boundary: the reference's `crypto` crate keeps its Rust API and calls
 * these entry points through a thin FFI shim.  Every entry point names the
 * reference interface it replaces (paths under /root/reference).
 *
 * Conventions
 *   - Plain pointers and sizes only; all buffers are caller-owned.  Host entry points take
 *     host memory; `nwc_dev_*` entry points take device (HBM) pointers and a hipStream_t
 *     passed as void* (NULL = the library's own stream) and are asynchronous on it.
 *   - Single verdicts: 0 = valid (Rust `Ok(())`), 1 = invalid (`Err(CryptoError)`),
 *     < 0 = runtime/device/argument error (never reported as "invalid"; the Rust shim panics).
 *   - Batch calls return 0 on success (< 0 on error) and fill bitmaps: bit i of a bitmap is
 *     byte i/8, bit i%8 (LSB first); 1 = valid for verdict bitmaps, 1 = bad for bad-vote bitmaps.
 *     Device bitmaps are arrays of uint64_t words with the same bit order.
 *   - Messages at the crypto surface are always 32-byte `Digest`s (crypto/src/lib.rs:203,214).
 *   - Thread-safe and reentrant (tokio tasks call concurrently: worker/src/worker.rs:182,227).
 */
#ifndef NWC_H
#define NWC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWC_OK 0
#define NWC_INVALID 1
#define NWC_ERR_DEVICE (-1)
#define NWC_ERR_ARG (-2)
#define NWC_ERR_NOT_INIT (-3)
#define NWC_ERR_NO_DEVICE (-4)

/* ---- lifecycle ------------------------------------------------------------------------ */
/* Node start-up hook (node/src/main.rs:69-134).  device_mask: bit d = use HIP device d
 * (0 = device 0).  Builds the basepoint table on each device.  Idempotent. */
int nwc_init(uint32_t device_mask);
void nwc_shutdown(void);
/* Text of the last error on the calling thread ("" if none). */
const char* nwc_last_error(void);
/* Code (< 0) of the last error on the calling thread (0 if none): what an entry that returns a
 * pointer, such as nwc_signer_create, would have returned as an int. */
int nwc_last_error_code(void);
/* ABI version (major << 16 | minor). */
int nwc_version(void);
/* Number of devices initialised. */
int nwc_device_count(void);
/* Identity of this build: a hash over the library's sources (narwhal_amd/csrc, this header)
 * and compile flags, computed by narwhal_amd/build.py, so a caller or test can check that the
 * binary it loaded was compiled from the tree it came with.  "unknown" for other builds. */
const char* nwc_build_id(void);

/* ---- device memory (a primary and a worker may share one GPU) ------------------------ */
/* Bytes held by this process on the calling thread's device (nwc_dev_set_device): tables =
 * basepoint tables (radix-2^24 ladder tables 2.1 GB, radix-2^22 comb 3.2 GB unless NWC_COMB16=0,
 * small ones), built by the first call that verifies (or generates a workload with
 * nwc_dev_keygen_sign) -- 0 in a process that only digests; a signer (nwc_signer_create) adds only
 * its own 60-KB basepoint table, so a process that only signs reports less than 1 MiB here;
 * committee = the nwc_set_committee cache (20 MB per key with combs); auto_cache = the auto key
 * cache (NWC_AUTO_KEYS) and the launch keys (20 MB of comb per key that joined); scratch =
 * per-launch buffers grown on demand (ladder tables, Straus tables, MSM groups, staging, message
 * buffers; the batch entries' buffers above NWC_VERIFY_KEEP_BYTES are freed by the next launch of
 * another path); digesters = the device buffers of live nwc_digesters on this device;
 * device_free / device_total = hipMemGetInfo. */
typedef struct nwc_memory {
  uint64_t tables, committee, auto_cache, scratch, digesters, device_free, device_total;
} nwc_memory;
int nwc_memory_info(nwc_memory* out);
/* Frees the calling thread's device's on-demand scratch (re-allocated by the next call that
 * needs it); waits for the device to be idle.  Tables and caches stay. */
int nwc_trim(void);

/* Test / A-B knobs, settable at run time instead of through the environment (which is read
 * once): "straus_nq" = votes per sub-batch of nwc_dev_verify_batch_straus (1..16, default 12,
 * env NWC_STRAUS_NQ); "force_windows" = half-ladder windows forced on every wave (33..37, 0 = off,
 * env NWC_FORCE_WINDOWS; verdicts must not change); "launch_keys" = 0 / 1 (default 1, env
 * NWC_LAUNCH_KEYS; nwc_launch_keys_info); "msm_group" = votes per Pippenger group of the MSM
 * entry (a multiple of 64 in 64..4096; 0, the default = sized per launch; env NWC_MSM_GROUP);
 * "msm_adapt" = 0 / 1 (default 1, env NWC_MSM_ADAPT): the MSM entry's skip policy (0 = the
 * equation on every group); "dalek_seed" = a fixed 32-bit seed of the batch entries' random z_i
 * (z_i = SHA-512(seed as 4 LE bytes || 28 zero bytes || u64le(i))[..16]; 0, the default = 32 bytes
 * of the host CSPRNG per launch), so tests can compute dalek's equation for the same z_i;
 * "sign_path" = the signers' kernel: 0 (default) by size (NWC_SIGN_WIDE_MAX), 1 = the
 * signature-per-lane kernel, 2 = the wave-per-signature kernel, at any n.
 * NWC_ERR_ARG for an unknown name or value.
 * Not part of the crate's API. */
int nwc_diag_set(const char* name, int64_t value);

/* The shader clock the headline kernel holds under load: one launch of a diagnostic build of the
 * strict verification kernel (k_verify with in-kernel stamps; the verdict path never runs it) on
 * the caller's device inputs, as nwc_dev_verify(.., strict = 1, ..), synchronised on `stream`.
 * Every wave stamps s_memtime / s_memrealtime at entry and exit; *clock_ghz = the median over
 * waves of delta(memtime) / delta(realtime) x 100 MHz, *waves = the waves counted.  Call it after
 * some seconds of back-to-back launches (MI355X_MICROARCH.md, DVFS item 6).  The verdict words
 * are written as by nwc_dev_verify.  NWC_ERR_ARG with a committee cache set (strict launches would
 * take the comb kernel, which has no stamps) or n > NWC_VERIFY_MAX_LAUNCH (a split launch).
 * Diagnostics only, not part of the crate's API. */
int nwc_diag_verify_clock(const void* d_msgs, uint64_t msg_stride, const void* d_pks, const void* d_sigs, uint64_t n,
                          void* d_verdict_words, void* stream, double* clock_ghz, uint32_t* waves);

/* ---- verification ----------------------------------------------------------------------- */
/* crypto::Signature::verify -> dalek verify_strict.  Replaces crypto/src/lib.rs:200-204
 * (called from primary/src/messages.rs:63-66 Header::verify and :138-141 Vote::verify). */
int nwc_verify_strict(const uint8_t msg32[32], const uint8_t pk[32], const uint8_t sig[64]);

/* crypto::Signature::verify_batch(digest, votes).  Replaces crypto/src/lib.rs:206-219
 * (called from primary/src/messages.rs:214 Certificate::verify).  Votes are n (pk, sig) pairs
 * laid out as pks[32*n], sigs[64*n].  n == 0 -> valid.  bad_bitmap (nullable, ceil(n/8)
 * bytes) receives the exact set of failing votes (the per-signature leaf). */
int nwc_verify_batch(const uint8_t msg32[32], const uint8_t* pks, const uint8_t* sigs, size_t n,
                     uint8_t* bad_bitmap);

/* n independent Signature::verify calls (BASELINE configs 2 and 5). */
int nwc_verify_strict_many(const uint8_t* msgs32, const uint8_t* pks, const uint8_t* sigs, size_t n,
                           uint8_t* verdict_bitmap);

/* m certificates (BASELINE config 3): certificate c has digest digests[32c] and votes
 * [offsets[c], offsets[c+1]) of pks/sigs; offsets[0] must be 0.  cert_ok_bitmap: m bits,
 * bad_vote_bitmap (nullable): offsets[m] bits. */
int nwc_verify_batch_many(const uint8_t* digests, const uint32_t* offsets, const uint8_t* pks,
                          const uint8_t* sigs, size_t m, uint8_t* cert_ok_bitmap,
                          uint8_t* bad_vote_bitmap);
/* The same m certificates through dalek's own batch equation (ed25519-dalek 1.0.1 batch.rs, the
 * algorithm behind crypto/src/lib.rs:218): random 128-bit z_i, one Straus pass per sub-batch of
 * ~12 votes on the GPU (nwc_dev_verify_batch_straus), the exact per-vote leaves for the sub-batches
 * it rejects.  Same verdicts and bad sets as nwc_verify_batch_many on the deterministic domain; on
 * dalek's randomized domain (pure-torsion residuals, torsion-bearing keys) dalek's probabilities
 * instead of Err.  Faster on clean traffic, slower at ~1 % bad votes. */
int nwc_verify_batch_straus_many(const uint8_t* digests, const uint32_t* offsets, const uint8_t* pks,
                                 const uint8_t* sigs, size_t m, uint8_t* cert_ok_bitmap,
                                 uint8_t* bad_vote_bitmap);

/* The same m certificates with dalek's batch semantics (crypto/src/lib.rs:218):
 * each certificate passes iff dalek's equation holds for it with random 128-bit z_i.  Where key
 * combs apply (a committee cache, or >= 65,536 votes whose keys repeat: launch keys) every vote is
 * first decided by the exact leaf on the comb path; then dalek's equation is evaluated once per
 * certificate over the votes the leaves rejected (the others contribute the identity whatever
 * z_i is), exactly, in the 8-torsion group -- the deterministic domain is the leaves' verdict, and
 * on the randomized one (pure-torsion residuals, torsion-bearing keys) a certificate passes with
 * dalek's probability, its failing votes then cleared from the bad set.  Otherwise the Pippenger
 * MSM per group of up to 4,096 consecutive votes (nwc_dev_verify_batch_msm) decides first and the
 * votes of the groups it rejects go to the exact leaves.  Every vote meets at most one random
 * equation: its certificate's, or (no combs) its group's. */
int nwc_verify_batch_msm_many(const uint8_t* digests, const uint32_t* offsets, const uint8_t* pks,
                              const uint8_t* sigs, size_t m, uint8_t* cert_ok_bitmap,
                              uint8_t* bad_vote_bitmap);

/* ---- signing with a registered key ------------------------------------------------------- */
/* crypto::Signature::new, SignatureService and generate_keypair (crypto/src/lib.rs:163-191,
 * 222-250; called for every header and vote: primary/src/messages.rs:24-46, 115-129).  A signer
 * is an opaque handle (void*) that owns the expanded key -- a = clamp(h[..32]) mod l, prefix =
 * h[32..] and A = aB for h = SHA-512(seed) -- in memory of the calling thread's device
 * (nwc_dev_set_device), computed once by create; the host side keeps the public half only, and the
 * pinned stage the seed crossed is zeroed before create returns.  Signatures are RFC 8032 /
 * dalek Keypair::sign over the 32 digest bytes: deterministic, byte-identical to dalek's.
 *
 * Deliberate deviation from ed25519-dalek 1.0.1: its Keypair::from_bytes does not check that
 * secret64[32..64] is the public key of the seed and then signs with whatever public half it was
 * given -- a signature that fails verification and, next to one made with the right half, gives
 * the key away.  nwc_signer_create derives A and refuses a secret whose public half differs
 * (NULL, nwc_last_error_code = NWC_ERR_ARG).
 *
 * The sign kernels read no memory address, take no branch and bound no loop by the key, the nonce
 * or their digits (DESIGN.md "Signing"); kernel arguments carry a pointer to the key record, never
 * key bytes.  Signing builds none of the verification tables: a signer uses a 60-KB basepoint table
 * of its own, built on the device by the first create.
 *
 * Conventions as everywhere here: thread-safe (calls on one signer are serialised on its device),
 * errors < 0, NWC_ERR_ARG for null pointers, NWC_ERR_NOT_INIT before nwc_init, n == 0 is a no-op
 * returning 0.  n <= NWC_SIGN_WIDE_MAX (environment, default 256, measured: DESIGN.md "Signing") takes the
 * wave-per-signature kernel, larger calls the signature-per-lane kernel; host calls stage their
 * digests in pinned memory that the kernels read and write in place, and calls of <= 1024 digests
 * poll it instead of waiting for the stream (NWC_SPIN_WAIT=0 turns that off). */
/* generate_keypair: seed = 32 bytes of the CALLER's CSPRNG -> secret64 = seed || A
 * (Keypair::to_bytes).  seed and secret64 may overlap at secret64[0]. */
int nwc_keypair_from_seed(const uint8_t seed[32], uint8_t secret64[64]);
/* SignatureService::new / Keypair::from_bytes.  NULL on failure (nwc_last_error,
 * nwc_last_error_code). */
void* nwc_signer_create(const uint8_t secret64[64]);
int nwc_signer_public_key(const void* signer, uint8_t pk[32]);
/* Signature::new(digest, secret) */
int nwc_signer_sign(void* signer, const uint8_t msg32[32], uint8_t sig[64]);
/* n digests msgs32[32 i] -> sigs[64 i] in one launch (a round's votes; what a SignatureService
 * drains from its queue) */
int nwc_signer_sign_many(void* signer, const uint8_t* msgs32, size_t n, uint8_t* sigs);
/* Device-resident: d_msgs (16-byte aligned) holds digest i at msg_stride * i, msg_stride = 32, or
 * 0 for one digest signed n times; d_sigs n x 64 B.  Asynchronous on `stream`.  n < 2^31. */
int nwc_dev_sign(void* signer, const void* d_msgs, uint64_t msg_stride, uint64_t n, void* d_sigs, void* stream);
/* Vote::new (primary/src/messages.rs:115-129): sig = sign(SHA-512(id || round LE || origin)[..32]),
 * the digest computed on the device in the same launch as the signature, for a header the caller
 * has already accepted.  id and origin are only hashed (any 32 bytes).  Conventions, chunking,
 * polling and the choice of kernel ("sign_path", NWC_SIGN_WIDE_MAX) as nwc_signer_sign_many. */
int nwc_signer_vote(void* signer, const uint8_t id32[32], uint64_t round, const uint8_t origin32[32], uint8_t sig[64]);
int nwc_signer_vote_many(void* signer, const uint8_t* ids32, const uint64_t* rounds, const uint8_t* origins32,
                         size_t n, uint8_t* sigs);
/* device-resident: d_ids, d_origins 16-byte aligned, d_rounds 8-byte, d_sigs 4-byte; asynchronous on stream */
int nwc_dev_vote(void* signer, const void* d_ids, const void* d_rounds, const void* d_origins, uint64_t n,
                 void* d_sigs, void* stream);
/* Overwrites the key record with zeros (a memset on the signer's device stream, waited for), then
 * frees it; waits for the device first, so launches of nwc_dev_sign still in flight finish.  No
 * call on the signer may start after destroy.  nwc_shutdown does the same to signers still alive,
 * which then answer NWC_ERR_NOT_INIT; destroy them afterwards all the same. */
int nwc_signer_destroy(void* signer);

/* ---- concurrent small verify calls behind one launch -------------------------------------- */
/* Every verification a primary makes is a small call: Signature::verify is one equation
 * (crypto/src/lib.rs:200-204; Header::verify and Vote::verify, primary/src/messages.rs:63-66,
 * 138-141), Signature::verify_batch one certificate (crypto/src/lib.rs:206-219;
 * Certificate::verify, primary/src/messages.rs:214) -- and the reference makes them from many tokio
 * tasks at once (node/src/main.rs:17, worker/src/worker.rs:182,227).  nwc_verify_strict and
 * nwc_verify_batch answer such calls one at a time per device.  A verifier is an opaque handle
 * (void*, as a signer) bound to the calling thread's device (nwc_dev_set_device), like a
 * digester: concurrent blocking calls on one verifier are packed into GROUPS that share a launch,
 * and each caller returns as soon as its own verdict bytes are in.  Opt-in; the plain entries are
 * unchanged.
 *
 * Verdicts and bad sets are exactly those of nwc_verify_strict / nwc_verify_batch on the same
 * inputs (dalek verify_strict; the exact batch leaves, Err on the randomized domain): every
 * equation carries its own mode into the shared launch.
 *
 * A group closes when it holds max_requests requests (0 = as many as fit), when the next request's
 * equations do not fit its capacity (4,096 equations; NWC_VERIFIER_GROUP_EQ in the environment, read
 * by the first create), or when max_wait_us have passed since its first request arrived.
 * max_wait_us == 0 never waits for company: a group is then whatever arrived while the previous
 * group was in flight, and a lone caller launches at once.  Two group buffers of coherent pinned
 * host memory (145 B per equation of capacity: 0.6 MB each by default) are read in place by the
 * kernels; a verifier holds no device memory of its own.
 *
 * Conventions as everywhere here: both verify calls block and may be made from any number of
 * threads; n == 0 is Ok at once; null pointers give NWC_ERR_ARG; NWC_ERR_NOT_INIT before nwc_init; a
 * request of more than 1,024 votes (or more than a group holds) is handed to nwc_verify_batch
 * (bypassed_requests).  A device error in a group reaches exactly that group's callers as a code
 * < 0, never as "invalid".  destroy lets queued requests finish, wakes blocked callers and waits
 * for them to leave (no call on the verifier may start after destroy); nwc_shutdown does the same
 * to verifiers still alive, which then answer NWC_ERR_NOT_INIT; destroy them afterwards all the
 * same.  create returns NULL on failure (nwc_last_error, nwc_last_error_code). */
typedef struct nwc_verifier_stats_t {
  uint64_t groups, requests, equations, wide_equations, cold_equations, redone_equations, bypassed_requests,
      max_requests_in_group;
} nwc_verifier_stats_t;
void* nwc_verifier_create(uint32_t max_requests, uint32_t max_wait_us);
/* Signature::verify: 0 valid, 1 invalid, < 0 error */
int nwc_verifier_verify_strict(void* verifier, const uint8_t msg32[32], const uint8_t pk[32], const uint8_t sig[64]);
/* Signature::verify_batch(digest, votes): as nwc_verify_batch, bad_bitmap nullable */
int nwc_verifier_verify_batch(void* verifier, const uint8_t msg32[32], const uint8_t* pks, const uint8_t* sigs, size_t n,
                              uint8_t* bad_bitmap);
/* out: eight uint64_t laid out as nwc_verifier_stats_t.  requests / equations are counted when a
 * request joins a group, the rest when the group launches: groups = launches shared; wide /
 * cold_equations = equations whose key a cache held / first-sight equations; redone_equations =
 * equations decided again on the general path (a key missing on the device after all, a failed
 * lattice reduction, an unwritten verdict byte). */
int nwc_verifier_stats(void* verifier, uint64_t* out);
int nwc_verifier_destroy(void* verifier);

/* ---- concurrent wire messages behind one pipeline launch ---------------------------------- */
/* A primary receives its wire messages one at a time, on one tokio task per peer connection
 * (PrimaryReceiverHandler::dispatch, primary/src/primary.rs:224-240), and needs the
 * Core::sanitize_header / sanitize_vote / sanitize_certificate verdict of each before Core may act
 * on it.  nwc_sanitize_messages (below) is a batch entry: with one message it holds the device for
 * the whole call and makes two host round trips, so concurrent callers run one after another.  A
 * sanitizer is an opaque handle (void*, as a verifier) bound to the calling thread's device:
 * concurrent blocking calls, each carrying ONE bincode PrimaryMessage, are packed into GROUPS; one
 * fixed set of launches (parse, decide, finalize) decides a group with no host round trip inside
 * it, and each caller returns as soon as its own result word is in.  Opt-in; the batch entry is
 * unchanged.
 *
 * The code (NWC_DAG_*), digest and kind are exactly those of nwc_sanitize_messages on this message
 * alone with the same gc_round and vote_target (its DagError precedence; the batch leaves, Err on
 * the randomized domain).  gc_round and vote_target (72 bytes as there, or NULL) belong to the
 * request: Core's state moves while messages are in flight, so two messages of one group may carry
 * different values, and each is judged by its own.
 *
 * A group closes when it holds max_messages messages (0 = as many as fit), when the next message's
 * bytes do not fit, or when max_wait_us have passed since it was opened.  max_wait_us == 0 never
 * waits for company: a lone caller launches at once, and under load a group is whatever arrived
 * during the previous flight.  A group holds NWC_SANITIZER_GROUP_BYTES wire bytes (1 MiB, ~100
 * certificates of a 100-node committee; every message starts 16-byte aligned) and
 * NWC_SANITIZER_GROUP_MSGS messages (256), both read from the environment by the first create.  A
 * sanitizer holds two group buffers of coherent pinned host memory, read in place by the kernels,
 * and one block of HBM scratch (nwc_memory_info: scratch; kept by nwc_trim, released by destroy).
 *
 * Conventions as the verifier's: calls block and may be made from any number of threads; a null
 * sanitizer, or a null msg with len > 0, gives NWC_ERR_ARG; len == 0 is a message of no bytes
 * (NWC_DAG_SERIALIZATION_ERROR) as in the batch entry; NWC_ERR_NOT_INIT before nwc_init and before
 * nwc_set_committee_config (create then returns NULL).  A message larger than a group is handed to
 * nwc_sanitize_messages (bypassed_messages), and so is every message while the grouped kernels'
 * preconditions do not hold: the committee cache is the configured committee
 * (nwc_set_committee_config was the last to set it) and has its combs (<= 1,024 keys), NWC_COLD
 * and NWC_VERIFY_PATH at their defaults.  A device error in a group reaches exactly that group's
 * callers as a code < 0, never as a NWC_DAG_* code.  destroy lets queued requests finish, wakes
 * blocked callers and waits for them to leave (no call on the sanitizer may start after destroy);
 * nwc_shutdown does the same to sanitizers still alive, which then answer NWC_ERR_NOT_INIT; destroy
 * them afterwards all the same.  create returns NULL on failure (nwc_last_error,
 * nwc_last_error_code). */
typedef struct nwc_sanitizer_stats_t {
  uint64_t groups, messages, bytes, equations, redone_messages, bypassed_messages,
      max_messages_in_group, reserved;
} nwc_sanitizer_stats_t;
void* nwc_sanitizer_create(uint32_t max_messages, uint32_t max_wait_us);
/* Core::sanitize_header / sanitize_vote / sanitize_certificate of ONE wire message.
 * Returns NWC_DAG_* (>= 0) or an error < 0.  digest32, kind nullable. */
int nwc_sanitizer_sanitize(void* sanitizer, const uint8_t* msg, size_t len, uint64_t gc_round,
                           const uint8_t* vote_target, uint8_t digest32[32], uint8_t* kind);
/* out: eight uint64_t laid out as nwc_sanitizer_stats_t.  messages / bytes are counted when a
 * message joins a group, groups / max_messages_in_group when a group launches, equations (the
 * signature equations the groups decided: a message's own once every earlier check of its
 * precedence chain but Header::digest has passed, a certificate's votes once its vote list is
 * sound) and redone_messages (messages decided again by nwc_sanitize_messages: the result word
 * asked for it or was still unwritten after the stream had been waited for) when a caller leaves. */
int nwc_sanitizer_stats(void* sanitizer, uint64_t* out);
/* Core::process_header's next step in the same flight (primary/src/core.rs:202-217 -> Vote::new,
 * messages.rs:115-129).  As nwc_sanitizer_sanitize; additionally, when the message is a header and
 * its code is NWC_DAG_OK, vote_sig64 receives Vote::new(header, signer's key).signature and
 * *voted = 1; otherwise *voted = 0 and vote_sig64 is zeroed (on an error < 0 too).  signer must live
 * on the sanitizer's device (NWC_ERR_ARG otherwise); vote_sig64 and voted must not be NULL.
 *
 * A group in which at least one request carries a signer gets one more launch, shared by all of
 * its headers; groups without such requests run exactly the launches of nwc_sanitizer_sanitize.
 * Requests with and without a signer, and with different signers, may share a group.
 *
 * Two things that are not obvious:
 *   - The library is stateless about voting.  Core's last_voted check (at most one vote per origin
 *     and round, core.rs:206-212) stays the caller's duty; a signature that Core then decides not
 *     to send is simply dropped.  Ed25519 signing is deterministic, so an unused signature leaks
 *     nothing that a used one would not.
 *   - A vote is signed only AFTER the header's code is Ok (the result word of its slot, or the
 *     batch entry's code for a message that was redone or bypassed), never speculatively on
 *     unverified wire bytes.
 * The signer may not be destroyed while a call that carries it is in progress. */
int nwc_sanitizer_sanitize_vote(void* sanitizer, void* signer, const uint8_t* msg, size_t len, uint64_t gc_round,
                                const uint8_t* vote_target, uint8_t digest32[32], uint8_t* kind,
                                uint8_t vote_sig64[64], int32_t* voted);
/* votes signed inside a group flight / by the one-message fallback.  Either pointer may be NULL. */
int nwc_sanitizer_vote_stats(void* sanitizer, uint64_t* in_flight, uint64_t* alone);
/* The device's decode from the same flight: nwc_sanitizer_sanitize_vote plus the
 * message's nwc_msg_view record, which is declared below with the batch entries that return it.
 *   view == NULL   the call IS nwc_sanitizer_sanitize_vote -- without a signer,
 *                  nwc_sanitizer_sanitize -- and body, body_cap, body_used are ignored and untouched.
 *   view != NULL   one nwc_msg_view record of 160 bytes.  body and body_used are required, body_cap >=
 *                  nwc_msg_view_body_bound(len, 1); a call that breaks a rule returns NWC_ERR_ARG
 *                  before anything is queued (nwc_sanitizer_stats does not move).  signer may be
 *                  NULL: vote_sig64 and voted are then ignored; with a signer both are required and
 *                  it must live on the sanitizer's device.
 * The record, *body_used and the body areas the record names are what nwc_sanitize_messages_view
 * returns for this message in a call of its own (m = 1, the same gc_round, vote_target and signer),
 * the three body offsets included: one message's areas are handed out from offset 0 in the order
 * payload, parents, voters.  A message that does not decode still gets its record (decoded = 0,
 * kind, code).  On an error < 0 the record is zeroed and *body_used = 0.
 *
 * A group in which at least one request asks for a view gets one more launch (one wave per
 * message) behind the result words and before the votes' launch; groups without such requests run
 * exactly the launches they ran before.  A request whose message was redone or bypassed gets
 * record and decision from one call of nwc_sanitize_messages_view. */
int nwc_sanitizer_sanitize_view(void* sanitizer, void* signer /* or NULL */, const uint8_t* msg, size_t len,
                                uint64_t gc_round, const uint8_t* vote_target, uint8_t digest32[32], uint8_t* kind,
                                uint8_t vote_sig64[64], int32_t* voted, /* required with a signer, else ignored */
                                void* view,                             /* one nwc_msg_view, or NULL */
                                uint8_t* body, uint64_t body_cap, uint64_t* body_used);
/* views delivered by a group flight / by the one-message fallback.  Either pointer may be NULL. */
int nwc_sanitizer_view_stats(void* sanitizer, uint64_t* in_flight, uint64_t* alone);
int nwc_sanitizer_destroy(void* sanitizer);

/* Committee key cache (config/src/lib.rs:154-156 Committee).  Optional: verdicts never
 * depend on it. */
int nwc_set_committee(const uint8_t* pks, size_t n);

/* Key caches of the calling thread's device (nwc_dev_set_device): keys in the committee cache,
 * and in the auto key cache -- keys of small host calls (<= 1024 equations) outside the
 * committee cache, added the second time they are seen, so that a node's repeated certificates
 * take the latency kernel without nwc_set_committee (NWC_AUTO_KEYS = capacity, 0 = off).
 * Diagnostics only: verdicts never depend on either cache.  Not part of the crate's API. */
int nwc_cache_stats(uint32_t* committee_keys, uint32_t* auto_keys);

/* Auto key cache lifecycle of the calling thread's device: capacity (NWC_AUTO_KEYS), insert
 * batches built so far, and calls served by the latency kernel over it.  Once full, new keys
 * replace the oldest (FIFO); nwc_set_committee empties it.  Any pointer may be NULL.
 * Diagnostics only, not part of the crate's API. */
int nwc_auto_cache_info(uint32_t* capacity, uint64_t* builds, uint64_t* hits);

/* Launch keys of the calling thread's device: a batch-leaf launch of >= 65,536 equations without a
 * committee cache samples its keys, and keys it repeats (>= ~1/4096 of the sample) join a
 * device-resident set with their flags and radix-2^14 combs (built once; room for 20 MB of comb
 * per key is reserved as keys ask to join: the first launch measures its demand, later ones grow
 * it from the demand the previous launch recorded, so a key that did not fit joins at the next
 * launch), so that votes of a committee the caller never registered take the comb kernel --
 * cross-certificate key aggregation, no nwc_set_committee needed.  Up to `capacity` keys; emptied by nwc_set_committee
 * and nwc_trim, and replaced by a launch whose repeated keys do not fit while the held ones cover
 * less than a quarter of its sample (a new committee); NWC_LAUNCH_KEYS=0 (or
 * nwc_diag_set("launch_keys", 0)) turns it off.
 * Verdicts never depend on it.  Waits for the device.  Diagnostics only. */
int nwc_launch_keys_info(uint32_t* held, uint32_t* capacity);

/* Where a precomputed point table of the calling thread's device lives, for tests that audit the
 * stored entries (tests/test_gpu_tables.py): the device address (0 if the table is not built),
 * the size of one element in bytes, the number of elements and, for the per-key arrays, the keys
 * held (elements = keys x elements per key; 0 otherwise).  Names: "base_table" (2 x 129 Niels
 * entries of 120 bytes), "sign_table" (64 x 8), "base24" (2 x (2^23 + 1) padded entries of 128
 * bytes), "comb_base" (32 x 129), "comb16" (12 x (2^21 + 1)); "committee_keys" (32-byte keys),
 * "committee_flags" (32-bit words: 1 decodes, 2 small order, 4 torsion), "committee_tables" (129
 * entries per key), "committee_comb" (19 x 8,193 padded entries per key); "auto_keys", "auto_flags",
 * "auto_tables", "auto_comb" (the auto key cache, the same shapes); "launch_keys", "launch_flags",
 * "launch_comb" (the launch keys; they keep no 129-entry tables).  Read-only: it never allocates or
 * builds, and returns NWC_ERR_ARG for any other name.  Waits for the device.  The address holds
 * until the next library call that can build, rebuild, regrow or free the table (any verifying or
 * signing call, nwc_set_committee, nwc_trim, nwc_shutdown); the memory stays the library's and is
 * only to be read.  Any out pointer may be NULL.  Diagnostics only, not part of the crate's API. */
int nwc_diag_table(const char* name, uint64_t* address, uint32_t* elem_bytes, uint64_t* elements, uint32_t* keys);

/* ---- worker batch digests behind a Processor-shaped queue (worker/src/processor.rs:35-55) ----
 * Replaces the Processor's per-batch `Sha512::digest(&batch)[..32]` (:38) for workers that can
 * hand batches over in groups.  A digester owns a drain thread on the calling thread's device
 * (nwc_dev_set_device): it takes the first submitted batch, then whatever else arrives within
 * max_wait_us (up to max_group batches), and digests the group with one GPU launch on its own
 * stream.  Batches are BORROWED: the caller keeps each one alive until its digest has been
 * polled (the Processor stores the batch after hashing it anyway).  Digests come back in
 * submission order with the caller's tag.  One 500-KB batch alone takes ~28 ms on the GPU (a
 * sequential SHA-512 chain on one lane) against ~0.36 ms on one host core: measured, the GPU ties 16
 * host cores at ~1,000 batches per group and is ~3.8x faster at 100,000 (PCIe-bound, ~40 GB/s;
 * 54 GB/s from the receive arena below).  Data path: NWC_DIGEST_STAGES (4) pinned 32-MB stages filled by
 * NWC_DIGEST_COPY_THREADS (8) host threads; one launch holds at most NWC_DIGEST_MAX_BYTES
 * (16 GiB) of batches in HBM (larger groups are cut), and a device buffer above
 * NWC_DIGEST_KEEP_BYTES (1 GiB) is freed after its group.  create returns NULL on failure
 * (nwc_last_error).  poll waits up to wait_us for a result and returns one run of results with
 * the same status: digests (returns 0), or the tags of a group that failed on the device (returns
 * the error code < 0; digests32 zeroed) -- every submitted tag comes back exactly once, in order.
 * After a failure submit refuses new batches, and poll returns the error (n_done = 0) once every
 * batch submitted before it has come back.  destroy digests what is queued, wakes threads blocked in poll and
 * waits for them to leave, then frees the digester (no call on it may start after destroy). */
typedef struct nwc_digester nwc_digester;
nwc_digester* nwc_digester_create(uint32_t max_group, uint32_t max_wait_us);
int nwc_digester_submit(nwc_digester* q, const uint8_t* batch, size_t len, uint64_t tag);
int nwc_digester_poll(nwc_digester* q, size_t max, uint32_t wait_us, uint64_t* tags, uint8_t* digests32,
                      size_t* n_done);
int nwc_digester_stats(nwc_digester* q, uint64_t* groups, uint64_t* batches, uint64_t* bytes);
/* Receive arena: `bytes` of pinned host memory owned by the digester (freed by destroy), for a
 * worker that receives batches straight into it (the network read's destination, instead of a
 * Vec the Processor later hands over).  A group whose batches all lie in the arena, each placed
 * at the previous one's offset + its length rounded up to 16 bytes (starts 16-byte aligned),
 * skips the stage fill: each contiguous run of batches is one DMA from the arena into HBM (at most
 * 1,024 runs per group; otherwise, or with any batch outside the arena, the group takes the stage
 * path).  Batches stay borrowed as with any submit: do not overwrite a batch's bytes before its
 * digest has been polled.  Create it before the first submit; a later call returns the same
 * arena if `bytes` fits.  Returns NULL on failure (nwc_last_error).  No counterpart in the
 * reference (its Processor gets a Vec<u8>). */
uint8_t* nwc_digester_arena(nwc_digester* q, size_t bytes);
/* Groups that took the arena's direct path so far (diagnostics). */
int nwc_digester_direct_groups(nwc_digester* q, uint64_t* direct_groups);
int nwc_digester_destroy(nwc_digester* q);

/* ---- primary messages ---------------------------------------- */
/* config::Committee for the message checks (config/src/lib.rs:134-212): n authorities with
 * their keys, stakes (Committee::stake) and worker ids (Committee::worker): authority k runs
 * workers worker_ids[worker_offsets[k] .. worker_offsets[k+1]).  Also sets the key cache
 * (nwc_set_committee); a later nwc_set_committee drops the stake/worker tables.  At most 4096
 * authorities. */
int nwc_set_committee_config(const uint8_t* pks, const uint64_t* stakes, size_t n,
                             const uint32_t* worker_offsets, const uint32_t* worker_ids);

/* DagError codes of nwc_sanitize_messages (primary/src/error.rs) */
#define NWC_DAG_OK 0
#define NWC_DAG_INVALID_SIGNATURE 1
#define NWC_DAG_INVALID_HEADER_ID 2
#define NWC_DAG_MALFORMED_HEADER 3
#define NWC_DAG_UNKNOWN_AUTHORITY 4
#define NWC_DAG_AUTHORITY_REUSE 5
#define NWC_DAG_CERTIFICATE_REQUIRES_QUORUM 6
#define NWC_DAG_TOO_OLD 7
#define NWC_DAG_SERIALIZATION_ERROR 8
#define NWC_DAG_UNEXPECTED_VOTE 9
#define NWC_DAG_UNEXPECTED_MESSAGE 10
/* not a DagError: decoding a PublicKey whose base64 gives < 32 bytes panics in the reference
 * (crypto/src/lib.rs:75 `bytes[..32]`, inside bincode::deserialize at primary/src/primary.rs:230) */
#define NWC_DAG_DECODE_PANIC 11

/* Core::sanitize_header / sanitize_vote / sanitize_certificate (primary/src/core.rs:306-346)
 * for a batch of wire messages, each the bincode bytes of a PrimaryMessage as received by
 * PrimaryReceiverHandler::dispatch (primary/src/primary.rs:224-240): message i is
 * data[offsets[i] .. offsets[i+1]).  Decoding (incl. the base64 PublicKeys), Header::digest,
 * Vote::digest, Certificate::digest, the committee checks of Header::verify / Vote::verify /
 * Certificate::verify (primary/src/messages.rs:48-67, 131-142, 189-215) and every signature run
 * on the GPU.  gc_round: TooOld for headers and certificates (0 disables).  vote_target
 * (nullable, 72 B = id || round u64 LE || origin): the current header of sanitize_vote.
 * codes[i] = NWC_DAG_*; digests32 (nullable): the message's digest; kinds (nullable):
 * 0 header, 1 vote, 2 certificate, 3 other.  Needs nwc_set_committee_config. */
int nwc_sanitize_messages(const uint8_t* data, const uint64_t* offsets, size_t m, uint64_t gc_round,
                          const uint8_t* vote_target, int32_t* codes, uint8_t* digests32, uint8_t* kinds);

/* Device-resident variant: d_data (4-byte aligned, >= 16 readable bytes past the last message)
 * and d_offsets (device u64[m+1], d_offsets[0] = 0, d_offsets[m] = total) in HBM; d_codes device
 * i32[m], d_digests32 (nullable) device m x 32 B.  Synchronises once (the vote count). */
int nwc_dev_sanitize_messages(const void* d_data, const void* d_offsets, uint64_t m, uint64_t total,
                              uint64_t gc_round, const uint8_t* vote_target, void* d_codes,
                              void* d_digests32, void* stream);

/* The batch entry with Core's state per message and Vote::new from the same call: what a batching
 * task needs when it drains frames across a state change.  Message i is judged
 * under gc_rounds[i] and target record i; a NULL gc_rounds means gc_round for every message, a NULL
 * vote_targets80 means vote_target (72 B or NULL, as nwc_sanitize_messages) for every message.  A
 * target record is 80 bytes: id (32), round (u64 LE), origin (32), one "enabled" byte of which only
 * bit 0 is read (0: no current header, every vote passes sanitize_vote's target check), seven zero
 * bytes.  codes, digests32 (nullable) and kinds (nullable) of message i are exactly those of
 * nwc_sanitize_messages on message i alone with that state; with both arrays NULL and no signer the
 * outputs are byte-identical to nwc_sanitize_messages'.
 *
 * signer (a nwc_signer, or NULL): voted[i] = 1 and vote_sigs + 64 i holds
 * Vote::new(header, signer's key).signature iff message i is a header and codes[i] is NWC_DAG_OK;
 * otherwise voted[i] = 0 and the 64 bytes are zero.  On an error < 0 every vote output is zero.
 * vote_sigs (m x 64 B) and voted (m bytes) are required with a signer (NWC_ERR_ARG) and untouched
 * without one.  The two rules of nwc_sanitizer_sanitize_vote hold here as well:
 *   - The library is stateless about voting: Core's last_voted check (core.rs:206-212) stays the
 *     caller's duty, and a signature Core decides not to send is simply dropped.
 *   - A vote is signed only AFTER the message's final code is Ok (one more launch behind the codes,
 *     one wave per message), never speculatively on unverified wire bytes.
 * A call without a signer builds no signing table and launches nothing more than
 * nwc_sanitize_messages does.  The signer may not be destroyed while a call that carries it runs.
 *
 * Devices: a host call that carries a signer is not sharded; it runs whole on the signer's device.
 * Calls without a signer shard as nwc_sanitize_messages does.  Conventions as everywhere here: null
 * data, offsets or codes give NWC_ERR_ARG, NWC_ERR_NOT_INIT before nwc_init and before
 * nwc_set_committee_config; m == 0 is a no-op returning 0 (whatever else is passed, a signer with
 * NULL vote outputs excepted). */
int nwc_sanitize_messages_ex(const uint8_t* data, const uint64_t* offsets, size_t m,
                             const uint64_t* gc_rounds,      /* m values, or NULL: gc_round for every message */
                             uint64_t gc_round,
                             const uint8_t* vote_targets80,  /* m x 80 B, or NULL: vote_target for every message */
                             const uint8_t* vote_target,     /* 72 B or NULL */
                             void* signer,                   /* nwc_signer or NULL */
                             int32_t* codes, uint8_t* digests32, uint8_t* kinds,
                             uint8_t* vote_sigs,             /* m x 64 B, required with a signer */
                             uint8_t* voted);                /* m bytes, required with a signer */

/* Device-resident variant: d_data, d_offsets, total, d_codes, d_digests32 and stream as
 * nwc_dev_sanitize_messages; d_gc_rounds (nullable, device u64[m], 8-byte aligned),
 * d_vote_targets80 (nullable, device m x 80 B, 4-byte aligned), d_kinds (nullable, device m bytes),
 * d_vote_sigs (device m x 64 B, 4-byte aligned) and d_voted (device m bytes) are the twins of the
 * host entry's arrays; vote_target stays a host pointer.  With a signer, d_digests32 may be NULL
 * and is otherwise 16-byte aligned.  The signer must live on the calling thread's device
 * (nwc_dev_set_device; NWC_ERR_ARG otherwise).  Synchronises once (the vote count); the codes, the
 * votes and the kinds are queued on `stream` behind it. */
int nwc_dev_sanitize_messages_ex(const void* d_data, const void* d_offsets, uint64_t m, uint64_t total,
                                 const void* d_gc_rounds, uint64_t gc_round, const void* d_vote_targets80,
                                 const uint8_t* vote_target, void* signer, void* d_codes, void* d_digests32,
                                 void* d_kinds, void* d_vote_sigs, void* d_voted, void* stream);

/* Decoded message views: the batch entries hand back what the device decoded, so that Core does not
 * deserialise the message a second time.  A view is an index
 * into the wire bytes the caller still holds plus what the wire does not contain in usable form: the
 * message's own keys decoded (32 raw bytes and the committee index), a certificate's voters as
 * committee indices, and the canonical BTreeMap / BTreeSet form of a payload or of parents that did
 * NOT arrive strictly ascending.  Honest encoders send them ascending: those stay in the wire and the
 * view gives their offsets.  One fixed record per message (160 bytes, little-endian, 8-byte aligned)
 * and a small variable part in `body`. */
#define NWC_VIEW_PAYLOAD_IN_BODY 1
#define NWC_VIEW_PARENTS_IN_BODY 2
typedef struct nwc_msg_view {
  uint8_t decoded;      /* 1 iff the message decoded: every code except SERIALIZATION_ERROR,
                           UNEXPECTED_MESSAGE and DECODE_PANIC.  0: kind and code are set, all else zero */
  uint8_t kind;         /* as kinds[i] */
  uint8_t flags;        /* NWC_VIEW_PAYLOAD_IN_BODY | NWC_VIEW_PARENTS_IN_BODY */
  uint8_t reserved0;    /* 0 */
  int32_t code;         /* == codes[i] */
  uint64_t round;       /* Header.round (certificate: its header's) / Vote.round */
  uint8_t author[32];   /* decoded key: Header.author / Vote.author */
  uint8_t origin[32];   /* Vote.origin; zero for headers and certificates */
  uint8_t id[32];       /* Header.id / Vote.id, as on the wire */
  int32_t author_index; /* index in the order of the committee configuration's keys, -1 = not a member */
  int32_t origin_index; /* votes only; -1 otherwise */
  uint32_t n_payload;   /* canonical counts: after dedupe, a map key keeps its LAST value */
  uint32_t n_parents;
  uint32_t n_votes;     /* certificates; 0 otherwise */
  uint32_t sig_off;     /* byte offset from the message's start of the header's / vote's 64-B signature */
  uint64_t payload_off; /* IN_BODY: byte offset into body, else offset from the message's start.
                           n_payload x (32-B digest, u32 LE worker id) */
  uint64_t parents_off; /* same rule; n_parents x 32 B */
  uint64_t votes_off;   /* byte offset into body of n_votes x { int32 member_index; uint32 vote_off; }
                           (0 when n_votes is 0); vote_off = offset from the message's start of the
                           vote's key string (its u64 length field); the signature follows the string */
} nwc_msg_view;

/* The bytes of body a call over m messages in `total` wire bytes can use at most: total + 64 m.  (A
 * message's body holds at most 36 P + 32 Q + 8 V bytes in three 16-byte-aligned areas, less than its
 * wire length + 64.) */
uint64_t nwc_msg_view_body_bound(uint64_t total, uint64_t m);

/* nwc_sanitize_messages_ex with the views: the first 13 arguments, codes, digests32, kinds,
 * vote_sigs and voted are exactly that entry's, byte for byte.  views: m nwc_msg_view records.
 * With views == NULL the entry IS nwc_sanitize_messages_ex: nothing more is launched or allocated
 * and body, body_cap and body_used are ignored.  With views, body and body_used are required,
 * body_cap >= nwc_msg_view_body_bound(offsets[m] - offsets[0], m), and every message is shorter
 * than 2^32 bytes: a call that breaks one of these returns NWC_ERR_ARG before anything is queued.
 *
 * The body's areas come from a bump allocator on the device in 16-byte units: their order is
 * unspecified, they never overlap, every one starts on a multiple of 16, and *body_used is the
 * allocator's final value in bytes (<= the bound).  Only the records (160 m bytes) and body_used
 * bytes of body come back, never body_cap.  On an error < 0 every view is zero and *body_used = 0.
 * The views are written by one more launch behind the codes (one wave per message), whatever the
 * number of chunks.
 *
 * Devices: a host call that asks for views is not sharded; it runs whole on the calling thread's
 * device (nwc_dev_set_device), or on the signer's when it carries one.  m == 0 is a no-op returning
 * 0; NWC_ERR_NOT_INIT before nwc_init and before nwc_set_committee_config.  The sanitizer handle
 * keeps returning code, digest and kind only. */
int nwc_sanitize_messages_view(const uint8_t* data, const uint64_t* offsets, size_t m,
                               const uint64_t* gc_rounds, uint64_t gc_round,
                               const uint8_t* vote_targets80, const uint8_t* vote_target, void* signer,
                               int32_t* codes, uint8_t* digests32, uint8_t* kinds,
                               uint8_t* vote_sigs, uint8_t* voted,
                               void* views,            /* m nwc_msg_view records, or NULL */
                               uint8_t* body, size_t body_cap,
                               uint64_t* body_used);   /* bytes of body in use */

/* Device-resident variant: the arguments of nwc_dev_sanitize_messages_ex, then d_views (device
 * m x 160 B, 8-byte aligned), d_body (device, 16-byte aligned, body_cap bytes), d_body_used (device
 * u64); `stream` stays last.  d_views == NULL: nwc_dev_sanitize_messages_ex.  The offsets live on
 * the device, so a message of 2^32 bytes or more is not refused here: it gets decoded = 0.
 * Synchronises no more often than the _ex entry; the views, the body and d_body_used are queued on
 * `stream` behind the codes.  On an error < 0 the views and d_body_used are zeroed on `stream`. */
int nwc_dev_sanitize_messages_view(const void* d_data, const void* d_offsets, uint64_t m, uint64_t total,
                                   const void* d_gc_rounds, uint64_t gc_round, const void* d_vote_targets80,
                                   const uint8_t* vote_target, void* signer, void* d_codes, void* d_digests32,
                                   void* d_kinds, void* d_vote_sigs, void* d_voted, void* d_views, void* d_body,
                                   uint64_t body_cap, void* d_body_used, void* stream);

/* ---- digests -------------------------------------------------------------------------- */
/* Sha512::digest(bytes)[..32] -- worker/src/processor.rs:38 and crypto's `Hash for &[u8]`
 * (crypto/src/tests/crypto_tests.rs:8-12). */
int nwc_digest32(const uint8_t* data, size_t len, uint8_t out32[32]);
/* n messages data[offsets[i] .. offsets[i+1]) -> out32[32*i]. */
int nwc_sha512_trunc32_many(const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out32);

/* ---- device-resident variants (inputs already in HBM) ---------------------------------- */
/* strict != 0: verify_strict semantics; strict == 0: batch-leaf semantics.  msg_index
 * (nullable, device u32[n]) selects the digest of equation i; otherwise digest i*msg_stride.
 * n < 2^32 per call (NWC_ERR_ARG otherwise). */
int nwc_dev_verify(const void* d_msgs, const void* d_msg_index, uint64_t msg_stride,
                   const void* d_pks, const void* d_sigs, uint64_t n, int strict,
                   void* d_verdict_words, void* stream);
/* Per-certificate AND of leaf verdict words (d_offsets: device u32[m+1]). */
int nwc_dev_cert_reduce(const void* d_leaf_words, const void* d_offsets, uint64_t m, uint64_t nvotes,
                        void* d_cert_words, void* d_bad_words, void* stream);
/* Signature::verify_batch over m certificates as dalek's own batch equation (crypto/src/lib.rs:
 * 206-219; ed25519-dalek 1.0.1 batch.rs) over sub-batches of ~12 consecutive votes (any
 * certificates; NWC_STRAUS_NQ overrides): sum z_i R_i + sum (z_i k_i mod l) A_i -
 * (sum z_i s_i mod l) B == O with random 128-bit z_i, one Straus pass with shared doublings per
 * lane (k_verify_straus); the votes of sub-batches it rejects are then re-decided by the exact
 * per-vote leaves, so d_leaf_words (a bit per vote, as nwc_dev_verify's) feeds nwc_dev_cert_reduce
 * for the certificate verdicts and the exact bad-vote set.  d_offsets: m + 1 uint32 vote offsets
 * (checked non-null; the sub-batches do not follow them); d_msg_index: the certificate of each
 * vote.  Same verdicts and bad sets as the leaf path on the deterministic domain; on dalek's
 * randomized domain (pure-torsion residuals, torsion-bearing keys) a vote's sub-batch passes with
 * dalek's probability (~1/ord) where the leaf path answers Err.  Without the basepoint comb
 * (NWC_COMB16=0) it runs the leaves. */
int nwc_dev_verify_batch_straus(const void* d_digests, const void* d_offsets, const void* d_msg_index, uint64_t m,
                                uint64_t nvotes, const void* d_pks, const void* d_sigs, void* d_leaf_words,
                                void* stream);
/* Signature::verify_batch over m certificates with dalek's batch semantics, device-resident (as
 * nwc_verify_batch_msm_many).  With key combs (committee cache, or launch keys at >= 65,536 votes):
 * the comb-path leaves, then dalek's equation per certificate over the leaves' failing votes, in
 * E[8].  Without: dalek's batch equation as a Pippenger MSM per group of
 * consecutive votes (up to 4,096, sized so the groups fill whole rounds of the resident waves;
 * NWC_MSM_GROUP / nwc_diag_set("msm_group") fixes it): one wave per group sorts its points into 512
 * buckets per 10-bit window in LDS and reduces the buckets across its 64 lanes; the votes of groups
 * that fail go to the exact per-vote leaves (no second random equation: on dalek's randomized
 * domain a vote passes iff its group's equation holds).  Skip policy (device-side, no host
 * synchronisation; its state is per device, shared by every caller and stream of the device): when
 * more than half of a launch's groups fail (a bad-vote rate of about one per group or more), the next
 * 7 launches skip the equation and hand every vote straight to the leaves; the one after them runs
 * it on every group again and decides anew.  d_leaf_words as nwc_dev_verify_batch_straus's. */
int nwc_dev_verify_batch_msm(const void* d_digests, const void* d_offsets, const void* d_msg_index, uint64_t m,
                             uint64_t nvotes, const void* d_pks, const void* d_sigs, void* d_leaf_words,
                             void* stream);
/* Groups of the MSM entry on the calling thread's device since nwc_init: passed (their votes'
 * bits set by the equation), failed (re-decided by the leaves), of the failed ones, groups with
 * more distinct keys than the LDS key table holds (126), and groups the skip policy handed to the
 * leaves without the equation.  Any pointer may be null.  Waits for the device.  Diagnostics
 * only. */
int nwc_msm_stats(uint64_t* groups_passed, uint64_t* groups_failed, uint64_t* key_overflows, uint64_t* groups_skipped);
int nwc_dev_sha512_trunc32(const void* d_data, const void* d_offsets, uint64_t n, void* d_out32,
                           void* stream);
/* Same, message i = d_data[d_starts[i] .. d_ends[i]) (device u64 arrays): any layout, e.g. a
 * pool of resident batches hashed repeatedly.  Starts 16-byte aligned take the fast path. */
int nwc_dev_sha512_trunc32_ranges(const void* d_data, const void* d_starts, const void* d_ends, uint64_t n,
                                  void* d_out32, void* stream);
/* Synthetic workload generation (BASELINE configs 2/3/5): out_i = SHA-512(tag||u64le(first+i))[..32]
 * and RFC 8032 keygen+sign of (seed_i, msg_i): a key per lane, derived anew on every call.  For
 * signing with a node's key use a signer (above). */
int nwc_dev_derive32(const uint8_t* tag, int taglen, uint64_t first, uint64_t n, void* d_out,
                     void* stream);
int nwc_dev_keygen_sign(const void* d_seeds, const void* d_msgs, uint64_t n, void* d_pks,
                        void* d_sigs, void* stream);
/* Select the HIP device used by nwc_dev_* on the calling thread (index into the init mask). */
int nwc_dev_set_device(int device);

/* ---- sharding (host only; no device needed) --------------------------------------------- */
/* independent units split over `world` GPUs/ranks.  [*lo, *hi) of n units for
 * `rank`: contiguous, every shard but the last starts on a multiple of 64 (whole verdict words),
 * so shards never share a byte of a verdict bitmap.  Used by the host entry points' per-device
 * threads and mirrored by narwhal_amd/shard.py shard_bounds for one-process-per-GPU runs. */
int nwc_shard_bounds(uint64_t n, uint32_t world, uint32_t rank, uint64_t* lo, uint64_t* hi);
/* Vote-index cuts (world + 1 values, cuts[0] = 0, cuts[world] = offsets[m]) on certificate
 * boundaries, balanced by vote count: a certificate's votes never split (config 3). */
int nwc_cert_cuts(const uint32_t* offsets, size_t m, uint32_t world, uint64_t* cuts);

#ifdef __cplusplus
}
#endif
#endif /* NWC_H */
