//! `crypto_nwc`: the device side of Narwhal's `crypto` crate (/root/reference/crypto/src/lib.rs).
//!
//! The reference crate keeps its types and API; its verification bodies forward here
//!:
//!
//! ```ignore
//! // crypto/src/lib.rs:200-204  Signature::verify
//! pub fn verify(&self, digest: &Digest, public_key: &PublicKey) -> Result<(), CryptoError> {
//!     if crypto_nwc::verify_strict(&digest.0, &public_key.0, &self.flatten()) { Ok(()) }
//!     else { Err(CryptoError::new()) }
//! }
//! // crypto/src/lib.rs:206-219  Signature::verify_batch
//! pub fn verify_batch<'a, I>(digest: &Digest, votes: I) -> Result<(), CryptoError>
//! where I: IntoIterator<Item = &'a (PublicKey, Signature)> {
//!     let (pks, sigs): (Vec<[u8; 32]>, Vec<[u8; 64]>) =
//!         votes.into_iter().map(|(k, s)| (k.0, s.flatten())).unzip();
//!     if crypto_nwc::verify_batch(&digest.0, &pks, &sigs) { Ok(()) } else { Err(CryptoError::new()) }
//! }
//! // worker/src/processor.rs:38
//! let digest = Digest(crypto_nwc::digest32(&batch));
//! // crypto/src/lib.rs:180-191  Signature::new, with a Signer made once from the node's SecretKey
//! let sig = signer.sign(&digest.0);   // part1 = sig[..32], part2 = sig[32..]
//! ```
//!
//! Return convention of the C ABI: 0 = valid, 1 = invalid, < 0 = device/runtime failure, which
//! is never reported as an invalid signature -- these wrappers panic on it, as the crate's
//! callers have no error path for a broken device.
mod ffi;

pub use ffi::*;

use std::ffi::CStr;
use std::os::raw::c_int;
use std::sync::Once;

static INIT: Once = Once::new();

/// `nwc_init(device_mask)` once per process (node start-up, node/src/main.rs:69-134).  Later
/// calls are no-ops; the wrappers below call it with mask 0 (device 0) if nobody did.
pub fn init(device_mask: u32) {
    INIT.call_once(|| {
        let rc = unsafe { ffi::nwc_init(device_mask) };
        check(rc);
    });
}

/// The hash of the sources and flags the linked libnwc.so was compiled from (nwc_build_id):
/// build.rs compiles with the repository's recipe (narwhal_amd/build.py --hipcc-args), so this
/// equals `python3 narwhal_amd/build.py --source-id` of the same tree; "unknown" for other builds.
pub fn build_id() -> String {
    unsafe { CStr::from_ptr(ffi::nwc_build_id()) }.to_string_lossy().into_owned()
}

fn check(rc: c_int) -> bool {
    if rc < 0 {
        let msg = unsafe { CStr::from_ptr(ffi::nwc_last_error()) };
        panic!("libnwc failure {}: {}", rc, msg.to_string_lossy());
    }
    rc == 0
}

/// `Signature::verify` = dalek `verify_strict` (crypto/src/lib.rs:200-204).
pub fn verify_strict(digest: &[u8; 32], public_key: &[u8; 32], signature: &[u8; 64]) -> bool {
    init(0);
    check(unsafe { ffi::nwc_verify_strict(digest.as_ptr(), public_key.as_ptr(), signature.as_ptr()) })
}

/// `Signature::verify_batch` = dalek `verify_batch` over one digest (crypto/src/lib.rs:206-219).
/// An empty batch is valid.
pub fn verify_batch(digest: &[u8; 32], public_keys: &[[u8; 32]], signatures: &[[u8; 64]]) -> bool {
    assert_eq!(public_keys.len(), signatures.len());
    init(0);
    let pks: Vec<u8> = public_keys.iter().flat_map(|k| k.iter().copied()).collect();
    let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.iter().copied()).collect();
    check(unsafe {
        ffi::nwc_verify_batch(digest.as_ptr(), pks.as_ptr(), sigs.as_ptr(), public_keys.len(), std::ptr::null_mut())
    })
}

/// Many certificates at once (certificate c = `digests[c]` over votes `offsets[c]..offsets[c+1]`):
/// per-certificate verdicts and the bad-vote set.  `dalek_batch = false`: the exact per-vote leaves
/// (deterministic; Err on dalek's randomized domain); `true`: dalek's batch semantics -- each
/// certificate passes iff dalek's random-linear-combination equation holds for it: the comb-path
/// leaves for every vote, then the equation once per certificate over the votes they rejected
/// (exact in the 8-torsion group; the committee's repeated keys give the comb path without
/// `set_committee`), or, where no key combs apply, a Pippenger MSM per group of votes with the
/// leaves for the groups it rejects.  Each vote meets at most one random equation.  Returns
/// (certificate ok, vote bad) as bitmaps.
pub fn verify_batch_many(digests: &[[u8; 32]], offsets: &[u32], public_keys: &[[u8; 32]], signatures: &[[u8; 64]],
                         dalek_batch: bool) -> (Vec<u8>, Vec<u8>) {
    let m = digests.len();
    assert_eq!(offsets.len(), m + 1);
    assert_eq!(public_keys.len(), signatures.len());
    assert_eq!(offsets[m] as usize, public_keys.len());
    init(0);
    let dg: Vec<u8> = digests.iter().flat_map(|d| d.iter().copied()).collect();
    let pks: Vec<u8> = public_keys.iter().flat_map(|k| k.iter().copied()).collect();
    let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.iter().copied()).collect();
    let mut ok = vec![0u8; (m + 7) / 8];
    let mut bad = vec![0u8; (public_keys.len() + 7) / 8];
    let f = if dalek_batch { ffi::nwc_verify_batch_msm_many } else { ffi::nwc_verify_batch_many };
    let rc = unsafe { f(dg.as_ptr(), offsets.as_ptr(), pks.as_ptr(), sigs.as_ptr(), m, ok.as_mut_ptr(), bad.as_mut_ptr()) };
    assert!(rc == 0, "libnwc failure {}", rc);
    (ok, bad)
}

/// `Sha512::digest(bytes)[..32]` (worker/src/processor.rs:38).
pub fn digest32(data: &[u8]) -> [u8; 32] {
    init(0);
    let mut out = [0u8; 32];
    check(unsafe { ffi::nwc_digest32(data.as_ptr(), data.len(), out.as_mut_ptr()) });
    out
}

/// The committee's keys (config/src/lib.rs:154-156), cached on the devices.  Optional: verdicts
/// never depend on it.
pub fn set_committee(public_keys: &[[u8; 32]]) {
    init(0);
    let pks: Vec<u8> = public_keys.iter().flat_map(|k| k.iter().copied()).collect();
    check(unsafe { ffi::nwc_set_committee(pks.as_ptr(), public_keys.len()) });
}

/// The worker's grouped batch digests (worker/src/processor.rs:35-55): a libnwc digester whose
/// drain thread hashes whatever has queued up (up to `max_group` batches, or what arrived within
/// `max_wait_us` of the first) in one GPU launch.  Batches are borrowed until their digest comes
/// back, so the queue owns them here and hands each back with its digest, in submission order.
pub struct BatchDigester {
    q: *mut ffi::nwc_digester,
    next_tag: u64,
    held: std::collections::VecDeque<(u64, Vec<u8>)>,
}

unsafe impl Send for BatchDigester {}

impl BatchDigester {
    pub fn new(max_group: u32, max_wait_us: u32) -> Self {
        init(0);
        let q = unsafe { ffi::nwc_digester_create(max_group, max_wait_us) };
        if q.is_null() {
            let msg = unsafe { CStr::from_ptr(ffi::nwc_last_error()) };
            panic!("libnwc digester: {}", msg.to_string_lossy());
        }
        BatchDigester { q, next_tag: 0, held: std::collections::VecDeque::new() }
    }

    /// Queue a batch (the Processor's `rx_batch.recv()`); it comes back from `next`.
    pub fn submit(&mut self, batch: Vec<u8>) {
        let tag = self.next_tag;
        self.next_tag += 1;
        check(unsafe { ffi::nwc_digester_submit(self.q, batch.as_ptr(), batch.len(), tag) });
        self.held.push_back((tag, batch));   // the Vec's heap buffer does not move
    }

    /// The oldest outstanding batch with its digest, waiting up to `wait_us` (None on timeout).
    /// A batch whose group failed on the device comes back as `Err(batch)` -- the caller keeps
    /// it (to hash on the CPU, retry or drop) -- so `held` and the returned tags never diverge;
    /// the library's sticky error with nothing left to return panics like every device error.
    pub fn next(&mut self, wait_us: u32) -> Option<Result<([u8; 32], Vec<u8>), Vec<u8>>> {
        if self.held.is_empty() {
            return None;
        }
        let (mut tag, mut dig, mut n) = (0u64, [0u8; 32], 0usize);
        let rc = unsafe { ffi::nwc_digester_poll(self.q, 1, wait_us, &mut tag, dig.as_mut_ptr(), &mut n) };
        if n == 0 {
            check(rc);
            return None;
        }
        let (t, batch) = self.held.pop_front().unwrap();
        assert_eq!(t, tag, "digests come back in submission order");
        Some(if rc < 0 { Err(batch) } else { Ok((dig, batch)) })
    }
}

impl Drop for BatchDigester {
    fn drop(&mut self) {
        unsafe { ffi::nwc_digester_destroy(self.q) };
    }
}

/// `generate_keypair` (crypto/src/lib.rs:167-175): `seed || A` (dalek `Keypair::to_bytes`) for 32
/// bytes of the caller's CSPRNG.
pub fn keypair_from_seed(seed: &[u8; 32]) -> [u8; 64] {
    init(0);
    let mut out = [0u8; 64];
    check(unsafe { ffi::nwc_keypair_from_seed(seed.as_ptr(), out.as_mut_ptr()) });
    out
}

/// A registered signing key (`nwc_signer`): what `Signature::new` and `SignatureService`
/// (crypto/src/lib.rs:180-191, 222-250) sign with.  The key is expanded once into device memory;
/// dropping the signer zeroes and frees that copy.  Unlike dalek 1.0.1's `Keypair::from_bytes`,
/// `new` refuses a secret whose public half is not the seed's (`None`).
pub struct Signer {
    h: *mut std::os::raw::c_void,
}

unsafe impl Send for Signer {}
unsafe impl Sync for Signer {}   // libnwc serialises calls on one signer

impl Signer {
    /// `secret64` = `SecretKey` bytes (seed || public key).  `None` for a mismatched public half;
    /// panics on a device failure.
    pub fn new(secret64: &[u8; 64]) -> Option<Self> {
        init(0);
        let h = unsafe { ffi::nwc_signer_create(secret64.as_ptr()) };
        if h.is_null() {
            if unsafe { ffi::nwc_last_error_code() } == -2 {
                return None;
            }
            let msg = unsafe { CStr::from_ptr(ffi::nwc_last_error()) };
            panic!("libnwc signer: {}", msg.to_string_lossy());
        }
        Some(Signer { h })
    }

    pub fn public_key(&self) -> [u8; 32] {
        let mut pk = [0u8; 32];
        check(unsafe { ffi::nwc_signer_public_key(self.h, pk.as_mut_ptr()) });
        pk
    }

    /// `Signature::new(digest, secret)`: R || s.
    pub fn sign(&self, digest: &[u8; 32]) -> [u8; 64] {
        let mut sig = [0u8; 64];
        check(unsafe { ffi::nwc_signer_sign(self.h, digest.as_ptr(), sig.as_mut_ptr()) });
        sig
    }

    /// One launch for all of `digests`: what a `SignatureService` task drains from its channel.
    pub fn sign_many(&self, digests: &[[u8; 32]]) -> Vec<[u8; 64]> {
        let mut sigs = vec![[0u8; 64]; digests.len()];
        check(unsafe {
            ffi::nwc_signer_sign_many(self.h, digests.as_ptr() as *const u8, digests.len(), sigs.as_mut_ptr() as *mut u8)
        });
        sigs
    }

    /// `Vote::new(header, ..).signature` (primary/src/messages.rs:115-129) for a header the caller
    /// has accepted: the signature of SHA-512(id || round LE || origin)[..32], digest and signature
    /// in one launch.
    pub fn vote(&self, id: &[u8; 32], round: u64, origin: &[u8; 32]) -> [u8; 64] {
        let mut sig = [0u8; 64];
        check(unsafe { ffi::nwc_signer_vote(self.h, id.as_ptr(), round, origin.as_ptr(), sig.as_mut_ptr()) });
        sig
    }

    /// One launch for all of a round's votes: (ids[i], rounds[i], origins[i]) -> signature i.
    pub fn vote_many(&self, ids: &[[u8; 32]], rounds: &[u64], origins: &[[u8; 32]]) -> Vec<[u8; 64]> {
        assert!(ids.len() == rounds.len() && ids.len() == origins.len());
        let mut sigs = vec![[0u8; 64]; ids.len()];
        check(unsafe {
            ffi::nwc_signer_vote_many(self.h, ids.as_ptr() as *const u8, rounds.as_ptr(), origins.as_ptr() as *const u8,
                                      ids.len(), sigs.as_mut_ptr() as *mut u8)
        });
        sigs
    }
}

impl Drop for Signer {
    fn drop(&mut self) {
        unsafe { ffi::nwc_signer_destroy(self.h) };
    }
}

/// Concurrent `Signature::verify` / `verify_batch` calls behind shared launches (`nwc_verifier`):
/// tokio tasks that verify at the same time (node/src/main.rs:17, worker/src/worker.rs:182,227)
/// call one process-wide `Verifier`; requests that arrive together share a launch and each caller
/// returns when its own verdicts are in.  Same verdicts as `verify_strict` / `verify_batch`.
pub struct Verifier {
    h: *mut std::os::raw::c_void,
}

unsafe impl Send for Verifier {}
unsafe impl Sync for Verifier {}   // every call on a verifier may be made from any number of threads

/// Counters of a `Verifier` (`nwc_verifier_stats_t`).
#[repr(C)]
#[derive(Default, Debug, Clone, Copy)]
pub struct VerifierStats {
    pub groups: u64,
    pub requests: u64,
    pub equations: u64,
    pub wide_equations: u64,
    pub cold_equations: u64,
    pub redone_equations: u64,
    pub bypassed_requests: u64,
    pub max_requests_in_group: u64,
}

impl Verifier {
    /// A group closes at `max_requests` requests (0 = as many as fit) or `max_wait_us` after its
    /// first request (0 = never wait for company).  Panics on a device failure.
    pub fn new(max_requests: u32, max_wait_us: u32) -> Self {
        init(0);
        let h = unsafe { ffi::nwc_verifier_create(max_requests, max_wait_us) };
        if h.is_null() {
            let msg = unsafe { CStr::from_ptr(ffi::nwc_last_error()) };
            panic!("libnwc verifier: {}", msg.to_string_lossy());
        }
        Verifier { h }
    }

    /// `Signature::verify` = dalek `verify_strict`.
    pub fn verify(&self, digest: &[u8; 32], public_key: &[u8; 32], signature: &[u8; 64]) -> bool {
        check(unsafe { ffi::nwc_verifier_verify_strict(self.h, digest.as_ptr(), public_key.as_ptr(), signature.as_ptr()) })
    }

    /// `Signature::verify_batch` over one digest.  An empty batch is valid.
    pub fn verify_batch(&self, digest: &[u8; 32], public_keys: &[[u8; 32]], signatures: &[[u8; 64]]) -> bool {
        assert_eq!(public_keys.len(), signatures.len());
        check(unsafe {
            ffi::nwc_verifier_verify_batch(self.h, digest.as_ptr(), public_keys.as_ptr() as *const u8,
                                           signatures.as_ptr() as *const u8, public_keys.len(), std::ptr::null_mut())
        })
    }

    pub fn stats(&self) -> VerifierStats {
        let mut s = VerifierStats::default();
        check(unsafe { ffi::nwc_verifier_stats(self.h, &mut s as *mut VerifierStats as *mut u64) });
        s
    }
}

impl Drop for Verifier {
    fn drop(&mut self) {
        unsafe { ffi::nwc_verifier_destroy(self.h) };
    }
}

/// Concurrent wire messages behind shared pipeline launches (`nwc_sanitizer`): the tasks of
/// `PrimaryReceiverHandler::dispatch` (primary/src/primary.rs:224-240) call one process-wide
/// `Sanitizer`, each with the bincode `PrimaryMessage` it received; messages that arrive together
/// share one set of launches and each caller returns when its own verdict is in.  Same codes,
/// digests and kinds as `nwc_sanitize_messages` on the message alone.  The committee is the one
/// last given to `nwc_set_committee_config`.
pub struct Sanitizer {
    h: *mut std::os::raw::c_void,
}

unsafe impl Send for Sanitizer {}
unsafe impl Sync for Sanitizer {}   // every call on a sanitizer may be made from any number of threads

/// Counters of a `Sanitizer` (`nwc_sanitizer_stats_t`).
#[repr(C)]
#[derive(Default, Debug, Clone, Copy)]
pub struct SanitizerStats {
    pub groups: u64,
    pub messages: u64,
    pub bytes: u64,
    pub equations: u64,
    pub redone_messages: u64,
    pub bypassed_messages: u64,
    pub max_messages_in_group: u64,
    pub reserved: u64,
}

/// What `Core::sanitize_*` says about one wire message.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct Verdict {
    /// `NWC_DAG_*`: 0 = Ok, otherwise the `DagError` variant.
    pub code: u32,
    /// `Header::digest` / `Vote::digest` / `Certificate::digest` of the message.
    pub digest: [u8; 32],
    /// 0 header, 1 vote, 2 certificate, 3 anything else.
    pub kind: u8,
}

impl Sanitizer {
    /// A group closes at `max_messages` messages (0 = as many as fit) or `max_wait_us` after it was
    /// opened (0 = never wait for company).  Panics on a device failure, and before
    /// `nwc_set_committee_config`.
    pub fn new(max_messages: u32, max_wait_us: u32) -> Self {
        init(0);
        let h = unsafe { ffi::nwc_sanitizer_create(max_messages, max_wait_us) };
        if h.is_null() {
            let msg = unsafe { CStr::from_ptr(ffi::nwc_last_error()) };
            panic!("libnwc sanitizer: {}", msg.to_string_lossy());
        }
        Sanitizer { h }
    }

    /// One wire message under the caller's `gc_round` and, for votes, the current header
    /// (`id || round (LE) || author`, 72 bytes).  Panics on a device failure.
    pub fn sanitize(&self, wire: &[u8], gc_round: u64, vote_target: Option<&[u8; 72]>) -> Verdict {
        let mut v = Verdict { code: 0, digest: [0u8; 32], kind: 3 };
        let rc = unsafe {
            ffi::nwc_sanitizer_sanitize(self.h, wire.as_ptr(), wire.len(), gc_round,
                                        vote_target.map_or(std::ptr::null(), |t| t.as_ptr()), v.digest.as_mut_ptr(), &mut v.kind)
        };
        check(rc);
        v.code = rc as u32;
        v
    }

    /// `sanitize`, and for a header whose code is Ok the signature of `Vote::new(header, ..)` under
    /// `signer`'s key from the same flight.  The library keeps no voting state: Core's `last_voted`
    /// check stays with the caller, and a vote is signed only after the header's code is Ok.
    /// `signer` must live on the sanitizer's device.  Panics on a device failure.
    pub fn sanitize_vote(&self, signer: &Signer, wire: &[u8], gc_round: u64,
                         vote_target: Option<&[u8; 72]>) -> (Verdict, Option<[u8; 64]>) {
        let mut v = Verdict { code: 0, digest: [0u8; 32], kind: 3 };
        let mut sig = [0u8; 64];
        let mut voted: i32 = 0;
        let rc = unsafe {
            ffi::nwc_sanitizer_sanitize_vote(self.h, signer.h, wire.as_ptr(), wire.len(), gc_round,
                                             vote_target.map_or(std::ptr::null(), |t| t.as_ptr()), v.digest.as_mut_ptr(),
                                             &mut v.kind, sig.as_mut_ptr(), &mut voted)
        };
        check(rc);
        v.code = rc as u32;
        (v, if voted != 0 { Some(sig) } else { None })
    }

    /// `sanitize_vote` (`signer`: `None` = `sanitize`) plus what the device decoded, from the same
    /// flight: the message's `MsgView` and the body its offsets point into (`ViewEntries::new(&view,
    /// wire, &body)`), so that Core does not deserialise the frame again.  Panics on a device failure.
    pub fn sanitize_view(&self, signer: Option<&Signer>, wire: &[u8], gc_round: u64,
                         vote_target: Option<&[u8; 72]>) -> (Verdict, Option<[u8; 64]>, MsgView, Vec<u8>) {
        let mut v = Verdict { code: 0, digest: [0u8; 32], kind: 3 };
        let mut sig = [0u8; 64];
        let mut voted: i32 = 0;
        let mut view: MsgView = unsafe { std::mem::zeroed() };
        let cap = unsafe { ffi::nwc_msg_view_body_bound(wire.len() as u64, 1) };
        let mut body = vec![0u8; cap as usize];
        let mut used: u64 = 0;
        let rc = unsafe {
            ffi::nwc_sanitizer_sanitize_view(self.h, signer.map_or(std::ptr::null_mut(), |s| s.h), wire.as_ptr(), wire.len(),
                                             gc_round, vote_target.map_or(std::ptr::null(), |t| t.as_ptr()),
                                             v.digest.as_mut_ptr(), &mut v.kind, sig.as_mut_ptr(), &mut voted,
                                             &mut view as *mut MsgView as *mut std::ffi::c_void, body.as_mut_ptr(), cap, &mut used)
        };
        check(rc);
        v.code = rc as u32;
        body.truncate(used as usize);
        (v, if voted != 0 { Some(sig) } else { None }, view, body)
    }

    /// Views delivered by a group flight / by the one-message fallback.
    pub fn view_stats(&self) -> (u64, u64) {
        let (mut in_flight, mut alone) = (0u64, 0u64);
        check(unsafe { ffi::nwc_sanitizer_view_stats(self.h, &mut in_flight, &mut alone) });
        (in_flight, alone)
    }

    /// Votes signed inside a group flight / by the one-message fallback.
    pub fn vote_stats(&self) -> (u64, u64) {
        let (mut in_flight, mut alone) = (0u64, 0u64);
        check(unsafe { ffi::nwc_sanitizer_vote_stats(self.h, &mut in_flight, &mut alone) });
        (in_flight, alone)
    }

    pub fn stats(&self) -> SanitizerStats {
        let mut s = SanitizerStats::default();
        check(unsafe { ffi::nwc_sanitizer_stats(self.h, &mut s as *mut SanitizerStats as *mut u64) });
        s
    }
}

impl Drop for Sanitizer {
    fn drop(&mut self) {
        unsafe { ffi::nwc_sanitizer_destroy(self.h) };
    }
}

/// Core's state as it was when one frame was received: `gc_round`, and for votes the current
/// header (`id || round (LE) || author`, 72 bytes; `None`: no current header).
#[derive(Debug, Clone, Copy)]
pub struct FrameState<'a> {
    pub gc_round: u64,
    pub vote_target: Option<&'a [u8; 72]>,
}

/// The batch entry with Core's state per message and `Vote::new` from the same call
/// (`nwc_sanitize_messages_ex`): what a batching task calls with the frames it drained, each with
/// the `FrameState` recorded when it arrived.  Message `i` is `wires[i]`; its
/// verdict is that of `nwc_sanitize_messages` on it alone under `states[i]`.  With a `signer`,
/// every header whose code is Ok comes back with the signature of `Vote::new(header, ..)` under
/// the signer's key; the call then runs whole on the signer's device.  The library keeps no voting
/// state: Core's `last_voted` check stays with the caller, and a vote is signed only after the
/// header's code is Ok.  The committee is the one last given to `nwc_set_committee_config`.
/// Panics on a device failure.
pub fn sanitize_batch(wires: &[&[u8]], states: &[FrameState], signer: Option<&Signer>) -> Vec<(Verdict, Option<[u8; 64]>)> {
    assert_eq!(wires.len(), states.len());
    init(0);
    let m = wires.len();
    if m == 0 {
        return Vec::new();
    }
    let mut offsets = Vec::with_capacity(m + 1);
    let mut data = Vec::new();
    offsets.push(0u64);
    for w in wires {
        data.extend_from_slice(w);
        offsets.push(data.len() as u64);
    }
    data.push(0);   // never an empty buffer
    let gc_rounds: Vec<u64> = states.iter().map(|s| s.gc_round).collect();
    // the 80-byte record: id, round LE, origin, the "enabled" byte, seven zero bytes
    let mut targets = vec![0u8; 80 * m];
    for (i, s) in states.iter().enumerate() {
        if let Some(t) = s.vote_target {
            targets[80 * i..80 * i + 72].copy_from_slice(t);
            targets[80 * i + 72] = 1;
        }
    }
    let mut codes = vec![0i32; m];
    let mut digests = vec![0u8; 32 * m];
    let mut kinds = vec![3u8; m];
    let mut sigs = vec![0u8; 64 * m];
    let mut voted = vec![0u8; m];
    let rc = unsafe {
        ffi::nwc_sanitize_messages_ex(data.as_ptr(), offsets.as_ptr(), m, gc_rounds.as_ptr(), 0, targets.as_ptr(), std::ptr::null(),
                                      signer.map_or(std::ptr::null_mut(), |s| s.h), codes.as_mut_ptr(), digests.as_mut_ptr(),
                                      kinds.as_mut_ptr(), if signer.is_some() { sigs.as_mut_ptr() } else { std::ptr::null_mut() },
                                      if signer.is_some() { voted.as_mut_ptr() } else { std::ptr::null_mut() })
    };
    check(rc);
    (0..m).map(|i| {
        let mut v = Verdict { code: codes[i] as u32, digest: [0u8; 32], kind: kinds[i] };
        v.digest.copy_from_slice(&digests[32 * i..32 * i + 32]);
        let sig = if voted[i] != 0 {
            let mut s = [0u8; 64];
            s.copy_from_slice(&sigs[64 * i..64 * i + 64]);
            Some(s)
        } else {
            None
        };
        (v, sig)
    }).collect()
}

pub use ffi::nwc_msg_view as MsgView;

/// The views of one `sanitize_batch_view` call: a record per message and the body they share.
pub struct BatchViews {
    pub views: Vec<MsgView>,
    pub body: Vec<u8>,
}

/// `sanitize_batch` with the decoded views (`nwc_sanitize_messages_view`): what the device decoded
/// comes back, so Core builds its `Header` / `Vote` / `Certificate` from `(view, wire)` without
/// bincode or base64.  Verdicts and votes are exactly `sanitize_batch`'s.  The
/// call is not sharded: it runs whole on the calling thread's device, or on the signer's.
/// Panics on a device failure.
pub fn sanitize_batch_view(wires: &[&[u8]], states: &[FrameState], signer: Option<&Signer>)
                           -> (Vec<(Verdict, Option<[u8; 64]>)>, BatchViews) {
    assert_eq!(wires.len(), states.len());
    init(0);
    let m = wires.len();
    if m == 0 {
        return (Vec::new(), BatchViews { views: Vec::new(), body: Vec::new() });
    }
    let mut offsets = Vec::with_capacity(m + 1);
    let mut data = Vec::new();
    offsets.push(0u64);
    for w in wires {
        data.extend_from_slice(w);
        offsets.push(data.len() as u64);
    }
    let total = data.len() as u64;
    data.push(0);   // never an empty buffer
    let gc_rounds: Vec<u64> = states.iter().map(|s| s.gc_round).collect();
    let mut targets = vec![0u8; 80 * m];
    for (i, s) in states.iter().enumerate() {
        if let Some(t) = s.vote_target {
            targets[80 * i..80 * i + 72].copy_from_slice(t);
            targets[80 * i + 72] = 1;
        }
    }
    let mut codes = vec![0i32; m];
    let mut digests = vec![0u8; 32 * m];
    let mut kinds = vec![3u8; m];
    let mut sigs = vec![0u8; 64 * m];
    let mut voted = vec![0u8; m];
    let mut views: Vec<MsgView> = vec![unsafe { std::mem::zeroed() }; m];
    let cap = unsafe { ffi::nwc_msg_view_body_bound(total, m as u64) } as usize;
    let mut body = vec![0u8; cap];
    let mut used = 0u64;
    let rc = unsafe {
        ffi::nwc_sanitize_messages_view(data.as_ptr(), offsets.as_ptr(), m, gc_rounds.as_ptr(), 0, targets.as_ptr(), std::ptr::null(),
                                        signer.map_or(std::ptr::null_mut(), |s| s.h), codes.as_mut_ptr(), digests.as_mut_ptr(),
                                        kinds.as_mut_ptr(), if signer.is_some() { sigs.as_mut_ptr() } else { std::ptr::null_mut() },
                                        if signer.is_some() { voted.as_mut_ptr() } else { std::ptr::null_mut() },
                                        views.as_mut_ptr() as *mut std::os::raw::c_void, body.as_mut_ptr(), cap, &mut used)
    };
    check(rc);
    body.truncate(used as usize);
    let verdicts = (0..m).map(|i| {
        let mut v = Verdict { code: codes[i] as u32, digest: [0u8; 32], kind: kinds[i] };
        v.digest.copy_from_slice(&digests[32 * i..32 * i + 32]);
        let sig = if voted[i] != 0 {
            let mut s = [0u8; 64];
            s.copy_from_slice(&sigs[64 * i..64 * i + 64]);
            Some(s)
        } else {
            None
        };
        (v, sig)
    }).collect();
    (verdicts, BatchViews { views, body })
}

/// One decoded message: its view, its wire bytes and the call's body.  The iterators read the wire
/// only at the offsets the view names; entries come out in `BTreeMap` / `BTreeSet` order, so
/// `BTreeMap::from_iter(entries.payload())` inserts already-sorted entries.
pub struct ViewEntries<'a> {
    pub view: &'a MsgView,
    pub wire: &'a [u8],
    pub body: &'a [u8],
}

impl<'a> ViewEntries<'a> {
    /// `None` for a message that did not decode.
    pub fn new(view: &'a MsgView, wire: &'a [u8], body: &'a [u8]) -> Option<Self> {
        if view.decoded != 0 { Some(ViewEntries { view, wire, body }) } else { None }
    }

    fn area(&self, in_body: bool, off: u64, len: usize) -> &'a [u8] {
        let src = if in_body { self.body } else { self.wire };
        &src[off as usize..off as usize + len]
    }

    /// The header's or the vote's signature.
    pub fn signature(&self) -> &'a [u8] {
        &self.wire[self.view.sig_off as usize..self.view.sig_off as usize + 64]
    }

    /// `(digest, worker_id)` of `Header.payload`, ascending by digest.
    pub fn payload(&self) -> impl Iterator<Item = (&'a [u8], u32)> + 'a {
        let v = self.view;
        let a = self.area(v.flags & ffi::NWC_VIEW_PAYLOAD_IN_BODY != 0, v.payload_off, 36 * v.n_payload as usize);
        a.chunks_exact(36).map(|e| (&e[..32], u32::from_le_bytes([e[32], e[33], e[34], e[35]])))
    }

    /// `Header.parents`, ascending.
    pub fn parents(&self) -> impl Iterator<Item = &'a [u8]> + 'a {
        let v = self.view;
        self.area(v.flags & ffi::NWC_VIEW_PARENTS_IN_BODY != 0, v.parents_off, 32 * v.n_parents as usize).chunks_exact(32)
    }

    /// `(member_index, signature)` of a certificate's votes in wire order; an index of -1 is a voter
    /// outside the committee, whose key text lies at `vote_key_text`.
    pub fn votes(&self) -> impl Iterator<Item = (i32, &'a [u8])> + 'a {
        let wire = self.wire;
        self.area(true, self.view.votes_off, 8 * self.view.n_votes as usize).chunks_exact(8).map(move |e| {
            let idx = i32::from_le_bytes([e[0], e[1], e[2], e[3]]);
            let off = u32::from_le_bytes([e[4], e[5], e[6], e[7]]) as usize;
            let mut l = [0u8; 8];
            l.copy_from_slice(&wire[off..off + 8]);
            let sig = off + 8 + u64::from_le_bytes(l) as usize;
            (idx, &wire[sig..sig + 64])
        })
    }

    /// The base64 text of vote `k`'s key, for a voter whose index is -1.
    pub fn vote_key_text(&self, k: usize) -> &'a [u8] {
        let e = self.area(true, self.view.votes_off + 8 * k as u64, 8);
        let off = u32::from_le_bytes([e[4], e[5], e[6], e[7]]) as usize;
        let mut l = [0u8; 8];
        l.copy_from_slice(&self.wire[off..off + 8]);
        &self.wire[off + 8..off + 8 + u64::from_le_bytes(l) as usize]
    }
}
