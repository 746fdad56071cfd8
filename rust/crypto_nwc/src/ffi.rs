//! Raw declarations of every entry point of include/nwc.h (checked against the header by
//! tests/test_rust_shim.py: same names, same parameter types, same order).
#![allow(dead_code)]
use std::os::raw::{c_char, c_int, c_void};

/// Opaque handle of a batch digester (nwc_digester_create).
#[allow(non_camel_case_types)]
pub enum nwc_digester {}

/// Device bytes this process holds on one device (nwc_memory_info).
#[allow(non_camel_case_types)]
#[repr(C)]
#[derive(Default, Debug, Clone, Copy)]
pub struct nwc_memory {
    pub tables: u64,
    pub committee: u64,
    pub auto_cache: u64,
    pub scratch: u64,
    pub digesters: u64,
    pub device_free: u64,
    pub device_total: u64,
}

/// One decoded message of `nwc_sanitize_messages_view` (160 bytes; include/nwc.h).
#[allow(non_camel_case_types)]
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct nwc_msg_view {
    pub decoded: u8,
    pub kind: u8,
    pub flags: u8,
    pub reserved0: u8,
    pub code: i32,
    pub round: u64,
    pub author: [u8; 32],
    pub origin: [u8; 32],
    pub id: [u8; 32],
    pub author_index: i32,
    pub origin_index: i32,
    pub n_payload: u32,
    pub n_parents: u32,
    pub n_votes: u32,
    pub sig_off: u32,
    pub payload_off: u64,
    pub parents_off: u64,
    pub votes_off: u64,
}
pub const NWC_VIEW_PAYLOAD_IN_BODY: u8 = 1;
pub const NWC_VIEW_PARENTS_IN_BODY: u8 = 2;

#[link(name = "nwc")]
extern "C" {
    pub fn nwc_init(device_mask: u32) -> c_int;
    pub fn nwc_shutdown();
    pub fn nwc_last_error() -> *const c_char;
    pub fn nwc_last_error_code() -> c_int;
    pub fn nwc_version() -> c_int;
    pub fn nwc_device_count() -> c_int;
    pub fn nwc_build_id() -> *const c_char;
    pub fn nwc_memory_info(out: *mut nwc_memory) -> c_int;
    pub fn nwc_trim() -> c_int;
    pub fn nwc_diag_set(name: *const c_char, value: i64) -> c_int;
    pub fn nwc_diag_verify_clock(d_msgs: *const c_void, msg_stride: u64, d_pks: *const c_void, d_sigs: *const c_void,
                                 n: u64, d_verdict_words: *mut c_void, stream: *mut c_void, clock_ghz: *mut f64,
                                 waves: *mut u32) -> c_int;

    pub fn nwc_verify_strict(msg32: *const u8, pk: *const u8, sig: *const u8) -> c_int;
    pub fn nwc_verify_batch(msg32: *const u8, pks: *const u8, sigs: *const u8, n: usize, bad_bitmap: *mut u8) -> c_int;
    pub fn nwc_verify_strict_many(msgs32: *const u8, pks: *const u8, sigs: *const u8, n: usize,
                                  verdict_bitmap: *mut u8) -> c_int;
    pub fn nwc_verify_batch_many(digests: *const u8, offsets: *const u32, pks: *const u8, sigs: *const u8, m: usize,
                                 cert_ok_bitmap: *mut u8, bad_vote_bitmap: *mut u8) -> c_int;
    pub fn nwc_verify_batch_straus_many(digests: *const u8, offsets: *const u32, pks: *const u8, sigs: *const u8,
                                        m: usize, cert_ok_bitmap: *mut u8, bad_vote_bitmap: *mut u8) -> c_int;
    pub fn nwc_verify_batch_msm_many(digests: *const u8, offsets: *const u32, pks: *const u8, sigs: *const u8,
                                        m: usize, cert_ok_bitmap: *mut u8, bad_vote_bitmap: *mut u8) -> c_int;
    pub fn nwc_keypair_from_seed(seed: *const u8, secret64: *mut u8) -> c_int;
    pub fn nwc_signer_create(secret64: *const u8) -> *mut c_void;
    pub fn nwc_signer_public_key(signer: *const c_void, pk: *mut u8) -> c_int;
    pub fn nwc_signer_sign(signer: *mut c_void, msg32: *const u8, sig: *mut u8) -> c_int;
    pub fn nwc_signer_sign_many(signer: *mut c_void, msgs32: *const u8, n: usize, sigs: *mut u8) -> c_int;
    pub fn nwc_dev_sign(signer: *mut c_void, d_msgs: *const c_void, msg_stride: u64, n: u64, d_sigs: *mut c_void,
                        stream: *mut c_void) -> c_int;
    pub fn nwc_signer_vote(signer: *mut c_void, id32: *const u8, round: u64, origin32: *const u8, sig: *mut u8) -> c_int;
    pub fn nwc_signer_vote_many(signer: *mut c_void, ids32: *const u8, rounds: *const u64, origins32: *const u8, n: usize,
                                sigs: *mut u8) -> c_int;
    pub fn nwc_dev_vote(signer: *mut c_void, d_ids: *const c_void, d_rounds: *const c_void, d_origins: *const c_void, n: u64,
                        d_sigs: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn nwc_signer_destroy(signer: *mut c_void) -> c_int;
    pub fn nwc_verifier_create(max_requests: u32, max_wait_us: u32) -> *mut c_void;
    pub fn nwc_verifier_verify_strict(verifier: *mut c_void, msg32: *const u8, pk: *const u8, sig: *const u8) -> c_int;
    pub fn nwc_verifier_verify_batch(verifier: *mut c_void, msg32: *const u8, pks: *const u8, sigs: *const u8, n: usize,
                                     bad_bitmap: *mut u8) -> c_int;
    pub fn nwc_verifier_stats(verifier: *mut c_void, out: *mut u64) -> c_int;
    pub fn nwc_verifier_destroy(verifier: *mut c_void) -> c_int;
    pub fn nwc_sanitizer_create(max_messages: u32, max_wait_us: u32) -> *mut c_void;
    pub fn nwc_sanitizer_sanitize(sanitizer: *mut c_void, msg: *const u8, len: usize, gc_round: u64, vote_target: *const u8,
                                  digest32: *mut u8, kind: *mut u8) -> c_int;
    pub fn nwc_sanitizer_stats(sanitizer: *mut c_void, out: *mut u64) -> c_int;
    pub fn nwc_sanitizer_sanitize_vote(sanitizer: *mut c_void, signer: *mut c_void, msg: *const u8, len: usize, gc_round: u64,
                                       vote_target: *const u8, digest32: *mut u8, kind: *mut u8, vote_sig64: *mut u8,
                                       voted: *mut i32) -> c_int;
    pub fn nwc_sanitizer_vote_stats(sanitizer: *mut c_void, in_flight: *mut u64, alone: *mut u64) -> c_int;
    pub fn nwc_sanitizer_sanitize_view(sanitizer: *mut c_void, signer: *mut c_void, msg: *const u8, len: usize, gc_round: u64,
                                       vote_target: *const u8, digest32: *mut u8, kind: *mut u8, vote_sig64: *mut u8,
                                       voted: *mut i32, view: *mut c_void, body: *mut u8, body_cap: u64,
                                       body_used: *mut u64) -> c_int;
    pub fn nwc_sanitizer_view_stats(sanitizer: *mut c_void, in_flight: *mut u64, alone: *mut u64) -> c_int;
    pub fn nwc_sanitizer_destroy(sanitizer: *mut c_void) -> c_int;
    pub fn nwc_set_committee(pks: *const u8, n: usize) -> c_int;
    pub fn nwc_cache_stats(committee_keys: *mut u32, auto_keys: *mut u32) -> c_int;
    pub fn nwc_auto_cache_info(capacity: *mut u32, builds: *mut u64, hits: *mut u64) -> c_int;
    pub fn nwc_launch_keys_info(held: *mut u32, capacity: *mut u32) -> c_int;
    /// Diagnostics only (the table audit of tests/test_gpu_tables.py), not part of the crate's API.
    pub fn nwc_diag_table(name: *const c_char, address: *mut u64, elem_bytes: *mut u32, elements: *mut u64,
                          keys: *mut u32) -> c_int;

    pub fn nwc_set_committee_config(pks: *const u8, stakes: *const u64, n: usize, worker_offsets: *const u32,
                                    worker_ids: *const u32) -> c_int;
    pub fn nwc_sanitize_messages(data: *const u8, offsets: *const u64, m: usize, gc_round: u64, vote_target: *const u8,
                                 codes: *mut i32, digests32: *mut u8, kinds: *mut u8) -> c_int;
    pub fn nwc_dev_sanitize_messages(d_data: *const c_void, d_offsets: *const c_void, m: u64, total: u64, gc_round: u64,
                                     vote_target: *const u8, d_codes: *mut c_void, d_digests32: *mut c_void,
                                     stream: *mut c_void) -> c_int;
    pub fn nwc_sanitize_messages_ex(data: *const u8, offsets: *const u64, m: usize, gc_rounds: *const u64, gc_round: u64,
                                    vote_targets80: *const u8, vote_target: *const u8, signer: *mut c_void,
                                    codes: *mut i32, digests32: *mut u8, kinds: *mut u8, vote_sigs: *mut u8,
                                    voted: *mut u8) -> c_int;
    pub fn nwc_dev_sanitize_messages_ex(d_data: *const c_void, d_offsets: *const c_void, m: u64, total: u64,
                                        d_gc_rounds: *const c_void, gc_round: u64, d_vote_targets80: *const c_void,
                                        vote_target: *const u8, signer: *mut c_void, d_codes: *mut c_void,
                                        d_digests32: *mut c_void, d_kinds: *mut c_void, d_vote_sigs: *mut c_void,
                                        d_voted: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn nwc_msg_view_body_bound(total: u64, m: u64) -> u64;
    /// `views`: m `nwc_msg_view` records (or null: `nwc_sanitize_messages_ex`).
    pub fn nwc_sanitize_messages_view(data: *const u8, offsets: *const u64, m: usize, gc_rounds: *const u64, gc_round: u64,
                                      vote_targets80: *const u8, vote_target: *const u8, signer: *mut c_void,
                                      codes: *mut i32, digests32: *mut u8, kinds: *mut u8, vote_sigs: *mut u8,
                                      voted: *mut u8, views: *mut c_void, body: *mut u8, body_cap: usize,
                                      body_used: *mut u64) -> c_int;
    pub fn nwc_dev_sanitize_messages_view(d_data: *const c_void, d_offsets: *const c_void, m: u64, total: u64,
                                          d_gc_rounds: *const c_void, gc_round: u64, d_vote_targets80: *const c_void,
                                          vote_target: *const u8, signer: *mut c_void, d_codes: *mut c_void,
                                          d_digests32: *mut c_void, d_kinds: *mut c_void, d_vote_sigs: *mut c_void,
                                          d_voted: *mut c_void, d_views: *mut c_void, d_body: *mut c_void, body_cap: u64,
                                          d_body_used: *mut c_void, stream: *mut c_void) -> c_int;

    pub fn nwc_digest32(data: *const u8, len: usize, out32: *mut u8) -> c_int;
    pub fn nwc_sha512_trunc32_many(data: *const u8, offsets: *const u64, n: usize, out32: *mut u8) -> c_int;
    pub fn nwc_digester_create(max_group: u32, max_wait_us: u32) -> *mut nwc_digester;
    pub fn nwc_digester_submit(q: *mut nwc_digester, batch: *const u8, len: usize, tag: u64) -> c_int;
    pub fn nwc_digester_poll(q: *mut nwc_digester, max: usize, wait_us: u32, tags: *mut u64, digests32: *mut u8,
                             n_done: *mut usize) -> c_int;
    pub fn nwc_digester_stats(q: *mut nwc_digester, groups: *mut u64, batches: *mut u64, bytes: *mut u64) -> c_int;
    pub fn nwc_digester_destroy(q: *mut nwc_digester) -> c_int;
    pub fn nwc_digester_arena(q: *mut nwc_digester, bytes: usize) -> *mut u8;
    pub fn nwc_digester_direct_groups(q: *mut nwc_digester, direct_groups: *mut u64) -> c_int;

    pub fn nwc_dev_verify(d_msgs: *const c_void, d_msg_index: *const c_void, msg_stride: u64, d_pks: *const c_void,
                          d_sigs: *const c_void, n: u64, strict: c_int, d_verdict_words: *mut c_void,
                          stream: *mut c_void) -> c_int;
    pub fn nwc_dev_cert_reduce(d_leaf_words: *const c_void, d_offsets: *const c_void, m: u64, nvotes: u64,
                               d_cert_words: *mut c_void, d_bad_words: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn nwc_dev_verify_batch_straus(d_digests: *const c_void, d_offsets: *const c_void, d_msg_index: *const c_void,
                                       m: u64, nvotes: u64, d_pks: *const c_void, d_sigs: *const c_void,
                                       d_leaf_words: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn nwc_dev_verify_batch_msm(d_digests: *const c_void, d_offsets: *const c_void, d_msg_index: *const c_void,
                                       m: u64, nvotes: u64, d_pks: *const c_void, d_sigs: *const c_void,
                                       d_leaf_words: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn nwc_msm_stats(groups_passed: *mut u64, groups_failed: *mut u64, key_overflows: *mut u64,
                         groups_skipped: *mut u64) -> c_int;
    pub fn nwc_dev_sha512_trunc32(d_data: *const c_void, d_offsets: *const c_void, n: u64, d_out32: *mut c_void,
                                  stream: *mut c_void) -> c_int;
    pub fn nwc_dev_sha512_trunc32_ranges(d_data: *const c_void, d_starts: *const c_void, d_ends: *const c_void, n: u64,
                                         d_out32: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn nwc_dev_derive32(tag: *const u8, taglen: c_int, first: u64, n: u64, d_out: *mut c_void,
                            stream: *mut c_void) -> c_int;
    pub fn nwc_dev_keygen_sign(d_seeds: *const c_void, d_msgs: *const c_void, n: u64, d_pks: *mut c_void,
                               d_sigs: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn nwc_dev_set_device(device: c_int) -> c_int;

    pub fn nwc_shard_bounds(n: u64, world: u32, rank: u32, lo: *mut u64, hi: *mut u64) -> c_int;
    pub fn nwc_cert_cuts(offsets: *const u32, m: usize, world: u32, cuts: *mut u64) -> c_int;
}
