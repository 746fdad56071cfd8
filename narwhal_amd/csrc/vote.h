// Vote::new on the device (primary/src/messages.rs:115-129): the signature of
// Vote::digest = SHA-512(id || round LE || origin)[..32] under a signer's registered key.
//
//   k_vote        throughput: one vote per lane, table in LDS (as k_sign)
//   k_vote_wide   latency: one wave per vote (as k_sign_wide)
//   k_vote_group  the sanitizer's group flight: one wave per message of the group, after
//                 k_finalize_group; signs for the headers whose code is Ok and whose caller asked
//   k_vote_msgs   the batch entries (nwc_sanitize_messages_ex with a signer): one wave per message
//                 of the call, after k_finalize_messages; signs for the headers whose code is Ok
//   k_vote_wire   one wire header the host has already accepted (the queue's fallback)
//
// Every kernel is vote_digest (digest72 of messages.h, one SHA-512 block) followed by the signing
// body of sign.h (sign_lane / sign_wave: nonce, fixed-base multiplication, response, store), and
// sign.h's secret-independence rules hold here unchanged: nothing branches on, bounds a loop by or
// forms an address from a, prefix, r, their digits or s; kernel arguments and the group buffer
// carry the address of a key record, never key bytes.  What the kernels do branch on is public:
// the message's kind and code, the "asked for a vote" key slot, lengths read from the wire.
#pragma once
#include "messages.h"
#include "sign.h"

namespace nwc {

// Vote::digest (primary/src/messages.rs:145-153)
FE_DEV void vote_digest(const u32 id[8], uint64_t round, const u32 origin[8], u32 m[8]) { digest72(id, round, origin, m); }

// Lane i: ids + 32 i, rounds[i], origins + 32 i (ids and origins 16-byte aligned) -> sigs + 64 i.
__global__ __launch_bounds__(256) void k_vote(const SignKey* __restrict__ key, const ge_niels* __restrict__ table,
                                              const uint8_t* __restrict__ ids, const uint64_t* __restrict__ rounds,
                                              const uint8_t* __restrict__ origins, uint64_t n, uint8_t* __restrict__ sigs,
                                              uint8_t* __restrict__ flags) {
  __shared__ ge_niels sT[SIGN_TABLE_ENTRIES];
  sign_table_to_lds(table, sT);
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 id[8], origin[8], m[8];
  load_words8(ids + 32 * i, id);
  load_words8(origins + 32 * i, origin);
  vote_digest(id, rounds[i], origin, m);
  sign_lane(key, sT, m, sigs, flags, i);
}

// Block (one wave) i signs vote i.
__global__ __launch_bounds__(64) void k_vote_wide(const SignKey* __restrict__ key, const ge_niels* __restrict__ table,
                                                  const uint8_t* __restrict__ ids, const uint64_t* __restrict__ rounds,
                                                  const uint8_t* __restrict__ origins, uint64_t n,
                                                  uint8_t* __restrict__ sigs, uint8_t* __restrict__ flags) {
  const uint64_t i = blockIdx.x;
  if (i >= n) return;   // block-uniform
  const int lane = threadIdx.x & 63;
  u32 id[8], origin[8], m[8];
  load_words8(ids + 32 * i, id);
  load_words8(origins + 32 * i, origin);
  vote_digest(id, rounds[i], origin, m);
  sign_wave(key, table, m, lane, sigs, flags, i);
}

// The group's vote requests, in the pinned group buffer: per message the device address of the
// signer's key record (0 = no vote asked), 64 bytes for the signature and the "written" byte.
struct GroupVotes {
  const uint64_t* keys;
  uint8_t* sigs;
  uint8_t* flags;
};
// After k_finalize_group on the group's stream.  Block i leaves at once (block-uniformly) unless
// slot i carries a key, its result word is written without "decide me again", its code is Ok and
// it is a header.  The header's id is the digest the group published for it (equal to the id on
// the wire, since the code is Ok), its origin the parsed author (the first 32 decoded bytes,
// whatever the length of the key's text) and its round the u64 behind the author string.
__global__ __launch_bounds__(64) void k_vote_group(const ge_niels* __restrict__ table, GroupVotes v,
                                                   const uint32_t* results, const uint32_t* __restrict__ rec,
                                                   const uint8_t* __restrict__ digests, const uint8_t* __restrict__ eq_pk,
                                                   const uint8_t* __restrict__ data, const uint64_t* __restrict__ starts,
                                                   const uint32_t* __restrict__ lens, uint32_t nmsg) {
  const uint32_t i = blockIdx.x;
  if (i >= nmsg) return;   // block-uniform, as every exit below
  // the key, then the word: the host clears a slot's word before it writes a new key there, so a
  // block of an earlier group's launch that is still running never pairs a new key with an old word
  const uint64_t kaddr = __hip_atomic_load(v.keys + i, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
  if (!kaddr) return;
  const u32 w = __hip_atomic_load(results + i, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
  if (!(w & GROUP_WRITTEN) || (w & GROUP_REDO) || (w & 255u) != DAG_OK) return;
  if ((rec[4 * i] & 255u) != MSG_HEADER) return;
  const uint64_t beg = starts[i], len = lens[i];
  const uint64_t L = ld_u64(data, beg + 4);
  if (L > len || 20 + L > len) return;   // (a header that parsed holds its round; never read past the message)
  const uint64_t round = ld_u64(data, beg + 12 + L);
  u32 id[8], origin[8], m[8];
  load_words8(digests + 32 * (size_t)i, id);
  load_words8(eq_pk + 32 * (size_t)i, origin);
  vote_digest(id, round, origin, m);
  sign_wave(reinterpret_cast<const SignKey*>(kaddr), table, m, (int)(threadIdx.x & 63), v.sigs, v.flags, i);
}

// The batch entries' votes (nwc_sanitize_messages_ex with a signer): after k_finalize_messages on
// the call's stream, block (one wave) i for message i of the call.  Every block writes its slot:
// voted[i] = 1 and the signature for a header whose final code is Ok, zeros otherwise -- the
// outputs need no memset, and nothing is signed before codes[i] says Ok.  The header's id is the
// digest the pipeline published (equal to the id on the wire, since the code is Ok), its origin
// the parsed author at eq_pk + 32 i and its round the u64 behind the author string, read only
// when it lies inside the message.  Every exit is block-uniform: codes, rec and the wire lengths
// are the same in every lane.  sigs is 4-byte aligned.
__global__ __launch_bounds__(64) void k_vote_msgs(const SignKey* __restrict__ key, const ge_niels* __restrict__ table,
                                                  const int32_t* __restrict__ codes, const uint32_t* __restrict__ rec,
                                                  const uint8_t* __restrict__ digests, const uint8_t* __restrict__ eq_pk,
                                                  const uint8_t* __restrict__ data, const uint64_t* __restrict__ offsets,
                                                  uint64_t m, uint8_t* __restrict__ sigs, uint8_t* __restrict__ voted) {
  const uint64_t i = blockIdx.x;
  if (i >= m) return;   // block-uniform, as every exit below
  const int lane = (int)(threadIdx.x & 63);
  bool vote = codes[i] == (int32_t)DAG_OK && (rec[4 * i] & 255u) == MSG_HEADER;
  uint64_t beg = 0, L = 0;
  if (vote) {
    beg = offsets[i];
    const uint64_t len = offsets[i + 1] - beg;
    L = len >= 12 ? ld_u64(data, beg + 4) : ~0ull;
    vote = L <= len && 20 + L <= len;   // (a header that parsed holds its round; never read past the message)
  }
  if (!vote) {
    if (lane < 16) reinterpret_cast<uint32_t*>(sigs + 64 * i)[lane] = 0u;
    if (lane == 0) voted[i] = 0;
    return;
  }
  const uint64_t round = ld_u64(data, beg + 12 + L);
  u32 id[8], origin[8], dg[8];
  load_words8(digests + 32 * i, id);
  load_words8(eq_pk + 32 * i, origin);
  vote_digest(id, round, origin, dg);
  sign_wave(key, table, dg, lane, sigs, nullptr, i);
  if (lane == 0) voted[i] = 1;
}

// One wire message the host has sanitized to Ok + header (its id is `id32`): msg is 16-byte
// aligned with >= 16 readable bytes behind its len bytes.  The author is decoded as the parse
// does (MsgReader::key); a message that is no header or does not decode leaves the flag unwritten.
__global__ __launch_bounds__(64) void k_vote_wire(const SignKey* __restrict__ key, const ge_niels* __restrict__ table,
                                                  const uint8_t* __restrict__ msg, uint64_t len,
                                                  const uint8_t* __restrict__ id32, uint8_t* __restrict__ sig,
                                                  uint8_t* __restrict__ flag) {
  if (len < 4 || ld_u32(msg, 0) != MSG_HEADER) return;   // block-uniform
  MsgReader r{msg, 4, len, true, false};
  u32 origin[8];
  r.key(origin);
  const uint64_t round = r.u64();
  if (!r.ok) return;   // block-uniform: every lane reads the same bytes
  u32 id[8], m[8];
  load_words8(id32, id);
  vote_digest(id, round, origin, m);
  sign_wave(key, table, m, (int)(threadIdx.x & 63), sig, flag, 0);
}

}  // namespace nwc
