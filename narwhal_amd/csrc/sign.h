// Signing with a registered key (RFC 8032 / dalek Keypair::sign over a 32-byte Digest):
// crypto::Signature::new and SignatureService (crypto/src/lib.rs:177-191, 222-250).
//
//   k_build_sign_table  the signer's basepoint table, built on the device (no embedded constants)
//   k_sign_expand       SecretKey -> key record (a mod l, prefix, A), once per signer
//   k_sign              throughput: one signature per lane, table in LDS (body: sign_lane)
//   k_sign_wide         latency: one wave per signature, one window per lane (body: sign_wave)
// The vote kernels of vote.h run the same two bodies on Vote::digest.
//
// Table: signed radix-16, doubling-free.  SIGN_TABLE[8 w + (j - 1)] = j * 16^w * B for the 64
// windows w and j = 1..8, affine Niels (120 B): 64 x 8 x 120 B = 61,440 B.  A scalar < 2^253 recodes
// (sc_recode_radix16) into 64 digits in [-8, 7], so a fixed-base multiplication is 64 mixed
// additions and no doubling.  dalek's 32 x 8 layout (30 KB, 4 doublings) would halve the LDS, but
// k_sign's residency is bounded by its registers, not by LDS (two blocks of 256 lanes fit a CU's
// 160 KiB either way), so the doublings would be pure extra work ("Signing").
//
// Secret independence (a review criterion; DESIGN.md "Signing"): nothing below branches on, bounds a
// loop by, or forms an address from a, prefix, r, their digits, k*a or s.
//   - A window's entry is taken by reading all 8 candidates of that window -- addresses depend on
//     the window number (a loop counter in k_sign, the lane number in k_sign_wide) only -- and
//     AND-ing each with an all-ones / all-zeros mask derived from |digit| == j; digit 0 leaves the
//     Niels identity.  In k_sign every lane reads the same LDS addresses (broadcast reads).
//   - The digit's sign swaps y+x / y-x and negates 2dxy through masks (sign_select).
//   - Digits are consumed by shifting the packed digit string (k_sign) or by a select over its
//     eight words with the lane number (k_sign_wide), never by indexing with a digit.
//   - s = r + k a mod l is a fixed-trip schoolbook product, an add with carries and sc_reduce512,
//     whose conditional subtractions are selects.
//   - Kernel arguments carry a pointer to the key record, never key bytes.
// The additions themselves are ge25519.h's complete formulas (no special cases for the identity).
#pragma once
#include "fe_sliced.h"
#include "ge25519.h"
#include "sc25519.h"

namespace nwc {

constexpr int SIGN_WINDOWS = 64;
constexpr int SIGN_TABLE_ENTRIES = SIGN_WINDOWS * 8;
constexpr size_t SIGN_TABLE_BYTES = SIGN_TABLE_ENTRIES * sizeof(ge_niels);
static_assert(SIGN_TABLE_BYTES == 61440, "signer basepoint table");

// The expanded key of one signer, in device memory owned by its handle: a = clamp(h[..32]) mod l,
// prefix = h[32..], A = aB compressed (h = SHA-512(seed)).
struct SignKey { u32 a[8]; u32 prefix[8]; u32 A[8]; };
static_assert(sizeof(SignKey) == 96, "key record");

// One lane per entry: 16^w B by 4 w doublings, times j by a 4-bit double-and-add, one inversion.
__global__ void k_build_sign_table(ge_niels* table) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= SIGN_TABLE_ENTRIES) return;
  const int w = i >> 3, j = (i & 7) + 1;
  ge_p3 b = ge_base_point();
#pragma unroll 1
  for (int k = 0; k < 4 * w; ++k) b = ge_p1p1_to_p3(ge_p2_dbl(ge_p3_to_p2(b)));
  const ge_cached bc = ge_p3_to_cached(b);
  ge_p3 acc = ge_p3_identity();
#pragma unroll 1
  for (int bit = 3; bit >= 0; --bit) {
    acc = ge_p1p1_to_p3(ge_p2_dbl(ge_p3_to_p2(acc)));
    const ge_p3 sum = ge_p1p1_to_p3(ge_add_cached(acc, bc));
    const bool take = (j >> bit) & 1;   // j is the entry number: public
    _Pragma("unroll") for (int q = 0; q < 40; ++q)
      reinterpret_cast<i32*>(&acc)[q] = take ? reinterpret_cast<const i32*>(&sum)[q] : reinterpret_cast<const i32*>(&acc)[q];
  }
  table[i] = ge_p3_to_niels(acc);
}

// all-ones if x == y, else 0 (no compare-and-branch: a subtraction's borrow)
FE_DEV u32 sign_eq_mask(u32 x, u32 y) {
  const u32 d = x ^ y;
  return (u32)(((u64)d - 1) >> 32);   // d == 0 -> 0xFFFFFFFF
}

// Entry |d| of window w (|d| in 0..8; 0 = the Niels identity) out of its 8 candidates, all of
// which are read; then the sign.  nib = d + 8 in 0..15.  `win` points at the window's 8 entries.
FE_DEV ge_niels sign_select(const ge_niels* win, u32 nib) {
  const i32 d = (i32)nib - 8;
  const u32 neg = (u32)(d >> 31);               // all-ones if d < 0
  const u32 absd = ((u32)d ^ neg) - neg;
  ge_niels e = ge_niels_identity();
  u32* ev = reinterpret_cast<u32*>(&e);
  _Pragma("unroll") for (u32 j = 0; j < 8; ++j) {
    const u32 m = sign_eq_mask(absd, j + 1);
    const u32* cv = reinterpret_cast<const u32*>(win + j);
    _Pragma("unroll") for (int q = 0; q < 30; ++q) ev[q] = (ev[q] & ~m) | (cv[q] & m);
  }
  // -(x, y) = (-x, y): swap y+x <-> y-x, negate 2dxy
  ge_niels r;
  _Pragma("unroll") for (int q = 0; q < 10; ++q) {
    const u32 p = (u32)e.ypx.v[q], mi = (u32)e.ymx.v[q], t = (u32)e.xy2d.v[q];
    const u32 x = (p ^ mi) & neg;
    r.ypx.v[q] = (i32)(p ^ x);
    r.ymx.v[q] = (i32)(mi ^ x);
    r.xy2d.v[q] = (i32)((t ^ neg) - neg);
  }
  return r;
}

// sc * B for a reduced scalar, 64 mixed additions; T = the table (LDS in k_sign, HBM in the key
// expansion).  The loop runs over the window number; the digit string is shifted, not indexed.
FE_DEV ge_p3 sign_base_mult(const u32 sc[8], const ge_niels* T) {
  u32 dg[8];
  sc_recode_radix16(sc, dg);
  ge_p3 acc = ge_p3_identity();
#pragma unroll 1
  for (int w = 0; w < SIGN_WINDOWS; ++w) {
    const u32 nib = dg[0] & 15u;
    _Pragma("unroll") for (int q = 0; q < 7; ++q) dg[q] = (dg[q] >> 4) | (dg[q + 1] << 28);
    dg[7] >>= 4;
    acc = ge_p1p1_to_p3(ge_add_niels(acc, sign_select(T + 8 * w, nib)));
  }
  return acc;
}

// r = SHA-512(prefix || M) mod l
FE_DEV void sign_nonce(const SignKey* key, const u32 m[8], u32 r[8]) {
  u32 buf[28];
  _Pragma("unroll") for (int j = 0; j < 28; ++j) buf[j] = 0;
  _Pragma("unroll") for (int j = 0; j < 8; ++j) { buf[j] = key->prefix[j]; buf[8 + j] = m[j]; }
  u32 h[16];
  sha512_one_block(buf, 64, h);
  sc_reduce512(h, r);
}

// s = r + SHA-512(R || A || M) a mod l
FE_DEV void sign_response(const SignKey* key, const u32 R[8], const u32 m[8], const u32 r[8], u32 s[8]) {
  u32 buf[28];
  _Pragma("unroll") for (int j = 0; j < 28; ++j) buf[j] = 0;
  _Pragma("unroll") for (int j = 0; j < 8; ++j) { buf[j] = R[j]; buf[8 + j] = key->A[j]; buf[16 + j] = m[j]; }
  u32 kh[16];
  sha512_one_block(buf, 96, kh);
  u32 k[8];
  sc_reduce512(kh, k);
  u32 a[8];
  _Pragma("unroll") for (int j = 0; j < 8; ++j) a[j] = key->a[j];
  u32 prod[16];
  _Pragma("unroll") for (int j = 0; j < 16; ++j) prod[j] = 0;
  _Pragma("unroll") for (int x = 0; x < 8; ++x) {
    u64 carry = 0;
    _Pragma("unroll") for (int y = 0; y < 8; ++y) {
      const u64 t = (u64)k[x] * a[y] + prod[x + y] + carry;
      prod[x + y] = (u32)t;
      carry = t >> 32;
    }
    prod[x + 8] = (u32)carry;
  }
  u64 carry = 0;
  _Pragma("unroll") for (int j = 0; j < 16; ++j) {
    const u64 t = (u64)prod[j] + (j < 8 ? r[j] : 0u) + carry;
    prod[j] = (u32)t;
    carry = t >> 32;
  }
  sc_reduce512(prod, s);
}

// One signature's 16 words; with `flag` (a zero-copy host call: sig and flag are pinned host
// memory) the words go out as system-scope stores, then a fence, then the "written" byte the
// host polls.
FE_DEV void sign_store(uint8_t* sig, const u32 R[8], const u32 s[8], uint8_t* flag) {
  uint32_t* so = reinterpret_cast<uint32_t*>(sig);
  if (flag) {
    _Pragma("unroll") for (int j = 0; j < 8; ++j) {
      __hip_atomic_store(so + j, R[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(so + 8 + j, s[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __threadfence_system();
    __hip_atomic_store(flag, (uint8_t)0x80u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  } else {
    _Pragma("unroll") for (int j = 0; j < 8; ++j) { so[j] = R[j]; so[8 + j] = s[j]; }
  }
}

// Key expansion (nwc_signer_create, nwc_keypair_from_seed): in = seed (32 B) || claimed public half
// (32 B, read only if check != 0); out_pk = the derived A; *status = 1 (ok) or 2 (check != 0 and the
// claimed half differs from A -- a public fact).  The record is written only for status 1.  One
// wave, every lane computes the same values, lane 0 stores.
__global__ __launch_bounds__(64) void k_sign_expand(const uint8_t* __restrict__ in, int check,
                                                    const ge_niels* __restrict__ table, SignKey* __restrict__ key,
                                                    uint8_t* __restrict__ out_pk, uint32_t* __restrict__ status) {
  u32 seed[8], pub[8];
  load_words8(in, seed);
  load_words8(in + 32, pub);
  u32 sbuf[28];
  _Pragma("unroll") for (int j = 0; j < 28; ++j) sbuf[j] = j < 8 ? seed[j] : 0u;
  u32 h[16];
  sha512_one_block(sbuf, 32, h);
  u32 wide[16];
  _Pragma("unroll") for (int j = 0; j < 16; ++j) wide[j] = j < 8 ? h[j] : 0u;
  wide[0] &= 0xFFFFFFF8u; wide[7] &= 0x7FFFFFFFu; wide[7] |= 0x40000000u;
  u32 a[8];
  sc_reduce512(wide, a);   // aB = (a mod l) B: B has order l
  u32 A[8];
  ge_p3_compress(sign_base_mult(a, table), A);
  u32 diff = 0;
  _Pragma("unroll") for (int j = 0; j < 8; ++j) diff |= A[j] ^ pub[j];
  const bool ok = !check || diff == 0;   // A and the claimed half are public
  if (threadIdx.x == 0) {
    uint32_t* po = reinterpret_cast<uint32_t*>(out_pk);
    _Pragma("unroll") for (int j = 0; j < 8; ++j) po[j] = A[j];
    if (key && ok) {
      _Pragma("unroll") for (int j = 0; j < 8; ++j) { key->a[j] = a[j]; key->prefix[j] = h[8 + j]; key->A[j] = A[j]; }
    }
    *status = ok ? 1u : 2u;
  }
}

// One lane's signature of the digest m: nonce, fixed-base multiplication over the table T (LDS in
// k_sign and k_vote), response, store to sigs + 64 i (and flags + i, when there are flags).  The
// body of k_sign; k_vote (vote.h) runs it on Vote::digest.
FE_DEV void sign_lane(const SignKey* key, const ge_niels* T, const u32 m[8], uint8_t* sigs, uint8_t* flags, uint64_t i) {
  u32 r[8];
  sign_nonce(key, m, r);
  u32 R[8];
  ge_p3_compress(sign_base_mult(r, T), R);
  u32 s[8];
  sign_response(key, R, m, r, s);
  sign_store(sigs + 64 * i, R, s, flags ? flags + i : nullptr);
}

// Copies the table into the block's LDS (all of the block's threads call it).
FE_DEV void sign_table_to_lds(const ge_niels* table, ge_niels* sT) {
  for (int i = threadIdx.x; i < SIGN_TABLE_ENTRIES * 30; i += blockDim.x)
    reinterpret_cast<i32*>(sT)[i] = reinterpret_cast<const i32*>(table)[i];
  __syncthreads();
}

// Throughput kernel: lane i signs digest i (msgs + stride * i, stride 32 or 0).
__global__ __launch_bounds__(256) void k_sign(const SignKey* __restrict__ key, const ge_niels* __restrict__ table,
                                              const uint8_t* __restrict__ msgs, uint64_t stride, uint64_t n,
                                              uint8_t* __restrict__ sigs, uint8_t* __restrict__ flags) {
  __shared__ ge_niels sT[SIGN_TABLE_ENTRIES];
  sign_table_to_lds(table, sT);
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 m[8];
  load_words8(msgs + stride * i, m);
  sign_lane(key, sT, m, sigs, flags, i);
}

// One wave's signature of the digest m (every lane holds the same m).  Every lane derives r; lane
// w takes window w's entry (all 8 candidates read, masked); the 64 points are summed by a 6-level
// butterfly, after which every lane holds R; the inversion of Z runs limb-sliced (fe_sliced.h,
// every row the same element), as k_verify_comb_wide's decompression does.  Lane 0 stores to
// sigs + 64 i (and flags + i, when there are flags).  The body of k_sign_wide; the vote kernels
// (vote.h) run it on Vote::digest.
FE_DEV void sign_wave(const SignKey* key, const ge_niels* table, const u32 m[8], const int lane, uint8_t* sigs,
                      uint8_t* flags, uint64_t i) {
  u32 r[8];
  sign_nonce(key, m, r);
  u32 dg[8];
  sc_recode_radix16(r, dg);
  // digit `lane`: a select over the eight words by the lane number
  u32 word = dg[0];
  _Pragma("unroll") for (int q = 1; q < 8; ++q) word = (q == (lane >> 3)) ? dg[q] : word;
  const u32 nib = (word >> (4 * (lane & 7))) & 15u;
  const ge_niels e = sign_select(table + 8 * lane, nib);
  ge_p3 sum = ge_p1p1_to_p3(ge_niels_to_p1p1(e));
#pragma unroll 1
  for (int mk = 1; mk < 64; mk <<= 1) {
    const ge_p3 o = shfl_xor_p3(sum, mk);
    sum = ge_p1p1_to_p3(ge_add_cached(sum, ge_p3_to_cached(o)));
  }
  // 1 / Z = Z^(p - 2), limb-sliced
  const fes z = fes_from_fe(sum.Z);
  const fes zi = fes_mul(fes_sqn(fes_pow22523(z), 3), fes_mul(fes_sq(z), z));
  const fe x = fe_from_fes(fes_mul(fes_from_fe(sum.X), zi));
  const fe y = fe_from_fes(fes_mul(fes_from_fe(sum.Y), zi));
  u32 R[8];
  fe_to_words(y, R);
  R[7] |= (u32)fe_is_negative(x) << 31;
  u32 s[8];
  sign_response(key, R, m, r, s);
  if (lane == 0) sign_store(sigs + 64 * i, R, s, flags ? flags + i : nullptr);
}

// Latency kernel: block (one wave) i signs digest i.
__global__ __launch_bounds__(64) void k_sign_wide(const SignKey* __restrict__ key, const ge_niels* __restrict__ table,
                                                  const uint8_t* __restrict__ msgs, uint64_t stride, uint64_t n,
                                                  uint8_t* __restrict__ sigs, uint8_t* __restrict__ flags) {
  const uint64_t i = blockIdx.x;
  if (i >= n) return;   // block-uniform
  const int lane = threadIdx.x & 63;
  u32 m[8];
  load_words8(msgs + stride * i, m);
  sign_wave(key, table, m, lane, sigs, flags, i);
}

}  // namespace nwc
