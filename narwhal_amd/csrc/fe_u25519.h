// GF(2^255 - 19) on NON-NEGATIVE limbs for gfx950 (MI355X), one field element per lane: the field
// of the half-size verify path (kernels.hip: verify_half's uncached branch).
//
// Representation: ten u32 limbs, radix 2^25.5 as in fe25519.h (limb i has weight 2^ceil(25.5 i)),
// every limb >= 0.  With unsigned limbs a column of the product can start from the previous
// column's carry (v_mad_u64_u32's addend), so the separate carry pass of fe25519.h -- twelve
// 64-bit shift / mask / 64-bit add steps and ten bias subtractions per product -- shrinks to a
// shift and a mask per column inside the product (feu_asm.h, tools/gen_fe_asm.py; the layout was
// chosen by tools/microbench/mad_chain.hip).  The price is a +2p / +3p / +4p bias in every
// subtraction.
//
// Bound contract.  Classes are per-limb maxima, written as multiples of
//   T ("tight"): f_i <= 2^26 - 1 + 2^11 (even i) / 2^25 - 1 + 2^11 (odd i), limb 1 <= 2^25 - 1 + 2^18.
//   feu_mul / feu_sq / feu_sq2 output (exact masks but for limb 1, which keeps limb 0's last
//   carry), feu_weak output (masks + at most 19 * 2^6), unpacked table entries and decoded bytes
//   are tight.  k T means every limb <= k times its tight maximum.
//   feu_mul(f, g):  19 g_i < 2^32 needs g <= 3.3 T (the RIGHT operand); 2 f_i < 2^32 lets the LEFT
//                   operand reach 9.5 T; every 64-bit column holds while left x right <= 31 T^2.
//   feu_sq(f), feu_sq2(f):  38 f_i < 2^32 needs f <= 3.3 T.
//   feu_add(a, b) = a + b;  feu_weak(f) takes any f <= 64 T;  feu_sub<K>(a, b) = a + K p - b needs b <= K p limb by limb:
//                   K = 2 for b <= T, K = 3 for b <= 2 T, K = 4 for b <= 3 T; the result is class(a) + K.
// Every call site of the verify path names the class of each operand; tests/cpp/feu_host.cpp
// evaluates each (left, right) pair at its maxima in 128-bit arithmetic.
//
// A tight feu is a valid loose fe (fe25519.h), so feu_as_fe is a reinterpretation and
// fe_to_words / fe_is_zero work on it unchanged (they accept up to 8 T).  feu_from_fe<K> adds K p.
//
// The header also compiles for the host (plain u64 arithmetic in place of the asm).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FEU_FN __host__ __device__ __forceinline__
#else
#define FEU_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define FEU_USE_ASM 1
#else
#define FEU_USE_ASM 0
#endif

namespace nwc {

typedef uint32_t u32;
typedef uint64_t u64;

struct feu { u32 v[10]; };

constexpr u32 FEU_M26 = (1u << 26) - 1u, FEU_M25 = (1u << 25) - 1u;
// limb i of p
FEU_FN constexpr u32 feu_p_limb(int i) { return i == 0 ? FEU_M26 - 18u : ((i & 1) ? FEU_M25 : FEU_M26); }

FEU_FN feu feu_zero() { feu r; for (int i = 0; i < 10; ++i) r.v[i] = 0; return r; }
FEU_FN feu feu_one() { feu r = feu_zero(); r.v[0] = 1; return r; }

FEU_FN feu feu_add(const feu& a, const feu& b) {
  feu r;
#pragma unroll
  for (int i = 0; i < 10; ++i) r.v[i] = a.v[i] + b.v[i];
  return r;
}
// a + K p - b, for b <= K p limb by limb
template <int K>
FEU_FN feu feu_sub(const feu& a, const feu& b) {
  feu r;
#pragma unroll
  for (int i = 0; i < 10; ++i) r.v[i] = a.v[i] + (u32)K * feu_p_limb(i) - b.v[i];
  return r;
}
// K p - a, for a <= K p limb by limb (class K)
template <int K>
FEU_FN feu feu_neg(const feu& a) {
  feu r;
#pragma unroll
  for (int i = 0; i < 10; ++i) r.v[i] = (u32)K * feu_p_limb(i) - a.v[i];
  return r;
}
// r = c ? b : a
FEU_FN feu feu_select(const feu& a, const feu& b, bool c) {
  feu r;
#pragma unroll
  for (int i = 0; i < 10; ++i) r.v[i] = c ? b.v[i] : a.v[i];
  return r;
}
// One parallel 32-bit carry step: limb i keeps its low bits and takes what limb i - 1 carried
// (limb 0: 19 x limb 9's).  Any class up to 64 T in, tight out (each mask + at most 19 * 2^6).
FEU_FN feu feu_weak(const feu& f) {
  feu r;
  r.v[0] = (f.v[0] & FEU_M26) + 19u * (f.v[9] >> 25);
#pragma unroll
  for (int i = 1; i < 10; ++i)
    r.v[i] = (f.v[i] & ((i & 1) ? FEU_M25 : FEU_M26)) + (f.v[i - 1] >> ((i & 1) ? 26 : 25));
  return r;
}

// The products.  FEU_OP / FEU_PREP: a prepared operand (k x a limb, must stay below 2^32);
// FEU_ACC / FEU_MA: a column accumulator (must stay below 2^64) and a multiply-add into it;
// FEU_COL_END: hook after the last multiply-add of a column.  A bound shadow redefines them.
#define FEU_OP u32
#define FEU_PREP(k, x) ((u32)((k) * (x)))
#define FEU_ACC u64
#define FEU_MA(h, a, b) h += (u64)(a) * (b)
#define FEU_COL_END(h)
#include "feu_asm.h"
#undef FEU_OP
#undef FEU_PREP
#undef FEU_ACC
#undef FEU_MA
#undef FEU_COL_END

// Low 255 bits of a little-endian 256-bit value (bit 255 ignored, values >= p accepted): tight.
FEU_FN feu feu_from_words(const u32 w[8]) {
  feu r;
  const int off[10] = {0, 26, 51, 77, 102, 128, 153, 179, 204, 230};
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int wi = off[i] >> 5, sh = off[i] & 31;
    const u64 v = ((u64)w[wi] | ((u64)(wi + 1 < 8 ? w[wi + 1] : 0u) << 32)) >> sh;
    r.v[i] = (u32)v & ((i & 1) ? FEU_M25 : FEU_M26);
  }
  return r;
}

// Conversions with the signed limbs of fe25519.h: s + K p.  A tight signed element (|s_i| <= 1.01 *
// 2^25 / 2^24) + p has limbs in (0.49, 1.51) x 2^26 / 2^25; a sum or difference of two of them
// (an affine Niels y + x, y - x) + 2p has limbs in (0.99, 3.01) x 2^26 / 2^25, still a valid right
// operand.  The other way a tight feu already is a loose signed element: the limbs are reinterpreted.
template <int K>
FEU_FN feu feu_from_signed(const int32_t s[10]) {
  feu r;
#pragma unroll
  for (int i = 0; i < 10; ++i) r.v[i] = (u32)(s[i] + (int32_t)((u32)K * feu_p_limb(i)));
  return r;
}
FEU_FN void feu_to_signed(const feu& f, int32_t s[10]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) s[i] = (int32_t)f.v[i];
}

}  // namespace nwc

#if defined(__HIPCC__)
#include "fe25519.h"
namespace nwc {
__device__ __forceinline__ fe feu_as_fe(const feu& f) { fe r; feu_to_signed(f, r.v); return r; }
template <int K>
__device__ __forceinline__ feu feu_from_fe(const fe& f) { return feu_from_signed<K>(f.v); }
// fe_to_words biases by 16p and carries twice: any f <= 8 T
__device__ __forceinline__ bool feu_is_zero(const feu& f) { return fe_is_zero(feu_as_fe(f)); }
__device__ __forceinline__ bool feu_is_negative(const feu& f) { return fe_is_negative(feu_as_fe(f)); }
__device__ __forceinline__ feu feu_sqn(feu f, int n) {
  _Pragma("unroll 1") for (int i = 0; i < n; ++i) f = feu_sq(f);
  return f;
}
}  // namespace nwc
#endif
