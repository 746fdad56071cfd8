// Second probe library, for tests/test_gpu_half.py (tests/half_probe.py builds and wraps it): the
// layer between the primitives (tests/hip/prim_probe.hip) and the verdicts -- the half-size scalars
// (lattice.h: lat::reduce as the device compiles it), the challenge, the basepoint scalar's path
// (ds_mod_l, base_digits, recode24 and the LDS layout base_fetch reads), the recodings of |c| and d
// (recode16, recode256, geu_recode4 and every way of draining them), the wave's window counts and
// the two half-size ladders.  Those functions live in kernels.hip, not in a header, so this
// translation unit includes kernels.hip whole and adds entries of its own.  Test infrastructure:
// compiled with the library's flags, never linked into it, kept out of narwhal_amd/csrc so the
// library's build id does not depend on it, and it launches only the kernels named k_hp_* below
// (none of kernels.hip's own).
//
// Scalar-side entries:  int probe_X(const u32* in, u32* out, u32 n, hipStream_t stream), as in
// prim_probe.hip: n records of IN words, n records of OUT words, one lane per record, 256-thread
// blocks.  The lanes of a ragged last wave stay in the kernel on record 0, as k_verify keeps idle
// lanes on equation 0 (the wave votes and the wave-uniform window counts need whole waves), and
// store nothing.
//
// Ladder entries:  int probe_X(const u32* par, const u32* in, u32* out, u32 n, hipStream_t stream)
// with one parameter record per launch (PAR words): the address of base24 (nwc_diag_table), of a
// test-owned scratch buffer of 2 * TAB_BYTES_PER_LANE bytes per lane slot and the number of slots,
// and for the cached entry the address of the committee's key tables and the number of keys.  The
// kernels declare the LDS block k_verify<true, ..> declares.
//
// The glue of the two ladder kernels restates about ten lines of verify_half (kernels.hip), after
// lat::reduce, line for line: it is a copy, so an edit of verify_half's glue is not seen here.  Every
// piece of that glue has a scalar-side entry of its own above, and the real glue's behaviour on
// ordinary values stays pinned by the verdict tests.  The probe's register allocation is not
// k_verify's: these entries test the source-level functions (recodings, table builders, ladders),
// not the machine code of the headline kernel.
//
// The ladder entries index device tables with their digits.  A lane whose (c, d) are outside the
// ladders' contract (a bit length above 146, d even, a key index past the committee) runs on c = 0,
// d = 1, key 0 instead and reports flag 2 in its `ok` word; the test hands no such record in.
#include "kernels.hip"

#ifndef NWC_PROBE_ID
#define NWC_PROBE_ID "unset"
#endif
#define HP_EXPORT extern "C" __attribute__((visibility("default")))

using namespace nwc;

namespace {

constexpr int BLOCK = 256;

// this lane's record: its own, or record 0 for an idle lane of the last wave
__device__ __forceinline__ u32 record_of(u32 n, bool& live) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  live = t < n;
  return live ? t : 0u;
}

// in: k[8].  out: c[5], d[5], c_neg, ok, bits of lat::reduce (the kernels' instantiation)
constexpr int IN_LAT = 8, OUT_LAT = 13;
__global__ void k_hp_lat_reduce(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  bool live;
  const u32 t = record_of(n, live);
  u32 k[8];
  _Pragma("unroll") for (int i = 0; i < 8; ++i) k[i] = in[(size_t)t * IN_LAT + i];
  const lat::HalfScalars h = lat::reduce(k);
  if (!live) return;
  u32* o = out + (size_t)t * OUT_LAT;
  _Pragma("unroll") for (int i = 0; i < 5; ++i) { o[i] = h.c[i]; o[5 + i] = h.d[i]; }
  o[10] = h.c_neg ? 1u : 0u;
  o[11] = h.ok ? 1u : 0u;
  o[12] = (u32)h.bits;
}

// in: R[8], A[8], M[8].  out: challenge<false>[8], challenge<true>[8]
constexpr int IN_CHAL = 24, OUT_CHAL = 16;
__global__ void k_hp_challenge(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  bool live;
  const u32 t = record_of(n, live);
  u32 rw[8], aw[8], mw[8], k0[8], k1[8];
  _Pragma("unroll") for (int i = 0; i < 8; ++i) {
    rw[i] = in[(size_t)t * IN_CHAL + i];
    aw[i] = in[(size_t)t * IN_CHAL + 8 + i];
    mw[i] = in[(size_t)t * IN_CHAL + 16 + i];
  }
  challenge<false>(rw, aw, mw, k0);
  challenge<true>(rw, aw, mw, k1);
  if (!live) return;
  u32* o = out + (size_t)t * OUT_CHAL;
  _Pragma("unroll") for (int i = 0; i < 8; ++i) { o[i] = k0[i]; o[8 + i] = k1[i]; }
}

// in: d[5], s[8].  out: eb[8] (ds_mod_l); el's six digits and eh's five (base_digits), least
// significant first; the eleven digits read back from the LDS words base_digits_park wrote, by
// base_fetch's indexing (d0 of windows 0, 6, .., 30, then d1 of windows 0, 6, .., 24); the number of
// digits base_window_digits hands out over windows 0..36.
constexpr int IN_BASE = 13, OUT_BASE = 31;
__global__ void k_hp_base_digits(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  __shared__ i32 lds[BASE_DIGIT_WORDS * BLOCK];
  const BaseDigits bd{lds + threadIdx.x};
  bool live;
  const u32 t = record_of(n, live);
  u32 d[5], s[8], eb[8];
  _Pragma("unroll") for (int i = 0; i < 5; ++i) d[i] = in[(size_t)t * IN_BASE + i];
  _Pragma("unroll") for (int i = 0; i < 8; ++i) s[i] = in[(size_t)t * IN_BASE + 5 + i];
  ds_mod_l(d, s, eb);
  Digits24 el, eh;
  base_digits(d, s, el, eh);
  base_digits_park(bd, el, eh);
  if (!live) return;
  u32* o = out + (size_t)t * OUT_BASE;
  _Pragma("unroll") for (int i = 0; i < 8; ++i) o[i] = eb[i];
  _Pragma("unroll") for (int i = 0; i < B24_LO_DIGITS; ++i) o[8 + i] = (u32)el.d[i];
  _Pragma("unroll") for (int i = 0; i < B24_HI_DIGITS; ++i) o[14 + i] = (u32)eh.d[i + B24_LO_DIGITS - B24_HI_DIGITS];
  int handed = 0;
  for (int w = HALF_WINDOWS_MAX - 1; w >= 0; --w) {
    const int nb = base_window_digits(w);
    handed += nb;
    if (nb) {
      const int i = w / 6;                                   // base_fetch
      o[19 + i] = (u32)bd.p[i * 256];
      if (nb == 2) o[25 + i] = (u32)bd.p[(BD_HI + i) * 256];
    }
  }
  o[30] = (u32)handed;
}

// in: x[5], W (33..37), W4 (66..74); W and W4 are taken from the wave's first lane (the kernels hold
// them in scalar registers), x < 2^(4W-1) and x < 2^(2 W4 - 1).  out:
//   [0, 6)    recode16(x, W): w[5], top          [6, 42)   digits W-2 .. 0 by next16, at their window
//   [42, 78)  the same digits by digit16_of      [78, 83)  recode256(x, ndig).w, ndig = (((W | 1) - 1) >> 1) + 1
//   [83, 102) digits ndig-1 .. 0 by next256, at their index           [102] ndig
//   [103]     geu_recode4(x, W4, y)              [104, 109) y[5]      [109, 182) digits 0 .. W4-2 by geu_digit4
// Slots past a string's length hold 0x7777.
constexpr int IN_RECODE = 7, OUT_RECODE = 182;
__global__ void k_hp_half_recode(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  bool live;
  const u32 t = record_of(n, live);
  const u32* r = in + (size_t)t * IN_RECODE;
  u32 x[5];
  _Pragma("unroll") for (int i = 0; i < 5; ++i) x[i] = r[i];
  const int W = __builtin_amdgcn_readfirstlane((int)r[5]);
  const int W4 = __builtin_amdgcn_readfirstlane((int)r[6]);
  if (W < HALF_WINDOWS_MIN || W > HALF_WINDOWS_MAX || W4 < JOINT_WINDOWS_MIN || W4 > JOINT_WINDOWS_MAX) return;
  if (!live) return;
  u32* o = out + (size_t)t * OUT_RECODE;
  for (int i = 0; i < OUT_RECODE; ++i) o[i] = 0x7777u;
  const Digits16 d16 = recode16(x, W);
  _Pragma("unroll") for (int i = 0; i < 5; ++i) o[i] = d16.w[i];
  o[5] = (u32)d16.top;
  Digits16 q = d16;
  for (int w = W - 2; w >= 0; --w) {
    o[6 + w] = (u32)next16(q);
    o[42 + w] = (u32)digit16_of(d16, w, W);
  }
  const int ndig = (((W | 1) - 1) >> 1) + 1;
  Digits256 d256 = recode256(x, ndig);
  _Pragma("unroll") for (int i = 0; i < 5; ++i) o[78 + i] = d256.w[i];
  for (int i = ndig - 1; i >= 0; --i) o[83 + i] = (u32)next256(d256);
  o[102] = (u32)ndig;
  u32 y[5];
  o[103] = (u32)geu_recode4(x, W4, y);
  _Pragma("unroll") for (int i = 0; i < 5; ++i) o[104 + i] = y[i];
  for (int w = 0; w < W4 - 1; ++w) {
    u32 word = y[0];
    _Pragma("unroll") for (int i = 1; i < 5; ++i) word = (w >> 4) == i ? y[i] : word;
    o[109 + w] = (u32)geu_digit4(word, w);
  }
}

// in: a bit length.  out: wave_windows, wave_windows4 of the lane's wave
constexpr int IN_WW = 1, OUT_WW = 2;
__global__ void k_hp_wave_windows(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  bool live;
  const u32 t = record_of(n, live);
  const int bits = (int)in[t];
  const int w16 = wave_windows(bits), w4 = wave_windows4(bits);
  if (!live) return;
  out[(size_t)t * OUT_WW] = (u32)w16;
  out[(size_t)t * OUT_WW + 1] = (u32)w4;
}

// ---- ladders ----------------------------------------------------------------------------------
// par: base24 (2 words), scratch (2), lane slots, key tables (2), keys
constexpr int PAR = 8;
struct LadderPar {
  const ge_niels_pad* T24;
  uint8_t* scratch;
  u32 slots;
  const ge_niels* key_tables;
  u32 keys;
};
__device__ __forceinline__ LadderPar load_par(const u32* par) {
  LadderPar p;
  p.T24 = reinterpret_cast<const ge_niels_pad*>(((uint64_t)par[1] << 32) | par[0]);
  p.scratch = reinterpret_cast<uint8_t*>(((uint64_t)par[3] << 32) | par[2]);
  p.slots = par[4];
  p.key_tables = reinterpret_cast<const ge_niels*>(((uint64_t)par[6] << 32) | par[5]);
  p.keys = par[7];
  return p;
}
__device__ __forceinline__ bool in_contract(const u32 c[5], const u32 d[5]) {
  return lat::bitlen5(c) <= lat::HALF_BITS && lat::bitlen5(d) <= lat::HALF_BITS && (d[0] & 1u);
}

// in: c[5] (|c|), c_neg, d[5], s[8], A[8], R[8].  out: X, Y, Z of the ladder's result (unsigned
// limbs), ident as verify_half forms it, W, ok (bit 0: both points decode; bit 1: out of contract)
constexpr int IN_LADDER_U = 35, OUT_LADDER = 33;
__global__ __launch_bounds__(256, NWC_VERIFY_WAVES_PER_SIMD) void k_hp_half_ladder_u(const u32* __restrict__ par,
                                                                                     const u32* __restrict__ in,
                                                                                     u32* __restrict__ out, u32 n) {
  __shared__ uint4 lds[4 * STAGE_U4_PER_WAVE + BASE_DIGIT_WORDS * 64];
  const LadderPar lp = load_par(par);
  if ((uint64_t)gridDim.x * BLOCK > lp.slots) return;
  uint4* stage = lds + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * STAGE_U4_PER_WAVE;
  const BaseDigits bd{reinterpret_cast<i32*>(lds + 4 * STAGE_U4_PER_WAVE) + threadIdx.x};
  const size_t slot = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const LaneTable ta{reinterpret_cast<uint4*>(lp.scratch + slot * 2 * TAB_BYTES_PER_LANE)};
  bool live;
  const u32 t = record_of(n, live);
  const u32* r = in + (size_t)t * IN_LADDER_U;
  lat::HalfScalars h;
  u32 sw[8], aw[8], rw[8];
  _Pragma("unroll") for (int i = 0; i < 5; ++i) { h.c[i] = r[i]; h.d[i] = r[6 + i]; }
  h.c_neg = r[5] != 0;
  _Pragma("unroll") for (int i = 0; i < 8; ++i) { sw[i] = r[11 + i]; aw[i] = r[19 + i]; rw[i] = r[27 + i]; }
  const bool fits = in_contract(h.c, h.d);
  if (!fits) {
    _Pragma("unroll") for (int i = 0; i < 5; ++i) { h.c[i] = 0; h.d[i] = 0; }
    h.d[0] = 1;
  }
  const int cb = lat::bitlen5(h.c), db = lat::bitlen5(h.d);
  h.bits = cb > db ? cb : db;
  // ---- the uncached branch of verify_half after lat::reduce
  geu_p3 A, R;
  u32 ya[8], yr[8];
  bool oka, okr;
  decompress_u(&A, aw, ya, &oka);
  decompress_u(&R, rw, yr, &okr);
  const int W = wave_windows4(h.bits);
  {
    Digits24 el, eh;
    base_digits(h.d, sw, el, eh);
    base_digits_park(bd, el, eh);
  }
  int c_top, d_top;
  {
    u32 y[5];
    c_top = geu_recode4(h.c, W, y);
    park4(bd, BD_C, y);
    d_top = geu_recode4(h.d, W, y);
    park4(bd, BD_D, y);
  }
  build_joint_table_u(ta, geu_p3_neg(A, !h.c_neg), geu_p3_neg(R, true));
  const geu_p2 q = half_scalarmult(ta, c_top, d_top, bd, lp.T24, stage, W);
  const bool ident = feu_is_zero(q.X) && feu_is_zero(feu_sub<2>(q.Y, q.Z));
  // ----
  if (!live) return;
  u32* o = out + (size_t)t * OUT_LADDER;
  _Pragma("unroll") for (int i = 0; i < 10; ++i) { o[i] = q.X.v[i]; o[10 + i] = q.Y.v[i]; o[20 + i] = q.Z.v[i]; }
  o[30] = ident ? 1u : 0u;
  o[31] = (u32)W;
  o[32] = (oka && okr ? 1u : 0u) | (fits ? 0u : 2u);
}

// in: c[5], c_neg, d[5], s[8], key index, R[8].  out as above (signed limbs)
constexpr int IN_LADDER_C = 28;
__global__ __launch_bounds__(256, NWC_VERIFY_WAVES_PER_SIMD) void k_hp_half_ladder_cached(const u32* __restrict__ par,
                                                                                          const u32* __restrict__ in,
                                                                                          u32* __restrict__ out, u32 n) {
  __shared__ uint4 lds[4 * STAGE_U4_PER_WAVE + BASE_DIGIT_WORDS * 64];
  const LadderPar lp = load_par(par);
  if ((uint64_t)gridDim.x * BLOCK > lp.slots || lp.keys == 0) return;
  uint4* stage = lds + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * STAGE_U4_PER_WAVE;
  const BaseDigits bd{reinterpret_cast<i32*>(lds + 4 * STAGE_U4_PER_WAVE) + threadIdx.x};
  const size_t slot = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const LaneTable tr{reinterpret_cast<uint4*>(lp.scratch + slot * 2 * TAB_BYTES_PER_LANE + TAB_BYTES_PER_LANE)};
  bool live;
  const u32 t = record_of(n, live);
  const u32* r = in + (size_t)t * IN_LADDER_C;
  lat::HalfScalars h;
  u32 sw[8], rw[8];
  _Pragma("unroll") for (int i = 0; i < 5; ++i) { h.c[i] = r[i]; h.d[i] = r[6 + i]; }
  h.c_neg = r[5] != 0;
  _Pragma("unroll") for (int i = 0; i < 8; ++i) { sw[i] = r[11 + i]; rw[i] = r[20 + i]; }
  u32 key = r[19];
  const bool fits = in_contract(h.c, h.d) && key < lp.keys;
  if (!fits) {
    _Pragma("unroll") for (int i = 0; i < 5; ++i) { h.c[i] = 0; h.d[i] = 0; }
    h.d[0] = 1;
    key = 0;
  }
  const int cb = lat::bitlen5(h.c), db = lat::bitlen5(h.d);
  h.bits = cb > db ? cb : db;
  // ---- the cached branch of verify_half after lat::reduce
  ge_p3 R[1];
  u32 yr[1][8];
  bool r_ok[1];
  decompress_k<1>(R, rw, yr, r_ok);
  const int W = wave_windows(h.bits) | 1;
  {
    Digits24 el, eh;
    base_digits(h.d, sw, el, eh);
    base_digits_park(bd, el, eh);
  }
  const Digits16 dd = recode16(h.d, W);
  const Digits256 ca = recode256(h.c, ((W - 1) >> 1) + 1);
  build_table(tr, ge_p3_neg(R[0]));
  const ge_p2 q = half_scalarmult_cached(tr, dd, ca, h.c_neg, lp.key_tables + (size_t)key * 129, bd, lp.T24, stage, W);
  const bool ident = fe_is_zero(q.X) && fe_is_zero(fe_sub(q.Y, q.Z));
  // ----
  if (!live) return;
  u32* o = out + (size_t)t * OUT_LADDER;
  _Pragma("unroll") for (int i = 0; i < 10; ++i) { o[i] = (u32)q.X.v[i]; o[10 + i] = (u32)q.Y.v[i]; o[20 + i] = (u32)q.Z.v[i]; }
  o[30] = ident ? 1u : 0u;
  o[31] = (u32)W;
  o[32] = (r_ok[0] ? 1u : 0u) | (fits ? 0u : 2u);
}

template <class K>
int launch(K kernel, const u32* in, u32* out, u32 n, hipStream_t stream) {
  if (n == 0) return (int)hipSuccess;
  if (!in || !out) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, in, out, n);
  return (int)hipGetLastError();
}
template <class K>
int launch_ladder(K kernel, const u32* par, const u32* in, u32* out, u32 n, hipStream_t stream) {
  if (n == 0) return (int)hipSuccess;
  if (!par || !in || !out) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, par, in, out, n);
  return (int)hipGetLastError();
}

}  // namespace

#define HALF_PROBE(name, kernel)                                                       \
  HP_EXPORT int name(const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t stream) { \
    return launch(kernel, in, out, n, stream);                                         \
  }
#define HALF_PROBE_LADDER(name, kernel)                                                                      \
  HP_EXPORT int name(const uint32_t* par, const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t stream) { \
    return launch_ladder(kernel, par, in, out, n, stream);                                                   \
  }

HALF_PROBE(probe_lat_reduce, k_hp_lat_reduce)
HALF_PROBE(probe_challenge, k_hp_challenge)
HALF_PROBE(probe_base_digits, k_hp_base_digits)
HALF_PROBE(probe_half_recode, k_hp_half_recode)
HALF_PROBE(probe_wave_windows, k_hp_wave_windows)
HALF_PROBE_LADDER(probe_half_ladder_u, k_hp_half_ladder_u)
HALF_PROBE_LADDER(probe_half_ladder_cached, k_hp_half_ladder_cached)

// words per record (in, out) of an entry, so the wrapper's table is checked against this file; the
// ladder entries' parameter record has probe_ladder_par_words() words
HP_EXPORT int probe_record_words(const char* name, int* in_words, int* out_words) {
  struct { const char* n; int i, o; } const t[] = {
      {"probe_lat_reduce", IN_LAT, OUT_LAT},          {"probe_challenge", IN_CHAL, OUT_CHAL},
      {"probe_base_digits", IN_BASE, OUT_BASE},       {"probe_half_recode", IN_RECODE, OUT_RECODE},
      {"probe_wave_windows", IN_WW, OUT_WW},          {"probe_half_ladder_u", IN_LADDER_U, OUT_LADDER},
      {"probe_half_ladder_cached", IN_LADDER_C, OUT_LADDER},
  };
  for (const auto& e : t) {
    const char *a = e.n, *b = name;
    while (*a && *a == *b) { ++a; ++b; }
    if (*a == 0 && *b == 0) { *in_words = e.i; *out_words = e.o; return 0; }
  }
  return -1;
}
HP_EXPORT int probe_ladder_par_words() { return PAR; }
// bytes of scratch per lane slot of the ladder entries
HP_EXPORT int probe_ladder_slot_bytes() { return (int)(2 * TAB_BYTES_PER_LANE); }

HP_EXPORT const char* probe_build_id() {
  static const char id[] = "NWC_HALF_PROBE_ID:" NWC_PROBE_ID;
  return id + 18;
}
