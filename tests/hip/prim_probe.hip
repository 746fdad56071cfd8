// Probe library for tests/test_gpu_prims.py (tests/prim_probe.py builds and wraps it): one
// translation unit around the device-only primitives of narwhal_amd/csrc -- the signed field
// (fe25519.h, fe_asm.h), the limb-sliced field and group (fe_sliced.h, ge_sliced.h), the asm half of
// the unsigned field (feu_asm.h), the scalars (sc25519.h), point decoding (ge25519.h,
// ge_u25519.h) and the per-lane group layer (ge25519.h) -- and, for tests/test_gpu_tables.py, two
// readers of the stored point tables (a gather and an audit, below).  Test infrastructure: compiled
// with the library's flags, never linked into it, and kept out of narwhal_amd/csrc so the library's
// build id does not depend on it.
//
// Every entry is  int probe_X(const u32* in, u32* out, u32 n, hipStream_t stream): n records of
// IN_X words at `in`, n records of OUT_X words at `out` (device pointers), one kernel launch, the HIP
// error code back.  One lane per record; the sliced field takes one 16-lane row per record (four
// different records per wave) and the sliced group one wave per record.  Idle lanes of a sliced
// probe stay in the kernel on a clamped record (DPP and the lane swaps need whole rows and waves)
// and store nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fe25519.h"
#include "ge25519.h"
#include "ge_u25519.h"
#include "sc25519.h"
#include "fe_sliced.h"
#include "ge_sliced.h"

#ifndef NWC_PROBE_ID
#define NWC_PROBE_ID "unset"
#endif

using namespace nwc;

namespace {

constexpr int BLOCK = 256;

__device__ __forceinline__ fe ld_fe(const u32* p) {
  fe r;
  _Pragma("unroll") for (int i = 0; i < 10; ++i) r.v[i] = (i32)p[i];
  return r;
}
__device__ __forceinline__ void st_fe(u32* p, const fe& f) {
  _Pragma("unroll") for (int i = 0; i < 10; ++i) p[i] = (u32)f.v[i];
}
__device__ __forceinline__ feu ld_feu(const u32* p) {
  feu r;
  _Pragma("unroll") for (int i = 0; i < 10; ++i) r.v[i] = p[i];
  return r;
}
__device__ __forceinline__ void st_feu(u32* p, const feu& f) {
  _Pragma("unroll") for (int i = 0; i < 10; ++i) p[i] = f.v[i];
}
__device__ __forceinline__ void ld_words(const u32* p, u32 w[8]) {
  _Pragma("unroll") for (int i = 0; i < 8; ++i) w[i] = p[i];
}
__device__ __forceinline__ void st_p3(u32* p, const ge_p3& q) {
  st_fe(p, q.X); st_fe(p + 10, q.Y); st_fe(p + 20, q.Z); st_fe(p + 30, q.T);
}
// limb k of a per-lane element (k = the lane's place in its row, taken mod 10)
__device__ __forceinline__ i32 limb_of(const fe& f, int k) {
  i32 r = 0;
  _Pragma("unroll") for (int i = 0; i < 10; ++i) r = (k % 10 == i) ? f.v[i] : r;
  return r;
}

// ---- signed field ---------------------------------------------------------------------------
// in: f[10] g[10] c.  out: fe_mul(f, g), fe_sq(f), fe_sq2(f), fe_mul_small(f, c)
constexpr int IN_FE_OPS = 21, OUT_FE_OPS = 40;
__global__ void k_fe_ops(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  const u32* r = in + (size_t)t * IN_FE_OPS;
  u32* o = out + (size_t)t * OUT_FE_OPS;
  const fe f = ld_fe(r), g = ld_fe(r + 10);
  const i32 c = (i32)r[20];
  st_fe(o, fe_mul(f, g));
  st_fe(o + 10, fe_sq(f));
  st_fe(o + 20, fe_sq2(f));
  st_fe(o + 30, fe_mul_small(f, c));
}

// in: 8 words.  out: fe_from_words[10], fe_tighten of it[10], fe_to_words of it[8]
constexpr int IN_FE_WORDS = 8, OUT_FE_WORDS = 28;
__global__ void k_fe_words(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  u32 w[8], c[8];
  ld_words(in + (size_t)t * IN_FE_WORDS, w);
  u32* o = out + (size_t)t * OUT_FE_WORDS;
  const fe y = fe_from_words(w);
  st_fe(o, y);
  st_fe(o + 10, fe_tighten(y));
  fe_to_words(y, c);
  _Pragma("unroll") for (int i = 0; i < 8; ++i) o[20 + i] = c[i];
}

// in: a[10] b[10].  out: fe_to_words(a)[8], fe_is_zero(a), fe_is_negative(a), fe_equal(a, b)
constexpr int IN_FE_CANON = 20, OUT_FE_CANON = 11;
__global__ void k_fe_canon(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  const u32* r = in + (size_t)t * IN_FE_CANON;
  u32* o = out + (size_t)t * OUT_FE_CANON;
  const fe a = ld_fe(r), b = ld_fe(r + 10);
  u32 c[8];
  fe_to_words(a, c);
  _Pragma("unroll") for (int i = 0; i < 8; ++i) o[i] = c[i];
  o[8] = fe_is_zero(a) ? 1u : 0u;
  o[9] = fe_is_negative(a) ? 1u : 0u;
  o[10] = fe_equal(a, b) ? 1u : 0u;
}

// in: z[10].  out: fe_pow22523(z), fe_invert(z)
constexpr int IN_FE_POW = 10, OUT_FE_POW = 20;
__global__ void k_fe_pow(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  const fe z = ld_fe(in + (size_t)t * IN_FE_POW);
  u32* o = out + (size_t)t * OUT_FE_POW;
  st_fe(o, fe_pow22523(z));
  st_fe(o + 10, fe_invert(z));
}

// ---- sliced field: one 16-lane row per record ------------------------------------------------
// in: f[10] g[10] c.  out, 16 lanes each: fes_mul(f, g), fes_sq(f), fes_mul_small(f, c),
// fes_from_fe(f), and limb (lane mod 10) of fe_from_fes(fes_from_fe(g)) as every lane sees it
constexpr int IN_FES_OPS = 21, OUT_FES_OPS = 80;
__global__ void k_fes_ops(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 row = blockIdx.x * (BLOCK / 16) + (threadIdx.x >> 4);
  const bool live = row < n;
  const u32 rec = live ? row : n - 1;
  const int k = fes_lane();
  const u32* r = in + (size_t)rec * IN_FES_OPS;
  const fe f = ld_fe(r), g = ld_fe(r + 10);
  const i32 c = (i32)r[20];
  const fes fs = fes_from_fe(f), gs = fes_from_fe(g);
  const fes m = fes_mul(fs, gs), s = fes_sq(fs), ms = fes_mul_small(fs, c);
  const fe back = fe_from_fes(gs);
  if (!live) return;
  u32* o = out + (size_t)rec * OUT_FES_OPS + k;
  o[0] = (u32)m.v;
  o[16] = (u32)s.v;
  o[32] = (u32)ms.v;
  o[48] = (u32)fs.v;
  o[64] = (u32)limb_of(back, k);
}

// in: z[10].  out: fes_pow22523(z), 16 lanes
constexpr int IN_FES_POW = 10, OUT_FES_POW = 16;
__global__ void k_fes_pow(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 row = blockIdx.x * (BLOCK / 16) + (threadIdx.x >> 4);
  const bool live = row < n;
  const u32 rec = live ? row : n - 1;
  const fes z = fes_from_fe(ld_fe(in + (size_t)rec * IN_FES_POW));
  const fes r = fes_pow22523(z);
  if (!live) return;
  out[(size_t)rec * OUT_FES_POW + fes_lane()] = (u32)r.v;
}

// ---- sliced group: one wave per record -------------------------------------------------------
// in: P (X Y Z T), Q (X Y Z T), 80 limbs.  out, once per row of the wave (4 x 81 words):
// gs_to_p3(gs_dbl(P))[40], gs_to_p3(gs_add_cached(P, gs_to_cached(Q)))[40], gs_has_torsion(P)
constexpr int IN_GS = 80, OUT_GS = 4 * 81;
__device__ __forceinline__ gs_p3 ld_gs(const u32* p) {
  gs_p3 r;
  r.X = fes_from_fe(ld_fe(p)); r.Y = fes_from_fe(ld_fe(p + 10));
  r.Z = fes_from_fe(ld_fe(p + 20)); r.T = fes_from_fe(ld_fe(p + 30));
  return r;
}
// gathered by every lane (row broadcasts), before the lanes that store part from the others
__device__ __forceinline__ ge_p3 gs_gather(const gs_p3& q) {
  ge_p3 r;
  r.X = fe_from_fes(q.X); r.Y = fe_from_fes(q.Y); r.Z = fe_from_fes(q.Z); r.T = fe_from_fes(q.T);
  return r;
}
__global__ void k_gs(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 wave = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  const bool live = wave < n;
  const u32 rec = live ? wave : n - 1;
  const u32* r = in + (size_t)rec * IN_GS;
  const gs_p3 P = ld_gs(r), Q = ld_gs(r + 40);
  const ge_p3 d = gs_gather(gs_to_p3(gs_dbl(gs_p3_to_p2(P))));
  const ge_p3 a = gs_gather(gs_to_p3(gs_add_cached(P, gs_to_cached(Q))));
  const bool tor = gs_has_torsion(P, SC_L);
  if (!live || fes_lane() != 0) return;
  u32* o = out + (size_t)rec * OUT_GS + fes_row() * 81;
  st_p3(o, d);
  st_p3(o + 40, a);
  o[80] = tor ? 1u : 0u;
}

// ---- unsigned field, the device (asm) half: the record layout of tests/cpp/feu_host.cpp ------
constexpr int IN_FEU = 20, OUT_FEU = 110;
__global__ void k_feu_field(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  const u32* r = in + (size_t)t * IN_FEU;
  u32* o = out + (size_t)t * OUT_FEU;
  const feu a = ld_feu(r), b = ld_feu(r + 10);
  st_feu(o, feu_mul(a, b));
  st_feu(o + 10, feu_sq(b));
  st_feu(o + 20, feu_sq2(b));
  st_feu(o + 30, feu_add(a, b));
  st_feu(o + 40, feu_sub<2>(a, b));
  st_feu(o + 50, feu_sub<3>(a, b));
  st_feu(o + 60, feu_sub<4>(a, b));
  st_feu(o + 70, feu_weak(a));
  int32_t s[10], ts[10];
  _Pragma("unroll") for (int k = 0; k < 10; ++k) s[k] = (int32_t)(b.v[k] & 0x7fffffffu) - (1 << ((k & 1) ? 24 : 25));
  st_feu(o + 80, feu_from_signed<1>(s));
  st_feu(o + 90, feu_from_signed<2>(s));
  feu_to_signed(a, ts);
  _Pragma("unroll") for (int k = 0; k < 10; ++k) o[100 + k] = (u32)ts[k];
}

// ---- scalars -----------------------------------------------------------------------------------
constexpr int IN_SC_REDUCE = 16, OUT_SC_REDUCE = 8;
__global__ void k_sc_reduce(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  u32 x[16], r[8];
  _Pragma("unroll") for (int i = 0; i < 16; ++i) x[i] = in[(size_t)t * IN_SC_REDUCE + i];
  sc_reduce512(x, r);
  _Pragma("unroll") for (int i = 0; i < 8; ++i) out[(size_t)t * OUT_SC_REDUCE + i] = r[i];
}

constexpr int IN_SC_LT = 8, OUT_SC_LT = 1;
__global__ void k_sc_lt_l(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  u32 s[8];
  ld_words(in + (size_t)t * IN_SC_LT, s);
  out[t] = sc_lt_l(s) ? 1u : 0u;
}

// packed string[9], then digit_at<BITS> of every window as a two's complement word
template <int BITS, int WINDOWS>
__device__ __forceinline__ void recode_probe(const u32 s[8], u32* o) {
  u32 d[9];
  sc_recode_radix<BITS, WINDOWS>(s, d);
  _Pragma("unroll") for (int i = 0; i < 9; ++i) o[i] = d[i];
  _Pragma("unroll 1") for (int w = 0; w < WINDOWS; ++w) o[9 + w] = (u32)digit_at<BITS>(d, w);
}
// in: s[8].  out: radix16[8] radix256[8] radix65536[8], then <12, 22>, <22, 12>, <14, 19> (the
// generic recoding's wrapper, the basepoint comb's and the key comb's shapes)
constexpr int IN_SC_RECODE = 8, OUT_SC_RECODE = 24 + (9 + 22) + (9 + 12) + (9 + 19);
__global__ void k_sc_recode(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  u32 s[8], d[8];
  ld_words(in + (size_t)t * IN_SC_RECODE, s);
  u32* o = out + (size_t)t * OUT_SC_RECODE;
  sc_recode_radix16(s, d);
  _Pragma("unroll") for (int i = 0; i < 8; ++i) o[i] = d[i];
  sc_recode_radix256(s, d);
  _Pragma("unroll") for (int i = 0; i < 8; ++i) o[8 + i] = d[i];
  sc_recode_radix65536(s, d);
  _Pragma("unroll") for (int i = 0; i < 8; ++i) o[16 + i] = d[i];
  recode_probe<12, 22>(s, o + 24);
  recode_probe<22, 12>(s, o + 24 + 31);
  recode_probe<14, 19>(s, o + 24 + 31 + 21);
}

// ---- decoding: per encoding X Y Z T [40], ok, canonical y [8], ycanon_is_small_order ---------
constexpr int DEC = 50;
__device__ __forceinline__ void st_dec(u32* o, const ge_p3& p, bool ok, const u32 yc[8]) {
  st_p3(o, p);
  o[40] = ok ? 1u : 0u;
  _Pragma("unroll") for (int i = 0; i < 8; ++i) o[41 + i] = yc[i];
  o[49] = ycanon_is_small_order(yc) ? 1u : 0u;
}
__global__ void k_decompress1(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  u32 w[8], yc[8];
  ld_words(in + (size_t)t * 8, w);
  ge_p3 p;
  bool ok;
  ge_decompress1(w, p, yc, ok);
  st_dec(out + (size_t)t * DEC, p, ok, yc);
}
// two different encodings per lane
__global__ void k_decompress2(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  u32 w0[8], w1[8], yc[2][8];
  ld_words(in + (size_t)t * 16, w0);
  ld_words(in + (size_t)t * 16 + 8, w1);
  const u32* const w[2] = {w0, w1};
  ge_p3 p[2];
  bool ok[2];
  ge_decompressN<2>(p, w, yc, ok);
  st_dec(out + (size_t)t * 2 * DEC, p[0], ok[0], yc[0]);
  st_dec(out + (size_t)t * 2 * DEC + DEC, p[1], ok[1], yc[1]);
}
__global__ void k_geu_decompress(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  u32 w[8], yc[8];
  ld_words(in + (size_t)t * 8, w);
  geu_p3 p;
  bool ok;
  geu_decompress(w, p, yc, ok);
  ge_p3 q;
  q.X = feu_as_fe(p.X); q.Y = feu_as_fe(p.Y); q.Z = feu_as_fe(p.Z); q.T = feu_as_fe(p.T);
  st_dec(out + (size_t)t * DEC, q, ok, yc);
}

// ---- per-lane group layer (ge25519.h) --------------------------------------------------------
// in: P (X Y Z T), Q (X Y Z T), q = the affine Niels form of Q (ypx ymx xy2d), 110 limbs.
// out: 2P through ge_p1p1_to_p3 [40], _to_p2 [30], _to_p3_acc [40], _to_p2_acc [30]; P + Q and P - Q
// through ge_add_cached [40 each]; P + q and P - q through ge_add_niels [40 each]; ge_p3_neg(P) [40]
constexpr int IN_GE_OPS = 110, OUT_GE_OPS = 340;
__device__ __forceinline__ ge_p3 ld_p3(const u32* p) {
  ge_p3 r;
  r.X = ld_fe(p); r.Y = ld_fe(p + 10); r.Z = ld_fe(p + 20); r.T = ld_fe(p + 30);
  return r;
}
__device__ __forceinline__ void st_p2(u32* p, const ge_p2& q) { st_fe(p, q.X); st_fe(p + 10, q.Y); st_fe(p + 20, q.Z); }
__global__ void k_ge_ops(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  const u32* r = in + (size_t)t * IN_GE_OPS;
  u32* o = out + (size_t)t * OUT_GE_OPS;
  const ge_p3 P = ld_p3(r), Q = ld_p3(r + 40);
  ge_niels q;
  q.ypx = ld_fe(r + 80); q.ymx = ld_fe(r + 90); q.xy2d = ld_fe(r + 100);
  const ge_p1p1 d = ge_p2_dbl(ge_p3_to_p2(P));
  st_p3(o, ge_p1p1_to_p3(d));
  st_p2(o + 40, ge_p1p1_to_p2(d));
  st_p3(o + 70, ge_p1p1_to_p3_acc(d));
  st_p2(o + 110, ge_p1p1_to_p2_acc(d));
  const ge_cached qc = ge_p3_to_cached(Q);
  st_p3(o + 140, ge_p1p1_to_p3(ge_add_cached(P, qc)));
  st_p3(o + 180, ge_p1p1_to_p3(ge_add_cached(P, ge_cached_cneg(qc, true))));
  st_p3(o + 220, ge_p1p1_to_p3(ge_add_niels(P, q)));
  st_p3(o + 260, ge_p1p1_to_p3(ge_add_niels(P, ge_niels_cneg(q, true))));
  st_p3(o + 300, ge_p3_neg(P));
}

// ---- stored point tables (tests/test_gpu_tables.py) -------------------------------------------
// An entry is an affine Niels point: ypx[10] ymx[10] xy2d[10] signed limbs, 120 bytes, or 128 with
// two pad words.  The tables are read through addresses the caller vouches for: the wrapper
// (tests/prim_probe.py) takes them from nwc_diag_table or from a buffer it owns, and checks every
// index against the element count before it launches.
// in: address (lo, hi), stride in bytes (120 or 128; 32 / 4 for the key / flag arrays), index.
// out: the element's words (32 at most), the rest 0
constexpr int IN_GATHER = 4, OUT_GATHER = 32;
__global__ void k_table_gather(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n) return;
  const u32* r = in + (size_t)t * IN_GATHER;
  const uint64_t addr = ((uint64_t)r[1] << 32) | r[0];
  const u32 stride = r[2], words = stride / 4 < 32 ? stride / 4 : 32;
  const u32* src = reinterpret_cast<const u32*>(addr + (uint64_t)r[3] * stride);
  u32* o = out + (size_t)t * OUT_GATHER;
  for (u32 i = 0; i < 32; ++i) o[i] = i < words ? src[i] : 0u;
}

// The audit: one lane per entry of `windows` windows of `entries` entries each, one flag word per
// entry.  Entry j of a window claims to be j * (the window's entry 1); entry 1 of window w is the
// table's element one_offset + w * one_stride.
//   j = 0: the Niels identity, ypx = ymx = 1 mod p                                        (AUDIT_CHAIN)
//   j > 0: entry[j] = entry[j - 1] + entry[1] by the affine addition law of -x^2 + y^2 = 1 + d x^2 y^2,
//          x3 (1 + d x1 x2 y1 y2) = x1 y2 + y1 x2,  y3 (1 - d x1 x2 y1 y2) = y1 y2 + x1 x2,
//          on X = 2x = ypx - ymx and Y = 2y = ypx + ymx:  X3 (16 + d M) = 8 (X1 Y2 + Y1 X2),
//          Y3 (16 - d M) = 8 (Y1 Y2 + X1 X2),  M = X1 X2 Y1 Y2                               (AUDIT_CHAIN)
//   every j: 2 xy2d = d X Y                                                                 (AUDIT_NIELS)
//            |limb| <= 2 x tight for ypx and ymx, tight for xy2d (the bounds come in the record)  (AUDIT_BOUND)
//            the pad words of a 128-byte entry are 0                                        (AUDIT_PAD)
// Only fe_mul, fe_mul_small, fe_add, fe_sub and fe_equal: the group formulas that built the tables
// do not judge them.  With entries 0 and 1 of every window checked exactly by the host, a window
// without a flag is proven entry by entry.  Stored limbs of any size are first carried into tight
// form (fe_mul_small by 1 takes whole 32-bit limbs), so an entry out of bounds still has its value.
// in (one record for the launch): address (lo, hi), stride, windows, entries, one_offset, one_stride,
// tight bound of an even limb, of an odd limb.  out: n = windows x entries flag words
constexpr int IN_AUDIT = 9, OUT_AUDIT = 1;
constexpr u32 AUDIT_CHAIN = 1, AUDIT_NIELS = 2, AUDIT_BOUND = 4, AUDIT_PAD = 8;
struct AuditEntry { fe ypx, ymx, xy2d; bool in_bounds, pad_clear; };
__device__ __forceinline__ AuditEntry audit_load(uint64_t addr, u32 stride, uint64_t idx, u32 tight_even, u32 tight_odd) {
  const u32* src = reinterpret_cast<const u32*>(addr + idx * stride);
  AuditEntry e;
  e.in_bounds = true;
  fe raw[3];
  _Pragma("unroll") for (int k = 0; k < 3; ++k) {
    raw[k] = ld_fe(src + 10 * k);
    _Pragma("unroll") for (int i = 0; i < 10; ++i) {
      const int64_t bound = (int64_t)((i & 1) ? tight_odd : tight_even) * (k < 2 ? 2 : 1);
      const int64_t v = raw[k].v[i];
      e.in_bounds = e.in_bounds && v <= bound && v >= -bound;
    }
  }
  e.ypx = fe_mul_small(raw[0], 1);
  e.ymx = fe_mul_small(raw[1], 1);
  e.xy2d = fe_mul_small(raw[2], 1);
  e.pad_clear = true;
  for (u32 i = 30; i < stride / 4; ++i) e.pad_clear = e.pad_clear && src[i] == 0u;
  return e;
}
__global__ void k_table_audit(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  const uint64_t addr = ((uint64_t)in[1] << 32) | in[0];
  const u32 stride = in[2], windows = in[3], entries = in[4], one_offset = in[5], one_stride = in[6];
  if (t >= n || (uint64_t)t >= (uint64_t)windows * entries) return;
  const u32 w = t / entries, j = t % entries;
  const AuditEntry cur = audit_load(addr, stride, t, in[7], in[8]);
  u32 flags = (cur.in_bounds ? 0u : AUDIT_BOUND) | (cur.pad_clear ? 0u : AUDIT_PAD);
  const fe X3 = fe_sub(cur.ypx, cur.ymx), Y3 = fe_add(cur.ypx, cur.ymx);
  if (!fe_equal(fe_mul_small(cur.xy2d, 2), fe_mul(fe_mul(X3, Y3), FE_D))) flags |= AUDIT_NIELS;
  if (j == 0) {
    if (!fe_equal(cur.ypx, fe_one()) || !fe_equal(cur.ymx, fe_one())) flags |= AUDIT_CHAIN;
  } else {
    const AuditEntry prev = audit_load(addr, stride, (uint64_t)t - 1, in[7], in[8]);
    const AuditEntry one = audit_load(addr, stride, (uint64_t)one_offset + (uint64_t)w * one_stride, in[7], in[8]);
    const fe X1 = fe_sub(prev.ypx, prev.ymx), Y1 = fe_add(prev.ypx, prev.ymx);
    const fe X2 = fe_sub(one.ypx, one.ymx), Y2 = fe_add(one.ypx, one.ymx);
    const fe a = fe_mul(X1, Y2), b = fe_mul(Y1, X2), c = fe_mul(Y1, Y2), e = fe_mul(X1, X2);
    const fe dm = fe_mul(fe_mul(a, b), FE_D);
    fe sixteen = fe_zero();
    sixteen.v[0] = 16;
    const bool x_ok = fe_equal(fe_mul(X3, fe_add(sixteen, dm)), fe_mul_small(fe_add(a, b), 8));
    const bool y_ok = fe_equal(fe_mul(Y3, fe_sub(sixteen, dm)), fe_mul_small(fe_add(c, e), 8));
    if (!x_ok || !y_ok) flags |= AUDIT_CHAIN;
  }
  out[t] = flags;
}

template <class K>
int launch(K kernel, u32 per_block, const u32* in, u32* out, u32 n, hipStream_t stream) {
  if (n == 0) return (int)hipSuccess;
  if (!in || !out) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((n + per_block - 1) / per_block), dim3(BLOCK), 0, stream, in, out, n);
  return (int)hipGetLastError();
}

}  // namespace

#define PROBE(name, kernel, per_block)                                                    \
  extern "C" int name(const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t stream) { \
    return launch(kernel, per_block, in, out, n, stream);                                 \
  }

PROBE(probe_fe_ops, k_fe_ops, BLOCK)
PROBE(probe_fe_words, k_fe_words, BLOCK)
PROBE(probe_fe_canon, k_fe_canon, BLOCK)
PROBE(probe_fe_pow, k_fe_pow, BLOCK)
PROBE(probe_fes_ops, k_fes_ops, BLOCK / 16)
PROBE(probe_fes_pow, k_fes_pow, BLOCK / 16)
PROBE(probe_gs, k_gs, BLOCK / 64)
PROBE(probe_feu_field, k_feu_field, BLOCK)
PROBE(probe_sc_reduce, k_sc_reduce, BLOCK)
PROBE(probe_sc_lt_l, k_sc_lt_l, BLOCK)
PROBE(probe_sc_recode, k_sc_recode, BLOCK)
PROBE(probe_decompress1, k_decompress1, BLOCK)
PROBE(probe_decompress2, k_decompress2, BLOCK)
PROBE(probe_geu_decompress, k_geu_decompress, BLOCK)
PROBE(probe_ge_ops, k_ge_ops, BLOCK)
PROBE(probe_table_gather, k_table_gather, BLOCK)
// one parameter record at `in`, n flag words at `out` (n = windows x entries)
PROBE(probe_table_audit, k_table_audit, BLOCK)

// words per record (in, out) of an entry, so the wrapper's table is checked against this file
extern "C" int probe_record_words(const char* name, int* in_words, int* out_words) {
  struct { const char* n; int i, o; } const t[] = {
      {"probe_fe_ops", IN_FE_OPS, OUT_FE_OPS},       {"probe_fe_words", IN_FE_WORDS, OUT_FE_WORDS},
      {"probe_fe_canon", IN_FE_CANON, OUT_FE_CANON}, {"probe_fe_pow", IN_FE_POW, OUT_FE_POW},
      {"probe_fes_ops", IN_FES_OPS, OUT_FES_OPS},    {"probe_fes_pow", IN_FES_POW, OUT_FES_POW},
      {"probe_gs", IN_GS, OUT_GS},                   {"probe_feu_field", IN_FEU, OUT_FEU},
      {"probe_sc_reduce", IN_SC_REDUCE, OUT_SC_REDUCE}, {"probe_sc_lt_l", IN_SC_LT, OUT_SC_LT},
      {"probe_sc_recode", IN_SC_RECODE, OUT_SC_RECODE}, {"probe_decompress1", 8, DEC},
      {"probe_decompress2", 16, 2 * DEC},            {"probe_geu_decompress", 8, DEC},
      {"probe_ge_ops", IN_GE_OPS, OUT_GE_OPS},       {"probe_table_gather", IN_GATHER, OUT_GATHER},
      {"probe_table_audit", IN_AUDIT, OUT_AUDIT},
  };
  for (const auto& e : t) {
    const char *a = e.n, *b = name;
    while (*a && *a == *b) { ++a; ++b; }
    if (*a == 0 && *b == 0) { *in_words = e.i; *out_words = e.o; return 0; }
  }
  return -1;
}

extern "C" const char* probe_build_id() {
  static const char id[] = "NWC_PROBE_ID:" NWC_PROBE_ID;
  return id + 13;
}
