// Edwards25519 group arithmetic on the non-negative field (fe_u25519.h): the formulas of
// ge25519.h (add-2008-hwcd-3, dbl-2008-hwcd) with every subtraction biased and every operand's
// class (fe_u25519.h: multiples of the tight bound T) named at its call site.  Host-compilable up
// to the decompression, which needs fe25519.h's canonical encoding.
//
// A completed point (X:Y:Z:T) is always converted with the products X.T, Z.Y, Z.T, X.Y: X and Z
// are LEFT operands (any class up to 9.5 T), T and Y RIGHT operands (<= 3.3 T), so every formula
// below leaves T and Y at 3 T or less.  Where two subtractions would stack up to 4 T on T, one
// feu_weak (a parallel 32-bit carry, ~30 VOP2) brings it back to T.
// Table entries keep 2Z instead of Z, so the doubled Z.Z' product of an addition arrives tight.
#pragma once
#include "fe_u25519.h"
#include "feu_consts.h"

namespace nwc {

struct geu_p2 { feu X, Y, Z; };
struct geu_p3 { feu X, Y, Z, T; };
struct geu_p1p1 { feu X, Y, Z, T; };
struct geu_cached { feu YpX, YmX, Z2, T2d; };   // (Y+X, Y-X, 2Z, 2dT)

// p: X <= 5 T, Z <= 4 T (left); T, Y <= 3 T (right)
FEU_FN geu_p2 geu_p1p1_to_p2(const geu_p1p1& p) {
  geu_p2 r;
  r.X = feu_mul(p.X, p.T);   // 5 T x 3 T
  r.Y = feu_mul(p.Z, p.Y);   // 4 T x 3 T
  r.Z = feu_mul(p.Z, p.T);   // 4 T x 3 T
  return r;
}
FEU_FN geu_p3 geu_p1p1_to_p3(const geu_p1p1& p) {
  geu_p3 r;
  r.X = feu_mul(p.X, p.T);   // 5 T x 3 T
  r.Y = feu_mul(p.Z, p.Y);   // 4 T x 3 T
  r.Z = feu_mul(p.Z, p.T);   // 4 T x 3 T
  r.T = feu_mul(p.X, p.Y);   // 5 T x 3 T
  return r;
}

// dbl-2008-hwcd, a = -1, from (X:Y:Z).  X <= 2 T, Y <= T (so X + Y <= 3 T), Z <= T.
// Out: X = E 4 T, Y = -H 2 T, Z = G 3 T, T = -F tight.
FEU_FN geu_p1p1 geu_p2_dbl(const geu_p2& p) {
  geu_p1p1 r;
  const feu xx = feu_sq(p.X);                  // 2 T
  const feu yy = feu_sq(p.Y);                  // T
  const feu b = feu_sq2(p.Z);                  // T
  const feu a = feu_sq(feu_add(p.X, p.Y));     // 3 T
  r.Y = feu_add(yy, xx);                       // 2 T
  r.Z = feu_sub<2>(yy, xx);                    // T + 2p - T: 3 T
  r.X = feu_sub<3>(a, r.Y);                    // T + 3p - 2 T: 4 T
  // b - G = b + xx - yy: 4 T, and the right operand of X.T and Z.T, so carried once
  r.T = feu_weak(feu_sub<2>(feu_add(b, xx), yy));
  return r;
}

// p + q for an extended p (all four tight) and q given as (qa, qb, q2z, qt) = (Y+X, Y-X, 2Z, 2dT),
// each <= 3 T; neg: add -q instead -- the caller passes (Y-X, Y+X) for (qa, qb), and the sign of
// 2dT moves onto the sum and difference below.  Out: X 3 T, Y 2 T, Z and T <= 3 T.
FEU_FN geu_p1p1 geu_add_cached(const geu_p3& p, const feu& qa, const feu& qb, const feu& q2z, const feu& qt,
                               bool neg) {
  geu_p1p1 r;
  const feu pp = feu_mul(feu_add(p.Y, p.X), qa);      // 2 T x 3 T
  const feu mm = feu_mul(feu_sub<2>(p.Y, p.X), qb);   // 3 T x 3 T
  r.X = feu_sub<2>(pp, mm);                           // 3 T
  r.Y = feu_add(pp, mm);                              // 2 T
  const feu zz2 = feu_mul(p.Z, q2z);                  // T x 3 T
  const feu tt = feu_mul(p.T, qt);                    // T x 3 T
  const feu s = feu_add(zz2, tt);                     // 2 T
  const feu d = feu_sub<2>(zz2, tt);                  // 3 T
  r.Z = feu_select(s, d, neg);
  r.T = feu_select(d, s, neg);
  return r;
}

// p + q for an extended p (tight) and an affine Niels q = (y+x, y-x, 2dxy) from a signed table:
// qa, qb <= 3.01 T (a sum of two signed tight elements + 2p), qt <= 1.51 T (a signed tight element
// + p); neg as above.  Out: X 3 T, Y 2 T, Z 4 T, T tight (2Z + 2p - tt is 4 T: carried).
FEU_FN geu_p1p1 geu_add_niels(const geu_p3& p, const feu& qa, const feu& qb, const feu& qt, bool neg) {
  geu_p1p1 r;
  const feu pp = feu_mul(feu_add(p.Y, p.X), qa);      // 2 T x 3.01 T
  const feu mm = feu_mul(feu_sub<2>(p.Y, p.X), qb);   // 3 T x 3.01 T
  r.X = feu_sub<2>(pp, mm);                           // 3 T
  r.Y = feu_add(pp, mm);                              // 2 T
  const feu zz2 = feu_add(p.Z, p.Z);                  // 2 T
  const feu tt = feu_mul(p.T, qt);                    // T x 1.51 T
  const feu s = feu_add(zz2, tt);                     // 3 T
  const feu d = feu_sub<2>(zz2, tt);                  // 4 T
  r.Z = feu_select(s, d, neg);                        // 4 T, a left operand
  r.T = feu_weak(feu_select(d, s, neg));
  return r;
}

// (Y+X, Y-X, 2Z, 2dT) of an extended point with X, T <= 2 T (a decoded point or its negative: X is
// r or 2p - r, so X <= 2p limb by limb) and Y, Z tight.  Out: YpX, YmX 3 T, Z2 2 T, T2d tight.
FEU_FN geu_cached geu_p3_to_cached(const geu_p3& p) {
  geu_cached r;
  r.YpX = feu_add(p.Y, p.X);           // 3 T
  r.YmX = feu_sub<2>(p.Y, p.X);        // T + 2p - X: 3 T
  r.Z2 = feu_add(p.Z, p.Z);            // 2 T
  r.T2d = feu_mul(p.T, FEU_D2);        // 2 T x T
  return r;
}
// X, T <= 2p limb by limb in (tight, or 2p - tight), the same out: 2 T
FEU_FN geu_p3 geu_p3_neg(const geu_p3& p, bool neg) {
  geu_p3 r = p;
  r.X = feu_select(p.X, feu_neg<2>(p.X), neg);
  r.T = feu_select(p.T, feu_neg<2>(p.T), neg);
  return r;
}

// ---- the joint signed radix-4 table of two decoded points, its recoding and its ladder --------
// The uncached half-size ladder computes c P + d Q (P = +-A, Q = -R) two scalar bits of each per
// window from ONE table of a P + b Q, a, b in {-2..2}: 12 points up to sign and the identity.
// Entry index of (a, b): |5 a + b| (0 identity; 1, 2: Q, 2Q; 3..7: P - 2Q .. P + 2Q; 8..12:
// 2P - 2Q .. 2P + 2Q); the sign of 5 a + b is the sign of the pair, so j = 5 a + b is the joint code.
// P and Q arrive as decoded (Z = 1, T = X Y, X and T of class 2 T: r or 2p - r), which the
// builder uses: 2 Z^2 and 2 Z1 Z2 are the constant 2, 2 X Y is 2 T, and adding P or Q to a running
// point is a Niels addition (3M).  Every formula is the unified one, complete on this curve, so
// P = +-Q, small-order points and the identity take the same path as any other input.
// Keeps the instruction scheduler from interleaving two independent chains of field operations
// (each keeps a point's worth of registers live): the 2-waves-per-SIMD register budget.
#if defined(__HIP_DEVICE_COMPILE__)
#define GEU_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define GEU_SCHED_FENCE() ((void)0)
#endif
constexpr int JOINT_ENTRIES = 13;
constexpr int JOINT_WINDOWS_MIN = 66, JOINT_WINDOWS_MAX = 74;
FEU_FN int geu_joint_code(int a, int b) { return 5 * a + b; }

FEU_FN feu feu_two() { feu r = feu_zero(); r.v[0] = 2; return r; }

// 2 P of a decoded point (dbl-2008-hwcd with Z = 1): B = 2 Z^2 = 2, and E = (X + Y)^2 - X^2 - Y^2 =
// 2 X Y = 2 T costs no square.  X, T <= 2 T, Y tight.  Out as geu_p2_dbl: X 4 T, Y 2 T, Z 3 T, T tight.
FEU_FN geu_p1p1 geu_dbl_affine(const geu_p3& p) {
  geu_p1p1 r;
  const feu xx = feu_sq(p.X);                  // 2 T
  const feu yy = feu_sq(p.Y);                  // T
  r.X = feu_add(p.T, p.T);                     // 4 T
  r.Y = feu_add(yy, xx);                       // 2 T
  r.Z = feu_sub<2>(yy, xx);                    // T + 2p - T: 3 T
  r.T = feu_weak(feu_sub<2>(feu_add(feu_two(), xx), yy));   // 2 + T + 2p - T: carried
  return r;
}
// P + Q (neg: P - Q) of two decoded points: D = 2 Z1 Z2 = 2, and tt = T_P . 2d T_Q is shared by the
// two (it changes sign with Q).  (pa, pb) = (Y + X, Y - X) of P, (qa, qb) the same of Q, swapped by
// the caller for -Q: each 3 T; tt tight.  Out: X 3 T, Y 2 T, Z and T <= 3 T (2 + tt is tight: limb 0 of
// a product is an exact mask, so + 2 stays in T's slack; 2 + 2p - tt <= 2p + 2).
FEU_FN geu_p1p1 geu_add_affine(const feu& pa, const feu& pb, const feu& qa, const feu& qb, const feu& tt, bool neg) {
  geu_p1p1 r;
  const feu pp = feu_mul(pa, qa);              // 3 T x 3 T
  const feu mm = feu_mul(pb, qb);              // 3 T x 3 T
  r.X = feu_sub<2>(pp, mm);                    // 3 T
  r.Y = feu_add(pp, mm);                       // 2 T
  const feu g = feu_add(feu_two(), tt);        // tight
  const feu f = feu_sub<2>(feu_two(), tt);     // 2 + 2p - T
  r.Z = feu_select(g, f, neg);
  r.T = feu_select(f, g, neg);
  return r;
}

// The table: tab(e, entry) stores entry e as (Y+X, Y-X, 2Z, 2dT) with every coordinate <= 3 T
// (kernels.hip packs it tight), tab.load(e, k) reads coordinate k of a stored entry back, tight.
// 12S + 69M.  P and Q die after their doublings and their own entries: the loop holds the shared
// product tt and ONE running point (P + Q, then P - Q) and reads the coordinates of P and Q back
// from their entries where it needs them, as the ladder's additions do.
template <class Tab>
FEU_FN void geu_build_joint(const Tab& tab, const geu_p3& P, const geu_p3& Q) {
  constexpr int EP = 5, EQ = 1;                // geu_joint_code(1, 0), (0, 1)
  tab.identity();                              // entry 0: (1, 1, 2, 0)
  tab(geu_joint_code(2, 0), geu_p3_to_cached(geu_p1p1_to_p3(geu_dbl_affine(P))));
  GEU_SCHED_FENCE();
  tab(geu_joint_code(0, 2), geu_p3_to_cached(geu_p1p1_to_p3(geu_dbl_affine(Q))));
  GEU_SCHED_FENCE();
  feu tt;
  {
    const geu_cached cq = geu_p3_to_cached(Q); // YpX, YmX 3 T, Z2 = 2, T2d tight
    tab(EQ, cq);
    tt = feu_mul(P.T, cq.T2d);                 // 2 T x T
    tab(EP, geu_p3_to_cached(P));
  }
#pragma unroll 1
  for (int b = 1; b >= -1; b -= 2) {
    const bool neg = b < 0;
    const int ka = neg ? 1 : 0, kb = neg ? 0 : 1;                                            // b Q: -Q swaps Y + X, Y - X
    const geu_p3 cur = geu_p1p1_to_p3(geu_add_affine(tab.load(EP, 0), tab.load(EP, 1), tab.load(EQ, ka),
                                                     tab.load(EQ, kb), tt, neg));           // P + b Q: all tight
    tab(geu_joint_code(1, b), geu_p3_to_cached(cur));
    GEU_SCHED_FENCE();
    // + b Q and + P: Niels additions of an affine point from its entry, (2 T, 3 T) x T and T x T
    tab(geu_joint_code(1, 2 * b), geu_p3_to_cached(geu_p1p1_to_p3(
        geu_add_niels(cur, tab.load(EQ, ka), tab.load(EQ, kb), tab.load(EQ, 3), neg))));
    GEU_SCHED_FENCE();
    tab(geu_joint_code(2, b), geu_p3_to_cached(geu_p1p1_to_p3(
        geu_add_niels(cur, tab.load(EP, 0), tab.load(EP, 1), tab.load(EP, 3), false))));
    GEU_SCHED_FENCE();
    geu_p2 c2; c2.X = cur.X; c2.Y = cur.Y; c2.Z = cur.Z;
    tab(geu_joint_code(2, 2 * b), geu_p3_to_cached(geu_p1p1_to_p3(geu_p2_dbl(c2))));
  }
}

// Signed radix-4 digits of x < 2^(2W-1) for a wave-uniform W in [66, 74], least significant first:
// digits 0..W-2 in [-2, 1] by recode16's carry rule (v = two bits + carry; carry = (v + 2) >> 2),
// digit W-1 in [0, 2] takes the last carry.  Adding 2 to every digit below W-1 in ONE 160-bit
// addition propagates exactly those carries: with y = x + sum_{i < W-1} 2 . 4^i, digit i is
// ((y >> 2i) & 3) - 2 and the top digit is y >> 2(W-1).  Returns the top digit (clamped to the
// table for lanes whose scalars are out of range: their verdict comes from the fallback).
FEU_FN int geu_recode4(const u32 x[5], int W, u32 y[5]) {
  const u32 sh = 2u * (u32)(W - 1) - 128u;     // 2 .. 18
  u64 c = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    c += (u64)x[i] + (i < 4 ? 0xAAAAAAAAu : (0xAAAAAAAAu & ((1u << sh) - 1u)));
    y[i] = (u32)c;
    c >>= 32;
  }
  const u32 top = y[4] >> sh;
  return (int)(top < 2u ? top : 2u);
}
// digit w (< W-1) from word w >> 4 of y
FEU_FN int geu_digit4(u32 word, int w) { return (int)((word >> (2 * (w & 15))) & 3u) - 2; }

// The ladder's first entry as a completed point (2X : 2Y : 2Z : 2Z): X 3 T, Y 2 T, Z = T tight.
// tab.load(e, k): coordinate k (0 Y+X, 1 Y-X, 2 2Z, 3 2dT) of entry e, tight.
template <class Tab>
FEU_FN geu_p1p1 geu_joint_first(const Tab& tab, int e) {
  const feu ypx = tab.load(e, 0), ymx = tab.load(e, 1);
  geu_p1p1 r;
  r.X = feu_sub<2>(ypx, ymx);
  r.Y = feu_add(ypx, ymx);
  r.Z = tab.load(e, 2);
  r.T = r.Z;
  return r;
}
// t + (neg ? -q : q) for q = tab[e]: the entry is read coordinate by coordinate, Y+X and Y-X (swapped
// for -q, a per-lane address choice) before the extended form is built, 2Z and 2dT after.
// t: X <= 4 T, Z <= 4 T, T and Y <= 3 T (the output of a doubling or of an addition).
template <class Tab>
FEU_FN geu_p1p1 geu_joint_add(const geu_p1p1& t, const Tab& tab, int e, bool neg) {
  const feu qa = tab.load(e, neg ? 1 : 0);     // tight
  const feu qb = tab.load(e, neg ? 0 : 1);     // tight
  const geu_p3 p = geu_p1p1_to_p3(t);          // all tight
  GEU_SCHED_FENCE();
  const feu qz = tab.load(e, 2);               // tight
  const feu qt = tab.load(e, 3);               // tight
  return geu_add_cached(p, qa, qb, qz, qt, neg);
}
// c P + d Q (+ what `base` adds) over W joint windows: per window ONE rolled doubling body run
// twice and ONE table addition, so the hot loop stays inside the instruction cache; the first
// window starts from its entry.  dg.c(w), dg.d(w): digit w of |c| and d; the top digits are >= 0.
// base.fetch(w) runs before window w's doublings, base.add(t, w) after its table addition.
template <class Tab, class Digits, class Base>
FEU_FN geu_p2 geu_joint_ladder(const Tab& tab, const Digits& dg, int top_c, int top_d, int W, Base& base) {
  geu_p1p1 t = geu_joint_first(tab, geu_joint_code(top_c, top_d));
#pragma unroll 1
  for (int w = W - 1; w >= 0; --w) {
    base.fetch(w);
    if (w != W - 1) {
#pragma unroll 1
      for (int k = 0; k < 2; ++k) t = geu_p2_dbl(geu_p1p1_to_p2(t));
      const int j = geu_joint_code(dg.c(w), dg.d(w));
      t = geu_joint_add(t, tab, j < 0 ? -j : j, j < 0);
    }
    base.add(t, w);
  }
  return geu_p1p1_to_p2(t);
}

// The carries of a packed table coordinate: any f <= 3 T to limbs in [0, 2^26) / [0, 2^25) (limb 1
// < 2^25 + 2), tight.
FEU_FN void feu_pack_carry(const feu& f, u32 h[10]) {
  u32 c = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int w = (i & 1) ? 25 : 26;
    const u32 v = f.v[i] + c;
    c = v >> w;
    h[i] = v & ((1u << w) - 1u);
  }
  h[0] += 19u * c;                     // c <= 3: h[0] < 2^26 + 57
  h[1] += h[0] >> 26;
  h[0] &= (1u << 26) - 1u;
}

}  // namespace nwc

#if defined(__HIPCC__)
#include "ge25519.h"
namespace nwc {

// ge_decompressN<1> (ge25519.h) on the non-negative field: the same dalek semantics, the same
// exponentiation chain.  out: X <= 2 T (r or 2p - r), Y, Z, T tight.
__device__ __forceinline__ feu feu_pow22523(const feu& z) {
  const feu z2 = feu_sq(z);
  const feu z9 = feu_mul(z, feu_sqn(z2, 2));
  const feu z11 = feu_mul(z2, z9);
  const feu t0 = feu_mul(z9, feu_sq(z11));            // 2^5 - 1
  const feu t1 = feu_mul(feu_sqn(t0, 5), t0);         // 2^10 - 1
  const feu t2 = feu_mul(feu_sqn(t1, 10), t1);        // 2^20 - 1
  const feu t3 = feu_mul(feu_sqn(t2, 20), t2);        // 2^40 - 1
  const feu t4 = feu_mul(feu_sqn(t3, 10), t1);        // 2^50 - 1
  const feu t5 = feu_mul(feu_sqn(t4, 50), t4);        // 2^100 - 1
  const feu t6 = feu_mul(feu_sqn(t5, 100), t5);       // 2^200 - 1
  const feu t7 = feu_mul(feu_sqn(t6, 50), t4);        // 2^250 - 1
  return feu_mul(feu_sqn(t7, 2), z);                  // 2^252 - 3; every operand tight
}
__device__ __forceinline__ void geu_decompress(const u32 w[8], geu_p3& out, u32 ycanon[8], bool& ok) {
  const feu one = feu_one();
  const feu y = feu_from_words(w);                            // tight
  const feu yy = feu_sq(y);
  const feu u = feu_sub<2>(yy, one);                          // 3 T
  const feu v = feu_add(feu_mul(yy, FEU_D), one);             // tight (+1 on limb 0: 2^26 <= T's slack)
  const feu v3 = feu_mul(feu_sq(v), v);
  const feu v7 = feu_mul(feu_sq(v3), v);
  const feu b = feu_pow22523(feu_mul(u, v7));                 // 3 T x T
  feu r = feu_mul(feu_mul(u, v3), b);                         // 3 T x T, T x T
  // v again (a square and a product) instead of ten registers held through the exponentiation
  const feu vv = feu_add(feu_mul(feu_sq(y), FEU_D), one);
  const feu check = feu_mul(vv, feu_sq(r));
  const bool correct = feu_is_zero(feu_sub<4>(check, u));     // T + 4p - 3 T: 5 T
  const bool flipped = feu_is_zero(feu_add(check, u));        // 4 T
  // dalek also multiplies r by sqrt(-1) when check == -u sqrt(-1); that case only ever picks a root
  // for an encoding that does not decode (ok is false either way), so its product and zero test
  // are left out: the verdict never reads such a point, and its classes below do not change
  r = feu_select(r, feu_mul(r, FEU_SQRTM1), flipped);
  const bool sign = (w[7] >> 31) & 1;
  // dalek: r := |r| (the non-negative root), then x := -r if the sign bit is set, even when r == 0
  out.X = feu_select(r, feu_neg<2>(r), feu_is_negative(r) != sign);   // 2 T
  out.Y = y;
  out.Z = one;
  out.T = feu_mul(out.X, y);                                  // 2 T x T
  fe_to_words(feu_as_fe(y), ycanon);
  ok = correct || flipped;
}

}  // namespace nwc
#endif
