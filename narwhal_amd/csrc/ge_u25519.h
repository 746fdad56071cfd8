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
  const bool flipped_i = feu_is_zero(feu_add(check, feu_mul(u, FEU_SQRTM1)));   // 3 T x T; 2 T
  r = feu_select(r, feu_mul(r, FEU_SQRTM1), flipped || flipped_i);
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
