// Host driver of the non-negative field (narwhal_amd/csrc/fe_u25519.h, ge_u25519.h) for
// tests/test_feu_host.py.  Stand-alone: built with the address and undefined-behaviour sanitizers
// linked in, run as a child process.
//   feu_host field IN OUT    IN: records of 20 u32 (a, b).  OUT per record 11 x 10 u32:
//                            mul(a,b) sq(b) sq2(b) add(a,b) sub<2> sub<3> sub<4>(a,b) weak(a)
//                            from_signed<1>(s) from_signed<2>(s) to_signed(a), s_i = b_i - 2^(w_i - 1)
//   feu_host bounds          stdin: "mul a0..a9 b0..b9" | "sq f0..f9" | "sq2 f0..f9" per line; the product
//                            is evaluated with 64-bit operands and 128-bit columns.  stdout per line:
//                            <largest prepared operand> <largest column, hi lo> r0..r9
//   feu_host group IN OUT    IN: records of 81 u32: P (X Y Z T), Q (X Y Z T, Z = 1), neg.
//                            OUT per record 5 x 40 u32, each an extended point: 2P; P + (neg ? -Q : Q)
//                            with Q's cached entry as built, with it carried tight (a packed entry),
//                            with Q as an affine Niels entry; and 2P of the negated P.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ge_u25519.h"

using nwc::feu;
using nwc::u32;
using nwc::u64;

namespace shadow {
using nwc::feu;
using nwc::u32;
typedef unsigned __int128 u128;
static u64 op_max;
static u128 col_max;
static inline u64 prep(u64 v) { if (v > op_max) op_max = v; return v; }
static inline void col_end(u128 h) { if (h > col_max) col_max = h; }
#define FEU_OP u64
#define FEU_PREP(k, x) shadow::prep((u64)(k) * (u64)(x))
#define FEU_ACC shadow::u128
#define FEU_MA(h, a, b) h += (shadow::u128)(a) * (b)
#define FEU_COL_END(h) shadow::col_end(h)
#include "feu_asm.h"
}  // namespace shadow

static std::vector<u32> read_all(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<u32> v((size_t)n / 4);
  if (n && fread(v.data(), 4, v.size(), f) != v.size()) { perror("read"); exit(2); }
  fclose(f);
  return v;
}
static void write_all(const char* path, const std::vector<u32>& v) {
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); exit(2); }
  if (!v.empty() && fwrite(v.data(), 4, v.size(), f) != v.size()) { perror("write"); exit(2); }
  fclose(f);
}
static feu load(const u32* p) { feu r; memcpy(r.v, p, 40); return r; }
static void put(std::vector<u32>& out, const feu& f) { out.insert(out.end(), f.v, f.v + 10); }
static void put(std::vector<u32>& out, const nwc::geu_p3& p) { put(out, p.X); put(out, p.Y); put(out, p.Z); put(out, p.T); }

static int run_field(const char* in, const char* outp) {
  const std::vector<u32> v = read_all(in);
  std::vector<u32> out;
  out.reserve(v.size() / 20 * 110);
  for (size_t i = 0; i + 20 <= v.size(); i += 20) {
    const feu a = load(&v[i]), b = load(&v[i + 10]);
    put(out, nwc::feu_mul(a, b));
    put(out, nwc::feu_sq(b));
    put(out, nwc::feu_sq2(b));
    put(out, nwc::feu_add(a, b));
    put(out, nwc::feu_sub<2>(a, b));
    put(out, nwc::feu_sub<3>(a, b));
    put(out, nwc::feu_sub<4>(a, b));
    put(out, nwc::feu_weak(a));
    int32_t s[10], t[10];
    for (int k = 0; k < 10; ++k) s[k] = (int32_t)(b.v[k] & 0x7fffffffu) - (1 << ((k & 1) ? 24 : 25));
    put(out, nwc::feu_from_signed<1>(s));
    put(out, nwc::feu_from_signed<2>(s));
    nwc::feu_to_signed(a, t);
    feu ts; for (int k = 0; k < 10; ++k) ts.v[k] = (u32)t[k];
    put(out, ts);
  }
  write_all(outp, out);
  return 0;
}

static int run_bounds() {
  char op[8];
  while (scanf("%7s", op) == 1) {
    feu a = nwc::feu_zero(), b = nwc::feu_zero();
    const bool mul = !strcmp(op, "mul");
    if (mul) for (int k = 0; k < 10; ++k) if (scanf("%u", &a.v[k]) != 1) return 2;
    for (int k = 0; k < 10; ++k) if (scanf("%u", &b.v[k]) != 1) return 2;
    shadow::op_max = 0;
    shadow::col_max = 0;
    feu r;
    if (mul) r = shadow::feu_mul(a, b);
    else if (!strcmp(op, "sq")) r = shadow::feu_sq(b);
    else if (!strcmp(op, "sq2")) r = shadow::feu_sq2(b);
    else return 2;
    printf("%llu %llu %llu", (unsigned long long)shadow::op_max, (unsigned long long)(shadow::col_max >> 64),
           (unsigned long long)(u64)shadow::col_max);
    for (int k = 0; k < 10; ++k) printf(" %u", r.v[k]);
    printf("\n");
  }
  return 0;
}

static nwc::geu_p3 load_p3(const u32* p) { nwc::geu_p3 r; r.X = load(p); r.Y = load(p + 10); r.Z = load(p + 20); r.T = load(p + 30); return r; }
static nwc::geu_p3 dbl(const nwc::geu_p3& P) {
  nwc::geu_p2 p2; p2.X = P.X; p2.Y = P.Y; p2.Z = P.Z;
  return nwc::geu_p1p1_to_p3(nwc::geu_p2_dbl(p2));
}

static int run_group(const char* in, const char* outp) {
  const std::vector<u32> v = read_all(in);
  std::vector<u32> out;
  for (size_t i = 0; i + 81 <= v.size(); i += 81) {
    const nwc::geu_p3 P = load_p3(&v[i]), Q = load_p3(&v[i + 40]);
    const bool neg = v[i + 80] != 0;
    put(out, dbl(P));
    const nwc::geu_cached c = nwc::geu_p3_to_cached(Q);
    const feu& qa = neg ? c.YmX : c.YpX;
    const feu& qb = neg ? c.YpX : c.YmX;
    // the additions take an extended point with tight coordinates: P through one doubling's products
    nwc::geu_p3 Pt = P;
    Pt.X = nwc::feu_weak(P.X);
    Pt.T = nwc::feu_weak(P.T);
    put(out, nwc::geu_p1p1_to_p3(nwc::geu_add_cached(Pt, qa, qb, c.Z2, c.T2d, neg)));
    put(out, nwc::geu_p1p1_to_p3(nwc::geu_add_cached(Pt, nwc::feu_weak(qa), nwc::feu_weak(qb), nwc::feu_weak(c.Z2),
                                                     nwc::feu_weak(c.T2d), neg)));
    put(out, nwc::geu_p1p1_to_p3(nwc::geu_add_niels(Pt, qa, qb, c.T2d, neg)));
    put(out, dbl(nwc::geu_p3_neg(P, true)));
  }
  write_all(outp, out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "field")) return run_field(argv[2], argv[3]);
  if (argc == 2 && !strcmp(argv[1], "bounds")) return run_bounds();
  if (argc == 4 && !strcmp(argv[1], "group")) return run_group(argv[2], argv[3]);
  fprintf(stderr, "usage: feu_host field IN OUT | bounds | group IN OUT\n");
  return 2;
}
