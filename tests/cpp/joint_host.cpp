// Host driver of the joint radix-4 table, its recoding and its ladder (narwhal_amd/csrc/ge_u25519.h)
// for tests/test_joint_table_host.py.  Stand-alone: built with the address and undefined-behaviour
// sanitizers linked in, run as a child process.
//   joint_host recode        stdin: "W c0..c4 d0..d4" per line (32-bit words of |c| and d).  stdout per line:
//                            W digits of c (least significant first, the top digit last), W digits of d,
//                            W joint codes.
//   joint_host build IN OUT  IN: records of 80 u32: P (X Y Z T), Q (X Y Z T), both with Z = 1.
//                            OUT per record 13 x 40 u32 (the entries as the kernel packs them: Y+X, Y-X,
//                            2Z, 2dT after the pack's carries) and one word: 1 if a coordinate handed to
//                            the store exceeded 3 T (the pack's contract).
//   joint_host ladder IN OUT IN: records of 91 u32: P, Q, c (5 words), d (5 words), W.
//                            OUT per record 30 u32: (X : Y : Z) of c P + d Q over W joint windows.
//   joint_host bounds        as feu_host bounds.
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
static nwc::geu_p3 load_p3(const u32* p) { nwc::geu_p3 r; r.X = load(p); r.Y = load(p + 10); r.Z = load(p + 20); r.T = load(p + 30); return r; }

// The lane table as the kernel keeps it: every coordinate through the pack's carries.
struct HostTable {
  feu (*e)[4];
  bool* loose;
  void operator()(int i, const nwc::geu_cached& c) const {
    if (i < 0 || i >= nwc::JOINT_ENTRIES) { fprintf(stderr, "entry %d out of range\n", i); exit(3); }
    const feu* co = &c.YpX;
    for (int k = 0; k < 4; ++k) {
      for (int l = 0; l < 10; ++l) {
        const u64 tight = l == 1 ? (1u << 25) - 1u + (1u << 18) : ((l & 1) ? (1u << 25) : (1u << 26)) - 1u + (1u << 11);
        if (co[k].v[l] > 3 * tight) *loose = true;
      }
      nwc::feu_pack_carry(co[k], e[i][k].v);
    }
  }
  void identity() const {
    e[0][0] = nwc::feu_one(); e[0][1] = nwc::feu_one(); e[0][2] = nwc::feu_two(); e[0][3] = nwc::feu_zero();
  }
  feu load(int i, int k) const {
    if (i < 0 || i >= nwc::JOINT_ENTRIES || k < 0 || k > 3) { fprintf(stderr, "load %d %d out of range\n", i, k); exit(3); }
    return e[i][k];
  }
};

struct HostDigits {
  u32 yc[5], yd[5];
  int c(int w) const { return nwc::geu_digit4(yc[w >> 4], w); }
  int d(int w) const { return nwc::geu_digit4(yd[w >> 4], w); }
};
struct NoBase {
  void fetch(int) {}
  void add(nwc::geu_p1p1&, int) {}
};

static int run_recode() {
  int W;
  while (scanf("%d", &W) == 1) {
    if (W < nwc::JOINT_WINDOWS_MIN || W > nwc::JOINT_WINDOWS_MAX) return 2;
    u32 c[5], d[5];
    for (int k = 0; k < 5; ++k) if (scanf("%u", &c[k]) != 1) return 2;
    for (int k = 0; k < 5; ++k) if (scanf("%u", &d[k]) != 1) return 2;
    HostDigits dg;
    const int tc = nwc::geu_recode4(c, W, dg.yc), td = nwc::geu_recode4(d, W, dg.yd);
    for (int w = 0; w < W; ++w) printf("%d ", w == W - 1 ? tc : dg.c(w));
    for (int w = 0; w < W; ++w) printf("%d ", w == W - 1 ? td : dg.d(w));
    for (int w = 0; w < W; ++w)
      printf("%d ", w == W - 1 ? nwc::geu_joint_code(tc, td) : nwc::geu_joint_code(dg.c(w), dg.d(w)));
    printf("\n");
  }
  return 0;
}

static int run_build(const char* in, const char* outp) {
  const std::vector<u32> v = read_all(in);
  std::vector<u32> out;
  for (size_t i = 0; i + 80 <= v.size(); i += 80) {
    feu e[nwc::JOINT_ENTRIES][4];
    memset(e, 0xff, sizeof e);
    bool loose = false;
    nwc::geu_build_joint(HostTable{e, &loose}, load_p3(&v[i]), load_p3(&v[i + 40]));
    for (int j = 0; j < nwc::JOINT_ENTRIES; ++j)
      for (int k = 0; k < 4; ++k) out.insert(out.end(), e[j][k].v, e[j][k].v + 10);
    out.push_back(loose ? 1u : 0u);
  }
  write_all(outp, out);
  return 0;
}

static int run_ladder(const char* in, const char* outp) {
  const std::vector<u32> v = read_all(in);
  std::vector<u32> out;
  for (size_t i = 0; i + 91 <= v.size(); i += 91) {
    feu e[nwc::JOINT_ENTRIES][4];
    bool loose = false;
    const HostTable tab{e, &loose};
    nwc::geu_build_joint(tab, load_p3(&v[i]), load_p3(&v[i + 40]));
    const int W = (int)v[i + 90];
    if (W < nwc::JOINT_WINDOWS_MIN || W > nwc::JOINT_WINDOWS_MAX) return 2;
    HostDigits dg;
    const int tc = nwc::geu_recode4(&v[i + 80], W, dg.yc), td = nwc::geu_recode4(&v[i + 85], W, dg.yd);
    NoBase base;
    const nwc::geu_p2 q = nwc::geu_joint_ladder(tab, dg, tc, td, W, base);
    out.insert(out.end(), q.X.v, q.X.v + 10);
    out.insert(out.end(), q.Y.v, q.Y.v + 10);
    out.insert(out.end(), q.Z.v, q.Z.v + 10);
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
    else return 2;
    printf("%llu %llu %llu", (unsigned long long)shadow::op_max, (unsigned long long)(shadow::col_max >> 64),
           (unsigned long long)(u64)shadow::col_max);
    for (int k = 0; k < 10; ++k) printf(" %u", r.v[k]);
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "recode")) return run_recode();
  if (argc == 4 && !strcmp(argv[1], "build")) return run_build(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "ladder")) return run_ladder(argv[2], argv[3]);
  if (argc == 2 && !strcmp(argv[1], "bounds")) return run_bounds();
  fprintf(stderr, "usage: joint_host recode | build IN OUT | ladder IN OUT | bounds\n");
  return 2;
}
