// How should the 100 v_mad_u64_u32 of a 10 x 25.5-bit field product be laid out when every
// column's chain is seeded with the previous column's carry (fe_u25519.h)?  Cycles per product
// on one SIMD at 1 and 2 waves per SIMD, nominal 2.4 GHz:
//   a   ten independent chains issued round-robin, no carry at all (the multiply-add floor)
//   a2  the same + today's separate 12-step signed carry (fe25519.h: fe_carry_wide)
//   b   one fully dependent chain of 100; a 64-bit shift and a mask after every tenth
//   c   two dependent half-chains (columns 0-4 and 5-9), joined as fe_carry_wide joins them
//   d   two products' serial chains interleaved instruction by instruction (per product)
// Every product's limbs feed the next product's operands, as in a squaring chain.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
constexpr int ITERS = 4096;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;

#define MAD(acc, a, b) "v_mad_u64_u32 " acc ", vcc, " a ", " b ", " acc "\n\t"
// ten multiply-adds into one accumulator (%0), operands %1..%10 against %11
#define CHAIN10 MAD("%0", "%1", "%11") MAD("%0", "%2", "%11") MAD("%0", "%3", "%11") MAD("%0", "%4", "%11") MAD("%0", "%5", "%11") \
                MAD("%0", "%6", "%11") MAD("%0", "%7", "%11") MAD("%0", "%8", "%11") MAD("%0", "%9", "%11") MAD("%0", "%10", "%11")
#define F10(f) "v"(f[0]), "v"(f[1]), "v"(f[2]), "v"(f[3]), "v"(f[4]), "v"(f[5]), "v"(f[6]), "v"(f[7]), "v"(f[8]), "v"(f[9])

__device__ __forceinline__ void init(u32 f[10], u32 g[10], u32 seed) {
  _Pragma("unroll") for (int i = 0; i < 10; ++i) {
    f[i] = (seed * 2654435761u + threadIdx.x * 40503u + i * 7919u) & 0x3ffffffu;
    g[i] = (seed * 40503u + blockIdx.x * 9973u + i * 104729u) & 0x3ffffffu;
  }
}
__device__ __forceinline__ void fin(u32* out, const u32 f[10]) {
  u32 r = 0; _Pragma("unroll") for (int i = 0; i < 10; ++i) r ^= f[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

// ten independent chains, round-robin: round r adds f[(k + r) % 10] * g[r] to column k
__device__ __forceinline__ void indep100(const u32 f[10], const u32 g[10], u64 h[10]) {
  _Pragma("unroll") for (int k = 0; k < 10; ++k) h[k] = 0;
  _Pragma("unroll") for (int r = 0; r < 10; ++r) {
    asm volatile(MAD("%0", "%10", "%20") MAD("%1", "%11", "%20") MAD("%2", "%12", "%20") MAD("%3", "%13", "%20") MAD("%4", "%14", "%20")
                 MAD("%5", "%15", "%20") MAD("%6", "%16", "%20") MAD("%7", "%17", "%20") MAD("%8", "%18", "%20") MAD("%9", "%19", "%20")
                 : "+v"(h[0]), "+v"(h[1]), "+v"(h[2]), "+v"(h[3]), "+v"(h[4]), "+v"(h[5]), "+v"(h[6]), "+v"(h[7]), "+v"(h[8]), "+v"(h[9])
                 : F10(f), "v"(g[r]) : "vcc");
  }
}

__global__ void k_a(u32* out, u32 seed) {
  u32 f[10], g[10]; init(f, g, seed);
  for (int it = 0; it < ITERS; ++it) {
    u64 h[10]; indep100(f, g, h);
    _Pragma("unroll") for (int k = 0; k < 10; ++k) f[k] = (u32)h[k];   // free: the low register
  }
  fin(out, f);
}

__global__ void k_a2(u32* out, u32 seed) {
  u32 f[10], g[10]; init(f, g, seed);
  for (int it = 0; it < ITERS; ++it) {
    u64 hu[10]; indep100(f, g, hu);
    i64 h[10]; _Pragma("unroll") for (int k = 0; k < 10; ++k) h[k] = (i64)hu[k];
    i64 c; u32 r[10];
#define FL(i, sh) { c = h[i] >> sh; r[i] = (u32)h[i] & ((1u << sh) - 1u); }
    FL(0, 26); h[1] += c; FL(4, 26); h[5] += c; FL(1, 25); h[2] += c; FL(5, 25); h[6] += c;
    FL(2, 26); h[3] += c; FL(6, 26); h[7] += c; FL(3, 25); h[4] = (i64)r[4] + c; FL(7, 25); h[8] += c;
    FL(4, 26); r[5] += (u32)c; FL(8, 26); h[9] += c; FL(9, 25); h[0] = (i64)r[0] + c * 19; FL(0, 26); r[1] += (u32)c;
#undef FL
    _Pragma("unroll") for (int k = 0; k < 10; ++k) f[k] = r[k] - ((k & 1) ? (1u << 24) : (1u << 25));
  }
  fin(out, f);
}

// one serial chain: column k starts from the carry of column k - 1
__device__ __forceinline__ void serial100(const u32 f[10], const u32 g[10], u32 r[10]) {
  u64 h = 0;
  _Pragma("unroll") for (int k = 0; k < 10; ++k) {
    asm volatile(CHAIN10 : "+v"(h) : F10(f), "v"(g[k]) : "vcc");
    const int sh = (k & 1) ? 25 : 26;
    r[k] = (u32)h & ((1u << sh) - 1u);
    h >>= sh;
  }
  const u64 t = (u64)r[0] + 19u * h;
  r[0] = (u32)t & 0x3ffffffu;
  r[1] += (u32)(t >> 26);
}

__global__ void k_b(u32* out, u32 seed) {
  u32 f[10], g[10]; init(f, g, seed);
  for (int it = 0; it < ITERS; ++it) {
    u32 r[10]; serial100(f, g, r);
    _Pragma("unroll") for (int k = 0; k < 10; ++k) f[k] = r[k];
  }
  fin(out, f);
}

// two chains of five columns each, interleaved instruction by instruction: %0 / %1 accumulators
#define CHAIN10X2 MAD("%0", "%2", "%12") MAD("%1", "%2", "%13") MAD("%0", "%3", "%12") MAD("%1", "%3", "%13") MAD("%0", "%4", "%12") MAD("%1", "%4", "%13") \
                  MAD("%0", "%5", "%12") MAD("%1", "%5", "%13") MAD("%0", "%6", "%12") MAD("%1", "%6", "%13") MAD("%0", "%7", "%12") MAD("%1", "%7", "%13") \
                  MAD("%0", "%8", "%12") MAD("%1", "%8", "%13") MAD("%0", "%9", "%12") MAD("%1", "%9", "%13") MAD("%0", "%10", "%12") MAD("%1", "%10", "%13") \
                  MAD("%0", "%11", "%12") MAD("%1", "%11", "%13")
__global__ void k_c(u32* out, u32 seed) {
  u32 f[10], g[10]; init(f, g, seed);
  for (int it = 0; it < ITERS; ++it) {
    u32 r[10];
    u64 ha = 0, hb = 0;
    _Pragma("unroll") for (int k = 0; k < 5; ++k) {
      asm volatile(CHAIN10X2 : "+v"(ha), "+v"(hb) : F10(f), "v"(g[k]), "v"(g[k + 5]) : "vcc");
      const int sa = (k & 1) ? 25 : 26, sb = (k & 1) ? 26 : 25;
      r[k] = (u32)ha & ((1u << sa) - 1u); ha >>= sa;
      r[k + 5] = (u32)hb & ((1u << sb) - 1u); hb >>= sb;
    }
    // joins: the low half's carry enters limb 5, the high half's (x 19) limb 0; one more step each
    const u64 t5 = (u64)r[5] + ha, t0 = (u64)r[0] + 19u * hb;
    r[5] = (u32)t5 & 0x1ffffffu; r[6] += (u32)(t5 >> 25);
    r[0] = (u32)t0 & 0x3ffffffu; r[1] += (u32)(t0 >> 26);
    _Pragma("unroll") for (int k = 0; k < 10; ++k) f[k] = r[k];
  }
  fin(out, f);
}

// two independent products, their serial chains interleaved (two products per iteration)
__global__ void k_d(u32* out, u32 seed) {
  u32 f[10], g[10]; init(f, g, seed);
  for (int it = 0; it < ITERS; ++it) {
    u32 r[10], q[10];
    u64 ha = 0, hb = 0;
    _Pragma("unroll") for (int k = 0; k < 10; ++k) {
      asm volatile(CHAIN10X2 : "+v"(ha), "+v"(hb) : F10(f), "v"(g[k]), "v"(g[9 - k]) : "vcc");
      const int sh = (k & 1) ? 25 : 26;
      r[k] = (u32)ha & ((1u << sh) - 1u); ha >>= sh;
      q[k] = (u32)hb & ((1u << sh) - 1u); hb >>= sh;
    }
    const u64 t = (u64)r[0] + 19u * ha, s = (u64)q[0] + 19u * hb;
    r[0] = (u32)t & 0x3ffffffu; r[1] += (u32)(t >> 26);
    q[0] = (u32)s & 0x3ffffffu; q[1] += (u32)(s >> 26);
    _Pragma("unroll") for (int k = 0; k < 10; ++k) { f[k] = r[k]; g[k] = q[k]; }
  }
  fin(out, f);
}

typedef void (*kfn)(u32*, u32);
struct K { const char* name; kfn f; int products; };

int main() {
  hipDeviceProp_t p; CHECK(hipGetDeviceProperties(&p, 0));
  const int cus = p.multiProcessorCount;
  printf("device %s CUs=%d; cycles at a nominal 2.4 GHz, one 100-multiply-add product per lane\n", p.gcnArchName, cus);
  K ks[] = {{"a  10 independent chains, no carry", k_a, 1}, {"a2 10 independent chains + 12-step carry", k_a2, 1},
            {"b  one serial chain, carry-seeded", k_b, 1}, {"c  two half-chains, joined", k_c, 1},
            {"d  two products' chains interleaved", k_d, 2}};
  u32* out;
  for (int wpc : {4, 8}) {
    const int threads = 64 * wpc, blocks = cus;
    CHECK(hipMalloc(&out, (size_t)blocks * threads * 4));
    hipEvent_t a, b; CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
    for (auto& k : ks) {
      hipLaunchKernelGGL(k.f, dim3(blocks), dim3(threads), 0, 0, out, 1u);
      CHECK(hipDeviceSynchronize());
      CHECK(hipEventRecord(a));
      const int REP = 5;
      for (int r = 0; r < REP; ++r) hipLaunchKernelGGL(k.f, dim3(blocks), dim3(threads), 0, 0, out, (u32)r + 2u);
      CHECK(hipEventRecord(b)); CHECK(hipEventSynchronize(b));
      float ms; CHECK(hipEventElapsedTime(&ms, a, b));
      const double products_per_simd = (double)REP * (wpc / 4) * ITERS * k.products;
      const double cyc = ms * 1e-3 * 2.4e9 / products_per_simd;
      printf("waves/SIMD=%d %-44s %8.1f cycles per product  %6.2f per multiply-add\n", wpc / 4, k.name, cyc, cyc / 100.0);
    }
    CHECK(hipFree(out));
  }
  return 0;
}
