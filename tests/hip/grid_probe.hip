// Third probe library, for tests/test_gpu_torsion_grid.py (tests/grid_probe.py builds and wraps it):
// the primitives of dalek's equation per certificate, each alone -- torsion_dlog, ge_mul_l and
// resolve_q8 (resolve.h), straus_z and sc_mul128 (straus.h).  Those headers lean on functions of
// kernels.hip, so this translation unit includes kernels.hip whole, as tests/hip/half_probe.hip does,
// and follows its conventions: compiled with the library's flags, never linked into it, kept out of
// narwhal_amd/csrc so the library's build id does not depend on it, and it launches only the kernels
// named k_gp_* below.
//
// Entries:  int probe_X(const u32* in, u32* out, u32 n, hipStream_t stream): n records of IN words, n
// records of OUT words, one lane per record, 256-thread blocks.  The lanes of a ragged last wave stay
// in the kernel on record 0 and store nothing.
#include "kernels.hip"

#ifndef NWC_PROBE_ID
#define NWC_PROBE_ID "unset"
#endif
#define GP_EXPORT extern "C" __attribute__((visibility("default")))

using namespace nwc;

namespace {

constexpr int BLOCK = 256;

// this lane's record: its own, or record 0 for an idle lane of the last wave
__device__ __forceinline__ u32 record_of(u32 n, bool& live) {
  const u32 t = blockIdx.x * BLOCK + threadIdx.x;
  live = t < n;
  return live ? t : 0u;
}

// in: X[10], Y[10], Z[10] signed limbs of a projective point (within the loose bound).  out: torsion_dlog
constexpr int IN_TDLOG = 30, OUT_TDLOG = 1;
__global__ void k_gp_torsion_dlog(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  bool live;
  const u32 t = record_of(n, live);
  const u32* r = in + (size_t)t * IN_TDLOG;
  ge_p2 P;
  _Pragma("unroll") for (int i = 0; i < 10; ++i) { P.X.v[i] = (i32)r[i]; P.Y.v[i] = (i32)r[10 + i]; P.Z.v[i] = (i32)r[20 + i]; }
  const u32 j = torsion_dlog(P);
  if (!live) return;
  out[(size_t)t * OUT_TDLOG] = j;
}

// in: an encoded point (8 words).  out: torsion_dlog(ge_mul_l(P)), whether the encoding decodes
constexpr int IN_MULL = 8, OUT_MULL = 2;
__global__ void k_gp_mul_l(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  bool live;
  const u32 t = record_of(n, live);
  u32 w[8], yc[8];
  _Pragma("unroll") for (int i = 0; i < 8; ++i) w[i] = in[(size_t)t * IN_MULL + i];
  ge_p3 P;
  bool ok;
  ge_decompress1(w, P, yc, ok);
  const u32 j = torsion_dlog(ge_mul_l(P));
  if (!live) return;
  out[(size_t)t * OUT_MULL] = j;
  out[(size_t)t * OUT_MULL + 1] = ok ? 1u : 0u;
}

// out of both entries below: z[4], z k mod l[8] (sc_mul128), q8 (resolve_q8), as k_vote_resolve chains them
constexpr int OUT_ZQ = 13;
__device__ __forceinline__ void store_zq(u32* o, const u32 z[4], const u32 k[8]) {
  u32 zk[8];
  sc_mul128(z, k, zk);
  _Pragma("unroll") for (int i = 0; i < 4; ++i) o[i] = z[i];
  _Pragma("unroll") for (int i = 0; i < 8; ++i) o[4 + i] = zk[i];
  o[12] = resolve_q8(z, k, zk);
}
// in: seed[8], v (low word, high word), k[8]: z = straus_z(seed, v)
constexpr int IN_ZQ = 18;
__global__ void k_gp_zq(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  bool live;
  const u32 t = record_of(n, live);
  const u32* r = in + (size_t)t * IN_ZQ;
  u32 seed[8], k[8], z[4];
  _Pragma("unroll") for (int i = 0; i < 8; ++i) { seed[i] = r[i]; k[i] = r[10 + i]; }
  straus_z(seed, ((uint64_t)r[9] << 32) | r[8], z);
  if (!live) return;
  store_zq(out + (size_t)t * OUT_ZQ, z, k);
}
// in: z[4], k[8]: the same with z given (z = 0, z = 2^128 - 1)
constexpr int IN_ZQ_DIRECT = 12;
__global__ void k_gp_zq_direct(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  bool live;
  const u32 t = record_of(n, live);
  const u32* r = in + (size_t)t * IN_ZQ_DIRECT;
  u32 k[8], z[4];
  _Pragma("unroll") for (int i = 0; i < 4; ++i) z[i] = r[i];
  _Pragma("unroll") for (int i = 0; i < 8; ++i) k[i] = r[4 + i];
  if (!live) return;
  store_zq(out + (size_t)t * OUT_ZQ, z, k);
}

template <class K>
int launch(K kernel, const u32* in, u32* out, u32 n, hipStream_t stream) {
  if (n == 0) return (int)hipSuccess;
  if (!in || !out) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, in, out, n);
  return (int)hipGetLastError();
}

}  // namespace

#define GRID_PROBE(name, kernel)                                                       \
  GP_EXPORT int name(const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t stream) { \
    return launch(kernel, in, out, n, stream);                                         \
  }

GRID_PROBE(probe_torsion_dlog, k_gp_torsion_dlog)
GRID_PROBE(probe_mul_l, k_gp_mul_l)
GRID_PROBE(probe_zq, k_gp_zq)
GRID_PROBE(probe_zq_direct, k_gp_zq_direct)

// words per record (in, out) of an entry, so the wrapper's table is checked against this file
GP_EXPORT int probe_record_words(const char* name, int* in_words, int* out_words) {
  struct { const char* n; int i, o; } const t[] = {
      {"probe_torsion_dlog", IN_TDLOG, OUT_TDLOG},    {"probe_mul_l", IN_MULL, OUT_MULL},
      {"probe_zq", IN_ZQ, OUT_ZQ},                    {"probe_zq_direct", IN_ZQ_DIRECT, OUT_ZQ},
  };
  for (const auto& e : t) {
    const char *a = e.n, *b = name;
    while (*a && *a == *b) { ++a; ++b; }
    if (*a == 0 && *b == 0) { *in_words = e.i; *out_words = e.o; return 0; }
  }
  return -1;
}

GP_EXPORT const char* probe_build_id() {
  static const char id[] = "NWC_GRID_PROBE_ID:" NWC_PROBE_ID;
  return id + 18;
}
