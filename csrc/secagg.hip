// Pairwise-masked secure aggregation (gfx950): the kernels of ops.fl.secagg_mask_rows / ring_sum / ring_unmask
// (worker/secagg_worker.py, algorithm/secagg_algorithm.py, oracle ops/ref.py). Everything is integer
// arithmetic in Z_{2^32}: exact, independent of order and launch geometry, so kernel and oracle agree bit
// for bit and no contraction flag matters (the one fp64 product, t · 2^f, is exact).
//
// w(κ, p)          word p % 4 of Philox4x32-10 with key (κ lo, κ hi) and counter (i lo, i hi, 0, 0x53413031),
//                  i = p / 4: one call gives the four mask words of a lane's four consecutive elements.
// secagg_mask_rows out[k][p] = low 32 bits of q(x[k][p]) + Σ_e sign_e · w(κ_e, p) over the entries [off[k],
//                  off[k + 1]) of row k; q(x) = rint(double(clamp(x, −R, R)) · 2^f), NaN → 0; stats[k] = (number
//                  of elements with |x| > R, number of NaNs). blockIdx.y is the row, so the entry list is
//                  uniform across the workgroup and is read through a uniform index (scalar loads). A lane
//                  owns G groups of four consecutive elements (one float4 load, one int4 store each), a
//                  stride apart, and expands U entries per loop trip: G · U independent Philox chains.
//                  Grid-stride loop under a block cap. A trip's loads come before its stores and no lane
//                  reads another lane's elements, so out == x is safe. The counters are reduced over the
//                  wave and added with one integer atomic per wave and counter (exact: still deterministic).
// ring_sum         acc[p] (int64) += Σ_k (int64) rows[k][p]; the clipped_sum_kernel shape (int4 loads, rows
//                  innermost, two longlong2 accumulators per lane).
// ring_unmask      acc[p] (int64) −= Σ_e sign_e · (int64) w(κ_e, p) over one flat entry list: the same
//                  expander, no fp32 input.
#include "common.h"
#include "dls.h"
#include "philox.h"

namespace {

constexpr int SA_TPB = 256;
constexpr int MASK_MAX_BLOCKS = 1024;  // per row (grid.x); grid.y = rows
constexpr int RING_MAX_BLOCKS = 8192;
constexpr uint32_t SA_TAG = 0x53413031u;  // "SA01", fourth counter word of the mask streams

typedef unsigned long long u64;

// the four words of entry (key, sm) at call index i added to s; sm = 0 (sign +1) or 0xffffffff (sign −1):
// (w ^ sm) − sm is w or −w in Z_{2^32}
__device__ inline void expand_add(long i, u64 key, uint32_t sm, uint32_t s[4]) {
  uint32_t w[4];
  philox4x32_10((uint32_t)((u64)i & 0xffffffffu), (uint32_t)((u64)i >> 32), 0u, SA_TAG, (uint32_t)(key & 0xffffffffull),
                (uint32_t)(key >> 32), w);
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] += (w[j] ^ sm) - sm;
}

__device__ inline uint32_t quantise(float x, float R, double scale, int& clamped, int& nans) {
  if (x != x) {
    ++nans;
    return 0u;
  }
  clamped += fabsf(x) > R ? 1 : 0;
  const float t = fminf(fmaxf(x, -R), R);
  return (uint32_t)(int)rint((double)t * scale);  // |t · 2^f| ≤ 2^31 − 1 (checked by the caller)
}

__device__ inline int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

template <int G, int U>
__global__ void __launch_bounds__(SA_TPB) secagg_mask_rows_kernel(const float* x, long ldx, int* out, long ldo, long P4,
                                                                  const int* __restrict__ off,
                                                                  const u64* __restrict__ keys,
                                                                  const int* __restrict__ signs, float R, double scale,
                                                                  int* __restrict__ stats) {
  const int row = blockIdx.y;
  const float* xr = x + (long)row * ldx;
  int* orow = out + (long)row * ldo;
  const int e0 = off[row], e1 = off[row + 1];
  const long stride = (long)gridDim.x * blockDim.x;
  int clamped = 0, nans = 0;
  for (long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x; i0 < P4; i0 += G * stride) {
    float4 v[G];
    uint32_t s[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const long i = i0 + g * stride;
      v[g] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < P4) v[g] = reinterpret_cast<const float4*>(xr)[i];
      s[g][0] = s[g][1] = s[g][2] = s[g][3] = 0u;
    }
    int e = e0;
    for (; e + U <= e1; e += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const u64 key = keys[e + u];
        const uint32_t sm = signs[e + u] < 0 ? 0xffffffffu : 0u;
#pragma unroll
        for (int g = 0; g < G; ++g) expand_add(i0 + g * stride, key, sm, s[g]);
      }
    }
    for (; e < e1; ++e) {
      const u64 key = keys[e];
      const uint32_t sm = signs[e] < 0 ? 0xffffffffu : 0u;
#pragma unroll
      for (int g = 0; g < G; ++g) expand_add(i0 + g * stride, key, sm, s[g]);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const long i = i0 + g * stride;
      if (i < P4) {
        int4 o;
        o.x = (int)(quantise(v[g].x, R, scale, clamped, nans) + s[g][0]);
        o.y = (int)(quantise(v[g].y, R, scale, clamped, nans) + s[g][1]);
        o.z = (int)(quantise(v[g].z, R, scale, clamped, nans) + s[g][2]);
        o.w = (int)(quantise(v[g].w, R, scale, clamped, nans) + s[g][3]);
        reinterpret_cast<int4*>(orow)[i] = o;
      }
    }
  }
  clamped = wave_sum(clamped);
  nans = wave_sum(nans);
  if ((threadIdx.x & 63) == 0) {
    if (clamped) atomicAdd(stats + 2 * row, clamped);
    if (nans) atomicAdd(stats + 2 * row + 1, nans);
  }
}

__global__ void __launch_bounds__(SA_TPB) ring_sum_kernel(const int* __restrict__ rows, long ld, int K,
                                                          long long* __restrict__ acc, long P4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < P4; i += (long)gridDim.x * blockDim.x) {
    longlong2 a = reinterpret_cast<longlong2*>(acc)[2 * i];
    longlong2 b = reinterpret_cast<longlong2*>(acc)[2 * i + 1];
    for (int k = 0; k < K; ++k) {
      const int4 v = reinterpret_cast<const int4*>(rows + (long)k * ld)[i];
      a.x += (long long)v.x;
      a.y += (long long)v.y;
      b.x += (long long)v.z;
      b.y += (long long)v.w;
    }
    reinterpret_cast<longlong2*>(acc)[2 * i] = a;
    reinterpret_cast<longlong2*>(acc)[2 * i + 1] = b;
  }
}

template <int U>
__global__ void __launch_bounds__(SA_TPB) ring_unmask_kernel(long long* __restrict__ acc, long P4,
                                                             const u64* __restrict__ keys,
                                                             const int* __restrict__ signs, int E) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < P4; i += (long)gridDim.x * blockDim.x) {
    long long s[4] = {0, 0, 0, 0};
    int e = 0;
    for (; e + U <= E; e += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        uint32_t w[4];
        const u64 key = keys[e + u];
        const long long sm = signs[e + u] < 0 ? -1ll : 0ll;
        philox4x32_10((uint32_t)((u64)i & 0xffffffffu), (uint32_t)((u64)i >> 32), 0u, SA_TAG,
                      (uint32_t)(key & 0xffffffffull), (uint32_t)(key >> 32), w);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += ((long long)w[j] ^ sm) - sm;
      }
    }
    for (; e < E; ++e) {
      uint32_t w[4];
      const u64 key = keys[e];
      const long long sm = signs[e] < 0 ? -1ll : 0ll;
      philox4x32_10((uint32_t)((u64)i & 0xffffffffu), (uint32_t)((u64)i >> 32), 0u, SA_TAG,
                    (uint32_t)(key & 0xffffffffull), (uint32_t)(key >> 32), w);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += ((long long)w[j] ^ sm) - sm;
    }
    longlong2 a = reinterpret_cast<longlong2*>(acc)[2 * i];
    longlong2 b = reinterpret_cast<longlong2*>(acc)[2 * i + 1];
    a.x -= s[0], a.y -= s[1], b.x -= s[2], b.y -= s[3];
    reinterpret_cast<longlong2*>(acc)[2 * i] = a;
    reinterpret_cast<longlong2*>(acc)[2 * i + 1] = b;
  }
}

inline int sa_grid(long n, int per_block, int cap) { return (int)max(1L, min((long)cap, (n + per_block - 1) / per_block)); }

template <int G, int U>
void launch_mask(const float* x, long ldx, int* out, long ldo, int K, long P4, const int* off, const u64* keys,
                 const int* signs, float R, double scale, int* stats, hipStream_t s) {
  const dim3 grid((unsigned)sa_grid(P4, SA_TPB * G, MASK_MAX_BLOCKS), (unsigned)K);
  hipLaunchKernelGGL((secagg_mask_rows_kernel<G, U>), grid, dim3(SA_TPB), 0, s, x, ldx, out, ldo, P4, off, keys, signs, R,
                     scale, stats);
}

inline int mask_groups(int variant) { return variant == SECAGG_VARIANT_G2U1 ? 2 : 1; }

}  // namespace

long secagg_mask_span(int variant) { return (long)MASK_MAX_BLOCKS * SA_TPB * 4 * mask_groups(variant); }

int secagg_mask_rows(const float* x, long ldx, int* out, long ldo, int K, long P, const int* off,
                     const unsigned long long* keys, const int* signs, float R, int frac_bits, int* stats, int variant,
                     hipStream_t s) {
  if (K <= 0 || P <= 0) return 0;
  // (the caller has checked these; a launch that breaks them would write out of bounds or misaligned)
  if (K > SECAGG_MAX_ROWS || P % 4 != 0 || ldx < P || ldo < P || ldx % 4 != 0 || ldo % 4 != 0) return -1;
  if (x == nullptr || out == nullptr || off == nullptr || stats == nullptr) return -1;
  if (frac_bits < 1 || frac_bits > 200 || !(R > 0.f)) return -1;
  const double scale = ldexp(1.0, frac_bits);
  CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(int) * 2 * (size_t)K, s));
  switch (variant) {
    case SECAGG_VARIANT_G1U1: launch_mask<1, 1>(x, ldx, out, ldo, K, P / 4, off, keys, signs, R, scale, stats, s); break;
    case SECAGG_VARIANT_G2U1: launch_mask<2, 1>(x, ldx, out, ldo, K, P / 4, off, keys, signs, R, scale, stats, s); break;
    case SECAGG_VARIANT_G1U2: launch_mask<1, 2>(x, ldx, out, ldo, K, P / 4, off, keys, signs, R, scale, stats, s); break;
    default: return -1;
  }
  return 0;
}

int ring_sum(const int* rows, long ld, int K, long P, long long* acc, hipStream_t s) {
  if (K <= 0 || P <= 0) return 0;
  if (K > SECAGG_MAX_ROWS || P % 4 != 0 || ld < P || ld % 4 != 0 || rows == nullptr || acc == nullptr) return -1;
  hipLaunchKernelGGL(ring_sum_kernel, dim3(sa_grid(P / 4, SA_TPB, RING_MAX_BLOCKS)), dim3(SA_TPB), 0, s, rows, ld, K, acc,
                     P / 4);
  return 0;
}

int ring_unmask(long long* acc, long P, const unsigned long long* keys, const int* signs, int E, int variant,
                hipStream_t s) {
  if (E <= 0 || P <= 0) return 0;
  if (E > SECAGG_MAX_ROWS * SECAGG_MAX_ROWS || P % 4 != 0 || acc == nullptr || keys == nullptr || signs == nullptr)
    return -1;
  const dim3 grid(sa_grid(P / 4, SA_TPB, RING_MAX_BLOCKS));
  if (variant == SECAGG_VARIANT_G1U2)
    hipLaunchKernelGGL((ring_unmask_kernel<2>), grid, dim3(SA_TPB), 0, s, acc, P / 4, keys, signs, E);
  else
    hipLaunchKernelGGL((ring_unmask_kernel<1>), grid, dim3(SA_TPB), 0, s, acc, P / 4, keys, signs, E);
  return 0;
}
