// Client-level DP-FedAvg (gfx950): per-row squared L2 norms, the clipped fp64 accumulation and the
// Gaussian noise draw — the kernels of ops.fl.row_sq_norms / clip_scales / clipped_sum / gaussian_add
// (algorithm/dp_algorithm.py, oracle ops/ref.py). Compiled with -ffp-contract=off (ops/build.py
// FILE_FLAGS): every multiply and the add that follows it are rounded separately.
//
// row_sq_norms   out[k] = Σ_p fl64(double(x[k][p])²) (the product is exact) in the summation order of
//                pairwise_sq_dists (krum.hip): spans of PAIR_SPAN columns added one term at a time in
//                ascending column order from +0.0, groups of PAIR_GROUP span sums, then the group sums.
//                A span sum is ONE sequential chain of 4096 dependent adds, so a lane owns a span:
//                  row_span_kernel  a one-wave workgroup owns NS = 64 consecutive spans of one row. It
//                                   stages CS = 32 columns of all 64 spans in LDS as [column][span]
//                                   (each span's 128 B piece is read by 8 lanes; the next stage's
//                                   loads are in flight while the current one is added up) and lane t
//                                   adds the terms of span t. Columns past P are staged as zeros
//                                   (partial sums are ≥ +0.0 or NaN: adding +0.0 changes nothing).
//                                   Span sums go to the scratch buffer [n][spans].
//                  row_fold_kernel  one workgroup per row: lane t adds the span sums of group t, t +
//                                   256, ... in order, lane 0 adds the group sums in ascending order.
// clip_scales    s[k] = clip / sqrt(nsq[k]) if sqrt(nsq[k]) > clip else 1.0; a non-finite nsq[k] gives
//                s[k] = 0 and rejected[k] = 1. sqrt and the division are correctly rounded.
// clipped_sum    out[p] = fl64(out[p] + fl64(s[k] · double(x[k][p]))) for k ascending, rejected rows
//                skipped; the weighted_sum_kernel shape (float4 / double4, rows innermost). s is formed
//                on the device by clip_scales_kernel in the same stream: no host read in between.
// gaussian_add   acc[p] += fl64(std · z[p]) where mask[p] != 0; one Philox4x32-10 call and one
//                Box-Muller pair per element pair, keyed by (seed, stream, p) alone.
// No atomics anywhere: every output element has one writer.
#include "common.h"
#include "dls.h"
#include "philox.h"

namespace {

constexpr int NS = 64;        // spans (= lanes) per workgroup of row_span_kernel
constexpr int CS = 32;        // columns per LDS stage
constexpr int LDR = NS + 1;   // stage line: the transposing stores of a half wave hit 32 banks
constexpr int QS = CS / 4;    // column quads per span and stage
constexpr int LOADS = QS;    // float4 loads per lane and stage (NS · QS quads over NS lanes)
constexpr int FOLD_TPB = 256;

__global__ __launch_bounds__(NS) void row_span_kernel(const float* __restrict__ x, long ld, long P, long S, int nwg,
                                                      double* __restrict__ part) {
  __shared__ float sa[CS * LDR];
  const int tid = threadIdx.x;
  const long row = blockIdx.x / (unsigned)nwg;
  const long span0 = (long)(blockIdx.x % (unsigned)nwg) * NS;
  const float* xr = x + row * ld;
  // the workgroup's first span is its longest: columns of a span that any of its spans still has
  const long wmax = min((long)PAIR_SPAN, P - span0 * PAIR_SPAN);

  float4 ra[LOADS];
  auto gload = [&](long cofs) {
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
      const int e = tid + k * NS, q = e % QS, sp = e / QS;
      // (P % 4 == 0 and PAIR_SPAN % 4 == 0: a quad never straddles P or a span's end)
      const long col = (span0 + sp) * PAIR_SPAN + cofs + 4 * q;
      ra[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (col < P) ra[k] = *reinterpret_cast<const float4*>(xr + col);
    }
  };
  auto sstore = [&]() {
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
      const int e = tid + k * NS, q = e % QS, sp = e / QS;
      float* pa = sa + (4 * q) * LDR + sp;
      pa[0] = ra[k].x, pa[LDR] = ra[k].y, pa[2 * LDR] = ra[k].z, pa[3 * LDR] = ra[k].w;
    }
  };

  double acc = 0.0;
  gload(0);
  for (long c0 = 0; c0 < wmax; c0 += CS) {
    __syncthreads();  // the previous stage has been read
    sstore();
    __syncthreads();
    if (c0 + CS < wmax) gload(c0 + CS);
#pragma unroll 8
    for (int c = 0; c < CS; ++c) {
      const double d = (double)sa[c * LDR + tid];
      const double t = d * d;  // (exact: 24-bit mantissa squared)
      acc = acc + t;
    }
  }
  if (span0 + tid < S) part[row * S + span0 + tid] = acc;
}

__global__ __launch_bounds__(FOLD_TPB) void row_fold_kernel(const double* __restrict__ part, long S,
                                                            double* __restrict__ out) {
  __shared__ double gs[FOLD_TPB];
  const int tid = threadIdx.x;
  const double* src = part + (long)blockIdx.x * S;
  const long ngroups = (S + PAIR_GROUP - 1) / PAIR_GROUP;
  double total = 0.0;
  for (long g0 = 0; g0 < ngroups; g0 += FOLD_TPB) {
    const long g = g0 + tid;
    double sum = 0.0;
    if (g < ngroups) {
      const long e1 = min(S, (g + 1) * PAIR_GROUP);
      for (long e = g * PAIR_GROUP; e < e1; ++e) sum = sum + src[e];
    }
    __syncthreads();  // lane 0 has read the previous chunk
    gs[tid] = sum;
    __syncthreads();
    if (tid == 0) {
      const int cnt = (int)min((long)FOLD_TPB, ngroups - g0);
      for (int t = 0; t < cnt; ++t) total = total + gs[t];
    }
  }
  if (tid == 0) out[blockIdx.x] = total;
}

__global__ void clip_scales_kernel(const double* __restrict__ nsq, double clip, int n, double* __restrict__ s,
                                   uint8_t* __restrict__ rejected) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const double v = nsq[k];
  const bool bad = !(fabs(v) < __builtin_huge_val());  // NaN or ±inf
  double sc = 0.0;
  if (!bad) {
    const double norm = sqrt(v);
    sc = norm > clip ? clip / norm : 1.0;
  }
  s[k] = sc;
  rejected[k] = bad ? 1 : 0;
}

__global__ void __launch_bounds__(256) clipped_sum_kernel(const float* __restrict__ x, const double* __restrict__ sc,
                                                          const uint8_t* __restrict__ rejected,
                                                          double* __restrict__ out, int K, long P4, long ld) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < P4; i += (long)gridDim.x * blockDim.x) {
    double4 a = reinterpret_cast<double4*>(out)[i];
    for (int k = 0; k < K; ++k) {
      if (rejected[k]) continue;  // (uniform) skipped, not multiplied: 0 · NaN would poison the sum
      const float4 v = reinterpret_cast<const float4*>(x + (long)k * ld)[i];
      const double w = sc[k];
      const double tx = w * (double)v.x, ty = w * (double)v.y, tz = w * (double)v.z, tw = w * (double)v.w;
      a.x = a.x + tx;
      a.y = a.y + ty;
      a.z = a.z + tz;
      a.w = a.w + tw;
    }
    reinterpret_cast<double4*>(out)[i] = a;
  }
}

__global__ void __launch_bounds__(256) gaussian_add_kernel(double* __restrict__ acc, const uint8_t* __restrict__ mask,
                                                           long P, double std, uint32_t k0, uint32_t k1,
                                                           uint32_t stream) {
  const long npairs = (P + 1) / 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += (long)gridDim.x * blockDim.x) {
    const long p0 = 2 * i, p1 = 2 * i + 1;
    const bool m0 = mask == nullptr || mask[p0] != 0;
    const bool m1 = p1 < P && (mask == nullptr || mask[p1] != 0);
    if (!m0 && !m1) continue;
    uint32_t w[4];
    philox4x32_10((uint32_t)((unsigned long)i & 0xffffffffu), (uint32_t)((unsigned long)i >> 32), stream, 0x44503031u,
                  k0, k1, w);
    const double u1 = (double)((((unsigned long)(w[0] >> 5)) << 26) + (unsigned long)(w[1] >> 6) + 1ul) * 0x1p-53;
    const double u2 = (double)((((unsigned long)(w[2] >> 5)) << 26) + (unsigned long)(w[3] >> 6)) * 0x1p-53;
    const double r = sqrt(-2.0 * log(u1));
    const double phi = 6.283185307179586 * u2;  // fl64(2π) · u2, rounded once
    if (m0) {
      const double z = r * cos(phi);
      const double t = std * z;
      acc[p0] = acc[p0] + t;
    }
    if (m1) {
      const double z = r * sin(phi);
      const double t = std * z;
      acc[p1] = acc[p1] + t;
    }
  }
}

inline long dp_spans_of(long P) { return (P + PAIR_SPAN - 1) / PAIR_SPAN; }

inline int dp_grid(long n, int per_block, int cap) {
  return (int)max(1L, min((long)cap, (n + per_block - 1) / per_block));
}

}  // namespace

long row_sq_norms_ws_doubles(int n, long P) { return n < 1 || P <= 0 ? 0 : (long)n * dp_spans_of(P); }

void row_sq_norms(const float* x, long ld, int n, long P, double* ws, double* out, hipStream_t s) {
  if (n < 1 || P <= 0) return;
  const long S = dp_spans_of(P);
  const long nwg = (S + NS - 1) / NS;
  if ((long)n * nwg > 0x7fffffffL) return;  // (checked by the caller)
  hipLaunchKernelGGL(row_span_kernel, dim3((unsigned)(n * nwg)), dim3(NS), 0, s, x, ld, P, S, (int)nwg, ws);
  hipLaunchKernelGGL(row_fold_kernel, dim3((unsigned)n), dim3(FOLD_TPB), 0, s, ws, S, out);
}

void clip_scales(const double* nsq, double clip, int n, double* scale, uint8_t* rejected, hipStream_t s) {
  if (n < 1) return;
  hipLaunchKernelGGL(clip_scales_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, nsq, clip, n, scale,
                     rejected);
}

void clipped_sum(const float* x, long ld, int n, long P, const double* nsq, double clip, double* scale,
                 uint8_t* rejected, double* out, hipStream_t s) {
  if (n < 1 || P <= 0) return;
  clip_scales(nsq, clip, n, scale, rejected, s);
  hipLaunchKernelGGL(clipped_sum_kernel, dim3(dp_grid(P / 4, 256, 8192)), dim3(256), 0, s, x, scale, rejected, out, n,
                     P / 4, ld);
}

void gaussian_add(double* acc, const uint8_t* mask, long P, double std, unsigned long long seed, unsigned stream,
                  hipStream_t s) {
  if (P <= 0) return;
  hipLaunchKernelGGL(gaussian_add_kernel, dim3(dp_grid((P + 1) / 2, 256, 16384)), dim3(256), 0, s, acc, mask, P, std,
                     (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), (uint32_t)stream);
}
