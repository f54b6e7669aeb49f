// GroupNorm kernels (gfx950) for channels-last activations [K][B][H·W][C]: G groups of Cg = C / G
// adjacent channels, one statistic per (client, sample, group) over n = H·W·Cg elements.
//
// One 512-thread workgroup per (sample, client) does everything that sample needs, so what is
// computed for a sample depends on that sample alone — not on K, B, `valid` or the slot it sits
// in (N ranks ≡ 1 rank, ragged steps exact, bitwise).
//   forward : sweep 1 Σx per channel → group means; sweep 2 Σ(x − μ)² per channel → group rstd
//             (two-pass variance: no Σx² − nμ² cancellation); sweep 3 y = (x − μ)·rstd·γ + β
//             (+ residual, ReLU), fp32 y and / or its split-bf16 planes. Sweeps 2 and 3 re-read a
//             sample of 32–256 KB that sweep 1 just pulled through the cache hierarchy.
//   backward: sweep 1 per-channel Σĝ, Σĝ·x̂ of the sample (ĝ = dy·[y > 0]) — these are the sample's
//             dβ / dγ partials, stored as one row per sample — and from them the group means of
//             γĝ and γĝx̂; sweep 2 dx = rstd·(γĝ − mean(γĝ) − x̂·mean(γĝx̂)) and dres = ĝ.
//             gn_param_fold_kernel then adds the rows of samples b < valid[k], b ascending.
// Every sum has a fixed order (per-thread pixel walk, LDS rows folded ascending, wave_sum over the
// channels of a group): no atomics, bitwise reproducible.
// Samples b ≥ valid[k] are never read (the halo convs leave them unwritten): their outputs are +0.
#include "common.h"
#include "dls.h"

namespace {

constexpr int GN_NT = 512;  // threads per workgroup (8 waves)

// Thread layout inside a channel block of `ctn` V-channel chunks: chunk cc = tid % ctn, pixel lane
// rl = tid / ctn of RT = GN_NT / ctn (threads with rl ≥ RT idle: ctn does not divide GN_NT).
struct GnLane {
  int ctn, RT, cc, rl, c0;
  bool on;
};
template <int V>
__device__ __forceinline__ GnLane gn_lane(int cg, int CT) {
  GnLane l;
  l.ctn = min(GN_NT, CT - cg);
  l.RT = GN_NT / l.ctn;
  l.cc = threadIdx.x % l.ctn;
  l.rl = threadIdx.x / l.ctn;
  l.c0 = (cg + l.cc) * V;
  l.on = l.rl < l.RT;
  return l;
}

// out[j] = Σ_r red[r·nch + j], r ascending: the RT per-thread partial rows of nch channels
__device__ __forceinline__ void gn_fold_rows(const float* red, float* out, int nch, int RT) {
  for (int j = threadIdx.x; j < nch; j += GN_NT) {
    float a = red[j];
    for (int r = 1; r < RT; ++r) a += red[r * nch + j];
    out[j] = a;
  }
}

// out[g] = Σ_{c in group g} w_c·cs[c] / n, one wave per group (lanes stride the channels, wave_sum)
template <typename T>
__device__ __forceinline__ void gn_group_means(const float* cs, const T* w, float* out, int G, int Cg, float n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int g = wave; g < G; g += GN_NT / 64) {
    float a = 0.f;
    for (int c = lane; c < Cg; c += 64) a += (w ? ldf(w + g * Cg + c) : 1.f) * cs[g * Cg + c];
    a = wave_sum(a);
    if (lane == 0) out[g] = a / n;
  }
}

template <int V>
__device__ __forceinline__ void gn_store_planes(bf16_t* hi, bf16_t* lo, const float* f) {
  if constexpr (V == 4) {
    uint32_t h[2], l[2];
    split_pair(f[0], f[1], h[0], l[0]);
    split_pair(f[2], f[3], h[1], l[1]);
    *reinterpret_cast<uint2*>(hi) = make_uint2(h[0], h[1]);
    *reinterpret_cast<uint2*>(lo) = make_uint2(l[0], l[1]);
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) split2(f[i], hi[i], lo[i]);
  }
}

// dynamic LDS (floats): red0[GN_NT·V], red1[GN_NT·V], cs0[C], cs1[C], g0[G], g1[G]
__host__ __device__ inline size_t gn_lds_floats(int V, int C, int G) { return (size_t)2 * GN_NT * V + 2 * C + 2 * G; }

// grid (B, K). yp (fp32 only): y's split planes, client k's hi plane at yp + 2·k·B·n, its lo plane
// B·n later ([K][2][B][n], the layout of ops split_planes), written next to the fp32 y.
template <typename T, int V>
__global__ void __launch_bounds__(GN_NT) gn_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                       const T* __restrict__ gamma, const T* __restrict__ beta,
                                                       T* __restrict__ y, bf16_t* __restrict__ yp,
                                                       float* __restrict__ mean, float* __restrict__ rstd,
                                                       const int* __restrict__ valid, long g_cs, int rep, int B,
                                                       int HW, int C, int G, float eps, int relu) {
  extern __shared__ float sm[];
  float* red = sm;
  float* cs = sm + 2 * GN_NT * V;
  float* gm = cs + 2 * C;
  float* gr = gm + G;
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int Cg = C / G, CT = C / V;
  const long n = (long)HW * C;
  const long so = ((long)k * B + b) * n;
  const T* xs = x + so;
  T* ys = y + so;
  bf16_t* hp = yp ? yp + ((long)2 * k * B + b) * n : nullptr;
  const long lo_off = (long)B * n;
  float* ms = mean + ((long)k * B + b) * G;
  float* rs = rstd + ((long)k * B + b) * G;
  if (valid && b >= valid[k]) {  // (block-uniform) a skipped sample: nothing is read
    float z[V];
#pragma unroll
    for (int i = 0; i < V; ++i) z[i] = 0.f;
    for (long i = (long)tid * V; i < n; i += (long)GN_NT * V) {
      store_vec<V>(ys + i, z);
      if (hp) gn_store_planes<V>(hp + i, hp + lo_off + i, z);
    }
    for (int g = tid; g < G; g += GN_NT) ms[g] = rs[g] = 0.f;
    return;
  }
  // sweep 1: Σx per channel
  for (int cg = 0; cg < CT; cg += GN_NT) {
    const GnLane l = gn_lane<V>(cg, CT);
    if (l.on) {
      float s[V];
#pragma unroll
      for (int i = 0; i < V; ++i) s[i] = 0.f;
#pragma unroll 4
      for (int p = l.rl; p < HW; p += l.RT) {
        float v[V];
        load_vec<V>(xs + (long)p * C + l.c0, v);
#pragma unroll
        for (int i = 0; i < V; ++i) s[i] += v[i];
      }
#pragma unroll
      for (int i = 0; i < V; ++i) red[(l.rl * l.ctn + l.cc) * V + i] = s[i];
    }
    __syncthreads();
    gn_fold_rows(red, cs + cg * V, l.ctn * V, l.RT);
    __syncthreads();
  }
  gn_group_means<T>(cs, nullptr, gm, G, Cg, (float)HW * Cg);
  __syncthreads();
  // sweep 2: Σ(x − μ)² per channel
  for (int cg = 0; cg < CT; cg += GN_NT) {
    const GnLane l = gn_lane<V>(cg, CT);
    if (l.on) {
      float s[V], mu[V];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        s[i] = 0.f;
        mu[i] = gm[(l.c0 + i) / Cg];
      }
#pragma unroll 4
      for (int p = l.rl; p < HW; p += l.RT) {
        float v[V];
        load_vec<V>(xs + (long)p * C + l.c0, v);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const float d = v[i] - mu[i];
          s[i] += d * d;
        }
      }
#pragma unroll
      for (int i = 0; i < V; ++i) red[(l.rl * l.ctn + l.cc) * V + i] = s[i];
    }
    __syncthreads();
    gn_fold_rows(red, cs + cg * V, l.ctn * V, l.RT);
    __syncthreads();
  }
  gn_group_means<T>(cs, nullptr, gr, G, Cg, (float)HW * Cg);  // (the biased variance for now)
  __syncthreads();
  for (int g = tid; g < G; g += GN_NT) {
    const float r = rsqrtf(gr[g] + eps);
    gr[g] = r;
    ms[g] = gm[g];
    rs[g] = r;
  }
  __syncthreads();
  // sweep 3: apply
  const T* gk = gamma + (long)(k / rep) * g_cs;
  const T* bk = beta + (long)(k / rep) * g_cs;
  const T* rr = res ? res + so : nullptr;
  for (int cg = 0; cg < CT; cg += GN_NT) {
    const GnLane l = gn_lane<V>(cg, CT);
    if (!l.on) continue;
    float mu[V], sc[V], bt[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int g = (l.c0 + i) / Cg;
      mu[i] = gm[g];
      sc[i] = gr[g] * ldf(gk + l.c0 + i);
      bt[i] = ldf(bk + l.c0 + i);
    }
#pragma unroll 2
    for (int p = l.rl; p < HW; p += l.RT) {
      const long off = (long)p * C + l.c0;
      float v[V], o[V];
      load_vec<V>(xs + off, v);
#pragma unroll
      for (int i = 0; i < V; ++i) o[i] = fmaf(v[i] - mu[i], sc[i], bt[i]);
      if (rr) {
        float rv[V];
        load_vec<V>(rr + off, rv);
#pragma unroll
        for (int i = 0; i < V; ++i) o[i] += rv[i];
      }
      if (relu) {
#pragma unroll
        for (int i = 0; i < V; ++i) o[i] = fmaxf(o[i], 0.f);
      }
      store_vec<V>(ys + off, o);
      if (hp) gn_store_planes<V>(hp + off, hp + lo_off + off, o);
    }
  }
}

// grid (B, K). part: [K][B][2][C] per-sample rows (Σĝx̂ = the sample's dγ, then Σĝ = its dβ)
template <typename T, int V>
__global__ void __launch_bounds__(GN_NT) gn_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                       const T* __restrict__ y, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const T* __restrict__ gamma,
                                                       const int* __restrict__ valid, long g_cs, int rep, int B,
                                                       int HW, int C, int G, int relu, T* __restrict__ dx,
                                                       T* __restrict__ dres, float* __restrict__ part) {
  extern __shared__ float sm[];
  float* red0 = sm;
  float* red1 = sm + GN_NT * V;
  float* cs0 = sm + 2 * GN_NT * V;
  float* cs1 = cs0 + C;
  float* ga = cs1 + C;
  float* gb = ga + G;
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int Cg = C / G, CT = C / V;
  const long n = (long)HW * C;
  const long so = ((long)k * B + b) * n;
  if (valid && b >= valid[k]) {  // skipped sample: dx = dres = +0, no partial row (the fold skips it)
    float z[V];
#pragma unroll
    for (int i = 0; i < V; ++i) z[i] = 0.f;
    for (long i = (long)tid * V; i < n; i += (long)GN_NT * V) {
      store_vec<V>(dx + so + i, z);
      if (dres) store_vec<V>(dres + so + i, z);
    }
    return;
  }
  const T* dys = dy + so;
  const T* xs = x + so;
  const T* ysm = y + so;
  const float* ms = mean + ((long)k * B + b) * G;
  const float* rs = rstd + ((long)k * B + b) * G;
  float* prow = part + ((long)k * B + b) * 2 * C;
  // sweep 1: per-channel Σĝx̂ and Σĝ
  for (int cg = 0; cg < CT; cg += GN_NT) {
    const GnLane l = gn_lane<V>(cg, CT);
    if (l.on) {
      float s0[V], s1[V], mu[V], r[V];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        s0[i] = s1[i] = 0.f;
        mu[i] = ms[(l.c0 + i) / Cg];
        r[i] = rs[(l.c0 + i) / Cg];
      }
#pragma unroll 2
      for (int p = l.rl; p < HW; p += l.RT) {
        const long off = (long)p * C + l.c0;
        float g[V], v[V];
        load_vec<V>(dys + off, g);
        load_vec<V>(xs + off, v);
        if (relu) {
          float yv[V];
          load_vec<V>(ysm + off, yv);
#pragma unroll
          for (int i = 0; i < V; ++i) g[i] = yv[i] > 0.f ? g[i] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
          s0[i] += g[i];
          s1[i] += g[i] * ((v[i] - mu[i]) * r[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < V; ++i) {
        red0[(l.rl * l.ctn + l.cc) * V + i] = s0[i];
        red1[(l.rl * l.ctn + l.cc) * V + i] = s1[i];
      }
    }
    __syncthreads();
    gn_fold_rows(red0, cs0 + cg * V, l.ctn * V, l.RT);
    gn_fold_rows(red1, cs1 + cg * V, l.ctn * V, l.RT);
    __syncthreads();
  }
  for (int c = tid; c < C; c += GN_NT) {
    prow[c] = cs1[c];
    prow[C + c] = cs0[c];
  }
  const T* gk = gamma + (long)(k / rep) * g_cs;
  gn_group_means<T>(cs0, gk, ga, G, Cg, (float)HW * Cg);
  gn_group_means<T>(cs1, gk, gb, G, Cg, (float)HW * Cg);
  __syncthreads();
  // sweep 2: dx (and the residual branch's gradient ĝ)
  for (int cg = 0; cg < CT; cg += GN_NT) {
    const GnLane l = gn_lane<V>(cg, CT);
    if (!l.on) continue;
    float mu[V], r[V], gw[V], ma[V], mb[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int g = (l.c0 + i) / Cg;
      mu[i] = ms[g];
      r[i] = rs[g];
      gw[i] = ldf(gk + l.c0 + i);
      ma[i] = ga[g];
      mb[i] = gb[g];
    }
#pragma unroll 2
    for (int p = l.rl; p < HW; p += l.RT) {
      const long off = (long)p * C + l.c0;
      float g[V], v[V], o[V];
      load_vec<V>(dys + off, g);
      load_vec<V>(xs + off, v);
      if (relu) {
        float yv[V];
        load_vec<V>(ysm + off, yv);
#pragma unroll
        for (int i = 0; i < V; ++i) g[i] = yv[i] > 0.f ? g[i] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float xh = (v[i] - mu[i]) * r[i];
        o[i] = r[i] * (gw[i] * g[i] - ma[i] - xh * mb[i]);
      }
      store_vec<V>(dx + so + off, o);
      if (dres) store_vec<V>(dres + so + off, g);
    }
  }
}

// dγ[k][c] = Σ_{b < valid[k]} part[k][b][0][c], dβ likewise from row 1, b ascending. grid (cdiv(C, 256), K)
__global__ void __launch_bounds__(256) gn_param_fold_kernel(const float* __restrict__ part,
                                                            const int* __restrict__ valid, int B, int C,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            long dg_cs) {
  const int k = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int nb = valid ? min(max(valid[k], 0), B) : B;
  const float* p = part + (long)k * B * 2 * C;
  float a = 0.f, d = 0.f;
  for (int b = 0; b < nb; ++b) {
    a += p[(long)b * 2 * C + c];
    d += p[(long)b * 2 * C + C + c];
  }
  dgamma[(long)k * dg_cs + c] = a;
  dbeta[(long)k * dg_cs + c] = d;
}

}  // namespace

long gn_workspace_floats(int K, int B, int C) { return (long)K * B * 2 * C; }

bool gn_shape_ok(int HW, int C, int G) {
  // LDS: 2·512·V + 2C + 2G floats ≤ 48 KiB at C = 2048 (ResNet-50's widest); int pixel offsets
  return HW > 0 && C > 0 && G > 0 && C % G == 0 && C <= 2048 && (long)HW * C < (1L << 31);
}

void gn_fwd(const void* x, const void* res, const void* gamma, const void* beta, void* y, bf16_t* yp, float* mean,
            float* rstd, const int* valid, long g_cs, int rep, int K, int B, int HW, int C, int G, float eps, int relu,
            int f32, hipStream_t s) {
  if (K == 0 || B == 0) return;
  dim3 grid(B, K);
  const int V = C % 4 == 0 ? 4 : 1;
  const size_t lds = gn_lds_floats(V, C, G) * sizeof(float);
#define GN_FWD(TT, VV)                                                                                              \
  hipLaunchKernelGGL((gn_fwd_kernel<TT, VV>), grid, dim3(GN_NT), lds, s, static_cast<const TT*>(x),                 \
                     static_cast<const TT*>(res), static_cast<const TT*>(gamma), static_cast<const TT*>(beta),      \
                     static_cast<TT*>(y), f32 ? yp : nullptr, mean, rstd, valid, g_cs, rep, B, HW, C, G, eps, relu)
  if (f32) {
    if (V == 4) GN_FWD(float, 4); else GN_FWD(float, 1);
  } else {
    if (V == 4) GN_FWD(bf16_t, 4); else GN_FWD(bf16_t, 1);
  }
#undef GN_FWD
}

void gn_bwd(const void* dy, const void* x, const void* y, const float* mean, const float* rstd, const void* gamma,
            const int* valid, long g_cs, int rep, int K, int B, int HW, int C, int G, int relu, void* dx, void* dres,
            float* dgamma, float* dbeta, long dg_cs, float* ws, int f32, hipStream_t s) {
  if (K == 0) return;
  dim3 grid(B, K);
  const int V = C % 4 == 0 ? 4 : 1;
  const size_t lds = gn_lds_floats(V, C, G) * sizeof(float);
#define GN_BWD(TT, VV)                                                                                             \
  hipLaunchKernelGGL((gn_bwd_kernel<TT, VV>), grid, dim3(GN_NT), lds, s, static_cast<const TT*>(dy),               \
                     static_cast<const TT*>(x), static_cast<const TT*>(y), mean, rstd, static_cast<const TT*>(gamma), \
                     valid, g_cs, rep, B, HW, C, G, relu, static_cast<TT*>(dx), static_cast<TT*>(dres), ws)
  if (B > 0) {
    if (f32) {
      if (V == 4) GN_BWD(float, 4); else GN_BWD(float, 1);
    } else {
      if (V == 4) GN_BWD(bf16_t, 4); else GN_BWD(bf16_t, 1);
    }
  }
#undef GN_BWD
  hipLaunchKernelGGL(gn_param_fold_kernel, dim3(cdiv(C, 256), K), dim3(256), 0, s, (const float*)ws, valid, B, C,
                     dgamma, dbeta, dg_cs);
}
