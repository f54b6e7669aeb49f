// Top-k sparse uploads with error feedback (gfx950): exact selection of the k largest-|u| elements
// of every row of u [K, P] into a packed (idx, val) payload, plus the receiver's decode and the
// server's fused fp64 accumulation (ops/compress.py SparsePayload).
//
// Selection rule (identical in the CPU oracle, ops/compress.py):
//   key(i) = bits(u[i]) & 0x7fffffff  (|u| as a monotone unsigned integer; −0 ≡ +0, NaN above inf);
//   inter-tensor padding is never eligible (one validity bit per element, vbits);
//   the k eligible elements with the largest keys are selected, ties at the threshold key τ go to
//   the lower flat index. k ≤ number of eligible elements, so exactly k are selected.
//
// Pipeline per pack (all rows at once, nothing read back to the host):
//   3 × (histogram pass over the row, one-workgroup-per-row bin pick): radix select of τ over the
//       31-bit key in 11 + 10 + 10 bits. Per-workgroup LDS histograms are flushed with integer adds
//       into hist [K][2048] (counts do not depend on arrival order). state [K][2] = (key prefix,
//       remaining rank); after the last pass it is (τ, r) with r = k − count(key > τ) ties to take.
//       The first pass of the error-feedback form reads delta and err and stores u = delta + err
//       into err (one IEEE add), so no separate add pass exists.
//   count:     per (row, 4096-element chunk) the elements with key > τ and with key == τ;
//   chunkscan: ordered exclusive scan of both counts over the chunks of a row;
//   emit:      element i is written at  G(i) + min(E(i), r)  — G/E the number of lower-index elements
//              with key > τ / key == τ (chunk base + in-chunk rank from wave ballots) — if
//              key > τ, or key == τ and E(i) < r. Rows therefore come out in ascending index order.
//              The error-feedback form zeroes the selected positions of err.
// No float atomics anywhere. Rows are 16-B aligned (layout offsets and P are multiples of 16).
#include "common.h"
#include "dls.h"

namespace {

constexpr int TPB = 256;           // 4 waves
constexpr int TILE = TPB * 4;      // one float4 per thread
constexpr int CHUNK = 4 * TILE;    // count / emit granularity (dls.h TOPK_CHUNK)
constexpr int HIST_LD = 2048;      // bins of the widest pass = row stride of hist
constexpr int ACC_SPAN = 2048;     // fp64 LDS accumulators per workgroup (16 KiB)
static_assert(CHUNK == TOPK_CHUNK, "dls.h TOPK_CHUNK");

__device__ __forceinline__ uint32_t valid4(const uint32_t* __restrict__ vbits, long i0) {
  return (vbits[i0 >> 5] >> (i0 & 31)) & 0xfu;  // i0 is a multiple of 4
}
__device__ __forceinline__ uint32_t key_of(float f) { return __float_as_uint(f) & 0x7fffffffu; }

// PASS 0: bits 30..20 (2048 bins); 1: bits 19..10 of the keys under the prefix; 2: bits 9..0.
// EF (PASS 0 only): u = src + err is formed here and stored into err.
template <int PASS, bool EF>
__global__ __launch_bounds__(TPB) void topk_hist_kernel(const float* __restrict__ src, long ld_s,
                                                        float* __restrict__ err, long ld_e,
                                                        const uint32_t* __restrict__ vbits,
                                                        const uint32_t* __restrict__ state,
                                                        uint32_t* __restrict__ hist, long P) {
  constexpr int NB = PASS == 0 ? 2048 : 1024;
  __shared__ uint32_t h[NB];
  const int tid = threadIdx.x, row = blockIdx.y;
  for (int i = tid; i < NB; i += TPB) h[i] = 0;
  __syncthreads();
  const uint32_t prefix = PASS ? state[2 * row] : 0u;
  const float* s = src + (long)row * ld_s;
  for (long i0 = (long)blockIdx.x * TILE + tid * 4; i0 < P; i0 += (long)gridDim.x * TILE) {
    float4 v = *reinterpret_cast<const float4*>(s + i0);
    if constexpr (EF) {
      float* e = err + (long)row * ld_e + i0;
      const float4 r = *reinterpret_cast<const float4*>(e);
      v.x += r.x;
      v.y += r.y;
      v.z += r.z;
      v.w += r.w;
      *reinterpret_cast<float4*>(e) = v;
    }
    const uint32_t nib = valid4(vbits, i0);
    const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!((nib >> j) & 1u)) continue;
      const uint32_t key = key_of(f[j]);
      if constexpr (PASS == 0) {
        atomicAdd(&h[key >> 20], 1u);
      } else if constexpr (PASS == 1) {
        if ((key >> 20) == (prefix >> 20)) atomicAdd(&h[(key >> 10) & 1023u], 1u);
      } else {
        if ((key >> 10) == (prefix >> 10)) atomicAdd(&h[key & 1023u], 1u);
      }
    }
  }
  __syncthreads();
  uint32_t* g = hist + (long)row * HIST_LD;
  for (int i = tid; i < NB; i += TPB) {
    const uint32_t c = h[i];
    if (c) atomicAdd(&g[i], c);
  }
}

// One workgroup per row: the bin holding the krem-th largest key under the prefix. Writes the
// extended prefix and the rank remaining inside that bin; leaves the row's bins zero again.
template <int NB>
__global__ __launch_bounds__(TPB) void topk_scan_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ state,
                                                        int shift, int first, uint32_t k) {
  constexpr int PER = NB / TPB;
  __shared__ uint32_t part[TPB];
  const int tid = threadIdx.x, row = blockIdx.x;
  uint32_t* g = hist + (long)row * HIST_LD + tid * PER;
  uint32_t b[PER], sum = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    b[j] = g[j];
    g[j] = 0;
    sum += b[j];
  }
  part[tid] = sum;
  const uint32_t prefix = first ? 0u : state[2 * row];
  const uint32_t krem = first ? k : state[2 * row + 1];
  __syncthreads();  // (also: every thread has read state before one of them writes it)
  uint32_t above = 0;
  for (int t = tid + 1; t < TPB; ++t) above += part[t];
#pragma unroll
  for (int j = PER - 1; j >= 0; --j) {
    const uint32_t c = b[j];
    if (above < krem && krem <= above + c) {
      state[2 * row] = prefix | ((uint32_t)(tid * PER + j) << shift);
      state[2 * row + 1] = krem - above;
    }
    above += c;
  }
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(TPB) void topk_count_kernel(const float* __restrict__ src, long ld,
                                                         const uint32_t* __restrict__ vbits,
                                                         const uint32_t* __restrict__ state,
                                                         uint32_t* __restrict__ cnt, long P, int nchunks) {
  __shared__ uint32_t red[TPB / 64][2];
  const int tid = threadIdx.x, row = blockIdx.y, c = blockIdx.x;
  const uint32_t tau = state[2 * row];
  const float* s = src + (long)row * ld;
  uint32_t ng = 0, ne = 0;
#pragma unroll
  for (int it = 0; it < CHUNK / TILE; ++it) {
    const long i0 = (long)c * CHUNK + it * TILE + tid * 4;
    if (i0 >= P) break;
    const float4 v = *reinterpret_cast<const float4*>(s + i0);
    const uint32_t nib = valid4(vbits, i0);
    const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t key = key_of(f[j]);
      const bool ok = (nib >> j) & 1u;
      ng += ok && key > tau;
      ne += ok && key == tau;
    }
  }
  ng = wave_sum_u32(ng);
  ne = wave_sum_u32(ne);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = ng;
    red[tid >> 6][1] = ne;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t a = 0, b = 0;
    for (int w = 0; w < TPB / 64; ++w) {
      a += red[w][0];
      b += red[w][1];
    }
    cnt[((long)row * nchunks + c) * 2] = a;
    cnt[((long)row * nchunks + c) * 2 + 1] = b;
  }
}

// One workgroup per row: excl[c] = Σ_{c' < c} cnt[c'] for both counts, in chunk order.
__global__ __launch_bounds__(TPB) void topk_chunkscan_kernel(const uint32_t* __restrict__ cnt,
                                                             uint32_t* __restrict__ excl, int nchunks) {
  __shared__ uint32_t pg[TPB], pe[TPB];
  const int tid = threadIdx.x, row = blockIdx.x;
  const int per = (nchunks + TPB - 1) / TPB;
  const int lo = min(tid * per, nchunks), hi = min(lo + per, nchunks);
  const uint32_t* c = cnt + (long)row * nchunks * 2;
  uint32_t* x = excl + (long)row * nchunks * 2;
  uint32_t g = 0, e = 0;
  for (int i = lo; i < hi; ++i) {
    g += c[2 * i];
    e += c[2 * i + 1];
  }
  pg[tid] = g;
  pe[tid] = e;
  __syncthreads();
  g = e = 0;
  for (int t = 0; t < tid; ++t) {
    g += pg[t];
    e += pe[t];
  }
  for (int i = lo; i < hi; ++i) {
    x[2 * i] = g;
    x[2 * i + 1] = e;
    g += c[2 * i];
    e += c[2 * i + 1];
  }
}

// ZERO: the selected positions of src (the residual rows) are set to +0.
template <bool ZERO>
__global__ __launch_bounds__(TPB) void topk_emit_kernel(float* __restrict__ src, long ld,
                                                        const uint32_t* __restrict__ vbits,
                                                        const uint32_t* __restrict__ state,
                                                        const uint32_t* __restrict__ cnt,
                                                        const uint32_t* __restrict__ excl, int* __restrict__ idx,
                                                        float* __restrict__ val, long P, int nchunks, uint32_t k) {
  __shared__ uint32_t wt[CHUNK / TILE][TPB / 64][2];
  const int tid = threadIdx.x, row = blockIdx.y, c = blockIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const uint32_t tau = state[2 * row], r = state[2 * row + 1];
  const long q = ((long)row * nchunks + c) * 2;
  uint32_t G = excl[q], E = excl[q + 1];
  if (cnt[q] == 0 && (cnt[q + 1] == 0 || E >= r)) return;  // nothing selected here (workgroup-uniform)
  const unsigned long long lt = (1ull << lane) - 1ull;
  float* s = src + (long)row * ld;
  int* oi = idx + (long)row * k;
  float* ov = val + (long)row * k;
#pragma unroll
  for (int it = 0; it < CHUNK / TILE; ++it) {
    const long i0 = (long)c * CHUNK + it * TILE + tid * 4;
    const bool in = i0 < P;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t nib = 0;
    if (in) {
      v = *reinterpret_cast<const float4*>(s + i0);
      nib = valid4(vbits, i0);
    }
    float f[4] = {v.x, v.y, v.z, v.w};
    uint32_t gm = 0, em = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t key = key_of(f[j]);
      const bool ok = (nib >> j) & 1u;
      gm |= (uint32_t)(ok && key > tau) << j;
      em |= (uint32_t)(ok && key == tau) << j;
    }
    // elements of lower lanes come first, then this lane's own lower elements
    uint32_t pgt = 0, peq = 0, tg = 0, te = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long bg = __ballot((gm >> j) & 1u), be = __ballot((em >> j) & 1u);
      pgt += __popcll(bg & lt);
      peq += __popcll(be & lt);
      tg += __popcll(bg);
      te += __popcll(be);
    }
    if (lane == 0) {
      wt[it][wave][0] = tg;
      wt[it][wave][1] = te;
    }
    __syncthreads();
    uint32_t wg = 0, we = 0, ag = 0, ae = 0;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) {
      const uint32_t a = wt[it][w][0], b = wt[it][w][1];
      if (w < wave) {
        wg += a;
        we += b;
      }
      ag += a;
      ae += b;
    }
    uint32_t g0 = G + wg + pgt, e0 = E + we + peq;
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t pos = k;
      if ((gm >> j) & 1u) {
        pos = g0 + min(e0, r);
        ++g0;
      } else if ((em >> j) & 1u) {
        if (e0 < r) pos = g0 + e0;
        ++e0;
      }
      if (pos < k) {
        oi[pos] = (int)(i0 + j);
        ov[pos] = f[j];
        f[j] = 0.f;
        any = true;
      }
    }
    if (ZERO && any) *reinterpret_cast<float4*>(s + i0) = make_float4(f[0], f[1], f[2], f[3]);
    G += ag;
    E += ae;
  }
}

__global__ __launch_bounds__(TPB) void topk_zero_kernel(float* __restrict__ out, long ld, long P) {
  const long i0 = ((long)blockIdx.x * TPB + threadIdx.x) * 4;
  if (i0 < P) *reinterpret_cast<float4*>(out + (long)blockIdx.y * ld + i0) = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(TPB) void topk_scatter_kernel(const int* __restrict__ idx, const float* __restrict__ val,
                                                           float* __restrict__ out, long ld, long P, int k) {
  const long j = (long)blockIdx.x * TPB + threadIdx.x;
  const int row = blockIdx.y;
  if (j >= k) return;
  const long i = idx[(long)row * k + j];
  if (i >= 0 && i < P) out[(long)row * ld + i] = val[(long)row * k + j];
}

__device__ __forceinline__ int lower_bound(const int* __restrict__ a, int n, long x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long)a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// acc[i] += Σ_k w[k]·val_k[i], per destination: one workgroup owns ACC_SPAN consecutive elements
// of acc as fp64 LDS slots and adds the clients' entries that fall in them in client order (a
// client's indices are unique, a barrier separates clients): one writer per element, fixed order.
__global__ __launch_bounds__(TPB) void topk_acc_kernel(const int* __restrict__ idx, const float* __restrict__ val,
                                                       const double* __restrict__ w, double* __restrict__ acc, long P,
                                                       int K, int k) {
  __shared__ double slot[ACC_SPAN];
  __shared__ int ba[TPB], bb[TPB];
  const int tid = threadIdx.x;
  const long lo = (long)blockIdx.x * ACC_SPAN, hi = min(lo + ACC_SPAN, P);
  for (int i = tid; i < ACC_SPAN; i += TPB) slot[i] = 0.0;
  for (int k0 = 0; k0 < K; k0 += TPB) {
    __syncthreads();
    if (k0 + tid < K) {  // the entry ranges of up to 256 clients, searched in parallel
      const int* a = idx + (long)(k0 + tid) * k;
      ba[tid] = lower_bound(a, k, lo);
      bb[tid] = lower_bound(a, k, hi);
    }
    __syncthreads();
    const int n = min(TPB, K - k0);
    for (int c = 0; c < n; ++c) {
      const int a = ba[c], b = bb[c];
      if (a == b) continue;  // (workgroup-uniform)
      const double wk = w[k0 + c];
      const long base = (long)(k0 + c) * k;
      for (int j = a + tid; j < b; j += TPB) {
        const long d = (long)idx[base + j] - lo;
        if (d >= 0 && d < ACC_SPAN) slot[d] += wk * (double)val[base + j];
      }
      __syncthreads();
    }
  }
  __syncthreads();
  for (long i = lo + tid; i < hi; i += TPB) acc[i] += slot[i - lo];
}

}  // namespace

void topk_pack(const float* delta, long ld_d, float* u, long ld_u, int ef, const uint32_t* vbits, uint32_t* hist,
               uint32_t* state, uint32_t* cnt, uint32_t* excl, int* idx, float* val, int K, long P, int k,
               hipStream_t s) {
  if (K == 0 || P == 0 || k <= 0) return;
  const int nchunks = cdiv(P, CHUNK);
  // histogram passes: a few thousand workgroups in all, each striding over its row
  const int tiles = cdiv(P, TILE), want = cdiv(4096, K) > 8 ? cdiv(4096, K) : 8;
  const int hx = tiles < want ? tiles : want;
  const dim3 hg(hx, K), blk(TPB);
  if (ef)
    hipLaunchKernelGGL((topk_hist_kernel<0, true>), hg, blk, 0, s, delta, ld_d, u, ld_u, vbits, state, hist, P);
  else
    hipLaunchKernelGGL((topk_hist_kernel<0, false>), hg, blk, 0, s, u, ld_u, nullptr, 0L, vbits, state, hist, P);
  hipLaunchKernelGGL((topk_scan_kernel<2048>), dim3(K), blk, 0, s, hist, state, 20, 1, (uint32_t)k);
  hipLaunchKernelGGL((topk_hist_kernel<1, false>), hg, blk, 0, s, u, ld_u, nullptr, 0L, vbits, state, hist, P);
  hipLaunchKernelGGL((topk_scan_kernel<1024>), dim3(K), blk, 0, s, hist, state, 10, 0, (uint32_t)k);
  hipLaunchKernelGGL((topk_hist_kernel<2, false>), hg, blk, 0, s, u, ld_u, nullptr, 0L, vbits, state, hist, P);
  hipLaunchKernelGGL((topk_scan_kernel<1024>), dim3(K), blk, 0, s, hist, state, 0, 0, (uint32_t)k);
  hipLaunchKernelGGL(topk_count_kernel, dim3(nchunks, K), blk, 0, s, u, ld_u, vbits, state, cnt, P, nchunks);
  hipLaunchKernelGGL(topk_chunkscan_kernel, dim3(K), blk, 0, s, cnt, excl, nchunks);
  if (ef)
    hipLaunchKernelGGL((topk_emit_kernel<true>), dim3(nchunks, K), blk, 0, s, u, ld_u, vbits, state, cnt, excl, idx,
                       val, P, nchunks, (uint32_t)k);
  else
    hipLaunchKernelGGL((topk_emit_kernel<false>), dim3(nchunks, K), blk, 0, s, u, ld_u, vbits, state, cnt, excl, idx,
                       val, P, nchunks, (uint32_t)k);
}

void topk_decode(const int* idx, const float* val, float* out, long ld, int K, long P, int k, hipStream_t s) {
  if (K == 0 || P == 0) return;
  hipLaunchKernelGGL(topk_zero_kernel, dim3(cdiv(P, TILE), K), dim3(TPB), 0, s, out, ld, P);
  if (k <= 0) return;
  hipLaunchKernelGGL(topk_scatter_kernel, dim3(cdiv(k, TPB), K), dim3(TPB), 0, s, idx, val, out, ld, P, k);
}

void topk_accumulate(const int* idx, const float* val, const double* w, double* acc, int K, long P, int k,
                     hipStream_t s) {
  if (K == 0 || P == 0 || k <= 0) return;
  hipLaunchKernelGGL(topk_acc_kernel, dim3(cdiv(P, ACC_SPAN)), dim3(TPB), 0, s, idx, val, w, acc, P, K, k);
}
