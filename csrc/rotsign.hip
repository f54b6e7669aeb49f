// 1-bit rotated uploads (DRIVE / EDEN, gfx950): per client row and per block of 4096 flat elements a
// randomised Hadamard rotation, one sign bit per coordinate and one fp32 scale; the receiver's decode
// and the server's fused fp64 accumulation (ops/compress.py RotSignPayload).
//
// Contract (identical in the CPU oracle, ops/compress.py; this file is built with -ffp-contract=off):
//   u_i   = the row's element i, +0.0 where i >= P or i is inter-tensor padding (vbits bit clear);
//   z_i   = u_i · d_i, d_i = −1 iff bit 31 of mix32(i, seed_k) is set (i the flat index);
//   FWHT  : stages h = 1, 2, 4, …, 2048 in that order, (a, b) → (a + b, a − b) for every pair
//           (j, j + h) with j & h = 0, one fp32 rounding each; then y = z′ · 2⁻⁶ (exact, 4096 = 4⁶);
//   L1, L2: Σ|y_j| and Σ y_j² in fp64, added as an adjacent-pair tree over j (12 levels);
//   S     = fp32(L2 / L1) (unbiased) or fp32(L1 / 4096) (mse); L1 = 0 gives S = 0;
//   bit j = sign bit of y_j, LSB-first (byte j >> 3, bit j & 7);
//   decode: t_j = ±S from the bits, the same FWHT, · 2⁻⁶, · d_i.
//
// One 256-lane workgroup transforms one block, 16 elements per lane, in three register rounds of four
// stages. Lane t, register e hold element
//   layout A: 16 t + e                              (stages 1..8;   the global-memory order)
//   layout B: 256 (t >> 4) + 16 e + (t & 15)        (stages 16..128)
//   layout C: 256 e + t                             (stages 256..2048)
// and the two changes of layout go through one LDS tile, padded by one float per 16 so that all
// three access patterns are (nearly) bank-conflict free. Every lane writes only the tile slots it read
// last, so one barrier per change of layout suffices. The pack returns to layout A for the trees (their
// levels 0..3 are then register adds) and stores a lane's 16 sign bits as one 2-byte word. No float
// atomics, no scratch.
#include "common.h"
#include "dls.h"

namespace {

constexpr int TPB = 256;                 // 4 waves
constexpr int EPL = 16;                  // elements per lane
constexpr int RB = ROTSIGN_BLOCK;        // 4096
constexpr int TILE_LD = RB + RB / 16;    // 17 KiB
static_assert(TPB * EPL == RB, "one workgroup per block");

__device__ __forceinline__ int pad(int j) { return j + (j >> 4); }
__device__ __forceinline__ int j_a(int t, int e) { return t * 16 + e; }
__device__ __forceinline__ int j_b(int t, int e) { return ((t >> 4) << 8) + (e << 4) + (t & 15); }
__device__ __forceinline__ int j_c(int t, int e) { return (e << 8) + t; }

__device__ __forceinline__ float flip(float x, uint32_t signbit) {
  return __uint_as_float(__float_as_uint(x) ^ signbit);
}

// four butterfly stages over the register index, on register pairs so that they compile to packed
// adds (a − b is formed as a + (−b): the same rounding)
__device__ __forceinline__ void fwht16(float (&v)[EPL]) {
  f32x2_t p[EPL / 2];
#pragma unroll
  for (int j = 0; j < EPL / 2; ++j) {  // h = 1: (a, b) → (a + b, a − b) inside a pair
    const f32x2_t aa = {v[2 * j], v[2 * j]}, bb = {v[2 * j + 1], -v[2 * j + 1]};
    p[j] = aa + bb;
  }
#pragma unroll
  for (int h = 1; h < EPL / 2; h <<= 1) {  // h = 2, 4, 8: between pairs
#pragma unroll
    for (int j = 0; j < EPL / 2; ++j) {
      if (j & h) continue;
      const f32x2_t a = p[j], b = p[j + h];
      p[j] = a + b;
      p[j + h] = a + (-b);
    }
  }
#pragma unroll
  for (int j = 0; j < EPL / 2; ++j) {
    v[2 * j] = p[j].x;
    v[2 * j + 1] = p[j].y;
  }
}

// v: layout A in, layout C out (scaled by 2⁻⁶). The caller guarantees that no lane still reads
// another lane's layout-A slots of the tile.
__device__ __forceinline__ void fwht4096(float (&v)[EPL], float* tile, int t) {
  fwht16(v);
#pragma unroll
  for (int e = 0; e < EPL; ++e) tile[pad(j_a(t, e))] = v[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < EPL; ++e) v[e] = tile[pad(j_b(t, e))];
  fwht16(v);
#pragma unroll
  for (int e = 0; e < EPL; ++e) tile[pad(j_b(t, e))] = v[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < EPL; ++e) v[e] = tile[pad(j_c(t, e))];
  fwht16(v);
#pragma unroll
  for (int e = 0; e < EPL; ++e) v[e] *= 0.015625f;
}

// layout C → layout A
__device__ __forceinline__ void c_to_a(float (&v)[EPL], float* tile, int t) {
#pragma unroll
  for (int e = 0; e < EPL; ++e) tile[pad(j_c(t, e))] = v[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < EPL; ++e) v[e] = tile[pad(j_a(t, e))];
}

// adjacent-pair tree over the block: levels 0..3 over the lane's 16 registers (layout A), 4..9 over
// the lanes of a wave, 10..11 over the four waves. Every lane returns the total.
__device__ __forceinline__ double block_tree_sum(double (&a)[EPL], double* red, int t) {
#pragma unroll
  for (int w = EPL; w > 1; w >>= 1) {
#pragma unroll
    for (int j = 0; j < w / 2; ++j) a[j] = a[2 * j] + a[2 * j + 1];
  }
  double s = a[0];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s = s + __shfl_xor(s, o, 64);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per (block, client). EF: u = delta + err, and err ← u − x̂ (0 at padding).
template <bool EF>
__global__ __launch_bounds__(TPB) void rotsign_pack_kernel(const float* __restrict__ delta, long ld_d,
                                                           float* __restrict__ err, long ld_e,
                                                           const uint32_t* __restrict__ vbits,
                                                           const uint32_t* __restrict__ seeds,
                                                           uint16_t* __restrict__ bits, float* __restrict__ scale,
                                                           long P, int nb, int mse) {
  __shared__ float tile[TILE_LD];
  __shared__ double red[2][TPB / 64];
  const int t = threadIdx.x, b = blockIdx.x, k = blockIdx.y;
  const long i0 = (long)b * RB + t * EPL;
  const bool in = i0 < P;  // P % 16 == 0: a lane's 16 elements are inside the row or all beyond it
  float u[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) u[e] = 0.f;
  uint32_t vm = 0;
  if (in) {
    load_vec<EPL>(delta + (long)k * ld_d + i0, u);
    if constexpr (EF) {
      float r[EPL];
      load_vec<EPL>(err + (long)k * ld_e + i0, r);
#pragma unroll
      for (int e = 0; e < EPL; ++e) u[e] += r[e];
    }
    vm = (vbits[i0 >> 5] >> (i0 & 31)) & 0xffffu;
  }
  const uint32_t seed = seeds[k];
  uint32_t dm = 0;  // bit e: d = −1 for element e
  float v[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    if (!((vm >> e) & 1u)) u[e] = 0.f;
    const uint32_t neg = mix32((uint32_t)(i0 + e), seed) >> 31;
    dm |= neg << e;
    v[e] = flip(u[e], neg << 31);
  }
  fwht4096(v, tile, t);
  c_to_a(v, tile, t);  // y in the global order: the trees pair index-adjacent elements
  double a1[EPL], a2[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const double y = (double)v[e];
    a1[e] = fabs(y);
    a2[e] = y * y;
  }
  const double L1 = block_tree_sum(a1, red[0], t);
  const double L2 = block_tree_sum(a2, red[1], t);
  const float S = mse ? (float)(L1 * (1.0 / 4096.0)) : (L1 == 0.0 ? 0.f : (float)(L2 / L1));
  uint32_t sb = 0;
#pragma unroll
  for (int e = 0; e < EPL; ++e) sb |= (__float_as_uint(v[e]) >> 31) << e;
  const long blk = (long)k * nb + b;
  bits[blk * TPB + t] = (uint16_t)sb;
  if (t == 0) scale[blk] = S;
  if constexpr (EF) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) v[e] = flip(S, ((sb >> e) & 1u) << 31);
    fwht4096(v, tile, t);
    c_to_a(v, tile, t);
    if (in) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const float xh = flip(v[e], ((dm >> e) & 1u) << 31);
        v[e] = ((vm >> e) & 1u) ? u[e] - xh : 0.f;
      }
      store_vec<EPL>(err + (long)k * ld_e + i0, v);
    }
  }
}

// the block's ±S in layout A from its code bytes
__device__ __forceinline__ void load_signs(float (&v)[EPL], const uint16_t* __restrict__ bits,
                                           const float* __restrict__ scale, long blk, int t) {
  const float S = scale[blk];
  const uint32_t sb = bits[blk * TPB + t];
#pragma unroll
  for (int e = 0; e < EPL; ++e) v[e] = flip(S, ((sb >> e) & 1u) << 31);
}

// out [K][P] (row stride ld): the decoded rows, 0.0 at padding; nothing is written at or beyond P.
__global__ __launch_bounds__(TPB) void rotsign_unpack_kernel(const uint16_t* __restrict__ bits,
                                                             const float* __restrict__ scale,
                                                             const uint32_t* __restrict__ vbits,
                                                             const uint32_t* __restrict__ seeds,
                                                             float* __restrict__ out, long ld, long P, int nb) {
  __shared__ float tile[TILE_LD];
  const int t = threadIdx.x, b = blockIdx.x, k = blockIdx.y;
  float v[EPL];
  load_signs(v, bits, scale, (long)k * nb + b, t);
  fwht4096(v, tile, t);
  const uint32_t seed = seeds[k];
  float* o = out + (long)k * ld;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const long i = (long)b * RB + j_c(t, e);
    if (i >= P) continue;
    const bool ok = (vbits[i >> 5] >> (i & 31)) & 1u;
    o[i] = ok ? flip(v[e], mix32((uint32_t)i, seed) & 0x80000000u) : 0.f;
  }
}

// acc[i] = acc[i] + w_k · x̂_k[i] for k = 0..K−1 in order, one workgroup per block: acc is read and
// written once, the K decoded blocks exist only in registers. (4 waves per SIMD: left to itself the
// compiler spreads this loop over 408 registers, one wave per SIMD; at 5 or more it spills to scratch.)
__global__ __launch_bounds__(TPB, 4) void rotsign_acc_kernel(const uint16_t* __restrict__ bits,
                                                          const float* __restrict__ scale,
                                                          const uint32_t* __restrict__ vbits,
                                                          const uint32_t* __restrict__ seeds,
                                                          const double* __restrict__ w, double* __restrict__ acc,
                                                          long P, int nb, int K) {
  __shared__ float tile[TILE_LD];
  const int t = threadIdx.x, b = blockIdx.x;
  double a[EPL];
  uint32_t vm = 0;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const long i = (long)b * RB + j_c(t, e);
    a[e] = 0.0;
    if (i < P && ((vbits[i >> 5] >> (i & 31)) & 1u)) {
      vm |= 1u << e;
      a[e] = acc[i];
    }
  }
#pragma nounroll
  for (int k = 0; k < K; ++k) {
    float v[EPL];
    load_signs(v, bits, scale, (long)k * nb + b, t);
    const uint32_t seed = seeds[k];
    const double wk = w[k];
    __syncthreads();  // the previous client's layout-C reads are done
    fwht4096(v, tile, t);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const uint32_t i = (uint32_t)b * RB + j_c(t, e);
      const double x = (double)flip(v[e], mix32(i, seed) & 0x80000000u);
      a[e] = a[e] + wk * x;  // (also where vm is clear: those registers are never stored)
    }
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e)
    if ((vm >> e) & 1u) acc[(long)b * RB + j_c(t, e)] = a[e];
}

}  // namespace

void rotsign_pack(const float* delta, long ld_d, float* err, long ld_e, const uint32_t* vbits, const uint32_t* seeds,
                  uint8_t* bits, float* scale, int K, long P, int mse, hipStream_t s) {
  if (K == 0 || P == 0) return;
  const int nb = cdiv(P, RB);
  uint16_t* b16 = reinterpret_cast<uint16_t*>(bits);
  if (err)
    hipLaunchKernelGGL((rotsign_pack_kernel<true>), dim3(nb, K), dim3(TPB), 0, s, delta, ld_d, err, ld_e, vbits, seeds,
                       b16, scale, P, nb, 1);
  else
    hipLaunchKernelGGL((rotsign_pack_kernel<false>), dim3(nb, K), dim3(TPB), 0, s, delta, ld_d, nullptr, 0L, vbits,
                       seeds, b16, scale, P, nb, mse);
}

void rotsign_unpack(const uint8_t* bits, const float* scale, const uint32_t* vbits, const uint32_t* seeds, float* out,
                    long ld, int K, long P, hipStream_t s) {
  if (K == 0 || P == 0) return;
  const int nb = cdiv(P, RB);
  hipLaunchKernelGGL(rotsign_unpack_kernel, dim3(nb, K), dim3(TPB), 0, s, reinterpret_cast<const uint16_t*>(bits),
                     scale, vbits, seeds, out, ld, P, nb);
}

void rotsign_accumulate(const uint8_t* bits, const float* scale, const uint32_t* vbits, const uint32_t* seeds,
                        const double* w, double* acc, int K, long P, hipStream_t s) {
  if (K == 0 || P == 0) return;
  const int nb = cdiv(P, RB);
  hipLaunchKernelGGL(rotsign_acc_kernel, dim3(nb), dim3(TPB), 0, s, reinterpret_cast<const uint16_t*>(bits), scale,
                     vbits, seeds, w, acc, P, nb, K);
}
