// Krum / Multi-Krum (gfx950): the n x n matrix of squared L2 distances between the rows of x [n, P] —
// the kernel of ops.fl.pairwise_sq_dists (algorithm/krum_algorithm.py, oracle ops/ref.py).
//
// Contract (identical in the CPU oracle):
//   term(i, j, p) = fl64(d · d) with d = fl64(double(x[i][p]) − double(x[j][p])); the multiply and
//   the add that follows are rounded separately (this file is compiled with -ffp-contract=off, see
//   ops/build.py FILE_FLAGS); denormal fp32 inputs are not flushed.
//   D[i][j] adds the terms in an order fixed by the column index alone: the columns are cut into
//   spans of W = PAIR_SPAN = 4096 columns (the last one may be shorter) and the spans into groups of
//   G = PAIR_GROUP = 8 consecutive spans;
//     span sum  = the span's terms added one at a time in ascending column order from +0.0,
//     group sum = the group's span sums added in ascending span order from +0.0,
//     D[i][j]   = the group sums added in ascending group order from +0.0.
//   Nothing depends on n, the row order, the launch geometry or the device. So D[i][i] = +0.0 for a
//   finite row, D[i][j] and D[j][i] have the same bits ((a − b)² and (b − a)² round alike), a row
//   permutation permutes D, zero columns change nothing (every partial sum is ≥ +0.0 or NaN, and
//   adding +0.0 leaves it as it is), D is finite where both rows are, and NaN / ±inf follow IEEE
//   (NaN payload bits are not part of the contract).
//
// Two launches, no atomics:
//   pair_dist  a workgroup owns one tile (row block bi ≤ row block bj, RB rows each) and `spw`
//              consecutive spans (1, or a whole group). It stages CS = 32 columns of both row blocks
//              in LDS as [column][row] — the next stage's global loads are in flight while the
//              current one is computed — and every lane keeps an R x R register block of pairs:
//              per column one LDS read of R floats for each side (the bj side: T lanes read RB
//              consecutive dwords, the bi side likewise with each address shared by T lanes), 2R conversions and R² independent
//              subtract / multiply / add chains. Span sums are added into the lane's group sum in
//              span order and stored tile-major [entry][tile][RB][RB] to the scratch buffer
//              (coalesced 32-B pieces). A diagonal tile is computed whole. Tiles of one entry are
//              adjacent in the grid, so the row blocks they share are re-read from cache. Columns
//              past a span's end and rows past n are staged as zeros.
//              n ≤ 16: RB 16, R 2; else RB 32, R 4 — 64 lanes, one wave per workgroup, either way.
//              (Measured on the ResNet-18 layout: 64-row tiles with 256 lanes are never faster —
//              5.8 against 4.4 ms at 50 rows, equal at 100, 53 against 49 ms at 256 — since small
//              tiles waste less on and beside the diagonal; giving three waves of a 64-row diagonal
//              tile a quadrant each and idling the fourth gains nothing, the busiest SIMD sets the
//              time.)
//   pair_fold  one workgroup per D[i][j]: lane t adds the entries of group t, t + 256, ... in order
//              (one entry if spw = G — then 0.0 + e = e — else G), and lane 0 adds the group sums in
//              ascending order. Entries below the diagonal are read from the mirrored tile.
// spw = 1 where the scratch buffer stays under 256 MiB (ResNet-18: up to 100 rows, 213 MiB; more and
// evener workgroups: 13.3 against 16.0 ms at 100 rows), else G (n = 512: 341 entries x 136 tiles x
// 8 KiB = 362 MiB; at 256 rows spw = 1 would take 767 MiB and is no faster).
#include "common.h"
#include "dls.h"

namespace {

constexpr int CS = 32;    // columns per LDS stage
constexpr int PADR = 4;   // row padding of a stage line: the transposing stores spread over the banks
constexpr int FOLD_TPB = 256;

template <int RB, int R>
__global__ __launch_bounds__((RB / R) * (RB / R)) void pair_dist_kernel(const float* __restrict__ x, long ld, int n,
                                                                        long P, int nb, int ntiles, int spw,
                                                                        double* __restrict__ part) {
  constexpr int T = RB / R, TPB = T * T;
  constexpr int QS = CS / 4;               // column quads per stage row
  constexpr int LOADS = RB * QS / TPB;     // float4 loads per lane, block and stage
  constexpr int LDR = RB + PADR;
  static_assert(RB * QS % TPB == 0 && (R == 2 || R == 4), "tile shape");
  __shared__ __align__(16) float sa[CS * LDR];
  __shared__ __align__(16) float sb[CS * LDR];

  const int tid = threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)ntiles);
  const long entry = blockIdx.x / (unsigned)ntiles;
  int bi = 0, bj = tile;  // upper-triangle tiles, row-major: row bi holds nb − bi of them
  while (bj >= nb - bi) {
    bj -= nb - bi;
    ++bi;
  }
  bj += bi;
  // the lane's R x R pairs: rows ia .. ia + R − 1 of block bi against rows jb .. of block bj
  const int ia = R * (tid / T), jb = R * (tid % T);

  float4 ra[LOADS], rb[LOADS];
  auto gload = [&](long c0, long cend) {
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
      const int e = tid + k * TPB, q = e % QS, row = e / QS;
      const long col = c0 + 4 * q;  // (P % 4 == 0 and W % 4 == 0: a quad never straddles cend)
      const int ga = bi * RB + row, gb = bj * RB + row;
      ra[k] = rb[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (col < cend) {
        if (ga < n) ra[k] = *reinterpret_cast<const float4*>(x + (long)ga * ld + col);
        if (gb < n) rb[k] = *reinterpret_cast<const float4*>(x + (long)gb * ld + col);
      }
    }
  };
  auto sstore = [&]() {
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
      const int e = tid + k * TPB, q = e % QS, row = e / QS;
      float* pa = sa + (4 * q) * LDR + row;
      float* pb = sb + (4 * q) * LDR + row;
      pa[0] = ra[k].x, pa[LDR] = ra[k].y, pa[2 * LDR] = ra[k].z, pa[3 * LDR] = ra[k].w;
      pb[0] = rb[k].x, pb[LDR] = rb[k].y, pb[2 * LDR] = rb[k].z, pb[3 * LDR] = rb[k].w;
    }
  };

  double tot[R][R];
#pragma unroll
  for (int p = 0; p < R; ++p)
#pragma unroll
    for (int q = 0; q < R; ++q) tot[p][q] = 0.0;

  for (int s = 0; s < spw; ++s) {
    const long cbeg = (entry * spw + s) * (long)PAIR_SPAN;
    if (cbeg >= P) break;
    const long cend = min(P, cbeg + (long)PAIR_SPAN);
    double acc[R][R];
#pragma unroll
    for (int p = 0; p < R; ++p)
#pragma unroll
      for (int q = 0; q < R; ++q) acc[p][q] = 0.0;
    gload(cbeg, cend);
    for (long c0 = cbeg; c0 < cend; c0 += CS) {
      __syncthreads();  // the previous stage has been read
      sstore();
      __syncthreads();
      if (c0 + CS < cend) gload(c0 + CS, cend);
#pragma unroll 4
      for (int c = 0; c < CS; ++c) {
        float a[R], b[R];
        if constexpr (R == 4) {
          const float4 va = *reinterpret_cast<const float4*>(sa + c * LDR + ia);
          const float4 vb = *reinterpret_cast<const float4*>(sb + c * LDR + jb);
          a[0] = va.x, a[1] = va.y, a[2] = va.z, a[3] = va.w;
          b[0] = vb.x, b[1] = vb.y, b[2] = vb.z, b[3] = vb.w;
        } else {
          const float2 va = *reinterpret_cast<const float2*>(sa + c * LDR + ia);
          const float2 vb = *reinterpret_cast<const float2*>(sb + c * LDR + jb);
          a[0] = va.x, a[1] = va.y;
          b[0] = vb.x, b[1] = vb.y;
        }
        double da[R], db[R];
#pragma unroll
        for (int p = 0; p < R; ++p) da[p] = (double)a[p], db[p] = (double)b[p];
#pragma unroll
        for (int p = 0; p < R; ++p)
#pragma unroll
          for (int q = 0; q < R; ++q) {
            const double d = da[p] - db[q];
            const double t = d * d;  // (rounded; contraction is off for this file)
            acc[p][q] = acc[p][q] + t;
          }
      }
    }
#pragma unroll
    for (int p = 0; p < R; ++p)
#pragma unroll
      for (int q = 0; q < R; ++q) tot[p][q] = tot[p][q] + acc[p][q];
  }

  double* dst = part + ((long)blockIdx.x * RB + ia) * RB + jb;  // [entry][tile][RB][RB]
#pragma unroll
  for (int p = 0; p < R; ++p)
#pragma unroll
    for (int q = 0; q < R; q += 2) *reinterpret_cast<double2*>(dst + p * RB + q) = make_double2(tot[p][q], tot[p][q + 1]);
}

// One workgroup per D[i][j]. `nent` scratch entries of `epg` entries per group.
__global__ __launch_bounds__(FOLD_TPB) void pair_fold_kernel(const double* __restrict__ part, int n, int rb, int nb,
                                                             int ntiles, long nent, int epg, double* __restrict__ out) {
  __shared__ double gs[FOLD_TPB];
  const int tid = threadIdx.x;
  const int i = blockIdx.x / (unsigned)n, j = blockIdx.x % (unsigned)n;
  int bi = i / rb, li = i % rb, bj = j / rb, lj = j % rb;
  if (bi > bj) {  // below the diagonal: the mirrored tile's entry (same bits)
    int t = bi;
    bi = bj, bj = t;
    t = li, li = lj, lj = t;
  }
  const long tile = (long)bi * nb - (long)bi * (bi - 1) / 2 + (bj - bi);
  const long stride = (long)ntiles * rb * rb;
  const double* src = part + (tile * rb + li) * rb + lj;
  const long ngroups = (nent + epg - 1) / epg;
  double total = 0.0;
  for (long g0 = 0; g0 < ngroups; g0 += FOLD_TPB) {
    const long g = g0 + tid;
    double sum = 0.0;
    if (g < ngroups) {
      const long e1 = min(nent, (g + 1) * epg);
      for (long e = g * epg; e < e1; ++e) sum = sum + src[e * stride];
    }
    __syncthreads();  // lane 0 has read the previous chunk
    gs[tid] = sum;
    __syncthreads();
    if (tid == 0) {
      const int cnt = (int)min((long)FOLD_TPB, ngroups - g0);
      for (int t = 0; t < cnt; ++t) total = total + gs[t];
    }
  }
  if (tid == 0) out[(long)i * n + j] = total;
}

inline int row_block(int n) { return n <= 16 ? 16 : 32; }

inline long tiles_of(int n) {
  const int rb = row_block(n), nb = (n + rb - 1) / rb;
  return (long)nb * (nb + 1) / 2;
}

inline long spans_of(long P) { return (P + PAIR_SPAN - 1) / PAIR_SPAN; }

}  // namespace

long pairwise_ws_doubles(int n, long P, int spw) {
  if (n < 1 || n > TRIM_MAX_ROWS || P <= 0 || (spw != 1 && spw != PAIR_GROUP)) return 0;
  const int rb = row_block(n);
  return (spans_of(P) + spw - 1) / spw * tiles_of(n) * rb * rb;
}

int pairwise_spans_per_wg(int n, long P) {
  return pairwise_ws_doubles(n, P, 1) * 8 <= (256L << 20) ? 1 : PAIR_GROUP;
}

void pairwise_sq_dists(const float* x, long ld, int n, long P, double* ws, int spw, double* out, hipStream_t s) {
  if (n < 1 || n > TRIM_MAX_ROWS || P <= 0 || (spw != 1 && spw != PAIR_GROUP)) return;  // (checked by the caller)
  const int rb = row_block(n), nb = (n + rb - 1) / rb;
  const int ntiles = (int)tiles_of(n);
  const long nent = (spans_of(P) + spw - 1) / spw;
  const unsigned grid = (unsigned)(nent * ntiles);
#define LAUNCH(RB, R)                                                                                              \
  hipLaunchKernelGGL((pair_dist_kernel<RB, R>), dim3(grid), dim3((RB / R) * (RB / R)), 0, s, x, ld, n, P, nb, ntiles, \
                     spw, ws)
  if (rb == 16) LAUNCH(16, 2);
  else LAUNCH(32, 4);
#undef LAUNCH
  hipLaunchKernelGGL(pair_fold_kernel, dim3((unsigned)(n * n)), dim3(FOLD_TPB), 0, s, ws, n, rb, nb, ntiles, nent,
                     PAIR_GROUP / spw, out);
}
