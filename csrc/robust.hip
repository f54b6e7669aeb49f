// Robust aggregation (gfx950): coordinate-wise trimmed sum of the rows of x [n, P] — the kernel of
// the trimmed-mean and median methods (algorithm/robust_algorithm.py, ops/ref.py trimmed_sum).
//
// Contract (identical in the CPU oracle):
//   key(v) = bits(v) ^ ((bits(v) >> 31) & 0x7fffffff), arithmetic shift: a signed 32-bit integer,
//   monotone over all non-NaN floats, −0 below +0, negative-sign NaNs below −inf, positive-sign NaNs
//   above +inf. Equal keys are equal bit patterns, so ties need no rule and the sort need not be stable.
//   Per column the n values are sorted by key, the b lowest and b highest dropped, and the remaining
//   n − 2b added as doubles ONE AT A TIME in ascending key order starting from +0.0 (fp64 sums of
//   fp32 values with a wide exponent spread depend on the order). A NaN sum is written as the
//   canonical quiet NaN 0x7ff8000000000000 (x86 and gfx950 disagree on the sign and payload of a
//   generated or propagated NaN). The caller divides by n − 2b.
//
// One launch, one workgroup per tile of C columns:
//   load   the [n, C] tile as keys into LDS, one float4 (16 B) per lane per row segment (coalesced);
//   sort   every column with a bitonic network whose compare-exchanges all put the smaller key at the
//          lower row (the first step of each merge compares i with its mirror in the 2j-block, the
//          others i with i + j). A network for the next power of two N2 ≥ n in which rows ≥ n hold
//          +∞ never moves those rows, so LDS holds n rows only and exchanges with such a row are
//          no-ops. A lane owns four adjacent columns: one ds_read_b128 / ds_write_b128 per row,
//          16 consecutive lanes cover 64 consecutive dwords (conflict-free, MI355X LDS banking).
//          Up to three consecutive steps run on 2, 4 or 8 rows held in registers (the rows that the
//          steps j, j/2, j/4 connect form an arithmetic progression, and so do the mirror step's
//          two halves), so a merge of 128 rows is 3 LDS round trips and barriers instead of 7;
//   walk   one lane per column adds rows b .. n−b−1 in order (fp64) and stores 8 B.
// The tile is widened for small n (C = 256 up to 32 rows ... 32 from 129 rows on) so that LDS per
// workgroup stays ≤ 32 KiB up to n = 256 (64 KiB at n = 512) and a 13-client cohort still fills
// every CU. Each input element is read from HBM once. No atomics of any kind.
#include "common.h"
#include "dls.h"

namespace {

constexpr int TPB = 256;

__device__ __forceinline__ int key_of(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }  // involution

__device__ __forceinline__ void cex(int4& a, int4& b) {
  const int4 lo = make_int4(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z), min(a.w, b.w));
  b = make_int4(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z), max(a.w, b.w));
  a = lo;
}

// T consecutive steps of the network on the R = 2^T rows they connect, held in registers.
// MIRROR (l = lk, the merge's level, T ≤ lk): the mirror step of the 2^lk-blocks and the T − 1
// half-cleaners after it; the rows are two progressions of R/2 rows with spacing 2^(lk−T), one in
// each half of the block, and the mirror step pairs row m with row R − 1 − m.
// else (l = lj, T − 1 ≤ lj): the half-cleaners j = 2^lj .. 2^(lj−T+1) on one progression with
// spacing 2^(lj−T+1). Rows ascend with m, a row ≥ n counts as +∞ and is neither read nor written,
// and a group whose second row is ≥ n has nothing to exchange.
template <int T, bool MIRROR, int Q, int G>
__device__ __forceinline__ void sort_pass(int4* tile, int n, int n2, int l, int q, int g) {
  constexpr int R = 1 << T, H = R / 2;
  const int ljl = MIRROR ? l - T : l - (T - 1), jl = 1 << ljl;
  for (int e = g; e < (n2 >> T); e += G) {
    const int off = e & (jl - 1);
    int row[R];
    if constexpr (MIRROR) {
      const int base = (e >> ljl) << l;
#pragma unroll
      for (int m = 0; m < H; ++m) {
        row[m] = base + off + m * jl;
        row[H + m] = base + (1 << (l - 1)) + (jl - 1 - off) + m * jl;
      }
    } else {
      const int i = ((e >> ljl) << (ljl + T)) + off;
#pragma unroll
      for (int m = 0; m < R; ++m) row[m] = i + m * jl;
    }
    if (row[1] >= n) continue;
    int4 v[R];
#pragma unroll
    for (int m = 0; m < R; ++m)
      v[m] = row[m] < n ? tile[row[m] * Q + q] : make_int4(INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX);
    if constexpr (MIRROR) {
#pragma unroll
      for (int m = 0; m < H; ++m) cex(v[m], v[R - 1 - m]);
    }
#pragma unroll
    for (int s = MIRROR ? 1 : 0; s < T; ++s) {
      const int st = 1 << (T - 1 - s);
#pragma unroll
      for (int m = 0; m < R; ++m)
        if (!(m & st)) cex(v[m], v[m + st]);
    }
#pragma unroll
    for (int m = 0; m < R; ++m)
      if (row[m] < n) tile[row[m] * Q + q] = v[m];
  }
}

template <int C>
__global__ __launch_bounds__(TPB) void trimmed_sum_kernel(const float* __restrict__ x, long ld, int n, int b,
                                                          int n2, long P, double* __restrict__ out) {
  constexpr int Q = C / 4;    // column quads per row
  constexpr int G = TPB / Q;  // rows handled per step
  extern __shared__ int4 tile[];  // [n][Q] quads of keys
  const int tid = threadIdx.x;
  const long c0 = (long)blockIdx.x * C;
  const int q = tid % Q, g = tid / Q;

  for (int r = g; r < n; r += G) {
    const long col = c0 + 4 * q;
    int4 v = make_int4(0, 0, 0, 0);
    if (col < P) v = *reinterpret_cast<const int4*>(x + (long)r * ld + col);  // P % 4 == 0
    tile[r * Q + q] = make_int4(key_of(v.x), key_of(v.y), key_of(v.z), key_of(v.w));
  }
  __syncthreads();

  int l2 = 0;
  while ((1 << l2) < n2) ++l2;
  for (int lk = 1; lk <= l2; ++lk) {
    // merge of sorted 2^(lk-1)-runs: lk steps (mirror, then half-cleaners j = 2^(lk-2) .. 1), ≤ 3 per pass
    int t = min(3, lk);
    if (t == 3) sort_pass<3, true, Q, G>(tile, n, n2, lk, q, g);
    else if (t == 2) sort_pass<2, true, Q, G>(tile, n, n2, lk, q, g);
    else sort_pass<1, true, Q, G>(tile, n, n2, lk, q, g);
    __syncthreads();
    for (int rem = lk - t; rem > 0; rem -= t) {
      t = min(3, rem);
      if (t == 3) sort_pass<3, false, Q, G>(tile, n, n2, rem - 1, q, g);
      else if (t == 2) sort_pass<2, false, Q, G>(tile, n, n2, rem - 1, q, g);
      else sort_pass<1, false, Q, G>(tile, n, n2, rem - 1, q, g);
      __syncthreads();
    }
  }

  const int* keys = reinterpret_cast<const int*>(tile);
  for (int c = tid; c < C; c += TPB) {
    if (c0 + c >= P) break;
    double acc = 0.0;
    for (int r = b; r < n - b; ++r) acc += (double)__int_as_float(key_of(keys[r * C + c]));
    if (acc != acc) acc = __longlong_as_double(0x7ff8000000000000LL);
    out[c0 + c] = acc;
  }
}

}  // namespace

void trimmed_sum(const float* x, long ld, int n, int b, long P, double* out, hipStream_t s) {
  if (n < 1 || n > TRIM_MAX_ROWS || b < 0 || 2 * b >= n || P <= 0) return;  // (checked by the caller)
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  const size_t rows_bytes = (size_t)n * 4;
#define LAUNCH(C)                                                                                          \
  hipLaunchKernelGGL(trimmed_sum_kernel<C>, dim3((unsigned)((P + C - 1) / C)), dim3(TPB), rows_bytes * C, s, x, \
                     ld, n, b, n2, P, out)
  if (n <= 32) LAUNCH(256);
  else if (n <= 64) LAUNCH(128);
  else if (n <= 128) LAUNCH(64);
  else LAUNCH(32);
#undef LAUNCH
}
