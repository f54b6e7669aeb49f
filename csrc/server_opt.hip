// Server optimisers on the aggregated pseudo-gradient (gfx950): FedAvgM (Hsu et al. 2019) and FedAdagrad /
// FedAdam / FedYogi (Reddi et al. 2021) — the kernel of ops.fl.server_opt_step (server/server_optimizer.py,
// oracle ops/ref.py). Compiled with -ffp-contract=off (ops/build.py FILE_FLAGS): every product and the sum
// that follows it are rounded separately, as the oracle's separate statements are.
//
// Per element, all in fp64, each operation rounded once:
//   d  = target − double(θ),  q = d·d
//   m' = β1·m + d (sgdm)  |  β1·m + c1·d (adagrad, adam, yogi)
//   v' = v + q (adagrad)  |  β2·v + c2·q (adam)  |  v − (c2·q)·sign(v − q) (yogi; sign ∈ {−1, 0, +1}, 0 for NaN)
//   x  = double(θ) + lr·m' (sgdm)  |  double(θ) + (lr·m') / (sqrt(v') + τ)
//   θ' = fl32(x)
// sqrt and / are the correctly rounded fp64 operations of the device library. A non-finite d gives θ' =
// fl32(target), x = target, and m, v are stored back with the bits that were loaded.
// One kernel templated on (rule, whether x is written). A lane owns 4 consecutive elements: one float4 of θ,
// one double4 of target / m / v (/ x); grid-stride loop under a block cap; the loads of a trip are issued
// before its stores; no LDS, no atomics, one writer per element.
#include "common.h"
#include "dls.h"

namespace {

constexpr int OPT_TPB = 256;
constexpr int OPT_MAX_BLOCKS = 8192;  // grid cap; beyond 8192 · 256 · 4 elements a lane takes another trip

struct OptArgs {
  double lr, beta1, c1, beta2, c2, tau;
};

template <int RULE>
__device__ inline void opt_elem(float& th, double t, double& m, double& v, double& x, const OptArgs& a) {
  const double th64 = (double)th;
  const double d = t - th64;
  if (!(fabs(d) < __builtin_huge_val())) {  // NaN or ±inf: θ' = fl32(target), the state keeps its bits
    x = t;
    th = (float)t;
    return;
  }
  const double q = d * d;
  double m1 = a.beta1 * m;
  if (RULE == SERVER_OPT_SGDM) {
    m1 = m1 + d;
  } else {
    const double g1 = a.c1 * d;
    m1 = m1 + g1;
  }
  double step = a.lr * m1;
  if (RULE != SERVER_OPT_SGDM) {
    double v1;
    if (RULE == SERVER_OPT_ADAGRAD) {
      v1 = v + q;
    } else if (RULE == SERVER_OPT_ADAM) {
      const double bv = a.beta2 * v;
      const double g2 = a.c2 * q;
      v1 = bv + g2;
    } else {
      const double g2 = a.c2 * q;
      const double z = v - q;
      const double sg = z > 0.0 ? 1.0 : z < 0.0 ? -1.0 : 0.0;
      const double gs = g2 * sg;
      v1 = v - gs;
    }
    const double root = sqrt(v1);
    const double den = root + a.tau;
    step = step / den;
    v = v1;
  }
  m = m1;
  x = th64 + step;
  th = (float)x;
}

template <int RULE, bool WITH_X>
__global__ void __launch_bounds__(OPT_TPB) server_opt_kernel(float* __restrict__ theta, const double* __restrict__ target,
                                                             double* __restrict__ m, double* __restrict__ v,
                                                             double* __restrict__ xo, long P4, OptArgs a) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < P4; i += (long)gridDim.x * blockDim.x) {
    float4 th = reinterpret_cast<float4*>(theta)[i];
    const double4 t = reinterpret_cast<const double4*>(target)[i];
    double4 mm = reinterpret_cast<double4*>(m)[i];
    double4 vv = make_double4(0.0, 0.0, 0.0, 0.0);
    if (RULE != SERVER_OPT_SGDM) vv = reinterpret_cast<double4*>(v)[i];
    double4 x;
    opt_elem<RULE>(th.x, t.x, mm.x, vv.x, x.x, a);
    opt_elem<RULE>(th.y, t.y, mm.y, vv.y, x.y, a);
    opt_elem<RULE>(th.z, t.z, mm.z, vv.z, x.z, a);
    opt_elem<RULE>(th.w, t.w, mm.w, vv.w, x.w, a);
    reinterpret_cast<float4*>(theta)[i] = th;
    reinterpret_cast<double4*>(m)[i] = mm;
    if (RULE != SERVER_OPT_SGDM) reinterpret_cast<double4*>(v)[i] = vv;
    if (WITH_X) reinterpret_cast<double4*>(xo)[i] = x;
  }
}

template <int RULE>
void launch_rule(float* theta, const double* target, double* m, double* v, double* x, long P4, const OptArgs& a,
                 hipStream_t s) {
  const int grid = (int)max(1L, min((long)OPT_MAX_BLOCKS, (P4 + OPT_TPB - 1) / OPT_TPB));
  if (x != nullptr)
    hipLaunchKernelGGL((server_opt_kernel<RULE, true>), dim3(grid), dim3(OPT_TPB), 0, s, theta, target, m, v, x, P4, a);
  else
    hipLaunchKernelGGL((server_opt_kernel<RULE, false>), dim3(grid), dim3(OPT_TPB), 0, s, theta, target, m, v, x, P4, a);
}

}  // namespace

int server_opt_max_blocks() { return OPT_MAX_BLOCKS; }

int server_opt_step(float* theta, const double* target, double* m, double* v, double* x, long P, int rule, double lr,
                    double beta1, double c1, double beta2, double c2, double tau, hipStream_t s) {
  if (P <= 0) return 0;
  // (the caller has checked these; a launch that breaks them would write out of bounds or misaligned)
  if (P % 4 != 0 || theta == nullptr || target == nullptr || m == nullptr) return -1;
  if ((rule == SERVER_OPT_SGDM) != (v == nullptr)) return -1;
  const OptArgs a{lr, beta1, c1, beta2, c2, tau};
  switch (rule) {
    case SERVER_OPT_SGDM: launch_rule<SERVER_OPT_SGDM>(theta, target, m, v, x, P / 4, a, s); break;
    case SERVER_OPT_ADAGRAD: launch_rule<SERVER_OPT_ADAGRAD>(theta, target, m, v, x, P / 4, a, s); break;
    case SERVER_OPT_ADAM: launch_rule<SERVER_OPT_ADAM>(theta, target, m, v, x, P / 4, a, s); break;
    case SERVER_OPT_YOGI: launch_rule<SERVER_OPT_YOGI>(theta, target, m, v, x, P / 4, a, s); break;
    default: return -1;
  }
  return 0;
}
