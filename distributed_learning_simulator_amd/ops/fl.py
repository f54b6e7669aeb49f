"""FL-level fused primitives over flat client-stacked buffers (backend-dispatched).

| primitive            | replaces (reference)                                           |
|----------------------|----------------------------------------------------------------|
| sgd_step             | torch.optim.SGD.step per client (K2), GradientWorker step (K3) |
| sgd_step_corrected   | — (FedProx / SCAFFOLD local step: g + (c − c_i) + μ(θ − θ_g))    |
| adam_step            | torch.optim.Adam.step per client                                |
| broadcast_rows       | load_parameters of θ_g into every client (`util/model.py:6-23`)|
| delta_rows           | ModelCache.get_parameter_diff (K4, `util/model_cache.py:30-36`)|
| weighted_sum         | FedAVGAlgorithm accumulate (K6, `fed_avg_algorithm.py:39-52`)  |
| trimmed_sum          | — (robust aggregation: trimmed mean / median, Yin et al. 2018)  |
| pairwise_sq_dists    | — (Krum / Multi-Krum distances, Blanchard et al. 2017)           |
| row_sq_norms         | — (DP-FedAvg per-client L2 norms, McMahan et al. 2018)           |
| clipped_sum          | — (DP-FedAvg clipped fp64 accumulation)                          |
| gaussian_add         | — (DP-FedAvg Gaussian mechanism, Philox4x32-10 + Box-Muller)     |
| server_opt_step      | — (FedAvgM / FedAdagrad / FedAdam / FedYogi server step, Reddi 2021)|
| secagg_mask_rows     | — (secure aggregation: fixed-point upload + pairwise masks, Bonawitz 2017) |
| ring_sum / ring_unmask / ring_decode | — (secure aggregation: the server's Z_{2^32} sum and unmasking) |
| mix_rows             | Shapley subset models (K8, `aggregation_algorithm.py:30-50`)   |
| masked_weighted_sum  | FedDropoutAvg aggregation (K10, `fed_dropout_avg/algorithm.py`)|
| dropout_mask         | FedDropoutAvg Bernoulli mask (K9, `fed_dropout_avg/worker.py`) |
| block_sq_norms       | OBD per-block ‖Δ‖ (K11, `obd_algorithm.py:129-145`)            |
| qsgd_quant/dequant   | stochastic quantisation (K13, `quantized_endpoint.py:74-83`)   |
| nnadq_quant/dequant  | NNADQ (K14, `quantized_endpoint.py:86-116`)                    |
| sign_pack / vote     | sign-SGD 1-bit exchange (M9/M10)                                |
"""

from __future__ import annotations

import math

import torch

from . import backend, ref


def sgd_step(theta, grad, mom, lr, active, first_step, weight_decay=0.0, momentum=0.0,
             dampening=0.0, nesterov=False, shadow=None, split=None):
    be = backend.get(theta)
    be.sgd_step(theta, grad, mom, lr, active, weight_decay, momentum, dampening, nesterov,
                first_step, shadow, split)


def sgd_step_seg(theta, grad, mom, lr, active, first_step, weight_decay, momentum, dampening, nesterov, split,
                 seg_table):
    """sgd_step over the spans of `seg_table` only (the rest stepped in their wgrad kernels)."""
    backend.get(theta).sgd_step_seg(theta, grad, mom, lr, active, weight_decay, momentum, dampening, nesterov,
                                    first_step, split, seg_table)


def sgd_step_corrected(theta, grad, mom, lr, active, first_step, weight_decay, momentum, dampening, nesterov, mu,
                       anchor, corr, shadow=None, split=None):
    """The SGD step of `sgd_step` on the drift-corrected gradient of FedProx (mu > 0, corr None) and
    SCAFFOLD (mu = 0, corr[k] = c − c_i); per active row k and element p

      g1 = fl32(g + corr[k, p])                                   (corr None: g1 = g)
      g2 = fl32(g1 + fl32(mu · fl32(θ[k, p] − anchor[p])))        (mu == 0: g2 = g1)
      θ, m ← the `sgd_step` arithmetic on g2 (weight decay, momentum, nesterov after the correction)

    every operation of the first two lines rounded to fp32 once, nothing contracted into an FMA.
    Contract: θ, momentum, `shadow` and the `split` planes have the bits of materialising g' with
    separate fp32 elementwise operations (`grad + corr`, `theta − anchor`, `· mu`, `+`) and calling
    `sgd_step` on it; g' itself is never written, and `grad`, `corr` [K, P] fp32 (its own row stride
    ≥ P) and `anchor` [P] fp32 (shared by all rows, required when mu != 0) are read-only. Inactive
    rows, `first_step`, per-row `lr`, row strides ≥ P and P % 16 == 0 behave as in `sgd_step`.
    Kernel: csrc/elementwise.hip sgd_corr_kernel; oracle and CPU path: ops/ref.py."""
    backend.get(theta).sgd_step_corrected(theta, grad, mom, lr, active, weight_decay, momentum, dampening, nesterov,
                                          first_step, mu, anchor, corr, shadow, split)


def split_rows(theta, split):
    """Refresh the pre-split (hi, lo) bf16 weight planes of θ rows (fp32 GEMM operand)."""
    backend.get(theta).split_rows(theta, split)


def adam_step(theta, grad, m, v, lr, active, step, beta1=0.9, beta2=0.999, eps=1e-8,
              weight_decay=0.0, shadow=None):
    be = backend.get(theta)
    be.adam_step(theta, grad, m, v, lr, active, step, beta1, beta2, eps, weight_decay, shadow)


def broadcast_rows(theta_rows, src, shadow_rows=None):
    """theta_rows[k,:] = src for every row (and bf16 shadow)."""
    be = backend.get(theta_rows)
    if be is ref:
        theta_rows.copy_(src.unsqueeze(0).expand_as(theta_rows))
        if shadow_rows is not None:
            shadow_rows.copy_(theta_rows.to(shadow_rows.dtype))
    else:
        be.broadcast_rows(theta_rows, src, shadow_rows)


def delta_rows(theta_rows, base, out=None):
    be = backend.get(theta_rows)
    if be is ref:
        d = theta_rows - base.unsqueeze(0)
        if out is None:
            return d
        out.copy_(d)
        return out
    return be.delta_rows(theta_rows, base, out)


def weighted_sum(x, w, out=None):
    """out (fp64 [P]; zeros if None) += Σ_k w_k x[k,:], fp64 accumulation. Returns `out`."""
    return backend.get(x).weighted_sum(x, w, out)


def trimmed_sum(x, b: int, out=None):
    """fp64 [P] coordinate-wise trimmed sum of the rows of x [n, P]: per column the n values sorted
    by the signed key bits ^ ((bits >> 31) & 0x7fffffff), the b lowest and b highest dropped, the
    other n − 2b added as doubles in ascending order from +0.0 (b = 0: the unweighted sum; b =
    (n − 1) // 2: the median times 1 or 2). NaN and ±inf uploads are just extreme values. 1 ≤ n ≤
    512 and 0 ≤ 2b < n, else ValueError. The kernel and the oracle agree bit for bit."""
    return backend.get(x).trimmed_sum(x, b, out)


def pairwise_sq_dists(x, out=None):
    """fp64 [n, n] squared L2 distances between the rows of x [n, P] fp32 (row stride ≥ P), the hot
    path of Krum / Multi-Krum (csrc/krum.hip; oracle and CPU path ops/ref.py).

    term(i, j, p) = fl64(d · d) with d = fl64(double(x[i, p]) − double(x[j, p])); the multiply and the
    add that follows are rounded separately (no FMA); denormal inputs are not flushed. D[i, j] adds
    the terms in an order fixed by the column index alone: the columns are cut into spans of W =
    ref.PAIR_SPAN = 4096 columns (the last may be shorter) and the spans into groups of G =
    ref.PAIR_GROUP = 8 consecutive spans;
      span sum  = the span's terms added one at a time in ascending column order from +0.0,
      group sum = the group's span sums added in ascending span order from +0.0,
      D[i, j]   = the group sums added in ascending group order from +0.0.
    Nothing depends on n, the row order, the launch geometry, the device or the rank count: D[i, i]
    is +0.0 for a finite row, D[i, j] and D[j, i] have the same bits, a row permutation permutes D,
    zero columns change nothing, D is finite where both rows are, NaN / ±inf follow IEEE (NaN payload
    bits are not part of the contract). No float atomics: bitwise reproducible, and the kernel and
    the oracle agree bit for bit. 1 ≤ n ≤ 512, else ValueError."""
    return backend.get(x).pairwise_sq_dists(x, out)


def krum_select(D, f: int, m: int, ids) -> list:
    """Row indices (sorted by client id) of the m uploads with the smallest (Krum score, client id):
    the score of row i is the sum of its k = clamp(n − f − 2, 1, n − 1) smallest D[i, j], j ≠ i,
    added in ascending order in fp64 (non-finite distances count as +inf; n = 1 scores 0). n < 2f + 3
    falls back to f = max(0, (n − 3) // 2) with a warning; m is clamped to [1, n]. D is copied to
    the host and the same code runs for both backends (`ops.ref.krum_select`)."""
    return ref.krum_select(D, f, m, ids)


def krum_scores(D, f: int):
    """(fp64 [n] Krum scores on the host, the f actually used): see `krum_select`."""
    return ref.krum_scores(D, f)


def row_sq_norms(x, out=None):
    """fp64 [n] squared L2 norms of the rows of x [n, P] fp32 (row stride ≥ P, 16-B aligned rows), the
    first pass of DP-FedAvg clipping (csrc/dp.hip; oracle and CPU path ops/ref.py).

    term(k, p) = fl64(double(x[k, p]) · double(x[k, p])): the product is exact, a 24-bit mantissa
    squared fits in 53 bits. The terms are added in the order `pairwise_sq_dists` defines: the columns
    are cut into spans of W = ref.PAIR_SPAN = 4096 columns (the last may be shorter) and the spans into
    groups of G = ref.PAIR_GROUP = 8 consecutive spans;
      span sum  = the span's terms added one at a time in ascending column order from +0.0,
      group sum = the group's span sums added in ascending span order from +0.0,
      out[k]    = the group sums added in ascending group order from +0.0.
    Denormal inputs are not flushed. Nothing depends on n, the launch geometry, the device or the rank:
    out[k] has the bits of pairwise_sq_dists(stack([x[k], zeros]))[0, 1], zero columns change nothing,
    a finite row whose sum does not overflow gives a finite norm, NaN / ±inf follow IEEE (NaN payload
    bits are not part of the contract). No float atomics: bitwise reproducible, and the kernel and the
    oracle agree bit for bit. Written into out[:n] if given."""
    return backend.get(x).row_sq_norms(x, out)


def clip_scales(nsq, clip):
    """(s fp64 [n], rejected bool [n]): the per-row factors of L2 clipping to `clip` > 0 from the squared
    norms nsq fp64 [n] (`row_sq_norms`).

      norm = sqrt(nsq);  s = clip / norm if norm > clip, else exactly 1.0;
      a non-finite nsq gives s = 0 and rejected = True — NaN or ±inf in the row, or a finite row
      whose square sum overflows.
    sqrt, the comparison and the division are correctly rounded IEEE operations, so both backends give
    the same bits, and s · norm ≤ clip · (1 + 2^-52). `clipped_sum` forms the same factors on the
    device; this function makes the rule observable."""
    return backend.get(nsq).clip_scales(nsq, clip)


def clipped_sum(x, nsq, clip, out=None):
    """out (fp64 [≥ P]; zeros [P] if None)[:P] += Σ_k s_k · x[k, :] over the rows of x [n, P] fp32, with
    (s, rejected) = clip_scales(nsq, clip): for rows in ascending k,

      out[p] = fl64(out[p] + fl64(s_k · double(x[k, p])))

    multiply and add rounded separately (no FMA; csrc/dp.hip is compiled with contraction off).
    Rejected rows are skipped, not multiplied: 0 · NaN would poison the sum. An unclipped row (s_k =
    1.0) adds double(x) exactly. s_k is formed on the device from `nsq` and `clip`: no host read
    between `row_sq_norms` and this call. `out` accumulates in place across calls (waves, cohorts);
    out[P:] is untouched; x and nsq are read-only. The kernel and the oracle agree bit for bit.
    Returns `out`."""
    return backend.get(x).clipped_sum(x, nsq, clip, out)


def gaussian_add(acc, std: float, seed: int, stream: int, mask=None):
    """acc (fp64 [P]) [p] += fl64(std · z[p]) for every p with mask[p] != 0 (`mask`: uint8 / bool [P], e.g.
    the layout's valid_mask; None: every p). Masked-out elements are not written; std == 0 writes
    nothing at all. seed: 64-bit int, stream: 32-bit int (the round number).

    z is Box-Muller on Philox4x32-10 (Random123: multipliers 0xD2511F53, 0xCD9E8D57, Weyl increments
    0x9E3779B9, 0xBB67AE85) with key (seed & 0xffffffff, seed >> 32) and, for the pair index i = p // 2,
    counter (i & 0xffffffff, i >> 32, stream, 0x44503031); the output words w0..w3 give
      u1 = (((w0 >> 5) << 26) + (w1 >> 6) + 1) · 2^-53 in (0, 1],
      u2 = (((w2 >> 5) << 26) + (w3 >> 6)) · 2^-53 in [0, 1),
      r = sqrt(−2 · log(u1)), φ = fl64(2π · u2), z[2i] = r · cos φ, z[2i + 1] = r · sin φ, all in fp64.
    z depends on (seed, stream, p) only: the same on every rank, in every launch geometry, across
    waves. The integer stage is exact on both backends; log, cos and sin come from two different
    libms, a few ulp apart, and r ≤ sqrt(2 · 53 · ln 2) = 8.57, so |z_kernel − z_oracle| ≲ 1.2e-14 (the
    tests bound it by 1e-13). Returns `acc`."""
    if float(std) == 0.0:
        return acc
    return backend.get(acc).gaussian_add(acc, float(std), int(seed), int(stream), mask)


def server_opt_step(theta, target, m, v, rule, lr, beta1=0.9, beta2=0.99, tau=1e-3, x_out=None):
    """One step of a server optimiser on the pseudo-gradient d = target − θ (FedAvgM, Hsu et al. 2019;
    FedAdagrad / FedAdam / FedYogi, Reddi et al. 2021, no bias correction). theta fp32 [P] is θ_t and
    becomes θ_{t+1} in place; target fp64 [≥ P] is what the aggregation produced (read-only, target[P:]
    is not read); m, v fp64 [P] are the state, updated in place (v is None for `sgdm`); x_out (fp64 [P],
    optional) receives the pre-cast x. rule ∈ `ref.SERVER_OPT_RULES`. c1 = 1.0 − beta1 and c2 = 1.0 −
    beta2 are formed here, once, in python doubles, and passed to both backends. Per element p:

      d  = target[p] − double(θ[p])
      q  = d·d
      m' = β1·m + d                      (sgdm)
      m' = β1·m + c1·d                   (adagrad, adam, yogi)
      v' = v + q                         (adagrad)
      v' = β2·v + c2·q                   (adam)
      v' = v − (c2·q)·sign(v − q)        (yogi; sign is −1, 0 or +1 and 0 for 0 and NaN: the product is exact)
      x  = double(θ) + lr·m'             (sgdm)
      x  = double(θ) + (lr·m') / (sqrt(v') + τ)    (adagrad, adam, yogi)
      θ'[p] = fl32(x)                    (round to nearest even, overflow to ±inf)

    Every operation is an fp64 operation rounded once; nothing is contracted into an FMA
    (csrc/server_opt.hip is compiled with contraction off); sqrt and / are the correctly rounded IEEE
    operations; denormals are not flushed. A non-finite d (NaN or ±inf in target[p] or θ[p]) gives θ'[p]
    = fl32(target[p]) and x = target[p], and m[p], v[p] keep their bits: the poisoned coordinate shows
    in θ as it does under plain aggregation, the state is not poisoned for good. Layout padding (θ =
    +0, target = +0) keeps +0 bits. Nothing outside [0, P) of any buffer is written. P % 4 == 0, theta
    16-B aligned, the fp64 buffers 32-B aligned; an unknown rule, a non-finite lr / β / τ, β outside [0,
    1), τ ≤ 0 for an adaptive rule or a misplaced operand raises ValueError before any launch. No
    atomics, one writer per element: two launches give the same bits, and the kernel and the oracle
    (`ops.ref.server_opt_step`, also the CPU path) agree bit for bit on θ', m', v' and x (NaN payload
    bits are not part of the contract). Returns `theta`."""
    rule, lr, beta1, beta2, tau = ref.check_server_opt(rule, lr, beta1, beta2, tau)
    c1, c2 = 1.0 - beta1, 1.0 - beta2
    return backend.get(theta).server_opt_step(theta, target, m, v, rule, lr, beta1, beta2, tau, c1, c2, x_out)


def secagg_frac_bits(R, m: int, f=None):
    """(R as fp32, f): the fixed-point code of secure aggregation for the range R and the fixed cohort size m.
    R must be finite and > 0 (rounded to fp32 once; the bound uses the rounded value). f is the given
    `f`, else the largest integer with m · R · 2^f ≤ 2^31 − 1. ValueError if a given f breaks that bound,
    or if f would be below 1."""
    return ref.secagg_frac_bits(R, m, f)


def secagg_mask_words(key: int, P: int, start: int = 0, device=None):
    """int64 [P]: the mask words w(κ, p) for p = start .. start + P − 1, unsigned 32-bit values. For the
    Philox call index i = p // 4, w(κ, p) is word p % 4 of Philox4x32-10 with key (κ & 0xffffffff, κ >> 32)
    and counter (i & 0xffffffff, i >> 32, 0, 0x53413031). w depends on (κ, p) alone. (torch; the kernels
    expand the same stream in registers.)"""
    return ref.secagg_mask_words(key, P, start, device)


def secagg_mask_rows(x, entries, R, f: int, out=None, variant: int | None = None):
    """The masked upload of secure aggregation (Bonawitz et al. 2017): (out int32 [K, P], stats int32 [K, 2]).

    x: fp32 [K, P], row stride ≥ P, rows 16-B aligned, P % 4 == 0, 1 ≤ K ≤ 512. entries = (offsets, keys,
    signs): row k owns the entries offsets[k] .. offsets[k + 1] − 1 of the flat lists keys (unsigned 64-bit
    python ints κ) and signs (+1 / −1); a row may have none, at most 512. R, f: `secagg_frac_bits` with the
    op's own bound R · 2^f ≤ 2^31 − 1.

      q(x)      t = x clamped to [−R, R] in fp32 (±inf clamp to ±R); q = rint(fl64(t) · 2^f), ties to even.
                Scaling by a power of two is exact in fp64: one rounding. A NaN gives q = 0.
      w(κ, p)   `secagg_mask_words`.
      out[k, p] = the low 32 bits of q(x[k, p]) + Σ_e sign_e · w(κ_e, p), read as int32.
      stats[k]  = (elements with |x| > R, infinities included; NaN elements).

    `out` may be the memory of x (x.view(torch.int32)): the upload overwrites the delta rows. Masks are
    drawn at every position of the padded layout; padding holds x = 0 and cancels like everything else.
    All of it is integer arithmetic in Z_{2^32}: no summation order, no contraction flag, no tolerance —
    the kernel (csrc/secagg.hip) and the oracle (`ops.ref.secagg_mask_rows`, also the CPU path) give the
    same integers. `variant` selects another ILP form of the kernel's expander (benchmarks): same bits.
    A wrong dtype, shape, stride, alignment or entry table raises ValueError before anything is written."""
    offsets, keys, signs = entries
    be = backend.get(x)
    if be is ref:
        return ref.secagg_mask_rows(x, offsets, keys, signs, R, f, out)
    return be.secagg_mask_rows(x, offsets, keys, signs, R, f, out, variant)


def ring_sum(rows, acc):
    """acc (int64 [P], 16-B aligned) [p] += Σ_k (int64) rows[k, p] over int32 rows [K, P] (row stride ≥ P,
    sign-extended). With K ≤ 512 rows a call there is no int64 overflow and the low 32 bits are the sum
    in Z_{2^32}: exact, so any order and any split over calls or ranks gives the same bits. Returns acc."""
    return backend.get(acc).ring_sum(rows, acc)


def ring_unmask(acc, entries, variant: int | None = None):
    """acc (int64 [P]) [p] −= Σ_e sign_e · (int64) w(κ_e, p) over one flat entry list entries = (keys, signs)
    of at most 512 · 512 entries (no overflow): the server's removal of the self masks of the clients
    that reported and of the pair masks of those that dropped. Returns acc."""
    keys, signs = entries
    be = backend.get(acc)
    if be is ref:
        return ref.ring_unmask(acc, keys, signs)
    return be.ring_unmask(acc, keys, signs, variant)


def ring_decode(acc, f: int):
    """fp64 [P]: v · 2^−f, v = the low 32 bits of acc[p] as a signed int32 — exact. P-sized, once a round:
    torch elementwise on both backends."""
    return ref.ring_decode(acc, f)


def mix_rows(x, w, out_dtype):
    """Rows of W[M, K] · x[K, P] in `out_dtype`: M weighted combinations of the K client rows
    in one pass (Shapley subset models, K8)."""
    return backend.get(x).mix_rows(x, w, out_dtype)


def masked_weighted_sum(x, mask, w, num=None, den=None):
    """(num, den) fp64 [P] += (Σ_k w_k m_k x_k, Σ_k w_k m_k)."""
    return backend.get(x).masked_weighted_sum(x, mask, w, num, den)


# ------------------------------------------------------------------ compression ops
def philox_uniform(shape, seed: int, offset: int, device) -> torch.Tensor:
    """Counter-based uniform [0,1) keyed by (seed, offset): identical on every rank and
    every backend (ref implementation mirrors the kernel's hash)."""
    n = int(math.prod(shape))
    idx = torch.arange(n, device=device, dtype=torch.int64) + offset
    h = _mix(idx, seed)
    return (h.float() * (1.0 / 4294967296.0)).reshape(shape)


def _mix(x: torch.Tensor, seed: int) -> torch.Tensor:
    m = 0xFFFFFFFF
    x = (x ^ ((seed * 0x9E3779B9) & m)) & m
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & m
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & m
    x = x ^ (x >> 16)
    return x


def row_seeds(seed: int, keys: list[int]) -> list[int]:
    """Per-row 32-bit seeds derived from (seed, CLIENT id): masks and rounding noise do not
    depend on which rank / wave / row hosts a client, so 1-GPU and N-GPU runs agree."""
    out = []
    for k in keys:
        h = (seed * 0x9E3779B1 + (k + 1) * 0x85EBCA77 + 0x27D4EB2F) & 0xFFFFFFFF
        h ^= h >> 15
        h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
        h ^= h >> 12
        out.append(h)
    return out


def uniform_rows(seeds: list[int], P: int, device) -> torch.Tensor:
    """[K, P] uniforms u[k, i] = hash(i, seeds[k]) (identical to the kernels' mix32)."""
    idx = torch.arange(P, device=device, dtype=torch.int64)
    return torch.stack([(_mix(idx, s).float() * (1.0 / 4294967296.0)) for s in seeds])


def dropout_mask(shape, p: float, seeds: list[int], device) -> torch.Tensor:
    """Bernoulli(1-p) keep-mask [K,P]; row k keyed by seeds[k]."""
    be = backend.get(torch.empty(0, device=device))
    if be is ref:
        return uniform_rows(seeds, shape[1], device) >= p
    return be.dropout_mask(shape, p, seeds)


def block_sq_norms(x, block_offsets, block_ids):
    """Per-(client, block) Σ x² for segments. x [K,P]; block_ids [P] int (−1 = padding).
    Returns [K, nblocks] fp32."""
    be = backend.get(x)
    if be is ref:
        nb = int(block_offsets.numel()) - 1
        out = torch.zeros((x.shape[0], nb), dtype=torch.float32, device=x.device)
        valid = block_ids >= 0
        out.index_add_(1, block_ids[valid].long(), (x[:, valid].float() ** 2))
        return out
    return be.block_sq_norms(x, block_offsets, block_ids)
