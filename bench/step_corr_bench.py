"""The drift-corrected SGD step (FedProx / SCAFFOLD) on the ResNet-18 layout: three variants of one
local step over [K, P], alternating on one device,

  (a) plain      `hip.sgd_step`                                      (what fed_avg runs),
  (b) corrected  `hip.sgd_step_corrected` with both terms, g' formed in registers,
  (c) two-pass   g' = grad + corr + mu·(θ − anchor) by torch elementwise passes, then `hip.sgd_step`,

momentum 0.9, split weight planes on, all rows active.

    python bench/step_corr_bench.py [--clients 13 50] [--reps 5] [--out profiles/step_corr_bench_mi355x.json]

Prints ONE JSON line (and writes it to --out if given): per cohort size the median (and best) time
of each variant over --reps timed repeats of --iters launches each, the ratios (b)/(a) and (c)/(a),
and the bytes per second of (a) and (b) over the bytes each must move per element — (a) 24 B: θ, g
and momentum read, θ, momentum and the two bf16 planes written; (b) 28 B: the correction row on top
(the shared anchor row, 4 B per element once per launch, is counted once, not per client). (b) and
(c) are also compared bit for bit (the kernel's contract).
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MU = 0.1


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, nargs="+", default=[13, 50])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="launches per timed repeat")
    ap.add_argument("--model", default="ResNet18")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step_corr_bench needs a GPU")

    from distributed_learning_simulator_amd.ops import build

    build.build()
    from distributed_learning_simulator_amd.data.datasets import get_spec
    from distributed_learning_simulator_amd.models.zoo import build_model
    from distributed_learning_simulator_amd.ops import hip

    dev = torch.device("cuda:0")
    layout = build_model(args.model, get_spec("CIFAR10", {})).layout
    P = layout.padded_size
    hyper = (0.0, 0.9, 0.0, False)  # weight decay, momentum, dampening, nesterov
    results = []
    for K in args.clients:
        g = torch.Generator(device=dev).manual_seed(K)
        theta0 = torch.randn(K, P, device=dev, generator=g)
        mom0 = torch.randn(K, P, device=dev, generator=g) * 0.1
        grad = torch.randn(K, P, device=dev, generator=g) * 0.1
        corr = torch.randn(K, P, device=dev, generator=g) * 0.05
        anchor = torch.randn(P, device=dev, generator=g)
        lr = torch.full((K,), 1e-3, device=dev)
        on = torch.ones(K, dtype=torch.bool, device=dev)
        off = torch.zeros(K, dtype=torch.bool, device=dev)
        theta, mom = theta0.clone(), mom0.clone()
        split = torch.zeros((K, 2, P), dtype=torch.bfloat16, device=dev)

        def plain():
            hip.sgd_step(theta, grad, mom, lr, on, *hyper, off, None, split)

        def corrected():
            hip.sgd_step_corrected(theta, grad, mom, lr, on, *hyper, off, MU, anchor, corr, None, split)

        def two_pass():
            gp = grad + corr
            d = theta - anchor
            d *= MU
            gp += d
            hip.sgd_step(theta, gp, mom, lr, on, *hyper, off, None, split)

        # the contract, on this run's operands: (b) has the bits of (c)
        outs = {}
        for key, fn in (("corrected", corrected), ("two_pass", two_pass)):
            theta.copy_(theta0)
            mom.copy_(mom0)
            fn()
            outs[key] = (theta.clone(), mom.clone(), split.clone().view(torch.int16))
        same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int32) if y.dtype == torch.float32 else y)
                   for x, y in zip(outs["corrected"], outs["two_pass"]))
        del outs
        variants = (("plain", plain), ("corrected", corrected), ("two_pass", two_pass))
        t = {k: [] for k, _ in variants}
        for rep in range(args.reps + 1):  # rep 0 warms every variant up
            for key, fn in variants:
                ms = _timed(fn, args.iters)
                if rep:
                    t[key].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        bytes_a = 24 * K * P
        bytes_b = 28 * K * P + 4 * P
        results.append({
            "clients": K,
            "plain_ms": round(med["plain"], 4), "plain_best_ms": round(min(t["plain"]), 4),
            "corrected_ms": round(med["corrected"], 4), "corrected_best_ms": round(min(t["corrected"]), 4),
            "two_pass_ms": round(med["two_pass"], 4), "two_pass_best_ms": round(min(t["two_pass"]), 4),
            "corrected_over_plain": round(med["corrected"] / med["plain"], 3),
            "two_pass_over_plain": round(med["two_pass"] / med["plain"], 3),
            "two_pass_over_corrected": round(med["two_pass"] / med["corrected"], 3),
            "plain_bytes": bytes_a, "corrected_bytes": bytes_b,
            "plain_TBps": round(bytes_a / (med["plain"] * 1e-3) / 1e12, 3),
            "corrected_TBps": round(bytes_b / (med["corrected"] * 1e-3) / 1e12, 3),
            "corrected_equals_two_pass_bitwise": bool(same),
        })
        del theta0, mom0, grad, corr, theta, mom, split
        torch.cuda.empty_cache()
    line = json.dumps({"bench": "step_corr", "model": args.model, "P": P, "num_params": layout.num_params,
                       "mu": MU, "momentum": 0.9, "split_planes": True, "reps": args.reps, "iters": args.iters,
                       "device": torch.cuda.get_device_name(0), "results": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
