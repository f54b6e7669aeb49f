"""Server optimiser step (`fed_avgm`, `fed_adagrad`, `fed_adam`, `fed_yogi`) on the ResNet-18 layout: the
fused kernel of csrc/server_opt.hip (`ops.fl.server_opt_step`) against the torch fp64 elementwise path
for the same step, alternating on one device.

    python bench/server_opt_bench.py [--reps 5] [--inner 20] [--out profiles/server_opt_bench_mi355x.json]

Prints ONE JSON line (and writes it to --out if given): per rule the median (and best) time per launch of
the kernel, of the kernel that also writes the pre-cast fp64 x (what the server stage runs) and of the
torch path (samples of --inner back-to-back launches); the bytes a launch must move against HBM — per
element θ 4 read + 4 written, target 8 read, m 8 + 8, v 8 + 8: 32 B for sgdm, 48 B for the adaptive rules,
8 B more with x — and the rates those imply; and the largest relative difference between the two paths
after one step from the same state (torch's sqrt and its fused multiply-adds round differently, so the
comparison is to 1e-12; bit equality with the oracle is what tests/test_server_opt_gpu.py checks).
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, inner):
    """Milliseconds per launch over `inner` back-to-back launches between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def torch_step(theta, target, m, v, rule, lr, beta1, beta2, tau):
    """The same step as separate torch fp64 elementwise operations (no non-finite rule)."""
    th = theta.double()
    d = target - th
    if rule == "sgdm":
        m.mul_(beta1).add_(d)
        x = th + lr * m
    else:
        q = d * d
        m.mul_(beta1).add_(d, alpha=1.0 - beta1)
        if rule == "adagrad":
            v.add_(q)
        elif rule == "adam":
            v.mul_(beta2).add_(q, alpha=1.0 - beta2)
        else:
            v.sub_((1.0 - beta2) * q * torch.sign(v - q))
        x = th + lr * m / (v.sqrt() + tau)
    theta.copy_(x)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="launches per timed sample")
    ap.add_argument("--model", default="ResNet18")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("server_opt_bench needs a GPU")

    from distributed_learning_simulator_amd.ops import build

    build.build()
    from distributed_learning_simulator_amd.data.datasets import get_spec
    from distributed_learning_simulator_amd.models.zoo import build_model
    from distributed_learning_simulator_amd.ops import fl, ref

    dev = torch.device("cuda:0")
    layout = build_model(args.model, get_spec("CIFAR10", {})).layout
    P = layout.padded_size
    valid = layout.valid_mask(dev)
    beta1, beta2, tau = 0.9, 0.99, 1e-3
    results = []
    for rule in ref.SERVER_OPT_RULES:
        lr = 1.0 if rule == "sgdm" else 0.01
        g = torch.Generator(device=dev).manual_seed(ref.SERVER_OPT_RULES.index(rule))
        theta0 = torch.randn(P, device=dev, generator=g) * 0.05 * valid
        target = theta0.double() + torch.randn(P, device=dev, generator=g, dtype=torch.float64) * 1e-3 * valid
        adaptive = rule != "sgdm"

        def fresh():
            return (theta0.clone(), torch.zeros(P, dtype=torch.float64, device=dev),
                    torch.full((P,), tau * tau, dtype=torch.float64, device=dev) if adaptive else None)

        # one step from the same state on both paths: how far apart they are
        a, b = fresh(), fresh()
        xa = torch.empty(P, dtype=torch.float64, device=dev)
        fl.server_opt_step(a[0], target, a[1], a[2], rule, lr, beta1, beta2, tau, x_out=xa)
        xb = torch_step(b[0], target, b[1], b[2], rule, lr, beta1, beta2, tau)
        rel = {"x": ((xa - xb).abs().max() / xb.abs().max()).item(),
               "m": ((a[1] - b[1]).abs().max() / b[1].abs().max()).item()}
        if adaptive:
            rel["v"] = ((a[2] - b[2]).abs().max() / b[2].abs().max()).item()

        # the timed launches step in place, as over the rounds of a run (same target: θ settles on it)
        k, kx, t = fresh(), fresh(), fresh()
        x = torch.empty(P, dtype=torch.float64, device=dev)
        steps = {
            "kernel": lambda: fl.server_opt_step(k[0], target, k[1], k[2], rule, lr, beta1, beta2, tau),
            "kernel_with_x": lambda: fl.server_opt_step(kx[0], target, kx[1], kx[2], rule, lr, beta1, beta2, tau, x_out=x),
            "torch": lambda: torch_step(t[0], target, t[1], t[2], rule, lr, beta1, beta2, tau),
        }
        ms = {key: [] for key in steps}
        for rep in range(args.reps + 1):  # rep 0 warms every path up
            for key, fn in steps.items():  # alternating: every path once per repetition
                sample = _timed(fn, args.inner)
                if rep:
                    ms[key].append(sample)
        med = {key: statistics.median(vals) for key, vals in ms.items()}
        per_elem = 48 if adaptive else 32
        nbytes = {"kernel": per_elem * P, "kernel_with_x": (per_elem + 8) * P}
        results.append({
            "rule": rule,
            **{f"{key}_ms": round(val, 4) for key, val in med.items()},
            **{f"{key}_best_ms": round(min(vals), 4) for key, vals in ms.items()},
            "speedup_vs_torch": round(med["torch"] / med["kernel"], 2),
            "bytes_per_element": per_elem,
            **{f"{key}_bytes": val for key, val in nbytes.items()},
            **{f"{key}_GBps": round(val / (med[key] * 1e-3) / 1e9, 1) for key, val in nbytes.items()},
            **{f"max_rel_diff_{key}": val for key, val in rel.items()},
            "paths_agree": bool(all(val < 1e-12 for val in rel.values())),
            "finite": bool(torch.isfinite(k[0]).all() and torch.isfinite(t[0]).all()),
        })
        steps = k = kx = t = a = b = x = xa = xb = None
        torch.cuda.empty_cache()
    line = json.dumps({"bench": "server_opt", "model": args.model, "P": P, "num_params": layout.num_params,
                       "reps": args.reps, "launches_per_sample": args.inner,
                       "device": torch.cuda.get_device_name(0), "results": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
