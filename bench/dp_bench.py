"""DP-FedAvg aggregation (`fed_dp_avg`) on the ResNet-18 layout: the three kernels of csrc/dp.hip
(`ops.fl.row_sq_norms`, `clipped_sum`, `gaussian_add`) against the torch path on the same rows —
`rows.double().square().sum(1)`, the clip factors, `fl.weighted_sum` with them, `torch.randn(P,
dtype=float64)` scaled and added — and against the plain `fl.weighted_sum` FedAvg runs, alternating
on one device.

    python bench/dp_bench.py [--clients 13 50] [--reps 5] [--out profiles/dp_bench_mi355x.json]

Prints ONE JSON line (and writes it to --out if given): per cohort size K the median (and best) time
per launch of each kernel and of each torch step (samples of --inner back-to-back launches), the
bytes each kernel must move against HBM (norms: 4·K·P read; clipped sum: 4·K·P read + 8·P read + 8·P
written; noise: 8·P read + 8·P written + P mask bytes) and the rates those imply, and the largest
relative difference between the two paths' norms and sums (torch adds in its own order and fuses, so
the comparison is to 1e-12; bit equality with the ordered oracle is what tests/test_dp_gpu.py checks).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, nargs="+", default=[13, 50])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="launches per timed sample")
    ap.add_argument("--model", default="ResNet18")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dp_bench needs a GPU")

    from distributed_learning_simulator_amd.ops import build

    build.build()
    from distributed_learning_simulator_amd.data.datasets import get_spec
    from distributed_learning_simulator_amd.models.zoo import build_model
    from distributed_learning_simulator_amd.ops import fl

    dev = torch.device("cuda:0")
    layout = build_model(args.model, get_spec("CIFAR10", {})).layout
    P = layout.padded_size
    valid = layout.valid_mask(dev)
    mask = valid.to(torch.uint8)
    std, seed = 0.5, 1234
    results = []
    for K in args.clients:
        g = torch.Generator(device=dev).manual_seed(K)
        rows = torch.randn(K, P, device=dev, generator=g) * 1e-2 * valid
        rows *= torch.linspace(0.5, 2.0, K, device=dev)[:, None]  # norms on both sides of the clip
        clip = float(rows.double().norm(dim=1).median())
        ones = torch.ones(K, dtype=torch.float64, device=dev)
        nsq = torch.empty(K, dtype=torch.float64, device=dev)
        acc = torch.zeros(P, dtype=torch.float64, device=dev)
        fl.row_sq_norms(rows, out=nsq)

        def torch_scale():
            norm = t_nsq.sqrt()
            return torch.where(norm > clip, clip / norm, torch.ones_like(norm))

        # every step accumulates in place, as in a round (the accumulator just keeps growing)
        steps = {
            "norms": lambda: fl.row_sq_norms(rows, out=nsq),
            "clipped_sum": lambda: fl.clipped_sum(rows, nsq, clip, out=acc),
            "gaussian_add": lambda: fl.gaussian_add(acc, std, seed, 1, mask),
            "torch_norms": lambda: rows.double().square().sum(1),
            "torch_scaled_sum": lambda: fl.weighted_sum(rows, torch_scale(), acc),
            "torch_randn_add": lambda: acc.add_(torch.randn(P, dtype=torch.float64, device=dev) * std),
            "weighted_sum": lambda: fl.weighted_sum(rows, ones, acc),
        }
        t_nsq = steps["torch_norms"]()
        ref = {"norms": nsq.clone(), "torch_norms": t_nsq,
               "clipped_sum": fl.clipped_sum(rows, nsq, clip), "torch_scaled_sum": fl.weighted_sum(rows, torch_scale())}
        t = {k: [] for k in steps}
        for rep in range(args.reps + 1):  # rep 0 warms every path up
            for key, fn in steps.items():  # alternating: every step once per repetition
                ms = _timed(fn, args.inner)
                if rep:
                    t[key].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        rel_n = ((ref["norms"] - ref["torch_norms"]).abs() / ref["torch_norms"]).max().item()
        rel_s = ((ref["clipped_sum"] - ref["torch_scaled_sum"]).abs().max() / ref["torch_scaled_sum"].abs().max()).item()
        nbytes = {"norms": 4 * K * P, "clipped_sum": 4 * K * P + 16 * P, "gaussian_add": 16 * P + P,
                  "weighted_sum": 4 * K * P + 16 * P}
        dp_ms = med["norms"] + med["clipped_sum"] + med["gaussian_add"]
        torch_ms = med["torch_norms"] + med["torch_scaled_sum"] + med["torch_randn_add"]
        results.append({
            "clients": K,
            **{f"{k}_ms": round(v, 4) for k, v in med.items()},
            **{f"{k}_best_ms": round(min(v), 4) for k, v in t.items()},
            "dp_kernels_ms": round(dp_ms, 4), "torch_path_ms": round(torch_ms, 4),
            "speedup_vs_torch_path": round(torch_ms / dp_ms, 2),
            "dp_over_weighted_sum": round(dp_ms / med["weighted_sum"], 2),
            **{f"{k}_bytes": v for k, v in nbytes.items()},
            **{f"{k}_GBps": round(v / (med[k] * 1e-3) / 1e9, 1) for k, v in nbytes.items()},
            "gaussian_Gdraws_per_s": round(P / (med["gaussian_add"] * 1e-3) / 1e9, 2),
            "max_rel_diff_norms": rel_n, "max_rel_diff_sum": rel_s, "paths_agree": bool(rel_n < 1e-12 and rel_s < 1e-12),
        })
        del ref, rows
        torch.cuda.empty_cache()
    line = json.dumps({"bench": "dp", "model": args.model, "P": P, "num_params": layout.num_params,
                       "reps": args.reps, "launches_per_sample": args.inner,
                       "device": torch.cuda.get_device_name(0), "results": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
