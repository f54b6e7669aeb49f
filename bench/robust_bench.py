"""Coordinate-wise trimmed sum on the ResNet-18 layout: the kernel (`ops.fl.trimmed_sum`,
csrc/robust.hip) against the torch path (`torch.sort(rows, dim=0)`, slice, fp64 sum) on the same
rows, alternating on one device.

    python bench/robust_bench.py [--clients 13 50 100] [--trim 0.1] [--reps 5]

Per cohort size n it times the trimmed mean's b = ⌊trim · n⌋ and the median's b = (n − 1) // 2.
Prints ONE JSON line: per (n, b) the median (and best) time of both paths, the kernel's achieved
GB/s over the bytes it must move (n·P·4 read once + 8P written), and whether both paths gave the
same sums (the torch path adds in torch's reduction order, so the comparison is to 1e-12 relative;
bit equality with the ordered oracle is what tests/test_robust.py checks).
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, nargs="+", default=[13, 50, 100])
    ap.add_argument("--trim", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model", default="ResNet18")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("robust_bench needs a GPU")

    from distributed_learning_simulator_amd.ops import build

    build.build()
    from distributed_learning_simulator_amd.data.datasets import get_spec
    from distributed_learning_simulator_amd.models.zoo import build_model
    from distributed_learning_simulator_amd.ops import fl

    dev = torch.device("cuda:0")
    layout = build_model(args.model, get_spec("CIFAR10", {})).layout
    P = layout.padded_size
    valid = layout.valid_mask(dev)
    results = []
    for n in args.clients:
        g = torch.Generator(device=dev).manual_seed(n)
        rows = torch.randn(n, P, device=dev, generator=g) * 1e-2 * valid
        out = torch.empty(P, dtype=torch.float64, device=dev)
        for name, b in (("trimmed_mean", int(args.trim * n)), ("median", (n - 1) // 2)):

            def kernel():
                return fl.trimmed_sum(rows, b, out=out)

            def torch_path():
                return torch.sort(rows, dim=0).values[b : n - b].sum(dim=0, dtype=torch.float64)

            t = {"kernel": [], "torch": []}
            ref = {}
            for rep in range(args.reps + 1):  # rep 0 warms both paths up
                for key, fn in (("kernel", kernel), ("torch", torch_path)):
                    ms, res = _timed(fn)
                    if rep:
                        t[key].append(ms)
                    else:
                        ref[key] = res.clone()
            scale = ref["torch"].abs().max().clamp(min=1e-300)
            rel = ((ref["kernel"] - ref["torch"]).abs().max() / scale).item()
            med = {k: statistics.median(v) for k, v in t.items()}
            nbytes = n * P * 4 + 8 * P
            results.append({
                "clients": n, "method": name, "b": b,
                "kernel_ms": round(med["kernel"], 3), "kernel_best_ms": round(min(t["kernel"]), 3),
                "torch_sort_ms": round(med["torch"], 3), "torch_sort_best_ms": round(min(t["torch"]), 3),
                "kernel_GBps": round(nbytes / (med["kernel"] * 1e-3) / 1e9, 1),
                "speedup": round(med["torch"] / med["kernel"], 2),
                "sums_max_rel_diff": rel, "sums_equal": bool(rel < 1e-12),
            })
            del ref
            torch.cuda.empty_cache()
        del rows
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "robust", "model": args.model, "P": P, "num_params": layout.num_params,
                      "trim": args.trim, "reps": args.reps, "device": torch.cuda.get_device_name(0),
                      "results": results}), flush=True)


if __name__ == "__main__":
    main()
