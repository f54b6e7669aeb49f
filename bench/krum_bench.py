"""Pairwise squared distances (Krum / Multi-Krum) on the ResNet-18 layout: the kernel
(`ops.fl.pairwise_sq_dists`, csrc/krum.hip) against the torch path (`torch.cdist` on fp64 copies of
the rows without the matmul shortcut, squared) on the same rows, alternating on one device.

    python bench/krum_bench.py [--clients 13 50 100] [--reps 5] [--out profiles/krum_bench_mi355x.json]

Prints ONE JSON line (and writes it to --out if given): per cohort size n the median (and best)
time of both paths, the speed-up, pair-elements per second (n² · P per launch: what the result
needs; the kernel computes the tiles on and above the diagonal, whole), the share of the chip's fp64
vector rate that is (MI355X datasheet: 78.6 TFLOP/s fp64 vector counts an FMA as two; the contract
forbids FMAs, so the ceiling is 39.3 T instructions/s, three per pair-element), the bytes the kernel
must move against HBM (n · P · 4 read once + the span sums written and read + 8 n²) and the largest
relative difference between the two paths (torch adds in its own order, so the comparison is to
1e-12; bit equality with the ordered oracle is what tests/test_krum.py checks).
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_VECTOR_TFLOPS = 78.6  # AMD Instinct MI355X datasheet, peak fp64 vector (FMA = 2 FLOP)


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model", default="ResNet18")
    ap.add_argument("--block-rows", type=int, default=128, help="rows per fp64 copy of the torch path")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("krum_bench needs a GPU")

    from distributed_learning_simulator_amd.ops import build

    build.build()
    from distributed_learning_simulator_amd.data.datasets import get_spec
    from distributed_learning_simulator_amd.models.zoo import build_model
    from distributed_learning_simulator_amd.ops import fl, hip

    dev = torch.device("cuda:0")
    layout = build_model(args.model, get_spec("CIFAR10", {})).layout
    P = layout.padded_size
    valid = layout.valid_mask(dev)
    results = []
    for n in args.clients:
        g = torch.Generator(device=dev).manual_seed(n)
        rows = torch.randn(n, P, device=dev, generator=g) * 1e-2 * valid
        out = torch.empty((n, n), dtype=torch.float64, device=dev)

        def kernel():
            return fl.pairwise_sq_dists(rows, out=out)

        def torch_path():
            res = torch.empty((n, n), dtype=torch.float64, device=dev)
            blocks = [(a, min(n, a + args.block_rows)) for a in range(0, n, args.block_rows)]
            for a0, a1 in blocks:
                xa = rows[a0:a1].double()
                for b0, b1 in blocks:
                    xb = xa if b0 == a0 else rows[b0:b1].double()
                    res[a0:a1, b0:b1] = torch.cdist(xa, xb, compute_mode="donot_use_mm_for_euclid_dist") ** 2
            return res

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
        scratch = hip.pairwise_scratch_doubles(n, P) * 8
        nbytes = n * P * 4 + 2 * scratch + 8 * n * n
        pe_s = n * n * P / (med["kernel"] * 1e-3)
        results.append({
            "clients": n, "kernel_ms": round(med["kernel"], 3), "kernel_best_ms": round(min(t["kernel"]), 3),
            "torch_cdist_ms": round(med["torch"], 3), "torch_cdist_best_ms": round(min(t["torch"]), 3),
            "speedup": round(med["torch"] / med["kernel"], 2),
            "pair_elements_per_s": round(pe_s / 1e12, 3),  # in 1e12 / s
            "fp64_vector_share": round(3 * pe_s / (FP64_VECTOR_TFLOPS * 1e12 / 2), 3),
            "hbm_bytes": nbytes, "scratch_bytes": scratch, "hbm_GBps": round(nbytes / (med["kernel"] * 1e-3) / 1e9, 1),
            "max_rel_diff": rel, "paths_agree": bool(rel < 1e-12),
        })
        del ref, rows
        torch.cuda.empty_cache()
    line = json.dumps({"bench": "krum", "model": args.model, "P": P, "num_params": layout.num_params,
                       "reps": args.reps, "device": torch.cuda.get_device_name(0),
                       "fp64_vector_peak_tflops": FP64_VECTOR_TFLOPS, "peak_source": "MI355X datasheet",
                       "results": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
