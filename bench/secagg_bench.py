"""Secure aggregation (`fed_secagg`) on the ResNet-18 layout: the kernels of csrc/secagg.hip (`ops.fl.secagg_mask_rows`,
`ring_sum`, `ring_unmask`) alternating on one device with their yardsticks — `fl.delta_rows` (the plain streaming
pass over the same rows), `fl.gaussian_add` (the other Philox consumer), `fl.weighted_sum` (FedAvg's accumulation)
and the torch path (`ops.ref.secagg_mask_rows` on device tensors).

    python bench/secagg_bench.py [--clients 13 50] [--degrees 0 8 32 99] [--reps 5] [--out profiles/secagg_bench_mi355x.json]

Prints ONE JSON line (and writes it to --out if given). Per cohort size K and degree d (every row carries d + 1
mask streams; d = 0 here means NO stream at all: the bare quantising pass) the median (and best) time per launch
of every ILP form of the expander (g1u1: one group of four elements per lane, one entry per loop trip; g2u1: two
groups per lane; g1u2: two entries per trip), the Philox calls per second (K · (d + 1) · P / 4 calls a launch),
the bytes of the d = 0 pass (8 · K · P) and its rate, and the per-round total for 100 clients that the K = 50
figure implies. All forms are checked to give the same words before anything is timed.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {"g1u1": 1, "g2u1": 2, "g1u2": 3}


def _timed(fn, inner):
    """Milliseconds per launch over `inner` back-to-back launches between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def _alternate(steps, reps, inner):
    t = {k: [] for k in steps}
    for rep in range(reps + 1):  # rep 0 warms every path up
        for key, fn in steps.items():
            ms = _timed(fn, inner)
            if rep:
                t[key].append(ms)
    return {k: statistics.median(v) for k, v in t.items()}, {k: min(v) for k, v in t.items()}


def _table(K, d):
    """Row k owns d + 1 streams (none at all for d = 0: the bare quantising pass)."""
    per = d + 1 if d else 0
    keys = [(0x9E3779B97F4A7C15 * (i + 1)) & (2 ** 64 - 1) for i in range(K * per)]
    signs = [1 if i % 3 else -1 for i in range(K * per)]
    return [k * per for k in range(K + 1)], keys, signs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, nargs="+", default=[13, 50])
    ap.add_argument("--degrees", type=int, nargs="+", default=[0, 8, 32, 99])
    ap.add_argument("--unmask", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="launches per timed sample")
    ap.add_argument("--model", default="ResNet18")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("secagg_bench needs a GPU")

    from distributed_learning_simulator_amd.ops import build

    build.build()
    from distributed_learning_simulator_amd.data.datasets import get_spec
    from distributed_learning_simulator_amd.models.zoo import build_model
    from distributed_learning_simulator_amd.ops import fl, hip, ref

    dev = torch.device("cuda:0")
    layout = build_model(args.model, get_spec("CIFAR10", {})).layout
    P = layout.padded_size
    valid = layout.valid_mask(dev)
    default = {v: k for k, v in VARIANTS.items()}[hip.secagg_default_variant()]
    R, f = 1.0, 20
    results = []
    for K in args.clients:
        g = torch.Generator(device=dev).manual_seed(K)
        rows = torch.randn(K, P, device=dev, generator=g) * 1e-2 * valid
        theta = torch.randn(P, device=dev, generator=g) * valid
        out = torch.empty((K, P), dtype=torch.int32, device=dev)
        scratch = torch.empty_like(rows)
        acc64 = torch.zeros(P, dtype=torch.float64, device=dev)
        acci = torch.zeros(P, dtype=torch.int64, device=dev)
        ones = torch.ones(K, dtype=torch.float64, device=dev)
        for d in args.degrees:
            table = _table(K, d)
            words = {name: fl.secagg_mask_rows(rows, table, R, f, variant=v)[0] for name, v in VARIANTS.items()}
            same = all(torch.equal(words["g1u1"], w) for w in words.values())
            del words
            steps = {name: (lambda v=v: fl.secagg_mask_rows(rows, table, R, f, out=out, variant=v))
                     for name, v in VARIANTS.items()}
            steps["delta_rows"] = lambda: fl.delta_rows(rows, theta, out=scratch)
            steps["gaussian_add"] = lambda: fl.gaussian_add(acc64, 0.5, 1234, 1)
            inner = args.inner if K * (d + 1) <= 2000 else max(2, args.inner // 4)
            med, best = _alternate(steps, args.reps, inner)
            calls = K * (d + 1 if d else 0) * (P // 4)
            row = {"clients": K, "degree": d, "streams_per_row": d + 1 if d else 0, "launches_per_sample": inner,
                   "variants_agree": same, **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                   **{f"{k}_best_ms": round(v, 4) for k, v in best.items()},
                   "gaussian_add_Gcalls_per_s": round((P / 2) / (med["gaussian_add"] * 1e-3) / 1e9, 2),
                   "delta_rows_GBps": round(8 * K * P / (med["delta_rows"] * 1e-3) / 1e9, 1)}
            if d == 0:
                row["bytes"] = 8 * K * P
                row.update({f"{k}_GBps": round(8 * K * P / (med[k] * 1e-3) / 1e9, 1) for k in VARIANTS})
            else:
                row["philox_calls"] = calls
                row.update({f"{k}_Gcalls_per_s": round(calls / (med[k] * 1e-3) / 1e9, 2) for k in VARIANTS})
                row["default_over_gaussian_add_calls_rate"] = round(
                    (calls / med[default]) / ((P / 2) / med["gaussian_add"]), 2)
            if K == max(args.clients):
                row["per_round_100_clients_ms"] = round(med[default] * 100.0 / K, 3)
            results.append(row)
        # the server side: the ring sum against FedAvg's weighted sum on the same K · P
        steps = {"ring_sum": lambda: fl.ring_sum(out, acci), "weighted_sum": lambda: fl.weighted_sum(rows, ones, acc64)}
        med, best = _alternate(steps, args.reps, args.inner)
        results.append({"clients": K, "ring_sum_ms": round(med["ring_sum"], 4), "weighted_sum_ms": round(med["weighted_sum"], 4),
                        "ring_sum_best_ms": round(best["ring_sum"], 4), "weighted_sum_best_ms": round(best["weighted_sum"], 4),
                        "bytes": 4 * K * P + 16 * P,
                        "ring_sum_GBps": round((4 * K * P + 16 * P) / (med["ring_sum"] * 1e-3) / 1e9, 1),
                        "weighted_sum_GBps": round((4 * K * P + 16 * P) / (med["weighted_sum"] * 1e-3) / 1e9, 1)})
        del rows, out, scratch
        torch.cuda.empty_cache()
    acci = torch.zeros(P, dtype=torch.int64, device=dev)
    for E in args.unmask:
        _, keys, signs = _table(1, E - 1)
        steps = {name: (lambda v=v: fl.ring_unmask(acci, (keys, signs), variant=v)) for name, v in VARIANTS.items()
                 if name != "g2u1"}
        med, best = _alternate(steps, args.reps, max(2, args.inner // 4))
        results.append({"unmask_entries": E, **{f"ring_unmask_{k}_ms": round(v, 4) for k, v in med.items()},
                        **{f"ring_unmask_{k}_Gcalls_per_s": round(E * (P // 4) / (v * 1e-3) / 1e9, 2) for k, v in med.items()}})
    # the torch path: the oracle's own mask routine on device tensors, K = 13, d = 8 (seconds: two samples of one)
    K, d = 13, 8
    rows = torch.randn(K, P, device=dev) * 1e-2 * valid
    table = _table(K, d)
    want = fl.secagg_mask_rows(rows, table, R, f)[0]
    got = ref.secagg_mask_rows(rows, *table, R, f)[0]
    torch_ms = min(_timed(lambda: ref.secagg_mask_rows(rows, *table, R, f), 1) for _ in range(2))
    kernel_ms = statistics.median(_timed(lambda: fl.secagg_mask_rows(rows, table, R, f), 5) for _ in range(3))
    results.append({"torch_path": True, "clients": K, "degree": d, "torch_ms": round(torch_ms, 2),
                    "kernel_alloc_out_ms": round(kernel_ms, 4), "speedup": round(torch_ms / kernel_ms, 1),
                    "paths_agree": bool(torch.equal(want, got))})
    line = json.dumps({"bench": "secagg", "measured": True, "model": args.model, "P": P, "num_params": layout.num_params,
                       "reps": args.reps, "launches_per_sample": args.inner, "default_variant": default,
                       "device": torch.cuda.get_device_name(0), "results": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
