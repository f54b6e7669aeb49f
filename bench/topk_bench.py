"""Top-k error-feedback upload + server accumulation on the ResNet-18 layout: the packed path
(`ops.compress.pack_topk_ef` + `SparsePayload.accumulate`, csrc/topk.hip) against the dense
`torch.topk` path (`TopKErrorFeedbackWorker.sparsify` + the residual update of
`ErrorFeedbackWorker._get_sent_data` + dense `fl.weighted_sum`) on the same rows, alternating on
one device. Every timed run starts from the same (Δ, e); restoring them is not timed.

    python bench/topk_bench.py [--clients 13 50] [--ratio 0.01] [--reps 5]

Prints ONE JSON line: per cohort size the median (and best) time of both paths, the packed path
split into pack and accumulate, and the pack's achieved GB/s over the bytes its passes must move
(28 B per element of K·P: 12 first pass, 4 + 4 the other two histogram passes, 4 count, 4 emit;
plus 16 B per selected entry), to set against the ~30 B/element estimate.
"""

import argparse
import json
import os
import statistics
import sys
import types

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
    ap.add_argument("--clients", type=int, nargs="+", default=[13, 50])
    ap.add_argument("--ratio", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model", default="ResNet18")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench needs a GPU")

    from distributed_learning_simulator_amd.ops import build

    build.build()
    from distributed_learning_simulator_amd.data.datasets import get_spec
    from distributed_learning_simulator_amd.models.zoo import build_model
    from distributed_learning_simulator_amd.ops import compress, fl
    from distributed_learning_simulator_amd.worker.error_feedback_worker import TopKErrorFeedbackWorker

    dev = torch.device("cuda:0")
    layout = build_model(args.model, get_spec("CIFAR10", {})).layout
    P, n = layout.padded_size, layout.num_params
    k = max(1, int(n * args.ratio))
    meta = compress.LayoutMeta.of(layout, dev)
    valid = layout.valid_mask(dev)
    stub = types.SimpleNamespace(trainer=types.SimpleNamespace(layout=layout), ratio=args.ratio)
    results = []
    for K in args.clients:
        g = torch.Generator(device=dev).manual_seed(K)
        delta0 = torch.randn(K, P, device=dev, generator=g) * 1e-2 * valid
        err0 = torch.randn(K, P, device=dev, generator=g) * 3e-3 * valid
        w = (torch.rand(K, device=dev, generator=g, dtype=torch.float64) + 0.5) * 100
        widx = torch.arange(K, device=dev)
        rows, error = torch.empty_like(delta0), torch.empty_like(err0)

        def restore():
            rows.copy_(delta0)
            error.copy_(err0)

        def dense():  # ErrorFeedbackWorker._get_sent_data + FedAVGAlgorithm._process, dense form
            rows.add_(error[widx])
            sparse, _ = TopKErrorFeedbackWorker.sparsify(stub, rows)
            error[widx] = rows - sparse
            rows.copy_(sparse)
            return fl.weighted_sum(rows, w, torch.zeros(P, dtype=torch.float64, device=dev))

        def pack():
            return compress.pack_topk_ef(rows, error, meta, k)

        def packed():
            p = pack()
            acc = torch.zeros(P, dtype=torch.float64, device=dev)
            p.accumulate(acc, w)
            return acc

        t = {"dense": [], "packed": [], "pack": [], "acc": []}
        ref = {}
        for rep in range(args.reps + 1):  # rep 0 warms both paths up
            for name, fn in (("dense", dense), ("packed", packed)):
                restore()
                ms, out = _timed(fn)
                if rep:
                    t[name].append(ms)
                else:
                    ref[name] = (out, error.clone())
            restore()
            ms, p = _timed(pack)
            ms2, _ = _timed(lambda: p.accumulate(torch.zeros(P, dtype=torch.float64, device=dev), w))
            if rep:
                t["pack"].append(ms)
                t["acc"].append(ms2)
        # same computation: equal up to torch.topk's tie placement and fp64 summation order
        (ad, ed), (ap_, ep) = ref["dense"], ref["packed"]
        rel = ((ad - ap_).abs().max() / ad.abs().max()).item()
        med = {kk: statistics.median(v) for kk, v in t.items()}
        pack_bytes = K * P * 28 + K * k * 16
        results.append({
            "clients": K, "k": k,
            "dense_topk_ms": round(med["dense"], 3), "dense_topk_best_ms": round(min(t["dense"]), 3),
            "packed_ms": round(med["packed"], 3), "packed_best_ms": round(min(t["packed"]), 3),
            "pack_ms": round(med["pack"], 3), "accumulate_ms": round(med["acc"], 3),
            "pack_GBps": round(pack_bytes / (med["pack"] * 1e-3) / 1e9, 1),
            "speedup": round(med["dense"] / med["packed"], 2),
            "acc_max_rel_diff": rel, "residual_equal": bool(torch.equal(ed, ep)),
        })
        del delta0, err0, rows, error, ref
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "topk", "model": args.model, "P": P, "num_params": n, "ratio": args.ratio,
                      "reps": args.reps, "device": torch.cuda.get_device_name(0), "results": results}), flush=True)


if __name__ == "__main__":
    main()
