"""GroupNorm kernels (csrc/groupnorm.hip) on ResNet-18 CIFAR's four normalised shapes, batch 64, at
13 and 50 clients with G = 2 and 32: the forward with ReLU and planes and the backward with the ReLU
gate, against (a) the standalone BatchNorm passes `hip.bn_fwd` / `hip.bn_bwd` on the same tensors,
which move the same bytes, and (b) torch's eager `F.group_norm` (+ ReLU) forward and backward. Median
of --reps timed repeats of --iters launches, the variants alternating on one device.

    python bench/gn_bench.py [--clients 13 50] [--groups 2 32] [--reps 5] [--out profiles/gn_bench_mi355x.json]
    python bench/gn_bench.py --rounds [--workers 50] [--out profiles/gn_rounds_mi355x.json]

Bytes a launch must move per element (fp32): forward x read, y and its two bf16 planes written = 12 B;
backward dy, x and the gate's y read, dx written = 16 B. The rate is those bytes over the median time,
also as a fraction of the 6.3 TB/s a float4 copy reaches on this device.

--rounds: whole `fed_avg` rounds of ResNet-18 with BatchNorm and with GroupNorm (50 clients resident, 1
local epoch, 5 rounds, median wall time of rounds 3-5). Prints ONE JSON line (and writes it to --out).
"""

import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"l1": (32, 32, 64), "l2": (16, 16, 128), "l3": (8, 8, 256), "l4": (4, 4, 512)}
COPY_TBPS = 6.3
FWD_BYTES, BWD_BYTES = 12, 16


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernels(args):
    import torch.nn.functional as F

    from distributed_learning_simulator_amd.ops import hip

    dev = torch.device("cuda:0")
    B = args.batch
    results = []
    for K in args.clients:
        for name, (H, W, C) in SHAPES.items():
            gen = torch.Generator(device=dev).manual_seed(K)
            x = torch.randn(K, B, H, W, C, device=dev, generator=gen)
            dy = torch.randn(K, B, H, W, C, device=dev, generator=gen)
            gamma = torch.rand(K, C, device=dev, generator=gen) + 0.5
            beta = torch.randn(K, C, device=dev, generator=gen)
            valid = torch.full((K,), B, dtype=torch.int32, device=dev)
            R = B * H * W
            x3, dy3 = x.view(K, R, C), dy.view(K, R, C)
            vr = valid * (H * W)
            gg, gb = torch.zeros(K, C, device=dev), torch.zeros(K, C, device=dev)
            yb, bmean, brstd, bmask, _ = hip.bn_fwd(x3, gamma, beta, vr, True, None, with_mask=True, planes=1)
            n = x.numel()
            for G in args.groups:
                y, mean, rstd, _ = hip.gn_fwd(x, gamma, beta, G, valid, True, None, planes=True)
                xt = x.view(K * B, H, W, C).permute(0, 3, 1, 2).detach().requires_grad_()
                wt, bt = gamma[0].clone().requires_grad_(), beta[0].clone().requires_grad_()
                dyt = dy.view(K * B, H, W, C).permute(0, 3, 1, 2)
                yt = F.relu(F.group_norm(xt, G, wt, bt))
                variants = (
                    ("gn_fwd", lambda: hip.gn_fwd(x, gamma, beta, G, valid, True, None, planes=True)),
                    ("gn_bwd", lambda: hip.gn_bwd(dy, x, y, mean, rstd, gamma, G, valid, True, False)),
                    ("bn_fwd", lambda: hip.bn_fwd(x3, gamma, beta, vr, True, None, with_mask=True, planes=1)),
                    ("bn_bwd", lambda: hip.bn_bwd(dy3, x3, yb, bmean, brstd, gamma, vr, True, gg, gb, False)),
                    ("bn_bwd_bits", lambda: hip.bn_bwd(dy3, x3, yb, bmean, brstd, gamma, vr, True, gg, gb, False,
                                                       relu_mask=bmask)),
                    ("torch_fwd", lambda: F.relu(F.group_norm(xt, G, wt, bt))),
                    ("torch_bwd", lambda: torch.autograd.grad(yt, (xt, wt, bt), dyt, retain_graph=True)),
                )
                t = {k: [] for k, _ in variants}
                for rep in range(args.reps + 1):  # rep 0 warms every variant up
                    for key, fn in variants:
                        ms = _timed(fn, args.iters)
                        if rep:
                            t[key].append(ms)
                med = {k: statistics.median(v) for k, v in t.items()}
                fb, bb = FWD_BYTES * n, BWD_BYTES * n
                row = {"clients": K, "layer": name, "shape": [B, H, W, C], "groups": G,
                       "fwd_bytes": fb, "bwd_bytes": bb}
                for k, v in med.items():
                    row[k + "_ms"] = round(v, 4)
                    row[k + "_best_ms"] = round(min(t[k]), 4)
                for k, nb in (("gn_fwd", fb), ("gn_bwd", bb), ("bn_fwd", fb), ("bn_bwd", bb)):
                    tbps = nb / (med[k] * 1e-3) / 1e12
                    row[k + "_TBps"] = round(tbps, 3)
                    row[k + "_of_copy"] = round(tbps / COPY_TBPS, 3)
                row["gn_over_bn_fwd"] = round(med["gn_fwd"] / med["bn_fwd"], 3)
                row["gn_over_bn_bwd"] = round(med["gn_bwd"] / med["bn_bwd"], 3)
                row["torch_over_gn_fwd"] = round(med["torch_fwd"] / med["gn_fwd"], 3)
                row["torch_over_gn_bwd"] = round(med["torch_bwd"] / med["gn_bwd"], 3)
                results.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del xt, wt, bt, dyt, yt, y, mean, rstd
            del x, dy, yb, bmask, x3, dy3
            torch.cuda.empty_cache()
    return {"bench": "gn", "measured": True, "batch": B, "reps": args.reps, "iters": args.iters,
            "copy_TBps": COPY_TBPS, "device": torch.cuda.get_device_name(0), "results": results}


def rounds(args):
    from distributed_learning_simulator_amd.config import load_config
    from distributed_learning_simulator_amd.parallel.comm import Comm
    from distributed_learning_simulator_amd.session import Session

    out = {"bench": "gn_rounds", "measured": True, "model": "ResNet18", "workers": args.workers, "rounds": 5,
           "epoch": 1, "device": torch.cuda.get_device_name(0)}
    for name, norm in (("batch", "batch"), ("group", "group"), ("batch_again", "batch"), ("group_again", "group")):
        with tempfile.TemporaryDirectory() as tmp:
            ov = {"model_name": "ResNet18", "model_kwargs.norm": norm, "worker_number": args.workers, "round": 5,
                  "epoch": 1, "save_models": False, "log_level": "WARNING", "save_dir": tmp}
            cfg = load_config(["--config-name", "fed_avg/cifar10.yaml"] + [f"++fed_avg.{k}={v}" for k, v in ov.items()])
            sess = Session(cfg, comm=Comm(device=torch.device("cuda:0")))
            sess.run()
            rows = sess.metrics
            out[name] = {"wall_s": [round(m["wall_s"], 4) for m in rows],
                         "train_s": [round(m.get("train_s", 0.0), 4) for m in rows],
                         "median_wall_s_after_round_2": round(statistics.median(m["wall_s"] for m in rows[2:]), 4)}
            del sess
            torch.cuda.empty_cache()
    out["group_over_batch"] = round(out["group"]["median_wall_s_after_round_2"]
                                    / out["batch"]["median_wall_s_after_round_2"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, nargs="+", default=[13, 50])
    ap.add_argument("--groups", type=int, nargs="+", default=[2, 32])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="launches per timed repeat")
    ap.add_argument("--rounds", action="store_true", help="whole fed_avg rounds, BatchNorm against GroupNorm")
    ap.add_argument("--workers", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gn_bench needs a GPU")
    from distributed_learning_simulator_amd.ops import build

    build.build()
    line = json.dumps(rounds(args) if args.rounds else kernels(args))
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
