"""Whole rounds with and without secure aggregation: `fed_avg` against `fed_secagg` on the complete mask graph and
on the degree-8 ring, ResNet-18, 50 clients resident, 1 local epoch, five rounds each; per-round wall, train and
aggregate seconds from the sessions' metrics and the median wall time of rounds 3-5.

    python bench/secagg_rounds.py [--workers 50] [--rounds 5] [--out profiles/secagg_rounds_mi355x.json]

Prints ONE JSON line (and writes it to --out if given).
"""

import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--model", default="ResNet18")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("secagg_rounds needs a GPU")
    from distributed_learning_simulator_amd.ops import build

    build.build()
    from distributed_learning_simulator_amd.config import load_config
    from distributed_learning_simulator_amd.parallel.comm import Comm
    from distributed_learning_simulator_amd.session import Session

    common = {"model_name": args.model, "worker_number": args.workers, "round": args.rounds, "epoch": 1,
              "save_models": False, "log_level": "WARNING"}
    secagg = {"algorithm_kwargs.random_client_number": "null", "algorithm_kwargs.failure_rate": 0,
              "algorithm_kwargs.secagg_range": 1.0}
    runs = {"fed_avg": ("fed_avg", {}),
            "fed_secagg_complete": ("fed_secagg", {**secagg, "algorithm_kwargs.secagg_degree": 0,
                                                   "algorithm_kwargs.secagg_threshold": "null"}),
            "fed_secagg_d8": ("fed_secagg", {**secagg, "algorithm_kwargs.secagg_degree": 8,
                                             "algorithm_kwargs.secagg_threshold": 5})}
    out = {"measured": True, "model": args.model, "workers": args.workers, "rounds": args.rounds, "epoch": 1,
           "device": torch.cuda.get_device_name(0)}
    for name, (method, extra) in runs.items():
        with tempfile.TemporaryDirectory() as tmp:
            ov = {**common, **extra, "save_dir": tmp}
            cfg = load_config(["--config-name", f"{method}/cifar10.yaml"] + [f"++{method}.{k}={v}" for k, v in ov.items()])
            sess = Session(cfg, comm=Comm(device=torch.device("cuda:0")))
            res = sess.run()
            rows = sess.metrics
            out[name] = {
                "wall_s": [round(m["wall_s"], 4) for m in rows],
                "train_s": [round(m.get("train_s", 0.0), 4) for m in rows],
                "aggregate_s": [round(m.get("aggregate_s", 0.0), 4) for m in rows],
                "median_wall_s_after_round_2": round(statistics.median(m["wall_s"] for m in rows[2:]), 4),
                "capacity": sess.trainer.capacity, "bytes_up": res["bytes_up"],
                **({"mask_streams": rows[-1]["secagg_mask_streams"], "frac_bits": rows[-1]["secagg_frac_bits"],
                    "clamped_fraction": rows[-1]["secagg_clamped_fraction"]} if method == "fed_secagg" else {}),
            }
            del sess
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
