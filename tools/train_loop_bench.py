#!/usr/bin/env python3
"""Throughput of the training loop a user runs — torchlib_compat.train(), the body of `train.py` without
--train_federated — eagerly and with --hip_graph, at bench.py's configuration (bf16, batch 256, 3 x 224 x 224, SGD,
lr 1e-4, weight decay 5e-4) on device-resident synthetic batches like train.py's SyntheticLoader.

The two modes run on two engines built from the same weights, alternating (eager, graph, eager, graph, ...), each run
a train() call over `--steps` batches bracketed by device synchronisations; one untimed train() call per mode first
(the graphed mode captures its step there).  Prints one JSON line: per mode the median and every run's ms per step and
images per second.  --dp times the DP-SGD loop (GroupNorm network, clip 1.0, noise multiplier 1.3: train.py with
differentially_private = yes) with --dp_noise torch (torch.randn; --hip_graph leaves its steps eager) or chacha (the
device ChaCha20 stream of primia_amd.dp_noise; --hip_graph replays the steps); --dp_norm frozen times it on the BatchNorm
network with frozen statistics (train.py's --dp_norm frozen) instead.  Needs a GPU (there is no CPU path)."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="train() batches per timed run")
    ap.add_argument("--runs", type=int, default=5, help="timed runs per mode")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--buffers", type=int, default=4, help="distinct device batches the loader cycles through")
    ap.add_argument("--modes", default="eager,graph")
    ap.add_argument("--dp", action="store_true", help="the DP-SGD loop (differentially_private = yes)")
    ap.add_argument("--dp_noise", choices=("torch", "chacha"), default="torch", help="with --dp: train.py's --dp_noise")
    ap.add_argument("--dp_norm", choices=("group", "frozen"), default="group", help="with --dp: train.py's --dp_norm")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_loop_bench needs a GPU")

    from primia_amd.engine import ResNet18Engine
    from primia_amd.optim import EngineOptimizer
    from primia_amd.torchlib_compat import train

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1000)
    bufs = [(torch.randn(a.batch, 3, a.size, a.size, generator=g).to(dev),
             torch.randint(0, 3, (a.batch,), generator=g).to(dev)) for _ in range(a.buffers)]
    loader = [bufs[i % a.buffers] for i in range(a.steps)]
    modes = a.modes.split(",")
    runs = {}
    for m in modes:
        torch.manual_seed(42)
        eng = ResNet18Engine(a.batch, 3, 3, a.size, "max", dtype=torch.bfloat16, device=dev,
                             norm=a.dp_norm if a.dp else "batch")
        eng.init_weights()
        if a.dp:
            eng.dp_params = {"max_grad_norm": 1.0, "noise_multiplier": 1.3}
            if a.dp_noise == "chacha":
                from primia_amd.dp_noise import DeviceNoise

                eng.dp_noise = DeviceNoise(dev)
        args = SimpleNamespace(optimizer="SGD", lr=1e-4, weight_decay=5e-4, log_interval=10 ** 9, mixup=False,
                               hip_graph=m == "graph")
        opt = EngineOptimizer.from_args(eng, args)
        train(args, eng, dev, loader[:max(3, a.buffers)], opt, 0, None, verbose=False)   # warm-up (+ capture)
        runs[m] = (eng, args, opt, [])
    torch.cuda.synchronize()
    for _ in range(a.runs):
        for m in modes:
            eng, args, opt, ts = runs[m]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train(args, eng, dev, loader, opt, 1, None, verbose=False)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / a.steps * 1e3)
    out = {"metric": "train_loop", "batch": a.batch, "size": a.size, "dtype": "bf16", "optimizer": "SGD",
           "steps": a.steps, "runs": a.runs}
    if a.dp:
        from primia_amd.graphed_train import captures

        out["dp_noise"] = a.dp_noise
        out["dp_norm"] = a.dp_norm
        out["graphed_keys"] = {m: len(captures(runs[m][0])) for m in modes}
    for m in modes:
        ts = runs[m][3]
        med = statistics.median(ts)
        out[m] = {"ms_per_step": round(med, 3), "images_per_sec": round(a.batch / med * 1e3, 1),
                  "ms_per_step_runs": [round(t, 3) for t in ts]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
