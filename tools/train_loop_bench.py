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
network with frozen statistics (train.py's --dp_norm frozen) instead.  --dp_sampling poisson times train.py's Poisson-sampled
loop: --records synthetic records, expected batch --batch, the engine at the capacity dp_accountant.capacity_for gives for
--planned_steps; every step is select + gather (primia_amd.dp_sampling.PoissonLoader) and the masked DP step; images per
second then counts the EXPECTED batch.  --dp_micro_batches K (train.py's flag) runs every step as K passes on an engine of
1 / K of the batch or capacity (primia_amd.dp_micro); ms per step is then per LOGICAL step.  --dp_clip adaptive (train.py's
flag) gives every mode's engine an adaptive clipping norm (primia_amd.dp_clip, its defaults); a mode named "eager:adaptive"
or "graph:adaptive" has one whatever the flag says, so `--modes graph,graph:adaptive` alternates the fixed and the adaptive
loop in one session, and the line then carries each such mode's final C.  --dp_augmult M (train.py's flag, with
--dp_sampling poisson) gives every record M views: capacity and expected batch are divided by M, so the engine keeps its
slots and a step does the same kernel work on M times fewer records; a mode with the suffix ":mM" (graph:m4) has M views
whatever the flag says, so `--modes graph,graph:m4` alternates the two in one session.  A mode with the suffix ":weighted"
(graph:weighted) sets a class-weight tensor on its DP engine — train.py's weight_classes = yes under DP, the per-sample
weighted loss of primia_amd.dp_weights — so `--modes graph,graph:weighted` alternates the two.  --capacity C fixes the capacity (in
slots of the M = 1 loop) instead of deriving it from --planned_steps.  With --dp the line also
carries the engine's slots and, per mode, the peak of torch.cuda.max_memory_allocated() over what was allocated before that
mode's engine was built (the batches, the records, an earlier mode's engine), read after the mode's warm-up: the engine,
its DP buffers and, graphed, the graphs' pools.  Needs a GPU (there is no CPU path)."""
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
    ap.add_argument("--dp_sampling", choices=("shuffle", "poisson"), default="shuffle",
                    help="with --dp: train.py's --dp_sampling")
    ap.add_argument("--records", type=int, default=1721, help="--dp_sampling poisson: records sampled from")
    ap.add_argument("--planned_steps", type=int, default=280, help="--dp_sampling poisson: steps the capacity is sized for")
    ap.add_argument("--dp_micro_batches", type=int, default=1, help="with --dp: train.py's --dp_micro_batches")
    ap.add_argument("--dp_clip", choices=("fixed", "adaptive"), default="fixed", help="with --dp: train.py's --dp_clip")
    ap.add_argument("--dp_augmult", type=int, default=1, help="with --dp --dp_sampling poisson: train.py's --dp_augmult")
    ap.add_argument("--capacity", type=int, default=0, help="--dp_sampling poisson: the capacity, instead of the accountant's")
    a = ap.parse_args()
    poisson = a.dp and a.dp_sampling == "poisson"
    K = a.dp_micro_batches if a.dp else 1
    if K < 1 or (not poisson and a.batch % K):
        raise SystemExit("--dp_micro_batches: at least 1, and in shuffle mode a divisor of --batch")
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
    capacity = a.batch
    if poisson:
        from primia_amd import dp_accountant
        from primia_amd.dp_sampling import DeviceSampler, PoissonLoader

        q = dp_accountant.q_of_threshold(dp_accountant.threshold_for((a.batch, a.records)))
        capacity = a.capacity or dp_accountant.capacity_for(a.records, q, a.planned_steps, 1e-5, sigma=1.3)
        records = torch.cat([bufs[i % a.buffers][0] for i in range(-(-a.records // a.batch))])[:a.records].contiguous()
        labels = torch.cat([bufs[i % a.buffers][1] for i in range(-(-a.records // a.batch))])[:a.records].contiguous()

        class Draws:
            """`count` Poisson batches of one PoissonLoader, whatever its epoch length."""

            def __init__(self, pl, count):
                self.pl, self.count = pl, count

            def __len__(self):
                return self.count

            def __iter__(self):
                return (self.pl.draw() for _ in range(self.count))
    modes = a.modes.split(",")
    views_of = {}
    for m in modes:
        base, _, suffix = m.partition(":m")
        views_of[m] = int(suffix) if suffix.isdigit() else (a.dp_augmult if a.dp else 1)
        if suffix.isdigit():
            m = base
        if m not in ("eager", "graph") and not (a.dp and m in ("eager:adaptive", "graph:adaptive", "eager:weighted",
                                                                 "graph:weighted")):
            raise SystemExit(f"mode {m!r}: eager or graph, with --dp also eager:adaptive or graph:adaptive, "
                             "eager:weighted or graph:weighted, and :mM")
    if any(v < 1 or (v > 1 and not poisson) for v in views_of.values()):
        raise SystemExit("--dp_augmult / a :mM mode: at least 1, and only with --dp --dp_sampling poisson")
    runs, peak = {}, {}
    for m in modes:
        torch.manual_seed(42)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        views = views_of[m]
        cap_m = capacity // views               # records: the engine keeps its slots
        eng = ResNet18Engine(-(-cap_m // K) * views, 3, 3, a.size, "max", dtype=torch.bfloat16, device=dev,
                             norm=a.dp_norm if a.dp else "batch")
        eng.init_weights()
        if a.dp:
            eng.dp_params = {"max_grad_norm": 1.0, "noise_multiplier": 1.3}
            eng.dp_micro_batches = K
            if a.dp_noise == "chacha":
                from primia_amd.dp_noise import DeviceNoise

                eng.dp_noise = DeviceNoise(dev)
            if a.dp_clip == "adaptive" or ":adaptive" in m:
                from primia_amd.dp_clip import AdaptiveClip

                eng.dp_clip = AdaptiveClip(dev, sigma_b=a.batch / 20.0)
                eng.dp_clip.tensors()
            if ":weighted" in m:    # the per-sample weighted loss; (1349, 2538, 1345): the chest X-ray set's class counts
                from primia_amd.dp_weights import balanced_weights

                eng.class_weight = balanced_weights(torch.tensor([1349, 2538, 1345])).to(dev).contiguous()
            if poisson:
                pl = PoissonLoader(records, labels, max(1, a.batch // views), cap_m, DeviceSampler(dev), micro_batches=K,
                                   views=views)
                eng.dp_params["expected_batch"] = pl.expected_batch
                if views > 1:
                    eng.dp_params["views"] = views
        args = SimpleNamespace(optimizer="SGD", lr=1e-4, weight_decay=5e-4, log_interval=10 ** 9, mixup=False,
                               hip_graph=m.startswith("graph"))
        opt = EngineOptimizer.from_args(eng, args)
        mine = Draws(pl, a.steps) if poisson else loader
        warm = Draws(pl, max(3, a.buffers)) if poisson else loader[:max(3, a.buffers)]
        train(args, eng, dev, warm, opt, 0, None, verbose=False)   # warm-up (+ capture)
        runs[m] = (eng, args, opt, [], mine)
        torch.cuda.synchronize()
        peak[m] = torch.cuda.max_memory_allocated() - held
    torch.cuda.synchronize()
    for _ in range(a.runs):
        for m in modes:
            eng, args, opt, ts, mine = runs[m]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train(args, eng, dev, mine, opt, 1, None, verbose=False)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / a.steps * 1e3)
    out = {"metric": "train_loop", "batch": a.batch, "size": a.size, "dtype": "bf16", "optimizer": "SGD",
           "steps": a.steps, "runs": a.runs}
    if a.dp:
        from primia_amd.graphed_train import captures

        out["dp_noise"] = a.dp_noise
        out["dp_norm"] = a.dp_norm
        out["graphed_keys"] = {m: len(captures(runs[m][0])) for m in modes}
        out["dp_sampling"] = a.dp_sampling
        out["dp_clip"] = {m: runs[m][0].dp_clip.value() if runs[m][0].dp_clip is not None else "fixed" for m in modes}
        out.update(dp_micro_batches=K, engine_slots=runs[modes[0]][0].N, peak_bytes_over_held=peak)
        out["dp_augmult"] = views_of
        out["class_weight"] = {m: runs[m][0].class_weight.tolist() if runs[m][0].class_weight is not None else None
                               for m in modes}
        if poisson:
            out.update(records=a.records, capacity=capacity, planned_steps=a.planned_steps,
                       overflow_events={m: runs[m][4].pl.sampler.overflow_events() for m in modes})
    for m in modes:
        ts = runs[m][3]
        med = statistics.median(ts)
        # (M views: a.batch // M records per step, each M images)
        out[m] = {"ms_per_step": round(med, 3), "images_per_sec": round(a.batch // views_of[m] * views_of[m] / med * 1e3, 1),
                  "ms_per_step_runs": [round(t, 3) for t in ts]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
