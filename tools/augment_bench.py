"""Wall-clock cost of the training-time transform chain per batch, host included.

    python tools/augment_bench.py --mode batch     [--preset configs/torch/pneumonia-resnet-pretrained.ini] [--batch 200]
    python tools/augment_bench.py --mode per_image ...

`per_image` builds a batch the way the loaders did before TrainTransform.batch existed — torch.stack([tf(img, rng) ...]) —
and uses nothing else of the transform, so the same file measures an older checkout; `batch` calls tf.batch(images, rng).
The inputs are synthetic decoded images of mixed sizes (sides between --min_side and --max_side, the range of chest X-ray
files), device resident before the clock starts.  The clock runs over --batches batches after --warmup, with a device
synchronisation at both ends; one JSON line is printed.
"""
import argparse
import configparser
import json
import os
import random
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from primia_amd.augment import TrainTransform  # noqa: E402

SWITCHES = ("clahe", "randomgamma", "randombrightness", "blur", "elastic", "optical_distortion", "grid_distortion",
            "grid_shuffle", "hsv", "invert", "cutout", "shadow", "fog", "sun_flare", "solarize", "equalize", "grid_dropout")


def preset_args(path, size):
    """The keys of an INI preset that the transform chain reads (torchlib_compat.Arguments' names)."""
    cfg = configparser.ConfigParser()
    assert cfg.read(path), path
    aug, albu = cfg["augmentation"], cfg["albumentations"]
    S = size or cfg.getint("config", "train_resolution")
    return SimpleNamespace(train_resolution=S, inference_resolution=cfg.getint("config", "inference_resolution", fallback=S),
                           rotation=aug.getfloat("rotation"), translate=aug.getfloat("translate"), scale=aug.getfloat("scale"),
                           shear=aug.getfloat("shear"), albu_prob=albu.getfloat("overall_prob"),
                           individual_albu_probs=albu.getfloat("individual_probs"), noise_std=albu.getfloat("noise_std"),
                           noise_prob=albu.getfloat("noise_prob"), **{k: albu.getboolean(k) for k in SWITCHES})


def main():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("per_image", "batch"), required=True)
    ap.add_argument("--preset", default=os.path.join(root, "configs", "torch", "pneumonia-resnet-pretrained.ini"))
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--size", type=int, default=0, help="train resolution (default: the preset's)")
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pool", type=int, default=64, help="distinct synthetic images the batches draw from")
    ap.add_argument("--min_side", type=int, default=900)
    ap.add_argument("--max_side", type=int, default=1800)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    args = preset_args(a.preset, a.size)
    dev = torch.device("cuda:0")
    C = 3
    rs = np.random.RandomState(a.seed)
    pool = []
    for _ in range(a.pool):
        H, W = rs.randint(a.min_side, a.max_side + 1, size=2)
        ramp = (np.add.outer(np.arange(H), np.arange(W)) % 256).astype(np.uint8)
        pool.append(torch.from_numpy(np.repeat(ramp[:, :, None], C, axis=2) ^ rs.randint(0, 32, (H, W, C)).astype(np.uint8)).to(dev))
    mean, std = torch.full((C,), 0.5), torch.full((C,), 0.25)
    tf = TrainTransform(args, mean, std, dev, C, seed=a.seed)
    rng, pick = random.Random(a.seed), random.Random(a.seed + 1)

    def one_batch():
        imgs = [pool[pick.randrange(a.pool)] for _ in range(a.batch)]
        if a.mode == "batch":
            return tf.batch(imgs, rng)
        return torch.stack([tf(im, rng) for im in imgs])

    for _ in range(a.warmup):
        one_batch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.batches):
        out = one_batch()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.batches
    assert out.shape == (a.batch, C, args.train_resolution, args.train_resolution) and torch.isfinite(out).all()
    print(json.dumps({"tool": "augment_bench", "mode": a.mode, "preset": os.path.basename(a.preset), "batch": a.batch,
                      "size": args.train_resolution, "batches": a.batches, "ms_per_batch": round(ms, 3),
                      "images_per_s": round(a.batch / ms * 1e3, 1)}))


if __name__ == "__main__":
    main()
