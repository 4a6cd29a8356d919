#!/usr/bin/env python
"""How often the reference's per-share truncation is expected to wrap in one encrypted pass of a folded ResNet-18: the
float64 plaintext forward (primia_amd.secure.expected_wraps) sums |z| / 2^64 over the pre-truncation values z of the three
kinds of product site -- conv2d, the folded norm, fc -- and reports the largest |z| / 2^62, the precondition of
--faithful_trunc.  CPU only: no GPU, no library.  DESIGN.md §4 quotes this output.

    python tools/secure_trunc_wraps.py [--size 32 224] [--pf 3 6] [--images 2] [--image_scale 1.0] [--seed 1]
    python tools/secure_trunc_wraps.py --model_weights CHECKPOINT [--size S] ...

Without a checkpoint: the 8-block network of the benchmark (primia_amd.resnet_spec's initialisation under --seed, three
classes) on N(0, 1) images times --image_scale.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from primia_amd import resnet_spec as rs                                      # noqa: E402
from primia_amd.secure import expected_wraps                                  # noqa: E402
from primia_amd.torchlib_compat import Arguments  # noqa: E402,F401  (checkpoints pickle an Arguments instance)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model_weights", default=None, help="a BatchNorm checkpoint of train.py (folded here, as --fold_norm does)")
    ap.add_argument("--size", type=int, nargs="+", default=[32, 224])
    ap.add_argument("--pf", type=int, nargs="+", default=[3, 6])
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--image_scale", type=float, default=1.0)
    ap.add_argument("--pooling", choices=("max", "avg"), default="max")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    for size in a.size:
        if a.model_weights:
            sd = torch.load(a.model_weights, map_location="cpu", weights_only=False)["model_state_dict"]
        else:
            torch.manual_seed(a.seed)
            sd = rs.init_state_dict(rs.resnet18_spec(3, 3, size, a.pooling))
        channels = int(sd["conv1.weight"].shape[1])
        images = torch.randn(a.images, channels, size, size, generator=torch.Generator().manual_seed(a.seed + 1)) * a.image_scale
        for pf in a.pf:
            e = expected_wraps(sd, images, pf, pooling=a.pooling)
            per_image = {k: e[k] / a.images for k in ("conv2d", "affine_eval", "linear", "total")}
            print(json.dumps({"metric": "expected_truncation_wraps", "size": size, "precision_fractional": pf, "images": a.images,
                              "image_scale": a.image_scale, **{k + "_per_image": float(f"{v:.4g}") for k, v in per_image.items()},
                              "images_per_wrap": None if per_image["total"] == 0 else float(f"{1 / per_image['total']:.4g}"),
                              "largest_z_over_2_62": float(f"{e['max_ratio']:.4g}")}))


if __name__ == "__main__":
    main()
