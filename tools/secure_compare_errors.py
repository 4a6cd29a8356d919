"""What the width of the FSS comparison does to an encrypted forward: the 8-block network of
tests/secure_batch_nets.py at 32 x 32, both parties in this process, at pf in {3, 6} and fss_bits in {32, 40, 64}.
    python tools/secure_compare_errors.py [--images 4] [--seed 5]
Per setting: the comparisons made, those whose opened bit differs from [d <= 0] (the context's `le` is wrapped to reconstruct
the difference d as well -- here only: a deployment never opens it), and max |logit - float64 plaintext logit|.  The step-by-step
chain runs (every comparison goes through `le`); the fused kernels compute the same bits."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from primia_amd.secure import Dealer, SecureContext, SecureResNet18, _default_blocks
from tests.secure_batch_nets import plain_forward, resnet18


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--seed", type=int, default=5, help="debug seed of the dealer (the same masks at every width, reduced to it)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = resnet18(32, 320)
    images = torch.randn(a.images, 3, 32, 32, generator=torch.Generator().manual_seed(321))
    print(f"{'pf':>3} {'fss_bits':>8} {'comparisons':>12} {'wrong':>8} {'largest |d|':>14} {'max |logit - plaintext|':>24}")
    for pf in (3, 6):
        plain = plain_forward(sd, images, _default_blocks(), pf)
        for bits in (32, 40, 64):
            ctx = SecureContext(Dealer(dev, seed=a.seed, fss_bits=bits), 10, pf)
            ctx.local_fused = False
            seen = {"n": 0, "wrong": 0, "top": 0}
            le = ctx.le

            def counting_le(x1, x2):
                bit = le(x1, x2)
                d = ctx.reconstruct(ctx.sub(x1, x2)).reshape(-1)
                got = ctx.reconstruct(bit).reshape(-1)
                seen["n"] += d.numel()
                seen["wrong"] += int((got != (d <= 0).to(got.dtype)).sum())
                seen["top"] = max(seen["top"], int(d.abs().max()))
                return bit

            ctx.le = counting_le
            logits = SecureResNet18(ctx, sd, 32)(images.to(dev)).cpu().numpy().astype(np.float64)
            err = float(np.abs(logits - plain).max())
            assert seen["n"] == ctx.stats["dif_evals"]
            print(f"{pf:>3} {bits:>8} {seen['n']:>12} {seen['wrong']:>8} {seen['top']:>14} {err:>24.6f}")
            print(json.dumps({"pf": pf, "fss_bits": bits, "images": a.images, "comparisons": seen["n"], "wrong": seen["wrong"],
                              "largest_abs_d": seen["top"], "max_abs_logit_error": round(err, 6),
                              "classes": logits.argmax(axis=1).tolist(), "plaintext_classes": plain.argmax(axis=1).tolist()}),
                  file=sys.stderr)


if __name__ == "__main__":
    main()
