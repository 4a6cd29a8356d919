#!/usr/bin/env python3
"""Per-layer time of the DP-SGD norm pass per sample (views = 1) and per record (--views M, augmentation multiplicity) on
the 20 convolutions of ResNet-18 at --batch slots of --size x --size, bf16, N(0, 1) operands: which kernel serves each layer
(primia_conv_wgrad_record_kernel_id) and the median of --iters device-event timings, the two forms alternating.  The stem
runs primia_stem_conv_wgrad_record_sqnorm on the padded input, as the engine does.  One line per layer, then a JSON line.
Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dp_augmult_layers needs a GPU")
    if a.batch % a.views:
        raise SystemExit("--views must divide --batch")
    from primia_amd import resnet_spec as rs
    from primia_amd._lib import ConvDesc, call, query

    dev = torch.device("cuda", 0)
    spec = rs.resnet18_spec(3, 3, a.size, "max")
    g = torch.Generator(device=dev).manual_seed(7)
    rows, total = [], {1: 0.0, a.views: 0.0}
    # the input height of every convolution: the stem halves, the pool halves, a block's conv1 / downsample see the block's
    # input and conv2 its output
    hw = {spec.stem.name: a.size}
    h = a.size // 4
    for blk in spec.blocks:
        hw[blk.conv1.name] = h
        if blk.down is not None:
            hw[blk.down.name] = h
        h = (h + 2 * blk.conv1.pad - blk.conv1.k) // blk.conv1.stride + 1
        hw[blk.conv2.name] = h
    for c in spec.convs:
        stem = c.name == "conv1"
        H = hw[c.name]
        cin = 4 if stem else c.cin
        d = ConvDesc.make(a.batch, H, H, cin, c.cout, c.k, c.k, c.stride, c.pad)
        dy = torch.randn(a.batch * d.Ho * d.Wo, c.cout, device=dev, generator=g).to(torch.bfloat16)
        if stem:
            x = torch.zeros(a.batch, H + 6, H + 8, 4, device=dev)
            x[:, 3:3 + H, 3:3 + H, :3] = torch.randn(a.batch, H, H, 3, device=dev, generator=g)
            x = x.to(torch.bfloat16)
        else:
            x = torch.randn(a.batch * H * H, cin, device=dev, generator=g).to(torch.bfloat16)
        sq = torch.zeros(a.batch, dtype=torch.float64, device=dev)

        def run(views):
            if stem:
                call("primia_stem_conv_wgrad_record_sqnorm", x, dy, sq, a.batch, H, H, views, 1)
            else:
                call("primia_conv2d_wgrad_record_sqnorm", d, x, dy, sq, views, 1)

        times = {1: [], a.views: []}
        for it in range(3 + a.iters):
            for views in times:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(views)
                e1.record()
                e1.synchronize()
                if it >= 3:
                    times[views].append(e0.elapsed_time(e1) * 1e3)
        med = {v: statistics.median(t) for v, t in times.items()}
        kid = {v: ("stem halo" if stem else query("primia_conv_wgrad_record_kernel_id", d, 1, v)) for v in times}
        for v in med:
            total[v] += med[v]
        rows.append({"layer": c.name, "kernel": kid, "us": {v: round(t, 1) for v, t in med.items()}})
        print("{:24s} views 1: kernel {!s:9s} {:8.1f} us   views {:d}: kernel {!s:9s} {:8.1f} us".format(
            c.name, kid[1], med[1], a.views, kid[a.views], med[a.views]))
        del x, dy
    print(json.dumps({"metric": "dp_norm_pass_layers", "batch": a.batch, "size": a.size, "views": a.views,
                      "total_us": {v: round(t, 1) for v, t in total.items()}, "layers": rows}))


if __name__ == "__main__":
    main()
