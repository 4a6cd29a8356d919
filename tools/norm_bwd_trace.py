#!/usr/bin/env python3
"""Per-layer table of the norm layers' backward kernels in a DP-SGD step, from a rocprofv3 rocpd database of
`tools/train_loop_bench.py --dp --dp_norm {frozen,group} --modes eager` (bf16, max pooling):

    python tools/norm_bwd_trace.py x_results.db frozen|group [out.txt] [--batch 256] [--size 224]

frozen: one `bn_frozen_bwd_kernel` launch per norm layer (20 per step).  group: a reduction launch
(`gn_sample_reduce_kernel` / `gn_colreduce2_kernel`) + `gn_bwd_apply_kernel` per layer; the stem runs fused with the max
pool there and is listed apart.  Launches are matched to layers by their order in the backward pass (blocks last to first:
bn2, bn1, then the downsample norm of a transition block; the stem last); per layer the median over the steps of the trace
(the first two are dropped).  GB/s = the bytes the pass must move / duration: y + dz (+ 1 mask byte per 16 of y where the
layer has a residual) read, dy written — at these shapes the masked gradient g_out is never written (every identity
block's conv1 takes primia_conv2d_dgrad_masked_acc).  The GroupNorm pair reads y + dz (+ mask) twice."""
import argparse
import re
import sqlite3
import statistics


def layers(batch, size):
    """[(name, elements, has_mask)] in backward order."""
    out = []
    hw = size // 4
    dims = {l: ((hw >> (l - 1)) ** 2, 64 << (l - 1)) for l in (1, 2, 3, 4)}
    for l in (4, 3, 2, 1):
        HW, C = dims[l]
        n = batch * HW * C
        for b in (1, 0):
            out.append((f"layer{l}.{b}.bn2", n, True))
            out.append((f"layer{l}.{b}.bn1", n, False))
            if b == 0 and l > 1:
                out.append((f"layer{l}.0.downsample.1", n, True))
    out.append(("bn1 (stem)", batch * (size // 2) ** 2 * 64, False))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("kind", choices=("frozen", "group"))
    ap.add_argument("out", nargs="?")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    a = ap.parse_args()
    db, kind, batch, size = a.db, a.kind, a.batch, a.size
    cur = sqlite3.connect(db).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    namecol = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rows = cur.execute(f"select {namecol}, start, end from kernels order by start").fetchall()
    marks = [i for i, r in enumerate(rows) if "nchw_to_nhwc" in r[0]]
    apply_name = "bn_frozen_bwd_kernel" if kind == "frozen" else "gn_bwd_apply_kernel"
    steps = [rows[i:j] for i, j in zip(marks[:-1], marks[1:])]
    steps = [st for st in steps if any(apply_name in n for n, _, _ in st)][2:]      # (whole steps only; two warm-up steps)
    if not steps:
        raise SystemExit("fewer than 3 whole steps in the trace")
    reduce_names = () if kind == "frozen" else ("gn_sample_reduce_kernel", "gn_colreduce2_kernel")
    lay = layers(batch, size)
    if kind == "group":
        lay = lay[:-1]                       # (the stem: primia_gn_relu_maxpool_bwd, another kernel pair)
    per = [[] for _ in lay]                  # per layer: [(reduce us, apply us)] over the steps
    for st in steps:
        app = [(e - s) / 1e3 for n, s, e in st if apply_name in n]
        # GnBwdFn reductions only (MODE 1 / the backward functor): the forward statistics use GnStatsFn
        red = [(e - s) / 1e3 for n, s, e in st if any(r in n for r in reduce_names) and "GnBwdFn" in n]
        if len(app) != len(lay) or (reduce_names and len(red) != len(lay)):
            raise SystemExit(f"a step has {len(app)} apply / {len(red)} reduce launches, expected {len(lay)}")
        for i in range(len(lay)):
            per[i].append((red[i] if reduce_names else 0.0, app[i]))
    lines = [f"{kind}: {len(steps)} steps, batch {batch}, {size} x {size}, bf16",
             f"{'layer':24s} {'MB to move':>10s} {'reduce us':>9s} {'apply us':>9s} {'total us':>9s} {'GB/s':>7s}"]
    tot = 0.0
    for (name, n, mask), ts in zip(lay, per):
        red_us, app_us = statistics.median(t[0] for t in ts), statistics.median(t[1] for t in ts)
        mb = (3 * 2 * n + (n // 8 if mask else 0)) / 1e6
        lines.append(f"{name:24s} {mb:10.1f} {red_us:9.1f} {app_us:9.1f} {red_us + app_us:9.1f} "
                     f"{mb / (red_us + app_us) * 1e3:7.0f}")
        tot += red_us + app_us
    lines.append(f"sum over these layers: {tot:.1f} us per step")
    names = {re.sub(r"\(.*", "", n) for st in steps[:1] for n, _, _ in st if apply_name in n or any(r in n for r in reduce_names)}
    lines.append("kernels: " + "; ".join(sorted(names)))
    out = "\n".join(lines)
    print(out)
    if a.out:
        open(a.out, "w").write(out + "\n")


if __name__ == "__main__":
    main()
