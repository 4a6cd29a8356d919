"""Mint tests/golden/conv_routes.npz: what every host-side convolution query of the library answers, per
(shape, dtype, option setting).

    python tests/golden/make_conv_routes_golden.py

The queries need no GPU (the CU count the linear-halo tile choice reads falls back to 256, the MI355X's own).  The table
was minted ONCE, from a build of the commit BEFORE the dispatch was moved onto one route decision per pass
(csrc/conv_route.h); tests/test_conv_routes_host.py imports the shapes, settings and `table()` from here and holds
the library to it.  Mint it again only when a kernel's shape rules change on purpose, and say so in that commit.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
OUT = os.path.join(HERE, "conv_routes.npz")

BF16, F32 = 1, 0
DTYPES = (BF16, F32)

# (option, value) pairs set on top of the defaults; the options are reset after each setting
OPTIONS = ("lh2", "lh4", "lh2_bm", "s2lh", "c64_blocks")
SETTINGS = ((), (("lh2", 0),), (("lh4", 0),), (("lh2_bm", 196),), (("lh2_bm", 392),), (("s2lh", 0),), (("s2lh", 2),),
            (("s2lh", 7),), (("c64_blocks", 2),), (("c64_blocks", 300),))

QUERIES = ("kernel_id fwd", "kernel_id dgrad", "stat_slots_for", "stats_per_tile", "fwd_pair_ok", "dgrad_bnsums_slots",
           "dgrad_masked_acc_ok", "dgrad_masked_acc_bnsums_slots", "dgrad_pair_bnsums_slots", "wgrad_ws_bytes",
           "wgrad_pair_ws_bytes", "wgrad_group_size 2", "wgrad_group_size 4", "wgrad_group_ws_bytes 2",
           "wgrad_group_ws_bytes 3", "wgrad_group_ws_bytes 4", "wgrad_persample_slab_bytes", "wgrad_kernel_id",
           "wgrad_persample_kernel_id")


def _resnet18(n, size):
    """The eleven distinct convolutions of ResNet-18 at a square input: N, H, W, C, K, R, S, stride, pad."""
    out = [(n, size, size, 4, 64, 7, 7, 2, 3)]
    h = size // 4
    out.append((n, h, h, 64, 64, 3, 3, 1, 1))
    c = 64
    for k in (128, 256, 512):
        out.append((n, h, h, c, k, 3, 3, 2, 1))
        out.append((n, h, h, c, k, 1, 1, 2, 0))
        h //= 2
        out.append((n, h, h, k, k, 3, 3, 1, 1))
        c = k
    return out


def shapes():
    sys.path.insert(0, ROOT)
    from tests import conv_bounds as cb

    s = []
    for size in (224, 64):
        for n in (1, 2, 32, 256, 257):
            s += _resnet18(n, size)
    for c in cb.FWD_DGRAD_CASES + cb.WGRAD_CASES:
        s.append((c.N, c.H, c.H, 4 if c.R == 7 else c.C, c.K, c.R, c.R, c.stride, c.pad))
    for w in (27, 28, 29, 30, 31):                       # around the linear-halo widths (forward 30, kernel 28)
        s += [(2, w, w, 128, 128, 3, 3, 1, 1), (2, 5, w, 256, 128, 3, 3, 1, 1), (300, w, w, 128, 256, 3, 3, 1, 1)]
    for h in (7, 15, 29):                                # odd H at stride 2: no parity classes
        s += [(4, h, h, 64, 128, 3, 3, 2, 1), (4, h, h, 64, 128, 1, 1, 2, 0), (4, h, 16, 256, 512, 3, 3, 2, 1)]
    s += [(8, 14, 14, 192, 128, 3, 3, 1, 1), (8, 14, 14, 128, 192, 3, 3, 1, 1), (8, 14, 14, 192, 192, 3, 3, 1, 1),
          (8, 28, 28, 64, 192, 3, 3, 2, 1), (8, 28, 28, 192, 256, 3, 3, 2, 1), (8, 28, 28, 192, 256, 1, 1, 2, 0)]
    s += [(4, 9, 9, 320, 64, 3, 3, 1, 0), (4, 9, 9, 320, 128, 3, 3, 1, 0), (4, 9, 9, 64, 64, 3, 3, 1, 0)]
    s += [(32, 14, 14, 256, 256, 1, 1, 1, 0), (32, 14, 14, 128, 256, 3, 3, 1, 1)]
    # one shape on each side of each element limit: N H W 64 = 2^31 (64 -> 64), M max(C, K) = 2^30 (linear halo, patch, parity planes)
    for n in (10699, 10700):
        s += [(n, 56, 56, 64, 64, 3, 3, 1, 1), (n, 28, 28, 128, 128, 3, 3, 1, 1)]
    for n in (5349, 5350):
        s += [(n, 56, 56, 64, 64, 3, 3, 1, 1), (n, 56, 56, 64, 128, 3, 3, 2, 1), (n, 56, 56, 64, 128, 1, 1, 2, 0)]
    for n in (2674, 2675):
        s += [(n, 28, 28, 512, 512, 3, 3, 1, 1), (n, 28, 28, 128, 512, 3, 3, 1, 1)]
    return list(dict.fromkeys(s))


def _ds_of(s):
    n, h, w, c, k = s[:5]
    return (n, h, w, c, k, 1, 1, 2, 0)


def table(L):
    """int64 [settings][shapes][dtypes][queries] from the loaded library module `L` (primia_amd._lib)."""
    shp = shapes()
    out = np.zeros((len(SETTINGS), len(shp), len(DTYPES), len(QUERIES)), np.int64)
    q = L.query
    L.lib().primia_reset_options()
    try:
        for si, setting in enumerate(SETTINGS):
            for name, value in setting:
                L.set_option(name, value)
            for hi, s in enumerate(shp):
                d = L.ConvDesc.make(*s)
                # the partner of the pair queries: the 1x1 / 2 downsample beside a 3x3 / 2, else the layer itself
                d2 = L.ConvDesc.make(*_ds_of(s)) if (s[5], s[7]) == (3, 2) else d
                for di, dt in enumerate(DTYPES):
                    out[si, hi, di] = (
                        q("primia_conv_kernel_id", d, 0, dt), q("primia_conv_kernel_id", d, 1, dt),
                        q("primia_conv_stat_slots_for", d, dt), q("primia_conv_stats_per_tile", d, dt),
                        q("primia_conv_fwd_pair_ok", d, d2, dt), q("primia_conv_dgrad_bnsums_slots", d, dt),
                        q("primia_conv_dgrad_masked_acc_ok", d, dt), q("primia_conv_dgrad_masked_acc_bnsums_slots", d, dt),
                        q("primia_conv_dgrad_pair_bnsums_slots", d, dt), q("primia_conv_wgrad_ws_bytes", d, dt),
                        q("primia_conv_wgrad_pair_ws_bytes", d, d2, dt), q("primia_conv_wgrad_group_size", d, 2, dt),
                        q("primia_conv_wgrad_group_size", d, 4, dt), q("primia_conv_wgrad_group_ws_bytes", d, 2, dt),
                        q("primia_conv_wgrad_group_ws_bytes", d, 3, dt), q("primia_conv_wgrad_group_ws_bytes", d, 4, dt),
                        q("primia_conv_wgrad_persample_slab_bytes", d, dt), q("primia_conv_wgrad_kernel_id", d, dt),
                        q("primia_conv_wgrad_persample_kernel_id", d, dt))
            L.lib().primia_reset_options()
    finally:
        L.lib().primia_reset_options()
    return out


def settings_array():
    """SETTINGS as integers: [setting][0] = index into OPTIONS (-1: the defaults), [1] = value."""
    return np.array([(OPTIONS.index(s[0][0]), s[0][1]) if s else (-1, 0) for s in SETTINGS], np.int64)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from primia_amd import _lib

    values = table(_lib)
    np.savez_compressed(OUT, shapes=np.array(shapes(), np.int64), dtypes=np.array(DTYPES, np.int64),
                        settings=settings_array(), values=values)
    ids = set(values[..., [0, 1, 17, 18]].flatten().tolist())
    print(f"{OUT}: {values.shape}, {os.path.getsize(OUT)} bytes, ids {sorted(ids)}")
