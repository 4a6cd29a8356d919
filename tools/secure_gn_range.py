#!/usr/bin/env python
"""Error of the secret-shared GroupNorm against float64 per decade of group variance, for the default form
(oracle_group_norm: the reference's damped Newton iteration) and the wide-range form (oracle_group_norm_wide: --wide_norm),
on the CPU composition of OracleContext methods -- no GPU, no library.  The GPU is held bit-identical to these compositions
(tests/test_gpu_secure_gn_wide.py), so these ARE the layer's figures; DESIGN.md §4 and the bounds in
tests/secure_gn_wide_nets.py quote this output.

    python tools/secure_gn_range.py [--pf 3 6] [--seeds 1 2 3] [--steps 28 30 32 34 36] [--x0 0.01] [--networks]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tests import secure_gn_wide_nets as W                      # noqa: E402
from tests.secure_groupnorm_nets import oracle_group_norm       # noqa: E402

DECADES = [(1e-3, 1e-2), (1e-2, 0.05), (0.05, 1.0), (1.0, 16.0), (16.0, 1e2), (1e2, 1e3), (1e3, 1.2e4)]


def per_decade(err, var):
    out = []
    for lo, hi in DECADES:
        pick = (var >= lo) & (var < hi)
        out.append(err[pick].max() if pick.any() else float("nan"))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pf", type=int, nargs="+", default=[3, 6])
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--steps", type=int, nargs="+", default=[W.STEPS], help="iterate counts to compare on the rsqrt grid")
    ap.add_argument("--x0", type=float, default=W.X0)
    ap.add_argument("--networks", action="store_true",
                    help="also the whole-network figures behind WIDE_NET_TOL (the CPU oracle's comparisons: minutes)")
    args = ap.parse_args()
    np.set_printoptions(linewidth=200)
    head = "  ".join(f"[{lo:g},{hi:g})" for lo, hi in DECADES)
    print(f"wide form: S_IT = {W.S_IT}, x0 = {W.X0}, {W.STEPS} iterates, floor = {W.FLOOR}; "
          f"{4 * (W.STEPS - 1) + 4} dealer requests per norm site (default form: 321)")
    for pf in args.pf:
        # the whole served range at every pf: at pf = 6 the raw squares of large variances meet the ring's headroom
        for label, rng in (("served range of this pf", None), ("whole range", W.VAR_SERVED)):
            if rng is None:
                x, w, b, _ = W.wide_layer_input(pf)
            else:
                kept = W.VAR_SERVED_PF6
                W.VAR_SERVED_PF6 = rng
                x, w, b, _ = W.wide_layer_input(pf)
                W.VAR_SERVED_PF6 = kept
            print(f"\npf = {pf}, [2, 64, 6, 6], {label}: max |error| against float64 F.group_norm per variance band\n"
                  f"{'':28s}{head}   constant group   all")
            for seed in args.seeds:
                for name, fn in (("default", oracle_group_norm), ("wide", W.oracle_group_norm_wide)):
                    err, var = W.layer_error(fn, pf, seed, x, w, b)
                    const = var < 1e-9
                    row = per_decade(err.max(1), np.where(const, -1.0, var))
                    print(f"  seed {seed} {name:8s}          " + "  ".join(f"{e:10.3g}" for e in row) +
                          f"   {err[const].max():10.3g}   {err.max():10.3g}")
    grid = np.geomspace(W.VAR_SERVED[0], W.VAR_SERVED[1], 60)
    print("\nrsqrt_newton: max relative error against v^-1/2 on 60 variances, geometric over", W.VAR_SERVED,
          "; value at v = floor (var = -eps) and at v = eps + floor (a constant group)")
    for steps in args.steps:
        for seed in args.seeds:
            r, vq = W.rsqrt_values(grid, seed, args.x0, steps)
            rel = np.abs(r * np.sqrt(vq) - 1)
            edge, eq = W.rsqrt_values([W.FLOOR / W.S_IT, (10 + W.FLOOR) / W.S_IT], seed, args.x0, steps)
            print(f"  steps {steps} seed {seed}: max {rel.max():.4g} (at v = {vq[rel.argmax()]:.4g}); below 1: {rel[vq < 1].max():.4g}; "
                  f"rsqrt(floor) = {edge[0]:.4g} (exact {eq[0] ** -0.5:.4g}), rsqrt(eps + floor) = {edge[1]:.4g} "
                  f"(exact {eq[1] ** -0.5:.4g})")
    if args.networks:
        print("\nwhole networks at pf = 3, three scaled images, ChaChaDealer(%d): max |logit error| per image against float64"
              % W.NET_DEALER_SEED)
        for name in W.wide_networks():
            err, lo, hi = W.measure_network(name)
            print(f"  {name}: {err.tolist()}; float64 group variances {lo:.4g} to {hi:.4g}")


if __name__ == "__main__":
    main()
