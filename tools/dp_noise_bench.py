#!/usr/bin/env python3
"""Time per call of DP-SGD's noise step at the gradient arena's size (P = 11,178,051 fp32): today's pair — torch.randn
into a P-element tensor, then primia_dp_add_noise — against the fused primia_dp_noise_add + primia_u64_add (noise drawn
from the ChaCha20 keystream in registers, csrc/dp_noise.hip).

The two alternate in one process (pair, fused, pair, fused, ...); a round is `--calls` back-to-back calls between two
device events, after two untimed rounds of each.  Prints one JSON line: per form the median, minimum and maximum over
the rounds of microseconds per call.  Needs a GPU (there is no CPU path)."""
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
    ap.add_argument("--n", type=int, default=11178051)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dp_noise_bench needs a GPU")
    from primia_amd._lib import call
    from primia_amd.dp_noise import DeviceNoise

    dev = torch.device("cuda", 0)
    g = torch.zeros(a.n, dtype=torch.float32, device=dev)
    noise = DeviceNoise(dev)
    sigma, inv_batch = 1.3, 0.5         # (0.5 keeps g bounded over thousands of calls)

    def pair():
        z = torch.randn(a.n, dtype=torch.float32, device=dev)
        call("primia_dp_add_noise", g, z, a.n, sigma, inv_batch)

    def fused():
        noise.add_to(g, a.n, sigma, inv_batch)

    forms = {"randn_plus_add_noise": pair, "fused_chacha": fused}
    times = {k: [] for k in forms}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(-2, a.rounds):
        for k, f in forms.items():
            e0.record()
            for _ in range(a.calls):
                f()
            e1.record()
            e1.synchronize()
            if r >= 0:
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    out = {"metric": "dp_noise_call", "n": a.n, "rounds": a.rounds, "calls_per_round": a.calls,
           "device": torch.cuda.get_device_name(0)}
    for k, ts in times.items():
        out[k] = {"us_per_call": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}
    out["fused_over_pair"] = round(out["fused_chacha"]["us_per_call"] / out["randn_plus_add_noise"]["us_per_call"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
