#!/usr/bin/env python3
"""us per call of the two launches a Poisson-sampled DP-SGD step adds in front of the step (csrc/dp_sample.hip):
primia_poisson_select over n records (one workgroup walking n in chunks of 8192; timed together with the primia_u64_add
that advances its counter, as DeviceSampler.select issues them) and primia_gather_batch of `capacity` fp32 images (one walk and one view
of the kernel behind the loader's primia_gather_records).
Each figure is the median over --runs timed loops of --calls back-to-back launches between two events (launch-rate
included: what the training loop pays).  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, calls, runs):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls * 1e3)
    return round(statistics.median(out), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="5163,1000000,16777216")
    ap.add_argument("--capacity", type=int, default=382)
    ap.add_argument("--expected_batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--gather_records", type=int, default=1721)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dp_sample_bench needs a GPU")
    from primia_amd import dp_accountant
    from primia_amd._lib import call
    from primia_amd.dp_sampling import DeviceSampler

    dev = torch.device("cuda", 0)
    s = DeviceSampler(dev)
    idx = torch.empty(a.capacity, dtype=torch.int64, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    out = {"metric": "dp_sample", "capacity": a.capacity, "select_us": {}}
    for n in [int(v) for v in a.records.split(",")]:
        thr = dp_accountant.threshold_for((min(a.expected_batch, n - 1), n))
        out["select_us"][str(n)] = timed(lambda: s.select(thr, n, idx, count), max(2, a.calls if n < 10 ** 7 else 3), a.runs)
    n = a.gather_records
    data = torch.randn(n, 3, a.size, a.size, device=dev)
    targets = torch.zeros(n, dtype=torch.int64, device=dev)
    s.select(dp_accountant.threshold_for((a.expected_batch, n)), n, idx, count)
    x = torch.empty(a.capacity, 3, a.size, a.size, device=dev)
    y = torch.empty(a.capacity, dtype=torch.int64, device=dev)
    row = 3 * a.size * a.size
    out["gather_us"] = timed(lambda: call("primia_gather_batch", data, row, n, targets, idx, 0, x, y, a.capacity, 0),
                             a.calls, a.runs)
    kept = int(count[1])
    out["gather_kept"] = kept
    out["gather_GBps"] = round((kept * 2 + (a.capacity - kept)) * row * 4 / out["gather_us"] / 1e3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
