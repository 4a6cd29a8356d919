#!/usr/bin/env python3
"""Headline benchmark: ResNet-18 federated-client training throughput on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full]

A "step" is one pass of the hot path over one synthetic batch on every client: forward, loss,
backward, SGD (lr 1e-4, wd 5e-4 — the reference's pneumonia-resnet-pretrained.ini), plus, for
N > 1, the FedAvg exchange every `sync_every_n_batch` = 3 steps (BASELINE.json configs[2]).
N = 1 is BASELINE.json configs[1]: bf16, batch 256, 3x224x224 synthetic, inputs resident in HBM.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps, writes
--dump-outputs and prints the contract fields with what the timed steps give beside them.
Everything else the benchmark measures runs only under --full, whose line also carries
  sustained    : the same steps over >= --sustain-s seconds (N = 1)
  roofline     : MFMA roofline of the dominant convolution kernel, measured live with HIP events
                 on the launch stream; algorithmic FLOPs = 2*MACs of the layers it ran
                 (10.881 GFLOP / image over fwd + dgrad + wgrad)
  cpu_baseline : the oracle (torch-CPU fp32 restatement of the reference step) timed on the host
                 cores on a bounded sample, rank 0 at N = 1 only
  encrypted_inference, dp_sgd : the other BASELINE metrics, each from a child process (N = 1)
  collective, cpu_baseline_b2 : which collective ran on which GPUs, and BASELINE.md B2 (N > 1)
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.3}  # dense, MI355X_MICROARCH.md
GFLOP_PER_IMAGE = 10.881                            # SURVEY.md §8d (fwd 3.627 + bwd 7.254)
TRAFFIC_FILE = "r06_hbm_traffic.json"               # rocprofv3 PMC passes over this command, see tools/hbm_traffic.py


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)      # >= 20 warm-up + >= 100 timed steps
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beside the headline: sustained clock, roofline, CPU baseline, encrypted "
                         "inference, DP-SGD, collective identification (the --no-* switches and --sustain-s trim them)")
    ap.add_argument("--sustain-s", type=float, default=5.0, help="length of the extra sustained-clock run at N = 1 (0: skip)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--sync-every", type=int, default=3)
    ap.add_argument("--secure-aggregation", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--dp", action="store_true", help="DP-SGD step (GroupNorm net, clip 1.0, noise 1.3): BASELINE configs[3]")
    ap.add_argument("--no-secure", action="store_true", help="skip the encrypted-inference leg (second BASELINE metric) and the DP-SGD leg: the A/B tools' form")
    ap.add_argument("--no-dp-leg", action="store_true", help="skip the DP-SGD leg (BASELINE configs[3]) of the N = 1 line")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel from Python instead of replaying a hipGraph")
    ap.add_argument("--cpu-baseline-batch", type=int, default=256)   # N = 256
    ap.add_argument("--no-fuse-sgd", action="store_true", help="gradient finalize, SGD and weight refresh as three passes")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE",
                    help="primia_set_option(NAME, VALUE) before anything is built (A/B runs; csrc/options.h)")
    ap.add_argument("--lib", default=None, metavar="PATH",
                    help="load this build of the kernel library instead of primia_amd/libprimia_hip.so (same-box A/B of two "
                         "builds; probe builds: python -m primia_amd.build --probe)")
    ap.add_argument("--engine-opt", action="append", default=[], metavar="NAME=VALUE",
                    help="ResNet18Engine(options={NAME: VALUE}) (schedule switches of the engine)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last one computed (logits, loss, weights) as DIR/<name>.npy "
                         "(rank 0): two builds run with the same arguments can then be compared output for output")
    return ap.parse_args()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """Write {name: tensor} as out_dir/<name>.npy in float32.  When the total would exceed DUMP_LIMIT_BYTES, the largest
    array is replaced by a fixed, seeded sample of its elements (<name>.npy) plus their flat indices (<name>_index.npy)."""
    import numpy as np

    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(v.nbytes for v in host.values())
    if total > DUMP_LIMIT_BYTES:
        big = max(host, key=lambda k: host[k].nbytes)
        flat = host[big].reshape(-1)
        # 4 bytes of value + 4 bytes of index per element; 4 KB left for the .npy headers
        keep = (DUMP_LIMIT_BYTES - 4096 - (total - flat.nbytes)) // 8
        idx = np.sort(np.random.default_rng(0).choice(flat.size, size=keep, replace=False)).astype(np.int32)
        host[big], host[big + "_index"] = flat[idx], idx
    os.makedirs(out_dir, exist_ok=True)
    for k, v in host.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)


def host_cpu():
    """(model name, physical cores, logical cpus) of the box the benchmark runs on."""
    model, phys = "unknown", set()
    try:
        pid = cid = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name":
                model = v
            elif k == "physical id":
                pid = v
            elif k == "core id":
                cid = v
            elif not k and pid is not None:
                phys.add((pid, cid))
                pid = cid = None
    except OSError:
        pass
    logical = os.cpu_count() or 1
    return model, (len(phys) or logical), logical


def cpu_baseline(batch, size, budget_s=30.0):
    """the oracle train step (torch-CPU fp32 — what a PySyft VirtualWorker executes natively) at the
    benchmark's own batch size.  torch-CPU stops scaling long before a big node's core count on this workload, so the
    thread count is chosen first (one step each at a quarter batch on 32 / 64 / all physical cores) and `value` is the
    BEST count's rate over >= 5 full-batch steps; the probe's rates are reported beside it."""
    from oracle import train_oracle as O
    from primia_amd import resnet_spec as rs

    model, phys, logical = host_cpu()
    torch.manual_seed(42)
    sd0 = rs.init_state_dict(rs.resnet18_spec(3, 3, size, "max"))
    x = torch.randn(batch, 3, size, size)
    y = torch.randint(0, 3, (batch,))

    def sample(threads, nb, min_steps, budget):
        torch.set_num_threads(threads)
        sd = {k: v.clone() for k, v in sd0.items()}
        O.train_step(sd, x[:nb], y[:nb], 1e-4, 5e-4)  # warm-up
        n, t0 = 0, time.perf_counter()
        while True:
            O.train_step(sd, x[:nb], y[:nb], 1e-4, 5e-4)
            n += 1
            el = time.perf_counter() - t0
            if n >= min_steps and (el > budget or n >= 10):
                break
        return round(nb * n / el, 2), n

    counts = sorted({c for c in (32, 64, phys) if c <= phys} or {phys})
    probe = {c: sample(c, max(8, batch // 4), 1, 0.0)[0] for c in counts}
    best = max(probe, key=probe.get)
    v, n = sample(best, batch, 5, budget_s)
    torch.set_num_threads(1)      # (the encrypted-inference child that follows is host-launch-bound: leave it the cores)
    return {"value": v, "unit": "images/s", "cores": best, "kind": "port", "cpu_model": model, "physical_cores": phys,
            "logical_cpus": logical,
            "sample": f"{n} fp32 train steps of batch {batch} at {size}x{size} on {best} threads, the best of "
                      f"{counts} (oracle/train_oracle.py, torch-CPU; BASELINE.md B1)",
            "thread_probe": {str(c): r for c, r in probe.items()}}


def roofline(eng, a, dtype, local_step):
    """The `roofline` field of a --full line."""
    # ---- roofline leg: per-launch HIP events around every convolution kernel ----------------------
    # One untimed eager step first (the timed region replays graphs), then `nprof` profiled steps.  A launch's
    # duration is the MEDIAN over the profiled steps: the events bracket the host-side call too, so a host hiccup
    # between the two records (GC, a page fault) would otherwise be booked as kernel time.
    local_step(0)
    torch.cuda.synchronize()
    eng.prof = []
    nprof = 5
    for i in range(nprof):
        local_step(i)
    torch.cuda.synchronize()
    # Launches are grouped by the kernel that serves them (the library's dispatch rules: conv_igemm.hip,
    # conv_wgrad.hip) so that every group's average duration can be checked against the rocprofv3
    # per-kernel averages under profiles/.
    # The library itself says which kernel its dispatch rules pick for a layer (primia_conv_kernel_id, include/primia_hip.h),
    # so runs under PRIMIA_LH2=0 / PRIMIA_WGP32=0 / ... are labelled with what ran.  Forward and data gradient of the
    # wide 3x3 layers are ONE kernel (same code, flipped taps) and therefore one family.
    from primia_amd import _lib
    from primia_amd._lib import query

    KNAME = {1: "conv_igemm_kernel", 5: "conv_s2lh_kernel (stride-2 3x3 + 1x1, fwd + dgrad)", 2: "conv3x3_c64_kernel (fwd + dgrad)", 4: "conv3x3_lh2_kernel (fwd + dgrad)",
             6: "conv3x3_lh4_kernel (fwd + dgrad)",
             13: "conv_wgrad_dma_kernel (per-tap, stride 2 / 1x1)", 14: "conv_wgrad_kernel (per-tap, stride 2 / 1x1)",
             16: "conv_wgrad_patch33_kernel + wgrad_patch32_reduce_kernel",
             18: "conv_wgrad_patch33lw_kernel + wgrad_patch32_reduce_kernel",
             17: "conv_wgrad_tap_kernel + wgrad_tile_reduce_kernel (per-tap, stride 2 / 1x1)"}
    dtc = _lib.dtype_code(dtype)

    def family(kind, name):     # (also used as family_of below)
        sp = eng.convs[name].spec
        if sp.k == 7:
            if kind != "wgrad":
                return "stem_conv_fwd_kernel"
            # (fused: the kernel also forms its dy tiles from y / dpooled / argmax — bn1, relu and maxpool backward)
            return "stem_conv_wgrad_kernel<fused>" if getattr(eng, "stem_bwd_fused_active", False) else "stem_conv_wgrad_kernel"
        d = eng.convs[name].desc
        if kind == "wgrad":
            return KNAME[query("primia_conv_wgrad_kernel_id", d, dtc)]
        kid = query("primia_conv_kernel_id", d, 0 if kind == "fwd" else 1, dtc)
        return KNAME.get(kid, "kernel id %d" % kid) + ("<%s>" % kind if kid == 1 else "")

    family_of = family
    per_launch = {}
    for kind, name, flops, e0, e1 in eng.prof:
        per_launch.setdefault((kind, name), (flops, []))[1].append(e0.elapsed_time(e1))
    launch_table = per_launch
    agg, fam, layers = {}, {}, {}
    for (kind, name), (flops, samples) in per_launch.items():
        samples.sort()
        layers[f"{kind}:{name}"] = round(samples[len(samples) // 2] * 1e3, 1)     # median launch, us
        ms = samples[len(samples) // 2] * nprof   # median launch, scaled so the tables below stay per-nprof sums
        for table, key in ((agg, kind), (fam, family(kind, name))):
            d = table.setdefault(key, {"ms": 0.0, "flops": 0.0, "launches": 0})
            d["ms"] += ms
            d["flops"] += flops * nprof
            d["launches"] += nprof
    eng.prof = None
    peak = MFMA_PEAK_TFLOPS[a.dtype]

    def summarise(table):
        return {k: {"tflops": round(d["flops"] / (d["ms"] * 1e-3) / 1e12, 2), "ms_per_step": round(d["ms"] / nprof, 4),
                    "avg_launch_us": round(d["ms"] * 1e3 / d["launches"], 2),
                    "launches_per_step": d["launches"] // nprof} for k, d in table.items()}

    kernels, by_pass = summarise(fam), summarise(agg)
    dom = max(fam, key=lambda k: fam[k]["ms"])
    conv_ms = sum(d["ms"] for d in agg.values()) / nprof
    conv_fl = sum(d["flops"] for d in agg.values()) / nprof
    # `traffic` needs PMC counters (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, tools/profile_round.sh),
    # which cannot be collected from inside the timed process.  The committed passes over this same command carry the
    # sha256 of the library sources they ran (primia_amd.build.source_digest): `traffic` is their per-launch figure when
    # that digest equals the one of the code running NOW, null otherwise (then `traffic_offline` still names the file,
    # marked stale).
    traffic = None
    traffic_offline = None
    tpath = os.path.join(ROOT, "profiles", TRAFFIC_FILE)
    if os.path.exists(tpath) and a.batch == 256 and a.size == 224 and a.dtype == "bf16":
        from primia_amd.build import source_digest
        rec = json.load(open(tpath))
        key = dom.split(" ")[0].split("<")[0]     # the kernel that ran; no record for it -> traffic_offline stays null
        if key in rec:
            same = rec.get("_source_sha256") == source_digest()
            per_launch = rec[key].get("hbm_bytes_per_launch")
            traffic_offline = {"hbm_bytes_per_launch": per_launch, "kernel": key,
                               "source": "profiles/" + TRAFFIC_FILE, "same_sources_as_this_run": same}
            if same:
                traffic = per_launch
    # the wide 3x3 / stride-1 layers (layer2-4 forward + data gradient) are ONE algorithm on two kernels — conv3x3_lh2_kernel
    # (392-pixel tiles) and conv3x3_lh4_kernel (196-pixel tiles, loader waves): reported together beside the dominant kernel
    wide = [k for k in fam if k.startswith("conv3x3_lh2_kernel") or k.startswith("conv3x3_lh4_kernel")]
    family = None
    if wide:
        f_ms, f_fl, f_n = (sum(fam[k][q] for k in wide) for q in ("ms", "flops", "launches"))
        family = {"kernels": wide, "tflops": round(f_fl / (f_ms * 1e-3) / 1e12, 2), "frac": round(f_fl / (f_ms * 1e-3) / 1e12 / peak, 4),
                  "ms_per_step": round(f_ms / nprof, 4), "avg_launch_us": round(f_ms * 1e3 / f_n, 2), "launches_per_step": f_n // nprof}
        # the family's FORWARD launches alone: since round 5 six of its data-gradient launches also form the BatchNorm backward
        # sums of the layer in front of them in their write-back (engine.dgrad_bnsums: the reduction passes they replace are
        # gone from the step), so the family's own time per FLOP went UP while the step's went down
        fw = [(fl_, sm_) for (kind_, name_), (fl_, sm_) in launch_table.items() if kind_ == "fwd" and family_of(kind_, name_) in wide]
        if fw:
            w_ms = sum(sorted(sm_)[len(sm_) // 2] for _, sm_ in fw)
            w_fl = sum(fl_ for fl_, _ in fw)
            family["forward_only"] = {"launches_per_step": len(fw), "tflops": round(w_fl / (w_ms * 1e-3) / 1e12, 2),
                                      "frac": round(w_fl / (w_ms * 1e-3) / 1e12 / peak, 4)}
            family["note"] = ("data-gradient launches with engine.dgrad_bnsums include the BatchNorm backward sums of the layer "
                              "in front of them")
    roof = {"bound": "mfma", "kernel": dom,
            "kernel_is": "the kernel (one C-ABI call; a weight-gradient call = the kernel + its ordered reduce) with the most time per step",
            "launch": "median over %d steps of the HIP-event bracket around one C-ABI call" % nprof,
            "achieved": kernels[dom]["tflops"], "peak": peak, "unit": "TFLOP/s",
            "frac": round(kernels[dom]["tflops"] / peak, 4), "traffic": traffic, "traffic_offline": traffic_offline,
            # (`frac` is priced at the nominal 2.4 GHz dense-bf16 peak; what the part sustains under matrix load is measured in
            # profiles/r04_mfma_ceilings.txt and discussed in DESIGN.md — no constants from there are repeated here)
            "wide3x3_family": family,
            "all_conv": {"tflops": round(conv_fl / (conv_ms * 1e-3) / 1e12, 2), "ms_per_step": round(conv_ms, 3),
                         "frac": round(conv_fl / (conv_ms * 1e-3) / 1e12 / peak, 4)},
            "kernels": kernels, "by_pass": by_pass, "layers_us": layers}
    return roof


def main():
    a = parse()
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        # `python bench.py --gpus N` on its own: start the N ranks as a CHILD (one process per GPU under
        # torch.distributed.run) before this process has made any GPU call, relay rank 0's JSON line and the exit
        # code.  (Never re-exec a process that touched the GPU; this parent never does.)
        import socket
        import subprocess

        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
        line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith('{"metric"')), None)
        if line is not None:
            print(line)
        else:
            sys.stdout.write(r.stdout)
        raise SystemExit(r.returncode if (r.returncode or line is not None) else 1)
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {a.gpus}, "
                         "or run `python bench.py --gpus N` on its own")
    import torch.distributed as dist

    ndev = torch.cuda.device_count()
    dev = torch.device("cuda", local_rank % max(ndev, 1))
    torch.cuda.set_device(dev)
    if world > 1:
        # RCCL over xGMI ("nccl" IS RCCL on ROCm).  PRIMIA_BENCH_BACKEND=gloo exists only to exercise the
        # N > 1 control flow on a single-GPU box (tests/test_gpu_federated.py).
        backend = os.environ.get("PRIMIA_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from primia_amd import fed
    from primia_amd.engine import ResNet18Engine

    from primia_amd import _lib as _plib

    if a.lib:
        _plib.LIB_PATH = os.path.abspath(a.lib)      # before the first call loads it; no fallback: a missing file raises
    for kv in a.opt:
        k, _, v = kv.partition("=")
        _plib.set_option(k, int(v))
    eopts = {}
    for kv in a.engine_opt:
        k, _, v = kv.partition("=")
        eopts[k] = {"true": True, "false": False}.get(v.lower(), int(v) if v.lstrip("-").isdigit() else v)
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    eng = ResNet18Engine(a.batch, 3, 3, a.size, "max", dtype=dtype, device=dev, norm="group" if a.dp else "batch",
                         options=eopts)
    if a.dp:
        eng.dp_params = {"max_grad_norm": 1.0, "noise_multiplier": 1.3}   # train.py:325-334
    # SGD follows the backward pass directly: gradient finalize + update + weight refresh as one pass per weight tile
    # (what EngineOptimizer("SGD") switches on for the training loops; --no-fuse-sgd: the three unfused passes)
    eng.fuse_sgd_tail = not a.no_fuse_sgd
    torch.manual_seed(42)           # the reference's default seed (pneumonia-resnet-pretrained.ini:17)
    eng.init_weights()
    g = torch.Generator().manual_seed(1000 + rank)
    nbuf = 2
    xs = [torch.randn(a.batch, 3, a.size, a.size, generator=g).to(dev) for _ in range(nbuf)]
    ys = [torch.randint(0, 3, (a.batch,), generator=g).to(dev) for _ in range(nbuf)]
    local_flat = torch.empty_like(eng.flat)
    scratch = torch.empty(eng.flat.numel(), dtype=torch.int64, device=dev) if a.secure_aggregation else None
    # secure aggregation across ranks goes onto the wire under pairwise one-time masks (fed.PairwiseMasks)
    masks = fed.PairwiseMasks.setup(eng.flat.numel(), dev) if (a.secure_aggregation and world > 1) else None
    lr, wd = 1e-4, 5e-4

    def local_step(i):
        eng.forward(xs[i % nbuf])
        eng.loss_backward(ys[i % nbuf])
        eng.sgd_step(lr, wd)

    sync_events = []        # (start, end) HIP events around every timed exchange

    def exchange(i, timed=False):
        """FedAvg over RCCL every `sync_every` batches (torchlib/utils.py:1175: batch_idx > 0 and batch_idx % s == 0)."""
        if world > 1 and i > 0 and i % a.sync_every == 0:
            if timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            fed.fedavg_allreduce(eng.flat, local_flat, None, a.secure_aggregation, 16, 10, None, None, scratch, masks)
            eng.flat.copy_(local_flat)
            eng.refresh_weights()
            if timed:
                e1.record()
                sync_events.append((e0, e1))

    def step(i, timed=False):
        local_step(i)
        exchange(i, timed)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # (the DP step draws its Gaussian noise through torch's default generator, which CUDA-graph capture supports: the
    # Philox offset advances per replay; if a torch build cannot capture it, the fallback below launches eagerly)
    # The local step is ~190 kernel launches; replaying it as a hipGraph (one per input buffer) removes the host
    # launch cost (7.5 -> 6.3 ms per step).  Only the client-local step is captured: the FedAvg exchange — the one
    # collective of the path — is launched between replays, so every rank count runs the same graphs.
    graphs = None
    if not a.no_graph:
        for i in range(2):
            local_step(i)
        barrier()
        graphs = []
        try:
            for b in range(nbuf):
                gph = torch.cuda.CUDAGraph()
                # thread_local: the process group's watchdog thread may touch the runtime while this thread captures
                with torch.cuda.graph(gph, capture_error_mode="thread_local"):
                    local_step(b)
                graphs.append(gph)
        except Exception as e:  # noqa: BLE001 - a rank that cannot capture still measures, launch by launch
            print(f"[bench] rank {rank}: graph capture failed ({type(e).__name__}: {e}); launching eagerly", file=sys.stderr)
            graphs = None
            torch.cuda.synchronize()
        if world > 1:
            # every rank must run the same way (a graph rank would wait for an eager one at each exchange anyway)
            ok = torch.tensor([1 if graphs is not None else 0], device=dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if ok.item() == 0:
                graphs = None

    if graphs is not None:
        def run(i, timed=False):
            graphs[i % nbuf].replay()
            eng.note_replayed_steps(1)
            exchange(i, timed)
    else:
        run = step

    for i in range(a.warmup):
        run(i)
    barrier()
    t0 = time.perf_counter()
    for i in range(a.steps):
        run(i, True)
    barrier()
    dt = time.perf_counter() - t0
    fedavg_ms = None
    if world > 1:
        # the exchange on its own (all-reduce of the 44.75 MB arena + copy back + weight refresh, stream time on this
        # rank; the slowest rank counts) — so that a scaling run shows what the collective costs per sync
        mine = sum(e0.elapsed_time(e1) for e0, e1 in sync_events) / max(1, len(sync_events))
        t = torch.tensor([dt, mine], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt, fedavg_ms = t[0].item(), round(t[1].item(), 3)
    loss = eng.loss.item()
    if a.dump_outputs and rank == 0:
        # the last timed step's results, before the legs below run more steps on the same engine.  Inputs are seeded
        # (weights: torch.manual_seed(42); batches: generator 1000 + rank), so equal arguments mean equal inputs.
        dump_outputs(a.dump_outputs, {"logits": eng.logits, "loss": eng.loss, "weights": eng.flat})
    ms_per_step = dt / a.steps * 1e3
    total_ips = a.batch * world * a.steps / dt
    peak = MFMA_PEAK_TFLOPS[a.dtype]
    out = {
        "metric": "images_per_sec", "value": round(total_ips, 1), "unit": "images/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
        "config": {"workload": f"ResNet-18 federated-client training step (fwd+loss+bwd+SGD), batch {a.batch}/client, "
                               f"3x{a.size}x{a.size}, 1 client per GPU"
                               + (f", FedAvg every {a.sync_every} batches over RCCL" if world > 1 else ""),
                   "batch_per_client": a.batch, "clients": world, "sync_every_n_batch": a.sync_every,
                   "secure_aggregation": bool(a.secure_aggregation), "dp_sgd": bool(a.dp)},
        "images_per_sec_per_client": round(total_ips / world, 1),
        "step_tflops": round(GFLOP_PER_IMAGE * 1e9 * a.batch / (dt / a.steps) / 1e12, 2),
        "step_mfma_frac": round(GFLOP_PER_IMAGE * 1e9 * a.batch / (dt / a.steps) / 1e12 / peak, 4),
        "final_loss": round(loss, 5), "hip_graph": graphs is not None,
        "fedavg_ms_per_sync": fedavg_ms,
    }
    # ---- --full: the legs that measure something besides the headline; a plain run prints the line above ----
    if a.full:
        # A second figure over >= 5 s of back-to-back steps: the 100-step region above lasts ~0.6 s, short enough for the
        # chip to ride its boost clock; this one shows what it sustains (same run() calls, own barriers).
        sustained = None
        if world == 1 and a.sustain_s > 0:
            n_sus = max(a.steps, int(a.sustain_s / (dt / a.steps)) + 1)
            barrier()
            t1 = time.perf_counter()
            for i in range(n_sus):
                run(i)
            barrier()
            dts = time.perf_counter() - t1
            sustained = {"steps": n_sus, "seconds": round(dts, 3), "images_per_sec": round(a.batch * n_sus / dts, 1),
                         "ms_per_step": round(dts / n_sus * 1e3, 3)}
        out["sustained"] = sustained
        out["roofline"] = roofline(eng, a, dtype, local_step)
    if a.full and world > 1:
        # proof that the exchange ran on RCCL with `world` ranks, and BASELINE.md B2 beside it
        ver = None
        try:
            ver = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            pass
        # every rank reports the physical device it ran on (PCI bus id where the runtime gives it)
        try:
            me = torch.cuda.get_device_properties(dev)
            ident = f"{local_rank}:{getattr(me, 'pci_bus_id', '?')}:{getattr(me, 'uuid', '')}"
        except Exception:
            ident = str(local_rank)
        gpu_ids = [None] * world
        dist.all_gather_object(gpu_ids, ident)
        out["collective"] = {"backend": dist.get_backend(), "ranks": dist.get_world_size(), "rccl_version": ver,
                             "op": "all_reduce(SUM) of the 44.75 MB parameter + running-statistics arena per sync",
                             "gpus_seen": sorted(set(gpu_ids))}
        out["cpu_baseline_b2"] = {
            "definition": "BASELINE.md B2: the reference's federated epoch visits its K in-process clients SEQUENTIALLY on the "
                          "host cores (torchlib/utils.py:1159-1174), so its per-client rate is B1 / K and its aggregate rate is B1",
            "K": world, "value_per_client": "cpu_baseline.value of the N = 1 line / %d" % world,
            "note": "cpu_baseline is timed on rank 0 at N = 1 only (bench contract); B1 does not depend on N"}
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(a.cpu_baseline_batch, a.size)
    if a.full and rank == 0 and world == 1 and not a.no_secure:
        # second BASELINE.json metric: encrypted-inference ms/image (3 roles on this GPU), as a child
        # process so that its allocations never share the training engine's pool
        import subprocess

        cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_secure.py"), "--images", "2"]
        if not a.no_cpu_baseline:
            cmd.append("--cpu-sample")
        del eng, xs, ys
        torch.cuda.empty_cache()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        try:
            out["encrypted_inference"] = json.loads(r.stdout.strip().splitlines()[-1])
        except Exception:  # noqa: BLE001 - the primary metric must still be reported
            out["encrypted_inference"] = {"error": (r.stderr or r.stdout)[-300:]}
    if a.full and rank == 0 and world == 1 and not a.dp and not a.no_dp_leg and not a.no_secure and a.dtype == "bf16":
        # BASELINE configs[3] beside the headline: the DP-SGD step (GroupNorm network, per-sample clip 1.0 + Gaussian noise 1.3) at
        # the same batch, as a child process with its own engine — so that the driver's line carries a DP figure, not only
        # profiles/ (VERDICT r05 weak #14).  Same contract: hipGraph replay, 30 timed steps, inputs resident.
        import subprocess

        cmd = [sys.executable, os.path.abspath(__file__), "--dp", "--steps", "30", "--warmup", "5", "--batch", str(a.batch),
               "--size", str(a.size)]
        if a.lib:
            cmd += ["--lib", a.lib]
        try:
            del eng, xs, ys
        except NameError:
            pass
        torch.cuda.empty_cache()
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            d = json.loads(r.stdout.strip().splitlines()[-1])
            out["dp_sgd"] = {"images_per_sec": d["value"], "ms_per_step": d["ms_per_step"], "step_mfma_frac": d["step_mfma_frac"],
                             "steps": d["steps"], "hip_graph": d["hip_graph"], "final_loss": d["final_loss"],
                             "workload": d["config"]["workload"] + ", DP-SGD (per-sample clip 1.0, noise multiplier 1.3, GroupNorm)"}
        except Exception as e:  # noqa: BLE001 - the primary metric must still be reported
            out["dp_sgd"] = {"error": repr(e)[:300]}
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
