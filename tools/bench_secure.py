"""Encrypted-inference timing (BASELINE.json configs[4], all three roles on one GPU):
ms/image for the online phase (primitives pre-provisioned) and for the dealer (triples + FSS keys).
    python tools/bench_secure.py [--size 224] [--pf 16] [--images 2]
    python tools/bench_secure.py --batch N [--size 224] [--pf 16] [--images 3]     the serving form on N images per pass only
    --pooling avg: the stem of a checkpoint trained with pooling_type = avg (ReLU, then a party-local average pool)
    --norm group:  a GroupNorm state dict (the network of differentially private training): every norm site computes its
                   statistics online -- a Beaver square and an 80-step Newton iteration on batch * 32 values per layer
    --norm folded: the benchmark's BatchNorm state dict after the model owner's fold (primia_amd.secure.fold_batch_norm): the
                   same legs as --norm batch, without the Newton iteration and with one product per norm site
    --faithful_trunc (with --norm folded): the products of conv2d, the folded norm and fc are truncated by
                   SecureContext.trunc_faithful, one more element-wise triple per site
    --wide_norm (with --norm group, --pf 3 to 6): the wide-range GroupNorm at every norm site -- a 32-iterate undamped Newton
                   iteration at a scale of 10^-6 in place of the 80-step damped one (the report names it)
    --reveal class: every pass ends with the secret-shared argmax and opens the class only (classes - 1 rounds of one comparison
                   launch and one select launch on `batch` elements; the report names it)
    --reveal confusion (with --batch): the passes of an encrypted evaluation -- the argmax, then batch * classes equality tests and
                   one [C, B] x [B, C] Beaver product into the shared confusion matrix; seeded labels, nothing opened per pass
    --reveal metrics --eval_images N (with --batch): the confusion passes over N seeded images, then the rank-count tail of the
                   ROC AUC on its own -- classes * N^2 comparisons at 64 bits -- timed with its dealer and on pre-provisioned
                   primitives, next to the same run's per-image online time
    --fss_bits N:  the width of the comparisons, 32 (default, the reference's) to 64: N levels per key and per evaluation (the
                   report names it when it is not 32)"""
import argparse, dataclasses, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from primia_amd import resnet_spec as rs
from primia_amd.secure import Dealer, PreloadedDealer, ProtocolForm, SecureContext, SecureResNet18, fold_batch_norm

def non_default(form):
    """The fields of a ProtocolForm that differ from their defaults, as a dict."""
    return {f.name: getattr(form, f.name) for f in dataclasses.fields(form) if getattr(form, f.name) != f.default}

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--pf", type=int, default=16)
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0,
                    help="time ONLY GraphedSecureInference(batch=N): ms per image online and with the dealer's refill included "
                         "(--images passes each), the static primitive bytes and the largest batch the card admits")
    ap.add_argument("--pooling", choices=("max", "avg"), default="max",
                    help="the stem pool of the served network (a checkpoint's pooling_type); the report names it when it is avg")
    ap.add_argument("--norm", choices=("batch", "group", "folded"), default="batch",
                    help="group: a synthetic GroupNorm(32, C) state dict, no running statistics; folded: the BatchNorm state "
                         "dict of --norm batch, folded by the model owner before sharing (the report names either)")
    ap.add_argument("--faithful_trunc", action="store_true",
                    help="with --norm folded: SecureContext.trunc_faithful at every product site (the report names it)")
    ap.add_argument("--wide_norm", action="store_true",
                    help="with --norm group and --pf 3..6: SecureContext.group_norm(wide=True) at every norm site (the report names it)")
    ap.add_argument("--reveal", choices=("logits", "class", "confusion", "metrics"), default="logits",
                    help="class: the passes end with SecureContext.argmax and open the predicted class only (the report names it); "
                         "confusion (with --batch): the passes of an encrypted evaluation, which add into the shared confusion matrix; "
                         "metrics (with --batch): those passes, then the rank-count tail of the ROC AUC over --eval_images images")
    ap.add_argument("--eval_images", type=int, default=624,
                    help="--reveal metrics: the images of the evaluation whose tail is timed (default 624)")
    ap.add_argument("--fss_bits", type=int, default=32,
                    help="the width of the DIF comparisons (32..64): key bytes and DIF kernel time grow linearly with it (the report "
                         "names it when it is not 32)")
    ap.add_argument("--cpu-sample", action="store_true", help="also time the CPU oracle on a bounded sample")
    ap.add_argument("--no-graph", action="store_true", help="skip the hipGraph replay of the online phase")
    ap.add_argument("--only-fss-roofline", action="store_true",
                    help="run the DIF keygen / eval kernels alone (the command the rocprofv3 --pmc passes of tools/pmc_secure.sh wrap)")
    a = ap.parse_args()
    if a.wide_norm and a.norm != "group":
        ap.error("--wide_norm is a form of the GroupNorm network: pass --norm group (a BatchNorm network: --norm folded)")
    if a.faithful_trunc and a.norm != "folded":
        ap.error("--faithful_trunc covers the products of a folded network: pass --norm folded")
    if a.reveal in ("confusion", "metrics") and not (a.batch and not a.only_fss_roofline):
        ap.error(f"--reveal {a.reveal} is timed in the serving form: pass --batch N")


    def cpu_sample_timings():
        """Bounded CPU sample of the same workload with the oracle, organised like the reference — run BEFORE this process
        touches the GPU (the worker processes are spawned from a process without a HIP context):
          * FSS evaluation above 50,000 elements fans out over N_CORES = max(4, cpu_count()) processes
            (mpc/fss.py:43-44,214-236): a 400k-comparison tensor is evaluated that way (both parties), and on one core;
          * FSS keygen (the crypto provider, mpc/fss.py:47-95) the same way;
          * torch-CPU int64 matmuls of the 21 Beaver products' shapes (3 products x 2 parties each), torch's own threads.
        Returns per-comparison / total-matmul seconds; cpu_sample_report() scales them to one image."""
        import multiprocessing as mp

        import numpy as np
        from oracle import secure_oracle as S

        ncores = max(4, os.cpu_count() or 1)
        n = 400_000
        rng = np.random.default_rng(0)
        alpha = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
        s0 = rng.integers(0, 2 ** 64, size=(2, 2, n), dtype=np.uint64); s0[:, 0] %= 2 ** 63
        x = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
        n1 = 20000
        t0 = time.perf_counter(); S.dif_keygen(alpha[:n1], s0[:, :, :n1]); t_kg1 = (time.perf_counter() - t0) / n1
        t0 = time.perf_counter(); _, keys = S.dif_keygen(alpha, s0); t_kg = (time.perf_counter() - t0) / n
        t0 = time.perf_counter(); [S.dif_eval(b, x[:n1], {k: (v[..., :n1] if hasattr(v, "shape") else v) for k, v in keys[b].items()})
                                   for b in range(2)]; t_ev1 = (time.perf_counter() - t0) / n1
        with mp.get_context("spawn").Pool(ncores) as pool:
            S.use_pool(pool, n_slices=ncores)               # the oracle slices the element axis over the pool (fss.py:214-266)
            [S.dif_eval(b, x, keys[b]) for b in range(2)]   # warm every worker (import numpy, load the SHA loop)
            t0 = time.perf_counter(); [S.dif_eval(b, x, keys[b]) for b in range(2)]; t_evp = (time.perf_counter() - t0) / n
            S.use_pool(None)
        shapes = [(12544, 147, 64)] + [(3136, 576, 64)] * 4 + [(784, 576, 128), (784, 64, 128)] + [(784, 1152, 128)] * 3 \
            + [(196, 1152, 256), (196, 128, 256)] + [(196, 2304, 256)] * 3 + [(49, 2304, 512), (49, 256, 512)] \
            + [(49, 4608, 512)] * 3 + [(1, 512, 3)]
        t_mm = 0.0
        per = {}
        for sh in shapes:
            if sh not in per:
                A = torch.randint(-2 ** 62, 2 ** 62, (sh[0], sh[1])); B = torch.randint(-2 ** 62, 2 ** 62, (sh[1], sh[2]))
                t0 = time.perf_counter(); torch.matmul(A, B); per[sh] = time.perf_counter() - t0
            t_mm += per[sh] * 3 * 2
        return dict(ncores=ncores, n=n, t_kg1=t_kg1, t_kg=t_kg, t_ev1=t_ev1, t_evp=t_evp, t_mm=t_mm)


    cpu_t = cpu_sample_timings() if (a.cpu_sample and not a.only_fss_roofline) else None   # before the first GPU call
    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    sd = rs.init_state_dict(rs.resnet18_spec(3, 3, a.size, a.pooling), "group" if a.norm == "group" else "batch")
    if a.norm == "folded":
        sd = fold_batch_norm(sd)
    form = ProtocolForm(pooling=a.pooling, reveal=a.reveal, fss_bits=a.fss_bits, wide_norm=a.wide_norm,
                        faithful_trunc=a.faithful_trunc)
    # (the report of the default keeps its keys: an option is named only where it differs from the default -- "pooling" for
    # avg only, "norm" for group and folded only -- and in the order the report has always had)
    named = {**non_default(form), **({} if a.norm == "batch" else {"norm": a.norm})}
    form_report = {k: named[k] for k in ("pooling", "norm", "wide_norm", "faithful_trunc", "reveal", "fss_bits") if k in named}
    g = torch.Generator().manual_seed(1)
    img = torch.randn(1, 3, a.size, a.size, generator=g).to(dev)

    def run(dealer, share_model=True):
        ctx = SecureContext(dealer, 10, a.pf)
        model = SecureResNet18(ctx, sd, input_size=a.size, form=form)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = model(img)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out, ctx

    PMC_FILE = "r06_secure_valu_pmc.json"

    def valu_pmc():
        """Counted vector instructions of the DIF kernels from the committed rocprofv3 --pmc pass (tools/pmc_secure.sh)."""
        pth = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", PMC_FILE)
        return json.load(open(pth)) if os.path.exists(pth) else None

    def fss_roofline():
        """The dominant secure kernel alone: fss.le of 2^20 comparisons for BOTH parties (primia_dif_eval_local: mask, open
        and 2 x 32 SHA-512 compressions per comparison; 1,204 bytes of key per comparison, read by both parties' threads).
        Bound: vector-instruction ISSUE.  64-bit integer code runs on 32-bit vector instructions (v_lshl_add_u64 adds,
        v_alignbit rotates, v_bitop3 Ch / Maj / xor3).  `peak` is the architectural issue rate: a SIMD-32 issues a wave64
        vector instruction over 2 cycles, 256 CUs x 4 SIMDs x 2.4 GHz / 2 = 1,228.8 G wave-instructions per second
        (MI355X_MICROARCH.md, "Wave scheduling").  `mix_ceiling` is what the instructions THIS kernel is made of reach in
        a register-only loop on the same chip (tools/micro/valu_rate.hip, profiles/r04_valu_issue_rate.txt): the
        three-operand forms issue every ~4 cycles (518-584 G/s), two-operand adds / xors at 828-868 G/s.
        `achieved` = the kernel's COUNTED instructions per launch (SQ_INSTS_VALU of the committed PMC pass over this very
        command, profiles/r06_secure_valu_pmc.json) / the launch time measured here."""
        n = 1 << 20
        d = Dealer(dev, seed=7)
        keys = d.dif_keys(n)
        x2 = [d.rand64(n), d.rand64(n)]
        out = [torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)]
        from primia_amd._lib import call
        k0, k1 = keys
        args = (None, None, 1, 0, x2[0], x2[1], 1, 0, 1, k0["alpha"], k1["alpha"], k0["s0"], k1["s0"], k0["bits"],
                k0["cw_sigma"], k0["cw_s"], k0["cw_leaf"], out[0], out[1], n)
        # (the per-party kernel of the three-role deployment, so that the PMC pass over this command counts it too)
        masked = torch.randint(0, 2 ** 31, (n,), dtype=torch.int32).to(dev)      # (host-drawn: no torch kernel in the trace)
        call("primia_dif_eval", 0, masked, k0["s0"], k0["bits"], k0["cw_sigma"], k0["cw_s"], k0["cw_leaf"], out[0], n)
        for _ in range(2):
            call("primia_dif_eval_local", *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        reps = 5
        for _ in range(reps):
            call("primia_dif_eval_local", *args)
        e1.record(); torch.cuda.synchronize()
        t = e0.elapsed_time(e1) / reps * 1e-3
        peak = 256 * 4 * 2.4e9 / 2
        mix_ceiling = 584.1e9      # v_bitop3_b32, the fastest of the kernel's three-operand instructions, alone
        pmc = valu_pmc()
        insts = (pmc or {}).get("dif_eval_local_kernel", {}).get("SQ_INSTS_VALU")
        rec = {"bound": "valu-issue", "kernel": "dif_eval_local_kernel", "peak": round(peak / 1e9, 1),
               "unit": "G wave64 vector instructions/s", "launch_us": round(t * 1e6, 1), "comparisons": n,
               "sha512_compressions_per_s_G": round(2 * n * 32 / t / 1e9, 3),
               "key_read_GBps": round(n * 1204 / t / 1e9, 1), "key_read_frac_of_hbm": round(n * 1204 / t / 8e12, 4)}
        if insts:
            rec.update(achieved=round(insts / t / 1e9, 1), frac=round(insts / t / peak, 4), insts_per_launch=int(insts),
                       insts_source="profiles/" + PMC_FILE,
                       mix_ceiling=round(mix_ceiling / 1e9, 1), frac_of_mix_ceiling=round(insts / t / mix_ceiling, 4),
                       note="three-operand integer instructions (80 % of this kernel: v_alignbit_b32, v_lshl_add_u64, "
                            "v_bitop3_b32) issue every ~4 cycles, not 2: alone in a register-only loop they reach 518-584 G/s "
                            "(profiles/r04_valu_issue_rate.txt).  frac_of_mix_ceiling > 1 because the other 20 % are "
                            "two-operand instructions at 828-868 G/s: the kernel sits on its issue limit, only fewer "
                            "instructions would make it faster")
        else:
            rec.update(achieved=None, frac=None, insts_source="no PMC record for this kernel: run tools/pmc_secure.sh")
        rec["valu_pmc"] = pmc
        return rec


    if a.batch:
        from primia_amd.secure import GraphedSecureInference, architecture_of, largest_batch_that_fits

        B, reps = a.batch, max(a.images, 3)
        imgs = torch.randn(B, 3, a.size, a.size, generator=g).to(dev)
        free = torch.cuda.mem_get_info(dev)[0]
        gi = GraphedSecureInference(sd, dev, input_size=a.size, precision_fractional=a.pf, seed=999, batch=B, form=form)
        # (an evaluation's passes carry the data owner's labels: seeded, one per image)
        lab_kw = {"labels": torch.randint(0, 3, (B,), generator=g)} if a.reveal in ("confusion", "metrics") else {}
        gi(imgs, refill=False, **lab_kw); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            gi(imgs, refill=False, **lab_kw)
        torch.cuda.synchronize()
        online = (time.perf_counter() - t0) / reps * 1e3
        gi(imgs, **lab_kw); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            gi(imgs, **lab_kw)          # the dealer's refill graph, then the online graph, on one stream
        torch.cuda.synchronize()
        both = (time.perf_counter() - t0) / reps * 1e3
        tail_kw = {}
        if a.reveal == "metrics":
            # the tail on its own: an evaluation of --eval_images images (replayed on the primitives the buffers hold: only the
            # rows matter here), finish() once on the tail's live dealer, which records its primitives, then once more on them
            gi.begin()
            passes = (a.eval_images + B - 1) // B
            for _ in range(passes):
                gi(imgs, refill=False, **lab_kw)
            torch.cuda.synchronize()
            tail_ctx = gi._tail_ctx
            tail_ctx.dealer.tape = []
            evals0 = tail_ctx.stats["dif_evals"]
            t0 = time.perf_counter(); gi.finish(); torch.cuda.synchronize()
            with_dealer = (time.perf_counter() - t0) * 1e3
            rows, classes = passes * B, int(sd["fc.weight"].shape[0])
            comparisons = tail_ctx.stats["dif_evals"] - evals0
            pre = SecureContext(PreloadedDealer(tail_ctx.dealer.tape, dev, fss_bits=form.fss_bits), 10, a.pf)
            for u in gi._model.U:
                u.zero_()
            t0 = time.perf_counter(); gi._model.finish(ctx=pre); torch.cuda.synchronize()
            tail_online = (time.perf_counter() - t0) * 1e3
            # (of which: gathering the rows the passes left -- one copy launch per pass, share and party)
            t0 = time.perf_counter(); gi._model.held_rows(); torch.cuda.synchronize()
            gather = (time.perf_counter() - t0) * 1e3
            tail_kw = {"eval_rows": rows, "tail_comparisons": comparisons, "tail_rank_comparisons_64bit": classes * rows * rows,
                       "tail_online_ms": round(tail_online, 1), "tail_gather_rows_ms": round(gather, 1), "tail_with_dealer_ms": round(with_dealer, 1),
                       "tail_online_in_images": round(tail_online / (online / B), 2),
                       "tail_expected_in_images": round(2 * classes * rows * rows / 3311616, 2)}
        print(json.dumps({"metric": "encrypted_inference_batch", **form_report, "batch": B, "size": a.size, "precision_fractional": a.pf,
                          "online_ms_per_image": round(online / B, 2), "with_refill_ms_per_image": round(both / B, 2),
                          "online_ms_per_pass": round(online, 2), "with_refill_ms_per_pass": round(both, 2),
                          "static_primitive_bytes": gi.static_bytes, "arena_mb": round(gi._arena.numel() * 8 / 1e6, 1),
                          "device_free_bytes_before": free,
                          "largest_batch_that_fits": largest_batch_that_fits(architecture_of(sd), a.size, free, form=form),
                          "dif_evals": gi.stats["dif_evals"], **({"dpf_evals": gi.stats["dpf_evals"]} if "dpf_evals" in gi.stats else {}),
                          "beaver_matmul": gi.stats["beaver_matmul"],
                          "beaver_mul": gi.stats["beaver_mul"], **tail_kw}))
        return

    if a.only_fss_roofline:
        d = Dealer(dev, seed=3)
        for _ in range(3):
            d.dif_keys(1 << 20)            # dif_keygen_kernel
        print(json.dumps({"roofline": fss_roofline()}))
        return

    # warm-up (JIT-free, but first launches / allocator)
    run(Dealer(dev, seed=0, fss_bits=form.fss_bits))
    res = []
    for i in range(a.images):
        d = Dealer(dev, seed=100 + i, fss_bits=form.fss_bits); d.tape = []
        t_total, out_a, ctx = run(d)
        t_online, out_b, _ = run(PreloadedDealer(d.tape, dev, fss_bits=form.fss_bits))
        assert torch.equal(out_a.cpu(), out_b.cpu()), "replayed run must be bit-identical"
        res.append((t_total, t_online))
        del d
    tt = sum(r[0] for r in res) / len(res); to = sum(r[1] for r in res) / len(res)

    # The online phase as ONE hipGraph (6,500 small launches per image): primitives sit in static buffers (a
    # deployment refills them from the dealer between images), the replay is checked bit for bit against the
    # eager run with the same primitives.
    graph_ms = refill_ms = pipe_ms = refill_nodes = arena_mb = None
    if not a.no_graph:
        try:
            from primia_amd.secure import GraphedSecureInference

            gi = GraphedSecureInference(sd, dev, input_size=a.size, precision_fractional=a.pf, seed=999, form=form)
            ctx_e = SecureContext(PreloadedDealer(gi.tape, dev, fss_bits=form.fss_bits), 10, a.pf)
            out_ref = SecureResNet18(ctx_e, sd, input_size=a.size, form=form)(img)
            assert torch.equal(gi(img, refill=False).cpu(), out_ref.cpu()), "graph replay must be bit-identical"
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(3):
                gi(img, refill=False)
            torch.cuda.synchronize()
            graph_ms = (time.perf_counter() - t0) / 3 * 1e3
            # the dealer's refill: ONE graph launch since round 6 (an eager loop of ~3,000 launches before)
            gi.refill(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                gi.refill()
            torch.cuda.synchronize()
            refill_ms = (time.perf_counter() - t0) / 3 * 1e3
            refill_nodes = 2 + sum(1 if op[0] == "triple" and op[1] == "mul" else (3 if op[0] == "triple" else 2) for op in gi._ops)
            arena_mb = gi._arena.numel() * 8 / 1e6
            del gi
            # a STREAM of images with the dealer hidden behind the online phase (two graph slots, the dealer refills one
            # on its own stream while the other replays): wall time per image, every image on fresh primitives
            from primia_amd.secure import PipelinedSecureInference

            pi = PipelinedSecureInference(sd, dev, input_size=a.size, precision_fractional=a.pf, seed=555, form=form)
            for _ in range(2):
                pi(img)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            n_stream = 8
            for _ in range(n_stream):
                pi(img)
            torch.cuda.synchronize()
            pipe_ms = (time.perf_counter() - t0) / n_stream * 1e3
        except Exception as e:  # capture is an optimisation of the measurement, not of the result
            print("hipGraph capture of the online phase failed:", repr(e)[:300], file=sys.stderr)

    def cpu_sample_report(t, n_cmp):
        online = t["t_evp"] * n_cmp + t["t_mm"]
        return {"value": round(online * 1e3, 0), "unit": "ms/image (online: FSS eval, both parties, + Beaver matmuls)",
                "cores": t["ncores"], "kind": "port",
                "fss_eval_ms": round(t["t_evp"] * n_cmp * 1e3, 0), "fss_eval_one_core_ms": round(t["t_ev1"] * n_cmp * 1e3, 0),
                "beaver_matmul_ms": round(t["t_mm"] * 1e3, 0), "dealer_keygen_ms": round(t["t_kg"] * n_cmp * 1e3, 0),
                "dealer_keygen_small_batch_ms": round(t["t_kg1"] * n_cmp * 1e3, 0),
                "sample": f"oracle DIF eval of {t['n']} comparisons x 2 parties in {t['ncores']} spawned processes (the "
                          f"reference's fan-out, mpc/fss.py:43-44,214-236), timed before this process touched the GPU; keygen of "
                          f"the same {t['n']} on one core; extrapolated to the {n_cmp} comparisons of one image; torch-CPU int64 "
                          "matmul of all 21 Beaver shapes x3 products x2 parties; excludes the reference's Python im2col, "
                          "Newton BN and RPC overhead: a FLOOR of the reference's time, not a measurement of it"}


    extra = {"cpu_baseline": cpu_sample_report(cpu_t, ctx.stats["dif_evals"])} if cpu_t else {}
    extra["roofline"] = fss_roofline()
    print(json.dumps({"metric": "encrypted_inference_ms_per_image", **form_report, "online_ms": round(to * 1e3, 1),
                      "online_graph_ms": None if graph_ms is None else round(graph_ms, 1),
                      "dealer_refill_ms": None if refill_ms is None else round(refill_ms, 1),
                      "dealer_refill_launches": refill_nodes, "dealer_keystream_mb_per_image": None if arena_mb is None else round(arena_mb, 1),
                      "with_dealer_ms": round(tt * 1e3, 1), "dealer_ms": round((tt - to) * 1e3, 1),
                      "with_dealer_pipelined_ms": None if pipe_ms is None else round(pipe_ms, 1),
                      "precision_fractional": a.pf, "size": a.size, "dif_evals": ctx.stats["dif_evals"],
                      "beaver_matmul": ctx.stats["beaver_matmul"], "beaver_mul": ctx.stats["beaver_mul"],
                      "topology": "party0 + party1 + dealer on one MI355X (LocalOpener)", **extra}))


if __name__ == "__main__":
    main()
