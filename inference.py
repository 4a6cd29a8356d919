#!/usr/bin/env python3
"""PriMIA-compatible inference CLI (inference.py:47-76, 279-323 of the reference).

    python inference.py --model_weights model_weights/final_*.pt [--data_dir DIR|synthetic]
                        [--encrypted_inference] [--cuda] [--websockets_config CSV] [--http_protocol]

Plain inference runs the HIP engine in eval mode.  `--encrypted_inference` shares the model and
each image between model_owner and data_owner (fixed precision 10^16, protocol "fss", a dealer as
crypto provider) and runs the secret-shared forward of primia_amd.secure, image by image like the
reference's loop, or `--batch_size N` images per protocol pass; the checkpoint's `pooling_type` (max | avg) decides the stem pool
of the plain and of every encrypted form, and a checkpoint without BatchNorm running statistics (train.py with
differentially_private = yes: GroupNorm(32, C) at every norm site) is served as the GroupNorm network, plain and encrypted.
The encrypted GroupNorm takes its inverse square root from the reference's Newton iteration, which is accurate to under 1 %
for group variances in about [0.05, 16] (1.6 % off at 0.01, 15 % at 0.001, orders of magnitude above 21); `--wide_norm` serves
a GroupNorm checkpoint for any group variance below 30,000 with the undamped iteration at a scale of 10^-6 (--precision_fractional
3 to 6; a form defined here, not by the reference).  The encrypted BatchNorm runs the same
iteration on shares of running_var, as the reference does, and is accurate on the same window only (the wrong sign from a
variance of 22); `--fold_norm` has the model owner fold every BatchNorm into scale = gamma / sqrt(running_var + 1e-5) and
shift = beta - running_mean * scale before sharing, so that each norm site is one private multiply-add and the encrypted pass
follows the plaintext model for any running statistics -- a form defined here, not by the reference; the plain path always
evaluates the checkpoint as it is.  `--reveal class` ends every encrypted pass with
a secret-shared argmax and opens the predicted class alone: the logits, the model owner's asset, are never reconstructed.  Output: the reference's JSON on stdout, {"Inference Results": {index: class}}.

`--evaluate` scores the model on a labelled set instead (`--data_dir` a class-folder tree <dir>/<class>/<image>, or `synthetic`
for seeded images and labels), plain or encrypted, and prints the reference's validation table and one JSON line
{"Evaluation": {"n": ..., "confusion_matrix": [[...]], "mcc": ...}}.  With `--reveal confusion` an encrypted evaluation opens
the confusion matrix and nothing else: no logit, no predicted class and no label leaves its owner.  `--reveal metrics` opens,
with the matrix, the pair counts of the reference's one-vs-one ROC AUC -- formed on shares after the last pass -- and prints the
table with the AUC ({"Evaluation": {..., "roc_auc": ...}}); still nothing per image.
"""
import argparse
import json
import os
import sys
from datetime import datetime
from warnings import warn

import torch

from primia_amd.engine import ResNet18Engine
from primia_amd.secure import (Dealer, ProtocolForm, SecureContext, SecureResNet18, check_faithful_trunc, check_wide_norm,
                               expected_wraps, fold_batch_norm, norm_of)
from primia_amd.torchlib_compat import Arguments  # noqa: F401  (checkpoints pickle an Arguments instance)


def synthetic_labels(n, classes, seed=1):
    """The seeded labels that go with the seeded noise images of `--evaluate --data_dir synthetic`: int64 [n]."""
    return torch.randint(0, classes, (n,), generator=torch.Generator().manual_seed(seed))


def labelled_files(data_dir, n, classes):
    """The class-folder tree <dir>/<class>/<image> of an evaluation, listed like the validation folder (imagefolder.scan):
    (files, int64 labels, class names).  `n` = None takes every image, else n of them evenly spaced over the listing, so
    that every class keeps its share."""
    from primia_amd import imagefolder

    if not os.path.isdir(data_dir):
        raise SystemExit("data_dir {!r} does not exist (pass 'synthetic' for seeded images and labels)".format(data_dir))
    names, samples = imagefolder.scan(data_dir)
    if not samples:
        raise SystemExit("no images under {!r}: --evaluate reads <dir>/<class>/<image>".format(data_dir))
    if len(names) > classes:
        raise SystemExit("{!r} holds {} class folders, the checkpoint has {} classes".format(data_dir, len(names), classes))
    if n is not None and n < len(samples):
        samples = [samples[i * len(samples) // n] for i in range(n)]
    return [f for f, _ in samples], torch.tensor([c for _, c in samples], dtype=torch.int64), names


def confusion_of(labels, predictions, classes):
    """int64 [classes, classes] counts of (label, prediction) pairs."""
    m = torch.zeros(classes, classes, dtype=torch.int64)
    for t, p in zip(labels.tolist(), predictions):
        m[int(t), int(p)] += 1
    return m


def roc_auc_of(labels, logits):
    """torchlib/utils.py:1418-1431: one-vs-one ROC AUC on the min-shifted, row-normalised logits; 0 where it is undefined."""
    from sklearn import metrics as mt

    scores = logits.double().numpy().copy()
    scores -= scores.min(axis=1)[:, None]
    scores = scores / scores.sum(axis=1)[:, None]
    auc = float("nan")
    try:
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if scores.shape[1] == 2:
                auc = float(mt.roc_auc_score(labels.numpy(), scores[:, 1]))
            else:
                auc = float(mt.roc_auc_score(labels.numpy(), scores, multi_class="ovo", labels=list(range(scores.shape[1]))))
    except ValueError:
        pass
    if auc != auc:      # undefined (one class among the labels, a row of equal logits): scikit-learn raises or answers nan
        print("ROC AUC score could not be calculated and was set to zero.", file=sys.stderr)
        return 0.0
    return auc


def load_images(data_dir, n, size, channels, device, mean, std, seed=0, clahe=False, files=None):
    """The reference's inference transform (inference.py:176-196: a.Resize(R, R) -> a.CenterCrop(R, R) -> a.ToFloat ->
    a.Normalize with the checkpoint's mean / std) for the first `n` images of `data_dir`, on the GPU through
    primia_image_prepare; RGB or single channel as the checkpoint's stem says (CombinedLoader.change_channels).
    `synthetic` (or no folder given) -> seeded noise; a folder that does not exist is an error.  `files`: these files
    instead of the folder's listing."""
    if files is None and data_dir in (None, "synthetic"):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(n, channels, size, size, generator=g).to(device)
    if files is None and not os.path.isdir(data_dir):
        raise SystemExit("data_dir {!r} does not exist (pass 'synthetic' for seeded noise)".format(data_dir))
    import numpy as np

    from primia_amd import imagefolder
    from primia_amd._lib import call

    if files is None:
        files = sorted(os.path.join(dp, f) for dp, _, fs in os.walk(data_dir) for f in fs
                       if f.lower().endswith(imagefolder.EXTENSIONS) and not f.startswith("._"))[:n]
    if not files:
        raise SystemExit("no images under {!r}".format(data_dir))
    out = torch.empty(len(files), channels, size, size, dtype=torch.float32, device=device)
    m = mean.to(device).float().reshape(-1).contiguous()
    s_ = std.to(device).float().reshape(-1).contiguous()
    if m.numel() != channels:          # a one-element statistic applies to every channel
        m, s_ = m[:1].repeat(channels), s_[:1].repeat(channels)
    if clahe:        # inference.py:182-183: a.CLAHE(always_apply=True, clip_limit=(1, 1)) between the crop and ToFloat
        from primia_amd._lib import query

        wsb = query("primia_clahe_workspace_bytes", size, size, channels)
        ws = torch.empty(wsb, dtype=torch.uint8, device=device)
        u8 = torch.empty(size, size, channels, dtype=torch.uint8, device=device)
    for i, fn in enumerate(files):
        img = torch.from_numpy(np.ascontiguousarray(imagefolder.decode(fn, channels))).to(device)
        if clahe:
            call("primia_image_resize_crop_u8", img, img.shape[0], img.shape[1], channels, size, 0, 0, size, 0, u8)
            call("primia_clahe_u8", u8, size, size, channels, 1.0, ws, wsb, u8)
            call("primia_image_finish", u8, size, channels, m, s_, out[i])
        else:
            call("primia_image_prepare", img, img.shape[0], img.shape[1], channels, size, 0, 0, size, 0, m, s_, out[i])
    return out


def faithful_trunc_choice(requested, encrypted, keys, fold):
    """What --faithful_trunc comes to: True when the encrypted pass is to truncate its products faithfully.  Without
    --encrypted_inference it warns and does nothing; on a network that is not folded the run ends with the reason."""
    if not requested:
        return False
    if not encrypted:
        warn("--faithful_trunc has no effect: without --encrypted_inference nothing is shared and nothing is truncated")
        return False
    norm = norm_of(keys)
    try:
        check_faithful_trunc("folded" if fold and norm == "batch" else norm)
    except ValueError as e:
        raise SystemExit(f"--faithful_trunc: {e}" + (" -- pass --fold_norm" if norm == "batch" else ""))
    return True


def warn_of_large_products(sd, images, precision_fractional, pooling):
    """--faithful_trunc holds while every product stays below 2^62 at scale^2: the plaintext forward of the data says how
    close this run comes (in a deployment each owner can bound its own factor; here one process holds both)."""
    e = expected_wraps(sd, images, precision_fractional, pooling=pooling)
    if e["max_ratio"] >= 0.5:
        warn(f"--faithful_trunc: the largest product of this run is {e['max_ratio']:.2f} x 2^62 at --precision_fractional "
             f"{precision_fractional}; at 1 the truncation's precondition |z| < 2^62 fails and the result is undefined -- lower "
             f"--precision_fractional or rescale the inputs")


def wide_norm_choice(requested, encrypted, keys, precision_fractional):
    """What --wide_norm comes to: True when the encrypted pass is to use the wide-range GroupNorm.  Without
    --encrypted_inference it warns and does nothing; on a BatchNorm checkpoint, or at a precision the form is not defined
    for, the run ends."""
    if not requested:
        return False
    if not encrypted:
        warn("--wide_norm has no effect: without --encrypted_inference nothing is shared, the plain engine computes "
             "GroupNorm in floating point for any group variance")
        return False
    if norm_of(keys) != "group":
        raise SystemExit("--wide_norm is a form of the secret-shared GroupNorm; this is a BatchNorm checkpoint, whose running "
                         "statistics are the model owner's plaintext: pass --fold_norm, which serves it for any running variance")
    try:
        check_wide_norm(10, precision_fractional)
    except ValueError as e:
        raise SystemExit(f"--wide_norm: {e} -- pass --precision_fractional 3 to 6")
    return True


if __name__ == "__main__":
    start_time = datetime.now()
    parser = argparse.ArgumentParser()
    parser.add_argument("--data_dir", default=None, help="data to classify")
    parser.add_argument("--model_weights", type=str, required=True, help="model weights to use")
    parser.add_argument("--encrypted_inference", action="store_true",
                        help="Perform encrypted inference (a GroupNorm checkpoint, one without running statistics, is "
                             "recognised by itself; its group variances should lie in about [0.05, 16], the range in which "
                             "the protocol's Newton inverse square root is accurate to under 1 %%)")
    parser.add_argument("--websockets_config", default=None, help="accepted for compatibility (in-process parties)")
    parser.add_argument("--cuda", action="store_true", help="Use GPU acceleration (always on here).")
    parser.add_argument("--http_protocol", action="store_true", help="accepted for compatibility")
    parser.add_argument("--num_images", type=int, default=None,
                        help="how many images (default 4; with --evaluate on a folder: all of them)")
    parser.add_argument("--evaluate", action="store_true",
                        help="score the model on a labelled set: --data_dir is a class-folder tree <dir>/<class>/<image> "
                             "(or `synthetic`: seeded images and labels); prints the validation table and one JSON line "
                             '{"Evaluation": {"n", "confusion_matrix", "mcc"}}.  Plain or encrypted, with every --reveal')
    parser.add_argument("--batch_size", type=int, default=1,
                        help="encrypted inference: images per protocol pass (default 1, the reference's loop); the last "
                             "pass of --hip_graph / --three_role is padded with all-zero images whose rows are dropped")
    parser.add_argument("--precision_fractional", type=int, default=16,
                        help="encrypted inference: fractional decimal digits of the fixed-point encoding (default 16, the "
                             "reference's literal, at which products wrap in the 2^64 ring; 3 keeps logits meaningful).  "
                             "More digits make the encoded activations larger and the 32-bit comparisons wrong more often: "
                             "see --fss_bits")
    parser.add_argument("--fss_bits", type=int, default=32,
                        help="encrypted inference: the width n of the ReLU / max-pool / argmax comparisons, 32 (default, the "
                             "reference's) to 64.  A comparison of two encoded values d apart is wrong with probability "
                             "|d| / 2^n over the provider's mask, and always beyond 2^(n-1): at 32 bits and 6 fractional "
                             "digits that is every activation above 2147.  Key bytes (60 + 37 n per comparison) and the "
                             "comparison kernels' time grow linearly with n")
    parser.add_argument("--hip_graph", action="store_true",
                        help="encrypted inference: capture the online phase once as a hipGraph and replay it per image "
                             "(the dealer refills the primitive buffers between images)")
    parser.add_argument("--three_role", action="store_true",
                        help="encrypted inference with model_owner, data_owner and crypto_provider as three ranks "
                             "(launch with `python -m torch.distributed.run --nproc-per-node 3 inference.py ...`): "
                             "one GPU each over RCCL when three are visible, else all on GPU 0 over gloo")
    parser.add_argument("--reveal", choices=("logits", "class", "confusion", "metrics"), default="logits",
                        help="encrypted inference: what a pass opens.  logits (default, the reference): the full score "
                             "vector, whose argmax is taken in the clear; class: the predicted class alone, through a "
                             "secret-shared argmax of classes - 1 comparison rounds (the logits are never reconstructed, so "
                             "PRIMIA_DUMP_LOGITS is refused); confusion (with --evaluate only): nothing per image -- every "
                             "pass adds into a secret-shared confusion matrix through classes equality tests per image, and "
                             "the matrix alone is opened after the last pass (no ROC AUC); metrics (with --evaluate only): the "
                             "confusion passes, then classes * n^2 64-bit comparisons of cross-multiplied scores on shares: "
                             "the matrix and 2 * classes * (classes - 1) pair counts are opened, from which the reference's "
                             "one-vs-one ROC AUC follows -- nothing per image")
    parser.add_argument("--fold_norm", action="store_true",
                        help="encrypted inference on a BatchNorm checkpoint: the model owner folds every BatchNorm into one "
                             "per-channel map before sharing -- scale = gamma / sqrt(running_var + 1e-5) and shift = beta - "
                             "running_mean * scale, computed in plaintext and shared in place of the statistics -- so a norm "
                             "site is one private multiply-add and the pass follows the plaintext model for any running "
                             "statistics.  The reference's form (the default) runs its Newton iteration on shares of "
                             "running_var and is accurate only for running variances in about [0.05, 16] (15 %% off at "
                             "0.001, the wrong sign from 22); the folded form is defined here, not by the reference.  Per "
                             "pass it drops the 237 Newton triples, their 80 masks and one of the two products of each of "
                             "the 20 norm sites.  Refused for a GroupNorm checkpoint, whose statistics depend on the image")
    parser.add_argument("--faithful_trunc", action="store_true",
                        help="encrypted inference with --fold_norm: truncate the products of conv2d, the folded norm and fc "
                             "with a form no mask can make wrap.  The reference has each party divide its own share, which "
                             "is off by 2^64 / scale whenever the signed shares wrap -- with probability |z| / 2^64 per "
                             "element: never in practice at --precision_fractional 3, about once in a few 224 x 224 images "
                             "at 6, where it puts 1.8e7 into an activation.  The faithful form costs one more element-wise "
                             "Beaver product on carry bits per site and is within two units of the last digit for every "
                             "mask while |z| < 2^62 (DESIGN.md §4; defined here, not by the reference).  With every "
                             "--reveal, --hip_graph, --batch_size, --evaluate and --three_role.  Refused without "
                             "--fold_norm and for a GroupNorm checkpoint: their Newton iterations truncate per share")
    parser.add_argument("--wide_norm", action="store_true",
                        help="encrypted inference on a GroupNorm checkpoint: the wide-range form of the secret-shared "
                             "GroupNorm -- the variance and its inverse square root carried at a scale of 10^-6 whatever "
                             "--precision_fractional, and the inverse square root from the undamped Newton iteration, which "
                             "is one for every group variance below 30,000 (the default form: about [0.05, 16], and off by "
                             "orders of magnitude above).  Defined here, not by the reference (DESIGN.md §4); 128 dealer "
                             "requests per norm site against 321; needs --precision_fractional 3 to 6.  With every "
                             "--reveal, --hip_graph, --batch_size, --evaluate and --three_role.  Refused for a BatchNorm "
                             "checkpoint: --fold_norm serves that one for any running variance")
    parser.add_argument("--debug_dealer_seed", type=int, default=None,
                        help="DEBUG ONLY: derive the crypto provider's key from this number (reproducible, hence "
                             "NOT private); by default the key comes from the OS entropy pool and never leaves the "
                             "provider")
    cmd_args = parser.parse_args()
    if cmd_args.debug_dealer_seed is not None:
        print("WARNING: --debug_dealer_seed makes every mask, triple and FSS key predictable: no confidentiality",
              file=sys.stderr)
    reveal = cmd_args.reveal
    fss_bits = cmd_args.fss_bits
    if not 32 <= fss_bits <= 64:
        raise SystemExit(f"--fss_bits must be in [32, 64], got {fss_bits}")
    evaluate = cmd_args.evaluate
    if reveal in ("confusion", "metrics") and not evaluate:
        raise SystemExit(f"--reveal {reveal} opens the confusion matrix of a labelled set and nothing per image: an inference "
                         "has no labels to count against and would print nothing -- pass --evaluate (and a class-folder "
                         "--data_dir or `synthetic`)")
    if reveal in ("confusion", "metrics") and not cmd_args.encrypted_inference:
        raise SystemExit(f"--reveal says what an ENCRYPTED run opens: --reveal {reveal} needs --encrypted_inference")
    if reveal != "logits" and os.environ.get("PRIMIA_DUMP_LOGITS"):
        raise SystemExit(f"--reveal {reveal}: the logits are never opened, there is nothing for PRIMIA_DUMP_LOGITS to write")
    if not torch.cuda.is_available():
        raise SystemExit("primia_amd runs inference on the GPU only (HIP kernels); no GPU visible")
    device = torch.device("cuda:0")
    state = torch.load(cmd_args.model_weights, map_location="cpu", weights_only=False)
    args = state["args"]
    if not isinstance(args, Arguments):
        args = Arguments.from_namespace(args)
    args.from_previous_checkpoint(cmd_args)
    size = getattr(args, "inference_resolution", args.train_resolution)
    sd = state["model_state_dict"]
    channels = int(sd["conv1.weight"].shape[1])       # 3 for pretrained = yes, else 1 (train.py:262)
    # inference.py:163-174: the checkpoint's statistics, else 0.5 / 0.2
    mean, std = state.get("val_mean_std", (torch.full((channels,), 0.5), torch.full((channels,), 0.2)))
    classes = int(sd["fc.weight"].shape[0])
    labels = class_names = None
    if evaluate and cmd_args.data_dir not in (None, "synthetic"):
        files, labels, class_names = labelled_files(cmd_args.data_dir, cmd_args.num_images, classes)
        images = load_images(cmd_args.data_dir, len(files), size, channels, device, mean, std,
                             clahe=bool(getattr(args, "clahe", False)), files=files)
    else:
        images = load_images(cmd_args.data_dir, 4 if cmd_args.num_images is None else cmd_args.num_images, size, channels,
                             device, mean, std, clahe=bool(getattr(args, "clahe", False)))
        if evaluate:
            labels = synthetic_labels(images.shape[0], classes)
    matrix = None      # --reveal confusion: the opened confusion matrix, all such a run learns
    rank_counts = None # --reveal metrics: the opened pair counts of the ROC AUC, next to the matrix
    logits = []        # the logits a run opened, pass by pass (none with --reveal class / confusion)
    total_pred = []
    bs = cmd_args.batch_size
    if bs < 1:
        raise SystemExit("--batch_size must be at least 1")
    pooling = getattr(args, "pooling_type", "max")
    fold = False
    if cmd_args.fold_norm and not args.encrypted_inference:
        warn("--fold_norm has no effect: without --encrypted_inference nothing is shared, the plain engine evaluates the "
             "checkpoint's BatchNorm as it is")
    elif cmd_args.fold_norm:
        if norm_of(sd.keys()) != "batch":
            raise SystemExit("--fold_norm folds BatchNorm running statistics, which are the model owner's plaintext; this is a "
                             "GroupNorm checkpoint (no running statistics), whose statistics depend on the image and cannot "
                             "be folded before sharing")
        fold = True
    wide = wide_norm_choice(cmd_args.wide_norm, args.encrypted_inference, sd.keys(), cmd_args.precision_fractional)
    faithful = faithful_trunc_choice(cmd_args.faithful_trunc, args.encrypted_inference, sd.keys(), fold)
    if faithful:
        warn_of_large_products(sd, images, cmd_args.precision_fractional, pooling)
    if args.encrypted_inference:
        # inference.py:279-286: fix_precision(precision_fractional=16, dtype="long").share(..., protocol="fss")
        form = ProtocolForm(pooling=pooling, reveal=reveal, fss_bits=fss_bits, wide_norm=wide, faithful_trunc=faithful)
        if cmd_args.three_role:
            import torch.distributed as dist

            from primia_amd.secure import PartyLink, architecture_of, folded_architecture, run_three_role

            multi = torch.cuda.device_count() >= 3
            rank = int(os.environ["RANK"])
            device = torch.device("cuda", rank if multi else 0)
            torch.cuda.set_device(device)
            dist.init_process_group(os.environ.get("PRIMIA_PARTY_BACKEND", "nccl" if multi else "gloo"))
            link = PartyLink(device)
            # one checkpoint file serves all three ranks of a single-node launch; each role is handed only what
            # it owns: the weights (party 0), the images (party 1), the architecture (everyone).  --fold_norm: the model
            # owner folds its weights, the other two ranks fold the architecture
            arch = architecture_of(sd)
            owned = None
            if link.role == 0:
                owned = fold_batch_norm(sd) if fold else sd
            result = run_three_role(link, folded_architecture(arch) if fold else arch, size, images.shape[0],
                                    state_dict=owned,
                                    images=images.to(device) if link.role == 1 else None,   # (this rank's GPU)
                                    seed=cmd_args.debug_dealer_seed, batch=bs,
                                    precision_fractional=cmd_args.precision_fractional, form=form,
                                    labels=labels if link.role == 1 and reveal in ("confusion", "metrics") else None)
            dist.barrier()
            dist.destroy_process_group()
            if link.role != 1:
                sys.exit(0)
            if reveal == "metrics":        # both parties hold the matrix and the counts
                matrix, rank_counts = result[0].cpu(), result[1].cpu()
            elif reveal == "confusion":    # both parties hold the matrix; the data owner's rank reports it
                matrix = result.cpu()
            elif reveal == "class":        # party 1 holds the class indices themselves
                total_pred = [int(c) for o in result for c in o.tolist()]
            else:
                logits = result
                total_pred = [int(c) for o in logits for c in o.argmax(dim=1).tolist()]
        else:
            # --fold_norm: what the model owner shares is the folded dict; `sd` itself stays the checkpoint
            shared_sd = fold_batch_norm(sd) if fold else sd
            if cmd_args.hip_graph:
                from primia_amd.secure import GraphedSecureInference

                model = GraphedSecureInference(shared_sd, device, input_size=size, precision_fractional=cmd_args.precision_fractional,
                                               seed=cmd_args.debug_dealer_seed, batch=bs, form=form)
            else:
                ctx = SecureContext(Dealer(device, seed=cmd_args.debug_dealer_seed, fss_bits=fss_bits), base=10,
                                    precision_fractional=cmd_args.precision_fractional)
                model = SecureResNet18(ctx, shared_sd, input_size=size, form=form)
            if reveal in ("confusion", "metrics"):      # an evaluation: the passes return nothing, the matrix is opened after the last
                model.begin()
                for i in range(0, images.shape[0], bs):
                    model(images[i:i + bs], labels=labels[i:i + bs])
                if reveal == "metrics":
                    matrix, rank_counts = (t.cpu() for t in model.finish())
                else:
                    matrix = model.finish().cpu()
            else:
                for i in range(0, images.shape[0], bs):
                    out = model(images[i:i + bs]).clone()     # (the graphed form returns its static output buffer: keep a copy)
                    if reveal == "class":      # int64 class indices: all the pass opened
                        total_pred += [int(c) for c in out.tolist()]
                    else:
                        logits.append(out)
                        total_pred += [int(c) for c in out.argmax(dim=1).tolist()]
        if logits and os.environ.get("PRIMIA_DUMP_LOGITS"):
            torch.save(torch.cat(logits).cpu(), os.environ["PRIMIA_DUMP_LOGITS"])
    else:
        # no running statistics: the BatchNorm-free network of differentially private training
        eng = ResNet18Engine(1, sd["fc.weight"].shape[0], sd["conv1.weight"].shape[1], size,
                             pooling, dtype=torch.float32, device=device, norm=norm_of(sd.keys()))
        eng.load_state_dict(sd)
        eng.eval()
        for i in range(images.shape[0]):
            logits.append(eng.forward(images[i:i + 1]).float().cpu())
            total_pred.append(int(logits[-1].argmax(dim=1).item()))
    if evaluate:
        from primia_amd.torchlib_compat import auc_from_rank_counts, confusion_mcc, confusion_report, stats_table

        # everything below is a function of the confusion matrix alone -- which is all --reveal confusion opened; the other
        # forms count the predictions they opened against the labels.  The ROC AUC comes from the logits, or with --reveal metrics from
        # the opened pair counts.
        if matrix is None:
            matrix = confusion_of(labels, total_pred, classes)
        cm = matrix.numpy()
        mcc = confusion_mcc(cm)
        auc = roc_auc_of(labels, torch.cat([t.float().cpu() for t in logits])) if reveal == "logits" and logits else None
        result = {"n": int(cm.sum()), "confusion_matrix": cm.tolist(), "mcc": mcc}
        if rank_counts is not None:
            auc = result["roc_auc"] = auc_from_rank_counts(rank_counts.numpy(), cm.sum(axis=1))
        print(stats_table(cm, confusion_report(cm), roc_auc=auc, matthews_coeff=mcc, class_names=class_names))
        print(json.dumps({"Evaluation": result}))
        print("Took {:s} seconds.".format(str(datetime.now() - start_time)), file=sys.stderr)
        sys.exit(0)
    print(json.dumps({"Inference Results": {i: p for i, p in enumerate(total_pred)}}))
    print("Took {:s} seconds.".format(str(datetime.now() - start_time)), file=sys.stderr)
