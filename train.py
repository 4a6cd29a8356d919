#!/usr/bin/env python3
"""PriMIA-compatible training CLI on the MI355X engine.

Same command line, INI keys and worker CSV as the reference's train.py (train.py:555-631):

    python train.py --config configs/torch/pneumonia-resnet-pretrained.ini --train_federated \
        [--unencrypted_aggregation] [--data_dir DIR|synthetic] [--cuda] [--resume_checkpoint P] \
        [--save_file F] [--training_name N] [--hip_graph] [--dp_noise {torch,chacha}] [--debug_dp_noise_seed N] \
        [--dp_norm {group,frozen}] [--dp_sampling {shuffle,poisson}] [--dp_delta D] [--dp_micro_batches K] \
        [--dp_clip {fixed,adaptive}] [--dp_clip_quantile G] [--dp_clip_lr R] [--dp_clip_sigma S] [--dp_clip_init C] \
        [--dp_augmult M] [--dp_weight_sigma S]

Two deployments of the same federated epoch (torchlib/utils.py:936-1233):

  * plain launch: every client of configs/websetting/config.csv lives in this process on GPU 0 and is visited
    in turn, like the reference's VirtualWorkers (`torchlib_compat.train_federated`);
  * `python -m torch.distributed.run --nproc-per-node K train.py ... --train_federated`: rank k IS client k of the CSV
    (crypto_provider row excluded, utils.py:531-542) on GPU k; the process group is created before anything touches
    the GPU's allocator, FedAvg is an RCCL all-reduce of the flat arena (`fed.federated_epoch`), secure aggregation
    hides every client's encoded update under pairwise one-time masks, rank 0 validates and writes the checkpoints.
    K must equal the number of clients in the CSV (PRIMIA_WEBSOCKETS_CONFIG selects another CSV, e.g.
    configs/websetting/config_8gpu.csv).

`--cuda` together with `--train_federated` is legal here (the reference refuses it, train.py:617-622).
`--data_dir synthetic` trains on seeded synthetic batches; a folder is read as the reference lays it out
(`<data_dir>/worker<i>/<class>/<image>` per client, `<data_dir>/validation/<class>/<image>`; vanilla training reads
`<data_dir>/<class>/<image>`), resized / cropped / normalised on the GPU (primia_amd.imagefolder).

`--dp_sampling poisson` (with differentially_private = yes) draws every step's batch by Poisson sampling on the device
(primia_amd.dp_sampling), divides the noised sum by the expected batch size and reports the (epsilon, delta) the run
has spent per client after every epoch (primia_amd.dp_accountant); the ledger travels in the checkpoint (`dp_privacy`).
`--dp_micro_batches K` runs every DP-SGD step as K passes on an engine of 1 / K of the batch (primia_amd.dp_micro): a
logical batch larger than one engine's activations allow, with one noise draw and one optimizer step per batch.
`--dp_clip adaptive` lets every client's clipping norm follow a quantile of its per-sample gradient norms
(primia_amd.dp_clip): each step releases a noisy count, the gradient noise is raised to pay for it, and the configured
noise multiplier — what the ledger is given — stays what it was.  C and the last released fraction are printed per client
after every epoch and travel in the checkpoint (`dp_clip`).
`--dp_augmult M` (with --dp_sampling poisson; augmentation multiplicity, De et al. 2022) gives every sampled record M
augmented views — stored walks of a federated client, M passes through the training transform otherwise — averages their
gradients and clips the average once: the sensitivity, the sampling rate and the reported (epsilon, delta) are those of
M = 1, the engine holds M times as many slots (combine with --dp_micro_batches).
`weight_classes = yes` with differentially_private = yes trains on the per-sample weighted loss w[y] * CE
(primia_amd.dp_weights): every client releases its per-class record counts once with Gaussian noise of
`--dp_weight_sigma S`, the release is entered in its ledger, and the counts travel in the checkpoint (`dp_class_counts`) so
that a resumed run does not pay again.  `mixup` stays refused under DP: a mixed sample contains two records.

`main(args, verbose, optuna_trial, cmd_args)` returns the best validation MCC like the reference's.
"""
import argparse
import configparser
import os
import random
import shutil
import sys
from dataclasses import dataclass
from os import path
from types import SimpleNamespace
from typing import Optional
from warnings import warn

import numpy as np
import torch

from primia_amd.engine import ResNet18Engine
from primia_amd.optim import EngineOptimizer
from primia_amd.torchlib_compat import (Arguments, LearningRateScheduler, read_websocket_config, save_model, test,
                                        train, train_federated)

WEBSOCKETS_CONFIG = os.environ.get("PRIMIA_WEBSOCKETS_CONFIG", "configs/websetting/config.csv")


class SyntheticLoader:
    """Device-resident synthetic shard: yields (x fp32 NCHW on the GPU, int64 labels) — or, with `args` of a federated
    run that has mixup / weight_classes on, the registered form of the same samples (one-hot rows, each sample blended
    with its predecessor: torchlib/utils.py:680-734 through primia_amd.imagefolder.register)."""

    def __init__(self, n_batches, batch, size, num_classes, device, seed, channels=3, args=None):
        g = torch.Generator().manual_seed(seed)
        self.data = [(torch.randn(batch, channels, size, size, generator=g).to(device),
                      torch.randint(0, num_classes, (batch,), generator=g).to(device)) for _ in range(n_batches)]
        # (a differentially private run keeps hard labels: its class weights enter the per-sample loss, dp_loss_backward)
        if args is not None and getattr(args, "train_federated", False) and (
                args.mixup or (args.weight_classes and not getattr(args, "differentially_private", False))):
            from types import SimpleNamespace

            from primia_amd.imagefolder import register

            once = SimpleNamespace(**{**vars(args), "repetitions_dataset": 1})   # synthetic shards are not repeated
            x, y = register([torch.cat([d for d, _ in self.data])], torch.cat([t for _, t in self.data]), once,
                            num_classes, seed)
            self.data = [(x[i * batch:(i + 1) * batch], y[i * batch:(i + 1) * batch]) for i in range(n_batches)]

    def __len__(self):
        return len(self.data)

    def __iter__(self):
        return iter(self.data)

    @property
    def targets(self):
        return torch.cat([t for _, t in self.data])


PRETRAINED_FILES = ("resnet18-5c106cde.pth", "resnet18-f37072fd.pth")      # torchvision's ImageNet ResNet-18 files


def load_pretrained(engine, num_classes, rank=0, world=1):
    """`pretrained = yes` (torchlib/models.py:488-496): the ImageNet state dict goes into the freshly constructed
    network, then `fc` is REPLACED by a new Linear(512, num_classes) with torch's default initialisation.  The
    reference downloads the file; here it is read from PRIMIA_PRETRAINED_RESNET18 or torch's hub cache
    (~/.cache/torch/hub/checkpoints/) — there is no network on the training box.  A missing file ENDS the run (the
    reference's main preset depends on these weights; training from scratch instead would be a different experiment)
    unless PRIMIA_ALLOW_RANDOM_INIT=1 says that is what is wanted.  Under torch.distributed.run rank 0 reads the file
    and every rank takes rank 0's arena, so all clients start from the same model whatever their own caches hold."""
    if engine.norm == "group":
        raise SystemExit("pretrained ImageNet weights carry BatchNorm statistics; differentially_private = yes builds "
                         "a GroupNorm network (train.py:304-334).  --dp_norm frozen keeps the BatchNorm network and "
                         "applies it with those statistics held fixed")
    # rank 0's outcome travels to every rank BEFORE anybody raises: 1 loaded, 0 no file, 2 the file does not fit / does
    # not load (a SystemExit on rank 0 alone left the others blocked in the broadcast until the RCCL timeout)
    status, problem = 1, ""
    if rank == 0:
        cands = [os.environ.get("PRIMIA_PRETRAINED_RESNET18")] + [
            path.join(path.expanduser("~"), ".cache", "torch", "hub", "checkpoints", f) for f in PRETRAINED_FILES]
        src = next((c for c in cands if c and path.isfile(c)), None)
        if src is None:
            status = 0
        else:
            try:
                sd = torch.load(src, map_location="cpu", weights_only=True)
                own = engine.state_dict()
                for k, v in sd.items():
                    if k.startswith("fc."):
                        continue
                    if k not in own or tuple(own[k].shape) != tuple(v.shape):
                        raise ValueError("{:s} does not fit this network ({} vs {})".format(
                            k, tuple(v.shape), tuple(own[k].shape) if k in own else None))
                    own[k] = v.to(torch.float32)
                fc = torch.nn.Linear(512, num_classes)        # model.fc = nn.Linear(512 * block.expansion, num_classes)
                own["fc.weight"], own["fc.bias"] = fc.weight.detach().clone(), fc.bias.detach().clone()
                engine.load_state_dict(own)
            except Exception as e:  # noqa: BLE001 - reported on every rank below
                status, problem = 2, "{:s}: {:s}".format(src, str(e))
    if world > 1:
        import torch.distributed as dist

        flag = torch.tensor([status], device=engine.flat.device)
        dist.broadcast(flag, 0)
        status = int(flag.item())
    if status == 2:
        raise SystemExit("pretrained = yes, but the ImageNet state dict could not be used" + (": " + problem if problem else
                         " (see rank 0's message)"))
    found = status == 1
    if not found:
        msg = ("pretrained = yes, but no ImageNet ResNet-18 state dict was found (set PRIMIA_PRETRAINED_RESNET18 to a "
               "torchvision resnet18 .pth)")
        if os.environ.get("PRIMIA_ALLOW_RANDOM_INIT") != "1":
            raise SystemExit(msg + "; PRIMIA_ALLOW_RANDOM_INIT=1 trains from the random initialisation instead")
        warn(msg + ": training starts from the random initialisation (PRIMIA_ALLOW_RANDOM_INIT=1)")
    if world > 1:
        dist.broadcast(engine.flat, 0)          # found or not: every client starts from rank 0's model
        engine.refresh_weights()
    return found


def setup_workers(args):
    """setup_pysyft (torchlib/utils.py:516-542): worker list from the CSV, crypto_provider split off."""
    worker_dict = read_websocket_config(WEBSOCKETS_CONFIG)
    names = [w["id"] for w in worker_dict.values()]
    crypto_in_config = "crypto_provider" in names
    assert args.unencrypted_aggregation or crypto_in_config, "No crypto provider in configuration"
    if crypto_in_config:
        names.remove("crypto_provider")
    return names, ("crypto_provider" if crypto_in_config else None)


def init_distributed():
    """(rank, world, device).  Under torch.distributed.run the process group is created FIRST, bound to this rank's
    GPU (backend "nccl" = RCCL; PRIMIA_BACKEND=gloo lets several ranks share one GPU in the tests)."""
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if not torch.cuda.is_available():
        raise SystemExit("primia_amd trains on the GPU only (HIP kernels); no GPU visible")
    device = torch.device("cuda", local_rank % torch.cuda.device_count())
    torch.cuda.set_device(device)
    if world == 1:
        return 0, 1, device
    import torch.distributed as dist

    backend = os.environ.get("PRIMIA_BACKEND", "nccl")
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=device)
    else:
        dist.init_process_group(backend)
    return dist.get_rank(), world, device


def resume(cmd_args, args, model, optimizer, worker_names, state=None):
    """The four checkpoint / configuration combinations of train.py:344-389.  Returns the epoch to start at —
    `state["epoch"]` itself, as the reference does (the saved epoch is run again).  `state`: the checkpoint, when the
    caller has loaded it already."""
    if state is None:
        state = torch.load(cmd_args.resume_checkpoint, map_location="cpu", weights_only=False)
    ckpt_args = state["args"]
    was_federated = bool(getattr(ckpt_args, "train_federated", False))
    opt_sd = state["optim_state_dict"]
    if args.train_federated and was_federated:
        for w in worker_names:
            if w not in opt_sd:
                warn("The worker names of the checkpoint and the current configuration cannot be matched.")
                raise SystemExit(1)
            if w in optimizer:          # per-rank launch: each rank restores its own client's optimizer
                optimizer[w].load_state_dict(opt_sd[w])
        for m in model.values():
            m.load_state_dict(state["model_state_dict"])
    elif args.train_federated and not was_federated:
        assert len(opt_sd) == 2 and "param_groups" in opt_sd and "state" in opt_sd  # no federated checkpoint
        for w in worker_names:
            if w in optimizer:
                optimizer[w].load_state_dict(opt_sd)
        for m in model.values():
            m.load_state_dict(state["model_state_dict"])
    elif not args.train_federated and was_federated:
        # no optimizer is loaded.  (The reference indexes model_state_dict["local_model"] here although save_model
        # stores the local model's state dict itself, utils.py:1484-1486 — both layouts are accepted.)
        sd = state["model_state_dict"]
        model.load_state_dict(sd["local_model"] if "local_model" in sd else sd)
    else:
        optimizer.load_state_dict(opt_sd)
        model.load_state_dict(state["model_state_dict"])
    return state["epoch"]


@dataclass(frozen=True)
class DPOptions:
    """What the command line and the config ask of DP-SGD, read once (`from_args`) at the top of main.  Without
    differentially_private = yes every --dp_* flag warns and does nothing."""
    on: bool = False                # differentially_private = yes
    noise: str = "torch"            # --dp_noise
    noise_seed: Optional[int] = None    # --debug_dp_noise_seed
    norm: str = "group"             # --dp_norm
    poisson: bool = False           # --dp_sampling poisson: batches are Poisson-sampled and an (epsilon, delta) is reported
    delta: float = 1e-5             # --dp_delta
    # K of --dp_micro_batches: every loader batch is one logical DP-SGD step run as K passes of an engine of 1 / K of its
    # size (primia_amd.dp_micro; plain gradient accumulation would change BatchNorm's statistics)
    micro: int = 1
    sigma: float = 1.3              # the noise multiplier: what every engine applies and every ledger is given
    # --dp_clip adaptive: the AdaptiveClip parameters and z_delta, or None for the fixed C = 1.  The count's noise is
    # --dp_clip_sigma or batch_size / 20 — the step's divisor B in shuffle and in Poisson mode alike, and a loader's ragged
    # last batch keeps it — and must exceed sigma / 2, else the run ends in from_args
    clip: Optional[dict] = None
    # M of --dp_augmult: every Poisson-sampled record fills M consecutive slots with augmented views whose gradients are
    # averaged and clipped once (engine.dp_loss_backward(views=M)); batches, capacities and the ledger count records
    augmult: int = 1
    # weight_classes = yes under DP: the per-sample weighted loss (engine.dp_loss_backward) with weights formed from every
    # client's per-class counts, released once with Gaussian noise of --dp_weight_sigma (primia_amd.dp_weights)
    weighted: bool = False
    weight_sigma: float = 20.0

    @classmethod
    def from_args(cls, args, cmd_args):
        """`cmd_args`: the parsed command line, a namespace that lacks some flags, or None (main() called from a study)."""
        def flag(name, default):
            return getattr(cmd_args, name, default)

        on = bool(args.differentially_private)
        sigma = cls.sigma       # (the field's default: the one place the number lives)

        def no_effect(text, consequence):
            warn("{:s} has no effect: the config has differentially_private = no, {:s}".format(text, consequence))

        noise, norm, sampling = flag("dp_noise", "torch"), flag("dp_norm", "group"), flag("dp_sampling", "shuffle")
        micro, adaptive = max(1, int(flag("dp_micro_batches", 1))), flag("dp_clip", "fixed") == "adaptive"
        augmult = int(flag("dp_augmult", 1))
        if augmult < 1:
            raise SystemExit("--dp_augmult {:d}: the views of a record, at least 1".format(augmult))
        if on and getattr(args, "mixup", False):
            raise SystemExit("differentially_private = yes cannot be combined with mixup: a mixed sample contains two "
                             "records, so one record is no longer bounded by one clipped gradient, and under Poisson "
                             "sampling the pairing itself depends on who was drawn")
        weighted = on and bool(getattr(args, "weight_classes", False))
        weight_sigma = float(flag("dp_weight_sigma", cls.weight_sigma))
        if not weight_sigma > 0.0:
            raise SystemExit("--dp_weight_sigma {:g}: the standard deviation of the noise on the released class counts "
                             "must be positive (exact counts of private records are not free)".format(weight_sigma))
        if on and augmult > 1 and sampling != "poisson":
            raise SystemExit("--dp_augmult {:d} needs --dp_sampling poisson: shuffled loaders hand out samples, not records "
                             "with their augmented views".format(augmult))
        if not on:
            if augmult > 1:
                no_effect("--dp_augmult {:d}".format(augmult), "every sample is one view")
            if noise == "chacha":
                no_effect("--dp_noise chacha", "no noise is applied")
            if norm == "frozen":
                no_effect("--dp_norm frozen", "BatchNorm trains as usual")
            if sampling == "poisson":
                no_effect("--dp_sampling poisson", "batches are shuffled as usual and no (epsilon, delta) is reported")
            if micro > 1:
                no_effect("--dp_micro_batches {:d}".format(micro), "every batch is one pass")
            if adaptive:
                no_effect("--dp_clip adaptive", "no gradient is clipped")
        elif norm == "frozen" and not args.pretrained:
            warn("--dp_norm frozen without pretrained = yes: the frozen statistics are the initial mean 0 / variance 1, every "
                 "norm layer is a learned per-channel affine map")
        clip = None
        if on and adaptive:
            from primia_amd import dp_clip

            given = flag("dp_clip_sigma", None)
            sigma_b = float(given) if given is not None else args.batch_size / 20.0
            try:
                z_delta = dp_clip.z_delta(sigma, sigma_b)
            except ValueError:
                raise SystemExit("--dp_clip adaptive: the count's noise {:s} = {:g} must exceed half the noise multiplier, "
                                 "{:g} / 2 = {:g}: below that bound no gradient noise can pay for the count's release".format(
                                     "--dp_clip_sigma" if given is not None else "batch_size / 20", sigma_b, sigma,
                                     sigma / 2.0))
            params = {"init": float(flag("dp_clip_init", 1.0)), "quantile": float(flag("dp_clip_quantile", 0.5)),
                      "lr": float(flag("dp_clip_lr", 0.2)), "sigma_b": sigma_b}
            try:
                dp_clip.AdaptiveClip("cpu", **params)       # (refuses a quantile outside (0, 1), a negative rate, an init out of range)
            except ValueError as e:
                raise SystemExit("--dp_clip adaptive: {:s}".format(str(e)))
            clip = dict(params, z_delta=z_delta)
        return cls(on=on, noise=noise, noise_seed=flag("debug_dp_noise_seed", None), norm=norm,
                   poisson=on and sampling == "poisson", delta=float(flag("dp_delta", 1e-5)), micro=micro if on else 1,
                   sigma=sigma, clip=clip, augmult=augmult if on else 1, weighted=weighted, weight_sigma=weight_sigma)


def micro_batch_size(slots, k, poisson):
    """M, the slots of one pass: batch_size / K in shuffle mode, where a batch_size K does not divide is refused;
    ceil(capacity / K) in Poisson mode (the K * M - capacity extra slots are padding)."""
    if poisson:
        return -(-int(slots) // int(k))
    if int(slots) % int(k):
        raise SystemExit("--dp_micro_batches {:d} does not divide batch_size {:d}: the passes of a shuffled batch are all "
                         "the same size".format(int(k), int(slots)))
    return int(slots) // int(k)


def saved_clip(state):
    """{client: AdaptiveClip state} of a loaded checkpoint's `dp_clip` ({} with a warning when it has none)."""
    saved = state.get("dp_clip")
    if saved is None:
        warn("the checkpoint holds no dp_clip entry: every client's clipping norm starts at --dp_clip_init")
        return {}
    return dict(saved)


def poisson_plan(name, n, batch_size, epochs, delta, sigma, spent=None, releases=()):
    """(q, planned steps, capacity) of a client with n records: q = floor(batch_size * 2^64 / n) / 2^64 — the probability
    the kernel samples with is the one the accountant is given — over epochs * ceil(n / batch_size) steps.  An expected
    batch that is not below the record count (q >= 1) ends the run: that is not a sampled mechanism.
    `spent` (a resumed run): the checkpoint's ledger.  The plan is then its steps plus the `epochs` still to run, and the
    capacity is the one that keeps the truncation event of ALL of them — the earlier steps at the capacities they ran
    at — within its 1% of delta.  `releases`: the (sigma, sensitivity) of every one-off release the ledger holds or will
    hold (the class counts of weight_classes): the capacity is sized on the epsilon of the steps PLUS those."""
    from primia_amd import dp_accountant

    try:
        q = dp_accountant.q_of_threshold(dp_accountant.threshold_for((batch_size, n)))
    except ValueError as e:
        raise SystemExit("--dp_sampling poisson, {:s}: batch_size {:d} over {:d} records: {:s}".format(
            name, batch_size, n, str(e)))
    ahead = epochs * -(-n // batch_size)
    if spent is None or not spent.steps:
        if not releases:
            return q, ahead, dp_accountant.capacity_for(n, q, ahead, delta, sigma=sigma)
        eps = dp_accountant.epsilon([[q, sigma, ahead]], dp_accountant.DELTA_SHARE * delta, releases=releases)[0]
        return q, ahead, dp_accountant.capacity_for(n, q, ahead, delta, eps=eps)
    eps = dp_accountant.epsilon(spent.segments + [[q, sigma, ahead]], dp_accountant.DELTA_SHARE * delta,
                                releases=releases)[0]
    return q, spent.steps + ahead, dp_accountant.capacity_for(n, q, ahead, delta, eps=eps,
                                                              spent=spent.truncation_mass())


def saved_privacy(state):
    """{client: Ledger} of a loaded checkpoint's `dp_privacy` ({} with a warning when it has none: it was not trained
    under Poisson sampling, what it spent is unknown)."""
    from primia_amd.dp_accountant import Ledger

    saved = state.get("dp_privacy")
    if saved is None:
        warn("the checkpoint holds no dp_privacy ledger: the reported (epsilon, delta) covers this run's steps only")
        return {}
    return {name: Ledger.from_state_dict(d) for name, d in saved.items()}


def main(args, verbose=True, optuna_trial=None, cmd_args=None):
    rank, world, device = init_distributed()
    torch.manual_seed(args.seed)
    random.seed(args.seed)
    np.random.seed(args.seed)
    num_classes = 3
    size = args.train_resolution
    channels = 3 if args.pretrained else 1
    if args.model != "resnet-18":
        raise NotImplementedError("only resnet-18 is on the accelerated path")
    if world > 1 and not args.train_federated:
        raise SystemExit("several ranks are several federated clients: launch with --train_federated")
    # (refuses DP with mixup — the per-sample clipped gradients take hard labels of ONE record — before any data is registered)
    dp = DPOptions.from_args(args, cmd_args)
    dtype = torch.float32 if os.environ.get("PRIMIA_DTYPE", "bf16") == "f32" else torch.bfloat16
    n_batches = int(os.environ.get("PRIMIA_SYNTHETIC_BATCHES", 8))
    synthetic = args.data_dir in (None, "synthetic")
    if not synthetic:
        if not path.isdir(str(args.data_dir)):
            # (round 2 silently trained on synthetic batches here)
            raise SystemExit("data_dir {!r} does not exist; pass --data_dir synthetic for seeded synthetic batches".format(
                args.data_dir))
        from primia_amd import imagefolder

    if dp.micro > 1 and not dp.poisson:     # (refused before any data is registered; a Poisson capacity is rounded up)
        m = micro_batch_size(args.batch_size, dp.micro, False)
        if rank == 0:
            print("dp_micro_batches: every step of {:d} samples runs as K = {:d} passes on an engine of M = {:d} "
                  "slots".format(args.batch_size, dp.micro, m))
    # --dp_clip adaptive: the ledger keeps receiving dp.sigma — the count's release is paid for by the gradient's noise
    if dp.clip is not None and rank == 0:
        print("dp_clip: adaptive clipping norm from C = {init:g}, target quantile {quantile:g}, rate {lr:g}, count noise "
              "{sigma_b:g}; gradient noise {z_delta:.4f} * C for a mechanism of multiplier {z:g}".format(z=dp.sigma,
                                                                                                       **dp.clip))
    clips = {}          # {client name: dp_clip.AdaptiveClip} of the engines that take steps
    privacy = {}        # Poisson sampling: {client name: dp_accountant.Ledger}
    # a resumed Poisson run sizes every client's capacity from what the checkpoint's ledger has spent plus the epochs
    # still to run, so the checkpoint is read before the loaders are built (and once: resume() below takes it)
    resume_state, spent, epochs_ahead = None, {}, args.epochs
    if cmd_args is not None and getattr(cmd_args, "resume_checkpoint", None):
        resume_state = torch.load(cmd_args.resume_checkpoint, map_location="cpu", weights_only=False)
        if dp.poisson:
            spent = saved_privacy(resume_state)
            epochs_ahead = max(0, args.epochs - int(resume_state["epoch"]) + 1)      # (the saved epoch is run again)
    reps = args.repetitions_dataset if "repetitions_dataset" in vars(args) else 1

    def saved_counts(name):
        """weight_classes under DP: the class counts client `name` released in the resumed checkpoint (`dp_class_counts`),
        or None.  Counts released at this run's --dp_weight_sigma are used again and not paid for twice; at another sigma
        the client releases again, and its ledger then holds both."""
        held = (resume_state or {}).get("dp_class_counts") or {}
        entry = held.get(name)
        if entry is None or float(entry["sigma"]) != dp.weight_sigma or len(entry["counts"]) != num_classes:
            return None
        if dp.poisson:      # ... and only where the checkpoint's ledger shows that release paid for
            old = spent.get(name)
            if old is None or not any(s == dp.weight_sigma for s, _, _ in old.releases):
                return None
        return [int(c) for c in entry["counts"]]

    augmult_warned = []     # (the warning about repeated stored views is given once)

    def poisson_loader(name, base, client):
        """The Poisson-sampled form of a client's loader: its records, an expected batch of batch_size, the capacity the
        planned number of steps needs, a sampler and a ledger of the client's own (nonce rule: make_engine's)."""
        from primia_amd import dp_accountant, dp_sampling as dps

        # (a registered folder holds repetitions_dataset walks of its records; synthetic shards are not repeated)
        fed_reps = int(reps or 1) if args.train_federated and not synthetic else 1
        n = dps.records_of(base, fed_reps)
        old = spent.get(name)
        if spent and old is None:
            warn("the checkpoint's dp_privacy has no ledger for {:s}: its count starts at zero".format(name))
        if old is not None and old.n != n:
            warn("{:s}: the checkpoint counted {:d} records, this run has {:d}; its segments are kept as they are".format(
                name, old.n, n))
        # the one-off releases the ledger will hold: the checkpoint's, and this run's class counts unless they are reused
        releases = [(s, k) for s, k, _ in old.releases] if old is not None else []
        if dp.weighted and saved_counts(name) is None:
            releases.append((dp.weight_sigma, 1.0))
        _, planned, capacity = poisson_plan(name, n, args.batch_size, epochs_ahead, dp.delta, dp.sigma, spent=old,
                                            releases=releases)
        nonce = client if client is not None else 0
        sampler = dps.DeviceSampler(device, nonce=nonce, debug_seed=dp.noise_seed)
        led = privacy[name] = dp_accountant.Ledger(n, capacity, dp.delta, planned)
        if old is not None:     # the ledger goes on counting; a changed q, sigma or capacity opens a new segment
            led.segments, led.capacities, led.overflow_events = old.segments, old.capacities, old.overflow_events
            led.releases = old.releases
        if dp.micro > 1 and rank == 0:
            print("dp_micro_batches: {:s}'s steps of capacity {:d} run as K = {:d} passes on an engine of M = {:d} "
                  "slots".format(name, capacity, dp.micro, micro_batch_size(capacity, dp.micro, True) * dp.augmult))
        if dp.augmult > 1:
            stored = not hasattr(base, "images")      # (stored walks; a transforming loader draws fresh views)
            if stored and dp.augmult > fed_reps and not augmult_warned:
                augmult_warned.append(name)
                warn("--dp_augmult {:d} with {:d} stored walk(s) per record: the views repeat stored copies, and identical "
                     "views add nothing to the average".format(dp.augmult, fed_reps))
            if rank == 0:
                print("dp_augmult: {:s}: capacity {:d} records, {:d} views per record, engine of {:d} slots".format(
                    name, capacity, dp.augmult, micro_batch_size(capacity, dp.micro, True) * dp.augmult))
        return dps.from_loader(base, args.batch_size, capacity, sampler, fed_reps, (channels, size, size),
                               micro_batches=dp.micro, views=dp.augmult)

    def synthetic_records(batches, seed):
        sl = SyntheticLoader(batches, args.batch_size, size, num_classes, device, seed, channels)
        from primia_amd.imagefolder import DeviceLoader

        return DeviceLoader(torch.cat([d for d, _ in sl.data]), sl.targets, args.batch_size, True, seed)

    def make_engine(client=None, batch=None, expected_batch=None, name=None):
        # differentially_private = yes (train.py:304-334 of the reference): BatchNorm is rejected by the
        # PrivacyEngine, so the network is built with GroupNorm — or (--dp_norm frozen) BatchNorm is applied with its
        # running statistics held fixed, which keeps samples independent too — and every step clips / noises per sample
        # (--dp_micro_batches K: the engine holds one PASS, 1 / K of the loaders' batch or capacity)
        # (--dp_augmult M: batch, capacity and M-of-a-pass count records; the engine holds M slots per record)
        views = dp.augmult if expected_batch is not None else 1     # (the model that only holds the aggregate: no records)
        slots = micro_batch_size(args.batch_size if batch is None else batch, dp.micro, dp.poisson) * views
        eng = ResNet18Engine(slots, num_classes, channels, size, args.pooling_type,
                             dtype=dtype, device=device, norm=dp.norm if dp.on else "batch")
        if dp.on:
            eng.dp_micro_batches = dp.micro
            eng.dp_params = {"max_grad_norm": 1.0, "noise_multiplier": dp.sigma}
            if expected_batch is not None:      # padded Poisson batches: masked loss / clip, the noised sum over q * n
                eng.dp_params["expected_batch"] = float(expected_batch)
            if views > 1:
                eng.dp_params["views"] = views
            if dp.noise == "chacha":
                # a key of its own from the OS entropy pool per engine; the nonce is the client index (the model that
                # holds a federated run's aggregate never takes a step: it gets the last nonce; a vanilla run's one model
                # has nonce 0 like federated client 0 — independent under OS keys, the SAME stream under a debug seed)
                from primia_amd.dp_noise import DeviceNoise

                nonce = client if client is not None else (2 ** 64 - 1 if args.train_federated else 0)
                eng.dp_noise = DeviceNoise(device, nonce=nonce, debug_seed=dp.noise_seed)
            if dp.clip is not None and name is not None:
                # a state of its own per model that takes steps (FedAvg averages weights, never clipping norms)
                from primia_amd.dp_clip import AdaptiveClip

                eng.dp_clip = clips[name] = AdaptiveClip(device, **{k: v for k, v in dp.clip.items() if k != "z_delta"})
                eng.dp_clip.tensors()       # on the device before any step graph is captured
        return eng

    vanilla_loader = None
    if dp.poisson and not args.train_federated:
        # the engine's batch is the capacity, which follows from the record count: the loader comes first
        if synthetic:
            base = synthetic_records(max(2, n_batches), args.seed)
        else:
            base, (m, s) = imagefolder.client_loader(args.data_dir, args, device, channels, args.seed)
            val_mean_std_vanilla = (m.cpu(), s.cpu())
        vanilla_loader = poisson_loader("model", base, None)
        local = make_engine(batch=vanilla_loader.capacity, expected_batch=vanilla_loader.expected_batch,
                            name=None if args.train_federated else "model")
    else:
        local = make_engine(name=None if args.train_federated else "model")
    local.init_weights()
    if args.pretrained:
        load_pretrained(local, num_classes, rank, world)
    val_mean_std = (torch.zeros(channels), torch.ones(channels))
    exp_name = "{:s}_{:s}".format("federated" if args.train_federated else "vanilla", args.name)
    group = None
    masks = None

    if args.train_federated:
        workers, crypto_provider = setup_workers(args)
        if world > 1:
            import torch.distributed as dist

            from primia_amd import fed

            if len(workers) != world:
                raise SystemExit("{:d} ranks but {:d} clients in {:s}: one rank per client".format(
                    world, len(workers), WEBSOCKETS_CONFIG))
            mine = [workers[rank]]
        else:
            mine = list(workers)
        model = {"local_model": local}
        train_loader, stats = {}, {}

        def client_data(w):
            i = workers.index(w)
            if synthetic and dp.poisson:
                train_loader[w] = poisson_loader(w, synthetic_records(max(2, n_batches - i), args.seed + i), i)
                stats[w] = (torch.zeros(channels, device=device), torch.ones(channels, device=device))
            elif synthetic:
                # deliberately uneven shards (exercises weighted averaging and exhausted clients)
                train_loader[w] = SyntheticLoader(max(1, n_batches - i), args.batch_size, size, num_classes, device,
                                                  args.seed + i, channels, args)
                stats[w] = (torch.zeros(channels, device=device), torch.ones(channels, device=device))
            else:
                train_loader[w], stats[w] = imagefolder.client_loader(
                    path.join(args.data_dir, "worker{:d}".format(i + 1)), args, device, channels, args.seed + i)
                if dp.poisson:
                    train_loader[w] = poisson_loader(w, train_loader[w], i)

        if dp.poisson:  # the engine's batch is the capacity, which follows from the record count: the loaders come first
            for w in mine:
                client_data(w)
        for w in mine:
            tl = train_loader.get(w)
            model[w] = make_engine(client=workers.index(w), batch=tl.capacity if dp.poisson else None,
                                   expected_batch=tl.expected_batch if dp.poisson else None, name=w)
            model[w].load_state_dict(local.state_dict())
        if not dp.poisson:
            for w in mine:
                client_data(w)
        # setup_pysyft's secure average of the clients' (mean, std) (utils.py:764-794) -> val_mean_std
        if world > 1 and not args.unencrypted_aggregation:
            masks = fed.PairwiseMasks.setup(local.flat.numel(), device, group)
        if world > 1:
            m, s = fed.exchange_mean_std(*stats[mine[0]], masks=masks)
        else:
            from primia_amd import fed

            m, s = fed.secure_mean_of([stats[w] for w in mine])
        val_mean_std = (m.cpu(), s.cpu())
        optimizer = {w: EngineOptimizer.from_args(model[w], args) for w in mine}
        # train.py:335-342: Cross_entropy_one_hot (soft targets) with mixup or federated weight_classes
        # (a DP run's weight_classes keeps hard labels: the weights enter the per-sample loss)
        soft = bool(args.mixup or (args.weight_classes and not dp.on))
        loss_fn = {w: SimpleNamespace(soft=soft) for w in mine}
    else:
        workers, mine = [], []
        model = local
        if vanilla_loader is not None:
            train_loader = vanilla_loader
            if not synthetic:
                val_mean_std = val_mean_std_vanilla
        elif synthetic:
            train_loader = SyntheticLoader(n_batches, args.batch_size, size, num_classes, device, args.seed, channels)
        else:
            train_loader, (m, s) = imagefolder.client_loader(args.data_dir, args, device, channels, args.seed)
            val_mean_std = (m.cpu(), s.cpu())
        optimizer = EngineOptimizer.from_args(model, args)
        loss_fn = None
    if synthetic or not path.isdir(path.join(str(args.data_dir), "validation")):
        val_loader = SyntheticLoader(2, args.batch_size, size, num_classes, device, args.seed + 999, channels)
    else:
        val_loader = imagefolder.validation_loader(path.join(args.data_dir, "validation"), args, device, channels,
                                                   val_mean_std)

    # class weights (train.py:192-195, utils.py:469-513): counted over the training targets of every client — across
    # ranks the per-class counts are summed — and handed to every engine's loss
    class_counts_released = {}      # DP: {client: {"counts": [...], "sigma": s}}, the checkpoint's `dp_class_counts`
    if dp.weighted:
        # Under DP the counts are a release of private data (primia_amd.dp_weights): every client's per-class RECORD counts
        # are noised on its own stream (or taken from the resumed checkpoint) BEFORE anything is summed, the ledger is
        # charged once, the noised integers are summed like the exact ones below, and balanced_weights — 1.0 everywhere on
        # balanced data — is applied once; the per-sample weighted loss is dp_loss_backward's
        from primia_amd.dp_weights import balanced_weights, noised_counts

        loaders = train_loader if isinstance(train_loader, dict) else {"model": train_loader}
        engines_by_name = model if isinstance(model, dict) else {"model": model}
        occ = torch.zeros(num_classes, dtype=torch.int64, device=device)
        for name in sorted(loaders):
            counts = saved_counts(name)
            if counts is None:
                tl = loaders[name]
                t = tl.targets
                if hasattr(tl, "threshold"):        # a Poisson loader: its n records
                    t = t[:tl.n]
                elif not hasattr(tl, "images") and args.train_federated and not synthetic:
                    t = t[:t.shape[0] // int(reps or 1)]        # a registered folder holds repetitions_dataset walks
                counts = noised_counts(t.to(device), num_classes, dp.weight_sigma,
                                       engines_by_name[name].dp_noise).tolist()
                if name in privacy:
                    privacy[name].add_release(dp.weight_sigma)
            class_counts_released[name] = {"counts": counts, "sigma": dp.weight_sigma}
            occ += torch.tensor(counts, dtype=torch.int64, device=device)
        if world > 1:
            import torch.distributed as dist

            if masks is not None:
                occ = fed.masked_sum(occ, masks)
            else:
                dist.all_reduce(occ)
        cw = balanced_weights(occ).to(device).contiguous()      # ONE tensor for every engine
        for m in engines_by_name.values():
            m.class_weight = cw
        if rank == 0:
            print("dp_weights: released class counts (all clients, noise sigma {:g} per client) = {}, weights = {}".format(
                dp.weight_sigma, [int(c) for c in occ.tolist()], [round(float(w), 6) for w in cw.tolist()]))
            if not dp.poisson:
                print("dp_weights: every client's class counts were released once with Gaussian noise of sigma {:g}; "
                      "shuffle mode reports no (epsilon, delta)".format(dp.weight_sigma))
    elif args.weight_classes:
        from primia_amd.datapipe import class_counts, class_weights_from_counts

        # counted from the loaders' held targets (no batch is drawn: the augmentation and shuffle streams stay where
        # they are); across ranks the per-class COUNTS are summed (the weights are not additive), under the pairwise
        # masks when aggregation is secure
        occ = class_counts(train_loader, num_classes)
        if world > 1:
            import torch.distributed as dist

            if masks is not None:
                occ = fed.masked_sum(occ.to(device), masks).cpu()
            else:
                occ = occ.to(device)
                dist.all_reduce(occ)
                occ = occ.cpu()
        cw = class_weights_from_counts(occ)
        engines = [m for m in model.values()] if isinstance(model, dict) else [model]
        for m in engines:
            m.class_weight = cw.to(device).float().contiguous()

    start_at_epoch = 1
    if cmd_args is not None and getattr(cmd_args, "resume_checkpoint", None):
        print("Resume training from a given checkpoint.")
        start_at_epoch = resume(cmd_args, args, model, optimizer, workers, state=resume_state)
        if clips:
            old = saved_clip(resume_state)
            for name, clip in clips.items():
                if name in old:
                    # C and the update count come from the checkpoint; the parameters stay the command line's, which
                    # this run has checked against the bound and announced
                    for k, (mine_, saved) in clip.differing_parameters(old[name]).items():
                        warn("{:s}: the checkpoint's dp_clip was saved with {:s} = {}, this run uses {}".format(
                            name, k, saved, mine_))
                    clip.load_state_dict(old[name], keep_parameters=True)
                    if rank == 0:
                        print("dp_clip: {:s}: resumed at C = {:.9g} after {:d} updates".format(name, clip.value(),
                                                                                              clip.updates))
                elif old:
                    warn("the checkpoint's dp_clip has no entry for {:s}: its clipping norm starts at --dp_clip_init".format(
                        name))
    scheduler = LearningRateScheduler(args.epochs, np.log10(args.lr), np.log10(args.end_lr), restarts=args.restarts)
    poisson_loaders = train_loader if isinstance(train_loader, dict) else {"model": train_loader}
    overflow_before = {name: led.overflow_events for name, led in privacy.items()}
    counted = {name: 0 for name in privacy}

    def all_ranks(states):
        """{name: state} of every rank's clients, merged (this rank's own dict without torch.distributed.run)."""
        if world == 1:
            return states
        import torch.distributed as dist

        gathered = [None] * world
        dist.all_gather_object(gathered, states)
        return {k: v for g in gathered for k, v in g.items()}

    def account(final=False):
        """The steps this epoch sampled go into the ledgers; rank 0 prints every client's (epsilon, delta).  Returns the
        checkpoint's `dp_privacy` entry ({client: ledger state}; every rank's under torch.distributed.run)."""
        for name, led in privacy.items():
            tl = poisson_loaders[name]
            led.add_steps(tl.q, dp.sigma, tl.draws - counted[name])
            counted[name] = tl.draws
            led.overflow_events = overflow_before[name] + tl.sampler.overflow_events()
        states = all_ranks({name: led.state_dict() for name, led in privacy.items()})
        if rank == 0:
            from primia_amd.dp_accountant import Ledger

            for name in sorted(states):
                led = Ledger.from_state_dict(states[name])
                if not led.report()["within_plan"]:
                    warn("{:s}: the truncation event of {:d} steps ({:d} were planned for, capacity {:d}) no longer fits "
                         "its share of delta; the reported delta is larger than --dp_delta".format(
                             name, led.steps, led.planned_steps, led.capacity))
                print(led.line(name) + (" (end of run)" if final else ""))
        return states

    def clip_report():
        """Rank 0 prints every client's C and last released fraction — functions of released values, unlike the raw
        counts, which never leave the device.  Returns the checkpoint's `dp_clip` entry ({client: state}; every rank's
        under torch.distributed.run)."""
        states = all_ranks({name: clip.state_dict() for name, clip in clips.items()})
        if rank == 0:
            for name in sorted(states):
                print("dp_clip: {:s}: C = {:.6g}, released fraction at or below C = {:.4f} (target {:g}), {:d} "
                      "updates".format(name, states[name]["clip_norm"], states[name]["released"],
                                       states[name]["quantile"], states[name]["updates"]))
        return states

    # released values: every rank's clients', so that a resumed run uses them again and does not pay twice
    class_counts_ckpt = all_ranks(class_counts_released) if dp.weighted else None
    objectives, model_paths = [], []
    local_flat = None
    for epoch in range(start_at_epoch, args.epochs + 1):
        for o in (optimizer.values() if args.train_federated else [optimizer]):
            scheduler.adjust_learning_rate(o, epoch - 1)
        if args.train_federated and world > 1:
            w = mine[0]
            avg_loss, _, local_flat, optimizer[w] = fed.federated_epoch(
                model[w], train_loader[w], args, optimizer[w], group=group, local_flat=local_flat, masks=masks,
                soft_targets=soft)
            local.flat.copy_(local_flat)              # "local_model": the last global average
            for b in local.num_batches_tracked:
                local.num_batches_tracked[b] = 0
            local.refresh_weights()
            if verbose and rank == 0:
                print("Train Epoch: {} \tLoss: {:.6f}".format(epoch, avg_loss))
            eval_model = local
        elif args.train_federated:
            model = train_federated(args, model, device, train_loader, optimizer, epoch, loss_fn, crypto_provider,
                                    verbose=verbose)
            eval_model = model["local_model"]
        else:
            model = train(args, model, device, train_loader, optimizer, epoch, loss_fn, num_classes, verbose=verbose)
            eval_model = model
        ckpt_extra = {"dp_privacy": account()} if dp.poisson else {}
        if dp.clip is not None:
            ckpt_extra["dp_clip"] = clip_report()
        if class_counts_ckpt is not None:
            ckpt_extra["dp_class_counts"] = class_counts_ckpt
        if epoch % args.test_interval == 0:
            # the checkpoint holds every worker's optimizer state (utils.py:1471-1472): collect them on rank 0.  (One process
            # keeps handing save_model the optimizer OBJECTS, as before: not all_ranks' own world == 1 case, which would
            # hand it state dicts.)
            opt_for_ckpt = all_ranks({w: o.state_dict() for w, o in optimizer.items()}) if world > 1 else optimizer
            # rank 0 validates; what it decides (pruned / failed) reaches every rank BEFORE anybody moves on, so a
            # pruned trial or a validation error ends all ranks together instead of leaving them in a barrier until
            # the RCCL timeout.  The pruning check precedes the checkpoint, as train.py:505-517 of the reference.
            verdict = [None]        # None = go on, "pruned", or the exception rank 0 hit
            if rank == 0:
                try:
                    _, objective = test(args, eval_model, device, val_loader, epoch, loss_fn, num_classes,
                                        verbose=verbose)
                    objectives.append(objective)
                    if optuna_trial:
                        optuna_trial.report(objective, epoch * reps)
                        if optuna_trial.should_prune():
                            verdict[0] = "pruned"
                    if verdict[0] is None:
                        p = "model_weights/{:s}_epoch_{:03d}.pt".format(exp_name, epoch * reps)
                        save_model(eval_model, opt_for_ckpt, p, args, epoch, val_mean_std=val_mean_std,
                                   extra=ckpt_extra or None)
                        model_paths.append(p)
                except Exception as e:  # noqa: BLE001 - forwarded to every rank, re-raised below
                    verdict[0] = e
            if world > 1:
                dist.broadcast_object_list(verdict, src=0)
            if verdict[0] is not None:
                if world > 1:
                    dist.destroy_process_group()
                if isinstance(verdict[0], str):
                    try:
                        import optuna

                        raise optuna.TrialPruned()
                    except ImportError:
                        raise RuntimeError("trial pruned") from None
                raise verdict[0]
    if dp.poisson:
        account(final=True)
    best_score = 0.0
    if rank == 0 and objectives:
        # the LAST occurrence of the highest score wins (train.py:514-521)
        scores = np.array(objectives)[::-1]
        best = len(scores) - int(np.argmax(scores)) - 1
        final = "model_weights/final_{:s}.pt".format(exp_name)
        shutil.copyfile(model_paths[best], final)
        for p in model_paths:
            if path.exists(p):
                os.remove(p)
        best_score = float(objectives[best])
        if verbose:
            print("Highest matthews coefficient was {:.1f}% in epoch {:d}".format(
                best_score, (best + 1) * args.test_interval * (reps if args.train_federated else 1)))
    if args.hip_graph and dp.on and dp.noise == "chacha" and rank == 0:
        from primia_amd.graphed_train import captures

        engines = [m for m in (model.values() if isinstance(model, dict) else [model]) if hasattr(m, "_root")]
        n = sum(1 for e in engines for k in captures(e) if "DP with device noise" in k)
        print("hip_graph: {:d} DP-SGD step graph(s) captured and replayed".format(n), file=sys.stderr)
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return best_score


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, required=True, help="Path to the configuration file (.ini).")
    parser.add_argument("--train_federated", action="store_true", help="Train with federated learning.")
    parser.add_argument("--unencrypted_aggregation", action="store_true", help="Turns off secure aggregation.")
    parser.add_argument("--data_dir", type=str, default="data/train", help="Data folder, or 'synthetic'.")
    parser.add_argument("--visdom", action="store_true", help="Accepted for compatibility (ignored).")
    parser.add_argument("--cuda", action="store_true", help="Use GPU acceleration (always on here).")
    parser.add_argument("--resume_checkpoint", type=str, default=None, help="Start from an older checkpoint")
    parser.add_argument("--websockets", action="store_true", help="Accepted for compatibility (ignored).")
    parser.add_argument("--verbose", action="store_true")
    parser.add_argument("--save_file", type=str, default="model_weights/completed_trainings.csv")
    parser.add_argument("--training_name", default=None, type=str)
    parser.add_argument("--hip_graph", action="store_true",
                        help="training: capture each training step once as a hipGraph and replay it per batch (the "
                             "learning rate and Adam's step reach the replay on the device; FedAvg runs between replays)")
    parser.add_argument("--dp_noise", choices=("torch", "chacha"), default="torch",
                        help="differentially_private = yes: where the Gaussian noise comes from.  torch: torch.randn, seeded "
                             "by the config's seed (steps run eagerly under --hip_graph).  chacha: a ChaCha20 keystream on "
                             "the device under a key from the OS entropy pool, applied to the gradient in one kernel; "
                             "--hip_graph then replays the DP steps too.  The stream's counter is not checkpointed: a "
                             "resumed run draws a new key.")
    parser.add_argument("--debug_dp_noise_seed", type=int, default=None,
                        help="derive the --dp_noise chacha key from this seed: a reproducible, PREDICTABLE noise stream "
                             "that restarts from its beginning when a run is resumed, and is shared by a vanilla run and "
                             "federated client 0 (tests only: no privacy)")
    parser.add_argument("--dp_norm", choices=("group", "frozen"), default="group",
                        help="differentially_private = yes: the norm layers that keep samples independent.  group: "
                             "GroupNorm(32, C), trained from a random initialisation (pretrained = yes is refused).  frozen: "
                             "the BatchNorm network applied with its running statistics held fixed (gamma / beta train): "
                             "DP-SGD fine-tuning of pretrained weights; the checkpoint is an ordinary BatchNorm state dict.")
    parser.add_argument("--dp_sampling", choices=("shuffle", "poisson"), default="shuffle",
                        help="differentially_private = yes: how a step's batch is drawn.  shuffle: the loaders' seeded "
                             "shuffle, as before; no (epsilon, delta) is reported.  poisson: every record joins every "
                             "step's batch independently with probability batch_size / records, drawn on the device from a "
                             "ChaCha20 stream under an OS key; batches are padded to a fixed capacity, the noised sum is "
                             "divided by batch_size, and the (epsilon, delta) spent is printed per client after every epoch "
                             "and stored in the checkpoint (dp_privacy).")
    parser.add_argument("--dp_delta", type=float, default=1e-5,
                        help="--dp_sampling poisson: the delta of the reported (epsilon, delta)")

    parser.add_argument("--dp_clip", choices=("fixed", "adaptive"), default="fixed",
                        help="differentially_private = yes: the per-sample clipping norm C.  fixed: 1.0, as before.  "
                             "adaptive: a device word that follows a quantile of the per-sample gradient norms (each step "
                             "releases a noisy count of the samples at or below C; the gradient noise is raised so that "
                             "the step keeps the configured noise multiplier and the reported (epsilon, delta)); C is "
                             "printed per client after every epoch and stored in the checkpoint (dp_clip).")
    parser.add_argument("--dp_clip_quantile", type=float, default=0.5,
                        help="--dp_clip adaptive: the fraction of per-sample norms C aims to sit above")
    parser.add_argument("--dp_clip_lr", type=float, default=0.2,
                        help="--dp_clip adaptive: the geometric rate, C *= exp(-rate * (fraction - quantile))")
    parser.add_argument("--dp_clip_sigma", type=float, default=None,
                        help="--dp_clip adaptive: the standard deviation of the count's noise (default batch_size / 20); "
                             "must exceed half the noise multiplier, 0.65")
    parser.add_argument("--dp_clip_init", type=float, default=1.0, help="--dp_clip adaptive: the C of the first step")

    def passes(text):
        k = int(text)
        if k < 1:
            raise argparse.ArgumentTypeError("at least 1 pass per step")
        return k

    parser.add_argument("--dp_augmult", type=int, default=1, metavar="M",
                        help="with differentially_private = yes and --dp_sampling poisson: augmentation multiplicity — every "
                             "sampled record contributes the average gradient of M augmented views, clipped once (De et al. "
                             "2022).  The privacy cost is that of M = 1; the engine holds M times as many slots")
    parser.add_argument("--dp_weight_sigma", type=float, default=20.0, metavar="S",
                        help="differentially_private = yes with weight_classes = yes: the standard deviation of the Gaussian "
                             "noise every client adds to its per-class record counts before they are summed into the class "
                             "weights — a one-off release entered in the client's ledger (at n = 1721, batch 256, 280 steps: "
                             "epsilon 14.0286 without, 14.0321 with S = 20, 14.0426 with S = 10).  Must be positive")
    parser.add_argument("--dp_micro_batches", type=passes, default=1, metavar="K",
                        help="differentially_private = yes: run every step as K passes of (forward, per-sample clip, "
                             "clipped sum) on an engine of 1 / K of the batch (shuffle: batch_size must be a multiple of K) "
                             "or of the capacity (poisson: rounded up, the extra slots are padding); the sums meet in an "
                             "fp32 accumulator, noise is added once, the sum is divided once and one optimizer step "
                             "follows.  The mechanism and the reported (epsilon, delta) are those of the whole batch; "
                             "activation memory is that of one pass.")
    return parser


if __name__ == "__main__":
    parser = build_parser()
    cmd_args = parser.parse_args()
    if cmd_args.debug_dp_noise_seed is not None:
        if cmd_args.dp_noise != "chacha":
            parser.error("--debug_dp_noise_seed needs --dp_noise chacha")
        print("WARNING: --debug_dp_noise_seed makes the DP-SGD noise predictable: no differential privacy",
              file=sys.stderr)
    config = configparser.ConfigParser()
    assert path.isfile(cmd_args.config), "Configuration file not found"
    config.read(cmd_args.config)
    cmd_args.websockets = False  # in-process / RCCL clients replace the websocket transport
    args = Arguments(cmd_args, config, mode="train", verbose=int(os.environ.get("RANK", 0)) == 0)
    args.hip_graph = cmd_args.hip_graph
    if args.train_federated and (args.mixup or args.weight_classes):
        if args.mixup and args.mixup_lambda == 0.5:
            args.mixup_lambda = 0.499
    if int(os.environ.get("RANK", 0)) == 0:
        print(str(args))
    main(args, cmd_args=cmd_args)
