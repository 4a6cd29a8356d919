"""Class weights for DP-SGD (`weight_classes = yes` with `differentially_private = yes`; csrc/dp_weighted.hip).

The weights of the reference (calc_class_weights) are a function of exact per-class counts of private records.  A run
that reports an (epsilon, delta) cannot use those for free, so every client releases its counts ONCE through a Gaussian
mechanism — `noised_counts`, drawn from the client's own ChaCha20 noise stream and entered in its ledger
(dp_accountant.Ledger.add_release) — and the weights are formed from the sum of the released integers
(`balanced_weights`).  Everything after the release is post-processing.

The loss the weights enter is the per-sample one, loss_n = w[y_n] * CE_n (engine.dp_loss_backward): the weighted mean of
the non-DP path divides by the batch's weight sum, which would couple every sample's gradient to the other samples drawn.
The normalisation is therefore fixed here, before training: w_c = total / (C * count_c), which is 1 for every class of a
balanced data set — such a run trains as the unweighted step does, and max_grad_norm keeps its meaning."""
import torch

from ._lib import call

MAX_CLASSES = 16        # one block of the noise stream (primia_dp_class_counts)


def noised_counts(targets, num_classes, sigma, noise=None):
    """int64 [num_classes] on the device: max(0, rint(count_c + sigma * z_c)) over the hard labels `targets` of a client's
    RECORDS (a Poisson loader's records, not their repetitions or views).  `noise`: the client's DeviceNoise — z is its
    stream's next block and the counter moves on by one; None (--dp_noise torch): z from torch.randn."""
    if targets.dtype != torch.int64 or targets.dim() != 1:
        raise ValueError("noised_counts: hard int64 labels [n], one per record")
    C = int(num_classes)
    if not 0 < C <= MAX_CLASSES:
        raise ValueError(f"noised_counts: {C} classes; one block of the noise stream serves up to {MAX_CLASSES}")
    if not float(sigma) >= 0.0:
        raise ValueError(f"noised_counts: sigma {sigma} is negative")
    targets = targets.contiguous()
    out = torch.empty(C, dtype=torch.int64, device=targets.device)
    if noise is not None:
        ctr = noise.counter
        call("primia_dp_class_counts_chacha", *noise.key_words, noise.nonce, ctr, 0, targets, int(targets.numel()), C,
             float(sigma), out)
        call("primia_u64_add", ctr, 1)
    else:
        z = torch.randn(C, dtype=torch.float32, device=targets.device)
        call("primia_dp_class_counts", targets, int(targets.numel()), C, z, float(sigma), out)
    return out


def balanced_weights(counts):
    """fp32 [C]: w_c = sum(counts) / (C * counts_c) in float64, `counts` the sum of every client's released counts,
    clamped at 1 per class (a released count can be 0).  Equal counts give exactly 1.0 everywhere."""
    c = torch.as_tensor(counts).detach().to("cpu", torch.float64).reshape(-1).clamp(min=1.0)
    return (c.sum() / (c.numel() * c)).to(torch.float32)
