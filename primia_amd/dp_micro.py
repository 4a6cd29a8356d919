"""A DP-SGD step on a logical batch larger than the engine: `train.py --dp_micro_batches K`.

The step is linear in the per-sample terms, and samples are independent under GroupNorm and under frozen BatchNorm
statistics, so the clipped sum splits exactly:

    sum_n clip_n g_n  =  sum over micro-batches k of ( sum over the samples of micro-batch k of clip_n g_n )

The logical batch runs as passes of (forward, per-sample clip, clipped sum) on an engine of M = root.N slots.  Every pass
is told its phase ("first", "more", "last"; None for a step of one pass) and the logical batch size as ARGUMENTS, which
step.eager_step / graphed_train.graphed_step hand to loss_backward: nothing is left on the engine between passes.  Every pass
but the last adds its clipped sum to the root's fp32 accumulator (primia_dp_accumulate into engine.dp_acc), the last one
adds the accumulator, the noise — ONE draw, one counter advance — and the division in one kernel
(primia_dp_noise_add_acc), and ONE optimizer step follows.  The mechanism, its sensitivity and the accountant are those
of the whole batch; only the execution is cut into pieces (pytorch-dp calls this a virtual step).  An adaptive clipping
norm (engine.dp_clip) is read by every pass and moved once, by the last one, on the counts summed over all passes.

Not bit-identical to the same batch on one large engine: the clipped sum is added up in another order (per pass, then
across passes in float32).  Bit-identical: a pass whose slots are all padding (target -1) adds exact zeros, and a step
replayed as graphs equals the step run eagerly.
"""
import torch

from . import _lib


def views(n, size):
    """[(start, stop)] of the contiguous passes of a logical batch of n rows on an engine of `size` slots."""
    return [(s, min(s + size, n)) for s in range(0, n, size)]


def phase_of(i, count):
    """The phase of pass i of `count`: None for a step of one pass (an ordinary step)."""
    if count == 1:
        return None
    return "first" if i == 0 else ("last" if i == count - 1 else "more")


def step(engine, optimizer, data, target, hip_graph=False, soft=False):
    """One logical DP-SGD step of `engine` (the loop's model) on (data, target): contiguous views of root.N rows — a
    shorter final view runs on sibling() — each through eager_step under its phase, the last of which takes the ONE
    optimizer step.  `hip_graph`: every pass goes through graphed_step instead (one graph per phase; the last phase's
    graph holds the optimizer step; a ragged pass runs eagerly there).  `soft`: handed on — a DP engine refuses soft
    targets.  Returns a device scalar, the mean of the pass losses weighted by their valid rows; nothing here waits for
    the device."""
    root = engine._root
    if root.dp_params is None:
        raise _lib.PrimiaError("dp_micro.step: the engine has no dp_params (micro-batches are a DP-SGD feature: plain "
                               "gradient accumulation would change BatchNorm's statistics)")
    if hip_graph:
        from .graphed_train import graphed_step as one_pass
    else:
        from .step import eager_step as one_pass
    masked = root.dp_params.get("expected_batch") is not None
    n = int(data.shape[0])
    # (augmentation multiplicity: a record is dp_params["views"] consecutive rows, root.N a whole number of records — no
    # record straddles two passes — and the logical batch is counted in records)
    records = n // int(root.dp_params.get("views", 1))
    cuts = views(n, root.N)
    total, weight = None, None
    for i, (a, b) in enumerate(cuts):
        x, y = data[a:b], target[a:b]
        loss = one_pass(engine, optimizer, x, y, soft=soft, phase=phase_of(i, len(cuts)), logical_batch=records)
        if len(cuts) == 1:
            return loss
        # (a masked pass's loss is the mean over ITS valid rows, 0 when it has none)
        w = (y >= 0).sum().to(torch.float32) if masked else float(b - a)
        total = loss * w if total is None else total + loss * w
        weight = w if weight is None else weight + w
    if masked:
        return (total / weight.clamp(min=1.0)).reshape(loss.shape)
    return (total / weight).reshape(loss.shape)
