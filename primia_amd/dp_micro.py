"""A DP-SGD step on a logical batch larger than the engine: `train.py --dp_micro_batches K`.

The step is linear in the per-sample terms, and samples are independent under GroupNorm and under frozen BatchNorm
statistics, so the clipped sum splits exactly:

    sum_n clip_n g_n  =  sum over micro-batches k of ( sum over the samples of micro-batch k of clip_n g_n )

The logical batch runs as passes of (forward, per-sample clip, clipped sum) on an engine of M = root.N slots; every pass
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


def step(engine, optimizer, data, target, hip_graph=False):
    """One logical DP-SGD step of `engine` (the loop's model) on (data, target): contiguous views of root.N rows — a
    shorter final view runs on sibling() — each through forward and loss_backward under its phase, then optimizer.step()
    once.  `hip_graph`: every full-size pass goes through graphed_step (one graph per phase; the last phase's graph holds
    the optimizer step).  Returns a device scalar, the mean of the pass losses weighted by their valid rows; nothing
    here waits for the device."""
    root = engine._root
    if root.dp_params is None:
        raise _lib.PrimiaError("dp_micro.step: the engine has no dp_params (micro-batches are a DP-SGD feature: plain "
                               "gradient accumulation would change BatchNorm's statistics)")
    masked = root.dp_params.get("expected_batch") is not None
    n = int(data.shape[0])
    cuts = views(n, root.N)
    if hip_graph:
        from .graphed_train import graphed_step
    total, weight = None, None
    try:
        root.dp_logical_batch = n
        for i, (a, b) in enumerate(cuts):
            root.dp_phase = phase = phase_of(i, len(cuts))
            x, y = data[a:b], target[a:b]
            if hip_graph:
                loss = graphed_step(engine, optimizer, x, y)
            else:
                eng = root.sibling(b - a)
                optimizer.zero_grad()
                eng.forward(x)
                loss = eng.loss_backward(y)
                if phase in (None, "last"):
                    optimizer.step() if eng is optimizer.engine else optimizer.step(eng)
            if len(cuts) == 1:
                return loss
            # (a masked pass's loss is the mean over ITS valid rows, 0 when it has none)
            w = (y >= 0).sum().to(torch.float32) if masked else float(b - a)
            total = loss * w if total is None else total + loss * w
            weight = w if weight is None else weight + w
    finally:
        root.dp_phase = None
        root.dp_logical_batch = None
    if masked:
        return (total / weight.clamp(min=1.0)).reshape(loss.shape)
    return (total / weight).reshape(loss.shape)
