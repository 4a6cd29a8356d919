"""The training step of the host loops (torchlib_compat.train, torchlib_compat.secure_aggregation_epoch,
fed.federated_epoch): `train_step` is their one entry, `eager_step` the step as it runs without --hip_graph.

A DP-SGD step cut into micro-batch passes (primia_amd.dp_micro) runs eager_step — or graphed_step — once per pass, with
the pass's phase and the logical batch size as ARGUMENTS: nothing about a step is kept on the engine between calls.
"""


def eager_step(engine, optimizer, data, target, soft=False, phase=None, logical_batch=None):
    """zero_grad, forward, loss_backward and the optimizer step of `engine` on (data, target).  `engine` is the loop's
    model, the root engine `optimizer` was built on: "the engine itself ran the batch" is what chooses optimizer.step()
    over optimizer.step(sibling).  Another batch size than the engine's (a loader's ragged last batch, MixUp's half batch) runs on engine.sibling(n): the same
    parameters and optimizer state.  `phase` (dp_micro.phase_of) and `logical_batch`: a pass of a DP-SGD step cut into
    micro-batches; "first" and "more" accumulate and take no optimizer step.  Returns the device loss scalar."""
    n = int(data.shape[0])
    eng = engine if n == getattr(engine, "N", n) or not hasattr(engine, "sibling") else engine.sibling(n)
    optimizer.zero_grad()
    eng.forward(data)
    if phase is None:
        loss = eng.loss_backward(target, soft=soft)
    else:
        loss = eng.loss_backward(target, soft=soft, phase=phase, logical_batch=logical_batch)
    if phase in (None, "last"):
        optimizer.step() if eng is engine else optimizer.step(eng)
    return loss


def train_step(engine, optimizer, data, target, soft=False, hip_graph=False):
    """One step of a host loop: a DP engine of dp_micro_batches > 1 takes the loader's batch as ONE logical step run as
    passes of its size (dp_micro.step); otherwise --hip_graph replays the step as a graph where it can (graphed_step);
    otherwise eager_step.  Returns the device loss scalar, which the next step overwrites: keep `.item()` or `.clone()`."""
    if getattr(engine, "dp_micro_batches", 1) > 1:
        from . import dp_micro

        return dp_micro.step(engine, optimizer, data, target, hip_graph=hip_graph, soft=soft)
    if hip_graph:
        from .graphed_train import graphed_step

        return graphed_step(engine, optimizer, data, target, soft=soft)
    return eager_step(engine, optimizer, data, target, soft=soft)
