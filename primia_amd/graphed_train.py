"""One training step of the host loops (forward + loss + backward + optimizer.step(), torchlib/utils.py:1016-1030 /
:1236-1292) replayed as a captured hipGraph: `train.py --hip_graph`.

The eager step launches ~130 kernels from Python; replaying the captured step removes that launch cost (bench.py measures
the same capture on its fixed inputs).  What a training loop needs beyond bench.py's capture:

  * the scheduler's learning rate and Adam's bias corrections change between steps: the graph launches the optimizer's
    device-scalar entry points (primia_*_dev) and primia_opt_hyper_set writes the scalars before every replay, on the
    replay's stream (no host-to-device copy, no synchronisation);
  * the batch is copied into the graph's static input buffers (skipped when the caller already wrote them);
  * Adam's moments belong to the graphs of the root engine: the optimizer objects the loops re-create at every FedAvg
    sync (engine.reset_optimizer), `keep_optim_dict` and checkpoint loads all leave `engine.opt_state` pointing at
    other tensors (or None); before a replay the graph's pair takes their values (zeros for None) and is bound again;
  * the host counters a replay does not advance (num_batches_tracked, opt_steps) are advanced by what one captured
    step advanced them by, so eager and graphed steps mix freely on one model;
  * a replay must never read memory the allocator has freed: the data pointers of every buffer the step touches are
    compared with those seen at capture, and a mismatch captures again.

Graphs live on the engine they replay (the root engine or a `sibling()`, so that sibling eviction drops them with their
buffers), keyed by batch size, soft targets, optimizer kind, fuse_sgd_tail and class-weight presence.  Only the root's
batch size and MixUp's half batch are captured; other sizes (a loader's ragged last batch) run eagerly, and so does DP-SGD
unless its noise comes from a device stream (engine.dp_noise, primia_amd.dp_noise.DeviceNoise: the noise node reads the
stream's device counter and the next node advances it, so every replay draws fresh noise).  Poisson-sampled DP batches
(dp_sampling.PoissonLoader) always have the engine's size — padded slots carry target -1 — so ONE graph, keyed
"Poisson-sampled", serves every step whatever the number of records selected.  The
first step of a key runs eagerly (real training that also allocates the engine's lazy buffers), the second is captured
and replayed.

A DP-SGD step cut into micro-batch passes (primia_amd.dp_micro hands graphed_step each pass's `phase` and the
`logical_batch`, which go on to _key, _StepGraph and loss_backward as arguments) is captured per PHASE: the key gains
("micro-batch", phase, 1 / batch), the "first" and "more" graphs end with the clipped sum going into the root's
accumulator and hold no optimizer step (they advance no step count), the "last" graph holds the noise node and the
optimizer step.  Two graphs per engine for two passes, three for more.  A ragged final pass runs eagerly under the size
rule above, between replayed ones: the accumulator is a plain buffer.

An adaptive clipping norm (engine.dp_clip, primia_amd.dp_clip.AdaptiveClip) adds its parameters — rate, quantile, the
count's noise, the range and z_delta — to the key, never the value of C: the clip-factor, noise and update nodes read and
write C, the counts and the released fraction in device tensors that exist before the capture.

Class weights (engine.class_weight; under DP-SGD the per-sample weighted loss of primia_xent_dp_weighted) enter the key by
their presence only: the loss node reads the weights from device memory, so new values written INTO the same tensor take
effect at the next replay without a new capture, and the tensor's pointer is among those _fingerprint compares — another
tensor captures again.
"""
import gc
import warnings

import torch

from . import _lib
from ._lib import call, query
from .step import eager_step

_dp_warned = False


def eager_reason(engine, optimizer, batch_size):
    """Why a step of `batch_size` samples on `engine` runs eagerly under graphed_step, or None when it is graphed."""
    root = getattr(engine, "_root", engine)
    if getattr(root, "dp_params", None) is not None and getattr(root, "dp_noise", None) is None:
        # torch.randn's generator state is host-side; a DeviceNoise (engine.dp_noise) keeps its counter on the device
        return "DP-SGD runs eagerly: its noise draws have not been shown bit-identical between eager and graphed steps"
    if getattr(optimizer, "kind", None) not in ("SGD", "Adam"):
        return "not an EngineOptimizer"
    if batch_size not in (root.N, root.N // 2):
        return f"batch size {batch_size} is neither the engine's ({root.N}) nor its half (MixUp)"
    if not root.training:
        return "engine in eval mode"
    return None


def _key(eng, optimizer, soft, phase=None, logical_batch=None):
    key = (eng.N, bool(soft), optimizer.kind, bool(eng.fuse_sgd_tail), eng.class_weight is not None)
    if eng.norm == "frozen":        # (a frozen-statistics step launches other kernels than a GroupNorm one)
        key += ("frozen BatchNorm",)
    root = eng._root
    if getattr(root, "dp_params", None) is not None:
        # the DP-SGD parameters are frozen into the graph as kernel arguments, and so is the noise stream's key
        dp = root.dp_params
        key += ("DP with device noise", float(dp.get("max_grad_norm", 1.0)), float(dp.get("noise_multiplier", 1.3)),
                root.dp_noise.key_words + (root.dp_noise.nonce,))
        if dp.get("expected_batch") is not None:
            # padded fixed-capacity batches (dp_sampling.PoissonLoader): other loss and clip kernels, 1 / L in the noise node
            key += ("Poisson-sampled", float(dp["expected_batch"]))
        if int(dp.get("views", 1)) > 1:
            # augmentation multiplicity: the record kernels, 1 / views in the loss gradient's scale
            key += ("records of views", int(dp["views"]))
        if phase is not None:
            # a pass of a step cut into micro-batches: other tail kernels per phase, 1 / batch in the last one's noise node
            inv = 1.0 / float(dp["expected_batch"] if dp.get("expected_batch") is not None else logical_batch)
            key += ("micro-batch", phase, inv)
        clip = getattr(root, "dp_clip", None)
        if clip is not None:
            # an adaptive clipping norm (dp_clip.AdaptiveClip): its PARAMETERS are launch arguments of the update and noise
            # nodes; the value of C is a device word the nodes read, so C moving never captures again
            key += ("adaptive clip",) + clip.key(float(dp.get("noise_multiplier", 1.3)), _divisor(eng, dp, phase, logical_batch))
    return key


def _divisor(eng, dp, phase=None, logical_batch=None):
    """B, what a DP-SGD step of `eng` divides its noised sum by (dp_loss_backward's rule)."""
    if dp.get("expected_batch") is not None:
        return float(dp["expected_batch"])
    if phase is not None:
        return int(logical_batch)
    return eng.N // int(dp.get("views", 1))       # (records under augmentation multiplicity)


def _sync_moments(root):
    """Bind the graphs' Adam moments to the optimizer state the host currently holds (see the module docstring)."""
    own, st = getattr(root, "_graph_moments", None), root._opt_state
    if own is None:
        if st is None:
            st = (torch.zeros_like(root._grads), torch.zeros_like(root._grads))
            root._opt_steps = 0
        root._graph_moments = root._opt_state = st
        return
    if st is None:          # a fresh optimizer (reset_optimizer): adam_step would start from zeros and step 0
        own[0].zero_()
        own[1].zero_()
        root._opt_steps = 0
    elif st[0] is not own[0] or st[1] is not own[1]:      # load_state_dict / another object's moments
        own[0].copy_(st[0])
        own[1].copy_(st[1])
    root._opt_state = own


def _fingerprint(eng, g):
    """Data pointers of every buffer the captured step reads or writes that may be (re)allocated after construction."""
    ts = [eng.flat, eng._grads, eng.dw_acc, eng.wgrad_ws, eng.x0, eng.x0p, eng.pool_argmax, eng.stat_sums, eng.bn_ws,
          eng.feat, eng.dfeat, eng.logits, eng.dlogits, eng.loss, eng.class_weight, eng._stem_sums,
          g.x, g.target, g.hyper]
    ts += list(eng.t.values()) + list(eng.relu_masks.values())
    for sm, si in eng.save.values():
        ts += [sm, si]
    for c in eng.convs.values():
        ts += [c.w_fwd, c.w_dgrad]
    if eng.opt_state is not None:
        ts += list(eng.opt_state)
    if getattr(eng._root, "dp_params", None) is not None:       # (the per-step DP buffers are the graph pool's own)
        ts += [eng._root.dp_noise.counter] + list(eng._dp_keep_buffers().values())
        ts += [eng._root.__dict__.get("_dp_acc")]         # (None unless a step has run as micro-batch passes)
        if getattr(eng._root, "dp_clip", None) is not None:         # C, the counts and the released fraction
            ts += eng._root.dp_clip.tensors()
    return tuple(t.data_ptr() if t is not None else 0 for t in ts) + (len(eng.relu_masks),)


class _StepGraph:
    """One captured training step of one engine and key."""

    def __init__(self, eng, optimizer, soft, data, target, phase=None, logical_batch=None):
        root = eng._root
        self.kind, self.soft = optimizer.kind, bool(soft)      # (no reference to the engine: it owns this object)
        self.x = torch.empty_like(data, memory_format=torch.contiguous_format)
        self.target = torch.empty_like(target, memory_format=torch.contiguous_format)
        self.hyper = torch.zeros(8, dtype=torch.float32, device=eng.device)
        if self.kind == "Adam":
            _sync_moments(root)
        if getattr(root, "dp_noise", None) is not None:
            root.dp_noise.counter       # exists BEFORE the capture: allocated inside, every replay would zero it again
        step_kw = {}
        if phase is not None:
            step_kw = {"phase": phase, "logical_batch": logical_batch}
            eng.dp_acc                  # likewise: the passes of a step hand their sums on through it
        clip = getattr(root, "dp_clip", None)
        if clip is not None:
            clip.tensors()              # likewise: C lives across replays
        # capture runs the step's Python (forward / optimizer.step advance the host counters) without executing a kernel:
        # keep what one step advances them by, and put them back
        nbt = dict(eng.num_batches_tracked)
        steps = root._opt_steps
        updates = clip.updates if clip is not None else 0
        self.graph = torch.cuda.CUDAGraph()
        # No garbage collection inside the capture: a collected engine (every engine is a reference cycle through
        # `_root`) would destroy its own graphs and release their memory pools in the middle of this capture, which the
        # runtime refuses by aborting the process.  Dead engines go now, outside it.
        gc.collect()
        gc_on = gc.isenabled()
        gc.disable()
        try:
            # thread_local: another thread of the process (a process group's watchdog) may touch the runtime meanwhile
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                eng.forward(self.x)
                eng.loss_backward(self.target, soft=self.soft, **step_kw)
                if phase in (None, "last"):
                    optimizer.step(eng, hyper=self.hyper)
        finally:
            if gc_on:
                gc.enable()
        self.nbt_delta = {k: v - nbt[k] for k, v in eng.num_batches_tracked.items() if v != nbt[k]}
        self.steps_delta = root._opt_steps - steps
        eng.num_batches_tracked.update(nbt)
        root._opt_steps = steps
        self.clip_updates_delta = 0
        if clip is not None:
            self.clip_updates_delta, clip.updates = clip.updates - updates, updates
        self.fingerprint = _fingerprint(eng, self)
        self.captures = 1

    def replay(self, eng, optimizer, data, target):
        root = eng._root
        for src, dst in ((data, self.x), (target, self.target)):
            if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
                raise ValueError(f"graphed step captured for {dst.dtype} {tuple(dst.shape)}, got {src.dtype} "
                                 f"{tuple(src.shape)}")
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src)
        g = optimizer.param_groups[0]
        if self.kind == "Adam":
            call("primia_opt_hyper_set", self.hyper, float(g["lr"]), float(g["weight_decay"]), float(g["betas"][0]),
                 float(g["betas"][1]), float(g["eps"]), root._opt_steps + 1)
        else:
            call("primia_opt_hyper_set", self.hyper, float(g["lr"]), float(g["weight_decay"]), 0.0, 0.0, 0.0, 0)
        self.graph.replay()
        for k, d in self.nbt_delta.items():
            eng.num_batches_tracked[k] += d
        root._opt_steps += self.steps_delta
        if self.clip_updates_delta:
            root.dp_clip.updates += self.clip_updates_delta
        return eng.loss


def graphed_step(engine, optimizer, data, target, soft=False, phase=None, logical_batch=None):
    """One training step of `engine` (the loop's model: its sibling of data's batch size runs it) with `optimizer`
    (primia_amd.optim.EngineOptimizer), as a replayed hipGraph where it can be (see the module docstring), eagerly
    (step.eager_step) otherwise.  `phase`, `logical_batch`: a pass of a DP-SGD step cut into micro-batches (dp_micro).
    Returns the engine's device loss scalar; the next step overwrites it, so keep a `.clone()`."""
    global _dp_warned
    n = int(data.shape[0])
    reason = eager_reason(engine, optimizer, n)
    if reason is not None:
        if reason.startswith("DP-SGD") and not _dp_warned:
            _dp_warned = True
            warnings.warn("hip_graph: " + reason, RuntimeWarning, stacklevel=2)
        return eager_step(engine, optimizer, data, target, soft, phase, logical_batch)
    eng = engine if n == engine.N else engine.sibling(n)
    key = _key(eng, optimizer, soft, phase, logical_batch)
    graphs = eng.__dict__.setdefault("_step_graphs", {})
    g = graphs.get(key)
    if g is None:
        warm = eng.__dict__.setdefault("_step_graphs_warm", set())
        if key not in warm:
            warm.add(key)
            return eager_step(engine, optimizer, data, target, soft, phase, logical_batch)
    if query("primia_options_epoch") != eng._options_epoch:
        raise _lib.PrimiaError("library options changed (primia_set_option) after this engine sized its buffers: "
                               "set options first, then construct the engine")
    optimizer.zero_grad()
    earlier = 0
    if g is not None:
        if g.kind == "Adam":
            _sync_moments(eng._root)
        if _fingerprint(eng, g) != g.fingerprint:       # a buffer of the step was reallocated: capture again
            earlier = g.captures
            del graphs[key]
            g = None
    if g is None:
        g = graphs[key] = _StepGraph(eng, optimizer, soft, data, target, phase, logical_batch)
        g.captures += earlier
    return g.replay(eng, optimizer, data, target)


def captures(engine):
    """{key: number of captures} of the graphs held by `engine`'s root and its siblings (tests, tools)."""
    root = engine._root
    out = {}
    for e in [root] + list(root.__dict__.get("_siblings", {}).values()):
        for k, g in e.__dict__.get("_step_graphs", {}).items():
            out[k] = g.captures
    return out
