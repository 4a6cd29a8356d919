"""Device-side ResNet-18 training engine: one federated client = one GPU.

Replaces what a PySyft worker executes natively for one plaintext training step
(SURVEY.md §8b "commands one worker receives per step"; reference call site
torchlib/utils.py:1168-1174): forward, loss, backward and the optimizer step, all as HIP kernels
called through the C ABI of libprimia_hip.so.  torch is used for device memory, streams and (in
primia_amd.fed) torch.distributed — never for arithmetic.

Memory layout (all on one GPU):
  flat   fp32 [P + B]   parameters in reference named_parameters() order (OIHW conv weights), then
                        the BatchNorm running_mean/var buffers — exactly the 11,187,651 elements
                        FedAvg exchanges (torchlib/utils.py:1000-1092)
  grads  fp32 [P]       same order as the parameter part of `flat`
  per conv: compute-dtype weight copies in the implicit-GEMM layouts (+ fp32 wgrad accumulator)
  activations / gradients: NHWC tensors in the compute dtype (bf16 for throughput, fp32 for parity)
"""
import os
from collections import OrderedDict

import torch

from . import _lib
from ._lib import ConvDesc, call, query
from .resnet_spec import NetSpec, bn_name, buffer_entries, init_state_dict, param_entries, resnet18_spec, state_dict_keys

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
# Backward entries per norm kind: (relu without residual, 1-bit ReLU mask instead of z, general).  The kinds share one
# argument frame (ResNet18Engine._bn_bwd, the only caller); what each takes for the statistics and where its affine
# gradients go is chosen with the names at construction: the saved (mean, invstd) — frozen BatchNorm: (running_mean,
# running_var, eps) — and the gradient views — GroupNorm and frozen BatchNorm: per-sample rows, and a groups slot.
_NORM_BWD = {"batch": ("primia_bn_relu_bwd", "primia_bn_bwd_mask", "primia_bn_bwd"),
             "group": ("primia_gn_relu_bwd", "primia_gn_bwd_mask", "primia_gn_bwd"),
             "frozen": ("primia_bn_frozen_relu_bwd", "primia_bn_frozen_bwd_mask", "primia_bn_frozen_bwd")}


class _Conv:
    def __init__(self, spec, desc, c_real):
        self.spec, self.desc, self.c_real = spec, desc, c_real
        # How the layer's batched weight gradient is served — decided once by ResNet18Engine.__init__, read by _issue_wgrad:
        # "stem" (conv1 on the padded input), "pair" (half of a transition block's conv1 + downsample launch), "group"
        # (member of a stage's same-shape launch) or "single".  wg_hold, pairs and groups: (key of the hold, launches that
        # fill it, layers of the network that feed it).  wg_x, conv1 only: its operand, the padded input where one exists.
        self.wg, self.wg_hold, self.wg_x = "single", None, None
        # DP-SGD norm pass where the layer's tiles are not kept: (conv1's halo kernel serves it, conv1's operand for it)
        self.dp_norm = (False, None)
        # asked of the library at first use (the switches that gate them can be set after construction)
        self.pair_ok = self.bnsums_slots = self.acc_bnsums_slots = self.pair_bnsums_slots = None


class ResNet18Engine:
    def __init__(self, batch_size, num_classes=3, in_channels=3, input_size=224, pooling="max",
                 dtype=torch.bfloat16, device="cuda:0", norm="batch", groups=32, options=None, share=None):
        """norm="batch": the reference model.  norm="group": GroupNorm(groups, C) in place of every
        BatchNorm (ResNet's `norm_layer` hook, torchlib/models.py:355) — the BN-free network the
        DP-SGD configuration needs (train.py:308).  norm="frozen": the reference model with every BatchNorm applied
        with its running statistics in training too (gamma / beta train, the statistics are never written) — a sample's
        gradient depends on that sample alone, so DP-SGD can fine-tune pretrained BatchNorm weights; state dicts are
        the BatchNorm network's.
        `options`: {name: value} overriding the schedule switches below (class attributes such as fwd_pair,
        wgrad_overlap, wgrad_flush_last, fuse_stem, dp_keep ...) for THIS engine before its buffers are sized.  Nothing here
        reads the environment; the kernel library's own switches are `_lib.set_option` (primia_set_option).
        `share`: another engine of the same network whose PARAMETERS this one uses (see `sibling`)."""
        self._root = self if share is None else share._root
        self._options = dict(options or {})
        for k, v in self._options.items():
            if not hasattr(type(self), k):
                raise ValueError(f"unknown engine option {k!r}")
            setattr(self, k, v)
        if not torch.cuda.is_available():
            raise _lib.PrimiaError("ResNet18Engine needs a GPU (HIP kernels only, no CPU fallback)")
        _lib.lib()
        # every buffer below is sized from the library's *_bytes / *_slots queries, which read the process-wide option
        # table: remember its epoch — forward() refuses to run once it has moved (a later
        # primia_set_option("c64_blocks" | "lh2" | ...) would make kernels write more partials than were allocated)
        self._options_epoch = query("primia_options_epoch")
        self.spec: NetSpec = resnet18_spec(num_classes, in_channels, input_size, pooling)
        if norm not in ("batch", "group", "frozen"):
            raise ValueError("norm must be 'batch', 'group' or 'frozen'")
        self.norm, self.groups = norm, int(groups)
        # the two questions the step methods ask of the kind.  batch_stats: BatchNorm proper — statistics of the batch in
        # training (running ones in eval mode), the kernels that fuse across layers.  per_sample_norm: GroupNorm and frozen
        # BatchNorm — a sample's output depends on that sample alone, the same pass in training and eval mode, affine
        # gradients per sample (what DP-SGD needs).
        self.batch_stats = norm == "batch"
        self.per_sample_norm = not self.batch_stats
        # (of the per-sample kinds GroupNorm alone has the stem tail norm -> relu -> maxpool as one kernel each way)
        self._gn_stem_kernels = norm == "group"
        self.N = int(batch_size)
        self.dtype = dtype
        self.dt = _lib.dtype_code(dtype)
        self.device = torch.device(device)
        self.training = True
        dev = self.device

        # ---- flat arenas ---------------------------------------------------------------------
        self.p_entries = param_entries(self.spec)
        self.b_entries = buffer_entries(self.spec, norm)
        self.P = sum(int(torch.Size(s).numel()) for _, s in self.p_entries)
        self.B = sum(int(torch.Size(s).numel()) for _, s in self.b_entries)
        if share is None:
            self.flat = torch.zeros(self.P + self.B, dtype=torch.float32, device=dev)
            self._grads = torch.zeros(self.P, dtype=torch.float32, device=dev)   # (read through the `grads` property)
        else:       # the same arenas: a step of either engine moves the one set of weights
            if (share.spec.num_classes, share.spec.in_channels, share.spec.input_size, share.spec.pooling, share.norm,
                    share.dtype) != (num_classes, in_channels, input_size, pooling, norm, dtype):
                raise ValueError("a sibling engine must be the same network, norm and dtype as the engine it shares with")
            self.flat, self._grads = share.flat, share._grads
        self.views, self._gviews = {}, {}
        off = 0
        for k, s in self.p_entries:
            n = int(torch.Size(s).numel())
            self.views[k] = self.flat[off:off + n].view(s)
            self._gviews[k] = self._grads[off:off + n].view(s)
            off += n
        for k, s in self.b_entries:
            n = int(torch.Size(s).numel())
            self.views[k] = self.flat[off:off + n].view(s)
            off += n
        # BatchNorm's num_batches_tracked (only ever READ by torch when momentum is None, never by this network): a host
        # counter advanced by forward(); a captured hipGraph replays kernels, not Python, so a caller that replays steps
        # (bench.py) and then exports state_dict() must add its replay count itself (note_replayed_steps).
        self.num_batches_tracked = ({bn_name(c.name): 0 for c in self.spec.convs} if share is None
                                    else share.num_batches_tracked)
        if share is None:
            self._opt_state = None  # Adam moments, created lazily
            self._opt_steps = 0

        # ---- conv descriptors, weight copies --------------------------------------------------
        N = self.N
        self.convs = {}
        H = input_size
        stem = self.spec.stem
        if in_channels > 4:
            raise _lib.PrimiaError("stem supports in_channels <= 4")
        self.convs[stem.name] = _Conv(stem, ConvDesc.make(N, H, H, 4, 64, 7, 7, 2, 3), in_channels)
        H = self.convs[stem.name].desc.Ho  # 112
        self.stem_hw = H
        H = (H + 2 - 3) // 2 + 1           # 56 after the 3x3/2 pool
        self.pool_hw = H
        for blk in self.spec.blocks:
            c1 = blk.conv1
            d1 = ConvDesc.make(N, H, H, c1.cin, c1.cout, 3, 3, c1.stride, 1)
            self.convs[c1.name] = _Conv(c1, d1, c1.cin)
            if blk.down is not None:
                dd = ConvDesc.make(N, H, H, blk.down.cin, blk.down.cout, 1, 1, blk.down.stride, 0)
                self.convs[blk.down.name] = _Conv(blk.down, dd, blk.down.cin)
            H = d1.Ho
            c2 = blk.conv2
            self.convs[c2.name] = _Conv(c2, ConvDesc.make(N, H, H, c2.cin, c2.cout, 3, 3, 1, 1), c2.cin)
        self.final_hw = H
        if self.final_hw != input_size // 32:
            raise _lib.PrimiaError("input_size must be a multiple of 32")

        # fp32 weight-gradient accumulators (forward layout), one arena.  The layers served by the atomic-free
        # path (primia_conv2d_wgrad_ws OVERWRITES its accumulator) sit behind the ones that accumulate with
        # atomics, so that only the front part needs zeroing every step.
        acc_total = 0
        ws_need = {c.spec.name: query("primia_conv_wgrad_ws_bytes", c.desc, self.dt) for c in self.convs.values()}
        stem_ws = query("primia_stem_conv_wgrad_ws_bytes", N, input_size, input_size)
        for overwriting in (False, True):
            for c in self.convs.values():
                # (conv1's 64 KiB slab stays in the zeroed part: odd input sizes take its accumulate path)
                if (ws_need[c.spec.name] > 0 and c.spec.name != "conv1") != overwriting:
                    continue
                c.wfwd_n = query("primia_conv_wfwd_elems", c.desc)
                c.acc_off = acc_total
                acc_total += (c.wfwd_n + 3) // 4 * 4
            if not overwriting:
                self._acc_zero_n = acc_total
                # ... and nothing but conv1's slab may be in it: the padded-input stem kernels overwrite that one too
                self._acc_zero_only_stem = all(ws_need[c.spec.name] > 0 for c in self.convs.values() if c.spec.name != "conv1")
        self.dw_acc = torch.zeros(acc_total, dtype=torch.float32, device=dev)
        for c in self.convs.values():
            if share is not None:       # kernel-layout weight copies do not depend on the batch size: one set
                c.w_fwd, c.w_dgrad = share.convs[c.spec.name].w_fwd, share.convs[c.spec.name].w_dgrad
                c.acc = self.dw_acc[c.acc_off:c.acc_off + c.wfwd_n]
                continue
            c.w_fwd = torch.empty(c.wfwd_n, dtype=dtype, device=dev)
            c.w_dgrad = None
            if c.spec.name != stem.name:
                c.w_dgrad = torch.empty(query("primia_conv_wdgrad_elems", c.desc), dtype=dtype, device=dev)
            c.acc = self.dw_acc[c.acc_off:c.acc_off + c.wfwd_n]
        # ---- how each conv's batched weight gradient is served: decided here, recorded on the _Conv (wg, wg_hold), read by
        # _issue_wgrad — the plain backward pass and the DP-SGD clipped sums issue through that one method ----
        # a transition block's conv1 + downsample weight gradients as one launch (primia_conv2d_wgrad_pair_ws)
        shared_ws = [0]
        for blk in self.spec.blocks:
            if blk.down is not None:
                c1, cd = self.convs[blk.conv1.name], self.convs[blk.down.name]
                shared_ws.append(query("primia_conv_wgrad_pair_ws_bytes", c1.desc, cd.desc, self.dt))
                if shared_ws[-1] > 0:
                    c1.wg = cd.wg = "pair"
                    c1.wg_hold = cd.wg_hold = (blk.prefix, 2, 2)
        # several layers of one shape in ONE weight-gradient launch (primia_conv2d_wgrad_group_ws): the 3x3 / stride-1
        # layers of a stage share a shape; a layer's (x, dy) is held back until its siblings' are ready
        if dtype == torch.bfloat16:
            shapes = {}
            for c in self.spec.convs:
                d = self.convs[c.name].desc
                if d.R == 3 and d.stride == 1 and c.name != stem.name:
                    shapes.setdefault((d.H, d.W, d.C, d.K), []).append(c.name)
            for key, names in shapes.items():
                d = self.convs[names[0]].desc
                n = query("primia_conv_wgrad_group_size", d, len(names), self.dt)
                if n >= 2:
                    for nm in names:
                        self.convs[nm].wg, self.convs[nm].wg_hold = "group", (key, n, len(names))
                    shared_ws.append(query("primia_conv_wgrad_group_ws_bytes", d, n, self.dt))
        self._wg_held = {}         # hold key -> [(name, x, dy), ...] waiting for the launch they share
        self._wg_seen = {}         # hold key -> layers feeding it that this pass has reached
        # workspace of the atomic-free weight-gradient path (primia_conv2d_wgrad_ws): the layers run one after
        # the other on one stream, so they share one buffer sized for the largest (38 MB at batch 256)
        ws_bytes = max(max(ws_need.values()), stem_ws, max(shared_ws))
        if ws_bytes <= 0:   # (conv1's generic kernel alone asks for one at every shape the checks above let through)
            raise _lib.PrimiaError("no weight-gradient workspace: primia_conv_wgrad_ws_bytes answered nothing positive")
        self.wgrad_ws = torch.empty(max(ws_bytes, 16) // 4, dtype=torch.float32, device=dev)
        self.wgrad_ws_bytes = ws_bytes
        self._wg_stream, self._wg_pending = None, False      # second stream of wgrad_overlap, created at first use

        # ---- activations ------------------------------------------------------------------------
        def act(hw, ch):
            return torch.empty(N * hw * hw, ch, dtype=dtype, device=dev)

        self.x0 = torch.empty(N * input_size * input_size, 4, dtype=dtype, device=dev)
        # bf16: the stem also keeps a spatially padded copy of the input for primia_stem_conv_fwd (3 zero rows
        # above / below, 3 zero columns left, 5 right; zeroed once, only the interior is rewritten)
        self.x0p = None
        if dtype == torch.bfloat16 and input_size % 32 == 0:
            self.x0p_dims = (input_size + 6, input_size + 8)
            self.x0p = torch.zeros(N * self.x0p_dims[0] * self.x0p_dims[1], 4, dtype=dtype, device=dev)
        self.t = {}  # named tensors
        t = self.t
        t["stem.y"] = act(self.stem_hw, 64)
        t["stem.z"] = act(self.stem_hw, 64)
        t["stem.dz"] = act(self.stem_hw, 64)
        t["stem.dy"] = act(self.stem_hw, 64)
        t["pool.out"] = act(self.pool_hw, 64)
        self.pool_argmax = torch.empty(N * self.pool_hw * self.pool_hw * 64, dtype=torch.uint8, device=dev)
        for blk in self.spec.blocks:
            p = blk.prefix
            d1 = self.convs[blk.conv1.name].desc
            hw, ch = d1.Ho, blk.conv1.cout
            for nm in ("y1", "a1", "y2", "out", "dy1", "da1", "dy2"):
                t[f"{p}.{nm}"] = act(hw, ch)
            if blk.down is not None:
                for nm in ("yd", "idn", "dyd"):
                    t[f"{p}.{nm}"] = act(hw, ch)
        # Gradient w.r.t. each block's output.  An identity block accumulates its input gradient in
        # place (masked residual gradient + conv1 dgrad), so its input-gradient buffer IS its own
        # `dout`; a projection block gets a fresh buffer of the input's shape.
        blocks = self.spec.blocks
        for i in range(len(blocks) - 1, -1, -1):
            blk = blocks[i]
            d1 = self.convs[blk.conv1.name].desc
            key = blk.prefix + ".dout"
            if key not in t:
                t[key] = act(d1.Ho, blk.conv1.cout)
            din = t[key] if blk.down is None else act(d1.H, blk.conv1.cin)
            t[(blocks[i - 1].prefix + ".dout") if i > 0 else "pool.dout"] = din
        # stem tail bn1 -> relu -> maxpool as ONE fused op in training (z = relu(bn(y)) is never written)
        self.fuse_stem = True
        self.relu_masks = {}         # residual layers: 1-bit ReLU masks for the backward passes (see _bn)
        # the stem convolutions read the padded input copy where there is one — conv1's weight gradient too — and DP-SGD's
        # norm pass does where the halo kernel serves the shape (exactly where it asks for a workspace); the unpadded copy
        # is written only where something reads it
        c = self.convs[stem.name]
        halo = self.x0p is not None and stem_ws > 0
        if self.x0p is not None:
            c.wg, c.wg_x = "stem", self.x0p
        else:
            c.wg_x = self.x0
        c.dp_norm = (halo, self.x0p if halo else self.x0)
        self._x0_valid = self.x0p is None or (self.per_sample_norm and not halo)
        self.stat_slots = query("primia_conv_stat_slots")
        for c in self.spec.convs:   # slots the kernel serving this conv writes (per-block partials for layer1's)
            self.convs[c.name].stat_slots = (query("primia_conv_stat_slots_for", self.convs[c.name].desc, self.dt)
                                             if c.name != "conv1" else self.stat_slots)
        per = lambda c: self.convs[c.name].stat_slots * 2 * c.cout
        self.stat_sums = torch.zeros(sum(per(c) for c in self.spec.convs), dtype=torch.float32, device=dev)
        off = 0
        for c in self.spec.convs:
            self.convs[c.name].sums = self.stat_sums[off:off + per(c)]
            off += per(c)
        # Layers whose conv kernel emits the BatchNorm partial sums for free (deterministic per-block partials out
        # of the write-back phase): the statistics pass over their output is dropped.
        self.free_stats = {c.name for c in self.spec.convs
                           if dtype == torch.bfloat16 and norm == "batch" and c.name != "conv1"
                           and query("primia_conv_stats_per_tile", self.convs[c.name].desc, self.dt) == 1}
        # (Two experiments lived here and were measured to lose, profiles/r01_negative_results.txt: atomically accumulated
        # batch sums for the late stages, and BatchNorm-backward sums emitted by the data-gradient kernels' write-backs —
        # 6.375 -> 6.449 ms per step.)
        # identity blocks: can conv1's accumulating data gradient apply bn2's ReLU mask to the old values itself?
        self.masked_acc_ok = {blk.conv1.name: query("primia_conv_dgrad_masked_acc_ok", self.convs[blk.conv1.name].desc,
                                                    self.dt) == 1
                              for blk in self.spec.blocks if blk.down is None}
        # ---- norm layers: what the kind keeps per layer; the step methods read these, none of them asks for the kind ----
        def f32_pair(*shape):
            return tuple(torch.empty(*shape, dtype=torch.float32, device=dev) for _ in range(2))

        bns = [(bn_name(c.name), c) for c in self.spec.convs]
        # saved (mean, invstd): per channel, GroupNorm's per (sample, group)
        self.save = {b: f32_pair(N * self.groups if norm == "group" else c.cout) for b, c in bns}
        norm_ws = [query("primia_bn_workspace_bytes", 1, 512), 1024 * 3 * 512 * 4]   # (pair backward: 3 sums)
        if norm == "group":
            norm_ws.append(query("primia_gn_workspace_bytes", N, 512, self.groups))
        if norm == "frozen":
            norm_ws += [query("primia_bn_frozen_workspace_bytes", N, self.convs[c.name].desc.Ho ** 2, c.cout) for b, c in bns]
        self.bn_ws_bytes = max(norm_ws)
        self.bn_ws = torch.zeros(self.bn_ws_bytes, dtype=torch.uint8, device=dev)  # holds a completion counter
        # _bn_bwd's entries and, per layer, their operands for the statistics and for dgamma / dbeta
        self._bwd_entries = _NORM_BWD[norm]
        self._bwd_stats = {b: (self.views[b + ".running_mean"], self.views[b + ".running_var"], BN_EPS) if norm == "frozen"
                           else self.save[b] for b, c in bns}
        if self.per_sample_norm:
            # per-sample affine gradients [N][C] per layer, summed over the samples by _reduce_affine
            self.ps_affine = {b: f32_pair(N, c.cout) for b, c in bns}
            self.ones_n = torch.ones(N, dtype=torch.float32, device=dev)
            self._bwd_affine = self.ps_affine
            self._ps_groups = (self.groups,) if norm == "group" else ()
        else:
            self._bwd_affine = {b: (self._gviews[b + ".weight"], self._gviews[b + ".bias"]) for b, c in bns}
        # state of the stem's fusions: decided by every forward(), read by backward()
        self._stem_fused = self._stem_fused_gn = False
        self._stem_sums, self._stem_slots = None, 0   # bn1's partial sums out of the padded-input stem conv (first use)
        self._pool_sums = None       # (partials, slots) of bn1's backward sums where layer1.0.conv1's data gradient forms them
        self._stem_bwd_fused_ok = None      # the library's gate for primia_stem_bwd_fused at this shape, asked at first use
        self._bwd_sum_bufs = {}      # partial tables of the *_bnsums fusions, by producer (see _bwd_sums)
        # DP-SGD: built at first use — the kept-tile buffers, the argument arrays of the *_many launches
        self._dp_keep = self._sqnorm_many = self._colsum_many = self._scale_many = None
        self.dp = None  # set by dp_backward: {"wgrads": [...]} defers the weight gradients
        self.feat = torch.empty(N, 512, dtype=torch.float32, device=dev)
        self.dfeat = torch.empty(N, 512, dtype=torch.float32, device=dev)
        self.logits = torch.empty(N, num_classes, dtype=torch.float32, device=dev)
        self.dlogits = torch.empty(N, num_classes, dtype=torch.float32, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.class_weight = None  # optional fp32 [classes] device tensor (CrossEntropyLoss weight)

    # ------------------------------------------------------------------------------------------
    # state
    # ------------------------------------------------------------------------------------------
    def init_weights(self):
        """Draw fresh weights from the global torch RNG the way the reference constructor does."""
        self.load_state_dict(init_state_dict(self.spec, self.norm))

    def state_dict(self):
        """Reference-compatible state dict (CPU tensors, OIHW, 122 keys incl. num_batches_tracked)."""
        host = self.flat.detach().cpu()
        sd = OrderedDict()
        off = {}
        o = 0
        for k, s in self.p_entries + self.b_entries:
            n = int(torch.Size(s).numel())
            off[k] = (o, n, s)
            o += n
        for k in state_dict_keys(self.spec, self.norm):
            if k.endswith("num_batches_tracked"):
                sd[k] = torch.tensor(self.num_batches_tracked[k.rsplit(".", 1)[0]], dtype=torch.long)
            else:
                o, n, s = off[k]
                sd[k] = host[o:o + n].view(s).clone()
        return sd

    def load_state_dict(self, sd):
        keys = state_dict_keys(self.spec, self.norm)
        missing = [k for k in keys if k not in sd]
        extra = [k for k in sd if k not in keys]
        if missing or extra:
            raise KeyError(f"state_dict mismatch: missing {missing[:3]} unexpected {extra[:3]}")
        for k in keys:
            if k.endswith("num_batches_tracked"):
                self.num_batches_tracked[k.rsplit(".", 1)[0]] = int(sd[k])
                continue
            v = sd[k]
            if tuple(v.shape) != tuple(self.views[k].shape):
                raise ValueError(f"shape mismatch for {k}: {tuple(v.shape)} vs {tuple(self.views[k].shape)}")
            self.views[k].copy_(v.to(torch.float32))
        self.refresh_weights()

    def _many_args(self):
        """Host-side argument arrays of the batched weight-refresh / wgrad-finalize calls (built once)."""
        if getattr(self, "_many", None) is None:
            import ctypes

            cs = list(self.convs.values())
            n = len(cs)
            vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
            self._many = dict(
                n=n, descs=(ConvDesc * n)(*[c.desc for c in cs]), creal=(ctypes.c_int * n)(*[c.c_real for c in cs]),
                w=(ctypes.c_void_p * n)(*[vp(self.views[c.spec.name + ".weight"]) for c in cs]),
                wf=(ctypes.c_void_p * n)(*[vp(c.w_fwd) for c in cs]),
                wd=(ctypes.c_void_p * n)(*[vp(c.w_dgrad) for c in cs]),
                acc=(ctypes.c_void_p * n)(*[vp(c.acc) for c in cs]),
                gw=(ctypes.c_void_p * n)(*[vp(self._gviews[c.spec.name + ".weight"]) for c in cs]))
        return self._many

    # Adam's moments and step count belong to the PARAMETERS: siblings read and write the root engine's
    @property
    def opt_state(self):
        return self._root._opt_state

    @opt_state.setter
    def opt_state(self, v):
        self._root._opt_state = v

    @property
    def opt_steps(self):
        return self._root._opt_steps

    @opt_steps.setter
    def opt_steps(self, v):
        self._root._opt_steps = v

    @property
    def gviews(self):
        """{name: view of the gradient arena}.  Reading it finishes a deferred conv-gradient pass first (fuse_sgd_tail leaves
        the conv gradients in their accumulators between loss_backward() and step()), like `grads`."""
        self.materialize_grads()
        return self._gviews

    max_siblings = 6      # batch sizes kept besides the root's (each owns its activations and workspaces)

    def sibling(self, batch_size):
        """An engine for ANOTHER batch size on the SAME parameters, gradients, running statistics, kernel-layout weight
        copies and optimizer state (activations and workspaces are its own): forward / loss_backward / sgd_step /
        adam_step on either one train the one model.  The reference's local training loop needs it — MixUp halves a batch
        with probability mixup_prob (torchlib/utils.py:1262-1267, :336-347), so consecutive steps see B or B / 2 samples."""
        n = int(batch_size)
        if n == self.N:
            return self
        if n == self._root.N:         # (asked of a sibling: the root itself, not a second full-size engine)
            self._root.train(self.training)
            return self._root
        sib = self._root.__dict__.setdefault("_siblings", {})
        if n in sib:
            sib[n] = sib.pop(n)       # (a hit moves the entry to the back of the dict: the front is the least recently USED)
        elif len(sib) >= self.max_siblings:
            # activations and workspaces of an engine are ~12 MB per image: keep the most recently used few batch sizes only
            # (MixUp halves, the ragged final batch of train / validation loaders); the freed blocks stay in torch's
            # caching allocator for the engine that replaces them
            del sib[next(iter(sib))]
        if n not in sib:
            sib[n] = ResNet18Engine(n, self.spec.num_classes, self.spec.in_channels, self.spec.input_size,
                                    self.spec.pooling, dtype=self.dtype, device=self.device, norm=self.norm,
                                    groups=self.groups, options=self._root._options, share=self._root)
        # what the host sets on the root after construction travels with every call: the optimizer's fused tail and —
        # above all — the DP-SGD parameters (a halved or ragged batch must be clipped and noised like every other)
        for attr in ("fuse_sgd_tail", "dp_params", "dp_noise", "dp_clip", "dp_micro_batches", "class_weight"):
            setattr(sib[n], attr, getattr(self._root, attr))
        sib[n].train(self.training)
        return sib[n]

    def refresh_weights(self):
        """fp32 master (OIHW) -> compute-dtype implicit-GEMM copies; call after any change of `flat`."""
        m = self._many_args()
        call("primia_conv_weight_prepare_many", m["descs"], m["creal"], m["w"], m["wf"], m["wd"], m["n"], self.dt)

    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    # ------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------
    def _relu_mask(self, b, y):
        """Norm layer b's 1-bit ReLU mask, sized from its input y.  Allocated at first use: an engine that only evaluates
        holds none."""
        mask = self.relu_masks.get(b)
        if mask is None:
            mask = self.relu_masks[b] = torch.empty(y.numel() * y.element_size() // 16, dtype=torch.uint8, device=y.device)
        return mask

    def _bn(self, conv_name, y, z, residual, relu):
        b = bn_name(conv_name)
        C = y.shape[1]
        M = y.shape[0]
        g, be = self.views[b + ".weight"], self.views[b + ".bias"]
        # residual layer in training: also write the 1-bit ReLU mask the backward passes read instead of z
        mask = None
        if self.training and residual is not None and relu and (self.batch_stats or self.gn_relu_masks):
            mask = self._relu_mask(b, y)
        sm, si = self.save[b]
        if self.norm == "group":  # identical in train and eval mode: no running statistics
            if mask is not None:
                call("primia_gn_fwd_mask", y, residual, z, mask, g, be, sm, si, self.N, M // self.N, C, self.groups, BN_EPS,
                     self.bn_ws, self.bn_ws_bytes, self.dt)
            else:
                call("primia_gn_fwd", y, residual, z, g, be, sm, si, self.N, M // self.N, C, self.groups, BN_EPS, int(relu),
                     self.bn_ws, self.bn_ws_bytes, self.dt)
            return
        rm, rv = self.views[b + ".running_mean"], self.views[b + ".running_var"]
        if not (self.batch_stats and self.training):
            # eval mode — and frozen BatchNorm in either mode: the running statistics are read, never written
            if mask is not None:
                call("primia_bn_fwd_eval_mask", y, residual, z, mask, g, be, rm, rv, M, C, BN_EPS, self.dt)
            else:
                call("primia_bn_fwd_eval", y, residual, z, g, be, rm, rv, M, C, BN_EPS, int(relu), self.dt)
            return
        c = self.convs[conv_name]
        have_sums = conv_name in self.free_stats
        if mask is not None:
            call("primia_bn_fwd_train_mask", y, residual, z, mask, g, be, rm, rv, sm, si, c.sums if have_sums else None,
                 c.stat_slots if have_sums else 0, M, C, BN_EPS, BN_MOMENTUM, self.bn_ws, self.bn_ws_bytes, self.dt)
        elif have_sums:
            call("primia_bn_fwd_train_from_sums", y, residual, z, g, be, rm, rv, sm, si, c.sums, c.stat_slots, M, C, BN_EPS,
                 BN_MOMENTUM, int(relu), self.dt)
        else:
            call("primia_bn_fwd_train", y, residual, z, g, be, rm, rv, sm, si, M, C, BN_EPS, BN_MOMENTUM, int(relu),
                 self.bn_ws, self.bn_ws_bytes, self.dt)
        self.num_batches_tracked[b] += 1

    # Optional per-launch timing of the convolution kernels (bench.py roofline leg): when
    # `self.prof` is a list, every conv launch is bracketed by events on the launch stream.
    prof = None
    # Optional copies of buffers the backward pass consumes IN PLACE (tests): when `self.taps` is a dict, backward() stores
    # "<block>.dout_in" — the gradient w.r.t. the block's output as its bn2 backward pass reads it, before conv1's
    # accumulating data gradient turns the same buffer into the gradient of the block in front.
    taps = None

    @staticmethod
    def _macs(c):
        d = c.desc
        return d.N * d.Ho * d.Wo * d.K * c.c_real * d.R * d.S

    def _timed(self, kind, c, fn, extra_macs=0):
        if self.prof is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        self.prof.append((kind, c.spec.name, 2.0 * (self._macs(c) + extra_macs), e0, e1))

    def _conv_fwd(self, name, x, y):
        c = self.convs[name]
        if self.training and name in self.free_stats:
            self._timed("fwd", c, lambda: call("primia_conv2d_fwd_stats", c.desc, x, c.w_fwd, y, c.sums, self.dt))
        else:
            self._timed("fwd", c, lambda: call("primia_conv2d_fwd", c.desc, x, c.w_fwd, y, self.dt))

    fwd_pair = True
    # eval mode, BatchNorm + max pooling: the stem head as one kernel (primia_stem_conv_pool_eval).  One block per image —
    # from this batch size on it beats the three-kernel chain (178 us for any batch up to 256; the chain: 1.4 us per image)
    stem_eval_one_pass_min_batch = 160

    def _stem_eval_one_pass(self):
        if self.training or not self.batch_stats or self.spec.pooling != "max" or self.prof is not None:
            return False
        if self.N < self.stem_eval_one_pass_min_batch:
            return False
        S = self.spec.input_size
        return query("primia_stem_conv_pool_ok", self.N, S, S, self.dt) == 1

    def _conv_fwd_pair(self, blk, x, y1, yd):
        """conv1 + downsample of a transition block as one launch; False where the library does not serve the pair."""
        c1, cd = self.convs[blk.conv1.name], self.convs[blk.down.name]
        if c1.pair_ok is None:
            c1.pair_ok = self.fwd_pair and query("primia_conv_fwd_pair_ok", c1.desc, cd.desc, self.dt) == 1
        if not c1.pair_ok:
            return False
        stats = self.training and self.batch_stats
        s1 = c1.sums if stats and blk.conv1.name in self.free_stats else None
        sd = cd.sums if stats and blk.down.name in self.free_stats else None
        if stats and (s1 is None or sd is None):
            return False        # (a layer whose statistics come from a separate pass: keep the single launches)
        self._timed("fwd", c1, lambda: call("primia_conv2d_fwd_stats_pair", c1.desc, x, c1.w_fwd, y1, s1, cd.desc, cd.w_fwd,
                                            yd, sd, self.dt), extra_macs=self._macs(cd))
        return True

    def forward(self, x_nchw):
        """x_nchw: fp32 [N, in_channels, S, S] on this GPU.  Returns fp32 logits [N, classes]."""
        N, S, t = self.N, self.spec.input_size, self.t
        if tuple(x_nchw.shape) != (N, self.spec.in_channels, S, S) or x_nchw.dtype != torch.float32:
            raise ValueError(f"expected fp32 input {(N, self.spec.in_channels, S, S)}, got {tuple(x_nchw.shape)}")
        x_nchw = x_nchw.contiguous()
        if query("primia_options_epoch") != self._options_epoch:
            raise _lib.PrimiaError("library options changed (primia_set_option) after this engine sized its buffers: "
                                   "set options first, then construct the engine")
        if self._x0_valid:
            call("primia_nchw_to_nhwc", x_nchw, self.x0, N, self.spec.in_channels, S, S, 4, self.dt)
        stem_done = False
        if self.x0p is not None:
            call("primia_nchw_to_nhwc_padded", x_nchw, self.x0p, N, self.spec.in_channels, S, S, 4, 3, 3,
                 self.x0p_dims[0], self.x0p_dims[1], self.dt)
            c = self.convs["conv1"]
            if self.training and self.batch_stats:   # + bn1's per-block partial sums, for free
                if self._stem_sums is None:
                    self._stem_slots = query("primia_stem_conv_stat_slots", N, S, S)
                    self._stem_sums = torch.zeros(self._stem_slots, 2, 64, dtype=torch.float32, device=self.device)
                self._timed("fwd", c, lambda: call("primia_stem_conv_fwd_stats", self.x0p, c.w_fwd, t["stem.y"],
                                                   self._stem_sums, N, S, S, self.dt))
            elif self._stem_eval_one_pass():
                # eval mode: conv1 -> bn1 -> relu -> maxpool as one pass over the input (neither stem tensor is written)
                call("primia_stem_conv_pool_eval", self.x0p, c.w_fwd, t["pool.out"], self.pool_argmax,
                     self.views["bn1.weight"], self.views["bn1.bias"], self.views["bn1.running_mean"],
                     self.views["bn1.running_var"], BN_EPS, N, S, S, self.dt)
                stem_done = True
            else:
                self._timed("fwd", c, lambda: call("primia_stem_conv_fwd", self.x0p, c.w_fwd, t["stem.y"], N, S, S,
                                                   self.dt))
        else:
            self._conv_fwd("conv1", self.x0, t["stem.y"])
        hw = self.stem_hw
        self._stem_fused = self.fuse_stem and self.training and self.batch_stats and self.spec.pooling == "max"
        # GroupNorm: gn1 -> relu -> maxpool as one op each way (primia_gn_relu_maxpool_fwd / _bwd; _bwd wants even sizes)
        self._stem_fused_gn = (self.fuse_stem and self.gn_stem_fused and self._gn_stem_kernels
                               and self.spec.pooling == "max" and hw % 2 == 0)
        if stem_done:
            pass
        elif self._stem_fused and self.x0p is not None:  # (bn1's sums came with the padded-input stem conv above)
            sm, si = self.save["bn1"]
            call("primia_bn_relu_maxpool_fwd_from_sums", t["stem.y"], t["pool.out"], self.pool_argmax,
                 self.views["bn1.weight"], self.views["bn1.bias"], self.views["bn1.running_mean"],
                 self.views["bn1.running_var"], sm, si, self._stem_sums, self._stem_slots, N, hw, hw, 64, BN_EPS,
                 BN_MOMENTUM, self.dt)
            self.num_batches_tracked["bn1"] += 1
        elif self._stem_fused:
            sm, si = self.save["bn1"]
            call("primia_bn_relu_maxpool_fwd", t["stem.y"], t["pool.out"], self.pool_argmax, self.views["bn1.weight"],
                 self.views["bn1.bias"], self.views["bn1.running_mean"], self.views["bn1.running_var"], sm, si, N, hw,
                 hw, 64, BN_EPS, BN_MOMENTUM, self.bn_ws, self.bn_ws_bytes, self.dt)
            self.num_batches_tracked["bn1"] += 1
        elif self._stem_fused_gn:
            sm, si = self.save["bn1"]
            call("primia_gn_relu_maxpool_fwd", t["stem.y"], t["pool.out"], self.pool_argmax, self.views["bn1.weight"],
                 self.views["bn1.bias"], sm, si, N, hw, hw, 64, self.groups, BN_EPS, self.bn_ws, self.bn_ws_bytes, self.dt)
        else:
            self._bn("conv1", t["stem.y"], t["stem.z"], None, True)
        if self._stem_fused or self._stem_fused_gn or stem_done:
            pass
        elif self.spec.pooling == "max":
            call("primia_maxpool3x3s2_fwd", t["stem.z"], t["pool.out"], self.pool_argmax, N, hw, hw, 64, self.dt)
        else:
            call("primia_avgpool3x3s2_fwd", t["stem.z"], t["pool.out"], N, hw, hw, 64, self.dt)
        x = t["pool.out"]
        for blk in self.spec.blocks:
            p = blk.prefix
            # transition block: conv1 and the downsample read the same x — one launch (primia_conv2d_fwd_stats_pair)
            down_done = blk.down is not None and self._conv_fwd_pair(blk, x, t[p + ".y1"], t[p + ".yd"])
            if not down_done:
                self._conv_fwd(blk.conv1.name, x, t[p + ".y1"])
            self._bn(blk.conv1.name, t[p + ".y1"], t[p + ".a1"], None, True)
            self._conv_fwd(blk.conv2.name, t[p + ".a1"], t[p + ".y2"])
            idn = x
            if blk.down is not None and self.training and self.batch_stats:
                # transition block: both BatchNorms in one apply pass (the downsample branch's output is never stored)
                if not down_done:
                    self._conv_fwd(blk.down.name, x, t[p + ".yd"])
                b2, bd = bn_name(blk.conv2.name), bn_name(blk.down.name)
                y2 = t[p + ".y2"]
                mask = self._relu_mask(b2, y2)
                c2 = self.convs[blk.conv2.name]
                have = blk.conv2.name in self.free_stats
                cd = self.convs[blk.down.name]
                have_d = blk.down.name in self.free_stats
                (sm2, si2), (smd, sid) = self.save[b2], self.save[bd]
                call("primia_bn_fwd_train_pair", y2, t[p + ".yd"], t[p + ".out"], mask,
                     self.views[b2 + ".weight"], self.views[b2 + ".bias"], self.views[b2 + ".running_mean"],
                     self.views[b2 + ".running_var"], sm2, si2, c2.sums if have else None, c2.stat_slots if have else 0,
                     self.views[bd + ".weight"], self.views[bd + ".bias"], self.views[bd + ".running_mean"],
                     self.views[bd + ".running_var"], smd, sid, cd.sums if have_d else None, cd.stat_slots if have_d else 0,
                     y2.shape[0], y2.shape[1], BN_EPS, BN_MOMENTUM, self.bn_ws, self.bn_ws_bytes, self.dt)
                self.num_batches_tracked[b2] += 1
                self.num_batches_tracked[bd] += 1
                x = t[p + ".out"]
                continue
            if blk.down is not None:
                if not down_done:
                    self._conv_fwd(blk.down.name, x, t[p + ".yd"])
                self._bn(blk.down.name, t[p + ".yd"], t[p + ".idn"], None, False)
                idn = t[p + ".idn"]
            self._bn(blk.conv2.name, t[p + ".y2"], t[p + ".out"], idn, True)
            x = t[p + ".out"]
        hw = self.final_hw
        call("primia_head_fwd", x, self.views["fc.weight"], self.views["fc.bias"], self.feat, self.logits, N, hw * hw,
             512, self.spec.num_classes, self.dt)
        return self.logits

    __call__ = forward

    # ------------------------------------------------------------------------------------------
    # loss + backward
    # ------------------------------------------------------------------------------------------
    dp_params = None  # e.g. {"max_grad_norm": 1.0, "noise_multiplier": 1.3}: loss_backward() becomes DP-SGD
    dp_noise = None   # a primia_amd.dp_noise.DeviceNoise: the DP-SGD noise is its ChaCha20 stream instead of torch.randn
    # a primia_amd.dp_clip.AdaptiveClip: the clipping norm is ITS device word (dp_params' max_grad_norm is not read), every
    # logical step releases a noisy count and moves it.  The root's, like dp_noise: a sibling on a ragged batch uses it.
    dp_clip = None
    # A logical DP-SGD step larger than the engine (primia_amd.dp_micro.step): the host loops run it as this many passes of
    # N slots each, and tell loss_backward the phase of each pass.
    dp_micro_batches = 1

    @property
    def dp_acc(self):
        """fp32 [P]: the clipped sums of a logical step's passes so far.  The root's, like dp_noise: a ragged piece on a
        sibling accumulates into the same sum.  Created at first use — before any capture (graphed_train)."""
        root = self._root
        if root.__dict__.get("_dp_acc") is None:
            root._dp_acc = torch.zeros(self.P, dtype=torch.float32, device=self.device)
        return root._dp_acc

    def loss_backward(self, target, soft=False, phase=None, logical_batch=None):
        """Cross entropy (hard int64 labels, or soft [N, classes] fp32 targets as in
        Cross_entropy_one_hot) + full backward into `grads`.  Returns the device loss scalar.
        `phase`, `logical_batch` (DP-SGD only): this call is a pass of a logical step cut into micro-batches
        (primia_amd.dp_micro) — dp_loss_backward's `accumulate` and `logical_batch`."""
        if self.dp_params is not None:
            if soft:
                raise _lib.PrimiaError("DP-SGD path takes hard labels")
            return self.dp_loss_backward(target, **self.dp_params, accumulate=phase, logical_batch=logical_batch)
        if soft:
            call("primia_xent_soft", self.logits, target, self.class_weight, self.loss, self.dlogits, self.N,
                 self.spec.num_classes)
        else:
            call("primia_xent_hard", self.logits, target, self.class_weight, self.loss, self.dlogits, self.N,
                 self.spec.num_classes)
        self.backward()
        return self.loss

    def _bn_bwd(self, conv_name, y, z, dz, dy, g_out, relu, keep_g=True, from_sums=None, mask=None):
        """Backward pass of the norm layer behind conv `conv_name`, whatever the kind.
        `mask`: 1-bit ReLU mask applied to dz instead of reading z — by default the layer's own, where its forward pass
        wrote one (residual layers); a transition block's downsample norm is given bn2's, with g_out=None.
        keep_g=False (with a mask only): the masked gradient g is NOT written back over dz — the accumulating data
        gradient that consumes it applies the mask itself (primia_conv2d_dgrad_masked_acc).
        `from_sums` (partials, slots): the producer of dz has formed the backward sums (training BatchNorm statistics)."""
        b = bn_name(conv_name)
        if mask is None and relu and g_out is not None:
            mask = self.relu_masks.get(b)
        gam = self.views[b + ".weight"]
        M, C = y.shape
        if mask is not None and from_sums is not None:
            sm, si = self.save[b]
            call("primia_bn_bwd_mask_from_sums", y, mask, dz, dy, g_out if keep_g else None, gam, sm, si,
                 self._gviews[b + ".weight"], self._gviews[b + ".bias"], from_sums[0], from_sums[1], M, C, self.dt)
            return
        # one argument frame for the three kinds: the statistics operands, where dgamma / dbeta go (the gradient views; per
        # sample for GroupNorm and frozen BatchNorm), the dimensions
        relu_bwd, bwd_mask, bwd = self._bwd_entries
        dims = (M, C) if self.batch_stats else (self.N, M // self.N, C) + self._ps_groups
        frame = self._bwd_stats[b] + self._bwd_affine[b] + dims
        if mask is not None:
            # mask bytes instead of z
            call(bwd_mask, y, mask, dz, dy, g_out if keep_g else None, gam, *frame, self.bn_ws, self.bn_ws_bytes, self.dt)
        elif relu and g_out is None:
            # z = relu(norm(y)), no residual: the mask is recomputed from y, z is not read
            call(relu_bwd, y, dz, dy, gam, self.views[b + ".bias"], *frame, self.bn_ws, self.bn_ws_bytes, self.dt)
        else:
            call(bwd, y, z, dz, dy, g_out, gam, *frame, int(relu), self.bn_ws, self.bn_ws_bytes, self.dt)
        self._reduce_affine(b)

    def _reduce_affine(self, b):
        """Per-sample kinds: dgamma / dbeta of norm layer b = the sum over samples of its per-sample affine gradients —
        unless a DP-SGD pass is in flight, which clips them first (_dp_clipped_sums)."""
        if self.per_sample_norm and self.dp is None:
            psg, psb = self.ps_affine[b]
            C = psg.shape[1]
            call("primia_weighted_colsum", psg, self.ones_n, self._gviews[b + ".weight"], self.N, C)
            call("primia_weighted_colsum", psb, self.ones_n, self._gviews[b + ".bias"], self.N, C)

    # a stage's LAST same-shape layer does not wait for a group that can no longer fill (layer4 at batch 256: groups of 2 for 3
    # layers): its weight gradient runs as soon as its dy exists instead of at the end of the backward pass (round 6)
    wgrad_flush_last = True
    # GroupNorm residual layers with the BatchNorm path's 1-bit ReLU masks (and its mask-applying accumulate dgrad)
    gn_relu_masks = True
    gn_stem_fused = True
    # (bf16: a stage's same-shape 3x3 weight gradients run as one launch, primia_conv2d_wgrad_group_ws.  All 13 layers in ONE
    # launch at the end of the backward pass was built and measured no better than the per-stage groups — 5.16 vs 5.14 ms:
    # by then every operand comes from HBM, while a stage's group still finds its newest dy in the Infinity Cache — and is
    # not kept: profiles/r03_negative_results.txt)

    def _wgrad(self, name, x, dy):
        """The backward pass has reached layer `name`'s dy: issue its weight gradient — under DP-SGD, note the operands
        for the norm pass and the clipped sums, which issue it once the rows of dy carry the clip factors."""
        if self.dp is not None:
            self.dp["wgrads"].append((name, x, dy))
            return
        self._issue_wgrad(name, x, dy)

    # measurement hook (tools/power_idle_ab.py): called after every grouped 3x3 weight-gradient launch; None in every product run
    after_wgrad_hook = None

    def _issue_wgrad(self, name, x, dy):
        """THE scheduler of the batched weight gradients, for the plain backward pass and the DP-SGD clipped sums alike: the
        layer's own launch now, or — half of a transition pair, member of a same-shape group (c.wg_hold, decided by the
        constructor) — held until the launch it shares is complete.  _finalize_wgrads closes the pass."""
        c = self.convs[name]
        if c.wg_hold is None:
            return self._launch_wgrads([(name, x, dy)])
        key, fill, feeders = c.wg_hold
        held = self._wg_held.setdefault(key, [])
        held.append((name, x, dy))
        self._wg_seen[key] = self._wg_seen.get(key, 0) + 1
        # a full launch — or the stage's last layer (layer4 at batch 256: groups of 2 for 3 layers): it runs NOW, while its
        # dy is the newest tensor in the Infinity Cache, not at the end of the pass
        if len(held) == fill or (self.wgrad_flush_last and self._wg_seen[key] == feeders):
            self._flush_wgrads(key)

    def _flush_wgrads(self, key):
        held = self._wg_held.pop(key)
        try:
            self._launch_wgrads(held)
        finally:
            if self.after_wgrad_hook is not None and self.convs[held[0][0]].wg == "group":
                self.after_wgrad_hook()

    def _launch_wgrads(self, held):
        """One launch for (name, x, dy) triples that share one: a transition block's (conv1, downsample) in the order the
        backward pass reaches them, two to four layers of one shape — or a layer alone, a group's left-over one included.
        One workspace: the launches stay in order on whichever stream."""
        c = self.convs[held[0][0]]
        ws = (self.wgrad_ws, self.wgrad_ws_bytes)
        extra = 0
        if len(held) == 1:
            (_, x, dy), = held
            if c.wg == "stem":
                S = self.spec.input_size
                fn = lambda: call("primia_stem_conv_wgrad_ws", x, dy, c.acc, *ws, self.N, S, S, self.dt)
            else:
                fn = lambda: call("primia_conv2d_wgrad_ws", c.desc, x, dy, c.acc, *ws, self.dt)
        elif c.wg == "pair":
            (_, x, dy1), (down, _, dyd) = held
            cd = self.convs[down]
            extra = self._macs(cd)
            fn = lambda: call("primia_conv2d_wgrad_pair_ws", c.desc, x, dy1, c.acc, cd.desc, dyd, cd.acc, *ws, self.dt)
        else:
            args = [a for nm, x, dy in held for a in (x, dy, self.convs[nm].acc)] + [None] * (3 * (4 - len(held)))
            extra = (len(held) - 1) * self._macs(c)
            fn = lambda: call("primia_conv2d_wgrad_group_ws", c.desc, len(held), *args, *ws, self.dt)
        self._on_wgrad_stream(lambda: self._timed("wgrad", c, fn, extra_macs=extra), transition=c.wg == "pair")

    def _finalize_wgrads(self):
        """Closing half of _issue_wgrad: what is still held (groups that never filled: odd layer counts), the second
        stream, then accumulators -> OIHW gradients."""
        for key in list(self._wg_held):
            self._flush_wgrads(key)
        self._join_wgrad_stream()
        if self.fuse_sgd_tail and self.dp is None and self._sgd_tail_plan() is not None:
            # the accumulators stay as they are: sgd_step() turns them into gradients, new weights and new kernel-layout
            # copies in one pass per tile; anything else that wants the gradients calls materialize_grads()
            self._grads_pending = True
            return
        m = self._many_args()
        call("primia_conv_wgrad_finalize_many", m["descs"], m["creal"], m["acc"], m["gw"], m["n"])

    # Every batched weight-gradient launch goes through _on_wgrad_stream (from _launch_wgrads; primia_stem_bwd_fused from
    # backward()), in the plain pass and in DP-SGD's clipped sums alike.  With wgrad_overlap = 0 — every product run — it
    # runs the launch where it stands.  The option:
    # Weight gradients are leaves of the backward graph (nothing reads them before the finalize) and every layer
    # has its own dy buffer, so they can run on a second stream.  Overlapping them with EVERYTHING was slower
    # (7.70 -> 7.91 ms: wgrad and dgrad tiles evict each other from the CUs).  With `wgrad_overlap` the schedule is
    # narrower: a layer's wgrad starts after its sibling dgrad and runs beside the BatchNorm backward chain that
    # follows (HBM-bound kernels and 7-us finalize launches); the next dgrad waits for it.  Also slower on
    # MI355X (7.10 ms serial -> 7.30 ms): kept as an option for other shapes, off by default.
    # wgrad_overlap = 3: see _on_wgrad_stream.
    # Re-measured in round 3 with the workspace kernels (wgrad_overlap = 1: the schedule above; = 2: the weight
    # gradients free-running on the second stream until the finalize): see profiles/r03_negative_results.txt.
    wgrad_overlap = 0

    def _on_wgrad_stream(self, fn, transition=False):
        if self.wgrad_overlap == 3 and not transition and self.prof is None:
            # mode 3 (round 6): ONLY a transition block's paired weight gradient leaves the main stream — it runs beside the
            # block's paired data gradient, two launches that each leave the matrix pipe idle 80 % of the time (short reduction
            # axes: their tiles are write-back and staging latency) — and every other weight gradient stays in line, behind it
            # (one workspace)
            self._join_wgrad_stream()
            return fn()
        if not self.wgrad_overlap or self.prof is not None:
            return fn()
        if self._wg_stream is None:
            self._wg_stream = torch.cuda.Stream(device=self.device)
        main = torch.cuda.current_stream()
        self._wg_stream.wait_stream(main)        # dy (and the zeroed accumulators) are ready
        with torch.cuda.stream(self._wg_stream):
            fn()
        self._wg_pending = True

    def _join_wgrad_stream(self):
        if self._wg_pending:
            torch.cuda.current_stream().wait_stream(self._wg_stream)
            self._wg_pending = False

    @property
    def _fuse_bwd_sums(self):
        """Training BatchNorm statistics and no DP-SGD pass in flight: whatever completes a gradient may also form the
        backward sums of the BatchNorm that consumes it (the *_bnsums entries).  Each site adds its own terms."""
        return self.batch_stats and self.dp is None

    @property
    def _fuse_bwd_sums_bf16(self):
        return self._fuse_bwd_sums and self.dtype == torch.bfloat16

    def _head_bnsums_ok(self):
        # primia_head_bwd_bnsums: 256 threads must be a multiple of the 16-byte chunks of a 512-channel row
        return 256 % (512 // (4 if self.dtype == torch.float32 else 8)) == 0

    def _stem_bwd_fused_wanted(self):
        """The stem's backward tail runs as primia_bn_relu_maxpool_bwd (sums only) + primia_stem_bwd_fused."""
        if self._stem_bwd_fused_ok is None:     # asked once: the library's own gate for this shape
            S0 = self.spec.input_size
            self._stem_bwd_fused_ok = query("primia_stem_bwd_fused_ok", self.N, S0, S0, self.dt) == 1
        return bool(self._stem_fused and self.x0p is not None and self.dp is None and self._stem_bwd_fused_ok)

    def _dgrad_bnsums_slots(self, name):
        """Rows of the partial table conv `name`'s data gradient writes for the BatchNorm in front of it (0: not served)."""
        c = self.convs[name]
        if c.bnsums_slots is None:      # (a property of the layer: asked once, whatever self.dp is then)
            c.bnsums_slots = query("primia_conv_dgrad_bnsums_slots", c.desc, self.dt) if self.dtype == torch.bfloat16 else 0
        return c.bnsums_slots if self.dp is None else 0

    def _bwd_sums(self, name, slots, channels):
        tab = self._bwd_sum_bufs
        if name not in tab or tab[name].numel() != slots * 2 * channels:
            tab[name] = torch.empty(slots * 2 * channels, dtype=torch.float32, device=self.device)
        return tab[name]

    def _dgrad(self, name, dy, dx, accumulate):
        """Data gradient of conv `name` into dx (accumulate: added to what dx holds)."""
        c = self.convs[name]
        if self.wgrad_overlap == 1:
            self._join_wgrad_stream()   # (narrow overlap) two MFMA-bound kernels never run side by side
        self._timed("dgrad", c,
                    lambda: call("primia_conv2d_dgrad", c.desc, dy, c.w_dgrad, dx, int(accumulate), self.dt))

    def _backward_conv2(self, blk):
        """conv2's weight and data gradients, then bn1's backward pass.  The weight gradient goes first, so that the
        BatchNorm backward pass finds the data gradient it reads still in the Infinity Cache."""
        t, p = self.t, blk.prefix
        self._wgrad(blk.conv2.name, t[p + ".a1"], t[p + ".dy2"])
        # where the linear-halo kernels serve conv2, its data gradient also forms bn1's backward sums
        # (primia_conv2d_dgrad_bnsums): the reduction pass over (y1, da1) is dropped
        # (no DP or dtype term here: _dgrad_bnsums_slots has them)
        slots = self._dgrad_bnsums_slots(blk.conv2.name) if self.batch_stats else 0
        if not slots:
            self._dgrad(blk.conv2.name, t[p + ".dy2"], t[p + ".da1"], False)
            self._bn_bwd(blk.conv1.name, t[p + ".y1"], t[p + ".a1"], t[p + ".da1"], t[p + ".dy1"], None, True)
            return
        c2, b1 = self.convs[blk.conv2.name], bn_name(blk.conv1.name)
        sm1, si1 = self.save[b1]
        if self.wgrad_overlap == 1:
            self._join_wgrad_stream()   # (as _dgrad does: two MFMA-bound kernels never run side by side)
        sums = self._bwd_sums(blk.conv2.name, slots, blk.conv1.cout)
        self._timed("dgrad", c2, lambda: call(
            "primia_conv2d_dgrad_bnsums", c2.desc, t[p + ".dy2"], c2.w_dgrad, t[p + ".da1"], t[p + ".y1"], sm1, si1,
            self.views[b1 + ".weight"], self.views[b1 + ".bias"], sums, self.dt))
        y1 = t[p + ".y1"]
        call("primia_bn_relu_bwd_from_sums", y1, t[p + ".da1"], t[p + ".dy1"], self.views[b1 + ".weight"],
             self.views[b1 + ".bias"], sm1, si1, self._gviews[b1 + ".weight"], self._gviews[b1 + ".bias"], sums, slots,
             y1.shape[0], y1.shape[1], self.dt)

    def _backward_identity(self, blk, prev, x_in, dx_in):
        """Identity block: dx_in aliases dout, which conv1's accumulating data gradient completes in place."""
        t, p = self.t, blk.prefix
        dout, dy1 = t[p + ".dout"], t[p + ".dy1"]
        b2 = bn_name(blk.conv2.name)
        # bn2 (+residual, relu): dy2, and the masked gradient g written back over dout — unless conv1's accumulating data
        # gradient can apply bn2's ReLU mask to the old values itself (one tensor write less)
        masked_acc = self.masked_acc_ok[blk.conv1.name] and b2 in self.relu_masks
        self._bn_bwd(blk.conv2.name, t[p + ".y2"], t[p + ".out"], dout, t[p + ".dy2"], dout, True, keep_g=not masked_acc,
                     from_sums=self._dout_sums.pop(p, None))
        self._backward_conv2(blk)
        self._wgrad(blk.conv1.name, x_in, dy1)
        if not masked_acc:
            self._dgrad(blk.conv1.name, dy1, dx_in, True)
            return
        c1 = self.convs[blk.conv1.name]
        if self.wgrad_overlap == 1:
            self._join_wgrad_stream()
        # ... whose write-back also forms the backward sums of the BatchNorm whose output gradient it completes
        # (primia_conv2d_dgrad_masked_acc_bnsums; 64 -> 64 layers): the previous block's bn2 (mode 2), or the stem's bn1
        # through the max-pool (mode 3) — the two most expensive reduction passes of the step (43 + 48 us)
        mode = 0
        if self._fuse_bwd_sums_bf16:
            if prev is not None and prev.down is None and bn_name(prev.conv2.name) in self.relu_masks:
                mode = 2
            elif prev is None and self._stem_bwd_fused_wanted():
                mode = 3
        if mode and c1.acc_bnsums_slots is None:
            c1.acc_bnsums_slots = query("primia_conv_dgrad_masked_acc_bnsums_slots", c1.desc, self.dt)
        slots = c1.acc_bnsums_slots if mode else 0
        if slots > 0 and mode == 2:
            sums = self._bwd_sums(blk.conv1.name + ".acc", slots, prev.conv2.cout)
            pb2 = bn_name(prev.conv2.name)
            smp, sip = self.save[pb2]
            self._timed("dgrad", c1, lambda: call(
                "primia_conv2d_dgrad_masked_acc_bnsums", c1.desc, dy1, c1.w_dgrad, dx_in, self.relu_masks[b2], 2,
                t[prev.prefix + ".y2"], self.relu_masks[pb2], smp, sip, sums, self.dt))
            self._dout_sums[prev.prefix] = (sums, slots)
        elif slots > 0:
            sums = self._bwd_sums(blk.conv1.name + ".acc", slots, 64)
            self._timed("dgrad", c1, lambda: call(
                "primia_conv2d_dgrad_masked_acc_bnsums", c1.desc, dy1, c1.w_dgrad, dx_in, self.relu_masks[b2], 3,
                t["pool.out"], None, self.views["bn1.bias"], self.views["bn1.weight"], sums, self.dt))
            self._pool_sums = (sums, slots)
        else:
            self._timed("dgrad", c1, lambda: call("primia_conv2d_dgrad_masked_acc", c1.desc, dy1, c1.w_dgrad, dx_in,
                                                  self.relu_masks[b2], self.dt))

    def _backward_transition(self, blk, prev, x_in, dx_in):
        """Transition block: both BatchNorm backward passes, then ONE weight-gradient and ONE data-gradient launch for
        conv1 + downsample (primia_conv2d_dgrad_pair)."""
        t, p = self.t, blk.prefix
        dout, dy1, dyd = t[p + ".dout"], t[p + ".dy1"], t[p + ".dyd"]
        b2, bd = bn_name(blk.conv2.name), bn_name(blk.down.name)
        mask = self.relu_masks.get(b2)
        if mask is not None and self.batch_stats:
            # bn2 and the downsample BatchNorm share the incoming gradient -> ONE fused backward pass (primia_bn_bwd_pair)
            (sm2, si2), (smd, sid) = self.save[b2], self.save[bd]
            call("primia_bn_bwd_pair", t[p + ".y2"], t[p + ".yd"], dout, mask, t[p + ".dy2"], dyd,
                 self.views[b2 + ".weight"], sm2, si2, self.views[bd + ".weight"], smd, sid, self._gviews[b2 + ".weight"],
                 self._gviews[b2 + ".bias"], self._gviews[bd + ".weight"], self._gviews[bd + ".bias"],
                 t[p + ".y2"].shape[0], t[p + ".y2"].shape[1], self.bn_ws, self.bn_ws_bytes, self.dt)
            self._backward_conv2(blk)
        else:
            # no paired kernel: two calls.  With a mask the downsample norm's backward pass applies bn2's ReLU mask to dout
            # itself, so bn2's does not write the masked gradient
            self._bn_bwd(blk.conv2.name, t[p + ".y2"], t[p + ".out"], dout, t[p + ".dy2"], dout, True, keep_g=mask is None)
            self._backward_conv2(blk)
            self._bn_bwd(blk.down.name, t[p + ".yd"], None, dout, dyd, None, False, mask=mask)
        c1, cd = self.convs[blk.conv1.name], self.convs[blk.down.name]
        if self.wgrad_overlap == 1:
            self._join_wgrad_stream()
        self._wgrad(blk.conv1.name, x_in, dy1)
        self._wgrad(blk.down.name, x_in, dyd)    # (completes the pair where the library serves one)
        # the paired data gradient also forms the backward sums of the residual BatchNorm in front of the block
        # (primia_conv2d_dgrad_pair_bnsums: conv_s2lh_kernel for 64-channel dx, conv_igemm_kernel's parity-class walk for
        # layer3.0 / layer4.0)
        pslots = 0
        pb2 = bn_name(prev.conv2.name) if prev is not None else None
        if self._fuse_bwd_sums_bf16 and prev is not None and prev.down is None and pb2 in self.relu_masks:
            if c1.pair_bnsums_slots is None:
                c1.pair_bnsums_slots = query("primia_conv_dgrad_pair_bnsums_slots", c1.desc, self.dt)
            pslots = c1.pair_bnsums_slots
        if pslots > 0:
            sums = self._bwd_sums(blk.conv1.name + ".pair", pslots, prev.conv2.cout)
            smp, sip = self.save[pb2]
            self._timed("dgrad", c1, lambda: call(
                "primia_conv2d_dgrad_pair_bnsums", c1.desc, dy1, c1.w_dgrad, cd.desc, dyd, cd.w_dgrad, dx_in,
                t[prev.prefix + ".y2"], self.relu_masks[pb2], smp, sip, sums, self.dt), extra_macs=self._macs(cd))
            self._dout_sums[prev.prefix] = (sums, pslots)
        else:
            self._timed("dgrad", c1, lambda: call("primia_conv2d_dgrad_pair", c1.desc, dy1, c1.w_dgrad, cd.desc, dyd,
                                                  cd.w_dgrad, dx_in, self.dt), extra_macs=self._macs(cd))

    def backward(self):
        N, t = self.N, self.t
        nc = self.spec.num_classes
        if query("primia_options_epoch") != self._options_epoch:
            raise _lib.PrimiaError("library options changed (primia_set_option) after this engine sized its buffers")
        self._grads_pending = False      # (accumulators of an earlier pass that nobody consumed are overwritten now)
        self._wg_seen = {}
        self._dout_sums = {}             # block prefix -> (partials, slots): backward sums of its bn2 formed by the producer of dout
        if self.dp is None:
            # the other layers' accumulators are overwritten — conv1's too where its weight gradient runs on the padded input
            # (primia_stem_bwd_fused ends in an ordered reduce that WRITES the slab): then the step has
            # no fill launch at all (tests: test_weight_gradient_accumulators_are_overwritten poisons the arena between steps)
            stem_overwrites = self._acc_zero_only_stem and self._stem_bwd_fused_wanted()
            if not stem_overwrites:
                self.dw_acc[:self._acc_zero_n].zero_()
        else:
            self.dw_acc.zero_()
        # (under DP-SGD fc.weight / fc.bias gradients are overwritten later from the clipped dlogits)
        call("primia_linear_bwd", self.feat, self.views["fc.weight"], self.dlogits, None,
             self._gviews["fc.weight"], self._gviews["fc.bias"], N, 512, nc)
        last = self.spec.blocks[-1].prefix
        hw = self.final_hw
        blocks = self.spec.blocks
        lb2 = bn_name(blocks[-1].conv2.name)
        if self._fuse_bwd_sums and blocks[-1].down is None and lb2 in self.relu_masks and self._head_bnsums_ok():
            # ... forming the backward sums of the last block's bn2 on the way (one value per image and channel)
            sums = self._bwd_sums("head", N, 512)
            sml, sil = self.save[lb2]
            call("primia_head_bwd_bnsums", self.views["fc.weight"], self.dlogits, t[last + ".dout"], t[last + ".y2"],
                 self.relu_masks[lb2], sml, sil, sums, N, hw * hw, 512, nc, self.dt)
            self._dout_sums[last] = (sums, N)
        else:
            call("primia_head_bwd", self.views["fc.weight"], self.dlogits, t[last + ".dout"], N, hw * hw, 512, nc, self.dt)
        for i in range(len(blocks) - 1, -1, -1):
            blk, prev = blocks[i], (blocks[i - 1] if i > 0 else None)
            x_in = t[prev.prefix + ".out"] if prev is not None else t["pool.out"]
            dx_in = t[prev.prefix + ".dout"] if prev is not None else t["pool.dout"]
            if self.taps is not None:
                self.taps[blk.prefix + ".dout_in"] = t[blk.prefix + ".dout"].clone()
            if blk.down is None:
                self._backward_identity(blk, prev, x_in, dx_in)
            else:
                self._backward_transition(blk, prev, x_in, dx_in)
        hw = self.stem_hw
        # the stem's tail in two launches less and without the dy tensor (411 MB at batch 256): bn1's backward sums at
        # pooled resolution, then conv1's weight gradient forming its dy tiles on the fly (primia_stem_bwd_fused)
        stem_bwd_fused = self._stem_bwd_fused_wanted()
        self.stem_bwd_fused_active = stem_bwd_fused
        pool_sums, self._pool_sums = self._pool_sums, None
        if stem_bwd_fused:
            sm, si = self.save["bn1"]
            c = self.convs["conv1"]
            S = self.spec.input_size
            if pool_sums is not None:     # the reduction over (pooled, dpooled) happened in layer1.0.conv1's data gradient
                call("primia_bn_relu_maxpool_bwd_from_sums", t["stem.y"], t["pool.out"], t["pool.dout"], self.pool_argmax,
                     self.views["bn1.weight"], self.views["bn1.bias"], sm, si, self._gviews["bn1.weight"],
                     self._gviews["bn1.bias"], pool_sums[0], pool_sums[1], N, hw, hw, 64, self.dt)
            else:
                call("primia_bn_relu_maxpool_bwd", t["stem.y"], t["pool.out"], t["pool.dout"], self.pool_argmax, None,
                     self.views["bn1.weight"], self.views["bn1.bias"], sm, si, self._gviews["bn1.weight"],
                     self._gviews["bn1.bias"], N, hw, hw, 64, self.bn_ws, self.bn_ws_bytes, self.dt)
            self._on_wgrad_stream(lambda: self._timed("wgrad", c, lambda: call(
                "primia_stem_bwd_fused", self.x0p, t["stem.y"], t["pool.dout"], self.pool_argmax,
                self.views["bn1.weight"], self.views["bn1.bias"], sm, si, self._gviews["bn1.weight"],
                self._gviews["bn1.bias"], c.acc, self.wgrad_ws, self.wgrad_ws_bytes, N, S, S, self.dt)))
            if self.dp is None:
                self._finalize_wgrads()
            return
        if self._stem_fused:
            sm, si = self.save["bn1"]
            call("primia_bn_relu_maxpool_bwd", t["stem.y"], t["pool.out"], t["pool.dout"], self.pool_argmax, t["stem.dy"],
                 self.views["bn1.weight"], self.views["bn1.bias"], sm, si, self._gviews["bn1.weight"],
                 self._gviews["bn1.bias"], N, hw, hw, 64, self.bn_ws, self.bn_ws_bytes, self.dt)
        elif self._stem_fused_gn:
            sm, si = self.save["bn1"]
            psg, psb = self.ps_affine["bn1"]
            call("primia_gn_relu_maxpool_bwd", t["stem.y"], t["pool.out"], t["pool.dout"], self.pool_argmax, t["stem.dy"],
                 self.views["bn1.weight"], self.views["bn1.bias"], sm, si, psg, psb, N, hw, hw, 64, self.groups,
                 self.bn_ws, self.bn_ws_bytes, self.dt)
            self._reduce_affine("bn1")
        else:
            if self.spec.pooling == "max":
                call("primia_maxpool3x3s2_bwd", t["pool.dout"], self.pool_argmax, t["stem.dz"], N, hw, hw, 64, self.dt)
            else:
                call("primia_avgpool3x3s2_bwd", t["pool.dout"], t["stem.dz"], N, hw, hw, 64, self.dt)
            self._bn_bwd("conv1", t["stem.y"], t["stem.z"], t["stem.dz"], t["stem.dy"], None, True)
        self._wgrad("conv1", self.convs["conv1"].wg_x, t["stem.dy"])
        if self.dp is None:
            self._finalize_wgrads()

    # The step's tail — accumulator -> OIHW gradient, SGD on the fp32 master, master -> compute-dtype copies — as ONE
    # pass per weight tile (primia_conv_sgd_step_many: 95 -> ~55 us at batch 256, bit-identical weights and gradients).
    # Opt-in: between loss_backward() and sgd_step() the conv gradients then live in the accumulators only;
    # materialize_grads() (called by every other reader in this class) writes them out the unfused way.
    fuse_sgd_tail = False
    _grads_pending = False

    def _sgd_tail_plan(self):
        """(fused conv args, remaining conv args or None, SGD ranges outside the fused weights) — built once."""
        if getattr(self, "_sgd_plan", None) is None:
            import ctypes

            cs = list(self.convs.values())
            fus = [c for c in cs if query("primia_conv_sgd_fusable", c.desc, c.c_real) == 1 and c.w_dgrad is not None
                   and all(tt.data_ptr() % 16 == 0 for tt in (c.acc, c.w_fwd, c.w_dgrad, self.views[c.spec.name + ".weight"],
                                                              self._gviews[c.spec.name + ".weight"]))]
            rest = [c for c in cs if c not in fus]
            vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)

            def pack(lst):
                n = len(lst)
                if n == 0:
                    return None
                return dict(
                    n=n, descs=(ConvDesc * n)(*[c.desc for c in lst]), creal=(ctypes.c_int * n)(*[c.c_real for c in lst]),
                    w=(ctypes.c_void_p * n)(*[vp(self.views[c.spec.name + ".weight"]) for c in lst]),
                    wf=(ctypes.c_void_p * n)(*[vp(c.w_fwd) for c in lst]),
                    wd=(ctypes.c_void_p * n)(*[vp(c.w_dgrad) for c in lst]),
                    acc=(ctypes.c_void_p * n)(*[vp(c.acc) for c in lst]),
                    gw=(ctypes.c_void_p * n)(*[vp(self._gviews[c.spec.name + ".weight"]) for c in lst]))

            fused_keys = {c.spec.name + ".weight" for c in fus}
            ranges, off = [], 0
            for k, shp in self.p_entries:
                n = int(torch.Size(shp).numel())
                if k not in fused_keys:
                    if ranges and ranges[-1][0] + ranges[-1][1] == off:
                        ranges[-1][1] += n
                    else:
                        ranges.append([off, n])
                off += n
            if not fus or len(ranges) > 32:
                self._sgd_plan = False
            else:
                nr = len(ranges)
                self._sgd_plan = (pack(fus), pack(rest), (ctypes.c_int64 * nr)(*[r[0] for r in ranges]),
                                  (ctypes.c_int64 * nr)(*[r[1] for r in ranges]), nr)
        return self._sgd_plan or None

    @property
    def grads(self):
        """The flat gradient arena.  Reading it finishes a deferred conv-gradient pass first (fuse_sgd_tail), so a
        caller never sees gradients that still live in the accumulators; `gviews[...]` are views of the same storage —
        call materialize_grads() before reading THOSE between loss_backward() and sgd_step() under fuse_sgd_tail."""
        self.materialize_grads()
        return self._grads

    def materialize_grads(self):
        """Write the conv gradients out of the accumulators if a fused tail has left them there."""
        if self._grads_pending:
            m = self._many_args()
            call("primia_conv_wgrad_finalize_many", m["descs"], m["creal"], m["acc"], m["gw"], m["n"])
            self._grads_pending = False

    # ------------------------------------------------------------------------------------------
    # DP-SGD (BASELINE.json configs[3]; parameter values of train.py:325-334)
    # ------------------------------------------------------------------------------------------
    def dp_loss_backward(self, target, max_grad_norm=1.0, noise_multiplier=1.3, noise=None, generator=None,
                         expected_batch=None, accumulate=None, logical_batch=None, views=1):
        """Per-sample gradient clipping + Gaussian noise, pytorch-dp semantics:
            g = (1/B) * ( sum_n min(1, C / (||g_n|| + 1e-6)) * g_n  +  N(0, (noise_multiplier*C)^2 I) )
        with g_n the gradient of sample n's OWN loss over all 62 parameter tensors (flat L2 norm).
        Needs norm="group" or norm="frozen".  `noise` (fp32 [P], standard normal) may be given for reproducibility; without it (and without
        a `generator`) the root engine's `dp_noise` stream is used when set, torch.randn otherwise.

        How: one ordinary backward pass yields every layer's activation gradient dy (samples are
        independent under GroupNorm and under BatchNorm with frozen statistics).  Pass 1 runs the weight-gradient kernels with one pixel split per image
        and has every block add the squares of ITS (complete) per-sample tile to ||g_n||^2 — the per-sample
        gradients are never written; then each sample's rows of
        dy are scaled by its clip factor and the ordinary batched wgrad — linear in dy — produces
        sum_n clip_n * g_n directly.

        `expected_batch` (a float L: dp_params of a Poisson-sampled run, primia_amd.dp_sampling): the batch is a
        fixed-capacity one whose padded slots carry target -1.  Those get a zero dlogits row and a zero clip factor —
        every contribution of theirs to the norms and the clipped sums is exactly zero — and the noised sum is divided
        by L, not by the number of slots: the sampled Gaussian mechanism the accountant (dp_accountant) bounds.

        `accumulate` (primia_amd.dp_micro: a logical step of `logical_batch` samples cut into passes of N slots; the sum
        above splits exactly into the passes' clipped sums).  "first" / "more": everything up to the clipped sums as
        usual, then dp_acc = grads / dp_acc += grads — no noise, no division.  "last": grads = ((dp_acc + grads) +
        noise) / B in one kernel, B = expected_batch on masked batches and logical_batch otherwise: one noise draw and
        one counter advance per logical step.  None: an ordinary step.

        With the root's `dp_clip` set (primia_amd.dp_clip.AdaptiveClip) C is that object's device word instead of
        `max_grad_norm`: the clip factors come with the step's {below, valid} counts (dp_stats["counts"]: private, for
        tests), the noise is z_delta * C, and the last (or only) pass moves C once — see _dp_adaptive_tail.

        `views` (m > 1: augmentation multiplicity, De et al. 2022; `train.py --dp_augmult`): the N slots are R = N / m
        RECORDS of m consecutive views of one image (same target; a padded record has m targets of -1).  A record
        contributes the AVERAGE of its views' gradients, clipped once:
            g_r = (1/m) sum_{n in record r} g_n,   c_r = min(1, C / (||g_r|| + 1e-6)),   g = (sum_r c_r g_r + noise) / B
        with B, expected_batch and logical_batch counted in records.  The dlogits rows are scaled by 1/m up front, so
        every slot gradient below is g_n / m and a record's gradient a plain sum; the norm pass completes each kernel's
        tile over a record's images (primia_conv2d_wgrad_record_sqnorm: the cross terms between views), dp_stats has
        R entries, and each record's clip factor is expanded to its slots for the clipped sums.  The kept-tile forms
        are per sample: an engine with views > 1 runs the two-pass form on every layer.

        With `self.class_weight` set (fp32 [classes] on the device; train.py: weight_classes, primia_amd.dp_weights) the
        loss is the PER-SAMPLE weighted one, loss_n = w[y_n] * CE_n, and g_n above its gradient: w[y_n] times the
        unweighted one.  There is no division by the batch's weight sum as in the non-DP weighted mean — it would make
        g_n depend on which other samples were drawn; the normalisation of w is fixed before training (equal class
        counts give w = 1 and the unweighted step, bit for bit).  primia_xent_dp_weighted forms w[y_n] / views *
        (softmax - onehot) on masked and full batches alike and stands in for the loss kernel and the scale after it;
        everything that follows is a function of dlogits.  engine.loss is the mean of w[y_n] * CE_n over the valid slots."""
        masked = expected_batch is not None
        if accumulate not in (None, "first", "more", "last"):
            raise ValueError("dp_loss_backward: accumulate is None, 'first', 'more' or 'last'")
        if accumulate is not None and not masked and not logical_batch:
            raise ValueError("dp_loss_backward: a micro-batch pass needs logical_batch (or expected_batch)")
        if self.norm not in ("group", "frozen"):
            raise _lib.PrimiaError("DP-SGD needs per-sample independent norm layers: ResNet18Engine(norm='group') or "
                                   "norm='frozen' (BatchNorm with fixed statistics)")
        m = int(views)
        if m < 1 or self.N % m:
            raise ValueError(f"dp_loss_backward: views = {views} does not cut the engine's {self.N} slots into records")
        N, nc, dev = self.N, self.spec.num_classes, self.device
        R = N // m      # a sample is a record of one view
        # per-slot loss gradients: softmax - onehot (xent gives them divided by the batch size), over the record's m views
        if self.class_weight is not None:   # w[y_n] / m * (softmax - onehot), zeros on padded rows: one launch, no scale
            call("primia_xent_dp_weighted", self.logits, target, self.class_weight, 1.0 / m, self.loss, self.dlogits, N, nc)
        elif masked:    # softmax - onehot on valid rows, zeros on padded ones; the loss is the mean over the valid rows
            call("primia_xent_hard_masked", self.logits, target, self.loss, self.dlogits, N, nc)
            if m > 1:
                call("primia_scale", self.dlogits, self.dlogits.numel(), 1.0 / m)
        else:
            call("primia_xent_hard", self.logits, target, None, self.loss, self.dlogits, N, nc)
            call("primia_scale", self.dlogits, self.dlogits.numel(), float(N) / m)
        self.dp = {"wgrads": []}
        try:
            self.backward()
            sq = torch.zeros(R, dtype=torch.float64, device=dev)
            # fc: g_W[n] = dlogits[n]^T feat[n], g_b[n] = dlogits[n]
            ps_fc = torch.empty(N, nc * 512 + nc, dtype=torch.float32, device=dev)
            call("primia_fc_persample_grads", self.feat, self.dlogits, ps_fc, N, 512, nc)
            trace = getattr(self, "dp_trace", None)  # optional {name: cumulative sq norms} for debugging

            def mark(name):
                if trace is not None:
                    trace[name] = sq.clone()

            call("primia_record_sqnorm", ps_fc, N, nc * 512 + nc, m, sq)
            mark("fc")
            if trace is None:   # all 40 per-slot affine gradients in one launch
                if self._sqnorm_many is None:
                    xs = [tt.data_ptr() for pair in self.ps_affine.values() for tt in pair]
                    ws_ = [tt.shape[1] for pair in self.ps_affine.values() for tt in pair]
                    self._sqnorm_many = (torch.tensor(xs, dtype=torch.int64, device=dev),
                                         torch.tensor(ws_, dtype=torch.int32, device=dev), len(xs))
                call("primia_record_sqnorm_many", self._sqnorm_many[0], self._sqnorm_many[1], self._sqnorm_many[2], N, m, sq)
            else:
                for b, (psg, psb) in self.ps_affine.items():
                    call("primia_record_sqnorm", psg, N, psg.shape[1], m, sq)
                    call("primia_record_sqnorm", psb, N, psb.shape[1], m, sq)
                    mark(b)
            # layers whose per-sample gradient tiles are small enough to KEEP (the stem, layer1's 64 -> 64 convs): the
            # norm pass stores them and the clipped sum is a weighted reduce — no row scaling of dy, no second pass.
            # The kept-tile forms are per sample: records of several views run the two-pass form on every layer
            kept = self._dp_keep_buffers() if m == 1 else {}
            for name, x, dy in self.dp["wgrads"]:
                self._dp_norm_pass(name, x, dy, sq, kept.get(name), m)
                mark(name)
            # one clip factor per record (record r's target is slot r * m's), then one per slot for the clipped sums
            clip = torch.empty(R, dtype=torch.float32, device=dev)
            target_r = None if not masked else target if m == 1 else target[::m].contiguous()
            adaptive = self._root.dp_clip
            if adaptive is not None:    # C from the device word; the step's counts start over on its first (or only) pass
                adaptive.factors(sq, target_r, clip, R, overwrite=accumulate in (None, "first"))
            elif masked:
                call("primia_dp_clip_factors_masked", sq, target_r, clip, R, float(max_grad_norm))
            else:
                call("primia_dp_clip_factors", sq, clip, R, float(max_grad_norm))
            clip_slots = clip
            if m > 1:
                clip_slots = torch.empty(N, dtype=torch.float32, device=dev)
                call("primia_dp_expand_clip", clip, clip_slots, N, m)
            self._dp_clipped_sums(clip_slots, ps_fc, kept)
        finally:
            if getattr(self, "dp_keep_operands", False):      # tests: the (layer, x, dy) triples the norm pass walked
                self.dp_operands = list(self.dp["wgrads"])
            self.dp = None
        return self._dp_tail(sq, clip, adaptive, R, masked, expected_batch, accumulate, logical_batch, max_grad_norm,
                             noise_multiplier, noise, generator)

    def _dp_norm_pass(self, name, x, dy, sq, keep, m):
        """sq[r] += ||record r's gradient of conv `name`||^2.  Three forms: the one that also keeps every sample's tile
        (`keep`: the layer's buffer of _dp_keep_buffers), conv1's halo kernel on the padded input — one block per record,
        where the constructor found the shape served — and the generic record form.  An error of any of them is the
        caller's: none stands in for another."""
        c, N, S = self.convs[name], self.N, self.spec.input_size
        halo, x_stem = c.dp_norm
        if x_stem is not None:      # conv1: the input copy the form chosen for it reads
            x = x_stem
        if keep is not None and name == "conv1":
            call("primia_stem_conv_wgrad_persample_sqnorm_keep", x, dy, sq, keep, keep.numel() * 4, N, S, S, self.dt)
        elif keep is not None:
            call("primia_conv2d_wgrad_persample_sqnorm_keep", c.desc, x, dy, sq, keep, keep.numel() * 4, self.dt)
        elif halo:
            call("primia_stem_conv_wgrad_record_sqnorm", x, dy, sq, N, S, S, m, self.dt)
        else:
            call("primia_conv2d_wgrad_record_sqnorm", c.desc, x, dy, sq, m, self.dt)

    def _dp_clipped_sums(self, clip, ps_fc, kept):
        """grads = sum_n clip[n] g_n over the N slots of a DP-SGD pass (self.dp holds the backward pass's operands): the
        rows of dy scaled and the batched weight gradient, the weighted reduce of the `kept` layers' tiles, the weighted
        column sums of the per-sample affine and fc gradients."""
        N, nc, dev = self.N, self.spec.num_classes, self.device
        # every dy of a layer whose tiles are not kept, scaled by the clip factors in ONE launch (a dozen tensors)
        to_scale = [dy for name, _, dy in self.dp["wgrads"] if name not in kept]
        many = 0 < len(to_scale) <= 16
        if many:
            key = tuple(tt.data_ptr() for tt in to_scale)
            if self._scale_many is None or self._scale_many[0] != key:
                import ctypes

                self._scale_many = (key, (ctypes.c_void_p * len(key))(*key),
                                    (ctypes.c_int64 * len(key))(*[tt.numel() // N for tt in to_scale]))
            call("primia_scale_rows_many", self._scale_many[1], self._scale_many[2], len(key), clip, N, self.dt)
        self._wg_seen = {}
        for name, x, dy in self.dp["wgrads"]:
            if name in kept:
                c = self.convs[name]
                if name == "conv1":
                    call("primia_stem_conv_wgrad_clipped_sum", kept[name], clip, c.acc, N)
                else:
                    call("primia_conv_wgrad_clipped_sum", c.desc, kept[name], clip, c.acc, self.dt)
                continue
            if not many:
                call("primia_scale_rows", dy, clip, N, dy.numel() // N, self.dt)
            # the clipped SUM is an ordinary batched weight gradient, issued as the plain backward pass issues it: atomic-free
            # kernels, pairs and groups once their last dy is scaled, and for the stem the halo kernel on the padded input
            # (118 us instead of 444 us for the per-tap one)
            self._issue_wgrad(name, x, dy)
        self._finalize_wgrads()
        # clipped sums of the per-sample affine gradients: all 40 (dgamma, dbeta) pairs in ONE launch
        if self._colsum_many is None:
            xs, outs, ws_ = [], [], []
            for b, (psg, psb) in self.ps_affine.items():
                xs += [psg.data_ptr(), psb.data_ptr()]
                outs += [self._gviews[b + ".weight"].data_ptr(), self._gviews[b + ".bias"].data_ptr()]
                ws_ += [psg.shape[1], psb.shape[1]]
            self._colsum_many = (torch.tensor(xs, dtype=torch.int64, device=dev),
                                 torch.tensor(outs, dtype=torch.int64, device=dev),
                                 torch.tensor(ws_, dtype=torch.int32, device=dev), len(xs), max(ws_))
        xs_d, outs_d, ws_d, cnt, mw = self._colsum_many
        call("primia_weighted_colsum_many", xs_d, clip, outs_d, ws_d, cnt, mw, N)
        call("primia_weighted_colsum", ps_fc[:, :nc * 512].contiguous(), clip, self._gviews["fc.weight"].view(-1), N,
             nc * 512)
        call("primia_weighted_colsum", ps_fc[:, nc * 512:].contiguous(), clip, self._gviews["fc.bias"], N, nc)

    def _dp_tail(self, sq, clip, adaptive, units, masked, expected_batch, accumulate, logical_batch, max_grad_norm,
                 noise_multiplier, noise, generator):
        """The end of dp_loss_backward once `grads` holds the pass's clipped sum: accumulate, or noise and the division
        by B — in samples, or in records (`units` of this engine) under augmentation multiplicity."""
        dev = self.device
        self.dp_stats = {"sq_norms": sq, "clip": clip}
        if adaptive is not None:        # (tests: the raw count is private, never printed or saved)
            self.dp_stats["counts"] = adaptive.counts
        if accumulate in ("first", "more"):
            call("primia_dp_accumulate", self.dp_acc, self.grads, self.P, 1 if accumulate == "first" else 0)
            return self.loss
        acc = self.dp_acc if accumulate == "last" else None
        batch = float(expected_batch) if masked else (units if acc is None else int(logical_batch))
        inv_batch = 1.0 / batch
        if adaptive is not None:
            return self._dp_adaptive_tail(adaptive, acc, batch, inv_batch, noise_multiplier, noise, generator)
        sigma = float(noise_multiplier * max_grad_norm)
        if noise is None and generator is None and self._root.dp_noise is not None:
            # the ROOT's stream, whichever sibling runs the step: a halved or ragged batch advances the one counter
            self._root.dp_noise.add_to(self.grads, self.P, sigma, inv_batch, acc=acc)
        else:
            if noise is None:
                noise = torch.randn(self.P, dtype=torch.float32, device=dev, generator=generator)
            if acc is None:
                call("primia_dp_add_noise", self.grads, noise, self.P, sigma, inv_batch)
            else:
                call("primia_dp_add_noise_acc", self.grads, acc, noise, self.P, sigma, inv_batch)
        return self.loss

    def _dp_adaptive_tail(self, adaptive, acc, batch, inv_batch, z, noise, generator):
        """The end of a logical DP-SGD step under an adaptive clipping norm (engine.dp_clip): noise z_delta * C on the
        clipped sum — C read on the device, z_delta paying for the count's release so that the step as a whole is a
        Gaussian mechanism with multiplier z — then the update of C on the step's counts, once per logical step.  The
        count's draw is the block right after the gradient's: one counter advance of blocks(P) + 1.  Host-supplied noise
        has P + 1 elements, the last one the count's."""
        dev, P = self.device, self.P
        nm = adaptive.noise_multiplier(z, batch)
        stream = self._root.dp_noise
        if noise is None and generator is None and stream is not None:
            blocks = query("primia_dp_noise_blocks", P)
            call("primia_dp_noise_add_dev", *stream.key_words, stream.nonce, stream.counter, 0, self.grads, acc, P,
                 adaptive.norm, nm, inv_batch)
            adaptive.update(batch, noise=stream, block_offset=blocks)
            call("primia_u64_add", stream.counter, blocks + 1)
        else:
            if noise is None:
                noise = torch.randn(P + 1, dtype=torch.float32, device=dev, generator=generator)
            if noise.numel() != P + 1:
                raise ValueError(f"dp_loss_backward: with an adaptive clipping norm the noise has P + 1 = {P + 1} elements "
                                 f"(the last one is the count's), got {noise.numel()}")
            call("primia_dp_add_noise_dev", self.grads, acc, noise, P, adaptive.norm, nm, inv_batch)
            adaptive.update(batch, z0=noise[P:])
        return self.loss

    dp_keep = True

    def _dp_keep_buffers(self):
        """{conv name: fp32 buffer} for the layers whose per-sample tiles the DP-SGD norm pass keeps (built once)."""
        if self._dp_keep is None:
            self._dp_keep = {}
            if self.dp_keep and self.dtype == torch.bfloat16:
                for c in self.spec.convs:
                    if c.name == "conv1":
                        S = self.spec.input_size
                        n = query("primia_stem_conv_wgrad_persample_slab_bytes", self.N, S, S) if self.x0p is not None else 0
                    else:
                        n = query("primia_conv_wgrad_persample_slab_bytes", self.convs[c.name].desc, self.dt)
                    if n > 0:
                        self._dp_keep[c.name] = torch.empty(n // 4, dtype=torch.float32, device=self.device)
        return self._dp_keep

    # ------------------------------------------------------------------------------------------
    # optimizer
    # ------------------------------------------------------------------------------------------
    def zero_grad(self):
        self._grads_pending = False
        self.grads.zero_()

    def note_replayed_steps(self, n):
        """Training steps that ran as hipGraph replays: advance the host-side counters forward() would have advanced."""
        if self.norm != "frozen":        # (frozen statistics: no batch is ever tracked)
            for b in self.num_batches_tracked:
                self.num_batches_tracked[b] += int(n)
        if self.opt_state is not None:
            self.opt_steps += int(n)

    def reset_optimizer(self):
        """The reference re-creates its optimizers at every FedAvg sync (utils.py:1131-1145,1208-1218)."""
        self.opt_state = None
        self.opt_steps = 0

    def sgd_step(self, lr, weight_decay=0.0, hyper=None):
        """`hyper`: an fp32 [8] device tensor written by primia_opt_hyper_set — the step then reads lr / weight_decay
        from it on the device (the *_dev entry points: what a captured graph of the step replays) and ignores the two
        arguments."""
        if self._grads_pending:
            fus, rest, rb, rl, nr = self._sgd_tail_plan()
            self._grads_pending = False
            if hyper is None:
                call("primia_conv_sgd_step_many", fus["descs"], fus["creal"], fus["acc"], fus["gw"], fus["w"], fus["wf"],
                     fus["wd"], fus["n"], float(lr), float(weight_decay), self.dt)
            else:
                call("primia_conv_sgd_step_many_dev", fus["descs"], fus["creal"], fus["acc"], fus["gw"], fus["w"],
                     fus["wf"], fus["wd"], fus["n"], hyper, self.dt)
            if rest is not None:
                call("primia_conv_wgrad_finalize_many", rest["descs"], rest["creal"], rest["acc"], rest["gw"], rest["n"])
            if hyper is None:
                call("primia_sgd_step_ranges", self.flat, self._grads, rb, rl, nr, float(lr), float(weight_decay))
            else:
                call("primia_sgd_step_ranges_dev", self.flat, self._grads, rb, rl, nr, hyper)
            if rest is not None:
                call("primia_conv_weight_prepare_many", rest["descs"], rest["creal"], rest["w"], rest["wf"], rest["wd"],
                     rest["n"], self.dt)
            return
        if hyper is None:
            call("primia_sgd_step", self.flat, self.grads, self.P, float(lr), float(weight_decay))
        else:
            call("primia_sgd_step_dev", self.flat, self.grads, self.P, hyper)
        self.refresh_weights()

    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, hyper=None):
        """`hyper`: as in sgd_step; it must hold this step's bias corrections (primia_opt_hyper_set with step =
        opt_steps + 1, the count this call advances to)."""
        self.materialize_grads()
        if self.opt_state is None:
            self.opt_state = (torch.zeros_like(self.grads), torch.zeros_like(self.grads))
            self.opt_steps = 0
        self.opt_steps += 1
        m, v = self.opt_state
        if hyper is None:
            call("primia_adam_step", self.flat, self.grads, m, v, self.P, float(lr), float(betas[0]), float(betas[1]),
                 float(eps), float(weight_decay), self.opt_steps)
        else:
            call("primia_adam_step_dev", self.flat, self.grads, m, v, self.P, hyper)
        self.refresh_weights()

    def train_step(self, x_nchw, target, lr, weight_decay=0.0, soft=False):
        """forward + loss + backward + SGD: the body of the reference's per-batch loop."""
        self.forward(x_nchw)
        self.loss_backward(target, soft=soft)
        self.sgd_step(lr, weight_decay)
        return self.loss
