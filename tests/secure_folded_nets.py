"""The definition of a norm site folded by the model owner (the reference has none: its encrypted BatchNorm runs Newton's
iteration on shares of running_var), the forward composed from it, an independent float64 restatement of the fold, networks
whose running variances leave the Newton domain, the float64 plaintext reference and the host twin of a 64-bit device dealer,
shared by tests/test_secure_folded_host.py and tests/test_gpu_secure_folded.py: a module of helpers, not of tests.
Everything is composed from oracle.secure_oracle's own functions; nothing under oracle/ knows about folding."""
import numpy as np
import torch

from oracle import secure_oracle as S
from oracle import train_oracle as O
from tests import fss_wide_ref as W
from tests.secure_avgpool_nets import oracle_avg_pool
from tests.secure_batch_nets import mini_resnet, resnet18
from tests.secure_groupnorm_nets import ChaChaDealer

I64, U64 = np.int64, np.uint64
EPS = 1e-5
# running variances set channel by channel: all finite under the reference's Newton iteration (x0 = (21 - v) / 20, 79 steps),
# which is 15 % off at 1e-3, 1.6 % at 1e-2, under 1 % from 0.05 to 16, and returns -0.2 and -0.1826 -- the wrong sign -- at 25
# and 30
WIDE_VARIANCES = (1e-3, 1e-2, 0.3, 1.0, 4.0, 25.0, 30.0)
NARROW_VARIANCES = (0.3, 0.5, 1.0, 2.0, 4.0)
# Bound of the accuracy tests: TWICE the largest max |folded secure logits - float64 plaintext logits| the CPU composition
# (oracle_folded_forward on WideChaChaDealer, a host dealer with 64-bit comparison keys) measured at pf = 6 with 64-bit
# comparisons on wide_resnet18(32, 720) and two N(0, 1) images (seed 721): 3.18e-5, 1.87e-5, 3.56e-5 under dealer seeds 1, 2, 3
# (tests/test_secure_folded_host.py prints them; logits of 1.0 to 1.7).  The narrow network (seed 730) measured 8.6e-6 under
# seed 1; the reference's form on the wide checkpoint 8.1e6 (its logits are in the millions).
FOLDED_TOL = 2 * 3.57e-5


def oracle_affine_eval(ctx, x, scale, shift):
    """x * scale + shift per channel on the shares x [B, C, H, W] on an OracleContext -- THE definition of a folded norm site
    (DESIGN.md §4): exactly the affine tail of OracleContext.batch_norm_eval.  One triple ("mul", (B*H*W, C), (C,)); the
    element order inside it is part of the definition."""
    B, C, H, W = x[0].shape
    rows = [np.ascontiguousarray(np.transpose(x[j], (1, 0, 2, 3)).reshape(C, -1).T) for j in range(2)]
    result = ctx.add(ctx.fpt_mul(rows, scale), shift)
    return [np.ascontiguousarray(np.transpose(result[j].T.reshape(C, B, H, W), (1, 0, 2, 3))) for j in range(2)]


def fold64(sd, eps=EPS):
    """The fold restated independently of primia_amd.secure.fold_batch_norm: name -> float32 tensor, <prefix>.scale =
    gamma / sqrt(running_var + eps) and <prefix>.shift = beta - running_mean * scale in float64 from the float32 values,
    in place of the BatchNorm tensors; conv and fc tensors as they are."""
    out = {}
    for k, v in sd.items():
        if k.endswith((".running_mean", ".running_var", ".num_batches_tracked")):
            continue
        p = k.rsplit(".", 1)[0]
        if (p + ".running_var") not in sd:
            out[k] = v
            continue
        g, b, m, var = (np.asarray(sd[p + s].numpy(), np.float64) for s in (".weight", ".bias", ".running_mean", ".running_var"))
        s = g / np.sqrt(var + eps)
        if k.endswith(".weight"):
            out[p + ".scale"] = torch.from_numpy(s.astype(np.float32))
        else:
            out[p + ".shift"] = torch.from_numpy((b - m * s).astype(np.float32))
    return out


def oracle_folded_forward(ctx, state_dict, images, blocks=None, pooling="max"):
    """The secure forward of images [B, C, S, S] on a FOLDED state dict (float32 numpy arrays), composed from OracleContext's
    own methods, oracle_avg_pool and oracle_affine_eval: tests/secure_batch_nets.py's oracle_forward with every norm site an
    oracle_affine_eval and nothing hoisted.  The model is shared in share_order (no buffers: the dict's own order)."""
    p = {}
    for k in S.share_order(list(state_dict.keys())):
        p[k] = ctx.share(S.fix_encode(state_dict[k], ctx.base, ctx.pf))
    if blocks is None:
        blocks = [(f"layer{li}.{bi}", (2 if (li > 1 and bi == 0) else 1)) for li in range(1, 5) for bi in range(2)]
    x = ctx.share(S.fix_encode(images, ctx.base, ctx.pf))

    def bn(t, prefix):
        return oracle_affine_eval(ctx, t, p[prefix + ".scale"], p[prefix + ".shift"])

    x = bn(ctx.conv2d(x, p["conv1.weight"], 2, 3), "bn1")
    if pooling == "max":
        x = ctx.relu(ctx.max_pool2d_3x3s2(x))
    else:
        x = oracle_avg_pool(ctx.relu(x), 3, 2, 1)
    for prefix, stride in blocks:
        identity = x
        out = ctx.conv2d(x, p[prefix + ".conv1.weight"], stride, 1)
        out = ctx.relu(bn(out, prefix + ".bn1"))
        out = ctx.conv2d(out, p[prefix + ".conv2.weight"], 1, 1)
        out = bn(out, prefix + ".bn2")
        if (prefix + ".downsample.0.weight") in p:
            identity = ctx.conv2d(x, p[prefix + ".downsample.0.weight"], stride, 0)
            identity = bn(identity, prefix + ".downsample.1")
        x = ctx.relu(ctx.add(out, identity))
    x = ctx.avg_pool2d(x, x[0].shape[-1])
    B = x[0].shape[0]
    x = [t.reshape(B, -1) for t in x]
    return ctx.linear(x, p["fc.weight"], p["fc.bias"])


# ---- networks -------------------------------------------------------------------------------------------------------------
def conv_of(norm):
    """The convolution whose output a norm site normalises."""
    if norm == "bn1":
        return "conv1"
    head, last = norm.rsplit(".", 1)
    return head + (".0" if last == "1" else ".conv" + last[-1])      # <block>.downsample.1 / <block>.bn1 / <block>.bn2


def set_variances(sd, values):
    """Every running_var of a BatchNorm network set channel by channel from `values` (site k starts at values[k % len]), the
    rows of the convolution in front of the site and its running_mean scaled by sqrt(var / old var): the activations the
    site sees have about the variance its statistics record, as a trained checkpoint's do, and the normalised output keeps
    its scale whatever the variance."""
    sd = dict(sd)
    for k, name in enumerate(n[:-len(".running_var")] for n in list(sd) if n.endswith(".running_var")):
        c = sd[name + ".running_var"].numel()
        var = torch.tensor([values[(k + i) % len(values)] for i in range(c)], dtype=torch.float32)
        f = torch.sqrt(var / sd[name + ".running_var"])
        conv = conv_of(name) + ".weight"
        sd[conv] = sd[conv] * f.view(-1, 1, 1, 1)
        sd[name + ".running_mean"] = sd[name + ".running_mean"] * f
        sd[name + ".running_var"] = var
    return sd


def wide_resnet18(size, seed):
    """tests/secure_batch_nets.py's 8-block ResNet-18 with running variances from 1e-3 to 30, most of them outside the Newton
    domain: a checkpoint the reference's encrypted BatchNorm does not decode to."""
    return set_variances(resnet18(size, seed), WIDE_VARIANCES)


def narrow_resnet18(size, seed):
    """The same network with every running variance inside [0.3, 4]."""
    return set_variances(resnet18(size, seed), NARROW_VARIANCES)


def wide_mini(gen):
    """The mini network (stem, an identity block, a projection block) with the wide variances."""
    return set_variances(mini_resnet(gen), WIDE_VARIANCES)


def quantise(v, pf):
    return torch.from_numpy(S.fix_encode(v.numpy(), 10, pf).astype(np.float64) / 10 ** pf)


def plaintext_logits(sd, images, pf, size, pooling="max"):
    """oracle.train_oracle.forward(training=False) -- F.batch_norm with eps = 1e-5 -- in float64 on what the secure forward
    decodes: the fixed-point-rounded convolution / fc tensors and images; the BatchNorm tensors, which the folded form never
    encodes one by one, at the checkpoint's float32 values."""
    norm = lambda k: k.rsplit(".", 1)[0] + ".running_var" in sd
    sd64 = {k: (v if not v.is_floating_point() else v.double() if norm(k) else quantise(v, pf)) for k, v in sd.items()}
    with torch.no_grad():
        return O.forward(sd64, quantise(images, pf), training=False, pooling=pooling, input_size=size).numpy()


# ---- a host dealer with wide comparison keys ------------------------------------------------------------------------------
class WideChaChaDealer(ChaChaDealer):
    """ChaChaDealer -- the keystream and order of draws of primia_amd.secure.Dealer(device, seed=seed) -- whose comparison keys
    have `bits` levels (alpha and its mask reduced mod 2^bits, as primia_fss_alpha_split_n does).  Not held bit for bit to
    Dealer(seed, fss_bits=bits) by any test: the accuracy bound measured on it is a statistic over dealer seeds."""

    def __init__(self, seed, bits=64):
        super().__init__(seed)
        self.bits = bits

    def dif_keys(self, n):
        self.requests.append(("dif_keys", (n,)))
        alpha = self._rand((n,)).view(U64) & W.width_mask(self.bits)
        s0 = self._rand((2, 2, n)).view(U64).copy()
        s0[:, 0] &= U64(2 ** 63 - 1)
        r = self._rand((n,)).view(U64)
        return list(W.split_alpha(alpha, r, self.bits)), W.dif_keygen(alpha, s0, self.bits)
