"""The definition of the secret-shared GroupNorm (the reference has none; tests/secure_batch_nets.py's oracle_forward places it
at every norm site for norm="group"), the float64 plaintext reference of a GroupNorm network, CPU dealers and networks shared
by tests/test_secure_groupnorm_host.py and tests/test_gpu_secure_groupnorm.py: a module of helpers, not of tests.
Everything is composed from oracle.secure_oracle's own functions; nothing under oracle/ knows about GroupNorm."""
import hashlib

import numpy as np
import torch

from oracle import secure_oracle as S
from oracle import train_oracle as O
from primia_amd import resnet_spec
from tests.cpu_standins import chacha20_words

I64, U64 = np.int64, np.uint64
GROUPS = 32
EPS = 1e-5
VAR_DOMAIN = (0.05, 16.0)      # where the reference's Newton iteration approximates v^-1/2 to under 1 %
# Bounds of the tests, each TWICE what the CPU composition of OracleContext methods measured against float64 (the GPU is
# held bit-identical to that composition, so the CPU figure is the measurement):
#   LAYER_TOL   oracle_group_norm at pf = 6 on the [2, 64, 6, 6] input of tests/test_secure_groupnorm_host.py (group
#               variances 0.41 to 3.57) against F.group_norm: max |error| 4.98e-4, 5.00e-4, 4.99e-4 under three dealer seeds.
#   GROUP_TOL   oracle_forward(norm="group") at pf = 3 of group_resnet18(32, 520) on three N(0, 1) images (seed 521) on
#               ChaChaDealer(53) -- the host twin of Dealer(seed=53) -- against plaintext_group_logits: max |error| per image
#               0.00619, 0.00398, 0.00379 (group variances of the float64 forward: 0.063 to 13.02).
LAYER_TOL = 2 * 5.0e-4
GROUP_TOL = 2 * 0.0062


def _row_mean(x, m):
    """AST.mean over the last axis of one share (additive_shared.py:719-729): wrapping sum, truncating division."""
    s = np.ascontiguousarray(x).view(U64).sum(axis=-1, dtype=U64).view(I64)
    return S.trunc_div(s, m)


def oracle_group_norm(ctx, x, weight, bias, groups=GROUPS):
    """GroupNorm(groups, C) of the shares x [B, C, H, W] on an OracleContext -- THE definition of the layer.
    The element order inside each triple is part of it: it decides which dealer word meets which element."""
    B, C, H, W = x[0].shape
    assert C % groups == 0
    R, m = B * groups, (C // groups) * H * W
    X = [np.ascontiguousarray(x[j]).reshape(R, m) for j in range(2)]
    mean = [_row_mean(X[j], m) for j in range(2)]                                   # 1
    Xc = [S.rsub(X[j], mean[j][:, None]) for j in range(2)]                         # 2
    Sq = ctx.fpt_mul(Xc, Xc)                                                        # 3  ("mul", (R, m), (R, m))
    var = [_row_mean(Sq[j], m) for j in range(2)]                                   # 4
    eps_q = int(S.fix_encode(EPS, ctx.base, ctx.pf))
    v = ctx.sub_public_scalar(var, -eps_q)                                          # 5  (always: one const_mask(1))
    inv = ctx.reciprocal_newton(v)                                                  # 6
    N = ctx.fpt_mul(inv, [np.ascontiguousarray(Xc[j].T) for j in range(2)])         # 7  ("mul", (R,), (m, R))
    n = [np.ascontiguousarray(N[j].T).reshape(B, C, H, W) for j in range(2)]
    rows = [np.ascontiguousarray(np.transpose(n[j], (1, 0, 2, 3)).reshape(C, -1).T) for j in range(2)]      # 8
    result = ctx.add(ctx.fpt_mul(rows, weight), bias)
    return [np.ascontiguousarray(np.transpose(result[j].T.reshape(C, B, H, W), (1, 0, 2, 3))) for j in range(2)]


def default_blocks():
    return [(f"layer{li}.{bi}", (2 if (li > 1 and bi == 0) else 1)) for li in range(1, 5) for bi in range(2)]


def quantise(v, pf):
    return torch.from_numpy(S.fix_encode(v.numpy(), 10, pf).astype(np.float64) / 10 ** pf)


def plaintext_group_logits(sd, images, pf, size, pooling="max"):
    """oracle.train_oracle.forward(training=False) in float64 on the fixed-point-rounded parameters and images; with no
    running_mean in the state dict that forward takes its F.group_norm(x, 32, w, b, 1e-5) branch."""
    sd64 = {k: (quantise(v, pf) if v.is_floating_point() else v) for k, v in sd.items()}
    assert "bn1.running_mean" not in sd64
    with torch.no_grad():
        return O.forward(sd64, quantise(images, pf), training=False, pooling=pooling, input_size=size).numpy()


def plain_group_forward(sd, images, blocks, pf, pooling="max", variances=None):
    """The same float64 forward written out for a network given as (state dict, blocks) -- the mini network is not a
    ResNet-18 -- which also hands every norm site's (biased) group variances to `variances` (a list), the quantity the
    Newton domain is about."""
    F = torch.nn.functional
    p = {k: quantise(v, pf) for k, v in sd.items() if v.is_floating_point()}

    def gn(t, n):
        if variances is not None:
            variances.append(t.reshape(t.shape[0], GROUPS, -1).var(dim=2, unbiased=False).reshape(-1))
        return F.group_norm(t, GROUPS, p[n + ".weight"], p[n + ".bias"], EPS)

    with torch.no_grad():
        x = F.relu(gn(F.conv2d(quantise(images, pf), p["conv1.weight"], stride=2, padding=3), "bn1"))
        x = F.max_pool2d(x, 3, 2, 1) if pooling == "max" else F.avg_pool2d(x, 3, 2, 1)
        for prefix, stride in blocks:
            out = F.relu(gn(F.conv2d(x, p[prefix + ".conv1.weight"], stride=stride, padding=1), prefix + ".bn1"))
            out = gn(F.conv2d(out, p[prefix + ".conv2.weight"], stride=1, padding=1), prefix + ".bn2")
            if (prefix + ".downsample.0.weight") in p:
                x = gn(F.conv2d(x, p[prefix + ".downsample.0.weight"], stride=stride), prefix + ".downsample.1")
            x = F.relu(out + x)
        x = x.mean(dim=(2, 3))
        return (x @ p["fc.weight"].t() + p["fc.bias"]).numpy()


# ---- networks -------------------------------------------------------------------------------------------------------------
def draw_gn(sd, name, c, gen):
    """A GroupNorm whose affine part is not the identity: weight U[0.5, 1.5), bias N(0, 0.1)."""
    sd[name + ".weight"] = torch.rand(c, generator=gen) + 0.5
    sd[name + ".bias"] = torch.randn(c, generator=gen) * 0.1


def group_resnet18(size, seed, pooling="max"):
    """The 8-block GroupNorm ResNet-18 for `size` x `size` RGB images and 3 classes from the reference's initialisation
    under a fixed seed, every norm's affine part redrawn; no running statistics.  layer4's convolutions are scaled by 1.5:
    at 32 x 32 its maps are 1 x 1, a group is 16 values, and the sample variance of 16 values of the plain initialisation
    falls below the Newton domain's 0.05 for about one group in a thousand (0.026 to 0.048 over twenty seeds); a GroupNorm
    takes the factor back out, so nothing downstream changes scale."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        sd = resnet_spec.init_state_dict(resnet_spec.resnet18_spec(3, 3, size, pooling), "group")
    assert not any(k.endswith("running_mean") or k.endswith("num_batches_tracked") for k in sd)
    for k in [k for k in sd if k.startswith("layer4.") and sd[k].dim() == 4]:
        sd[k] = sd[k] * 1.5
    gen = torch.Generator().manual_seed(seed + 1)
    for k in [k for k in sd if k.endswith(".weight") and sd[k].dim() == 1]:
        draw_gn(sd, k[:-len(".weight")], sd[k].numel(), gen)
    return sd


def group_mini(gen):
    """tests/secure_batch_nets.py's mini network (stem, an identity block, a projection block) with GroupNorm."""
    sd = {}

    def conv(name, o, i, k):
        sd[name + ".weight"] = torch.randn(o, i, k, k, generator=gen) * (1.0 / (i * k * k) ** 0.5)

    conv("conv1", 64, 3, 7)
    draw_gn(sd, "bn1", 64, gen)
    for p, cin, cout in (("layer1.0", 64, 64), ("layer2.0", 64, 128)):
        conv(p + ".conv1", cout, cin, 3)
        draw_gn(sd, p + ".bn1", cout, gen)
        conv(p + ".conv2", cout, cout, 3)
        draw_gn(sd, p + ".bn2", cout, gen)
    conv("layer2.0.downsample.0", 128, 64, 1)
    draw_gn(sd, "layer2.0.downsample.1", 128, gen)
    sd["fc.weight"] = torch.randn(3, 128, generator=gen) * 0.1
    sd["fc.bias"] = torch.randn(3, generator=gen) * 0.1
    return sd


# ---- CPU dealers ----------------------------------------------------------------------------------------------------------
class RecordingDealer:
    """A crypto provider on the host for OracleContext: uniform int64 primitives from a seeded numpy generator, every request
    recorded as (kind, args) in the form of primia_amd.secure.Dealer.requests (without the owner, which an OracleContext
    does not pass on)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.requests = []

    def _rand(self, shape):
        return self.rng.integers(-2 ** 63, 2 ** 63 - 1, size=tuple(shape), dtype=I64, endpoint=True)

    def triple(self, op, xshape, yshape):
        self.requests.append(("triple", (op, tuple(xshape), tuple(yshape))))
        a = [self._rand(xshape), self._rand(xshape)]
        b = [self._rand(yshape), self._rand(yshape)]
        c = S.rmul(S.radd(*a), S.radd(*b)) if op == "mul" else S.rmatmul(S.radd(*a), S.radd(*b))
        c0 = self._rand(c.shape)
        return [(a[0], b[0], c0), (a[1], b[1], S.rsub(c, c0))]

    def dif_keys(self, n):
        self.requests.append(("dif_keys", (n,)))
        alpha = self.rng.integers(0, 2 ** 32, size=n, dtype=U64)
        s0 = self.rng.integers(0, 2 ** 64 - 1, size=(2, 2, n), dtype=U64, endpoint=True)
        s0[:, 0] &= U64(2 ** 63 - 1)
        r = self.rng.integers(0, 2 ** 32, size=n, dtype=U64)
        _, keys = S.dif_keygen(alpha, s0)
        return list(S.split_alpha(alpha, r)), keys

    def const_mask(self, *shape):
        self.requests.append(("const_mask", tuple(shape)))
        return self._rand(shape)


class ChaChaDealer(RecordingDealer):
    """primia_amd.secure.Dealer(device, seed=seed) on the host: the same ChaCha20 keystream under the same debug key, drawn in
    the same order (triple: a0, a1, b0, b1, c0; comparison keys: alpha, both seeds, alpha's mask, then
    primia_fss_alpha_split's masking), so an OracleContext on this dealer computes, bit for bit, what a SecureContext on
    that Dealer computes -- the GPU tests hold the two equal through the recorded log; this class lets the host MEASURE the
    composition on the very primitives the GPU test will draw."""

    def __init__(self, seed):
        self.requests = []
        raw = hashlib.sha256(b"primia-dealer-debug-seed:%d" % int(seed)).digest() + bytes(8)
        self._key = [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(4)] + [int.from_bytes(raw[32:40], "little")]
        self._block = 0

    def _rand(self, shape):
        n = int(np.prod(shape, dtype=np.int64)) if len(tuple(shape)) else 1
        out = chacha20_words(self._key, self._block, n).view(I64).reshape(tuple(shape))
        self._block += (n + 7) // 8
        return out

    def dif_keys(self, n):
        self.requests.append(("dif_keys", (n,)))
        m32 = U64(0xFFFFFFFF)
        alpha = self._rand((n,)).view(U64) & m32
        s0 = self._rand((2, 2, n)).view(U64).copy()
        s0[:, 0] &= U64(2 ** 63 - 1)
        r = self._rand((n,)).view(U64) & m32
        _, keys = S.dif_keygen(alpha, s0)
        return list(S.split_alpha(alpha, r)), keys


class ScheduleContext(S.OracleContext):
    """An OracleContext for a schedule-only walk: comparisons request their keys and return shares of zero instead of
    evaluating 32 SHA-512 levels per element (the bits are wrong; the REQUESTS, which depend on shapes alone, are not)."""

    def le(self, x1, x2):
        self.dealer.requests.append(("dif_keys", (x1[0].size,)))
        return [np.zeros(x1[0].shape, I64), np.zeros(x1[0].shape, I64)]
