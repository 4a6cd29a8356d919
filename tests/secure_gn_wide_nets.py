"""The definition of the WIDE-RANGE secret-shared GroupNorm (SecureContext.group_norm(wide=True), inference.py --wide_norm),
its reciprocal square root, the inputs and the bounds shared by tests/test_secure_gn_wide_host.py,
tests/test_gpu_secure_gn_wide.py and tools/secure_gn_range.py: a module of helpers, not of tests.  Everything is composed
from OracleContext methods, as tests/secure_groupnorm_nets.py composes the default form; nothing under oracle/ changes."""
import contextlib

import numpy as np
import torch

from oracle import secure_oracle as S
from tests import secure_batch_nets
from tests.secure_groupnorm_nets import EPS, GROUPS, _row_mean

I64 = np.int64
S_IT = 10 ** 6        # the scale of the variance and of v^-1/2, whatever the fixed-point scale of the network
X0 = 0.01             # the public first guess: the iteration serves 0 < v < 3 / X0^2 = 30,000
STEPS = 32            # iterates, the locally formed first one included: STEPS - 1 dealer-backed steps
FLOOR = 2             # units of 1 / S_IT added to var + eps, see oracle_group_norm_wide
PF_RANGE = (3, 6)     # below 3, s * s < S_IT; at 16 the products do not fit the ring
VAR_SERVED = (1e-3, 1.2e4)      # the group variances the layer is measured on (tools/secure_gn_range.py)
VAR_SERVED_PF6 = (1e-3, 1e2)    # ... at pf = 6, where the raw square Xc^2 * s^2 is what the ring's headroom limits

# Bounds of the tests, each TWICE what the CPU composition measured against float64 (tools/secure_gn_range.py prints the
# figures; the GPU is held bit-identical to the composition, so the CPU figure is the measurement):
#   WIDE_LAYER_TOL[pf]  oracle_group_norm_wide on wide_layer_input(pf) against F.group_norm, max |error| over dealer seeds
#                       1, 2, 3, the constant group included: pf 3: 0.0156, 0.0156, 0.0278; pf 6: 0.00302, 0.00220, 0.00299.
#   RSQRT_REL_TOL       rsqrt_newton on a geometric grid of 60 variances over VAR_SERVED, max relative error against
#                       v^-1/2 (v the encoded value) under seeds 1, 2, 3: 0.00261, 0.00143, 0.00143 (the iteration runs at S_IT whatever
#                       the pf; the maximum sits at the top of the range, below v = 1 it is under 1e-6).
#   WIDE_NET_TOL        oracle_forward at pf = 3 with the wide layer at every norm site against plaintext_group_logits, per
#                       network of tests/test_gpu_secure_gn_wide.py (figures there).
WIDE_LAYER_TOL = {3: 2 * 0.0278, 6: 2 * 0.00302}
RSQRT_REL_TOL = 2 * 0.00261


def check_pf(pf):
    if not PF_RANGE[0] <= pf <= PF_RANGE[1]:
        raise ValueError(f"the wide-range GroupNorm is defined for {PF_RANGE[0]} <= precision_fractional <= {PF_RANGE[1]}, "
                         f"got {pf}")


def oracle_rsqrt_newton(ctx, v, x0=X0, steps=STEPS):
    """v^-1/2 of shares v at scale S_IT by the UNDAMPED Newton iteration x <- x (3 - v x^2) / 2.  From any
    0 < x0 < sqrt(3 / v) it rises monotonically (1.5x per step while v x^2 << 1, then quadratically) and never overshoots.
    The first iterate needs no dealer: x0 is public, so x1 = 1.5 x0 - v x0^3 / 2 = 1.5 x0 - trunc(v, 2 / x0^3) is formed by
    the parties locally, party 0 holding the constant (the reference forms its x0 = (21 - v) / 20 locally too)."""
    x0_q = int(round(x0 * S_IT))
    first_div = 2 * S_IT ** 3 // x0_q ** 3
    const = [np.array([3 * x0_q // 2], I64), np.array([0], I64)]
    x = ctx.add(ctx.neg(ctx.trunc(v, first_div)), const)
    for _ in range(steps - 1):
        xx = ctx.trunc(ctx.beaver_mul(x, x), S_IT)
        vxx = ctx.trunc(ctx.beaver_mul(v, xx), S_IT)
        y = ctx.neg(ctx.sub_public_scalar(vxx, 3 * S_IT))
        x = ctx.trunc(ctx.beaver_mul(y, x), 2 * S_IT)
    return x


def oracle_group_norm_wide(ctx, x, weight, bias, groups=GROUPS):
    """GroupNorm(groups, C) of the shares x [B, C, H, W] for ANY group variance in (0, 3 / X0^2) -- THE definition of
    SecureContext.group_norm(wide=True).  The element order inside each triple is part of it.
    It differs from oracle_group_norm in the scale of the variance (S_IT, so that at pf = 3 a variance of 1e-3 keeps three
    digits instead of one) and in the iteration (undamped Newton: a reciprocal square root on the whole range, where the
    reference's damped form is one on about [0.05, 16] only).

    FLOOR.  With s*s/S_IT = d, step 3 truncates each share of a square by d and step 4 each share of the row sum by m.  A
    value z shared as (z0, z - z0) has shares of opposite sign (|z| << 2^63), and truncating both toward zero gives
    trunc(z0 / d) + trunc((z - z0) / d) in (z / d - 1, z / d + 1).  So every square reconstructs to more than its true value
    minus one unit, their mean to more than the true mean minus one, and the division by m takes off less than one more: the
    reconstructed variance is above the true one minus 2 units of 1 / S_IT.  FLOOR = 2 keeps v = var + eps + FLOOR above
    the true variance + eps, in particular positive for a constant group (a zero padding image): the undamped iteration
    diverges for v < 0, where the damped one merely stalls."""
    check_pf(ctx.pf)
    B, C, H, W = x[0].shape
    assert C % groups == 0
    R, m = B * groups, (C // groups) * H * W
    s = ctx.scale
    X = [np.ascontiguousarray(x[j]).reshape(R, m) for j in range(2)]
    mean = [_row_mean(X[j], m) for j in range(2)]                                   # 1
    Xc = [S.rsub(X[j], mean[j][:, None]) for j in range(2)]                         # 2
    Sq = ctx.trunc(ctx.beaver_mul(Xc, Xc), s * s // S_IT)                           # 3  ("mul", (R, m), (R, m)); pf 3: by 1
    var = [_row_mean(Sq[j], m) for j in range(2)]                                   # 4  at scale S_IT
    v = ctx.sub_public_scalar(var, -(int(round(EPS * S_IT)) + FLOOR))               # 5  one public constant: eps + floor
    inv = oracle_rsqrt_newton(ctx, v)                                               # 6  at scale S_IT
    N = ctx.trunc(ctx.beaver_mul(inv, [np.ascontiguousarray(Xc[j].T) for j in range(2)]), S_IT)     # 7  ("mul", (R,), (m, R))
    n = [np.ascontiguousarray(N[j].T).reshape(B, C, H, W) for j in range(2)]        #    at scale s
    rows = [np.ascontiguousarray(np.transpose(n[j], (1, 0, 2, 3)).reshape(C, -1).T) for j in range(2)]      # 8
    result = ctx.add(ctx.fpt_mul(rows, weight), bias)
    return [np.ascontiguousarray(np.transpose(result[j].T.reshape(C, B, H, W), (1, 0, 2, 3))) for j in range(2)]


def wide_site_requests(R, m, rows, C, steps=STEPS):
    """What one norm site of the wide form asks a RecordingDealer for, in order."""
    t = lambda xs, ys: ("triple", ("mul", tuple(xs), tuple(ys)))
    step = [t((R,), (R,)), t((R,), (R,)), ("const_mask", (1,)), t((R,), (R,))]
    return [t((R, m), (R, m)), ("const_mask", (1,))] + (steps - 1) * step + [t((R,), (m, R)), t((rows, C), (C,))]


@contextlib.contextmanager
def wide_sites():
    """tests.secure_batch_nets.oracle_forward(norm="group") with oracle_group_norm_wide at every norm site: the forward
    looks the layer up by name, and that file stays as it is."""
    kept = secure_batch_nets.oracle_group_norm
    secure_batch_nets.oracle_group_norm = oracle_group_norm_wide
    try:
        yield
    finally:
        secure_batch_nets.oracle_group_norm = kept


def oracle_forward_wide(ctx, state_dict, images, blocks=None, pooling="max"):
    with wide_sites():
        return secure_batch_nets.oracle_forward(ctx, state_dict, images, blocks, pooling, "group")


def wide_layer_input(pf, seed=700):
    """(x [2, 64, 6, 6], weight, bias, true per-group standard deviations [64]) for the layer tests: the 64 groups' standard
    deviations spread geometrically over the served range of this pf (VAR_SERVED / VAR_SERVED_PF6), group 5 constant."""
    lo, hi = VAR_SERVED if pf < 6 else VAR_SERVED_PF6
    g = torch.Generator().manual_seed(seed)
    std = torch.from_numpy(np.geomspace(np.sqrt(lo) * 1.05, np.sqrt(hi) * 0.95, 64)).float()
    x = torch.randn(64, 72, generator=g)
    x = (x - x.mean(1, keepdim=True)) / x.std(1, unbiased=False, keepdim=True) * std[:, None] + torch.randn(64, 1, generator=g)
    x[5] = 0.75
    w, b = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    return x.reshape(2, 64, 6, 6), w, b, std


def layer_error(fn, pf, seed, x, w, b, dealer=None):
    """(|fn(shares) - float64 F.group_norm| per element [64 groups, 72], float64 group variances [64]) on a RecordingDealer."""
    from tests.secure_groupnorm_nets import RecordingDealer
    enc = lambda t: S.fix_encode(t.numpy(), 10, pf)
    xq, wq, bq = (torch.from_numpy(enc(t).astype(np.float64) / 10 ** pf) for t in (x, w, b))
    ref = torch.nn.functional.group_norm(xq, GROUPS, wq, bq, EPS).numpy()
    ctx = S.OracleContext(dealer or RecordingDealer(seed), 10, pf)
    out = fn(ctx, ctx.share(enc(x)), ctx.share(enc(w)), ctx.share(enc(b)))
    dec = S.radd(out[0], out[1]).astype(np.float64) / 10 ** pf
    B = x.shape[0]
    var = xq.reshape(B * GROUPS, -1).var(dim=1, unbiased=False).numpy()
    return np.abs(dec - ref).reshape(B * GROUPS, -1), var


def rsqrt_values(v, seed=9, x0=X0, steps=STEPS):
    """oracle_rsqrt_newton of the public values v (encoded at S_IT, shared with a random mask), decoded; and the encoded v."""
    from tests.secure_groupnorm_nets import RecordingDealer
    ctx = S.OracleContext(RecordingDealer(seed), 10, 6)
    q = np.round(np.asarray(v, np.float64) * S_IT).astype(I64)
    out = oracle_rsqrt_newton(ctx, ctx.share(q), x0, steps)
    return S.radd(out[0], out[1]).astype(np.float64) / S_IT, q.astype(np.float64) / S_IT


# ---- networks whose group variances leave the default form's window ------------------------------------------------------------
IMAGE_SCALES = (0.15, 1.0, 6.0)      # per image: the stem's group variances scale with the square
CONV_SCALES = {"layer1.0.conv1.weight": 6.0, "layer1.0.conv2.weight": 0.25, "layer2.0.conv1.weight": 5.0}
NET_DEALER_SEED = 57                 # Dealer(seed=57) on the device, ChaChaDealer(57) on the host: the same primitives


def spread_network(sd):
    """`sd` with three convolutions scaled (CONV_SCALES: names that the mini network and the ResNet-18 share).  The GroupNorm
    behind each takes the factor back out, so the model is the same function; its group variances at those sites are not."""
    return {k: (v * CONV_SCALES[k] if k in CONV_SCALES else v) for k, v in sd.items()}


def spread_images(seed=721):
    """Three 32 x 32 images scaled by IMAGE_SCALES."""
    images = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(seed))
    return images * torch.tensor(IMAGE_SCALES).view(3, 1, 1, 1)


def wide_networks():
    """name -> (state dict, blocks) of the two whole-network cases."""
    from tests.secure_batch_nets import MINI_BLOCKS
    from tests.secure_groupnorm_nets import group_mini, group_resnet18
    return {"mini": (spread_network(group_mini(torch.Generator().manual_seed(31))), MINI_BLOCKS),
            "resnet18": (spread_network(group_resnet18(32, 520)), None)}


# oracle_forward_wide at pf = 3 on ChaChaDealer(NET_DEALER_SEED) over spread_images() against plain_group_forward, max |error|
# per image, and the float64 group variances over all sites (measure_network below; tools/secure_gn_range.py --networks prints them):
#   mini:      0.00405, 0.00289, 0.00159; variances 0.0103 to 227.6  (the default form on the same input: 5.0e12, 1.3e13, 3.2e12)
#   resnet18:  0.01259, 0.00350, 0.00425; variances 0.00145 to 271.8
WIDE_NET_TOL = {"mini": 2 * 0.00405, "resnet18": 2 * 0.01259}


def measure_network(name, wide=True):
    """(max |error| per image [3], smallest and largest float64 group variance) of the CPU composition on network `name`."""
    from tests.secure_batch_nets import numpy_sd, oracle_forward
    from tests.secure_groupnorm_nets import ChaChaDealer, default_blocks, plain_group_forward
    sd, blocks = wide_networks()[name]
    images = spread_images()
    variances = []
    plain = plain_group_forward(sd, images, blocks or default_blocks(), 3, "max", variances)
    ctx = S.OracleContext(ChaChaDealer(NET_DEALER_SEED), 10, 3)
    fwd = oracle_forward_wide if wide else (lambda *a: oracle_forward(*a, "max", "group"))
    out = fwd(ctx, numpy_sd(sd), images.numpy(), blocks)
    dec = S.radd(out[0], out[1]).astype(np.float64) / 10 ** 3
    lo, hi = min(float(v.min()) for v in variances), max(float(v.max()) for v in variances)
    return np.abs(dec - plain).max(axis=1), lo, hi
