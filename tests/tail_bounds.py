"""Per-element error bounds for the kernels that close every training step (primia_amd/csrc/pool_fc_loss.hip, optim.hip):
float64 references, the bound each output element must keep, and checkers that take the kernel's outputs as plain CPU arrays —
tests/test_tail_bounds_host.py feeds them a CPU stand-in and tampered outputs, tests/test_gpu_tail_elementwise.py the outputs
of the HIP kernels.  Nothing here imports primia_amd or needs a device.  _judge, BoundError, check_guards, same_bits, UB, UF
and TINY are conv_bounds.py's; the tap / mask helpers are norm_bounds.py's.

Why per element.  tests/test_gpu_ops.py judges these kernels by ||a - b|| / ||b|| against torch fp32 at one or two shapes
each: post-ReLU square inputs for the pools, out_f = 3 and N <= 5 for the head, N = 37 for the loss, 98 blocks for the flat
kernels, Adam after three steps at 1e-5.  A pad read as 0, a lost second loop trip, a dropped weight decay pass all of that.

Conventions.  Operands are rounded to the compute type BEFORE use; references are float64 on the rounded operands.
uf = 2^-24 per rounded fp32 operation, us = ub = 2^-8 (bf16) or uf (fp32) for the store, g(k) = k uf / (1 - k uf).  The compiler
may contract a*b+c to an fma: that REMOVES a rounding, a per-operation bound still holds.  Sums are bounded order-free: k
nonzero terms take k - 1 additions that round (a zero start and zero partials add exactly), every partial sum is at most the
sum of the |terms|.  A division or sqrtf gets one ulp = 2 uf (as norm_bounds.py's eval mode).  Where a kernel consumes a
value it stored itself (feat in head_fwd_kernel, dx in head_bwd_bnsums_kernel, Adam's new exp_avg / exp_avg_sq) the reference
takes the stored value, and that value is judged by its own check.  With E the error before the store, every stored
activation keeps
    |out - ref| <= (1 + us) E + us |ref| + 2^-126        (`store_bound`; fp32 results of a last fp32 operation: E + 2^-126)

primia_maxpool3x3s2_fwd (pool3x3s2_fwd_kernel<T, true>)  exact: y has the BITS of the first maximum, r-major, over the taps
    inside the image; the argmax byte is that tap's r * 3 + s.  A window holding a NaN yields NaN and names a NaN tap.
primia_maxpool3x3s2_bwd  ref = sum of dy over the (<= 4) windows whose code names the pixel, codes as verified above.
    g = 0 + t1 + t2 + t3 + t4: at most 3 additions round, each by uf S, S = sum |dy| of those windows:  E = 3 uf S.
primia_avgpool3x3s2_fwd  t in-image taps summed (t - 1 additions), the constant fl(1/9) (uf), the product (uf); divisor 9
    always (count_include_pad):  E = g(t + 1) sum|x| / 9.
primia_avgpool3x3s2_bwd  m <= 4 windows, each dy * fl(1/9) (constant uf + product uf), m - 1 additions:
    E = g(m + 1) sum|dy| / 9.
primia_global_avgpool_fwd, primia_head_fwd (feat)  HW <= 64 here: HW terms in any grouping (row groups through LDS or one
    chain) round at most HW - 1 times, then the division:  E = (g(HW) + 2 uf) sum|x| / HW;  feat is fp32: E + 2^-126.
primia_global_avgpool_bwd  dfeat / HW, then the store:  E = 2 uf |ref|.
primia_linear_fwd, primia_head_fwd (logits)  ref = sum_i x_i w_ji + b_j on the kernel's own stored feat.  C products (uf
    each) and C + 1 terms with the bias: C additions:  E = g(C + 1) (sum|x w| + |b|), fp32.
primia_linear_bwd  dx: out_f products, out_f - 1 additions: g(out_f) sum|dy w|.  dw: g(N) sum|dy x|.  db: g(N) sum|dy|.
primia_head_bwd  a = sum_j dy w (g(out_f)), / HW (2 uf), store:  E = g(out_f + 2) sum|dy w| / HW.  Every pixel of a sample
    holds the same bits per channel.
primia_head_bwd_bnsums  dx bit-identical to primia_head_bwd.  With vr the STORED dx value, ngrp = 256 / cpr thread groups
    per channel chunk, L = ceil(HW / ngrp) pixels per thread, on = the mask bit:
    sums[n][0][c] = vr count: ngrp products vr * cnt_g (counts are exact integers) and ngrp - 1 additions: g(ngrp) |vr| count.
    sums[n][1][c] = vr invstd sum_on (y - mean): fl(y - mean) (1) and a thread's chain (L - 1), the product with vr (1),
    ngrp - 1 additions, the product with invstd (1):  g(L + ngrp + 1) |vr| invstd sum_on |y - mean|.
primia_xent_hard / primia_xent_soft (xent_kernel).  EXP_ULPS / LOG_ULPS: the accuracy of device expf / logf cannot be derived.
    The ROCm install carries no copy of the device-math accuracy table (searched for under its share/ and doc trees), so
    both are ASSUMED to be 2 ulp (ee = EXP_ULPS 2 uf, le = LOG_ULPS 2 uf relative); they were not tuned to a run.  Per row,
    with G = max_c |o_c - mx|:  fl(o_c - mx) errs by uf |o_c - mx| and enters exp as an ABSOLUTE error, so
      e_c = exp(o_c - mx)(1 + eta_c), |eta_c| <= ee + uf |o_c - mx|;  se (C positive terms): rs = ee + uf G + g(C);
      inv = 1 / se: rs + 2 uf;  p_c = e_c inv: rp_c = eta_c + rs + 3 uf;
      lse = mx + logf(se): d_lse = rs + le |log se| + uf |lse|.
    hard:  T_n = wt (lse - o_t): d_T = wt d_lse + 2 uf |T_n|;  num = sum T_n over 256 threads and a tree: d_num = sum d_T +
      g(N) sum|T|;  den = sum wt: d_den = g(N) den;  loss = num / den: (d_num + |loss| d_den) / (den - d_den) + 2 uf |loss|.
      dlogits = fl(wt / den)(p_c - [c = t]):  E = |w| (p_c rp_c + uf |p_c - [c = t]|) + |ref| (g(N) + 3 uf), w = wt / den.
    soft:  a = sum_c cw_c t_c (1 without weights): d_a = g(C) sum|cw t|;  l = -sum_c t_c (o_c - lse): d_l = sum|t_c| d_lse +
      g(C + 1) sum|t_c (o_c - lse)|;  T_n = a l: d_T = |a| d_l + |l| d_a + uf |T|;  loss = num / N.
      dlogits = (a / N)(p_c ts - t_c), ts = sum t (d_ts = g(C) sum|t|):  d_q = p_c (|ts| (rp_c + uf) + d_ts),
      d_in = d_q + uf |p_c ts - t_c|, d_coef = d_a / N + 2 uf |a / N|:  E = |a / N| d_in + |p_c ts - t_c| d_coef + uf |ref|.
primia_sgd_step(_dev)  p - lr (g + wd p): fl(wd p), the addition, the product with lr — three operations — and the final
    subtraction, whose rounding is the store:  E = 3 uf lr (|g| + |wd p|),  (1 + uf) E + uf |ref| + 2^-126.
primia_adam_step(_dev)  one step from a given fp32 state, with the scalars the kernel uses: beta1, beta2, eps, wd as floats,
    fl(1 - beta) in fp32, step_size = (float)(lr / bc1), inv_sqrt_bc2 = (float)(1 / sqrt(bc2)), bc = 1 - beta^step in double.
      g' = g + wd p: d_g = 2 uf (|g| + |wd p|)
      exp_avg'    = m b1 + (1 - b1) g':  E = uf |m b1| + (1 - b1)(d_g + uf |g'|), the addition is the store
      exp_avg_sq' = v b2 + ((1 - b2) g') g':  E = uf |v b2| + (1 - b2)(2 |g'| d_g + d_g^2 + 2 uf g'^2)
      p' = p - step_size (m' / (sqrtf(v') inv_sqrt_bc2 + eps)) on the STORED m', v': sqrtf (2 uf), the product, the addition
           (all terms positive: 4 uf on the denominator), the division (2 uf), the product with step_size:
           E = g(7) |u|, u = step_size m' / denom; the subtraction is the store.
    The _dev forms read primia_opt_hyper_set's words and must give the BITS of the host-scalar forms.
primia_scale, primia_axpy, primia_divide, primia_fx_encode, primia_fx_decode  exact by bits against the same fp32 expression
    on the CPU: fl(x a); fl(y + fl(x a)), the product rounded first; fl(x / d); trunc toward zero of fl(x scale);
    fl(fl(q) / scale).

No constant here was taken from a run of a kernel.

What the bounds can and cannot see (measured with the stand-in of test_tail_bounds_host.py; figures in its docstring): the
max-pool checks are exact, so any wrong tap, tie order or byte is seen; a bf16 activation check is dominated by ub |ref|, so
a neighbour's value, a fill value or a truncating store is seen but a lost low-order addend is not; the fp32 checks see
everything down to a few uf of the sum of |terms|: one missing term of dw / db at N <= 40, Adam's weight decay in exp_avg
(0.1 wd |p| against ~3 uf |g|); they cannot see a wrong summation ORDER, nor an error in a dlogits row whose class weight is 0.
"""
import functools
import math
from collections import namedtuple

import torch

from tests.conv_bounds import BF16, F32, TINY, UB, UF, BoundError, _judge, check_guards, same_bits  # noqa: F401  (re-exported)
from tests.norm_bounds import chunk, mask_bits, mask_bytes, pool_out, pool_taps, rnd, store_bound, us_of  # noqa: F401

EXP_ULPS = 2.0       # assumed, see the docstring
LOG_ULPS = 2.0       # assumed

PoolCase = namedtuple("PoolCase", "N H W C dtype")
HeadCase = namedtuple("HeadCase", "N HW C out_f dtype")
LinCase = namedtuple("LinCase", "N in_f out_f omit")            # omit: "" | "b" | "db" | "dx": the pointer passed as NULL
XentCase = namedtuple("XentCase", "N C")

# channels every pool case carries (C >= 4)
CH_NEG, CH_CONST, CH_RELU, CH_CORNER = 0, 1, 2, 3
CONST_VALUE, CORNER_VALUE = 0.625, 96.0

# (N, H, W, C): 1 x 7 and 7 x 1 images (one chunk per pixel in bf16); 2 x 2 -> one output pixel; C = 72: 9 (bf16) / 18
# (fp32) chunks, no power of two, H != W both ways; odd square; two blocks and more; C = CH = 4 in fp32
POOL_SHAPES = [(1, 1, 7, 8), (3, 7, 1, 8), (1, 2, 2, 64), (2, 5, 12, 72), (2, 12, 5, 64), (1, 9, 9, 64), (2, 16, 16, 64)]
POOL_CASES = [PoolCase(*s, dt) for s in POOL_SHAPES for dt in (BF16, F32)] + [PoolCase(2, 5, 6, 4, F32)]
POOL_NAN_CASES = [PoolCase(1, 5, 6, 8, BF16), PoolCase(1, 5, 6, 8, F32)]

# (N, HW, C, out_f): the training head; a second trip of the out_f loop; one output; nine outputs on one pixel; tpr = 1 in
# bf16 (rpp = 256 > HW); tpr = 256 (rpp = 1) in either type; C = 192 in fp32: 48 chunks do not divide 256 -> general kernels
HEAD_CASES = ([HeadCase(*s, dt) for s in [(5, 49, 512, 3), (3, 49, 512, 5), (2, 4, 64, 1), (2, 1, 64, 9), (2, 49, 8, 3)]
               for dt in (BF16, F32)] + [HeadCase(2, 7, 2048, 3, BF16), HeadCase(2, 7, 1024, 3, F32)])
HEAD_FALLBACK_CASE = HeadCase(3, 6, 192, 3, F32)
# (N, in_f, out_f): one lane idle, bias column in the block of column 0; in_f = 64: the bias column alone in a second
# block, N = 16: every sample group holds one; N = 17: a second trip for group 0; the training shape's in_f with N > 32
LIN_CASES = [LinCase(1, 63, 1, ""), LinCase(16, 64, 3, "db"), LinCase(17, 65, 5, ""), LinCase(40, 512, 3, "dx"),
             LinCase(5, 100, 2, "b")]
# (N, C): 64 / 65: one wave and one sample more; 257: a thread's second sample; 600 x 16: kMaxClasses
XENT_CASES = [XentCase(*s) for s in [(1, 1), (37, 3), (64, 2), (65, 3), (257, 3), (600, 16)]]
# n: no vector body; one vector; vector + tail; a ragged block; 98 blocks; 4 195 507 = 2 * 2048 * 256 * 4 + 1200 + 3: two
# full grid-stride trips, a ragged third (300 vectors) and a three-element scalar tail
FLAT_N = [1, 2, 3, 4, 5, 1023, 100003, 4195507]
FX_N = FLAT_N[:-1] + [524588]          # 524 588 = 2048 * 256 + 300: a ragged second trip; int64 buffers stay under 16 MB
ADAM_STEPS = [1, 2, 1000]
FLAT_BLOCK_CAP = 2048


def case_id(c):
    return "x".join(str(v) for v in c if v != "")


def gam(k):
    return k * UF / (1.0 - k * UF)


def _d(a, shape=None):
    t = torch.as_tensor(a).detach().cpu().to(torch.float64)
    return t.reshape(shape) if shape is not None else t


def _f(a, shape=None):
    t = torch.as_tensor(a).detach().cpu().to(torch.float32)
    return t.reshape(shape) if shape is not None else t


def f32(v):
    """A Python number rounded to fp32, as a double: what a `float` argument of the C ABI carries."""
    return torch.tensor(v, dtype=torch.float64).to(torch.float32).double().item()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def check_exact(name, got, want, axes=("i",)):
    """got / want: fp32 or int64 arrays; equal by bits (so -0 != +0, and a NaN equals the same NaN).  Raises BoundError
    naming the first few positions."""
    got, want = torch.as_tensor(got).detach().cpu(), torch.as_tensor(want).detach().cpu()
    assert got.dtype == want.dtype and got.numel() == want.numel(), (got.dtype, want.dtype, got.shape, want.shape)
    got = got.reshape(want.shape)
    bad = _bits(got) != _bits(want)
    if bad.any():
        pos = bad.nonzero()[:5].tolist()
        raise BoundError(f"{name}: {int(bad.sum())} of {bad.numel()} differ by bits, first at " + "; ".join(
            "(" + ", ".join(f"{a}={v}" for a, v in zip(axes, p)) + f"): got {got[tuple(p)].item()!r} want "
            f"{want[tuple(p)].item()!r}" for p in pos))
    return 0.0


PIX_AXES = ("image", "row", "col", "channel")


# ---- 3x3 / 2 pools -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_operands(c):
    """x [N, H, W, C], dy [N, Ho, Wo, C]: fp32 tensors holding values of the compute type.  Shared: read-only."""
    g = torch.Generator().manual_seed(7000 + 1000 * c.H + 10 * c.W + c.C + c.N)
    x = torch.randn(c.N, c.H, c.W, c.C, generator=g)
    x[..., CH_NEG] = -(x[..., CH_NEG].abs() + 0.125)            # negative everywhere: a 0 start or a 0 pad wins every window
    x[..., CH_CONST] = CONST_VALUE                               # every window ties: the first tap inside the image must win
    x[..., CH_RELU] = x[..., CH_RELU].clamp_min(0.0)             # what the training step feeds
    x[:, c.H - 1, c.W - 1, CH_CORNER] = CORNER_VALUE             # one large value, in the last corner
    dy = torch.randn(c.N, pool_out(c.H), pool_out(c.W), c.C, generator=g)
    return rnd(x, c.dtype), rnd(dy, c.dtype)


@functools.lru_cache(maxsize=None)
def pool_nan_operands(c):
    x, dy = pool_operands(c)
    x = x.clone()
    x[0, 2, 3, 0] = x[0, 0, 0, 1] = x[0, c.H - 1, c.W - 1, 5] = float("nan")
    x[0, 1, 1, 6] = x[0, 2, 2, 6] = float("nan")                 # two in one window
    return x, dy


def maxpool_ref(x):
    """(y, code, nanwin): first maximum in scan order over the taps inside the image, its r * 3 + s, and the windows that
    hold a NaN (y, code meaningless there)."""
    taps = pool_taps(x, float("-inf"))
    best = torch.full(taps.shape[1:], float("-inf"))
    pos = torch.full(taps.shape[1:], 255, dtype=torch.uint8)
    for k in range(9):
        up = (taps[k] > best) | ((pos == 255) & (taps[k] != float("-inf")) & ~torch.isnan(taps[k]))
        best = torch.where(up, taps[k], best)
        pos = torch.where(up, torch.full_like(pos, k), pos)
    return best, pos, torch.isnan(taps).any(0)


def check_maxpool_fwd(name, y, argmax, x):
    """y / argmax: N*Ho*Wo*C elements in [N][Ho][Wo][C] order; x [N, H, W, C] fp32 values of the compute type."""
    ref, code, nanwin = maxpool_ref(x)
    y = _f(y, ref.shape)
    got_code = torch.as_tensor(argmax).detach().cpu().reshape(ref.shape)
    taps = pool_taps(x, float("-inf"))
    at = taps.gather(0, got_code.clamp(max=8).to(torch.int64).unsqueeze(0))[0]
    bad = torch.where(nanwin, ~torch.isnan(y), _bits(y) != _bits(ref))
    if bad.any():
        pos = bad.nonzero()[:5].tolist()
        raise BoundError(f"{name} y: {int(bad.sum())} of {bad.numel()} differ by bits, first at " + "; ".join(
            "(" + ", ".join(f"{a}={v}" for a, v in zip(PIX_AXES, p)) + f"): got {y[tuple(p)].item()!r} want "
            f"{ref[tuple(p)].item()!r}" for p in pos))
    bad = torch.where(nanwin, (got_code > 8) | ~torch.isnan(at), got_code != code)
    if bad.any():
        pos = bad.nonzero()[:5].tolist()
        raise BoundError(f"{name} argmax: {int(bad.sum())} of {bad.numel()} differ, first at " + "; ".join(
            "(" + ", ".join(f"{a}={v}" for a, v in zip(PIX_AXES, p)) + f"): got {int(got_code[tuple(p)])} want "
            f"{int(code[tuple(p)])}" for p in pos))
    return 0.0


def _scatter(terms, H, W):
    """terms [9, N, Ho, Wo, C] (float64) sent back to the taps of their windows -> [N, H, W, C]."""
    _, N, Ho, Wo, C = terms.shape
    g = torch.zeros(N, H + 2, W + 2, C, dtype=torch.float64)
    for k in range(9):
        r, s = divmod(k, 3)
        g[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] += terms[k]
    return g[:, 1:H + 1, 1:W + 1].contiguous()


def check_maxpool_bwd(name, dx, dy, argmax, c):
    dy = _d(dy, (c.N, pool_out(c.H), pool_out(c.W), c.C))
    code = torch.as_tensor(argmax).detach().cpu().reshape(dy.shape)
    terms = torch.stack([dy * (code == k) for k in range(9)])
    ref, S = _scatter(terms, c.H, c.W), _scatter(terms.abs(), c.H, c.W)
    return _judge(f"{name} dx", _d(dx, ref.shape), ref, store_bound(ref, 3.0 * UF * S, c.dtype), PIX_AXES)


def check_avgpool_fwd(name, y, x, c):
    taps = pool_taps(x.double(), 0.0)
    t = pool_taps(torch.ones(x.shape, dtype=torch.float64), 0.0).sum(0)
    ref, A = taps.sum(0) / 9.0, taps.abs().sum(0) / 9.0
    return _judge(f"{name} y", _d(y, ref.shape), ref, store_bound(ref, gam(t + 1.0) * A, c.dtype), PIX_AXES)


def check_avgpool_bwd(name, dx, dy, c):
    dy = _d(dy, (c.N, pool_out(c.H), pool_out(c.W), c.C))
    terms = dy.unsqueeze(0).expand(9, *dy.shape)
    ref, S = _scatter(terms, c.H, c.W) / 9.0, _scatter(terms.abs(), c.H, c.W) / 9.0
    m = _scatter(torch.ones_like(terms), c.H, c.W)
    return _judge(f"{name} dx", _d(dx, ref.shape), ref, store_bound(ref, gam(m + 1.0) * S, c.dtype), PIX_AXES)


# ---- global average pool, linear, head ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_operands(c):
    """x, bn_y [N, HW, C] (values of the compute type), keep (bool, the ReLU mask), w [out_f, C], b [out_f], dy [N, out_f]
    (the logits' gradient), dfeat [N, C], mean / invstd [C]: fp32.  Shared: read-only."""
    g = torch.Generator().manual_seed(9000 + 100 * c.HW + c.C + 7 * c.out_f + c.N)
    o = {"x": rnd(torch.randn(c.N, c.HW, c.C, generator=g).clamp_min(-0.25), c.dtype),
         "bn_y": rnd(torch.randn(c.N, c.HW, c.C, generator=g) * 1.5 + 0.5, c.dtype),
         "keep": torch.rand(c.N, c.HW, c.C, generator=g) > 0.4,
         "w": torch.randn(c.out_f, c.C, generator=g) * 0.05, "b": torch.randn(c.out_f, generator=g),
         "dy": torch.randn(c.N, c.out_f, generator=g), "dfeat": torch.randn(c.N, c.C, generator=g),
         "mean": torch.randn(c.C, generator=g) * 0.5 + 0.5, "invstd": 0.5 + torch.rand(c.C, generator=g)}
    o["keep"][:, :, 1] = False                                    # a channel no pixel of which is kept
    o["keep"][:, :, 2] = True
    return o


HEAD_AXES = ("sample", "pixel", "channel")


def check_feat(name, feat, x, c):
    x = x.double()
    ref, A = x.mean(1), x.abs().mean(1)
    return _judge(f"{name} feat", _d(feat, ref.shape), ref, (gam(c.HW) + 2.0 * UF) * A + TINY, ("sample", "channel"))


def check_gap_bwd(name, dx, dfeat, c):
    ref = (_d(dfeat, (c.N, 1, c.C)) / c.HW).expand(c.N, c.HW, c.C).contiguous()
    return _judge(f"{name} dx", _d(dx, ref.shape), ref, store_bound(ref, 2.0 * UF * ref.abs(), c.dtype), HEAD_AXES)


@functools.lru_cache(maxsize=None)
def lin_operands(c):
    g = torch.Generator().manual_seed(11000 + 100 * c.N + c.in_f + 7 * c.out_f)
    return {"x": torch.randn(c.N, c.in_f, generator=g), "w": torch.randn(c.out_f, c.in_f, generator=g) * 0.1,
            "b": torch.randn(c.out_f, generator=g), "dy": torch.randn(c.N, c.out_f, generator=g)}


def check_linear_fwd(name, y, x, w, b):
    """x: the [N, in_f] fp32 input (the kernel's own stored feat for the head), b None: no bias."""
    x, w = _d(x), _d(w)
    ref, A = x @ w.t(), x.abs() @ w.abs().t()
    if b is not None:
        ref, A = ref + _d(b), A + _d(b).abs()
    return _judge(f"{name} logits", _d(y, ref.shape), ref, gam(x.shape[1] + 1.0) * A + TINY, ("sample", "output"))


def check_linear_bwd(name, dx, dw, db, x, w, dy):
    """dx / db None: not asked for."""
    x, w, dy = _d(x), _d(w), _d(dy)
    N, out_f = dy.shape
    worst = []
    if dx is not None:
        worst.append(_judge(f"{name} dx", _d(dx, x.shape), dy @ w, gam(out_f) * (dy.abs() @ w.abs()) + TINY, ("sample", "input")))
    worst.append(_judge(f"{name} dw", _d(dw, w.shape), dy.t() @ x, gam(N) * (dy.abs().t() @ x.abs()) + TINY, ("output", "input")))
    if db is not None:
        worst.append(_judge(f"{name} db", _d(db, (out_f,)), dy.sum(0), gam(N) * dy.abs().sum(0) + TINY, ("output",)))
    return max(worst)


def check_head_bwd(name, dx, w, dy, c):
    w, dy = _d(w), _d(dy)
    dxf = _f(dx, (c.N, c.HW, c.C))
    same = _bits(dxf) != _bits(dxf[:, :1].expand_as(dxf).contiguous())
    if same.any():
        pos = same.nonzero()[:5].tolist()
        raise BoundError(f"{name} dx: {int(same.sum())} elements differ by bits from pixel 0 of their sample, first at " + "; ".join(
            "(" + ", ".join(f"{a}={v}" for a, v in zip(HEAD_AXES, p)) + ")" for p in pos))
    ref = ((dy @ w) / c.HW).unsqueeze(1).expand(c.N, c.HW, c.C).contiguous()
    A = ((dy.abs() @ w.abs()) / c.HW).unsqueeze(1).expand_as(ref)
    return _judge(f"{name} dx", dxf.double(), ref, store_bound(ref, gam(c.out_f + 2.0) * A, c.dtype), HEAD_AXES)


def bnsums_groups(c):
    """(ngrp, L): thread groups per channel chunk and pixels per thread of head_bwd_bnsums_kernel."""
    ngrp = 256 // (c.C // chunk(c.dtype))
    return ngrp, -(-c.HW // ngrp)


def check_head_bnsums(name, sums, dx, bn_y, keep, mean, invstd, c):
    """sums [N][2][C]; dx: the kernel's own stored gradient [N, HW, C]; keep: bool [N, HW, C]."""
    ngrp, L = bnsums_groups(c)
    vr = _d(dx, (c.N, c.HW, c.C))[:, 0]
    keep = torch.as_tensor(keep).reshape(c.N, c.HW, c.C).double()
    dev = (_d(bn_y, keep.shape) - _d(mean)) * keep
    inv = _d(invstd)
    ref = torch.stack([vr * keep.sum(1), vr * inv * dev.sum(1)], 1)
    bound = torch.stack([gam(ngrp) * vr.abs() * keep.sum(1), gam(L + ngrp + 1.0) * vr.abs() * inv * dev.abs().sum(1)], 1) + TINY
    return _judge(f"{name} sums", _d(sums, ref.shape), ref, bound, ("sample", "which", "channel"))


# ---- cross entropy -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def xent_operands(c):
    """logits [N, C] (every fifth row: one logit 30 above the rest), hard targets (int64), soft targets (>= 0, rows do not
    sum to 1), class weights with a 0 entry (C > 1)."""
    g = torch.Generator().manual_seed(13000 + 10 * c.N + c.C)
    logits = torch.randn(c.N, c.C, generator=g) * 2.0
    rows = torch.arange(0, c.N, 5)
    logits[rows, rows % c.C] = logits[rows].max(1).values + 30.0
    hard = torch.randint(0, c.C, (c.N,), generator=g)
    hard[0] = c.C - 1                                            # a sample whose weight is not 0
    soft = torch.rand(c.N, c.C, generator=g) * 1.3
    cw = 0.5 + torch.rand(c.C, generator=g)
    if c.C > 1:
        cw[0] = 0.0
    return {"logits": logits, "hard": hard, "soft": soft, "cw": cw}


def xent_ref(c, soft, weighted):
    """loss, d_loss (scalars), dlogits, d_dlogits [N, C]: float64 reference and bounds."""
    o = xent_operands(c)
    z = o["logits"].double()
    N, C = z.shape
    ee, le = EXP_ULPS * 2.0 * UF, LOG_ULPS * 2.0 * UF
    mx = z.max(1, keepdim=True).values
    gap = (z - mx).abs()
    e = torch.exp(z - mx)
    se = e.sum(1, keepdim=True)
    eta = ee + UF * gap
    rs = ee + UF * gap.max(1, keepdim=True).values + gam(C)
    p, rp = e / se, eta + rs + 3.0 * UF
    lse = mx + torch.log(se)
    d_lse = rs + le * torch.log(se).abs() + UF * lse.abs()
    cw = o["cw"].double() if weighted else None
    if soft:
        t = o["soft"].double()
        a = (t * cw).sum(1, keepdim=True) if weighted else torch.ones(N, 1, dtype=torch.float64)
        d_a = gam(C) * (t * cw).abs().sum(1, keepdim=True) if weighted else torch.zeros(N, 1, dtype=torch.float64)
        terms = t * (z - lse)
        l_ = -terms.sum(1, keepdim=True)
        d_l = t.abs().sum(1, keepdim=True) * d_lse + gam(C + 1.0) * terms.abs().sum(1, keepdim=True)
        T = a * l_
        d_T = a.abs() * d_l + l_.abs() * d_a + UF * T.abs()
        loss = T.sum() / N
        d_loss = (d_T.sum() + gam(N) * T.abs().sum()) / N + 2.0 * UF * loss.abs()
        ts = t.sum(1, keepdim=True)
        d_ts = gam(C) * t.abs().sum(1, keepdim=True)
        inner, coef = p * ts - t, a / N
        d_in = p * (ts.abs() * (rp + UF) + d_ts) + UF * inner.abs()
        d_coef = d_a / N + 2.0 * UF * coef.abs()
        dl = coef * inner
        d_dl = coef.abs() * d_in + inner.abs() * d_coef + UF * dl.abs()
    else:
        t = o["hard"]
        hot = torch.zeros(N, C, dtype=torch.float64).scatter_(1, t.unsqueeze(1), 1.0)
        wt = cw[t].unsqueeze(1) if weighted else torch.ones(N, 1, dtype=torch.float64)
        T = wt * (lse - z.gather(1, t.unsqueeze(1)))
        d_T = wt * d_lse + 2.0 * UF * T.abs()
        den = wt.sum()
        d_den = gam(N) * den
        loss = T.sum() / den
        d_loss = (d_T.sum() + gam(N) * T.abs().sum() + loss.abs() * d_den) / (den - d_den) + 2.0 * UF * loss.abs()
        w_ = wt / den
        dl = w_ * (p - hot)
        d_dl = w_ * (p * rp + UF * (p - hot).abs()) + dl.abs() * (gam(N) + 3.0 * UF)
    return loss, d_loss + TINY, dl, d_dl + TINY


def check_xent(name, loss, dlogits, c, soft, weighted):
    """(worst loss ratio, worst dlogits ratio); dlogits None: not asked for."""
    ref, d_loss, dl, d_dl = xent_ref(c, soft, weighted)
    w_loss = _judge(f"{name} loss", _d(loss, (1,)), ref.reshape(1), d_loss.reshape(1), ("loss",))
    if dlogits is None:
        return w_loss, 0.0
    return w_loss, _judge(f"{name} dlogits", _d(dlogits, dl.shape), dl, d_dl, ("sample", "class"))


# ---- flat kernels ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flat_operands(n):
    """p, g, m, v (>= 0), x: fp32 [n]; q: int64 [n] with magnitudes beyond 2^24.  Elements with g = 0 and v = 0 (and m = 0 at
    some of them) are spread through the array, the last element among them.  Shared: read-only."""
    g_ = torch.Generator().manual_seed(15000 + n % 9973)
    p, g, m = (torch.randn(n, generator=g_) for _ in range(3))
    v = torch.randn(n, generator=g_) ** 2 * 1e-2
    g[::7] = 0.0
    v[::7] = 0.0
    m[::14] = 0.0
    g[n - 1] = v[n - 1] = 0.0
    x = torch.randn(n, generator=g_) * 3.0
    q = (torch.randn(n, generator=g_, dtype=torch.float64) * 2.0 ** 30).to(torch.int64)
    return {"p": p, "g": g, "m": m, "v": v, "x": x, "q": q}


FLAT_AXES = ("i",)


def check_sgd(name, p_new, p, g, lr, wd):
    lr, wd = f32(lr), f32(wd)
    p, g = _d(p), _d(g)
    ref = p - lr * (g + wd * p)
    E = 3.0 * UF * lr * (g.abs() + (wd * p).abs())
    return _judge(f"{name} p", _d(p_new, ref.shape), ref, (1.0 + UF) * E + UF * ref.abs() + TINY, FLAT_AXES)


def adam_scalars(lr, beta1, beta2, eps, wd, step):
    """The scalars AdamFn holds, as doubles: (b1, 1 - b1, b2, 1 - b2, eps, wd, step_size, inv_sqrt_bc2)."""
    b1, b2 = f32(beta1), f32(beta2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return b1, f32(1.0 - b1), b2, f32(1.0 - b2), f32(eps), f32(wd), f32(f32(lr) / bc1), f32(1.0 / math.sqrt(bc2))


def check_adam(name, p_new, m_new, v_new, p, g, m, v, scalars):
    """(worst p, worst exp_avg, worst exp_avg_sq) after ONE step from the fp32 state (p, g, m, v)."""
    b1, omb1, b2, omb2, eps, wd, step_size, isb = scalars
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    m_st, v_st = _d(m_new, p.shape), _d(v_new, p.shape)
    g2 = g + wd * p
    d_g = 2.0 * UF * (g.abs() + (wd * p).abs())
    ref_m = m * b1 + omb1 * g2
    E_m = UF * (m * b1).abs() + omb1 * (d_g + UF * g2.abs())
    w_m = _judge(f"{name} exp_avg", m_st, ref_m, (1.0 + UF) * E_m + UF * ref_m.abs() + TINY, FLAT_AXES)
    ref_v = v * b2 + omb2 * g2 * g2
    E_v = UF * (v * b2).abs() + omb2 * (2.0 * g2.abs() * d_g + d_g * d_g + 2.0 * UF * g2 * g2)
    w_v = _judge(f"{name} exp_avg_sq", v_st, ref_v, (1.0 + UF) * E_v + UF * ref_v.abs() + TINY, FLAT_AXES)
    u = step_size * m_st / (torch.sqrt(v_st.clamp_min(0.0)) * isb + eps)
    ref_p = p - u
    w_p = _judge(f"{name} p", _d(p_new, p.shape), ref_p, (1.0 + UF) * gam(7.0) * u.abs() + UF * ref_p.abs() + TINY, FLAT_AXES)
    return w_p, w_m, w_v


def _s(a):
    return torch.tensor(a, dtype=torch.float32)


def ref_scale(x, a):
    return _f(x) * _s(a)


def ref_axpy(y, x, a):
    return _f(y) + _f(x) * _s(a)         # two torch operations: the product is rounded before the addition


def ref_divide(x, d):
    return _f(x) / _s(d)


def ref_fx_encode(x, scale):
    return (_f(x) * _s(scale)).to(torch.int64)     # a C cast: truncation toward zero


def ref_fx_decode(q, scale):
    return torch.as_tensor(q).cpu().to(torch.float32) / _s(scale)
