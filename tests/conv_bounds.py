"""Per-element error bounds for the convolution kernels: float64 references, the bound each output element must keep, and
checkers that take the kernel's output as a plain CPU array — so that tests/test_conv_bounds_host.py can feed them tampered
outputs without a GPU, and tests/test_gpu_conv_elementwise.py the outputs of the HIP kernels.  Nothing here imports
primia_amd or needs a device.

Why per element.  relerr = ||a - b|| / ||b|| over a whole tensor (the 1e-2 of test_gpu_ops.py, the 3e-3 of
test_gpu_train_step.py) cannot see ONE wrong pixel: at N = 66, H = 28, C = K = 128 a tap dropped at a single output pixel moves
it to 2.2e-3.  A tiled kernel's typical mistakes are exactly that local: a tap lost at an image border, a wrong pixel at the seam
of two tiles, one row of a ragged last tile, a store that truncates.

The bounds.  Operands are rounded to the compute type BEFORE use, the reference sees the values the kernel sees.  With
ub = 2^-8 (bf16, round to nearest) and uf = 2^-24 (fp32, round to nearest), ref the float64 result, A the same operation on the
absolute values of the operands (the sum of the |terms| of every output element) and n the number of terms per element:

    forward             n = C R S        |y  - ref| <= ub |ref| + 2 n uf A + 2^-126
    data gradient       n = K R S        |dx - ref| <= ub |ref| + 2 n uf A + 2^-126
    ... accumulating    ref = base * keep + dgrad,  A_total = |base| * keep + A,  n + 1 terms (keep = 1 without a mask)
    weight gradient     n = N Ho Wo      |dw - ref| <= 2 n uf A                       (fp32 result: no ub term)
    fp32 kernels        2 (n + 1) uf A, no ub term

Derivation.
  * A product of two bf16 numbers has 16 significant bits: it is EXACT in fp32.  Only the additions round.
  * n terms take n - 1 additions (n with a zero start).  Whatever their order or grouping — tiles, split reductions, tree or
    chain — every partial sum is bounded by the sum of the |terms| it covers, so each addition that rounds to nearest errs by
    at most uf times that, and an element's total error is below n uf A (first order; the second-order part is n^2 uf^2 A,
    a 2^-10 of it at the largest n used here).
  * The factor 2 pays for additions that CHOP instead (error up to one ulp = 2 uf): the matrix unit's internal additions are
    not documented to round to nearest.
  * ub |ref| is the single final rounding to bf16 (|fl(v) - v| <= ub |v|, and |v| differs from |ref| by the accumulation
    error only: second order).  2^-126 covers a result below the normal range.  A weight gradient stays in fp32: no such term.
  * The accumulating forms add the old value (a bf16 number, exact in fp32) to the fp32 accumulator before the one rounding:
    one more term, the old value's magnitude joins A.
  * fp32 kernels: the products round too (uf |product| each, uf A in all): n + 1 in place of n.
No constant depends on a kernel's tiling or summation order, and none was taken from a run of a kernel.  A route with a
legitimate extra rounding in its code gets a term derived from that code, next to a comment citing the lines — none has one.

What the bound can and cannot see (measured with the stand-in of test_conv_bounds_host.py — torch's fp32 convolution on the
rounded operands, result stored as bf16):
  * a truncating bf16 store (error up to 2 ub |ref|) exceeds it while the accumulation term is small next to ub |ref|: worst
    err / bound 1.14 - 1.96 on the shapes with n <= 2304; at n = 4608 (C = 512, 3x3) the accumulation term has grown to
    where the worst ratio is 0.74 — the bound no longer sees a truncating store there;
  * one missing term t of a weight gradient is seen while |t| > 2 n uf A ~ 2 n^2 uf tbar (tbar the mean |term|), i.e. for a
    typical term while n < 2^11.5 ~ 2900, and with room to spare at n <= 800; at the training shapes (n = 12 544 ... 802 816
    at batch 256) thousands of typical terms fit under it.  The same growth makes the forward bound at C = 512 (n = 4608)
    blind to a single typical term of 9 * 512, but every localized fault listed above drops or moves WHOLE taps or pixels.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

UB = 2.0 ** -8
UF = 2.0 ** -24
TINY = 2.0 ** -126

BF16, F32 = "bf16", "f32"
_TORCH = {BF16: torch.bfloat16, F32: torch.float32}

# N, H (= W), C, K, R (= S), stride, pad, dtype
ConvCase = namedtuple("ConvCase", "N H C K R stride pad dtype", defaults=(BF16,))


def case_id(c):
    return f"{c.N}x{c.H}x{c.C}-{c.K}k{c.R}s{c.stride}p{c.pad}" + ("-f32" if c.dtype == F32 else "")


def out_size(c):
    return (c.H + 2 * c.pad - c.R) // c.stride + 1


# ---- the shapes: the smallest that still reach the edge named ------------------------------------------------------
def _c3(N, H, C, K, dtype=BF16):
    return ConvCase(N, H, C, K, 3, 1, 1, dtype)


# conv3x3_lh4 / conv3x3_lh2 (wide 3x3 / stride 1; a pass is served where its OUTPUT channels are a multiple of 128)
LH_CASES = [
    _c3(3, 5, 128, 128),      # one ragged tile, M = 75
    _c3(7, 9, 192, 256),      # forward: 3 chunks, 2 channel tiles, ragged last tile (M = 567)
    _c3(7, 9, 256, 192),      # ... the same walk in the data gradient (its output has the 256 channels there)
    _c3(2, 2, 128, 128),      # every tap but the centre leaves the image
    _c3(1, 28, 128, 128),     # widest image, 4 exact tiles
]
# conv3x3_lh2 with 196-pixel tiles on 256 blocks: 65 pixel tiles x 4 channel tiles = 260 tiles, 4 blocks walk 2 tiles and
# 252 walk 1 (N = 256 gives 64 x 4 = 256 tiles, one each; N = 281 gives 71 x 4 = 284: 28 blocks with 2)
LH2_PERSISTENT_FWD = _c3(257, 7, 64, 512)
LH2_PERSISTENT_DGRAD = _c3(257, 7, 512, 64)     # the same tile walk for the three data-gradient forms
C64_CASES = [
    _c3(3, 12, 64, 64),       # ragged 8x8 patches
    _c3(5, 8, 64, 64),        # one patch per image
    _c3(1, 56, 64, 64),       # exact tiling
]
S2_CASES = [                                  # 3x3 / stride 2 transition blocks (the 1x1 / 2 downsample rides along)
    ConvCase(2, 16, 64, 128, 3, 2, 1),
    ConvCase(2, 6, 64, 128, 3, 2, 1),
    ConvCase(3, 14, 256, 512, 3, 2, 1),       # 256-channel dx
    ConvCase(1, 6, 64, 128, 3, 2, 1),         # 3 x 3 parity grid
    ConvCase(5, 4, 128, 128, 3, 2, 1),        # 2 x 2 parity grid, 128-channel dx
]
IGEMM_CASES = [
    ConvCase(2, 16, 64, 128, 3, 2, 1),
    ConvCase(2, 16, 64, 128, 1, 2, 0),
    ConvCase(3, 7, 256, 512, 3, 2, 1),        # odd size
    _c3(1, 31, 64, 128),                      # too wide for the linear-halo forward
    _c3(1, 10, 128, 128, F32),
    ConvCase(2, 16, 64, 128, 3, 2, 1, F32),
]
STEM_CASES = [ConvCase(5, 32, 3, 64, 7, 2, 3), ConvCase(3, 96, 3, 64, 7, 2, 3)]
WGRAD_PATCH_CASES = [_c3(3, 14, 256, 256), _c3(2, 28, 128, 128), _c3(3, 12, 64, 64), _c3(5, 8, 64, 64), _c3(4, 7, 512, 512)]
WGRAD_TAP_CASES = [ConvCase(2, 16, 64, 128, 3, 2, 1), ConvCase(4, 14, 256, 512, 1, 2, 0), ConvCase(3, 7, 256, 512, 3, 2, 1)]
WGRAD_F32_CASE = _c3(1, 10, 128, 128, F32)


def ds_of(c):
    """The 1x1 / stride-2 downsample beside a transition block's 3x3 / stride-2 convolution."""
    return ConvCase(c.N, c.H, c.C, c.K, 1, 2, 0, c.dtype)


FWD_DGRAD_CASES = (LH_CASES + [LH2_PERSISTENT_FWD, LH2_PERSISTENT_DGRAD] + C64_CASES + S2_CASES + [ds_of(c) for c in S2_CASES]
                   + IGEMM_CASES)
FWD_DGRAD_CASES = list(dict.fromkeys(FWD_DGRAD_CASES))
WGRAD_CASES = list(dict.fromkeys(WGRAD_PATCH_CASES + WGRAD_TAP_CASES + [WGRAD_F32_CASE] + STEM_CASES))


# ---- operands and float64 references, cached per shape -------------------------------------------------------------
def rnd(x, dtype):
    """Round to the compute type and return as fp32: the values the kernel sees."""
    return x.to(_TORCH[dtype]).to(torch.float32)


@functools.lru_cache(maxsize=None)
def operands(c):
    """x [N,C,H,H], w [K,C,R,R], dy [N,K,Ho,Ho], base (the old dx of the accumulating forms) and keep (its ReLU mask, bool):
    fp32 tensors holding values of the compute type.  Treat as read-only: they are shared."""
    g = torch.Generator().manual_seed(1000 * c.H + 10 * c.C + c.K + c.N + c.R)
    Ho = out_size(c)
    x = rnd(torch.randn(c.N, c.C, c.H, c.H, generator=g), c.dtype)
    w = rnd(torch.randn(c.K, c.C, c.R, c.R, generator=g) * 0.05, c.dtype)
    dy = rnd(torch.randn(c.N, c.K, Ho, Ho, generator=g), c.dtype)
    base = rnd(torch.randn(c.N, c.C, c.H, c.H, generator=g), c.dtype)
    keep = torch.rand(c.N, c.C, c.H, c.H, generator=g) > 0.4
    return x, w, dy, base, keep


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def fwd_ref(c):
    """(ref, A) of the forward pass, float64, [N,Ho,Wo,K]."""
    x, w, _, _, _ = operands(c)
    x, w = x.double(), w.double()
    return nhwc(F.conv2d(x, w, None, c.stride, c.pad)), nhwc(F.conv2d(x.abs(), w.abs(), None, c.stride, c.pad))


@functools.lru_cache(maxsize=None)
def dgrad_ref(c):
    """(ref, A) of the data gradient, float64, [N,H,W,C]."""
    x, w, dy, _, _ = operands(c)
    w, dy = w.double(), dy.double()
    ref = torch.nn.grad.conv2d_input(x.shape, w, dy, c.stride, c.pad)
    return nhwc(ref), nhwc(torch.nn.grad.conv2d_input(x.shape, w.abs(), dy.abs(), c.stride, c.pad))


@functools.lru_cache(maxsize=None)
def wgrad_ref(c):
    """(ref, A) of the weight gradient, float64, OIHW [K,C,R,S]."""
    x, w, dy, _, _ = operands(c)
    x, dy = x.double(), dy.double()
    ref = torch.nn.grad.conv2d_weight(x, w.shape, dy, c.stride, c.pad)
    return ref, torch.nn.grad.conv2d_weight(x.abs(), w.shape, dy.abs(), c.stride, c.pad)


# ---- checkers ------------------------------------------------------------------------------------------------------
class BoundError(AssertionError):
    pass


def _f64(a, shape):
    t = torch.as_tensor(a).detach().cpu()
    assert t.numel() == ref_numel(shape), (tuple(t.shape), tuple(shape))
    return t.to(torch.float64).reshape(shape)


def ref_numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _judge(what, got, ref, bound, axes):
    """Raise BoundError naming the count, the worst err / bound and the positions of the worst few; else return the worst
    err / bound.  A NaN or an infinity in `got` violates."""
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    bad = ratio > 1.0
    count = int(bad.sum())
    if count:
        flat = ratio.flatten()
        top = torch.topk(flat, min(5, count)).indices
        where = []
        for i in top.tolist():
            pos = []
            for s in reversed(ref.shape):
                pos.append(i % s)
                i //= s
            pos = tuple(reversed(pos))
            where.append(f"({', '.join(f'{a}={p}' for a, p in zip(axes, pos))}): got {got[pos].item():.9g} ref {ref[pos].item():.9g} "
                         f"err/bound {ratio[pos].item():.3g}")
        raise BoundError(f"{what}: {count} of {ratio.numel()} elements outside the bound, worst err/bound "
                         f"{flat.max().item():.3g}; worst at " + "; ".join(where))
    return float(ratio.max())


_PIX = ("image", "row", "col", "channel")


def _act_bound(ref, A, n, dtype):
    if dtype == F32:
        return 2.0 * (n + 1) * UF * A
    return UB * ref.abs() + 2.0 * n * UF * A + TINY


def check_fwd(y, c):
    """y: the forward result, N*Ho*Wo*K elements in [N][Ho][Wo][K] order."""
    ref, A = fwd_ref(c)
    return _judge(f"fwd {case_id(c)}", _f64(y, ref.shape), ref, _act_bound(ref, A, c.C * c.R * c.R, c.dtype), _PIX)


def check_dgrad(dx, c, base=None, keep=None):
    """dx: the data gradient in [N][H][W][C] order.  base: the old dx of an accumulating call ([N,C,H,H] as operands() returns
    it), keep: the ReLU mask applied to it (None: all kept)."""
    ref, A = dgrad_ref(c)
    n = c.K * c.R * c.R
    name = "dgrad"
    if base is not None:
        b = nhwc(base).double()
        if keep is not None:
            b = b * nhwc(keep).double()
        ref, A, n = b + ref, b.abs() + A, n + 1
        name = "dgrad+=" if keep is None else "dgrad+=masked"
    return _judge(f"{name} {case_id(c)}", _f64(dx, ref.shape), ref, _act_bound(ref, A, n, c.dtype), _PIX)


def check_wgrad(dw, c):
    """dw: the weight gradient, fp32, OIHW [K][C][R][S]."""
    ref, A = wgrad_ref(c)
    Ho = out_size(c)
    n = c.N * Ho * Ho
    bound = 2.0 * (n + 1 if c.dtype == F32 else n) * UF * A
    return _judge(f"wgrad {case_id(c)}", _f64(dw, ref.shape), ref, bound, ("k", "c", "r", "s"))


_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64, torch.uint8: torch.uint8}


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(_INT[a.dtype]), b.view(_INT[b.dtype]))


def check_guards(arena, lo, hi, fill):
    """arena: 1-D CPU array whose elements [lo, hi) are an output; everything in front and behind must still hold the bit
    pattern of `fill`.  Raises BoundError with the count and the offsets (relative to the output's first / one-past-last
    element) of the first few changed elements; returns 0.0."""
    arena = torch.as_tensor(arena).detach().cpu().reshape(-1)
    want = torch.full_like(arena, fill).view(_INT[arena.dtype])
    diff = arena.view(_INT[arena.dtype]) != want
    diff[lo:hi] = False
    count = int(diff.sum())
    if count:
        idx = diff.nonzero().flatten()[:8].tolist()
        names = [f"out[{i - lo}]" if i < lo else f"end+{i - hi}" for i in idx]
        raise BoundError(f"guard band: {count} elements written outside the output: " + ", ".join(names))
    return 0.0
