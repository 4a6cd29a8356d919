"""Per-element error bounds for the BatchNorm and GroupNorm kernels (primia_amd/csrc/bn.hip, gn.hip): float64 references,
the bound each output element must keep, and checkers that take the kernel's outputs as plain CPU arrays —
tests/test_norm_bounds_host.py feeds them a CPU stand-in and tampered outputs, tests/test_gpu_norm_elementwise.py the outputs of
the HIP kernels.  Nothing here imports primia_amd or needs a device.  _judge, BoundError, check_guards, same_bits, UB, UF and
TINY are conv_bounds.py's.

Why per element.  test_batchnorm_train and test_groupnorm_kernels (test_gpu_ops.py) compare with torch fp32 by
||a - b|| / ||b|| (1e-2 .. 2e-2 in bf16) on well conditioned channels: one wrong pixel, one wrong channel of 512 or a last row
never written does not move that number; every other test of the two files is a bit-identity between two launches of the
same base kernels.

Operands are rounded to the compute type BEFORE use.  ub = 2^-8 (bf16), uf = 2^-24 (fp32), both round to nearest; us = ub or
uf is the rounding of the store.  eps and momentum are the FLOATS 1e-5f and 0.1f widened to double, as the kernels take them.

Forward statistics, per channel (BatchNorm, n = M rows) or per (sample, group) (GroupNorm, n = HW C/G)
(bn_finalize_kernel, bn_inline_finalize_stats, gn_stats_finalize_kernel, gn_sample_reduce_kernel<0>):
    e1 = chain uf sum|y|                  the fp32 sums of y
    e2 = (chain + 1) uf sum y^2           the fp32 sums of y^2 (one more rounding for the product; bf16 products are exact)
    d_mean = e1 / n                       (+ uf |mean| once stored as save_mean)
    d_var  = e2 / n + 2 |mean| e1 / n + (e1 / n)^2
    invstd in [1 / sqrt(var + d_var + eps), 1 / sqrt(max(var - d_var, 0) + eps)]     (+ uf invstd once stored)
  * `chain`: the partial of a slab of rows is formed in fp32 (colreduce2_kernel / gn_colreduce2_kernel: per-thread chains
    over the slab's rows, then a serial sum of the rpp row groups through LDS), the partials are combined in fp64
    (fin_gather, gn_*_finalize_kernel; 2^-53 per addition: dropped).  Whatever the order inside a slab, every fp32 partial
    sum is bounded by the sum of the |terms| it covers, so a slab of L rows errs by at most L uf times that (L additions
    with the zero start): chain = the slab length — reduce_geometry's rows per block, ceil(HW / kGnSlabs) on GroupNorm's
    slab path, ceil(HW / row groups) on its one-block-per-sample path, whose row groups are combined in fp64
    (bn_slab_rows / gn_chain below restate them).  The channels of a group are combined in fp64.  The order-free
    chain = n would be blind from M ~ 65 000 on.  For the *_from_sums / apply_inline entry points the test forms the
    [slots][2][C] partials itself from float64 sums rounded once to fp32: chain = 1.
  * the variance is sum y^2 / n - mean^2 in fp64 ON the fp32 partials (bn.hip:198-200, gn.hip:163-165), clamped at 0.
    The reference variance is the two-pass one; d_var is the error of the kernel's formula, term by term.
  * the interval for invstd is exact, not first order: a constant channel has var = 0 and d_var / eps is not small at the
    large M.  save_mean / save_invstd are one (float) cast each: uf.
  * running_mean' = (1 - m) rm + m mean, running_var' = (1 - m) rv + m var_unbiased (biased for M = 1, bn.hip:204), formed
    in fp64 and cast once: m d_mean resp. m d_var M / (M - 1), plus uf |ref|.

Forward output, z = act(fma(y - mean, fl(invstd gamma), beta) [+ residual]) (bn_affine, common.h:125; gn_value, gn.hip:72):
    E = |gamma| ((invstd + d_invstd) d_mean + |y - mean| d_invstd) + k uf (|gamma| invstd |y - mean| + |beta| + |residual|)
    |z - ref| <= (1 + us) E + us |ref| + 2^-126
  * k = 3 without, 4 with a residual: fl(invstd gamma), fl(y - mean), the fma, the residual add; each is relative to a partial
    result no larger than the sum in the parenthesis.
  * ReLU is 1-Lipschitz.  The store rounds the value the kernel HAS, |v| <= |ref| + E: the factor (1 + us).
  * eval mode (bn_apply_kernel, eval_mode = 1): the statistics are inputs (d_mean = 0) and invstd = 1.f / sqrtf(var + eps) in
    fp32: half a rounding from the sum, at most one ulp = 2 uf each from sqrtf and the division: d_invstd = 4.5 uf invstd.
  * primia_bn_fwd_train_pair (bn_apply_pair_kernel): z = relu(bn2(y2) + round_T(bn_d(yd))): E = E2 + (1 + us) E_d
    + us |bn_d| + uf (|bn2| + |bn_d|) for the add.

Backward (colreduce2_kernel<BwdFn>, bn_bwd_pair_reduce_kernel, bn_bwd_apply_kernel, bn_bwd_pair_apply_kernel).  The reference
takes what the kernel takes: y, dz, keep (the mask bytes, z > 0 of the z handed in, or — the forms that recompute it — the sign
of the exact fl(y - mean) * fl(invstd gamma) + beta, which is the sign of the kernel's fma), gamma, and save_mean / save_invstd
as the fp32 numbers they are: no conditioning term, and a ReLU decision near zero cannot fail a correct kernel.  With
g = dz keep and xhat = (y - mean) invstd in float64:
    dbeta  = sum g         d_dbeta  = chain uf sum|g| + uf |dbeta|
    dgamma = sum g xhat    d_dgamma = (chain + 3) uf sum|g xhat| + uf |dgamma|      (fl(y - mean), fl(. invstd), the product)
    dy = gamma invstd (g - dbeta / M - xhat dgamma / M)
    E  = |gamma invstd| (d_dbeta / M + |xhat| d_dgamma / M + 8 uf (|g| + |dbeta| / M + |xhat dgamma| / M))
    |dy - ref| <= (1 + us) E + us |ref| + 2^-126
  * 8: the term xhat * fl(dgamma * inv_m) carries 2 (xhat) + 2 (inv_m = (float)(1 / M), the product) + 1 (its own product),
    then the last subtraction, fl(gamma invstd) and the final product; the other two terms carry fewer.
GroupNorm (GnBwdFn, gn_bwd_finalize_kernel, gn_sample_reduce_kernel<1>, gn_bwd_apply_kernel): per-sample
ps_dbeta / ps_dgamma [N][C] as above (sums over HW); the group sums A = sum_c gamma_c ps_dbeta, B = sum_c gamma_c ps_dgamma are
formed in fp64 from the fp64 sums and cast once: d_A = sum_c |gamma_c| chain uf sum|g| + uf |A|, d_B likewise; m = HW C/G;
    dy = invstd (gamma g - A / m - xhat B / m)
    E  = invstd (d_A / m + |xhat| d_B / m + 7 uf (|gamma g| + |A| / m + |xhat B| / m))
  (7: as above without fl(gamma invstd)).
Exact checks, by bits: mask byte q has bit i set exactly when the kernel's own stored z[q CH + i] > 0; g_out is dz where kept and
+0 elsewhere.

Fused norm + ReLU + max-pool(3, 2, 1) (bn_relu_pool_fwd_kernel, bn_relu_pool_fwd_key_kernel; PoolScatterFn,
GnPoolScatterFn, bn_relu_pool_bwd_apply*_kernel, gn_relu_pool_bwd_apply2x2_kernel).
  * forward: the kernel takes the maximum of the ROUNDED activations; rounding is monotone, so that is the rounded maximum
    of the unrounded ones, and a maximum is 1-Lipschitz in the sup norm: with Ew the largest E among the window's taps inside
    the image, |pooled - max ref| <= (1 + us) Ew + us |max ref| + 2^-126 =: Bw.
  * every argmax byte is 0..8 and names a tap inside the image; the tap it names holds a rounded value no smaller than the
    true maximum's, so its reference lies within 2 Bw of the reference maximum.  (Tie order: the existing bit-identity test
    against the unfused chain.)
  * backward: the reference scatters dpooled through the kernel's OWN argmax codes: g(h, w) = keep(h, w) * sum of the <= 4
    windows that name (h, w), keep recomputed from y as above.  dy as above, plus |scale| 3 uf sum|dpooled terms| for the
    fp32 sum of the four windows.  dbeta / dgamma are summed per WINDOW: the sum|.| of their bounds runs over the windows'
    |dpooled| terms.
  * the pooled-resolution dgamma uses xhat = (p - beta) (1 / gamma) from the STORED p (PoolScatterFn, bn.hip:885-887):
    p = fl_T(v), v = the forward fma, so each term carries |g| (us |p| + 3 uf mag + 4 uf (|p| + |beta|)) / |gamma| more
    (store, the forward's k = 3 roundings on mag = |gamma| invstd |y - mean| + |beta|, then fl(p - beta), 1 / gamma to one
    ulp and the product), where pool_xhat_recoverable(gamma, beta); elsewhere xhat comes from y and the plain bound applies.

No constant here was taken from a run of a kernel.

What the bounds can and cannot see (measured with the stand-in of test_norm_bounds_host.py; figures in its docstrings):
  * the per-element z / dy bound is dominated by us |ref| in bf16: a neighbour's value, a fill value, a NaN, a truncating
    store (up to 2 ub |ref|) are seen; in fp32 everything down to a few uf is.
  * a save_invstd off by 1 % is always seen by the statistics check; the output check alone sees only the elements with
    |gamma| invstd |y - mean| 1 % > ub |ref| + ...: a fraction of the channel in bf16.
  * one row missing from dgamma / dbeta is seen while |term| > chain uf sum|terms|: with the slab-length chain (33 .. 257) at
    every M used here; the order-free chain = M stops seeing a typical term near M ~ 2^12.
  * it cannot see a wrong summation ORDER, a lost low bit of a well conditioned channel's variance, an error in a channel
    whose gamma is 0 other than in beta, or a wrong choice among pool taps whose values agree within 2 Bw.
"""
import functools
from collections import namedtuple

import torch

from tests.conv_bounds import BF16, F32, TINY, UB, UF, BoundError, _judge  # noqa: F401  (re-exported)

_TORCH = {BF16: torch.bfloat16, F32: torch.float32}
EPS = torch.tensor(1e-5, dtype=torch.float32).double().item()
MOMENTUM = torch.tensor(0.1, dtype=torch.float32).double().item()

BnCase = namedtuple("BnCase", "M C dtype")
PoolCase = namedtuple("PoolCase", "N H C dtype")               # BatchNorm stem tail, W = H
GnCase = namedtuple("GnCase", "N H C G dtype")                 # HW = H * H

# channels every BatchNorm case carries (C >= 8); CH_TINY is not pool_xhat_recoverable (|gamma| < 2^-6 |beta|), nor is CH_GAMMA0
CH_OFFSET, CH_ZERO, CH_CONST, CH_GAMMA0, CH_NEG, CH_TINY = 0, 1, 2, 3, 4, 5

BN_SHAPES = [(1, 64), (33, 8), (75, 512), (243, 128), (6272, 64), (32805, 256), (65573, 64)]
BN_CASES = [BnCase(M, C, dt) for M, C in BN_SHAPES for dt in (BF16, F32)]
# bn_bwd_apply_kernel<T, 2>: nchunks >= 4 * 2048 * 256 (bn.hip:996, :1758, :1789): 2 097 448 and 2 097 744 chunks
TWO_CHUNK_CASES = [BnCase(262181, 64, BF16), BnCase(131109, 64, F32)]
POOL_CASES = [PoolCase(N, H, 64, dt) for N, H in [(2, 16), (1, 9), (3, 14)] for dt in (BF16, F32)]
GN_SHAPES = [(3, 6, 64, 32), (3, 7, 256, 32), (130, 5, 128, 32), (130, 24, 64, 32), (2, 6, 64, 64), (2, 6, 512, 8),
             (130, 4, 512, 8)]
GN_CASES = [GnCase(*s, dt) for s in GN_SHAPES for dt in (BF16, F32)]


def case_id(c):
    return "x".join(str(v) for v in c[:-1]) + "-" + c.dtype


def chunk(dtype):
    """Elements per 16-byte chunk."""
    return 4 if dtype == F32 else 8


def us_of(dtype):
    return UF if dtype == F32 else UB


def rnd(x, dtype):
    return x.to(_TORCH[dtype]).to(torch.float32)


# ---- launch geometry restated (pinned by test_norm_bounds_host.py::test_geometry) -----------------------------------
def bn_slab_rows(M):
    """(blocks, rows per block) of BatchNorm's two-level reductions: reduce_geometry, bn.hip:948-958."""
    nb = min(max((M + 31) // 32, 1), 1024)
    rpb = (M + nb - 1) // nb
    return (M + rpb - 1) // rpb, rpb


def stream_blocks(nchunks):
    """Grid of the streaming apply kernels: stream_blocks, bn.hip:960-963."""
    return min(max((nchunks + 255) // 256, 1), 2048)


def two_chunk(M, C, dtype):
    return M * C // chunk(dtype) >= 4 * 2048 * 256


def gn_sample_blocks(N, C, dtype):
    """One 1024-thread block per sample: gn_sample_blocks, gn.hip:732-735."""
    tpr = C // chunk(dtype)
    return N >= 128 and 2 * C <= 1024 and 1024 % tpr == 0 and 1024 // tpr >= 1024 // (2 * C)


def gn_chain(N, HW, C, dtype):
    """Longest fp32 run of GroupNorm's reductions over HW rows: a slab of ceil(HW / kGnSlabs) rows (gn.hip:740, :768), or on
    the one-block-per-sample path one row group's share, ceil(HW / (1024 / threads per row)) (gn.hip:209, :222-225; the row
    groups are combined in fp64, :242)."""
    if gn_sample_blocks(N, C, dtype):
        rpp = 1024 // (C // chunk(dtype))
        return (HW + rpp - 1) // rpp
    return (HW + 31) // 32


def gn_apply_trips(N, HW, C, dtype):
    """Trips of a thread of gn_apply_kernel / gn_bwd_apply_kernel: gn_sample_grid, gn.hip:710-717."""
    cps = HW * (C // chunk(dtype))
    per = max(min((cps + 255) // 256, max((2048 + N - 1) // N, 1)), 1)
    return (cps + per * 256 - 1) // (per * 256)


def pool_out(H):
    return (H - 1) // 2 + 1


# ---- operands --------------------------------------------------------------------------------------------------------
def _params(C, g):
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = torch.randn(C, generator=g) * 0.5
    gamma[CH_GAMMA0] = 0.0
    gamma[CH_NEG] = -0.75
    gamma[CH_TINY], beta[CH_TINY] = 2.0 ** -8, 1.0
    return gamma, beta


@functools.lru_cache(maxsize=2)
def bn_operands(c):
    """fp32 tensors holding values of the compute type ([M, C]: y, yd, res, dz; keep: bool) and fp32 parameters.  Read-only:
    shared."""
    g = torch.Generator().manual_seed(7919 * c.C + c.M)
    M, C = c.M, c.C

    def act():
        t = torch.randn(M, C, generator=g) * (0.5 + 2.0 * torch.rand(C, generator=g)) + torch.randn(C, generator=g)
        t[:, CH_OFFSET] = 8.0 + 0.5 * torch.randn(M, generator=g)       # mean = 16 std
        t[:, CH_ZERO] = 0.0
        t[:, CH_CONST] = 0.3
        return rnd(t, c.dtype)

    o = dict(y=act(), dz=rnd(torch.randn(M, C, generator=g), c.dtype), keep=torch.rand(M, C, generator=g) > 0.4)
    o["gamma"], o["beta"] = _params(C, g)
    o["gamma_d"], o["beta_d"] = _params(C, g)
    o["rm0"], o["rv0"] = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    if M < 100000:                      # (the two-chunk cases run the backward pass only)
        o["yd"], o["res"] = act(), rnd(torch.randn(M, C, generator=g), c.dtype)
    return o


@functools.lru_cache(maxsize=2)
def pool_operands(c):
    """The BatchNorm operands of M = N H H rows plus dp [N Ho Wo, C]."""
    o = dict(bn_operands(BnCase(c.N * c.H * c.H, c.C, c.dtype)))
    g = torch.Generator().manual_seed(31 * c.H + c.N)
    o["dp"] = rnd(torch.randn(c.N * pool_out(c.H) ** 2, c.C, generator=g), c.dtype)
    return o


@functools.lru_cache(maxsize=2)
def gn_operands(c):
    """y, res, dz [N, HW, C], keep, dp [N, Ho Wo, C], gamma, beta.  Sample 0's group 0 has mean = 16 std, its group 1 is
    all zero, the last sample's group 1 is constant 0.3."""
    g = torch.Generator().manual_seed(104729 * c.G + 131 * c.C + 7 * c.H + c.N)
    N, HW, C, cpg = c.N, c.H * c.H, c.C, c.C // c.G
    y = torch.randn(N, HW, C, generator=g) * (0.5 + 2.0 * torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    y[0, :, 0:cpg] = 8.0 + 0.5 * torch.randn(HW, cpg, generator=g)
    y[0, :, cpg:2 * cpg] = 0.0
    y[N - 1, :, cpg:2 * cpg] = 0.3
    o = dict(y=rnd(y, c.dtype), res=rnd(torch.randn(N, HW, C, generator=g), c.dtype),
             dz=rnd(torch.randn(N, HW, C, generator=g), c.dtype), keep=torch.rand(N, HW, C, generator=g) > 0.4,
             dp=rnd(torch.randn(N, pool_out(c.H) ** 2, C, generator=g), c.dtype))
    o["gamma"], o["beta"] = _params(C, g)
    return o


def row_range_sums(a, b, slots):
    """[slots][2][C] fp32 partials of (sum a, sum b) over `slots` contiguous row ranges: float64 sums, rounded once."""
    M = a.shape[0]
    edges = [M * s // slots for s in range(slots + 1)]
    out = torch.zeros(slots, 2, a.shape[1], dtype=torch.float64)
    for s in range(slots):
        out[s, 0] = a[edges[s]:edges[s + 1]].double().sum(0)
        out[s, 1] = b[edges[s]:edges[s + 1]].double().sum(0)
    return out.to(torch.float32)


def mask_bytes(keep, ch):
    """One byte per chunk of `ch` elements, bit i = element i (the mask_out layout of bn_apply_kernel / gn_apply_kernel)."""
    bits = keep.reshape(-1, ch).to(torch.int32)
    return (bits << torch.arange(ch, dtype=torch.int32)).sum(1).to(torch.uint8)


def mask_bits(mask, ch, shape):
    m = torch.as_tensor(mask).cpu().reshape(-1, 1).to(torch.int32)
    return ((m >> torch.arange(ch, dtype=torch.int32)) & 1).bool().reshape(shape)


def _d(a, shape=None):
    t = torch.as_tensor(a).detach().cpu().to(torch.float64)
    return t.reshape(shape) if shape is not None else t


def _f(a):
    return torch.as_tensor(a).detach().cpu().to(torch.float32)


def gn_view(t, c):
    """[N, HW, C] -> [N, HW, G, C/G]."""
    return torch.as_tensor(t).detach().cpu().reshape(c.N, c.H * c.H, c.G, c.C // c.G)


# ---- forward statistics ------------------------------------------------------------------------------------------------
# mean .. d_invstd broadcast against the activations ([1, C] for BatchNorm, [N, 1, G, 1] for GroupNorm); n = elements per
# statistic; d_mean / d_invstd are those of the fp64 values, before the cast
Stats = namedtuple("Stats", "mean var invstd d_mean d_var d_invstd n")


def stats_ref(y, chain, dims=(0,)):
    """float64 two-pass reference over `dims` of y (values of the compute type) and the error of the kernel's sums."""
    y = _d(y)
    n = 1
    for d in dims:
        n *= y.shape[d]
    mean = y.sum(dims, keepdim=True) / n
    var = ((y - mean) ** 2).sum(dims, keepdim=True) / n
    d_mean = chain * UF * y.abs().sum(dims, keepdim=True) / n
    d_var = (chain + 1) * UF * (y * y).sum(dims, keepdim=True) / n + 2 * mean.abs() * d_mean + d_mean ** 2
    invstd = 1.0 / torch.sqrt(var + EPS)
    lo = 1.0 / torch.sqrt(var + d_var + EPS)
    hi = 1.0 / torch.sqrt((var - d_var).clamp_min(0.0) + EPS)
    return Stats(mean, var, invstd, d_mean, d_var, torch.maximum(invstd - lo, hi - invstd), n)


def gn_stats_ref(y, c, chain):
    return stats_ref(gn_view(y, c), chain, (1, 3))


def stored(st):
    """The bounds of save_mean / save_invstd as stored fp32 numbers (one cast each)."""
    return st.d_mean + UF * st.mean.abs(), st.d_invstd + UF * (st.invstd + st.d_invstd)


def given_stats(mean, invstd, like):
    """save_mean / save_invstd taken as exact inputs, shaped like the Stats `like`."""
    m, i = _d(mean).reshape(like.mean.shape), _d(invstd).reshape(like.mean.shape)
    z = torch.zeros_like(m)
    return Stats(m, None, i, z, z, z, like.n)


def check_stats(name, st, save_mean, save_invstd, running_mean=None, running_var=None, rm0=None, rv0=None,
                axes=("channel",)):
    """The worst err / bound of the per-statistic outputs; BoundError names the channel (or sample and group)."""
    dm, di = stored(st)
    shape = [s for s in st.mean.shape if s > 1] or [1]
    r = lambda t: _d(t).reshape(shape)   # noqa: E731
    worst = max(_judge(f"{name} save_mean", r(save_mean), r(st.mean), r(dm), axes),
                _judge(f"{name} save_invstd", r(save_invstd), r(st.invstd), r(di), axes))
    if running_mean is not None:
        unb = st.n / (st.n - 1) if st.n > 1 else 1.0
        ref_m = (1.0 - MOMENTUM) * r(rm0) + MOMENTUM * r(st.mean)
        ref_v = (1.0 - MOMENTUM) * r(rv0) + MOMENTUM * r(st.var) * unb
        worst = max(worst,
                    _judge(f"{name} running_mean", r(running_mean), ref_m, MOMENTUM * r(st.d_mean) + UF * ref_m.abs() + TINY, axes),
                    _judge(f"{name} running_var", r(running_var), ref_v, MOMENTUM * unb * r(st.d_var) + UF * ref_v.abs() + TINY,
                           axes))
    return worst


def eval_stats(running_mean, running_var):
    """Eval mode: the statistics are inputs; invstd = 1.f / sqrtf(var + eps) in fp32 (bn.hip:369)."""
    mean, var = _d(running_mean).reshape(1, -1), _d(running_var).reshape(1, -1)
    invstd = 1.0 / torch.sqrt(var + EPS)
    z = torch.zeros_like(mean)
    return Stats(mean, var, invstd, z, z, 4.5 * UF * invstd, 0)


# ---- forward output ----------------------------------------------------------------------------------------------------
RC_AXES = ("row", "channel")
GN_AXES = ("sample", "pixel", "group", "channel")
PIX_AXES = ("image", "row", "col", "channel")


def affine_ref(y, st, gamma, beta, res=None, train=True):
    """(ref, E, mag) of gamma invstd (y - mean) + beta [+ res] before the activation and the store; gamma / beta broadcast
    against y.  train: the statistics went through save_mean / save_invstd (one cast each)."""
    dm, di = stored(st) if train else (st.d_mean, st.d_invstd)
    y, gamma, beta = _d(y), _d(gamma), _d(beta)
    dev = y - st.mean
    ref = gamma * st.invstd * dev + beta
    mag = (gamma.abs() * st.invstd) * dev.abs() + beta.abs()
    k = 3
    if res is not None:
        ref, mag, k = ref + _d(res), mag + _d(res).abs(), 4
    E = gamma.abs() * ((st.invstd + di) * dm + dev.abs() * di) + k * UF * mag
    return ref, E, mag


def store_bound(ref, E, dtype):
    us = us_of(dtype)
    return (1.0 + us) * E + us * ref.abs() + TINY


def check_fwd(name, z, y, st, gamma, beta, res, relu, dtype, train=True, axes=RC_AXES):
    ref, E, _ = affine_ref(y, st, gamma, beta, res, train)
    if relu:
        ref = ref.clamp_min(0.0)
    return _judge(f"{name} z", _d(z, ref.shape), ref, store_bound(ref, E, dtype), axes)


def check_fwd_pair(name, z, y2, st2, gamma2, beta2, yd, std, gamma_d, beta_d, dtype):
    us = us_of(dtype)
    r2, E2, _ = affine_ref(y2, st2, gamma2, beta2)
    rd, Ed, _ = affine_ref(yd, std, gamma_d, beta_d)
    E = E2 + (1.0 + us) * Ed + us * rd.abs() + UF * (r2.abs() + rd.abs())
    ref = (r2 + rd).clamp_min(0.0)
    return _judge(f"{name} z", _d(z, ref.shape), ref, store_bound(ref, E, dtype), RC_AXES)


def _exact(name, what, bad, got, want, axes):
    if bad.any():
        pos = bad.nonzero()[:5].tolist()
        raise BoundError(f"{name} {what}: {int(bad.sum())} of {bad.numel()} differ, first at " + "; ".join(
            "(" + ", ".join(f"{a}={v}" for a, v in zip(axes, p)) + f"): got {got[tuple(p)].item():.6g} want "
            f"{want[tuple(p)].item():.6g}" for p in pos))
    return 0.0


def check_mask(name, mask, z, dtype, axes=RC_AXES):
    """Bit i of byte q set exactly when the STORED z[q CH + i] > 0."""
    z = _f(z)
    got = mask_bits(mask, chunk(dtype), z.shape)
    want = z > 0
    return _exact(name, "mask bits against the stored z", got != want, got.float(), want.float(), axes)


def relu_keep(y, mean, invstd, gamma, beta):
    """The ReLU decision the kernels recompute from y: fma(fl(y - mean), fl(invstd gamma), beta) > 0 (bn.hip:509 with :471;
    gn.hip:72-81); arguments broadcast.  The product of two fp32 numbers is exact in float64 and a float64 sum keeps the
    sign of the exact one."""
    dev = _f(y) - _f(mean)
    scale = _f(invstd) * _f(gamma)
    return dev.double() * scale.double() + _f(beta).double() > 0


def check_g_out(name, g_out, dz, keep, axes=RC_AXES):
    """g_out = dz where kept, +0 elsewhere, by bits."""
    g = _f(g_out).reshape(keep.shape)
    want = torch.where(keep, _f(dz).reshape(keep.shape), torch.zeros(()))
    return _exact(name, "g_out against dz * keep", g.view(torch.int32) != want.view(torch.int32), g, want, axes)


# ---- backward ----------------------------------------------------------------------------------------------------------
# one kernel's backward outputs and the chain of its reduction; dy = None: the parameter gradients only
Bwd = namedtuple("Bwd", "name dy dgamma dbeta chain")


def _pooled_extra(ga, gam, inv, dev, beta, us, dims):
    """What xhat = (p - beta) / gamma from the STORED pooled value adds to the bound of sum g xhat (see the docstring)."""
    mag = (gam * inv).abs() * dev.abs() + beta.abs()
    p = (gam * inv * dev + beta).clamp_min(0.0)
    rec = gam.abs() >= 2.0 ** -6 * beta.abs().clamp_min(1e-30)          # pool_xhat_recoverable, common.h:151
    extra = (ga * (us * p + 3 * UF * mag + 4 * UF * (p + beta.abs()))).sum(dims, keepdim=True) / gam.abs().clamp_min(1e-300)
    return torch.where(rec, extra, torch.zeros_like(extra))


def check_bn_bwd(name, dy, dgamma, dbeta, y, g, gamma, save_mean, save_invstd, chain, dtype, **kw):
    """One kernel's outputs: see check_bn_bwd_all.  Returns the worst ratios (dy, dgamma, dbeta)."""
    return check_bn_bwd_all([Bwd(name, dy, dgamma, dbeta, chain)], y, g, gamma, save_mean, save_invstd, dtype, **kw)[0]


def check_bn_bwd_all(outs, y, g, gamma, save_mean, save_invstd, dtype, block=16, g_abs=None, pooled_beta=None):
    """outs: a list of Bwd (dy [M, C], dgamma / dbeta [C]) of kernels that were given the same operands, judged against ONE
    float64 reference on (y, g = dz keep, gamma, save_mean, save_invstd), `block` channels at a time (a few float64
    [M, block] temporaries).  g_abs: the sum of the |terms| of g where g is itself a sum (the pool's gather).  pooled_beta:
    dgamma was summed with xhat from the stored pooled value.  Returns a list of the worst ratios (dy, dgamma, dbeta)."""
    y, g, gamma, mean, invstd = (torch.as_tensor(t).detach().cpu() for t in (y, g, gamma, save_mean, save_invstd))
    M, C = g.shape
    y = y.reshape(M, C)
    outs = [(o.name, None if o.dy is None else torch.as_tensor(o.dy).detach().cpu().reshape(M, C), _d(o.dgamma), _d(o.dbeta), o.chain)
            for o in outs]
    worst = [[0.0, 0.0, 0.0] for _ in outs]
    for c0 in range(0, C, block):
        s = slice(c0, min(c0 + block, C))
        ax_c = "channel" if c0 == 0 else f"{c0}+channel"
        gs = g[:, s].double()
        ga = gs.abs() if g_abs is None else torch.as_tensor(g_abs)[:, s].double()
        gam, inv = gamma[s].double(), invstd[s].double()
        dev = y[:, s].double() - mean[s].double()
        xhat = dev * inv
        ref_db, ref_dg = gs.sum(0), (gs * xhat).sum(0)
        A1, A2 = ga.sum(0), (ga * xhat.abs()).sum(0)
        extra = 0.0
        if pooled_beta is not None:
            extra = _pooled_extra(ga, gam, inv, dev, _d(pooled_beta)[s], us_of(dtype), 0)[0]
        scale = gam * inv
        a, b = ref_db / M, ref_dg / M
        ref = scale * (gs - a - xhat * b)
        mag = 8 * UF * (gs.abs() + a.abs() + (xhat * b).abs())
        if g_abs is not None:
            mag = mag + 3 * UF * ga
        for w, (n, got_dy, got_dg, got_db, ch) in zip(worst, outs):
            d_db = ch * UF * A1 + UF * ref_db.abs()
            d_dg = (ch + 3) * UF * A2 + UF * ref_dg.abs() + extra
            w[1] = max(w[1], _judge(f"{n} dgamma", got_dg[s], ref_dg, d_dg, (ax_c,)))
            w[2] = max(w[2], _judge(f"{n} dbeta", got_db[s], ref_db, d_db, (ax_c,)))
            if got_dy is not None:
                E = scale.abs() * (d_db / M + xhat.abs() * (d_dg / M) + mag)
                w[0] = max(w[0], _judge(f"{n} dy", got_dy[:, s].double(), ref, store_bound(ref, E, dtype), ("row", ax_c)))
    return [tuple(w) for w in worst]


def check_gn_bwd(name, dy, ps_dgamma, ps_dbeta, c, y, g, gamma, save_mean, save_invstd, chain, **kw):
    """One kernel's outputs: see check_gn_bwd_all.  Returns the worst ratios (dy, ps_dgamma, ps_dbeta)."""
    return check_gn_bwd_all([Bwd(name, dy, ps_dgamma, ps_dbeta, chain)], c, y, g, gamma, save_mean, save_invstd, **kw)[0]


def check_gn_bwd_all(outs, c, y, g, gamma, save_mean, save_invstd, g_abs=None, pooled_beta=None):
    """outs: a list of Bwd (dy [N, HW, C], ps_dgamma / ps_dbeta [N, C]) of GroupNorm case c; otherwise as check_bn_bwd_all."""
    N, HW, G, cpg = c.N, c.H * c.H, c.G, c.C // c.G
    y4, g4 = gn_view(y, c).double(), gn_view(g, c).double()
    ga = g4.abs() if g_abs is None else gn_view(g_abs, c).double()
    gam = _d(gamma).reshape(1, 1, G, cpg)
    mean, inv = _d(save_mean).reshape(N, 1, G, 1), _d(save_invstd).reshape(N, 1, G, 1)
    dev = y4 - mean
    xhat = dev * inv
    s1, s2 = g4.sum(1, keepdim=True), (g4 * xhat).sum(1, keepdim=True)                        # [N, 1, G, cpg]
    A1, A2 = ga.sum(1, keepdim=True), (ga * xhat.abs()).sum(1, keepdim=True)
    extra = 0.0
    if pooled_beta is not None:
        extra = _pooled_extra(ga, gam, inv, dev, _d(pooled_beta).reshape(1, 1, G, cpg), us_of(c.dtype), 1)
    m = HW * cpg
    A, B = (gam * s1).sum(3, keepdim=True), (gam * s2).sum(3, keepdim=True)                   # [N, 1, G, 1]
    ref = inv * (gam * g4 - A / m - xhat * B / m)
    mag = 7 * UF * ((gam * g4).abs() + A.abs() / m + (xhat * B).abs() / m)
    if g_abs is not None:
        mag = mag + gam.abs() * 3 * UF * ga
    ax = ("sample", "group", "channel")
    sq = lambda t: t.reshape(N, G, cpg)   # noqa: E731
    res = []
    for n, got_dy, got_dg, got_db, ch in outs:
        d1, d2 = ch * UF * A1, (ch + 3) * UF * A2 + extra
        w_dg = _judge(f"{n} ps_dgamma", _d(got_dg, (N, G, cpg)), sq(s2), sq(d2 + UF * s2.abs()), ax)
        w_db = _judge(f"{n} ps_dbeta", _d(got_db, (N, G, cpg)), sq(s1), sq(d1 + UF * s1.abs()), ax)
        w_dy = 0.0
        if got_dy is not None:
            dA = (gam.abs() * d1).sum(3, keepdim=True) + UF * A.abs()
            dB = (gam.abs() * d2).sum(3, keepdim=True) + UF * B.abs()
            E = inv * (dA / m + xhat.abs() * dB / m + mag)
            w_dy = _judge(f"{n} dy", _d(got_dy, ref.shape), ref, store_bound(ref, E, c.dtype), GN_AXES)
        res.append((w_dy, w_dg, w_db))
    return res


# ---- fused norm + ReLU + max-pool(3, 2, 1) -------------------------------------------------------------------------------
def pool_taps(t, fill):
    """t [N, H, W, C] -> the nine taps of every window [9, N, Ho, Wo, C] in scan order, `fill` outside the image."""
    N, H, W, C = t.shape
    Ho, Wo = pool_out(H), pool_out(W)
    p = torch.full((N, H + 2, W + 2, C), fill, dtype=t.dtype)
    p[:, 1:H + 1, 1:W + 1] = t
    return torch.stack([p[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] for r in range(3) for s in range(3)])


def check_pool_fwd(name, pooled, argmax, ref, E, dtype):
    """pooled / argmax [N, Ho, Wo, C] against ref = relu(norm(y)) [N, H, W, C] (float64) and its pre-store bound E."""
    us = us_of(dtype)
    taps = pool_taps(ref, float("-inf"))
    ref_p = taps.max(0).values
    Bw = (1.0 + us) * pool_taps(E, 0.0).max(0).values + us * ref_p.abs() + TINY
    worst = _judge(f"{name} pooled", _d(pooled, ref_p.shape), ref_p, Bw, PIX_AXES)
    code = torch.as_tensor(argmax).cpu().reshape(ref_p.shape).to(torch.int64)
    inside = code <= 8
    at = taps.gather(0, code.clamp(max=8).unsqueeze(0))[0]
    inside &= torch.isfinite(at)
    _exact(name, "argmax codes naming a tap inside the image", ~inside, code.float(), torch.full_like(ref_p, -1.0), PIX_AXES)
    gap = ref_p - at
    return max(worst, _judge(f"{name} argmax tap", gap, torch.zeros_like(gap), 2.0 * Bw, PIX_AXES))


def pool_scatter(dp, argmax, N, H, C):
    """(g, g_abs) [N, H, H, C]: dp [N, Ho, Wo, C] and its magnitude sent to the taps the argmax codes name."""
    Ho = pool_out(H)
    dp = _d(dp, (N, Ho, Ho, C))
    code = torch.as_tensor(argmax).cpu().reshape(N, Ho, Ho, C)
    g = torch.zeros(N, H + 2, H + 2, C, dtype=torch.float64)
    ga = torch.zeros_like(g)
    for k in range(9):
        r, s = divmod(k, 3)
        t = dp * (code == k)
        g[:, r:r + 2 * Ho - 1:2, s:s + 2 * Ho - 1:2] += t
        ga[:, r:r + 2 * Ho - 1:2, s:s + 2 * Ho - 1:2] += t.abs()
    return g[:, 1:H + 1, 1:H + 1].contiguous(), ga[:, 1:H + 1, 1:H + 1].contiguous()
