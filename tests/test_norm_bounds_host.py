"""tests/norm_bounds.py checked on the CPU: a stand-in plays each kernel of bn.hip / gn.hip (fp32 slab sums, fp64 finalize,
fp32 apply in the kernel's operand order, result stored in the compute type) and must stay inside every bound on every shape
of tests/test_gpu_norm_elementwise.py (worst err / bound printed with -s); planted faults must each be rejected at the position
planted.  No GPU, no marker."""
import re

import pytest
import torch

from tests import norm_bounds as nb
from tests.conv_bounds import check_guards
from tests.norm_bounds import BF16, F32, BoundError, case_id

# ---- the stand-in ------------------------------------------------------------------------------------------------------


def fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def store(v, dtype, truncate=False):
    if truncate and dtype == BF16:
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return nb.rnd(v, dtype)


def covered_rows(L, rpp, unroll, tail=True):
    """Rows of a slab of L that colreduce2_kernel's loops visit: row group rg walks rg, rg + rpp, ...; `unroll` rows per trip
    while a whole trip fits (bn.hip:41-44), the tail loop (:45) takes the rest."""
    keep = torch.ones(L, dtype=torch.bool)
    if tail:
        return keep
    for rg in range(min(rpp, L)):
        n = (L - rg + rpp - 1) // rpp
        for k in range(n // unroll * unroll, n):
            keep[rg + k * rpp] = False
    return keep


def slab_sums(t, rows, rpp=None, unroll=4, tail=True):
    """Two-level column sums of t [M, C] (fp32): fp32 within slabs of `rows`, fp64 across."""
    M = t.shape[0]
    tot = torch.zeros(t.shape[1], dtype=torch.float64)
    for r0 in range(0, M, rows):
        s = t[r0:r0 + rows]
        if not tail:
            s = s[covered_rows(s.shape[0], rpp, unroll, False)]
        tot += s.sum(0, dtype=torch.float32).double()
    return tot


def finalize(a, b, n):
    mean = a / n
    var = (b / n - mean * mean).clamp_min(0.0)
    return mean, var, 1.0 / torch.sqrt(var + nb.EPS)


def sim_bn_stats(y, rows, rm0=None, rv0=None, partials=None, lossy=False, **kw):
    """save_mean, save_invstd, running_mean, running_var.  partials [slots][2][C]: the *_from_sums forms.  lossy: the sum of
    squares loses its low bits (rounded to bf16)."""
    M = y.shape[0]
    if partials is not None:
        a, b = partials[:, 0].double().sum(0), partials[:, 1].double().sum(0)
    else:
        a, b = slab_sums(y, rows, **kw), slab_sums(y * y, rows, **kw)
    if lossy:
        b = b.to(torch.bfloat16).double()
    mean, var, invstd = finalize(a, b, M)
    out = [mean.float(), invstd.float()]
    if rm0 is not None:
        unb = var * M / (M - 1) if M > 1 else var
        out += [((1.0 - nb.MOMENTUM) * rm0.double() + nb.MOMENTUM * mean).float(),
                ((1.0 - nb.MOMENTUM) * rv0.double() + nb.MOMENTUM * unb).float()]
    return out


def sim_apply(y, res, mean, invstd, gamma, beta, relu, dtype, truncate=False):
    v = fma32(y - mean, invstd * gamma, beta)
    if res is not None:
        v = v + res
    if relu:
        v = v.clamp_min(0.0)
    return store(v, dtype, truncate)


def sim_eval_invstd(var):
    return 1.0 / torch.sqrt(var + torch.tensor(1e-5, dtype=torch.float32))


def sim_bn_bwd(y, g, gamma, mean, invstd, rows, dtype, M=None, partials=None, **kw):
    """dy, dgamma, dbeta (bn_bwd_impl; M: the rows of the statistics when g is gathered from a pool)."""
    M = M or y.shape[0]
    xh = (y - mean) * invstd
    if partials is not None:
        s1, s2 = partials[:, 0].double().sum(0), partials[:, 1].double().sum(0)
    else:
        s1, s2 = slab_sums(g, rows, **kw), slab_sums(g * xh, rows, **kw)
    dbeta, dgamma = s1.float(), s2.float()
    inv_m = torch.tensor(1.0 / M, dtype=torch.float64).float()
    dy = (gamma * invstd) * (g - dbeta * inv_m - xh * (dgamma * inv_m))
    return store(dy, dtype), dgamma, dbeta


def sim_pool_fwd(z4):
    """pooled, argmax of stored activations z4 [N, H, W, C]: first maximum in scan order."""
    taps = nb.pool_taps(z4, float("-inf"))
    best = torch.full(taps.shape[1:], float("-inf"))
    pos = torch.zeros(taps.shape[1:], dtype=torch.uint8)
    for k in range(9):
        up = taps[k] > best
        best = torch.where(up, taps[k], best)
        pos = torch.where(up, torch.full_like(pos, k), pos)
    return best, pos


def sim_pool_sums(p, dp, argmax, y4, mean, invstd, gamma, beta):
    """Per-window terms of (sum g, sum g xhat) at pooled resolution (PoolScatterFn / GnPoolScatterFn); mean / invstd
    broadcast against [N, Ho, Wo, C]."""
    g = torch.where(p > 0, dp, torch.zeros(()))
    rec = gamma.abs() >= 2.0 ** -6 * beta.abs().clamp_min(1e-30)
    xh = (p - beta) * torch.where(rec, 1.0 / gamma, torch.zeros(()))
    y_at = nb.pool_taps(y4, 0.0).gather(0, argmax.to(torch.int64).unsqueeze(0))[0]
    xh = torch.where(rec, xh, (y_at - mean) * invstd)
    return g, g * xh


def gn_sums(t, c, rows):
    """[N, C] two-level sums over the HW rows of every sample.  On the one-block-per-sample shapes the kernel's fp32 runs are a
    row group's STRIDED share of `rows` rows (gn.hip:222-225), here contiguous slabs of `rows`: the bound is order-free within
    a run of that length, so either grouping must stay inside it."""
    return torch.stack([slab_sums(t[n], rows) for n in range(c.N)])


def sim_gn_stats(y, c, rows):
    N, G, cpg = c.N, c.G, c.C // c.G
    a = gn_sums(y, c, rows).reshape(N, G, cpg).sum(2)
    b = gn_sums(y * y, c, rows).reshape(N, G, cpg).sum(2)
    mean, _, invstd = finalize(a, b, c.H * c.H * cpg)
    return mean.float(), invstd.float()


def per_channel(t, c):
    """[N, G] -> [N, 1, C]."""
    return t.repeat_interleave(c.C // c.G, dim=1).unsqueeze(1)


def sim_gn_bwd(y, g, gamma, mean, invstd, c, rows, s1=None, s2=None):
    """dy, ps_dgamma, ps_dbeta (gn_bwd_impl)."""
    N, G, cpg = c.N, c.G, c.C // c.G
    mu, inv = per_channel(mean, c), per_channel(invstd, c)
    xh = (y - mu) * inv
    if s1 is None:
        s1, s2 = gn_sums(g, c, rows), gn_sums(g * xh, c, rows)
    A = (gamma.double() * s1).reshape(N, G, cpg).sum(2).float()
    B = (gamma.double() * s2).reshape(N, G, cpg).sum(2).float()
    inv_m = torch.tensor(1.0 / (c.H * c.H * cpg), dtype=torch.float64).float()
    dy = inv * (gamma * g - per_channel(A, c) * inv_m - xh * (per_channel(B, c) * inv_m))
    return store(dy, c.dtype), s2.float(), s1.float()


def show(what, c, ratio):
    print(f"norm-bound stand-in {what} case={case_id(c)} worst={ratio:.3g}")
    assert ratio <= 1.0


# ---- the stand-in stays inside every bound -----------------------------------------------------------------------------
def test_geometry():
    """The launch geometry norm_bounds.py restates, at the shapes used: reduce_geometry (bn.hip:948-958), stream_blocks
    (:960-963), the two-chunk threshold (:996), gn_sample_blocks / kGnSlabs / gn_sample_grid (gn.hip:17, :710-735)."""
    assert [nb.bn_slab_rows(M) for M, _ in nb.BN_SHAPES] == [(1, 1), (2, 17), (3, 25), (8, 31), (196, 32), (995, 33), (1009, 65)]
    assert nb.bn_slab_rows(32768) == (1024, 32) and nb.bn_slab_rows(32769) == (993, 33)
    assert [nb.bn_slab_rows(c.M) for c in nb.TWO_CHUNK_CASES] == [(1021, 257), (1017, 129)]
    assert nb.stream_blocks(8) == 1 and nb.stream_blocks(524289) == 2048
    # a second grid-stride trip of the apply kernels: more than 2048 * 256 chunks
    assert 65573 * 64 // 8 == 524584 and 524584 - 2048 * 256 == 296
    for c in nb.TWO_CHUNK_CASES:
        nch = c.M * c.C // nb.chunk(c.dtype)
        assert nch == {BF16: 2097448, F32: 2097744}[c.dtype] and nb.two_chunk(c.M, c.C, c.dtype) and not nb.two_chunk(c.M - 38, c.C, c.dtype)
    assert [nb.gn_sample_blocks(N, C, dt) for N, _, C, _ in nb.GN_SHAPES for dt in (BF16,)] == [False, False, True, True, False,
                                                                                                False, True]
    assert nb.gn_sample_blocks(130, 512, F32) and nb.gn_chain(130, 16, 512, BF16) == 1 and nb.gn_chain(130, 16, 512, F32) == 2
    assert nb.gn_chain(3, 36, 64, BF16) == 2 and nb.gn_chain(130, 576, 64, BF16) == 5 and nb.gn_chain(130, 576, 64, F32) == 9
    assert nb.gn_apply_trips(130, 576, 64, BF16) == 2 and nb.gn_apply_trips(130, 25, 128, BF16) == 1
    assert nb.gn_apply_trips(130, 576, 64, F32) == 3


def two_chunk_walk(nchunks, guard=True):
    """The chunks bn_bwd_apply_kernel<T, 2> stores (bn.hip:477-520): per trip a thread takes q0 and q0 + stride; the second is
    skipped when past the end (`if (q >= nchunks) break`)."""
    stride = nb.stream_blocks(nchunks) * 256
    q0 = torch.arange(0, nchunks, dtype=torch.int64)
    q0 = q0[(q0 // stride) % 2 == 0]                    # first chunks: trips start at t, t + 2 stride, ...
    q1 = q0 + stride
    live = q1 < nchunks
    return q0, q1 if not guard else q1[live], int((~live).sum())


def test_two_chunk_walk():
    """The index walk of the two-chunk backward at the shapes of the GPU test: 2 097 448 = 4 * 524 288 + 296 chunks, every chunk
    stored once; the third trip has 296 live threads whose second chunk lies one grid stride past their first, behind the end.
    The load clamp (`qc = q < nchunks ? q : q0`) keeps that read inside y; the value is dropped by `if (q >= nchunks) break`.
    Without the break those threads store 296 chunks at end + 524 288 - 296 chunks: test_bn_two_chunk_backward keeps a guard
    band of one grid stride behind dy and g_out, and its check names them (modelled here with one element per chunk)."""
    nch = 2097448
    stride = nb.stream_blocks(nch) * 256
    q0, q1, clamped = two_chunk_walk(nch)
    assert clamped == 296 and torch.equal(torch.cat([q0, q1]).sort().values, torch.arange(nch))
    q0, q1, _ = two_chunk_walk(nch, guard=False)
    over = q1[q1 >= nch]
    assert over.numel() == 296 and int(over.min()) - nch == stride - 296 and int(over.max()) - nch < stride
    arena = torch.full((256 + nch + stride + 256,), -123.0)
    arena[256:256 + nch] = 0.0
    arena[256 + over] = 1.0
    with pytest.raises(BoundError, match=rf"296 elements.*end\+{stride - 296}"):
        check_guards(arena, 256, 256 + nch, -123.0)


def bn_forward_all(c, o, report=show):
    """Every forward form of case c on the stand-in; returns z of the residual + ReLU form and the saved statistics
    of both BatchNorms."""
    M, C = c.M, c.C
    y, res, gamma, beta = o["y"], o["res"], o["gamma"], o["beta"]
    rows = nb.bn_slab_rows(M)[1]
    st = nb.stats_ref(y, rows)
    sm, si, rm, rv = sim_bn_stats(y, rows, o["rm0"], o["rv0"])
    report("stats", c, nb.check_stats("fwd_train", st, sm, si, rm, rv, o["rm0"], o["rv0"]))
    for r, relu in ((None, 0), (res, 1)):
        z = sim_apply(y, r, sm, si, gamma, beta, relu, c.dtype)
        report(f"fwd_train res={r is not None} relu={relu}", c, nb.check_fwd("fwd_train", z, y, st, gamma, beta, r, relu, c.dtype))
    # from_sums: chain 1
    parts = nb.row_range_sums(y.double(), y.double() ** 2, 3)
    st1 = nb.stats_ref(y, 1)
    sm1, si1, rm1, rv1 = sim_bn_stats(y, rows, o["rm0"], o["rv0"], partials=parts)
    report("from_sums stats", c, nb.check_stats("from_sums", st1, sm1, si1, rm1, rv1, o["rm0"], o["rv0"]))
    z1 = sim_apply(y, None, sm1, si1, gamma, beta, 1, c.dtype)
    report("from_sums", c, nb.check_fwd("from_sums", z1, y, st1, gamma, beta, None, 1, c.dtype))
    # apply_inline: the same statistics, mask + residual
    zi = sim_apply(y, res, sm1, si1, gamma, beta, 1, c.dtype)
    report("apply_inline", c, nb.check_fwd("apply_inline", zi, y, st1, gamma, beta, res, 1, c.dtype))
    nb.check_mask("apply_inline", nb.mask_bytes(zi > 0, nb.chunk(c.dtype)), zi, c.dtype)
    # eval (residual, no ReLU) and eval_mask (residual + ReLU + mask)
    ste = nb.eval_stats(o["rm0"], o["rv0"])
    for name, relu in (("eval", 0), ("eval_mask", 1)):
        ze = sim_apply(y, res, o["rm0"], sim_eval_invstd(o["rv0"]), gamma, beta, relu, c.dtype)
        report(name, c, nb.check_fwd(name, ze, y, ste, gamma, beta, res, relu, c.dtype, train=False))
    nb.check_mask("eval_mask", nb.mask_bytes(ze > 0, nb.chunk(c.dtype)), ze, c.dtype)
    # pair
    yd = o["yd"]
    std = nb.stats_ref(yd, rows)
    smd, sid = sim_bn_stats(yd, rows)
    idn = sim_apply(yd, None, smd, sid, o["gamma_d"], o["beta_d"], 0, c.dtype)
    zp = sim_apply(y, idn, sm, si, gamma, beta, 1, c.dtype)
    report("pair", c, nb.check_fwd_pair("pair", zp, y, st, gamma, beta, yd, std, o["gamma_d"], o["beta_d"], c.dtype))
    nb.check_mask("mask", nb.mask_bytes(z > 0, nb.chunk(c.dtype)), z, c.dtype)
    return z, sm, si, smd, sid


@pytest.mark.parametrize("c", nb.BN_CASES, ids=case_id)
def test_standin_batchnorm(c):
    o = nb.bn_operands(c)
    M = c.M
    rows = nb.bn_slab_rows(M)[1]
    z, sm, si, smd, sid = bn_forward_all(c, o)
    y, dz, gamma = o["y"], o["dz"], o["gamma"]
    for name, keep in (("bwd z", z > 0), ("bwd mask", o["keep"]), ("relu_bwd", nb.relu_keep(y, sm, si, gamma, o["beta"]))):
        g = torch.where(keep, dz, torch.zeros(()))
        dy, dg, db = sim_bn_bwd(y, g, gamma, sm, si, rows, c.dtype)
        nb.check_g_out(name, g, dz, keep)
        for what, r in zip(("dy", "dgamma", "dbeta"), nb.check_bn_bwd(name, dy, dg, db, y, g, gamma, sm, si, rows, c.dtype)):
            show(f"{name} {what}", c, r)
    # from_sums: chain 1
    g = torch.where(o["keep"], dz, torch.zeros(()))
    xh = (y.double() - sm.double()) * si.double()
    parts = nb.row_range_sums(g.double(), g.double() * xh, 5)
    dy, dg, db = sim_bn_bwd(y, g, gamma, sm, si, rows, c.dtype, partials=parts)
    for what, r in zip(("dy", "dgamma", "dbeta"), nb.check_bn_bwd("from_sums", dy, dg, db, y, g, gamma, sm, si, 1, c.dtype)):
        show(f"bwd from_sums {what}", c, r)
    # pair: the downsample branch with the same g
    dyd, dgd, dbd = sim_bn_bwd(o["yd"], g, o["gamma_d"], smd, sid, rows, c.dtype)
    for what, r in zip(("dyd", "dgamma_d", "dbeta_d"),
                       nb.check_bn_bwd("pair", dyd, dgd, dbd, o["yd"], g, o["gamma_d"], smd, sid, rows, c.dtype)):
        show(f"bwd pair {what}", c, r)


@pytest.mark.parametrize("c", nb.TWO_CHUNK_CASES, ids=case_id)
def test_standin_two_chunk_backward(c):
    o = nb.bn_operands(c)
    y, dz, gamma = o["y"], o["dz"], o["gamma"]
    rows = nb.bn_slab_rows(c.M)[1]
    sm, si = sim_bn_stats(y, rows)
    g = torch.where(o["keep"], dz, torch.zeros(()))
    dy, dg, db = sim_bn_bwd(y, g, gamma, sm, si, rows, c.dtype)
    for what, r in zip(("dy", "dgamma", "dbeta"), nb.check_bn_bwd("bwd_mask", dy, dg, db, y, g, gamma, sm, si, rows, c.dtype)):
        show(f"bwd_mask {what}", c, r)


def pool_forward(c, o, rows):
    N, H, C = c.N, c.H, c.C
    y, gamma, beta = o["y"], o["gamma"], o["beta"]
    st = nb.stats_ref(y, rows)
    sm, si = sim_bn_stats(y, rows)
    z = sim_apply(y, None, sm, si, gamma, beta, 1, c.dtype)
    p, am = sim_pool_fwd(z.reshape(N, H, H, C))
    ref, E, _ = nb.affine_ref(y, st, gamma, beta)
    return st, sm, si, p, am, ref.clamp_min(0.0).reshape(N, H, H, C), E.reshape(N, H, H, C)


@pytest.mark.parametrize("c", nb.POOL_CASES, ids=case_id)
def test_standin_stem_tail(c):
    o = nb.pool_operands(c)
    N, H, C = c.N, c.H, c.C
    M, Ho = N * H * H, nb.pool_out(H)
    y, gamma, beta = o["y"], o["gamma"], o["beta"]
    st, sm, si, p, am, ref, E = pool_forward(c, o, nb.bn_slab_rows(M)[1])
    show("pool fwd", c, nb.check_pool_fwd("pool", p, am, ref, E, c.dtype))
    dp = o["dp"].reshape(N, Ho, Ho, C)
    rows_p = nb.bn_slab_rows(N * Ho * Ho)[1]
    t1, t2 = sim_pool_sums(p, dp, am, y.reshape(N, H, H, C), sm, si, gamma, beta)
    s1, s2 = slab_sums(t1.reshape(-1, C), rows_p), slab_sums(t2.reshape(-1, C), rows_p)
    keep = nb.relu_keep(y, sm, si, gamma, beta)
    g, ga = (t.reshape(M, C) * keep for t in nb.pool_scatter(dp, am, N, H, C))
    dy, dg, db = sim_bn_bwd(y, g.float(), gamma, sm, si, 0, c.dtype, partials=torch.stack([s1, s2]).float().unsqueeze(0))
    for what, r in zip(("dy", "dgamma", "dbeta"), nb.check_bn_bwd("pool bwd", dy, dg, db, y, g, gamma, sm, si, rows_p, c.dtype,
                                                                  g_abs=ga, pooled_beta=beta)):
        show(f"pool bwd {what}", c, r)


def gn_forward(c, o, chain):
    y, res, gamma, beta = o["y"], o["res"], o["gamma"], o["beta"]
    st = nb.gn_stats_ref(y, c, chain)
    sm, si = sim_gn_stats(y, c, chain)
    show("gn stats", c, nb.check_stats("gn", st, sm, si, axes=("sample", "group")))
    mu, inv = per_channel(sm, c), per_channel(si, c)
    out = []
    for r, relu in ((None, 0), (res, 1)):
        z = sim_apply(y, r, mu, inv, gamma, beta, relu, c.dtype)
        show(f"gn fwd res={r is not None}", c, nb.check_fwd("gn", nb.gn_view(z, c), nb.gn_view(y, c), st, nb.gn_view(gamma, c._replace(N=1, H=1)),
                                                           nb.gn_view(beta, c._replace(N=1, H=1)), None if r is None else nb.gn_view(r, c),
                                                           relu, c.dtype, axes=nb.GN_AXES))
        out.append(z)
    return st, sm, si, out[1]


@pytest.mark.parametrize("c", nb.GN_CASES, ids=case_id)
def test_standin_groupnorm(c):
    o = nb.gn_operands(c)
    N, H, C = c.N, c.H, c.C
    chain = nb.gn_chain(N, H * H, C, c.dtype)
    y, dz, gamma, beta = o["y"], o["dz"], o["gamma"], o["beta"]
    st, sm, si, z = gn_forward(c, o, chain)
    mu, inv = per_channel(sm, c), per_channel(si, c)
    for name, keep in (("gn bwd z", z > 0), ("gn bwd mask", o["keep"])):
        g = torch.where(keep, dz, torch.zeros(()))
        dy, dg, db = sim_gn_bwd(y, g, gamma, sm, si, c, chain)
        for what, r in zip(("dy", "ps_dgamma", "ps_dbeta"), nb.check_gn_bwd(name, dy, dg, db, c, y, g, gamma, sm, si, chain)):
            show(f"{name} {what}", c, r)
    # no residual: the keep primia_gn_relu_bwd recomputes from y
    g = torch.where(nb.relu_keep(y, mu, inv, gamma, beta), dz, torch.zeros(()))
    dy, dg, db = sim_gn_bwd(y, g, gamma, sm, si, c, chain)
    for what, r in zip(("dy", "ps_dgamma", "ps_dbeta"), nb.check_gn_bwd("gn relu_bwd", dy, dg, db, c, y, g, gamma, sm, si, chain)):
        show(f"gn relu_bwd {what}", c, r)
    # stem tail
    zs = sim_apply(y, None, mu, inv, gamma, beta, 1, c.dtype)
    p, am = sim_pool_fwd(zs.reshape(N, H, H, C))
    g4 = lambda t: nb.gn_view(t, c._replace(N=1, H=1))   # noqa: E731
    ref, E, _ = nb.affine_ref(nb.gn_view(y, c), st, g4(gamma), g4(beta))
    show("gn pool fwd", c, nb.check_pool_fwd("gn pool", p, am, ref.clamp_min(0.0).reshape(N, H, H, C), E.reshape(N, H, H, C), c.dtype))
    if H % 2:
        return          # primia_gn_relu_maxpool_bwd serves even sizes only (gn.hip:932)
    Ho = nb.pool_out(H)
    cp = c._replace(H=Ho)
    chain_p = nb.gn_chain(N, Ho * Ho, C, c.dtype)
    dp = o["dp"].reshape(N, Ho, Ho, C)
    t1, t2 = sim_pool_sums(p, dp, am, y.reshape(N, H, H, C), mu.reshape(N, 1, 1, C), inv.reshape(N, 1, 1, C), gamma, beta)
    s1, s2 = gn_sums(t1.reshape(N, -1, C), cp, chain_p), gn_sums(t2.reshape(N, -1, C), cp, chain_p)
    keep = nb.relu_keep(y, mu, inv, gamma, beta)
    g, ga = (t.reshape(N, H * H, C) * keep for t in nb.pool_scatter(dp, am, N, H, C))
    dy, dg, db = sim_gn_bwd(y, g.float(), gamma, sm, si, c, 0, s1, s2)
    for what, r in zip(("dy", "ps_dgamma", "ps_dbeta"),
                       nb.check_gn_bwd("gn pool bwd", dy, dg, db, c, y, g, gamma, sm, si, chain_p, g_abs=ga, pooled_beta=beta)):
        show(f"gn pool bwd {what}", c, r)


# ---- planted faults ----------------------------------------------------------------------------------------------------
FAULT = nb.BnCase(243, 128, BF16)            # ragged: 243 rows, 8 slabs of 31


def _at(msg, **pos):
    """The message's worst position is the one planted."""
    first = str(msg).split("worst at ")[-1].split(";")[0]
    return all(re.search(rf"{k}={v}\b", first) for k, v in pos.items())


@pytest.fixture(scope="module")
def fault_base():
    o = nb.bn_operands(FAULT)
    rows = nb.bn_slab_rows(FAULT.M)[1]
    st = nb.stats_ref(o["y"], rows)
    sm, si = sim_bn_stats(o["y"], rows)
    z = sim_apply(o["y"], o["res"], sm, si, o["gamma"], o["beta"], 1, BF16)
    g = torch.where(o["keep"], o["dz"], torch.zeros(()))
    dy, dg, db = sim_bn_bwd(o["y"], g, o["gamma"], sm, si, rows, BF16)
    return o, rows, st, sm, si, z, g, dy, dg, db


def test_fault_neighbour_element(fault_base):
    """One element of z / dy replaced by its row neighbour's (the next channel of the same row)."""
    o, rows, st, sm, si, z, g, dy, dg, db = fault_base
    for name, t in (("z", z), ("dy", dy)):
        d = (t[:, 6:-1] - t[:, 7:]).abs()
        r, ch = divmod(int(d.argmax()), d.shape[1])
        bad = t.clone()
        bad[r, ch + 6] = t[r, ch + 7]
        with pytest.raises(BoundError) as e:
            if name == "z":
                nb.check_fwd("t", bad, o["y"], st, o["gamma"], o["beta"], o["res"], 1, BF16)
            else:
                nb.check_bn_bwd("t", bad, dg, db, o["y"], g, o["gamma"], sm, si, rows, BF16, block=128)
        assert "1 of" in str(e.value) and _at(e.value, row=r, channel=ch + 6)


@pytest.mark.parametrize("fill", [-123.0, float("nan")])
def test_fault_last_row_not_written(fault_base, fill):
    o, rows, st, sm, si, z, g, dy, dg, db = fault_base
    bad = z.clone()
    bad[-1] = fill
    with pytest.raises(BoundError) as e:
        nb.check_fwd("t", bad, o["y"], st, o["gamma"], o["beta"], o["res"], 1, BF16)
    assert "row=242" in str(e.value) and "row=241" not in str(e.value)
    bad = dy.clone()
    bad[-1] = fill
    with pytest.raises(BoundError) as e:
        nb.check_bn_bwd("t", bad, dg, db, o["y"], g, o["gamma"], sm, si, rows, BF16, block=128)
    assert "row=242" in str(e.value) and "row=241" not in str(e.value)


def test_fault_invstd_one_percent(fault_base):
    """One channel's save_invstd off by 1 %: the statistics check names the channel.  The output check alone sees only part
    of that channel's elements (bf16: those whose 1 % of |gamma| invstd |y - mean| exceeds ub |ref| and the rest of the
    bound) — measured on the stand-in at 243 x 128: 30 % .. 44 % of the elements of channels 7 .. 12; printed with -s."""
    o, rows, st, sm, si, z, g, dy, dg, db = fault_base
    shares = []
    for ch in range(7, 13):
        bad = si.clone()
        bad[ch] *= 1.01
        with pytest.raises(BoundError) as e:
            nb.check_stats("t", st, sm, bad)
        assert "save_invstd" in str(e.value) and _at(e.value, channel=ch)
        zb = sim_apply(o["y"], o["res"], sm, bad, o["gamma"], o["beta"], 1, BF16)
        ref, E, _ = nb.affine_ref(o["y"], st, o["gamma"], o["beta"], o["res"])
        ref = ref.clamp_min(0.0)
        out = (zb.double() - ref).abs() > nb.store_bound(ref, E, BF16)
        assert not out[:, :ch].any() and not out[:, ch + 1:].any()
        shares.append(out[:, ch].float().mean().item())
    print("share of the channel's z elements the output check sees:", " ".join(f"{s:.2f}" for s in shares))
    assert 0.0 < min(shares) and max(shares) < 0.6


def test_fault_truncating_store(fault_base):
    o, rows, st, sm, si, z, g, dy, dg, db = fault_base
    bad = sim_apply(o["y"], o["res"], sm, si, o["gamma"], o["beta"], 1, BF16, truncate=True)
    with pytest.raises(BoundError, match="z:"):
        nb.check_fwd("t", bad, o["y"], st, o["gamma"], o["beta"], o["res"], 1, BF16)


def test_fault_row_missing_from_sums():
    """One row left out of dgamma / dbeta.  A term t is seen while |t| > chain uf sum|t| ~ chain M uf mean|t|.  With the slab
    length as `chain` (<= 257 here) that is 0.25 mean|t| at M = 65 573 and less at every other M of the suite.  The order-free
    chain = M needs |t| > M^2 uf mean|t|: a typical term is seen only up to M = 2^12; the row is still rejected at M = 243
    and no longer at M = 65 573 (terms below 256 mean|t|)."""
    for M, order_free_sees in ((243, True), (65573, False)):
        c = nb.BnCase(M, 64, BF16)
        o = nb.bn_operands(c)
        rows = nb.bn_slab_rows(M)[1]
        y, gamma = o["y"], o["gamma"]
        sm, si = sim_bn_stats(y, rows)
        g = torch.where(o["keep"], o["dz"], torch.zeros(()))
        gm = g.clone()
        r = int(g[:, 8:].abs().min(1).values.argmax())       # a row whose terms are all of ordinary size
        gm[r] = 0.0
        _, dg, db = sim_bn_bwd(y, gm, gamma, sm, si, rows, BF16)
        with pytest.raises(BoundError, match="dgamma|dbeta"):
            nb.check_bn_bwd("t", None, dg, db, y, g, gamma, sm, si, rows, BF16, block=64)
        if order_free_sees:
            with pytest.raises(BoundError):
                nb.check_bn_bwd("t", None, dg, db, y, g, gamma, sm, si, M, BF16, block=64)
        else:
            nb.check_bn_bwd("t", None, dg, db, y, g, gamma, sm, si, M, BF16, block=64)


def test_fault_colreduce_tail():
    """colreduce2_kernel without its `r < r1` tail loop (bn.hip:45): at 32 805 x 256 a slab has 33 rows on 8 (bf16) row
    groups, the unrolled loop takes 4 rows per trip and group: group 0's fifth row is dropped.  Statistics and backward sums
    leave their bounds."""
    c = nb.BnCase(32805, 256, BF16)
    o = nb.bn_operands(c)
    rows = nb.bn_slab_rows(c.M)[1]
    rpp = 256 // (c.C // 8)
    assert rows == 33 and rpp == 8 and int((~covered_rows(33, rpp, 4, tail=False)).sum()) == 1
    y = o["y"]
    st = nb.stats_ref(y, rows)
    sm, si = sim_bn_stats(y, rows, rpp=rpp, unroll=4, tail=False)
    with pytest.raises(BoundError, match="save_mean"):
        nb.check_stats("t", st, sm, si)
    sm, si = sim_bn_stats(y, rows)
    g = torch.where(o["keep"], o["dz"], torch.zeros(()))
    _, dg, db = sim_bn_bwd(y, g, o["gamma"], sm, si, rows, BF16, rpp=rpp, unroll=2, tail=False)
    with pytest.raises(BoundError, match="dgamma|dbeta"):
        nb.check_bn_bwd("t", None, dg, db, y, g, o["gamma"], sm, si, rows, BF16, block=64)


def test_fault_lossy_variance(fault_base):
    """sum y^2 / M - mean^2 on a sum of squares that lost its low bits (rounded to bf16): a relative error d of the sum moves
    invstd by d (1 + mean^2 / var) / 2 — 128 d in the offset channel (mean = 16 std), where the fault in that channel alone is
    rejected; the bound scales with the same factor, so every channel with data sees its own."""
    o, rows, st, sm, si, *_ = fault_base
    sm2, si2 = sim_bn_stats(o["y"], rows, lossy=True)
    bad = si.clone()
    bad[nb.CH_OFFSET] = si2[nb.CH_OFFSET]
    assert abs(bad[0] / si[0] - 1) > 1e-2
    with pytest.raises(BoundError) as e:
        nb.check_stats("t", st, sm, bad)
    assert "save_invstd: 1 of 128" in str(e.value) and _at(e.value, channel=nb.CH_OFFSET)
    with pytest.raises(BoundError, match="save_invstd: 127 of 128"):       # all but the all-zero channel
        nb.check_stats("t", st, sm2, si2)


def test_fault_mask_bit(fault_base):
    o, rows, st, sm, si, z, *_ = fault_base
    m = nb.mask_bytes(z > 0, 8)
    nb.check_mask("t", m, z, BF16)
    m[(100 * 128 + 40) // 8] ^= 1 << 3
    with pytest.raises(BoundError, match=r"row=100, channel=43"):
        nb.check_mask("t", m, z, BF16)


def test_fault_g_out(fault_base):
    o, rows, st, sm, si, z, g, *_ = fault_base
    bad = g.clone()
    r, ch = [int(v) for v in (~o["keep"]).nonzero()[50]]
    bad[r, ch] = o["dz"][r, ch]
    with pytest.raises(BoundError, match=rf"row={r}, channel={ch}\)"):
        nb.check_g_out("t", bad, o["dz"], o["keep"])


def test_fault_pool():
    """A pooled element replaced by a neighbour's; an argmax code naming a tap outside the image (window (0, 0), tap 0 lies at
    row -1); a code naming a tap whose activation is far below the maximum."""
    c = nb.PoolCase(1, 9, 64, BF16)
    o = nb.pool_operands(c)
    st, sm, si, p, am, ref, E = pool_forward(c, o, nb.bn_slab_rows(81)[1])
    nb.check_pool_fwd("t", p, am, ref, E, BF16)
    bad = am.clone()
    bad[0, 0, 2, 9] = 0
    with pytest.raises(BoundError, match=r"inside the image.*image=0, row=0, col=2, channel=9\)"):
        nb.check_pool_fwd("t", p, bad, ref, E, BF16)
    bad = am.clone()
    bad[0, 3, 3, 9] = 9
    with pytest.raises(BoundError, match="inside the image"):
        nb.check_pool_fwd("t", p, bad, ref, E, BF16)
    taps = nb.pool_taps(ref, float("inf"))
    lo = taps[:, 0, 2, 2, 10].argmin()
    assert taps[lo, 0, 2, 2, 10] < ref[0].reshape(-1, 64)[:, 10].max() and am[0, 2, 2, 10] != lo
    bad = am.clone()
    bad[0, 2, 2, 10] = lo
    with pytest.raises(BoundError, match=r"argmax tap.*row=2, col=2, channel=10\)"):
        nb.check_pool_fwd("t", p, bad, ref, E, BF16)
    bad = p.clone()
    bad[0, 1, 1, 12] = p[0, 1, 2, 12] + 1.0
    with pytest.raises(BoundError, match=r"pooled.*row=1, col=1, channel=12\)"):
        nb.check_pool_fwd("t", bad, am, ref, E, BF16)


def test_fault_guard():
    arena = torch.full((600,), -123.0)
    arena[256:344] = 1.0
    check_guards(arena, 256, 344, -123.0)
    arena[344] = 0.0
    with pytest.raises(BoundError, match=r"end\+0"):
        check_guards(arena, 256, 344, -123.0)
