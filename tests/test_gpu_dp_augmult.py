"""GPU: DP-SGD with augmentation multiplicity (De et al. 2022): a RECORD is `views` consecutive
slots, its gradient the average over them, clipped once.  The norm-pass kernels per record (every family) against the
explicit per-sample slabs summed over each record in float64; the small record kernels against torch; the engine's step
against the oracle's per-sample gradients averaged per record and clipped by oracle.train_oracle.dp_clip_and_average."""
import math
import os
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu

from primia_amd import _lib  # noqa: E402
from oracle import train_oracle as O  # noqa: E402
from primia_amd import dp_micro  # noqa: E402
from primia_amd._lib import ConvDesc, PrimiaError, call, query  # noqa: E402
from primia_amd import engine as engine_module  # noqa: E402
from primia_amd.dp_clip import AdaptiveClip  # noqa: E402
from primia_amd.dp_noise import DeviceNoise  # noqa: E402
from primia_amd.dp_sampling import DeviceSampler, PoissonLoader  # noqa: E402
from primia_amd.engine import ResNet18Engine  # noqa: E402
from primia_amd.graphed_train import captures  # noqa: E402
from primia_amd.optim import EngineOptimizer  # noqa: E402
from tests import dp_clip_ref  # noqa: E402
from tests.test_gpu_dp_frozen import _flat, rel  # noqa: E402
from tests.test_gpu_dp_micro import bits, noise_of  # noqa: E402
from tests.test_gpu_dp_poisson import (CAP, HALF, N_REC, UNCLIPPED, check_lines, dp_config, ledger_lines, per_sample,  # noqa: E402
                                       run_cli, sampler_seed, weights)

BOUND = 2e-5        # per-record relative error of ||g||^2, two accumulation orders (test_dp_norm_pass_at_batch_256_...)
BF16, F32 = torch.bfloat16, torch.float32

# (N, H, C, K, R, stride, pad, views) -> the family the record norm pass must run on in bf16 (a set where either patch form
# may serve); fp32 runs on the generic kernel (14; the stem: 15)
CASES = [
    ((6, 16, 64, 64, 3, 1, 1, 2), {24}), ((6, 14, 128, 128, 3, 1, 1, 3), {24}),
    ((36, 16, 256, 256, 3, 1, 1, 4), {25}), ((33, 7, 512, 256, 3, 1, 1, 3), {25}), ((16, 12, 256, 512, 3, 1, 1, 2), {25}),
    # the Gram-matrix kernels' shapes (21 / 22 at views = 1): the patch kernel
    ((12, 7, 512, 512, 3, 1, 1, 4), {24, 25}), ((6, 7, 64, 128, 3, 1, 1, 2), {24, 25}),
    ((72, 56, 64, 128, 3, 2, 1, 4), {26}), ((36, 28, 128, 256, 3, 2, 1, 3), {26}), ((9, 14, 256, 512, 3, 2, 1, 3), {26}),
    ((300, 14, 256, 512, 1, 2, 0, 4), {26}), ((6, 28, 128, 256, 1, 2, 0, 2), {26}),
    ((4, 32, 4, 64, 7, 2, 3, 2), {15}),
]
IDS = ["-".join(map(str, c)) for c, _ in CASES]


def operands(cuda, case, dtype, identical=False):
    """(desc, x, dy) of a case with N(0, 1) operands; identical: every view of a record is the record's first."""
    N, H, C, K, R, s, p, m = case
    d = ConvDesc.make(N, H, H, C, K, R, R, s, p)
    g = torch.Generator().manual_seed(H * C + K + m)
    x = torch.randn(N, H * H, C, generator=g)
    if R == 7:
        x[..., 3] = 0       # the stem's fourth channel is padding
    dy = torch.randn(N, d.Ho * d.Wo, K, generator=g)
    if identical:
        x = x[::m].repeat_interleave(m, 0)
        dy = dy[::m].repeat_interleave(m, 0)
    return d, x.reshape(-1, C).to(dtype).to(cuda), dy.reshape(-1, K).to(dtype).to(cuda)


def record_reference(cuda, d, x, dy, m, dt):
    """||sum over the record of the explicit per-sample slabs||^2, summed and squared in float64."""
    ne = query("primia_conv_wfwd_elems", d)
    slab = torch.zeros(d.N, ne, device=cuda)
    call("primia_conv2d_wgrad_persample", d, x, dy, slab, dt)
    ref = torch.empty(d.N // m, dtype=torch.float64, device=cuda)
    for r in range(d.N // m):       # (record by record: the float64 copy of all slabs at once would be gigabytes)
        ref[r] = slab[r * m:(r + 1) * m].double().sum(0).pow(2).sum()
    return ref


def worst(got, ref):
    return ((got - ref).abs() / ref).max().item()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case,family", CASES, ids=IDS)
def test_record_sqnorm_matches_summed_slabs(cuda, dtype, case, family):
    m = case[-1]
    dt = _lib.dtype_code(dtype)
    d, x, dy = operands(cuda, case, dtype)
    kid = query("primia_conv_wgrad_record_kernel_id", d, dt, m)
    if dtype == BF16:
        assert kid in family and kid not in (21, 22, 23), (kid, family)
    else:
        assert kid == (15 if case[4] == 7 else 14), kid
    ref = record_reference(cuda, d, x, dy, m, dt)
    sq = torch.full((d.N // m,), 0.5, dtype=torch.float64, device=cuda)     # accumulates on top of what is there
    call("primia_conv2d_wgrad_record_sqnorm", d, x, dy, sq, m, dt)
    e = worst(sq - 0.5, ref)
    print(f"record norms {case} {dtype} kernel {kid}: worst relative error {e:.2e}")
    assert e < BOUND, (case, kid, e)


DECISIVE = [0, 2, 3, 5, 8, 11, 12]      # one or two cases of every family


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", [CASES[i][0] for i in DECISIVE], ids=[IDS[i] for i in DECISIVE])
def test_identical_views_give_m_squared(cuda, dtype, case):
    """All m views of a record identical: ||sum||^2 = m^2 ||g||^2.  A kernel that flushes per image gives m ||g||^2."""
    N, H, C, K, R, s, p, m = case
    dt = _lib.dtype_code(dtype)
    d, x, dy = operands(cuda, case, dtype, identical=True)
    sq = torch.zeros(N // m, dtype=torch.float64, device=cuda)
    call("primia_conv2d_wgrad_record_sqnorm", d, x, dy, sq, m, dt)
    d1 = ConvDesc.make(N // m, H, H, C, K, R, R, s, p)
    one = torch.zeros(N // m, dtype=torch.float64, device=cuda)
    first = lambda t: t.view(N // m, m, -1)[:, 0].reshape(-1, t.shape[1]).contiguous()
    call("primia_conv2d_wgrad_record_sqnorm", d1, first(x), first(dy), one, 1, dt)
    e = worst(sq, one * m * m)
    print(f"identical views {case} {dtype}: worst relative error {e:.2e}")
    assert e < BOUND, (case, e)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", [c for c, _ in CASES], ids=IDS)
def test_one_view_is_the_per_sample_entry_point(cuda, dtype, case):
    dt = _lib.dtype_code(dtype)
    d, x, dy = operands(cuda, case, dtype)
    assert query("primia_conv_wgrad_record_kernel_id", d, dt, 1) == query("primia_conv_wgrad_persample_kernel_id", d, dt)
    a = torch.zeros(d.N, dtype=torch.float64, device=cuda)
    b = torch.zeros(d.N, dtype=torch.float64, device=cuda)
    call("primia_conv2d_wgrad_record_sqnorm", d, x, dy, a, 1, dt)
    call("primia_conv2d_wgrad_persample_sqnorm", d, x, dy, b, dt)
    assert ((a - b).norm() / b.norm()).item() < 1e-6


def test_record_entry_points_refuse_ragged_records(cuda):
    d = ConvDesc.make(6, 16, 16, 64, 64, 3, 3, 1, 1)
    x = torch.zeros(6 * 256, 64, dtype=BF16, device=cuda)
    sq = torch.zeros(6, dtype=torch.float64, device=cuda)
    for views in (0, -1, 4):
        assert query("primia_conv_wgrad_record_kernel_id", d, 1, views) == -1
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_conv2d_wgrad_record_sqnorm", d, x, x, sq, views, 1)
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_stem_conv_wgrad_record_sqnorm", x, x, sq, 6, 64, 64, views, 1)


@pytest.mark.parametrize("identical", [False, True], ids=["random", "identical"])
def test_stem_halo_record_sqnorm(cuda, identical):
    """primia_stem_conv_wgrad_record_sqnorm on the padded input (one block per record) at N = 6, 64 x 64, m = 3, against
    the explicit slabs of the generic stem kernel on the unpadded input; identical views: m^2 times one view's norm."""
    N, S, m = 6, 64, 3
    g = torch.Generator().manual_seed(5)
    x4 = torch.zeros(N, S, S, 4)
    x4[..., :3] = torch.randn(N, S, S, 3, generator=g)
    dy = torch.randn(N, (S // 2) ** 2, 64, generator=g)
    if identical:
        x4, dy = x4[::m].repeat_interleave(m, 0), dy[::m].repeat_interleave(m, 0)
    xp = torch.zeros(N, S + 6, S + 8, 4)
    xp[:, 3:3 + S, 3:3 + S] = x4
    xp, x4, dy = xp.to(BF16).to(cuda), x4.to(BF16).to(cuda), dy.reshape(-1, 64).to(BF16).to(cuda)
    sq = torch.full((N // m,), 0.5, dtype=torch.float64, device=cuda)
    call("primia_stem_conv_wgrad_record_sqnorm", xp, dy, sq, N, S, S, m, 1)
    d = ConvDesc.make(N, S, S, 4, 64, 7, 7, 2, 3)
    ref = record_reference(cuda, d, x4.view(-1, 4), dy, m, 1)
    e = worst(sq - 0.5, ref)
    print(f"stem halo record norms: worst relative error {e:.2e}")
    assert e < BOUND
    if identical:
        one = torch.zeros(N, dtype=torch.float64, device=cuda)
        call("primia_stem_conv_wgrad_persample_sqnorm", xp, dy, one, N, S, S, 1)
        assert worst(sq - 0.5, one[::m] * m * m) < BOUND
    a = torch.zeros(N, dtype=torch.float64, device=cuda)
    b = torch.zeros(N, dtype=torch.float64, device=cuda)
    call("primia_stem_conv_wgrad_record_sqnorm", xp, dy, a, N, S, S, 1, 1)
    call("primia_stem_conv_wgrad_persample_sqnorm", xp, dy, b, N, S, S, 1)
    assert ((a - b).norm() / b.norm()).item() < 1e-6


# ---- the small record kernels ---------------------------------------------------------------------------------------
GUARD = 64


@pytest.mark.parametrize("m", [2, 3])
def test_record_sqnorm_small_kernels(cuda, m):
    """primia_record_sqnorm / _many against torch in float64: widths of one 16-byte chunk +- 1 and a long row, N in
    {m, 5m, 130m}; the accumulator sits between guard bands."""
    for R in (1, 5, 130):
        N = R * m
        g = torch.Generator().manual_seed(N)
        widths = [3, 4, 5, 64, 1537]
        xs = [torch.randn(N, w, generator=g).to(cuda) for w in widths]
        want = torch.zeros(R, dtype=torch.float64, device=cuda)
        whole = torch.full((GUARD + R + GUARD,), 0.25, dtype=torch.float64, device=cuda)
        for x in xs:
            want += x.double().view(R, m, -1).sum(1).pow(2).sum(1)
            call("primia_record_sqnorm", x, N, x.shape[1], m, whole[GUARD:])
        assert worst(whole[GUARD:GUARD + R] - 0.25, want) < 1e-10
        assert (whole[:GUARD] == 0.25).all() and (whole[GUARD + R:] == 0.25).all()
        ptrs = torch.tensor([x.data_ptr() for x in xs], dtype=torch.int64, device=cuda)
        wd = torch.tensor(widths, dtype=torch.int32, device=cuda)
        whole2 = torch.full((GUARD + R + GUARD,), 0.25, dtype=torch.float64, device=cuda)
        call("primia_record_sqnorm_many", ptrs, wd, len(widths), N, m, whole2[GUARD:])
        assert worst(whole2[GUARD:GUARD + R] - 0.25, want) < 1e-10
        assert (whole2[:GUARD] == 0.25).all() and (whole2[GUARD + R:] == 0.25).all()
        # one view: the per-sample kernels' quantity
        one = torch.zeros(N, dtype=torch.float64, device=cuda)
        call("primia_record_sqnorm", xs[-1], N, widths[-1], 1, one)
        assert worst(one, xs[-1].double().pow(2).sum(1)) < 1e-10
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
        call("primia_record_sqnorm", xs[0], N + 1, 3, m, whole)
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
        call("primia_record_sqnorm_many", ptrs, wd, len(widths), N, 0, whole)


@pytest.mark.parametrize("m", [2, 3])
def test_expand_clip(cuda, m):
    for R in (1, 5, 130):
        N = R * m
        clip = torch.rand(R, generator=torch.Generator().manual_seed(R)).to(cuda)
        whole = torch.full((GUARD + N + GUARD,), 7.0, device=cuda)
        call("primia_dp_expand_clip", clip, whole[GUARD:], N, m)
        assert torch.equal(whole[GUARD:GUARD + N], clip.repeat_interleave(m))
        assert (whole[:GUARD] == 7.0).all() and (whole[GUARD + N:] == 7.0).all()
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
        call("primia_dp_expand_clip", clip, whole, N + 1, m)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("m,reps,first", [(2, 5, 0), (3, 5, 4), (3, 2, 1), (2, 1, 0), (1, 5, 3)])
def test_gather_records(cuda, dtype, m, reps, first):
    """out[s * m + v] = data[((first + v) % reps) * n_rows + idx[s]], targets alike; padded (-1) and out-of-range records
    give m zero rows with target -1; rows of one chunk, three chunks and a 3 x 32 x 32 image; guard bands on both outputs."""
    per = 4 if dtype == F32 else 8
    n_rows, cap, SENT = 7, 6, -77
    for row_elems in (per, 3 * per, 3 * 32 * 32):
        g = torch.Generator().manual_seed(row_elems + m)
        data = torch.randn(reps * n_rows, row_elems, generator=g).to(dtype).to(cuda)
        targets = torch.randint(0, 3, (reps * n_rows,), generator=g).to(cuda)
        idx = torch.tensor([3, -1, 0, n_rows, 6, -1], dtype=torch.int64, device=cuda)
        out = torch.full((GUARD + cap * m * row_elems + GUARD,), 7.0, dtype=dtype, device=cuda)
        out_t = torch.full((8 + cap * m + 8,), SENT, dtype=torch.int64, device=cuda)
        call("primia_gather_records", data, row_elems, n_rows, targets, idx, first, reps, m, out[GUARD:], out_t[8:], cap,
             _lib.dtype_code(dtype))
        want = torch.zeros(cap * m, row_elems, dtype=dtype, device=cuda)
        want_t = torch.full((cap * m,), -1, dtype=torch.int64, device=cuda)
        for s, r in enumerate(idx.tolist()):
            for v in range(m):
                if 0 <= r < n_rows:
                    row = ((first + v) % reps) * n_rows + r
                    want[s * m + v] = data[row]
                    want_t[s * m + v] = targets[row]
        iv = torch.int32 if dtype == F32 else torch.int16
        assert torch.equal(out[GUARD:GUARD + cap * m * row_elems].view(iv), want.reshape(-1).view(iv))
        assert (out[:GUARD] == 7.0).all() and (out[GUARD + cap * m * row_elems:] == 7.0).all()
        assert torch.equal(out_t[8:8 + cap * m], want_t)
        assert (out_t[:8] == SENT).all() and (out_t[8 + cap * m:] == SENT).all()
    for bad in ({"views": 0}, {"reps": 0}, {"first": -1}):
        a = {"views": m, "reps": reps, "first": first, **bad}
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_gather_records", data, row_elems, n_rows, targets, idx, a["first"], a["reps"], a["views"], out[GUARD:],
                 out_t[8:], cap, _lib.dtype_code(dtype))


# ---- the engine's step --------------------------------------------------------------------------------------------------
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
M = 2
_RECORDS = {}


def record_means(per, m):
    """[{key: mean over a record's m per-sample gradients}]: what a record contributes before it is clipped."""
    return [OrderedDict((k, sum(per[r * m + v][k] for v in range(m)) / m) for k in per[0]) for r in range(len(per) // m)]


def records(norm):
    """4 records of 2 DIFFERENT views at 64 x 64 (a record's views share its target), the oracle's per-sample gradients,
    their record means and C = the median record norm — computed once per norm kind and left unchanged."""
    if norm not in _RECORDS:
        sd = weights(norm, 64, 71)
        g = torch.Generator().manual_seed(72)
        x = torch.randn(4 * M, 3, 64, 64, generator=g)
        y = torch.randint(0, 3, (4,), generator=g).repeat_interleave(M)
        means = record_means(per_sample(norm, sd, x, y), M)
        C = float(O.dp_clip_and_average(means, 1.0, 0.0)[1].median())
        _RECORDS[norm] = (sd, x, y, means, C)
    return _RECORDS[norm]


def fp32_engine(cuda, slots, norm, sd, micro=1):
    eng = ResNet18Engine(slots, 3, 3, 64, "max", dtype=F32, device=cuda, norm=norm)
    eng.load_state_dict(sd)
    eng.dp_micro_batches = micro
    return eng


@pytest.mark.parametrize("norm", ["group", "frozen"])
def test_record_step_fp32_against_the_oracle(cuda, norm):
    """fp32, 64 x 64, 4 records x 2 views: norms and clip factors per record (rtol 5e-3), every tensor rel < 5e-3 — the
    bounds of the split-step test at this size."""
    sd, x, y, means, C = records(norm)
    eng = fp32_engine(cuda, 4 * M, norm, sd)
    noise_flat, noise = noise_of(eng, 73)
    want, norms, clip = O.dp_clip_and_average(means, C, 1.3, noise)
    assert (clip < 1).any() and (clip == 1).any(), "test should exercise clipped and unclipped records"
    eng.forward(x.to(cuda))
    eng.dp_loss_backward(y.to(cuda), max_grad_norm=C, noise_multiplier=1.3, noise=noise_flat.to(cuda), views=M)
    sq, got_clip = eng.dp_stats["sq_norms"].cpu(), eng.dp_stats["clip"].cpu()
    assert sq.numel() == got_clip.numel() == 4
    assert torch.allclose(sq.sqrt(), norms, rtol=5e-3), (sq.sqrt(), norms)
    assert torch.allclose(got_clip.double(), clip, rtol=5e-3)
    for k, _ in eng.p_entries:
        assert rel(eng.gviews[k], want[k]) < 5e-3, k
    # the same through dp_params, as the training loop calls it
    eng.dp_params = {"max_grad_norm": C, "noise_multiplier": 1.3, "noise": noise_flat.to(cuda), "views": M}
    eng.forward(x.to(cuda))
    eng.loss_backward(y.to(cuda))
    for k, _ in eng.p_entries:
        assert rel(eng.gviews[k], want[k]) < 5e-3, k
    with pytest.raises(ValueError, match="records"):
        eng.dp_loss_backward(y.to(cuda), C, 1.3, noise=noise_flat.to(cuda), views=3)


@pytest.mark.parametrize("norm", ["group", "frozen"])
def test_masked_record_step_fp32(cuda, norm):
    """Capacity 4 records, 3 valid, L = 3.5, m = 2: the oracle over the valid records, divided by L; the padded record holds
    junk images."""
    sd, x, y, means, C = records(norm)
    valid, L = 3, 3.5
    eng = fp32_engine(cuda, 4 * M, norm, sd)
    noise_flat, noise = noise_of(eng, 74)
    want, norms, clip = O.dp_clip_and_average(means[:valid], C, 1.3, noise)
    assert (clip < 1).any() and (clip == 1).any()
    xm, ym = x.clone(), y.clone()
    xm[valid * M:] *= 3.0
    ym[valid * M:] = -1
    eng.forward(xm.to(cuda))
    eng.dp_loss_backward(ym.to(cuda), max_grad_norm=C, noise_multiplier=1.3, noise=noise_flat.to(cuda), expected_batch=L,
                         views=M)
    sq, got_clip = eng.dp_stats["sq_norms"].cpu(), eng.dp_stats["clip"].cpu()
    assert torch.allclose(sq[:valid].sqrt(), norms, rtol=5e-3), (sq[:valid].sqrt(), norms)
    assert torch.allclose(got_clip[:valid].double(), clip, rtol=5e-3)
    assert (sq[valid:] == 0).all() and (got_clip[valid:] == 0).all()
    for k, _ in eng.p_entries:
        assert rel(eng.gviews[k], want[k] * (valid / L)) < 5e-3, k


def test_all_padded_record_pass_adds_exact_zeros(cuda):
    """The masked record step on an engine of 4 records against the same slots plus an all-padding pass (K = 2), the padding
    pass second or first: the same bits."""
    sd, x, y, _, _ = records("group")
    L = 3.5
    ym = y.clone()
    ym[3 * M:] = -1
    pad_x = torch.randn(4 * M, 3, 64, 64, generator=torch.Generator().manual_seed(75)) * 3.0
    pad_y = torch.full((4 * M,), -1, dtype=torch.int64)

    def fresh(micro):
        eng = fp32_engine(cuda, 4 * M, "group", sd, micro)
        eng.dp_params = dict(UNCLIPPED, expected_batch=L, views=M)
        eng.dp_noise = DeviceNoise(cuda, debug_seed=7)
        return eng

    one = fresh(1)
    one.forward(x.to(cuda))
    one.loss_backward(ym.to(cuda))
    want = one.grads.clone()
    assert float(want.abs().max()) > 0
    for first_real in (True, False):
        xs = torch.cat([x, pad_x] if first_real else [pad_x, x]).to(cuda)
        ys = torch.cat([ym, pad_y] if first_real else [pad_y, ym]).to(cuda)
        eng = fresh(2)
        dp_micro.step(eng, EngineOptimizer(eng, "SGD", lr=0.0), xs, ys)
        assert torch.equal(eng.grads, want), first_real
        assert eng.dp_noise.blocks_drawn() == math.ceil(eng.P / 16)


@pytest.mark.parametrize("dtype,slack", [(F32, 1e-4), (BF16, 0.02)], ids=["f32", "bf16"])
def test_one_record_moves_the_sum_by_at_most_c(cuda, dtype, slack):
    """Sensitivity: sigma = 0, one valid record among padded ones, a C far below its norm: ||grads * L|| <= C."""
    sd, x, y, _, C = records("group")
    C, L = C / 50.0, 3.5
    eng = ResNet18Engine(4 * M, 3, 3, 64, "max", dtype=dtype, device=cuda, norm="group")
    eng.load_state_dict(sd)
    ym = torch.full_like(y, -1)
    ym[M:2 * M] = y[M:2 * M]
    eng.forward(x.to(cuda))
    eng.dp_loss_backward(ym.to(cuda), C, 0.0, noise=torch.zeros(eng.P, device=cuda), expected_batch=L, views=M)
    assert eng.dp_stats["clip"].cpu().tolist()[0] == 0.0 and 0.0 < eng.dp_stats["clip"].cpu().tolist()[1] < 1.0
    n = (eng.grads.double() * L).norm().item()
    print(f"one record, {dtype}: ||grads * L|| / C = {n / C:.6f}")
    assert 0.0 < n <= C * (1 + slack)


def test_record_step_bf16_against_the_oracles(cuda, monkeypatch):
    """bf16, 64 x 64, 8 records x 2 views: the record kernels the engine's layers take are asserted (no layer keeps its
    tiles, none runs a Gram-matrix kernel), and the clipped mean is held to the bf16-storage oracle within the band the
    storage format opens (test_dp_step_bf16_at_224_against_oracle)."""
    R_ = 8
    sd = weights("group", 64, 81)
    g = torch.Generator().manual_seed(82)
    x = torch.randn(R_ * M, 3, 64, 64, generator=g)
    y = torch.randint(0, 3, (R_,), generator=g).repeat_interleave(M)
    m16 = record_means(per_sample("group", sd, x, y, bf16_storage=True), M)
    m32 = record_means(per_sample("group", sd, x, y), M)
    C = float(O.dp_clip_and_average(m16, 1.0, 0.0)[1].median())
    want16, norms16, clip16 = O.dp_clip_and_average(m16, C, 0.0)
    want32, norms32, clip32 = O.dp_clip_and_average(m32, C, 0.0)
    assert (clip16 < 1).any() and (clip16 == 1).any()
    eng = ResNet18Engine(R_ * M, 3, 3, 64, "max", dtype=BF16, device=cuda, norm="group")
    eng.load_state_dict(sd)
    assert eng._dp_keep_buffers(), "at views = 1 this engine keeps tiles"
    kern = {c.name: query("primia_conv_wgrad_record_kernel_id", eng.convs[c.name].desc, eng.dt, M) for c in eng.spec.convs}
    assert kern["conv1"] == 15 and all(kern[f"layer1.{b}.conv{c}"] == 24 for b in (0, 1) for c in (1, 2)), kern
    for k in ("layer2.0.conv1", "layer2.0.downsample.0", "layer3.0.conv1", "layer3.0.downsample.0", "layer4.0.conv1",
              "layer4.0.downsample.0"):
        assert kern[k] == 26, (k, kern)
    assert {kern[f"layer4.{b}.conv{c}"] for b, c in ((0, 2), (1, 1), (1, 2))} == {25}, kern
    assert not set(kern.values()) & {21, 22, 23}, kern
    names = []
    real = engine_module.call
    monkeypatch.setattr(engine_module, "call", lambda name, *a, **kw: (names.append(name), real(name, *a, **kw))[1])
    eng.forward(x.to(cuda))
    eng.dp_loss_backward(y.to(cuda), C, 0.0, noise=torch.zeros(eng.P, device=cuda), views=M)
    assert not [n for n in names if "keep" in n or "clipped_sum" in n or "persample_sqnorm" in n], names
    assert names.count("primia_conv2d_wgrad_record_sqnorm") + names.count("primia_stem_conv_wgrad_record_sqnorm") == 20
    got_norms = eng.dp_stats["sq_norms"].sqrt().cpu()
    got_clip = eng.dp_stats["clip"].cpu().double()
    e16 = ((got_norms - norms16).abs() / norms16).max().item()
    o16 = ((norms16 - norms32).abs() / norms32).max().item()
    gvec = _flat(eng.gviews, eng)
    d16, oo = rel(gvec, _flat(want16, eng)), rel(_flat(want16, eng), _flat(want32, eng))
    print(f"record norms: engine vs bf16-storage oracle {e16:.3e}, oracles {o16:.3e}; clipped mean: engine vs bf16-storage "
          f"oracle {d16:.3e}, oracles {oo:.3e}")
    assert d16 < 1.25 * oo + 0.02, (d16, oo)
    bound = max(5e-3, 2 * o16)
    assert e16 < bound and torch.allclose(got_clip, clip16, rtol=bound)
    assert gvec.norm().item() <= C * 1.02


def test_a_sample_is_a_record_of_one_view(cuda, monkeypatch):
    """The engine of the test above (bf16, 64 x 64, 16 slots: it keeps tiles) without `views` and with views = 1 passed: one
    pass, the same launches — kept tiles where there are buffers, the record entry points with one view everywhere else, no
    launch that only records of several views need.  The two runs differ only in the order of the norm pass's fp64 atomics
    (test_persample_sqnorm_many: below 1e-13 on a squared norm), which reaches the gradients through one fp32 rounding of
    the clip factor: rel < 1e-6, and a factor of exactly 0 or 1 is the same in both."""
    N, L = 16, 3.5
    sd = weights("group", 64, 81)
    g = torch.Generator().manual_seed(83)
    x = torch.randn(N, 3, 64, 64, generator=g).to(cuda)
    y = torch.randint(0, 3, (N,), generator=g)
    ym = y.clone()
    ym[[2, 7, 13, 14, 15]] = -1
    y, ym = y.to(cuda), ym.to(cuda)
    eng = ResNet18Engine(N, 3, 3, 64, "max", dtype=BF16, device=cuda, norm="group")
    eng.load_state_dict(sd)
    kept = eng._dp_keep_buffers()
    assert len(kept) > 0
    zeros = torch.zeros(eng.P, device=cuda)
    eng.forward(x)
    eng.dp_loss_backward(ym, 1e9, 0.0, noise=zeros, expected_batch=L)
    C = float(eng.dp_stats["sq_norms"][ym >= 0].sqrt().median())       # half of the valid samples are clipped
    names = []
    real = engine_module.call
    monkeypatch.setattr(engine_module, "call", lambda name, *a, **kw: (names.append(name), real(name, *a, **kw))[1])

    def step(target, **kw):
        del names[:]
        eng.forward(x)
        eng.dp_loss_backward(target, C, 0.0, noise=zeros, **kw)
        return list(names), eng.grads.clone(), eng.dp_stats["clip"].clone()

    plain, g0, c0 = step(ym, expected_batch=L)
    one, g1, c1 = step(ym, expected_batch=L, views=1)
    assert plain == one
    assert c0.numel() == N and (c0[ym < 0] == 0).all() and (c0 == 1).any() and ((c0 > 0) & (c0 < 1)).any()
    assert "primia_dp_expand_clip" not in plain and "primia_scale" not in plain
    assert len([n for n in plain if "_keep" in n]) == len([n for n in plain if "clipped_sum" in n]) == len(kept)
    assert plain.count("primia_conv2d_wgrad_record_sqnorm") + plain.count("primia_stem_conv_wgrad_record_sqnorm") == \
        20 - len(kept)
    assert plain.count("primia_record_sqnorm_many") == 1 and plain.count("primia_record_sqnorm") == 1
    assert not [n for n in plain if "persample_sqnorm" in n and "_keep" not in n], plain
    e = rel(g1, g0)
    print(f"views = 1 against no views: rel = {e:.3e}")
    assert float(g0.abs().max()) > 0 and e < 1e-6
    fixed = (c0 == 0) | (c0 == 1)
    assert torch.equal(c1[fixed], c0[fixed])
    unmasked, _, _ = step(y)
    assert unmasked.count("primia_scale") == 1 and "primia_dp_expand_clip" not in unmasked


# ---- combinations ----------------------------------------------------------------------------------------------------------
def test_record_step_in_two_passes_matches_one_pass(cuda):
    """--dp_micro_batches: 4 records x 2 views as K = 2 passes on an engine of 2 records against one pass on an engine of 4;
    the logical batch is counted in records."""
    sd, x, y, means, C = records("group")
    whole = fp32_engine(cuda, 4 * M, "group", sd)
    noise_flat, noise = noise_of(whole, 76)
    dp = {"max_grad_norm": C, "noise_multiplier": 1.3, "noise": noise_flat.to(cuda), "views": M}
    whole.dp_params = dict(dp)
    whole.forward(x.to(cuda))
    whole.loss_backward(y.to(cuda))
    split = fp32_engine(cuda, 2 * M, "group", sd, micro=2)
    split.dp_params = dict(dp)
    opt = EngineOptimizer(split, "Adam", lr=0.0)
    dp_micro.step(split, opt, x.to(cuda), y.to(cuda))
    assert split.opt_steps == 1
    print(f"record step, split against whole: rel = {rel(split.grads, whole.grads):.3e}")
    assert rel(split.grads, whole.grads) < 5e-3
    want = O.dp_clip_and_average(means, C, 1.3, noise)[0]
    for k, _ in split.p_entries:
        assert rel(split.gviews[k], want[k]) < 5e-3, k


def test_adaptive_clip_counts_records(cuda):
    """--dp_clip adaptive: {below, valid} count RECORDS — 3 valid of 4 here — at the record norms."""
    sd, x, y, _, C = records("group")
    ym = y.clone()
    ym[3 * M:] = -1
    eng = fp32_engine(cuda, 4 * M, "group", sd)
    eng.dp_params = {"max_grad_norm": 1.0, "noise_multiplier": 1.3, "expected_batch": 3.5, "views": M}
    eng.dp_noise = DeviceNoise(cuda, debug_seed=9)
    eng.dp_clip = AdaptiveClip(cuda, init=C, lr=0.0, sigma_b=2.0)
    eng.forward(x.to(cuda))
    eng.loss_backward(ym.to(cuda))
    sq = eng.dp_stats["sq_norms"].cpu().numpy()
    want = dp_clip_ref.counts(sq, ym[::M].numpy(), eng.dp_clip.value())
    assert eng.dp_stats["counts"].tolist() == list(want) and want[1] == 3 and 0 < want[0] < 3, want
    assert eng.dp_clip.updates == 1


def record_loop(cuda, sd, data, targets, seed, graphed):
    """Three Poisson steps of records with 2 views from 2 stored walks, K = 2 passes each."""
    loader = PoissonLoader(data, targets, None, CAP, DeviceSampler(cuda, debug_seed=seed), repetitions=2, threshold=HALF,
                           micro_batches=2, views=M)
    eng = fp32_engine(cuda, loader.micro_size * M, "group", sd, 2)
    eng.dp_params = dict(UNCLIPPED, expected_batch=loader.expected_batch, views=M)
    eng.dp_noise = DeviceNoise(cuda, debug_seed=8)
    opt = EngineOptimizer(eng, "SGD", lr=1e-2, weight_decay=5e-4)
    arenas, grads, losses = [], [], []
    for _ in range(3):
        xb, yb = loader.draw()
        losses.append(dp_micro.step(eng, opt, xb, yb, hip_graph=graphed).clone())
        grads.append(eng._grads.clone())
        arenas.append(eng.flat.clone())
    torch.cuda.synchronize()
    return eng, loader, arenas, grads, losses


def test_graphed_record_steps_match_eager(cuda):
    seed, want_counts = sampler_seed()
    sd = weights("group", 64, 11)
    g = torch.Generator().manual_seed(21)
    data = torch.randn(2 * N_REC, 3, 64, 64, generator=g).to(cuda)
    targets = torch.randint(0, 3, (N_REC,), generator=g).repeat(2).to(cuda)
    e, le, ae, ge, lse = record_loop(cuda, sd, data, targets, seed, graphed=False)
    gr, lg, ag, gg, lsg = record_loop(cuda, sd, data, targets, seed, graphed=True)
    assert e.N == gr.N == 4 * M and le.x.shape[0] == 2 * 4 * M and le.expected_batch == 6.0
    for i in range(3):
        assert torch.equal(bits(ae[i]), bits(ag[i])), i
        assert torch.equal(bits(ge[i]), bits(gg[i])), i
        assert torch.equal(lse[i], lsg[i]) and float(lse[i]) > 0
    assert not torch.equal(ae[0], ae[1]) and not torch.equal(ae[1], ae[2])
    caps = captures(gr)
    micro = {k: v for k, v in caps.items() if "micro-batch" in k}
    assert len(caps) == len(micro) == 2 and list(micro.values()) == [1, 1], caps       # nothing is captured twice
    assert sorted(k[k.index("micro-batch") + 1] for k in micro) == ["first", "last"]
    assert all(k[k.index("micro-batch") + 2] == 1.0 / le.expected_batch and k[k.index("records of views") + 1] == M
               for k in micro)
    assert captures(e) == {}
    assert le.count.cpu().tolist() == lg.count.cpu().tolist() == [want_counts[2]] * 2
    assert le.sampler.blocks_drawn() == lg.sampler.blocks_drawn() == 3 * 2
    assert e.dp_noise.blocks_drawn() == gr.dp_noise.blocks_drawn() == 3 * math.ceil(e.P / 16)
    # the batch: record s in rows s * m + v, view v from stored walk v
    kept = want_counts[2]
    idx = lg.idx.cpu().tolist()
    for s in range(kept):
        for v in range(M):
            assert torch.equal(lg.x[s * M + v], data[v * N_REC + idx[s]]) and int(lg.y[s * M + v]) == int(targets[idx[s]])
    assert (lg.x[kept * M:] == 0).all() and (lg.y[kept * M:] == -1).all()


def test_augmenting_loader_transforms_every_kept_image_m_times(cuda):
    """The vanilla loop's loader with 3 views: every kept image goes through the transform three times in a row, each pass
    with its own draws (a stand-in transform that numbers its draws), targets repeated, the rest padded."""
    from primia_amd.dp_sampling import PoissonAugmentingLoader, from_loader

    class Tf:
        def batch(self, images, rng):
            return torch.stack([im.permute(2, 0, 1).float() / 255.0 + k for k, im in enumerate(images)])

    n, cap, m = 9, 6, 3
    g = torch.Generator().manual_seed(4)
    images = [torch.randint(0, 256, (8, 8, 1), generator=g, dtype=torch.uint8).to(cuda) for _ in range(n)]
    targets = torch.randint(0, 3, (n,), generator=g).to(cuda)
    base = type("AugmentingLoader", (), {})()
    base.images, base.targets, base.tf, base.rng = images, targets, Tf(), None
    loader = from_loader(base, 3, cap, DeviceSampler(cuda, debug_seed=6), shape=(1, 8, 8), views=m)
    assert isinstance(loader, PoissonAugmentingLoader) and len(loader) == 3
    seen = 0
    for x, y in loader:
        kept = int(loader.count[1])
        idx = loader.idx[:kept].cpu().tolist()
        assert x.shape == (cap * m, 1, 8, 8)
        for s, i in enumerate(idx):
            for v in range(m):
                assert torch.equal(x[s * m + v], images[i].permute(2, 0, 1).float() / 255.0 + (s * m + v))
                assert int(y[s * m + v]) == int(targets[i])
        assert (x[kept * m:] == 0).all() and (y[kept * m:] == -1).all()
        seen += kept
    assert seen > 0


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_cli_augmult_with_micro_batches_under_hip_graph(tmp_path):
    """Federated synthetic clients: the ledger sees q and the capacity in RECORDS, the same as the run without the flag."""
    ini = dp_config(tmp_path)
    ckpt = os.path.join(ROOT, "model_weights", "final_federated_dpaugmult.pt")
    steps = {"alice": 3, "bob": 2, "charlie": 2}
    try:
        r = run_cli(ini, "dpaugmult", ["--dp_sampling", "poisson", "--dp_augmult", "2", "--dp_micro_batches", "2",
                                       "--hip_graph"])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = ledger_lines(r.stdout, final=True)
        check_lines(got, steps)
        for name in steps:
            cap = got[name]["capacity"]
            assert "dp_augmult: {:s}: capacity {:d} records, 2 views per record, engine of {:d} slots".format(
                name, cap, -(-cap // 2) * 2) in r.stdout
        assert (r.stdout + r.stderr).count("identical views add nothing") == 1       # synthetic shards store one walk
        state = torch.load(ckpt, map_location="cpu", weights_only=False)
        assert all(bool(torch.isfinite(v).all()) for v in state["model_state_dict"].values())
        plain = run_cli(ini, "dpaugmult", ["--dp_sampling", "poisson", "--hip_graph"])
        assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
        want = ledger_lines(plain.stdout, final=True)
        for name in steps:
            assert {k: got[name][k] for k in ("q", "steps", "capacity", "sigma", "eps", "delta")} == \
                {k: want[name][k] for k in ("q", "steps", "capacity", "sigma", "eps", "delta")}
    finally:
        if os.path.exists(ckpt):
            os.remove(ckpt)
