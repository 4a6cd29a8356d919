"""GPU: DP-SGD with class weights (csrc/dp_weighted.hip, primia_amd/dp_weights.py).

The two kernels alone against tests/dp_weighted_ref.py (float64) inside guard bands; then the engine's step: unit weights
are the unweighted step bit for bit, power-of-two weights scale a sample's squared norm exactly, the clipped sum is the
weighted sum of the per-class unweighted steps, records of views obey the same scaling, the launches are the ones the
design names, a graphed step reads the weights from device memory, and train.py releases the counts once and pays once.

Tolerances.  A dlogits element is ONE rounding to float32 of a float64 value, and the device's exp may differ from numpy's
in the last float64 place: 1 ulp of float32.  The loss is a float64 sum of at most 257 terms rounded once: 4 ulp."""
import math
import os
import re
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from primia_amd import dp_accountant as A  # noqa: E402
from primia_amd import engine as engine_module  # noqa: E402
from primia_amd._lib import PrimiaError, call  # noqa: E402
from primia_amd.dp_noise import DeviceNoise  # noqa: E402
from primia_amd.dp_weights import balanced_weights, noised_counts  # noqa: E402
from primia_amd.engine import ResNet18Engine  # noqa: E402
from primia_amd.graphed_train import captures, graphed_step  # noqa: E402
from primia_amd.optim import EngineOptimizer  # noqa: E402
from tests import dp_noise_ref as R  # noqa: E402
from tests import dp_weighted_ref as W  # noqa: E402
from tests.test_gpu_dp_poisson import ROOT, UNCLIPPED, dp_config, run_cli, weights  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
GUARD = 64
SENT = 7.0


# ---- 5. the loss kernel -------------------------------------------------------------------------------------------------
def loss_case(N, C, seed, all_padded=False):
    """Logits up to |40|, weights that are no powers of two, some rows padded, one row with target = C (N > 1)."""
    rng = np.random.default_rng(seed)
    logits = rng.uniform(-40.0, 40.0, size=(N, C)).astype(np.float32)
    target = rng.integers(0, C, size=N).astype(np.int64)
    target[rng.random(N) < 0.3] = -1
    if N == 1:
        target[0] = 0
    if all_padded:
        target[:] = -1
    w = rng.uniform(0.3, 5.0, size=C).astype(np.float32)
    return logits, target, w


def run_loss_kernel(cuda, logits, target, w, scale, with_dlogits=True):
    N, C = logits.shape
    arena = torch.full((GUARD + N * C + GUARD,), SENT, dtype=F32, device=cuda)
    loss = torch.full((GUARD + 1 + GUARD,), SENT, dtype=F32, device=cuda)
    call("primia_xent_dp_weighted", torch.from_numpy(logits).to(cuda), torch.from_numpy(target).to(cuda),
         torch.from_numpy(w).to(cuda), float(scale), loss[GUARD:], arena[GUARD:] if with_dlogits else None, N, C)
    a, l = arena.cpu().numpy(), loss.cpu().numpy()
    assert (a[:GUARD] == SENT).all() and (a[GUARD + N * C:] == SENT).all(), "a word outside dlogits was written"
    assert (l[:GUARD] == SENT).all() and (l[GUARD + 1:] == SENT).all(), "a word outside the loss was written"
    return a[GUARD:GUARD + N * C].reshape(N, C), l[GUARD]


def ulps(got, want):
    """|got - float64 value| in units of the float32 spacing at that value."""
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("C", [2, 3, 16])
@pytest.mark.parametrize("N", [1, 7, 257])
def test_loss_kernel_against_float64(cuda, N, C, scale):
    logits, target, w = loss_case(N, C, 1000 * N + 10 * C)
    want_d, want_loss = W.xent_weighted(logits, target, w, scale)
    got_d, got_loss = run_loss_kernel(cuda, logits, target, w, scale)
    valid, padded = target >= 0, target < 0
    assert valid.any() and (padded.any() or N == 1)
    assert (got_d[padded] == 0).all() and not np.signbit(got_d[padded]).any()
    u = ulps(got_d[valid], want_d[valid]).max()
    lu = ulps(got_loss, want_loss)
    print(f"N = {N}, C = {C}, scale = {scale}: dlogits worst {u:.3f} ulp, loss {lu:.3f} ulp")
    assert u <= 1.0, u
    assert lu <= 4.0, (got_loss, want_loss)
    assert np.abs(got_d[valid]).max() > 0
    # loss only: the same value, dlogits untouched
    _, again = run_loss_kernel(cuda, logits, target, w, scale, with_dlogits=False)
    assert again == got_loss


@pytest.mark.parametrize("C", [2, 3, 16])
def test_loss_kernel_padding_and_poison(cuda, C):
    for N in (1, 7, 257):
        logits, target, w = loss_case(N, C, 77 * N + C, all_padded=True)
        got_d, got_loss = run_loss_kernel(cuda, logits, target, w, 0.25)
        assert (got_d == 0).all() and got_loss == 0.0
    for N in (7, 257):
        logits, target, w = loss_case(N, C, 78 * N + C)
        bad = N - 2
        target[bad] = C
        want_d, want_loss = W.xent_weighted(logits, target, w, 1.0)
        got_d, got_loss = run_loss_kernel(cuda, logits, target, w, 1.0)
        assert np.isnan(got_d[bad]).all() and np.isnan(got_loss) and np.isnan(want_loss)
        ok = (target >= 0) & (target < C)
        assert ulps(got_d[ok], want_d[ok]).max() <= 1.0 and (got_d[target < 0] == 0).all()


def test_loss_kernel_refusals(cuda):
    logits, target, w = (torch.from_numpy(a).to(cuda) for a in loss_case(7, 3, 5))
    loss, d = torch.zeros(1, device=cuda), torch.zeros(7, 3, device=cuda)
    for args in ((logits, target, None, 1.0, loss, d, 7, 3), (logits, target, w, 0.0, loss, d, 7, 3),
                 (logits, target, w, 1.0, loss, d, 0, 3), (logits, target, w, 1.0, None, d, 7, 3)):
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_xent_dp_weighted", *args)


# ---- 6. the counts kernel -----------------------------------------------------------------------------------------------
def count_targets(n, C, seed):
    """Labels over [0, C) with out-of-range ones (negative, C, far above) sprinkled in."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, C, size=n).astype(np.int64)
    odd = rng.random(n) < 0.1
    t[odd] = rng.choice(np.array([-1, -7, C, C + 1, 2 ** 40], dtype=np.int64), size=int(odd.sum()))
    return t


def counts_arena(cuda, C):
    return torch.full((8 + C + 8,), -77, dtype=torch.int64, device=cuda)


def check_counts_arena(arena, C):
    a = arena.cpu()
    assert (a[:8] == -77).all() and (a[8 + C:] == -77).all(), "a word outside counts_out was written"
    return a[8:8 + C].numpy()


@pytest.mark.parametrize("C", [3, 16])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 8193])
def test_counts_kernel(cuda, n, C):
    t = count_targets(n, C, 31 * n + C)
    td = torch.from_numpy(t).to(cuda)
    hist = W.histogram(t, C)
    assert hist.sum() <= n and (n < 255 or hist.sum() < n)
    for z in (None, torch.randn(C, generator=torch.Generator().manual_seed(n + C))):
        out = counts_arena(cuda, C)
        call("primia_dp_class_counts", td, n, C, None if z is None else z.to(cuda), 0.0, out[8:])
        assert np.array_equal(check_counts_arena(out, C), hist)            # sigma 0: the exact histogram
    z = (3.0 * torch.randn(C, generator=torch.Generator().manual_seed(7 * n + C))).to(F32)
    z[0] = -2.0                         # (on empty input class 0 goes below zero: the clamp)
    for sigma in (2.5, 20.0):
        out = counts_arena(cuda, C)
        call("primia_dp_class_counts", td, n, C, z.to(cuda), sigma, out[8:])
        got, want = check_counts_arena(out, C), W.noised_counts(t, C, z.numpy(), sigma)
        assert np.array_equal(got, want), (got, want)
        assert (got >= 0).all() and (n > 0 or got[0] == 0)
    # the stream form: z = element c of block counter + block_offset, the counter read and not moved
    for start, offset in ((5, 0), (2 ** 32 - 2, 3)):
        zc = R.reference_noise(R.KEY, R.NONCE, start + offset, 16)[:C].astype(np.float32)
        counter = torch.tensor([start], dtype=torch.int64, device=cuda)
        for sigma in (2.5, 20.0):
            a, b = counts_arena(cuda, C), counts_arena(cuda, C)
            call("primia_dp_class_counts_chacha", *R.KEY, R.NONCE, counter, offset, td, n, C, sigma, a[8:])
            call("primia_dp_class_counts", td, n, C, torch.from_numpy(zc).to(cuda), sigma, b[8:])
            assert np.array_equal(check_counts_arena(a, C), check_counts_arena(b, C))
            assert np.array_equal(check_counts_arena(a, C), W.noised_counts(t, C, zc, sigma))
        assert int(counter.item()) == start
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
        call("primia_dp_class_counts", td, n, 17, None, 1.0, counts_arena(cuda, 17)[8:])
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
        call("primia_dp_class_counts", td, n, C, None, -1.0, counts_arena(cuda, C)[8:])


def test_noised_counts_advances_the_stream_by_one_block(cuda):
    t = count_targets(300, 3, 3)
    t = t[(t >= 0) & (t < 3)]
    noise = DeviceNoise(cuda, debug_seed=11, nonce=2)
    first = noised_counts(torch.from_numpy(t).to(cuda), 3, 20.0, noise)
    second = noised_counts(torch.from_numpy(t).to(cuda), 3, 20.0, noise)
    assert noise.blocks_drawn() == 2 and first.dtype == torch.int64 and first.device.type == "cuda"
    for blk, got in enumerate((first, second)):
        z = R.reference_noise(noise.key_words, noise.nonce, blk, 16)[:3].astype(np.float32)
        assert np.array_equal(got.cpu().numpy(), W.noised_counts(t, 3, z, 20.0))
    assert not torch.equal(first, second)
    torch.manual_seed(5)
    host = noised_counts(torch.from_numpy(t).to(cuda), 3, 2.5, None)          # --dp_noise torch
    torch.manual_seed(5)
    z = torch.randn(3, dtype=F32, device=cuda).cpu().numpy()
    assert np.array_equal(host.cpu().numpy(), W.noised_counts(t, 3, z, 2.5))
    with pytest.raises(ValueError):
        noised_counts(torch.zeros(4, 3, device=cuda), 3, 1.0, None)


# ---- the engine's step ----------------------------------------------------------------------------------------------------
N, L = 6, 4.5
Y = [0, 1, 2, 1, -1, 0]             # one padded slot, every class present
POW2 = (0.5, 1.0, 4.0)
_ENGINES, _DATA = {}, {}


def data(cuda):
    if not _DATA:
        g = torch.Generator().manual_seed(91)
        _DATA["sd"] = weights("group", 64, 90)
        _DATA["x"] = torch.randn(8, 3, 64, 64, generator=g).to(cuda)
        _DATA["noise"] = None
    return _DATA


def engine(cuda, dtype, slots=N):
    key = (dtype, slots)
    if key not in _ENGINES:
        eng = ResNet18Engine(slots, 3, 3, 64, "max", dtype=dtype, device=cuda, norm="group")
        eng.load_state_dict(data(cuda)["sd"])
        _ENGINES[key] = eng
    return _ENGINES[key]


def step(cuda, dtype, y, w, C, sigma=0.0, noise=None, slots=N, views=1, expected_batch=L):
    """One masked DP step of the shared engine; (grads, sq_norms, clip) as clones."""
    eng = engine(cuda, dtype, slots)
    eng.class_weight = None if w is None else torch.tensor(w, dtype=F32, device=cuda)
    if noise is None:
        noise = torch.zeros(eng.P, device=cuda)
    eng.forward(data(cuda)["x"][:slots])
    eng.dp_loss_backward(torch.tensor(y, device=cuda), C, sigma, noise=noise, expected_batch=expected_batch, views=views)
    out = eng.grads.clone(), eng.dp_stats["sq_norms"].clone(), eng.dp_stats["clip"].clone()
    eng.class_weight = None
    return out


def median_norm(cuda, dtype, y=Y, **kw):
    sq = step(cuda, dtype, y, None, 1e9, **kw)[1]
    return float(sq[sq > 0].sqrt().median())


def bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_unit_weights_are_the_unweighted_step(cuda, dtype):
    """class_weight = ones against None: the same bits wherever the step is a function of dlogits alone.  The norm pass
    adds its tiles with fp64 atomics, so sq_norms (and through the clip factors, grads) are compared bitwise only if the
    unweighted step itself repeats bitwise; dlogits are compared bitwise always."""
    C = median_norm(cuda, dtype)
    noise = torch.randn(engine(cuda, dtype).P, generator=torch.Generator().manual_seed(92)).to(cuda)
    g0, sq0, c0 = step(cuda, dtype, Y, None, C, 1.3, noise)
    d0 = engine(cuda, dtype).dlogits.clone()
    g0b, sq0b, c0b = step(cuda, dtype, Y, None, C, 1.3, noise)
    g1, sq1, c1 = step(cuda, dtype, Y, (1.0, 1.0, 1.0), C, 1.3, noise)
    d1 = engine(cuda, dtype).dlogits.clone()
    assert torch.equal(bits(d0), bits(d1)), "the weighted kernel's rounding differs from the masked kernel's"
    assert (c0 < 1).any() and (c0 == 1).any() and float(c0[4]) == 0.0 and float(sq0[4]) == 0.0
    repeats = torch.equal(bits(sq0), bits(sq0b)) and torch.equal(bits(g0), bits(g0b))
    print(f"unit weights, {dtype}: the unweighted step repeats bitwise: {repeats}")
    if repeats:
        assert torch.equal(bits(sq0), bits(sq1)) and torch.equal(bits(c0), bits(c1)) and torch.equal(bits(g0), bits(g1))
    else:
        spread = ((sq0 - sq0b).abs() / sq0.clamp(min=1e-300)).max().item()
        assert ((sq1 - sq0).abs() / sq0.clamp(min=1e-300)).max().item() <= 4 * spread
        # ... and reaches the gradients through one fp32 rounding of a clip factor (test_a_sample_is_a_record_of_one_view)
        fixed = (c0 == 0) | (c0 == 1)
        assert torch.equal(c1[fixed], c0[fixed]) and torch.allclose(c1, c0, rtol=2.0 ** -22, atol=0)
        assert ((g1 - g0).norm() / g0.norm()).item() < 1e-6


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_weights_scale_a_samples_gradient(cuda, dtype):
    """Weights (0.5, 1, 4): powers of two scale every intermediate exactly, so sq_norms_weighted[n] = w[y_n]^2 sq_norms[n]
    — exactly if the unweighted step repeats, within 4 x its run-to-run difference otherwise.  Fails where the engine
    ignores class_weight."""
    C = median_norm(cuda, dtype)
    _, sq_a, _ = step(cuda, dtype, Y, None, C)
    _, sq_b, _ = step(cuda, dtype, Y, None, C)
    _, sq_w, clip_w = step(cuda, dtype, Y, POW2, C)
    factor = torch.tensor([POW2[t] ** 2 if t >= 0 else 0.0 for t in Y], dtype=torch.float64, device=cuda)
    want = factor * sq_a
    valid = torch.tensor([t >= 0 for t in Y], device=cuda)
    spread = ((sq_a - sq_b).abs()[valid] / sq_a[valid]).max().item()
    err = ((sq_w - want).abs()[valid] / want[valid]).max().item()
    print(f"weighted norms, {dtype}: run-to-run difference of the unweighted step {spread:.3e}, weighted against scaled {err:.3e}")
    assert float(sq_w[4]) == 0.0 and float(clip_w[4]) == 0.0
    if spread == 0.0:
        assert torch.equal(bits(sq_w), bits(want))
    else:
        assert err <= 4 * spread, (err, spread)
    assert not torch.equal(sq_w, sq_a)
    ref = torch.empty(N, dtype=F32, device=cuda)
    y = torch.tensor(Y, device=cuda)
    call("primia_dp_clip_factors_masked", sq_w, y, ref, N, float(C))
    assert torch.equal(bits(ref), bits(clip_w))
    if spread == 0.0:
        call("primia_dp_clip_factors_masked", want, y, ref, N, float(C))
        assert torch.equal(bits(ref), bits(clip_w))
    assert (clip_w < 1).any() and (clip_w == 1).any()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_the_clipped_sum_is_the_weighted_sum(cuda, dtype):
    """No clipping, no noise.  G_c = the unweighted step with every other class's slots padded (GroupNorm keeps samples
    independent).  Yardstick: sum_c G_c against the unweighted all-classes step, per parameter tensor, relative to its
    largest element; the weighted step against sum_c w_c G_c may be at most 4 x that (4 = the largest weight)."""
    eng = engine(cuda, dtype)
    G = [step(cuda, dtype, [t if t == c else -1 for t in Y], None, 1e9)[0].double() for c in range(3)]
    g_all = step(cuda, dtype, Y, None, 1e9)[0].double()
    g_w = step(cuda, dtype, Y, POW2, 1e9)[0].double()
    plain, weighted = sum(G), sum(w * g for w, g in zip(POW2, G))
    worst = (0.0, 0.0)
    off = 0
    for k, s in eng.p_entries:
        n = int(torch.Size(s).numel())
        sl = slice(off, off + n)
        off += n
        yard = ((plain[sl] - g_all[sl]).abs().max() / g_all[sl].abs().max()).item()
        err = ((g_w[sl] - weighted[sl]).abs().max() / weighted[sl].abs().max()).item()
        worst = max(worst, (err, yard))
        if yard == 0.0:
            assert err == 0.0, k
        else:
            assert err <= 4 * yard, (k, err, yard)
    assert off == eng.P and float(g_w.abs().max()) > 0
    print(f"clipped sum, {dtype}: worst tensor: weighted against sum_c w_c G_c {worst[0]:.3e}, its yardstick {worst[1]:.3e}")
    assert not torch.equal(g_w, g_all)


def test_records_of_views_obey_the_scaling(cuda):
    """8 slots as 4 records of 2 views (one record padded): 4 norms, scaled by w^2 of the record's class."""
    y = [0, 0, 2, 2, -1, -1, 1, 1]
    C = median_norm(cuda, F32, y, slots=8, views=2, expected_batch=3.5)
    kw = dict(slots=8, views=2, expected_batch=3.5)
    _, sq_a, _ = step(cuda, F32, y, None, C, **kw)
    _, sq_b, _ = step(cuda, F32, y, None, C, **kw)
    _, sq_w, clip_w = step(cuda, F32, y, POW2, C, **kw)
    assert sq_w.numel() == clip_w.numel() == 4 and float(sq_w[2]) == 0.0 and float(clip_w[2]) == 0.0
    factor = torch.tensor([POW2[0] ** 2, POW2[2] ** 2, 0.0, POW2[1] ** 2], dtype=torch.float64, device=cuda)
    want = factor * sq_a
    valid = torch.tensor([True, True, False, True], device=cuda)
    spread = ((sq_a - sq_b).abs()[valid] / sq_a[valid]).max().item()
    err = ((sq_w - want).abs()[valid] / want[valid]).max().item()
    print(f"records of views: run-to-run difference {spread:.3e}, weighted against scaled {err:.3e}")
    if spread == 0.0:
        assert torch.equal(bits(sq_w), bits(want))
    else:
        assert err <= 4 * spread


# ---- 11. launches --------------------------------------------------------------------------------------------------------
def test_launches(cuda, monkeypatch):
    names = []
    real = engine_module.call
    monkeypatch.setattr(engine_module, "call", lambda name, *a, **kw: (names.append(name), real(name, *a, **kw))[1])
    eng = engine(cuda, F32, 8)
    x = data(cuda)["x"]
    zeros = torch.zeros(eng.P, device=cuda)
    w = torch.tensor(POW2, dtype=F32, device=cuda)

    def launches(y, weight, **kw):
        eng.class_weight = weight
        eng.forward(x)
        del names[:]
        eng.dp_loss_backward(torch.tensor(y, device=cuda), 1.0, 0.0, noise=zeros, **kw)
        eng.class_weight = None
        return list(names)

    y1, y2 = [0, 1, 2, 1, -1, 0, 2, -1], [0, 0, 2, 2, -1, -1, 1, 1]
    y_full = [0, 1, 2, 1, 0, 0, 2, 1]
    for y, kw, loss_launches in ((y1, dict(expected_batch=L), ["primia_xent_hard_masked"]),
                                 (y2, dict(expected_batch=3.5, views=2), ["primia_xent_hard_masked", "primia_scale"]),
                                 (y_full, dict(), ["primia_xent_hard", "primia_scale"]),
                                 (y_full, dict(views=2), ["primia_xent_hard", "primia_scale"])):
        plain = launches(y, None, **kw)
        weighted = launches(y, w, **kw)
        assert plain[:len(loss_launches)] == loss_launches, plain[:3]     # an unweighted step's list is what it was
        assert "primia_xent_dp_weighted" not in plain
        assert weighted.count("primia_xent_dp_weighted") == 1 and weighted[0] == "primia_xent_dp_weighted"
        for gone in ("primia_xent_hard", "primia_xent_hard_masked", "primia_scale"):
            assert gone not in weighted, gone
        assert weighted[1:] == plain[len(loss_launches):]


# ---- 12. graph against eager ----------------------------------------------------------------------------------------------
def test_graphed_weighted_steps_match_eager_and_read_the_weights_from_memory(cuda):
    sd = data(cuda)["sd"]
    g = torch.Generator().manual_seed(93)
    xs = [torch.randn(N, 3, 64, 64, generator=g).to(cuda) for _ in range(2)]
    ys = [torch.tensor(Y, device=cuda), torch.tensor([2, -1, 0, 1, 1, 2], device=cuda)]
    w1, w2 = (0.7, 1.3, 2.1), (1.9, 0.6, 1.1)

    def loop(graphed):
        eng = ResNet18Engine(N, 3, 3, 64, "max", dtype=F32, device=cuda, norm="group")
        eng.load_state_dict(sd)
        eng.dp_params = dict(UNCLIPPED, expected_batch=L)
        eng.dp_noise = DeviceNoise(cuda, debug_seed=8)
        eng.class_weight = torch.tensor(w1, dtype=F32, device=cuda)
        opt = EngineOptimizer(eng, "SGD", lr=1e-2, weight_decay=5e-4)
        arenas, losses = [], []
        for i in range(5):
            if i == 3:
                eng.class_weight.copy_(torch.tensor(w2, dtype=F32, device=cuda))     # in place: the same tensor
            x, y = xs[i % 2], ys[i % 2]
            if graphed:
                losses.append(graphed_step(eng, opt, x, y).clone())
            else:
                opt.zero_grad()
                eng.forward(x)
                losses.append(eng.loss_backward(y).clone())
                opt.step()
            arenas.append(eng.flat.clone())
        torch.cuda.synchronize()
        return eng, arenas, losses

    e, ae, le = loop(False)
    gr, ag, lg = loop(True)
    for i in range(5):
        assert torch.equal(bits(ae[i]), bits(ag[i])), i
        assert torch.equal(le[i], lg[i]) and float(le[i]) > 0, i
    caps = captures(gr)
    assert list(caps.values()) == [1], caps            # the new weights did not capture again
    key = list(caps)[0]
    assert key[4] is True and "Poisson-sampled" in key and captures(e) == {}
    assert e.dp_noise.blocks_drawn() == gr.dp_noise.blocks_drawn() == 5 * math.ceil(e.P / 16)
    # the weights matter: the same loop without the overwrite ends elsewhere
    w2 = w1
    _, same, _ = loop(True)
    assert torch.equal(bits(same[2]), bits(ag[2])) and not torch.equal(same[3], ag[3])


# ---- 13. the command line -------------------------------------------------------------------------------------------------
LINE = re.compile(r"\[dp\] (\w+): \(epsilon, delta\) = \(([^,]+), ([^)]+)\) at order ([\d.]+), q = ([^,]+), "
                  r"sigma = ([^,]+), steps = (\d+), capacity = (\d+), overflow events = (\d+)(.*)$", re.M)
COUNTS = re.compile(r"^dp_weights: released class counts .*$", re.M)


def final_lines(stdout):
    out = {}
    for m in LINE.finditer(stdout):
        if m.group(10).endswith("(end of run)"):
            out[m.group(1)] = dict(eps=float(m.group(2)), q=float(m.group(5)), sigma=float(m.group(6)), steps=int(m.group(7)),
                                   tail=m.group(10))
    return out


def test_cli_weight_classes_under_dp_releases_once_and_pays_once(tmp_path):
    plain_ini = dp_config(tmp_path, epochs=10)          # two federated epochs
    text = open(plain_ini).read()
    assert "weight_classes = no" in text
    weighted_ini = tmp_path / "dpw.ini"
    weighted_ini.write_text(text.replace("weight_classes = no", "weight_classes = yes"))
    ckpt = os.path.join(ROOT, "model_weights", "final_federated_dpweighted.pt")
    kept = str(tmp_path / "first.pt")
    clients = {"alice": 6, "bob": 4, "charlie": 4}
    sigma_w = 12.0
    try:
        r = run_cli(str(weighted_ini), "dpweighted", ["--dp_sampling", "poisson", "--hip_graph", "--dp_weight_sigma", "12"])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        released = COUNTS.findall(r.stdout)
        assert len(released) == 1 and "sigma 12" in released[0], r.stdout[-2000:]
        got = final_lines(r.stdout)
        p = run_cli(plain_ini, "dpweightedplain", ["--dp_sampling", "poisson", "--hip_graph"])
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert not COUNTS.findall(p.stdout) and "release" not in p.stdout
        base = final_lines(p.stdout)
        assert sorted(got) == sorted(base) == sorted(clients)
        for name, steps in clients.items():
            a, b = got[name], base[name]
            assert a["steps"] == b["steps"] == steps and a["q"] == b["q"] and a["sigma"] == b["sigma"] == 1.3
            assert "class counts at sigma = 12.0" in a["tail"] and "release" not in b["tail"]
            seg = [(a["q"], 1.3, steps)]
            want_plain = A.epsilon(seg, 0.99e-5)[0]
            want_weighted = A.epsilon(seg, 0.99e-5, releases=[(sigma_w, 1.0)])[0]
            assert abs(b["eps"] - want_plain) <= 1e-5 * want_plain
            assert abs(a["eps"] - want_weighted) <= 1e-5 * want_weighted
            assert a["eps"] > b["eps"]
            assert abs((a["eps"] - b["eps"]) - (want_weighted - want_plain)) <= 2e-5 * want_weighted
        state = torch.load(ckpt, map_location="cpu", weights_only=False)
        assert sorted(state["dp_class_counts"]) == sorted(clients)
        for name in clients:
            entry = state["dp_class_counts"][name]
            assert entry["sigma"] == sigma_w and len(entry["counts"]) == 3 and all(c >= 0 for c in entry["counts"])
            assert state["dp_privacy"][name]["releases"] == [[sigma_w, 1.0, "class counts"]]
        total = [sum(state["dp_class_counts"][n]["counts"][c] for n in clients) for c in range(3)]
        assert str(total) in released[0]
        assert all(bool(torch.isfinite(v).all()) for v in state["model_state_dict"].values())
        shutil.copyfile(ckpt, kept)
        r2 = run_cli(str(weighted_ini), "dpweighted", ["--dp_sampling", "poisson", "--dp_weight_sigma", "12",
                                                       "--resume_checkpoint", kept])
        assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
        assert COUNTS.findall(r2.stdout) == released            # the same released values, not a second draw
        again = torch.load(ckpt, map_location="cpu", weights_only=False)
        assert again["dp_class_counts"] == state["dp_class_counts"]
        for name in clients:
            assert again["dp_privacy"][name]["releases"] == [[sigma_w, 1.0, "class counts"]]
            assert sum(t for _, _, t in again["dp_privacy"][name]["segments"]) > 0
        assert all(v["tail"].count("release of") == 1 for v in final_lines(r2.stdout).values())
    finally:
        for p_ in (ckpt, ckpt.replace("dpweighted", "dpweightedplain")):
            if os.path.exists(p_):
                os.remove(p_)
