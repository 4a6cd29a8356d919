"""GPU: DP-SGD with an adaptive clipping norm held on the device (primia_amd.dp_clip, csrc/dp_clip.hip, train.py --dp_clip
adaptive).  The kernels that READ C are bit for bit the ones that take it as a host float; the counts are exact; the update
is the float64 reference (tests/dp_clip_ref.py) to one float32 unit in the last place — one rounding of a float64 value
whose device exp may differ from NumPy's in its last double bits: 2^-23 relative; the engine's step, eager, masked, cut
into micro-batch passes and graphed, does each of these once per logical step; and the command line."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

from primia_amd import dp_micro  # noqa: E402
from primia_amd._lib import PrimiaError, call, query  # noqa: E402
from primia_amd.dp_clip import AdaptiveClip, z_delta  # noqa: E402
from primia_amd.dp_noise import DeviceNoise  # noqa: E402
from primia_amd.engine import ResNet18Engine  # noqa: E402
from primia_amd.graphed_train import captures, graphed_step  # noqa: E402
from primia_amd.optim import EngineOptimizer  # noqa: E402
from tests import dp_clip_ref as C  # noqa: E402
from tests import dp_noise_ref as R  # noqa: E402
from tests.test_gpu_dp_poisson import dp_config, run_cli, weights  # noqa: E402

KEY = R.KEY + (R.NONCE,)
ULP = C.ULP
CS = [1.0, 0.37, 1e-3, 250.0]
Z = 1.3


def bits(t):
    return t.view(torch.int32)


def f32s(cuda, *v):
    return torch.tensor(v, dtype=torch.float32, device=cuda)


# ---- 1. clip factors and counts --------------------------------------------------------------------------------------------
def norms_around(n, c, seed):
    """float64 squared norms spread over four decades around C^2, with sq == C * C exactly (counted) and the next double
    above it (not counted) among them when there is room."""
    c2 = float(np.float32(c)) ** 2
    rng = np.random.default_rng(seed)
    sq = c2 * 10.0 ** rng.uniform(-2.0, 2.0, n)
    if n >= 1:
        sq[0] = c2
    if n >= 2:
        sq[n // 2] = np.nextafter(c2, np.inf)
    if n >= 3:
        sq[n - 1] = np.nextafter(c2, 0.0)
    return sq


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1275])
def test_clip_factors_are_the_fixed_ones_and_the_counts_are_exact(cuda, n):
    for c in CS:
        sq_h = norms_around(n, c, 7 * n + 1)
        sq = torch.from_numpy(sq_h).to(cuda)
        norm = f32s(cuda, c)
        rng = np.random.default_rng(n)
        interleaved = np.where(rng.random(n) < 0.4, -1, rng.integers(0, 3, n))
        for target_h in (None, interleaved, np.full(n, -1)):
            target = None if target_h is None else torch.from_numpy(target_h.astype(np.int64)).to(cuda)
            want = torch.full((n,), -1.0, device=cuda)
            if target is None:
                call("primia_dp_clip_factors", sq, want, n, c)
            else:
                call("primia_dp_clip_factors_masked", sq, target, want, n, c)
            got = torch.full((n + 8,), -1.0, device=cuda)                   # (a guard behind the n factors)
            counts = torch.tensor([-5, -5, 77], dtype=torch.int32, device=cuda)
            call("primia_dp_clip_factors_dev", sq, target, got, n, norm, counts, 1)
            assert torch.equal(bits(got[:n]), bits(want)), (n, c)
            assert (got[n:] == -1.0).all()
            below, valid = C.counts(sq_h, target_h, c)
            assert counts.tolist() == [below, valid, 77], (n, c, counts.tolist(), below, valid)
            if target_h is not None and (target_h < 0).all():
                assert (below, valid) == (0, 0) and (got[:n] == 0).all()
            # overwrite = 0 adds to what is there
            call("primia_dp_clip_factors_dev", sq, target, got, n, norm, counts, 0)
            assert counts.tolist() == [2 * below, 2 * valid, 77]
            assert norm.item() == np.float32(c)                              # read only
        if n >= 3:      # the exact boundary: sq == C * C is at or below, the next double is not
            got = torch.empty(n, device=cuda)
            counts = torch.zeros(2, dtype=torch.int32, device=cuda)
            edge = torch.from_numpy(sq_h[[0, n // 2, n - 1]].copy()).to(cuda)
            call("primia_dp_clip_factors_dev", edge, None, got, 3, norm, counts, 1)
            assert counts.tolist() == [2, 3]


def test_clip_factor_refusals(cuda):
    sq, clip, norm = torch.ones(4, dtype=torch.float64, device=cuda), torch.ones(4, device=cuda), f32s(cuda, 1.0)
    counts = torch.zeros(2, dtype=torch.int32, device=cuda)
    for args in ((None, None, clip, 4, norm, counts), (sq, None, None, 4, norm, counts), (sq, None, clip, 4, None, counts),
                 (sq, None, clip, 4, norm, None), (sq, None, clip, 0, norm, counts), (sq, None, clip, -1, norm, counts)):
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_dp_clip_factors_dev", *args, 1)


# ---- 2. the noise kernels, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4101])
def test_noise_kernels_are_the_fixed_ones_at_the_float32_product(cuda, n):
    """sigma = float32(noise_multiplier) * float32(C) as ONE float32 product; C and the multiplier chosen so that the
    product is not representable (the float64 product of the two float32 values differs from its float32 rounding)."""
    inv_batch = 1.0 / 7.0
    ctr = torch.tensor([5], dtype=torch.int64, device=cuda)
    for c, nm in ((0.37, 1.3007), (250.0 / 3.0, z_delta(Z, 1.0))):
        c32, nm32 = np.float32(c), np.float32(nm)
        sigma = float(c32 * nm32)                                           # numpy: one float32 product
        assert float(c32) * float(nm32) != sigma, "the product should need a rounding"
        norm = f32s(cuda, c)
        g0 = torch.randn(n + 16, generator=torch.Generator(device=cuda).manual_seed(n), device=cuda)
        a0 = torch.randn(n + 16, generator=torch.Generator(device=cuda).manual_seed(n + 1), device=cuda)
        z = torch.randn(n, generator=torch.Generator(device=cuda).manual_seed(n + 2), device=cuda)
        for acc in (None, a0):
            for host_noise in (False, True):
                want, got = g0.clone(), g0.clone()
                if host_noise and acc is None:
                    call("primia_dp_add_noise", want, z, n, sigma, inv_batch)
                elif host_noise:
                    call("primia_dp_add_noise_acc", want, acc, z, n, sigma, inv_batch)
                elif acc is None:
                    call("primia_dp_noise_add", *KEY, ctr, 3, want, n, sigma, inv_batch)
                else:
                    call("primia_dp_noise_add_acc", *KEY, ctr, 3, want, acc, n, sigma, inv_batch)
                if host_noise:
                    call("primia_dp_add_noise_dev", got, acc, z, n, norm, float(nm), inv_batch)
                else:
                    call("primia_dp_noise_add_dev", *KEY, ctr, 3, got, acc, n, norm, float(nm), inv_batch)
                assert torch.equal(bits(got), bits(want)), (n, c, acc is not None, host_noise)    # and the 16 behind
                assert not torch.equal(got[:n], g0[:n]) and torch.equal(got[n:], g0[n:])
        assert torch.equal(a0, torch.randn(n + 16, generator=torch.Generator(device=cuda).manual_seed(n + 1), device=cuda))
    assert int(ctr.item()) == 5                                             # read, not advanced


def test_noise_kernel_refusals(cuda):
    g, norm = torch.zeros(32, device=cuda), f32s(cuda, 1.0)
    for args in ((None, None, 16, norm), (g[1:], None, 16, norm), (g, g[1:], 16, norm), (g, None, -1, norm),
                 (g, None, 16, None)):
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_dp_noise_add_dev", *KEY, None, 0, *args, 1.0, 1.0)
    call("primia_dp_noise_add_dev", *KEY, None, 0, None, None, 0, None, 1.0, 1.0)        # n == 0: a no-op
    for args in ((None, None, g, 16, norm), (g, None, None, 16, norm), (g, None, g, -1, norm), (g, None, g, 16, None)):
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_dp_add_noise_dev", *args, 1.0, 1.0)
    call("primia_dp_add_noise_dev", None, None, None, 0, None, 1.0, 1.0)
    assert (g == 0).all()


# ---- 3. the update ---------------------------------------------------------------------------------------------------------
GRID = [(0, 0), (0, 8), (3, 8), (4, 8), (8, 8), (1, 1), (700, 1275)]


def held(got, want):
    return abs(float(got) - want) <= ULP * abs(want)


@pytest.mark.parametrize("c0", CS)
def test_update_against_the_reference(cuda, c0):
    for below, valid in GRID:
        for z0 in (0.0, -1.7, 0.31, 5.2):
            for lo, hi in ((1e-6, 1e6), (c0 * 0.99, c0 * 1.01)):          # the second range clamps at both ends
                for eta, gamma in ((0.2, 0.5), (1.5, 0.9)):
                    inv = 1.0 / max(valid, 8)
                    norm, counts = f32s(cuda, c0), torch.tensor([below, valid], dtype=torch.int32, device=cuda)
                    out = f32s(cuda, -9.0)
                    call("primia_dp_clip_update", norm, counts, f32s(cuda, z0), 1.0, inv, eta, gamma, lo, hi, out)
                    want = C.update(c0, below, valid, z0, 1.0, inv, eta, gamma, lo, hi)
                    b = C.released(below, valid, z0, 1.0, inv)
                    got = norm.item()
                    assert held(got, want), (c0, below, valid, z0, lo, hi, got, want)
                    assert held(out.item(), b), (c0, below, valid, z0, out.item(), b)
                    assert np.float32(lo) <= np.float32(got) <= np.float32(hi)
                    assert counts.tolist() == [below, valid]                # read only
    # both ends of a narrow range are reached, and `released` may be NULL
    norm, counts = f32s(cuda, c0), torch.tensor([8, 8], dtype=torch.int32, device=cuda)
    call("primia_dp_clip_update", norm, counts, f32s(cuda, 0.0), 1.0, 0.125, 50.0, 0.5, c0 * 0.9, c0 * 1.1, None)
    assert norm.item() == np.float32(c0 * 0.9)
    counts[0] = 0
    call("primia_dp_clip_update", norm, counts, f32s(cuda, 0.0), 1.0, 0.125, 50.0, 0.5, c0 * 0.9, c0 * 1.1, None)
    call("primia_dp_clip_update", norm, counts, f32s(cuda, 0.0), 1.0, 0.125, 50.0, 0.5, c0 * 0.9, c0 * 1.1, None)
    assert norm.item() == np.float32(c0 * 1.1)


def test_update_refusals(cuda):
    from tests.test_dp_clip_host import BAD, update_args

    norm, counts, z = f32s(cuda, 1.0), torch.zeros(2, dtype=torch.int32, device=cuda), f32s(cuda, 0.0)
    for ptrs in ((None, counts, z), (norm, None, z), (norm, counts, None)):
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_dp_clip_update", *ptrs, *update_args(), None)
    for ptrs in ((None, counts), (norm, None)):
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_dp_clip_update_chacha", *KEY, None, 0, *ptrs, *update_args(), None)
    for bad in BAD:
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_dp_clip_update", norm, counts, z, *update_args(**bad), None)
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_dp_clip_update_chacha", *KEY, None, 0, norm, counts, *update_args(**bad), None)
    assert norm.item() == 1.0


def device_z0(cuda, key, block):
    """Element 0 of `block` of the noise stream under `key` (k0..k3, nonce), bit-exact: primia_dp_noise_add on 16 zeros with
    sigma = 1 and inv_batch = 1 leaves (0 + z * 1) * 1 = z.  (That this z is the definition's is test_gpu_dp_noise.py's.)"""
    g = torch.zeros(16, device=cuda)
    call("primia_dp_noise_add", *key, None, int(block), g, 16, 1.0, 1.0)
    return float(g[0].item())


@pytest.mark.parametrize("block,ctr", [(0, None), (3, 5), (2 ** 33 + 1, 7)])
def test_chacha_update_draws_element_zero_of_its_block(cuda, block, ctr):
    counter = None if ctr is None else torch.tensor([ctr], dtype=torch.int64, device=cuda)
    z0 = device_z0(cuda, KEY, block + (ctr or 0))
    assert z0 != 0.0 and abs(z0) <= R.TAIL
    for c0, (below, valid) in ((1.0, (3, 8)), (250.0, (8, 8)), (1e-3, (0, 0))):
        norm, counts, out = f32s(cuda, c0), torch.tensor([below, valid], dtype=torch.int32, device=cuda), f32s(cuda, -9.0)
        call("primia_dp_clip_update_chacha", *KEY, counter, block, norm, counts, 1.0, 0.125, 0.2, 0.5, 1e-6, 1e6, out)
        assert held(norm.item(), C.update(c0, below, valid, z0, 1.0, 0.125, 0.2, 0.5, 1e-6, 1e6))
        assert held(out.item(), C.released(below, valid, z0, 1.0, 0.125))
    if counter is not None:
        assert int(counter.item()) == ctr                                   # read, not advanced


# ---- 4. the engine -----------------------------------------------------------------------------------------------------------
SIGMA_B = 1.0
ZD = z_delta(Z, SIGMA_B)
_BATCH = {}


def batch(norm, rows=8):
    """Weights and `rows` samples at 64 x 64, made once per norm kind and left unchanged."""
    if (norm, rows) not in _BATCH:
        sd = weights(norm, 64, 51)
        g = torch.Generator().manual_seed(52)
        _BATCH[norm, rows] = (sd, torch.randn(rows, 3, 64, 64, generator=g), torch.randint(0, 3, (rows,), generator=g))
    return _BATCH[norm, rows]


def engine(cuda, norm, sd, slots=8, clip=None, seed=4, expected_batch=None):
    eng = ResNet18Engine(slots, 3, 3, 64, "max", dtype=torch.bfloat16, device=cuda, norm=norm)
    eng.load_state_dict(sd)
    eng.dp_params = {"max_grad_norm": 1.0, "noise_multiplier": Z}
    if expected_batch is not None:
        eng.dp_params["expected_batch"] = expected_batch
    eng.dp_noise = DeviceNoise(cuda, debug_seed=seed)
    if clip is not None:
        eng.dp_clip = AdaptiveClip(cuda, sigma_b=SIGMA_B, **clip)
    return eng


def stream_key(eng):
    return eng.dp_noise.key_words + (eng.dp_noise.nonce,)


@pytest.mark.parametrize("norm", ["group", "frozen"])
def test_step_with_rate_zero_is_the_fixed_step_at_z_delta(cuda, norm):
    sd, x, y = batch(norm)
    fixed = engine(cuda, norm, sd)
    fixed.dp_params["noise_multiplier"] = ZD
    fixed.forward(x.to(cuda))
    fixed.loss_backward(y.to(cuda))
    eng = engine(cuda, norm, sd, clip=dict(init=1.0, lr=0.0))
    eng.forward(x.to(cuda))
    eng.loss_backward(y.to(cuda))
    assert torch.equal(bits(eng.grads), bits(fixed.grads))
    assert torch.equal(bits(eng.dp_stats["clip"]), bits(fixed.dp_stats["clip"]))
    assert eng.dp_clip.value() == 1.0 and eng.dp_clip.updates == 1
    blocks = query("primia_dp_noise_blocks", eng.P)
    assert fixed.dp_noise.blocks_drawn() == blocks and eng.dp_noise.blocks_drawn() == blocks + 1
    sq = eng.dp_stats["sq_norms"].cpu().numpy()
    assert eng.dp_stats["counts"].tolist() == list(C.counts(sq, None, 1.0))
    assert held(eng.dp_clip.last_released(), C.released(*C.counts(sq, None, 1.0), device_z0(cuda, stream_key(eng), blocks),
                                                        SIGMA_B, 1.0 / 8))


@pytest.mark.parametrize("norm", ["group", "frozen"])
@pytest.mark.parametrize("init", [1e3, 1e-4])
def test_trajectory_follows_the_reference(cuda, norm, init):
    """Six steps from a C far above (every sample at or below it: C must fall) and far below (none: C must rise) the
    norms.  After each step C is the reference update, fed the engine's own norms, the device's z0 of block
    counter_before + blocks(P) and the C before the step, to one float32 unit; C moves in the reference's direction on
    every step.  The reference moves C whenever |b - gamma| > 0: that is asserted first, on the CPU — the test FAILS
    rather than skips should an input ever make b == gamma."""
    sd, x, y = batch(norm)
    eng = engine(cuda, norm, sd, clip=dict(init=init, quantile=0.5, lr=0.2))
    blocks = query("primia_dp_noise_blocks", eng.P)
    c = eng.dp_clip.value()
    assert c == np.float32(init)
    for step in range(6):
        before = eng.dp_noise.blocks_drawn()
        eng.forward(x.to(cuda))         # (no optimizer step: at C = 1e3 the noise alone would wreck the weights)
        eng.loss_backward(y.to(cuda))
        sq = eng.dp_stats["sq_norms"].cpu().numpy()
        below, valid = C.counts(sq, None, c)
        assert eng.dp_stats["counts"].tolist() == [below, valid] and valid == 8
        z0 = device_z0(cuda, stream_key(eng), before + blocks)
        b = C.released(below, valid, z0, SIGMA_B, 1.0 / 8)
        want = C.update(c, below, valid, z0, SIGMA_B, 1.0 / 8, 0.2, 0.5, 1e-6, 1e6)
        assert abs(b - 0.5) > 0 and want != c, "the reference itself does not move C on this input"
        got = eng.dp_clip.value()
        print(f"{norm} init {init:g} step {step}: below {below}/8, z0 {z0:+.3f}, b {b:.4f}, C {c:.6g} -> {got:.6g} "
              f"(reference {want:.6g})")
        assert held(got, want), (step, got, want)
        assert (got < c) == (want < c) and got != c
        assert held(eng.dp_clip.last_released(), b)
        assert eng.dp_noise.blocks_drawn() == before + blocks + 1
        c = got
    assert eng.dp_clip.updates == 6
    assert c < init if init > 1 else c > init


@pytest.mark.parametrize("norm", ["group", "frozen"])
def test_host_noise_has_one_more_element_for_the_count(cuda, norm):
    sd, x, y = batch(norm)
    eng = engine(cuda, norm, sd, clip=dict(init=0.5, lr=0.2))
    noise = torch.randn(eng.P + 1, generator=torch.Generator().manual_seed(9)).to(cuda)
    eng.dp_params["noise"] = noise
    eng.forward(x.to(cuda))
    eng.loss_backward(y.to(cuda))
    assert eng.dp_noise.blocks_drawn() == 0                                 # the stream is not touched
    # the same clipped sum from a fixed-C engine (an accumulating pass stops before noise and division), then the _dev
    # kernel and the update by hand
    fixed = engine(cuda, norm, sd)
    fixed.forward(x.to(cuda))
    fixed.dp_loss_backward(y.to(cuda), max_grad_norm=0.5, accumulate="first", logical_batch=8)
    want = fixed.grads.clone()
    call("primia_dp_add_noise_dev", want, None, noise, eng.P, f32s(cuda, 0.5), ZD, 1.0 / 8)
    assert torch.equal(bits(eng.grads), bits(want))
    sq = eng.dp_stats["sq_norms"].cpu().numpy()
    below, valid = C.counts(sq, None, 0.5)
    assert held(eng.dp_clip.value(), C.update(0.5, below, valid, float(noise[eng.P]), SIGMA_B, 1.0 / 8, 0.2, 0.5, 1e-6, 1e6))
    # generator=: the same step as noise= torch.randn(P + 1) from a generator in the same state
    seeded = engine(cuda, norm, sd, clip=dict(init=0.5, lr=0.2))
    seeded.dp_params["generator"] = torch.Generator(device=cuda).manual_seed(11)
    seeded.forward(x.to(cuda))
    seeded.loss_backward(y.to(cuda))
    given = engine(cuda, norm, sd, clip=dict(init=0.5, lr=0.2))
    given.dp_params["noise"] = torch.randn(eng.P + 1, dtype=torch.float32, device=cuda,
                                           generator=torch.Generator(device=cuda).manual_seed(11))
    given.forward(x.to(cuda))
    given.loss_backward(y.to(cuda))
    assert torch.equal(bits(seeded.grads), bits(given.grads)) and not torch.equal(seeded.grads, eng.grads)
    assert torch.equal(bits(seeded.dp_clip.norm), bits(given.dp_clip.norm)) and seeded.dp_clip.value() != 0.5
    assert seeded.dp_noise.blocks_drawn() == 0 and seeded.dp_clip.updates == 1
    eng.dp_params["noise"] = noise[:eng.P]
    eng.forward(x.to(cuda))
    with pytest.raises(ValueError, match="P \\+ 1"):
        eng.loss_backward(y.to(cuda))


@pytest.mark.parametrize("norm", ["group", "frozen"])
def test_padded_slots_are_not_counted(cuda, norm):
    sd, x, y = batch(norm)
    L = 6.0
    eng = engine(cuda, norm, sd, clip=dict(init=1e3, lr=0.2), expected_batch=L)
    blocks = query("primia_dp_noise_blocks", eng.P)
    ym = y.clone()
    ym[[1, 4, 7]] = -1
    eng.forward(x.to(cuda))
    eng.loss_backward(ym.to(cuda))
    sq = eng.dp_stats["sq_norms"].cpu().numpy()
    assert eng.dp_stats["counts"].tolist() == list(C.counts(sq, ym.numpy(), 1e3)) == [5, 5]
    assert (eng.dp_stats["clip"].cpu()[[1, 4, 7]] == 0).all()
    c1 = eng.dp_clip.value()
    assert held(c1, C.update(1e3, 5, 5, device_z0(cuda, stream_key(eng), blocks), SIGMA_B, 1.0 / L, 0.2, 0.5, 1e-6, 1e6))
    # an all-padding step: counts {0, 0}, C moves by the noise term alone
    eng.forward(x.to(cuda))
    eng.loss_backward(torch.full((8,), -1, dtype=torch.int64, device=cuda))
    assert eng.dp_stats["counts"].tolist() == [0, 0]
    z0 = device_z0(cuda, stream_key(eng), 2 * blocks + 1)
    want = C.update(c1, 0, 0, z0, SIGMA_B, 1.0 / L, 0.2, 0.5, 1e-6, 1e6)
    assert held(eng.dp_clip.value(), want) and want != c1 and (want < c1) == (z0 > 0)


@pytest.mark.parametrize("norm", ["group", "frozen"])
def test_micro_batches_update_once_per_logical_step(cuda, monkeypatch, norm):
    """16 rows as two passes on an engine of 8: the counts are the sum over both passes, both clip with the same C, and
    the update, the noise draw and the counter advance of blocks(P) + 1 happen once."""
    sd, x, y = batch(norm, rows=16)
    eng = engine(cuda, norm, sd, clip=dict(init=1e3, lr=0.2))
    eng.dp_micro_batches = 2
    opt = EngineOptimizer(eng, "SGD", lr=0.0)
    blocks = query("primia_dp_noise_blocks", eng.P)
    seen, launches = [], []
    inner = ResNet18Engine.dp_loss_backward

    def recording(self, *a, **kw):
        c_before = self._root.dp_clip.value()
        out = inner(self, *a, **kw)
        seen.append((c_before, self.dp_stats["sq_norms"].cpu().numpy().copy(), self.dp_stats["counts"].tolist()))
        return out

    import primia_amd.dp_clip as dc
    import primia_amd.engine as en
    real_clip_call, real_engine_call = dc.call, en.call

    def spy(real):
        def f(name, *a, **kw):
            if name in ("primia_dp_clip_update_chacha", "primia_dp_clip_update", "primia_dp_noise_add_dev", "primia_u64_add"):
                launches.append((name, a[1] if name == "primia_u64_add" else None))
            return real(name, *a, **kw)
        return f

    monkeypatch.setattr(ResNet18Engine, "dp_loss_backward", recording)
    monkeypatch.setattr(dc, "call", spy(real_clip_call))
    monkeypatch.setattr(en, "call", spy(real_engine_call))
    dp_micro.step(eng, opt, x.to(cuda), y.to(cuda))
    assert launches == [("primia_dp_noise_add_dev", None), ("primia_dp_clip_update_chacha", None),
                        ("primia_u64_add", blocks + 1)]
    assert len(seen) == 2 and seen[0][0] == seen[1][0] == 1e3               # both passes clip with the same C
    first, second = C.counts(seen[0][1], None, 1e3), C.counts(seen[1][1], None, 1e3)
    assert seen[0][2] == list(first) and seen[1][2] == [first[0] + second[0], 16]
    assert eng.dp_noise.blocks_drawn() == blocks + 1 and eng.dp_clip.updates == 1
    z0 = device_z0(cuda, stream_key(eng), blocks)
    assert held(eng.dp_clip.value(), C.update(1e3, first[0] + second[0], 16, z0, SIGMA_B, 1.0 / 16, 0.2, 0.5, 1e-6, 1e6))


def steps(cuda, norm, graphed, micro):
    sd, x, y = batch(norm, rows=16 if micro else 8)
    eng = engine(cuda, norm, sd, clip=dict(init=1.0, lr=0.5))
    eng.dp_micro_batches = 2 if micro else 1
    opt = EngineOptimizer(eng, "SGD", lr=1e-3, weight_decay=5e-4)
    xs, ys = x.to(cuda), y.to(cuda)
    out = []
    for _ in range(3):
        if micro:
            dp_micro.step(eng, opt, xs, ys, hip_graph=graphed)
        elif graphed:
            graphed_step(eng, opt, xs, ys)
        else:
            opt.zero_grad()
            eng.forward(xs)
            eng.loss_backward(ys)
            opt.step()
        out.append((eng._grads.clone(), eng.flat.clone(), eng.dp_clip.norm.clone(), eng.dp_clip.released.clone()))
    torch.cuda.synchronize()
    return eng, out


@pytest.mark.parametrize("norm", ["group", "frozen"])
@pytest.mark.parametrize("micro", [False, True])
def test_graphed_steps_match_eager_and_c_moving_captures_nothing(cuda, micro, norm):
    e, eager = steps(cuda, norm, False, micro)
    g, graphed = steps(cuda, norm, True, micro)
    for i in range(3):
        for a, b in zip(eager[i], graphed[i]):
            assert torch.equal(bits(a), bits(b)), i
    cs = [float(s[2]) for s in graphed]
    assert len({1.0, *cs}) == 4                                             # C changed on every step
    assert not torch.equal(graphed[0][1], graphed[1][1]) and not torch.equal(graphed[1][1], graphed[2][1])
    caps = captures(g)
    dp = {k: v for k, v in caps.items() if "DP with device noise" in k and "adaptive clip" in k}
    assert len(caps) == len(dp) == (2 if micro else 1) and set(dp.values()) == {1}, caps
    assert all(("frozen BatchNorm" in k) == (norm == "frozen") for k in dp)
    if micro:
        assert sorted(k[k.index("micro-batch") + 1] for k in dp) == ["first", "last"]
    assert captures(e) == {}
    blocks = query("primia_dp_noise_blocks", e.P)
    assert e.dp_noise.blocks_drawn() == g.dp_noise.blocks_drawn() == 3 * (blocks + 1)
    assert e.dp_clip.updates == g.dp_clip.updates == 3


# ---- 5. the command line ---------------------------------------------------------------------------------------------------------
def test_cli_adaptive_clip_reports_saves_and_resumes(tmp_path):
    import re

    ini = dp_config(tmp_path, epochs=1)
    ckpt = os.path.join(ROOT, "model_weights", "final_vanilla_dpclip.pt")
    kept = str(tmp_path / "first.pt")
    flags = ["--debug_dp_noise_seed", "1", "--dp_clip", "adaptive", "--dp_clip_sigma", "1.0", "--dp_clip_init", "50"]
    line = re.compile(r"dp_clip: model: C = ([^,]+), released fraction at or below C = ([^ ]+) \(target 0\.5\), (\d+) updates")
    try:
        r = run_cli(ini, "dpclip", flags, federated=False)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        m = line.search(r.stdout)
        assert m is not None, r.stdout[-2000:]
        state = torch.load(ckpt, map_location="cpu", weights_only=False)
        saved = state["dp_clip"]["model"]
        assert saved["clip_norm"] != 50.0 and 1e-6 <= saved["clip_norm"] <= 1e6 and saved["updates"] == int(m.group(3)) == 3
        assert float(m.group(1)) == float("{:.6g}".format(saved["clip_norm"]))
        assert "counts" not in saved and saved["sigma_b"] == 1.0 and saved["init"] == 50.0
        assert all(bool(torch.isfinite(v).all()) for v in state["model_state_dict"].values())
        shutil.copyfile(ckpt, kept)
        r = run_cli(ini, "dpclip", flags + ["--resume_checkpoint", kept], federated=False)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        m = re.search(r"dp_clip: model: resumed at C = ([^ ]+) after (\d+) updates", r.stdout)
        assert m is not None, r.stdout[-2000:]
        assert float(m.group(1)) == float("{:.9g}".format(saved["clip_norm"])) and int(m.group(2)) == 3
        assert torch.load(ckpt, map_location="cpu", weights_only=False)["dp_clip"]["model"]["updates"] == 6
        r = run_cli(ini, "dpclip", ["--debug_dp_noise_seed", "1"], federated=False)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "dp_clip:" not in r.stdout
        assert "dp_clip" not in torch.load(ckpt, map_location="cpu", weights_only=False)
    finally:
        if os.path.exists(ckpt):
            os.remove(ckpt)
