"""GPU: a DP-SGD step cut into micro-batch passes (train.py --dp_micro_batches, primia_amd.dp_micro) — the three kernels bit
for bit against the ones they extend, the split step against the oracle's clip-and-average at the bounds
tests/test_gpu_dp_poisson.py holds the unsplit step to at this size (fp32, 64 x 64, 8 samples: norms and clip factors rtol
5e-3, every tensor rel < 5e-3), all-padding passes exact, the Poisson loaders' K * M slots, graphed passes against eager
ones, and the command line."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

from oracle import train_oracle as O  # noqa: E402
from primia_amd import dp_micro  # noqa: E402
from primia_amd._lib import call, query  # noqa: E402
from primia_amd.dp_noise import DeviceNoise  # noqa: E402
from primia_amd.dp_sampling import DeviceSampler, PoissonLoader  # noqa: E402
from primia_amd.engine import ResNet18Engine  # noqa: E402
from primia_amd.graphed_train import captures  # noqa: E402
from primia_amd.optim import EngineOptimizer  # noqa: E402
from tests import dp_noise_ref as R  # noqa: E402
from tests.test_gpu_dp_frozen import rel  # noqa: E402
from tests.test_gpu_dp_poisson import (CAP, HALF, N_REC, UNCLIPPED, check_lines, dp_config, ledger_lines, per_sample,  # noqa: E402
                                       run_cli, sampler_seed, weights)

KEY = R.KEY + (R.NONCE,)
GUARD = 64
SIZES = [0, 1, 15, 16, 17, 4096, 4097, 65537]       # around one 16-byte chunk, one noise block, one workgroup; odd and large


def guarded(cuda, n, seed):
    """(the whole buffer, its n elements in the middle): 64 floats of guard on both sides, the middle 16-byte aligned."""
    whole = torch.randn(n + 2 * GUARD, generator=torch.Generator(device=cuda).manual_seed(seed), device=cuda)
    return whole, whole[GUARD:GUARD + n]


def bits(t):
    return t.view(torch.int32)


# ---- 1. the kernels, bit for bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_is_torchs_float32_sum(cuda, n):
    for overwrite in (1, 0):
        gw, g = guarded(cuda, n, 2 * n + 1)
        aw, acc = guarded(cuda, n, 2 * n + 2)
        g0, a0 = gw.clone(), aw.clone()
        call("primia_dp_accumulate", acc, g, n, overwrite)
        want = a0.clone()
        want[GUARD:GUARD + n] = g0[GUARD:GUARD + n] if overwrite else a0[GUARD:GUARD + n] + g0[GUARD:GUARD + n]
        assert torch.equal(bits(aw), bits(want)), (n, overwrite)        # the sum AND the guards
        assert torch.equal(bits(gw), bits(g0))                          # g is read only


@pytest.mark.parametrize("n", SIZES)
def test_finish_kernels_are_the_plain_ones_on_the_sum(cuda, n):
    """primia_dp_noise_add_acc(g, acc) = primia_dp_noise_add(acc + g) and primia_dp_add_noise_acc(g, acc, z) =
    primia_dp_add_noise(acc + g, z): the same expression from the same compiler, so no tolerance.  Same key, nonce, a
    device counter preset to 5 and block offset 3."""
    sigma, inv_batch = 1.3, 1.0 / 7.0
    ctr = torch.tensor([5], dtype=torch.int64, device=cuda)
    for host_noise in (False, True):
        gw, g = guarded(cuda, n, 3 * n + 1)
        aw, acc = guarded(cuda, n, 3 * n + 2)
        g0, a0 = gw.clone(), aw.clone()
        z = torch.randn(max(n, 1), generator=torch.Generator(device=cuda).manual_seed(n + 9), device=cuda)
        ww, want = guarded(cuda, n, 3 * n + 1)                          # the same g again
        want.copy_(a0[GUARD:GUARD + n] + g0[GUARD:GUARD + n])           # torch's float32 sum
        if host_noise:
            call("primia_dp_add_noise", want, z, n, sigma, inv_batch)
            call("primia_dp_add_noise_acc", g, acc, z, n, sigma, inv_batch)
        else:
            call("primia_dp_noise_add", *KEY, ctr, 3, want, n, sigma, inv_batch)
            call("primia_dp_noise_add_acc", *KEY, ctr, 3, g, acc, n, sigma, inv_batch)
        assert torch.equal(bits(gw), bits(ww)), (n, host_noise)         # the result AND the guards
        assert torch.equal(bits(aw), bits(a0))                          # acc is unchanged
        if n:
            assert not torch.equal(g, g0[GUARD:GUARD + n])
    assert int(ctr.item()) == 5                                         # read, not advanced


# ---- 2. split against whole, shuffled batches ---------------------------------------------------------------------------
_CASES = {}


def case(norm):
    """8 samples, their oracle per-sample gradients, C = the median oracle norm, explicit noise — computed once per norm."""
    if norm not in _CASES:
        sd = weights(norm, 64, 31)
        g = torch.Generator().manual_seed(32)
        x = torch.randn(8, 3, 64, 64, generator=g)
        y = torch.randint(0, 3, (8,), generator=g)
        per = per_sample(norm, sd, x, y)
        C = float(O.dp_clip_and_average(per, 1.0, 0.0)[1].median())
        _CASES[norm] = (sd, x, y, per, C)
    return _CASES[norm]


def noise_of(eng, seed):
    flat = torch.randn(eng.P, generator=torch.Generator().manual_seed(seed))
    per_key, off = {}, 0
    for k, s in eng.p_entries:
        n = int(torch.Size(s).numel())
        per_key[k] = flat[off:off + n].view(s)
        off += n
    return flat, per_key


def engine(cuda, slots, norm, sd, micro=1):
    eng = ResNet18Engine(slots, 3, 3, 64, "max", dtype=torch.float32, device=cuda, norm=norm)
    eng.load_state_dict(sd)
    eng.dp_micro_batches = micro
    return eng


@pytest.mark.parametrize("norm", ["group", "frozen"])
def test_split_step_against_the_whole_one_and_the_oracle(cuda, norm, monkeypatch):
    sd, x, y, per, C = case(norm)
    whole = engine(cuda, 8, norm, sd)
    noise_flat, noise = noise_of(whole, 33)
    stats = []
    inner = ResNet18Engine.dp_loss_backward

    def recording(self, *a, **kw):      # dp_stats stays per pass: keep every pass's
        out = inner(self, *a, **kw)
        stats.append((self.dp_stats["sq_norms"].cpu().clone(), self.dp_stats["clip"].cpu().clone()))
        return out

    monkeypatch.setattr(ResNet18Engine, "dp_loss_backward", recording)

    def held_to_the_oracle(eng, count):
        want, norms, clip = O.dp_clip_and_average(per[:count], C, 1.3, noise)
        assert (clip < 1).any() and (clip == 1).any(), "test should exercise clipped and unclipped samples"
        sq = torch.cat([s for s, _ in stats])
        got_clip = torch.cat([c for _, c in stats])
        assert sq.numel() == count
        assert torch.allclose(sq.sqrt(), norms, rtol=5e-3), (sq.sqrt(), norms)
        assert torch.allclose(got_clip.double(), clip, rtol=5e-3)
        for k, _ in eng.p_entries:
            assert rel(eng.gviews[k], want[k]) < 5e-3, (count, k)

    dp = {"max_grad_norm": C, "noise_multiplier": 1.3, "noise": noise_flat.to(cuda)}
    # the whole batch on an engine of 8, one ordinary step
    whole.dp_params = dict(dp)
    whole.forward(x.to(cuda))
    whole.loss_backward(y.to(cuda))
    held_to_the_oracle(whole, 8)
    g_whole = whole.grads.clone()
    # 8 = 4 + 4 and 7 = 4 + 3 (a sibling; divided by 7) on an engine of 4.  Adam at lr 0: the step count moves, no weight does
    split = engine(cuda, 4, norm, sd, micro=2)
    split.dp_params = dict(dp)
    opt = EngineOptimizer(split, "Adam", lr=0.0)
    for count in (8, 7):
        del stats[:]
        before = split.opt_steps
        loss = dp_micro.step(split, opt, x[:count].to(cuda), y[:count].to(cuda))
        assert split.opt_steps == before + 1
        assert not hasattr(split, "dp_phase") and not hasattr(split, "dp_logical_batch")
        assert len(stats) == 2 and math.isfinite(float(loss))
        held_to_the_oracle(split, count)
        if count == 8:
            print(f"{norm}: split against whole, rel = {rel(split.grads, g_whole):.3e}")
            assert rel(split.grads, g_whole) < 5e-3
    # sigma 0 through the device stream: a clipped sum of 8 over 8 has norm <= C; ONE draw of ceil(P / 16) blocks per step
    split.dp_params = {"max_grad_norm": C, "noise_multiplier": 0.0}
    split.dp_noise = DeviceNoise(cuda, debug_seed=5)
    before = split.opt_steps
    dp_micro.step(split, opt, x.to(cuda), y.to(cuda))
    assert split.grads.double().norm().item() <= C * (1 + 1e-4)
    assert split.grads.double().norm().item() > 0
    assert split.opt_steps == before + 1
    assert split.dp_noise.blocks_drawn() == math.ceil(split.P / 16) == query("primia_dp_noise_blocks", split.P)


# ---- 3. padding passes are exact ---------------------------------------------------------------------------------------------
def test_all_padding_passes_add_exact_zeros(cuda):
    """Capacity 4 with 3 valid samples, every clip factor 1: the masked step on an engine of 4 against the same 4 slots
    plus an all-padding pass (K = 2), the padding pass second or first, zero or junk images in the padded slots."""
    L, size = 3.0, 64
    sd = weights("group", size, 41)
    g = torch.Generator().manual_seed(42)
    x4 = torch.zeros(4, 3, size, size)
    x4[:3] = torch.randn(3, 3, size, size, generator=g)
    y4 = torch.tensor([0, 2, 1, -1])
    junk = torch.randn(8, 3, size, size, generator=g) * 3.0
    pad_x, pad_y = torch.zeros(4, 3, size, size), torch.full((4,), -1, dtype=torch.int64)

    def fresh(micro):
        eng = engine(cuda, 4, "group", sd, micro)
        eng.dp_params = dict(UNCLIPPED, expected_batch=L)
        eng.dp_noise = DeviceNoise(cuda, debug_seed=7)
        return eng

    one = fresh(1)
    one.forward(x4.to(cuda))
    want_loss = float(one.loss_backward(y4.to(cuda)))
    want = one.grads.clone()
    assert float(want.abs().max()) > 0 and want_loss > 0
    for first_real in (True, False):
        for with_junk in (False, True):
            real_x, px = x4.clone(), pad_x.clone()
            if with_junk:
                real_x[3], px = junk[0], junk[4:8].clone()
            xs = torch.cat([real_x, px] if first_real else [px, real_x]).to(cuda)
            ys = torch.cat([y4, pad_y] if first_real else [pad_y, y4]).to(cuda)
            eng = fresh(2)
            opt = EngineOptimizer(eng, "SGD", lr=0.0)
            loss = float(dp_micro.step(eng, opt, xs, ys))
            assert torch.equal(eng.grads, want), (first_real, with_junk)    # as floats: -0.0 == +0.0
            assert abs(loss - want_loss) <= 1e-6 * want_loss
            assert eng.dp_noise.blocks_drawn() == one.dp_noise.blocks_drawn() == math.ceil(eng.P / 16)


# ---- 4. the Poisson loader ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,M", [(2, 4), (3, 3)])
def test_poisson_loader_pads_to_k_times_m_slots(cuda, K, M):
    seed, want_counts = sampler_seed()
    g = torch.Generator().manual_seed(21)
    data = torch.randn(N_REC, 3, 8, 8, generator=g).to(cuda)
    targets = torch.randint(0, 3, (N_REC,), generator=g).to(cuda)
    plain = PoissonLoader(data, targets, None, CAP, DeviceSampler(cuda, debug_seed=seed), threshold=HALF)
    micro = PoissonLoader(data, targets, None, CAP, DeviceSampler(cuda, debug_seed=seed), threshold=HALF, micro_batches=K)
    assert (micro.micro_size, micro.slots, micro.capacity) == (M, K * M, CAP)
    assert (micro.q, micro.threshold, micro.expected_batch, len(micro)) == (plain.q, plain.threshold, plain.expected_batch,
                                                                          len(plain))
    for step in range(3):
        plain.draw()
        x, y = micro.draw()
        assert x.shape[0] == y.shape[0] == K * M
        assert torch.equal(micro.idx, plain.idx) and torch.equal(micro.count, plain.count)
        assert micro.count.cpu().tolist() == [want_counts[step]] * 2
        kept = want_counts[step]
        idx = micro.idx.cpu().tolist()
        assert idx[:kept] == sorted(idx[:kept]) and idx[kept:] == [-1] * (CAP - kept)
        assert torch.equal(x[:kept], data[idx[:kept]]) and torch.equal(y[:kept], targets[idx[:kept]])
        assert (x[kept:] == 0).all() and (y[kept:] == -1).all()             # up to K * M
        assert torch.equal(x[:CAP], plain.x) and torch.equal(y[:CAP], plain.y)
    assert micro.draws == plain.draws == 3
    assert micro.sampler.blocks_drawn() == plain.sampler.blocks_drawn() == 3 * 2
    assert micro.sampler.overflow_events() == plain.sampler.overflow_events() == 0


# ---- 5. graphed equals eager ---------------------------------------------------------------------------------------------------
def micro_steps(cuda, sd, data, targets, seed, graphed, K=2):
    loader = PoissonLoader(data, targets, None, CAP, DeviceSampler(cuda, debug_seed=seed), threshold=HALF, micro_batches=K)
    eng = engine(cuda, loader.micro_size, "group", sd, K)
    eng.dp_params = dict(UNCLIPPED, expected_batch=loader.expected_batch)
    eng.dp_noise = DeviceNoise(cuda, debug_seed=8)
    opt = EngineOptimizer(eng, "SGD", lr=1e-2, weight_decay=5e-4)
    arenas, grads, losses = [], [], []
    for _ in range(3):
        x, y = loader.draw()
        if K == 1:
            opt.zero_grad()
            eng.forward(x)
            losses.append(eng.loss_backward(y).clone())
            grads.append(eng.grads.clone())
            opt.step()
        else:
            losses.append(dp_micro.step(eng, opt, x, y, hip_graph=graphed).clone())
            grads.append(eng._grads.clone())
        arenas.append(eng.flat.clone())
    torch.cuda.synchronize()
    return eng, loader, arenas, grads, losses


def test_graphed_micro_batch_steps_match_eager(cuda):
    seed, _ = sampler_seed()
    sd = weights("group", 64, 11)
    g = torch.Generator().manual_seed(21)
    data = torch.randn(N_REC, 3, 64, 64, generator=g).to(cuda)
    targets = torch.randint(0, 3, (N_REC,), generator=g).to(cuda)
    e, le, ae, ge, lse = micro_steps(cuda, sd, data, targets, seed, graphed=False)
    gr, lg, ag, gg, lsg = micro_steps(cuda, sd, data, targets, seed, graphed=True)
    assert e.N == gr.N == 4
    for i in range(3):
        assert torch.equal(bits(ae[i]), bits(ag[i])), i
        assert torch.equal(bits(ge[i]), bits(gg[i])), i
        assert torch.equal(lse[i], lsg[i]) and float(lse[i]) > 0
    assert not torch.equal(ae[0], ae[1]) and not torch.equal(ae[1], ae[2])
    caps = captures(gr)
    micro = {k: v for k, v in caps.items() if "micro-batch" in k}
    assert len(caps) == len(micro) == 2 and list(micro.values()) == [1, 1], caps
    assert sorted(k[k.index("micro-batch") + 1] for k in micro) == ["first", "last"]
    assert all(k[k.index("micro-batch") + 2] == 1.0 / le.expected_batch and "Poisson-sampled" in k for k in micro)
    assert captures(e) == {}
    assert le.sampler.blocks_drawn() == lg.sampler.blocks_drawn() == 3 * 2
    assert e.dp_noise.blocks_drawn() == gr.dp_noise.blocks_drawn() == 3 * math.ceil(e.P / 16)
    assert le.draws == lg.draws == 3
    # the first step's records on an engine of 8 in one pass: only the order of the float32 sum differs
    w, lw, aw, gw, lsw = micro_steps(cuda, sd, data, targets, seed, graphed=False, K=1)
    assert w.N == 8
    print(f"first step, split against whole: gradient rel = {rel(ge[0], gw[0]):.3e}, weights rel = {rel(ae[0], aw[0]):.3e}")
    assert rel(ge[0], gw[0]) < 5e-3 and rel(ae[0], aw[0]) < 5e-3
    assert abs(float(lse[0]) - float(lsw[0])) <= 1e-5 * float(lsw[0])


# ---- 6. the command line -------------------------------------------------------------------------------------------------------
def test_cli_poisson_micro_batches_under_hip_graph(tmp_path):
    """The ledger does not know about K: the same q, steps and capacity as the run without the flag."""
    ini = dp_config(tmp_path)
    ckpt = os.path.join(ROOT, "model_weights", "final_federated_dpmicro.pt")
    steps = {"alice": 3, "bob": 2, "charlie": 2}
    try:
        r = run_cli(ini, "dpmicro", ["--dp_sampling", "poisson", "--dp_micro_batches", "2", "--hip_graph"])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "K = 2 passes" in r.stdout
        got = ledger_lines(r.stdout, final=True)
        check_lines(got, steps)
        check_lines(ledger_lines(r.stdout, final=False), steps)
        state = torch.load(ckpt, map_location="cpu", weights_only=False)
        assert sorted(state["dp_privacy"]) == ["alice", "bob", "charlie"]
        assert all(bool(torch.isfinite(v).all()) for v in state["model_state_dict"].values())
        plain = run_cli(ini, "dpmicro", ["--dp_sampling", "poisson", "--hip_graph"])
        assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
        want = ledger_lines(plain.stdout, final=True)
        for name in steps:
            assert {k: got[name][k] for k in ("q", "steps", "capacity", "sigma", "eps", "delta")} == \
                {k: want[name][k] for k in ("q", "steps", "capacity", "sigma", "eps", "delta")}
    finally:
        if os.path.exists(ckpt):
            os.remove(ckpt)


def test_cli_shuffle_micro_batches(tmp_path):
    ini = dp_config(tmp_path)
    ckpt = os.path.join(ROOT, "model_weights", "final_federated_dpmicroshuffle.pt")
    try:
        r = run_cli(ini, "dpmicroshuffle", ["--dp_micro_batches", "2"])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "K = 2 passes on an engine of M = 4 slots" in r.stdout
        state = torch.load(ckpt, map_location="cpu", weights_only=False)
        assert all(bool(torch.isfinite(v).all()) for v in state["model_state_dict"].values())
        r = run_cli(ini, "dpmicroshuffle", ["--dp_micro_batches", "3"])
        assert r.returncode != 0 and "3 does not divide batch_size 8" in r.stderr
    finally:
        if os.path.exists(ckpt):
            os.remove(ckpt)
