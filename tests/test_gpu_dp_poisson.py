"""GPU: DP-SGD on Poisson-sampled, padded batches — ResNet18Engine.dp_loss_backward(expected_batch=L) against the oracle's
per-sample gradients, PoissonLoader + graphed_step against the same steps run eagerly, and train.py --dp_sampling poisson.

The oracle side: O.dp_clip_and_average on the VALID samples averages over their number v; the engine divides by the
expected batch L, so the oracle's result is rescaled by v / L.  Tolerances are those tests/test_gpu_dp_frozen.py holds
the unpadded step to at the same sizes (norms rtol 5e-3, every tensor rel < 5e-3; bf16: the oracle-distance rule)."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

from oracle import train_oracle as O  # noqa: E402
from primia_amd import dp_accountant as A  # noqa: E402
from primia_amd import resnet_spec as rs  # noqa: E402
from primia_amd.dp_noise import DeviceNoise  # noqa: E402
from primia_amd.dp_sampling import DeviceSampler, PoissonAugmentingLoader, PoissonLoader, from_loader  # noqa: E402
from primia_amd.engine import ResNet18Engine  # noqa: E402
from primia_amd.graphed_train import captures, graphed_step  # noqa: E402
from primia_amd.optim import EngineOptimizer  # noqa: E402
from tests import dp_noise_ref as R  # noqa: E402
from tests.cpu_standins import chacha20_words  # noqa: E402
from tests.test_gpu_dp_frozen import _flat, eval_per_sample_gradients, frozen_state_dict, rel  # noqa: E402
from tests.test_gpu_dp_noise import Z_TOL, recovered_z  # noqa: E402

# every clip factor is exactly 1.0 (no per-sample norm comes near 1e9), so the order-dependent fp64 sums of the norm pass
# cannot reach the gradient, and sigma = noise_multiplier * max_grad_norm is still 1.3 (tests/test_gpu_dp_noise.py)
UNCLIPPED = {"max_grad_norm": 1e9, "noise_multiplier": 1.3e-9}


def weights(norm, size, seed):
    if norm == "frozen":
        return frozen_state_dict(size, "max", seed)
    torch.manual_seed(seed)
    return rs.init_state_dict(rs.resnet18_spec(3, 3, size, "max"), "group")


def per_sample(norm, sd, x, y, bf16_storage=False):
    if norm == "frozen":
        return eval_per_sample_gradients(sd, x, y, "max", bf16_storage=bf16_storage)
    return O.per_sample_gradients({k: v.clone() for k, v in sd.items()}, x, y, "max", bf16_storage=bf16_storage)


@pytest.mark.parametrize("norm", ["group", "frozen"])
def test_masked_dp_step_fp32(cuda, norm):
    """fp32, 64 x 64, capacity 8 with 5 valid samples, L = 6."""
    cap, valid, size, L = 8, 5, 64, 6.0
    sd = weights(norm, size, 9)
    eng = ResNet18Engine(cap, 3, 3, size, "max", dtype=torch.float32, device=cuda, norm=norm)
    eng.load_state_dict(sd)
    g = torch.Generator().manual_seed(10)
    xv = torch.randn(valid, 3, size, size, generator=g)
    yv = torch.randint(0, 3, (valid,), generator=g)
    junk = torch.randn(cap - valid, 3, size, size, generator=g) * 3.0
    noise_flat = torch.randn(eng.P, generator=g)
    noise, off = {}, 0
    for k, s in eng.p_entries:
        n = int(torch.Size(s).numel())
        noise[k] = noise_flat[off:off + n].view(s)
        off += n
    x = torch.zeros(cap, 3, size, size)
    x[:valid] = xv
    y = torch.full((cap,), -1, dtype=torch.int64)
    y[:valid] = yv
    xj = x.clone()
    xj[valid:] = junk
    # 1. against the oracle's per-sample gradients, C = the median of their norms
    per = per_sample(norm, sd, xv, yv)
    _, norms1, _ = O.dp_clip_and_average(per, 1.0, 0.0)
    C = float(norms1.median())
    want, norms, clip = O.dp_clip_and_average(per, C, 1.3, noise)
    assert (clip < 1).any() and (clip == 1).any(), "test should exercise clipped and unclipped samples"
    logits = eng.forward(x.to(cuda)).clone()
    loss = eng.dp_loss_backward(y.to(cuda), max_grad_norm=C, noise_multiplier=1.3, noise=noise_flat.to(cuda),
                                expected_batch=L)
    sq, got_clip = eng.dp_stats["sq_norms"].cpu(), eng.dp_stats["clip"].cpu()
    assert torch.allclose(sq[:valid].sqrt(), norms, rtol=5e-3), (sq[:valid].sqrt(), norms)
    assert torch.allclose(got_clip[:valid].double(), clip, rtol=5e-3)
    assert (sq[valid:] == 0).all() and (got_clip[valid:] == 0).all()
    for k, _ in eng.p_entries:
        assert rel(eng.gviews[k], want[k] * (valid / L)) < 5e-3, k
    want_loss = float(F.cross_entropy(logits[:valid].double().cpu(), yv))
    assert abs(float(loss) - want_loss) <= 1e-6 * want_loss
    # without noise: the clipped sum over L has norm <= C * valid / L
    eng.forward(x.to(cuda))
    eng.dp_loss_backward(y.to(cuda), C, 0.0, noise=torch.zeros(eng.P, device=cuda), expected_batch=L)
    assert eng.grads.double().norm().item() <= C * valid / L * (1 + 1e-4)
    # 2. what the padded slots hold does not reach the gradient: zeros or finite junk, bit for bit
    zeros = torch.zeros(eng.P, device=cuda)
    eng.forward(x.to(cuda))
    eng.dp_loss_backward(y.to(cuda), **UNCLIPPED, noise=zeros, expected_batch=L)
    a, clip_a = eng.grads.clone(), eng.dp_stats["clip"].clone()
    eng.forward(xj.to(cuda))
    eng.dp_loss_backward(y.to(cuda), **UNCLIPPED, noise=zeros, expected_batch=L)
    assert clip_a.cpu().tolist() == [1.0] * valid + [0.0] * (cap - valid)
    assert torch.equal(eng.grads.view(torch.int32), a.view(torch.int32))
    assert (eng.dp_stats["sq_norms"][valid:] == 0).all()
    assert float(a.abs().max()) > 0
    # 3. an all-padding batch is legal: loss 0 and the step is the noise term alone, sigma z / L — z against the float64
    #    definition within test_gpu_dp_noise's bound: out = (0 + sigma z) * (1 / L) in float32 is the product's and the
    #    scaling's rounding plus the rounding of 1 / L itself, the three units recovered_z allows
    stream = DeviceNoise(cuda, debug_seed=5, nonce=2)
    eng.dp_noise = stream
    none = torch.full((cap,), -1, dtype=torch.int64, device=cuda)
    eng.forward(xj.to(cuda))
    loss = eng.dp_loss_backward(none, **UNCLIPPED, expected_batch=L)
    assert float(loss) == 0.0
    assert (eng.dp_stats["sq_norms"] == 0).all() and (eng.dp_stats["clip"] == 0).all()
    sigma = np.float32(UNCLIPPED["max_grad_norm"] * UNCLIPPED["noise_multiplier"])
    z, rounding = recovered_z(eng.grads, torch.zeros(eng.P), sigma, 1.0 / L)
    err = np.abs(z - R.reference_noise(stream.key_words, stream.nonce, 0, eng.P))
    print(f"all-padding step: max |z - reference| = {err.max():.3e} (allowance {Z_TOL + rounding.max():.3e})")
    assert (err <= Z_TOL + rounding).all()
    assert stream.blocks_drawn() == math.ceil(eng.P / 16)


def test_masked_dp_step_bf16_against_oracles(cuda):
    """bf16, frozen statistics, capacity 16 at 32 x 32 with 11 valid samples, L = 12: the rule of
    test_frozen_dp_step_bf16_against_oracles — norms and clip factors within max(5e-3, twice the two oracles' own
    distance), the gradient within 1.25 x the oracles' distance + 0.02."""
    cap, valid, size, L = 16, 11, 32, 12.0
    sd = frozen_state_dict(size, "max", 61)
    eng = ResNet18Engine(cap, 3, 3, size, "max", dtype=torch.bfloat16, device=cuda, norm="frozen")
    eng.load_state_dict(sd)
    g = torch.Generator().manual_seed(62)
    xv = torch.randn(valid, 3, size, size, generator=g)
    yv = torch.randint(0, 3, (valid,), generator=g)
    x = torch.zeros(cap, 3, size, size)
    x[:valid] = xv
    y = torch.full((cap,), -1, dtype=torch.int64)
    y[:valid] = yv
    per16 = eval_per_sample_gradients(sd, xv, yv, "max", bf16_storage=True)
    per32 = eval_per_sample_gradients(sd, xv, yv, "max")
    _, n16, _ = O.dp_clip_and_average(per16, 1.0, 0.0)
    C = float(n16.median())
    want16, norms16, clip16 = O.dp_clip_and_average(per16, C, 0.0)
    want32, norms32, clip32 = O.dp_clip_and_average(per32, C, 0.0)
    assert (clip16 < 1).any() and (clip16 == 1).any()
    eng.forward(x.to(cuda))
    eng.dp_loss_backward(y.to(cuda), C, 0.0, noise=torch.zeros(eng.P, device=cuda), expected_batch=L)
    sq, clip = eng.dp_stats["sq_norms"].cpu(), eng.dp_stats["clip"].cpu().double()
    got_norms = sq[:valid].sqrt()
    gvec = _flat(eng.gviews, eng)
    e16 = ((got_norms - norms16).abs() / norms16).max().item()
    e32 = ((got_norms - norms32).abs() / norms32).max().item()
    o16 = ((norms16 - norms32).abs() / norms32).max().item()
    d16 = rel(gvec, _flat(want16, eng) * (valid / L))
    oo = rel(_flat(want16, eng), _flat(want32, eng))
    print(f"norms: engine vs fp32 oracle {e32:.3e}, vs bf16-storage oracle {e16:.3e}, oracles {o16:.3e}; gradient: engine "
          f"vs bf16-storage oracle {d16:.3e}, oracles {oo:.3e}")
    bound = max(5e-3, 2 * o16)
    assert e16 < bound and e32 < bound
    assert torch.allclose(clip[:valid], clip16, rtol=bound) and torch.allclose(clip[:valid], clip32, rtol=bound)
    assert d16 < 1.25 * oo + 0.02
    assert gvec.norm().item() <= C * 1.02 * valid / L
    assert (sq[valid:] == 0).all() and (clip[valid:] == 0).all()


# ---- PoissonLoader + graphed_step -----------------------------------------------------------------------------------
N_REC, CAP, HALF = 12, 8, 2 ** 63


def counts_of(seed, steps):
    """What a DeviceSampler(debug_seed=seed) selects from N_REC records at q = 1/2 in its first steps (host reference)."""
    s = DeviceSampler("cpu", debug_seed=seed)
    blocks = (N_REC + 7) // 8
    return [int((chacha20_words(s.key_words + (s.nonce,), i * blocks, N_REC) < np.uint64(HALF)).sum())
            for i in range(steps)]


def sampler_seed():
    """The first debug seed whose first three batches have three different sizes, none empty, none above capacity."""
    for seed in range(1, 200):
        c = counts_of(seed, 3)
        if len(set(c)) == 3 and min(c) >= 1 and max(c) <= CAP:
            return seed, c
    raise AssertionError("no seed found")


def poisson_steps(cuda, sd, data, targets, seed, graphed):
    eng = ResNet18Engine(CAP, 3, 3, 64, "max", dtype=torch.float32, device=cuda, norm="group")
    eng.load_state_dict(sd)
    loader = PoissonLoader(data, targets, None, CAP, DeviceSampler(cuda, debug_seed=seed), threshold=HALF)
    eng.dp_params = dict(UNCLIPPED, expected_batch=loader.expected_batch)
    eng.dp_noise = DeviceNoise(cuda, debug_seed=8)
    opt = EngineOptimizer(eng, "SGD", lr=1e-2, weight_decay=5e-4)
    arenas, counts, losses = [], [], []
    for _ in range(3):
        x, y = loader.draw()
        counts.append(loader.count.cpu().tolist())
        if graphed:
            losses.append(graphed_step(eng, opt, x, y).clone())
        else:
            opt.zero_grad()
            eng.forward(x)
            losses.append(eng.loss_backward(y).clone())
            opt.step()
        arenas.append(eng.flat.clone())
    torch.cuda.synchronize()
    return eng, loader, arenas, counts, losses


def test_graphed_poisson_steps_match_eager(cuda):
    seed, want_counts = sampler_seed()
    sd = weights("group", 64, 11)
    g = torch.Generator().manual_seed(21)
    data = torch.randn(N_REC, 3, 64, 64, generator=g).to(cuda)
    targets = torch.randint(0, 3, (N_REC,), generator=g).to(cuda)
    e, le, ae, ce, lse = poisson_steps(cuda, sd, data, targets, seed, graphed=False)
    gr, lg, ag, cg, lsg = poisson_steps(cuda, sd, data, targets, seed, graphed=True)
    assert ce == cg == [[c, c] for c in want_counts], (ce, cg, want_counts)
    assert le.expected_batch == 6.0 and le.q == 0.5
    for i, (a, b) in enumerate(zip(ae, ag)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i
        assert torch.equal(lse[i], lsg[i]) and float(lse[i]) > 0
    assert not torch.equal(ae[0], ae[1]) and not torch.equal(ae[1], ae[2])
    caps = captures(gr)
    assert list(caps.values()) == [1], caps
    key = list(caps)[0]
    assert "Poisson-sampled" in key and "DP with device noise" in key and key[0] == CAP
    assert captures(e) == {}
    assert le.sampler.blocks_drawn() == lg.sampler.blocks_drawn() == 3 * 2
    assert e.dp_noise.blocks_drawn() == gr.dp_noise.blocks_drawn() == 3 * math.ceil(e.P / 16)
    assert le.sampler.overflow_events() == lg.sampler.overflow_events() == 0
    assert le.draws == lg.draws == 3
    # the batch itself: the selected records in ascending order, then zero images with target -1
    idx = lg.idx.cpu().tolist()
    kept = want_counts[2]
    assert idx[:kept] == sorted(idx[:kept]) and idx[kept:] == [-1] * (CAP - kept)
    assert torch.equal(lg.x[:kept], data[idx[:kept]]) and torch.equal(lg.y[:kept], targets[idx[:kept]])
    assert (lg.x[kept:] == 0).all() and (lg.y[kept:] == -1).all()


def test_poisson_loader_walks_and_refusals(cuda):
    """Two stored walks of 5 records: an epoch samples over the 5 and reads its own walk; len = ceil(n / L); L = n is
    refused."""
    data = torch.arange(10, dtype=torch.float32, device=cuda).view(10, 1).repeat(1, 4).contiguous()
    targets = (torch.arange(10, device=cuda) % 5) % 3
    loader = PoissonLoader(data, targets, 2, 5, DeviceSampler(cuda, debug_seed=3), repetitions=2)
    assert len(loader) == 3 and loader.n == 5 and loader.threshold == (2 << 64) // 5
    assert loader.q == loader.threshold / 2 ** 64
    for epoch in range(3):
        walk = epoch % 2
        for x, y in loader:
            kept = int(loader.count[1])
            rows = x[:kept, 0].cpu().tolist()
            assert all(5 * walk <= r < 5 * walk + 5 for r in rows), (epoch, rows)
            assert rows == [5.0 * walk + i for i in loader.idx[:kept].cpu().tolist()]
            assert (y[kept:] == -1).all() and (x[kept:] == 0).all()
    assert loader.draws == 9 and loader.sampler.blocks_drawn() == 9
    with pytest.raises(ValueError, match=">= 1"):
        PoissonLoader(data, targets, 5, 5, DeviceSampler(cuda, debug_seed=3), repetitions=2)
    # a record that is not a whole number of 16-byte chunks (a 1 x 3 x 3 fp32 image) is refused by name, before any draw
    with pytest.raises(ValueError, match="16-byte chunks"):
        PoissonLoader(torch.zeros(10, 1, 3, 3, device=cuda), targets, 2, 5, DeviceSampler(cuda, debug_seed=3))


def test_poisson_augmenting_loader_pads_the_transformed_batch(cuda):
    """The vanilla loop's loader: the kernel selects, the host reads idx / count back, the transform sees the kept images
    only and the batch is padded to capacity.  (A stand-in transform: uint8 HWC -> float CHW / 255.)"""
    class Tf:
        calls = []

        def batch(self, images, rng):
            self.calls.append(len(images))
            return torch.stack([im.permute(2, 0, 1).float() / 255.0 for im in images])

    n, cap = 9, 6
    g = torch.Generator().manual_seed(4)
    images = [torch.randint(0, 256, (8, 8, 1), generator=g, dtype=torch.uint8).to(cuda) for _ in range(n)]
    targets = torch.randint(0, 3, (n,), generator=g).to(cuda)
    base = type("AugmentingLoader", (), {})()
    base.images, base.targets, base.tf, base.rng = images, targets, Tf(), None
    sampler = DeviceSampler(cuda, debug_seed=6)
    loader = from_loader(base, 3, cap, sampler, shape=(1, 8, 8))
    assert isinstance(loader, PoissonAugmentingLoader) and len(loader) == 3 and loader.threshold == (3 << 64) // 9
    key = sampler.key_words + (sampler.nonce,)
    for step, (x, y) in enumerate(loader):
        sel = np.nonzero(chacha20_words(key, 2 * step, n) < np.uint64(loader.threshold))[0][:cap]
        assert loader.count.cpu().tolist()[1] == len(sel) and x.shape == (cap, 1, 8, 8)
        for s, i in enumerate(sel):
            assert torch.equal(x[s], images[i].permute(2, 0, 1).float() / 255.0) and int(y[s]) == int(targets[i])
        assert (x[len(sel):] == 0).all() and (y[len(sel):] == -1).all()
    assert loader.draws == 3 and sum(1 for c in Tf.calls if c == 0) == 0


# ---- the CLI ---------------------------------------------------------------------------------------------------------
LINE = re.compile(r"\[dp\] (\w+): \(epsilon, delta\) = \(([^,]+), ([^)]+)\) at order ([\d.]+), q = ([^,]+), "
                  r"sigma = ([^,]+), steps = (\d+), capacity = (\d+), overflow events = (\d+)( \(end of run\))?")


def dp_config(tmp_path, epochs=5):
    """epochs = 5: ONE federated epoch (the federated loop runs epochs / repetitions_dataset of them)."""
    text = open(os.path.join(ROOT, "configs", "torch", "smoke-federated.ini")).read()
    for a, b in (("differentially_private = no", "differentially_private = yes"), ("pretrained = yes", "pretrained = no"),
                 ("epochs = 10", "epochs = {:d}".format(epochs))):
        assert a in text, a
        text = text.replace(a, b)
    ini = tmp_path / "dp.ini"
    ini.write_text(text)
    return str(ini)


def run_cli(ini, name, extra, federated=True, noise="chacha"):
    env = dict(os.environ, PRIMIA_SYNTHETIC_BATCHES="3", PRIMIA_DTYPE="bf16")
    cmd = [sys.executable, "train.py", "--config", ini, "--cuda", "--data_dir", "synthetic", "--dp_noise", noise,
           "--training_name", name] + (["--train_federated"] if federated else []) + extra
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def ledger_lines(stdout, final):
    out = {}
    for m in LINE.finditer(stdout):
        if bool(m.group(10)) == final:
            out[m.group(1)] = dict(eps=float(m.group(2)), delta=float(m.group(3)), alpha=float(m.group(4)),
                                   q=float(m.group(5)), sigma=float(m.group(6)), steps=int(m.group(7)),
                                   capacity=int(m.group(8)), overflow=int(m.group(9)))
    return out


def check_lines(lines, steps, past_plan=False):
    """Three clients with 24 / 16 / 16 synthetic records (three, two, two batches of 8).  epsilon is the accountant's at
    0.99 of the TARGET delta; the reported delta is the target unless the truncation event outgrew its 1% (possible in
    the resumed run: its first epoch ran at a capacity sized for that epoch alone), when it is larger."""
    assert sorted(lines) == ["alice", "bob", "charlie"], lines
    for name, n in (("alice", 24), ("bob", 16), ("charlie", 16)):
        got = lines[name]
        assert got["q"] == ((8 << 64) // n) / 2 ** 64 and got["sigma"] == 1.3
        assert got["delta"] >= 1e-5 if past_plan else got["delta"] == 1e-5
        assert got["steps"] == steps[name]
        eps, alpha = A.epsilon([(got["q"], got["sigma"], got["steps"])], 0.99 * 1e-5)
        assert abs(got["eps"] - eps) <= 1e-5 * eps and got["alpha"] == alpha
        assert math.ceil(got["q"] * n) <= got["capacity"] <= n


def test_cli_poisson_sampling_reports_and_resumes(tmp_path):
    """train.py --dp_sampling poisson under --hip_graph: one (epsilon, delta) line per client and epoch, the accountant's
    for the printed q, sigma and steps; the checkpoint carries the ledger and a resumed epoch goes on counting."""
    ini = dp_config(tmp_path)
    ckpt = os.path.join(ROOT, "model_weights", "final_federated_dppoisson.pt")
    kept = str(tmp_path / "first.pt")
    try:
        r = run_cli(ini, "dppoisson", ["--dp_sampling", "poisson", "--hip_graph"])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        first = {"alice": 3, "bob": 2, "charlie": 2}
        check_lines(ledger_lines(r.stdout, final=False), first)
        check_lines(ledger_lines(r.stdout, final=True), first)
        state = torch.load(ckpt, map_location="cpu", weights_only=False)
        assert sorted(state["dp_privacy"]) == ["alice", "bob", "charlie"]
        led = A.Ledger.from_state_dict(state["dp_privacy"]["alice"])
        assert led.steps == 3 and led.n == 24 and len(led.segments) == 1 and led.segments[0][1] == 1.3
        assert all(bool(torch.isfinite(v).all()) for v in state["model_state_dict"].values())
        shutil.copyfile(ckpt, kept)
        r = run_cli(ini, "dppoisson", ["--dp_sampling", "poisson", "--resume_checkpoint", kept])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = ledger_lines(r.stdout, final=True)
        check_lines(lines, {k: 2 * v for k, v in first.items()}, past_plan=True)
        assert ("no longer fits its share of delta" in r.stderr) == any(v["delta"] > 1e-5 for v in lines.values())
        again = torch.load(ckpt, map_location="cpu", weights_only=False)["dp_privacy"]
        assert A.Ledger.from_state_dict(again["bob"]).segments == [[((8 << 64) // 16) / 2 ** 64, 1.3, 4]]
        # the resumed run planned for the checkpoint's steps plus its own epoch, and every segment knows its capacity
        alice = A.Ledger.from_state_dict(again["alice"])
        assert alice.planned_steps == 6 and alice.steps == 6 and sum(t for _, _, t in alice.segments) == 6
        assert len(alice.capacities) == len(alice.segments) and alice.capacities[0] == state["dp_privacy"]["alice"]["capacity"]
        assert alice.capacities[-1] == lines["alice"]["capacity"] >= alice.capacities[0]
    finally:
        if os.path.exists(ckpt):
            os.remove(ckpt)


def test_cli_without_poisson_sampling_reports_nothing(tmp_path):
    ckpt = os.path.join(ROOT, "model_weights", "final_federated_dpshuffle.pt")
    try:
        r = run_cli(dp_config(tmp_path), "dpshuffle", [])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "[dp]" not in r.stdout and "(epsilon, delta)" not in r.stdout
        assert "dp_privacy" not in torch.load(ckpt, map_location="cpu", weights_only=False)
    finally:
        if os.path.exists(ckpt):
            os.remove(ckpt)


def test_cli_vanilla_poisson_sampling_with_torch_noise(tmp_path):
    """Without --train_federated the one model is the one client ("model", 24 synthetic records, two epochs of three
    steps); --dp_noise torch is allowed."""
    ckpt = os.path.join(ROOT, "model_weights", "final_vanilla_dppoissonvanilla.pt")
    try:
        r = run_cli(dp_config(tmp_path, epochs=2), "dppoissonvanilla", ["--dp_sampling", "poisson", "--dp_delta", "1e-6"],
                    federated=False, noise="torch")
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        final = ledger_lines(r.stdout, final=True)
        assert sorted(final) == ["model"] and final["model"]["steps"] == 6 and final["model"]["delta"] == 1e-6
        assert final["model"]["q"] == ((8 << 64) // 24) / 2 ** 64
        eps, _ = A.epsilon([(final["model"]["q"], 1.3, 6)], 0.99e-6)
        assert abs(final["model"]["eps"] - eps) <= 1e-5 * eps
        per_epoch = [m for m in LINE.finditer(r.stdout) if not m.group(10)]
        assert [int(m.group(7)) for m in per_epoch] == [3, 6]
        led = torch.load(ckpt, map_location="cpu", weights_only=False)["dp_privacy"]["model"]
        # (the final checkpoint is the best epoch's: its ledger is that epoch's)
        assert led["segments"] in ([[final["model"]["q"], 1.3, 3]], [[final["model"]["q"], 1.3, 6]]) and led["delta"] == 1e-6
    finally:
        if os.path.exists(ckpt):
            os.remove(ckpt)
