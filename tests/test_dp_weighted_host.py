"""Host: DP-SGD with class weights before anything touches a GPU — the new entry points' declarations and refusals, the
weights formed from released counts, the ledger's one-off releases, and what train.py decides about weight_classes / mixup
under differentially_private = yes (no GPU needed)."""
import ctypes
import math
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import train
from primia_amd import _lib
from primia_amd import dp_accountant as A
from primia_amd.dp_weights import balanced_weights
from tests import dp_weighted_ref as W


# ---- 1. the C ABI ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_refuse_bad_arguments():
    protos = _lib.protos()
    lib = _lib.lib()
    for n in ("primia_xent_dp_weighted", "primia_dp_class_counts", "primia_dp_class_counts_chacha"):
        assert n in protos and hasattr(lib, n), n
        assert protos[n][0] is ctypes.c_int
    assert [a for _, a in protos["primia_xent_dp_weighted"][1]] == ["logits", "target", "class_weight", "scale", "loss",
                                                                     "dlogits", "N", "C", "stream"]
    assert [t for t, _ in protos["primia_xent_dp_weighted"][1]][3] is ctypes.c_float
    assert [a for _, a in protos["primia_dp_class_counts"][1]] == ["targets", "n", "C", "z", "sigma", "counts_out", "stream"]
    assert [a for _, a in protos["primia_dp_class_counts_chacha"][1]] == [
        "k0", "k1", "k2", "k3", "nonce", "counter", "block_offset", "targets", "n", "C", "sigma", "counts_out", "stream"]
    # refused before any launch (non-null pointers that are never dereferenced)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    x = lib.primia_xent_dp_weighted
    for bad in ((None, p, p, 1.0, p, p, 4, 3), (p, None, p, 1.0, p, p, 4, 3), (p, p, None, 1.0, p, p, 4, 3),
                (p, p, p, 1.0, None, p, 4, 3), (p, p, p, 0.0, p, p, 4, 3), (p, p, p, -0.5, p, p, 4, 3),
                (p, p, p, float("nan"), p, p, 4, 3), (p, p, p, 1.0, p, p, 0, 3), (p, p, p, 1.0, p, p, 4, 0)):
        assert x(*bad, None) == -1, bad
    c, h = lib.primia_dp_class_counts, lib.primia_dp_class_counts_chacha
    for n, C, sigma, out, tg in ((5, 17, 1.0, p, p), (5, 0, 1.0, p, p), (-1, 3, 1.0, p, p), (5, 3, -1.0, p, p),
                                 (5, 3, float("inf"), p, p), (5, 3, 1.0, None, p), (5, 3, 1.0, p, None)):
        assert c(tg, n, C, p, sigma, out, None) == -1, (n, C, sigma)
        assert h(1, 2, 3, 4, 5, p, 0, tg, n, C, sigma, out, None) == -1, (n, C, sigma)


# ---- 2. the weights -------------------------------------------------------------------------------------------------------
def test_balanced_weights():
    for k in (1, 7, 1349, 10 ** 9):
        for C in (2, 3, 16):
            w = balanced_weights(torch.full((C,), k, dtype=torch.int64))
            assert w.dtype == torch.float32 and w.tolist() == [1.0] * C
    counts = (1349, 2538, 1345)
    w = balanced_weights(torch.tensor(counts))
    want = W.balanced_weights(counts)
    assert np.array_equal(w.numpy(), want.astype(np.float32))
    assert np.allclose(want, [sum(counts) / (3 * c) for c in counts], rtol=1e-15)
    assert w[1] < 1 < w[0] < w[2]
    z = balanced_weights(torch.tensor([0, 10, 20]))         # a released count can be 0: it is clamped at 1
    assert torch.isfinite(z).all() and z.tolist() == [np.float32(31 / 3), np.float32(31 / 30), np.float32(31 / 60)]
    assert torch.equal(balanced_weights([0.0, 10.0, 20.0]), z) and torch.equal(balanced_weights(torch.tensor([-4, 10, 20])), z)


# ---- 3. the ledger --------------------------------------------------------------------------------------------------------
Q, SIGMA, STEPS, DELTA = 256 / 1721, 1.3, 280, 1e-5


def test_one_release_is_the_gaussian_mechanism():
    led = A.Ledger(1721, 300, DELTA, STEPS)
    led.add_release(5.0)
    want = min(a / 50.0 + math.log(1.0 / (0.99 * DELTA)) / (a - 1.0) for a in led.alphas)
    r = led.report()
    assert abs(r["epsilon"] - want) <= 1e-12 and r["steps"] == 0 and r["within_plan"]
    assert A.epsilon([], 0.99 * DELTA, releases=[(5.0, 1.0)])[0] == r["epsilon"]
    assert A.total_rdp([], [2.0, 8.0], [(5.0, 1.0), (10.0, 2.0)]) == [2.0 / 50 + 2.0 * 4 / 200, 8.0 / 50 + 8.0 * 4 / 200]
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            led.add_release(bad)


def test_steps_plus_a_release():
    plain = A.Ledger(1721, 300, DELTA, STEPS)
    plain.add_steps(Q, SIGMA, STEPS)
    both = A.Ledger(1721, 300, DELTA, STEPS)
    both.add_steps(Q, SIGMA, STEPS)
    both.add_release(20.0)
    alone = A.Ledger(1721, 300, DELTA, STEPS)
    alone.add_release(20.0)
    e0, e1, er = plain.report()["epsilon"], both.report()["epsilon"], alone.report()["epsilon"]
    assert e0 < e1 < e0 + er
    # what a caller that passes no releases gets has not moved: the README's Poisson example
    assert e0 == A.epsilon([(Q, SIGMA, STEPS)], 0.99 * DELTA)[0] == A.epsilon([(Q, SIGMA, STEPS)], 0.99 * DELTA, None, ())[0]
    assert A.total_rdp([(Q, SIGMA, STEPS)]) == A.total_rdp([(Q, SIGMA, STEPS)], None, ())
    assert abs(e0 - 14.0286) < 5e-5 and abs(e1 - 14.0321) < 5e-5
    ten = A.epsilon([(Q, SIGMA, STEPS)], 0.99 * DELTA, releases=[(10.0, 1.0)])[0]
    assert abs(ten - 14.0426) < 5e-5
    assert "class counts at sigma = 20.0" in both.line("alice") and "release" not in plain.line("alice")
    # the capacity plan sizes itself on the steps plus the release
    assert A.capacity_for(1721, Q, STEPS, DELTA, eps=e1) >= A.capacity_for(1721, Q, STEPS, DELTA, sigma=SIGMA)


def test_releases_travel_in_the_state_dict():
    led = A.Ledger(1721, 300, DELTA, STEPS)
    led.add_steps(Q, SIGMA, 7)
    led.add_release(20.0)
    led.add_release(8.0, sensitivity=0.5, what="another histogram")
    sd = led.state_dict()
    assert sd["releases"] == [[20.0, 1.0, "class counts"], [8.0, 0.5, "another histogram"]]
    back = A.Ledger.from_state_dict(sd)
    assert back.releases == led.releases and back.report() == led.report() and back.state_dict() == sd
    old = {k: v for k, v in sd.items() if k != "releases"}        # a checkpoint from before releases existed
    before = A.Ledger.from_state_dict(old)
    assert before.releases == []
    assert before.report()["epsilon"] == A.epsilon([(Q, SIGMA, 7)], 0.99 * DELTA)[0]
    assert before.state_dict()["releases"] == []


# ---- 4. train.py's decisions ------------------------------------------------------------------------------------------------
def config(**kw):
    return SimpleNamespace(**{"differentially_private": True, "pretrained": False, "batch_size": 8, "mixup": False,
                              "weight_classes": False, **kw})


def test_mixup_stays_refused_and_says_why():
    for cmd in (None, SimpleNamespace(dp_sampling="poisson"), SimpleNamespace(dp_sampling="shuffle")):
        for wc in (False, True):
            with pytest.raises(SystemExit, match="two records") as e:
                train.DPOptions.from_args(config(mixup=True, weight_classes=wc), cmd)
            assert "mixup" in str(e.value) and "Poisson" in str(e.value) and "weight_classes" not in str(e.value)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not train.DPOptions.from_args(config(differentially_private=False, mixup=True, weight_classes=True), None).weighted


def test_weight_classes_is_accepted_under_dp():
    p = train.build_parser()
    assert p.parse_args(["--config", "x.ini"]).dp_weight_sigma == 20.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        dp = train.DPOptions.from_args(config(weight_classes=True), p.parse_args(["--config", "x.ini"]))
        assert dp.on and dp.weighted and dp.weight_sigma == 20.0
        dp = train.DPOptions.from_args(config(weight_classes=True),
                                       p.parse_args(["--config", "x.ini", "--dp_weight_sigma", "7.5", "--dp_sampling", "poisson"]))
        assert dp.weighted and dp.weight_sigma == 7.5 and dp.poisson
        assert train.DPOptions.from_args(config(weight_classes=True), None).weight_sigma == 20.0
        assert not train.DPOptions.from_args(config(), None).weighted
        assert not train.DPOptions().weighted and train.DPOptions().weight_sigma == 20.0


def test_a_count_noise_of_zero_is_refused():
    p = train.build_parser()
    for bad in ("0", "-3"):
        with pytest.raises(SystemExit, match="dp_weight_sigma"):
            train.DPOptions.from_args(config(weight_classes=True), p.parse_args(["--config", "x.ini", "--dp_weight_sigma", bad]))


def test_the_dp_path_keeps_hard_labels():
    """imagefolder.register and SyntheticLoader make one-hot rows for federated weight_classes only without DP."""
    from primia_amd.imagefolder import register

    data, targets = torch.zeros(4, 1, 2, 2), torch.tensor([0, 1, 2, 1])
    args = SimpleNamespace(train_federated=True, mixup=False, weight_classes=True, differentially_private=True,
                           repetitions_dataset=2)
    x, y = register([data, data], targets, args, 3, 0)
    assert y.dtype == torch.int64 and y.tolist() == [0, 1, 2, 1] * 2 and x.shape[0] == 8
    sl = train.SyntheticLoader(2, 4, 8, 3, "cpu", 1, 1, SimpleNamespace(**{**vars(args), "mixup_prob": 0.9}))
    assert sl.targets.dtype == torch.int64 and sl.targets.dim() == 1
