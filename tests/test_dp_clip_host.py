"""Host: the arithmetic of DP-SGD's adaptive clipping norm (primia_amd.dp_clip, tests/dp_clip_ref.py), the entry points'
declarations and host-side refusals, and what train.py decides about --dp_clip before anything touches a GPU."""
import ctypes
import math
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import train
from primia_amd import _lib, dp_clip, graphed_train
from primia_amd.dp_noise import DeviceNoise
from tests import dp_clip_ref as C

ZS = (0.5, 1.0, 1.3, 4.0)
RATIOS = (0.5 + 1e-9, 0.51, 0.75, 1.0, 10.0, 1e3)       # sigma_b / z: from just above the bound upwards


@pytest.mark.parametrize("z", ZS)
def test_z_delta_pays_exactly_for_the_count(z):
    for r in RATIOS:
        sigma_b = r * z
        for zd in (dp_clip.z_delta(z, sigma_b), C.z_delta(z, sigma_b)):
            total = zd ** -2 + (2.0 * sigma_b) ** -2
            assert abs(total - z ** -2) <= 1e-12 * z ** -2, (z, sigma_b, zd)
            assert zd > z                                   # the gradient's noise is raised, never lowered
    assert abs(dp_clip.z_delta(1.3, 12.8) - 1.3) < 2e-3     # at B / 20 of a batch of 256 the raise is 0.13%


@pytest.mark.parametrize("z", ZS)
def test_z_delta_refuses_the_bound_and_below(z):
    for sigma_b in (z / 2.0, z / 2.0 * (1 - 1e-12), z / 4.0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            dp_clip.z_delta(z, sigma_b)
        with pytest.raises(ValueError):
            C.z_delta(z, sigma_b)
    with pytest.raises(ValueError, match=r"z / 2 = 0\.65"):
        dp_clip.z_delta(1.3, 0.65)


def test_reference_update_moves_towards_the_quantile_and_stays_in_range():
    kw = dict(sigma_b=1.0, inv_batch=1.0 / 8, eta=0.2, gamma=0.5, c_min=1e-6, c_max=1e6)
    for c0 in (C.f32(1e-4), 1.0, 250.0):
        for below in range(9):
            for z0 in (-2.0, 0.0, 0.25, 2.0):
                b = C.released(below, 8, z0, 1.0, 1.0 / 8)
                assert b == ((below - 4.0) + z0) / 8 + 0.5
                c1 = C.update(c0, below, 8, z0, **kw)
                if b > 0.5:
                    assert c1 < c0
                elif b < 0.5:
                    assert c1 > c0
                else:
                    assert c1 == c0
                assert 1e-6 <= c1 <= 1e6
    # the ends of the range hold whatever the count says
    assert C.update(1.0, 8, 8, 0.0, 1.0, 1 / 8, 50.0, 0.5, 0.9, 1.1) == C.f32(0.9)
    assert C.update(1.0, 0, 8, 0.0, 1.0, 1 / 8, 50.0, 0.5, 0.9, 1.1) == C.f32(1.1)
    # an empty step (no valid sample) moves C by its noise alone
    assert C.update(2.0, 0, 0, 0.0, **kw) == 2.0 and C.update(2.0, 0, 0, 1.0, **kw) == 2.0 * math.exp(-C.f32(0.2) / 8)


def test_reference_counts():
    sq = np.array([0.25, 1.0, np.nextafter(1.0, 2.0), 4.0, 0.0])
    assert C.counts(sq, None, 1.0) == (3, 5)
    assert C.counts(sq, [0, -1, 2, 1, -1], 1.0) == (1, 3)
    assert C.counts(sq, [-1] * 5, 1.0) == (0, 0)
    c = np.float32(0.37)            # C * C in float64 of the float32 value, as the kernel forms it
    c2 = float(c) * float(c)
    assert C.counts([c2, np.nextafter(c2, 1.0)], None, 0.37) == (1, 2)


def test_adaptive_clip_parameters_and_state_dict():
    a = dp_clip.AdaptiveClip("cpu")
    assert (a.init, a.quantile, a.lr, a.sigma_b, a.c_min, a.c_max, a.updates) == (1.0, 0.5, 0.2, None, 1e-6, 1e6, 0)
    assert a.sigma_b_for(256) == 12.8 and a.noise_multiplier(1.3, 256) == dp_clip.z_delta(1.3, 12.8)
    with pytest.raises(ValueError):
        a.noise_multiplier(1.3, 13)                         # 13 / 20 = 0.65 = z / 2
    assert a.key(1.3, 256) == (0.2, 0.5, 12.8, 1e-6, 1e6, dp_clip.z_delta(1.3, 12.8))
    for bad in (dict(quantile=0.0), dict(quantile=1.0), dict(lr=-0.1), dict(c_min=0.0), dict(c_min=2.0, c_max=1.0),
                dict(init=1e7), dict(sigma_b=0.0), dict(lr=float("inf"))):
        with pytest.raises(ValueError):
            dp_clip.AdaptiveClip("cpu", **bad)
    b = dp_clip.AdaptiveClip("cpu", init=50.0, quantile=0.7, lr=0.3, sigma_b=2.0)
    assert b.value() == 50.0 and b.norm.dtype.is_floating_point and b.counts.tolist() == [0, 0]
    b.norm.fill_(12.5)
    b.updates = 9
    state = b.state_dict()
    assert state["clip_norm"] == 12.5 and state["updates"] == 9 and "counts" not in state      # the raw count is private
    ptr = a.norm.data_ptr()
    a.load_state_dict(state)
    assert a.norm.data_ptr() == ptr                         # in place: captured graphs read this word
    assert (a.value(), a.updates, a.quantile, a.lr, a.sigma_b, a.init) == (12.5, 9, 0.7, 0.3, 2.0, 50.0)
    state["clip_norm"] = 1e9
    with pytest.raises(ValueError):
        a.load_state_dict(state)
    # a resumed run (train.py) keeps ITS parameters and is told which of the saved ones differ
    c = dp_clip.AdaptiveClip("cpu", init=50.0, quantile=0.5, lr=0.3, sigma_b=1.0)
    state["clip_norm"] = 7.25
    assert c.differing_parameters(state) == {"quantile": (0.5, 0.7), "sigma_b": (1.0, 2.0)}
    c.load_state_dict(state, keep_parameters=True)
    assert (c.value(), c.updates, c.quantile, c.lr, c.sigma_b) == (7.25, 9, 0.5, 0.3, 1.0)
    assert b.differing_parameters(b.state_dict()) == {}


def test_entry_points_declared_and_exported():
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = ("primia_dp_clip_factors_dev", "primia_dp_noise_add_dev", "primia_dp_add_noise_dev", "primia_dp_clip_update",
             "primia_dp_clip_update_chacha")
    for name in names:
        assert name in protos, name
        assert hasattr(lib, name), name
    assert [n for _, n in protos["primia_dp_clip_factors_dev"][1]] == ["sq", "target", "clip", "N", "clip_norm", "counts",
                                                                      "overwrite", "stream"]
    assert [n for _, n in protos["primia_dp_noise_add_dev"][1]] == ["k0", "k1", "k2", "k3", "nonce", "counter", "block_offset",
                                                                   "g", "acc", "n", "clip_norm", "noise_multiplier",
                                                                   "inv_batch", "stream"]
    assert [n for _, n in protos["primia_dp_add_noise_dev"][1]] == ["g", "acc", "noise", "n", "clip_norm", "noise_multiplier",
                                                                   "inv_batch", "stream"]
    assert [n for _, n in protos["primia_dp_clip_update"][1]] == ["clip_norm", "counts", "z", "sigma_b", "inv_batch", "eta",
                                                                 "gamma", "c_min", "c_max", "released", "stream"]
    assert [n for _, n in protos["primia_dp_clip_update_chacha"][1]][:8] == ["k0", "k1", "k2", "k3", "nonce", "counter",
                                                                            "block_offset", "clip_norm"]
    assert _lib.lib().primia_abi_version() == 1            # additions only


OK = ctypes.c_void_p(64)
GOOD = dict(sigma_b=1.0, inv_batch=0.125, eta=0.2, gamma=0.5, c_min=1e-6, c_max=1e6)
BAD = [dict(sigma_b=0.0), dict(sigma_b=-1.0), dict(inv_batch=0.0), dict(inv_batch=-0.5), dict(eta=-0.1), dict(gamma=0.0),
       dict(gamma=1.0), dict(gamma=-0.2), dict(gamma=1.5), dict(c_min=0.0), dict(c_min=-1.0), dict(c_min=2.0, c_max=1.0)]
BAD += [{k: v} for k in GOOD for v in (float("nan"), float("inf"))]


def update_args(**over):
    p = dict(GOOD, **over)
    return tuple(p[k] for k in ("sigma_b", "inv_batch", "eta", "gamma", "c_min", "c_max"))


def test_update_refuses_bad_arguments_before_launching():
    """Checked on the host: nothing here reaches a launch (the pointers are not device memory)."""
    f, h = _lib.lib().primia_dp_clip_update, _lib.lib().primia_dp_clip_update_chacha
    k = (1, 2, 3, 4, 5)
    for ptrs in ((None, OK, OK), (OK, None, OK), (OK, OK, None)):
        assert f(*ptrs, *update_args(), None, None) == -1
    for ptrs in ((None, OK), (OK, None)):
        assert h(*k, None, 0, *ptrs, *update_args(), None, None) == -1
    for bad in BAD:
        assert f(OK, OK, OK, *update_args(**bad), None, None) == -1, bad
        assert h(*k, None, 0, OK, OK, *update_args(**bad), None, None) == -1, bad


def test_factor_and_noise_entry_points_refuse_bad_arguments_before_launching():
    c = _lib.lib().primia_dp_clip_factors_dev
    assert c(None, None, OK, 4, OK, OK, 1, None) == -1 and c(OK, None, None, 4, OK, OK, 1, None) == -1
    assert c(OK, None, OK, 4, None, OK, 1, None) == -1 and c(OK, None, OK, 4, OK, None, 1, None) == -1
    assert c(OK, None, OK, 0, OK, OK, 1, None) == -1 and c(OK, OK, OK, -3, OK, OK, 0, None) == -1
    # as primia_dp_noise_add / primia_dp_noise_add_acc: NULL or misaligned g, misaligned acc, n < 0; n == 0 is a no-op
    f = _lib.lib().primia_dp_noise_add_dev
    k = (1, 2, 3, 4, 5)
    assert f(*k, None, 0, None, None, 16, OK, 1.0, 1.0, None) == -1
    assert f(*k, None, 0, ctypes.c_void_p(68), None, 16, OK, 1.0, 1.0, None) == -1
    assert f(*k, None, 0, OK, ctypes.c_void_p(68), 16, OK, 1.0, 1.0, None) == -1
    assert f(*k, None, 0, OK, None, -1, OK, 1.0, 1.0, None) == -1
    assert f(*k, None, 0, OK, None, 16, None, 1.0, 1.0, None) == -1              # no clipping norm
    assert f(*k, None, 0, None, None, 0, None, 1.0, 1.0, None) == 0
    # as primia_dp_add_noise / primia_dp_add_noise_acc
    a = _lib.lib().primia_dp_add_noise_dev
    assert a(None, None, OK, 16, OK, 1.0, 1.0, None) == -1 and a(OK, None, None, 16, OK, 1.0, 1.0, None) == -1
    assert a(OK, None, OK, 16, None, 1.0, 1.0, None) == -1 and a(OK, None, OK, -1, OK, 1.0, 1.0, None) == -1
    assert a(None, None, None, 0, None, 1.0, 1.0, None) == 0


# ---- train.py -------------------------------------------------------------------------------------------------------------
def test_parser_defaults():
    p = train.build_parser()
    a = p.parse_args(["--config", "x.ini"])
    assert (a.dp_clip, a.dp_clip_quantile, a.dp_clip_lr, a.dp_clip_sigma, a.dp_clip_init) == ("fixed", 0.5, 0.2, None, 1.0)
    a = p.parse_args(["--config", "x.ini", "--dp_clip", "adaptive", "--dp_clip_quantile", "0.7", "--dp_clip_lr", "0.1",
                      "--dp_clip_sigma", "2.5", "--dp_clip_init", "50"])
    assert (a.dp_clip, a.dp_clip_quantile, a.dp_clip_lr, a.dp_clip_sigma, a.dp_clip_init) == ("adaptive", 0.7, 0.1, 2.5, 50.0)
    with pytest.raises(SystemExit):
        p.parse_args(["--config", "x.ini", "--dp_clip", "median"])


def cmd(**kw):
    return SimpleNamespace(**dict(dict(dp_clip="adaptive", dp_clip_quantile=0.5, dp_clip_lr=0.2, dp_clip_sigma=None,
                                       dp_clip_init=1.0), **kw))


def test_adaptive_clip_without_dp_warns_and_does_nothing():
    plain = SimpleNamespace(differentially_private=False, batch_size=8)
    with pytest.warns(UserWarning, match="--dp_clip adaptive has no effect"):
        assert train.DPOptions.from_args(plain, cmd(dp_clip_sigma=0.1)).clip is None        # (not even the bound is looked at)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert train.DPOptions.from_args(plain, cmd(dp_clip="fixed")).clip is None
        assert train.DPOptions.from_args(plain, SimpleNamespace()).clip is None
        assert train.DPOptions.from_args(SimpleNamespace(differentially_private=True, batch_size=8), None).clip is None
        got = train.DPOptions.from_args(SimpleNamespace(differentially_private=True, batch_size=256), cmd()).clip
    assert got == dict(init=1.0, quantile=0.5, lr=0.2, sigma_b=12.8, z_delta=dp_clip.z_delta(1.3, 12.8))


def test_a_count_noise_at_or_below_half_the_multiplier_ends_the_run():
    dp = SimpleNamespace(differentially_private=True, batch_size=256)
    for sigma in (0.65, 0.5, 0.0, -1.0):
        with pytest.raises(SystemExit, match=r"--dp_clip_sigma = .* must exceed half the noise multiplier, 1\.3 / 2 = 0\.65"):
            train.DPOptions.from_args(dp, cmd(dp_clip_sigma=sigma)).clip
    assert train.DPOptions.from_args(dp, cmd(dp_clip_sigma=0.66)).clip["sigma_b"] == 0.66
    # the default batch_size / 20: batches under 14 fall at or below the bound
    for batch in (13, 8, 1):
        with pytest.raises(SystemExit, match=r"batch_size / 20 = .* 1\.3 / 2 = 0\.65"):
            train.DPOptions.from_args(SimpleNamespace(differentially_private=True, batch_size=batch), cmd()).clip
    assert train.DPOptions.from_args(SimpleNamespace(differentially_private=True, batch_size=14), cmd()).clip["sigma_b"] == 0.7
    with pytest.raises(SystemExit, match="quantile"):
        train.DPOptions.from_args(dp, cmd(dp_clip_quantile=1.0)).clip


def test_a_checkpoint_without_the_entry_warns():
    with pytest.warns(UserWarning, match="holds no dp_clip entry"):
        assert train.saved_clip({"epoch": 1}) == {}
    assert train.saved_clip({"dp_clip": {"model": {"clip_norm": 2.0}}}) == {"model": {"clip_norm": 2.0}}


# ---- graph key --------------------------------------------------------------------------------------------------------------
class _Engine:
    """What _key reads of an engine."""

    def __init__(self, n):
        self.N, self._root, self.training = n, self, True
        self.fuse_sgd_tail, self.class_weight, self.norm = True, None, "group"
        self.dp_params = {"max_grad_norm": 1.0, "noise_multiplier": 1.3}
        self.dp_noise = DeviceNoise("cpu", debug_seed=3)


class _Opt:
    kind = "SGD"


def test_the_graph_key_holds_the_parameters_and_never_c():
    eng = _Engine(32)
    plain = graphed_train._key(eng, _Opt(), False)
    eng.dp_clip = None
    assert graphed_train._key(eng, _Opt(), False) == plain
    eng.dp_clip = dp_clip.AdaptiveClip("cpu", sigma_b=1.0)
    key = graphed_train._key(eng, _Opt(), False)
    assert key == plain + ("adaptive clip", 0.2, 0.5, 1.0, 1e-6, 1e6, dp_clip.z_delta(1.3, 1.0))
    eng.dp_clip.norm.fill_(123.0)                           # C moves: the same key
    eng.dp_clip.updates = 5
    assert graphed_train._key(eng, _Opt(), False) == key
    eng.dp_clip.lr = 0.1                                    # a parameter moves: another graph
    assert graphed_train._key(eng, _Opt(), False) != key
    # the default count noise follows the step's divisor: N, the logical batch of a micro-batch pass, the expected batch
    eng.dp_clip = dp_clip.AdaptiveClip("cpu")
    assert graphed_train._key(eng, _Opt(), False)[-4] == 32 / 20
    assert graphed_train._key(eng, _Opt(), False, phase="first", logical_batch=64)[-4] == 64 / 20
    eng.dp_params["expected_batch"] = 48.0
    assert graphed_train._key(eng, _Opt(), False, phase="first", logical_batch=64)[-4] == 48.0 / 20
