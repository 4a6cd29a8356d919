"""CPU checks of the DP-SGD device noise (primia_dp_noise_add, primia_amd.dp_noise.DeviceNoise, train.py --dp_noise): the
two entry points are declared and exported, bad arguments are refused on the host, the DEFINITION of the noise (its float64
form, tests/dp_noise_ref.py) is a standard normal sample truncated at 5.77, keys are handled as documented, the CLI offers
the flag and an engine with a device noise stream is no longer held to eager steps (no GPU needed)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import torch

from primia_amd import _lib, graphed_train
from primia_amd.dp_noise import DeviceNoise
from tests import dp_noise_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_entry_points_declared_and_exported():
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("primia_dp_noise_add", "primia_dp_noise_blocks"):
        assert name in protos, name
        assert hasattr(lib, name), name
    assert [n for _, n in protos["primia_dp_noise_add"][1]] == ["k0", "k1", "k2", "k3", "nonce", "counter", "block_offset",
                                                               "g", "n", "sigma", "inv_batch", "stream"]
    assert protos["primia_dp_noise_blocks"][0] is ctypes.c_int64
    assert _lib.lib().primia_abi_version() == 1            # additions only


def test_blocks_per_call():
    assert [_lib.query("primia_dp_noise_blocks", n) for n in (0, 1, 16, 17)] == [0, 1, 1, 2]
    assert _lib.query("primia_dp_noise_blocks", 11178051) == R.noise_blocks(11178051) == 698629


def test_refuses_bad_arguments_before_launching():
    # checked on the host: a null or misaligned gradient pointer and a negative count never reach a launch
    f = _lib.lib().primia_dp_noise_add
    k = R.KEY + (R.NONCE,)
    assert f(*k, None, 0, None, 16, 1.0, 1.0, None) == -1
    assert f(*k, None, 0, ctypes.c_void_p(20), 16, 1.0, 1.0, None) == -1
    assert f(*k, None, 0, ctypes.c_void_p(16), -1, 1.0, 1.0, None) == -1
    assert f(*k, None, 0, None, 0, 1.0, 1.0, None) == 0             # n == 0: a no-op, pointers may be null


def test_the_definition_is_a_truncated_standard_normal():
    """2^20 values of the float64 reference from block 7 of the fixed key: mean, variance, excess kurtosis, the correlation
    of the two values of a Box-Muller pair and the lag-1 correlation, each within 5 standard errors; no value past the
    24-bit truncation point.  (Measured: 0.45, 0.03, 0.45, 0.7 and 1.4 standard errors, max |z| = 5.23.)"""
    n = 2 ** 20
    z = R.reference_noise(R.KEY, R.NONCE, 7, n)
    assert z.shape == (n,)
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2 - 3.0
    pair = (z[0::2] * z[1::2]).mean()
    lag1 = (z[:-1] * z[1:]).mean()
    figures = {"mean": (mean, 1 / np.sqrt(n)), "variance": (var - 1.0, np.sqrt(2 / n)), "kurtosis": (kurt, np.sqrt(24 / n)),
               "even/odd": (pair, 1 / np.sqrt(n / 2)), "lag 1": (lag1, 1 / np.sqrt(n))}
    for name, (v, se) in figures.items():
        print(f"{name}: {v:+.3e} = {abs(v) / se:.2f} standard errors")
    print(f"max |z| = {np.abs(z).max():.3f}")
    for name, (v, se) in figures.items():
        assert abs(v) <= 5 * se, (name, v, se)
    assert np.abs(z).max() <= R.TAIL
    # the pieces of the definition: a partial block is a prefix, a later block is an offset into the same stream
    assert np.array_equal(R.reference_noise(R.KEY, R.NONCE, 7, 21), z[:21])
    assert np.array_equal(R.reference_noise(R.KEY, R.NONCE, 9, 16), z[32:48])


def test_device_noise_keys():
    a, b = DeviceNoise("cpu"), DeviceNoise("cpu")
    assert len(a.key) == 32 and a.key != b.key and not a.predictable
    s1, s2, s3, s4 = (DeviceNoise("cpu", debug_seed=1), DeviceNoise("cpu", debug_seed=1),
                      DeviceNoise("cpu", debug_seed=1, nonce=1), DeviceNoise("cpu", debug_seed=2))
    assert s1.predictable and s1.key == s2.key and s1.key_words == s2.key_words
    assert s3.key != s1.key and s4.key != s1.key and s3.nonce == 1
    k = bytes(range(32))
    d = DeviceNoise("cpu", key=k, nonce=R.NONCE)
    assert d.key_words == R.KEY and d.nonce == R.NONCE and not d.predictable
    # the counter is a device word created at first use: one int64 zero
    assert d.counter.dtype == torch.int64 and d.counter.numel() == 1 and d.blocks_drawn() == 0


def test_train_cli_lists_dp_noise():
    r = subprocess.run([sys.executable, "train.py", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--dp_noise" in r.stdout and "--debug_dp_noise_seed" in r.stdout


class _Engine:
    """What eager_reason reads of an engine."""

    def __init__(self, n):
        self.N, self._root, self.training = n, self, True
        self.dp_params = {"max_grad_norm": 1.0, "noise_multiplier": 1.3}


class _Opt:
    kind = "SGD"


def test_device_noise_lifts_the_eager_rule():
    eng = _Engine(4)
    assert "DP-SGD" in graphed_train.eager_reason(eng, _Opt(), 4)           # no dp_noise attribute at all
    eng.dp_noise = None
    assert "DP-SGD" in graphed_train.eager_reason(eng, _Opt(), 4)
    eng.dp_noise = DeviceNoise("cpu", debug_seed=3)
    assert graphed_train.eager_reason(eng, _Opt(), 4) is None
    assert "batch size 3" in graphed_train.eager_reason(eng, _Opt(), 3)     # the other rules still hold
