"""Host: what train.py decides about --dp_micro_batches before anything touches a GPU, the three entry points of a DP-SGD
step cut into micro-batch passes (declared, exported, bad arguments refused before a launch), and that an engine without
a phase keeps the graph key it had (no GPU needed)."""
import ctypes
import warnings
from types import SimpleNamespace

import pytest

import train
from primia_amd import _lib, dp_micro, graphed_train
from primia_amd.dp_noise import DeviceNoise


def test_parser_default_and_refusal():
    p = train.build_parser()
    assert p.parse_args(["--config", "x.ini"]).dp_micro_batches == 1
    assert p.parse_args(["--config", "x.ini", "--dp_micro_batches", "5"]).dp_micro_batches == 5
    for bad in ("0", "-2", "two"):
        with pytest.raises(SystemExit):
            p.parse_args(["--config", "x.ini", "--dp_micro_batches", bad])


def test_micro_batches_without_dp_warn_and_do_nothing():
    cmd = SimpleNamespace(dp_micro_batches=4)
    with pytest.warns(UserWarning, match="--dp_micro_batches 4 has no effect"):
        assert train.DPOptions.from_args(SimpleNamespace(differentially_private=False), cmd).micro == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert train.DPOptions.from_args(SimpleNamespace(differentially_private=True), cmd).micro == 4
        assert train.DPOptions.from_args(SimpleNamespace(differentially_private=False), SimpleNamespace()).micro == 1
        assert train.DPOptions.from_args(SimpleNamespace(differentially_private=False),
                                         SimpleNamespace(dp_micro_batches=1)).micro == 1
        assert train.DPOptions.from_args(SimpleNamespace(differentially_private=True), None).micro == 1


def test_the_size_of_a_pass():
    with pytest.raises(SystemExit, match=r"3 does not divide batch_size 8"):
        train.micro_batch_size(8, 3, False)
    assert train.micro_batch_size(8, 2, False) == 4 and train.micro_batch_size(8, 1, False) == 8
    assert train.micro_batch_size(8, 2, True) == 4 and train.micro_batch_size(8, 3, True) == 3
    assert train.micro_batch_size(1275, 5, True) == 255 and train.micro_batch_size(7, 1, True) == 7
    assert dp_micro.views(8, 4) == [(0, 4), (4, 8)] and dp_micro.views(7, 4) == [(0, 4), (4, 7)]
    assert dp_micro.views(9, 3) == [(0, 3), (3, 6), (6, 9)] and dp_micro.views(3, 4) == [(0, 3)]
    assert [dp_micro.phase_of(i, 3) for i in range(3)] == ["first", "more", "last"]
    assert [dp_micro.phase_of(i, 2) for i in range(2)] == ["first", "last"] and dp_micro.phase_of(0, 1) is None


def test_the_plan_does_not_know_about_micro_batches():
    """q, the planned steps and the capacity come from (records, batch_size, epochs, delta, sigma) alone: poisson_plan has
    no K to be given, and the loaders' capacity is the plan's whatever K."""
    import inspect

    assert "micro" not in " ".join(inspect.signature(train.poisson_plan).parameters)
    plan = train.poisson_plan("alice", 5163, 1024, 40, 1e-5, 1.3)
    assert plan[2] == 1275 and plan[1] == 240
    for k in (1, 2, 5):
        assert train.micro_batch_size(plan[2], k, True) * k >= plan[2]
        assert train.poisson_plan("alice", 5163, 1024, 40, 1e-5, 1.3) == plan


def test_entry_points_declared_and_exported():
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("primia_dp_accumulate", "primia_dp_noise_add_acc", "primia_dp_add_noise_acc"):
        assert name in protos, name
        assert hasattr(lib, name), name
    assert [n for _, n in protos["primia_dp_accumulate"][1]] == ["acc", "g", "n", "overwrite", "stream"]
    assert [n for _, n in protos["primia_dp_noise_add_acc"][1]] == ["k0", "k1", "k2", "k3", "nonce", "counter", "block_offset",
                                                                   "g", "acc", "n", "sigma", "inv_batch", "stream"]
    assert [n for _, n in protos["primia_dp_add_noise_acc"][1]] == ["g", "acc", "noise", "n", "sigma", "inv_batch", "stream"]
    assert _lib.lib().primia_abi_version() == 1            # additions only


def test_refuse_bad_arguments_before_launching():
    # checked on the host: null or misaligned pointers and a negative count never reach a launch
    f = _lib.lib().primia_dp_accumulate
    ok = ctypes.c_void_p(64)
    assert f(None, ok, 16, 0, None) == -1 and f(ok, None, 16, 1, None) == -1
    assert f(ctypes.c_void_p(68), ok, 16, 0, None) == -1          # a misaligned acc
    assert f(ok, ctypes.c_void_p(72), 16, 0, None) == -1          # a misaligned g
    assert f(ok, ok, -1, 0, None) == -1
    assert f(None, None, 0, 0, None) == 0                         # n == 0: a no-op, pointers may be null
    h = _lib.lib().primia_dp_noise_add_acc
    k = (1, 2, 3, 4, 5)
    assert h(*k, None, 0, None, ok, 16, 1.0, 1.0, None) == -1 and h(*k, None, 0, ok, None, 16, 1.0, 1.0, None) == -1
    assert h(*k, None, 0, ok, ctypes.c_void_p(68), 16, 1.0, 1.0, None) == -1
    assert h(*k, None, 0, ctypes.c_void_p(68), ok, 16, 1.0, 1.0, None) == -1
    assert h(*k, None, 0, None, None, 0, 1.0, 1.0, None) == 0
    a = _lib.lib().primia_dp_add_noise_acc
    assert a(None, ok, ok, 16, 1.0, 1.0, None) == -1 and a(ok, None, ok, 16, 1.0, 1.0, None) == -1
    assert a(ok, ok, None, 16, 1.0, 1.0, None) == -1 and a(None, None, None, 0, 1.0, 1.0, None) == 0


class _Engine:
    """What _key reads of an engine: one from before micro-batches, with no phase attribute at all."""

    def __init__(self, n):
        self.N, self._root, self.training = n, self, True
        self.fuse_sgd_tail, self.class_weight, self.norm = True, None, "group"
        self.dp_params = {"max_grad_norm": 1.0, "noise_multiplier": 1.3, "expected_batch": 6.0}
        self.dp_noise = DeviceNoise("cpu", debug_seed=3)


class _Opt:
    kind = "SGD"


def test_the_key_without_a_phase_is_the_key_as_it_was():
    eng = _Engine(4)
    want = (4, False, "SGD", True, False, "DP with device noise", 1.0, 1.3, eng.dp_noise.key_words + (eng.dp_noise.nonce,),
            "Poisson-sampled", 6.0)
    assert graphed_train._key(eng, _Opt(), False) == want
    assert graphed_train._key(eng, _Opt(), False, phase=None, logical_batch=None) == want
    assert graphed_train._key(eng, _Opt(), False, phase="first", logical_batch=8) == want + ("micro-batch", "first", 1.0 / 6.0)
    del eng.dp_params["expected_batch"]
    assert graphed_train._key(eng, _Opt(), False, phase="last", logical_batch=8) == want[:-2] + ("micro-batch", "last", 1.0 / 8.0)
    assert graphed_train.eager_reason(eng, _Opt(), 4) is None and "batch size 3" in graphed_train.eager_reason(eng, _Opt(), 3)
