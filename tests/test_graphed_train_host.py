"""CPU checks of the graphed training step (train.py --hip_graph): the device-scalar optimizer entry points are declared and
exported, the CLI offers the flag, and a DP-SGD engine is never captured (no GPU needed)."""
import ctypes
import os
import subprocess
import sys
import warnings

import pytest
import torch

from primia_amd import _lib
from primia_amd import graphed_train

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("primia_sgd_step_dev", "primia_sgd_step_ranges_dev", "primia_conv_sgd_step_many_dev", "primia_adam_step_dev",
       "primia_opt_hyper_set")


def test_device_scalar_entry_points_declared_and_exported():
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in protos, name
        assert hasattr(lib, name), name
    # the hyper array is a device pointer; the host-scalar forms keep their signatures
    assert [n for _, n in protos["primia_sgd_step_dev"][1]] == ["p", "g", "n", "hyper", "stream"]
    assert [n for _, n in protos["primia_sgd_step"][1]] == ["p", "g", "n", "lr", "weight_decay", "stream"]
    assert _lib.lib().primia_abi_version() == 1


def test_hyper_set_refuses_bad_arguments_before_launching():
    # checked on the host: null / misaligned arrays and negative steps never reach a launch
    assert _lib.lib().primia_opt_hyper_set(None, 1e-3, 0.0, 0.9, 0.999, 1e-8, 1, None) == -1
    assert _lib.lib().primia_opt_hyper_set(ctypes.c_void_p(16), 1e-3, 0.0, 0.9, 0.999, 1e-8, -1, None) == -1
    assert _lib.lib().primia_opt_hyper_set(ctypes.c_void_p(20), 1e-3, 0.0, 0.9, 0.999, 1e-8, 1, None) == -1


def test_train_cli_lists_hip_graph():
    r = subprocess.run([sys.executable, "train.py", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--hip_graph" in r.stdout


class _Engine:
    """The parts of ResNet18Engine graphed_step touches, recording the eager calls."""

    def __init__(self, n, dp):
        self.N, self._root, self.training = n, self, True
        self.dp_params = {"max_grad_norm": 1.0, "noise_multiplier": 1.3} if dp else None
        self.fuse_sgd_tail, self.class_weight = True, None
        self.calls = []
        self.loss = torch.zeros(1)

    def sibling(self, n):
        raise AssertionError("same batch size: no sibling")

    def forward(self, x):
        self.calls.append("forward")

    def loss_backward(self, target, soft=False):
        self.calls.append("loss_backward")
        return self.loss


class _Opt:
    kind = "SGD"
    param_groups = [{"lr": 1e-3, "weight_decay": 0.0}]

    def __init__(self, eng):
        self.eng = eng

    def zero_grad(self):
        pass

    def step(self, engine=None, hyper=None):
        assert hyper is None
        self.eng.calls.append("step")


def test_dp_engine_is_not_captured_and_runs_eagerly(monkeypatch):
    monkeypatch.setattr(graphed_train, "_dp_warned", False)
    eng = _Engine(4, dp=True)
    opt = _Opt(eng)
    assert "DP-SGD" in graphed_train.eager_reason(eng, opt, 4)
    x, y = torch.zeros(4, 3, 8, 8), torch.zeros(4, dtype=torch.long)
    with pytest.warns(RuntimeWarning, match="DP-SGD"):
        loss = graphed_train.graphed_step(eng, opt, x, y)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                  # warned once only
        graphed_train.graphed_step(eng, opt, x, y)
    assert loss is eng.loss
    assert eng.calls == ["forward", "loss_backward", "step"] * 2
    assert "_step_graphs" not in eng.__dict__ and "_step_graphs_warm" not in eng.__dict__


def test_which_steps_are_graphed():
    eng = _Engine(8, dp=False)
    opt = _Opt(eng)
    assert graphed_train.eager_reason(eng, opt, 8) is None
    assert graphed_train.eager_reason(eng, opt, 4) is None          # MixUp's half batch
    assert "batch size 5" in graphed_train.eager_reason(eng, opt, 5)
    eng.training = False
    assert graphed_train.eager_reason(eng, opt, 8) is not None
