"""CPU checks of DP-SGD on the BatchNorm network with frozen statistics (ResNet18Engine(norm="frozen"), train.py --dp_norm):
the state dict is the BatchNorm network's, the library exports the new entry points with prototypes _lib parses, the CLI
offers the flag, and a frozen engine's step graph has a key of its own (no GPU needed)."""
import ctypes
import importlib.util
import os

import pytest

from primia_amd import _lib, graphed_train, resnet_spec as rs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

BWD_TAIL = ["ps_dgamma", "ps_dbeta", "N", "HW", "C"]
WS_TAIL = ["workspace", "workspace_bytes", "dtype", "stream"]
STATS = ["gamma", "running_mean", "running_var", "eps"]


def test_frozen_state_dict_is_the_batchnorm_one():
    for pooling in ("max", "avg"):
        spec = rs.resnet18_spec(3, 3, 64, pooling)
        assert rs.state_dict_keys(spec, "frozen") == rs.state_dict_keys(spec, "batch")
        assert len(rs.state_dict_keys(spec, "frozen")) == 122
        assert rs.buffer_entries(spec, "frozen") == rs.buffer_entries(spec, "batch") != []
        assert rs.buffer_entries(spec, "group") == []
    a, b = rs.init_state_dict(spec, "frozen"), rs.init_state_dict(spec, "batch")
    assert list(a) == list(b) and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)


def test_entry_points_declared_and_exported():
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = lambda f: [n for _, n in protos[f][1]]
    for f in ("primia_bn_frozen_bwd", "primia_bn_frozen_bwd_mask", "primia_bn_frozen_relu_bwd", "primia_bn_fwd_eval_mask",
              "primia_bn_frozen_workspace_bytes"):
        assert f in protos, f
        assert hasattr(lib, f), f
    assert names("primia_bn_frozen_bwd") == ["y", "z", "dz", "dy", "g_out"] + STATS + BWD_TAIL + ["relu"] + WS_TAIL
    assert names("primia_bn_frozen_bwd_mask") == ["y", "relu_mask", "dz", "dy", "g_out"] + STATS + BWD_TAIL + WS_TAIL
    assert names("primia_bn_frozen_relu_bwd") == (["y", "dz", "dy", "gamma", "beta", "running_mean", "running_var", "eps"]
                                                  + BWD_TAIL + WS_TAIL)
    assert names("primia_bn_fwd_eval_mask") == ["y", "residual", "z", "relu_mask", "gamma", "beta", "running_mean",
                                                "running_var", "M", "C", "eps", "dtype", "stream"]
    assert names("primia_bn_frozen_workspace_bytes") == ["N", "HW", "C"]
    assert protos["primia_bn_frozen_workspace_bytes"][0] is ctypes.c_int64
    assert [t for t, n in protos["primia_bn_frozen_bwd"][1] if n == "eps"] == [ctypes.c_float]
    assert _lib.lib().primia_abi_version() == 1            # additions only


def test_workspace_query():
    """Per-slab partials [N][slabs][2][C] floats: at least one slab per sample, never more than 32; nothing for nonsense."""
    q = lambda *a: _lib.query("primia_bn_frozen_workspace_bytes", *a)
    for N, HW, C in ((5, 1, 512), (4, 16, 64), (3, 36, 128), (130, 25, 256), (256, 12544, 64), (8, 49, 512)):
        b = q(N, HW, C)
        assert b % (N * 2 * C * 4) == 0 and 1 <= b // (N * 2 * C * 4) <= min(32, HW), (N, HW, C, b)
    assert q(5, 1, 512) == 5 * 2 * 512 * 4 and q(4, 16, 64) == 4 * 2 * 64 * 4          # one slab: the sample is small
    assert q(3, 36, 128) > 3 * 2 * 128 * 4                                             # several
    assert q(0, 36, 128) == 0 and q(3, 0, 128) == 0 and q(3, 36, 0) == 0


def test_backward_refuses_null_pointers_on_the_host():
    """Checked before anything is launched (no GPU here): every null operand is PRIMIA_ERR_ARG (-1)."""
    f = _lib.lib().primia_bn_frozen_bwd
    p = ctypes.c_void_p(4096)
    ok = [p, p, p, p, None, p, p, p, 1e-5, p, p, 3, 36, 128, 1, p, 1 << 20, _lib.PRIMIA_BF16, None]
    for i in (0, 1, 2, 3, 5, 6, 7, 9, 10, 15):
        args = list(ok)
        args[i] = None
        assert f(*args) == -1, i
    for i, v in ((11, 0), (12, 0), (13, 12), (13, 1024), (17, 7)):
        args = list(ok)
        args[i] = v
        assert f(*args) == -1, (i, v)
    short = list(ok)
    short[16] = _lib.query("primia_bn_frozen_workspace_bytes", 3, 36, 128) - 1
    assert f(*short) == -4          # PRIMIA_ERR_WORKSPACE: no silent fallback


def _train_module():
    spec = importlib.util.spec_from_file_location("primia_train_cli", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_cli_dp_norm(capsys):
    parser = _train_module().build_parser()
    assert parser.parse_args(["--config", "x.ini"]).dp_norm == "group"
    assert parser.parse_args(["--config", "x.ini", "--dp_norm", "frozen"]).dp_norm == "frozen"
    assert parser.parse_args(["--config", "x.ini", "--dp_norm", "group"]).dp_norm == "group"
    for bad in ("batch", "layer", ""):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(["--config", "x.ini", "--dp_norm", bad])
        assert e.value.code == 2
    assert "--dp_norm" in capsys.readouterr().err
    assert "--dp_norm" in parser.format_help()


class _Engine:
    """What graphed_train._key reads of an engine."""

    fuse_sgd_tail, class_weight, dp_params, N = False, None, None, 8

    def __init__(self, norm):
        self.norm, self._root = norm, self


class _Opt:
    kind = "SGD"


def test_step_graph_key_tells_frozen_from_group():
    keys = {n: graphed_train._key(_Engine(n), _Opt(), False) for n in ("batch", "group", "frozen")}
    assert keys["frozen"] != keys["group"] and keys["frozen"] != keys["batch"]
    assert keys["group"] == keys["batch"] == (8, False, "SGD", False, False)      # as before
