"""Host: ring_mfma = 2 sends the thin-channel 7 x 7 / 2 convolution to the limb kernels, unsliced; 0 and 1 do not; the Python
layers and inference.py carry the level."""
import os
import subprocess
import sys

import pytest

from primia_amd import _lib
from primia_amd.secure import SecureContext, ring_mfma_level

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEM = (1, 3, 224, 224, 64, 7, 7, 2, 3)      # B, C, H, W, O, R, S, stride, pad


def test_route_follows_the_level():
    route, split = _lib.lib().primia_ring_conv2d_route, _lib.lib().primia_ring_conv2d_split
    try:
        for level, want in ((0, 0), (1, 0), (2, 1)):
            _lib.set_option("ring_mfma", level)
            assert [route(*STEM, jobs) for jobs in (1, 2)] == [want, want], level
        assert [route(1, c, 224, 224, 64, 7, 7, 2, 3, 2) for c in (1, 4, 5)] == [1, 1, 0]
        assert route(1, 64, 56, 56, 64, 3, 3, 1, 1, 2) == 1 and route(1, 64, 56, 56, 128, 1, 1, 2, 0, 1) == 1
        assert route(1, 64, 56, 56, 64, 5, 5, 1, 2, 1) == -3
        assert split(*STEM, 1) == 1 and split(*STEM, 2) == 1
    finally:
        _lib.set_option("ring_mfma", 0)


def test_python_and_the_cli_carry_the_level():
    assert [ring_mfma_level(v) for v in (False, True, 0, 1, 2)] == [0, 1, 0, 1, 2]
    for bad in (3, -1, 2.0, "2", None):
        with pytest.raises(ValueError):
            ring_mfma_level(bad)
    with pytest.raises(ValueError):
        SecureContext(None, 10, 6, ring_mfma=3)      # refused before anything touches a device
    # argparse takes the arguments in order: a level is parsed (or refused, exit status 2) before --help ends the run
    for args, status in ((["--ring_mfma", "2"], 0), (["--ring_mfma", "3"], 2)):
        r = subprocess.run([sys.executable, "inference.py", *args, "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == status, (args, r.stderr)
