"""CPU: the option ring_mfma exists and is off by default; inference.py has the flag."""
import os
import subprocess
import sys

from primia_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_defaults_to_off_and_the_flag_exists():
    _lib.lib().primia_reset_options()
    assert _lib.get_option("ring_mfma") == 0
    r = subprocess.run([sys.executable, "inference.py", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--ring_mfma" in r.stdout
