"""Host: FSS keys from the ChaCha20 PRG before anything touches a GPU -- the yardstick's block function against
RFC 8439, tests/fss_chacha_ref.py against the plain comparison, the `*_prg` entry points' refusals, the option by name."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from primia_amd import _lib
from primia_amd.secure import ProtocolForm
from tests import fss_chacha_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("dif", 32), ("dif", 33), ("dif", 64), ("dpf", 32)]


def test_reference_block_is_rfc_8439():
    """RFC 8439 §2.3.2: key 00..1f, block counter 1, nonce 00:00:00:09 00:00:00:4a 00:00:00:00 -- in chacha_block.h's layout the
    counter's high word (13) carries the nonce's first word."""
    state = np.array([*R.SIGMA, *np.frombuffer(bytes(range(32)), "<u4"), 1, 0x09000000, 0x4A000000, 0], np.uint32).reshape(16, 1)
    want = [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3, 0xC7F4D1C7, 0x0368C033, 0x9AAA2204, 0x4E6CD4C3,
            0x466482D2, 0x09AA9F07, 0x05D7C214, 0xA2028BD9, 0xD19C12B5, 0xB94E16DE, 0xE883D0CB, 0x4E3C50A2]
    assert R.chacha20_block(state)[:, 0].tolist() == want and R.TAG_DIF != R.TAG_DPF


@pytest.mark.parametrize("kind,bits", CASES)
def test_reference_reconstructs_the_plain_comparison(kind, bits):
    alpha, x, s0 = R.inputs(bits, 300, bits)
    keys = R.keygen(kind, alpha, s0, bits)
    out = [R.evaluate(kind, b, x, keys[b], bits) for b in range(2)]
    want = (x <= alpha) if kind == "dif" else (x == alpha)
    assert want[-1] and not want[-2] and x[-4] == 0 and x[-5] == 2 ** bits - 1      # x = alpha, alpha + 1, ..., 0, 2^bits - 1
    assert np.array_equal(out[0] + out[1], want.astype(np.int64))


@pytest.mark.parametrize("name", [f"primia_{kind}_{what}_prg" for kind in ("dif", "dpf") for what in ("keygen", "eval", "eval_local")])
def test_entry_point_is_declared_and_refuses_bad_arguments(name):
    protos, fn = _lib.protos(), getattr(_lib.lib(), name)
    buf = ctypes.create_string_buffer(64)
    p, q = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(ctypes.addressof(buf) + 8)      # never dereferenced
    params = protos[name][1][:-1]
    names = [a for _, a in params]
    assert protos[name][0] is ctypes.c_int and protos[name][1][-1][1] == "stream" and names[-1] == "prg"
    assert (names[-2] == "bits") == ("dif" in name)
    # a valid call: every pointer non-null (the two outputs of a local form distinct), 4 elements, 64 bits, prg set below
    valid = [(q if a == "out1" else p) if t is ctypes.c_void_p else {"n": 4, "bits": 64, "w1": 1, "w2": 1, "len": 1}.get(a, 0)
             for t, a in params]
    refused = lambda **change: fn(*[change.get(a, v) for a, v in zip(names, valid)], None) == -1
    assert refused(prg=2) and refused(prg=-1)
    for prg in (0, 1):
        assert all(refused(prg=prg, **{a: None}) for t, a in params
                   if t is ctypes.c_void_p and not (a.startswith("x1_") and name == "primia_dif_eval_local_prg")), prg
        assert "dif" not in name or (refused(prg=prg, bits=31) and refused(prg=prg, bits=65))


def test_fss_prg_is_refused_by_name():
    with pytest.raises(ValueError, match="'sha' / 'chacha'.*'aes'"):
        ProtocolForm(fss_prg="aes")
    assert ProtocolForm() == ProtocolForm(fss_prg="sha") != ProtocolForm(fss_prg="chacha") and ProtocolForm().fss_prg == "sha"
    r = subprocess.run([sys.executable, "inference.py", "--model_weights", "none.pt", "--encrypted_inference", "--fss_prg", "aes"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--fss_prg" in r.stderr and "'sha'" in r.stderr and "'chacha'" in r.stderr
