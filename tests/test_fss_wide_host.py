"""CPU: the DIF comparison at a width of n bits (tests/fss_wide_ref.py).  At n = 32 the restatement is the
oracle, bit for bit; above it the parties' outputs add up to [(d + alpha) mod 2^n <= alpha], which Python ints compute, and to
[d <= 0] on every pair that does not wrap.  And the host arithmetic of the wider keys."""
import numpy as np
import pytest

from oracle import secure_oracle as S
from primia_amd import resnet_spec
from primia_amd.secure import (DIF_KEY_BYTES, architecture_of, check_fss_bits, image_requests, primitive_bytes,
                               serving_bytes)
from tests import fss_wide_ref as W
from tests.fss_wide_ref import CRAFTED_D, as_i64, crafted_pairs, seeds, shares_of

U64, I64 = np.uint64, np.int64


# ---- 1. n = 32 is the oracle ----------------------------------------------------------------------------------------------
def test_width_32_is_the_oracle_bit_for_bit():
    """64 random elements and the edge cases x = alpha, alpha + 1, alpha - 1 and a wrap past 2^32: split, open, every key
    field, both parties' evaluations and fss_le equal the oracle's."""
    rng = np.random.default_rng(8)
    alpha = np.concatenate([rng.integers(0, 2 ** 32, size=64, dtype=U64), np.array([7, 7, 7, 2 ** 32 - 1, 0, 5], U64)])
    d = np.concatenate([rng.integers(-2 ** 20, 2 ** 20, size=64), np.array([0, 1, -1, 1, -1, 2 ** 32 - 3])]).astype(I64)
    n = alpha.size
    r = rng.integers(0, 2 ** 64, size=n, dtype=U64)
    s0 = seeds(rng, n)
    a_w, a_o = W.split_alpha(alpha, r, 32), S.split_alpha(alpha, r)
    assert all(np.array_equal(a_w[j], a_o[j]) for j in range(2))
    _, k_o = S._dif_keygen_serial(alpha, s0)
    k_w = W.dif_keygen(alpha, s0, 32)
    for b in range(2):
        assert k_w[b].keys() == k_o[b].keys()
        for name in k_o[b]:
            assert k_w[b][name].dtype == k_o[b][name].dtype and np.array_equal(k_w[b][name], k_o[b][name]), name
    x1, x2 = shares_of(rng, d), shares_of(rng, np.zeros(n, I64))
    rm = [S.fss_mask(x1[j], x2[j], a_o[j]) for j in range(2)]
    masked = S.fss_open(rm[0], rm[1])
    assert np.array_equal(W.fss_open(rm[0], rm[1], 32), masked)
    assert np.array_equal(masked[64:67], np.array([7, 8, 6], U64))                    # x = alpha, alpha + 1, alpha - 1
    for b in range(2):
        assert np.array_equal(W.dif_eval(b, masked, k_w[b], 32), S._dif_eval_serial(b, masked, k_o[b]))
    le_w, le_o = W.fss_le(x1, x2, a_w, k_w, 32), S.fss_le(x1, x2, a_o, k_o)
    assert all(np.array_equal(le_w[j], le_o[j]) for j in range(2))
    bit = S.radd(le_w[0], le_w[1])
    assert bit[64:70].tolist() == [1, 0, 1, 1, 0, 1]      # the wraps: 2^32 - 1 + 1 -> 0 <= alpha; 0 - 1 -> 2^32 - 1 > 0; 5 + 2^32 - 3 -> 2


# ---- 2. the definition above 32 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 40, 64])
def test_reconstructed_bit_is_the_definition(n):
    """Random alpha against every crafted d, and the crafted alpha: the two outputs add up to [(d + alpha) mod 2^n <= alpha];
    wherever alpha + d stays in [0, 2^n) that is [d <= 0].  At 64 the pairs that wrap are exactly the crafted ones."""
    rng = np.random.default_rng(n)
    pairs = crafted_pairs(n)
    fits = [d for d in CRAFTED_D if abs(d) < 2 ** (n - 1)]
    assert len(fits) == {33: 7, 40: 9, 64: 11}[n]
    for _ in range(200 // len(fits) + 1):
        pairs += [(int(rng.integers(0, 2 ** 64, dtype=U64)) % 2 ** n, d) for d in fits]
    alpha = np.array([a for a, _ in pairs], dtype=U64)
    d = as_i64([q for _, q in pairs])
    N = alpha.size
    r = rng.integers(0, 2 ** 64, size=N, dtype=U64)
    a_sh = W.split_alpha(alpha, r, n)
    assert np.array_equal((a_sh[0] + a_sh[1]) & W.width_mask(n), alpha) and int(max(a_sh[0].max(), a_sh[1].max())) < 2 ** n
    keys = W.dif_keygen(alpha, seeds(rng, N), n)
    assert keys[0]["bits"].shape == (n, 4, N) and keys[0]["cw_sigma"].shape == keys[0]["cw_s"].shape == (n, 2, N)
    assert keys[0]["cw_leaf"].shape == (n + 1, N) and keys[0]["cw_leaf"].dtype == np.int32
    out = W.fss_le(shares_of(rng, d), shares_of(rng, np.zeros(N, I64)), a_sh, keys, n)
    bit = S.radd(out[0], out[1])
    want = np.array([W.defined_bit(a, q, n) for a, q in pairs], I64)
    assert np.array_equal(bit, want)
    n_crafted = len(crafted_pairs(n))
    wrapped = [i for i, (a, q) in enumerate(pairs) if W.wraps(a, q, n)]
    calm = [i for i in range(N) if i not in set(wrapped)]
    assert all(bit[i] == int(pairs[i][1] <= 0) for i in calm)
    assert {n_crafted - 2, n_crafted - 1} <= set(wrapped) and len(calm) + len(wrapped) == N and len(calm) > N // 2
    if n == 64:
        # every wrap is a crafted one (a random 64-bit alpha is not within 2^40 of either end: probability 2^-22 per draw, fixed
        # seed): alpha = 0 with the four negative d, alpha = 1 with the three below -1, alpha = 2^64 - 1 with the six positive d,
        # and the two crafted pairs
        assert max(wrapped) < n_crafted and len(wrapped) == 4 + 3 + 6 + 2
        assert len(calm) == N - 15 >= 200


# ---- 3. what the width buys -----------------------------------------------------------------------------------------------
def test_a_difference_of_2_pow_32_is_positive_at_64_bits_and_zero_at_32():
    """d = 2^32 under any alpha: 32 bits see d = 0 and answer 1; 64 bits answer 0 (no alpha drawn here is within 2^32 of
    2^64)."""
    rng = np.random.default_rng(3)
    N = 24
    raw = rng.integers(0, 2 ** 64 - 2 ** 33, size=N, dtype=U64)
    d = as_i64([2 ** 32] * N)
    x1, x2 = shares_of(rng, d), shares_of(rng, np.zeros(N, I64))
    r, s0 = rng.integers(0, 2 ** 64, size=N, dtype=U64), seeds(rng, N)
    for n, answer in ((32, 1), (64, 0)):
        alpha = raw & W.width_mask(n)
        out = W.fss_le(x1, x2, W.split_alpha(alpha, r, n), W.dif_keygen(alpha, s0, n), n)
        assert S.radd(out[0], out[1]).tolist() == [answer] * N


# ---- 4. host arithmetic ---------------------------------------------------------------------------------------------------
def test_key_bytes_and_request_lists():
    assert DIF_KEY_BYTES == 1244 and DIF_KEY_BYTES(32) == 1244 and DIF_KEY_BYTES(64) == 2428 and DIF_KEY_BYTES(40) == 60 + 37 * 40
    for bad in (31, 65, 0):
        with pytest.raises(ValueError):
            check_fss_bits(bad)
        with pytest.raises(ValueError):
            DIF_KEY_BYTES(bad)
    arch = architecture_of(resnet_spec.init_state_dict(resnet_spec.resnet18_spec(3, 3, 224, "max")))
    req = image_requests(arch, 224, 1)      # the request list does not know the width: the same at every one
    comparisons = sum(args[0] for kind, args, _ in req if kind == "dif_keys")
    assert comparisons == 3_311_616
    b32, b64 = primitive_bytes(req), primitive_bytes(req, 64)
    assert primitive_bytes(req, 32) == b32 and b64 - b32 == comparisons * (2428 - 1244)
    assert primitive_bytes(req, 40) - b32 == comparisons * 37 * 8
    s64 = serving_bytes(arch, 224, 1, fss_bits=64)
    assert s64 == b64 + b64 // 8 and serving_bytes(arch, 224, 1) == b32 + b32 // 8
