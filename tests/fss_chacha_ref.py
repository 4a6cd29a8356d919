"""FSS keys from a ChaCha20 PRG in NumPy: the block function in uint32 arithmetic, H / G by the definition, and
the DIF / DPF on the reference's pieces with the PRG swapped -- tests/fss_wide_ref.py's level step and the oracle's DPF run
unchanged while `chacha_prg()` stands in for oracle.secure_oracle's prg_H / prg_G.  A module of helpers, not of tests."""
import contextlib

import numpy as np

from oracle import secure_oracle as S
from tests import fss_wide_ref as W

U32, U64 = np.uint32, np.uint64
SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
TAG_DIF, TAG_DPF = 0x31464944, 0x31465044      # "DIF1", "DPF1"
QUARTERS = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15), (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))


def chacha20_block(state):
    """state uint32 [16, n] (constants, key 4-11, counter 12-13, nonce 14-15) -> the 16 output words, [16, n]."""
    s = np.asarray(state, U32)
    x = s.copy()
    for _ in range(10):
        for a, b, c, d in QUARTERS:
            for p, q, r, rot in ((a, b, d, 16), (c, d, b, 12), (a, b, d, 8), (c, d, b, 7)):      # p += q; r = rotl(r ^ p, rot)
                x[p] += x[q]
                v = x[r] ^ x[p]
                x[r] = (v << U32(rot)) | (v >> U32(32 - rot))
    return x + s


def prg_buf(seed, tag):
    """seed uint64 [2, n] -> buf uint64 [8, n]: the block of key (lo s0, hi s0, lo s1, hi s1) twice, counter 0, nonce (tag, 0)."""
    seed = np.asarray(seed, U64)
    k = np.stack([seed[0] & U64(0xFFFFFFFF), seed[0] >> U64(32), seed[1] & U64(0xFFFFFFFF), seed[1] >> U64(32)]).astype(U32)
    const = lambda *vs: np.array(vs, U32).reshape(-1, 1).repeat(seed.shape[1], 1)
    blk = chacha20_block(np.concatenate([const(*SIGMA), k, k, const(0, 0, tag, 0)]))
    return blk[0::2].astype(U64) | (blk[1::2].astype(U64) << U64(32))


def _sides(buf, words):
    """[2 sides, 3 rows per 2 words (w & ~1, the next word, w & 1), n]: the oracle's prg_H (words = 4) / prg_G (2) layout."""
    return np.stack([np.concatenate([[buf[j] & ~U64(1), buf[j + 1], buf[j] & U64(1)] for j in range(words * side, words * side + words, 2)])
                     for side in range(2)])


@contextlib.contextmanager
def chacha_prg():
    saved = S.prg_H, S.prg_G
    S.prg_H, S.prg_G = (lambda seed: _sides(prg_buf(seed, TAG_DIF), 4)), (lambda seed: _sides(prg_buf(seed, TAG_DPF), 2))
    try:
        yield
    finally:
        S.prg_H, S.prg_G = saved


def keygen(kind, alpha, s0_pair, bits):
    with chacha_prg():
        if kind == "dif":
            return W._keygen_serial(np.asarray(alpha, U64), np.asarray(s0_pair, U64), bits)
        return S.dpf_keygen(np.asarray(alpha, U64), s0_pair)[1]


def evaluate(kind, b, x, key, bits):
    with chacha_prg():
        return W._eval_serial(b, np.asarray(x), key, bits) if kind == "dif" else S.dpf_eval(b, x, key)


def inputs(bits, n, seed):
    """(alpha, x, s0_pair) of n tests at a width: random pairs, ending in x = 2^bits - 1, 0, alpha - 1, alpha + 1, alpha."""
    rng = np.random.default_rng(seed)
    m = W.width_mask(bits)
    alpha = rng.integers(0, 2 ** 64, size=n, dtype=U64) & m
    x = rng.integers(0, 2 ** 64, size=n, dtype=U64) & m
    edges = np.stack([alpha, (alpha + U64(1)) & m, (alpha - U64(1)) & m, np.zeros(n, U64), np.full(n, m, U64)])
    for j in range(min(n, 5)):      # (one test: x = alpha)
        x[n - 1 - j] = edges[j, n - 1 - j]
    return alpha, x, W.seeds(rng, n)
