"""The float64 form of the DP-SGD noise definition (include/primia_hip.h, primia_dp_noise_add) on the CPU.

Element i lives in ChaCha20 block B = block0 + i / 16; 64-bit keystream word 8B + p (p = (i % 16) / 2) as
tests.cpu_standins.chacha20_words lays it out has a = its low half and c = its high half;
u1 = ((a >> 8) + 1) * 2^-24, u2 = (c >> 8) * 2^-24, r = sqrt(-2 ln u1); even i: r cos(2 pi u2), odd i: r sin(2 pi u2)."""
import numpy as np

from tests.cpu_standins import chacha20_words

KEY = (0x0706050403020100, 0x0f0e0d0c0b0a0908, 0x1716151413121110, 0x1f1e1d1c1b1a1918)
NONCE = 0x4a00000000
TAIL = 5.77          # sqrt(48 ln 2) = 5.768...: where 24-bit uniforms truncate the Gaussian


def noise_blocks(n):
    return (n + 15) // 16


def reference_noise(key, nonce, block0, n):
    """float64 [n]: z of the definition for elements 0..n-1 of a call whose first block is `block0`."""
    if n == 0:
        return np.zeros(0)
    words = chacha20_words(tuple(key) + (nonce,), block0, 8 * noise_blocks(n))
    a = (words & np.uint64(0xFFFFFFFF)).astype(np.int64)
    c = (words >> np.uint64(32)).astype(np.int64)
    u1 = ((a >> 8) + 1).astype(np.float64) * 2.0 ** -24
    u2 = (c >> 8).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.empty(2 * words.size)
    z[0::2] = r * np.cos(2.0 * np.pi * u2)
    z[1::2] = r * np.sin(2.0 * np.pi * u2)
    return z[:n]
