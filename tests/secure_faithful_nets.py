"""The definition of the faithful truncation of a shared product (the reference has none: each party divides its own share,
which is off by 2^64 / d whenever the signed shares wrap), oracle contexts whose product sites use it, its restatement on
Python integers, shares built to wrap, and the network of the accuracy case, shared by tests/test_secure_faithful_host.py
and tests/test_gpu_secure_faithful.py: a module of helpers, not of tests.  Everything is composed from
oracle.secure_oracle's own functions; nothing under oracle/ knows about it."""
import numpy as np
import torch

from oracle import secure_oracle as S
from tests import fss_wide_ref as W
from tests.secure_folded_nets import wide_resnet18

I64, U64 = np.int64, np.uint64
M64 = (1 << 64) - 1
# The stated bound: out = floor(z / d) + e with e in ERR, for every mask, while |z| < 2^62.
ERR = (-1, 0, 1, 2)
DIVISORS = (10 ** 3, 10 ** 6, 20, 49)
# masks every test of the definition includes (party 0's share of z)
EDGE_MASKS = (0, 2 ** 62, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 2 ** 62 - 1, 2 ** 64 - 2 ** 62 + 1, 2 ** 64 - 1)


def oracle_trunc_faithful(ctx, z, d):
    """THE definition of SecureContext.trunc_faithful on an OracleContext: shares z of a value |z| < 2^62 ->
    shares of floor(z / d) + e, e in ERR.  One triple ("mul", shape, shape): the carry product m_0 * m_1 with the first
    operand shared as [m_0, 0] and the second as [0, m_1], through the context's own beaver_mul (no truncation)."""
    d = int(d)
    assert 0 < d < 2 ** 62
    u = [S.radd(z[0], I64(2 ** 62)), np.asarray(z[1], I64)]
    m = [(u[j].view(U64) >> U64(63)).view(I64) for j in range(2)]
    zero = np.zeros_like(m[0])
    p = ctx.beaver_mul([m[0], zero], [zero, m[1]])
    w = ctx.sub(m, p)
    q64, q62 = (2 ** 64 // d) & M64, 2 ** 62 // d
    out = []
    for j in range(2):
        q = (u[j].view(U64) // U64(d)).view(I64)
        q = S.rsub(q, S.rmul(w[j], np.array(q64, dtype=U64).view(I64)))
        out.append(S.rsub(q, I64(q62)) if j == 0 else q)
    return out


def int_trunc_faithful(z0, z1, d, a0, a1, b0, b1, c0):
    """The definition once more on Python integers mod 2^64, one element: (out_0, out_1) from the shares (z0, z1) and the
    carry triple's shares (a0, a1, b0, b1, c0; c1 completes c = a * b)."""
    c1 = (((a0 + a1) * (b0 + b1)) - c0) & M64
    u0, u1 = (z0 + 2 ** 62) & M64, z1 & M64
    m0, m1 = u0 >> 63, u1 >> 63
    delta, eps = (m0 - a0 - a1) & M64, (m1 - b0 - b1) & M64
    p0 = (delta * b0 + a0 * eps + c0 + delta * eps) & M64
    p1 = (delta * b1 + a1 * eps + c1) & M64
    q64, q62 = 2 ** 64 // d, 2 ** 62 // d
    return (u0 // d - (m0 - p0) * q64 - q62) & M64, (u1 // d - (m1 - p1) * q64) & M64


def signed(v):
    v &= M64
    return v - 2 ** 64 if v >= 2 ** 63 else v


def int_trunc_reference(z0, z1, d):
    """The reference's form on Python integers: each party divides its own signed share toward zero."""
    t = lambda v: abs(signed(v)) // d * (1 if signed(v) >= 0 else -1)
    return signed(t(z0) + t(z1))


def wrapping_pair(z, rng):
    """int64 shares (z0, z1) of the int64 values z, |z| >= 4, whose SIGNED sum wraps: both shares have the sign of -z and
    magnitudes near 2^63 -- z0 = -2^63 + r for z > 0 and 2^63 - 1 - r for z < 0, r uniform in [0, |z| / 2] -- so that the
    integer sum of the signed shares is z -+ 2^64 and the per-share quotients sum to z / d -+ 2^64 / d."""
    z = np.asarray(z, I64)
    assert (np.abs(z) >= 4).all()
    r = rng.integers(0, np.abs(z) // 2, dtype=I64, endpoint=True)
    z0 = np.where(z > 0, np.iinfo(I64).min + r, np.iinfo(I64).max - r).astype(I64)
    return z0, S.rsub(z, z0)


class FaithfulProducts:
    """Mixin for an OracleContext: the products at scale s^2 that a folded forward truncates -- fpt_mul (oracle_affine_eval's)
    and fpt_matmul (conv2d's and linear's) -- are truncated by oracle_trunc_faithful; relu, the pools and everything else are
    the context's own."""

    def fpt_mul(self, x, y):
        return oracle_trunc_faithful(self, self.beaver_mul(x, y), self.scale)

    def fpt_matmul(self, x, y):
        t = self.dealer.triple("matmul", x[0].shape, y[0].shape)
        return oracle_trunc_faithful(self, S.beaver("matmul", x, y, t), self.scale)


class FaithfulOracleContext(FaithfulProducts, S.OracleContext):
    pass


class FaithfulWideOracleContext(FaithfulProducts, W.WideOracleContext):
    pass


# ---- the accuracy case ------------------------------------------------------------------------------------------------------
# tests/secure_folded_nets.py's wide-variance 8-block network at 32 x 32 (seed 720) and its two images (seed 721), the images
# and conv1 each scaled by 50: the folded norms are fixed affine maps, so every activation behind conv1 grows about 2,500
# times (logits of 1,400 to 3,200) and at pf = 6 primia_amd.secure.expected_wraps reports 30.7 expected wraps of the
# reference's per-share form over the one pass and a largest |z| of 0.025 * 2^62 (the tests assert >= 20 and < 1/2).
WRAP_IMAGE_SCALE = 50.0
WRAP_CONV1_SCALE = 50.0


def wrap_case():
    sd = dict(wide_resnet18(32, 720))
    sd["conv1.weight"] = sd["conv1.weight"] * WRAP_CONV1_SCALE
    images = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(721)) * WRAP_IMAGE_SCALE
    return sd, images


# Bound of the accuracy test: TWICE the largest max |faithful secure logits - float64 plaintext logits| that the CPU
# composition (oracle_folded_forward on FaithfulWideOracleContext over WideChaChaDealer, the host dealer with 64-bit
# comparison keys) measured on wrap_case at pf = 6 under dealer seeds 1, 2, 3 -- `python -m tests.secure_faithful_nets` prints
# them.  The logits are 1,400 to 3,200, so the bound is about 2e-5 of a logit.  The three differ in the fifth digit only: the
# error is not the truncations' (two units of 1e-6 each) but the 1e-6 rounding of the folded scales, which the plaintext
# reference keeps in float32, times activations in the thousands -- the same for every mask.
FAITHFUL_TOL_MEASURED = (0.031218734703088558, 0.031232734703280585, 0.031242734703027963)
FAITHFUL_TOL = 2 * max(FAITHFUL_TOL_MEASURED)


def measure_faithful_error(seeds=(1, 2, 3), workers=16):
    """max |secure - float64 plaintext| of the composed faithful forward on wrap_case, per dealer seed (minutes on a CPU)."""
    import multiprocessing as mp

    from primia_amd.secure import fold_batch_norm
    from tests.secure_batch_nets import numpy_sd
    from tests.secure_folded_nets import WideChaChaDealer, oracle_folded_forward, plaintext_logits

    sd, images = wrap_case()
    plain = plaintext_logits(sd, images, 6, 32)
    folded = numpy_sd(fold_batch_norm(sd))
    errs = []
    with mp.get_context("spawn").Pool(workers) as pool:
        S.use_pool(pool, n_slices=2 * workers)
        try:
            for seed in seeds:
                ctx = FaithfulWideOracleContext(WideChaChaDealer(seed, 64), 10, 6, 64)
                out = oracle_folded_forward(ctx, folded, images.numpy())
                dec = S.radd(out[0], out[1]).astype(np.float64) / 10 ** 6
                errs.append(float(np.abs(dec - plain).max()))
                print("faithful, wrap_case, pf = 6, dealer seed", seed, ": max |error|", errs[-1], "logits", dec.tolist(), flush=True)
        finally:
            S.use_pool(None)
    return errs


if __name__ == "__main__":
    measure_faithful_error()
