"""The float64 form of DP-SGD's adaptive clipping norm (include/primia_hip.h: primia_dp_clip_factors_dev,
primia_dp_clip_update) on the CPU.

    below = #{valid n : sq_n <= C * C},  valid = #{n : target_n >= 0}  (every n without targets)
    s  = (below - valid / 2) + sigma_b * z0
    b  = s * inv_batch + 1 / 2
    C' = clamp(C * exp(-eta * (b - gamma)), c_min, c_max), rounded once to float32

Every float the C ABI takes as a float32 is rounded to float32 FIRST (f32 below): the reference sees the parameters the
kernel sees, so what is left between the two is the device's exp against NumPy's in the last bits of a double, and the one
rounding to float32 — at most one float32 unit in the last place, 2^-23 relative."""
import numpy as np

ULP = 2.0 ** -23        # the bound the device's C' and released fraction are held to, relative


def f32(v):
    """The double a float32 argument of the C ABI carries."""
    return float(np.float32(v))


def z_delta(z, sigma_b):
    """The gradient's noise multiplier: z_delta^-2 + (2 sigma_b)^-2 = z^-2; no such number at or below sigma_b = z / 2."""
    z, sigma_b = float(z), float(sigma_b)
    if not sigma_b > z / 2.0:
        raise ValueError("sigma_b must exceed z / 2")
    return 1.0 / np.sqrt(1.0 / (z * z) - 1.0 / (4.0 * sigma_b * sigma_b))


def counts(sq, target, C):
    """(below, valid) for float64 squared norms sq, int targets (None: unmasked) and the float32 value C."""
    sq = np.asarray(sq, dtype=np.float64)
    ok = np.ones(sq.shape, dtype=bool) if target is None else np.asarray(target) >= 0
    c = f32(C)
    return int((ok & (sq <= c * c)).sum()), int(ok.sum())


def released(below, valid, z0, sigma_b, inv_batch):
    """b, the noisy fraction of norms at or below C (float64)."""
    s = (float(below) - 0.5 * float(valid)) + f32(sigma_b) * f32(z0)
    return s * f32(inv_batch) + 0.5


def update(C, below, valid, z0, sigma_b, inv_batch, eta, gamma, c_min, c_max):
    """C' as a float64 BEFORE the rounding to float32 (compare with |got - want| <= ULP * want), inside the range."""
    b = released(below, valid, z0, sigma_b, inv_batch)
    c = f32(C) * np.exp(-f32(eta) * (b - f32(gamma)))
    return float(min(max(c, f32(c_min)), f32(c_max)))
