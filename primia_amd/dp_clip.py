"""DP-SGD's clipping norm C as a device word that follows a quantile of the per-sample gradient norms
(`train.py --dp_clip adaptive`; kernels: csrc/dp_clip.hip; the mechanism and its privacy argument: DESIGN.md section 7).

Quantile-based adaptive clipping (Andrew, Thakkar, McMahan, Ramaswamy, NeurIPS 2021).  Every logical step releases, with
Gaussian noise of standard deviation sigma_b, the number of samples whose gradient norm is at most C (centred: each record
contributes +-1/2), and C moves geometrically towards the norm below which a fraction `quantile` of the samples lie:

    b  = (below - valid / 2 + sigma_b * z0) / B + 1 / 2
    C' = clamp(C * exp(-lr * (b - quantile)), c_min, c_max)

The gradient noise is raised from z * C to z_delta * C with z_delta = (z^-2 - (2 sigma_b)^-2)^(-1/2), so that the joint
release of gradient and count is a Gaussian mechanism with the configured multiplier z: the accountant is given z as
before.  The step that releases b clips with the C it started with; C' takes effect at the next step.

C lives on the device because a captured step (graphed_train) freezes its launch arguments: the clip-factor and noise
kernels read it, the update kernel writes it, and C moving never captures a graph again.  One object serves one model:
the root engine holds it (`engine.dp_clip`) and every sibling() uses the root's.
"""
import math

import torch

from ._lib import call


def z_delta(z, sigma_b):
    """The gradient's noise multiplier that pays for a count released with noise sigma_b under a total multiplier z
    (float64): z_delta^-2 + (2 sigma_b)^-2 == z^-2.  Raises ValueError at and below the bound sigma_b = z / 2, where the
    count alone would use up the whole budget."""
    z, sigma_b = float(z), float(sigma_b)
    if not (z > 0.0 and math.isfinite(z)):
        raise ValueError(f"z_delta: the noise multiplier must be positive and finite, got {z}")
    if not (math.isfinite(sigma_b) and sigma_b > z / 2.0):
        raise ValueError(f"z_delta: the count's noise sigma_b = {sigma_b} must exceed z / 2 = {z / 2.0} (noise multiplier "
                         f"{z}): below that bound no gradient noise can make up for the count's release")
    return (z ** -2 - (2.0 * sigma_b) ** -2) ** -0.5


class AdaptiveClip:
    """`init`: the C of the first step.  `quantile` (gamma): the fraction of per-sample norms C aims to sit above.  `lr`
    (eta): the geometric rate.  `sigma_b`: the count's noise; None = B / 20 (the paper's recommendation), resolved when a
    step's divisor B is known.  `c_min`, `c_max`: the range C is held in."""

    def __init__(self, device, init=1.0, quantile=0.5, lr=0.2, sigma_b=None, c_min=1e-6, c_max=1e6):
        self.device = torch.device(device)
        self.init, self.quantile, self.lr = float(init), float(quantile), float(lr)
        self.sigma_b = None if sigma_b is None else float(sigma_b)
        self.c_min, self.c_max = float(c_min), float(c_max)
        if not 0.0 < self.quantile < 1.0:
            raise ValueError("AdaptiveClip: the quantile lies strictly between 0 and 1")
        if not (self.lr >= 0.0 and math.isfinite(self.lr)):
            raise ValueError("AdaptiveClip: lr is a finite number >= 0")
        if not (0.0 < self.c_min <= self.c_max and math.isfinite(self.c_max)):
            raise ValueError("AdaptiveClip: the range is 0 < c_min <= c_max")
        if not self.c_min <= self.init <= self.c_max:
            raise ValueError("AdaptiveClip: init lies inside [c_min, c_max]")
        if self.sigma_b is not None and not (self.sigma_b > 0.0 and math.isfinite(self.sigma_b)):
            raise ValueError("AdaptiveClip: sigma_b is positive")
        self.updates = 0        # logical steps that moved C (a host count: a graph replay adds what its capture added, graphed_train)
        self._state = None

    # ---- device state ------------------------------------------------------------------------------------------
    def _alloc(self):
        """norm fp32 [1], counts int32 [2], released fp32 [1]: created at first use — before any capture
        (graphed_train), like DeviceNoise.counter."""
        if self._state is None:
            self._state = (torch.full((1,), self.init, dtype=torch.float32, device=self.device),
                           torch.zeros(2, dtype=torch.int32, device=self.device),
                           torch.full((1,), 0.5, dtype=torch.float32, device=self.device))
        return self._state

    @property
    def norm(self):
        return self._alloc()[0]

    @property
    def counts(self):
        """{below, valid} of the step so far.  The raw count is PRIVATE: tests only, never printed or saved."""
        return self._alloc()[1]

    @property
    def released(self):
        """b of the last update: a released value."""
        return self._alloc()[2]

    def tensors(self):
        return list(self._alloc())

    def value(self):
        """C as a host float (synchronises: tests and tools)."""
        return float(self.norm.item())

    def last_released(self):
        """The last released fraction b as a host float (synchronises)."""
        return float(self.released.item())

    # ---- parameters ----------------------------------------------------------------------------------------------
    def sigma_b_for(self, batch):
        """The count's noise on steps whose divisor is `batch`."""
        return self.sigma_b if self.sigma_b is not None else float(batch) / 20.0

    def noise_multiplier(self, z, batch):
        """z_delta for the configured multiplier z on steps whose divisor is `batch` (raises below the bound)."""
        return z_delta(z, self.sigma_b_for(batch))

    def key(self, z, batch):
        """What a captured step freezes of this object: the parameters, never the value of C."""
        return (self.lr, self.quantile, self.sigma_b_for(batch), self.c_min, self.c_max, self.noise_multiplier(z, batch))

    # ---- launches --------------------------------------------------------------------------------------------------
    def factors(self, sq, target, clip, n, overwrite):
        call("primia_dp_clip_factors_dev", sq, target, clip, int(n), self.norm, self.counts, 1 if overwrite else 0)

    def update(self, batch, z0=None, noise=None, block_offset=0):
        """Move C on the counts of the step that just ran.  `z0`: a device float [1] (host-supplied noise); otherwise
        `noise` (a DeviceNoise): element 0 of its block counter + block_offset, the counter left as it is."""
        args = (self.sigma_b_for(batch), 1.0 / float(batch), self.lr, self.quantile, self.c_min, self.c_max, self.released)
        if z0 is not None:
            call("primia_dp_clip_update", self.norm, self.counts, z0, *args)
        else:
            call("primia_dp_clip_update_chacha", *noise.key_words, noise.nonce, noise.counter, int(block_offset), self.norm,
                 self.counts, *args)
        self.updates += 1

    # ---- checkpoints -------------------------------------------------------------------------------------------------
    def state_dict(self):
        """C, the last released fraction, the parameters and the number of updates: functions of released values only."""
        return {"clip_norm": self.value(), "released": self.last_released(), "updates": int(self.updates), "init": self.init,
                "quantile": self.quantile, "lr": self.lr, "sigma_b": self.sigma_b, "c_min": self.c_min, "c_max": self.c_max}

    PARAMETERS = ("init", "quantile", "lr", "sigma_b", "c_min", "c_max")

    def differing_parameters(self, state):
        """{name: (this object's value, the saved one)} of the parameters a saved state holds differently."""
        return {k: (getattr(self, k), state[k]) for k in self.PARAMETERS if k in state and state[k] != getattr(self, k)}

    def load_state_dict(self, state, keep_parameters=False):
        """Takes C, the released fraction and the update count, and the parameters too, so that the object goes on as the
        saved one ran — unless `keep_parameters` (train.py --resume_checkpoint: the command line's parameters, which the run
        has validated and announced, stay; the caller warns about the ones that differ).  The device tensors keep their
        addresses (captured graphs read them)."""
        if not keep_parameters:
            for k in ("init", "quantile", "lr", "c_min", "c_max"):
                setattr(self, k, float(state[k]))
            self.sigma_b = None if state["sigma_b"] is None else float(state["sigma_b"])
        c = float(state["clip_norm"])
        if not self.c_min <= c <= self.c_max:
            raise ValueError(f"AdaptiveClip: the saved C = {c} lies outside [{self.c_min}, {self.c_max}]")
        self.norm.fill_(c)
        self.released.fill_(float(state.get("released", 0.5)))
        self.counts.zero_()
        self.updates = int(state["updates"])
