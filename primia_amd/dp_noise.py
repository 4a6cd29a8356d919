"""DP-SGD's Gaussian noise from a ChaCha20 keystream on the device (`primia_dp_noise_add`, csrc/dp_noise.hip).

The Gaussian mechanism's guarantee rests on its noise being unpredictable, so the key comes from the operating system's
entropy pool — never from the command line's seed, as torch.randn's Philox state does.  The block counter is a DEVICE
word: a captured training step (graphed_train) reads it in the noise node and advances it in the next node, so every
replay draws fresh noise.  One object serves one model: the root engine holds it and every sibling() uses the root's,
because two steps that reuse keystream under one key would void the guarantee."""
import hashlib
import os

import torch

from ._lib import call, query


class DeviceNoise:
    """`key`: 32 bytes (None: os.urandom).  `nonce`: 64-bit stream selector (train.py: the client index).  `debug_seed`:
    derive the key from SHA-256 of the seed and the nonce instead — reproducible, therefore predictable: tests only."""

    def __init__(self, device, key=None, nonce=0, debug_seed=None):
        self.device = torch.device(device)
        self.nonce = int(nonce) & (2 ** 64 - 1)
        self.predictable = debug_seed is not None
        if debug_seed is not None:
            if key is not None:
                raise ValueError("DeviceNoise: give a key or a debug seed, not both")
            key = hashlib.sha256(b"primia dp noise" + (int(debug_seed) & (2 ** 64 - 1)).to_bytes(8, "little")
                                 + self.nonce.to_bytes(8, "little")).digest()
        elif key is None:
            key = os.urandom(32)
        key = bytes(key)
        if len(key) != 32:
            raise ValueError("DeviceNoise: the key is 32 bytes")
        self.key = key
        self.key_words = tuple(int.from_bytes(key[8 * i:8 * i + 8], "little") for i in range(4))
        self._counter = None

    @property
    def counter(self):
        """The block counter: one int64 word on the device (the bits of the kernel's uint64), created at first use."""
        if self._counter is None:
            self._counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        return self._counter

    def blocks_drawn(self):
        """The counter's value (synchronises: tests and tools)."""
        return int(self.counter.item()) & (2 ** 64 - 1)

    def add_to(self, g, n, sigma, inv_batch, acc=None):
        """g[:n] = (g[:n] + sigma * z) * inv_batch with z the next ceil(n / 16) blocks of the stream; two launches on the
        current stream, both capturable.  `acc` (fp32, read only: the clipped sums of a step's earlier micro-batch
        passes) is added to g first, in the same kernel."""
        ctr = self.counter
        if acc is None:
            call("primia_dp_noise_add", *self.key_words, self.nonce, ctr, 0, g, int(n), float(sigma), float(inv_batch))
        else:
            call("primia_dp_noise_add_acc", *self.key_words, self.nonce, ctr, 0, g, acc, int(n), float(sigma),
                 float(inv_batch))
        call("primia_u64_add", ctr, query("primia_dp_noise_blocks", int(n)))
