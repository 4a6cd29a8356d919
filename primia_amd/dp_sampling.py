"""Poisson-sampled batches for DP-SGD (`train.py --dp_sampling poisson`; kernels: csrc/dp_sample.hip).

The privacy bound the accountant reports (dp_accountant) is that of the SAMPLED Gaussian mechanism: at every step each
record joins the batch independently with probability q, by a draw an observer cannot predict.  A shuffled loader seeded
from the command line is neither.  Here record i reads one 64-bit word of a ChaCha20 keystream and joins iff
word < threshold = floor(q * 2^64); the key comes from the operating system's entropy pool and the block counter is a
device word, exactly as for the noise (dp_noise.DeviceNoise) — under a key of its OWN: the two streams must be
independent.

A Poisson batch changes size at every step; the engine's buffers and a captured step do not.  Every batch therefore
has `capacity` slots (K * ceil(capacity / K) with `micro_batches=K`: a step run as K passes of an engine that size,
dp_micro): the selected records in ascending order, then padding (a zero image, target -1) which the masked
loss and clip kernels of ResNet18Engine.dp_loss_backward(expected_batch=L) turn into exactly nothing.  Select, counter
advance and gather are three launches on the current stream without a host synchronisation, into ONE reused buffer
pair whose addresses a replayed graph (graphed_train) reads as its static input.
"""
import hashlib
import os

import torch

from . import dp_accountant
from ._lib import call, dtype_code, query


class DeviceSampler:
    """The selection stream of one client.  `key`: 32 bytes (None: os.urandom).  `nonce`: 64-bit stream selector
    (train.py: the client index).  `debug_seed`: derive the key from SHA-256 of a label of its own, the seed and the
    nonce — reproducible, therefore predictable: tests only."""

    def __init__(self, device, key=None, nonce=0, debug_seed=None):
        self.device = torch.device(device)
        self.nonce = int(nonce) & (2 ** 64 - 1)
        self.predictable = debug_seed is not None
        if debug_seed is not None:
            if key is not None:
                raise ValueError("DeviceSampler: give a key or a debug seed, not both")
            key = hashlib.sha256(b"primia dp sampler" + (int(debug_seed) & (2 ** 64 - 1)).to_bytes(8, "little")
                                 + self.nonce.to_bytes(8, "little")).digest()
        elif key is None:
            key = os.urandom(32)
        key = bytes(key)
        if len(key) != 32:
            raise ValueError("DeviceSampler: the key is 32 bytes")
        self.key = key
        self.key_words = tuple(int.from_bytes(key[8 * i:8 * i + 8], "little") for i in range(4))
        self._state = None

    @property
    def state(self):
        """[block counter, overflow events]: two int64 words on the device (the bits of the kernel's uint64s)."""
        if self._state is None:
            self._state = torch.zeros(2, dtype=torch.int64, device=self.device)
        return self._state

    @property
    def counter(self):
        return self.state[0:1]

    def blocks_drawn(self):
        """The counter's value (synchronises: tests, tools, the end of an epoch)."""
        return int(self.state[0].item()) & (2 ** 64 - 1)

    def overflow_events(self):
        """Steps that selected more records than the batch has slots (synchronises)."""
        return int(self.state[1].item())

    def select(self, threshold, n, idx, count):
        """idx [capacity] int64 and count [2] int32 of primia_poisson_select over n records, then the counter moves on by
        ceil(n / 8) blocks; two launches on the current stream, both capturable."""
        st = self.state
        call("primia_poisson_select", *self.key_words, self.nonce, st[0:1], 0, int(threshold), int(n), int(idx.numel()),
             idx, count, st[1:2])
        call("primia_u64_add", st[0:1], query("primia_poisson_blocks", int(n)))


class _PoissonBase:
    """`expected_batch`: the integer L of q = L / n (threshold = floor(L * 2^64 / n), in integers), or None with an
    explicit `threshold` (tests)."""

    def __init__(self, n, expected_batch, capacity, sampler, threshold=None, micro_batches=1, views=1):
        self.n, self.capacity, self.sampler = int(n), int(capacity), sampler
        # augmentation multiplicity (train.py --dp_augmult): every record fills `views` consecutive rows of the batch.  n,
        # expected_batch, capacity, micro_size and slots keep counting RECORDS — what the accountant sees does not change —
        # and the batch (and an engine of one pass) has views times as many rows
        self.views = int(views)
        if self.views < 1:
            raise ValueError("views must be at least 1")
        # a step run as K micro-batch passes (dp_micro): an engine of M = ceil(capacity / K) slots walks K * M >= capacity
        # slots; the selection, its capacity and its stream do not know about K, the extra slots are padding for ever
        self.micro_batches = int(micro_batches)
        if self.micro_batches < 1:
            raise ValueError("micro_batches must be at least 1")
        self.micro_size = -(-self.capacity // self.micro_batches)
        self.slots = self.micro_batches * self.micro_size
        if threshold is None:
            threshold = dp_accountant.threshold_for((int(expected_batch), self.n))     # refuses q >= 1
        self.threshold = int(threshold)
        self.q = dp_accountant.q_of_threshold(self.threshold)       # what the accountant is given
        self.expected_batch = self.q * self.n                       # the L the noised sum is divided by
        L = int(expected_batch) if expected_batch is not None else max(1, int(round(self.expected_batch)))
        self.steps_per_epoch = -(-self.n // L)
        self.draws = 0              # steps sampled so far (host count: the ledger reads its growth per epoch)
        dev = sampler.device
        self.idx = torch.full((self.capacity,), -1, dtype=torch.int64, device=dev)
        self.count = torch.zeros(2, dtype=torch.int32, device=dev)

    def __len__(self):
        return self.steps_per_epoch


class PoissonLoader(_PoissonBase):
    """Poisson batches over a device-resident (data, targets) pair (imagefolder.DeviceLoader's case).  `data` holds
    `repetitions` walks of the same n records, laid out as walk * n + k (imagefolder.register): sampling is over the n
    RECORDS — one person is one record for the accountant however many augmented copies are stored.  __len__ = ceil(n / L).
    Every iteration yields the SAME [capacity, ...] buffer pair, rewritten in place.  A record fills rows s * m .. s * m +
    m - 1 (m = `views`; 1: epoch e reads walk e % repetitions) with its walks (e * m + v) % repetitions, v < m, of epoch e
    (primia_gather_records); with m > repetitions the views repeat stored copies."""

    def __init__(self, data, targets, expected_batch, capacity, sampler, repetitions=1, threshold=None, micro_batches=1,
                 views=1):
        reps = int(repetitions)
        if data.shape[0] % reps or targets.shape[0] != data.shape[0] or targets.dtype != torch.int64 or targets.dim() != 1:
            raise ValueError("PoissonLoader: data [repetitions * n, ...] with hard int64 targets [repetitions * n]")
        super().__init__(data.shape[0] // reps, expected_batch, capacity, sampler, threshold, micro_batches, views)
        self.data, self.targets, self.repetitions = data.contiguous(), targets.contiguous(), reps
        self.row_elems = int(self.data[0].numel())
        self.dt = dtype_code(self.data.dtype)
        row_bytes = self.row_elems * self.data.element_size()
        if row_bytes % 16:
            # (primia_gather_batch copies 16-byte chunks and would refuse every draw with a bare PRIMIA_ERR_ARG)
            raise ValueError("PoissonLoader: one record is {} = {:d} elements of {} = {:d} bytes, not a whole number of "
                             "16-byte chunks; the batch gather needs that (one-channel fp32 images: an even "
                             "train_resolution)".format(tuple(self.data.shape[1:]), self.row_elems, self.data.dtype,
                                                        row_bytes))
        # (the gather writes the first `capacity` slots; the K * M - capacity behind them stay a zero image with target -1)
        rows = self.slots * self.views
        self.x = torch.zeros((rows,) + tuple(self.data.shape[1:]), dtype=self.data.dtype, device=data.device)
        self.y = torch.full((rows,), -1, dtype=torch.int64, device=data.device)
        self.epochs = 0

    def walks(self, epoch):
        """The stored walks a record's views read in epoch `epoch`: (epoch * views + v) % repetitions."""
        return [(int(epoch) * self.views + v) % self.repetitions for v in range(self.views)]

    def draw(self, walk=0):
        """One batch into (self.x, self.y): select, advance, gather — no host synchronisation.  `walk`: the walk of a
        record's first view (the next views - 1 follow it, modulo repetitions)."""
        self.sampler.select(self.threshold, self.n, self.idx, self.count)
        call("primia_gather_records", self.data, self.row_elems, self.n, self.targets, self.idx, int(walk),
             self.repetitions, self.views, self.x, self.y, self.capacity, self.dt)
        self.draws += 1
        return self.x, self.y

    def __iter__(self):
        walk = self.walks(self.epochs)[0]
        self.epochs += 1
        for _ in range(len(self)):
            yield self.draw(walk)


class PoissonAugmentingLoader(_PoissonBase):
    """Poisson batches over a transforming dataset (imagefolder.AugmentingLoader's case: vanilla training on an image
    folder).  The selection is the same kernel; idx and count are read back (one small copy per step: this loader is
    host-driven anyway), the kept images go through TrainTransform.batch and the result is padded to capacity.  `views`
    = m > 1: every kept image goes through the transform m times in a row, each time with its own draws."""

    def __init__(self, images, targets, transform, rng, expected_batch, capacity, sampler, shape, micro_batches=1, views=1):
        super().__init__(len(images), expected_batch, capacity, sampler, micro_batches=micro_batches, views=views)
        self.images, self.targets, self.tf, self.rng = images, targets, transform, rng
        rows = self.slots * self.views
        self.x = torch.zeros((rows,) + tuple(shape), dtype=torch.float32, device=sampler.device)
        self.y = torch.full((rows,), -1, dtype=torch.int64, device=sampler.device)

    def __iter__(self):
        for _ in range(len(self)):
            self.sampler.select(self.threshold, self.n, self.idx, self.count)
            kept = int(self.count[1].item())
            idx = self.idx[:kept]
            self.x.zero_()
            self.y.fill_(-1)
            if kept:
                m = self.views
                self.x[:kept * m] = self.tf.batch([self.images[i] for i in idx.tolist() for _ in range(m)], self.rng)
                self.y[:kept * m] = self.targets.index_select(0, idx).repeat_interleave(m)
            self.draws += 1
            yield self.x, self.y


def records_of(loader, repetitions=1):
    """The number of RECORDS behind an imagefolder loader (a registered dataset holds `repetitions` walks of them)."""
    if hasattr(loader, "images"):
        return len(loader.images)
    return int(loader.data.shape[0]) // int(repetitions)


def from_loader(loader, expected_batch, capacity, sampler, repetitions=1, shape=None, micro_batches=1, views=1):
    """The Poisson-sampled form of imagefolder.DeviceLoader (-> PoissonLoader) or imagefolder.AugmentingLoader
    (-> PoissonAugmentingLoader; `shape`: one transformed image's)."""
    if hasattr(loader, "images"):
        return PoissonAugmentingLoader(loader.images, loader.targets, loader.tf, loader.rng, expected_batch, capacity,
                                       sampler, shape, micro_batches=micro_batches, views=views)
    return PoissonLoader(loader.data, loader.targets, expected_batch, capacity, sampler, repetitions,
                         micro_batches=micro_batches, views=views)
