"""CPU: the definition of the confusion-matrix tail of an encrypted evaluation (tests/secure_confusion_nets.py) against numpy's
counts on crafted logits and labels, equality on 32 bits, and the host-side schedule and memory arithmetic of a pass with
reveal="confusion" (no device is touched)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import secure_oracle as S
from primia_amd import _lib
from primia_amd.secure import (DIF_KEY_BYTES, DPF_KEY_BYTES, architecture_of, argmax_requests, confusion_requests, dpf_key_fields,
                               image_requests, largest_batch_that_fits, primitive_bytes, serving_bytes)
from tests.secure_argmax_nets import CRAFTED, first_argmax, spread
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet, resnet18
from tests.secure_confusion_nets import (GPU_TAIL_SEEDS, ConfusionChaChaDealer, ConfusionRecordingDealer, ConfusionReplayDealer,
                                         confusion_tail_requests, crafted_cases, numpy_confusion, onehot, oracle_confusion,
                                         oracle_eq, zero_matrix)
from tests.secure_groupnorm_nets import ScheduleContext, group_mini, group_resnet18

I64 = np.int64
SHAPES = sorted(CRAFTED)
ids = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_oracle_confusion_counts_what_numpy_counts(shape):
    """oracle_confusion on a recording dealer over ALL crafted cases of a shape as the passes of one evaluation, under two
    fixed dealer seeds: P reconstructs to the one-hot of the first-index argmax, Mc to the pass's counts and the final M to
    numpy's confusion of first_argmax against the labels; sum(M) is the number of labelled rows (padding rows add nothing);
    the cases fill diagonal and off-diagonal cells and have a padding row; the requests are the tail's, in order; no share
    is the value it hides."""
    B, C = shape
    cases = crafted_cases(shape)
    for seed in (1, 2):
        d = ConfusionRecordingDealer(1000 * B + 10 * C + seed)
        ctx = S.OracleContext(d, 10, 3)
        M, want = zero_matrix(C), np.zeros((C, C), I64)
        for q, labels, y, counts in cases:
            assert spread(q) < 2 ** 31 and spread(q) <= 20_000      # |d| / 2^32 < 5e-6 per comparison
            shares = ctx.share(q)
            n0 = len(d.requests)
            P, Mc, M = oracle_confusion(ctx, shares, y, M)
            assert d.requests[n0:] == confusion_tail_requests(B, C)
            assert np.array_equal(S.radd(*P), onehot(first_argmax(q), C))
            assert np.array_equal(S.radd(*Mc), counts)
            assert not np.array_equal(P[0], S.radd(*P)) and not np.array_equal(Mc[1], counts)
            want += counts
        got = S.radd(*M)
        assert got.dtype == I64 and got.shape == (C, C)
        assert np.array_equal(got, want)
        assert np.array_equal(got, numpy_confusion(np.concatenate([c[1] for c in cases]),
                                                   np.concatenate([first_argmax(c[0]) for c in cases]), C))
        assert int(got.sum()) == sum(int((c[1] >= 0).sum()) for c in cases)
    assert any((c[1] < 0).any() for c in cases)                      # an all-zero label row
    assert np.trace(want) > 0 and want.sum() - np.trace(want) > 0    # diagonal and off-diagonal cells


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_gpu_seeds_are_seeds_for_which_the_oracle_alone_is_right(shape):
    """All crafted cases of a shape as the passes of one evaluation on the host mirror of the device dealer, under the debug seed the
    GPU test of the tail uses for this shape: the counts are right, so a GPU failure under that seed is the device code's."""
    B, C = shape
    ctx = S.OracleContext(ConfusionChaChaDealer(GPU_TAIL_SEEDS[shape]), 10, 3)
    M, want = zero_matrix(C), np.zeros((C, C), I64)
    for q, _, y, counts in crafted_cases(shape):
        _, _, M = oracle_confusion(ctx, ctx.share(q), y, M)
        want += counts
    assert np.array_equal(S.radd(*M), want)


def test_oracle_eq_sees_32_bits():
    """eq answers 1 for equal values and 0 for different ones, whatever the shares look like -- and 1 for two values 2^32
    apart: the layer sees the low 32 bits of the difference, and this pins that."""
    x1 = np.array([[3, 0, -5, 2 ** 32 + 7, 7, -1], [2 ** 40, 1, 2, 5 * 2 ** 32, 2 ** 31, 9]], I64)
    x2 = np.array([[3, 1, -5, 7, 2 ** 32 + 7, 2 ** 32 - 1], [2 ** 40, 1, 3, 0, -2 ** 31, 2 ** 33 + 9]], I64)
    want = np.array([[1, 0, 1, 1, 1, 1], [1, 1, 0, 1, 1, 1]], I64)
    for seed in (5, 6):
        d = ConfusionRecordingDealer(seed)
        ctx = S.OracleContext(d, 10, 3)
        a, b = ctx.share(x1), ctx.share(x2)
        out = oracle_eq(ctx, a, b)
        assert d.requests[-1] == ("dpf_keys", (12,))
        assert out[0].shape == (2, 6) and out[0].dtype == I64
        assert np.array_equal(S.radd(*out), want)
        assert not np.array_equal(out[0], want)


NETS = [("mini-batch", lambda: mini_resnet(torch.Generator().manual_seed(21)), MINI_BLOCKS),
        ("mini-group", lambda: group_mini(torch.Generator().manual_seed(31)), MINI_BLOCKS),
        ("resnet18-batch", lambda: resnet18(32, 320), None),
        ("resnet18-group", lambda: group_resnet18(32, 520), None)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("net", NETS, ids=lambda n: n[0])
def test_confusion_schedule_extends_the_class_schedule(net, B):
    """image_requests(reveal="confusion") is the class form's list, itself the logits form's list plus the walk, followed by
    exactly what oracle_confusion records after the walk; confusion_requests names the owners; the bytes grow by exactly the
    appended requests, a DPF key counted at the size its field shapes give."""
    _, make, blocks = net
    arch = architecture_of(make())
    C = arch["fc.weight"][0]
    for pooling in ("max", "avg"):
        logits = image_requests(arch, 32, B, blocks, pooling, reveal="logits")
        klass = image_requests(arch, 32, B, blocks, pooling, reveal="class")
        full = image_requests(arch, 32, B, blocks, pooling, reveal="confusion")
        assert len(logits) < len(klass) < len(full)
        assert full[:len(klass)] == klass and klass[:len(logits)] == logits
        tail = full[len(klass):]
        assert tail == confusion_requests(B, C) and klass[len(logits):] == argmax_requests(B, C)
        assert [kw for _, _, kw in tail] == [{"owner": 1}, {"owner": None}, {}, {}]
        d = ConfusionRecordingDealer(0)
        z = [np.zeros((B, C), I64), np.zeros((B, C), I64)]
        oracle_confusion(ScheduleContext(d, 10, 3), z, np.zeros((B, C), I64), zero_matrix(C))
        assert [(k, a) for k, a, _ in full[len(logits):]] == d.requests == confusion_tail_requests(B, C)
        extra = primitive_bytes(tail)
        assert extra == 2 * 8 * B * C + DPF_KEY_BYTES * B * C + 16 * (2 * B * C + C * C)
        assert primitive_bytes(full) == primitive_bytes(klass) + extra
        assert primitive_bytes(full, 64) == primitive_bytes(klass, 64) + extra      # equality stays at 32 bits
        assert serving_bytes(arch, 32, B, blocks, pooling, reveal="confusion") == primitive_bytes(full) + primitive_bytes(full) // 8
    budget = serving_bytes(arch, 32, 4, blocks, reveal="confusion")
    assert largest_batch_that_fits(arch, 32, budget, blocks, reveal="confusion") == 4
    assert largest_batch_that_fits(arch, 32, budget - 1, blocks, reveal="confusion") == 3


def test_dpf_key_bytes_follow_the_field_shapes():
    """One DPF key: raw alpha, its mask and party 0's share, both parties' seeds, and the correction words at the sizes of
    dpf_key_fields -- which are the shapes the header gives (cw_bits uint8 [32][n], cw_s uint64 [32][2][n], the leaf int64
    [n]) and the shapes the oracle's keygen produces."""
    n = 5
    fields = dpf_key_fields(n)
    assert fields == [((32, n), torch.uint8), ((32, 2, n), torch.int64), ((n,), torch.int64)]
    cw = sum(int(np.prod(s)) * torch.empty(0, dtype=dt).element_size() for s, dt in fields)
    assert cw == n * (32 + 32 * 2 * 8 + 8)
    assert DPF_KEY_BYTES == 3 * 8 + 2 * 2 * 8 + cw // n == 608 < DIF_KEY_BYTES
    assert primitive_bytes([("dpf_keys", (n,), {})]) == n * DPF_KEY_BYTES == primitive_bytes([("dpf_keys", (n,), {})], 64)
    rng = np.random.default_rng(3)
    alpha = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    s0 = rng.integers(0, 2 ** 63, size=(2, 2, n), dtype=np.uint64)
    _, keys = S.dpf_keygen(alpha, s0)
    assert [tuple(keys[0][k].shape) for k in ("bits", "cw_s", "cw_n")] == [(32, 2, n), (32, 2, n), (n,)]      # (bits: one byte per side)


def test_replay_dealer_serves_dpf_entries():
    """ConfusionReplayDealer re-derives the equality keys of a ("dpf", ...) log entry with the oracle's keygen and splits alpha
    like the device dealer; an entry of another kind in its place is refused."""
    n = 4
    rng = np.random.default_rng(9)
    alpha = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    s0 = rng.integers(0, 2 ** 63, size=(2, 2, n), dtype=np.uint64)
    r = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    d = ConfusionReplayDealer([("dpf", n, alpha.view(I64), s0.view(I64), r.view(I64)), ("mask", np.zeros(2, I64))])
    (a0, a1), keys = d.dpf_keys(n)
    assert np.array_equal((a0 + a1) & np.uint64(0xFFFFFFFF), alpha) and np.array_equal(a1, r)
    _, want = S.dpf_keygen(alpha, s0)
    assert all(np.array_equal(keys[b][k], want[b][k]) for b in range(2) for k in want[b])
    x = alpha.copy()
    x[1] ^= np.uint64(1)
    assert np.array_equal(S.radd(S.dpf_eval(0, x, keys[0]), S.dpf_eval(1, x, keys[1])), np.array([1, 0, 1, 1], I64))
    with pytest.raises(AssertionError):
        d.dpf_keys(2)


def test_header_declares_the_two_kernels():
    """primia_dpf_eval_local takes primia_dif_eval_local's operands with the DPF key fields; primia_confusion_combine_local the
    labels, the one-hot classes, the six triple pointers and the accumulator in place -- and the built library exports both."""
    protos = _lib.parse_header()
    names = lambda f: [n for _, n in protos[f][1]]
    dif = names("primia_dif_eval_local")
    assert names("primia_dpf_eval_local") == dif[:dif.index("cw_bits")] + ["cw_bits", "cw_s", "cw_n", "out0", "out1", "n", "stream"]
    assert names("primia_confusion_combine_local") == ["y0", "y1", "p0", "p1", "a0", "b0", "c0", "a1", "b1", "c1", "m0", "m1", "B",
                                                       "C", "stream"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "primia_dpf_eval_local") and hasattr(lib, "primia_confusion_combine_local")
