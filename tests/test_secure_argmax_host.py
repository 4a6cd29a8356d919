"""CPU: the definition of the secret-shared argmax (tests/secure_argmax_nets.py) against np.argmax on crafted logits, and the
host-side schedule and memory arithmetic of a pass that reveals the class only (no device is touched)."""
import numpy as np
import pytest
import torch

from oracle import secure_oracle as S
from primia_amd import _lib
from primia_amd.secure import (DIF_KEY_BYTES, REVEALS, architecture_of, argmax_requests, image_requests, largest_batch_that_fits,
                               primitive_bytes, serving_bytes)
from tests.secure_argmax_nets import CRAFTED, first_argmax, oracle_argmax, spread, tail_requests
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet, resnet18
from tests.secure_groupnorm_nets import RecordingDealer, ScheduleContext, group_mini, group_resnet18


@pytest.mark.parametrize("shape", sorted(CRAFTED), ids=lambda s: "x".join(map(str, s)))
def test_oracle_argmax_is_the_first_index_argmax(shape):
    """oracle_argmax on a recording dealer, every comparison evaluated: the reconstructed indices are np.argmax's (the first
    index on ties) and the reconstructed maxima the row maxima, for exact ties, all-equal rows, negative values and the
    maximum in the first, middle and last column; the requests are the tail's, in order.  Every pairwise difference of the
    crafted logits is below 2^31 (asserted)."""
    B, C = shape
    firsts = set()
    for n, q in enumerate(CRAFTED[shape]):
        assert q.shape == shape and q.dtype == np.int64
        assert spread(q) < 2 ** 31
        want = first_argmax(q)
        firsts.update(int(w) for w in want)
        for seed in (1, 2):
            d = RecordingDealer(100 * n + seed)
            ctx = S.OracleContext(d, 10, 3)
            shares = ctx.share(q)
            n0 = len(d.requests)
            I, V = oracle_argmax(ctx, shares)
            assert d.requests[n0:] == tail_requests(B, C)
            got, top = S.radd(I[0], I[1]), S.radd(V[0], V[1])
            assert got.shape == (B,) and got.dtype == np.int64
            assert np.array_equal(got, want), (q.tolist(), got.tolist(), want.tolist())
            assert np.array_equal(top, q.max(axis=1))
            # the shares themselves are masked: neither party's word is the index
            assert not np.array_equal(I[0], want) and not np.array_equal(I[1], want)
    assert {0, C - 1} <= firsts and (C < 3 or firsts & set(range(1, C - 1)))      # first, last and a middle column win


NETS = [("mini-batch", lambda: mini_resnet(torch.Generator().manual_seed(21)), MINI_BLOCKS),
        ("mini-group", lambda: group_mini(torch.Generator().manual_seed(31)), MINI_BLOCKS),
        ("resnet18-batch", lambda: resnet18(32, 320), None),
        ("resnet18-group", lambda: group_resnet18(32, 520), None)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("net", NETS, ids=lambda n: n[0])
def test_class_schedule_is_the_logits_schedule_plus_the_walk(net, B):
    """image_requests(reveal="class") is the logits form's list followed by exactly what oracle_argmax records on a
    schedule-only context for [B, classes] logits; without the argument, and with reveal="logits", the list is the one the
    project had before; primitive_bytes, serving_bytes and largest_batch_that_fits grow by exactly the appended requests."""
    _, make, blocks = net
    arch = architecture_of(make())
    classes = arch["fc.weight"][0]
    for pooling in ("max", "avg"):
        plain = image_requests(arch, 32, B, blocks, pooling)
        assert plain == image_requests(arch, 32, B, blocks, pooling, reveal="logits")
        assert plain[-1] == ("triple", ("matmul", (B, arch["fc.weight"][1]), (arch["fc.weight"][1], classes)), {})
        assert not any(k == "triple" and a[1] == (B, 2) for k, a, _ in plain)
        full = image_requests(arch, 32, B, blocks, pooling, reveal="class")
        assert full[:len(plain)] == plain and len(full) == len(plain) + 1 + 3 * (classes - 1)
        d = RecordingDealer(0)
        ctx = ScheduleContext(d, 10, 3)
        oracle_argmax(ctx, [np.zeros((B, classes), np.int64), np.zeros((B, classes), np.int64)])
        tail = full[len(plain):]
        assert [(k, a) for k, a, _ in tail] == d.requests == tail_requests(B, classes)
        assert tail == argmax_requests(B, classes)
        assert all(kw == {"owner": None} for k, _, kw in tail if k == "const_mask")
        extra = primitive_bytes(tail)
        assert extra == 8 * B * classes + (classes - 1) * (DIF_KEY_BYTES * B + 16 * 3 * 2 * B)
        assert primitive_bytes(full) == primitive_bytes(plain) + extra
        assert serving_bytes(arch, 32, B, blocks, pooling, reveal="class") == primitive_bytes(full) + primitive_bytes(full) // 8
        assert serving_bytes(arch, 32, B, blocks, pooling) == primitive_bytes(plain) + primitive_bytes(plain) // 8
    budget = serving_bytes(arch, 32, 4, blocks, reveal="class")
    assert largest_batch_that_fits(arch, 32, budget, blocks, reveal="class") == 4
    assert largest_batch_that_fits(arch, 32, budget - 1, blocks, reveal="class") == 3
    assert largest_batch_that_fits(arch, 32, serving_bytes(arch, 32, 4, blocks), blocks) == 4


def test_reveal_argument_is_checked():
    arch = architecture_of(mini_resnet(torch.Generator().manual_seed(21)))
    assert REVEALS == ("logits", "class")
    for fn in (lambda r: image_requests(arch, 32, 1, MINI_BLOCKS, reveal=r), lambda r: serving_bytes(arch, 32, 1, MINI_BLOCKS, reveal=r)):
        with pytest.raises(ValueError, match="reveal"):
            fn("argmax")


def test_header_declares_the_argmax_step():
    """primia_argmax_combine_local: bit, the [B][w] logits with width and column, the shares of K, the six triple pointers, V
    and I in place, B and the stream -- and the built library exports it."""
    protos = _lib.parse_header()
    assert "primia_argmax_combine_local" in protos
    names = [n for _, n in protos["primia_argmax_combine_local"][1]]
    assert names == ["bit0", "bit1", "logits0", "logits1", "w", "start", "k0", "k1", "a0", "b0", "c0", "a1", "b1", "c1", "v0",
                     "v1", "i0", "i1", "B", "stream"]
    import ctypes

    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "primia_argmax_combine_local")
