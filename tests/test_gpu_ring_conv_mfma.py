"""GPU: the ring convolution on int8 MFMA limbs (options ring_mfma + conv_triples, csrc/ring_conv_mfma.hip) against NumPy's
wrapping uint64 convolution, bit for bit: every form and geometry, past the accumulators' bound, and through the mini network,
eager and graphed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from primia_amd import _lib  # noqa: E402
from primia_amd._lib import call  # noqa: E402
from primia_amd.secure import (Dealer, GraphedSecureInference, PreloadedDealer, ProtocolForm, SecureContext,  # noqa: E402
                               SecureResNet18)
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet  # noqa: E402
from tests.test_gpu_conv_triples import args_of, conv_ref, shapes_of, words  # noqa: E402
from tests.test_gpu_fss_wide import Guarded, dev  # noqa: E402
from tests.test_gpu_ring_mfma import PLANTED  # noqa: E402

U64 = np.uint64
# B, C, H, W, O, R, stride, pad
SHAPES = [(1, 5, 9, 9, 70, 3, 1, 1),        # ragged pixel tile, O across 64, a chunk of 5 live channels
          (2, 70, 9, 9, 8, 3, 1, 1),        # C across the 64 chunk, two images
          (2, 3, 9, 9, 5, 3, 2, 1),         # stride 2, odd size
          (1, 66, 8, 8, 5, 3, 2, 1),        # stride 2, even size, C across a chunk
          (1, 65, 9, 9, 6, 1, 2, 0),        # 1 x 1 / 2
          (1, 160, 7, 7, 64, 3, 1, 1)]      # one block: the split exceeds 1, the last chunk is ragged


@pytest.fixture
def mfma():
    _lib.set_option("ring_mfma", 1)
    try:
        yield
    finally:
        _lib.set_option("ring_mfma", 0)


def operands(rng, xs, ws):
    """Full-range words; the planted ones meet along the channels of output (0, 0, 0, 0) and along an input row."""
    x, w = words(rng, xs), words(rng, ws)
    n, mid = min(xs[1], 12), ws[2] // 2
    x[0, :n, 0, 0] = np.array((PLANTED + PLANTED)[:n], U64)
    w[0, :n, mid, mid] = np.array((PLANTED + PLANTED[::-1])[:n], U64)
    x[-1, -1, 1, :6] = np.array(PLANTED, U64)
    return x, w


@pytest.mark.parametrize("form", ["plain", "accumulate", "two-pairs"])
@pytest.mark.parametrize("g", SHAPES, ids=lambda g: "x".join(map(str, g)))
def test_kernel_equals_the_integer_convolution(cuda, mfma, g, form):
    xs, ws, zs = shapes_of(g)
    rng = np.random.default_rng(g[1] * 100 + g[4])
    assert _lib.query("primia_ring_conv2d_route", *args_of(g), 1) == 1
    assert g[1] != 160 or _lib.query("primia_ring_conv2d_split", *args_of(g), 1) > 1
    out = Guarded(zs, torch.int64, cuda)
    (x, w), c = operands(rng, xs, ws), words(rng, zs)
    want = conv_ref(x, w, g[6], g[7])
    if form != "plain":
        out.view.copy_(dev(c, cuda))
        want = want + c
    if form == "two-pairs":      # party 1's combine z = c + conv(delta, b) + conv(a, eps), in place on c
        a, e = operands(rng, xs, ws)
        call("primia_beaver_combine_conv", 1, dev(x, cuda), dev(e, cuda), dev(a, cuda), dev(w, cuda), out.view, out.view, None,
             *args_of(g))
        want = want + conv_ref(a, e, g[6], g[7])
    else:
        call("primia_ring_conv2d", dev(x, cuda), dev(w, cuda), out.view, *args_of(g), int(form == "accumulate"))
    assert out.intact() and np.array_equal(out.host().view(U64), want)


def test_slice_cap(cuda, mfma):
    """960 channels x 9 taps, two pairs, 256 blocks (no few-block split): every word is 0x80..80, every digit -128, and the
    centre output's diagonal 7 would reach 2 x 960 x 9 x 2^17 = 2.26e9 > 2^31 in one slice (derived, not measured)."""
    g = (256, 960, 3, 3, 8, 3, 1, 1)
    xs, ws, zs = shapes_of(g)
    assert _lib.query("primia_ring_conv2d_split", *args_of(g), 1) > 1
    x, w = dev(np.full(xs, PLANTED[3], U64), cuda), dev(np.full(ws, PLANTED[3], U64), cuda)
    c = words(np.random.default_rng(4), zs)
    out = Guarded(zs, torch.int64, cuda)
    call("primia_beaver_combine_conv", 1, x, w, x, w, dev(c, cuda), out.view, None, *args_of(g))
    one = conv_ref(np.full((1,) + xs[1:], PLANTED[3], U64), np.full((1,) + ws[1:], PLANTED[3], U64), 1, 1)
    assert out.intact() and np.array_equal(out.host().view(U64), c + U64(2) * one)


def test_network_is_bit_equal(cuda):
    """The mini network at 32 x 32, batch 2, conv_triples, one dealer seed: the output shares with ring_mfma are those
    without; two replays of the serving graph captured with both equal the eager pass of the vector-ALU kernels."""
    gen = torch.Generator().manual_seed(530)
    sd = mini_resnet(gen)
    images = torch.randn(2, 3, 32, 32, generator=gen).to(cuda)
    form = ProtocolForm(fss_bits=64, conv_triples=True)

    def model(dealer, on):
        return SecureResNet18(SecureContext(dealer, 10, 6, ring_mfma=on), sd, 32, MINI_BLOCKS, form=form)

    try:
        shares = {}
        for on in (True, False):
            m = model(Dealer(cuda, seed=531, fss_bits=64), on)
            shares[on] = [t.cpu() for t in m.forward_shares(m.ctx.share(m.ctx.encode(images), owner=1))]
        assert torch.equal(shares[True][0], shares[False][0]) and torch.equal(shares[True][1], shares[False][1])
        gi = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=6, seed=531, blocks=MINI_BLOCKS, batch=2,
                                    form=form, ring_mfma=True)
        for step in range(2):      # the primitives of the constructor's refill, then of one replayed refill
            out = gi(images, refill=step > 0).clone()
            assert torch.equal(out, model(PreloadedDealer(gi.tape, cuda, 64), False)(images)), step
    finally:
        _lib.set_option("ring_mfma", 0)
