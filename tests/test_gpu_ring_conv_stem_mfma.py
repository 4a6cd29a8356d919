"""GPU: the thin-channel 7 x 7 / 2 ring convolution on int8 MFMA limbs (ring_mfma = 2 with conv_triples,
csrc/ring_conv_stem_mfma.hip) against NumPy's wrapping uint64 convolution, bit for bit: every form, the two-job grid with the
epilogue's truncation against the vector-ALU kernel, and through the mini network, eager and graphed."""
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
from tests.test_gpu_ring_conv_mfma import operands  # noqa: E402

U64 = np.uint64
# B, C, H, W, O, R, stride, pad: the zero row 7, tap 7 and channel pad; the halo on all four sides and on none; patch row and
# column 21; O and pixels past the tile
SHAPES = [(1, 3, 18, 18, 70, 7, 2, 3),      # 9 x 9 outputs: ragged pixel tiles in both directions, O across 64
          (2, 1, 15, 17, 5, 7, 2, 3),       # grayscale, two images, odd and non-square (8 x 9 outputs)
          (1, 4, 48, 48, 8, 7, 2, 3),       # every channel byte live; of the 3 x 3 tiles the centre one touches no border
          (1, 2, 9, 9, 3, 7, 2, 0)]         # no padding, 2 x 2 outputs inside one tile


@pytest.fixture
def level():
    try:
        yield lambda v: _lib.set_option("ring_mfma", v)
    finally:
        _lib.set_option("ring_mfma", 0)


@pytest.mark.parametrize("form", ["plain", "accumulate", "two-pairs"])
@pytest.mark.parametrize("g", SHAPES, ids=lambda g: "x".join(map(str, g)))
def test_kernel_equals_the_integer_convolution(cuda, level, g, form):
    level(2)
    xs, ws, zs = shapes_of(g)
    rng = np.random.default_rng(g[1] * 100 + g[4])
    assert _lib.query("primia_ring_conv2d_route", *args_of(g), 1) == 1
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


@pytest.mark.parametrize("div", [10 ** 6, 0])
def test_two_jobs_and_the_truncation_equal_the_vector_alu(cuda, level, div):
    """primia_beaver_conv_local: both parties' sums in one grid, truncated in the epilogue (div = 0: left whole)."""
    g = (2, 3, 18, 18, 70, 7, 2, 3)
    xs, ws, zs = shapes_of(g)
    rng = np.random.default_rng(72)      # x0 x1 w0 w1 a0 b0 c0 a1 b1 c1
    shares = [dev(words(rng, s), cuda) for s in (xs, xs, ws, ws, xs, ws, zs, xs, ws, zs)]
    scratch = torch.empty(_lib.query("primia_beaver_conv_local_scratch_elems", *args_of(g)[:7]), dtype=torch.int64, device=cuda)
    got = {}
    for value in (2, 0):
        level(value)
        assert _lib.query("primia_ring_conv2d_route", *args_of(g), 2) == value // 2
        outs = [Guarded(zs, torch.int64, cuda) for _ in range(2)]
        call("primia_beaver_conv_local", *shares, outs[0].view, outs[1].view, scratch, *args_of(g), div)
        assert outs[0].intact() and outs[1].intact()
        got[value] = [o.host() for o in outs]
    assert all(np.array_equal(got[2][j], got[0][j]) for j in range(2))


def test_network_is_bit_equal(cuda, level):
    """The mini network at 32 x 32, batch 2, conv_triples, one dealer seed: the shares at ring_mfma = 2 are those without; two
    replays of the serving graph captured at level 2 (its refill completes the stem's triple on the new kernel) equal the
    eager pass of the vector-ALU kernels."""
    gen = torch.Generator().manual_seed(530)
    sd = mini_resnet(gen)
    images = torch.randn(2, 3, 32, 32, generator=gen).to(cuda)
    form = ProtocolForm(fss_bits=64, conv_triples=True)

    def model(dealer, on):
        return SecureResNet18(SecureContext(dealer, 10, 6, ring_mfma=on), sd, 32, MINI_BLOCKS, form=form)

    shares = {}
    for on in (2, False):
        m = model(Dealer(cuda, seed=531, fss_bits=64), on)
        shares[on] = [t.cpu() for t in m.forward_shares(m.ctx.share(m.ctx.encode(images), owner=1))]
        assert _lib.get_option("ring_mfma") == int(on)
    assert torch.equal(shares[2][0], shares[False][0]) and torch.equal(shares[2][1], shares[False][1])
    gi = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=6, seed=531, blocks=MINI_BLOCKS, batch=2,
                                form=form, ring_mfma=2)
    assert _lib.get_option("ring_mfma") == 2
    for step in range(2):      # the primitives of the constructor's refill, then of one replayed refill
        out = gi(images, refill=step > 0).clone()
        assert torch.equal(out, model(PreloadedDealer(gi.tape, cuda, 64), False)(images)), step
