"""GPU: the Z_2^64 GEMM on int8 MFMA limbs (option ring_mfma, csrc/ring_gemm_mfma.hip) against wrapping uint64 arithmetic, bit for
bit: through every entry point that launches it, in the two-party grid against the vector-ALU kernel, past the accumulators'
k bound, and through the mini network, eager and graphed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from primia_amd import _lib  # noqa: E402
from primia_amd._lib import call  # noqa: E402
from primia_amd.secure import (Dealer, GraphedSecureInference, PreloadedDealer, ProtocolForm, SecureContext,  # noqa: E402
                               SecureResNet18)
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet  # noqa: E402
from tests.test_gpu_fss_wide import Guarded, dev  # noqa: E402

U64 = np.uint64
# zero, all ones, the sign bit, the recoding constant (digits -128, -127 x 7), the largest all-positive digits, one digit of -128
PLANTED = [0, 2 ** 64 - 1, 2 ** 63, 0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0x80]
SHAPES = [(1, 1, 1), (70, 147, 5), (16, 65, 130), (33, 200, 64), (49, 4608, 64)]
FORMS = ["plain", "accumulate", "combine-j0", "combine-j1", "dealer"]


def operands(rng, M, K, N):
    """Full-range A [M][K] and B [K][N] with the planted words in row 0 of A and column 0 of B (squares, then mixed pairs)."""
    A = rng.integers(0, 2 ** 64, size=(M, K), dtype=U64)
    B = rng.integers(0, 2 ** 64, size=(K, N), dtype=U64)
    n = min(K, 2 * len(PLANTED))
    A[0, :n] = np.array((PLANTED + PLANTED)[:n], U64)
    B[:n, 0] = np.array((PLANTED + PLANTED[::-1])[:n], U64)
    return A, B


def words(rng, *shape):
    return rng.integers(0, 2 ** 64, size=shape, dtype=U64)


@pytest.fixture
def mfma():
    _lib.set_option("ring_mfma", 1)
    try:
        yield
    finally:
        _lib.set_option("ring_mfma", 0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_integer_product(cuda, mfma, shape, form):
    M, K, N = shape
    rng = np.random.default_rng(M * 1000 + K)
    A, B = operands(rng, M, K, N)
    out = Guarded((M, N), torch.int64, cuda)
    if form in ("plain", "accumulate"):
        c = words(rng, M, N)
        out.view.copy_(dev(c, cuda))
        call("primia_ring_matmul", dev(A, cuda), dev(B, cuda), out.view, M, K, N, int(form == "accumulate"))
        want = A @ B + (c if form == "accumulate" else U64(0))
    elif form == "dealer":
        a1, b1, c0 = words(rng, M, K), words(rng, K, N), words(rng, M, N)
        scratch = Guarded((M * K + K * N,), torch.int64, cuda)
        call("primia_triple_matmul_c1", dev(A, cuda), dev(a1, cuda), dev(B, cuda), dev(b1, cuda), dev(c0, cuda), out.view,
             scratch.view, M, K, N)
        assert scratch.intact()
        want = (A + a1) @ (B + b1) - c0
    else:      # z = c + delta @ (b [+ eps]) + a @ eps: A, B are delta, b
        j = int(form[-1])
        a, eps, c = words(rng, M, K), words(rng, K, N), words(rng, M, N)
        scratch = Guarded((K * N,), torch.int64, cuda)
        call("primia_beaver_combine_matmul", j, dev(A, cuda), dev(eps, cuda), dev(a, cuda), dev(B, cuda), dev(c, cuda), out.view,
             scratch.view, M, K, N)
        assert scratch.intact()
        want = c + A @ (B + eps if j == 0 else B) + a @ eps
    assert out.intact() and np.array_equal(out.host().view(U64), want)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_two_party_grid(cuda, shape):
    """primia_beaver_matmul_local with the option on: both shares are the vector-ALU kernel's, and they add up to x @ y."""
    M, K, N = shape
    rng = np.random.default_rng(M * 1000 + K + 1)
    x0, y0 = operands(rng, M, K, N)
    x1, y1, a1, b1, c0 = words(rng, M, K), words(rng, K, N), words(rng, M, K), words(rng, K, N), words(rng, M, N)
    a0, b0 = operands(rng, M, K, N)
    c1 = (a0 + a1) @ (b0 + b1) - c0
    inputs = [dev(t, cuda) for t in (x0, x1, y0, y1, a0, b0, c0, a1, b1, c1)]
    got = {}
    try:
        for on in (1, 0):
            _lib.set_option("ring_mfma", on)
            z = [Guarded((M, N), torch.int64, cuda) for _ in range(2)]
            scratch = Guarded((M * K + 2 * K * N,), torch.int64, cuda)
            call("primia_beaver_matmul_local", *inputs, z[0].view, z[1].view, scratch.view, M, K, N)
            assert scratch.intact() and z[0].intact() and z[1].intact()
            got[on] = [t.host().view(U64) for t in z]
    finally:
        _lib.set_option("ring_mfma", 0)
    assert np.array_equal(got[1][0], got[0][0]) and np.array_equal(got[1][1], got[0][1])
    assert np.array_equal(got[1][0] + got[1][1], (x0 + x1) @ (y0 + y1))


@pytest.mark.parametrize("pairs", [1, 2])
def test_slice_cap(cuda, mfma, pairs):
    """K = 16,704 at 256 tiles, where the tile rule alone gives one slice.  A[m][k] = u[m], B[k][n] = v[n]: C = K u v.  For the
    pair of 0x8080808080808080 diagonal 7 gains 2 * 128 * 127 + 6 * 127^2 = 129,286 per k, 2.16e9 > 2^31 over all of K (derived,
    not measured): an accumulator that is not cut at 16,320 k wraps.  pairs = 2: the combine's two products share the
    accumulators, so its slices are half as deep; delta = a and b = eps here, z = c + 2 K u v."""
    M = N = 1024
    K = 16704
    cyc = [PLANTED[3]] + PLANTED[:3] + PLANTED[4:]
    u = np.array([cyc[i % 6] for i in range(M)], U64)
    v = np.array([cyc[(i * 5) % 6] for i in range(N)], U64)      # (5 is coprime to 6: every pair of planted words meets)
    A, B = dev(np.repeat(u[:, None], K, axis=1), cuda), dev(np.repeat(v[None, :], K, axis=0), cuda)
    out = Guarded((M, N), torch.int64, cuda)
    want = U64(K) * (u[:, None] * v[None, :])
    if pairs == 1:
        call("primia_ring_matmul", A, B, out.view, M, K, N, 0)
    else:
        c = words(np.random.default_rng(3), M, N)
        call("primia_beaver_combine_matmul", 1, A, B, A, B, dev(c, cuda), out.view, None, M, K, N)
        want = c + U64(2) * want
    assert out.intact() and np.array_equal(out.host().view(U64), want)


def test_network_is_bit_equal(cuda):
    """The mini network at 32 x 32, batch 2, one dealer seed: the output shares with ring_mfma are those without; two replays
    of the serving graph captured with it equal the eager pass of the default kernels on the primitives the graph holds."""
    gen = torch.Generator().manual_seed(520)
    sd = mini_resnet(gen)
    images = torch.randn(2, 3, 32, 32, generator=gen).to(cuda)
    form = ProtocolForm(fss_bits=64)

    def model(dealer, on):
        return SecureResNet18(SecureContext(dealer, 10, 6, ring_mfma=on), sd, 32, MINI_BLOCKS, form=form)

    try:
        shares = {}
        for on in (True, False):
            m = model(Dealer(cuda, seed=521, fss_bits=64), on)
            assert _lib.get_option("ring_mfma") == int(on)
            shares[on] = [t.cpu() for t in m.forward_shares(m.ctx.share(m.ctx.encode(images), owner=1))]
        assert torch.equal(shares[True][0], shares[False][0]) and torch.equal(shares[True][1], shares[False][1])
        g = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=6, seed=521, blocks=MINI_BLOCKS, batch=2, form=form,
                                   ring_mfma=True)
        for step in range(2):      # the primitives of the constructor's refill, then of one replayed refill
            out = g(images, refill=step > 0).clone()
            assert torch.equal(out, model(PreloadedDealer(g.tape, cuda, 64), False)(images)), step
    finally:
        _lib.set_option("ring_mfma", 0)
