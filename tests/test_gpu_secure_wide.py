"""GPU: encrypted inference with comparisons wider than 32 bits (fss_bits).  Every protocol form -- the layers
fused and step by step, the argmax tail, whole networks eager, graphed and revealing the class only, three ranks, the CLI -- is
held bit for bit to tests/fss_wide_ref.py's WideOracleContext replaying the GPU dealer's log, and to the plain comparison
[d <= 0] where Python ints say the masked difference does not wrap."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import secure_oracle as S  # noqa: E402
from primia_amd.secure import (Dealer, GraphedSecureInference, PreloadedDealer, SecureContext, SecureResNet18,  # noqa: E402
                               architecture_of, image_requests, model_requests, serving_bytes)
from tests import fss_wide_ref as W  # noqa: E402
from tests.secure_argmax_nets import CRAFTED, first_argmax, oracle_argmax  # noqa: E402
from tests.secure_batch_nets import numpy_sd, oracle_forward  # noqa: E402
from tests.secure_common import (host, in_process_logits, json_line, oracle_pool, run_inference, shares_equal,  # noqa: E402,F401
                                 three_role_logits, write_checkpoint)
from tests.three_role_cases import wide_net as net  # noqa: E402

I64 = torch.int64
PF = 6


def wide_context(cuda, seed, bits, fused=True, pf=PF):
    dealer = Dealer(cuda, seed=seed, fss_bits=bits)
    dealer.log = []
    ctx = SecureContext(dealer, 10, pf)
    ctx.local_fused = fused
    ctx.fuse_newton = fused
    assert ctx.fss_bits == bits
    return dealer, ctx


def wide_oracle(dealer, bits, pf=PF):
    return W.WideOracleContext(W.WideReplayDealer(dealer.log, bits), 10, pf, bits)


def wrapped_count(octx):
    """Comparisons of the replay whose (alpha, d) wrap, and the largest |d| seen (Python ints)."""
    n_wrap, n, top = 0, 0, 0
    for alpha, d in octx.compared:
        for a, q in zip(alpha.tolist(), d.tolist()):
            n_wrap += W.wraps(a, q, octx.bits)
            top = max(top, abs(q))
            n += 1
    return n_wrap, n, top


# ---- 1. layers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "steps"])
def test_relu_and_max_pool_beyond_2_pow_31(cuda, fused):
    """[2, 4, 8, 8] values up to +-5000 at pf = 6: encoded magnitudes up to 5e9 > 2^31, which a 32-bit comparison gets wrong.
    At 64 bits both layers equal the oracle replay bit for bit, no logged (alpha, d) wraps, and the reconstructed ReLU is
    max(x, 0), the reconstructed pool the window maximum, exactly."""
    gen = torch.Generator().manual_seed(64)
    x = (torch.rand(2, 4, 8, 8, generator=gen) * 2 - 1) * 5000
    x[0, 0, 0, :4] = torch.tensor([5000.0, -5000.0, 0.0, 2147.5])
    dealer, ctx = wide_context(cuda, 640 + fused, 64, fused)
    xs = ctx.share(ctx.encode(x.to(cuda)))
    relu, pool = ctx.relu(xs), ctx.max_pool2d_3x3s2(xs)
    octx = wide_oracle(dealer, 64)
    q = S.fix_encode(x.numpy(), 10, PF)
    ox = octx.share(q)
    orelu, opool = octx.relu(ox), octx.max_pool2d_3x3s2(ox)
    assert octx.dealer.pos == len(dealer.log)
    assert shares_equal(relu, orelu) and shares_equal(pool, opool)
    n_wrap, n, top = wrapped_count(octx)
    assert n == 512 + 128 * (4 + 2 + 1 + 1) and n_wrap == 0 and top > 2 ** 32 and int(np.abs(q).max()) > 2 ** 31
    assert np.array_equal(host(ctx.reconstruct(relu)), np.maximum(q, 0))
    pad = np.zeros((2, 4, 10, 10), np.int64)      # (the reference pads the unrolled windows with zeros, nn/functional.py:460-508)
    pad[:, :, 1:9, 1:9] = q
    want = np.stack([pad[:, :, i:i + 8:2, j:j + 8:2] for i in range(3) for j in range(3)]).max(axis=0)
    assert np.array_equal(host(ctx.reconstruct(pool)), want)


# ---- 2. argmax ------------------------------------------------------------------------------------------------------------
WIDE_ROWS = np.array([[0, 2 ** 33, -2 ** 33, 5, 2 ** 33],
                      [2 ** 40, 2 ** 40 - 2 ** 33, 2 ** 40 + 2 ** 33, -2 ** 40, 2 ** 40 + 2 ** 33],
                      [-2 ** 33, -2 ** 34, -2 ** 35, -2 ** 33, -2 ** 36]], np.int64)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "steps"])
def test_argmax_at_64_bits_is_np_argmax(cuda, fused):
    """The crafted logits of tests/secure_argmax_nets.py and rows whose pairwise differences are 2^33 and more: shares of I and
    V equal oracle_argmax on the replay, and the opened index is the first-index argmax."""
    cases = [q for group in CRAFTED.values() for q in group] + [WIDE_ROWS]
    for k, q in enumerate(cases):
        dealer, ctx = wide_context(cuda, 700 + k, 64, fused)
        xs = ctx.share(torch.from_numpy(q).to(cuda))
        I, V = ctx.argmax(xs, values=True)
        octx = wide_oracle(dealer, 64)
        oI, oV = oracle_argmax(octx, octx.share(q))
        assert octx.dealer.pos == len(dealer.log)
        assert shares_equal(I, oI) and shares_equal(V, oV)
        assert wrapped_count(octx)[0] == 0
        assert np.array_equal(host(ctx.reconstruct(I)), first_argmax(q)), (k, q.tolist())
        assert np.array_equal(host(ctx.reconstruct(V)), q.max(axis=1))


# ---- 3. whole networks ----------------------------------------------------------------------------------------------------
SEED = 96


@pytest.fixture(scope="module")
def eager64(cuda, oracle_pool):  # noqa: F811
    """The 8-block network at 32 x 32, two images, pf = 6, 64-bit comparisons, with the argmax tail: the GPU's logit shares
    and classes, and the oracle replay's -- computed once."""
    sd, images = net()
    dealer, ctx = wide_context(cuda, SEED, 64)
    dealer.requests = []
    model = SecureResNet18(ctx, sd, 32, reveal="class")
    L = model.forward_shares(ctx.share(ctx.encode(images.to(cuda)), owner=1))
    classes = host(ctx.open_to(ctx.argmax(L)))
    arch = architecture_of(sd)
    assert dealer.requests == model_requests(arch) + image_requests(arch, 32, 2, reveal="class")
    octx = wide_oracle(dealer, 64)
    oL = oracle_forward(octx, numpy_sd(sd), images.numpy())
    oI, _ = oracle_argmax(octx, oL)
    assert octx.dealer.pos == len(dealer.log)
    return dict(sd=sd, images=images, L=L, classes=classes, oL=oL, oI=oI, octx=octx, stats=dict(ctx.stats))


def test_eager_network_at_64_bits_bit_exact(eager64):
    e = eager64
    assert shares_equal(e["L"], e["oL"])
    q = S.radd(e["oL"][0], e["oL"][1])
    assert np.array_equal(e["classes"], S.radd(e["oI"][0], e["oI"][1])) and np.array_equal(e["classes"], first_argmax(q))
    n_wrap, n, top = wrapped_count(e["octx"])
    print("comparisons", n, "wrapped", n_wrap, "largest |d|", top)
    assert n == e["stats"]["dif_evals"] and n_wrap == 0


def test_graphed_network_at_64_bits_equals_eager_over_two_refills(cuda, eager64):
    sd, images = eager64["sd"], eager64["images"].to(cuda)
    for reveal in ("logits", "class"):
        g = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=PF, seed=SEED + 1, batch=2, reveal=reveal,
                                   fss_bits=64)
        arch = architecture_of(sd)
        assert g.static_bytes == serving_bytes(arch, 32, 2, reveal=reveal, fss_bits=64) > serving_bytes(arch, 32, 2, reveal=reveal)
        keys = [e[0] for e in g.tape if isinstance(e, list) and isinstance(e[0], dict)]
        assert len(keys) == 21 + (2 if reveal == "class" else 0) and all(k["cw_leaf"].shape[0] == 65 for k in keys)
        for step in range(3):      # the primitives of the constructor's refill, then two more refills
            out = g(images, refill=step > 0).clone()
            ectx = SecureContext(PreloadedDealer(g.tape, cuda, 64), 10, PF)
            want = SecureResNet18(ectx, sd, 32, reveal=reveal)(images)
            assert ectx.dealer.pos == len(g.tape) and out.dtype == want.dtype and torch.equal(out, want), (reveal, step)
        assert g.refills == 3


def test_eager_network_at_40_bits_bit_exact(cuda, oracle_pool):  # noqa: F811
    sd, images = net()
    dealer, ctx = wide_context(cuda, SEED + 2, 40)
    model = SecureResNet18(ctx, sd, 32)
    L = model.forward_shares(ctx.share(ctx.encode(images.to(cuda)), owner=1))
    octx = wide_oracle(dealer, 40)
    oL = oracle_forward(octx, numpy_sd(sd), images.numpy())
    assert octx.dealer.pos == len(dealer.log) and shares_equal(L, oL)


# ---- 4. three roles -------------------------------------------------------------------------------------------------------
def test_three_roles_at_64_bits_equal_the_in_process_run(cuda, tmp_path):
    """model_owner / data_owner / crypto_provider as three fresh processes on one GPU over gloo (tests/party_worker.py): both
    parties decode the logits of the in-process run under the same dealer seed."""
    want = in_process_logits(cuda, "wide", PF, SEED + 3)
    for j, got in enumerate(three_role_logits("wide", PF, SEED + 3, tmp_path)):
        assert torch.equal(got, want), j


# ---- 5. CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_fss_bits(cuda, tmp_path):
    """inference.py --fss_bits 64 --precision_fractional 6 prints the classes of the in-process run under the same debug seed;
    --fss_bits 70 is refused before anything runs."""
    sd, _ = net()
    ckpt = write_checkpoint(tmp_path / "bn.pt", sd)
    run = lambda bits: run_inference(ckpt, 2, PF, ["--encrypted_inference", "--fss_bits", str(bits)], batch_size=2)
    res = json_line(run(64))["Inference Results"]
    assert sorted(res) == ["0", "1"] and set(res.values()) <= {0, 1, 2}
    bad = run(70)
    assert bad.returncode != 0 and "--fss_bits must be in [32, 64]" in bad.stderr
