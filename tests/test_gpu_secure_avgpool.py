"""GPU: encrypted inference for a checkpoint trained with pooling_type = avg.  The stem keeps the order the network was
trained with, conv1 -> bn1 -> ReLU -> AvgPool2d(3, 2, 1) (the reference's pool / ReLU swap is an identity for a max pool
only); the pool is a party-local window sum and truncating division by 9, read in place by primia_avg_pool_syft(_2p).
Kernels and whole networks are held BIT-EXACT to the CPU oracle, the decoded logits to the float64 plaintext forward of the
avg model, in the eager, graphed, pipelined, three-role and CLI forms."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import secure_oracle as S  # noqa: E402
from primia_amd import resnet_spec  # noqa: E402
from primia_amd._lib import PrimiaError, call  # noqa: E402
from primia_amd.secure import (Dealer, GraphedSecureInference, PipelinedSecureInference, PreloadedDealer,  # noqa: E402
                               SecureContext, SecureResNet18, architecture_of, image_requests, model_requests)
from tests.secure_avgpool_nets import oracle_avg_pool, plaintext_logits  # noqa: E402
from tests.secure_batch_nets import MINI_BLOCKS, draw_bn, mini_resnet, numpy_sd, oracle_forward, resnet18  # noqa: E402
from tests.secure_common import (I64, PLAIN_TOL, context, guarded, guards_intact, host, in_process_logits,  # noqa: E402,F401
                                 json_line, oracle_pool, run_inference, shares_equal, three_role_logits, time_limit,
                                 wrapping_shares, write_checkpoint)


# ---- 1. the kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,pad", [(3, 2, 1), (7, 7, 0)])
@pytest.mark.parametrize("shape", [(1, 64, 112, 112), (3, 5, 33, 33), (2, 130, 7, 7)])
def test_avg_pool_kernels_equal_the_chain_and_the_oracle(cuda, shape, k, stride, pad):
    """primia_avg_pool_syft and primia_avg_pool_syft_2p against (a) the chain primia_pool_unroll_syft -> primia_ring_rowsum
    -> primia_trunc_div they replace and (b) pre_pool + wrapping sum + trunc_div on the host, bit for bit, on shares whose
    window sums wrap; nothing is written outside the outputs (guard words on both sides stay)."""
    B, C, H, W = shape
    rng = np.random.default_rng(H * 1000 + C * 10 + k)
    xs = [wrapping_shares(rng, shape) for _ in range(2)]
    want = oracle_avg_pool(xs, k, stride, pad)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    assert want[0].shape == (B, C, Ho, Wo)
    rows = B * C * Ho * Wo
    xd = [torch.from_numpy(x).to(cuda) for x in xs]
    chain = []
    for j in range(2):
        im = torch.empty(rows, k * k, dtype=I64, device=cuda)
        call("primia_pool_unroll_syft", xd[j], im, B, C, H, W, k, stride, pad)
        s = torch.empty(rows, dtype=I64, device=cuda)
        call("primia_ring_rowsum", im, s, rows, k * k)
        o = torch.empty(rows, dtype=I64, device=cuda)
        call("primia_trunc_div", s, k * k, o, rows)
        chain.append(o)
        assert np.array_equal(host(o).reshape(B, C, Ho, Wo), want[j]), j
    for j in range(2):
        buf, out = guarded(rows, cuda)
        call("primia_avg_pool_syft", xd[j], out, B, C, H, W, k, stride, pad)
        assert torch.equal(out, chain[j]), j
        assert np.array_equal(host(out).reshape(B, C, Ho, Wo), want[j]), j
        assert guards_intact(buf, rows)
    (b0, o0), (b1, o1) = guarded(rows, cuda), guarded(rows, cuda)
    call("primia_avg_pool_syft_2p", xd[0], xd[1], o0, o1, B, C, H, W, k, stride, pad)
    assert torch.equal(o0, chain[0]) and torch.equal(o1, chain[1])
    assert guards_intact(b0, rows) and guards_intact(b1, rows)
    # the sums did wrap: the exact (unbounded) window sum of some window lies outside int64
    im0, _ = S.pre_pool(xs[0], k, stride, pad)
    exact = im0.astype(object).sum(axis=-1)
    assert (np.abs(exact) >= 2 ** 63).any()


def test_avg_pool_kernels_refuse_invalid_arguments(cuda):
    x = torch.zeros(1, 2, 8, 8, dtype=I64, device=cuda)
    o = torch.zeros(1, 2, 8, 8, dtype=I64, device=cuda)
    bad = [dict(k=3, stride=2, pad=3), dict(k=3, stride=0, pad=1), dict(k=0, stride=1, pad=0), dict(k=3, stride=2, pad=-1),
           dict(k=11, stride=1, pad=1), dict(B=0), dict(C=0), dict(H=0)]
    for kw in bad:
        a = dict(B=1, C=2, H=8, W=8, k=3, stride=2, pad=1)
        a.update(kw)
        dims = (a["B"], a["C"], a["H"], a["W"], a["k"], a["stride"], a["pad"])
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_avg_pool_syft", x, o, *dims)
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_avg_pool_syft_2p", x, x, o, o.clone(), *dims)
    for args in ((None, o), (x, None), (x, x)):
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_avg_pool_syft", *args, 1, 2, 8, 8, 3, 2, 1)
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
        call("primia_avg_pool_syft_2p", x, x, o, o, 1, 2, 8, 8, 3, 2, 1)      # one output buffer for both parties
    assert not bool(o.any())


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "steps"])
def test_context_avg_pool_on_both_paths(cuda, fused):
    """SecureContext.avg_pool2d_3x3s2 on the in-process (2p kernel) and the step-by-step path (one share per launch, what a
    three-role party runs): the oracle's bits, and nothing asked of the dealer."""
    dealer, ctx = context(cuda, 7, 3, fused)
    dealer.requests = []
    x = torch.randn(2, 6, 11, 11, generator=torch.Generator().manual_seed(3)) * 3
    xs = ctx.share(ctx.encode(x.to(cuda)))
    n = len(dealer.requests)
    out = ctx.avg_pool2d_3x3s2(xs)
    assert len(dealer.requests) == n and ctx.stats == {"beaver_mul": 0, "beaver_matmul": 0, "dif_evals": 0}
    assert tuple(out[0].shape) == (2, 6, 6, 6)
    assert shares_equal(out, oracle_avg_pool([host(s) for s in xs], 3, 2, 1))
    dec = ctx.decode(ctx.reconstruct(out)).cpu()
    # each party truncates its own share: the reconstruction is within 1 unit of the last digit (+ the encoding's) of the pool
    assert float((dec - torch.nn.functional.avg_pool2d(x, 3, 2, 1)).abs().max()) < 3e-3


# ---- 2. whole network, bit-exact ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pf", [3, 16])
@pytest.mark.parametrize("B", [1, 3])
def test_resnet18_avg_bit_exact(cuda, oracle_pool, B, pf):
    """The 8-block ResNet-18 at 32 x 32 with pooling="avg": both output shares equal the oracle forward composed with the avg
    stem on the replayed dealer log, which is consumed exactly; the dealer was asked for what image_requests(pooling="avg")
    lists; 294 element-wise and 21 matrix Beaver products."""
    sd = resnet18(32, 320)
    images = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(321))
    dealer, ctx = context(cuda, 40 + pf + B, pf)
    dealer.requests = []
    model = SecureResNet18(ctx, sd, 32, pooling="avg")
    n_model = len(dealer.requests)
    out = model.forward_shares(ctx.share(ctx.encode(images.to(cuda)), owner=1))
    want = image_requests(architecture_of(sd), 32, B, pooling="avg")
    assert dealer.requests[n_model:] == want and dealer.requests[:n_model] == model_requests(architecture_of(sd))
    assert dealer.requests[n_model:] != image_requests(architecture_of(sd), 32, B)
    octx = S.OracleContext(S.ReplayDealer(dealer.log), 10, pf)
    oout = oracle_forward(octx, numpy_sd(sd), images.numpy(), pooling="avg")
    assert octx.dealer.pos == len(dealer.log)
    assert tuple(out[0].shape) == (B, 3)
    assert shares_equal(out, oout)
    assert ctx.stats["beaver_mul"] == 294 and ctx.stats["beaver_matmul"] == 21
    assert ctx.stats["dif_evals"] == sum(a[0] for kind, a, _ in want if kind == "dif_keys")


def test_unknown_pooling_is_refused(cuda):
    sd = mini_resnet(torch.Generator().manual_seed(21))
    ctx = SecureContext(Dealer(cuda, seed=1), 10, 3)
    with pytest.raises(ValueError, match="pooling"):
        SecureResNet18(ctx, sd, 32, MINI_BLOCKS, pooling="median")
    with pytest.raises(ValueError, match="pooling"):
        GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=3, blocks=MINI_BLOCKS, pooling="AVG")


# ---- 3. it is the avg model, not the max model --------------------------------------------------------------------------
def test_avg_logits_follow_the_avg_plaintext_model(cuda):
    """pf = 3, the 8-block network at 32 x 32 (seed 320) on three images (seed 321): the decoded logits are within PLAIN_TOL of
    oracle.train_oracle.forward(pooling="avg") in float64 on the fixed-point-rounded parameters, and further than PLAIN_TOL
    from the same forward with pooling="max".  The two plaintext forwards differ by 0.53 / 0.86 / 0.71 (max over the
    logits of each image), so the bound separates them.
    The test prints the measured errors (not recorded here yet: no MI355X run of this test has been made)."""
    sd = resnet18(32, 320)
    images = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(321))
    p_avg, p_max = (plaintext_logits(sd, images, 3, 32, p) for p in ("avg", "max"))
    assert np.abs(p_avg - p_max).max(axis=1).min() > 0.1          # (the seeds were chosen for this)
    ctx = SecureContext(Dealer(cuda, seed=43), 10, 3)
    dec = host(SecureResNet18(ctx, sd, 32, pooling="avg")(images.to(cuda))).astype(np.float64)
    err = np.abs(dec - p_avg).max(axis=1)
    print("avg 32x32: max |secure - plaintext avg| per image:", err.tolist(), "vs plaintext max:",
          np.abs(dec - p_max).max(axis=1).tolist(), "logits:", dec.tolist())
    assert (err <= PLAIN_TOL).all(), err
    assert (np.abs(dec - p_max).max(axis=1) > PLAIN_TOL).all()
    # and the max path on the same weights is the other model
    mctx = SecureContext(Dealer(cuda, seed=43), 10, 3)
    dmax = host(SecureResNet18(mctx, sd, 32)(images.to(cuda))).astype(np.float64)
    assert (np.abs(dmax - p_max).max(axis=1) <= PLAIN_TOL).all()
    assert mctx.stats["beaver_mul"] == 298 and ctx.stats["beaver_mul"] == 294


# ---- 4. serving forms ---------------------------------------------------------------------------------------------------
def test_graphed_avg_matches_eager_and_refills(cuda):
    sd = mini_resnet(torch.Generator().manual_seed(21))
    imgs = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(22)).to(cuda)
    pf = 3
    g = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=pf, seed=5, blocks=MINI_BLOCKS, batch=2,
                               pooling="avg")
    assert g.requests[g._n_model:] == image_requests(architecture_of(sd), 32, 2, MINI_BLOCKS, pooling="avg")
    assert g.requests[:g._n_model] == model_requests(architecture_of(sd))
    out_g = g(imgs[:2], refill=False).clone()
    ctx = SecureContext(PreloadedDealer(g.tape, cuda), 10, pf)
    out_e = SecureResNet18(ctx, sd, 32, MINI_BLOCKS, pooling="avg")(imgs[:2])
    assert ctx.dealer.pos == len(g.tape)
    assert tuple(out_g.shape) == (2, 3) and torch.equal(out_g, out_e)
    # not the max network's logits
    mctx = SecureContext(Dealer(cuda, seed=5), 10, pf)
    out_m = SecureResNet18(mctx, sd, 32, MINI_BLOCKS)(imgs[:2])
    assert float((out_m - out_g).abs().max()) > 2 * PLAIN_TOL
    arena = g._arena.clone()
    out_r = g(imgs[:2]).clone()                                       # a second pass, after refill()
    assert g.refills == 2 and int((g._arena == arena).sum()) <= 2
    assert torch.equal(out_r.argmax(dim=1), out_g.argmax(dim=1)) and torch.allclose(out_r, out_g, atol=2 * PLAIN_TOL)
    plain = torch.from_numpy(plaintext_avg_mini(sd, imgs[:2].cpu(), pf)).float()
    assert torch.allclose(out_r.cpu(), plain, atol=PLAIN_TOL) and torch.allclose(out_g.cpu(), plain, atol=PLAIN_TOL)


def plaintext_avg_mini(sd, images, pf):
    """float64 forward of the mini network (tests/secure_batch_nets.py's plain_forward) with the avg stem."""
    F = torch.nn.functional

    def q(v):
        return torch.from_numpy(S.fix_encode(v.numpy(), 10, pf).astype(np.float64) / 10 ** pf)

    p = {k: q(v) for k, v in sd.items() if v.is_floating_point()}

    def bn(t, n):
        sh = (1, -1, 1, 1)
        return (t - p[n + ".running_mean"].view(sh)) / p[n + ".running_var"].view(sh).sqrt() * p[n + ".weight"].view(sh) \
            + p[n + ".bias"].view(sh)

    x = F.relu(bn(F.conv2d(q(images), p["conv1.weight"], stride=2, padding=3), "bn1"))
    x = F.avg_pool2d(x, 3, 2, 1)
    for prefix, stride in MINI_BLOCKS:
        out = F.relu(bn(F.conv2d(x, p[prefix + ".conv1.weight"], stride=stride, padding=1), prefix + ".bn1"))
        out = bn(F.conv2d(out, p[prefix + ".conv2.weight"], stride=1, padding=1), prefix + ".bn2")
        if (prefix + ".downsample.0.weight") in p:
            x = bn(F.conv2d(x, p[prefix + ".downsample.0.weight"], stride=stride), prefix + ".downsample.1")
        x = F.relu(out + x)
    x = x.mean(dim=(2, 3))
    return (x @ p["fc.weight"].t() + p["fc.bias"]).numpy()


def test_pipelined_avg_returns_what_its_slots_return(cuda):
    """PipelinedSecureInference(pooling="avg", batch=2): chunk i comes out as the single-slot serving form produces it from
    the same dealer seed -- slot i % 2 after i // 2 refills -- and each row is the avg model's logits."""
    sd = mini_resnet(torch.Generator().manual_seed(21))
    imgs = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(22)).to(cuda)
    pf = 3
    p = PipelinedSecureInference(sd, cuda, input_size=32, precision_fractional=pf, seed=11, blocks=MINI_BLOCKS, batch=2,
                                 pooling="avg")
    assert all(sl.pooling == "avg" for sl in p.slots)
    index = ([0, 1], [1, 2], [2], [0, 1])
    chunks = [imgs[c[0]:c[-1] + 1] for c in index]
    got = [p(c) for c in chunks]
    torch.cuda.synchronize()
    serial = [GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=pf, seed=11 + 7919 * k, blocks=MINI_BLOCKS,
                                     batch=2, pooling="avg") for k in range(2)]
    for i, c in enumerate(chunks):
        ref = serial[i % 2](c, refill=i >= 2).clone()
        assert torch.equal(got[i], ref), (i, got[i].tolist(), ref.tolist())
    assert tuple(got[2].shape) == (1, 3)
    plain = torch.from_numpy(plaintext_avg_mini(sd, imgs.cpu(), pf)).float()
    for c, rows in zip(index, got):
        assert torch.allclose(rows.cpu(), plain[c], atol=PLAIN_TOL), (c, rows.tolist(), plain[c].tolist())


# ---- 5. three roles -----------------------------------------------------------------------------------------------------
def test_three_role_avg_bit_identical_to_in_process(cuda, tmp_path):
    """model_owner / data_owner / crypto_provider as three processes on one GPU over gloo with pooling="avg" (the parties run
    the single-share kernel, the dealer derives the avg schedule): both parties' decoded logits equal the in-process run's
    under the same debug seed."""
    pf, seed = 3, 5
    want = in_process_logits(cuda, "avg", pf, seed)
    assert not torch.allclose(want[0], want[1], atol=1e-2)
    for j, got in enumerate(three_role_logits("avg", pf, seed, tmp_path)):
        assert torch.equal(got, want), j


# ---- 6. CLI -------------------------------------------------------------------------------------------------------------
def test_cli_serves_the_pooling_the_checkpoint_holds(cuda, tmp_path):
    """inference.py --encrypted_inference on a checkpoint whose pickled args say pooling_type = "avg": the eager form's dumped
    logits are those of SecureResNet18(pooling="avg") under the same debug seed (bit for bit), --hip_graph prints the same
    classes, and the SAME weights saved with pooling_type = "max" give the max path's logits -- there is no flag, the
    checkpoint decides."""
    sd = resnet18(32, 320)
    images = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(0))      # load_images' synthetic set

    def checkpoint(pooling):
        return write_checkpoint(tmp_path / f"net_{pooling}.pt", sd, pooling)

    def run(ckpt, extra, dump):
        r = run_inference(ckpt, 3, 3, ["--encrypted_inference"] + extra, dump=dump)
        return json_line(r)["Inference Results"], torch.load(dump)

    def eager(pooling):
        ctx = SecureContext(Dealer(cuda, seed=7), 10, 3)
        model = SecureResNet18(ctx, sd, 32, pooling=pooling)
        return torch.cat([model(images[i:i + 1].to(cuda)) for i in range(3)]).cpu()

    want_avg, want_max = eager("avg"), eager("max")
    assert float((want_avg - want_max).abs().max()) > 2 * PLAIN_TOL
    classes = {str(i): int(c) for i, c in enumerate(want_avg.argmax(dim=1))}
    c_avg, l_avg = run(checkpoint("avg"), [], str(tmp_path / "avg.pt"))
    c_gr, l_gr = run(checkpoint("avg"), ["--hip_graph"], str(tmp_path / "avg_graph.pt"))
    c_max, l_max = run(checkpoint("max"), [], str(tmp_path / "max.pt"))
    assert torch.equal(l_avg, want_avg) and c_avg == classes
    assert c_gr == classes
    p_avg = plaintext_logits(sd, images, 3, 32, "avg")
    for lg in (l_avg, l_gr):
        assert np.abs(lg.numpy().astype(np.float64) - p_avg).max() <= PLAIN_TOL
    assert torch.equal(l_max, want_max)
    assert c_max == {str(i): int(c) for i, c in enumerate(want_max.argmax(dim=1))}


# ---- 7. full size, once -------------------------------------------------------------------------------------------------
def test_224_resnet18_avg_bit_exact_and_close_to_plaintext(cuda, oracle_pool):
    """One 224 x 224 image, pf = 3, pooling="avg", on the network recipe of tests/test_gpu_secure_batch.py's full-size test
    (reference initialisation under seed 224, every BatchNorm redrawn under seed 225, an N(0, 1) image from the same
    generator): both output shares equal the composed oracle forward on the replayed dealer stream, 2,308,096 comparisons
    (802,816 of them the stem ReLU on the 112 x 112 map), and the decoded logits are within PLAIN_TOL of the float64
    plaintext forward of the avg model.  Its own limit: 15 minutes.
    The test prints the measured error (not recorded here yet: no MI355X run of this test has been made)."""
    with time_limit(900):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(224)
            sd = resnet_spec.init_state_dict(resnet_spec.resnet18_spec(3, 3, 224, "avg"))
        gen = torch.Generator().manual_seed(225)
        for k in [k for k in sd if k.endswith(".running_var")]:
            draw_bn(sd, k[:-len(".running_var")], sd[k].numel(), gen)
        images = torch.randn(1, 3, 224, 224, generator=gen)
        pf = 3
        dealer, ctx = context(cuda, 2243, pf)
        model = SecureResNet18(ctx, sd, 224, pooling="avg")
        out = model.forward_shares(ctx.share(ctx.encode(images.to(cuda)), owner=1))
        assert ctx.stats == {"dif_evals": 2_308_096, "beaver_matmul": 21, "beaver_mul": 294}
        octx = S.OracleContext(S.ReplayDealer(dealer.log), 10, pf)
        oout = oracle_forward(octx, numpy_sd(sd), images.numpy(), pooling="avg")
        assert octx.dealer.pos == len(dealer.log)
        assert shares_equal(out, oout)
        dec = host(ctx.decode(ctx.reconstruct(out))).astype(np.float64)
        plain = plaintext_logits(sd, images, pf, 224, "avg")
        err = np.abs(dec - plain).max()
        print("224 avg: max |secure - plaintext|:", float(err), "logits:", dec.tolist(), "plaintext:", plain.tolist())
        assert np.abs(dec - sd["fc.bias"].numpy()).max() > 0.1
        assert err <= PLAIN_TOL, err
