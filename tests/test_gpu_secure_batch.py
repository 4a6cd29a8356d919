"""GPU: encrypted inference on a BATCH of images per protocol pass.  Every share is held BIT-EXACT to the CPU oracle
replaying the GPU dealer's stream (oracle/secure_oracle.py's OracleContext is written for [B, C, H, W]; the forward is
composed from its methods in tests/secure_batch_nets.py because secure_resnet_forward ends in reshape(1, -1)), on the fused
in-process path and on the step-by-step path a three-role run executes; B = 1 stays what it was."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import secure_oracle as S  # noqa: E402
from oracle import train_oracle as O  # noqa: E402
from primia_amd._lib import call  # noqa: E402
from primia_amd.secure import (Dealer, GraphedSecureInference, PipelinedSecureInference, PreloadedDealer,  # noqa: E402
                               SecureContext, SecureResNet18, architecture_of, image_requests, model_requests)
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet, numpy_sd, oracle_forward, plain_forward, resnet18  # noqa: E402
from tests.secure_common import (I64, PLAIN_TOL, context, host, in_process_logits, json_line, oracle_pool,  # noqa: E402,F401
                                 run_inference, shares_equal, three_role_logits, write_checkpoint)


# ---- 0. the layout kernels on their own ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,HW", [(1, 48, 49), (2, 48, 49), (3, 48, 196), (3, 64, 1024), (2, 5, 33), (4, 130, 7)])
def test_rows_layout_kernels(cuda, B, C, HW):
    """primia_nchw_to_rows is x.permute(1,0,2,3).reshape(C,-1).t() (row b*HW + p), primia_rows_to_nchw its inverse; tiles at
    the ragged edges of C and HW write nothing outside the output (guard words on both sides stay)."""
    rng = np.random.default_rng(B * 1000 + C + HW)
    x = rng.integers(-2 ** 63, 2 ** 63 - 1, size=(B, C, HW), dtype=np.int64)
    want = np.ascontiguousarray(np.transpose(x, (1, 0, 2)).reshape(C, -1).T)
    n, guard = B * C * HW, 64
    buf = torch.full((n + 2 * guard,), 0x5A5A5A5A, dtype=I64, device=cuda)
    rows = buf[guard:guard + n]
    call("primia_nchw_to_rows", torch.from_numpy(x).to(cuda), rows, B, C, HW)
    assert np.array_equal(host(rows).reshape(B * HW, C), want)
    assert bool((buf[:guard] == 0x5A5A5A5A).all()) and bool((buf[guard + n:] == 0x5A5A5A5A).all())
    buf2 = torch.full((n + 2 * guard,), 0x5A5A5A5A, dtype=I64, device=cuda)
    back = buf2[guard:guard + n]
    call("primia_rows_to_nchw", rows, back, B, C, HW)
    assert np.array_equal(host(back).reshape(B, C, HW), x)
    assert bool((buf2[:guard] == 0x5A5A5A5A).all()) and bool((buf2[guard + n:] == 0x5A5A5A5A).all())


# ---- 1. per op, both paths ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "steps"])
@pytest.mark.parametrize("B,C,H", [(2, 48, 7), (3, 48, 7), (2, 48, 14), (3, 48, 14)])
@pytest.mark.parametrize("pf", [3, 16])
def test_batch_norm_eval_of_a_batch_bit_exact(cuda, fused, B, C, H, pf):
    """eval BatchNorm on [B, 48, H, H]: C and H*H are no multiples of the 32 x 32 tile, so every edge of the grid is ragged
    and the tiles of image b end where those of image b + 1 begin.  With the Newton reciprocal inside (inv = None)."""
    dealer, ctx = context(cuda, 100 + B + H + pf, pf, fused)
    g = torch.Generator().manual_seed(B * 10 + H)
    x = torch.randn(B, C, H, H, generator=g) * 2
    bn = dict(mean=torch.randn(C, generator=g) * 0.1, var=torch.rand(C, generator=g) + 0.5,
              weight=torch.rand(C, generator=g) + 0.5, bias=torch.randn(C, generator=g) * 0.1)

    def run(c, enc):
        xs = c.share(enc(x))
        b = {k: c.share(enc(v)) for k, v in bn.items()}
        return c.batch_norm_eval(xs, b["mean"], b["var"], b["weight"], b["bias"])

    gout = run(ctx, lambda v: ctx.encode(v.to(cuda)))
    octx = S.OracleContext(S.ReplayDealer(dealer.log), 10, pf)
    oout = run(octx, lambda v: S.fix_encode(v.numpy(), 10, pf))
    assert octx.dealer.pos == len(dealer.log)
    assert tuple(gout[0].shape) == (B, C, H, H)
    assert shares_equal(gout, oout)
    if pf == 3:
        dec = ctx.decode(ctx.reconstruct(gout)).cpu()
        plain = (x - bn["mean"][None, :, None, None]) / bn["var"].sqrt()[None, :, None, None] \
            * bn["weight"][None, :, None, None] + bn["bias"][None, :, None, None]
        assert float((dec - plain).abs().max()) < 0.05


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "steps"])
@pytest.mark.parametrize("pf", [3, 16])
def test_conv_pool_linear_of_a_batch_bit_exact(cuda, fused, pf):
    """conv2d (3x3 and 1x1, stride 1 and 2), the 9-window max tree, relu, avg_pool2d and linear on B = 3 images."""
    B = 3
    dealer, ctx = context(cuda, 200 + pf, pf, fused)
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, 6, 10, 10, generator=g) * 2
    w = {"c3s1": (torch.randn(10, 6, 3, 3, generator=g) * 0.3, 1, 1), "c3s2": (torch.randn(10, 6, 3, 3, generator=g) * 0.3, 2, 1),
         "c1s1": (torch.randn(10, 6, 1, 1, generator=g) * 0.3, 1, 0), "c1s2": (torch.randn(10, 6, 1, 1, generator=g) * 0.3, 2, 0)}
    fcw, fcb = torch.randn(3, 10, generator=g) * 0.2, torch.randn(3, generator=g) * 0.1

    def run(c, enc):
        xs = c.share(enc(x))
        outs = {}
        for name, (wt, stride, pad) in w.items():
            outs[name] = c.conv2d(xs, c.share(enc(wt)), stride, pad)
        outs["pool"] = c.max_pool2d_3x3s2(xs)
        outs["relu"] = c.relu(outs["c3s1"])
        outs["avg"] = c.avg_pool2d(outs["relu"], 10)
        fw, fb = c.share(enc(fcw)), c.share(enc(fcb))
        outs["fc"] = c.linear([t.reshape(B, -1) for t in outs["avg"]], fw, fb)
        return outs

    gout = run(ctx, lambda v: ctx.encode(v.to(cuda)))
    octx = S.OracleContext(S.ReplayDealer(dealer.log), 10, pf)
    oout = run(octx, lambda v: S.fix_encode(v.numpy(), 10, pf))
    assert octx.dealer.pos == len(dealer.log)
    for k in gout:
        assert shares_equal(gout[k], oout[k]), f"{k} shares differ (pf={pf}, fused={fused})"
    assert tuple(gout["fc"][0].shape) == (B, 3)
    assert ctx.stats["beaver_matmul"] == 5


# ---- 2. whole network ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pf", [16, 3])
def test_resnet18_batch_of_three_bit_exact(cuda, oracle_pool, pf):
    """The 8-block ResNet-18 at 32 x 32 on B = 3 images: both output shares equal the composed oracle forward on the replayed
    log, which is consumed exactly; the comparisons are B times one image's, the 21 matrix products and the element-wise
    Beaver products (Newton's 237, two per BatchNorm, the pool tree's and the ReLUs') are per batch."""
    B = 3
    sd = resnet18(32, 320)
    images = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(321))
    one = SecureContext(Dealer(cuda, seed=1), 10, pf)
    SecureResNet18(one, sd, 32)(images[:1].to(cuda))
    dealer, ctx = context(cuda, 32 + pf, pf, True)
    dealer.requests = []
    model = SecureResNet18(ctx, sd, 32)
    n_model = len(dealer.requests)
    out = model.forward_shares(ctx.share(ctx.encode(images.to(cuda)), owner=1))
    assert dealer.requests[n_model:] == image_requests(architecture_of(sd), 32, B)
    assert dealer.requests[:n_model] == model_requests(architecture_of(sd))
    octx = S.OracleContext(S.ReplayDealer(dealer.log), 10, pf)
    oout = oracle_forward(octx, numpy_sd(sd), images.numpy())
    assert octx.dealer.pos == len(dealer.log)
    assert tuple(out[0].shape) == (B, 3)
    assert shares_equal(out, oout)
    assert ctx.stats == {"dif_evals": B * one.stats["dif_evals"], "beaver_matmul": 21, "beaver_mul": one.stats["beaver_mul"]}
    assert one.stats["beaver_mul"] == 298 and one.stats["beaver_matmul"] == 21


# ---- 3. B = 1 is untouched ----------------------------------------------------------------------------------------------
def test_one_image_keeps_its_schedule_and_its_bits(cuda):
    """A [1, ...] tensor through the batch-general code asks the dealer for exactly what the host-side schedule of ONE image
    lists (the schedule every earlier test and the three-role dealer were built on), whether served eagerly or by
    GraphedSecureInference(batch=1), and the two forms return the same bits."""
    sd = resnet18(32, 320)
    img = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(cuda)
    dealer = Dealer(cuda, seed=77)
    dealer.requests = []
    ctx = SecureContext(dealer, 10, 3)
    model = SecureResNet18(ctx, sd, 32)
    n_model = len(dealer.requests)
    model(img)
    want = image_requests(architecture_of(sd), 32, 1)
    assert dealer.requests[n_model:] == want and dealer.requests[:n_model] == model_requests(architecture_of(sd))
    assert ("triple", ("matmul", (1, 256, 147), (147, 64)), {}) == want[1 + 1 + 79 * 4]
    g = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=3, seed=77)
    assert g.batch == 1 and g.requests[g._n_model:] == want and g._n_model == n_model
    out_g = g(img, refill=False)
    assert out_g is g.out
    ectx = SecureContext(PreloadedDealer(g.tape, cuda), 10, 3)
    out_e = SecureResNet18(ectx, sd, 32)(img)
    assert torch.equal(out_g, out_e) and tuple(out_e.shape) == (1, 3)


# ---- 4. graphed and pipelined forms -------------------------------------------------------------------------------------
def test_graphed_batch_of_two_matches_eager_refills_and_pads(cuda):
    sd = mini_resnet(torch.Generator().manual_seed(21))
    gen = torch.Generator().manual_seed(22)
    imgs = torch.randn(3, 3, 32, 32, generator=gen).to(cuda)
    pf = 3
    g = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=pf, seed=5, blocks=MINI_BLOCKS, batch=2)
    assert g.requests[g._n_model:] == image_requests(architecture_of(sd), 32, 2, MINI_BLOCKS)
    assert g.requests[:g._n_model] == model_requests(architecture_of(sd))
    out_g = g(imgs[:2], refill=False).clone()
    ctx = SecureContext(PreloadedDealer(g.tape, cuda), 10, pf)
    out_e = SecureResNet18(ctx, sd, 32, MINI_BLOCKS)(imgs[:2])
    assert ctx.dealer.pos == len(g.tape)
    assert tuple(out_g.shape) == (2, 3) and torch.equal(out_g, out_e)
    assert not torch.allclose(out_g[0], out_g[1], atol=1e-2)          # two different images: two different rows
    # fresh primitives: other shares (the arena is redrawn), same decoded class, logits up to fixed-point noise
    arena = g._arena.clone()
    out_r = g(imgs[:2]).clone()
    assert int((g._arena == arena).sum()) <= 2
    # (each is within PLAIN_TOL of the plaintext logits, see below: twice that between the two)
    assert torch.equal(out_r.argmax(dim=1), out_g.argmax(dim=1)) and torch.allclose(out_r, out_g, atol=2 * PLAIN_TOL)
    # a short last batch: three images, two per pass -> exactly three rows; the third equals what comes out when it is served
    # in an explicitly padded batch (all-zero second image) on the same primitives
    h = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=pf, seed=5, blocks=MINI_BLOCKS, batch=2)
    rows = [h(imgs[:2]).clone(), h(imgs[2:3]).clone()]      # (the form returns its static buffer: copy before the next pass)
    assert [tuple(r.shape) for r in rows] == [(2, 3), (1, 3)]
    padded = h(torch.cat([imgs[2:3], torch.zeros_like(imgs[:1])]), refill=False).clone()
    assert torch.equal(padded[:1], rows[1])
    assert torch.equal(rows[0], out_r)                               # (same seed, same number of refills before it)
    with pytest.raises(ValueError):
        h(imgs[:3])


@pytest.mark.parametrize("batch", [2, 1])
def test_pipelined_batch_returns_what_its_slots_return(cuda, batch):
    """PipelinedSecureInference(batch=...): image chunks (for batch 2 one of them short) come out exactly as the single-slot
    serving form produces them from the same dealer seeds -- chunk i on slot i % 2 after i // 2 refills -- and every row is
    the image's logits: at three fractional digits a refill that leaves a triple incomplete shows (found here: the zeroing of
    c1 before a split-K product, a memset node of the captured refill graph, was lost on replays once a second instance
    existed, for one image per pass too; at the reference's 16 digits every image decodes to the fc bias and hides it)."""
    sd = mini_resnet(torch.Generator().manual_seed(21))
    imgs = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(22)).to(cuda)
    pf = 3
    p = PipelinedSecureInference(sd, cuda, input_size=32, precision_fractional=pf, seed=11, blocks=MINI_BLOCKS, batch=batch)
    index = ([0, 1], [1, 2], [2], [0, 1]) if batch == 2 else ([0], [1], [2], [0])
    chunks = [imgs[c[0]:c[-1] + 1] for c in index]
    got = [p(c) for c in chunks]
    torch.cuda.synchronize()
    serial = [GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=pf, seed=11 + 7919 * k, blocks=MINI_BLOCKS,
                                     batch=batch) for k in range(2)]
    for i, c in enumerate(chunks):
        ref = serial[i % 2](c, refill=i >= 2).clone()
        assert torch.equal(got[i], ref), (i, got[i].tolist(), ref.tolist())
    assert tuple(got[2].shape) == (1, 3)
    # the three images' float64 plaintext logits; the secure rows within the bound of the deeper 224 network
    plain = torch.from_numpy(plain_forward(sd, imgs.cpu(), MINI_BLOCKS, pf)).float()
    for c, rows in zip(index, got):
        assert torch.allclose(rows.cpu(), plain[c], atol=PLAIN_TOL), (c, rows.tolist(), plain[c].tolist())
    # every triple in the refilled buffers multiplies out
    for g in serial + p.slots:
        for i in range(g._n_model, len(g.tape)):
            kind, args, _ = g.requests[i]
            if kind == "triple":
                op, xs, ys = args
                aa, bb, cc = (S.radd(host(g.tape[i][0][k]), host(g.tape[i][1][k])) for k in range(3))
                want = S.rmul(aa, bb) if op == "mul" else S.rmatmul(aa.reshape(-1, xs[-1]), bb).reshape(cc.shape)
                assert np.array_equal(cc, want), (i, args)


def test_a_batch_that_does_not_fit_is_refused_with_the_largest_that_does(cuda):
    sd = mini_resnet(torch.Generator().manual_seed(21))
    from primia_amd.secure import largest_batch_that_fits, serving_bytes

    arch = architecture_of(sd)
    budget = serving_bytes(arch, 32, 3, MINI_BLOCKS) + 1000
    assert largest_batch_that_fits(arch, 32, budget, MINI_BLOCKS) == 3
    with pytest.raises(ValueError, match="largest batch that fits is 3"):
        GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=3, seed=5, blocks=MINI_BLOCKS, batch=4,
                               memory_budget=budget)
    # the estimate covers what the form holds: primitives on the tape plus the arena
    g = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=3, seed=5, blocks=MINI_BLOCKS, batch=3,
                               memory_budget=budget)
    held = g._arena.numel() * 8
    for (kind, _, _), e in zip(g.requests[g._n_model:], g.tape[g._n_model:]):
        if kind == "dif_keys":
            held += sum(e[0][k].numel() * e[0][k].element_size() for k in ("alpha", "bits", "cw_sigma", "cw_s", "cw_leaf"))
        elif kind == "triple":
            held += e[1][2].numel() * 8                              # c1: the one share outside the arena
    assert held <= g.static_bytes


# ---- 5. full size, once -------------------------------------------------------------------------------------------------


def plaintext_logits(sd, images, pf, size):
    """float64 forward on the fixed-point-rounded parameters and images; the secure BatchNorm has no eps: the reference's
    1e-5 is taken back out of running_var."""
    def q(v):
        return torch.from_numpy(S.fix_encode(v.numpy(), 10, pf).astype(np.float64) / 10 ** pf)

    sd64 = {k: (q(v) if v.is_floating_point() else v) for k, v in sd.items()}
    for k in sd64:
        if k.endswith(".running_var"):
            sd64[k] = sd64[k] - 1e-5
    with torch.no_grad():
        return O.forward(sd64, q(images), training=False, pooling="max", input_size=size).numpy()


def test_224_resnet18_batch_of_two_bit_exact_and_close_to_plaintext(cuda, oracle_pool):
    """B = 2 at 224 x 224, pf = 3, fused path, on the network recipe of tests/test_gpu_secure_fullsize.py (reference
    initialisation under seed 224, every BatchNorm redrawn under seed 225, two N(0, 1) images from the same generator): both
    output shares equal the composed oracle forward on the replayed dealer stream, 2 x 3,311,616 comparisons, and each
    row's decoded logits are within 0.05 of the float64 plaintext forward.  The dealer is seeded (2242), so the checked
    values are fixed: max |secure - plaintext| 0.0038 (row 0, logits -11.336 / 3.664 / 1.524) and 0.0138 (row 1, logits
    -11.244 / 3.553 / 1.529) on an MI355X."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(224)
        from primia_amd import resnet_spec

        sd = resnet_spec.init_state_dict(resnet_spec.resnet18_spec(3, 3, 224, "max"))
    gen = torch.Generator().manual_seed(225)
    from tests.secure_batch_nets import draw_bn

    for k in [k for k in sd if k.endswith(".running_var")]:
        draw_bn(sd, k[:-len(".running_var")], sd[k].numel(), gen)
    images = torch.cat([torch.randn(1, 3, 224, 224, generator=gen) for _ in range(2)])
    pf = 3
    dealer, ctx = context(cuda, 2242, pf, True)
    model = SecureResNet18(ctx, sd, 224)
    out = model.forward_shares(ctx.share(ctx.encode(images.to(cuda)), owner=1))
    octx = S.OracleContext(S.ReplayDealer(dealer.log), 10, pf)
    oout = oracle_forward(octx, numpy_sd(sd), images.numpy())
    assert octx.dealer.pos == len(dealer.log)
    assert shares_equal(out, oout)
    assert ctx.stats == {"dif_evals": 2 * 3_311_616, "beaver_matmul": 21, "beaver_mul": 298}
    dec = host(ctx.decode(ctx.reconstruct(out))).astype(np.float64)
    plain = plaintext_logits(sd, images, pf, 224)
    err = np.abs(dec - plain).max(axis=1)
    print("224 batch of two: max |secure - plaintext| per row:", err.tolist(), "logits:", dec.tolist())
    assert np.abs(dec - sd["fc.bias"].numpy()).max() > 0.1
    assert not np.allclose(dec[0], dec[1], atol=1e-2)
    assert (err <= PLAIN_TOL).all(), err


# ---- 6. three roles -----------------------------------------------------------------------------------------------------
def test_three_role_batch_bit_identical_to_in_process(cuda, tmp_path):
    """model_owner / data_owner / crypto_provider as three processes on one GPU over gloo, two images per protocol pass and a
    padded second pass (three images): both parties' decoded logits equal the in-process run's under the same debug seed."""
    pf, seed = 3, 5
    want = in_process_logits(cuda, "batch", pf, seed)
    assert not torch.allclose(want[0], want[1], atol=1e-2)
    for j, got in enumerate(three_role_logits("batch", pf, seed, tmp_path)):
        assert torch.equal(got, want), j


# ---- 7. CLI -------------------------------------------------------------------------------------------------------------
def test_cli_batch_size(cuda, tmp_path):
    """inference.py --encrypted_inference --batch_size 2 --num_images 3 prints the classes the image-by-image loop prints, in
    the eager and the --hip_graph form, at three fractional digits (where logits depend on the image); the dumped rows are
    within PLAIN_TOL of the float64 plaintext forward -- the bound of the 224 network, which the same eight blocks on 49
    times fewer positions per layer do not exceed -- and agree in class with per-image eager runs on tapes of their own."""
    sd = resnet18(32, 320)
    ckpt = write_checkpoint(tmp_path / "net.pt", sd)

    def run(batch_size, extra, dump):
        r = run_inference(ckpt, 3, 3, ["--encrypted_inference"] + extra, batch_size, dump)
        return json_line(r)["Inference Results"], torch.load(dump)

    one, l_one = run(None, [], str(tmp_path / "one.pt"))
    two, l_two = run(2, [], str(tmp_path / "two.pt"))
    gr, l_gr = run(2, ["--hip_graph"], str(tmp_path / "graph.pt"))
    assert sorted(one) == ["0", "1", "2"] and one == two == gr
    assert l_one.shape == l_two.shape == l_gr.shape == (3, 3)
    images = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(0))      # load_images' synthetic set
    plain = plaintext_logits(sd, images, 3, 32)
    for lg in (l_one, l_two, l_gr):
        assert np.abs(lg.numpy().astype(np.float64) - plain).max() <= PLAIN_TOL
        assert [int(c) for c in lg.argmax(dim=1)] == [one[str(i)] for i in range(3)]
    assert not torch.allclose(l_two[0], l_two[1], atol=1e-2)
    for i in range(3):
        ctx = SecureContext(Dealer(cuda, seed=1000 + i), 10, 3)
        row = SecureResNet18(ctx, sd, 32)(images[i:i + 1].to(cuda)).cpu()
        assert int(row.argmax(dim=1)) == two[str(i)]
