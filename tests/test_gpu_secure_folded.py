"""GPU: encrypted inference on a BatchNorm checkpoint the model owner folded before sharing (primia_amd.secure.fold_batch_norm).
The reference has no such form: a folded norm site is defined in tests/secure_folded_nets.py from the oracle's own methods;
the kernel and whole networks are held BIT-EXACT to that composition, the decoded logits to the float64 plaintext model and
to the plain engine on running variances far outside the Newton domain, in the eager, graphed, three-role and CLI forms."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import secure_oracle as S  # noqa: E402
from primia_amd._lib import PrimiaError, call  # noqa: E402
from primia_amd.engine import ResNet18Engine  # noqa: E402
from primia_amd.secure import (Dealer, GraphedSecureInference, PreloadedDealer, SecureContext, SecureResNet18,  # noqa: E402
                               architecture_of, fold_batch_norm, image_requests, model_requests, serving_bytes)
from tests.secure_batch_nets import MINI_BLOCKS, numpy_sd  # noqa: E402
from tests.secure_common import (I64, PLAIN_TOL, context, guarded, guards_intact, host, host_ptrs, in_process_logits,  # noqa: E402,F401
                                 json_line, oracle_pool, run_inference, shares_equal, three_role_logits, time_limit,
                                 wrapping_shares, write_checkpoint)
from tests.secure_folded_nets import (FOLDED_TOL, oracle_affine_eval, oracle_folded_forward, plaintext_logits,  # noqa: E402
                                      wide_mini, wide_resnet18)
from tests.secure_groupnorm_nets import group_resnet18  # noqa: E402


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
# ragged channel and pixel tiles, a single pixel, several tiles, several planes
SHAPES = [(1, 8, 1), (1, 40, 49), (3, 40, 49), (1, 64, 1024), (2, 96, 33)]


@pytest.mark.parametrize("pf", [3, 6])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_affine_eval_kernel_equals_the_chain(cuda, shape, pf):
    """primia_affine_eval_local / _batch against _to_rows, fpt_mul, add, rows_to_nchw on the same triple, bit for bit for both
    parties, on shares near +-2^63 (products and sums wrap, truncation meets the most negative value); the chain is
    oracle_affine_eval on the same primitives; nothing is written outside the outputs."""
    B, C, HW = shape
    rng = np.random.default_rng(1000 * C + HW + pf)
    dev = lambda a: torch.from_numpy(a).to(cuda)
    xs = [dev(wrapping_shares(rng, (B, C, HW, 1))) for _ in range(2)]
    scale = [dev(wrapping_shares(rng, (C,))) for _ in range(2)]
    shift = [dev(wrapping_shares(rng, (C,))) for _ in range(2)]
    dealer = Dealer(cuda, seed=40 + pf)
    dealer.log = []
    t = dealer.triple("mul", (B * HW, C), (C,))
    chain_ctx = SecureContext(PreloadedDealer([t], cuda), 10, pf)
    chain_ctx.local_fused = False
    chain = chain_ctx.affine_eval(xs, scale, shift)
    assert chain_ctx.dealer.pos == 1 and chain_ctx.stats["beaver_mul"] == 1
    octx = S.OracleContext(S.ReplayDealer(dealer.log), 10, pf)
    want = oracle_affine_eval(octx, [host(v) for v in xs], [host(v) for v in scale], [host(v) for v in shift])
    assert octx.dealer.pos == 1 and shares_equal(chain, want)
    n = B * C * HW
    (b0, o0), (b1, o1) = guarded(n, cuda), guarded(n, cuda)
    if B == 1:
        call("primia_affine_eval_local", xs[0], xs[1], scale[0], scale[1], shift[0], shift[1], host_ptrs(t), o0, o1, C, HW,
             10 ** pf)
    else:
        call("primia_affine_eval_local_batch", xs[0], xs[1], scale[0], scale[1], shift[0], shift[1], host_ptrs(t), o0, o1, B, C,
             HW, 10 ** pf)
    assert guards_intact(b0, n) and guards_intact(b1, n)
    assert torch.equal(o0.view(B, C, HW, 1), chain[0]) and torch.equal(o1.view(B, C, HW, 1), chain[1])
    # the batch entry point with one plane is the single-image one; the context's fused path is the kernel
    fused_ctx = SecureContext(PreloadedDealer([t], cuda), 10, pf)
    fused = fused_ctx.affine_eval(xs, scale, shift)
    assert fused_ctx.stats["beaver_mul"] == 1 and torch.equal(fused[0], chain[0]) and torch.equal(fused[1], chain[1])
    if B == 1:
        (c0, p0), (c1, p1) = guarded(n, cuda), guarded(n, cuda)
        call("primia_affine_eval_local_batch", xs[0], xs[1], scale[0], scale[1], shift[0], shift[1], host_ptrs(t), p0, p1, 1,
             C, HW, 10 ** pf)
        assert guards_intact(c0, n) and guards_intact(c1, n) and torch.equal(p0, o0) and torch.equal(p1, o1)


def test_affine_eval_kernel_refuses_invalid_arguments(cuda):
    C, HW = 40, 6
    z = lambda *s: torch.zeros(*s, dtype=I64, device=cuda)
    t = [z(HW, C), z(C), z(HW, C)] * 2
    arr = lambda ts: (ctypes.c_void_p * 6)(*[q.data_ptr() for q in ts])
    good = [z(C, HW), z(C, HW), z(C), z(C), z(C), z(C), arr(t), z(C, HW), z(C, HW), C, HW, 1000]
    call("primia_affine_eval_local", *good)
    for i in range(9):
        bad = list(good)
        bad[i] = None
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_affine_eval_local", *bad)
    bad = list(good)
    bad[6] = (ctypes.c_void_p * 6)(*[t[0].data_ptr()] * 5, None)
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
        call("primia_affine_eval_local", *bad)
    bad = list(good)
    bad[8] = bad[7]                                                   # one buffer for both parties' outputs
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
        call("primia_affine_eval_local", *bad)
    for i in (9, 10, 11):                                             # C, HW, div
        bad = list(good)
        bad[i] = 0
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_affine_eval_local", *bad)
    batch = good[:9] + [1, C, HW, 1000]
    call("primia_affine_eval_local_batch", *batch)
    for b in (0, 65536):
        bad = list(batch)
        bad[9] = b
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_affine_eval_local_batch", *bad)


# ---- 2. whole networks, bit exact -------------------------------------------------------------------------------------------
def networks():
    return {"mini": (wide_mini(torch.Generator().manual_seed(41)), MINI_BLOCKS, 6), "resnet18": (wide_resnet18(32, 720), None, 20)}


@pytest.mark.parametrize("pf", [3, 6])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("net", ["mini", "resnet18"])
def test_folded_network_bit_exact(cuda, oracle_pool, net, B, pf):  # noqa: F811
    """SecureResNet18 on a folded dict: both logit shares equal oracle_folded_forward on the replayed dealer log, which is
    consumed exactly; the dealer was asked for model_requests + image_requests of the folded architecture; the step-by-step
    form asks for the same and gives the same bits; the counters are those of the list (no Newton product)."""
    sd, blocks, sites = networks()[net]
    folded = fold_batch_norm(sd)
    arch = architecture_of(folded)
    images = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(721))
    outs = []
    for fused in (True, False):
        dealer, ctx = context(cuda, 70 + pf + B, pf, fused)
        dealer.requests = []
        model = SecureResNet18(ctx, folded, 32, blocks)
        assert model.norm == "folded"
        n_model = len(dealer.requests)
        outs.append(model.forward_shares(ctx.share(ctx.encode(images.to(cuda)), owner=1)))
        want = image_requests(arch, 32, B, blocks)
        assert dealer.requests == model_requests(arch) + want and n_model == len(arch)
        muls = sum(1 for k, a, _ in want if k == "triple" and a[0] == "mul")
        assert ctx.stats["beaver_mul"] == muls
        assert sum(1 for k, a, _ in want if k == "triple" and a[0] == "mul" and len(a[2]) == 1) == sites
        assert ctx.stats["beaver_matmul"] == sum(1 for k, a, _ in want if k == "triple" and a[0] == "matmul")
        assert ctx.stats["dif_evals"] == sum(a[0] for k, a, _ in want if k == "dif_keys")
        if fused:
            log = dealer.log
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    octx = S.OracleContext(S.ReplayDealer(log), 10, pf)
    oout = oracle_folded_forward(octx, numpy_sd(folded), images.numpy(), blocks)
    assert octx.dealer.pos == len(log)
    assert tuple(outs[0][0].shape) == (B, 3)
    assert shares_equal(outs[0], oout)
    # the unfolded checkpoint still takes the reference's path, down to the request list
    assert image_requests(architecture_of(sd), 32, B, blocks) != want


# ---- 3. graphed ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reveal", ["logits", "class"])
def test_graphed_folded_matches_eager_across_a_refill(cuda, reveal):
    """GraphedSecureInference on the folded mini network: the replay equals the eager model fed the same tape, bit for bit,
    before and after a refill; the static bytes are those of the folded list, fewer than the unfolded dict's."""
    sd = wide_mini(torch.Generator().manual_seed(41))
    folded = fold_batch_norm(sd)
    imgs = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(42)).to(cuda)
    pf, B = 3, 2
    g = GraphedSecureInference(folded, cuda, input_size=32, precision_fractional=pf, seed=5, blocks=MINI_BLOCKS, batch=B,
                               reveal=reveal)
    arch = architecture_of(folded)
    assert g.requests == model_requests(arch) + image_requests(arch, 32, B, MINI_BLOCKS, reveal=reveal)
    assert g.static_bytes == serving_bytes(arch, 32, B, MINI_BLOCKS, reveal=reveal)
    assert g.static_bytes < serving_bytes(architecture_of(sd), 32, B, MINI_BLOCKS, reveal=reveal)
    seen = []
    for step in range(2):
        chunk = imgs[step:step + B]
        out_g = g(chunk, refill=step > 0).clone()
        ctx = SecureContext(PreloadedDealer(g.tape, cuda), 10, pf)
        out_e = SecureResNet18(ctx, folded, 32, MINI_BLOCKS, reveal=reveal)(chunk)
        assert ctx.dealer.pos == len(g.tape)
        assert tuple(out_g.shape) == ((B, 3) if reveal == "logits" else (B,)) and torch.equal(out_g, out_e), step
        seen.append(g._arena.clone())
    assert g.refills == 2 and int((seen[0] == seen[1]).sum()) <= 2


# ---- 4. three roles -----------------------------------------------------------------------------------------------------------
def test_three_role_folded_bit_identical_to_in_process(cuda, tmp_path):
    """model_owner / data_owner / crypto_provider as three processes on one GPU over gloo (tests/party_worker.py): rank 0 folds
    the weights, the other two the architecture alone; both parties' decoded logits equal the in-process run's under the
    same debug seed."""
    pf, seed = 3, 5
    with time_limit(600):
        want = in_process_logits(cuda, "folded", pf, seed)
        assert not torch.allclose(want[0], want[1], atol=1e-2)
        for j, got in enumerate(three_role_logits("folded", pf, seed, tmp_path)):
            assert torch.equal(got, want), j


# ---- 5. it is the plaintext model, for any statistics ----------------------------------------------------------------------------
def test_folded_logits_follow_the_plain_engine_on_wide_variances(cuda):
    """pf = 6, 64-bit comparisons, the 8-block network at 32 x 32 with running variances from 1e-3 to 30 (seed 720), the two
    images of the CPU measurement (seed 721), dealer seed 1: the folded encrypted logits are within FOLDED_TOL of the float64
    plaintext model (the CPU composition measured at most half of it under three dealer seeds; an MI355X run of this test
    measured 4.17e-5) and within FOLDED_TOL + PLAIN_TOL of ResNet18Engine's fp32 eval logits on the unfolded checkpoint
    (measured: 1.3e-3), with the same argmax."""
    pf = 6
    sd = wide_resnet18(32, 720)
    images = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(721))
    ctx = SecureContext(Dealer(cuda, seed=1, fss_bits=64), 10, pf)
    dec = host(SecureResNet18(ctx, fold_batch_norm(sd), 32)(images.to(cuda))).astype(np.float64)
    plain = plaintext_logits(sd, images, pf, 32)
    eng = ResNet18Engine(1, 3, 3, 32, "max", dtype=torch.float32, device=cuda)
    eng.load_state_dict(sd)
    eng.eval()
    fp32 = np.concatenate([host(eng.forward(images[i:i + 1].to(cuda)).float()) for i in range(2)]).astype(np.float64)
    err, err_eng = np.abs(dec - plain).max(), np.abs(dec - fp32).max()
    print("folded 32x32, wide variances: max |secure - float64 plaintext|", err, "max |secure - engine fp32|", err_eng,
          "logits", dec.tolist(), "engine", fp32.tolist())
    assert err <= FOLDED_TOL, err
    assert err_eng <= FOLDED_TOL + PLAIN_TOL, err_eng
    assert (dec.argmax(axis=1) == fp32.argmax(axis=1)).all()


# ---- 6. CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli_fold_norm(cuda, tmp_path):
    """inference.py --encrypted_inference --fold_norm on the wide-variance checkpoint prints the classes the plain run of the
    same command prints (the plain path keeps the unfolded checkpoint; with it the flag only warns), --hip_graph too; a
    GroupNorm checkpoint is refused with the reason."""
    def checkpoint(name, state):
        return write_checkpoint(tmp_path / f"{name}.pt", state)

    def run(ckpt, extra):
        return run_inference(ckpt, 3, 6, ["--fss_bits", "64", "--fold_norm"] + extra)

    def classes(r):
        return json_line(r)["Inference Results"]

    ckpt = checkpoint("wide", wide_resnet18(32, 720))
    plain = run(ckpt, [])
    assert "--fold_norm has no effect" in plain.stderr
    want = classes(plain)
    assert len(want) == 3
    enc = run(ckpt, ["--encrypted_inference"])
    assert "--fold_norm has no effect" not in enc.stderr
    assert classes(enc) == want
    assert classes(run(ckpt, ["--encrypted_inference", "--hip_graph"])) == want
    refused = run(checkpoint("gn", group_resnet18(32, 520)), ["--encrypted_inference"])
    assert refused.returncode != 0 and "statistics depend on the image" in refused.stderr
