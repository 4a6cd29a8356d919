"""GPU: the wide-range secret-shared GroupNorm (SecureContext.group_norm(wide=True), inference.py --wide_norm).  The layer is
defined in tests/secure_gn_wide_nets.py from the oracle's own methods; the new entry points, the fused iteration, the
step-by-step chain and whole networks are held BIT-EXACT to that composition, the decoded logits to the float64 plaintext
forward within twice what the CPU composition measured, in the eager, graphed, three-role and CLI forms."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import secure_oracle as S  # noqa: E402
from primia_amd._lib import PrimiaError, call, query  # noqa: E402
from primia_amd.secure import (GN_WIDE_FLOOR, GN_WIDE_SCALE, GN_WIDE_STEPS, GN_WIDE_X0, Dealer,  # noqa: E402
                               GraphedSecureInference, PreloadedDealer, SecureContext, SecureResNet18, architecture_of,
                               image_requests, model_requests, serving_bytes)
from tests import secure_gn_wide_nets as W  # noqa: E402
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet, numpy_sd  # noqa: E402
from tests.secure_common import (context, guarded, guards_intact, host, host_ptrs, json_line,  # noqa: E402,F401
                                 oracle_pool, run_inference, shares_equal, six, three_roles, write_checkpoint)
from tests.three_role_cases import CASES  # noqa: E402
from tests.secure_groupnorm_nets import VAR_DOMAIN, default_blocks, plain_group_forward  # noqa: E402

SHAPES = [(1, 64, 6, 6), (3, 64, 5, 5), (2, 128, 4, 4)]      # (3, 64, 5, 5): m = 50, R = 96, two workgroups of the iteration
FIRST_DIV = 2 * GN_WIDE_SCALE ** 3 // GN_WIDE_X0 ** 3
EPS_Q = GN_WIDE_SCALE // 100000 + GN_WIDE_FLOOR
SITE = 4 * (GN_WIDE_STEPS - 1) + 4                            # dealer requests of one norm site


def layer_input(shape, pf, seed):
    """x whose group standard deviations spread geometrically over 0.05 .. 60 (pf 6: .. 8), every group off centre, group 3
    constant; weight, bias."""
    B, C, H, Wd = shape
    R = B * 32
    gen = torch.Generator().manual_seed(seed)
    std = torch.from_numpy(np.geomspace(0.05, 60.0 if pf < 6 else 8.0, R)).float()[torch.randperm(R, generator=gen)]
    x = torch.randn(R, C // 32 * H * Wd, generator=gen) * std[:, None] + torch.randn(R, 1, generator=gen)
    x[3] = -1.25
    return x.reshape(shape), torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.1


# ---- 1. the pieces ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pf", [3, 6])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wide_kernels_equal_the_chain_and_the_oracle(cuda, shape, pf):
    """The step-by-step chain of group_norm(wide=True) gives oracle_group_norm_wide's shares on the replayed dealer log
    (consumed exactly); primia_gn_moments_wide_local, primia_rsqrt_newton_local and primia_gn_apply_wide_local on the
    primitives the chain consumed give the chain's shares and write nothing outside their outputs; so does the fused
    context as a whole, asking the dealer for the same list."""
    B, C, H, Wd = shape
    R, m, HW = B * 32, (C // 32) * H * Wd, H * Wd
    x, w, b = layer_input(shape, pf, C * 100 + H * 10 + pf)
    dealer, ctx = context(cuda, 700 + pf, pf, fused=False)
    xs, ws, bs = (ctx.share(ctx.encode(t.to(cuda))) for t in (x, w, b))
    dealer.tape, dealer.requests = [], []
    chain = ctx.group_norm(xs, ws, bs, wide=True)
    tape, dealer.tape = dealer.tape, None
    assert len(tape) == SITE and ctx.stats["beaver_mul"] == 3 + 3 * (GN_WIDE_STEPS - 1)
    assert [(k, a) for k, a, _ in dealer.requests] == W.wide_site_requests(R, m, B * HW, C)
    octx = S.OracleContext(S.ReplayDealer(dealer.log), 10, pf)
    want = W.oracle_group_norm_wide(octx, *[octx.share(S.fix_encode(t.numpy(), 10, pf)) for t in (x, w, b)])
    assert octx.dealer.pos == len(dealer.log)
    assert shares_equal(chain, want)
    # the entry points on the same primitives
    bufs = [guarded(R, cuda) for _ in range(4)]
    call("primia_gn_moments_wide_local", xs[0], xs[1], *six(tape[0]), *[v for _, v in bufs], None, R, m,
         ctx.scale * ctx.scale // GN_WIDE_SCALE)
    assert all(guards_intact(buf, R) for buf, _ in bufs)
    mean, var = [bufs[0][1], bufs[1][1]], [bufs[2][1], bufs[3][1]]
    pctx = SecureContext(PreloadedDealer(tape[1:-2], cuda), 10, pf)
    inv = pctx.rsqrt_newton(pctx.sub_public_scalar(var, -EPS_Q))
    assert pctx.dealer.pos == SITE - 3
    (b0, o0), (b1, o1) = guarded(x.numel(), cuda), guarded(x.numel(), cuda)
    call("primia_gn_apply_wide_local", xs[0], xs[1], mean[0], mean[1], inv[0], inv[1], ws[0], ws[1], bs[0], bs[1],
         host_ptrs(tape[-2]), host_ptrs(tape[-1]), o0, o1, B, C, HW, 32, GN_WIDE_SCALE, ctx.scale)
    assert guards_intact(b0, x.numel()) and guards_intact(b1, x.numel())
    assert torch.equal(o0.view(shape), chain[0]) and torch.equal(o1.view(shape), chain[1])
    # the fused context, fed the same primitives
    fctx = SecureContext(PreloadedDealer(tape, cuda), 10, pf)
    fused = fctx.group_norm(xs, ws, bs, wide=True)
    assert fctx.dealer.pos == SITE and fctx.stats == ctx.stats
    assert torch.equal(fused[0], chain[0]) and torch.equal(fused[1], chain[1])
    # a live fused context asks for the same list
    d2, c2 = context(cuda, 700 + pf, pf, fused=True)
    d2.requests = []
    xs2, ws2, bs2 = (c2.share(c2.encode(t.to(cuda))) for t in (x, w, b))
    live = c2.group_norm(xs2, ws2, bs2, wide=True)
    assert d2.requests[3:] == dealer.requests
    assert torch.equal(live[0], chain[0]) and torch.equal(live[1], chain[1])
    # the input leaves the default form's window on both sides (the error against float64 is the host tests' subject: the
    # shares above ARE the composition's)
    q = torch.from_numpy(S.fix_encode(x.numpy(), 10, pf).astype(np.float64) / 10 ** pf)
    var64 = q.reshape(R, -1).var(dim=1, unbiased=False)
    assert float(var64.max()) > VAR_DOMAIN[1] and float(var64[var64 > 1e-9].min()) < VAR_DOMAIN[0] and float(var64[3]) < 1e-9


@pytest.mark.parametrize("n", [5, 96, 200])
def test_rsqrt_newton_fused_equals_chain_equals_oracle(cuda, n):
    """SecureContext.rsqrt_newton on n values from 1e-5 to 2.9e4 (n = 200: four workgroups, the last ragged): the fused launch
    and the chain ask the dealer for the same primitives and give the same shares, which are oracle_rsqrt_newton's on the
    replayed log (whose error against v^-1/2 the host tests measure).  Below the served range the squares of the iterates
    approach the ring's headroom (x^2 s_it^2 = s_it^2 / v) and a per-share truncation may fail: the bits agree there too."""
    v = np.geomspace(1e-5, 2.9e4, n)
    q = torch.from_numpy(np.round(v * GN_WIDE_SCALE).astype(np.int64)).to(cuda)
    outs, reqs, logs = [], [], []
    for fused in (True, False):
        dealer, ctx = context(cuda, 33, 3, fused)
        dealer.requests = []
        outs.append(ctx.rsqrt_newton(ctx.share(q)))
        reqs.append(dealer.requests)
        logs.append(dealer.log)
        assert ctx.stats["beaver_mul"] == 3 * (GN_WIDE_STEPS - 1)
    assert reqs[0] == reqs[1] and len(reqs[0]) == 1 + 4 * (GN_WIDE_STEPS - 1)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    octx = S.OracleContext(S.ReplayDealer(logs[1]), 10, 3)
    want = W.oracle_rsqrt_newton(octx, octx.share(host(q)))
    assert octx.dealer.pos == len(logs[1])
    assert shares_equal(outs[0], want)


# ---- 2. invalid arguments ---------------------------------------------------------------------------------------------------
def test_wide_entry_points_refuse_invalid_arguments(cuda):
    R, m, C, HW, T = 32, 8, 64, 4, 3
    z = lambda *s: torch.zeros(*s, dtype=torch.int64, device=cuda)
    x, t, o = [z(R, m), z(R, m)], [z(R, m) for _ in range(6)], [z(R) for _ in range(4)]
    good = [x[0], x[1], *t, *o, None, R, m, 1]
    call("primia_gn_moments_wide_local", *good)
    for i, val in [(i, None) for i in range(12)] + [(13, 0), (14, 0), (15, 0), (15, -1), (14, 2048)]:
        bad = list(good)
        bad[i] = val
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_gn_moments_wide_local", *bad)
    prims = [z(R) for _ in range(19 * (T - 1))]
    table = torch.tensor([p.data_ptr() for p in prims], dtype=torch.int64).to(cuda)
    v, out = [z(R) + 5, z(R)], [z(R), z(R)]
    good = [v[0], v[1], table, GN_WIDE_SCALE, GN_WIDE_X0, FIRST_DIV, T, out[0], out[1], R]
    call("primia_rsqrt_newton_local", *good)
    call("primia_rsqrt_newton_local", *(good[:2] + [None] + good[3:6] + [1] + good[7:]))      # one iterate: no primitives
    for i, val in [(0, None), (1, None), (2, None), (7, None), (8, None), (8, out[0]), (3, 0), (4, 0), (5, 0), (6, 0), (9, 0), (9, -4)]:
        bad = list(good)
        bad[i] = val
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_rsqrt_newton_local", *bad)
    vec = [z(R) for _ in range(4)] + [z(C) for _ in range(4)]
    t1, t2 = [z(R), z(m, R), z(m, R)] * 2, [z(HW, C), z(C), z(HW, C)] * 2
    arr = lambda ts: (ctypes.c_void_p * 6)(*[p.data_ptr() for p in ts])
    o2 = [z(1, C, 2, 2), z(1, C, 2, 2)]
    good = [x[0], x[1], *vec, arr(t1), arr(t2), o2[0], o2[1], 1, C, HW, 32, GN_WIDE_SCALE, 1000]
    call("primia_gn_apply_wide_local", *good)
    hole = (ctypes.c_void_p * 6)(*[t1[0].data_ptr()] * 5, None)
    for i, val in [(i, None) for i in list(range(10)) + [12, 13]] + [(10, hole), (11, hole), (13, o2[0])] + \
            [(i, 0) for i in (14, 15, 16, 17, 18, 19)]:
        bad = list(good)
        bad[i] = val
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_gn_apply_wide_local", *bad)
    bad = list(good)
    bad[17] = 24
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_UNSUPPORTED"):
        call("primia_gn_apply_wide_local", *bad)
    assert query("primia_gn_moments_local_scratch_elems", R, m) == 0


def test_wide_norm_is_refused_where_it_is_not_defined(cuda):
    gn, blocks = W.wide_networks()["mini"]
    bn = mini_resnet(torch.Generator().manual_seed(21))
    ctx = SecureContext(Dealer(cuda, seed=1), 10, 3)
    assert SecureResNet18(ctx, gn, 32, blocks, wide_norm=True).wide_norm
    with pytest.raises(ValueError, match="fold_norm"):
        SecureResNet18(ctx, bn, 32, blocks, wide_norm=True)
    with pytest.raises(ValueError, match="fold_norm"):
        GraphedSecureInference(bn, cuda, input_size=32, precision_fractional=3, seed=1, blocks=blocks, wide_norm=True)
    for pf in (2, 16):
        with pytest.raises(ValueError, match="precision_fractional"):
            SecureResNet18(SecureContext(Dealer(cuda, seed=1), 10, pf), gn, 32, blocks, wide_norm=True)
    z = lambda *s: torch.zeros(*s, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match="precision_fractional"):
        SecureContext(Dealer(cuda, seed=1), 10, 16).group_norm([z(1, 64, 2, 2)] * 2, [z(64)] * 2, [z(64)] * 2, wide=True)


# ---- 3. whole networks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rows", [("mini", slice(2, 3)), ("resnet18", slice(0, 1))], ids=["mini", "resnet18"])
def test_wide_network_bit_exact(cuda, oracle_pool, name, rows):
    """Both logit shares of the network with wide_norm=True equal oracle_forward with oracle_group_norm_wide at every norm site
    on the replayed dealer log, which is consumed exactly; the dealer was asked for image_requests(wide_norm=True).  One image
    each (the oracle's comparisons are the test's time): the one scaled by 6 on the mini network, the one scaled by 0.15 on the
    ResNet-18; batches are the subject of the kernel, graphed and three-role tests."""
    sd, blocks = W.wide_networks()[name]
    images = W.spread_images()[rows]
    B = len(images)
    dealer, ctx = context(cuda, 90 + B, 3)
    dealer.requests = []
    model = SecureResNet18(ctx, sd, 32, blocks, wide_norm=True)
    n_model = len(dealer.requests)
    out = model.forward_shares(ctx.share(ctx.encode(images.to(cuda)), owner=1))
    arch = architecture_of(sd)
    want = image_requests(arch, 32, B, blocks, wide_norm=True)
    assert dealer.requests[n_model:] == want and dealer.requests[:n_model] == model_requests(arch)
    assert want != image_requests(arch, 32, B, blocks)
    octx = S.OracleContext(S.ReplayDealer(dealer.log), 10, 3)
    oout = W.oracle_forward_wide(octx, numpy_sd(sd), images.numpy(), blocks)
    assert octx.dealer.pos == len(dealer.log)
    assert shares_equal(out, oout)
    assert ctx.stats["beaver_mul"] == sum(1 for k, a, _ in want if k == "triple" and a[0] == "mul")


@pytest.mark.parametrize("name", ["mini", "resnet18"])
def test_wide_logits_follow_the_plaintext_model_outside_the_default_window(cuda, name):
    """pf = 3, three images scaled by 0.15, 1 and 6 on a network with three convolutions scaled: group variances of the float64
    forward leave [0.05, 16] on both sides (asserted on the reference).  The decoded logits of the wide form are within
    WIDE_NET_TOL of the float64 forward -- twice what the CPU composition measured on ChaChaDealer(57), the host twin of this
    dealer (tests/secure_gn_wide_nets.py) -- and those of the default form are not."""
    sd, blocks = W.wide_networks()[name]
    images = W.spread_images()
    variances = []
    plain = plain_group_forward(sd, images, blocks or default_blocks(), 3, "max", variances)
    lo, hi = min(float(v.min()) for v in variances), max(float(v.max()) for v in variances)
    assert lo < VAR_DOMAIN[0] / 2 and hi > 2 * VAR_DOMAIN[1] and hi < W.VAR_SERVED[1], (lo, hi)
    ctx = SecureContext(Dealer(cuda, seed=W.NET_DEALER_SEED), 10, 3)
    dec = host(SecureResNet18(ctx, sd, 32, blocks, wide_norm=True)(images.to(cuda))).astype(np.float64)
    err = np.abs(dec - plain).max(axis=1)
    print(name, "wide: max |secure - plaintext| per image:", err.tolist(), "group variances", lo, "to", hi)
    assert (err <= W.WIDE_NET_TOL[name]).all(), err
    ctx = SecureContext(Dealer(cuda, seed=W.NET_DEALER_SEED), 10, 3)
    old = host(SecureResNet18(ctx, sd, 32, blocks)(images.to(cuda))).astype(np.float64)
    assert np.abs(old - plain).max() > 1.0


# ---- 4. serving forms -------------------------------------------------------------------------------------------------------
def test_graphed_wide_matches_eager_on_two_image_sets(cuda):
    """GraphedSecureInference(wide_norm=True) on the mini network, batch 2: ONE captured graph replayed on two different image
    pairs (and a refill between) equals the eager forward on the same static primitives, bit for bit; the pointer tables of
    the six iterations are built once."""
    sd, blocks = W.wide_networks()["mini"]
    imgs = W.spread_images().to(cuda)
    g = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=3, seed=5, blocks=blocks, batch=2, wide_norm=True)
    arch = architecture_of(sd)
    assert g.requests[g._n_model:] == image_requests(arch, 32, 2, blocks, wide_norm=True)
    assert g.static_bytes == serving_bytes(arch, 32, 2, blocks, wide_norm=True) < serving_bytes(arch, 32, 2, blocks)
    graph, tables = g.graph, [t for _, t in g._ctx._newton_tables]
    assert len(tables) == 6
    results = []
    for step, pair in enumerate((imgs[0:2], imgs[1:3])):
        out_g = g(pair, refill=step > 0).clone()
        ctx = SecureContext(PreloadedDealer(g.tape, cuda), 10, 3)
        out_e = SecureResNet18(ctx, sd, 32, blocks, wide_norm=True)(pair)
        assert ctx.dealer.pos == len(g.tape)
        assert tuple(out_g.shape) == (2, 3) and torch.equal(out_g, out_e), step
        results.append(out_g)
    assert g.graph is graph and all(a is b for a, (_, b) in zip(tables, g._ctx._newton_tables))
    assert not torch.equal(results[0], results[1])


def test_three_role_wide_bit_identical_to_in_process(cuda, tmp_path):
    """model_owner / data_owner / crypto_provider as three processes on one GPU over gloo (the "gn-wide" case of
    tests/three_role_cases.py through the suite's worker and launcher): the parties run the wide form's step-by-step chain, the dealer follows
    image_requests(wide_norm=True); both parties' logits equal the in-process run's under the same debug seed."""
    pf, seed, batch = 3, 5, CASES["gn-wide"].batch
    assert batch == 2
    sd, blocks = W.wide_networks()["mini"]
    images = W.spread_images()
    dealer = Dealer(cuda, seed=seed)
    dealer.requests = []
    model = SecureResNet18(SecureContext(dealer, 10, pf), sd, 32, blocks, wide_norm=True)
    dv = images.to(cuda)
    pad = torch.cat([dv[2:3], torch.zeros_like(dv[:1])])
    want = torch.cat([model(dv[0:2]), model(pad)[:1]]).cpu()
    arch = architecture_of(sd)
    assert dealer.requests == model_requests(arch) + 2 * image_requests(arch, 32, batch, blocks, wide_norm=True)
    out = str(tmp_path / "logits")
    three_roles("gn-wide", pf, seed, out)
    for j in range(2):
        assert torch.equal(torch.load(f"{out}.{j}"), want), j


# ---- 5. CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_wide_norm(cuda, tmp_path):
    """inference.py --encrypted_inference --wide_norm dumps the logits of SecureResNet18(wide_norm=True) under the same debug
    seed bit for bit; on a BatchNorm checkpoint the run ends naming --fold_norm."""
    sd, _ = W.wide_networks()["resnet18"]
    images = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(0))      # load_images' synthetic set
    ctx = SecureContext(Dealer(cuda, seed=7), 10, 3)
    model = SecureResNet18(ctx, sd, 32, wide_norm=True)
    want = torch.cat([model(images[i:i + 1].to(cuda)) for i in range(2)]).cpu()
    dump = str(tmp_path / "wide.pt")
    r = run_inference(write_checkpoint(tmp_path / "gn.pt", sd), 2, 3, ["--encrypted_inference", "--wide_norm"], dump=dump)
    classes = json_line(r)["Inference Results"]
    assert torch.equal(torch.load(dump), want)
    assert classes == {str(i): int(c) for i, c in enumerate(want.argmax(dim=1))}
    from tests.secure_batch_nets import resnet18
    r = run_inference(write_checkpoint(tmp_path / "bn.pt", resnet18(32, 320)), 1, 3, ["--encrypted_inference", "--wide_norm"])
    assert r.returncode != 0 and "--fold_norm" in r.stderr
