"""GPU: convolution-shaped Beaver triples (csrc/ring_conv.hip) -- the direct ring convolution against exact
integers bit for bit, the dealer's completion and both combine paths, the truncation, and conv_triples=True through the
network, the serving graph, three roles and inference.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from primia_amd import _lib  # noqa: E402
from primia_amd._lib import call  # noqa: E402
from primia_amd.secure import (Dealer, GraphedSecureInference, PreloadedDealer, ProtocolForm, SecureContext,  # noqa: E402
                               SecureResNet18, architecture_of, fold_batch_norm, image_requests, model_requests)
from tests import conv_triples_cases  # noqa: E402,F401  (registers the "conv-triples" three-role case)
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet, plain_forward  # noqa: E402
from tests.secure_common import ROOT, json_line, padded, run_inference, run_roles, write_checkpoint  # noqa: E402
from tests.secure_folded_nets import plaintext_logits, wide_mini  # noqa: E402
from tests.test_gpu_fss_wide import Guarded, dev  # noqa: E402
from tests.three_role_cases import CASES, wide_net  # noqa: E402

U64, I64 = np.uint64, np.int64

# name -> B, C, H, W, O, R, stride, pad: the smallest shapes at which the kernel can go wrong (8 x 8 pixel tiles, 64 output
# channels per block, chunks of 1 / 4 / 16 input channels for 7 x 7 / 3 x 3 / 1 x 1)
GEOMETRIES = {
    "stem-rgb": (2, 3, 18, 18, 8, 7, 2, 3),           # 9 x 9 outputs: a ragged second tile in both directions, two images
    "stem-gray": (1, 1, 16, 16, 4, 7, 2, 3),
    "3x3-ragged": (1, 5, 9, 9, 70, 3, 1, 1),          # ragged pixel tile, O across the 64 boundary, C across a chunk
    "3x3s2-odd": (2, 3, 9, 9, 5, 3, 2, 1),
    "3x3s2-even": (1, 6, 8, 8, 5, 3, 2, 1),
    "1x1s2": (1, 17, 9, 9, 6, 1, 2, 0),               # C across the chunk of 16
    "split": (1, 160, 7, 7, 64, 3, 1, 1),             # one block: the launcher slices the input channels
}


def conv_ref(x, w, stride, pad):
    """The integer convolution mod 2^64 on an explicit zero-padded unroll: uint64 products and sums wrap exactly."""
    (B, C, H, W), (O, _, R, S) = x.shape, w.shape
    xp = np.zeros((B, C, H + 2 * pad, W + 2 * pad), U64)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    out = np.zeros((B, O, Ho, Wo), U64)
    for r in range(R):
        for s in range(S):
            patch = xp[:, :, r:r + stride * Ho:stride, s:s + stride * Wo:stride]
            out += (patch[:, None] * w[None, :, :, r, s, None, None]).sum(axis=2, dtype=U64)
    return out


def shapes_of(g):
    B, C, H, W, O, R, stride, pad = g
    return (B, C, H, W), (O, C, R, R), (B, O, (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1)


def args_of(g):
    return (*g[:6], g[5], g[6], g[7])


def words(rng, shape):
    return rng.integers(0, 2 ** 64, size=shape, dtype=U64)      # full range: every carry path is live


@pytest.mark.parametrize("form", ["plain", "accumulate", "two-pairs"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_kernel_equals_the_integer_convolution(cuda, name, form):
    """plain: out = conv(x, w); accumulate: out += conv(x, w); two-pairs: party 1's combine z = c + conv(delta, b) +
    conv(a, eps), in place on c."""
    g = GEOMETRIES[name]
    xs, ws, zs = shapes_of(g)
    rng = np.random.default_rng(len(name) * 100 + g[1])
    assert (_lib.query("primia_ring_conv2d_split", *args_of(g), 1) > 1) == (name == "split")
    out = Guarded(zs, torch.int64, cuda)
    x, w, c = words(rng, xs), words(rng, ws), words(rng, zs)
    want = conv_ref(x, w, g[6], g[7])
    if form != "plain":
        out.view.copy_(dev(c, cuda))
        want = want + c
    if form == "two-pairs":
        a, e = words(rng, xs), words(rng, ws)
        call("primia_beaver_combine_conv", 1, dev(x, cuda), dev(e, cuda), dev(a, cuda), dev(w, cuda), out.view, out.view, None,
             *args_of(g))
        want = want + conv_ref(a, e, g[6], g[7])
    else:
        call("primia_ring_conv2d", dev(x, cuda), dev(w, cuda), out.view, *args_of(g), int(form == "accumulate"))
    assert out.intact() and np.array_equal(out.host().view(U64), want)


def u64(t):
    return t.cpu().numpy().view(U64)


def product_shares(cuda, g, x, w, pf, fused, seed=31):
    """ctx.conv2d under the new form on the given shares, with a dealer of this seed; scale = 10^pf (pf = 0: no truncation)."""
    ctx = SecureContext(Dealer(cuda, seed=seed), 10, pf, conv_triples=True)
    ctx.local_fused = fused
    return [t.cpu().numpy() for t in ctx.conv2d([dev(t, cuda) for t in x], [dev(t, cuda) for t in w], g[6], g[7])]


@pytest.mark.parametrize("name", ["stem-rgb", "3x3-ragged", "1x1s2", "split"])
def test_triple_combine_and_truncation(cuda, name):
    """The dealer's c0 + c1 is conv(a, b).  At scale 1 (truncation by 1 is the identity) the fused entry point and the
    per-party chain give equal shares of full-range inputs, which reconstruct to their integer convolution.  With encoded
    inputs below 2^15 (|z| < 2^40: the signed shares wrap with probability under 2^-23 per element, and not under this seed,
    checked on the scale-1 shares of the same dealer seed) every share at pf = 3 is its party's quotient toward zero, and the
    reconstruction is within 2 of trunc(z / scale), each division losing less than 1."""
    g = GEOMETRIES[name]
    xs, ws, zs = shapes_of(g)
    t = Dealer(cuda, seed=30).triple("conv", xs, ws, stride=g[6], padding=g[7])
    a, b, c = (u64(t[0][k]) + u64(t[1][k]) for k in range(3))
    assert c.shape == zs and np.array_equal(c, conv_ref(a, b, g[6], g[7]))
    rng = np.random.default_rng(7)
    x, w = [words(rng, xs) for _ in range(2)], [words(rng, ws) for _ in range(2)]
    fused, chain = (product_shares(cuda, g, x, w, 0, f) for f in (True, False))
    assert all(np.array_equal(fused[j], chain[j]) for j in range(2))
    assert np.array_equal((fused[0] + fused[1]).view(U64), conv_ref(x[0] + x[1], w[0] + w[1], g[6], g[7]))
    secret = [rng.integers(-2 ** 15, 2 ** 15, size=s, dtype=I64) for s in (xs, ws)]
    x, w = ([m, v.view(U64) - m] for v, m in zip(secret, x[:1] + w[:1]))
    z = conv_ref(secret[0].view(U64), secret[1].view(U64), g[6], g[7]).view(I64)
    assert np.abs(z).max() < 2 ** 40
    for f in (True, False):
        raw, got = (product_shares(cuda, g, x, w, pf, f) for pf in (0, 3))
        assert np.array_equal(raw[0].astype(object) + raw[1].astype(object), z.astype(object))      # no wrap under this seed
        assert all(np.array_equal(got[j], np.sign(raw[j]) * (np.abs(raw[j]) // 1000)) for j in range(2))
        assert np.abs(got[0] + got[1] - np.sign(z) * (np.abs(z) // 1000)).max() <= 2


PF, SEED = 6, 511


def nets(kind):
    gen = torch.Generator().manual_seed(510)
    sd = (wide_mini if kind == "faithful" else mini_resnet)(gen)
    images = torch.randn(2, 3, 32, 32, generator=gen)
    return sd, (fold_batch_norm(sd) if kind == "faithful" else sd), images


@pytest.mark.parametrize("kind", ["batch", "faithful"])
def test_network_graph_equals_eager_and_follows_the_plaintext(cuda, kind):
    """Three replays of the serving graph equal the eager pass on the primitives it holds, bit for bit, and the dealer was
    asked for image_requests(conv_triples=True).  Accuracy is measured against the default form: e0, its largest error
    against the float64 plaintext logits on the same images and seed; the new form's independent truncation errors of the
    same distribution must stay within 2 e0 + 2 * 10^-pf."""
    sd, shared, images = nets(kind)
    faithful = kind == "faithful"
    form = lambda conv: ProtocolForm(fss_bits=64, faithful_trunc=faithful, conv_triples=conv)

    def eager(conv, dealer):
        return SecureResNet18(SecureContext(dealer, 10, PF), shared, 32, MINI_BLOCKS, form=form(conv))(images.to(cuda))

    # (the folded form keeps BatchNorm's eps = 1e-5, plain_forward has none: it is given the variances with eps added)
    ref = {k: v + 1e-5 if faithful and k.endswith("running_var") else v for k, v in sd.items()}
    plain = plain_forward(ref, images, MINI_BLOCKS, PF)
    err = [np.abs(eager(conv, Dealer(cuda, seed=SEED, fss_bits=64)).cpu().numpy().astype(np.float64) - plain).max()
           for conv in (False, True)]
    print(f"{kind}: max |secure - plaintext| default form e0 = {err[0]:.3e}, conv_triples = {err[1]:.3e}")
    assert err[1] <= 2 * err[0] + 2 * 10.0 ** -PF
    g = GraphedSecureInference(shared, cuda, input_size=32, precision_fractional=PF, seed=SEED, blocks=MINI_BLOCKS, batch=2,
                               form=form(True))
    arch = architecture_of(shared)
    assert g.requests == model_requests(arch) + image_requests(arch, 32, 2, MINI_BLOCKS, form=form(True))
    assert sum(a[0] == "conv" for k, a, _ in g.requests if k == "triple") == 6
    for step in range(3):      # the primitives of the constructor's refill, then two more refills
        out = g(images.to(cuda), refill=step > 0).clone()
        assert torch.equal(out, eager(True, PreloadedDealer(g.tape, cuda, 64))), step


def test_three_roles_equal_the_in_process_run(cuda, tmp_path):
    """model_owner / data_owner / crypto_provider as three processes (the "batch" case under conv_triples: two images per pass,
    a padded second pass): both parties' logits equal the in-process run's under the same dealer seed, whose requests are the
    schedule the dealer rank follows."""
    pf, seed, c = 3, 5, CASES["conv-triples"]
    sd, images = c.tensors()
    dealer = Dealer(cuda, seed=seed)
    dealer.requests = []
    model = SecureResNet18(SecureContext(dealer, 10, pf), sd, c.size, c.blocks, form=c.form())
    dv = images.to(cuda)
    rows = [model(padded(dv[i:i + c.batch], c.batch))[:len(dv[i:i + c.batch])] for i in range(0, len(dv), c.batch)]
    arch = architecture_of(sd)
    assert dealer.requests == model_requests(arch) + len(rows) * image_requests(arch, c.size, c.batch, c.blocks, form=c.form())
    out = str(tmp_path / "logits")
    cmd = [sys.executable, os.path.join(ROOT, "tests", "conv_triples_cases.py"), out, "conv-triples", str(pf), str(seed)]
    run_roles([cmd] * 3, out, what="conv-triples")
    for j in range(2):
        assert torch.equal(torch.load(f"{out}.{j}"), torch.cat(rows).cpu()), j


def test_cli_conv_triples(cuda, tmp_path):
    """inference.py --encrypted_inference --conv_triples gives the classes of the default form; the float64 plaintext logits of
    these images have no pair within 10 e0 of a tie, e0 the default form's largest error against them."""
    sd = wide_net()[0]
    ckpt = write_checkpoint(tmp_path / "bn.pt", sd)

    def run(extra, dump):
        r = run_inference(ckpt, 2, PF, ["--encrypted_inference", "--fss_bits", "64"] + extra, batch_size=2, dump=str(dump))
        return json_line(r)["Inference Results"], torch.load(str(dump)).numpy().astype(np.float64)

    (res0, l0), (res1, _) = run([], tmp_path / "a.pt"), run(["--conv_triples"], tmp_path / "b.pt")
    images = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(0))      # load_images' synthetic set
    plain = plaintext_logits(sd, images, PF, 32)
    top = np.sort(plain, axis=1)
    assert (top[:, -1] - top[:, -2]).min() > 10 * np.abs(l0 - plain).max()
    assert sorted(res1) == ["0", "1"] and res1 == res0 == {str(i): int(c) for i, c in enumerate(plain.argmax(axis=1))}
