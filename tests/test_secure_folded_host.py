"""CPU: the model owner's BatchNorm fold (primia_amd.secure.fold_batch_norm) against its float64 formula, the request list of a
folded pass against a walk of the composed oracle forward (tests/secure_folded_nets.py), and the accuracy of the folded
forward -- and of the reference's form -- on running variances outside the Newton domain."""
import numpy as np
import pytest
import torch

from oracle import secure_oracle as S
from primia_amd.secure import (NORMS, architecture_of, fold_batch_norm, folded_architecture, image_requests,
                               largest_batch_that_fits, model_requests, norm_of, primitive_bytes, serving_bytes)
from tests import fss_wide_ref as W
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet, numpy_sd, oracle_forward, resnet18
from tests.secure_folded_nets import (EPS, FOLDED_TOL, NARROW_VARIANCES, WIDE_VARIANCES, WideChaChaDealer, fold64,
                                      narrow_resnet18, oracle_folded_forward, plaintext_logits, wide_mini, wide_resnet18)
from tests.secure_groupnorm_nets import RecordingDealer, ScheduleContext, group_mini


# ---- the fold ---------------------------------------------------------------------------------------------------------------
def test_fold_is_the_float64_formula():
    """Keys, order, dtypes and values: <prefix>.scale / .shift stand where .weight / .bias stood, the statistics and
    num_batches_tracked are gone, conv and fc tensors are the very tensors of the checkpoint, and every value is the float32
    rounding of gamma / sqrt(var + 1e-5) and beta - mean * scale evaluated in float64."""
    sd = wide_mini(torch.Generator().manual_seed(41))
    folded = fold_batch_norm(sd)
    sites = [k[:-len(".running_var")] for k in sd if k.endswith(".running_var")]
    assert len(sites) == 6
    want_keys = []
    for k in sd:
        p, leaf = k.rsplit(".", 1)
        if p in sites:
            want_keys += {"weight": [p + ".scale"], "bias": [p + ".shift"]}.get(leaf, [])
        else:
            want_keys.append(k)
    assert list(folded) == want_keys
    for k, v in folded.items():
        if k.rsplit(".", 1)[0] not in sites:
            assert v is sd[k]
    for p in sites:
        g, b, m, var = (sd[p + s].double() for s in (".weight", ".bias", ".running_mean", ".running_var"))
        assert sorted(set(var.tolist())) == sorted(float(np.float32(v)) for v in WIDE_VARIANCES)
        s = g / torch.sqrt(var + 1e-5)
        for name, ref in ((".scale", s), (".shift", b - m * s)):
            got = folded[p + name]
            assert got.dtype == torch.float32 and tuple(got.shape) == tuple(g.shape)
            assert torch.equal(got, ref.float()), p + name
    ref = fold64(sd)
    assert list(ref) == list(folded) and all(torch.equal(ref[k], folded[k]) for k in ref)
    other = fold_batch_norm(sd, eps=1e-3)
    assert torch.equal(other["bn1.scale"], (sd["bn1.weight"].double() / torch.sqrt(sd["bn1.running_var"].double() + 1e-3)).float())
    assert not torch.equal(other["bn1.scale"], folded["bn1.scale"])
    assert "bn1.weight" in sd and "bn1.scale" not in sd      # (the checkpoint itself is left as it was)


def test_fold_refusals():
    bn = mini_resnet(torch.Generator().manual_seed(21))
    with pytest.raises(ValueError, match="folding needs BatchNorm statistics"):
        fold_batch_norm(group_mini(torch.Generator().manual_seed(31)))
    with pytest.raises(ValueError, match="already folded"):
        fold_batch_norm(fold_batch_norm(bn))
    for bad in (-1e-3, float("nan"), float("inf")):
        sd = dict(bn)
        sd["layer1.0.bn2.running_var"] = bn["layer1.0.bn2.running_var"].clone()
        sd["layer1.0.bn2.running_var"][5] = bad
        with pytest.raises(ValueError, match="layer1.0.bn2.running_var holds a negative or non-finite variance"):
            fold_batch_norm(sd)
    zero = dict(bn)
    zero["bn1.running_var"] = torch.zeros(64)
    assert torch.isfinite(fold_batch_norm(zero)["bn1.scale"]).all()      # (a zero variance is a variance: eps carries it)
    with pytest.raises(ValueError, match="folding needs BatchNorm statistics"):
        folded_architecture(architecture_of(group_mini(torch.Generator().manual_seed(31))))
    with pytest.raises(ValueError, match="already folded"):
        folded_architecture(folded_architecture(architecture_of(bn)))


def test_folded_architecture_and_norm_detection():
    gn, bn = group_mini(torch.Generator().manual_seed(31)), mini_resnet(torch.Generator().manual_seed(21))
    full = resnet18(32, 320)
    for sd in (bn, full):
        assert folded_architecture(architecture_of(sd)) == architecture_of(fold_batch_norm(sd))
        assert list(folded_architecture(architecture_of(sd))) == list(architecture_of(fold_batch_norm(sd)))
    folded = fold_batch_norm(bn)
    assert "folded" in NORMS
    assert norm_of(folded.keys()) == norm_of(folded.keys(), "folded") == norm_of(architecture_of(folded)) == "folded"
    assert norm_of(bn.keys()) == "batch" and norm_of(gn.keys()) == "group"
    for keys, norm in ((bn.keys(), "folded"), (folded.keys(), "batch"), (folded.keys(), "group"), (gn.keys(), "folded")):
        with pytest.raises(ValueError, match="norm"):
            norm_of(keys, norm)
    # shared as parameters, where the BatchNorm weights stood; no buffers
    assert S.share_order(list(folded.keys())) == list(folded.keys())
    assert [a for _, a, _ in model_requests(architecture_of(folded))] == [tuple(v.shape) for v in folded.values()]


# ---- request lists ------------------------------------------------------------------------------------------------------------
def flat(req):
    """A same-shape element-wise triple by its element count (the oracle's max tree asks for [B, C, P, w] where the device
    asks for the same elements as [rows, w])."""
    kind, args = req
    if kind == "triple" and args[0] == "mul" and args[1] == args[2]:
        return kind, ("mul", int(np.prod(args[1])))
    return req


def walk_requests(folded, images, blocks, pooling, pf=3):
    """(model requests, image requests) of oracle_folded_forward as (kind, args) pairs."""
    d = RecordingDealer(0)
    oracle_folded_forward(ScheduleContext(d, 10, pf), folded, images, blocks, pooling)
    n_model = len(S.share_order(list(folded.keys())))
    return d.requests[:n_model], d.requests[n_model:]


@pytest.mark.parametrize("pooling", ["max", "avg"])
@pytest.mark.parametrize("B", [1, 3])
def test_image_requests_of_a_folded_pass(B, pooling):
    """image_requests of a folded architecture equals what a walk of oracle_folded_forward asks its dealer for -- the mini
    network and the 8-block ResNet-18 at 32 x 32; it holds no Newton triple and exactly one element-wise triple per norm
    site; against the BatchNorm list of the same convolutions it lacks exactly the 237 Newton triples, their 80 masks and one
    triple per site, in place; the static bytes follow the list as in every other form."""
    images = np.zeros((B, 3, 32, 32), np.float32)
    for sd, blocks, sites in ((mini_resnet(torch.Generator().manual_seed(21)), MINI_BLOCKS, 6), (resnet18(32, 320), None, 20)):
        folded = fold_batch_norm(sd)
        arch = architecture_of(folded)
        assert arch == folded_architecture(architecture_of(sd)) and norm_of(arch) == "folded"
        got = image_requests(arch, 32, B, blocks, pooling)
        model_req, image_req = walk_requests(numpy_sd(folded), images, blocks, pooling)
        assert [flat((k, a)) for k, a, _ in got] == [flat(r) for r in image_req]
        assert len(model_req) == len(arch) and model_req == [(k, a) for k, a, _ in model_requests(arch)]
        assert got[0] == ("const_mask", (B, 3, 32, 32), {"owner": 1})
        assert not any(k == "const_mask" for k, _, _ in got[1:])
        muls = [a for k, a, _ in got if k == "triple" and a[0] == "mul"]
        assert not any(len(a[1]) == 1 and a[1] == a[2] for a in muls)                                # no ("mul", (n,), (n,))
        site = [a for a in muls if len(a[1]) == 2 and len(a[2]) == 1]
        assert len(site) == sites and all(a[1][1] == a[2][0] and a[1][0] % B == 0 for a in site)     # ("mul", (B*h*h, c), (c,))
        # the BatchNorm list of the same convolutions: drop Newton (its first mask, then 79 x (triple, triple, mask, triple))
        # and the ("mul", (c,), (B*h*h, c)) triple of every site, and the folded list is what remains
        bn_req = image_requests(architecture_of(sd), 32, B, blocks, pooling)
        channels = sum(v[0] for k, v in architecture_of(sd).items() if k.endswith(".running_var"))
        newton = [r for r in bn_req if r == ("const_mask", (1,), {"owner": None}) or
                  r == ("triple", ("mul", (channels,), (channels,)), {})]
        assert len(newton) == 80 + 237 and bn_req[1:1 + 317] == newton
        first = [r for r in bn_req if r[0] == "triple" and r[1][0] == "mul" and len(r[1][1]) == 1 and len(r[1][2]) == 2]
        assert len(first) == sites
        rest = [r for r in bn_req[:1] + bn_req[318:] if r not in first]
        assert rest == got and len(bn_req) - len(got) == 237 + 80 + sites
        assert bn_req == image_requests(architecture_of(sd), 32, B, blocks, pooling, reveal="logits")
        b = primitive_bytes(got)
        assert serving_bytes(arch, 32, B, blocks, pooling) == b + b // 8 == b * 9 // 8
        assert serving_bytes(arch, 32, B, blocks, pooling) < serving_bytes(architecture_of(sd), 32, B, blocks, pooling)
        budget = serving_bytes(arch, 32, 2, blocks, pooling)
        assert largest_batch_that_fits(arch, 32, budget, blocks, pooling) == 2
        assert largest_batch_that_fits(arch, 32, budget - 1, blocks, pooling) == 1


def test_a_folded_pass_at_224_saves_what_the_survey_counts():
    """At 224 x 224 the folded list has 61 element-wise triples where the BatchNorm list has 298, and holds 2,483,712 fewer
    elements in the per-site products: about 79 MB of b and c shares per image."""
    from primia_amd import resnet_spec

    sd = resnet_spec.init_state_dict(resnet_spec.resnet18_spec(3, 3, 224, "max"))
    bn_req = image_requests(architecture_of(sd), 224, 1)
    got = image_requests(folded_architecture(architecture_of(sd)), 224, 1)
    count = lambda req: sum(1 for k, a, _ in req if k == "triple" and a[0] == "mul")
    assert count(bn_req) == 298 and count(got) == 298 - 237 - 20
    dropped = [a for k, a, _ in bn_req if k == "triple" and a[0] == "mul" and len(a[1]) == 1 and len(a[2]) == 2]
    assert sum(a[2][0] * a[2][1] for a in dropped) == 2_483_712
    saved = primitive_bytes(bn_req) - primitive_bytes(got)
    assert saved == 16 * (2 * 2_483_712 + 4800) + 237 * 16 * 3 * 4800 + 80 * 8
    assert sum(a[0] for k, a, _ in got if k == "dif_keys") == 3_311_616


# ---- accuracy -------------------------------------------------------------------------------------------------------------------
def secure_logits(forward, dealer_seed, pf, *args, **kw):
    """Decoded logits (float64) of a composed forward at 64-bit comparisons on a seeded host dealer (WideChaChaDealer)."""
    ctx = W.WideOracleContext(WideChaChaDealer(dealer_seed, 64), 10, pf, 64)
    out = forward(ctx, *args, **kw)
    assert not any(W.wraps(int(a), int(d), 64) for alpha, diff in ctx.compared for a, d in zip(alpha[:64], diff[:64]))
    return S.radd(out[0], out[1]).astype(np.float64) / 10 ** pf


def test_folded_forward_follows_the_plaintext_model_where_the_reference_form_does_not():
    """pf = 6, 64-bit comparisons, the 8-block ResNet-18 at 32 x 32 (seed 720) with running variances set channel by channel
    from {1e-3, 1e-2, 0.3, 1, 4, 25, 30}, two N(0, 1) images (seed 721): the decoded logits of oracle_folded_forward on
    fold_batch_norm's dict against float64 oracle.train_oracle.forward(training=False) on the decoded inputs.
    Measured on the CPU: max |error| 3.18e-5, 1.87e-5, 3.56e-5 under dealer seeds 1, 2, 3 (logits of 1.0 to 1.7); the bound
    FOLDED_TOL is twice the largest, 7.14e-5.  The reference's form (oracle_forward, norm "batch": Newton on shares of
    running_var, no eps) on the same checkpoint and dealer seed 1 misses the bound: it measured 8.1e6 -- logits in the
    millions (the iteration returns the wrong sign at 25 and 30 and is 15 % off at 1e-3, at every one of 20 norm sites)."""
    pf = 6
    sd = wide_resnet18(32, 720)
    images = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(721))
    plain = plaintext_logits(sd, images, pf, 32)
    folded = numpy_sd(fold_batch_norm(sd))
    errs = []
    for seed in (1, 2, 3):
        dec = secure_logits(oracle_folded_forward, seed, pf, folded, images.numpy())
        errs.append(float(np.abs(dec - plain).max()))
        print("folded, wide variances, pf = 6, dealer seed", seed, ": max |error|", errs[-1], "logits", dec.tolist())
    ref = secure_logits(oracle_forward, 1, pf, numpy_sd(sd), images.numpy(), norm="batch")
    ref_err = float(np.abs(ref - plain).max())
    print("reference form on the same checkpoint: max |error|", ref_err, "logits", ref.tolist(), "plain", plain.tolist())
    assert max(errs) <= FOLDED_TOL, errs
    assert ref_err > FOLDED_TOL, ref_err
    assert np.abs(plain[0] - plain[1]).max() > 100 * FOLDED_TOL      # (the two images are told apart far above the bound)


def test_folded_forward_inside_the_newton_domain():
    """The same network with every running variance in [0.3, 4] (seed 730, images seed 731, dealer seed 1): the folded
    forward is within FOLDED_TOL of the plaintext model there too.  Measured: 8.6e-6."""
    pf = 6
    sd = narrow_resnet18(32, 730)
    assert min(NARROW_VARIANCES) >= 0.3 and max(NARROW_VARIANCES) <= 4
    images = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(731))
    plain = plaintext_logits(sd, images, pf, 32)
    dec = secure_logits(oracle_folded_forward, 1, pf, numpy_sd(fold_batch_norm(sd)), images.numpy())
    err = float(np.abs(dec - plain).max())
    print("folded, variances in [0.3, 4], pf = 6, dealer seed 1: max |error|", err)
    assert err <= FOLDED_TOL, err
    assert EPS == 1e-5
