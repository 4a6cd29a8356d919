"""CPU: the faithful truncation of a shared product (tests/secure_faithful_nets.py's definition) against Python integers on
every kind of mask, the reference's per-share form on shares built to wrap, the request list and static bytes of a pass
with faithful_trunc, primia_amd.secure.expected_wraps against a direct sum, the refusals, and the accuracy bound of the
composed forward's inputs."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import secure_oracle as S
from primia_amd.secure import (SecureContext, SecureResNet18, architecture_of, check_faithful_trunc, expected_wraps,
                               fold_batch_norm, image_requests, largest_batch_that_fits, primitive_bytes, serving_bytes)
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet, numpy_sd, resnet18
from tests.secure_faithful_nets import (DIVISORS, EDGE_MASKS, ERR, FAITHFUL_TOL, FAITHFUL_TOL_MEASURED, M64, FaithfulProducts,
                                        int_trunc_faithful, int_trunc_reference, oracle_trunc_faithful, signed, wrap_case,
                                        wrapping_pair)
from tests.secure_folded_nets import oracle_folded_forward
from tests.secure_groupnorm_nets import RecordingDealer, ScheduleContext, group_mini

I64, U64 = np.int64, np.uint64


def as_i64(values):
    return np.array([v & M64 for v in values], dtype=U64).view(I64)


# ---- 1. the definition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIVISORS)
def test_definition_against_python_integers(d):
    """oracle_trunc_faithful on 20,000 random z over the whole of -2^62 <= z < 2^62 (both ends among them) under uniform
    masks, and on every (z, mask) of a grid of edge values with masks 0, 2^62, 2^63 - 1, 2^63, 2^64 - 2^62 -+ 1, 2^64 - 1:
    both output shares are int_trunc_faithful's -- the definition restated on Python integers -- and their sum is
    floor(z / d) + e with e in {-1, 0, 1, 2}, the bound DESIGN.md states, for every case."""
    rng = np.random.default_rng(d)
    zs = [int(v) for v in rng.integers(-2 ** 62, 2 ** 62, size=20000, dtype=I64)]
    masks = [int(v) for v in rng.integers(0, 2 ** 64, size=20000, dtype=U64)]
    edges = [-2 ** 62, -2 ** 62 + 1, -d - 1, -d, -1, 0, 1, d - 1, d, 2 ** 61, 2 ** 62 - d, 2 ** 62 - 1]
    for z in edges:
        for m in EDGE_MASKS + tuple((mm - z) & M64 for mm in EDGE_MASKS):      # party 0's share, and party 1's, at each edge
            zs.append(z)
            masks.append(m)
    z0 = as_i64(masks)
    z1 = S.rsub(as_i64(zs), z0)
    dealer = RecordingDealer(7)
    ctx = S.OracleContext(dealer, 10, 3)
    out = oracle_trunc_faithful(ctx, [z0, z1], d)
    assert dealer.requests == [("triple", ("mul", (len(zs),), (len(zs),)))]
    got = S.radd(out[0], out[1])
    errs = set()
    for i, z in enumerate(zs):
        e = int(got[i]) - z // d
        errs.add(e)
        assert e in ERR, (z, masks[i], d, e)
    assert len(errs) >= 3      # (the bound is not slack: at least three of its four values occur)
    # the same shares from the restatement on integers, on a replay of the triple
    dealer2 = RecordingDealer(7)
    (a0, b0, c0), (a1, b1, _) = dealer2.triple("mul", (len(zs),), (len(zs),))
    for i in list(range(0, 20000, 97)) + list(range(20000, len(zs))):
        w0, w1 = int_trunc_faithful(int(z0[i]), int(z1[i]), d, *(int(t[i]) & M64 for t in (a0, a1, b0, b1, c0)))
        assert (w0, w1) == (int(out[0][i]) & M64, int(out[1][i]) & M64), i


@pytest.mark.parametrize("d", DIVISORS)
def test_reference_form_is_off_by_2_64_over_d_on_wrapping_shares(d):
    """Shares whose signed sum wraps (wrapping_pair): the reference's per-share division -- OracleContext.trunc, restated on
    integers -- is off by 2^64 / d, to within two units, on every element; the faithful form on the very same shares is
    inside its bound."""
    rng = np.random.default_rng(100 + d)
    z = rng.integers(-2 ** 62, 2 ** 62, size=4000, dtype=I64)
    z[np.abs(z) < 4] = 4
    z[:4] = [4, -4, 2 ** 62 - 1, -2 ** 62]
    z0, z1 = wrapping_pair(z, rng)
    assert np.array_equal(S.radd(z0, z1), z)
    ctx = S.OracleContext(RecordingDealer(8), 10, 3)
    ref = ctx.trunc([z0, z1], d)
    ref = S.radd(ref[0], ref[1])
    out = oracle_trunc_faithful(ctx, [z0, z1], d)
    got = S.radd(out[0], out[1])
    for i in range(len(z)):
        zi = int(z[i])
        assert signed(int(z0[i])) + signed(int(z1[i])) == zi - (2 ** 64 if zi > 0 else -2 ** 64)      # the signed sum wraps
        off = int(ref[i]) - zi // d
        assert int(ref[i]) == int_trunc_reference(int(z0[i]), int(z1[i]), d)
        assert abs(abs(off) - 2 ** 64 // d) <= 2 and (off < 0) == (zi > 0), (zi, off)
        assert int(got[i]) - zi // d in ERR


# ---- 2. the schedule ----------------------------------------------------------------------------------------------------------
class FaithfulScheduleContext(FaithfulProducts, ScheduleContext):
    pass


def flat(req):
    kind, args = req[0], req[1]
    if kind == "triple" and args[0] == "mul" and args[1] == args[2]:
        return kind, ("mul", int(np.prod(args[1])))
    return kind, args


@pytest.mark.parametrize("reveal", ["logits", "class"])
@pytest.mark.parametrize("B", [1, 3])
def test_image_requests_with_the_flag(B, reveal):
    """image_requests(faithful_trunc=True) of a folded architecture is the flag-off list with one ("mul", shape, shape) triple
    right after each conv2d, affine_eval and linear product triple, shape that of the product; it is what a walk of
    oracle_folded_forward on a context with FaithfulProducts asks for; with the flag off the list is the default's, and an option
    passed by position is a TypeError; the primitive bytes grow by exactly the carry triples', the static bytes follow."""
    for sd, blocks, convs in ((mini_resnet(torch.Generator().manual_seed(21)), MINI_BLOCKS, 6), (resnet18(32, 320), None, 20)):
        folded = fold_batch_norm(sd)
        arch = architecture_of(folded)
        off = image_requests(arch, 32, B, blocks, pooling="max", reveal=reveal)
        with pytest.raises(TypeError):      # an option by position
            image_requests(arch, 32, B, blocks, "max", reveal, False, False)
        assert off == image_requests(arch, 32, B, blocks, pooling="max", reveal=reveal, faithful_trunc=False)
        on = image_requests(arch, 32, B, blocks, pooling="max", reveal=reveal, faithful_trunc=True)
        want, carries = [], []
        for kind, args, kw in off:
            want.append((kind, args, kw))
            if kind != "triple" or (args[0] == "mul" and not (len(args[1]) == 2 and len(args[2]) == 1)):
                continue
            shape = args[1][:-1] + (args[2][-1],) if args[0] == "matmul" else args[1]
            carries.append(shape)
            want.append(("triple", ("mul", shape, shape), {}))
        assert on == want and len(carries) == 2 * convs + 1      # a conv2d and a norm per site, and fc
        if reveal == "logits":
            d = RecordingDealer(0)
            oracle_folded_forward(FaithfulScheduleContext(d, 10, 3), numpy_sd(folded), np.zeros((B, 3, 32, 32), np.float32), blocks)
            assert [flat(r) for r in d.requests[len(arch):]] == [flat(r) for r in on]
        extra = sum(16 * 3 * int(np.prod(s)) for s in carries)
        b_off, b_on = primitive_bytes(off), primitive_bytes(on)
        assert b_on - b_off == extra
        assert serving_bytes(arch, 32, B, blocks, pooling="max", reveal=reveal) == b_off + b_off // 8
        assert serving_bytes(arch, 32, B, blocks, pooling="max", reveal=reveal, faithful_trunc=True) == b_on + b_on // 8
        budget = serving_bytes(arch, 32, 2, blocks, pooling="max", reveal=reveal, faithful_trunc=True)
        assert largest_batch_that_fits(arch, 32, budget, blocks, pooling="max", reveal=reveal, faithful_trunc=True) == 2
        assert largest_batch_that_fits(arch, 32, budget - 1, blocks, pooling="max", reveal=reveal, faithful_trunc=True) == 1
        assert largest_batch_that_fits(arch, 32, budget - 1, blocks, pooling="max", reveal=reveal) >= 2


# ---- 3. expected_wraps ----------------------------------------------------------------------------------------------------------
def test_expected_wraps_against_a_direct_sum():
    """A stem and a head (no blocks): conv1 2 x 3 x 7 x 7, a folded norm, the max stem, the global average and fc, two 8 x 8
    images of large pixels at pf = 6.  expected_wraps is the direct sum of |z| / 2^64 over the convolution's outputs, the
    norm's products and fc's products, with z = value * 10^12, and the largest |z| / 2^62; an unfolded dict is folded first."""
    gen = torch.Generator().manual_seed(5)
    bn = {"conv1.weight": torch.randn(2, 3, 7, 7, generator=gen), "bn1.weight": torch.tensor([1.5, -0.5]),
          "bn1.bias": torch.tensor([0.25, 1.0]), "bn1.running_mean": torch.tensor([0.5, -1.0]),
          "bn1.running_var": torch.tensor([4.0, 0.25]), "fc.weight": torch.randn(3, 2, generator=gen),
          "fc.bias": torch.randn(3, generator=gen)}
    sd = fold_batch_norm(bn)
    images = torch.randn(2, 3, 8, 8, generator=gen) * 1000
    got = expected_wraps(sd, images, 6, blocks=[])
    s2 = 10.0 ** 12
    w, x = sd["conv1.weight"].double().numpy(), images.double().numpy()
    xp = np.pad(x, ((0, 0), (0, 0), (3, 3), (3, 3)))
    conv = np.zeros((2, 2, 4, 4))
    for b in range(2):
        for o in range(2):
            for i in range(4):
                for j in range(4):
                    conv[b, o, i, j] = (xp[b, :, 2 * i:2 * i + 7, 2 * j:2 * j + 7] * w[o]).sum()
    prod = conv * sd["bn1.scale"].double().numpy().reshape(1, 2, 1, 1)
    y = torch.from_numpy(prod + sd["bn1.shift"].double().numpy().reshape(1, 2, 1, 1))
    feat = torch.relu(F.max_pool2d(y, 3, 2, 1)).mean(dim=(2, 3)).numpy()
    fc = feat[:, None, :] * sd["fc.weight"].double().numpy()[None]      # [B, classes, features]: summed over the features
    fc = fc.sum(axis=2)
    want = {"conv2d": np.abs(conv).sum() * s2 / 2.0 ** 64, "affine_eval": np.abs(prod).sum() * s2 / 2.0 ** 64,
            "linear": np.abs(fc).sum() * s2 / 2.0 ** 64}
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-9), k
    assert got["total"] == pytest.approx(sum(want.values()), rel=1e-9)
    assert got["max_ratio"] == pytest.approx(max(np.abs(conv).max(), np.abs(prod).max(), np.abs(fc).max()) * s2 / 2.0 ** 62, rel=1e-9)
    assert got["conv2d"] > 1e-4      # (pixels of 1,000: a wrap in ten thousand truncations, where pf = 3 has none in 10^9)
    assert expected_wraps(bn, images, 6, blocks=[]) == got
    assert expected_wraps(sd, images, 3, blocks=[])["total"] == pytest.approx(got["total"] / 1e6, rel=1e-9)


def test_the_accuracy_case_meets_its_conditions():
    """The network and images of the accuracy case (wrap_case): at pf = 6 the reference's form is expected to wrap at least
    20 times in the one pass, and the largest pre-truncation value is below 2^61, half the faithful form's precondition."""
    sd, images = wrap_case()
    e = expected_wraps(sd, images, 6)
    print("wrap_case: expected_wraps", e)
    assert e["total"] >= 20 and e["max_ratio"] < 0.5
    assert FAITHFUL_TOL == 2 * max(FAITHFUL_TOL_MEASURED) and len(FAITHFUL_TOL_MEASURED) == 3
    assert expected_wraps(sd, images, 3)["total"] < 1e-4


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_networks_that_are_not_folded_are_refused():
    bn, gn = mini_resnet(torch.Generator().manual_seed(21)), group_mini(torch.Generator().manual_seed(31))
    for sd, why in ((bn, "fold the BatchNorm statistics first"), (gn, "cannot be folded")):
        arch = architecture_of(sd)
        with pytest.raises(ValueError, match="faithful_trunc covers the products of a folded network") as info:
            image_requests(arch, 32, 1, MINI_BLOCKS, faithful_trunc=True)
        assert why in str(info.value) and "Newton" in str(info.value)
        with pytest.raises(ValueError, match=why):
            serving_bytes(arch, 32, 1, MINI_BLOCKS, faithful_trunc=True)
        ctx = SecureContext(types.SimpleNamespace(device=torch.device("cpu")), 10, 6)
        with pytest.raises(ValueError, match=why):
            SecureResNet18(ctx, sd, 32, MINI_BLOCKS, faithful_trunc=True)
        assert not ctx.faithful_trunc
        with pytest.raises(ValueError, match=why):      # (a context that carries the flag is checked as well)
            SecureResNet18(SecureContext(types.SimpleNamespace(device=torch.device("cpu")), 10, 6, faithful_trunc=True), sd, 32,
                           MINI_BLOCKS)
    with pytest.raises(ValueError, match="cannot be folded"):
        expected_wraps(gn, torch.zeros(1, 3, 32, 32), 6, blocks=MINI_BLOCKS)
    check_faithful_trunc("folded")
    assert image_requests(architecture_of(fold_batch_norm(bn)), 32, 1, MINI_BLOCKS, faithful_trunc=True)
