"""CPU: the definition of the secret-shared GroupNorm (tests/secure_groupnorm_nets.py) against float64, the request list of a
GroupNorm pass against a walk of the composed oracle forward, and the domain of the reference's Newton iteration."""
import numpy as np
import pytest
import torch

from oracle import secure_oracle as S
from primia_amd.secure import architecture_of, image_requests, model_requests, norm_of, primitive_bytes, serving_bytes
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet, numpy_sd, oracle_forward, resnet18
from tests.secure_groupnorm_nets import (LAYER_TOL, VAR_DOMAIN, RecordingDealer, ScheduleContext, group_mini, group_resnet18,
                                         oracle_group_norm)


def test_oracle_group_norm_is_a_group_norm():
    """oracle_group_norm at pf = 6 on a [2, 64, 6, 6] input whose float64 group variances lie in the Newton domain (asserted
    on the reference) against float64 F.group_norm on the decoded inputs.  Measured on the CPU: max |error| 5.0e-4 (4.98e-4,
    5.00e-4, 4.99e-4 under dealer seeds 1, 2, 3); the bound LAYER_TOL is twice that, 1.0e-3."""
    pf = 6
    g = torch.Generator().manual_seed(600)
    x = torch.randn(2, 64, 6, 6, generator=g) * (torch.rand(2, 64, 1, 1, generator=g) * 1.5 + 0.5)
    w, b = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    enc = lambda t: S.fix_encode(t.numpy(), 10, pf)
    xq, wq, bq = (torch.from_numpy(enc(t).astype(np.float64) / 10 ** pf) for t in (x, w, b))
    var = xq.reshape(2, 32, -1).var(dim=2, unbiased=False)
    assert VAR_DOMAIN[0] <= float(var.min()) and float(var.max()) <= VAR_DOMAIN[1]
    ref = torch.nn.functional.group_norm(xq, 32, wq, bq, 1e-5).numpy()
    for seed in (1, 2, 3):
        d = RecordingDealer(seed)
        ctx = S.OracleContext(d, 10, pf)
        xs, ws, bs = ctx.share(enc(x)), ctx.share(enc(w)), ctx.share(enc(b))
        n0 = len(d.requests)
        out = oracle_group_norm(ctx, xs, ws, bs)
        dec = S.radd(out[0], out[1]).astype(np.float64) / 10 ** pf
        err = np.abs(dec - ref).max()
        print("oracle_group_norm pf = 6, dealer seed", seed, ": max |error|", err)
        assert err <= LAYER_TOL, err
        # the primitives, in order: the square, eps, the Newton iteration on R = 64 values, the two products
        R, m = 64, 72
        newton = [("const_mask", (1,))] + 79 * [("triple", ("mul", (R,), (R,))), ("triple", ("mul", (R,), (R,))),
                                                ("const_mask", (1,)), ("triple", ("mul", (R,), (R,)))]
        assert d.requests[n0:] == [("triple", ("mul", (R, m), (R, m))), ("const_mask", (1,))] + newton + \
            [("triple", ("mul", (R,), (m, R))), ("triple", ("mul", (72, 64), (64,)))]


def flat(req):
    """A same-shape element-wise triple by its element count: the oracle's max tree asks for [B, C, P, w] where the device
    asks for the same elements as [rows, w] (ReplayDealer restores the shape; the element order is identical)."""
    kind, args = req
    if kind == "triple" and args[0] == "mul" and args[1] == args[2]:
        return kind, ("mul", int(np.prod(args[1])))
    return req


def walk_requests(state_dict, images, blocks, pooling, norm, pf=3):
    """(model requests, image requests) of oracle_forward as (kind, args) pairs."""
    d = RecordingDealer(0)
    oracle_forward(ScheduleContext(d, 10, pf), state_dict, images, blocks, pooling, norm)
    n_model = len(S.share_order(list(state_dict.keys())))
    return d.requests[:n_model], d.requests[n_model:]


@pytest.mark.parametrize("pooling", ["max", "avg"])
@pytest.mark.parametrize("B", [1, 3])
def test_image_requests_of_a_groupnorm_pass(B, pooling):
    """image_requests equals what a walk of oracle_forward asks its dealer for -- the GroupNorm and the BatchNorm form of the
    mini network and of the 8-block ResNet-18 at 32 x 32 -- has the data owner's mask first and public masks after it, and
    the GroupNorm list differs from the BatchNorm list of the same convolutions.  The walk's model part is model_requests
    (an OracleContext passes no owner on)."""
    images = np.zeros((B, 3, 32, 32), np.float32)
    for sd, blocks, norm in ((group_mini(torch.Generator().manual_seed(31)), MINI_BLOCKS, "group"),
                             (group_resnet18(32, 520), None, "group"),
                             (mini_resnet(torch.Generator().manual_seed(21)), MINI_BLOCKS, "batch"),
                             (resnet18(32, 320), None, "batch")):
        arch = architecture_of(sd)
        assert norm_of(arch) == norm
        got = image_requests(arch, 32, B, blocks, pooling)
        model_req, image_req = walk_requests(numpy_sd(sd), images, blocks, pooling, norm)
        assert [flat((k, a)) for k, a, _ in got] == [flat(r) for r in image_req]
        assert len(model_req) == len(arch)
        assert model_req == [(k, a) for k, a, _ in model_requests(arch)]
        assert got[0][2] == {"owner": 1} and all(kw == {"owner": None} for k, _, kw in got[1:] if k == "const_mask")
        assert serving_bytes(arch, 32, B, blocks, pooling) == primitive_bytes(got) + primitive_bytes(got) // 8
    bn = mini_resnet(torch.Generator().manual_seed(21))
    assert norm_of(architecture_of(bn)) == "batch"
    bn_req = image_requests(architecture_of(bn), 32, B, MINI_BLOCKS, pooling)
    gn_req = image_requests(architecture_of(group_mini(torch.Generator().manual_seed(31))), 32, B, MINI_BLOCKS, pooling)
    assert bn_req != gn_req
    count = lambda req: sum(1 for k, a, _ in req if k == "triple" and a[0] == "mul")
    assert count(gn_req) - count(bn_req) == 6 * (3 * 79 + 1) - 3 * 79      # six norm sites: a Newton call and a square each, against ONE hoisted call


def test_norm_detection_and_refusals():
    gn, bn = group_mini(torch.Generator().manual_seed(31)), mini_resnet(torch.Generator().manual_seed(21))
    assert norm_of(gn.keys()) == norm_of(gn.keys(), "group") == "group" and norm_of(bn.keys(), "batch") == "batch"
    for keys, norm in ((gn.keys(), "batch"), (bn.keys(), "group"), (bn.keys(), "instance")):
        with pytest.raises(ValueError, match="norm"):
            norm_of(keys, norm)
    arch = architecture_of(gn)
    arch["conv1.weight"], arch["bn1.weight"] = (48, 3, 7, 7), (48,)
    with pytest.raises(ValueError, match="groups"):
        image_requests(arch, 32, 1, MINI_BLOCKS)


def newton(v, pf):
    """OracleContext.reciprocal_newton of the public values v (shared with a random mask), decoded."""
    ctx = S.OracleContext(RecordingDealer(9), 10, pf)
    q = np.round(np.asarray(v, np.float64) * 10 ** pf).astype(np.int64)
    out = ctx.reciprocal_newton(ctx.share(q))
    return S.radd(out[0], out[1]).astype(np.float64) / 10 ** pf


def test_newton_domain():
    """The domain of the reference's iteration (x0 = (21 - v) / 20, 79 steps), reproduced from
    OracleContext.reciprocal_newton: relative error against v^-1/2 at most 0.7 % (pf = 3) / 0.3 % (pf = 6) for v in
    [0.05, 16], 1.6 % at 0.01, 15 % at 0.001, and about 49 at v = 0."""
    grid = np.concatenate([np.geomspace(0.05, 16, 40), [0.05, 0.1, 1.0, 4.0, 16.0]])
    for pf, bound in ((3, 0.007), (6, 0.003)):
        rel = np.abs(newton(grid, pf) * np.sqrt(grid) - 1)
        print("pf", pf, "max relative error on [0.05, 16]:", rel.max())
        assert rel.max() <= bound, (pf, rel.max())
    for pf in (3, 6):
        r = newton([0.01, 0.001, 0.0], pf)
        rel = np.abs(r[:2] * np.sqrt([0.01, 0.001]) - 1)
        print("pf", pf, "relative error at 0.01, 0.001:", rel.tolist(), "newton(0):", r[2])
        assert 0.012 <= rel[0] <= 0.02 and 0.12 <= rel[1] <= 0.18
        assert 45 <= r[2] <= 53
