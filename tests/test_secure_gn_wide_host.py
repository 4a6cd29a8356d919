"""CPU: the wide-range secret-shared GroupNorm (tests/secure_gn_wide_nets.py, inference.py --wide_norm) against float64, the
domain of its undamped Newton iteration, what the default form does outside its window, the request list of a wide pass
against a walk of the composed oracle forward, and the refusals."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import inference
from oracle import secure_oracle as S
from primia_amd import secure
from primia_amd.secure import (architecture_of, image_requests, largest_batch_that_fits, norm_of, primitive_bytes,
                               serving_bytes)
from tests import secure_gn_wide_nets as W
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet, numpy_sd, resnet18
from tests.secure_groupnorm_nets import RecordingDealer, ScheduleContext, group_mini, group_resnet18, oracle_group_norm
from tests.test_secure_groupnorm_host import flat


def test_constants_agree():
    """The library runs the definition's constants."""
    assert (secure.GN_WIDE_SCALE, secure.GN_WIDE_STEPS, secure.GN_WIDE_FLOOR, secure.GN_WIDE_PF) == \
        (W.S_IT, W.STEPS, W.FLOOR, W.PF_RANGE)
    assert secure.GN_WIDE_X0 == round(W.X0 * W.S_IT)


@pytest.mark.parametrize("pf", [3, 6])
def test_wide_group_norm_is_a_group_norm_on_the_served_range(pf):
    """oracle_group_norm_wide on a [2, 64, 6, 6] input whose float64 group variances span the served range of this pf (1e-3 to
    1.2e4 at pf 3; to 1e2 at pf 6, where the raw squares Xc^2 * s^2 of larger variances meet the ring's headroom: asserted on
    the reference), one group constant, against float64 F.group_norm under three dealer seeds.  The bound is twice what the
    CPU composition measured (tests/secure_gn_wide_nets.py)."""
    x, w, b, _ = W.wide_layer_input(pf)
    lo, hi = W.VAR_SERVED if pf < 6 else W.VAR_SERVED_PF6
    for seed in (1, 2, 3):
        d = RecordingDealer(seed)
        err, var = W.layer_error(W.oracle_group_norm_wide, pf, seed, x, w, b, dealer=d)
        const = var < 1e-9
        assert const.sum() == 1 and const[5]
        assert lo <= var[~const].min() < 2 * lo and hi / 2 < var[~const].max() <= hi, (var.min(), var.max())
        print("oracle_group_norm_wide pf =", pf, "dealer seed", seed, ": max |error|", err.max(), "constant group:", err[const].max())
        assert np.isfinite(err).all() and err.max() <= W.WIDE_LAYER_TOL[pf], err.max()
        n0 = 3      # the shares of x, weight, bias
        assert d.requests[n0:] == W.wide_site_requests(64, 72, 72, 64)
        assert len(d.requests[n0:]) == 4 * (W.STEPS - 1) + 4 == 128


def test_rsqrt_newton_domain():
    """oracle_rsqrt_newton on a geometric grid over the served range: relative error against v^-1/2 within twice the measured
    figure; beyond the grid, down to v = floor (var = -eps, the smallest v the layer can form) the result is finite and
    within 1 % of v^-1/2, as it is just below the largest variance served, 3 / x0^2."""
    grid = np.geomspace(W.VAR_SERVED[0], W.VAR_SERVED[1], 60)
    for seed in (1, 2, 3):
        r, vq = W.rsqrt_values(grid, seed)
        rel = np.abs(r * np.sqrt(vq) - 1)
        print("rsqrt_newton seed", seed, ": max relative error", rel.max(), "at v =", vq[rel.argmax()])
        assert rel.max() <= W.RSQRT_REL_TOL, rel.max()
        assert (r > 0).all()
    edge, eq = W.rsqrt_values([W.FLOOR / W.S_IT, (10 + W.FLOOR) / W.S_IT, 2.9e4])
    assert np.isfinite(edge).all() and (np.abs(edge * np.sqrt(eq) - 1) <= 0.01).all(), edge
    # fewer iterates do not reach the small end: STEPS is not slack
    short, _ = W.rsqrt_values([W.FLOOR / W.S_IT], steps=W.STEPS - 6)
    assert short[0] < 0.5 * eq[0] ** -0.5


def test_default_form_is_wrong_at_variance_100_and_the_wide_form_is_not():
    """The regression this form exists for: one group of variance 100 among unit-variance groups.  oracle_group_norm is off
    by more than 1 there (by orders of magnitude: its iteration changes sign at v = 21); the wide form is within its bound."""
    pf = 3
    g = torch.Generator().manual_seed(41)
    x = torch.randn(64, 72, generator=g)
    x[7] = (x[7] - x[7].mean()) / x[7].std(unbiased=False) * 10.0
    x = x.reshape(2, 64, 6, 6)
    w, b = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    err_d, var = W.layer_error(oracle_group_norm, pf, 1, x, w, b)
    err_w, _ = W.layer_error(W.oracle_group_norm_wide, pf, 1, x, w, b)
    assert 99 <= var[7] <= 101
    print("variance", var[7], ": default form max |error|", err_d[7].max(), ", wide form", err_w[7].max())
    assert err_d[7].max() > 1.0
    assert err_w.max() <= W.WIDE_LAYER_TOL[pf]


def walk(sd, images, blocks, pooling):
    d = RecordingDealer(0)
    W.oracle_forward_wide(ScheduleContext(d, 10, 3), numpy_sd(sd), images, blocks, pooling)
    return d.requests[len(S.share_order(list(sd.keys()))):]


@pytest.mark.parametrize("B", [1, 3])
def test_image_requests_of_a_wide_pass(B):
    """image_requests(wide_norm=True) equals what a walk of oracle_forward with the wide layer at every norm site asks its
    dealer for (mini network and 8-block ResNet-18 at 32 x 32); wide_norm=False is the list it was; the sizing functions
    follow the list."""
    images = np.zeros((B, 3, 32, 32), np.float32)
    for sd, blocks in ((group_mini(torch.Generator().manual_seed(31)), MINI_BLOCKS), (group_resnet18(32, 520), None)):
        arch = architecture_of(sd)
        got = image_requests(arch, 32, B, blocks, wide_norm=True)
        assert [flat((k, a)) for k, a, _ in got] == [flat(r) for r in walk(sd, images, blocks, "max")]
        assert all(kw == {"owner": None} for k, _, kw in got[1:] if k == "const_mask")
        old = image_requests(arch, 32, B, blocks)
        assert old == image_requests(arch, 32, B, blocks, wide_norm=False) != got
        sites = len(secure._norm_prefixes(arch, blocks or secure._default_blocks()))
        assert len(old) - len(got) == sites * (321 - 128)
        assert serving_bytes(arch, 32, B, blocks, wide_norm=True) == primitive_bytes(got) + primitive_bytes(got) // 8
        assert serving_bytes(arch, 32, B, blocks) == primitive_bytes(old) + primitive_bytes(old) // 8
        budget = serving_bytes(arch, 32, 2, blocks, wide_norm=True)
        assert largest_batch_that_fits(arch, 32, budget, blocks, wide_norm=True) == 2
        assert largest_batch_that_fits(arch, 32, budget, blocks) <= 2


def test_wide_norm_refusals():
    gn, bn = group_mini(torch.Generator().manual_seed(31)), mini_resnet(torch.Generator().manual_seed(21))
    for sd in (bn, secure.fold_batch_norm(bn)):
        arch = architecture_of(sd)
        assert norm_of(arch) in ("batch", "folded")
        with pytest.raises(ValueError, match="fold_norm"):
            image_requests(arch, 32, 1, MINI_BLOCKS, wide_norm=True)
        with pytest.raises(ValueError, match="fold_norm"):
            serving_bytes(arch, 32, 1, MINI_BLOCKS, wide_norm=True)
        with pytest.raises(ValueError, match="fold_norm"):
            secure.check_wide_norm(10, 3, norm_of(arch))
    for pf in (2, 7, 16):
        with pytest.raises(ValueError, match="precision_fractional"):
            secure.check_wide_norm(10, pf)
        with pytest.raises(ValueError, match="precision_fractional"):
            W.check_pf(pf)
    for pf in (3, 4, 5, 6):
        secure.check_wide_norm(10, pf)
    with pytest.raises(ValueError, match="base"):
        secure.check_wide_norm(2, 4)
    image_requests(architecture_of(gn), 32, 1, MINI_BLOCKS, wide_norm=True)


def test_cli_flag_logic():
    """inference.py's --wide_norm: off by default; without --encrypted_inference a warning and nothing else; a BatchNorm
    checkpoint ends the run naming --fold_norm; a precision outside 3..6 ends it naming --precision_fractional."""
    gn, bn = group_resnet18(32, 520), resnet18(32, 320)
    assert inference.wide_norm_choice(False, True, gn.keys(), 3) is False
    assert inference.wide_norm_choice(True, True, gn.keys(), 3) is True
    assert inference.wide_norm_choice(True, True, gn.keys(), 6) is True
    with pytest.warns(UserWarning, match="--wide_norm has no effect"):
        assert inference.wide_norm_choice(True, False, gn.keys(), 3) is False
    with pytest.warns(UserWarning, match="--wide_norm has no effect"):
        assert inference.wide_norm_choice(True, False, bn.keys(), 16) is False
    with pytest.raises(SystemExit, match="--fold_norm"):
        inference.wide_norm_choice(True, True, bn.keys(), 3)
    with pytest.raises(SystemExit, match="--precision_fractional 3 to 6"):
        inference.wide_norm_choice(True, True, gn.keys(), 16)


def test_cli_parser_knows_the_flag():
    """The flag is on inference.py's command line (its --help, which touches no GPU)."""
    r = subprocess.run([sys.executable, "inference.py", "--help"], cwd=inference.os.path.dirname(inference.__file__) or ".",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--wide_norm" in r.stdout, r.stderr[-500:]
