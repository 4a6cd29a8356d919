"""The checkers of tests/conv_bounds.py checked, without a GPU.  A CPU stand-in plays the kernel: torch's fp32 convolution
on the rounded operands, the result stored in the compute type.  It must pass every checker on every shape of the GPU
suite (tests/test_gpu_conv_elementwise.py) — a bound the honest stand-in broke would be a wrong bound — and each of the
localized faults a tiled kernel produces, planted into its output, must be rejected."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_bounds as cb
from tests.conv_bounds import BoundError, ConvCase, case_id

IDS = dict(ids=case_id)


def store(v, dtype):
    return v if dtype == cb.F32 else v.to(torch.bfloat16)


def standin_fwd32(c):
    x, w, _, _, _ = cb.operands(c)
    return cb.nhwc(F.conv2d(x, w, None, c.stride, c.pad))


def standin_dgrad32(c, acc=False, masked=False):
    x, w, dy, base, keep = cb.operands(c)
    g = torch.nn.grad.conv2d_input(x.shape, w, dy, c.stride, c.pad)
    if acc:
        g = g + (base * keep if masked else base)
    return cb.nhwc(g)


def standin_wgrad(c):
    x, w, dy, _, _ = cb.operands(c)
    return torch.nn.grad.conv2d_weight(x, w.shape, dy, c.stride, c.pad)


def truncate_to_bf16(v):
    """fp32 -> bf16 by dropping the low 16 bits: rounding toward zero."""
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


# ---- the honest stand-in is inside every bound -------------------------------------------------------------------------
@pytest.mark.parametrize("c", cb.FWD_DGRAD_CASES + cb.STEM_CASES, **IDS)
def test_standin_forward_is_within_the_bound(c):
    r = cb.check_fwd(store(standin_fwd32(c), c.dtype), c)
    print(f"fwd {case_id(c)}: worst err/bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("c", cb.FWD_DGRAD_CASES, **IDS)
def test_standin_data_gradients_are_within_the_bound(c):
    _, _, _, base, keep = cb.operands(c)
    r0 = cb.check_dgrad(store(standin_dgrad32(c), c.dtype), c)
    r1 = cb.check_dgrad(store(standin_dgrad32(c, acc=True), c.dtype), c, base=base)
    r2 = cb.check_dgrad(store(standin_dgrad32(c, acc=True, masked=True), c.dtype), c, base=base, keep=keep)
    print(f"dgrad {case_id(c)}: worst err/bound {r0:.3f} plain, {r1:.3f} accumulating, {r2:.3f} masked")
    assert max(r0, r1, r2) <= 1.0


@pytest.mark.parametrize("c", cb.WGRAD_CASES, **IDS)
def test_standin_weight_gradient_is_within_the_bound(c):
    r = cb.check_wgrad(standin_wgrad(c), c)
    print(f"wgrad {case_id(c)}: worst err/bound {r:.3f}")
    assert r <= 1.0


# ---- planted faults ----------------------------------------------------------------------------------------------------
def test_a_dropped_tap_at_one_border_pixel_is_rejected():
    """One tap (all input channels) missing at one pixel of the top image row, on the shape with the most pixels of the suite
    (M = 12 593): the normwise error goes from 1.7e-3 to 3.8e-3, under the 1e-2 test_gpu_ops.py allows for bf16."""
    c = max(cb.FWD_DGRAD_CASES + cb.STEM_CASES, key=lambda c: c.N * cb.out_size(c) ** 2)
    assert c == cb.LH2_PERSISTENT_FWD
    x, w, _, _, _ = cb.operands(c)
    y = standin_fwd32(c).clone()
    n, row, col, r, s = 100, 0, 3, 1, 0                      # tap (1, 0) at output (0, 3) reads input (0, 2)
    good = store(y, c.dtype)
    y[n, row, col] -= w[:, :, r, s] @ x[n, :, row + r - 1, col + s - 1]
    bad = store(y, c.dtype)
    ref = cb.fwd_ref(c)[0]
    normwise = [((v.double() - ref).norm() / ref.norm()).item() for v in (good, bad)]
    print(f"dropped tap {case_id(c)}: normwise error {normwise[0]:.3e} untouched, {normwise[1]:.3e} with the tap dropped")
    assert normwise[1] < 1e-2                                 # test_gpu_ops.py's bf16 bound does not notice
    assert cb.check_fwd(good, c) <= 1.0
    with pytest.raises(BoundError) as e:
        cb.check_fwd(bad, c)
    # the failure names the pixel, and only that pixel's channels are counted
    assert f"image={n}, row={row}, col={col}" in str(e.value)
    count = int(str(e.value).split(": ")[1].split(" of ")[0])
    assert 0.9 * c.K <= count <= c.K, e.value


@pytest.mark.parametrize("c", [cb.LH_CASES[1], cb.C64_CASES[0], cb.S2_CASES[0]], **IDS)
@pytest.mark.parametrize("which", ["fwd", "dgrad"])
def test_two_swapped_neighbouring_pixels_are_rejected(c, which):
    v = store(standin_fwd32(c) if which == "fwd" else standin_dgrad32(c), c.dtype).clone()
    n, row, col = c.N - 1, v.shape[1] // 2, v.shape[2] - 2
    v[n, row, [col, col + 1]] = v[n, row, [col + 1, col]]
    with pytest.raises(BoundError) as e:
        (cb.check_fwd if which == "fwd" else cb.check_dgrad)(v, c)
    assert f"image={n}, row={row}, col={col}" in str(e.value) or f"image={n}, row={row}, col={col + 1}" in str(e.value)


@pytest.mark.parametrize("c", [cb.LH_CASES[0], cb.C64_CASES[1], cb.IGEMM_CASES[2], cb.IGEMM_CASES[4]], **IDS)
def test_a_channel_vector_rotated_by_one_is_rejected(c):
    v = store(standin_fwd32(c), c.dtype).clone()
    v[0, 0, 1] = torch.roll(v[0, 0, 1], 1)
    with pytest.raises(BoundError) as e:
        cb.check_fwd(v, c)
    assert "image=0, row=0, col=1" in str(e.value)


TRUNC_CASES = [c for c in cb.FWD_DGRAD_CASES + cb.STEM_CASES if c.dtype == cb.BF16 and c.C * c.R * c.R <= 2304]


@pytest.mark.parametrize("c", TRUNC_CASES, **IDS)
def test_a_truncating_store_is_rejected(c):
    """Rounding toward zero in place of round-to-nearest doubles the store's worst error (2 ub |ref|).  Only where the
    accumulation term 2 n uf A is small next to ub |ref| does that break the bound: every shape with n <= 2304 (worst
    err / bound 1.14 - 1.96 with this stand-in); at n = 4608 (C = 512, 3x3) the worst ratio is 0.74 — there the bound does
    NOT see a truncating store, which is why those shapes are not listed here."""
    assert cb.check_fwd(store(standin_fwd32(c), c.dtype), c) <= 1.0
    with pytest.raises(BoundError) as e:
        cb.check_fwd(truncate_to_bf16(standin_fwd32(c)), c)
    print(f"truncating store {case_id(c)}: {str(e.value).split(';')[0]}")


def test_one_missing_contribution_to_a_weight_gradient_is_rejected():
    """One output pixel's contribution removed from one tap of dw (a K x C outer product of that pixel's dy and x), at
    M = N Ho Wo = 320.  The bound is 2 n uf A with A ~ n tbar (tbar: the mean |term|), i.e. 2 n^2 uf tbar: a single term t
    is seen while |t| / tbar > 2 n^2 uf — 0.012 at n = 320, 0.076 at n = 800, 1 at n ~ 2900, 19 at the n = 12 544 of
    layer4 at batch 256.  Larger M cannot see one term; a kernel that loses a whole ROW of a tile loses about n / 100."""
    c = cb.C64_CASES[1]
    assert c.N * cb.out_size(c) ** 2 <= 800
    x, _, dy, _, _ = cb.operands(c)
    dw = standin_wgrad(c).clone()
    assert cb.check_wgrad(dw, c) <= 1.0
    n, ho, wo, r, s = 2, 3, 4, 0, 2
    dw[:, :, r, s] -= torch.outer(dy[n, :, ho, wo], x[n, :, ho + r - 1, wo + s - 1])
    with pytest.raises(BoundError) as e:
        cb.check_wgrad(dw, c)
    assert f"r={r}, s={s}" in str(e.value)
    count = int(str(e.value).split(": ")[1].split(" of ")[0])
    assert count > 0.5 * c.K * c.C, e.value


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("at", [0, 255, 256 + 75 * 128, 256 + 75 * 128 + 255])
def test_a_changed_guard_element_is_rejected(dtype, at):
    n = 75 * 128
    arena = torch.full((n + 512,), -123.0, dtype=dtype)
    arena[256:256 + n] = float("nan")
    assert cb.check_guards(arena, 256, 256 + n, -123.0) == 0.0
    arena[at] = -123.5                                        # one bit of the pattern
    with pytest.raises(BoundError) as e:
        cb.check_guards(arena, 256, 256 + n, -123.0)
    assert "1 elements" in str(e.value)
    assert (f"out[{at - 256}]" if at < 256 else f"end+{at - 256 - n}") in str(e.value)


def test_a_negative_zero_in_the_guard_band_is_seen_bitwise():
    arena = torch.zeros(600)
    assert cb.check_guards(arena, 256, 344, 0.0) == 0.0
    arena[10] = -0.0
    with pytest.raises(BoundError):
        cb.check_guards(arena, 256, 344, 0.0)


def test_a_nan_in_the_output_is_rejected():
    c = cb.LH_CASES[0]
    v = store(standin_fwd32(c), c.dtype).clone()
    v[2, 4, 4, 127] = float("nan")                            # the last element: a ragged tile's row never written
    with pytest.raises(BoundError) as e:
        cb.check_fwd(v, c)
    assert "image=2, row=4, col=4, channel=127" in str(e.value)
