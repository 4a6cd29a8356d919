"""GPU: the frozen-BatchNorm backward kernels (csrc/bn_frozen.hip), element by element, against float64.

z comes from primia_bn_fwd_eval / primia_bn_fwd_eval_mask on the device and the reference takes its ReLU mask from that
stored z, so no element sits on the wrong side of the discontinuity; everything else of the reference is float64 from the
inputs rounded to the storage dtype.  With u = 2^-24 and u_out = 2^-8 (bf16) / 2^-24 (fp32):

    |dy - ref|        <= (u_out + 6u) |ref|            one output rounding + at most six fp32 roundings in rv + eps, the
                                                       square root, the divide and two products
    |ps_dbeta - ref|  <= HW u sum|g|                   an fp32 sum of HW terms in any order
    |ps_dgamma - ref| <= (HW + 6) u sum|g xhat|        ... plus the roundings of each term
    g_out             == mask * dz                     bitwise

The bounds are derived, not tuned.  The worst err / bound of every output is printed (`-s`).  (N, H) = (3, 6) and (130, 5)
run several slabs per sample + the finalize launch (the last slab ragged); (5, 1) and (4, 4) one slab per sample, whose
block writes the sums itself."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from primia_amd import _lib  # noqa: E402
from primia_amd._lib import PrimiaError, call, query  # noqa: E402
from tests.conv_bounds import check_guards  # noqa: E402

U = 2.0 ** -24
EPS = 1e-5
GUARD = 256
FILL = -123.0               # exact in bf16 and fp32, not a NaN: compared bitwise


def guarded(shape, dtype, dev):
    n = int(torch.Size(shape).numel())
    arena = torch.full((n + 2 * GUARD,), FILL, dtype=dtype, device=dev)
    out = arena[GUARD:GUARD + n]
    assert out.data_ptr() % 16 == 0
    out.fill_(float("nan"))
    return arena, out.view(shape)


def intact(arena, n):
    check_guards(arena.cpu(), GUARD, GUARD + n, FILL)


def make_case(dtype, N, H, C, relu, res, dev):
    HW = H * H
    g = torch.Generator().manual_seed(1000 * C + 10 * N + H)
    rnd = lambda t: t.to(dtype)
    t = dict(N=N, HW=HW, C=C, relu=relu, res=res, dtype=dtype, dt=_lib.dtype_code(dtype))
    t["y"] = rnd(torch.randn(N * HW, C, generator=g) * 2 + 0.3).to(dev)
    t["r"] = rnd(torch.randn(N * HW, C, generator=g)).to(dev) if res else None
    t["dz"] = rnd(torch.randn(N * HW, C, generator=g)).to(dev)
    t["gamma"] = (torch.rand(C, generator=g) + 0.5).to(dev)
    t["beta"] = torch.randn(C, generator=g).to(dev)
    t["rm"] = torch.randn(C, generator=g).to(dev)
    rv = torch.rand(C, generator=g) * 1.5 + 0.5
    rv[0], rv[1] = 0.0, 1e-3
    t["rv"] = rv.to(dev)
    t["wsb"] = query("primia_bn_frozen_workspace_bytes", N, HW, C)
    assert t["wsb"] > 0 and t["wsb"] % 4 == 0
    # forward on the device: the stored z (and, on residual layers, its mask bytes)
    z = torch.empty(N * HW, C, dtype=dtype, device=dev)
    call("primia_bn_fwd_eval", t["y"], t["r"], z, t["gamma"], t["beta"], t["rm"], t["rv"], N * HW, C, EPS, relu, t["dt"])
    t["z"] = z
    if relu and res:
        z2 = torch.empty_like(z)
        t["mask"] = torch.zeros(z.numel() * z.element_size() // 16, dtype=torch.uint8, device=dev)
        call("primia_bn_fwd_eval_mask", t["y"], t["r"], z2, t["mask"], t["gamma"], t["beta"], t["rm"], t["rv"], N * HW, C, EPS,
             t["dt"])
        assert torch.equal(z2, z)
    return t


def reference(t):
    """float64 from the rounded inputs; the mask from the stored z."""
    N, HW, C = t["N"], t["HW"], t["C"]
    d = lambda k: t[k].double().cpu()
    y, dz, gamma, rm, rv = d("y"), d("dz"), d("gamma"), d("rm"), d("rv")
    eps = float(torch.tensor(EPS, dtype=torch.float32))          # the float the kernel receives
    invstd = 1.0 / torch.sqrt(rv + eps)
    mask = (t["z"].float().cpu() > 0) if t["relu"] else torch.ones(N * HW, C, dtype=torch.bool)
    g = torch.where(mask, dz, torch.zeros_like(dz))
    xhat = (y - rm) * invstd
    per = lambda v: v.view(N, HW, C)
    return dict(mask=mask, g=g, dy=g * (gamma * invstd),
                psb=per(g).sum(1), psb_abs=per(g).abs().sum(1),
                psg=per(g * xhat).sum(1), psg_abs=per(g * xhat).abs().sum(1))


def run(t, entry, g_out=None, dz=None, ws_bytes=None):
    """One backward call into guarded outputs; returns (dy, ps_dgamma, ps_dbeta) after the guard bands were checked."""
    N, HW, C, dev = t["N"], t["HW"], t["C"], t["y"].device
    dz = t["dz"] if dz is None else dz
    a_dy, dy = guarded((N * HW, C), t["dtype"], dev)
    a_g, psg = guarded((N, C), torch.float32, dev)
    a_b, psb = guarded((N, C), torch.float32, dev)
    a_ws, ws = guarded((t["wsb"] // 4,), torch.float32, dev)
    wsb = t["wsb"] if ws_bytes is None else ws_bytes
    tail = (psg, psb, N, HW, C)
    if entry == "primia_bn_frozen_bwd":
        call(entry, t["y"], t["z"] if t["relu"] else None, dz, dy, g_out, t["gamma"], t["rm"], t["rv"], EPS, *tail, t["relu"], ws,
             wsb, t["dt"])
    elif entry == "primia_bn_frozen_bwd_mask":
        call(entry, t["y"], t["mask"], dz, dy, g_out, t["gamma"], t["rm"], t["rv"], EPS, *tail, ws, wsb, t["dt"])
    else:
        call(entry, t["y"], dz, dy, t["gamma"], t["beta"], t["rm"], t["rv"], EPS, *tail, ws, wsb, t["dt"])
    torch.cuda.synchronize()
    intact(a_dy, dy.numel())
    intact(a_g, psg.numel())
    intact(a_b, psb.numel())
    intact(a_ws, ws.numel())
    return dy.clone(), psg.clone(), psb.clone()


def worst(err, bound):
    """max err / bound; an element whose bound is 0 must be exact."""
    assert bool((err[bound == 0] == 0).all())
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,relu,res", [(64, 1, 0), (128, 1, 1), (512, 0, 0), (256, 1, 1)])
@pytest.mark.parametrize("N,H", [(3, 6), (130, 5), (5, 1), (4, 4)])
def test_frozen_bn_backward_per_element(cuda, dtype, C, relu, res, N, H):
    t = make_case(dtype, N, H, C, relu, res, cuda)
    ref = reference(t)
    HW = t["HW"]
    if relu:
        assert bool(ref["mask"].any()) and bool((~ref["mask"]).any()), "both mask values must occur"
    before = {k: t[k].clone() for k in ("y", "dz", "z")}
    g_out = torch.full_like(t["dz"], float("nan"))
    dy, psg, psb = run(t, "primia_bn_frozen_bwd", g_out=g_out)
    for k, v in before.items():
        assert torch.equal(t[k], v), f"input {k} changed"
    u_out = 2.0 ** -8 if dtype == torch.bfloat16 else U
    r_dy = worst((dy.double().cpu() - ref["dy"]).abs(), (u_out + 6 * U) * ref["dy"].abs())
    r_b = worst((psb.double().cpu() - ref["psb"]).abs(), HW * U * ref["psb_abs"])
    r_g = worst((psg.double().cpu() - ref["psg"]).abs(), (HW + 6) * U * ref["psg_abs"])
    print(f"frozen-bn dtype={str(dtype)[6:]} N={N} HW={HW} C={C} relu={relu} res={res}: worst err / bound dy {r_dy:.3g} "
          f"ps_dbeta {r_b:.3g} ps_dgamma {r_g:.3g}")
    assert r_dy <= 1.0 and r_b <= 1.0 and r_g <= 1.0
    want_g = torch.where(ref["mask"].to(cuda), t["dz"], torch.zeros_like(t["dz"]))
    assert torch.equal(g_out, want_g)
    # the other two mask sources: the same bits
    if relu and not res:
        dy2, psg2, psb2 = run(t, "primia_bn_frozen_relu_bwd")
        assert torch.equal(dy2, dy) and torch.equal(psg2, psg) and torch.equal(psb2, psb)
    if relu and res:
        g2 = torch.full_like(t["dz"], float("nan"))
        dy2, psg2, psb2 = run(t, "primia_bn_frozen_bwd_mask", g_out=g2)
        assert torch.equal(dy2, dy) and torch.equal(psg2, psg) and torch.equal(psb2, psb) and torch.equal(g2, want_g)
    # g_out aliasing dz: the same dy, and dz then holds g
    alias = t["dz"].clone()
    dy3, psg3, psb3 = run(t, "primia_bn_frozen_bwd", g_out=alias, dz=alias)
    assert torch.equal(dy3, dy) and torch.equal(psg3, psg) and torch.equal(psb3, psb) and torch.equal(alias, want_g)
    # run after run: the same bits
    dy4, psg4, psb4 = run(t, "primia_bn_frozen_bwd")
    assert torch.equal(dy4, dy) and torch.equal(psg4, psg) and torch.equal(psb4, psb)


def test_frozen_bn_backward_refuses_bad_calls(cuda):
    """No silent fallback: a short workspace is PRIMIA_ERR_WORKSPACE, a null y PRIMIA_ERR_ARG — and nothing is launched."""
    t = make_case(torch.bfloat16, 3, 6, 128, 1, 1, cuda)
    for entry in ("primia_bn_frozen_bwd", "primia_bn_frozen_bwd_mask"):
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_WORKSPACE"):
            run(t, entry, ws_bytes=t["wsb"] - 1)
    t2 = make_case(torch.float32, 3, 6, 64, 1, 0, cuda)
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_WORKSPACE"):
        run(t2, "primia_bn_frozen_relu_bwd", ws_bytes=0)
    for entry, tt in (("primia_bn_frozen_bwd", t), ("primia_bn_frozen_bwd_mask", t), ("primia_bn_frozen_relu_bwd", t2)):
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            N, HW, C = tt["N"], tt["HW"], tt["C"]
            dy = torch.empty_like(tt["y"])
            ps = torch.empty(N, C, device=cuda)
            ws = torch.empty(tt["wsb"], dtype=torch.uint8, device=cuda)
            if entry == "primia_bn_frozen_bwd":
                call(entry, None, tt["z"], tt["dz"], dy, None, tt["gamma"], tt["rm"], tt["rv"], EPS, ps, ps, N, HW, C, 1, ws,
                     tt["wsb"], tt["dt"])
            elif entry == "primia_bn_frozen_bwd_mask":
                call(entry, None, tt["mask"], tt["dz"], dy, None, tt["gamma"], tt["rm"], tt["rv"], EPS, ps, ps, N, HW, C, ws,
                     tt["wsb"], tt["dt"])
            else:
                call(entry, None, tt["dz"], dy, tt["gamma"], tt["beta"], tt["rm"], tt["rv"], EPS, ps, ps, N, HW, C, ws, tt["wsb"],
                     tt["dt"])
    # a channel count the chunk width does not divide
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
        bad = torch.empty(36, 12, dtype=torch.bfloat16, device=cuda)
        f = torch.ones(12, device=cuda)
        ps = torch.empty(1, 12, device=cuda)
        ws = torch.empty(4096, dtype=torch.uint8, device=cuda)
        call("primia_bn_frozen_bwd", bad, None, bad, bad.clone(), None, f, f, f, EPS, ps, ps, 1, 36, 12, 0, ws, 4096,
             _lib.PRIMIA_BF16)
