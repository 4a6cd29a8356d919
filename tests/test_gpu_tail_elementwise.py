"""GPU: every pooling, head, loss and optimizer entry point of pool_fc_loss.hip and optim.hip, element by element, against float64
(tests/tail_bounds.py: references, bounds and their derivation; tests/test_tail_bounds_host.py: the checkers checked on a CPU
stand-in).  test_gpu_ops.py judges these kernels by ||a - b|| / ||b|| against torch fp32 at one or two shapes each; here every
output element keeps its own bound — or its exact bits — at the shapes that reach each loop trip and launch variant.

Every call goes through the C ABI.  Every output and in-place operand lives inside an arena with 256 elements of a fixed bit
pattern in front and behind, pre-filled with NaN (bytes: 0xff) where the call overwrites; after the call the slack and the
inputs are compared bit for bit.  The worst err / bound of every check is printed (`-s`); DESIGN.md keeps the table measured
on the MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from primia_amd import _lib  # noqa: E402
from primia_amd._lib import PrimiaError, call  # noqa: E402
from tests import tail_bounds as tb  # noqa: E402
from tests.tail_bounds import BF16, F32, case_id, check_guards, same_bits  # noqa: E402

GUARD = 256
FILL = {torch.float32: -123.0, torch.bfloat16: -123.0, torch.float64: -123.0, torch.uint8: 0xA5}   # exact, compared bitwise
UNSET = {torch.float32: float("nan"), torch.bfloat16: float("nan"), torch.float64: float("nan"), torch.uint8: 0xFF}
TORCH = {BF16: torch.bfloat16, F32: torch.float32}
f32 = torch.float32


class Arena:
    """An n-element output with guard bands; .out is the device view, .get() the CPU copy once the bands were found intact."""

    def __init__(self, n, dtype, dev, prefill=None):
        self.n = n
        self.arena = torch.full((GUARD + n + GUARD,), FILL[dtype], dtype=dtype, device=dev)
        self.out = self.arena[GUARD:GUARD + n]
        assert self.out.data_ptr() % 16 == 0
        if isinstance(prefill, torch.Tensor):
            self.out.copy_(prefill.reshape(-1))
        else:
            self.out.fill_(UNSET[dtype] if prefill is None else prefill)

    def get(self):
        host = self.arena.cpu()
        check_guards(host, GUARD, GUARD + self.n, FILL[host.dtype])
        return host[GUARD:GUARD + self.n]


class Intact:
    """Bitwise copies of a call's inputs, compared after it."""

    def __init__(self, **tensors):
        self.t = {k: v for k, v in tensors.items() if v is not None}
        self.copy = {k: v.clone() for k, v in self.t.items()}

    def check(self, what):
        torch.cuda.synchronize()
        for k, v in self.t.items():
            a, b = v, self.copy[k]
            if a.dtype == torch.int64:
                assert torch.equal(a, b), f"{what}: input {k} changed"
            else:
                assert same_bits(a, b), f"{what}: input {k} changed"


def report(entry, what, c, ratio):
    print(f"tail-bound entry={entry} {what} case={c if isinstance(c, (int, str)) else case_id(c)} worst={ratio:.3g}")
    assert ratio <= 1.0


def dev_of(t, dtype, dev):
    return t.reshape(-1).to(dtype).to(dev)


def untouched(arena):
    """The whole output still holds its NaN prefill."""
    return bool(torch.isnan(arena.get().float()).all())


# ---- 3x3 / 2 pools -------------------------------------------------------------------------------------------------------
def run_maxpool_fwd(cuda, c, x):
    dtype, dt = TORCH[c.dtype], _lib.dtype_code(TORCH[c.dtype])
    no = c.N * tb.pool_out(c.H) * tb.pool_out(c.W) * c.C
    x_d = dev_of(x, dtype, cuda)
    y, am = Arena(no, dtype, cuda), Arena(no, torch.uint8, cuda)
    ins = Intact(x=x_d)
    call("primia_maxpool3x3s2_fwd", x_d, y.out, am.out, c.N, c.H, c.W, c.C, dt)
    ins.check("maxpool_fwd")
    return y.get(), am


@pytest.mark.parametrize("c", tb.POOL_CASES, ids=case_id)
def test_pools(cuda, c):
    """C / CH = 1 (1x1x7x8 bf16, 2x5x6x4 fp32), 9 and 18 chunks (C = 72), H != W both ways, images one pixel high / wide, a
    single output pixel, more than one block (2x16x16x64).  Channels: negative everywhere, constant, post-ReLU, one large value
    in the last corner."""
    dtype, dt = TORCH[c.dtype], _lib.dtype_code(TORCH[c.dtype])
    x, dy = tb.pool_operands(c)
    nx, no = x.numel(), dy.numel()
    y, am = run_maxpool_fwd(cuda, c, x)
    code = am.get()
    report("maxpool3x3s2_fwd", "y+argmax", c, tb.check_maxpool_fwd("maxpool_fwd", y, code, x))

    dy_d = dev_of(dy, dtype, cuda)
    dx = Arena(nx, dtype, cuda)
    ins = Intact(dy=dy_d, argmax=am.arena)
    call("primia_maxpool3x3s2_bwd", dy_d, am.out, dx.out, c.N, c.H, c.W, c.C, dt)
    ins.check("maxpool_bwd")
    report("maxpool3x3s2_bwd", "dx", c, tb.check_maxpool_bwd("maxpool_bwd", dx.get(), dy, code, c))

    x_d = dev_of(x, dtype, cuda)
    y = Arena(no, dtype, cuda)
    ins = Intact(x=x_d)
    call("primia_avgpool3x3s2_fwd", x_d, y.out, c.N, c.H, c.W, c.C, dt)
    ins.check("avgpool_fwd")
    report("avgpool3x3s2_fwd", "y", c, tb.check_avgpool_fwd("avgpool_fwd", y.get(), x, c))

    dx = Arena(nx, dtype, cuda)
    ins = Intact(dy=dy_d)
    call("primia_avgpool3x3s2_bwd", dy_d, dx.out, c.N, c.H, c.W, c.C, dt)
    ins.check("avgpool_bwd")
    report("avgpool3x3s2_bwd", "dx", c, tb.check_avgpool_bwd("avgpool_bwd", dx.get(), dy, c))


@pytest.mark.parametrize("c", tb.POOL_NAN_CASES, ids=case_id)
def test_maxpool_nan(cuda, c):
    """A window holding a NaN yields NaN and names a NaN tap; every other window is exact."""
    x, _ = tb.pool_nan_operands(c)
    y, am = run_maxpool_fwd(cuda, c, x)
    assert int(torch.isnan(y.float()).sum()) == int(tb.maxpool_ref(x)[2].sum()) > 0
    report("maxpool3x3s2_fwd", "nan", c, tb.check_maxpool_fwd("maxpool_fwd", y, am.get(), x))


# ---- global average pool, head ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", tb.HEAD_CASES + [tb.HEAD_FALLBACK_CASE], ids=case_id)
def test_head(cuda, c):
    """primia_global_avgpool_fwd/_bwd, primia_head_fwd (feat, logits from the stored feat), primia_head_bwd,
    primia_head_bwd_bnsums.  out_f = 5 and 9: a wave's second and third logit; tpr = 1 (49x8 bf16: rpp = 256 > HW), tpr = 256
    (2048 bf16, 1024 fp32: rpp = 1); C = 192 fp32: primia_head_fwd falls back to the two general kernels, the backward entry
    points answer PRIMIA_ERR_ARG and write nothing."""
    dtype, dt = TORCH[c.dtype], _lib.dtype_code(TORCH[c.dtype])
    o = tb.head_operands(c)
    N, HW, C, out_f, CH = c.N, c.HW, c.C, c.out_f, tb.chunk(c.dtype)
    x_d = dev_of(o["x"], dtype, cuda)
    w_d, b_d, dy_d, dfeat_d = (o[k].to(cuda) for k in ("w", "b", "dy", "dfeat"))

    feat = Arena(N * C, f32, cuda)
    ins = Intact(x=x_d)
    call("primia_global_avgpool_fwd", x_d, feat.out, N, HW, C, dt)
    ins.check("global_avgpool_fwd")
    report("global_avgpool_fwd", "feat", c, tb.check_feat("gap_fwd", feat.get(), o["x"], c))

    dx = Arena(N * HW * C, dtype, cuda)
    ins = Intact(dfeat=dfeat_d)
    call("primia_global_avgpool_bwd", dfeat_d, dx.out, N, HW, C, dt)
    ins.check("global_avgpool_bwd")
    report("global_avgpool_bwd", "dx", c, tb.check_gap_bwd("gap_bwd", dx.get(), o["dfeat"], c))

    feat, logits = Arena(N * C, f32, cuda), Arena(N * out_f, f32, cuda)
    ins = Intact(x=x_d, w=w_d, b=b_d)
    call("primia_head_fwd", x_d, w_d, b_d, feat.out, logits.out, N, HW, C, out_f, dt)
    ins.check("head_fwd")
    fh = feat.get()
    report("head_fwd", "feat", c, tb.check_feat("head_fwd", fh, o["x"], c))
    report("head_fwd", "logits", c, tb.check_linear_fwd("head_fwd", logits.get(), fh.reshape(N, C), o["w"], o["b"]))

    mask_d = tb.mask_bytes(o["keep"], CH).to(cuda)
    y_d, mean_d, inv_d = dev_of(o["bn_y"], dtype, cuda), o["mean"].to(cuda), o["invstd"].to(cuda)
    if c == tb.HEAD_FALLBACK_CASE:
        dx, sums = Arena(N * HW * C, dtype, cuda), Arena(N * 2 * C, f32, cuda)
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_head_bwd", w_d, dy_d, dx.out, N, HW, C, out_f, dt)
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_head_bwd_bnsums", w_d, dy_d, dx.out, y_d, mask_d, mean_d, inv_d, sums.out, N, HW, C, out_f, dt)
        torch.cuda.synchronize()
        assert untouched(dx) and untouched(sums)
        return

    dx = Arena(N * HW * C, dtype, cuda)
    ins = Intact(w=w_d, dy=dy_d)
    call("primia_head_bwd", w_d, dy_d, dx.out, N, HW, C, out_f, dt)
    ins.check("head_bwd")
    dxh = dx.get()
    report("head_bwd", "dx", c, tb.check_head_bwd("head_bwd", dxh, o["w"], o["dy"], c))

    dx2, sums = Arena(N * HW * C, dtype, cuda), Arena(N * 2 * C, f32, cuda)
    ins = Intact(w=w_d, dy=dy_d, bn_y=y_d, mask=mask_d, mean=mean_d, invstd=inv_d)
    call("primia_head_bwd_bnsums", w_d, dy_d, dx2.out, y_d, mask_d, mean_d, inv_d, sums.out, N, HW, C, out_f, dt)
    ins.check("head_bwd_bnsums")
    assert same_bits(dx2.get(), dxh), "head_bwd_bnsums: dx differs by bits from primia_head_bwd"
    report("head_bwd_bnsums", "sums", c, tb.check_head_bnsums("head_bwd_bnsums", sums.get(), dxh.float(), o["bn_y"], o["keep"],
                                                             o["mean"], o["invstd"], c))


# ---- linear ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", tb.LIN_CASES, ids=case_id)
def test_linear(cuda, c):
    """in_f = 63 / 64 / 65 / 100 / 512: the bias column inside the last block of inputs, alone in a block of its own, and
    behind a ragged one; N = 17 and 40: a sample group's second and third trip; b, db and dx each passed as NULL once."""
    o = tb.lin_operands(c)
    N, in_f, out_f = c.N, c.in_f, c.out_f
    x_d, w_d, dy_d = (o[k].to(cuda) for k in ("x", "w", "dy"))
    b_h = None if c.omit == "b" else o["b"]
    b_d = None if b_h is None else b_h.to(cuda)
    y = Arena(N * out_f, f32, cuda)
    ins = Intact(x=x_d, w=w_d, b=b_d)
    call("primia_linear_fwd", x_d, w_d, b_d, y.out, N, in_f, out_f)
    ins.check("linear_fwd")
    report("linear_fwd", "y", c, tb.check_linear_fwd("linear_fwd", y.get(), o["x"], o["w"], b_h))

    dx, dw, db = Arena(N * in_f, f32, cuda), Arena(out_f * in_f, f32, cuda), Arena(out_f, f32, cuda)
    ins = Intact(x=x_d, w=w_d, dy=dy_d)
    call("primia_linear_bwd", x_d, w_d, dy_d, None if c.omit == "dx" else dx.out, dw.out, None if c.omit == "db" else db.out, N,
         in_f, out_f)
    ins.check("linear_bwd")
    dxh, dbh = dx.get(), db.get()
    if c.omit == "dx":
        assert bool(torch.isnan(dxh).all())
    if c.omit == "db":
        assert bool(torch.isnan(dbh).all())
    report("linear_bwd", "dx/dw/db", c, tb.check_linear_bwd("linear_bwd", None if c.omit == "dx" else dxh, dw.get(),
                                                           None if c.omit == "db" else dbh, o["x"], o["w"], o["dy"]))


# ---- cross entropy -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("c", tb.XENT_CASES, ids=case_id)
def test_xent(cuda, c, soft, weighted):
    """N = 65 / 257 / 600: a second wave, a thread's second and third sample; C = 1 and C = 16; every fifth row holds a logit
    30 above the rest; the weights hold a 0; the soft targets do not sum to 1.  Without dlogits the loss keeps its bits."""
    o = tb.xent_operands(c)
    entry = "primia_xent_soft" if soft else "primia_xent_hard"
    z_d = o["logits"].to(cuda)
    t_d = (o["soft"] if soft else o["hard"]).to(cuda)
    cw_d = o["cw"].to(cuda) if weighted else None
    loss, dl = Arena(1, f32, cuda), Arena(c.N * c.C, f32, cuda)
    ins = Intact(logits=z_d, target=t_d, cw=cw_d)
    call(entry, z_d, t_d, cw_d, loss.out, dl.out, c.N, c.C)
    ins.check(entry)
    lh = loss.get()
    wl, wd = tb.check_xent(entry, lh, dl.get(), c, soft, weighted)
    tag = f"{'soft' if soft else 'hard'}{'+cw' if weighted else ''}"
    report(entry[7:], f"loss {tag}", c, wl)
    report(entry[7:], f"dlogits {tag}", c, wd)
    loss2 = Arena(1, f32, cuda)
    call(entry, z_d, t_d, cw_d, loss2.out, None, c.N, c.C)
    assert same_bits(loss2.get(), lh)


# ---- flat kernels ------------------------------------------------------------------------------------------------------------
LR, WD, B1, B2, EPS = 0.1, 0.01, 0.9, 0.999, 1e-8
ADAM_LR = 1e-3


def hyper_words(cuda, lr, wd, step):
    h = Arena(8, f32, cuda)
    call("primia_opt_hyper_set", h.out, lr, wd, B1, B2, EPS, step)
    torch.cuda.synchronize()
    h.get()
    return h


@pytest.mark.parametrize("n", tb.FLAT_N)
def test_sgd(cuda, n):
    """n < 4: no vector body; 4 195 507: two full grid-stride trips, a ragged third, a three-element tail.  wd = 0 and != 0;
    primia_sgd_step_dev gives the bits of primia_sgd_step."""
    o = tb.flat_operands(n)
    g_d = o["g"].to(cuda)
    for wd in (0.0, WD):
        p = Arena(n, f32, cuda, o["p"])
        ins = Intact(g=g_d)
        call("primia_sgd_step", p.out, g_d, n, LR, wd)
        ins.check("sgd_step")
        ph = p.get()
        report("sgd_step", f"p wd={wd}", n, tb.check_sgd("sgd_step", ph, o["p"], o["g"], LR, wd))
        h = hyper_words(cuda, LR, wd, 0)
        p2 = Arena(n, f32, cuda, o["p"])
        ins = Intact(g=g_d, hyper=h.arena)
        call("primia_sgd_step_dev", p2.out, g_d, n, h.out)
        ins.check("sgd_step_dev")
        assert same_bits(p2.get(), ph), "sgd_step_dev differs by bits from sgd_step"
        report("sgd_step_dev", f"p wd={wd}", n, 0.0)


@pytest.mark.parametrize("step", tb.ADAM_STEPS)
@pytest.mark.parametrize("n", tb.FLAT_N)
def test_adam(cuda, n, step):
    """p, exp_avg and exp_avg_sq after ONE step (numbered 1, 2, 1000) from a given state that holds elements with g = 0, v = 0;
    primia_adam_step_dev gives the bits of primia_adam_step."""
    o = tb.flat_operands(n)
    g_d = o["g"].to(cuda)
    for wd in (0.0, WD):
        sc = tb.adam_scalars(ADAM_LR, B1, B2, EPS, wd, step)
        p, m, v = (Arena(n, f32, cuda, o[k]) for k in ("p", "m", "v"))
        ins = Intact(g=g_d)
        call("primia_adam_step", p.out, g_d, m.out, v.out, n, ADAM_LR, B1, B2, EPS, wd, step)
        ins.check("adam_step")
        ph, mh, vh = p.get(), m.get(), v.get()
        for what, r in zip(("p", "exp_avg", "exp_avg_sq"),
                           tb.check_adam("adam_step", ph, mh, vh, o["p"], o["g"], o["m"], o["v"], sc)):
            report("adam_step", f"{what} step={step} wd={wd}", n, r)
        h = hyper_words(cuda, ADAM_LR, wd, step)
        p2, m2, v2 = (Arena(n, f32, cuda, o[k]) for k in ("p", "m", "v"))
        ins = Intact(g=g_d, hyper=h.arena)
        call("primia_adam_step_dev", p2.out, g_d, m2.out, v2.out, n, h.out)
        ins.check("adam_step_dev")
        assert same_bits(p2.get(), ph) and same_bits(m2.get(), mh) and same_bits(v2.get(), vh), "adam_step_dev differs by bits"
        report("adam_step_dev", f"step={step} wd={wd}", n, 0.0)


@pytest.mark.parametrize("n", tb.FLAT_N)
def test_scale_axpy_divide(cuda, n):
    """Exact by bits: fl(x a); fl(y + fl(x a)), the product rounded before the sum; fl(x / d)."""
    o = tb.flat_operands(n)
    a, d = 0.3, 7.0
    x = Arena(n, f32, cuda, o["x"])
    call("primia_scale", x.out, n, a)
    report("scale", "x", n, tb.check_exact("scale", x.get(), tb.ref_scale(o["x"], a)))
    x_d = o["x"].to(cuda)
    y = Arena(n, f32, cuda, o["p"])
    ins = Intact(x=x_d)
    call("primia_axpy", y.out, x_d, n, a)
    ins.check("axpy")
    report("axpy", "y", n, tb.check_exact("axpy", y.get(), tb.ref_axpy(o["p"], o["x"], a)))
    x = Arena(n, f32, cuda, o["x"])
    call("primia_divide", x.out, n, d)
    report("divide", "x", n, tb.check_exact("divide", x.get(), tb.ref_divide(o["x"], d)))


@pytest.mark.parametrize("n", tb.FX_N)
def test_fx(cuda, n):
    """Exact: truncation toward zero of the fp32 product; fl(fl(q) / scale) with |q| beyond 2^24.  524 588: a ragged second
    grid-stride trip of the two kernels."""
    o = tb.flat_operands(n)
    scale = 65536.0
    x_d, q_d = o["x"].to(cuda), o["q"].to(cuda)
    q = Arena(n, torch.float64, cuda)                              # int64 words inside float64 guard bands
    ins = Intact(x=x_d)
    call("primia_fx_encode", x_d, q.out.view(torch.int64), n, scale)
    ins.check("fx_encode")
    report("fx_encode", "q", n, tb.check_exact("fx_encode", q.get().view(torch.int64), tb.ref_fx_encode(o["x"], scale)))
    x = Arena(n, f32, cuda)
    ins = Intact(q=q_d)
    call("primia_fx_decode", q_d, x.out, n, scale)
    ins.check("fx_decode")
    report("fx_decode", "x", n, tb.check_exact("fx_decode", x.get(), tb.ref_fx_decode(o["q"], scale)))
