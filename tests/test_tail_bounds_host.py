"""tests/tail_bounds.py checked on the CPU: a torch stand-in plays each kernel of pool_fc_loss.hip / optim.hip in fp32, in the
kernel's operand order (first-wins window scan, per-row-group partial sums through "LDS", lane chains and the wave butterfly,
256 thread chains for the loss), stores in the compute type, and must stay inside every bound on every case of the tables
(worst err / bound printed with -s); planted faults, each at ONE position, must be rejected at that position.  No GPU, no
marker.

The stand-in's worst err / bound (torch CPU, its expf / logf; the MI355X figures are in DESIGN.md section 4).  Wherever one
rounding is the whole bound the worst case sits just under 1: every bf16 store (pools, gap / head backward: 0.99), the SGD
and Adam p (the final subtraction: 0.997 / 0.998), linear dx at out_f = 1 (one product against g(1): 0.94), bnsums' count
sum at ngrp = 1 (fp32, C = 1024: 0.997).  Elsewhere: pools fp32 0.48; feat 0.30; head logits 0.07; linear forward 0.009;
head backward fp32 0.46; bnsums bf16 0.35; cross entropy 0.02 (loss) and 0.48 (dlogits, soft); Adam exp_avg 0.97,
exp_avg_sq 0.985.

What the bounds cannot see: a wrong summation ORDER; in bf16, anything below ub |ref| — a truncating store is rejected at
the elements where it costs more than half an ulp (the test plants it at the worst one), about half of them; a dlogits row
whose class weight is 0 (reference and result are both 0 whatever the row's softmax is); Adam's p is judged from the stored
moments, so a wrong moment is seen by the moment's own check only."""
import pytest
import torch

from tests import tail_bounds as tb
from tests.tail_bounds import BF16, F32, BoundError, case_id, check_guards

ONE9 = torch.tensor(1.0 / 9.0, dtype=torch.float32)
NINF = float("-inf")


def show(what, c, ratio):
    print(f"tail-standin {what} case={c if isinstance(c, (int, str)) else case_id(c)} worst={ratio:.3g}")
    assert ratio <= 1.0


def store(v, dtype, truncate=False):
    if truncate and dtype == BF16:
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return tb.rnd(v, dtype)


def rejects(fn, *where):
    with pytest.raises(BoundError) as e:
        fn()
    for w in where:
        assert w in str(e.value), (w, str(e.value))
    return str(e.value)


def at(axes, pos):
    return "(" + ", ".join(f"{a}={v}" for a, v in zip(axes, pos)) + ")"


def plant(good, bad, pos):
    """good with ONE element taken from bad."""
    assert not torch.equal(good[pos].reshape(1), bad[pos].reshape(1)) or (good[pos] != good[pos]), "the fault does not show at this position"
    out = good.clone()
    out[pos] = bad[pos]
    return out


# ---- pools ---------------------------------------------------------------------------------------------------------------
def sim_maxpool_fwd(x, start=None, pad=NINF, last_wins=False):
    """start: the value `best` begins with (None: the first tap inside the image); pad: what a tap outside the image reads as
    (-inf: skipped)."""
    taps = tb.pool_taps(x, pad)
    best = torch.full(taps.shape[1:], NINF if start is None else start)
    pos = torch.full(taps.shape[1:], 255, dtype=torch.uint8)
    for k in range(9):
        inside = taps[k] != NINF
        nan = torch.isnan(taps[k])
        up = inside & (((pos == 255) if start is None else torch.zeros_like(inside)) | nan
                       | ((taps[k] >= best) if last_wins else (taps[k] > best)))
        best = torch.where(up, taps[k], best)
        pos = torch.where(up, torch.full_like(pos, k), pos)
    return best, pos


def sim_pool_bwd(dy, code, c, is_max):
    """The gather of pool3x3s2_bwd_kernel: a pixel adds its windows in (r, s) order, in fp32."""
    Ho, Wo = dy.shape[1:3]
    g = torch.zeros(c.N, c.H + 2, c.W + 2, c.C)
    for k in range(9):
        r, s = divmod(k, 3)
        g[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] += torch.where(code == k, dy, torch.zeros(())) if is_max else dy * ONE9
    return store(g[:, 1:c.H + 1, 1:c.W + 1].contiguous(), c.dtype)


def sim_avgpool_fwd(x, c, by_count=False, truncate=False):
    taps = tb.pool_taps(x, 0.0)
    s = torch.zeros(taps.shape[1:])
    for k in range(9):
        s = s + taps[k]
    if by_count:
        s = s / tb.pool_taps(torch.ones_like(x), 0.0).sum(0)
    else:
        s = s * ONE9
    return store(s, c.dtype, truncate)


@pytest.mark.parametrize("c", tb.POOL_CASES, ids=case_id)
def test_pool_standin(c):
    x, dy = tb.pool_operands(c)
    y, code = sim_maxpool_fwd(x)
    show("maxpool_fwd", c, tb.check_maxpool_fwd("maxpool", y, code, x))
    show("maxpool_bwd", c, tb.check_maxpool_bwd("maxpool", sim_pool_bwd(dy, code, c, True), dy, code, c))
    show("avgpool_fwd", c, tb.check_avgpool_fwd("avgpool", sim_avgpool_fwd(x, c), x, c))
    show("avgpool_bwd", c, tb.check_avgpool_bwd("avgpool", sim_pool_bwd(dy, None, c, False), dy, c))


@pytest.mark.parametrize("c", tb.POOL_NAN_CASES, ids=case_id)
def test_pool_nan(c):
    x, _ = tb.pool_nan_operands(c)
    y, code = sim_maxpool_fwd(x)
    assert torch.isnan(y[0, 1, 1, 6]) and torch.isnan(y[0, 0, 0, 1]) and torch.isnan(y[0, 2, 2, 5])
    tb.check_maxpool_fwd("maxpool", y, code, x)
    _, clean = sim_maxpool_fwd(torch.nan_to_num(x, nan=-5.0))
    yb = y.clone()
    yb[0, 1, 2, 0] = 1.0                                          # the window around (2, 3): the NaN swallowed
    rejects(lambda: tb.check_maxpool_fwd("maxpool", yb, code, x), at(tb.PIX_AXES, (0, 1, 2, 0)))
    cb = code.clone()
    cb[0, 0, 0, 1] = 8                                            # names a tap that is no NaN
    rejects(lambda: tb.check_maxpool_fwd("maxpool", y, cb, x), "argmax", at(tb.PIX_AXES, (0, 0, 0, 1)))
    assert clean.max() <= 8


def test_pool_faults():
    c = tb.PoolCase(2, 5, 12, 72, BF16)
    x, dy = tb.pool_operands(c)
    y, code = sim_maxpool_fwd(x)
    Ho, Wo = y.shape[1:3]
    chk = lambda y_, c_: (lambda: tb.check_maxpool_fwd("maxpool", y_, c_, x))  # noqa: E731
    # best started at 0: an interior window of the all-negative channel
    y0, _ = sim_maxpool_fwd(x, start=0.0)
    p = (1, 1, 2, tb.CH_NEG)
    rejects(chk(plant(y, y0, p), code), "maxpool y", at(tb.PIX_AXES, p))
    # padding read as 0: a border window of the same channel (interior windows are untouched by this fault)
    yp, cp = sim_maxpool_fwd(x, pad=0.0)
    assert torch.equal(yp[:, 1:Ho - 1, 1:Wo - 1], y[:, 1:Ho - 1, 1:Wo - 1])
    p = (0, 0, 3, tb.CH_NEG)
    rejects(chk(plant(y, yp, p), code), "maxpool y", at(tb.PIX_AXES, p))
    # H and W swapped in the input index: the 5 x 12 image read as 12 x 5 memory
    ys, _ = sim_maxpool_fwd(x.transpose(1, 2).contiguous().reshape(x.shape))
    p = (1, 2, 4, 9)
    rejects(chk(plant(y, ys, p), code), "maxpool y", at(tb.PIX_AXES, p))
    # last-wins ties: the constant channel names the last tap; the value is the same
    yl, cl = sim_maxpool_fwd(x, last_wins=True)
    assert torch.equal(yl, y)
    p = (0, 1, 1, tb.CH_CONST)
    assert int(code[p]) == 0 and int(cl[p]) == 8
    rejects(chk(y, plant(code, cl, p)), "maxpool argmax", at(tb.PIX_AXES, p))
    # first tap inside the image at the corner window of the constant channel is (1, 1) = 4
    assert int(code[0, 0, 0, tb.CH_CONST]) == 4
    # one argmax byte off
    p = (1, 2, 5, 40)
    rejects(chk(y, plant(code, (code + 1) % 9, p)), "maxpool argmax", at(tb.PIX_AXES, p))
    # the corner value wins the last window
    assert y[0, Ho - 1, Wo - 1, tb.CH_CORNER] == tb.CORNER_VALUE
    # backward through a wrong code
    dx = sim_pool_bwd(dy, code, c, True)
    dxb = sim_pool_bwd(dy, (code + 1) % 9, c, True)
    p = tuple((dx != dxb).nonzero()[7].tolist())
    rejects(lambda: tb.check_maxpool_bwd("maxpool", plant(dx, dxb, p), dy, code, c), at(tb.PIX_AXES, p))
    # avg-pool dividing by the taps inside the image: a border window
    ya, yc = sim_avgpool_fwd(x, c), sim_avgpool_fwd(x, c, by_count=True)
    assert torch.equal(yc[:, 1:Ho - 1, 1:Wo - 1], store(tb.pool_taps(x, 0.0).sum(0) / 9.0, BF16)[:, 1:Ho - 1, 1:Wo - 1])
    p = (0, 0, 2, 17)
    rejects(lambda: tb.check_avgpool_fwd("avgpool", plant(ya, yc, p), x, c), at(tb.PIX_AXES, p))
    # one output row left at its fill
    yr = ya.clone()
    yr[1, Ho - 1] = -123.0
    msg = rejects(lambda: tb.check_avgpool_fwd("avgpool", yr, x, c), f"{Wo * c.C} of", f"image=1, row={Ho - 1}")
    assert f"row={Ho - 2}" not in msg
    # a truncating bf16 store, at the element where it costs most
    yt = sim_avgpool_fwd(x, c, truncate=True)
    flat = int(((yt - ya).abs() / ya.abs().clamp_min(1e-30)).flatten().argmax())
    p = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), ya.shape))
    rejects(lambda: tb.check_avgpool_fwd("avgpool", plant(ya, yt, p), x, c), at(tb.PIX_AXES, p))
    # avg backward: a window's share dropped
    da = sim_pool_bwd(dy, None, c, False)
    db_ = da.clone()
    db_[0, 2, 2, 3] = 0.0
    rejects(lambda: tb.check_avgpool_bwd("avgpool", db_, dy, c), at(tb.PIX_AXES, (0, 2, 2, 3)))


# ---- head, linear ----------------------------------------------------------------------------------------------------------
def wave_tree(s):
    """s [..., 64] -> lane 0 of the xor butterfly (32, 16, ..., 1)."""
    while s.shape[-1] > 1:
        h = s.shape[-1] // 2
        s = s[..., :h] + s[..., h:]
    return s[..., 0]


def lane_dot(x, w):
    """[N, C] . [out_f, C] as linear_fwd_kernel / head_fwd_kernel: lanes stride the features, then the butterfly."""
    prod = x.unsqueeze(1) * w.unsqueeze(0)
    C = prod.shape[-1]
    pad = (-C) % 64
    prod = torch.cat([prod, torch.zeros(*prod.shape[:-1], pad)], -1).reshape(*prod.shape[:-1], -1, 64)
    s = torch.zeros(*prod.shape[:-2], 64)
    for k in range(prod.shape[-2]):
        s = s + prod[..., k, :]
    return wave_tree(s)


def sim_feat(x, c, fused=True, div=None):
    """fused: head_fwd_kernel's rpp row groups combined serially; else gap_fwd_kernel's one chain."""
    rpp = 256 // (c.C // tb.chunk(c.dtype)) if fused else 1
    part = torch.zeros(rpp, c.N, c.C)
    for p in range(c.HW):
        part[p % rpp] = part[p % rpp] + x[:, p]
    a = torch.zeros(c.N, c.C)
    for g in range(rpp):
        a = a + part[g]
    return a / torch.tensor(float(div or c.HW))


def sim_linear_fwd(x, w, b):
    y = lane_dot(x, w)
    return y + b if b is not None else y


def sim_linear_bwd(x, w, dy, skip=None):
    N, out_f = dy.shape
    dx = torch.zeros_like(x)
    for j in range(out_f):
        dx = dx + dy[:, j:j + 1] * w[j]
    red = torch.zeros(16, out_f, x.shape[1] + 1)
    x1 = torch.cat([x, torch.ones(N, 1)], 1)
    for n in range(N):
        if n != skip:
            red[n % 16] = red[n % 16] + dy[n].unsqueeze(1) * x1[n]
    s = red[0]
    for g in range(1, 16):
        s = s + red[g]
    return dx, s[:, :-1].contiguous(), s[:, -1].contiguous()


def sim_head_bwd(w, dy, c, truncate=False):
    a = torch.zeros(c.N, c.C)
    for j in range(c.out_f):
        a = a + dy[:, j:j + 1] * w[j]
    a = store(a / torch.tensor(float(c.HW)), c.dtype, truncate)
    return a.unsqueeze(1).expand(c.N, c.HW, c.C).contiguous()


def sim_bnsums(dx, bn_y, keep, mean, invstd, c):
    ngrp, _ = tb.bnsums_groups(c)
    vr = dx[:, 0]
    cnt, sx = torch.zeros(ngrp, c.N, c.C), torch.zeros(ngrp, c.N, c.C)
    for p in range(c.HW):
        g = p % ngrp
        cnt[g] = cnt[g] + keep[:, p].float()
        sx[g] = sx[g] + torch.where(keep[:, p], bn_y[:, p] - mean, torch.zeros(()))
    a0, a1 = torch.zeros(c.N, c.C), torch.zeros(c.N, c.C)
    for g in range(ngrp):
        a0, a1 = a0 + vr * cnt[g], a1 + vr * sx[g]
    return torch.stack([a0, a1 * invstd], 1)


@pytest.mark.parametrize("c", tb.HEAD_CASES + [tb.HEAD_FALLBACK_CASE], ids=case_id)
def test_head_standin(c):
    o = tb.head_operands(c)
    fused = c != tb.HEAD_FALLBACK_CASE
    feat = sim_feat(o["x"], c, fused)
    show("feat", c, tb.check_feat("head", feat, o["x"], c))
    show("gap_fwd", c, tb.check_feat("gap", sim_feat(o["x"], c, False), o["x"], c))
    show("logits", c, tb.check_linear_fwd("head", sim_linear_fwd(feat, o["w"], o["b"]), feat, o["w"], o["b"]))
    gb = store((o["dfeat"] / torch.tensor(float(c.HW))).unsqueeze(1).expand(c.N, c.HW, c.C).contiguous(), c.dtype)
    show("gap_bwd", c, tb.check_gap_bwd("gap", gb, o["dfeat"], c))
    if fused:
        dx = sim_head_bwd(o["w"], o["dy"], c)
        show("head_bwd", c, tb.check_head_bwd("head", dx, o["w"], o["dy"], c))
        sums = sim_bnsums(dx, o["bn_y"], o["keep"], o["mean"], o["invstd"], c)
        show("bnsums", c, tb.check_head_bnsums("head", sums, dx, o["bn_y"], o["keep"], o["mean"], o["invstd"], c))


@pytest.mark.parametrize("c", tb.LIN_CASES, ids=case_id)
def test_linear_standin(c):
    o = tb.lin_operands(c)
    b = None if c.omit == "b" else o["b"]
    show("linear_fwd", c, tb.check_linear_fwd("linear", sim_linear_fwd(o["x"], o["w"], b), o["x"], o["w"], b))
    dx, dw, db = sim_linear_bwd(o["x"], o["w"], o["dy"])
    show("linear_bwd", c, tb.check_linear_bwd("linear", None if c.omit == "dx" else dx, dw, None if c.omit == "db" else db,
                                             o["x"], o["w"], o["dy"]))


def test_head_faults():
    c = tb.HeadCase(3, 49, 512, 5, BF16)
    o = tb.head_operands(c)
    H3, S2 = tb.HEAD_AXES, ("sample", "channel")
    feat = sim_feat(o["x"], c)
    # feat divided by HW - 1
    p = (1, 300)
    rejects(lambda: tb.check_feat("head", plant(feat, sim_feat(o["x"], c, div=c.HW - 1), p), o["x"], c), at(S2, p))
    # one channel left at its fill
    fb = feat.clone()
    fb[:, 77] = -123.0
    rejects(lambda: tb.check_feat("head", fb, o["x"], c), f"{c.N} of", "channel=77")
    # a logit without its bias; the fifth logit missing
    y = sim_linear_fwd(feat, o["w"], o["b"])
    p = (2, 1)
    rejects(lambda: tb.check_linear_fwd("head", plant(y, sim_linear_fwd(feat, o["w"], None), p), feat, o["w"], o["b"]),
            at(("sample", "output"), p))
    yb = y.clone()
    yb[1, 4] = float("nan")
    rejects(lambda: tb.check_linear_fwd("head", yb, feat, o["w"], o["b"]), at(("sample", "output"), (1, 4)))
    # head backward: one pixel differs from the others of its sample; a truncating store
    dx = sim_head_bwd(o["w"], o["dy"], c)
    db_ = dx.clone()
    db_[1, 48, 5] = db_[1, 48, 6]
    rejects(lambda: tb.check_head_bwd("head", db_, o["w"], o["dy"], c), "pixel 0", at(H3, (1, 48, 5)))
    dt = sim_head_bwd(o["w"], o["dy"], c, truncate=True)
    ch = int(((dt - dx).abs() / dx.abs().clamp_min(1e-30))[0, 0].argmax())
    mixed = dx.clone()
    mixed[0, :, ch] = dt[0, :, ch]
    rejects(lambda: tb.check_head_bwd("head", mixed, o["w"], o["dy"], c), f"sample=0, pixel=0, channel={ch}")
    # bnsums: a count one short; the xhat sum without invstd
    args = (dx, o["bn_y"], o["keep"], o["mean"], o["invstd"], c)
    sums = sim_bnsums(*args)
    sb = sums.clone()
    sb[2, 0, 9] = sb[2, 0, 9] - dx[2, 0, 9]
    rejects(lambda: tb.check_head_bnsums("head", sb, *args), at(("sample", "which", "channel"), (2, 0, 9)))
    sb = sums.clone()
    sb[0, 1, 40] = sb[0, 1, 40] / o["invstd"][40]
    rejects(lambda: tb.check_head_bnsums("head", sb, *args), at(("sample", "which", "channel"), (0, 1, 40)))
    # linear backward: the 17th sample missing from dw; db in the wrong slot
    lc = tb.LinCase(17, 65, 5, "")
    lo = tb.lin_operands(lc)
    dxl, dw, db = sim_linear_bwd(lo["x"], lo["w"], lo["dy"])
    _, dw16, _ = sim_linear_bwd(lo["x"], lo["w"], lo["dy"], skip=16)
    p = (3, 64)
    rejects(lambda: tb.check_linear_bwd("linear", dxl, plant(dw, dw16, p), db, lo["x"], lo["w"], lo["dy"]), "dw", at(("output", "input"), p))
    dbb = db.clone()
    dbb[2] = db[1]
    rejects(lambda: tb.check_linear_bwd("linear", dxl, dw, dbb, lo["x"], lo["w"], lo["dy"]), "db", "(output=2)")
    dxb = dxl.clone()
    dxb[16, 64] = dxb[16, 64] - lo["dy"][16, 4] * lo["w"][4, 64]
    rejects(lambda: tb.check_linear_bwd("linear", dxb, dw, db, lo["x"], lo["w"], lo["dy"]), "dx", at(("sample", "input"), (16, 64)))


# ---- cross entropy ---------------------------------------------------------------------------------------------------------
def block_sum(per_sample):
    """[N] -> the 256 thread chains (thread t takes samples t, t + 256, ...), the wave butterflies, sh[0] + .. + sh[3]."""
    N = per_sample.shape[0]
    pad = torch.cat([per_sample, torch.zeros((-N) % 256)]).reshape(-1, 256)
    s = torch.zeros(256)
    for k in range(pad.shape[0]):
        s = s + pad[k]
    sh = wave_tree(s.reshape(4, 64))
    return ((sh[0] + sh[1]) + sh[2]) + sh[3]


def sim_xent(c, soft, weighted, by_n=False):
    o = tb.xent_operands(c)
    z, N, C = o["logits"], c.N, c.C
    cw = o["cw"] if weighted else None
    mx = z.max(1, keepdim=True).values
    e = torch.exp(z - mx)
    se = torch.zeros(N, 1)
    for k in range(C):
        se = se + e[:, k:k + 1]
    lse = mx + torch.log(se)
    inv = 1.0 / se
    if soft:
        t = o["soft"]
        a, l_, ts = torch.zeros(N, 1) if weighted else torch.ones(N, 1), torch.zeros(N, 1), torch.zeros(N, 1)
        for k in range(C):
            if weighted:
                a = a + cw[k] * t[:, k:k + 1]
            l_ = l_ - t[:, k:k + 1] * (z[:, k:k + 1] - lse)
            ts = ts + t[:, k:k + 1]
        den = torch.tensor(float(N))
        loss = block_sum((a * l_).flatten()) / den
        return loss, a / den * (e * inv * ts - t)
    t = o["hard"].unsqueeze(1)
    wt = cw[t] if weighted else torch.ones(N, 1)
    num, den = block_sum((wt * (lse - z.gather(1, t))).flatten()), block_sum(wt.flatten())
    hot = torch.zeros(N, C).scatter_(1, t, 1.0)
    return num / den, (wt / (torch.tensor(float(N)) if by_n else den)) * (e * inv - hot)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("c", tb.XENT_CASES, ids=case_id)
def test_xent_standin(c, soft, weighted):
    loss, dl = sim_xent(c, soft, weighted)
    wl, wd = tb.check_xent("xent", loss, dl, c, soft, weighted)
    show(f"xent_{'soft' if soft else 'hard'}{'_w' if weighted else ''} loss", c, wl)
    show(f"xent_{'soft' if soft else 'hard'}{'_w' if weighted else ''} dlogits", c, wd)


def test_xent_faults():
    c = tb.XentCase(257, 3)
    o = tb.xent_operands(c)
    assert (o["cw"] == 0).any() and (o["soft"].sum(1) - 1).abs().min() > 1e-3
    assert float((o["logits"].max(1).values - o["logits"].median(1).values).max()) >= 30.0
    loss, dl = sim_xent(c, False, True)
    # the gradient normalised by N instead of by the sum of the weights
    _, dn = sim_xent(c, False, True, by_n=True)
    row = int((o["cw"][o["hard"]] != 0).nonzero()[3])
    p = (row, 1)
    rejects(lambda: tb.check_xent("xent", loss, plant(dl, dn, p), c, False, True), "dlogits", at(("sample", "class"), p))
    # the 257th sample's row unwritten
    for soft in (False, True):
        loss, dl = sim_xent(c, soft, False)
        db_ = dl.clone()
        db_[256] = float("nan")
        rejects(lambda: tb.check_xent("xent", loss, db_, c, soft, False), "3 of", "sample=256")
        # ... and missing from the loss
        lo = tb.xent_ref(c, soft, False)
        per = 1.0 / c.N
        rejects(lambda: tb.check_xent("xent", loss * (1.0 - per), None, c, soft, False), "loss")
        assert lo[1] < 1e-4 * abs(lo[0])
    # soft: the softmax term without the targets' sum
    loss, dl = sim_xent(c, True, True)
    wrong = (o["soft"] * o["cw"]).sum(1, keepdim=True) / c.N * (torch.softmax(o["logits"], 1) - o["soft"])
    p = (101, 2)
    rejects(lambda: tb.check_xent("xent", loss, plant(dl, wrong, p), c, True, True), at(("sample", "class"), p))


# ---- flat kernels ------------------------------------------------------------------------------------------------------------
LR, WD, B1, B2, EPS = 0.1, 0.01, 0.9, 0.999, 1e-8


def sim_sgd(p, g, lr, wd):
    lr, wd = torch.tensor(lr, dtype=torch.float32), torch.tensor(wd, dtype=torch.float32)
    return p - lr * (g + wd * p)


def sim_adam(p, g, m, v, sc, bc2_on_numerator=False):
    b1, omb1, b2, omb2, eps, wd, step_size, isb = (torch.tensor(s, dtype=torch.float32) for s in sc)
    g = g + wd * p
    m = m * b1 + omb1 * g
    v = v * b2 + omb2 * g * g
    if bc2_on_numerator:
        return p - step_size * (m * isb / (torch.sqrt(v) + eps)), m, v
    return p - step_size * (m / (torch.sqrt(v) * isb + eps)), m, v


def covered(n, trips=None):
    """Elements flat_kernel updates when every block runs `trips` grid-stride trips at most (None: all)."""
    nv = n >> 2
    blocks = min(max((nv + 255) // 256, 1), tb.FLAT_BLOCK_CAP)
    keep = torch.zeros(n, dtype=torch.bool)
    top = nv if trips is None else min(nv, trips * blocks * 256)
    keep[:top * 4] = True
    keep[nv * 4:] = True
    assert n - nv * 4 <= blocks * 256
    return keep


@pytest.mark.parametrize("n", tb.FLAT_N)
def test_flat_standin(n):
    o = tb.flat_operands(n)
    assert covered(n).all()
    for wd in (0.0, WD):
        show(f"sgd wd={wd}", n, tb.check_sgd("sgd", sim_sgd(o["p"], o["g"], LR, wd), o["p"], o["g"], LR, wd))
    for step in tb.ADAM_STEPS if n < 10 ** 6 else tb.ADAM_STEPS[:1]:
        for wd in (0.0, WD):
            sc = tb.adam_scalars(1e-3, B1, B2, EPS, wd, step)
            pn, mn, vn = sim_adam(o["p"], o["g"], o["m"], o["v"], sc)
            for what, r in zip(("p", "exp_avg", "exp_avg_sq"), tb.check_adam("adam", pn, mn, vn, o["p"], o["g"], o["m"], o["v"], sc)):
                show(f"adam step={step} wd={wd} {what}", n, r)


def test_flat_exact_refs():
    """The exact references are the expressions the kernels state: product rounded before the sum, truncation toward zero."""
    x = torch.tensor([1.5, -1.5, 0.99999994, -0.0, 3.0e-5], dtype=torch.float32)
    assert tb.ref_fx_encode(x, 65536.0).tolist() == [98304, -98304, 65535, 0, 1]
    q = torch.tensor([2 ** 24 + 1, -(2 ** 24 + 3), 7], dtype=torch.int64)
    assert tb.ref_fx_decode(q, 2.0).tolist() == [2.0 ** 23, -(2.0 ** 23 + 2.0), 3.5]
    tb.check_exact("same", x, x.clone())
    rejects(lambda: tb.check_exact("sign of zero", x, x.abs() * torch.tensor([1.0, -1.0, 1.0, 1.0, 1.0])), "(i=3)")


def test_flat_faults():
    n = 4195507
    o = tb.flat_operands(n)
    p, g, m, v = o["p"], o["g"], o["m"], o["v"]
    # Adam without weight decay: exp_avg moves by (1 - b1) wd p; with bc2 on the numerator: p
    sc = tb.adam_scalars(1e-3, B1, B2, EPS, WD, 2)
    good = sim_adam(p, g, m, v, sc)
    nowd = sim_adam(p, g, m, v, tb.adam_scalars(1e-3, B1, B2, EPS, 0.0, 2))
    i = 1234567
    rejects(lambda: tb.check_adam("adam", good[0], plant(good[1], nowd[1], i), good[2], p, g, m, v, sc), "exp_avg", f"(i={i})")
    rejects(lambda: tb.check_adam("adam", good[0], good[1], plant(good[2], nowd[2], i), p, g, m, v, sc), "exp_avg_sq", f"(i={i})")
    num = sim_adam(p, g, m, v, sc, bc2_on_numerator=True)
    rejects(lambda: tb.check_adam("adam", plant(good[0], num[0], i), good[1], good[2], p, g, m, v, sc), "adam p", f"(i={i})")
    # ... and a p formed from the OLD moments while the new ones are stored
    stale = p - torch.tensor(sc[6], dtype=torch.float32) * (m / (torch.sqrt(v) * torch.tensor(sc[7], dtype=torch.float32) + EPS))
    rejects(lambda: tb.check_adam("adam", plant(good[0], stale, i), good[1], good[2], p, g, m, v, sc), "adam p", f"(i={i})")
    # an SGD tail element not updated (g = 0 there: only the weight decay moves it)
    pn = sim_sgd(p, g, LR, WD)
    rejects(lambda: tb.check_sgd("sgd", plant(pn, p, n - 1), p, g, LR, WD), f"(i={n - 1})")
    rejects(lambda: tb.check_sgd("sgd", plant(pn, p, n - 3), p, g, LR, WD), f"(i={n - 3})")
    # the last grid-stride trip dropped: 300 vectors stay as they were
    keep = covered(n, trips=2)
    lost = (~keep).nonzero().flatten()
    assert lost.numel() == 1200 and int(lost[0]) == 4194304 and int(lost[-1]) == n - 4
    msg = rejects(lambda: tb.check_sgd("sgd", torch.where(keep, pn, p), p, g, LR, WD), "of 4195507")
    bad = int(msg.split(" of ")[0].split()[-1])
    assert 1000 <= bad <= 1200 and all(4194304 <= int(s.split(")")[0]) < n - 3 for s in msg.split("(i=")[1:])
    xs = tb.ref_scale(o["x"], 0.3)
    rejects(lambda: tb.check_exact("scale", torch.where(keep, xs, o["x"]), xs), "1200 of", "(i=4194304)")
    # exact kernels: axpy with the product fused into the sum; encode rounding to nearest; one element each
    a = 0.3
    fused = (p.double() + o["x"].double() * tb.f32(a)).float()
    ya = tb.ref_axpy(p, o["x"], a)
    i = int((fused != ya).nonzero()[0])
    rejects(lambda: tb.check_exact("axpy", plant(ya, fused, i), ya), f"(i={i})")
    enc = tb.ref_fx_encode(o["x"], 65536.0)
    near = torch.round(o["x"] * torch.tensor(65536.0)).to(torch.int64)
    i = int((near != enc).nonzero()[0])
    rejects(lambda: tb.check_exact("fx_encode", plant(enc, near, i), enc), f"(i={i})")
    # one write past n
    arena = torch.full((256 + 5 + 256,), -123.0)
    arena[256:261] = 1.0
    assert check_guards(arena, 256, 261, -123.0) == 0.0
    arena[261] = 1.0
    rejects(lambda: check_guards(arena, 256, 261, -123.0), "end+0")
    arena[261] = -123.0
    arena[255] = 0.0
    rejects(lambda: check_guards(arena, 256, 261, -123.0), "out[-1]")


def test_tables():
    """The shapes reach the paths their comments name."""
    assert {c.C // tb.chunk(c.dtype) for c in tb.POOL_CASES} >= {1, 9, 18, 8, 16}
    assert any(c.H != c.W for c in tb.POOL_CASES) and any(c.H == 1 for c in tb.POOL_CASES) and any(c.W == 1 for c in tb.POOL_CASES)

    def head_ok(c):
        cpr = c.C // tb.chunk(c.dtype)
        return c.C % tb.chunk(c.dtype) == 0 and cpr <= 256 and 256 % cpr == 0 and c.C <= 2048

    assert all(head_ok(c) for c in tb.HEAD_CASES) and not head_ok(tb.HEAD_FALLBACK_CASE)
    tprs = {(c.dtype, c.C // tb.chunk(c.dtype)) for c in tb.HEAD_CASES}
    assert (BF16, 1) in tprs and (BF16, 256) in tprs and (F32, 256) in tprs
    assert any(c.out_f > 4 for c in tb.HEAD_CASES) and any(c.out_f == 1 for c in tb.HEAD_CASES)
    for c in tb.HEAD_CASES:                                        # head_bwd_bnsums' LDS stays under its 48 KiB
        assert (1 + 2 * tb.bnsums_groups(c)[0]) * c.C * 4 <= 48 * 1024
    assert {c.omit for c in tb.LIN_CASES} == {"", "b", "db", "dx"} and any(c.N > 16 for c in tb.LIN_CASES)
    n = tb.FLAT_N[-1]
    assert (n >> 2) > 2 * tb.FLAT_BLOCK_CAP * 256 and n % 4 == 3 and n * 4 <= 16 * 2 ** 20 + 2 ** 16
    assert tb.FX_N[-1] > tb.FLAT_BLOCK_CAP * 256 and tb.FX_N[-1] * 8 <= 16 * 2 ** 20
