"""GPU: every BatchNorm / GroupNorm entry point of bn.hip and gn.hip, element by element, against float64 (tests/norm_bounds.py:
references, bounds and their derivation; tests/test_norm_bounds_host.py: the checkers checked on a CPU stand-in).
test_gpu_ops.py judges these kernels by ||a - b|| / ||b|| against torch fp32 on well conditioned data, or shows that one
variant gives the bits of another; here every output element keeps its own bound, at the shapes that reach each launch variant.

Every call goes through the C ABI, in bf16 and fp32.  Every output lives inside an arena with a fixed bit pattern in front and
behind, pre-filled with NaN (bytes: 0xff) where the call overwrites; after the call the slack and the inputs are compared bit
for bit.  The workspace is filled with NaN.  Every BatchNorm shape carries an offset channel (mean = 16 std), an all-zero
channel, a constant channel, a channel with gamma = 0, one with negative gamma and one whose gamma is tiny against beta.
`chain` is the slab length the launch geometry gives (norm_bounds.bn_slab_rows / gn_chain, pinned by test_geometry), 1 where
the test forms the partial sums itself.  The worst err / bound of every check is printed (`-s`); DESIGN.md keeps the table
measured on the MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from primia_amd import _lib  # noqa: E402
from primia_amd._lib import call, query  # noqa: E402
from tests import norm_bounds as nb  # noqa: E402
from tests.conv_bounds import check_guards, same_bits  # noqa: E402
from tests.norm_bounds import BF16, F32, case_id  # noqa: E402

GUARD = 256
FILL = {torch.float32: -123.0, torch.bfloat16: -123.0, torch.uint8: 0xA5}      # exact in every type, compared bitwise
UNSET = {torch.float32: float("nan"), torch.bfloat16: float("nan"), torch.uint8: 0xFF}
TORCH = {BF16: torch.bfloat16, F32: torch.float32}
EPS, MOM = 1e-5, 0.1


class Arena:
    """An n-element output with guard bands; .out is the device view, .get() the CPU copy once the bands were found intact."""

    def __init__(self, n, dtype, dev, prefill=None, tail=GUARD):
        self.n = n
        self.arena = torch.full((GUARD + n + tail,), FILL[dtype], dtype=dtype, device=dev)
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
            assert same_bits(v, self.copy[k]), f"{what}: input {k} changed"


def report(entry, what, c, ratio):
    print(f"norm-bound entry={entry} {what} case={case_id(c)} worst={ratio:.3g}")
    assert ratio <= 1.0


def report3(entry, c, ratios, names=("dy", "dgamma", "dbeta")):
    for what, r in zip(names, ratios):
        report(entry, what, c, r)


def dev_of(t, dtype, dev):
    return t.reshape(-1).to(dtype).to(dev)


def workspace(nbytes, dev):
    assert nbytes % 4 == 0
    return torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev)


class Params:
    """gamma / beta / statistics buffers of one BatchNorm on the device."""

    def __init__(self, o, C, dev, suffix=""):
        self.gamma, self.beta = o["gamma" + suffix].to(dev), o["beta" + suffix].to(dev)
        self.rm0, self.rv0 = o["rm0"], o["rv0"]
        self.dev, self.C = dev, C

    def fresh(self):
        """(running_mean, running_var, save_mean, save_invstd) arenas."""
        f32 = torch.float32
        return (Arena(self.C, f32, self.dev, self.rm0), Arena(self.C, f32, self.dev, self.rv0), Arena(self.C, f32, self.dev),
                Arena(self.C, f32, self.dev))


def judge_stats(entry, c, st, bufs, p):
    rm, rv, sm, si = (b.get() for b in bufs)
    report(entry, "stats", c, nb.check_stats(entry, st, sm, si, rm, rv, p.rm0, p.rv0))
    return sm, si


# ---- BatchNorm forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", nb.BN_CASES, ids=case_id)
def test_bn_forward(cuda, c):
    """The forward forms with a statistics pass of their own: primia_bn_fwd_train (plain, and residual + ReLU), _mask, _pair.
    M = 32 805: the partial-block cap binds, 995 slabs of 33 rows against an unroll of 4; M = 65 573 gives every apply kernel
    a second, ragged grid-stride trip (296 chunks)."""
    dtype, dt = TORCH[c.dtype], _lib.dtype_code(TORCH[c.dtype])
    M, C, CH = c.M, c.C, nb.chunk(c.dtype)
    o = nb.bn_operands(c)
    y, res, yd = o["y"], o["res"], o["yd"]
    p, pd = Params(o, C, cuda), Params(o, C, cuda, "_d")
    y_d, res_d, yd_d = (dev_of(t, dtype, cuda) for t in (y, res, yd))
    rows = nb.bn_slab_rows(M)[1]
    st = nb.stats_ref(y, rows)
    n, nbytes = M * C, query("primia_bn_workspace_bytes", M, C)

    # primia_bn_fwd_train: plain, then residual + ReLU
    for r_h, r_d, relu in ((None, None, 0), (res, res_d, 1)):
        ws, z, bufs = workspace(nbytes, cuda), Arena(n, dtype, cuda), p.fresh()
        ins = Intact(y=y_d, res=r_d, gamma=p.gamma, beta=p.beta)
        call("primia_bn_fwd_train", y_d, r_d, z.out, p.gamma, p.beta, bufs[0].out, bufs[1].out, bufs[2].out, bufs[3].out, M, C, EPS,
             MOM, relu, ws, nbytes, dt)
        ins.check("fwd_train")
        judge_stats("bn_fwd_train", c, st, bufs, p)
        report("bn_fwd_train", f"z relu={relu}", c, nb.check_fwd("fwd_train", z.get(), y, st, o["gamma"], o["beta"], r_h, relu, c.dtype))

    # primia_bn_fwd_train_mask with its own statistics pass
    ws, z, mask, bufs = workspace(nbytes, cuda), Arena(n, dtype, cuda), Arena(n // CH, torch.uint8, cuda), p.fresh()
    ins = Intact(y=y_d, res=res_d, gamma=p.gamma, beta=p.beta)
    call("primia_bn_fwd_train_mask", y_d, res_d, z.out, mask.out, p.gamma, p.beta, bufs[0].out, bufs[1].out, bufs[2].out,
         bufs[3].out, None, 0, M, C, EPS, MOM, ws, nbytes, dt)
    ins.check("fwd_train_mask")
    judge_stats("bn_fwd_train_mask", c, st, bufs, p)
    zh = z.get()
    report("bn_fwd_train_mask", "z", c, nb.check_fwd("fwd_train_mask", zh, y, st, o["gamma"], o["beta"], res, 1, c.dtype))
    report("bn_fwd_train_mask", "mask", c, nb.check_mask("fwd_train_mask", mask.get(), zh.float().reshape(M, C), c.dtype))

    # primia_bn_fwd_train_pair, statistics passes of its own
    std = nb.stats_ref(yd, rows)
    ws, z, mask, bufs, bufsd = workspace(nbytes, cuda), Arena(n, dtype, cuda), Arena(n // CH, torch.uint8, cuda), p.fresh(), pd.fresh()
    ins = Intact(y2=y_d, yd=yd_d, gamma=p.gamma, beta=p.beta, gamma_d=pd.gamma, beta_d=pd.beta)
    call("primia_bn_fwd_train_pair", y_d, yd_d, z.out, mask.out, p.gamma, p.beta, bufs[0].out, bufs[1].out, bufs[2].out, bufs[3].out,
         None, 0, pd.gamma, pd.beta, bufsd[0].out, bufsd[1].out, bufsd[2].out, bufsd[3].out, None, 0, M, C, EPS, MOM, ws, nbytes, dt)
    ins.check("fwd_train_pair")
    judge_stats("bn_fwd_train_pair", c, st, bufs, p)
    judge_stats("bn_fwd_train_pair(d)", c, std, bufsd, pd)
    zh = z.get()
    report("bn_fwd_train_pair", "z", c, nb.check_fwd_pair("fwd_train_pair", zh, y, st, o["gamma"], o["beta"], yd, std, o["gamma_d"],
                                                           o["beta_d"], c.dtype))
    report("bn_fwd_train_pair", "mask", c, nb.check_mask("fwd_train_pair", mask.get(), zh.float().reshape(M, C), c.dtype))


@pytest.mark.parametrize("c", nb.BN_CASES, ids=case_id)
def test_bn_forward_given_statistics(cuda, c):
    """The forward forms that are handed their sums or statistics: primia_bn_fwd_train_from_sums, primia_bn_finalize_stats,
    primia_bn_fwd_train_apply_inline (mask + residual), primia_bn_fwd_eval and _eval_mask.  The partial sums are the test's own,
    float64 sums over row ranges rounded once: chain 1.  apply_inline takes its two-launch form where the grid has fewer blocks
    than C / 4 (M = 1, 33, 75) and the folded finalize (bn_inline_finalize_stats) elsewhere: 16 finalizing blocks at C = 64, 32 at
    C = 128, 64 at 32 805 x 256 — there among 2048 blocks that walk 3 (bf16) or 5 (fp32) grid-stride trips."""
    dtype, dt = TORCH[c.dtype], _lib.dtype_code(TORCH[c.dtype])
    M, C, CH = c.M, c.C, nb.chunk(c.dtype)
    o = nb.bn_operands(c)
    y, res = o["y"], o["res"]
    p = Params(o, C, cuda)
    y_d, res_d = dev_of(y, dtype, cuda), dev_of(res, dtype, cuda)
    n = M * C
    slots = 3
    sums = nb.row_range_sums(y.double(), y.double() ** 2, slots).to(cuda)
    st1 = nb.stats_ref(y, 1)
    z, bufs = Arena(n, dtype, cuda), p.fresh()
    ins = Intact(y=y_d, sums=sums, gamma=p.gamma, beta=p.beta)
    call("primia_bn_fwd_train_from_sums", y_d, None, z.out, p.gamma, p.beta, bufs[0].out, bufs[1].out, bufs[2].out, bufs[3].out, sums,
         slots, M, C, EPS, MOM, 1, dt)
    ins.check("fwd_train_from_sums")
    judge_stats("bn_fwd_train_from_sums", c, st1, bufs, p)
    report("bn_fwd_train_from_sums", "z", c, nb.check_fwd("from_sums", z.get(), y, st1, o["gamma"], o["beta"], None, 1, c.dtype))

    bufs = p.fresh()
    ins = Intact(sums=sums)
    call("primia_bn_finalize_stats", sums, slots, M, C, EPS, MOM, bufs[0].out, bufs[1].out, bufs[2].out, bufs[3].out)
    ins.check("bn_finalize_stats")
    judge_stats("bn_finalize_stats", c, st1, bufs, p)

    z, mask, bufs = Arena(n, dtype, cuda), Arena(n // CH, torch.uint8, cuda), p.fresh()
    flags = torch.zeros((C + 3) // 4, dtype=torch.int32, device=cuda)
    ins = Intact(y=y_d, res=res_d, sums=sums, gamma=p.gamma, beta=p.beta)
    call("primia_bn_fwd_train_apply_inline", y_d, res_d, z.out, mask.out, p.gamma, p.beta, bufs[0].out, bufs[1].out, bufs[2].out,
         bufs[3].out, sums, slots, M, C, EPS, MOM, 1, flags, dt)
    ins.check("fwd_train_apply_inline")
    judge_stats("bn_fwd_train_apply_inline", c, st1, bufs, p)
    zh = z.get()
    report("bn_fwd_train_apply_inline", "z", c, nb.check_fwd("apply_inline", zh, y, st1, o["gamma"], o["beta"], res, 1, c.dtype))
    report("bn_fwd_train_apply_inline", "mask", c, nb.check_mask("apply_inline", mask.get(), zh.float().reshape(M, C), c.dtype))

    # eval mode on given running statistics
    ste = nb.eval_stats(o["rm0"], o["rv0"])
    rm_d, rv_d = o["rm0"].to(cuda), o["rv0"].to(cuda)
    z = Arena(n, dtype, cuda)
    ins = Intact(y=y_d, res=res_d, rm=rm_d, rv=rv_d)
    call("primia_bn_fwd_eval", y_d, res_d, z.out, p.gamma, p.beta, rm_d, rv_d, M, C, EPS, 0, dt)
    ins.check("fwd_eval")
    report("bn_fwd_eval", "z", c, nb.check_fwd("eval", z.get(), y, ste, o["gamma"], o["beta"], res, 0, c.dtype, train=False))
    z, mask = Arena(n, dtype, cuda), Arena(n // CH, torch.uint8, cuda)
    call("primia_bn_fwd_eval_mask", y_d, res_d, z.out, mask.out, p.gamma, p.beta, rm_d, rv_d, M, C, EPS, dt)
    ins.check("fwd_eval_mask")
    zh = z.get()
    report("bn_fwd_eval_mask", "z", c, nb.check_fwd("eval_mask", zh, y, ste, o["gamma"], o["beta"], res, 1, c.dtype, train=False))
    report("bn_fwd_eval_mask", "mask", c, nb.check_mask("eval_mask", mask.get(), zh.float().reshape(M, C), c.dtype))


# ---- BatchNorm backward --------------------------------------------------------------------------------------------------
def bwd_outputs(n, C, dtype, dev, g_out=True, tail=GUARD):
    f32 = torch.float32
    return (Arena(n, dtype, dev, tail=tail), Arena(n, dtype, dev, tail=tail) if g_out else None, Arena(C, f32, dev), Arena(C, f32, dev))


@pytest.mark.parametrize("c", nb.BN_CASES, ids=case_id)
def test_bn_backward(cuda, c):
    """primia_bn_bwd (with z and g_out), _bwd_mask, _bwd_mask_from_sums and the bn2 half of _bwd_pair against ONE reference (the
    mask bytes were checked against the stored z: the same keep); primia_bn_relu_bwd_from_sums and primia_bn_relu_bwd with the keep
    they recompute from y; the downsample half of primia_bn_bwd_pair.  z, mask, save_mean and save_invstd come from primia_bn_fwd_train_mask
    / primia_bn_fwd_train in this test and are judged first.  fp32 at 32 805 x 256 has 2 099 520 chunks: the two-chunk apply
    kernel."""
    dtype, dt = TORCH[c.dtype], _lib.dtype_code(TORCH[c.dtype])
    M, C, CH = c.M, c.C, nb.chunk(c.dtype)
    o = nb.bn_operands(c)
    y, res, yd, dz = o["y"], o["res"], o["yd"], o["dz"]
    p, pd = Params(o, C, cuda), Params(o, C, cuda, "_d")
    y_d, res_d, yd_d, dz_d = (dev_of(t, dtype, cuda) for t in (y, res, yd, dz))
    rows = nb.bn_slab_rows(M)[1]
    n, nbytes = M * C, query("primia_bn_workspace_bytes", M, C)

    # forward: z, mask, statistics of bn2; statistics of the downsample branch
    ws, z, mask, bufs = workspace(nbytes, cuda), Arena(n, dtype, cuda), Arena(n // CH, torch.uint8, cuda), p.fresh()
    call("primia_bn_fwd_train_mask", y_d, res_d, z.out, mask.out, p.gamma, p.beta, bufs[0].out, bufs[1].out, bufs[2].out,
         bufs[3].out, None, 0, M, C, EPS, MOM, ws, nbytes, dt)
    st = nb.stats_ref(y, rows)
    sm, si = judge_stats("bn_fwd_train_mask", c, st, bufs, p)
    zh = z.get().float().reshape(M, C)
    report("bn_fwd_train_mask", "z", c, nb.check_fwd("fwd_train_mask", zh, y, st, o["gamma"], o["beta"], res, 1, c.dtype))
    nb.check_mask("fwd_train_mask", mask.get(), zh, c.dtype)
    ws, idn, bufsd = workspace(nbytes, cuda), Arena(n, dtype, cuda), pd.fresh()
    call("primia_bn_fwd_train", yd_d, None, idn.out, pd.gamma, pd.beta, bufsd[0].out, bufsd[1].out, bufsd[2].out, bufsd[3].out, M, C,
         EPS, MOM, 0, ws, nbytes, dt)
    smd, sid = judge_stats("bn_fwd_train(d)", c, nb.stats_ref(yd, rows), bufsd, pd)
    sm_d, si_d, smd_d, sid_d = bufs[2].out, bufs[3].out, bufsd[2].out, bufsd[3].out
    keep = zh > 0
    g = torch.where(keep, dz, torch.zeros(()))

    same_g = []

    def took(name, outs, chain, g_out=True):
        dy, go, dg, db = outs
        if go is not None and g_out:
            report(name, "g_out", c, nb.check_g_out(name, go.get(), dz, keep))
        same_g.append(nb.Bwd(name, dy.get(), dg.get(), db.get(), chain))

    ws, outs = workspace(nbytes, cuda), bwd_outputs(n, C, dtype, cuda)
    ins = Intact(y=y_d, z=z.out, dz=dz_d, gamma=p.gamma, sm=sm_d, si=si_d)
    call("primia_bn_bwd", y_d, z.out, dz_d, outs[0].out, outs[1].out, p.gamma, sm_d, si_d, outs[2].out, outs[3].out, M, C, 1, ws,
         nbytes, dt)
    ins.check("bn_bwd")
    took("bn_bwd", outs, rows)

    ws, outs = workspace(nbytes, cuda), bwd_outputs(n, C, dtype, cuda)
    ins = Intact(y=y_d, mask=mask.out, dz=dz_d, gamma=p.gamma, sm=sm_d, si=si_d)
    call("primia_bn_bwd_mask", y_d, mask.out, dz_d, outs[0].out, outs[1].out, p.gamma, sm_d, si_d, outs[2].out, outs[3].out, M, C, ws,
         nbytes, dt)
    ins.check("bn_bwd_mask")
    took("bn_bwd_mask", outs, rows)

    slots = 5
    xhat = (y.double() - sm.double()) * si.double()
    sums = nb.row_range_sums(g.double(), g.double() * xhat, slots).to(cuda)
    outs = bwd_outputs(n, C, dtype, cuda)
    ins = Intact(y=y_d, mask=mask.out, dz=dz_d, sums=sums)
    call("primia_bn_bwd_mask_from_sums", y_d, mask.out, dz_d, outs[0].out, outs[1].out, p.gamma, sm_d, si_d, outs[2].out, outs[3].out,
         sums, slots, M, C, dt)
    ins.check("bn_bwd_mask_from_sums")
    took("bn_bwd_mask_from_sums", outs, 1)

    # primia_bn_bwd_pair keeps THREE sums per partial block where primia_bn_workspace_bytes counts two (bn.hip:1379, :1712;
    # include/primia_hip.h: "workspace >= 1024 * 3 * C floats")
    ws3 = workspace(nbytes * 3 // 2, cuda)
    outs, outsd = bwd_outputs(n, C, dtype, cuda, g_out=False), bwd_outputs(n, C, dtype, cuda, g_out=False)
    ins = Intact(y2=y_d, yd=yd_d, dz=dz_d, mask=mask.out, sm=sm_d, si=si_d, smd=smd_d, sid=sid_d)
    call("primia_bn_bwd_pair", y_d, yd_d, dz_d, mask.out, outs[0].out, outsd[0].out, p.gamma, sm_d, si_d, pd.gamma, smd_d, sid_d,
         outs[2].out, outs[3].out, outsd[2].out, outsd[3].out, M, C, ws3, ws3.numel() * 4, dt)
    ins.check("bn_bwd_pair")
    took("bn_bwd_pair", outs, rows)

    for out, r in zip(same_g, nb.check_bn_bwd_all(same_g, y, g, o["gamma"], sm, si, c.dtype)):
        report3(out.name, c, r)
    report3("bn_bwd_pair(d)", c, nb.check_bn_bwd("bn_bwd_pair(d)", outsd[0].get(), outsd[2].get(), outsd[3].get(), yd, g, o["gamma_d"],
                                                  smd, sid, rows, c.dtype))

    # no residual: the ReLU decision is recomputed from y
    keep_r = nb.relu_keep(y, sm, si, o["gamma"], o["beta"])
    g_r = torch.where(keep_r, dz, torch.zeros(()))
    sums = nb.row_range_sums(g_r.double(), g_r.double() * xhat, slots).to(cuda)
    outs = bwd_outputs(n, C, dtype, cuda, g_out=False)
    ins = Intact(y=y_d, dz=dz_d, sums=sums, beta=p.beta)
    call("primia_bn_relu_bwd_from_sums", y_d, dz_d, outs[0].out, p.gamma, p.beta, sm_d, si_d, outs[2].out, outs[3].out, sums, slots, M,
         C, dt)
    ins.check("bn_relu_bwd_from_sums")
    ws, outs2 = workspace(nbytes, cuda), bwd_outputs(n, C, dtype, cuda, g_out=False)
    ins = Intact(y=y_d, dz=dz_d, beta=p.beta, sm=sm_d, si=si_d)
    call("primia_bn_relu_bwd", y_d, dz_d, outs2[0].out, p.gamma, p.beta, sm_d, si_d, outs2[2].out, outs2[3].out, M, C, ws, nbytes, dt)
    ins.check("bn_relu_bwd")
    same_g = [nb.Bwd("bn_relu_bwd_from_sums", outs[0].get(), outs[2].get(), outs[3].get(), 1),
              nb.Bwd("bn_relu_bwd", outs2[0].get(), outs2[2].get(), outs2[3].get(), rows)]
    for out, r in zip(same_g, nb.check_bn_bwd_all(same_g, y, g_r, o["gamma"], sm, si, c.dtype)):
        report3(out.name, c, r)


@pytest.mark.parametrize("c", nb.TWO_CHUNK_CASES, ids=case_id)
def test_bn_two_chunk_backward(cuda, c):
    """bn_bwd_apply_kernel<T, 2> (bn.hip:996): 2 097 448 chunks in bf16 — four full trips' worth plus 296: the third trip has
    296 live threads whose second chunk is clamped — and 2 097 744 in fp32.  primia_bn_bwd_mask with g_out,
    primia_bn_bwd_mask_from_sums and primia_bn_relu_bwd_from_sums (the *_from_sums forms take the two-chunk kernel in bf16 only,
    bn.hip:1751-1765, :1782-1796).  The backward pass takes save_mean / save_invstd and the mask as inputs: here they are the
    float64 statistics rounded to fp32 and a random mask, so no forward pass over 17 M elements is needed.  dy and g_out keep a
    guard band of one grid stride (2048 x 256 chunks) behind them: a second chunk stored without the `q >= nchunks` test lands
    there (test_norm_bounds_host.py::test_two_chunk_walk)."""
    dtype, dt = TORCH[c.dtype], _lib.dtype_code(TORCH[c.dtype])
    M, C, CH = c.M, c.C, nb.chunk(c.dtype)
    assert nb.two_chunk(M, C, c.dtype)
    o = nb.bn_operands(c)
    y, dz, keep = o["y"], o["dz"], o["keep"]
    rows = nb.bn_slab_rows(M)[1]
    st = nb.stats_ref(y, rows)
    sm, si = st.mean.reshape(-1).float(), st.invstd.reshape(-1).float()
    gamma_d, beta_d, sm_d, si_d = o["gamma"].to(cuda), o["beta"].to(cuda), sm.to(cuda), si.to(cuda)
    y_d, dz_d = dev_of(y, dtype, cuda), dev_of(dz, dtype, cuda)
    mask_d = nb.mask_bytes(keep, CH).to(cuda)
    n, nbytes = M * C, query("primia_bn_workspace_bytes", M, C)
    tail = 2048 * 256 * CH + GUARD
    g = torch.where(keep, dz, torch.zeros(()))

    ws, outs = workspace(nbytes, cuda), bwd_outputs(n, C, dtype, cuda, tail=tail)
    ins = Intact(y=y_d, mask=mask_d, dz=dz_d, sm=sm_d, si=si_d)
    call("primia_bn_bwd_mask", y_d, mask_d, dz_d, outs[0].out, outs[1].out, gamma_d, sm_d, si_d, outs[2].out, outs[3].out, M, C, ws,
         nbytes, dt)
    ins.check("bn_bwd_mask")
    report("bn_bwd_mask", "g_out", c, nb.check_g_out("bn_bwd_mask", outs[1].get(), dz, keep))
    same_g = [nb.Bwd("bn_bwd_mask", outs[0].get(), outs[2].get(), outs[3].get(), rows)]
    del outs

    slots = 7
    xhat = (y.double() - sm.double()) * si.double()
    sums = nb.row_range_sums(g.double(), g.double() * xhat, slots).to(cuda)
    outs = bwd_outputs(n, C, dtype, cuda, tail=tail)
    ins = Intact(y=y_d, mask=mask_d, dz=dz_d, sums=sums)
    call("primia_bn_bwd_mask_from_sums", y_d, mask_d, dz_d, outs[0].out, outs[1].out, gamma_d, sm_d, si_d, outs[2].out, outs[3].out,
         sums, slots, M, C, dt)
    ins.check("bn_bwd_mask_from_sums")
    report("bn_bwd_mask_from_sums", "g_out", c, nb.check_g_out("bn_bwd_mask_from_sums", outs[1].get(), dz, keep))
    same_g.append(nb.Bwd("bn_bwd_mask_from_sums", outs[0].get(), outs[2].get(), outs[3].get(), 1))
    del outs
    for out, r in zip(same_g, nb.check_bn_bwd_all(same_g, y, g, o["gamma"], sm, si, c.dtype)):
        report3(out.name, c, r)
    del same_g

    keep_r = nb.relu_keep(y, sm, si, o["gamma"], o["beta"])
    g_r = torch.where(keep_r, dz, torch.zeros(()))
    sums = nb.row_range_sums(g_r.double(), g_r.double() * xhat, slots).to(cuda)
    del xhat
    outs = bwd_outputs(n, C, dtype, cuda, g_out=False, tail=tail)
    ins = Intact(y=y_d, dz=dz_d, sums=sums)
    call("primia_bn_relu_bwd_from_sums", y_d, dz_d, outs[0].out, gamma_d, beta_d, sm_d, si_d, outs[2].out, outs[3].out, sums, slots, M,
         C, dt)
    ins.check("bn_relu_bwd_from_sums")
    report3("bn_relu_bwd_from_sums", c, nb.check_bn_bwd("bn_relu_bwd_from_sums", outs[0].get(), outs[2].get(), outs[3].get(), y, g_r,
                                                         o["gamma"], sm, si, 1, c.dtype))


# ---- the fused stem tail ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", nb.POOL_CASES, ids=case_id)
def test_bn_stem_tail(cuda, c):
    """primia_bn_relu_maxpool_fwd, _fwd_from_sums, _bwd and _bwd_from_sums, C = 64.  H = 16 pools to a width of 8 (two windows per
    thread), H = 9 to 5 and H = 14 to 7 (one); even H takes bn_relu_pool_bwd_apply2x2_kernel, H = 9 the generic apply kernel.
    Channels 3 (gamma = 0) and 5 (gamma = 2^-8, beta = 1) are not pool_xhat_recoverable: their dgamma comes from y at the argmax
    positions."""
    dtype, dt = TORCH[c.dtype], _lib.dtype_code(TORCH[c.dtype])
    N, H, C = c.N, c.H, c.C
    M, Ho = N * H * H, nb.pool_out(H)
    Mp = N * Ho * Ho
    o = nb.pool_operands(c)
    y, dp, gamma, beta = o["y"], o["dp"], o["gamma"], o["beta"]
    p = Params(o, C, cuda)
    y_d, dp_d = dev_of(y, dtype, cuda), dev_of(dp, dtype, cuda)
    nbytes = query("primia_bn_workspace_bytes", M, C)
    rows = nb.bn_slab_rows(M)[1]

    def judge_fwd(entry, st, pooled, am, bufs):
        sm, si = judge_stats(entry, c, st, bufs, p)
        ref, E, _ = nb.affine_ref(y, st, gamma, beta)
        ph, ah = pooled.get(), am.get()
        report(entry, "pooled", c, nb.check_pool_fwd(entry, ph, ah, ref.clamp_min(0.0).reshape(N, H, H, C), E.reshape(N, H, H, C), c.dtype))
        return sm, si, ph, ah

    ws, pooled, am, bufs = workspace(nbytes, cuda), Arena(Mp * C, dtype, cuda), Arena(Mp * C, torch.uint8, cuda), p.fresh()
    ins = Intact(y=y_d, gamma=p.gamma, beta=p.beta)
    call("primia_bn_relu_maxpool_fwd", y_d, pooled.out, am.out, p.gamma, p.beta, bufs[0].out, bufs[1].out, bufs[2].out, bufs[3].out, N,
         H, H, C, EPS, MOM, ws, nbytes, dt)
    ins.check("bn_relu_maxpool_fwd")
    sm, si, ph, ah = judge_fwd("bn_relu_maxpool_fwd", nb.stats_ref(y, rows), pooled, am, bufs)

    slots = 3
    sums = nb.row_range_sums(y.double(), y.double() ** 2, slots).to(cuda)
    pooled1, am1, bufs1 = Arena(Mp * C, dtype, cuda), Arena(Mp * C, torch.uint8, cuda), p.fresh()
    ins = Intact(y=y_d, sums=sums)
    call("primia_bn_relu_maxpool_fwd_from_sums", y_d, pooled1.out, am1.out, p.gamma, p.beta, bufs1[0].out, bufs1[1].out, bufs1[2].out,
         bufs1[3].out, sums, slots, N, H, H, C, EPS, MOM, dt)
    ins.check("bn_relu_maxpool_fwd_from_sums")
    judge_fwd("bn_relu_maxpool_fwd_from_sums", nb.stats_ref(y, 1), pooled1, am1, bufs1)

    # backward through the kernel's own argmax codes
    keep = nb.relu_keep(y, sm, si, gamma, beta)
    g, ga = (t.reshape(M, C) * keep for t in nb.pool_scatter(dp, ah, N, H, C))
    rows_p = nb.bn_slab_rows(Mp)[1]
    sm_d, si_d = bufs[2].out, bufs[3].out
    ws, outs = workspace(nbytes, cuda), bwd_outputs(M * C, C, dtype, cuda, g_out=False)
    ins = Intact(y=y_d, pooled=pooled.out, dp=dp_d, argmax=am.out, sm=sm_d, si=si_d)
    call("primia_bn_relu_maxpool_bwd", y_d, pooled.out, dp_d, am.out, outs[0].out, p.gamma, p.beta, sm_d, si_d, outs[2].out, outs[3].out,
         N, H, H, C, ws, nbytes, dt)
    ins.check("bn_relu_maxpool_bwd")
    report3("bn_relu_maxpool_bwd", c, nb.check_bn_bwd("bn_relu_maxpool_bwd", outs[0].get(), outs[2].get(), outs[3].get(), y, g, gamma, sm,
                                                       si, rows_p, c.dtype, g_abs=ga, pooled_beta=beta))

    # ... with the pooled-resolution sums formed by the test: float64, exact xhat, a zero second sum where the kernel is to read y
    xhat = (y.double() - sm.double()) * si.double()
    rec = gamma.abs() >= 2.0 ** -6 * beta.abs().clamp_min(1e-30)
    sums = nb.row_range_sums(g, g * xhat * rec, slots).to(cuda)
    dg, db = Arena(C, torch.float32, cuda), Arena(C, torch.float32, cuda)
    ins = Intact(y=y_d, pooled=pooled.out, dp=dp_d, argmax=am.out, sums=sums)
    call("primia_bn_relu_maxpool_bwd_from_sums", y_d, pooled.out, dp_d, am.out, p.gamma, p.beta, sm_d, si_d, dg.out, db.out, sums, slots,
         N, H, H, C, dt)
    ins.check("bn_relu_maxpool_bwd_from_sums")
    report3("bn_relu_maxpool_bwd_from_sums", c, nb.check_bn_bwd("bn_relu_maxpool_bwd_from_sums", None, dg.get(), db.get(), y, g, gamma, sm,
                                                                 si, 1, c.dtype, g_abs=ga))


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", nb.GN_CASES, ids=case_id)
def test_groupnorm(cuda, c):
    """primia_gn_fwd, _fwd_mask, _bwd (with z and g_out), _bwd_mask, _relu_bwd, _relu_maxpool_fwd and (even sizes: gn.hip:932) _bwd.
    N = 130 takes one 1024-thread block per sample (gn_sample_blocks) — 130 x 4 x 4 x 512 / 8 too: 2 C = 1024 columns still
    fit the block — the other shapes the slab path; 130 x 24 x 24 x 64 gives the apply kernels a second (fp32: a third) trip
    per thread; 64 / 64 is one channel per group, 512 / 8 sixty-four.  Sample 0's group 0 has mean = 16 std."""
    dtype, dt = TORCH[c.dtype], _lib.dtype_code(TORCH[c.dtype])
    N, H, C, G = c.N, c.H, c.C, c.G
    HW, CH = H * H, nb.chunk(c.dtype)
    o = nb.gn_operands(c)
    y, res, dz, gamma, beta = o["y"], o["res"], o["dz"], o["gamma"], o["beta"]
    gamma_d, beta_d = gamma.to(cuda), beta.to(cuda)
    y_d, res_d, dz_d = (dev_of(t, dtype, cuda) for t in (y, res, dz))
    chain = nb.gn_chain(N, HW, C, c.dtype)
    n, nbytes = N * HW * C, query("primia_gn_workspace_bytes", N, C, G)
    f32 = torch.float32
    st = nb.gn_stats_ref(y, c, chain)
    one = c._replace(N=1, H=1)
    g4, b4, y4 = nb.gn_view(gamma, one), nb.gn_view(beta, one), nb.gn_view(y, c)

    def stats_of(entry, sm, si):
        smh, sih = sm.get(), si.get()
        report(entry, "stats", c, nb.check_stats(entry, st, smh, sih, axes=("sample", "group")))
        return smh, sih

    ws, z, sm, si = workspace(nbytes, cuda), Arena(n, dtype, cuda), Arena(N * G, f32, cuda), Arena(N * G, f32, cuda)
    ins = Intact(y=y_d, gamma=gamma_d, beta=beta_d)
    call("primia_gn_fwd", y_d, None, z.out, gamma_d, beta_d, sm.out, si.out, N, HW, C, G, EPS, 0, ws, nbytes, dt)
    ins.check("gn_fwd")
    stats_of("gn_fwd", sm, si)
    report("gn_fwd", "z", c, nb.check_fwd("gn_fwd", z.get(), y4, st, g4, b4, None, 0, c.dtype, axes=nb.GN_AXES))

    ws, z, mask, sm, si = (workspace(nbytes, cuda), Arena(n, dtype, cuda), Arena(n // CH, torch.uint8, cuda), Arena(N * G, f32, cuda),
                           Arena(N * G, f32, cuda))
    ins = Intact(y=y_d, res=res_d, gamma=gamma_d, beta=beta_d)
    call("primia_gn_fwd_mask", y_d, res_d, z.out, mask.out, gamma_d, beta_d, sm.out, si.out, N, HW, C, G, EPS, ws, nbytes, dt)
    ins.check("gn_fwd_mask")
    smh, sih = stats_of("gn_fwd_mask", sm, si)
    zh = z.get().float().reshape(N, HW, C)
    report("gn_fwd_mask", "z", c, nb.check_fwd("gn_fwd_mask", zh, y4, st, g4, b4, nb.gn_view(res, c), 1, c.dtype, axes=nb.GN_AXES))
    report("gn_fwd_mask", "mask", c, nb.check_mask("gn_fwd_mask", mask.get(), zh, c.dtype, axes=("sample", "pixel", "channel")))

    keep = zh > 0
    g = torch.where(keep, dz, torch.zeros(()))
    got = []
    for entry in ("gn_bwd", "gn_bwd_mask"):
        ws, dy, go, dg, db = (workspace(nbytes, cuda), Arena(n, dtype, cuda), Arena(n, dtype, cuda), Arena(N * C, f32, cuda),
                              Arena(N * C, f32, cuda))
        ins = Intact(y=y_d, z=z.out, mask=mask.out, dz=dz_d, sm=sm.out, si=si.out)
        if entry == "gn_bwd":
            call("primia_gn_bwd", y_d, z.out, dz_d, dy.out, go.out, gamma_d, sm.out, si.out, dg.out, db.out, N, HW, C, G, 1, ws, nbytes, dt)
        else:
            call("primia_gn_bwd_mask", y_d, mask.out, dz_d, dy.out, go.out, gamma_d, sm.out, si.out, dg.out, db.out, N, HW, C, G, ws,
                 nbytes, dt)
        ins.check(entry)
        report(entry, "g_out", c, nb.check_g_out(entry, go.get(), dz, keep, axes=("sample", "pixel", "channel")))
        got.append(nb.Bwd(entry, dy.get(), dg.get(), db.get(), chain))
    for out, r in zip(got, nb.check_gn_bwd_all(got, c, y, g, gamma, smh, sih)):
        report3(out.name, c, r, ("dy", "ps_dgamma", "ps_dbeta"))

    # no residual: the ReLU decision is recomputed from y
    per_c = lambda t: t.reshape(N, G).repeat_interleave(C // G, dim=1).unsqueeze(1)   # noqa: E731
    g_r = torch.where(nb.relu_keep(y, per_c(smh), per_c(sih), gamma, beta), dz, torch.zeros(()))
    ws, dy, dg, db = workspace(nbytes, cuda), Arena(n, dtype, cuda), Arena(N * C, f32, cuda), Arena(N * C, f32, cuda)
    ins = Intact(y=y_d, dz=dz_d, sm=sm.out, si=si.out, beta=beta_d)
    call("primia_gn_relu_bwd", y_d, dz_d, dy.out, gamma_d, beta_d, sm.out, si.out, dg.out, db.out, N, HW, C, G, ws, nbytes, dt)
    ins.check("gn_relu_bwd")
    report3("gn_relu_bwd", c, nb.check_gn_bwd("gn_relu_bwd", dy.get(), dg.get(), db.get(), c, y, g_r, gamma, smh, sih, chain),
            ("dy", "ps_dgamma", "ps_dbeta"))

    # the stem tail under GroupNorm
    Ho = nb.pool_out(H)
    npool = N * Ho * Ho * C
    ws, pooled, am, sm, si = (workspace(nbytes, cuda), Arena(npool, dtype, cuda), Arena(npool, torch.uint8, cuda), Arena(N * G, f32, cuda),
                              Arena(N * G, f32, cuda))
    ins = Intact(y=y_d, gamma=gamma_d, beta=beta_d)
    call("primia_gn_relu_maxpool_fwd", y_d, pooled.out, am.out, gamma_d, beta_d, sm.out, si.out, N, H, H, C, G, EPS, ws, nbytes, dt)
    ins.check("gn_relu_maxpool_fwd")
    smh, sih = stats_of("gn_relu_maxpool_fwd", sm, si)
    ref, E, _ = nb.affine_ref(y4, st, g4, b4)
    ah = am.get()
    report("gn_relu_maxpool_fwd", "pooled", c, nb.check_pool_fwd("gn_relu_maxpool_fwd", pooled.get(), ah,
                                                                 ref.clamp_min(0.0).reshape(N, H, H, C), E.reshape(N, H, H, C), c.dtype))
    if H % 2:
        return
    keep = nb.relu_keep(y, per_c(smh), per_c(sih), gamma, beta)
    g, ga = (t.reshape(N, HW, C) * keep for t in nb.pool_scatter(o["dp"], ah, N, H, C))
    dp_d = dev_of(o["dp"], dtype, cuda)
    ws, dy, dg, db = workspace(nbytes, cuda), Arena(n, dtype, cuda), Arena(N * C, f32, cuda), Arena(N * C, f32, cuda)
    ins = Intact(y=y_d, pooled=pooled.out, dp=dp_d, argmax=am.out, sm=sm.out, si=si.out)
    call("primia_gn_relu_maxpool_bwd", y_d, pooled.out, dp_d, am.out, dy.out, gamma_d, beta_d, sm.out, si.out, dg.out, db.out, N, H, H, C,
         G, ws, nbytes, dt)
    ins.check("gn_relu_maxpool_bwd")
    chain_p = nb.gn_chain(N, Ho * Ho, C, c.dtype)
    report3("gn_relu_maxpool_bwd", c, nb.check_gn_bwd("gn_relu_maxpool_bwd", dy.get(), dg.get(), db.get(), c, y, g, gamma, smh, sih,
                                                       chain_p, g_abs=ga, pooled_beta=beta), ("dy", "ps_dgamma", "ps_dbeta"))
