"""GPU: every convolution kernel, element by element, against float64 (tests/conv_bounds.py: references, bounds and their
derivation; tests/test_conv_bounds_host.py: the checkers checked).  test_gpu_ops.py and test_gpu_train_step.py judge these
kernels by ||a - b|| / ||b|| over whole tensors (1e-2 / 3e-3), which one wrong pixel does not move, and the bit-identity
tests compare kernels that share their tiling; here every output element keeps its own bound.

Every call goes through the C ABI.  Every output lives inside an arena with 256 elements of a fixed bit pattern in front and
behind (the output stays 16-byte aligned), pre-filled with NaN where the call overwrites; after the call the slack and the
inputs (x, prepared weights, dy, mask) are compared bit for bit: a ragged tile that stores one row too many, or a kernel that
scribbles on an operand, fails.  Every case asserts the kernel the dispatch chooses for it (primia_conv_kernel_id /
primia_conv_wgrad_kernel_id), so a change of the dispatch rules cannot quietly turn it into a test of another kernel.
The worst err / bound of every check is printed (`-s`); DESIGN.md keeps the table measured on the MI355X."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from primia_amd import _lib  # noqa: E402
from primia_amd._lib import ConvDesc, call, query  # noqa: E402
from tests import conv_bounds as cb  # noqa: E402
from tests.conv_bounds import ConvCase, case_id, same_bits  # noqa: E402

GUARD = 256
FILL = -123.0               # exact in bf16 and fp32, not a NaN: compared bitwise
DEFAULTS = dict(lh4=1, lh2_bm=0, s2lh=1, c64_blocks=512)
TORCH = {cb.BF16: torch.bfloat16, cb.F32: torch.float32}


@contextlib.contextmanager
def options(**kw):
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            _lib.set_option(k, v)


def guarded(n, dtype, dev, prefill=float("nan")):
    """(arena, the n-element output inside it)."""
    arena = torch.full((n + 2 * GUARD,), FILL, dtype=dtype, device=dev)
    out = arena[GUARD:GUARD + n]
    assert out.data_ptr() % 16 == 0
    if isinstance(prefill, torch.Tensor):
        out.copy_(prefill.reshape(-1))
    else:
        out.fill_(prefill)
    return arena, out


def collect(arena, n):
    """The output as a CPU array, after the guard bands were found intact."""
    host = arena.cpu()
    cb.check_guards(host, GUARD, GUARD + n, FILL)
    return host[GUARD:GUARD + n]


class Intact:
    """Bitwise copies of a call's inputs, compared after it."""

    def __init__(self, **tensors):
        self.t = {k: v for k, v in tensors.items() if v is not None}
        self.copy = {k: v.clone() for k, v in self.t.items()}

    def check(self, what):
        torch.cuda.synchronize()
        for k, v in self.t.items():
            assert same_bits(v, self.copy[k]), f"{what}: input {k} changed"


def report(route, pas, c, ratio):
    print(f"conv-bound route={route} pass={pas} case={case_id(c)} worst={ratio:.3g}")
    assert ratio <= 1.0


def desc_of(c, C=None):
    return ConvDesc.make(c.N, c.H, c.H, C or c.C, c.K, c.R, c.R, c.stride, c.pad)


def flat_nhwc(t, dtype, dev):
    return cb.nhwc(t).reshape(-1).to(dtype).to(dev)


def prepared_weights(desc, w, c_real, dtype, dev, dgrad=True):
    wf = torch.empty(query("primia_conv_wfwd_elems", desc), dtype=dtype, device=dev)
    wd = torch.empty(query("primia_conv_wdgrad_elems", desc), dtype=dtype, device=dev) if dgrad else None
    call("primia_conv_weight_prepare", desc, c_real, w.to(dev), wf, wd, _lib.dtype_code(dtype))
    return wf, wd


def mask_bytes(keep, dev):
    """bit j of byte i = element 8 i + j of the [N][H][W][C] tensor (the layout primia_bn_fwd_train_mask writes)."""
    bits = cb.nhwc(keep).reshape(-1, 8).to(torch.int32)
    return (bits << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8).to(dev)


def run_fwd_dgrad(dev, c, fwd_id, dgrad_id, passes):
    """The passes named in `passes` ("fwd", "dgrad", "acc": accumulate = 1, "masked": primia_conv2d_dgrad_masked_acc) of
    case c under the options in force, on the routes fwd_id / dgrad_id."""
    dtype, dt = TORCH[c.dtype], _lib.dtype_code(TORCH[c.dtype])
    x, w, dy, base, keep = cb.operands(c)
    desc = desc_of(c)
    Ho = cb.out_size(c)
    wf, wd = prepared_weights(desc, w, c.C, dtype, dev)
    if "fwd" in passes:
        assert query("primia_conv_kernel_id", desc, 0, dt) == fwd_id
        xd = flat_nhwc(x, dtype, dev)
        n = c.N * Ho * Ho * c.K
        arena, y = guarded(n, dtype, dev)
        ins = Intact(x=xd, w_fwd=wf)
        call("primia_conv2d_fwd", desc, xd, wf, y, dt)
        ins.check("fwd")
        report(fwd_id, "fwd", c, cb.check_fwd(collect(arena, n), c))
    if not set(passes) & {"dgrad", "acc", "masked"}:
        return
    assert query("primia_conv_kernel_id", desc, 1, dt) == dgrad_id
    dyd = flat_nhwc(dy, dtype, dev)
    n = c.N * c.H * c.H * c.C
    if "dgrad" in passes:
        arena, dx = guarded(n, dtype, dev)
        ins = Intact(dy=dyd, w_dgrad=wd)
        call("primia_conv2d_dgrad", desc, dyd, wd, dx, 0, dt)
        ins.check("dgrad")
        report(dgrad_id, "dgrad", c, cb.check_dgrad(collect(arena, n), c))
    if "acc" in passes:
        arena, dx = guarded(n, dtype, dev, prefill=flat_nhwc(base, dtype, dev))
        ins = Intact(dy=dyd, w_dgrad=wd)
        call("primia_conv2d_dgrad", desc, dyd, wd, dx, 1, dt)
        ins.check("dgrad +=")
        report(dgrad_id, "dgrad+=", c, cb.check_dgrad(collect(arena, n), c, base=base))
    if "masked" in passes:
        assert query("primia_conv_dgrad_masked_acc_ok", desc, dt) == 1
        mask = mask_bytes(keep, dev)
        arena, dx = guarded(n, dtype, dev, prefill=flat_nhwc(base, dtype, dev))
        ins = Intact(dy=dyd, w_dgrad=wd, mask=mask)
        call("primia_conv2d_dgrad_masked_acc", desc, dyd, wd, dx, mask, dt)
        ins.check("dgrad += masked")
        report(dgrad_id, "dgrad+=masked", c, cb.check_dgrad(collect(arena, n), c, base=base, keep=keep))


ALL = ("fwd", "dgrad", "acc", "masked")
BWD = ("dgrad", "acc", "masked")

# The linear-halo kernels serve a pass where its OUTPUT channels are a multiple of 128: 7x9x192-256 is theirs in the forward
# pass only (its data gradient, 192 channels wide, is the implicit GEMM's), 7x9x256-192 in the data gradient only.
LH_PASSES = [
    (cb.LH_CASES[0], ALL),
    (cb.LH_CASES[1], ("fwd",)),
    (cb.LH_CASES[2], BWD),
    (cb.LH_CASES[3], ALL),
    (cb.LH_CASES[4], ALL),
]


@pytest.mark.parametrize("c,passes", LH_PASSES, ids=lambda v: case_id(v) if isinstance(v, ConvCase) else None)
def test_loader_wave_kernel(cuda, c, passes):
    """conv3x3_lh4_kernel (id 6): the default for the shapes that take 196-pixel tiles."""
    with options():
        run_fwd_dgrad(cuda, c, 6, 6, passes)


LH2_PASSES = [(c, p, {"lh4": 0}) for c, p in LH_PASSES] + [
    (cb.LH_CASES[1], ("fwd",), {"lh2_bm": 392}),              # M = 567: two 392-pixel tiles, the second ragged
    (cb.LH_CASES[2], BWD, {"lh2_bm": 392}),
    # persistent: N = 257 at H = 7 is the smallest batch with more 196-pixel tiles than the 256 blocks of the grid
    # (conv3x3_lh2_dispatch: grid = min(tiles, CUs)) — 65 pixel tiles x 4 channel tiles = 260 tiles, blocks lb with
    # floor(260 (lb + 1) / 256) - floor(260 lb / 256) = 2 (four of them) walk two tiles, the other 252 one.  N = 256 has
    # 64 x 4 = 256 tiles: one each.  The 512 output channels are y's in the forward pass (C = 64, K = 512) and dx's in the
    # data gradient (C = 512, K = 64); the other pass of each shape has 64 output channels and is not this kernel's.
    (cb.LH2_PERSISTENT_FWD, ("fwd",), {"lh4": 0, "lh2_bm": 196}),
    (cb.LH2_PERSISTENT_DGRAD, BWD, {"lh4": 0, "lh2_bm": 196}),
]


@pytest.mark.parametrize("c,passes,opts", LH2_PASSES,
                         ids=lambda v: case_id(v) if isinstance(v, ConvCase) else
                         "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_linear_halo_kernel(cuda, c, passes, opts):
    """conv3x3_lh2_kernel (id 4): 196-pixel tiles with lh4 = 0, 392-pixel tiles with lh2_bm = 392, and a grid on which
    blocks walk unequal numbers of tiles."""
    with options(**opts):
        run_fwd_dgrad(cuda, c, 4, 4, passes)


@pytest.mark.parametrize("c,blocks", [(c, 512) for c in cb.C64_CASES] + [(cb.C64_CASES[0], 2)],
                         ids=lambda v: case_id(v) if isinstance(v, ConvCase) else f"blocks{v}")
def test_layer1_kernel(cuda, c, blocks):
    """conv3x3_c64_kernel (id 2); c64_blocks = 2: 12 patches on two blocks, each walks six."""
    with options(c64_blocks=blocks):
        run_fwd_dgrad(cuda, c, 2, 2, ALL)


@pytest.mark.parametrize("c", cb.S2_CASES[:2], ids=case_id)
def test_parity_plane_kernel_default_route(cuda, c):
    """conv_s2lh_kernel (id 5) as the training step uses it: the data gradient of the 64-channel transition block."""
    with options():
        run_fwd_dgrad(cuda, c, None, 5, ("dgrad",))


@pytest.mark.parametrize("c", [cb.S2_CASES[0]] + cb.S2_CASES[2:], ids=case_id)
def test_parity_plane_kernel_every_pass(cuda, c):
    """... and with s2lh = 7: forward of the 3x3 / 2 convolution and of the 1x1 / 2 downsample, data gradient at 64-, 128- and
    256-channel dx."""
    with options(s2lh=7):
        run_fwd_dgrad(cuda, c, 5, 5, ("fwd", "dgrad"))
        run_fwd_dgrad(cuda, cb.ds_of(c), 5, None, ("fwd",))


@pytest.mark.parametrize("c", cb.IGEMM_CASES, ids=case_id)
def test_implicit_gemm(cuda, c):
    """conv_igemm_kernel (id 1), bf16 and fp32.  (2x16x64-128 k3 s2 in bf16: its plain data gradient is conv_s2lh_kernel's
    by default and is covered above; s2lh = 0 keeps it here.)"""
    with options(s2lh=0):
        run_fwd_dgrad(cuda, c, 1, 1, ("fwd", "dgrad", "acc"))


# ---- weight gradients ------------------------------------------------------------------------------------------------
def run_wgrad(dev, c, want_id, form):
    """form "ws": primia_conv2d_wgrad_ws into an accumulator holding 7.0 (it overwrites), "acc": primia_conv2d_wgrad into a
    zeroed one; then primia_conv_wgrad_finalize.  Accumulator, workspace and dw each sit in a guarded arena."""
    dtype, dt = TORCH[c.dtype], _lib.dtype_code(TORCH[c.dtype])
    x, w, dy, _, _ = cb.operands(c)
    desc = desc_of(c)
    assert query("primia_conv_wgrad_kernel_id", desc, dt) == want_id
    xd, dyd = flat_nhwc(x, dtype, dev), flat_nhwc(dy, dtype, dev)
    na = query("primia_conv_wfwd_elems", desc)
    ins = Intact(x=xd, dy=dyd)
    if form == "ws":
        need = query("primia_conv_wgrad_ws_bytes", desc, dt)
        assert need > 0 and need % 4 == 0
        ws_arena, ws = guarded(need // 4, torch.float32, dev)
        acc_arena, acc = guarded(na, torch.float32, dev, prefill=7.0)
        call("primia_conv2d_wgrad_ws", desc, xd, dyd, acc, ws, need, dt)
        collect(ws_arena, need // 4)
    else:
        acc_arena, acc = guarded(na, torch.float32, dev, prefill=0.0)
        call("primia_conv2d_wgrad", desc, xd, dyd, acc, dt)
    ins.check("wgrad")
    collect(acc_arena, na)
    nw = c.K * c.C * c.R * c.R
    dw_arena, dw = guarded(nw, torch.float32, dev)
    ins = Intact(acc=acc)
    call("primia_conv_wgrad_finalize", desc, c.C, acc, dw)
    ins.check("finalize")
    report(want_id, "wgrad" if form == "ws" else "wgrad+=", c, cb.check_wgrad(collect(dw_arena, nw), c))


@pytest.mark.parametrize("c,want_id", [(c, 18) for c in cb.WGRAD_PATCH_CASES] + [(c, 17) for c in cb.WGRAD_TAP_CASES]
                         + [(cb.WGRAD_F32_CASE, 14)], ids=lambda v: case_id(v) if isinstance(v, ConvCase) else f"id{v}")
def test_weight_gradient(cuda, c, want_id):
    """conv_wgrad_patch33lw_kernel (18), conv_wgrad_tap_kernel (17), conv_wgrad_kernel (14, fp32) and their ordered reduce."""
    with options():
        run_wgrad(cuda, c, want_id, "ws")


@pytest.mark.parametrize("c,want_id", [(cb.WGRAD_PATCH_CASES[3], 18), (cb.WGRAD_TAP_CASES[0], 17), (cb.WGRAD_TAP_CASES[1], 17),
                                       (cb.WGRAD_F32_CASE, 14)],
                         ids=lambda v: case_id(v) if isinstance(v, ConvCase) else f"id{v}")
def test_weight_gradient_accumulating_form(cuda, c, want_id):
    """primia_conv2d_wgrad (atomic adds into a zeroed accumulator), once per id.  conv_wgrad_tap_kernel needs a workspace:
    without one the shapes it is named for (17) run on the generic kernels — conv_wgrad_kernel for 2x16x64-128,
    conv_wgrad_dma_kernel for the wide 4x14x256-512 (conv2d_wgrad_impl) — the id query does not know the form of the call."""
    with options():
        run_wgrad(cuda, c, want_id, "acc")


# ---- the stem ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cb.STEM_CASES, ids=case_id)
def test_stem(cuda, c):
    """primia_stem_conv_fwd on the padded input [N][S + 6][S + 8][4], primia_stem_conv_wgrad_ws and primia_stem_conv_wgrad
    (id 15).  The fourth channel and the padding are zeros: n counts the 3 * 7 * 7 real terms (adding an exact zero does not
    round)."""
    dtype = torch.bfloat16
    dt = _lib.dtype_code(dtype)
    N, S = c.N, c.H
    x, w, dy, _, _ = cb.operands(c)
    desc = desc_of(c, C=4)
    assert query("primia_conv_wgrad_kernel_id", desc, dt) == 15
    wf, _ = prepared_weights(desc, w, 3, dtype, cuda, dgrad=False)
    Hp, Wp = S + 6, S + 8
    xp = torch.zeros(N, Hp, Wp, 4)
    xp[:, 3:3 + S, 3:3 + S, :3] = cb.nhwc(x)
    xp = xp.reshape(-1).to(dtype).to(cuda)
    dyd = flat_nhwc(dy, dtype, cuda)
    with options():
        n = N * (S // 2) ** 2 * 64
        arena, y = guarded(n, dtype, cuda)
        ins = Intact(x=xp, w_fwd=wf)
        call("primia_stem_conv_fwd", xp, wf, y, N, S, S, dt)
        ins.check("stem fwd")
        report("stem", "fwd", c, cb.check_fwd(collect(arena, n), c))

        na = query("primia_conv_wfwd_elems", desc)
        for form in ("ws", "acc"):
            ins = Intact(x=xp, dy=dyd)
            if form == "ws":
                need = query("primia_stem_conv_wgrad_ws_bytes", N, S, S)
                assert need >= 0 and need % 4 == 0
                ws_arena, ws = guarded(max(need // 4, 4), torch.float32, cuda)
                # (need = 0: this shape takes the accumulate path and wants a zeroed accumulator)
                acc_arena, acc = guarded(na, torch.float32, cuda, prefill=7.0 if need else 0.0)
                call("primia_stem_conv_wgrad_ws", xp, dyd, acc, ws, need, N, S, S, dt)
                collect(ws_arena, max(need // 4, 4))
            else:
                acc_arena, acc = guarded(na, torch.float32, cuda, prefill=0.0)
                call("primia_stem_conv_wgrad", xp, dyd, acc, N, S, S, dt)
            ins.check("stem wgrad")
            collect(acc_arena, na)
            nw = 64 * 3 * 49
            dw_arena, dw = guarded(nw, torch.float32, cuda)
            call("primia_conv_wgrad_finalize", desc, 3, acc, dw)
            report(15, "wgrad" if form == "ws" else "wgrad+=", c, cb.check_wgrad(collect(dw_arena, nw), c))
