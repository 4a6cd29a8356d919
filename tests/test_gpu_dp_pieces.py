"""GPU: the small kernels of the DP-SGD step (csrc/gn.hip, "DP-SGD per-sample pieces"), each one alone against a plain
float64 restatement on the CPU.  Inside ResNet18Engine.dp_loss_backward they are only judged through whole-gradient
errors of 5e-3, which a skipped tensor of a `_many` launch, a dropped row of a column sum, an fp32 norm or a clip factor
without its 1e-6 term all pass — and the first of these UNDER-estimates ||g_n||, i.e. clips a sample too little.

Bounds: where the kernel performs one fp32 operation per element (scale_rows, fc_persample_grads) the result is
bit-equal to the same operation in torch; where it sums in fp64 and rounds once (weighted_colsum) the bound is one fp32
rounding; the fp64 norms keep the 1e-10 that test_gpu_dp.py already holds primia_persample_sqnorm to.
Outputs live in ONE arena tensor per call with slack behind them (and, for several outputs, as consecutive slices), and
the whole arena is compared: a write past a tensor's end or into another sample's rows fails the comparison.

The check_* functions take the kernel's output as an array, so that they can be fed a tampered one without a GPU."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from primia_amd import _lib  # noqa: E402
from primia_amd._lib import PrimiaError, call  # noqa: E402

EPS32 = 2.0 ** -23          # one fp32 ulp of 1.0 (a single rounding to nearest is within half of it)
F32, BF16 = torch.float32, torch.bfloat16


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def same_bits(a, b):
    """Equal as bit patterns (NaN slack included; +0 and -0 differ)."""
    iv = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(iv[a.dtype]), b.view(iv[b.dtype]))


def signed(shape, g, lo=0.5, hi=1.5):
    """Random sign, magnitude in [lo, hi): no zeros, no denormals, no sample whose norm is small by accident."""
    mag = torch.rand(shape, generator=g) * (hi - lo) + lo
    return mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def dev_table(tensors, device):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64, device=device)


# ---- primia_persample_sqnorm / _many --------------------------------------------------------------------------------
def sqnorm_ref(x):
    return (x.double() ** 2).sum(1)


def check_sqnorm(got, prefill, ref):
    """got[n] = prefill[n] + sum_j x[n][j]^2 in fp64: the increment to 1e-10 per sample, exactly 0 for a zero sample."""
    got, inc = got.cpu(), got.cpu() - prefill
    zero = ref == 0
    assert torch.equal(got[zero], prefill[zero]), (got[zero], prefill[zero])
    err = (inc[~zero] - ref[~zero]).abs() / ref[~zero]
    assert (err < 1e-10).all(), (err, inc, ref)


def sqnorm_samples(N, per, g):
    """Sample 1 all zeros, sample 2 around 1e-20 (squares are sub-normal in fp32, ordinary in fp64), the others O(1)."""
    x = signed((N, per), g)
    if N > 2:
        x[1] = 0.0
        x[2] *= 1e-20
    # prefill: the kernel ACCUMULATES.  0.75 would swallow the ~1e-40 increments of the tiny sample
    prefill = torch.full((N,), 0.75, dtype=torch.float64)
    if N > 2:
        prefill[2] = 3e-38
    return x, prefill


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("per", [1, 255, 257, 1539, 64 * 256 + 3])       # 64 * 256 + 3: past the 64-block cap
def test_persample_sqnorm(cuda, N, per):
    x, prefill = sqnorm_samples(N, per, torch.Generator().manual_seed(per + N))
    sq = prefill.clone().to(cuda)
    call("primia_persample_sqnorm", x.to(cuda), N, per, sq)
    check_sqnorm(sq, prefill, sqnorm_ref(x))


ENGINE_WIDTHS = tuple((64, 128, 256, 512)[i % 4] for i in range(40))     # ps_affine: 20 norm layers x (dgamma, dbeta)


@pytest.mark.parametrize("N", [3, 130])
@pytest.mark.parametrize("widths", [ENGINE_WIDTHS, (1, 3, 257)], ids=["engine40", "odd3"])
def test_persample_sqnorm_many(cuda, N, widths):
    g = torch.Generator().manual_seed(N + len(widths))
    xs = [signed((N, w), g) for w in widths]
    arena = torch.cat([x.reshape(-1) for x in xs]).to(cuda)
    views, off = [], 0
    for w in widths:
        views.append(arena[off:off + N * w].view(N, w))
        off += N * w
    ptrs, wd = dev_table(views, cuda), torch.tensor(widths, dtype=torch.int32, device=cuda)
    prefill = torch.full((N,), 0.75, dtype=torch.float64)
    sq = prefill.clone().to(cuda)
    call("primia_persample_sqnorm_many", ptrs, wd, len(widths), N, sq)
    check_sqnorm(sq, prefill, sum(sqnorm_ref(x) for x in xs))
    # one tensor of one sample made large: that sample's sum follows, nobody else's moves
    k, m = len(widths) - 2, N // 2
    xs[k][m] = 1e3
    views[k][m] = 1e3
    sq2 = prefill.clone().to(cuda)
    call("primia_persample_sqnorm_many", ptrs, wd, len(widths), N, sq2)
    check_sqnorm(sq2, prefill, sum(sqnorm_ref(x) for x in xs))
    others = torch.arange(N) != m
    # (one fp64 atomic per tensor in any order: two runs differ by at most 2 * len(widths) roundings of 2^-53 < 1e-13)
    assert torch.allclose(sq2.cpu()[others], sq.cpu()[others], rtol=1e-13, atol=0.0)


def test_persample_sqnorm_many_of_nothing(cuda):
    call("primia_persample_sqnorm_many", None, None, 0, 4, None)


# ---- primia_dp_clip_factors -----------------------------------------------------------------------------------------
def clip_ref(sq, C):
    return torch.clamp(C / (sq.sqrt() + 1e-6), max=1.0)


def check_clip(got, sq, C):
    ref, gd = clip_ref(sq, C), got.cpu().double()
    assert (gd <= 1.0).all()
    # one fp32 rounding of the fp64 value.  (2^-126: where the value is below the fp32 range — sq = 1e300 gives
    # 1e-150 — that rounding yields 0 or a sub-normal, an ABSOLUTE error below the smallest normal number)
    assert ((gd - ref).abs() <= EPS32 * ref + 2.0 ** -126).all(), ((gd - ref).abs() / ref).max()
    # the sensitivity bound itself: no sample's clipped norm exceeds C by more than that rounding
    assert (gd * sq.sqrt() <= C * (1 + EPS32)).all(), (gd * sq.sqrt()).max()
    assert gd[0] == 1.0                      # sq = 0
    assert gd[1] < 1.0                       # sq = C^2 exactly: C / (C + 1e-6)


def clip_inputs(N, C, g):
    c2 = C * C                               # exact in fp64 (C is an fp32 number)
    sq = c2 * torch.exp(torch.rand(N, generator=g, dtype=torch.float64) * 8 - 4)
    sq[:6] = torch.tensor([0.0, c2, c2 * (1 + 1e-9), c2 * (1 - 1e-9), 1e-30, 1e300], dtype=torch.float64)
    assert (sq[6:] < c2).any() and (sq[6:] > c2).any()
    return sq


@pytest.mark.parametrize("C", [1.0, 0.05])
def test_dp_clip_factors(cuda, C):
    N = 257                                  # two blocks, the second one nearly empty
    C = float(torch.tensor(C, dtype=torch.float32))          # the value the float argument carries
    sq = clip_inputs(N, C, torch.Generator().manual_seed(7))
    arena = torch.full((512,), float("nan"), device=cuda)
    call("primia_dp_clip_factors", sq.to(cuda), arena, N, C)
    assert torch.isnan(arena[N:]).all()
    check_clip(arena[:N], sq, C)


# ---- primia_scale_rows / _many --------------------------------------------------------------------------------------
def scale_ref(x, s):
    """One fp32 multiply per element and, for bf16, one round-to-nearest-even (common.h: Chunk<T>::pack)."""
    return (x.float() * s[:, None]).to(x.dtype)


def scale_inputs(N, per, dtype, g):
    x = (signed((N, per), g) * 2.0 ** torch.randint(-3, 4, (N, per), generator=g).float()).to(dtype)
    return x, torch.rand(N, generator=g) * 0.9 + 0.1          # every product stays in the normal range


def scale_many(views, s, N, dt, count=None):
    ptrs = (ctypes.c_void_p * len(views))(*[v.data_ptr() for v in views])
    per = (ctypes.c_int64 * len(views))(*[v.numel() // N for v in views])
    call("primia_scale_rows_many", ptrs, per, len(views) if count is None else count, s, N, dt)


# chunks (of 16 bytes) per sample; at N = 300 gn_rows_grid gives 7 blocks per sample and 8 * 256 + 5 chunks need 9
@pytest.mark.parametrize("N,chunks", [(3, 1), (5, 257), (300, 8 * 256 + 5)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_scale_rows(cuda, dtype, N, chunks):
    ch = 4 if dtype == F32 else 8
    per, dt = chunks * ch, _lib.dtype_code(dtype)
    x, s = scale_inputs(N, per, dtype, torch.Generator().manual_seed(N + chunks))
    slack = torch.full((2 * ch,), 3.0, dtype=dtype)
    start = torch.cat([x.reshape(-1), slack])
    want = torch.cat([scale_ref(x, s).reshape(-1), slack])
    arena = start.clone().to(cuda)
    call("primia_scale_rows", arena, s.to(cuda), N, per, dt)
    assert same_bits(arena, want)
    # the _many launch with a single tensor: the same bits
    arena2 = start.clone().to(cuda)
    scale_many([arena2[:N * per]], s.to(cuda), N, dt)
    assert same_bits(arena2, arena)


MANY_CHUNKS = (1, 8 * 256 + 5, 257, 2, 3, 64, 255, 256, 1, 513, 7, 100, 257, 31, 1024, 5)     # 16: the launch's limit


@pytest.mark.parametrize("N", [3, 300])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_scale_rows_many(cuda, dtype, N):
    ch = 4 if dtype == F32 else 8
    dt = _lib.dtype_code(dtype)
    g = torch.Generator().manual_seed(N)
    s = torch.rand(N, generator=g) * 0.9 + 0.1
    xs = [scale_inputs(N, c * ch, dtype, g)[0] for c in MANY_CHUNKS]
    slack = torch.full((2 * ch,), 3.0, dtype=dtype)
    arena = torch.cat([x.reshape(-1) for x in xs] + [slack]).to(cuda)
    want = torch.cat([scale_ref(x, s).reshape(-1) for x in xs] + [slack])
    views, off = [], 0
    for x in xs:
        views.append(arena[off:off + x.numel()])
        off += x.numel()
    scale_many(views, s.to(cuda), N, dt)
    assert same_bits(arena, want)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_scale_rows_refuses_what_it_cannot_chunk(cuda, dtype):
    ch = 4 if dtype == F32 else 8
    N, dt = 3, _lib.dtype_code(dtype)
    start = torch.full((N * (3 * ch + 1) + 16 * ch,), 3.0, dtype=dtype)
    x, s = start.to(cuda), torch.full((N,), 0.5, device=cuda)
    with pytest.raises(PrimiaError):
        call("primia_scale_rows", x, s, N, 3 * ch + 1, dt)
    with pytest.raises(PrimiaError):           # one bad size among good ones: nothing is launched
        scale_many([x[:N * ch], x[N * ch:N * ch + N * (ch + 1)]], s, N, dt)
    with pytest.raises(PrimiaError):           # 17 tensors: one more than a launch carries
        scale_many([x[i * ch:(i + 1) * ch] for i in range(17)], s, 1, dt)
    assert same_bits(x, start)


# ---- primia_fc_persample_grads --------------------------------------------------------------------------------------
def fc_ref(x, dy):
    return torch.cat([(dy[:, :, None] * x[:, None, :]).flatten(1), dy], 1)


# (3, 7, 2): 16 elements per sample, a block spans all of them; (130, 512, 3): the engine's fc at a large batch
@pytest.mark.parametrize("N,in_f,out_f", [(5, 512, 3), (3, 7, 2), (130, 512, 3)])
def test_fc_persample_grads(cuda, N, in_f, out_f):
    g = torch.Generator().manual_seed(N + in_f)
    x, dy = signed((N, in_f), g), signed((N, out_f), g, 0.01, 1.0)
    per = out_f * in_f + out_f
    arena = torch.full((N * per + 300,), float("nan"), device=cuda)
    call("primia_fc_persample_grads", x.to(cuda), dy.to(cuda), arena, N, in_f, out_f)
    want = torch.cat([fc_ref(x, dy).reshape(-1), torch.full((300,), float("nan"))])
    assert same_bits(arena, want)


# ---- primia_weighted_colsum / _many ---------------------------------------------------------------------------------
def colsum_ref(x, w):
    return (w.double()[:, None] * x.double()).sum(0)


def check_colsum(got, x, w):
    """fp64 sum, one rounding to fp32."""
    got = got.cpu()
    assert not torch.isnan(got).any(), torch.isnan(got).nonzero().flatten()
    assert rel(got, colsum_ref(x, w)) < EPS32


@pytest.mark.parametrize("C", [1, 3, 16, 17, 512, 1536])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 130])
def test_weighted_colsum(cuda, N, C):
    g = torch.Generator().manual_seed(N * 2000 + C)
    x, w = signed((N, C), g), torch.rand(N, generator=g) * 0.9 + 0.1
    arena = torch.full((C + 40,), float("nan"), device=cuda)       # the kernel overwrites: every column, nothing else
    call("primia_weighted_colsum", x.to(cuda), w.to(cuda), arena, N, C)
    assert torch.isnan(arena[C:]).all()
    check_colsum(arena[:C], x, w)


# 42 jobs as in a DP-SGD step (the affine tensors and fc): jobs narrower than one block's 16 columns and the widest one
# in the same launch, so that most blocks of the narrow jobs return at once next to working ones
COLSUM_WIDTHS = ENGINE_WIDTHS[:7] + (3,) + ENGINE_WIDTHS[7:21] + (1536,) + ENGINE_WIDTHS[21:39] + (17,)


@pytest.mark.parametrize("N", [1, 17, 130])
def test_weighted_colsum_many(cuda, N):
    assert len(COLSUM_WIDTHS) == 42
    g = torch.Generator().manual_seed(N)
    w = torch.rand(N, generator=g) * 0.9 + 0.1
    xs = [signed((N, c), g) for c in COLSUM_WIDTHS]
    xd, wd = [x.to(cuda) for x in xs], w.to(cuda)
    total = sum(COLSUM_WIDTHS)
    arena = torch.full((total + 40,), float("nan"), device=cuda)
    outs, off = [], 0
    for c in COLSUM_WIDTHS:
        outs.append(arena[off:off + c])
        off += c
    call("primia_weighted_colsum_many", dev_table(xd, cuda), wd, dev_table(outs, cuda),
         torch.tensor(COLSUM_WIDTHS, dtype=torch.int32, device=cuda), len(xs), max(COLSUM_WIDTHS), N)
    assert torch.isnan(arena[total:]).all()
    single = torch.full_like(arena, float("nan"))
    off = 0
    for x, c in zip(xd, COLSUM_WIDTHS):
        call("primia_weighted_colsum", x, wd, single[off:off + c], N, c)
        off += c
    assert same_bits(arena, single)            # the same summation order in both kernels
    check_colsum(arena[:total], torch.cat(xs, 1), w)
    for x, o in zip(xs, outs):                 # and job by job: a small job's error must not hide in the vector
        check_colsum(o, x, w)


# ---- primia_dp_add_noise --------------------------------------------------------------------------------------------
def noise_ref(g, noise, sigma, inv_b):
    return (g.double() + noise.double() * sigma) * inv_b


@pytest.mark.parametrize("sigma", [1.3 * 0.05, 0.0])
@pytest.mark.parametrize("n", [1, 255, 4096 * 256 + 7])                  # 4096 * 256 + 7: past the 4096-block cap
def test_dp_add_noise(cuda, n, sigma):
    gen = torch.Generator().manual_seed(n)
    g, noise = signed((n,), gen), torch.randn(n, generator=gen)
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))          # the values the float arguments carry
    sigma, inv_b = f32(sigma), f32(1.0 / 130)
    slack = torch.full((40,), 3.0)
    arena = torch.cat([g, slack]).to(cuda)
    call("primia_dp_add_noise", arena, noise.to(cuda), n, sigma, inv_b)
    assert same_bits(arena[n:], slack)
    # three fp32 roundings (product, sum, product), or two where the compiler contracts the multiply-add
    assert rel(arena[:n], noise_ref(g, noise, sigma, inv_b)) < 2 * EPS32
    if sigma == 0.0:
        assert same_bits(arena[:n], g * torch.tensor(inv_b))


def test_dp_add_noise_to_nothing(cuda):
    call("primia_dp_add_noise", None, None, 0, 1.0, 1.0)
