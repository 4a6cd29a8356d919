"""GPU: the kernels of Poisson-sampled DP-SGD (csrc/dp_sample.hip), each alone.

primia_poisson_select is an integer function of a ChaCha20 keystream: bit for bit against a selection made here from
tests.cpu_standins.chacha20_words.  primia_gather_batch copies: bit for bit.  The masked loss forms its softmax in fp64
and rounds once, so a valid dlogits element is within ONE fp32 rounding (2^-24 relative) of the float64 softmax - onehot
— plus 1e-15 absolute for the fp64 evaluation itself (a few 1e-16 on values of at most 1; the logits here keep every
probability away from 1, so softmax - 1 does not cancel).  The masked clip factors obey check_clip's bound
(tests/test_gpu_dp_pieces.py) on valid rows.  Padded rows are exactly zero everywhere.

Outputs live in arenas of sentinel words, and every word outside the output proper is compared with the sentinel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from primia_amd._lib import PrimiaError, call, query  # noqa: E402
from tests.cpu_standins import chacha20_words  # noqa: E402
from tests.test_gpu_dp_pieces import check_clip, clip_inputs  # noqa: E402

KEY = (0x0706050403020100, 0x0f0e0d0c0b0a0908, 0x1716151413121110, 0x1f1e1d1c1b1a1918)
NONCE = 0x4a00000000
K = KEY + (NONCE,)
SENT = 0x5A5A5A5A5A5A5A5A
PAD = 8
Q149 = (149 << 64) // 1000          # floor(0.149 * 2^64)
THRESHOLDS = [0, 2 ** 63, Q149, 2 ** 64 - 1]
# the kernel walks n in chunks of CHUNK records (1024 threads x one 8-record block): the sizes from 8191 on cross chunk
# boundaries, where the running base, the double-buffered wave totals and the one barrier per chunk come into play
CHUNK = 8192
SIZES = [0, 1, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 5163, 8191, 8192, 8193, 16385, 20000]


def selected_ref(block0, threshold, n):
    """Ascending indices i < n whose keystream word (word i % 8 of block block0 + i / 8) is below the threshold."""
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    words = chacha20_words(K, block0, n)
    return np.nonzero(words < np.uint64(threshold))[0].astype(np.int64)


class Arena:
    """[PAD | idx: capacity words | PAD | count: one word = two int32 | PAD | overflow: one word | PAD] of int64."""

    def __init__(self, cuda, capacity, overflow=0):
        self.cap = capacity
        self.t = torch.full((capacity + 2 + 4 * PAD,), SENT, dtype=torch.int64, device=cuda)
        self.i0, self.c0, self.o0 = PAD, 2 * PAD + capacity, 3 * PAD + capacity + 1
        self.t[self.o0] = overflow
        self.idx = self.t[self.i0:self.i0 + capacity]
        self.count = self.t[self.c0:self.c0 + 1].view(torch.int32)
        self.overflow = self.t[self.o0:self.o0 + 1]

    def check(self, sel, overflow_want):
        t = self.t.cpu()
        outside = torch.ones(t.numel(), dtype=torch.bool)
        outside[self.i0:self.i0 + self.cap] = False
        outside[self.c0] = False
        outside[self.o0] = False
        assert (t[outside] == SENT).all(), "a word outside idx / count / overflow_events was written"
        kept = min(len(sel), self.cap)
        idx = t[self.i0:self.i0 + self.cap].numpy()
        assert np.array_equal(idx[:kept], sel[:kept]), (idx[:kept], sel[:kept])
        assert (idx[kept:] == -1).all()
        assert self.count.cpu().tolist() == [len(sel), kept]
        assert int(t[self.o0]) == overflow_want


def select(arena, counter, block_offset, threshold, n):
    call("primia_poisson_select", *K, counter, block_offset, threshold, n, arena.cap, arena.idx, arena.count,
         arena.overflow)


@pytest.mark.parametrize("threshold", THRESHOLDS, ids=["t0", "half", "q149", "tmax"])
@pytest.mark.parametrize("n", SIZES)
def test_poisson_select_matches_the_keystream(cuda, n, threshold):
    """A counter start that is not zero and one from which the second block carries into state word 13, with and without
    a block offset; capacity above the selected count (padding is -1, overflow_events stays) and below it (the first
    `capacity` are kept, overflow_events moves by one).  Then two consecutive calls with primia_u64_add between them."""
    for start, offset in ((5, 0), (2 ** 32 - 1, 0), (7, 2 ** 32 + 3)):
        sel = selected_ref(start + offset, threshold, n)
        counter = torch.tensor([start], dtype=torch.int64, device=cuda)
        roomy = Arena(cuda, len(sel) + 3, overflow=11)
        select(roomy, counter, offset, threshold, n)
        roomy.check(sel, 11)
        if len(sel) == 1:           # capacity == selected: full, no padding, no overflow
            exact = Arena(cuda, 1, overflow=4)
            select(exact, counter, offset, threshold, n)
            exact.check(sel, 4)
        if len(sel) >= 2:
            tight = Arena(cuda, len(sel) // 2, overflow=11)
            select(tight, counter, offset, threshold, n)
            tight.check(sel, 12)
        assert int(counter.item()) == start                 # read, not advanced
    if threshold == 0:
        assert len(sel) == 0
    if threshold == 2 ** 64 - 1 and n:
        assert len(sel) >= n - 1                            # (a word equal to 2^64 - 1 alone is not selected)
    # two calls in a row
    blocks = query("primia_poisson_blocks", n)
    assert blocks == (n + 7) // 8
    counter = torch.tensor([1000], dtype=torch.int64, device=cuda)
    for step in range(2):
        a = Arena(cuda, n + 1)
        select(a, counter, 0, threshold, n)
        a.check(selected_ref(1000 + step * blocks, threshold, n), 0)
        if blocks:
            call("primia_u64_add", counter, blocks)
    assert int(counter.item()) == 1000 + 2 * blocks


@pytest.mark.parametrize("threshold", [2 ** 63, Q149, 2 ** 64 - 1], ids=["half", "q149", "tmax"])
@pytest.mark.parametrize("n", [20000, 3 * CHUNK, 13 * CHUNK + 5])
def test_poisson_select_cut_inside_a_later_chunk(cuda, n, threshold):
    """Three and fourteen chunks per launch (the last one partial or a few records): the capacity cut falls in the middle
    of the second chunk's selection, in the middle of the third's, exactly at the first and the second chunk's end, and
    one record into the third chunk; the kept prefix, the -1 padding and the counts are the reference's, and
    overflow_events moves by exactly one."""
    start = 2 ** 32 - 3
    sel = selected_ref(start, threshold, n)
    per_chunk = np.bincount(sel // CHUNK, minlength=-(-n // CHUNK))
    assert len(per_chunk) >= 3 and per_chunk[1] >= 2 and per_chunk[2] >= 4
    c1, c2, c3 = (int(v) for v in per_chunk[:3])
    counter = torch.tensor([start], dtype=torch.int64, device=cuda)
    for cap in (c1 + c2 // 2, c1 + c2 + c3 // 2, c1, c1 + c2, c1 + c2 + 1):
        assert cap < len(sel)
        a = Arena(cuda, cap, overflow=7)
        select(a, counter, 0, threshold, n)
        a.check(sel, 8)
    roomy = Arena(cuda, len(sel) + 5, overflow=7)
    select(roomy, counter, 0, threshold, n)
    roomy.check(sel, 7)
    # twice the same call: the same bits (no position depends on timing)
    again = Arena(cuda, len(sel) + 5, overflow=7)
    select(again, counter, 0, threshold, n)
    assert torch.equal(again.t, roomy.t)


def test_poisson_select_without_a_counter_and_refusals(cuda):
    a = Arena(cuda, 40)
    select(a, None, 9, Q149, 200)
    a.check(selected_ref(9, Q149, 200), 0)
    for bad in (dict(n=-1), dict(cap=0), dict(idx=None), dict(count=None), dict(overflow=None), dict(n=2 ** 31)):
        args = dict(n=8, cap=a.cap, idx=a.idx, count=a.count, overflow=a.overflow)
        args.update(bad)
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_poisson_select", *K, None, 0, Q149, args["n"], args["cap"], args["idx"], args["count"],
                 args["overflow"])
    a.check(selected_ref(9, Q149, 200), 0)                  # a refused call writes nothing


def test_poisson_select_replayed_graph_selects_fresh_sets(cuda):
    n, cap = 1025, 200
    blocks = query("primia_poisson_blocks", n)
    a = Arena(cuda, cap)
    counter = torch.zeros(1, dtype=torch.int64, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up outside the capture, then put the counter back
        select(a, counter, 0, Q149, n)
        call("primia_u64_add", counter, blocks)
        counter.zero_()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        select(a, counter, 0, Q149, n)
        call("primia_u64_add", counter, blocks)
    sets = []
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        sel = selected_ref(i * blocks, Q149, n)
        assert len(sel) <= cap
        a.check(sel, 0)
        sets.append(tuple(sel))
    assert len(set(sets)) == 3
    assert int(counter.item()) == 3 * blocks


# ---- primia_gather_batch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("chunks", [1, 3, 3 * 32 * 32 * 4 // 16], ids=["one_chunk", "three_chunks", "3x32x32_f32_bytes"])
@pytest.mark.parametrize("row_offset", [0, 7])
def test_gather_batch(cuda, dtype, chunks, row_offset):
    """Rows of one 16-byte chunk, an odd number of chunks and (f32) a 3 x 32 x 32 image — for bf16 the same byte count and,
    below, 3 * 32 * 32 elements; interior and trailing -1, an index at n_rows (out of range), a non-zero row offset."""
    per = 4 if dtype == torch.float32 else 8
    for row_elems in sorted({chunks * per, 3 * 32 * 32} if chunks > 3 else {chunks * per}):
        n_rows, cap = 7, 8
        g = torch.Generator().manual_seed(row_elems + row_offset)
        data = torch.randn(2 * n_rows, row_elems, generator=g).to(dtype).to(cuda)
        targets = torch.randint(0, 3, (2 * n_rows,), generator=g).to(cuda)
        idx = torch.tensor([3, -1, 0, 6, n_rows, 5, -1, -1], dtype=torch.int64, device=cuda)
        G = 64
        out = torch.full((G + cap * row_elems + G,), 7.0, dtype=dtype, device=cuda)
        out_t = torch.full((PAD + cap + PAD,), SENT, dtype=torch.int64, device=cuda)
        call("primia_gather_batch", data, row_elems, n_rows, targets, idx, row_offset, out[G:], out_t[PAD:], cap,
             0 if dtype == torch.float32 else 1)
        want = torch.zeros(cap, row_elems, dtype=dtype, device=cuda)
        want_t = torch.full((cap,), -1, dtype=torch.int64, device=cuda)
        for s, r in enumerate(idx.tolist()):
            if 0 <= r < n_rows:
                want[s] = data[row_offset + r]
                want_t[s] = targets[row_offset + r]
        iv = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(out[G:G + cap * row_elems].view(iv), want.reshape(-1).view(iv))
        assert (out[:G] == 7.0).all() and (out[G + cap * row_elems:] == 7.0).all()
        assert torch.equal(out_t[PAD:PAD + cap], want_t)
        assert (out_t[:PAD] == SENT).all() and (out_t[PAD + cap:] == SENT).all()


def test_gather_batch_refusals(cuda):
    data = torch.zeros(4, 16, dtype=torch.bfloat16, device=cuda)
    f32 = torch.zeros(4, 16, device=cuda)
    targets = torch.zeros(4, dtype=torch.int64, device=cuda)
    idx = torch.zeros(2, dtype=torch.int64, device=cuda)
    out = torch.zeros(2 * 16 + 8, dtype=torch.bfloat16, device=cuda)
    out_t = torch.zeros(2, dtype=torch.int64, device=cuda)
    call("primia_gather_batch", data, 16, 4, targets, idx, 0, out, out_t, 2, 1)
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):        # 6 bf16 elements = 12 bytes
        call("primia_gather_batch", data, 6, 4, targets, idx, 0, out, out_t, 2, 1)
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):        # 6 f32 elements = 24 bytes
        call("primia_gather_batch", f32, 6, 4, targets, idx, 0, out, out_t, 2, 0)
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):        # out 4 bytes off a 16-byte boundary
        call("primia_gather_batch", data, 16, 4, targets, idx, 0, out[2:], out_t, 2, 1)
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
        call("primia_gather_batch", data.view(-1)[2:], 16, 3, targets, idx, 0, out, out_t, 2, 1)
    for hole in range(5):
        ptrs = [data, targets, idx, out, out_t]
        ptrs[hole] = None
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_gather_batch", ptrs[0], 16, 4, ptrs[1], ptrs[2], 0, ptrs[3], ptrs[4], 2, 1)


# ---- masked loss and clip factors -----------------------------------------------------------------------------------
N, C = 257, 3           # two strides of the single block's 256 threads; two blocks of the clip kernel


def masks():
    g = torch.Generator().manual_seed(3)
    mixed = torch.rand(N, generator=g) < 0.4
    mixed[:6] = False                       # (check_clip reads its special cases from the first six rows)
    mixed[-1] = True
    return {"all_valid": torch.zeros(N, dtype=torch.bool), "all_padding": torch.ones(N, dtype=torch.bool), "mixed": mixed}


@pytest.mark.parametrize("which", ["all_valid", "all_padding", "mixed"])
def test_xent_hard_masked(cuda, which):
    pad = masks()[which]
    g = torch.Generator().manual_seed(17)
    logits = torch.randn(N, C, generator=g) * 2.0
    target = torch.randint(0, C, (N,), generator=g)
    target[pad] = -torch.randint(1, 5, (int(pad.sum()),), generator=g)      # any negative value is padding
    arena = torch.full((N * C + 64,), float("nan"), device=cuda)
    loss = torch.full((4,), float("nan"), device=cuda)
    call("primia_xent_hard_masked", logits.to(cuda), target.to(cuda), loss, arena, N, C)
    assert torch.isnan(arena[N * C:]).all() and torch.isnan(loss[1:]).all()
    got = arena[:N * C].view(N, C).cpu().double()
    valid = ~pad
    ls = torch.log_softmax(logits.double(), 1)
    ref = ls.exp()
    ref[torch.arange(N)[valid], target[valid]] -= 1.0
    err = (got[valid] - ref[valid]).abs()
    bound = 2.0 ** -24 * ref[valid].abs() + 1e-15
    if valid.any():
        print(f"{which}: max |dlogits - ref| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert (got[pad] == 0).all() and not torch.signbit(got[pad]).any()
    if valid.any():
        want = float(-ls[torch.arange(N)[valid], target[valid]].mean())
        assert abs(float(loss[0]) - want) <= 2.0 ** -24 * abs(want) + 1e-13, (float(loss[0]), want)
    else:
        assert float(loss[0]) == 0.0


def test_xent_hard_masked_poisons_a_label_past_the_classes(cuda):
    logits = torch.randn(4, C, device=cuda)
    target = torch.tensor([0, C, -1, 2], device=cuda)
    loss, dl = torch.zeros(1, device=cuda), torch.zeros(4, C, device=cuda)
    call("primia_xent_hard_masked", logits, target, loss, dl, 4, C)
    assert torch.isnan(loss).all() and torch.isnan(dl[1]).all()
    assert torch.isfinite(dl[0]).all() and (dl[2] == 0).all() and torch.isfinite(dl[3]).all()


@pytest.mark.parametrize("which", ["all_valid", "all_padding", "mixed"])
@pytest.mark.parametrize("Cn", [1.0, 0.05])
def test_dp_clip_factors_masked(cuda, which, Cn):
    pad = masks()[which]
    Cn = float(torch.tensor(Cn, dtype=torch.float32))
    sq = clip_inputs(N, Cn, torch.Generator().manual_seed(7))
    target = torch.zeros(N, dtype=torch.int64)
    target[pad] = -1
    arena = torch.full((512,), float("nan"), device=cuda)
    call("primia_dp_clip_factors_masked", sq.to(cuda), target.to(cuda), arena, N, Cn)
    assert torch.isnan(arena[N:]).all()
    got = arena[:N].cpu()
    assert (got[pad] == 0).all()
    if (~pad).any():
        check_clip(got[~pad], sq[~pad], Cn)
        # the unmasked kernel's bits on valid rows
        plain = torch.empty(N, device=cuda)
        call("primia_dp_clip_factors", sq.to(cuda), plain, N, Cn)
        assert torch.equal(got[~pad], plain.cpu()[~pad])
