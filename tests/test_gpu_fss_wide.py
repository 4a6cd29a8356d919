"""GPU: the DIF kernels at a run-time width (primia_*_n, csrc/fss.hip) against tests/fss_wide_ref.py, bit for bit, on N = 300
comparisons -- two blocks of 256 with a ragged tail -- that begin with the crafted (alpha, d) pairs of
tests/test_fss_wide_host.py.  Every buffer a kernel writes sits between guard elements.  At 32 bits the new entry points
return what the old ones return."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import secure_oracle as S  # noqa: E402
from primia_amd._lib import PrimiaError, call  # noqa: E402
from primia_amd.secure import dif_key_fields  # noqa: E402
from tests import fss_wide_ref as W  # noqa: E402
from tests.fss_wide_ref import as_i64, crafted_pairs, seeds, shares_of  # noqa: E402

U64, I64 = np.uint64, np.int64
N = 300
PAD = 64
FILL = {torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}


class Guarded:
    """A device buffer of `shape` between two runs of PAD guard elements."""

    def __init__(self, shape, dtype, cuda):
        self.n = int(np.prod(shape))
        self.fill = FILL[dtype]
        self.buf = torch.full((self.n + 2 * PAD,), self.fill, dtype=dtype).to(cuda)
        self.view = self.buf[PAD:PAD + self.n].view(tuple(shape))

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:PAD] == self.fill).all()) and bool((b[PAD + self.n:] == self.fill).all())

    def host(self):
        return self.view.cpu().numpy()


def dev(a, cuda):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(I64) if a.dtype == U64 else a).to(cuda)


@functools.lru_cache(maxsize=None)
def case(n):
    """Inputs and the restatement's outputs at width n, computed once: alpha / d begin with the crafted pairs."""
    rng = np.random.default_rng(1000 + n)
    pairs = crafted_pairs(n)
    ds = [q for _, q in pairs]
    while len(pairs) < N:
        pairs.append((int(rng.integers(0, 2 ** 64, dtype=U64)) % 2 ** n, ds[len(pairs) % len(ds)]))
    alpha = np.array([a for a, _ in pairs], dtype=U64)
    d = as_i64([q for _, q in pairs])
    raw_alpha = alpha | (rng.integers(0, 2 ** 64, size=N, dtype=U64) & ~W.width_mask(n))      # garbage above the width
    r = rng.integers(0, 2 ** 64, size=N, dtype=U64)
    s0 = seeds(rng, N)
    raw_s0 = s0 | (rng.integers(0, 2, size=s0.shape, dtype=U64) << U64(63)) * np.array([1, 0], U64).reshape(1, 2, 1)
    a_sh = W.split_alpha(alpha, r, n)
    keys = W.dif_keygen(alpha, s0, n)
    v = rng.integers(-2 ** 63, 2 ** 63, size=N, dtype=I64)      # x2 = v, x1 = v + d: the difference is d
    x1, x2 = shares_of(rng, S.radd(v, d)), shares_of(rng, v)
    rm = [S.fss_mask(x1[j], x2[j], a_sh[j]) for j in range(2)]
    masked = W.fss_open(rm[0], rm[1], n)
    out = [W.dif_eval(b, masked, keys[b], n) for b in range(2)]
    return dict(pairs=pairs, alpha=alpha, raw_alpha=raw_alpha, d=d, r=r, s0=s0, raw_s0=raw_s0, a_sh=a_sh, keys=keys, x1=x1,
                x2=x2, rm=rm, masked=masked, out=out)


def gpu_keygen(cuda, alpha, s0, n, count=N):
    """primia_dif_keygen_n into guarded buffers -> the four Guarded fields."""
    fields = [Guarded(shape, dt, cuda) for shape, dt in dif_key_fields(count, n)]
    call("primia_dif_keygen_n", dev(alpha, cuda), dev(s0, cuda), *[f.view for f in fields], count, n)
    assert all(f.intact() for f in fields)
    return fields


# ---- 1. keygen ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 64])
def test_keygen_n_equals_the_restatement(cuda, n):
    c = case(n)
    bits, cw_sigma, cw_s, leaf = gpu_keygen(cuda, c["alpha"], c["s0"], n)
    k = c["keys"][0]
    assert np.array_equal(bits.host(), W.packed_bits(k["bits"]))
    assert np.array_equal(cw_sigma.host().view(U64), k["cw_sigma"]) and np.array_equal(cw_s.host().view(U64), k["cw_s"])
    assert leaf.host().shape == (n + 1, N) and np.array_equal(leaf.host(), k["cw_leaf"])
    # bits of alpha above the width change nothing
    again = gpu_keygen(cuda, c["raw_alpha"], c["s0"], n)
    assert all(torch.equal(a.view, b.view) for a, b in zip(again, (bits, cw_sigma, cw_s, leaf)))


def test_keygen_n_at_32_equals_the_32_bit_entry_point(cuda):
    c = case(32)
    new = gpu_keygen(cuda, c["alpha"], c["s0"], 32)
    old = [Guarded(shape, dt, cuda) for shape, dt in dif_key_fields(N, 32)]
    call("primia_dif_keygen", dev(c["alpha"], cuda), dev(c["s0"], cuda), *[f.view for f in old], N)
    assert all(torch.equal(a.view, b.view) for a, b in zip(new, old))
    assert np.array_equal(new[3].host(), c["keys"][0]["cw_leaf"])


# ---- 2. alpha split and open ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 40, 64])
def test_alpha_split_n_and_open_n(cuda, n):
    """The split reduces alpha and r mod 2^n in place, clears bit 63 of word 0 of both seeds and leaves word 1 alone; the open
    is the sum mod 2^n.  At 32 both equal the 32-bit calls."""
    c = case(n)
    alpha, s0, r, a0 = (Guarded(sh, torch.int64, cuda) for sh in ((N,), (2, 2, N), (N,), (N,)))
    for g, src in ((alpha, c["raw_alpha"]), (s0, c["raw_s0"]), (r, c["r"])):
        g.view.copy_(dev(src, cuda))
    call("primia_fss_alpha_split_n", alpha.view, s0.view, r.view, a0.view, N, n)
    assert all(g.intact() for g in (alpha, s0, r, a0))
    assert np.array_equal(alpha.host().view(U64), c["alpha"]) and np.array_equal(s0.host().view(U64), c["s0"])
    assert np.array_equal(a0.host().view(U64), c["a_sh"][0]) and np.array_equal(r.host().view(U64), c["a_sh"][1])
    x = Guarded((N,), torch.int64, cuda)
    call("primia_fss_open_n", dev(c["rm"][0], cuda), dev(c["rm"][1], cuda), x.view, N, n)
    assert x.intact() and np.array_equal(x.host().view(U64), c["masked"])
    if n == 32:
        o = [dev(src, cuda) for src in (c["raw_alpha"], c["raw_s0"], c["r"])] + [torch.empty(N, dtype=torch.int64, device=cuda)]
        call("primia_fss_alpha_split", *o, N)
        assert all(torch.equal(a, b.view) for a, b in zip(o, (alpha, s0, r, a0)))
        x32 = torch.empty(N, dtype=torch.int32, device=cuda)
        call("primia_fss_open", dev(c["rm"][0], cuda), dev(c["rm"][1], cuda), x32, N)
        assert np.array_equal(x32.cpu().numpy().view(np.uint32).astype(U64), c["masked"])


# ---- 3. eval --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 40, 64])
def test_eval_n_equals_the_restatement_and_the_definition(cuda, n):
    c = case(n)
    key = [dev(W.packed_bits(c["keys"][0]["bits"]), cuda)] + [dev(c["keys"][0][f], cuda) for f in ("cw_sigma", "cw_s", "cw_leaf")]
    got = []
    for b in range(2):
        out = Guarded((N,), torch.int64, cuda)
        call("primia_dif_eval_n", b, dev(c["masked"], cuda), dev(c["keys"][b]["s0"], cuda), *key, out.view, N, n)
        assert out.intact() and np.array_equal(out.host(), c["out"][b]), b
        got.append(out.host())
    bit = S.radd(got[0], got[1])
    assert np.array_equal(bit, np.array([W.defined_bit(a, q, n) for a, q in c["pairs"]], I64))
    calm = [i for i, (a, q) in enumerate(c["pairs"]) if not W.wraps(a, q, n)]
    assert len(calm) > N // 2 and all(bit[i] == int(c["pairs"][i][1] <= 0) for i in calm)
    if n == 32:
        old = torch.empty(N, dtype=torch.int64, device=cuda)
        call("primia_dif_eval", 1, dev(c["masked"].astype(np.uint32).view(np.int32), cuda), dev(c["keys"][1]["s0"], cuda), *key, old, N)
        assert np.array_equal(old.cpu().numpy(), got[1])


# ---- 4. the fused local form ----------------------------------------------------------------------------------------------
def chain(cuda, x1, x2, a_sh, s0, fields, count, n):
    """mask -> open -> eval with the step-by-step entry points: both parties' shares."""
    r = [torch.empty(count, dtype=torch.int64, device=cuda) for _ in range(2)]
    for j in range(2):
        call("primia_fss_mask", x1[j], x2[j], a_sh[j], r[j], count)
    x = torch.empty(count, dtype=torch.int64, device=cuda)
    call("primia_fss_open_n", r[0], r[1], x, count, n)
    out = [torch.empty(count, dtype=torch.int64, device=cuda) for _ in range(2)]
    for j in range(2):
        call("primia_dif_eval_n", j, x, s0[j], *fields, out[j], count, n)
    return out


@pytest.mark.parametrize("n", [40, 64])
def test_eval_local_n_equals_the_chain(cuda, n):
    """x1 = NULL (ReLU), two plain operands, and column ranges of [37][9] matrices from column 4, 3 wide (the pool tree)."""
    c = case(n)
    fields = [f.view for f in gpu_keygen(cuda, c["alpha"], c["s0"], n)]
    a_sh = [dev(c["a_sh"][j], cuda) for j in range(2)]
    s0 = [dev(c["s0"][j], cuda) for j in range(2)]
    x1 = [dev(c["x1"][j], cuda) for j in range(2)]
    x2 = [dev(c["x2"][j], cuda) for j in range(2)]
    zero = [torch.zeros(N, dtype=torch.int64).to(cuda) for _ in range(2)]

    def local(a, wa, sa, b, wb, sb, length, alpha, seed, flds, count):
        out = [Guarded((count,), torch.int64, cuda) for _ in range(2)]
        call("primia_dif_eval_local_n", None if a is None else a[0], None if a is None else a[1], wa, sa, b[0], b[1], wb, sb,
             length, alpha[0], alpha[1], seed[0], seed[1], *flds, out[0].view, out[1].view, count, n)
        assert out[0].intact() and out[1].intact()
        return [o.view for o in out]

    relu = local(None, 1, 0, x2, 1, 0, 1, a_sh, s0, fields, N)
    want = chain(cuda, zero, x2, a_sh, s0, fields, N, n)
    assert all(torch.equal(relu[j], want[j]) for j in range(2))
    plain = local(x1, 1, 0, x2, 1, 0, 1, a_sh, s0, fields, N)
    want = chain(cuda, x1, x2, a_sh, s0, fields, N, n)
    assert all(torch.equal(plain[j], want[j]) for j in range(2))
    assert np.array_equal(plain[0].cpu().numpy(), c["out"][0]) and np.array_equal(plain[1].cpu().numpy(), c["out"][1])
    # column ranges: 37 x 3 comparisons, keys of their own (the key arrays' stride is the comparison count)
    rows, w, start, length = 37, 9, 4, 3
    m = rows * length
    rng = np.random.default_rng(n)
    left = [dev(rng.integers(-2 ** 63, 2 ** 63, size=(rows, w), dtype=I64), cuda) for _ in range(2)]
    right = [dev(rng.integers(-2 ** 63, 2 ** 63, size=(rows, w), dtype=I64), cuda) for _ in range(2)]
    alpha_m = rng.integers(0, 2 ** 64, size=m, dtype=U64) & W.width_mask(n)
    sh_m = [dev(v, cuda) for v in W.split_alpha(alpha_m, rng.integers(0, 2 ** 64, size=m, dtype=U64), n)]
    s0_m = seeds(rng, m)
    fields_m = [f.view for f in gpu_keygen(cuda, alpha_m, s0_m, n, m)]
    seed_m = [dev(s0_m[j], cuda) for j in range(2)]
    cols = local(left, w, start, right, w, start + 2, length, sh_m, seed_m, fields_m, m)
    cut = lambda t, s: [t[j][:, s:s + length].contiguous().view(-1) for j in range(2)]
    want = chain(cuda, cut(left, start), cut(right, start + 2), sh_m, seed_m, fields_m, m, n)
    assert all(torch.equal(cols[j], want[j]) for j in range(2))


# ---- 5. refused widths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [31, 65])
def test_a_width_outside_32_to_64_is_refused(cuda, bits):
    z = lambda *s: torch.zeros(*s, dtype=torch.int64, device=cuda)
    keys = [torch.zeros(shape, dtype=dt, device=cuda) for shape, dt in dif_key_fields(4, 64)]
    calls = {
        "primia_fss_alpha_split_n": (z(4), z(2, 2, 4), z(4), z(4), 4),
        "primia_fss_open_n": (z(4), z(4), z(4), 4),
        "primia_dif_keygen_n": (z(4), z(2, 2, 4), *keys, 4),
        "primia_dif_eval_n": (0, z(4), z(2, 4), *keys, z(4), 4),
        "primia_dif_eval_local_n": (None, None, 1, 0, z(4), z(4), 1, 0, 1, z(4), z(4), z(2, 4), z(2, 4), *keys, z(4), z(4), 4),
    }
    for name, args in calls.items():
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call(name, *args, bits)
        call(name, *args, 64)      # the same arguments at a valid width are accepted
