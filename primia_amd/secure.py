"""Encrypted inference on GPU: fixed-precision additive secret sharing over Z_2^64 between two
parties (model_owner = party 0, data_owner = party 1) with a dealer (crypto provider) handing out
Beaver triples and FSS keys — the arithmetic of PySyft's FPT > AST tensor chain as PriMIA's
inference.py drives it (inference.py:279-321, protocol "fss").

Each method below is the host-side orchestration of one reference operation; the arithmetic runs
in the party-local HIP kernels of libprimia_hip.so (the functions PySyft registers with
@allow_command).  A shared tensor is a pair [share_0, share_1] of int64 device tensors.  An
"open" sums the two parties' buffers: with both parties on one GPU that is one ring-add kernel,
with one party per GPU it is a 2-rank RCCL all-reduce (`DistOpener`).

Randomness is never drawn implicitly: every triple, FSS key and re-sharing mask comes from a
`Dealer`, so a run is a bit-exact function of the dealer's stream (and can be replayed by the CPU
oracle in the tests).

Reference map (paths under syft/frameworks/torch/):
  encode / share / open      tensors/interpreters/precision.py:117-144, additive_shared.py:287-365
  beaver mul / matmul        mpc/spdz.py:21-197, mpc/beaver.py:7-63
  truncation                 precision.py:146-160, additive_shared.py:672-678
  fss comparison             mpc/fss.py:97-281, mpc/primitives.py:237-253
  relu                       additive_shared.py:922-925
  conv2d / pools / bn / lin  nn/functional.py:10-14, 44-75, 204-308, 460-525
  public add / sub / rsub    additive_shared.py:440-527 (constants are RE-SHARED with fresh randomness)
"""
import ctypes
import dataclasses
import os

import torch

from . import _lib
from ._lib import call

I64 = torch.int64

# The width of the FSS comparison: a comparison of d = x1 - x2 answers [(d + alpha) mod 2^n <= alpha], which is
# [d <= 0] while |d| < 2^(n-1) and alpha + d does not wrap -- an error of probability |d| / 2^n over the dealer's draw.  32 is the
# reference's width (mpc/fss.py:27) and the default; key bytes and the DIF kernels' time grow linearly with it.
FSS_BITS = 32
FSS_BITS_MAX = 64


def check_fss_bits(bits):
    bits = int(bits)
    if not FSS_BITS <= bits <= FSS_BITS_MAX:
        raise ValueError(f"fss_bits must be in [{FSS_BITS}, {FSS_BITS_MAX}], got {bits}")
    return bits


def fss_call(name, bits, *args):
    """A DIF entry point of the library at width `bits`: the reference's 32-bit one (primia_<name>), or its width-general
    form (primia_<name>_n, which takes the width last).  The one place where the width selects anything."""
    if bits == FSS_BITS:
        call("primia_" + name, *args)
    else:
        call("primia_" + name + "_n", *args, bits)


def masked_dtype(bits):
    """What holds an opened masked input: uint32 words at the reference's width, uint64 words above it."""
    return torch.int32 if bits == FSS_BITS else I64


def _empty_like(t):
    return torch.empty_like(t)


def _pair(shape, device):
    """Two empty int64 tensors: the outputs of a launch that writes both parties' shares."""
    return [torch.empty(tuple(shape), dtype=I64, device=device) for _ in range(2)]


def _six(t):
    """A triple's shares as the two-party kernels take them: a, b, c of party 0, then of party 1."""
    return (*t[0], *t[1])


def _ptr_table(t):
    """The host pointer table of a triple's six shares."""
    return (ctypes.c_void_p * 6)(*[q.data_ptr() for q in _six(t)])


def _transposed(t, rows, cols):
    """One share [rows, cols] -> [cols, rows] (weight.reshape(O, -1).t() of a conv / linear weight)."""
    o = torch.empty(cols, rows, dtype=I64, device=t.device)
    call("primia_col2out_syft", t.contiguous(), None, o, 1, rows, cols)
    return o


class Dealer:
    """The crypto provider: generates correlated randomness on the GPU.

    build_triple (mpc/beaver.py:7-63): a, b uniform int64, c = a∘b, each split into two shares.
    build_fss_keys (mpc/primitives.py:237-253): DIF keys + alpha additively split mod 2^32 -- mod 2^fss_bits, with fss_bits
    levels per key, for a dealer of another comparison width (the contexts it serves read the width from it).

    Randomness is a ChaCha20 keystream (`primia_chacha20_fill`) under a 256-bit key taken from the operating
    system's entropy pool (`os.urandom`) when the dealer is constructed — never shared, never derived from anything
    public: the parties' privacy rests on not being able to predict these masks (the request schedule itself IS
    public).  `seed` is for tests, benchmarks and oracle replay only: it derives the key from the seed
    (SHA-256), making the whole stream reproducible — and therefore worthless as a secret."""

    def __init__(self, device, seed=None, fss_bits=FSS_BITS):
        import hashlib
        import os

        self.device = torch.device(device)
        self.fss_bits = check_fss_bits(fss_bits)
        self.seeded = seed is not None
        raw = os.urandom(40) if seed is None else hashlib.sha256(b"primia-dealer-debug-seed:%d" % int(seed)).digest() + bytes(8)
        self._key = [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(4)]
        self._nonce = int.from_bytes(raw[32:40], "little")
        self._block = 0
        self.log = None  # set to a list to record every primitive handed out (tests replay it)
        self.tape = None  # set to a list to keep every primitive ON THE DEVICE (offline phase, see PreloadedDealer)
        self.requests = None  # set to a list to record (method, args) of every request (GraphedSecureInference)

    def rand64(self, *shape):
        out = torch.empty(shape, dtype=I64, device=self.device)
        n = out.numel()
        call("primia_chacha20_fill", *self._key, self._nonce, self._block, out, n)
        self._block += (n + 7) // 8
        return out

    def _split(self, v):
        r = self.rand64(*v.shape)
        s1 = _empty_like(v)
        call("primia_ring_sub", v, r, s1, v.numel(), v.numel())
        return [r, s1]

    def triple(self, op, xshape, yshape):
        if self.requests is not None:
            self.requests.append(("triple", (op, tuple(xshape), tuple(yshape)), {}))
        # the input shares are drawn directly (a = a0 + a1 with both shares uniform IS the sharing of a uniform a that
        # build_triple produces by drawing a and one share, mpc/beaver.py:7-63): 9 launches per triple instead of 21
        sa = [self.rand64(*xshape), self.rand64(*xshape)]
        sb = [self.rand64(*yshape), self.rand64(*yshape)]
        c0 = self.rand64(*_triple_c_shape(op, xshape, yshape))
        c1 = _empty_like(c0)
        self.triple_c1(op, xshape, yshape, sa[0], sa[1], sb[0], sb[1], c0, c1)
        sc = [c0, c1]
        t = [(sa[j], sb[j], sc[j]) for j in range(2)]
        if self.log is not None:
            self.log.append(("triple", op, [tuple(x.cpu().numpy() for x in t[j]) for j in range(2)]))
        if self.tape is not None:
            self.tape.append(t)
        return t

    def triple_c1(self, op, xshape, yshape, a0, a1, b0, b1, c0, c1, scratch=None):
        """c1 = (a0 + a1) o (b0 + b1) - c0: the product share that completes a triple whose other five shares are uniform."""
        if op == "mul":
            # element-wise with the smaller operand broadcast over the leading dims
            if a0.numel() >= b0.numel():
                call("primia_triple_mul_c1", a0, a1, b0, b1, c0, c1, a0.numel(), b0.numel())
            else:
                call("primia_triple_mul_c1", b0, b1, a0, a1, c0, c1, b0.numel(), a0.numel())
        else:
            # a [B, L, K] operand (conv2d of a batch) is the [B*L, K] matrix: the leading dimensions are rows
            K, N = xshape[-1], yshape[-1]
            M = int(torch.Size(xshape).numel()) // K
            if scratch is None:
                scratch = torch.empty(M * K + K * N, dtype=I64, device=self.device)
            call("primia_triple_matmul_c1", a0, a1, b0, b1, c0, c1, scratch, M, K, N)

    def dif_keys(self, n, bits=None):
        """bits=None: keys of the dealer's comparison width; a value: keys of that width -- the same keystream words are drawn,
        the width decides their reduction and the number of levels (the rank comparisons of an evaluation with a ROC AUC
        are 64 bits wide whatever the dealer's width, SecureContext.auc_counts)."""
        if self.requests is not None:
            self.requests.append(("dif_keys", (n,), {} if bits is None else {"bits": int(bits)}))
        dev, w = self.device, self.fss_bits if bits is None else check_fss_bits(bits)
        # raw keystream words, then build_fss_keys' arithmetic in place (primia_fss_alpha_split): alpha and its mask r below
        # 2^32 (mpc/fss.py:346, mpc/primitives.py:249), word 0 of each seed 63 bits (randbit, fss.py:495-501), and
        # primitives.py:249-251: party 0 receives (alpha - mask) mod 2^32, party 1 the mask (2^fss_bits at another width: the
        # same words are drawn, the width decides their reduction)
        alpha = self.rand64(n)
        s0 = self.rand64(2, 2, n)
        r = self.rand64(n)
        a0 = torch.empty(n, dtype=I64, device=dev)
        fss_call("fss_alpha_split", w, alpha, s0, r, a0, n)
        bits, cw_sigma, cw_s, leaf = (torch.empty(shape, dtype=dt, device=dev) for shape, dt in dif_key_fields(n, w))
        fss_call("dif_keygen", w, alpha, s0, bits, cw_sigma, cw_s, leaf, n)
        keys = [dict(alpha=[a0, r][b], s0=s0[b], bits=bits, cw_sigma=cw_sigma, cw_s=cw_s, cw_leaf=leaf) for b in range(2)]
        if self.log is not None:
            self.log.append(("dif", n, alpha.cpu().numpy(), s0.cpu().numpy(), r.cpu().numpy()))
        if self.tape is not None:
            self.tape.append(keys)
        return keys

    def dpf_keys(self, n):
        """Keys of n equality tests (fss.eq, the reference's DPF): the raw words of dif_keys -- alpha, both parties' seeds,
        alpha's mask -- and the same split of alpha, always mod 2^32: the operands are class indices, and equality mod 2^32
        has no error term, so the dealer's comparison width does not enter."""
        if self.requests is not None:
            self.requests.append(("dpf_keys", (n,), {}))
        dev = self.device
        alpha = self.rand64(n)
        s0 = self.rand64(2, 2, n)
        r = self.rand64(n)
        a0 = torch.empty(n, dtype=I64, device=dev)
        call("primia_fss_alpha_split", alpha, s0, r, a0, n)
        bits, cw_s, cw_n = (torch.empty(shape, dtype=dt, device=dev) for shape, dt in dpf_key_fields(n))
        call("primia_dpf_keygen", alpha, s0, bits, cw_s, cw_n, n)
        keys = [dict(alpha=[a0, r][b], s0=s0[b], bits=bits, cw_s=cw_s, cw_n=cw_n) for b in range(2)]
        if self.log is not None:
            self.log.append(("dpf", n, alpha.cpu().numpy(), s0.cpu().numpy(), r.cpu().numpy()))
        if self.tape is not None:
            self.tape.append(keys)
        return keys

    def const_mask(self, *shape, owner=None):
        """The mask of a fresh sharing; `owner` (None = public value, else the party that holds the secret)
        only matters to a distributed dealer, which sends the mask to the owner alone."""
        if self.requests is not None:
            self.requests.append(("const_mask", tuple(shape), {"owner": owner}))
        r = self.rand64(*shape)
        if self.log is not None:
            self.log.append(("mask", r.cpu().numpy()))
        if self.tape is not None:
            self.tape.append(r)
        return r


def dif_key_fields(n, bits=FSS_BITS):
    """(shape, dtype) of the correction words of n comparisons at width `bits`, common to both parties: the packed control
    bits, cw_sigma, cw_s and the leaf words (include/primia_hip.h)."""
    return [((bits, n), torch.uint8), ((bits, 2, n), I64), ((bits, 2, n), I64), ((bits + 1, n), torch.int32)]


def dpf_key_fields(n):
    """(shape, dtype) of the correction words of n equality tests, common to both parties: the packed control bits, cw_s and
    the leaf word (include/primia_hip.h; always 32 levels)."""
    return [((FSS_BITS, n), torch.uint8), ((FSS_BITS, 2, n), I64), ((n,), I64)]


class PreloadedDealer:
    """Online phase only: hands out primitives that a Dealer generated earlier (its `tape`), in
    the same order — the reference's pre-provisioned crypto store (mpc/primitives.py:161-235).  `fss_bits`: the width of
    the dealer that generated them."""

    def __init__(self, tape, device, fss_bits=FSS_BITS):
        self.tape, self.pos, self.device = tape, 0, torch.device(device)
        self.fss_bits = check_fss_bits(fss_bits)
        self.log = None

    def _next(self):
        v = self.tape[self.pos]
        self.pos += 1
        return v

    def triple(self, op, xshape, yshape):
        return self._next()

    def dif_keys(self, n, bits=None):
        return self._next()

    def dpf_keys(self, n):
        return self._next()

    def const_mask(self, *shape, owner=None):
        return self._next()


class LocalOpener:
    """Both parties' shares live on this GPU: open = one ring add."""

    def open(self, shares):
        out = _empty_like(shares[0])
        call("primia_ring_add", shares[0], shares[1], out, shares[0].numel(), shares[0].numel())
        return out


class DistOpener:
    """One party per rank (party j = rank j of the 2-rank party group, e.g. two GPUs over xGMI): open = an
    int64 all_reduce(SUM) of the local share, which wraps mod 2^64 — the 2-party exchange the reference routes
    through the orchestrator (mpc/spdz.py:162-176, mpc/fss.py:158-170)."""

    def __init__(self, group=None, party=None):
        import torch.distributed as dist

        self.dist, self.group = dist, group
        self.party = dist.get_rank(group) if party is None else party

    def open(self, shares):
        mine = shares[self.party].clone()
        self.dist.all_reduce(mine, op=self.dist.ReduceOp.SUM, group=self.group)
        return mine


class SecureContext:
    def __init__(self, dealer, base=10, precision_fractional=16, opener=None, party=None, link=None, faithful_trunc=False):
        """party=None: both parties' shares live in this process (a share is a 2-list).  party=j: this process
        is party j of a distributed run — every 2-list carries only entry j (the other is None), `opener` must
        be a DistOpener and `link` a PartyLink for the owner-to-peer transfer of freshly shared secrets.
        faithful_trunc=True: conv2d, affine_eval and linear truncate their products with `trunc_faithful`, which no mask
        can make wrap, where the reference's per-share division is off by 2^64 / scale with probability |z| / 2^64."""
        self.dealer = dealer
        self.faithful_trunc = bool(faithful_trunc)
        self.base = base
        self.pf = precision_fractional
        self.scale = base ** precision_fractional
        self.opener = opener or LocalOpener()
        self.party = party
        self.parties = (0, 1) if party is None else (party,)
        self.link = link
        self.stats = {"beaver_mul": 0, "beaver_matmul": 0, "dif_evals": 0}
        self.fuse_newton = True
        self._newton_tables, self._newton_calls = [], 0     # see _reciprocal_newton_fused
        self._wt_cache = {}                                 # transposed weight shares of conv2d / linear (static per model)

    # Both parties hosted here: a layer's mask -> open -> combine -> truncate -> re-layout chain runs as one pass over the
    # shares of party 0 AND party 1 (csrc/secure_local.hip; an open is an addition of two values that sit side by side).
    # The dealer's primitives are requested in exactly the order of the step-by-step chain, results are bit-identical;
    # `local_fused = False` selects the chain (what a three-role run executes, where the opens are messages).
    local_fused = True

    @property
    def fss_bits(self):
        """The width of the comparisons, which is the width of the dealer's keys (32 for a dealer that names none)."""
        return getattr(self.dealer, "fss_bits", FSS_BITS)

    @property
    def _in_process(self):
        return self.party is None and isinstance(self.opener, LocalOpener)

    @property
    def _local(self):
        return self._in_process and self.local_fused

    # ---- encode / share / reconstruct -----------------------------------------------------------
    def encode(self, x):
        q = torch.empty(x.shape, dtype=I64, device=x.device)
        call("primia_fx_encode", x.contiguous().to(torch.float32), q, x.numel(), float(self.scale))
        return q

    def decode(self, q):
        x = torch.empty(q.shape, dtype=torch.float32, device=q.device)
        call("primia_fx_decode", q, x, q.numel(), float(self.scale))
        return x

    def share(self, q, owner=None, shape=None):
        """share_secret (additive_shared.py:317-365): (r, q - r) with r from the crypto provider.
        `owner`: the party that knows q (0 = model owner, 1 = data owner) or None for a value both parties
        know.  In a distributed run the mask goes to the owner only (to both for a public value); the owner
        forms q - r and hands the peer ITS share; a non-owner passes q = None and `shape`."""
        shape = tuple(q.shape) if q is not None else tuple(shape)
        if self.party is None:
            r = self.dealer.const_mask(*shape, owner=owner)
            s1 = _empty_like(q)
            call("primia_ring_sub", q, r, s1, q.numel(), q.numel())
            return [r, s1]
        me, out = self.party, [None, None]
        if owner is None or owner == me:
            r = self.dealer.const_mask(*shape, owner=owner)
            s1 = _empty_like(r)
            call("primia_ring_sub", q, r, s1, r.numel(), r.numel())
            mine, theirs = (r, s1) if me == 0 else (s1, r)
            out[me] = mine
            if owner is not None:
                self.link.send_to_peer(theirs)
        else:
            out[me] = self.link.recv_from_peer(shape)
        return out

    def reconstruct(self, x):
        return self.opener.open(x)

    def _ref(self, x):
        """The share this process holds (shapes / devices are read from it)."""
        return x[self.parties[0]]

    def _each(self, fn):
        """[fn(j) for the parties hosted here], as a 2-list."""
        out = [None, None]
        for j in self.parties:
            out[j] = fn(j)
        return out

    # ---- local (per-share) ops -------------------------------------------------------------------
    def _ew(self, fn, a, b):
        if self._local and fn in ("primia_ring_add", "primia_ring_sub"):
            big, small = a[0], b[0]
            if small.numel() > big.numel():
                raise ValueError("second operand must not be larger")
            o = [_empty_like(big), _empty_like(big)]
            call("primia_ring_ew_2p", 0 if fn == "primia_ring_add" else 1, a[0], a[1], b[0], b[1], o[0], o[1], big.numel(),
                 small.numel())
            return o

        def one(j):
            big, small = (a[j], b[j])
            if small.numel() > big.numel():
                raise ValueError("second operand must not be larger")
            o = _empty_like(big)
            call(fn, big, small, o, big.numel(), small.numel())
            return o

        return self._each(one)

    def add(self, a, b):
        return self._ew("primia_ring_add", a, b)

    def sub(self, a, b):
        return self._ew("primia_ring_sub", a, b)

    def neg(self, a):
        def one(j):
            o = _empty_like(a[j])
            call("primia_ring_scale", a[j], -1, o, a[j].numel())
            return o

        return self._each(one)

    def trunc(self, a, d):
        def one(j):
            o = _empty_like(a[j])
            call("primia_trunc_div", a[j], int(d), o, a[j].numel())
            return o

        return self._each(one)

    def _carry_triple(self, shape):
        """The triple of a faithful truncation's carry product, requested right after the site's product triple."""
        self.stats["beaver_mul"] += 1
        return self.dealer.triple("mul", tuple(shape), tuple(shape))

    def trunc_faithful(self, z, d):
        """Shares of floor(z / d) + e, e in {-1, 0, 1, 2}, for EVERY mask, from shares z of a value |z| < 2^62.  The
        reference has no such form (each party divides its own share, which is off by 2^64 / d whenever the signed shares
        wrap: with probability |z| / 2^64 over the mask); it is DEFINED by tests/secure_faithful_nets.py's
        oracle_trunc_faithful and not pinned against the reference.  On unsigned words mod 2^64:
          u_0 = z_0 + 2^62, u_1 = z_1                 shares of z + 2^62, which lies in [0, 2^63)
          m_j = u_j >> 63                              party local; the carry of u_0 + u_1 is m_0 OR m_1
          p   = beaver_mul([m_0, 0], [0, m_1])         triple ("mul", shape, shape), both opens, no truncation
          out_j = u_j / d - (m_j - p_j) floor(2^64 / d) - [j = 0] floor(2^62 / d)
        Both parties here: one launch (primia_trunc_faithful_col2out_2p in its identity layout); otherwise the chain, which
        a three-role run executes -- same dealer request, same bits."""
        zr = self._ref(z)
        shape, n, dev = tuple(zr.shape), zr.numel(), zr.device
        t = self._carry_triple(shape)
        if self._local:
            out = _pair(shape, dev)
            call("primia_trunc_faithful_col2out_2p", z[0].contiguous(), z[1].contiguous(), None, None, _ptr_table(t), out[0],
                 out[1], 1, 1, n, int(d))
            return out
        u, m = [None, None], [None, None]
        for j in self.parties:
            u[j] = z[j].contiguous()
            if j == 0:
                u[j] = _empty_like(u[j])
                call("primia_ring_add", z[j].contiguous(), self._const(2 ** 62, dev), u[j], n, 1)
            m[j] = _empty_like(u[j])
            call("primia_trunc_carry_bits", u[j], m[j], n)
        zero = self._const(0, dev, n)
        dm, em = [None, None], [None, None]
        for j in self.parties:  # spdz_mask: the first operand is [m_0, 0], the second [0, m_1]
            dm[j], em[j] = _empty_like(u[j]), _empty_like(u[j])
            call("primia_beaver_mask", m[j] if j == 0 else zero, t[j][0], dm[j], n, zero if j == 0 else m[j], t[j][1], em[j], n)
        delta, eps = self.opener.open(dm), self.opener.open(em)

        def one(j):
            p = _empty_like(u[j])
            call("primia_beaver_combine_mul", j, delta, eps, *t[j], p, n, n)
            o = _empty_like(u[j])
            call("primia_trunc_faithful_finish", j, u[j], m[j], p, int(d), o, n)
            return o

        return self._each(one)

    def trunc_product(self, z):
        """The truncation of a product at scale s^2 back to s: the reference's per-share division, or `trunc_faithful`."""
        return self.trunc_faithful(z, self.scale) if self.faithful_trunc else self.trunc(z, self.scale)

    def sub_public_scalar(self, a, value):
        """AST - int (additive_shared.py:453-484, 506-524): the constant becomes a FRESH random
        sharing of shape [1] that is subtracted share-wise (broadcast)."""
        return self.sub(a, self.share(self._const(int(value), self._ref(a).device)))

    def _const(self, value, device, n=1):
        """A public constant as a device tensor, uploaded once per (value, length) and kept (no fill kernel per use; a captured
        forward finds it in the cache its eager pass filled — an upload cannot be captured)."""
        cache = self.__dict__.setdefault("_consts", {})
        key = (value, n, str(device))
        if key not in cache:
            cache[key] = torch.full((n,), value, dtype=I64).to(device)
        return cache[key]

    # ---- Beaver -----------------------------------------------------------------------------------
    def beaver_mul(self, x, y, trunc=None):
        """Element-wise private product; trunc = d: followed by each party's truncation of its share by d (fpt_mul).
        One operand may be a vector broadcast over the other's leading dims; the ring product is symmetric so the
        big one is taken first."""
        xr, yr = self._ref(x), self._ref(y)
        swap = xr.numel() < yr.numel()
        t = self.dealer.triple("mul", tuple(xr.shape), tuple(yr.shape))
        if swap:
            x, y, xr, yr = y, x, yr, xr
            t = [None if tj is None else (tj[1], tj[0], tj[2]) for tj in t]
        n, nb = xr.numel(), yr.numel()
        if self._local:
            out = [_empty_like(xr), _empty_like(xr)]
            call("primia_fpt_mul_local", x[0], x[1], y[0], y[1], *_six(t), None, None, out[0], out[1], n, nb,
                 0 if trunc is None else int(trunc))
            self.stats["beaver_mul"] += 1
            return out
        d, e = [None, None], [None, None]
        for j in self.parties:  # spdz_mask
            d[j], e[j] = _empty_like(xr), _empty_like(yr)
            call("primia_beaver_mask", x[j], t[j][0], d[j], n, y[j], t[j][1], e[j], nb)
        delta, eps = self.opener.open(d), self.opener.open(e)

        def one(j):  # spdz_compute
            o = _empty_like(xr)
            if trunc is not None:
                call("primia_beaver_combine_mul_trunc", j, delta, eps, *t[j], o, n, nb, int(trunc))
            else:
                call("primia_beaver_combine_mul", j, delta, eps, *t[j], o, n, nb)
            return o

        self.stats["beaver_mul"] += 1
        return self._each(one)

    def beaver_matmul(self, x, y):
        """x [..., K] @ y [K, N]: the leading dimensions of x are rows of ONE product (a batch's [B, L, K] im2col operand is
        the [B*L, K] matrix); the triple is requested with the operand's own shape, as the reference's batched call does."""
        xr, yr = self._ref(x), self._ref(y)
        K, N = xr.shape[-1], yr.shape[-1]
        M = xr.numel() // K
        t = self.dealer.triple("matmul", tuple(xr.shape), tuple(yr.shape))
        if self._local:
            out = _pair((*xr.shape[:-1], N), xr.device)
            scratch = torch.empty(M * K + 2 * K * N, dtype=I64, device=xr.device)
            call("primia_beaver_matmul_local", x[0], x[1], y[0], y[1], *_six(t), out[0], out[1], scratch, M, K, N)
            self.stats["beaver_matmul"] += 1
            return out
        d, e = [None, None], [None, None]
        for j in self.parties:
            d[j], e[j] = _empty_like(xr), _empty_like(yr)
            call("primia_beaver_mask", x[j], t[j][0], d[j], xr.numel(), y[j], t[j][1], e[j], yr.numel())
        delta, eps = self.opener.open(d), self.opener.open(e)
        scratch = torch.empty(K * N, dtype=I64, device=xr.device)

        def one(j):
            o = torch.empty(*xr.shape[:-1], N, dtype=I64, device=xr.device)
            call("primia_beaver_combine_matmul", j, delta, eps, *t[j], o, scratch, M, K, N)
            return o

        self.stats["beaver_matmul"] += 1
        return self._each(one)

    def fpt_mul(self, x, y):
        """FPT * FPT (precision.py:309-316, 356-358): Beaver mul, then per-share truncation."""
        return self.beaver_mul(x, y, trunc=self.scale)

    def fpt_matmul(self, x, y):
        """FPT @ FPT (precision.py:419-463)."""
        return self.trunc(self.beaver_matmul(x, y), self.scale)

    # ---- FSS comparison ------------------------------------------------------------------------------
    def _dif_keys(self, n, bits):
        """(keys, width) of n comparisons: the dealer's width, or `bits` when the caller fixes one."""
        if bits is None:
            return self.dealer.dif_keys(n), self.fss_bits
        return self.dealer.dif_keys(n, bits=bits), check_fss_bits(bits)

    def _le_local(self, x1, x2, n, shape, cols1=(1, 0), cols2=(1, 0), length=1, bits=None):
        """fss.le with both parties here: mask_builder, the open and both DIF evaluations in one launch.  x1 = None stands
        for shares of zero; colsK = (row width, first column) when operand K is a column range of a matrix; bits: a width
        other than the dealer's."""
        keys, w = self._dif_keys(n, bits)
        out = _pair(shape, x2[0].device)
        k0, k1 = keys
        fss_call("dif_eval_local", w, None if x1 is None else x1[0], None if x1 is None else x1[1], cols1[0], cols1[1],
                 x2[0], x2[1], cols2[0], cols2[1], length, k0["alpha"], k1["alpha"], k0["s0"], k1["s0"], k0["bits"],
                 k0["cw_sigma"], k0["cw_s"], k0["cw_leaf"], out[0], out[1], n)
        self.stats["dif_evals"] += n
        return out

    def le(self, x1, x2, bits=None):
        """fss.le(x1, x2) (mpc/fss.py:97-185, 279): int64 shares of the bit [x1 <= x2], compared at the dealer's width or at
        `bits` (requested as dif_keys(n, bits=bits))."""
        xr = self._ref(x1)
        n = xr.numel()
        if self._local:
            return self._le_local(x1, x2, n, tuple(xr.shape), bits=bits)
        keys, w = self._dif_keys(n, bits)
        r = [None, None]
        for j in self.parties:  # mask_builder
            r[j] = _empty_like(xr)
            call("primia_fss_mask", x1[j], x2[j], keys[j]["alpha"], r[j], n)
        masked = torch.empty(n, dtype=masked_dtype(w), device=xr.device)
        if self.party is None:
            fss_call("fss_open", w, r[0], r[1], masked, n)
        else:  # the parties exchange their masked shares; the sum is taken mod 2^32 (fss.py:158-170; mod 2^fss_bits)
            opened = self.opener.open(r)
            fss_call("fss_open", w, opened, self._const(0, opened.device, opened.numel()), masked, n)

        def one(j):  # evaluate
            o = _empty_like(xr)
            k = keys[j]
            fss_call("dif_eval", w, j, masked, k["s0"], k["bits"], k["cw_sigma"], k["cw_s"], k["cw_leaf"], o, n)
            return o

        self.stats["dif_evals"] += n
        return self._each(one)

    def relu(self, x):
        """AST.relu under fss (additive_shared.py:922-925): x * (x >= 0), (x >= 0) = le(x - x, x)."""
        if self._local:      # le(x - x, x): the first operand is a sharing of zero (no launch for it)
            xr = x[0]
            return self.beaver_mul(x, self._le_local(None, x, xr.numel(), tuple(xr.shape)))
        zero = self.sub(x, x)
        return self.beaver_mul(x, self.le(zero, x))

    def _max_pair(self, left, right):
        """left + (right >= left) * (right - left)  (nn/functional.py:494)."""
        bit = self.le(left, right)
        return self.add(left, self.beaver_mul(bit, self.sub(right, left)))

    def _max_pair_cols(self, left, wl, sl, right, wr, sr, rows, length):
        """_max_pair on column ranges (both parties here): comparison, Beaver product and the final add in two launches."""
        n = rows * length
        bit = self._le_local(left, right, n, (rows, length), (wl, sl), (wr, sr), length)
        t = self.dealer.triple("mul", (rows, length), (rows, length))
        out = _pair((rows, length), left[0].device)
        call("primia_max_combine_local", bit[0], bit[1], left[0], left[1], wl, sl, right[0], right[1], wr, sr, *_six(t),
             out[0], out[1], rows, length)
        self.stats["beaver_mul"] += 1
        return out

    def _cols(self, x, rows, w, start, length):
        def one(j):
            o = torch.empty(rows, length, dtype=I64, device=x[j].device)
            call("primia_ring_slice_cols", x[j], o, rows, w, start, length)
            return o

        return self._each(one)

    # ---- argmax: the tail that opens the predicted class only --------------------------------------------------
    def argmax(self, x, values=False):
        """Shares of the first-index argmax over the classes of the logits x [B, C] -- raw, unscaled int64 [B] -- so that a
        pass can open the predicted class and nothing else.  The reference has no such layer: it is DEFINED here from the
        reference's operations (tests/secure_argmax_nets.py's oracle_argmax) and is not pinned against the
        reference.  V = x[:, C-1], I = share(C-1); then for k = C-2 .. 0:
          bit = le(V, x[:, k])                       dif_keys(B)
          K   = share(full([B], k))                  const_mask(B): a public constant, re-shared like every other
          R   = beaver_mul(bit2, [x[:, k] - V, K - I])       triple ("mul", (B, 2), (B, 2)); the bit is unscaled: no truncation
          V  += R[:, 0];  I += R[:, 1]
        Walking down with [x_k >= V] sends a tie to the lower index, torch.argmax's rule.  The comparison sees the low
        `fss_bits` bits of the masked difference (32 unless the dealer says otherwise): the result is the true argmax while all
        pairwise differences of the encoded logits stay below 2^(fss_bits-1), and a deterministic function of the wrapped values
        otherwise.  (Like every comparison of the reference, one on a difference d errs with probability |d| / 2^fss_bits over
        the dealer's mask: 2e-7 at 32 bits for two pf = 3 logits 1.0 apart.)
        Both parties here: two launches per class (primia_dif_eval_local, primia_argmax_combine_local); otherwise the
        step-by-step chain, which a three-role run executes -- same dealer requests, same bits.
        values=True: (I, V), with the shares of the maximum as well (tests; a deployment opens I alone)."""
        xr = self._ref(x)
        if xr.dim() != 2 or xr.shape[1] < 1:
            raise ValueError(f"argmax takes logits [B, classes], got {tuple(xr.shape)}")
        B, C = xr.shape
        dev = xr.device
        x = self._each(lambda j: x[j].contiguous())
        flat = lambda t: [None if q is None else q.view(B) for q in t]
        V = flat(self._cols(x, B, C, C - 1, 1))

        first = self.share(self._const(C - 1, dev, B))

        def own(j):      # (party 0's share of a fresh sharing IS the dealer's mask: I is updated in place, so it gets buffers of its own)
            o = _empty_like(first[j])
            call("primia_ring_scale", first[j], 1, o, B)
            return o

        I = self._each(own)
        for k in range(C - 2, -1, -1):
            if self._local:
                bit = self._le_local(V, x, B, (B,), (1, 0), (C, k), 1)
                K = self.share(self._const(k, dev, B))
                t = self.dealer.triple("mul", (B, 2), (B, 2))
                call("primia_argmax_combine_local", bit[0], bit[1], x[0], x[1], C, k, K[0], K[1], *_six(t), V[0], V[1], I[0],
                     I[1], B)
                self.stats["beaver_mul"] += 1
                continue
            Lk = flat(self._cols(x, B, C, k, 1))
            bit = self.le(V, Lk)
            K = self.share(self._const(k, dev, B))
            R = self.beaver_mul(self._stack2(bit, bit, B), self._stack2(self.sub(Lk, V), self.sub(K, I), B))
            Rt = self._each(lambda j: _transposed(R[j], B, 2))
            V = self.add(V, self._each(lambda j: Rt[j][0]))
            I = self.add(I, self._each(lambda j: Rt[j][1]))
        return (I, V) if values else I

    # ---- equality and the confusion-matrix tail of an encrypted evaluation ---------------------------------------
    def eq(self, x1, x2, cols1=(1, 0), cols2=(1, 0), length=1, shape=None):
        """fss.eq(x1, x2) (mpc/fss.py:97-185 with op = "eq"): raw int64 shares of the bit [x1 == x2 mod 2^32], one DPF key per
        element (`dpf_keys(n)`, row-major).  Always 32 bits wide: equality has no error term, and what it compares here are
        class indices.  Both parties here: mask, open and both evaluations in one launch (primia_dpf_eval_local), where
        colsK = (row width, first column) and `length` make operand K a column range of a matrix and `shape` = (rows, length)
        the result's; otherwise primia_fss_mask, the open and primia_dpf_eval, on whole tensors -- same keys, same bits."""
        ref = self._ref(x2)
        shape = tuple(ref.shape) if shape is None else tuple(shape)
        n = int(torch.Size(shape).numel())
        keys = self.dealer.dpf_keys(n)
        self.stats["dpf_evals"] = self.stats.get("dpf_evals", 0) + n
        if self._local:
            out = _pair(shape, ref.device)
            k0, k1 = keys
            call("primia_dpf_eval_local", x1[0], x1[1], cols1[0], cols1[1], x2[0], x2[1], cols2[0], cols2[1], length,
                 k0["alpha"], k1["alpha"], k0["s0"], k1["s0"], k0["bits"], k0["cw_s"], k0["cw_n"], out[0], out[1], n)
            return out
        if (cols1, cols2, length) != ((1, 0), (1, 0), 1):
            x1 = self._cols(x1, n // length, cols1[0], cols1[1], length)
            x2 = self._cols(x2, n // length, cols2[0], cols2[1], length)
        r = [None, None]
        for j in self.parties:  # mask_builder
            r[j] = torch.empty(n, dtype=I64, device=ref.device)
            call("primia_fss_mask", x1[j], x2[j], keys[j]["alpha"], r[j], n)
        masked = torch.empty(n, dtype=torch.int32, device=ref.device)
        if self.party is None:
            call("primia_fss_open", r[0], r[1], masked, n)
        else:
            opened = self.opener.open(r)
            call("primia_fss_open", opened, self._const(0, opened.device, n), masked, n)

        def one(j):  # evaluate
            o = torch.empty(shape, dtype=I64, device=ref.device)
            k = keys[j]
            call("primia_dpf_eval", j, masked, k["s0"], k["bits"], k["cw_s"], k["cw_n"], o, n)
            return o

        return self._each(one)

    def _class_grid(self, B, C, device):
        """tile(arange(C), (B, 1)) as a device tensor, uploaded once per shape and kept (see _const)."""
        cache = self.__dict__.setdefault("_consts", {})
        key = ("class_grid", B, C, str(device))
        if key not in cache:
            cache[key] = torch.arange(C, dtype=I64).repeat(B, 1).contiguous().to(device)
        return cache[key]

    def confusion(self, logits, labels_onehot, acc, kept=None):
        """One pass of an encrypted evaluation (defined by tests/secure_confusion_nets.py's oracle_confusion, not
        pinned against the reference, which opens the predictions): acc += Y^T @ onehot(argmax(logits)) on shares, nothing
        opened but masked operands.  logits: shares [B, C]; labels_onehot: the data owner's raw int64 one-hot labels [B, C]
        (all-zero rows for padding images; None in the process of party 0); acc: the shares of the [C, C] confusion matrix,
        updated IN PLACE -- acc[j][k] counts label j predicted as k.
          I    = argmax(logits)                        the class form's tail and requests, unchanged
          Y    = share(labels_onehot, owner=1)         const_mask((B, C), owner=1)
          Kmat = share(tile(arange(C), (B, 1)))        const_mask((B, C)); Ib = I repeated along the classes, party-local
          P    = eq(Ib, Kmat)                          dpf_keys(B * C)
          acc += beaver_matmul(Y^T, P)                 triple ("matmul", (C, B), (B, C)), no truncation
        Both parties here: primia_dpf_eval_local and primia_confusion_combine_local (Y is read row-major, no transposed
        copy); otherwise the step-by-step chain -- same requests, same bits.  Returns the shares of P (tests).
        kept: a list that receives this pass's (logits, Y) shares, copied party-locally (reveal="metrics": the rank-count
        tail after the last pass reads them; the requests are unchanged)."""
        xr = self._ref(logits)
        B, C = xr.shape
        dev = xr.device
        I = self.argmax(logits)
        if self.party in (None, 1):
            if labels_onehot is None or tuple(labels_onehot.shape) != (B, C) or labels_onehot.dtype != I64:
                raise ValueError(f"the data owner passes int64 one-hot labels [{B}, {C}]")
            Y = self.share(labels_onehot.contiguous(), owner=1)
        else:
            Y = self.share(None, owner=1, shape=(B, C))
        if kept is not None:
            kept.append((self._copy(logits), self._copy(Y)))
        Kmat = self.share(self._class_grid(B, C, dev))
        zero = self._const(0, dev, C * B)
        rows = self.add(self._each(lambda j: zero), I)                  # [C, B]: every row is I
        Ib = self._each(lambda j: _transposed(rows[j], C, B))           # [B, C]: I repeated along the class axis
        P = self.eq(Ib, Kmat)
        if self._local:
            t = self.dealer.triple("matmul", (C, B), (B, C))
            call("primia_confusion_combine_local", Y[0], Y[1], P[0], P[1], *_six(t), acc[0], acc[1], B, C)
            self.stats["beaver_matmul"] += 1
            return P
        Mc = self.beaver_matmul(self._each(lambda j: _transposed(Y[j], B, C)), P)
        for j in self.parties:      # (out of place, then back into the accumulator's own buffer)
            o = _empty_like(acc[j])
            call("primia_ring_add", acc[j], Mc[j], o, C * C, C * C)
            acc[j].copy_(o)
        return P

    def _copy(self, x):
        """A party-local copy of shares, by the library's own copy (a ring scale by 1)."""
        def one(j):
            src = x[j].contiguous()
            o = _empty_like(src)
            call("primia_ring_scale", src, 1, o, src.numel())
            return o

        return self._each(one)

    def auc_counts(self, logits, labels_onehot, U, block_rows=None):
        """The rank counts of the reference's one-vs-one ROC AUC over all rows of an encrypted evaluation (DESIGN.md §4;
        defined by tests/secure_auc_nets.py's oracle_auc_counts, not pinned against the reference, which computes the AUC on
        opened scores): U[p][a][q] += #{(i, j): label(i) = p, label(j) = q, p_a(i) <= p_a(j)} on shares, for the
        min-shifted, row-normalised scores p_a = n_a / d -- nothing opened but masked operands.  logits: shares of the
        fixed-point logits [N, C] of every row held; labels_onehot: SHARES of the raw one-hot labels [N, C] (all-zero rows
        for padding images), the ones the confusion tail made; U: shares [C, C, C], updated IN PLACE.  Raw int64, no scale.
          Vn  = argmax(-L, values=True)[1]             the class form's walk and requests on -L, its index dropped
          n   = L + Vn[:, None];  d = rowsum(n)        party-local (n^T = L^T + Vn, then transposed back)
          per block of Rb = auc_block_rows(N, C) rows (the last ragged), R rows `blk`:
            A  = beaver_matmul(n[blk] [R C, 1], d [1, N])          triple ("matmul", (R C, 1), (1, N))
            Bm = beaver_matmul(d[blk] [R, 1], n^T [1, C N])        triple ("matmul", (R, 1), (1, C N))
            G  = le(A, Bm, bits=64) [R, C, N]                      dif_keys(R C N, bits=64): [p_a(i) <= p_a(j)], exact
            T  = beaver_matmul(G [R C, N], Y)                      triple ("matmul", (R C, N), (N, C))
            U += beaver_matmul(Y[blk]^T [C, R], T [R, C C])        triple ("matmul", (C, R), (R, C C))
        The rank comparisons are 64 bits wide whatever the dealer's width: their operands are products of two fixed-point
        values.  The products must stay below 2^63 (pf 3 and 6 with |logit| < 50; at pf 16 they wrap).  A row of all-equal
        logits has d = 0 and ties with every row.
        Both parties here: primia_auc_cross_local (A and Bm in one launch, n and d read in place), primia_dif_eval_local_n,
        primia_beaver_matmul_local and primia_auc_count_combine_local; otherwise the step-by-step chain, which a three-role
        run executes -- same requests, same bits."""
        xr = self._ref(logits)
        if xr.dim() != 2 or tuple(self._ref(labels_onehot).shape) != tuple(xr.shape):
            raise ValueError(f"auc_counts takes logits and one-hot label shares [N, classes], got {tuple(xr.shape)}")
        N, C = xr.shape
        if tuple(self._ref(U).shape) != (C, C, C):
            raise ValueError(f"auc_counts adds into shares [{C}, {C}, {C}]")
        Rb = auc_block_rows(N, C) if block_rows is None else int(block_rows)
        if Rb < 1:
            raise ValueError("block_rows must be at least 1")
        L = self._each(lambda j: logits[j].contiguous())
        Y = self._each(lambda j: labels_onehot[j].contiguous())
        _, Vn = self.argmax(self.neg(L), values=True)
        nT = self.add(self._each(lambda j: _transposed(L[j], N, C)), Vn)      # [C, N]: L^T - min, the minimum broadcast
        n = self._each(lambda j: _transposed(nT[j], C, N))                    # [N, C]

        def rowsum(j):
            o = torch.empty(N, dtype=I64, device=xr.device)
            call("primia_ring_rowsum", n[j], o, N, C)
            return o

        d = self._each(rowsum)
        for r0 in range(0, N, Rb):
            R = min(Rb, N - r0)
            Yb = self._each(lambda j: Y[j][r0:r0 + R])
            if self._local:
                ta = self.dealer.triple("matmul", (R * C, 1), (1, N))
                tb = self.dealer.triple("matmul", (R, 1), (1, C * N))
                A, Bm = _pair((R, C, N), xr.device), _pair((R, C, N), xr.device)
                call("primia_auc_cross_local", n[0], n[1], d[0], d[1], _ptr_table(ta), _ptr_table(tb), A[0], A[1], Bm[0], Bm[1],
                     N, C, r0, R)
                self.stats["beaver_matmul"] += 2
                G = self._le_local(A, Bm, R * C * N, (R, C, N), bits=AUC_BITS)
                T = self.beaver_matmul([g.view(R * C, N) for g in G], Y)
                t = self.dealer.triple("matmul", (C, R), (R, C * C))
                call("primia_auc_count_combine_local", Yb[0], Yb[1], T[0], T[1], *_six(t), U[0], U[1], R, C)
                self.stats["beaver_matmul"] += 1
                continue
            A = self.beaver_matmul(self._each(lambda j: n[j][r0:r0 + R].reshape(R * C, 1)), self._each(lambda j: d[j].view(1, N)))
            Bm = self.beaver_matmul(self._each(lambda j: d[j][r0:r0 + R].reshape(R, 1)), self._each(lambda j: nT[j].view(1, C * N)))
            G = self.le(self._each(lambda j: A[j].view(R, C, N)), self._each(lambda j: Bm[j].view(R, C, N)), bits=AUC_BITS)
            T = self.beaver_matmul(self._each(lambda j: G[j].view(R * C, N)), Y)
            Uc = self.beaver_matmul(self._each(lambda j: _transposed(Yb[j], R, C)), self._each(lambda j: T[j].view(R, C * C)))
            for j in self.parties:      # (out of place, then back into the accumulator's own buffer)
                o = _empty_like(U[j])
                call("primia_ring_add", U[j], Uc[j], o, C * C * C, C * C * C)
                U[j].copy_(o)
        return U

    def auc_open(self, M, U):
        """The opening of an evaluation with a ROC AUC: each party zeroes its shares of the entries U[p][a][q] the score does
        not read -- those with (p == a) == (q == a) -- by a ring product with a public 0 / 1 tensor; then M [C, C] and
        U [C, C, C] are reconstructed through the context's opener, to both parties.  -> (M, U)."""
        C = self._ref(M).shape[0]
        cache = self.__dict__.setdefault("_consts", {})
        dev = self._ref(U).device
        key = ("auc_needed", C, str(dev))
        if key not in cache:
            cache[key] = auc_needed(C).to(I64).to(dev)

        def masked(j):
            o = _empty_like(U[j])
            call("primia_ring_mul", U[j].contiguous(), cache[key], o, C * C * C, C * C * C)
            return o

        return self.reconstruct(M), self.reconstruct(self._each(masked))

    def _stack2(self, a, b, n):
        """stack([a, b], axis=1) of two [n] vectors, per share: [n, 2]."""
        def one(j):
            rows = torch.empty(2, n, dtype=I64, device=a[j].device)
            call("primia_ring_scale", a[j], 1, rows[0], n)
            call("primia_ring_scale", b[j], 1, rows[1], n)
            return _transposed(rows, 2, n)

        return self._each(one)

    def open_to(self, x, to=1):
        """Open x towards party `to` alone: the other party sends its share and learns nothing (the reference `.get()`s a
        prediction to one worker).  With both parties in this process that is `reconstruct`; in a distributed run the
        receiving party returns the value, the sending party None."""
        if self.party is None:
            return self.reconstruct(x)
        mine = x[self.party]
        if self.party != to:
            self.link.send_to_peer(mine)
            return None
        theirs = self.link.recv_from_peer(tuple(mine.shape))
        out = _empty_like(mine)
        call("primia_ring_add", mine, theirs, out, mine.numel(), mine.numel())
        return out

    # ---- layers (nn/functional.py) ------------------------------------------------------------------
    def conv2d(self, x, w, stride, padding):
        """conv2d (nn/functional.py:204-308): per-share im2col, Beaver matmul + truncation,
        per-share reshape.  x shares [B,C,H,W]; w shares [O,C,R,S]; no bias in ResNet convs."""
        B, C, H, W = self._ref(x).shape
        O, _, R, S = self._ref(w).shape
        Ho, Wo = (H + 2 * padding - R) // stride + 1, (W + 2 * padding - S) // stride + 1
        K = C * R * S
        if self._local:
            dev = x[0].device
            im = _pair((B, Ho * Wo, K), dev)
            call("primia_im2col_syft_2p", x[0], x[1], im[0], im[1], B, C, H, W, R, S, stride, padding)
            wt = self._weight_t(w, O, K)
            res = self.beaver_matmul(im, wt)
            out = _pair((B, O, Ho, Wo), dev)
            if self.faithful_trunc:
                tc = self._carry_triple((B, Ho * Wo, O))
                call("primia_trunc_faithful_col2out_2p", res[0], res[1], None, None, _ptr_table(tc), out[0], out[1], B, Ho * Wo,
                     O, int(self.scale))
                return out
            call("primia_trunc_col2out_2p", res[0], res[1], None, None, out[0], out[1], B, Ho * Wo, O, int(self.scale))
            return out
        im, wt = [None, None], [None, None]
        for j in self.parties:
            a = torch.empty(B, Ho * Wo, K, dtype=I64, device=x[j].device)
            call("primia_im2col_syft", x[j], a, B, C, H, W, R, S, stride, padding)
            im[j] = a
            wt[j] = _transposed(w[j], O, K)
        res = self.trunc_product(self.beaver_matmul(im, wt))      # (fpt_matmul, or its faithful form)

        def one(j):
            o = torch.empty(B, O, Ho, Wo, dtype=I64, device=res[j].device)
            call("primia_col2out_syft", res[j], None, o, B, Ho * Wo, O)
            return o

        return self._each(one)

    _wt_cache_max = 64      # a ResNet-18 has 21 shared weight matrices: room for three models on one context

    def _weight_t(self, w, O, K):
        """weight.reshape(O, -1).t() of both parties' (static) weight shares, formed once per model.

        The cache is keyed on the share TENSORS, which it keeps alive (so an address the caching allocator hands out again
        can never alias an entry) and compares by identity together with their in-place version counters.  torch bumps a
        version counter for ITS in-place writes only: a caller that rewrites shares in place through the C ABI (a kernel
        launched on `data_ptr()` — nothing in this module does that to model shares) must call `invalidate_weight_cache()`,
        as `SecureResNet18.__init__` does when a model is (re-)shared.  At most `_wt_cache_max` entries, least recently used
        evicted: a long-lived context fed changing weight objects does not grow."""
        key = (id(w[0]), id(w[1]), O, K)
        hit = self._wt_cache.get(key)
        if hit is not None:
            w0, w1, v0, v1, wt = hit
            if w0 is w[0] and w1 is w[1] and v0 == w[0]._version and v1 == w[1]._version:
                self._wt_cache[key] = self._wt_cache.pop(key)      # most recently used: to the back
                return wt
            del self._wt_cache[key]
        wt = [_transposed(w[j], O, K) for j in (0, 1)]
        while len(self._wt_cache) >= self._wt_cache_max:
            del self._wt_cache[next(iter(self._wt_cache))]
        self._wt_cache[key] = (w[0], w[1], w[0]._version, w[1]._version, wt)
        return wt

    def invalidate_weight_cache(self):
        """Forget every cached transposed weight share (call after re-sharing or editing a model's weights)."""
        self._wt_cache.clear()

    def reciprocal_newton(self, v):
        """FPT.reciprocal(method="newton") (precision.py:507-518), C = 20, 80 iterations.

        With both parties in this process (the default deployment) the whole iteration is ONE launch
        (`primia_newton_reciprocal_local`): the primitives are requested from the dealer in exactly the order the
        step-by-step chain below consumes them and handed to the kernel as a pointer table, so the two forms are
        bit-identical — the chain is what a three-role run (opens = messages) executes, and `fuse_newton = False`
        selects it here too."""
        if self._in_process and self.fuse_newton:
            return self._reciprocal_newton_fused(v)
        C = 20
        # x0 = (C + 1 - v) / C
        y = self.neg(self.sub_public_scalar(v, (C + 1) * self.scale))
        x = self.trunc(y, C)
        for _ in range(79):
            xx = self.fpt_mul(x, x)
            vxx = self.fpt_mul(v, xx)
            y = self.neg(self.sub_public_scalar(vxx, (C + 1) * self.scale))
            x = self.trunc(self.fpt_mul(y, x), C)
        return x

    def rsqrt_newton(self, v):
        """v^-1/2 of shares v at the scale GN_WIDE_SCALE by the UNDAMPED Newton iteration x <- x (3 - v x^2) / 2: a reciprocal
        square root for every 0 < v < 3 / x0^2 (x0 = 0.01: 30,000), where `reciprocal_newton`'s damped form is one on about
        [0.05, 16].  From x0 below v^-1/2 it rises monotonically -- 1.5x per step, then quadratically -- and, in exact arithmetic, never overshoots;
        GN_WIDE_STEPS iterates reach v^-1/2 for v down to the floor of `group_norm(wide=True)`.  Defined by
        tests/secure_gn_wide_nets.py's oracle_rsqrt_newton:
          x_1 = 3 x0 / 2 - trunc(v, 2 / x0^3)          x0 public: party local, party 0 holds the constant, no dealer request
          xx = trunc(x * x, s_it); vxx = trunc(v * xx, s_it); y = 3 s_it - vxx (re-shared constant); x = trunc(y * x, 2 s_it)
        Both parties here: one launch (`primia_rsqrt_newton_local`), its primitives requested in the order the chain below
        consumes them; the chain is what a three-role run executes and what `fuse_newton = False` selects -- same bits."""
        s_it, x0 = GN_WIDE_SCALE, GN_WIDE_X0
        first_div = 2 * s_it ** 3 // x0 ** 3
        if self._in_process and self.fuse_newton:
            shape, n, dev = tuple(v[0].shape), v[0].numel(), v[0].device
            prims = []
            for _ in range(GN_WIDE_STEPS - 1):
                prims += _six(self.dealer.triple("mul", shape, shape))
                prims += _six(self.dealer.triple("mul", shape, shape))
                prims.append(self.dealer.const_mask(1, owner=None))
                prims += _six(self.dealer.triple("mul", shape, shape))
            table = self._newton_table([p.data_ptr() for p in prims], dev)
            out = _pair(shape, dev)
            call("primia_rsqrt_newton_local", v[0].contiguous(), v[1].contiguous(), table, s_it, x0, first_div, GN_WIDE_STEPS,
                 out[0], out[1], n)
            self.stats["beaver_mul"] += 3 * (GN_WIDE_STEPS - 1)
            return out
        x = self.neg(self.trunc(v, first_div))
        if 0 in self.parties:
            x1 = _empty_like(x[0])
            call("primia_ring_add", x[0], self._const(3 * x0 // 2, x[0].device), x1, x1.numel(), 1)
            x[0] = x1
        for _ in range(GN_WIDE_STEPS - 1):
            xx = self.beaver_mul(x, x, trunc=s_it)
            vxx = self.beaver_mul(v, xx, trunc=s_it)
            y = self.neg(self.sub_public_scalar(vxx, 3 * s_it))
            x = self.beaver_mul(y, x, trunc=2 * s_it)
        return x

    def _newton_table(self, ptrs, dev):
        """The device pointer table of a fused iteration's primitives.  Static primitive buffers (pre-provisioned store,
        GraphedSecureInference): cached per call position, so a replayed / captured forward uploads nothing (a
        host-to-device copy cannot be captured into a hipGraph); nothing is retained beyond the table: the tape owns the
        buffers.  Live dealer: fresh primitives every call -- the table is built and every reference dropped (the launch is
        on the current stream and torch's allocator is stream-ordered)."""
        if not isinstance(self.dealer, PreloadedDealer):
            return torch.tensor(ptrs, dtype=I64).to(dev)
        idx = self._newton_calls
        self._newton_calls += 1
        if idx < len(self._newton_tables) and self._newton_tables[idx][0] == ptrs:
            return self._newton_tables[idx][1]
        table = torch.tensor(ptrs, dtype=I64).to(dev)
        if idx < len(self._newton_tables):
            self._newton_tables[idx] = (ptrs, table)
        else:
            self._newton_tables.append((ptrs, table))
        return table

    def _reciprocal_newton_fused(self, v):
        shape = tuple(v[0].shape)
        n = v[0].numel()
        dev = v[0].device
        prims = [self.dealer.const_mask(1, owner=None)]
        for _ in range(79):
            for k in range(3):
                if k == 2:
                    m = self.dealer.const_mask(1, owner=None)
                    prims.append(m)
                t = self.dealer.triple("mul", shape, shape)
                prims += _six(t)
        table = self._newton_table([p.data_ptr() for p in prims], dev)      # (the 237 triples are dropped on return)
        out = _pair(shape, dev)
        call("primia_newton_reciprocal_local", v[0].contiguous(), v[1].contiguous(), table, int(self.scale), out[0], out[1], n)
        self.stats["beaver_mul"] += 3 * 79
        return out

    def _to_rows(self, x, B, C, HW):
        """NCHW shares -> [B*HW, C] rows (row b*HW + p): permute(1,0,2,3).reshape(C,-1).t()."""
        def one(j):
            o = torch.empty(B * HW, C, dtype=I64, device=x[j].device)
            if B == 1:
                call("primia_col2out_syft", x[j], None, o, 1, C, HW)
            else:
                call("primia_nchw_to_rows", x[j], o, B, C, HW)
            return o

        return self._each(one)

    def _affine_to_nchw(self, rows, weight, bias, B, C, H, W, faithful=False):
        """fpt_mul(rows, weight) + bias on [B*H*W, C] rows, back to NCHW: the affine tail of both norms' step-by-step paths.
        faithful: the product is truncated by `trunc_faithful` (a folded norm site of a faithful_trunc context)."""
        prod = self.trunc_faithful(self.beaver_mul(rows, weight), self.scale) if faithful else self.fpt_mul(rows, weight)
        result = self.add(prod, bias)

        def back(j):
            o = torch.empty(B, C, H, W, dtype=I64, device=result[j].device)
            if B == 1:
                call("primia_col2out_syft", result[j], None, o, 1, H * W, C)
            else:
                call("primia_rows_to_nchw", result[j], o, B, C, H * W)
            return o

        return self._each(back)

    def batch_norm_eval(self, x, mean, var, weight, bias, inv=None):
        """batch_norm in eval mode (nn/functional.py:44-75): ((x - mean) * newton(var)) * w + b on
        [H*W, C] rows — no explicit sqrt and no eps, exactly as the reference computes it (its
        "newton" iteration converges to var^-1/2).  `inv` may carry shares of newton(var) computed
        earlier (see SecureResNet18.precompute_inv)."""
        B, C, H, W = self._ref(x).shape
        if self._local:
            if inv is None:
                inv = self.reciprocal_newton(var)
            HW = B * H * W
            t1 = self.dealer.triple("mul", (C,), (HW, C))           # fpt_mul(inv, rows - mean)
            t2 = self.dealer.triple("mul", (HW, C), (C,))           # fpt_mul(normalized, weight)
            out = _pair((B, C, H, W), x[0].device)
            if B == 1:
                call("primia_bn_eval_local", x[0], x[1], mean[0], mean[1], inv[0], inv[1], weight[0], weight[1], bias[0],
                     bias[1], _ptr_table(t1), _ptr_table(t2), out[0], out[1], C, HW, int(self.scale))
            else:
                call("primia_bn_eval_local_batch", x[0], x[1], mean[0], mean[1], inv[0], inv[1], weight[0], weight[1], bias[0],
                     bias[1], _ptr_table(t1), _ptr_table(t2), out[0], out[1], B, C, H * W, int(self.scale))
            self.stats["beaver_mul"] += 2
            return out
        rows = self._to_rows(x, B, C, H * W)
        if inv is None:
            inv = self.reciprocal_newton(var)
        normalized = self.fpt_mul(inv, self.sub(rows, mean))
        return self._affine_to_nchw(normalized, weight, bias, B, C, H, W)

    def affine_eval(self, x, scale, shift):
        """A norm site of a network whose BatchNorm the model owner folded before sharing (`fold_batch_norm`): the
        per-channel map x * scale + shift on shares [B, C, H, W], scale / shift shares [C].  The reference has no such form:
        it is DEFINED here (tests/secure_folded_nets.py's oracle_affine_eval) as exactly the affine tail of
        batch_norm_eval and is not pinned against the reference:
          rows = x.permute(1,0,2,3).reshape(C,-1).t()          [B*H*W, C], row b*H*W + p
          out  = fpt_mul(rows, scale) + shift                  triple ("mul", (B*H*W, C), (C,)), truncation per share
        back in NCHW.  The element order inside the triple is part of the definition.  No Newton iteration: the result
        follows the plaintext BatchNorm for any running statistics.
        Both parties here: one launch (primia_affine_eval_local / _batch); otherwise the step-by-step chain, which a
        three-role run executes -- same dealer request, same bits."""
        B, C, H, W = self._ref(x).shape
        if self._local:
            t = self.dealer.triple("mul", (B * H * W, C), (C,))
            out = _pair((B, C, H, W), x[0].device)
            x = [x[0].contiguous(), x[1].contiguous()]
            self.stats["beaver_mul"] += 1
            if self.faithful_trunc:
                tc = self._carry_triple((B * H * W, C))
                if B == 1:
                    call("primia_affine_eval_faithful_local", x[0], x[1], scale[0], scale[1], shift[0], shift[1], _ptr_table(t),
                         _ptr_table(tc), out[0], out[1], C, H * W, int(self.scale))
                else:
                    call("primia_affine_eval_faithful_local_batch", x[0], x[1], scale[0], scale[1], shift[0], shift[1],
                         _ptr_table(t), _ptr_table(tc), out[0], out[1], B, C, H * W, int(self.scale))
            elif B == 1:
                call("primia_affine_eval_local", x[0], x[1], scale[0], scale[1], shift[0], shift[1], _ptr_table(t), out[0],
                     out[1], C, H * W, int(self.scale))
            else:
                call("primia_affine_eval_local_batch", x[0], x[1], scale[0], scale[1], shift[0], shift[1], _ptr_table(t),
                     out[0], out[1], B, C, H * W, int(self.scale))
            return out
        return self._affine_to_nchw(self._to_rows(x, B, C, H * W), scale, shift, B, C, H, W, faithful=self.faithful_trunc)

    def group_norm(self, x, weight, bias, groups=32, wide=False):
        """GroupNorm(groups, C) on shares [B, C, H, W] -- the norm of the BatchNorm-free network that differentially private
        training builds.  The reference has no secret-shared GroupNorm: this layer is DEFINED here from the reference's
        building blocks and is not pinned against the reference.  With X_j = x_j.reshape(R, m), R = B * groups
        and m = (C / groups) * H * W (a group is m contiguous elements of NCHW):
          mean = trunc_div(row sum of X_j, m)          per share, as AST.mean (additive_shared.py:719-729)
          Xc   = X - mean[:, None]                     party local
          var  = trunc_div(row sum of fpt_mul(Xc, Xc)_j, m)         triple ("mul", (R, m), (R, m))
          inv  = reciprocal_newton(var + eps)          eps = fix_encode(1e-5), a re-shared constant; per layer: it depends
                                                       on the image (batch_norm's does not and is hoisted)
          N    = fpt_mul(inv, Xc.T).T                  triple ("mul", (R,), (m, R))
          out  = fpt_mul(rows(N), weight) + bias       rows [B*H*W, C], exactly batch_norm_eval's affine part
        The Newton iteration approximates v^-1/2 to under 1 % for v in about [0.05, 16]: group variances outside that range
        are normalised wrongly (1.6 % at 0.01, 15 % at 0.001).
        Both parties here: two fused launches around the Newton launch (primia_gn_moments_local, primia_gn_apply_local);
        otherwise the step-by-step chain, which a three-role run executes -- same dealer requests, same bits.

        wide=True: the wide-range form (tests/secure_gn_wide_nets.py's oracle_group_norm_wide), right for any
        group variance in (0, 30,000) and defined for 3 <= precision_fractional <= 6.  With s_it = GN_WIDE_SCALE = 10^6:
          var  = trunc_div(row sum of trunc(beaver_mul(Xc, Xc), s * s / s_it)_j, m)          at scale s_it (pf 3: raw squares)
          inv  = rsqrt_newton(var + eps + floor)       one re-shared constant; floor = GN_WIDE_FLOOR units of 1 / s_it, above
                                                       the truncations' largest negative error: v > 0 for a constant group
          N    = trunc(beaver_mul(inv, Xc.T), s_it).T  at scale s
        and the mean and the affine tail as above; the same triples in the same order, 128 dealer requests per site against
        321.  Launches: primia_gn_moments_wide_local, primia_rsqrt_newton_local, primia_gn_apply_wide_local."""
        B, C, H, W = self._ref(x).shape
        groups = int(groups)
        if groups < 1 or C % groups != 0:
            raise ValueError(f"group_norm: {C} channels do not divide into {groups} groups")
        R, m, HW = B * groups, (C // groups) * H * W, H * W
        scale = int(self.scale)
        if wide:
            check_wide_norm(self.base, self.pf)
            sq_div, inv_div = scale * scale // GN_WIDE_SCALE, GN_WIDE_SCALE
            eps_q = GN_WIDE_SCALE // 100000 + GN_WIDE_FLOOR      # eps = 1e-5 at s_it, and the floor
            newton = self.rsqrt_newton
        else:
            sq_div = inv_div = scale
            eps_q = _eps_q(self.base, self.pf)
            newton = self.reciprocal_newton
        if self._local:
            dev = x[0].device
            x = [x[0].contiguous(), x[1].contiguous()]
            ts = self.dealer.triple("mul", (R, m), (R, m))           # fpt_mul(Xc, Xc)
            mean, var = _pair((R,), dev), _pair((R,), dev)
            n_scratch = _lib.query("primia_gn_moments_local_scratch_elems", R, m)
            scratch = torch.empty(n_scratch, dtype=I64, device=dev) if n_scratch > 0 else None
            call("primia_gn_moments_wide_local" if wide else "primia_gn_moments_local", x[0], x[1], *_six(ts), mean[0], mean[1],
                 var[0], var[1], scratch, R, m, sq_div)
            self.stats["beaver_mul"] += 1
            inv = newton(self.sub_public_scalar(var, -eps_q))
            t1 = self.dealer.triple("mul", (R,), (m, R))             # fpt_mul(inv, Xc.T)
            t2 = self.dealer.triple("mul", (B * HW, C), (C,))        # fpt_mul(rows, weight)
            out = _pair((B, C, H, W), dev)
            if wide:
                call("primia_gn_apply_wide_local", x[0], x[1], mean[0], mean[1], inv[0], inv[1], weight[0], weight[1], bias[0],
                     bias[1], _ptr_table(t1), _ptr_table(t2), out[0], out[1], B, C, HW, groups, inv_div, scale)
            else:
                call("primia_gn_apply_local", x[0], x[1], mean[0], mean[1], inv[0], inv[1], weight[0], weight[1], bias[0],
                     bias[1], _ptr_table(t1), _ptr_table(t2), out[0], out[1], B, C, HW, groups, scale)
            self.stats["beaver_mul"] += 2
            return out

        def transpose(t, rows, cols):      # [rows, cols] -> [cols, rows]
            return self._each(lambda j: _transposed(t[j], rows, cols))

        def row_mean(t):                   # [R, m] -> trunc_div(row sum, m)  [R]
            def one(j):
                s = torch.empty(R, dtype=I64, device=t[j].device)
                call("primia_ring_rowsum", t[j].contiguous(), s, R, m)
                o = _empty_like(s)
                call("primia_trunc_div", s, m, o, R)
                return o

            return self._each(one)

        mean = row_mean(x)
        xct = self.sub(transpose(x, R, m), mean)                     # Xc.T [m, R]: the mean broadcasts over the leading dim
        xc = transpose(xct, m, R)                                    # Xc [R, m]
        var = row_mean(self.beaver_mul(xc, xc, trunc=sq_div))
        inv = newton(self.sub_public_scalar(var, -eps_q))
        nt = self.beaver_mul(inv, xct, trunc=inv_div)                # [m, R]
        n = [None if t is None else t.view(B, C, H, W) for t in transpose(nt, m, R)]
        return self._affine_to_nchw(self._to_rows(n, B, C, HW), weight, bias, B, C, H, W)

    def max_pool2d_3x3s2(self, x):
        """_pool2d(mode="max") for a 3x3 window (nn/functional.py:460-508): unroll to 9 columns,
        binary tree on the first 8, then against the 9th."""
        B, C, H, W = self._ref(x).shape
        Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        rows = B * C * Ho * Wo

        def unroll(j):
            o = torch.empty(rows, 9, dtype=I64, device=x[j].device)
            call("primia_pool_unroll_syft", x[j], o, B, C, H, W, 3, 2, 1)
            return o

        if self._local:
            im = _pair((rows, 9), x[0].device)
            call("primia_pool_unroll_syft_2p", x[0], x[1], im[0], im[1], B, C, H, W, 3, 2, 1)
            res = self._max_pair_cols(im, 9, 0, im, 9, 4, rows, 4)
            res = self._max_pair_cols(res, 4, 0, res, 4, 2, rows, 2)
            left = self._max_pair_cols(res, 2, 0, res, 2, 1, rows, 1)
            res = self._max_pair_cols(left, 1, 0, im, 9, 8, rows, 1)
            return [r.view(B, C, Ho, Wo) for r in res]
        im = self._each(unroll)
        res = self._max_pair(self._cols(im, rows, 9, 0, 4), self._cols(im, rows, 9, 4, 4))
        res = self._max_pair(self._cols(res, rows, 4, 0, 2), self._cols(res, rows, 4, 2, 2))
        left = self._max_pair(self._cols(res, rows, 2, 0, 1), self._cols(res, rows, 2, 1, 1))
        res = self._max_pair(left, self._cols(im, rows, 9, 8, 1))
        return [None if r is None else r.view(B, C, Ho, Wo) for r in res]

    def avg_pool2d(self, x, k):
        """_pool2d(mode="avg"), stride = kernel (nn.AvgPool2d(k)): per-share window sum, then the
        per-share truncating division of AST.mean (additive_shared.py:719-729)."""
        B, C, H, W = self._ref(x).shape
        Ho, Wo = (H - k) // k + 1, (W - k) // k + 1
        rows = B * C * Ho * Wo

        def one(j):
            im = torch.empty(rows, k * k, dtype=I64, device=x[j].device)
            call("primia_pool_unroll_syft", x[j], im, B, C, H, W, k, k, 0)
            s = torch.empty(rows, dtype=I64, device=x[j].device)
            call("primia_ring_rowsum", im, s, rows, k * k)
            o = _empty_like(s)
            call("primia_trunc_div", s, k * k, o, rows)
            return o.view(B, C, Ho, Wo)

        return self._each(one)

    def avg_pool2d_3x3s2(self, x):
        """_pool2d(mode="avg") for AvgPool2d(3, 2, 1), the stem pool of a network trained with pooling_type = avg
        (nn/functional.py:460-525): zero padding of the shares, per-share window sum, then the per-share truncating
        division of AST.mean by 9 for every window, border windows included (count_include_pad, torch's default).  Party
        local -- no comparison, no Beaver product, nothing from the dealer -- and read in place: one launch, no
        [rows, 9] intermediate; bit-identical to the unroll / rowsum / trunc_div chain of `avg_pool2d`."""
        B, C, H, W = self._ref(x).shape
        Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        if self._local:
            out = _pair((B, C, Ho, Wo), x[0].device)
            call("primia_avg_pool_syft_2p", x[0], x[1], out[0], out[1], B, C, H, W, 3, 2, 1)
            return out

        def one(j):
            o = torch.empty(B, C, Ho, Wo, dtype=I64, device=x[j].device)
            call("primia_avg_pool_syft", x[j], o, B, C, H, W, 3, 2, 1)
            return o

        return self._each(one)

    def linear(self, x, w, b):
        """F.linear -> torch.addmm(bias, input, weight.t()) -> FPT.addmm (nn/functional.py:10-14,
        precision.py:822-827): matmul + truncation, then + bias."""
        O, I = self._ref(w).shape
        wt = self._weight_t(w, O, I) if self._local else self._each(lambda j: _transposed(w[j], O, I))
        if self.faithful_trunc and self._local:      # truncation and bias in one launch: HoWo = 1 is the identity layout
            res = self.beaver_matmul(x, wt)
            rows = res[0].numel() // O
            tc = self._carry_triple((rows, O))
            out = _pair(tuple(res[0].shape), res[0].device)
            call("primia_trunc_faithful_col2out_2p", res[0], res[1], b[0], b[1], _ptr_table(tc), out[0], out[1], rows, 1, O,
                 int(self.scale))
            return out
        return self.add(self.trunc_product(self.beaver_matmul(x, wt)), b)


POOLINGS = ("max", "avg")


def _check_pooling(pooling):
    """The stem pool a checkpoint was trained with (train.py's pooling_type)."""
    if pooling not in POOLINGS:
        raise ValueError(f"pooling must be one of {POOLINGS}, got {pooling!r}")
    return pooling


REVEALS = ("logits", "class")      # what a pass of an inference may open, per image
CONFUSION = "confusion"            # an evaluation on labelled images: nothing per image, the confusion matrix at the end
METRICS = "metrics"                # the same evaluation, which also opens the rank counts of the reference's ROC AUC
EVALUATION_REVEALS = REVEALS + (CONFUSION, METRICS)
ACCUMULATING = (CONFUSION, METRICS)

# The rank comparisons of the ROC AUC tail (SecureContext.auc_counts) are 64 bits wide whatever the dealer's
# width -- the mirror image of the equality test fixed at 32: their operands are products of two fixed-point values, whose
# difference reaches about 2^28 at precision_fractional = 3.  They are made in blocks of rows of at most this many.
AUC_BITS = 64
AUC_BLOCK_COMPARISONS = 2 ** 20


def auc_block_rows(rows, classes):
    """Rows per block of the rank-count tail over `rows` rows: a public function of public sizes, and part of the layer's
    definition -- the order of the dealer's requests depends on it."""
    N, C = int(rows), int(classes)
    return max(1, min(N, AUC_BLOCK_COMPARISONS // (C * N)))


def auc_needed(classes):
    """bool [C, C, C]: the entries U[p][a][q] the one-vs-one AUC reads -- exactly one of p, q is the score column a."""
    k = torch.arange(int(classes))
    pa, qa = (k[:, None, None] == k[None, :, None]), (k[None, None, :] == k[None, :, None])
    return pa != qa


def _check_reveal(reveal):
    """What a pass opens (`ProtocolForm`)."""
    if reveal not in EVALUATION_REVEALS:
        raise ValueError(f"reveal must be one of {EVALUATION_REVEALS}, got {reveal!r}")
    return reveal


NORMS = ("batch", "group", "folded")
GN_GROUPS = 32      # GroupNorm(32, C) at every norm site: the network train.py builds for differentially_private = yes
# the wide-range GroupNorm (SecureContext.group_norm(wide=True)); fixed from tools/secure_gn_range.py's output
GN_WIDE_SCALE = 10 ** 6     # scale of the variance and of v^-1/2, whatever the network's fixed-point scale
GN_WIDE_X0 = 10 ** 4        # the public first guess 0.01 at that scale: serves 0 < v < 3 / 0.01^2
GN_WIDE_STEPS = 32          # iterates, the locally formed first one included
GN_WIDE_FLOOR = 2           # units of 1 / GN_WIDE_SCALE added to var + eps
GN_WIDE_PF = (3, 6)
BN_EPS = 1e-5       # nn.BatchNorm2d's eps, which the plaintext model adds to running_var (the reference's encrypted form does not)


def norm_of(keys, norm=None):
    """The normalisation a state dict / architecture holds: "folded" when it has bn1.scale (a BatchNorm network after
    `fold_batch_norm`), "group" when it has no running statistics (the BatchNorm-free network of differentially private
    training), else "batch".  An explicit `norm` is checked against the keys."""
    found = "folded" if "bn1.scale" in keys else "batch" if "bn1.running_mean" in keys else "group"
    if norm is None:
        return found
    if norm not in NORMS:
        raise ValueError(f"norm must be one of {NORMS} or None, got {norm!r}")
    if norm != found:
        raise ValueError(f"norm={norm!r}, but the state dict holds a {found}-norm network (bn1.scale is "
                         f"{'present' if found == 'folded' else 'absent'}, bn1.running_mean is "
                         f"{'present' if found == 'batch' else 'absent'})")
    return norm


_BN_TENSORS = (".weight", ".bias", ".running_mean", ".running_var", ".num_batches_tracked")


def _foldable_prefixes(keys):
    """The norm prefixes of a BatchNorm state dict / architecture (`_norm_prefixes`, read off the keys: every site has a
    running_var), after the refusals folding makes on the keys alone."""
    if any(k.endswith(".scale") or k.endswith(".shift") for k in keys):
        raise ValueError("the state dict is already folded (it holds <norm>.scale / <norm>.shift)")
    prefixes = [k[:-len(".running_var")] for k in keys if k.endswith(".running_var")]
    if not prefixes:
        raise ValueError("folding needs BatchNorm statistics: this state dict has no running_mean / running_var (a GroupNorm "
                         "network's statistics depend on the image and cannot be folded)")
    return prefixes


def _fold_keys(items, prefixes, scale_of, shift_of):
    """The folded mapping in the unfolded one's order: <prefix>.weight becomes <prefix>.scale, <prefix>.bias becomes
    <prefix>.shift, the statistics drop out, everything else passes through."""
    norm_keys = {p + s: (p, s) for p in prefixes for s in _BN_TENSORS}
    out = {}
    for k, v in items:
        if k not in norm_keys:
            out[k] = v
            continue
        p, s = norm_keys[k]
        if s == ".weight":
            out[p + ".scale"] = scale_of(p)
        elif s == ".bias":
            out[p + ".shift"] = shift_of(p)
    return out


def fold_batch_norm(state_dict, eps=BN_EPS):
    """The model owner's fold of every eval-mode BatchNorm into one per-channel affine map, BEFORE sharing: the statistics
    are its own plaintext, so scale = gamma / sqrt(running_var + eps) and shift = beta - running_mean * scale are computed
    exactly (in float64 from the checkpoint's float32 values, stored as float32) and shared as <prefix>.scale /
    <prefix>.shift in place of the five BatchNorm tensors; conv and fc tensors pass through untouched.  A SecureResNet18 on
    the result evaluates every norm site as `SecureContext.affine_eval`: it follows F.batch_norm(..., training=False)
    for any statistics, where the reference's form (no eps, Newton's iteration on shares of running_var) is accurate only
    for variances in about [0.05, 16].  Refused (ValueError): a dict without running statistics, a dict that is already
    folded, a negative or non-finite variance."""
    prefixes = _foldable_prefixes(state_dict.keys())
    scale, shift = {}, {}
    for p in prefixes:
        var = state_dict[p + ".running_var"].detach().double()
        if not bool(torch.isfinite(var).all()) or bool((var < 0).any()):
            raise ValueError(f"{p}.running_var holds a negative or non-finite variance")
        s = state_dict[p + ".weight"].detach().double() / torch.sqrt(var + float(eps))
        t = state_dict[p + ".bias"].detach().double() - state_dict[p + ".running_mean"].detach().double() * s
        if not bool(torch.isfinite(s).all() and torch.isfinite(t).all()):
            raise ValueError(f"{p}: the folded scale / shift is not finite (running_var + eps = 0, or a non-finite tensor)")
        scale[p], shift[p] = s.float(), t.float()
    return _fold_keys(state_dict.items(), prefixes, scale.__getitem__, shift.__getitem__)


def folded_architecture(arch):
    """`fold_batch_norm` on a name -> shape map (`architecture_of`): all the data owner and the crypto provider of a
    three-role run, who never see the weights, need to follow a folded model."""
    prefixes = _foldable_prefixes(arch.keys())
    shape = lambda p: tuple(arch[p + ".running_var"])
    return _fold_keys(arch.items(), prefixes, shape, shape)


def check_wide_norm(base, pf, norm="group"):
    """The wide-range GroupNorm is a form of the GroupNorm network at 3 <= precision_fractional <= 6, base 10: refuse the rest.
    base = pf = None (a request list, which does not depend on the precision): the norm part alone."""
    if norm != "group":
        raise ValueError(f"wide_norm is a form of the secret-shared GroupNorm, and this is a {norm}-norm network: a BatchNorm "
                         f"checkpoint is served for any running variance by folding its statistics (fold_batch_norm, "
                         f"inference.py --fold_norm)")
    if (base, pf) != (None, None) and (base != 10 or not GN_WIDE_PF[0] <= pf <= GN_WIDE_PF[1]):
        raise ValueError(f"wide_norm is defined for base 10 and {GN_WIDE_PF[0]} <= precision_fractional <= {GN_WIDE_PF[1]} (below, "
                         f"the squares are coarser than the iteration's scale 10^-6; above, the products do not fit the "
                         f"ring), got base {base}, precision_fractional {pf}")


def check_faithful_trunc(norm):
    """The faithful truncation covers the three product sites of a FOLDED network (conv2d, affine_eval, linear): refuse the
    networks whose norm sites truncate products of their own."""
    if norm != "folded":
        raise ValueError(f"faithful_trunc covers the products of a folded network (conv2d, affine_eval, linear), and this is a "
                         f"{norm}-norm network, whose Newton iteration truncates per share about a million small products per "
                         f"pass that the flag would leave as they are: "
                         + ("fold the BatchNorm statistics first (fold_batch_norm, inference.py --fold_norm)" if norm == "batch"
                            else "a GroupNorm network's statistics depend on the image and cannot be folded"))


@dataclasses.dataclass(frozen=True)
class ProtocolForm:
    """The options of an encrypted inference the three roles must agree on beyond the architecture, the input size, the blocks
    and the batch -- public, like the request schedule they select.  Every entry point takes one as `form=`, or its fields as
    keywords (`of`); construction validates the values, `check` makes the refusals that depend on the network.
    pooling: the stem pool the checkpoint was trained with (train.py's pooling_type).  "max" is the reference's stem, swap
    included (conv1 -> bn1 -> MAXPOOL -> RELU).  That swap is an identity for a max pool only (relu(avg(x)) != avg(relu(x))), so
    "avg" keeps the order the network was trained with, conv1 -> bn1 -> RELU -> AvgPool2d(3, 2, 1), with zero padding and the
    divisor 9 for every window: it decodes to the model the checkpoint holds.  This stem is NOT pinned against the reference
    (whose behaviour for this case has not been checked); it follows the plaintext model.  It requests one ReLU at conv1's
    output resolution and a party-local average pool that requests nothing (2,308,096 comparisons and 294 element-wise triples
    per 224 x 224 image, against 3,311,616 and 298 with the max tree).
    reveal: what a pass opens.  "logits" (the default) is the reference's behaviour, unchanged down to the dealer's request
    list, which is a strict prefix of the class form's.
    "class" ends the pass with `SecureContext.argmax` on the logit shares (its requests follow the fc triple) and opens the
    class indices alone, to the data owner: the logits, the model owner's asset, are never reconstructed.  Graphed: the tail is
    part of the captured graph and the static output is the int64 [batch] buffer of class indices.  Three roles: party 0 sends
    its share of the indices to party 1, which returns one int64 [<= batch] tensor per pass; party 0 learns nothing and returns
    None, like the dealer, which follows the extended schedule.
    "confusion" scores the model on labelled images: `begin()`, then passes with the data owner's labels, each ending with
    `SecureContext.confusion` (its requests follow the argmax tail's: the class form's list is a strict prefix) and returning
    nothing, then `finish()`, which opens the confusion matrix -- to both parties -- and nothing else: no logit, no class, no
    label.  Graphed: the tail is captured too; the one-hot labels are a static int64 [batch, classes] buffer next to the images
    (`load` zero-fills the rows of padding images), the shares of the matrix a static buffer the captured pass adds into.  Three
    roles: party 1 also passes `labels`, int64 [n_images]; both parties return the matrix, the dealer None.
    "metrics" is that evaluation with the reference's third overall figure, the one-vs-one ROC AUC: the passes are the
    confusion passes, requests included, and keep their logit and label shares; `finish()` runs `SecureContext.auc_counts` over
    every row held (once, after the last pass: auc_requests) and opens the matrix and the rank counts U [C, C, C] -- `(M, U)`,
    to both parties -- and nothing per image; `torchlib_compat.auc_from_rank_counts(U, M.sum(1))` is the score.  Graphed: the
    captured pass leaves copies of its logit and label shares in buffers of the graph, copied out after each replay; the tail
    runs eagerly on a dealer of its own, seeded apart under a debug seed.  Three roles: after the last pass the dealer serves
    auc_requests(passes * batch, classes), the parties run the tail and both return (M, U).
    fss_bits: the width of the comparisons (see FSS_BITS), the dealer's.  A request list does not depend on it (image_requests
    ignores it); wider keys count in serving_bytes and in the serving form's refusal of a batch that does not fit.
    SecureResNet18 takes the width from its context's dealer, not from here.
    wide_norm (GroupNorm only): every norm site is `group_norm(wide=True)`, right for any group variance in (0, 30,000) at 3 <=
    precision_fractional <= 6; refused for a BatchNorm or folded network (fold_batch_norm is the remedy there).  The site's
    iteration is `rsqrt_newton`'s, GN_WIDE_STEPS - 1 steps of three triples and a mask with no leading mask: 128 requests per
    site against 321.  Three roles: the parties run its step-by-step chain.
    faithful_trunc (folded only): the products of conv2d, affine_eval and linear are truncated by `SecureContext.trunc_faithful`
    (SecureResNet18 sets its context's flag), each site requesting the carry triple ("mul", shape, shape) right after its
    product triple, shape that of the product; the Newton norms of the other networks truncate per share and are refused.  Three
    roles: the parties run the chain (two more opens per site)."""
    pooling: str = "max"
    reveal: str = "logits"
    fss_bits: int = FSS_BITS
    wide_norm: bool = False
    faithful_trunc: bool = False

    def __post_init__(self):
        for name, checked in (("pooling", _check_pooling), ("reveal", _check_reveal), ("fss_bits", check_fss_bits),
                              ("wide_norm", bool), ("faithful_trunc", bool)):
            object.__setattr__(self, name, checked(getattr(self, name)))

    @classmethod
    def of(cls, form=None, **options):
        """`form` itself, or the form the options spell; both at once, or an unknown option, is a TypeError."""
        if form is not None and options:
            raise TypeError(f"pass form= or the options {sorted(options)}, not both")
        return cls(**options) if form is None else form

    def check(self, norm, base=None, pf=None):
        """The refusals that depend on the network (`norm_of`) and, where a context is built (`base`, `pf`), on its precision."""
        if self.wide_norm:
            check_wide_norm(base, pf, norm)
        if self.faithful_trunc:
            check_faithful_trunc(norm)


def expected_wraps(state_dict, images, pf, base=10, blocks=None, pooling="max"):
    """What the reference's per-share truncation is expected to get wrong on these images: the float64 plaintext forward of
    a BatchNorm or folded state dict (folded here when it is not), which at each of the three kinds of product site of the
    folded network takes the pre-truncation values z = product * scale^2 and sums |z| / 2^64 -- the probability, over the
    mask, that the signed shares of z wrap and the sum of the per-share quotients is off by 2^64 / scale.
    -> {"conv2d": sum, "affine_eval": sum, "linear": sum, "total": their sum, "max_ratio": the largest |z| / 2^62}: the
    faithful form's precondition is max_ratio < 1.  Host only, no device."""
    import torch.nn.functional as F

    sd = dict(state_dict)
    if norm_of(sd.keys()) == "batch":
        sd = fold_batch_norm(sd)
    check_faithful_trunc(norm_of(sd.keys()))
    _check_pooling(pooling)
    blocks = _default_blocks() if blocks is None else blocks
    s2 = float(base ** pf) ** 2
    sums = {"conv2d": 0.0, "affine_eval": 0.0, "linear": 0.0}
    peak = [0.0]

    def site(kind, product):
        z = product.abs() * s2
        sums[kind] += float(z.sum()) / 2.0 ** 64
        peak[0] = max(peak[0], float(z.max()) / 2.0 ** 62)
        return product

    p = {k: v.detach().double().cpu() for k, v in sd.items()}
    conv = lambda x, name, stride, pad: site("conv2d", F.conv2d(x, p[name + ".weight"], None, stride, pad))
    bn = lambda x, name: site("affine_eval", x * p[name + ".scale"].view(1, -1, 1, 1)) + p[name + ".shift"].view(1, -1, 1, 1)
    with torch.no_grad():
        x = bn(conv(images.detach().double().cpu(), "conv1", 2, 3), "bn1")
        x = torch.relu(F.max_pool2d(x, 3, 2, 1)) if pooling == "max" else F.avg_pool2d(torch.relu(x), 3, 2, 1)
        for prefix, stride in blocks:
            identity = x
            out = torch.relu(bn(conv(x, prefix + ".conv1", stride, 1), prefix + ".bn1"))
            out = bn(conv(out, prefix + ".conv2", 1, 1), prefix + ".bn2")
            if (prefix + ".downsample.0.weight") in p:
                identity = bn(conv(x, prefix + ".downsample.0", stride, 0), prefix + ".downsample.1")
            x = torch.relu(out + identity)
        x = F.avg_pool2d(x, x.shape[-1]).reshape(x.shape[0], -1)
        site("linear", x @ p["fc.weight"].t())
    return dict(sums, total=sum(sums.values()), max_ratio=peak[0])


def _eps_q(base, pf):
    """GroupNorm's eps = 1e-5 in fixed point, as fix_precision encodes it (precision.py:117-132: a float32 product,
    truncated): 0 below five fractional digits."""
    up = torch.tensor(1e-5, dtype=torch.float32) * torch.tensor(float(base ** pf), dtype=torch.float32)
    return int(up.double().trunc().item())


def _norm_prefixes(keys, blocks):
    out = ["bn1"]
    for prefix, _ in blocks:
        out += [prefix + ".bn1", prefix + ".bn2"]
        if (prefix + ".downsample.0.weight") in keys:
            out.append(prefix + ".downsample.1")
    return out


def share_order(keys):
    """model.fix_precision().share() walks `parameters()` and then `buffers()` (hook.py:624-632,738-765)."""
    keys = [k for k in keys if not k.endswith("num_batches_tracked")]
    buf = [k for k in keys if k.endswith("running_mean") or k.endswith("running_var")]
    return [k for k in keys if k not in buf] + buf


class _FormFields:
    """The fields of `self.form`, readable on the object that holds it."""
    pooling = property(lambda self: self.form.pooling)
    reveal = property(lambda self: self.form.reveal)
    wide_norm = property(lambda self: self.form.wide_norm)
    faithful_trunc = property(lambda self: self.form.faithful_trunc)


class SecureResNet18(_FormFields):
    """ResNet-18 forward on secret shares — `model.fix_precision().share()` followed by
    `model(data)` in inference.py:279-321, including the stem swap `model.pool, model.relu =
    model.relu, model.pool` (:289): conv1 -> bn1 -> MAXPOOL -> RELU.

    norm="group" serves the BatchNorm-free network of differentially private training (GroupNorm(32, C) at every norm
    site, no running statistics in the state dict): every norm site is `SecureContext.group_norm`, whose statistics depend
    on the image -- one Beaver square and one 80-step Newton iteration on B * 32 values per layer, online.  Like the avg
    stem it is NOT pinned against the reference, which has no such layer; it follows the plaintext model.

    norm="folded" serves a BatchNorm checkpoint after the model owner's `fold_batch_norm` (<norm>.scale / <norm>.shift in
    place of the BatchNorm tensors, shared in `share_order` as parameters; no buffers): every norm site is
    `SecureContext.affine_eval`, one Beaver product -- no Newton iteration, hoisted or not, and no `precompute_inv`.  NOT
    pinned against the reference either: it follows the plaintext model (F.batch_norm in eval mode, eps included) for any
    running statistics, where the reference's form is accurate only for variances in about [0.05, 16]."""

    def __init__(self, ctx: SecureContext, state_dict, input_size=224, blocks=None, batched_newton=True, *, norm=None,
                 form=None, **options):
        """batched_newton=False consumes the provider's primitives in exactly the reference's order (newton(running_var)
        inside every batch_norm call, nn/functional.py:62-69) — the mode the reference-minted fixtures pin; the
        default hoists the image-independent iterations of all BatchNorm layers into one batched vector.  (Ignored with
        GroupNorm: nothing there is image independent; and with a folded dict: there is no iteration.)
        norm=None: "folded" when the state dict has bn1.scale, "group" when it has no bn1.running_mean, else "batch"; an
        explicit value must agree.
        `form` or its fields by keyword: `ProtocolForm` (the width is the context's dealer's; a faithful context makes it faithful)."""
        form = ProtocolForm.of(form, **options)
        self.ctx = ctx
        self.input_size = input_size
        self.batched_newton = batched_newton
        self.norm = norm_of(state_dict.keys(), norm)
        self.blocks = blocks if blocks is not None else _default_blocks()
        self.form = dataclasses.replace(form, faithful_trunc=True) if ctx.faithful_trunc else form
        self.form.check(self.norm, ctx.base, ctx.pf)
        ctx.faithful_trunc = self.form.faithful_trunc
        if self.norm == "group":
            for n in _norm_prefixes(state_dict.keys(), self.blocks):
                c = int(state_dict[n + ".weight"].shape[0])
                if c % GN_GROUPS != 0:
                    raise ValueError(f"{n}: {c} channels do not divide into {GN_GROUPS} groups")
        dev = ctx.dealer.device
        self.p = {}
        ctx.invalidate_weight_cache()      # (a model shared on this context before: its transposed shares go with it)
        # hook.py:624-632,738-765: every parameter is encoded and shared, THEN every buffer (`parameters()` before
        # `buffers()`); the 0-dim num_batches_tracked buffers draw no randomness (generate_shares sizes its random
        # share with LongTensor(torch.Size([])) = an empty tensor, additive_shared.py:352) and are never read.
        for k in share_order(state_dict.keys()):
            v = state_dict[k]
            if ctx.party in (None, 0):  # the model owner is party 0 (inference.py:279-283)
                self.p[k] = ctx.share(ctx.encode(v.to(dev)), owner=0)
            else:
                self.p[k] = ctx.share(None, owner=0, shape=v.shape)
        self.acc = self.U = self.kept = None
        if self.reveal in ACCUMULATING:
            self.classes = C = int(state_dict["fc.weight"].shape[0])
            self.acc = ctx._each(lambda j: torch.zeros(C, C, dtype=I64).to(dev))
        if self.reveal == METRICS:
            self.U = ctx._each(lambda j: torch.zeros(C, C, C, dtype=I64).to(dev))
            self.kept = []      # per pass: (logit shares, one-hot label shares) [B, classes], padding rows included

    def begin(self):
        """Start an evaluation: the shares of the confusion matrix are zeroed (reveal="metrics": those of the rank counts
        too, and the rows kept from earlier passes are dropped)."""
        if self.reveal not in ACCUMULATING:
            raise ValueError('begin() belongs to reveal="confusion" and "metrics"')
        for j in self.ctx.parties:
            self.acc[j].zero_()
            if self.U is not None:
                self.U[j].zero_()
        if self.kept is not None:
            self.kept = []

    def held_rows(self):
        """reveal="metrics": (L, Y), the logit and one-hot label shares [N, classes] of every row since begin(), all passes
        side by side (by the library's own copy)."""
        c = self.ctx
        if not self.kept:
            raise ValueError('reveal="metrics": no pass since begin()')
        total = sum(c._ref(l).shape[0] for l, _ in self.kept)

        def cat(which):
            def one(j):
                out = torch.empty(total, self.classes, dtype=I64, device=self.kept[0][which][j].device)
                off = 0
                for entry in self.kept:
                    v = entry[which][j]
                    call("primia_ring_scale", v, 1, out[off:off + v.shape[0]], v.numel())
                    off += v.shape[0]
                return out

            return c._each(one)

        return cat(0), cat(1)

    def finish(self, ctx=None, block_rows=None):
        """End an evaluation: open the confusion matrix -- int64 [classes, classes], row = label, column = predicted class --
        through the context's opener, which hands it to both parties.
        reveal="metrics": first the rank-count tail over every row held (`SecureContext.auc_counts`, on `ctx` when the
        passes ran on a context whose dealer cannot serve it: the graphed form's), then the matrix AND the counts are
        opened, nothing else: -> (M, U), U int64 [classes, classes, classes] (torchlib_compat.auc_from_rank_counts)."""
        if self.reveal not in ACCUMULATING:
            raise ValueError('finish() belongs to reveal="confusion" and "metrics"')
        if self.reveal == CONFUSION:
            return self.ctx.reconstruct(self.acc)
        c = self.ctx if ctx is None else ctx
        L, Y = self.held_rows()
        c.auc_counts(L, Y, self.U, block_rows)
        return c.auc_open(self.acc, self.U)

    def onehot(self, labels, batch):
        """int64 labels [n <= batch] -> raw int64 one-hot [batch, classes] on the device, the rows past n all zero (padding
        images count nowhere); formed on the host and uploaded.  A [batch, classes] tensor is taken as the one-hot itself."""
        dev = self.ctx.dealer.device
        if labels.dim() == 2:
            return labels
        lab = labels.detach().to("cpu", I64).reshape(-1)
        if lab.numel() > batch or (lab.numel() and not (0 <= int(lab.min()) and int(lab.max()) < self.classes)):
            raise ValueError(f"labels: at most {batch} values in [0, {self.classes}), got {lab.tolist()}")
        y = torch.zeros(batch, self.classes, dtype=I64)
        y[torch.arange(lab.numel()), lab] = 1
        return y.to(dev)

    def bn_prefixes(self):
        return _norm_prefixes(self.p, self.blocks)

    def precompute_inv(self):
        """newton(running_var) of every BatchNorm layer in ONE batched 80-step iteration.

        The reference recomputes it layer by layer inside each forward (nn/functional.py:62-69);
        it does not depend on the image, and the iteration is element-wise, so running all layers'
        channels as one vector performs exactly the same arithmetic per channel — it only turns
        20 x 80 x 3 tiny Beaver rounds into 80 x 3 (the per-element randomness is whatever slice of
        the batched triple that channel receives)."""
        c = self.ctx
        names = self.bn_prefixes()
        var = self._var_cat()
        inv = c.reciprocal_newton(var)
        out, off = {}, 0
        for n in names:
            k = c._ref(self.p[n + ".running_var"]).numel()
            out[n] = c._each(lambda j: inv[j][off:off + k].contiguous())
            off += k
        return out

    def _var_cat(self):
        """Every BatchNorm layer's running_var shares side by side (static per model: formed once, by the library's own copy —
        a ring scale by 1 — not by torch.cat)."""
        if getattr(self, "_var_cat_cache", None) is None:
            c, names = self.ctx, self.bn_prefixes()
            total = sum(c._ref(self.p[n + ".running_var"]).numel() for n in names)

            def one(j):
                out = torch.empty(total, dtype=I64, device=self.p[names[0] + ".running_var"][j].device)
                off = 0
                for n in names:
                    v = self.p[n + ".running_var"][j]
                    call("primia_ring_scale", v, 1, out[off:off + v.numel()], v.numel())
                    off += v.numel()
                return out

            self._var_cat_cache = c._each(one)
        return self._var_cat_cache

    def _bn(self, x, prefix):
        p = self.p
        if self.norm == "group":
            return self.ctx.group_norm(x, p[prefix + ".weight"], p[prefix + ".bias"], GN_GROUPS, wide=self.wide_norm)
        if self.norm == "folded":
            return self.ctx.affine_eval(x, p[prefix + ".scale"], p[prefix + ".shift"])
        return self.ctx.batch_norm_eval(x, p[prefix + ".running_mean"], p[prefix + ".running_var"],
                                        p[prefix + ".weight"], p[prefix + ".bias"], inv=self._inv[prefix])

    def forward_shares(self, x):
        c, p = self.ctx, self.p
        if self.norm == "batch":
            self._inv = self.precompute_inv() if self.batched_newton else {n: None for n in self.bn_prefixes()}
        x = c.conv2d(x, p["conv1.weight"], 2, 3)
        x = self._bn(x, "bn1")
        if self.pooling == "max":
            x = c.max_pool2d_3x3s2(x)      # swapped stem (inference.py:289)
            x = c.relu(x)
        else:
            x = c.avg_pool2d_3x3s2(c.relu(x))      # the plaintext order: the swap is an identity for a max pool only
        for prefix, stride in self.blocks:
            identity = x
            out = c.conv2d(x, p[prefix + ".conv1.weight"], stride, 1)
            out = c.relu(self._bn(out, prefix + ".bn1"))
            out = c.conv2d(out, p[prefix + ".conv2.weight"], 1, 1)
            out = self._bn(out, prefix + ".bn2")
            if (prefix + ".downsample.0.weight") in p:
                identity = c.conv2d(x, p[prefix + ".downsample.0.weight"], stride, 0)
                identity = self._bn(identity, prefix + ".downsample.1")
            x = c.relu(c.add(out, identity))
        k = c._ref(x).shape[-1]
        x = c.avg_pool2d(x, k)
        B = c._ref(x).shape[0]
        x = [None if t is None else t.reshape(B, -1) for t in x]
        return c.linear(x, p["fc.weight"], p["fc.bias"])

    def __call__(self, image, batch=1, labels=None):
        """image: fp32 [B, C, S, S] on the GPU -> decoded fp32 logits [B, classes]: the B images go through ONE protocol
        pass.  The data owner is party 1 (inference.py:292-300); in a distributed run party 0 passes image = None and
        `batch`, the number of images it is to expect (it receives shares, never an image).
        reveal="class": -> int64 [B] class indices, the only value the pass reconstructs; in a distributed run party 0 sends
        its share of them to party 1, which returns the classes, and returns None itself.
        reveal="confusion": `labels` are the data owner's int64 labels [n <= B] of the first n images (the rest are padding and
        count nowhere); party 0 passes none.  The pass adds into the shared confusion matrix and returns None.
        reveal="metrics": the confusion pass, requests included; its logit and label shares are kept for `finish()`."""
        c = self.ctx
        if c.party in (None, 1):
            xs = c.share(c.encode(image), owner=1)
        else:
            cin = c._ref(self.p["conv1.weight"]).shape[1]        # 3 (pretrained) or 1 (train.py:262)
            xs = c.share(None, owner=1, shape=(int(batch), cin, self.input_size, self.input_size))
        out = self.forward_shares(xs)
        if self.reveal in ACCUMULATING:
            y = None
            if c.party in (None, 1):
                if labels is None:
                    raise ValueError(f'reveal="{self.reveal}": the data owner passes the labels of the images')
                y = self.onehot(labels, c._ref(out).shape[0])
            c.confusion(out, y, self.acc, kept=self.kept)
            return None
        if self.reveal == "class":
            return c.open_to(c.argmax(out), to=1)
        return c.decode(c.reconstruct(out))


def _default_blocks():
    return [(f"layer{li}.{bi}", (2 if (li > 1 and bi == 0) else 1)) for li in range(1, 5) for bi in range(2)]


def model_requests(arch):
    """The masks sharing a model of architecture `arch` (name -> shape) requests, one per shared tensor in share_order, in the
    form `Dealer.requests` records them: what constructing a SecureResNet18 asks for (tests hold the two equal)."""
    return [("const_mask", tuple(arch[k]), {"owner": 0}) for k in share_order(arch)]


def argmax_requests(batch, classes):
    """What `SecureContext.argmax` on [batch, classes] logits requests: the mask of the first index, then per class walked
    the comparison keys, the mask of the class's index and the ("mul", (B, 2), (B, 2)) triple of the select."""
    B = int(batch)
    mask = ("const_mask", (B,), {"owner": None})
    return [mask] + (int(classes) - 1) * [("dif_keys", (B,), {}), mask, ("triple", ("mul", (B, 2), (B, 2)), {})]


def confusion_requests(batch, classes):
    """What the tail of `SecureContext.confusion` requests after the argmax walk on [batch, classes] logits: the mask of the
    data owner's one-hot labels, the mask of the re-shared class indices, the keys of batch * classes equality tests and the
    triple of the [C, B] x [B, C] product."""
    B, C = int(batch), int(classes)
    return [("const_mask", (B, C), {"owner": 1}), ("const_mask", (B, C), {"owner": None}), ("dpf_keys", (B * C,), {}),
            ("triple", ("matmul", (C, B), (B, C)), {})]


def auc_requests(rows, classes, block_rows=None):
    """What `SecureContext.auc_counts` requests over `rows` rows (all passes, padding rows included): the argmax walk on
    the negated logits, then per block of rows the two K = 1 product triples, the keys of R * C * N comparisons at 64 bits,
    and the triples of the two counting products."""
    N, C = int(rows), int(classes)
    Rb = auc_block_rows(N, C) if block_rows is None else int(block_rows)
    req = argmax_requests(N, C)
    for r0 in range(0, N, Rb):
        R = min(Rb, N - r0)
        req += [("triple", ("matmul", (R * C, 1), (1, N)), {}), ("triple", ("matmul", (R, 1), (1, C * N)), {}),
                ("dif_keys", (R * C * N,), {"bits": AUC_BITS}), ("triple", ("matmul", (R * C, N), (N, C)), {}),
                ("triple", ("matmul", (C, R), (R, C * C)), {})]
    return req


def image_requests(arch, input_size, batch=1, blocks=None, pooling=..., *, form=None, **options):
    """The primitives ONE protocol pass over `batch` images requests from the crypto provider, in order and in the form
    `Dealer.requests` records them — derived on the host from the architecture (name -> shape) alone, without a device:
    what `SecureResNet18.__call__` asks for (tests hold the two equal), so that the memory a serving form needs is known
    BEFORE anything is allocated.  Per batch, not per image: the 80-step Newton reciprocal (237 triples over all BatchNorm
    channels) and the weight side of every matmul triple; per image: everything with a row of its own.
    An architecture without running statistics is the GroupNorm network: no hoisted Newton; every norm site requests its
    square triple, the mask of eps, a Newton iteration on batch * 32 values and the two product triples.
    A folded architecture (`folded_architecture`, bn1.scale among its names): no Newton at all; every norm site requests the
    single triple ("mul", (B*h*h, c), (c,)) of `SecureContext.affine_eval`.
    `form` or its fields by keyword: `ProtocolForm`, which says what each option requests; the width is ignored.  (`pooling`
    alone is still taken as fifth positional argument too, here and in the two functions below: existing callers pass it so.)"""
    form = ProtocolForm.of(form, **(options if pooling is ... else {"pooling": pooling, **options}))
    B, req = int(batch), []
    blocks = _default_blocks() if blocks is None else blocks
    triple = lambda op, xs, ys: req.append(("triple", (op, tuple(xs), tuple(ys)), {}))
    mask = lambda shape, owner: req.append(("const_mask", tuple(shape), {"owner": owner}))
    out_hw = lambda h, k, stride, pad: (h + 2 * pad - k) // stride + 1
    cin = arch["conv1.weight"][1]
    mask((B, cin, input_size, input_size), 1)                                  # the images, shared by the data owner
    norm = norm_of(arch)
    group = norm == "group"
    form.check(norm)
    carry = lambda *shape: triple("mul", shape, shape) if form.faithful_trunc else None
    names = _norm_prefixes(arch, blocks)

    def newton(n, wide=False):
        if not wide:
            mask((1,), None)
        for _ in range(GN_WIDE_STEPS - 1 if wide else 79):
            triple("mul", (n,), (n,))
            triple("mul", (n,), (n,))
            mask((1,), None)
            triple("mul", (n,), (n,))

    if norm == "batch":
        newton(sum(arch[n + ".running_var"][0] for n in names))                # reciprocal_newton of all layers at once

    def conv(name, h, stride, pad):
        o, c, r, _ = arch[name + ".weight"]
        ho = out_hw(h, r, stride, pad)
        triple("matmul", (B, ho * ho, c * r * r), (c * r * r, o))
        carry(B, ho * ho, o)
        return o, ho

    def bn(c, h):
        if group:                                                              # SecureContext.group_norm, per layer
            if c % GN_GROUPS != 0:
                raise ValueError(f"{c} channels do not divide into {GN_GROUPS} groups")
            R, m = B * GN_GROUPS, (c // GN_GROUPS) * h * h
            triple("mul", (R, m), (R, m))
            mask((1,), None)                                                   # + eps (wide: + eps + floor)
            newton(R, form.wide_norm)
            triple("mul", (R,), (m, R))
        elif norm == "batch":
            triple("mul", (c,), (B * h * h, c))
        triple("mul", (B * h * h, c), (c,))                                    # (a folded norm: SecureContext.affine_eval's, alone)
        carry(B * h * h, c)

    def relu(c, h):
        req.append(("dif_keys", (B * c * h * h,), {}))
        triple("mul", (B, c, h, h), (B, c, h, h))

    c, h = conv("conv1", input_size, 2, 3)
    bn(c, h)
    if form.pooling == "avg":
        relu(c, h)                                                             # ReLU first, then the pool: no primitives
        h = out_hw(h, 3, 2, 1)
    else:
        h = out_hw(h, 3, 2, 1)
        rows = B * c * h * h
        for length in (4, 2, 1, 1):                                            # the 9-window max tree
            req.append(("dif_keys", (rows * length,), {}))
            triple("mul", (rows, length), (rows, length))
        relu(c, h)
    for prefix, stride in blocks:
        o, ho = conv(prefix + ".conv1", h, stride, 1)
        bn(o, ho)
        relu(o, ho)
        conv(prefix + ".conv2", ho, 1, 1)
        bn(o, ho)
        if (prefix + ".downsample.0.weight") in arch:
            conv(prefix + ".downsample.0", h, stride, 0)
            bn(o, ho)
        relu(o, ho)
        c, h = o, ho
    classes, feat = arch["fc.weight"]
    triple("matmul", (B, feat), (feat, classes))
    carry(B, classes)
    if form.reveal != "logits":
        req += argmax_requests(B, classes)
    if form.reveal in ACCUMULATING:
        req += confusion_requests(B, classes)
    return req


# bytes of one comparison's DIF key as Dealer.dif_keys lays it out: raw alpha, its mask and party 0's share (3 x 8), both
# parties' seeds (2 x 2 x 8), the packed control bits (32), cw_sigma and cw_s (32 x 2 x 8 each), the leaf words (33 x 4) --
# at a width of n bits: n control bytes, n x 2 x 8 twice, n + 1 leaf words: 60 + 37 n
class _DifKeyBytes(int):
    """The bytes at the reference's width, as the number it has always been; called with a width, the bytes at that width."""

    def __call__(self, bits=FSS_BITS):
        bits = check_fss_bits(bits)
        return 3 * 8 + 32 + bits + 2 * bits * 2 * 8 + (bits + 1) * 4


DIF_KEY_BYTES = _DifKeyBytes(3 * 8 + 32 + 32 + 2 * 32 * 2 * 8 + 33 * 4)


def _dpf_key_bytes():
    """Bytes of one equality test's DPF key as Dealer.dpf_keys lays it out: raw alpha, its mask and party 0's share (3 x 8),
    both parties' seeds (2 x 2 x 8) and the correction words at the sizes their field shapes give (32 control bytes,
    32 x 2 x 8 of cw_s, one int64 leaf): 608, whatever the comparison width."""
    cw = sum(int(torch.Size(shape).numel()) * torch.empty(0, dtype=dt).element_size() for shape, dt in dpf_key_fields(1))
    return 3 * 8 + 2 * 2 * 8 + cw


DPF_KEY_BYTES = _dpf_key_bytes()


def primitive_bytes(requests, fss_bits=FSS_BITS):
    """Device bytes of the primitives a request list stands for (both parties' halves), its comparison keys at `fss_bits`
    (a request that names a width of its own, {"bits": n}: at that width)."""
    key_bytes = DIF_KEY_BYTES(fss_bits)
    numel = lambda shape: int(torch.Size(shape).numel())
    total = 0
    for kind, args, kw in requests:
        if kind == "const_mask":
            total += 8 * numel(args)
        elif kind == "dif_keys":
            total += (DIF_KEY_BYTES(kw["bits"]) if "bits" in kw else key_bytes) * args[0]
        elif kind == "dpf_keys":
            total += DPF_KEY_BYTES * args[0]
        else:
            op, xs, ys = args
            total += 16 * (numel(xs) + numel(ys) + numel(_triple_c_shape(op, xs, ys)))
    return total


def serving_bytes(arch, input_size, batch, blocks=None, pooling=..., *, form=None, **options):
    """What GraphedSecureInference(batch=...) holds in static buffers: every primitive of one pass (dominated by the DIF
    keys: 1,244 bytes per comparison, 3,311,616 comparisons per 224 x 224 image, 2,308,096 with pooling="avg") plus one eighth on top for the arena copy of
    their random words while both exist (5/6 of a triple, 48 of a key's 1,244 bytes) and the captured graph's activations
    (im2col and pool-unroll operands: under 2 % of the keys at every layer).  A key of `fss_bits` levels takes 60 + 37 fss_bits
    bytes: 2,428 at 64.  `form` or its fields by keyword: `ProtocolForm`."""
    form = ProtocolForm.of(form, **(options if pooling is ... else {"pooling": pooling, **options}))
    b = primitive_bytes(image_requests(arch, input_size, batch, blocks, form=form), form.fss_bits)
    return b + b // 8


def largest_batch_that_fits(arch, input_size, budget, blocks=None, pooling=..., *, form=None, **options):
    """The largest batch whose static buffers fit in `budget` bytes (0: not even one image).  serving_bytes is affine in the
    batch (a per-batch part, Newton and the weight masks, plus a per-image part) up to its rounding, so two evaluations
    give the answer and the neighbours settle the rounding.  `form` or its fields by keyword: `ProtocolForm`."""
    form = ProtocolForm.of(form, **(options if pooling is ... else {"pooling": pooling, **options}))
    need = lambda k: serving_bytes(arch, input_size, k, blocks, form=form)
    one, two = need(1), need(2)
    per_image, fixed = two - one, 2 * one - two
    k = max(0, (int(budget) - fixed) // per_image)
    while need(k + 1) <= budget:
        k += 1
    while k > 0 and need(k) > budget:
        k -= 1
    return k


class GraphedSecureInference(_FormFields):
    """Serving form of the encrypted forward: the online phase (about 6,500 small launches per image) is
    captured ONCE as a hipGraph over static buffers — the input image and every correlated-randomness
    primitive — and replayed per image; `refill()` has the dealer regenerate all per-image primitives into
    the same buffers (the reference's pre-provisioned crypto store, mpc/primitives.py:161-235, refilled
    between requests).  Results are bit-identical to the eager SecureResNet18 fed the same primitives.

    The refill is ONE graph launch too (round 6).  Every uniformly random word of an image's primitives — triple input
    shares and c0, re-sharing masks, FSS alpha / seeds / alpha masks — lives in ONE int64 arena that the tape entries are
    views of: a single ChaCha20 launch fills it (`primia_chacha20_fill_ctr`: the block counter is a DEVICE word the graph's
    last node advances, so every replay draws fresh keystream — a host counter would be frozen into the graph and every
    image would get the same masks), then one launch per triple forms c1 = a o b - c0 and two per comparison batch form
    the key (alpha split, DIF keygen).  ~3,000 eager launches per image became ~450 graph nodes; `refill_graph = False`
    launches the same calls eagerly (same bits).  The constructor ends with one refill: no image is ever served on the
    primitives the all-zero warm-up image consumed (opened values on a known input reveal the masks).

    `batch` images per protocol pass: the static input buffer, the arena and both captured graphs are for that ONE batch
    size; fewer images (the last ones of a stream) are padded with all-zero images whose rows consume their own primitives
    and are dropped.  The static buffers are sized on the host first (`serving_bytes`) and a batch that does not fit in
    `memory_budget` bytes (default: the device's free memory plus what torch's allocator holds unused) is refused with the
    largest batch that would.
    `form` or its fields by keyword: `ProtocolForm`, which says what each `reveal` captures and holds in static buffers."""

    refill_graph = True
    fss_bits = property(lambda self: self.form.fss_bits)      # (this form's own dealers are built at the form's width)

    def __init__(self, state_dict, device, input_size=224, precision_fractional=16, base=10, seed=None, blocks=None, batch=1,
                 memory_budget=None, *, form=None, **options):
        self.form = form = ProtocolForm.of(form, **options)
        self.device = torch.device(device)
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError("batch must be at least 1")
        arch = architecture_of(state_dict)
        self.static_bytes = serving_bytes(arch, input_size, self.batch, blocks, form=form)
        if memory_budget is None:
            free, _ = torch.cuda.mem_get_info(self.device)
            memory_budget = free + torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        if self.static_bytes > memory_budget:
            fits = largest_batch_that_fits(arch, input_size, memory_budget, blocks, form=form)
            raise ValueError(f"a batch of {self.batch} images at {input_size}x{input_size} needs {self.static_bytes} bytes of static "
                             f"primitives, {int(memory_budget)} are free: the largest batch that fits is {fits}")
        # (all-zero warm-up images, uploaded: no fill kernel of torch's on the path)
        self.image = torch.zeros(self.batch, state_dict["conv1.weight"].shape[1], input_size, input_size, dtype=torch.float32).to(self.device)
        self.labels = None
        if self.reveal in ACCUMULATING:      # (all-zero one-hot rows: the warm-up images are padding)
            self.labels = torch.zeros(self.batch, int(state_dict["fc.weight"].shape[0]), dtype=I64).to(self.device)
        self.dealer = Dealer(self.device, seed, self.fss_bits)
        self.dealer.tape, self.dealer.requests = [], []
        ctx = SecureContext(self.dealer, base, precision_fractional)
        model = SecureResNet18(ctx, state_dict, input_size, blocks, form=form)
        self._n_model = len(self.dealer.tape)          # primitives consumed by sharing the model (kept)
        model(self.image, labels=self.labels)          # offline pass: fills the tape, warms every kernel
        self.tape, self.requests = self.dealer.tape, self.dealer.requests
        self.dealer.tape = self.dealer.requests = None
        self.stats = dict(ctx.stats)
        self._rehome_tape()                            # per-image random words -> one arena (before any pointer is captured)
        pre = PreloadedDealer(self.tape, self.device, self.fss_bits)
        self._ctx = SecureContext(pre, base, precision_fractional)
        self._model = SecureResNet18(self._ctx, state_dict, input_size, blocks, form=form)      # re-shares with the same masks
        self._model(self.image, labels=self.labels)    # eager pass over the static buffers: builds the pointer tables
        pre.pos, self._ctx._newton_calls = self._n_model, 0
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=side):
                self.out = self._model(self.image, labels=self.labels)
        torch.cuda.current_stream().wait_stream(side)
        self._static_rows = self._tail_ctx = None
        if self.reveal == METRICS:
            # the captured pass left its copies of the logit and label shares in buffers of the graph's own: every replay
            # rewrites them, and __call__ copies them out.  The tail runs eagerly after the last pass, on a dealer of its
            # own (this form's dealer draws on the device from here on, inside the refill graph)
            self._static_rows = self._model.kept[-1]
            self._tail_ctx = SecureContext(Dealer(self.device, None if seed is None else seed + 104729, self.fss_bits), base,
                                           precision_fractional)
        # the provider's block counter moves to the device, behind everything the offline pass drew
        self._ctr = torch.tensor([self.dealer._block], dtype=I64).to(self.device)      # (uploaded: no fill kernel)
        self.dealer._block = None                      # (the host counter is dead from here on: rand64 would raise)
        self.refills = 0
        self._refill_launches()                        # eager: warms the dealer kernels AND replaces the warm-up primitives
        self.refills = 1
        self._refill_g = None
        if self.refill_graph:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._refill_g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._refill_g, stream=side):
                    self._refill_launches()
            torch.cuda.current_stream().wait_stream(side)
        if self.reveal in ACCUMULATING:
            self.begin()                               # (the warm-up passes added shares of zero)

    def begin(self):
        """Start an evaluation: zero the static shares of the confusion matrix (reveal="metrics": and of the rank counts, and
        drop the rows kept)."""
        self._model.begin()

    def finish(self, block_rows=None):
        """Open the confusion matrix of the passes since begin(): int64 [classes, classes], row = label.
        reveal="metrics": run the rank-count tail eagerly over the rows the passes left, then open -> (M, U)."""
        if self.reveal == METRICS:
            return self._model.finish(ctx=self._tail_ctx, block_rows=block_rows)
        return self._model.finish()

    def _rehome_tape(self):
        """Move every uniformly random tensor of the per-image primitives into ONE int64 arena (64-byte aligned slices, current
        values kept) and record, per primitive, the launches that complete it after a fill."""
        dev = self.device
        al = lambda n: (n + 7) // 8 * 8
        total, plan = 0, []
        for i in range(self._n_model, len(self.tape)):
            kind, args, _ = self.requests[i]
            e = self.tape[i]
            if kind == "const_mask":
                sizes = [e.numel()]
            elif kind == "triple":
                (a0, b0, c0), (a1, b1, _c1) = e
                sizes = [a0.numel(), a1.numel(), b0.numel(), b1.numel(), c0.numel()]
            elif kind in ("dif_keys", "dpf_keys"):
                sizes = [args[0], 4 * args[0], args[0]]        # raw alpha, both parties' seeds, alpha's mask
            else:
                raise _lib.PrimiaError(f"unknown primitive kind {kind!r}")
            offs = []
            for n in sizes:
                offs.append(total)
                total += al(n)
            plan.append(offs)
        self._arena = torch.empty(max(total, 8), dtype=I64, device=dev)

        def view(off, src=None, shape=None):
            shape = tuple(src.shape) if src is not None else shape
            n = 1
            for d in shape:
                n *= d
            v = self._arena[off:off + n].view(shape)
            if src is not None:
                v.copy_(src)
            return v

        self._ops, max_kn = [], 1
        for i, offs in zip(range(self._n_model, len(self.tape)), plan):
            kind, args, _ = self.requests[i]
            e = self.tape[i]
            if kind == "const_mask":
                self.tape[i] = view(offs[0], e)
            elif kind == "triple":
                op, xshape, yshape = args
                (a0, b0, c0), (a1, b1, c1) = e
                a0, a1, b0, b1, c0 = (view(o, t) for o, t in zip(offs, (a0, a1, b0, b1, c0)))
                self.tape[i] = [(a0, b0, c0), (a1, b1, c1)]
                self._ops.append(("triple", op, xshape, yshape, a0, a1, b0, b1, c0, c1))
                if op != "mul":      # triple_c1's scratch: a = a0 + a1 [B*L, K] and b = b0 + b1 [K, N]
                    max_kn = max(max_kn, a0.numel() + b0.numel())
            else:
                (n,) = args
                k0, k1 = e
                alpha = view(offs[0], shape=(n,))
                s0 = view(offs[1], shape=(2, 2, n))
                s0[0].copy_(k0["s0"])
                s0[1].copy_(k1["s0"])
                r = view(offs[2], k1["alpha"])
                k0["s0"], k1["s0"], k1["alpha"] = s0[0], s0[1], r
                if kind == "dpf_keys":
                    self._ops.append(("dpf", n, alpha, s0, r, k0["alpha"], k0["bits"], k0["cw_s"], k0["cw_n"]))
                    continue
                self._ops.append(("dif", n, alpha, s0, r, k0["alpha"], k0["bits"], k0["cw_sigma"], k0["cw_s"], k0["cw_leaf"]))
        self._mm_scratch = torch.empty(max_kn, dtype=I64, device=dev)

    def _refill_launches(self):
        d = self.dealer
        n = self._arena.numel()
        call("primia_chacha20_fill_ctr", *d._key, d._nonce, self._ctr, 0, self._arena, n)
        for op in self._ops:
            if op[0] == "triple":
                _, kind, xshape, yshape, a0, a1, b0, b1, c0, c1 = op
                d.triple_c1(kind, xshape, yshape, a0, a1, b0, b1, c0, c1, scratch=self._mm_scratch)
            elif op[0] == "dpf":
                _, m, alpha, s0, r, a0, bits, cw_s, cw_n = op
                call("primia_fss_alpha_split", alpha, s0, r, a0, m)
                call("primia_dpf_keygen", alpha, s0, bits, cw_s, cw_n, m)
            else:
                _, m, alpha, s0, r, a0, bits, cw_sigma, cw_s, leaf = op
                fss_call("fss_alpha_split", d.fss_bits, alpha, s0, r, a0, m)
                fss_call("dif_keygen", d.fss_bits, alpha, s0, bits, cw_sigma, cw_s, leaf, m)
        call("primia_u64_add", self._ctr, (n + 7) // 8)

    def refill(self):
        """Fresh per-image primitives from the dealer, written into the captured buffers (on the current stream)."""
        if self._refill_g is not None:
            self._refill_g.replay()
        else:
            self._refill_launches()
        self.refills += 1

    def load(self, image, labels=None):
        """Copy [n <= batch, C, S, S] images into the static input buffer, the rest of it zero; returns n.
        reveal="confusion": `labels`, int64 [n], become the one-hot rows of the static label buffer; the rows of padding images
        are zero-filled."""
        if self.labels is not None:
            if labels is None or labels.numel() != image.shape[0]:
                raise ValueError(f'reveal="{self.reveal}": one label per image')
            self.labels.copy_(self._model.onehot(labels, self.batch))
        if self.batch == 1:
            self.image.copy_(image)
            return 1
        n = image.shape[0]
        if not 1 <= n <= self.batch:
            raise ValueError(f"this form serves 1 to {self.batch} images per pass, got {n}")
        self.image[:n].copy_(image)
        if n < self.batch:
            self.image[n:].zero_()
        return n

    def rows(self, n):
        """The first n rows of the static output (all of it, the very buffer, for a full batch)."""
        if self.out is None:      # reveal="confusion" / "metrics": a pass returns nothing
            return None
        return self.out if n == self.batch else self.out[:n]

    def __call__(self, image, refill=True, labels=None):
        """image [n <= batch, C, S, S] -> logits [n, classes], or with reveal="class" int64 class indices [n] (a view of the
        static output buffer).
        refill=False replays on the primitives the buffers hold (bit-identity checks against an eager forward on the
        same tape; a deployment never serves two images on one set of primitives)."""
        if refill:
            self.refill()
        n = self.load(image, labels)
        self.graph.replay()
        if self._static_rows is not None:
            self._model.kept.append(tuple(self._ctx._copy(t) for t in self._static_rows))
        return self.rows(n)


class PipelinedSecureInference:
    """A stream of encrypted inferences with the crypto provider HIDDEN behind the online phase.

    The reference provisions primitives on demand, serially with the protocol (mpc/fss.py:142-146, primitives.py:161-235).
    Here two `GraphedSecureInference` slots (each its own dealer, static primitive buffers and captured online graph)
    alternate: while image i replays slot i % 2 on the caller's stream, the dealer refills the OTHER slot for image i + 1
    on its own stream — one graph launch of its own (round 6; ~3,000 eager launches before) whose 21 key generations share the
    vector ALUs with the online evaluation.  Events order a slot's refill after the replay that consumed it and the next replay after
    the refill.  Every image's shares are those of an eager SecureResNet18 on the slot's primitives (the graph is
    bit-identical to it, tests/test_gpu_secure.py); nothing about the protocol changes, only who waits for whom.
    In the three-role deployment the same overlap is physical: the dealer rank runs ahead of the parties on its own GPU.
    `form` or its fields by keyword: `ProtocolForm`; every slot is built with the one form."""

    def __init__(self, state_dict, device, input_size=224, precision_fractional=16, base=10, seed=None, blocks=None, slots=2,
                 batch=1, *, form=None, **options):
        self.form = form = ProtocolForm.of(form, **options)
        self.device = torch.device(device)
        if form.reveal in ACCUMULATING:
            raise ValueError(f'reveal="{form.reveal}" accumulates in one set of static buffers: use GraphedSecureInference')
        self.slots = [GraphedSecureInference(state_dict, device, input_size, precision_fractional, base,
                                             None if seed is None else seed + 7919 * k, blocks, batch, form=form)
                      for k in range(slots)]
        self.stats = self.slots[0].stats
        self.dealer_stream = torch.cuda.Stream(device=self.device)
        # event: slot k's primitives are fresh.  None = fresh since construction: GraphedSecureInference ends its constructor
        # with a refill, so the first image of a slot never runs on the primitives the all-zero warm-up image consumed
        assert all(sl.refills >= 1 for sl in self.slots)
        self._ready = [None] * slots
        self._n = 0

    def __call__(self, image):
        """One encrypted pass over [n <= batch] images; returns what SecureResNet18 returns (a copy: the slot's buffers are
        reused)."""
        k = self._n % len(self.slots)
        slot = self.slots[k]
        main = torch.cuda.current_stream()
        if self._ready[k] is not None:
            main.wait_event(self._ready[k])
        n = slot.load(image)
        slot.graph.replay()
        out = slot.rows(n).clone()
        consumed = torch.cuda.Event()
        consumed.record(main)
        # the dealer regenerates this slot's primitives for image n + len(slots) while the next image runs on another slot
        with torch.cuda.stream(self.dealer_stream):
            self.dealer_stream.wait_event(consumed)
            slot.refill()
            ev = torch.cuda.Event()
            ev.record(self.dealer_stream)
        self._ready[k] = ev
        self._n += 1
        return out


# ---- three-role deployment: party 0 (model owner), party 1 (data owner), crypto provider --------------------
# inference.py:262-321 runs the same three roles as websocket workers (configs/websetting/config_inference.csv);
# here each role is one rank of a torch.distributed job — one GPU each over xGMI with the RCCL backend — and the
# only traffic is what the protocol itself exchanges: dealer -> party primitives, owner -> peer fresh shares, and
# the 2-party opens of DistOpener.

DEALER_RANK = 2


class PartyLink:
    """Point-to-point transport between the three roles, expressed as broadcasts inside 2-rank groups so the
    same code runs on RCCL (device buffers over xGMI) and on gloo (tests).  Every rank of the job constructs
    it (group creation is collective)."""

    def __init__(self, device, ranks=(0, 1, 2)):
        import torch.distributed as dist

        self.dist, self.device = dist, torch.device(device)
        self.rank = dist.get_rank()
        p0, p1, d = ranks
        self.ranks, self.dealer_rank = (p0, p1), d
        self.role = {p0: 0, p1: 1, d: "dealer"}[self.rank]
        self.parties_group = dist.new_group([p0, p1])
        self.dealer_groups = [dist.new_group(sorted([p0, d])), dist.new_group(sorted([p1, d]))]
        self.all_group = dist.new_group(sorted(ranks))

    # party <-> party
    def send_to_peer(self, t):
        self.dist.broadcast(t.contiguous(), src=self.rank, group=self.parties_group)

    def recv_from_peer(self, shape, dtype=I64):
        t = torch.empty(tuple(shape), dtype=dtype, device=self.device)
        self.dist.broadcast(t, src=self.ranks[1 - self.role], group=self.parties_group)
        return t

    # dealer -> party (to = 0 / 1) or dealer -> both (to = None)
    def _dealer_group(self, to):
        return self.all_group if to is None else self.dealer_groups[to]

    def dealer_send(self, t, to=None):
        self.dist.broadcast(t.contiguous(), src=self.dealer_rank, group=self._dealer_group(to))

    def from_dealer(self, shape, dtype=I64, private=True):
        t = torch.empty(tuple(shape), dtype=dtype, device=self.device)
        self.dist.broadcast(t, src=self.dealer_rank, group=self._dealer_group(self.role if private else None))
        return t


DPF_CW_NAMES = ("bits", "cw_s", "cw_n")


def _triple_c_shape(op, xshape, yshape):
    if op == "mul":
        nx = int(torch.Size(xshape).numel())
        return tuple(xshape) if nx >= int(torch.Size(yshape).numel()) else tuple(yshape)
    return tuple(xshape[:-1]) + (yshape[-1],)


class PartyDealer:
    """What party j sees of the crypto provider: it receives ITS half of each primitive, in protocol order
    (mpc/primitives.py:161-235 keeps the same per-worker store; here nothing is requested — the provider
    follows the public request schedule of the network, see model_requests and image_requests)."""

    def __init__(self, link: PartyLink, fss_bits=FSS_BITS):
        self.link, self.device, self.j = link, link.device, link.role
        self.fss_bits = check_fss_bits(fss_bits)      # the provider's width: public, like the request schedule
        self.log = None

    def _mine(self, v):
        out = [None, None]
        out[self.j] = v
        return out

    def triple(self, op, xshape, yshape):
        f = self.link.from_dealer
        return self._mine((f(xshape), f(yshape), f(_triple_c_shape(op, xshape, yshape))))

    def dif_keys(self, n, bits=None):
        f = self.link.from_dealer
        k = dict(alpha=f((n,)), s0=f((2, n)))
        w = self.fss_bits if bits is None else check_fss_bits(bits)
        for name, (shape, dt) in zip(("bits", "cw_sigma", "cw_s", "cw_leaf"), dif_key_fields(n, w)):
            k[name] = f(shape, dt, private=False)
        return self._mine(k)

    def dpf_keys(self, n):
        f = self.link.from_dealer
        k = dict(alpha=f((n,)), s0=f((2, n)))
        for name, (shape, dt) in zip(DPF_CW_NAMES, dpf_key_fields(n)):
            k[name] = f(shape, dt, private=False)
        return self._mine(k)

    def const_mask(self, *shape, owner=None):
        return self.link.from_dealer(shape, private=owner is not None)


def architecture_of(state_dict):
    """name -> shape of every shared tensor: all a non-owner needs to know about the model."""
    return {k: tuple(v.shape) for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}


class DealerService:
    """The crypto provider's rank: generate each scheduled primitive on its GPU and ship each half to its
    party (build_triple / build_fss_keys, mpc/beaver.py:7-63, mpc/primitives.py:237-253)."""

    def __init__(self, dealer: Dealer, link: PartyLink):
        self.dealer, self.link = dealer, link

    def serve(self, requests):
        send = self.link.dealer_send
        for kind, args, kw in requests:
            v = getattr(self.dealer, kind)(*args, **kw)
            if kind == "triple":
                for j in range(2):
                    for t in v[j]:
                        send(t, j)
            elif kind == "dif_keys":
                for j in range(2):
                    send(v[j]["alpha"], j)
                    send(v[j]["s0"], j)
                for name in ("bits", "cw_sigma", "cw_s", "cw_leaf"):
                    send(v[0][name], None)
            elif kind == "dpf_keys":      # alpha share and seed private, correction words to both
                for j in range(2):
                    send(v[j]["alpha"], j)
                    send(v[j]["s0"], j)
                for name in DPF_CW_NAMES:
                    send(v[0][name], None)
            else:
                send(v, kw.get("owner"))


def party_context(link: PartyLink, precision_fractional=16, base=10, *, form=None, **options):
    """SecureContext of the party this rank plays, at the width and with the truncation of the `ProtocolForm`."""
    form = ProtocolForm.of(form, **options)
    return SecureContext(PartyDealer(link, form.fss_bits), base, precision_fractional,
                         opener=DistOpener(link.parties_group, link.role), party=link.role, link=link,
                         faithful_trunc=form.faithful_trunc)


def run_three_role(link: PartyLink, arch, input_size, n_images, state_dict=None, images=None, seed=None, blocks=None,
                   precision_fractional=16, base=10, batch=1, *, labels=None, form=None, **options):
    """One rank's part of the three-role encrypted inference of inference.py:279-321.
    Party 0 passes `state_dict`, party 1 passes `images` (fp32 [n,3,S,S] on its GPU), the dealer neither;
    all know the architecture, the input size, the `ProtocolForm` (`form`, or its fields by keyword), how many images will be
    classified and how many go through one protocol pass (`batch`; the last pass is padded with all-zero images, whose rows are
    dropped).  Parties return the list of decoded logits, one [<= batch, classes] tensor per pass (the reference `.get()`s the
    prediction to the orchestrator), the dealer None; what the other `reveal`s return, and who passes `labels`: `ProtocolForm`."""
    form = ProtocolForm.of(form, **options)
    form.check(norm_of(arch), base, precision_fractional)
    passes = (n_images + batch - 1) // batch
    if link.role == "dealer":      # follows the public schedule, derived on the host: this rank runs no layer kernel
        image_req = image_requests(arch, input_size, batch, blocks, form=form)
        svc = DealerService(Dealer(link.device, seed, form.fss_bits), link)
        svc.serve(model_requests(arch))
        for _ in range(passes):
            svc.serve(image_req)
        if form.reveal == METRICS:      # the rank-count tail over every row held, padding rows included
            svc.serve(auc_requests(passes * batch, arch["fc.weight"][0]))
        return None
    ctx = party_context(link, precision_fractional, base, form=form)
    if link.role == 0:
        if state_dict is None:
            raise ValueError("party 0 is the model owner: it needs the state dict")
        shapes = {k: v for k, v in state_dict.items()}
    else:
        if images is None:
            raise ValueError("party 1 is the data owner: it needs the images")
        shapes = {k: torch.empty(shape, device="meta") for k, shape in arch.items()}
    model = SecureResNet18(ctx, shapes, input_size, blocks, form=form)
    if form.reveal in ACCUMULATING:
        if link.role == 1 and (labels is None or labels.numel() != n_images):
            raise ValueError("party 1 is the data owner: it needs one label per image")
        model.begin()
    out = []
    for i in range(0, n_images, batch):
        n = min(batch, n_images - i)
        chunk = None
        if link.role == 1:
            chunk = images[i:i + n]
            if n < batch:
                chunk = torch.cat([chunk, chunk.new_zeros((batch - n,) + tuple(chunk.shape[1:]))])
        res = model(chunk, batch=batch, labels=labels[i:i + n] if form.reveal in ACCUMULATING and link.role == 1 else None)
        if res is not None:
            out.append(res if n == batch else res[:n])
    if form.reveal in ACCUMULATING:
        return model.finish()
    return None if form.reveal == "class" and link.role == 0 else out
