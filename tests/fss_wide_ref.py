"""The DIF comparison at a width of n bits, 32 <= n <= 64, restated from oracle.secure_oracle's own pieces --
prg_H, convert, _sel, radd / rsub -- for tests/test_fss_wide_host.py and the GPU tests of the wide comparison: a module of
helpers, not of tests.  Nothing under oracle/ is changed or patched; at n = 32 every function here returns what the oracle's
32-bit one returns (tests/test_fss_wide_host.py holds them equal).

Definition.  M = 2^n.  The dealer reduces alpha and its mask r mod M; party 0 gets (alpha - r) mod M, party 1 gets r.  The
masked input is x = (r_0 + r_1) mod M with r_j = x1_j - x2_j + alpha_j in Z_2^64.  Keygen and eval are the reference's level
step n times, on bits n-1 .. 0 of alpha and of x, most significant first, with the reference's leaf (convert = low 31 bits of
the last word, cw_leaf cast to int32).  The parties' outputs add up to [(d + alpha) mod M <= alpha] for d = x1 - x2."""
import numpy as np

from oracle import secure_oracle as S

U64, I64 = np.uint64, np.int64


def width_mask(n):
    assert 32 <= n <= 64
    return U64((1 << n) - 1)


def bit_rows(x, n):
    """Bits n-1 .. 0 of x, most significant first: [n, len(x)] of 0 / 1 (uint64)."""
    x = np.asarray(x).astype(U64) & width_mask(n)
    return np.stack([(x >> U64(n - 1 - i)) & U64(1) for i in range(n)])


def split_alpha(alpha, r, n):
    """(alpha - r) mod 2^n for party 0, r mod 2^n for party 1."""
    m = width_mask(n)
    r = np.asarray(r, U64) & m
    return ((np.asarray(alpha, U64) & m) - r) & m, r


def fss_open(r0, r1, n):
    return S.radd(r0, r1).view(U64) & width_mask(n)


def _uncompressed(key_bits, cw_sigma, cw_s, n_el):
    """Both sides of a level's correction word from its compressed parts (fss.py:456-477)."""
    cwi = np.empty((2, 6, n_el), U64)
    for side in range(2):
        cwi[side, 0:2] = cw_sigma
        cwi[side, 2] = key_bits[2 * side]
        cwi[side, 3:5] = cw_s
        cwi[side, 5] = key_bits[2 * side + 1]
    return cwi


def _keygen_serial(alpha, s0_pair, n):
    n_el = alpha.shape[0]
    a_bits = bit_rows(alpha, n)
    s = np.asarray(s0_pair, U64).copy()
    t = np.stack([np.zeros(n_el, U64), np.ones(n_el, U64)])
    bits = np.empty((n, 4, n_el), U64)
    cw_sigma = np.empty((n, 2, n_el), U64)
    cw_s = np.empty((n, 2, n_el), U64)
    cw_leaf = np.empty((n + 1, n_el), I64)
    one = np.ones((1, n_el), U64)
    for i in range(n):
        ai = a_bits[i]
        on = ai.astype(bool)
        h = [S.prg_H(s[0]), S.prg_H(s[1])]
        s_rand = np.where(on, h[0][0, 3:5] ^ h[1][0, 3:5], h[0][1, 3:5] ^ h[1][1, 3:5])
        sg_rand = np.where(on, h[0][0, 0:2] ^ h[1][0, 0:2], h[0][1, 0:2] ^ h[1][1, 0:2])
        tab = np.empty((2, 6, n_el), U64)
        tab[0, 0:3] = ai * np.concatenate([sg_rand, one])
        tab[1, 0:3] = (U64(1) - ai) * np.concatenate([sg_rand, one])
        tab[0, 3:6] = (U64(1) - ai) * np.concatenate([s_rand, one])
        tab[1, 3:6] = ai * np.concatenate([s_rand, one])
        cw = tab ^ h[0] ^ h[1]
        bits[i] = np.stack([cw[0, 2], cw[0, 5], cw[1, 2], cw[1, 5]]) & U64(1)
        cw_sigma[i] = np.where(on, cw[1, 0:2], cw[0, 0:2])
        cw_s[i] = np.where(on, cw[0, 3:5], cw[1, 3:5])
        cwi = _uncompressed(bits[i], cw_sigma[i], cw_s[i], n_el)
        sig, tau = [None, None], [None, None]
        s_next, t_next = np.empty_like(s), np.empty_like(t)
        for b in range(2):
            dual = h[b] ^ (t[b] * cwi)
            state = S._sel(dual, ai)
            s_next[b], t_next[b] = state[3:5], state[5]
            anti = S._sel(dual, U64(1) - ai)
            sig[b], tau[b] = anti[0:2], anti[2]
        sign = np.where(tau[1].astype(bool), I64(-1), I64(1))
        cw_leaf[i] = sign * (I64(1) - S.convert(sig[0]) + S.convert(sig[1]) - (I64(1) - ai.astype(I64)))
        s, t = s_next, t_next
    sign = np.where(t[1].astype(bool), I64(-1), I64(1))
    cw_leaf[n] = sign * (I64(1) - S.convert(s[0]) + S.convert(s[1]))
    return [dict(s0=np.asarray(s0_pair, U64)[b].copy(), bits=bits.astype(np.uint8), cw_sigma=cw_sigma, cw_s=cw_s,
                 cw_leaf=cw_leaf.astype(np.int32)) for b in range(2)]


def _eval_serial(b, x, key, n):
    x_bits = bit_rows(x, n)
    n_el = x_bits.shape[1]
    s = key["s0"].copy()
    t = np.full(n_el, b, U64)
    leaf = key["cw_leaf"].astype(I64)
    sgn = I64(-1) if b else I64(1)
    acc = np.zeros(n_el, U64)
    for i in range(n):
        state = S._sel(S.prg_H(s) ^ (t * _uncompressed(key["bits"][i], key["cw_sigma"][i], key["cw_s"][i], n_el)), x_bits[i])
        sigma, tau, s, t = state[0:2], state[2], state[3:5], state[5]
        acc = acc + (sgn * (tau.astype(I64) * leaf[i] + S.convert(sigma))).view(U64)
    return (acc + (sgn * (t.astype(I64) * leaf[n] + S.convert(s))).view(U64)).view(I64)


def _keygen_job(args):
    return _keygen_serial(*args)


def _eval_job(args):
    return _eval_serial(*args)


def _sliced(key, a, c):
    return {name: np.ascontiguousarray(v[..., a:c]) for name, v in key.items()}


def dif_keygen(alpha, s0_pair, n):
    """keys[b] = dict(s0 [2, N], bits uint8 [n, 4, N] (tauL, tL, tauR, tR), cw_sigma [n, 2, N], cw_s [n, 2, N], cw_leaf int32
    [n + 1, N]).  Above the oracle's MULTI_LIMIT, element slices go to the pool the oracle has installed (S.use_pool), like the
    oracle's own."""
    alpha, s0_pair = np.asarray(alpha, U64), np.asarray(s0_pair, U64)
    if S._POOL is None or alpha.shape[0] <= S.MULTI_LIMIT:
        return _keygen_serial(alpha, s0_pair, n)
    pool, k = S._POOL
    parts = pool.map(_keygen_job, [(alpha[a:c], np.ascontiguousarray(s0_pair[:, :, a:c]), n) for a, c in S._cuts(alpha.shape[0], k)])
    return [{name: np.concatenate([p[b][name] for p in parts], axis=-1) for name in parts[0][b]} for b in range(2)]


def dif_eval(b, x, key, n):
    """Party b's int64 share of [x <= alpha] on the masked input x (its low n bits)."""
    x = np.asarray(x)
    if S._POOL is None or x.shape[0] <= S.MULTI_LIMIT:
        return _eval_serial(b, x, key, n)
    pool, k = S._POOL
    return np.concatenate(pool.map(_eval_job, [(b, x[a:c], _sliced(key, a, c), n) for a, c in S._cuts(x.shape[0], k)]))


def fss_le(x1, x2, alpha_shares, keys, n):
    """Shares of [x1 <= x2] at width n: mask, open mod 2^n, both parties' evaluations."""
    r = [S.fss_mask(x1[j], x2[j], alpha_shares[j]) for j in range(2)]
    masked = fss_open(r[0], r[1], n)
    return [dif_eval(j, masked, keys[j], n) for j in range(2)]


def packed_bits(bits):
    """The library's control-bit bytes [n, N] (bit0 tauL, bit1 tL, bit2 tauR, bit3 tR) from the restatement's [n, 4, N]."""
    b = bits.astype(np.uint8)
    return b[:, 0] | (b[:, 1] << 1) | (b[:, 2] << 2) | (b[:, 3] << 3)


# ---- the definition, in Python ints -------------------------------------------------------------------------------------
def defined_bit(alpha, d, n):
    """[(d + alpha) mod 2^n <= alpha] for alpha in [0, 2^n) and an integer d."""
    return int((int(d) + int(alpha)) % (1 << n) <= int(alpha))


def wraps(alpha, d, n):
    """alpha + d leaves [0, 2^n): the comparison's answer is then not [d <= 0] in general."""
    return not 0 <= int(alpha) + int(d) < (1 << n)


# ---- inputs the tests share ----------------------------------------------------------------------------------------------
CRAFTED_D = (0, 1, -1, 2 ** 31 - 1, -(2 ** 31 - 1), 2 ** 31, 3 * 2 ** 30, 2 ** 32, -2 ** 33, 2 ** 40, -2 ** 40)


def seeds(rng, n):
    s0 = rng.integers(0, 2 ** 64, size=(2, 2, n), dtype=U64)
    s0[:, 0] &= U64(2 ** 63 - 1)
    return s0


def as_i64(values):
    """Python ints (any sign, below 2^64 in magnitude) as ring elements."""
    return np.array([v % 2 ** 64 for v in values], dtype=U64).view(I64)


def shares_of(rng, secret):
    r = rng.integers(-2 ** 63, 2 ** 63, size=secret.shape, dtype=I64)
    return [r, S.rsub(secret, r)]


def crafted_pairs(n):
    """(alpha, d) in Python ints: every crafted alpha with every crafted d that fits in n bits, and the two wraps."""
    alphas = [0, 1, 2 ** n - 1, 2 ** (n - 1)]
    pairs = [(a, d) for a in alphas for d in CRAFTED_D if abs(d) < 2 ** (n - 1)]
    return pairs + [(5, -6), (12345, -2 ** 33)]


# ---- replaying a dealer's log at a width ---------------------------------------------------------------------------------
class WideReplayDealer(S.ReplayDealer):
    """ReplayDealer whose comparison keys have n levels: the log's raw alpha and mask are reduced mod 2^n here."""

    def __init__(self, log, bits):
        super().__init__(log)
        self.bits = bits

    def dif_keys(self, n):
        _, en, alpha, s0, r = self._next("dif")
        assert en == n
        alpha, r = alpha.view(U64) & width_mask(self.bits), r.view(U64)
        keys = dif_keygen(alpha, s0.view(U64), self.bits)
        a0, a1 = split_alpha(alpha, r, self.bits)
        return [a0, a1], keys


class WideOracleContext(S.OracleContext):
    """OracleContext whose comparisons are n bits wide; relu, max_pair, max_pool2d_3x3s2 and every forward built on `le` run
    on it unchanged.  `compared` collects, per call of le, (alpha, d): the reduced alpha and the signed difference x1 - x2."""

    def __init__(self, dealer, base=10, precision_fractional=16, bits=32):
        super().__init__(dealer, base, precision_fractional)
        self.bits = bits
        self.compared = []

    def le(self, x1, x2):
        shape = x1[0].shape
        alpha_sh, keys = self.dealer.dif_keys(x1[0].size)
        f1, f2 = [v.reshape(-1) for v in x1], [v.reshape(-1) for v in x2]
        alpha = (alpha_sh[0] + alpha_sh[1]) & width_mask(self.bits)
        self.compared.append((alpha, S.rsub(S.radd(f1[0], f1[1]), S.radd(f2[0], f2[1]))))
        return [o.reshape(shape) for o in fss_le(f1, f2, alpha_sh, keys, self.bits)]
