"""The definition of the secret-shared argmax that ends an encrypted pass with reveal="class" (the reference has none: it opens
the logits and takes the argmax in the clear), crafted logits and the request list of the tail, shared by
tests/test_secure_argmax_host.py and tests/test_gpu_secure_argmax.py: a module of helpers, not of tests.
Everything is composed from oracle.secure_oracle's own functions; nothing under oracle/ knows about the layer."""
import numpy as np

from oracle import secure_oracle as S

I64 = np.int64


def oracle_argmax(ctx, logits):
    """The first-index argmax over the classes of the shared fixed-point logits [B, C] on an OracleContext -- THE definition
    of the layer.  Returns (I, V): shares of the raw, unscaled int64 class indices [B] and of the maxima [B];
    a pass reconstructs I alone.  The order of the requests and of the elements inside each triple is part of the
    definition.  Walking from the last class down with le(V, L_k) = [L_k >= V] sends a tie to the lower index."""
    B, C = logits[0].shape
    col = lambda k: [np.ascontiguousarray(logits[j][:, k]) for j in range(2)]
    V = col(C - 1)                                                                  # 1
    I = ctx.share(np.full((B,), C - 1, I64))                                        #    (one const_mask(B))
    for k in range(C - 2, -1, -1):                                                  # 2
        Lk = col(k)
        bit = ctx.le(V, Lk)                                                         #    dif_keys(B)
        K = ctx.share(np.full((B,), k, I64))                                        #    const_mask(B)
        D = [np.stack([S.rsub(Lk[j], V[j]), S.rsub(K[j], I[j])], axis=1) for j in range(2)]
        bit2 = [np.ascontiguousarray(np.stack([bit[j], bit[j]], axis=1)) for j in range(2)]
        R = ctx.beaver_mul(bit2, D)                                                 #    ("mul", (B, 2), (B, 2)), no truncation
        V = [S.radd(V[j], np.ascontiguousarray(R[j][:, 0])) for j in range(2)]
        I = [S.radd(I[j], np.ascontiguousarray(R[j][:, 1])) for j in range(2)]
    return I, V                                                                     # 3  (only I is ever reconstructed)


def tail_requests(B, C):
    """What oracle_argmax asks its dealer for, as (kind, args) pairs."""
    return [("const_mask", (B,))] + (C - 1) * [("dif_keys", (B,)), ("const_mask", (B,)), ("triple", ("mul", (B, 2), (B, 2)))]


def first_argmax(q):
    """np.argmax over the classes of encoded logits [B, C]: the first index on ties, as torch.argmax."""
    return np.argmax(np.asarray(q, I64), axis=1).astype(I64)


def spread(q):
    """The largest pairwise difference inside a row of encoded logits [B, C] (as a Python int: no wrap)."""
    q = np.asarray(q, I64)
    return max(int(r.max()) - int(r.min()) for r in q)


# (B, C) -> encoded logits: exact ties, all-equal rows, negative values, the maximum in the first, middle and last column.
# Every pairwise difference d is below 2^31 (the tests assert it) -- and small: the reference's comparison adds a uniform
# 32-bit mask alpha to the difference and tests the sum WITHOUT its carry (mpc/fss.py:158), so it answers wrongly when
# alpha + d wraps, with probability |d| / 2^32 over the dealer's draw.  With |d| <= 20,000 that is under 5e-6 per comparison
# (about 100 comparisons are made here, under fixed dealer seeds).
BIG = 10_000
CRAFTED = {
    (1, 2): [np.array([[5, 5]], I64), np.array([[-7, 3]], I64), np.array([[BIG, -BIG]], I64), np.array([[-3, -9]], I64)],
    (1, 3): [np.array([[1, 9, 9]], I64), np.array([[-4, -4, -4]], I64), np.array([[-BIG, 0, BIG]], I64),
             np.array([[2, 7, -1]], I64), np.array([[8, 8, 3]], I64)],
    (4, 3): [np.array([[10, -2, 3], [-5, -1, -9], [0, 0, 1], [7, 7, 7]], I64),
             np.array([[-BIG, BIG, BIG], [BIG, -BIG, BIG], [-1, -1, -2], [1234, -1234, 1233]], I64)],
    (3, 5): [np.array([[0, 1, 2, 3, 4], [4, 3, 9, 1, 0], [6, 6, 6, 6, 6]], I64),
             np.array([[-8, -3, -3, -9, -3], [BIG, 0, -BIG, BIG, 1], [-1000, -999, -998, -997, -998]], I64),
             np.array([[9, 0, 0, 0, 0], [0, 0, 5, 5, 0], [-2, -2, -2, -2, -1]], I64)],
}
