"""The definition of the rank-count tail that ends an encrypted evaluation with reveal="metrics" (the reference computes its
one-vs-one ROC AUC on opened scores), the exact counts in Python ints, crafted evaluations and host-side dealers that serve
comparison keys at a requested width, shared by tests/test_secure_auc_host.py and tests/test_gpu_secure_auc.py: a
module of helpers, not of tests.  Everything is composed from oracle.secure_oracle's own functions and
tests/fss_wide_ref.py's restatement of the wide comparison; nothing under oracle/ knows about the layer."""
import numpy as np

from oracle import secure_oracle as S
from tests import fss_wide_ref as W
from tests.secure_argmax_nets import CRAFTED, oracle_argmax, tail_requests
from tests.secure_confusion_nets import ConfusionChaChaDealer, ConfusionRecordingDealer, ConfusionReplayDealer, onehot

I64, U64 = np.int64, np.uint64
AUC_BITS = 64                      # the width of the rank comparisons, whatever the dealer's
AUC_BLOCK_COMPARISONS = 2 ** 20


def block_rows_of(N, C):
    """Rows per block: a public function of public sizes, part of the definition (the request order depends on it)."""
    return max(1, min(N, AUC_BLOCK_COMPARISONS // (C * N)))


def ring_rowsum(x):
    return np.asarray(x, I64).view(U64).sum(axis=1, dtype=U64).view(I64)


def oracle_auc_counts(ctx, L, Y, U, block_rows=None):
    """The tail on an OracleContext -- THE definition of the layer.  L: shares of the fixed-point logits [N, C]
    of every row the evaluation held, padding rows included; Y: SHARES of the raw one-hot labels [N, C], all-zero rows for
    padding; U: shares of the [C, C, C] accumulator.  Returns the updated shares of U: U[p][a][q] counts (i of label p, j of
    label q) with n[i][a] d[j] <= d[i] n[j][a], n = L - rowmin(L), d = rowsum(n) -- the order of the normalised scores
    n_a / d, cross-multiplied.  Raw int64 throughout, no scale.  The dealer's dif_keys takes `bits`: the rank comparisons are
    64 bits wide, the min walk runs at the dealer's own width.  The order of the requests and of the elements inside each
    primitive is part of the definition."""
    N, C = L[0].shape
    _, Vn = oracle_argmax(ctx, ctx.neg(L))                                          # 1  max of -L: the walk, its index dropped
    n = [S.radd(L[j], Vn[j][:, None]) for j in range(2)]                            #    L - min, party-local
    d = [ring_rowsum(n[j]) for j in range(2)]
    nT = [np.ascontiguousarray(n[j].T) for j in range(2)]
    Rb = block_rows_of(N, C) if block_rows is None else int(block_rows)
    for r0 in range(0, N, Rb):                                                      # 2  row blocks, the last ragged
        R = min(Rb, N - r0)
        blk = slice(r0, r0 + R)
        t = ctx.dealer.triple("matmul", (R * C, 1), (1, N))
        A = S.beaver("matmul", [n[j][blk].reshape(R * C, 1) for j in range(2)], [d[j].reshape(1, N) for j in range(2)], t)
        t = ctx.dealer.triple("matmul", (R, 1), (1, C * N))
        Bm = S.beaver("matmul", [d[j][blk].reshape(R, 1) for j in range(2)], [nT[j].reshape(1, C * N) for j in range(2)], t)
        alpha_sh, keys = ctx.dealer.dif_keys(R * C * N, bits=AUC_BITS)
        G = W.fss_le([A[j].reshape(-1) for j in range(2)], [Bm[j].reshape(-1) for j in range(2)], alpha_sh, keys, AUC_BITS)
        t = ctx.dealer.triple("matmul", (R * C, N), (N, C))
        T = S.beaver("matmul", [G[j].reshape(R * C, N) for j in range(2)], Y, t)    #    no truncation: both factors unscaled
        t = ctx.dealer.triple("matmul", (C, R), (R, C * C))
        Uc = S.beaver("matmul", [np.ascontiguousarray(Y[j][blk].T) for j in range(2)], [T[j].reshape(R, C * C) for j in range(2)], t)
        U = [S.radd(U[j], Uc[j].reshape(C, C, C)) for j in range(2)]
    return U


def zero_counts(C):
    return [np.zeros((C, C, C), I64), np.zeros((C, C, C), I64)]


def auc_tail_requests(N, C, block_rows=None):
    """What oracle_auc_counts asks its dealer for, as (kind, args[, kwargs]) entries in the recording dealers' form."""
    Rb = block_rows_of(N, C) if block_rows is None else int(block_rows)
    req = tail_requests(N, C)
    for r0 in range(0, N, Rb):
        R = min(Rb, N - r0)
        req += [("triple", ("matmul", (R * C, 1), (1, N))), ("triple", ("matmul", (R, 1), (1, C * N))),
                ("dif_keys", (R * C * N,), {"bits": AUC_BITS}), ("triple", ("matmul", (R * C, N), (N, C))),
                ("triple", ("matmul", (C, R), (R, C * C)))]
    return req


def needed(C):
    """bool [C, C, C]: the entries U[p][a][q] the score reads (exactly one of p, q is a); the others are zeroed before the
    opening."""
    k = np.arange(C)
    return (k[:, None, None] == k[None, :, None]) != (k[None, None, :] == k[None, :, None])


def exact_counts(q, labels, opened=False):
    """The counts in Python ints: q integer logits [N, C], labels int [N] with -1 for a padding row.  opened=True: the entries
    the score does not read are zero, as in what an evaluation opens."""
    q = [[int(v) for v in row] for row in np.asarray(q).tolist()]
    labels = [int(l) for l in np.asarray(labels).tolist()]
    N, C = len(q), len(q[0])
    n = [[v - min(row) for v in row] for row in q]
    d = [sum(row) for row in n]
    U = np.zeros((C, C, C), I64)
    for i in range(N):
        for j in range(N):
            if labels[i] < 0 or labels[j] < 0:
                continue
            for a in range(C):
                if n[i][a] * d[j] <= d[i] * n[j][a]:
                    U[labels[i], a, labels[j]] += 1
    return U * needed(C) if opened else U


def largest_product(q):
    """The largest |n[i][a] d[j]| of a set of integer logits, as a Python int: must stay below 2^63."""
    rows = [[int(v) for v in row] for row in np.asarray(q).tolist()]
    n = [[v - min(row) for v in row] for row in rows]
    return max(max(r) for r in n) * max(sum(r) for r in n)


# ---- crafted evaluations ---------------------------------------------------------------------------------------------------
# (N, C): the rows of every CRAFTED shape of C classes, stacked and repeated in order to N rows.  The rows bring exact ties
# of the normalised scores between different rows (a repeated row; the zero of every row's smallest class; [1, 9, 9] and
# [-BIG, BIG, BIG]), a row of all-equal logits (d = 0: it ties with every row) among the first three, and the last row is a
# padding row.  Row k carries label k mod C: every class is labelled wherever N - 1 >= C, i.e. everywhere but (4, 5), where
# three labelled rows cannot cover five classes -- that case holds the counts to the integers all the same, and the score
# derived from them is the undefined one, 0.0.
CASES = [(N, C) for N in (4, 7, 12) for C in (2, 3, 5)]
_ALL_EQUAL_FIRST = {2: [0, 1, 2, 3], 3: [1, 0, 2, 3, 4], 5: [2, 0, 1]}      # the order of the first rows of each class count


def crafted_rows(C):
    rows = np.concatenate([arr for shape in sorted(CRAFTED) if shape[1] == C for arr in CRAFTED[shape]])
    head = _ALL_EQUAL_FIRST[C]
    order = head + [k for k in range(len(rows)) if k not in head]
    return rows[order]


def crafted_case(N, C):
    """(encoded logits [N, C], labels [N] with -1 for the padding row, raw one-hot labels [N, C])."""
    rows = crafted_rows(C)
    q = np.ascontiguousarray(rows[np.arange(N) % len(rows)], I64)
    labels = np.arange(N, dtype=I64) % C
    labels[N - 1] = -1
    assert any(len(set(r)) == 1 for r in q[:N - 1].tolist())                     # an all-equal row, labelled
    assert largest_product(q) < 2 ** 40
    return q, labels, onehot(labels, C)


def every_class_labelled(labels, C):
    return set(range(C)) <= set(int(l) for l in labels)


def has_cross_row_ties(q, labels):
    """Two different labelled rows with d > 0 and an equal normalised score in some class."""
    rows = [[int(v) for v in row] for row in np.asarray(q).tolist()]
    n = [[v - min(row) for v in row] for row in rows]
    d = [sum(r) for r in n]
    ok = [i for i in range(len(rows)) if labels[i] >= 0 and d[i] > 0]
    return any(n[i][a] * d[j] == d[i] * n[j][a] for i in ok for j in ok if i != j for a in range(len(rows[0])))


# the debug dealer seeds of the crafted evaluations: under each, oracle_auc_counts on an AucChaChaDealer -- whose 32-bit min
# walk errs with probability about 5e-6 per comparison at these magnitudes -- reconstructs exact_counts at every block size
# (tests/test_secure_auc_host.py holds that on the host, so a GPU test on the same seed cannot meet a wrong comparison)
HOST_SEEDS = {case: 200 + k for k, case in enumerate(CASES)}
GPU_CASE = (7, 3)
GPU_BLOCK_ROWS = 3                 # two full blocks and a ragged one on 7 rows


# ---- host-side dealers whose dif_keys takes `bits` ----------------------------------------------------------------------------
def _wide_keys(alpha, s0, r, bits):
    m = W.width_mask(bits)
    alpha = np.asarray(alpha, U64) & m
    keys = W.dif_keygen(alpha, s0, bits)
    return list(W.split_alpha(alpha, r, bits)), keys


class AucRecordingDealer(ConfusionRecordingDealer):
    """ConfusionRecordingDealer whose comparison keys may name a width: the same words are drawn, the width decides their
    reduction and the number of levels; the request records the width the way primia_amd.secure.Dealer.requests does."""

    def dif_keys(self, n, bits=None):
        if bits is None:
            return super().dif_keys(n)
        self.requests.append(("dif_keys", (n,), {"bits": int(bits)}))
        alpha = self.rng.integers(0, 2 ** 64 - 1, size=n, dtype=U64, endpoint=True)
        s0 = self.rng.integers(0, 2 ** 64 - 1, size=(2, 2, n), dtype=U64, endpoint=True)
        s0[:, 0] &= U64(2 ** 63 - 1)
        r = self.rng.integers(0, 2 ** 64 - 1, size=n, dtype=U64, endpoint=True)
        return _wide_keys(alpha, s0, r, bits)


class AucChaChaDealer(ConfusionChaChaDealer):
    """primia_amd.secure.Dealer(device, seed=seed) on the host, dif_keys(n, bits=...) included: the words Dealer.dif_keys
    draws, in its order, under primia_fss_alpha_split_n's masking at the requested width."""

    def dif_keys(self, n, bits=None):
        if bits is None:
            return super().dif_keys(n)
        self.requests.append(("dif_keys", (n,), {"bits": int(bits)}))
        alpha = self._rand((n,)).view(U64)
        s0 = self._rand((2, 2, n)).view(U64).copy()
        s0[:, 0] &= U64(2 ** 63 - 1)
        r = self._rand((n,)).view(U64)
        return _wide_keys(alpha, s0, r, bits)


class AucReplayDealer(ConfusionReplayDealer):
    """ConfusionReplayDealer for a log that holds comparison keys of two widths: the log's entry carries the raw words, the
    REQUEST says at which width they were reduced -- the dealer's (`fss_bits`, 32 by default) or the one it names."""

    def __init__(self, log, fss_bits=32):
        super().__init__(log)
        self.fss_bits = fss_bits

    def dif_keys(self, n, bits=None):
        w = self.fss_bits if bits is None else int(bits)
        if w == 32:
            return super().dif_keys(n)
        _, en, alpha, s0, r = self._next("dif")
        assert en == n
        return _wide_keys(alpha.view(U64), s0.view(U64), r.view(U64), w)
