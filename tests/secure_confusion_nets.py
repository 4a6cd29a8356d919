"""The definition of the confusion-matrix tail that ends the passes of an encrypted evaluation with reveal="confusion" (the
reference's encrypted test() opens the predictions and counts them in the clear), the labels that go with the crafted logits of
tests/secure_argmax_nets.py, and host-side dealers that know the one new primitive, shared by
tests/test_secure_confusion_host.py, tests/test_gpu_secure_confusion.py and tests/three_role_cases.py: a module of
helpers, not of tests.  Everything is composed from oracle.secure_oracle's own functions; nothing under oracle/ knows about the
layer."""
import numpy as np

from oracle import secure_oracle as S
from tests.secure_argmax_nets import CRAFTED, first_argmax, oracle_argmax, tail_requests
from tests.secure_groupnorm_nets import ChaChaDealer, RecordingDealer

I64, U64 = np.int64, np.uint64


def oracle_eq(ctx, x1, x2):
    """fss.eq(x1, x2) (mpc/fss.py:97-185 with op = "eq") on an OracleContext: raw int64 shares of [x1 == x2 mod 2^32], one
    DPF key per element in row-major order (`dpf_keys(n)`).  32 bits whatever the width of the comparisons."""
    shape = x1[0].shape
    alpha_sh, keys = ctx.dealer.dpf_keys(x1[0].size)
    r = [S.fss_mask(x1[j].reshape(-1), x2[j].reshape(-1), alpha_sh[j]) for j in range(2)]
    masked = S.fss_open(r[0], r[1])
    return [S.dpf_eval(j, masked, keys[j]).reshape(shape) for j in range(2)]


def oracle_confusion(ctx, logits, labels_onehot, M):
    """One pass of the evaluation on an OracleContext -- THE definition of the layer.  logits: shares of the
    fixed-point logits [B, C]; labels_onehot: the data owner's raw int64 one-hot labels [B, C], all-zero rows for padding
    images; M: the shares of the [C, C] accumulator.  Returns (P, Mc, M): shares of the unscaled one-hot of the predicted
    class, of this pass's counts and of the updated accumulator -- M[j][k] counts label j predicted as k; after the last pass
    M, and nothing else, is reconstructed.  The order of the requests and of the elements inside each primitive is part of
    the definition."""
    B, C = logits[0].shape
    I, _ = oracle_argmax(ctx, logits)                                               # 1  the class form's tail, unchanged
    Y = ctx.share(np.ascontiguousarray(labels_onehot, I64))                         #    const_mask((B, C)), owner = party 1
    Kmat = ctx.share(np.tile(np.arange(C, dtype=I64), (B, 1)))                      # 2  const_mask((B, C))
    Ib = [np.ascontiguousarray(np.repeat(I[j][:, None], C, axis=1)) for j in range(2)]
    P = oracle_eq(ctx, Ib, Kmat)                                                    # 3  dpf_keys(B * C)
    t = ctx.dealer.triple("matmul", (C, B), (B, C))                                 # 4  no truncation: both factors unscaled
    Mc = S.beaver("matmul", [np.ascontiguousarray(Y[j].T) for j in range(2)], P, t)
    return P, Mc, [S.radd(M[j], Mc[j]) for j in range(2)]


def zero_matrix(C):
    return [np.zeros((C, C), I64), np.zeros((C, C), I64)]


def confusion_tail_requests(B, C):
    """What oracle_confusion asks its dealer for, as (kind, args) pairs."""
    return tail_requests(B, C) + [("const_mask", (B, C)), ("const_mask", (B, C)), ("dpf_keys", (B * C,)),
                                  ("triple", ("matmul", (C, B), (B, C)))]


def onehot(labels, C):
    """int labels [B], -1 for a padding image -> raw int64 one-hot [B, C] with an all-zero row per padding image."""
    labels = np.asarray(labels, I64)
    y = np.zeros((len(labels), C), I64)
    real = labels >= 0
    y[np.nonzero(real)[0], labels[real]] = 1
    return y


def numpy_confusion(labels, classes, C):
    """Counts of (label, class) pairs over the labelled rows: int64 [C, C]."""
    m = np.zeros((C, C), I64)
    for t, p in zip(np.asarray(labels).tolist(), np.asarray(classes).tolist()):
        if t >= 0:
            m[t, p] += 1
    return m


# The labels of the crafted logits, case by case (-1: a padding image).  With the first-index argmax of each row (in the
# comment) every shape fills diagonal and off-diagonal cells and has an all-zero label row.
LABELS = {
    (1, 2): [[0], [0], [1], [-1]],                                     # classes 0 | 1 | 0 | 0
    (1, 3): [[1], [2], [2], [0], [-1]],                                # classes 1 | 0 | 2 | 1 | 0
    (4, 3): [[0, 2, -1, 0], [1, 1, 0, -1]],                            # classes 0 1 2 0 | 1 0 0 0
    (3, 5): [[4, -1, 3], [1, 4, -1], [-1, 2, 0]],                      # classes 4 2 0 | 1 0 3 | 0 2 4
}
assert all(len(LABELS[s]) == len(CRAFTED[s]) and all(len(l) == s[0] for l in LABELS[s]) for s in CRAFTED)


def crafted_cases(shape):
    """[(encoded logits, labels, one-hot labels, expected counts)] of a crafted shape."""
    C = shape[1]
    return [(q, np.asarray(l, I64), onehot(l, C), numpy_confusion(l, first_argmax(q), C)) for q, l in zip(CRAFTED[shape], LABELS[shape])]


# ---- host-side dealers that know dpf_keys ---------------------------------------------------------------------------------
def _dpf_from_words(alpha, s0, r):
    _, keys = S.dpf_keygen(alpha, s0)
    return list(S.split_alpha(alpha, r)), keys


class ConfusionRecordingDealer(RecordingDealer):
    """RecordingDealer with the equality keys: the raw words of dif_keys (alpha, both seeds, alpha's mask), DPF.keygen."""

    def dpf_keys(self, n):
        self.requests.append(("dpf_keys", (n,)))
        alpha = self.rng.integers(0, 2 ** 32, size=n, dtype=U64)
        s0 = self.rng.integers(0, 2 ** 64 - 1, size=(2, 2, n), dtype=U64, endpoint=True)
        s0[:, 0] &= U64(2 ** 63 - 1)
        r = self.rng.integers(0, 2 ** 32, size=n, dtype=U64)
        return _dpf_from_words(alpha, s0, r)


class ConfusionChaChaDealer(ChaChaDealer):
    """primia_amd.secure.Dealer(device, seed=seed) on the host, dpf_keys included: the words Dealer.dpf_keys draws, in its
    order, under primia_fss_alpha_split's masking -- the host can run the crafted cases on the very primitives a GPU test
    will draw, and keep the seeds under which the 32-bit comparisons of the argmax walk are all right."""

    def dpf_keys(self, n):
        self.requests.append(("dpf_keys", (n,)))
        m32 = U64(0xFFFFFFFF)
        alpha = self._rand((n,)).view(U64) & m32
        s0 = self._rand((2, 2, n)).view(U64).copy()
        s0[:, 0] &= U64(2 ** 63 - 1)
        r = self._rand((n,)).view(U64) & m32
        return _dpf_from_words(alpha, s0, r)


class ConfusionReplayDealer(S.ReplayDealer):
    """ReplayDealer that also serves ("dpf", n, alpha, s0_pair, r) log entries, the keys re-derived HERE with the oracle's
    DPF.keygen."""

    def dpf_keys(self, n):
        _, en, alpha, s0, r = self._next("dpf")
        assert en == n
        return _dpf_from_words(alpha.astype(U64), s0.view(U64), r.astype(U64))


# the debug dealer seeds of the GPU tests of the tail on the crafted cases, per shape: under each, oracle_confusion on a
# ConfusionChaChaDealer reconstructs the expected counts for all cases of the shape run as the passes of one evaluation
# (tests/test_secure_confusion_host.py holds that on the host)
GPU_TAIL_SEEDS = {(1, 2): 31, (1, 3): 32, (4, 3): 33, (3, 5): 34}


def plaintext_classes(norm, sd, images, pf):
    """The float64 plaintext classes of a network of tests.three_role_cases.network_case (its margins are documented there)."""
    from tests.secure_batch_nets import plain_forward
    from tests.secure_groupnorm_nets import default_blocks, plain_group_forward

    fwd = plain_forward if norm == "batch" else plain_group_forward
    return np.argmax(fwd(sd, images.cpu(), default_blocks(), pf), axis=1).astype(I64)      # (float logits: not first_argmax, which casts)


def chosen_labels(classes, C=3):
    """Labels for the four images of network_case, from their float64 plaintext classes: the first and third agree with the
    class, the second and fourth are moved on by one and by two classes -- diagonal and off-diagonal cells are filled."""
    return (np.asarray(classes, I64) + np.array([0, 1, 0, 2], I64)) % C
