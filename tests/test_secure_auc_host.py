"""CPU: the ROC AUC of an encrypted evaluation from rank counts (primia_amd.torchlib_compat.auc_from_rank_counts) against
scikit-learn, the definition of the rank-count tail (tests/secure_auc_nets.py) against the counts in Python ints on crafted
evaluations, and the host-side schedule and memory arithmetic of reveal="metrics" (no device is touched)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from oracle import secure_oracle as S
from primia_amd import _lib, secure
from primia_amd.secure import (DIF_KEY_BYTES, architecture_of, argmax_requests, auc_block_rows, auc_requests, image_requests,
                               largest_batch_that_fits, primitive_bytes, serving_bytes)
from primia_amd.torchlib_compat import auc_from_rank_counts
from tests.secure_auc_nets import (AUC_BITS, CASES, GPU_BLOCK_ROWS, GPU_CASE, HOST_SEEDS, AucChaChaDealer, AucRecordingDealer,
                                   AucReplayDealer, auc_tail_requests, block_rows_of, crafted_case, every_class_labelled,
                                   exact_counts, has_cross_row_ties, largest_product, needed, oracle_auc_counts, zero_counts)
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet, resnet18
from tests.secure_groupnorm_nets import group_resnet18

I64 = np.int64
ids = lambda s: "x".join(map(str, s))


# ---- 1. the score from the counts -----------------------------------------------------------------------------------------
def sklearn_auc(q, labels):
    """The reference's score on float-normalised scores: roc_auc_score(..., multi_class="ovo") (binary: on column 1)."""
    from sklearn import metrics as mt

    scores = np.asarray(q, np.float64)
    scores = scores - scores.min(axis=1)[:, None]
    scores = scores / scores.sum(axis=1)[:, None]
    C = scores.shape[1]
    if C == 2:
        return float(mt.roc_auc_score(labels, scores[:, 1]))
    return float(mt.roc_auc_score(labels, scores, multi_class="ovo", labels=list(range(C))))


def random_logit_sets():
    """30 sets of integer logits with 3 to 5 classes (and four with 2) and 8 to 40 rows, a third of them tie-heavy (values
    drawn from four levels), rows of all-equal logits removed, every class labelled."""
    rng = np.random.default_rng(20)
    out = []
    for k in range(34):
        C = 2 if k >= 30 else int(rng.integers(3, 6))
        N = int(rng.integers(8, 41))
        q = rng.integers(0, 4, size=(N, C)) * 1000 if k % 3 == 0 else rng.integers(-30_000, 30_000, size=(N, C))
        q = q[q.max(axis=1) > q.min(axis=1)]
        labels = np.concatenate([np.arange(C), rng.integers(0, C, size=len(q) - C)])
        out.append((q.astype(I64), labels.astype(I64)))
    return out


def test_auc_from_rank_counts_is_sklearns_auc():
    """auc_from_rank_counts on the exact counts equals scikit-learn's one-vs-one AUC on the float-normalised scores within
    1e-12 (measured: 1.1e-16), on random and tie-heavy integer logits; the counts it is given hold nothing but the entries an
    evaluation opens."""
    worst = 0.0
    for q, labels in random_logit_sets():
        C = q.shape[1]
        U = exact_counts(q, labels, opened=True)
        got = auc_from_rank_counts(U, np.bincount(labels, minlength=C))
        want = sklearn_auc(q, labels)
        worst = max(worst, abs(got - want))
        assert got == auc_from_rank_counts(exact_counts(q, labels), np.bincount(labels, minlength=C))      # only `needed` is read
    print("max |auc_from_rank_counts - sklearn| =", worst)
    assert worst <= 1e-12


def test_auc_of_an_absent_class_is_zero_and_two_classes_are_binary(capsys):
    """A class without a labelled image: 0.0 with the reference's warning.  Two classes: AUC(1|0), the binary form -- and, rows
    of equal logits apart, what the one-vs-one mean gives too."""
    q = np.array([[3, 1, 2], [0, 5, 1], [2, 2, 9], [4, 0, 0]], I64)
    labels = np.array([0, 1, 0, 1], I64)
    assert auc_from_rank_counts(exact_counts(q, labels), np.bincount(labels, minlength=3)) == 0.0
    assert "could not be calculated" in capsys.readouterr().err
    q2 = np.array([[3, 1], [0, 5], [2, 9], [4, 0], [1, 2], [7, 6]], I64)
    l2 = np.array([0, 1, 1, 0, 0, 1], I64)
    U = exact_counts(q2, l2)
    n = np.bincount(l2, minlength=2)
    binary = 0.5 + (int(U[0, 1, 1]) - int(U[1, 1, 0])) / (2 * int(n[0]) * int(n[1]))
    other = 0.5 + (int(U[1, 0, 0]) - int(U[0, 0, 1])) / (2 * int(n[0]) * int(n[1]))
    assert auc_from_rank_counts(U, n) == binary == other
    assert abs(binary - sklearn_auc(q2, l2)) <= 1e-12
    with pytest.raises(ValueError):
        auc_from_rank_counts(np.zeros((3, 3, 2), I64), [1, 1, 1])


# ---- 2. the definition against the integers -------------------------------------------------------------------------------
def test_crafted_cases_hold_what_they_promise():
    for N, C in CASES:
        q, labels, y = crafted_case(N, C)
        assert q.shape == y.shape == (N, C) and labels[-1] == -1 and not y[-1].any() and int(y.sum()) == N - 1
        assert every_class_labelled(labels, C) == (N - 1 >= C)
        assert has_cross_row_ties(q, labels) or N == 4      # (four rows: the all-equal row's ties only)
        assert largest_product(q) < 2 ** 31                 # far below 2^63: a 64-bit comparison errs with p < 2^-33 each
    assert sum(every_class_labelled(crafted_case(N, C)[1], C) for N, C in CASES) == len(CASES) - 1


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_oracle_auc_counts_reconstruct_the_exact_counts(case):
    """oracle_auc_counts on the host mirror of the device dealer, under the case's fixed debug seed, at the default block size
    (one block), 3 rows and 1 row per block: U reconstructs to exact_counts -- ties, the all-equal row, the padding row
    included; no share is the value it hides; the requests are auc_tail_requests, and primia_amd.secure.auc_requests names
    the same ones.  The 32-bit min walk errs with about 5e-6 per comparison at these magnitudes: that every seed here gives
    the exact counts IS the assertion that the seeds are good ones (the GPU test runs under one of them)."""
    N, C = case
    q, labels, y = crafted_case(N, C)
    want = exact_counts(q, labels)
    for block_rows in (None, 3, 1):
        d = AucChaChaDealer(HOST_SEEDS[case])
        ctx = S.OracleContext(d, 10, 3)
        L, Y = ctx.share(q), ctx.share(y)
        n0 = len(d.requests)
        U = oracle_auc_counts(ctx, L, Y, zero_counts(C), block_rows)
        assert np.array_equal(S.radd(*U), want), block_rows
        assert not np.array_equal(U[0], want) and not np.array_equal(U[1], want)
        asked = d.requests[n0:]
        assert asked == auc_tail_requests(N, C, block_rows)
        mine = auc_requests(N, C, block_rows)
        assert [(k, a) for k, a, _ in mine] == [(e[0], e[1]) for e in asked]
        assert [kw for k, _, kw in mine if k == "dif_keys"] == (C - 1) * [{}] + [{"bits": AUC_BITS}] * -(-N // (block_rows or N))
    if every_class_labelled(labels, C):
        assert 0.0 < auc_from_rank_counts(want * needed(C), y.sum(axis=0)) < 1.0


def test_counts_accumulate_and_the_recording_dealer_serves_widths():
    """On the numpy dealer: a second evaluation adds to what U held; keys of 64 levels come from dif_keys(n, bits=64)."""
    N, C = GPU_CASE
    q, labels, y = crafted_case(N, C)
    d = AucRecordingDealer(77)
    ctx = S.OracleContext(d, 10, 3)
    U = oracle_auc_counts(ctx, ctx.share(q), ctx.share(y), zero_counts(C), GPU_BLOCK_ROWS)
    U = oracle_auc_counts(ctx, ctx.share(q), ctx.share(y), U, GPU_BLOCK_ROWS)
    assert np.array_equal(S.radd(*U), 2 * exact_counts(q, labels))
    (a0, a1), keys = d.dif_keys(3, bits=40)
    assert keys[0]["cw_leaf"].shape == (41, 3) and int((a0 + a1).max()) < 2 ** 41
    assert d.requests[-1] == ("dif_keys", (3,), {"bits": 40})


def test_replay_dealer_serves_both_widths():
    """AucReplayDealer re-derives the keys of a ("dif", ...) entry at 32 levels by default and at the width a request names."""
    n = 3
    rng = np.random.default_rng(4)
    words = lambda: rng.integers(0, 2 ** 63, size=n, dtype=np.uint64)
    s0 = rng.integers(0, 2 ** 63, size=(2, 2, n), dtype=np.uint64)
    a32, r32, a64, r64 = words() & np.uint64(0xFFFFFFFF), words() & np.uint64(0xFFFFFFFF), words(), words()
    d = AucReplayDealer([("dif", n, a32.view(I64), s0.view(I64), r32.view(I64)), ("dif", n, a64.view(I64), s0.view(I64), r64.view(I64))])
    _, k32 = d.dif_keys(n)
    (b0, b1), k64 = d.dif_keys(n, bits=64)
    assert k32[0]["cw_leaf"].shape[0] == 33 and k64[0]["cw_leaf"].shape == (65, n)
    assert np.array_equal(b0 + b1, a64) and np.array_equal(b1, r64)


# ---- 3. schedule and bytes ------------------------------------------------------------------------------------------------
def test_block_rows_are_a_public_function_of_the_sizes():
    assert auc_block_rows(624, 3) == block_rows_of(624, 3) == 560 and auc_block_rows(7, 3) == 7 and auc_block_rows(2000, 5) == 104
    assert auc_block_rows(2 ** 20, 2) == 1 and secure.AUC_BLOCK_COMPARISONS == 2 ** 20 and secure.AUC_BITS == 64
    req = auc_requests(624, 3)
    assert req[:len(argmax_requests(624, 3))] == argmax_requests(624, 3)
    blocks = req[len(argmax_requests(624, 3)):]
    assert len(blocks) == 10 and blocks[2] == ("dif_keys", (560 * 3 * 624,), {"bits": 64})
    assert blocks[5:] == [("triple", ("matmul", (64 * 3, 1), (1, 624)), {}), ("triple", ("matmul", (64, 1), (1, 3 * 624)), {}),
                          ("dif_keys", (64 * 3 * 624,), {"bits": 64}), ("triple", ("matmul", (64 * 3, 624), (624, 3)), {}),
                          ("triple", ("matmul", (3, 64), (64, 9)), {})]
    assert sum(a[0] for k, a, _ in req if k == "dif_keys") == 2 * 624 + 3 * 624 * 624


def test_primitive_bytes_count_the_wide_keys_at_their_width():
    n = 11
    assert primitive_bytes([("dif_keys", (n,), {"bits": 64})]) == n * DIF_KEY_BYTES(64) == n * 2428
    assert primitive_bytes([("dif_keys", (n,), {"bits": 64})], 40) == n * DIF_KEY_BYTES(64)
    assert primitive_bytes([("dif_keys", (n,), {})]) == n * DIF_KEY_BYTES == n * 1244
    assert primitive_bytes([("dif_keys", (n,), {})], 40) == n * DIF_KEY_BYTES(40)
    N, C = 7, 3
    tail = auc_requests(N, C, 3)
    triples = sum(16 * (R * C + N + R * C * N + R + C * N + R * C * N + R * C * N + N * C + R * C * C + C * R + R * C * C + C * C * C)
                  for R in (3, 3, 1))
    assert primitive_bytes(tail) == primitive_bytes(argmax_requests(N, C)) + triples + C * N * N * DIF_KEY_BYTES(64)


NETS = [("mini-batch", lambda: mini_resnet(torch.Generator().manual_seed(21)), MINI_BLOCKS),
        ("resnet18-batch", lambda: resnet18(32, 320), None),
        ("resnet18-group", lambda: group_resnet18(32, 520), None)]


@pytest.mark.parametrize("net", NETS, ids=lambda n: n[0])
def test_existing_request_lists_are_unchanged_by_the_new_argument(net):
    """No pass names a width: every comparison request of the logits, class and confusion lists is ("dif_keys", (n,), {}), the
    form it has always had; a metrics pass IS a confusion pass, down to the bytes and the largest batch."""
    _, make, blocks = net
    arch = architecture_of(make())
    for pooling in ("max", "avg"):
        lists = {r: image_requests(arch, 32, 3, blocks, pooling, reveal=r) for r in secure.EVALUATION_REVEALS}
        for r, req in lists.items():
            assert all(kw == {} for k, _, kw in req if k in ("dif_keys", "dpf_keys", "triple")), r
            assert all(set(kw) == {"owner"} for k, _, kw in req if k == "const_mask"), r
        assert lists["metrics"] == lists["confusion"] and len(lists["class"]) < len(lists["confusion"])
        assert serving_bytes(arch, 32, 3, blocks, pooling, reveal="metrics") == serving_bytes(arch, 32, 3, blocks, pooling, reveal="confusion")
    budget = serving_bytes(arch, 32, 4, blocks, reveal="metrics")
    assert largest_batch_that_fits(arch, 32, budget - 1, blocks, reveal="metrics") == 3
    assert secure.REVEALS == ("logits", "class") and secure.EVALUATION_REVEALS == ("logits", "class", "confusion", "metrics")
    assert secure.METRICS == "metrics"
    for cls in (secure.Dealer, secure.PreloadedDealer, secure.PartyDealer):
        assert inspect.signature(cls.dif_keys).parameters["bits"].default is None
    assert inspect.signature(secure.SecureContext.le).parameters["bits"].default is None


def test_header_declares_the_two_kernels():
    """primia_auc_cross_local takes the shares of n and d, the two triples' pointer tables, the four outputs and the block;
    primia_auc_count_combine_local the confusion combine's operands with R in place of B -- and the built library exports
    both."""
    protos = _lib.parse_header()
    names = lambda f: [n for _, n in protos[f][1]]
    assert names("primia_auc_cross_local") == ["n0", "n1", "d0", "d1", "ta", "tb", "a_out0", "a_out1", "b_out0", "b_out1", "N", "C",
                                               "row0", "R", "stream"]
    assert names("primia_auc_count_combine_local") == ["y0", "y1", "t0", "t1", "a0", "b0", "c0", "a1", "b1", "c1", "u0", "u1", "R",
                                                       "C", "stream"]
    conf = names("primia_confusion_combine_local")
    assert len(names("primia_auc_count_combine_local")) == len(conf)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "primia_auc_cross_local") and hasattr(lib, "primia_auc_count_combine_local")
