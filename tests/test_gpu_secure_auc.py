"""GPU: an encrypted evaluation that opens the confusion matrix and the rank counts of the reference's ROC AUC, and nothing per
image (reveal="metrics").  The tail is defined in tests/secure_auc_nets.py from the oracle's own methods; the two kernels are
held bit for bit to the chain of existing launches they replace, `SecureContext.auc_counts`, fused and step by step, to that
definition on the dealer's log, and whole networks -- eager, graphed, three roles, the CLI -- to the counts in Python ints of
the logit shares the evaluation itself kept; a recording opener shows what an evaluation opens."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import secure_oracle as S  # noqa: E402
from primia_amd import secure  # noqa: E402
from primia_amd._lib import PrimiaError, call  # noqa: E402
from primia_amd.secure import (Dealer, GraphedSecureInference, LocalOpener, PreloadedDealer, SecureContext,  # noqa: E402
                               SecureResNet18, _ptr_table, architecture_of, argmax_requests, auc_requests, image_requests,
                               model_requests)
from primia_amd.torchlib_compat import auc_from_rank_counts  # noqa: E402
from tests.secure_auc_nets import (GPU_BLOCK_ROWS, GPU_CASE, HOST_SEEDS, AucReplayDealer, crafted_case, exact_counts,  # noqa: E402
                                   oracle_auc_counts, zero_counts)
from tests.secure_common import (chunks, context, guarded, guards_intact, host, json_line, padded, run_inference,  # noqa: E402
                                 shares_equal, six, three_roles, wrapping_shares, write_checkpoint)
from tests.three_role_cases import AUC_LABELS as LABELS, THREE_RANK_BATCH, network_case  # noqa: E402

I64 = torch.int64
PF, SEED = 3, 83
ids = lambda s: "x".join(map(str, s))


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------
# (R, C, N): one thread; an odd count inside a wavefront; a tail past a 256-thread block (5 * 70 = 350); the widest class count
@pytest.mark.parametrize("shape", [(1, 2, 2), (3, 3, 7), (5, 3, 70), (2, 16, 9)], ids=ids)
def test_auc_cross_kernel_equals_the_two_matmuls(cuda, shape):
    """primia_auc_cross_local on shares near +-2^63 against the two primia_beaver_matmul chains (reshaped copies of n[blk] and
    d[blk], a transposed copy of n, primia_beaver_mask, the opens, primia_beaver_combine_matmul) on the same two triples:
    both shares of A and of Bm, bit for bit, for a block that starts inside the rows; nothing is written outside the four
    outputs and the inputs are left alone."""
    R, C, N = shape
    r0 = (N - R + 1) // 2
    rng = np.random.default_rng(R * 1000 + C * 100 + N)
    dev = lambda a: torch.from_numpy(a).to(cuda)
    n, d = ([dev(wrapping_shares(rng, s)) for _ in range(2)] for s in ((N, C), (N,)))
    dealer = Dealer(cuda, seed=47)
    ta = dealer.triple("matmul", (R * C, 1), (1, N))
    tb = dealer.triple("matmul", (R, 1), (1, C * N))
    ctx = SecureContext(PreloadedDealer([ta, tb], cuda), 10, PF)
    ctx.local_fused = False
    A = ctx.beaver_matmul([n[j][r0:r0 + R].reshape(R * C, 1) for j in range(2)], [d[j].view(1, N) for j in range(2)])
    Bm = ctx.beaver_matmul([d[j][r0:r0 + R].reshape(R, 1) for j in range(2)], [n[j].t().contiguous().view(1, C * N) for j in range(2)])
    keep = [x.clone() for x in (*n, *d, *six(ta), *six(tb))]
    bufs = [guarded(R * C * N, cuda) for _ in range(4)]
    call("primia_auc_cross_local", n[0], n[1], d[0], d[1], _ptr_table(ta), _ptr_table(tb), *[v for _, v in bufs], N, C, r0, R)
    assert all(guards_intact(b, R * C * N) for b, _ in bufs)
    assert all(torch.equal(a, b) for a, b in zip(keep, (*n, *d, *six(ta), *six(tb))))
    for k, want in enumerate((A[0], A[1], Bm[0], Bm[1])):
        assert torch.equal(bufs[k][1], want.reshape(-1)), k


def test_auc_cross_kernel_refuses_invalid_arguments(cuda):
    R, C, N, r0 = 2, 3, 5, 1
    z = lambda *s: torch.zeros(*s, dtype=I64, device=cuda)
    dealer = Dealer(cuda, seed=3)
    ta, tb = dealer.triple("matmul", (R * C, 1), (1, N)), dealer.triple("matmul", (R, 1), (1, C * N))
    good = [z(N, C), z(N, C), z(N), z(N), _ptr_table(ta), _ptr_table(tb), z(R * C * N), z(R * C * N), z(R * C * N), z(R * C * N),
            N, C, r0, R]
    call("primia_auc_cross_local", *good)
    for i in range(10):
        bad = list(good)
        bad[i] = None
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_auc_cross_local", *bad)
    # N, C outside 1 .. 16, a block that starts before or ends past the rows, an empty block
    for i, v in ((10, 0), (11, 0), (11, 17), (12, -1), (12, N - R + 1), (13, 0), (13, N + 1)):
        bad = list(good)
        bad[i] = v
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_auc_cross_local", *bad)
    for i, j in ((6, 7), (8, 9), (6, 8), (6, 0), (9, 3)):      # an output aliasing another output or an input
        bad = list(good)
        bad[i] = bad[j]
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_auc_cross_local", *bad)
    hole = (secure.ctypes.c_void_p * 6)(*[q.data_ptr() for q in six(ta)[:5]], None)      # a triple with a share missing
    bad = list(good)
    bad[4] = hole
    with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
        call("primia_auc_cross_local", *bad)


@pytest.mark.parametrize("shape", [(1, 2), (3, 5), (70, 3), (5, 16)], ids=ids)      # 16 .. 8192 threads; C = 16 is the most
def test_auc_count_combine_kernel_equals_the_chain(cuda, shape):
    """primia_auc_count_combine_local on shares near +-2^63 against the step-by-step chain (a transposed copy of Y[blk],
    primia_beaver_mask, two opens, primia_beaver_combine_matmul, an add) on the same triple: both shares of U, bit for bit,
    added to what U held; nothing is written outside U and the inputs are left alone."""
    R, C = shape
    rng = np.random.default_rng(R * 100 + C)
    dev = lambda a: torch.from_numpy(a).to(cuda)
    Y, T, U0 = ([dev(wrapping_shares(rng, s)) for _ in range(2)] for s in ((R, C), (R, C * C), (C, C * C)))
    t = Dealer(cuda, seed=43).triple("matmul", (C, R), (R, C * C))
    ctx = SecureContext(PreloadedDealer([t], cuda), 10, PF)
    ctx.local_fused = False
    Uc = ctx.beaver_matmul([Y[j].t().contiguous() for j in range(2)], T)
    want = [U0[j] + Uc[j] for j in range(2)]
    bufs = [guarded(C * C * C, cuda) for _ in range(2)]
    for (_, view), src in zip(bufs, U0):
        view.copy_(src.reshape(-1))
    keep = [x.clone() for x in (*Y, *T, *six(t))]
    call("primia_auc_count_combine_local", Y[0], Y[1], T[0], T[1], *six(t), bufs[0][1], bufs[1][1], R, C)
    assert all(guards_intact(b, C * C * C) for b, _ in bufs)
    assert all(torch.equal(a, b) for a, b in zip(keep, (*Y, *T, *six(t))))
    for j in range(2):
        assert torch.equal(bufs[j][1].view(C, C * C), want[j]), j


def test_auc_count_combine_kernel_refuses_invalid_arguments(cuda):
    R, C = 4, 3
    z = lambda *s: torch.zeros(*s, dtype=I64, device=cuda)
    good = [z(R, C), z(R, C), z(R, C * C), z(R, C * C), z(C, R), z(R, C * C), z(C, C * C), z(C, R), z(R, C * C), z(C, C * C),
            z(C, C * C), z(C, C * C), R, C]
    call("primia_auc_count_combine_local", *good)
    for i in range(12):
        bad = list(good)
        bad[i] = None
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_auc_count_combine_local", *bad)
    for i, v in ((12, 0), (12, -1), (13, 0), (13, 17)):      # R, and C outside 1 .. 16
        bad = list(good)
        bad[i] = v
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_auc_count_combine_local", *bad)
    for i, j in ((10, 11), (10, 6), (11, 9), (10, 2)):      # U aliasing itself or an input
        bad = list(good)
        bad[i] = bad[j]
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_auc_count_combine_local", *bad)


# ---- 2. the tail ------------------------------------------------------------------------------------------------------------
def test_context_auc_counts_equal_the_definition(cuda):
    """The crafted evaluation of 7 rows and 3 classes at 3 rows per block (two full blocks and a ragged one), fused and step by
    step, against oracle_auc_counts on the replayed dealer log (consumed exactly): both shares of U, bit for bit, added to what
    U held; U opens to the counts in Python ints -- ties, the all-equal row and the padding row included; the requests are
    auc_requests; the rank comparisons asked for 64-bit keys from a 32-bit dealer."""
    N, C = GPU_CASE
    q, labels, y = crafted_case(N, C)
    want = exact_counts(q, labels)
    start = wrapping_shares(np.random.default_rng(5), (2, C, C, C))
    runs = []
    for fused in (True, False):
        dealer, ctx = context(cuda, HOST_SEEDS[GPU_CASE], PF, fused)
        assert dealer.fss_bits == 32
        L, Y = ctx.share(torch.from_numpy(q).to(cuda)), ctx.share(torch.from_numpy(y).to(cuda))
        dealer.requests = []
        U = [torch.from_numpy(start[j].copy()).to(cuda) for j in range(2)]
        keep = [t.clone() for t in (*L, *Y)]
        out = ctx.auc_counts(L, Y, U, block_rows=GPU_BLOCK_ROWS)
        assert out is U and dealer.requests == auc_requests(N, C, GPU_BLOCK_ROWS)
        assert all(torch.equal(a, b) for a, b in zip(keep, (*L, *Y)))
        assert ctx.stats["dif_evals"] == (C - 1) * N + C * N * N
        runs.append(U)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    octx = S.OracleContext(AucReplayDealer(dealer.log), 10, PF)
    oL, oY = octx.share(q), octx.share(y)
    ref = oracle_auc_counts(octx, oL, oY, [start[0].copy(), start[1].copy()], GPU_BLOCK_ROWS)
    assert octx.dealer.pos == len(dealer.log)
    assert shares_equal(runs[0], ref)
    opened = host(ctx.reconstruct(runs[0]))
    assert np.array_equal(opened, S.radd(S.radd(start[0], start[1]), want))
    # from zero, at the default block size (one block), opened through auc_open: the unread entries are gone
    dealer, ctx = context(cuda, HOST_SEEDS[GPU_CASE], PF)
    L, Y = ctx.share(torch.from_numpy(q).to(cuda)), ctx.share(torch.from_numpy(y).to(cuda))
    U = [torch.zeros(C, C, C, dtype=I64).to(cuda) for _ in range(2)]
    ctx.auc_counts(L, Y, U)
    M = [torch.zeros(C, C, dtype=I64).to(cuda) for _ in range(2)]
    _, Uo = ctx.auc_open(M, U)
    assert np.array_equal(host(Uo), exact_counts(q, labels, opened=True)) and np.array_equal(host(ctx.reconstruct(U)), want)
    with pytest.raises(ValueError):
        ctx.auc_counts(L, Y, M)


# ---- 3. whole networks ------------------------------------------------------------------------------------------------------
def roc_auc_of_kept(q, labels):
    """inference.roc_auc_of -- scikit-learn on the min-shifted, row-normalised scores -- on the decoded kept logits."""
    import inference

    real = labels >= 0
    return inference.roc_auc_of(torch.from_numpy(labels[real]), torch.from_numpy(q[real]).double() / 10 ** PF)


def check_against_the_kept_rows(model, ctx, M, U, want_M, labels, batch):
    """What every form must satisfy: M is the confusion form's matrix; U is exact_counts of the logit shares the model kept,
    reconstructed HERE (the reference is the integers, not the code under test); the score is scikit-learn's on them."""
    L, Y = model.held_rows()
    q, y = host(ctx.reconstruct(L)), host(ctx.reconstruct(Y))
    rows = np.full(len(q), -1, np.int64)
    off = 0
    for _, lab in chunks(labels, labels, batch):
        rows[off:off + len(lab)] = lab.numpy()
        off += batch
    assert off == len(q) and np.array_equal(y, np.eye(3, dtype=np.int64)[np.maximum(rows, 0)] * (rows >= 0)[:, None])
    assert np.array_equal(host(M), want_M)
    assert np.array_equal(host(U), exact_counts(q, rows, opened=True))
    got, ref = auc_from_rank_counts(host(U), host(M).sum(axis=1)), roc_auc_of_kept(q, rows)
    print("roc_auc", got, "scikit-learn", ref, "U", host(U).tolist())
    assert 0.0 <= got <= 1.0
    assert abs(got - ref) <= 1e-12
    return got


@pytest.fixture(scope="module", params=["batch", "group"])
def net(request, cuda):
    """(norm, state dict, images on the device, labels, the matrix of the eager confusion form under SEED at 2 per pass)."""
    sd, images = network_case(request.param)
    images, labels = images.to(cuda), torch.tensor(LABELS, dtype=I64)
    model = SecureResNet18(SecureContext(Dealer(cuda, seed=SEED), 10, PF), sd, 32, reveal="confusion")
    model.begin()
    for chunk, lab in chunks(images, labels, 2):
        model(chunk, labels=lab)
    want = host(model.finish())
    assert want.sum() == 4 and (want.sum(axis=1) > 0).all()
    return request.param, sd, images, labels, want


def test_eager_evaluation(cuda, net):
    """Four images at two per pass under the confusion fixture's seed: the dealer was asked for model_requests, one confusion
    list per pass and auc_requests(4, 3) -- so the passes ARE the confusion passes, and M is the confusion form's, share
    stream and all; U, the score: check_against_the_kept_rows.  begin() starts over."""
    norm, sd, images, labels, want = net
    dealer = Dealer(cuda, seed=SEED)
    dealer.requests = []
    ctx = SecureContext(dealer, 10, PF)
    model = SecureResNet18(ctx, sd, 32, reveal="metrics")
    model.begin()
    for chunk, lab in chunks(images, labels, 2):
        assert model(chunk, labels=lab) is None
    arch = architecture_of(sd)
    assert dealer.requests == model_requests(arch) + 2 * image_requests(arch, 32, 2, reveal="confusion")
    assert image_requests(arch, 32, 2, reveal="metrics") == image_requests(arch, 32, 2, reveal="confusion")
    n0 = len(dealer.requests)
    M, U = model.finish()
    assert dealer.requests[n0:] == auc_requests(4, 3)
    assert M.dtype == U.dtype == I64 and tuple(U.shape) == (3, 3, 3)
    check_against_the_kept_rows(model, ctx, M, U, want, labels, 2)
    model.begin()
    assert model.kept == [] and not model.U[0].any() and not model.acc[1].any()
    with pytest.raises(ValueError):
        model.finish()


def test_graphed_evaluation(cuda, net):
    """Four images at three per pass (the second pass padded with two all-zero images, whose rows count nowhere): the captured
    pass is the confusion pass; the rows copied out after each replay give, through the eager tail in finish(), the matrix of
    the confusion form and the exact counts of those very rows."""
    norm, sd, images, labels, want = net
    B = THREE_RANK_BATCH
    g = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=PF, seed=SEED, batch=B, reveal="metrics")
    arch = architecture_of(sd)
    assert g.requests[g._n_model:] == image_requests(arch, 32, B, reveal="confusion")
    assert g.static_bytes == secure.serving_bytes(arch, 32, B, reveal="confusion")
    assert g.out is None and g._model.kept == [] and not g._model.acc[0].any() and not g._model.U[0].any()
    for step, (chunk, lab) in enumerate(chunks(images, labels, B)):
        assert g(chunk, labels=lab) is None
        assert len(g._model.kept) == step + 1
    tail = g._tail_ctx.dealer
    tail.requests = []
    M, U = g.finish()
    assert tail.requests == auc_requests(2 * B, 3)
    check_against_the_kept_rows(g._model, g._ctx, M, U, want, labels, B)
    g.begin()
    assert g._model.kept == []


class RecordingOpener:
    """Records the shape of everything opened (not a LocalOpener: the context then runs the step-by-step chain, whose opens
    all go through here or through primia_fss_open / primia_fss_open_n)."""

    def __init__(self, events):
        self.events, self.inner = events, LocalOpener()

    def open(self, shares):
        self.events.append(("open", tuple(shares[0].shape)))
        return self.inner.open(shares)


def test_an_evaluation_opens_masked_operands_and_the_two_results(cuda, net, monkeypatch):
    """The eager form with a recording opener, every open counted: each pass opens what a confusion pass opens; the tail opens
    the walk's masked inputs and products on the 4 rows, then the operands of the two K = 1 products, ONE masked 64-bit
    comparison input of C N^2 elements and the operands of the two counting products; the only values ever reconstructed
    are M and U, once each, after the tail -- no logit, no score, no bit, no label."""
    norm, sd, images, labels, want = net
    N, C = 4, 3
    events = []
    real = secure.call

    def recording_call(name, *args, **kw):
        if name in ("primia_fss_open", "primia_fss_open_n"):
            events.append(("fss" if name == "primia_fss_open" else "fss64", int(args[3])))
        return real(name, *args, **kw)

    def run(reveal):
        del events[:]
        ctx = SecureContext(Dealer(cuda, seed=SEED), 10, PF, opener=RecordingOpener(events))
        inner = ctx.opener.inner

        def reconstruct(x):
            events.append(("reconstruct", tuple(x[0].shape)))
            return inner.open(x)

        ctx.reconstruct = reconstruct
        model = SecureResNet18(ctx, sd, 32, reveal=reveal)
        model.begin()
        for chunk, lab in chunks(images, labels, 2):
            model(chunk, labels=lab)
        mark = len(events)
        out = model.finish()
        return list(events), mark, out

    with monkeypatch.context() as m:
        m.setattr(secure, "call", recording_call)
        ev_c, mark_c, Mc = run("confusion")
        ev_m, mark_m, (M, U) = run("metrics")
    assert mark_c == mark_m and ev_m[:mark_m] == ev_c[:mark_c]
    assert ev_c[mark_c:] == [("reconstruct", (C, C))]
    walk = (C - 1) * [("fss", N), ("open", (N, 2)), ("open", (N, 2))]
    block = [("open", (N * C, 1)), ("open", (1, N)), ("open", (N, 1)), ("open", (1, C * N)), ("fss64", C * N * N),
             ("open", (N * C, N)), ("open", (N, C)), ("open", (C, N)), ("open", (N, C * C))]
    assert ev_m[mark_m:] == walk + block + [("reconstruct", (C, C)), ("reconstruct", (C, C, C))]
    assert [e for e in ev_m if e[0] == "reconstruct"] == [("reconstruct", (C, C)), ("reconstruct", (C, C, C))]
    assert np.array_equal(host(M), host(Mc)) and np.array_equal(host(M), want)
    assert not host(U)[~secure.auc_needed(C).numpy()].any()


# ---- 4. three roles ---------------------------------------------------------------------------------------------------------
def test_three_roles_both_parties_hold_the_matrix_and_the_counts(cuda, net, tmp_path):
    """model_owner / data_owner / crypto_provider as three processes on one GPU over gloo, four images at three per pass, each
    process under its own time limit; every exit status is checked and after a failure nothing further is started.  Both
    parties hold the (M, U) of the in-process evaluation under the same debug seed -- itself held to the integers of its
    kept rows -- and the dealer, which served auc_requests after the last pass, holds nothing (asserted in its process)."""
    norm, sd, images, labels, want = net
    B = THREE_RANK_BATCH
    dealer = Dealer(cuda, seed=SEED)
    dealer.requests = []
    ctx = SecureContext(dealer, 10, PF)
    model = SecureResNet18(ctx, sd, 32, reveal="metrics")
    model.begin()
    for chunk, lab in chunks(images, labels, B):
        model(padded(chunk, B), labels=lab)
    M, U = model.finish()
    arch = architecture_of(sd)
    assert dealer.requests == model_requests(arch) + 2 * image_requests(arch, 32, B, reveal="metrics") + auc_requests(2 * B, 3)
    check_against_the_kept_rows(model, ctx, M, U, want, labels, B)
    out = str(tmp_path / "metrics")
    three_roles(f"metrics-{norm}", PF, SEED, out)
    for j in range(2):
        sM, sU = torch.load(f"{out}.{j}")
        assert np.array_equal(sM.numpy(), host(M)) and np.array_equal(sU.numpy(), host(U)), (j, sM.tolist(), sU.tolist())
    assert not os.path.exists(out + ".dealer")


# ---- 5. CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_evaluate_metrics(cuda, tmp_path):
    """inference.py --evaluate --encrypted_inference --reveal metrics --precision_fractional 3 on `synthetic` (four images,
    one pass, every class among the seeded labels) prints the validation table with a numeric AUC and one JSON line with
    "roc_auc": the score scikit-learn gives on the logits a --reveal logits run opens under the same debug seed (one pass:
    the same logit shares), next to the confusion form's matrix and MCC; --reveal metrics without --evaluate exits with a
    message that says why."""
    import inference

    sd, _ = network_case("batch")
    ckpt = write_checkpoint(tmp_path / "bn.pt", sd)
    dump = str(tmp_path / "logits.pt")
    run = lambda extra, dump=None: run_inference(ckpt, 4, 3, ["--encrypted_inference"] + extra, batch_size=4, dump=dump)
    results = json_line

    labels = inference.synthetic_labels(4, 3)
    assert set(labels.tolist()) == {0, 1, 2}
    r = run(["--evaluate", "--reveal", "metrics"])
    got = results(r)["Evaluation"]
    assert sorted(got) == ["confusion_matrix", "mcc", "n", "roc_auc"] and got["n"] == 4
    plain = results(run(["--evaluate", "--reveal", "logits"], dump))["Evaluation"]
    assert sorted(plain) == ["confusion_matrix", "mcc", "n"]
    assert got["confusion_matrix"] == plain["confusion_matrix"] and got["mcc"] == plain["mcc"]
    want = inference.roc_auc_of(labels, torch.load(dump))
    print("roc_auc", got["roc_auc"], "scikit-learn on the opened logits", want)
    assert isinstance(got["roc_auc"], float) and abs(got["roc_auc"] - want) <= 1e-12
    assert "AUC ROC score" in r.stdout and "n/a" not in r.stdout and "{:.3f}".format(got["roc_auc"]) in r.stdout
    assert "Inference Results" not in r.stdout
    r = run(["--reveal", "metrics"])
    assert r.returncode != 0 and "--evaluate" in r.stderr and "labels" in r.stderr and not r.stdout.strip()
