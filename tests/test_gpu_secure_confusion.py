"""GPU: an encrypted evaluation that opens the confusion matrix only (reveal="confusion").  The tail is defined in
tests/secure_confusion_nets.py from the oracle's own methods; `SecureContext.eq` and `SecureContext.confusion`, fused and step
by step, are held bit for bit to that definition on the dealer's log, whole networks -- eager, graphed, three roles, the CLI --
to the counts of the float64 plaintext classes against chosen labels, and a recording opener shows what an evaluation opens."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import secure_oracle as S  # noqa: E402
from primia_amd import secure  # noqa: E402
from primia_amd._lib import PrimiaError, call  # noqa: E402
from primia_amd.secure import (Dealer, GraphedSecureInference, LocalOpener, PreloadedDealer, SecureContext,  # noqa: E402
                               SecureResNet18, architecture_of, confusion_requests, image_requests, model_requests)
from tests.secure_argmax_nets import CRAFTED, first_argmax  # noqa: E402
from tests.secure_common import (chunks, context, guarded, guards_intact, host, json_line, padded, run_inference,  # noqa: E402
                                 shares_equal, six, three_roles, wrapping_shares, write_checkpoint)
from tests.secure_confusion_nets import (GPU_TAIL_SEEDS, ConfusionReplayDealer, chosen_labels, crafted_cases,  # noqa: E402
                                         numpy_confusion, onehot, oracle_confusion, oracle_eq, plaintext_classes, zero_matrix)
from tests.three_role_cases import THREE_RANK_BATCH, network_case  # noqa: E402

I64 = torch.int64
PF, SEED = 3, 83
ids = lambda s: "x".join(map(str, s))


def dev_pair(arrs, cuda):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrs]


# ---- 1. equality ------------------------------------------------------------------------------------------------------------
# one thread, an odd count inside a wavefront, a tail past one block (300 = 256 + 44), and a column range of a wider matrix
@pytest.mark.parametrize("case", [(1, 1, None), (3, 5, None), (60, 5, None), (7, 3, (8, 2, 6, 1))], ids=str)
def test_context_eq_equals_the_definition(cuda, case):
    """SecureContext.eq, in one launch and step by step, against oracle_eq on the dealer's log: both output shares, bit for
    bit, on shares near +-2^63 of small integers of which about a third are equal, one pair 2^32 apart (equal to the layer);
    the reconstructed bits are the truth mod 2^32.  With column-range operands both forms read columns [start, start + len)
    of [rows, w] matrices."""
    rows, length, cols = case
    w1, s1, w2, s2 = cols or (length, 0, length, 0)
    rng = np.random.default_rng(rows * 10 + length)
    v1 = rng.integers(0, 3, size=(rows, w1)).astype(np.int64)
    v2 = rng.integers(0, 3, size=(rows, w2)).astype(np.int64)
    v1[0, s1] = v2[0, s2] + 2 ** 32
    x1s, x2s = [], []
    for v, xs in ((v1, x1s), (v2, x2s)):
        r = wrapping_shares(rng, v.shape)
        xs += [r, (v.view(np.uint64) - r.view(np.uint64)).view(np.int64)]
    want = ((v1[:, s1:s1 + length] - v2[:, s2:s2 + length]) % 2 ** 32 == 0).astype(np.int64)
    assert 0 < want.sum() and (want.size == 1 or want.sum() < want.size)
    outs = []
    for fused in (True, False):
        dealer, ctx = context(cuda, 91, PF, fused)
        dealer.requests = []
        a, b = dev_pair(x1s, cuda), dev_pair(x2s, cuda)
        if cols:
            out = ctx.eq(a, b, (w1, s1), (w2, s2), length, shape=(rows, length))
        else:
            out = ctx.eq(a, b)
        assert dealer.requests == [("dpf_keys", (rows * length,), {})]
        assert tuple(out[0].shape) == (rows, length) and out[0].dtype == I64
        assert ctx.stats["dpf_evals"] == rows * length
        outs.append(out)
        assert np.array_equal(host(ctx.reconstruct(out)), want)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    octx = S.OracleContext(ConfusionReplayDealer(dealer.log), 10, PF)
    sl = lambda xs, s: [np.ascontiguousarray(x[:, s:s + length]) for x in xs]
    ref = oracle_eq(octx, sl(x1s, s1), sl(x2s, s2))
    assert octx.dealer.pos == len(dealer.log) == 1
    assert shares_equal(outs[0], ref)


def test_dpf_eval_local_refuses_invalid_arguments(cuda):
    n = 6
    d = Dealer(cuda, seed=5)
    k0, k1 = d.dpf_keys(n)
    z = lambda: torch.zeros(n, dtype=I64, device=cuda)
    good = [z(), z(), 1, 0, z(), z(), 1, 0, 1, k0["alpha"], k1["alpha"], k0["s0"], k1["s0"], k0["bits"], k0["cw_s"], k0["cw_n"],
            z(), z(), n]
    call("primia_dpf_eval_local", *good)
    for i in [0, 1, 4, 5, 9, 10, 11, 12, 13, 14, 15, 16, 17]:      # (both operands are required, each share of them)
        bad = list(good)
        bad[i] = None
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_dpf_eval_local", *bad)
    for i, v in ((8, 0), (8, 4), (6, 0), (7, 1), (7, -1), (2, 0), (3, 1)):      # len, widths and columns past the row
        bad = list(good)
        bad[i] = v
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_dpf_eval_local", *bad)
    for pair in ((0, 1), (16, 17)):      # x1 absent as a pair (the DIF form's shares of zero: not taken here); one output buffer
        bad = list(good)
        bad[pair[0]], bad[pair[1]] = (None, None) if pair == (0, 1) else (bad[16], bad[16])
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_dpf_eval_local", *bad)


# ---- 2. the combine kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2), (3, 5), (70, 3), (5, 16)], ids=ids)      # 8 .. 512 threads; C = 16 is the most
def test_confusion_combine_kernel_equals_the_chain(cuda, shape):
    """primia_confusion_combine_local on shares near +-2^63 against the step-by-step chain (a transposed copy of Y,
    primia_beaver_mask, two opens, primia_beaver_combine_matmul, an add) on the same triple: both shares of M, bit for bit,
    added to what M held; nothing is written outside M and the inputs are left alone."""
    B, C = shape
    rng = np.random.default_rng(B * 100 + C)
    dev = lambda a: torch.from_numpy(a).to(cuda)
    Y, P, M0 = ([dev(wrapping_shares(rng, s)) for _ in range(2)] for s in ((B, C), (B, C), (C, C)))
    t = Dealer(cuda, seed=43).triple("matmul", (C, B), (B, C))
    ctx = SecureContext(PreloadedDealer([t], cuda), 10, PF)
    ctx.local_fused = False
    Mc = ctx.beaver_matmul([Y[j].t().contiguous() for j in range(2)], P)
    want = [M0[j] + Mc[j] for j in range(2)]
    bufs = [guarded(C * C, cuda) for _ in range(2)]
    for (_, view), src in zip(bufs, M0):
        view.copy_(src.reshape(-1))
    keep = [x.clone() for x in (*Y, *P, *six(t))]
    call("primia_confusion_combine_local", Y[0], Y[1], P[0], P[1], *six(t), bufs[0][1], bufs[1][1], B, C)
    assert all(guards_intact(b, C * C) for b, _ in bufs)
    assert all(torch.equal(a, b) for a, b in zip(keep, (*Y, *P, *six(t))))
    for j in range(2):
        assert torch.equal(bufs[j][1].view(C, C), want[j]), j


def test_confusion_combine_kernel_refuses_invalid_arguments(cuda):
    B, C = 4, 3
    z = lambda *s: torch.zeros(*s, dtype=I64, device=cuda)
    good = [z(B, C), z(B, C), z(B, C), z(B, C), z(C, B), z(B, C), z(C, C), z(C, B), z(B, C), z(C, C), z(C, C), z(C, C), B, C]
    call("primia_confusion_combine_local", *good)
    for i in range(12):
        bad = list(good)
        bad[i] = None
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_confusion_combine_local", *bad)
    for i, v in ((12, 0), (12, -1), (13, 0), (13, 17)):      # B, and C outside 1 .. 16
        bad = list(good)
        bad[i] = v
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_confusion_combine_local", *bad)
    for i, j in ((10, 11), (10, 6), (11, 9), (10, 0)):      # M aliasing itself or an input
        bad = list(good)
        bad[i] = bad[j]
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_confusion_combine_local", *bad)


# ---- 3. the tail ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(CRAFTED), ids=ids)
def test_context_confusion_equals_the_definition(cuda, shape):
    """All crafted cases of a shape as the passes of one evaluation, fused and step by step, against
    oracle_confusion on the replayed dealer log (consumed exactly): every share of P, of each pass's Mc (the change of the
    accumulator) and of M, bit for bit; the passes accumulate, the padding rows add nothing, M opens to numpy's counts
    and sums to the number of labelled rows; the requests are the tail's."""
    B, C = shape
    cases = crafted_cases(shape)
    runs = []
    for fused in (True, False):
        dealer, ctx = context(cuda, GPU_TAIL_SEEDS[shape], PF, fused)
        dealer.requests = []
        acc = [torch.zeros(C, C, dtype=I64).to(cuda) for _ in range(2)]
        steps = []
        for q, _, y, _ in cases:
            xs = ctx.share(torch.from_numpy(q).to(cuda))
            n0 = len(dealer.requests)
            before = [a.clone() for a in acc]
            P = ctx.confusion(xs, torch.from_numpy(y).to(cuda), acc)
            assert dealer.requests[n0:] == secure.argmax_requests(B, C) + confusion_requests(B, C)
            steps.append((P, [acc[j] - before[j] for j in range(2)], [a.clone() for a in acc]))
        assert ctx.stats["dpf_evals"] == len(cases) * B * C and ctx.stats["beaver_matmul"] == len(cases)
        runs.append(steps)
    for a, b in zip(*runs):
        for x, y_ in zip(a, b):
            assert torch.equal(x[0], y_[0]) and torch.equal(x[1], y_[1])
    octx = S.OracleContext(ConfusionReplayDealer(dealer.log), 10, PF)
    M, want = zero_matrix(C), np.zeros((C, C), np.int64)
    for (q, labels, y, counts), (P, Mc, Macc) in zip(cases, runs[0]):
        oP, oMc, M = oracle_confusion(octx, octx.share(q), y, M)
        assert shares_equal(P, oP) and shares_equal(Mc, oMc) and shares_equal(Macc, M)
        assert np.array_equal(host(ctx.reconstruct(P)), onehot(first_argmax(q), C))
        want += counts
        assert np.array_equal(host(ctx.reconstruct(Macc)), want)
    assert octx.dealer.pos == len(dealer.log)
    assert any((c[1] < 0).any() for c in cases) and len(cases) >= 2
    assert int(want.sum()) == sum(int((c[1] >= 0).sum()) for c in cases)


# ---- 4. whole networks ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["batch", "group"])
def net(request, cuda):
    """(norm, state dict, images on the device, labels, the counts of the float64 plaintext classes against the labels)."""
    sd, images = network_case(request.param)
    classes = plaintext_classes(request.param, sd, images, PF)
    labels = chosen_labels(classes)
    want = numpy_confusion(labels, classes, 3)
    assert np.trace(want) > 0 and want.sum() - np.trace(want) > 0 and want.sum() == 4
    return request.param, sd, images.to(cuda), torch.from_numpy(labels), want


def test_eager_and_graphed_evaluation(cuda, net):
    """Four images at three per pass (the second pass padded with two all-zero images): the graphed form, and the eager form
    on the primitives its buffers hold, end every pass with identical shares of the accumulator; the opened matrix is the
    confusion of the float64 plaintext classes against the labels; the graph's requests are image_requests(reveal=
    "confusion"); a pass returns nothing; begin() starts over."""
    norm, sd, images, labels, want = net
    B = THREE_RANK_BATCH
    g = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=PF, seed=SEED, batch=B, reveal="confusion")
    arch = architecture_of(sd)
    assert g.requests[g._n_model:] == image_requests(arch, 32, B, reveal="confusion")
    assert g.static_bytes == secure.serving_bytes(arch, 32, B, reveal="confusion") > secure.serving_bytes(arch, 32, B, reveal="class")
    assert g.out is None and tuple(g.labels.shape) == (B, 3) and g.labels.dtype == I64
    acc = g._model.acc
    assert not acc[0].any() and not acc[1].any()      # the constructor's warm-up passes were wiped
    ptrs = [a.data_ptr() for a in acc]
    prev = [a.clone() for a in acc]
    for step, (chunk, lab) in enumerate(chunks(images, labels, THREE_RANK_BATCH)):
        assert g(chunk, refill=step > 0, labels=lab) is None
        assert np.array_equal(host(g.labels), onehot(lab.numpy().tolist() + [-1] * (B - len(lab)), 3))
        # the eager form on the very primitives the buffers hold: a model of its own, whose accumulator starts at zero
        pre = PreloadedDealer(g.tape, cuda)
        ctx = SecureContext(pre, 10, PF)
        model = SecureResNet18(ctx, sd, 32, reveal="confusion")
        model.begin()
        assert model(padded(chunk, B), labels=lab) is None and pre.pos == len(g.tape)
        for j in range(2):
            assert torch.equal(acc[j], prev[j] + model.acc[j]), (step, j)
        prev = [a.clone() for a in acc]
    assert [a.data_ptr() for a in acc] == ptrs
    M = g.finish()
    print(norm, "confusion", M.tolist())
    assert M.dtype == I64 and np.array_equal(host(M), want)
    g.begin()
    assert not host(g.finish()).any()


class RecordingOpener:
    """Records the shape of everything opened (not a LocalOpener: the context then runs the step-by-step chain, whose opens
    all go through here or through primia_fss_open)."""

    def __init__(self, events):
        self.events, self.inner = events, LocalOpener()

    def open(self, shares):
        self.events.append(("open", tuple(shares[0].shape)))
        return self.inner.open(shares)


def test_eager_evaluation_requests_and_opens(cuda, net, monkeypatch):
    """The eager form under a debug dealer seed with a recording opener, every open counted: the dealer was asked for
    model_requests + one image_requests(reveal="confusion") per pass; every pass ends with the walk's opens, ONE masked
    equality input of B * C elements and the (delta, epsilon) pair of the [C, B] x [B, C] product; the only value ever
    reconstructed is M, once, after the last pass -- it is the expected matrix; and the opens before each tail are those of
    the logits form without its final reconstruction."""
    norm, sd, images, labels, want = net
    B, C = THREE_RANK_BATCH, 3
    events = []
    real = secure.call

    def recording_call(name, *args, **kw):
        if name == "primia_fss_open":
            events.append(("fss", int(args[3])))
        return real(name, *args, **kw)

    def run(reveal):
        del events[:]
        dealer = Dealer(cuda, seed=SEED)
        dealer.requests = []
        ctx = SecureContext(dealer, 10, PF, opener=RecordingOpener(events))
        inner = ctx.opener.inner

        def reconstruct(x):
            events.append(("reconstruct", tuple(x[0].shape)))
            return inner.open(x)

        ctx.reconstruct = reconstruct
        model = SecureResNet18(ctx, sd, 32, reveal=reveal)
        marks = []
        if reveal == "confusion":
            model.begin()
        for chunk, lab in chunks(images, labels, THREE_RANK_BATCH):
            model(padded(chunk, B), **({"labels": lab} if reveal == "confusion" else {}))
            marks.append(len(events))
        out = model.finish() if reveal == "confusion" else None
        return list(events), marks, dealer.requests, out

    with monkeypatch.context() as m:
        m.setattr(secure, "call", recording_call)
        ev_l, marks_l, _, _ = run("logits")
        ev_c, marks_c, requests, M = run("confusion")
    arch = architecture_of(sd)
    assert requests == model_requests(arch) + 2 * image_requests(arch, 32, B, reveal="confusion")
    walk = (C - 1) * [("fss", B), ("open", (B, 2)), ("open", (B, 2))]
    tail = walk + [("fss", B * C), ("open", (C, B)), ("open", (B, C))]
    first_l = ev_l[:marks_l[0]]
    assert first_l[-1] == ("reconstruct", (B, C))
    per_pass = first_l[:-1] + tail
    assert ev_c[:marks_c[0]] == per_pass and ev_c[marks_c[0]:marks_c[1]] == per_pass
    assert ev_c[marks_c[1]:] == [("reconstruct", (C, C))]
    assert [e for e in ev_c if e[0] == "reconstruct"] == [("reconstruct", (C, C))]
    assert np.array_equal(host(M), want)


# ---- 5. three roles ---------------------------------------------------------------------------------------------------------
def test_three_roles_both_parties_hold_the_matrix(cuda, net, tmp_path):
    """model_owner / data_owner / crypto_provider as three processes on one GPU over gloo, four images at three per pass,
    each process under its own time limit; every exit status is checked and after a failure nothing further is started.
    Both parties hold the matrix of the in-process evaluation under the same debug seed -- the expected counts -- and the
    dealer, which followed the extended schedule, holds nothing (asserted in its process)."""
    norm, sd, images, labels, want = net
    dealer = Dealer(cuda, seed=SEED)
    dealer.requests = []
    model = SecureResNet18(SecureContext(dealer, 10, PF), sd, 32, reveal="confusion")
    model.begin()
    for chunk, lab in chunks(images, labels, THREE_RANK_BATCH):
        model(padded(chunk, THREE_RANK_BATCH), labels=lab)
    arch = architecture_of(sd)
    assert dealer.requests == model_requests(arch) + 2 * image_requests(arch, 32, THREE_RANK_BATCH, reveal="confusion")
    in_process = host(model.finish())
    assert np.array_equal(in_process, want)
    out = str(tmp_path / "matrix")
    three_roles(f"confusion-{norm}", PF, SEED, out)
    for j in range(2):
        seen = torch.load(f"{out}.{j}")
        assert seen.dtype == I64 and np.array_equal(seen.numpy(), in_process), (j, seen.tolist())
    assert not os.path.exists(out + ".dealer")


# ---- 6. CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_evaluate(cuda, tmp_path):
    """inference.py --evaluate --encrypted_inference --reveal confusion --precision_fractional 3 on `synthetic` prints the
    validation table and one JSON line whose matrix is the one built from the predictions of a --reveal class run (same
    checkpoint, same debug seed, one pass over the three images: the same logit shares) and the seeded labels, with that
    matrix's MCC and no ROC AUC; --evaluate --reveal class prints the same matrix; --reveal confusion without --evaluate
    exits with a message that says why."""
    import inference
    from primia_amd.torchlib_compat import confusion_mcc

    sd, _ = network_case("batch")
    ckpt = write_checkpoint(tmp_path / "bn.pt", sd)
    run = lambda extra: run_inference(ckpt, 3, 3, ["--encrypted_inference"] + extra, batch_size=3)
    results = json_line
    classes = results(run(["--reveal", "class"]))["Inference Results"]
    labels = inference.synthetic_labels(3, 3)
    want = inference.confusion_of(labels, [classes[str(i)] for i in range(3)], 3)
    r = run(["--evaluate", "--reveal", "confusion"])
    got = results(r)
    assert list(got) == ["Evaluation"] and sorted(got["Evaluation"]) == ["confusion_matrix", "mcc", "n"]
    assert got["Evaluation"]["confusion_matrix"] == want.tolist() and got["Evaluation"]["n"] == 3
    assert got["Evaluation"]["mcc"] == confusion_mcc(want.numpy())
    assert "matthews coeff" in r.stdout and "n/a" in r.stdout and "Inference Results" not in r.stdout
    assert results(run(["--evaluate", "--reveal", "class"])) == got
    r = run(["--reveal", "confusion"])
    assert r.returncode != 0 and "--evaluate" in r.stderr and "labels" in r.stderr and not r.stdout.strip()
