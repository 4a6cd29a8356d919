"""GPU: encrypted inference that opens the predicted class only (reveal="class").  The secret-shared argmax is defined in
tests/secure_argmax_nets.py from the oracle's own methods; the fused step kernel is held bit-exact to the step-by-step chain,
`SecureContext.argmax` to that definition on the same dealer tape, and whole networks -- eager, graphed, batched with a ragged
last pass, three ranks, the CLI -- to the first-index argmax of the encoded logits the logits form reconstructs from the very
same shares; a recording opener shows what a pass opens.
(No MI355X run of this file has been made yet; the kernel's index arithmetic and the fused walk have so far been checked against
oracle_argmax in a host model only.)"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import secure_oracle as S  # noqa: E402
from primia_amd import secure  # noqa: E402
from primia_amd._lib import PrimiaError, call  # noqa: E402
from primia_amd.secure import (Dealer, GraphedSecureInference, LocalOpener, PipelinedSecureInference,  # noqa: E402
                               PreloadedDealer, SecureContext, SecureResNet18, architecture_of, image_requests,
                               model_requests)
from tests.secure_argmax_nets import first_argmax, oracle_argmax, spread  # noqa: E402
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet  # noqa: E402
from tests.secure_common import (context, guarded, guards_intact, host, json_line, padded, run_inference,  # noqa: E402
                                 shares_equal, six, three_roles, wrapping_shares, write_checkpoint)
from tests.three_role_cases import THREE_RANK_BATCH, network_case  # noqa: E402

I64 = torch.int64
SHAPES = [(1, 2), (3, 5), (70, 3)]      # one thread pair, an odd count inside a wavefront, a tail past one wavefront (140 threads)


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_argmax_step_kernel_equals_the_chain(cuda, shape):
    """primia_argmax_combine_local on shares near +-2^63 against the step-by-step chain (two stacks, primia_beaver_mask, two
    opens, primia_beaver_combine_mul, two adds) on the same triple: both shares of V and of I, bit for bit, for every column
    k of the logits; nothing is written outside V and I, and the inputs are left alone."""
    B, C = shape
    rng = np.random.default_rng(B * 10 + C)
    dev = lambda a: torch.from_numpy(a).to(cuda)
    L = [dev(wrapping_shares(rng, (B, C))) for _ in range(2)]
    bit, K, V0, I0 = ([dev(wrapping_shares(rng, (B,))) for _ in range(2)] for _ in range(4))
    dealer = Dealer(cuda, seed=41)
    t = dealer.triple("mul", (B, 2), (B, 2))
    for k in range(C):
        ctx = SecureContext(PreloadedDealer([t], cuda), 10, 3)
        ctx.local_fused = False
        Lk = [L[j][:, k].contiguous() for j in range(2)]
        R = ctx.beaver_mul(ctx._stack2(bit, bit, B), ctx._stack2(ctx.sub(Lk, V0), ctx.sub(K, I0), B))
        assert tuple(R[0].shape) == (B, 2) and ctx.dealer.pos == 1
        want_v = [V0[j] + R[j][:, 0] for j in range(2)]
        want_i = [I0[j] + R[j][:, 1] for j in range(2)]
        bufs = [guarded(B, cuda) for _ in range(4)]
        for (_, view), src in zip(bufs, (V0[0], V0[1], I0[0], I0[1])):
            view.copy_(src)
        keep = [x.clone() for x in (*L, *bit, *K, *six(t))]
        call("primia_argmax_combine_local", bit[0], bit[1], L[0], L[1], C, k, K[0], K[1], *six(t), bufs[0][1], bufs[1][1],
             bufs[2][1], bufs[3][1], B)
        assert all(guards_intact(b, B) for b, _ in bufs)
        assert all(torch.equal(a, b) for a, b in zip(keep, (*L, *bit, *K, *six(t))))
        for j in range(2):
            assert torch.equal(bufs[j][1], want_v[j]) and torch.equal(bufs[2 + j][1], want_i[j]), (k, j)
        # ... and it is the Beaver identity: V + bit * (L_k - V), I + bit * (K - I) in the ring
        opened = lambda s: host(s[0]).view(np.uint64) + host(s[1]).view(np.uint64)
        b_, v_, i_, k_, l_ = opened(bit), opened(V0), opened(I0), opened(K), opened(Lk)
        assert np.array_equal(opened([bufs[0][1], bufs[1][1]]), v_ + b_ * (l_ - v_))
        assert np.array_equal(opened([bufs[2][1], bufs[3][1]]), i_ + b_ * (k_ - i_))


def test_argmax_step_kernel_refuses_invalid_arguments(cuda):
    B, C = 4, 3
    z = lambda *s: torch.zeros(*s, dtype=I64, device=cuda)
    good = [z(B), z(B), z(B, C), z(B, C), C, 1, z(B), z(B)] + [z(B, 2) for _ in range(6)] + [z(B), z(B), z(B), z(B), B]
    call("primia_argmax_combine_local", *good)
    for i in [0, 1, 2, 3, 6, 7] + list(range(8, 18)):
        bad = list(good)
        bad[i] = None
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_argmax_combine_local", *bad)
    for i, v in ((4, 0), (5, -1), (5, C), (18, 0), (18, -2)):      # width, column below / past the row, B
        bad = list(good)
        bad[i] = v
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_argmax_combine_local", *bad)
    for i, j in ((14, 15), (16, 17), (14, 16), (14, 0), (16, 6), (15, 9)):      # V / I aliasing each other or an input
        bad = list(good)
        bad[i] = bad[j]
        with pytest.raises(PrimiaError, match="PRIMIA_ERR_ARG"):
            call("primia_argmax_combine_local", *bad)


# ---- 2. the layer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pf", [3, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_context_argmax_equals_the_definition(cuda, shape, pf):
    """SecureContext.argmax, fused and step by step, against oracle_argmax on the replayed dealer log (consumed exactly):
    every share of I and of V, bit for bit.  pf = 3: logits with ties whose differences are far below 2^31 (asserted) -- the
    opened indices are np.argmax's; pf = 16: the differences exceed 2^32 and the result is the same deterministic function of
    the wrapped values on both sides."""
    B, C = shape
    gen = torch.Generator().manual_seed(B * 100 + C * 10 + pf)
    x = (torch.randn(B, C, generator=gen) * 3).round(decimals=1)      # one decimal: ties among 70 x 3 values, exact at pf = 3
    if B > 1:
        x[0, :] = x[0, 0]                                              # an all-equal row
        x[1, C - 1] = x[1].max()                                       # a tie with the last column
    outs = []
    for fused in (True, False):
        dealer, ctx = context(cuda, 70 + pf, pf, fused)
        dealer.requests = []
        xs = ctx.share(ctx.encode(x.to(cuda)))
        n0 = len(dealer.requests)
        I, V = ctx.argmax(xs, values=True)
        assert dealer.requests[n0:] == secure.argmax_requests(B, C)
        assert ctx.stats == {"beaver_mul": C - 1, "beaver_matmul": 0, "dif_evals": B * (C - 1)}
        assert tuple(I[0].shape) == (B,) and I[0].dtype == I64
        outs.append((I, V))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    octx = S.OracleContext(S.ReplayDealer(dealer.log), 10, pf)
    q = S.fix_encode(x.numpy(), 10, pf)
    oI, oV = oracle_argmax(octx, octx.share(q))
    assert octx.dealer.pos == len(dealer.log)
    assert shares_equal(outs[0][0], oI) and shares_equal(outs[0][1], oV)
    if pf == 3:
        assert spread(q) < 2 ** 31 and spread(q) < 100_000
        got = host(ctx.reconstruct(outs[0][0]))
        assert np.array_equal(got, first_argmax(q)), (got.tolist(), first_argmax(q).tolist())
        assert np.array_equal(host(ctx.reconstruct(outs[0][1])), q.max(axis=1))
        assert (B == 1 or got[0] == 0) and (B < 70 or len(set(got.tolist())) == C)
    else:
        assert spread(q) > 2 ** 32


# ---- 3. whole networks ------------------------------------------------------------------------------------------------------
PF, SEED = 3, 83


def logits_form_classes(cuda, sd, tape, chunk):
    """The logits form (SecureResNet18 as it was: reveal="logits") on the primitives in `tape`, of which it consumes a
    prefix: the ENCODED logits it reconstructs, their spread asserted below 2^31, and their first-index argmax."""
    pre = PreloadedDealer(tape, cuda)
    ctx = SecureContext(pre, 10, PF)
    model = SecureResNet18(ctx, sd, 32)
    assert model.reveal == "logits"
    q = host(ctx.reconstruct(model.forward_shares(ctx.share(ctx.encode(chunk), owner=1))))
    assert q.shape == (len(chunk), 3) and spread(q) < 2 ** 31
    return first_argmax(q), pre.pos


@pytest.fixture(scope="module", params=["batch", "group"])
def net(request, cuda):
    sd, images = network_case(request.param)
    return request.param, sd, images.to(cuda)


def test_eager_class_form_opens_the_argmax_of_the_logits(cuda, net):
    """One pass over all four images at pf = 3 under one debug dealer seed: the class form returns int64 [4], equal to the
    first-index argmax of the encoded logits of the logits form on the same primitives (its schedule is a strict prefix: the
    tail's primitives are what it leaves on the tape); at least two classes occur; the dealer was asked for
    image_requests(reveal="class"); and the logits form under the same seed returns what it returned before."""
    norm, sd, images = net
    dealer = Dealer(cuda, seed=SEED)
    dealer.requests, dealer.tape = [], []
    ctx = SecureContext(dealer, 10, PF)
    model = SecureResNet18(ctx, sd, 32, reveal="class")
    assert model.norm == norm
    got = model(images)
    arch = architecture_of(sd)
    assert dealer.requests == model_requests(arch) + image_requests(arch, 32, 4, reveal="class")
    assert got.dtype == I64 and tuple(got.shape) == (4,)
    want, used = logits_form_classes(cuda, sd, dealer.tape, images)
    assert len(dealer.tape) - used == 1 + 3 * 2
    print(norm, "classes", got.tolist())
    assert np.array_equal(host(got), want)
    assert len(set(got.tolist())) >= 2
    plain = SecureResNet18(SecureContext(Dealer(cuda, seed=SEED), 10, PF), sd, 32)(images)
    assert plain.dtype == torch.float32 and np.array_equal(host(plain).argmax(axis=1), want)


@pytest.mark.parametrize("B", [1, 3])
def test_graphed_class_form(cuda, net, B):
    """GraphedSecureInference(reveal="class"): the tail is captured, the static output is an int64 [B] buffer and rows(n) a
    view of it.  B = 1: two replays on different images, a refill between them; B = 3: a full pass and a ragged one (one
    image, two all-zero rows dropped).  After every replay the logits form on the primitives the buffers hold gives encoded
    logits whose argmax is the replayed output, padding rows included."""
    norm, sd, images = net
    g = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=PF, seed=SEED + B, batch=B, reveal="class")
    arch = architecture_of(sd)
    assert g.requests[g._n_model:] == image_requests(arch, 32, B, reveal="class")
    assert g.static_bytes == secure.serving_bytes(arch, 32, B, reveal="class") > secure.serving_bytes(arch, 32, B)
    assert g.out.dtype == I64 and tuple(g.out.shape) == (B,)
    seen = []
    for step, chunk in enumerate((images[0:B], images[B:B + 1] if B == 1 else images[3:4])):
        out = g(chunk, refill=step > 0)
        assert out.data_ptr() == g.out.data_ptr() and tuple(out.shape) == (len(chunk),)
        want, used = logits_form_classes(cuda, sd, g.tape, padded(chunk, B))
        assert len(g.tape) - used == 1 + 3 * 2
        assert np.array_equal(host(g.out), want), (step, g.out.tolist(), want.tolist())
        assert np.array_equal(host(g.rows(len(chunk))), want[:len(chunk)])
        seen += out.tolist()
    print(norm, B, "classes", seen)
    assert len(set(seen)) >= 2


def test_pipelined_passes_reveal_through(cuda):
    sd, images = network_case("batch")
    images = images.to(cuda)
    p = PipelinedSecureInference(sd, cuda, input_size=32, precision_fractional=PF, seed=SEED, batch=2, reveal="class")
    assert all(s.reveal == "class" for s in p.slots)
    got = p(images[:2])
    torch.cuda.synchronize()
    ref = GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=PF, seed=SEED, batch=2, reveal="class")
    assert got.dtype == I64 and torch.equal(got, ref(images[:2], refill=False))


def in_process_reference(cuda, sd, images, batch):
    """The class form in ONE process under the debug seed, pass by pass as the three ranks run it: per pass the encoded logits
    (reconstructed HERE, from the shares the tail walks over; the pass itself never opens them), their first-index argmax,
    and the classes the pass opens.  The dealer is held to the host-side schedule the dealer rank will follow."""
    dealer = Dealer(cuda, seed=SEED)
    dealer.requests = []
    ctx = SecureContext(dealer, 10, PF)
    model = SecureResNet18(ctx, sd, 32, reveal="class")
    want, got = [], []
    for i in range(0, len(images), batch):
        chunk = images[i:i + batch]
        L = model.forward_shares(ctx.share(ctx.encode(padded(chunk, batch)), owner=1))
        q = host(ctx.reconstruct(L))
        assert spread(q) < 2 ** 31
        want.append(first_argmax(q)[:len(chunk)])
        got.append(host(ctx.open_to(ctx.argmax(L)))[:len(chunk)])
    arch = architecture_of(sd)
    passes = len(want)
    assert dealer.requests == model_requests(arch) + passes * image_requests(arch, 32, batch, reveal="class")
    return np.concatenate(want), np.concatenate(got)


def test_three_ranks_reveal_the_class_to_the_data_owner_only(cuda, net, tmp_path):
    """model_owner / data_owner / crypto_provider as three processes on one GPU over gloo, four images at three per pass (a
    ragged last pass): party 1 ends up with the first-index argmax of the encoded logits, party 0 returns None (asserted in
    its process) and writes nothing, the dealer follows the extended schedule (a mismatch would stall: the worker's limit)."""
    norm, sd, images = net
    want, got = in_process_reference(cuda, sd, images, THREE_RANK_BATCH)
    assert np.array_equal(got, want) and len(set(want.tolist())) >= 2
    out = str(tmp_path / "classes")
    three_roles(f"class-{norm}", PF, SEED, out)
    assert not os.path.exists(out + ".0")
    seen = torch.load(out + ".1")
    assert seen.dtype == I64 and np.array_equal(seen.numpy(), want), (seen.tolist(), want.tolist())


# ---- 4. what is opened ------------------------------------------------------------------------------------------------------
class RecordingOpener:
    """Records the shape of everything opened (not a LocalOpener: the context then runs the step-by-step chain, whose opens
    all go through here or through primia_fss_open)."""

    def __init__(self, events):
        self.events, self.inner = events, LocalOpener()

    def open(self, shares):
        self.events.append(("open", tuple(shares[0].shape)))
        return self.inner.open(shares)


def opened_by(cuda, monkeypatch, sd, images, reveal):
    events, recon = [], []
    real = secure.call

    def recording_call(name, *args, **kw):
        if name == "primia_fss_open":
            events.append(("fss", int(args[3])))
        return real(name, *args, **kw)

    with monkeypatch.context() as m:
        m.setattr(secure, "call", recording_call)
        ctx = SecureContext(Dealer(cuda, seed=SEED), 10, PF, opener=RecordingOpener(events))

        def reconstruct(x):
            events.append(("reconstruct", tuple(x[0].shape)))
            recon.append(ctx.opener.inner.open(x))
            return recon[-1]

        ctx.reconstruct = reconstruct
        out = SecureResNet18(ctx, sd, 16, MINI_BLOCKS, reveal=reveal)(images)
    return events, out, recon


def test_a_class_pass_opens_the_logits_pass_plus_the_walk_and_never_the_logits(cuda, monkeypatch):
    """The step-by-step chain of the mini network on two 16 x 16 images, every open recorded: the class form opens exactly
    what the logits form opens up to its final reconstruction, then per class walked one masked FSS input of B elements and
    one (delta, epsilon) pair of shape [B, 2], and reconstructs ONE tensor, of shape [B]; no [B, C] tensor."""
    B, C = 2, 3
    gen = torch.Generator().manual_seed(21)
    sd = mini_resnet(gen)
    images = torch.randn(B, 3, 16, 16, generator=gen).to(cuda)
    ev_l, _, recon_l = opened_by(cuda, monkeypatch, sd, images, "logits")
    ev_c, out_c, recon_c = opened_by(cuda, monkeypatch, sd, images, "class")
    assert ev_l[-1] == ("reconstruct", (B, C)) and sum(1 for e in ev_l if e[0] == "reconstruct") == 1
    walk = (C - 1) * [("fss", B), ("open", (B, 2)), ("open", (B, 2))]
    assert ev_c == ev_l[:-1] + walk + [("reconstruct", (B,))]
    assert not any(e[0] != "fss" and e[1] == (B, C) for e in ev_c[len(ev_l) - 1:])
    assert sum(1 for e in ev_c if e[0] == "reconstruct") == 1
    q = host(recon_l[0])      # the encoded logits the logits form opened: the same shares, the same dealer stream up to here
    assert len(recon_c) == 1 and out_c is recon_c[0] and spread(q) < 2 ** 31
    assert np.array_equal(host(out_c), first_argmax(q))


# ---- 5. CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_reveal_class(cuda, tmp_path):
    """inference.py --reveal class prints the JSON of --reveal logits on the same checkpoint and debug
    seed at --precision_fractional 3 (one pass over the three images); --hip_graph --batch_size 2 serves the same images; with PRIMIA_DUMP_LOGITS set it refuses, saying
    that the logits are never opened, and writes nothing."""
    sd, _ = network_case("batch")
    ckpt = write_checkpoint(tmp_path / "bn.pt", sd)
    # by default one pass over the three images: both forms then walk the same dealer stream, and the logits under the argmax
    # are the same shares, bit for bit
    run = lambda extra, batch_size=3, dump=None: run_inference(ckpt, 3, 3, ["--encrypted_inference"] + extra, batch_size, dump)
    results = json_line

    base = results(run(["--reveal", "logits"]))
    assert sorted(base["Inference Results"]) == ["0", "1", "2"]
    assert results(run(["--reveal", "class"])) == base
    graphed = results(run(["--reveal", "class", "--hip_graph"], 2))["Inference Results"]      # (other primitives
    assert graphed.keys() == base["Inference Results"].keys() and set(graphed.values()) <= {0, 1, 2}            # after a refill)
    dump = str(tmp_path / "logits.pt")
    r = run(["--reveal", "class"], dump=dump)
    assert r.returncode != 0 and "never opened" in r.stderr and not os.path.exists(dump)
