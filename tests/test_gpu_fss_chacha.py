"""GPU: FSS keys from the ChaCha20 PRG (csrc/fss_chacha.hip) -- the `*_prg` entry points against
tests/fss_chacha_ref.py bit for bit, the two-party forms against the step-by-step chain, and fss_prg="chacha" through the
network, the serving graph and inference.py against the default PRG under the same dealer seed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from primia_amd._lib import call  # noqa: E402
from primia_amd.secure import (Dealer, GraphedSecureInference, PreloadedDealer, ProtocolForm, SecureContext,  # noqa: E402
                               SecureResNet18, dif_key_fields, dpf_key_fields)
from tests import fss_chacha_ref as R  # noqa: E402
from tests.fss_wide_ref import packed_bits  # noqa: E402
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet  # noqa: E402
from tests.secure_common import json_line, run_inference, write_checkpoint  # noqa: E402
from tests.test_gpu_fss_wide import Guarded, dev  # noqa: E402
from tests.three_role_cases import wide_net  # noqa: E402

I64 = np.int64
CHACHA = 1


def keygen(cuda, kind, alpha, s0, n, bits):
    """The dealer's entry point into guarded buffers -> (the key's fields as device views, what follows them in every call)."""
    fields = [Guarded(sh, dt, cuda) for sh, dt in (dif_key_fields(n, bits) if kind == "dif" else dpf_key_fields(n))]
    tail = (n, bits, CHACHA) if kind == "dif" else (n, CHACHA)
    call(f"primia_{kind}_keygen_prg", dev(alpha, cuda), dev(s0, cuda), *[f.view for f in fields], *tail)
    assert all(f.intact() for f in fields)
    return fields, tail


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("kind,bits", [("dif", 32), ("dif", 33), ("dif", 64), ("dpf", 32)])
def test_keygen_and_eval_equal_the_reference(cuda, kind, bits, n):
    alpha, x, s0 = R.inputs(bits, n, 50 * bits + n)
    fields, tail = keygen(cuda, kind, alpha, s0, n, bits)
    keys = R.keygen(kind, alpha, s0, bits)
    k = keys[0]
    if kind == "dif":
        want, xd = [packed_bits(k["bits"]), k["cw_sigma"], k["cw_s"], k["cw_leaf"]], dev(x, cuda)
    else:
        want, xd = [k["bits"][:, 0] | k["bits"][:, 1] << 1, k["cw_s"], k["cw_n"]], dev(x.astype(np.uint32).view(np.int32), cuda)
    for f, w in zip(fields, want):
        got = f.host()
        assert got.shape == w.shape and np.array_equal(got.view(w.dtype) if got.dtype == I64 else got, w)
    out = []
    for b in range(2):
        o = Guarded((n,), torch.int64, cuda)
        call(f"primia_{kind}_eval_prg", b, xd, dev(s0[b], cuda), *[f.view for f in fields], o.view, *tail)
        assert o.intact() and np.array_equal(o.host(), R.evaluate(kind, b, x, keys[b], bits)), b
        out.append(o.host())
    assert np.array_equal(out[0] + out[1], (x <= alpha if kind == "dif" else x == alpha).astype(I64))


@pytest.mark.parametrize("kind,bits", [("dif", 32), ("dif", 64), ("dpf", 32)])
def test_eval_local_equals_the_chain(cuda, kind, bits):
    """One primia_*_eval_local_prg launch against primia_fss_mask, the open and primia_*_eval_prg per party on the same keys
    (the same dealer seed): ReLU (x1 = NULL) and the max pool of a [1, 2, 8, 8] input (column ranges of the [32][9] unrolled
    windows) for the DIF, column ranges 0..3 against 4..7 of [16][8] matrices for the DPF."""
    gen = torch.Generator().manual_seed(bits)
    x = torch.randint(-1000, 1000, (1, 2, 8, 8), generator=gen)      # (a 32-bit comparison errs with probability |d| / 2^32)
    y = x.view(16, 8).roll(4, 1).clone()
    y[::2] += 1      # columns 4..7 of y equal columns 0..3 of x in every other row

    def run(fused):
        ctx = SecureContext(Dealer(cuda, seed=77, fss_bits=bits, fss_prg="chacha"), 10, 3)
        ctx.local_fused = fused
        xs = ctx.share(x.to(cuda))
        if kind == "dif":
            return ctx, [ctx.relu(xs), ctx.max_pool2d_3x3s2(xs)]
        xs = [t.view(16, 8) for t in xs]
        return ctx, [ctx.eq(xs, ctx.share(y.to(cuda)), cols1=(8, 0), cols2=(8, 4), length=4, shape=(16, 4))]

    (ctx, fused), (_, steps) = run(True), run(False)
    assert all(torch.equal(a[j], b[j]) for a, b in zip(fused, steps) for j in range(2))
    want = torch.relu(x) if kind == "dif" else (x.view(16, 8)[:, :4] == y[:, 4:]).long()
    assert torch.equal(ctx.reconstruct(fused[0]).cpu(), want)


PF, SEED = 6, 411
form_of = lambda prg, reveal: ProtocolForm(reveal=reveal, fss_bits=64, fss_prg=prg)


@pytest.fixture(scope="module")
def mini():
    gen = torch.Generator().manual_seed(410)
    return mini_resnet(gen), torch.randn(2, 3, 32, 32, generator=gen), torch.tensor([0, 2])


@pytest.mark.parametrize("reveal", ["logits", "class", "confusion"])
def test_network_under_chacha_equals_sha(cuda, mini, reveal):
    """ReLU, max pool, the argmax tail (class) and the equality tests of the confusion tail: what is opened is the same, eager
    and (logits, class) over three replays of the serving graph, which equal the eager pass on the primitives they hold."""
    sd, images, labels = mini[0], mini[1].to(cuda), mini[2]

    def eager(prg, dealer):
        ctx = SecureContext(dealer, 10, PF)
        model = SecureResNet18(ctx, sd, 32, MINI_BLOCKS, form=form_of(prg, reveal))
        if reveal != "confusion":
            return model(images), ctx.stats
        model.begin()
        model(images, labels=labels)
        return model.finish(), ctx.stats

    (a, stats), (b, _) = (eager(prg, Dealer(cuda, seed=SEED, fss_bits=64, fss_prg=prg)) for prg in ("sha", "chacha"))
    assert a.dtype == b.dtype and torch.equal(a, b)
    assert stats["dif_evals"] > 0 and (reveal != "confusion" or (stats["dpf_evals"] > 0 and int(a.sum()) == 2))
    if reveal == "confusion":
        return
    g = {prg: GraphedSecureInference(sd, cuda, input_size=32, precision_fractional=PF, seed=SEED, blocks=MINI_BLOCKS, batch=2,
                                     form=form_of(prg, reveal)) for prg in ("sha", "chacha")}
    assert g["sha"].static_bytes == g["chacha"].static_bytes and g["sha"].requests == g["chacha"].requests
    for step in range(3):      # the primitives of the constructor's refill, then two more refills
        out = {prg: g[prg](images, refill=step > 0).clone() for prg in g}
        want, _ = eager("chacha", PreloadedDealer(g["chacha"].tape, cuda, 64, "chacha"))
        assert torch.equal(out["sha"], out["chacha"]) and torch.equal(out["chacha"], want), step


def test_cli_fss_prg(cuda, tmp_path):
    ckpt = write_checkpoint(tmp_path / "bn.pt", wide_net()[0])
    run = lambda prg: json_line(run_inference(ckpt, 2, PF, ["--encrypted_inference", "--fss_bits", "64", "--fss_prg", prg],
                                              batch_size=2))["Inference Results"]
    res = run("chacha")
    assert sorted(res) == ["0", "1"] and res == run("sha")
