"""GPU: the training step replayed as a hipGraph (primia_amd.graphed_train, train.py --hip_graph) against the eager step.

The step is deterministic (no floating-point atomics on its path) and the optimizer's device-scalar kernels share the
host-scalar kernels' arithmetic, so every comparison here is torch.equal: graphed training computes exactly what eager
training computes."""
import ctypes
import os
import random
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

from primia_amd import fed  # noqa: E402
from primia_amd import resnet_spec as rs  # noqa: E402
from primia_amd._lib import call  # noqa: E402
from primia_amd.engine import ResNet18Engine  # noqa: E402
from primia_amd.graphed_train import captures  # noqa: E402
from primia_amd.optim import EngineOptimizer  # noqa: E402
from primia_amd.torchlib_compat import secure_aggregation_epoch, train  # noqa: E402


def targs(kind="SGD", hip_graph=False, **kw):
    a = dict(optimizer=kind, lr=1e-3, weight_decay=5e-4, beta1=0.5, beta2=0.99, log_interval=1, mixup=False,
             hip_graph=hip_graph, sync_every_n_batch=1, keep_optim_dict=False, weighted_averaging=False,
             unencrypted_aggregation=False, precision_fractional=16)
    a.update(kw)
    return SimpleNamespace(**a)


def batches(cuda, n, batch, size, seed, soft=False):
    g = torch.Generator(device=cuda).manual_seed(seed)
    out = []
    for _ in range(n):
        x = torch.randn(batch, 3, size, size, generator=g, device=cuda)
        y = torch.randint(0, 3, (batch,), generator=g, device=cuda)
        out.append((x, y))
    return out


def engine_pair(cuda, batch, size, dtype, seed=7):
    torch.manual_seed(seed)
    sd = rs.init_state_dict(rs.resnet18_spec(3, 3, size, "max"))
    engs = []
    for _ in range(2):
        e = ResNet18Engine(batch, 3, 3, size, "max", dtype=dtype, device=cuda)
        e.load_state_dict(sd)
        engs.append(e)
    return engs


def assert_same(a, b, oa=None, ob=None):
    assert torch.equal(a.flat, b.flat)
    assert torch.equal(a.logits, b.logits)
    assert torch.equal(a.loss, b.loss)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    if oa is not None:
        da, db = oa.state_dict(), ob.state_dict()
        assert da["param_groups"] == db["param_groups"]
        assert sorted(da["state"]) == sorted(db["state"])
        for i in da["state"]:
            assert da["state"][i]["step"] == db["state"][i]["step"], i
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(da["state"][i][k], db["state"][i][k]), (i, k)


# ---- 1. the device-scalar kernels against the host-scalar ones ---------------------------------------------------------
def hyper_of(cuda, lr, wd, b1=0.0, b2=0.0, eps=0.0, step=0):
    h = torch.full((8,), float("nan"), dtype=torch.float32, device=cuda)
    call("primia_opt_hyper_set", h, lr, wd, b1, b2, eps, step)
    return h


def test_sgd_dev_kernels_bitwise(cuda):
    g = torch.Generator(device=cuda).manual_seed(1)
    n = 4 * 12345 + 3                                     # odd tail after the float4 body
    p = torch.randn(n, generator=g, device=cuda)
    gr = torch.randn(n, generator=g, device=cuda)
    lr, wd = 0.0123, 5e-4
    a, b = p.clone(), p.clone()
    call("primia_sgd_step", a, gr, n, lr, wd)
    call("primia_sgd_step_dev", b, gr, n, hyper_of(cuda, lr, wd))
    assert torch.equal(a, b) and not torch.equal(a, p)
    # ranges
    begin = (ctypes.c_int64 * 3)(0, 1000, 40001)
    length = (ctypes.c_int64 * 3)(17, 5000, 9)
    a, b = p.clone(), p.clone()
    call("primia_sgd_step_ranges", a, gr, begin, length, 3, lr, wd)
    call("primia_sgd_step_ranges_dev", b, gr, begin, length, 3, hyper_of(cuda, lr, wd))
    assert torch.equal(a, b) and not torch.equal(a, p)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_tiled_sgd_dev_bitwise(cuda, dtype):
    """The fused gradient-finalize + SGD + weight-refresh pass (primia_conv_sgd_step_many[_dev]) and the ranges it leaves
    over, through the engine: master weights, gradients and the compute-dtype weight copies."""
    a, b = engine_pair(cuda, 8, 64, dtype)
    for e in (a, b):
        e.fuse_sgd_tail = True
    (x, y), = batches(cuda, 1, 8, 64, 3)
    lr, wd = 0.037, 5e-4
    for e in (a, b):
        e.forward(x)
        e.loss_backward(y)
        assert e._grads_pending
    a.sgd_step(lr, wd)
    b.sgd_step(999.0, 999.0, hyper=hyper_of(cuda, lr, wd))
    assert torch.equal(a.flat, b.flat) and torch.equal(a.grads, b.grads)
    for name, c in a.convs.items():
        assert torch.equal(c.w_fwd, b.convs[name].w_fwd), name
        if c.w_dgrad is not None:
            assert torch.equal(c.w_dgrad, b.convs[name].w_dgrad), name


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_dev_kernel_bitwise(cuda, step):
    g = torch.Generator(device=cuda).manual_seed(step)
    n = 4 * 3001 + 1
    p, gr = torch.randn(n, generator=g, device=cuda), torch.randn(n, generator=g, device=cuda)
    m, v = torch.randn(n, generator=g, device=cuda) * 0.1, torch.rand(n, generator=g, device=cuda) * 0.01
    lr, b1, b2, eps, wd = 1e-3, 0.5, 0.99, 1e-8, 5e-4
    a = [t.clone() for t in (p, m, v)]
    b = [t.clone() for t in (p, m, v)]
    call("primia_adam_step", a[0], gr, a[1], a[2], n, lr, b1, b2, eps, wd, step)
    call("primia_adam_step_dev", b[0], gr, b[1], b[2], n, hyper_of(cuda, lr, wd, b1, b2, eps, step))
    for u, w in zip(a, b):
        assert torch.equal(u, w)
    assert not torch.equal(a[0], p)


# ---- 2. train(): graphed against eager ---------------------------------------------------------------------------------
def run_train(model, args, data, lr2):
    """train() over the batches with the learning rate changed between steps 3 and 4 (the scheduler's write)."""
    opt = EngineOptimizer.from_args(model, args)
    train(args, model, None, data[:3], opt, 1, None, verbose=False)
    opt.param_groups[0]["lr"] = lr2
    train(args, model, None, data[3:], opt, 1, None, verbose=False)
    torch.cuda.synchronize()
    return opt


@pytest.mark.parametrize("dtype,size,batch", [(torch.float32, 64, 8), (torch.bfloat16, 224, 256)])
@pytest.mark.parametrize("kind", ["SGD", "Adam"])
def test_train_graphed_matches_eager(cuda, dtype, size, batch, kind):
    data = batches(cuda, 6, batch, size, 5)
    eager, graphed = engine_pair(cuda, batch, size, dtype)
    oe = run_train(eager, targs(kind), data, 3e-4)
    og = run_train(graphed, targs(kind, hip_graph=True), data, 3e-4)
    assert_same(eager, graphed, oe, og)
    assert eager.num_batches_tracked["bn1"] == 6
    assert list(captures(graphed).values()) == [1]
    assert captures(eager) == {}


# ---- 3. Adam state across optimizer re-creation and load_state_dict -----------------------------------------------------
def test_adam_state_changes_without_recapture(cuda):
    data = batches(cuda, 8, 8, 64, 9)
    runs = []
    for hg in (False, True):
        model = engine_pair(cuda, 8, 64, torch.float32)[0]
        args = targs("Adam", hip_graph=hg)
        opt = EngineOptimizer.from_args(model, args)
        train(args, model, None, data[:3], opt, 1, None, verbose=False)
        saved = opt.state_dict()                                  # step 3
        opt = EngineOptimizer.from_args(model, args)              # a FedAvg sync re-creates it: moments dropped
        train(args, model, None, data[3:5], opt, 1, None, verbose=False)
        opt.load_state_dict(saved)                                # checkpoint resume mid-run
        train(args, model, None, data[5:], opt, 1, None, verbose=False)
        torch.cuda.synchronize()
        runs.append((model, opt))
    (a, oa), (b, ob) = runs
    assert_same(a, b, oa, ob)
    assert ob.state_dict()["state"][0]["step"] == 6
    assert list(captures(b).values()) == [1]


# ---- 4. a ragged last batch runs eagerly -------------------------------------------------------------------------------
def test_ragged_last_batch_runs_eagerly(cuda):
    full = batches(cuda, 3, 8, 64, 13)
    x5, y5 = batches(cuda, 1, 5, 64, 14)[0]
    loader = full + [(x5, y5)]
    runs = []
    for hg in (False, True):
        model = engine_pair(cuda, 8, 64, torch.float32)[0]
        args = targs("SGD", hip_graph=hg)
        opt = EngineOptimizer.from_args(model, args)
        for ep in range(2):
            train(args, model, None, loader, opt, ep, None, verbose=False)
        runs.append((model, opt))
    (a, _), (b, _) = runs
    assert_same(a, b)
    assert torch.equal(a.sibling(5).logits, b.sibling(5).logits)
    assert [k[0] for k in captures(b)] == [8]
    assert "_step_graphs" not in b.sibling(5).__dict__


# ---- 5. MixUp: B and B / 2 alternate -----------------------------------------------------------------------------------
def test_mixup_halves_graphed(cuda):
    data = batches(cuda, 10, 8, 64, 17)
    runs = []
    for hg in (False, True):
        model = engine_pair(cuda, 8, 64, torch.float32)[0]
        args = targs("SGD", hip_graph=hg, mixup=True, mixup_prob=0.5, mixup_lambda=0.3)
        opt = EngineOptimizer.from_args(model, args)
        random.seed(1234)
        train(args, model, None, data, opt, 1, None, verbose=False)
        torch.cuda.synchronize()
        runs.append((model, opt))
    (a, _), (b, _) = runs
    assert_same(a, b)
    caps = captures(b)
    assert 1 <= len(caps) <= 2 and set(caps.values()) == {1}
    assert {k[0] for k in caps} <= {8, 4}


# ---- 6. federated epochs -----------------------------------------------------------------------------------------------
def test_secure_aggregation_epoch_graphed(cuda):
    shards = {"alice": 4, "bob": 3}
    data = {w: batches(cuda, n, 8, 64, 20 + i) for i, (w, n) in enumerate(shards.items())}
    runs = []
    for hg in (False, True):
        torch.manual_seed(3)
        sd = rs.init_state_dict(rs.resnet18_spec(3, 3, 64, "max"))
        models = {}
        for w in ["local_model"] + list(shards):
            models[w] = ResNet18Engine(8, 3, 3, 64, "max", dtype=torch.float32, device=cuda)
            models[w].load_state_dict(sd)
        args = targs("Adam", hip_graph=hg, unencrypted_aggregation=False, sync_every_n_batch=1)
        opts = {w: EngineOptimizer.from_args(models[w], args) for w in shards}
        losses = []
        for ep in range(2):
            models, avg = secure_aggregation_epoch(args, models, cuda, data, opts, ep, None, None)
            losses.append(avg)
        runs.append((models, losses))
    (ma, la), (mb, lb) = runs
    assert la == lb
    for w in shards:
        assert_same(ma[w], mb[w])
    sa, sb = ma["local_model"].state_dict(), mb["local_model"].state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert all(v == 1 for w in shards for v in captures(mb[w]).values())


def test_federated_epoch_world_one_graphed(cuda):
    data = batches(cuda, 5, 8, 64, 31)
    runs = []
    for hg in (False, True):
        model = engine_pair(cuda, 8, 64, torch.float32)[0]
        args = targs("SGD", hip_graph=hg, sync_every_n_batch=2)
        out = fed.federated_epoch(model, data, args)
        torch.cuda.synchronize()
        runs.append((model, out))
    (a, oa), (b, ob) = runs
    assert oa[0] == ob[0] and oa[1] == ob[1]
    assert torch.equal(oa[2], ob[2])
    assert_same(a, b)


# ---- 7. the CLI --------------------------------------------------------------------------------------------------------
def test_cli_hip_graph_checkpoint_matches_eager():
    env = dict(os.environ, PRIMIA_ALLOW_RANDOM_INIT="1", PRIMIA_SYNTHETIC_BATCHES="3", PRIMIA_DTYPE="bf16")
    sds = []
    for name, extra in (("hgeager", []), ("hggraph", ["--hip_graph"])):
        cmd = [sys.executable, "train.py", "--config", "configs/torch/smoke-federated.ini", "--train_federated",
               "--data_dir", "synthetic", "--training_name", name] + extra
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        ckpt = os.path.join(ROOT, "model_weights", f"final_federated_{name}.pt")
        sds.append(torch.load(ckpt, map_location="cpu", weights_only=False)["model_state_dict"])
        os.remove(ckpt)
    a, b = sds
    assert list(a) == list(b) and len(a) == 122
    for k in a:
        assert torch.equal(a[k], b[k]), k
