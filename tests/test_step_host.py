"""Host: the one training step of the host loops (primia_amd.step) on recording stand-ins — the eager step and its
sibling rule, micro-batch phases as arguments, the dispatch of train_step, and that the three loops (torchlib_compat.train,
torchlib_compat.secure_aggregation_epoch, fed.federated_epoch) all take their steps through it (no GPU needed)."""
from types import SimpleNamespace

import pytest
import torch

from primia_amd import fed, step, torchlib_compat
from primia_amd.optim import EngineOptimizer
from tests.cpu_standins import CpuArenaOps, ToyEngine


class _Engine:
    """The parts of ResNet18Engine a step touches, recording the calls of the root and of its siblings in one list."""

    def __init__(self, n, dp=False, micro=1, root=None):
        self.N, self._root = n, root or self
        self.calls = [] if root is None else root.calls
        self.siblings = {}
        self.pass_losses = iter(())         # what the next loss_backward calls return; zeros when exhausted
        self.fail_at = None                 # the number of the loss_backward call that raises
        self.dp_params = {"max_grad_norm": 1.0, "noise_multiplier": 1.3} if dp else None
        self.dp_micro_batches = micro

    def sibling(self, n):
        root = self._root
        if n == root.N:
            return root
        if n not in root.siblings:
            root.siblings[n] = _Engine(n, root=root)
        return root.siblings[n]

    def forward(self, x):
        assert x.shape[0] == self.N
        self.calls.append(("forward", self.N))

    def loss_backward(self, target, soft=False, **kw):
        root = self._root
        self.calls.append(("loss_backward", self.N, soft, kw))
        if root.fail_at == sum(1 for c in self.calls if c[0] == "loss_backward"):
            raise RuntimeError("the stand-in's pass failed")
        return torch.tensor([next(root.pass_losses, 0.0)])


class _Bare:
    """An engine from before siblings: no `sibling`, no `N`, a two-argument loss_backward."""

    def __init__(self):
        self.calls = []

    def forward(self, x):
        self.calls.append("forward")

    def loss_backward(self, target, soft=False):
        self.calls.append("loss_backward")
        return torch.zeros(1)


class _Opt:
    kind = "SGD"

    def __init__(self, eng):
        self.engine = eng

    def zero_grad(self):
        self.engine.calls.append("zero_grad")

    def step(self, engine=None):
        self.engine.calls.append(("step", engine))


def batch(n):
    return torch.zeros(n, 3, 8, 8), torch.zeros(n, dtype=torch.long)


def steps_taken(eng):
    return [c for c in eng.calls if c[0] == "step"]


def test_eager_step_at_the_engines_size_on_a_sibling_and_on_a_bare_engine():
    eng = _Engine(4)
    loss = step.eager_step(eng, _Opt(eng), *batch(4), soft=True)
    assert eng.calls == ["zero_grad", ("forward", 4), ("loss_backward", 4, True, {}), ("step", None)]
    assert loss.shape == (1,) and not eng.siblings
    del eng.calls[:]
    step.eager_step(eng, _Opt(eng), *batch(3))                  # a ragged batch: the sibling runs it and is stepped
    sib = eng.siblings[3]
    assert eng.calls == ["zero_grad", ("forward", 3), ("loss_backward", 3, False, {}), ("step", sib)]
    bare = _Bare()
    step.eager_step(bare, _Opt(bare), *batch(5))
    assert bare.calls == ["zero_grad", "forward", "loss_backward", ("step", None)]
    del bare.calls[:]
    step.train_step(bare, _Opt(bare), *batch(5))                # no dp_micro_batches, no hip_graph: the same step
    assert bare.calls == ["zero_grad", "forward", "loss_backward", ("step", None)]


@pytest.mark.parametrize("phase,stepped", [(None, True), ("first", False), ("more", False), ("last", True)])
def test_only_the_last_phase_steps_and_a_phase_reaches_loss_backward(phase, stepped):
    eng = _Engine(4, dp=True)
    step.eager_step(eng, _Opt(eng), *batch(4), phase=phase, logical_batch=12)
    kw = {} if phase is None else {"phase": phase, "logical_batch": 12}
    assert eng.calls[:3] == ["zero_grad", ("forward", 4), ("loss_backward", 4, False, kw)]
    assert eng.calls[3:] == ([("step", None)] if stepped else [])


def test_a_micro_batch_engine_runs_the_batch_as_passes_with_their_phases():
    eng = _Engine(2, dp=True, micro=3)
    eng.pass_losses = iter((1.0, 2.0, 3.0))
    eng.sibling(1)                          # (the ragged pass's engine exists: a sibling is no state of a step)
    before = sorted(eng.__dict__)
    loss = step.train_step(eng, _Opt(eng), *batch(5))
    passes = [(c[1], c[3]["phase"], c[3]["logical_batch"]) for c in eng.calls if c[0] == "loss_backward"]
    assert passes == [(2, "first", 5), (2, "more", 5), (1, "last", 5)]
    assert steps_taken(eng) == [("step", eng.siblings[1])] and eng.calls[-1][0] == "step"
    assert loss.shape == (1,) and loss.item() == pytest.approx(1.8, rel=1e-6)      # (2 * 1 + 2 * 2 + 1 * 3) / 5
    assert sorted(eng.__dict__) == before and sorted(eng.siblings[1].__dict__) == before


def test_an_error_in_a_pass_leaves_nothing_behind():
    eng = _Engine(2, dp=True, micro=3)
    opt = _Opt(eng)
    eng.fail_at = 2
    with pytest.raises(RuntimeError, match="stand-in's pass failed"):
        step.train_step(eng, opt, *batch(6))
    assert [c[3]["phase"] for c in eng.calls if c[0] == "loss_backward"] == ["first", "more"]
    assert steps_taken(eng) == []
    del eng.calls[:]
    eng.fail_at = None
    step.train_step(eng, opt, *batch(2))    # one pass: an ordinary step, with no phase left over from the failed one
    assert eng.calls == ["zero_grad", ("forward", 2), ("loss_backward", 2, False, {}), ("step", None)]


def test_hip_graph_sends_the_step_and_every_pass_to_graphed_step(monkeypatch):
    from primia_amd import graphed_train

    seen = []

    def recorder(engine, optimizer, data, target, soft=False, phase=None, logical_batch=None):
        seen.append((int(data.shape[0]), soft, phase, logical_batch))
        return torch.ones(1)

    monkeypatch.setattr(graphed_train, "graphed_step", recorder)
    eng = _Engine(4)
    assert step.train_step(eng, _Opt(eng), *batch(4), soft=True, hip_graph=True).item() == 1.0
    assert seen == [(4, True, None, None)] and eng.calls == []
    del seen[:]
    eng = _Engine(2, dp=True, micro=3)
    step.train_step(eng, _Opt(eng), *batch(5), hip_graph=True)
    assert seen == [(2, False, "first", 5), (2, False, "more", 5), (1, False, "last", 5)] and eng.calls == []
    del seen[:]
    step.train_step(eng, _Opt(eng), *batch(2), hip_graph=True)        # one pass: no phase; the size is not a key's business
    assert seen == [(2, False, None, 2)]


# ---- the three loops ----------------------------------------------------------------------------------------------------
class _Toy(ToyEngine):
    """ToyEngine (a real least-squares step under a real EngineOptimizer), recording."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, data):
        self.calls.append("forward")
        return super().forward(data)

    def loss_backward(self, target, soft=False):
        self.calls.append(("loss_backward", soft))
        return super().loss_backward(target, soft)

    def sgd_step(self, lr, weight_decay):
        self.calls.append("step")
        super().sgd_step(lr, weight_decay)


ARGS = dict(optimizer="SGD", lr=0.05, weight_decay=0.0, sync_every_n_batch=8, keep_optim_dict=False,
            weighted_averaging=False, unencrypted_aggregation=True, mixup=False, log_interval=1)


def toy_batches():
    g = torch.Generator().manual_seed(3)
    return [(torch.randn(6, 16, generator=g), torch.randn(6, generator=g)) for _ in range(2)]


def run_train(eng, data):
    args = SimpleNamespace(**ARGS)
    torchlib_compat.train(args, eng, "cpu", data, EngineOptimizer.from_args(eng, args), 1, None, verbose=False)


def run_secure_aggregation_epoch(eng, data):
    args = SimpleNamespace(**ARGS)
    models = {"local_model": _Toy(), "alice": eng}
    torchlib_compat.secure_aggregation_epoch(args, models, "cpu", {"alice": data}, {"alice": None}, 1,
                                             {"alice": SimpleNamespace(soft=False)}, None)


def run_federated_epoch(eng, data):
    fed.federated_epoch(eng, data, SimpleNamespace(**ARGS), ops=CpuArenaOps())


@pytest.mark.parametrize("module,loop", [(torchlib_compat, run_train), (torchlib_compat, run_secure_aggregation_epoch),
                                         (fed, run_federated_epoch)])
def test_every_loop_takes_its_steps_through_train_step(monkeypatch, module, loop):
    data = toy_batches()
    want = _Toy()
    args = SimpleNamespace(**ARGS)
    opt = EngineOptimizer.from_args(want, args)
    for x, y in data:
        step.eager_step(want, opt, x, y)
    assert want.calls == ["forward", ("loss_backward", False), "step"] * 2

    through = []

    def counted(*a, **kw):
        through.append(kw)
        return step.train_step(*a, **kw)

    monkeypatch.setattr(module, "train_step", counted)
    # (aggregation works on the arenas with HIP kernels: not what is looked at here)
    monkeypatch.setattr(torchlib_compat, "aggregation", lambda local_model, *a, **kw: local_model)
    monkeypatch.setattr(torchlib_compat, "send_new_models", lambda local_model, models: models)
    eng = _Toy()
    loop(eng, data)
    assert eng.calls == want.calls
    assert through == [{"soft": False, "hip_graph": False}] * 2
    assert torch.equal(eng.flat, want.flat)         # (the average of one client that the epoch ends on is its own arena)
