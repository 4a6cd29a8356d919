"""Host: what train.py decides about --dp_sampling poisson before anything touches a GPU, and the probability the
accountant is given."""
import warnings
from types import SimpleNamespace

import pytest

import train
from primia_amd import dp_accountant as A


def test_parser_defaults():
    p = train.build_parser()
    a = p.parse_args(["--config", "x.ini"])
    assert a.dp_sampling == "shuffle" and a.dp_delta == 1e-5
    a = p.parse_args(["--config", "x.ini", "--dp_sampling", "poisson", "--dp_delta", "1e-6"])
    assert a.dp_sampling == "poisson" and a.dp_delta == 1e-6
    with pytest.raises(SystemExit):
        p.parse_args(["--config", "x.ini", "--dp_sampling", "bernoulli"])


def test_poisson_without_dp_warns_and_does_nothing():
    cmd = SimpleNamespace(dp_sampling="poisson")
    with pytest.warns(UserWarning, match="--dp_sampling poisson has no effect"):
        assert train.DPOptions.from_args(SimpleNamespace(differentially_private=False), cmd).poisson is False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert train.DPOptions.from_args(SimpleNamespace(differentially_private=True), cmd).poisson is True
        assert train.DPOptions.from_args(SimpleNamespace(differentially_private=True),
                                         SimpleNamespace(dp_sampling="shuffle")).poisson is False
        assert train.DPOptions.from_args(SimpleNamespace(differentially_private=False), SimpleNamespace()).poisson is False
        assert train.DPOptions.from_args(SimpleNamespace(differentially_private=True), None).poisson is False


@pytest.mark.parametrize("n", [8, 7, 1])
def test_an_expected_batch_of_all_records_is_refused(n):
    with pytest.raises(SystemExit, match=">= 1"):
        train.poisson_plan("alice", n, 8, 1, 1e-5, 1.3)


def test_the_accountant_is_given_the_kernels_probability():
    """q = floor(L * 2^64 / n) / 2^64: the threshold word the kernel compares with, not L / n rounded some other way."""
    for n, L, epochs in ((1721, 256, 40), (24, 8, 1), (3, 1, 2)):
        q, planned, capacity = train.poisson_plan("alice", n, L, epochs, 1e-5, 1.3)
        t = (L << 64) // n
        assert q == t / 2 ** 64 == A.q_of_threshold(A.threshold_for((L, n)))
        assert planned == epochs * -(-n // L)
        assert capacity == A.capacity_for(n, q, planned, 1e-5, sigma=1.3) and q * n <= capacity <= n
    assert train.poisson_plan("alice", 1721, 256, 40, 1e-5, 1.3)[2] in range(370, 400)


def test_a_resumed_plan_adds_the_epochs_ahead_to_the_ledgers_steps():
    q, planned, k = train.poisson_plan("alice", 1721, 64, 10, 1e-5, 1.3)
    led = A.Ledger(1721, k, 1e-5, planned)
    led.add_steps(q, 1.3, planned)
    q2, planned2, k2 = train.poisson_plan("alice", 1721, 64, 3, 1e-5, 1.3, spent=led)
    assert q2 == q and planned2 == planned + 3 * 27 and k <= k2 <= 1721
    assert train.poisson_plan("alice", 1721, 64, 3, 1e-5, 1.3, spent=A.Ledger(1721, k, 1e-5, 0))[1:] == \
        train.poisson_plan("alice", 1721, 64, 3, 1e-5, 1.3)[1:]
