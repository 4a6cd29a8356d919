"""Host: the privacy accountant of Poisson-sampled DP-SGD (primia_amd/dp_accountant.py) against an independent
reference — the defining integral of the sampled Gaussian mechanism's Renyi divergence, by mpmath quadrature:

    rdp(q, sigma, alpha) = log( integral N(z; 0, sigma^2) * ((1 - q) + q * exp((2 z - 1) / (2 sigma^2)))^alpha dz ) / (alpha - 1)

(the divergence D_alpha(mixture || N(0, sigma^2)), the larger of the two directions: Mironov, Talwar, Zhang 2019, section
3.1).  Tolerance 1e-6 relative; the series of this module agree with the quadrature to 3e-10 over this grid (the test
prints each case's figure)."""
import math
from fractions import Fraction

import pytest

from primia_amd import dp_accountant as A


@pytest.fixture(scope="module")
def mp():
    import mpmath          # installed with torch's sympy

    return mpmath


def rdp_quad(mp, q, sigma, alpha):
    mp.mp.dps = 40
    q, s, a = mp.mpf(q), mp.mpf(sigma), mp.mpf(alpha)

    def f(z):
        return mp.npdf(z, 0, s) * ((1 - q) + q * mp.exp((2 * z - 1) / (2 * s * s))) ** a

    # the integrand's mass sits between the two Gaussians' bulks and, for large alpha, around z = alpha
    pts = [-mp.inf, -10 * s, 0, 1, float(alpha), float(alpha) + 10 * s, mp.inf]
    return float(mp.log(mp.quad(f, sorted(set(pts)))) / (a - 1))


GRID = [(q, s, a) for q in (0.01, 0.149, 0.5) for s in (0.7, 1.3, 4.0) for a in (1.1, 2, 5.5, 32, 63)]


@pytest.mark.parametrize("q,sigma,alpha", GRID)
def test_rdp_against_quadrature(mp, q, sigma, alpha):
    ref = rdp_quad(mp, q, sigma, alpha)
    got = A.rdp_sampled_gaussian(q, sigma, alpha)
    print(f"q={q} sigma={sigma} alpha={alpha}: got {got!r} ref {ref!r} rel {abs(got - ref) / ref:.3e}")
    assert abs(got - ref) <= 1e-6 * ref


def test_closed_forms():
    for sigma in (0.7, 1.3, 4.0):
        for alpha in (1.1, 2, 5.5, 32, 63):
            assert A.rdp_sampled_gaussian(1.0, sigma, alpha) == alpha / (2 * sigma ** 2)
            assert A.rdp_sampled_gaussian(0.0, sigma, alpha) == 0.0
    with pytest.raises(ValueError):
        A.rdp_sampled_gaussian(0.1, 1.0, 1.0)


def test_default_orders():
    assert A.DEFAULT_ALPHAS == [1 + x / 10.0 for x in range(1, 100)] + list(range(12, 64))


def test_epsilon_monotone():
    q, delta = 256 / 1721, 1e-5
    eps_t = [A.epsilon([(q, 1.3, t)], delta)[0] for t in (1, 10, 100, 280, 281, 1000)]
    assert all(a <= b for a, b in zip(eps_t, eps_t[1:])), eps_t
    eps_s = [A.epsilon([(q, s, 280)], delta)[0] for s in (0.6, 0.9, 1.3, 2.0, 4.0)]
    assert all(a >= b for a, b in zip(eps_s, eps_s[1:])), eps_s
    assert eps_t[0] > 0 and eps_s[-1] > 0


def test_segments_compose_to_the_sum():
    segs = [(0.149, 1.3, 280), (0.05, 0.9, 120)]
    alphas = [1.5, 2, 7.3, 32]
    both = A.total_rdp(segs, alphas)
    one, two = A.total_rdp(segs[:1], alphas), A.total_rdp(segs[1:], alphas)
    for b, x, y, a in zip(both, one, two, alphas):
        assert b == pytest.approx(x + y, rel=1e-15)
        assert x == pytest.approx(280 * A.rdp_sampled_gaussian(0.149, 1.3, a), rel=1e-15)
    eps, a = A.epsilon(segs, 1e-5, alphas)
    assert eps == min(b + math.log(1e5) / (al - 1) for b, al in zip(both, alphas))
    # the same (q, sigma) in two segments is the same as one
    assert A.epsilon([(0.149, 1.3, 100), (0.149, 1.3, 180)], 1e-5)[0] == pytest.approx(
        A.epsilon([(0.149, 1.3, 280)], 1e-5)[0], rel=1e-14)


def test_orientation_figures():
    """The issue's three settings (sigma 1.3, delta 1e-5): printed, and held only to the broad side of its '~'."""
    for n, L, T, eps_about in ((1721, 256, 280, 14.0), (5163, 256, 840, 7.5), (1721, 64, 270, 3.2)):
        q = A.q_of_threshold(A.threshold_for((L, n)))
        eps, alpha = A.epsilon([(q, 1.3, T)], A.DELTA_SHARE * 1e-5)
        k = A.capacity_for(n, q, T, 1e-5, sigma=1.3)
        print(f"n={n} L={L} T={T}: eps {eps:.3f} at order {alpha}, capacity {k}")
        assert abs(eps - eps_about) < 0.1 * eps_about


# ---- capacity -------------------------------------------------------------------------------------------------------
def tail(n, q, k):
    """P[Binomial(n, q) > k] summed with math.lgamma, largest terms last."""
    terms = [math.exp(math.lgamma(n + 1) - math.lgamma(j + 1) - math.lgamma(n - j + 1) + j * math.log(q)
                      + (n - j) * math.log1p(-q)) for j in range(k + 1, n + 1)]
    return math.fsum(terms)


@pytest.mark.parametrize("n,L,T,sigma,delta", [(1721, 256, 280, 1.3, 1e-5), (5163, 256, 840, 1.3, 1e-5),
                                               (1721, 64, 270, 1.3, 1e-5), (40, 8, 5, 1.3, 1e-5),
                                               (100, 1, 50, 4.0, 1e-3)])
def test_capacity_for(n, L, T, sigma, delta):
    q = A.q_of_threshold(A.threshold_for((L, n)))
    eps = A.epsilon([(q, sigma, T)], 0.99 * delta)[0]
    k = A.capacity_for(n, q, T, delta, sigma=sigma)
    print(f"n={n} L={L} T={T}: eps {eps:.4f} capacity {k}")
    cost = lambda kk: (1 + math.exp(eps)) * T * tail(n, q, kk)  # noqa: E731
    assert cost(k) <= 0.01 * delta
    assert k >= math.ceil(q * n)
    if k > math.ceil(q * n):
        assert cost(k - 1) > 0.01 * delta
    assert k <= n


# ---- threshold ------------------------------------------------------------------------------------------------------
def test_threshold_is_exact():
    for L, n in ((256, 1721), (64, 1721), (256, 5163), (1, 3), (1, 2), (5, 7), (1720, 1721)):
        t = A.threshold_for((L, n))
        assert t == (L << 64) // n and t == A.threshold_for(Fraction(L, n))
        assert t * n <= L << 64 < (t + 1) * n           # floor, in integers
        assert 0 <= t < 2 ** 64
        qa = A.q_of_threshold(t)
        assert Fraction(qa) == Fraction(t, 2 ** 64) or abs(Fraction(qa) - Fraction(t, 2 ** 64)) <= Fraction(1, 2 ** 53)
        assert qa == t / 2 ** 64
    assert A.threshold_for(0.5) == 2 ** 63
    assert A.threshold_for(0) == 0
    for bad in ((7, 7), (8, 7), 1.0, Fraction(3, 2)):
        with pytest.raises(ValueError):
            A.threshold_for(bad)
    with pytest.raises(ValueError):
        A.threshold_for(-0.1)


# ---- ledger ---------------------------------------------------------------------------------------------------------
def test_ledger_segments_and_round_trip(tmp_path):
    import torch

    q = A.q_of_threshold(A.threshold_for((64, 1721)))
    led = A.Ledger(n=1721, capacity=122, delta=1e-5, planned_steps=270)
    for _ in range(27):
        led.add_steps(q, 1.3)
    led.add_steps(q, 1.3, 3)
    assert led.segments == [[q, 1.3, 30]]
    led.add_steps(q, 1.1, 2)                 # a changed sigma opens a new segment
    led.add_steps(q / 2, 1.1, 1)             # and so does a changed q
    led.overflow_events = 1
    assert [s[2] for s in led.segments] == [30, 2, 1] and led.steps == 33
    path = tmp_path / "ck.pt"
    torch.save({"dp_privacy": {"client0": led.state_dict()}}, path)
    back = A.Ledger.from_state_dict(torch.load(path)["dp_privacy"]["client0"])
    assert back.state_dict() == led.state_dict()
    assert back.report() == led.report()
    back.add_steps(q / 2, 1.1, 4)            # a resumed run keeps counting
    assert back.segments[-1] == [q / 2, 1.1, 5]
    r = back.report()
    assert r["epsilon"] == A.epsilon(back.segments, 0.99e-5)[0] and r["steps"] == 37 and r["overflow_events"] == 1
    assert r["epsilon"] > led.report()["epsilon"]


def test_ledger_reports_a_larger_delta_past_the_plan():
    n, L, T, delta = 1721, 64, 270, 1e-5
    q = A.q_of_threshold(A.threshold_for((L, n)))
    k = A.capacity_for(n, q, T, delta, sigma=1.3)
    led = A.Ledger(n, k, delta, T)
    led.add_steps(q, 1.3, T)
    assert led.report()["within_plan"] and led.report()["delta"] == delta
    led.add_steps(q, 1.3, 200 * T)           # far beyond the plan: the capacity condition fails
    r = led.report()
    assert not r["within_plan"] and r["delta"] > delta


def test_resumed_plan_counts_what_was_spent():
    """A ledger remembers the capacity each segment ran at; a resumed run's capacity keeps the truncation event of the
    earlier steps (at their capacity) plus its own within 1% of delta, or truncates nothing when they no longer fit."""
    n, L, delta = 1721, 64, 1e-5
    q = A.q_of_threshold(A.threshold_for((L, n)))
    k1 = A.capacity_for(n, q, 270, delta, sigma=1.3)
    led = A.Ledger(n, k1, delta, 270)
    led.add_steps(q, 1.3, 270)
    assert led.capacities == [k1] and led.report()["within_plan"]
    mass = led.truncation_mass()
    assert mass == pytest.approx(270 * math.exp(A.log_binom_tail(n, q, k1)), rel=1e-12)
    eps = A.epsilon([[q, 1.3, 270], [q, 1.3, 270]], 0.99 * delta)[0]
    k2 = A.capacity_for(n, q, 270, delta, eps=eps, spent=mass)
    assert k1 <= k2 <= n
    back = A.Ledger.from_state_dict(led.state_dict())
    back.capacity = k2
    back.add_steps(q, 1.3, 270)
    assert back.capacities == ([k1, k2] if k2 != k1 else [k1]) and back.steps == 540
    r = back.report()
    cost = (1 + math.exp(r["epsilon"])) * back.truncation_mass()
    assert r["epsilon"] == eps and r["within_plan"] == (cost <= 0.01 * delta)
    if k2 < n:
        assert r["within_plan"] and r["delta"] == delta
    # earlier steps that alone outgrew the share: capacity n (nothing more is truncated), and the report says so
    assert A.capacity_for(n, q, 270, delta, eps=eps, spent=1.0) == n
    old = A.Ledger.from_state_dict({**led.state_dict(), "segment_capacities": [math.ceil(q * n)]})
    assert not old.report()["within_plan"] and old.report()["delta"] > delta
    # a state dict from before segments carried capacities reads as the ledger's own
    d = led.state_dict()
    del d["segment_capacities"]
    assert A.Ledger.from_state_dict(d).capacities == [k1]
