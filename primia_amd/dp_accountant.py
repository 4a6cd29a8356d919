"""Privacy accounting for DP-SGD on Poisson-sampled batches (float64 on the host, no GPU).

The mechanism of one step: every one of the n records joins the batch independently with probability q
(primia_poisson_select, threshold = floor(q * 2^64)), each selected record's gradient is clipped to L2 norm C, the sum gets
N(0, (sigma * C)^2 I) noise and is divided by the FIXED expected batch size L = q * n.  Adding or removing one record
changes the sum by at most C, so a step is the sampled Gaussian mechanism with noise multiplier sigma, whose Renyi
divergence of order alpha is bounded by

    rdp_sampled_gaussian(q, sigma, alpha)      (Mironov, Talwar and Zhang, "Renyi Differential Privacy of the Sampled
                                                Gaussian Mechanism", 2019, sections 3.3: integer and fractional alpha)

RDP adds over steps, and (alpha, r)-RDP gives (r + log(1 / delta) / (alpha - 1), delta)-DP for every alpha; `epsilon`
takes the best of a list of orders (the reference's PrivacyEngine list by default).

The batch has `capacity` slots.  A step that selects more than `capacity` records drops the excess, which the bound
above does not cover.  `capacity_for` makes that event rare enough to be paid for out of delta: a mechanism within
total variation beta of an (eps, delta')-DP one is (eps, delta' + (1 + e^eps) * beta)-DP, and beta is at most
T * P[Binomial(n, q) > capacity] over T steps.  eps is therefore computed at 0.99 * delta and the capacity is the
smallest one whose (1 + e^eps) * beta stays below 0.01 * delta.
"""
import functools
import math
from fractions import Fraction

DEFAULT_ALPHAS = [1 + x / 10.0 for x in range(1, 100)] + list(range(12, 64))
DELTA_SHARE = 0.99          # of delta goes to the RDP conversion, the rest to the truncation event

TWO64 = 1 << 64


# ---- the sampling probability ---------------------------------------------------------------------------------------
def threshold_for(q):
    """floor(q * 2^64) in integer arithmetic.  `q`: a Fraction, an (L, n) pair, an int or a float (a float is taken at
    its exact binary value).  q >= 1 is refused: every record in every batch is not a sampled mechanism, and 2^64 does
    not fit the kernel's threshold word."""
    if isinstance(q, tuple):
        q = Fraction(int(q[0]), int(q[1]))
    q = Fraction(q)
    if q < 0:
        raise ValueError(f"sampling probability {float(q)} is negative")
    if q >= 1:
        raise ValueError(f"sampling probability {float(q)} >= 1: Poisson sampling needs an expected batch below the "
                         "number of records")
    return (q.numerator * TWO64) // q.denominator


def q_of_threshold(threshold):
    """The probability the kernel samples with: threshold / 2^64 (as a float: the nearest double)."""
    t = int(threshold)
    if not 0 <= t < TWO64:
        raise ValueError("threshold outside [0, 2^64)")
    return t / TWO64          # int / int: correctly rounded


# ---- RDP of the sampled Gaussian mechanism --------------------------------------------------------------------------
def _log_add(a, b):
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    hi, lo = (a, b) if a > b else (b, a)
    return hi + math.log1p(math.exp(lo - hi))


def _log_sub(a, b):
    """log(e^a - e^b), a >= b."""
    if b == -math.inf:
        return a
    if a == b:
        return -math.inf
    if a < b:
        raise ValueError("log of a negative difference")
    return a + math.log1p(-math.exp(b - a))


def _log_comb(n, k):
    return math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)


def _log_erfc(x):
    """log(erfc(x)): math.erfc underflows near x = 26; beyond that the asymptotic series (relative error below 1e-12
    from x = 20 on)."""
    if x < 20.0:
        return math.log(math.erfc(x))
    x2 = x * x
    return (-x2 - math.log(x) - 0.5 * math.log(math.pi)
            + math.log1p(-0.5 / x2 + 0.75 / x2 ** 2 - 1.875 / x2 ** 3 + 6.5625 / x2 ** 4))


def _log_a_int(q, sigma, alpha):
    """log A_alpha for integer alpha: sum_k C(alpha, k) (1 - q)^(alpha - k) q^k exp((k^2 - k) / (2 sigma^2))."""
    log_a = -math.inf
    for k in range(alpha + 1):
        log_a = _log_add(log_a, _log_comb(alpha, k) + k * math.log(q) + (alpha - k) * math.log1p(-q)
                         + (k * k - k) / (2.0 * sigma ** 2))
    return log_a


def _log_a_frac(q, sigma, alpha):
    """log A_alpha for fractional alpha: the two series over the half lines split at z0 (section 3.3 of the paper)."""
    log_a0, log_a1 = -math.inf, -math.inf
    z0 = sigma ** 2 * math.log(1.0 / q - 1.0) + 0.5
    k, coef = 0, 1.0            # coef = C(alpha, k), signed: alternating once k > alpha
    while True:
        log_coef = math.log(abs(coef)) if coef != 0.0 else -math.inf
        j = alpha - k
        log_t0 = log_coef + k * math.log(q) + j * math.log1p(-q)
        log_t1 = log_coef + j * math.log(q) + k * math.log1p(-q)
        log_e0 = math.log(0.5) + _log_erfc((k - z0) / (math.sqrt(2.0) * sigma))
        log_e1 = math.log(0.5) + _log_erfc((z0 - j) / (math.sqrt(2.0) * sigma))
        log_s0 = log_t0 + (k * k - k) / (2.0 * sigma ** 2) + log_e0
        log_s1 = log_t1 + (j * j - j) / (2.0 * sigma ** 2) + log_e1
        if coef > 0:
            log_a0, log_a1 = _log_add(log_a0, log_s0), _log_add(log_a1, log_s1)
        elif coef < 0:
            log_a0, log_a1 = _log_sub(log_a0, log_s0), _log_sub(log_a1, log_s1)
        coef *= (alpha - k) / (k + 1)
        k += 1
        # Past k = alpha the terms alternate and fall like k^-(alpha + 2) (the Gaussian factors cancel), so the tail is
        # below the last term: e^-30 against A >= 1.  Orders near 1 take some 10^4 terms; rdp_sampled_gaussian caches.
        if k > alpha + 1 and max(log_s0, log_s1) < -30.0:
            break
        if k > 1000000:
            raise ArithmeticError("rdp_sampled_gaussian: the fractional-order series did not converge")
    return _log_add(log_a0, log_a1)


def rdp_sampled_gaussian(q, sigma, alpha):
    """Renyi divergence of order alpha > 1 of ONE step of the sampled Gaussian mechanism with sampling probability q
    and noise multiplier sigma (noise standard deviation over sensitivity)."""
    return _rdp(float(q), float(sigma), float(alpha))


@functools.lru_cache(maxsize=4096)
def _rdp(q, sigma, alpha):
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"sampling probability {q} outside [0, 1]")
    if alpha <= 1.0:
        raise ValueError(f"Renyi order {alpha} must exceed 1")
    if q == 0.0:
        return 0.0
    if sigma <= 0.0:
        return math.inf
    if q == 1.0:
        return alpha / (2.0 * sigma ** 2)
    if alpha == math.floor(alpha):
        log_a = _log_a_int(q, sigma, int(alpha))
    else:
        log_a = _log_a_frac(q, sigma, alpha)
    return max(log_a, 0.0) / (alpha - 1.0)


def rdp_release(sigma, sensitivity, alpha):
    """Renyi divergence of order alpha of ONE Gaussian release (no sampling) of a vector in which one record moves one
    entry by `sensitivity`, with noise standard deviation sigma per entry: alpha * sensitivity^2 / (2 sigma^2)."""
    sigma, sensitivity = float(sigma), float(sensitivity)
    if sigma <= 0.0:
        return math.inf
    return alpha * sensitivity ** 2 / (2.0 * sigma ** 2)


def total_rdp(segments, alphas=None, releases=()):
    """[sum over segments (q, sigma, steps) of steps * rdp(q, sigma, alpha), plus the `releases` (sigma, sensitivity) of
    rdp_release, for alpha in alphas]."""
    alphas = DEFAULT_ALPHAS if alphas is None else alphas
    out = [sum(int(t) * rdp_sampled_gaussian(q, s, a) for q, s, t in segments if int(t) > 0) for a in alphas]
    if releases:
        out = [r + sum(rdp_release(s, d, a) for s, d in releases) for a, r in zip(alphas, out)]
    return out


def epsilon(segments, delta, alphas=None, releases=()):
    """(eps, best order) with eps = min over alpha of total RDP + log(1 / delta) / (alpha - 1)."""
    if not 0.0 < delta < 1.0:
        raise ValueError(f"delta {delta} outside (0, 1)")
    alphas = DEFAULT_ALPHAS if alphas is None else alphas
    best = (math.inf, None)
    for a, r in zip(alphas, total_rdp(segments, alphas, releases)):
        e = r + math.log(1.0 / delta) / (a - 1.0)
        if e < best[0]:
            best = (e, a)
    return best


# ---- the capacity of the fixed-size batch ---------------------------------------------------------------------------
def log_binom_tail(n, q, k):
    """log P[Binomial(n, q) > k], summed term by term in log space."""
    n, k = int(n), int(k)
    if k >= n or q <= 0.0:
        return -math.inf
    if k < 0:
        return 0.0
    lq, l1q = math.log(q), math.log1p(-q)
    out = -math.inf
    for j in range(k + 1, n + 1):
        t = _log_comb(n, j) + j * lq + (n - j) * l1q
        out = _log_add(out, t)
        if j > n * q and t < out - 60.0:      # past the mode the terms only fall
            break
    return out


def truncation_cost(n, q, steps, capacity, eps):
    """(1 + e^eps) * T * P[Binomial(n, q) > capacity]: what the dropped-excess event adds to delta."""
    lt = log_binom_tail(n, q, capacity)
    if lt == -math.inf or steps <= 0:
        return 0.0
    x = math.log1p(math.exp(eps)) if eps < 700 else eps
    lg = x + math.log(steps) + lt
    return math.exp(lg) if lg < 700 else math.inf


def capacity_for(n, q, planned_steps, delta, sigma=None, eps=None, alphas=None, spent=0.0):
    """The smallest k with (1 + e^eps) * T * P[Binomial(n, q) > k] <= 0.01 * delta, where eps is the one the T planned
    steps reach at 0.99 * delta (give `sigma`, or that `eps` itself).  `spent` (a resumed run): the truncation
    probability earlier steps have used, Ledger.truncation_mass(); with `eps` the one of ALL steps, the k returned
    keeps (1 + e^eps) * (spent + T * P[...]) within the share — or is n, which truncates nothing, when the earlier steps
    alone no longer fit."""
    n, T = int(n), int(planned_steps)
    if eps is None:
        if sigma is None:
            raise ValueError("capacity_for needs sigma or eps")
        eps = epsilon([(q, sigma, T)], DELTA_SHARE * delta, alphas)[0]
    budget = (1.0 - DELTA_SHARE) * delta
    if spent > 0.0:
        budget -= (1.0 + math.exp(eps)) * spent if eps < 700 else math.inf
        if budget <= 0.0:
            return n
    lo = max(0, math.ceil(q * n) - 1)       # P[X > k] >= ~1/2 below the mean: never within a budget < 1e-2
    while truncation_cost(n, q, T, lo, eps) <= budget and lo > 0:      # (only for a tiny n * q: walk down)
        lo -= 1
    k = lo
    while truncation_cost(n, q, T, k, eps) > budget:
        k += 1
    return max(k, math.ceil(q * n))


# ---- the ledger -----------------------------------------------------------------------------------------------------
class Ledger:
    """What one client's training has spent: (q, sigma, steps) segments, and the facts of the truncated sampler."""

    def __init__(self, n, capacity, delta, planned_steps, alphas=None):
        self.n, self.capacity, self.delta = int(n), int(capacity), float(delta)
        self.planned_steps = int(planned_steps)
        self.alphas = list(DEFAULT_ALPHAS if alphas is None else alphas)
        self.segments = []          # [[q, sigma, steps], ...]
        self.capacities = []        # the capacity each segment's steps ran at
        self.overflow_events = 0
        self.releases = []          # [[sigma, sensitivity, what], ...]: one-off Gaussian releases (add_release)

    def add_release(self, sigma, sensitivity=1.0, what="class counts"):
        """One Gaussian mechanism on a vector in which one record moves one entry by `sensitivity` (a histogram of the
        client's records: one count), noise standard deviation `sigma` per entry, no sampling: alpha * sensitivity^2 /
        (2 sigma^2) at every order, added to the segments' RDP in report()."""
        sigma, sensitivity = float(sigma), float(sensitivity)
        if not sigma > 0.0 or not sensitivity >= 0.0:
            raise ValueError(f"add_release: sigma {sigma} must be positive and sensitivity {sensitivity} non-negative")
        self.releases.append([sigma, sensitivity, str(what)])

    def add_steps(self, q, sigma, steps=1):
        """A changed q, sigma or capacity (a resumed run sizes its own) opens a new segment."""
        q, sigma = float(q), float(sigma)
        if int(steps) <= 0:
            return
        if not 0.0 <= q < 1.0:
            raise ValueError(f"sampling probability {q} outside [0, 1)")
        if (self.segments and self.segments[-1][0] == q and self.segments[-1][1] == sigma
                and self.capacities[-1] == self.capacity):
            self.segments[-1][2] += int(steps)
        else:
            self.segments.append([q, sigma, int(steps)])
            self.capacities.append(self.capacity)

    def truncation_mass(self):
        """sum over the segments of steps * P[Binomial(n, q) > the segment's capacity]: the total-variation distance
        from the untruncated mechanism (multiply by 1 + e^eps for its share of delta)."""
        out = 0.0
        for (q, _, t), k in zip(self.segments, self.capacities):
            lt = log_binom_tail(self.n, q, k)
            out += t * math.exp(lt) if lt > -math.inf else 0.0
        return out

    @property
    def steps(self):
        return sum(s[2] for s in self.segments)

    def report(self):
        """{"epsilon", "delta", "alpha", "steps", "capacity", "overflow_events", "within_plan"}: eps at 0.99 * delta; the
        reported delta is the target while the truncation event fits its 1% share, and 0.99 * delta + its cost after."""
        rel = [(s, d) for s, d, _ in self.releases]
        eps, alpha = (epsilon(self.segments, DELTA_SHARE * self.delta, self.alphas, rel) if self.steps or rel
                      else (0.0, None))
        cost = sum(truncation_cost(self.n, q, t, k, eps) for (q, _, t), k in zip(self.segments, self.capacities))
        ok = cost <= (1.0 - DELTA_SHARE) * self.delta
        return {"epsilon": eps, "delta": self.delta if ok else DELTA_SHARE * self.delta + cost, "alpha": alpha,
                "steps": self.steps, "capacity": self.capacity, "overflow_events": int(self.overflow_events),
                "within_plan": ok}

    def state_dict(self):
        return {"n": self.n, "capacity": self.capacity, "delta": self.delta, "planned_steps": self.planned_steps,
                "alphas": list(self.alphas), "segments": [list(s) for s in self.segments],
                "segment_capacities": list(self.capacities),
                "overflow_events": int(self.overflow_events), "releases": [list(r) for r in self.releases]}

    @classmethod
    def from_state_dict(cls, d):
        led = cls(d["n"], d["capacity"], d["delta"], d["planned_steps"], d["alphas"])
        led.segments = [[float(q), float(s), int(t)] for q, s, t in d["segments"]]
        led.capacities = [int(k) for k in d.get("segment_capacities", [led.capacity] * len(led.segments))]
        led.overflow_events = int(d["overflow_events"])
        led.releases = [[float(s), float(k), str(w)] for s, k, w in d.get("releases", [])]     # (absent before releases)
        return led

    def line(self, name):
        r = self.report()
        q, sigma = (self.segments[-1][0], self.segments[-1][1]) if self.segments else (0.0, 0.0)
        rel = "".join(f", incl. release of {w} at sigma = {s!r}" for s, _, w in self.releases)
        return (f"[dp] {name}: (epsilon, delta) = ({r['epsilon']:.6g}, {r['delta']:.3g}) at order {r['alpha']}, "
                f"q = {q!r}, sigma = {sigma!r}, steps = {r['steps']}, capacity = {r['capacity']}, "
                f"overflow events = {r['overflow_events']}{rel}")
