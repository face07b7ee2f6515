"""The rule by which the sweep's refinement drops a hypothesis
(refine_costs_compact): with non-negative terms summed in fp32, a prefix with
prefix / wn >= b implies final / wn >= b, so the consumer's `final / wn < b`
is false. Checked in numpy fp32 (round-to-nearest, IEEE division, as on the
device) on random and adversarial inputs: ties, subnormals, weights 1..15, up
to 31 terms in [0, 2.6], NaN and infinite terms. A cheaper threshold that
replaces the division must pass the same check.
"""
import numpy as np

F = np.float32


def _check(w, c, b):
    """w, c: (cases, terms) fp32; b: (cases,) fp32 bounds."""
    wn = np.zeros(len(w), F)
    for j in range(w.shape[1]):  # the kernel's weight_norm: ascending j
        wn = (wn + w[:, j]).astype(F)
    acc = np.zeros(len(w), F)
    dead = np.zeros(len(w), bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(w.shape[1]):
            acc = (acc + (w[:, j] * c[:, j]).astype(F)).astype(F)
            dead |= (acc / wn).astype(F) >= b
        final_wins = (acc / wn).astype(F) < b
    assert not (dead & final_wins).any()
    return dead


def test_random_sums():
    rng = np.random.default_rng(7)
    n = 200000
    for terms in (1, 2, 5, 9, 31):
        w = rng.integers(1, 16, (n, terms)).astype(F)
        c = rng.uniform(0, 2.6, (n, terms)).astype(F)
        # bounds spread round the mean cost, so prefixes land on both sides
        b = rng.uniform(0, 2.6, n).astype(F)
        dead = _check(w, c, b)
        assert 0.05 < dead.mean() < 0.999


def test_ties_and_constant_costs():
    rng = np.random.default_rng(8)
    n = 100000
    for terms in (2, 9, 31):
        w = rng.integers(1, 16, (n, terms)).astype(F)
        k = rng.choice(np.array([0.0, 2.0, 1.0, 0.3, 2.6], F), n)
        c = np.repeat(k[:, None], terms, 1)
        # the bound is the cost itself, or one ulp to either side
        b = np.stack([k, np.nextafter(k, F(3)), np.nextafter(k, F(-1))])[rng.integers(0, 3, n), np.arange(n)]
        _check(w, c, b.astype(F))


def test_subnormal_and_tiny_terms():
    rng = np.random.default_rng(9)
    n = 100000
    tiny = np.array([0.0, 1e-45, 1e-40, 1.1754944e-38, 2.0 ** -24, 6e-8], F)
    for terms in (3, 31):
        w = rng.integers(1, 16, (n, terms)).astype(F)
        c = rng.choice(tiny, (n, terms))
        c[rng.random((n, terms)) < 0.2] = F(2.0)  # large terms that absorb the tiny ones
        b = rng.choice(np.concatenate([tiny, np.array([2.0, 0.5], F)]), n)
        _check(w, c, b)


def test_nan_and_infinite_terms():
    rng = np.random.default_rng(10)
    n = 100000
    w = rng.integers(1, 16, (n, 9)).astype(F)
    c = rng.uniform(0, 2.6, (n, 9)).astype(F)
    c[rng.random((n, 9)) < 0.1] = np.nan
    c[rng.random((n, 9)) < 0.1] = np.inf
    b = rng.uniform(0, 2.6, n).astype(F)
    b[rng.random(n) < 0.1] = np.nan
    dead = _check(w, c, b)
    assert not dead[np.isnan(b)].any()  # a NaN bound drops nothing
