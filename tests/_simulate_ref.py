"""Exact laws and test statistics for the simulator kernels (csrc/simulate.hip: mm_simulate, mm_std_normal), no GPU:

  gof / conditional_gof     chi-square goodness of fit of an integer sample against an exact pmf, alone or within groups of cells
  nb_quantile_exact         the negative-binomial quantile from extended-precision cumulative sums, with the distances of u to
                            the two CDF steps around the answer and the rounding distance of the device routine
  make / std_normal_ref     the stream keys of include/memento_hip.h restated in uint64 numpy
  CASES                     the (mu, theta) menu of the law tests, each with a planted alternative

tests/test_cpu_simulate_ref.py pins all of it on numpy's own samplers; tests/test_gpu_simulate_kernels.py applies it to the
kernels."""

import numpy as np
import scipy.special
import scipy.stats

MIN_EXPECTED = 20.0           # smallest expected count of a chi-square bin
P_FLOOR = 1e-6                # every law test: p-value of the true law above this ...
P_ALT = 1e-12                 # ... and p-value of the planted alternative below this
N_LAW = 1 << 20               # cells of a law test

# ---------------------------------------------------------------------------------------------------------------------------
# the case menu.  "nb": z ~ NB(mean mu, size theta), alternative NB(mu, theta * alt);  "poisson": theta = 1e12 on the device
# (the gamma mixing moves lambda by 1e-6 relative), law Poisson(mu), alternative Poisson(mu * alt).  The alternatives differ by
# case because the information about theta in a sample does: a 3 % step of theta is rejected at 1e-30 for (9, 2.9) and not at
# all for (0.05, 0.25).  Each is the smallest step of the half-decade ladder 1.0003, 1.001, 1.003, 1.01, 1.03, 1.1, 1.3, 2
# (for the dispersion floor, where only a smaller theta is another law: 0.3, 0.1, ..., 0.001) that numpy's own sample of N_LAW
# cells rejects at P_ALT^2 -- the square, so that another sample of the same size, the kernel's, rejects at P_ALT
# (tests/test_cpu_simulate_ref.py re-derives both: this step is rejected, the step below it is not).
# ---------------------------------------------------------------------------------------------------------------------------
LADDER = [1.0003, 1.001, 1.003, 1.01, 1.03, 1.1, 1.3, 2.0]
LADDER_FLOOR = [0.3, 0.1, 0.03, 0.01, 0.003, 0.001]
CASES = {
    "boost_0.05_0.25": dict(kind="nb", mu=0.05, theta=0.25, alt=1.3),          # a < 1: the boost of the gamma sampler
    "disp_2_0.01": dict(kind="nb", mu=2.0, theta=0.01, alt=1.1),               # extreme dispersion
    "disp_25_0.067": dict(kind="nb", mu=25.0, theta=0.067, alt=1.1),
    "nb_9_2.9": dict(kind="nb", mu=9.0, theta=2.9, alt=1.03),
    "nb_140_25": dict(kind="nb", mu=140.0, theta=25.0, alt=1.03),
    "floor_3_1e5": dict(kind="nb", mu=3.0, theta=1e5, alt=0.001),              # the dispersion floor of simulate_transcriptomes
    "pois_9.5": dict(kind="poisson", mu=9.5, theta=1e12, alt=1.01),            # below the multiplication / PTRS switch
    "pois_10.5": dict(kind="poisson", mu=10.5, theta=1e12, alt=1.01),          # above it
    "pois_300": dict(kind="poisson", mu=300.0, theta=1e12, alt=1.001),
    "pois_5000": dict(kind="poisson", mu=5000.0, theta=1e12, alt=1.0003),
}
# capture laws: the Poisson capture's mean q z scaled (1.03: the ladder step that numpy's capture of the smallest problem, 2^18
# cells, rejects at P_ALT^2), and the urn of the hypergeometric capture doubled (same proportions, the finite-population
# correction of a larger urn)
ALT_CAPTURE_MEAN = 1.03
ALT_URN_SCALE = 2


def nb_pmf(mu, theta):
    n, p = theta, theta / (theta + mu)
    return lambda k: scipy.stats.nbinom.pmf(k, n, p)


def poisson_pmf(lam):
    return lambda k: scipy.stats.poisson.pmf(k, lam)


def case_laws(case):
    """(pmf of the true law, pmf of the planted alternative) of one entry of CASES."""
    if case["kind"] == "nb":
        return nb_pmf(case["mu"], case["theta"]), nb_pmf(case["mu"], case["theta"] * case["alt"])
    return poisson_pmf(case["mu"]), poisson_pmf(case["mu"] * case["alt"])


# ---------------------------------------------------------------------------------------------------------------------------
# chi-square goodness of fit
# ---------------------------------------------------------------------------------------------------------------------------
def gof_bins(expected):
    """The binning rule on the expected counts of the values 0, 1, ..., K: walking upwards from 0, adjacent values are merged
    until the bin's expected count reaches MIN_EXPECTED; whatever is left after the last such bin (a short trailing run and all
    the mass beyond K) belongs to the last bin.  Returns the largest value of every bin but the last (ascending): value v is
    in bin searchsorted(edges, v, 'left')."""
    edges, acc = [], 0.0
    for k, e in enumerate(np.asarray(expected, dtype=np.float64)):
        acc += e
        if acc >= MIN_EXPECTED:
            edges.append(k)
            acc = 0.0
    return np.asarray(edges[:-1], dtype=np.int64)


def gof_stat(sample, pmf):
    """(chi-square, degrees of freedom, bins) of the integer ``sample`` (>= 0) against ``pmf`` (callable on an integer array)."""
    sample = np.asarray(sample).astype(np.int64).ravel()
    n = len(sample)
    assert n > 0 and sample.min() >= 0
    prob = np.asarray(pmf(np.arange(int(sample.max()) + 1)), dtype=np.float64)
    edges = gof_bins(n * prob)
    nb = len(edges) + 1
    cum = np.concatenate([[0.0], np.cumsum(prob)[edges], [1.0]])
    expected = n * np.diff(cum)                                     # the last bin takes the remainder of the mass
    observed = np.bincount(np.searchsorted(edges, sample, side="left"), minlength=nb)
    if nb == 1:
        return 0.0, 0, 1
    return float(((observed - expected) ** 2 / expected).sum()), nb - 1, nb


def gof(sample, pmf):
    """Chi-square goodness of fit: (p-value, number of bins).  One bin (nothing to test) has p-value 1."""
    chi2, df, nb = gof_stat(sample, pmf)
    return (float(scipy.stats.chi2.sf(chi2, df)) if df else 1.0), nb


def conditional_gof(x, key, law, n_keys=30):
    """Law of x given key: cells are grouped by ``key`` (an integer per cell, or an integer row per cell), and within each of
    the ``n_keys`` most frequent keys (ties: the smaller key first) ``x`` is tested against ``law(key)`` (a pmf) by gof_stat;
    the chi-squares and the degrees of freedom add.  Returns (p-value, degrees of freedom, keys used)."""
    x, key = np.asarray(x), np.asarray(key)
    uniq, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.ravel()
    order = np.argsort(-cnt, kind="stable")[:n_keys]
    chi2 = df = used = 0
    for j in order:
        c, d, _ = gof_stat(x[inv == j], law(uniq[j]))
        if d:
            chi2, df, used = chi2 + c, df + d, used + 1
    return (float(scipy.stats.chi2.sf(chi2, df)) if df else 1.0), df, used


def mvhg_code(x, z):
    """A captured vector x of the urn z (three genes) as one integer: the last gene follows from the row sum."""
    return x[..., 0] * (int(z[1]) + 1) + x[..., 1]


def mvhg_pmf(z, s, urn_scale=1):
    """pmf over mvhg_code of the multivariate hypergeometric draw of ``s`` molecules from the urn ``urn_scale * z`` (product form:
    prod_i C(z_i, x_i) / C(T, s)); codes whose vector is impossible have probability 0."""
    z = np.asarray(z, dtype=np.int64)
    zz = z * urn_scale
    lg = scipy.special.gammaln

    def lchoose(n, k):
        return lg(n + 1.0) - lg(k + 1.0) - lg(n - k + 1.0)

    def pmf(code):
        code = np.asarray(code, dtype=np.int64)
        x0, x1 = code // (z[1] + 1), code % (z[1] + 1)
        x2 = s - x0 - x1
        ok = (x0 <= zz[0]) & (x1 <= zz[1]) & (x2 >= 0) & (x2 <= zz[2])
        x0c, x1c, x2c = np.where(ok, x0, 0), np.where(ok, x1, 0), np.where(ok, x2, 0)
        lp = lchoose(zz[0], x0c) + lchoose(zz[1], x1c) + lchoose(zz[2], x2c) - lchoose(zz.sum(), s)
        return np.where(ok, np.exp(lp), 0.0)

    return pmf


# ---------------------------------------------------------------------------------------------------------------------------
# the exact negative-binomial quantile
# ---------------------------------------------------------------------------------------------------------------------------
EPS = 2.0 ** -53              # unit roundoff of the device's fp64
LIBM_ULPS = 4.0               # error allowed to one libm call (lgamma, log, exp, erfc) in units of EPS


def nb_quantile_exact(u, mu, theta):
    """The smallest k with CDF(k) >= u for NB(mean mu, size theta), every u in [0, 1).  Cumulative sums in np.longdouble:
    pmf(0) = p^theta, pmf(k + 1) = pmf(k) (k + theta) / (k + 1) q, upwards from 0.  Returns (k, CDF(k) - u, u - CDF(k - 1),
    margin), float64 but for k; CDF(-1) = 0.  ``margin`` is the rounding distance of the device routine at that k (see
    quantile_margin): where one of the two distances is below it, the device may be one off on that side."""
    L = np.longdouble
    u = np.atleast_1d(np.asarray(u, dtype=np.float64))
    assert ((u >= 0) & (u < 1)).all()
    mu_l, th_l = L(mu), L(theta)
    q = mu_l / (th_l + mu_l)
    pmf0 = np.exp(th_l * np.log1p(-q))
    target = L(u.max())
    chunks, last_pmf, last_cdf, k_next = [], pmf0, pmf0, 1
    cdf_parts, pmf_parts = [np.array([pmf0], dtype=L)], [np.array([pmf0], dtype=L)]
    while last_cdf < target:
        k = np.arange(k_next, k_next + 65536, dtype=L)
        pmf = last_pmf * np.cumprod((k - 1 + th_l) / k * q)
        cdf = last_cdf + np.cumsum(pmf)
        pmf_parts.append(pmf)
        cdf_parts.append(cdf)
        last_pmf, last_cdf, k_next = pmf[-1], cdf[-1], k_next + 65536
        assert k_next < 1 << 27, "the cumulative sum does not reach max(u)"
    pmf, cdf = np.concatenate(pmf_parts), np.concatenate(cdf_parts)
    k = np.searchsorted(cdf, u.astype(L), side="left")
    above = (cdf[k] - u.astype(L)).astype(np.float64)
    below = (u.astype(L) - np.where(k > 0, cdf[np.maximum(k - 1, 0)], L(0))).astype(np.float64)
    return k.astype(np.int64), above, below, quantile_margin(u, k, mu, theta, pmf, cdf)


def stirlerr(n):
    """log n! - log(sqrt(2 pi n) (n / e)^n), as the routine forms it."""
    if n > 15.0:
        nn = n * n
        return (1 / 12 - (1 / 360 - (1 / 1260 - (1 / 1680 - (1 / 1188) / nn) / nn) / nn) / nn) / n
    return scipy.special.gammaln(n + 1.0) - (n + 0.5) * np.log(n) + n - 0.5 * np.log(2 * np.pi)


def bd0(x, m):
    """The deviance x log(x / m) + m - x (its value; the routine sums a series where x is close to m)."""
    return float(x * np.log(np.longdouble(x) / np.longdouble(m)) + np.longdouble(m) - np.longdouble(x))


def quantile_margin(u, k, mu, theta, pmf, cdf):
    """How far the device's running sum at k can be from CDF(k), relative to its u -- from the routine's own arithmetic, not from
    what it returns.  With EPS = 2^-53 and LIBM_ULPS per libm call:
      - the start term at k0 = max(0, floor(mu - 9 sd)): for k0 = 0, exp(theta log p); above, the exponential of the sum of
        stirlerr(n), stirlerr(theta), stirlerr(k0), bd0(theta, n p), bd0(k0, n q), n = k0 + theta, times a prefactor of six
        operations.  Every term t of the exponent carries (LIBM_ULPS + 5) EPS |t| (its calls, its own few operations or the
        tail of its series, and its share of the additions), so the exponent an absolute error A EPS, A = (LIBM_ULPS + 5) sum |t|,
        which exp() turns into a relative error of every pmf; exp() and the prefactor add LIBM_ULPS + 6;
      - each step of the recurrence multiplies by a rounded ratio of four operations: pmf(j) carries 4 (j - k0) EPS more;
      - so |sum - CDF(k)| <= EPS * sum_{j <= k} pmf(j) (A + LIBM_ULPS + 6 + 4 (j - k0)), the compensated summation adding 2 EPS;
      - u = erfc(-y / sqrt 2) / 2 carries LIBM_ULPS + 1 roundings of its own size;
      - the extended-precision reference: 2^-63 (|theta log p| + 4 k) CDF(k)."""
    p, q = theta / (theta + mu), mu / (theta + mu)
    sd = np.sqrt(mu + mu * mu / theta)
    k0 = np.floor(max(0.0, mu - 9.0 * sd))
    if k0 > 0:
        n = k0 + theta
        terms = np.abs([stirlerr(n), stirlerr(theta), stirlerr(k0), bd0(theta, n * p), bd0(k0, n * q)])
    else:
        terms = np.abs([theta * np.log(p)])
    A = (LIBM_ULPS + 5.0) * terms.sum()
    j = np.arange(len(pmf), dtype=np.float64)
    w = np.cumsum((pmf * np.maximum(j - k0, 0.0)).astype(np.float64))
    c = cdf[k].astype(np.float64)
    dev = EPS * ((A + LIBM_ULPS + 6.0) * c + 4.0 * w[k] + 2.0)
    ref = 2.0 ** -63 * (abs(theta * np.log(p)) + 4.0 * k) * c
    return dev + EPS * (LIBM_ULPS + 1.0) * np.asarray(u) + ref


def excused(got, want, above, below, margin):
    """Element-wise: got == want, or one off on the side where u lies within ``margin`` of the CDF step."""
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    above, below = np.asarray(above, dtype=np.float64), np.asarray(below, dtype=np.float64)
    return (got == want) | ((got == want + 1) & (above <= margin)) | ((got == want - 1) & (below <= margin))


# ---------------------------------------------------------------------------------------------------------------------------
# the stream keys (include/memento_hip.h, mm_simulate)
# ---------------------------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
TAG_CAPTURE = (1 << 32) | 0x5EED
TAG_NORMAL = (2 << 32) | 0x6A55


def mix(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def make(seed, a, b):
    """Start state of the stream (seed, a, b); a and b may be arrays."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return mix(np.uint64(seed & M64) ^ mix(a * np.uint64(GOLDEN) + np.uint64(0x632BE59BD9B4E019)) ^ mix(b + np.uint64(0xD1B54A32D192ED03)))


def uniform_at(state, n):
    """The n-th uniform (n = 1, 2, ...) of the streams that start at ``state``."""
    with np.errstate(over="ignore"):
        bits = mix(np.asarray(state, dtype=np.uint64) + np.uint64((n * GOLDEN) & M64))
    return ((bits >> np.uint64(11)).astype(np.float64) + 0.5) / 9007199254740992.0


def std_normal_ref(seed, n, tag=TAG_NORMAL):
    """mm_std_normal in fp64 numpy: one Box-Muller pair per element, the cosine branch."""
    s = make(seed, np.arange(n, dtype=np.uint64), tag)
    return np.sqrt(-2.0 * np.log(uniform_at(s, 1))) * np.cos(2.0 * np.pi * uniform_at(s, 2))


def first_nb_normal_ref(seed, cells, gene):
    """The first Box-Muller proposal inside the NB draw of (cell, gene): what a colliding normal stream would repeat."""
    s = make(seed, np.asarray(cells, dtype=np.uint64), gene)
    return np.sqrt(-2.0 * np.log(uniform_at(s, 1))) * np.cos(2.0 * np.pi * uniform_at(s, 2))


# ---------------------------------------------------------------------------------------------------------------------------
# bounds shared by the CPU pins and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def corr_bound(n, n_tests, level=P_FLOOR):
    """Two-sided Bonferroni bound on a sample correlation of n independent pairs, r sqrt(n) ~ N(0, 1), over n_tests tests."""
    return float(scipy.stats.norm.isf(level / (2.0 * n_tests)) / np.sqrt(n))


def corr_columns(a, b=None):
    """Correlation matrix of the columns of a (with those of b), fp64."""
    a = np.asarray(a, dtype=np.float64)
    a = (a - a.mean(axis=0)) / a.std(axis=0)
    if b is None:
        return a.T @ a / len(a)
    b = np.asarray(b, dtype=np.float64)
    b = (b - b.mean(axis=0)) / b.std(axis=0)
    return a.T @ b / len(a)


def lag_corr(x, lag):
    x = np.asarray(x, dtype=np.float64)
    x = (x - x.mean()) / x.std()
    return float((x[:-lag] * x[lag:]).mean())


def normal_report(x):
    """The statistics of the mm_std_normal test on a vector x: KS p-value, chi-square p-value on 64 equiprobable bins, the count
    beyond +-4 with its exact binomial interval at P_FLOOR, the autocorrelations at lags 1, 64, 256 and their bound."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    edges = scipy.stats.norm.ppf(np.arange(1, 64) / 64.0)
    obs = np.bincount(np.searchsorted(edges, x), minlength=64)
    chi2 = float(((obs - n / 64.0) ** 2 / (n / 64.0)).sum())
    p_tail = 2.0 * scipy.stats.norm.sf(4.0)
    lo, hi = scipy.stats.binom.interval(1.0 - P_FLOOR, n, p_tail)
    return dict(ks_p=float(scipy.stats.kstest(x, "norm").pvalue), chi2_p=float(scipy.stats.chi2.sf(chi2, 63)),
                tail=int((np.abs(x) > 4.0).sum()), tail_lo=int(lo), tail_hi=int(hi),
                acorr={lag: lag_corr(x, lag) for lag in (1, 64, 256)}, acorr_bound=5.5 / np.sqrt(n))


def check_normal_report(r):
    assert r["ks_p"] > P_FLOOR and r["chi2_p"] > P_FLOOR, r
    assert r["tail_lo"] <= r["tail"] <= r["tail_hi"], r
    assert all(abs(v) < r["acorr_bound"] for v in r["acorr"].values()), r


# ---------------------------------------------------------------------------------------------------------------------------
# the quantile menu: (mu, theta) and the hand-made scores
# ---------------------------------------------------------------------------------------------------------------------------
QCASES = [(0.05, 0.25), (1.0, 0.1), (1.0, 0.01), (50.0, 0.02), (5.0, 0.05), (9.0, 2.9), (140.0, 25.0), (2500.0, 62500.0), (1e4, 1e5)]
SCORE_MAX = 6.5               # what 2e10 standard normals reach


def phi(y):
    """Phi(y) in fp64 as the device forms it: erfc(-y / sqrt 2) / 2."""
    return 0.5 * scipy.special.erfc(-np.asarray(y, dtype=np.float64) * 0.70710678118654752440)


def quantile_scores(mu, theta, n_grid=521, n_steps=48):
    """float32 scores: a regular grid over [-SCORE_MAX, SCORE_MAX], and around n_steps CDF steps spread over the same range the
    float32 neighbours of the score whose Phi is the step (the nearest float32 and the next one on either side)."""
    grid = np.linspace(-SCORE_MAX, SCORE_MAX, n_grid).astype(np.float32)
    at = np.linspace(-SCORE_MAX, SCORE_MAX, n_steps + 2)[1:-1]
    k, above, _, _ = nb_quantile_exact(phi(at), mu, theta)
    step = phi(at) + above                                           # CDF(k): a step at or just above Phi(at)
    step = step[(step > 0) & (step < 1)]
    y = scipy.stats.norm.ppf(step)
    y = np.where(step > 0.5, -scipy.stats.norm.isf(step), y).astype(np.float32)
    near = np.concatenate([np.nextafter(y, np.float32(-np.inf)), y, np.nextafter(y, np.float32(np.inf))])
    near = near[np.abs(near) <= SCORE_MAX]
    return np.unique(np.concatenate([grid, near]))
