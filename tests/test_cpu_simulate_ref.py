"""The exact laws and test statistics of tests/_simulate_ref.py checked on their own (no GPU), so that the conditions
tests/test_gpu_simulate_kernels.py puts on the simulator kernels are conditions a correct sampler meets: numpy's negative
binomial, Poisson, hypergeometric and standard-normal samples, at the cell counts of the GPU tests and fixed seeds, pass every
bound applied there, and reject every planted alternative; the extended-precision quantile equals 40-digit sums; the binning
rule, the key grouping and the tie margins do what they say on hand-made inputs; the stream keys collide where the old tags
did and nowhere with the new ones."""

import numpy as np
import pytest
import scipy.stats

import _simulate_ref as R
from _simulate_ref import CASES, N_LAW, P_ALT, P_FLOOR


@pytest.fixture(scope="module")
def samples():
    """numpy's sample of every case, drawn in the order of CASES from one generator."""
    rng = np.random.default_rng(20261021)
    out = {}
    for name, c in CASES.items():
        if c["kind"] == "nb":
            out[name] = rng.negative_binomial(c["theta"], c["theta"] / (c["theta"] + c["mu"]), size=N_LAW)
        else:
            out[name] = rng.poisson(c["mu"], size=N_LAW)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_numpy_sample_passes_and_rejects_the_planted_alternative(samples, name):
    c, s = CASES[name], samples[name]
    law, alt = R.case_laws(c)
    p, nb = R.gof(s, law)
    p_alt, _ = R.gof(s, alt)
    assert p > P_FLOOR and nb >= 5, (p, nb)
    assert p_alt < P_ALT ** 2, p_alt
    # the step below on the ladder is not rejected at that level: the planted step is the smallest that is
    ladder = R.LADDER_FLOOR if c["alt"] < 1 else R.LADDER
    i = ladder.index(c["alt"])
    if i > 0:
        below = dict(c, alt=ladder[i - 1])
        assert R.gof(s, R.case_laws(below)[1])[0] >= P_ALT ** 2


def _capture_law(q, scale=1.0):
    return lambda z: R.poisson_pmf(q * scale * float(z))


@pytest.mark.parametrize("n,zlaw,q", [(1 << 18, ("nb", 6.0, 2.0), 0.5), (N_LAW, ("poisson", 6.0), 0.3), (N_LAW, ("poisson", 60.0), 0.25)])
def test_numpy_poisson_capture_passes_the_conditional_law(n, zlaw, q):
    rng = np.random.default_rng(7)
    z = rng.negative_binomial(zlaw[2], zlaw[2] / (zlaw[2] + zlaw[1]), size=n) if zlaw[0] == "nb" else rng.poisson(zlaw[1], size=n)
    x = rng.poisson(q * z)
    p, df, used = R.conditional_gof(x, z, _capture_law(q))
    assert p > P_FLOOR and used >= 15 and df >= 100, (p, df, used)
    assert R.conditional_gof(x, z, _capture_law(q, R.ALT_CAPTURE_MEAN))[0] < P_ALT ** 2


def hyper_rows(q, T):
    return np.minimum(np.rint(q * T), T).astype(np.int64)


def test_numpy_hypergeometric_capture_passes_the_vector_law():
    rng = np.random.default_rng(8)
    q = 0.4
    Z = rng.poisson([2, 3, 1], size=(N_LAW, 3))
    T = Z.sum(axis=1)
    S = hyper_rows(q, T)
    rest = Z[:, 1] + Z[:, 2]
    x0 = np.where(T > 0, rng.hypergeometric(Z[:, 0], rest + (T == 0), np.where(T > 0, S, 0)), 0)
    x1 = np.where(rest > 0, rng.hypergeometric(Z[:, 1], Z[:, 2] + (rest == 0), np.where(rest > 0, S - x0, 0)), 0)
    X = np.stack([x0, x1, S - x0 - x1], axis=1)
    assert (X >= 0).all() and (X <= Z).all()

    def law(scale):
        return lambda z: R.mvhg_pmf(z, int(hyper_rows(q, z.sum())), scale)

    code = X[:, 0] * (Z[:, 1] + 1) + X[:, 1]
    p, df, used = R.conditional_gof(code, Z, law(1))
    assert p > P_FLOOR and used >= 20 and df >= 50, (p, df, used)
    assert R.conditional_gof(code, Z, law(R.ALT_URN_SCALE))[0] < P_ALT ** 2


def test_mvhg_pmf_is_the_product_form():
    z, s = np.array([3, 4, 2]), 4
    pmf = R.mvhg_pmf(z, s)
    codes = np.arange((z[0] + 1) * (z[1] + 1))
    pr = pmf(codes)
    assert abs(pr.sum() - 1) < 1e-12
    mh = pytest.importorskip("scipy.stats").multivariate_hypergeom
    for c in codes:
        x0, x1 = c // (z[1] + 1), c % (z[1] + 1)
        x2 = s - x0 - x1
        want = mh.pmf([x0, x1, x2], z, s) if 0 <= x2 <= z[2] else 0.0
        assert abs(pr[c] - want) < 1e-12, (c, pr[c], want)
    assert R.mvhg_code(np.array([[2, 1, 1]]), z)[0] == 2 * 5 + 1


def test_numpy_normals_pass_the_normal_report():
    rng = np.random.default_rng(9)
    x = rng.standard_normal(N_LAW).astype(np.float32)
    r = R.normal_report(x)
    R.check_normal_report(r)
    assert (r["tail_lo"], r["tail_hi"]) == (31, 110)                   # Binomial(2^20, 2 Phi(-4)): mean 66.4
    y = rng.standard_normal(N_LAW).astype(np.float32)
    assert abs(R.corr_columns(x[:, None], y[:, None])[0, 0]) < 5.5 / np.sqrt(N_LAW)
    # a sampler whose tails are cut at 4 sd, and one with a lag-64 echo, fail it
    bad = R.normal_report(np.clip(x, -4, 4))
    assert bad["tail"] < bad["tail_lo"]
    echo = x.copy()
    echo[64:] += 0.01 * x[:-64]
    assert abs(R.normal_report(echo)["acorr"][64]) > 5.5 / np.sqrt(N_LAW)


def test_numpy_columns_pass_the_independence_bounds():
    rng = np.random.default_rng(10)
    n, G = 1 << 16, 64
    Z = rng.negative_binomial(2.9, 2.9 / (2.9 + 9.0), size=(n, G))
    bound = R.corr_bound(n, G * (G - 1) // 2)
    assert 0.0242 < bound < 0.0244                                       # 6.22 / sqrt(2^16): isf(1e-6 / 4032)
    C = R.corr_columns(Z)
    assert np.abs(C[~np.eye(G, dtype=bool)]).max() < bound
    assert max(abs(R.lag_corr(Z[:, g], 1)) for g in range(G)) < bound
    Z2 = Z.copy()
    Z2[:, 5] = Z[:, 4] + (rng.random(n) < 0.05)                          # a shared stream shows at once
    assert np.abs(R.corr_columns(Z2)[4, 5]) > bound


# ---- gof: binning rule and key grouping on hand-made inputs ---------------------------------------------------------------
def test_binning_rule():
    # expected counts 30 | 5 + 16 | 19.5 + 0.5 | 25 | 3 + 1: four closed bins, the trailing run joins the last
    e = [30, 5, 16, 19.5, 0.5, 25, 3, 1]
    np.testing.assert_array_equal(R.gof_bins(e), [0, 2, 4])
    assert len(R.gof_bins([5, 5, 5])) == 0 and len(R.gof_bins([25])) == 0  # one bin: nothing to test
    np.testing.assert_array_equal(R.gof_bins([20, 20, 19.99]), [0])
    # a sample with exactly the expected counts has chi-square 0; the mass beyond the sample's maximum is in the last bin
    pmf = lambda k: np.array([0.3, 0.05, 0.16, 0.195, 0.005, 0.25, 0.03, 0.01])[k]
    sample = np.repeat([0, 1, 2, 3, 4, 5, 6], [30, 5, 16, 19, 1, 25, 4])
    chi2, df, nb = R.gof_stat(sample, pmf)
    assert (df, nb) == (3, 4) and chi2 < 1e-20
    moved = np.repeat([0, 1, 2, 3, 4, 5, 6], [40, 5, 16, 19, 1, 15, 4])    # 10 cells moved from the last bin to the first
    chi2, df, _ = R.gof_stat(moved, pmf)
    assert abs(chi2 - (100 / 30 + 100 / 29)) < 1e-9
    p, nb = R.gof(moved, pmf)
    assert abs(p - scipy.stats.chi2.sf(100 / 30 + 100 / 29, 3)) < 1e-12 and nb == 4
    assert R.gof(np.zeros(10, dtype=int), lambda k: np.ones(len(k))) == (1.0, 1)


def test_key_grouping():
    rng = np.random.default_rng(3)
    key = np.repeat([5, 2, 9, 7], [4000, 3000, 50, 3000])
    x = rng.poisson(0.5 * key)
    seen = []

    def law(k):
        seen.append(int(k))
        return R.poisson_pmf(0.5 * float(k))

    p, df, used = R.conditional_gof(x, key, law, n_keys=3)
    assert seen == [5, 2, 7] and used == 3 and p > 1e-4                    # most frequent first, ties by key; 9 is left out
    sep = [R.gof_stat(x[key == k], R.poisson_pmf(0.5 * k)) for k in (5, 2, 7)]
    assert df == sum(s[1] for s in sep)
    assert abs(scipy.stats.chi2.isf(p, df) - sum(s[0] for s in sep)) < 1e-6
    # vector keys: rows are grouped as a whole
    key2 = np.stack([key, key % 2], axis=1)
    got = []
    R.conditional_gof(x, key2, lambda k: (got.append(tuple(int(v) for v in k)), R.poisson_pmf(0.5 * float(k[0])))[1], n_keys=2)
    assert got == [(5, 1), (2, 0)]
    # a wrong law within one key only is found
    x_bad = np.where(key == 2, rng.poisson(1.3, size=len(key)), x)
    assert R.conditional_gof(x_bad, key, lambda k: R.poisson_pmf(0.5 * float(k)), n_keys=3)[0] < 1e-12


# ---- the exact quantile -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu,theta", R.QCASES)
def test_exact_quantile_equals_forty_digit_sums(mu, theta):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    y = np.linspace(-R.SCORE_MAX, R.SCORE_MAX, 401).astype(np.float32)
    u = R.phi(y)
    k, above, below, margin = R.nb_quantile_exact(u, mu, theta)
    m, t = mp.mpf(mu), mp.mpf(theta)
    q = m / (m + t)
    pmf = mp.exp(t * mp.log(t / (m + t)))
    cdf, j, prev = pmf, 0, mp.mpf(0)
    for i in np.argsort(u, kind="stable"):
        ui = mp.mpf(float(u[i]))
        while cdf < ui:
            pmf *= (j + t) / (j + 1) * q
            j += 1
            prev, cdf = cdf, cdf + pmf
        assert k[i] == j, (y[i], k[i], j)
        tol = 1e-18 + 2.0 ** -63 * (abs(theta * np.log(theta / (theta + mu))) + 4.0 * j)      # the reference's own rounding
        assert abs(float(cdf - ui) - above[i]) <= tol + 2.0 ** -52 * above[i]        # (and fp64 holds the distance)
        assert abs(float(ui - prev) - below[i]) <= tol + 2.0 ** -52 * below[i] or j == 0
    assert (above >= 0).all() and (below > 0).all() and (margin > 0).all()


def test_exact_quantile_against_scipy_and_the_reported_cap():
    """scipy's ppf agrees away from ties, and two over-dispersed genes: the former cap mu + 40 sd + 60 lies below the exact
    quantile at high scores."""
    for mu, theta in R.QCASES[:7]:
        y = np.linspace(-5.5, 5.5, 401).astype(np.float32)
        u = R.phi(y)
        k, above, below, margin = R.nb_quantile_exact(u, mu, theta)
        clear = (above > 1e-13 * np.maximum(u, 1e-3)) & (below > 1e-13 * np.maximum(u, 1e-3))
        want = scipy.stats.nbinom.ppf(u, theta, theta / (theta + mu))
        assert clear.mean() > 0.95
        np.testing.assert_array_equal(k[clear], want[clear])
    for mu, theta, cap in ((1.0, 0.01, 463), (50.0, 0.02, 14255)):
        assert int(mu + 40 * np.sqrt(mu + mu * mu / theta) + 60) in (cap - 1, cap, cap + 1)
        k = R.nb_quantile_exact(R.phi(np.float32([4.0, 4.5, 5.5, 6.5])), mu, theta)[0]
        assert k[0] < cap < k[1] < k[2] < k[3], k


def test_tie_margins():
    mu, theta = 9.0, 2.9
    k, above, below, margin = R.nb_quantile_exact(np.array([0.5]), mu, theta)
    cdf = scipy.stats.nbinom.cdf(np.arange(40), theta, theta / (theta + mu))
    assert k[0] == np.searchsorted(cdf, 0.5) and abs(above[0] - (cdf[k[0]] - 0.5)) < 1e-14 and abs(below[0] - (0.5 - cdf[k[0] - 1])) < 1e-14
    assert 10 * R.EPS < margin[0] < 300 * R.EPS                            # theta log p = -4.1, a dozen recurrence steps
    # u exactly one ulp above / below a CDF step
    step = float(cdf[7])
    lo, hi = np.nextafter(step, 0.0), np.nextafter(step, 1.0)
    k, above, below, margin = R.nb_quantile_exact(np.array([lo, hi]), mu, theta)
    assert (k[1] == k[0] + 1 == 8) or (k[0] == k[1] == 7) or (k[0] == k[1] == 8)  # (scipy's own cdf is rounded: either side)
    assert (np.minimum(above, below) < margin).all()
    # excused(): only one off, and only on the side where u is close
    want, ab, be, mg = np.array([7, 7, 7, 7, 7]), np.array([1e-17, 1e-17, 0.1, 0.1, 1e-17]), np.array([0.1, 0.1, 1e-17, 0.1, 1e-17]), 1e-15
    np.testing.assert_array_equal(R.excused([8, 6, 6, 8, 9], want, ab, be, mg), [True, False, True, False, False])
    assert R.excused([7], [7], [0.1], [0.1], 0.0).all()
    # a start above 0: the saddle-point terms are of the size of log pmf(k0), not of lgamma(k0 + theta)
    k, _, _, big = R.nb_quantile_exact(np.array([0.5]), 1e4, 1e5)
    assert abs(R.bd0(9055.0, 109055.0 / 11) - 38.0) < 2 and abs(R.stirlerr(20.0) - (scipy.special.gammaln(21.0) - 20.5 * np.log(20.0) + 20 - 0.5 * np.log(2 * np.pi))) < 1e-13
    assert margin[0] < big[0] < 1e-12                                        # (the lgamma form: 1e6 * EPS * 9 = 1e-9)


def test_quantile_scores_sit_on_both_sides_of_steps():
    for mu, theta in [(9.0, 2.9), (1.0, 0.01)]:
        y = R.quantile_scores(mu, theta)
        assert y.dtype == np.float32 and np.abs(y).max() <= R.SCORE_MAX and len(y) >= 521 + 30
        k = R.nb_quantile_exact(R.phi(y), mu, theta)[0]
        assert (np.diff(k) >= 0).all()
        d = np.diff(y.astype(np.float64))
        adjacent = d <= 1.01 * np.spacing(np.abs(y[:-1])).astype(np.float64)
        assert (adjacent & (np.diff(k) == 1)).sum() >= 10                # neighbouring float32 scores with different quantiles


# ---- stream keys ----------------------------------------------------------------------------------------------------------
def test_stream_keys():
    cells = np.arange(1000)
    for seed in (0, 42343, 2 ** 63 + 5):
        # the tags before this scheme were gene indices: the capture stream of a cell was the NB stream of (cell, gene 24301)
        np.testing.assert_array_equal(R.make(seed, cells, 0x5EED), R.make(seed, cells, 24301))
        np.testing.assert_array_equal(R.make(seed, cells, 0x6A55), R.make(seed, cells, 27221))
        for tag in (R.TAG_CAPTURE, R.TAG_NORMAL):
            assert tag >= 2 ** 32
            assert not (R.make(seed, cells, tag) == R.make(seed, cells, tag & 0xFFFF)).any()
    assert R.TAG_CAPTURE != R.TAG_NORMAL
    # mix is a bijection: distinct b, distinct states (sampled)
    b = np.concatenate([np.arange(40000), [R.TAG_CAPTURE, R.TAG_NORMAL]]).astype(np.uint64)
    assert len(np.unique(R.make(7, 3, b))) == len(b)
    x = R.std_normal_ref(5, 1 << 16)
    assert abs(x.mean()) < 5 / 256 and abs(x.std() - 1) < 0.02
    np.testing.assert_array_equal(R.std_normal_ref(5, 100, tag=27221), R.first_nb_normal_ref(5, np.arange(100), 27221))
