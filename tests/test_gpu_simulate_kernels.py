"""The simulator kernels (csrc/simulate.hip: mm_simulate, mm_std_normal) through the C-ABI on hand-built parameter arrays, each
law against its exact statement (tests/_simulate_ref.py; tests/test_cpu_simulate_ref.py shows that numpy's samplers meet the
same conditions at the same sizes):

  A  the NB draw against scipy's pmf by chi-square, incl. the a < 1 boost, extreme dispersion, the dispersion floor and the
     Poisson limit either side of the multiplication / PTRS switch; dead genes; totals == row sums
  B  mm_std_normal: KS, chi-square, tails, autocorrelation, seeds, prefix property, edge sizes, the documented key
  C  independence across genes, cells and seeds; a count is a pure function of (seed, cell, gene)
  D  the three stream families do not meet, whatever the seeds
  E  the capture laws conditional on the transcriptome: multivariate hypergeometric (vector law, exact row sums with ties to
     even, q = 0 and 1) and Poisson (multiplication and PTRS), per-cell rates
  F  structure of the three passes, sentinels, edge sizes, argument checks
  G  the copula quantile on hand-made scores against extended-precision sums, one off only within the routine's own rounding
     distance of a CDF step; +-inf and NaN scores

Every law test also rejects a planted alternative (a wrong theta / Poisson mean / urn) at p < 1e-12, so none is vacuous.  The
figures each test sees are printed (pytest -s), profiles/simulate_kernel_tests.txt records them."""

import numpy as np
import pytest
import scipy.stats

import _simulate_ref as R
from _simulate_ref import CASES, N_LAW, P_ALT, P_FLOOR

pytestmark = pytest.mark.gpu

SENT = -7777                                            # sentinel of every output buffer
PAD = 8


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


def _report(test, **figures):
    print("SIMK", test, " ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()), flush=True)


def _full(eng, n, dtype, value=SENT):
    import torch

    return torch.full((n + PAD,), value, dtype=dtype, device="cuda")


def _tail_ok(eng, t, n, value=SENT):
    return bool((eng.host(t[n:]) == value).all())


class Sim:
    """One parameter set on the device; every pass is one mm_simulate call with sentinel-padded outputs, whose tails are
    checked after every call."""

    def __init__(self, eng, mu, theta, n_cells, seed_z, gauss=None):
        import torch

        self.eng, self.n, self.G, self.seed_z = eng, int(n_cells), len(mu), int(seed_z)
        self.d_mu, self.d_theta = eng.dev(np.asarray(mu, dtype=np.float64)), eng.dev(np.asarray(theta, dtype=np.float64))
        self.d_gauss = None if gauss is None else eng.dev(np.ascontiguousarray(gauss, dtype=np.float32))
        self.d_raw = None
        if gauss is not None:
            self.d_raw = _full(eng, self.n, torch.int64)
            self.call(2, 3)
            assert _tail_ok(eng, self.d_raw, self.n)

    def call(self, process, mode, d_qs=None, seed_c=0, totals=None, row_nnz=None, row_ptr=None, idx=None, val=None):
        P = self.eng.P
        self.eng._lib.call("mm_simulate", P(self.d_mu), P(self.d_theta), self.G, self.n, P(d_qs),
                           self.seed_z, int(seed_c), int(process), int(mode), P(totals), P(row_nnz), P(row_ptr), P(idx), P(val),
                           P(self.d_gauss), P(None), P(self.d_raw), self.eng._stream())

    def totals(self):
        import torch

        t = _full(self.eng, self.n, torch.int64)
        self.call(2, 0, totals=t)
        assert _tail_ok(self.eng, t, self.n)
        return t

    def csr(self, process=2, qs=None, seed_c=0):
        """(indptr, indices, data) on the host after the count and the write pass; process 0 runs the totals pass first."""
        import torch

        eng, n = self.eng, self.n
        d_qs = None if qs is None else eng.dev(np.broadcast_to(np.asarray(qs, dtype=np.float64), (n,)).copy() if n else np.zeros(1))
        totals = self.totals() if process == 0 else None
        nnz_row = _full(eng, n, torch.int64)
        self.call(process, 1, d_qs, seed_c, totals=totals, row_nnz=nnz_row)
        assert _tail_ok(eng, nnz_row, n)
        counts = eng.host(nnz_row[:n])
        assert (counts >= 0).all() and (counts <= self.G).all()
        indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        nnz = int(indptr[-1])
        idx, val = _full(eng, nnz, torch.int32), _full(eng, nnz, torch.float32, float(SENT))
        self.call(process, 2, d_qs, seed_c, totals=totals, row_ptr=eng.dev(indptr), idx=idx, val=val)
        assert _tail_ok(eng, idx, nnz) and _tail_ok(eng, val, nnz, float(SENT))
        if totals is not None:
            assert _tail_ok(eng, totals, n)
        i, v = eng.host(idx[:nnz]), eng.host(val[:nnz])
        # canonical rows: every cell of the CSR written, indices ascending within a row, data positive integers
        assert (i >= 0).all() and (i < self.G).all() and (v > 0).all() and (v == np.rint(v)).all()
        inner = np.ones(nnz, dtype=bool)
        inner[indptr[:-1][counts > 0]] = False
        assert (np.diff(i.astype(np.int64), prepend=-1)[inner] > 0).all()
        return indptr, i, v

    def dense(self, **kw):
        return _dense(self.csr(**kw), self.n, self.G)


def _dense(csr, n, G):
    indptr, idx, val = csr
    Z = np.zeros((n, G), dtype=np.int64)
    Z[np.repeat(np.arange(n), np.diff(indptr)), idx] = val.astype(np.int64)
    return Z


def _column(csr, n, g):
    indptr, idx, val = csr
    at = np.flatnonzero(idx == g)
    out = np.zeros(n, dtype=np.int64)
    out[np.searchsorted(indptr, at, side="right") - 1] = val[at].astype(np.int64)
    return out


def _std_normal(eng, seed, n, size=None):
    import torch

    out = torch.full(((n if size is None else size) + PAD,), float(SENT), dtype=torch.float32, device="cuda")
    eng._lib.call("mm_std_normal", int(seed), n, eng.P(out), eng._stream())
    return eng.host(out)


# -------------------------------------------------------------------------------------------------
# A. the NB law
# -------------------------------------------------------------------------------------------------
DEAD = [0.0, -1.0, np.nan]


@pytest.fixture(scope="module")
def nb_launch(eng):
    """One launch of N_LAW cells: a gene per case of CASES, then the dead genes (mean 0, < 0, NaN)."""
    mu = [c["mu"] for c in CASES.values()] + DEAD
    theta = [c["theta"] for c in CASES.values()] + [1.0] * len(DEAD)
    sim = Sim(eng, mu, theta, N_LAW, seed_z=1234)
    return sim, sim.dense()


@pytest.mark.parametrize("name", list(CASES))
def test_nb_draw_follows_its_law(nb_launch, name):
    _, Z = nb_launch
    z = Z[:, list(CASES).index(name)]
    law, alt = R.case_laws(CASES[name])
    p, nb = R.gof(z, law)
    p_alt, _ = R.gof(z, alt)
    _report("A:" + name, p=p, bins=nb, p_alt=p_alt, mean=float(z.mean()), max=int(z.max()))
    assert p > P_FLOOR and nb >= 5, (p, nb)
    assert p_alt < P_ALT, p_alt


def test_dead_genes_and_totals(nb_launch, eng):
    sim, Z = nb_launch
    assert (Z[:, len(CASES):] == 0).all() and (Z[:, :len(CASES)].sum(axis=0) > 0).all()
    np.testing.assert_array_equal(eng.host(sim.totals())[:sim.n], Z.sum(axis=1))
    np.testing.assert_array_equal(sim.dense(), Z)                      # the same seed, the same matrix


# -------------------------------------------------------------------------------------------------
# B. mm_std_normal
# -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def normals(eng):
    x = _std_normal(eng, 99, N_LAW)
    assert (x[N_LAW:] == SENT).all()
    return x[:N_LAW]


def test_std_normal_is_standard_normal(normals):
    r = R.normal_report(normals)
    _report("B:normal", ks_p=r["ks_p"], chi2_p=r["chi2_p"], tail=r["tail"], tail_lo=r["tail_lo"], tail_hi=r["tail_hi"],
            acorr1=r["acorr"][1], acorr64=r["acorr"][64], acorr256=r["acorr"][256], bound=float(r["acorr_bound"]))
    R.check_normal_report(r)


def test_std_normal_seeds_prefix_and_key(eng, normals):
    other = _std_normal(eng, 100, N_LAW)[:N_LAW]
    r = float(R.corr_columns(normals[:, None], other[:, None])[0, 0])
    _report("B:seeds", corr=r, bound=5.5 / np.sqrt(N_LAW))
    assert abs(r) < 5.5 / np.sqrt(N_LAW)
    short = _std_normal(eng, 99, 1000)
    assert (short[1000:] == SENT).all()
    np.testing.assert_array_equal(short[:1000].view(np.int32), normals[:1000].view(np.int32))
    # the documented key scheme, restated in numpy (fp64 libm against the device's: float32 rounding and a little more)
    want = R.std_normal_ref(99, 4096)
    np.testing.assert_allclose(normals[:4096], want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_std_normal_edge_sizes(eng, n):
    x = _std_normal(eng, 5, n, size=300)
    assert (x[n:] == SENT).all() and (x[:n] != SENT).all() and np.isfinite(x[:n]).all()
    np.testing.assert_array_equal(x[:n], _std_normal(eng, 5, 257)[:n])


def test_std_normal_argument_checks(eng):
    import torch

    out = torch.full((16,), float(SENT), dtype=torch.float32, device="cuda")
    for args in [(1, 4, eng.P(None)), (1, -1, eng.P(out)), (1, 256 * 2147483647, eng.P(out))]:
        with pytest.raises(eng._lib.MementoHipError, match="bad argument"):
            eng._lib.call("mm_std_normal", *args, eng._stream())
    assert (eng.host(out) == SENT).all()


# -------------------------------------------------------------------------------------------------
# C. independence; a count is a pure function of (seed, cell, gene)
# -------------------------------------------------------------------------------------------------
def test_independent_branch_is_independent(eng):
    n, G = 1 << 16, 64
    mu, theta = np.full(G, 9.0), np.full(G, 2.9)
    Z = Sim(eng, mu, theta, n, seed_z=77).dense()
    bound = R.corr_bound(n, G * (G - 1) // 2)
    off = np.abs(R.corr_columns(Z)[~np.eye(G, dtype=bool)]).max()
    lag = max(abs(R.lag_corr(Z[:, g], 1)) for g in range(G))
    Z1 = Sim(eng, mu, theta, n, seed_z=78).dense()
    seeds = np.abs(R.corr_columns(Z, Z1)).max()                        # every column of one seed against every column of the next
    bound_seeds = R.corr_bound(n, G * G)
    _report("C:independence", max_offdiag=float(off), max_lag1=float(lag), bound=bound, max_seeds=float(seeds), bound_seeds=bound_seeds)
    assert off < bound and lag < bound and seeds < bound_seeds
    # gene g of a 64-gene launch is gene g of a 32-gene launch; rows 0..254 of a 257-cell launch are the 255-cell launch
    np.testing.assert_array_equal(Sim(eng, mu[:32], theta[:32], n, seed_z=77).dense(), Z[:, :32])
    Z257 = Sim(eng, mu, theta, 257, seed_z=77).dense()
    np.testing.assert_array_equal(Z257, Z[:257])
    np.testing.assert_array_equal(Sim(eng, mu, theta, 255, seed_z=77).dense(), Z257[:255])


# -------------------------------------------------------------------------------------------------
# D. stream separation
# -------------------------------------------------------------------------------------------------
def _poisson_law(q, scale=1.0):
    return lambda z: R.poisson_pmf(q * scale * float(z))


def test_capture_stream_is_not_an_nb_stream(eng):
    """seed_z == seed_capture, genes 24300 and 24301 = 0x5EED alive: the capture stream of a cell once was the NB stream of
    (cell, 24301), so the captured count of that gene depended on its transcriptome count beyond Poisson(q z)."""
    n, G, q, seed = 1 << 18, 24302, 0.5, 4242
    mu, theta = np.zeros(G), np.ones(G)
    mu[[24300, 24301]], theta[[24300, 24301]] = 6.0, 2.0
    sim = Sim(eng, mu, theta, n, seed_z=seed)
    zc, xc = sim.csr(), sim.csr(process=1, qs=q, seed_c=seed)
    for g in (24300, 24301):
        z, x = _column(zc, n, g), _column(xc, n, g)
        p_z, _ = R.gof(z, R.nb_pmf(6.0, 2.0))
        p, df, used = R.conditional_gof(x, z, _poisson_law(q))
        p_alt = R.conditional_gof(x, z, _poisson_law(q, R.ALT_CAPTURE_MEAN))[0]
        _report(f"D:capture gene {g}", p=p, df=df, keys=used, p_alt=p_alt, p_z=p_z)
        assert p_z > P_FLOOR
        assert p > P_FLOOR and used >= 15, (g, p, df, used)
        assert p_alt < P_ALT, (g, p_alt)


def test_normal_stream_is_not_an_nb_stream(eng):
    """The same seed: mm_std_normal's element i once was the first Box-Muller proposal of the NB draw of (cell i, gene 27221 =
    0x6A55), the gamma deviate that sets the count."""
    n, G, seed = 1 << 16, 27222, 31337
    mu, theta = np.zeros(G), np.ones(G)
    mu[27221], theta[27221] = 50.0, 5.0
    z = _column(Sim(eng, mu, theta, n, seed_z=seed).csr(), n, 27221)
    x = _std_normal(eng, seed, n)[:n]
    rho = float(scipy.stats.spearmanr(x, z)[0])
    # the proposal that stream would share, restated: the test can see what it excludes
    shared = float(scipy.stats.spearmanr(R.first_nb_normal_ref(seed, np.arange(n), 27221), z)[0])
    _report("D:normal", spearman=rho, bound=5.5 / np.sqrt(n), spearman_of_the_nb_streams_own_proposal=shared)
    assert shared > 0.5                                                # not vacuous: the NB stream's proposal does drive z
    assert abs(rho) < 5.5 / np.sqrt(n), rho
    assert abs(z.mean() - 50.0) < 5 * np.sqrt((50 + 500) / n)


# -------------------------------------------------------------------------------------------------
# E. capture laws, conditional on Z
# -------------------------------------------------------------------------------------------------
POISSON_THETA = 1e12


def _hyper_rows(q, T):
    return np.minimum(np.rint(q * T), T).astype(np.int64)


@pytest.fixture(scope="module")
def three_genes(eng):
    sim = Sim(eng, [2.0, 3.0, 1.0], [POISSON_THETA] * 3, N_LAW, seed_z=555)
    return sim, sim.dense()


def test_hypergeometric_capture_vector_law(three_genes):
    sim, Z = three_genes
    q = 0.4
    X = sim.dense(process=0, qs=q, seed_c=9)
    T = Z.sum(axis=1)
    assert (X >= 0).all() and (X <= Z).all()
    np.testing.assert_array_equal(X.sum(axis=1), _hyper_rows(q, T))

    def law(scale):
        return lambda z: R.mvhg_pmf(z, int(_hyper_rows(q, z.sum())), scale)

    code = X[:, 0] * (Z[:, 1] + 1) + X[:, 1]
    p, df, used = R.conditional_gof(code, Z, law(1))
    p_alt = R.conditional_gof(code, Z, law(R.ALT_URN_SCALE))[0]
    _report("E:hyper", p=p, df=df, keys=used, p_alt=p_alt)
    assert p > P_FLOOR and used >= 20 and df >= 50, (p, df, used)
    assert p_alt < P_ALT


def test_hypergeometric_row_sums_ties_and_extremes(three_genes):
    sim, Z = three_genes
    T = Z.sum(axis=1)
    X = sim.dense(process=0, qs=0.5, seed_c=10)
    want = _hyper_rows(0.5, T)
    assert want[T == 3][0] == 2 and want[T == 5][0] == 2 and want[T == 7][0] == 4 and (T == 3).sum() > 1000 and (T == 5).sum() > 1000
    np.testing.assert_array_equal(X.sum(axis=1), want)                 # ties half to even
    assert (X <= Z).all()
    assert sim.dense(process=0, qs=0.0, seed_c=10).sum() == 0
    np.testing.assert_array_equal(sim.dense(process=0, qs=1.0, seed_c=10), Z)
    ptr, idx, val = sim.csr(process=0, qs=0.0, seed_c=10)
    assert ptr[-1] == 0 and len(idx) == 0


@pytest.mark.parametrize("mean,q", [(6.0, 0.3), (60.0, 0.25)], ids=["multiplication", "ptrs"])
def test_poisson_capture_law(eng, mean, q):
    """x | z ~ Poisson(q z): q z < 10 throughout (the multiplication method), and q z in about 10..20 (the capture's own PTRS)."""
    sim = Sim(eng, [mean], [POISSON_THETA], N_LAW, seed_z=556)
    z, x = sim.dense()[:, 0], sim.dense(process=1, qs=q, seed_c=11)[:, 0]
    p, df, used = R.conditional_gof(x, z, _poisson_law(q))
    p_alt = R.conditional_gof(x, z, _poisson_law(q, R.ALT_CAPTURE_MEAN))[0]
    keys = np.unique(z, return_counts=True)
    top = keys[0][np.argsort(-keys[1], kind="stable")[:30]]
    _report(f"E:poisson mean {mean}", p=p, df=df, keys=used, p_alt=p_alt, lam_lo=float(q * top.min()), lam_hi=float(q * top.max()))
    assert (q * top.max() < 10) if mean < 10 else (q * top.min() >= 10)
    assert p > P_FLOOR and used >= 15 and df >= 100, (p, df, used)
    assert p_alt < P_ALT


def test_per_cell_capture_rates(eng):
    sim = Sim(eng, [6.0, 4.0], [POISSON_THETA] * 2, N_LAW, seed_z=557)
    Z = sim.dense()
    qs = np.where(np.arange(N_LAW) % 2 == 0, 0.2, 0.6)
    X = sim.dense(process=1, qs=qs, seed_c=12)
    for par, q in ((0, 0.2), (1, 0.6)):
        m = np.arange(N_LAW) % 2 == par
        p, df, used = R.conditional_gof(X[m, 0], Z[m, 0], _poisson_law(q))
        p_alt = R.conditional_gof(X[m, 0], Z[m, 0], _poisson_law(q, R.ALT_CAPTURE_MEAN))[0]
        _report(f"E:per-cell q {q}", p=p, df=df, keys=used, p_alt=p_alt)
        assert p > P_FLOOR and used >= 15 and p_alt < P_ALT, (q, p, p_alt)
    H = sim.dense(process=0, qs=qs, seed_c=12)
    np.testing.assert_array_equal(H.sum(axis=1), _hyper_rows(qs, Z.sum(axis=1)))


# -------------------------------------------------------------------------------------------------
# F. structure
# -------------------------------------------------------------------------------------------------
F_MU, F_THETA = [0.3, 4.0, 0.0, 12.0, 1.5], [0.5, 2.0, 1.0, POISSON_THETA, 0.05]


@pytest.mark.parametrize("process", [0, 1, 2])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_passes_agree_at_edge_sizes(eng, n, process):
    """Sim.csr checks on every call: the mode-1 counts are the mode-2 row lengths (every cell of the CSR is written and none
    beyond), indices ascend, data are positive integers, the sentinel tails of all outputs are untouched."""
    sim = Sim(eng, F_MU, F_THETA, n, seed_z=21)
    big = Sim(eng, F_MU, F_THETA, 300, seed_z=21)
    qs = None if process == 2 else np.linspace(0.2, 0.9, 300)
    X = _dense(sim.csr(process=process, qs=None if qs is None else qs[:n], seed_c=22), n, 5)
    np.testing.assert_array_equal(X, big.dense(process=process, qs=qs, seed_c=22)[:n])
    assert X.shape == (n, 5) and (X[:, 2] == 0).all()
    if n >= 255:
        assert (X[:, [0, 1, 3, 4]].sum(axis=0) > 0).all()


def test_argument_checks_raise_without_a_launch(eng):
    import torch

    n = 64
    sim = Sim(eng, F_MU, F_THETA, n, seed_z=21)
    i64 = lambda: _full(eng, n, torch.int64)
    totals, nnz, ptr = i64(), i64(), eng.dev(np.arange(n + 1, dtype=np.int64) * 5)
    idx, val = _full(eng, 5 * n, torch.int32), _full(eng, 5 * n, torch.float32, float(SENT))
    qs = eng.dev(np.full(n, 0.5))
    gauss = eng.dev(np.zeros((5, n), dtype=np.float32))
    size = eng.dev(np.full(n, 10.0))
    P, NULL = eng.P, eng.P(None)

    def args(**kw):
        a = dict(mu=P(sim.d_mu), theta=P(sim.d_theta), G=5, n=n, qs=P(qs), process=0, mode=2, totals=P(totals), nnz=P(nnz), ptr=P(ptr),
                 idx=P(idx), val=P(val), gauss=NULL, size=NULL, raw=NULL)
        a.update(kw)
        return (a["mu"], a["theta"], a["G"], a["n"], a["qs"], 21, 22, a["process"], a["mode"], a["totals"], a["nnz"], a["ptr"], a["idx"],
                a["val"], a["gauss"], a["size"], a["raw"], eng._stream())

    bad = [dict(mu=NULL), dict(theta=NULL), dict(G=0), dict(G=-3), dict(n=-1), dict(process=-1), dict(process=3), dict(mode=-1), dict(mode=4),
           dict(mode=3), dict(mode=3, gauss=P(gauss)), dict(mode=3, raw=P(totals)),                  # mode 3 needs scores and raw totals
           dict(gauss=P(gauss), size=P(size)),                                                      # rescaling needs raw totals
           dict(mode=0, totals=NULL), dict(mode=1, nnz=NULL), dict(ptr=NULL), dict(idx=NULL), dict(val=NULL),
           dict(mode=1, process=0, qs=NULL), dict(mode=2, process=1, qs=NULL),                       # a capture needs rates ...
           dict(mode=1, process=0, totals=NULL), dict(mode=2, process=0, totals=NULL),               # ... the urn needs totals
           dict(n=256 * 2147483647)]                                                                # more blocks than a grid holds
    for kw in bad:
        with pytest.raises(eng._lib.MementoHipError, match="bad argument"):
            eng._lib.call("mm_simulate", *args(**kw))
    import torch

    torch.cuda.synchronize()
    for t in (totals, nnz, idx):
        assert (eng.host(t) == SENT).all()
    assert (eng.host(val) == SENT).all()
    eng._lib.call("mm_simulate", *args(mode=0, process=2, qs=NULL))     # the baseline itself is a good call
    assert (eng.host(totals)[:n] >= 0).all() and _tail_ok(eng, totals, n)


# -------------------------------------------------------------------------------------------------
# G. the copula quantile
# -------------------------------------------------------------------------------------------------
def _quantiles(eng, scores, mu, theta):
    y = np.asarray(scores, dtype=np.float32)
    sim = Sim(eng, [mu], [theta], len(y), seed_z=1, gauss=y[None, :])
    k = sim.dense()[:, 0]
    np.testing.assert_array_equal(eng.host(sim.d_raw)[:len(y)], k)     # the mode-3 pass: raw totals of a one-gene problem
    return k


@pytest.mark.parametrize("mu,theta", R.QCASES)
def test_copula_quantile_is_exact_up_to_ties(eng, mu, theta):
    y = R.quantile_scores(mu, theta)
    want, above, below, margin = R.nb_quantile_exact(R.phi(y), mu, theta)
    got = _quantiles(eng, y, mu, theta)
    ok = R.excused(got, want, above, below, margin)
    diff = got - want
    tight = np.minimum(above, below) <= margin
    _report(f"G:quantile ({mu:g}, {theta:g})", scores=len(y), kmax=int(want.max()), one_off=int((diff != 0).sum()), within_margin=int(tight.sum()),
            max_abs_diff=int(np.abs(diff).max()), max_margin=float(margin.max()), min_step=float((above + below).min()))
    assert ok.all(), (y[~ok][:5], got[~ok][:5], want[~ok][:5], above[~ok][:5], below[~ok][:5], margin[~ok][:5])
    assert tight.mean() < 0.25                                          # the excuse is no blanket: most scores are decided


def _stop_k(mu, theta, thresh):
    """The k at which the routine's tail bound pmf(k) R / (1 - R), R = max(r_k, q), falls below ``thresh`` (extended precision)."""
    L = np.longdouble
    q = L(mu) / (L(mu) + L(theta))
    pmf, k = np.exp(L(theta) * np.log1p(-q)), 0
    while True:
        r = (k + L(theta)) / (k + 1) * q
        rmax = max(r, q)
        if rmax < 1 and pmf * rmax < thresh * (1 - rmax):
            return k
        pmf, k = pmf * r, k + 1


@pytest.mark.parametrize("mu,theta", [(0.05, 0.25), (1.0, 0.1), (9.0, 2.9), (2500.0, 62500.0)])
def test_copula_quantile_of_infinite_and_nan_scores(eng, mu, theta):
    """Documented in include/memento_hip.h: Phi == 1 (+inf, and every score from 8.3) runs until the running sum rounds to 1 or
    the bound on the remaining tail reaches 2^-54: at least to the quantile of 1 - 2^-54 less the routine's rounding distance
    (R.quantile_margin), at most to the k of that bound.
    Phi == 0 (-inf, scores below -38.5) and NaN return the start of the sum, max(0, floor(mean - 9 sd)).  The launch returns:
    the loop is bounded."""
    got = _quantiles(eng, [np.inf, 8.5, 40.0, -np.inf, -39.0, np.nan], mu, theta)
    k0 = int(max(0.0, np.floor(mu - 9.0 * np.sqrt(mu + mu * mu / theta))))
    hi = _stop_k(mu, theta, 2.0 ** -54.5)
    # the running sum rounds to 1 from 1 - 2^-54 on, and lies within the routine's rounding distance of the CDF
    margin = R.nb_quantile_exact(np.array([1.0 - 2.0 ** -50]), mu, theta)[3][0]
    lo = R.nb_quantile_exact(np.array([1.0 - 2.0 ** -54 - margin]), mu, theta)[0][0]
    _report(f"G:inf ({mu:g}, {theta:g})", got_inf=int(got[0]), lo=int(lo), margin=float(margin), stop_hi=hi, k0=k0)
    assert got[0] == got[1] == got[2] and lo <= got[0] <= hi
    assert got[3] == got[4] == got[5] == k0
