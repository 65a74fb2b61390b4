"""GPU tests of the sequential bootstrap: ht_1d_vs_control(rng='fast', max_boot=..., min_extreme=...).

A control and 5 guide groups of 1,500 to 3,000 cells, 40 well-expressed genes, a two-fold mean shift planted in guides 1 and 2
for 5 genes; num_boot = 200, max_boot = 3200, fixed fill_seed.  The genes are expressed (4 to 10 counts per cell) and overdispersed
(squared CV of the rate about 0.6) strongly enough that the variance estimate of a 750-cell group (guide x 2 replicates) is some
eight standard errors above zero: at 1.5 to 4 counts and a squared CV of 0.3 a few of its 1.5 M replicates came out invalid.
Premise of every exactness statement below, asserted: no replicate of the one-shot 3200-replicate call is invalid, so nothing
is refilled and the rounds' replicates ARE the one-shot call's.
"""

from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

N_GENES = 40
SIZES = (3000, 1500, 1800, 2100, 2500, 3000)        # control, guides 1..5
PLANTED_GUIDES, PLANTED_GENES = (1, 2), (3, 11, 19, 27, 35)
NUM_BOOT, MAX_BOOT, FILL_SEED = 200, 3200, 17
SCHEDULE = (200, 400, 800, 1600, 3200)
COLS = ["de_coef", "de_se", "de_pval", "dv_coef", "dv_se", "dv_pval"]


def _adata(n_rep=1, seed=5):
    from scrna_parameter_estimation_amd.anndata_lite import AnnDataLite

    rng = np.random.default_rng(seed)
    guide = np.repeat(np.arange(len(SIZES)), SIZES)
    n = len(guide)
    mu = rng.uniform(4.0, 10.0, size=N_GENES)
    lam = mu[None, :] * rng.lognormal(0.0, 0.25, size=n)[:, None] * rng.gamma(2.0, 0.5, size=(n, N_GENES))
    for g in PLANTED_GUIDES:
        lam[np.ix_(guide == g, PLANTED_GENES)] *= 2.0
    X = sp.csr_matrix(rng.poisson(lam).astype(np.float32))
    obs = pd.DataFrame({"guide": guide, "rep": np.arange(n) % n_rep, "q": np.full(n, 0.07)}, index=[f"c{i}" for i in range(n)])
    return AnnDataLite(X, obs, pd.DataFrame(index=[f"g{i}" for i in range(N_GENES)]))


def _prepared(n_rep=1):
    from scrna_parameter_estimation_amd import memento

    adata = _adata(n_rep)
    memento.setup_memento(adata, q_column="q", filter_mean_thresh=0.07)
    memento.create_groups(adata, label_columns=["guide"] if n_rep == 1 else ["guide", "rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.7)
    assert len(adata.uns["memento"]["_hip"].gene_idx) == N_GENES
    return memento, adata


def _call(memento, adata, **kw):
    """One ht_1d_vs_control(rng='fast') call from a fixed state of the global numpy stream (the chains' hash uniforms) -> ``df``,
    ``rec`` = the records (st_m, st_v) and ``n_inv`` = the refill counts of the last gene chunk (the only one unless ``max_rows``
    is given), ``uns``, and ``n_open`` of a sequential call: the tests open after every round."""
    np.random.seed(23)
    kw.setdefault("num_boot", NUM_BOOT)
    strata = "rep" in adata.obs.columns and adata.obs["rep"].max() > 0
    control = "0" if strata else adata.uns["memento"]["groups"].index("sg^0")
    df = memento.ht_1d_vs_control(adata, control, rng="fast", fill_seed=FILL_SEED, num_cpus=1,
                                  treatment_col="guide" if strata else None, **kw)
    st = adata.uns["memento"]["_hip"]
    assert "max_rows" in kw or st.last_chunk == (0, N_GENES)
    return SimpleNamespace(df=df.copy(), rec=[r.copy() for r in st.last_records], n_inv=st.last_n_inv.copy(),
                           uns=dict(adata.uns["memento"]["1d_ht_vs_control"]),
                           n_open=list(st.last_sequential.n_open) if "max_boot" in kw else None)


@pytest.fixture(scope="module")
def prep():
    return _prepared()


@pytest.fixture(scope="module")
def one_shot(prep):
    """The one-shot 3200-replicate call (tail fits included), computed once."""
    return _call(*prep, num_boot=MAX_BOOT)


@pytest.fixture(scope="module")
def plain(prep):
    """The plain 200-replicate call."""
    return _call(*prep)


@pytest.fixture(scope="module")
def seq(prep):
    """The sequential call with the default min_extreme."""
    return _call(*prep, max_boot=MAX_BOOT)


def _same_bits(a, b, what=""):
    np.testing.assert_array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64), err_msg=what)


def _exactness(one_shot, got):
    """``got``: a sequential call in which nothing closes early, against the one-shot call with max_boot replicates."""
    df1, rec1, df, rec, uns = one_shot.df, one_shot.rec, got.df, got.rec, got.uns
    assert (one_shot.n_inv == 0).all(), "premise: the one-shot call refills nothing"
    assert len(df) == len(df1) == N_GENES * 5 and list(df.columns) == ["gene", "group"] + COLS + ["de_nboot", "dv_nboot"]
    for tag, r1, r in (("de", rec1[0], rec[0]), ("dv", rec1[1], rec[1])):
        live = np.isfinite(r1[:, 0])
        assert live.all()                                           # well-expressed genes: every test has a coefficient
        for k in (2, 3, 6):                                          # n_valid, n_extreme, n_raw_extreme
            np.testing.assert_array_equal(r[:, k], r1[:, k])
        assert (df[tag + "_nboot"].values == MAX_BOOT).all() and (r[:, 2] == MAX_BOOT).all()
        _same_bits(df[tag + "_coef"], df1[tag + "_coef"], tag)
        np.testing.assert_allclose(df[tag + "_se"].values, df1[tag + "_se"].values, rtol=1e-12, atol=0)
        emp = r1[:, 3] > 10                                          # where the one-shot call took the empirical branch
        assert emp.sum() > 100 and (tag == "dv" or (~emp).sum() >= 10)
        _same_bits(df[tag + "_pval"].values[emp], df1[tag + "_pval"].values[emp], tag)
        np.testing.assert_array_equal(df[tag + "_pval"].values, (r1[:, 3] + 1) / (MAX_BOOT + 1))
    assert uns["max_boot"] == MAX_BOOT and (uns["mean_nboot"] == MAX_BOOT).all() and (uns["var_nboot"] == MAX_BOOT).all()


def test_nothing_closes_early_is_the_one_shot_call(prep, one_shot):
    got = _call(*prep, max_boot=MAX_BOOT, min_extreme=MAX_BOOT + 1)
    _exactness(one_shot, got)
    assert got.uns["min_extreme"] == MAX_BOOT + 1
    assert list(prep[1].uns["memento"]["_hip"].last_sequential.schedule) == list(SCHEDULE) and got.n_open == [N_GENES * 5] * len(SCHEDULE)


def test_nothing_closes_early_with_a_treatment_col():
    """Guide x 2 replicates at the same sizes: the design-table tests, whose chains are several groups per arm."""
    prep2 = _prepared(n_rep=2)
    assert len(prep2[1].uns["memento"]["groups"]) == 12
    one = _call(*prep2, num_boot=MAX_BOOT)
    _exactness(one, _call(*prep2, max_boot=MAX_BOOT, min_extreme=MAX_BOOT + 1))


def test_round_0_is_the_plain_call(plain, seq):
    df0, rec0, uns0, df = plain.df, plain.rec, plain.uns, seq.df
    assert "de_nboot" not in df0.columns and "max_boot" not in uns0 and "mean_nboot" not in uns0
    _same_bits(df["de_coef"], df0["de_coef"])
    _same_bits(df["dv_coef"], df0["dv_coef"])
    n_same = 0
    for tag, r0 in (("de", rec0[0]), ("dv", rec0[1])):
        same = (df[tag + "_nboot"].values == NUM_BOOT) & (r0[:, 3] > 10)
        n_same += int(same.sum())
        for k in ("_coef", "_se", "_pval"):
            _same_bits(df[tag + k].values[same], df0[tag + k].values[same], tag + k)
    assert n_same > 100


def test_stopping_invariants(prep, seq, one_shot):
    df, rec, uns = seq.df, seq.rec, seq.uns
    assert uns["max_boot"] == MAX_BOOT and uns["min_extreme"] == 10
    closed_round0 = ran_out = 0
    for tag, r, key in (("de", rec[0], "mean_nboot"), ("dv", rec[1], "var_nboot")):
        nboot, c, p = df[tag + "_nboot"].values, r[:, 3], df[tag + "_pval"].values
        np.testing.assert_array_equal(uns[key], nboot)
        np.testing.assert_array_equal(nboot, r[:, 2])
        live = np.isfinite(p)
        assert live.sum() > 150 and np.isin(nboot[live], SCHEDULE).all()
        assert ((c > 10) | (nboot == MAX_BOOT))[live].all()
        np.testing.assert_array_equal(p[live], ((c + 1) / (nboot + 1))[live])
        closed_round0 += int((nboot == NUM_BOOT).sum())
        ran_out += int(((nboot == MAX_BOOT) & (c <= 10)).sum())
    assert closed_round0 >= 1
    # a test stops when BOTH its planes are closed: the two planes of a test have the same replicates
    both = np.isfinite(df["de_pval"].values) & np.isfinite(df["dv_pval"].values)
    np.testing.assert_array_equal(df["de_nboot"].values[both], df["dv_nboot"].values[both])
    planted = np.flatnonzero(df["gene"].isin([f"g{g}" for g in PLANTED_GENES]).values
                             & df["group"].isin([f"sg^{k}" for k in PLANTED_GUIDES]).values)
    assert len(planted) == 10
    c_de = rec[0][planted, 3]
    assert (df["de_nboot"].values[planted] == MAX_BOOT).all() and (c_de <= 10).any()
    np.testing.assert_array_equal(df["de_pval"].values[planted], (c_de + 1) / 3201)
    assert ran_out >= 1
    # the replicates behind a test that ran to max_boot are the one-shot call's (premise: nothing refilled there)
    assert (one_shot.n_inv == 0).all()
    full = (df["de_nboot"].values == MAX_BOOT) & (df["dv_nboot"].values == MAX_BOOT)
    for k in (2, 3, 6):
        np.testing.assert_array_equal(rec[0][full, k], one_shot.rec[0][full, k])
        np.testing.assert_array_equal(rec[1][full, k], one_shot.rec[1][full, k])
    n_open = np.asarray(seq.n_open)
    assert (np.diff(n_open) <= 0).all() and 0 < n_open[-1] < n_open[0] < N_GENES * 5


def test_gene_chunks_change_no_number(prep, seq):
    memento, adata = prep
    ng = len(adata.uns["memento"]["groups"])
    got = _call(memento, adata, max_boot=MAX_BOOT, max_rows=14 * ng)          # 14 genes per chunk: three chunks, the last one short
    assert adata.uns["memento"]["_hip"].last_chunk == (28, N_GENES)
    df, df1 = got.df, seq.df
    assert list(df.columns) == list(df1.columns) and (df["gene"] == df1["gene"]).all() and (df["group"] == df1["group"]).all()
    for k in COLS + ["de_nboot", "dv_nboot"]:
        _same_bits(df[k], df1[k], k)
    assert got.n_open == seq.n_open


@pytest.mark.parametrize("kw", [dict(rng="replay"), dict(approx=True), dict(ci=0.95), dict(max_boot=NUM_BOOT - 1), dict(min_extreme=-1)])
def test_argument_errors(prep, kw):
    memento, adata = prep
    st = adata.uns["memento"]["_hip"]
    st.last_bootstrap = "untouched"
    args = dict(num_boot=NUM_BOOT, rng="fast", max_boot=MAX_BOOT)
    args.update(kw)
    with pytest.raises(ValueError):
        memento.ht_1d_vs_control(adata, 0, **args)
    assert st.last_bootstrap == "untouched"                          # raised before the call's first device work
    st.last_bootstrap = None
