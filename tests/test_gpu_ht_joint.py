"""``ht_1d_joint`` end to end on a small synthetic matrix (3,000 cells x 60 genes, 3 levels x 2 replicates = 6 groups,
num_boot = 300): against the marginal test of ``ht_1d_moments`` for one treatment column, the label-name forms and the coding of
the factor, gene chunking under both generators, the last chunk's resident planes through the numpy restatement
(tests/_joint_ref.py), genes with bad groups, planted three-level shifts and the argument check.

Eight genes carry a planted mean shift 1 : 1.5 : 2.2 over the three levels (binomial thinning of the counts).  Three genes are
given bad groups by hand, through a negative residual variance in ``uns['memento']['1d_moments']`` (the test of
hypothesis_test.py:167-171 then skips these groups): one loses both groups of a level, one loses one group, one loses all."""

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _joint_ref as ref

pytestmark = pytest.mark.gpu
B = 300
SEED, FILL = 5, 9
N_PLANTED = 8
COLS = ["df", "de_stat", "de_pval", "dv_stat", "dv_pval"]


@pytest.fixture(scope="module")
def prepared():
    """(adata, memento, group frame, names of the genes with planted shifts, {role: gene name} of the genes with bad groups)."""
    from scrna_parameter_estimation_amd import memento
    from scrna_parameter_estimation_amd.anndata_lite import AnnDataLite
    from scrna_parameter_estimation_amd.synth import synth_adata

    base = synth_adata(3000, 60, 0.45, 3, 2, seed=17, dtype=np.float32)
    X = np.asarray(base.X.todense()).astype(np.int64)
    rng = np.random.default_rng(18)
    planted = np.argsort(-X.sum(axis=0))[:N_PLANTED]                # the most expressed genes
    cond = base.obs["cond"].values
    for level, keep in ((0, 1 / 2.2), (1, 1.5 / 2.2)):
        rows = np.flatnonzero(cond == level)
        X[np.ix_(rows, planted)] = rng.binomial(X[np.ix_(rows, planted)], keep)
    adata = AnnDataLite(sp.csr_matrix(X.astype(np.float32)), base.obs, base.var)
    memento.setup_memento(adata, q_column="q")
    memento.create_groups(adata, label_columns=["cond", "rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.7)
    m = adata.uns["memento"]
    names = np.asarray(adata.var.index)
    gdf = memento.get_groups(adata)
    planted_names = [f"g{j}" for j in planted if f"g{j}" in set(names)]
    assert len(planted_names) == N_PLANTED and len(names) >= 30
    rv = np.stack([m["1d_moments"][g][2] for g in m["groups"]])
    free = [k for k, n in enumerate(names) if n not in planted_names and np.isfinite(rv[:, k]).all()]      # all groups usable so far
    roles = {"level": free[1], "one": free[4], "all": free[len(free) // 2]}
    for role, k in roles.items():
        for i, g in enumerate(m["groups"]):
            hit = {"level": gdf["cond"].values[i] == 2, "one": i == 3, "all": True}[role]
            if hit:
                m["1d_moments"][g][2][k] = -1.0
    return adata, memento, gdf, planted_names, {role: names[k] for role, k in roles.items()}


def _joint(prepared, treatment="cond", covariate=("rep",), **kw):
    adata, memento = prepared[0], prepared[1]
    np.random.seed(SEED)
    covariate = list(covariate) if isinstance(covariate, tuple) else covariate
    return memento.ht_1d_joint(adata, treatment, covariate=covariate, num_boot=B, fill_seed=FILL, **kw)


def _same(a, b, cols=COLS):
    assert list(a["gene"]) == list(b["gene"])
    for c in cols:
        np.testing.assert_array_equal(a[c].values, b[c].values, err_msg=c)         # NaNs in the same places, the same bits elsewhere


@pytest.fixture(scope="module")
def one_chunk(prepared):
    return _joint(prepared)


def _host_planes(st, eng):
    bs = st.last_bootstrap
    return eng.host(bs.ym).copy(), eng.host(bs.yv).copy(), bs.ld


def test_single_column_against_the_marginal_test(prepared):
    """One treatment column, the same seed and max_rows as ht_1d_moments: the same replicate planes, Q_0 = ss * coef^2 and the
    marginal p-value wherever its extreme count exceeds 10."""
    from scrna_parameter_estimation_amd import engine
    from scrna_parameter_estimation_amd.memento import design

    adata, memento, gdf, _, _ = prepared
    m = adata.uns["memento"]
    st = m["_hip"]
    dose = pd.DataFrame({"dose": gdf["cond"].values.astype(np.float64)}, index=gdf.index)
    rep = pd.DataFrame({"rep": (gdf["rep"].values == 1).astype(np.float64)}, index=gdf.index)
    np.random.seed(SEED)
    memento.ht_1d_moments(adata, covariate=rep, treatment=dose, num_boot=B, num_cpus=1, verbose=0, resampling="bootstrap", fill_seed=FILL)
    marg = dict(m["1d_ht"])
    ym1, yv1, ld = _host_planes(st, engine)
    df = _joint(prepared, treatment=dose, covariate=rep)
    ym2, yv2, _ = _host_planes(st, engine)
    np.testing.assert_array_equal(ym1, ym2)                         # the same replicate planes
    np.testing.assert_array_equal(yv1, yv2)
    good, ng = st.last_good, len(gdf)
    Nc = np.array([m["group_cells"][g].shape[0] for g in m["groups"]], dtype=np.float64)
    n_eq = n_tie = 0
    for k in range(len(df)):
        if not good[k].any():
            assert np.isnan(df["de_stat"].values[k]) and np.isnan(marg["mean_coef"][k])
            continue
        W, ss = design.weight_rows(rep.values, dose.values, Nc, good[k], return_ss=True)
        for plane, y, tag, col in ((0, ym1, "mean", "de"), (1, yv1, "var", "dv")):
            coef0 = marg[tag + "_coef"][k]
            np.testing.assert_allclose(df[col + "_stat"].values[k], ss[0] * coef0 ** 2, rtol=1e-9, err_msg=f"gene {k} {tag}")
            rows = np.arange(k * ng, (k + 1) * ng)[good[k]]
            ok = np.isfinite(ym1[rows, :B + 1]).all(axis=0) & np.isfinite(yv1[rows, :B + 1]).all(axis=0)
            coef = W[0, good[k]] @ np.where(ok, y[rows, :B + 1], 0.0)
            nul = np.abs(coef[1:] - coef[0])[ok[1:]]
            count = int((nul > abs(coef[0])).sum())
            if count <= 10:
                continue
            tie = bool((np.abs(nul - abs(coef[0])) <= 1e-12 * abs(coef[0])).any())
            p_m, p_j = marg[tag + "_asl"][k], df[col + "_pval"].values[k]
            if tie:
                n_tie += 1
                assert abs(p_m - p_j) * (1 + len(nul)) <= 1 + 1e-9
            else:
                assert p_m == p_j == (1 + count) / (1 + len(nul)), f"gene {k} {tag}"
                n_eq += 1
    print(f"\nsingle column: {n_eq} p-values equal to the marginal test's, {n_tie} near ties")
    assert n_tie <= 1 and n_eq >= len(df)
    assert (df["df"].values[good.any(axis=1)] == 1).all()


def test_label_forms_and_codings(prepared, one_chunk):
    adata, memento, gdf, _, _ = prepared
    cond, rep = gdf["cond"].values, gdf["rep"].values
    explicit = np.stack([cond == 1, cond == 2], axis=1).astype(np.float64)
    rep_col = (rep == 1).astype(np.float64)[:, None]
    _same(one_chunk, _joint(prepared, treatment=explicit, covariate=rep_col))
    m = adata.uns["memento"]["1d_ht_joint"]
    assert m["treatment"] == ["treatment_0", "treatment_1"] and m["covariate"] == ["covariate_0"]
    other = _joint(prepared, treatment=pd.DataFrame({"c0": cond == 0, "c2": cond == 2}, index=gdf.index).astype(float), covariate=rep_col)
    _same(one_chunk, other, ["df", "de_pval", "dv_pval"])          # another level dropped: no p-value moves
    for c in ("de_stat", "dv_stat"):
        np.testing.assert_allclose(other[c].values, one_chunk[c].values, rtol=1e-9, equal_nan=True)
    alld = _joint(prepared, treatment=np.stack([cond == v for v in (0, 1, 2)], axis=1).astype(np.float64), covariate=rep_col)
    _same(one_chunk, alld, ["df"])                                  # all three dummies: still rank 2
    np.testing.assert_allclose(alld["de_stat"].values, one_chunk["de_stat"].values, rtol=1e-9, equal_nan=True)


def test_result_layout(prepared, one_chunk):
    adata = prepared[0]
    m = adata.uns["memento"]
    assert list(one_chunk.columns) == ["gene"] + COLS and list(one_chunk["gene"]) == list(adata.var.index)
    _same(one_chunk, _joint(prepared))                              # the call again: the same numbers, and its arrays in uns
    out = m["1d_ht_joint"]
    assert set(out) == {"mean_stat", "mean_asl", "var_stat", "var_asl", "df", "n_valid", "treatment", "covariate"}
    assert out["treatment"] == ["cond=1", "cond=2"] and out["covariate"] == ["rep=1"]
    np.testing.assert_array_equal(out["mean_asl"], one_chunk["de_pval"].values)
    live = one_chunk["df"].values > 0
    assert (out["n_valid"][live] == B).all() and (out["n_valid"][~live] == 0).all()
    p = one_chunk["de_pval"].values[live]
    assert (p >= 1 / (B + 1)).all() and (p <= 1).all()              # the floor of the count
    approx = _joint(prepared, approx=True)
    _same(one_chunk, approx, ["df", "de_stat", "dv_stat"])
    pa = approx["de_pval"].values[live]
    mid = p > 0.1               # counts of 30 and more: their Monte-Carlo sd on the log scale is below 0.18, so 1.0 is 5 of them and more
    assert mid.sum() > 10 and np.abs(np.log(pa[mid] / p[mid])).max() < 1.0 and pa.min() < 1 / (B + 1)


@pytest.mark.parametrize("rng", ["replay", "fast"])
def test_chunking_changes_no_number(prepared, one_chunk, rng):
    adata = prepared[0]
    st = adata.uns["memento"]["_hip"]
    whole = one_chunk if rng == "replay" else _joint(prepared, rng=rng)
    assert st.last_chunk == (0, len(whole))
    parts = _joint(prepared, rng=rng, max_rows=6 * 7)               # 7 genes a chunk
    assert st.last_chunk[1] == len(whole) and st.last_chunk[1] - st.last_chunk[0] <= 7
    _same(whole, parts)
    if rng == "fast":
        assert (whole["de_pval"].values != one_chunk["de_pval"].values).sum() > len(whole) // 4     # other draws than the replay


def test_last_chunk_against_the_restatement(prepared):
    """The last chunk's resident planes through tests/_joint_ref.py, design and all, reproduce the returned rows."""
    from scrna_parameter_estimation_amd import engine

    adata, memento, gdf, _, _ = prepared
    m = adata.uns["memento"]
    st = m["_hip"]
    df = _joint(prepared, max_rows=6 * 11)
    g0, g1 = st.last_chunk
    assert 0 < g0 < g1 == len(df)
    ym, yv, _ = _host_planes(st, engine)
    ng = len(gdf)
    cond, rep = gdf["cond"].values, gdf["rep"].values
    trt = np.stack([cond == 1, cond == 2], axis=1).astype(np.float64)
    cov = (rep == 1).astype(np.float64)[:, None]
    Nc = np.array([m["group_cells"][g].shape[0] for g in m["groups"]], dtype=np.float64)
    n_p = 0
    for k in range(g1 - g0):
        L, idx = ref.joint_design(cov, trt, Nc, st.last_good[k])
        rows = k * ng + idx
        recs = ref.joint_records(L, ym[rows, :B + 1], yv[rows, :B + 1])
        q0, qs, ok = ref.q_columns(L, ym[rows, :B + 1], yv[rows, :B + 1])
        assert df["df"].values[g0 + k] == L.shape[0]
        for plane, col in ((0, "de"), (1, "dv")):
            np.testing.assert_allclose(df[col + "_stat"].values[g0 + k], recs[plane][0], rtol=1e-9, equal_nan=True)
            if L.shape[0] and ref.near_ties(q0[plane], qs[plane], ok, rel=1e-9) == 0:
                assert df[col + "_pval"].values[g0 + k] == ref.pvalues(recs[plane])[0]
                n_p += 1
    assert n_p >= 2 * (g1 - g0) - 3


def test_bad_groups(prepared, one_chunk):
    roles = prepared[4]
    row = one_chunk.set_index("gene")
    assert row.loc[roles["level"], "df"] == 1                       # a whole level lost: two levels left
    assert row.loc[roles["one"], "df"] == 2                         # one group lost: its level still has the other replicate
    assert np.isfinite(row.loc[[roles["level"], roles["one"]], COLS].values).all()
    assert row.loc[roles["all"], "df"] == 0 and np.isnan(row.loc[roles["all"], COLS[1:]].values.astype(float)).all()
    others = row.drop(list(roles.values()))                         # (a gene may have a bad group of its own: a variance <= 0)
    assert (others["df"] <= 2).all() and (others["df"] == 2).mean() > 0.8
    assert np.isfinite(others.loc[others["df"] > 0, COLS].values).all()


def test_planted_effects(prepared, one_chunk):
    planted, roles = prepared[3], prepared[4]
    row = one_chunk.set_index("gene")
    assert (row.loc[planted, "de_pval"] <= 0.01).all()
    rest = row.drop(planted + list(roles.values()))
    print(f"\nplanted: largest de_pval {row.loc[planted, 'de_pval'].max():.4f}; others: median {rest['de_pval'].median():.3f}")
    assert rest["de_pval"].median() > 0.2


def test_unknown_rng_raises(prepared):
    with pytest.raises(ValueError, match="rng must be"):
        _joint(prepared, rng="numpy")
