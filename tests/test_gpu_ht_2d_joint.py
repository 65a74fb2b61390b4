"""``ht_2d_joint`` end to end on a small synthetic matrix (6,000 cells x 150 genes, 3 levels x 2 replicates = 6 groups, 60 distinct
pairs among well-expressed genes, num_boot = 300): against the marginal test of ``ht_2d_moments`` for one treatment column, the
label-name forms and the coding of the factor, pair chunking under both generators, the last chunk's resident correlation rows
through the numpy restatement (tests/_joint_ref.py), duplicates, a self pair and pairs with skipped groups, planted three-level
changes and the argument check.

Six pairs carry a planted change: in the cells of level 1 gene b gets a thinned copy (THIN) of gene a added, as
``_guide_adata(coupled=...)`` of tests/test_gpu_vs_control_2d.py does.  Three unplanted pairs are given skipped groups by hand,
through a NaN true correlation in ``uns['memento']['2d_moments']`` after ``compute_2d_moments`` (the test of
hypothesis_test.py:325 then skips these (pair, group)): one loses one group, one both groups of a level, one all groups."""

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _joint_ref as ref
from test_gpu_vs_control_2d import _prepare, _top_pairs

pytestmark = pytest.mark.gpu
B = 300
SEED, FILL = 5, 9
N_PLANTED = 6
THIN = 0.15                                 # (from 0.25 on the estimated correlation of level 1 reaches the clip at 1 and its groups are skipped)
COLS = ["df", "corr_stat", "corr_pval"]
ONE, LEVEL, ALL = 20, 21, 22                # positions (in the base pair list) of the pairs that lose groups
DUP_OF = 10


@pytest.fixture(scope="module")
def prepared():
    """SimpleNamespace: adata, memento, gdf (group frame), pairs, the positions of the special pairs and ``pristine``, the result
    of the default call before any true correlation was overwritten."""
    from types import SimpleNamespace

    from scrna_parameter_estimation_amd.synth import synth_adata

    adata = synth_adata(6000, 150, 0.2, 3, 2, seed=71, dtype=np.float32)
    X = adata.X.toarray()
    rng = np.random.default_rng(74)
    top = np.argsort(-X.mean(axis=0), kind="stable")[3:27]         # (as _guide_adata: the few best expressed genes can fail the variance filter)
    cells = np.flatnonzero(adata.obs["cond"].values == 1)
    for k in range(N_PLANTED):
        a, b = top[2 * k], top[2 * k + 1]
        X[cells, b] = X[cells, b] + rng.binomial(X[cells, a].astype(np.int64), THIN)
    adata.X = sp.csr_matrix(X.astype(np.float32))
    names = np.array(adata.var.index.tolist())[top]
    base = _top_pairs(names, 60, 72, coupled=N_PLANTED)
    pairs_in = base + [(base[DUP_OF][1], base[DUP_OF][0]), (str(names[0]), str(names[0]))]
    memento, pairs = _prepare(adata, ["cond", "rep"], pairs_in)
    assert pairs == pairs_in
    p = SimpleNamespace(adata=adata, memento=memento, gdf=memento.get_groups(adata), pairs=pairs, n_base=len(base), dup=len(base), self_pair=len(base) + 1)
    m = adata.uns["memento"]
    p.Nc = np.array([m["group_cells"][g].shape[0] for g in m["groups"]], dtype=np.float64)
    cond, rep = p.gdf["cond"].values.astype(int), p.gdf["rep"].values.astype(int)
    p.trt = np.stack([cond == 1, cond == 2], axis=1).astype(np.float64)
    p.cov = (rep == 1).astype(np.float64)[:, None]
    p.corr0 = np.stack([m["2d_moments"][g]["corr"].copy() for g in m["groups"]], axis=1)      # [pair][group], as computed
    p.pristine = _joint(p)
    for i, g in enumerate(m["groups"]):
        if i == 3:
            m["2d_moments"][g]["corr"][ONE] = np.nan
        if cond[i] == 2:
            m["2d_moments"][g]["corr"][LEVEL] = np.nan
        m["2d_moments"][g]["corr"][ALL] = np.nan
    return p


def _joint(p, treatment="cond", covariate=("rep",), **kw):
    np.random.seed(SEED)
    covariate = list(covariate) if isinstance(covariate, tuple) else covariate
    return p.memento.ht_2d_joint(p.adata, treatment, covariate=covariate, num_boot=B, fill_seed=FILL, **kw)


def _same(a, b, cols=COLS):
    assert list(a["gene_1"]) == list(b["gene_1"]) and list(a["gene_2"]) == list(b["gene_2"])
    for c in cols:
        np.testing.assert_array_equal(a[c].values, b[c].values, err_msg=c)         # NaNs in the same places, the same bits elsewhere


@pytest.fixture(scope="module")
def one_chunk(prepared):
    return _joint(prepared)


def _last_chunk(p):
    """(host rows [pair x group][ld], good [pair][group], position in the requested list of every pair of the last chunk), in
    device pair order."""
    from scrna_parameter_estimation_amd import engine
    from scrna_parameter_estimation_amd.memento import _ht

    m = p.adata.uns["memento"]
    st = m["_hip"]
    bs = st.last_bootstrap2d
    lo, hi = st.last_chunk2d
    first, _ = _ht.distinct_pairs(m["2d_moments"]["gene_idx_1"], m["2d_moments"]["gene_idx_2"])
    ng = len(p.gdf)
    assert bs.n_pairs == hi - lo
    return engine.host(bs.yc).copy()[:bs.n_pairs * ng], bs.active.reshape(bs.n_pairs, ng).copy(), first[lo + np.asarray(bs.order)]


def test_single_column_against_the_marginal_test(prepared):
    """One treatment column, the same seed as ht_2d_moments: the same replicate rows, the same stream state afterwards,
    Q_0 = ss * corr_coef^2, df = 1 and the marginal p-value wherever its extreme count exceeds 10."""
    from scrna_parameter_estimation_amd.memento import design

    p = prepared
    m = p.adata.uns["memento"]
    gdf, ng = p.gdf, len(p.gdf)
    dose = pd.DataFrame({"dose": gdf["cond"].values.astype(np.float64)}, index=gdf.index)
    cov = pd.DataFrame({"intercept": np.ones(ng), "rep": (gdf["rep"].values.astype(int) == 1).astype(np.float64)}, index=gdf.index)
    np.random.seed(SEED)
    p.memento.ht_2d_moments(p.adata, covariate=cov, treatment=dose, num_boot=B, num_cpus=1, verbose=0, resampling="bootstrap",
                            resample_rep=False, approx=False, fill_seed=FILL)
    after_marginal = np.random.random()
    marg = {k: np.asarray(m["2d_ht"][k]).copy() for k in ("corr_coef", "corr_asl")}
    y1, good1, pos1 = _last_chunk(p)
    df = _joint(p, treatment=dose, covariate=cov)
    assert np.random.random() == after_marginal                    # the global stream was consumed identically
    y, good, pos = _last_chunk(p)
    np.testing.assert_array_equal(y1, y)                           # the same replicate rows
    np.testing.assert_array_equal(good1, good)
    np.testing.assert_array_equal(pos1, pos)
    assert len(pos) == p.n_base                                    # one chunk: every distinct pair
    n_eq = n_tie = 0
    for k, c in enumerate(pos):
        if not good[k].any():
            assert c == ALL and df["df"].values[c] == 0 and np.isnan(df["corr_stat"].values[c]) and np.isnan(marg["corr_coef"][c])
            continue
        assert df["df"].values[c] == 1
        W, ss = design.weight_rows(cov.values, dose.values, p.Nc, good[k], return_ss=True)
        coef0 = marg["corr_coef"][c]
        np.testing.assert_allclose(df["corr_stat"].values[c], ss[0] * coef0 ** 2, rtol=1e-9, err_msg=f"pair {c}")
        rows = np.arange(k * ng, (k + 1) * ng)[good[k]]
        ok = np.isfinite(y[rows, :B + 1]).all(axis=0)
        coef = W[0, good[k]] @ np.where(ok, y[rows, :B + 1], 0.0)
        nul = np.abs(coef[1:] - coef[0])[ok[1:]]
        count = int((nul > abs(coef[0])).sum())
        if count <= 10:
            continue
        tie = bool((np.abs(nul - abs(coef[0])) <= 1e-12 * abs(coef[0])).any())
        p_m, p_j = marg["corr_asl"][c], df["corr_pval"].values[c]
        if tie:
            n_tie += 1
            assert abs(p_m - p_j) * (1 + len(nul)) <= 1 + 1e-9
        else:
            assert p_m == p_j == (1 + count) / (1 + len(nul)), f"pair {c}"
            n_eq += 1
    print(f"\nsingle column: {n_eq} p-values equal to the marginal test's, {n_tie} near ties")
    assert n_tie <= 1 and n_eq >= p.n_base // 2                    # most unplanted pairs have counts far above 10


def test_label_forms_and_codings(prepared, one_chunk):
    p = prepared
    cond = p.gdf["cond"].values.astype(int)
    _same(one_chunk, _joint(p, treatment=p.trt, covariate=p.cov))  # the label name and the explicit drop-first dummies: the same bits
    out = p.adata.uns["memento"]["2d_ht_joint"]
    assert out["treatment"] == ["treatment_0", "treatment_1"] and out["covariate"] == ["covariate_0"]
    other = _joint(p, treatment=pd.DataFrame({"c0": cond == 0, "c2": cond == 2}, index=p.gdf.index).astype(float), covariate=p.cov)
    alld = _joint(p, treatment=np.stack([cond == v for v in (0, 1, 2)], axis=1).astype(np.float64), covariate=p.cov)
    for coded in (other, alld):                                     # another level dropped, all three dummies: the same test
        _same(one_chunk, coded, ["df"])
        np.testing.assert_allclose(coded["corr_stat"].values, one_chunk["corr_stat"].values, rtol=1e-9, equal_nan=True)


@pytest.mark.parametrize("rng", ["replay", "fast"])
def test_chunking_changes_no_number(prepared, one_chunk, rng):
    p = prepared
    st = p.adata.uns["memento"]["_hip"]
    ng = len(p.gdf)
    whole = one_chunk if rng == "replay" else _joint(p, rng=rng)
    if rng == "fast":
        assert st.last_chunk2d == (0, p.n_base)
    parts = _joint(p, rng=rng, max_rows=ng * 17)                    # 17 pairs a chunk: 4 chunks
    assert st.last_chunk2d == (51, p.n_base)
    _same(whole, parts)
    if rng == "fast":
        live = one_chunk["df"].values > 0
        assert (whole["corr_pval"].values != one_chunk["corr_pval"].values)[live].sum() > live.sum() // 4    # other draws than the replay
        np.testing.assert_array_equal(whole["corr_stat"].values, one_chunk["corr_stat"].values)             # the observed column is the replay's
        np.random.seed(SEED)
        reseeded = p.memento.ht_2d_joint(p.adata, "cond", covariate=["rep"], num_boot=B, fill_seed=FILL + 1, rng=rng)
        assert (reseeded["corr_pval"].values != whole["corr_pval"].values)[live].sum() > live.sum() // 4


@pytest.mark.parametrize("approx", [False, True])
def test_last_chunk_against_the_restatement(prepared, approx):
    """The last chunk's resident correlation rows through tests/_joint_ref.py, design and all, reproduce the returned rows."""
    p = prepared
    ng = len(p.gdf)
    df = _joint(p, max_rows=ng * 17, approx=approx)
    n_valid = p.adata.uns["memento"]["2d_ht_joint"]["n_valid"]
    y, good, pos = _last_chunk(p)
    assert len(pos) == p.n_base - 51
    n_p = n_tie = 0
    for k, c in enumerate(pos):
        L, idx = ref.joint_design(p.cov, p.trt, p.Nc, good[k])
        rows = k * ng + idx
        rec = ref.joint_records(L, y[rows, :B + 1], y[rows, :B + 1])[0]
        q0, qs, ok = ref.q_columns(L, y[rows, :B + 1], y[rows, :B + 1])
        assert df["df"].values[c] == L.shape[0] and n_valid[c] == rec[2]
        np.testing.assert_allclose(df["corr_stat"].values[c], rec[0], rtol=1e-9, equal_nan=True)
        if not L.shape[0]:
            assert np.isnan(df["corr_pval"].values[c])
            continue
        want, got = ref.pvalues(rec, approx)[0], df["corr_pval"].values[c]
        if approx:
            np.testing.assert_allclose(got, want, rtol=1e-6)
        elif ref.near_ties(q0[0], qs[0], ok, rel=1e-12):
            n_tie += 1
            assert abs(got - want) * (1 + rec[2]) <= 1 + 1e-9
        else:
            assert got == want, f"pair {c}"
        n_p += 1
    assert n_p >= len(pos) - 1 and n_tie <= 1


def test_pair_handling_and_result_layout(prepared, one_chunk):
    p = prepared
    out = p.adata.uns["memento"]["2d_ht_joint"]
    _same(one_chunk, _joint(p))                                     # the call again: the same numbers, and its arrays in uns
    out = p.adata.uns["memento"]["2d_ht_joint"]
    assert list(one_chunk.columns) == ["gene_1", "gene_2"] + COLS and len(one_chunk) == len(p.pairs)
    assert list(zip(one_chunk["gene_1"], one_chunk["gene_2"])) == p.pairs
    assert set(out) == {"corr_stat", "corr_asl", "df", "n_valid", "treatment", "covariate"}
    assert out["treatment"] == ["cond=1", "cond=2"] and out["covariate"] == ["rep=1"]
    for k in ("corr_stat", "corr_asl", "df", "n_valid"):
        assert out[k].shape == (len(p.pairs),)
    np.testing.assert_array_equal(out["corr_asl"], one_chunk["corr_pval"].values)
    np.testing.assert_array_equal(out["df"], one_chunk["df"].values)
    row = one_chunk[COLS].values
    np.testing.assert_array_equal(row[p.dup], row[DUP_OF])          # the reversed duplicate: the first one's result
    assert np.isfinite(row[DUP_OF]).all()
    for dead in (p.self_pair, ALL):                                 # the self pair, the pair with no good group
        assert row[dead, 0] == 0 and np.isnan(row[dead, 1:]).all() and out["n_valid"][dead] == 0
    assert row[ONE, 0] == 2 and np.isfinite(row[ONE]).all()         # one group lost: its level still has the other replicate
    assert p.pristine["df"].values[ONE] == 2 and row[ONE, 1] != p.pristine["corr_stat"].values[ONE]
    assert row[LEVEL, 0] == 1 and np.isfinite(row[LEVEL]).all()     # a whole level lost: two levels left
    assert p.pristine["df"].values[LEVEL] == 2 and p.pristine["df"].values[ALL] == 2
    live = one_chunk["df"].values > 0
    assert (out["n_valid"][live] == B).all()
    pv = one_chunk["corr_pval"].values[live]
    assert (pv >= 1 / (B + 1)).all() and (pv <= 1).all()            # the floor of the count


def test_planted_changes(prepared, one_chunk):
    p = prepared
    cond = p.gdf["cond"].values.astype(int)
    level_corr = np.stack([p.corr0[:, cond == v].mean(axis=1) for v in (0, 1, 2)], axis=1)         # [pair][level]
    planted = np.arange(N_PLANTED)
    gap = np.minimum(level_corr[planted, 1] - level_corr[planted, 0], level_corr[planted, 1] - level_corr[planted, 2])
    print(f"\nplanted pairs: correlation of level 1 above the other levels by {np.round(gap, 3)}")
    assert (gap >= 0.2).all()                                       # the input: raise THIN if this fails
    pv = one_chunk["corr_pval"].values
    with np.errstate(invalid="ignore"):
        usable = (~np.isnan(p.corr0) & (np.abs(p.corr0) != 1)).all(axis=1)
    assert usable[planted].all() and (one_chunk["df"].values[planted] == 2).all()      # the input: no planted group at the clip
    rest = np.setdiff1d(np.flatnonzero(usable[:p.n_base]), np.r_[planted, ONE, LEVEL, ALL])
    assert (one_chunk["df"].values[rest] == 2).all() and len(rest) >= 45
    print(f"planted: corr_pval {np.round(pv[planted], 4)}; {len(rest)} others: median {np.median(pv[rest]):.3f}")
    assert (pv[planted] <= 0.05).sum() >= 5
    assert 0.2 <= np.median(pv[rest]) <= 0.8


def test_unknown_rng_raises(prepared):
    with pytest.raises(ValueError, match="rng must be"):
        _joint(prepared, rng="other")
