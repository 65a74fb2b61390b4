"""``ht_1d_posthoc`` end to end on the small synthetic matrix of tests/test_gpu_ht_joint.py (3,000 cells x 60 genes, 3 levels x
2 replicates = 6 groups, num_boot = 300): every member against the ``ht_1d_vs_control`` call it restates, the many-to-one form,
the adjusted columns and the simultaneous intervals of the last chunk through the numpy restatement (tests/_family_ref.py), gene
chunking under both generators, whole groups as levels, genes with bad groups, planted three-level shifts.

Eight genes carry a planted mean shift 1 : 1.5 : 2.2 over the three levels (binomial thinning of the counts).  Three genes are
given bad groups by hand, through a negative residual variance in ``uns['memento']['1d_moments']`` (the test of
hypothesis_test.py:167-171 then skips these groups): one loses both groups of a level, one loses one group, one loses all."""

import numpy as np
import pytest
import scipy.sparse as sp

import _family_ref as ref

pytestmark = pytest.mark.gpu
B = 300
SEED, FILL = 5, 9
N_PLANTED = 8
CI = 0.95
TEST_COLS = ["de_coef", "de_se", "de_pval", "dv_coef", "dv_se", "dv_pval"]
ADJ_COLS = ["de_pval_adj", "dv_pval_adj", "n_family"]
SCI_COLS = ["de_sci_lo", "de_sci_hi", "dv_sci_lo", "dv_sci_hi"]


def _matrix():
    from scrna_parameter_estimation_amd.synth import synth_adata

    base = synth_adata(3000, 60, 0.45, 3, 2, seed=17, dtype=np.float32)
    X = np.asarray(base.X.todense()).astype(np.int64)
    rng = np.random.default_rng(18)
    planted = np.argsort(-X.sum(axis=0))[:N_PLANTED]                # the most expressed genes
    cond = base.obs["cond"].values
    for level, keep in ((0, 1 / 2.2), (1, 1.5 / 2.2)):
        rows = np.flatnonzero(cond == level)
        X[np.ix_(rows, planted)] = rng.binomial(X[np.ix_(rows, planted)], keep)
    return base, sp.csr_matrix(X.astype(np.float32)), planted


@pytest.fixture(scope="module")
def prepared():
    """(adata, memento, group frame, names of the genes with planted shifts, {role: gene name} of the genes with bad groups)."""
    from scrna_parameter_estimation_amd import memento
    from scrna_parameter_estimation_amd.anndata_lite import AnnDataLite

    base, X, planted = _matrix()
    adata = AnnDataLite(X, base.obs, base.var)
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


def _posthoc(prepared, treatment_col="cond", **kw):
    adata, memento = prepared[0], prepared[1]
    np.random.seed(SEED)
    return memento.ht_1d_posthoc(adata, treatment_col, num_boot=B, fill_seed=FILL, **kw)


def _vs_control(prepared, control, **kw):
    adata, memento = prepared[0], prepared[1]
    np.random.seed(SEED)
    return memento.ht_1d_vs_control(adata, control, num_boot=B, fill_seed=FILL, treatment_col="cond", **kw)


def _levels(prepared):
    """The levels of ``cond`` in the order of their first appearance among the groups, as the strings of the group labels."""
    return list(dict.fromkeys(str(v) for v in prepared[2]["cond"].values))


def _pairs(prepared):
    """[(level_a, level_b)]: a after b; ordered by b, then a."""
    lv = _levels(prepared)
    return [(lv[a], lv[b]) for a, b in ref.pairwise(len(lv))]


def _same(a, b, cols):
    assert len(a) == len(b) and list(a["gene"]) == list(b["gene"])
    for c in cols:
        np.testing.assert_array_equal(a[c].values, b[c].values, err_msg=c)         # NaNs in the same places, the same bits elsewhere


@pytest.fixture(scope="module")
def one_chunk(prepared):
    return _posthoc(prepared, ci=CI)


def test_result_layout(prepared, one_chunk):
    adata = prepared[0]
    df = one_chunk
    n_genes = len(adata.var.index)
    assert list(df.columns) == ["gene", "level_a", "level_b"] + TEST_COLS[:3] + ["de_pval_adj"] + TEST_COLS[3:] + ["dv_pval_adj", "n_family"] + SCI_COLS
    assert len(df) == 3 * n_genes and list(df["gene"]) == list(np.repeat(np.asarray(adata.var.index), 3))
    lv, pairs = _levels(prepared), _pairs(prepared)
    assert sorted(lv) == ["0", "1", "2"] and pairs == [(lv[1], lv[0]), (lv[2], lv[0]), (lv[2], lv[1])]
    assert list(zip(df["level_a"], df["level_b"])) == pairs * n_genes                                      # a after b; by b, then a
    out = adata.uns["memento"]["1d_ht_posthoc"]
    assert out["levels"] == lv and list(zip(out["level_a"], out["level_b"])) == pairs and out["control"] is None and out["treatment_col"] == "cond" and out["ci"] == CI
    np.testing.assert_array_equal(out["mean_asl_adj"], df["de_pval_adj"].values)
    np.testing.assert_array_equal(out["var_sci"][:, 1], df["dv_sci_hi"].values)
    _same(df, _posthoc(prepared), TEST_COLS + ADJ_COLS)              # without ci: the same numbers, no interval columns
    assert "ci" not in adata.uns["memento"]["1d_ht_posthoc"]


@pytest.mark.parametrize("approx", [False, True])
def test_every_member_is_the_vs_control_test(prepared, one_chunk, approx):
    """For every control level b: the rows with level_b = b are the rows ht_1d_vs_control(control=b) has for the later levels,
    bit for bit, NaNs included."""
    df = one_chunk if not approx else _posthoc(prepared, approx=True)
    n_checked = 0
    lv = _levels(prepared)
    for b, later in ((lv[0], lv[1:]), (lv[1], lv[2:])):
        vc = _vs_control(prepared, int(b), approx=approx)
        for a in later:
            mine = df[(df["level_b"] == b) & (df["level_a"] == a)]
            theirs = vc[vc["group"] == a]
            _same(mine, theirs, TEST_COLS)
            n_checked += int(np.isfinite(mine["de_pval"].values).sum())
    assert n_checked > 3 * 0.8 * (len(df) // 3)
    if approx:
        _same(df, one_chunk, ["de_coef", "de_se", "dv_coef", "dv_se", "n_family"])
        assert (df["de_pval"].values != one_chunk["de_pval"].values).sum() > len(df) // 2


def test_many_to_one(prepared, one_chunk):
    """control=0, and likewise 1 and 2: the rows of ht_1d_vs_control(control=...) plus the adjusted columns, the other levels in
    their order of appearance.  The family against the first level is the first two members of the pairwise family, which is
    larger, so no adjusted p-value is above the pairwise family's."""
    adata = prepared[0]
    lv = _levels(prepared)
    for control in (0, 1, 2):
        one = _posthoc(prepared, control=control)
        vc = _vs_control(prepared, control)
        _same(one, vc, TEST_COLS)
        assert list(one["level_a"]) == list(vc["group"]) and list(one["level_a"][:2]) == [v for v in lv if v != str(control)]
        assert (one["level_b"] == str(control)).all() and adata.uns["memento"]["1d_ht_posthoc"]["control"] == str(control)
        if str(control) == lv[0]:
            df = one
    pair = one_chunk[one_chunk["level_b"] == lv[0]]
    for c in ("de_pval_adj", "dv_pval_adj"):
        p, q = df[c].values, pair[c].values
        both = np.isfinite(p) & np.isfinite(q) & (df["n_family"].values == 2) & (pair["n_family"].values == 3)
        assert both.sum() > len(df) // 2 and (p[both] <= q[both]).all() and (p[both] < q[both]).any()


def test_invariants(prepared, one_chunk):
    df = one_chunk
    for c in ("de", "dv"):
        p, q = df[c + "_pval"].values, df[c + "_pval_adj"].values
        assert (np.isnan(q) >= np.isnan(p)).all() and (q[np.isfinite(q)] >= p[np.isfinite(q)]).all()
        assert (q[np.isfinite(q)] >= 1 / (B + 1)).all() and (q[np.isfinite(q)] <= 1).all()
        lo, hi, coef = df[c + "_sci_lo"].values, df[c + "_sci_hi"].values, df[c + "_coef"].values
        live = np.isfinite(q)
        assert (lo[live] < coef[live]).all() and (coef[live] < hi[live]).all() and np.isnan(lo[~live]).all() and np.isnan(hi[~live]).all()
    n_finite = df.groupby("gene", sort=False)["de_pval_adj"].apply(lambda s: int(np.isfinite(s.values).sum()))
    np.testing.assert_array_equal(df["n_family"].values[::3], n_finite.values)
    # A 0.95 simultaneous interval that leaves out 0 has t0 above the 0.95 quantile of M: with n >= 250 valid columns at most 15 of
    # them lie above it, so the count-based adjusted p-value is at most 16 / 251 < 0.065 (the reported one: that or the raw one)
    out_of = (df["de_sci_lo"].values > 0) | (df["de_sci_hi"].values < 0)
    assert (df["de_pval_adj"].values[out_of] <= np.maximum(0.065, df["de_pval"].values[out_of])).all() and out_of.sum() >= N_PLANTED


@pytest.mark.parametrize("rng", ["replay", "fast"])
def test_chunking_changes_no_number(prepared, one_chunk, rng):
    adata = prepared[0]
    st = adata.uns["memento"]["_hip"]
    whole = one_chunk if rng == "replay" else _posthoc(prepared, rng=rng, ci=CI)
    n_genes = len(whole) // 3
    assert st.last_chunk == (0, n_genes)
    parts = _posthoc(prepared, rng=rng, ci=CI, max_rows=6 * 7)      # 7 genes a chunk
    assert st.last_chunk[1] == n_genes and st.last_chunk[1] - st.last_chunk[0] <= 7 and n_genes > 14
    _same(whole, parts, TEST_COLS + ADJ_COLS + SCI_COLS)
    if rng == "fast":
        assert (whole["de_pval_adj"].values != one_chunk["de_pval_adj"].values).sum() > len(whole) // 4    # other draws than the replay


def test_last_chunk_against_the_restatement(prepared):
    """The last chunk's resident planes and design tables through tests/_family_ref.py reproduce the adjusted columns and the
    simultaneous intervals of the returned rows."""
    from scrna_parameter_estimation_amd import engine

    adata = prepared[0]
    st = adata.uns["memento"]["_hip"]
    df = _posthoc(prepared, ci=CI, max_rows=6 * 11)
    g0, g1 = st.last_chunk
    assert 0 < g0 < g1 == len(df) // 3
    bs, last = st.last_bootstrap, st.last_posthoc
    ym, yv = engine.host(bs.ym), engine.host(bs.yv)
    test_gene, test_design, ptr, grp, w = last.tables
    ng, n_exact = 6, 0
    for k in range(g1 - g0):
        t = np.arange(last.family_ptr[k], last.family_ptr[k + 1])
        assert len(t) == 3 and (test_gene[t] == k).all()
        designs = [(grp[ptr[d]:ptr[d + 1]], w[ptr[d]:ptr[d + 1]]) for d in test_design[t]]
        rows = slice(k * ng, (k + 1) * ng)
        own = ref.family(ym[rows, :B + 1], yv[rows, :B + 1], designs)
        np.testing.assert_allclose(last.scale[t], own["scale"], rtol=1e-9)
        fam = ref.family(ym[rows, :B + 1], yv[rows, :B + 1], designs, last.scale[t])
        np.testing.assert_array_equal(last.adj[t, :, 0], fam["t0"])
        np.testing.assert_array_equal(last.fam[k, :, 0], fam["n_valid"])
        np.testing.assert_array_equal(last.fam[k, :, 1], fam["n_included"])
        got = df.iloc[3 * (g0 + k):3 * (g0 + k) + 3]
        assert (got["n_family"].values == fam["n_included"][0]).all()
        crit = ref.crit(fam, CI)
        for plane, c in ((0, "de"), (1, "dv")):
            raw = got[c + "_pval"].values
            half = np.where(np.isnan(fam["t0"][:, plane]), np.nan, crit[plane] * got[c + "_se"].values)
            np.testing.assert_allclose(got[c + "_sci_lo"].values, got[c + "_coef"].values - half, rtol=1e-12, equal_nan=True)
            np.testing.assert_allclose(got[c + "_sci_hi"].values, got[c + "_coef"].values + half, rtol=1e-12, equal_nan=True)
            if ref.near_ties(fam) == 0:
                np.testing.assert_array_equal(last.adj[t, plane, 1], fam["n_adj"][:, plane])
                with np.errstate(invalid="ignore"):
                    want = np.where(np.isnan(fam["t0"][:, plane]), np.nan, np.maximum(ref.p_adj(fam)[:, plane], raw))
                np.testing.assert_array_equal(got[c + "_pval_adj"].values, want)
                n_exact += 1
    assert n_exact >= 2 * (g1 - g0) - 3


def test_whole_groups_as_levels_on_a_one_column_grouping(prepared):
    """Grouped by ``cond`` alone, every group is a level: treatment_col=None gives the numbers of treatment_col='cond', with the
    group labels as level names."""
    from scrna_parameter_estimation_amd import memento
    from scrna_parameter_estimation_amd.anndata_lite import AnnDataLite

    base, X, _ = _matrix()
    adata = AnnDataLite(X, base.obs, base.var)
    memento.setup_memento(adata, q_column="q")
    memento.create_groups(adata, label_columns=["cond"])
    memento.compute_1d_moments(adata, min_perc_group=0.7)
    groups = adata.uns["memento"]["groups"]
    np.random.seed(SEED)
    by_group = memento.ht_1d_posthoc(adata, num_boot=B, fill_seed=FILL, ci=CI)
    np.random.seed(SEED)
    by_level = memento.ht_1d_posthoc(adata, "cond", num_boot=B, fill_seed=FILL, ci=CI)
    _same(by_group, by_level, TEST_COLS + ADJ_COLS + SCI_COLS)
    assert list(by_group["level_a"][:3]) == [groups[1], groups[2], groups[2]] and list(by_group["level_b"][:3]) == [groups[0], groups[0], groups[1]]
    cond = [g.split("^")[1] for g in groups]
    assert list(by_level["level_a"][:3]) == [cond[1], cond[2], cond[2]] and np.isfinite(by_level["de_pval_adj"].values).mean() > 0.8
    np.random.seed(SEED)
    one = memento.ht_1d_posthoc(adata, control=groups[1], num_boot=B, fill_seed=FILL)
    np.random.seed(SEED)
    _same(one, memento.ht_1d_posthoc(adata, "cond", control=cond[1], num_boot=B, fill_seed=FILL), TEST_COLS + ADJ_COLS)
    assert list(one["level_a"][:2]) == [groups[0], groups[2]] and (one["level_b"] == groups[1]).all()


def test_genes_with_lost_groups(prepared, one_chunk):
    roles = prepared[4]
    by_gene = {g: d for g, d in one_chunk.groupby("gene", sort=False)}
    one = by_gene[roles["one"]]                                     # one group lost: its level still has the other replicate
    assert (one["n_family"] == 3).all() and np.isfinite(one[TEST_COLS + ADJ_COLS + SCI_COLS].values.astype(float)).all()
    level = by_gene[roles["level"]]                                 # level 2 lost: the family is the one contrast of levels 0 and 1
    with_2 = ((level["level_a"] == "2") | (level["level_b"] == "2")).values
    assert (level["n_family"] == 1).all() and with_2.sum() == 2
    assert np.isfinite(level[TEST_COLS + ADJ_COLS + SCI_COLS].values[~with_2].astype(float)).all()
    assert np.isnan(level[TEST_COLS + ADJ_COLS[:2] + SCI_COLS].values[with_2].astype(float)).all()
    # a family of one: the adjusted p-value is the count-based one, at or above the reported raw one
    assert level["de_pval_adj"].values[~with_2][0] >= level["de_pval"].values[~with_2][0]
    lost = by_gene[roles["all"]]
    assert (lost["n_family"] == 0).all() and np.isnan(lost[TEST_COLS + ADJ_COLS[:2] + SCI_COLS].values.astype(float)).all()
    others = one_chunk[~one_chunk["gene"].isin(list(roles.values()))]
    assert (others["n_family"] == 3).mean() > 0.8


def test_planted_effects(prepared, one_chunk):
    """The level-0 against level-2 contrast of the eight planted genes: de_pval_adj <= 0.05 for all of them.  The omnibus test of the
    same genes sits at the floor 1 / 301.  Observed: 1 / 301 = 0.00332 on all eight, so do these; of
    the other genes the median is 0.774 and 4.9 % are at or below 0.05."""
    planted, roles = prepared[3], prepared[4]
    ends = one_chunk[["level_a", "level_b"]].apply(lambda r: {r["level_a"], r["level_b"]} == {"0", "2"}, axis=1).values
    far = one_chunk[ends].set_index("gene")
    assert len(far) == len(one_chunk) // 3
    p = far.loc[planted, "de_pval_adj"].values
    rest = far.drop(planted + list(roles.values()))
    print(f"\nplanted, levels 0 and 2: de_pval_adj {np.sort(p)}; others: median {np.nanmedian(rest['de_pval_adj'].values):.3f}, "
          f"share <= 0.05 {np.nanmean(rest['de_pval_adj'].values <= 0.05):.3f}")
    assert (p <= 0.05).all()
    assert np.nanmedian(rest["de_pval_adj"].values) > 0.2


def test_unknown_rng_raises(prepared):
    with pytest.raises(ValueError, match="rng must be"):
        _posthoc(prepared, rng="numpy")
