"""``ht_1d_eqtl(interaction=...)`` on small synthetic donor x context data (6,000 cells, 24 donors x 2 contexts = 48 groups, 12
genes with 1-11 SNPs each, 300 replicates, one planted response eQTL, one SNP with carriers in one context only): against one
``ht_1d_moments`` call per SNP on the full per-test design, its independence of the gene chunking, the rows behind the records of
the resampled call, the interaction columns, and the plain call left bit for bit as it was."""

import numpy as np
import pandas as pd
import pytest

from _replicate_ref import COUNT_COLUMNS, _np_stats

pytestmark = pytest.mark.gpu
B = 300
COLUMNS = ["gene", "snp", "de_coef", "de_se", "de_pval", "dv_coef", "dv_se", "dv_pval"]
ONE_CONTEXT, PLANTED, N_GENES = "rs1", "rs0", 12


def _names(adata):
    from scrna_parameter_estimation_amd.memento.main import _var_names

    return [str(g) for g in _var_names(adata)[:len(adata.uns["memento"]["_hip"].gene_idx)]]


@pytest.fixture(scope="module")
def donors():
    """24 donors x 2 contexts (one group each), prepared: (adata, memento, covariate, context, genotypes, gene -> SNP list, the
    planted gene).  Donor genotypes are the same in both contexts, except ``ONE_CONTEXT``, which has carriers in context 1 only;
    the cells of the carriers of ``PLANTED`` in context 1 have twice the counts of the planted gene."""
    from scrna_parameter_estimation_amd import memento
    from scrna_parameter_estimation_amd.anndata_lite import AnnDataLite
    from scrna_parameter_estimation_amd.synth import synth_adata
    import scipy.sparse as sp

    base = synth_adata(6000, 40, 0.25, 2, 24, seed=11, dtype=np.float32)
    rng = np.random.default_rng(5)
    donor_g = rng.integers(0, 3, size=(24, 30)).astype(float)
    donor_g[:, 0] = np.arange(24) % 3
    X = base.X.toarray()
    planted = int(np.argmax((X > 0).mean(axis=0)))                            # the densest gene: kept for sure
    boosted = (base.obs["cond"].values == 1) & (donor_g[base.obs["rep"].values, 0] > 0)
    X[boosted, planted] *= 1 + donor_g[base.obs["rep"].values, 0][boosted]
    adata = AnnDataLite(sp.csr_matrix(X), base.obs, base.var)
    memento.setup_memento(adata, q_column="q")
    memento.create_groups(adata, label_columns=["cond", "rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.7)
    gdf = memento.get_groups(adata)
    assert len(gdf) == 48
    ctx = pd.Series(gdf["cond"].values.astype(float), index=gdf.index, name="stim")
    geno = pd.DataFrame(donor_g[gdf["rep"].values], columns=[f"rs{j}" for j in range(30)], index=gdf.index)
    geno[ONE_CONTEXT] = np.where(ctx.values == 1, np.maximum(geno[ONE_CONTEXT].values, (gdf["rep"].values % 2 == 0) * 1.0), 0.0)
    cov = pd.DataFrame({"age": rng.normal(size=24)[gdf["rep"].values], "batch": (gdf["rep"].values % 2).astype(float)}, index=gdf.index)
    names = _names(adata)
    planted_name = str(base.var.index[planted])
    assert planted_name in names and len(names) >= N_GENES
    listed = [planted_name] + [g for g in names if g != planted_name][:N_GENES - 1]
    pairs = {g: [f"rs{j}" for j in rng.choice(np.arange(2, 30), size=int(rng.integers(1, 12)), replace=False)] for g in listed}
    pairs[planted_name] = [PLANTED, ONE_CONTEXT] + [f"rs{j}" for j in range(2, 11)]                      # 11 SNPs: a partial second tile
    pairs[listed[1]] = pairs[listed[1]][:3] + [ONE_CONTEXT]
    return adata, memento, cov, ctx, geno, pairs, planted_name


def _eqtl(donors, seed=2, **kw):
    adata, memento, cov, ctx, geno, pairs, _ = donors
    np.random.seed(seed)
    return memento.ht_1d_eqtl(adata, geno, pairs, covariate=cov, num_boot=B, fill_seed=4, **kw)


@pytest.mark.parametrize("rng", ["replay", "fast"])
def test_rows_against_one_ht_1d_moments_call_per_snp(donors, rng):
    """resample_rep=False: for four (gene, SNP) pairs over two genes the row equals ht_1d_moments(covariate=[cov | ctx | g_s],
    treatment=g_s * ctx) under the same np.random seed -- the bootstrap and its keys are the same, only the weight row's rounding
    differs: 1e-8 for coef and se, 1e-5 for p (the README's parity tolerances)."""
    adata, memento, cov, ctx, geno, pairs, planted = donors
    got = _eqtl(donors, interaction=ctx, approx=True, rng=rng)
    assert list(got.columns) == COLUMNS
    assert list(zip(got["gene"], got["snp"])) == [(g, s) for g in _names(adata) if g in pairs for s in pairs[g]]
    other = [g for g in pairs if g != planted][1]
    for gene, snp in ((planted, PLANTED), (planted, pairs[planted][4]), (other, pairs[other][0]), (other, pairs[other][-1])):
        full = cov.assign(stim=ctx.values, g=geno[snp].values)
        np.random.seed(2)
        memento.ht_1d_moments(adata, covariate=full, treatment=pd.DataFrame({"gxc": geno[snp].values * ctx.values}, index=cov.index),
                              num_boot=B, num_cpus=1, verbose=0, resampling="bootstrap", fill_seed=4, approx=True, rng=rng)
        want = memento.get_1d_ht_result(adata)
        want = want[want["gene"] == gene].iloc[0]
        row = got[(got["gene"] == gene) & (got["snp"] == snp)].iloc[0]
        for k, tol in (("de_coef", 1e-8), ("de_se", 1e-8), ("dv_coef", 1e-8), ("dv_se", 1e-8), ("de_pval", 1e-5), ("dv_pval", 1e-5)):
            print(f"rng {rng} {gene} {snp} {k}: {row[k]!r} against {want[k]!r}: difference {abs(row[k] - want[k]):.3g}")
            assert np.isfinite(want[k]) and abs(row[k] - want[k]) <= tol, (gene, snp, k)
    ht = adata.uns["memento"]["1d_ht_eqtl"]
    assert ht["interaction"] is True
    np.testing.assert_array_equal(ht["context"], ctx.values)


@pytest.mark.parametrize("rng", ["replay", "fast"])
def test_resampled_call_chunking_and_rows(donors, rng, monkeypatch):
    """resample_rep=True: two values of max_rows give identical frames; with approx=False the tail fits read their rows through the
    closure (rank-one copies + the per-test kernel: mm_residualize_rank1 is launched), with approx=True nothing reads a row."""
    from scrna_parameter_estimation_amd import engine

    adata, memento, cov, ctx, geno, pairs, planted = donors
    n_genes, ng = len(adata.uns["memento"]["_hip"].gene_idx), 48
    launched, call = [], engine._lib.call
    monkeypatch.setattr(engine._lib, "call", lambda name, *a: (launched.append(name), call(name, *a))[1])
    one = _eqtl(donors, interaction=ctx, resample_rep=True, approx=False, rng=rng, max_rows=n_genes * ng)
    assert "mm_residualize_rank1" in launched and "mm_cross_resampled_block_cov" in launched and "mm_cross_resampled_block" not in launched
    few = _eqtl(donors, interaction=ctx, resample_rep=True, approx=False, rng=rng, max_rows=5 * ng)
    pd.testing.assert_frame_equal(few, one, check_exact=True)
    del launched[:]
    fast = _eqtl(donors, interaction=ctx, resample_rep=True, approx=True, rng=rng, max_rows=n_genes * ng)
    assert "mm_residualize_rank1" not in launched and "mm_cross_resampled_block_cov" in launched
    for k in ("de_coef", "de_se", "dv_coef", "dv_se"):
        np.testing.assert_array_equal(fast[k].values, one[k].values)
    live = np.isfinite(one["de_pval"].values)
    assert live.sum() > len(one) // 2 and (one["de_pval"].values[live] > 0).all()
    assert np.isnan(one.loc[one["snp"] == ONE_CONTEXT, COLUMNS[2:]].values).all()


def test_resampled_records_are_those_of_their_rows(donors):
    """The engine call behind the resampled scan, on the last chunk's replicate rows: the counts of every record are those of the
    coefficient row the closure returns for the test, coef0 and the range bit for bit."""
    from scrna_parameter_estimation_amd.memento import _ht

    adata, memento, cov, ctx, geno, pairs, planted = donors
    _eqtl(donors, interaction=ctx, resample_rep=True, approx=True, rng="fast")
    st = adata.uns["memento"]["_hip"]
    bs, (g0, g1) = st.last_bootstrap, st.last_chunk
    mv = _ht.moments_view(adata.uns["memento"])
    names = _names(adata)[g0:g1]
    gene_cols = _ht.eqtl_gene_columns(geno, pairs, names)
    good = np.ones((g1 - g0, 48), dtype=bool)
    d = _ht.eqtl_interaction_tables(good, gene_cols, cov.values, ctx.values, geno.values, mv.Nc_list)
    keep = np.flatnonzero(d.has_test)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(d.test_row[keep], minlength=g1 - g0))])
    st_m, st_v, rows = bs.cross_resampled_block(ptr, d.tt_mat[keep], good, d.row_mask, d.Mstack, mv.Nc_list, seed=21,
                                                gene_key=np.arange(g0, g1), zt=d.zt_mat[keep])
    idx = np.arange(len(keep))
    assert len(idx) > 20
    for which, stt in ((0, st_m), (1, st_v)):
        got = rows(which, idx)
        for k in idx:
            want = _np_stats(got[k, :B + 1])
            np.testing.assert_array_equal(stt[k, COUNT_COLUMNS], want[COUNT_COLUMNS])
            np.testing.assert_array_equal(stt[k, [0, 7]], want[[0, 7]])


def test_interaction_columns_and_gene_level_adjustment(donors):
    """The planted response eQTL stands out of its gene's null pairs; the one-context SNP has no test, is outside the family, and
    every adjusted p-value is at least the SNP's own."""
    adata, memento, cov, ctx, geno, pairs, planted = donors
    df = _eqtl(donors, interaction=ctx, adjust=True, approx=True, rng="fast")
    assert list(df.columns) == COLUMNS + ["de_pval_adj", "dv_pval_adj", "n_family"]
    mine = df[df["gene"] == planted].set_index("snp")
    t = (mine["de_coef"].abs() / mine["de_se"])
    assert np.isnan(t[ONE_CONTEXT]) and t[PLANTED] > t.drop([PLANTED, ONE_CONTEXT]).max() and mine.loc[PLANTED, "de_coef"] > 0
    assert np.isnan(df.loc[df["snp"] == ONE_CONTEXT, COLUMNS[2:] + ["de_pval_adj", "dv_pval_adj"]].values).all()
    assert (mine["n_family"] == len(pairs[planted]) - 1).all()                # the one-context SNP is no member
    tested = df[df["snp"] != ONE_CONTEXT]
    assert np.isfinite(tested["de_pval_adj"]).all() and (tested["de_pval_adj"] >= tested["de_pval"]).all()
    assert (tested["dv_pval_adj"].dropna() >= tested["dv_pval"][tested["dv_pval_adj"].notna()]).all()
    genes = memento.get_eqtl_gene_result(adata)
    assert len(genes) == len(pairs) and genes.set_index("gene").loc[planted, "de_lead_snp"] == PLANTED
    plain = _eqtl(donors, interaction=ctx, adjust=False, approx=True, rng="fast")
    pd.testing.assert_frame_equal(df[COLUMNS], plain, check_exact=True)


@pytest.mark.parametrize("resample_rep", [False, True])
def test_without_interaction_nothing_changes(donors, resample_rep):
    """interaction=None is the call without the argument, bit for bit, and leaves no trace in ``uns``; the combination that is not
    offered raises."""
    adata, memento, cov, ctx, geno, pairs, planted = donors
    a = _eqtl(donors, resample_rep=resample_rep, approx=True, adjust=True)
    b = _eqtl(donors, resample_rep=resample_rep, approx=True, adjust=True, interaction=None)
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    assert "interaction" not in adata.uns["memento"]["1d_ht_eqtl"]
    with pytest.raises(NotImplementedError):
        _eqtl(donors, interaction=ctx, adjust=True, resample_rep=True)
    for bad in (ctx.values[:-1], np.column_stack([ctx.values, ctx.values]), np.where(np.arange(48) == 3, np.nan, ctx.values)):
        with pytest.raises(ValueError):
            _eqtl(donors, interaction=bad)
