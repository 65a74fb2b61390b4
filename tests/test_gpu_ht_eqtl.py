"""``ht_1d_eqtl`` on small synthetic donor data (3,000 cells, 24 donor groups, 2 covariates, 40 genes, 1-40 SNPs per gene, 300
replicates) against ``ht_1d_moments(treatment_for_gene=...)`` on the same inputs, its independence of the gene chunking, its row
order and its argument checks."""

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu
B = 300
COLUMNS = ["gene", "snp", "de_coef", "de_se", "de_pval", "dv_coef", "dv_se", "dv_pval"]


def _names(adata):
    """The kept genes, in the order of the tests."""
    from scrna_parameter_estimation_amd.memento.main import _var_names

    return [str(g) for g in _var_names(adata)[:len(adata.uns["memento"]["_hip"].gene_idx)]]


@pytest.fixture(scope="module")
def donors():
    """24 donors (one group each), prepared; (adata, memento, covariate, genotypes, gene -> SNP list)."""
    from scrna_parameter_estimation_amd import memento
    from scrna_parameter_estimation_amd.synth import synth_adata

    adata = synth_adata(3000, 40, 0.25, 1, 24, seed=11, dtype=np.float32)
    memento.setup_memento(adata, q_column="q")
    memento.create_groups(adata, label_columns=["rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.7)
    gdf = memento.get_groups(adata)
    rng = np.random.default_rng(5)
    cov = pd.DataFrame({"age": rng.normal(size=len(gdf)), "batch": rng.integers(0, 2, size=len(gdf)).astype(float)}, index=gdf.index)
    geno = pd.DataFrame(rng.integers(0, 3, size=(len(gdf), 60)).astype(float), columns=[f"rs{j}" for j in range(60)], index=gdf.index)
    geno["rs7"] = 1.0                                                        # one SNP constant over the donors
    names = _names(adata)
    assert len(gdf) == 24 and len(names) >= 20
    pairs = {g: [f"rs{j}" for j in rng.choice(60, size=int(rng.integers(1, 41)), replace=False)] for g in names}
    pairs[names[0]] = ["rs7", "rs3"]
    pairs[names[1]] = ["rs7"]                                                # a gene whose whole treatment is all ones: never resampled
    return adata, memento, cov, geno, pairs


def _both(donors, **kw):
    adata, memento, cov, geno, pairs = donors
    np.random.seed(2)
    memento.ht_1d_moments(adata, covariate=cov, treatment=geno, treatment_for_gene=pairs, num_boot=B, num_cpus=1, verbose=0,
                          resampling="bootstrap", fill_seed=4, **kw)
    want = memento.get_1d_ht_result(adata)
    np.random.seed(2)
    got = memento.ht_1d_eqtl(adata, geno, pairs, covariate=cov, num_boot=B, num_cpus=1, resampling="bootstrap", fill_seed=4, **kw)
    return got, want


@pytest.mark.parametrize("rng", ["replay", "fast"])
@pytest.mark.parametrize("approx", [True, False])
@pytest.mark.parametrize("resample_rep", [False, True])
def test_one_chunk_call_against_ht_1d_moments(donors, resample_rep, approx, rng):
    """Same np.random seed, fill_seed and keywords, one chunk: identical NaN sets, equal coefficients, standard errors to 1e-10 and
    p-values to 1e-8 (identical inputs: at most the order of a reduction differs)."""
    got, want = _both(donors, resample_rep=resample_rep, approx=approx, rng=rng)
    assert list(got.columns) == COLUMNS and len(got) == len(want) > 100
    assert (got["gene"].values == want["gene"].values).all() and (got["snp"].values == want["tx"].values).all()
    for k in COLUMNS[2:]:
        np.testing.assert_array_equal(np.isnan(got[k].values), np.isnan(want[k].values), err_msg=k)
    live = np.isfinite(want["de_coef"].values)
    assert live.sum() > len(want) // 2
    for k in ("de_coef", "dv_coef"):
        np.testing.assert_array_equal(got[k].values, want[k].values, err_msg=k)
    for k, tol in (("de_se", 1e-10), ("dv_se", 1e-10), ("de_pval", 1e-8), ("dv_pval", 1e-8)):
        err = np.nanmax(np.abs(got[k].values - want[k].values))
        print(f"resample_rep {resample_rep} approx {approx} rng {rng}: max |{k} difference| {err:.3g}")
        np.testing.assert_allclose(got[k].values, want[k].values, rtol=0, atol=tol, equal_nan=True, err_msg=k)


@pytest.mark.parametrize("rng", ["replay", "fast"])
@pytest.mark.parametrize("resample_rep", [False, True])
def test_chunking_changes_no_bit(donors, resample_rep, rng):
    """max_rows forcing 1, 3 and all genes per chunk: bit-identical frames.  (The device draws of resample_rep are keyed by the gene's
    position among the kept genes; those of ht_1d_moments by its slot in the chunk, which moves with max_rows.)"""
    adata, memento, cov, geno, pairs = donors
    n_genes, ng = len(adata.uns["memento"]["_hip"].gene_idx), 24
    frames = []
    for per_chunk in (1, 3, n_genes):
        np.random.seed(2)
        frames.append(memento.ht_1d_eqtl(adata, geno, pairs, covariate=cov, num_boot=B, rng=rng, fill_seed=4, max_rows=per_chunk * ng,
                                         approx=resample_rep, resample_rep=resample_rep))
        assert adata.uns["memento"]["_hip"].last_chunk[1] - adata.uns["memento"]["_hip"].last_chunk[0] == (
            per_chunk if n_genes % per_chunk == 0 else n_genes % per_chunk)
    for f in frames[1:]:
        pd.testing.assert_frame_equal(f, frames[0], check_exact=True)
    assert np.isfinite(frames[0]["de_pval"]).sum() > len(frames[0]) // 2


def test_rows_and_stored_arrays(donors):
    """Gene-major over the kept genes, each gene's SNPs in its list order; a frame of pairs gives the same result as the dict; a
    gene without a list has no row; the arrays are kept in ``uns``."""
    adata, memento, cov, geno, pairs = donors
    names = _names(adata)
    np.random.seed(2)
    df = memento.ht_1d_eqtl(adata, geno, pairs, covariate=cov, num_boot=B, approx=True)
    assert list(df.columns) == COLUMNS
    assert list(zip(df["gene"], df["snp"])) == [(g, s) for g in names for s in pairs[g]]
    ht = adata.uns["memento"]["1d_ht_eqtl"]
    np.testing.assert_array_equal(ht["mean_coef"], df["de_coef"].values)
    np.testing.assert_array_equal(ht["var_asl"], df["dv_pval"].values)
    frame = pd.DataFrame([(g, s) for g in reversed(names[2:]) for s in pairs[g]] + [("no_such_gene", "rs1")], columns=["gene", "snp"])
    np.random.seed(2)
    sub = memento.ht_1d_eqtl(adata, geno, frame, covariate=cov, num_boot=B, approx=True)
    assert list(zip(sub["gene"], sub["snp"])) == [(g, s) for g in names[2:] for s in pairs[g]]
    keep = ~df["gene"].isin(names[:2]).values
    pd.testing.assert_frame_equal(sub.reset_index(drop=True), df[keep].reset_index(drop=True), check_exact=True)
    no_cov = memento.ht_1d_eqtl(adata, geno, {names[3]: pairs[names[3]]}, num_boot=B, approx=True)
    assert len(no_cov) == len(pairs[names[3]])


def test_rejected_arguments(donors):
    adata, memento, cov, geno, pairs = donors
    for kw in (dict(strict=True), dict(ci=0.9), dict(max_boot=4 * B), dict(treatment_for_gene=pairs)):
        with pytest.raises(TypeError):
            memento.ht_1d_eqtl(adata, geno, pairs, covariate=cov, num_boot=B, **kw)
    with pytest.raises(ValueError):
        memento.ht_1d_eqtl(adata, geno, pairs, covariate=cov, num_boot=B, rng="numpy")
    with pytest.raises(ValueError, match="rs999"):
        memento.ht_1d_eqtl(adata, geno, {_names(adata)[0]: ["rs999"]}, covariate=cov, num_boot=B)
    with pytest.raises(ValueError):
        memento.ht_1d_eqtl(adata, geno.iloc[:5], pairs, covariate=cov, num_boot=B)
