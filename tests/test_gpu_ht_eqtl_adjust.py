"""``ht_1d_eqtl(adjust=True)`` on the small synthetic donor data of tests/test_gpu_ht_eqtl.py (3,000 cells, 24 donor groups, 2
covariates, 40 genes, 1-40 SNPs per gene, 300 replicates): the unadjusted columns do not move, the adjusted ones equal the numpy
restatement (tests/_eqtl_family_ref.py, tests/_family_ref.py) on the rows of the last chunk, the gene chunking changes no bit,
copies of one SNP do not change a gene's adjusted p-value, and the eGene table."""

import numpy as np
import pandas as pd
import pytest

import _eqtl_family_ref as ref
import _family_ref

pytestmark = pytest.mark.gpu
B = 300
COLUMNS = ["gene", "snp", "de_coef", "de_se", "de_pval", "dv_coef", "dv_se", "dv_pval"]
ADJUSTED = ["de_pval_adj", "dv_pval_adj", "n_family"]


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
    for k in range(9):
        geno[f"copy{k}"] = geno["rs3"]                                       # one genotype column under nine names
    names = _names(adata)
    assert len(gdf) == 24 and len(names) >= 20
    pairs = {g: [f"rs{j}" for j in rng.choice(60, size=int(rng.integers(1, 41)), replace=False)] for g in names}
    pairs[names[0]] = ["rs7", "rs3"]
    pairs[names[1]] = ["rs7"]                                                # a gene whose whole treatment is all ones: never resampled
    return adata, memento, cov, geno, pairs


def _run(donors, pairs=None, **kw):
    adata, memento, cov, geno, all_pairs = donors
    np.random.seed(2)
    return memento.ht_1d_eqtl(adata, geno, all_pairs if pairs is None else pairs, covariate=cov, num_boot=B, num_cpus=1, fill_seed=4, **kw)


def test_adjust_adds_its_columns_and_arrays(donors):
    df = _run(donors, adjust=True, approx=True)
    assert list(df.columns) == COLUMNS + ADJUSTED and len(df) > 100
    ht = donors[0].uns["memento"]["1d_ht_eqtl"]
    np.testing.assert_array_equal(ht["mean_asl_adj"], df["de_pval_adj"].values)
    np.testing.assert_array_equal(ht["var_asl_adj"], df["dv_pval_adj"].values)
    np.testing.assert_array_equal(ht["n_family"], df["n_family"].values)
    assert ht["n_family"].dtype == ht["var_n_family"].dtype == np.int64 and len(ht["var_n_family"]) == len(df)
    live = np.isfinite(df["de_pval_adj"].values)
    assert live.sum() > len(df) // 2
    assert (df["de_pval_adj"].values[live] >= df["de_pval"].values[live]).all() and (df["de_pval_adj"].values[live] <= 1).all()
    plain = _run(donors, approx=True)
    assert list(plain.columns) == COLUMNS and "mean_asl_adj" not in donors[0].uns["memento"]["1d_ht_eqtl"]
    assert donors[0].uns["memento"]["_hip"].last_eqtl is None


@pytest.mark.parametrize("rng", ["replay", "fast"])
@pytest.mark.parametrize("resample_rep", [False, True])
def test_the_unadjusted_columns_do_not_move(donors, resample_rep, rng):
    kw = dict(resample_rep=resample_rep, rng=rng, approx=not resample_rep)
    off, on = _run(donors, **kw), _run(donors, adjust=True, **kw)
    pd.testing.assert_frame_equal(on[COLUMNS], off, check_exact=True)


@pytest.mark.parametrize("rng", ["replay", "fast"])
@pytest.mark.parametrize("resample_rep", [False, True])
def test_one_chunk_call_against_the_restatement(donors, resample_rep, rng):
    """All rows of the call through ``st.last_eqtl``; per gene and plane the restatement of the rule on them gives the frame's
    adjusted p-values and family sizes exactly.  resample_rep=False: the family is all the gene's tests, and it also equals
    ``_family_ref.family`` on the weight-row designs and the resident replicate planes.  resample_rep=True: the resampled tests."""
    from scrna_parameter_estimation_amd import engine

    adata = donors[0]
    st = adata.uns["memento"]["_hip"]
    df = _run(donors, adjust=True, resample_rep=resample_rep, rng=rng, approx=True)
    le, bs = st.last_eqtl, st.last_bootstrap
    n_genes, ng = len(_names(adata)), 24
    assert st.last_chunk == (0, n_genes) and len(le.gene_ptr) == n_genes + 1
    idx = le.rr_idx if resample_rep else np.arange(len(df))                   # the frame rows of the family members
    assert le.gene_ptr[-1] == len(idx) == len(le.scale) and (len(idx) < len(df)) == resample_rep
    position = {g: k for k, g in enumerate(_names(adata))}
    gene_of_row = np.array([position[g] for g in df["gene"].values])
    want_adj = {c: np.full(len(df), np.nan) for c in ("de", "dv")}
    want_n = np.zeros((len(df), 2), dtype=np.int64)
    some_invalid = 0
    for which, c in ((0, "de"), (1, "dv")):
        rows = le.rows(which, np.arange(len(idx)))
        coef0, own = df[c + "_coef"].values[idx], df[c + "_pval"].values[idx]
        np.testing.assert_array_equal(rows[:, 0][np.isfinite(coef0)], coef0[np.isfinite(coef0)])
        for g in range(n_genes):
            lo, hi = le.gene_ptr[g], le.gene_ptr[g + 1]
            nb = B + 1 if not resample_rep else (B if le.n_valid is None else int(le.n_valid[g]) - 1)
            f = ref.family(rows[lo:hi, :max(nb, 0)], coef0[lo:hi], le.scale[lo:hi, which])
            np.testing.assert_array_equal(le.adj[lo:hi, which, 0], f["t0"])
            np.testing.assert_array_equal(le.adj[lo:hi, which, 1], f["n_adj"])
            assert le.fam[g, which].tolist() == [f["n_valid"], f["n_included"]]
            some_invalid += f["n_included"] > 0 and f["n_valid"] < nb - 1
            with np.errstate(invalid="ignore"):
                p = np.where(np.isnan(f["t0"]), np.nan, np.maximum((1 + f["n_adj"]) / (1 + f["n_valid"]), own[lo:hi]))
            want_adj[c][idx[lo:hi]] = p
            want_n[gene_of_row == g, which] = int(f["n_included"])
        np.testing.assert_array_equal(df[c + "_pval_adj"].values, want_adj[c])
    np.testing.assert_array_equal(df["n_family"].values, want_n[:, 0])
    np.testing.assert_array_equal(adata.uns["memento"]["1d_ht_eqtl"]["var_n_family"], want_n[:, 1])
    assert np.isfinite(want_adj["de"]).sum() > len(idx) // 2
    print(f"resample_rep {resample_rep} rng {rng}: families with an invalid slot {some_invalid}")
    if resample_rep:
        return
    ym, yv = engine.host(bs.ym), engine.host(bs.yv)
    test_gene, test_design, ptr, grp, w = le.tables
    n_exact = 0
    for g in range(n_genes):
        t = np.arange(le.gene_ptr[g], le.gene_ptr[g + 1])
        assert (test_gene[t] == g).all()
        designs = [(grp[ptr[d]:ptr[d + 1]], w[ptr[d]:ptr[d + 1]]) for d in test_design[t]]
        fam = _family_ref.family(ym[g * ng:(g + 1) * ng, :B + 1], yv[g * ng:(g + 1) * ng, :B + 1], designs, le.scale[t])
        np.testing.assert_array_equal(le.adj[t, :, 0], fam["t0"])
        np.testing.assert_array_equal(le.fam[g, :, 0], fam["n_valid"])
        np.testing.assert_array_equal(le.fam[g, :, 1], fam["n_included"])
        if _family_ref.near_ties(fam) == 0:
            np.testing.assert_array_equal(le.adj[t, :, 1], fam["n_adj"])
            n_exact += 1
    assert n_exact >= n_genes - 3


@pytest.mark.parametrize("rng", ["replay", "fast"])
@pytest.mark.parametrize("resample_rep", [False, True])
def test_chunking_changes_no_bit(donors, resample_rep, rng):
    """max_rows forcing 1, 3 and all genes per chunk: bit-identical frames -- a family never spans chunks."""
    adata = donors[0]
    n_genes, ng = len(adata.uns["memento"]["_hip"].gene_idx), 24
    frames = [_run(donors, adjust=True, resample_rep=resample_rep, rng=rng, approx=True, max_rows=per_chunk * ng)
              for per_chunk in (1, 3, n_genes)]
    for f in frames[1:]:
        pd.testing.assert_frame_equal(f, frames[0], check_exact=True)
    assert np.isfinite(frames[0]["de_pval_adj"]).sum() > len(frames[0]) // 2


@pytest.mark.parametrize("resample_rep", [False, True])
def test_copies_of_one_snp_do_not_change_the_adjusted_pvalue(donors, resample_rep):
    """One genotype column under nine names (more than a tile) against the same gene with the one-SNP list: the maximum over equal
    members is the member, so every adjusted p-value equals the single one bit for bit, and none is below its own p-value."""
    gene = _names(donors[0])[4]
    kw = dict(adjust=True, resample_rep=resample_rep, approx=True)
    nine = _run(donors, pairs={gene: [f"copy{k}" for k in range(9)]}, **kw)
    one = _run(donors, pairs={gene: ["rs3"]}, **kw)
    assert len(nine) == 9 and len(one) == 1 and nine["n_family"].tolist() == [9] * 9 and one["n_family"].tolist() == [1]
    for c in ("de", "dv"):
        assert np.isfinite(one[c + "_pval_adj"].values).all()
        assert (nine[c + "_pval_adj"].values.view(np.int64) == one[c + "_pval_adj"].values.view(np.int64)[0]).all()
        assert (one[c + "_pval_adj"].values >= one[c + "_pval"].values).all() and (nine[c + "_pval_adj"].values >= nine[c + "_pval"].values).all()


def test_a_constant_snp_is_outside_the_family(donors):
    """resample_rep=True: the gene whose list is rs7 alone (all ones) has a plain test, which is no joint draw with resampled
    tests: NaN adjusted values, a family of none.  In every gene ``n_family`` counts the members with an adjusted value."""
    adata = donors[0]
    names = _names(adata)
    df = _run(donors, adjust=True, resample_rep=True, approx=True)
    alone = df[df["gene"] == names[1]]
    assert alone["snp"].tolist() == ["rs7"] and np.isfinite(alone["de_pval"].values).all()
    assert np.isnan(alone[["de_pval_adj", "dv_pval_adj"]].values).all() and alone["n_family"].tolist() == [0]
    var_n = adata.uns["memento"]["1d_ht_eqtl"]["var_n_family"]
    for g in names:
        mine = (df["gene"] == g).values
        assert (df["n_family"].values[mine] == np.isfinite(df["de_pval_adj"].values[mine]).sum()).all()
        assert (var_n[mine] == np.isfinite(df["dv_pval_adj"].values[mine]).sum()).all()
    assert (df["n_family"].values > 1).sum() > len(df) // 2


@pytest.mark.parametrize("resample_rep", [False, True])
def test_gene_table(donors, resample_rep):
    from scrna_parameter_estimation_amd.memento import util

    adata, memento = donors[0], donors[1]
    df = _run(donors, adjust=True, resample_rep=resample_rep, approx=True)
    genes = memento.get_eqtl_gene_result(adata)
    names = _names(adata)
    assert genes["gene"].tolist() == names and genes["n_snps"].tolist() == [len(donors[4][g]) for g in names]
    for c in ("de", "dv"):
        gene_p = []
        for k, g in enumerate(names):
            mine = df[df["gene"] == g]
            p_adj = mine[c + "_pval_adj"].values
            if np.isnan(p_adj).all():
                assert genes[c + "_lead_snp"][k] is None and np.isnan(genes[c + "_gene_pval"][k])
                gene_p.append(np.nan)
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                t0 = np.where(np.isnan(p_adj), np.nan, np.abs(mine[c + "_coef"].values) * (1.0 / mine[c + "_se"].values))
            lead = mine.iloc[int(np.nanargmax(t0))]
            assert genes[c + "_lead_snp"][k] == lead["snp"]
            assert genes[c + "_coef"][k] == lead[c + "_coef"] and genes[c + "_se"][k] == lead[c + "_se"] and genes[c + "_pval"][k] == lead[c + "_pval"]
            assert genes[c + "_gene_pval"][k] == np.nanmin(p_adj)
            gene_p.append(np.nanmin(p_adj))
        np.testing.assert_array_equal(genes[c + "_gene_qval"].values, util._fdrcorrect(np.array(gene_p)))
    assert genes["n_family"].tolist() == [int(df.loc[df["gene"] == g, "n_family"].iloc[0]) for g in names]
    _run(donors, resample_rep=resample_rep, approx=True)
    with pytest.raises(ValueError):
        memento.get_eqtl_gene_result(adata)


def test_adjust_needs_the_centred_bootstrap(donors):
    with pytest.raises(ValueError, match="adjust"):
        _run(donors, adjust=True, resampling="permutation")
