"""Guide-vs-control tests with replicate covariates on the GPU (ht_1d_vs_control(..., treatment_col=...),
mm_contrast_design_stats / mm_contrast_design_rows): exact against the oracle's _regress_1d on each test's subset design,
consistent with the unstratified call, the C-ABI on its own, against the REAL reference's per-guide loop with a replicate
covariate (fixture guide_loop_strata), and at the configs[4] shape with 3 replicate strata."""

import os
import subprocess
import sys
import time

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KEYS = ["de_coef", "de_se", "de_pval", "dv_coef", "dv_se", "dv_pval"]


def _strata_adata(seed=41, n_cells=6000, n_genes=200, density=0.12):
    """4 guides + control (guide 0) x 3 replicates; guide 4 only in replicate 0, so that a bad control group in that replicate
    leaves no stratum with both arms.  Sparse genes make some groups bad."""
    from scrna_parameter_estimation_amd.synth import synth_adata

    adata = synth_adata(n_cells, n_genes, density, 1, 3, seed, dtype=np.float32)
    rng = np.random.default_rng(seed + 7)
    guide = rng.choice(5, size=n_cells, p=[0.32, 0.17, 0.17, 0.17, 0.17])
    rep = adata.obs["rep"].values.copy()
    rep[guide == 4] = 0
    adata.obs["rep"] = rep
    adata.obs["guide"] = guide
    return adata


def _prepare(adata, label_columns, min_perc_group=0.5):
    from scrna_parameter_estimation_amd import memento

    memento.setup_memento(adata, q_column="q")
    memento.create_groups(adata, label_columns=label_columns)
    memento.compute_1d_moments(adata, min_perc_group=min_perc_group)
    return memento


def _oracle_check(adata, df, approx, max_tests=None):
    """Every test of the resident gene chunk against orc.regress_1d on the reference's subset design."""
    from oracle import memento_oracle as orc
    from scrna_parameter_estimation_amd import engine

    m = adata.uns["memento"]
    st = m["_hip"]
    groups = m["groups"]
    ng = len(groups)
    lab = np.array([g.split("^")[1:] for g in groups])
    Nc = np.array([m["group_cells"][k].shape[0] for k in groups], dtype=float)
    guides = m["1d_ht_vs_control"]["groups"]
    ctrl = m["1d_ht_vs_control"]["control"]
    bs, (g0, g1), good = st.last_bootstrap, st.last_chunk, st.last_good
    n_checked = n_nan = 0
    tests = [(gi, k) for gi in range(g0, g1) for k in range(len(guides))]
    if max_tests is not None:
        r = np.random.default_rng(5)
        tests = [tests[i] for i in r.choice(len(tests), size=min(max_tests, len(tests)), replace=False)]
    for gi, k in tests:
        g = guides[k]
        S = np.flatnonzero((lab[:, 0] == g) | (lab[:, 0] == ctrl))
        mask = good[gi - g0][S]
        Sg = S[mask]
        is_g = lab[Sg, 0] == g
        both = set(lab[Sg[is_g], 1]) & set(lab[Sg[~is_g], 1])
        got = df.iloc[gi * len(guides) + k][KEYS].values.astype(float)
        if not both:                                          # no good guide / control group, or no stratum with both arms
            assert np.isnan(got).all(), (gi, g, got)
            n_nan += 1
            continue
        dummies = pd.get_dummies(pd.Series(lab[S, 1]), drop_first=True).values.astype(float)[mask]
        cov = np.column_stack([np.ones(len(Sg)), dummies])
        rows = (gi - g0) * ng + Sg
        ym, yv = engine.host(bs.ym[rows]), engine.host(bs.yv[rows])
        ref = orc.regress_1d(cov, is_g.astype(float)[:, None], ym, yv, Nc[Sg], resampling="bootstrap", approx=approx)
        want = np.array([ref[0][0], ref[1][0], ref[2][0], ref[3][0], ref[4][0], ref[5][0]])
        np.testing.assert_allclose(got[[0, 1, 3, 4]], want[[0, 1, 3, 4]], rtol=1e-8, atol=1e-8, err_msg=f"gene {gi} guide {g}")
        np.testing.assert_allclose(got[[2, 5]], want[[2, 5]], rtol=0, atol=1e-5, err_msg=f"gene {gi} guide {g}")
        n_checked += 1
    return n_checked, n_nan


@pytest.mark.parametrize("approx", [True, False])
def test_strata_exact_against_the_oracle(approx):
    adata = _strata_adata()
    memento = _prepare(adata, ["guide", "rep"])
    np.random.seed(7)
    df = memento.ht_1d_vs_control(adata, control=0, num_boot=200, num_cpus=4, approx=approx, treatment_col="guide")
    m = adata.uns["memento"]
    rec = m["1d_ht_vs_control"]
    assert rec["treatment_col"] == "guide" and rec["covariates"] == ["rep"] and rec["control"] == "0"
    assert sorted(rec["groups"]) == ["1", "2", "3", "4"]
    G = len(m["_hip"].gene_idx)
    assert list(df.columns) == ["gene", "group"] + KEYS and len(df) == G * 4
    assert m["_hip"].last_chunk == (0, G)
    n_checked, n_nan = _oracle_check(adata, df, approx)
    print(f"\nstrata vs oracle (approx={approx}): {n_checked} tests exact, {n_nan} NaN tests")
    assert n_checked > 100 and n_nan > 0
    # some tests use a design with a bad stratum (fewer than all of their groups)
    good = m["_hip"].last_good
    assert not good.all()


def test_strata_rejects_bad_arguments():
    adata = _strata_adata(n_cells=3000, n_genes=150, density=0.15)
    memento = _prepare(adata, ["guide", "rep"])
    with pytest.raises(ValueError):
        memento.ht_1d_vs_control(adata, control=0, num_boot=50, treatment_col="cond")
    with pytest.raises(ValueError):
        memento.ht_1d_vs_control(adata, control=9, num_boot=50, treatment_col="guide")
    np.random.seed(1)
    a = memento.ht_1d_vs_control(adata, control="0", num_boot=50, treatment_col="guide")
    np.random.seed(1)
    b = memento.ht_1d_vs_control(adata, control=0, num_boot=50, treatment_col="guide")
    for k in KEYS:
        np.testing.assert_array_equal(a[k].values, b[k].values)


def test_single_label_column_equals_the_unstratified_call_and_chunks_agree():
    adata = _strata_adata(seed=43)
    memento = _prepare(adata, ["guide"])
    m = adata.uns["memento"]
    ctrl = [k for k in m["groups"] if k.split("^")[-1] == "0"][0]
    np.random.seed(11)
    old = memento.ht_1d_vs_control(adata, control=ctrl, num_boot=300, num_cpus=2, approx=False)
    np.random.seed(11)
    new = memento.ht_1d_vs_control(adata, control=0, num_boot=300, num_cpus=2, approx=False, treatment_col="guide")
    assert len(old) == len(new) and (old["gene"].values == new["gene"].values).all()
    assert [g.split("^")[-1] for g in old["group"].values] == list(new["group"].values)
    for k in KEYS:
        np.testing.assert_array_equal(np.isnan(old[k].values), np.isnan(new[k].values), err_msg=k)
        np.testing.assert_allclose(new[k].values, old[k].values, rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=k)
    # several gene chunks == one chunk (stratified design)
    adata2 = _strata_adata(seed=44)
    memento = _prepare(adata2, ["guide", "rep"])
    np.random.seed(12)
    one = memento.ht_1d_vs_control(adata2, control=0, num_boot=200, num_cpus=2, approx=True, treatment_col="guide")
    ng = len(adata2.uns["memento"]["groups"])
    np.random.seed(12)
    many = memento.ht_1d_vs_control(adata2, control=0, num_boot=200, num_cpus=2, approx=True, treatment_col="guide", max_rows=ng * 17)
    st = adata2.uns["memento"]["_hip"]
    assert st.last_chunk[0] > 0                                    # it did run in several chunks
    assert (one["gene"].values == many["gene"].values).all() and (one["group"].values == many["group"].values).all()
    for k in ("de_coef", "dv_coef"):
        np.testing.assert_allclose(many[k].values, one[k].values, rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=k)
    # the replay streams are per chain and the refill streams are keyed by (gene, group): standard errors and p-values too
    assert np.isfinite(one["de_se"].values).sum() > len(one) // 4
    for k in KEYS:
        np.testing.assert_array_equal(many[k].values, one[k].values, err_msg=k)


CHILD = r'''
import ctypes, sys
import numpy as np
assert "torch" not in sys.modules
lib = ctypes.CDLL(sys.argv[1])
lib.mm_last_error.restype = ctypes.c_char_p
V = ctypes.c_void_p
def ck(rc):
    if rc != 0:
        raise RuntimeError(lib.mm_last_error().decode())
def dmalloc(nbytes):
    p = V(); ck(lib.mm_malloc(ctypes.byref(p), ctypes.c_size_t(max(nbytes, 16)))); return p
def to_dev(a):
    a = np.ascontiguousarray(a); p = dmalloc(a.nbytes)
    if a.nbytes:
        ck(lib.mm_memcpy_h2d(p, a.ctypes.data_as(V), ctypes.c_size_t(a.nbytes), None))
    return p
def to_host(p, shape, dtype):
    out = np.empty(shape, dtype=dtype)
    ck(lib.mm_sync(None))
    if out.nbytes:
        ck(lib.mm_memcpy_d2h(out.ctypes.data_as(V), p, ctypes.c_size_t(out.nbytes), None))
    return out
i32, i64 = ctypes.c_int32, ctypes.c_int64
d = np.load(sys.argv[2])
ym, yv = d["ym"], d["yv"]
ld, B, ng = int(d["ld"]), int(d["B"]), int(d["ng"])
tg, td, ptr, grp, w = d["test_gene"], d["test_design"], d["ptr"], d["grp"], d["w"]
n = len(tg)
args = [to_dev(ym), to_dev(yv), i64(ld), i32(B), i32(ng), to_dev(tg), to_dev(td), to_dev(ptr), to_dev(grp), to_dev(w), i64(n)]
d_sm, d_sv = dmalloc(n * 64), dmalloc(n * 64)
ck(lib.mm_contrast_design_stats(*args, d_sm, d_sv, None))
out = {"sm": to_host(d_sm, (n, 8), np.float64), "sv": to_host(d_sv, (n, 8), np.float64)}
for which in (0, 1):
    d_r = dmalloc(n * ld * 8)
    ck(lib.mm_contrast_design_rows(*args, i32(which), d_r, None))
    out[f"rows{which}"] = to_host(d_r, (n, ld), np.float64)
np.savez(sys.argv[3], **out)
print("ok")
'''


def _np_stats(row):
    """The 8-double record of k_contrast_design_stats / k_contract_stats restated in numpy for one coefficient row (NaN = dropped)."""
    c0 = row[0]
    ok = np.isfinite(row)
    v = row[1:][ok[1:]]
    n = len(v)
    mean1 = v.mean() if n else np.nan
    allv = row[ok]
    lo, hi = (allv.min(), allv.max()) if len(allv) else (np.inf, -np.inf)
    return np.array([c0, np.sqrt(((v - mean1) ** 2).sum() / n) if n else np.nan, n, (np.abs(v - c0) > abs(c0)).sum(), mean1 - c0,
                     1.0 if lo == hi else 0.0, (np.abs(v) > abs(c0)).sum(), hi - lo])


def test_design_contrast_cabi_without_torch(tmp_path):
    rng = np.random.default_rng(21)
    n_genes, ng, B = 3, 7, 600
    ld = B + 3                                                    # a leading dimension larger than B + 1
    ym = rng.normal(0, 1, size=(n_genes * ng, ld))
    yv = rng.normal(0, 1, size=(n_genes * ng, ld))
    ym[2, 5] = np.nan; yv[4, 17] = np.inf; ym[9, 0] = np.nan; yv[15, 100:140] = np.nan; ym[20, 599] = -np.inf
    ptr = np.array([0, 3, 3, 7, 9], dtype=np.int32)               # design 1 is empty (a NaN test)
    grp = np.array([0, 2, 4, 1, 3, 5, 6, 2, 6], dtype=np.int32)
    w = rng.normal(0, 1, size=len(grp))
    w[5] = 0.0                                                    # a zero weight still decides the column's validity
    test_gene = np.array([0, 0, 1, 1, 2, 2, 0, 1, 2, 1], dtype=np.int32)
    test_design = np.array([0, 1, 2, 3, 0, 2, 3, 0, 3, 1], dtype=np.int32)
    np.savez(tmp_path / "in.npz", ym=ym, yv=yv, ld=ld, B=B, ng=ng, test_gene=test_gene, test_design=test_design, ptr=ptr, grp=grp, w=w)
    child = tmp_path / "child.py"
    child.write_text(CHILD)
    lib = os.path.join(ROOT, "scrna_parameter_estimation_amd", "csrc", "libmemento_hip.so")
    r = subprocess.run([sys.executable, str(child), lib, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = np.load(tmp_path / "out.npz")
    for t in range(len(test_gene)):
        p0, p1 = ptr[test_design[t]], ptr[test_design[t] + 1]
        rows = test_gene[t] * ng + grp[p0:p1]
        for which, y, key in ((0, ym, "sm"), (1, yv, "sv")):
            if p1 == p0:
                want_row = np.full(B + 1, np.nan)
                want = np.array([np.nan, np.nan, 0, 0, np.nan, 0, np.nan, np.nan])
            else:
                ok = np.isfinite(ym[rows, :B + 1]).all(axis=0) & np.isfinite(yv[rows, :B + 1]).all(axis=0)
                want_row = np.where(ok, (w[p0:p1, None] * y[rows, :B + 1]).sum(axis=0), np.nan)
                want = _np_stats(want_row)
            np.testing.assert_allclose(out[f"rows{which}"][t, :B + 1], want_row, rtol=1e-13, atol=1e-13, equal_nan=True)
            np.testing.assert_allclose(out[key][t], want, rtol=1e-11, atol=1e-12, equal_nan=True, err_msg=f"test {t} {key}")


def test_strata_against_the_references_per_guide_loop():
    """The reference's per-guide loop with a replicate covariate (fixture guide_loop_strata: subset to control + guide,
    create_groups(['is_guide', 'rep']), covariates intercept + rep dummies, num_boot=400, approx=True) against ONE batched
    ht_1d_vs_control(..., treatment_col='guide') call.  The mean coefficient is the same quantity (W applied to the same group
    log-means with the global size factors) where both use the same groups; SEs differ by Monte-Carlo error only; the
    variability coefficient differs by the pooled mean-variance fit (all groups here, the subset there)."""
    from scrna_parameter_estimation_amd import AnnDataLite, memento

    g = dict(np.load(os.path.join(GOLDEN, "guide_loop_strata.npz"), allow_pickle=False))
    X = sp.csr_matrix((g["in_data"].astype(np.float32), g["in_indices"], g["in_indptr"]), shape=tuple(g["in_shape"]))
    obs = pd.DataFrame({"guide": g["in_guide"], "rep": g["in_rep"], "q": g["in_q"]}, index=[f"c{i}" for i in range(X.shape[0])])
    adata = AnnDataLite(X, obs, pd.DataFrame(index=g["in_gene_names"].tolist()))
    memento.setup_memento(adata, q_column="q")
    np.testing.assert_allclose(adata.obs["memento_size_factor"].values, g["size_factor"], rtol=1e-12)
    memento.create_groups(adata, label_columns=["guide", "rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.9)
    m = adata.uns["memento"]
    names = memento.main._var_names(adata).tolist()
    with np.errstate(invalid="ignore"):
        usable = {k: ~(np.isnan(m["1d_moments"][k][0]) | np.isnan(m["1d_moments"][k][2]) | (m["1d_moments"][k][0] == 0)
                       | (m["1d_moments"][k][2] < 0)) for k in m["groups"]}
    np.random.seed(5)
    df = memento.ht_1d_vs_control(adata, control=0, num_boot=400, num_cpus=1, approx=True, treatment_col="guide")
    n_guides = int(g["n_guides"])
    ratio_se, diff_dv, n, n_same = [], [], 0, 0
    for gid in range(1, n_guides + 1):
        sub = df[df["group"] == str(gid)].set_index("gene")
        genes = [x for x in g[f"g{gid}_genes"].tolist() if x in sub.index]
        assert len(genes) > 0.6 * len(g[f"g{gid}_genes"])
        idx = [g[f"g{gid}_genes"].tolist().index(x) for x in genes]
        ours = sub.loc[genes]
        ref_groups = g[f"g{gid}_groups"].tolist()                  # "is_guide^rep"
        with np.errstate(invalid="ignore"):
            ref_usable = ~(np.isnan(g[f"g{gid}_mean"]) | np.isnan(g[f"g{gid}_rv"]) | (g[f"g{gid}_mean"] == 0) | (g[f"g{gid}_rv"] < 0))
        our_label = {lab: f"sg^{gid if lab.split('^')[0] == '1' else 0}^{lab.split('^')[1]}" for lab in ref_groups}
        ref_de, ref_se, ref_dv = g[f"g{gid}_mean_coef"][idx], g[f"g{gid}_mean_se"][idx], g[f"g{gid}_var_coef"][idx]
        same = np.array([all(bool(usable[our_label[lab]][names.index(x)]) == bool(ref_usable[j, i]) for j, lab in enumerate(ref_groups))
                         for x, i in zip(genes, idx)])
        ok = np.isfinite(ref_de) & np.isfinite(ours["de_coef"].values)
        np.testing.assert_allclose(ours["de_coef"].values[ok & same], ref_de[ok & same], rtol=1e-8, atol=1e-8, err_msg=f"guide {gid}")
        ratio_se.append(np.median(ours["de_se"].values[ok] / ref_se[ok]))
        okv = ok & np.isfinite(ref_dv) & np.isfinite(ours["dv_coef"].values)
        diff_dv.append(np.median(np.abs(ours["dv_coef"].values[okv] - ref_dv[okv])))
        n += int(ok.sum())
        n_same += int((ok & same).sum())
    print(f"\nper-guide loop with replicates vs batched: {n} (gene, guide) tests ({n_same} with the same usable groups); median de_se "
          f"ratio per guide {np.round(ratio_se, 3).tolist()}; median |dv_coef diff| per guide {np.round(diff_dv, 4).tolist()}")
    assert n_same > 0.9 * n and n > 150
    assert all(0.85 < r < 1.15 for r in ratio_se)
    assert max(diff_dv) < 0.1


def test_c5_perturbseq_full_shape_with_replicate_strata():
    """configs[4] (200k cells x 15k genes, 500 guides + control, B = 5,000) with 3 replicate strata through
    ht_1d_vs_control(..., treatment_col='guide'): 1,503 groups, one test per (kept gene, guide)."""
    import torch

    import bench
    from oracle import memento_oracle as orc
    from scrna_parameter_estimation_amd import AnnDataLite, memento
    from scrna_parameter_estimation_amd.memento import design

    cells, genes, n_guides, n_rep, B = 200_000, 15_000, 500, 3, 5_000
    csr = bench.synth_device_csr(dict(cells=cells, genes=genes, density=0.05), 20250117 + 5, torch)
    rng = np.random.default_rng(20250117 + 5)
    is_ctrl = rng.random(cells) < 0.2
    guide = np.where(is_ctrl, 0, 1 + rng.integers(0, n_guides, size=cells))
    rep = rng.integers(0, n_rep, size=cells)
    obs = pd.DataFrame({"guide": guide, "rep": rep, "q": np.full(cells, 0.07)})
    adata = AnnDataLite(sp.csr_matrix((cells, genes), dtype=np.float32), obs, pd.DataFrame(index=[f"g{i}" for i in range(genes)]))
    memento.setup_memento(adata, q_column="q", device_csr=csr)
    memento.create_groups(adata, label_columns=["guide", "rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.7, subset_var=False)
    m = adata.uns["memento"]
    st = m["_hip"]
    groups = m["groups"]
    ng = len(groups)
    assert ng == (n_guides + 1) * n_rep
    G = len(st.gene_idx)
    np.random.seed(0)
    torch.cuda.synchronize(); t0 = time.time()
    df = memento.ht_1d_vs_control(adata, control=0, num_boot=B, num_cpus=8, approx=True, treatment_col="guide")
    torch.cuda.synchronize(); t1 = time.time()
    print(f"\nC5 x {n_rep} strata: {G} genes x {n_guides} guides = {len(df)} tests, {ng} groups, B={B}: {t1 - t0:.1f} s -> "
          f"{len(df) / (t1 - t0):.0f} tests/s")
    guides = m["1d_ht_vs_control"]["groups"]
    assert len(df) == G * n_guides and G > 1000 and len(guides) == n_guides
    # ---- invariants over all tests --------------------------------------------------------------------------------
    lab = np.array([g.split("^")[1:] for g in groups])
    Nc = np.array([m["group_cells"][k].shape[0] for k in groups], dtype=float)
    mean = np.stack([m["1d_moments"][g][0] for g in groups])        # [group][gene]
    rv = np.stack([m["1d_moments"][g][2] for g in groups])
    with np.errstate(invalid="ignore", divide="ignore"):
        usable = ~(np.isnan(mean) | np.isnan(rv) | (mean == 0) | (rv < 0))
        lmean = np.log(mean)
    de, dv, pv = (df[k].values.reshape(G, n_guides) for k in ("de_coef", "dv_coef", "de_pval"))
    want_ok = np.zeros((G, n_guides), dtype=bool)
    want_de = np.full((G, n_guides), np.nan)
    ctrl_rows = {r: np.flatnonzero((lab[:, 0] == "0") & (lab[:, 1] == str(r)))[0] for r in range(n_rep)}
    for k, gv in enumerate(guides):
        S = np.flatnonzero((lab[:, 0] == gv) | (lab[:, 0] == "0"))
        trt = (lab[S, 0] == gv).astype(float)[:, None]
        cov = np.column_stack([np.ones(len(S)), pd.get_dummies(pd.Series(lab[S, 1]), drop_first=True).values.astype(float)])
        U = usable[S].T                                              # [gene][|S|]
        both = np.zeros(G, dtype=bool)
        for r in range(n_rep):
            gr = np.flatnonzero((lab[:, 0] == gv) & (lab[:, 1] == str(r)))
            if len(gr):
                both |= usable[gr[0]] & usable[ctrl_rows[r]]
        want_ok[:, k] = both
        codes = U.astype(np.int64) @ (np.int64(1) << np.arange(len(S), dtype=np.int64))
        _, first, inv = np.unique(codes, return_index=True, return_inverse=True)
        for u, row in enumerate(first):
            sel = np.asarray(inv).reshape(-1) == u
            if not both[row]:
                continue
            W = design.weight_rows(cov, trt, Nc[S], U[row])[0]
            with np.errstate(invalid="ignore"):
                want_de[sel, k] = np.where(U[row][None, :], W[None, :] * lmean[S][:, sel].T, 0.0).sum(axis=1)
    ok = np.isfinite(de)
    np.testing.assert_array_equal(ok, want_ok)
    assert 0.5 < ok.mean() < 1.0, ok.mean()
    np.testing.assert_allclose(de[ok], want_de[ok], rtol=1e-9, atol=1e-10)
    assert np.isfinite(dv[ok]).mean() > 0.99
    assert ((pv[ok] >= 0) & (pv[ok] <= 1)).all() and (df["de_se"].values.reshape(G, n_guides)[ok] > 0).all()
    assert 0.3 < np.median(pv[ok]) < 0.7                              # guide labels are independent of the counts
    # ---- oracle spot check: 20 tests of the last gene chunk == _regress_1d on the reference's subset design -------------
    n_checked, _ = _oracle_check(adata, df, approx=True, max_tests=20)
    assert n_checked >= 15
