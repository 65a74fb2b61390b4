"""Guide-vs-control coexpression tests on the GPU (ht_2d_vs_control, Bootstrap2D.contrast_design, mm_contrast_design1_stats /
mm_contrast_design1_rows): the kernels against numpy, the batched call against the REAL reference's per-guide loop (fixture
guide_loop_2d, plain and with a replicate covariate), the two-group identity with ht_2d_moments, chunk invariance, the API
edges, and one sizeable Perturb-seq shaped run checked through invariants."""

import os
import time

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from _replicate_ref import _np_stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KEYS = ["corr_coef", "corr_se", "corr_pval"]


def _plane(yc, ng, B, ld):
    """A Bootstrap2D that only holds replicate rows (what contrast_design reads)."""
    from scrna_parameter_estimation_amd import engine

    bs = object.__new__(engine.Bootstrap2D)
    bs.yc, bs.ld, bs.B, bs.ng, bs.n_pairs, bs.n_q = engine.dev(yc), ld, B, ng, yc.shape[0] // ng, yc.shape[0]
    return bs


def test_single_plane_contrast_kernels_against_numpy():
    rng = np.random.default_rng(31)
    n_pairs, R, B = 5, 3, 700
    ng = 4 * R                                                    # control + 3 guides, R strata
    ld = B + 4                                                    # a leading dimension larger than B + 1
    y = np.tanh(rng.normal(0, 0.6, size=(n_pairs * ng, ld)))
    y[2, 5] = np.nan; y[4, 17] = np.inf; y[9, 0] = np.nan; y[15, 100:140] = np.nan; y[20, B] = -np.inf; y[2 * ng + 3, 1:B + 1:7] = np.nan
    y[3 * ng + 1] = 0.25                                           # a constant row: with design 5 below, an all-equal test
    y[3 * ng + 2] = 0.25
    # designs: 0 = empty, 1..3 = plain {(guide, +1), (control, -1)}, 4 = 2R entries with regression-like weights (one of them
    # zero: it still decides the column's validity), 5 = two constant rows
    ptr = np.array([0, 0, 2, 4, 6, 6 + 2 * R, 8 + 2 * R], dtype=np.int32)
    grp = np.array([3, 0, 7, 0, 11, 2] + list(range(0, 2 * R)) + [1, 2], dtype=np.int32)
    w = np.concatenate([np.tile([1.0, -1.0], 3), rng.normal(0, 1, size=2 * R), [1.0, -1.0]])
    w[6 + 2] = 0.0
    test_pair = np.array([0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 0, 1, 3], dtype=np.int32)
    test_design = np.array([1, 2, 4, 0, 3, 4, 1, 5, 2, 4, 0, 3, 4, 4], dtype=np.int32)
    bs = _plane(y, ng, B, ld)
    stats, rows_of = bs.contrast_design(test_pair, test_design, ptr, grp, w)
    rows = rows_of(np.arange(len(test_pair)))
    assert stats.shape == (len(test_pair), 8) and rows.shape == (len(test_pair), ld)
    n_empty = n_dropped = 0
    for t in range(len(test_pair)):
        p0, p1 = ptr[test_design[t]], ptr[test_design[t] + 1]
        r = test_pair[t] * ng + grp[p0:p1]
        if p1 == p0:
            want_row = np.full(B + 1, np.nan)
            want = np.array([np.nan, np.nan, 0, 0, np.nan, 0, np.nan, np.nan])
            n_empty += 1
        else:
            ok = np.isfinite(y[r, :B + 1]).all(axis=0)
            acc = np.zeros(B + 1)
            with np.errstate(invalid="ignore"):
                for q in range(p0, p1):                            # the kernel's summation order
                    acc = acc + w[q] * y[test_pair[t] * ng + grp[q], :B + 1]
            want_row = np.where(ok, acc, np.nan)
            want = _np_stats(want_row)
            n_dropped += int((~ok).sum())
        np.testing.assert_allclose(rows[t, :B + 1], want_row, rtol=1e-13, atol=1e-13, equal_nan=True, err_msg=f"test {t}")
        np.testing.assert_allclose(stats[t], want, rtol=1e-11, atol=1e-12, equal_nan=True, err_msg=f"test {t}")
    assert n_empty == 2 and n_dropped > 100
    assert stats[7, 5] == 1.0                                      # the all-equal flag of the constant test
    # a subset of rows on demand is the same rows
    np.testing.assert_array_equal(rows_of([4, 2])[:, :B + 1], rows[[4, 2], :B + 1])      # (columns beyond B + 1 are padding, never written)
    # the kernel trusts its tables: the host refuses bad ones
    for bad in (dict(test_pair=np.array([n_pairs])), dict(test_design=np.array([len(ptr) - 1])), dict(grp=np.r_[grp[:-1], ng]),
                dict(ptr=np.r_[ptr[:-1], ptr[-1] + 1]), dict(w=w[:-1]), dict(grp=np.r_[grp[:-1], -1])):
        a = dict(test_pair=test_pair[:1], test_design=test_design[:1], ptr=ptr, grp=grp, w=w)
        a.update(bad)
        with pytest.raises(ValueError):
            bs.contrast_design(a["test_pair"], a["test_design"], a["ptr"], a["grp"], a["w"])
    stats0, _ = bs.contrast_design(np.zeros(0, np.int32), np.zeros(0, np.int32), ptr, grp, w)
    assert stats0.shape == (0, 8)


# -------------------------------------------------------------------------------------------------
# against the reference's per-guide loop
# -------------------------------------------------------------------------------------------------


def _fixture_adata(g, label_columns):
    from scrna_parameter_estimation_amd import AnnDataLite, memento

    X = sp.csr_matrix((g["in_data"].astype(np.float32), g["in_indices"], g["in_indptr"]), shape=tuple(g["in_shape"]))
    obs = pd.DataFrame({"guide": g["in_guide"], "rep": g["in_rep"], "q": g["in_q"]}, index=[f"c{i}" for i in range(X.shape[0])])
    adata = AnnDataLite(X, obs, pd.DataFrame(index=g["in_gene_names"].tolist()))
    memento.setup_memento(adata, q_column="q")
    np.testing.assert_allclose(adata.obs["memento_size_factor"].values, g["size_factor"], rtol=1e-12)
    memento.create_groups(adata, label_columns=label_columns)
    memento.compute_1d_moments(adata, min_perc_group=0.9)
    return adata, memento


@pytest.mark.parametrize("strata", [False, True])
def test_against_the_references_per_guide_loop(strata):
    """The reference's per-guide coexpression loop (fixture guide_loop_2d: subset to control + guide, create_groups, compute_1d_moments,
    compute_2d_moments, ht_2d_moments with num_boot=400, approx=True; with strata the covariates are intercept + rep dummies) against
    ONE batched ht_2d_vs_control call.  The per-group correlation uses the global size factors and no mean-variance fit, so corr_coef
    is the same number (1e-8) wherever both sides use the same groups, and the NaN tests are the same there; SEs differ by
    Monte-Carlo error only (two reference runs with different seeds stay within 0.85..1.15 as well: make_guide_2d_fixture.py)."""
    g = dict(np.load(os.path.join(GOLDEN, "guide_loop_2d.npz"), allow_pickle=False))
    tag = "s" if strata else "p"
    adata, memento = _fixture_adata(g, ["guide", "rep"] if strata else ["guide"])
    m = adata.uns["memento"]
    kept = set(memento.main._var_names(adata).tolist())
    all_pairs = list(zip(g["in_pair_1"].tolist(), g["in_pair_2"].tolist()))
    ours_idx = [i for i, (a, b) in enumerate(all_pairs) if a in kept and b in kept]
    assert len(ours_idx) > 0.9 * len(all_pairs)
    memento.compute_2d_moments(adata, [all_pairs[i] for i in ours_idx])
    np.random.seed(5)
    if strata:
        df = memento.ht_2d_vs_control(adata, control=0, num_boot=int(g["num_boot"]), num_cpus=1, approx=True, treatment_col="guide")
    else:
        df = memento.ht_2d_vs_control(adata, control="sg^0", num_boot=int(g["num_boot"]), num_cpus=1, approx=True)
    n_guides = int(g["n_guides"])
    tested = m["2d_ht_vs_control"]["groups"]
    assert len(df) == len(ours_idx) * n_guides and list(df.columns) == ["gene_1", "gene_2", "group"] + KEYS
    groups = m["groups"]
    with np.errstate(invalid="ignore"):
        our_usable = {k: ~(np.isnan(m["2d_moments"][k]["corr"]) | (np.abs(m["2d_moments"][k]["corr"]) == 1)) for k in groups}
    n = n_same = n_nan = 0
    ratios = []
    for gid in range(1, n_guides + 1):
        label = str(gid) if strata else f"sg^{gid}"
        k = tested.index(label)
        ours = {key: df[key].values.reshape(len(ours_idx), n_guides)[:, k] for key in KEYS}
        ref_pairs = g[f"{tag}_g{gid}_pairs"].tolist()
        common = [i for i in ours_idx if i in ref_pairs]
        assert len(common) > 0.9 * len(all_pairs)
        oi = np.array([ours_idx.index(i) for i in common])
        ri = np.array([ref_pairs.index(i) for i in common])
        ref_groups = g[f"{tag}_g{gid}_groups"].tolist()            # "is_guide^rep" or "is_guide"
        ref_corr = g[f"{tag}_g{gid}_corr"][:, ri]
        with np.errstate(invalid="ignore"):
            ref_usable = ~(np.isnan(ref_corr) | (np.abs(ref_corr) == 1))

        def our_label(lab):
            parts = lab.split("^")
            return "^".join(["sg", str(gid) if parts[0] == "1" else "0"] + parts[1:])

        # the per-group correlation of the subset run is the one of the all-groups run
        for j, lab in enumerate(ref_groups):
            np.testing.assert_allclose(m["2d_moments"][our_label(lab)]["corr"][oi], ref_corr[j], rtol=1e-8, atol=1e-8, equal_nan=True)
        same = np.array([all(bool(our_usable[our_label(lab)][o]) == bool(ref_usable[j, c]) for j, lab in enumerate(ref_groups))
                         for c, o in enumerate(oi)])
        same |= np.array([all_pairs[i][0] == all_pairs[i][1] for i in common])     # self pairs are skipped by rule on both sides
        ref_coef, ref_se = g[f"{tag}_g{gid}_corr_coef"][ri], g[f"{tag}_g{gid}_corr_se"][ri]
        got_coef, got_se = ours["corr_coef"][oi], ours["corr_se"][oi]
        print(f"\n[{'strata' if strata else 'plain'}] guide {gid}: {len(common)} pairs, same usable groups {int(same.sum())}, NaN ours "
              f"{int(np.isnan(got_coef).sum())} / reference {int(np.isnan(ref_coef).sum())}, max |coef diff| "
              f"{np.nanmax(np.abs(got_coef - ref_coef)[same]):.3g}")
        np.testing.assert_array_equal(np.isnan(got_coef[same]), np.isnan(ref_coef[same]), err_msg=f"guide {gid}")
        np.testing.assert_allclose(got_coef[same], ref_coef[same], rtol=1e-8, atol=1e-8, equal_nan=True, err_msg=f"guide {gid}")
        ok = np.isfinite(ref_se) & np.isfinite(got_se)
        ratios.append(float(np.median(got_se[ok] / ref_se[ok])))
        pv = ours["corr_pval"][oi]
        assert ((pv[ok] >= 0) & (pv[ok] <= 1)).all()
        n += len(common)
        n_same += int(same.sum())
        n_nan += int(np.isnan(got_coef[same]).sum())
    print(f"[{'strata' if strata else 'plain'}] {n} (pair, guide) tests, {n_same} with the same usable groups ({n_nan} of them NaN); "
          f"median corr_se ratio ours / reference per guide {np.round(ratios, 3).tolist()}")
    assert n > 150 and n - n_same <= 0.1 * n
    assert all(0.85 < r < 1.15 for r in ratios), ratios


# -------------------------------------------------------------------------------------------------
# identities of the public call
# -------------------------------------------------------------------------------------------------


def _guide_adata(seed, n_cells=6000, n_genes=150, density=0.2, n_guides=1, n_rep=1, coupled=0):
    """Guides 1..n_guides + control 0 (a third of the cells).  ``coupled`` > 0: in the cells of guide 1 the counts of gene
    top[2k + 1] get a thinned copy of gene top[2k] added for k < coupled -- pairs whose correlation really
    differs between guide and control, so that their extreme counts are small and the tail fit of approx=False triggers."""
    from scrna_parameter_estimation_amd.synth import synth_adata

    adata = synth_adata(n_cells, n_genes, density, 1, n_rep, seed, dtype=np.float32)
    rng = np.random.default_rng(seed + 3)
    guide = rng.choice(n_guides + 1, size=n_cells, p=np.r_[1 / 3, np.full(n_guides, 2 / 3 / n_guides)])
    X = adata.X.toarray()
    top = np.argsort(-X.mean(axis=0), kind="stable")[3:27]         # (the few best expressed genes dominate the size factor and can fail the variance filter)
    cells = np.flatnonzero(guide == 1)
    for k in range(coupled):
        a, b = top[2 * k], top[2 * k + 1]
        X[cells, b] = X[cells, b] + rng.binomial(X[cells, a].astype(np.int64), 0.12)
    adata.X = sp.csr_matrix(X.astype(np.float32))
    adata.obs["guide"] = guide
    names = np.array(adata.var.index.tolist())
    return adata, names[top]


def _prepare(adata, label_columns, pairs, min_perc_group=0.7):
    from scrna_parameter_estimation_amd import memento

    memento.setup_memento(adata, q_column="q")
    memento.create_groups(adata, label_columns=label_columns)
    memento.compute_1d_moments(adata, min_perc_group=min_perc_group)
    kept = set(memento.main._var_names(adata).tolist())
    pairs = [p for p in pairs if p[0] in kept and p[1] in kept]
    memento.compute_2d_moments(adata, pairs)
    return memento, pairs


def _top_pairs(top, n, seed, coupled=0):
    rng = np.random.default_rng(seed)
    pairs = [(top[2 * k], top[2 * k + 1]) for k in range(coupled)]
    seen = {frozenset(p) for p in pairs}
    while len(pairs) < n:                                          # distinct unordered pairs, no self pairs
        a, b = rng.integers(0, len(top), size=2)
        if a != b and frozenset((top[a], top[b])) not in seen:
            seen.add(frozenset((top[a], top[b])))
            pairs.append((top[a], top[b]))
    return [(str(a), str(b)) for a, b in pairs]


@pytest.mark.parametrize("approx", [True, False])
def test_two_groups_equal_ht_2d_moments(approx):
    """With exactly {control, one guide} the two calls draw the same uniforms and see identical replicate rows: coefficient and SE
    agree to 1e-10, p-values to 1e-8 -- a test may differ by up to 2/(B+1) where rounding moves a replicate across the
    extreme-count threshold (w1*a + w2*b there, a - b here), for at most 2 % of the tests.  approx=False runs at a B where the
    tail fit triggers (pairs coupled in the guide's cells have extreme counts <= 10)."""
    B = 300
    adata, top = _guide_adata(51, coupled=6)
    memento, pairs = _prepare(adata, ["guide"], _top_pairs(top, 60, 52, coupled=6) + [(str(top[0]), str(top[0]))])
    m = adata.uns["memento"]
    gdf = memento.get_groups(adata)
    cov = pd.DataFrame({"intercept": np.ones(len(gdf))}, index=gdf.index)
    trt = pd.DataFrame({"is_guide": (gdf["guide"].astype(int) == 1).astype(float)}, index=gdf.index)
    np.random.seed(9)
    memento.ht_2d_moments(adata, covariate=cov, treatment=trt, num_boot=B, num_cpus=1, verbose=0, resampling="bootstrap", approx=approx,
                          resample_rep=False)
    after_old = np.random.random()
    old = {k: np.asarray(m["2d_ht"][k]).copy() for k in ("corr_coef", "corr_se", "corr_asl")}
    active = m["_hip"].last_bootstrap2d.active.copy()
    np.random.seed(9)
    df = memento.ht_2d_vs_control(adata, control="sg^0", num_boot=B, num_cpus=1, approx=approx)
    assert np.random.random() == after_old                         # the global stream was consumed identically
    assert m["_hip"].last_bootstrap2d.active.all() and active.all()  # both groups of every tested pair are good: same tests on both sides
    assert len(df) == len(pairs) and (df["group"] == "sg^1").all()
    stats_c = m["_hip"].last_bootstrap2d
    assert stats_c is not None and m["_hip"].last_chunk2d == (0, len(pairs) - 1)
    new = {k: df[c].values for k, c in zip(("corr_coef", "corr_se", "corr_asl"), KEYS)}
    for k in old:
        np.testing.assert_array_equal(np.isnan(new[k]), np.isnan(old[k]), err_msg=k)
    assert np.isnan(new["corr_coef"]).sum() == 1                   # the self pair
    np.testing.assert_allclose(new["corr_coef"], old["corr_coef"], rtol=1e-10, atol=1e-10, equal_nan=True)
    np.testing.assert_allclose(new["corr_se"], old["corr_se"], rtol=1e-10, atol=1e-10, equal_nan=True)
    fin = np.isfinite(old["corr_asl"])
    dp = np.abs(new["corr_asl"][fin] - old["corr_asl"][fin])
    loose = dp > 1e-8
    print(f"\ntwo groups (approx={approx}): {int(fin.sum())} tests, max |dp| {dp.max():.3g}, {int(loose.sum())} beyond 1e-8; smallest p "
          f"{old['corr_asl'][fin].min():.3g}")
    assert (dp[loose] <= 2.0 / (B + 1) + 1e-12).all() and loose.sum() <= 0.02 * fin.sum()
    if not approx:
        # the tail fit did trigger: p-values below 11 / (B + 1) come from it (hypothesis_test.py:88-141)
        assert (old["corr_asl"][fin] < 10.5 / (B + 1)).sum() >= 3


def test_chunks_agree_and_api_edges():
    adata, top = _guide_adata(61, n_guides=3, n_rep=2)
    base = _top_pairs(top, 40, 62)
    pairs_in = [base[0], (base[0][1], base[0][0]), (str(top[3]), str(top[3]))] + base[1:] + [base[5], (base[7][1], base[7][0])]
    memento, pairs = _prepare(adata, ["guide", "rep"], pairs_in)
    assert pairs == pairs_in
    m = adata.uns["memento"]
    ng = len(m["groups"])
    np.random.seed(21)
    one = memento.ht_2d_vs_control(adata, control=0, num_boot=200, num_cpus=1, approx=True, treatment_col="guide")
    assert m["_hip"].last_chunk2d[0] == 0
    rec = m["2d_ht_vs_control"]
    assert set(rec) == {"corr_coef", "corr_se", "corr_asl", "control", "groups", "treatment_col", "covariates"}
    assert rec["control"] == "0" and rec["treatment_col"] == "guide" and rec["covariates"] == ["rep"] and sorted(rec["groups"]) == ["1", "2", "3"]
    n_t = 3
    assert len(one) == len(pairs) * n_t and list(one.columns) == ["gene_1", "gene_2", "group"] + KEYS
    assert one["gene_1"].tolist() == [a for a, _ in pairs for _ in range(n_t)] and one["group"].tolist() == rec["groups"] * len(pairs)
    for k, c in zip(("corr_coef", "corr_se", "corr_asl"), KEYS):
        assert rec[k].shape == (len(pairs) * n_t,)
        np.testing.assert_array_equal(rec[k], one[c].values)
    tab = {c: one[c].values.reshape(len(pairs), n_t) for c in KEYS}
    for c in KEYS:
        assert np.isnan(tab[c][2]).all()                           # the self pair
        assert np.isfinite(tab[c][0]).all()
        np.testing.assert_array_equal(tab[c][1], tab[c][0])        # reversed duplicate: the first one's result
        np.testing.assert_array_equal(tab[c][-2], tab[c][3 + 4])   # base[5] again
        np.testing.assert_array_equal(tab[c][-1], tab[c][3 + 6])   # base[7] reversed
    # at least 3 chunks give the same table
    np.random.seed(21)
    many = memento.ht_2d_vs_control(adata, control=0, num_boot=200, num_cpus=1, approx=True, treatment_col="guide", max_rows=ng * 11)
    lo, hi = m["_hip"].last_chunk2d
    assert lo >= 22 and hi == 40                                   # 40 distinct pairs, 11 per chunk: the last of 4 chunks
    for c in KEYS:
        np.testing.assert_allclose(many[c].values, one[c].values, rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=c)
    # errors: an absent control value, a treatment column that is not a label column, resample_rep is not accepted
    with pytest.raises(ValueError):
        memento.ht_2d_vs_control(adata, control=9, num_boot=50, treatment_col="guide")
    with pytest.raises(ValueError):
        memento.ht_2d_vs_control(adata, control=0, num_boot=50, treatment_col="cond")
    with pytest.raises(ValueError):
        memento.ht_2d_vs_control(adata, control="sg^9^0", num_boot=50)
    with pytest.raises(TypeError):
        memento.ht_2d_vs_control(adata, control=0, num_boot=50, treatment_col="guide", resample_rep=True)
    # a control given as label value and as string; plain form: index and label
    np.random.seed(3)
    a = memento.ht_2d_vs_control(adata, control="0", num_boot=60, approx=True, treatment_col="guide")
    np.random.seed(3)
    b = memento.ht_2d_vs_control(adata, control=0, num_boot=60, approx=True, treatment_col="guide")
    ctrl = m["groups"][2]
    np.random.seed(3)
    c_lab = memento.ht_2d_vs_control(adata, control=ctrl, num_boot=60, approx=True)
    np.random.seed(3)
    c_idx = memento.ht_2d_vs_control(adata, control=2, num_boot=60, approx=True)
    rec = m["2d_ht_vs_control"]
    assert set(rec) == {"corr_coef", "corr_se", "corr_asl", "control", "groups"} and rec["control"] == ctrl
    assert rec["groups"] == [k for k in m["groups"] if k != ctrl] and len(c_idx) == len(pairs) * (ng - 1)
    for c in KEYS:
        np.testing.assert_array_equal(a[c].values, b[c].values)
        np.testing.assert_array_equal(c_lab[c].values, c_idx[c].values)
    # the plain statistic is the difference of the stored per-group correlations
    corr = np.stack([m["2d_moments"][k]["corr"] for k in m["groups"]], axis=1)       # [pair][group]
    want = np.delete(corr, 2, axis=1) - corr[:, [2]]
    got = c_idx["corr_coef"].values.reshape(len(pairs), ng - 1)
    fin = np.isfinite(got)
    assert fin.mean() > 0.9
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=1e-12)


def test_perturbseq_shape_with_replicate_strata():
    """About 200 guides + control x 3 replicate strata, 2,000 pairs among the best expressed genes, B = 2,000, guide labels
    independent of the counts: 603 groups, one test per (pair, guide), several pair chunks."""
    import torch

    import bench
    from scrna_parameter_estimation_amd import AnnDataLite, memento
    from scrna_parameter_estimation_amd.memento import design

    cells, genes, n_guides, n_rep, B, n_pairs = 120_000, 3_000, 200, 3, 2_000, 2_000
    csr = bench.synth_device_csr(dict(cells=cells, genes=genes, density=0.05), 20250117 + 6, torch)
    rng = np.random.default_rng(20250117 + 6)
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
    names = memento.main._var_names(adata)
    mean_all = np.mean([m["1d_moments"][k][0] for k in groups], axis=0)
    top = names[np.argsort(-mean_all, kind="stable")[:90]]
    iu, ju = np.triu_indices(len(top), 1)
    pick = rng.choice(len(iu), size=n_pairs, replace=False)
    pairs = [(str(top[a]), str(top[b])) for a, b in zip(iu[pick], ju[pick])]
    memento.compute_2d_moments(adata, pairs)
    np.random.seed(0)
    torch.cuda.synchronize(); t0 = time.time()
    df = memento.ht_2d_vs_control(adata, control=0, num_boot=B, num_cpus=8, approx=True, treatment_col="guide")
    torch.cuda.synchronize(); t1 = time.time()
    print(f"\n{n_pairs} pairs x {n_guides} guides = {len(df)} tests, {ng} groups, B={B}: {t1 - t0:.1f} s -> {len(df) / (t1 - t0):.0f} tests/s; "
          f"last chunk {st.last_chunk2d}")
    tested = m["2d_ht_vs_control"]["groups"]
    assert len(df) == n_pairs * n_guides and len(tested) == n_guides and st.last_chunk2d[0] > 0
    # ---- the design rule and the folded weights, recomputed on the host from the stored per-group correlations ----------------
    lab = np.array([g.split("^")[1:] for g in groups])
    Nc = np.array([m["group_cells"][k].shape[0] for k in groups], dtype=float)
    corr = np.stack([m["2d_moments"][k]["corr"] for k in groups])                     # [group][pair]
    with np.errstate(invalid="ignore"):
        usable = ~(np.isnan(corr) | (np.abs(corr) == 1))
    coef, se, pv = (df[k].values.reshape(n_pairs, n_guides) for k in KEYS)
    want_ok = np.zeros((n_pairs, n_guides), dtype=bool)
    want = np.full((n_pairs, n_guides), np.nan)
    ctrl_rows = {r: np.flatnonzero((lab[:, 0] == "0") & (lab[:, 1] == str(r)))[0] for r in range(n_rep)}
    for k, gv in enumerate(tested):
        S = np.flatnonzero((lab[:, 0] == gv) | (lab[:, 0] == "0"))
        trt = (lab[S, 0] == gv).astype(float)[:, None]
        cov = np.column_stack([np.ones(len(S)), pd.get_dummies(pd.Series(lab[S, 1]), drop_first=True).values.astype(float)])
        U = usable[S].T                                              # [pair][|S|]
        both = np.zeros(n_pairs, dtype=bool)
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
                want[sel, k] = np.where(U[row][None, :], W[None, :] * corr[S][:, sel].T, 0.0).sum(axis=1)
    ok = np.isfinite(coef)
    np.testing.assert_array_equal(ok, want_ok)
    print(f"finite tests {ok.mean():.4f}; usable (pair, group) {usable.mean():.4f}; median p {np.median(pv[ok]):.3f}")
    assert ok.mean() > 0.5
    np.testing.assert_allclose(coef[ok], want[ok], rtol=1e-9, atol=1e-9)
    assert (se[ok] > 0).all() and ((pv[ok] >= 0) & (pv[ok] <= 1)).all()
    assert 0.3 < np.median(pv[ok]) < 0.7                              # guide labels are independent of the counts
