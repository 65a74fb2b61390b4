"""``ht_2d_posthoc`` end to end on the matrix and the pair list of tests/test_gpu_ht_2d_joint.py (6,000 cells x 150 genes, 3 levels x
2 replicates = 6 groups, 60 distinct pairs among well-expressed genes plus a reversed duplicate and a self pair, num_boot = 300):
every member against the ``ht_2d_vs_control`` call it restates, the many-to-one form, the invariants of the adjusted columns, pair
chunking under both generators, the last chunk's resident correlation rows through the numpy restatement (tests/_family_ref.py given
the plane twice), whole groups as levels, pairs with skipped groups, planted changes and the argument check.

Six pairs carry a planted change: in the cells of level 1 gene b gets a thinned copy (THIN) of gene a added.  Three unplanted pairs
are given skipped groups by hand, through a NaN true correlation in ``uns['memento']['2d_moments']`` after ``compute_2d_moments``: one
loses one group, one both groups of a level, one all groups."""

import numpy as np
import pytest
import scipy.sparse as sp

import _family_ref as ref
from test_gpu_vs_control_2d import _prepare, _top_pairs

pytestmark = pytest.mark.gpu
B = 300
SEED, FILL = 5, 9
N_PLANTED = 6
THIN = 0.15
CI = 0.95
ONE, LEVEL, ALL = 20, 21, 22                # positions (in the base pair list) of the pairs that lose groups
DUP_OF = 10
TEST_COLS = ["corr_coef", "corr_se", "corr_pval"]
ADJ_COLS = ["corr_pval_adj", "n_family"]
SCI_COLS = ["corr_sci_lo", "corr_sci_hi"]
N_MEM = 3


def _matrix():
    """(adata, requested pairs, number of distinct pairs): the matrix and the pair list of tests/test_gpu_ht_2d_joint.py."""
    from scrna_parameter_estimation_amd.synth import synth_adata

    adata = synth_adata(6000, 150, 0.2, 3, 2, seed=71, dtype=np.float32)
    X = adata.X.toarray()
    rng = np.random.default_rng(74)
    top = np.argsort(-X.mean(axis=0), kind="stable")[3:27]
    cells = np.flatnonzero(adata.obs["cond"].values == 1)
    for k in range(N_PLANTED):
        a, b = top[2 * k], top[2 * k + 1]
        X[cells, b] = X[cells, b] + rng.binomial(X[cells, a].astype(np.int64), THIN)
    adata.X = sp.csr_matrix(X.astype(np.float32))
    names = np.array(adata.var.index.tolist())[top]
    base = _top_pairs(names, 60, 72, coupled=N_PLANTED)
    return adata, base + [(base[DUP_OF][1], base[DUP_OF][0]), (str(names[0]), str(names[0]))], len(base)


@pytest.fixture(scope="module")
def prepared():
    """SimpleNamespace: adata, memento, gdf (group frame), pairs, the positions of the special pairs and ``joint``, the result of
    ``ht_2d_joint`` on the same matrix before any true correlation was overwritten."""
    from types import SimpleNamespace

    adata, pairs_in, n_base = _matrix()
    memento, pairs = _prepare(adata, ["cond", "rep"], pairs_in)
    assert pairs == pairs_in
    p = SimpleNamespace(adata=adata, memento=memento, gdf=memento.get_groups(adata), pairs=pairs, n_base=n_base, dup=n_base, self_pair=n_base + 1)
    m = adata.uns["memento"]
    cond = p.gdf["cond"].values.astype(int)
    np.random.seed(SEED)
    p.joint = memento.ht_2d_joint(adata, "cond", covariate=["rep"], num_boot=B, fill_seed=FILL)
    for i, g in enumerate(m["groups"]):
        if i == 3:
            m["2d_moments"][g]["corr"][ONE] = np.nan
        if cond[i] == 2:
            m["2d_moments"][g]["corr"][LEVEL] = np.nan
        m["2d_moments"][g]["corr"][ALL] = np.nan
    p.levels = list(dict.fromkeys(str(v) for v in p.gdf["cond"].values))      # in the order of their first appearance among the groups
    p.level_pairs = [(p.levels[a], p.levels[b]) for a, b in ref.pairwise(len(p.levels))]
    return p


def _posthoc(p, treatment_col="cond", **kw):
    np.random.seed(SEED)
    return p.memento.ht_2d_posthoc(p.adata, treatment_col, num_boot=B, fill_seed=FILL, **kw)


def _vs_control(p, control, **kw):
    np.random.seed(SEED)
    return p.memento.ht_2d_vs_control(p.adata, control, num_boot=B, fill_seed=FILL, treatment_col="cond", **kw)


def _same(a, b, cols):
    assert len(a) == len(b) and list(a["gene_1"]) == list(b["gene_1"]) and list(a["gene_2"]) == list(b["gene_2"])
    for c in cols:
        np.testing.assert_array_equal(a[c].values, b[c].values, err_msg=c)         # NaNs in the same places, the same bits elsewhere


@pytest.fixture(scope="module")
def one_chunk(prepared):
    return _posthoc(prepared, ci=CI)


@pytest.fixture(scope="module")
def vs_controls(prepared):
    """{control level: ht_2d_vs_control(control=level)} for the three levels, approx=False."""
    return {b: _vs_control(prepared, int(b)) for b in prepared.levels}


def _block(df, pos):
    return df.iloc[N_MEM * pos:N_MEM * (pos + 1)]


def test_result_layout(prepared, one_chunk):
    p, df = prepared, one_chunk
    n = len(p.pairs)
    assert list(df.columns) == ["gene_1", "gene_2", "level_a", "level_b"] + TEST_COLS + ADJ_COLS + SCI_COLS
    assert len(df) == N_MEM * n
    assert list(zip(df["gene_1"], df["gene_2"])) == [pair for pair in p.pairs for _ in range(N_MEM)]      # pair-major, the requested order
    lv = p.levels
    assert sorted(lv) == ["0", "1", "2"] and p.level_pairs == [(lv[1], lv[0]), (lv[2], lv[0]), (lv[2], lv[1])]
    assert list(zip(df["level_a"], df["level_b"])) == p.level_pairs * n                                    # a after b; by b, then a
    out = p.adata.uns["memento"]["2d_ht_posthoc"]
    assert set(out) == {"corr_coef", "corr_se", "corr_asl", "corr_asl_adj", "n_family", "corr_sci", "ci", "levels", "level_a", "level_b",
                        "treatment_col", "control"}
    assert out["levels"] == lv and list(zip(out["level_a"], out["level_b"])) == p.level_pairs
    assert out["control"] is None and out["treatment_col"] == "cond" and out["ci"] == CI
    for k in ("corr_coef", "corr_se", "corr_asl", "corr_asl_adj", "n_family"):
        assert out[k].shape == (N_MEM * n,)
    assert out["corr_sci"].shape == (N_MEM * n, 2) and out["n_family"].dtype == np.int64
    np.testing.assert_array_equal(out["corr_asl"], df["corr_pval"].values)
    np.testing.assert_array_equal(out["corr_asl_adj"], df["corr_pval_adj"].values)
    np.testing.assert_array_equal(out["corr_sci"][:, 1], df["corr_sci_hi"].values)
    plain = _posthoc(p)                                             # without ci: the same numbers, no interval columns
    _same(df, plain, TEST_COLS + ADJ_COLS)
    assert list(plain.columns) == list(df.columns)[:-2]
    out = p.adata.uns["memento"]["2d_ht_posthoc"]
    assert "ci" not in out and "corr_sci" not in out


@pytest.mark.parametrize("approx", [False, True])
def test_every_member_is_the_vs_control_test(prepared, one_chunk, vs_controls, approx):
    """For every control level b: the rows with level_b = b are the rows ht_2d_vs_control(control=b) has for the later levels, bit
    for bit, NaNs included."""
    p = prepared
    df = one_chunk if not approx else _posthoc(p, approx=True)
    lv = p.levels
    n_checked = 0
    for b, later in ((lv[0], lv[1:]), (lv[1], lv[2:])):
        vc = vs_controls[b] if not approx else _vs_control(p, int(b), approx=True)
        for a in later:
            mine = df[(df["level_b"] == b) & (df["level_a"] == a)]
            theirs = vc[vc["group"] == a]
            _same(mine, theirs, TEST_COLS)
            n_checked += int(np.isfinite(mine["corr_pval"].values).sum())
    assert n_checked > N_MEM * 0.9 * p.n_base
    if approx:
        _same(df, one_chunk, ["corr_coef", "corr_se", "n_family"])
        assert (df["corr_pval"].values != one_chunk["corr_pval"].values).sum() > len(df) // 2


def test_many_to_one(prepared, one_chunk, vs_controls):
    """control=0, and likewise 1 and 2: the rows of ht_2d_vs_control(control=...) plus the adjusted columns, the other levels in
    their order of appearance.  The family against the first level is the first two members of the pairwise family, which is
    larger: no adjusted p-value of the smaller family is above the pairwise family's for the same member."""
    p = prepared
    lv = p.levels
    for control in (0, 1, 2):
        one = _posthoc(p, control=control)
        vc = vs_controls[str(control)]
        _same(one, vc, TEST_COLS)
        assert list(one["level_a"]) == list(vc["group"]) and list(one["level_a"][:2]) == [v for v in lv if v != str(control)]
        assert (one["level_b"] == str(control)).all() and p.adata.uns["memento"]["2d_ht_posthoc"]["control"] == str(control)
        assert list(one.columns) == ["gene_1", "gene_2", "level_a", "level_b"] + TEST_COLS + ADJ_COLS and (one["n_family"] <= 2).all()
        if str(control) == lv[0]:
            small = one
    large = one_chunk[one_chunk["level_b"] == lv[0]]
    _same(small, large, TEST_COLS)
    q_small, q_large = small["corr_pval_adj"].values, large["corr_pval_adj"].values
    both = np.isfinite(q_small) & np.isfinite(q_large)
    print(f"\nmany-to-one: {both.sum()} members in both families, {(q_small[both] < q_large[both]).sum()} with a smaller adjusted p-value, "
          f"{(q_small[both] > q_large[both]).sum()} with a larger one")
    assert both.sum() > len(small) * 0.9 and (q_small[both] <= q_large[both]).all() and (q_small[both] < q_large[both]).any()
    assert (np.isnan(q_small) == np.isnan(q_large)).all()


def test_invariants(prepared, one_chunk):
    df = one_chunk
    p, q = df["corr_pval"].values, df["corr_pval_adj"].values
    coef, se = df["corr_coef"].values, df["corr_se"].values
    with np.errstate(invalid="ignore"):
        has_test = np.isfinite(coef) & np.isfinite(se) & (se > 0)
    assert (np.isnan(q) == ~has_test).all() and has_test.sum() > 0.9 * len(df)         # NaN exactly where the member has no test
    live = np.isfinite(q)
    assert (q[live] >= p[live]).all()
    assert (q[live] >= 1 / (B + 1)).all() and (q[live] <= 1).all()  # n_valid <= B: never below 1 / (n_valid + 1)
    lo, hi = df["corr_sci_lo"].values, df["corr_sci_hi"].values
    assert (lo[live] < coef[live]).all() and (coef[live] < hi[live]).all() and np.isnan(lo[~live]).all() and np.isnan(hi[~live]).all()
    n_family = df["n_family"].values.reshape(-1, N_MEM)
    assert (n_family == n_family[:, :1]).all()                      # constant within a pair
    np.testing.assert_array_equal(n_family[:, 0], live.reshape(-1, N_MEM).sum(axis=1))
    # A 0.95 simultaneous interval that leaves out 0 has t0 above the 0.95 quantile of M: with n >= 250 valid columns at most 15 of
    # them lie above it, so the count-based adjusted p-value is at most 16 / 251 < 0.065 (the reported one: that or the raw one)
    out_of = (lo > 0) | (hi < 0)
    assert (q[out_of] <= np.maximum(0.065, p[out_of])).all() and out_of.sum() >= N_PLANTED


@pytest.mark.parametrize("rng", ["replay", "fast"])
def test_chunking_changes_no_number(prepared, one_chunk, rng):
    p = prepared
    st = p.adata.uns["memento"]["_hip"]
    ng = len(p.gdf)
    whole = one_chunk if rng == "replay" else _posthoc(p, rng=rng, ci=CI)
    if rng == "fast":
        assert st.last_chunk2d == (0, p.n_base)
    parts = _posthoc(p, rng=rng, ci=CI, max_rows=(ng + 1) * 17)     # 17 pairs a chunk (a pair: its groups' rows and its maximum row): 4 chunks
    assert st.last_chunk2d == (51, p.n_base)
    _same(whole, parts, TEST_COLS + ADJ_COLS + SCI_COLS)
    _posthoc(p, rng=rng, max_rows=ng * 17)                          # the maximum row counts: the same max_rows without it would be 17 pairs
    assert st.last_chunk2d == (56, p.n_base)                        # 14 pairs a chunk
    if rng == "fast":
        live = np.isfinite(one_chunk["corr_pval_adj"].values)
        assert (whole["corr_pval_adj"].values != one_chunk["corr_pval_adj"].values)[live].sum() > live.sum() // 4   # other draws than the replay
        np.testing.assert_array_equal(whole["corr_coef"].values, one_chunk["corr_coef"].values)                     # the observed column is the replay's


def test_last_chunk_against_the_restatement(prepared):
    """The last chunk's resident correlation rows and design tables through tests/_family_ref.py (the plane given twice) reproduce
    the adjusted columns and the simultaneous intervals of the returned rows."""
    from scrna_parameter_estimation_amd import engine
    from scrna_parameter_estimation_amd.memento import _ht

    p = prepared
    m = p.adata.uns["memento"]
    st = m["_hip"]
    ng = len(p.gdf)
    df = _posthoc(p, ci=CI, max_rows=(ng + 1) * 17)
    lo, hi = st.last_chunk2d
    assert (lo, hi) == (51, p.n_base)
    bs, last = st.last_bootstrap2d, st.last_posthoc2d
    assert bs.n_pairs == hi - lo and last.scale.shape == ((hi - lo) * N_MEM, 1)
    first, _ = _ht.distinct_pairs(m["2d_moments"]["gene_idx_1"], m["2d_moments"]["gene_idx_2"])
    pos = first[lo + np.asarray(bs.order)]                          # position in the requested list of every pair, device pair order
    y = engine.host(bs.yc)
    test_pair, test_design, ptr, grp, w = last.tables
    n_exact = 0
    for k in range(hi - lo):
        t = np.arange(last.family_ptr[k], last.family_ptr[k + 1])
        assert len(t) == N_MEM and (test_pair[t] == k).all()
        designs = [(grp[ptr[d]:ptr[d + 1]], w[ptr[d]:ptr[d + 1]]) for d in test_design[t]]
        rows = y[k * ng:(k + 1) * ng, :B + 1]
        own = ref.family(rows, rows, designs)
        np.testing.assert_allclose(last.scale[t, 0], own["scale"][:, 0], rtol=1e-9)
        fam = ref.family(rows, rows, designs, np.column_stack([last.scale[t, 0], last.scale[t, 0]]))
        np.testing.assert_array_equal(last.adj[t, 0, 0], fam["t0"][:, 0])
        assert last.fam[k, 0, 0] == fam["n_valid"][0] and last.fam[k, 0, 1] == fam["n_included"][0]
        got = _block(df, pos[k])
        assert (got["n_family"].values == fam["n_included"][0]).all()
        dead = np.isnan(fam["t0"][:, 0])
        half = np.where(dead, np.nan, ref.crit(fam, CI)[0] * got["corr_se"].values)
        np.testing.assert_allclose(got["corr_sci_lo"].values, got["corr_coef"].values - half, rtol=1e-12, equal_nan=True)
        np.testing.assert_allclose(got["corr_sci_hi"].values, got["corr_coef"].values + half, rtol=1e-12, equal_nan=True)
        if ref.near_ties(fam) == 0:
            np.testing.assert_array_equal(last.adj[t, 0, 1], fam["n_adj"][:, 0])
            with np.errstate(invalid="ignore"):
                want = np.where(dead, np.nan, np.maximum(ref.p_adj(fam)[:, 0], got["corr_pval"].values))   # (the reported one: after the max with the raw p)
            np.testing.assert_array_equal(got["corr_pval_adj"].values, want)
            n_exact += 1
    assert n_exact >= (hi - lo) - 1


def test_whole_groups_as_levels_on_a_one_column_grouping():
    """Grouped by ``cond`` alone, every group is a level: treatment_col=None gives the numbers of treatment_col='cond', with the
    group labels as level names."""
    adata, pairs_in, _ = _matrix()
    memento, pairs = _prepare(adata, ["cond"], pairs_in)
    groups = adata.uns["memento"]["groups"]
    assert len(groups) == 3 and len(pairs) >= 50
    np.random.seed(SEED)
    by_group = memento.ht_2d_posthoc(adata, num_boot=B, fill_seed=FILL, ci=CI)
    np.random.seed(SEED)
    by_level = memento.ht_2d_posthoc(adata, "cond", num_boot=B, fill_seed=FILL, ci=CI)
    _same(by_group, by_level, TEST_COLS + ADJ_COLS + SCI_COLS)
    assert list(by_group["level_a"][:3]) == [groups[1], groups[2], groups[2]] and list(by_group["level_b"][:3]) == [groups[0], groups[0], groups[1]]
    cond = [g.split("^")[1] for g in groups]
    assert list(by_level["level_a"][:3]) == [cond[1], cond[2], cond[2]] and list(by_level["level_b"][:3]) == [cond[0], cond[0], cond[1]]
    assert np.isfinite(by_level["corr_pval_adj"].values).mean() > 0.9
    np.random.seed(SEED)
    one = memento.ht_2d_posthoc(adata, control=groups[1], num_boot=B, fill_seed=FILL)
    np.random.seed(SEED)
    _same(one, memento.ht_2d_posthoc(adata, "cond", control=cond[1], num_boot=B, fill_seed=FILL), TEST_COLS + ADJ_COLS)
    assert list(one["level_a"][:2]) == [groups[0], groups[2]] and (one["level_b"] == groups[1]).all()


def test_pairs_with_lost_groups(prepared, one_chunk):
    p, df = prepared, one_chunk
    num = TEST_COLS + ADJ_COLS[:1] + SCI_COLS
    one = _block(df, ONE)                                           # one group lost: its level still has the other replicate
    assert (one["n_family"] == 3).all() and np.isfinite(one[num].values.astype(float)).all()
    level = _block(df, LEVEL)                                       # level 2 lost: the family is the one contrast of levels 0 and 1
    with_2 = ((level["level_a"] == "2") | (level["level_b"] == "2")).values
    assert (level["n_family"] == 1).all() and with_2.sum() == 2
    assert np.isfinite(level[num].values[~with_2].astype(float)).all() and np.isnan(level[num].values[with_2].astype(float)).all()
    # a family of one: the adjusted p-value is the count-based one, at or above the reported raw one
    assert level["corr_pval_adj"].values[~with_2][0] >= level["corr_pval"].values[~with_2][0]
    for dead in (ALL, p.self_pair):                                 # the pair with no good group, the self pair
        lost = _block(df, dead)
        assert (lost["n_family"] == 0).all() and np.isnan(lost[num].values.astype(float)).all()
    dup, orig = _block(df, p.dup), _block(df, DUP_OF)               # the reversed duplicate: the first one's rows
    assert list(dup["gene_1"]) == list(orig["gene_2"]) and list(dup["gene_2"]) == list(orig["gene_1"])
    for c in num + ["n_family"]:
        np.testing.assert_array_equal(dup[c].values, orig[c].values, err_msg=c)
    assert np.isfinite(orig[num].values.astype(float)).all()
    others = np.setdiff1d(np.arange(p.n_base), [ONE, LEVEL, ALL])
    assert (df["n_family"].values.reshape(-1, N_MEM)[others, 0] == 3).mean() > 0.9


def test_planted_changes(prepared, one_chunk):
    """Every planted pair whose ``ht_2d_joint`` p-value on the same matrix is at the floor 1 / 301: the smaller corr_pval_adj of its
    two contrasts involving level 1 is <= 0.05.  (The contrast of levels 0 and 2 carries no planted change and is not asserted.)
    Observed: ht_2d_joint is at the floor on five of the six planted pairs (2 / 301 on the sixth); the smaller corr_pval_adj is
    1 / 301 = 0.0033 on those five and 0.0199 on the sixth; their contrasts of levels 0 and 2 have 0.12 .. 1.0.  Of the rows of the 51
    unplanted pairs 0.65 % are at or below 0.05 (median 0.784)."""
    p, df = prepared, one_chunk
    planted = np.arange(N_PLANTED)
    at_floor = planted[p.joint["corr_pval"].values[planted] == 1 / (B + 1)]
    q = df["corr_pval_adj"].values.reshape(-1, N_MEM)
    with_1 = np.array(["1" in pair for pair in p.level_pairs])
    assert with_1.sum() == 2
    smaller = np.nanmin(q[np.ix_(planted, np.flatnonzero(with_1))], axis=1)
    rest = np.setdiff1d(np.arange(p.n_base), np.r_[planted, ONE, LEVEL, ALL])
    print(f"\nplanted pairs: ht_2d_joint corr_pval {np.round(p.joint['corr_pval'].values[planted], 4)}; smaller corr_pval_adj of the two contrasts "
          f"with level 1 {np.round(smaller, 4)}; contrast of levels 0 and 2 {np.round(q[planted][:, ~with_1].reshape(-1), 4)}; "
          f"{len(rest)} unplanted pairs: share of rows <= 0.05 {np.nanmean(q[rest] <= 0.05):.4f}, median {np.nanmedian(q[rest]):.3f}")
    assert len(at_floor) >= 4                                       # the input: the reference test sees the planted changes
    assert (smaller[at_floor] <= 0.05).all()


def test_unknown_rng_raises(prepared):
    with pytest.raises(ValueError, match="rng must be"):
        _posthoc(prepared, rng="other")
