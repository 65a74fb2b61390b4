"""mm_joint_stats (the joint test of a treatment block) on synthetic replicate planes through ``engine.Bootstrap1D.joint``, against
the numpy restatement tests/_joint_ref.py, at the smallest sizes where the kernel changes path: fewer replicate columns than
threads, a ragged second stride, padded rows, one and two groups, a bad group that is not listed, the group counts either side of
the two register tiers (8 and 32 groups), the first design past the LDS
staging of L and the last one inside it, more forms than threads, dropped columns, a dropped column 0, several designs and an
empty one in one launch, and replicates that all equal the observed column.

Q_0, mean, sd and max agree to rtol 1e-11 (the bar of the statistics kernels against numpy), n_valid, r and the flag exactly,
and so does n_extreme: every case first asserts in numpy that no Q*_c lies within 1e-10 * Q_0 of Q_0, so the restatement alone
decides every count."""

from types import SimpleNamespace

import numpy as np
import pytest

import _joint_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


@pytest.fixture(scope="module")
def ht():
    from scrna_parameter_estimation_amd.memento import _ht

    return _ht


def _planes(eng, ym, yv, B, ng):
    """A Bootstrap1D that only holds replicate rows (what the statistics kernels read)."""
    bs = object.__new__(eng.Bootstrap1D)
    bs.ym, bs.yv, bs.ld, bs.B, bs.ng = eng.dev(ym), eng.dev(yv), ym.shape[1], B, ng
    bs.n_tested = bs.n_pairs = ym.shape[0] // ng
    return bs


def _one_way(levels, drop_first=True):
    lv = np.unique(levels)[1 if drop_first else 0:]
    return np.stack([(levels == v).astype(np.float64) for v in lv], axis=1)


def _random_planes(n_genes, ng, B, pad, seed):
    """Normal planes [n_genes * ng][B + 1 + pad]; the padding is poisoned (NaN and 1e300 alternating): it is never read."""
    rng = np.random.default_rng(seed)
    ld = B + 1 + pad
    ym = rng.normal(0, 1, size=(n_genes * ng, ld))
    yv = rng.normal(0, 1, size=(n_genes * ng, ld))
    for y in (ym, yv):
        y[:, B + 1::2] = np.nan
        y[:, B + 2::2] = 1e300
    return ym, yv


def _expected(tables, t, gene, ym, yv, B, ng):
    d = tables.test_design[t]
    grp = tables.design_grp[tables.design_ptr[d]:tables.design_ptr[d + 1]]
    r = int(tables.design_rank[d])
    L = tables.design_L[tables.design_lofs[d]:tables.design_lofs[d] + r * len(grp)].reshape(r, len(grp))
    rows = gene * ng + grp
    q0, qs, ok = ref.q_columns(L, ym[rows, :B + 1], yv[rows, :B + 1])
    for k in range(2):
        if r and len(grp) and not np.isnan(q0[k]):
            assert ref.near_ties(q0[k], qs[k], ok) == 0, f"test {t} plane {k}: a Q* within 1e-10 of Q_0, pick another seed"
    return ref.joint_records(L, ym[rows, :B + 1], yv[rows, :B + 1])


def _check(eng, ym, yv, B, ng, test_gene, tables):
    """Both records of every test against the restatement; returns them (mean [n_tests][8], var [n_tests][8])."""
    bs = _planes(eng, ym, yv, B, ng)
    st_m, st_v = bs.joint(test_gene, tables)
    assert st_m.shape == st_v.shape == (len(test_gene), 8)
    for t, gene in enumerate(test_gene):
        want = _expected(tables, t, gene, ym, yv, B, ng)
        for k, got in enumerate((st_m[t], st_v[t])):
            msg = f"test {t} plane {k}"
            np.testing.assert_allclose(got, want[k], rtol=1e-11, atol=0, equal_nan=True, err_msg=msg)
            np.testing.assert_array_equal(got[ref.COUNT_COLUMNS], want[k][ref.COUNT_COLUMNS], err_msg=msg)
    return st_m, st_v


def _seven_groups(ht, n_genes=1):
    """8 groups: a 4-level factor over 7 of them (r = 3) with a covariate, and group 5, which is bad: not listed."""
    ng = 8
    levels = np.array([0, 0, 1, 1, 2, 9, 2, 3])
    rng = np.random.default_rng(11)
    cov = rng.normal(0, 1, size=(ng, 1))
    Nc = rng.integers(200, 2000, size=ng).astype(np.float64)
    good = np.ones((n_genes, ng), dtype=bool)
    good[:, 5] = False
    tables = ht.joint_tables(good, cov, _one_way(levels), Nc)
    assert list(tables.design_rank) == [3] and list(np.diff(tables.design_ptr)) == [7]
    return ng, tables


@pytest.mark.parametrize("B, pad", [(5, 0), (300, 0), (300, 5), (256, 1), (257, 2)])
def test_seven_groups_rank_three_with_an_unlisted_bad_group(eng, ht, B, pad):
    ng, tables = _seven_groups(ht)
    ym, yv = _random_planes(1, ng, B, pad, seed=100 + B + pad)
    ym[5], yv[5] = np.nan, np.nan                                  # the bad group's rows: all NaN, never read
    st_m, st_v = _check(eng, ym, yv, B, ng, np.array([0]), tables)
    assert st_m[0, 2] == B and st_m[0, 7] == 3
    assert B == 5 or 0 < st_m[0, 3] < B                           # a count in the middle: the comparison matters


@pytest.mark.parametrize("ng", [9, 32, 33])
def test_group_counts_either_side_of_the_register_tiers(eng, ht, ng):
    """Up to 8 and up to 32 groups a thread keeps its column in registers; 9, 32 and 33 groups are the first and the last size of
    the wider tier and the first one past it (8 is ``_seven_groups``).  A 5-level factor with a covariate; gene 1 has three bad
    groups, the first and the last group among them; a dropped column in either plane."""
    B = 300
    rng = np.random.default_rng(ng)
    levels = np.arange(ng) % 5
    cov = rng.normal(0, 1, size=(ng, 1))
    Nc = rng.integers(200, 2000, size=ng).astype(np.float64)
    good = np.ones((2, ng), dtype=bool)
    good[1, [0, 2, ng - 1]] = False
    tables = ht.joint_tables(good, cov, _one_way(levels), Nc)
    assert list(tables.design_rank) == [4, 4] and list(np.diff(tables.design_ptr)) == [ng, ng - 3]
    ym, yv = _random_planes(2, ng, B, 1, seed=200 + ng)
    ym[ng - 1, 33] = np.nan
    yv[ng + 1, 299] = np.inf
    ym[ng + ng - 1] = np.nan                                        # a bad group
    st_m, st_v = _check(eng, ym, yv, B, ng, np.array([0, 1]), tables)
    assert list(st_m[:, 2]) == [B - 1, B - 1] and list(st_v[:, 7]) == [4, 4]


def test_one_group_and_two_groups(eng, ht):
    """n_d = 1: nothing to test (r = 0, the NaN record); n_d = 2: r = 1, the two-group difference."""
    ng, B = 3, 300
    levels = np.array([0, 1, 2])
    Nc = np.array([300.0, 900.0, 500.0])
    good = np.array([[True, False, False], [True, False, True], [True, True, True]])
    tables = ht.joint_tables(good, np.ones((ng, 0)), _one_way(levels), Nc)
    assert list(tables.design_rank) == [0, 1, 2]
    ym, yv = _random_planes(3, ng, B, 1, seed=21)
    st_m, st_v = _check(eng, ym, yv, B, ng, np.arange(3), tables)
    np.testing.assert_array_equal(st_m[0], ref.NAN_RECORD)
    np.testing.assert_array_equal(st_v[0], ref.NAN_RECORD)
    # two groups: Q = w_a w_c (y_a - y_c)^2 with w the cell-count shares
    w = Nc[[0, 2]] / Nc[[0, 2]].sum()
    np.testing.assert_allclose(st_m[1, 0], w[0] * w[1] * (ym[3, 0] - ym[5, 0]) ** 2, rtol=1e-11)
    assert np.isnan(ref.pvalues(st_m)[0]) and 0 < ref.pvalues(st_m)[1] <= 1


@pytest.mark.parametrize("n_grp, staged", [(64, True), (65, False)])
def test_either_side_of_the_lds_staging(eng, ht, n_grp, staged):
    """65 groups one-way: r = 64, 4,160 doubles of L, the smallest such design past the 4,096 that are staged; the same design cut
    to 64 groups (r = 63, 4,032 doubles) is staged.  Both against the restatement, with a column dropped through the variability
    plane."""
    ng, B = 65, 300
    rng = np.random.default_rng(31)
    Nc = rng.integers(200, 2000, size=ng).astype(np.float64)
    good = np.ones((1, ng), dtype=bool)
    good[0, n_grp:] = False
    tables = ht.joint_tables(good, np.ones((ng, 0)), _one_way(np.arange(ng)), Nc)
    assert list(tables.design_rank) == [n_grp - 1]
    assert ((n_grp - 1) * n_grp <= 4096) == staged
    ym, yv = _random_planes(1, ng, B, 3, seed=32)
    yv[7, 7] = np.nan
    st_m, st_v = _check(eng, ym, yv, B, ng, np.array([0]), tables)
    assert st_m[0, 2] == B - 1 and st_v[0, 2] == B - 1


def test_staged_and_cached_paths_give_identical_numbers(eng, ht):
    """A design of 4,096 doubles of L (staged) and the same forms with an all-zero 65th group column appended (4,160 doubles:
    read through the cache) on planes whose extra group is finite: the arithmetic differs by adding exact zeros only, so the two
    records are the same bits."""
    B, r, nd = 300, 64, 64
    rng = np.random.default_rng(41)
    L = rng.normal(0, 0.3, size=(r, nd))
    ng = nd + 1
    ym, yv = _random_planes(1, ng, B, 0, seed=42)
    def tab(Lmat):
        n = Lmat.shape[1]
        return SimpleNamespace(test_design=np.zeros(1, np.int32), design_ptr=np.array([0, n], np.int32), design_rank=np.array([r], np.int32),
                               design_lofs=np.zeros(1, np.int64), design_grp=np.arange(n, dtype=np.int32), design_L=Lmat.reshape(-1))
    small, big = tab(L), tab(np.concatenate([L, np.zeros((r, 1))], axis=1))
    assert small.design_L.size == 4096 and big.design_L.size == 4160
    a_m, a_v = _check(eng, ym, yv, B, ng, np.array([0]), small)
    b_m, b_v = _check(eng, ym, yv, B, ng, np.array([0]), big)
    np.testing.assert_array_equal(a_m.view(np.int64), b_m.view(np.int64))
    np.testing.assert_array_equal(a_v.view(np.int64), b_v.view(np.int64))


def test_more_forms_than_threads(eng, ht):
    """260 groups one-way with B = 40: r = 259 forms, more than the 256 threads that form z_0."""
    ng, B = 260, 40
    rng = np.random.default_rng(51)
    Nc = rng.integers(200, 2000, size=ng).astype(np.float64)
    tables = ht.joint_tables(np.ones((1, ng), dtype=bool), np.ones((ng, 0)), _one_way(np.arange(ng)), Nc)
    assert list(tables.design_rank) == [259]
    ym, yv = _random_planes(1, ng, B, 2, seed=52)
    st_m, _ = _check(eng, ym, yv, B, ng, np.array([0]), tables)
    assert st_m[0, 7] == 259 and st_m[0, 2] == B


def test_dropped_columns_and_a_dropped_column_zero(eng, ht):
    """A NaN at column 7 of one group in the variability plane only drops the column on BOTH planes; an inf in the mean plane
    likewise; a NaN in column 0 gives the NaN record on both planes; non-finite values in the unlisted bad group change nothing."""
    B = 300
    ng, tables = _seven_groups(ht, n_genes=3)
    ym, yv = _random_planes(3, ng, B, 4, seed=61)
    clean_m, clean_v = ym.copy(), yv.copy()
    yv[0 * ng + 2, 7] = np.nan
    ym[0 * ng + 6, 299] = np.inf
    ym[0 * ng + 0, 300] = -np.inf                                  # the last replicate column
    ym[0 * ng + 5, :] = np.nan                                     # the bad group
    yv[1 * ng + 3, 0] = np.nan                                     # gene 1: column 0, in the variability plane only
    st_m, st_v = _check(eng, ym, yv, B, ng, np.arange(3), tables)
    assert st_m[0, 2] == B - 3 and st_v[0, 2] == B - 3
    np.testing.assert_array_equal(st_m[1], ref.NAN_RECORD)
    np.testing.assert_array_equal(st_v[1], ref.NAN_RECORD)
    ref_m, ref_v = _check(eng, clean_m, clean_v, B, ng, np.arange(3), tables)
    assert ref_m[0, 2] == B and (ref_m[0, [1, 4]] != st_m[0, [1, 4]]).all()          # the dropped columns did count before
    np.testing.assert_array_equal(ref_m[2], st_m[2])
    np.testing.assert_array_equal(ref_v[2], st_v[2])


def test_several_designs_and_an_empty_one_in_one_launch(eng, ht):
    """Three genes with different good masks: a 5-level factor with a covariate on 10 groups, no good group at all (the empty
    design), and 7 good groups; the tests are issued out of gene order and one gene twice."""
    ng, B = 10, 300
    levels = np.repeat(np.arange(5), 2)
    rng = np.random.default_rng(71)
    cov = rng.normal(0, 1, size=(ng, 2))
    Nc = rng.integers(200, 2000, size=ng).astype(np.float64)
    good = np.ones((3, ng), dtype=bool)
    good[1] = False
    good[2, [0, 1, 9]] = False                                     # level 0 is gone: r = 3
    tables = ht.joint_tables(good, cov, _one_way(levels), Nc)
    assert list(tables.design_rank) == [4, 0, 3] and list(np.diff(tables.design_ptr)) == [10, 0, 7]
    ym, yv = _random_planes(3, ng, B, 0, seed=72)
    ym[2 * ng + 9], yv[1 * ng:2 * ng] = np.nan, np.nan
    test_gene = np.array([2, 0, 1, 2])
    t4 = SimpleNamespace(**{**tables.__dict__, "test_design": tables.test_design[test_gene]})
    st_m, st_v = _check(eng, ym, yv, B, ng, test_gene, t4)
    np.testing.assert_array_equal(st_m[2], ref.NAN_RECORD)
    np.testing.assert_array_equal(st_m[0], st_m[3])
    assert list(st_m[:, 7][[0, 1, 3]]) == [3, 4, 3]
    st0_m, st0_v = _planes(eng, ym, yv, B, ng).joint(np.zeros(0, np.int64), SimpleNamespace(**{**tables.__dict__, "test_design": np.zeros(0, np.int32)}))
    assert st0_m.shape == (0, 8) and st0_v.shape == (0, 8)         # no tests: a no-op


def test_replicates_equal_to_the_observed_column(eng, ht):
    """Every replicate column equals column 0: every Q* is exactly 0 (column 0 goes through the same arithmetic), all_equal = 1,
    nothing is extreme and the p-value is NaN."""
    from scrna_parameter_estimation_amd.memento.main import joint_pvalues

    B = 300
    ng, tables = _seven_groups(ht)
    ym, yv = _random_planes(1, ng, B, 2, seed=81)
    ym[:, 1:B + 1] = ym[:, :1]
    yv[:, 1:B + 1] = yv[:, :1]
    st_m, st_v = _check(eng, ym, yv, B, ng, np.array([0]), tables)
    for st in (st_m, st_v):
        np.testing.assert_array_equal(st[0, 1:7], [0.0, B, 0.0, 0.0, 1.0, 0.0])
        assert st[0, 0] > 0 and np.isnan(joint_pvalues(st)[0]) and np.isnan(joint_pvalues(st, approx=True)[0])


def test_the_tables_are_checked_on_the_host(eng, ht):
    ng, tables = _seven_groups(ht)
    ym, yv = _random_planes(1, ng, 5, 0, seed=91)
    bs = _planes(eng, ym, yv, 5, ng)
    def broken(**kw):
        return SimpleNamespace(**{**tables.__dict__, **kw})
    for bad in (broken(design_rank=np.array([8])), broken(design_grp=np.arange(2, 9)), broken(design_lofs=np.array([1])),
                broken(test_design=np.array([1])), broken(design_ptr=np.array([0, 6])), broken(design_rank=np.array([-1]))):
        with pytest.raises(ValueError, match="joint:"):
            bs.joint(np.array([0]), bad)
    with pytest.raises(ValueError, match="joint:"):
        bs.joint(np.array([1]), tables)
