"""mm_joint1_stats (the joint test of a treatment block on ONE response plane) on synthetic planes through
``engine.Bootstrap2D.joint``, against the numpy restatement tests/_joint_ref.py (``joint_records(L, y, y)[0]``) and, bit for bit,
against the mean record of ``Bootstrap1D.joint`` (mm_joint_stats) given the plane twice.  The sizes are the smallest where the
kernel changes path: fewer replicate columns than threads, a ragged second stride, padded rows, one and two groups, a bad group
that is not listed, the group counts either side of the two register tiers (8 and 32 groups), the last design inside the LDS
staging of L and the first one past it, more forms than threads, dropped columns, a dropped column 0, several designs and an empty
one in one launch, and replicates that all equal the observed column.

Q_0, mean, sd and max agree with the restatement to rtol 1e-11, n_valid, r and the flag exactly, and so does n_extreme: every case
first asserts in numpy that no Q*_c lies within 1e-10 * Q_0 of Q_0, so the restatement alone decides every count."""

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


def _plane2d(eng, y, B, ng):
    """What ``Bootstrap2D.joint`` reads: yc, ld, B, ng, n_pairs."""
    return SimpleNamespace(yc=eng.dev(y), ld=y.shape[1], B=B, ng=ng, n_pairs=y.shape[0] // ng)


def _planes1d(eng, y, B, ng):
    """What ``Bootstrap1D.joint`` reads, with the one plane as both of its planes."""
    d = eng.dev(y)
    return SimpleNamespace(ym=d, yv=d, ld=y.shape[1], B=B, ng=ng, n_tested=y.shape[0] // ng)


def _one_way(levels, drop_first=True):
    lv = np.unique(levels)[1 if drop_first else 0:]
    return np.stack([(levels == v).astype(np.float64) for v in lv], axis=1)


def _random_plane(n_pairs, ng, B, pad, seed):
    """A correlation-like plane [n_pairs * ng][B + 1 + pad]; the padding is poisoned (NaN and 1e300 alternating): it is never read."""
    rng = np.random.default_rng(seed)
    y = np.tanh(rng.normal(0, 0.6, size=(n_pairs * ng, B + 1 + pad)))
    y[:, B + 1::2] = np.nan
    y[:, B + 2::2] = 1e300
    return y


def _expected(tables, t, pair, y, B, ng):
    d = tables.test_design[t]
    grp = tables.design_grp[tables.design_ptr[d]:tables.design_ptr[d + 1]]
    r = int(tables.design_rank[d])
    L = tables.design_L[tables.design_lofs[d]:tables.design_lofs[d] + r * len(grp)].reshape(r, len(grp))
    rows = pair * ng + grp
    q0, qs, ok = ref.q_columns(L, y[rows, :B + 1], y[rows, :B + 1])
    if r and len(grp) and not np.isnan(q0[0]):
        assert ref.near_ties(q0[0], qs[0], ok) == 0, f"test {t}: a Q* within 1e-10 of Q_0, pick another seed"
    return ref.joint_records(L, y[rows, :B + 1], y[rows, :B + 1])[0]


def _check(eng, y, B, ng, test_pair, tables):
    """The record of every test against the restatement and, bit for bit, against the two-plane kernel; returns it [n_tests][8]."""
    st = eng.Bootstrap2D.joint(_plane2d(eng, y, B, ng), test_pair, tables)
    assert st.shape == (len(test_pair), 8)
    for t, pair in enumerate(test_pair):
        want = _expected(tables, t, pair, y, B, ng)
        np.testing.assert_allclose(st[t], want, rtol=1e-11, atol=0, equal_nan=True, err_msg=f"test {t}")
        np.testing.assert_array_equal(st[t][ref.COUNT_COLUMNS], want[ref.COUNT_COLUMNS], err_msg=f"test {t}")
    st_m, st_v = eng.Bootstrap1D.joint(_planes1d(eng, y, B, ng), test_pair, tables)
    np.testing.assert_array_equal(st, st_m)                         # NaNs in the same places, the same bits elsewhere
    np.testing.assert_array_equal(st, st_v)
    return st


def _seven_groups(ht, n_pairs=1):
    """8 groups: a 4-level factor over 7 of them (r = 3) with a covariate, and group 5, which is bad: not listed."""
    ng = 8
    levels = np.array([0, 0, 1, 1, 2, 9, 2, 3])
    rng = np.random.default_rng(11)
    cov = rng.normal(0, 1, size=(ng, 1))
    Nc = rng.integers(200, 2000, size=ng).astype(np.float64)
    good = np.ones((n_pairs, ng), dtype=bool)
    good[:, 5] = False
    tables = ht.joint_tables(good, cov, _one_way(levels), Nc)
    assert list(tables.design_rank) == [3] and list(np.diff(tables.design_ptr)) == [7]
    return ng, tables


@pytest.mark.parametrize("B, pad", [(5, 0), (300, 0), (256, 1), (257, 2)])
def test_seven_groups_rank_three_with_an_unlisted_bad_group(eng, ht, B, pad):
    ng, tables = _seven_groups(ht)
    y = _random_plane(1, ng, B, pad, seed=100 + B + pad)
    y[5] = np.nan                                                  # the bad group's row: all NaN, never read
    st = _check(eng, y, B, ng, np.array([0]), tables)
    assert st[0, 2] == B and st[0, 7] == 3
    assert B == 5 or 0 < st[0, 3] < B                              # a count in the middle: the comparison matters


@pytest.mark.parametrize("ng", [8, 9, 32, 33])
def test_group_counts_either_side_of_the_register_tiers(eng, ht, ng):
    """Up to 8 and up to 32 groups a thread keeps its column in registers: 8 | 9 and 32 | 33 groups are the last size of a tier
    and the first one past it.  A 5-level factor with a covariate; pair 1 has three bad groups, the first and the last group
    among them; a dropped column in either pair."""
    B = 300
    rng = np.random.default_rng(ng)
    levels = np.arange(ng) % 5
    cov = rng.normal(0, 1, size=(ng, 1))
    Nc = rng.integers(200, 2000, size=ng).astype(np.float64)
    good = np.ones((2, ng), dtype=bool)
    good[1, [0, 2, ng - 1]] = False
    tables = ht.joint_tables(good, cov, _one_way(levels), Nc)
    assert list(tables.design_rank) == [4, 4 if ng > 8 else 3] and list(np.diff(tables.design_ptr)) == [ng, ng - 3]
    y = _random_plane(2, ng, B, 1, seed=200 + ng)
    y[ng - 1, 33] = np.nan
    y[ng + 1, 299] = np.inf
    y[ng + ng - 1] = np.nan                                         # a bad group
    st = _check(eng, y, B, ng, np.array([0, 1]), tables)
    assert list(st[:, 2]) == [B - 1, B - 1] and list(st[:, 7]) == list(tables.design_rank)


def test_one_group_and_two_groups(eng, ht):
    """n_d = 1: nothing to test (r = 0, the NaN record); n_d = 2: r = 1, the two-group difference."""
    ng, B = 3, 300
    levels = np.array([0, 1, 2])
    Nc = np.array([300.0, 900.0, 500.0])
    good = np.array([[True, False, False], [True, False, True], [True, True, True]])
    tables = ht.joint_tables(good, np.ones((ng, 0)), _one_way(levels), Nc)
    assert list(tables.design_rank) == [0, 1, 2]
    y = _random_plane(3, ng, B, 1, seed=21)
    st = _check(eng, y, B, ng, np.arange(3), tables)
    np.testing.assert_array_equal(st[0], ref.NAN_RECORD)
    # two groups: Q = w_a w_c (y_a - y_c)^2 with w the cell-count shares
    w = Nc[[0, 2]] / Nc[[0, 2]].sum()
    np.testing.assert_allclose(st[1, 0], w[0] * w[1] * (y[3, 0] - y[5, 0]) ** 2, rtol=1e-11)
    assert np.isnan(ref.pvalues(st)[0]) and 0 < ref.pvalues(st)[1] <= 1


def _explicit(L, r):
    n = L.shape[1]
    return SimpleNamespace(test_design=np.zeros(1, np.int32), design_ptr=np.array([0, n], np.int32), design_rank=np.array([r], np.int32),
                           design_lofs=np.zeros(1, np.int64), design_grp=np.arange(n, dtype=np.int32), design_L=L.reshape(-1))


@pytest.mark.parametrize("n_grp, staged", [(64, True), (65, False)])
def test_full_rank_either_side_of_the_lds_staging(eng, ht, n_grp, staged):
    """64 listed groups at full rank: r * n_d = 4,096 doubles of L, the last design that is staged in LDS; 65 x 65 = 4,225 is just
    past it and read through the cache.  With a dropped column."""
    B = 300
    rng = np.random.default_rng(31 + n_grp)
    tables = _explicit(rng.normal(0, 0.3, size=(n_grp, n_grp)), n_grp)
    assert (tables.design_L.size <= 4096) == staged
    y = _random_plane(1, n_grp, B, 3, seed=32)
    y[7, 7] = np.nan
    st = _check(eng, y, B, n_grp, np.array([0]), tables)
    assert st[0, 2] == B - 1 and st[0, 7] == n_grp


def test_staged_and_cached_paths_give_identical_numbers(eng, ht):
    """The entry point has no knob for the stage, so one design goes through both paths as in the two-plane test: 4,096 doubles of
    L (staged) and the same forms with an all-zero 65th group column appended (4,160 doubles: read through the cache) on a plane
    whose extra group is finite.  The arithmetic differs by adding exact zeros only, so the two records are the same bits."""
    B, r, nd = 300, 64, 64
    rng = np.random.default_rng(41)
    L = rng.normal(0, 0.3, size=(r, nd))
    ng = nd + 1
    y = _random_plane(1, ng, B, 0, seed=42)
    small, big = _explicit(L, r), _explicit(np.concatenate([L, np.zeros((r, 1))], axis=1), r)
    assert small.design_L.size == 4096 and big.design_L.size == 4160
    a = _check(eng, y, B, ng, np.array([0]), small)
    b = _check(eng, y, B, ng, np.array([0]), big)
    np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))


def test_more_forms_than_threads(eng, ht):
    """260 groups one-way with B = 40: r = 259 forms, more than the 256 threads that form z_0."""
    ng, B = 260, 40
    rng = np.random.default_rng(51)
    Nc = rng.integers(200, 2000, size=ng).astype(np.float64)
    tables = ht.joint_tables(np.ones((1, ng), dtype=bool), np.ones((ng, 0)), _one_way(np.arange(ng)), Nc)
    assert list(tables.design_rank) == [259]
    y = _random_plane(1, ng, B, 2, seed=52)
    st = _check(eng, y, B, ng, np.array([0]), tables)
    assert st[0, 7] == 259 and st[0, 2] == B


def test_dropped_columns_and_a_dropped_column_zero(eng, ht):
    """NaN and +-inf planted in replicate columns of listed groups drop those columns: n_valid falls and the record is that of the
    remaining ones; a NaN in column 0 gives the NaN record; non-finite values in the unlisted bad group change nothing."""
    B = 300
    ng, tables = _seven_groups(ht, n_pairs=3)
    y = _random_plane(3, ng, B, 4, seed=61)
    clean = y.copy()
    y[0 * ng + 2, 7] = np.nan
    y[0 * ng + 6, 299] = np.inf
    y[0 * ng + 0, 300] = -np.inf                                   # the last replicate column
    y[0 * ng + 5, :] = np.nan                                      # the bad group
    y[1 * ng + 3, 0] = np.nan                                      # pair 1: column 0
    st = _check(eng, y, B, ng, np.arange(3), tables)
    assert st[0, 2] == B - 3
    np.testing.assert_array_equal(st[1], ref.NAN_RECORD)
    before = _check(eng, clean, B, ng, np.arange(3), tables)
    assert before[0, 2] == B and (before[0, [1, 4]] != st[0, [1, 4]]).all()            # the dropped columns did count before
    assert before[0, 0] == st[0, 0]                                 # Q_0 does not see them
    np.testing.assert_array_equal(before[2], st[2])


def test_several_designs_and_an_empty_one_in_one_launch(eng, ht):
    """Three pairs with different good masks: a 5-level factor with a covariate on 10 groups, no good group at all (the empty
    design), and 7 good groups; the tests are issued out of pair order and one pair twice.  Then r = 0 on listed groups (a
    treatment inside the span of the covariates), and no test at all."""
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
    y = _random_plane(3, ng, B, 0, seed=72)
    y[2 * ng + 9], y[1 * ng:2 * ng] = np.nan, np.nan
    test_pair = np.array([2, 0, 1, 2])
    t4 = SimpleNamespace(**{**tables.__dict__, "test_design": tables.test_design[test_pair]})
    st = _check(eng, y, B, ng, test_pair, t4)
    np.testing.assert_array_equal(st[2], ref.NAN_RECORD)
    np.testing.assert_array_equal(st[0], st[3])
    assert list(st[:, 7][[0, 1, 3]]) == [3, 4, 3]
    flat = ht.joint_tables(good[:1], cov, cov[:, :1] * 2 - 1, Nc)   # r = 0 over 10 listed groups
    assert list(flat.design_rank) == [0] and list(np.diff(flat.design_ptr)) == [10]
    np.testing.assert_array_equal(_check(eng, y, B, ng, np.array([0]), flat)[0], ref.NAN_RECORD)
    none = SimpleNamespace(**{**tables.__dict__, "test_design": np.zeros(0, np.int32)})
    st0 = eng.Bootstrap2D.joint(_plane2d(eng, y, B, ng), np.zeros(0, np.int64), none)
    assert st0.shape == (0, 8)                                     # no tests: a no-op


def test_replicates_equal_to_the_observed_column(eng, ht):
    """Every replicate column equals column 0: every Q* is exactly 0 (column 0 goes through the same arithmetic), all_equal = 1,
    nothing is extreme and the p-value is NaN."""
    from scrna_parameter_estimation_amd.memento.main import joint_pvalues

    B = 300
    ng, tables = _seven_groups(ht)
    y = _random_plane(1, ng, B, 2, seed=81)
    y[:, 1:B + 1] = y[:, :1]
    st = _check(eng, y, B, ng, np.array([0]), tables)
    np.testing.assert_array_equal(st[0, 1:7], [0.0, B, 0.0, 0.0, 1.0, 0.0])
    assert st[0, 0] > 0 and np.isnan(joint_pvalues(st)[0]) and np.isnan(joint_pvalues(st, approx=True)[0])


def test_the_tables_are_checked_on_the_host(eng, ht):
    ng, tables = _seven_groups(ht)
    bs = _plane2d(eng, _random_plane(1, ng, 5, 0, seed=91), 5, ng)
    def broken(**kw):
        return SimpleNamespace(**{**tables.__dict__, **kw})
    for bad in (broken(design_rank=np.array([8])), broken(design_grp=np.arange(2, 9)), broken(design_lofs=np.array([1])),
                broken(test_design=np.array([1])), broken(design_ptr=np.array([0, 6])), broken(design_rank=np.array([-1]))):
        with pytest.raises(ValueError, match="joint:"):
            eng.Bootstrap2D.joint(bs, np.array([0]), bad)
    with pytest.raises(ValueError, match="joint:"):
        eng.Bootstrap2D.joint(bs, np.array([1]), tables)            # a pair the plane does not have
