"""CPU tests of the sequential bootstrap's pure parts (memento/_ht.py): the fold of per-round test records, the round schedule,
the stopping rule, the refill seed of a round, the argument checks of ``ht_1d_vs_control(max_boot=...)`` and the C-ABI
declaration of the replicate-range launch."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(coef0, cols):
    """THE TEST RECORD (csrc/contract.hip) of one coefficient row in plain numpy: ``cols`` are the replicate columns, NaN = dropped."""
    v = cols[~np.isnan(cols)]
    n = len(v)
    a0 = abs(coef0)
    allv = np.concatenate([[coef0], v])
    return np.array([coef0, v.std() if n else np.nan, n, (np.abs(v - coef0) > a0).sum(), v.mean() - coef0 if n else np.nan,
                     float(allv.min() == allv.max()), (np.abs(v) > a0).sum(), allv.max() - allv.min()])


def _cut(n_cols, n_rounds, rng):
    """``n_rounds`` unequal consecutive column ranges of [0, n_cols)."""
    cuts = np.sort(rng.choice(np.arange(1, n_cols), size=n_rounds - 1, replace=False)) if n_rounds > 1 else np.zeros(0, dtype=np.int64)
    b = np.concatenate([[0], cuts, [n_cols]]).astype(int)
    return list(zip(b[:-1], b[1:]))


@pytest.mark.parametrize("n_rounds", [1, 2, 3, 4, 5])
def test_merge_records_is_the_record_of_the_concatenation(n_rounds):
    """Random coefficient rows cut into 1..5 unequal rounds, with dropped (NaN) columns, one round of every row's second half
    without a valid column, and an all-equal row: counts exactly equal, se and mean within 1e-12 relative (fp64 summation order)."""
    from scrna_parameter_estimation_amd.memento._ht import merge_records

    rng = np.random.default_rng(100 + n_rounds)
    n_tests, n_cols = 40, 317
    coef0 = rng.normal(0.0, 1.0, size=n_tests)
    rows = coef0[:, None] + rng.normal(0.3, 1.0, size=(n_tests, n_cols))
    rows[rng.random(rows.shape) < 0.07] = np.nan
    rows[7] = coef0[7]                                      # all equal, column 0 included
    rows[8, ::3] = np.nan
    rows[8, ~np.isnan(rows[8])] = coef0[8]                  # all equal with dropped columns
    rounds = _cut(n_cols, n_rounds, rng)
    empty_round = min(1, n_rounds - 1)
    lo, hi = rounds[empty_round]
    if n_rounds > 1:
        rows[20:, lo:hi] = np.nan                           # a round without a valid column (n_j = 0)
    per_round = [np.stack([_record(coef0[t], rows[t, a:b]) for t in range(n_tests)]) for a, b in rounds]
    if n_rounds > 1:
        assert (per_round[empty_round][20:, 2] == 0).all() and np.isnan(per_round[empty_round][20:, 1]).all()
    want = np.stack([_record(coef0[t], rows[t]) for t in range(n_tests)])
    got = merge_records(per_round)
    assert got.shape == (n_tests, 8)
    np.testing.assert_array_equal(got[:, 0], want[:, 0])
    for k in (2, 3, 6):
        np.testing.assert_array_equal(got[:, k], want[:, k])
    np.testing.assert_array_equal(got[:, 5], want[:, 5])
    assert got[7, 5] == 1 and got[8, 5] == 1 and got[:, 5].sum() == 2
    live = want[:, 5] == 0
    np.testing.assert_allclose(got[live, 1], want[live, 1], rtol=1e-12, atol=0)
    # the all-equal rows: the true se is 0, and a computed mean of n equal numbers x is off by at most n 2^-53 |x| on either side
    np.testing.assert_allclose(got[~live, 1], 0.0, rtol=0, atol=n_cols * 2.0 ** -53 * np.abs(coef0[~live]).max())
    np.testing.assert_allclose(want[~live, 1], 0.0, rtol=0, atol=n_cols * 2.0 ** -53 * np.abs(coef0[~live]).max())
    np.testing.assert_allclose(got[:, 4] + coef0, want[:, 4] + coef0, rtol=1e-12, atol=0)
    if n_rounds > 1:
        assert np.isnan(got[:, 7]).all()                    # range is not mergeable
    else:
        np.testing.assert_array_equal(got, per_round[0])    # one round: the record itself
    assert got is not per_round[0]


def test_merge_records_of_rounds_without_any_valid_column():
    from scrna_parameter_estimation_amd.memento._ht import merge_records

    nan_rec = np.array([[0.5, np.nan, 0, 0, np.nan, 1, 0, 0.0]])
    got = merge_records([nan_rec, nan_rec])
    assert got[0, 0] == 0.5 and got[0, 2] == 0 and got[0, 3] == 0 and np.isnan(got[0, 1]) and np.isnan(got[0, 4]) and got[0, 5] == 1
    one = np.array([[0.5, 0.25, 10, 3, 0.1, 0, 2, 1.0]])
    got = merge_records([one, nan_rec])                      # the empty round contributes nothing, not even its all_equal flag
    np.testing.assert_array_equal(got[0, :7], one[0, :7])


def test_sequential_schedule():
    from scrna_parameter_estimation_amd.memento._ht import sequential_schedule

    assert sequential_schedule(1000, 1000) == [1000]
    assert sequential_schedule(200, 3200) == [200, 400, 800, 1600, 3200]
    assert sequential_schedule(300, 1000) == [300, 600, 1000]                # non-power-of-two ratio: a short last round
    assert sequential_schedule(1000, 1_000_000) == [1000 * 2 ** k for k in range(10)] + [1_000_000]
    assert sequential_schedule(1, 3) == [1, 2, 3]
    with pytest.raises(ValueError):
        sequential_schedule(10, 9)
    with pytest.raises(ValueError):
        sequential_schedule(0, 9)


def test_open_tests():
    from scrna_parameter_estimation_amd.memento._ht import open_tests, sequential_pvalues

    #                 coef0   se    n    c   mean  alleq raw range
    recs = np.array([[0.5,    0.1,  200, 10, 0.0,  0,    50, 1.0],          # c == min_extreme: open
                     [0.5,    0.1,  200, 11, 0.0,  0,    5,  1.0],          # c == min_extreme + 1: closed
                     [np.nan, 0.1,  200, 0,  0.0,  0,    0,  1.0],          # no coefficient
                     [0.5,    np.nan, 0, 0,  np.nan, 0,  0,  np.nan],       # no valid replicate
                     [0.5,    0.0,  200, 0,  0.0,  1,    0,  0.0],          # all equal
                     [np.inf, 0.1,  200, 0,  0.0,  0,    0,  1.0],
                     [0.5,    0.1,  200, 0,  0.0,  0,    0,  1.0]])
    np.testing.assert_array_equal(open_tests(recs, 10, 'bootstrap'), [True, False, False, False, False, False, True])
    np.testing.assert_array_equal(open_tests(recs), open_tests(recs, 10, 'bootstrap'))
    np.testing.assert_array_equal(open_tests(recs, 10, 'permutation'), [False, True, False, False, False, False, True])
    np.testing.assert_array_equal(open_tests(recs, 0, 'bootstrap'), [False, False, False, False, False, False, True])
    p = sequential_pvalues(recs, 'bootstrap')
    np.testing.assert_array_equal(p[[0, 1, 6]], [11 / 201, 12 / 201, 1 / 201])
    assert np.isnan(p[[2, 3, 4, 5]]).all()
    np.testing.assert_array_equal(sequential_pvalues(recs, 'permutation')[[0, 1]], [51 / 201, 6 / 201])


def test_round_fill_seed():
    from scrna_parameter_estimation_amd.memento._ht import _mix64, round_fill_seed

    assert _mix64(0) == 0xE220A8397B1DCDAF                     # splitmix64's first output from state 0
    assert round_fill_seed(5, 0) == 5 and round_fill_seed(-1, 0) == 2 ** 64 - 1
    seeds = {round_fill_seed(s, j) for s in range(4) for j in range(1, 12)}
    assert len(seeds) == 44 and all(0 <= x < 2 ** 64 for x in seeds)


@pytest.mark.parametrize("kw", [dict(rng='replay'), dict(approx=True), dict(ci=0.95), dict(max_boot=199), dict(min_extreme=-1),
                                dict(max_boot=400.0), dict(min_extreme=2.5), dict(max_boot=True), dict(max_boot=2 ** 31)])
def test_argument_errors_come_before_adata_is_touched(kw):
    """``adata`` is an object without a single attribute: the ValueError must come first."""
    from scrna_parameter_estimation_amd import memento

    args = dict(num_boot=200, rng='fast', max_boot=3200)
    args.update(kw)
    with pytest.raises(ValueError):
        memento.ht_1d_vs_control(object(), 0, **args)


def test_without_max_boot_the_checks_let_everything_through():
    from scrna_parameter_estimation_amd import memento
    from scrna_parameter_estimation_amd.memento._ht import check_sequential

    assert check_sequential(None, -5, 10, 'replay', True, 0.9) is False
    assert check_sequential(400, 0, 200, 'fast', False, None) is True
    assert check_sequential(np.int64(200), np.int32(10), 200, 'fast', False, None) is True
    sig = inspect.signature(memento.ht_1d_vs_control).parameters
    assert sig['max_boot'].default is None and sig['min_extreme'].default == 10
    assert sig['max_boot'].kind is sig['min_extreme'].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (memento.ht_1d_moments, memento.ht_2d_vs_control, memento.ht_1d_joint, memento.ht_1d_posthoc):
        assert 'max_boot' not in inspect.signature(fn).parameters


def test_cabi_declares_and_binds_the_range_launch():
    from scrna_parameter_estimation_amd import _lib, build
    from scrna_parameter_estimation_amd.engine import Bootstrap1D

    hdr = open(os.path.join(ROOT, "include", "memento_hip.h")).read()
    decl = re.search(r"\bint mm_boot1d_fast_range\s*\(([^;]*)\);", hdr)
    assert decl and "mm_boot1d_fast_range" in _lib.EXPORTS
    params = [a.strip() for a in decl.group(1).split(",")]
    one_shot = [a.strip() for a in re.search(r"\bint mm_boot1d_fast\s*\(([^;]*)\);", hdr).group(1).split(",")]
    assert params == one_shot[:13] + ["int32_t rep_lo", "int32_t rep_n"] + one_shot[14:]      # num_boot -> rep_lo, rep_n
    args, res = _lib._SIGS["mm_boot1d_fast_range"]
    ref = _lib._SIGS["mm_boot1d_fast"][0]
    assert args == ref[:13] + [ctypes.c_int32, ctypes.c_int32] + ref[14:] and res is ctypes.c_int
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mm_boot1d_fast_range")
    src = open(os.path.join(ROOT, "scrna_parameter_estimation_amd", "csrc", "boot.hip")).read()
    assert src.count("void k_boot1d_fast(") == 1 and src.count("hipLaunchKernelGGL(k_boot1d_fast,") == 1     # one kernel, one launch
    assert {"launch_range", "run_range"} <= set(vars(Bootstrap1D))
