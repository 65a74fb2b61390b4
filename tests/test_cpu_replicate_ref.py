"""The numpy restatements of tests/_replicate_ref.py checked on their own (no GPU): the mixer against the published
splitmix64 vector, and the refill rule's own properties, so that a kernel test that compares with them compares with the rule."""

import numpy as np
import pytest
import scipy.stats

from _replicate_ref import cross_draws, draws_chi2, fill_picks, mix64


def test_mixer_is_splitmix64():
    # splitmix64.c (Vigna), seed 0: the first three outputs.  The generator adds the golden-ratio increment to its state and
    # mixes it; mix64 folds that addition in, so output k is mix64((k - 1) * increment).
    inc = 0x9E3779B97F4A7C15
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    got = [int(mix64((k * inc) & (2**64 - 1))[0]) for k in range(3)]
    assert got == want
    np.testing.assert_array_equal(mix64(np.array([0, inc], dtype=np.uint64)), np.array(want[:2], dtype=np.uint64))
    assert int(mix64(-1)[0]) == int(mix64(2**64 - 1)[0])                      # signed keys are taken as their two's complement


def test_refill_rule_fills_everything_and_says_where_the_rejection_draws_ended():
    B = 1500
    valid = np.zeros(B, dtype=bool)
    valid[700] = True
    pick, fallback = fill_picks(valid, 0, 0, 0)
    assert pick[700] == -1 and (np.delete(pick, 700) == 700).all()
    # each of the 1499 entries misses 4096 draws with probability (1 - 1/1500)^4096 = 0.0651: 97.6 expected, sd 9.6
    assert 50 < fallback.sum() < 150 and not fallback[700]
    # three valid of 6000: (1 - 1/2000)^4096 = 0.129 of the entries take the rank fallback, which reaches every valid replicate
    valid = np.zeros(6000, dtype=bool)
    valid[[0, 3000, 5999]] = True
    pick, fallback = fill_picks(valid, 0, 1, 1)
    assert set(pick[~valid]) == {0, 3000, 5999} and (pick[valid] == -1).all()
    assert 600 < fallback.sum() < 950 and set(pick[fallback]) == {0, 3000, 5999}
    assert (fill_picks(np.zeros(5, dtype=bool), 1, 2, 0)[0] == -1).all() and (fill_picks(np.ones(5, dtype=bool), 1, 2, 0)[0] == -1).all()


def test_cross_draws_ranges_and_identity_column():
    rep, bcol = cross_draws(5, 3, 12, 250, 300)
    assert rep.dtype == np.int16 and bcol.dtype == np.int32 and rep.shape == bcol.shape == (12, 300)
    np.testing.assert_array_equal(rep[:, 0], np.arange(12))
    assert (bcol[:, 0] == 0).all() and rep.min() == 0 and rep.max() == 11 and bcol[:, 1:].min() == 1 and bcol.max() == 250


@pytest.mark.parametrize("seed", [0, 0xDEADBEEF12345678, 5])
@pytest.mark.parametrize("gene, n, nb", [(0, 12, 300), (0, 12, 263), (1, 10, 300), (3, 12, 7), (70000, 200, 41)])
def test_cross_draws_are_uniform(seed, gene, n, nb):
    """The restated rule is unbiased: chi-square of the drawn groups over the n good groups and of the drawn columns over the nb
    surviving ones against equal shares, each below chi2.isf(1e-6, dof).  A modulo of the wrong quantity, a shift that loses
    bits or a stream shared by r and bb shows here, not in a test that has the same rule on both sides."""
    rep, bcol = cross_draws(seed, gene, n, nb, 300)
    chi2_r, dof_r, chi2_b, dof_b = draws_chi2(rep, bcol, n, nb)
    assert chi2_r < scipy.stats.chi2.isf(1e-6, dof_r) and chi2_b < scipy.stats.chi2.isf(1e-6, dof_b), (chi2_r, dof_r, chi2_b, dof_b)
    # r and bb of a draw come from two mixes of one counter: their joint counts over a 4 x 4 folding are uniform too
    joint = np.bincount((rep[:, 1:].astype(np.int64) % 4 * 4 + bcol[:, 1:] % 4).ravel(), minlength=16)
    if n % 4 == 0 and nb % 4 == 0:
        want = joint.sum() / 16
        assert ((joint - want) ** 2 / want).sum() < scipy.stats.chi2.isf(1e-6, 15)
