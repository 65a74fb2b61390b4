"""The definition of the max-T adjustment (tests/_family_ref.py) on its own: the properties a single-step adjustment must have,
and its calibration under a true null on simulated families of independent groups.  No GPU.

Simulation: group g has sd_g = 1 / sqrt(Nc_g), Nc ~ U(200, 800); the observed column y_0 ~ N(0, sd^2) and the replicates
y_c = y_0 + N(0, sd^2); contrasts y_a - y_b; 2,000 families, ``default_rng(1)`` per case.  A family rejects when its smallest
adjusted p-value is <= 0.05; with 2,000 families the binomial sd of a 0.05 rejection rate is 0.0049, so [0.03, 0.07] is +- 4 sd."""

import numpy as np
import pytest

import _family_ref as ref

N_FAM = 2000


def _planes(rng, n_groups, B, scale=1.0):
    y0 = rng.normal(0, scale, size=(n_groups, 1))
    return np.concatenate([y0, y0 + rng.normal(0, scale, size=(n_groups, B))], axis=1)


def _pair_designs(pairs):
    return [([a, b], [1.0, -1.0]) for a, b in pairs]


def test_one_member_counts_what_the_record_counts():
    rng = np.random.default_rng(3)
    for _ in range(20):
        ym, yv = _planes(rng, 2, 300), _planes(rng, 2, 300)
        fam = ref.family(ym, yv, _pair_designs([(1, 0)]))
        np.testing.assert_array_equal(fam["n_adj"][0], fam["records"][0, :, 3])
        np.testing.assert_array_equal(fam["n_valid"], fam["records"][0, :, 2])
        np.testing.assert_array_equal(ref.p_adj(fam)[0], [ref.count_pvalue(fam["records"][0, k]) for k in range(2)])


def test_adding_a_member_never_lowers_an_adjusted_p_value():
    rng = np.random.default_rng(4)
    pairs = ref.pairwise(5)
    ym, yv = _planes(rng, 5, 300), _planes(rng, 5, 300)
    before = None
    for m in range(1, len(pairs) + 1):
        p = ref.p_adj(ref.family(ym, yv, _pair_designs(pairs[:m])))
        if before is not None:
            assert (p[:m - 1] >= before).all()
        before = p
    assert (before[:1] > ref.p_adj(ref.family(ym, yv, _pair_designs(pairs[:1])))).any()       # and it does raise some


def test_excluded_members_change_nothing_for_the_others():
    rng = np.random.default_rng(5)
    ym, yv = _planes(rng, 5, 300), _planes(rng, 5, 300)
    ym[4, 7] = np.nan                                                   # group 4 drops column 7 -- of its own members only
    yv[3] = yv[3, :1]                                                   # group 3 is constant on the variability plane
    live = _pair_designs([(1, 0), (2, 0), (2, 1)])
    want = ref.family(ym, yv, live)
    # an empty design, a member of a constant group (all_equal on the variability plane only) and one with scale 0 by hand
    designs = [live[0], ([], []), live[1], ([3], [1.0]), live[2], ([4, 0], [1.0, -1.0])]
    got = ref.family(ym, yv, designs)
    assert got["scale"][3, 1] == 0 and got["scale"][3, 0] > 0 and got["scale"][1].tolist() == [0, 0]
    scale = got["scale"].copy()
    scale[5] = 0
    scale[3] = 0
    got = ref.family(ym, yv, designs, scale)
    keep = [0, 2, 4]
    for key in ("t0", "n_adj"):
        np.testing.assert_array_equal(got[key][keep], want[key])
    np.testing.assert_array_equal(got["maxrow"], want["maxrow"])
    np.testing.assert_array_equal(got["n_valid"], want["n_valid"])
    assert np.isnan(got["t0"][[1, 3, 5]]).all() and (got["n_adj"][[1, 3, 5]] == 0).all() and np.isnan(ref.p_adj(got)[[1, 3, 5]]).all()
    assert got["n_included"].tolist() == [3, 3] and got["n_valid"].tolist() == [300, 300]
    # included, the member on group 4 takes its dropped column out of the whole family
    with_4 = ref.family(ym, yv, designs)
    assert with_4["n_included"].tolist() == [5, 4] and with_4["n_valid"].tolist() == [299, 299] and np.isnan(with_4["maxrow"][:, 7]).all()


def test_adjusted_is_never_below_the_count_on_the_family_valid_columns():
    rng = np.random.default_rng(6)
    ym, yv = _planes(rng, 4, 300), _planes(rng, 4, 300)
    ym[2, 11], yv[0, 200] = np.inf, np.nan
    designs = _pair_designs(ref.pairwise(4))
    fam = ref.family(ym, yv, designs)
    p = ref.p_adj(fam)
    for k in range(2):
        valid = ~np.isnan(fam["maxrow"][k])
        assert valid.sum() == 298
        for j, (grp, w) in enumerate(designs):
            coef, _ = ref.coef_rows(ym, yv, np.asarray(grp), np.asarray(w))
            count = (np.abs(coef[k, valid] - coef[k, 0]) > abs(coef[k, 0])).sum()
            assert p[j, k] >= (1 + count) / (1 + valid.sum())


def _simulate(n_levels, pairs, B, seed=1):
    """-> (rejection rate by the smallest adjusted p-value, by the smallest raw p-value, coverage of every member by the 0.95
    simultaneous interval), on the mean plane of N_FAM null families."""
    rng = np.random.default_rng(seed)
    designs = _pair_designs(pairs)
    rej_adj = rej_raw = covered = 0
    for _ in range(N_FAM):
        sd = 1 / np.sqrt(rng.uniform(200, 800, size=n_levels))
        y0 = rng.normal(0, 1, size=n_levels) * sd
        y = np.concatenate([y0[:, None], y0[:, None] + rng.normal(0, 1, size=(n_levels, B)) * sd[:, None]], axis=1)
        fam = ref.family(y, y, designs)
        rej_adj += ref.p_adj(fam)[:, 0].min() <= 0.05
        rej_raw += min(ref.count_pvalue(fam["records"][j, 0]) for j in range(len(pairs))) <= 0.05
        covered += fam["t0"][:, 0].max() <= ref.crit(fam, 0.95)[0]      # the truth is 0: |coef0| <= crit * se for every member
    return rej_adj / N_FAM, rej_raw / N_FAM, covered / N_FAM


def test_null_calibration_five_levels_pairwise():
    adj, raw, cover = _simulate(5, ref.pairwise(5), 400)
    print(f"\n5 levels pairwise, B = 400: rejection {adj:.4f} adjusted, {raw:.4f} raw; coverage {cover:.4f}")
    assert 0.03 <= adj <= 0.07
    assert raw > 0.2                                                    # the unadjusted minimum does fail: the check can fail
    assert cover >= 0.93


def test_null_calibration_three_levels_pairwise():
    adj, _, _ = _simulate(3, ref.pairwise(3), 400)
    print(f"\n3 levels pairwise, B = 400: rejection {adj:.4f}")
    assert 0.03 <= adj <= 0.07


def test_null_calibration_many_to_one():
    adj, _, _ = _simulate(6, [(a, 0) for a in range(1, 6)], 400)
    print(f"\n6 levels against one control, B = 400: rejection {adj:.4f}")
    assert adj <= 0.07                                                  # conservative is allowed
