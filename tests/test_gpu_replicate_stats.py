"""The last stage on synthetic replicate planes: mm_boot_fill_log (K8), the contractions and the 8-double test record
(mm_contract_stats; the plain two-group ``contrast`` of Bootstrap1D / Bootstrap2D, which runs the two-entry designs
{(group, +1), (control, -1)} through mm_contrast_design_stats / _rows and their one-plane twins; K9+K10) and the resample_rep helpers (mm_valid_cols, mm_residualize,
mm_cross_resampled), each against a plain numpy restatement (tests/_replicate_ref.py) at the sizes where the kernels change
path: one replicate, one short of / exactly / one past a wave and a 256-thread workgroup, several tiles, more groups than
threads.  The planes are hand-built: every kernel here takes plain [rows][ld] fp64 planes."""

import ctypes

import numpy as np
import pytest
import scipy.stats

from _replicate_ref import COUNT_COLUMNS, NAN_RECORD, _np_stats, cross_draws, draws_chi2, fill_picks

pytestmark = pytest.mark.gpu

FIT = (0.05, 1.1, 0.3)                                  # mv_fit: a non-trivial quadratic in log(mean)


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import memento_oracle

    return memento_oracle


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# -------------------------------------------------------------------------------------------------
# A. mm_boot_fill_log
# -------------------------------------------------------------------------------------------------


def _fill_log(eng, mean, var, B, mode, seed=0, keys=None):
    """mm_boot_fill_log through the C-ABI, as Bootstrap1D._fill_log calls it: (mean, var, n_invalid) after the call (host)."""
    import torch

    n_rows, ld = mean.shape
    d_m, d_v = eng.dev(mean), eng.dev(var)
    n_inv = eng.empty((n_rows, 2), torch.int32)
    fit = (ctypes.c_double * 3)(*FIT)
    d_keys = eng.dev(np.asarray(keys, dtype=np.int64)) if keys is not None else None
    eng._lib.call("mm_boot_fill_log", eng.P(d_m), eng.P(d_v), n_rows, ld, B, fit, int(mode), int(seed), eng.P(n_inv), eng.P(d_keys),
                  eng._stream())
    return eng.host(d_m), eng.host(d_v), eng.host(n_inv)


def _blank_planes(n_rows, B, rng):
    """All-valid planes [n_rows][B + 4] with pairwise distinct values; column 0 and the three padding columns hold sentinels
    (negative integers, different in every cell of both planes) that occur nowhere else."""
    ld = B + 4
    mean = rng.uniform(0.2, 9.0, size=(n_rows, ld))
    var = rng.uniform(0.2, 9.0, size=(n_rows, ld))
    for k, col in enumerate([0, B + 1, B + 2, B + 3]):
        mean[:, col] = -(1000.0 + 4 * np.arange(n_rows) + k)
        var[:, col] = -(500000.0 + 4 * np.arange(n_rows) + k)
    return mean, var


BAD = [0.0, -0.0, -1.5, np.nan]
ROW_KINDS = ["all valid", "bad mean", "bad var", "mean <= 0 with var > 0", "res_var underflows", "no valid mean", "no valid res_var",
             "one valid", "valid at 0 and B - 1"]


def _fill_planes(B, seed):
    """One row of every kind in ROW_KINDS, then the same kinds again with other values and other invalid positions."""
    rng = np.random.default_rng(seed)
    n_rows = 2 * len(ROW_KINDS)
    mean, var = _blank_planes(n_rows, B, rng)
    m, v = mean[:, 1:B + 1], var[:, 1:B + 1]                                  # views: the replicate columns
    for i in range(n_rows):
        kind = ROW_KINDS[i % len(ROW_KINDS)]
        some = np.flatnonzero(rng.random(B) < 0.3)
        bad = np.array([BAD[j % 4] for j in range(len(some))])
        if kind == "bad mean":
            m[i, some] = bad
        elif kind == "bad var":
            v[i, some] = bad
        elif kind == "mean <= 0 with var > 0":
            m[i, some] = np.where(np.isnan(bad), -2.5, bad)
        elif kind == "res_var underflows":
            m[i, some] = rng.uniform(1e6, 2e6, size=len(some))                 # prediction ~ e^25, variance the smallest denormal:
            v[i, some] = 5e-324                                               # exp(-744 - 25) is 0 in fp64
        elif kind == "no valid mean":
            m[i] = np.array([BAD[j % 4] for j in range(B)])
        elif kind == "no valid res_var":
            v[i] = np.array([BAD[j % 4] for j in range(B)])
        elif kind == "one valid":
            keep = B // 2 if i < len(ROW_KINDS) else B // 3
            m[i, np.arange(B) != keep] = np.nan
            v[i, rng.random(B) < 0.3] = 0.0                                    # var: invalid wherever mean is, and on its own
            v[i, keep] = 3.25 + i
        elif kind == "valid at 0 and B - 1":
            m[i, 1:B - 1] = np.array([BAD[j % 4] for j in range(max(0, B - 2))])
            if i >= len(ROW_KINDS) and B > 1:
                v[i, 0] = -1.0                                                # res_var: only the last replicate is valid
    return mean, var


def _expected_mode1(orc, mean, var, B):
    m, v = mean[:, 1:B + 1], var[:, 1:B + 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        res = np.stack([orc.residual_variance(m[i], v[i], FIT) for i in range(len(m))])
        want_m = np.where(m > 0, np.log(m), np.nan)
        want_v = np.where(res > 0, np.log(res), np.nan)
    n_inv = np.stack([np.isnan(want_m).sum(axis=1), np.isnan(want_v).sum(axis=1)], axis=1)
    return want_m, want_v, np.where(n_inv == B, -1, n_inv)


def _check_frame(mean, var, out_m, out_v, B):
    """Column 0 and the padding columns come back untouched, bit for bit."""
    cols = [0, B + 1, B + 2, B + 3]
    np.testing.assert_array_equal(_bits(out_m[:, cols]), _bits(mean[:, cols]))
    np.testing.assert_array_equal(_bits(out_v[:, cols]), _bits(var[:, cols]))


def _picks(filled_row, strict_row):
    """Which replicate every refilled entry took: filled_row (mode 0) against strict_row (mode 1) of the same row and plane,
    whose finite values are pairwise distinct.  -1 at the entries that were valid; fails on a value that is not of this row."""
    pos = np.flatnonzero(np.isfinite(strict_row))
    order = np.argsort(strict_row[pos])
    vals = strict_row[pos][order]
    assert (np.diff(vals) > 0).all(), "the valid values of a row are not pairwise distinct"
    pick = np.full(len(filled_row), -1, dtype=np.int64)
    inv = np.flatnonzero(~np.isfinite(strict_row))
    if not len(pos):
        assert np.isnan(filled_row).all()
        return pick
    assert np.isfinite(filled_row).all(), f"{np.isnan(filled_row).sum()} of {len(inv)} invalid entries were left unfilled"
    at = np.clip(np.searchsorted(vals, filled_row[inv]), 0, len(vals) - 1)
    assert (_bits(vals[at]) == _bits(filled_row[inv])).all(), "a refilled value is not a valid value of its own row and plane"
    pick[inv] = pos[order][at]
    return pick


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130, 700])
def test_fill_log_strict_mode_against_numpy_and_refill_against_strict(eng, orc, B):
    """fill_mode 1 against numpy (residual variance, log, NaN pattern, n_invalid with its -1), then fill_mode 0 against
    fill_mode 1 on the same input: the valid entries are the same bits, every invalid entry of a row and plane with a valid
    replicate holds a valid value OF THAT ROW AND PLANE, a plane with none is left alone, the frame is untouched."""
    mean, var = _fill_planes(B, seed=100 + B)
    want_m, want_v, want_inv = _expected_mode1(orc, mean, var, B)
    kinds = {(int(a), int(b)) for a, b in np.sign(want_inv)}
    assert kinds >= {(0, 0), (-1, -1), (0, -1)} and (B == 1 or (1, 1) in kinds and (0, 1) in kinds)     # the fixture has the rows it claims
    m1, v1, inv1 = _fill_log(eng, mean, var, B, mode=1)
    _check_frame(mean, var, m1, v1, B)
    np.testing.assert_allclose(m1[:, 1:B + 1], want_m, rtol=1e-13, equal_nan=True)
    np.testing.assert_allclose(v1[:, 1:B + 1], want_v, rtol=1e-9, atol=1e-12, equal_nan=True)
    np.testing.assert_array_equal(inv1, want_inv)
    # every finite output value occurs once in the whole launch: a value names its row, its plane and its replicate
    finite = np.concatenate([m1[:, 1:B + 1].ravel(), v1[:, 1:B + 1].ravel()])
    finite = finite[np.isfinite(finite)]
    assert len(np.unique(finite)) == len(finite) and finite.min() > -100

    m0, v0, inv0 = _fill_log(eng, mean, var, B, mode=0, seed=4321)
    _check_frame(mean, var, m0, v0, B)
    np.testing.assert_array_equal(inv0, inv1)
    n_filled = 0
    for strict, filled in ((m1, m0), (v1, v0)):
        s, f = strict[:, 1:B + 1], filled[:, 1:B + 1]
        ok = np.isfinite(s)
        np.testing.assert_array_equal(_bits(f[ok]), _bits(s[ok]))
        for i in range(len(s)):
            pick = _picks(f[i], s[i])                                         # asserts: all filled, from this row and plane
            n_filled += int((pick >= 0).sum())
    assert B == 1 or n_filled > B


def _few_valid_planes(B, valid_sets, seed):
    """Rows whose mean plane is valid exactly at valid_sets[i][0] and whose res_var plane exactly at valid_sets[i][1]."""
    rng = np.random.default_rng(seed)
    mean, var = _blank_planes(len(valid_sets), B, rng)
    for i, (vm, vv) in enumerate(valid_sets):
        assert set(vv) <= set(vm)                                             # res_var needs a valid mean
        keep_m, keep_v = np.zeros(B, bool), np.zeros(B, bool)
        keep_m[list(vm)] = True
        keep_v[list(vv)] = True
        mean[i, 1:B + 1][~keep_m] = np.nan
        var[i, 1:B + 1][~keep_v] = 0.0
    return mean, var


def _picks_of_launch(eng, mean, var, B, seed, keys=None):
    m1, v1, _ = _fill_log(eng, mean, var, B, mode=1)
    m0, v0, inv0 = _fill_log(eng, mean, var, B, mode=0, seed=seed, keys=keys)
    pm = np.stack([_picks(m0[i, 1:B + 1], m1[i, 1:B + 1]) for i in range(len(mean))])
    pv = np.stack([_picks(v0[i, 1:B + 1], v1[i, 1:B + 1]) for i in range(len(mean))])
    return pm, pv, (m0, v0, inv0)


@pytest.mark.parametrize("B, sets, min_fallback", [
    (1500, [([700], [700]), ([3, 801, 1499], [3, 801, 1499]), ([0, 5, 1499], [1499])], 200),
    (6000, [([0, 3000, 5999], [0, 3000, 5999])], 1200)])
def test_refill_fills_rows_with_very_few_valid_replicates(eng, B, sets, min_fallback):
    """B = 1500 with one valid replicate and with three: every entry is filled (the rejection draws alone leave
    (1 - V / B)^4096 of them NaN: 6.5 % with V = 1), with three all three values occur, and the picks are the restatement's,
    the rank fallback included.  With three valid of 1500 the fallback is rare (0.03 %), so B = 6000 with three (12.9 %)
    shows that it reaches every rank.  n_invalid is unchanged by the refill."""
    seed = 0
    mean, var = _few_valid_planes(B, sets, seed=7)
    pm, pv, (m0, v0, inv0) = _picks_of_launch(eng, mean, var, B, seed)
    assert np.isfinite(m0[:, 1:B + 1]).all() and np.isfinite(v0[:, 1:B + 1]).all()      # no NaN remains
    np.testing.assert_array_equal(inv0, [[B - len(vm), B - len(vv)] for vm, vv in sets])
    n_fallback = 0
    for i, (vm, vv) in enumerate(sets):
        for plane, (valid_at, got) in enumerate(((vm, pm[i]), (vv, pv[i]))):
            valid = np.zeros(B, bool)
            valid[valid_at] = True
            want, fallback = fill_picks(valid, seed, i, plane)
            np.testing.assert_array_equal(got, want, err_msg=f"row {i} plane {plane}")
            assert set(got[got >= 0]) == set(valid_at)                        # every valid replicate is taken by someone
            if B == 6000:
                assert set(got[fallback]) == set(valid_at)                    # and by someone the rejection draws had left
            n_fallback += int(fallback.sum())
    assert n_fallback > min_fallback                                          # the case is about the entries the draws miss


def test_refill_picks_are_the_documented_draws(eng):
    """B = 130 with a dozen invalid entries per row: the kernel's picks are those of the rule in include/memento_hip.h, index
    for index, for row-number keys and for caller's keys (negative and beyond 2^32 included)."""
    B, seed = 130, 987654321987
    rng = np.random.default_rng(5)
    all_r = set(range(B))
    sets = []
    for i in range(4):
        bad_m = set(rng.choice(B, size=12, replace=False).tolist())
        bad_v = bad_m | set(rng.choice(B, size=5, replace=False).tolist())
        sets.append((sorted(all_r - bad_m), sorted(all_r - bad_v)))
    mean, var = _few_valid_planes(B, sets, seed=8)
    for keys in (None, [5, 1 << 40, -3, 0]):
        pm, pv, _ = _picks_of_launch(eng, mean, var, B, seed, keys)
        for i, (vm, vv) in enumerate(sets):
            for plane, (valid_at, got) in enumerate(((vm, pm[i]), (vv, pv[i]))):
                valid = np.zeros(B, bool)
                valid[valid_at] = True
                want, fallback = fill_picks(valid, seed, i if keys is None else keys[i], plane)
                assert not fallback.any()
                np.testing.assert_array_equal(got, want, err_msg=f"keys {keys} row {i} plane {plane}")


def test_refill_is_uniform_over_the_valid_replicates(eng):
    """B = 4000, 8 valid replicates at both ends of the row and on both sides of wave and mid-row boundaries: chi-square of
    the pick counts against equal shares below chi2.isf(1e-6, 7) = 40.5.  Row 0 (key 7): the same 8 in both planes; row 1
    (key 8): a different 8 in the res_var plane (they have to be valid in the mean plane too, which has 16 there).  Seed
    and keys are fixed, so the test is deterministic; a sampler that never takes an end position, or favours one, is off by
    orders of magnitude (one empty cell of 8 alone gives 499)."""
    B, seed = 4000, 12345
    a = [0, 1, 63, 64, 1999, 2000, 3998, 3999]
    b = [2, 62, 65, 127, 128, 2048, 3000, 3997]
    mean, var = _few_valid_planes(B, [(a, a), (sorted(a + b), b)], seed=9)
    pm, pv, _ = _picks_of_launch(eng, mean, var, B, seed, keys=[7, 8])
    bound = scipy.stats.chi2.isf(1e-6, 7)
    for name, got, valid_at in (("mean, row 0", pm[0], a), ("res_var, row 0", pv[0], a), ("res_var, row 1", pv[1], b)):
        counts = np.bincount(got[got >= 0], minlength=B)
        assert counts.sum() == B - 8 and counts[valid_at].sum() == B - 8
        chi2 = float(((counts[valid_at] - (B - 8) / 8) ** 2 / ((B - 8) / 8)).sum())
        print(f"refill uniformity, {name}: counts {counts[valid_at].tolist()} chi2 {chi2:.2f} (bound {bound:.1f})")
        assert chi2 < bound, name


def test_refill_streams_are_keyed_by_seed_key_and_plane(eng):
    """The draws of a row are a function of (fill_seed, key of the row, plane, replicate) and of nothing else: the same rows
    launched in another order with their keys give the same rows bit for bit, no keys means keys 0..n-1, and another key,
    another seed or the other plane gives other picks."""
    B, seed = 130, 77
    rng = np.random.default_rng(6)
    valid = sorted(set(range(B)) - set(rng.choice(B, size=40, replace=False).tolist()))
    mean, var = _few_valid_planes(B, [(valid, valid)] * 2 + [(valid[::2], valid[::4]), (valid[:3], valid[:1]), ([], []), (valid, [])], seed=10)
    mean[1], var[1] = mean[0], var[0]                                          # two identical rows
    n = len(mean)
    keys = np.array([11, 12, 3, 4, 5, 6])
    pm, pv, (m0, v0, inv0) = _picks_of_launch(eng, mean, var, B, seed, keys)
    perm = np.array([4, 2, 0, 5, 3, 1])
    pm_p, pv_p, (m0_p, v0_p, inv0_p) = _picks_of_launch(eng, mean[perm], var[perm], B, seed, keys[perm])
    np.testing.assert_array_equal(_bits(m0_p), _bits(m0[perm]))
    np.testing.assert_array_equal(_bits(v0_p), _bits(v0[perm]))
    np.testing.assert_array_equal(inv0_p, inv0[perm])
    _, _, (m0_n, v0_n, _) = _picks_of_launch(eng, mean, var, B, seed, None)
    _, _, (m0_r, v0_r, _) = _picks_of_launch(eng, mean, var, B, seed, np.arange(n))
    np.testing.assert_array_equal(_bits(m0_n), _bits(m0_r))
    np.testing.assert_array_equal(_bits(v0_n), _bits(v0_r))
    # 40 refilled entries with 90 candidates each: two independent streams agree on all of them with probability 90^-40
    assert (pm[0] != pm[1]).sum() > 20 and (pv[0] != pv[1]).sum() > 20        # same row, other key
    assert (pm[0] != pv[0]).sum() > 20                                        # same row and key, other plane (same valid set)
    pm_s, pv_s, _ = _picks_of_launch(eng, mean, var, B, seed + 1, keys)
    assert (pm[0] != pm_s[0]).sum() > 20 and (pv[0] != pv_s[0]).sum() > 20    # other seed


# -------------------------------------------------------------------------------------------------
# B. the test record: mm_contract_stats, and the plain two-group contrast on the design kernels
# -------------------------------------------------------------------------------------------------


def _planes(eng, ym, yv, B, ng):
    """A Bootstrap1D that only holds replicate rows (what the statistics kernels read)."""
    bs = object.__new__(eng.Bootstrap1D)
    bs.ym, bs.yv, bs.ld, bs.B, bs.ng = eng.dev(ym), eng.dev(yv), ym.shape[1], B, ng
    bs.n_tested = bs.n_pairs = ym.shape[0] // ng
    return bs


def _assert_record(got, row, nothing_to_test=False, msg=""):
    # the exact count columns come from ``row``, which the callers build in numpy: on the random planes it is the kernel's row to
    # rounding only, and a count would move only at a near tie, which these seeds do not have; exact ties: test_records_at_exact_ties
    want = NAN_RECORD if nothing_to_test else _np_stats(row)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-12, equal_nan=True, err_msg=msg)
    np.testing.assert_array_equal(got[COUNT_COLUMNS], want[COUNT_COLUMNS], err_msg=msg)


def _check_contract(eng, ym, yv, B, ng, good, test_gene, W):
    """Bootstrap1D.contract, both responses: coefficient rows against numpy in the kernel's summation order (good groups
    ascending; a column is valid when every good group is finite in BOTH planes), all eight record columns against _np_stats."""
    bs = _planes(eng, ym, yv, B, ng)
    n_nan = 0
    for which in (0, 1):
        coef, stats = bs.contract(test_gene, W, good, which)
        coef = eng.host(coef)
        assert stats.shape == (len(test_gene), 8)
        for t, gene in enumerate(test_gene):
            rows = gene * ng + np.flatnonzero(good[gene])
            msg = f"which {which} test {t}"
            if not len(rows):
                assert np.isnan(coef[t, :B + 1]).all(), msg
                _assert_record(stats[t], None, nothing_to_test=True, msg=msg)
                n_nan += 1
                continue
            ok = np.isfinite(ym[rows, :B + 1]).all(axis=0) & np.isfinite(yv[rows, :B + 1]).all(axis=0)
            acc = np.zeros(B + 1)
            with np.errstate(invalid="ignore"):
                for r in rows:
                    acc = acc + W[t, r - gene * ng] * (yv if which else ym)[r, :B + 1]
            want_row = np.where(ok, acc, np.nan)
            np.testing.assert_allclose(coef[t, :B + 1], want_row, rtol=1e-13, atol=1e-13, equal_nan=True, err_msg=msg)
            _assert_record(stats[t], want_row, msg=msg)
    return n_nan


def _check_contrast(eng, ym, yv, B, ng, good, test_gene, test_grp, ctrl):
    """Bootstrap1D.contrast: both records and both rows(which, ...); a column is valid when all four operands are finite.  A
    bad guide or control group gives the NaN record; rows does not take the mask and gives the difference row all the same.
    The rows are the IEEE difference y[a] - y[c] bit for bit (up to the sign of an exact zero, which assert_array_equal
    does not see): (0.0 + 1.0 * a) + (-1.0 * b), unfused, is a - b."""
    bs = _planes(eng, ym, yv, B, ng)
    st_m, st_v, rows_of = bs.contrast(test_gene, test_grp, ctrl, good)
    idx = np.arange(len(test_gene))
    n_nan = 0
    for which, (y, st) in enumerate(((ym, st_m), (yv, st_v))):
        rows = rows_of(which, idx)
        assert st.shape == (len(test_gene), 8) and rows.shape == (len(test_gene), ym.shape[1])
        for t, (gene, grp) in enumerate(zip(test_gene, test_grp)):
            a, c = gene * ng + grp, gene * ng + ctrl
            ok = np.isfinite(ym[[a, c], :B + 1]).all(axis=0) & np.isfinite(yv[[a, c], :B + 1]).all(axis=0)
            with np.errstate(invalid="ignore"):
                want_row = np.where(ok, y[a, :B + 1] - y[c, :B + 1], np.nan)
            msg = f"which {which} test {t}"
            np.testing.assert_array_equal(rows[t, :B + 1], want_row, err_msg=msg)
            nothing = not (good[gene, grp] and good[gene, ctrl])
            _assert_record(st[t], want_row, nothing_to_test=nothing, msg=msg)
            n_nan += int(nothing)
    np.testing.assert_array_equal(rows_of(1, [3, 0])[:, :B + 1], rows_of(1, idx)[[3, 0], :B + 1])
    return n_nan


def _stat_planes(B, ng, n_genes, seed):
    """ym / yv [n_genes * ng][B + 4] with non-finite entries in ym only, in yv only and in column 0, and a run of ~40 dropped
    columns; ``good``: gene 0 partial (its bad group is non-finite throughout: to be ignored), gene 1 all good, gene 2 all bad,
    gene 3 a single good group, gene 4 partial."""
    rng = np.random.default_rng(seed)
    ld = B + 4
    ym = rng.normal(0, 1, size=(n_genes * ng, ld))
    yv = rng.normal(0, 1, size=(n_genes * ng, ld))
    good = np.ones((n_genes, ng), dtype=bool)
    good[0, 1] = False
    ym[0 * ng + 1, :] = np.nan
    yv[0 * ng + 1, ::2] = np.inf
    good[2] = False
    good[3] = False
    good[3, ng - 2] = True
    good[4, [0, ng - 1]] = False

    def col(c):                                                               # a replicate column that exists at this B
        return min(c, B)

    ym[0 * ng + 0, col(5)] = np.nan                                           # gene 0: mean plane only
    ym[0 * ng + 2, col(17)] = -np.inf
    yv[0 * ng + 3, col(B - 1)] = np.nan                                       #         variability plane only
    yv[0 * ng + ng - 1, col(B)] = np.inf                                      #         the last replicate
    ym[1 * ng + 2, 0] = np.nan                                                # gene 1: column 0, coef0 is NaN
    lo = min(B // 3, max(0, B - 40))
    ym[1 * ng + 0, 1 + lo:1 + lo + 40] = np.nan                               #         a run of dropped columns (padding is not read)
    yv[3 * ng + ng - 2, 1:B + 1:7] = np.nan                                   # gene 3: every 7th replicate, its only good group
    yv[4 * ng + 0, :] = np.nan                                                # gene 4: in bad groups only
    ym[4 * ng + ng - 1, 0] = np.inf
    ym[:, B + 1:] = np.nan                                                    # padding: never read
    yv[:, B + 1:] = np.nan
    return ym, yv, good


@pytest.mark.parametrize("B", [1, 63, 255, 256, 257, 700])
def test_contract_records_and_rows_against_numpy(eng, B):
    ng, n_genes = 6, 5
    ym, yv, good = _stat_planes(B, ng, n_genes, seed=200 + B)
    rng = np.random.default_rng(B)
    test_gene = np.array([0, 1, 2, 3, 4, 0, 1, 4, 3, 2, 1])
    W = rng.normal(0, 1, size=(len(test_gene), ng))
    W[5, 2] = 0.0                                                              # a zero weight still decides the column's validity
    assert _check_contract(eng, ym, yv, B, ng, good, test_gene, W) == 4       # gene 2 twice, both responses


@pytest.mark.parametrize("B", [1, 63, 255, 256, 257, 700])
def test_contrast_records_and_rows_against_numpy(eng, B):
    ng, n_genes, ctrl = 6, 5, 4
    ym, yv, good = _stat_planes(B, ng, n_genes, seed=300 + B)
    test_gene = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 4, 4, 4, 1, 0])
    test_grp = np.array([0, 1, 2, 5, 0, 2, 3, 0, 5, 4, 1, 1, 0, 5, 4, 3])     # a bad guide, a bad control, guide == control
    assert _check_contrast(eng, ym, yv, B, ng, good, test_gene, test_grp, ctrl) == 2 * 6


def _plane(eng, yc, B, ng):
    """A Bootstrap2D that only holds replicate rows: one plane [pair * ng + group][ld]."""
    bs = object.__new__(eng.Bootstrap2D)
    bs.yc, bs.ld, bs.B, bs.ng, bs.n_q = eng.dev(yc), yc.shape[1], B, ng, yc.shape[0]
    bs.n_pairs = yc.shape[0] // ng
    return bs


@pytest.mark.parametrize("B", [1, 256, 257])
def test_one_plane_contrast_records_and_rows_against_numpy(eng, B):
    """Bootstrap2D.contrast, the one-plane mirror of the test above: the mean plane of _stat_planes as the correlation rows of 5
    pairs.  A column is valid when the guide's and the control's entries are finite; the rows are the IEEE difference; a masked
    test has the NaN record and the rows that contrast_design gives for its unmasked design."""
    ng, n_pairs, ctrl = 6, 5, 4
    y, _, good = _stat_planes(B, ng, n_pairs, seed=400 + B)
    test_pair = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 4, 4, 4, 1, 0])
    test_grp = np.array([0, 1, 2, 5, 0, 2, 3, 0, 5, 4, 1, 1, 0, 5, 4, 3])     # a bad guide, a bad control, guide == control
    bs = _plane(eng, y, B, ng)
    stats, rows_of = bs.contrast(test_pair, test_grp, ctrl, good)
    idx = np.arange(len(test_pair))
    rows = rows_of(idx)
    assert stats.shape == (len(test_pair), 8) and rows.shape == (len(test_pair), y.shape[1])
    n_nan = 0
    for t, (pair, grp) in enumerate(zip(test_pair, test_grp)):
        a, c = pair * ng + grp, pair * ng + ctrl
        ok = np.isfinite(y[[a, c], :B + 1]).all(axis=0)
        with np.errstate(invalid="ignore"):
            want_row = np.where(ok, y[a, :B + 1] - y[c, :B + 1], np.nan)
        np.testing.assert_array_equal(rows[t, :B + 1], want_row, err_msg=f"test {t}")
        nothing = not (good[pair, grp] and good[pair, ctrl])
        _assert_record(stats[t], want_row, nothing_to_test=nothing, msg=f"test {t}")
        n_nan += int(nothing)
    assert n_nan == 6
    np.testing.assert_array_equal(rows_of([3, 0])[:, :B + 1], rows[[3, 0], :B + 1])
    # the unmasked designs, built here: design j = {(j, +1), (ctrl, -1)}
    ptr = 2 * np.arange(ng + 1)
    dgrp = np.stack([np.arange(ng), np.full(ng, ctrl)], axis=1).reshape(-1)
    st_all, rows_all = bs.contrast_design(test_pair, test_grp, ptr, dgrp, np.tile([1.0, -1.0], ng))
    np.testing.assert_array_equal(_bits(rows[:, :B + 1]), _bits(rows_all(idx)[:, :B + 1]))        # (the padding is not written)
    live = good[test_pair, test_grp] & good[test_pair, ctrl]
    np.testing.assert_array_equal(_bits(stats[live]), _bits(st_all[live]))


@pytest.mark.parametrize("plane", ["two planes", "one plane"])
def test_contrast_refuses_groups_out_of_range(eng, monkeypatch, plane):
    """``ctrl`` or an entry of ``test_grp`` outside [0, ng): ValueError, and nothing is launched."""
    B, ng, n = 5, 6, 5
    ym, yv, good = _stat_planes(B, ng, n, seed=7)
    bs = _planes(eng, ym, yv, B, ng) if plane == "two planes" else _plane(eng, ym, B, ng)

    def no_launch(name, *args):
        raise AssertionError(f"{name} was called")

    monkeypatch.setattr(eng._lib, "call", no_launch)
    rows, grps = np.array([0, 1, 2]), np.array([0, 5, 2])
    for ctrl in (-1, ng, ng + 7):
        with pytest.raises(ValueError, match="contrast:"):
            bs.contrast(rows, grps, ctrl, good)
    for bad in (-1, ng, 2 ** 20):
        with pytest.raises(ValueError, match="contrast:"):
            bs.contrast(rows, np.array([0, bad, 2]), 4, good)


def test_records_at_exact_ties(eng):
    """P-values are made from the counts [3] and [6] and the flag [5]; '>' against '>=' shows at exact ties only.  Planes of
    multiples of 0.25 and weights +-1 make the arithmetic exact: replicate coefficients 2 coef0, 0 and -coef0 have a null or a
    raw value of exactly |coef0| and are NOT extreme; with coef0 == 0 every non-zero null is; a constant test has the
    all-equal flag and range 0, and so has guide == control.  Counts, flag, range and coef0 are exact."""
    reps = 43
    B = 7 * reps                                                              # 301: more than one pass of the 256 threads
    pattern = np.array([3.0, 0.0, -1.5, 1.5, 3.25, -0.25, -1.75])            # with coef0 = 1.5: 4 extreme nulls, 3 raw extremes
    d = np.zeros((5, B + 1))
    d[0] = np.r_[1.5, np.tile(pattern, reps)]
    d[1] = -d[0]                                                              # coef0 = -1.5: the mirror image, same counts
    d[2] = np.r_[0.0, np.tile([0.0, 0.25, -0.5, 0.0, 2.0, -0.25, 0.0], reps)]  # coef0 = 0: 4 of 7 are non-zero
    d[3] = 0.75                                                               # constant
    d[4] = np.r_[1.5, np.tile(pattern, reps)]
    d[4, 2::7] = np.nan                                                       # the 0 entries dropped: 4 extreme, 3 raw of 6 a period
    want = {0: (1.5, B, 4 * reps, 0, 3 * reps, 5.0), 1: (-1.5, B, 4 * reps, 0, 3 * reps, 5.0), 2: (0.0, B, 4 * reps, 0, 4 * reps, 2.5),
            3: (0.75, B, 0, 1, 0, 0.0), 4: (1.5, B - reps, 4 * reps, 0, 3 * reps, 5.0)}
    rng = np.random.default_rng(1)
    ng, ld = 2, B + 3
    ym, yv = np.full((5 * ng, ld), np.nan), np.full((5 * ng, ld), np.nan)
    for g in range(5):
        base_m = rng.integers(-8, 9, size=B + 1) * 0.25
        base_v = rng.integers(-8, 9, size=B + 1) * 0.25
        ym[g * ng, :B + 1], ym[g * ng + 1, :B + 1] = base_m, base_m + np.nan_to_num(d[g])
        yv[g * ng, :B + 1], yv[g * ng + 1, :B + 1] = base_v, base_v - np.nan_to_num(d[g])     # the variability response: -d
        ym[g * ng + 1, :B + 1][np.isnan(d[g])] = np.nan                      # dropped through the mean plane, for both responses
    good = np.ones((5, ng), dtype=bool)
    bs = _planes(eng, ym, yv, B, ng)

    def check(stats, sign, genes, label):
        for t, g in enumerate(genes):
            c0, n, ext, flag, raw, rng_ = want[g]
            msg = f"{label} gene {g}"
            np.testing.assert_array_equal(stats[t, [0, 2, 3, 5, 6, 7]], [sign * c0, n, ext, flag, raw, rng_], err_msg=msg)
            _assert_record(stats[t], sign * d[g], msg=msg)

    genes = np.arange(5)
    st_m, st_v, rows_of = bs.contrast(genes, np.ones(5, np.int64), 0, good)
    check(st_m, 1.0, genes, "contrast mean")
    check(st_v, -1.0, genes, "contrast var")
    np.testing.assert_array_equal(rows_of(0, genes)[:, :B + 1], d)
    np.testing.assert_array_equal(rows_of(1, genes)[:, :B + 1], -d)
    st_m, st_v, rows_of = bs.contrast(genes, np.zeros(5, np.int64), 0, good)  # guide == control: 0 everywhere
    for st in (st_m, st_v):
        np.testing.assert_array_equal(st[:4], np.tile([0.0, 0.0, B, 0, 0.0, 1.0, 0, 0.0], (4, 1)))
    np.testing.assert_array_equal(rows_of(0, genes[:4])[:, :B + 1], np.zeros((4, B + 1)))
    W = np.tile([-1.0, 1.0], (5, 1))
    for which, sign in ((0, 1.0), (1, -1.0)):
        coef, stats = bs.contract(genes, W, good, which)
        check(stats, sign, genes, f"contract which {which}")
        np.testing.assert_array_equal(eng.host(coef)[:, :B + 1], sign * d)


def test_records_with_more_groups_than_threads(eng):
    """n_groups = 300: beyond the 256 threads that stage the weight row, the good list and the shared-memory sizes."""
    B, ng, n_genes = 70, 300, 3
    rng = np.random.default_rng(12)
    ld = B + 2
    ym = rng.normal(0, 1, size=(n_genes * ng, ld))
    yv = rng.normal(0, 1, size=(n_genes * ng, ld))
    good = np.ones((n_genes, ng), dtype=bool)
    good[1] = rng.random(ng) < 0.7
    good[1, [0, 255, 256, 299]] = [False, True, True, True]
    good[2] = False
    good[2, 299] = True
    ym[1 * ng + 0, :] = np.nan                                                # a bad group: ignored
    ym[0 * ng + 299, 9] = np.nan                                              # the last group decides too
    yv[0 * ng + 256, 31] = np.inf
    yv[1 * ng + 257, 0] = np.nan
    test_gene = np.array([0, 1, 2, 1, 0])
    W = rng.normal(0, 1, size=(len(test_gene), ng))
    assert _check_contract(eng, ym, yv, B, ng, good, test_gene, W) == 0
    test_gene = np.array([0, 0, 0, 1, 1, 2, 2])
    test_grp = np.array([0, 256, 298, 255, 0, 299, 7])
    assert _check_contrast(eng, ym, yv, B, ng, good, test_gene, test_grp, ctrl=299) == 2 * 2


# -------------------------------------------------------------------------------------------------
# C. mm_valid_cols, mm_residualize, mm_cross_resampled
# -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_cols", [1, 64, 256, 257, 700, 1025])
def test_valid_cols_against_numpy(eng, n_cols):
    """About 30 % of the columns non-finite at random, in the mean plane only or the variability plane only, so the counts carried
    across the four waves and across the 256-column tiles are all in use; non-finite values in bad groups are ignored;
    a gene with nothing surviving and one with only column 0.  Entries of col_map beyond n_valid are unspecified."""
    B, ng, n_genes = n_cols - 1, 5, 5
    rng = np.random.default_rng(n_cols)
    ld = n_cols + 3
    ym = rng.normal(0, 1, size=(n_genes * ng, ld))
    yv = rng.normal(0, 1, size=(n_genes * ng, ld))
    good = np.ones((n_genes, ng), dtype=bool)
    good[0, 2] = good[1, 0] = good[1, 4] = good[3, 1] = False
    for gene in range(n_genes):
        for j in np.flatnonzero(~good[gene]):                                 # bad groups: non-finite all over
            ym[gene * ng + j, ::2] = np.nan
            yv[gene * ng + j, 1::3] = -np.inf
        frac = {3: 1.0, 4: 1.0}.get(gene, 0.3)                                # gene 3: nothing survives; gene 4: column 0 only
        cols = np.flatnonzero(rng.random(n_cols) < frac)
        if gene == 4:
            cols = cols[cols > 0]
        grp = rng.choice(np.flatnonzero(good[gene]), size=len(cols))
        in_mean = rng.random(len(cols)) < 0.5
        bad = rng.choice([np.nan, np.inf, -np.inf], size=len(cols))
        ym[gene * ng + grp[in_mean], cols[in_mean]] = bad[in_mean]
        yv[gene * ng + grp[~in_mean], cols[~in_mean]] = bad[~in_mean]
    ym[:, n_cols:] = np.nan                                                   # padding: never read
    bs = _planes(eng, ym, yv, B, ng)
    col_map, n_valid = bs.valid_cols(good)
    col_map = eng.host(col_map)
    assert col_map.shape == (n_genes, n_cols)
    for gene in range(n_genes):
        rows = gene * ng + np.flatnonzero(good[gene])
        want = np.flatnonzero(np.isfinite(ym[rows, :n_cols]).all(axis=0) & np.isfinite(yv[rows, :n_cols]).all(axis=0))
        assert n_valid[gene] == len(want), f"gene {gene}"
        np.testing.assert_array_equal(col_map[gene, :len(want)], want, err_msg=f"gene {gene}")
    assert n_valid[3] == 0 and n_valid[4] == 1 and (n_cols < 64 or 0 < n_valid[0] < n_cols)


def _residualize(eng, src, n_cols, ng, gene_mask, M):
    """mm_residualize through the C-ABI into a destination preset to -7: the destination on the host."""
    d_src, d_dst = eng.dev(src), eng.dev(np.full_like(src, -7.0))
    d_gm, d_M = eng.dev(gene_mask), eng.dev(M)
    eng._lib.call("mm_residualize", eng.P(d_src), eng.P(d_dst), src.shape[1], n_cols, ng, len(gene_mask), eng.P(d_gm), eng.P(d_M),
                  eng._stream())
    return eng.host(d_dst)


@pytest.mark.parametrize("n_cols", [5, 256, 700])
@pytest.mark.parametrize("ng", [3, 130, 300])
def test_residualize_against_an_exact_matrix_product(eng, ng, n_cols):
    """dst = M src per gene and column, against a long-double product over the non-zero terms.  An exact zero of M skips its
    operand, so the NaN rows of zero-weight groups do not spread; a row of M that is all zero comes out NaN.  Bound per
    element: n_groups * 2^-52 * sum_j |M_ij y_j|, the worst case of rounding every product and a sequential fp64 sum of
    n_groups terms (n * 2^-53 * sum, to first order) with a factor 2 for the higher orders and the reference's own rounding."""
    rng = np.random.default_rng(1000 * ng + n_cols)
    n_genes, ld = 3, n_cols + 3
    src = rng.normal(0, 1, size=(n_genes * ng, ld))
    M = rng.normal(0, 1, size=(2, ng, ng))
    M[rng.random(M.shape) < 0.1] = 0.0                                        # scattered exact zeros
    dead = [np.array([1]), np.array([0, ng - 1])]                             # mask 0 / mask 1: groups with a zero row and column
    for k in range(2):
        M[k][dead[k], :] = 0.0
        M[k][:, dead[k]] = 0.0
    gene_mask = np.array([1, 0, 1], dtype=np.int32)
    for gene in range(n_genes):
        src[gene * ng + dead[gene_mask[gene]], :] = np.nan                    # zero-weight groups: NaN source rows
    src[0 * ng + dead[1][0], 2] = np.inf
    dst = _residualize(eng, src, n_cols, ng, gene_mask, M)
    np.testing.assert_array_equal(dst[:, n_cols:], -7.0)                      # columns beyond n_cols are not written
    for gene in range(n_genes):
        k = gene_mask[gene]
        y = src[gene * ng:(gene + 1) * ng, :n_cols].copy()
        y[dead[k]] = 0.0                                                      # their weights are exact zeros: the terms are skipped
        want = (M[k].astype(np.longdouble) @ y.astype(np.longdouble))
        bound = ng * 2.0 ** -52 * (np.abs(M[k]) @ np.abs(y))
        got = dst[gene * ng:(gene + 1) * ng, :n_cols]
        live = np.setdiff1d(np.arange(ng), dead[k])
        assert np.isnan(got[dead[k]]).all(), f"gene {gene}: all-zero rows of M"
        err = np.abs((got[live].astype(np.longdouble) - want[live]).astype(np.float64))
        assert np.isfinite(got[live]).all() and (err <= bound[live]).all(), f"gene {gene}: worst error / bound {np.max(err / bound[live]):.3g}"


def _cross_resampled(eng, yt, B, ng, test_gene, tt, good, Nc, rep, bcol, col_map, n_valid, seed):
    """mm_cross_resampled through the C-ABI: (coefficient rows [n_tests][ld], records [n_tests][8]) on the host."""
    import torch

    n_tests, ld = len(test_gene), yt.shape[1]
    coef, stats = eng.empty((n_tests, ld), torch.float64), eng.empty((n_tests, 8), torch.float64)
    d = [eng.dev(yt), eng.dev(np.asarray(test_gene, dtype=np.int32)), eng.dev(tt), eng.dev(good.astype(np.uint8)), eng.dev(Nc)]
    d_rep = eng.dev(np.ascontiguousarray(rep, dtype=np.int16)) if rep is not None else None
    d_bcol = eng.dev(np.ascontiguousarray(bcol, dtype=np.int32)) if bcol is not None else None
    d_cm = eng.dev(np.ascontiguousarray(col_map, dtype=np.int32)) if col_map is not None else None
    d_nv = eng.dev(np.ascontiguousarray(n_valid, dtype=np.int32)) if n_valid is not None else None
    eng._lib.call("mm_cross_resampled", eng.P(d[0]), ld, B, ng, eng.P(d[1]), eng.P(d[2]), eng.P(d[3]), eng.P(d[4]), eng.P(d_rep), eng.P(d_bcol),
                  eng.P(d_cm), eng.P(d_nv), int(seed), n_tests, eng.P(coef), eng.P(stats), eng._stream())
    return eng.host(coef), eng.host(stats)


def _cross_problem(B, ng, seed):
    """Four genes of 12 groups: all good, ten good, one good (every column degenerate), all good.  Dropped columns for the
    col_map variant: gene 0 loses 37, gene 1 none, gene 2 five, gene 3 all but column 0 (n_valid = 1)."""
    rng = np.random.default_rng(seed)
    n_genes, ld = 4, B + 2
    yt = rng.normal(0, 1, size=(n_genes * ng, ld))
    yt[:, B + 1:] = np.nan
    good = np.ones((n_genes, ng), dtype=bool)
    good[1, [3, 7]] = False
    yt[1 * ng + 3] = np.nan                                                    # a bad group's rows are never read
    good[2] = False
    good[2, 5] = True
    test_gene = np.array([0, 1, 2, 1, 0, 3])
    tt = rng.normal(0, 1, size=(len(test_gene), ng))
    Nc = rng.integers(200, 900, size=ng).astype(np.float64)
    col_map = np.zeros((n_genes, B + 1), dtype=np.int32)
    n_valid = np.zeros(n_genes, dtype=np.int32)
    for gene, dropped in enumerate([np.r_[4, 60:95, B], [], [1, 2, 3, 64, B - 1], np.arange(1, B + 1)]):
        keep = np.setdiff1d(np.arange(B + 1), dropped)
        col_map[gene, :len(keep)] = keep
        n_valid[gene] = len(keep)
    return yt, good, test_gene, tt, Nc, col_map, n_valid


@pytest.mark.parametrize("seed", [0, 0xDEADBEEF12345678])
@pytest.mark.parametrize("dropped", [False, True])
def test_cross_resampled_device_draws_are_the_documented_ones(eng, dropped, seed):
    """d_rep == NULL draws by the rule of include/memento_hip.h: the launch that draws on the device equals, bit for bit, the
    same kernel fed with rep / bcol tables built from the numpy restatement of that rule -- coefficient rows and records,
    with all columns and with some dropped through col_map / n_valid.  Edges: n_valid <= 1 gives the NaN record and a NaN row, a
    single good group gives NaN everywhere (the degenerate-column rule), columns nb..B of every row are NaN.  Both sides of
    that comparison follow the same rule, so the rule itself is checked on the host: ranges 0 <= r < n, 1 <= bb <= nb, and the
    chi-squares of r over n and of bb over nb cells against equal shares below chi2.isf(1e-6, dof)."""
    B, ng = 300, 12
    yt, good, test_gene, tt, Nc, col_map, n_valid = _cross_problem(B, ng, seed=21)
    if not dropped:
        col_map = n_valid = None
    rep = np.zeros((len(good), ng, B), dtype=np.int16)
    bcol = np.zeros((len(good), ng, B), dtype=np.int32)
    nbs, n_uniform = [], 0
    for gene in range(len(good)):
        n, nb = int(good[gene].sum()), int(n_valid[gene]) - 1 if dropped else B
        nbs.append(nb)
        if nb >= 1:
            rep[gene, :n], bcol[gene, :n] = cross_draws(seed, gene, n, nb, B)
        if nb >= 1 and n >= 10:                                               # host-side, on the restated draws: ranges and uniformity
            chi2_r, dof_r, chi2_b, dof_b = draws_chi2(rep[gene, :n], bcol[gene, :n], n, nb)
            print(f"device draws, seed {seed} gene {gene}: chi2 of r {chi2_r:.1f} (dof {dof_r}), of bb {chi2_b:.1f} (dof {dof_b})")
            assert chi2_r < scipy.stats.chi2.isf(1e-6, dof_r) and chi2_b < scipy.stats.chi2.isf(1e-6, dof_b)
            n_uniform += 1
    assert n_uniform == (2 if dropped else 3)                                 # genes 0, 1 and, with its columns, 3
    coef_d, st_d = _cross_resampled(eng, yt, B, ng, test_gene, tt, good, Nc, None, None, col_map, n_valid, seed)
    coef_t, st_t = _cross_resampled(eng, yt, B, ng, test_gene, tt, good, Nc, rep, bcol, col_map, n_valid, seed + 1)   # tables: the seed is unused
    np.testing.assert_array_equal(_bits(coef_d[:, :B + 1]), _bits(coef_t[:, :B + 1]))
    np.testing.assert_array_equal(_bits(st_d), _bits(st_t))
    for t, gene in enumerate(test_gene):
        nb, row = nbs[gene], coef_d[t, :B + 1]
        if nb < 1:                                                            # gene 3 with its columns dropped
            assert np.isnan(row).all()
            _assert_record(st_d[t], None, nothing_to_test=True)
            continue
        assert np.isnan(row[nb:]).all()
        if gene == 2:                                                         # one good group
            assert np.isnan(row).all() and st_d[t, 2] == 0 and np.isnan(st_d[t, :2]).all()
        else:                                                                 # 10+ groups: no degenerate column (P < 1e-3 each) on these seeds
            assert np.isfinite(row[:nb]).all() and st_d[t, 2] == nb - 1
        _assert_record(st_d[t], np.r_[row[:nb], np.full(B + 1 - nb, np.nan)])
    other, _ = _cross_resampled(eng, yt, B, ng, test_gene, tt, good, Nc, None, None, col_map, n_valid, seed + 1)
    assert (other[0, 1:nbs[0]] != coef_d[0, 1:nbs[0]]).all() and other[0, 0] == coef_d[0, 0]    # another seed: other draws, same column 0
    assert (coef_d[0, 1:nbs[0]] != coef_d[4, 1:nbs[0]]).all()                  # same gene, same draws, another treatment row
