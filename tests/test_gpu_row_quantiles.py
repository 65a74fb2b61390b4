"""mm_row_quantiles (order statistics of replicate rows) through the C-ABI on hand-built planes, row by row against
np.nanquantile(row[1:B + 1], probs, method='linear').

The selection is exact and the interpolation is numpy's _lerp written out (three unfused fp64 operations), so the results must
be bit-equal wherever the weight t = h - floor(h), h = (n - 1) p, is 0 (probs 0 and 1, n == 1, every integer h) and within
rtol = 1e-13 elsewhere; n_valid must be exact.  Planes have ld = B + 4; column 0 and the three padding columns hold sentinels
that occur nowhere else, and no result may equal one.  Sizes: one replicate, two, one short of / exactly / one past a wave and
a 256-thread workgroup, several strides (1000), the real size (10,000) and a row longer than the LDS of a CU could hold
(40,000); 1, 3 and 1000 rows (more workgroups than CUs).

One rule goes beyond numpy: where an order statistic that takes part is +-inf, numpy's _lerp returns NaN (inf - inf, or inf * 0)
and the kernel returns the order statistic itself when t == 0 or both are equal (include/memento_hip.h).  The expectation of
those entries, and of those only, is that rule restated in numpy (``_with_inf_rule``)."""

import ctypes
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P5 = [0.0, 0.025, 0.5, 0.975, 1.0]
P1 = [0.5]
P8 = [0.0, 0.1, 0.25, 0.5, 0.5, 0.9, 0.999, 1.0]           # 8 at once, one of them twice
PROB_SETS = [P5, P1, P8]
KINDS = ["distinct", "all equal", "three values", "equal in the top 56 bits", "mixed signs, zeros, subnormals", "inf at both ends",
         "30 % NaN", "NaN but one", "all NaN", "NaN in column 0"]
MARK = 12345.0                                               # what the output buffers hold before a launch


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


def _sentinels(n_rows, B):
    """[n_rows][4]: the values of column 0 and of the three padding columns; negative integers below -1e6, all different."""
    return -(1.0e6 + 4 * np.arange(n_rows)[:, None] + np.arange(4)[None, :])


def _fill_row(kind, B, rng, i):
    """The B replicate values of one row of the given kind."""
    if kind in ("distinct", "NaN in column 0"):
        return rng.permutation(np.linspace(-3.0, 7.0, B) + rng.uniform(0, 1e-3 / B))
    if kind == "all equal":
        return np.full(B, 2.5 + i)
    if kind == "three values":
        return rng.choice([-1.25, 0.5, 3.0], size=B)
    if kind == "equal in the top 56 bits":
        return 1.0 + rng.integers(0, 200, size=B) * 2.0 ** -52
    if kind == "mixed signs, zeros, subnormals":
        v = rng.normal(size=B) * 10.0 ** rng.integers(-3, 4, size=B)
        special = np.array([-0.0, 0.0, 5e-324, -5e-324, 1.1e-308, -1e-310, 1e-300, -1e-300, 1e300, -1e300])
        pick = rng.random(B) < 0.4
        v[pick] = rng.choice(special, size=int(pick.sum()))
        return v
    if kind == "inf at both ends":
        v = rng.uniform(-5.0, 5.0, size=B)
        if B == 1:
            v[0] = np.inf
        elif B < 8:
            v[0], v[-1] = np.inf, -np.inf
        else:
            pos = rng.choice(B, size=4, replace=False)
            v[pos[:2]], v[pos[2:]] = -np.inf, np.inf
        return v
    if kind == "30 % NaN":
        v = rng.uniform(-2.0, 2.0, size=B)
        v[rng.random(B) < 0.3] = np.nan
        return v
    if kind == "NaN but one":
        v = np.full(B, np.nan)
        v[int(rng.integers(0, B))] = -7.75 - i
        return v
    if kind == "all NaN":
        return np.full(B, np.nan)
    raise AssertionError(kind)


def _plane(kinds, B, seed):
    """One row per entry of ``kinds``: (plane [n_rows][B + 4], sentinels)."""
    rng = np.random.default_rng(seed)
    n_rows, ld = len(kinds), B + 4
    sent = _sentinels(n_rows, B)
    plane = np.empty((n_rows, ld))
    plane[:, [0, B + 1, B + 2, B + 3]] = sent
    for i, kind in enumerate(kinds):
        plane[i, 1:B + 1] = _fill_row(kind, B, rng, i)
        if kind == "NaN in column 0":
            plane[i, 0] = np.nan
    return plane, sent


def _rq(eng, plane, B, probs):
    """mm_row_quantiles as engine.row_quantiles calls it: (q [n_rows][n_probs], n_valid [n_rows]) on the host; the output
    buffers are pre-filled so that an entry the kernel does not write shows."""
    import torch

    n_rows, ld = plane.shape
    d = eng.dev(plane)
    q = torch.full((n_rows, len(probs)), MARK, dtype=torch.float64, device="cuda")
    nv = torch.full((n_rows,), -77, dtype=torch.int32, device="cuda")
    pr = (ctypes.c_double * len(probs))(*probs)
    eng._lib.call("mm_row_quantiles", eng.P(d), n_rows, ld, B, pr, len(probs), eng.P(q), eng.P(nv), eng._stream())
    return eng.host(q), eng.host(nv)


def _lerp_parts(vals, p):
    """(n, a, b, t) of numpy's 'linear' method for the non-NaN values ``vals``."""
    s = np.sort(vals)
    n = len(s)
    h = (n - 1) * p
    lo = min(int(np.floor(h)), n - 1)
    return n, s[lo], s[min(lo + 1, n - 1)], h - np.floor(h)


def _with_inf_rule(want, vals, probs):
    """``want`` = np.nanquantile(vals, probs) with the entries whose order statistics include +-inf replaced by the header's rule."""
    if not np.isinf(vals).any():
        return want
    want = want.copy()
    for k, p in enumerate(probs):
        n, a, b, t = _lerp_parts(vals, p)
        if np.isinf(a) or np.isinf(b):
            with np.errstate(invalid="ignore"):
                want[k] = a if (t == 0 or a == b) else (a + (b - a) * t if t < 0.5 else b - (b - a) * (1 - t))
    return want


def _check(plane, sent, B, probs, q, nv):
    """Every row of the launch against np.nanquantile; -> how many entries had to be bit-equal."""
    n_exact = 0
    assert q.shape == (len(plane), len(probs)) and nv.shape == (len(plane),)
    assert not np.isin(q, sent).any() and not (q == MARK).any()
    for i in range(len(plane)):
        row = plane[i, 1:B + 1]
        vals = row[~np.isnan(row)]
        assert nv[i] == len(vals), (i, nv[i], len(vals))
        if not len(vals):
            assert np.isnan(q[i]).all(), (i, q[i])
            continue
        with warnings.catch_warnings(), np.errstate(invalid="ignore"):
            warnings.simplefilter("ignore", RuntimeWarning)
            want = np.nanquantile(row, probs, method="linear")
        want = _with_inf_rule(want, vals, probs)
        np.testing.assert_allclose(q[i], want, rtol=1e-13, atol=0, equal_nan=True, err_msg=f"row {i}, B {B}, probs {probs}")
        h = (len(vals) - 1) * np.asarray(probs)
        exact = (h == np.floor(h)) | (len(vals) == 1)
        same = (q[i] == want) | (np.isnan(q[i]) & np.isnan(want))      # == : bit-equal but for the sign of a zero
        assert same[exact].all(), (i, B, probs, q[i], want)
        n_exact += int(exact.sum())
    return n_exact


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_every_row_kind_at_the_sizes_where_the_paths_change(eng, B):
    plane, sent = _plane(KINDS, B, seed=100 + B)
    n_exact = 0
    for probs in PROB_SETS:
        q, nv = _rq(eng, plane, B, probs)
        n_exact += _check(plane, sent, B, probs, q, nv)
    assert n_exact >= 2 * len(KINDS)                               # probs 0 and 1 of every row at the least
    assert nv[KINDS.index("all NaN")] == 0 and nv[KINDS.index("NaN but one")] == 1 and nv[KINDS.index("NaN in column 0")] == B


def test_the_real_size(eng):
    B = 10_000
    plane, sent = _plane(KINDS[:8], B, seed=7)
    # ranks inside runs of ties: the three-value row has runs of ~3,333 and every wanted rank of P8 falls inside one
    parts = [_lerp_parts(plane[2, 1:B + 1], p) for p in P8]
    assert all(a == b for _, a, b, _ in parts) and len({a for _, a, _, _ in parts}) == 3
    for probs in PROB_SETS:
        q, nv = _rq(eng, plane, B, probs)
        _check(plane, sent, B, probs, q, nv)
    assert set(np.unique(q[2])) == {-1.25, 0.5, 3.0}              # (q: the P8 launch)


def test_a_row_longer_than_the_lds(eng):
    B = 40_000                                                      # 320 KB per row
    plane, sent = _plane(["distinct", "30 % NaN"], B, seed=8)
    for probs in (P5, P8):
        q, nv = _rq(eng, plane, B, probs)
        _check(plane, sent, B, probs, q, nv)


@pytest.mark.parametrize("n_rows", [1, 3, 1000])
def test_row_counts(eng, n_rows):
    B = 257
    kinds = [KINDS[(3 * i) % len(KINDS)] for i in range(n_rows)]
    plane, sent = _plane(kinds, B, seed=900 + n_rows)
    q, nv = _rq(eng, plane, B, P5)
    _check(plane, sent, B, P5, q, nv)
    if n_rows == 1000:                                             # every row its own result: shuffled rows, shuffled results
        perm = np.random.default_rng(1).permutation(n_rows)
        q2, nv2 = _rq(eng, plane[perm], B, P5)
        np.testing.assert_array_equal(q2, q[perm])
        np.testing.assert_array_equal(nv2, nv[perm])


def test_inf_sorts_to_the_ends_and_comes_out_as_inf(eng):
    B = 1000
    rng = np.random.default_rng(5)
    plane, sent = _plane(["distinct"], B, seed=6)
    pos = rng.choice(B, size=10, replace=False) + 1
    plane[0, pos[:5]], plane[0, pos[5:]] = -np.inf, np.inf
    probs = [0.0, 0.05, 0.5, 0.95, 1.0]                             # ranks 49.95, 499.5, 949.05 are finite; 0 and 999 are not
    q, nv = _rq(eng, plane, B, probs)
    assert nv[0] == B and q[0, 0] == -np.inf and q[0, 4] == np.inf
    want = np.nanquantile(plane[0, 1:B + 1], probs[1:4], method="linear")
    assert np.isfinite(want).all()
    np.testing.assert_allclose(q[0, 1:4], want, rtol=1e-13, atol=0)


def test_engine_wrapper(eng):
    B = 300
    plane, sent = _plane(KINDS, B, seed=11)
    q_ref, nv_ref = _rq(eng, plane, B, P5)
    q, nv = eng.row_quantiles(eng.dev(plane), B + 4, B, P5)
    assert tuple(q.shape) == (len(KINDS), 5) and q.is_cuda
    np.testing.assert_array_equal(eng.host(q), q_ref)
    np.testing.assert_array_equal(nv, nv_ref)
    q0, nv0 = eng.row_quantiles(eng.dev(plane)[:0], B + 4, B, P5)   # no rows: no launch
    assert tuple(q0.shape) == (0, 5) and len(nv0) == 0


@pytest.mark.parametrize("case", ["n_probs 0", "n_probs 9", "prob 1.5", "prob NaN", "ld too small", "num_boot 0"])
def test_argument_errors(eng, case):
    import torch

    B = 100
    plane, _ = _plane(["distinct", "three values"], B, seed=3)
    n_rows, ld = plane.shape
    probs, n_probs, num_boot = [0.1, 0.5, 0.9] + [0.5] * 6, 3, B
    if case == "n_probs 0":
        n_probs = 0
    elif case == "n_probs 9":
        n_probs = 9
    elif case == "prob 1.5":
        probs[1] = 1.5
    elif case == "prob NaN":
        probs[2] = float("nan")
    elif case == "ld too small":
        ld = B                                                     # < num_boot + 1 (the buffer itself is large enough)
    elif case == "num_boot 0":
        num_boot = 0
    lib = eng._lib.load()
    d = eng.dev(plane)
    q = torch.full((n_rows, 9), MARK, dtype=torch.float64, device="cuda")
    nv = torch.full((n_rows,), -77, dtype=torch.int32, device="cuda")
    rc = lib.mm_row_quantiles(eng.P(d), n_rows, ld, num_boot, (ctypes.c_double * 9)(*probs), n_probs, eng.P(q), eng.P(nv), eng._stream())
    assert rc != 0
    assert b"bad argument" in lib.mm_last_error()
    torch.cuda.synchronize()
    assert (eng.host(q) == MARK).all() and (eng.host(nv) == -77).all()
    with pytest.raises(eng._lib.MementoHipError):
        eng._lib.call("mm_row_quantiles", eng.P(d), n_rows, ld, num_boot, (ctypes.c_double * 9)(*probs), n_probs, eng.P(q), eng.P(nv),
                      eng._stream())
