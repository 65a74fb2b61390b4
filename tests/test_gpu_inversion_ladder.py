"""GPU tests of the two forms of the fp32 inversion search's ladder (csrc/npy_rng.h) through mm_debug_inversion_ladder: form 0, the
nested ifs that state what the search computes, and form 1, the device's asm statement with one saved EXEC mask.  For every case
(U, n, p) the two forms must agree bit for bit on the return value (X, or -1), the steps taken and the Uf and px the search stopped
with -- whatever the other lanes of the wave do, with full, partial and masked waves -- and every thread must come out of the call
(its marker is there; a lane that ran the searches has stored its results behind them).

The cases: n of 1, 5, 8, 9, 10, 59, 60, 61, 127, 128 and 50,000; p so that n p covers (0, 30], p = 0.5 included; U of 0, 2^-53,
1 - 2^-53, the midpoint of every step k <= 60 of the fp64 CDF that has some mass (the search must stop there and return k), U
inside the guard at X = 0 and at X > 0 (-1), and a sweep of U just below 1.  No distribution with n p <= 30 has mass worth the
name beyond k of about 52, so where a search in the far tail stops -- step 53 .. 60, or past 60, or in the zero-factor tail behind
n -- is decided by the fp32 rounding of its 50 odd steps: the sweep is there to produce those stops, form 0 says where each case
stopped, and the test asserts that every stop step 0 .. 60, a search that runs past 60 and a zero-factor tail were all produced.
The wave shapes are then put together from cases picked by form 0's stop step.
"""

import ctypes

import numpy as np
import pytest
from scipy import stats

pytestmark = pytest.mark.gpu

NS = (1, 5, 8, 9, 10, 59, 60, 61, 127, 128, 50_000)
SENTINEL = np.int32(-0x5EED5EED)
RET, STEPS, UF, PX = 0, 1, 2, 3
FULL = (1 << 64) - 1
ODD = 0xAAAAAAAAAAAAAAAA


def _np_pairs():
    out = []
    for n in NS:
        ps = {0.5, 0.25, 0.1, 0.02, 30.0 / n, 29.5 / n, 20.0 / n, 10.0 / n, 3.0 / n, 1.0 / n, 0.1 / n}
        if n == NS[-1]:
            # the far tail (steps 53 .. 60 and beyond) has the most mass for large n at n p near 30, and even there less than the
            # rounding of the steps before it: whether a search of such an (n, p) can get to step 59 at all is the luck of its
            # roundings (about one p in three, worked through in fp32 on the host), so the sweep below gets many p to try
            ps |= {x / n for x in np.arange(28.0, 30.0, 0.05)}
        out += [(n, float(p)) for p in sorted(ps) if 0.0 < p <= 0.5 and n * p <= 30.0]
    return out


def _cases():
    """(U, n, p, want): want = the draw the search must return, -1 where U sits inside the guard, -2 where the test does not say."""
    rows = []
    for n, p in _np_pairs():
        k = np.arange(0, min(n, 60) + 1)
        pmf = stats.binom.pmf(k, n, p)
        below = np.concatenate([[0.0], np.cumsum(pmf)[:-1]])                     # CDF(k - 1)
        rows += [(0.0, n, p, -2), (2.0 ** -53, n, p, -2), (1.0 - 2.0 ** -53, n, p, -2)]
        for kk in k[pmf > 1e-4]:                                                  # the midpoint of step kk: clear of every guard above 1e-3
            rows.append((below[kk] + 0.5 * pmf[kk], n, p, int(kk) if pmf[kk] > 1e-3 else -2))
        if pmf[0] > 1e-3:                                                         # inside the guard at X = 0
            rows.append((pmf[0] - 5e-7, n, p, -1))
        for kk in (1, 5):                                                         # inside the guard at X > 0
            if kk <= n and pmf[kk] > 1e-3 and pmf[kk - 1] > 1e-3:
                rows.append((below[kk] + 5e-7, n, p, -1))
        sweep = 2048 if n * p >= 20.0 else 64                                     # the far tail: U = 1 - j 2^-24
        rows += [(1.0 - j * 2.0 ** -24, n, p, -2) for j in range(1, sweep + 1)]
    U, n, p, want = (np.array(c) for c in zip(*rows))
    return U.astype(np.float64), n.astype(np.int32), p.astype(np.float64), want.astype(np.int32)


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


def _run(eng, U, n, p, mask=FULL):
    """out [2 forms][4 fields][count] (SENTINEL where nothing was stored) and the markers of one launch of len(U) threads."""
    import torch

    count = len(U)
    out = torch.full((2, 4, count), int(SENTINEL), dtype=torch.int32, device="cuda")
    marker = torch.zeros(count, dtype=torch.int32, device="cuda")
    dU, dn, dp = eng.dev(U, np.float64), eng.dev(n, np.int32), eng.dev(p, np.float64)
    eng._lib.call("mm_debug_inversion_ladder", eng.P(dU), eng.P(dn), eng.P(dp), count, ctypes.c_uint64(mask), eng.P(out), eng.P(marker),
                  eng._stream())
    torch.cuda.synchronize()
    return eng.host(out), eng.host(marker)


@pytest.fixture(scope="module")
def pool(eng):
    """Every case once, in full waves: computed once, shared, left unchanged."""
    U, n, p, want = _cases()
    out, marker = _run(eng, U, n, p)
    f0 = out[0]
    uf, px = f0[UF].view(np.float32), f0[PX].view(np.float32)
    stopped = ~(uf > px)                                  # the search stopped at a compare (it did not run out of steps)
    by_step = {}
    for i in np.flatnonzero(stopped):
        by_step.setdefault(int(f0[STEPS][i]), int(i))
    past = np.flatnonzero(~stopped & (f0[STEPS] == 60))
    for a in (out, marker, U, n, p, want):
        a.setflags(write=False)
    return dict(U=U, n=n, p=p, want=want, out=out, marker=marker, stopped=stopped, by_step=by_step, past=past)


def test_forms_agree_on_every_case(pool):
    out = pool["out"]
    assert not (out == SENTINEL).any()
    np.testing.assert_array_equal(pool["marker"], np.arange(1, len(pool["U"]) + 1))
    for f, name in ((RET, "return value"), (STEPS, "steps"), (UF, "Uf bits"), (PX, "px bits")):
        np.testing.assert_array_equal(out[1][f], out[0][f], err_msg=name)
    ret, steps = out[0][RET], out[0][STEPS]
    assert ((ret == -1) | (ret == steps)).all() and steps.min() == 0 and steps.max() == 60


def test_clear_cases_return_the_draw_and_guarded_cases_defer(pool):
    want = pool["want"]
    said = want > -2
    assert (want == -1).sum() >= 20 and (want >= 0).sum() >= 500
    for form in (0, 1):
        np.testing.assert_array_equal(pool["out"][form][RET][said], want[said])
    # a search that ran out of steps is never a draw
    assert (pool["out"][1][RET][pool["past"]] == -1).all()


def test_cases_cover_every_stop_step_and_both_tails(pool):
    assert sorted(pool["by_step"]) == list(range(61))                    # 0, 1, 8, 9, 10, 26, 27, 28, 59, 60 and all between
    assert len(pool["past"]) > 0                                         # ran past step 60
    n, steps = pool["n"], pool["out"][0][STEPS]
    assert ((n < 9) & (steps > n)).any()                                 # the zero-factor tail behind n
    for nn in NS:
        assert (n == nn).any()
    npv = pool["n"] * pool["p"]
    assert (pool["p"] == 0.5).any() and npv.max() == 30.0 and npv.min() <= 0.1 and len(np.unique(np.ceil(npv))) >= 12


def _lane_mod_61(pool, count):
    return np.array([pool["by_step"][i % 61] for i in range(count)])


def _shapes(pool):
    """name -> (pool indices of the launch's threads, lane mask)."""
    zero, sixty = pool["by_step"][0], pool["by_step"][60]
    zeros = np.flatnonzero(pool["stopped"] & (pool["out"][0][STEPS] == 0))
    shapes = {f"{c} threads": (np.array([pool["by_step"][(60 - i) % 61] for i in range(c)]), FULL) for c in (1, 63, 64, 65)}
    shapes["odd lanes"] = (_lane_mod_61(pool, 128), ODD)
    shapes["odd lanes, 65 threads"] = (_lane_mod_61(pool, 65), ODD)        # the second wave's only lane is masked off
    shapes["no lane"] = (_lane_mod_61(pool, 64), 0)
    shapes["all stop at step 0"] = (zeros[np.arange(64) * 7 % len(zeros)], FULL)
    for name, long_one in (("one lane to step 60", sixty), ("one lane past step 60", int(pool["past"][0]))):
        idx = np.full(64, zero)
        idx[37] = long_one
        shapes[name] = (idx, FULL)
    shapes["lane i stops at step i mod 61"] = (_lane_mod_61(pool, 192), FULL)
    return shapes


SHAPES = ["1 threads", "63 threads", "64 threads", "65 threads", "odd lanes", "odd lanes, 65 threads", "no lane", "all stop at step 0",
          "one lane to step 60", "one lane past step 60", "lane i stops at step i mod 61"]


@pytest.mark.parametrize("shape", SHAPES)
def test_wave_shapes(eng, pool, shape):
    idx, mask = _shapes(pool)[shape]
    count = len(idx)
    if shape == "lane i stops at step i mod 61":
        np.testing.assert_array_equal(pool["out"][0][STEPS][idx], np.arange(count) % 61)
        assert pool["stopped"][idx].all()
    out, marker = _run(eng, pool["U"][idx], pool["n"][idx], pool["p"][idx], mask)
    np.testing.assert_array_equal(marker, np.arange(1, count + 1))       # every thread came out of the call, masked ones included
    on = np.array([(mask >> (i % 64)) & 1 for i in range(count)], dtype=bool)
    want = pool["out"][0][:, idx]                                         # what form 0 said of these cases in full waves
    for form in (0, 1):
        np.testing.assert_array_equal(out[form][:, on], want[:, on], err_msg=f"form {form}")
        assert (out[form][:, ~on] == SENTINEL).all()
