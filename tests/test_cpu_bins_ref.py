"""The numpy restatement of the 1D bin stage (tests/_bins_ref.py) checked on its own (no GPU), on the problem the device tests
use: against the oracle's np.unique bins, against numpy's own multinomial draws, and against engine._replay_order -- the
arithmetic of the host fallback, which needs no device."""

import numpy as np
import pytest

from _bins_ref import K_1905, MAX_COUNT, pair_cells, problem_1905, ref_count, ref_order, ref_table, ulp_diff


@pytest.fixture(scope="module")
def orc():
    from oracle import memento_oracle

    return memento_oracle


@pytest.fixture(scope="module")
def prob():
    return problem_1905()


@pytest.fixture(scope="module")
def ordered(prob):
    """ref_order of all ten (gene, group) pairs, computed once: [pair] -> (table, (bin, x, mult, pk, lq, a, b))."""
    out = []
    for p in range(prob.n_genes * prob.ng):
        x, sbin = pair_cells(prob, p)
        t = ref_table(x, sbin, prob.n_bins, int(x.max()) + 1)
        out.append((t, ref_order(t, prob.sf_table, prob.r1[p], prob.r0[p], len(x))))
    return out


def test_problem_has_the_designed_chains(prob, ordered):
    assert prob.sizes == [20000, 4000]
    assert [[ref_count(ordered[g * 2 + k][0]) for k in range(2)] for g in range(5)] == K_1905
    t = ordered[3 * 2 + 0][0]
    assert t.shape == (4, MAX_COUNT + 1) and t[3, MAX_COUNT] == 1 and prob.X[:, 3].max() == MAX_COUNT
    assert (ordered[4 * 2 + 0][0] != 0).all()                      # gene 4, group 0: every one of the 4 x 256 bins is occupied
    for p, (t, _) in enumerate(ordered):
        assert t.sum() == prob.sizes[p % 2]


def test_ref_table_counts_cells():
    t = ref_table([0, 0, 3, 1, 3, 0], [1, 1, 0, 2, 0, 2], 3, 5)
    assert t.dtype == np.uint32 and t.tolist() == [[0, 0, 0, 2, 0], [2, 0, 0, 0, 0], [1, 1, 0, 0, 0]]
    assert ref_count(t) == 4 and ref_count(np.zeros((2, 1), np.uint32)) == 0
    with pytest.raises(AssertionError):
        ref_table([5], [0], 1, 5)


def test_ref_order_small_case_by_hand():
    """Three bins, worked by hand: codes 0.25 * x + 0.5 * sf = 1.0 (bin 1, x 0), 0.75 (bin 0, x 1), 0.5 (bin 0, x 0)."""
    t = np.array([[5, 2], [1, 0]], dtype=np.uint32)
    bi, xi, mult, pk, lq, a, b = ref_order(t, [1.0, 2.0], 0.25, 0.5, 8)
    assert (bi.tolist(), xi.tolist(), mult.tolist()) == ([0, 0, 1], [0, 1, 0], [5, 2, 1])
    assert pk.tolist() == [5 / 8, (2 / 8) / (1.0 - 5 / 8), (1 / 8) / (1.0 - 5 / 8 - 2 / 8)]
    assert ulp_diff(lq, np.log(np.array([1.0 - (1.0 - 5 / 8), 1.0 - (1.0 - (2 / 8) / (3 / 8)), 1.0]))).max() <= 1 and lq[2] == 0.0
    assert (a.tolist(), b.tolist()) == ([1.0, 1.0, 0.5], [1.0, 1.0, 0.25])
    with pytest.raises(AssertionError):
        ref_order(np.ones((2, 3), np.uint32), [1.0, 2.0], 0.25, 0.25, 6)      # (x 1, sf 1) and (x 0, sf 2) both have the code 0.5


def test_ref_order_gives_the_oracles_bins(orc, prob, ordered):
    """The one place the reference's own algorithm (np.unique on the code of every cell) enters: same (expr, mult, 1/sf, 1/sf^2)
    sequence for all ten pairs, bit for bit."""
    for p, (_, (bi, xi, mult, pk, lq, a, b)) in enumerate(ordered):
        x, sbin = pair_cells(prob, p)
        inv_sf, inv_sf_sq, expr, om = orc.unique_bins_1d(x.astype(np.float64), prob.sf_table[sbin], prob.r1[p], prob.r0[p])
        np.testing.assert_array_equal(expr, xi.astype(np.float64), err_msg=f"pair {p}")
        np.testing.assert_array_equal(om, mult, err_msg=f"pair {p}")
        np.testing.assert_array_equal(inv_sf, a, err_msg=f"pair {p}")
        np.testing.assert_array_equal(inv_sf_sq, b, err_msg=f"pair {p}")
        np.testing.assert_array_equal(1.0 / prob.sf_table[bi], a)
        assert mult.sum() == len(x)


@pytest.mark.parametrize("p", [2 * 2 + 1, 1 * 2 + 0], ids=["K=20", "K=11453"])
def test_ref_pk_reproduces_numpys_multinomial(orc, prob, ordered, p):
    """pk is the success probability numpy's random_multinomial hands to its binomial sampler: a hand-written chain of
    Generator(PCG64(5)).binomial(n_left, pk[k]) draws gives the weights of orc.multinomial_weights(N, mult, 8)."""
    _, (_, _, mult, pk, _, _, _) = ordered[p]
    K, N, B = len(mult), prob.sizes[p % 2], 8
    assert K == K_1905[p // 2][p % 2]
    want = orc.multinomial_weights(N, mult, B)
    gen = np.random.Generator(np.random.PCG64(5))
    got = np.zeros((K, B), dtype=np.int64)
    for b in range(B):
        left = N
        for k in range(K - 1):
            w = int(gen.binomial(left, pk[k]))
            got[k, b] = w
            left -= w
            if left <= 0:
                break
        if left > 0:
            got[K - 1, b] = left
    np.testing.assert_array_equal(got, want)
    assert (want.sum(axis=0) == N).all()


def test_replay_order_on_the_host_agrees_with_the_restatement(prob, ordered):
    """engine._replay_order (the arithmetic of Bootstrap1D._order_on_host) on the canonical bins of every pair: the order and pk
    bit for bit, lq within 2 ulp (the same log of the same argument)."""
    from scrna_parameter_estimation_amd.engine import _replay_order

    worst = 0
    for p, (t, (bi, xi, mult, pk, lq, a, b)) in enumerate(ordered):
        cb, cx = np.nonzero(t)
        code = cx.astype(np.float64) * prob.r1[p] + prob.r0[p] * prob.sf_table[cb]
        o, got_pk, got_lq = _replay_order(code, t[cb, cx], prob.sizes[p % 2])
        np.testing.assert_array_equal(cb[o], bi, err_msg=f"pair {p}")
        np.testing.assert_array_equal(cx[o], xi, err_msg=f"pair {p}")
        np.testing.assert_array_equal(got_pk.view(np.int64), pk.view(np.int64), err_msg=f"pair {p}")
        d = int(ulp_diff(got_lq, lq).max())
        worst = max(worst, d)
        assert d <= 2, (p, d)
        # the sequential remaining_p, once more as numpy's own left fold
        pix = mult.astype(np.float64) / prob.sizes[p % 2]
        rem = np.subtract.accumulate(np.concatenate([[1.0], pix]))[:-1]
        np.testing.assert_array_equal((pix / rem).view(np.int64), pk.view(np.int64))
    print(f"\nlargest lq difference: {worst} ulp")
    with pytest.raises(NotImplementedError):
        _replay_order(np.array([0.5, 0.25, 0.5]), np.array([1, 1, 1]), 3)


def test_ulp_diff():
    one = np.float64(1.0)
    assert ulp_diff([1.0, 0.0, -1.0, 1.0], [np.nextafter(one, 2), -0.0, np.nextafter(-one, -2), 1.0]).tolist() == [1, 0, 1, 0]
    assert ulp_diff([5e-324], [-5e-324]).tolist() == [2] and ulp_diff([np.nan], [1.0])[0] == 2 ** 63 - 1
