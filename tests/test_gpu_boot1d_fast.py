"""GPU tests of rng='fast' on the 1D path: the replicate-parallel kernel mm_boot1d_fast (one wave per 64 replicates of one
(gene, group) chain, every replicate on its own counter-derived PCG64 stream keyed by (seed, chain key, replicate)),
Bootstrap1D.run(fast=True, chain_keys=...), and ht_1d_moments / ht_1d_vs_control(rng='fast').

The kernel problem follows test_gpu_boot2d_fast: groups of 17,003 (three count blocks) / 8,192 / 300 / 6 cells plus ungrouped
cells, 150 genes, 30 size-factor bins, the 6-cell group in one size-factor bin (chains with K == 1), two highly expressed genes
(chains of several hundred bins), a never-expressed gene (one bin per occupied size-factor bin), a gene expressed in one group
only and a gene that is a copy of another (equal operands).  Replicate r of the chain with key k draws from the PCG64 stream
fast_state(fill_seed, k, r) of tests/_fast_ref.py, so the dumped weights of the really ingested chains are compared draw for draw
with numpy's own multinomial on that stream (part (e); the kernel on synthetic planes: tests/test_gpu_fast_draws.py).  Beside that
the kernel's arithmetic is checked against the oracle's formulas in extended precision on the kernel's OWN dumped weights, the
weights against the multinomial law (a guard of the statistics should the stream rule ever be changed on purpose), and the keys
against the promise that they -- not the rows, the chunks or the shards -- decide the numbers.
"""

import os
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

N_SF_BINS = 30
N_GENES = 150
H0, H1 = 5, 6           # highly expressed genes
NEVER = 3               # never expressed
ONE_GROUP = 7           # expressed in group 0 only
TWIN_A, TWIN_B = 50, 51  # gene 51 is a copy of gene 50
Q_GROUP = 0.07
SIZES = (17003, 8192, 300, 6)
SKIPPED = ((20, 0), (20, 1), (20, 2), (20, 3), (33, 1), (H1, 2))      # (gene, group) chains the caller skips
FIRST_GENE = 2          # first_pair = FIRST_GENE * n_groups: the rows of genes 0 and 1 are left alone
Z_GENES = [H0, 40, TWIN_A, TWIN_B, 60, NEVER]
Z_SEED = 11             # fill_seed of the multinomial test; numpy's own multinomial passes the same bounds with this seed (checked in the test)
KEY_GENES = [H0, 12, 13, NEVER, 40, 41, TWIN_A, TWIN_B, 90, 91, 92, 149]
U = 2.0 ** -53


def _problem(seed=2025):
    rng = np.random.default_rng(seed)
    ng = len(SIZES)
    gid = np.concatenate([np.full(s, g, dtype=np.int32) for g, s in enumerate(SIZES)] + [np.full(150, -1, dtype=np.int32)])
    rng.shuffle(gid)
    n = len(gid)
    X = rng.poisson(rng.uniform(0.05, 0.9, size=N_GENES) * rng.gamma(2.0, 0.5, size=(n, N_GENES))).astype(np.int64)
    X[:, H0] = rng.poisson(rng.gamma(3.0, 2.5, size=n))
    X[:, H1] = rng.poisson(rng.gamma(3.0, 2.0, size=n))
    X[:, NEVER] = 0
    X[gid != 0, ONE_GROUP] = 0
    X[:, TWIN_B] = X[:, TWIN_A]
    sf = rng.lognormal(0.0, 0.3, size=n)
    sf_bin = rng.integers(0, N_SF_BINS, size=n).astype(np.uint8)
    sf_bin[gid == ng - 1] = 4                                 # the 6-cell group sits in one size-factor bin: chains with K == 1
    return SimpleNamespace(X=X, csr=sp.csr_matrix(X.astype(np.float32)), gid=gid, ng=ng, sf=sf, sf_bin=sf_bin,
                           sf_table=np.linspace(0.4, 2.5, N_SF_BINS), sel=[np.flatnonzero(gid == g) for g in range(ng)],
                           grp_q=np.full(ng, Q_GROUP))


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import memento_oracle

    return memento_oracle


@pytest.fixture(scope="module")
def prob():
    return _problem()


@pytest.fixture(scope="module")
def dev_blocks(eng, prob):
    blocks = eng.CountBlocks(eng.DeviceCSR(prob.csr), prob.gid, prob.ng)
    _, _, maxx = blocks.moments(1.0 / prob.sf)
    return blocks, maxx


def _uniforms(prob):
    """The two hash uniforms of every (gene, group) chain of the problem, [N_GENES][ng] each; the copied gene gets its original's."""
    u = np.random.default_rng(79).random((2, N_GENES, prob.ng))
    u[:, TWIN_B] = u[:, TWIN_A]
    return u


def _boot(eng, prob, dev_blocks, genes, B, pad=0):
    """Bootstrap1D of a gene list (histograms and bin counts done) with its outputs allocated -- column 0 holds a recognisable value
    per row, ``pad`` extra columns lie behind the B replicate columns -- and the chains' hash uniforms."""
    blocks, maxx = dev_blocks
    genes = np.asarray(genes, dtype=np.int64)
    bs = eng.Bootstrap1D(blocks, genes, maxx, prob.sf_bin, prob.sf_table, prob.grp_q, B)
    bs.ld = B + 1 + pad
    col0 = 1000.0 + np.arange(bs.n_pairs)
    bs.alloc_outputs(col0, -col0)
    u = _uniforms(prob)
    return SimpleNamespace(bs=bs, genes=genes, B=B, col0=col0, r1=u[0][genes].reshape(-1), r0=u[1][genes].reshape(-1))


def _run(bt, skip=None, **kw):
    bs = bt.bs
    skip = np.zeros(bs.n_pairs, dtype=bool) if skip is None else skip
    kw.setdefault("fill_seed", 3)
    return bs.run(skip, bt.r1, bt.r0, (0.0, 1.0, 0.0), fill_mode=1, fast=True, dump_weights=True, **kw)


def _chain_bins(eng, orc, prob, bt, p):
    """Chain p's bins in replay order, from the oracle and -- asserted equal row for row -- from the device's histogram:
    (1/sf, 1/sf^2, expr, multiplicity), the chain probabilities pk of the draws, and the group's cell count."""
    gi, g = divmod(int(p), prob.ng)
    sel = prob.sel[g]
    vals, sf = prob.X[sel, bt.genes[gi]].astype(np.float64), prob.sf_table[prob.sf_bin[sel]]
    a, b, e, mult = orc.unique_bins_1d(vals, sf, bt.r1[p], bt.r0[p])
    bi, xi, mu = bt.bs.bins_of_pair(p)
    o, pk, _ = eng._replay_order(xi.astype(np.float64) * bt.r1[p] + bt.r0[p] * prob.sf_table[bi], mu, len(sel))
    assert len(e) == len(o) == int(bt.bs.K[p])
    np.testing.assert_array_equal(e, xi[o].astype(np.float64))
    np.testing.assert_array_equal(a, 1.0 / prob.sf_table[bi[o]])
    np.testing.assert_array_equal(mult, mu[o])
    return (a, b, e, mult), pk, len(sel)


# ------------------------------------------------------------------------------------------------------------------------
# (a) the kernel's arithmetic is exact given its own weights
# ------------------------------------------------------------------------------------------------------------------------


def _moments_longdouble(e, a, b, w, n, q):
    """oracle.replicate_moments_1d (estimator.py:171-174, :182-183) in np.longdouble: (mean, M2 / n, var) per replicate."""
    L = np.longdouble
    e, a, b, w = (x.astype(L).reshape(-1, 1) for x in (e, a, b, w.astype(np.float64)))
    w = w.reshape(len(e), -1)
    m1 = (e * w * a).sum(axis=0) / L(n)
    m2 = (e ** 2 * w * b - (L(1) - L(q)) * e * w * b).sum(axis=0) / L(n)
    return m1, m2, m2 - m1 ** 2


@pytest.mark.parametrize("mean_only", [0, 1])
@pytest.mark.parametrize("B", [130, 64, 1])
def test_replicates_are_the_oracles_formulas_on_the_dumped_weights(eng, orc, prob, dev_blocks, B, mean_only):
    """Bootstrap1D.run(fast=True, dump_weights=True, fill_mode=1) over all 150 genes at B = 130 (two full 64-replicate chunks and a
    ragged one of 2), 64 (exactly one chunk) and 1 (one lane), mean_only 0 and 1.  For every active chain: the dumped columns are
    non-negative and sum to the group's cell count; the bins are the oracle's, in its order; raw_mean / raw_var equal
    oracle.replicate_moments_1d evaluated in np.longdouble on those weights.  Tolerance (derived, not measured): both sums add K
    non-negative terms sequentially in fp64, so mean: relative error <= (K + 8) 2^-53, var: absolute error <=
    (K + 8) 2^-53 (M2 / n + mean^2).  mean_only: mean + 1 at the same bound, var exactly 10.  Rows with K < 2, skipped rows and
    rows below first_pair are NaN beyond column 0, column 0 and the padding columns behind the replicates are untouched.  The
    draws of the checked chains lie on both sides of numpy's inversion / BTPE switch (n min(p, 1 - p) = 30), some with pk > 0.5."""
    pad = 3
    bt = _boot(eng, prob, dev_blocks, np.arange(N_GENES), B, pad=pad)
    bs, ng = bt.bs, prob.ng
    skip = np.zeros(bs.n_pairs, dtype=bool)
    for gene, g in SKIPPED:
        skip[gene * ng + g] = True
    first = FIRST_GENE * ng
    _run(bt, skip, mean_only=bool(mean_only), first_pair=first)
    active = ~skip & (bs.K >= 2)
    active[:first] = False
    np.testing.assert_array_equal(bs.active, active)
    rm, rv = eng.host(bs.raw_mean), eng.host(bs.raw_var)
    assert rm.shape == rv.shape == (bs.n_pairs, B + 1 + pad) and bs.n_tiles >= 2
    np.testing.assert_array_equal(rm[:, 0], bt.col0)
    np.testing.assert_array_equal(rv[:, 0], -bt.col0)
    assert np.isnan(rm[:, B + 1:]).all() and np.isnan(rv[:, B + 1:]).all()          # the padding columns were never written
    assert np.isnan(rm[~active, 1:]).all() and np.isnan(rv[~active, 1:]).all()
    assert np.isfinite(rm[active, 1:B + 1]).all() and np.isfinite(rv[active, 1:B + 1]).all()
    k1 = np.flatnonzero(~skip & (bs.K == 1) & (np.arange(bs.n_pairs) >= first))
    assert len(k1) >= 1 and (k1 % ng == ng - 1).all() and NEVER * ng + ng - 1 in k1 and skip.sum() == len(SKIPPED)
    assert bs.K[NEVER * ng] == N_SF_BINS and bs.K[ONE_GROUP * ng + 1] == N_SF_BINS and bs.K[ONE_GROUP * ng] > N_SF_BINS
    assert bs.K[H0 * ng] >= 300 and bs.K[H1 * ng] >= 300 and (bs.K[:first] >= 2).any()
    n_inv = n_btpe = n_flip = 0
    worst_m = worst_v = 0.0
    for p in np.flatnonzero(active):
        (a, b, e, mult), pk, n = _chain_bins(eng, orc, prob, bt, p)
        K = int(bs.K[p])
        w = bs.weights_of(p)
        assert w.shape == (K, B) and w.dtype == np.int32
        assert (w >= 0).all() and (w.sum(axis=0) == n).all(), p
        remaining = n - (np.cumsum(w, axis=0) - w)[:-1]             # cells left before each of the K - 1 draws, per replicate
        drawn = remaining > 0
        npq = remaining * np.minimum(pk[:-1], 1.0 - pk[:-1])[:, None]
        n_inv += int((drawn & (npq <= 30)).sum())
        n_btpe += int((drawn & (npq > 30)).sum())
        n_flip += int((drawn & (pk[:-1] > 0.5)[:, None]).sum())
        m1, m2, var = _moments_longdouble(e, a, b, w, n, Q_GROUP)
        tol = (K + 8) * U
        err_m = np.abs(rm[p, 1:B + 1].astype(np.longdouble) - (m1 + mean_only))
        assert (err_m <= tol * (m1 + mean_only)).all(), f"chain {p} (K = {K}, {n} cells): mean off by {float(err_m.max()):.3e}"
        worst_m = max(worst_m, float((err_m / np.maximum(tol * (m1 + mean_only), np.finfo(np.longdouble).tiny)).max()))
        if mean_only:
            assert (rv[p, 1:B + 1] == 10.0).all()
        else:
            err_v = np.abs(rv[p, 1:B + 1].astype(np.longdouble) - var)
            bound = tol * (m2 + m1 ** 2)
            assert (err_v <= bound).all(), f"chain {p} (K = {K}, {n} cells): var off by {float(err_v.max()):.3e}, bound {float(bound.min()):.3e}"
            worst_v = max(worst_v, float((err_v / np.maximum(bound, np.finfo(np.longdouble).tiny)).max()))
    print(f"\nB = {B}, mean_only = {mean_only}: {int(active.sum())} chains in {bs.n_tiles} tiles, {len(k1)} with K == 1; draws: {n_inv} "
          f"inversion, {n_btpe} BTPE, {n_flip} with pk > 0.5; worst error / bound: mean {worst_m:.3f}, var {worst_v:.3f}")
    assert n_inv > 0 and n_btpe > 0 and n_flip > 0


# ------------------------------------------------------------------------------------------------------------------------
# (b) the weights are multinomial and the streams are distinct
# ------------------------------------------------------------------------------------------------------------------------


def _z_mean(mean_w, p, n, B):
    return float(np.abs((mean_w - n * p) / np.sqrt(n * p * (1 - p) / B)).max())


def _z_var(var_w, p, n, B):
    """|s^2 - n p (1 - p)| in standard errors of the unbiased sample variance of B binomial(n, p) draws, over the bins with n p >= 5
    (Var s^2 = (mu_4 - sigma^4 (B - 3) / (B - 1)) / B with the binomial's mu_4 = sigma^2 (1 + 3 (n - 2) p (1 - p)))."""
    ok = n * p >= 5
    p, s2 = p[ok], n * p[ok] * (1 - p[ok])
    mu4 = s2 * (1 + 3 * (n - 2) * p * (1 - p))
    se = np.sqrt((mu4 - s2 ** 2 * (B - 3) / (B - 1)) / B)
    return float(np.abs((var_w[ok] - s2) / se).max()) if ok.any() else 0.0


def test_weights_are_multinomial_and_streams_distinct(eng, orc, prob, dev_blocks):
    """B = 2,048, fill_seed = Z_SEED, the genes Z_GENES.  For every bin of every chain with n >= 300 cells z = (mean_r w_k - n p_k) /
    sqrt(n p_k (1 - p_k) / B) has max |z| < 5: with the few thousand bins here a correct sampler misses that by chance less than
    once in 1e2 seeds (2 Phi(-5) = 5.7e-7 per bin); for the bins with n p_k >= 5 the variance of w_k over the replicates lies within
    5 standard errors of n p_k (1 - p_k).  numpy's own multinomial with the same seed on the same chains is held to both bounds
    first, on the host.  Within a chain of K >= 50 no two replicate columns are equal (neighbouring lanes and the same lane in
    different 64-chunks included); the gene and its copy -- equal operands, different keys -- share no column; a second run with
    the same seed and keys is bit-identical; another fill_seed changes every chain of K >= 50."""
    B = 2048
    bt = _boot(eng, prob, dev_blocks, Z_GENES, B)
    bs, ng = bt.bs, prob.ng
    chains = [p for p in range(bs.n_pairs) if SIZES[p % ng] >= 300]
    assert all(bs.K[p] >= 2 for p in chains) and len(chains) == 3 * len(Z_GENES)
    bins = {p: _chain_bins(eng, orc, prob, bt, p)[0][3] for p in chains}
    n_bins = sum(len(m) for m in bins.values())
    gen = np.random.Generator(np.random.PCG64(Z_SEED))
    zm_numpy = zv_numpy = 0.0
    for p in chains:
        n = SIZES[p % ng]
        w = gen.multinomial(n, bins[p] / n, size=B)
        zm_numpy = max(zm_numpy, _z_mean(w.mean(axis=0), bins[p] / n, n, B))
        zv_numpy = max(zv_numpy, _z_var(w.var(axis=0, ddof=1), bins[p] / n, n, B))
    assert zm_numpy < 5 and zv_numpy < 5 and 2000 < n_bins < 6000, (zm_numpy, zv_numpy, n_bins)
    _run(bt, fill_seed=Z_SEED)
    proj = np.random.default_rng(1).integers(1, 1 << 30, size=int(bs.K.max()), dtype=np.int64)
    zm = zv = 0.0
    n_long, W = 0, {}
    for p in chains:
        w = W[p] = bs.weights_of(p)
        n, K = SIZES[p % ng], int(bs.K[p])
        assert w.shape == (K, B) and (w.sum(axis=0) == n).all() and (w >= 0).all()
        zm = max(zm, _z_mean(w.mean(axis=1), bins[p] / n, n, B))
        zv = max(zv, _z_var(w.var(axis=1, ddof=1), bins[p] / n, n, B))
        if K >= 50:
            h = proj[:K] @ w.astype(np.int64)                      # equal columns have equal projections
            if len(np.unique(h)) < B:
                assert len(np.unique(w.T, axis=0)) == B, f"chain {p}: two replicates drew the same weights"
            n_long += 1
    print(f"\n{len(chains)} chains, {n_bins} bins, B = {B}: max |z| of the means {zm:.3f} (numpy's multinomial, seed {Z_SEED}: {zm_numpy:.3f}), "
          f"of the variances {zv:.3f} (numpy: {zv_numpy:.3f}); {n_long} chains with K >= 50")
    assert n_long >= 8
    ia, ib = Z_GENES.index(TWIN_A), Z_GENES.index(TWIN_B)
    for g in range(3):
        pa, pb = ia * ng + g, ib * ng + g
        np.testing.assert_array_equal(bins[pa], bins[pb])           # equal operands: same bins in the same order
        assert bs.K[pa] >= 50 and (W[pa] != W[pb]).any(axis=0).all(), (pa, pb)
    first = bs.w_dump.clone(), eng.host(bs.raw_mean), eng.host(bs.raw_var), bs.tile_slot.copy()
    _run(bt, fill_seed=Z_SEED)
    np.testing.assert_array_equal(bs.tile_slot, first[3])
    assert eng._torch().equal(bs.w_dump, first[0])
    np.testing.assert_array_equal(eng.host(bs.raw_mean), first[1])
    np.testing.assert_array_equal(eng.host(bs.raw_var), first[2])
    assert np.isfinite(first[1][chains, 1:]).all() and (first[1][chains, 1:] > 0).sum() > B
    _run(bt, fill_seed=Z_SEED + 1)
    for p in chains:
        if bs.K[p] >= 50:
            assert (bs.weights_of(p) != W[p]).any(axis=0).all(), f"chain {p}: another seed, the same weights"
    assert zm < 5 and zv < 5, (zm, zv)


# ------------------------------------------------------------------------------------------------------------------------
# (c) keys, not rows, decide the numbers
# ------------------------------------------------------------------------------------------------------------------------


def test_chain_keys_not_rows_decide_the_numbers(eng, prob, dev_blocks):
    """The chains of KEY_GENES as one Bootstrap1D and as two Bootstrap1D over the two halves of the gene list, chain_keys numbering
    the chains over the whole list: dumped weights, raw_mean and raw_var are bit-identical chain for chain.  With the default keys
    (the row number) the first half is still the whole run's -- its rows are its keys -- and every chain of the second half with
    K >= 50 differs in every replicate."""
    B, ng = 130, prob.ng
    whole = _boot(eng, prob, dev_blocks, KEY_GENES, B)
    _run(whole)
    n = whole.bs.n_pairs
    want_w = [whole.bs.weights_of(p) if whole.bs.K[p] >= 2 else None for p in range(n)]
    want_m, want_v = eng.host(whole.bs.raw_mean), eng.host(whole.bs.raw_var)
    half = len(KEY_GENES) // 2
    assert (whole.bs.K >= 50).sum() >= 6 and (whole.bs.K == 1).sum() >= 1
    for keyed in (True, False):
        n_diff = 0
        for lo, hi in ((0, half), (half, len(KEY_GENES))):
            part = _boot(eng, prob, dev_blocks, KEY_GENES[lo:hi], B)
            rows = np.arange(lo * ng, hi * ng)
            np.testing.assert_array_equal(part.bs.K, whole.bs.K[rows])
            _run(part, chain_keys=rows if keyed else None)
            got_m, got_v = eng.host(part.bs.raw_mean), eng.host(part.bs.raw_var)
            same = keyed or lo == 0
            if same:
                np.testing.assert_array_equal(got_m[:, 1:], want_m[rows, 1:])
                np.testing.assert_array_equal(got_v[:, 1:], want_v[rows, 1:])
            for i, p in enumerate(rows):
                if part.bs.K[i] < 2:
                    continue
                w = part.bs.weights_of(i)
                if same:
                    np.testing.assert_array_equal(w, want_w[p], err_msg=f"chain {p}")
                elif part.bs.K[i] >= 50:
                    assert (w != want_w[p]).any(axis=0).all(), f"chain {p}: row-keyed streams in another chunk, the same weights"
                    assert (got_m[i, 1:] != want_m[p, 1:]).any()
                    n_diff += 1
        assert keyed or n_diff >= 3
    with pytest.raises(ValueError):
        _run(whole, chain_keys=np.arange(n - 1))


# ------------------------------------------------------------------------------------------------------------------------
# (e) the engine's weights are numpy's, draw for draw, on the stated streams
# ------------------------------------------------------------------------------------------------------------------------


def test_engine_weights_are_numpys_on_the_stated_streams(eng, orc, prob, dev_blocks):
    """Bootstrap1D.run(fast=True, dump_weights=True) on the chains of KEY_GENES, B = 130, with the default keys (the row numbers)
    under fill_seed 3 and with chain_keys (2^40 and a negative key among them) under fill_seed 0xDEADBEEF12345678: weights_of(p)
    of EVERY active chain equals fast_weights(bins of p in replay order, fill_seed, key of p, arange(B)).  Then launch_range on
    [64, 134) and on the last 70 replicates below 2^31 - 1, a third of the chains closed: w_dump_range equals fast_weights on
    rep_lo + arange(rep_n), and the closed chains dump nothing."""
    from _fast_ref import fast_weights

    torch = eng._torch()
    B, ng = 130, prob.ng
    bt = _boot(eng, prob, dev_blocks, KEY_GENES, B)
    bs = bt.bs
    n = bs.n_pairs
    custom = 7000 + 11 * np.arange(n, dtype=np.int64)
    custom[0], custom[1], custom[2] = 2 ** 40, -3, 0
    bins, checked = {}, 0
    for keys, seed in ((None, 3), (custom, 0xDEADBEEF12345678)):
        _run(bt, fill_seed=seed, chain_keys=keys)
        key_of = np.arange(n) if keys is None else keys
        act = np.flatnonzero(bs.active)
        assert len(act) >= 30 and (bs.K[act] >= 50).sum() >= 6 and {0, 1, 2} <= set(act.tolist())
        for p in act:
            if p not in bins:
                bins[p] = _chain_bins(eng, orc, prob, bt, p)[0][3].astype(np.int64)
            np.testing.assert_array_equal(bs.weights_of(p), fast_weights(bins[p], seed, int(key_of[p]), np.arange(B)),
                                          err_msg=f"chain {p} (K = {bs.K[p]}), key {key_of[p]}, seed {seed:#x}")
            checked += bins[p].size * B
    closed = np.arange(n) % 3 == 1
    open_pairs = np.flatnonzero(~closed)
    for rep_lo, rep_n in ((64, 70), (2 ** 31 - 1 - 70, 70)):
        planes = [torch.full((n, rep_n + 1), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
        keep = bs.launch_range(rep_lo, rep_n, open_pairs, planes, open_pairs, dump_weights=True)
        wr = eng.host(bs.w_dump_range)
        del keep
        for p in np.flatnonzero(bs.active):
            K, slot = int(bs.K[p]), int(bs.tile_slot[p])
            if closed[p]:
                assert (wr[slot] == 0).all(), p
                continue
            want = fast_weights(bins[p], seed, int(custom[p]), rep_lo + np.arange(rep_n))
            np.testing.assert_array_equal(wr[slot, :K], want, err_msg=f"chain {p}, replicates from {rep_lo}")
            if rep_lo == 64:
                np.testing.assert_array_equal(want[:, :B - 64], bs.weights_of(p)[:, 64:])
            checked += want.size
    print(f"\n{checked} weights of really ingested chains equal numpy's on the fast streams")


# ------------------------------------------------------------------------------------------------------------------------
# (d) the API: gene chunking changes no number
# ------------------------------------------------------------------------------------------------------------------------


def test_ht_1d_moments_fast_is_chunk_invariant(api_small):
    """ht_1d_moments(rng='fast', fill_seed=7, approx=True) on api_small with max_rows=None (one chunk) and max_rows=40 (several):
    coefficients, standard errors and p-values are bit-identical, NaN pattern included."""
    from test_gpu_api import _design, _run_to_moments

    memento, adata = _run_to_moments(api_small)
    cov, trt = _design(memento, adata, api_small)
    m = adata.uns["memento"]
    ng, G = len(m["groups"]), len(m["_hip"].gene_idx)
    assert G * ng > 3 * 40                                          # max_rows = 40 makes more than three chunks
    res = []
    for max_rows in (None, 40):
        np.random.seed(int(api_small["ht_seed"]))
        memento.ht_1d_moments(adata, covariate=cov, treatment=trt, num_boot=int(api_small["num_boot"]), num_cpus=1, verbose=0,
                              resampling="bootstrap", approx=True, rng="fast", fill_seed=7, max_rows=max_rows)
        res.append({k: np.asarray(m["1d_ht"][k]).copy() for k in ("mean_coef", "mean_se", "mean_asl", "var_coef", "var_se", "var_asl")})
        assert (m["_hip"].last_bootstrap.n_pairs == G * ng) == (max_rows is None)     # one chunk, then several
    assert np.isfinite(res[0]["mean_se"]).sum() > G // 2
    for k in res[0]:
        np.testing.assert_array_equal(res[0][k], res[1][k], err_msg=k)


@pytest.mark.parametrize("rng", ["replay", "fast"])
def test_ht_1d_vs_control_is_chunk_invariant(guide_loop, rng):
    """ht_1d_vs_control on the guide_loop fixture's inputs (6,000 cells x 150 genes, 5 guides + control), in one gene chunk and in
    chunks of 17 genes, in both rng modes: every result column -- de_se, dv_se and the p-values included, which depend on the
    bootstrap streams (rng='fast') and on the device refill streams (both modes) -- is bit-identical."""
    from scrna_parameter_estimation_amd import AnnDataLite, memento

    g = guide_loop
    X = sp.csr_matrix((g["in_data"].astype(np.float32), g["in_indices"], g["in_indptr"]), shape=tuple(g["in_shape"]))
    obs = pd.DataFrame({"guide": g["in_guide"], "q": g["in_q"]}, index=[f"c{i}" for i in range(X.shape[0])])
    adata = AnnDataLite(X, obs, pd.DataFrame(index=g["in_gene_names"].tolist()))
    memento.setup_memento(adata, q_column="q")
    memento.create_groups(adata, label_columns=["guide"])
    memento.compute_1d_moments(adata, min_perc_group=0.9)
    m = adata.uns["memento"]
    st, ng = m["_hip"], len(m["groups"])
    ctrl = [k for k in m["groups"] if k.split("^")[-1] == "0"][0]
    res = []
    for max_rows in (None, ng * 17):
        np.random.seed(5)
        res.append(memento.ht_1d_vs_control(adata, control=ctrl, num_boot=300, num_cpus=1, approx=True, rng=rng, fill_seed=4, max_rows=max_rows))
        assert (st.last_chunk[0] > 0) == (max_rows is not None)     # one chunk, then several
    one, many = res
    assert (one["gene"].values == many["gene"].values).all() and (one["group"].values == many["group"].values).all()
    assert np.isfinite(one["de_se"].values).sum() > len(one) // 4 and np.isfinite(one["dv_pval"].values).sum() > 0
    for k in ("de_coef", "de_se", "de_pval", "dv_coef", "dv_se", "dv_pval"):
        np.testing.assert_array_equal(one[k].values, many[k].values, err_msg=k)
