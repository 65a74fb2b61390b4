"""GPU parity tests of the gene-pair (2D) kernels, one by one, against plain host references in fp64 or higher:
mm_extract_cols, mm_pair_cross, mm_pair_hist / mm_pair_bins_count, mm_bins_order2d (small kernel, big kernel, host fallback),
mm_boot2d_replay / mm_boot2d_replay_rec (both tile regimes), the replay-hash collision report, and the CSR column kernels.

One test problem carries every edge (``_problem``): a group of three count blocks, one of exactly 8,192 cells, one of 300 and
one of 6 cells, cells outside every group; G = 150 genes (a ragged last slice) with three highly expressed genes (one count
of 300), a gene that is never expressed, one expressed in one group only, one silent in the middle block of the large group.
The pair list (``_pair_list``) holds a left gene with 11 partners, one with a single partner, self pairs, (i, j) and (j, i),
a duplicated pair, the pair of the two highly expressed genes and pairs with the empty genes on either side, plus enough
ordinary pairs for more than 2,048 chains.

Integer results (columns, histograms, bin counts, CSR splits) must be bit-exact; pair sums within the rounding bound of the
kernel's longest summation path; replicate correlations at the tolerance of the existing full-size 2D spot check.  The
host-only test at the end checks the module's own reference helpers against the oracle where there is no device.
"""

import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

gpu = pytest.mark.gpu

BLOCK = 8192
N_SF_BINS = 30
N_GENES = 150           # slices of 64, 64 and 22 genes
H0, H1, H2 = 0, 1, 2    # highly expressed genes (H1 carries the single count of 300)
NEVER = 3               # never expressed
BLK_SILENT = 5          # silent in block 1 of group 0, present in blocks 0 and 2
ONE_GROUP = 7           # expressed in group 0 only
MANY = 10               # left gene with 11 partners (two passes of the 8-waves partner loop)
LONE = 20               # left gene with exactly one partner
Q_GROUP = 0.07
SMALL_K, BIG_K = 1024, 4096      # the K ranges of mm_bins_order2d: small kernel / big kernel / host


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import memento_oracle

    return memento_oracle


# ------------------------------------------------------------------------------------------------------------------------
# the test problem and the host references
# ------------------------------------------------------------------------------------------------------------------------


def _plan(gid, ng, block):
    """Count blocks as the ingest cuts them: cells of a group in ascending original order, in ceil(n / block) near-equal
    blocks.  List of (group, original cell indices in block order)."""
    out = []
    for g in range(ng):
        cells = np.flatnonzero(gid == g)
        n = len(cells)
        nb = -(-n // block)
        out += [(g, cells[n * k // nb:n * (k + 1) // nb]) for k in range(nb)]
    return out


def _problem(sizes=(17003, 8192, 300, 6), n_out=150, block=BLOCK, seed=2024):
    rng = np.random.default_rng(seed)
    ng = len(sizes)
    gid = np.concatenate([np.full(s, g, dtype=np.int32) for g, s in enumerate(sizes)] + [np.full(n_out, -1, dtype=np.int32)])
    rng.shuffle(gid)
    n = len(gid)
    # ordinary genes: sparse and overdispersed (a Poisson gene's residual variance is zero up to noise, and its chains would be skipped)
    X = rng.poisson(rng.uniform(0.05, 0.9, size=N_GENES) * rng.gamma(2.0, 0.5, size=(n, N_GENES))).astype(np.int64)
    X[:, H0] = rng.poisson(rng.gamma(3.0, 2.5, size=n))       # mean 7.5, overdispersed: columns of thousands of entries per block
    X[:, H1] = rng.poisson(rng.gamma(3.0, 2.0, size=n))       # mean 6
    X[:, H2] = rng.poisson(rng.gamma(5.0, 1.1, size=n))       # mean 5.5
    X[np.flatnonzero(gid == 0)[11], H1] = 300                 # the one large count (xcap 301 in group 0)
    X[:, NEVER] = 0
    X[gid != 0, ONE_GROUP] = 0
    plan = _plan(gid, ng, block)
    assert [g for g, _ in plan[:3]] == [0, 0, 0] and plan[3][0] == 1, "group 0 must span exactly three blocks"
    X[plan[1][1], BLK_SILENT] = 0
    sf = rng.lognormal(0.0, 0.3, size=n)
    sf_bin = rng.integers(0, N_SF_BINS, size=n).astype(np.uint8)
    sf_bin[gid == ng - 1] = 4                                 # the 6-cell group sits in one size-factor bin: chains with K == 1
    sf_table = np.linspace(0.4, 2.5, N_SF_BINS)
    return SimpleNamespace(X=X, csr=sp.csr_matrix(X.astype(np.float32)), gid=gid, ng=ng, sizes=sizes, plan=plan, sf=sf,
                           sf_bin=sf_bin, sf_table=sf_table, sel=[np.flatnonzero(gid == g) for g in range(ng)],
                           grp_q=np.full(ng, Q_GROUP))


SPECIAL_PAIRS = [(H0, H1), (H1, H0), (H0, H0), (H0, H2), (H2, H0), (H2, H2), (H0, 70), (H2, 71), (30, 30), (40, 41), (41, 40),
                 (50, 51), (50, 51), (LONE, 21), (NEVER, 60), (60, NEVER), (NEVER, NEVER), (BLK_SILENT, 61), (61, BLK_SILENT),
                 (ONE_GROUP, 62), (62, ONE_GROUP), (63, 64), (127, 128), (N_GENES - 1, 65)] \
    + [(MANY, j) for j in list(range(100, 110)) + [N_GENES - 1]]


def _pair_list():
    """Special pairs first (see the module docstring), then ordinary sparse pairs (more than 2,048 live chains: asserted where it matters)."""
    fill = [(i, j) for i in range(80, 140) for j in range(i + 1, i + 15) if j < N_GENES]
    pairs = np.array(SPECIAL_PAIRS + fill, dtype=np.int64)
    assert (pairs[:, 0] == LONE).sum() == 1 and (pairs[:, 0] == MANY).sum() == 11
    return pairs[:, 0], pairs[:, 1]


def _ref_column(X, cells, gene):
    """(cell_local, count) of the non-zero entries of ``gene`` among a block's cells, cell_local ascending."""
    col = X[cells, gene]
    loc = np.flatnonzero(col)
    return loc, col[loc]


def _ref_cross(X, inv_sf, cells, c1, c2, chunk=64):
    """sum_c x_ci x_cj inv_sf_c^2 over ``cells`` for the pairs (c1, c2), in np.longdouble: integer products are exact, every
    other operation rounds at 2^-64, and the terms are summed pairwise (contiguous rows)."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble must be wider than fp64 for this reference"
    w2 = inv_sf[cells].astype(np.longdouble) ** 2
    Xg = X[cells]
    out = np.empty(len(c1), dtype=np.longdouble)
    for s in range(0, len(c1), chunk):
        terms = (Xg[:, c1[s:s + chunk]] * Xg[:, c2[s:s + chunk]]).astype(np.longdouble) * w2[:, None]
        out[s:s + chunk] = np.ascontiguousarray(terms.T).sum(axis=1)
    return out


def _ref_bins(xi, xj, sbin):
    """The (sf_bin, x_i, x_j) bins of one (pair, group): rows in ascending (sf_bin, x_i, x_j) order and their multiplicities."""
    rows, mult = np.unique(np.stack([sbin.astype(np.int64), xi, xj], axis=1), axis=0, return_counts=True)
    return rows, mult


def _ref_table(xi, xj, sbin):
    """Dense [sf_bin][x_i][x_j] cell counts of one (pair, group), the layout of Bootstrap2D's tables."""
    t = np.zeros((N_SF_BINS, int(xi.max()) + 1, int(xj.max()) + 1), dtype=np.uint32)
    np.add.at(t, (sbin.astype(np.int64), xi, xj), 1)
    return t


def _k_range(K):
    """0 / 1 / 2: ordered by the small in-LDS kernel, the big one, or on the host (engine defaults)."""
    return (np.asarray(K) > SMALL_K).astype(int) + (np.asarray(K) > BIG_K).astype(int)


def _true_corr_and_skip(orc, prob, c1, c2):
    """Column 0 of the replicate rows and the chains the API would skip (true correlation NaN or +-1), [pair][group]."""
    X64 = sp.csc_matrix(prob.X.astype(np.float64))
    tc = np.empty((len(c1), prob.ng))
    for g, sel in enumerate(prob.sel):
        Xg = X64[sel]
        cov = orc.cov_2d_sparse(Xg, prob.sf[sel], Q_GROUP, c1, c2)
        _, var = orc.moments_1d_sparse(Xg, prob.sf[sel], Q_GROUP)
        tc[:, g] = orc.corr_from_cov(cov, var[c1], var[c2])
    return tc, np.abs(tc) == 1


# ------------------------------------------------------------------------------------------------------------------------
# fixtures on the device
# ------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prob():
    return _problem()


@pytest.fixture(scope="module")
def dev_cols(eng, prob):
    """The ranged ingest of the test problem and every gene's column."""
    blocks = eng.CountBlocks(eng.DeviceCSR(prob.csr), prob.gid, prob.ng)
    assert blocks.ranged
    return blocks, eng.GeneColumns(blocks, np.arange(N_GENES))


@pytest.fixture(scope="module")
def boot(eng, orc, prob, dev_cols):
    """Bootstrap2D of the whole pair list (histograms and bin counts done, nothing replayed yet) with its hash uniforms."""
    blocks, cols = dev_cols
    c1, c2 = _pair_list()
    _, _, maxx = blocks.moments(1.0 / prob.sf)
    B = 48
    bs = eng.Bootstrap2D(cols, c1, c2, maxx, prob.sf_bin, prob.sf_table, prob.grp_q, B)
    tc, skip = _true_corr_and_skip(orc, prob, c1[bs.order], c2[bs.order])
    for pair in SPECIAL_PAIRS:       # left live on purpose: self pairs, the 6-cell group, (60, NEVER) -- the kernel itself meets the zero variances
        if pair not in ((NEVER, 60), (ONE_GROUP, 62), (62, ONE_GROUP)):
            skip[(c1[bs.order] == pair[0]) & (c2[bs.order] == pair[1])] = False
    u = np.random.default_rng(77).random((3, bs.n_q))
    return SimpleNamespace(bs=bs, c1=c1[bs.order], c2=c2[bs.order], B=B, true_corr=tc.reshape(-1), skip=skip.reshape(-1), ra=u[0], rb=u[1],
                           r0=u[2])


def _run(eng, monkeypatch, bt, small_cap=SMALL_K, big_cap=BIG_K, records=True, many_tiles=False):
    """One Bootstrap2D.run with every switch set explicitly -> (yc on the host, what ran)."""
    monkeypatch.setattr(eng, "ORDER_SMALL_CAP", small_cap)
    monkeypatch.setattr(eng, "ORDER_BIG_CAP_2D", big_cap)
    monkeypatch.setattr(eng, "BOOT2D_RECORDS", records)
    monkeypatch.setattr(eng, "PACK_MAX_RESIDENT", 10 ** 9 if many_tiles else 2048)      # many_tiles: one chain per tile
    bt.bs.run(bt.skip, bt.ra, bt.rb, bt.r0, bt.true_corr, target_waves=10 ** 7 if many_tiles else None)
    return eng.host(bt.bs.yc).copy(), dict(bt.bs.order_path, kernel=bt.bs.replay_kernel, n_tiles=bt.bs.n_tiles)


def _pair_cells(prob, bt, q):
    """Dense per-cell counts of both genes and the size-factor bins of chain q = sorted_pair * n_groups + group."""
    p, g = divmod(int(q), prob.ng)
    sel = prob.sel[g]
    return prob.X[sel, bt.c1[p]], prob.X[sel, bt.c2[p]], prob.sf_bin[sel]


def _special_chains(prob, bt):
    """Every chain of every special pair, and 40 chains of ordinary pairs."""
    is_special = np.zeros(len(bt.c1), dtype=bool)
    for a, b in SPECIAL_PAIRS:
        is_special |= (bt.c1 == a) & (bt.c2 == b)
    ps = np.concatenate([np.flatnonzero(is_special), np.flatnonzero(~is_special)[::73][:10]])
    return (ps[:, None] * prob.ng + np.arange(prob.ng)[None, :]).reshape(-1)


# ------------------------------------------------------------------------------------------------------------------------
# 1. column extraction
# ------------------------------------------------------------------------------------------------------------------------


def _check_columns(eng, prob, blocks, cols, ordered):
    """Every (block, column) of ``cols`` against the host decoder.  Returns whether cell_local ascends in every column."""
    ptr = eng.host(cols.col_ptr)
    data = eng.host(cols.cols, np.uint32)
    assert blocks.n_blocks == len(prob.plan)
    ascending, longest = True, 0
    for b, (g, cells) in enumerate(prob.plan):
        assert blocks.blk_group[b] == g
        np.testing.assert_array_equal(blocks.cell_order[blocks.blk_cell0[b]:blocks.blk_cell0[b + 1]], cells)
        for m, gene in enumerate(cols.genes):
            e = data[ptr[b, m]:ptr[b, m + 1]]
            loc, cnt = _ref_column(prob.X, cells, gene)
            assert len(e) == blocks.blk_cnt[b, gene] == len(loc), (b, gene)
            assert (e != 0).all(), (b, gene)
            got_loc, got_cnt = (e & (BLOCK - 1)).astype(np.int64), (e >> 13).astype(np.int64)
            asc = bool((np.diff(got_loc) > 0).all())
            ascending &= asc
            if ordered:
                assert asc, (b, gene)
            o = np.argsort(got_loc, kind="stable")
            np.testing.assert_array_equal(got_loc[o], loc, err_msg=f"block {b} gene {gene}")
            np.testing.assert_array_equal(got_cnt[o], cnt, err_msg=f"block {b} gene {gene}")
            longest = max(longest, len(e))
    assert longest > 256                                     # a column of more than one 64-row work item
    assert ptr[-1, -1] == len(data) == blocks.nnz_sel        # every entry of the selected cells is in exactly one column
    return ascending


@gpu
def test_extract_cols_ranged_ingest(eng, prob, dev_cols):
    """mm_extract_cols on the range-partitioned ingest: every (block, column) holds exactly the gene's (cell_local, count) entries
    among the block's cells, cell_local strictly ascending, no zero entry, blk_cnt entries long -- for all 150 genes (ragged last
    slice), columns of thousands of entries, the empty gene, and the gene that is silent in one block."""
    blocks, cols = dev_cols
    assert _check_columns(eng, prob, blocks, cols, ordered=True)
    ptr = eng.host(cols.col_ptr)
    assert (np.diff(ptr, axis=1)[:, NEVER] == 0).all()
    present = np.diff(ptr, axis=1) > 0                        # [block][gene]
    assert present[:3, BLK_SILENT].tolist() == [True, False, True] and present[3, BLK_SILENT]
    assert present[:, ONE_GROUP].tolist() == [True, True, True, False, False, False]
    np.testing.assert_array_equal(present, np.stack([prob.X[cells].any(axis=0) for _, cells in prob.plan]))


@gpu
def test_extract_cols_unpartitioned_ingest(eng, prob):
    """The same matrix with the entries of every row shuffled takes the unpartitioned ingest (``ranged == False``), whose per-gene
    cursors still pack a gene's entries front to back -- in whatever order the waves of the block reach them.  The columns hold
    the same entries as a set per (block, column).  Observed on the MI355X: cell_local does NOT ascend in every column there (the
    rows of a block are scattered by 16 waves at once, so the order depends on their timing and is not asserted); no consumer
    needs an order: the pair kernels join through a dense per-cell vector.  The test prints what it saw."""
    import torch

    X = prob.csr
    rng = np.random.default_rng(3)
    row = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    o = np.lexsort((rng.random(X.nnz), row))                 # a random order inside every row
    assert (np.diff(X.indices[o])[np.diff(row) == 0] < 0).any()
    csr = eng.DeviceCSR.from_device(torch.from_numpy(X.indptr.astype(np.int64)).cuda(), torch.from_numpy(X.indices[o].astype(np.int32)).cuda(),
                                    torch.from_numpy(X.data[o].astype(np.float32)).cuda(), X.shape)
    blocks = eng.CountBlocks(csr, prob.gid, prob.ng)
    assert not blocks.ranged
    ascending = _check_columns(eng, prob, blocks, eng.GeneColumns(blocks, np.arange(N_GENES)), ordered=False)
    print(f"\nunpartitioned ingest: cell_local ascending in every column: {ascending}")


# ------------------------------------------------------------------------------------------------------------------------
# 2. pair_cross
# ------------------------------------------------------------------------------------------------------------------------


@gpu
def test_pair_cross_against_longdouble(eng, prob, dev_cols):
    """prod[group][pair] = sum_c x_ci x_cj inv_sf_c^2 against the np.longdouble reference.  All terms are non-negative, so the
    kernel's relative error is bounded by the roundings on its longest path: 3 per term ((x_i w) w, times x_j) + the sequential
    adds of a lane (ceil(longest right column in a block / 64)) + 6 shuffle adds + one add per block of the group = n_r;
    |got - ref| <= 2 n_r 2^-53 ref, the factor 2 covering the reference."""
    blocks, cols = dev_cols
    c1, c2 = _pair_list()
    inv_sf = 1.0 / prob.sf
    got = eng.pair_cross(cols, c1, c2, inv_sf)
    assert got.shape == (prob.ng, len(c1))
    lens = blocks.blk_cnt.astype(np.int64)                                       # [block][gene], checked by the extraction tests
    blk_of = [[b for b, (g, _) in enumerate(prob.plan) if g == k] for k in range(prob.ng)]
    assert [len(b) for b in blk_of] == [3, 1, 1, 1]
    u = 2.0 ** -53
    n_r_max = 0
    where = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(c1, c2))}          # (last occurrence of a duplicated pair)
    dup = np.flatnonzero((c1 == 50) & (c2 == 51))
    assert len(dup) == 2
    for k in range(prob.ng):
        ref = _ref_cross(prob.X, inv_sf, prob.sel[k], c1, c2)
        n_r = 3 + -(-lens[blk_of[k]][:, c2].max(axis=0) // 64) + 6 + len(blk_of[k])        # [pair]
        n_r_max = max(n_r_max, int(n_r.max()))
        err = np.abs(got[k].astype(np.longdouble) - ref)
        bad = np.flatnonzero(err > 2 * n_r * u * ref)
        assert len(bad) == 0, (k, bad[:5], err[bad[:5]], ref[bad[:5]])
        empty = ref == 0
        assert (got[k][empty] == 0.0).all() and not np.signbit(got[k][empty]).any()
        for a, b in ((H0, H1), (40, 41), (H0, H2), (BLK_SILENT, 61), (ONE_GROUP, 62), (NEVER, 60)):
            i, j = where[(a, b)], where[(b, a)]
            assert abs(got[k, i] - got[k, j]) <= 2 * max(n_r[i], n_r[j]) * u * float(ref[i]), (k, a, b)
        assert got[k, dup[0]] == got[k, dup[1]]
    assert n_r_max > 3 + 64 + 6 + 3                                               # the dense columns: > 4,096 entries in a block
    assert got[0, (c1 == BLK_SILENT) & (c2 == 61)][0] > 0 and (got[1:, c1 == ONE_GROUP] == 0).all() and (got[:, c1 == NEVER] == 0).all()


@gpu
def test_compute_2d_moments_cov_vs_oracle(eng, orc, prob):
    """The API on the same matrix: compute_2d_moments' covariances (mm_pair_cross + the 1D sums, with the self-pair correction)
    against oracle.cov_2d_sparse, at the tolerance test_moments_vs_oracle uses for variances."""
    import pandas as pd

    from scrna_parameter_estimation_amd import AnnDataLite, memento

    n = prob.csr.shape[0]
    obs = pd.DataFrame({"grp": [f"g{k}" for k in prob.gid], "q": np.full(n, Q_GROUP)}, index=[f"c{i}" for i in range(n)])
    adata = AnnDataLite(prob.csr.copy(), obs, pd.DataFrame(index=[f"gene{i}" for i in range(N_GENES)]))
    memento.setup_memento(adata, q_column="q")
    memento.create_groups(adata, label_columns=["grp"])
    memento.compute_1d_moments(adata, min_perc_group=0.3)
    m = adata.uns["memento"]
    names = list(adata.var.index)
    kept = np.array([int(s[4:]) for s in names])
    assert {H0, H1, H2, 30, 40, 41, 50, 51, MANY} <= set(kept.tolist()) and NEVER not in kept
    pos = {int(g): i for i, g in enumerate(kept)}
    want_pairs = [(a, b) for a, b in SPECIAL_PAIRS if a in pos and b in pos]
    assert (H0, H0) in want_pairs and (30, 30) in want_pairs and (H0, H1) in want_pairs and len(want_pairs) >= 20
    memento.compute_2d_moments(adata, [(f"gene{a}", f"gene{b}") for a, b in want_pairs])
    i1, i2 = np.array([pos[a] for a, _ in want_pairs]), np.array([pos[b] for _, b in want_pairs])
    sf = adata.obs["memento_size_factor"].values
    Xk = sp.csc_matrix(prob.X[:, kept].astype(np.float64))
    gid = m["_hip"].group_id
    assert len(m["groups"]) == prob.ng + 1                     # the cells outside the four groups form a fifth one here
    for k, label in enumerate(m["groups"]):
        sel = np.flatnonzero(gid == k)
        cov = orc.cov_2d_sparse(Xk[sel], sf[sel], m["group_q"][label], i1, i2)
        np.testing.assert_allclose(m["2d_moments"][label]["cov"], cov, rtol=1e-9, atol=1e-13, err_msg=label)


# ------------------------------------------------------------------------------------------------------------------------
# 3. histograms and bin counts
# ------------------------------------------------------------------------------------------------------------------------


@gpu
def test_pair_histograms_and_bin_counts_exact(eng, prob, boot):
    """mm_pair_hist + mm_pair_bins_count: for every special pair (and some ordinary ones) in every group the dense table equals the
    host's cell counts entry by entry -- the x_j == 0 column, derived on the device as 1D table minus row sum, on its own -- the
    bins equal np.unique's (sf_bin, x_i, x_j, multiplicity) rows, K is their number and the multiplicities sum to N_g."""
    bs = boot.bs
    n_zero_col = 0
    for q in _special_chains(prob, boot):
        xi, xj, sbin = _pair_cells(prob, boot, q)
        want = _ref_table(xi, xj, sbin)
        assert (bs.n_bins, int(bs.xcap_i[q]), int(bs.xcap_j[q])) == want.shape, q
        t0 = int(bs.tab_ptr[q])
        tab = eng.host(bs.tab[t0:t0 + want.size], np.uint32).reshape(want.shape)
        np.testing.assert_array_equal(tab[:, :, 0], want[:, :, 0], err_msg=f"x_j == 0 column of chain {q}")
        np.testing.assert_array_equal(tab, want, err_msg=f"chain {q}")
        n_zero_col += int((want[:, :, 0] != 0).sum())
        rows, mult = _ref_bins(xi, xj, sbin)
        bi, bxi, bxj, mu = bs.bins_of(q)
        np.testing.assert_array_equal(np.stack([bi, bxi, bxj], axis=1), rows)
        np.testing.assert_array_equal(mu, mult)
        assert bs.K[q] == len(mult) and mu.sum() == prob.sizes[q % prob.ng]
    assert n_zero_col > 1000


# ------------------------------------------------------------------------------------------------------------------------
# 4. ordering regimes, both replay kernels, both tile regimes
# ------------------------------------------------------------------------------------------------------------------------


@gpu
def test_ordering_paths_and_replay_kernels_agree_bit_for_bit(eng, prob, boot, monkeypatch):
    """The same chains ordered by the small in-LDS kernel / the big one (CAP 4096, 512 threads) / the host, replayed from operand
    records (mm_boot2d_replay_rec) or from [row][64] planes (mm_boot2d_replay), in <= 2048 wide tiles or in > 2048 one-chain tiles
    (the three-waves-per-SIMD builds): every combination run here gives bit-identical replicate correlations, NaNs included."""
    bs = boot.bs
    live = ~boot.skip & (bs.K >= 1)
    n_live = int(live.sum())
    per_range = np.bincount(_k_range(bs.K[live]), minlength=3)
    print(f"\nchains: {n_live} live of {bs.n_q}; K <= 1024: {per_range[0]}, 1024 < K <= 4096: {per_range[1]}, K > 4096: {per_range[2]}; "
          f"K max {bs.K.max()}")
    assert (per_range > 0).all() and n_live > 2048
    base, ran = _run(eng, monkeypatch, boot)
    assert ran == dict(small=per_range[0], big=per_range[1], host=per_range[2], kernel="mm_boot2d_replay_rec", n_tiles=ran["n_tiles"])
    assert 0 < ran["n_tiles"] <= 2048
    assert np.isnan(base[~live, 1:]).all() and np.isfinite(base[live]).all()
    np.testing.assert_array_equal(base[:, 0], boot.true_corr)
    variants = [
        (dict(small_cap=0), dict(small=0, big=per_range[0] + per_range[1], host=per_range[2], kernel="mm_boot2d_replay_rec")),
        (dict(small_cap=0, big_cap=0), dict(small=0, big=0, host=n_live, kernel="mm_boot2d_replay_rec")),
        (dict(records=False), dict(small=per_range[0], big=per_range[1], host=per_range[2], kernel="mm_boot2d_replay")),
        (dict(small_cap=0, records=False), dict(small=0, big=per_range[0] + per_range[1], host=per_range[2], kernel="mm_boot2d_replay")),
        (dict(many_tiles=True), dict(small=per_range[0], big=per_range[1], host=per_range[2], kernel="mm_boot2d_replay_rec")),
        (dict(many_tiles=True, records=False), dict(small=per_range[0], big=per_range[1], host=per_range[2], kernel="mm_boot2d_replay")),
    ]
    for kw, want in variants:
        yc, ran = _run(eng, monkeypatch, boot, **kw)
        n_tiles = ran.pop("n_tiles")
        assert ran == want, kw
        assert (n_tiles > 2048) if kw.get("many_tiles") else (0 < n_tiles <= 2048), (kw, n_tiles)
        np.testing.assert_array_equal(yc, base, err_msg=str(kw))
        print(f"{kw}: {ran}, {n_tiles} tiles: identical")


# ------------------------------------------------------------------------------------------------------------------------
# 5. replicate correlations against the oracle
# ------------------------------------------------------------------------------------------------------------------------


@gpu
def test_replicate_correlations_vs_oracle(eng, orc, prob, boot, monkeypatch):
    """yc[q, 1:] of every chain of every special pair (and 40 ordinary chains) against corr_from_cov(*bootstrap_2d(...)) on the same
    hash uniforms, at the tolerance of the full-size 2D spot check.  Skipped chains stay NaN; where the oracle meets a variance
    <= 0 (its 5.0 sentinel, clipped to 1) the kernel must give exactly 1.0; no replicate of a live chain is NaN."""
    bs = boot.bs
    yc, _ = _run(eng, monkeypatch, boot)
    checked, sentinels, ranges, k1 = 0, 0, set(), 0
    for q in _special_chains(prob, boot):
        got = yc[q]
        if boot.skip[q]:
            assert np.isnan(got[1:]).all(), q
            continue
        xi, xj, sbin = _pair_cells(prob, boot, q)
        n = len(xi)
        cov, v1, v2 = orc.bootstrap_2d(xi.astype(np.float64), xj.astype(np.float64), prob.sf_table[sbin], Q_GROUP, boot.B,
                                       (boot.ra[q], boot.rb[q]), boot.r0[q])
        want = orc.corr_from_cov(cov, v1, v2)
        assert got[0] == boot.true_corr[q]
        np.testing.assert_allclose(got[1:], want, rtol=1e-9, atol=1e-12, equal_nan=True, err_msg=f"chain {q} (K = {bs.K[q]}, {n} cells)")
        sent = (v1 <= 0) | (v2 <= 0)
        np.testing.assert_array_equal(got[1:][sent], want[sent], err_msg=f"chain {q}: sentinel replicates")
        assert (want[sent] == 1.0).all() and (np.abs(got[1:]) <= 1).all()
        sentinels += int(sent.sum())
        ranges.add(int(_k_range(bs.K[q])))
        k1 += int(bs.K[q] == 1)
        checked += 1
    print(f"\n{checked} chains compared, {sentinels} sentinel replicates, {k1} chains with K == 1")
    assert checked > 80 and ranges == {0, 1, 2} and sentinels > 100 and k1 >= 1
    assert boot.skip[_special_chains(prob, boot)].sum() >= 5


# ------------------------------------------------------------------------------------------------------------------------
# 6. replay-hash collision
# ------------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("caps", [(SMALL_K, BIG_K), (0, BIG_K), (0, 0)], ids=["small-kernel", "big-kernel", "host"])
@pytest.mark.parametrize("records", [True, False], ids=["records", "planes"])
def test_hash_collision_is_reported(eng, monkeypatch, caps, records):
    """With r1a == r1b the bins (x_i, x_j) = (1, 2) and (2, 1) of one size-factor bin get the same code, which np.unique would
    merge: every ordering path must report it (NotImplementedError from the status word; nothing faults)."""
    rng = np.random.default_rng(5)
    n = 200
    X = rng.poisson(0.7, size=(n, 3)).astype(np.int64)
    X[10, :2], X[20, :2] = (1, 2), (2, 1)
    sf_bin = rng.integers(0, 4, size=n).astype(np.uint8)
    sf_bin[[10, 20]] = 2
    sf_table = np.linspace(0.5, 2.0, 4)
    gid = np.zeros(n, dtype=np.int32)
    blocks = eng.CountBlocks(eng.DeviceCSR(sp.csr_matrix(X.astype(np.float32))), gid, 1)
    _, _, maxx = blocks.moments(np.ones(n))
    cols = eng.GeneColumns(blocks, np.arange(3))
    bs = eng.Bootstrap2D(cols, [0, 2], [1, 0], maxx, sf_bin, sf_table, np.full(1, Q_GROUP), 8)
    monkeypatch.setattr(eng, "ORDER_SMALL_CAP", caps[0])
    monkeypatch.setattr(eng, "ORDER_BIG_CAP_2D", caps[1])
    monkeypatch.setattr(eng, "BOOT2D_RECORDS", records)
    ra, rb, r0 = rng.random((3, 2))
    skip, zeros = np.zeros(2, dtype=bool), np.zeros(2)
    bs.run(skip, ra, rb, r0, zeros)                                                 # generic multipliers: no collision
    assert np.isfinite(eng.host(bs.yc)).all()
    path = "small" if caps[0] else "big" if caps[1] else "host"
    assert bs.order_path[path] == 2 and sum(bs.order_path.values()) == 2
    with pytest.raises(NotImplementedError):
        bs.run(skip, ra, ra, r0, zeros)


# ------------------------------------------------------------------------------------------------------------------------
# 7. CSR column kernels
# ------------------------------------------------------------------------------------------------------------------------


def _csr_problem():
    rng = np.random.default_rng(12)
    n, G = 333, 200                                   # rows of ~100 entries: more than one 64-lane pass per row
    X = (rng.random((n, G)) < 0.5) * rng.integers(1, 9, size=(n, G))
    X[:, 0] = 0
    X[:, G - 1] = 0
    X[[0, 17, 64, n - 1], :] = 0
    return sp.csr_matrix(X.astype(np.float32))


def _filter_rows(indptr, indices, data, new_id):
    """Host reference of the column split: keep the entries with new_id[column] >= 0, in their order, renumbered."""
    keep = new_id[indices] >= 0
    row = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=len(indptr) - 1))])
    return ptr, new_id[indices[keep]], data[keep]


@gpu
@pytest.mark.parametrize("shuffled", [False, True], ids=["canonical", "rows-shuffled"])
def test_csr_column_kernels_exact(eng, shuffled):
    """DeviceCSR.colsplit / colselect / colsum (mm_csr_colcount, _colsplit, _mapcount, _mapsplit, _colsum) on a matrix with empty rows,
    an empty first and last column and 333 rows: indptr, indices, data bit-equal to scipy's column slice, the order inside rows
    preserved (also for rows that are not sorted), totals exact."""
    import torch

    X = _csr_problem()
    n, G = X.shape
    indptr, indices, data = X.indptr.astype(np.int64), X.indices.copy(), X.data.copy()
    if shuffled:
        row = np.repeat(np.arange(n), np.diff(indptr))
        o = np.lexsort((np.random.default_rng(1).random(X.nnz), row))
        indices, data = indices[o], data[o]
    csr = eng.DeviceCSR.from_device(torch.from_numpy(indptr).cuda(), torch.from_numpy(indices.astype(np.int32)).cuda(),
                                    torch.from_numpy(data.astype(np.float32)).cuda(), X.shape)

    def check(out, genes):
        new_id = np.full(G, -1, dtype=np.int64)
        new_id[genes] = np.arange(len(genes))
        ptr, idx, dat = _filter_rows(indptr, indices, data, new_id)
        assert out.shape == (n, len(genes)) and out.nnz == len(idx)
        np.testing.assert_array_equal(eng.host(out.indptr), ptr)
        np.testing.assert_array_equal(eng.host(out.indices), idx)
        np.testing.assert_array_equal(eng.host(out.data), dat)
        if not shuffled:                                                     # and scipy's own slice
            S = X[:, genes]
            S.sort_indices()
            np.testing.assert_array_equal(ptr, S.indptr)
            np.testing.assert_array_equal(idx, S.indices)
            np.testing.assert_array_equal(dat, S.data)

    for lo, hi in [(5, 5), (0, 0), (G, G), (0, G), (0, 1), (G - 1, G), (0, 70), (1, G - 1), (130, G), (63, 65)]:
        check(csr.colsplit(lo, hi), np.arange(lo, hi))
    scattered = np.sort(np.random.default_rng(2).choice(G, size=37, replace=False))
    for genes in (scattered, np.array([0, G - 1]), np.array([0, 1, 64, G - 2, G - 1]), np.arange(G), np.zeros(0, dtype=np.int64)):
        check(csr.colselect(genes), genes)
    tot = csr.colsum()
    assert tot.dtype == np.float64
    np.testing.assert_array_equal(tot, np.asarray(X.astype(np.float64).sum(axis=0)).ravel())
    assert tot[0] == 0 and tot[-1] == 0
    with pytest.raises(ValueError):
        csr.colsplit(3, G + 1)
    with pytest.raises(ValueError):
        csr.colselect([4, 4])


# ------------------------------------------------------------------------------------------------------------------------
# host only: the references themselves
# ------------------------------------------------------------------------------------------------------------------------


def test_host_references_agree_with_the_oracle(orc):
    """No device: the block plan, the per-block column decoder, the bin multiset, the longdouble pair sums and the K-range check of
    this module on a reduced problem (blocks of 256 cells) against engine.plan_blocks, oracle.unique_bins_2d, exact rational
    arithmetic and oracle.cov_2d_sparse; and the full problem's K ranges, which the device tests then assert from bs.K."""
    from scrna_parameter_estimation_amd.engine import plan_blocks

    small = _problem(sizes=(700, 256, 60, 6), n_out=20, block=256)
    order, blk_cell0, blk_group, grp_blk0, counts = plan_blocks(small.gid, small.ng, block_cells=256)
    assert len(small.plan) == len(blk_group) == 6 and counts.tolist() == [700, 256, 60, 6]
    rebuilt = np.zeros_like(small.X)
    for b, (g, cells) in enumerate(small.plan):
        assert blk_group[b] == g and len(cells) <= 256
        np.testing.assert_array_equal(order[blk_cell0[b]:blk_cell0[b + 1]], cells)
        for gene in range(N_GENES):
            loc, cnt = _ref_column(small.X, cells, gene)
            assert (cnt > 0).all() and (np.diff(loc) > 0).all()
            rebuilt[cells[loc], gene] = cnt
    rebuilt[small.gid < 0] = small.X[small.gid < 0]
    np.testing.assert_array_equal(rebuilt, small.X)
    assert small.X[small.plan[1][1], BLK_SILENT].sum() == 0 and small.X[small.plan[0][1], BLK_SILENT].sum() > 0
    assert small.X[:, NEVER].sum() == 0 and small.X[small.gid != 0, ONE_GROUP].sum() == 0 and small.X[:, ONE_GROUP].sum() > 0
    # bins: the (sf_bin, x_i, x_j) rows of np.unique against the oracle's hash-coded bins
    ra, rb, r0 = np.random.default_rng(6).random(3)          # generic multipliers: the hash separates what np.unique over rows does
    for a, b in SPECIAL_PAIRS[:24:3]:
        for g, sel in enumerate(small.sel):
            xi, xj, sbin = small.X[sel, a], small.X[sel, b], small.sf_bin[sel]
            rows, mult = _ref_bins(xi, xj, sbin)
            inv, _, e1, e2, om = orc.unique_bins_2d(xi.astype(np.float64), xj.astype(np.float64), small.sf_table[sbin], (ra, rb), r0)
            got = sorted(zip(np.round(small.sf_table[rows[:, 0]], 12).tolist(), rows[:, 1].tolist(), rows[:, 2].tolist(), mult.tolist()))
            assert got == sorted(zip(np.round(1.0 / inv, 12).tolist(), e1.astype(int).tolist(), e2.astype(int).tolist(), om.tolist()))
            tab = _ref_table(xi, xj, sbin)
            assert tab.sum() == len(sel) and int((tab != 0).sum()) == len(mult)
            np.testing.assert_array_equal(tab[rows[:, 0], rows[:, 1], rows[:, 2]], mult)
    # pair sums: longdouble against exact rationals, and against the oracle's covariance
    inv_sf = 1.0 / small.sf
    i1, i2 = np.array([H0, H1, H0, 30, 40, NEVER, BLK_SILENT]), np.array([H1, H0, H0, 30, 41, 60, 61])
    for g, sel in enumerate(small.sel):
        ref = _ref_cross(small.X, inv_sf, sel, i1, i2)
        for k in range(len(i1)):
            exact = sum(Fraction(int(small.X[c, i1[k]] * small.X[c, i2[k]])) * Fraction(float(inv_sf[c])) ** 2 for c in sel)
            assert abs(Fraction(float(ref[k])) - exact) <= exact * Fraction(1, 2 ** 51)      # (float(): one more rounding, to fp64)
            if np.finfo(np.longdouble).eps < 2.0 ** -60:
                hi = float(ref[k])
                assert abs(Fraction(hi) + Fraction(float(ref[k] - np.longdouble(hi))) - exact) <= exact * Fraction(1, 2 ** 58)
        Xg = sp.csc_matrix(small.X[sel].astype(np.float64))
        n = len(sel)
        mean = np.asarray(Xg.T.dot(inv_sf[sel])).ravel() / n
        cov = ref.astype(np.float64) / n - mean[i1] * mean[i2]
        same = i1 == i2
        cov[same] -= (1 - Q_GROUP) * np.asarray(Xg[:, i1[same]].T.dot(inv_sf[sel] ** 2)).ravel() / n
        np.testing.assert_allclose(cov, orc.cov_2d_sparse(Xg, small.sf[sel], Q_GROUP, i1, i2), rtol=1e-9, atol=1e-13)
    # K ranges
    assert _k_range([1, 1024, 1025, 4096, 4097]).tolist() == [0, 0, 1, 1, 2]
    full = _problem()
    assert [len(c) for _, c in full.plan] == [5667, 5668, 5668, 8192, 300, 6] and (full.gid < 0).sum() == 150
    seen = set()
    for a, b in ((H0, H1), (H0, H2), (H2, H2), (H0, 70), (40, 41)):
        for g, sel in enumerate(full.sel):
            xi, xj = full.X[sel, a].astype(np.float64), full.X[sel, b].astype(np.float64)
            K = len(orc.unique_bins_2d(xi, xj, full.sf_table[full.sf_bin[sel]], (ra, rb), r0)[4])
            assert K == len(_ref_bins(full.X[sel, a], full.X[sel, b], full.sf_bin[sel])[1])
            seen.add(int(_k_range(K)))
    assert seen == {0, 1, 2}
    assert full.X[:, H1].max() == 300 and full.X[:, [H0, H1, H2]].mean(axis=0).min() >= 5
