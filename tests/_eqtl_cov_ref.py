"""Plain numpy restatement of the gene-major resampled coefficient with a covariate PER TEST (mm_cross_cov_beta,
mm_cross_resampled_block_cov, mm_residualize_rank1 of include/memento_hip.h), with a rounding bound from its own sums of absolute
terms, and the hand-built problem the kernel tests and their CPU check share.  No GPU, no project code."""

import numpy as np

from _replicate_ref import cross_draws

L = np.longdouble
U = 2.0 ** -53                                          # unit round-off of fp64
TT = 8                                                  # engine.CROSS_BLOCK_TT
COUNTS = [TT + 1, 2 * TT + 3, 1, TT, 0, TT - 1]         # tests per gene, as in test_gpu_eqtl_block
SEED = 0xDEADBEEF12345678                               # of the device draws in the kernel tests
KEYS = [4, 0, 3, 5, 1, 2 ** 31 + 9]                     # gene keys there (one above 2^31: the key is 64 bits wide)
ZERO_Z_TEST = 3                                         # a test of gene 0's first tile whose zt row is zero; its neighbours' are not


def cov_problem(B, ng, seed=21, counts=COUNTS):
    """The problem of test_gpu_eqtl_block._problem -- six genes of ``ng`` groups: all good, two bad, one good, all good, all good,
    two bad; ``counts[g]`` tests each; test 1 of gene 0 with ONE group off the others' common treatment value (a column that misses
    it is degenerate for this test alone); dropped columns for the col_map variant -- with a covariate row ``zt`` per test beside
    ``tt``.  Row ``ZERO_Z_TEST`` of zt is zero.  -> yt, good, gene_ptr, tt, zt, Nc, col_map, n_valid."""
    rng = np.random.default_rng(seed)
    n_genes, ld = len(counts), B + 2
    yt = rng.normal(0, 1, size=(n_genes * ng, ld))
    yt[:, B + 1:] = np.nan
    good = np.ones((n_genes, ng), dtype=bool)
    for g in (1, 5):
        good[g, [3, 7]] = False
        yt[g * ng + 3] = np.nan                                                # a bad group's rows are never read
    good[2] = False
    good[2, 5] = True
    gene_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    tt = rng.normal(0, 1, size=(int(gene_ptr[-1]), ng))
    tt[1] = 0.25
    tt[1, ng - 2] = -1.5
    Nc = rng.integers(200, 900, size=ng).astype(np.float64)
    col_map = np.zeros((n_genes, B + 1), dtype=np.int32)
    n_valid = np.zeros(n_genes, dtype=np.int32)
    for gene, dropped in enumerate([np.r_[4, 60:95, B], [], [1, 2, 3, 64, B - 1], np.arange(1, B + 1), [], [2]]):
        keep = np.setdiff1d(np.arange(B + 1), dropped)
        col_map[gene, :len(keep)] = keep
        n_valid[gene] = len(keep)
    zt = rng.normal(0, 1, size=tt.shape)
    zt[ZERO_Z_TEST] = 0.0
    return yt, good, gene_ptr, tt, zt, Nc, col_map, n_valid


def poison_dropped(yt, good, col_map, n_valid):
    """A copy of ``yt`` with NaN in the first good group of every gene at the columns that col_map leaves out (why valid_cols would
    have dropped them): beta is NaN there, and nothing may read it."""
    yt = yt.copy()
    ng = good.shape[1]
    for g in range(len(good)):
        if good[g].any():
            out = np.setdiff1d(np.arange(col_map.shape[1]), col_map[g, :n_valid[g]])
            yt[g * ng + int(np.flatnonzero(good[g])[0]), out] = np.nan
    return yt


def draw_tables(good, n_valid, B, seed, keys):
    """rep / bcol [gene][group][B] from the numpy restatement of the draw rule, gene g under key ``keys[g]``."""
    n_genes, ng = good.shape
    rep, bcol = np.zeros((n_genes, ng, B), dtype=np.int16), np.zeros((n_genes, ng, B), dtype=np.int32)
    for g in range(n_genes):
        n, nb = int(good[g].sum()), (int(n_valid[g]) - 1 if n_valid is not None else B)
        if nb >= 1:
            rep[g, :n], bcol[g, :n] = cross_draws(seed, int(keys[g]), n, nb, B)
    return rep, bcol


def cov_beta(y, z, Nc, good):
    """beta [ld] = sum_j Nc_j z_j y[j] / sum_j Nc_j z_j^2 over the good groups of one gene's residualised plane ``y`` [ng][ld]
    (zero when the denominator is zero), in np.longdouble, and how far fp64 weights and a sequential fp64 sum of n terms may be
    from it: (2 n + 8) 2^-53 sum_j |w_j y_j| -- (n + 2) for the sum, (n + 4) for the relative error of a weight, whose
    denominator is a sum of n non-negative terms, and 2 to spare.  Columns with a non-finite entry give NaN."""
    idx = np.flatnonzero(good)
    n = len(idx)
    zL, wL, yL = z[idx].astype(L), Nc[idx].astype(L), y[idx].astype(L)
    den = (wL * zL * zL).sum()
    wz = wL * zL / den if den > 0 else np.zeros(n, dtype=L)
    with np.errstate(invalid="ignore"):
        terms = wz[:, None] * yL
        return terms.sum(axis=0), (2 * n + 8) * U * np.abs(terms).sum(axis=0)


def cov_row(y, z, a, Nc, good, rep, bcol, col_map, nb, B):
    """The coefficient row [B + 1] of ONE test: ``y`` [ng][ld] the gene's residualised plane, ``z`` / ``a`` [ng] the test's covariate
    and treatment, ``rep`` / ``bcol`` [>= n][B] the gene's draws (column 0 is the identity), ``col_map`` [B + 1] or None, ``nb`` the
    resampled columns.  Column c < nb: rows i take group j = glist[rep[i][c]] and replicate column bb = col_map[bcol[i][c]] of
    y_t = y - z beta, and the coefficient is the weighted slope of _cross_coef_resampled on the drawn groups' treatment, NaN
    where their weighted variance of the treatment is <= 1e-24 max|a|^2 (the degenerate-column rule) and from column nb on.

    -> (row, bound, y_t [ng][ld]) in np.longdouble.  ``bound``: how far an fp64 evaluation with sequential sums may be from
    ``row``, first order, from the restatement's own sums of absolute terms.  With u = 2^-53 and n drawn rows:
      d_yk  = |z| d_beta + 2 u (|y| + |z beta|)                                        the response of a drawn row
      d_mB  = sum w d_yk / sw + (n + 3) u sum w |yk| / sw,   d_mA = (n + 3) u sum w |a| / sw
      d_da  = d_mA + u (|a| + |mA|),   d_dy = d_yk + d_mB + u (|yk| + |mB|)
      d_num = sum (d_da w |dy| + |da| w d_dy) + (n + 6) u sum |da w dy|
      d_ss  = sum 2 |da| w d_da + (n + 6) u ss
      bound = (d_num + 4 u |num|) / ss + |num| d_ss / ss^2."""
    idx = np.flatnonzero(good)
    n = len(idx)
    row, bound = np.full(B + 1, np.nan, dtype=L), np.full(B + 1, np.nan, dtype=L)
    beta, d_beta = cov_beta(y, z, Nc, good)
    with np.errstate(invalid="ignore"):
        y_t = y.astype(L) - z.astype(L)[:, None] * beta[None, :]
    if n == 0 or nb < 1:
        return row, bound, y_t
    r, bb = rep[:n, :nb].astype(np.int64), bcol[:n, :nb].astype(np.int64)
    r[:, 0], bb[:, 0] = np.arange(n), 0
    if col_map is not None:
        bb = np.asarray(col_map, dtype=np.int64)[bb]
    J = idx[r]                                                                 # [n][nb] the drawn groups
    Y, Z, A, W = y[J, bb].astype(L), z[J].astype(L), a[J].astype(L), Nc[J].astype(L)
    Bt, dBt = beta[bb], d_beta[bb]
    yk = Y - Z * Bt
    d_yk = np.abs(Z) * dBt + 2 * U * (np.abs(Y) + np.abs(Z * Bt))
    sw = W.sum(axis=0)
    mB, mA = (W * yk).sum(axis=0) / sw, (W * A).sum(axis=0) / sw
    d_mB = (W * d_yk).sum(axis=0) / sw + (n + 3) * U * (W * np.abs(yk)).sum(axis=0) / sw
    d_mA = (n + 3) * U * (W * np.abs(A)).sum(axis=0) / sw
    da, dy = A - mA, yk - mB
    d_da = d_mA + U * (np.abs(A) + np.abs(mA))
    d_dy = d_yk + d_mB + U * (np.abs(yk) + np.abs(mB))
    ss, num = (da * da * W).sum(axis=0), (da * W * dy).sum(axis=0)
    d_num = (d_da * W * np.abs(dy) + np.abs(da) * W * d_dy).sum(axis=0) + (n + 6) * U * np.abs(da * W * dy).sum(axis=0)
    d_ss = (2 * np.abs(da) * W * d_da).sum(axis=0) + (n + 6) * U * ss
    amax = np.abs(A).max(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        val = num / sw / (ss / sw)
        bnd = (d_num + 4 * U * np.abs(num)) / ss + np.abs(num) * d_ss / (ss * ss)
        dead = ss / sw <= L(1e-24) * amax * amax
    row[:nb], bound[:nb] = np.where(dead, np.nan, val), np.where(dead, np.nan, bnd)
    return row, bound, y_t


def cov_rows(yt, good, gene_ptr, tt, zt, Nc, rep, bcol, col_map, n_valid, B):
    """``cov_row`` for every test of a problem -> (rows, bounds) [n_tests][B + 1] in np.longdouble."""
    ng = good.shape[1]
    test_gene = np.repeat(np.arange(len(gene_ptr) - 1), np.diff(gene_ptr))
    rows, bounds = np.full((len(tt), B + 1), np.nan, dtype=L), np.full((len(tt), B + 1), np.nan, dtype=L)
    for t, g in enumerate(test_gene):
        nb = int(n_valid[g]) - 1 if n_valid is not None else B
        rows[t], bounds[t], _ = cov_row(yt[g * ng:(g + 1) * ng], zt[t], tt[t], Nc, good[g], rep[g], bcol[g],
                                        col_map[g] if col_map is not None else None, nb, B)
    return rows, bounds


def count_limits(row, bound):
    """What the count columns of a record may be when every coefficient is within ``bound`` of ``row``: (lo, hi) [2] for n_extreme
    (#{|v - c0| > |c0|}) and n_raw_extreme (#{|v| > |c0|}) over the valid columns 1.., and the number of (column) cells that are
    closer to their threshold than the bounds allow to decide (``hi - lo`` summed over the two counts)."""
    row, bound = np.asarray(row, dtype=L), np.asarray(bound, dtype=L)
    ok = ~np.isnan(row[1:])
    if np.isnan(row[0]):
        return np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64), 0
    v, b, c0, b0 = row[1:][ok], bound[1:][ok], row[0], bound[0]
    lo, hi = [], []
    for stat, slack in ((np.abs(v - c0) - abs(c0), b + 2 * b0), (np.abs(v) - abs(c0), b + b0)):
        lo.append(int((stat > slack).sum()))
        hi.append(int((stat >= -slack).sum()))
    lo, hi = np.array(lo), np.array(hi)
    return lo, hi, int((hi - lo).sum())
