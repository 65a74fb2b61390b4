"""Plain numpy restatement of the 1D histogram / bin-count / bin-order stage (mm_hist1d_sell, mm_bins_count, mm_bins_order and the
host fallback), for the kernel tests.  Nothing here imports the engine: the replay order, the success probabilities and the
operands are written out again from the reference's definition (bootstrap.py:62-71 and numpy's random_multinomial), one IEEE
fp64 operation at a time, so that a kernel built with contraction off can be compared bit for bit.

``problem_1905`` is the test problem with genuinely long chains that tests/test_cpu_bins_ref.py and tests/test_gpu_bins_1d.py
share; ``ulp_diff`` measures a distance in units in the last place."""

from types import SimpleNamespace

import numpy as np

MAX_COUNT = (1 << 19) - 1            # the largest count the stage carries: all 19 bits of the payload's count field


def ref_table(x, sf_bin, n_bins, xcap):
    """Dense [n_bins][xcap] uint32 table of one (gene, group): how many of its cells have (size-factor bin, count) = (row, column).
    ``x``: the dense per-cell counts (zeros included), ``sf_bin``: the cells' size-factor bins."""
    x = np.asarray(x, dtype=np.int64)
    b = np.asarray(sf_bin, dtype=np.int64)
    assert x.shape == b.shape and x.ndim == 1
    assert len(x) == 0 or (x.min() >= 0 and x.max() < xcap and b.min() >= 0 and b.max() < n_bins)
    return np.bincount(b * xcap + x, minlength=n_bins * xcap).astype(np.uint32).reshape(n_bins, xcap)


def ref_count(table):
    """K: the number of non-empty bins."""
    return int(np.count_nonzero(table))


def ref_order(table, sf_table, r1, r0, n_cells):
    """The bins of ``table`` in replay order with the bootstrap operands of each: (bin, x, mult, pk, lq, a, b), K long each.

    code = fl(fl(x * r1) + fl(r0 * sf)) ascending (a stable argsort of the canonical, bin-major order; the codes must be pairwise
    distinct, np.unique would merge equal ones); pix = mult / n_cells; remaining_p starts at 1.0 and loses pix[k] after bin k, one
    rounded subtraction after the other; pk = pix / remaining_p; lq = log(1 - p) with p = pk or, above one half, 1 - pk;
    a = 1 / sf; b = 1 / (sf * sf)."""
    table = np.asarray(table)
    bi, xi = np.nonzero(table)                                     # canonical order: bin major, count minor
    mult = table[bi, xi].astype(np.int64)
    sf = np.asarray(sf_table, dtype=np.float64)[bi]
    cx = xi.astype(np.float64) * np.float64(r1)
    cs = np.float64(r0) * sf
    code = cx + cs
    o = np.argsort(code, kind="stable")
    assert (code[o][1:] != code[o][:-1]).all(), "two bins have the same code"
    pix = mult[o].astype(np.float64) / np.float64(n_cells)
    rem = np.empty(len(pix), dtype=np.float64)
    left = np.float64(1.0)
    for k in range(len(pix)):
        rem[k] = left
        left = left - pix[k]
    pk = pix / rem
    p = np.where(pk <= 0.5, pk, 1.0 - pk)
    with np.errstate(divide="ignore", invalid="ignore"):
        lq = np.log(1.0 - p)
    sfo = sf[o]
    return bi[o], xi[o], mult[o], pk, lq, 1.0 / sfo, 1.0 / (sfo * sfo)


def ulp_diff(a, b):
    """Distance between fp64 arrays in units in the last place (the difference of their positions on the ordered line of doubles;
    +0 and -0 coincide).  NaN in either gives the largest int64."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)

    def line(v):
        i = v.view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i).astype(object)

    d = np.abs(line(a) - line(b))
    d[np.isnan(a) | np.isnan(b)] = 2 ** 63 - 1
    return np.array([min(int(v), 2 ** 63 - 1) for v in d.ravel()], dtype=np.int64).reshape(a.shape)


# K of every (gene, group) of problem_1905, [gene][group]: the small ordering kernel exactly at its cap (1024), the big one
# (1935, 2400, 3525) and the host (11453), with the engine's default caps
K_1905 = [[2400, 1935], [11453, 3525], [24, 20], [40, 34], [1024, 1009]]


def problem_1905():
    """24,000 cells in two groups (20,000: three count blocks; 4,000), four size-factor bins, five dense genes whose chains have
    K_1905 bins; gene 3 carries one count of 2^19 - 1 in size-factor bin 3 of group 0.  The two hash uniforms of every (gene, group)
    come from the same generator; no two bins of a chain collide in them."""
    rng = np.random.default_rng(1905)
    n = 24000
    gid = np.zeros(n, dtype=np.int32)
    gid[20000:] = 1
    gid = gid[rng.permutation(n)]
    sf_table = np.array([0.6, 0.9, 1.3, 2.1])
    sf_bin = rng.integers(0, 4, size=n).astype(np.uint8)
    X = np.zeros((n, 5), dtype=np.int64)
    X[:, 0] = rng.integers(0, 600, size=n)
    X[:, 1] = rng.integers(0, 4000, size=n)
    X[:, 2] = rng.poisson(0.5, size=n)
    X[:, 3] = rng.poisson(2.0, size=n)
    c = np.flatnonzero(gid == 0)[7]
    X[c, 3], sf_bin[c] = MAX_COUNT, 3
    X[:, 4] = rng.integers(0, 256, size=n)                          # 4 x 256 = 1024 possible bins
    r = rng.random((2, 10))
    sel = [np.flatnonzero(gid == k) for k in range(2)]
    return SimpleNamespace(n=n, ng=2, n_genes=5, n_bins=4, gid=gid, sf_table=sf_table, sf_bin=sf_bin, X=X, r1=r[0], r0=r[1], sel=sel,
                           sizes=[len(s) for s in sel], big_cell=int(c), grp_q=np.array([0.07, 0.11]))


def pair_cells(prob, p):
    """(dense counts, size-factor bins) of the cells of pair p = gene * n_groups + group."""
    g, k = divmod(int(p), prob.ng)
    return prob.X[prob.sel[k], g], prob.sf_bin[prob.sel[k]]
