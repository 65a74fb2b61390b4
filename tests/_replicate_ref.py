"""Plain numpy restatements of what the replicate-statistics kernels promise (include/memento_hip.h): the 8-double test record,
the splitmix64 mixer, the refill draws of mm_boot_fill_log (fill_mode 0) and the device draws of mm_cross_resampled
(d_rep == NULL).  No GPU, no project code: the tests compare the kernels with these."""

import numpy as np

U = np.uint64
FILL_ATTEMPTS = 4096


def _np_stats(row):
    """The 8-double record of the contrast kernels restated in numpy for one coefficient row (NaN = dropped column)."""
    c0 = row[0]
    ok = np.isfinite(row)
    v = row[1:][ok[1:]]
    n = len(v)
    mean1 = v.mean() if n else np.nan
    allv = row[ok]
    lo, hi = (allv.min(), allv.max()) if len(allv) else (np.inf, -np.inf)
    return np.array([c0, np.sqrt(((v - mean1) ** 2).sum() / n) if n else np.nan, n, (np.abs(v - c0) > abs(c0)).sum(), mean1 - c0,
                     1.0 if lo == hi else 0.0, (np.abs(v) > abs(c0)).sum(), hi - lo])


NAN_RECORD = np.array([np.nan, np.nan, 0, 0, np.nan, 0, np.nan, np.nan])      # a test with nothing to test
COUNT_COLUMNS = [2, 3, 5, 6]                                                 # n_valid, extreme, all-equal, raw extreme: exact


def _u64(x):
    """Anything integer (Python int up to 2^64 - 1, negative int64 keys, arrays) as a uint64 array, two's complement."""
    if isinstance(x, int):
        return np.array([x & 0xFFFFFFFFFFFFFFFF], dtype=U)
    x = np.atleast_1d(np.asarray(x))
    return x if x.dtype == U else x.astype(np.int64).view(U)


def mix64(x):
    """The splitmix64 output function (Steele, Lea, Flood 2014; Vigna's splitmix64.c): state 0 gives 0xE220A8397B1DCDAF."""
    x = _u64(x)
    with np.errstate(over="ignore"):
        x = x + U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
    return x ^ (x >> U(31))


def fill_picks(valid, seed, key, plane):
    """mm_boot_fill_log, fill_mode 0: which replicate every invalid entry of one plane of one row takes.

    ``valid`` [B] bool: the originally valid replicates of the plane (0 mean, 1 res_var) of the row with key ``key``.
    Returns (pick [B] int64: the 0-based replicate taken, -1 at valid entries and everywhere when nothing is valid;
    fallback [B] bool: the entries that missed all FILL_ATTEMPTS rejection draws and took the valid replicate of rank hash mod V)."""
    valid = np.asarray(valid, dtype=bool)
    B = len(valid)
    pick = np.full(B, -1, dtype=np.int64)
    fallback = np.zeros(B, dtype=bool)
    inv, pos = np.flatnonzero(~valid), np.flatnonzero(valid)
    if not len(inv) or not len(pos):
        return pick, fallback
    with np.errstate(over="ignore"):
        c0 = mix64(_u64(seed) ^ mix64(_u64(key) * U(2) + U(plane)) ^ (inv.astype(U) << U(20)))
        ctr = c0.copy()
        todo = np.arange(len(inv))
        for attempt in range(FILL_ATTEMPTS):
            ctr[todo] = mix64(ctr[todo] + U(attempt))
            idx = (ctr[todo] % U(B)).astype(np.int64)
            hit = valid[idx]
            pick[inv[todo[hit]]] = idx[hit]
            todo = todo[~hit]
            if not len(todo):
                break
        if len(todo):
            pick[inv[todo]] = pos[(mix64(~c0[todo]) % U(len(pos))).astype(np.int64)]
            fallback[inv[todo]] = True
    return pick, fallback


def cross_draws(seed, gene, n, nb, num_boot):
    """mm_cross_resampled with d_rep == NULL: the draws of gene ``gene`` with ``n`` good groups and ``nb`` resampled columns, as the
    tables the kernel takes instead: (rep [n][num_boot] int16 in [0, n), bcol [n][num_boot] int32 in [1, nb]); column 0 is the
    identity (rep = i, bcol = 0).  Columns >= nb are drawn by the same rule; the kernel does not read them."""
    i = np.arange(n, dtype=U)[:, None]
    c = np.arange(num_boot, dtype=U)[None, :]
    h = mix64(_u64(seed) ^ mix64((U(gene) << U(32)) ^ (i << U(24)) ^ c))
    rep = (h % U(n)).astype(np.int16)
    bcol = (mix64(h) % U(nb)).astype(np.int32) + 1
    rep[:, 0] = np.arange(n)
    bcol[:, 0] = 0
    return rep, bcol


def draws_chi2(rep, bcol, n, nb):
    """Ranges and uniformity of one gene's restated draws (columns 1.. of cross_draws): asserts 0 <= r < n and 1 <= bb <= nb, and
    returns the chi-squares of the counts of r over its n values and of bb over its nb values against equal shares, each with
    its degrees of freedom: (chi2_r, n - 1, chi2_bb, nb - 1).  Wants at least 5 expected draws per cell."""
    r, bb = rep[:, 1:].astype(np.int64).ravel(), bcol[:, 1:].astype(np.int64).ravel()
    assert r.min() >= 0 and r.max() < n and bb.min() >= 1 and bb.max() <= nb
    assert len(r) >= 5 * max(n, nb)
    out = []
    for counts in (np.bincount(r, minlength=n), np.bincount(bb - 1, minlength=nb)):
        want = len(r) / len(counts)
        out += [float(((counts - want) ** 2 / want).sum()), len(counts) - 1]
    return tuple(out)
