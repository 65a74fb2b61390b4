"""Plain numpy restatement of the single-step max-T adjustment over a family of design contrasts (``ht_1d_posthoc``,
mm_family_maxt), written from the definition in the stated arithmetic order and independent of ``memento/design.py`` and the kernel.

A family is the m contrasts of one gene; member j is a sparse design (groups, weights) over the gene's replicate rows,
coef_j[c] = sum_p w_p * y[grp_p][c] (p ascending, unfused, from 0.0).  Per plane, with scale_j = 1 / se_j for an included member and
0 otherwise:  M[c] = max_j |coef_j[c] - coef_j[0]| * scale_j over the included members (j ascending) on the family-valid columns
c >= 1 -- those where every included member is valid, i.e. all its groups are finite in BOTH planes --,  t0_j = |coef_j[0]| * scale_j,
n_adj_j = #{ c : M[c] > t0_j }  and  p_adj_j = (1 + n_adj_j) / (1 + n_valid_family)."""

import numpy as np

NAN_RECORD = np.array([np.nan, np.nan, 0.0, 0.0, np.nan, 0.0, np.nan, np.nan])


def coef_rows(ym, yv, grp, w):
    """Coefficient rows of one member on both planes from the gene's rows ym / yv [n_groups][B + 1]: -> (coef [2][B + 1], NaN in the
    columns that are not valid; ok [B + 1]).  An empty design is valid nowhere."""
    n_cols = ym.shape[1]
    coef = np.zeros((2, n_cols))
    ok = np.full(n_cols, len(grp) > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        for g, wp in zip(grp, w):
            ok &= np.isfinite(ym[g]) & np.isfinite(yv[g])
            coef[0] = coef[0] + wp * ym[g]
            coef[1] = coef[1] + wp * yv[g]
    coef[:, ~ok] = np.nan
    return coef, ok


def record(row, ok):
    """The test record (include/memento_hip.h, mm_contract_stats) of one coefficient row: [coef0, se, n_valid, n_extreme,
    mean - coef0, all_equal, n_raw_extreme, range]."""
    if not ok.any():
        return NAN_RECORD.copy()
    v = row[1:][ok[1:]]
    n = len(v)
    c0 = row[0]                                                       # (NaN when column 0 is not valid: not a test)
    allv = row[ok]
    if n == 0:
        return np.array([c0, np.nan, 0.0, 0.0, np.nan, float(allv.min() == allv.max()), 0.0, allv.max() - allv.min()])
    mean = v.sum() / n
    with np.errstate(invalid="ignore"):
        ext = (np.abs(v - c0) > abs(c0)).sum()
        raw = (np.abs(v) > abs(c0)).sum()
    return np.array([c0, np.sqrt(((v - mean) ** 2).sum() / n), n, ext, mean - c0, float(allv.min() == allv.max()), raw,
                     allv.max() - allv.min()])


def scale_of(rec):
    """1 / se where the record is a test (finite coef0, finite se > 0, n_valid >= 1, not all_equal), else 0."""
    c0, se, n, _, _, all_equal = rec[:6]
    return 1.0 / se if np.isfinite(c0) and np.isfinite(se) and se > 0 and n >= 1 and all_equal == 0 else 0.0


def family(ym, yv, designs, scale=None):
    """One family on the gene's rows ym / yv [n_groups][B + 1].  ``designs``: [(groups, weights)] per member; ``scale`` [m][2], or
    None = from the members' own records.  -> dict with ``maxrow`` [2][B + 1] (NaN in column 0 and where a column is not
    family-valid), ``t0`` [m][2], ``n_adj`` [m][2], ``n_valid`` [2], ``n_included`` [2], ``records`` [m][2][8] and ``scale`` [m][2]."""
    m, n_cols = len(designs), ym.shape[1]
    coefs, oks = [], []
    for grp, w in designs:
        c, ok = coef_rows(ym, yv, np.asarray(grp, dtype=np.int64), np.asarray(w, dtype=np.float64))
        coefs.append(c)
        oks.append(ok)
    records = np.array([[record(coefs[j][k], oks[j]) for k in range(2)] for j in range(m)]).reshape(m, 2, 8)
    if scale is None:
        scale = np.array([[scale_of(records[j, k]) for k in range(2)] for j in range(m)]).reshape(m, 2)
    scale = np.asarray(scale, dtype=np.float64).reshape(m, 2)
    maxrow = np.full((2, n_cols), np.nan)
    t0, n_adj = np.full((m, 2), np.nan), np.zeros((m, 2))
    n_valid, n_inc = np.zeros(2), np.zeros(2)
    for k in range(2):
        inc = [j for j in range(m) if np.isfinite(scale[j, k]) and scale[j, k] > 0 and oks[j][0] and np.isfinite(coefs[j][k, 0])]
        n_inc[k] = len(inc)
        if not inc:
            continue
        valid = np.ones(n_cols, dtype=bool)
        valid[0] = False
        mx = np.full(n_cols, -np.inf)
        with np.errstate(invalid="ignore", over="ignore"):
            for j in inc:                                             # ascending test order
                valid &= oks[j]
                mx = np.fmax(mx, np.abs(coefs[j][k] - coefs[j][k, 0]) * scale[j, k])
                t0[j, k] = abs(coefs[j][k, 0]) * scale[j, k]
        maxrow[k, valid] = mx[valid]
        n_valid[k] = valid.sum()
        for j in inc:
            n_adj[j, k] = (maxrow[k, valid] > t0[j, k]).sum()
    return dict(maxrow=maxrow, t0=t0, n_adj=n_adj, n_valid=n_valid, n_included=n_inc, records=records, scale=scale)


def p_adj(fam):
    """(1 + n_adj) / (1 + n_valid_family) [m][2]; NaN for a member that is not included."""
    p = (1 + fam["n_adj"]) / (1 + fam["n_valid"][None, :])
    return np.where(np.isnan(fam["t0"]), np.nan, p)


def count_pvalue(rec):
    """The count-based raw p-value of a record, (1 + n_extreme) / (1 + n_valid); NaN where the record is not a test."""
    return (1 + rec[3]) / (1 + rec[2]) if scale_of(rec) > 0 else np.nan


def near_ties(fam, rel=1e-10):
    """How many (member, family-valid column) pairs have M[c] within ``rel`` (relative) of t0: there a count could depend on rounding."""
    n = 0
    for k in range(2):
        row = fam["maxrow"][k]
        row = row[~np.isnan(row)]
        for t in fam["t0"][:, k]:
            if not np.isnan(t):
                n += int((np.abs(row - t) <= rel * t).sum())
    return n


def crit(fam, level):
    """The critical value of the simultaneous interval per plane: np.nanquantile(M[1:], level); NaN for a family without a valid column."""
    out = np.full(2, np.nan)
    for k in range(2):
        if fam["n_valid"][k] > 0:
            out[k] = np.nanquantile(fam["maxrow"][k, 1:], level)
    return out


def pairwise(n_levels):
    """All unordered pairs (a, b), a after b, ordered by b then a."""
    return [(a, b) for b in range(n_levels) for a in range(b + 1, n_levels)]
