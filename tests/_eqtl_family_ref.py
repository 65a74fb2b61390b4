"""Plain numpy restatement of the single-step max-T over the resampled tests of one gene (``ht_1d_eqtl(adjust=True)``,
mm_cross_resampled_family), written from the rule in include/memento_hip.h and independent of the kernel.

A family is the m tests of one gene.  ``rows`` [m][nb] holds the slots of the resampled coefficient rows that the record is taken
over: slot 0 the observed coefficient, slots 1..nb - 1 the replicates, NaN where a slot is degenerate for that member.  With
``coef0`` [m] (the record's, equal to rows[:, 0]) and ``scale`` [m] (1 / se, or 0 for no test):
  member j is included when scale_j is finite and > 0 and coef0_j is finite;  t0_j = |coef0_j| * scale_j, NaN if not;
  slot c >= 1 is family-valid when no included member is NaN there;
  M[c] = max_j |rows[j][c] - coef0_j| * scale_j over the included members, j ascending, on the family-valid slots, NaN elsewhere;
  n_adj_j = #{family-valid c : M[c] > t0_j}.
A family without an included member (or without a member, or with nb < 1) has an all-NaN row and zero counts."""

import numpy as np


def family_loops(rows, coef0, scale):
    """The rule as plain loops -> dict(maxrow [nb], t0 [m], n_adj [m], n_valid, n_included)."""
    rows = np.asarray(rows, dtype=np.float64)
    m = len(coef0)
    nb = rows.shape[1] if rows.ndim == 2 else 0
    inc = [bool(np.isfinite(scale[j]) and scale[j] > 0 and np.isfinite(coef0[j])) for j in range(m)]
    t0 = np.array([abs(coef0[j]) * scale[j] if inc[j] else np.nan for j in range(m)], dtype=np.float64)
    maxrow = np.full(nb, np.nan)
    n_valid = 0
    if any(inc):
        for c in range(1, nb):
            ok, mx = True, -np.inf
            for j in range(m):
                if not inc[j]:
                    continue
                v = rows[j, c]
                if np.isnan(v):
                    ok = False
                    continue
                mx = max(mx, abs(v - coef0[j]) * scale[j])
            if ok:
                maxrow[c] = mx
                n_valid += 1
    n_adj = np.zeros(m)
    for j in range(m):
        if inc[j]:
            n_adj[j] = sum(1 for c in range(1, nb) if maxrow[c] > t0[j])      # (NaN on either side: not counted)
    return dict(maxrow=maxrow, t0=t0, n_adj=n_adj, n_valid=float(n_valid), n_included=float(sum(inc)))


def family(rows, coef0, scale):
    """The same rule vectorised over the slots (what the tests of larger problems use; pinned against ``family_loops``)."""
    rows = np.asarray(rows, dtype=np.float64)
    coef0, scale = np.asarray(coef0, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    m = len(coef0)
    nb = rows.shape[1] if rows.ndim == 2 else 0
    with np.errstate(invalid="ignore"):
        inc = np.isfinite(scale) & (scale > 0) & np.isfinite(coef0)
        t0 = np.where(inc, np.abs(coef0) * scale, np.nan)
    maxrow = np.full(nb, np.nan)
    n_adj = np.zeros(m)
    if inc.any() and nb > 1:
        r = rows[inc]
        valid = ~np.isnan(r).any(axis=0)
        valid[0] = False
        mx = np.full(nb, -np.inf)
        with np.errstate(invalid="ignore"):
            for j in range(len(r)):                                           # ascending member order
                mx = np.fmax(mx, np.abs(r[j] - coef0[inc][j]) * scale[inc][j])
        maxrow[valid] = mx[valid]
        with np.errstate(invalid="ignore"):
            n_adj[inc] = (maxrow[None, valid] > t0[inc][:, None]).sum(axis=1)
    return dict(maxrow=maxrow, t0=t0, n_adj=n_adj, n_valid=float((~np.isnan(maxrow)).sum()), n_included=float(inc.sum()))


def near_ties(fam, rel=1e-10):
    """How many (member, family-valid slot) pairs have M[c] within ``rel`` (relative) of t0: there a count could depend on rounding."""
    row = fam["maxrow"][~np.isnan(fam["maxrow"])]
    return sum(int((np.abs(row - t) <= rel * t).sum()) for t in fam["t0"] if not np.isnan(t))
