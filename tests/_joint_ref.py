"""Plain numpy restatement of the joint test of a treatment block (``ht_1d_joint``): the design, the joint record of
mm_joint_stats and the p-values, written from the definition and independent of ``memento/design.py`` and the kernel.

With w = Nc / sum(Nc) on the good groups, D = diag(w), M the residual maker of the weighted least-squares fit on [1, cov]
and the thin SVD  D^1/2 M trt = U S V'  of rank r:  L = U[:, :r]' D^1/2 M,  Q(y) = ||L y||^2,  and over the valid replicate
columns c >= 1 the centred null  Q*_c = ||L y_c - L y_0||^2,  p = (1 + #{Q*_c > Q_0}) / (1 + n_valid)."""

import numpy as np
import scipy.stats

NAN_RECORD = np.array([np.nan, np.nan, 0.0, 0.0, np.nan, 0.0, np.nan, np.nan])
COUNT_COLUMNS = [2, 3, 5, 7]                                     # n_valid, n_extreme, all_equal, r: exact


def joint_design(cov, trt, Nc, good):
    """L on the good groups (r x n_good) and their indices.  M comes from a least-squares solve, not from a pseudo-inverse."""
    idx = np.flatnonzero(np.asarray(good, dtype=bool))
    n = len(idx)
    trt = np.asarray(trt, dtype=np.float64).reshape(len(good), -1)
    if n == 0 or trt.shape[1] == 0 or (trt[idx] == 1).all():
        return np.zeros((0, n)), idx
    w = np.asarray(Nc, dtype=np.float64)[idx]
    w = w / w.sum()
    sw = np.sqrt(w)
    X = np.column_stack([np.ones(n), np.asarray(cov, dtype=np.float64).reshape(len(good), -1)[idx]])
    beta, *_ = np.linalg.lstsq(X * sw[:, None], np.diag(sw), rcond=None)          # the weighted fit of every unit vector
    M = np.eye(n) - X @ beta
    U, s, _ = np.linalg.svd(sw[:, None] * (M @ trt[idx]), full_matrices=False)
    r = int((s > 1e-10 * max(1.0, s.max())).sum())
    return U[:, :r].T @ (sw[:, None] * M), idx


def forms(L, y):
    """L y column by column in the kernel's order: every form sums its groups in ascending order, unfused."""
    z = np.zeros((L.shape[0], y.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(L.shape[1]):
            z = z + L[:, p:p + 1] * y[p:p + 1, :]
    return z


def q_columns(L, ym, yv):
    """(Q_0, Q* [B], valid [B]) per plane for replicate rows ym / yv [n_d][B + 1] of the listed groups: -> (q0 [2], qs [2][B], ok)."""
    ok_all = np.isfinite(ym).all(axis=0) & np.isfinite(yv).all(axis=0)
    q0, qs = np.full(2, np.nan), np.full((2, ym.shape[1] - 1), np.nan)
    if L.shape[0] == 0 or L.shape[1] == 0 or not ok_all[0]:
        return q0, qs, np.zeros(ym.shape[1] - 1, dtype=bool)
    for k, y in enumerate((ym, yv)):
        z = forms(L, y)
        q = np.zeros(y.shape[1])
        q_0 = 0.0
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(L.shape[0]):                           # forms in ascending order
                q_0 = q_0 + z[j, 0] * z[j, 0]
                d = z[j] - z[j, 0]
                q = q + d * d
        q0[k], qs[k] = q_0, np.where(ok_all[1:], q[1:], np.nan)
    return q0, qs, ok_all[1:]


def record(q_0, qs, ok, r):
    """The 8 doubles of one test and plane from Q_0 and the Q* row."""
    if r == 0 or np.isnan(q_0):
        return NAN_RECORD.copy()
    v = qs[ok]
    n = len(v)
    if n == 0:
        return np.array([q_0, np.nan, 0.0, 0.0, np.nan, 0.0, np.nan, float(r)])
    mean = v.sum() / n
    return np.array([q_0, np.sqrt(((v - mean) ** 2).sum() / n), n, (v > q_0).sum(), mean, float((v == 0).all()), v.max(), float(r)])


def joint_records(L, ym, yv):
    """Both records (mean plane, variability plane) of one test."""
    q0, qs, ok = q_columns(L, ym, yv)
    r = L.shape[0] if L.shape[1] else 0
    return record(q0[0], qs[0], ok, r), record(q0[1], qs[1], ok, r)


def near_ties(q_0, qs, ok, rel=1e-10):
    """How many valid Q* lie within ``rel`` * Q_0 of Q_0: there a count could depend on rounding."""
    return int((np.abs(qs[ok] - q_0) <= rel * q_0).sum())


def pvalues(rec, approx=False):
    """P-value of records [test][8]: the count, or the Satterthwaite fit a chi2_nu with a = s^2 / (2 m), nu = 2 m^2 / s^2."""
    rec = np.atleast_2d(rec)
    p = np.full(len(rec), np.nan)
    for t, (q_0, s, n, ext, mean, all_equal, _, _) in enumerate(rec):
        if np.isnan(q_0) or n < 1 or all_equal == 1:
            continue
        if approx:
            p[t] = scipy.stats.chi2.sf(q_0 / (s * s / (2 * mean)), 2 * mean * mean / (s * s)) if s > 0 else np.nan
        else:
            p[t] = (1 + ext) / (1 + n)
    return p
