"""Host side of K9: fold the per-gene meta-regression into one weight row per treatment column.

Everything ``_regress_1d`` / ``_regress_2d`` do before ``_compute_asl`` is LINEAR in the per-group
replicate vector (/root/reference/memento/hypothesis_test.py:262-271, :290-291, :218-228), so for a given
set of valid groups it is a fixed matrix ``W`` (T x n_groups):  coef[t, b] = sum_j W[t, j] * y[j, b].
The HIP kernel mm_contract_stats applies it; this module only builds W (tiny dense algebra, numpy).
``joint_rows`` builds, in the same way, the block of linear forms of the joint test of several treatment columns (mm_joint_stats).
"""

import numpy as np


def weight_rows(cov, trt, Nc, good, return_ss=False):
    """W (T x n_groups, zero on groups that are not ``good``) for covariates ``cov`` (n x C), treatment
    ``trt`` (n x T) and cell-count weights ``Nc`` (n,).

    all-ones treatment  -> Nc-weighted average               (hypothesis_test.py:262-265)
    otherwise           -> residualise response and treatment on [1, cov] by weighted least squares
                           (what sklearn LinearRegression(sample_weight=Nc) predicts, :269-271), then the
                           weighted slope of _cross_coef (:218-228).
    ``return_ss=True`` also returns the weighted sum of squares of the residualised treatment per column (T,): zero
    (up to round-off) when the treatment lies in the span of [1, cov] on the good groups.
    """
    cov = np.asarray(cov, dtype=np.float64)
    trt = np.asarray(trt, dtype=np.float64)
    Nc = np.asarray(Nc, dtype=np.float64)
    good = np.asarray(good, dtype=bool)
    idx = np.flatnonzero(good)
    n, T = len(idx), trt.shape[1]
    W = np.zeros((T, len(good)))
    if n == 0:
        return (W, np.zeros(T)) if return_ss else W
    c, t, w = cov[idx], trt[idx], Nc[idx]
    wbar = w / w.sum()
    if (t == 1).mean() == 1:
        W[:, idx] = wbar[None, :]
        return (W, np.full(T, np.nan)) if return_ss else W
    Xa = np.column_stack([np.ones(n), c])
    sw = np.sqrt(w)
    # hat matrix of the weighted fit: H = Xa (sw Xa)^+ sw
    H = Xa @ (np.linalg.pinv(Xa * sw[:, None]) * sw[None, :])
    M = np.eye(n) - H
    tt = M @ t                                  # residualised treatment (n x T)
    Ac = tt - wbar @ tt                         # weighted centring
    ss = wbar @ (Ac ** 2)                       # weighted sum of squares per treatment column
    center = np.eye(n) - np.outer(np.ones(n), wbar)
    with np.errstate(divide="ignore", invalid="ignore"):
        Wg = ((Ac * wbar[:, None]).T @ center @ M) / ss[:, None]
    W[:, idx] = Wg
    return (W, ss) if return_ss else W


def residual_parts(cov, trt, Nc, good):
    """For resample_rep=True (hypothesis_test.py:269-286): the residual maker M = I - H of the weighted fit on
    [1, cov] embedded in an n_groups x n_groups matrix (zero rows/columns on groups that are not ``good``), and
    the residualised treatment (T x n_groups, zero on bad groups)."""
    cov = np.asarray(cov, dtype=np.float64)
    trt = np.asarray(trt, dtype=np.float64)
    Nc = np.asarray(Nc, dtype=np.float64)
    good = np.asarray(good, dtype=bool)
    idx = np.flatnonzero(good)
    n = len(idx)
    ng = len(good)
    M = np.zeros((ng, ng))
    tt = np.zeros((trt.shape[1], ng))
    if n == 0:
        return M, tt
    Xa = np.column_stack([np.ones(n), cov[idx]])
    w = Nc[idx]
    sw = np.sqrt(w)
    H = Xa @ (np.linalg.pinv(Xa * sw[:, None]) * sw[None, :])
    Mg = np.eye(n) - H
    M[np.ix_(idx, idx)] = Mg
    # The residualised TREATMENT follows sklearn's own arithmetic (centre by the weighted means, min-norm lstsq on the
    # sqrt-weighted centred design, intercept from the offsets): groups with equal treatment then get bit-identical
    # residuals, which the degenerate resampled columns (every drawn group has the same treatment -> 0/0 -> NaN,
    # ignored by nanstd) rely on.
    c, t = cov[idx], trt[idx]
    c_off, t_off = np.average(c, axis=0, weights=w), np.average(t, axis=0, weights=w)
    coef, *_ = np.linalg.lstsq((c - c_off) * sw[:, None], (t - t_off) * sw[:, None], rcond=None)
    pred = c @ coef + (t_off - c_off @ coef)
    tt[:, idx] = (t - pred).T
    return M, tt


# singular values of the weighted residualised treatment block at or below RANK_TOL * max(1, s_max) are zero (joint_rows)
RANK_TOL = 1e-10


def joint_rows(cov, trt, Nc, good):
    """The design of the joint test of a treatment BLOCK (``ht_1d_joint``): L (r x n_groups, zero on groups that are not
    ``good``) with the statistic Q(y) = ||L y||^2 -- the weighted sum of squares of the covariate-adjusted response that the
    treatment columns explain together.

    With w = Nc / sum(Nc) on the good groups, D = diag(w), M the residual maker of the weighted fit on [1, cov] (the pinv hat
    matrix of ``weight_rows``) and the thin SVD  D^1/2 M trt = U S V':  r = #{s > RANK_TOL * max(1, s_max)} and
    L = U[:, :r]' D^1/2 M.  L [1, cov] = 0 and L D^-1 L' = I_r; Q depends on the column SPACE of the residualised block only
    (which dummy is dropped, or all dummies given: the same Q); for one column L = +-sqrt(ss) * weight_rows, so Q = ss * coef^2.
    Shape (0, n_groups) -- nothing to test -- when no group is good, when the residualised block is numerically zero (the
    treatment lies in the span of [1, cov]) and when the treatment is all ones on the good groups."""
    cov = np.asarray(cov, dtype=np.float64)
    trt = np.asarray(trt, dtype=np.float64)
    Nc = np.asarray(Nc, dtype=np.float64)
    good = np.asarray(good, dtype=bool)
    idx = np.flatnonzero(good)
    n, ng = len(idx), len(good)
    if n == 0 or trt.shape[1] == 0:
        return np.zeros((0, ng))
    c, t, w = cov[idx], trt[idx], Nc[idx]
    if (t == 1).mean() == 1:
        return np.zeros((0, ng))
    Xa = np.column_stack([np.ones(n), c])
    sw = np.sqrt(w)
    H = Xa @ (np.linalg.pinv(Xa * sw[:, None]) * sw[None, :])
    M = np.eye(n) - H
    sd = np.sqrt(w / w.sum())
    U, s, _ = np.linalg.svd(sd[:, None] * (M @ t), full_matrices=False)
    r = int((s > RANK_TOL * max(1.0, s.max())).sum())
    L = np.zeros((r, ng))
    L[:, idx] = U[:, :r].T @ (sd[:, None] * M)
    return L


# residualised-treatment sums of squares at or below this are "no stratum holds both arms" (exact zero up to round-off; the
# smallest genuine value is of the order of the smallest group's weight share)
SS_DEGENERATE = 1e-20


class VsControlDesigns:
    """Design tables of the guide-vs-control test with covariates (``ht_1d_vs_control(..., treatment_col=...)``).

    ``labels``: [n_groups][n_label_columns] label components of the groups (strings, as in the group labels);
    ``k_trt``: the treatment column; ``control``: its control value (string); ``Nc``: cells per group.
    The test of guide value ``g`` uses the groups whose treatment value is ``g`` or ``control`` (any stratum) and the design
    the reference's per-guide loop builds on that subset: intercept, the ``is_g`` indicator and main-effect dummies
    (drop_first) of every other label column, weighted by Nc.  For a gene's good groups it folds into one sparse weight row
    (weight_rows); it is built once per distinct (guide, good mask over the guide's groups) and kept in a CSR table
    (``ptr``, ``grp``, ``w``).  A design without a good guide group, without a good control group or without a stratum
    holding both arms is empty: its tests are NaN.
    """

    def __init__(self, labels, k_trt, control, Nc):
        import pandas as pd

        labels = np.asarray(labels, dtype=object).astype(str)
        self.Nc = np.asarray(Nc, dtype=np.float64)
        tv = labels[:, k_trt]
        self.ctrl_groups = np.flatnonzero(tv == str(control))
        if len(self.ctrl_groups) == 0:
            raise ValueError(f"control value {control!r} does not occur in the treatment column")
        self.guides = list(dict.fromkeys(v for v in tv if v != str(control)))          # first-appearance order
        others = [c for c in range(labels.shape[1]) if c != k_trt]
        self.sets, self.cov, self.trt = [], [], []
        for g in self.guides:
            S = np.flatnonzero((tv == g) | (tv == str(control)))
            parts = [np.ones((len(S), 0))]
            for c in others:
                parts.append(pd.get_dummies(pd.Series(labels[S, c]), drop_first=True).values.astype(np.float64))
            self.sets.append(S)
            self.cov.append(np.concatenate(parts, axis=1))
            self.trt.append((tv[S] == g).astype(np.float64)[:, None])
        self.cache = {}
        self.ptr, self.grp, self.w = [0], [], []

    def _design(self, k, mask):
        S, n_ctrl = self.sets[k], self.trt[k][:, 0] == 0
        if mask[~n_ctrl].any() and mask[n_ctrl].any():
            W, ss = weight_rows(self.cov[k], self.trt[k], self.Nc[S], mask, return_ss=True)
            if ss[0] > SS_DEGENERATE:
                w = W[0, mask]
                if mask.sum() == 2:            # one group per arm: the slope through two points is their difference, exactly
                    w = np.where(self.trt[k][mask, 0] == 1, 1.0, -1.0)
                return S[mask], w
        return np.zeros(0, np.int32), np.zeros(0)

    def tests(self, good):
        """Design id per test for the genes of ``good`` [n_genes][n_groups] (gene-major x guide), adding new designs."""
        good = np.asarray(good, dtype=bool)
        G = good.shape[0]
        out = np.empty((G, len(self.guides)), dtype=np.int32)
        for k, S in enumerate(self.sets):
            M = good[:, S]
            if M.shape[1] <= 62:
                codes = M.astype(np.int64) @ (np.int64(1) << np.arange(M.shape[1], dtype=np.int64))
                _, first, inv = np.unique(codes, return_index=True, return_inverse=True)
            else:
                _, first, inv = np.unique(np.packbits(M, axis=1), axis=0, return_index=True, return_inverse=True)
            ids = np.empty(len(first), dtype=np.int32)
            for u, row in enumerate(first):
                key = (k, M[row].tobytes())
                d = self.cache.get(key)
                if d is None:
                    grp, w = self._design(k, M[row])
                    d = self.cache[key] = len(self.ptr) - 1
                    self.grp.append(grp)
                    self.w.append(w)
                    self.ptr.append(self.ptr[-1] + len(grp))
                ids[u] = d
            out[:, k] = ids[np.asarray(inv).reshape(-1)]
        return out.reshape(-1)

    def tables(self):
        """(design_ptr int32, design_grp int32, design_w fp64) of every design built so far."""
        grp = np.concatenate(self.grp).astype(np.int32) if self.grp else np.zeros(0, np.int32)
        w = np.concatenate(self.w).astype(np.float64) if self.w else np.zeros(0)
        return np.asarray(self.ptr, dtype=np.int32), grp, w
