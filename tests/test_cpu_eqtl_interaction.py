"""CPU tests of ``ht_1d_eqtl(interaction=...)``: the numpy restatement of the per-test-covariate coefficient (``_eqtl_cov_ref``)
against a direct fit, the host tables (``_ht.eqtl_interaction_tables``) against ``design.weight_rows`` / ``design.residual_parts`` on
the full per-test design, and the argument checks that run before ``adata`` is read."""

import ctypes
import inspect
import os
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

import _eqtl_cov_ref as ref
from scrna_parameter_estimation_amd import _lib, engine, memento
from scrna_parameter_estimation_amd.memento import _ht, design

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-11, atol=1e-12)      # the project's tolerance for a sum in another order (tests/test_gpu_eqtl_block.py)


def test_exports_header_and_limits():
    hdr = open(os.path.join(ROOT, "include", "memento_hip.h")).read()
    for name in ("mm_cross_cov_beta", "mm_cross_resampled_block_cov", "mm_residualize_rank1"):
        assert f"int {name}(" in hdr and name in _lib.EXPORTS
    assert len(_lib._SIGS["mm_cross_resampled_block_cov"][0]) == len(_lib._SIGS["mm_cross_resampled_block"][0]) + 4      # zt, tile_lo, tile_hi, beta
    assert _lib._SIGS["mm_cross_cov_beta"][1] is ctypes.c_int
    # 140 bytes of LDS per group (tt and zt tiles, Nc, the good list) and 8 more: the largest n_groups inside 64 KB
    assert engine.CROSS_COV_MAX_GROUPS == (64 * 1024 - 8) // (2 * engine.CROSS_BLOCK_TT * 8 + 12) == 468
    assert ref.TT == engine.CROSS_BLOCK_TT


# ----------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------


def _wls_slope_after(y, cols, a, w):
    """The coefficient of ``a`` in the weighted least-squares fit of y on [1 | cols | a]."""
    X = np.column_stack([np.ones(len(y)), cols, a]) * np.sqrt(w)[:, None]
    return np.linalg.lstsq(X, y * np.sqrt(w), rcond=None)[0][-1]


def test_restatement_column_zero_is_the_fit_with_the_covariate():
    """Column 0 (the identity draw) of ``cov_row`` on a plane residualised on [1 | c] with z = M g and tt the fully residualised
    treatment is the coefficient of ``a`` in the weighted fit of y on [1 | c | g | a]; with z = 0 it is the fit without g; and y_t is
    W-orthogonal to z."""
    rng = np.random.default_rng(3)
    ng, B = 12, 20
    good = np.ones(ng, dtype=bool)
    good[[2, 9]] = False
    idx = np.flatnonzero(good)
    Nc = rng.integers(200, 900, size=ng).astype(np.float64)
    c, g, a = rng.normal(size=(ng, 1)), rng.integers(0, 3, size=ng).astype(float), rng.normal(size=ng)
    y = rng.normal(size=(ng, B + 1))
    M, res = design.residual_parts(c, np.column_stack([g, a]), Nc, good)
    z, at = res
    w = Nc[idx]
    tt = np.zeros(ng)
    tt[idx] = at[idx] - z[idx] * (w * z[idx] * at[idx]).sum() / (w * z[idx] ** 2).sum()
    rep, bcol = ref.cross_draws(5, 0, len(idx), B, B)
    row, bound, y_t = ref.cov_row(M @ y, z, tt, Nc, good, rep, bcol, None, B, B)
    want = _wls_slope_after(y[idx, 0], np.column_stack([c[idx], g[idx]]), a[idx], w)
    np.testing.assert_allclose(float(row[0]), want, **TOL)
    assert np.isfinite(row[:B].astype(np.float64)).all() and np.isnan(row[B])                  # nb = B slots: 0 observed, 1..B - 1 resampled
    assert (bound[:B] > 0).all() and float(bound[:B].max()) < 1e-12
    np.testing.assert_allclose((w[:, None] * z[idx, None] * y_t[idx]).sum(axis=0).astype(np.float64), 0, atol=1e-9)
    row0, _, y_0 = ref.cov_row(M @ y, np.zeros(ng), at, Nc, good, rep, bcol, None, B, B)
    np.testing.assert_allclose(float(row0[0]), _wls_slope_after(y[idx, 0], c[idx], a[idx], w), **TOL)
    np.testing.assert_array_equal(y_0[idx].astype(np.float64), (M @ y)[idx])


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("B", [63, 64, 65, 257])
def test_restatement_decides_the_counts_of_the_kernel_problem(B, dropped):
    """On the inputs of tests/test_gpu_eqtl_cov_block.py the bounds leave at most 1 % of the (test, column) cells too close to a count's
    threshold to decide, the degenerate-column test has fewer valid columns than its neighbours, and the zero-covariate test is
    the plain coefficient."""
    ng = 12
    yt, good, gene_ptr, tt, zt, Nc, col_map, n_valid = ref.cov_problem(B, ng)
    if dropped:
        yt = ref.poison_dropped(yt, good, col_map, n_valid)
    else:
        col_map = n_valid = None
    rep, bcol = ref.draw_tables(good, n_valid, B, ref.SEED, ref.KEYS)
    rows, bounds = ref.cov_rows(yt, good, gene_ptr, tt, zt, Nc, rep, bcol, col_map, n_valid, B)
    cells = int((~np.isnan(rows[:, 1:])).sum())
    open_cells = sum(ref.count_limits(r, b)[2] for r, b in zip(rows, bounds))
    print(f"B {B} dropped {dropped}: {open_cells} of {cells} cells undecided, largest bound {float(np.nanmax(bounds)):.3g}")
    assert cells > 20 * B and open_cells <= 0.01 * cells
    valid = (~np.isnan(rows[:, 1:])).sum(axis=1)
    assert 0 < valid[1] < valid[0] == valid[2]
    plain, _ = ref.cov_rows(yt, good, gene_ptr, tt, np.zeros_like(zt), Nc, rep, bcol, col_map, n_valid, B)
    np.testing.assert_array_equal(rows[ref.ZERO_Z_TEST].astype(np.float64), plain[ref.ZERO_Z_TEST].astype(np.float64))
    assert (rows[0, :5] != plain[0, :5]).all()


# ----------------------------------------------------------------------------------------------
# the host tables
# ----------------------------------------------------------------------------------------------


def _design_problem(seed=0):
    """24 groups = 12 donors x 2 contexts, 2 bad under the second mask; SNP 0..5 genuine, 6 with carriers in context 1 only, 7
    monomorphic, 8 equal to the second covariate (inside the shared span: no covariate, and an interaction that is a genuine test)."""
    rng = np.random.default_rng(seed)
    ng = 24
    ctx = np.tile([0.0, 1.0], 12)
    donor_g = rng.integers(0, 3, size=(12, 9)).astype(float)
    donor_g[:, 0] = np.arange(12) % 3
    trt = np.repeat(donor_g, 2, axis=0)
    trt[:, 6] = np.where(ctx == 1, trt[:, 6].clip(0, 1) + (np.arange(ng) % 4 == 1), 0.0)
    trt[:, 7] = 2.0
    cov = np.column_stack([rng.normal(size=ng), np.repeat(rng.integers(0, 2, size=12), 2).astype(float)])
    trt[:, 8] = cov[:, 1]
    Nc = rng.integers(200, 900, size=ng).astype(np.float64)
    good = np.ones((4, ng), dtype=bool)
    good[1, [4, 17]] = False
    good[3] = False
    cols = [(0, 1, 2, 6, 7), (3, 0, 6, 5, 8), (), (1, 2)]
    return ng, ctx, trt, cov, Nc, good, cols


@pytest.mark.parametrize("ctx_in_cov", [False, True])
def test_tables_against_the_full_per_test_design(ctx_in_cov):
    """Per (mask, SNP): the weight row is ``design.weight_rows`` on [cov | ctx | g_s] with treatment g_s * ctx, zt and tt are the
    residual parts of g_s on [cov | ctx] and of g_s * ctx on [cov | ctx | g_s]; the degenerate designs have no test and zero rows;
    one maker per mask; ctx among the covariates as well changes nothing."""
    ng, ctx, trt, cov, Nc, good, cols = _design_problem()
    cov_in = np.column_stack([cov, ctx]) if ctx_in_cov else cov
    d = _ht.eqtl_interaction_tables(good, cols, cov_in, ctx, trt, Nc)
    assert d.gene_ptr.tolist() == [0, 5, 10, 10, 12] and d.test_row.tolist() == [0] * 5 + [1] * 5 + [3] * 2
    assert d.Mstack.shape == (3, ng, ng) and d.row_mask.tolist() == [0, 1, 0, 2]
    flat = [j for k in cols for j in k]
    assert d.has_test.tolist() == [True, True, True, False, False, True, True, False, True, True, False, False]
    worst = dict(W=0.0, zt=0.0, tt=0.0)
    for t, (k, s) in enumerate(zip(d.test_row, flat)):
        g, a = trt[:, s], trt[:, s] * ctx
        full = np.column_stack([cov, ctx, g])
        np.testing.assert_allclose(d.Mstack[d.row_mask[k]], design.residual_parts(np.column_stack([cov, ctx]), a[:, None], Nc, good[k])[0], **TOL)
        if not d.has_test[t]:
            assert not d.tt_mat[t].any() and not d.Wmat[t].any()
            if good[k].any():
                W, ss = design.weight_rows(full, a[:, None], Nc, good[k], return_ss=True)
                assert ss[0] <= design.SS_DEGENERATE
            continue
        W, ss = design.weight_rows(full, a[:, None], Nc, good[k], return_ss=True)
        assert ss[0] > 1e-3
        z_ref = design.residual_parts(np.column_stack([cov, ctx]), g[:, None], Nc, good[k])[1][0]
        tt_ref = design.residual_parts(full, a[:, None], Nc, good[k])[1][0]
        if s == 8:                                                             # g = a covariate: inside the shared span, taken as exactly zero
            assert np.abs(z_ref).max() < 1e-12 and not d.zt_mat[t].any()
        else:
            np.testing.assert_allclose(d.zt_mat[t], z_ref, **TOL)
        np.testing.assert_allclose(d.Wmat[t], W[0], **TOL)
        np.testing.assert_allclose(d.tt_mat[t], tt_ref, **TOL)
        assert not d.Wmat[t][~good[k]].any() and not d.tt_mat[t][~good[k]].any() and not d.zt_mat[t][~good[k]].any()
        for name, got, want in (("W", d.Wmat[t], W[0]), ("zt", d.zt_mat[t], z_ref if s != 8 else 0 * z_ref), ("tt", d.tt_mat[t], tt_ref)):
            worst[name] = max(worst[name], float(np.abs(got - want).max()))
    print("largest differences from the full per-test design:", {k: f"{v:.2g}" for k, v in worst.items()})


def test_tables_constant_context_all_ones_and_nothing():
    ng, ctx, trt, cov, Nc, good, cols = _design_problem()
    d = _ht.eqtl_interaction_tables(good, cols, cov, np.ones(ng), trt, Nc)      # a constant context: g * ctx = g, no test anywhere
    assert not d.has_test.any() and not d.Wmat.any()
    ones = np.ones((ng, 1))
    d = _ht.eqtl_interaction_tables(good[:1], [(0,)], cov, np.ones(ng), ones, Nc)                         # treatment all ones
    assert d.has_test.tolist() == [False]
    d = _ht.eqtl_interaction_tables(good[:0], [], cov, ctx, trt, Nc)
    assert d.gene_ptr.tolist() == [0] and d.Wmat.shape == d.zt_mat.shape == d.tt_mat.shape == (0, ng) and d.Mstack.shape == (0, ng, ng)


# ----------------------------------------------------------------------------------------------
# arguments
# ----------------------------------------------------------------------------------------------


def test_signature_and_docstring():
    sig = inspect.signature(memento.ht_1d_eqtl)
    assert "interaction" in sig.parameters and sig.parameters["interaction"].default is None
    assert list(sig.parameters)[-2:] == ["interaction", "not_offered"]
    doc = memento.ht_1d_eqtl.__doc__
    for word in ("interaction", "SS_DEGENERATE", "NotImplementedError", "``adjust=True`` together with ``resample_rep=True``"):
        assert word in doc                                                     # what is not offered is said
    assert "zt" in engine.Bootstrap1D.cross_resampled_family.__doc__


def test_interaction_is_checked_before_adata_is_read():
    fake = SimpleNamespace(uns={"memento": {"groups": list("abcdef")}})         # (no '_hip': nothing else of adata is read)
    for bad in (np.zeros(5), np.zeros((6, 2)), pd.DataFrame(np.zeros((6, 2))), np.r_[np.zeros(5), np.nan], np.r_[np.zeros(5), np.inf]):
        with pytest.raises(ValueError, match="interaction"):
            memento.ht_1d_eqtl(fake, None, None, interaction=bad)
    with pytest.raises(NotImplementedError, match="interaction"):
        memento.ht_1d_eqtl(object(), None, None, interaction=np.zeros(6), adjust=True, resample_rep=True)
    for ok in (np.arange(6.0), pd.Series(np.arange(6.0)), pd.DataFrame({"stim": np.arange(6.0)}), np.arange(6.0)[:, None]):
        np.testing.assert_array_equal(_ht.interaction_context(ok, 6), np.arange(6.0))


def test_engine_checks_zt_on_the_host():
    """zt of another shape, a non-finite zt and too many groups raise before anything is uploaded."""
    ng, B = 6, 40
    tt, good = np.ones((4, ng)), np.ones((2, ng), dtype=bool)
    args = (B, ng, 2, [0, 2, 4], tt, good, [0, 0], np.zeros((1, ng, ng)), np.ones(ng), None, None, None, None)
    assert engine._block_tables(*args, zt=np.zeros((4, ng)))[-1].shape == (4, ng)
    bad = np.zeros((4, ng))
    bad[2, 1] = np.nan
    for zt in (np.zeros((3, ng)), np.zeros((4, ng + 1)), bad):
        with pytest.raises(ValueError, match="zt"):
            engine._block_tables(*args, zt=zt)
    ng = engine.CROSS_COV_MAX_GROUPS + 1
    big = (B, ng, 1, [0, 1], np.ones((1, ng)), np.ones((1, ng), dtype=bool), [0], np.zeros((1, ng, ng)), np.ones(ng), None, None, None, None)
    engine._block_tables(*big)
    with pytest.raises(NotImplementedError):
        engine._block_tables(*big, zt=np.zeros((1, ng)))
