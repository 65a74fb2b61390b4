"""CPU tests of the host side of ``ci=`` (percentile intervals of the ht_* coefficients): the level check ``_ht.ci_probs``, that
every driver runs it before it touches its data, and the result getters, which add the interval columns if and only if the
interval arrays are in ``uns``.  No device: the getters read a hand-built ``uns`` dict."""

from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from scrna_parameter_estimation_amd import memento
from scrna_parameter_estimation_amd.memento import _ht

KEYS_1D = ["de_coef", "de_se", "de_pval", "dv_coef", "dv_se", "dv_pval"]
KEYS_2D = ["corr_coef", "corr_se", "corr_pval"]


def test_ci_probs():
    assert _ht.ci_probs(None) is None
    lo, hi = _ht.ci_probs(0.95)
    assert abs(lo - 0.025) <= 1e-15 and abs(hi - 0.975) <= 1e-15
    lo, hi = _ht.ci_probs(np.float32(0.5))
    assert (lo, hi) == (0.25, 0.75) and type(lo) is float
    for level in (1e-9, 0.9, 1 - 1e-9):
        lo, hi = _ht.ci_probs(level)
        assert 0 < lo < 0.5 < hi < 1 and abs((hi - lo) - level) <= 1e-15 and abs((lo + hi) - 1) <= 1e-15


@pytest.mark.parametrize("bad", [0, 1, 0.0, 1.0, -0.1, 1.5, 95, float("nan"), float("inf"), "x", "0.9", True, [0.9], (0.05, 0.95)])
def test_ci_probs_rejects(bad):
    with pytest.raises(ValueError, match="ci must be"):
        _ht.ci_probs(bad)


@pytest.mark.parametrize("bad", [0, 1, "x"])
def test_every_driver_checks_ci_before_it_reads_anything(bad):
    """``adata`` is an object without ``uns``: whatever touches it raises AttributeError, the level check comes first."""
    nothing = object()
    with pytest.raises(ValueError, match="ci must be"):
        memento.ht_1d_moments(nothing, None, None, resampling="bootstrap", ci=bad)
    with pytest.raises(ValueError, match="ci must be"):
        memento.ht_2d_moments(nothing, None, None, resampling="bootstrap", ci=bad)
    with pytest.raises(ValueError, match="ci must be"):
        memento.ht_1d_vs_control(nothing, 0, ci=bad)
    with pytest.raises(ValueError, match="ci must be"):
        memento.ht_2d_vs_control(nothing, 0, ci=bad)
    with pytest.raises(AttributeError):                             # a valid level gets past the check
        memento.ht_1d_vs_control(nothing, 0, ci=0.9)


def test_ci_over_several_ranks_is_refused_up_front():
    """Gathering intervals across ranks is not built: the two calls that run gene- or pair-sharded say so before they read the
    moments (the stand-in has none: anything further raises KeyError)."""
    st = SimpleNamespace(comm=SimpleNamespace(world=2, rank=0))
    adata = SimpleNamespace(uns={"memento": {"_hip": st}})
    with pytest.raises(NotImplementedError, match="ci="):
        memento.ht_1d_moments(adata, None, None, resampling="bootstrap", ci=0.9)
    with pytest.raises(NotImplementedError, match="ci="):
        memento.ht_2d_moments(adata, None, None, resampling="bootstrap", ci=0.9)
    with pytest.raises(KeyError):                                   # without ci= the call goes on as before
        memento.ht_1d_moments(adata, None, None, resampling="bootstrap")


def _uns_1d(with_ci):
    names = ["g0", "g1", "g2"]
    trt = pd.DataFrame({"a": [0.0, 1.0], "b": [1.0, 0.0]})
    n = len(names) * 2
    ht = {"gene_names": names, "treatment": trt, "covariate": None}
    for i, k in enumerate(("mean_coef", "mean_se", "mean_asl", "var_coef", "var_se", "var_asl")):
        ht[k] = np.arange(n) + 10.0 * i
    if with_ci:
        ht["mean_ci"] = np.column_stack([np.arange(n) - 0.5, np.arange(n) + 0.5])
        ht["var_ci"] = np.column_stack([np.arange(n) + 29.0, np.arange(n) + 31.0])
        ht["mean_ci"][3] = np.nan
        ht["ci"] = 0.9
    return SimpleNamespace(uns={"memento": {"1d_ht": ht}}), ht


def test_get_1d_ht_result_adds_the_interval_columns_iff_the_keys_are_there():
    adata, ht = _uns_1d(False)
    df = memento.get_1d_ht_result(adata)
    assert list(df.columns) == ["gene", "tx"] + KEYS_1D and len(df) == 6
    adata, ht = _uns_1d(True)
    df = memento.get_1d_ht_result(adata)
    assert list(df.columns) == ["gene", "tx"] + KEYS_1D + ["de_ci_lo", "de_ci_hi", "dv_ci_lo", "dv_ci_hi"]
    np.testing.assert_array_equal(df["de_ci_lo"].values, ht["mean_ci"][:, 0])
    np.testing.assert_array_equal(df["de_ci_hi"].values, ht["mean_ci"][:, 1])
    np.testing.assert_array_equal(df["dv_ci_lo"].values, ht["var_ci"][:, 0])
    np.testing.assert_array_equal(df["dv_ci_hi"].values, ht["var_ci"][:, 1])
    np.testing.assert_array_equal(df["de_coef"].values, ht["mean_coef"])         # the other columns are what they were
    assert np.isnan(df["de_ci_lo"].values[3]) and np.isnan(df["de_ci_hi"].values[3])


def test_get_2d_ht_result_adds_the_interval_columns_iff_the_key_is_there():
    pairs = [("g0", "g1"), ("g1", "g2"), ("g2", "g2")]
    ht = {"corr_coef": np.array([0.1, -0.2, np.nan]), "corr_se": np.array([0.01, 0.02, np.nan]), "corr_asl": np.array([0.5, 0.04, np.nan])}
    adata = SimpleNamespace(uns={"memento": {"2d_moments": {"gene_pairs": pairs}, "2d_ht": ht}})
    df = memento.get_2d_ht_result(adata)
    assert list(df.columns) == ["gene_1", "gene_2"] + KEYS_2D
    ht["corr_ci"] = np.array([[0.05, 0.15], [-0.3, -0.1], [np.nan, np.nan]])
    ht["ci"] = 0.9
    df = memento.get_2d_ht_result(adata)
    assert list(df.columns) == ["gene_1", "gene_2"] + KEYS_2D + ["corr_ci_lo", "corr_ci_hi"]
    np.testing.assert_array_equal(df["corr_ci_lo"].values, ht["corr_ci"][:, 0])
    np.testing.assert_array_equal(df["corr_ci_hi"].values, ht["corr_ci"][:, 1])
    np.testing.assert_array_equal(df["corr_coef"].values, ht["corr_coef"])


def test_the_library_exports_the_entry_point():
    import os

    from scrna_parameter_estimation_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "memento_hip.h")).read()
    assert "int mm_row_quantiles(" in hdr and "mm_row_quantiles" in _lib.EXPORTS
    assert hasattr(_lib.load(require_gpu=False), "mm_row_quantiles")
    assert "`mm_row_quantiles`" in open(os.path.join(root, "INTEGRATION.md")).read()
