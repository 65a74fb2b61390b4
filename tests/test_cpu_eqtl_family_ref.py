"""CPU tests of the gene-level max-T of ``ht_1d_eqtl(adjust=True)``: the numpy restatement of mm_cross_resampled_family's rule
(``_eqtl_family_ref``) on hand cases and against its vectorised form, and the host part of the API -- families of variable size
through ``_ht.adjusted_columns``, the eGene table on a hand-built ``uns``, the argument checks and the new export."""

import os
from types import SimpleNamespace

import numpy as np
import pytest

import _eqtl_family_ref as ref
from _replicate_ref import _np_stats
from scrna_parameter_estimation_amd import _lib, engine, memento
from scrna_parameter_estimation_amd.memento import _ht, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.nan


def _same(a, b):
    for k in ("maxrow", "t0", "n_adj"):
        np.testing.assert_array_equal(np.asarray(a[k]).view(np.int64), np.asarray(b[k]).view(np.int64), err_msg=k)
    assert a["n_valid"] == b["n_valid"] and a["n_included"] == b["n_included"]


def _both(rows, coef0, scale):
    a = ref.family_loops(np.asarray(rows, dtype=np.float64), np.asarray(coef0, dtype=np.float64), np.asarray(scale, dtype=np.float64))
    _same(a, ref.family(rows, coef0, scale))
    return a


def test_an_excluded_member_in_the_middle():
    """Member 1 has scale 0: its large deviations and its NaN slot do not enter; members 0 and 2 make the row."""
    rows = [[1.0, 1.5, 0.0, 3.0, 1.0],
            [2.0, 99., NAN, -99, 2.0],
            [-1., -1., 1.0, -2., 0.0]]
    f = _both(rows, [1.0, 2.0, -1.0], [2.0, 0.0, 0.5])
    np.testing.assert_array_equal(f["maxrow"], [NAN, 1.0, 2.0, 4.0, 0.5])       # max(|v - 1| * 2, |v + 1| * 0.5)
    np.testing.assert_array_equal(f["t0"], [2.0, NAN, 0.5])
    np.testing.assert_array_equal(f["n_adj"], [1.0, 0.0, 3.0])                  # M > 2: {4}; M > 0.5: {1, 2, 4}; a tie (0.5) is not counted
    assert f["n_valid"] == 4 and f["n_included"] == 2


def test_a_nan_slot_of_one_member_is_invalid_for_all():
    rows = [[1.0, 1.5, 0.0, 3.0],
            [2.0, 2.5, NAN, 0.0]]
    f = _both(rows, [1.0, 2.0], [1.0, 1.0])
    np.testing.assert_array_equal(f["maxrow"], [NAN, 0.5, NAN, 2.0])
    np.testing.assert_array_equal(f["n_adj"], [1.0, 0.0])
    assert f["n_valid"] == 2 and f["n_included"] == 2
    # scale NaN or inf, coef0 NaN: not included, and then its NaN slot does not matter
    for c0, sc in ((2.0, NAN), (2.0, np.inf), (NAN, 1.0), (2.0, -1.0)):
        g = _both(rows, [1.0, c0], [1.0, sc])
        np.testing.assert_array_equal(g["maxrow"], [NAN, 0.5, 1.0, 2.0])
        assert g["n_valid"] == 3 and g["n_included"] == 1 and np.isnan(g["t0"][1]) and g["n_adj"][1] == 0


def test_no_included_member_no_member_and_a_single_slot():
    f = _both([[1.0, 2.0, 3.0], [1.0, 0.0, 2.0]], [1.0, 1.0], [0.0, NAN])
    assert np.isnan(f["maxrow"]).all() and np.isnan(f["t0"]).all() and not f["n_adj"].any() and f["n_valid"] == f["n_included"] == 0
    f = _both(np.zeros((0, 4)), [], [])
    assert np.isnan(f["maxrow"]).all() and len(f["t0"]) == 0 and f["n_valid"] == f["n_included"] == 0
    f = _both([[1.0], [2.0]], [1.0, 2.0], [1.0, 3.0])                           # nb = 1: the observed slot alone, no replicate
    np.testing.assert_array_equal(f["maxrow"], [NAN])
    np.testing.assert_array_equal(f["t0"], [1.0, 6.0])                          # the members are included; nothing to count
    assert not f["n_adj"].any() and f["n_valid"] == 0 and f["n_included"] == 2


def test_a_family_of_one_counts_what_its_record_counts():
    """m = 1: M[c] = |coef[c] - coef0| / se and t0 = |coef0| / se, so n_adj is the record's n_extreme and n_valid_family its
    n_valid, whenever no M[c] is within rounding of t0."""
    rng = np.random.default_rng(3)
    checked = 0
    for trial in range(40):
        row = rng.normal(0.4 * rng.normal(), 1.0, size=120)
        row[rng.integers(1, 120, size=5)] = NAN
        rec = _np_stats(row)
        f = _both(row[None, :], [rec[0]], [1.0 / rec[1]])
        assert f["n_valid"] == rec[2] and f["n_included"] == 1
        if ref.near_ties(f) == 0:
            assert f["n_adj"][0] == rec[3]
            checked += 1
    assert checked >= 35


def test_loops_against_the_vectorised_form():
    rng = np.random.default_rng(8)
    for trial in range(60):
        m, nb = int(rng.integers(1, 12)), int(rng.integers(1, 40))
        rows = rng.normal(size=(m, nb))
        rows[rng.random((m, nb)) < 0.03] = NAN
        scale = rng.uniform(0.5, 2.0, size=m)
        scale[rng.random(m) < 0.2] = rng.choice([0.0, NAN, np.inf, -1.0])
        coef0 = rows[:, 0].copy()
        f = _both(rows, coef0, scale)
        assert np.isnan(f["maxrow"][0])


def test_adjusted_columns_with_families_of_variable_size():
    """Families of 2, 0, 3 and 1 members: the family's n_valid and n_included are repeated per member by the gene's own count."""
    n_mem = np.array([2, 0, 3, 1])
    adj = np.array([[1.0, 4], [NAN, 0], [0.5, 0], [2.0, 9], [0.1, 19], [NAN, 0]])
    fam = np.array([[9.0, 1], [0.0, 0], [19.0, 3], [0.0, 0]])
    p = np.array([0.7, 0.2, 0.01, 0.3, NAN, 0.5])
    p_adj, n_family, half = _ht.adjusted_columns(p, adj[:, :], fam, n_mem)
    np.testing.assert_array_equal(p_adj, [0.7, NAN, 1 / 20, 10 / 20, NAN, NAN])   # max with the own p; NaN own p -> NaN; not included -> NaN
    np.testing.assert_array_equal(n_family, [1, 1, 3, 3, 3, 0])
    assert half is None and n_family.dtype == np.int64
    same = _ht.adjusted_columns(p[:4], adj[:4], np.array([[9.0, 1], [19.0, 3]]), 2)   # the scalar form of ht_1d_posthoc still works
    np.testing.assert_array_equal(same[0], [0.7, NAN, 1 / 20, 10 / 20])


def _uns():
    """Three genes with 3, 1 and 2 SNPs; gene g1's only member is not included on the mean plane; g2 has none on either."""
    ht = dict(gene=np.array(["g0"] * 3 + ["g1"] + ["g2"] * 2, dtype=object), snp=np.array(["a", "b", "c", "d", "e", "f"], dtype=object),
              mean_coef=np.array([1.0, -3.0, 2.0, 1.0, NAN, NAN]), mean_se=np.array([1.0, 1.5, 0.5, NAN, NAN, NAN]),
              mean_asl=np.array([0.3, 0.04, 0.001, NAN, NAN, NAN]), mean_asl_adj=np.array([0.6, 0.2, 0.01, NAN, NAN, NAN]),
              var_coef=np.array([0.1, 0.2, NAN, -0.5, NAN, NAN]), var_se=np.array([0.1, 0.1, NAN, 0.25, NAN, NAN]),
              var_asl=np.array([0.5, 0.2, NAN, 0.03, NAN, NAN]), var_asl_adj=np.array([0.7, 0.8, NAN, 0.03, NAN, NAN]),
              n_family=np.array([3, 3, 3, 0, 0, 0]), var_n_family=np.array([2, 2, 2, 1, 0, 0]))
    return SimpleNamespace(uns={"memento": {"1d_ht_eqtl": ht}})


def test_gene_table_on_a_hand_built_result():
    df = memento.get_eqtl_gene_result(_uns())
    assert list(df.columns) == ["gene", "n_snps", "n_family", "de_lead_snp", "de_coef", "de_se", "de_pval", "de_gene_pval", "de_gene_qval",
                                "dv_lead_snp", "dv_coef", "dv_se", "dv_pval", "dv_gene_pval", "dv_gene_qval"]
    assert df["gene"].tolist() == ["g0", "g1", "g2"] and df["n_snps"].tolist() == [3, 1, 2] and df["n_family"].tolist() == [3, 0, 0]
    assert df["de_lead_snp"].tolist() == ["c", None, None]                      # t0 = 1, 2, 4
    np.testing.assert_array_equal(df["de_coef"], [2.0, NAN, NAN])
    np.testing.assert_array_equal(df["de_se"], [0.5, NAN, NAN])
    np.testing.assert_array_equal(df["de_pval"], [0.001, NAN, NAN])
    np.testing.assert_array_equal(df["de_gene_pval"], [0.01, NAN, NAN])
    np.testing.assert_array_equal(df["de_gene_qval"], util._fdrcorrect(np.array([0.01, NAN, NAN])))
    assert df["dv_lead_snp"].tolist() == ["b", "d", None]                       # t0 = 1, 2 (the first of equals would be a: 1 < 2)
    np.testing.assert_array_equal(df["dv_gene_pval"], [0.7, 0.03, NAN])          # the minimum over the members, not the lead's
    np.testing.assert_array_equal(df["dv_pval"], [0.2, 0.03, NAN])
    np.testing.assert_array_equal(df["dv_gene_qval"], util._fdrcorrect(np.array([0.7, 0.03, NAN])))
    assert df["dv_gene_qval"].tolist() == [0.7, 0.06, 1.0]


def test_gene_table_needs_an_adjusted_result():
    ad = _uns()
    for k in ("mean_asl_adj", "var_asl_adj", "n_family", "var_n_family"):
        del ad.uns["memento"]["1d_ht_eqtl"][k]
    with pytest.raises(ValueError, match="adjust=True"):
        memento.get_eqtl_gene_result(ad)
    with pytest.raises(ValueError, match="adjust=True"):
        memento.get_eqtl_gene_result(SimpleNamespace(uns={"memento": {}}))
    empty = {k: v[:0] for k, v in _uns().uns["memento"]["1d_ht_eqtl"].items()}
    assert len(memento.get_eqtl_gene_result(SimpleNamespace(uns={"memento": {"1d_ht_eqtl": empty}}))) == 0


def test_adjust_checks_its_arguments_first():
    with pytest.raises(ValueError, match="adjust"):
        memento.ht_1d_eqtl(object(), None, None, adjust=True, resampling="permutation")      # (object() has no .uns: nothing is read)
    for kw in (dict(strict=True), dict(ci=0.9), dict(max_boot=20000)):
        with pytest.raises(TypeError, match=next(iter(kw))):
            memento.ht_1d_eqtl(object(), None, None, adjust=True, **kw)
    with pytest.raises(AttributeError):
        memento.ht_1d_eqtl(object(), None, None, adjust=True)                  # accepted: the call goes on to read adata


def test_export_and_header():
    hdr = open(os.path.join(ROOT, "include", "memento_hip.h")).read()
    assert "int mm_cross_resampled_family(" in hdr and "mm_cross_resampled_family" in _lib.EXPORTS
    args, _ = _lib._SIGS["mm_cross_resampled_family"]
    assert len(args) == len(_lib._SIGS["mm_cross_resampled_block"][0]) + 5      # + scale, slab, maxrow, adj, fam
    assert callable(engine.Bootstrap1D.cross_resampled_family) and callable(memento.get_eqtl_gene_result)
