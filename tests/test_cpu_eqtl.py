"""CPU tests of the host side of ``ht_1d_eqtl``: the (gene, SNP) pair list, the gene-major tables against ``design_tables``, the
weight rows as CSR designs, and the argument checks that run before ``adata`` is read."""

import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from scrna_parameter_estimation_amd import _lib, engine, memento
from scrna_parameter_estimation_amd.memento import _ht

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _genotypes(ng, n_snps, seed=0):
    rng = np.random.default_rng(seed)
    g = pd.DataFrame(rng.integers(0, 3, size=(ng, n_snps)).astype(float), columns=[f"rs{j}" for j in range(n_snps)])
    g["rs_ones"] = 1.0
    return g


def test_exports_and_header():
    hdr = open(os.path.join(ROOT, "include", "memento_hip.h")).read()
    for name in ("mm_cross_resampled_block", "mm_cross_resampled_keyed"):
        assert f"int {name}(" in hdr and name in _lib.EXPORTS
    args, res = _lib._SIGS["mm_cross_resampled_block"]
    assert len(args) == 19 and res is ctypes.c_int
    assert len(_lib._SIGS["mm_cross_resampled_keyed"][0]) == len(_lib._SIGS["mm_cross_resampled"][0]) + 1
    assert engine.CROSS_BLOCK_TT == 8 and callable(memento.ht_1d_eqtl)


def test_pair_list_as_dict_and_as_frame():
    geno = _genotypes(6, 5)
    names = ["g0", "g1", "g2", "g3"]
    as_dict = {"g0": ["rs3", "rs0"], "g2": [], "g3": ["rs4"], "not_kept": ["rs1"], "g1": ["rs_ones", "rs2", "rs0"]}
    frame = pd.DataFrame({"gene": ["g1", "g0", "not_kept", "g1", "g3", "g0", "g1"],
                          "snp": ["rs_ones", "rs3", "rs1", "rs2", "rs4", "rs0", "rs0"]})
    want = [(3, 0), (5, 2, 0), (), (4,)]
    assert _ht.eqtl_gene_columns(geno, as_dict, names) == want              # list order kept, unlisted / empty genes have no test
    assert _ht.eqtl_gene_columns(geno, frame, names) == want                # rows keep their order within a gene
    assert _ht.eqtl_gene_columns(geno, {}, names) == [(), (), (), ()]
    with pytest.raises(ValueError, match="rs9"):
        _ht.eqtl_gene_columns(geno, {"g0": ["rs0", "rs9"]}, names)
    with pytest.raises(ValueError, match="rs9"):
        _ht.eqtl_gene_columns(geno, pd.DataFrame({"gene": ["g3"], "snp": ["rs9"]}), names)
    _ht.eqtl_gene_columns(geno, {"not_kept": ["rs9"]}, names)               # a gene outside the kept set is not looked at
    with pytest.raises(ValueError):
        _ht.eqtl_gene_columns(geno, pd.DataFrame({"gene": ["g3"], "snp": ["rs1"], "x": [0]}), names)


def _eight_genes():
    """8 genes, 3 distinct good masks, a SNP list of its own per gene (one empty, one all ones on its good groups)."""
    ng = 9
    rng = np.random.default_rng(1)
    geno = _genotypes(ng, 12)
    masks = [np.ones(ng, dtype=bool), np.r_[np.ones(6, dtype=bool), np.zeros(3, dtype=bool)], np.arange(ng) % 4 != 1]
    good = np.stack([masks[k] for k in (0, 1, 2, 0, 1, 2, 0, 1)])
    cols = [(0, 1, 2), (3,), (4, 5, 6, 7, 1), (), (8, 9), (12,), (10, 11, 0, 3), (2, 5)]
    cov = rng.normal(size=(ng, 2))
    Nc = rng.integers(100, 900, size=ng).astype(np.float64)
    return good, cols, cov, np.asarray(geno.values, dtype=np.float64), Nc


@pytest.mark.parametrize("resampled", [False, True])
def test_gene_major_tables_against_design_tables(resampled):
    good, cols, cov, trt, Nc = _eight_genes()
    d = _ht.eqtl_tables(good, cols, cov, trt, Nc, resampled=resampled)
    ref = _ht.design_tables(good, cols, cov, trt, Nc, resampled=resampled)
    counts = [len(c) for c in cols]
    np.testing.assert_array_equal(d.gene_ptr, np.concatenate([[0], np.cumsum(counts)]))     # a CSR over the tests in gene order
    assert d.gene_ptr.dtype == np.int64 and d.gene_ptr[-1] == len(d.test_row) == sum(counts)
    np.testing.assert_array_equal(d.test_row, ref.test_row)
    np.testing.assert_array_equal(_bits(d.Wmat), _bits(ref.Wmat))
    if not resampled:
        assert d.tt_mat is None and d.Mstack is None and d.rr_test is None
        return
    np.testing.assert_array_equal(_bits(d.tt_mat), _bits(ref.tt_mat))
    np.testing.assert_array_equal(d.rr_test, ref.rr_test)
    assert not d.rr_test[d.test_row == 5].any() and d.rr_test[d.test_row != 5].all()       # gene 5: all ones -> the plain branch
    assert d.Mstack.shape == (3, 9, 9) and ref.Mstack.shape[0] == 8         # one residual maker per good mask, not per gene
    for k in range(len(good)):
        np.testing.assert_array_equal(_bits(d.Mstack[d.row_mask[k]]), _bits(ref.Mstack[ref.row_mask[k]]))


def test_tables_of_genes_without_groups_or_tests():
    good, cols, cov, trt, Nc = _eight_genes()
    good = good.copy()
    good[6] = False
    d = _ht.eqtl_tables(good, cols, cov, trt, Nc, resampled=True)
    assert d.Mstack.shape[0] == 4 and not d.Mstack[d.row_mask[6]].any()
    assert not d.rr_test[d.test_row == 6].any() and not d.Wmat[d.test_row == 6].any()
    none = _ht.eqtl_tables(good, [()] * 8, cov, trt, Nc, resampled=True)
    assert len(none.test_row) == 0 and none.gene_ptr.tolist() == [0] * 9 and none.tt_mat.shape == (0, 9) and none.Mstack.shape[0] == 4


def test_weight_rows_as_designs():
    good, cols, cov, trt, Nc = _eight_genes()
    good = good.copy()
    good[6] = False
    d = _ht.eqtl_tables(good, cols, cov, trt, Nc)
    test_design, ptr, grp, w = _ht.weight_row_designs(d.test_row, d.Wmat, good)
    np.testing.assert_array_equal(test_design, np.arange(len(d.test_row)))
    assert ptr[0] == 0 and ptr[-1] == len(grp) == len(w)
    for t, k in enumerate(d.test_row):
        lo, hi = ptr[t], ptr[t + 1]
        np.testing.assert_array_equal(grp[lo:hi], np.flatnonzero(good[k]))   # the gene's good groups, ascending; none: the empty design
        np.testing.assert_array_equal(_bits(w[lo:hi]), _bits(d.Wmat[t, good[k]]))
    empty = _ht.weight_row_designs(d.test_row[:0], d.Wmat[:0], good)
    assert len(empty[0]) == 0 and empty[1].tolist() == [0] and len(empty[2]) == len(empty[3]) == 0


def test_ht_1d_eqtl_checks_its_arguments_first():
    for kw in (dict(strict=True), dict(ci=0.9), dict(max_boot=20000), dict(treatment_for_gene={})):
        with pytest.raises(TypeError, match=next(iter(kw))):
            memento.ht_1d_eqtl(object(), None, None, **kw)                  # (object() has no .uns: nothing of adata is read)
    with pytest.raises(ValueError, match="rng"):
        memento.ht_1d_eqtl(object(), None, None, rng="numpy")
    sharded = SimpleNamespace(uns={"memento": {"_hip": SimpleNamespace(comm=SimpleNamespace(world=2, rank=0))}})
    with pytest.raises(NotImplementedError):
        memento.ht_1d_eqtl(sharded, None, None)
