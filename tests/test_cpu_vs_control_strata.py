"""CPU tests of the guide-vs-control test with covariates (ht_1d_vs_control(..., treatment_col=...)): the host design tables
equal design.weight_rows on each test's subset design (the reference's per-guide loop: subset to {guide, control},
create_groups([is_guide, rep]), covariates intercept + rep dummies), and the C-ABI declares and binds the new entry points."""

import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grouping():
    """guide 0 = control, guides 1..3, replicates 0..2; guide 3 has no cells in replicate 2 (a missing stratum).  Group order
    is a shuffled first-appearance order, as create_groups produces it."""
    labels = [(g, r) for g in range(4) for r in range(3) if not (g == 3 and r == 2)]
    order = np.random.default_rng(3).permutation(len(labels))
    labels = [[str(labels[i][0]), str(labels[i][1])] for i in order]
    Nc = np.random.default_rng(4).integers(50, 400, size=len(labels)).astype(float)
    return labels, Nc


def _good(labels):
    ng = len(labels)
    idx = {(int(a), int(b)): j for j, (a, b) in enumerate(labels)}
    good = np.ones((5, ng), dtype=bool)
    good[1, idx[1, 0]] = False                                   # gene 1: a bad guide stratum
    good[2, [idx[0, r] for r in range(3)]] = False               # gene 2: no good control group -> every guide NaN
    good[3, [idx[2, 1], idx[2, 2], idx[0, 0]]] = False           # gene 3: guide 2 only in rep 0, control only in reps 1, 2
    good[4, idx[3, 0]] = False                                   # gene 4: guide 3 keeps rep 1 only
    return good, idx


def _expected(labels, Nc, good_row, guide):
    """weight_rows on the reference's subset design for one (gene, guide); None where the test is NaN."""
    from scrna_parameter_estimation_amd.memento import design

    lab = np.array(labels)
    S = np.flatnonzero((lab[:, 0] == guide) | (lab[:, 0] == "0"))
    sub = pd.DataFrame({"is_g": (lab[S, 0] == guide).astype(int), "rep": lab[S, 1]})
    cov = np.column_stack([np.ones(len(S)), pd.get_dummies(sub["rep"], drop_first=True).values.astype(float)])
    trt = sub[["is_g"]].values.astype(float)
    mask = good_row[S]
    if not (mask & (trt[:, 0] == 1)).any() or not (mask & (trt[:, 0] == 0)).any():
        return None
    W, ss = design.weight_rows(cov, trt, Nc[S], mask, return_ss=True)
    if ss[0] <= 1e-20:
        return None
    full = np.zeros(len(labels))
    full[S] = W[0]
    return full, S[mask]


def test_design_tables_equal_weight_rows_on_each_subset():
    from scrna_parameter_estimation_amd.memento import design

    labels, Nc = _grouping()
    good, idx = _good(labels)
    d = design.VsControlDesigns(labels, 0, "0", Nc)
    assert d.guides == list(dict.fromkeys(l[0] for l in labels if l[0] != "0"))
    test_design = d.tests(good)
    ptr, grp, w = d.tables()
    assert ptr.dtype == np.int32 and grp.dtype == np.int32 and w.dtype == np.float64
    assert ptr[0] == 0 and ptr[-1] == len(grp) == len(w) and (np.diff(ptr) >= 0).all()
    n_guides = len(d.guides)
    assert len(test_design) == good.shape[0] * n_guides
    nan_tests = set()
    for gene in range(good.shape[0]):
        for k, guide in enumerate(d.guides):
            t = gene * n_guides + k                             # gene-major x guide
            dd = test_design[t]
            got = np.zeros(len(labels))
            got[grp[ptr[dd]:ptr[dd + 1]]] = w[ptr[dd]:ptr[dd + 1]]
            want = _expected(labels, Nc, good[gene], guide)
            if want is None:
                assert ptr[dd + 1] == ptr[dd], (gene, guide)
                nan_tests.add((gene, guide))
                continue
            # the design lists exactly the test's good groups (validity is checked over all of them, zero weights included)
            assert sorted(grp[ptr[dd]:ptr[dd + 1]].tolist()) == sorted(want[1].tolist())
            np.testing.assert_allclose(got, want[0], rtol=1e-10, atol=1e-12, err_msg=f"gene {gene} guide {guide}")
    assert nan_tests == {(2, "1"), (2, "2"), (2, "3"), (3, "2")}
    # with no bad groups the treatment is the guide-vs-control contrast, adjusted for the replicate: the weights of each arm sum
    # to +1 / -1 and the weights are orthogonal to every replicate indicator of the design
    lab = np.array(labels)
    dd = test_design[0]
    wrow = np.zeros(len(labels))
    wrow[grp[ptr[dd]:ptr[dd + 1]]] = w[ptr[dd]:ptr[dd + 1]]
    g1 = lab[:, 0] == d.guides[0]
    np.testing.assert_allclose(wrow[g1].sum(), 1.0, rtol=1e-12)
    np.testing.assert_allclose(wrow[lab[:, 0] == "0"].sum(), -1.0, rtol=1e-12)
    for r in "012":
        np.testing.assert_allclose(wrow[lab[:, 1] == r].sum(), 0.0, atol=1e-12)


def test_design_cache_builds_one_design_per_guide_and_mask():
    from scrna_parameter_estimation_amd.memento import design

    labels, Nc = _grouping()
    good, _ = _good(labels)
    d = design.VsControlDesigns(labels, 0, "0", Nc)
    many = np.repeat(good, 50, axis=0)                           # 250 genes, the same 5 masks
    ids = d.tests(many).reshape(250, -1)
    distinct = {(k, many[i][d.sets[k]].tobytes()) for i in range(250) for k in range(len(d.guides))}
    assert len(d.ptr) - 1 == len(distinct)
    ids2 = d.tests(good).reshape(5, -1)                         # a later gene chunk reuses the designs
    assert len(d.ptr) - 1 == len(distinct)
    np.testing.assert_array_equal(ids[::50], ids2)


def test_design_single_label_column_is_the_plain_difference():
    from scrna_parameter_estimation_amd.memento import design

    labels = [["3"], ["0"], ["1"], ["2"]]
    d = design.VsControlDesigns(labels, 0, 0, np.array([10.0, 40.0, 25.0, 7.0]))
    ids = d.tests(np.ones((1, 4), dtype=bool))
    ptr, grp, w = d.tables()
    for k, g in enumerate(d.guides):
        dd = ids[k]
        row = dict(zip(grp[ptr[dd]:ptr[dd + 1]].tolist(), w[ptr[dd]:ptr[dd + 1]].tolist()))
        assert set(row) == {1, labels.index([g])}
        np.testing.assert_allclose([row[labels.index([g])], row[1]], [1.0, -1.0], rtol=1e-13)


def test_design_rejects_an_absent_control_value():
    from scrna_parameter_estimation_amd.memento import design

    with pytest.raises(ValueError):
        design.VsControlDesigns([["1", "0"], ["2", "0"]], 0, "0", np.ones(2))


def test_cabi_declares_and_binds_the_design_contrast():
    hdr = open(os.path.join(ROOT, "include", "memento_hip.h")).read()
    declared = set(re.findall(r"\b(mm_[a-z0-9_]+)\s*\(", hdr))
    from scrna_parameter_estimation_amd import _lib

    for name in ("mm_contrast_design_stats", "mm_contrast_design_rows"):
        assert name in declared and name in _lib.EXPORTS
    args, res = _lib._SIGS["mm_contrast_design_stats"]
    assert len(args) == 14 and res is ctypes.c_int
    args, res = _lib._SIGS["mm_contrast_design_rows"]
    assert len(args) == 14 and res is ctypes.c_int
