"""Host side of ``ht_2d_posthoc`` (no GPU): the one-plane entry point's declaration, binding and signature, the driver's signature,
the argument checks that run before any device work, ``family_scale`` on one record array and the scale check per plane count."""

import inspect
import os
from types import SimpleNamespace

import numpy as np
import pytest

from test_cpu_posthoc import _fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_entry_point():
    from ctypes import c_int32, c_int64, c_void_p

    from scrna_parameter_estimation_amd import _lib, memento

    hdr = open(os.path.join(ROOT, "include", "memento_hip.h")).read()
    assert "int mm_family_maxt1(" in hdr and "mm_family_maxt1" in _lib.EXPORTS
    assert hasattr(_lib.load(require_gpu=False), "mm_family_maxt1")
    assert "`mm_family_maxt1`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    args, res = _lib._SIGS["mm_family_maxt1"]
    design_stats = _lib._SIGS["mm_contrast_design1_stats"][0]
    # the plane and the design tables of mm_contrast_design1_stats, with family_ptr in front of the tables, then scale, stage_cap,
    # n_fam, the three outputs and the stream
    assert args[:4] == design_stats[:4] == [c_void_p, c_int64, c_int32, c_int32]
    assert args[4] is c_void_p and args[5:10] == design_stats[4:9] == [c_void_p] * 5
    assert args[10:] == [c_void_p, c_int32, c_int64] + [c_void_p] * 4 and res is _lib._SIGS["mm_family_maxt"][1]
    # the two-plane entry with one plane less
    assert args == _lib._SIGS["mm_family_maxt"][0][1:]
    assert callable(memento.ht_2d_posthoc)


def test_signature():
    from scrna_parameter_estimation_amd import memento

    sig = inspect.signature(memento.ht_2d_posthoc)
    assert sig == inspect.signature(memento.ht_1d_posthoc)
    assert list(sig.parameters) == ["adata", "treatment_col", "control", "num_boot", "num_cpus", "rng", "fill_seed", "max_rows", "approx", "ci"]
    assert sig.parameters["ci"].kind is inspect.Parameter.KEYWORD_ONLY
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [None, None, 10000, 1, "replay", 0, None, False, None]
    for word in ("resample_rep", "strict", "treatment_for_gene", "resampling", "several ranks"):
        assert word in memento.ht_2d_posthoc.__doc__                   # what is not offered is said


def test_argument_checks_come_first():
    """None of these reaches the pair plan: the fake ``adata`` has no 2D moments and nothing here needs a device."""
    from scrna_parameter_estimation_amd import memento

    with pytest.raises(ValueError, match="rng must be"):
        memento.ht_2d_posthoc(object(), "cond", rng="numpy")
    for bad in (1.5, 0, True, "0.9"):
        with pytest.raises(ValueError, match="ci must be"):
            memento.ht_2d_posthoc(object(), "cond", ci=bad)
    groups = ["sg^a^0", "sg^b^0", "sg^c^1", "sg^a^1"]
    with pytest.raises(NotImplementedError, match="several ranks"):
        memento.ht_2d_posthoc(_fake(groups, ["ct", "rep"], comm=SimpleNamespace(world=2, rank=0)), "ct")
    with pytest.raises(ValueError, match="label columns"):
        memento.ht_2d_posthoc(_fake(groups, ["ct", "rep"]), "dose")
    with pytest.raises(ValueError, match="does not occur"):
        memento.ht_2d_posthoc(_fake(groups, ["ct", "rep"]), "ct", control="z")
    with pytest.raises(ValueError, match="not one of the groups"):
        memento.ht_2d_posthoc(_fake(groups, ["ct", "rep"]), control="sg^z^0")
    with pytest.raises(ValueError, match="control index"):
        memento.ht_2d_posthoc(_fake(groups, ["ct", "rep"]), control=4)
    with pytest.raises(ValueError, match="two levels"):
        memento.ht_2d_posthoc(_fake(["sg^a^0", "sg^a^1"], ["ct", "rep"]), "ct")
    with pytest.raises(ValueError, match="two levels"):
        memento.ht_2d_posthoc(_fake(["sg^a^0"], ["ct", "rep"]))


def test_family_scale_on_one_plane():
    from scrna_parameter_estimation_amd import engine

    rec = np.array([[1.0, 0.5, 300, 7, 0.0, 0, 7, 2.0],           # a test
                    [np.nan, np.nan, 0, 0, np.nan, 0, np.nan, np.nan],          # the NaN record
                    [1.0, 0.0, 300, 0, 0.0, 1, 0, 0.0],           # se 0, all equal
                    [1.0, np.nan, 0, 0, np.nan, 0, 0, 0.0],       # no valid replicate
                    [np.nan, 0.5, 300, 0, 0.0, 0, 0, 1.0],        # column 0 dropped
                    [1.0, 0.0, 300, 0, 0.0, 0, 0, 0.0],           # se 0 alone
                    [1.0, 0.5, 0, 0, 0.0, 0, 0, 0.0],             # n_valid 0 alone
                    [1.0, 0.5, 300, 0, 0.0, 1, 0, 0.0],           # all_equal alone
                    [-2.0, 0.25, 17, 0, 0.0, 0, 0, 1.0]])         # a test
    one = engine.family_scale(rec)
    assert one.shape == (len(rec), 1) and one[:, 0].tolist() == [2.0, 0, 0, 0, 0, 0, 0, 0, 4.0]
    two = engine.family_scale(rec, rec)
    assert two.shape == (len(rec), 2)
    np.testing.assert_array_equal(one[:, 0], two[:, 0])
    np.testing.assert_array_equal(two[:, 0], two[:, 1])
    three = engine.family_scale(rec, rec[::-1], rec)
    assert three.shape == (len(rec), 3) and three[:, 1].tolist() == one[::-1, 0].tolist()
    assert engine.family_scale(np.zeros((0, 8))).shape == (0, 1)


def test_the_scale_is_checked_against_the_number_of_planes():
    from scrna_parameter_estimation_amd import engine

    ok = ([0, 2, 3], [0, 0, 1], [0, 1, 0], [0, 2, 4], [0, 1, 2, 1], [1.0, -1.0, 1.0, -1.0])
    for n_planes, bad in ((1, np.ones((3, 2))), (1, np.ones(3)), (1, np.ones((2, 1))), (2, np.ones((3, 1)))):
        with pytest.raises(ValueError, match=rf"family_maxt: scale must be \[n_tests\]\[{n_planes}\]"):
            engine._family_tables(*ok, bad, 2, 3, n_planes)
    with pytest.raises(ValueError, match="family_maxt: family_ptr"):
        engine._family_tables([0, 2], *ok[1:], np.ones((3, 1)), 2, 3, 1)
    with pytest.raises(ValueError, match="family_maxt: the tests of a family"):
        engine._family_tables([0, 1, 3], *ok[1:], np.ones((3, 1)), 2, 3, 1)


def test_adjusted_columns():
    """The helper both drivers assemble their adjusted columns with, on two families of three members."""
    from scrna_parameter_estimation_amd.memento import _ht

    adj = np.array([[2.0, 5], [np.nan, 0], [0.5, 99], [1.0, 0], [1.0, 0], [np.nan, 0]])
    fam = np.array([[99.0, 2], [199.0, 2]])
    p = np.array([0.01, 0.3, 0.5, 0.2, 0.001, np.nan])
    se = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    p_adj, n_family, half = _ht.adjusted_columns(p, adj, fam, 3, se, np.array([2.0, 3.0]))
    np.testing.assert_array_equal(p_adj, [0.06, np.nan, 1.0, 0.2, 1 / 200, np.nan])
    assert n_family.dtype == np.int64 and n_family.tolist() == [2, 2, 2, 2, 2, 2]
    np.testing.assert_array_equal(half, [2.0, np.nan, 6.0, 12.0, 15.0, np.nan])
    assert _ht.adjusted_columns(p, adj, fam, 3)[2] is None
