"""CPU tests of the joint coexpression test (``ht_2d_joint``, ``Bootstrap2D.joint``, mm_joint1_stats): the entry point is
declared, bound, exported by the built library and documented, and the public call checks its arguments before it touches the
device.  No device."""

import os
from types import SimpleNamespace

import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_entry_point():
    from scrna_parameter_estimation_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "memento_hip.h")).read()
    assert "int mm_joint1_stats(" in hdr
    assert "mm_joint1_stats" in _lib.EXPORTS
    assert hasattr(_lib.load(require_gpu=False), "mm_joint1_stats")
    assert "`mm_joint1_stats`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_binding_matches_the_declaration():
    """14 arguments: the plane, ld, num_boot, n_groups, the seven tables, n_tests, the record and the stream."""
    import ctypes

    from scrna_parameter_estimation_amd import _lib

    args, res = _lib._SIGS["mm_joint1_stats"]
    assert len(args) == 14 and res is ctypes.c_int
    assert args[1] is ctypes.c_int64 and args[2] is args[3] is ctypes.c_int32 and args[11] is ctypes.c_int64
    two = _lib._SIGS["mm_joint_stats"][0]
    assert len(two) == 16 and args == two[1:14] + two[15:]          # mm_joint_stats less one plane and one record


def test_the_public_call_is_exported():
    import scrna_parameter_estimation_amd.memento as memento
    from scrna_parameter_estimation_amd import engine
    from scrna_parameter_estimation_amd.memento import main

    assert callable(memento.ht_2d_joint) and memento.ht_2d_joint is main.ht_2d_joint
    assert callable(engine.Bootstrap2D.joint)


def test_ht_2d_joint_checks_its_arguments_first():
    from scrna_parameter_estimation_amd import memento

    with pytest.raises(ValueError, match="rng must be"):
        memento.ht_2d_joint(object(), "cond", rng="other")
    m = {"_hip": SimpleNamespace(), "groups": ["sg^a^0", "sg^b^0", "sg^c^1"], "label_columns": ["ct", "rep"], "label_delimiter": "^"}
    with pytest.raises(ValueError, match="label columns"):
        memento.ht_2d_joint(SimpleNamespace(uns={"memento": m}), "dose")
    with pytest.raises(ValueError, match="3 groups"):
        memento.ht_2d_joint(SimpleNamespace(uns={"memento": m}), pd.DataFrame({"x": [0.0, 1.0]}))
    with pytest.raises(TypeError):
        memento.ht_2d_joint(SimpleNamespace(uns={"memento": m}), "ct", ci=0.9)         # no ci, no strict, no resample_rep
