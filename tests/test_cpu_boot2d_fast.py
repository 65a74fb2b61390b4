"""CPU tests of rng='fast' on the gene-pair (2D) path: the argument checks of ht_2d_moments / ht_2d_vs_control (they run before
anything touches the device), and the C-ABI entry point mm_boot2d_fast declared, exported and bound with matching arity."""

import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rng_argument_is_validated():
    from scrna_parameter_estimation_amd import memento

    for fn in (memento.ht_2d_moments, memento.ht_2d_vs_control):
        assert inspect.signature(fn).parameters["rng"].default == "replay"
    with pytest.raises(ValueError, match="rng must be 'replay' or 'fast'"):
        memento.ht_2d_moments(None, None, None, rng="bogus", resampling="bootstrap")
    with pytest.raises(ValueError, match="rng must be 'replay' or 'fast'"):
        memento.ht_2d_vs_control(None, 0, rng="bogus")
    with pytest.raises(ValueError, match="strict=True needs rng='replay'"):
        memento.ht_2d_moments(None, None, None, strict=True, rng="fast", resampling="bootstrap")


def test_cabi_declares_and_binds_the_fast_2d_bootstrap():
    from scrna_parameter_estimation_amd import _lib, build
    from scrna_parameter_estimation_amd.engine import Bootstrap2D

    hdr = open(os.path.join(ROOT, "include", "memento_hip.h")).read()
    decl = re.search(r"\bint mm_boot2d_fast\s*\(([^;]*)\);", hdr)
    assert decl and "mm_boot2d_fast" in _lib.EXPORTS
    args, res = _lib._SIGS["mm_boot2d_fast"]
    assert len(args) == len(decl.group(1).split(",")) == 20 and res is ctypes.c_int
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mm_boot2d_fast")
    src = open(os.path.join(ROOT, "scrna_parameter_estimation_amd", "csrc", "boot.hip")).read()
    assert "k_boot2d_fast" in src and src.count("close_replicate_2d(") >= 3       # one definition, called from both 2D kernels
    run = inspect.signature(Bootstrap2D.run).parameters
    assert [run[k].default for k in ("fast", "fast_seed", "pair_key", "dump_weights")] == [False, 0, None, False]
