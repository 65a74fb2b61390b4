"""CPU tests of the sequential bootstrap of the gene-pair tests (ht_2d_moments(rng='fast', max_boot=..., min_extreme=...)): the
signature, the argument checks that run before ``adata`` is touched, the C-ABI of the range launch (mm_boot2d_fast_range) and the
engine surface it is reached through.  The records, the schedule, the stopping rule and the p-values are the 1D call's
(tests/test_cpu_sequential.py)."""

import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_parameters_are_keyword_only():
    from scrna_parameter_estimation_amd import memento

    sig = inspect.signature(memento.ht_2d_moments).parameters
    assert sig['max_boot'].default is None and sig['min_extreme'].default == 10
    assert sig['max_boot'].kind is sig['min_extreme'].kind is inspect.Parameter.KEYWORD_ONLY
    names = list(sig)
    assert names.index('max_boot') < names.index('kwargs') and names.index('min_extreme') < names.index('kwargs')
    assert sig['kwargs'].kind is inspect.Parameter.VAR_KEYWORD


@pytest.mark.parametrize("kw", [dict(rng='replay'), dict(approx=True), dict(ci=0.95), dict(resample_rep=True), dict(max_boot=199),
                                dict(max_boot=400.0), dict(max_boot=True), dict(max_boot=2 ** 31), dict(min_extreme=-1),
                                dict(min_extreme=2.5)])
def test_argument_errors_come_before_adata_is_touched(kw):
    """``adata`` is an object without a single attribute, covariate and treatment are None: the ValueError must come first."""
    from scrna_parameter_estimation_amd import memento

    args = dict(num_boot=200, rng='fast', max_boot=3200, resampling='bootstrap')
    args.update(kw)
    with pytest.raises(ValueError):
        memento.ht_2d_moments(object(), covariate=None, treatment=None, **args)


def test_cabi_declares_and_binds_the_range_launch():
    from scrna_parameter_estimation_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "memento_hip.h")).read()
    decl = re.search(r"\bint mm_boot2d_fast_range\s*\(([^;]*)\);", hdr)
    assert decl and "mm_boot2d_fast_range" in _lib.EXPORTS
    params = [a.strip() for a in decl.group(1).split(",")]
    one_shot = [a.strip() for a in re.search(r"\bint mm_boot2d_fast\s*\(([^;]*)\);", hdr).group(1).split(",")]
    assert len(one_shot) == 20 and one_shot[14] == "int32_t num_boot" and len(params) == 21
    assert params == one_shot[:14] + ["int32_t rep_lo", "int32_t rep_n"] + one_shot[15:]      # num_boot -> rep_lo, rep_n
    args, res = _lib._SIGS["mm_boot2d_fast_range"]
    ref = _lib._SIGS["mm_boot2d_fast"][0]
    assert args == ref[:14] + [ctypes.c_int32, ctypes.c_int32] + ref[15:] and res is ctypes.c_int
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mm_boot2d_fast_range")
    src = open(os.path.join(ROOT, "scrna_parameter_estimation_amd", "csrc", "boot.hip")).read()
    assert src.count("void k_boot2d_fast(") == 1 and src.count("hipLaunchKernelGGL(k_boot2d_fast,") == 1     # one kernel, one launch


def test_engine_surface():
    from scrna_parameter_estimation_amd import engine
    from scrna_parameter_estimation_amd.memento import _ht

    assert "launch_range" in vars(engine.Bootstrap2D) and "run_range" not in vars(engine.Bootstrap2D)
    assert inspect.signature(engine.Bootstrap2D.run).parameters["keep_fast"].default is False
    assert list(inspect.signature(engine.Bootstrap2D.launch_range).parameters) == ["self", "rep_lo", "rep_n", "open_q", "plane", "row_of_q",
                                                                                   "dump_weights"]
    assert callable(engine.contract_plane) and callable(_ht.continue_chunk_2d)
    assert inspect.signature(_ht.run_chunk_2d).parameters["keep_fast"].default is False
