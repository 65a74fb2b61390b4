"""CPU tests of rng='fast' on the 1D path: the C-ABI entry point mm_boot1d_fast declared, exported and bound with matching arity
(keys and the weight dump included), Bootstrap1D.run's chain_keys, and both API calls handing keys to it."""

import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cabi_declares_and_binds_the_keyed_fast_1d_bootstrap():
    from scrna_parameter_estimation_amd import _lib, build
    from scrna_parameter_estimation_amd.engine import Bootstrap1D

    hdr = open(os.path.join(ROOT, "include", "memento_hip.h")).read()
    decl = re.search(r"\bint mm_boot1d_fast\s*\(([^;]*)\);", hdr)
    assert decl and "mm_boot1d_fast" in _lib.EXPORTS
    params = [a.strip() for a in decl.group(1).split(",")]
    args, res = _lib._SIGS["mm_boot1d_fast"]
    assert len(args) == len(params) == 21 and res is ctypes.c_int
    assert params[10:13] == ["const int64_t *d_slot_row", "const int64_t *d_slot_key", "uint64_t seed"]
    assert params[18:] == ["int32_t *d_w_dump", "int32_t kmax_dump", "void *stream"]
    assert args[11] is ctypes.c_void_p and args[12] is ctypes.c_uint64 and args[18:] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mm_boot1d_fast")
    src = open(os.path.join(ROOT, "scrna_parameter_estimation_amd", "csrc", "boot.hip")).read()
    kern = src[src.index("void k_boot1d_fast("):src.index("// FREE-RUNNING tile kernel")]
    assert "slot_key[slot]" in kern and "row * 0x100000001B3ull" not in kern          # the streams are keyed, not row-numbered
    assert "MM_ARG(!d_w_dump || kmax_dump > 0);" in src[src.index("int mm_boot1d_fast("):]
    run = inspect.signature(Bootstrap1D.run).parameters
    assert [run[k].default for k in ("fast", "fill_keys", "chain_keys", "dump_weights")] == [False, None, None, False]


def test_both_api_calls_pass_chain_keys():
    """Neither call reaches Bootstrap1D.run without a device, so this reads the calls: each hands its ``fill_keys`` and ``chain_keys``
    to its one ``_ht.run_chunk_1d``, whose one ``bs.run`` (the non-strict one, ``fill_mode=0``) passes them on."""
    from scrna_parameter_estimation_amd.memento import _ht, main

    src = inspect.getsource(_ht.run_chunk_1d)
    assert src.startswith("def run_chunk_1d(c, mv, rng, fill_seed, fill_keys, chain_keys, uniforms=None):")
    calls = [c for c in re.findall(r"bs\.run\(([^#]*?)\)\s", src, flags=re.S) if "fill_mode=0" in c]
    assert len(calls) == 1
    assert "fill_keys=fill_keys" in calls[0] and "chain_keys=chain_keys" in calls[0] and "fast=(rng == 'fast')" in calls[0]
    for fn in (main.ht_1d_moments, main.ht_1d_vs_control):
        src = inspect.getsource(fn)
        assert not [c for c in re.findall(r"bs\.run\(([^#]*?)\)\s", src, flags=re.S) if "fill_mode=0" in c], fn.__name__
        calls = re.findall(r"_ht\.run_chunk_1d\(([^#]*?)\)\s", src, flags=re.S)
        assert len(calls) == 1, fn.__name__
        assert re.fullmatch(r"c, mv, rng, fill_seed, \w+, \w+(, uniforms)?", calls[0]), fn.__name__
    src = inspect.getsource(main.ht_1d_vs_control)
    assert "keys = np.arange(c.g0 * ng, c.g1 * ng, dtype=np.int64)" in src and "run_chunk_1d(c, mv, rng, fill_seed, keys, keys)" in src
    assert "run_chunk_1d(c, mv, rng, fill_seed, keys, chain_keys, uniforms)" in inspect.getsource(main.ht_1d_moments)
