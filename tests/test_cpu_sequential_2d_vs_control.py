"""CPU tests of the sequential bootstrap of the 2D screen (ht_2d_vs_control_sequential(rng='fast', max_boot=..., min_extreme=...)): the
signature, the argument checks that run before ``adata`` is touched, the C-ABI of the launch over a list of slots
(mm_boot2d_fast_slots), the engine surface it is reached through, and the two pure table routines of a round
(``_ht.design_round_tables``, ``_ht.design_batches``) against brute-force loops.  The records, the schedule, the stopping rule and
the p-values are the 1D call's (tests/test_cpu_sequential.py)."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_parameters_are_keyword_only():
    """ht_2d_vs_control_sequential is ht_2d_vs_control -- whose parameter list tests/test_cpu_sequential.py and
    tests/test_cpu_vs_control_2d.py pin -- with the same parameters, kinds and defaults, plus the two keyword-only ones."""
    from scrna_parameter_estimation_amd import memento

    plain = inspect.signature(memento.ht_2d_vs_control).parameters
    sig = inspect.signature(memento.ht_2d_vs_control_sequential).parameters
    assert sig['max_boot'].default is None and sig['min_extreme'].default == 10
    assert sig['max_boot'].kind is sig['min_extreme'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig) == list(plain) + ['max_boot', 'min_extreme'] and 'max_boot' not in plain
    for name, p in plain.items():
        assert (sig[name].kind, sig[name].default) == (p.kind, p.default), name
    with pytest.raises(TypeError):
        memento.ht_2d_vs_control_sequential(None, 'ctrl', 200, 1, 0, None, False, 'bootstrap', 'fast', 3200)
    with pytest.raises(TypeError):
        memento.ht_2d_vs_control(None, 'ctrl', num_boot=200, rng='fast', max_boot=3200)


class _Untouchable:
    """An ``adata`` whose ``uns`` raises on access."""

    @property
    def uns(self):
        raise AssertionError("adata.uns was read before the arguments were checked")


@pytest.mark.parametrize("kw", [dict(rng='replay'), dict(approx=True), dict(ci=0.9), dict(max_boot=199), dict(max_boot=400.0),
                                dict(max_boot=True), dict(max_boot=2 ** 31), dict(min_extreme=-1), dict(min_extreme=2.5),
                                dict(min_extreme=None)])
@pytest.mark.parametrize("treatment_col", [None, 'guide'])
def test_argument_errors_come_before_adata_is_touched(kw, treatment_col):
    from scrna_parameter_estimation_amd import memento

    args = dict(num_boot=200, rng='fast', max_boot=3200, treatment_col=treatment_col)
    args.update(kw)
    with pytest.raises(ValueError):
        memento.ht_2d_vs_control_sequential(_Untouchable(), 'ctrl', **args)
    with pytest.raises(AssertionError):                      # (the probe works: a valid call does reach adata.uns)
        memento.ht_2d_vs_control_sequential(_Untouchable(), 'ctrl', num_boot=200, rng='fast', max_boot=3200, treatment_col=treatment_col)


def test_check_sequential_names_the_call():
    from scrna_parameter_estimation_amd.memento import _ht

    assert "ht_2d_vs_control_sequential" in _ht.check_sequential.__doc__


def test_cabi_declares_and_binds_the_listed_launch():
    from scrna_parameter_estimation_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "memento_hip.h")).read()
    decl = re.search(r"\bint mm_boot2d_fast_slots\s*\(([^;]*)\);", hdr)
    assert decl and "mm_boot2d_fast_slots" in _lib.EXPORTS
    params = [a.strip() for a in decl.group(1).split(",")]
    ranged = [a.strip() for a in re.search(r"\bint mm_boot2d_fast_range\s*\(([^;]*)\);", hdr).group(1).split(",")]
    assert ranged[18:20] == ["int32_t *d_w_dump", "int32_t kmax_dump"]
    assert params == ranged[:18] + ["const int64_t *d_slot_list", "int64_t n_list"] + ranged[20:]     # the weight dump -> the list
    args, res = _lib._SIGS["mm_boot2d_fast_slots"]
    ref = _lib._SIGS["mm_boot2d_fast_range"][0]
    assert args == ref[:18] + [ctypes.c_void_p, ctypes.c_int64] + ref[20:] and res is ctypes.c_int
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mm_boot2d_fast_slots")
    comment = hdr[:decl.start()].rsplit("/*", 1)[1]
    assert "listed twice" in comment and "written twice with the same values" in comment and "engine never does" in comment
    src = open(os.path.join(ROOT, "scrna_parameter_estimation_amd", "csrc", "boot.hip")).read()
    # one body, two instantiations, one launch each
    assert src.count("void boot2d_fast_body(") == 1 and src.count("boot2d_fast_body<false>(") == 1 and src.count("boot2d_fast_body<true>(") == 1
    assert src.count("void k_boot2d_fast_slots(") == 1 and src.count("hipLaunchKernelGGL(k_boot2d_fast_slots,") == 1


def test_engine_surface():
    from scrna_parameter_estimation_amd import engine
    from scrna_parameter_estimation_amd.memento import _ht

    ranged = list(inspect.signature(engine.Bootstrap2D.launch_range).parameters)
    assert list(inspect.signature(engine.Bootstrap2D.launch_listed).parameters) == ranged
    for name in ("continue_chunk_2d_designs", "design_round_tables", "design_batches", "_rounds_2d"):
        assert callable(getattr(_ht, name))
    sig = inspect.signature(_ht.continue_chunk_2d_designs).parameters
    assert sig["budget"].default is None and sig["n_chains"].default is None and sig["open_mask"].default is None
    # one round loop: both 2D continuations go through _rounds_2d and hold no loop over the schedule themselves
    for fn in (_ht.continue_chunk_2d, _ht.continue_chunk_2d_designs):
        body = inspect.getsource(fn)
        assert "_rounds_2d(" in body and "merge_records(" not in body.split('"""', 2)[2] and "open_tests(" not in body.split('"""', 2)[2]


# ----------------------------------------------------------------------------------------------
# the table builder
# ----------------------------------------------------------------------------------------------

NG = 12


def _random_tables(rng, n_designs=40):
    """CSR design tables over NG groups: two-entry {+1, -1} designs, 2-6-entry weighted ones and empty ones, in random order."""
    ptr, grp, w = [0], [], []
    for d in range(n_designs):
        kind = rng.integers(0, 4)
        if kind == 0:
            g, ww = [], []
        elif kind == 1:
            g, ww = list(rng.choice(NG, size=2, replace=False)), [1.0, -1.0]
        else:
            n = int(rng.integers(2, 7))
            g, ww = list(rng.choice(NG, size=n, replace=False)), list(rng.normal(size=n))
        grp += g
        w += ww
        ptr.append(len(grp))
    return np.asarray(ptr, dtype=np.int32), np.asarray(grp, dtype=np.int32), np.asarray(w, dtype=np.float64)


def _brute(test_pair, test_design, ptr, grp, w):
    """Per test: its (chain, weight) entries in design order; and the sorted distinct chains."""
    per_test = []
    for p, d in zip(test_pair, test_design):
        per_test.append([(int(p) * NG + int(grp[e]), float(w[e])) for e in range(int(ptr[d]), int(ptr[d + 1]))])
    chains = sorted({q for t in per_test for q, _ in t})
    return per_test, chains


def _check_tables(test_pair, test_design, tables):
    from scrna_parameter_estimation_amd.memento import _ht

    ptr, grp, w = tables
    chains, t_ptr, rows, t_w = _ht.design_round_tables(test_pair, test_design, ptr, grp, w, NG)
    per_test, want_chains = _brute(test_pair, test_design, ptr, grp, w)
    # rows are a bijection onto the chains: row i <-> chain chains[i], ascending, every chain once
    assert list(chains) == want_chains and len(set(chains)) == len(chains)
    assert len(t_ptr) == len(test_pair) + 1 and t_ptr[0] == 0 and t_ptr[-1] == len(rows) == len(t_w)
    if len(rows):
        assert rows.min() >= 0 and rows.max() < len(chains) and set(rows) == set(range(len(chains)))
    for t, want in enumerate(per_test):                    # entry order and weights are the shared design's
        lo, hi = int(t_ptr[t]), int(t_ptr[t + 1])
        assert [(int(chains[r]), float(x)) for r, x in zip(rows[lo:hi], t_w[lo:hi])] == want
    np.testing.assert_array_equal(chains, _ht._design_chains(test_pair, test_design, ptr, grp, NG))
    return chains


@pytest.mark.parametrize("seed", range(6))
def test_round_tables_against_a_brute_force_loop(seed):
    rng = np.random.default_rng(seed)
    tables = _random_tables(rng)
    n_designs = len(tables[0]) - 1
    assert (np.diff(tables[0]) == 0).any() and (np.diff(tables[0]) == 2).any() and (np.diff(tables[0]) > 2).any()
    n = int(rng.integers(1, 200))
    test_pair = np.sort(rng.integers(0, 50, size=n))       # pair-major, several tests per pair
    test_design = rng.integers(0, n_designs, size=n)
    _check_tables(test_pair, test_design, tables)


def test_round_tables_share_a_pairs_control_chains():
    """Four open guides of ONE pair over strata designs {guide stratum rows, control stratum rows}: the three control chains appear
    once, every guide chain once, and the tests of another pair do not share them."""
    ctrl = [0, 1, 2]
    ptr, grp, w = [0], [], []
    for g in range(1, 4):
        grp += [3 * g, 3 * g + 1, 3 * g + 2] + ctrl
        w += [0.3, 0.3, 0.4, -0.3, -0.3, -0.4]
        ptr.append(len(grp))
    tables = (np.asarray(ptr, dtype=np.int32), np.asarray(grp, dtype=np.int32), np.asarray(w))
    chains = _check_tables(np.array([7, 7, 7]), np.array([0, 1, 2]), tables)
    assert list(chains) == [7 * NG + g for g in range(12)]
    chains = _check_tables(np.array([7, 7, 9]), np.array([0, 2, 2]), tables)
    assert list(chains) == [7 * NG + g for g in (0, 1, 2, 3, 4, 5, 9, 10, 11)] + [9 * NG + g for g in (0, 1, 2, 9, 10, 11)]


def test_round_tables_without_an_open_test_and_with_empty_designs_only():
    from scrna_parameter_estimation_amd.memento import _ht

    tables = _random_tables(np.random.default_rng(0))
    chains, t_ptr, rows, t_w = _ht.design_round_tables(np.zeros(0, np.int64), np.zeros(0, np.int64), *tables, NG)
    assert len(chains) == 0 and list(t_ptr) == [0] and len(rows) == 0 and len(t_w) == 0
    assert _ht.design_batches(np.zeros(0, np.int64), np.zeros(0, np.int64), tables[0], tables[1], NG, 5) == []
    empty = int(np.flatnonzero(np.diff(tables[0]) == 0)[0])
    chains = _check_tables(np.array([3, 4]), np.array([empty, empty]), tables)
    assert len(chains) == 0


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("cap", [1, 3, 7, 20, 10 ** 6])
def test_batches_are_contiguous_runs_within_the_budget(seed, cap):
    """Every run is a contiguous range, the runs tile the tests in order, a run reads at most ``cap`` distinct chains unless it is
    a single test, and it is as long as fits: the next test would have taken it over ``cap``."""
    from scrna_parameter_estimation_amd.memento import _ht

    rng = np.random.default_rng(100 + seed)
    ptr, grp, w = _random_tables(rng)
    n = 150
    test_pair = np.sort(rng.integers(0, 30, size=n))
    test_design = rng.integers(0, len(ptr) - 1, size=n)
    runs = _ht.design_batches(test_pair, test_design, ptr, grp, NG, cap)
    assert runs[0][0] == 0 and runs[-1][1] == n and all(a[1] == b[0] for a, b in zip(runs[:-1], runs[1:])) and all(lo < hi for lo, hi in runs)

    def distinct(lo, hi):
        return len(_brute(test_pair[lo:hi], test_design[lo:hi], ptr, grp, w)[1])

    for lo, hi in runs:
        assert distinct(lo, hi) <= cap or hi == lo + 1
        assert hi == n or distinct(lo, hi + 1) > cap
    if cap == 10 ** 6:
        assert runs == [(0, n)]
