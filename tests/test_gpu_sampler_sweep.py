"""An (n, p) sweep of the binomial samplers on the hardware, draw for draw against numpy.

The guarded fp32 fast paths of csrc/npy_rng.h run on the device through the hardware's reciprocal, logarithm, exponential and
square-root instructions; their guards are proven on the host only (tests/host_shim/btpe_stress.cpp), and the kernel tests reach the
samplers only at the multiplicities of tests/_replay_ref.py: menu (n <= 24,000 but for one chain).  Here tests/_fast_ref.py:
sweep_mults gives chains of three bins whose two binomial draws cover n from 3 to 2^31 - 1 (the neighbours of 2^24, 60 and 61
and both ends included), n p from 0.05 to n / 2 and conditional probabilities on both sides of the p > 0.5 flip:

  * 8,192 chains x 64 replicates through mm_boot1d_fast (binomial_pre<int32_t, true> per lane; every (chain, replicate) is a
    stream of its own: about a million independent (n, p, U) cases), every dumped weight equal to fast_weights;
  * the first 2,048 chains x 64 replicates through mm_boot1d_replay (binomial_pre_capped), mm_boot1d_free, mm_boot1d_chain (the
    wave-uniform form with the cooperative generator) and mm_boot1d_async (the lane_* state machine) under PCG64(5) and
    PCG64(12345), and mm_boot1d_replay once more in exact arithmetic (mm_debug_replay_arith(1): the plain samplers), every weight
    equal to ref_weights.

Before anything is launched the reference draws are counted by sampler and size (sweep_regimes) and held to the floors of
tests/_fast_ref.py: SWEEP_FLOORS per 2,048 chains, so the sweep cannot become vacuous.  No case is left out of a comparison."""

import ctypes

import numpy as np
import pytest

from _fast_ref import SWEEP_B, SWEEP_FLOORS, SWEEP_KEY0, SWEEP_SEED, fast_weights_many, sweep_mults, sweep_regimes
from _replay_ref import PAD, SENTINEL, adhoc_chain, layout, ref_weights

pytestmark = pytest.mark.gpu

S_FAST, S_REPLAY, B = 8192, 2048, SWEEP_B
GUARD = 4096


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


def _sweep_layout(S):
    """The first S sweep chains, 64 to a tile, chain s in slot s."""
    mults = sweep_mults(S)
    chains = [adhoc_chain(f"sweep{s}", mults[s]) for s in range(S)]
    L = layout([{lane: ("run", chains[t * 64 + lane]) for lane in range(64)} for t in range(S // 64)])
    assert L.n_slots == S and [e.slot for e in L.ents] == list(range(S)) and (L.slot_K == 3).all()
    np.testing.assert_array_equal(L.slot_nobs, mults.sum(axis=1).astype(np.float64))
    return mults, L


def _floors(mults, w, what):
    got = vars(sweep_regimes(mults, w))
    scale = len(mults) // 2048
    print(f"\n{what}: {len(mults)} chains x {w.shape[2]} replicates, draws numpy made: " + ", ".join(f"{k} {v}" for k, v in got.items()))
    for k, floor in SWEEP_FLOORS.items():
        assert got[k] >= scale * floor, (what, k, got[k], scale * floor)


def _mismatch(got, want, mults, what):
    bad = np.argwhere(got != want)
    if len(bad):
        s, k, r = bad[0].tolist()
        raise AssertionError(f"{what}: {len(bad)} of {want.size} weights differ from numpy's, the first at chain {s} (multiplicities "
                             f"{mults[s].tolist()}), bin {k}, replicate {r}: {got[s, k, r]} instead of {want[s, k, r]}; chains affected: "
                             f"{np.unique(bad[:, 0])[:20].tolist()}")


def test_fast_kernel_sweep(eng):
    """mm_boot1d_fast on 8,192 sweep chains, B = 64, seed SWEEP_SEED, key = SWEEP_KEY0 + chain index: all 8,192 x 3 x 64 dumped
    weights equal numpy's on the per-replicate streams, the cells beyond K and the guard bands keep the pad pattern."""
    mults, L = _sweep_layout(S_FAST)
    want = fast_weights_many(mults, SWEEP_SEED, SWEEP_KEY0 + np.arange(S_FAST), np.arange(B))
    assert want.shape == (S_FAST, 3, B) and (want.sum(axis=1) == mults.sum(axis=1)[:, None]).all()
    _floors(mults, want, "mm_boot1d_fast")
    P, d = eng.P, eng.dev
    ld = B + 4
    init = np.full((L.n_rows, ld), SENTINEL)
    d_m, d_v = d(init), d(init)
    n_w = L.n_slots * L.kmax * B
    assert L.kmax >= 3 and L.slot_row.min() >= 0 and L.slot_row.max() < L.n_rows and L.planes.shape == (5, int(L.tile_ptr[-1]) * 64)
    d_w = d(np.full(n_w + 2 * GUARD, PAD, dtype=np.uint32))
    planes = [d(L.planes[i]) for i in range(5)]
    tabs = [d(x) for x in (L.tile_ptr, L.slot_K, L.slot_nobs, L.slot_omq, L.slot_row, SWEEP_KEY0 + np.arange(S_FAST, dtype=np.int64))]
    eng._lib.call("mm_boot1d_fast", *map(P, planes), P(tabs[0]), L.n_slots, *map(P, tabs[1:]), SWEEP_SEED, B, 0, ld, P(d_m), P(d_v),
                  ctypes.c_void_p(d_w.data_ptr() + 4 * GUARD), L.kmax, eng._stream())
    w = eng.host(d_w, np.uint32)
    body = w[GUARD:GUARD + n_w].reshape(L.n_slots, L.kmax, B)
    _mismatch(body[:, :3].astype(np.int32).astype(np.int64), want, mults, "mm_boot1d_fast")
    assert (body[:, 3:] == PAD).all() and (w[:GUARD] == PAD).all() and (w[GUARD + n_w:] == PAD).all()
    m = eng.host(d_m)
    rows = L.slot_row
    assert np.isfinite(m[rows, 1:1 + B]).all() and np.isnan(m[rows, 1 + B:]).all()


@pytest.fixture(scope="module")
def replay_world(eng):
    import torch

    from test_gpu_replay_kernels import Dev

    mults, L = _sweep_layout(S_REPLAY)
    want = {}
    for seed in (5, 12345):
        want[seed] = np.stack([ref_weights(mults[s], B, seed) for s in range(S_REPLAY)])
        want[seed].setflags(write=False)
    yield mults, Dev(eng, L), want
    torch.cuda.empty_cache()


def test_replay_sweep_is_not_vacuous(replay_world):
    mults, D, want = replay_world
    for seed, w in want.items():
        _floors(mults, w, f"replay forms, PCG64({seed})")


def _replay_weights(eng, D, kernel, seed):
    from test_gpu_replay_kernels import _launch

    L = D.L
    res = _launch(eng, D, kernel, B, seed=seed)
    n = L.n_chains if kernel == "chain" else L.n_slots
    assert n == S_REPLAY and [e.ci for e in L.ents] == list(range(S_REPLAY))
    got = res.w[GUARD:GUARD + n * L.kmax * B].reshape(n, L.kmax, B)
    assert (got[:, 3:] == PAD).all() and (res.w[:GUARD] == PAD).all() and (res.w[GUARD + n * L.kmax * B:] == PAD).all()
    return got[:, :3].astype(np.int32).astype(np.int64)


@pytest.mark.parametrize("seed", [5, 12345])
@pytest.mark.parametrize("kernel", ["replay", "free", "chain", "async"])
def test_replay_forms_sweep(eng, replay_world, kernel, seed):
    """The first 2,048 sweep chains through the four strict kernels, B = 64: every weight is numpy's Generator(PCG64(seed)).multinomial's."""
    mults, D, want = replay_world
    _mismatch(_replay_weights(eng, D, kernel, seed), want[seed], mults, f"mm_boot1d_{kernel}, PCG64({seed})")


def test_replay_exact_arithmetic_sweep(eng, replay_world):
    """mm_boot1d_replay under mm_debug_replay_arith(1) -- the plain samplers without the fp32 fast paths -- on the same chains."""
    mults, D, want = replay_world
    eng._lib.call("mm_debug_replay_arith", 1)
    try:
        got = _replay_weights(eng, D, "replay", 5)
    finally:
        eng._lib.call("mm_debug_replay_arith", 0)
    _mismatch(got, want[5], mults, "mm_boot1d_replay in exact arithmetic, PCG64(5)")
