"""Plain numpy restatement of the streams of rng='fast' (csrc/boot.hip: fast_stream; include/memento_hip.h: mm_boot1d_fast), for
the draw-for-draw tests of the fast kernels.  Nothing here imports the engine.

Replicate r of the chain with key ``key`` owns a plain PCG64 whose four words are

    h = mix64(seed ^ mix64(key * 0x100000001B3 + r))                         (mod 2^64; mix64 = the splitmix64 output function)
    state = (mix64(h), mix64(h + 1))      increment = (mix64(h + 2), mix64(h + 3) | 1)           (high word, low word)

numpy's PCG64 takes any (state, inc) through its ``.state`` setter and then follows the recurrence of csrc/npy_rng.h
(tests/test_cpu_fast_ref.py pins that), so ``Generator(PCG64 set to that state).multinomial(N, mult / N)`` is, draw for draw, what
replicate r of the chain must produce: ``fast_weights``.  ``sweep_mults`` is the (n, p) sweep of tests/test_gpu_sampler_sweep.py and
``sweep_regimes`` counts how numpy drew it."""

from types import SimpleNamespace

import numpy as np

from _replicate_ref import _u64, mix64

U = np.uint64
KEY_MULT = 0x100000001B3
MAX_DISTINCT_KEY = ((1 << 64) - 1) // KEY_MULT          # the largest key below 2^64 / KEY_MULT (include/memento_hip.h: mm_boot1d_fast_range)


def fast_state(seed, key, reps):
    """The four uint64 words (state high, state low, increment high, increment low) of the streams of the global replicates ``reps``
    of the chain(s) with key ``key``: arrays of the broadcast shape of ``key`` and ``reps``.  ``key`` is taken as int64 and read as
    its two's complement; ``seed`` is any integer below 2^64."""
    key = _u64(key) if isinstance(key, int) else np.asarray(key, dtype=np.int64).view(U)
    reps = np.asarray(reps, dtype=np.int64)
    assert (reps >= 0).all() and (reps <= 2 ** 31 - 1).all()
    with np.errstate(over="ignore"):
        h = mix64(_u64(int(seed)) ^ mix64(key * U(KEY_MULT) + reps.view(U)))
        return mix64(h), mix64(h + U(1)), mix64(h + U(2)), mix64(h + U(3)) | U(1)


_BG = np.random.PCG64(0)
_GEN = np.random.Generator(_BG)
_STATE = {"bit_generator": "PCG64", "state": {"state": 0, "inc": 1}, "has_uint32": 0, "uinteger": 0}


def set_stream(hi, lo, ihi, ilo):
    """The module's one reusable generator, set to the stream with these four words."""
    _STATE["state"]["state"] = (int(hi) << 64) | int(lo)
    _STATE["state"]["inc"] = (int(ihi) << 64) | int(ilo)
    _BG.state = _STATE
    return _GEN


def fast_weights(mult, seed, key, reps):
    """[K][len(reps)] weights of the chain with multiplicities ``mult`` (in replay order) and key ``key``: column i is numpy's own
    Generator.multinomial(N, mult / N) on the stream of global replicate reps[i]."""
    mult = np.asarray(mult, dtype=np.int64)
    reps = np.asarray(reps, dtype=np.int64).reshape(-1)
    N = int(mult.sum())
    pv = mult / np.float64(N)
    hi, lo, ihi, ilo = (x.tolist() for x in fast_state(seed, int(key), reps))
    out = np.empty((len(reps), len(mult)), dtype=np.int64)
    for i in range(len(reps)):
        out[i] = set_stream(hi[i], lo[i], ihi[i], ilo[i]).multinomial(N, pv)
    return out.T


def fast_weights_many(mults, seed, keys, reps):
    """fast_weights of S chains of equal length at once: ``mults`` [S][K], ``keys`` [S] -> [S][K][len(reps)]."""
    mults = np.asarray(mults, dtype=np.int64)
    reps = np.asarray(reps, dtype=np.int64).reshape(-1)
    S, K = mults.shape
    st = fast_state(seed, np.asarray(keys, dtype=np.int64)[:, None], reps[None, :])
    hi, lo, ihi, ilo = (x.tolist() for x in st)
    out = np.empty((S, len(reps), K), dtype=np.int64)
    for s in range(S):
        N = int(mults[s].sum())
        pv = mults[s] / np.float64(N)
        h, l, ih, il, o = hi[s], lo[s], ihi[s], ilo[s], out[s]
        for i in range(len(reps)):
            o[i] = set_stream(h[i], l[i], ih[i], il[i]).multinomial(N, pv)
    return out.transpose(0, 2, 1)


# ------------------------------------------------------------------------------------------------------------------------
# the (n, p) sweep
# ------------------------------------------------------------------------------------------------------------------------

SWEEP_FIXED_N = (2 ** 31 - 1, 2 ** 31 - 2, 2 ** 24 + 1, 2 ** 24, 2 ** 24 - 1, 61, 60, 3)


def sweep_mults(S, seed=4242):
    """[S][3] integer multiplicities [m0, m1, N - m0 - m1], every entry >= 1: N log-uniform in [3, 2^31 - 1] behind the fixed first
    entries SWEEP_FIXED_N; m0 such that N p0 is log-uniform in [0.05, N / 2] (at least one cell); m1 such that the conditional
    probability m1 / (N - m0) of the second draw is uniform in [0.5, 0.9999] for the even chains (the pk > 0.5 flip) and
    log-uniform in [1e-7, 0.5] for the odd ones.  Chain s of a shorter sweep is chain s of a longer one."""
    rng = np.random.default_rng(seed)
    u = rng.random((S, 3))
    N = np.floor(np.exp(np.log(3.0) + u[:, 0] * (np.log(2.0 ** 31 - 1) - np.log(3.0)))).astype(np.int64)
    N = np.clip(N, 3, 2 ** 31 - 1)
    N[:min(S, len(SWEEP_FIXED_N))] = SWEEP_FIXED_N[:S]
    np0 = np.exp(np.log(0.05) + u[:, 1] * (np.log(N / 2.0) - np.log(0.05)))
    m0 = np.clip(np.rint(np0).astype(np.int64), 1, N - 2)
    rest = N - m0
    even = np.arange(S) % 2 == 0
    pc = np.where(even, 0.5 + u[:, 2] * 0.4999, np.exp(np.log(1e-7) + u[:, 2] * (np.log(0.5) - np.log(1e-7))))
    m1 = np.clip(np.rint(pc * rest).astype(np.int64), 1, rest - 1)
    out = np.stack([m0, m1, N - m0 - m1], axis=1)
    assert (out >= 1).all() and (out.sum(axis=1) == N).all()
    return out


def sweep_pk(mults):
    """[S][K] chain probabilities of the draws (tests/_replay_ref.py: chain_operands, vectorised over chains)."""
    mults = np.asarray(mults, dtype=np.int64)
    pix = mults.astype(np.float64) / mults.sum(axis=1).astype(np.float64)[:, None]
    pk = np.empty_like(pix)
    left = np.ones(len(pix))
    for k in range(pix.shape[1]):
        pk[:, k] = pix[:, k] / left
        left = left - pix[:, k]
    return pk


def sweep_regimes(mults, w):
    """How numpy drew the weights ``w`` [S][K][B] of the chains ``mults`` [S][K]: counts of the binomial draws it actually made
    (bins k < K - 1 with cells left and pk > 0), by sampler (inversion up to n min(p, 1 - p) = 30, BTPE above), by the pk > 0.5
    flip, by size (n >= 2^24: beyond fp32's integers; n < 200) and on either side of the sampler switch
    (25 < n min(p, 1 - p) <= 35), n being the cells left when the draw was made."""
    mults, w = np.asarray(mults, dtype=np.int64), np.asarray(w, dtype=np.int64)
    K = mults.shape[1]
    pk = sweep_pk(mults)[:, :K - 1, None]
    left = mults.sum(axis=1)[:, None, None] - (np.cumsum(w, axis=1) - w)[:, :K - 1]              # cells left BEFORE bin k
    drawn = (left > 0) & (pk > 0)
    npq = left * np.minimum(pk, 1.0 - pk)
    inv, bt = drawn & (npq <= 30.0), drawn & (npq > 30.0)
    c = lambda x: int(x.sum())
    return SimpleNamespace(inversion=c(inv), btpe=c(bt), flipped=c(drawn & (pk > 0.5)), btpe_n_ge_2p24=c(bt & (left >= 2 ** 24)),
                           inversion_n_ge_2p24=c(inv & (left >= 2 ** 24)), btpe_n_lt_200=c(bt & (left < 200)),
                           near_switch=c(drawn & (npq > 25.0) & (npq <= 35.0)))


# floors of the regime counts per 2,048 sweep chains at B = 64: about 80 % of what the sweep gives per 2,048 chains with seed 17
# and keys 1000 + chain index -- the lower of the first 2,048 chains' count (inversion 118,058, BTPE 143,990, flipped 64,188,
# BTPE n >= 2^24 51,539, inversion n >= 2^24 9,828, BTPE n < 200 2,811, near the switch 5,842) and a quarter of the 8,192 chains'
# (121,637 / 140,420 / 64,173 / 50,181 / 9,625 / 2,557 / 4,722).  tests/test_cpu_fast_ref.py asserts them on the host,
# tests/test_gpu_sampler_sweep.py before it launches.
SWEEP_FLOORS = dict(inversion=94_000, btpe=112_000, flipped=51_000, btpe_n_ge_2p24=40_000, inversion_n_ge_2p24=7_700, btpe_n_lt_200=2_000,
                    near_switch=3_700)
SWEEP_SEED, SWEEP_KEY0, SWEEP_B = 17, 1000, 64
