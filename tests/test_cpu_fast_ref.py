"""tests/_fast_ref.py (the numpy restatement of the rng='fast' streams) pinned on the host: the generator numpy runs from a stream's
four words is the PCG64 of csrc/npy_rng.h, the stream rule is the one csrc/boot.hip states, and the product's guarded sampler code
(binomial_pre<int32_t, true>, what k_boot1d_fast / k_boot2d_fast run per lane), compiled for the host, draws numpy's weights on
such streams.  CPU only."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _fast_ref import (KEY_MULT, MAX_DISTINCT_KEY, SWEEP_B, SWEEP_FLOORS, SWEEP_KEY0, SWEEP_SEED, fast_state, fast_weights, fast_weights_many,
                       set_stream, sweep_mults, sweep_pk, sweep_regimes)
from _replay_ref import chain_operands, menu
from _replicate_ref import mix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 0xDEADBEEF12345678)
KEYS = (0, 1, 2 ** 40, MAX_DISTINCT_KEY, -5)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim_fast") / "libnpyrng_host.so"
    src = os.path.join(ROOT, "tests", "host_shim", "npy_rng_host.cpp")
    inc = os.path.join(ROOT, "scrna_parameter_estimation_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", inc, src, "-o", str(out)])
    return ctypes.CDLL(str(out))


def _words(st, i):
    return (ctypes.c_uint64 * 4)(*[int(x[i]) for x in st])


def test_set_generator_is_the_products_pcg64(shim):
    """(a) 16 raw outputs of numpy's generator set to a stream's (state, inc) equal host_pcg64_raw -- pcg64_next64 of the product's
    header -- on the same four words, for every seed, key and a few replicates (the last one the kernel can store included)."""
    reps = np.array([0, 1, 63, 64, 2 ** 31 - 2])
    out = (ctypes.c_uint64 * 16)()
    for seed in SEEDS:
        for key in KEYS:
            st = fast_state(seed, key, reps)
            for i in range(len(reps)):
                shim.host_pcg64_raw(_words(st, i), 16, out)
                gen = set_stream(*[x[i] for x in st])
                assert list(out) == gen.bit_generator.random_raw(16).tolist(), (seed, key, int(reps[i]))


def test_increment_is_odd_and_words_follow_the_rule():
    """(b) the increment's low word is odd (a PCG64 stream needs that), and the four words are the stated function of h, written
    out here once more in Python integers."""
    M = (1 << 64) - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    assert mix(0) == 0xE220A8397B1DCDAF == int(mix64(0)[0])
    reps = np.array([0, 5, 64, 2 ** 31 - 2])
    for seed in SEEDS:
        for key in KEYS:
            st = fast_state(seed, key, reps)
            assert (st[3] & np.uint64(1) == 1).all()
            for i, r in enumerate(reps.tolist()):
                h = mix(seed ^ mix(((key & M) * KEY_MULT + r) & M))
                assert [int(x[i]) for x in st] == [mix(h), mix((h + 1) & M), mix((h + 2) & M), mix((h + 3) & M) | 1]


def test_promised_pairs_give_distinct_states():
    """(c) include/memento_hip.h: distinct (key, r) with 0 <= key <= MAX_DISTINCT_KEY and 0 <= r < 2^31 give distinct streams.
    key * KEY_MULT + r does not wrap there (2^64 - MAX_DISTINCT_KEY * KEY_MULT = KEY_MULT - 435 * 2^24 > 2^31) and is injective
    (r < KEY_MULT), mix64 is a bijection of 2^64, so h and the state's high word are distinct: checked on the corners of the key
    range, neighbouring keys with the extreme replicates (where an off-by-one in the multiplier would collide) and 200,000 random
    pairs."""
    assert MAX_DISTINCT_KEY * KEY_MULT + 2 ** 31 - 1 < 2 ** 64 <= (MAX_DISTINCT_KEY + 1) * KEY_MULT and 2 ** 31 - 1 < KEY_MULT
    assert 2 ** 64 - MAX_DISTINCT_KEY * KEY_MULT == KEY_MULT - 435 * 2 ** 24
    rng = np.random.default_rng(9)
    keys = np.concatenate([[0, 0, 1, 1, 2, MAX_DISTINCT_KEY - 1, MAX_DISTINCT_KEY - 1, MAX_DISTINCT_KEY, MAX_DISTINCT_KEY],
                           rng.integers(0, MAX_DISTINCT_KEY + 1, size=200_000)]).astype(np.int64)
    reps = np.concatenate([[0, 2 ** 31 - 2, 0, 2 ** 31 - 2, 0, 0, 2 ** 31 - 2, 0, 2 ** 31 - 2], rng.integers(0, 2 ** 31 - 1, size=200_000)])
    pairs = np.unique(np.stack([keys, reps], axis=1), axis=0)
    assert len(pairs) > 200_000
    for seed in SEEDS:
        hi, lo, ihi, ilo = fast_state(seed, pairs[:, 0], pairs[:, 1])
        assert len(np.unique(hi)) == len(pairs) and len(np.unique(lo)) == len(pairs)
    # a key beyond the rule and a negative one still have streams of their own against small keys
    hi = np.concatenate([fast_state(3, k, np.arange(130))[0] for k in (0, 1, 2 ** 40, -5, MAX_DISTINCT_KEY)])
    assert len(np.unique(hi)) == len(hi)


def _shim_multinomial(shim, words, mult):
    mult = np.asarray(mult, dtype=np.int64)
    pv = np.ascontiguousarray(mult / np.float64(int(mult.sum())))
    out = np.zeros((1, len(mult)), dtype=np.int64)
    shim.host_multinomial_fast(words, ctypes.c_int64(int(mult.sum())), pv.ctypes.data_as(ctypes.c_void_p), len(mult), 1,
                               out.ctypes.data_as(ctypes.c_void_p))
    return out[0]


def test_products_sampler_on_fast_streams_is_fast_weights(shim):
    """(d) host_multinomial_fast -- binomial_pre<int32_t, true>, the call of k_boot1d_fast -- on the four words of a stream equals
    fast_weights: 9 menu chains x 2 seeds x 5 keys x 5 replicates and the first 64 sweep chains x 4 replicates (706 streams)."""
    m = menu()
    reps = np.array([0, 1, 64, 129, 2 ** 31 - 2])
    n = 0
    for name in ("k2", "k3_flip", "six_ones", "k64", "k65", "btpe12", "huge", "tail_tiny", "f07"):
        for seed in SEEDS:
            for key in KEYS:
                want = fast_weights(m[name].mult, seed, key, reps)
                st = fast_state(seed, key, reps)
                for i in range(len(reps)):
                    np.testing.assert_array_equal(_shim_multinomial(shim, _words(st, i), m[name].mult), want[:, i], err_msg=f"{name} {seed} {key} {reps[i]}")
                    n += 1
    mults = sweep_mults(64)
    reps = np.array([0, 7, 63, 64])
    want = fast_weights_many(mults, SWEEP_SEED, SWEEP_KEY0 + np.arange(64), reps)
    for s in range(64):
        st = fast_state(SWEEP_SEED, SWEEP_KEY0 + s, reps)
        for i in range(len(reps)):
            np.testing.assert_array_equal(_shim_multinomial(shim, _words(st, i), mults[s]), want[s, :, i], err_msg=f"sweep chain {s} rep {reps[i]}")
            n += 1
    assert n == 706


def test_pinned_known_answer():
    """(e) one (seed, key, r) written out: the stream's words, its first raw outputs and the weights of k3_flip = [950, 30, 20]."""
    st = fast_state(0xDEADBEEF12345678, -5, np.array([0, 1, 2 ** 31 - 2]))
    assert [x.tolist() for x in st] == [[2910230857400106152, 14931355683338517255, 10413394343210768207],
                                        [1982312432053130949, 18375269112370004343, 8205060107889454171],
                                        [7338966139424667557, 3625786617348641749, 11553471054541179422],
                                        [12450361595104849699, 8239906230258683551, 16162168599429396435]]
    np.testing.assert_array_equal(fast_weights([950, 30, 20], 3, 7, np.arange(3)), [[947, 939, 945], [32, 42, 30], [21, 19, 25]])
    np.testing.assert_array_equal(fast_weights_many([[950, 30, 20]] * 2, 3, [7, 8], np.arange(3))[0], [[947, 939, 945], [32, 42, 30], [21, 19, 25]])


def test_stream_rule_is_the_one_the_source_and_the_header_state():
    src = open(os.path.join(ROOT, "scrna_parameter_estimation_amd", "csrc", "boot.hip")).read()
    body = src[src.index("fast_stream(uint64_t seed, uint64_t key, int r)"):][:400]
    assert "mix64(seed ^ mix64(key * 0x100000001B3ull + (uint64_t)r))" in body
    assert "npyrng::Pcg64{mix64(h), mix64(h + 1), mix64(h + 2), mix64(h + 3) | 1ull}" in body
    hdr = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "memento_hip.h")).read())
    assert "h = mix64(seed ^ mix64(key * 0x100000001B3 + r))" in hdr and "restated in numpy in tests/_fast_ref.py" in hdr
    assert "not draw-for-draw identical" not in hdr


def test_sweep_is_the_designed_one():
    """The sweep's chains: the fixed sizes first, every multiplicity >= 1, the first draw's n p0 from 0.05 up to N / 2, the second
    draw flipped (pk > 0.5) in the even chains and not in the odd ones; a shorter sweep is a prefix of a longer one; sweep_pk is
    chain_operands; and the regime floors of the first 2,048 chains hold on the reference draws (the GPU test asserts the same
    before it launches)."""
    mults = sweep_mults(2048)
    N = mults.sum(axis=1)
    assert N[:8].tolist() == [2 ** 31 - 1, 2 ** 31 - 2, 2 ** 24 + 1, 2 ** 24, 2 ** 24 - 1, 61, 60, 3]
    assert N.min() == 3 and N.max() == 2 ** 31 - 1 and (mults >= 1).all() and (mults[:, 0] <= N / 2 + 1).all()
    np.testing.assert_array_equal(sweep_mults(8192)[:2048], mults)
    pk = sweep_pk(mults)
    for s in (0, 1, 5, 7, 100, 2047):
        np.testing.assert_array_equal(pk[s], chain_operands(mults[s], np.zeros(3), np.ones(3))[0])
    big = N >= 1000
    assert (pk[big & (np.arange(2048) % 2 == 0), 1] >= 0.499).all() and (pk[np.arange(2048) % 2 == 1, 1] <= 0.5).all()
    w = fast_weights_many(mults, SWEEP_SEED, SWEEP_KEY0 + np.arange(2048), np.arange(SWEEP_B))
    assert (w >= 0).all() and (w.sum(axis=1) == N[:, None]).all()
    got = vars(sweep_regimes(mults, w))
    print("\nregimes of the first 2,048 sweep chains, B = 64:", got)
    for k, floor in SWEEP_FLOORS.items():
        assert got[k] >= floor, (k, got[k], floor)
