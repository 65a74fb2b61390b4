"""The five rng='fast' entry points (csrc/boot.hip: mm_boot1d_fast, mm_boot1d_fast_range, mm_boot2d_fast, mm_boot2d_fast_range,
mm_boot2d_fast_slots) draw for draw against numpy, on the synthetic menus of tests/_replay_ref.py and tests/_replay2d_ref.py.

Replicate r of the chain with key ``key`` owns the PCG64 stream of tests/_fast_ref.py: fast_state(seed, key, r), and numpy's own
Generator.multinomial on that stream (fast_weights) is what the kernel must dump, cell for cell.  The C-ABI is called on the
hand-built layouts of the replay kernel tests (five tiles with 64, 5, 4 and 1 active lanes and one of lanes that must write
nothing), which the fast kernels read through the same planes, tile_ptr and slot tables, plus a key per slot and a seed:

  * every cell of d_w_dump of every active slot equals fast_weights; the cells of unused, K < 2 (1D) / K <= 0 (2D) and row < 0
    slots, the cells beyond K and the guard bands keep the pad pattern;
  * the replicate means and variances (1D) and correlations (2D) lie within the derived bounds of ref_moments / ref_corr_2d
    evaluated in np.longdouble on numpy's weights -- not on the kernel's own dump --, and every other output cell keeps its bits;
  * B = 1, 63, 64, 65 and 130 (the 64-replicate chunk boundary; lanes >= num_boot walk along and store nothing), seeds 0 and
    0xDEADBEEF12345678, keys 0, 1, 2^40, the largest key of the header's distinctness rule and a negative one, equal operands under
    different keys, equal keys (equal weights: a key, not a slot, owns a stream), rep_lo = 0, 64 and 2^31 - 1 - rep_n, chains
    closed through row -1, and slot lists whose wave count is no multiple of the four waves of a workgroup."""

import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from _fast_ref import MAX_DISTINCT_KEY, fast_weights
from _replay_ref import PAD, SENTINEL, chain_operands, full_tiles, layout, menu, ref_moments
from _replay2d_ref import full_tiles_2d, layout2d, menu2d

pytestmark = pytest.mark.gpu

GUARD = 4096
SENT_BITS = np.array([SENTINEL]).view(np.int64)[0]
SEEDS = (0, 0xDEADBEEF12345678)
BS = (1, 63, 64, 65, 130)
TOP = 2 ** 31 - 1
# (tile, lane) -> key, the same places in the 1D and the 2D layout (tests/_replay_ref.py: full_tiles, tests/_replay2d_ref.py:
# full_tiles_2d).  btpe12 and huge sit in tile 0 (lane by permutation) and again in lanes 7 and 40 of tile 1: the two btpe12 get
# the keys 2^40 and 1 (equal operands, different keys), the two huge one key (equal keys: equal weights)
SPECIAL_KEYS = {(1, 0): 0, (1, 7): 1, (1, 31): MAX_DISTINCT_KEY, (1, 63): -5, (1, 40): 424242, (3, 17): -(2 ** 63)}
TILE0_KEYS = {"btpe12": 2 ** 40, "huge": 424242}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


def _keys(L):
    keys = (np.arange(L.n_slots, dtype=np.int64) * 7919 + 13) % 1000003
    for (t, lane), k in SPECIAL_KEYS.items():
        keys[t * 64 + lane] = k
    for e in L.ents:
        if e.tile == 0 and e.chain is not None and e.chain.name in TILE0_KEYS:
            keys[e.slot] = TILE0_KEYS[e.chain.name]
    return keys


def _pair(W, name):
    """The slots of chain ``name`` in tile 0 and in tile 1."""
    a, b = [e.slot for e in W.active if e.chain.name == name and e.tile in (0, 1)]
    return a, b


@functools.lru_cache(maxsize=None)
def _want(dim, name, seed, key, rep_lo, nb):
    """numpy's weights [K][nb] of a menu chain on the streams of the global replicates rep_lo .. rep_lo + nb - 1 (computed once)."""
    m = menu() if dim == 1 else menu2d()
    w = fast_weights(m[name].mult, seed, key, rep_lo + np.arange(nb))
    w.setflags(write=False)
    return w


class World:
    """A layout on the device with its keys."""

    def __init__(self, eng, L, dim):
        d = eng.dev
        self.L, self.dim = L, dim
        self.keys = _keys(L)
        self.planes = [d(L.planes[i]) for i in range(5 if dim == 1 else 6)]
        self.tile_ptr = d(L.tile_ptr)
        self.slot = [d(L.slot_K), d(L.slot_nobs), d(L.slot_omq)]
        self.d_row, self.d_key = d(L.slot_row), d(self.keys)
        self.active = [e for e in L.ents if e.kind == "run"]


@pytest.fixture(scope="module")
def worlds(eng):
    import torch

    w = SimpleNamespace(one=World(eng, layout(full_tiles()), 1), two=World(eng, layout2d(full_tiles_2d()), 2))
    yield w
    torch.cuda.empty_cache()


def _launch(eng, W, seed, nb, rep_lo=None, mean_only=0, closed=(), listed=None):
    """One launch over the layout ``W``: mm_boot{1,2}d_fast (rep_lo None), _range, or (``listed``: slots) mm_boot2d_fast_slots, on
    sentinel outputs with ld = nb + 4 and a weight dump of pad pattern between guard bands.  ``closed``: slots given row -1."""
    L, P, dim = W.L, eng.P, W.dim
    ld = nb + 4
    init = np.full((L.n_rows, ld), SENTINEL)
    init[:, 0] = 1000.0 + np.arange(L.n_rows)
    outs = [eng.dev(init) for _ in range(3 - dim)]
    n_w = L.n_slots * L.kmax * nb
    assert L.kmax >= max(e.K for e in L.ents) and all(0 <= e.row < L.n_rows for e in W.active)
    d_w = eng.dev(np.full(n_w + 2 * GUARD, PAD, dtype=np.uint32))
    p_w = ctypes.c_void_p(d_w.data_ptr() + 4 * GUARD)
    d_row = W.d_row
    if len(closed):
        row = L.slot_row.copy()
        row[list(closed)] = -1
        d_row = eng.dev(row)
    head = [*map(P, W.planes), P(W.tile_ptr), L.n_slots, *map(P, W.slot), P(d_row), P(W.d_key), seed]
    mo = [mean_only] if dim == 1 else []
    s = eng._stream()
    if listed is not None:
        d_list = eng.dev(np.asarray(listed, dtype=np.int64))
        eng._lib.call("mm_boot2d_fast_slots", *head, rep_lo, nb, ld, P(outs[0]), P(d_list), len(listed), s)
    elif rep_lo is None:
        eng._lib.call(f"mm_boot{dim}d_fast", *head, nb, *mo, ld, *map(P, outs), p_w, L.kmax, s)
    else:
        eng._lib.call(f"mm_boot{dim}d_fast_range", *head, rep_lo, nb, *mo, ld, *map(P, outs), p_w, L.kmax, s)
    res = SimpleNamespace(L=L, nb=nb, init=init, out=[eng.host(o) for o in outs], w=eng.host(d_w, np.uint32), seed=seed,
                          rep_lo=rep_lo or 0, closed=set(closed), listed=None if listed is None else set(int(x) for x in listed))
    res.ran = [e for e in W.active if e.slot not in res.closed and (res.listed is None or e.slot in res.listed)]
    res.want = {e.slot: _want(dim, e.chain.name, seed, int(W.keys[e.slot]), res.rep_lo, nb) for e in res.ran}
    return res


def _check_weights(res, what):
    """Every weight cell: fast_weights in k < K of the slots that ran, the pad pattern everywhere else."""
    L, nb = res.L, res.nb
    want = np.full(res.w.shape, PAD, dtype=np.uint32)
    body = want[GUARD:GUARD + L.n_slots * L.kmax * nb].reshape(L.n_slots, L.kmax, nb)
    got = res.w[GUARD:GUARD + L.n_slots * L.kmax * nb].reshape(L.n_slots, L.kmax, nb)
    for e in res.ran:
        w = res.want[e.slot]
        assert w.shape == (e.K, nb)
        bad = np.argwhere(got[e.slot, :e.K].astype(np.int32).astype(np.int64) != w)
        assert len(bad) == 0, (f"{what}: {e.label}: {len(bad)} of {w.size} weights differ from numpy's, the first at (bin, replicate) = "
                               f"{bad[0].tolist()}: {got[e.slot][tuple(bad[0])]} instead of {w[tuple(bad[0])]}")
        body[e.slot, :e.K] = w.astype(np.uint32)
    if not np.array_equal(res.w, want):
        at = np.flatnonzero(res.w != want)
        raise AssertionError(f"{what}: {len(at)} weight cells outside k < K of the slots that ran changed, the first at word "
                             f"{int(at[0]) - GUARD} (guard band: {GUARD} words): {res.w[at[0]]:#x}")


def _check_untouched(res, written, what):
    for plane in res.out:
        bad = np.argwhere(~written & (_bits(plane) != _bits(res.init)))
        if len(bad):
            owner = {e.row: e.label for e in res.L.ents}
            r, c = bad[0]
            raise AssertionError(f"{what}: {len(bad)} cells that must stay untouched changed, the first at row {r} column {c} "
                                 f"({owner.get(int(r), 'a row nothing addresses')}): {plane[r, c]!r}")


def _check_moments_1d(res, what, mean_only=0):
    """Means and variances within ref_moments' bounds of the longdouble evaluation on numpy's weights; everything else untouched."""
    nb = res.nb
    written = np.zeros(res.init.shape, dtype=bool)
    worst = [0.0, 0.0]
    L_ = np.longdouble
    for e in res.ran:
        c = e.chain
        _, _, v, a, b = chain_operands(c.mult, c.v, c.sf)
        m1, var, b1, bv = ref_moments(v, a, b, res.want[e.slot], c.N, c.q, mean_only=bool(mean_only))
        written[e.row, 1:1 + nb] = True
        for i, (ref, bound, name) in enumerate(((m1, b1, "mean"), (var, bv, "variance"))):
            got = res.out[i][e.row, 1:1 + nb]
            assert (_bits(got) != SENT_BITS).all(), f"{what}: {e.label}: replicates not written"
            err = np.abs(got.astype(L_) - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf)).astype(np.float64)
            r = int(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)))
            assert ratio[r] <= 1.0, f"{what}: {e.label}: replicate {r}: {name} {got[r]!r} is {ratio[r]:.3g} of its bound from {float(ref[r])!r}"
            worst[i] = max(worst[i], float(ratio[r]))
    _check_untouched(res, written, what)
    return worst


def _check_corr_2d(res, what):
    """Correlations against ref_corr_2d on numpy's weights, by the rules of tests/test_gpu_replay2d_kernels.py: _check (a launch of
    which ``res`` is made to look like: the chains that did not run are lanes that must write nothing)."""
    from test_gpu_replay2d_kernels import _check, _cut, _ref_on

    ran = {e.slot for e in res.ran}
    ents = [e if (e.kind != "run" or e.slot in ran) else SimpleNamespace(**{**vars(e), "kind": "idle"}) for e in res.L.ents]
    view = SimpleNamespace(L=SimpleNamespace(ents=ents), nb=res.nb, entry="fast", init=res.init, out=res.out[0])
    st = _check(view, lambda e: _cut(_ref_on(e.chain, res.want[e.slot]), res.nb))
    print(f"\n{what}: {len(ran)} chains: worst ratio to the derived bound {st.worst:.3g}; {st.n_value} value, {st.n_sent} sentinel, "
          f"{st.n_amb} ambiguous replicates")
    return st


def _slot(t, lane):
    return t * 64 + lane


def _check_pairs(res, W):
    """The dumped weights (already equal to numpy's) of the two huge chains -- one key -- are equal; those of the two btpe12 chains
    -- equal operands, keys 2^40 and 1 -- share no replicate (11 draws of n p of several hundred each)."""
    got = res.w[GUARD:GUARD + res.L.n_slots * res.L.kmax * res.nb].reshape(res.L.n_slots, res.L.kmax, res.nb)
    a, b = _pair(W, "huge")
    np.testing.assert_array_equal(got[a], got[b])
    a, b = _pair(W, "btpe12")
    assert (got[a, :12] != got[b, :12]).any(axis=0).all()


# ------------------------------------------------------------------------------------------------------------------------
# 1D
# ------------------------------------------------------------------------------------------------------------------------


def test_layouts_and_keys_are_the_designed_ones(worlds):
    """Both layouts: 64 / 5 / 4 / 1 / 0 active lanes; every special key once, the two huge chains under one key, the btpe12 chains of
    tiles 0 and 1 under 2^40 and 1, no other two active slots with one key."""
    for W in (worlds.one, worlds.two):
        L = W.L
        assert [sum(1 for e in L.ents if e.tile == t and e.kind == "run") for t in range(5)] == [64, 5, 4, 1, 0]
        a, b = _pair(W, "huge")
        assert W.keys[a] == W.keys[b] == 424242
        keys = [int(W.keys[e.slot]) for e in W.active]
        for k in (0, 1, 2 ** 40, MAX_DISTINCT_KEY, -5, -(2 ** 63)):
            assert keys.count(k) == 1
        assert [int(W.keys[s]) for s in _pair(W, "btpe12")] == [2 ** 40, 1]
        assert len(set(keys)) == len(keys) - 1                               # one pair of equal keys, no other
    assert sorted(e.kind for e in worlds.one.L.ents if e.tile == 4) == ["k0", "k1", "norec", "norow"]


@pytest.mark.parametrize("seed", SEEDS, ids=["seed0", "seedbig"])
@pytest.mark.parametrize("nb", BS)
def test_boot1d_fast_draw_for_draw(eng, worlds, nb, seed):
    """mm_boot1d_fast on the full layout: every weight cell (fast_weights in k < K of the 74 active slots, the pad pattern in the
    K == 1, K == 0, row -1 and empty slots, beyond K and in the guard bands), means and variances within ref_moments' bounds on
    numpy's weights (B = 63 with mean_only: mean + 1 and exactly 10), every other output cell untouched."""
    mean_only = int(nb == 63)
    res = _launch(eng, worlds.one, seed, nb, mean_only=mean_only)
    what = f"mm_boot1d_fast B = {nb} seed {seed:#x}"
    _check_weights(res, what)
    worst = _check_moments_1d(res, what, mean_only)
    if mean_only:
        assert all((res.out[1][e.row, 1:1 + nb] == 10.0).all() for e in res.ran)
    _check_pairs(res, worlds.one)
    print(f"\n{what}: {len(res.ran)} chains, {sum(w.size for w in res.want.values())} weights equal numpy's; worst ratio to the derived "
          f"bound: mean {worst[0]:.3g}, variance {worst[1]:.3g}")


RANGES = [(0, 65, 0), (64, 66, 1), (64, 1, 0), (TOP - 65, 65, 1), (TOP - 130, 130, 0), (TOP - 1, 1, 1)]


def _closed(W):
    """Chains closed through row -1: the key-0 chain, one of the equal-key pair, and every third lane of the 64-lane tile."""
    return [_slot(1, 0), _slot(1, 40)] + [e.slot for e in W.active if e.tile == 0 and e.lane % 3 == 0]


@pytest.mark.parametrize("rep_lo, nb, si", RANGES, ids=[f"lo{a}-n{b}" for a, b, _ in RANGES])
def test_boot1d_fast_range_draw_for_draw(eng, worlds, rep_lo, nb, si):
    """mm_boot1d_fast_range: local replicate i is global replicate rep_lo + i, up to the last one (rep_lo + rep_n = 2^31 - 1); with
    rep_lo = 64 the chains closed through row -1 write and dump nothing."""
    W = worlds.one
    closed = _closed(W) if rep_lo == 64 else ()
    res = _launch(eng, W, SEEDS[si], nb, rep_lo=rep_lo, closed=closed)
    what = f"mm_boot1d_fast_range [{rep_lo}, {rep_lo + nb}) seed {SEEDS[si]:#x}"
    assert len(res.ran) == len(W.active) - len(closed) and (not closed or len(closed) >= 20)
    _check_weights(res, what)
    worst = _check_moments_1d(res, what)
    if rep_lo == 64 and nb == 66:          # the range continues the one-shot run: its columns are that run's columns 64 ..
        for e in res.ran[:5]:
            np.testing.assert_array_equal(res.want[e.slot], _want(1, e.chain.name, SEEDS[si], int(W.keys[e.slot]), 0, 130)[:, 64:])
    print(f"\n{what}: {len(res.ran)} chains ({len(closed)} closed): worst ratio to the derived bound: mean {worst[0]:.3g}, variance {worst[1]:.3g}")


def test_boot1d_range_arguments_beyond_the_last_replicate_are_refused(eng, worlds):
    """rep_lo + rep_n = 2^31 is refused before any launch (the last replicate a lane may store is 2^31 - 2)."""
    W = worlds.one
    for rep_lo, nb in ((TOP - 64, 65), (TOP, 1)):
        with pytest.raises(eng._lib.MementoHipError):
            _launch(eng, W, 0, nb, rep_lo=rep_lo)


# ------------------------------------------------------------------------------------------------------------------------
# 2D
# ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("seed", SEEDS, ids=["seed0", "seedbig"])
@pytest.mark.parametrize("nb", BS)
def test_boot2d_fast_draw_for_draw(eng, worlds, nb, seed):
    """mm_boot2d_fast on the full 2D layout: every weight cell as in 1D (a K == 1 chain runs and dumps its cell count), the
    correlations by the rules of ref_corr_2d on numpy's weights, every other output cell untouched."""
    res = _launch(eng, worlds.two, seed, nb)
    what = f"mm_boot2d_fast B = {nb} seed {seed:#x}"
    _check_weights(res, what)
    _check_corr_2d(res, what)
    _check_pairs(res, worlds.two)
    one =[e for e in res.ran if e.K == 1]
    assert len(one) == 1 and (res.want[one[0].slot] == one[0].chain.N).all()          # a K == 1 chain runs: the observed sample


@pytest.mark.parametrize("rep_lo, nb, si", RANGES, ids=[f"lo{a}-n{b}" for a, b, _ in RANGES])
def test_boot2d_fast_range_draw_for_draw(eng, worlds, rep_lo, nb, si):
    """mm_boot2d_fast_range on the ranges of the 1D test, the same chains closed through row -1 when rep_lo = 64."""
    W = worlds.two
    closed = _closed(W) if rep_lo == 64 else ()
    res = _launch(eng, W, SEEDS[si], nb, rep_lo=rep_lo, closed=closed)
    what = f"mm_boot2d_fast_range [{rep_lo}, {rep_lo + nb}) seed {SEEDS[si]:#x}"
    assert len(res.ran) == len(W.active) - len(closed)
    _check_weights(res, what)
    _check_corr_2d(res, what)


LISTS = [(0, 65, 0, 7), (64, 64, 1, 9), (TOP - 130, 130, 0, 5), (0, 1, 1, 74)]


@pytest.mark.parametrize("rep_lo, nb, si, n_list", LISTS, ids=[f"lo{a}-n{b}-list{d}" for a, b, _, d in LISTS])
def test_boot2d_fast_slots_draw_for_draw(eng, worlds, rep_lo, nb, si, n_list):
    """mm_boot2d_fast_slots dumps no weights: the correlations of the listed chains are ref_corr_2d's on numpy's weights, and the
    rows of every chain that is not listed keep their bits.  Lists of 7 slots x 2 chunks, 9 x 1 and 5 x 3 waves (no multiple of the
    four waves of a workgroup) and the whole layout; each list also names a K = 0 slot and a row -1 slot, which write nothing."""
    W = worlds.two
    L = W.L
    act = [e.slot for e in W.active]
    pick = act if n_list >= len(act) else [act[i] for i in np.random.default_rng(n_list).choice(len(act), size=n_list - 2, replace=False)]
    if n_list < len(act):
        pick = sorted(pick + [e.slot for e in L.ents if e.kind in ("k0", "norow")])
        assert len(pick) == n_list and (n_list * -(-nb // 64)) % 4 != 0
    res = _launch(eng, W, SEEDS[si], nb, rep_lo=rep_lo, listed=pick)
    what = f"mm_boot2d_fast_slots [{rep_lo}, {rep_lo + nb}) seed {SEEDS[si]:#x}, {n_list} slots"
    assert len(res.ran) == (len(act) if n_list >= len(act) else n_list - 2)
    assert (res.w == PAD).all()
    _check_corr_2d(res, what)
