"""Kernel-level tests of the strict gene-pair (2D) replay bootstrap (csrc/boot.hip: k_boot2d_replay<MINW, FAST, REC> behind
mm_boot2d_replay and mm_boot2d_replay_rec) and of mm_boot2d_fast against the numpy restatement of tests/_replay2d_ref.py.

The C-ABI is called on hand-built slot tables (tests/_replay2d_ref.py: layout2d), torch tensors serving as device memory: five
tiles with 64, 5 (one more than BOOT_TAIL_LANES; lane 63 a twin of long600), 4 and 1 active lanes and one of lanes that must
write nothing (K = 0 with a row; K = 5 without one; slot_rec = -1 with a valid K and row); every chain written once into the six
[rows][64] planes and once as 8-double records; output rows a permutation of the slots, 7 rows nothing addresses, ld = B + 4, a
payload in column 0 and a payload NaN in every other cell.  For EVERY active chain and every replicate the correlation is
written and lies within the derived rounding bound of ref_corr_2d on numpy's own multinomial draws -- or is exactly 1.0 where the
reference meets the sentinel, or (ambiguous replicates: a variance within 1000 of its own bounds of 0; at most 1 % of them) just
inside [-1, 1] -- and every other cell keeps its bits.  The worst ratios are printed (profiles/replay2d_kernel_tests.txt).

The strict kernels dump no weights: their draws are checked through the correlations (numpy's weights in the reference) and the
bit-identity of everything else to those launches; the sampler itself is proven draw for draw by tests/test_gpu_replay_kernels.py
on the same multiplicities."""

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from _replay_ref import PAD, SENTINEL, ref_weights
from _replay2d_ref import (AMBIGUOUS, SENT, SPECIAL, VALUE, chain_operands_2d, full_tiles_2d, layout2d, many_tiles_2d, menu2d, ref_corr_2d,
                           twin_tiles_2d)

pytestmark = pytest.mark.gpu

B = 150
ENTRIES = ["planes", "records"]                  # mm_boot2d_replay, mm_boot2d_replay_rec
NAME = {"planes": "mm_boot2d_replay", "records": "mm_boot2d_replay_rec", "fast": "mm_boot2d_fast"}
GUARD = 4096                                     # int32 cells of pad pattern on both ends of a weight buffer
SENT_BITS = np.array([SENTINEL]).view(np.int64)[0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


# ------------------------------------------------------------------------------------------------------------------------
# references (computed once per module, never changed) and launches
# ------------------------------------------------------------------------------------------------------------------------

_REF = {}
_FIELDS = ("corr", "raw", "bound", "kind")


def _ref_on(c, w):
    o = chain_operands_2d(c)
    return ref_corr_2d(c.x1, c.x2, o.ops[4], o.ops[5], w, c.N, c.q)


def _cut(r, nb):
    return SimpleNamespace(**{f: getattr(r, f)[:nb] for f in _FIELDS})


def _ref(name, nb, seed=5):
    """ref_corr_2d of a menu chain on numpy's weights (B = 150 replicates; a shorter run draws the first ones of them)."""
    if (name, seed) not in _REF:
        c = menu2d()[name]
        r = _ref_on(c, ref_weights(c.mult, B, seed))
        for f in _FIELDS:
            getattr(r, f).setflags(write=False)
        _REF[name, seed] = r
    return _cut(_REF[name, seed], nb)


class Dev:
    """A layout on the device."""

    def __init__(self, eng, L):
        self.L = L
        d = eng.dev
        self.planes = [d(L.planes[i]) for i in range(6)]
        self.recs = d(L.recs)
        self.tile_ptr = d(L.tile_ptr)
        nobs, omq = d(L.slot_nobs), d(L.slot_omq)
        self.slot = [d(L.slot_K), nobs, omq, d(L.slot_row)]
        self.rec = [d(L.slot_rec), d(L.rec_K), nobs, omq, d(L.rec_row)]
        self.key = d(L.slot_key)


def _args(eng, D, entry, state, nb, ld, d_out, n_tiles):
    P = eng.P
    if entry == "planes":
        return [*map(P, D.planes), P(D.tile_ptr), n_tiles, *map(P, D.slot), state, nb, ld, P(d_out), eng._stream()]
    return [P(D.recs), P(D.rec[0]), n_tiles, *map(P, D.rec[1:]), state, nb, ld, P(d_out), eng._stream()]


def _launch(eng, D, entry, nb, seed=5, n_tiles=None):
    """One launch of an entry point over the layout ``D`` on a sentinel output."""
    L = D.L
    init = L.out_init(nb)
    d_out = eng.dev(init)
    eng._lib.call(NAME[entry], *_args(eng, D, entry, eng.pcg64_state(seed), nb, nb + 4, d_out, L.n_tiles if n_tiles is None else n_tiles))
    return SimpleNamespace(L=L, nb=nb, entry=entry, init=init, out=eng.host(d_out))            # (synchronises)


def _launch_fast(eng, D, nb, seed=3):
    """mm_boot2d_fast over the planes of ``D`` with a weight dump [slot][kmax][nb] of pad pattern between two guard bands."""
    L, P = D.L, eng.P
    init = L.out_init(nb)
    d_out = eng.dev(init)
    n_w = L.n_slots * L.kmax * nb
    d_w = eng.dev(np.full(n_w + 2 * GUARD, PAD, dtype=np.uint32))
    eng._lib.call("mm_boot2d_fast", *map(P, D.planes), P(D.tile_ptr), L.n_slots, *map(P, D.slot), P(D.key), seed, nb, nb + 4, P(d_out),
                  ctypes.c_void_p(d_w.data_ptr() + 4 * GUARD), L.kmax, eng._stream())
    return SimpleNamespace(L=L, nb=nb, entry="fast", init=init, out=eng.host(d_out), w=eng.host(d_w, np.uint32))


def _check(res, ref_of):
    """Everything part A asks of one launch; ``ref_of(e)`` is the reference of entry ``e`` (the fields of ref_corr_2d, [nb]).
    Returns the worst ratio of error to derived bound and the counts of value, sentinel and ambiguous replicates."""
    L, nb, what = res.L, res.nb, NAME[res.entry]
    active = [e for e in L.ents if e.kind == "run"]
    assert len(active) > 0
    written = np.zeros(res.init.shape, dtype=bool)
    st = SimpleNamespace(worst=0.0, n_value=0, n_sent=0, n_amb=0, n_amb_ordinary=0, n_ordinary=0)
    L_ = np.longdouble
    for e in active:
        got = res.out[e.row, 1:1 + nb]
        written[e.row, 1:1 + nb] = True
        assert (_bits(got) != SENT_BITS).all(), f"{what}: {e.label}: {int((_bits(got) == SENT_BITS).sum())} replicates not written"
        assert (np.abs(got) <= 1.0).all(), f"{what}: {e.label}: a replicate outside [-1, 1] (or NaN): {got[~(np.abs(got) <= 1.0)][:3]!r}"
        r = ref_of(e)
        sent, val, amb = r.kind == SENT, r.kind == VALUE, r.kind == AMBIGUOUS
        bad = np.flatnonzero(sent & (got != 1.0))
        assert len(bad) == 0, f"{what}: {e.label}: replicate {bad[0]}: {got[bad[0]]!r} where the reference keeps the 5.0 sentinel (exactly 1.0)"
        err = np.abs(got.astype(L_) - np.where(val, r.corr, L_(0.0)))
        ratio = np.where(val, err / np.where(val, r.bound, L_(1.0)), L_(0.0)).astype(np.float64)
        k = int(np.argmax(ratio))
        assert ratio[k] <= 1.0, (f"{what}: {e.label}: replicate {k}: {got[k]!r} is {ratio[k]:.3g} of its bound {float(r.bound[k]):.3g} from "
                                 f"{float(r.corr[k])!r}")
        clipped = val & (np.abs(r.raw) > 1 + r.bound)                  # beyond the clip by more than the bound: exactly +-1.0
        bad = np.flatnonzero(clipped & (got != np.sign(r.raw).astype(np.float64)))
        assert len(bad) == 0, f"{what}: {e.label}: replicate {bad[0]}: {got[bad[0]]!r} where the reference is clipped from {float(r.raw[bad[0]])!r}"
        st.worst = max(st.worst, float(ratio[k]))
        st.n_value, st.n_sent, st.n_amb = st.n_value + int(val.sum()), st.n_sent + int(sent.sum()), st.n_amb + int(amb.sum())
        if e.chain.name in SPECIAL:
            assert not amb.any(), e.label
            want = {"anti": -1.0}.get(e.chain.name, 1.0)               # zero_left, overflow, one_bin2d: the sentinel; same, anti: the clip
            assert (got == want).all(), f"{what}: {e.label}: {got[got != want][:3]!r} instead of exactly {want}"
        else:
            st.n_ordinary += nb
            st.n_amb_ordinary += int(amb.sum())
            assert amb.sum() <= 0.05 * max(nb, 20), f"{what}: {e.label}: {int(amb.sum())} ambiguous replicates"
    assert st.n_amb_ordinary <= 0.01 * max(st.n_ordinary, 100), f"{what}: {st.n_amb_ordinary} ambiguous replicates of {st.n_ordinary}"
    # every other cell -- column 0, the padding columns, unaddressed rows, rows of lanes that must write nothing -- as it was
    bad = np.argwhere(~written & (_bits(res.out) != _bits(res.init)))
    if len(bad):
        owner = {e.row: e.label for e in L.ents}
        r, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} cells that must stay untouched changed, the first at row {r} column {c} "
                             f"({owner.get(int(r), 'a row nothing addresses')}): {res.out[r, c]!r}")
    return st


def _numpy_ref(nb, seed=5):
    return lambda e: _ref(e.chain.name, nb, seed)


def _report(res, st, extra=""):
    print(f"\n{NAME[res.entry]}: B = {res.nb}{extra}, {sum(e.kind == 'run' for e in res.L.ents)} chains: worst ratio to the derived bound "
          f"{st.worst:.3g}; {st.n_value} value, {st.n_sent} sentinel, {st.n_amb} ambiguous replicates")


@pytest.fixture(scope="module")
def world(eng):
    """The layouts on the device and the launches the tests share: ``run(entry)`` is the part A launch (B = 150, full layout)."""
    import torch

    w = SimpleNamespace(full=Dev(eng, layout2d(full_tiles_2d())), small=Dev(eng, layout2d(full_tiles_2d(with_long_twin=False, first=False))),
                        cache={})

    def run(entry):
        if entry not in w.cache:
            w.cache[entry] = _launch(eng, w.full, entry, B)
        return w.cache[entry]

    w.run = run
    yield w
    w.cache.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------
# A. each entry point against numpy
# ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_point_against_numpy(world, entry):
    """B = 150, seed 5, the full layout: every replicate of every active chain is written and is ref_corr_2d's within the derived
    bound (exactly 1.0 at the sentinel; ambiguous ones inside [-1, 1]), the special chains give their exact values, and column 0,
    the three pad columns, the unaddressed rows and the rows of the k0, norow and norec lanes keep their bits."""
    res = world.run(entry)
    L = res.L
    assert [sum(1 for e in L.ents if e.tile == t and e.kind == "run") for t in range(5)] == [64, 5, 4, 1, 0]
    assert sorted(e.kind for e in L.ents if e.tile == 4) == ["k0", "norec", "norow"]
    st = _check(res, _numpy_ref(B))
    _report(res, st)
    assert st.n_sent > 4 * B and st.n_value > 60 * B


# ------------------------------------------------------------------------------------------------------------------------
# B. bit-identity between paths
# ------------------------------------------------------------------------------------------------------------------------


def _same_chains(res, base, what, by_position=False, n_tiles=None):
    """Every active chain of ``res`` (of its first ``n_tiles`` tiles) against the chain of the same name (or at the same tile and
    lane) in ``base``: the first res.nb replicates are bit-identical.  Returns the number of chains compared."""
    first = {}
    for e in base.L.ents:
        if e.kind == "run":
            first.setdefault((e.tile, e.lane) if by_position else e.chain.name, e)
    n = 0
    for e in res.L.ents:
        if e.kind != "run" or (n_tiles is not None and e.tile >= n_tiles):
            continue
        o = first[(e.tile, e.lane) if by_position else e.chain.name]
        assert o.chain.name == e.chain.name
        a, b = res.out[e.row, 1:1 + res.nb], base.out[o.row, 1:1 + res.nb]
        bad = np.flatnonzero(_bits(a) != _bits(b))
        assert len(bad) == 0, f"{what}: {e.label} differs from {o.label} in {len(bad)} replicates, the first {bad[0]}: {a[bad[0]]!r} / {b[bad[0]]!r}"
        n += 1
    return n


def test_two_entry_points_agree_bit_for_bit(world):
    """The whole output planes of mm_boot2d_replay and mm_boot2d_replay_rec on the full layout, as int64 views."""
    a, b = world.run("planes"), world.run("records")
    bad = np.argwhere(_bits(a.out) != _bits(b.out))
    assert len(bad) == 0, f"{len(bad)} cells differ, the first at {bad[0].tolist()}: {a.out[tuple(bad[0])]!r} / {b.out[tuple(bad[0])]!r}"
    assert _same_chains(a, b, "planes / records", by_position=True) == 74


@pytest.mark.parametrize("entry", ENTRIES)
def test_twin_layout_gives_the_same_bits(eng, world, entry):
    """The same chains in other lanes, tiles and company (the special chains of the 5- and 4-lane tiles inside the 64-lane tile,
    four fillers in their place, the tile of unused lanes first): every chain's row is bit-identical to the full layout's."""
    res = _launch(eng, Dev(eng, layout2d(twin_tiles_2d())), entry, B)
    _check(res, _numpy_ref(B))
    assert _same_chains(res, world.run(entry), f"{NAME[entry]}, twin layout") == 74
    base = world.run(entry)                                                  # and the twins inside the full layout (long600, btpe12, ...)
    first, twins = {}, 0
    for e in base.L.ents:
        if e.kind == "run" and first.setdefault(e.chain.name, e) is not e:
            o = first[e.chain.name]
            assert np.array_equal(_bits(base.out[e.row, 1:1 + B]), _bits(base.out[o.row, 1:1 + B])), f"{NAME[entry]}: {e.label} != {o.label}"
            twins += 1
    assert twins >= 5


# ------------------------------------------------------------------------------------------------------------------------
# C. replicate counts around a wave
# ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nb", [1, 64, 65])
@pytest.mark.parametrize("entry", ENTRIES)
def test_small_num_boot(eng, world, entry, nb):
    """The reduced layout (tiles 1 to 4 without the long600 twin) with 1, 64 and 65 replicates: everything part A asks, and
    replicate r is replicate r of the B = 150 launch bit for bit."""
    res = _launch(eng, world.small, entry, nb)
    st = _check(res, _numpy_ref(nb))
    _report(res, st, " (reduced layout)")
    assert _same_chains(res, world.run(entry), f"{NAME[entry]}, B = {nb}") == 9


# ------------------------------------------------------------------------------------------------------------------------
# D. the variants nothing small reaches
# ------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def many(eng):
    """More than 2,048 tiles: the five real ones and 2,044 tiles of one k2 chain each."""
    import torch

    D = Dev(eng, layout2d(many_tiles_2d()))
    assert D.L.n_tiles == 2049
    yield D
    del D
    torch.cuda.empty_cache()


@pytest.fixture
def exact_arith(eng):
    """Switches mm_debug_replay_arith(1) on when called.  The switch is process-wide: the finalizer takes it back whatever the
    test does, so a failing assertion cannot leak it into later tests."""
    yield lambda: eng._lib.call("mm_debug_replay_arith", 1)
    eng._lib.call("mm_debug_replay_arith", 0)


@pytest.mark.parametrize("entry", ENTRIES)
def test_three_waves_per_simd_build(eng, world, many, entry):
    """n_tiles = 2,049 > 2,048: the launch takes k_boot2d_replay<3, ., .>.  All 2,118 chains against numpy; the five real tiles
    bit-identical to part A's (the two-wave build)."""
    base = world.run(entry)
    res = _launch(eng, many, entry, B)
    _check(res, _numpy_ref(B))
    assert _same_chains(res, base, f"{NAME[entry]}, 2,049 tiles", by_position=True, n_tiles=5) == 74
    assert _same_chains(res, base, f"{NAME[entry]}, 2,049 tiles") == 74 + 2044


@pytest.mark.parametrize("tiles", ["five-tiles", "many-tiles"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_exact_arithmetic_instantiations(eng, world, many, exact_arith, entry, tiles):
    """The FAST = false instantiations (two and three waves per SIMD) of both entry points: bit-identical to the default build."""
    base = world.run(entry)                           # the default arithmetic: launched (or cached) before the switch goes on
    exact_arith()
    if tiles == "five-tiles":
        res = _launch(eng, world.full, entry, B)
        _check(res, _numpy_ref(B))
        assert np.array_equal(_bits(res.out), _bits(base.out))
    else:
        res = _launch(eng, many, entry, 65)
        _check(res, _numpy_ref(65))
        assert _same_chains(res, base, f"{NAME[entry]}, exact arithmetic, 2,049 tiles") == 74 + 2044


@pytest.mark.parametrize("entry", ENTRIES)
def test_second_seed(eng, world, entry):
    """pcg_state of PCG64(11) on the full layout: numpy's multinomial with that seed (a hard-coded state or increment would fail
    here), and other draws than seed 5's."""
    res = _launch(eng, world.full, entry, B, seed=11)
    st = _check(res, _numpy_ref(B, 11))
    _report(res, st, ", seed 11")
    base = world.run(entry)
    differ = sum(not np.array_equal(_bits(res.out[e.row]), _bits(base.out[e.row])) for e in res.L.ents if e.kind == "run" and e.chain.K > 1)
    assert differ >= 40


# ------------------------------------------------------------------------------------------------------------------------
# E. guards: every call here returns before any launch
# ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("entry", ENTRIES)
def test_guards(eng, world, entry):
    """A NULL pointer among the required ones, num_boot = 0, ld = num_boot, n_tiles < 0 and n_tiles >= 2^31 - 1 give the library's
    argument error and a text in mm_last_error; n_tiles = 0 returns 0.  None of them writes a cell."""
    D = world.small
    lib = eng._lib.load()
    fn = getattr(lib, NAME[entry])
    nb = 8
    init = D.L.out_init(nb)
    d_out = eng.dev(init)
    state = eng.pcg64_state(5)
    null = ctypes.c_void_p(0)

    def args(nb=nb, ld=nb + 4, n=D.L.n_tiles, null_at=None):
        a = _args(eng, D, entry, state, nb, ld, d_out, n)
        if null_at is not None:
            assert isinstance(a[null_at], ctypes.c_void_p) and a[null_at].value
            a[null_at] = null
        return a

    i_out = len(args()) - 2
    cases = {"d_out_corr NULL": dict(null_at=i_out), "num_boot = 0": dict(nb=0), "ld = num_boot": dict(ld=nb), "n_tiles = -1": dict(n=-1),
             "n_tiles = 2^31 - 1": dict(n=2 ** 31 - 1), "n_tiles = 2^40": dict(n=2 ** 40)}
    for i in range(7 if entry == "planes" else 2):                     # the operand planes and tile_ptr / the records and slot_rec
        cases[f"argument {i} NULL"] = dict(null_at=i)
    for i in range(4):                                                 # slot_K, slot_nobs, slot_omq, slot_row
        cases[f"slot table {i} NULL"] = dict(null_at=(8 if entry == "planes" else 3) + i)
    bad_arg = fn(*args(nb=0))
    assert bad_arg < 0
    for what, kw in cases.items():
        rc = fn(*args(**kw))
        assert rc == bad_arg, f"{NAME[entry]}: {what}: status {rc}"
        assert b"bad argument" in lib.mm_last_error(), what
    a = args()
    a[i_out - 3] = None                                                # pcg_state NULL
    assert fn(*a) == bad_arg
    assert fn(*args(n=0)) == 0
    eng._torch().cuda.synchronize()
    assert np.array_equal(_bits(eng.host(d_out)), _bits(init))


# ------------------------------------------------------------------------------------------------------------------------
# F. mm_boot2d_fast on the same layout
# ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("which, nb", [("full", B), ("reduced", 65)])
def test_fast_kernel_on_the_layout(eng, world, which, nb):
    """mm_boot2d_fast on the planes of the layout (full at B = 150; reduced at B = 65: one full wave of replicates and one with a
    single live lane, whose other 63 lanes must store nothing): the dumped weights of every active chain are non-negative and sum
    to its cell count, each replicate is ref_corr_2d of those weights within the same bound, the k0 and norow lanes (and the
    empty lanes) write and dump nothing -- every weight cell outside k < K of the active slots keeps the pad pattern between the
    guard bands -- and every other output cell keeps its bits."""
    D = world.full if which == "full" else world.small
    L = D.L
    res = _launch_fast(eng, D, nb)
    body = res.w[GUARD:GUARD + L.n_slots * L.kmax * nb].reshape(L.n_slots, L.kmax, nb)
    want = np.full(res.w.shape, PAD, dtype=np.uint32)
    want_body = want[GUARD:GUARD + L.n_slots * L.kmax * nb].reshape(L.n_slots, L.kmax, nb)
    weights = {}
    for e in L.ents:
        if e.kind != "run":
            continue
        w = body[e.slot, :e.K].astype(np.int32).astype(np.int64)
        assert (body[e.slot, :e.K] != PAD).all(), f"mm_boot2d_fast: {e.label}: weights not dumped"
        assert (w >= 0).all() and (w.sum(axis=0) == e.chain.N).all(), f"mm_boot2d_fast: {e.label}: weights do not sum to {e.chain.N}"
        weights[e.slot] = w
        want_body[e.slot, :e.K] = body[e.slot, :e.K]
    if not np.array_equal(res.w, want):
        at = np.flatnonzero(res.w != want)
        raise AssertionError(f"mm_boot2d_fast: {len(at)} weight cells outside k < K of the active slots changed, the first at word "
                             f"{int(at[0]) - GUARD} (guard band: {GUARD} words): {res.w[at[0]]:#x}")
    st = _check(res, lambda e: _cut(_ref_on(e.chain, weights[e.slot]), nb))
    _report(res, st, f" ({which} layout)")
    # streams are keyed by slot: twins of one chain draw different weights, replicates of one chain differ
    twins = [e for e in L.ents if e.kind == "run" and e.chain.name == "btpe12"]
    assert len(twins) == (2 if which == "full" else 1)
    if which == "full":
        assert not np.array_equal(weights[twins[0].slot], weights[twins[1].slot])
    assert len({weights[twins[0].slot][:, r].tobytes() for r in range(nb)}) == nb
