"""Kernel-level tests of the strict 1D replay bootstrap (csrc/boot.hip: mm_boot1d_replay, mm_boot1d_free, mm_boot1d_chain,
mm_boot1d_async, the mm_chain_tiles argument of the first two) against the numpy restatement of tests/_replay_ref.py.

Parts B to D call the C-ABI on hand-built slot tables (tests/_replay_ref.py: layout), torch tensors serving as device memory:
five tiles with 64, 5 (one more than BOOT_TAIL_LANES), 4 and 1 active lanes and one of lanes that must write nothing; every chain
written once into the [rows][64] planes and once as 8-double records; output rows a permutation of the slots, 7 rows nothing
addresses, ld = B + 4, every output cell a payload NaN, every weight cell outside k < K a pad pattern between guard bands.  For
EVERY active chain and every replicate the int32 weights equal numpy's multinomial draws and the means and variances lie within
the derived rounding bound of a np.longdouble evaluation (the worst ratios are printed; profiles/replay_kernel_tests.txt).  Part C
runs what no small shape reaches otherwise (tiles that are chains, the three-waves-per-SIMD builds, the exact-arithmetic
instantiations, a second PCG64 seed), part D the argument guards, part E the engine's routing on a 3,000-cell ingest.

The async kernel knows an unused lane by K < 2 alone (include/memento_hip.h), so the "K = 5, row = -1" lane of tile 4 is K = 0 in
that kernel's tables; the chain kernel takes the active chains only (it needs K >= 2)."""

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from _bins_ref import pair_cells, ref_count, ref_order, ref_table
from _replay_ref import PAD, SENTINEL, chain_operands, full_tiles, layout, menu, ref_moments, ref_weights, routing_problem

pytestmark = pytest.mark.gpu

B = 150
KERNELS = ["replay", "free", "chain", "async"]
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

_REF_W, _REF_M = {}, {}


def _ref_w(name, seed=5):
    """numpy's weights [K][B] of a menu chain (B = 150 replicates; a shorter run draws the first ones of them)."""
    if (name, seed) not in _REF_W:
        w = ref_weights(menu()[name].mult, B, seed)
        w.setflags(write=False)
        _REF_W[name, seed] = w
    return _REF_W[name, seed]


def _ref_m(name, nb, mean_only, seed=5):
    key = (name, nb, mean_only, seed)
    if key not in _REF_M:
        c = menu()[name]
        pk, lq, v, a, b = chain_operands(c.mult, c.v, c.sf)
        _REF_M[key] = ref_moments(v, a, b, _ref_w(name, seed)[:, :nb], c.N, c.q, mean_only=bool(mean_only))
    return _REF_M[key]


class Dev:
    """A layout on the device."""

    def __init__(self, eng, L):
        self.L = L
        d = eng.dev
        self.planes = [d(L.planes[i]) for i in range(5)]
        self.recs = d(L.recs)
        self.tile_ptr = d(L.tile_ptr)
        self.slot = [d(x) for x in (L.slot_K, L.slot_nobs, L.slot_omq, L.slot_row)]
        self.free = [d(x) for x in (L.slot_rec, L.free_K, L.slot_nobs, L.slot_omq, L.free_row)]
        self.asy = [d(x) for x in (L.as_base, L.as_K, L.as_nobs, L.as_omq, L.as_row)]
        one = lambda x, dt: d(x if len(x) else np.zeros(1, dtype=dt))
        self.ch = [one(L.ch_base, np.int64), one(L.ch_K, np.int32), one(L.ch_nobs, np.float64), one(L.ch_omq, np.float64),
                   one(L.ch_row, np.int64)]
        self.tile_chain = d(L.tile_chain)


def _weight_buffer(eng, K_of, kmax, nb, zeroed=True):
    """Device int32 buffer [len(K_of)][kmax][nb] between two guard bands: 0 where k < K (``zeroed``; the pad pattern there too
    without it), the pad pattern everywhere else.  Returns (tensor, pointer to the first weight, the host copy of what was uploaded)."""
    K_of = np.asarray(K_of, dtype=np.int64) * int(zeroed)
    body = np.where(np.arange(kmax)[None, :] < K_of[:, None], 0, PAD).astype(np.uint32)
    body = np.broadcast_to(body[:, :, None], (len(K_of), kmax, nb)).reshape(-1)
    buf = np.concatenate([np.full(GUARD, PAD, dtype=np.uint32), body, np.full(GUARD, PAD, dtype=np.uint32)])
    t = eng.dev(buf)
    return t, ctypes.c_void_p(t.data_ptr() + 4 * GUARD), buf


def _launch(eng, D, kernel, nb, mean_only=0, seed=5, flags=None, co_resident=0, n_tiles=None, chain_stride_pad=2, zeroed=True):
    """One launch of ``kernel`` over the layout ``D`` with sentinel outputs and padded weight buffers.  ``flags``: None = no
    mm_chain_tiles argument; "layout" = the layout's own tile_chain; "none" = a full mm_chain_tiles whose tile_chain is all -1."""
    L = D.L
    P = eng.P
    ld = nb + 1 + 3
    init = np.full((L.n_rows, ld), SENTINEL)
    init[:, 0] = 1000.0 + np.arange(L.n_rows)
    d_m, d_v = eng.dev(init), eng.dev(init)
    n_tiles = L.n_tiles if n_tiles is None else n_tiles
    state, s = eng.pcg64_state(seed), eng._stream()
    jump = eng.pcg64_jump_table(seed)
    res = SimpleNamespace(L=L, nb=nb, ld=ld, kernel=kernel, init=init, flags=flags, kmax_c=L.kmax + chain_stride_pad, w_chain=None, w=None)
    chains, keep = None, []
    if flags is not None:
        assert kernel in ("replay", "free")
        d_tc = D.tile_chain if flags == "layout" else eng.dev(np.full(L.n_tiles, -1, dtype=np.int32))
        t_c, p_c, res.w_chain0 = _weight_buffer(eng, L.ch_K, res.kmax_c, nb, zeroed)
        ct = eng._lib.ChainTiles(P(d_tc), P(D.recs), *map(P, D.ch), P(jump), p_c, res.kmax_c)
        chains = ctypes.byref(ct)
        keep += [d_tc, t_c, ct]
    if kernel == "chain":
        t_w, p_w, res.w0 = _weight_buffer(eng, L.ch_K, L.kmax, nb, zeroed)
        eng._lib.call("mm_boot1d_chain", P(D.recs), *map(P, D.ch), L.n_chains, P(jump), state, nb, mean_only, ld, P(d_m), P(d_v), p_w,
                      L.kmax, s)
    else:
        K_of = {"replay": L.slot_K, "free": L.free_K, "async": L.as_K}[kernel]
        t_w, p_w, res.w0 = _weight_buffer(eng, K_of, L.kmax, nb, zeroed)
        if kernel == "replay":
            eng._lib.call("mm_boot1d_replay", *map(P, D.planes), P(D.tile_ptr), n_tiles, *map(P, D.slot), state, nb, mean_only, ld,
                          P(d_m), P(d_v), p_w, L.kmax, co_resident, chains, s)
        elif kernel == "free":
            eng._lib.call("mm_boot1d_free", P(D.recs), P(D.free[0]), n_tiles, *map(P, D.free[1:]), state, nb, mean_only, ld, P(d_m), P(d_v),
                          p_w, L.kmax, chains, s)
        else:
            eng._lib.call("mm_boot1d_async", P(D.recs), *map(P, D.asy), L.n_slots, state, nb, mean_only, ld, P(d_m), P(d_v), p_w, L.kmax, s)
    res.mean, res.var = eng.host(d_m), eng.host(d_v)                       # (synchronises)
    res.w = eng.host(t_w, np.uint32)
    if flags is not None:
        res.w_chain = eng.host(t_c, np.uint32)
    del keep
    return res


def _runs(e, kernel, flagged=False):
    """Does entry ``e`` of a layout run in a launch of ``kernel``?  (Flagged chains run in launches that take the flags.)"""
    return e.kind == "run" or (e.kind == "flag" and (kernel == "chain" or flagged))


def _weights_of(res, e):
    """[K][nb] weights the launch wrote for entry ``e``."""
    L, nb = res.L, res.nb
    if res.kernel == "chain" or e.kind == "flag":
        buf, stride = (res.w, L.kmax) if res.kernel == "chain" else (res.w_chain, res.kmax_c)
        return buf[GUARD:GUARD + L.n_chains * stride * nb].reshape(L.n_chains, stride, nb)[e.ci, :e.K]
    return res.w[GUARD:GUARD + L.n_slots * L.kmax * nb].reshape(L.n_slots, L.kmax, nb)[e.slot, :e.K]


def _check(res, mean_only=0, seed=5, n_tiles=None):
    """Everything part B asks of one launch.  Returns the worst ratios (mean, variance) to the derived bounds."""
    L, nb, kernel = res.L, res.nb, res.kernel
    flagged = res.flags == "layout"
    ents = [e for e in L.ents if n_tiles is None or e.tile < n_tiles]
    active = [e for e in ents if _runs(e, kernel, flagged)]
    assert len(active) > 0
    written = np.zeros(res.init.shape, dtype=bool)
    # weights: exact, chain by chain; then every weight cell at once (what no chain owns holds what was uploaded)
    want, want_c = res.w0, (res.w_chain0.copy() if res.w_chain is not None else None)      # (res.w0 becomes the expected buffer)
    for e in active:
        w = _ref_w(e.chain.name, seed)[:, :nb]
        got = _weights_of(res, e)
        bad = np.argwhere(got.astype(np.int64) != w)
        assert len(bad) == 0, (f"{kernel}: {e.label}: {len(bad)} weights differ from numpy's, the first at (bin, replicate) = {bad[0].tolist()}: "
                               f"{got[tuple(bad[0])]} instead of {w[tuple(bad[0])]}")
        if kernel == "chain" or e.kind == "flag":
            buf, stride = (want, L.kmax) if kernel == "chain" else (want_c, res.kmax_c)
            buf[GUARD:GUARD + L.n_chains * stride * nb].reshape(L.n_chains, stride, nb)[e.ci, :e.K] = w
        else:
            want[GUARD:GUARD + L.n_slots * L.kmax * nb].reshape(L.n_slots, L.kmax, nb)[e.slot, :e.K] = w
    for got, exp, what in ((res.w, want, "w_dump"), (res.w_chain, want_c, "chains->d_w_dump")):
        if got is not None and not np.array_equal(got, exp):
            at = np.flatnonzero(got != exp)
            raise AssertionError(f"{kernel}: {len(at)} cells of {what} outside k < K of the active chains changed, the first at word "
                                 f"{int(at[0]) - GUARD} (guard band: {GUARD} words): {got[at[0]]:#x} instead of {exp[at[0]]:#x}")
    # moments: inside the derived bound, replicate by replicate
    worst_m = worst_v = 0.0
    for e in active:
        m1, var, b1, bv = _ref_m(e.chain.name, nb, mean_only, seed)
        got_m, got_v = res.mean[e.row, 1:1 + nb], res.var[e.row, 1:1 + nb]
        written[e.row, 1:1 + nb] = True
        assert (_bits(got_m) != SENT_BITS).all() and (_bits(got_v) != SENT_BITS).all(), f"{kernel}: {e.label}: replicates not written"
        L_ = np.longdouble
        for got, ref, bound, what in ((got_m, m1, b1, "mean"), (got_v, var, bv, "variance")):
            err = np.abs(got.astype(L_) - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf)).astype(np.float64)
            r = int(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)))
            assert ratio[r] <= 1.0, (f"{kernel}: {e.label}: replicate {r}: {what} {got[r]!r} is {ratio[r]:.3g} of its bound from "
                                     f"{float(ref[r])!r}")
            if what == "mean":
                worst_m = max(worst_m, float(ratio[r]))
            else:
                worst_v = max(worst_v, float(ratio[r]))
    # K == 1 rows: NaN (not the sentinel) from the tile kernels; untouched by the async kernel (K < 2 = unused) and the chain kernel
    for e in ents:
        if e.kind == "k1" and kernel in ("replay", "free"):
            for plane in (res.mean, res.var):
                x = plane[e.row, 1:1 + nb]
                assert np.isnan(x).all() and (_bits(x) != SENT_BITS).all(), f"{kernel}: {e.label}: a K == 1 row must be NaN"
            written[e.row, 1:1 + nb] = True
    # every other cell -- column 0, the padding columns, unaddressed rows, rows of lanes that must write nothing -- as it was
    for plane, what in ((res.mean, "mean"), (res.var, "variance")):
        bad = np.argwhere(~written & (_bits(plane) != _bits(res.init)))
        if len(bad):
            owner = {e.row: e.label for e in L.ents}
            r, c = bad[0]
            raise AssertionError(f"{kernel}: {len(bad)} {what} cells that must stay untouched changed, the first at row {r} column {c} "
                                 f"({owner.get(int(r), 'a row nothing addresses')}): {plane[r, c]!r}")
    return worst_m, worst_v


@pytest.fixture(scope="module")
def world(eng):
    """The layouts on the device and the launches the tests share: ``run(kernel)`` is the part B launch (B = 150, full layout),
    ``run_small(kernel, mean_only, nb)`` the one on the reduced layout (tiles 1 to 4 without the long600 twin)."""
    import torch

    w = SimpleNamespace(full=Dev(eng, layout(full_tiles())), small=Dev(eng, layout(full_tiles(with_long_twin=False, first=False))), cache={})

    def run(kernel):
        if ("full", kernel) not in w.cache:
            w.cache["full", kernel] = _launch(eng, w.full, kernel, B)
        return w.cache["full", kernel]

    def run_small(kernel, mean_only, nb):
        key = ("small", kernel, mean_only, nb)
        if key not in w.cache:
            w.cache[key] = _launch(eng, w.small, kernel, nb, mean_only=mean_only)
        return w.cache[key]

    w.run, w.run_small = run, run_small
    yield w
    w.cache.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------
# B. each kernel against numpy
# ------------------------------------------------------------------------------------------------------------------------


def test_layout_is_the_designed_one(world):
    L = world.full.L
    assert [sum(1 for e in L.ents if e.tile == t and e.kind == "run") for t in range(5)] == [64, 5, 4, 1, 0]
    assert [e.chain.name for e in L.ents if (e.tile, e.lane) == (1, 63)] == ["long600"]
    assert "btpe12" in [e.chain.name for e in L.ents if e.tile == 1] and len({e.chain.q for e in L.ents if e.chain is not None}) == 2
    assert sorted(e.kind for e in L.ents if e.tile == 4) == ["k0", "k1", "norec", "norow"]
    assert all(e.row != e.slot for e in L.ents) and all(e.row != e.ci for e in L.ents if e.kind == "run")
    assert L.n_rows == len(L.row_used) + 7


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_against_numpy(world, kernel):
    """B = 150 on the full layout: the weights of every active chain and replicate equal numpy's, the means and variances lie
    within ref_moments' bounds, the K == 1 row is NaN (tile kernels) or untouched (async), and every cell outside -- column 0, the
    padding columns, the unaddressed rows, the rows of the lanes that must write nothing, the weight cells outside k < K and the
    guard bands -- holds the bit pattern it was given."""
    res = world.run(kernel)
    worst_m, worst_v = _check(res)
    print(f"\n{kernel}: B = {B}, {len([e for e in res.L.ents if _runs(e, kernel)])} chains: worst ratio to the derived bound: "
          f"mean {worst_m:.3g}, variance {worst_v:.3g}")


@pytest.mark.parametrize("mean_only, nb", [(1, B), (0, 1), (0, 64), (0, 65)], ids=["mean-only", "B1", "B64", "B65"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_mean_only_and_small_num_boot(world, kernel, mean_only, nb):
    """The reduced layout with mean_only (replicates are [mean + 1, 10]) and with 1, 64 and 65 replicates (the chain kernel stores
    replicates in groups of 64: one ragged group, one full one, a full and a ragged one)."""
    res = world.run_small(kernel, mean_only, nb)
    worst_m, worst_v = _check(res, mean_only=mean_only)
    if mean_only:
        for e in res.L.ents:
            if e.kind == "run":
                assert (res.var[e.row, 1:1 + nb] == 10.0).all(), e.label
    print(f"\n{kernel}: mean_only = {mean_only}, B = {nb}: worst ratio to the derived bound: mean {worst_m:.3g}, variance {worst_v:.3g}")


def _same_rows(ra, rb, what):
    """The active chains' rows and weights of two launches over one layout are bit-identical."""
    for e in ra.L.ents:
        if e.kind != "run":
            continue
        for pa, pb, plane in ((ra.mean, rb.mean, "mean"), (ra.var, rb.var, "variance")):
            bad = np.flatnonzero(_bits(pa[e.row]) != _bits(pb[e.row]))
            assert len(bad) == 0, f"{what}: {e.label}: {plane} differs in {len(bad)} columns, the first {bad[0]}: {pa[e.row, bad[0]]!r} / {pb[e.row, bad[0]]!r}"
        assert np.array_equal(_weights_of(ra, e), _weights_of(rb, e)), f"{what}: {e.label}: weights differ"


def test_four_kernels_agree_bit_for_bit(world):
    """Mean and variance planes as int64 views: the two tile kernels' whole planes are identical, the chain and the async kernel's
    too (they leave the K == 1 row alone), and the rows of every active chain are identical across all four; so are the weights."""
    r = {k: world.run(k) for k in KERNELS}
    for a, b in (("replay", "free"), ("chain", "async")):
        assert np.array_equal(_bits(r[a].mean), _bits(r[b].mean)) and np.array_equal(_bits(r[a].var), _bits(r[b].var)), (a, b)
    for k in KERNELS[1:]:
        _same_rows(r["replay"], r[k], f"replay / {k}")


@pytest.mark.parametrize("kernel", KERNELS)
def test_twins_equal_their_originals(world, kernel):
    """Chains with equal operands in different tiles, lanes and company (long600 beside 63 neighbours and beside 4, btpe12 in
    tiles of 64, 5 and 4 lanes, ...) give the same bits."""
    res = world.run(kernel)
    first, twins = {}, 0
    for e in res.L.ents:
        if e.kind != "run":
            continue
        o = first.setdefault(e.chain.name, e)
        if o is e:
            continue
        twins += 1
        for plane, what in ((res.mean, "mean"), (res.var, "variance")):
            assert np.array_equal(_bits(plane[e.row, 1:1 + B]), _bits(plane[o.row, 1:1 + B])), f"{kernel}: {what} of {e.label} != {o.label}"
        assert np.array_equal(_weights_of(res, e), _weights_of(res, o)), f"{kernel}: weights of {e.label} != {o.label}"
    assert twins >= 10


@pytest.mark.parametrize("kernel", KERNELS)
def test_w_dump_behind_the_bin_where_the_cells_ran_out(eng, world, kernel):
    """What include/memento_hip.h says of d_w_dump, on a buffer that is NOT zeroed (pad pattern in every cell): the lock-step and
    the free kernel write every k < K of an active slot -- zeros behind the bin where a replicate's cells ran out --; the chain
    and the async kernel leave those cells alone, which is why their caller zeroes the buffer."""
    res = _launch(eng, world.small, kernel, B, zeroed=False)
    n_behind = 0
    for e in res.L.ents:
        if e.kind != "run":
            continue
        w = _ref_w(e.chain.name)
        out_at = np.argmax(np.cumsum(w, axis=0) >= e.chain.N, axis=0)               # the bin that took a replicate's last cell
        behind = np.arange(e.K)[:, None] > out_at[None, :]
        assert (w[behind] == 0).all()
        n_behind += int(behind.sum())
        got = _weights_of(res, e)
        want = w.astype(np.uint32)
        if kernel in ("chain", "async"):
            want = np.where(behind, np.uint32(PAD), want)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{kernel}: {e.label}: (bin, replicate) = {bad[0].tolist()} holds {got[tuple(bad[0])]:#x}, not {want[tuple(bad[0])]:#x}"
    assert n_behind > 100


# ------------------------------------------------------------------------------------------------------------------------
# C. the variants nothing small reaches
# ------------------------------------------------------------------------------------------------------------------------


def _flagged_tiles():
    t = full_tiles()
    return [t[1], "long600", t[2], t[3], "six_ones", t[4]]


def _same_as_part_b(world, res, kernel, what):
    """Every chain of a launch over another layout against the part B launch of the same kernel: same name, same bits."""
    base = world.run(kernel)
    by_name = {}
    for e in base.L.ents:
        if e.kind == "run":
            by_name.setdefault(e.chain.name, e)
    n = 0
    for e in res.L.ents:
        if not _runs(e, kernel, res.flags == "layout"):
            continue
        o = by_name[e.chain.name]
        for pa, pb, plane in ((res.mean, base.mean, "mean"), (res.var, base.var, "variance")):
            assert np.array_equal(_bits(pa[e.row, 1:1 + B]), _bits(pb[o.row, 1:1 + B])), f"{what}: {plane} of {e.label} differs from part B's"
        assert np.array_equal(_weights_of(res, e), _weights_of(base, o)), f"{what}: weights of {e.label} differ from part B's"
        n += 1
    return n


@pytest.mark.parametrize("kernel", ["replay", "free"])
def test_tiles_that_are_chains(eng, world, kernel):
    """mm_chain_tiles: six tiles, of which tiles 1 (long600) and 4 (six_ones) are chains of the record form without bin rows.  Their
    results go to d_ch_row and their weights to chains->d_w_dump with stride chains->kmax_dump (another stride than the tiles');
    everything is what part B's launch gave, and what numpy gives."""
    D = Dev(eng, layout(_flagged_tiles()))
    L = D.L
    flagged = {e.tile: e for e in L.ents if e.kind == "flag"}
    assert L.tile_chain.tolist() == [-1, flagged[1].ci, -1, -1, flagged[4].ci, -1] and min(flagged[1].ci, flagged[4].ci) > 0
    assert (flagged[1].chain.name, flagged[4].chain.name) == ("long600", "six_ones")
    assert L.tile_ptr[2] == L.tile_ptr[1] and L.tile_ptr[5] == L.tile_ptr[4]
    res = _launch(eng, D, kernel, B, flags="layout")
    assert res.kmax_c != L.kmax
    _check(res)
    assert _same_as_part_b(world, res, kernel, f"{kernel} with flagged tiles") == 5 + 4 + 1 + 2


@pytest.mark.parametrize("kernel", ["replay", "free"])
def test_no_flagged_tile_is_no_chains_argument(eng, world, kernel):
    """tile_chain[t] = -1 for every tile behaves exactly as chains = NULL: same planes, same weights, chains->d_w_dump untouched."""
    base = world.run_small(kernel, 0, 65)
    res = _launch(eng, world.small, kernel, 65, flags="none")
    _check(res)
    assert np.array_equal(_bits(res.mean), _bits(base.mean)) and np.array_equal(_bits(res.var), _bits(base.var))
    assert np.array_equal(res.w, base.w) and np.array_equal(res.w_chain, res.w_chain0)


def test_replay_three_waves_per_simd_build(eng, world):
    """co_resident_waves = 2047 with 5 tiles: n_tiles + co_resident_waves > 2048, the launch takes k_boot1d_replay<3, .> on tiny
    work.  Bit-identical to the two-wave build."""
    base = world.run("replay")
    res = _launch(eng, world.full, "replay", B, co_resident=2047)
    _check(res)
    assert np.array_equal(_bits(res.mean), _bits(base.mean)) and np.array_equal(_bits(res.var), _bits(base.var))
    assert np.array_equal(res.w, base.w)


def test_free_three_waves_per_simd_build(eng):
    """2,049 tiles of one K = 3 chain each (the lane moves with the tile), B = 4: k_boot1d_free<3, .>.  The same tables launched
    with n_tiles = 2,048 take the two-wave build: the rows of those tiles are bit-identical, and tile 2,048's row equals them."""
    nb = 4
    D = Dev(eng, layout([{(t * 29) % 64: ("run", "k3_flip")} for t in range(2049)]))
    r3 = _launch(eng, D, "free", nb)
    _check(r3)
    r2 = _launch(eng, D, "free", nb, n_tiles=2048)
    _check(r2, n_tiles=2048)
    last = D.L.ents[-1]
    assert last.tile == 2048 and (_bits(r2.mean[last.row]) == _bits(r2.init[last.row])).all()
    for e in D.L.ents[:-1]:
        assert np.array_equal(_bits(r3.mean[e.row]), _bits(r2.mean[e.row])) and np.array_equal(_bits(r3.var[e.row]), _bits(r2.var[e.row])), e.label
    first = D.L.ents[0]
    assert np.array_equal(_bits(r3.mean[last.row, 1:]), _bits(r3.mean[first.row, 1:])) and np.array_equal(_bits(r3.var[last.row, 1:]), _bits(r3.var[first.row, 1:]))
    assert np.array_equal(_weights_of(r3, last), _weights_of(r2, first))


@pytest.fixture
def exact_arith(eng):
    """Switches mm_debug_replay_arith(1) on when called.  The switch is process-wide: the finalizer takes it back whatever the
    test does, so a failing assertion cannot leak it into later tests."""
    yield lambda: eng._lib.call("mm_debug_replay_arith", 1)
    eng._lib.call("mm_debug_replay_arith", 0)


@pytest.mark.parametrize("kernel", KERNELS + ["replay-flagged", "free-flagged"])
def test_exact_arithmetic_instantiations(eng, world, exact_arith, kernel):
    """The FAST = false instantiations of the four kernels and of the flagged-tile launch: weights and moments identical to the
    default arithmetic's (part B), and numpy's."""
    flagged = kernel.endswith("-flagged")
    kernel = kernel.split("-")[0]
    base = world.run(kernel)                           # the default arithmetic: launched (or cached) before the switch goes on
    exact_arith()
    if flagged:
        res = _launch(eng, Dev(eng, layout(_flagged_tiles())), kernel, B, flags="layout")
        _check(res)
        assert _same_as_part_b(world, res, kernel, f"exact arithmetic, {kernel} with flagged tiles") == 12
        return
    res = _launch(eng, world.full, kernel, B)
    _check(res)
    assert np.array_equal(_bits(res.mean), _bits(base.mean)) and np.array_equal(_bits(res.var), _bits(base.var))
    assert np.array_equal(res.w, base.w)


@pytest.mark.parametrize("kernel", KERNELS)
def test_second_seed(eng, world, kernel):
    """pcg_state of PCG64(12345) and its jump table on the reduced layout, B = 65: numpy's multinomial with that seed in all four
    kernels (a hard-coded increment or jump table would fail here), and other draws than seed 5's."""
    res = _launch(eng, world.small, kernel, 65, seed=12345)
    _check(res, seed=12345)
    assert any((_ref_w(e.chain.name, 12345) != _ref_w(e.chain.name)).any() for e in res.L.ents if e.kind == "run")


# ------------------------------------------------------------------------------------------------------------------------
# D. guards: every call here returns before any launch
# ------------------------------------------------------------------------------------------------------------------------


def _guard_args(eng, D, kernel, outs, nb=8, ld=None, null_first=False, n=None, chains=None):
    """Argument list of ``kernel`` over layout ``D`` with the given outputs (mean, var, weights)."""
    P = eng.P
    L = D.L
    ld = nb + 4 if ld is None else ld
    state, s = eng.pcg64_state(5), eng._stream()
    null = ctypes.c_void_p(0)
    first = lambda p: null if null_first else p
    tail = [state, nb, 0, ld, P(outs[0]), P(outs[1]), P(outs[2]), L.kmax]
    if kernel == "replay":
        pl = [P(x) for x in D.planes]
        return [first(pl[0]), *pl[1:], P(D.tile_ptr), L.n_tiles if n is None else n, *map(P, D.slot), *tail, 0, chains, s]
    if kernel == "free":
        return [first(P(D.recs)), P(D.free[0]), L.n_tiles if n is None else n, *map(P, D.free[1:]), *tail, chains, s]
    if kernel == "chain":
        return [first(P(D.recs)), *map(P, D.ch), L.n_chains if n is None else n, P(eng.pcg64_jump_table(5)), *tail, s]
    return [first(P(D.recs)), *map(P, D.asy), L.n_slots if n is None else n, *tail, s]


@pytest.mark.parametrize("kernel", KERNELS)
def test_guards(eng, world, kernel):
    """A NULL operand, num_boot = 0, ld = num_boot and (tile kernels) a mm_chain_tiles with one NULL member give a negative status
    and a text in mm_last_error; n_tiles / n_chains / n_slots = 0 returns 0.  None of them writes a cell."""
    D = world.small
    L = D.L
    lib = eng._lib.load()
    nb = 8
    init = np.full((L.n_rows, nb + 4), SENTINEL)
    outs = [eng.dev(init), eng.dev(init), eng.dev(np.full(L.n_slots * L.kmax * nb, PAD, dtype=np.uint32))]
    fn = getattr(lib, f"mm_boot1d_{kernel}")
    cases = {"a NULL operand": dict(null_first=True), "num_boot = 0": dict(nb=0, ld=12), "ld = num_boot": dict(nb=nb, ld=nb)}
    keep = []
    if kernel in ("replay", "free"):
        members = [eng.P(D.tile_chain), eng.P(D.recs), *map(eng.P, D.ch), eng.P(eng.pcg64_jump_table(5))]
        for i in (0, 4, 7):
            m = list(members)
            m[i] = ctypes.c_void_p(0)
            ct = eng._lib.ChainTiles(*m, ctypes.c_void_p(0), 0)
            keep.append(ct)
            cases[f"mm_chain_tiles member {i} NULL"] = dict(chains=ctypes.byref(ct))
    for what, kw in cases.items():
        rc = fn(*_guard_args(eng, D, kernel, outs, **{"nb": nb, **kw}))
        assert rc < 0, f"{kernel}: {what}: status {rc}"
        assert len(lib.mm_last_error()) > 0 and b"bad argument" in lib.mm_last_error(), what
    assert fn(*_guard_args(eng, D, kernel, outs, nb=nb, n=0)) == 0
    eng._torch().cuda.synchronize()
    assert (_bits(eng.host(outs[0])) == SENT_BITS).all() and (_bits(eng.host(outs[1])) == SENT_BITS).all()
    assert (eng.host(outs[2], np.uint32) == PAD).all()


# ------------------------------------------------------------------------------------------------------------------------
# E. the engine's routing at small size
# ------------------------------------------------------------------------------------------------------------------------

B_E = 70
ROUTES = ["default", "lone-chains", "tiles-only", "free-tiles", "async"]


@pytest.fixture(scope="module")
def routed(eng):
    """One ingest of routing_problem, one Bootstrap1D, numpy's weights of every pair; ``run(route)`` caches what each configuration
    left behind."""
    import torch

    prob = routing_problem()
    blocks = eng.CountBlocks(eng.DeviceCSR(sp.csr_matrix(prob.X.astype(np.float32))), prob.gid, prob.ng)
    S, sumx, maxx = blocks.moments(1.0 / prob.sf_table[prob.sf_bin])
    bs = eng.Bootstrap1D(blocks, np.arange(prob.n_genes), maxx, prob.sf_bin, prob.sf_table, prob.grp_q, B_E)
    want = []
    for p in range(bs.n_pairs):
        x, sbin = pair_cells(prob, p)
        t = ref_table(x, sbin, prob.n_bins, int(x.max()) + 1)
        K = ref_count(t)
        mult = ref_order(t, prob.sf_table, prob.r1[p], prob.r0[p], len(x))[2]
        want.append((K, ref_weights(mult, B_E) if K >= 2 else None))
    st = SimpleNamespace(prob=prob, bs=bs, want=want, runs={})

    def run(route):
        if route in st.runs:
            return st.runs[route]
        mp = pytest.MonkeyPatch()
        seen = []
        choose = bs._choose_kernels
        try:
            for name, value in (("TILE_MODE", "lockstep"), ("TILE_FREE", False), ("CHAIN_MIN_K", 0), ("CHAIN_LONE", True), ("CHAIN_ALL_MAX", 8192)):
                mp.setattr(eng, name, value)
            target = None
            if route != "default":
                mp.setattr(eng, "CHAIN_ALL_MAX", 0)
                target = 10
            if route == "tiles-only":
                mp.setattr(eng, "CHAIN_LONE", False)
            if route == "free-tiles":
                mp.setattr(eng, "TILE_FREE", True)
            if route == "async":
                target = None
                mp.setattr(eng, "TILE_MODE", "async")
                mp.setattr(eng, "ASYNC_CHAIN_MIN_K", int(np.median(bs.K[bs.K >= 2])))
                mp.setattr(eng, "ASYNC_LANES", 7)
            mp.setattr(bs, "_choose_kernels", lambda *a: seen.append(choose(*a)) or seen[-1])
            zeros = np.zeros(bs.n_pairs)
            bs.alloc_outputs(zeros, zeros)
            bs.run(np.zeros(bs.n_pairs, dtype=bool), prob.r1, prob.r0, [0.0, 1.0, 0.0], fill_mode=1, dump_weights=True, target_waves=target)
        finally:
            mp.undo()
        c = seen[0]
        lanes = np.bincount(c.slot_of // 64, minlength=c.n_tiles) if c.n_tiles else np.zeros(0, dtype=np.int64)
        out = SimpleNamespace(c=c, lanes=lanes, n_tiles=bs.n_tiles, n_chain=bs.n_chain, n_async=bs.n_async, n_chain_launch=bs.n_chain_launch,
                              use_free=c.use_free, raw_mean=eng.host(bs.raw_mean).copy(), raw_var=eng.host(bs.raw_var).copy(),
                              weights=[bs.weights_of(p).copy() if bs.active[p] else None for p in range(bs.n_pairs)], active=bs.active.copy())
        st.runs[route] = out
        return out

    st.run = run
    yield st
    st.runs.clear()
    for name in ("tab", "_opsbuf", "_ops", "w_dump", "w_dump_chain", "w_dump_async", "raw_mean", "raw_var"):
        if hasattr(bs, name):
            setattr(bs, name, None)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("route", ROUTES)
def test_engine_routing(routed, route):
    """Bootstrap1D._choose_kernels / _lay_out_operands / _launch / weights_of on 120 chains of 1 to ~600 bins: each configuration
    routes the chains as designed, weights_of(p) is numpy's multinomial for every active pair, and raw_mean / raw_var are
    bit-identical to the default configuration's."""
    bs, want = routed.bs, routed.want
    assert [int(k) for k in bs.K] == [k for k, _ in want]
    K_act = bs.K[bs.K >= 2]
    assert K_act.min() == 2 and K_act.max() > 300 and (bs.K < 2).any()
    run = routed.run(route)
    n_act = int(run.active.sum())
    assert n_act == len(K_act)
    if route == "default":                                   # every chain a wave of its own
        assert (run.n_chain, run.n_chain_launch, run.n_tiles, run.n_async) == (n_act, n_act, 0, 0)
    elif route == "async":
        assert run.n_async > 0 and run.n_chain_launch > 0 and run.n_tiles == 0 and run.n_async + run.n_chain_launch == n_act
    else:
        shared = run.lanes[run.lanes > 0]
        assert run.n_chain_launch == 0 and run.n_async == 0 and run.use_free == (route == "free-tiles")
        if route == "tiles-only":
            assert run.c.tile_chain is None and run.n_chain == 0 and (run.lanes == 1).any() and (run.lanes >= 2).any()
        else:
            assert (run.c.tile_chain >= 0).sum() == run.n_chain > 0                       # lone tiles run as chains ...
            assert len(shared) > 0 and shared.min() >= 2 and run.n_chain + int(shared.sum()) == n_act      # ... beside shared tiles
    for p, (K, w) in enumerate(want):
        if run.active[p]:
            np.testing.assert_array_equal(run.weights[p], w, err_msg=f"{route}: pair {p} (K = {K})")
    base = routed.run("default")
    assert np.isfinite(base.raw_mean[base.active, 1:]).all()
    np.testing.assert_array_equal(_bits(run.raw_mean), _bits(base.raw_mean), err_msg=route)
    np.testing.assert_array_equal(_bits(run.raw_var), _bits(base.raw_var), err_msg=route)
