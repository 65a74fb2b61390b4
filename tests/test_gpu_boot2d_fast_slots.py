"""GPU tests of mm_boot2d_fast_slots (Bootstrap2D.launch_listed): the 2D rng='fast' kernel on a replicate range, launched over a
LIST of slots instead of the chunk's whole tile layout.  A listed chain gets bit for bit the columns that the range launch
(mm_boot2d_fast_range, tests/test_gpu_boot2d_fast_range.py) gives it, and nothing else is written: not column 0, not the columns
behind rep_n, not the row of a chain that is not listed.

The problem is that of test_gpu_boot2d_fast_range (groups of 700 / 70 / 6 cells, 12 genes, a heavy size-factor bin, a highly
expressed gene, a never-expressed one, one expressed in one group only, one chain the caller skips) with ALL 66 pairs of the 12
genes and a self pair: 201 chains in four 64-slot tiles, the last one with unused slots (K <= 0).  The reference is one
run(fast=True, keep_fast=True) over 465 replicates, computed once; every launch under test reads what that run kept.
"""

from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

N_SF_BINS = 30
N_GENES = 12
HIGH, NEVER, ONE_GROUP = 4, 2, 8
SIZES = (700, 70, 6)
PAIRS = [(a, b) for a in range(N_GENES) for b in range(a + 1, N_GENES)] + [(5, 5)]
SKIPPED = 2 * len(SIZES) + 1
B_REF = 465
SEED = 3
REP_LO = (0, 200)
REP_N = (1, 63, 64, 65, 200)
PAD = 3                                  # columns behind the rep_n replicate columns
EXTRA_ROWS = 5                           # rows of the plane that no chain owns
SENTINEL = np.int64(0x7FF8_5EED_0BAD_CAFE)     # a NaN payload no kernel produces


def _problem(seed=77):
    rng = np.random.default_rng(seed)
    ng = len(SIZES)
    gid = np.concatenate([np.full(s, g, dtype=np.int32) for g, s in enumerate(SIZES)] + [np.full(40, -1, dtype=np.int32)])
    rng.shuffle(gid)
    n = len(gid)
    X = rng.poisson(rng.uniform(0.05, 0.9, size=N_GENES) * rng.gamma(2.0, 0.5, size=(n, N_GENES))).astype(np.int64)
    X[:, HIGH] = rng.poisson(rng.gamma(3.0, 2.5, size=n))
    X[:, NEVER] = 0
    X[gid != 0, ONE_GROUP] = 0
    sf = rng.lognormal(0.0, 0.3, size=n)
    sf_bin = rng.integers(0, N_SF_BINS, size=n).astype(np.uint8)
    sf_bin[rng.random(n) < 1 / 3] = 7
    sf_bin[gid == ng - 1] = 4
    return SimpleNamespace(csr=sp.csr_matrix(X.astype(np.float32)), gid=gid, ng=ng, sf=sf, sf_bin=sf_bin,
                           sf_table=np.linspace(0.4, 2.5, N_SF_BINS), grp_q=np.full(ng, 0.07))


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


@pytest.fixture(scope="module")
def ref(eng):
    """The one-shot reference launch, computed once and left unchanged."""
    prob = _problem()
    blocks = eng.CountBlocks(eng.DeviceCSR(prob.csr), prob.gid, prob.ng)
    _, _, maxx = blocks.moments(1.0 / prob.sf)
    cols = eng.GeneColumns(blocks, np.arange(N_GENES))
    p = np.array(PAIRS, dtype=np.int64)
    bs = eng.Bootstrap2D(cols, p[:, 0], p[:, 1], maxx, prob.sf_bin, prob.sf_table, prob.grp_q, B_REF)
    col0 = 1000.0 + np.arange(bs.n_q)
    u = np.random.default_rng(79).random((3, bs.n_q))
    skip = np.zeros(bs.n_q, dtype=bool)
    skip[SKIPPED] = True
    keys = 5000 + 3 * np.arange(bs.n_q, dtype=np.int64)              # stream keys that are not the rows
    bs.run(skip, u[0], u[1], u[2], col0, fast=True, fast_seed=SEED, pair_key=keys, keep_fast=True)
    active = ~skip & (bs.K >= 1)
    np.testing.assert_array_equal(bs.active, active)
    return SimpleNamespace(bs=bs, active=active, raw=eng.host(bs.yc).copy(), slot=bs.pair_slot.copy())


def _sentinel_plane(eng, n_rows, ld):
    torch = eng._torch()
    return torch.full((n_rows, ld), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)


def _bits(eng, plane):
    return eng.host(plane.view(eng._torch().int64))


def _want(ref, n_rows, ld, rep_lo, rep_n, chains, rows):
    """The sentinel plane with the reference's columns [rep_lo, rep_lo + rep_n) of the chains that ran in the given rows."""
    want = np.full((n_rows, ld), SENTINEL, dtype=np.int64)
    ran = ref.active[chains]
    want[rows[ran], 1:1 + rep_n] = np.ascontiguousarray(ref.raw[chains[ran], 1 + rep_lo:1 + rep_lo + rep_n]).view(np.int64)
    return want


def _lists(ref):
    """The lists of chains a launch is given, by name: one slot; every chain (the skipped one among them); slots in the middle of
    a tile; slots spanning three tiles; two chains in three; none."""
    q = np.arange(ref.bs.n_q)
    slot = ref.slot
    return {"one": q[slot == 77], "all": q, "mid_tile": q[(slot >= 70) & (slot < 90)], "three_tiles": q[(slot >= 50) & (slot < 140)],
            "two_thirds": q[q % 3 != (q // 3) % 3], "none": q[:0]}


def test_the_problem_has_the_layout_it_promises(eng, ref):
    bs = ref.bs
    assert bs.n_q == len(PAIRS) * len(SIZES) == 201 and bs.n_tiles == 4 and bs._fast.n_slots == 256
    assert bs.replay_kernel == "mm_boot2d_fast" and ref.active.sum() == bs.n_q - 1 and ref.slot[SKIPPED] < 0
    assert sorted(ref.slot[ref.active]) == list(range(200))          # dense: slots 200..255 of the last tile are unused
    assert (eng.host(bs._fast.d_slot_K)[200:] <= 0).all() and (bs.K[ref.active] == 1).any()
    assert np.isfinite(ref.raw[ref.active, 1:]).all() and np.isnan(ref.raw[SKIPPED, 1:]).all()
    lists = _lists(ref)
    assert len(lists["one"]) == 1 and len(lists["mid_tile"]) == 20 and len(lists["three_tiles"]) == 90 and SKIPPED in lists["two_thirds"]


@pytest.mark.parametrize("rep_n", REP_N)
@pytest.mark.parametrize("rep_lo", REP_LO)
def test_a_listed_launch_is_the_range_launchs_columns_and_nothing_else_is_written(eng, ref, rep_lo, rep_n):
    """Every list, with compact rows (row i for the i-th listed chain) and with rows in the pair-granular positions (row q), on
    a sentinel plane with PAD columns behind the replicates and EXTRA_ROWS rows that no chain owns."""
    bs = ref.bs
    ld = 1 + rep_n + PAD
    for name, chains in _lists(ref).items():
        for rows, n_rows in ((np.arange(len(chains)), len(chains) + EXTRA_ROWS), (chains, bs.n_q + EXTRA_ROWS)):
            plane = _sentinel_plane(eng, n_rows, ld)
            keep = bs.launch_listed(rep_lo, rep_n, chains, plane, rows)
            got = _bits(eng, plane)
            del keep
            np.testing.assert_array_equal(got, _want(ref, n_rows, ld, rep_lo, rep_n, chains, rows), err_msg=f"{name}, {n_rows} rows")


@pytest.mark.parametrize("rep_lo,rep_n", [(0, 65), (200, 200)])
def test_a_list_of_every_slot_is_the_range_launch_on_the_whole_plane(eng, ref, rep_lo, rep_n):
    bs = ref.bs
    q = np.arange(bs.n_q)
    rows = bs.n_q - 1 - q                                              # rows that are not the chains' own
    planes = []
    for launch in (bs.launch_range, bs.launch_listed):
        plane = _sentinel_plane(eng, bs.n_q, 1 + rep_n + PAD)
        keep = launch(rep_lo, rep_n, q, plane, rows)
        planes.append(_bits(eng, plane))
        del keep
    np.testing.assert_array_equal(planes[1], planes[0])
    assert (planes[0][rows[ref.active], 1:1 + rep_n] != SENTINEL).all() and (planes[0][rows[SKIPPED]] == SENTINEL).all()


def test_a_chain_given_twice_and_an_unsorted_list(eng, ref):
    """The engine's list is ascending and unique whatever the order of ``open_q``; a chain given twice takes its last row, as in
    the range launch."""
    bs = ref.bs
    chains = np.array([150, 3, 77, 3, 40])
    rows = np.array([0, 1, 2, 3, 4])
    planes = []
    for launch in (bs.launch_range, bs.launch_listed):
        plane = _sentinel_plane(eng, 5, 1 + 70)
        keep = launch(37, 70, chains, plane, rows)
        planes.append(_bits(eng, plane))
        if launch == bs.launch_listed:
            assert eng.host(keep[0]).tolist() == sorted({int(s) for s in ref.slot[chains]})
        del keep
    np.testing.assert_array_equal(planes[1], planes[0])
    assert (planes[1][1] == SENTINEL).all() and (planes[1][3, 1:] != SENTINEL).all()


def _entry(eng, ref, plane, d_slot_row, d_list, n_list, rep_lo=0, rep_n=8, ld=None, n_slots=None):
    f = ref.bs._fast
    P = eng.P
    return eng._lib.call("mm_boot2d_fast_slots", *map(P, f.ops), P(f.d_tile_ptr), f.n_slots if n_slots is None else n_slots, P(f.d_slot_K),
                         P(f.d_nobs), P(f.d_omq), P(d_slot_row), P(f.d_slot_key), f.seed, rep_lo, rep_n, plane.shape[1] if ld is None else ld,
                         P(plane), P(d_list), n_list, eng._stream())


def test_unused_slots_closed_rows_and_a_slot_listed_twice(eng, ref):
    """The entry point itself, on a slot-row table of its own: a listed slot with K <= 0 (the unused slots of the last tile,
    with valid rows) writes nothing, a listed slot with row -1 writes nothing, a slot with a row that is NOT listed writes
    nothing, and a slot listed twice is written with the same values."""
    bs = ref.bs
    rep_lo, rep_n = 200, 65
    q_of_slot = np.full(256, -1)
    q_of_slot[ref.slot[ref.active]] = np.flatnonzero(ref.active)
    slot_row = np.arange(256, dtype=np.int64)                         # every slot has a row of its own ...
    slot_row[[10, 130]] = -1                                          # ... but two closed ones
    listed = np.array([5, 10, 64, 64, 130, 199, 200, 230, 255], dtype=np.int64)
    plane = _sentinel_plane(eng, 256, 1 + rep_n + PAD)
    d_rows, d_list = eng.dev(slot_row), eng.dev(listed)
    _entry(eng, ref, plane, d_rows, d_list, len(listed), rep_lo, rep_n)
    got = _bits(eng, plane)
    want = np.full(got.shape, SENTINEL, dtype=np.int64)
    for s in (5, 64, 199):
        want[s, 1:1 + rep_n] = ref.raw[q_of_slot[s], 1 + rep_lo:1 + rep_lo + rep_n].view(np.int64)
    np.testing.assert_array_equal(got, want)
    # the empty list: no launch, with or without a list pointer
    plane = _sentinel_plane(eng, 4, 9)
    assert _entry(eng, ref, plane, d_rows, None, 0) == 0 and _entry(eng, ref, plane, d_rows, d_list, 0) == 0
    assert (_bits(eng, plane) == SENTINEL).all()


def test_the_entry_point_checks_its_arguments(eng, ref):
    plane = _sentinel_plane(eng, 256, 9)
    d_rows, d_list = eng.dev(np.arange(256, dtype=np.int64)), eng.dev(np.array([3, 4], dtype=np.int64))
    for bad in (dict(n_list=-1), dict(d_list=None), dict(rep_n=0), dict(rep_lo=-1), dict(rep_lo=2 ** 31 - 5), dict(ld=8), dict(n_slots=-64),
                dict(n_slots=100), dict(d_slot_row=None), dict(plane=None)):
        kw = dict(plane=plane, d_slot_row=d_rows, d_list=d_list, n_list=2, ld=9)
        kw.update(bad)
        with pytest.raises(eng._lib.MementoHipError, match="mm_boot2d_fast_slots failed"):
            _entry(eng, ref, **kw)
    assert (_bits(eng, plane) == SENTINEL).all()
    assert _entry(eng, ref, plane, d_rows, d_list, 2) == 0             # (the unchanged arguments go through)
    assert (_bits(eng, plane)[3:5, 1:] != SENTINEL).all()


def test_launch_listed_checks_its_arguments(eng, ref):
    torch = eng._torch()
    bs = ref.bs
    plane = torch.zeros((bs.n_q, 9), dtype=torch.float64, device="cuda")
    q4 = np.arange(4)
    for bad in (dict(open_q=np.array([0, 1, 2, bs.n_q])), dict(open_q=np.array([0, 1, 2, -1])), dict(row_of_q=np.array([0, 1, 2, bs.n_q])),
                dict(row_of_q=np.array([0, 1, 2, -1])), dict(row_of_q=np.arange(3)), dict(dump_weights=True), dict(rep_lo=-1), dict(rep_n=0),
                dict(rep_n=9), dict(rep_lo=2 ** 31 - 5), dict(plane=plane.to(torch.float32)), dict(plane=None)):
        kw = dict(rep_lo=0, rep_n=8, open_q=q4, plane=plane, row_of_q=q4)
        kw.update(bad)
        with pytest.raises(ValueError):
            bs.launch_listed(**kw)
    assert float(plane.abs().sum().item()) == 0.0
