"""GPU tests of mm_boot1d_fast_range (Bootstrap1D.launch_range): the rng='fast' kernel on a replicate range.  Replicate
rep_lo + i of a chain, made by a later launch for some of the chains, is bit for bit column 1 + rep_lo + i of a one-shot launch
over more replicates, and the launch writes nothing else: not column 0, not the columns behind rep_n, not a closed chain's row,
not a K == 1 row.

One small problem (in the style of test_gpu_boot1d_fast): groups of 700 / 70 / 6 cells plus ungrouped cells, 12 genes, 30
size-factor bins -- a third of the cells in one of them, so that the sparse genes of the 700-cell group have bins of some hundred
cells (numpy's BTPE sampler, n min(p, 1 - p) > 30) -- the 6-cell group in one size-factor bin (chains with K == 1 where its
cells share a count), one highly expressed gene (chains of some hundred bins), one never-expressed gene and one chain the
caller skips.
"""

import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_SF_BINS = 30
N_GENES = 12
HIGH, NEVER = 4, 2
SIZES = (700, 70, 6)
SKIPPED = 9 * len(SIZES) + 1            # the chain (gene 9, group 1)
B_REF = 4200
SEED = 3
RANGES = [(0, 1), (1, 63), (37, 70), (64, 64), (128, 2), (4133, 65), (0, 4200)]
PAD = 3                                  # columns behind the rep_n replicate columns
EXTRA_ROWS = 5                           # rows of the range planes that no chain owns
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
    sf = rng.lognormal(0.0, 0.3, size=n)
    sf_bin = rng.integers(0, N_SF_BINS, size=n).astype(np.uint8)
    sf_bin[rng.random(n) < 1 / 3] = 7                         # a heavy bin: bins of some hundred cells in the 700-cell group
    sf_bin[gid == ng - 1] = 4                                 # the 6-cell group sits in one size-factor bin: chains with K == 1
    return SimpleNamespace(csr=sp.csr_matrix(X.astype(np.float32)), gid=gid, ng=ng, sf=sf, sf_bin=sf_bin,
                           sf_table=np.linspace(0.4, 2.5, N_SF_BINS), grp_q=np.full(ng, 0.07))


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


@pytest.fixture(scope="module")
def ref(eng):
    """The one-shot reference launch, computed once and left unchanged: run(fast=True) with B_REF replicates, its raw (pre-fill)
    planes and dumped weights on the host."""
    prob = _problem()
    blocks = eng.CountBlocks(eng.DeviceCSR(prob.csr), prob.gid, prob.ng)
    _, _, maxx = blocks.moments(1.0 / prob.sf)
    bs = eng.Bootstrap1D(blocks, np.arange(N_GENES), maxx, prob.sf_bin, prob.sf_table, prob.grp_q, B_REF)
    col0 = 1000.0 + np.arange(bs.n_pairs)
    bs.alloc_outputs(col0, -col0)
    u = np.random.default_rng(79).random((2, bs.n_pairs))
    skip = np.zeros(bs.n_pairs, dtype=bool)
    skip[SKIPPED] = True
    keys = 5000 + 3 * np.arange(bs.n_pairs, dtype=np.int64)           # stream keys that are not the rows
    bs.run(skip, u[0], u[1], (0.0, 1.0, 0.0), fill_mode=1, fill_seed=SEED, fast=True, dump_weights=True, chain_keys=keys)
    active = ~skip & (bs.K >= 2)
    np.testing.assert_array_equal(bs.active, active)
    return SimpleNamespace(prob=prob, bs=bs, u=u, active=active, raw_mean=eng.host(bs.raw_mean), raw_var=eng.host(bs.raw_var))


def test_the_problem_has_the_chains_it_promises(eng, ref):
    """K == 1 chains, the skipped chain, a chain of some hundred bins, and -- from the reference launch's own weights -- draws of the
    700-cell chains on both sides of numpy's inversion / BTPE switch."""
    bs, prob, ng = ref.bs, ref.prob, ref.prob.ng
    assert bs.n_pairs == N_GENES * ng and bs.K[NEVER * ng + ng - 1] == 1 and (bs.K[ng - 1::ng] == 1).sum() >= 2
    assert not ref.active[SKIPPED] and bs.K[SKIPPED] >= 2 and (bs.K[np.arange(bs.n_pairs) % ng < ng - 1] >= 2).all()
    assert bs.K[HIGH * ng] >= 200 and bs.K[NEVER * ng] == N_SF_BINS
    assert ref.active.sum() == (bs.K >= 2).sum() - 1
    assert np.isfinite(ref.raw_mean[ref.active, 1:]).all() and np.isfinite(ref.raw_var[ref.active, 1:]).all()
    n_inv = n_btpe = 0
    for p in range(0, bs.n_pairs, ng):                      # the 700-cell chains
        bi, xi, mu = bs.bins_of_pair(p)
        o, pk, _ = eng._replay_order(xi.astype(np.float64) * ref.u[0][p] + ref.u[1][p] * prob.sf_table[bi], mu, SIZES[0])
        w = bs.weights_of(p)[:, :256]
        assert w.shape == (int(bs.K[p]), 256) and (w.sum(axis=0) == SIZES[0]).all()
        remaining = SIZES[0] - (np.cumsum(w, axis=0) - w)[:-1]
        npq = remaining * np.minimum(pk[:-1], 1.0 - pk[:-1])[:, None]
        n_inv += int(((remaining > 0) & (npq <= 30)).sum())
        n_btpe += int(((remaining > 0) & (npq > 30)).sum())
    assert n_inv > 1000 and n_btpe > 1000


@pytest.mark.parametrize("rep_lo,rep_n", RANGES)
def test_a_range_is_the_one_shot_launchs_columns_and_nothing_else_is_written(eng, ref, rep_lo, rep_n):
    torch = eng._torch()
    bs = ref.bs
    n_rows, ld = bs.n_pairs + EXTRA_ROWS, 1 + rep_n + PAD
    pairs = np.arange(bs.n_pairs)
    closed = pairs % 3 == (pairs // 3) % 3                           # a third of the chains stay closed: group (gene % 3) of every gene
    assert closed.sum() * 3 == bs.n_pairs and not closed[SKIPPED] and (closed & ref.active).sum() >= 6 and (~closed & (bs.K == 1)).any()
    open_pairs = np.flatnonzero(~closed)                             # (K == 1 chains and the skipped one among them)
    row_of_pair = n_rows - 1 - open_pairs                            # rows that are not the chains' own
    planes = [torch.full((n_rows, ld), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64) for _ in range(2)]
    dump = (rep_lo, rep_n) == (37, 70)
    keep = bs.launch_range(rep_lo, rep_n, open_pairs, planes, row_of_pair, dump_weights=dump)
    got = [eng.host(p.view(torch.int64)) for p in planes]
    del keep
    written = ~closed & ref.active
    assert written.sum() >= 12
    for g, raw in zip(got, (ref.raw_mean, ref.raw_var)):
        want = np.full((n_rows, ld), SENTINEL, dtype=np.int64)
        want[row_of_pair[written[open_pairs]], 1:1 + rep_n] = raw[written, 1 + rep_lo:1 + rep_lo + rep_n].view(np.int64)
        np.testing.assert_array_equal(g, want)
    if dump:
        for p in np.flatnonzero(written):
            K, slot = int(bs.K[p]), int(bs.tile_slot[p])
            np.testing.assert_array_equal(eng.host(bs.w_dump_range[slot, :K, :]), bs.weights_of(p)[:, rep_lo:rep_lo + rep_n])
        closed_slots = eng.dev(bs.tile_slot[np.flatnonzero(closed & ref.active)])
        assert int(bs.w_dump_range[closed_slots].abs().sum().item()) == 0        # closed chains dump nothing


def test_a_launch_of_more_than_2_32_threads_runs_all_of_them(eng, ref):
    """The 64 slots of the problem's one tile x (2^20 + 3) chunks of 64 replicates are 2^32 + 12288 threads, more than one grid
    dimension holds: a launch that put them all into gridDim.x ran only part of its blocks and left the other replicates
    unwritten.  Open: the two shortest active chains (the highest slots: a few bins, so that 2^26 replicates of them cost
    nothing); every replicate column of their rows must be written, and the first B_REF of them are the reference launch's."""
    torch = eng._torch()
    bs = ref.bs
    rep_n = (1 << 26) + 3 * 64 - 17
    assert bs.n_tiles == 1 and 64 * ((rep_n + 63) // 64) * 64 > 2 ** 32
    act = np.flatnonzero(ref.active)
    open_pairs = act[np.argsort(bs.tile_slot[act])[-2:]]
    assert (bs.K[open_pairs] <= 3).all()
    planes = [torch.full((2, 1 + rep_n), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64) for _ in range(2)]
    keep = bs.launch_range(0, rep_n, open_pairs, planes, np.array([1, 0]))
    for p, raw in zip(planes, (ref.raw_mean, ref.raw_var)):
        bits = p.view(torch.int64)
        assert int((bits[:, 1:] == int(SENTINEL)).sum().item()) == 0 and int((bits[:, 0] != int(SENTINEL)).sum().item()) == 0
        assert bool(torch.isfinite(p[:, 1:]).all().item())
        np.testing.assert_array_equal(eng.host(bits[:, 1:1 + B_REF]), raw[open_pairs[::-1], 1:].view(np.int64))
    del keep


def test_launch_range_checks_its_arguments(eng, ref):
    torch = eng._torch()
    bs = ref.bs
    planes = [torch.zeros((bs.n_pairs, 9), dtype=torch.float64, device="cuda") for _ in range(2)]
    pairs = np.arange(4)
    for bad in (dict(rep_lo=-1), dict(rep_n=0), dict(rep_n=9), dict(rep_lo=2 ** 31 - 5), dict(row_of_pair=np.array([0, 1, 2, bs.n_pairs])),
                dict(row_of_pair=np.array([0, 1, 2, -1])), dict(open_pairs=np.array([0, 1, 2, bs.n_pairs])), dict(row_of_pair=np.arange(3))):
        kw = dict(rep_lo=0, rep_n=8, open_pairs=pairs, planes=planes, row_of_pair=pairs)
        kw.update(bad)
        with pytest.raises(ValueError):
            bs.launch_range(**kw)
    assert all(float(p.abs().sum().item()) == 0.0 for p in planes)


def test_run_range_raises_after_a_replay_run(eng):
    prob = _problem()
    blocks = eng.CountBlocks(eng.DeviceCSR(prob.csr), prob.gid, prob.ng)
    _, _, maxx = blocks.moments(1.0 / prob.sf)
    bs = eng.Bootstrap1D(blocks, np.arange(3), maxx, prob.sf_bin, prob.sf_table, prob.grp_q, 16)
    bs.alloc_outputs(np.zeros(bs.n_pairs), np.zeros(bs.n_pairs))
    torch = eng._torch()
    planes = [torch.zeros((bs.n_pairs, 9), dtype=torch.float64, device="cuda") for _ in range(2)]
    args = (16, 8, np.arange(2), planes, np.arange(2), (0.0, 1.0, 0.0), 0, np.arange(bs.n_pairs))
    with pytest.raises(RuntimeError):
        bs.run_range(*args)                                          # before any run
    u = np.random.default_rng(1).random((2, bs.n_pairs))
    bs.run(np.zeros(bs.n_pairs, dtype=bool), u[0], u[1], (0.0, 1.0, 0.0), fill_seed=SEED)
    with pytest.raises(RuntimeError):
        bs.run_range(*args)
    assert all(float(p.abs().sum().item()) == 0.0 for p in planes)
