"""Kernel-level tests of the 1D histogram, bin-count and bin-order stage (mm_hist1d_sell, mm_bins_count, mm_bins_order in
csrc/hist.hip; Bootstrap1D.__init__, _order_bins and _order_on_host) against the numpy restatement of tests/_bins_ref.py.

Part B runs the whole stage on ``problem_1905``: 24,000 cells, a group of three count blocks, five dense genes whose chains have
K = 2400 / 1935, 11453 / 3525, 24 / 20, 40 / 34 (one count of 2^19 - 1) and 1024 / 1009 bins -- with the engine's default caps
six of them take the small ordering kernel (one exactly at its cap), three the big one and one the host.  Part C drives
mm_bins_count and mm_bins_order through the C-ABI on hand-built tables, part D checks the argument guards.

The integers (tables, K, weights) and the operands pk, count, 1/sf, 1/sf^2 must be bit-exact (the library is built with contraction
off, both sides do the same IEEE operations in the same order); lq = log(1 - p) within 2 ulp (one correctly-rounded-to-1-ulp log
on each side); replicate moments within the rounding bound of a sequential fp64 sum of K terms."""

from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from _bins_ref import K_1905, MAX_COUNT, pair_cells, problem_1905, ref_count, ref_order, ref_table, ulp_diff

pytestmark = pytest.mark.gpu

B = 8
SMALL_CAP, BIG_CAP = 1024, 8192                          # k_bins_order<1024, 64, Bins1D> / k_bins_order<8192, 512, Bins1D>
U = 2.0 ** -53
SENTINEL = np.array([0x7FF8DEADBEEF0BAD], dtype=np.uint64).view(np.float64)[0]      # a NaN with a payload no kernel produces


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import memento_oracle

    return memento_oracle


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------------------------------
# B. the whole stage on a problem with real long chains
# ------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prob():
    return problem_1905()


@pytest.fixture(scope="module")
def ref(prob):
    """[pair] -> (table, ref_order of it), computed once and left unchanged."""
    out = []
    for p in range(prob.n_genes * prob.ng):
        x, sbin = pair_cells(prob, p)
        t = ref_table(x, sbin, prob.n_bins, int(x.max()) + 1)
        out.append((t, ref_order(t, prob.sf_table, prob.r1[p], prob.r0[p], len(x))))
    return out


@pytest.fixture(scope="module")
def stage(eng, prob):
    """One ingest and one Bootstrap1D (histograms and bin counts done, nothing ordered yet) for the module; ``runs`` caches what
    every (caps, layout) run of _run left behind."""
    import torch

    csr = sp.csr_matrix(prob.X.astype(np.float32))
    blocks = eng.CountBlocks(eng.DeviceCSR(csr), prob.gid, prob.ng)
    sf = prob.sf_table[prob.sf_bin]
    S, sumx, maxx = blocks.moments(1.0 / sf)
    bs = eng.Bootstrap1D(blocks, np.arange(prob.n_genes), maxx, prob.sf_bin, prob.sf_table, prob.grp_q, B)
    st = SimpleNamespace(blocks=blocks, bs=bs, S=S, sumx=sumx, maxx=maxx, sf=sf, runs={})
    yield st
    st.runs.clear()
    for name in ("tab", "_opsbuf", "_ops", "w_dump", "w_dump_chain", "raw_mean", "raw_var"):      # (gene 3's table alone is 8 MB)
        if hasattr(bs, name):
            setattr(bs, name, None)
    torch.cuda.empty_cache()


def test_ingest_and_moments_at_the_count_limit(eng, prob, stage):
    """CountBlocks takes a count of 2^19 - 1, maxx reports it, sumx is exact and the three fp64 sums match np.longdouble column
    sums at the tolerance of test_moments_vs_oracle; group 0 spans three count blocks."""
    assert eng.MAX_COUNT == MAX_COUNT and prob.X[prob.big_cell, 3] == MAX_COUNT and prob.gid[prob.big_cell] == 0
    blocks = stage.blocks
    assert blocks.blk_group.tolist() == [0, 0, 0, 1] and blocks.grp_ncells.tolist() == prob.sizes
    assert stage.maxx[0, 3] == MAX_COUNT and stage.maxx[1, 3] < 100
    for k in range(prob.ng):
        Xg = prob.X[prob.sel[k]]
        np.testing.assert_array_equal(stage.maxx[k], Xg.max(axis=0).astype(np.uint32))
        np.testing.assert_array_equal(stage.sumx[k], Xg.sum(axis=0).astype(np.uint64))
        w = (1.0 / stage.sf[prob.sel[k]]).astype(np.longdouble)[:, None]
        w2 = (1.0 / stage.sf[prob.sel[k]] ** 2).astype(np.longdouble)[:, None]
        XL = Xg.astype(np.longdouble)
        np.testing.assert_allclose(stage.S[0, k], (XL * w).sum(axis=0).astype(np.float64), rtol=1e-12)
        np.testing.assert_allclose(stage.S[1, k], (XL * XL * w2).sum(axis=0).astype(np.float64), rtol=1e-12)
        np.testing.assert_allclose(stage.S[2, k], (XL * w2).sum(axis=0).astype(np.float64), rtol=1e-12)


def test_histograms_and_bin_counts_exact(prob, ref, stage):
    """mm_hist1d_sell + mm_bins_count for all ten pairs: the design's K values first, then every table cell (the atomics of three
    count blocks meet in group 0's tables), the bins, K, and xcap = 2^19 for the pair with the largest count."""
    bs = stage.bs
    assert [[ref_count(ref[g * 2 + k][0]) for k in range(2)] for g in range(5)] == K_1905, "the test problem drifted"
    assert bs.K.reshape(5, 2).tolist() == K_1905
    assert bs.xcap[3 * 2 + 0] == MAX_COUNT + 1 == 524288
    for p, (t, _) in enumerate(ref):
        assert bs.xcap[p] == t.shape[1], p
        bi, xi, mu = bs.bins_of_pair(p)
        wb, wx = np.nonzero(t)
        np.testing.assert_array_equal(bi, wb, err_msg=f"pair {p}")
        np.testing.assert_array_equal(xi, wx, err_msg=f"pair {p}")
        np.testing.assert_array_equal(mu, t[wb, wx], err_msg=f"pair {p}")
        assert bs.K[p] == ref_count(t) and int(mu.astype(np.int64).sum()) == prob.sizes[p % 2] == int(t.sum())
    assert (ref[4 * 2 + 0][0] != 0).all()                          # gene 4, group 0: all 4 x 256 bins occupied, K at the small cap


CONFIGS = [(caps, layout) for caps in ((SMALL_CAP, BIG_CAP), (0, BIG_CAP), (0, 0)) for layout in ("records", "planes")]


def _path_counts(caps):
    K = np.array(K_1905).ravel()
    return {"small": int((K <= caps[0]).sum()), "big": int(((K > caps[0]) & (K <= caps[1])).sum()), "host": int((K > caps[1]).sum())}


def _run(eng, prob, stage, caps, layout):
    """Bootstrap1D.run with the ordering caps and the operand layout set explicitly (cached per module): records = the default
    few-chain route (every chain one wave, 8-double records), planes = every chain a lane of a lock-step tile."""
    key = (caps, layout)
    if key in stage.runs:
        return stage.runs[key]
    bs = stage.bs
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(eng, "ORDER_SMALL_CAP", caps[0])
        mp.setattr(eng, "ORDER_BIG_CAP", caps[1])
        mp.setattr(eng, "TILE_MODE", "lockstep")
        mp.setattr(eng, "TILE_FREE", False)
        mp.setattr(eng, "CHAIN_MIN_K", 0)
        if layout == "planes":
            mp.setattr(eng, "CHAIN_ALL_MAX", 0)
            mp.setattr(eng, "CHAIN_LONE", False)
        zeros = np.zeros(bs.n_pairs)
        bs.alloc_outputs(zeros, zeros)
        bs.run(np.zeros(bs.n_pairs, dtype=bool), prob.r1, prob.r0, [0.0, 1.0, 0.0], fill_mode=1, dump_weights=True)
    finally:
        mp.undo()
    buf = eng.host(bs._opsbuf)
    plane = int(bs._ops[0].numel())
    ops = []
    for p in range(bs.n_pairs):
        K, slot = int(bs.K[p]), int(bs.pair_slot[p])
        if slot & eng.CHAIN_SLOT:
            rec = buf[(slot & (eng.CHAIN_SLOT - 1)) * 8:][:8 * K].reshape(K, 8)
            ops.append([rec[:, i].copy() for i in range(5)])
        else:
            idx = (int(bs.tile_ptr[slot >> 6]) + np.arange(K, dtype=np.int64)) * 64 + (slot & 63)
            ops.append([buf[i * plane:(i + 1) * plane][idx] for i in range(5)])
    out = SimpleNamespace(order_path=dict(bs.order_path), records=(bs.pair_slot & eng.CHAIN_SLOT) != 0, ops=ops,
                          raw_mean=eng.host(bs.raw_mean).copy(), raw_var=eng.host(bs.raw_var).copy(),
                          weights=[bs.weights_of(p).copy() for p in range(bs.n_pairs)], active=bs.active.copy())
    stage.runs[key] = out
    return out


@pytest.mark.parametrize("caps, layout", CONFIGS, ids=[f"{n}-{l}" for n in ("default-caps", "big-kernel", "host") for l in ("records", "planes")])
def test_ordering_on_every_path(eng, prob, ref, stage, caps, layout):
    """The ten chains ordered by the small kernel / the big kernel / the host as the caps say, written as records or into planes:
    pk, count, 1/sf and 1/sf^2 equal ref_order bit for bit, lq within 2 ulp, and the replicate means and variances of every run
    are bit-identical to those of the default one."""
    run = _run(eng, prob, stage, caps, layout)
    assert run.order_path == _path_counts(caps)
    if caps == (SMALL_CAP, BIG_CAP):
        assert run.order_path == {"small": 6, "big": 3, "host": 1}           # K <= 1024: 24, 20, 40, 34, 1024, 1009; host: 11453
    np.testing.assert_array_equal(run.records, np.full(10, layout == "records"))
    assert run.active.all()
    worst = 0
    for p, (_, (bi, xi, mult, pk, lq, a, b)) in enumerate(ref):
        g_pk, g_lq, g_v, g_a, g_b = run.ops[p]
        np.testing.assert_array_equal(g_v, xi.astype(np.float64), err_msg=f"pair {p}: counts in replay order")
        np.testing.assert_array_equal(_bits(g_pk), _bits(pk), err_msg=f"pair {p}: pk")
        np.testing.assert_array_equal(_bits(g_a), _bits(a), err_msg=f"pair {p}: 1/sf")
        np.testing.assert_array_equal(_bits(g_b), _bits(b), err_msg=f"pair {p}: 1/sf^2")
        d = int(ulp_diff(g_lq, lq).max())
        worst = max(worst, d)
        assert d <= 2, f"pair {p}: lq differs by {d} ulp"
    print(f"\n{caps} {layout}: {run.order_path}; largest lq difference {worst} ulp")
    base = _run(eng, prob, stage, (SMALL_CAP, BIG_CAP), "records")
    assert np.isfinite(base.raw_mean[:, 1:]).all() and np.isfinite(base.raw_var[:, 1:]).all()
    np.testing.assert_array_equal(_bits(run.raw_mean), _bits(base.raw_mean))
    np.testing.assert_array_equal(_bits(run.raw_var), _bits(base.raw_var))


@pytest.mark.parametrize("layout", ["records", "planes"])
def test_weights_and_replicate_moments_of_the_long_chains(eng, orc, prob, ref, stage, layout):
    """All ten chains, K = 11,453 included: the int32 weights equal numpy's multinomial draws exactly, and the replicate means and
    variances lie within the rounding bound of the kernel's sequential fp64 sums of a np.longdouble evaluation of
    replicate_moments_1d:  |d m1| <= (K + 4) 2^-53 sum|term| / N, the same for the second moment, and for the variance the
    second-moment bound + 2 m1 |d m1| + 4 ulp of m1^2."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble must be wider than fp64 for this reference"
    run = _run(eng, prob, stage, (SMALL_CAP, BIG_CAP), layout)
    worst_m, worst_v = 0.0, 0.0
    L = np.longdouble
    for p, (_, (bi, xi, mult, pk, lq, a, b)) in enumerate(ref):
        K, N, omq = len(mult), prob.sizes[p % 2], 1.0 - prob.grp_q[p % 2]
        w = orc.multinomial_weights(N, mult, B)
        np.testing.assert_array_equal(run.weights[p], w, err_msg=f"pair {p} (K = {K})")
        e = xi.astype(np.float64)
        want_m, want_v = orc.replicate_moments_1d(e, a, b, w, N, prob.grp_q[p % 2])
        eL, aL, bL, wL = e.astype(L)[:, None], a.astype(L)[:, None], b.astype(L)[:, None], w.astype(L)
        t1 = eL * wL * aL
        t2a, t2b = eL * eL * wL * bL, L(omq) * eL * wL * bL
        m1 = t1.sum(axis=0) / N
        m2 = (t2a - t2b).sum(axis=0) / N
        var = m2 - m1 * m1
        bound1 = (K + 4) * U * np.abs(t1).sum(axis=0) / N
        bound2 = (K + 4) * U * (np.abs(t2a) + np.abs(t2b)).sum(axis=0) / N
        bound_v = bound2 + 2 * m1 * bound1 + 4 * U * m1 * m1
        got_m, got_v = run.raw_mean[p, 1:], run.raw_var[p, 1:]
        rm = float((np.abs(got_m.astype(L) - m1) / bound1).max())
        rv = float((np.abs(got_v.astype(L) - var) / bound_v).max())
        worst_m, worst_v = max(worst_m, rm), max(worst_v, rv)
        assert rm <= 1.0, f"pair {p} (K = {K}): replicate mean off by {rm:.3g} of its bound"
        assert rv <= 1.0, f"pair {p} (K = {K}): replicate variance off by {rv:.3g} of its bound"
        np.testing.assert_allclose(got_m, want_m, rtol=1e-11)                # and the oracle's own fp64 evaluation, loosely
        np.testing.assert_allclose(got_v, want_v, rtol=1e-7, atol=1e-12)
    print(f"\n{layout}: worst ratio to the bound: mean {worst_m:.3g}, variance {worst_v:.3g}")


# ------------------------------------------------------------------------------------------------------------------------
# C. mm_bins_count and mm_bins_order on hand-built tables through the C-ABI
# ------------------------------------------------------------------------------------------------------------------------

PAD = 0xA5A5A5A5                       # cells around and between the tables, which no kernel may touch
NG = 3


@pytest.mark.parametrize("n_pairs, n_sf_bins", [(1, 1), (4, 5), (5, 256), (7, 5), (7, 1), (6, 256)])
def test_bins_count_on_hand_built_tables(eng, n_pairs, n_sf_bins):
    """mm_bins_count: tables of xcap 1 (a gene that is never expressed: nothing but the zero column), 2, 64, 65, 66 and 129 in three
    groups, with a size-factor bin that holds no cell, one whose cells all have a count (zero column 0: not a bin) and column 0
    pre-filled with garbage: K and the zero column exact, every other cell -- the padding between the tables and the K entries
    past n_pairs (the last workgroup is partly empty) included -- unchanged."""
    rng = np.random.default_rng(1000 * n_pairs + n_sf_bins)
    xcaps = np.array([1, 2, 64, 65, 66, 129, 129])[:n_pairs] if n_pairs > 1 else np.array([65])
    gbc = rng.integers(1, 400, size=(NG, n_sf_bins)).astype(np.uint32)
    if n_sf_bins > 1:
        gbc[:, n_sf_bins // 2] = 0                                         # a bin without cells
    elif n_pairs > 1:
        gbc[0, 0] = 0                                                      # (with one bin: in group 0 only)
    tab_ptr, parts, want_parts, want_K = [], [np.full(64, PAD, dtype=np.uint32)], [np.full(64, PAD, dtype=np.uint32)], []
    pos = 64
    kinds = set()
    for p in range(n_pairs):
        xc, grp = int(xcaps[p]), p % NG
        t = np.zeros((n_sf_bins, xc), dtype=np.uint32)
        for bin_ in range(n_sf_bins):
            c = int(gbc[grp, bin_])
            if xc > 1 and c > 0:
                full = (bin_ + p) % 2 == 0                                 # every cell of the bin has a count
                s = c if full else int(rng.integers(0, c))
                at = rng.integers(1, xc, size=s)
                t[bin_] = np.bincount(at, minlength=xc)
                kinds.add("full" if full else "mixed")
            else:
                kinds.add("empty" if c == 0 else "zeros only")
        want = t.copy()
        want[:, 0] = gbc[grp] - t[:, 1:].sum(axis=1, dtype=np.uint32)
        assert want.sum() == gbc[grp].sum()
        t[:, 0] = 0xBAD0 + np.arange(n_sf_bins)                            # garbage where the kernel must write
        tab_ptr.append(pos)
        gap = np.full(1 + p, PAD, dtype=np.uint32)
        parts += [t.ravel(), gap]
        want_parts += [want.ravel(), gap]
        want_K.append(ref_count(want))
        pos += t.size + len(gap)
    assert kinds >= ({"empty", "full", "mixed"} if n_pairs > 1 else {"full"})
    d_tab = eng.dev(np.concatenate(parts))
    d_ptr, d_xcap, d_gbc = eng.dev(np.array(tab_ptr, dtype=np.int64)), eng.dev(xcaps.astype(np.int32)), eng.dev(gbc)
    d_K = eng.dev(np.full(n_pairs + 9, -77, dtype=np.int32))
    eng._lib.call("mm_bins_count", eng.P(d_tab), eng.P(d_ptr), eng.P(d_xcap), n_pairs, NG, n_sf_bins, eng.P(d_gbc), eng.P(d_K), eng._stream())
    np.testing.assert_array_equal(eng.host(d_K), np.concatenate([want_K, np.full(9, -77)]))
    np.testing.assert_array_equal(eng.host(d_tab, np.uint32), np.concatenate(want_parts))


SF8 = np.array([0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 2.5, 3.0])
GRP_N = np.array([100003.0, 250000.0, 70001.0])


def _table(rng, K, n_bins, xcap, n_cells, dense=False):
    """[n_bins][xcap] table with K non-empty bins whose multiplicities sum to n_cells."""
    t = np.zeros(n_bins * xcap, dtype=np.uint32)
    at = np.arange(K) if dense else rng.choice(n_bins * xcap, size=K, replace=False)
    t[at] = 1 + rng.multinomial(n_cells - K, np.full(K, 1.0 / K))
    return t.reshape(n_bins, xcap)


def _spec(K, xcap=None, slot="rec", listed=True, r=None, claim=None, table=None, dense=False):
    return SimpleNamespace(K=K, xcap=xcap, slot=slot, listed=listed, r=r, claim=claim, table=table, dense=dense)


def _order_launch(eng, specs, big, seed, n_bins=8, sf_table=SF8):
    """One mm_bins_order launch on the hand-built tables of ``specs`` (pair p = position in the list, group p % 3).  A spec's slot
    is "rec" (8-double records), (tile, lane) of the planes, or None (pair_slot -1); ``claim`` is the K entry when it is not the
    table's.  Every operand word starts as SENTINEL.  Returns (status, operand buffer after the launch, the buffer expected from
    ref_order -- SENTINEL wherever no written pair owns the word --, a mask of the lq words, what ref_order gave per pair, the words
    of every pair that has a slot)."""
    import torch

    rng = np.random.default_rng(seed)
    n = len(specs)
    tabs, tab_ptr, pos = [], [], 0
    for p, s in enumerate(specs):
        if s.table is None:
            if s.xcap is None:
                s.xcap = s.K // n_bins if s.dense else max(2, -(-3 * s.K // (2 * n_bins)) + p % 3)
            s.table = _table(rng, s.K, n_bins, s.xcap, int(GRP_N[p % NG]), dense=s.dense)
        s.xcap = s.table.shape[1]
        assert s.table.shape[0] == n_bins and s.xcap <= MAX_COUNT + 1 and ref_count(s.table) == s.K
        if s.r is None:
            s.r = tuple(rng.random(2))
        tab_ptr.append(pos)
        tabs.append(s.table.ravel())
        pos += s.table.size
    # tiles: rows of a tile = its longest chain, whether that chain is listed or not
    tiles = sorted({s.slot[0] for s in specs if isinstance(s.slot, tuple)})
    assert tiles == list(range(len(tiles)))
    tile_k = np.zeros(len(tiles) + 1, dtype=np.int64)
    for s in specs:
        if isinstance(s.slot, tuple):
            tile_k[s.slot[0]] = max(tile_k[s.slot[0]], s.K + 1)            # one spare row under the longest chain
    tile_ptr = np.concatenate([[0], np.cumsum(tile_k)]).astype(np.int64)
    plane = max(1, int(tile_ptr[-1])) * 64
    rec_K = np.array([s.K + 1 if s.slot == "rec" else 0 for s in specs], dtype=np.int64)      # one spare record behind each chain
    rec_base = 5 * plane // 8 + np.concatenate([[0], np.cumsum(rec_K)])
    pair_slot = np.full(n, -1, dtype=np.int64)
    for p, s in enumerate(specs):
        if s.slot == "rec":
            pair_slot[p] = eng.CHAIN_SLOT | int(rec_base[p])
        elif s.slot is not None:
            pair_slot[p] = s.slot[0] * 64 + s.slot[1]
    assert len(set(pair_slot[pair_slot >= 0].tolist())) == int((pair_slot >= 0).sum())
    total = int(rec_base[-1]) * 8 + 64
    want = np.full(total, SENTINEL)
    is_lq = np.zeros(total, dtype=bool)
    refs, own = {}, {}

    def words(p, s, i):
        if s.slot == "rec":
            return (int(rec_base[p]) + np.arange(s.K)) * 8 + i
        return i * plane + (int(tile_ptr[s.slot[0]]) + np.arange(s.K)) * 64 + s.slot[1]

    for p, s in enumerate(specs):
        claim = s.K if s.claim is None else s.claim
        cap = BIG_CAP if big else SMALL_CAP
        if s.slot is not None:
            own[p] = np.concatenate([words(p, s, i) for i in range(5)])
        if not s.listed or s.slot is None or claim != s.K or s.K > cap:
            continue                                                       # nothing may be written for this pair
        try:
            bi, xi, mult, pk, lq, a, b = refs[p] = ref_order(s.table, sf_table, s.r[0], s.r[1], GRP_N[p % NG])
        except AssertionError:
            refs[p] = None                                                 # equal codes: the kernel reports it, the words are not compared
            continue
        vals = (pk, lq, xi.astype(np.float64), a, b)
        for i, v in enumerate(vals):
            want[words(p, s, i)] = v
            is_lq[words(p, s, i)] = i == 1
    lst = np.array([p for p, s in enumerate(specs) if s.listed], dtype=np.int64)
    d_tab = eng.dev(np.concatenate(tabs))
    d_ptr, d_xcap = eng.dev(np.array(tab_ptr, dtype=np.int64)), eng.dev(np.array([s.xcap for s in specs], dtype=np.int32))
    d_K = eng.dev(np.array([s.K if s.claim is None else s.claim for s in specs], dtype=np.int32))
    d_list, d_sf, d_N = eng.dev(lst), eng.dev(np.asarray(sf_table, dtype=np.float64)), eng.dev(GRP_N)
    d_r1, d_r0 = eng.dev(np.array([s.r[0] for s in specs])), eng.dev(np.array([s.r[1] for s in specs]))
    d_slot, d_tptr = eng.dev(pair_slot), eng.dev(tile_ptr)
    buf = eng.dev(np.full(total, SENTINEL))
    ops = [buf[i * plane:(i + 1) * plane] for i in range(5)]
    status = eng.zeros((1,), torch.int32)
    eng._lib.call("mm_bins_order", eng.P(d_tab), eng.P(d_ptr), eng.P(d_xcap), eng.P(d_K), eng.P(d_list), len(lst), int(big), NG, n_bins,
                  eng.P(d_sf), eng.P(d_r1), eng.P(d_r0), eng.P(d_slot), eng.P(d_tptr), eng.P(d_N), *map(eng.P, ops), eng.P(status),
                  eng._stream())
    st = int(status.item())
    got = eng.host(buf)
    del d_tab, d_ptr, d_xcap, d_K, d_list, d_sf, d_N, d_r1, d_r0, d_slot, d_tptr
    return SimpleNamespace(st=st, got=got, want=want, is_lq=is_lq, refs=refs, own=own)


def _compare(got, want, is_lq):
    """Bitwise equality of every operand word but the lq words, which may differ by 2 ulp.  Returns the largest lq difference."""
    d = ulp_diff(got[is_lq], want[is_lq])
    worst = int(d.max()) if len(d) else 0
    assert worst <= 2, f"lq differs by {worst} ulp"
    g = got.copy()
    g[is_lq] = want[is_lq]
    bad = np.flatnonzero(_bits(g) != _bits(want))
    assert len(bad) == 0, f"{len(bad)} operand words differ, the first at {bad[:8]}: {g[bad[:8]]} instead of {want[bad[:8]]}"
    return worst


SMALL_KS = [2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024]
BIG_ONLY_KS = [1025, 4097, 8192]


def _generic_specs(Ks, layout):
    """Pairs of the given K: as records, or as lanes 0 / 17 / 63 of tiles shared by three chains of different length; a dense table
    (every cell a bin) where K is a kernel's cap.  Behind them a pair with pair_slot -1 and one that is not listed."""
    specs = []
    for i, K in enumerate(Ks):
        slot = "rec" if layout == "records" else (i // 3, (0, 17, 63)[i % 3])
        specs.append(_spec(K, slot=slot, dense=K in (SMALL_CAP, BIG_CAP)))
    specs.append(_spec(40, slot=None))
    specs.append(_spec(50, slot="rec" if layout == "records" else ((len(Ks) - 1) // 3, 40), listed=False))
    return specs


@pytest.mark.parametrize("layout", ["records", "planes"])
@pytest.mark.parametrize("big", [0, 1], ids=["small-kernel", "big-kernel"])
def test_bins_order_on_hand_built_tables(eng, big, layout):
    """Both instantiations of k_bins_order on chains of 2 ... 1024 bins (the big one also 1025, 4097 and 8192: its cap, all of its
    128 KiB of LDS and the strided loops of its sort), with hash uniforms that interleave the size-factor bins: every operand
    word equals ref_order's (lq within 2 ulp), every word no listed pair owns keeps its sentinel -- the rows below a shorter chain
    of a shared tile, the lanes nobody has, the pair with pair_slot -1 and the pair missing from pair_list."""
    Ks = SMALL_KS + (BIG_ONLY_KS if big else [])
    specs = _generic_specs(Ks, layout)
    res = _order_launch(eng, specs, big, seed=77 + big)
    assert res.st == 0
    assert sorted(res.refs) == list(range(len(Ks)))
    descents = [int((np.diff(res.refs[p][0]) < 0).sum()) for p in range(len(Ks)) if Ks[p] >= 63]
    assert min(descents) > 10                                              # the codes interleave across the size-factor bins
    worst = _compare(res.got, res.want, res.is_lq)
    assert int((_bits(res.want) == _bits(SENTINEL)).sum()) > 64                # and there are words that must stay as they were
    print(f"\nbig = {big}, {layout}: K = {Ks}: largest lq difference {worst} ulp")


@pytest.mark.parametrize("big", [0, 1], ids=["small-kernel", "big-kernel"])
def test_bins_order_descending_input_and_mixed_layouts(eng, big):
    """A pair whose canonical (bin-major) order is exactly descending in code (negative multipliers: the sort has to reverse it),
    as a record chain beside tile lanes in one launch."""
    specs = [_spec(600, xcap=100, slot=(0, 5), r=(-1e-4, -0.81)), _spec(70, slot="rec"), _spec(9, slot=(0, 6)),
             _spec(600, xcap=100, slot="rec", r=(-1e-4, -0.81))]
    res = _order_launch(eng, specs, big, seed=5)
    assert res.st == 0
    for p in (0, 3):
        bi, xi = res.refs[p][0], res.refs[p][1]
        wb, wx = np.nonzero(specs[p].table)
        np.testing.assert_array_equal(bi, wb[::-1])
        np.testing.assert_array_equal(xi, wx[::-1])
    _compare(res.got, res.want, res.is_lq)


@pytest.mark.parametrize("big", [0, 1], ids=["small-kernel", "big-kernel"])
def test_bins_order_every_payload_bit(eng, big):
    """Size-factor bin 255 with a count of 2^19 - 1 sets every bit of the 1D payload word bin << 19 | x (256 bins of 2^19 cells: the
    compaction walks 2^27 cells).  The table is built on the device."""
    import torch

    n_bins, xcap = 256, MAX_COUNT + 1
    cells = [(255, MAX_COUNT), (0, 0), (255, 0), (128, 1), (0, MAX_COUNT), (127, 262144), (1, 0)]
    mult = np.array([1, 40000, 30000, 20000, 5000, 5001, 1], dtype=np.uint32)
    assert mult.sum() == GRP_N[0]
    sf_table = np.linspace(0.4, 2.5, n_bins)
    r1, r0 = 3.1e-6, 0.77                                                  # count and size-factor terms of similar size
    d_tab = eng.zeros((n_bins * xcap,), torch.int32)
    flat = np.array([b * xcap + x for b, x in cells], dtype=np.int64)
    d_tab[eng.dev(flat)] = eng.dev(mult)
    order = np.argsort([x * r1 + r0 * sf_table[b] for b, x in cells])
    K = len(cells)
    buf = eng.dev(np.full(8 * (K + 1) + 5 * 64, SENTINEL))
    ops = [buf[i * 64:(i + 1) * 64] for i in range(5)]
    d_ptr, d_list = eng.dev(np.zeros(1, dtype=np.int64)), eng.dev(np.zeros(1, dtype=np.int64))
    d_xcap, d_K = eng.dev(np.array([xcap], dtype=np.int32)), eng.dev(np.array([K], dtype=np.int32))
    d_sf, d_r1, d_r0, d_N = eng.dev(sf_table), eng.dev(np.array([r1])), eng.dev(np.array([r0])), eng.dev(GRP_N)
    d_slot, d_tptr = eng.dev(np.array([eng.CHAIN_SLOT | 40], dtype=np.int64)), eng.dev(np.array([0, 1], dtype=np.int64))
    status = eng.zeros((1,), torch.int32)
    eng._lib.call("mm_bins_order", eng.P(d_tab), eng.P(d_ptr), eng.P(d_xcap), eng.P(d_K), eng.P(d_list), 1, int(big), NG, n_bins,
                  eng.P(d_sf), eng.P(d_r1), eng.P(d_r0), eng.P(d_slot), eng.P(d_tptr), eng.P(d_N), *map(eng.P, ops), eng.P(status),
                  eng._stream())
    assert int(status.item()) == 0
    got = eng.host(buf)
    del d_tab
    torch.cuda.empty_cache()
    # the restatement on the seven cells (ref_order's arithmetic, without the 512 MB dense table on the host)
    bo = np.array([cells[i][0] for i in order])
    xo = np.array([cells[i][1] for i in order], dtype=np.float64)
    pix = mult[order].astype(np.float64) / GRP_N[0]
    rem = np.subtract.accumulate(np.concatenate([[1.0], pix]))[:-1]
    pk = pix / rem
    lq = np.log(1.0 - np.where(pk <= 0.5, pk, 1.0 - pk))
    sf = sf_table[bo]
    assert (255, MAX_COUNT) in cells and len(set(np.round([x * r1 + r0 * sf_table[b] for b, x in cells], 9))) == K
    rec = got[40 * 8:40 * 8 + 8 * K].reshape(K, 8)
    np.testing.assert_array_equal(rec[:, 2], xo)
    np.testing.assert_array_equal(_bits(rec[:, 0]), _bits(pk))
    np.testing.assert_array_equal(_bits(rec[:, 3]), _bits(1.0 / sf))
    np.testing.assert_array_equal(_bits(rec[:, 4]), _bits(1.0 / (sf * sf)))
    assert ulp_diff(rec[:, 1], lq).max() <= 2
    untouched = np.ones(len(got), dtype=bool)
    untouched[40 * 8:40 * 8 + 8 * K].reshape(K, 8)[:, :5] = False
    assert (_bits(got[untouched]) == _bits(SENTINEL)).all()


def _dense_over(n_cells_nonzero, n_bins=8):
    """A table with ``n_cells_nonzero`` non-empty bins, all ones (its multiplicities are never used: the pair is refused)."""
    xcap = -(-n_cells_nonzero // n_bins) + 3
    t = np.zeros(n_bins * xcap, dtype=np.uint32)
    t[np.arange(n_cells_nonzero) * 1 + 5] = 1
    return t.reshape(n_bins, xcap)


@pytest.mark.parametrize("layout", ["records", "planes"])
@pytest.mark.parametrize("big", [0, 1], ids=["small-kernel", "big-kernel"])
def test_bins_order_status_word(eng, big, layout):
    """The kernel's early returns: more bins than the instantiation holds (status 2), a K entry that is one more or one less than
    the table's non-empty cells, or a table with more than CAP non-empty cells under a claimed K <= CAP (status 4: the compaction
    stops storing at CAP), two equal codes (status 8).  Nothing is written for a refused pair (2, 4), and a generic pair in the same
    launch is written correctly every time."""
    cap = BIG_CAP if big else SMALL_CAP
    slot = (lambda i: "rec") if layout == "records" else (lambda i: (0, (3, 44)[i]))
    cases = [
        (2, _spec(cap + 1, slot=slot(0))),
        (4, _spec(100, slot=slot(0), claim=101)),
        (4, _spec(100, slot=slot(0), claim=99)),
        (4, _spec(cap + 70, slot=slot(0), claim=cap, table=_dense_over(cap + 70))),
        (4, _spec(cap + 1, slot=slot(0), claim=cap - 1, table=_dense_over(cap + 1))),
    ]
    for i, (code, bad) in enumerate(cases):
        res = _order_launch(eng, [bad, _spec(130, slot=slot(1))], big, seed=300 + i)
        assert res.st == code, (i, res.st)
        assert list(res.refs) == [1]                                        # the expected buffer holds the generic pair alone
        _compare(res.got, res.want, res.is_lq)
    # equal codes: (bin 2, x 2) and (bin 5, x 1) with r1 == r0 == 0.25 and size factors 1.0 and 2.0 both give 0.75
    t = np.zeros((8, 4), dtype=np.uint32)
    t[2, 2], t[5, 1], t[0, 0], t[7, 3] = 3, 4, int(GRP_N[0]) - 9, 2
    tie = _spec(4, slot=slot(0), table=t, r=(0.25, 0.25))
    res = _order_launch(eng, [tie, _spec(130, slot=slot(1))], big, seed=400)
    assert res.st == 8 and res.refs[0] is None and res.refs[1] is not None
    # the pair with the tie is reported, not refused (include/memento_hip.h: "d_status[0] |= 8"): its own four rows hold whatever
    # order the sort left the equal codes in and are not compared; every other word is
    g, w = res.got.copy(), res.want.copy()
    g[res.own[0]] = w[res.own[0]] = 0.0
    _compare(g, w, res.is_lq)


# ------------------------------------------------------------------------------------------------------------------------
# D. argument guards
# ------------------------------------------------------------------------------------------------------------------------


def _some_buffers(eng, n):
    return [eng.dev(np.zeros(8, dtype=np.int64)) for _ in range(n)]


def test_hist1d_rejects_more_genes_than_its_slice_table_holds(eng):
    """mm_hist1d_sell stages a block's item pointers in LDS for at most 1024 slices of 64 genes: n_genes = 65537 is a bad argument,
    returned before any launch (n_blocks = 0 here, so nothing could be launched either way); 65536 is accepted."""
    b = _some_buffers(eng, 13)
    args = lambda n_genes: [*map(eng.P, b[:9]), 0, n_genes, *map(eng.P, b[9:13]), eng._stream()]
    eng._lib.call("mm_hist1d_sell", *args(65536))
    with pytest.raises(eng._lib.MementoHipError, match="n_genes <= 65536"):
        eng._lib.call("mm_hist1d_sell", *args(65537))


@pytest.mark.parametrize("entry", ["mm_bins_order", "mm_bins_order2d"])
@pytest.mark.parametrize("bad", ["n_groups", "n_sf_bins"])
def test_bins_order_rejects_nonpositive_group_and_bin_counts(eng, entry, bad):
    """Both ordering entries divide by n_groups and loop to n_sf_bins: zero or a negative value of either is a bad argument, returned
    before any launch (n_list = 0 here, so nothing could be launched either way); positive values are accepted."""
    n_ptr = 5 if entry == "mm_bins_order" else 6
    n_tail = 13 if entry == "mm_bins_order" else 15
    b = _some_buffers(eng, n_ptr + n_tail - 1)
    args = lambda ng, nb: [*map(eng.P, b[:n_ptr]), 0, 0, ng, nb, *map(eng.P, b[n_ptr:]), eng._stream()]
    eng._lib.call(entry, *args(1, 1))
    for v in (0, -1):
        with pytest.raises(eng._lib.MementoHipError, match=f"{bad} > 0"):
            eng._lib.call(entry, *(args(v, 4) if bad == "n_groups" else args(2, v)))
