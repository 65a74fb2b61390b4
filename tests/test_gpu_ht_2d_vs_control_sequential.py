"""GPU tests of the sequential bootstrap of the 2D screen: ht_2d_vs_control_sequential(rng='fast', max_boot=..., min_extreme=...).

The matrix of tests/test_gpu_ht_2d_sequential.py widened to 4 guide values x 3 replicates: 6,000 cells x 150 genes in twelve
groups of 500 cells.  62 distinct pairs: 6 whose genes share a latent factor in the cells of guide 1 only, 54 pairs of independent
well-expressed genes, one pair of sparse genes (0.3 counts per cell) and one pair with a gene that is never seen in the control
cells (guide 0): its control chains are skipped, so none of its tests has a good control group.  A duplicate of one pair and a
self pair are requested on top.  num_boot = 200, max_boot = 3200, the schedule is (200, 400, 800, 1600, 3200); fill_seed is fixed
and np.random.seed is set before every call.

Every check runs in both modes of the call: ``groups`` -- treatment_col=None, the one control group (guide 0, replicate 0) against
each of the eleven others, two-entry designs -- and ``strata`` -- treatment_col='guide' with the replicate as stratum, three guides
against guide 0, weighted designs of up to six entries.

The 2D path refills nothing, so a test that is never closed early has the valid, extreme and raw-extreme counts of the one-shot
num_boot = 3200 call, whatever the chunking and the sub-batching of a round.
"""

from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

N_CELLS, N_GENES = 6000, 150
COUPLED = [(2 * i, 2 * i + 1) for i in range(6)]
OTHERS = [(20 + i, 80 + i) for i in range(54)]
SPARSE = (140, 141)
NO_CTRL = (142, 143)                     # gene 142 has no count in the cells of guide 0
DUP_OF, SELF = OTHERS[0], (30, 30)
PAIRS = COUPLED + OTHERS + [SPARSE, NO_CTRL, DUP_OF, SELF]
I_NO_CTRL, I_DUP, I_SELF = len(PAIRS) - 3, len(PAIRS) - 2, len(PAIRS) - 1
N_DISTINCT = len(COUPLED) + len(OTHERS) + 2
NUM_BOOT, MAX_BOOT, FILL_SEED = 200, 3200, 17
SCHEDULE = (200, 400, 800, 1600, 3200)
KEYS = ("corr_coef", "corr_se", "corr_asl", "corr_nboot")
NG = 12
COUPLING = 0.5                           # shape of the latent factor, gamma(shape, 1 / shape): mean 1, variance 2.  The log-normal(0, 0.5)
#                                          factor of test_gpu_ht_2d_sequential (variance 0.28, 1,000-cell groups) leaves a 500-cell guide
#                                          group against a 500-cell control group too little power for EVERY planted test to stay open
#                                          after 200 replicates (measured: 5 of 18 closed in round 0; 1 of 18 at log-normal(0, 1.0))
MODES = {"groups": SimpleNamespace(name="groups", control="sg^0^0", treatment_col=None, n_t=11),
         "strata": SimpleNamespace(name="strata", control=0, treatment_col="guide", n_t=3)}


def _adata(seed=5, n_guides=4, n_rep=3):
    from scrna_parameter_estimation_amd.anndata_lite import AnnDataLite

    rng = np.random.default_rng(seed)
    guide, rep = np.arange(N_CELLS) % n_guides, (np.arange(N_CELLS) // n_guides) % n_rep
    mu = rng.uniform(2.0, 6.0, size=N_GENES)
    mu[list(SPARSE)] = 0.3
    lam = mu[None, :] * rng.lognormal(0.0, 0.25, size=N_CELLS)[:, None] * rng.gamma(2.0, 0.5, size=(N_CELLS, N_GENES))
    for a, b in COUPLED:
        z = rng.gamma(COUPLING, 1.0 / COUPLING, size=N_CELLS)
        sel = guide == 1
        lam[sel, a] *= z[sel]
        lam[sel, b] *= z[sel]
    X = rng.poisson(lam).astype(np.float32)
    if n_guides > 2:
        X[guide == 0, NO_CTRL[0]] = 0
    obs = pd.DataFrame({"guide": guide, "rep": rep, "q": np.full(N_CELLS, 0.07)}, index=[f"c{i}" for i in range(N_CELLS)])
    return AnnDataLite(sp.csr_matrix(X), obs, pd.DataFrame(index=[f"g{i}" for i in range(N_GENES)]))


@pytest.fixture(scope="module")
def adata():
    from scrna_parameter_estimation_amd import memento

    adata = _adata()
    memento.setup_memento(adata, q_column="q", filter_mean_thresh=0.07)
    memento.create_groups(adata, label_columns=["guide", "rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.7)
    m = adata.uns["memento"]
    assert len(m["_hip"].gene_idx) == N_GENES and len(m["groups"]) == NG and m["groups"][0] == "sg^0^0"
    memento.compute_2d_moments(adata, [(f"g{a}", f"g{b}") for a, b in PAIRS])
    return adata


def _records(adata, n_t):
    """The test records of the call's one pair chunk (device pair order) as [requested pair][tested guide][8]; NaN rows where
    there is no test."""
    from scrna_parameter_estimation_amd.memento import _ht

    m = adata.uns["memento"]
    st = m["_hip"]
    assert st.last_chunk2d == (0, N_DISTINCT)
    _, members = _ht.distinct_pairs(m["2d_moments"]["gene_idx_1"], m["2d_moments"]["gene_idx_2"])
    rec, order = np.asarray(st.last_records2d).reshape(N_DISTINCT, n_t, 8), st.last_bootstrap2d.order
    out = np.full((len(PAIRS), n_t, 8), np.nan)
    for k in range(N_DISTINCT):
        out[members[int(order[k])]] = rec[k]
    return out


def _call(adata, mode, **kw):
    """One call (rng='fast', approx=False) from a fixed state of the global numpy stream: ht_2d_vs_control_sequential with
    ``max_boot``, the plain ht_2d_vs_control without."""
    from scrna_parameter_estimation_amd import memento

    np.random.seed(23)
    kw.setdefault("num_boot", NUM_BOOT)
    call = memento.ht_2d_vs_control_sequential if "max_boot" in kw else memento.ht_2d_vs_control
    df = call(adata, control=mode.control, treatment_col=mode.treatment_col, num_cpus=1, rng="fast", fill_seed=FILL_SEED, approx=False, **kw)
    m = adata.uns["memento"]
    st = m["_hip"]
    assert st.last_bootstrap2d.replay_kernel == "mm_boot2d_fast" and len(df) == len(PAIRS) * mode.n_t
    uns = {k: (np.array(v).reshape(len(PAIRS), mode.n_t) if isinstance(v, np.ndarray) else v) for k, v in m["2d_ht_vs_control"].items()}
    seq = st.last_sequential if "max_boot" in kw else None
    return SimpleNamespace(uns=uns, df=df.copy(), rec=None if "max_rows" in kw else _records(adata, mode.n_t),
                           n_open=list(seq.n_open) if seq else None, n_chains=list(seq.n_chains) if seq else None,
                           schedule=list(seq.schedule) if seq else None, open_mask=[None if a is None else a.copy() for a in seq.open_mask] if seq else None)


@pytest.fixture(scope="module", params=list(MODES))
def runs(request, adata):
    """The mode and its four shared calls, computed once: the one-shot 3200-replicate call, the plain 200-replicate call, the
    sequential call with the default min_extreme (LAST: the chunk it leaves is what the tests below continue from) and the one in
    which nothing closes early."""
    mode = MODES[request.param]
    one_shot = _call(adata, mode, num_boot=MAX_BOOT)
    plain = _call(adata, mode)
    never_closed = _call(adata, mode, max_boot=MAX_BOOT, min_extreme=MAX_BOOT)
    seq = _call(adata, mode, max_boot=MAX_BOOT)
    return SimpleNamespace(mode=mode, one_shot=one_shot, plain=plain, never_closed=never_closed, seq=seq)


def _view(adata, mode):
    """The tests of the last call's one chunk as the driver hands them to the continuation (device pair order, pair-major):
    test_pair, test_design and the CSR tables, rebuilt from the chunk's good groups."""
    from scrna_parameter_estimation_amd.memento import _ht, main

    m = adata.uns["memento"]
    bs = m["_hip"].last_bootstrap2d
    tested, designs, (ctrl, _), _ = main._vs_control_plan(m, mode.control, mode.treatment_col)
    good = bs.active.reshape(bs.n_pairs, bs.ng)
    d = _ht._TwoGroupDesigns(bs.ng, ctrl) if designs is None else designs
    test_design = d.tests(good)
    assert len(tested) == mode.n_t and bs.ng == NG and bs.n_pairs == N_DISTINCT
    return SimpleNamespace(bs=bs, test_pair=np.repeat(np.arange(bs.n_pairs), mode.n_t), test_design=test_design, tables=d.tables())


def _same_bits(a, b, what=""):
    np.testing.assert_array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64), err_msg=what)


def _brute_chains(v, tests):
    ptr, grp, _ = v.tables
    return {int(v.test_pair[t]) * NG + int(grp[e]) for t in tests for e in range(int(ptr[v.test_design[t]]), int(ptr[v.test_design[t] + 1]))}


def test_nothing_closes_early_is_the_one_shot_call(runs):
    one, got, n_t = runs.one_shot, runs.never_closed, runs.mode.n_t
    r1, r, u1, u = one.rec, got.rec, one.uns, got.uns
    live = np.isfinite(r1[:, :, 0])
    print(f"\n{runs.mode.name}: {int(live.sum())} live tests; one-shot n_valid min {r1[live][:, 2].min():.0f} max {r1[live][:, 2].max():.0f}; "
          f"extreme counts <= 10: {int((r1[live][:, 3] <= 10).sum())}; n_open {got.n_open}; n_chains {got.n_chains}")
    assert live[:I_NO_CTRL].all() and live[I_DUP].all() and not live[I_NO_CTRL].any() and not live[I_SELF].any()
    assert "corr_nboot" not in u1 and "max_boot" not in u1 and "corr_nboot" not in one.df.columns
    assert u["max_boot"] == MAX_BOOT and u["min_extreme"] == MAX_BOOT and list(got.df.columns)[-1] == "corr_nboot"
    for k in (2, 3, 6):                                                           # n_valid, n_extreme, n_raw_extreme
        np.testing.assert_array_equal(r[live][:, k], r1[live][:, k])
    assert (r1[live][:, 2] == MAX_BOOT).all()
    np.testing.assert_array_equal(u["corr_nboot"], np.where(live, r1[:, :, 2], 0).astype(np.int64))           # corr_nboot == n_valid
    np.testing.assert_array_equal(got.df["corr_nboot"].values, u["corr_nboot"].reshape(-1))
    _same_bits(u["corr_coef"], u1["corr_coef"], "corr_coef")
    np.testing.assert_array_equal(np.isnan(u["corr_se"]), ~live)
    np.testing.assert_allclose(u["corr_se"][live], u1["corr_se"][live], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(u["corr_asl"][live], ((r1[:, :, 3] + 1) / (r1[:, :, 2] + 1))[live])
    n_tests = int(live.sum()) - n_t                                               # (the duplicate shares its partner's tests)
    assert got.schedule == list(SCHEDULE) and got.n_open == [n_tests] * len(SCHEDULE) and n_tests == (N_DISTINCT - 1) * n_t


def test_round_0_is_the_plain_call(runs):
    u0, u, r0 = runs.plain.uns, runs.seq.uns, runs.plain.rec
    assert "corr_nboot" not in u0 and "max_boot" not in u0 and "min_extreme" not in u0 and "corr_nboot" not in runs.plain.df.columns
    _same_bits(u["corr_coef"], u0["corr_coef"])
    same = u["corr_nboot"] == NUM_BOOT
    print(f"\n{runs.mode.name}: {int(same.sum())} tests closed in round 0")
    assert same.sum() >= 30 and (r0[same][:, 3] > 10).all()
    _same_bits(u["corr_se"][same], u0["corr_se"][same], "corr_se")
    np.testing.assert_array_equal(u["corr_asl"][same], (r0[same][:, 3] + 1) / (NUM_BOOT + 1))
    _same_bits(u["corr_asl"][same], u0["corr_asl"][same], "corr_asl")             # (c > 10: the plain call's empirical p-value)
    _same_bits(runs.seq.rec[same], r0[same])


def test_stopping_invariants(runs):
    seq, one, mode = runs.seq, runs.one_shot, runs.mode
    u, rec = seq.uns, seq.rec
    assert u["max_boot"] == MAX_BOOT and u["min_extreme"] == 10
    nboot, c, p = u["corr_nboot"], rec[:, :, 3], u["corr_asl"]
    live = np.isfinite(p)
    print(f"\n{mode.name}: n_open {seq.n_open}; n_chains {seq.n_chains}; corr_nboot counts {dict(zip(*np.unique(nboot, return_counts=True)))}")
    assert nboot.dtype == np.int64 and np.isin(nboot[live], SCHEDULE).all() and (nboot[~live] == 0).all()
    np.testing.assert_array_equal(nboot[live], rec[live][:, 2])
    assert (c > 10)[live & (nboot < MAX_BOOT)].all()
    np.testing.assert_array_equal(p[live], ((c + 1) / (nboot + 1))[live])
    n_open = np.asarray(seq.n_open)
    assert len(n_open) == len(SCHEDULE) and (np.diff(n_open) <= 0).all() and 0 < n_open[-1] < n_open[0] < (N_DISTINCT - 1) * mode.n_t
    # the planted tests: the coupled pairs against guide 1 (groups: against each of its three replicate groups)
    cols = [i for i, g in enumerate(u["groups"]) if g == "1" or g.startswith("sg^1^")]
    planted = nboot[:len(COUPLED)][:, cols]
    assert len(cols) == (3 if mode.treatment_col is None else 1) and (planted > NUM_BOOT).all() and (planted == MAX_BOOT).any()
    full = live & (nboot == MAX_BOOT)                                             # the replicates behind these are the one-shot call's
    for k in (2, 3, 6):
        np.testing.assert_array_equal(rec[full][:, k], one.rec[full][:, k])
    _same_bits(u["corr_coef"], one.uns["corr_coef"])
    assert list(seq.df["corr_nboot"].values) == list(nboot.reshape(-1))


def test_degenerate_pairs(runs):
    u = runs.seq.uns
    i_first = PAIRS.index(DUP_OF)
    for k in KEYS:                                                                # the duplicate shares its pair's rows
        _same_bits(u[k][I_DUP], u[k][i_first], k)
    assert np.isfinite(u["corr_asl"][I_DUP]).all()
    for i in (I_SELF, I_NO_CTRL):
        assert np.isnan([u[k][i] for k in KEYS[:3]]).all() and (u["corr_nboot"][i] == 0).all()


def test_a_round_launches_the_chains_its_open_tests_read(runs, adata):
    """``n_chains[j]`` against the distinct chains of the designs of the tests open before round j, recomputed from the recorded
    masks; round 0 ran every active chain.  After round 0 a pair has open and closed tests, and round 1 launches fewer chains
    than all twelve groups of every pair with an open test."""
    seq, mode = runs.seq, runs.mode
    v = _view(adata, mode)
    assert seq.n_chains[0] == int(v.bs.active.sum()) and seq.open_mask[0].all() and len(seq.open_mask) == len(SCHEDULE)
    for j in range(1, len(SCHEDULE)):
        mask = seq.open_mask[j]
        assert mask.shape == v.test_pair.shape and int(mask.sum()) == seq.n_open[j - 1]
        assert seq.n_chains[j] == len(_brute_chains(v, np.flatnonzero(mask)))
    per_pair = seq.open_mask[1].reshape(N_DISTINCT, mode.n_t)
    mixed = per_pair.any(axis=1) & ~per_pair.all(axis=1)
    print(f"\n{mode.name}: pairs with an open and a closed test after round 0: {int(mixed.sum())}; with an open test: {int(per_pair.any(axis=1).sum())}")
    assert mixed.any() and 0 < seq.n_chains[1] < per_pair.any(axis=1).sum() * NG


def test_pair_chunks_change_no_number(runs, adata):
    seq = runs.seq
    got = _call(adata, runs.mode, max_boot=MAX_BOOT, max_rows=21 * NG)            # 21 pairs per chunk: three chunks, the last one short
    assert adata.uns["memento"]["_hip"].last_chunk2d == (42, N_DISTINCT)
    for k in KEYS:
        _same_bits(got.uns[k], seq.uns[k], k)
    assert list(got.df.columns) == list(seq.df.columns) and got.n_open == seq.n_open and got.n_chains == seq.n_chains
    _call(adata, runs.mode, max_boot=MAX_BOOT)                                    # (leave the one-chunk call's chunk behind, as ``runs`` did)


def test_sub_batches_change_no_number(runs, adata):
    """The continuation on the sequential call's own kept chunk and round-0 records, with a budget of seven chains in round 1
    (three, one and one in the later rounds: runs of single tests): the merged records are the call's, bit for bit."""
    from scrna_parameter_estimation_amd.memento import _ht

    mode, st = runs.mode, adata.uns["memento"]["_hip"]
    v = _view(adata, mode)
    stats0, rows = v.bs.contrast_design(v.test_pair, v.test_design, *v.tables)
    del rows
    _same_bits(stats0[:, 0], np.asarray(st.last_records2d)[:, 0])
    budget = 7 * (1 + NUM_BOOT)
    open1 = np.flatnonzero(runs.seq.open_mask[1])
    n_runs = len(_ht.design_batches(v.test_pair[open1], v.test_design[open1], v.tables[0], v.tables[1], NG, budget // (1 + NUM_BOOT)))
    assert n_runs >= 3
    n_open, n_chains, masks = [0] * len(SCHEDULE), [0] * len(SCHEDULE), [None] * len(SCHEDULE)
    got = _ht.continue_chunk_2d_designs(SimpleNamespace(bs=v.bs), NG, v.test_pair, v.test_design, v.tables, stats0, list(SCHEDULE), 10, "bootstrap",
                                        n_open, n_chains, masks, budget=budget)
    _same_bits(got, np.asarray(st.last_records2d))
    assert n_open == runs.seq.n_open and n_chains[1:] == runs.seq.n_chains[1:]
    for a, b in zip(masks[1:], runs.seq.open_mask[1:]):
        np.testing.assert_array_equal(a, b)


def test_dropped_columns_fold_into_the_one_shot_counts(runs, adata):
    """NaN replicate columns: the same (chain, global replicate) cells are NaN in a one-shot plane of 3200 replicates (the
    chunk's own layout, launch_range) and in the rounds' compact planes (design_round_tables, launch_listed), all made from the
    sequential call's kept run; engine._contrast_design -- the driver's routine -- on each and merge_records over the rounds give
    the one-shot record's counts, with n_valid < 3200 for the tests that read a poisoned chain."""
    from scrna_parameter_estimation_amd import engine
    from scrna_parameter_estimation_amd.memento import _ht

    torch = engine._torch()
    v = _view(adata, runs.mode)
    bs, (d_ptr, d_grp, d_w) = v.bs, v.tables
    tests = np.flatnonzero(np.diff(d_ptr)[v.test_design] > 0)                      # the tests with a design
    t_pair, t_design = v.test_pair[tests], v.test_design[tests]
    chains, t_ptr, t_rows, t_w = _ht.design_round_tables(t_pair, t_design, d_ptr, d_grp, d_w, NG)
    assert bs.active[chains].all() and len(chains) >= (N_DISTINCT - 1) * 4
    rng = np.random.default_rng(3)
    cells_q = np.repeat(rng.choice(chains, size=20, replace=False), 40)            # 40 NaN cells in each of 20 chains
    cells_r = rng.integers(0, MAX_BOOT, size=len(cells_q))
    cells_r[:40] = np.arange(40) * 5                                               # (one chain with NaN cells in round 0)
    active = np.flatnonzero(bs.active)

    def poison(plane, rows, rep_lo, rep_n):
        hit = (cells_r >= rep_lo) & (cells_r < rep_lo + rep_n)
        plane[engine.dev(rows[hit]), engine.dev(1 + cells_r[hit] - rep_lo)] = float("nan")

    one_plane = torch.full((bs.n_q, 1 + MAX_BOOT), float("nan"), dtype=torch.float64, device="cuda")
    one_plane[:, 0] = bs.yc[:bs.n_q, 0]
    keep = bs.launch_range(0, MAX_BOOT, active, one_plane, active)
    poison(one_plane, cells_q, 0, MAX_BOOT)
    (one,), _ = engine._contrast_design([one_plane], 1 + MAX_BOOT, MAX_BOOT, NG, bs.n_pairs, t_pair, t_design, d_ptr, d_grp, d_w)
    del keep, one_plane

    def record(rep_lo, rep_n):
        plane = torch.full((len(chains), 1 + rep_n), float("nan"), dtype=torch.float64, device="cuda")
        plane[:, 0] = bs.yc[engine.dev(chains), 0]
        keep = bs.launch_listed(rep_lo, rep_n, chains, plane, np.arange(len(chains)))
        poison(plane, np.searchsorted(chains, cells_q), rep_lo, rep_n)
        (rec,), _ = engine._contrast_design([plane], 1 + rep_n, rep_n, len(chains), 1, np.zeros(len(tests), dtype=np.int32), np.arange(len(tests)),
                                            t_ptr, t_rows, t_w)
        del keep
        return rec

    bounds = [0] + list(SCHEDULE)
    rounds = [record(lo, hi - lo) for lo, hi in zip(bounds[:-1], bounds[1:])]
    merged = _ht.merge_records(rounds)
    reads = np.array([np.isin(chains[t_rows[t_ptr[t]:t_ptr[t + 1]]], cells_q).any() for t in range(len(tests))])
    dropped = MAX_BOOT - one[:, 2]
    print(f"\n{runs.mode.name}: {int(reads.sum())} of {len(tests)} tests read a poisoned chain: dropped columns min {dropped[reads].min():.0f} "
          f"max {dropped[reads].max():.0f}")
    assert reads.sum() >= 20 and (dropped[reads] >= 30).all() and (dropped[~reads] == 0).all() and (rounds[0][reads, 2] < NUM_BOOT).any()
    for k in (2, 3, 6):
        np.testing.assert_array_equal(merged[:, k], one[:, k])
    _same_bits(merged[:, 0], one[:, 0])
    np.testing.assert_allclose(merged[:, 1], one[:, 1], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(_ht.sequential_pvalues(merged), (one[:, 3] + 1) / (one[:, 2] + 1))


def test_two_groups_equal_ht_2d_moments():
    """Exactly {control, one guide}: both calls draw the same uniforms, run the same chains under the same stream keys and see
    identical replicate rows.  ht_2d_moments forms w1 * a + w2 * b with regression weights, this call a - b, so -- as in
    tests/test_gpu_vs_control_2d.py for the plain calls -- the coefficient and the SE agree to 1e-10 and rounding may move a
    replicate across the extreme-count threshold for at most 2 % of the tests; every other test has the same replicate count
    and the same p-value."""
    from scrna_parameter_estimation_amd import memento

    adata = _adata(n_guides=2, n_rep=1)
    memento.setup_memento(adata, q_column="q", filter_mean_thresh=0.07)
    memento.create_groups(adata, label_columns=["guide"])
    memento.compute_1d_moments(adata, min_perc_group=0.7)
    memento.compute_2d_moments(adata, [(f"g{a}", f"g{b}") for a, b in PAIRS])
    m = adata.uns["memento"]
    gdf = memento.get_groups(adata)
    cov = pd.DataFrame({"intercept": np.ones(len(gdf))}, index=gdf.index)
    trt = pd.DataFrame({"is_guide": (gdf["guide"].astype(int) == 1).astype(float)}, index=gdf.index)
    np.random.seed(23)
    memento.ht_2d_moments(adata, covariate=cov, treatment=trt, num_boot=NUM_BOOT, num_cpus=1, verbose=0, resampling="bootstrap", rng="fast",
                          fill_seed=FILL_SEED, approx=False, max_boot=MAX_BOOT)
    old = {k: np.asarray(m["2d_ht"][k]).copy() for k in KEYS}
    n_open_old = list(m["_hip"].last_sequential.n_open)
    np.random.seed(23)
    df = memento.ht_2d_vs_control_sequential(adata, control="sg^0", num_boot=NUM_BOOT, num_cpus=1, rng="fast", fill_seed=FILL_SEED, approx=False,
                                  max_boot=MAX_BOOT)
    new = {k: df[c].values for k, c in zip(KEYS, ("corr_coef", "corr_se", "corr_pval", "corr_nboot"))}
    assert len(df) == len(PAIRS) and (df["group"] == "sg^1").all()
    live = np.isfinite(old["corr_asl"])
    assert live.sum() == len(PAIRS) - 1 and not live[I_SELF]
    for k in KEYS[:3]:
        np.testing.assert_array_equal(np.isnan(new[k]), ~live, err_msg=k)
    np.testing.assert_allclose(new["corr_coef"][live], old["corr_coef"][live], rtol=1e-10, atol=1e-10)
    same = live & (new["corr_nboot"] == old["corr_nboot"]) & (new["corr_asl"] == old["corr_asl"])
    print(f"\ntwo groups: {int(live.sum())} tests, {int((live & ~same).sum())} with another count; n_open {n_open_old} / "
          f"{m['_hip'].last_sequential.n_open}; corr_nboot counts {dict(zip(*np.unique(old['corr_nboot'][live], return_counts=True)))}")
    assert (live & ~same).sum() <= 0.02 * live.sum() and (new["corr_nboot"][~live] == 0).all()
    np.testing.assert_allclose(new["corr_se"][same], old["corr_se"][same], rtol=1e-10, atol=1e-10)
    assert (old["corr_nboot"][live] > NUM_BOOT).any() and (old["corr_nboot"][live] == NUM_BOOT).any()


@pytest.mark.parametrize("kw", [dict(rng="replay"), dict(approx=True), dict(ci=0.9), dict(max_boot=NUM_BOOT - 1), dict(min_extreme=-1)])
def test_argument_errors(adata, kw):
    from scrna_parameter_estimation_amd import memento

    st = adata.uns["memento"]["_hip"]
    before = st.last_bootstrap2d
    st.last_bootstrap2d = "untouched"
    args = dict(num_boot=NUM_BOOT, rng="fast", max_boot=MAX_BOOT, treatment_col="guide")
    args.update(kw)
    with pytest.raises(ValueError):
        memento.ht_2d_vs_control_sequential(adata, 0, **args)
    assert st.last_bootstrap2d == "untouched"                        # raised before the call's first device work
    st.last_bootstrap2d = before
