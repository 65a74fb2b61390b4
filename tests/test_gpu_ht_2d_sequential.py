"""GPU tests of the sequential bootstrap of the gene-pair tests: ht_2d_moments(rng='fast', max_boot=..., min_extreme=...).

6,000 cells x 150 genes in 2 conditions x 3 replicates (six groups of 1,000 cells); covariate = intercept + replicate dummies,
treatment = the condition.  61 distinct pairs: 6 whose genes share a latent factor in condition 1 only (``one_sample``: in every
cell), 54 pairs of independent well-expressed genes and one pair of sparse genes (0.3 counts per cell: some of its replicates have
a non-positive variance); a duplicate of one pair and a self pair are requested on top.  num_boot = 200, max_boot = 3200, the
schedule is (200, 400, 800, 1600, 3200); fill_seed is fixed and np.random.seed is set before every call.

The 2D path refills nothing, so the exactness statement has no premise: a test that is never closed early has the valid,
extreme and raw-extreme counts of the one-shot num_boot = 3200 call.

On dropped (NaN) replicate columns.  close_replicate_2d (csrc/boot.hip) follows estimator._corr_from_cov: where a replicate's
variance is not positive it stores the 5.0 sentinel clipped to 1.0, a FINITE number, and a chain that runs writes every column
-- so for a live test of ht_2d_moments n_valid equals the replicate count in every call, sparse pair included, and no choice
of data makes the one-shot call drop a column (measured on the data below: n_valid == 3200 for all 61 tests; the sparse pair's
rows hold sentinel replicates instead, which is asserted).  That premise of the plan for this file is therefore replaced by its
content: ``test_dropped_columns_fold_into_the_one_shot_counts`` poisons the same (chain, global replicate) cells with NaN in a
one-shot plane and in the rounds' planes made by Bootstrap2D.launch_range, contracts both with the driver's own
engine.contract_plane and asserts that the merged n_valid, n_extreme, n_raw_extreme equal the one-shot record's with
n_valid < 3200.
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
DUP_OF, SELF = OTHERS[0], (30, 30)
PAIRS = COUPLED + OTHERS + [SPARSE, DUP_OF, SELF]
I_SPARSE, I_DUP, I_SELF = len(PAIRS) - 3, len(PAIRS) - 2, len(PAIRS) - 1
N_DISTINCT = len(COUPLED) + len(OTHERS) + 1
NUM_BOOT, MAX_BOOT, FILL_SEED = 200, 3200, 17
SCHEDULE = (200, 400, 800, 1600, 3200)
KEYS = ("corr_coef", "corr_se", "corr_asl", "corr_nboot")


def _adata(one_sample, seed=5):
    from scrna_parameter_estimation_amd.anndata_lite import AnnDataLite

    rng = np.random.default_rng(seed)
    cond, rep = np.arange(N_CELLS) % 2, (np.arange(N_CELLS) // 2) % 3
    mu = rng.uniform(2.0, 6.0, size=N_GENES)
    mu[list(SPARSE)] = 0.3
    lam = mu[None, :] * rng.lognormal(0.0, 0.25, size=N_CELLS)[:, None] * rng.gamma(2.0, 0.5, size=(N_CELLS, N_GENES))
    for a, b in COUPLED:
        z = rng.lognormal(0.0, 0.5, size=N_CELLS)
        sel = np.ones(N_CELLS, dtype=bool) if one_sample else cond == 1
        lam[sel, a] *= z[sel]
        lam[sel, b] *= z[sel]
    X = sp.csr_matrix(rng.poisson(lam).astype(np.float32))
    obs = pd.DataFrame({"cond": cond, "rep": rep, "q": np.full(N_CELLS, 0.07)}, index=[f"c{i}" for i in range(N_CELLS)])
    return AnnDataLite(X, obs, pd.DataFrame(index=[f"g{i}" for i in range(N_GENES)]))


def _prepared(one_sample=False):
    from scrna_parameter_estimation_amd import memento

    adata = _adata(one_sample)
    memento.setup_memento(adata, q_column="q", filter_mean_thresh=0.07)
    memento.create_groups(adata, label_columns=["cond", "rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.7)
    assert len(adata.uns["memento"]["_hip"].gene_idx) == N_GENES
    memento.compute_2d_moments(adata, [(f"g{a}", f"g{b}") for a, b in PAIRS])
    gdf = memento.get_groups(adata)
    assert len(gdf) == 6
    cov = pd.concat([pd.DataFrame({"intercept": np.ones(len(gdf))}, index=gdf.index),
                     pd.get_dummies(gdf["rep"].astype(str), prefix="rep", drop_first=True).astype(float)], axis=1)
    trt = pd.DataFrame({"cond": np.ones(len(gdf)) if one_sample else gdf["cond"].astype(float).values}, index=gdf.index)
    return memento, adata, cov, trt


def _records(adata):
    """The test records of the call's one pair chunk (device pair order) as [requested pair][8]; NaN rows where there is no test."""
    from scrna_parameter_estimation_amd.memento import _ht

    m = adata.uns["memento"]
    st = m["_hip"]
    assert st.last_chunk2d == (0, N_DISTINCT)
    _, members = _ht.distinct_pairs(m["2d_moments"]["gene_idx_1"], m["2d_moments"]["gene_idx_2"])
    rec, order = np.asarray(st.last_records2d), st.last_bootstrap2d.order
    assert rec.shape == (N_DISTINCT, 8) and len(order) == N_DISTINCT
    out = np.full((len(PAIRS), 8), np.nan)
    for k in range(N_DISTINCT):
        out[members[int(order[k])]] = rec[k]
    return out


def _call(memento, adata, cov, trt, **kw):
    """One ht_2d_moments(rng='fast', approx=False) call from a fixed state of the global numpy stream (the chains' hash uniforms)."""
    np.random.seed(23)
    kw.setdefault("num_boot", NUM_BOOT)
    memento.ht_2d_moments(adata, covariate=cov, treatment=trt, num_cpus=1, verbose=0, resampling="bootstrap", rng="fast", fill_seed=FILL_SEED,
                          approx=False, **kw)
    m = adata.uns["memento"]
    st = m["_hip"]
    assert st.last_bootstrap2d.replay_kernel == "mm_boot2d_fast"
    uns = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in m["2d_ht"].items()}
    bs, n_sent = st.last_bootstrap2d, None
    if "max_rows" not in kw:            # the sparse pair is the last distinct pair: its sentinel replicates (exactly 1.0) in this call's rows
        k = int(np.flatnonzero(bs.order == N_DISTINCT - 1)[0])
        n_sent = int((bs.yc[k * bs.ng:(k + 1) * bs.ng, 1:] == 1.0).sum().item())
    return SimpleNamespace(uns=uns, n_sent=n_sent, df=memento.get_2d_ht_result(adata).copy(), rec=None if "max_rows" in kw else _records(adata),
                           n_open=list(st.last_sequential.n_open) if "max_boot" in kw else None,
                           schedule=list(st.last_sequential.schedule) if "max_boot" in kw else None)


@pytest.fixture(scope="module")
def prep():
    return _prepared()


@pytest.fixture(scope="module")
def one_shot(prep):
    """The one-shot 3200-replicate call (tail fits included), computed once."""
    return _call(*prep, num_boot=MAX_BOOT)


@pytest.fixture(scope="module")
def plain(prep):
    """The plain 200-replicate call."""
    return _call(*prep)


@pytest.fixture(scope="module")
def seq(prep):
    """The sequential call with the default min_extreme."""
    return _call(*prep, max_boot=MAX_BOOT)


@pytest.fixture(scope="module")
def never_closed(prep):
    """The sequential call in which nothing closes early."""
    return _call(*prep, max_boot=MAX_BOOT, min_extreme=MAX_BOOT + 1)


def _same_bits(a, b, what=""):
    np.testing.assert_array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64), err_msg=what)


def _exactness(one, got):
    """``got``: a sequential call in which nothing closes early, against the one-shot call with max_boot replicates, every test."""
    r1, r, u1, u = one.rec, got.rec, one.uns, got.uns
    live = np.isfinite(r1[:, 0])
    n_tests = int(live.sum())
    print(f"\n{n_tests} live tests of {len(PAIRS)} requested pairs; one-shot n_valid min {r1[live, 2].min():.0f} max {r1[live, 2].max():.0f}; "
          f"extreme counts <= 10: {int((r1[live, 3] <= 10).sum())}; n_open {got.n_open}")
    assert n_tests == len(PAIRS) - 1 and not live[I_SELF]                         # every pair but the self pair has a test
    n_distinct_tests = n_tests - 1                                                # (the duplicate shares its partner's test)
    assert "corr_nboot" not in u1 and "max_boot" not in u1 and "corr_nboot" not in one.df.columns
    assert u["max_boot"] == MAX_BOOT and u["min_extreme"] == MAX_BOOT + 1 and list(got.df.columns)[-1] == "corr_nboot"
    for k in (2, 3, 6):                                                           # n_valid, n_extreme, n_raw_extreme
        np.testing.assert_array_equal(r[:, k], r1[:, k])
    # (a chain that runs writes a finite number into every replicate column -- see the module docstring: nothing is dropped)
    assert (r1[live, 2] == MAX_BOOT).all()
    np.testing.assert_array_equal(u["corr_nboot"], np.where(live, r1[:, 2], 0).astype(np.int64))
    np.testing.assert_array_equal(got.df["corr_nboot"].values, u["corr_nboot"])
    _same_bits(u["corr_coef"], u1["corr_coef"], "corr_coef")
    np.testing.assert_array_equal(np.isnan(u["corr_se"]), ~live)
    np.testing.assert_allclose(u["corr_se"][live], u1["corr_se"][live], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(u["corr_asl"][live], ((r1[:, 3] + 1) / (r1[:, 2] + 1))[live])
    assert np.isnan(u["corr_asl"][~live]).all()
    emp = live & (r1[:, 3] > 10)                                                  # where the one-shot call took the empirical branch
    assert emp.sum() >= 30
    _same_bits(u["corr_asl"][emp], u1["corr_asl"][emp], "corr_asl")
    assert got.schedule == list(SCHEDULE) and got.n_open == [n_distinct_tests] * len(SCHEDULE) and n_distinct_tests == N_DISTINCT
    return live


def test_nothing_closes_early_is_the_one_shot_call(prep, one_shot, never_closed):
    live = _exactness(one_shot, never_closed)
    # the sparse pair: some of its replicates have a non-positive variance -- the clipped 5.0 sentinel, a finite 1.0
    print(f"sparse pair: {one_shot.n_sent} sentinel replicates among its 6 x {MAX_BOOT} of the one-shot call")
    assert live[I_SPARSE] and one_shot.n_sent >= 1


def test_treatment_for_gene_gives_the_same_bits(prep, one_shot, never_closed):
    memento, adata, cov, trt = prep
    tfg = {frozenset({f"g{g}"}): ["cond"] for g in range(N_GENES)}
    got = _call(memento, adata, cov, trt, max_boot=MAX_BOOT, min_extreme=MAX_BOOT + 1, treatment_for_gene=tfg)
    _exactness(one_shot, got)
    assert "treatment_for_gene" in got.uns
    for k in KEYS:
        _same_bits(got.uns[k], never_closed.uns[k], k)
    _same_bits(got.rec, never_closed.rec)


def test_round_0_is_the_plain_call(plain, seq):
    u0, u = plain.uns, seq.uns
    assert "corr_nboot" not in u0 and "max_boot" not in u0 and "min_extreme" not in u0 and "corr_nboot" not in plain.df.columns
    _same_bits(u["corr_coef"], u0["corr_coef"])
    same = (u["corr_nboot"] == NUM_BOOT) & (plain.rec[:, 3] > 10)
    print(f"\n{int(same.sum())} tests closed in round 0 on the empirical branch")
    assert same.sum() >= 30
    for k in ("corr_se", "corr_asl"):
        _same_bits(u[k][same], u0[k][same], k)
    _same_bits(seq.rec[same], plain.rec[same])


def test_stopping_invariants(seq, one_shot):
    u, rec = seq.uns, seq.rec
    assert u["max_boot"] == MAX_BOOT and u["min_extreme"] == 10
    nboot, c, p = u["corr_nboot"], rec[:, 3], u["corr_asl"]
    live = np.isfinite(p)
    n_tests = int(live.sum())
    print(f"\nn_open {seq.n_open}; corr_nboot counts {dict(zip(*np.unique(nboot[live], return_counts=True)))}")
    assert n_tests == len(PAIRS) - 1
    distinct = np.arange(len(PAIRS)) != I_DUP
    np.testing.assert_array_equal(nboot[live], rec[live, 2])
    assert np.isin(nboot[live], SCHEDULE).all() and ((c > 10) | (nboot == MAX_BOOT))[live].all()
    np.testing.assert_array_equal(p[live], ((c + 1) / (nboot + 1))[live])
    assert (nboot[live] == NUM_BOOT).sum() >= 1                                   # closed in round 0
    ran_out = live & (nboot == MAX_BOOT) & (c <= 10)
    assert ran_out.sum() >= 1 and ran_out[:len(COUPLED)].any()
    n_open = np.asarray(seq.n_open)
    assert len(n_open) == len(SCHEDULE) and (np.diff(n_open) <= 0).all() and 0 < n_open[-1] < n_open[0] < N_DISTINCT
    assert n_open[-1] == (ran_out & distinct).sum()
    full = live & (nboot == MAX_BOOT)                                             # the replicates behind these are the one-shot call's
    for k in (2, 3, 6):
        np.testing.assert_array_equal(rec[full, k], one_shot.rec[full, k])
    _same_bits(u["corr_coef"], one_shot.uns["corr_coef"])
    i_first = PAIRS.index(DUP_OF)
    for k in KEYS:                                                                # the duplicate shares its partner's row
        _same_bits(u[k][I_DUP], u[k][i_first], k)
    assert live[I_DUP] and np.isnan([u[k][I_SELF] for k in KEYS[:3]]).all() and nboot[I_SELF] == 0
    assert list(seq.df["corr_nboot"].values) == list(nboot) and nboot.dtype == np.int64


def test_one_sample_test():
    """Treatment all ones, the six coupled pairs coupled in every cell: the weighted-average branch of the design."""
    prep1 = _prepared(one_sample=True)
    one = _call(*prep1, num_boot=MAX_BOOT)
    got = _call(*prep1, max_boot=MAX_BOOT, min_extreme=MAX_BOOT + 1)
    _exactness(one, got)
    c, p = got.rec[:len(COUPLED), 3], got.uns["corr_asl"][:len(COUPLED)]
    print(f"coupled pairs: extreme counts {c.tolist()}")
    assert (c <= 10).any() and (got.uns["corr_nboot"][:len(COUPLED)] == MAX_BOOT).all()
    np.testing.assert_array_equal(p, (c + 1) / 3201)


def test_pair_chunks_change_no_number(prep, seq):
    memento, adata, cov, trt = prep
    ng = len(adata.uns["memento"]["groups"])
    got = _call(memento, adata, cov, trt, max_boot=MAX_BOOT, max_rows=25 * ng)    # 25 pairs per chunk: three chunks, the last one short
    assert adata.uns["memento"]["_hip"].last_chunk2d == (50, N_DISTINCT)
    for k in KEYS:
        _same_bits(got.uns[k], seq.uns[k], k)
    assert list(got.df.columns) == list(seq.df.columns) and got.n_open == seq.n_open


def test_dropped_columns_fold_into_the_one_shot_counts(prep):
    """NaN replicate columns (see the module docstring): the same (chain, global replicate) cells are NaN in a one-shot plane of
    3200 replicates and in the rounds' planes, all made by launch_range from one kept run; engine.contract_plane on each and
    merge_records over the rounds give the one-shot record's counts, with n_valid < 3200 for the poisoned tests."""
    from scrna_parameter_estimation_amd import engine
    from scrna_parameter_estimation_amd.memento import _ht

    memento, adata, cov, trt = prep
    _call(memento, adata, cov, trt, max_boot=NUM_BOOT)                             # one round; keeps the operands and the streams
    torch = engine._torch()
    bs = adata.uns["memento"]["_hip"].last_bootstrap2d
    ng, n_pairs = bs.ng, bs.n_pairs
    good = bs.active.reshape(n_pairs, ng)
    chains = np.flatnonzero(bs.active)
    rng = np.random.default_rng(3)
    W = rng.normal(size=(n_pairs, ng))
    poisoned = rng.choice(np.flatnonzero(good.all(axis=1)), size=20, replace=False)
    cells_q = np.repeat(poisoned * ng + rng.integers(0, ng, size=20), 40)          # 40 NaN cells in one chain of each poisoned pair
    cells_r = rng.integers(0, MAX_BOOT, size=len(cells_q))
    cells_r[:40] = np.arange(40) * 5                                               # (one pair with NaN cells in round 0)
    col0 = bs.yc[:bs.n_q, 0].clone()

    def record(rep_lo, rep_n):
        plane = torch.full((bs.n_q, 1 + rep_n), float("nan"), dtype=torch.float64, device="cuda")
        plane[:, 0] = col0
        keep = bs.launch_range(rep_lo, rep_n, chains, plane, chains)
        hit = (cells_r >= rep_lo) & (cells_r < rep_lo + rep_n)
        plane[engine.dev(cells_q[hit]), engine.dev(1 + cells_r[hit] - rep_lo)] = float("nan")
        _, rec = engine.contract_plane(plane, 1 + rep_n, rep_n, ng, n_pairs, np.arange(n_pairs), W, good)
        del keep
        return rec

    one = record(0, MAX_BOOT)
    bounds = [0] + list(SCHEDULE)
    rounds = [record(lo, hi - lo) for lo, hi in zip(bounds[:-1], bounds[1:])]
    merged = _ht.merge_records(rounds)
    live = good.any(axis=1)
    hit = np.isin(np.arange(n_pairs), poisoned)
    dropped = MAX_BOOT - one[:, 2]
    print(f"\n{int(hit.sum())} poisoned tests: dropped columns min {dropped[hit].min():.0f} max {dropped[hit].max():.0f}")
    assert live.all() and (dropped[hit] >= 30).all() and (dropped[hit] <= 40).all() and (dropped[~hit] == 0).all()
    assert (rounds[0][hit, 2] < NUM_BOOT).any()
    for k in (2, 3, 6):
        np.testing.assert_array_equal(merged[:, k], one[:, k])
    _same_bits(merged[:, 0], one[:, 0])
    np.testing.assert_allclose(merged[:, 1], one[:, 1], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(_ht.sequential_pvalues(merged), (one[:, 3] + 1) / (one[:, 2] + 1))


@pytest.mark.parametrize("kw", [dict(rng="replay"), dict(approx=True), dict(ci=0.95), dict(resample_rep=True), dict(max_boot=NUM_BOOT - 1),
                                dict(min_extreme=-1)])
def test_argument_errors(prep, kw):
    memento, adata, cov, trt = prep
    st = adata.uns["memento"]["_hip"]
    st.last_bootstrap2d = "untouched"
    args = dict(num_boot=NUM_BOOT, rng="fast", max_boot=MAX_BOOT, resampling="bootstrap")
    args.update(kw)
    with pytest.raises(ValueError):
        memento.ht_2d_moments(adata, covariate=cov, treatment=trt, **args)
    assert st.last_bootstrap2d == "untouched"                        # raised before the call's first device work
    st.last_bootstrap2d = None
