"""GPU parity tests of the individual HIP kernels (through the C-ABI) against the CPU oracle.

Integer / index results must be bit-exact; fp64 moment sums within 1e-12 relative (the summation
order differs from scipy's); replay-bootstrap weights bit-exact vs numpy; replicate moments to ~1 ulp
(numpy's pairwise summation over bins is not reproduced).
"""

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import golden_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import memento_oracle

    return memento_oracle


def _decode_blocks(eng, blocks):
    """SELL blocks -> list of (orig_cell, gene, count) triples (host), for exactness checks."""
    ent = eng.host(blocks.ent, np.uint32)
    perm = eng.host(blocks.perm)
    sw = eng.host(blocks.slice_w)
    sp_ = eng.host(blocks.slice_ptr)
    base = eng.host(blocks.blk_base)
    out = []
    for b in range(blocks.n_blocks):
        c0 = blocks.blk_cell0[b]
        for t in range(blocks.n_slices):
            w = sw[b, t]
            if w == 0:
                continue
            rows = ent[(base[b] + sp_[b, t]) * 256:(base[b] + sp_[b, t] + w) * 256].reshape(w, 64, 4)
            for lane in range(64):
                g = perm[b, t * 64 + lane]
                e = rows[:, lane, :].reshape(-1)
                e = e[e != 0]
                if len(e):
                    assert g >= 0
                    cells = blocks.cell_order[c0 + (e & 8191)]
                    out.append(np.stack([cells, np.full(len(e), g), e >> 13], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int64)


def _small_problem(seed=0, n=3000, g=300, density=0.08, ngroups=5):
    from scrna_parameter_estimation_amd.synth import synth_counts

    X = synth_counts(n, g, density, seed, dtype=np.float32)
    rng = np.random.default_rng(seed)
    gid = rng.integers(-1, ngroups, size=n).astype(np.int32)  # -1 = cell in no group
    sf = rng.lognormal(0, 0.3, size=n)
    return X, gid, ngroups, sf


def test_rowsum(eng):
    X, gid, ng, sf = _small_problem()
    csr = eng.DeviceCSR(X)
    np.testing.assert_array_equal(csr.rowsum(), np.asarray(X.sum(axis=1)).ravel().astype(np.float64))
    mask = np.random.default_rng(1).random(X.shape[1]) < 0.3
    np.testing.assert_array_equal(csr.rowsum(mask), np.asarray(X[:, mask].sum(axis=1)).ravel().astype(np.float64))


@pytest.mark.parametrize("shape", [(3000, 300, 0.08, 5), (20000, 130, 0.3, 2), (500, 70, 0.02, 7), (9000, 64, 0.9, 1), (2500, 1100, 0.5, 2), (700, 1024, 0.05, 2), (700, 2049, 0.03, 3),
                                   (300, 1, 0.6, 1)])
def test_ingest_roundtrip(eng, shape):
    n, g, dens, ngr = shape
    X, gid, ng, sf = _small_problem(seed=n, n=n, g=g, density=dens, ngroups=ngr)
    blocks = eng.CountBlocks(eng.DeviceCSR(X), gid, ng)
    trip = _decode_blocks(eng, blocks)
    Xs = X[gid >= 0].tocoo()
    sel = np.flatnonzero(gid >= 0)
    want = np.stack([sel[Xs.row], Xs.col, Xs.data.astype(np.int64)], axis=1)
    key = lambda a: a[np.lexsort((a[:, 1], a[:, 0]))]
    np.testing.assert_array_equal(key(trip.astype(np.int64)), key(want.astype(np.int64)))
    assert blocks.nnz_sel == len(want)
    # blocks hold one group each and at most 8192 cells
    assert np.diff(blocks.blk_cell0).max() <= 8192
    grp_sorted = gid[blocks.cell_order]
    for b in range(blocks.n_blocks):
        assert (grp_sorted[blocks.blk_cell0[b]:blocks.blk_cell0[b + 1]] == blocks.blk_group[b]).all()


def test_ingest_rejects_bad_counts(eng):
    X, gid, ng, sf = _small_problem()
    X = X.copy()
    X.data[5] = 2.5
    with pytest.raises(ValueError):
        eng.CountBlocks(eng.DeviceCSR(X), gid, ng)


@pytest.mark.parametrize("shape", [(3000, 300, 0.08, 5), (20000, 130, 0.3, 2), (9000, 64, 0.9, 1)])
def test_moments_vs_oracle(eng, orc, shape):
    n, g, dens, ngr = shape
    X, gid, ng, sf = _small_problem(seed=n + 1, n=n, g=g, density=dens, ngroups=ngr)
    blocks = eng.CountBlocks(eng.DeviceCSR(X), gid, ng)
    S, sumx, maxx = blocks.moments(1.0 / sf)
    X64 = X.astype(np.float64)
    for k in range(ng):
        sel = np.flatnonzero(gid == k)
        Xg = X64[sel].tocsc()
        w = 1.0 / sf[sel]
        np.testing.assert_allclose(S[0, k], Xg.T.dot(w), rtol=1e-12)
        np.testing.assert_allclose(S[1, k], Xg.power(2).T.dot(w ** 2), rtol=1e-12)
        np.testing.assert_allclose(S[2, k], Xg.T.dot(w ** 2), rtol=1e-12)
        np.testing.assert_array_equal(sumx[k], np.asarray(Xg.sum(axis=0)).ravel().astype(np.uint64))
        np.testing.assert_array_equal(maxx[k], np.asarray(Xg.max(axis=0).todense()).ravel().astype(np.uint32))
        q = 0.07
        m, v = orc.moments_1d_sparse(Xg, sf[sel], q)
        nobs = len(sel)
        mean = S[0, k] / nobs
        var = S[1, k] / nobs - (1 - q) * S[2, k] / nobs - mean ** 2
        np.testing.assert_allclose(mean, m, rtol=1e-12)
        np.testing.assert_allclose(var, v, rtol=1e-9, atol=1e-13)


def _boot_setup(eng, orc, g, num_boot, dump):
    X, gid, ng, q = golden_inputs(g)
    keep = np.flatnonzero(g["overall_gene_filter"])
    blocks = eng.CountBlocks(eng.DeviceCSR(X), gid, ng)
    S, sumx, maxx = blocks.moments(1.0 / g["size_factor"])
    approx, bidx, means = orc.bin_size_factor(g["size_factor"])
    # dedicated bin for the max-size-factor cell(s) (main.py:146-147)
    sf_table = np.concatenate([np.nan_to_num(means, nan=1.0), [g["size_factor"].max()]])
    bins = bidx.astype(np.uint8)
    bins[g["size_factor"] == g["size_factor"].max()] = len(means)
    np.testing.assert_array_equal(sf_table[bins], g["approx_sf"])
    bs = eng.Bootstrap1D(blocks, keep, maxx, bins, sf_table, g["group_q"], num_boot)
    return X, gid, ng, keep, blocks, bs, sf_table, bins


def test_bins_exact(eng, orc, api_small):
    g = api_small
    X, gid, ng, keep, blocks, bs, sf_table, bins = _boot_setup(eng, orc, g, 16, False)
    Xc = X.tocsc()
    for gs in [0, 3, 17, len(keep) - 1]:
        col = np.asarray(Xc[:, keep[gs]].todense()).ravel()
        for k in range(ng):
            sel = np.flatnonzero(gid == k)
            _, _, expr, mult = orc.unique_bins_1d(col[sel], g["approx_sf"][sel], 0.37, 0.61)
            asf = 1.0 / orc.unique_bins_1d(col[sel], g["approx_sf"][sel], 0.37, 0.61)[0]
            want = sorted(zip(np.round(asf, 12).tolist(), expr.astype(int).tolist(), mult.tolist()))
            bi, xi, mu = bs.bins_of_pair(gs * ng + k)
            got = sorted(zip(np.round(sf_table[bi], 12).tolist(), xi.tolist(), mu.tolist()))
            assert got == want
            assert bs.K[gs * ng + k] == len(want)


@pytest.mark.parametrize("caps", [(1024, 8192), (0, 8192), (0, 0)], ids=["small-kernel", "big-kernel", "host"])
@pytest.mark.parametrize("fast", [False, True], ids=["records", "planes"])
def test_hash_collision_is_reported(eng, monkeypatch, caps, fast):
    """With r1 == r0 == 0.25 the code of a bin is 0.25 * (x + sf) exactly, so bins with equal x + sf collide, which np.unique would
    merge -- among them (count 2, sf 1) and (count 1, sf 2) at 0.75, which the two forced cells guarantee for gene 0 whatever the
    Poisson draw gives: every ordering path must report it, whether the chains take records (replay: few chains, one per wave) or
    planes (fast) -- NotImplementedError from the status word; nothing faults."""
    rng = np.random.default_rng(5)
    n = 200
    X = rng.poisson(0.7, size=(n, 2)).astype(np.int64)
    sf_bin = rng.integers(0, 4, size=n).astype(np.uint8)
    X[10, 0], sf_bin[10] = 2, 0
    X[20, 0], sf_bin[20] = 1, 1
    sf_table = np.array([1.0, 2.0, 3.0, 4.0])
    blocks = eng.CountBlocks(eng.DeviceCSR(sp.csr_matrix(X.astype(np.float32))), np.zeros(n, dtype=np.int32), 1)
    _, _, maxx = blocks.moments(np.ones(n))
    bs = eng.Bootstrap1D(blocks, np.arange(2), maxx, sf_bin, sf_table, np.full(1, 0.1), 8)
    monkeypatch.setattr(eng, "ORDER_SMALL_CAP", caps[0])
    monkeypatch.setattr(eng, "ORDER_BIG_CAP", caps[1])
    skip, zeros = np.zeros(2, dtype=bool), np.zeros(2)
    bs.alloc_outputs(zeros, zeros)
    r1, r0 = rng.random((2, 2))
    bs.run(skip, r1, r0, [0.0, 1.0, 0.0], fast=fast)                                # generic multipliers: no collision
    assert np.isfinite(eng.host(bs.ym)).all()
    path = "small" if caps[0] else "big" if caps[1] else "host"
    assert bs.order_path[path] == 2 and sum(bs.order_path.values()) == 2
    np.testing.assert_array_equal((bs.pair_slot & eng.CHAIN_SLOT) != 0, np.full(2, not fast))      # records / planes
    with pytest.raises(NotImplementedError):
        bs.run(skip, np.full(2, 0.25), np.full(2, 0.25), [0.0, 1.0, 0.0], fast=fast)


def test_replay_bootstrap_bit_exact(eng, orc, api_small):
    g = api_small
    B = 40
    X, gid, ng, keep, blocks, bs, sf_table, bins = _boot_setup(eng, orc, g, B, True)
    rng = np.random.default_rng(7)
    r1, r0 = rng.random(bs.n_pairs), rng.random(bs.n_pairs)
    skip = np.zeros(bs.n_pairs, dtype=bool)
    skip[5] = True
    zeros = np.zeros(bs.n_pairs)
    bs.alloc_outputs(zeros, zeros)
    bs.run(skip, r1, r0, g["mv_regressor"], fill_mode=1, dump_weights=True)
    rm, rv = eng.host(bs.raw_mean), eng.host(bs.raw_var)
    Xc = X.tocsc()
    checked = 0
    for p in range(0, bs.n_pairs, 7):
        gs, k = divmod(p, ng)
        sel = np.flatnonzero(gid == k)
        col = np.asarray(Xc[:, keep[gs]].todense()).ravel()[sel]
        inv_sf, inv_sf_sq, expr, mult = orc.unique_bins_1d(col, g["approx_sf"][sel], r1[p], r0[p])
        if skip[p] or len(expr) <= 1:
            assert np.isnan(rm[p, 1:]).all()
            continue
        w = orc.multinomial_weights(len(sel), mult, B)
        np.testing.assert_array_equal(bs.weights_of(p), w)                 # integer draws: bit-exact vs numpy
        m, v = orc.replicate_moments_1d(expr, inv_sf, inv_sf_sq, w, len(sel), g["group_q"][k])
        # numpy sums the K bins pairwise (the weights are a transposed view, so the bin axis is contiguous);
        # the kernel accumulates sequentially in fp64: equal to ~1 ulp, far inside the 1e-5 bar.
        np.testing.assert_allclose(rm[p, 1:], m, rtol=1e-14)
        np.testing.assert_allclose(rv[p, 1:], v, rtol=1e-11, atol=1e-15)
        checked += 1
    assert checked > 10
    assert np.isnan(rm[5, 1:]).all()


def test_fill_log_and_contract(eng, orc, api_small):
    g = api_small
    B = 200
    X, gid, ng, keep, blocks, bs, sf_table, bins = _boot_setup(eng, orc, g, B, True)
    rng = np.random.default_rng(11)
    r1, r0 = rng.random(bs.n_pairs), rng.random(bs.n_pairs)
    tm = np.log(g["mean"].T.reshape(-1))
    tv = np.log(g["res_var"].T.reshape(-1))
    skip = ~(np.isfinite(tm) & np.isfinite(tv))
    bs.alloc_outputs(tm, tv)
    n_inv = bs.run(skip, r1, r0, g["mv_regressor"], fill_mode=1, dump_weights=True)
    rm, rv = eng.host(bs.raw_mean), eng.host(bs.raw_var)
    ym, yv = eng.host(bs.ym), eng.host(bs.yv)
    for p in range(bs.n_pairs):
        if not bs.active[p]:
            continue
        res = orc.residual_variance(rm[p, 1:], rv[p, 1:], g["mv_regressor"])
        with np.errstate(invalid="ignore", divide="ignore"):
            want_m = np.where(rm[p, 1:] > 0, np.log(rm[p, 1:]), np.nan)
            want_v = np.where(res > 0, np.log(res), np.nan)
        np.testing.assert_allclose(ym[p, 1:], want_m, rtol=1e-13, equal_nan=True)
        np.testing.assert_allclose(yv[p, 1:], want_v, rtol=1e-9, atol=1e-12, equal_nan=True)
        assert n_inv[p, 0] == np.isnan(want_m).sum() and n_inv[p, 1] == np.isnan(want_v).sum()
    # contraction vs the oracle's regression on the same (unfilled) matrices; NaN columns get dropped
    cov, trt = g["covariate"], g["treatment"]
    Nc = g["group_ncells"].astype(np.float64)
    from scrna_parameter_estimation_amd.memento import design

    good = (bs.active & (n_inv[:, 0] >= 0) & (n_inv[:, 1] >= 0)).reshape(-1, ng)
    genes = [gs for gs in range(bs.n_tested) if good[gs].any()]
    W = np.stack([design.weight_rows(cov, trt, Nc, good[gs])[0] for gs in genes])
    for which in (0, 1):
        coef, stats = bs.contract(genes, W, good, which)
        coef = eng.host(coef)
        for i, gs in enumerate(genes[:25]):
            rows = np.arange(gs * ng, gs * ng + ng)[good[gs]]
            out = orc.regress_1d(cov[good[gs]], trt[good[gs]], ym[rows], yv[rows], Nc[good[gs]], resampling="bootstrap", approx=False)
            c0, se = (out[0], out[1]) if which == 0 else (out[3], out[4])
            np.testing.assert_allclose(stats[i, 0], c0[0], rtol=1e-9, atol=1e-13)
            np.testing.assert_allclose(stats[i, 1], se[0], rtol=1e-9)
            ok = np.all(np.isfinite(ym[rows]), axis=0) & np.all(np.isfinite(yv[rows]), axis=0)
            assert stats[i, 2] == ok[1:].sum()
            assert np.array_equal(np.isnan(coef[i]), ~ok)


def test_pcg64_stream_table_equals_numpy(eng):
    """mm_pcg64_stream (lane-parallel jump-ahead): the table every lane of the tile kernel reads its uniforms from is numpy's
    Generator(PCG64(5)).random() stream, double for double -- also across the 64-output runs of the generating threads."""
    n = 300_001
    t = eng.pcg64_stream_table(5, n)
    np.testing.assert_array_equal(eng.host(t)[:n], np.random.Generator(np.random.PCG64(5)).random(n))
    t7 = eng.pcg64_stream_table(7, 1000)
    np.testing.assert_array_equal(eng.host(t7)[:1000], np.random.Generator(np.random.PCG64(7)).random(1000))
