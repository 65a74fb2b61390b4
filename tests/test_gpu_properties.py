"""Size-independent properties of the HIP path at BASELINE.json's full sizes -- configs[1] (C2: 100k cells x 20k genes,
5 % nnz, 8 groups) and configs[2], the shape the metric is quoted on (C3: 1M cells x 20k genes, 3 % nnz, 20 groups) -- where
the oracle would take too long: invariants the domain offers."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["C2", "C3"])
def big(request):
    import gc

    import torch

    import bench
    from scrna_parameter_estimation_amd import engine

    cfg = dict(bench.CONFIGS[request.param])
    ng = cfg["n_cond"] * cfg["n_rep"]
    csr = bench.synth_device_csr(cfg, 77, torch)
    rng = np.random.default_rng(5)
    gid = rng.integers(-1, ng, size=cfg["cells"]).astype(np.int32)          # -1: cells outside every group
    blocks = engine.CountBlocks(csr, gid, ng)
    sf = rng.lognormal(0, 0.3, size=cfg["cells"])
    yield engine, torch, csr, gid, blocks, sf
    del csr, blocks
    gc.collect()
    torch.cuda.empty_cache()


def test_ingest_conserves_counts(big):
    engine, torch, csr, gid, blocks, sf = big
    # every selected non-zero lands in exactly one block entry: nnz and total counts are conserved
    rows = torch.repeat_interleave(torch.arange(csr.shape[0], device="cuda"), csr.indptr[1:] - csr.indptr[:-1])
    sel = torch.from_numpy(gid >= 0).cuda()[rows]
    assert blocks.nnz_sel == int(sel.sum().item())
    ent = blocks.ent.view(torch.int32)
    x = (ent >> 13) & 0x7FFFF
    assert int((x != 0).sum().item()) == blocks.nnz_sel
    assert int(x.to(torch.int64).sum().item()) == int(csr.data[sel].to(torch.int64).sum().item())
    # padding stays below 6 % of the stored entries
    assert blocks.total_rows * 256 <= 1.06 * blocks.nnz_sel + 256 * blocks.n_blocks * blocks.n_slices


def test_ingest_is_bit_identical_and_cell_ordered_at_scale(big):
    """Two ingests of one CSR give the same count blocks bit for bit: no entry is placed by arrival order (row masks + popcount
    ranks) and the layout breaks ties between genes of equal length by gene id.  Inside a gene the entries ascend in the cell
    index -- checked on 600 random (block, gene) runs of the full-size blocks."""
    engine, torch, csr, gid, blocks, sf = big
    again = engine.CountBlocks(csr, gid, blocks.n_groups)
    assert blocks.ranged and again.ranged and blocks.total_rows == again.total_rows
    np.testing.assert_array_equal(blocks.blk_cnt, again.blk_cnt)
    assert torch.equal(blocks.slice_w, again.slice_w) and torch.equal(blocks.slice_ptr, again.slice_ptr)
    assert torch.equal(blocks.rank, again.rank) and torch.equal(blocks.perm, again.perm) and torch.equal(blocks.ent, again.ent)
    # ties by gene id: among genes of equal length in a block the ranks ascend with the gene id
    rk, cn = engine.host(blocks.rank)[0], blocks.blk_cnt[0]
    order = np.lexsort((np.arange(len(cn)), -cn.astype(np.int64)))
    np.testing.assert_array_equal(rk[order], np.arange(len(cn)))

    def run_of(bl, b, g, n):
        sl = int(bl.rank[b, g].item())
        r0 = int(engine.host(bl.blk_base)[b]) + int(bl.slice_ptr[b, sl >> 6].item())
        w = (n + 3) // 4
        e = bl.ent[r0 * 256:(r0 + w) * 256].view(torch.int32).reshape(w, 64, 4)[:, sl & 63, :].reshape(-1)
        return e[:n], e[n:]

    rng = np.random.default_rng(9)
    checked = 0
    for _ in range(600):
        b = int(rng.integers(blocks.n_blocks))
        nz = np.flatnonzero(blocks.blk_cnt[b] > 0)
        g = int(nz[rng.integers(len(nz))])
        n = int(blocks.blk_cnt[b, g])
        e1, pad1 = run_of(blocks, b, g, n)
        e2, _ = run_of(again, b, g, n)
        assert torch.equal(e1, e2) and bool((e1 != 0).all()) and bool((pad1 == 0).all())
        cell = (e1 & 8191).long()
        assert bool((cell[1:] > cell[:-1]).all())
        checked += n
    assert checked > 20_000
    del again


def test_moments_scaling_linearity_and_determinism(big):
    engine, torch, csr, gid, blocks, sf = big
    S, sumx, maxx = blocks.moments(1.0 / sf)
    S2, sumx2, maxx2 = blocks.moments(1.0 / sf)
    assert np.array_equal(S, S2) and np.array_equal(sumx, sumx2)          # fixed reduction order: bitwise repeatable
    c = 4.0                                                                # power of two: exact scaling
    Sc, _, _ = blocks.moments(1.0 / (sf * c))
    np.testing.assert_array_equal(Sc[0], S[0] / c)
    np.testing.assert_array_equal(Sc[1], S[1] / c ** 2)
    np.testing.assert_array_equal(Sc[2], S[2] / c ** 2)
    # sum over groups of sum_x equals the column sums of the selected rows; max over groups = column max
    rows = torch.repeat_interleave(torch.arange(csr.shape[0], device="cuda"), csr.indptr[1:] - csr.indptr[:-1])
    sel = torch.from_numpy(gid >= 0).cuda()[rows]
    colsum = torch.zeros(csr.shape[1], dtype=torch.float64, device="cuda").index_add_(0, csr.indices[sel].long(), csr.data[sel].double())
    np.testing.assert_array_equal(sumx.sum(axis=0), colsum.cpu().numpy().astype(np.uint64))
    # unit weights: S1 == sum x, S2 >= S1 with equality iff every count is 1, S3 == S1
    S1u, _, _ = blocks.moments(np.ones(csr.shape[0]))
    np.testing.assert_array_equal(S1u[0], sumx.astype(np.float64))
    np.testing.assert_array_equal(S1u[2], sumx.astype(np.float64))
    assert (S1u[1] >= S1u[0]).all() and ((S1u[1] == S1u[0]) == (maxx <= 1)).all()


def test_histograms_and_multinomial_invariants(big):
    engine, torch, csr, gid, blocks, sf = big
    S, sumx, maxx = blocks.moments(1.0 / sf)
    rng = np.random.default_rng(9)
    genes = np.sort(rng.choice(np.flatnonzero(sumx.sum(axis=0) > 2000), size=300, replace=False))
    n_bins = 31
    sf_bin = rng.integers(0, n_bins, size=csr.shape[0]).astype(np.uint8)
    sf_table = np.linspace(0.4, 2.5, n_bins)
    B = 64
    ng = blocks.n_groups
    bs = engine.Bootstrap1D(blocks, genes, maxx, sf_bin, sf_table, np.full(ng, 0.07), B)
    Nc = blocks.grp_ncells
    for p in rng.choice(bs.n_pairs, size=40, replace=False):
        bi, xi, mu = bs.bins_of_pair(int(p))
        g = int(p % ng)
        assert mu.sum() == Nc[g]                                           # bins partition the group's cells
        assert (mu[xi > 0] * xi[xi > 0]).sum() == sumx[g, genes[p // ng]]  # and carry the gene's total count
        assert xi.max() == maxx[g, genes[p // ng]]
    r = rng.random((2, bs.n_pairs))
    zeros = np.zeros(bs.n_pairs)
    bs.alloc_outputs(zeros, zeros)
    bs.run(np.zeros(bs.n_pairs, bool), r[0], r[1], [0.0, 1.0, 0.0], fill_mode=1, dump_weights=True)
    # multinomial weights of every replicate sum to N_g and are non-negative, whichever kernel drew them
    n_seen = 0
    if bs.n_tiles:                                                         # lock-step tiles: [slot][k][B] int32 on device
        w = bs.w_dump
        act = np.flatnonzero(bs.slot_pair >= 0)
        assert (w.sum(dim=1).cpu().numpy()[act] == Nc[bs.slot_pair[act] % ng][:, None]).all() and (w >= 0).all().item()
        n_seen += len(act)
    for wd, pairs, rows in ((bs.w_dump_chain, bs.chain_pairs, None), (bs.w_dump_async, bs.async_pairs, getattr(bs, "async_slot", None))):
        if len(pairs):                                                     # one chain per wave / lane-asynchronous tiles
            tot = wd.sum(dim=1).cpu().numpy()
            assert (tot[rows if rows is not None else slice(None)] == Nc[pairs % ng][:, None]).all() and (wd >= 0).all().item()
            n_seen += len(pairs)
    assert n_seen == int(bs.active.sum())
    # replicate means are non-negative and finite; bootstrap mean of the replicate means is close to the estimate
    rm = engine.host(bs.raw_mean)[:, 1:]
    assert np.isfinite(rm[bs.active]).all() and (rm[bs.active] >= 0).all()


def test_replay_is_independent_of_the_packing(big, monkeypatch):
    """The same chains packed as > 2048 single-chain tiles (many-tile regime: the 3-waves-per-SIMD kernel variant, tiles in
    several rounds) and as the default wide tiles give bit-identical replicate moments."""
    engine, torch, csr, gid, blocks, sf = big
    S, sumx, maxx = blocks.moments(1.0 / sf)
    rng = np.random.default_rng(21)
    ng = blocks.n_groups
    genes = np.sort(rng.choice(np.flatnonzero(sumx.sum(axis=0) > 2000), size=-(-2300 // ng), replace=False))
    n_bins = 31
    sf_bin = rng.integers(0, n_bins, size=csr.shape[0]).astype(np.uint8)
    sf_table = np.linspace(0.4, 2.5, n_bins)
    B = 40
    out = []
    for waves in (engine.PACK_WAVES, 10 ** 7):
        monkeypatch.setattr(engine, "PACK_MAX_RESIDENT", 2048 if waves == engine.PACK_WAVES else 10 ** 9)   # allow 1-chain tiles
        bs = engine.Bootstrap1D(blocks, genes, maxx, sf_bin, sf_table, np.full(ng, 0.07), B)
        r = np.random.default_rng(4).random((2, bs.n_pairs))
        zeros = np.zeros(bs.n_pairs)
        bs.alloc_outputs(zeros, zeros)
        bs.run(np.zeros(bs.n_pairs, bool), r[0], r[1], [0.0, 1.0, 0.0], fill_mode=1, dump_weights=True, target_waves=waves)
        out.append((bs.n_tiles, engine.host(bs.raw_mean), engine.host(bs.raw_var)))
    assert out[0][0] <= 2048 < out[1][0]
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][2], out[1][2])


def test_four_replay_kernels_agree_bit_for_bit(big, monkeypatch):
    """The same chains through (a) the lane-asynchronous tile kernel (mm_boot1d_async: every lane at its own pace, the draw as a
    resumable state machine), (b) the one-wave-per-chain kernel (mm_boot1d_chain: wave-uniform samplers fed by lane-parallel PCG64
    batches), (c) the lock-step tile kernel (mm_boot1d_replay: one BTPE attempt per bin step, the lanes meet at the end of the replicate)
    and (d) the tile kernel whose lanes run free across replicates on per-chain operand records (mm_boot1d_free): integer weights and
    replicate moments bit-identical."""
    engine, torch, csr, gid, blocks, sf = big
    S, sumx, maxx = blocks.moments(1.0 / sf)
    rng = np.random.default_rng(33)
    ng = blocks.n_groups
    genes = np.sort(rng.choice(np.flatnonzero(sumx.sum(axis=0) > 3000), size=40, replace=False))
    n_bins = 31
    sf_bin = rng.integers(0, n_bins, size=csr.shape[0]).astype(np.uint8)
    sf_table = np.linspace(0.4, 2.5, n_bins)
    B = 150           # > 128: several 64-replicate output groups of the chain kernel and a ragged last one
    out = []
    for mode, min_k in (("async", 0), ("lockstep", 2), ("lockstep", 0), ("free", 0)):
        monkeypatch.setattr(engine, "TILE_MODE", "lockstep" if mode == "free" else mode)
        monkeypatch.setattr(engine, "TILE_FREE", mode == "free")
        monkeypatch.setattr(engine, "ASYNC_CHAIN_MIN_K", 0)
        monkeypatch.setattr(engine, "CHAIN_MIN_K", min_k)
        monkeypatch.setattr(engine, "CHAIN_LONE", False)
        monkeypatch.setattr(engine, "CHAIN_ALL_MAX", 0)
        bs = engine.Bootstrap1D(blocks, genes, maxx, sf_bin, sf_table, np.full(ng, 0.07), B)
        r = np.random.default_rng(4).random((2, bs.n_pairs))
        zeros = np.zeros(bs.n_pairs)
        bs.alloc_outputs(zeros, zeros)
        bs.run(np.zeros(bs.n_pairs, bool), r[0], r[1], [0.0, 1.0, 0.0], fill_mode=1, dump_weights=True)
        n_act = int(bs.active.sum())
        assert (bs.n_async, bs.n_chain, bs.n_tiles > 0) == {("async", 0): (n_act, 0, False), ("lockstep", 2): (0, n_act, False),
                                                            ("lockstep", 0): (0, 0, True), ("free", 0): (0, 0, True)}[(mode, min_k)]
        out.append((engine.host(bs.raw_mean), engine.host(bs.raw_var), [bs.weights_of(p) for p in range(0, bs.n_pairs, 9)]))
    for other in out[1:]:
        np.testing.assert_array_equal(out[0][0], other[0])
        np.testing.assert_array_equal(out[0][1], other[1])
        for a, b in zip(out[0][2], other[2]):
            np.testing.assert_array_equal(a, b)
    assert np.isfinite(out[0][0][:, 1:]).any()


@pytest.mark.parametrize("tile_mode", ["lockstep", "async"])
def test_replay_weights_bit_exact_at_scale(big, monkeypatch, tile_mode):
    """BTPE-heavy stress of the samplers on the device: >1e6 draws on 12k-cell (C2) / 48k-cell (C3) groups must equal
    numpy's Generator(PCG64(5)).multinomial draw for draw -- the longer half of the chains through the one-wave-per-chain
    kernel, the shorter half through the lock-step tile kernel (every lane steps its own PCG64 generator) or the
    lane-asynchronous tile kernel."""
    engine, torch, csr, gid, blocks, sf = big
    S, sumx, maxx = blocks.moments(1.0 / sf)
    rng = np.random.default_rng(3)
    dense = np.flatnonzero(sumx.sum(axis=0) > 20000)
    genes = np.sort(rng.choice(dense, size=min(24, len(dense)), replace=False))
    n_bins = 31
    sf_bin = rng.integers(0, n_bins, size=csr.shape[0]).astype(np.uint8)
    sf_table = np.linspace(0.4, 2.5, n_bins)
    B = 96
    ng = blocks.n_groups
    bs = engine.Bootstrap1D(blocks, genes, maxx, sf_bin, sf_table, np.full(ng, 0.07), B)
    r = rng.random((2, bs.n_pairs))
    zeros = np.zeros(bs.n_pairs)
    bs.alloc_outputs(zeros, zeros)
    monkeypatch.setattr(engine, "CHAIN_MIN_K", int(np.median(bs.K[bs.K >= 2])) + 1)
    monkeypatch.setattr(engine, "TILE_MODE", tile_mode)
    monkeypatch.setattr(engine, "ASYNC_CHAIN_MIN_K", 0)
    monkeypatch.setattr(engine, "CHAIN_ALL_MAX", 0)
    bs.run(np.zeros(bs.n_pairs, bool), r[0], r[1], [0.0, 1.0, 0.0], fill_mode=1, dump_weights=True)
    n_draws = 0
    assert bs.n_chain > 0 and (bs.n_async if tile_mode == "async" else bs.n_tiles) > 0          # both kernels are exercised
    for p in range(bs.n_pairs):
        bi, xi, mu = bs.bins_of_pair(p)
        code = xi.astype(np.float64) * r[0][p] + r[1][p] * sf_table[bi]
        o = np.argsort(code, kind="stable")
        mult = mu[o].astype(np.int64)
        want = np.random.Generator(np.random.PCG64(5)).multinomial(int(blocks.grp_ncells[p % ng]), mult / mult.sum(), size=B).T
        np.testing.assert_array_equal(bs.weights_of(p), want, err_msg=f"pair {p}")
        n_draws += (len(mult) - 1) * B
    assert n_draws > 1_000_000


@pytest.mark.parametrize("rng_mode", ["replay", "fast"])
def test_null_calibration(rng_mode):
    """Statistical acceptance (the reference validates itself this way, analysis/simulation/calibration.ipynb): with
    group labels independent of the counts, DE p-values are uniform -- for the numpy-replay mode and for the
    replicate-parallel fast mode alike."""
    import pandas as pd
    import scipy.stats as stats

    from scrna_parameter_estimation_amd import memento
    from scrna_parameter_estimation_amd.synth import synth_adata

    adata = synth_adata(24000, 900, 0.12, 2, 3, seed=101, dtype=np.float32)
    memento.setup_memento(adata, q_column="q")
    memento.create_groups(adata, label_columns=["cond", "rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.7)
    gdf = memento.get_groups(adata)
    cov = pd.DataFrame({"intercept": np.ones(len(gdf))}, index=gdf.index)
    trt = pd.DataFrame({"cond": gdf["cond"].astype(float)}, index=gdf.index)
    np.random.seed(4)
    memento.ht_1d_moments(adata, covariate=cov, treatment=trt, num_boot=2000, num_cpus=1, verbose=0, resampling="bootstrap",
                          approx=True, rng=rng_mode, fill_seed=11)
    p = adata.uns["memento"]["1d_ht"]["mean_asl"]
    p = p[np.isfinite(p)]
    assert len(p) > 300
    chi2 = stats.chi2.isf(p, 1)
    lam = np.median(chi2) / stats.chi2.ppf(0.5, 1)          # genomic inflation factor; the reference reports 0.9956
    assert 0.75 < lam < 1.3, lam
    assert stats.kstest(p, "uniform").pvalue > 1e-4


def test_timed_mode_equals_strict_mode_on_genes_without_refills():
    """bench.py times strict=False (invalid replicates refilled on the device); the reference-pinned mode is strict=True (the
    reference's own _fill draws replayed from the global stream).  At configs[1] size (C2: 100k cells x 20k genes, 8 groups,
    1,000 bootstraps, exact ASL incl. the host tail fits), on a 200-gene sample: for EVERY gene none of whose chains needed a
    refill the two modes give bit-identical coefficients, standard errors and p-values; the others differ only by the refill
    draws.  The refilled fraction is what bench.py reports as bootstrap.refilled_gene_frac."""
    import pandas as pd
    import scipy.sparse as sp
    import torch

    import bench
    from scrna_parameter_estimation_amd import AnnDataLite, memento

    cfg = dict(bench.CONFIGS["C2"])
    N, G = cfg["cells"], cfg["genes"]
    csr = bench.synth_device_csr(cfg, 20250117, torch)
    rng = np.random.default_rng(20250117)
    grp = rng.integers(0, cfg["n_cond"] * cfg["n_rep"], size=N)
    obs = pd.DataFrame({"cond": grp // cfg["n_rep"], "rep": grp % cfg["n_rep"], "q": np.full(N, 0.07)})
    adata = AnnDataLite(sp.csr_matrix((N, G), dtype=np.float32), obs, pd.DataFrame(index=[f"g{i}" for i in range(G)]))
    memento.setup_memento(adata, q_column="q", device_csr=csr)
    memento.create_groups(adata, label_columns=["cond", "rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.7, subset_var=False)
    m = adata.uns["memento"]
    st = m["_hip"]
    kept = memento.main._var_names(adata)
    assert len(kept) > 1000
    sample = kept[:: len(kept) // 200][:200].tolist()
    memento.compute_1d_moments(adata, min_perc_group=0.7, subset_var=False, gene_list=sample)
    assert len(st.gene_idx) == 200
    gdf = memento.get_groups(adata)
    cov = pd.DataFrame({"intercept": np.ones(len(gdf))}, index=gdf.index)
    trt = pd.DataFrame({"cond": (gdf["cond"].astype(int) == 1).astype(float)}, index=gdf.index)
    res = {}
    for strict in (False, True):
        np.random.seed(31)
        memento.ht_1d_moments(adata, covariate=cov, treatment=trt, num_boot=cfg["num_boot"], num_cpus=4, verbose=0,
                              resampling="bootstrap", approx=False, strict=strict)
        res[strict] = {k: m["1d_ht"][k].copy() for k in ("mean_coef", "mean_se", "mean_asl", "var_coef", "var_se", "var_asl")}
        if not strict:
            refilled = st.refill_stats["gene_refilled"].copy()
    clean = ~refilled
    print(f"\nC2 sample: {int(refilled.sum())} of 200 genes have at least one refilled replicate "
          f"({st.refill_stats['chains_refilled']} of {st.refill_stats['chains']} chains)")
    assert clean.sum() >= 100
    for k in res[True]:
        np.testing.assert_array_equal(res[False][k][clean], res[True][k][clean], err_msg=k)            # bit-identical
        if k.endswith("coef"):
            np.testing.assert_allclose(res[False][k], res[True][k], rtol=1e-12, equal_nan=True)       # observed values never depend on it
    ok = refilled & np.isfinite(res[True]["var_se"])
    if ok.any():
        assert np.median(np.abs(res[False]["var_se"][ok] / res[True]["var_se"][ok] - 1)) < 0.05
