"""Time ``ht_1d_eqtl`` next to the equivalent ``ht_1d_moments(treatment_for_gene=..., resample_rep=True, approx=True)`` on a synthetic
donor shape (one group per donor, a list of cis SNPs per gene): wall time of every repetition after the warm-up, median and
spread, and the peak device memory of each call above what was allocated before it.  One JSON line per call and one with the
ratio.  The two calls are fed the same inputs and the same ``np.random`` seed; in a one-chunk run their coefficients are compared.
``--adjust`` also times ``ht_1d_eqtl(adjust=True)`` (the gene-level max-T).  The calls ALTERNATE within every repetition, so that a
drift of the device hits them alike.  ``--interaction`` times the genotype-by-context scan instead: ``--groups`` donors x 2 contexts,
``ht_1d_eqtl(interaction=ctx)`` with and without ``resample_rep`` beside the plain ``ht_1d_eqtl`` calls on the same tree, a few
``ht_1d_moments(covariate=[cov | ctx | g_s], treatment=g_s * ctx)`` calls (the per-SNP route, reported per call and SCALED), and
mm_cross_cov_beta alone on the call's replicate planes (device events) for its share of the resampled call.

    python tools/bench_eqtl.py --groups 120 --genes 256 --snps 256 --num-boot 3000 --reps 5 --warmup 1
    python tools/bench_eqtl.py --groups 120 --genes 300 --snps 256 --num-boot 3000 --adjust --skip-parent
    python tools/bench_eqtl.py --groups 120 --genes 300 --snps 256 --num-boot 3000 --interaction --reps 3
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(torch, st, fn, seed=5):
    st.last_bootstrap = st.last_eqtl = None
    torch.cuda.synchronize()
    np.random.seed(seed)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def interaction_bench(args, torch, memento):
    """The ``--interaction`` run: one JSON line for the shape, one per call, one for the per-SNP route, one for the beta kernel."""
    from scrna_parameter_estimation_amd import engine
    from scrna_parameter_estimation_amd.memento import _ht
    from scrna_parameter_estimation_amd.synth import synth_adata

    adata = synth_adata(2 * args.groups * args.cells_per_group, args.genes, args.density, 2, args.groups, seed=7, dtype=np.float32)
    memento.setup_memento(adata, q_column="q")
    memento.create_groups(adata, label_columns=["cond", "rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.7)
    gdf = memento.get_groups(adata)
    st = adata.uns["memento"]["_hip"]
    names = [g for g in memento.main._var_names(adata)[:len(st.gene_idx)]]
    rng = np.random.default_rng(1)
    donor = gdf["rep"].values
    ctx = pd.Series(gdf["cond"].values.astype(float), index=gdf.index)
    cov = pd.DataFrame({"age": rng.normal(size=args.groups)[donor], "sex": rng.integers(0, 2, size=args.groups).astype(float)[donor]},
                       index=gdf.index)
    geno = pd.DataFrame(rng.integers(0, 3, size=(args.groups, args.pool)).astype(float)[donor], columns=[f"rs{j}" for j in range(args.pool)],
                        index=gdf.index)
    pairs = {g: [f"rs{j}" for j in rng.choice(args.pool, size=args.snps, replace=False)] for g in names}
    n_tests, ld, ng = len(names) * args.snps, args.num_boot + 1, len(gdf)
    print(json.dumps(dict(shape=dict(donors=args.groups, groups=ng, kept_genes=len(names), snps_per_gene=args.snps, n_tests=n_tests,
                                     num_boot=args.num_boot, rng=args.rng, plane_bytes=len(names) * ng * ld * 8,
                                     device=torch.cuda.get_device_name(0)))), flush=True)

    def eqtl(**kw):
        return memento.ht_1d_eqtl(adata, geno, pairs, covariate=cov, num_boot=args.num_boot, rng=args.rng, fill_seed=3, approx=True,
                                  max_rows=args.max_rows, **kw)

    def per_snp(snp):
        memento.ht_1d_moments(adata, covariate=cov.assign(ctx=ctx.values, g=geno[snp].values),
                              treatment=pd.DataFrame({"gxc": geno[snp].values * ctx.values}, index=gdf.index), num_boot=args.num_boot,
                              verbose=0, rng=args.rng, fill_seed=3, approx=True, resampling="bootstrap")

    calls = [("interaction_resample_rep", lambda: eqtl(interaction=ctx, resample_rep=True)), ("plain_resample_rep", lambda: eqtl(resample_rep=True)),
             ("interaction", lambda: eqtl(interaction=ctx)), ("plain", lambda: eqtl())]
    times = {n: [] for n, _ in calls}
    for r in range(args.warmup + args.reps):
        for name, fn in calls:
            dt, _ = _timed(torch, st, fn)
            if r >= args.warmup:
                times[name].append(dt)
    med = {}
    for name, _ in calls:
        med[name] = float(np.median(times[name]))
        print(json.dumps(dict(call=name, seconds=[round(x, 4) for x in times[name]], median_s=round(med[name], 4))), flush=True)
    snps = pairs[names[0]][:4]
    _timed(torch, st, lambda: per_snp(snps[0]))
    t = [_timed(torch, st, lambda s=s: per_snp(s))[0] for s in snps]
    distinct = len({s for v in pairs.values() for s in v})
    print(json.dumps(dict(call="ht_1d_moments_per_snp", seconds=[round(x, 4) for x in t], median_s=round(float(np.median(t)), 4),
                          tests_per_call=len(names), distinct_snps=distinct,
                          SCALED_by_tests_s=round(float(np.median(t)) * n_tests / len(names), 1),
                          SCALED_by_distinct_snps_s=round(float(np.median(t)) * distinct, 1))), flush=True)
    # mm_cross_cov_beta alone, on the planes of a one-chunk resampled call, both planes, in the engine's batches
    _timed(torch, st, calls[0][1])
    bs, (g0, g1) = st.last_bootstrap, st.last_chunk
    if (g0, g1) != (0, len(names)):
        print(json.dumps(dict(beta_kernel=None, why="the call ran in more than one chunk")), flush=True)
        return
    mv = _ht.moments_view(adata.uns["memento"])
    good = np.ones((len(names), ng), dtype=bool)
    d = _ht.eqtl_interaction_tables(good, _ht.eqtl_gene_columns(geno, pairs, names), cov.values, ctx.values, geno.values, mv.Nc_list)
    tiles = len(names) * ((args.snps + engine.CROSS_BLOCK_TT - 1) // engine.CROSS_BLOCK_TT)
    batch = max(1, min(tiles, engine.CROSS_COV_SCRATCH_BYTES // (ld * engine.CROSS_BLOCK_TT * 8)))
    beta = engine.empty((batch * ld * engine.CROSS_BLOCK_TT,), torch.float64)
    d_ptr, d_zt, d_good, d_nc = engine.dev(d.gene_ptr.astype(np.int32)), engine.dev(d.zt_mat), engine.dev(good.astype(np.uint8)), engine.dev(mv.Nc_list)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    shots = []
    for r in range(1 + args.reps):
        ev[0].record()
        for plane in (bs.ym, bs.yv):                # (the kernel's cost does not depend on the plane being residualised)
            for lo in range(0, tiles, batch):
                engine._lib.call("mm_cross_cov_beta", engine.P(plane), bs.ld, args.num_boot, ng, engine.P(d_ptr), len(names), args.snps,
                                 engine.P(d_zt), engine.P(d_good), engine.P(d_nc), n_tests, lo, min(lo + batch, tiles), engine.P(beta),
                                 engine._stream())
        ev[1].record()
        torch.cuda.synchronize()
        if r:
            shots.append(ev[0].elapsed_time(ev[1]) / 1e3)
    print(json.dumps(dict(beta_kernel_s=[round(x, 4) for x in shots], median_s=round(float(np.median(shots)), 4), batches=2 * -(-tiles // batch),
                          share_of_interaction_resample_rep=round(float(np.median(shots)) / med["interaction_resample_rep"], 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=120)
    ap.add_argument("--genes", type=int, default=256, help="genes of the synthetic matrix (the kept ones are fewer)")
    ap.add_argument("--snps", type=int, default=256, help="cis SNPs per gene")
    ap.add_argument("--pool", type=int, default=4096, help="genotype columns the lists are drawn from")
    ap.add_argument("--cells-per-group", type=int, default=150)
    ap.add_argument("--density", type=float, default=0.35)
    ap.add_argument("--num-boot", type=int, default=3000)
    ap.add_argument("--rng", default="fast")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parent-max-rows", type=int, default=None, help="max_rows of the ht_1d_moments call (default: its own choice)")
    ap.add_argument("--max-rows", type=int, default=None, help="max_rows of the ht_1d_eqtl call")
    ap.add_argument("--skip-parent", action="store_true")
    ap.add_argument("--adjust", action="store_true", help="also time ht_1d_eqtl(adjust=True)")
    ap.add_argument("--interaction", action="store_true", help="time ht_1d_eqtl(interaction=ctx) on --groups donors x 2 contexts instead")
    args = ap.parse_args()

    import torch

    from scrna_parameter_estimation_amd import memento
    from scrna_parameter_estimation_amd.synth import synth_adata

    if args.interaction:
        return interaction_bench(args, torch, memento)

    adata = synth_adata(args.groups * args.cells_per_group, args.genes, args.density, 1, args.groups, seed=7, dtype=np.float32)
    memento.setup_memento(adata, q_column="q")
    memento.create_groups(adata, label_columns=["rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.7)
    gdf = memento.get_groups(adata)
    st = adata.uns["memento"]["_hip"]
    names = [g for g in memento.main._var_names(adata)[:len(st.gene_idx)]]
    rng = np.random.default_rng(1)
    cov = pd.DataFrame({"age": rng.normal(size=len(gdf)), "sex": rng.integers(0, 2, size=len(gdf)).astype(float)}, index=gdf.index)
    geno = pd.DataFrame(rng.integers(0, 3, size=(len(gdf), args.pool)).astype(float), columns=[f"rs{j}" for j in range(args.pool)],
                        index=gdf.index)
    pairs = {g: [f"rs{j}" for j in rng.choice(args.pool, size=args.snps, replace=False)] for g in names}
    n_tests = len(names) * args.snps
    ld = args.num_boot + 1
    shape = dict(groups=len(gdf), kept_genes=len(names), snps_per_gene=args.snps, n_tests=n_tests, num_boot=args.num_boot, rng=args.rng,
                 plane_bytes=len(names) * len(gdf) * ld * 8, rows_bytes=n_tests * ld * 8, device=torch.cuda.get_device_name(0))
    print(json.dumps(dict(shape=shape)), flush=True)

    def eqtl(**kw):
        return memento.ht_1d_eqtl(adata, geno, pairs, covariate=cov, num_boot=args.num_boot, rng=args.rng, fill_seed=3, approx=True,
                                  resample_rep=True, max_rows=args.max_rows, **kw)

    def parent():
        memento.ht_1d_moments(adata, covariate=cov, treatment=geno, treatment_for_gene=pairs, num_boot=args.num_boot, verbose=0,
                              rng=args.rng, fill_seed=3, approx=True, resample_rep=True, resampling="bootstrap",
                              max_rows=args.parent_max_rows)
        return memento.get_1d_ht_result(adata)

    results, frames = {}, {}
    calls = [("ht_1d_eqtl", eqtl)]
    if args.adjust:
        calls.append(("ht_1d_eqtl_adjust", lambda: eqtl(adjust=True)))
    if not args.skip_parent:
        calls.append(("ht_1d_moments", parent))
    times, peak, chunk = {n: [] for n, _ in calls}, {n: 0 for n, _ in calls}, {}
    for rep in range(args.warmup + args.reps):
        for name, fn in calls:
            st.last_bootstrap = st.last_eqtl = None
            frames.pop(name, None)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            np.random.seed(5)
            t0 = time.perf_counter()
            frames[name] = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            chunk[name] = int(st.last_chunk[1] - st.last_chunk[0])
            if rep >= args.warmup:
                times[name].append(dt)
                peak[name] = max(peak[name], torch.cuda.max_memory_allocated() - before)
    for name, _ in calls:
        t = np.array(times[name])
        results[name] = dict(call=name, seconds=[round(x, 4) for x in times[name]], median_s=round(float(np.median(t)), 4),
                             min_s=round(float(t.min()), 4), max_s=round(float(t.max()), 4), peak_device_bytes=int(peak[name]),
                             chunk_genes=chunk[name], max_rows=args.parent_max_rows if name == "ht_1d_moments" else args.max_rows)
        print(json.dumps(results[name]), flush=True)
    if args.adjust:
        a, b = frames["ht_1d_eqtl"], frames["ht_1d_eqtl_adjust"]
        print(json.dumps(dict(adjust_over_plain_median=round(results["ht_1d_eqtl_adjust"]["median_s"] / results["ht_1d_eqtl"]["median_s"], 3),
                              shared_columns_equal=bool(a.equals(b[list(a.columns)])),
                              genes_with_adjusted_p=int(np.isfinite(memento.get_eqtl_gene_result(adata)["de_gene_pval"]).sum())
                              if calls[-1][0] != "ht_1d_moments" else None)), flush=True)
    if not args.skip_parent:
        a, b = frames["ht_1d_eqtl"], frames["ht_1d_moments"]
        one_chunk = all(r["chunk_genes"] == len(names) for r in results.values())
        same = bool(one_chunk and np.array_equal(a["de_coef"].values, b["de_coef"].values, equal_nan=True)
                    and np.array_equal(a["dv_coef"].values, b["dv_coef"].values, equal_nan=True))
        print(json.dumps(dict(speedup_median=round(results["ht_1d_moments"]["median_s"] / results["ht_1d_eqtl"]["median_s"], 3),
                              peak_ratio=round(results["ht_1d_moments"]["peak_device_bytes"] / max(1, results["ht_1d_eqtl"]["peak_device_bytes"]), 3),
                              one_chunk=one_chunk, coefficients_equal=same if one_chunk else None)), flush=True)


if __name__ == "__main__":
    main()
