"""Perturb-seq shaped differential COEXPRESSION: n_guides guide groups x 1 shared control (20 % of the cells), n_pairs gene pairs
among the best expressed genes, every (pair, guide) tested guide-vs-control in ONE call (memento.ht_2d_vs_control), next to the
per-guide loop the reference's analyses use (subset to {control, guide} -> ht_2d_moments; here a loop of this project's own
ht_2d_moments over the subsets, timed on --loop-guides guides and scaled to all of them).
With --strata R every cell also gets a replicate 0..R-1 (column ``rep``): the groups are guide x replicate and the call is
ht_2d_vs_control(..., treatment_col='guide') with the replicate as covariate.
--rng fast runs the batched call with the replicate-parallel bootstrap (mm_boot2d_fast) instead of the replay kernel (the default).
--max-boot N (with --rng fast) runs the sequential bootstrap, ht_2d_vs_control_sequential(num_boot, max_boot=N, min_extreme=--min-extreme), with
approx=False, and prints the tests open after and the chains bootstrapped in every round; --exact runs a plain call with
approx=False too (tail fits on the host).  --repeat N: one warm-up call (allocator, kernel load), then N timed calls.
--compare-launches (with --max-boot): after the timed calls, on the kept last pair chunk, the open chains of every round are
bootstrapped once more into a compact plane by Bootstrap2D.launch_range (a grid over the chunk's tile layout) and by
Bootstrap2D.launch_listed (a grid over the chains), each timed with device events: one warm-up launch, then the median of 5.
usage: python tools/bench_vs_control_2d.py [--strata R] [--loop-guides K] [--repeat N] [--rng replay|fast] [--max-boot N] [--min-extreme M]
                                           [--exact] [--compare-launches] [cells genes n_guides n_pairs num_boot]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, pandas as pd, torch, scipy.sparse as sp
import bench
from scrna_parameter_estimation_amd import AnnDataLite, engine, memento


def _opt(name, default, conv=int):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = conv(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return v
    return default


def compare_launches(m, ctrl, treatment_col, plane_bytes=8 << 30):
    """Both launches on the open chains of every round of the last pair chunk (see the module docstring)."""
    from scrna_parameter_estimation_amd.memento import _ht
    st = m["_hip"]
    seq, bs = st.last_sequential, st.last_bootstrap2d
    _, designs, (ctrl_idx, _), _ = memento.main._vs_control_plan(m, ctrl, treatment_col)
    d = _ht._TwoGroupDesigns(bs.ng, ctrl_idx) if designs is None else designs
    test_design = d.tests(bs.active.reshape(bs.n_pairs, bs.ng))
    ptr, grp, _ = d.tables()
    test_pair = np.repeat(np.arange(bs.n_pairs), len(test_design) // bs.n_pairs)
    print(f"launch_range against launch_listed: last pair chunk, {bs.n_pairs} pairs, {bs.n_q} chains, {bs._fast.n_slots} slots", flush=True)
    for j in range(1, len(seq.schedule)):
        mask = seq.open_mask[j]
        if mask is None or not mask.any():
            break
        rep_lo, rep_n = seq.schedule[j - 1], seq.schedule[j] - seq.schedule[j - 1]
        chains = _ht._design_chains(test_pair[mask], test_design[mask], ptr, grp, bs.ng)
        n_all = len(chains)
        chains = chains[:max(1, plane_bytes // (8 * (1 + rep_n)))]
        plane = engine.empty((len(chains), 1 + rep_n), torch.float64)
        rows, ms = np.arange(len(chains)), {}
        for name, launch in (("range", bs.launch_range), ("listed", bs.launch_listed)):
            t = []
            for r in range(6):                                    # launch 0 is the warm-up
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                keep = launch(rep_lo, rep_n, chains, plane, rows)
                e1.record()
                torch.cuda.synchronize()
                t.append(e0.elapsed_time(e1))
                del keep
            ms[name] = (float(np.median(t[1:])), min(t[1:]), max(t[1:]))
        waves = ((rep_n + 63) // 64) * np.array([bs._fast.n_slots, len(chains)])
        print(f"  round {j}: replicates [{rep_lo}, {rep_lo + rep_n}), {int(mask.sum())} open tests, {n_all} chains"
              f"{'' if n_all == len(chains) else f' (the first {len(chains)} timed)'}; waves {waves[0]} / {waves[1]}; "
              f"range {ms['range'][0]:.3f} ms (min {ms['range'][1]:.3f} max {ms['range'][2]:.3f}), "
              f"listed {ms['listed'][0]:.3f} ms (min {ms['listed'][1]:.3f} max {ms['listed'][2]:.3f})", flush=True)
        del plane


def main():
    strata, loop_guides, repeat = _opt("--strata", 1), _opt("--loop-guides", 10), _opt("--repeat", 3)
    rng_mode, max_boot, min_extreme = _opt("--rng", "replay", str), _opt("--max-boot", None), _opt("--min-extreme", 10)
    flags = {f: f in sys.argv for f in ("--exact", "--compare-launches")}
    sys.argv[:] = [a for a in sys.argv if a not in flags]
    if rng_mode not in ("replay", "fast"):
        sys.exit("--rng must be replay or fast")
    cells, genes, n_guides, n_pairs, B = [int(x) for x in sys.argv[1:6]] if len(sys.argv) > 5 else (200_000, 15_000, 500, 2_000, 5_000)
    csr = bench.synth_device_csr(dict(cells=cells, genes=genes, density=0.05), 20250117 + 7, torch)
    rng = np.random.default_rng(20250117 + 7)
    is_ctrl = rng.random(cells) < 0.2
    guide = np.where(is_ctrl, 0, 1 + rng.integers(0, n_guides, size=cells))
    obs = pd.DataFrame({"guide": guide, "q": np.full(cells, 0.07)})
    if strata > 1:
        obs["rep"] = rng.integers(0, strata, size=cells)
    var = pd.DataFrame(index=[f"g{i}" for i in range(genes)])
    t0 = time.time()
    adata = AnnDataLite(sp.csr_matrix((cells, genes), dtype=np.float32), obs, var)
    memento.setup_memento(adata, q_column="q", device_csr=csr)
    memento.create_groups(adata, label_columns=["guide", "rep"] if strata > 1 else ["guide"])
    memento.compute_1d_moments(adata, min_perc_group=0.7, subset_var=False)
    m = adata.uns["memento"]
    names = memento.main._var_names(adata)
    mean_all = np.mean([m["1d_moments"][k][0] for k in m["groups"]], axis=0)
    n_top = max(8, int(np.ceil((1 + np.sqrt(1 + 8 * n_pairs)) / 2)) + 20)           # enough genes for n_pairs distinct pairs
    top = names[np.argsort(-mean_all, kind="stable")[:n_top]]
    iu, ju = np.triu_indices(len(top), 1)
    pick = rng.choice(len(iu), size=n_pairs, replace=False)
    pairs = [(str(top[a]), str(top[b])) for a, b in zip(iu[pick], ju[pick])]
    memento.compute_2d_moments(adata, pairs)
    torch.cuda.synchronize(); t1 = time.time()
    ctrl = [g for g in m["groups"] if g.split("^")[-1] == "0"][0] if strata == 1 else 0
    kw = dict(treatment_col="guide") if strata > 1 else {}
    kw["approx"] = not (flags["--exact"] or max_boot is not None)
    if rng_mode != "replay":
        kw["rng"] = rng_mode
    if max_boot is not None:
        kw.update(max_boot=max_boot, min_extreme=min_extreme)
    call = memento.ht_2d_vs_control if max_boot is None else memento.ht_2d_vs_control_sequential
    print(f"{call.__name__}(num_boot={B}, num_cpus=16, {', '.join(f'{k}={v!r}' for k, v in kw.items())})", flush=True)
    print(f"setup + moments {t1 - t0:.2f}s; genes kept {len(names)} groups {len(m['groups'])} pairs {n_pairs} (among the {n_top} best expressed "
          f"genes) B {B}", flush=True)
    times = []
    for r in range(repeat + 1):                                   # run 0 is the warm-up (allocator, kernel load)
        np.random.seed(0)
        torch.cuda.synchronize(); t2 = time.time()
        df = call(adata, control=ctrl, num_boot=B, num_cpus=16, **kw)
        torch.cuda.synchronize(); t3 = time.time()
        times.append(t3 - t2)
        print(f"  batched run {r}{' (warm-up)' if r == 0 else ''}: {t3 - t2:.2f}s", flush=True)
    n = len(df)
    timed = times[1:] or times
    t_b = float(np.median(timed))
    bs = m["_hip"].last_bootstrap2d
    print(f"ht_2d_vs_control: {n} (pair, guide) tests, median of {len(timed)} runs {t_b:.2f}s (min {min(timed):.2f} max {max(timed):.2f}) -> "
          f"{n / t_b:.0f} tests/s; finite corr_pval {np.isfinite(df.corr_pval).mean():.3f}; last pair chunk {m['_hip'].last_chunk2d}, "
          f"bins per chain mean {bs.K.mean():.0f} max {bs.K.max()}; p < 1/{B + 1}: {int((df.corr_pval.values < 1 / (B + 1)).sum())}", flush=True)
    if max_boot is not None:
        seq = m["_hip"].last_sequential
        print(f"sequential: schedule {seq.schedule}\n  tests open after each round {seq.n_open}\n  chains bootstrapped in each round "
              f"{seq.n_chains}\n  corr_nboot == max_boot: {int((df.corr_nboot.values == max_boot).sum())}", flush=True)
        if flags["--compare-launches"]:
            compare_launches(m, ctrl, kw.get("treatment_col"))
    m["_hip"].last_bootstrap2d = bs = None
    if loop_guides <= 0:
        return
    # the per-guide loop on this project's own ht_2d_moments: subset the cells, re-ingest, two (or 2 x strata) groups per guide
    sf = adata.obs["memento_size_factor"].values
    X = sp.csr_matrix((engine.host(csr.data), engine.host(csr.indices), engine.host(csr.indptr)), shape=csr.shape)
    guides = list(range(1, min(loop_guides, n_guides) + 1))
    loop_times = []
    for r in range(2):                                            # pass 0 is the warm-up
        torch.cuda.synchronize(); t4 = time.time()
        for gid in guides:
            rows = np.flatnonzero((guide == 0) | (guide == gid))
            o = obs.iloc[rows].reset_index(drop=True)
            o["is_guide"] = (o["guide"].values == gid).astype(int)
            sub = AnnDataLite(X[rows], o, var.copy())
            memento.setup_memento(sub, q_column="q", size_factor=sf[rows])       # the loop keeps the size factors of the whole matrix
            memento.create_groups(sub, label_columns=["is_guide", "rep"] if strata > 1 else ["is_guide"])
            memento.compute_1d_moments(sub, min_perc_group=0.7, subset_var=False)
            kept = set(memento.main._var_names(sub).tolist())
            memento.compute_2d_moments(sub, [p for p in pairs if p[0] in kept and p[1] in kept])
            gdf = memento.get_groups(sub)
            cov = pd.DataFrame({"intercept": np.ones(len(gdf))}, index=gdf.index)
            if strata > 1:
                cov = pd.concat([cov, pd.get_dummies(gdf["rep"].astype(str), prefix="rep", drop_first=True).astype(float)], axis=1)
            trt = pd.DataFrame({"is_guide": gdf["is_guide"].astype(float).values}, index=gdf.index)
            np.random.seed(gid)
            memento.ht_2d_moments(sub, covariate=cov, treatment=trt, num_boot=B, num_cpus=16, verbose=0, resampling="bootstrap", approx=True)
        torch.cuda.synchronize(); t5 = time.time()
        loop_times.append(t5 - t4)
        print(f"  loop pass {r}{' (warm-up)' if r == 0 else ''}: {len(guides)} guides in {t5 - t4:.2f}s", flush=True)
    per = loop_times[1] / len(guides)
    print(f"per-guide loop (ht_2d_moments on subsets): {per:.2f}s per guide -> {per * n_guides:.1f}s scaled to {n_guides} guides = "
          f"{per * n_guides / t_b:.1f}x the batched call", flush=True)


if __name__ == "__main__":
    main()
