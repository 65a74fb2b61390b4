"""Perturb-seq shape (BASELINE configs[4]): n_guides guide groups x 1 shared control (20 % of the cells), every kept gene
tested guide-vs-control in ONE call (memento.ht_1d_vs_control), next to the per-guide loop the reference's analyses use
(subset -> ht_1d_moments with 2 groups; here timed on a few guides through the same HIP path and extrapolated).
With --strata R every cell also gets a replicate 0..R-1 (column ``rep``): the groups are guide x replicate and the call is
ht_1d_vs_control(..., treatment_col='guide') with the replicate as covariate.
--rng fast selects the replicate-parallel bootstrap; with it, --max-boot N [--min-extreme M] runs the sequential bootstrap
(num_boot replicates for every test, up to N for the tests still open) and prints the tests open after every round.
--repeat K times the call K times after one untimed warm-up call, on the same inputs and seeds, and prints the median.
usage: python tools/bench_vs_control.py [--strata R] [--rng fast] [--max-boot N] [--min-extreme M] [--repeat K]
       [cells genes n_guides num_boot approx(0/1)]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, pandas as pd, torch, scipy.sparse as sp
import bench
from scrna_parameter_estimation_amd import AnnDataLite, memento


def _flag(name, default, kind=int):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    val = kind(sys.argv[i + 1])
    del sys.argv[i:i + 2]
    return val


def main():
    strata = _flag("--strata", 1)
    rng_mode, max_boot, min_extreme, repeat = _flag("--rng", "replay", str), _flag("--max-boot", None), _flag("--min-extreme", 10), _flag("--repeat", 0)
    cells, genes, n_guides, B, approx = [int(x) for x in sys.argv[1:6]] if len(sys.argv) > 5 else (200_000, 15_000, 500, 5_000, 0)
    cfg = dict(cells=cells, genes=genes, density=0.05)
    # multi-GPU: one process per GPU (torch.distributed.run); every rank holds all cells x its own gene shard of this shape
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)) % max(1, torch.cuda.device_count()))
    comm = None
    if world > 1:
        import torch.distributed as dist
        from scrna_parameter_estimation_amd.dist import Comm
        backend = os.environ.get("MM_DIST_BACKEND", "nccl")
        dist.init_process_group(backend=backend)
        comm = Comm(device="cuda" if backend == "nccl" else "cpu")
    csr = bench.synth_device_csr(cfg, 20250117 + 5 + 1000 * rank, torch)
    rng = np.random.default_rng(20250117 + 5)
    is_ctrl = rng.random(cells) < 0.2
    guide = np.where(is_ctrl, 0, 1 + rng.integers(0, n_guides, size=cells))
    obs = pd.DataFrame({"guide": guide, "q": np.full(cells, 0.07)})
    if strata > 1:
        obs["rep"] = rng.integers(0, strata, size=cells)
    adata = AnnDataLite(sp.csr_matrix((cells, genes), dtype=np.float32), obs, pd.DataFrame(index=[f"r{rank}g{i}" for i in range(genes)]))
    t0 = time.time()
    memento.setup_memento(adata, q_column="q", device_csr=csr, comm=comm)
    memento.create_groups(adata, label_columns=["guide", "rep"] if strata > 1 else ["guide"])
    torch.cuda.synchronize(); t1 = time.time()
    memento.compute_1d_moments(adata, min_perc_group=0.7, subset_var=False)
    torch.cuda.synchronize(); t2 = time.time()
    m = adata.uns["memento"]
    ctrl = [g for g in m["groups"] if g.split("^")[-1] == "0"][0] if strata == 1 else 0
    print(f"setup+groups {t1-t0:.2f}s compute_1d_moments {t2-t1:.2f}s genes kept {len(m['_hip'].gene_idx)} groups {len(m['groups'])} control {ctrl}", flush=True)
    kw = dict(treatment_col="guide") if strata > 1 else {}
    if rng_mode != "replay":
        kw["rng"] = rng_mode
    if max_boot is not None:
        kw.update(max_boot=max_boot, min_extreme=min_extreme)
    times = []
    for it in range(repeat + 1 if repeat else 1):       # (--repeat: the first call is the warm-up)
        np.random.seed(0)
        torch.cuda.synchronize(); t3 = time.time()
        df = memento.ht_1d_vs_control(adata, control=ctrl, num_boot=B, num_cpus=16, approx=bool(approx), **kw)
        torch.cuda.synchronize(); t4 = time.time()
        if it or not repeat:
            times.append(t4 - t3)
        if repeat:
            print(f"  call {it}: {t4 - t3:.3f}s", flush=True)
    n = len(df)
    if repeat:
        print(f"ht_1d_vs_control x{repeat} after a warm-up: median {np.median(times):.3f}s min {min(times):.3f}s max {max(times):.3f}s "
              f"({' '.join(f'{t:.3f}' for t in times)})", flush=True)
    if max_boot is not None:
        sq = m["_hip"].last_sequential
        nb = np.concatenate([df.de_nboot.values, df.dv_nboot.values])
        print(f"sequential: schedule {sq.schedule} tests open after each round {sq.n_open} of {n}; mean replicates per p-value "
              f"{nb.mean():.0f}; finite p-values below 1 / (num_boot + 1): de {(df.de_pval < 1 / (B + 1)).sum()} dv {(df.dv_pval < 1 / (B + 1)).sum()}", flush=True)
    print(f"ht_1d_vs_control: {n} (gene, guide) tests in {t4-t3:.2f}s -> {n/(t4-t3):.0f} tests/s ({n/(t4-t2+ (t2-t1)):.0f} incl. moments); "
          f"finite de_pval {np.isfinite(df.de_pval).mean():.3f} dv_pval {np.isfinite(df.dv_pval).mean():.3f}", flush=True)


if __name__ == "__main__":
    main()
