"""The max-T adjustment of ht_1d_posthoc: mm_family_maxt beside mm_contrast_design_stats on the same tests, and its share of one call.

Part 1, synthetic replicate planes (--genes x --groups rows of B + 1 normal values, generated on the device), two-entry designs:
  * pairwise: every gene's family is all pairs of the --groups groups (190 members at 20 groups);
  * many-to-one (--levels L, skipped at 0): --m2o-genes genes x (L + 1) groups, B = --m2o-boot, every group against group 0 --
    the shape of the recorded vs-control configuration (500 guides and a control, 5,000 replicates).
For each: mm_contrast_design_stats on the tests (the members' records: what the adjustment is added to) and mm_family_maxt on the
same tests with the scales of those records.  HIP events around back-to-back launches after a warm-up, median of three passes.
Part 2 (skipped with --no-call; --no-kernels skips part 1): a synthetic count matrix grouped by ONE label column of --groups levels,
one pairwise ht_1d_posthoc call timed by the host clock around a device synchronise, and both kernels alone on that call's last
chunk and tables.
usage: python tools/bench_posthoc.py [--genes 2000] [--groups 20] [--boot 10000] [--levels 500] [--m2o-genes 500] [--m2o-boot 5000]
                                     [--cells 100000] [--no-call] [--no-kernels]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, pandas as pd, torch, scipy.sparse as sp
from scrna_parameter_estimation_amd import AnnDataLite, _lib, engine, memento
from scrna_parameter_estimation_amd.memento import _ht
from bench_joint import _events, _opt


def _launches(bs, family_ptr, tables, scale=None):
    """mm_contrast_design_stats and mm_family_maxt on the same tests with everything uploaded once: -> (design launch, family launch,
    what they write to)."""
    if scale is None:
        st_m, st_v, _ = bs.contrast_design(*tables)
        scale = engine.family_scale(st_m, st_v)
    family_ptr, scale, d_tab = engine._family_tables(family_ptr, *tables, scale, bs.n_tested, bs.ng)
    n_fam, n_tests = len(family_ptr) - 1, len(scale)
    cap = min(engine.FAMILY_MAX_STAGED, int(np.diff(family_ptr).max()))
    d_fp, d_scale = engine.dev(family_ptr), engine.dev(scale.reshape(-1))
    st = [engine.empty((n_tests, 8), torch.float64) for _ in range(2)]
    maxrow, adj, fam = (engine.empty(s, torch.float64) for s in ((n_fam, 2, bs.ld), (n_tests, 2, 2), (n_fam, 2, 2)))
    planes = [engine.P(bs.ym), engine.P(bs.yv), bs.ld, bs.B, bs.ng]
    a_design = planes + [*map(engine.P, d_tab), n_tests, engine.P(st[0]), engine.P(st[1]), engine._stream()]
    a_family = planes + [engine.P(d_fp), *map(engine.P, d_tab), engine.P(d_scale), cap, n_fam, engine.P(maxrow), engine.P(adj), engine.P(fam),
                         engine._stream()]
    keep = (d_tab, d_fp, d_scale, st, maxrow, adj, fam)
    return (lambda: _lib.call("mm_contrast_design_stats", *a_design)), (lambda: _lib.call("mm_family_maxt", *a_family)), keep


def _report(tag, bs, family_ptr, tables, scale=None):
    design, family, keep = _launches(bs, family_ptr, tables, scale)
    t_d, p_d = _events(design, reps=3)
    t_f, p_f = _events(family, reps=3)
    fam = engine.host(keep[-1])
    print(f"{tag}: {len(family_ptr) - 1} families, {len(tables[0])} tests; mm_contrast_design_stats {t_d:.3f} ms (passes {[round(x, 3) for x in p_d]}); "
          f"mm_family_maxt {t_f:.3f} ms (passes {[round(x, 3) for x in p_f]}); ratio {t_f / t_d:.2f}; "
          f"n_included {int(fam[:, 0, 1].min())}..{int(fam[:, 0, 1].max())}, n_valid {int(fam[:, 0, 0].min())}..{int(fam[:, 0, 0].max())}", flush=True)
    return t_d, t_f


def _synthetic(genes, groups, B):
    bs = object.__new__(engine.Bootstrap1D)
    gen = torch.Generator(device="cuda").manual_seed(1)
    bs.ym = torch.randn((genes * groups, B + 1), dtype=torch.float64, device="cuda", generator=gen)
    bs.yv = torch.randn((genes * groups, B + 1), dtype=torch.float64, device="cuda", generator=gen)
    bs.ld, bs.B, bs.ng, bs.n_tested = B + 1, B, groups, genes
    print(f"planes: {genes} genes x {groups} groups x {B + 1} columns, {2 * bs.ym.numel() * 8 / 1e9:.2f} GB in both", flush=True)
    return bs


def kernels(genes, groups, B, control=None):
    bs = _synthetic(genes, groups, B)
    designs = _ht.PosthocDesigns([[str(g)] for g in range(groups)], None, control, np.ones(groups))
    n_mem = len(designs.pairs)
    tables = (np.repeat(np.arange(genes), n_mem), designs.tests(np.ones((genes, groups), dtype=bool)), *designs.tables())
    _report(f"{'pairwise' if control is None else 'many-to-one'}, {n_mem} members", bs, np.arange(genes + 1) * n_mem, tables)


def one_call(cells, genes, groups, B):
    import bench

    csr = bench.synth_device_csr(dict(cells=cells, genes=genes, density=0.1), 20250117 + 11, torch)
    obs = pd.DataFrame({"level": np.random.default_rng(3).integers(0, groups, size=cells), "q": np.full(cells, 0.07)})
    adata = AnnDataLite(sp.csr_matrix((cells, genes), dtype=np.float32), obs, pd.DataFrame(index=[f"g{i}" for i in range(genes)]))
    memento.setup_memento(adata, q_column="q", device_csr=csr)
    memento.create_groups(adata, label_columns=["level"])
    memento.compute_1d_moments(adata, min_perc_group=0.7, subset_var=False)
    st = adata.uns["memento"]["_hip"]
    print(f"call: {cells} cells, {len(st.gene_idx)} genes kept of {genes}, {groups} levels (one group each), B {B}", flush=True)
    times = []
    for run in range(3):                                             # run 0 is the warm-up
        np.random.seed(0)
        torch.cuda.synchronize(); t0 = time.time()
        df = memento.ht_1d_posthoc(adata, num_boot=B, approx=True)
        torch.cuda.synchronize(); times.append(time.time() - t0)
        print(f"  ht_1d_posthoc run {run}{' (warm-up)' if run == 0 else ''}: {times[-1]:.3f} s", flush=True)
    bs, (g0, g1), last = st.last_bootstrap, st.last_chunk, st.last_posthoc
    t_d, t_f = _report(f"last chunk ({g1 - g0} genes)", bs, last.family_ptr, last.tables, last.scale)
    t_call = float(np.median(times[1:]))
    n_genes = len(st.gene_idx)
    scale = n_genes / max(1, g1 - g0)                                # the call's chunks are equal but for the last
    print(f"ht_1d_posthoc (approx=True): {n_genes} genes, {len(df)} rows, {t_call:.3f} s a call; of it mm_family_maxt "
          f"{t_f * scale / 1e3 / t_call * 100:.2f} %, mm_contrast_design_stats {t_d * scale / 1e3 / t_call * 100:.2f} %", flush=True)


def main():
    genes, groups, B = _opt("--genes", 2000), _opt("--groups", 20), _opt("--boot", 10000)
    levels, m2o_genes, m2o_boot = _opt("--levels", 500), _opt("--m2o-genes", 500), _opt("--m2o-boot", 5000)
    cells = _opt("--cells", 100_000)
    no_call, no_kernels = "--no-call" in sys.argv, "--no-kernels" in sys.argv
    engine._lib.load(require_gpu=True)
    if not no_kernels:
        kernels(genes, groups, B)
        torch.cuda.empty_cache()
        if levels > 0:
            kernels(m2o_genes, levels + 1, m2o_boot, control=0)
            torch.cuda.empty_cache()
    if not no_call:
        one_call(cells, int(genes * 1.5), groups, B)


if __name__ == "__main__":
    main()
