"""The max-T adjustment of ht_1d_posthoc: mm_family_maxt beside mm_contrast_design_stats on the same tests, and its share of one call.
With --one-plane, that of ht_2d_posthoc: mm_family_maxt1 beside mm_contrast_design1_stats on ONE plane of the same shapes (the rows
of a gene stand for the replicate correlations of a pair), and its share of one ht_2d_posthoc(approx=True) call on the shape of
tools/bench_vs_control_2d.py (--cells cells, --call-genes genes, --guides guides + a control of 20 % of the cells, --pairs pairs
among the best expressed genes, B = --call-boot; every guide against the control: --guides members a family).

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
                                     [--cells 100000] [--no-call] [--no-kernels]
       python tools/bench_posthoc.py --one-plane [the kernel options above] [--cells 200000] [--call-genes 15000] [--guides 500]
                                     [--pairs 2000] [--call-boot 5000] [--no-call] [--no-kernels]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, pandas as pd, torch, scipy.sparse as sp
from scrna_parameter_estimation_amd import AnnDataLite, _lib, engine, memento
from scrna_parameter_estimation_amd.memento import _ht
from bench_joint import _events, _opt


def _names(bs):
    """The two entry points a bootstrap object's tests go through: (records, adjustment)."""
    one = isinstance(bs, engine.Bootstrap2D)
    return ("mm_contrast_design1_stats", "mm_family_maxt1") if one else ("mm_contrast_design_stats", "mm_family_maxt")


def _launches(bs, family_ptr, tables, scale=None):
    """mm_contrast_design_stats and mm_family_maxt (Bootstrap2D: their one-plane forms) on the same tests with everything uploaded
    once: -> (design launch, family launch, what they write to)."""
    one = isinstance(bs, engine.Bootstrap2D)
    planes, n_rows = ([bs.yc], bs.n_pairs) if one else ([bs.ym, bs.yv], bs.n_tested)
    n_p = len(planes)
    if scale is None:
        scale = engine.family_scale(bs.contrast_design(*tables)[0]) if one else engine.family_scale(*bs.contrast_design(*tables)[:2])
    family_ptr, scale, d_tab = engine._family_tables(family_ptr, *tables, scale, n_rows, bs.ng, n_p)
    n_fam, n_tests = len(family_ptr) - 1, len(scale)
    cap = min(engine.FAMILY_MAX_STAGED, int(np.diff(family_ptr).max()))
    d_fp, d_scale = engine.dev(family_ptr), engine.dev(scale.reshape(-1))
    st = [engine.empty((n_tests, 8), torch.float64) for _ in planes]
    maxrow, adj, fam = (engine.empty(s, torch.float64) for s in ((n_fam, n_p, bs.ld), (n_tests, n_p, 2), (n_fam, n_p, 2)))
    head = [*map(engine.P, planes), bs.ld, bs.B, bs.ng]
    a_design = head + [*map(engine.P, d_tab), n_tests, *map(engine.P, st), engine._stream()]
    a_family = head + [engine.P(d_fp), *map(engine.P, d_tab), engine.P(d_scale), cap, n_fam, engine.P(maxrow), engine.P(adj), engine.P(fam),
                       engine._stream()]
    keep = (d_tab, d_fp, d_scale, st, maxrow, adj, fam)
    k_design, k_family = _names(bs)
    return (lambda: _lib.call(k_design, *a_design)), (lambda: _lib.call(k_family, *a_family)), keep


def _report(tag, bs, family_ptr, tables, scale=None):
    design, family, keep = _launches(bs, family_ptr, tables, scale)
    t_d, p_d = _events(design, reps=3)
    t_f, p_f = _events(family, reps=3)
    fam = engine.host(keep[-1])
    k_design, k_family = _names(bs)
    print(f"{tag}: {len(family_ptr) - 1} families, {len(tables[0])} tests; {k_design} {t_d:.3f} ms (passes {[round(x, 3) for x in p_d]}); "
          f"{k_family} {t_f:.3f} ms (passes {[round(x, 3) for x in p_f]}); ratio {t_f / t_d:.2f}; "
          f"n_included {int(fam[:, 0, 1].min())}..{int(fam[:, 0, 1].max())}, n_valid {int(fam[:, 0, 0].min())}..{int(fam[:, 0, 0].max())}", flush=True)
    return t_d, t_f


def _synthetic(genes, groups, B, one_plane=False):
    gen = torch.Generator(device="cuda").manual_seed(1)
    if one_plane:
        bs = object.__new__(engine.Bootstrap2D)
        bs.yc = torch.randn((genes * groups, B + 1), dtype=torch.float64, device="cuda", generator=gen)
        bs.ld, bs.B, bs.ng, bs.n_pairs = B + 1, B, groups, genes
        print(f"plane: {genes} pairs x {groups} groups x {B + 1} columns, {bs.yc.numel() * 8 / 1e9:.2f} GB", flush=True)
        return bs
    bs = object.__new__(engine.Bootstrap1D)
    bs.ym = torch.randn((genes * groups, B + 1), dtype=torch.float64, device="cuda", generator=gen)
    bs.yv = torch.randn((genes * groups, B + 1), dtype=torch.float64, device="cuda", generator=gen)
    bs.ld, bs.B, bs.ng, bs.n_tested = B + 1, B, groups, genes
    print(f"planes: {genes} genes x {groups} groups x {B + 1} columns, {2 * bs.ym.numel() * 8 / 1e9:.2f} GB in both", flush=True)
    return bs


def kernels(genes, groups, B, control=None, one_plane=False):
    bs = _synthetic(genes, groups, B, one_plane)
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


def one_call_2d(cells, genes, n_guides, n_pairs, B):
    """One ht_2d_posthoc(approx=True) call on the shape of tools/bench_vs_control_2d.py (its matrix, groups and pairs), every guide
    against the control, and both kernels alone on that call's last pair chunk and tables."""
    import bench

    csr = bench.synth_device_csr(dict(cells=cells, genes=genes, density=0.05), 20250117 + 7, torch)
    rng = np.random.default_rng(20250117 + 7)
    is_ctrl = rng.random(cells) < 0.2
    guide = np.where(is_ctrl, 0, 1 + rng.integers(0, n_guides, size=cells))
    obs = pd.DataFrame({"guide": guide, "q": np.full(cells, 0.07)})
    adata = AnnDataLite(sp.csr_matrix((cells, genes), dtype=np.float32), obs, pd.DataFrame(index=[f"g{i}" for i in range(genes)]))
    memento.setup_memento(adata, q_column="q", device_csr=csr)
    memento.create_groups(adata, label_columns=["guide"])
    memento.compute_1d_moments(adata, min_perc_group=0.7, subset_var=False)
    m = adata.uns["memento"]
    names = memento.main._var_names(adata)
    mean_all = np.mean([m["1d_moments"][k][0] for k in m["groups"]], axis=0)
    n_top = max(8, int(np.ceil((1 + np.sqrt(1 + 8 * n_pairs)) / 2)) + 20)           # enough genes for n_pairs distinct pairs
    top = names[np.argsort(-mean_all, kind="stable")[:n_top]]
    iu, ju = np.triu_indices(len(top), 1)
    pick = rng.choice(len(iu), size=n_pairs, replace=False)
    memento.compute_2d_moments(adata, [(str(top[a]), str(top[b])) for a, b in zip(iu[pick], ju[pick])])
    ctrl = [g for g in m["groups"] if g.split("^")[-1] == "0"][0]
    st = m["_hip"]
    print(f"call: {cells} cells, {len(names)} genes kept of {genes}, {len(m['groups'])} groups, {n_pairs} pairs, B {B}", flush=True)
    times = []
    for run in range(2):                                             # run 0 is the warm-up
        np.random.seed(0)
        torch.cuda.synchronize(); t0 = time.time()
        df = memento.ht_2d_posthoc(adata, control=ctrl, num_boot=B, num_cpus=16, approx=True)
        torch.cuda.synchronize(); times.append(time.time() - t0)
        print(f"  ht_2d_posthoc run {run}{' (warm-up)' if run == 0 else ''}: {times[-1]:.3f} s", flush=True)
    bs, (lo, hi), last = st.last_bootstrap2d, st.last_chunk2d, st.last_posthoc2d
    t_d, t_f = _report(f"last chunk ({hi - lo} pairs)", bs, last.family_ptr, last.tables, last.scale)
    scale = n_pairs / max(1, hi - lo)                                # every pair has the same family: the kernels' time goes with the pairs
    print(f"ht_2d_posthoc (approx=True): {n_pairs} pairs, {len(df)} rows, finite corr_pval_adj {np.isfinite(df.corr_pval_adj).mean():.3f}, "
          f"{times[-1]:.3f} s a call; of it mm_family_maxt1 {t_f * scale / 1e3 / times[-1] * 100:.2f} %, mm_contrast_design1_stats "
          f"{t_d * scale / 1e3 / times[-1] * 100:.2f} %", flush=True)


def main():
    genes, groups, B = _opt("--genes", 2000), _opt("--groups", 20), _opt("--boot", 10000)
    levels, m2o_genes, m2o_boot = _opt("--levels", 500), _opt("--m2o-genes", 500), _opt("--m2o-boot", 5000)
    one_plane = "--one-plane" in sys.argv
    cells = _opt("--cells", 200_000 if one_plane else 100_000)
    call_genes, guides, n_pairs, call_boot = _opt("--call-genes", 15_000), _opt("--guides", 500), _opt("--pairs", 2_000), _opt("--call-boot", 5_000)
    no_call, no_kernels = "--no-call" in sys.argv, "--no-kernels" in sys.argv
    engine._lib.load(require_gpu=True)
    if not no_kernels:
        kernels(genes, groups, B, one_plane=one_plane)
        torch.cuda.empty_cache()
        if levels > 0:
            kernels(m2o_genes, levels + 1, m2o_boot, control=0, one_plane=one_plane)
            torch.cuda.empty_cache()
    if no_call:
        return
    if one_plane:
        one_call_2d(cells, call_genes, guides, n_pairs, call_boot)
    else:
        one_call(cells, int(genes * 1.5), groups, B)


if __name__ == "__main__":
    main()
