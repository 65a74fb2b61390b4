"""The joint test of a treatment block: mm_joint_stats against the r-row contraction it replaces, and its share of one ht_1d_joint call.

Part 1, synthetic replicate planes (--genes x --groups rows of B + 1 normal values, generated on the device): for every rank r of
--ranks (a one-way factor of r + 1 levels over the groups, cell counts unequal)
  * mm_joint_stats: one launch, both planes, nothing stored per replicate;
  * mm_contract_stats given the same r weight rows per gene on the same planes: one launch per plane, r tests per gene, each reading
    the gene's rows again and storing its coefficient row -- what a caller without the joint kernel would run before squaring and
    summing the rows on its own (that step is not timed).
HIP events around back-to-back launches after a warm-up, median of three passes.
Part 2 (skipped with --no-call; --no-kernels skips part 1): a synthetic count matrix with --groups groups (levels x 4 replicates), one ht_1d_joint call timed by
the host clock around a device synchronise, and mm_joint_stats alone on that call's last chunk and designs.
One-plane mode (--one-plane; nothing else runs): ONE synthetic plane of --genes row blocks (the pairs of ht_2d_joint) x --groups rows,
the designs of part 1, and for every rank
  * mm_joint1_stats on the plane: one record per test;
  * mm_joint_stats given that plane as both of its planes -- the only way to run the test without the one-plane kernel: the baseline.
Timed as in part 1.  n_groups chooses the instantiation: <8> up to 8 groups, <32> up to 32, <0> beyond.
usage: python tools/bench_joint.py [--genes 2000] [--groups 20] [--boot 10000] [--ranks 4,19] [--cells 100000] [--no-call] [--no-kernels]
                                   [--one-plane]"""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, pandas as pd, torch, scipy.sparse as sp
from scrna_parameter_estimation_amd import AnnDataLite, _lib, engine, memento
from scrna_parameter_estimation_amd.memento import _ht


def _opt(name, default, conv=int):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = conv(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return v
    return default


def _events(fn, reps, passes=3, warm=2):
    """Median over ``passes`` of the time per call of ``reps`` back-to-back calls of ``fn`` (ms, HIP events on the launch stream)."""
    timer, ms, stream = ctypes.c_void_p(), ctypes.c_float(), engine._stream()
    _lib.call("mm_timer_create", ctypes.byref(timer))
    for _ in range(warm):
        fn()
    out = []
    for _ in range(passes):
        _lib.call("mm_timer_begin", timer, stream)
        for _ in range(reps):
            fn()
        _lib.call("mm_timer_end", timer, stream)
        _lib.call("mm_timer_elapsed_ms", timer, ctypes.byref(ms))
        out.append(ms.value / reps)
    _lib.call("mm_timer_destroy", timer)
    return sorted(out)[len(out) // 2], out


def _joint_launch(bs, test_gene, tables):
    """mm_joint_stats with everything uploaded once: -> a function that only launches."""
    test_gene, d_tab = engine._joint_tables(test_gene, tables, bs.n_tested, bs.ng)
    n = len(test_gene)
    st_m, st_v = engine.empty((n, 8), torch.float64), engine.empty((n, 8), torch.float64)
    args = [engine.P(bs.ym), engine.P(bs.yv), bs.ld, bs.B, bs.ng, *map(engine.P, d_tab), n, engine.P(st_m), engine.P(st_v), engine._stream()]
    keep = (d_tab, st_m, st_v)
    return lambda: _lib.call("mm_joint_stats", *args), keep


def kernels(genes, groups, B, ranks):
    ld = B + 1
    bs = object.__new__(engine.Bootstrap1D)
    gen = torch.Generator(device="cuda").manual_seed(1)
    bs.ym = torch.randn((genes * groups, ld), dtype=torch.float64, device="cuda", generator=gen)
    bs.yv = torch.randn((genes * groups, ld), dtype=torch.float64, device="cuda", generator=gen)
    bs.ld, bs.B, bs.ng, bs.n_tested = ld, B, groups, genes
    Nc = np.random.default_rng(2).integers(200, 3000, size=groups).astype(np.float64)
    good = np.ones((genes, groups), dtype=bool)
    print(f"planes: {genes} genes x {groups} groups x {ld} columns, {2 * bs.ym.numel() * 8 / 1e9:.2f} GB in both", flush=True)
    for r in ranks:
        levels = np.arange(groups) % (r + 1)
        trt = np.stack([(levels == v).astype(np.float64) for v in range(1, r + 1)], axis=1)
        tables = _ht.joint_tables(good, np.ones((groups, 0)), trt, Nc)
        assert list(tables.design_rank) == [r]
        L = tables.design_L.reshape(r, groups)
        launch, keep = _joint_launch(bs, np.arange(genes), tables)
        t_joint, p_joint = _events(launch, reps=5)
        # the same forms as r contraction tests per gene, one launch per plane, coefficient rows stored
        n_tests = genes * r
        d_tg, d_W = engine.dev(np.repeat(np.arange(genes), r).astype(np.int32)), engine.dev(np.tile(L, (genes, 1)))
        d_good = engine.dev(good.astype(np.uint8))
        coef, stats = engine.empty((n_tests, ld), torch.float64), engine.empty((n_tests, 8), torch.float64)

        def contract():
            for which in (0, 1):
                _lib.call("mm_contract_stats", engine.P(bs.ym), engine.P(bs.yv), ld, B, groups, engine.P(d_tg), engine.P(d_W), engine.P(d_good),
                          n_tests, which, engine.P(coef), engine.P(stats), engine._stream())

        t_con, p_con = _events(contract, reps=3)
        flops = 2 * 4.0 * genes * B * r * groups             # two passes; a multiply and an add on each plane per (form, group, column)
        print(f"r = {r}: mm_joint_stats {t_joint:.3f} ms (passes {[round(x, 3) for x in p_joint]}), {flops / t_joint / 1e9:.2f} TFLOP/s fp64 in the forms; "
              f"mm_contract_stats x 2 planes, {n_tests} tests: {t_con:.3f} ms (passes {[round(x, 3) for x in p_con]}), "
              f"{coef.numel() * 8 / 1e9:.2f} GB of rows stored per plane; ratio {t_con / t_joint:.2f}", flush=True)
        del coef, stats, d_W, keep, launch
    del bs


def one_plane(pairs, groups, B, ranks):
    ld = B + 1
    gen = torch.Generator(device="cuda").manual_seed(1)
    y = torch.tanh(0.6 * torch.randn((pairs * groups, ld), dtype=torch.float64, device="cuda", generator=gen))
    two = object.__new__(engine.Bootstrap1D)
    two.ym, two.yv, two.ld, two.B, two.ng, two.n_tested = y, y, ld, B, groups, pairs
    Nc = np.random.default_rng(2).integers(200, 3000, size=groups).astype(np.float64)
    good = np.ones((pairs, groups), dtype=bool)
    tier = 8 if groups <= 8 else 32 if groups <= 32 else 0
    print(f"plane: {pairs} pairs x {groups} groups x {ld} columns, {y.numel() * 8 / 1e9:.2f} GB; instantiation <{tier}>", flush=True)
    for r in ranks:
        levels = np.arange(groups) % (r + 1)
        trt = np.stack([(levels == v).astype(np.float64) for v in range(1, r + 1)], axis=1)
        tables = _ht.joint_tables(good, np.ones((groups, 0)), trt, Nc)
        assert list(tables.design_rank) == [r]
        test_pair, d_tab = engine._joint_tables(np.arange(pairs), tables, pairs, groups)
        stats = engine.empty((pairs, 8), torch.float64)
        args = [engine.P(y), ld, B, groups, *map(engine.P, d_tab), pairs, engine.P(stats), engine._stream()]
        t_one, p_one = _events(lambda: _lib.call("mm_joint1_stats", *args), reps=5)
        launch, keep = _joint_launch(two, np.arange(pairs), tables)
        t_two, p_two = _events(launch, reps=5)
        print(f"r = {r}: mm_joint1_stats {t_one:.3f} ms (passes {[round(x, 3) for x in p_one]}), {2 * y.numel() * 8 / t_one / 1e9:.2f} TB/s over its two "
              f"passes; mm_joint_stats with the plane twice {t_two:.3f} ms (passes {[round(x, 3) for x in p_two]}); ratio {t_two / t_one:.2f}", flush=True)
        del keep, launch, stats, d_tab


def one_call(cells, genes, groups, B):
    import bench

    n_rep = 4
    n_lev = max(2, groups // n_rep)
    csr = bench.synth_device_csr(dict(cells=cells, genes=genes, density=0.1), 20250117 + 11, torch)
    rng = np.random.default_rng(3)
    grp = rng.integers(0, n_lev * n_rep, size=cells)
    obs = pd.DataFrame({"level": grp // n_rep, "rep": grp % n_rep, "q": np.full(cells, 0.07)})
    adata = AnnDataLite(sp.csr_matrix((cells, genes), dtype=np.float32), obs, pd.DataFrame(index=[f"g{i}" for i in range(genes)]))
    memento.setup_memento(adata, q_column="q", device_csr=csr)
    memento.create_groups(adata, label_columns=["level", "rep"])
    memento.compute_1d_moments(adata, min_perc_group=0.7, subset_var=False)
    st = adata.uns["memento"]["_hip"]
    print(f"call: {cells} cells, {len(st.gene_idx)} genes kept of {genes}, {n_lev} levels x {n_rep} replicates, B {B}", flush=True)
    times = []
    for run in range(3):                                             # run 0 is the warm-up
        np.random.seed(0)
        torch.cuda.synchronize(); t0 = time.time()
        df = memento.ht_1d_joint(adata, "level", covariate=["rep"], num_boot=B)
        torch.cuda.synchronize(); times.append(time.time() - t0)
        print(f"  ht_1d_joint run {run}{' (warm-up)' if run == 0 else ''}: {times[-1]:.3f} s", flush=True)
    bs, (g0, g1) = st.last_bootstrap, st.last_chunk
    launch, keep = _joint_launch(bs, np.arange(g1 - g0), st.last_joint_tables)
    t_k, passes = _events(launch, reps=5)
    t_call = float(np.median(times[1:]))
    scale = len(df) / max(1, g1 - g0)                                # the call's chunks are equal but for the last
    print(f"ht_1d_joint: {len(df)} genes, df {sorted(set(df['df']))}, {t_call:.3f} s a call; mm_joint_stats on the last chunk ({g1 - g0} genes): "
          f"{t_k:.3f} ms (passes {[round(x, 3) for x in passes]}) -> {t_k * scale / 1e3 / t_call * 100:.2f} % of the call", flush=True)


def main():
    genes, groups, B = _opt("--genes", 2000), _opt("--groups", 20), _opt("--boot", 10000)
    ranks = [int(x) for x in _opt("--ranks", "4,19", str).split(",")]
    cells = _opt("--cells", 100_000)
    no_call, no_kernels = "--no-call" in sys.argv, "--no-kernels" in sys.argv
    engine._lib.load(require_gpu=True)
    if "--one-plane" in sys.argv:
        return one_plane(genes, groups, B, ranks)
    if not no_kernels:
        kernels(genes, groups, B, ranks)
    if not no_call:
        torch.cuda.empty_cache()
        one_call(cells, int(genes * 1.5), groups, B)


if __name__ == "__main__":
    main()
