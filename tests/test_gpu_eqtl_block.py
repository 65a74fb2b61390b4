"""Kernel-level tests of mm_cross_resampled_block (include/memento_hip.h) through the C-ABI on hand-built planes: the gene-major
record of every test against the numpy record (``_replicate_ref._np_stats``) of the coefficient row that the per-test kernel
mm_cross_resampled returns for the same inputs, the keyed draws against their numpy restatement, and at the engine level the
rows-on-demand closure and the memory the call takes."""

import numpy as np
import pytest

from _replicate_ref import COUNT_COLUMNS, NAN_RECORD, _np_stats, cross_draws

pytestmark = pytest.mark.gpu

TT = 8                                                  # engine.CROSS_BLOCK_TT, asserted below
COUNTS = [TT + 1, 2 * TT + 3, 1, TT, 0, TT - 1]         # tests per gene: a partial last tile, three tiles, one test, a full tile, none, TT - 1


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    assert engine.CROSS_BLOCK_TT == TT
    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _problem(B, ng, seed=21, counts=COUNTS):
    """Six genes of ``ng`` groups with the good masks of the per-test kernel's problem -- all good, ten good (two bad), one good
    (every column degenerate), all good -- then all good and two bad again, and ``counts[g]`` tests each, gene-major.  Test 1 of
    gene 0 has ONE group that differs from the others' common treatment value: a column that misses that group is degenerate for
    this test and not for its neighbours.  Dropped columns for the col_map variant: gene 0 loses column 4, 60..94 and B, gene 1
    none, gene 2 five, gene 3 all but column 0 (n_valid = 1), gene 4 none, gene 5 column 2."""
    rng = np.random.default_rng(seed)
    n_genes, ld = len(counts), B + 2
    yt = rng.normal(0, 1, size=(n_genes * ng, ld))
    yt[:, B + 1:] = np.nan
    good = np.ones((n_genes, ng), dtype=bool)
    for g in (1, 5):
        good[g, [3, 7]] = False
        yt[g * ng + 3] = np.nan                                                # a bad group's rows are never read
    good[2] = False
    good[2, 5] = True
    gene_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    tt = rng.normal(0, 1, size=(int(gene_ptr[-1]), ng))
    tt[1] = 0.25
    tt[1, ng - 2] = -1.5
    Nc = rng.integers(200, 900, size=ng).astype(np.float64)
    col_map = np.zeros((n_genes, B + 1), dtype=np.int32)
    n_valid = np.zeros(n_genes, dtype=np.int32)
    for gene, dropped in enumerate([np.r_[4, 60:95, B], [], [1, 2, 3, 64, B - 1], np.arange(1, B + 1), [], [2]]):
        keep = np.setdiff1d(np.arange(B + 1), dropped)
        col_map[gene, :len(keep)] = keep
        n_valid[gene] = len(keep)
    return yt, good, gene_ptr, tt, Nc, col_map, n_valid


def _dev_or_none(eng, a, dtype):
    return eng.dev(np.ascontiguousarray(a, dtype=dtype)) if a is not None else None


def _per_test(eng, yt, B, ng, gene_ptr, tt, good, Nc, rep, bcol, col_map, n_valid, seed, key=None):
    """mm_cross_resampled (``key`` None) or mm_cross_resampled_keyed, one workgroup per test: (rows [n_tests][ld], records)."""
    import torch

    test_gene = np.repeat(np.arange(len(gene_ptr) - 1, dtype=np.int32), np.diff(gene_ptr))
    n_tests, ld = len(test_gene), yt.shape[1]
    coef, stats = eng.empty((n_tests, ld), torch.float64), eng.empty((n_tests, 8), torch.float64)
    d = [eng.dev(yt), eng.dev(test_gene), eng.dev(tt), eng.dev(good.astype(np.uint8)), eng.dev(Nc)]
    opt = [_dev_or_none(eng, rep, np.int16), _dev_or_none(eng, bcol, np.int32), _dev_or_none(eng, col_map, np.int32),
           _dev_or_none(eng, n_valid, np.int32)]
    if key is None:
        eng._lib.call("mm_cross_resampled", eng.P(d[0]), ld, B, ng, *map(eng.P, d[1:]), *map(eng.P, opt), int(seed), n_tests, eng.P(coef),
                      eng.P(stats), eng._stream())
    else:
        d_key = eng.dev(np.asarray(key, dtype=np.int64))
        eng._lib.call("mm_cross_resampled_keyed", eng.P(d[0]), ld, B, ng, *map(eng.P, d[1:]), *map(eng.P, opt), eng.P(d_key), int(seed),
                      n_tests, eng.P(coef), eng.P(stats), eng._stream())
    return eng.host(coef), eng.host(stats)


def _block(eng, yt, B, ng, gene_ptr, tt, good, Nc, rep, bcol, col_map, n_valid, seed, key=None, max_gene_tests=None):
    """mm_cross_resampled_block through the C-ABI: records [n_tests][8] on the host (pre-set to 7.0: every record must be written)."""
    import torch

    n_tests, ld = len(tt), yt.shape[1]
    stats = eng.dev(np.full((max(1, n_tests), 8), 7.0))
    d = [eng.dev(tt if n_tests else np.zeros((1, ng))), eng.dev(good.astype(np.uint8)), eng.dev(Nc)]
    opt = [_dev_or_none(eng, rep, np.int16), _dev_or_none(eng, bcol, np.int32), _dev_or_none(eng, col_map, np.int32),
           _dev_or_none(eng, n_valid, np.int32), _dev_or_none(eng, key, np.int64)]
    d_yt, d_ptr = eng.dev(yt), eng.dev(np.asarray(gene_ptr, dtype=np.int32))
    if max_gene_tests is None:
        max_gene_tests = int(np.diff(gene_ptr).max())
    eng._lib.call("mm_cross_resampled_block", eng.P(d_yt), ld, B, ng, eng.P(d_ptr), len(gene_ptr) - 1, max_gene_tests, *map(eng.P, d),
                  *map(eng.P, opt), int(seed), n_tests, eng.P(stats), eng._stream())
    torch.cuda.synchronize()
    return eng.host(stats)[:n_tests]


def _tables(good, n_valid, B, seed, keys):
    """rep / bcol [gene][group][B] from the numpy restatement of the draw rule, gene g under key ``keys[g]``."""
    n_genes, ng = good.shape
    rep, bcol = np.zeros((n_genes, ng, B), dtype=np.int16), np.zeros((n_genes, ng, B), dtype=np.int32)
    for g in range(n_genes):
        n, nb = int(good[g].sum()), (int(n_valid[g]) - 1 if n_valid is not None else B)
        if nb >= 1:
            rep[g, :n], bcol[g, :n] = cross_draws(seed, int(keys[g]), n, nb, B)
    return rep, bcol


def _assert_block_records(got, rows, st_ref, gene_ptr, n_valid, B, msg):
    """Every record of the block kernel against the numpy record of the per-test kernel's row: coef0, range and the count columns
    exactly, se and null_mean to the tolerance of a reduction in another order."""
    test_gene = np.repeat(np.arange(len(gene_ptr) - 1), np.diff(gene_ptr))
    assert len(got) == len(test_gene)
    for t, gene in enumerate(test_gene):
        nb = int(n_valid[gene]) - 1 if n_valid is not None else B
        m = f"{msg}, test {t} of gene {gene}"
        if nb < 1:
            want = NAN_RECORD
            assert np.isnan(rows[t, :B + 1]).all(), m
        else:
            want = _np_stats(np.r_[rows[t, :nb], np.full(B + 1 - nb, np.nan)])
        np.testing.assert_array_equal(_bits(got[t, [0, 7]]), _bits(want[[0, 7]]), err_msg=m)
        np.testing.assert_array_equal(got[t, COUNT_COLUMNS], want[COUNT_COLUMNS], err_msg=m)
        np.testing.assert_allclose(got[t, [1, 4]], want[[1, 4]], rtol=1e-11, atol=1e-12, equal_nan=True, err_msg=m)
    # the columns go to the threads and through the reductions as in the per-test kernel, so the record is that kernel's own
    np.testing.assert_array_equal(_bits(got), _bits(st_ref), err_msg=msg)


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("B", [63, 64, 65, 255, 256, 257, 700])
def test_block_records_against_the_per_test_rows(eng, B, dropped):
    """Tests per gene of 0, 1, TT - 1, TT, TT + 1 and 2 TT + 3 on the good masks of the per-test kernel's problem, with all columns
    and with some dropped through col_map / n_valid (one gene keeps column 0 alone: the NaN record).  Device draws, the same draws
    as tables, and gene_key = arange are bit-identical to each other; a test that is degenerate in columns where its neighbours
    are not has a smaller n_valid than they have."""
    ng, seed = 12, 0xDEADBEEF12345678
    yt, good, gene_ptr, tt, Nc, col_map, n_valid = _problem(B, ng)
    if not dropped:
        col_map = n_valid = None
    rows, st_ref = _per_test(eng, yt, B, ng, gene_ptr, tt, good, Nc, None, None, col_map, n_valid, seed)
    got = _block(eng, yt, B, ng, gene_ptr, tt, good, Nc, None, None, col_map, n_valid, seed)
    _assert_block_records(got, rows, st_ref, gene_ptr, n_valid, B, f"B {B}, dropped {dropped}")
    assert got[1, 2] < got[0, 2] == got[2, 2] and got[1, 2] > 0               # per-test validity inside one tile
    rep, bcol = _tables(good, n_valid, B, seed, np.arange(len(good)))
    by_table = _block(eng, yt, B, ng, gene_ptr, tt, good, Nc, rep, bcol, col_map, n_valid, seed + 1)      # tables: the seed is unused
    np.testing.assert_array_equal(_bits(by_table), _bits(got))
    by_key = _block(eng, yt, B, ng, gene_ptr, tt, good, Nc, None, None, col_map, n_valid, seed, key=np.arange(len(good)))
    np.testing.assert_array_equal(_bits(by_key), _bits(got))
    # a launch sized for more tests per gene than any gene has: the surplus workgroups write nothing
    wide = _block(eng, yt, B, ng, gene_ptr, tt, good, Nc, None, None, col_map, n_valid, seed, max_gene_tests=len(tt))
    np.testing.assert_array_equal(_bits(wide), _bits(got))


def test_both_entry_points_refuse_a_single_replicate(eng):
    """B = 1: mm_cross_resampled has no null to resample from one replicate and refuses the launch (num_boot > 1); there is no row to
    compare with, and the block entry point refuses alike."""
    B, ng = 1, 12
    yt, good, gene_ptr, tt, Nc, _, _ = _problem(B, ng)
    with pytest.raises(eng._lib.MementoHipError):
        _per_test(eng, yt, B, ng, gene_ptr, tt, good, Nc, None, None, None, None, 0)
    with pytest.raises(eng._lib.MementoHipError):
        _block(eng, yt, B, ng, gene_ptr, tt, good, Nc, None, None, None, None, 0)


def test_block_with_more_groups_than_threads(eng):
    """ng = 300 > the 256 threads of a workgroup (the staging loops stride), B = 70."""
    B, ng = 70, 300
    yt, good, gene_ptr, tt, Nc, col_map, n_valid = _problem(B, ng, seed=5)
    for cm, nv in ((None, None), (col_map, n_valid)):
        rows, st_ref = _per_test(eng, yt, B, ng, gene_ptr, tt, good, Nc, None, None, cm, nv, 3)
        got = _block(eng, yt, B, ng, gene_ptr, tt, good, Nc, None, None, cm, nv, 3)
        _assert_block_records(got, rows, st_ref, gene_ptr, nv, B, f"ng 300, dropped {cm is not None}")


@pytest.mark.parametrize("dropped", [False, True])
def test_gene_key_replaces_the_slot_in_the_draw_rule(eng, dropped):
    """A permuted key changes the replicate columns and not column 0, and the draws under key k are ``cross_draws(seed, k, ...)``:
    the keyed device draws equal the same kernel fed with tables restated in numpy for those keys, and the keyed per-test kernel."""
    B, ng, seed = 300, 12, 77
    yt, good, gene_ptr, tt, Nc, col_map, n_valid = _problem(B, ng)
    if not dropped:
        col_map = n_valid = None
    keys = np.array([4, 0, 3, 5, 1, 2 ** 31 + 9], dtype=np.int64)              # (a key above 2^31: the key is 64 bits wide)
    plain = _block(eng, yt, B, ng, gene_ptr, tt, good, Nc, None, None, col_map, n_valid, seed)
    keyed = _block(eng, yt, B, ng, gene_ptr, tt, good, Nc, None, None, col_map, n_valid, seed, key=keys)
    live = np.isfinite(plain[:, 0])
    assert live.sum() >= COUNTS[0] + COUNTS[1] + COUNTS[5]
    np.testing.assert_array_equal(_bits(keyed[:, 0]), _bits(plain[:, 0]))      # column 0 is the identity under every key
    assert (keyed[live, 1] != plain[live, 1]).all() and (keyed[live, 4] != plain[live, 4]).all()
    rep, bcol = _tables(good, n_valid, B, seed, keys)
    by_table = _block(eng, yt, B, ng, gene_ptr, tt, good, Nc, rep, bcol, col_map, n_valid, 0)
    np.testing.assert_array_equal(_bits(by_table), _bits(keyed))
    rows, st_keyed = _per_test(eng, yt, B, ng, gene_ptr, tt, good, Nc, None, None, col_map, n_valid, seed, key=keys)
    _assert_block_records(keyed, rows, st_keyed, gene_ptr, n_valid, B, f"keyed, dropped {dropped}")


def _bootstrap(eng, ym, yv, B, ng):
    """A Bootstrap1D that only holds replicate rows (what the statistics kernels read)."""
    bs = object.__new__(eng.Bootstrap1D)
    bs.ym, bs.yv, bs.ld, bs.B, bs.ng = eng.dev(ym), eng.dev(yv), ym.shape[1], B, ng
    bs.n_tested = bs.n_pairs = ym.shape[0] // ng
    return bs


def _engine_problem(n_genes, ng, B, per_gene, seed):
    rng = np.random.default_rng(seed)
    ld = B + 1
    ym, yv = rng.normal(0, 1, size=(n_genes * ng, ld)), rng.normal(0, 1, size=(n_genes * ng, ld))
    good = np.ones((n_genes, ng), dtype=bool)
    good[1, 2] = False
    masks = [np.ones(ng, dtype=bool), good[1]]
    M = np.zeros((2, ng, ng))
    for k, mask in enumerate(masks):                                           # the residual maker of an intercept, on the mask
        idx = np.flatnonzero(mask)
        M[k][np.ix_(idx, idx)] = np.eye(len(idx)) - 1.0 / len(idx)
    gene_mask = np.array([1 if g == 1 else 0 for g in range(n_genes)], dtype=np.int32)
    gene_ptr = np.arange(n_genes + 1) * per_gene
    tt = rng.normal(0, 1, size=(n_genes * per_gene, ng))
    Nc = rng.integers(200, 900, size=ng).astype(np.float64)
    return ym, yv, good, gene_mask, M, gene_ptr, tt, Nc


def test_engine_block_takes_no_memory_per_replicate_and_gives_rows_on_demand(eng):
    """8 genes x 16 groups, B = 2000, 512 tests per gene: one set of coefficient rows would be 65 MB; the scratch plane, tt, the
    records and the tables are under 4 MB, and the rise of the allocator's peak across ``cross_resampled_block`` on both planes
    stays below a quarter of n_tests x ld x 8 bytes.  The records equal those of ``contract_resampled`` (which stores the rows)
    and the ``rows`` closure returns its rows, for both planes, in any order of planes, into a caller's scratch."""
    import torch

    n_genes, ng, B, per_gene = 8, 16, 2000, 512
    ym, yv, good, gene_mask, M, gene_ptr, tt, Nc = _engine_problem(n_genes, ng, B, per_gene, seed=3)
    bs = _bootstrap(eng, ym, yv, B, ng)
    n_tests, ld = len(tt), bs.ld
    keys = np.arange(n_genes, dtype=np.int64)[::-1].copy()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    st_m, st_v, rows = bs.cross_resampled_block(gene_ptr, tt, good, gene_mask, M, Nc, seed=11, gene_key=keys)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 1e6:.2f} MB; one set of rows {n_tests * ld * 8 / 1e6:.1f} MB")
    assert rise < n_tests * ld * 8 / 4
    assert st_m.shape == st_v.shape == (n_tests, 8) and np.isfinite(st_m[:, :2]).all() and np.isfinite(st_v[:, :2]).all()
    # with key = slot the stored-row path of the engine is the reference: same records, same rows
    st_m0, st_v0, rows0 = bs.cross_resampled_block(gene_ptr, tt, good, gene_mask, M, Nc, seed=11)
    test_gene = np.repeat(np.arange(n_genes), per_gene)
    idx = np.array([0, 5, 511, 512, 1023, 1024, 4095, 2000, 7])
    for which, st in ((1, st_v0), (0, st_m0), (1, st_v0)):
        coef, st_ref = bs.contract_resampled(test_gene[idx], tt[idx], good, which, gene_mask, M, Nc, seed=11)
        np.testing.assert_array_equal(_bits(st[idx]), _bits(st_ref))
        got = rows0(which, idx)
        np.testing.assert_array_equal(_bits(got[:, :B + 1]), _bits(eng.host(coef)[:, :B + 1]))
    scratch = eng.empty((len(idx) + 2, ld), torch.float64)
    on_dev = rows0(0, idx, to_host=False, out=scratch)
    assert on_dev.data_ptr() == scratch.data_ptr()
    np.testing.assert_array_equal(_bits(eng.host(on_dev)), _bits(rows0(0, idx)))
    # the keyed closure: its rows give the keyed records
    got = rows(0, idx)
    for k, t in enumerate(idx):
        np.testing.assert_array_equal(st_m[t, COUNT_COLUMNS], _np_stats(got[k, :B + 1])[COUNT_COLUMNS])
        assert st_m[t, 0] == got[k, 0] == st_m0[t, 0]
    assert (st_m[:per_gene, 1] != st_m0[:per_gene, 1]).all()                  # gene 0 under key 7: other draws


def test_engine_block_checks_its_tables_on_the_host(eng):
    """The kernel trusts the tables: a pointer that is no CSR over tt, a mask index past M, draws that leave the good groups or
    the surviving columns, a negative key and a wrong n_valid all raise before anything is launched."""
    n_genes, ng, B, per_gene = 3, 6, 40, 2
    ym, yv, good, gene_mask, M, gene_ptr, tt, Nc = _engine_problem(n_genes, ng, B, per_gene, seed=4)
    bs = _bootstrap(eng, ym, yv, B, ng)
    rep, bcol = _tables(good, None, B, 0, np.arange(n_genes))
    bs.cross_resampled_block(gene_ptr, tt, good, gene_mask, M, Nc, rep=rep, bcol=bcol)
    bad_rep, bad_bcol = rep.copy(), bcol.copy()
    bad_rep[1, 0, 3] = 5                                                       # gene 1 has five good groups: 0..4
    bad_bcol[2, 1, 7] = B + 1
    for kwargs in (dict(gene_ptr=gene_ptr[:-1]), dict(gene_ptr=gene_ptr + 1), dict(gene_ptr=[0, 4, 2, 6]), dict(gene_mask=[0, 2, 0]),
                   dict(rep=bad_rep, bcol=bcol), dict(rep=rep, bcol=bad_bcol), dict(rep=rep), dict(gene_key=[0, -1, 2]),
                   dict(n_valid=[B + 2, 1, 1]), dict(tt=tt[:, :-1]), dict(good=good[:2])):
        args = dict(gene_ptr=gene_ptr, tt=tt, good=good, gene_mask=gene_mask, M=M, Nc=Nc)
        args.update(kwargs)
        with pytest.raises(ValueError):
            bs.cross_resampled_block(**args)
