"""Kernel-level tests of the gene-major resampled tests with a covariate PER TEST (mm_cross_cov_beta, mm_cross_resampled_block_cov,
mm_residualize_rank1 of include/memento_hip.h) through the C-ABI on hand-built planes: against mm_cross_resampled_block where the
covariate is zero, against mm_cross_resampled_keyed on the materialised responses bit for bit, against the numpy restatement
(``_eqtl_cov_ref``) inside its derived bound, and the tile range and scratch of the entry points."""

import numpy as np
import pytest

import _eqtl_cov_ref as ref
from _replicate_ref import COUNT_COLUMNS, NAN_RECORD, _np_stats

pytestmark = pytest.mark.gpu

TT = ref.TT
FILL = 7.0


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    assert engine.CROSS_BLOCK_TT == TT
    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _opt(eng, a, dtype):
    return eng.dev(np.ascontiguousarray(a, dtype=dtype)) if a is not None else None


def _n_tiles(gene_ptr):
    return (len(gene_ptr) - 1) * ((int(np.diff(gene_ptr).max()) + TT - 1) // TT)


class Problem:
    """A problem of ``ref.cov_problem`` on the device, with the draws as tables (``tables=True``) or made on the device under KEYS."""

    def __init__(self, eng, B, ng, dropped, tables, seed=21):
        self.eng, self.B, self.ng = eng, B, ng
        yt, self.good, self.gene_ptr, self.tt, self.zt, self.Nc, col_map, n_valid = ref.cov_problem(B, ng, seed=seed)
        self.col_map, self.n_valid = (col_map, n_valid) if dropped else (None, None)
        self.yt = ref.poison_dropped(yt, self.good, col_map, n_valid) if dropped else yt
        self.ld = yt.shape[1]
        self.keys = np.asarray(ref.KEYS, dtype=np.int64)
        self.rep, self.bcol = ref.draw_tables(self.good, self.n_valid, B, ref.SEED, self.keys)      # the restatement always has tables
        self.tables = tables
        self.test_gene = np.repeat(np.arange(len(self.good), dtype=np.int32), np.diff(self.gene_ptr))
        self.n_tiles = _n_tiles(self.gene_ptr)
        self.d_yt, self.d_ptr, self.d_good, self.d_nc = eng.dev(self.yt), eng.dev(self.gene_ptr), eng.dev(self.good.astype(np.uint8)), eng.dev(self.Nc)
        self.d_tt = eng.dev(self.tt)

    def draws(self, genes=None):
        """(rep, bcol, col_map, n_valid, key) device tensors or None, for all genes or gathered for the row blocks ``genes``."""
        g = slice(None) if genes is None else genes
        e = self.eng
        rep, bcol = (self.rep[g], self.bcol[g]) if self.tables else (None, None)
        cm, nv = (self.col_map[g], self.n_valid[g]) if self.col_map is not None else (None, None)
        return [_opt(e, rep, np.int16), _opt(e, bcol, np.int32), _opt(e, cm, np.int32), _opt(e, nv, np.int32),
                None if self.tables else _opt(e, self.keys[g], np.int64)]

    def seed(self):
        return 1 if self.tables else ref.SEED                                  # (tables: the seed is unused)

    def block(self):
        """mm_cross_resampled_block: records [n_tests][8]."""
        e = self.eng
        stats = e.dev(np.full((len(self.tt), 8), FILL))
        e._lib.call("mm_cross_resampled_block", e.P(self.d_yt), self.ld, self.B, self.ng, e.P(self.d_ptr), len(self.good),
                    int(np.diff(self.gene_ptr).max()), e.P(self.d_tt), e.P(self.d_good), e.P(self.d_nc), *map(e.P, self.draws()), self.seed(),
                    len(self.tt), e.P(stats), e._stream())
        return e.host(stats)

    def block_cov(self, zt, ranges=None, scratch_tiles=None, stats=None):
        """mm_cross_resampled_block_cov over the tile ranges ``ranges`` (default: all tiles in one launch) through a beta scratch of
        ``scratch_tiles`` tiles and one more, pre-set to FILL: (records, the scratch on the host [scratch_tiles + 1][ld][TT])."""
        e = self.eng
        ranges = [(0, self.n_tiles)] if ranges is None else ranges
        scratch_tiles = max(hi - lo for lo, hi in ranges) if scratch_tiles is None else scratch_tiles
        beta = e.dev(np.full((scratch_tiles + 1, self.ld, TT), FILL))
        stats = e.dev(np.full((len(self.tt), 8), FILL)) if stats is None else stats
        d_zt, tabs = e.dev(zt), self.draws()
        for lo, hi in ranges:
            assert hi - lo <= scratch_tiles
            e._lib.call("mm_cross_resampled_block_cov", e.P(self.d_yt), self.ld, self.B, self.ng, e.P(self.d_ptr), len(self.good),
                        int(np.diff(self.gene_ptr).max()), e.P(self.d_tt), e.P(d_zt), e.P(self.d_good), e.P(self.d_nc), *map(e.P, tabs),
                        self.seed(), len(self.tt), lo, hi, e.P(beta), e.P(stats), e._stream())
        return e.host(stats), e.host(beta)

    def materialised(self, zt):
        """mm_residualize_rank1 for every test, then mm_cross_resampled_keyed on the copies (test l on row block l with the tables of
        its gene): (rows [n_tests][ld], records, the copies [n_tests][ng][ld])."""
        import torch

        e, n = self.eng, len(self.tt)
        copies = e.dev(np.full((n * self.ng, self.ld), FILL))
        d_tg, d_zt = e.dev(self.test_gene), e.dev(zt)
        e._lib.call("mm_residualize_rank1", e.P(self.d_yt), self.ld, self.B, self.ng, e.P(d_tg), e.P(d_zt), e.P(self.d_good), e.P(self.d_nc), n,
                    e.P(copies), e._stream())
        rows, stats = e.dev(np.full((n, self.ld), FILL)), e.dev(np.full((n, 8), FILL))
        own, tabs = e.dev(np.arange(n, dtype=np.int32)), self.draws(self.test_gene)
        d_good = e.dev(self.good[self.test_gene].astype(np.uint8))
        e._lib.call("mm_cross_resampled_keyed", e.P(copies), self.ld, self.B, self.ng, e.P(own), e.P(self.d_tt), e.P(d_good), e.P(self.d_nc),
                    *map(e.P, tabs), self.seed(), n, e.P(rows), e.P(stats), e._stream())
        torch.cuda.synchronize()
        return e.host(rows), e.host(stats), e.host(copies).reshape(n, self.ng, self.ld)

    def nb(self, gene):
        return int(self.n_valid[gene]) - 1 if self.n_valid is not None else self.B


WORST = {}


@pytest.mark.parametrize("tables", [True, False])
@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("B", [63, 64, 65, 257])
def test_records_rows_and_restatement(eng, B, dropped, tables):
    """Tests per gene of 0, 1, TT - 1, TT, TT + 1 and 2 TT + 3 on masks all good / two bad / one good, all columns or some dropped
    (NaN there in the plane: beta is NaN in those columns and nobody reads it), draws from tables or made on the device under keys."""
    p = Problem(eng, B, 12, dropped, tables)
    n_tests = len(p.tt)
    # (1) a zero covariate: beta = 0, y - 0 = y -- the records of mm_cross_resampled_block, bit for bit
    plain = p.block()
    zero, _ = p.block_cov(np.zeros_like(p.zt))
    np.testing.assert_array_equal(_bits(zero), _bits(plain))
    # (2) the records equal those of the per-test kernel on the materialised responses, bit for bit; every record is written
    got, beta = p.block_cov(p.zt)
    rows, st_rows, copies = p.materialised(p.zt)
    assert not (got == FILL).all(axis=1).any()
    np.testing.assert_array_equal(_bits(got), _bits(st_rows))
    assert (beta[-1] == FILL).all()                                            # the scratch beyond the batch keeps its fill value
    live = np.isfinite(got[:, 0])
    assert live.sum() >= ref.COUNTS[0] + ref.COUNTS[1] + ref.COUNTS[5]
    assert got[1, 2] < got[0, 2] == got[2, 2] and got[1, 2] > 0               # test 1 of gene 0: degenerate where its neighbours are not
    z = ref.ZERO_Z_TEST                                                        # one zero covariate row among non-zero ones
    np.testing.assert_array_equal(_bits(got[z]), _bits(plain[z]))
    others = np.setdiff1d(np.flatnonzero(live), [z])
    assert (got[others, 0] != plain[others, 0]).all()
    # (3) every coefficient row against the numpy restatement, inside the bound it derives from its own sums of absolute terms
    want, bound = ref.cov_rows(p.yt, p.good, p.gene_ptr, p.tt, p.zt, p.Nc, p.rep, p.bcol, p.col_map, p.n_valid, B)
    worst, open_cells, cells = 0.0, 0, 0
    for t, gene in enumerate(p.test_gene):
        nb, m = p.nb(gene), f"B {B} dropped {dropped} tables {tables}: test {t} of gene {gene}"
        if nb < 1 or not p.good[gene].any():
            np.testing.assert_array_equal(got[t], NAN_RECORD, err_msg=m)
            assert np.isnan(rows[t, :B + 1]).all(), m
            continue
        r, w, b = rows[t, :nb], want[t, :nb], bound[t, :nb]
        np.testing.assert_array_equal(np.isnan(r), np.isnan(w), err_msg=m)
        assert np.isnan(rows[t, nb:B + 1]).all(), m
        ok = ~np.isnan(w)
        ratio = (np.abs(r[ok].astype(ref.L) - w[ok]) / b[ok]).astype(np.float64)
        if ok.any():
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, f"{m}: column {np.flatnonzero(ok)[ratio.argmax()]} is {ratio.max():.3g} of its bound"
        # the record is the record of its row; the counts also against the restatement wherever the bound decides them
        full = np.r_[r, np.full(B + 1 - nb, np.nan)]
        st = _np_stats(full)
        np.testing.assert_array_equal(_bits(got[t, [0, 7]]), _bits(st[[0, 7]]), err_msg=m)
        np.testing.assert_array_equal(got[t, COUNT_COLUMNS], st[COUNT_COLUMNS], err_msg=m)
        assert got[t, 2] == ok[1:].sum(), m
        lo, hi, n_open = ref.count_limits(np.r_[w, np.full(B + 1 - nb, np.nan)], np.r_[b, np.full(B + 1 - nb, np.nan)])
        assert lo[0] <= got[t, 3] <= hi[0] and lo[1] <= got[t, 6] <= hi[1], m
        open_cells, cells = open_cells + n_open, cells + int(ok[1:].sum())
        if ok[1:].any():
            big = 2 * float(np.nanmax(b))
            ref_st = _np_stats(np.r_[w, np.full(B + 1 - nb, np.nan)].astype(np.float64))
            np.testing.assert_allclose(got[t, [1, 4]], ref_st[[1, 4]], rtol=1e-11, atol=1e-12 + big, err_msg=m)
    assert cells > 20 * B and open_cells <= 0.01 * cells
    WORST[(B, dropped, tables)] = worst
    print(f"B {B} dropped {dropped} tables {tables}: largest |coefficient - restatement| / bound {worst:.3g}; "
          f"{open_cells} of {cells} cells left out of the count check")
    # (4) the materialised response and beta themselves
    for t in (0, z, n_tests - 1):
        gene = p.test_gene[t]
        b_ref, b_bound = ref.cov_beta(p.yt[gene * 12:(gene + 1) * 12], p.zt[t], p.Nc, p.good[gene])
        tile = gene * (p.n_tiles // len(p.good)) + (t - p.gene_ptr[gene]) // TT
        b_got = beta[tile, :B + 1, (t - p.gene_ptr[gene]) % TT]
        fin = np.isfinite(b_ref.astype(np.float64))[:B + 1]
        np.testing.assert_array_equal(np.isfinite(b_got), fin)
        assert (np.abs(b_got[fin].astype(ref.L) - b_ref[:B + 1][fin]) <= b_bound[:B + 1][fin]).all()
        idx = np.flatnonzero(p.good[gene])
        with np.errstate(invalid="ignore"):                                    # (NaN where beta is: the dropped columns)
            np.testing.assert_array_equal(copies[t][idx][:, :B + 1], p.yt[gene * 12 + idx][:, :B + 1] - p.zt[t][idx, None] * b_got[None, :])
        assert np.isnan(copies[t][~p.good[gene]][:, :B + 1]).all() and (copies[t][:, B + 1:] == FILL).all()


@pytest.mark.parametrize("dropped", [False, True])
def test_tile_ranges_change_no_bit_and_bound_the_scratch(eng, dropped):
    """One tile per launch through a scratch of ONE tile against all tiles in one launch: identical records; a launch over a range
    writes the records of its tiles and no other; an empty range does nothing; a range past the last tile is refused."""
    p = Problem(eng, 65, 12, dropped, tables=False)
    whole, _ = p.block_cov(p.zt)
    single, beta = p.block_cov(p.zt, ranges=[(k, k + 1) for k in range(p.n_tiles)], scratch_tiles=1)
    np.testing.assert_array_equal(_bits(single), _bits(whole))
    assert (beta[1] == FILL).all() and not (beta[0, :66] == FILL).all()
    tiles_per_gene = p.n_tiles // len(p.good)
    part, _ = p.block_cov(p.zt, ranges=[(tiles_per_gene, 2 * tiles_per_gene)])                            # gene 1 alone
    mine = p.test_gene == 1
    np.testing.assert_array_equal(_bits(part[mine]), _bits(whole[mine]))
    assert (part[~mine] == FILL).all()
    nothing, beta = p.block_cov(p.zt, ranges=[(3, 3)], scratch_tiles=1)
    assert (nothing == FILL).all() and (beta == FILL).all()
    with pytest.raises(eng._lib.MementoHipError):
        p.block_cov(p.zt, ranges=[(0, p.n_tiles + 1)], scratch_tiles=p.n_tiles + 1)


def test_more_groups_than_threads(eng):
    """ng = 300 > the 256 threads of a workgroup (the staging loops stride), B = 70: block against the materialised route, and a
    zero covariate against the plain block kernel."""
    for dropped in (False, True):
        p = Problem(eng, 70, 300, dropped, tables=False, seed=5)
        got, _ = p.block_cov(p.zt)
        rows, st_rows, _ = p.materialised(p.zt)
        np.testing.assert_array_equal(_bits(got), _bits(st_rows))
        assert np.isfinite(got[p.test_gene == 0]).all()
        np.testing.assert_array_equal(_bits(p.block_cov(np.zeros_like(p.zt))[0]), _bits(p.block()))


def _bootstrap(eng, ym, yv, B, ng):
    """A Bootstrap1D that only holds replicate rows (what the statistics kernels read)."""
    bs = object.__new__(eng.Bootstrap1D)
    bs.ym, bs.yv, bs.ld, bs.B, bs.ng = eng.dev(ym), eng.dev(yv), ym.shape[1], B, ng
    bs.n_tested = bs.n_pairs = ym.shape[0] // ng
    return bs


def test_engine_slices_by_the_scratch_and_gives_rows(eng):
    """``cross_resampled_block(zt=...)``: a scratch of one tile (and of one materialised test) against the default gives identical
    records and rows on both planes; the rows carry the records' counts; zt = 0 is the plain call; the family variant refuses."""
    rng = np.random.default_rng(8)
    n_genes, ng, B, per_gene = 5, 16, 120, 11
    ld = B + 1
    ym, yv = rng.normal(size=(n_genes * ng, ld)), rng.normal(size=(n_genes * ng, ld))
    good = np.ones((n_genes, ng), dtype=bool)
    good[1, 2] = False
    M = np.zeros((2, ng, ng))
    for k, mask in enumerate([np.ones(ng, dtype=bool), good[1]]):
        idx = np.flatnonzero(mask)
        M[k][np.ix_(idx, idx)] = np.eye(len(idx)) - 1.0 / len(idx)
    gene_mask = np.array([0, 1, 0, 0, 0], dtype=np.int32)
    gene_ptr = np.arange(n_genes + 1) * per_gene
    tt, zt = rng.normal(size=(n_genes * per_gene, ng)), rng.normal(size=(n_genes * per_gene, ng))
    Nc = rng.integers(200, 900, size=ng).astype(np.float64)
    keys = np.arange(n_genes, dtype=np.int64)[::-1].copy()
    bs = _bootstrap(eng, ym, yv, B, ng)
    args = (gene_ptr, tt, good, gene_mask, M, Nc)
    st_m, st_v, rows = bs.cross_resampled_block(*args, seed=11, gene_key=keys, zt=zt)
    st_m1, st_v1, rows1 = bs.cross_resampled_block(*args, seed=11, gene_key=keys, zt=zt, beta_scratch_bytes=1)
    np.testing.assert_array_equal(_bits(st_m1), _bits(st_m))
    np.testing.assert_array_equal(_bits(st_v1), _bits(st_v))
    assert np.isfinite(st_m[:, :2]).all() and np.isfinite(st_v[:, :2]).all()
    idx = np.array([0, 54, 11, 10, 12, 33])
    for which, st in ((1, st_v), (0, st_m), (1, st_v)):
        got = rows(which, idx)
        np.testing.assert_array_equal(_bits(rows1(which, idx)), _bits(got))
        for k, t in enumerate(idx):
            want = _np_stats(got[k, :B + 1])
            np.testing.assert_array_equal(st[t, COUNT_COLUMNS], want[COUNT_COLUMNS])
            np.testing.assert_array_equal(_bits(st[t, [0, 7]]), _bits(want[[0, 7]]))
    st_p, _, rows_p = bs.cross_resampled_block(*args, seed=11, gene_key=keys)
    st_z, _, rows_z = bs.cross_resampled_block(*args, seed=11, gene_key=keys, zt=np.zeros_like(zt))
    np.testing.assert_array_equal(_bits(st_z), _bits(st_p))
    np.testing.assert_array_equal(_bits(rows_z(0, idx)[:, :B + 1]), _bits(rows_p(0, idx)[:, :B + 1]))
    assert (st_m[:, 0] != st_p[:, 0]).all()
    with pytest.raises(NotImplementedError):
        bs.cross_resampled_family(*args, seed=11, zt=zt)
    with pytest.raises(ValueError, match="zt"):
        bs.cross_resampled_block(*args, zt=zt[:-1])
