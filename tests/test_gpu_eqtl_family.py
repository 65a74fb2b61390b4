"""Kernel-level tests of mm_cross_resampled_family (include/memento_hip.h) through the C-ABI on hand-built planes: the maximum row
of every gene bit for bit against the numpy restatement of the rule (``_eqtl_family_ref``) applied to the coefficient rows that
the per-test kernel mm_cross_resampled_keyed returns for the same inputs, with coef0 from the block kernel's records and the
scale from ``engine.family_scale``; the counts and the family sizes exactly; and, at the engine level, the ``family`` closure."""

import numpy as np
import pytest

import _eqtl_family_ref as ref
from _replicate_ref import cross_draws

pytestmark = pytest.mark.gpu

TT = 8                                                  # engine.CROSS_BLOCK_TT, asserted below
COUNTS = [TT + 1, 2 * TT + 3, 1, TT, 0, TT - 1]         # tests per gene: a partial last tile, three tiles, one test, a full tile, none, TT - 1
NG, SEED = 12, 0xDEADBEEF12345678
PAD = 3                                                 # cells of a maxrow row beyond num_boot: never written


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    assert engine.CROSS_BLOCK_TT == TT
    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _problem(B, ng=NG, seed=21, counts=COUNTS):
    """Six genes of ``ng`` groups: good masks all good, ten good (two bad), one good (every column degenerate), all good, all
    good, two bad, and ``counts[g]`` tests each, gene-major.  Test 1 of gene 0 has ONE group that differs from the others' common
    treatment value: a slot that misses that group is degenerate for this member and not for its neighbours.  Dropped columns for
    the col_map variant: gene 0 loses column 4, 60..94 and B, gene 1 none, gene 2 five, gene 3 all but column 0 (n_valid = 1),
    gene 4 none, gene 5 column 2."""
    rng = np.random.default_rng(seed)
    n_genes, ld = len(counts), B + 1 + PAD
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


def _tables(good, n_valid, B, seed, keys):
    """rep / bcol [gene][group][B] from the numpy restatement of the draw rule, gene g under key ``keys[g]``."""
    n_genes, ng = good.shape
    rep, bcol = np.zeros((n_genes, ng, B), dtype=np.int16), np.zeros((n_genes, ng, B), dtype=np.int32)
    for g in range(n_genes):
        n, nb = int(good[g].sum()), (int(n_valid[g]) - 1 if n_valid is not None else B)
        if nb >= 1:
            rep[g, :n], bcol[g, :n] = cross_draws(seed, int(keys[g]), n, nb, B)
    return rep, bcol


class _Call:
    """One set of inputs on the device, and the three entry points on it."""

    def __init__(self, eng, B, yt, good, gene_ptr, tt, Nc, rep=None, bcol=None, col_map=None, n_valid=None, key=None, seed=SEED):
        opt = lambda a, dt: eng.dev(np.ascontiguousarray(a, dtype=dt)) if a is not None else None
        self.eng, self.B, self.ng, self.ld, self.seed = eng, B, good.shape[1], yt.shape[1], int(seed)
        self.gene_ptr, self.n_valid, self.n_tests, self.n_genes = np.asarray(gene_ptr), n_valid, len(tt), len(good)
        self.yt, self.ptr = eng.dev(yt), eng.dev(np.asarray(gene_ptr, dtype=np.int32))
        self.test_gene = eng.dev(np.repeat(np.arange(self.n_genes, dtype=np.int32), np.diff(gene_ptr)))
        self.mid = [eng.dev(tt), eng.dev(good.astype(np.uint8)), eng.dev(Nc)]
        self.opt = [opt(rep, np.int16), opt(bcol, np.int32), opt(col_map, np.int32), opt(n_valid, np.int32), opt(key, np.int64)]
        self.max_tests = int(np.diff(gene_ptr).max())

    def rows(self):
        """mm_cross_resampled_keyed, one workgroup per test: (rows [n_tests][ld], records [n_tests][8]) on the host."""
        import torch

        e = self.eng
        coef, stats = e.empty((self.n_tests, self.ld), torch.float64), e.empty((self.n_tests, 8), torch.float64)
        e._lib.call("mm_cross_resampled_keyed", e.P(self.yt), self.ld, self.B, self.ng, e.P(self.test_gene), *map(e.P, self.mid),
                    *map(e.P, self.opt), self.seed, self.n_tests, e.P(coef), e.P(stats), e._stream())
        return e.host(coef), e.host(stats)

    def records(self):
        """mm_cross_resampled_block: the records, kept on the device for the family call, and on the host."""
        e = self.eng
        self.stats = e.dev(np.full((self.n_tests, 8), 7.0))
        e._lib.call("mm_cross_resampled_block", e.P(self.yt), self.ld, self.B, self.ng, e.P(self.ptr), self.n_genes, self.max_tests,
                    *map(e.P, self.mid), *map(e.P, self.opt), self.seed, self.n_tests, e.P(self.stats), e._stream())
        return e.host(self.stats)

    def family(self, scale, slab=0):
        """mm_cross_resampled_family on the records of ``records()``: (maxrow [n_genes][ld], adj [n_tests][2], fam [n_genes][2]) on
        the host, every output cell pre-set to 7.0."""
        import torch

        e = self.eng
        maxrow, adj, fam = (e.dev(np.full(s, 7.0)) for s in ((self.n_genes, self.ld), (self.n_tests, 2), (self.n_genes, 2)))
        e._lib.call("mm_cross_resampled_family", e.P(self.yt), self.ld, self.B, self.ng, e.P(self.ptr), self.n_genes, self.max_tests,
                    *map(e.P, self.mid), *map(e.P, self.opt), self.seed, self.n_tests, e.P(self.stats), e.P(e.dev(scale)), int(slab),
                    e.P(maxrow), e.P(adj), e.P(fam), e._stream())
        torch.cuda.synchronize()
        return e.host(maxrow), e.host(adj), e.host(fam)


def _want(call, rows, records, scale):
    """The restatement per gene on the rows of the per-test kernel: (maxrow [n_genes][ld] with 7.0 beyond num_boot, adj, fam)."""
    B = call.B
    maxrow = np.full((call.n_genes, call.ld), 7.0)
    maxrow[:, :B + 1] = np.nan
    adj, fam = np.zeros((call.n_tests, 2)), np.zeros((call.n_genes, 2))
    adj[:, 0] = np.nan
    for g in range(call.n_genes):
        lo, hi = call.gene_ptr[g], call.gene_ptr[g + 1]
        nb = int(call.n_valid[g]) - 1 if call.n_valid is not None else B
        if hi == lo or nb < 1:
            continue
        f = ref.family(rows[lo:hi, :nb], records[lo:hi, 0], scale[lo:hi])
        maxrow[g, :nb] = f["maxrow"]
        adj[lo:hi, 0], adj[lo:hi, 1] = f["t0"], f["n_adj"]
        fam[g] = f["n_valid"], f["n_included"]
    return maxrow, adj, fam


def _check(call, scale_edit=None, slabs=(0,)):
    """Records (block == per-test, bit for bit), then the family outputs against the restatement; -> (rows, records, scale, got)."""
    eng = call.eng
    rows, st_ref = call.rows()
    records = call.records()
    np.testing.assert_array_equal(_bits(records), _bits(st_ref))               # the block kernel's records have not moved
    np.testing.assert_array_equal(_bits(records[:, 0]), _bits(rows[:, 0]))     # coef0 is slot 0 of the row, bit for bit
    scale = eng.family_scale(records)[:, 0]
    if scale_edit is not None:
        scale = scale_edit(scale.copy())
    want = _want(call, rows, records, scale)
    got = None
    for slab in slabs:
        got = call.family(scale, slab)
        for name, g, w in zip(("maxrow", "adj", "fam"), got, want):
            np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{name}, slab {slab}")     # (7.0 left nowhere but beyond num_boot)
    return rows, records, scale, got


@pytest.mark.parametrize("B", [150, 257])
def test_device_draws_with_and_without_a_key(eng, B):
    """All columns, device draws keyed by the slot and by a permuted key.  Gene 2 (one good group: every slot degenerate) and
    gene 4 (no test) give an all-NaN row and (0, 0); member 1 of gene 0 is degenerate at slots where its neighbours are not, so
    the family of gene 0 has fewer valid slots than nb - 1.  Slab widths of 1 workgroup round, 64, 100 and one wider than the
    row give identical bytes."""
    yt, good, gene_ptr, tt, Nc, _, _ = _problem(B)
    call = _Call(eng, B, yt, good, gene_ptr, tt, Nc)
    rows, records, scale, (maxrow, adj, fam) = _check(call, slabs=(0, 64, 100, 7, B + 50))
    assert 0 < fam[0, 0] < B - 1 and fam[0, 1] == COUNTS[0]                    # n_valid_family < nb - 1
    assert records[1, 2] == fam[0, 0]                                          # ... exactly the slots its member 1 has
    assert fam[1].tolist() == [B - 1, COUNTS[1]] and fam[3].tolist() == [B - 1, TT] and fam[5].tolist() == [B - 1, TT - 1]
    assert fam[2].tolist() == [0, 0] and fam[4].tolist() == [0, 0] and np.isnan(maxrow[[2, 4], :B + 1]).all()
    assert np.isnan(adj[gene_ptr[2], 0]) and adj[gene_ptr[2], 1] == 0
    assert np.isnan(maxrow[:, 0]).all() and np.isnan(maxrow[:, B]).all()       # slot 0, and slot nb = B
    assert (adj[:, 1] > 0).sum() > 20 and (adj[:, 1] <= np.repeat(fam[:, 0], COUNTS)).all()
    keys = np.array([4, 0, 3, 5, 1, 2 ** 31 + 9], dtype=np.int64)
    keyed = _Call(eng, B, yt, good, gene_ptr, tt, Nc, key=keys)
    _, _, _, (maxrow_k, adj_k, _) = _check(keyed, slabs=(0, 100))
    np.testing.assert_array_equal(np.isnan(adj_k[:, 0]), np.isnan(adj[:, 0]))  # the same members are included
    assert (maxrow_k[0, 1:B] != maxrow[0, 1:B]).any()                          # other draws under another key


@pytest.mark.parametrize("B", [150, 257])
def test_tables_and_dropped_columns(eng, B):
    """rep / bcol tables (the restated draws: the same bytes as the device draws) and col_map / n_valid with dropped columns:
    gene 3 keeps column 0 alone (n_valid = 1, nb = 0: nothing), gene 0 has nb = B - 37 and its row is NaN from there on."""
    yt, good, gene_ptr, tt, Nc, col_map, n_valid = _problem(B)
    plain = _check(_Call(eng, B, yt, good, gene_ptr, tt, Nc), slabs=(0,))[3]
    rep, bcol = _tables(good, None, B, SEED, np.arange(len(good)))
    by_table = _check(_Call(eng, B, yt, good, gene_ptr, tt, Nc, rep=rep, bcol=bcol, seed=1), slabs=(0, 100))[3]      # (the seed is unused)
    for a, b in zip(by_table, plain):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    dropped = _Call(eng, B, yt, good, gene_ptr, tt, Nc, col_map=col_map, n_valid=n_valid)
    _, _, _, (maxrow, adj, fam) = _check(dropped, slabs=(0, 64))
    nb0 = int(n_valid[0]) - 1
    assert nb0 == B - 37 and np.isfinite(maxrow[0, 1:nb0]).any() and np.isnan(maxrow[0, nb0:B + 1]).all() and 0 < fam[0, 0] < nb0 - 1
    assert fam[3].tolist() == [0, 0] and np.isnan(maxrow[3, :B + 1]).all() and np.isnan(adj[gene_ptr[3]:gene_ptr[4], 0]).all()
    assert fam[5].tolist() == [B - 2, TT - 1]
    rep, bcol = _tables(good, n_valid, B, SEED, np.arange(len(good)))
    both = _check(_Call(eng, B, yt, good, gene_ptr, tt, Nc, rep=rep, bcol=bcol, col_map=col_map, n_valid=n_valid), slabs=(0,))[3]
    for a, b in zip(both, (maxrow, adj, fam)):
        np.testing.assert_array_equal(_bits(a), _bits(b))


def test_members_without_a_scale_inside_a_full_tile(eng):
    """Gene 3 is one full tile: member 2 gets scale 0 and member 5 scale NaN.  They are (NaN, 0), do not enter the maximum, and
    the family counts six; a gene whose every member is excluded has the all-NaN row."""
    B = 150
    yt, good, gene_ptr, tt, Nc, _, _ = _problem(B)
    lo = int(gene_ptr[3])

    def edit(scale):
        scale[lo + 2], scale[lo + 5] = 0.0, np.nan
        scale[gene_ptr[5]:gene_ptr[6]] = 0.0
        scale[gene_ptr[1] + TT:gene_ptr[1] + 2 * TT] = 0.0                     # the whole middle tile of gene 1: skipped
        return scale

    call = _Call(eng, B, yt, good, gene_ptr, tt, Nc)
    _, _, scale, (maxrow, adj, fam) = _check(call, scale_edit=edit, slabs=(0, 64))
    assert fam[3].tolist() == [B - 1, TT - 2] and np.isnan(adj[[lo + 2, lo + 5], 0]).all() and not adj[[lo + 2, lo + 5], 1].any()
    assert fam[5].tolist() == [0, 0] and np.isnan(maxrow[5, :B + 1]).all()
    assert fam[1].tolist() == [B - 1, COUNTS[1] - TT]
    full = call.family(eng.family_scale(eng.host(call.stats))[:, 0])
    assert (full[0][3, 1:B] >= maxrow[3, 1:B]).all() and (full[0][3, 1:B] > maxrow[3, 1:B]).any()      # two members fewer in the maximum


def test_more_groups_than_threads(eng):
    """ng = 300 > the 256 threads of a workgroup (the staging loops stride), B = 70."""
    B = 70
    yt, good, gene_ptr, tt, Nc, col_map, n_valid = _problem(B, ng=300, seed=5)
    _check(_Call(eng, B, yt, good, gene_ptr, tt, Nc, col_map=col_map, n_valid=n_valid), slabs=(0, 33))


def _bootstrap(eng, ym, yv, B, ng):
    """A Bootstrap1D that only holds replicate rows (what the statistics kernels read)."""
    bs = object.__new__(eng.Bootstrap1D)
    bs.ym, bs.yv, bs.ld, bs.B, bs.ng = eng.dev(ym), eng.dev(yv), ym.shape[1], B, ng
    bs.n_tested = bs.n_pairs = ym.shape[0] // ng
    return bs


def test_engine_family_closure(eng):
    """``Bootstrap1D.cross_resampled_family``: the records and rows of ``cross_resampled_block``, and a ``family`` closure whose
    outputs equal the restatement on the closure's own rows for both planes, whichever plane the scratch holds, and do not
    depend on ``slab``; a scale of the wrong shape raises."""
    n_genes, ng, B = 5, 10, 130
    rng = np.random.default_rng(9)
    ym, yv = rng.normal(0, 1, size=(n_genes * ng, B + 1)), rng.normal(0, 1, size=(n_genes * ng, B + 1))
    good = np.ones((n_genes, ng), dtype=bool)
    good[1, 2] = False
    M = np.zeros((2, ng, ng))
    for k, mask in enumerate((good[0], good[1])):                              # the residual maker of an intercept, on the mask
        idx = np.flatnonzero(mask)
        M[k][np.ix_(idx, idx)] = np.eye(len(idx)) - 1.0 / len(idx)
    gene_mask = np.array([0, 1, 0, 0, 0], dtype=np.int32)
    gene_ptr = np.array([0, 11, 14, 14, 22, 23])
    tt = rng.normal(0, 1, size=(23, ng))
    Nc = rng.integers(200, 900, size=ng).astype(np.float64)
    bs = _bootstrap(eng, ym, yv, B, ng)
    keys = np.array([3, 1, 4, 0, 2], dtype=np.int64)
    st_m, st_v, rows, family = bs.cross_resampled_family(gene_ptr, tt, good, gene_mask, M, Nc, seed=11, gene_key=keys)
    st_m0, st_v0, _ = bs.cross_resampled_block(gene_ptr, tt, good, gene_mask, M, Nc, seed=11, gene_key=keys)
    np.testing.assert_array_equal(_bits(st_m), _bits(st_m0))
    np.testing.assert_array_equal(_bits(st_v), _bits(st_v0))
    scale = eng.family_scale(st_m, st_v)
    maxrow, adj, fam = family(scale)
    assert adj.shape == (23, 2, 2) and fam.shape == (n_genes, 2, 2) and len(maxrow) == 2 and maxrow[0].shape == (n_genes, B + 1)
    rows(0, [0])                                                               # the scratch now holds the mean plane
    again = family(scale, slab=50)
    for which, st in ((0, st_m), (1, st_v)):
        got_rows = rows(which, np.arange(23))
        np.testing.assert_array_equal(_bits(eng.host(again[0][which])), _bits(eng.host(maxrow[which])))
        for g in range(n_genes):
            lo, hi = gene_ptr[g], gene_ptr[g + 1]
            f = ref.family(got_rows[lo:hi, :B], st[lo:hi, 0], scale[lo:hi, which])
            np.testing.assert_array_equal(_bits(eng.host(maxrow[which])[g, :B]), _bits(f["maxrow"]))
            assert np.isnan(eng.host(maxrow[which])[g, B])
            np.testing.assert_array_equal(_bits(adj[lo:hi, which, 0]), _bits(f["t0"]))
            np.testing.assert_array_equal(adj[lo:hi, which, 1], f["n_adj"])
            assert fam[g, which].tolist() == [f["n_valid"], f["n_included"]]
    np.testing.assert_array_equal(_bits(again[1]), _bits(adj))
    np.testing.assert_array_equal(_bits(again[2]), _bits(fam))
    assert fam[2].tolist() == [[0, 0], [0, 0]] and fam[0, 0].tolist() == [B - 1, 11]
    for bad in (scale[:, 0], scale[:-1], np.zeros((23, 3))):
        with pytest.raises(ValueError):
            family(bad)
    with pytest.raises(ValueError):
        family(scale, slab=-1)
