"""Kernel-level tests of the count-block ingest (K0: k_sell_split_count, k_sell_layout, k_sell_scatter_tiles and the unpartitioned
k_sell_count / k_sell_scatter) and of the 1D moment sums (K1 + K2: k_moments1d_sell, k_moments1d_reduce).

The layout is compared, whole arrays and bit for bit, with the numpy restatement in tests/_sell_ref.py; the moment sums with
extended-precision sums of the same products, within a bound derived below.  The inputs are STRUCTURED matrices: every builder
names the edge of the kernels it exists for, and tests/test_cpu_sell_ref.py asserts, without a GPU, that its matrix reaches it.
"""

import functools
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

import _sell_ref as ref

pytestmark = pytest.mark.gpu

MAX_COUNT = ref.MAX_COUNT


# ---------------------------------------------------------------------------------------------------------------------
# builders.  A builder describes the entries as (group, row inside the group, gene, count); _assemble scatters the groups'
# cells over the matrix in random positions (their order inside a group is kept: it is the block order), adds cells that
# belong to no group (gid = -1, with entries of their own, which must not arrive anywhere) and draws the size factors.

def _assemble(name, G, sizes, grp, row, gene, val, seed, **edges):
    rng = np.random.default_rng(seed)
    sizes = [int(n) for n in sizes]
    n_out = max(3, sum(sizes) // 9)
    gid = np.repeat(np.r_[np.arange(len(sizes)), -1], sizes + [n_out]).astype(np.int32)
    rng.shuffle(gid)
    cells = np.concatenate([np.flatnonzero(gid == k) for k in range(len(sizes))] + [np.zeros(0, dtype=np.int64)])
    first = np.concatenate([[0], np.cumsum(sizes)])
    grp, row, gene, val = (np.asarray(a, dtype=np.int64) for a in (grp, row, gene, val))
    assert len(grp) == 0 or (row < np.asarray(sizes)[grp]).all()
    r = cells[first[grp] + row] if len(grp) else np.zeros(0, dtype=np.int64)
    out = np.flatnonzero(gid < 0)
    k_out = min(5, G)
    r = np.concatenate([r, np.repeat(out, k_out)])
    gene = np.concatenate([gene, np.concatenate([np.sort(rng.choice(G, k_out, replace=False)) for _ in out])])
    val = np.concatenate([val, rng.integers(1, 4, size=len(out) * k_out)])
    assert len(np.unique(r * G + gene)) == len(r), "a builder must not store one (cell, gene) twice"
    X = sp.csr_matrix((val.astype(np.float32), (r, gene)), shape=(len(gid), G))
    X.sort_indices()
    assert X.has_canonical_format and X.nnz == len(r)
    sf = rng.lognormal(0.0, 0.4, size=len(gid))           # per cell: a wrong cell_local shows in the sums
    return SimpleNamespace(name=name, X=X, gid=gid, ng=len(sizes), sf=sf, G=G, sizes=sizes, **edges)


def _cat(parts):
    """[(group, rows, genes, counts), ...] with broadcastable members -> four flat arrays."""
    cols = [[], [], [], []]
    for p in parts:
        p = np.broadcast_arrays(*[np.asarray(a, dtype=np.int64) for a in p])
        for c, a in zip(cols, p):
            c.append(a.ravel())
    return [np.concatenate(c) if c else np.zeros(0, dtype=np.int64) for c in cols]


def _sprinkle(rng, group, n_rows, genes, density, hi=4):
    """Bernoulli(density) entries with counts 1..hi-1 on rows 0..n_rows-1 x ``genes`` of one group."""
    genes = np.asarray(genes)
    r, c = np.nonzero(rng.random((n_rows, len(genes)), dtype=np.float32) < density)
    return (group, r, genes[c], rng.integers(1, hi, size=len(r)))


ROW_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 512, 1024)


def case_rowlens():
    """k_sell_split_count reads 64 x 4 column indices per step with position e as the sentinel: rows whose total length is 0, 1, 63,
    64, 65, 255, 256, 257, 512 and 1,024, in one block of G = 2,049 genes (three ranges, the last one gene wide); rows that lie only
    in the first range, only in the last, in ranges 0 and 2 with range 1 empty (one lane owns several boundaries), and across a
    whole range (1,024 consecutive genes)."""
    rng = np.random.default_rng(11)
    G = 2049
    rows = [np.sort(rng.choice(G, L, replace=False)) for L in ROW_LENGTHS]
    rows += [np.sort(rng.choice(1024, L, replace=False)) for L in (1, 64, 257)]                               # first range only
    rows += [np.array([2048])]                                                                                 # last range only
    rows += [np.r_[np.sort(rng.choice(1024, L, replace=False)), 2048] for L in (1, 63, 300)]                   # ranges 0 and 2
    rows += [np.arange(1024, 2048), np.arange(1024), np.r_[np.arange(1024), 2048], np.arange(1024, 2049)]      # a whole range
    rows += [np.arange(s, s + L) for s, L in ((1000, 65), (960, 256), (1023, 2), (2047, 2), (700, 1024))]      # runs over a border
    rows = [np.zeros(0, dtype=np.int64)] + rows + [rows[i] for i in rng.permutation(len(rows))] * 2 + [np.zeros(0, dtype=np.int64)]
    parts = [(0, i, g, 1 + (g + i) % 5) for i, g in enumerate(rows)]
    return _assemble("rowlens", G, [len(rows)], *_cat(parts), seed=12)


BLOCKMAP_SIZES = (1, 127, 128, 129, 130, 131, 130, 129, 133, 130, 132)


def case_blockmap():
    """Block -> workgroup map of k_sell_scatter_tiles, b = (t / n_ranges) * 8 + x with the b >= n_blocks exit: 11 groups of ~130
    cells = 11 blocks (more than 8, no multiple of 8) x 3 ranges.  G = 2,049 is odd, so every second block's 16-bit counters start
    on an odd half-word of blk_cnt (the merge of k_sell_split_count).  Blocks of 1, 127, 128 and 129 cells; the 129-cell blocks end
    in a tile of one row."""
    rng = np.random.default_rng(21)
    G = 2049
    parts = [_sprinkle(rng, k, n, np.arange(G), 0.02) for k, n in enumerate(BLOCKMAP_SIZES)]
    return _assemble("blockmap", G, BLOCKMAP_SIZES, *_cat(parts), seed=22)


# the tiles the (block 0, range 0) workgroup of case_tiles must take, in order
TILES_WANT = [(128, 4096), (4, 4096), (4, 4000), (4, 4096), (64, 4096), (65, 4096), (128, 4096), (128, 0), (128, 0), (128, 3456),
              (23, 3712), (4, 4096), (1, 5)]


def case_tiles():
    """Tile extents of k_sell_scatter_tiles (<= 128 rows, <= 4,096 entries of the range).  Range 0 of one block, in this order:
    128 rows of 32 (T = 128, E = 4,096 exactly); 4 rows of 1,024 (T = 4, E = 4,096); 4 rows of 1,000 cut by the next row (E = 4,000);
    64 rows of 64 (T = 64: E comes from the first half's scan); 64 rows of 63 and one of 64 (T = 65: E from lane 0 of the second
    half); 4 rows of 1,024 and 400 rows with entries in range 1 only (a full tile that takes 124 empty rows along, then whole tiles
    with E = 0 between tiles that have entries); a last tile of one row."""
    G = 2048
    full = np.arange(1024)
    seg = [np.sort((i * 37 + np.arange(32) * 32) % 1024) for i in range(128)]
    seg += [full] * 4
    seg += [np.delete(full, i + np.arange(24) * 42) for i in range(4)]
    seg += [full] * 4
    seg += [np.sort((i * 5 + np.arange(64) * 16) % 1024) for i in range(64)]
    seg += [np.sort((i * 7 + np.arange(64) * 16) % 1024)[:63] for i in range(64)] + [np.sort((3 + np.arange(64) * 16) % 1024)]
    seg += [full] * 4
    seg += [full[:0]] * 400
    seg += [np.sort((i * 11 + np.arange(32) * 32) % 1024) for i in range(128)]
    seg += [full] * 7
    seg += [np.array([0, 1, 500, 1000, 1023])]
    parts = []
    for i, g in enumerate(seg):
        parts.append((0, i, g, 1 + (g + i) % 5))
        k = 5 if len(g) == 0 else i % 4                     # range 1: the rows that are empty in range 0 all have entries here
        g1 = 1024 + np.sort((i * 13 + np.arange(k) * 101) % 1024)
        parts.append((0, i, g1, 1 + (g1 + i) % 3))
    return _assemble("tiles", G, [len(seg)], *_cat(parts), seed=32)


# case_carry: gene -> the rows (of the one block) that hold it.  Tiles are 128 rows there, so rows 300 apart are >= 2 tiles apart.
CARRY_SPACED = {g: 40 + 300 * np.arange(k) for g, k in enumerate((1, 2, 3, 4, 5, 7))}       # genes 0..5: 1, 2, 3, 4, 5, 7 entries
CARRY_SPLIT = {6: [3, 700, 701, 702],                  # 1 entry waits in the carry; 3 complete the group two tiles later
               7: [3, 4, 700, 701],                    # 2 + 2
               8: [3, 4, 5, 700],                      # 3 + 1
               9: [3, 4, 5, 700, 701, 702, 703, 704, 705],       # 3 + 6: one group from the carry, one from the tile, 1 left over
               10: list(range(130, 138)),              # 8 in one tile: two groups without the carry
               11: list(range(130, 136)),              # 6 in one tile: one group, 2 left over
               12: [2399],                             # the last row of the block
               13: [0, 127, 128, 2399]}                # first and last row of a tile, last row of the block


def case_carry():
    """The 4-slot carry of k_sell_scatter_tiles: genes with 1, 2, 3, 4, 5 and 7 entries in a block whose consecutive entries are
    >= 2 tiles apart, so every group is completed from the carry (the e0 + i < c reads of P4) and counts = 0, 1, 2, 3 mod 4 leave
    every size of leftover; groups split 1 + 3, 2 + 2, 3 + 1 between the carry and a later tile.  The block has 2,400 cells: three
    row chunks of k_sell_split_count merge into one blk_cnt row.  G = 1,100: a 76-gene last range, 18 slices with 12 genes in the last."""
    rng = np.random.default_rng(41)
    G, n = 1100, 2400
    parts = [_sprinkle(rng, 0, n, np.arange(64, G), 0.01)]
    for g, rows in {**CARRY_SPACED, **CARRY_SPLIT}.items():
        rows = np.asarray(rows)
        parts.append((0, rows, g, 1 + (rows + g) % 7))
    return _assemble("carry", G, [n], *_cat(parts), seed=42)


# case_widths, block 0: count of the first slot of every slice -> slice widths 129, 65, 65, 64, 63, 9, 8, 7, 1, 1, 1, 0 ... rows
WIDTHS_FIRST = (516, 260, 257, 256, 252, 36, 32, 28, 4, 1, 1, 0, 0, 0, 0, 0, 0)


def case_widths():
    """k_sell_layout and the row batches of K1 (K1_UNROLL = 8 rows in flight, items of 64 rows).  Block 0 (520 cells, G = 1,025):
    first-slot counts 516, 260, 257, 256, 252, 36, 32, 28, 4, 1 -> slices of 129, 65, 65, 64, 63, 9, 8, 7, 1 and 1 rows, i.e. 3, 2,
    2, 1, ... items, then whole slices of zero-count genes (width 0, no item, equal item_ptr); long runs of equal counts whose slots
    go by gene id; one count of 524,287 among the small ones.  Block 1 (300 cells): every gene has the same count, so the slots are
    the gene ids.  Block 2 (40 cells): no entry at all."""
    rng = np.random.default_rng(51)
    G, n0, n1 = 1025, 520, 300
    W = WIDTHS_FIRST + (0,)
    slot = np.arange(G)
    cnt_by_slot = np.where(slot % 64 < 40, np.take(W, slot // 64), np.maximum(np.take(W, slot // 64 + 1), np.take(W, slot // 64) - 1))
    cnt = np.empty(G, dtype=np.int64)
    cnt[rng.permutation(G)] = cnt_by_slot                 # which gene gets which count: the slots are not the gene ids
    parts = []
    for g in np.flatnonzero(cnt):
        rows = (g * 7 + np.arange(cnt[g])) % n0
        parts.append((0, rows, g, 1 + (rows + g) % 4))
    parts.append((1, (slot[:, None] * 7 + np.arange(5)[None, :]) % n1, slot[:, None], 2))
    grp, row, gene, val = _cat(parts)
    val[np.flatnonzero((grp == 0) & (cnt[gene] == 252))[17]] = MAX_COUNT
    return _assemble("widths", G, [n0, n1, 40], grp, row, gene, val, seed=52, cnt0=cnt)


GENE_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025)


def case_genes(G):
    """k_sell_layout at G = 1, 63, 64, 65, 1,023, 1,024 and 1,025: the last slice full, one gene short, one gene over; one range
    and a second range of one gene.  Two blocks of 150 and 37 cells, few distinct counts (many ties)."""
    rng = np.random.default_rng(60 + G)
    dens = min(0.5, max(0.04, 6.0 / G))
    parts = [_sprinkle(rng, k, n, np.arange(G), dens) for k, n in enumerate((150, 37))]
    return _assemble(f"genes{G}", G, [150, 37], *_cat(parts), seed=61 + G)


BIG_SIZES = (16385, 8193, 0, 8192)


def case_big():
    """Groups of 16,385 cells (three blocks, reduced in block order), 8,193 (two blocks), none (its outputs are 0) and 8,192 (one
    FULL block: K1's 1/sf staging has no zero fill) x 1,025 genes with 2 % of entries.  Gene 0 is present in every cell: in the
    full block its count, the layout's histogram index and the scatter's 16-bit cursor take their largest value, 8,192, and every
    tile of that block has n = 128 for it with every mask bit set.  Gene 7 is present nowhere."""
    rng = np.random.default_rng(71)
    G = 1025
    genes = np.setdiff1d(np.arange(1, G), [7])
    parts = []
    for k, n in enumerate(BIG_SIZES):
        if n:
            parts.append(_sprinkle(rng, k, n, genes, 0.02))
            parts.append((k, np.arange(n), 0, 1 + np.arange(n) % 3))
    return _assemble("big", G, BIG_SIZES, *_cat(parts), seed=72)


BUILDERS = {"rowlens": case_rowlens, "blockmap": case_blockmap, "tiles": case_tiles, "carry": case_carry, "widths": case_widths,
            **{f"genes{G}": functools.partial(case_genes, G) for G in GENE_COUNTS}, "big": case_big}
CASES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, layout) of a structured matrix: built once per process and left unchanged."""
    c = BUILDERS[name]()
    lay = ref.sell_layout(c.X, c.gid, c.ng)
    for a in lay.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c, lay


@functools.lru_cache(maxsize=None)
def reference_moments(name):
    c, lay = reference(name)
    return ref.moment_sums(c.X, c.gid, c.ng, 1.0 / c.sf, layout=lay)


def shuffled_rows(X, seed):
    """The CSR arrays of X with the entries of every row in random order (what takes the unpartitioned ingest)."""
    rng = np.random.default_rng(seed)
    row = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    o = np.lexsort((rng.random(X.nnz), row))
    r = int(np.argmax(np.diff(X.indptr)))                  # the longest row backwards: out of order whatever was drawn
    o[X.indptr[r]:X.indptr[r + 1]] = np.arange(X.indptr[r], X.indptr[r + 1])[::-1]
    return X.indptr.astype(np.int64), X.indices[o].astype(np.int32), X.data[o].astype(np.float32)


def can_be_unsorted(X):
    """A row needs two entries to be out of order."""
    return int(np.diff(X.indptr).max(initial=0)) >= 2


UNSORTABLE = tuple(n for n in CASES if n != "genes1")      # with G = 1 there is no unpartitioned ingest to reach


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


def _from_arrays(eng, ptr, idx, dat, shape):
    import torch

    return eng.DeviceCSR.from_device(torch.from_numpy(np.ascontiguousarray(ptr, dtype=np.int64)).cuda(),
                                     torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).cuda(),
                                     torch.from_numpy(np.ascontiguousarray(dat, dtype=np.float32)).cuda(), shape)


@pytest.fixture(scope="module", params=CASES)
def prob(request, eng):
    """One structured matrix, its reference layout and ONE range-partitioned ingest, shared by the assertions on it."""
    c, lay = reference(request.param)
    return SimpleNamespace(case=c, lay=lay, name=request.param, blocks=eng.CountBlocks(eng.DeviceCSR(c.X), c.gid, c.ng), moments=[])


@pytest.fixture(scope="module", params=UNSORTABLE)
def uprob(request, eng):
    """The same matrices with the entries of every row permuted, handed in through DeviceCSR.from_device: ONE unpartitioned ingest."""
    c, lay = reference(request.param)
    blocks = eng.CountBlocks(_from_arrays(eng, *shuffled_rows(c.X, 5), c.X.shape), c.gid, c.ng)
    return SimpleNamespace(case=c, lay=lay, name=request.param, blocks=blocks, moments=[])


def _moments(prob):
    if not prob.moments:
        prob.moments.append(prob.blocks.moments(1.0 / prob.case.sf))
    return prob.moments[0]


TABLES = ("rank", "perm", "slice_w", "slice_ptr", "item_ptr", "blk_base", "blk_item_base")


def _assert_tables(eng, blocks, lay):
    np.testing.assert_array_equal(blocks.blk_cnt, lay["blk_cnt"], err_msg="blk_cnt")
    assert blocks.blk_cnt.dtype == np.uint16
    for name in TABLES:
        got = eng.host(getattr(blocks, name))
        assert got.shape == lay[name].shape, name
        np.testing.assert_array_equal(got, lay[name], err_msg=name)
    assert blocks.total_rows == lay["total_rows"] and blocks.total_items == lay["total_items"]
    assert blocks.nnz_sel == lay["nnz_sel"]
    for name in ("cell_order", "blk_cell0", "blk_group", "grp_blk0"):
        np.testing.assert_array_equal(getattr(blocks, name), lay["plan"][name])


def test_ranged_ingest_equals_the_reference_layout(eng, prob):
    """blocks.ranged: blk_cnt (k_sell_split_count), the layout tables (k_sell_layout) and the ENTIRE entry array
    (k_sell_scatter_tiles) are the reference's, bit for bit -- the layout is a pure function of the counts, ties go by gene id,
    a gene's entries ascend in the cell index and every other word is zero."""
    b = prob.blocks
    assert b.ranged
    _assert_tables(eng, b, prob.lay)
    ent = eng.host(b.ent, np.uint32)
    assert ent.shape == prob.lay["ent"].shape
    np.testing.assert_array_equal(ent, prob.lay["ent"])


def test_unpartitioned_ingest_equals_the_reference_layout(eng, uprob):
    """Rows with permuted entries take k_sell_count / k_sell_scatter: the same tables; the entries of a (block, gene) are placed in
    their order of arrival, so its first ``count`` words are the reference's words as a sorted set; every other word is zero."""
    b, lay = uprob.blocks, uprob.lay
    assert not b.ranged
    _assert_tables(eng, b, lay)
    ent = eng.host(b.ent, np.uint32)
    assert ent.shape == lay["ent"].shape
    key, word = lay["ent_key"], lay["ent_word"]            # the words of the first ``count`` entries of every (block, gene)
    got, want = ent[word].astype(np.int64), lay["ent"][word].astype(np.int64)
    np.testing.assert_array_equal(got[np.lexsort((got, key))], want[np.lexsort((want, key))])
    rest = ent.copy()
    rest[word] = 0
    assert not rest.any()


def _assert_moment_integers(prob):
    S, sumx, maxx = _moments(prob)
    _, sumx_ref, maxx_ref, _ = reference_moments(prob.name)
    np.testing.assert_array_equal(sumx, sumx_ref)
    np.testing.assert_array_equal(maxx, maxx_ref)
    assert sumx.dtype == np.uint64 and maxx.dtype == np.uint32
    # a (group, gene) without an entry: exact +0.0, no signed or denormal residue
    empty = sumx_ref == 0
    assert (S[:, empty].view(np.uint64) == 0).all()


def test_moment_integers_are_exact(prob):
    _assert_moment_integers(prob)


def test_moment_integers_are_exact_unpartitioned(uprob):
    _assert_moment_integers(uprob)


def _assert_moment_sums(prob):
    """S1 = sum x w, S2 = sum x^2 w^2, S3 = sum x w^2 (w = 1 / size factor) against extended-precision pairwise sums.

    The bound.  All terms are non-negative, so the relative error of a sum is at most the sum of the relative errors along the
    longest chain of roundings that leads to it, each <= u = 2^-53: a term carries at most 3 (x w, (x w) w, x ((x w) w); a fused
    multiply-add only removes one); a K1 work item holds at most 64 rows x 4 = 256 entries of a gene, hence at most 255 additions;
    K2 then makes one addition per work item of the gene's slice over the blocks of the group.  (3 + 255 + n_items) u to first
    order; 260 + n_items leaves the second-order terms (< n^2 u^2) and the reference's own error (~ log2(n) 2^-64) inside it.
    For a gene in every cell of three blocks of ~5,460 cells (22 items each) that is 3.6e-14."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("np.longdouble has no 64-bit mantissa on this platform: no reference precise enough for the bound")
    S = _moments(prob)[0]
    S_ref, _, _, n_items = reference_moments(prob.name)
    bound = ((260 + n_items) * np.longdouble(2.0) ** -53)[None] * S_ref
    err = np.abs(S.astype(np.longdouble) - S_ref)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), (worst, float(err[worst]), float(bound[worst]))


def test_moment_sums_within_the_derived_bound(prob):
    _assert_moment_sums(prob)


def test_moment_sums_within_the_derived_bound_unpartitioned(uprob):
    _assert_moment_sums(uprob)


def test_moments_are_bit_identical_across_calls_and_ingests(eng, prob):
    """Two moments() calls on one CountBlocks, and on two ingests of one CSR, give the same bits."""
    c = prob.case
    first = _moments(prob)
    again = prob.blocks.moments(1.0 / c.sf)
    other = eng.CountBlocks(eng.DeviceCSR(c.X), c.gid, c.ng)
    import torch

    assert torch.equal(other.ent, prob.blocks.ent)
    for u, v, w in zip(first, again, other.moments(1.0 / c.sf)):
        assert u.tobytes() == v.tobytes() == w.tobytes()


def test_moments_are_bit_identical_across_calls_unpartitioned(uprob):
    for u, v in zip(_moments(uprob), uprob.blocks.moments(1.0 / uprob.case.sf)):
        assert u.tobytes() == v.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# behaviour that is decided here and pinned

def _assert_empty_blocks(blocks, gid, ng, G):
    assert blocks.nnz_sel == 0
    assert blocks.blk_cnt.shape == (blocks.n_blocks, G) and not blocks.blk_cnt.any()
    S, sumx, maxx = blocks.moments(np.ones(len(gid)))
    assert S.shape == (3, ng, G) and (S.view(np.uint64) == 0).all() and not sumx.any() and not maxx.any()


def _small(seed, n, G, density):
    rng = np.random.default_rng(seed)
    X = sp.csr_matrix((rng.random((n, G)) < density).astype(np.float32) * rng.integers(1, 5, size=(n, G)).astype(np.float32))
    gid = rng.integers(-1, 3, size=n).astype(np.int32)
    return X, gid, 3


def test_no_stored_entry_among_the_selected_cells(eng):
    """Case 1: the cells of the groups are empty, other cells are not.  All-zero blk_cnt, zero moments, nnz_sel == 0, no error."""
    X, gid, ng = _small(1, 300, 1500, 0.05)
    X = sp.diags((gid < 0).astype(np.float32)).dot(X).tocsr()
    X.eliminate_zeros()
    assert X.nnz > 0 and X[gid >= 0].nnz == 0
    blocks = eng.CountBlocks(eng.DeviceCSR(X), gid, ng)
    assert blocks.ranged and blocks.total_rows == 0 and blocks.total_items == 0
    _assert_empty_blocks(blocks, gid, ng, 1500)
    assert not eng.host(blocks.ent).any()


@pytest.mark.parametrize("how", ["scipy", "from_device"])
def test_csr_without_any_stored_entry(eng, how):
    """Case 2: nnz == 0.  A tensor without elements has a null device pointer, which the C-ABI refuses, and the tile scatter reads
    element 0 of indices / data on behalf of an empty tile: the DeviceCSR lends one-element buffers (engine.DeviceCSR.entry_ptrs)."""
    _, gid, ng = _small(2, 300, 1500, 0.05)
    if how == "scipy":
        csr = eng.DeviceCSR(sp.csr_matrix((300, 1500), dtype=np.float32))
    else:
        csr = _from_arrays(eng, np.zeros(301), np.zeros(0), np.zeros(0), (300, 1500))
    assert csr.nnz == 0 and csr.indices.numel() == 0
    blocks = eng.CountBlocks(csr, gid, ng)
    assert blocks.ranged and blocks.total_rows == 0
    _assert_empty_blocks(blocks, gid, ng, 1500)
    np.testing.assert_array_equal(csr.rowsum(), np.zeros(300))
    np.testing.assert_array_equal(csr.colsum(), np.zeros(1500))
    assert csr.colsplit(100, 200).nnz == 0 and csr.colselect([3, 700, 1499]).nnz == 0


def test_gene_part_that_receives_no_entry(eng):
    """Case 3: engine.count_blocks(..., part_genes=64) on 130 genes with entries in genes 0..63 and 128..129 only: the middle part is a
    CSR without a stored entry (colsplit hands out empty slices)."""
    X, gid, ng = _small(3, 400, 130, 0.2)
    X = X.tolil()
    X[:, 64:128] = 0
    X = X.tocsr()
    X.eliminate_zeros()
    wide = eng.count_blocks(eng.DeviceCSR(X), gid, ng, part_genes=64)
    assert len(wide.parts) == 3 and wide.parts[1].nnz_sel == 0 and wide.parts[0].nnz_sel > 0 and wide.parts[2].nnz_sel > 0
    lay = ref.sell_layout(X, gid, ng)
    np.testing.assert_array_equal(wide.blk_cnt, lay["blk_cnt"])
    assert not wide.blk_cnt[:, 64:128].any() and wide.nnz_sel == lay["nnz_sel"]
    sf = np.random.default_rng(4).lognormal(0, 0.4, size=400)
    S, sumx, maxx = wide.moments(1.0 / sf)
    _, sumx_ref, maxx_ref, _ = ref.moment_sums(X, gid, ng, 1.0 / sf, layout=lay)
    np.testing.assert_array_equal(sumx, sumx_ref)
    np.testing.assert_array_equal(maxx, maxx_ref)
    assert (S[:, :, 64:128].view(np.uint64) == 0).all()


def _limit_problem(top):
    X, gid, ng = _small(5, 200, 70, 0.2)
    X = X.tolil()
    cell = int(np.flatnonzero(gid >= 0)[11])
    X[cell, 33] = top
    return X.tocsr(), gid, ng, cell


@pytest.mark.parametrize("path", ["ranged", "unpartitioned"])
def test_count_limit(eng, path):
    """524,287 (19 bits) is accepted and comes back from the entry array and from max x; 524,288 raises the documented error."""
    def ingest(X, gid, ng):
        csr = eng.DeviceCSR(X) if path == "ranged" else _from_arrays(eng, *shuffled_rows(X, 6), X.shape)
        blocks = eng.CountBlocks(csr, gid, ng)
        assert blocks.ranged == (path == "ranged") and can_be_unsorted(X)
        return blocks

    X, gid, ng, cell = _limit_problem(MAX_COUNT)
    blocks = ingest(X, gid, ng)
    lay = ref.sell_layout(X, gid, ng)
    ent = eng.host(blocks.ent, np.uint32)
    np.testing.assert_array_equal(np.sort(ent), np.sort(lay["ent"]))
    assert (ent >> 13).max() == MAX_COUNT and ((lay["ent"] >> 13) == MAX_COUNT).sum() == 1
    S, sumx, maxx = blocks.moments(np.ones(200))
    assert maxx[gid[cell], 33] == MAX_COUNT and maxx.max() == MAX_COUNT
    np.testing.assert_array_equal(sumx, ref.moment_sums(X, gid, ng, np.ones(200), layout=lay)[1])
    X, gid, ng, _ = _limit_problem(MAX_COUNT + 1)
    with pytest.raises(ValueError, match=f"positive integer counts <= {MAX_COUNT}"):
        ingest(X, gid, ng)
