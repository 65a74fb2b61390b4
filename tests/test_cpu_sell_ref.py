"""The numpy restatement of the count-block layout (tests/_sell_ref.py) and the structured matrices of
tests/test_gpu_ingest_moments.py, checked without a GPU: the reference entry array decodes back into the triples of the matrix,
the layout invariants of DESIGN.md section 2 hold, and every structured matrix REACHES the edge of the kernels it is named for --
a condition, not a measurement: a matrix that no longer hits its edge fails here."""

import numpy as np
import pytest

import _sell_ref as ref
import test_gpu_ingest_moments as gm
from test_gpu_ingest_moments import CASES, reference


def _triples(X, gid):
    sel = np.flatnonzero(np.asarray(gid) >= 0)
    C = X[sel].tocoo()
    a = np.stack([sel[C.row], C.col, C.data.astype(np.int64)], axis=1).astype(np.int64)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def _check_layout(X, gid, lay):
    G = X.shape[1]
    np.testing.assert_array_equal(ref.decode(lay), _triples(X, gid))
    assert lay["nnz_sel"] == X[np.asarray(gid) >= 0].nnz == int(lay["blk_cnt"].astype(np.int64).sum())
    nb, ns = lay["slice_w"].shape
    ent = lay["ent"]
    assert int(np.count_nonzero(ent)) == lay["nnz_sel"]                     # only zero padding
    for b in range(nb):
        perm, rank, cnt = lay["perm"][b], lay["rank"][b], lay["blk_cnt"][b].astype(np.int64)
        assert (perm[G:] == -1).all() and sorted(perm[:G]) == list(range(G))
        np.testing.assert_array_equal(rank[perm[:G]], np.arange(G))
        c = cnt[perm[:G]]
        assert (np.diff(c) <= 0).all()                                      # slots in descending count order
        assert (np.diff(perm[:G])[np.diff(c) == 0] > 0).all()               # ties ascend by gene id
        np.testing.assert_array_equal(lay["slice_w"][b], -(-c[::64] // 4))
        # every gene: ``count`` non-zero words at the head of its lane of the slice, cell_local strictly ascending, zeros behind
        rows = ent[int(lay["blk_base"][b]) * 256:(int(lay["blk_base"][b]) + int(lay["slice_ptr"][b, -1])) * 256].reshape(-1, 64, 4)
        for t in range(ns):
            e = rows[lay["slice_ptr"][b, t]:lay["slice_ptr"][b, t + 1]].transpose(1, 0, 2).reshape(64, -1)      # [lane][j]
            n = np.zeros(64, dtype=np.int64)
            n[:len(c[t * 64:t * 64 + 64])] = c[t * 64:t * 64 + 64]
            head = np.arange(e.shape[1])[None, :] < n[:, None]
            assert ((e != 0) == head).all()
            cl = (e & 8191).astype(np.int64)
            asc = np.diff(cl, axis=1) > 0
            assert (asc | ~head[:, 1:]).all()
    assert lay["blk_base"][0] == 0 and len(ent) == max(1, lay["total_rows"]) * 256


def test_reference_on_a_random_matrix():
    from scrna_parameter_estimation_amd.synth import synth_counts

    X = synth_counts(2500, 1100, 0.06, 3, dtype=np.float32)
    gid = np.random.default_rng(3).integers(-1, 4, size=2500).astype(np.int32)
    lay = ref.sell_layout(X, gid, 4)
    _check_layout(X, gid, lay)
    # the moment sums against scipy's fp64 products
    sf = np.random.default_rng(4).lognormal(0, 0.4, size=2500)
    S, sumx, maxx, n_items = ref.moment_sums(X, gid, 4, 1.0 / sf, layout=lay)
    for k in range(4):
        Xg = X[gid == k].astype(np.float64).tocsc()
        w = 1.0 / sf[gid == k]
        np.testing.assert_allclose(S[0, k].astype(np.float64), Xg.T.dot(w), rtol=1e-13)
        np.testing.assert_allclose(S[1, k].astype(np.float64), Xg.power(2).T.dot(w ** 2), rtol=1e-13)
        np.testing.assert_allclose(S[2, k].astype(np.float64), Xg.T.dot(w ** 2), rtol=1e-13)
        np.testing.assert_array_equal(sumx[k], np.asarray(Xg.sum(axis=0)).ravel().astype(np.uint64))
        np.testing.assert_array_equal(maxx[k], np.asarray(Xg.max(axis=0).todense()).ravel().astype(np.uint32))
    assert (n_items[sumx > 0] > 0).all()              # (a gene without entries shares the items of its slice)


@pytest.mark.parametrize("name", CASES)
def test_reference_on_the_structured_matrices(name):
    c, lay = reference(name)
    assert (c.gid < 0).any() and c.X[c.gid < 0].nnz > 0          # cells of no group, with entries that must not arrive
    assert c.X.has_canonical_format and c.X.dtype == np.float32
    _check_layout(c.X, c.gid, lay)


def test_tile_plan_rule():
    assert ref.tile_plan([]) == []
    assert ref.tile_plan([0] * 129) == [(128, 0), (1, 0)]
    assert ref.tile_plan([1024] * 5) == [(4, 4096), (1, 1024)]
    assert ref.tile_plan([1024, 1024, 1024, 1023, 2]) == [(4, 4095), (1, 2)]
    assert ref.tile_plan([32] * 128 + [1]) == [(128, 4096), (1, 1)]
    assert ref.tile_plan([33] * 128) == [(124, 4092), (4, 132)]


# ---------------------------------------------------------------------------------------------------------------------
# every structured matrix reaches the edge it is named for

def _tiles(c):
    """[block][range] -> tile list, and the segment lengths."""
    seg = ref.segment_lengths(c.X, reference(c.name)[1]["plan"])
    return [[ref.tile_plan(s) for s in blk] for blk in seg], seg


def test_rowlens_reaches_its_edges():
    c, lay = reference("rowlens")
    assert c.G == 2049 and lay["blk_cnt"].shape == (1, 2049)                 # one block, three ranges, the last one gene wide
    (seg,) = ref.segment_lengths(c.X, lay["plan"])
    seg = np.stack(seg, axis=1)                                              # [row][range]
    assert seg.shape[1] == 3 and seg.shape[0] > 64                           # more than one batch of 64 rows
    total = seg.sum(axis=1)
    assert set(gm.ROW_LENGTHS) <= set(total.tolist())
    assert total[0] == 0 and total[-1] == 0
    has = seg > 0
    assert (has == [True, False, False]).all(axis=1).any()                   # first range only
    assert ((has == [False, False, True]).all(axis=1) & (total == 1)).any()  # last range only
    assert (has == [True, False, True]).all(axis=1).any()                    # ranges 0 and 2, range 1 empty
    assert (seg[:, 1] == 1024).any() and (seg[:, 0] == 1024).any()           # a whole range
    assert ((seg[:, 1] == 1024) & (total == 1024)).any() and ((seg[:, 1] == 1024) & (seg[:, 2] == 1)).any()


def test_blockmap_reaches_its_edges():
    c, lay = reference("blockmap")
    nb = len(lay["plan"]["blk_group"])
    assert nb == 11 and nb > 8 and nb % 8 != 0 and -(-c.G // ref.RANGE_GENES) == 3
    assert c.G % 2 == 1 and nb >= 2                                          # counters of block 1 start on an odd half-word
    cells = np.diff(lay["plan"]["blk_cell0"])
    assert {1, 127, 128, 129} <= set(cells.tolist())
    tiles, _ = _tiles(c)
    for b in np.flatnonzero(cells == 129):
        for rg in range(3):
            assert [T for T, _ in tiles[b][rg]] == [128, 1]                  # a block whose last tile is one row
    assert all(E > 0 for blk in tiles for t in blk[:2] for _, E in t[:1])


def test_tiles_reaches_its_edges():
    c, lay = reference("tiles")
    tiles, seg = _tiles(c)
    assert len(tiles) == 1 and len(tiles[0]) == 2
    assert tiles[0][0] == gm.TILES_WANT
    want = gm.TILES_WANT
    assert (128, 4096) in want and (4, 4096) in want and (4, 4000) in want and (64, 4096) in want and (65, 4096) in want
    i = want.index((4, 4000))
    assert seg[0][0][sum(T for T, _ in want[:i]) + 4] + 4000 > 4096           # E = 4,000: cut by the next row
    i = want.index((65, 4096))
    r = sum(T for T, _ in want[:i])
    assert (seg[0][0][r:r + 64] == 63).all() and seg[0][0][r + 64] == 64
    i = want.index((128, 0))
    assert want[i + 1] == (128, 0) and want[i - 1][1] > 0 and want[i + 2][1] > 0    # whole empty tiles between tiles with entries
    r = sum(T for T, _ in want[:i])
    assert (seg[0][1][r:r + 256] > 0).all() and (seg[0][0][r:r + 256] == 0).all()   # ... whose rows have entries in the other range
    assert want[i - 1] == (128, 4096) and (seg[0][0][r - 124:r] == 0).all()          # (the full tile before took 124 empty rows along:
    assert (seg[0][0][r - 128:r - 124] == 1024).all()                               #  >= 300 consecutive rows without an entry here)
    assert want[-1][0] == 1 and want[-2][1] == 4096


def test_carry_reaches_its_edges():
    c, lay = reference("carry")
    tiles, seg = _tiles(c)
    n = len(seg[0][0])
    assert n == 2400 > 2 * ref.SC_ROWS                                       # three row chunks merge into one blk_cnt row
    assert [T for T, _ in tiles[0][0]] == [128] * (n // 128) + [n % 128]     # range 0: tile k = rows 128 k ...
    tile_of = lambda rows: np.asarray(rows) // 128
    cnt = lay["blk_cnt"][0]
    assert [int(cnt[g]) for g in range(6)] == [1, 2, 3, 4, 5, 7]
    for g, rows in gm.CARRY_SPACED.items():
        assert (np.diff(tile_of(rows)) >= 2).all()                          # consecutive entries >= 2 tiles apart
    assert {int(cnt[g]) % 4 for g in gm.CARRY_SPACED} == {0, 1, 2, 3}
    for g, split in ((6, (1, 3)), (7, (2, 2)), (8, (3, 1)), (9, (3, 6))):
        t = tile_of(gm.CARRY_SPLIT[g])
        assert tuple(np.bincount(t)[np.unique(t)]) == split and np.diff(np.unique(t))[0] >= 2
    assert c.G % 64 != 0 and c.G % 1024 == 76


def test_widths_reaches_its_edges():
    c, lay = reference("widths")
    first = lay["blk_cnt"][0][lay["perm"][0, ::64]]
    assert tuple(first) == gm.WIDTHS_FIRST
    sw = lay["slice_w"][0]
    assert {1, 7, 8, 9, 63, 64, 65, 129} <= set(sw.tolist())
    items = np.diff(lay["item_ptr"][0])
    for count, width, n_items in ((256, 64, 1), (257, 65, 2), (260, 65, 2), (516, 129, 3)):
        t = list(first).index(count)
        assert sw[t] == width and items[t] == n_items
    zero = np.flatnonzero(first == 0)
    assert len(zero) >= 2 and (sw[zero] == 0).all() and (items[zero] == 0).all()                  # whole slices of zero-count genes
    assert (lay["item_ptr"][0, zero] == lay["item_ptr"][0, zero + 1]).all()
    assert not np.array_equal(lay["perm"][0, :c.G], np.arange(c.G))
    assert (lay["blk_cnt"][1] == 5).all()                                                         # equal counts:
    np.testing.assert_array_equal(lay["perm"][1, :c.G], np.arange(c.G))                           # the slots are the gene ids
    assert not lay["blk_cnt"][2].any() and lay["slice_ptr"][2, -1] == 0
    assert (c.X.data == ref.MAX_COUNT).sum() == 1 and c.X.data[c.X.data != ref.MAX_COUNT].max() <= 4


def test_gene_counts():
    assert gm.GENE_COUNTS == (1, 63, 64, 65, 1023, 1024, 1025)
    # every matrix but the one-gene one has a row that can be put out of order, i.e. reaches the unpartitioned ingest
    assert [n for n in CASES if not gm.can_be_unsorted(reference(n)[0].X)] == ["genes1"] and set(gm.UNSORTABLE) == set(CASES) - {"genes1"}
    for G in gm.GENE_COUNTS:
        c, lay = reference(f"genes{G}")
        assert c.X.shape[1] == G and lay["perm"].shape == (2, -(-G // 64) * 64)
        ties = sum(len(np.unique(lay["blk_cnt"][b])) < G for b in range(2))
        assert ties == 2 or G == 1


def test_big_reaches_its_edges():
    c, lay = reference("big")
    p = lay["plan"]
    assert tuple(p["grp_ncells"]) == (16385, 8193, 0, 8192)
    np.testing.assert_array_equal(np.diff(p["grp_blk0"]), [3, 2, 0, 1])
    assert np.diff(p["blk_cell0"])[-1] == 8192                               # one full block
    assert c.X.shape == (len(c.gid), 1025) and 0.01 < c.X.nnz / np.prod(c.X.shape) < 0.05
    assert lay["blk_cnt"][-1, 0] == 8192 and lay["rank"][-1, 0] == 0          # the largest count a block can hold
    assert (lay["blk_cnt"][:, 0] == np.diff(p["blk_cell0"])).all()           # gene 0: in every cell ...
    tiles, seg = _tiles(c)
    assert all(T == 128 and E >= 128 for T, E in tiles[-1][0])               # ... so n = 128 in every tile of the full block
    assert not lay["blk_cnt"][:, 7].any()
    n_items = gm.reference_moments("big")[3]
    assert n_items[0, 0] == 3 * 22 and n_items[3, 0] == 32 and not n_items[2].any() and not n_items[:, 7].any()
