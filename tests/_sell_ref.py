"""Plain numpy restatement of the count-block layout (include/memento_hip.h) and of the 1D moment sums, for
tests/test_cpu_sell_ref.py and tests/test_gpu_ingest_moments.py.  Written from the documented layout, not from the kernels:

  * cells ordered by group, cut into blocks of <= 8192 cells of one group (engine.plan_blocks: host code, tested on its own);
  * per block the genes are ranked by their stored entries, descending, ties by ascending gene id; 64 slots per slice;
  * a slice is as wide as its FIRST slot needs: ceil(count / 4) rows of 64 lanes x 4 entries; work items of <= 64 rows;
  * entry j of a gene = its j-th cell of the block in ascending cell order, value cell_local | count << 13; the rest is 0.
"""

import numpy as np

from scrna_parameter_estimation_amd.engine import BLOCK_CELLS, MAX_COUNT, RANGE_GENES, plan_blocks

CELL_BITS = 13
JVEC = 4              # entries of one gene per slice row
ITEM_ROWS = 64        # rows of a K1 work item
K1_UNROLL = 8         # rows K1 has in flight (csrc/moments.hip)
TILE_ROWS = 128       # the tile scatter's tile: at most this many rows ...
TILE_ENTRIES = 4096   # ... and this many entries of one gene range
SC_ROWS = 1024        # rows of one workgroup of the row split (csrc/ingest.hip)
assert BLOCK_CELLS == 1 << CELL_BITS and MAX_COUNT == (1 << (32 - CELL_BITS)) - 1


def plan(group_id, n_groups):
    """The cell plan as a dict: cell_order, blk_cell0, blk_group, grp_blk0, grp_ncells."""
    names = ("cell_order", "blk_cell0", "blk_group", "grp_blk0", "grp_ncells")
    return dict(zip(names, plan_blocks(group_id, n_groups)))


def block_triples(X, group_id, n_groups):
    """The stored entries of the selected cells as (block, gene, cell_local, count) int64 arrays, sorted by (block, gene,
    cell_local), and the plan."""
    p = plan(group_id, n_groups)
    order, cell0 = p["cell_order"].astype(np.int64), p["blk_cell0"].astype(np.int64)
    C = X.tocsr()[order].tocoo()
    keep = C.data != 0
    r, g, x = C.row[keep].astype(np.int64), C.col[keep].astype(np.int64), C.data[keep]
    assert (x == np.floor(x)).all() and (x >= 1).all() and (x <= MAX_COUNT).all()
    b = np.searchsorted(cell0, r, side="right") - 1
    cl = r - cell0[b]
    o = np.lexsort((cl, g, b))
    return b[o], g[o], cl[o], x[o].astype(np.int64), p


def sell_layout(X, group_id, n_groups):
    """Every array a CountBlocks of (X, group_id) must hold, bit for bit, as a dict."""
    G = int(X.shape[1])
    b, g, cl, x, p = block_triples(X, group_id, n_groups)
    nb, ns = len(p["blk_group"]), -(-G // 64)
    blk_cnt = np.bincount(b * G + g, minlength=nb * G).reshape(nb, G)
    assert blk_cnt.max(initial=0) <= BLOCK_CELLS
    rank = np.empty((nb, G), dtype=np.int64)
    perm = np.full((nb, ns * 64), -1, dtype=np.int64)
    for k in range(nb):
        by_slot = np.lexsort((np.arange(G), -blk_cnt[k]))          # descending count, ties by ascending gene id
        perm[k, :G] = by_slot
        rank[k, by_slot] = np.arange(G)
    first = perm[:, ::64]                                          # the gene in the first slot of every slice (always a gene)
    slice_w = -(-np.take_along_axis(blk_cnt, first, axis=1) // JVEC)
    zero = np.zeros((nb, 1), dtype=np.int64)
    slice_ptr = np.concatenate([zero, np.cumsum(slice_w, axis=1)], axis=1)
    item_ptr = np.concatenate([zero, np.cumsum(-(-slice_w // ITEM_ROWS), axis=1)], axis=1)
    blk_base = np.concatenate([[0], np.cumsum(slice_ptr[:, -1])]).astype(np.int64)
    blk_item_base = np.concatenate([[0], np.cumsum(item_ptr[:, -1])]).astype(np.int64)
    # entry j of (block, gene): the triples are sorted, so j counts up inside every run of equal (block, gene)
    key = b * G + g
    run0 = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if len(key) else np.zeros(0, dtype=np.int64)
    j = np.arange(len(key)) - np.repeat(run0, np.diff(np.r_[run0, len(key)]))
    slot = rank[b, g]
    word = (blk_base[b] + slice_ptr[b, slot >> 6] + j // JVEC) * 256 + (slot & 63) * JVEC + j % JVEC
    ent = np.zeros(max(1, int(blk_base[-1])) * 256, dtype=np.uint32)
    ent[word] = (cl | (x << CELL_BITS)).astype(np.uint32)
    assert len(np.unique(word)) == len(word)
    return dict(plan=p, blk_cnt=blk_cnt.astype(np.uint16), rank=rank.astype(np.int32), perm=perm.astype(np.int32),
                slice_w=slice_w.astype(np.int32), slice_ptr=slice_ptr.astype(np.int32), item_ptr=item_ptr.astype(np.int32),
                blk_base=blk_base[:-1], blk_item_base=blk_item_base[:-1], total_rows=int(blk_base[-1]),
                total_items=int(blk_item_base[-1]), ent=ent, nnz_sel=len(key),
                ent_key=key, ent_word=word)         # (block * G + gene, word) of every entry: for the arrival-ordered path


def decode(lay):
    """The triples (original cell, gene, count) that the entry array of a layout holds, sorted: non-zero words only."""
    p = lay["plan"]
    nb, ns = lay["slice_w"].shape
    out = []
    for k in range(nb):
        rows = int(lay["slice_ptr"][k, -1])
        blk = lay["ent"][int(lay["blk_base"][k]) * 256:(int(lay["blk_base"][k]) + rows) * 256].reshape(rows, 64, JVEC)
        for t in range(ns):
            e = blk[lay["slice_ptr"][k, t]:lay["slice_ptr"][k, t + 1]]           # [slice_w][lane][4]
            r, lane, q = np.nonzero(e)
            w = e[r, lane, q].astype(np.int64)
            gene = lay["perm"][k, t * 64 + lane].astype(np.int64)
            assert (gene >= 0).all()
            cell = p["cell_order"][p["blk_cell0"][k] + (w & (BLOCK_CELLS - 1))].astype(np.int64)
            out.append(np.stack([cell, gene, w >> CELL_BITS], axis=1))
    a = np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int64)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def segment_lengths(X, p):
    """seg[block][range] = the per-row number of stored entries of that block's cells inside gene range ``range`` (1024 ids);
    ``p``: the cell plan (plan(), or the "plan" of a layout)."""
    G = int(X.shape[1])
    R = -(-G // RANGE_GENES)
    C = X.tocsr()[p["cell_order"].astype(np.int64)].tocoo()
    keep = C.data != 0
    per = np.bincount(C.row[keep].astype(np.int64) * R + C.col[keep] // RANGE_GENES, minlength=len(p["cell_order"]) * R)
    per = per.reshape(len(p["cell_order"]), R)
    return [[per[p["blk_cell0"][k]:p["blk_cell0"][k + 1], rg] for rg in range(R)] for k in range(len(p["blk_group"]))]


def tile_plan(seg_len):
    """The tiles (T rows, E entries) a (block, range) workgroup of the tile scatter takes, from the per-row segment lengths: T is
    the largest extent <= 128 whose entries stay <= 4096, at least 1, clipped at the block's end."""
    seg_len = np.asarray(seg_len, dtype=np.int64)
    assert seg_len.max(initial=0) <= RANGE_GENES
    out, r, n = [], 0, len(seg_len)
    while r < n:
        cum = np.cumsum(seg_len[r:r + TILE_ROWS])
        T = max(1, int((cum <= TILE_ENTRIES).sum()))
        out.append((T, int(cum[T - 1])))
        r += T
    return out


def moment_sums(X, group_id, n_groups, inv_sf, layout=None):
    """S [3][n_groups][G] (np.longdouble: S1 = sum x w, S2 = sum x^2 w^2, S3 = sum x w^2 with w = inv_sf of the cell, every
    product and np.sum's pairwise additions in extended precision), sumx and maxx (exact integers), and n_items [n_groups][G]:
    the K1 work items that feed a (group, gene) -- the items of the gene's slice, over the blocks of the group."""
    lay = layout if layout is not None else sell_layout(X, group_id, n_groups)
    G = int(X.shape[1])
    gid = np.asarray(group_id)
    S = np.zeros((3, n_groups, G), dtype=np.longdouble)
    sumx = np.zeros((n_groups, G), dtype=np.uint64)
    maxx = np.zeros((n_groups, G), dtype=np.uint32)
    n_items = np.zeros((n_groups, G), dtype=np.int64)
    w_all = np.asarray(inv_sf, dtype=np.float64).astype(np.longdouble)
    Xc = X.tocsr()
    for k in range(n_groups):
        cells = np.flatnonzero(gid == k)
        Xg = Xc[cells].tocsc()
        Xg.eliminate_zeros()
        w = w_all[cells]
        for gene in np.flatnonzero(np.diff(Xg.indptr)):
            rows = Xg.indices[Xg.indptr[gene]:Xg.indptr[gene + 1]]
            x = Xg.data[Xg.indptr[gene]:Xg.indptr[gene + 1]].astype(np.longdouble)
            xw = x * w[rows]
            S[0, k, gene] = np.sum(xw)
            S[1, k, gene] = np.sum(xw * xw)
            S[2, k, gene] = np.sum(xw * w[rows])
            xi = x.astype(np.uint64)
            sumx[k, gene] = xi.sum()
            maxx[k, gene] = xi.max()
        for blk in range(lay["plan"]["grp_blk0"][k], lay["plan"]["grp_blk0"][k + 1]):
            t = lay["rank"][blk] >> 6
            n_items[k] += lay["item_ptr"][blk, t + 1] - lay["item_ptr"][blk, t]
    return S, sumx, maxx, n_items
