"""Host-side driver of the HIP kernels: device CSR, SELL count blocks, moments, histograms, bootstrap.

torch is used only as plumbing here (device allocations, H2D/D2H copies, the current HIP stream); all
arithmetic on the hot path happens in libmemento_hip.so (csrc/*.hip) through the C-ABI in
include/memento_hip.h.  Nothing in this module has a CPU fallback.
"""

import ctypes
import functools
import os

from ctypes import c_void_p
from types import SimpleNamespace

import numpy as np

from . import _lib

BLOCK_CELLS = 8192
MAX_COUNT = (1 << 19) - 1
RANGE_GENES, MAX_RANGES = 1024, 64   # include/memento_hip.h: MM_RANGE_GENES, MM_MAX_RANGES (range-partitioned ingest)
MAX_PART_GENES = 60_000              # genes ONE CountBlocks holds (mm_sell_layout's rank table; the other K0 / K1 / K5 kernels stop at 65,536)
PART_GENES = 59_392                  # genes per part of a wider matrix (count_blocks): 58 ranges of 1024, a multiple of 64
ORDER_SMALL_CAP = 1024
ORDER_BIG_CAP = 8192
ORDER_BIG_CAP_2D = 4096
# Lane packing of the replay kernel.  (a) tile widths: every tile gets the same budget K_max * (C0 + C1 * lanes), the budget
# is set so that about PACK_WAVES tiles come out (2 per SIMD, never more than 2048: a third wave on a SIMD is a second round);
# C0/C1/PACK_WAVES were tuned on the hardware together with the pairing order below (profiles/README.md).
PACK_C0 = 220.0
PACK_C1 = 3.0
PACK_WAVES = 2000
# tile target and constants when a third wave per SIMD pays (pack_lanes): 3 x 1024 slots.  Round 3: re-swept for the 1D tile kernel
# that makes one BTPE attempt per bin step -- its wide tiles step 17 % faster, so the balance moves to fewer, wider tiles and more
# lone chains (tools/pack_sweep.py, C3: 3.79 s with round 2's 220 / 3 / 2750, 3.24-3.26 s with these; C2, two waves per SIMD, keeps
# 220 / 3: 267-270 ms against 283).  The 2D kernel keeps the constants it was tuned with.
PACK3_C0 = 260.0
PACK3_C1 = 2.2
PACK_WAVES3 = 4000
PACK2D = (220.0, 3.0, 220.0, 3.0, 2750)
PACK_OVERSUB = 1024      # tiles the three-waves-per-SIMD packing may have beyond the 3 x 1024 resident slots: the shortest ones, dispatched last, start as
                         # the first workgroups retire (C3, tools/pack_sweep.py: 3.18 s with 3,071 tiles, 3.07 / 3.02 / 3.00 / 3.07 / 3.57 s with 3,300 / 3,600 / 4,000 / 4,500 / 5,000)
# (b) measured time of one bin step of a wave of L chains running as the OLDER wave of its SIMD, us (tools/replay_balance.py,
# C3): used to rank tiles by length for the dispatch order (pair_tiles) and to predict a packing's longest tile.  PACK_COST: the 1D
# kernel of round 3 (one BTPE attempt per bin step; a lone chain is a chain wave: 0.70-0.73 us for the longest ones, which are served
# first, 0.9-1.2 for the others); PACK_COST_2D: the 2D kernel (round-2 table).
_PACK_L = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 24, 28, 32, 36, 40, 44, 48, 56, 64)
_PACK_US = (0.72, 1.42, 1.66, 1.88, 2.00, 2.08, 2.18, 2.26, 2.41, 2.49, 2.61, 2.68, 2.77, 2.86, 3.02, 3.13, 3.16, 3.17, 3.18, 3.26, 3.32, 3.60, 3.87)
_PACK_US_2D = (0.96, 1.30, 1.52, 1.72, 1.87, 1.97, 2.09, 2.20, 2.39, 2.56, 2.74, 2.83, 2.99, 3.13, 3.32, 3.55, 3.67, 3.79, 3.90, 4.05, 4.17, 4.50, 4.81)
PACK_COST = np.interp(np.arange(1, 65), _PACK_L, _PACK_US)
PACK_COST_2D = np.interp(np.arange(1, 65), _PACK_L, _PACK_US_2D if os.environ.get('MM_PACK2D_COST', '2d') == '2d' else _PACK_US)   # (env: tools only)
# (c) many-chain regime (more tiles than resident wave slots): 2 x 1024 slots; a SIMD retires ~1.46 lone-wave-seconds of tile
# time per second (older wave 1.0 + younger ~0.46); a tile may take at most PACK_TAIL of the work-bound run time
PACK_MAX_RESIDENT = 2048
PACK_RATE = 1024 * 1.46
PACK_TAIL = float(os.environ.get('MM_PACK_TAIL', '0.5'))   # (env: tools only)
PACK_FORCE = ""          # tools only (tools/pack_sweep.py): "res" / "cap" forces one of the two packings
PACK_LAST = {}          # diagnostics of the last pack_lanes decision (tools/)


def _torch():
    import torch

    return torch


def _stream():
    return c_void_p(_torch().cuda.current_stream().cuda_stream)


def dev(a, dtype=None):
    """numpy -> device tensor (contiguous)."""
    torch = _torch()
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.dtype == np.uint64:  # torch has limited uint64 support: ship the bits as int64
        return torch.from_numpy(a.view(np.int64)).cuda()
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda()
    return torch.from_numpy(a).cuda()


def empty(shape, dtype):
    torch = _torch()
    return torch.empty(shape, dtype=dtype, device="cuda")


def zeros(shape, dtype):
    torch = _torch()
    return torch.zeros(shape, dtype=dtype, device="cuda")


def P(t):
    """device pointer of a tensor (or NULL)."""
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def host(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


class DeviceCSR:
    """The user's CSR on the device: indptr int64, indices int32, data float32 (integer-valued counts)."""

    @classmethod
    def from_device(cls, indptr, indices, data, shape):
        """Wrap CSR arrays that already live in HBM (torch cuda tensors: int64 / int32 / float32).  Precondition (checked by
        the ingest kernel, which raises): every stored value is a positive integer count -- no explicitly stored zeros."""
        torch = _torch()
        assert indptr.dtype == torch.int64 and indices.dtype == torch.int32 and data.dtype == torch.float32
        self = cls.__new__(cls)
        self.shape = (int(shape[0]), int(shape[1]))
        self.nnz = int(indices.numel())
        self.indptr, self.indices, self.data = indptr.contiguous(), indices.contiguous(), data.contiguous()
        return self

    def __init__(self, X):
        import scipy.sparse as sp

        if not sp.isspmatrix_csr(X):
            raise TypeError("X must be a scipy.sparse.csr_matrix")
        if not X.has_canonical_format:
            X = X.copy()
            X.sum_duplicates()
        if X.nnz and (X.data == 0).any():
            # explicitly stored zeros (common after subsetting or arithmetic on adata.X; the reference accepts any scipy CSR,
            # main.py:44): they carry no count, drop them from the device copy
            X = X.copy()
            X.eliminate_zeros()
        self.shape = X.shape
        self.nnz = int(X.nnz)
        data = X.data
        if data.dtype != np.float32:
            d32 = data.astype(np.float32)
            if not np.array_equal(d32.astype(data.dtype), data):
                raise ValueError("count matrix values are not exactly representable in float32")
            data = d32
        self.indptr = dev(X.indptr, np.int64)
        self.indices = dev(X.indices, np.int32)
        self.data = dev(data, np.float32)

    @property
    def nbytes(self):
        return self.indptr.numel() * 8 + self.indices.numel() * 4 + self.data.numel() * 4

    _spare = None

    def entry_ptrs(self):
        """Device pointers of (indices, data) for the C-ABI.  A tensor without elements has a null pointer, which every entry point
        refuses, and the tile scatter reads element 0 on behalf of a tile without entries: a CSR without a stored entry lends a
        one-element buffer of each instead (as colsplit keeps one behind its outputs)."""
        if self.nnz:
            return P(self.indices), P(self.data)
        if self._spare is None:
            torch = _torch()
            self._spare = (zeros((1,), torch.int32), zeros((1,), torch.float32))
        return P(self._spare[0]), P(self._spare[1])

    def colsplit(self, lo, hi):
        """The gene (column) range [lo, hi) as a new device CSR with columns renumbered from 0 -- the device-side replacement
        of the host ``X[:, lo:hi]`` in front of gene-sharded multi-GPU runs (mm_csr_colcount + mm_csr_colsplit)."""
        torch = _torch()
        lo, hi = int(lo), int(hi)
        if not (0 <= lo <= hi <= self.shape[1]):
            raise ValueError("column range out of bounds")
        n = self.shape[0]
        row_nnz = empty((max(1, n),), torch.int64)
        _lib.call("mm_csr_colcount", P(self.indptr), self.entry_ptrs()[0], n, lo, hi, P(row_nnz), _stream())
        indptr = zeros((n + 1,), torch.int64)
        if n:
            indptr[1:] = torch.cumsum(row_nnz[:n], 0)
        nnz = int(indptr[-1].item())
        indices = empty((max(1, nnz),), torch.int32)
        data = empty((max(1, nnz),), torch.float32)
        _lib.call("mm_csr_colsplit", P(self.indptr), *self.entry_ptrs(), n, lo, hi, P(indptr), P(indices), P(data), _stream())
        return DeviceCSR.from_device(indptr, indices[:nnz], data[:nnz], (n, hi - lo))

    def colselect(self, genes):
        """The columns ``genes`` (ascending indices) as a new device CSR with columns renumbered 0..len(genes)-1: the gene SET
        of a cost-balanced shard (mm_csr_mapcount + mm_csr_mapsplit)."""
        torch = _torch()
        genes = np.asarray(genes, dtype=np.int64)
        if len(genes) and (np.diff(genes) <= 0).any():
            raise ValueError("gene indices must ascend")
        if len(genes) and not (0 <= genes[0] and genes[-1] < self.shape[1]):
            raise ValueError("gene index out of bounds")
        n = self.shape[0]
        col_map = np.full(self.shape[1], -1, dtype=np.int32)
        col_map[genes] = np.arange(len(genes), dtype=np.int32)
        d_map = dev(col_map)
        row_nnz = empty((max(1, n),), torch.int64)
        _lib.call("mm_csr_mapcount", P(self.indptr), self.entry_ptrs()[0], n, P(d_map), P(row_nnz), _stream())
        indptr = zeros((n + 1,), torch.int64)
        if n:
            indptr[1:] = torch.cumsum(row_nnz[:n], 0)
        nnz = int(indptr[-1].item())
        indices = empty((max(1, nnz),), torch.int32)
        data = empty((max(1, nnz),), torch.float32)
        _lib.call("mm_csr_mapsplit", P(self.indptr), *self.entry_ptrs(), n, P(d_map), P(indptr), P(indices), P(data), _stream())
        return DeviceCSR.from_device(indptr, indices[:nnz], data[:nnz], (n, len(genes)))

    def colsum(self):
        """Per-gene totals (host array): what the cost-balanced gene sharding is computed from."""
        torch = _torch()
        out = zeros((max(1, self.shape[1]),), torch.float64)
        _lib.call("mm_csr_colsum", *self.entry_ptrs(), self.nnz, P(out), _stream())
        return host(out)[: self.shape[1]]

    def rowsum(self, gene_mask=None):
        """K3: per-cell sums, optionally over a gene mask (estimator.py:65, :73)."""
        torch = _torch()
        out = empty((self.shape[0],), torch.float64)
        m = dev(np.asarray(gene_mask, dtype=np.uint8)) if gene_mask is not None else None
        _lib.call("mm_csr_rowsum", P(self.indptr), *self.entry_ptrs(), self.shape[0], P(m), P(out), _stream())
        return host(out)


def auto_max_rows(ld, arrays=2, fraction=0.4):
    """Rows of replicate buffers ([rows][ld] fp64, ``arrays`` of them plus one coefficient buffer) that fit in
    ``fraction`` of the currently free HBM."""
    torch = _torch()
    free, _ = torch.cuda.mem_get_info()
    free += max(0, torch.cuda.memory_reserved() - torch.cuda.memory_allocated())    # blocks the caching allocator holds but nobody uses
    return max(1024, int(free * fraction) // (int(ld) * 8 * (arrays + 1)))


def plan_blocks(group_id, n_groups, block_cells=BLOCK_CELLS):
    """Order cells by group (stable) and cut every group into near-equal blocks of <= block_cells.

    Returns cell_order, blk_cell0 (nb+1), blk_group (nb), grp_blk0 (n_groups+1), grp_ncells."""
    group_id = np.asarray(group_id)
    sel = np.flatnonzero(group_id >= 0)
    order = sel[np.argsort(group_id[sel], kind="stable")].astype(np.int32)
    counts = np.bincount(group_id[sel], minlength=n_groups).astype(np.int64)
    blk_cell0, blk_group, grp_blk0 = [0], [], [0]
    pos = 0
    for g in range(n_groups):
        n = int(counts[g])
        nb = max(1, -(-n // block_cells)) if n > 0 else 0
        for k in range(nb):
            pos_end = pos + (n * (k + 1)) // nb - (n * k) // nb
            blk_group.append(g)
            blk_cell0.append(pos_end)
            pos = pos_end
        grp_blk0.append(len(blk_group))
    return (order, np.asarray(blk_cell0, dtype=np.int32), np.asarray(blk_group, dtype=np.int32),
            np.asarray(grp_blk0, dtype=np.int32), counts)


def plan_parts(G, part_genes=PART_GENES):
    """Gene ranges [(lo, hi), ...] of the count-block parts of a G-gene matrix: ascending, contiguous, covering [0, G), each at most
    ``part_genes`` wide (every part but the last exactly that).  One part iff G <= part_genes."""
    G, part_genes = int(G), int(part_genes)
    if not 0 < part_genes <= MAX_PART_GENES:
        raise ValueError(f"part_genes must be in 1..{MAX_PART_GENES}")
    if G < 0:
        raise ValueError("G must not be negative")
    return [(lo, min(G, lo + part_genes)) for lo in range(0, max(1, G), part_genes)]


_BAD_COUNTS = f"count matrix must hold positive integer counts <= {MAX_COUNT} with valid column indices"


class CountBlocks:
    """K0 result: the group-ordered SELL-64x4 count blocks living in HBM (see include/memento_hip.h).  One object holds at most
    MAX_PART_GENES genes (LDS budgets of the K0 / K1 / K5 kernels); ``count_blocks`` builds wider matrices from several."""

    def __init__(self, csr, group_id, n_groups, timing=None):
        """``timing``: an optional dict that receives the HIP-event time (ms) of each of the three K0 launches
        (bench.py's CSR -> moments roofline; the launches are otherwise untimed)."""
        if int(csr.shape[1]) > MAX_PART_GENES:
            raise ValueError(f"one CountBlocks holds at most {MAX_PART_GENES} genes, got {int(csr.shape[1])}: "
                             "build the blocks of a wider matrix with engine.count_blocks")
        torch = _torch()
        call = _lib.call if timing is None else (lambda name, *a: _timed_call(timing, name, *a))
        self.G = int(csr.shape[1])
        self.n_groups = int(n_groups)
        (self.cell_order, self.blk_cell0, self.blk_group, self.grp_blk0, self.grp_ncells) = plan_blocks(group_id, n_groups)
        nb = self.n_blocks = len(self.blk_group)
        G = self.G
        self.n_slices = (G + 63) // 64
        ns = self.n_slices
        s = _stream()
        self.d_cell_order = dev(self.cell_order)
        self.d_blk_cell0 = dev(self.blk_cell0)
        self.d_blk_group = dev(self.blk_group)
        self.d_grp_blk0 = dev(self.grp_blk0)
        blk_cnt_buf = zeros((nb * G + 2,), torch.int16)     # (the fused split + count merges 16-bit halves by 32-bit atomics)
        blk_cnt = blk_cnt_buf[:nb * G].view(nb, G)
        status = zeros((1,), torch.int32)
        bad_data = ValueError(_BAD_COUNTS)
        # Range-partitioned ingest (rows with ascending column indices: every canonical CSR): a workgroup owns (block, range of
        # 1024 consecutive gene ids), so a row contributes one contiguous segment to it and the per-gene state of the range lives
        # in LDS (csrc/ingest.hip).
        n_sel = len(self.cell_order)
        R = -(-G // RANGE_GENES)          # (<= MAX_RANGES: G <= MAX_PART_GENES)
        rowsplit = empty((R + 1, max(1, n_sel)), torch.int64)     # [range][row]
        call("mm_sell_split_count", P(csr.indptr), csr.entry_ptrs()[0], P(self.d_cell_order), P(self.d_blk_cell0), nb, n_sel, G, R,
             P(rowsplit), P(blk_cnt_buf), P(status), s)
        self.ranged = (int(status.item()) & 2) == 0
        if not self.ranged:       # unsorted rows (or column indices out of range: reported by the count kernel): the unpartitioned kernels
            status.zero_()
            call("mm_sell_count", P(csr.indptr), *csr.entry_ptrs(), P(self.d_cell_order), P(self.d_blk_cell0), nb, G,
                 P(blk_cnt), P(status), s)
            if int(status.item()) != 0:
                raise bad_data
        self.rank = empty((nb, G), torch.int32)
        self.perm = empty((nb, ns * 64), torch.int32)
        self.slice_w = empty((nb, ns), torch.int32)
        self.slice_ptr = empty((nb, ns + 1), torch.int32)
        self.item_ptr = empty((nb, ns + 1), torch.int32)
        blk_rows = empty((nb,), torch.int64)
        blk_items = empty((nb,), torch.int32)
        call("mm_sell_layout", P(blk_cnt), nb, G, P(self.rank), P(self.perm), P(self.slice_w), P(self.slice_ptr),
                  P(self.item_ptr), P(blk_rows), P(blk_items), s)
        rows = host(blk_rows)
        items = host(blk_items).astype(np.int64)
        base = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        ibase = np.concatenate([[0], np.cumsum(items)]).astype(np.int64)
        self.total_rows = int(base[-1])
        self.total_items = int(ibase[-1])
        self.blk_base = dev(base[:-1])
        self.blk_item_base = dev(ibase[:-1])
        self.ent = zeros((max(1, self.total_rows) * 256,), torch.int32)
        if self.ranged:
            call("mm_sell_scatter_ranges", P(csr.indptr), *csr.entry_ptrs(), P(self.d_cell_order), P(self.d_blk_cell0), nb, G, R,
                 n_sel, P(rowsplit), P(self.rank), P(self.slice_ptr), P(self.blk_base), P(self.ent), P(status), s)
            if int(status.item()) & 1:
                raise bad_data
        else:
            call("mm_sell_scatter", P(csr.indptr), *csr.entry_ptrs(), P(self.d_cell_order), P(self.d_blk_cell0), nb, G,
                 P(self.rank), P(self.slice_ptr), P(self.blk_base), P(self.ent), s)
        del rowsplit
        self.blk_cnt = host(blk_cnt, np.uint16)            # nnz per (block, gene), host copy [nb][G]
        self.nnz_sel = int(self.blk_cnt.astype(np.int64).sum())
        del blk_cnt
        # slab for K1 partial sums (reused across calls)
        n = max(1, self.total_items) * 64
        self._slab = empty((n * 8,), torch.int32)          # 32-byte record per (item, lane): S1, S2, S3 (fp64), sum x, max x

    part_lo = (0,)

    @property
    def parts(self):
        """The gene parts the consumers loop over: this object, from gene 0 (a WideCountBlocks has several).  A property: stored on
        the object it would be a reference cycle, and the device buffers would wait for the cycle collector."""
        return (self,)

    @property
    def ent_bytes(self):
        return self.total_rows * 1024

    def moments_bytes(self):
        """Algorithmic HBM bytes of one mm_moments1d_sell launch on this layout: the packed entries (4 B each
        incl. the slice padding actually stored), per-item pointers, the staged 1/sf and the slab written."""
        return (self.total_rows * 1024 + self.n_blocks * (self.n_slices * 12 + 8) + len(self.cell_order) * 8
                + self.total_items * 64 * 32)

    def launch_moments(self, d_inv_sf):
        """Enqueue only the K1 kernel (used by bench.py to time the roofline kernel)."""
        _lib.call("mm_moments1d_sell", P(self.ent), P(self.blk_base), P(self.slice_w), P(self.slice_ptr), P(self.item_ptr),
                  P(self.blk_item_base), P(self.d_blk_cell0), P(d_inv_sf), self.n_blocks, self.G, P(self._slab), _stream())

    def moments(self, inv_sf_cells):
        """K1+K2.  ``inv_sf_cells``: 1/size_factor per ORIGINAL cell index.  Returns host arrays
        S (3, n_groups, G) float64, sumx (n_groups, G) uint64, maxx (n_groups, G) uint32."""
        torch = _torch()
        d_inv = dev(np.asarray(inv_sf_cells, dtype=np.float64)[self.cell_order])
        self.launch_moments(d_inv)
        out_S = empty((3, self.n_groups, self.G), torch.float64)
        out_sx = empty((self.n_groups, self.G), torch.int64)
        out_mx = empty((self.n_groups, self.G), torch.int32)
        _lib.call("mm_moments1d_reduce", P(self._slab), P(self.rank),
                  P(self.item_ptr), P(self.blk_item_base), P(self.d_grp_blk0), self.n_groups, self.G, P(out_S), P(out_sx),
                  P(out_mx), _stream())
        return host(out_S), host(out_sx, np.uint64), host(out_mx, np.uint32)


class WideCountBlocks:
    """Count blocks of a matrix with more genes than one CountBlocks holds: one CountBlocks per gene range of ``plan_parts``, all on
    the same cell plan (plan_blocks depends only on the grouping).  Offers what the consumers of count blocks read -- the common cell
    plan, ``blk_cnt`` / ``moments`` over the whole gene axis, and ``parts`` / ``part_lo`` for the kernels that read the entries:
    Bootstrap1D and GeneColumns launch once per part with that part's slice of their gene -> output map, into the one output."""

    def __init__(self, parts, part_lo, G):
        self.parts, self.part_lo, self.G = tuple(parts), tuple(int(lo) for lo in part_lo), int(G)
        p0 = self.parts[0]
        for name in ("n_groups", "n_blocks", "cell_order", "blk_cell0", "blk_group", "grp_blk0", "grp_ncells",
                     "d_cell_order", "d_blk_cell0", "d_blk_group", "d_grp_blk0"):
            setattr(self, name, getattr(p0, name))
        self.blk_cnt = np.concatenate([p.blk_cnt for p in self.parts], axis=1)      # [nb][G]
        self.nnz_sel = sum(p.nnz_sel for p in self.parts)
        self.ranged = all(p.ranged for p in self.parts)

    def moments(self, inv_sf_cells):
        """K1+K2 of every part, concatenated along the gene axis: S (3, n_groups, G), sumx (n_groups, G), maxx (n_groups, G)."""
        res = [p.moments(inv_sf_cells) for p in self.parts]
        return tuple(np.concatenate([r[i] for r in res], axis=-1) for i in range(3))


def count_blocks(csr, group_id, n_groups, timing=None, part_genes=None):
    """The count blocks of ``csr`` whatever its width: a CountBlocks when the genes fit one part (the same object and launches as the
    direct constructor), else a WideCountBlocks of one CountBlocks per gene range, each ingested from a column split of ``csr`` that
    is released before the next is cut (extra memory: one part's indices + data).  ``timing`` also receives the HIP-event time of
    the splits under 'colsplit'.  ``part_genes``: by default a matrix that fits one CountBlocks (<= MAX_PART_GENES genes) stays one part,
    as it always was, and a wider one is cut into parts of PART_GENES; a value (<= MAX_PART_GENES) cuts parts of exactly that width --
    it exists for tests that need several parts at small shapes."""
    G = int(csr.shape[1])
    ranges = plan_parts(G, part_genes if part_genes is not None else PART_GENES if G > MAX_PART_GENES else MAX_PART_GENES)
    if len(ranges) == 1:
        return CountBlocks(csr, group_id, n_groups, timing=timing)
    parts = []
    for lo, hi in ranges:
        sub = csr.colsplit(lo, hi) if timing is None else _timed(timing, "colsplit", _stream(), lambda: csr.colsplit(lo, hi))
        parts.append(CountBlocks(sub, group_id, n_groups, timing=timing))
        del sub
    wide = WideCountBlocks(parts, [lo for lo, _ in ranges], csr.shape[1])
    # colsplit drops an entry whose column lies in no part, so an invalid column index never reaches a part's ingest check: every
    # stored entry of the selected cells must have arrived in some part
    indptr = host(csr.indptr)
    if int((indptr[wide.cell_order.astype(np.int64) + 1] - indptr[wide.cell_order]).sum()) != wide.nnz_sel:
        raise ValueError(_BAD_COUNTS)
    return wide


def _timed(timing, key, stream, fn):
    """fn() bracketed by HIP events on ``stream``; elapsed ms is added to timing[key].  Returns fn's result."""
    t = c_void_p()
    ms = ctypes.c_float()
    _lib.call("mm_timer_create", ctypes.byref(t))
    _lib.call("mm_timer_begin", t, stream)
    res = fn()
    _lib.call("mm_timer_end", t, stream)
    _lib.call("mm_timer_elapsed_ms", t, ctypes.byref(ms))
    _lib.call("mm_timer_destroy", t)
    timing[key] = timing.get(key, 0.0) + float(ms.value)
    return res


def _timed_call(timing, name, *args):
    """_lib.call bracketed by HIP events on the launch stream (last argument); elapsed ms -> timing[name]."""
    _timed(timing, name, args[-1], lambda: _lib.call(name, *args))


def _tiles_from_lanes(lanes, n_act):
    slot_of = np.zeros(n_act, dtype=np.int64)
    n_tiles, pos = 0, 0
    while pos < n_act:
        L = int(lanes[pos])
        run_end = int(np.searchsorted(lanes, L, side="right"))
        cnt = run_end - pos
        idx = np.arange(cnt)
        slot_of[pos:run_end] = (n_tiles + idx // L) * 64 + idx % L
        n_tiles += -(-cnt // L)
        pos = run_end
    return slot_of, n_tiles


def pack_lanes(K_sorted_desc, target_waves, dense=False, consts=None, cost=None):
    """Lane packing of sequential chains into 64-wide tiles (one tile = one wave).

    ``K_sorted_desc``: steps of each chain, descending.  A chain is one sequential stream, so a wave costs about
    K_max(lanes) x c(L), c(L) = C0 + C1*L per bin step (lanes diverge between the inversion and BTPE samplers and every
    data-dependent loop runs for the slowest lane).  Wide waves are the most instruction-efficient, but the heaviest chain
    bounds the makespan; so every wave gets the same cost budget: L(K) = largest lane count with K*c(L) <= budget, and the
    budget is chosen (bisection) to yield about ``target_waves`` waves, all resident at once ("resident" packing).  With very
    many chains a second, work-bound packing (see below) is built as well and the one with the shorter predicted run time
    is returned.  ``dense``: plain 64-wide tiles (fast mode: one wave per chain, lanes = replicates).
    Returns (slot of every chain = tile*64 + lane, number of tiles)."""
    Ks = np.maximum(np.asarray(K_sorted_desc, dtype=np.float64), 1.0)
    n_act = len(Ks)
    if n_act == 0:
        return np.zeros(0, dtype=np.int64), 0
    if dense:
        return _tiles_from_lanes(np.full(n_act, 64, dtype=np.int64), n_act)
    C0, C1, C0_3, C1_3, WAVES3 = consts if consts is not None else (PACK_C0, PACK_C1, PACK3_C0, PACK3_C1, PACK_WAVES3)

    def resident(n_waves, C0, C1):
        def lanes_for(budget):
            return np.clip(np.floor((budget / Ks - C0) / C1), 1, 64)

        lo_b, hi_b = C0 + C1, float(Ks.max()) * (C0 + 64 * C1) * 4.0
        for _ in range(50):
            mid = 0.5 * (lo_b + hi_b)
            if (1.0 / lanes_for(mid)).sum() > n_waves:
                lo_b = mid
            else:
                hi_b = mid
        return np.maximum.accumulate(lanes_for(hi_b).astype(np.int64))

    lanes = resident(target_waves, C0, C1)
    c = PACK_COST if cost is None else cost
    # MANY chains (2D pair lists, hundreds of groups): 64-wide tiles no longer fit the resident wave slots, or they fit only
    # because even the longest chains were made 64 wide (a 64-wide step costs 6x a lone chain's, and that tile then runs
    # long after everything else has finished).  There the schedule should be work-bound instead: tiles run in several
    # rounds, the dispatcher refills slots as waves retire, every tile is capped at T = PACK_TAIL x (total work / machine
    # rate) with the measured step costs -- T is a fixed point because narrower tiles for the long chains add work.

    def width(T):
        return np.clip(np.searchsorted(c, T / Ks, side="right"), 1, 64)

    def work(L):
        return float((Ks * c[L - 1] / L).sum()) / PACK_RATE

    def gap(T):
        return T - PACK_TAIL * work(width(T))

    lo_t, hi_t = float(Ks[0]) * c[0], float(Ks[0]) * c[63]
    if gap(lo_t) >= 0:
        T = lo_t                      # the longest chain, alone in its wave, already is the tail
    elif gap(hi_t) <= 0:
        T = hi_t                      # so much work that even the longest chains can ride 64-wide
    else:
        for _ in range(40):
            mid = 0.5 * (lo_t + hi_t)
            if gap(mid) < 0:
                lo_t = mid
            else:
                hi_t = mid
        T = hi_t
    lanes_w = np.maximum.accumulate(width(T).astype(np.int64))
    # choose by predicted run time (in units of lone-wave step time): resident tiles finish when their longest tile does
    # (measured / predicted: C3 6.21 / 6.25 s; 2D kernel 1.33-1.38x on three sizes); the work-bound schedule takes about 1.35x
    # the larger of its ideal work time and its tile cap (C3 1.33x; 2D 1.4x on four sizes, after the same kernel factor)
    longest_resident = float((Ks * c[lanes - 1]).max())
    n_res = float((1.0 / lanes).sum())
    use_work_bound = n_res > PACK_MAX_RESIDENT or 1.35 * max(work(lanes_w), T) < longest_resident
    if PACK_FORCE:
        use_work_bound = PACK_FORCE == "cap" or n_res > PACK_MAX_RESIDENT
    PACK_LAST.update(chains=n_act, tiles_resident=n_res, longest_resident=longest_resident, work_resident=work(lanes),
                     T_work_bound=T, work_work_bound=work(lanes_w), tiles_work_bound=float((1.0 / lanes_w).sum()),
                     chosen="work-bound" if use_work_bound else "resident")
    if use_work_bound:
        lanes = lanes_w
    elif target_waves == PACK_WAVES and WAVES3 > PACK_WAVES:
        # A third wave per SIMD (the kernels' 3-wave build, taken above 2048 tiles): narrower tiles for the same chains.  It
        # pays when the longest tile gets shorter -- the waves of this kernel leave ~40 % of the issue slots empty, a third wave
        # fills some -- and costs when the longest chain is already alone in its tile (then only the work grows).  Measured
        # (tools/pack_sweep.py, 2000 vs 2750 tiles): C3 shapes with 250k / 500k / 1M cells 2889 -> 2738, 3162 -> 2993,
        # 3815 -> 3591 ms (model: longest tile -8 to -10 %); C2 368 -> 391 ms (model: longest tile unchanged).  Round-3 kernel: C3
        # 3.32-3.38 s with two waves per SIMD (2,018 tiles), 3.24-3.28 s with three (3,071; model -5 %); C2 (bounded by its longest
        # chain alone in a wave, 0.25 of 0.26 s) stays at two.
        lanes3, w3 = resident(WAVES3, C0_3, C1_3), WAVES3
        while _tiles_from_lanes(lanes3, n_act)[1] > 3 * PAIR_SLOTS + PACK_OVERSUB and w3 > PACK_WAVES:   # (whole tiles: every lane count rounds up)
            w3 -= 16
            lanes3 = resident(w3, C0_3, C1_3)
        if float((1.0 / lanes3).sum()) <= 3 * PAIR_SLOTS + PACK_OVERSUB and float((Ks * c[lanes3 - 1]).max()) <= 0.97 * longest_resident:
            lanes = lanes3
            PACK_LAST.update(chosen="resident, 3 waves / SIMD", tiles_resident=float((1.0 / lanes3).sum()))
    return _tiles_from_lanes(lanes, n_act)


# Which chains run one per WAVE (mm_boot1d_chain: wave-uniform samplers, the 64 lanes produce the PCG64 stream in batches)
# instead of one per lane of a tile.  CHAIN_LONE: every chain the packer leaves ALONE in its tile -- the long ones; a lone chain
# steps in 0.75 us there against 0.96-1.2 us as the only lane of a tile wave.  CHAIN_MIN_K > 0: in addition every chain with at
# least that many bins (tests / tools; 2 = all of them).  Both kernels replay the same draws, bit for bit.
CHAIN_SLOT = 1 << 62      # include/memento_hip.h: MM_CHAIN_SLOT
CHAIN_LONE = os.environ.get('MM_CHAIN_LONE', '1') != '0'        # (the MM_* environment overrides below exist for the measurement tools)
CHAIN_MIN_K = int(os.environ.get('MM_CHAIN_MIN_K', '0'))
# FEW chains (a gene shard of a multi-GPU run): with at most this many chains in a launch every chain gets a wave of its own --
# three rounds of the chip's wave slots at most; lane-sharing tiles only pay when there are far more chains than wave slots.
# Measured on the 8 / 4 / 2 cost-balanced gene shards of C3 (5.4k / 10.8k / 21.6k chains; bench.py --predict-shards): all chains one
# per wave 1.71-2.49 s / 3.13-3.19 s / 6.0 s per shard against 2.53-2.87 / 2.98-3.09 / 3.2-3.3 s with tiles + lone chains.
CHAIN_ALL_MAX = int(os.environ.get('MM_CHAIN_ALL_MAX', '8192'))
# The other chains: TILE_MODE "async" = lane-asynchronous tile kernel (mm_boot1d_async: every lane walks its own chain at its
# own pace, 64 chains of similar length per wave; chains with >= ASYNC_CHAIN_MIN_K bins go one per wave to mm_boot1d_chain);
# "lockstep" = round 1-2's tile kernel (mm_boot1d_replay with the cost-model packing below; kept for A/B runs and the 2D path).
TILE_MODE = os.environ.get('MM_TILE_MODE', 'lockstep')
# Tiles whose lanes also run free ACROSS replicates (mm_boot1d_free: per-chain operand records instead of shared rows).  OFF, measured at
# C3: 3.57 s against 2.99 s.  A lane no longer waits for the slowest lane of its replicate (1.13 bin steps per nominal step instead of
# 1.23) -- but those waits were cheap: the last steps of a replicate run with few lanes left and cost accordingly (3.21 us per step made on
# average against 4.12 us for a step of 64 busy lanes), so the launch pays for lane-steps either way; the records alone cost 3 %
# (3.09 s with the lanes meeting at the end of each replicate), the per-lane replicate epilogue 4 %.  Bit-identical, kept as a tested option.
TILE_FREE = os.environ.get('MM_TILE_FREE', '0') != '0'
# 2D replay on per-chain operand records with one BTPE attempt per bin step (mm_boot2d_replay_rec) instead of shared rows, every attempt in its step
BOOT2D_RECORDS = os.environ.get('MM_BOOT2D_RECORDS', '1') != '0'
ASYNC_CHAIN_MIN_K = int(os.environ.get('MM_ASYNC_CHAIN_MIN_K', '160'))
ASYNC_LANES = int(os.environ.get('MM_ASYNC_LANES', '64'))      # chains per wave of the async kernel (the other lanes idle)
CHAIN_CLOCK_OFF = 1 << 18   # int64 offset of the chain kernel's records in the mm_debug_wave_clock buffer (tools/)

PAIR_SLOTS = 1024      # SIMDs: tiles t and t + PAIR_SLOTS share one
PAIR_TILES = os.environ.get('MM_PAIR_TILES', '1') != '0'      # tools only: False = plain longest-first dispatch order


def pair_tiles(slot_of, n_tiles, K_of, cost=None):
    """Dispatch order of the replay tiles.  Two waves share a SIMD and the OLDER one is served first (measured: the
    younger wave runs at ~0.46 of its lone speed until the older retires, tools/replay_balance.py).  Workgroups are handed
    out round-robin, so tile t and tile t + 1024 meet on one SIMD: put the 1024 longest tiles first, longest first, and
    behind them the next 1024 in ASCENDING length -- the longest tile then shares its SIMD with the shortest partner
    instead of one of its own size; anything beyond 2048 follows longest-first and refills slots as they free up."""
    if not PAIR_TILES or n_tiles <= 2:
        return slot_of
    tile = slot_of // 64
    lanes = np.bincount(tile, minlength=n_tiles)
    kmax = np.zeros(n_tiles)
    np.maximum.at(kmax, tile, np.asarray(K_of, dtype=np.float64))
    est = kmax * (PACK_COST if cost is None else cost)[np.clip(lanes, 1, 64) - 1]
    by_len = np.argsort(-est, kind="stable")
    h = min(PAIR_SLOTS, n_tiles // 2 + n_tiles % 2)
    first, rest = by_len[:h], by_len[h:]
    second, tail = rest[:h][::-1], rest[h:]
    new_order = np.concatenate([first, second, tail])
    new_id = np.empty(n_tiles, dtype=np.int64)
    new_id[new_order] = np.arange(n_tiles)
    return new_id[tile] * 64 + slot_of % 64


_PCG_MULT = 0x2360ED051FC65DA44385DF649FCCF645
_JUMP_CACHE = {}
_SIDE_STREAM = []


def pcg64_jump_table(seed=5):
    """Device table [64][4] uint64 for mm_boot1d_chain: row j = (A^(j+1) hi, lo, C_(j+1) hi, lo) with
    state_(i+j+1) = A^(j+1) * state_i + C_(j+1) (mod 2^128) for np.random.PCG64(seed)'s increment."""
    if seed not in _JUMP_CACHE:
        inc = np.random.PCG64(seed).state["state"]["inc"]
        m64, M = (1 << 64) - 1, 1 << 128
        a, c, rows = 1, 0, []
        for _ in range(64):
            a = (a * _PCG_MULT) % M
            c = (c * _PCG_MULT + inc) % M
            rows.append([a >> 64, a & m64, c >> 64, c & m64])
        _JUMP_CACHE[seed] = dev(np.array(rows, dtype=np.uint64))
    return _JUMP_CACHE[seed]


_STREAM_CACHE = {}
def pcg64_stream_table(seed, n):
    """Device table of the first ``n`` uniforms of Generator(PCG64(seed)) (mm_pcg64_stream); cached and grown on demand -- its
    content depends on nothing but the seed.  (No kernel reads it: tile lanes that took their uniforms from it instead of stepping
    PCG64 measured 4.12-4.16 s against 3.53 s at C3, a wave's lanes sit at 64 different places of the table.)"""
    torch = _torch()
    t = _STREAM_CACHE.get(seed)
    if t is None or t.numel() < n:
        n_alloc = int(n * 1.25) + 4096
        t = empty((n_alloc,), torch.float64)
        _lib.call("mm_pcg64_stream", pcg64_state(seed), n_alloc, P(t), _stream())
        _STREAM_CACHE[seed] = t
    return t


def side_stream():
    """A second HIP stream (torch plumbing) on which the chain kernel runs beside the tile kernel."""
    if not _SIDE_STREAM:
        _SIDE_STREAM.append(_torch().cuda.Stream())
    return _SIDE_STREAM[0]


def pcg64_state(seed=5):
    """(state_hi, state_lo, inc_hi, inc_lo) of np.random.PCG64(seed) -- what bootstrap.py:102 constructs."""
    st = np.random.PCG64(seed).state["state"]
    m = (1 << 64) - 1
    return (ctypes.c_uint64 * 4)(st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m)


def _replay_order(code, mu, n_cells):
    """Replay order of ONE chain's bins computed on the host, with the arithmetic of k_bins_order: ``code``
    ascending (bootstrap.py:62-67), pk = pix / remaining_p, log(1 - p) after the p > 0.5 flip.  Returns (order, pk, lq)."""
    o = np.argsort(code, kind="stable")
    if len(o) > 1 and (np.diff(code[o]) == 0).any():
        raise NotImplementedError("two bins of one pair collided in the replay hash (np.unique would merge them)")
    pix = mu[o].astype(np.float64) / float(n_cells)
    rem = np.empty_like(pix)
    acc = 1.0
    for k in range(len(pix)):      # sequential rounding, exactly like numpy's remaining_p
        rem[k] = acc
        acc -= pix[k]
    pk = pix / rem
    peff = np.where(pk <= 0.5, pk, 1.0 - pk)
    with np.errstate(divide="ignore", invalid="ignore"):
        lq = np.log(1.0 - peff)
    return o, pk, lq


def _write_chain_operands(recbuf, ops, slot, tile_ptr, vals):
    """Operands of ONE chain, per bin the values ``vals`` (pk, lq, ...), written where the kernels read them: a CHAIN_SLOT slot = 8-double
    records in ``recbuf`` (the slot's low bits number the first record), any other slot = its lane of the tile's rows in the planes ``ops``."""
    if slot & CHAIN_SLOT:
        rec = np.zeros((len(vals[0]), 8))
        for i, x in enumerate(vals):
            rec[:, i] = x
        r0_ = (slot & (CHAIN_SLOT - 1)) * 8
        recbuf[r0_:r0_ + rec.size] = dev(rec.reshape(-1))
        return
    idx = dev((int(tile_ptr[slot >> 6]) + np.arange(len(vals[0]), dtype=np.int64)) * 64 + (slot & 63))
    for arr, x in zip(ops, vals):
        arr[idx] = dev(x)


def _per_slot(n_slots, slot_of, vals, fill, dtype):
    """[n_slots] array with vals[i] in slot slot_of[i] and ``fill`` in the unused slots."""
    a = np.full(n_slots, fill, dtype=dtype)
    a[slot_of] = vals
    return a


def _plan_tiles(K, order, slot_of, n_tiles, n_chains, grp_ncells, grp_q, ng):
    """Slot tables of a tile launch (1D and 2D): chain order[i] (of ``n_chains`` in all, group = chain % ng) runs in slot
    slot_of[i] = 64 * tile + lane.  tile_ptr: tile t owns operand rows [tile_ptr[t], tile_ptr[t + 1]), as many as its longest chain."""
    t = SimpleNamespace()
    t.pair_slot = _per_slot(n_chains, order, slot_of, -1, np.int64)
    t.slot_pair = _per_slot(n_tiles * 64, slot_of, order, -1, np.int64)
    t.slot_K = _per_slot(n_tiles * 64, slot_of, K[order], 0, np.int32)
    t.tile_k = t.slot_K.reshape(n_tiles, 64).max(axis=1) if n_tiles else np.zeros(0, dtype=np.int32)
    t.tile_ptr = np.concatenate([[0], np.cumsum(t.tile_k.astype(np.int64))]).astype(np.int64)
    t.nobs = _per_slot(n_tiles * 64, slot_of, grp_ncells[order % ng], 0.0, np.float64)
    t.omq = _per_slot(n_tiles * 64, slot_of, 1.0 - grp_q[order % ng], 0.0, np.float64)
    return t


def _plan_records(K, rec_pairs):
    """Chains whose operands are 8-double records, one behind the other: (bins of each, first record of each + the total)."""
    rec_K = K[rec_pairs].astype(np.int64)
    return rec_K, np.concatenate([[0], np.cumsum(rec_K)]).astype(np.int64)


def _order_bins(bs, kernel, d_xcaps, big_cap, order, t, r):
    """Replay order of the chains ``order`` (K descending) of ``bs`` written to t.ops by ``kernel`` (table arguments ``d_xcaps``, uniforms ``r``): one
    wave up to ORDER_SMALL_CAP bins, 512 threads up to ``big_cap``, the host beyond.  Returns (device status word, the device operands to keep)."""
    K = bs.K[order]
    small, big, on_host = order[K <= ORDER_SMALL_CAP], order[(K > ORDER_SMALL_CAP) & (K <= big_cap)], order[K > big_cap]
    bs.order_path = {"small": len(small), "big": len(big), "host": len(on_host)}     # diagnostics (tests)
    d_pair_slot, t.d_tile_ptr = dev(t.pair_slot), dev(t.tile_ptr)
    status = zeros((1,), _torch().int32)
    d_r = [dev(np.asarray(x, dtype=np.float64)) for x in r]
    d_sf, d_nc = dev(bs.sf_table), dev(bs.blocks.grp_ncells.astype(np.float64))
    keep = [d_pair_slot, t.d_tile_ptr, d_sf, d_nc, *d_r]
    for lst, is_big in ((small, 0), (big, 1)):
        if len(lst):
            keep.append(dev(lst))
            _lib.call(kernel, P(bs.tab), P(bs.d_tab_ptr), *map(P, d_xcaps), P(bs.d_K), P(keep[-1]), len(lst), is_big, bs.ng, bs.n_bins,
                      P(d_sf), *map(P, d_r), P(d_pair_slot), P(t.d_tile_ptr), P(d_nc), *map(P, t.ops), P(status), _stream())
    for p in on_host:    # more bins than the in-LDS sort holds (very highly expressed genes)
        bs._order_on_host(int(p), *[float(x[p]) for x in r], int(t.pair_slot[p]), t.tile_ptr, t.ops)
    return status, keep


def _check_order_status(status, kernel):
    """The device status word of ``kernel`` (2 = more bins than the kernel holds, 4 = bins found != K, 8 = two equal codes) as exceptions."""
    st = int(status.item())
    if st & 6:
        raise RuntimeError(f"{kernel} inconsistency (status {st})")
    if st & 8:
        raise NotImplementedError("two bins of one pair collided in the replay hash (np.unique would merge them)")


class Bootstrap1D:
    """K5 -> K8 for a set of tested genes: histograms, bins, replay order, replay bootstrap, fill+log.

    After ``run`` the device holds ym/yv [n_pairs][B+1] (pair = gene_slot*n_groups + group; column 0 =
    log true mean / log true residual variance) ready for the contraction kernel.
    """

    def __init__(self, blocks, gene_idx, maxx, sf_bin_cells, sf_table, grp_q, num_boot):
        torch = _torch()
        self.blocks = blocks
        self.ng = blocks.n_groups
        self.gene_idx = np.asarray(gene_idx, dtype=np.int64)
        self.n_tested = len(self.gene_idx)
        self.n_pairs = self.n_tested * self.ng
        self.B = int(num_boot)
        self.ld = self.B + 1
        self.n_bins = int(len(sf_table))
        if self.n_bins > 256:
            raise ValueError("at most 256 size-factor bins are supported")
        self.sf_table = np.asarray(sf_table, dtype=np.float64)
        self.grp_q = np.asarray(grp_q, dtype=np.float64)
        s = _stream()
        b = blocks
        # per (group, sf_bin) cell counts (the zero-count bins come from these)
        bins_sorted = np.asarray(sf_bin_cells, dtype=np.uint8)[b.cell_order]
        grp_of_sorted = np.repeat(np.arange(self.ng), b.grp_ncells)
        self.grp_bin_cells = np.bincount(grp_of_sorted.astype(np.int64) * self.n_bins + bins_sorted, minlength=self.ng * self.n_bins) \
            .reshape(self.ng, self.n_bins).astype(np.uint32)
        d_bins = dev(bins_sorted)
        pairbase = np.full(b.G, -1, dtype=np.int32)
        pairbase[self.gene_idx] = (np.arange(self.n_tested) * self.ng).astype(np.int32)
        xcap = (np.asarray(maxx, dtype=np.int64)[:, self.gene_idx].T.reshape(-1) + 1).astype(np.int32)  # [pair]
        tab_ptr = np.concatenate([[0], np.cumsum(xcap.astype(np.int64) * self.n_bins)]).astype(np.int64)
        self.d_xcap, self.d_tab_ptr = dev(xcap), dev(tab_ptr[:-1])
        self.tab = zeros((max(1, int(tab_ptr[-1])),), torch.int32)
        d_pairbase = dev(pairbase)  # NB: every device operand must stay referenced until after the call
        for p, lo in zip(b.parts, b.part_lo):      # one launch per gene part, each with its slice of the map, all into the one table
            if (pairbase[lo:lo + p.G] >= 0).any():
                _lib.call("mm_hist1d_sell", P(p.ent), P(p.blk_base), P(p.slice_w), P(p.slice_ptr), P(p.item_ptr), P(p.perm),
                          P(p.d_blk_cell0), P(p.d_blk_group), P(d_bins), p.n_blocks, p.G, P(d_pairbase[lo:lo + p.G]), P(self.d_tab_ptr),
                          P(self.d_xcap), P(self.tab), s)
        self.d_K = empty((self.n_pairs,), torch.int32)
        d_gbc = dev(self.grp_bin_cells)
        _lib.call("mm_bins_count", P(self.tab), P(self.d_tab_ptr), P(self.d_xcap), self.n_pairs, self.ng, self.n_bins,
                  P(d_gbc), P(self.d_K), s)
        self.K = host(self.d_K)
        self.xcap, self.tab_ptr = xcap, tab_ptr

    def bins_of_pair(self, p):
        """Debug/test helper: the canonical (sf_bin, count, multiplicity) bins of pair p (host arrays)."""
        t0, xc = int(self.tab_ptr[p]), int(self.xcap[p])
        tab = host(self.tab[t0:t0 + self.n_bins * xc], np.uint32).reshape(self.n_bins, xc)
        bi, xi = np.nonzero(tab)
        return bi, xi, tab[bi, xi]

    def _order_on_host(self, p, r1, r0, slot, tile_ptr, ops):
        """Replay order + bootstrap operands of ONE pair computed on the host (same arithmetic as k_bins_order:
        code = count*r1 + r0*approx_sf ascending; pk = pix/remaining_p; log(1-p)) and written into its tile lane."""
        bi, xi, mu = self.bins_of_pair(p)
        code = xi.astype(np.float64) * r1 + r0 * self.sf_table[bi]
        o, pk, lq = _replay_order(code, mu, self.blocks.grp_ncells[p % self.ng])
        sf = self.sf_table[bi[o]]      # (records lie behind the operand planes in the one allocation, numbered from its start)
        _write_chain_operands(self._opsbuf, ops, slot, tile_ptr, (pk, lq, xi[o].astype(np.float64), 1.0 / sf, 1.0 / (sf * sf)))

    def weights_of(self, p):
        """Test helper (after run(dump_weights=True)): the int32 multinomial weights [K][B] of pair p, whichever kernel drew them."""
        K = int(self.K[p])
        if self.async_index[p] >= 0:
            return host(self.w_dump_async[int(self.async_slot[self.async_index[p]]), :K, :])
        if self.chain_index[p] >= 0:
            return host(self.w_dump_chain[int(self.chain_index[p]), :K, :])
        return host(self.w_dump[int(self.tile_slot[p]), :K, :])

    def alloc_outputs(self, true_mean_log, true_rv_log):
        """ym/yv [n_pairs][B+1] = NaN, column 0 = log true mean / log true residual variance (hypothesis_test.py:174)."""
        torch = _torch()
        self.ym = torch.full((self.n_pairs, self.ld), float("nan"), dtype=torch.float64, device="cuda")
        self.yv = torch.full((self.n_pairs, self.ld), float("nan"), dtype=torch.float64, device="cuda")
        self.ym[:, 0] = dev(np.asarray(true_mean_log, dtype=np.float64))
        self.yv[:, 0] = dev(np.asarray(true_rv_log, dtype=np.float64))

    def run(self, skip, r1, r0, mv_fit, fill_mode=0, fill_seed=0, dump_weights=False, pcg_seed=5, first_pair=0, target_waves=None,
            fast=False, mean_only=False, fill_keys=None, chain_keys=None):
        """Order bins, replay the bootstrap and fill/log for every pair >= ``first_pair`` that is not skipped.

        ``skip``[pair] bool; ``r1``/``r0``[pair] the two uniforms of bootstrap.py:62,65.  Rows below
        ``first_pair`` are left untouched (used by the strict replay driver).  ``fill_keys`` [pair] int64: keys of the device
        refill streams (fill_mode 0; default: the row number).  ``chain_keys`` [pair] int64 (``fast`` only; default: the row number):
        replicate r of pair p draws from the PCG64 stream derived from (``fill_seed``, ``chain_keys[p]``, r), so keys that number the
        (gene, group) chains independently of gene chunking and sharding make the result independent of both.  Returns n_invalid
        [n_pairs - first_pair][2] (host): invalid (mean, res_var) replicates per row, -1 = no valid one."""
        if chain_keys is not None and np.shape(chain_keys) != (self.n_pairs,):
            raise ValueError("chain_keys must have one key per pair")
        active = (~np.asarray(skip, dtype=bool)) & (self.K >= 2)
        active[:first_pair] = False
        c = self._choose_kernels(active, fast, target_waves)
        t = self._lay_out_operands(c, dump_weights)
        status, ordered = _order_bins(self, "mm_bins_order", (self.d_xcap,), ORDER_BIG_CAP, c.order_all, t, (r1, r0))
        launched = self._launch(c, t, fast, mean_only, fill_seed, pcg_seed, dump_weights, chain_keys)
        _check_order_status(status, "mm_bins_order")      # (reads the word: after the launches are enqueued)
        del ordered, launched      # NB: every device operand must stay referenced until after the call that reads it
        self.raw_mean = self.ym.clone() if dump_weights else None
        self.raw_var = self.yv.clone() if dump_weights else None
        n_inv = self._fill_log(mv_fit, fill_mode, fill_seed, first_pair, fill_keys)
        self.active = active
        return n_inv

    def _choose_kernels(self, active, fast, target_waves):
        """Which kernel runs which chain: the longest ones one per wave (mm_boot1d_chain), the others one per lane of a tile
        (mm_boot1d_replay / _free / _fast) or of an async wave (mm_boot1d_async); then the tiles' packing and dispatch order, and
        the chains the packer left alone in their tile (they run as chains inside the tile launch)."""
        act = np.flatnonzero(active)
        c = SimpleNamespace()
        order_all = c.order_all = act[np.argsort(-self.K[act], kind="stable")]
        n_chain = 0 if (fast or not CHAIN_MIN_K) else int(np.searchsorted(-self.K[order_all], -CHAIN_MIN_K, side="right"))
        if not fast and target_waves is None and 0 < len(order_all) <= CHAIN_ALL_MAX:
            n_chain = len(order_all)
        c.use_async = TILE_MODE == "async" and not fast and target_waves is None
        if c.use_async and ASYNC_CHAIN_MIN_K:
            n_chain = max(n_chain, int(np.searchsorted(-self.K[order_all], -ASYNC_CHAIN_MIN_K, side="right")))
        chain_pairs, order = order_all[:n_chain], order_all[n_chain:]
        c.async_pairs = order if c.use_async else order[:0]       # K descending: the 64 chains of a wave have similar lengths
        if c.use_async:
            order = order[:0]
        # replay: cost-model lane packing (one lane = one sequential chain); fast: dense 64-wide tiles (one WAVE per pair)
        slot_of, n_tiles = pack_lanes(self.K[order], PACK_WAVES if target_waves is None else target_waves, dense=fast)
        if not fast:
            slot_of = pair_tiles(slot_of, n_tiles, self.K[order])
        c.n_launch = n_chain                  # chains of the separate mm_boot1d_chain launch (CHAIN_MIN_K / ASYNC_CHAIN_MIN_K rules)
        c.tile_chain = None
        if CHAIN_LONE and not fast and n_tiles:
            # A chain the packer left alone in its tile takes a whole wave either way: that wave runs it in the wave-uniform
            # form (chain_body inside the tile kernel), at the tile's place in the dispatch order -- the packing and pairing
            # above stay what they are, the lone waves just step faster.
            tile = slot_of // 64
            lone = np.bincount(tile, minlength=n_tiles)[tile] == 1
            if lone.any():
                c.tile_chain = np.full(n_tiles, -1, dtype=np.int32)
                c.tile_chain[tile[lone]] = n_chain + np.arange(int(lone.sum()))
                chain_pairs = np.concatenate([chain_pairs, order[lone]])
                order, slot_of = order[~lone], slot_of[~lone]
        c.chain_pairs, c.order, c.slot_of, c.n_tiles = chain_pairs, order, slot_of, n_tiles
        c.use_free = TILE_FREE and not fast and not c.use_async and n_tiles > 0 and len(order) > 0
        self.n_tiles, self.n_chain, self.n_async, self.n_chain_launch = n_tiles, len(chain_pairs), len(c.async_pairs), c.n_launch
        self.chain_pairs, self.async_pairs = chain_pairs, c.async_pairs
        self.draws_per_replicate = int(np.maximum(self.K[order_all] - 1, 0).sum())
        return c

    def _lay_out_operands(self, c, dump_weights):
        """Slot tables of the tile launch and ONE operand allocation: five [rows][64] planes of the tiles, then the 8-double
        records of every chain that reads records (chain kernel, async kernel, free-running tiles)."""
        torch = _torch()
        n_chain, n_async, n_tiles = self.n_chain, self.n_async, c.n_tiles
        t = _plan_tiles(self.K, c.order, c.slot_of, n_tiles, self.n_pairs, self.blocks.grp_ncells, self.grp_q, self.ng)
        t.plane = 64 if c.use_free else max(1, int(t.tile_ptr[-1])) * 64       # free-running tiles have no operand rows
        rec_pairs = np.concatenate([c.chain_pairs, c.async_pairs, c.order if c.use_free else c.order[:0]])
        t.rec_K, t.rec_base = _plan_records(self.K, rec_pairs)
        self._opsbuf = empty((5 * t.plane + 8 * max(1, int(t.rec_base[-1])),), torch.float64)
        t.ops = [self._opsbuf[i * t.plane:(i + 1) * t.plane] for i in range(5)]
        t.d_recs = c_void_p(self._opsbuf.data_ptr() + 5 * t.plane * 8)
        self.tile_slot = t.pair_slot.copy()                                 # (tile, lane) slot of the chains that run as lanes of a tile
        t.pair_slot[rec_pairs] = CHAIN_SLOT | (5 * t.plane // 8 + t.rec_base[:-1])
        self.chain_index = np.full(self.n_pairs, -1, dtype=np.int64)
        self.chain_index[c.chain_pairs] = np.arange(n_chain)
        self.async_index = np.full(self.n_pairs, -1, dtype=np.int64)
        self.async_index[c.async_pairs] = np.arange(n_async)
        t.slot_rec = _per_slot(n_tiles * 64, c.slot_of, t.rec_base[n_chain + n_async:-1], -1, np.int64) if c.use_free else None
        self.kmax_dump = int(t.tile_k.max()) if (dump_weights and n_tiles) else 0
        self.slot_pair, self.slot_K, self.pair_slot, self.tile_ptr = t.slot_pair, t.slot_K, t.pair_slot, t.tile_ptr
        self._ops, self._nobs = t.ops, t.nobs      # kept for diagnostics (tools/replay_balance.py)
        return t

    def _launch(self, c, t, fast, mean_only, fill_seed, pcg_seed, dump_weights, chain_keys=None):
        """The chain kernel on the side stream, beside it on the launch stream the async and the tile kernel.  Returns their device operands."""
        torch, s = _torch(), _stream()
        ng, B, ld = self.ng, self.B, self.ld
        n_chain, n_async, n_tiles, n_launch, kmax_dump = self.n_chain, self.n_async, c.n_tiles, c.n_launch, self.kmax_dump
        self._fast = None
        chain_pairs, async_pairs = c.chain_pairs, c.async_pairs
        self.w_dump = zeros((n_tiles * 64, kmax_dump, B), torch.int32) if dump_weights else None
        d_slot_K, d_nobs, d_omq, d_slot_pair = dev(t.slot_K), dev(t.nobs), dev(t.omq), dev(t.slot_pair)
        keep = [d_slot_K, d_nobs, d_omq, d_slot_pair]
        self.w_dump_chain = None
        chain_tiles = None
        if n_chain:
            ch_K = t.rec_K[:n_chain]
            kd = int(ch_K.max()) if dump_weights else 0
            self.w_dump_chain = zeros((n_chain, kd, B), torch.int32) if dump_weights else None
            d_chb, d_chK = dev(t.rec_base[:n_chain]), dev(ch_K.astype(np.int32))
            d_chn, d_cho = dev(self.blocks.grp_ncells[chain_pairs % ng].astype(np.float64)), dev(1.0 - self.grp_q[chain_pairs % ng])
            d_chr = dev(chain_pairs.astype(np.int64))
            keep += [d_chb, d_chK, d_chn, d_cho, d_chr]
            if c.tile_chain is not None:        # chains that run as waves of the tile kernel's own launch
                d_tc = dev(c.tile_chain)
                chain_tiles = _lib.ChainTiles(P(d_tc), t.d_recs, P(d_chb), P(d_chK), P(d_chn), P(d_cho), P(d_chr), P(pcg64_jump_table(pcg_seed)),
                                              P(self.w_dump_chain), kd)
                keep += [d_tc, chain_tiles]
        if n_launch:
            # the chain kernel goes out first, on its own stream, and runs beside the tile kernel; the launch stream waits for
            # it before the fill / log pass
            side, main = side_stream(), torch.cuda.current_stream()
            side.wait_stream(main)
            _lib.call("mm_boot1d_chain", t.d_recs, P(d_chb), P(d_chK), P(d_chn), P(d_cho), P(d_chr),
                      n_launch, P(pcg64_jump_table(pcg_seed)), pcg64_state(pcg_seed), B, int(mean_only), ld, P(self.ym), P(self.yv),
                      P(self.w_dump_chain), kd, c_void_p(side.cuda_stream))
        self.w_dump_async = None
        if n_async:
            rec_K, rec_base = t.rec_K[n_chain:n_chain + n_async], t.rec_base[n_chain:n_chain + n_async]
            ka = int(rec_K.max()) if dump_weights else 0
            # slot = 64 * wave + lane; a wave takes ASYNC_LANES consecutive chains of the K-descending list, its other lanes idle
            L = max(1, min(64, int(ASYNC_LANES)))
            idx = np.arange(n_async)
            a_slot = (idx // L) * 64 + idx % L
            n_slots = int(a_slot[-1]) + 1
            self.async_slot = a_slot
            self.w_dump_async = zeros((n_slots, ka, B), torch.int32) if dump_weights else None
            d_ab, d_aK, d_an, d_ao, d_ar = [dev(_per_slot(n_slots, a_slot, vals, 0, dtype)) for vals, dtype in (
                (rec_base, np.int64), (rec_K, np.int32), (self.blocks.grp_ncells[async_pairs % ng], np.float64),
                (1.0 - self.grp_q[async_pairs % ng], np.float64), (async_pairs, np.int64))]
            keep += [d_ab, d_aK, d_an, d_ao, d_ar]
            _lib.call("mm_boot1d_async", t.d_recs, P(d_ab), P(d_aK), P(d_an), P(d_ao), P(d_ar), n_slots,
                      pcg64_state(pcg_seed), B, int(mean_only), ld, P(self.ym), P(self.yv), P(self.w_dump_async), ka, s)
        chains = ctypes.byref(chain_tiles) if chain_tiles is not None else None
        if n_tiles and fast:
            keys = np.arange(self.n_pairs, dtype=np.int64) if chain_keys is None else np.asarray(chain_keys, dtype=np.int64)
            d_slot_key = dev(_per_slot(n_tiles * 64, c.slot_of, keys[c.order], 0, np.int64))
            keep.append(d_slot_key)
            _lib.call("mm_boot1d_fast", *[P(o) for o in t.ops], P(t.d_tile_ptr), n_tiles * 64, P(d_slot_K), P(d_nobs), P(d_omq), P(d_slot_pair),
                      P(d_slot_key), int(fill_seed) & ((1 << 64) - 1), B, int(mean_only), ld, P(self.ym), P(self.yv), P(self.w_dump),
                      kmax_dump, s)
            # what a later launch on a replicate range reads (run_range): the operand planes live in self._opsbuf
            self._fast = SimpleNamespace(ops=t.ops, d_tile_ptr=t.d_tile_ptr, n_slots=n_tiles * 64, d_slot_K=d_slot_K, d_nobs=d_nobs, d_omq=d_omq,
                                         pair_slot=self.tile_slot, d_slot_key=d_slot_key, kmax=int(t.tile_k.max()),
                                         seed=int(fill_seed) & ((1 << 64) - 1))
        elif n_tiles and c.use_free:
            d_slot_rec = dev(t.slot_rec)
            keep.append(d_slot_rec)
            _lib.call("mm_boot1d_free", t.d_recs, P(d_slot_rec), n_tiles, P(d_slot_K), P(d_nobs), P(d_omq),
                      P(d_slot_pair), pcg64_state(pcg_seed), B, int(mean_only), ld, P(self.ym), P(self.yv), P(self.w_dump), kmax_dump, chains, s)
        elif n_tiles:
            _lib.call("mm_boot1d_replay", *[P(o) for o in t.ops], P(t.d_tile_ptr), n_tiles, P(d_slot_K), P(d_nobs), P(d_omq), P(d_slot_pair),
                      pcg64_state(pcg_seed), B, int(mean_only), ld, P(self.ym), P(self.yv), P(self.w_dump), kmax_dump, n_launch, chains, s)
        if n_launch:
            torch.cuda.current_stream().wait_stream(side)
        return keep

    def launch_range(self, rep_lo, rep_n, open_pairs, planes, row_of_pair, mean_only=False, dump_weights=False):
        """After ``run(fast=True)``: the replicates [rep_lo, rep_lo + rep_n) of the chains ``open_pairs`` (mm_boot1d_fast_range on the
        kept operand planes, tile layout and stream keys; every other slot gets row -1 and writes nothing), raw -- before fill / log
        -- into columns 1..rep_n of the rows ``row_of_pair`` of the caller's ``planes`` = (mean, var), fp64 device tensors
        [rows][ld >= 1 + rep_n]; nothing else of them is written.  Chains of ``open_pairs`` that did not run (skipped, K < 2) are
        left out.  Replicate rep_lo + i of a chain is bit for bit the one a one-shot ``run`` over more replicates stores in column
        1 + rep_lo + i.  ``dump_weights``: keep the int32 weights in ``self.w_dump_range`` [slot][k][i] (slot =
        ``self.tile_slot[pair]``)."""
        torch, f = _torch(), getattr(self, "_fast", None)
        if f is None:
            raise RuntimeError("launch_range needs a preceding run(fast=True): the replay kernels keep no per-replicate streams")
        rep_lo, rep_n = int(rep_lo), int(rep_n)
        if rep_lo < 0 or rep_n < 1 or rep_lo + rep_n > 2 ** 31 - 1:
            raise ValueError("launch_range: need rep_lo >= 0, rep_n >= 1 and rep_lo + rep_n <= 2^31 - 1")
        pm, pv = planes
        for x in (pm, pv):
            if x.dtype != torch.float64 or not x.is_cuda or not x.is_contiguous() or x.dim() != 2 or x.shape != pm.shape or x.shape[1] < rep_n + 1:
                raise ValueError("launch_range: planes must be two contiguous fp64 device tensors [rows][>= 1 + rep_n]")
        open_pairs, row_of_pair = np.asarray(open_pairs, dtype=np.int64).reshape(-1), np.asarray(row_of_pair, dtype=np.int64).reshape(-1)
        if len(open_pairs) != len(row_of_pair) or (len(open_pairs) and (open_pairs.min() < 0 or open_pairs.max() >= self.n_pairs)):
            raise ValueError("launch_range: open_pairs / row_of_pair do not match the chains")
        if len(row_of_pair) and (row_of_pair.min() < 0 or row_of_pair.max() >= pm.shape[0]):
            raise ValueError("launch_range: row out of range")       # (the kernel trusts the rows)
        slot = f.pair_slot[open_pairs]
        slot_row = np.full(f.n_slots, -1, dtype=np.int64)
        slot_row[slot[slot >= 0]] = row_of_pair[slot >= 0]
        d_slot_row = dev(slot_row)
        self.w_dump_range = zeros((f.n_slots, f.kmax, rep_n), torch.int32) if dump_weights else None
        _lib.call("mm_boot1d_fast_range", *[P(o) for o in f.ops], P(f.d_tile_ptr), f.n_slots, P(f.d_slot_K), P(f.d_nobs), P(f.d_omq),
                  P(d_slot_row), P(f.d_slot_key), f.seed, rep_lo, rep_n, int(mean_only), pm.shape[1], P(pm), P(pv),
                  P(self.w_dump_range), f.kmax if dump_weights else 0, _stream())
        return d_slot_row      # NB: stays referenced until the caller's next call on the stream

    def run_range(self, rep_lo, rep_n, open_pairs, planes, row_of_pair, mv_fit, fill_seed, fill_keys, mean_only=False):
        """``launch_range``, then mm_boot_fill_log over ALL rows of ``planes`` with refill seed ``fill_seed`` and the refill keys
        ``fill_keys`` [row] (the chains' keys of the first run): an invalid replicate of the range is refilled from the valid
        replicates of the SAME range.  Raises after a replay-mode ``run``.  Returns n_invalid [rows][2] (host), -1 = no valid
        replicate (every row no chain wrote)."""
        torch = _torch()
        keep = self.launch_range(rep_lo, rep_n, open_pairs, planes, row_of_pair, mean_only)
        pm, pv = planes
        n_rows = pm.shape[0]
        if len(np.shape(fill_keys)) != 1 or len(fill_keys) != n_rows:
            raise ValueError("run_range: fill_keys must have one key per row")
        n_inv = empty((max(1, n_rows), 2), torch.int32)
        fit = (ctypes.c_double * 3)(*[float(x) for x in mv_fit])
        if n_rows > 0:
            d_keys = dev(np.asarray(fill_keys, dtype=np.int64))
            _lib.call("mm_boot_fill_log", P(pm), P(pv), n_rows, pm.shape[1], int(rep_n), fit, 0, int(fill_seed) & ((1 << 64) - 1), P(n_inv),
                      P(d_keys), _stream())
        out = host(n_inv)[:n_rows]
        del keep
        return out

    def _fill_log(self, mv_fit, fill_mode, fill_seed, first_pair, fill_keys):
        """mm_boot_fill_log on the rows >= first_pair; returns n_invalid [rows][2] (host)."""
        torch, ld = _torch(), self.ld
        n_rows = self.n_pairs - first_pair
        n_inv = empty((max(1, n_rows), 2), torch.int32)
        fit = (ctypes.c_double * 3)(*[float(x) for x in mv_fit])
        if n_rows > 0:
            d_keys = dev(np.asarray(fill_keys, dtype=np.int64)[first_pair:]) if fill_keys is not None else None
            _lib.call("mm_boot_fill_log", c_void_p(self.ym.data_ptr() + first_pair * ld * 8), c_void_p(self.yv.data_ptr() + first_pair * ld * 8),
                      n_rows, ld, self.B, fit, int(fill_mode), int(fill_seed) & ((1 << 64) - 1), P(n_inv), P(d_keys), _stream())
        return host(n_inv)[:n_rows]

    def contract(self, test_gene, W, good, which):
        """K9+K10 for tests (gene slot, weight row).  Returns (coef device tensor [n_tests][ld], stats host [n_tests][8])."""
        torch = _torch()
        n_tests = len(test_gene)
        coef = empty((max(1, n_tests), self.ld), torch.float64)
        stats = empty((max(1, n_tests), 8), torch.float64)
        d_tg, d_W, d_good = dev(np.asarray(test_gene, dtype=np.int32)), dev(np.asarray(W, dtype=np.float64)), dev(np.asarray(good, dtype=np.uint8))
        _lib.call("mm_contract_stats", P(self.ym), P(self.yv), self.ld, self.B, self.ng, P(d_tg), P(d_W), P(d_good), n_tests,
                  int(which), P(coef), P(stats), _stream())
        return coef, host(stats)[:n_tests]

    def contrast(self, test_gene, test_grp, ctrl, good):
        """Two-group contrasts against the control group ``ctrl`` (``_contrast``: the designs {(group, +1), (ctrl, -1)} through
        ``contrast_design``): returns (stats_mean, stats_var) host arrays [n_tests][8], the NaN record where ``good`` [gene][group]
        lacks the test's group or the control; ``rows(which, idx)`` gives the coefficient rows of selected tests on demand: a host
        array, or with ``to_host=False`` a device tensor [len(idx)][ld] (a view of the scratch tensor ``out`` when one is passed)."""
        (st_m, st_v), rows = _contrast([self.ym, self.yv], self.ld, self.B, self.ng, self.n_tested, test_gene, test_grp, ctrl, good)
        return st_m, st_v, rows

    def contrast_design(self, test_gene, test_design, design_ptr, design_grp, design_w):
        """Guide-vs-control contrasts with covariates (mm_contrast_design_stats): test t applies the sparse weight row
        ``design_grp/design_w[design_ptr[d]:design_ptr[d + 1]]``, d = ``test_design[t]``, to the replicate rows of gene
        ``test_gene[t]``.  Returns (stats_mean, stats_var) host arrays [n_tests][8] and ``rows(which, idx)``, as ``contrast``."""
        (st_m, st_v), rows = _contrast_design([self.ym, self.yv], self.ld, self.B, self.ng, self.n_tested, test_gene, test_design, design_ptr,
                                              design_grp, design_w)
        return st_m, st_v, rows

    def family_maxt(self, family_ptr, test_gene, test_design, design_ptr, design_grp, design_w, scale, stage_cap=None):
        """Single-step max-T adjustment over families of design contrasts (mm_family_maxt): the tests
        ``family_ptr[f]:family_ptr[f + 1]`` -- consecutive, on one gene -- are family f, with the tables of ``contrast_design``, and
        ``scale`` [test][2] holds 1 / se of every member on the mean and the variability plane, 0 for a member without a test
        (``family_scale`` of its records).  ``stage_cap``: how many members of a family keep their (coef0, scale) in LDS (default:
        the largest family, at most ``FAMILY_MAX_STAGED``); no number depends on it.  Returns ``maxrow`` (device [n_fam][2][ld]:
        the maximum row of every family and plane, NaN in column 0 and the columns that are not family-valid), ``adj`` (host
        [n_tests][2][2]: t0, n_adj) and ``fam`` (host [n_fam][2][2]: n_valid_family, n_included)."""
        return _family_maxt([self.ym, self.yv], self.ld, self.B, self.ng, self.n_tested, family_ptr, test_gene, test_design, design_ptr,
                            design_grp, design_w, scale, stage_cap)

    def joint(self, test_gene, tables):
        """Joint tests of a treatment block (mm_joint_stats): test t applies the linear forms of design ``tables.test_design[t]``
        (``memento._ht.joint_tables``: ``design_ptr``, ``design_rank``, ``design_lofs``, ``design_grp``, ``design_L``) to the
        replicate rows of gene ``test_gene[t]``.  Returns (stats_mean, stats_var) host arrays [n_tests][8], the joint record of
        include/memento_hip.h."""
        return tuple(_joint([self.ym, self.yv], self.ld, self.B, self.ng, self.n_tested, test_gene, tables))

    def valid_cols(self, good):
        """hypothesis_test.py:249-251 on the device: (col_map device tensor [n_tested][B+1], n_valid host [n_tested]) --
        the replicate columns in which every good group is finite in both the mean and the variability rows."""
        return _valid_cols(self.ym, self.yv, self.ld, self.B, self.ng, good, self.n_tested)

    def contract_resampled(self, test_gene, tt, good, which, gene_mask, M, Nc, rep=None, bcol=None, seed=0, col_map=None, n_valid=None):
        """resample_rep=True: residualise the response rows (into a scratch copy), then the resampled weighted slopes + null
        statistics.  ``rep``/``bcol`` [n_genes][n_groups][B] (int16/int32) replay np.random.choice; None -> drawn on the
        device.  ``col_map``/``n_valid`` (from ``valid_cols``): surviving replicate columns, None = all of them."""
        return _contract_resampled(self.yv if which else self.ym, self.ld, self.B, self.ng, self.n_tested, test_gene, tt, good, gene_mask,
                                   M, Nc, rep, bcol, seed, col_map, n_valid)

    def cross_resampled_block(self, gene_ptr, tt, good, gene_mask, M, Nc, rep=None, bcol=None, seed=0, col_map=None, n_valid=None,
                              gene_key=None, zt=None, beta_scratch_bytes=None):
        """resample_rep=True for tests that arrive gene-major (mm_cross_resampled_block): the tests of gene slot g are the rows
        ``gene_ptr[g]:gene_ptr[g + 1]`` of ``tt`` [n_tests][n_groups]; everything else as ``contract_resampled``, and ``gene_key``
        [n_genes] keys the device draws of a gene (None: its slot).  Each plane is residualised into ONE plane-sized scratch in
        turn; no coefficient row is stored.  Returns (stats_mean, stats_var) host arrays [n_tests][8] -- the records
        ``contract_resampled`` gives for the same tests -- and ``rows(which, idx, to_host=True, out=None)``, the contract of
        ``contrast_design``'s closure: the coefficient rows of the tests ``idx`` on plane ``which``, from the per-test kernel on
        that subset with the same draws (mm_cross_resampled_keyed).  The closure holds the scratch.

        ``zt`` [n_tests][n_groups] (finite; checked here, the kernel trusts it): a covariate PER TEST, residualised by ``M`` like the
        response -- test t then reads ``y - zt[t] * beta`` with beta the weighted slope of the residualised response on ``zt[t]``
        (mm_cross_resampled_block_cov; a zero row leaves the response as it is).  The tiles go through a beta scratch of at most
        ``beta_scratch_bytes`` (default ``CROSS_COV_SCRATCH_BYTES``; never less than one tile: 64 x ld bytes) a batch at a time,
        and no number depends on the batches; ``rows`` materialises the response of the listed tests (mm_residualize_rank1) into a
        scratch of the same bound and runs the per-test kernel on the copies: the block kernel's coefficients bit for bit."""
        (st_m, st_v), rows, _ = _cross_resampled_block([self.ym, self.yv], self.ld, self.B, self.ng, self.n_tested, gene_ptr, tt, good,
                                                       gene_mask, M, Nc, rep, bcol, seed, col_map, n_valid, gene_key, zt, beta_scratch_bytes)
        return st_m, st_v, rows

    def cross_resampled_family(self, gene_ptr, tt, good, gene_mask, M, Nc, rep=None, bcol=None, seed=0, col_map=None, n_valid=None,
                               gene_key=None, zt=None):
        """``cross_resampled_block`` with the single-step max-T over every gene's tests (mm_cross_resampled_family): the same call,
        the same records and ``rows``, and a third closure ``family(scale, slab=None)`` on the uploaded tables and the one residual
        scratch.  ``scale`` [n_tests][2] holds 1 / se of every test on the mean and the variability plane, 0 for a member without
        a test (``family_scale(st_m, st_v)``).  It returns ``maxrow`` (a device tensor [n_genes][ld] per plane: the maximum row of
        every gene, NaN in slot 0, the slots that are not family-valid and the slots from nb on), ``adj`` (host [n_tests][2][2]:
        t0, n_adj) and ``fam`` (host [n_genes][2][2]: n_valid_family, n_included), the layout of ``family_maxt``; beyond ``maxrow``
        it allocates nothing plane-sized, and the plane the scratch already holds is taken first.  ``slab``: the slots a
        workgroup takes (default: the kernel's); no number depends on it.  A covariate per test (``zt``) is not offered: the
        family kernel walks all tiles of a gene per slot and would need the beta rows of the whole gene at once."""
        if zt is not None:
            raise NotImplementedError("cross_resampled_family with a covariate per test (zt)")
        (st_m, st_v), rows, family = _cross_resampled_block([self.ym, self.yv], self.ld, self.B, self.ng, self.n_tested, gene_ptr, tt, good,
                                                            gene_mask, M, Nc, rep, bcol, seed, col_map, n_valid, gene_key)
        return st_m, st_v, rows, family


def _rows_out(out, n, ld):
    """Where a ``rows`` closure writes ``n`` coefficient rows: a fresh tensor, or the caller's scratch ``out`` [>= n][ld] (fp64,
    contiguous), reused from call to call."""
    torch = _torch()
    if out is None:
        return empty((max(1, n), ld), torch.float64)
    if out.dtype != torch.float64 or out.dim() != 2 or out.shape[1] != ld or out.shape[0] < max(1, n) or not out.is_contiguous():
        raise ValueError(f"rows: out must be a contiguous fp64 tensor [>= {max(1, n)}][{ld}]")
    return out


def row_quantiles(rows, ld, num_boot, probs):
    """np.nanquantile(row[1:num_boot + 1], probs) of every row of an [n_rows][ld] fp64 device tensor (mm_row_quantiles: an exact
    radix select per row; column 0 and the padding are not read).  Returns (q device tensor [n_rows][n_probs], n_valid host
    [n_rows] = the non-NaN columns of every row)."""
    torch = _torch()
    probs = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    if rows.dtype != torch.float64 or not rows.is_cuda or not rows.is_contiguous() or rows.numel() % ld:
        raise ValueError("row_quantiles: rows must be a contiguous fp64 device tensor of [n_rows][ld]")
    n_rows = rows.numel() // ld
    q = empty((max(1, n_rows), max(1, len(probs))), torch.float64)
    n_valid = empty((max(1, n_rows),), torch.int32)
    _lib.call("mm_row_quantiles", P(rows), n_rows, int(ld), int(num_boot), probs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(probs),
              P(q), P(n_valid), _stream())
    return q[:n_rows], host(n_valid)[:n_rows]


def _up(a):
    return dev(a if len(a) else np.zeros(1, a.dtype))


def _csr_tables(what, test_row, test_design, design_ptr, design_grp, n_rows, ng):
    """What the design and the joint tables share, coerced to int32 host arrays and checked (the kernels trust these indices):
    test t applies design ``test_design[t]`` -- the groups ``design_grp[design_ptr[d]:design_ptr[d + 1]]`` among the ``ng`` -- to row
    block ``test_row[t]`` < ``n_rows`` (a gene slot or a pair).  ``what`` names the caller in the messages."""
    test_row, test_design, design_ptr, design_grp = (np.asarray(a, dtype=np.int32) for a in (test_row, test_design, design_ptr, design_grp))
    n_tests, n_designs = len(test_row), len(design_ptr) - 1
    if len(test_design) != n_tests or n_designs < 0:
        raise ValueError(f"{what}: inconsistent table sizes")
    if design_ptr[0] != 0 or design_ptr[-1] != len(design_grp) or (np.diff(design_ptr) < 0).any():
        raise ValueError(f"{what}: design_ptr is not a CSR pointer over design_grp")
    if len(design_grp) and (design_grp.min() < 0 or design_grp.max() >= ng):
        raise ValueError(f"{what}: group index out of range")
    if n_tests and (test_row.min() < 0 or test_row.max() >= n_rows or test_design.min() < 0 or test_design.max() >= n_designs):
        raise ValueError(f"{what}: test index out of range")
    return test_row, test_design, design_ptr, design_grp


def _design_tables(test_row, test_design, design_ptr, design_grp, design_w, n_rows, ng, what="contrast_design", check=None):
    """The tables of the design-contrast kernels (``contrast_design`` of Bootstrap1D / Bootstrap2D): the CSR rows of
    ``_csr_tables`` with one weight ``design_w`` per listed group, checked and uploaded, empty arrays padded to one element.
    Returns test_row and test_design as int32 host arrays and the device tensors (test_row, test_design, design_ptr, design_grp,
    design_w), the order in which the kernels take them.  ``what`` names the caller in the messages; ``check(test_row)`` holds a
    caller's further checks, which also run before anything is uploaded."""
    design_w = np.asarray(design_w, dtype=np.float64)
    if len(design_w) != len(np.asarray(design_grp)):
        raise ValueError(f"{what}: inconsistent table sizes")
    test_row, test_design, design_ptr, design_grp = _csr_tables(what, test_row, test_design, design_ptr, design_grp, n_rows, ng)
    if check is not None:
        check(test_row)
    return test_row, test_design, (_up(test_row), _up(test_design), dev(design_ptr), _up(design_grp), _up(design_w))


FAMILY_MAX_STAGED = 1024      # members of a family whose (coef0, scale) mm_family_maxt can keep in LDS (contract.hip: FM_MAX_STAGED)


def family_scale(*stats):
    """``scale`` [test][plane] of ``family_maxt`` from the records of ``contrast_design``, one record array per plane (st_m, st_v of
    Bootstrap1D: [test][2]; the one of Bootstrap2D: [test][1]): 1 / se where the record is a test (finite coef0, finite se > 0,
    n_valid >= 1, not all_equal), else 0."""
    out = np.zeros((len(stats[0]), len(stats)))
    for k, st in enumerate(stats):
        st = np.asarray(st, dtype=np.float64).reshape(-1, 8)
        with np.errstate(invalid="ignore", divide="ignore"):
            live = np.isfinite(st[:, 0]) & np.isfinite(st[:, 1]) & (st[:, 1] > 0) & (st[:, 2] >= 1) & (st[:, 5] == 0)
            out[:, k] = np.where(live, 1.0 / st[:, 1], 0.0)
    return out


def _family_tables(family_ptr, test_row, test_design, design_ptr, design_grp, design_w, scale, n_rows, ng, n_planes=2):
    """The tables of mm_family_maxt / mm_family_maxt1, checked (the kernel trusts them) and uploaded: those of ``_design_tables``,
    ``family_ptr`` a CSR pointer over the tests whose families each sit on one row block, and one ``scale`` per test and plane.
    Returns family_ptr (int32) and scale (fp64 [n_tests][n_planes]) as host arrays and the device tensors of ``_design_tables``."""
    family_ptr = np.asarray(family_ptr, dtype=np.int64).reshape(-1)
    scale = np.asarray(scale, dtype=np.float64)

    def check(test_row):
        n_tests = len(test_row)
        if len(family_ptr) < 1 or family_ptr[0] != 0 or family_ptr[-1] != n_tests or (np.diff(family_ptr) < 0).any():
            raise ValueError("family_maxt: family_ptr is not a CSR pointer over the tests")
        fam_of = np.repeat(np.arange(len(family_ptr) - 1), np.diff(family_ptr))
        if n_tests and (test_row != test_row[family_ptr[fam_of]]).any():
            raise ValueError("family_maxt: the tests of a family must share one test_row")
        if scale.shape != (n_tests, n_planes):
            raise ValueError(f"family_maxt: scale must be [n_tests][{n_planes}]")

    _, _, d_tab = _design_tables(test_row, test_design, design_ptr, design_grp, design_w, n_rows, ng, what="family_maxt", check=check)
    return family_ptr.astype(np.int32), scale, d_tab


def _family_maxt(planes, ld, B, ng, n_rows, family_ptr, test_row, test_design, design_ptr, design_grp, design_w, scale, stage_cap=None):
    """``family_maxt`` of Bootstrap1D (``planes`` = [ym, yv]: mm_family_maxt) and Bootstrap2D ([yc]: mm_family_maxt1).  Returns
    ``maxrow`` (device [n_fam][n_planes][ld]), ``adj`` (host [n_tests][n_planes][2]) and ``fam`` (host [n_fam][n_planes][2])."""
    torch = _torch()
    n_planes = len(planes)
    family_ptr, scale, d_tab = _family_tables(family_ptr, test_row, test_design, design_ptr, design_grp, design_w, scale, n_rows, ng, n_planes)
    n_fam, n_tests = len(family_ptr) - 1, len(scale)
    if stage_cap is None:
        stage_cap = min(FAMILY_MAX_STAGED, int(np.diff(family_ptr).max()) if n_fam else 0)
    if not 0 <= int(stage_cap) <= FAMILY_MAX_STAGED:
        raise ValueError(f"family_maxt: stage_cap must lie in [0, {FAMILY_MAX_STAGED}]")
    maxrow = empty((max(1, n_fam), n_planes, ld), torch.float64)
    adj = empty((max(1, n_tests), n_planes, 2), torch.float64)
    fam = empty((max(1, n_fam), n_planes, 2), torch.float64)
    d_fp, d_scale = dev(family_ptr), _up(scale.reshape(-1))
    _lib.call("mm_family_maxt1" if n_planes == 1 else "mm_family_maxt", *map(P, planes), ld, B, ng, P(d_fp), *map(P, d_tab), P(d_scale),
              int(stage_cap), n_fam, P(maxrow), P(adj), P(fam), _stream())
    return maxrow[:n_fam], host(adj)[:n_tests], host(fam)[:n_fam]


def _contrast_design(planes, ld, B, ng, n_rows, test_row, test_design, design_ptr, design_grp, design_w, rows_design=None):
    """``contrast_design`` of Bootstrap1D (``planes`` = [ym, yv]: mm_contrast_design_stats / _rows) and Bootstrap2D ([yc]:
    mm_contrast_design1_stats / _rows).  Returns the records, one host array [n_tests][8] per plane, and
    ``rows(which, idx, to_host=True, out=None)``: the coefficient rows of the tests ``idx`` on plane ``which``, under the designs
    ``rows_design`` (checked by the caller) where given, not ``test_design``."""
    torch = _torch()
    one = "1" if len(planes) == 1 else ""
    test_row, test_design, d_tab = _design_tables(test_row, test_design, design_ptr, design_grp, design_w, n_rows, ng)
    if rows_design is None:
        rows_design = test_design
    n_tests = len(test_row)
    stats = [empty((max(1, n_tests), 8), torch.float64) for _ in planes]
    _lib.call(f"mm_contrast_design{one}_stats", *map(P, planes), ld, B, ng, *map(P, d_tab), n_tests, *map(P, stats), _stream())

    def rows(which, idx, to_host=True, out=None):
        idx = np.asarray(idx, dtype=np.int64)
        out = _rows_out(out, len(idx), ld)
        a, b = dev(test_row[idx]), dev(rows_design[idx])
        _lib.call(f"mm_contrast_design{one}_rows", *map(P, planes), ld, B, ng, P(a), P(b), *map(P, d_tab[2:]), len(idx),
                  *([] if one else [int(which)]), P(out), _stream())
        return host(out)[: len(idx)] if to_host else out[: len(idx)]

    return [host(s)[:n_tests] for s in stats], rows


def _contrast(planes, ld, B, ng, n_rows, test_row, test_grp, ctrl, good):
    """``contrast`` of Bootstrap1D / Bootstrap2D: the plain two-group tests of group ``test_grp[t]`` against group ``ctrl`` on row
    block ``test_row[t]``, as design contrasts.  Design j = {(j, +1.0), (ctrl, -1.0)} for every group j, the guide term first, and
    design ``ng`` is empty: a test takes design ``test_grp[t]`` where ``good`` [row block][group] has its group and the control, the
    empty one (the NaN record) otherwise; its ``rows`` are those of design ``test_grp[t]`` either way.  Returns as
    ``_contrast_design``."""
    test_row, test_grp, ctrl = np.asarray(test_row, dtype=np.int32), np.asarray(test_grp, dtype=np.int32), int(ctrl)
    good = np.asarray(good, dtype=bool).reshape(-1, ng)
    if not 0 <= ctrl < ng or (len(test_grp) and (test_grp.min() < 0 or test_grp.max() >= ng)):
        raise ValueError("contrast: group index out of range")
    if len(test_grp) != len(test_row) or (len(test_row) and (test_row.min() < 0 or test_row.max() >= min(n_rows, len(good)))):
        raise ValueError("contrast: test index out of range")
    design_ptr = np.concatenate([2 * np.arange(ng + 1), [2 * ng]])
    design_grp = np.column_stack([np.arange(ng), np.full(ng, ctrl)]).reshape(-1)
    test_design = np.where(good[test_row, test_grp] & good[test_row, ctrl], test_grp, ng)
    return _contrast_design(planes, ld, B, ng, n_rows, test_row, test_design, design_ptr, design_grp, np.tile([1.0, -1.0], ng),
                            rows_design=test_grp)


def _joint_tables(test_gene, tables, n_rows, ng):
    """The tables of mm_joint_stats / mm_joint1_stats (``Bootstrap1D.joint``, ``Bootstrap2D.joint``), coerced, checked (the kernels
    trust them) and uploaded, empty arrays padded to one element: the CSR rows of ``_csr_tables``, and every design has
    0 <= rank <= n_d <= ``ng`` groups and rank x n_d doubles of ``design_L`` at its offset.  Returns test_gene as an int32 host array
    and the device tensors (test_gene, test_design, design_ptr, design_rank, design_lofs, design_grp, design_L), the order in
    which the kernel takes them."""
    design_rank = np.asarray(tables.design_rank, dtype=np.int32)
    design_lofs = np.asarray(tables.design_lofs, dtype=np.int64)
    design_L = np.asarray(tables.design_L, dtype=np.float64).reshape(-1)
    n_designs = len(np.asarray(tables.design_ptr)) - 1
    if len(design_rank) != n_designs or len(design_lofs) != n_designs:
        raise ValueError("joint: inconsistent table sizes")
    test_gene, test_design, design_ptr, design_grp = _csr_tables("joint", test_gene, tables.test_design, tables.design_ptr, tables.design_grp,
                                                                 n_rows, ng)
    n_d = np.diff(design_ptr).astype(np.int64)
    if (n_d > ng).any() or (design_rank < 0).any() or (design_rank > n_d).any():
        raise ValueError("joint: a design needs 0 <= rank <= its number of groups <= n_groups")
    if n_designs and ((design_lofs < 0).any() or (design_lofs + design_rank * n_d > len(design_L)).any()):
        raise ValueError("joint: design_lofs / design_rank run past design_L")
    return test_gene, (_up(test_gene), _up(test_design), dev(design_ptr), _up(design_rank), _up(design_lofs), _up(design_grp), _up(design_L))


def _joint(planes, ld, B, ng, n_rows, test_row, tables):
    """``joint`` of Bootstrap1D (``planes`` = [ym, yv]: mm_joint_stats) and Bootstrap2D ([yc]: mm_joint1_stats): the joint records, one
    host array [n_tests][8] per plane."""
    torch = _torch()
    test_row, d_tab = _joint_tables(test_row, tables, n_rows, ng)
    n_tests = len(test_row)
    stats = [empty((max(1, n_tests), 8), torch.float64) for _ in planes]
    _lib.call("mm_joint1_stats" if len(planes) == 1 else "mm_joint_stats", *map(P, planes), ld, B, ng, *map(P, d_tab), n_tests,
              *map(P, stats), _stream())
    return [host(s)[:n_tests] for s in stats]


def _valid_cols(ym, yv, ld, B, ng, good, n_genes):
    torch = _torch()
    col_map = empty((max(1, n_genes), B + 1), torch.int32)
    n_valid = empty((max(1, n_genes),), torch.int32)
    d_good = dev(np.asarray(good, dtype=np.uint8))
    _lib.call("mm_valid_cols", P(ym), P(yv), ld, B, ng, P(d_good), n_genes, P(col_map), P(n_valid), _stream())
    return col_map, host(n_valid)[:n_genes]


def _contract_resampled(src, ld, B, ng, n_genes, test_gene, tt, good, gene_mask, M, Nc, rep, bcol, seed, col_map, n_valid):
    torch = _torch()
    s = _stream()
    n_tests = len(test_gene)
    if ng > 32767:
        raise NotImplementedError("resample_rep=True with more than 32767 groups")
    yt = torch.empty_like(src)
    d_gm, d_M = dev(np.asarray(gene_mask, dtype=np.int32)), dev(np.asarray(M, dtype=np.float64))
    _lib.call("mm_residualize", P(src), P(yt), ld, ld, ng, n_genes, P(d_gm), P(d_M), s)
    coef = empty((max(1, n_tests), ld), torch.float64)
    stats = empty((max(1, n_tests), 8), torch.float64)
    d_tg, d_tt, d_good = dev(np.asarray(test_gene, dtype=np.int32)), dev(np.asarray(tt, dtype=np.float64)), dev(np.asarray(good, dtype=np.uint8))
    d_nc = dev(np.asarray(Nc, dtype=np.float64))
    d_rep = dev(np.asarray(rep, dtype=np.int16)) if rep is not None else None
    d_bcol = dev(np.asarray(bcol, dtype=np.int32)) if bcol is not None else None
    d_nv = dev(np.asarray(n_valid, dtype=np.int32)) if n_valid is not None else None
    _lib.call("mm_cross_resampled", P(yt), ld, B, ng, P(d_tg), P(d_tt), P(d_good), P(d_nc), P(d_rep), P(d_bcol),
              P(col_map if n_valid is not None else None), P(d_nv), int(seed) & ((1 << 64) - 1), n_tests, P(coef), P(stats), s)
    return coef, host(stats)[:n_tests]


CROSS_BLOCK_TT = 8            # tests of one gene that a workgroup of mm_cross_resampled_block takes together (contract.hip: XB_TT)
CROSS_BLOCK_MAX_GROUPS = 860  # 76 bytes of LDS per group, 64 KB a workgroup
CROSS_COV_MAX_GROUPS = 468    # mm_cross_resampled_block_cov: 140 bytes of LDS per group (the tile's zt rows beside tt), 64 KB a workgroup
CROSS_COV_SCRATCH_BYTES = 256 << 20   # the beta scratch of a batch of tiles, and the materialised responses of ``rows``


def _block_tables(B, ng, n_genes,gene_ptr, tt, good, gene_mask, M, Nc, rep, bcol, n_valid, gene_key, zt=None):
    """The tables of mm_cross_resampled_block, coerced and checked on the host (the kernel trusts them): ``gene_ptr`` a CSR pointer
    over the rows of ``tt`` [n_tests][ng], one entry per gene slot; ``good`` [n_genes][ng]; ``gene_mask`` [n_genes] into ``M``
    [n_masks][ng][ng]; ``n_valid`` [n_genes] in 0..B + 1; ``rep`` / ``bcol`` [n_genes][ng][B] with, in the rows i < n of a gene with n
    good groups and the columns 1..nb - 1 the kernel reads, 0 <= rep < n and 1 <= bcol <= nb (nb = n_valid - 1, or B);
    ``gene_key`` [n_genes] >= 0; ``zt`` (or None) [n_tests][ng], finite."""
    gene_ptr = np.asarray(gene_ptr, dtype=np.int64).reshape(-1)
    tt = np.ascontiguousarray(tt, dtype=np.float64)
    good = np.ascontiguousarray(np.asarray(good, dtype=bool), dtype=np.uint8)
    gene_mask, M, Nc = np.asarray(gene_mask, dtype=np.int32), np.asarray(M, dtype=np.float64), np.asarray(Nc, dtype=np.float64)
    what = "cross_resampled_block"
    if ng > CROSS_BLOCK_MAX_GROUPS:
        raise NotImplementedError(f"cross_resampled_block with more than {CROSS_BLOCK_MAX_GROUPS} groups")
    if len(gene_ptr) != n_genes + 1 or gene_ptr[0] != 0 or (np.diff(gene_ptr) < 0).any() or tt.ndim != 2 or gene_ptr[-1] != len(tt):
        raise ValueError(f"{what}: gene_ptr is not a CSR pointer over the rows of tt, one entry per gene")
    if len(tt) >= 2 ** 31 - 1 or (len(tt) and tt.shape[1] != ng) or good.shape != (n_genes, ng) or Nc.shape != (ng,):
        raise ValueError(f"{what}: tt, good and Nc do not match the groups")
    if gene_mask.shape != (n_genes,) or M.ndim != 3 or M.shape[1:] != (ng, ng) or (n_genes and (gene_mask.min() < 0 or gene_mask.max() >= len(M))):
        raise ValueError(f"{what}: gene_mask does not index M [n_masks][n_groups][n_groups]")
    nb = np.full(n_genes, B, dtype=np.int64)
    if n_valid is not None:
        n_valid = np.asarray(n_valid, dtype=np.int32)
        if n_valid.shape != (n_genes,) or (n_genes and (n_valid.min() < 0 or n_valid.max() > B + 1)):
            raise ValueError(f"{what}: n_valid must hold 0..num_boot + 1 for every gene")
        nb = n_valid.astype(np.int64) - 1
    if (rep is None) != (bcol is None):
        raise ValueError(f"{what}: rep and bcol come together")
    if rep is not None:
        rep, bcol = np.ascontiguousarray(rep, dtype=np.int16), np.ascontiguousarray(bcol, dtype=np.int32)
        if rep.shape != (n_genes, ng, B) or bcol.shape != rep.shape:
            raise ValueError(f"{what}: rep / bcol must be [n_genes][n_groups][num_boot]")
        n_good = good.sum(axis=1)
        for g in np.flatnonzero((n_good > 0) & (nb >= 2) & (np.diff(gene_ptr) > 0)):
            r, b = rep[g, :n_good[g], 1:nb[g]], bcol[g, :n_good[g], 1:nb[g]]
            if r.min() < 0 or r.max() >= n_good[g] or b.min() < 1 or b.max() > nb[g]:
                raise ValueError(f"{what}: rep / bcol of gene {g} leave its good groups / surviving columns")
    if gene_key is not None:
        gene_key = np.asarray(gene_key, dtype=np.int64)
        if gene_key.shape != (n_genes,) or (n_genes and gene_key.min() < 0):
            raise ValueError(f"{what}: gene_key must hold one non-negative key per gene")
    if zt is not None:
        zt = np.ascontiguousarray(zt, dtype=np.float64)
        if ng > CROSS_COV_MAX_GROUPS:
            raise NotImplementedError(f"{what} with a covariate per test and more than {CROSS_COV_MAX_GROUPS} groups")
        if zt.shape != tt.shape or not np.isfinite(zt).all():
            raise ValueError(f"{what}: zt must be finite and [n_tests][n_groups], one row per row of tt")
    return gene_ptr.astype(np.int32), tt, good, gene_mask, M, Nc, rep, bcol, n_valid, gene_key, zt


def _cross_resampled_block(planes, ld, B, ng, n_genes, gene_ptr, tt, good, gene_mask, M, Nc, rep, bcol, seed, col_map, n_valid, gene_key,
                           zt=None, beta_scratch_bytes=None):
    """``Bootstrap1D.cross_resampled_block`` / ``cross_resampled_family``: the records of every plane of ``planes``, the ``rows``
    closure and the ``family`` closure."""
    torch = _torch()
    s = _stream()
    gene_ptr, tt, good, gene_mask, M, Nc, rep, bcol, n_valid, gene_key, zt = _block_tables(B, ng, n_genes, gene_ptr, tt, good, gene_mask, M,
                                                                                          Nc, rep, bcol, n_valid, gene_key, zt)
    n_tests = len(tt)
    if n_valid is not None and (col_map is None or col_map.dtype != torch.int32 or col_map.numel() < n_genes * (B + 1)):
        raise ValueError("cross_resampled_block: col_map must be the int32 device tensor [n_genes][num_boot + 1] of valid_cols")
    seed = int(seed) & ((1 << 64) - 1)
    test_gene = np.repeat(np.arange(n_genes, dtype=np.int32), np.diff(gene_ptr))
    max_tests = int(np.diff(gene_ptr).max()) if n_genes else 0
    yt = torch.empty_like(planes[0])               # the ONE plane-sized scratch: the residualised rows of plane ``held[0]``
    held = [None]
    d_gm, d_M, d_ptr, d_tt, d_good, d_nc = dev(gene_mask), _up(M.reshape(-1)), dev(gene_ptr), _up(tt.reshape(-1)), _up(good.reshape(-1)), dev(Nc)
    d_rep, d_bcol = (dev(rep), dev(bcol)) if rep is not None else (None, None)
    d_nv = dev(n_valid) if n_valid is not None else None
    d_cm = col_map if n_valid is not None else None
    d_key = _up(gene_key) if gene_key is not None else None
    if zt is not None:
        budget = CROSS_COV_SCRATCH_BYTES if beta_scratch_bytes is None else int(beta_scratch_bytes)
        n_tiles = n_genes * ((max_tests + CROSS_BLOCK_TT - 1) // CROSS_BLOCK_TT)
        batch = int(min(max(1, n_tiles), max(1, budget // (ld * CROSS_BLOCK_TT * 8))))
        d_zt, beta = _up(zt.reshape(-1)), empty((batch * ld * CROSS_BLOCK_TT,), torch.float64)

    def residualise(which):
        if held[0] != which and n_genes:
            _lib.call("mm_residualize", P(planes[which]), P(yt), ld, ld, ng, n_genes, P(d_gm), P(d_M), _stream())
        held[0] = which

    stats, d_stats = [], []
    for which in range(len(planes)):
        residualise(which)
        st = empty((max(1, n_tests), 8), torch.float64)
        if zt is None:
            _lib.call("mm_cross_resampled_block", P(yt), ld, B, ng, P(d_ptr), n_genes, max_tests, P(d_tt), P(d_good), P(d_nc), P(d_rep),
                      P(d_bcol), P(d_cm), P(d_nv), P(d_key), seed, n_tests, P(st), s)
        else:                                      # a batch of tiles at a time: beta of the batch, then its records (same stream)
            for lo in range(0, n_tiles if n_tests else 0, batch):
                _lib.call("mm_cross_resampled_block_cov", P(yt), ld, B, ng, P(d_ptr), n_genes, max_tests, P(d_tt), P(d_zt), P(d_good), P(d_nc),
                          P(d_rep), P(d_bcol), P(d_cm), P(d_nv), P(d_key), seed, n_tests, lo, min(lo + batch, n_tiles), P(beta), P(st), s)
        stats.append(host(st)[:n_tests])
        d_stats.append(st)                         # (the family pass reads coef0 from the records on the device)

    def rows(which, idx, to_host=True, out=None):
        idx = np.asarray(idx, dtype=np.int64)
        out = _rows_out(out, len(idx), ld)
        residualise(int(which))
        scrap = empty((max(1, len(idx)), 8), torch.float64)
        if zt is None:
            a, b = _up(test_gene[idx]), _up(tt[idx].reshape(-1))
            _lib.call("mm_cross_resampled_keyed", P(yt), ld, B, ng, P(a), P(b), P(d_good), P(d_nc), P(d_rep), P(d_bcol), P(d_cm), P(d_nv),
                      P(d_key), seed, len(idx), P(out), P(scrap), _stream())
        else:
            rows_cov(idx, out, scrap)
        return host(out)[: len(idx)] if to_host else out[: len(idx)]

    def rows_cov(idx, out, scrap):
        """The rows of the tests ``idx`` under a covariate per test: their responses are materialised a slice at a time, test l of a
        slice on row block l, and the per-test kernel runs on the copies with the tables (mask, draws, surviving columns, key) of the
        test's gene gathered to row block l."""
        per = int(min(max(1, len(idx)), max(1, budget // (ng * ld * 8))))
        copies = empty((per * ng, ld), torch.float64)
        keys = gene_key if gene_key is not None else np.arange(n_genes, dtype=np.int64)
        for lo in range(0, len(idx), per):
            sl = idx[lo:lo + per]
            g = test_gene[sl]
            d_g, d_z, d_t, d_gd, d_k = dev(g.astype(np.int32)), dev(zt[sl].reshape(-1)), dev(tt[sl].reshape(-1)), dev(good[g].reshape(-1)), dev(keys[g])
            _lib.call("mm_residualize_rank1", P(yt), ld, B, ng, P(d_g), P(d_z), P(d_good), P(d_nc), len(sl), P(copies), _stream())
            own = dev(np.arange(len(sl), dtype=np.int32))
            g_rep, g_bcol = (dev(rep[g]), dev(bcol[g])) if rep is not None else (None, None)
            g_cm = d_cm.view(-1)[: n_genes * (B + 1)].view(n_genes, B + 1)[d_g.long()].contiguous() if d_cm is not None else None
            g_nv = dev(n_valid[g]) if n_valid is not None else None
            o, sc = out[lo:lo + len(sl)], scrap[lo:lo + len(sl)]
            _lib.call("mm_cross_resampled_keyed", P(copies), ld, B, ng, P(own), P(d_t), P(d_gd), P(d_nc), P(g_rep), P(g_bcol), P(g_cm), P(g_nv),
                      P(d_k), seed, len(sl), P(o), P(sc), _stream())

    def family(scale, slab=None):
        scale = np.asarray(scale, dtype=np.float64)
        if scale.shape != (n_tests, len(planes)):
            raise ValueError(f"cross_resampled_family: scale must be [n_tests][{len(planes)}], one column per plane of records")
        slab = 0 if slab is None else int(slab)
        if not 0 <= slab < 2 ** 31:
            raise ValueError("cross_resampled_family: slab must be a positive number of slots (None: the kernel's default)")
        maxrow = [None] * len(planes)
        adj, fam = np.zeros((n_tests, len(planes), 2)), np.zeros((n_genes, len(planes), 2))
        order = sorted(range(len(planes)), key=lambda w: w != held[0])      # the plane the scratch holds first
        for which in order:
            residualise(which)
            maxrow[which] = empty((max(1, n_genes), ld), torch.float64)
            d_adj, d_fam = empty((max(1, n_tests), 2), torch.float64), empty((max(1, n_genes), 2), torch.float64)
            d_sc = _up(np.ascontiguousarray(scale[:, which]))
            _lib.call("mm_cross_resampled_family", P(yt), ld, B, ng, P(d_ptr), n_genes, max_tests, P(d_tt), P(d_good), P(d_nc), P(d_rep),
                      P(d_bcol), P(d_cm), P(d_nv), P(d_key), seed, n_tests, P(d_stats[which]), P(d_sc), slab, P(maxrow[which]), P(d_adj),
                      P(d_fam), _stream())
            adj[:, which], fam[:, which] = host(d_adj)[:n_tests], host(d_fam)[:n_genes]
            maxrow[which] = maxrow[which][:n_genes]
        return maxrow, adj, fam

    return stats, rows, family


# =================================================================================================
# 2D: gene pairs
# =================================================================================================


class GeneColumns:
    """Gene-contiguous copy of the columns of ``genes`` (indices into the blocks' gene space), per block
    (mm_extract_cols).  The pair kernels join two columns through a dense per-cell LDS vector."""

    def __init__(self, blocks, genes):
        torch = _torch()
        self.blocks = blocks
        self.genes = np.asarray(genes, dtype=np.int64)
        M = self.n_cols = len(self.genes)
        nb = blocks.n_blocks
        lens = blocks.blk_cnt[:, self.genes].astype(np.int64)               # [nb][M]
        ptr = np.zeros((nb, M + 1), dtype=np.int64)
        flat = np.cumsum(lens.reshape(-1))
        total = int(flat[-1]) if flat.size else 0
        starts = np.concatenate([[0], flat[:-1]]).reshape(nb, M) if flat.size else np.zeros((nb, M), dtype=np.int64)
        ptr[:, :M] = starts
        ptr[:, M] = starts[:, -1] + lens[:, -1] if M else 0
        self.col_ptr = dev(ptr)
        col_id = np.full(blocks.G, -1, dtype=np.int32)
        col_id[self.genes] = np.arange(M, dtype=np.int32)
        d_col_id = dev(col_id)
        self.cols = zeros((max(1, total),), torch.int32)
        for p, lo in zip(blocks.parts, blocks.part_lo):      # one launch per gene part, each with its slice of the map, all into the one store
            if M == 0 or (col_id[lo:lo + p.G] >= 0).any():       # (no column at all: the C-ABI refuses the launch)
                _lib.call("mm_extract_cols", P(p.ent), P(p.blk_base), P(p.slice_w), P(p.slice_ptr), P(p.item_ptr),
                          P(p.perm), nb, p.G, P(d_col_id[lo:lo + p.G]), M, P(self.col_ptr), P(self.cols), _stream())
        self.slot_of_gene = {int(g): i for i, g in enumerate(self.genes)}


def _group_pairs(col1, col2):
    """Sort pairs by left column -> (order, left_col, left_ptr, right_col_sorted)."""
    col1 = np.asarray(col1, dtype=np.int64)
    col2 = np.asarray(col2, dtype=np.int64)
    order = np.argsort(col1, kind="stable")
    c1s = col1[order]
    left_col, start = np.unique(c1s, return_index=True)
    left_ptr = np.concatenate([start, [len(c1s)]]).astype(np.int64)
    return order, left_col.astype(np.int32), left_ptr, col2[order].astype(np.int32)


def pair_cross(cols, col1, col2, inv_sf_cells):
    """prod[group][pair] = sum_c x_ci x_cj / sf_c^2 for pairs of column slots (K11).  Host array."""
    torch = _torch()
    b = cols.blocks
    order, left_col, left_ptr, right = _group_pairs(col1, col2)
    n_pairs = len(order)
    d_inv = dev(np.asarray(inv_sf_cells, dtype=np.float64)[b.cell_order])
    d_left, d_lptr, d_right = dev(left_col), dev(left_ptr), dev(right)
    scratch = empty((b.n_blocks, max(1, n_pairs)), torch.float64)
    out = empty((b.n_groups, max(1, n_pairs)), torch.float64)
    _lib.call("mm_pair_cross", P(cols.cols), P(cols.col_ptr), cols.n_cols, P(b.d_blk_cell0), P(b.d_grp_blk0), b.n_blocks, b.n_groups,
              P(d_inv), P(d_left), P(d_lptr), len(left_col), P(d_right), n_pairs, P(scratch), P(out), _stream())
    res = np.empty((b.n_groups, n_pairs))
    res[:, order] = host(out)[:, :n_pairs]
    return res


def pair_table_bytes(maxx, genes, col1, col2, n_groups, n_bins):
    """Bytes of the dense (x_i, x_j, sf_bin) histogram tables Bootstrap2D allocates, per pair (all groups): used to size pair
    chunks against the free HBM (a pair of highly expressed genes costs tens of MB per group)."""
    cap = np.asarray(maxx, dtype=np.int64)[:, np.asarray(genes, dtype=np.int64)] + 1            # [group][column slot]
    return (cap[:, np.asarray(col1, dtype=np.int64)] * cap[:, np.asarray(col2, dtype=np.int64)]).sum(axis=0) * int(n_bins) * 4


def contract_plane(plane, ld, B, ng, n_rows, test_row, W, good):
    """K9/K10 on ONE response plane the caller holds (``plane``: fp64 device tensor, rows [row * ng + group][ld], replicate columns
    1..B): test t applies the weight row ``W[t]`` to the groups ``good[test_row[t]]`` of row ``test_row[t]`` < ``n_rows``.
    Returns (coef device tensor [n_tests][ld], stats host [n_tests][8])."""
    torch = _torch()
    n_tests = len(test_row)
    test_row, good = np.asarray(test_row, dtype=np.int32), np.asarray(good, dtype=np.uint8)
    if good.shape != (n_rows, ng) or (n_tests and (test_row.min() < 0 or test_row.max() >= n_rows)) or plane.numel() < n_rows * ng * ld or ld < B + 1:
        raise ValueError("contract_plane: tests, good rows and plane do not match")      # (the kernel trusts the rows)
    coef = empty((max(1, n_tests), ld), torch.float64)
    stats = empty((max(1, n_tests), 8), torch.float64)
    d_tp, d_W, d_good = dev(test_row), dev(np.asarray(W, dtype=np.float64)), dev(good)
    _lib.call("mm_contract_stats", P(plane), P(plane), ld, B, ng, P(d_tp), P(d_W), P(d_good), n_tests, 0, P(coef), P(stats), _stream())
    return coef, host(stats)[:n_tests]


class Bootstrap2D:
    """2D analogue of Bootstrap1D for a list of gene pairs (column slots of a GeneColumns store):
    (x_i, x_j, sf_bin) histograms -> bins -> replay order -> replay bootstrap of the correlation."""

    def __init__(self, cols, col1, col2, maxx, sf_bin_cells, sf_table, grp_q, num_boot):
        torch = _torch()
        self.cols = cols
        b = self.blocks = cols.blocks
        ng = self.ng = b.n_groups
        self.B, self.ld = int(num_boot), int(num_boot) + 1
        self.n_bins = len(sf_table)
        self.sf_table = np.asarray(sf_table, dtype=np.float64)
        self.grp_q = np.asarray(grp_q, dtype=np.float64)
        self.order, left_col, left_ptr, right = _group_pairs(col1, col2)      # kernels see pairs in this order
        self.n_pairs = len(self.order)
        self.n_q = self.n_pairs * ng
        s = _stream()
        # 1D tables of every column (left genes need them for the x_j == 0 column)
        self.h1 = Bootstrap1D(b, cols.genes, maxx, sf_bin_cells, sf_table, grp_q, num_boot)
        c1s = np.asarray(col1, dtype=np.int64)[self.order]
        c2s = np.asarray(col2, dtype=np.int64)[self.order]
        q_left = (c1s[:, None] * ng + np.arange(ng)[None, :]).reshape(-1)
        q_right = (c2s[:, None] * ng + np.arange(ng)[None, :]).reshape(-1)
        xcap_i = self.h1.xcap[q_left].astype(np.int32)
        xcap_j = self.h1.xcap[q_right].astype(np.int32)
        sizes = self.n_bins * xcap_i.astype(np.int64) * xcap_j.astype(np.int64)
        tab_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.d_xi, self.d_xj, self.d_tab_ptr = dev(xcap_i), dev(xcap_j), dev(tab_ptr[:-1])
        self.tab = zeros((max(1, int(tab_ptr[-1])),), torch.int32)
        bins_sorted = np.asarray(sf_bin_cells, dtype=np.uint8)[b.cell_order]
        d_bins = dev(bins_sorted)
        d_left, d_lptr, d_right = dev(left_col), dev(left_ptr), dev(right)
        _lib.call("mm_pair_hist", P(cols.cols), P(cols.col_ptr), cols.n_cols, P(b.d_blk_cell0), P(b.d_blk_group), b.n_blocks, P(d_bins),
                  P(d_left), P(d_lptr), len(left_col), P(d_right), ng, P(self.d_tab_ptr), P(self.d_xi), P(self.d_xj), P(self.tab), s)
        d_hptr = dev(self.h1.tab_ptr[q_left])
        self.d_K = empty((max(1, self.n_q),), torch.int32)
        _lib.call("mm_pair_bins_count", P(self.tab), P(self.d_tab_ptr), P(self.d_xi), P(self.d_xj), P(self.h1.tab), P(d_hptr), self.n_q,
                  self.n_bins, P(self.d_K), s)
        self.K = host(self.d_K)[:self.n_q]
        self.xcap_i, self.xcap_j, self.tab_ptr = xcap_i, xcap_j, tab_ptr

    def bins_of(self, q):
        t0 = int(self.tab_ptr[q])
        ci, cj = int(self.xcap_i[q]), int(self.xcap_j[q])
        tab = host(self.tab[t0:t0 + self.n_bins * ci * cj], np.uint32).reshape(self.n_bins, ci, cj)
        bi, xi, xj = np.nonzero(tab)
        return bi, xi, xj, tab[bi, xi, xj]

    def _order_on_host(self, q, ra, rb, r0, slot, tile_ptr, ops):
        """Replay order + bootstrap operands of ONE (pair, group) with more bins than the in-LDS sort holds, computed on the host
        with the same arithmetic as k_bins_order: code = (x_i*r[0] + x_j*r[1]) + r0*approx_sf ascending (bootstrap.py:62-67)."""
        bi, xi, xj, mu = self.bins_of(q)
        code = (xi.astype(np.float64) * ra + xj.astype(np.float64) * rb) + r0 * self.sf_table[bi]
        o, pk, lq = _replay_order(code, mu, self.blocks.grp_ncells[q % self.ng])
        sf = self.sf_table[bi[o]]
        _write_chain_operands(ops[0], ops, slot, tile_ptr, (pk, lq, xi[o].astype(np.float64), xj[o].astype(np.float64), 1.0 / sf, 1.0 / (sf * sf)))

    def weights_of(self, q):
        """Test helper (after run(fast=True, dump_weights=True)): the int32 multinomial weights [K][B] of chain q."""
        return host(self.w_dump[int(self.pair_slot[q]), :int(self.K[q]), :])

    def run(self, skip, r1a, r1b, r0, true_corr, pcg_seed=5, target_waves=None, fast=False, fast_seed=0, pair_key=None, dump_weights=False,
            keep_fast=False):
        """All arrays are indexed by q = sorted_pair*n_groups + group (see ``self.order``).  Leaves the
        replicate correlations in self.yc [n_q][B+1] (column 0 = true correlation).

        ``fast``: the replicate-parallel kernel (mm_boot2d_fast) on dense 64-wide tiles of the operand planes instead of the replay
        kernels: replicate r of chain q draws from its own PCG64 stream derived from (``fast_seed``, ``pair_key[q]``, r) --
        ``pair_key`` [n_q] int64, default q; keys that do not depend on how the pairs were chunked or ordered make the result
        independent of both -- and ``pcg_seed`` is ignored.  ``dump_weights`` (fast only): keep the weights for ``weights_of``.
        ``keep_fast`` (fast only): keep what a later launch on a replicate range reads (``launch_range``) -- the operand planes, the
        tile layout, the slot tables, the stream keys and the seed.  The default keeps nothing."""
        if (dump_weights or keep_fast) and not fast:
            raise ValueError("dump_weights and keep_fast need fast=True")
        active = (~np.asarray(skip, dtype=bool)) & (self.K >= 1)
        c = self._choose_packing(active, fast, target_waves)
        t = self._lay_out_operands(c, fast)
        self.replay_kernel = None      # diagnostics (tests): the kernel launched
        status, ordered = _order_bins(self, "mm_bins_order2d", (self.d_xi, self.d_xj), ORDER_BIG_CAP_2D, c.order, t, (r1a, r1b, r0))
        launched = self._launch(c, t, fast, true_corr, pcg_seed, fast_seed, pair_key, dump_weights, keep_fast)
        _check_order_status(status, "mm_bins_order2d")
        del ordered, launched      # NB: every device operand must stay referenced until after the call that reads it
        self.active = active
        self.pair_slot = t.pair_slot

    def _choose_packing(self, active, fast, target_waves):
        """The chains, longest first, and their (tile, lane) slots.  fast: one WAVE per 64 replicates of a chain, lanes = replicates: plain
        64-wide tiles, longest chains dispatched first; replay: the cost-model lane packing and dispatch order of the 2D kernel."""
        act = np.flatnonzero(active)
        c = SimpleNamespace()
        order = c.order = act[np.argsort(-self.K[act], kind="stable")]
        if fast:
            c.slot_of, c.n_tiles = pack_lanes(self.K[order], 0, dense=True)
        else:
            slot_of, c.n_tiles = pack_lanes(self.K[order], PACK_WAVES if target_waves is None else target_waves, consts=PACK2D, cost=PACK_COST_2D)
            c.slot_of = pair_tiles(slot_of, c.n_tiles, self.K[order], cost=PACK_COST_2D)
        self.n_tiles = c.n_tiles
        self.draws_per_replicate = int(np.maximum(self.K[order] - 1, 0).sum())
        return c

    def _lay_out_operands(self, c, fast):
        """Slot tables of the tile launch and the operands: six [rows][64] planes, or (mm_boot2d_replay_rec) 8-double records."""
        torch = _torch()
        t = _plan_tiles(self.K, c.order, c.slot_of, c.n_tiles, self.n_q, self.blocks.grp_ncells, self.grp_q, self.ng)
        self.wave_steps_per_replicate = rows = int(t.tile_ptr[-1])
        t.use_rec = BOOT2D_RECORDS and c.n_tiles > 0 and not fast
        if t.use_rec:
            # per-chain operand records (8 doubles per bin) instead of [row][64] planes: a lane reads memory of its own wherever it is in
            # its chain, so the kernel can let a rejected BTPE attempt retry in the next bin step (mm_boot2d_replay_rec)
            rec_base = _plan_records(self.K, c.order)[1]
            t.ops = [empty((8 * max(1, int(rec_base[-1])),), torch.float64)] + [empty((8,), torch.float64) for _ in range(5)]
            self.tile_slot = t.pair_slot.copy()
            t.pair_slot[c.order] = CHAIN_SLOT | rec_base[:-1]
            t.slot_rec = _per_slot(c.n_tiles * 64, c.slot_of, rec_base[:-1], -1, np.int64)
        else:
            t.ops = [empty((max(1, rows) * 64,), torch.float64) for _ in range(6)]
        return t

    def _launch(self, c, t, fast, true_corr, pcg_seed, fast_seed, pair_key, dump_weights, keep_fast=False):
        """The replicate rows self.yc and the tile kernel that fills them.  Returns its device operands."""
        torch, s = _torch(), _stream()
        B, ld, n_tiles = self.B, self.ld, c.n_tiles
        self._fast = None
        self.yc = torch.full((max(1, self.n_q), ld), float("nan"), dtype=torch.float64, device="cuda")
        self.yc[: self.n_q, 0] = dev(np.asarray(true_corr, dtype=np.float64))
        d_slot_K, d_nobs, d_omq, d_slot_pair = dev(t.slot_K), dev(t.nobs), dev(t.omq), dev(t.slot_pair)
        keep = [d_slot_K, d_nobs, d_omq, d_slot_pair]
        kmax_dump = int(t.tile_k.max()) if dump_weights and n_tiles else 0      # (dump_weights: fast only)
        self.w_dump = zeros((n_tiles * 64, kmax_dump, B), torch.int32) if dump_weights and n_tiles else None
        if n_tiles and fast:
            keys = np.arange(self.n_q, dtype=np.int64) if pair_key is None else np.asarray(pair_key, dtype=np.int64)
            d_slot_key = dev(_per_slot(n_tiles * 64, c.slot_of, keys[c.order], 0, np.int64))
            keep.append(d_slot_key)
            _lib.call("mm_boot2d_fast", *map(P, t.ops), P(t.d_tile_ptr), n_tiles * 64, P(d_slot_K), P(d_nobs), P(d_omq), P(d_slot_pair),
                      P(d_slot_key), int(fast_seed) & ((1 << 64) - 1), B, ld, P(self.yc), P(self.w_dump), kmax_dump, s)
            self.replay_kernel = "mm_boot2d_fast"
            if keep_fast:      # what a later launch on a replicate range reads (launch_range)
                self._fast = SimpleNamespace(ops=t.ops, d_tile_ptr=t.d_tile_ptr, n_slots=n_tiles * 64, d_slot_K=d_slot_K, d_nobs=d_nobs, d_omq=d_omq,
                                             pair_slot=t.pair_slot, d_slot_key=d_slot_key, kmax=int(t.tile_k.max()),
                                             seed=int(fast_seed) & ((1 << 64) - 1))
        elif n_tiles and t.use_rec:
            d_slot_rec = dev(t.slot_rec)
            keep.append(d_slot_rec)
            _lib.call("mm_boot2d_replay_rec", P(t.ops[0]), P(d_slot_rec), n_tiles, P(d_slot_K), P(d_nobs), P(d_omq), P(d_slot_pair),
                      pcg64_state(pcg_seed), B, ld, P(self.yc), s)
            self.replay_kernel = "mm_boot2d_replay_rec"
        elif n_tiles:
            _lib.call("mm_boot2d_replay", *map(P, t.ops), P(t.d_tile_ptr), n_tiles, P(d_slot_K), P(d_nobs), P(d_omq), P(d_slot_pair),
                      pcg64_state(pcg_seed), B, ld, P(self.yc), s)
            self.replay_kernel = "mm_boot2d_replay"
        return keep

    def launch_range(self, rep_lo, rep_n, open_q, plane, row_of_q, dump_weights=False):
        """After ``run(fast=True, keep_fast=True)``: the replicates [rep_lo, rep_lo + rep_n) of the chains ``open_q`` (q = sorted_pair
        * n_groups + group; mm_boot2d_fast_range on the kept operand planes, tile layout and stream keys; every other slot gets row
        -1 and writes nothing) into columns 1..rep_n of the rows ``row_of_q`` of the caller's ``plane``, a contiguous fp64 device
        tensor [rows][ld >= 1 + rep_n]; nothing else of it is written.  Chains of ``open_q`` that did not run (skipped, K < 1) are
        left out.  Replicate rep_lo + i of a chain is bit for bit the one a one-shot ``run`` over more replicates stores in column
        1 + rep_lo + i.  ``dump_weights``: keep the int32 weights in ``self.w_dump_range`` [slot][k][i] (slot =
        ``self.pair_slot[q]``)."""
        return self._launch_range(rep_lo, rep_n, open_q, plane, row_of_q, dump_weights, False)

    def launch_listed(self, rep_lo, rep_n, open_q, plane, row_of_q, dump_weights=False):
        """``launch_range`` with a grid over the chains it is given: the launch covers only the slots of ``open_q``
        (mm_boot2d_fast_slots on their ascending, unique list: len(list) x ceil(rep_n / 64) waves instead of one wave per slot of
        the layout and 64 replicates) and only their entries of the slot-row table are written -- a table the chunk keeps from its
        first listed launch on, whose other entries no listed launch reads.  Same checks, and the cells written are those of
        ``launch_range``, bit for bit.  There is no weight dump: ``dump_weights`` raises.  Returns the device arrays the launch
        reads, to be kept like ``launch_range``'s."""
        return self._launch_range(rep_lo, rep_n, open_q, plane, row_of_q, dump_weights, True)

    def _launch_range(self, rep_lo, rep_n, open_q, plane, row_of_q, dump_weights, listed):
        torch, f = _torch(), getattr(self, "_fast", None)
        if f is None:
            raise RuntimeError("launch_range needs a preceding run(fast=True, keep_fast=True): nothing else keeps the operands and the streams")
        if listed and dump_weights:
            raise ValueError("launch_listed has no weight dump")
        rep_lo, rep_n = int(rep_lo), int(rep_n)
        if rep_lo < 0 or rep_n < 1 or rep_lo + rep_n > 2 ** 31 - 1:
            raise ValueError("launch_range: need rep_lo >= 0, rep_n >= 1 and rep_lo + rep_n <= 2^31 - 1")
        if (not torch.is_tensor(plane) or plane.dtype != torch.float64 or not plane.is_cuda or not plane.is_contiguous() or plane.dim() != 2
                or plane.shape[1] < rep_n + 1):
            raise ValueError("launch_range: plane must be a contiguous fp64 device tensor [rows][>= 1 + rep_n]")
        open_q, row_of_q = np.asarray(open_q, dtype=np.int64).reshape(-1), np.asarray(row_of_q, dtype=np.int64).reshape(-1)
        if len(open_q) != len(row_of_q) or (len(open_q) and (open_q.min() < 0 or open_q.max() >= self.n_q)):
            raise ValueError("launch_range: open_q / row_of_q do not match the chains")
        if len(row_of_q) and (row_of_q.min() < 0 or row_of_q.max() >= plane.shape[0]):
            raise ValueError("launch_range: row out of range")       # (the kernel trusts the rows)
        slot = f.pair_slot[open_q]
        if listed:
            has = slot >= 0
            by_slot = np.argsort(slot[has], kind="stable")
            slots, rows = slot[has][by_slot].astype(np.int64), row_of_q[has][by_slot]
            last = np.append(slots[1:] != slots[:-1], True)[:len(slots)]      # a chain given twice: its last row, as in the default launch
            slots, rows = slots[last], rows[last]
            if len(slots) and (slots[0] < 0 or slots[-1] >= f.n_slots):
                raise ValueError("launch_range: slot out of range")       # (the kernel trusts the list)
            if getattr(f, "d_slot_row", None) is None:
                f.d_slot_row = torch.full((max(1, f.n_slots),), -1, dtype=torch.int64, device="cuda")
            d_list, d_rows = _up(slots), _up(rows)
            if len(slots):
                f.d_slot_row[d_list] = d_rows
            _lib.call("mm_boot2d_fast_slots", *map(P, f.ops), P(f.d_tile_ptr), f.n_slots, P(f.d_slot_K), P(f.d_nobs), P(f.d_omq),
                      P(f.d_slot_row), P(f.d_slot_key), f.seed, rep_lo, rep_n, plane.shape[1], P(plane), P(d_list), len(slots), _stream())
            return d_list, d_rows      # NB: stay referenced until the caller's next call on the stream
        slot_row = np.full(f.n_slots, -1, dtype=np.int64)
        slot_row[slot[slot >= 0]] = row_of_q[slot >= 0]
        d_slot_row = dev(slot_row)
        self.w_dump_range = zeros((f.n_slots, f.kmax, rep_n), torch.int32) if dump_weights else None
        _lib.call("mm_boot2d_fast_range", *map(P, f.ops), P(f.d_tile_ptr), f.n_slots, P(f.d_slot_K), P(f.d_nobs), P(f.d_omq), P(d_slot_row),
                  P(f.d_slot_key), f.seed, rep_lo, rep_n, plane.shape[1], P(plane), P(self.w_dump_range), f.kmax if dump_weights else 0,
                  _stream())
        return d_slot_row      # NB: stays referenced until the caller's next call on the stream

    def valid_cols(self, good):
        """hypothesis_test.py:372-373 on the device (see Bootstrap1D.valid_cols)."""
        return _valid_cols(self.yc, self.yc, self.ld, self.B, self.ng, good, self.n_q // self.ng)

    def contract_resampled(self, test_pair, tt, good, pair_mask, M, Nc, rep=None, bcol=None, seed=0, col_map=None, n_valid=None):
        """resample_rep=True on the correlation rows (hypothesis_test.py:393-404).  Same kernels and conventions as
        Bootstrap1D.contract_resampled."""
        return _contract_resampled(self.yc, self.ld, self.B, self.ng, self.n_q // self.ng, test_pair, tt, good, pair_mask, M, Nc, rep, bcol,
                                   seed, col_map, n_valid)

    def contract(self, test_pair, W, good):
        """K9/K10 on the correlation rows: tests (sorted pair index, weight row)."""
        return contract_plane(self.yc, self.ld, self.B, self.ng, self.n_pairs, test_pair, W, np.asarray(good).reshape(self.n_pairs, self.ng))

    def contrast(self, test_pair, test_grp, ctrl, good):
        """Two-group contrasts of the correlation rows against the control group ``ctrl``, as ``Bootstrap1D.contrast``
        (``_contrast``) with ``good`` [pair][group] in device pair order.  Returns (stats, rows) as ``contrast_design``."""
        (stats,), rows = _contrast([self.yc], self.ld, self.B, self.ng, self.n_pairs, test_pair, test_grp, ctrl, good)
        return stats, functools.partial(rows, 0)

    def contrast_design(self, test_pair, test_design, design_ptr, design_grp, design_w):
        """Guide-vs-control contrasts on the correlation rows (mm_contrast_design1_stats): test t applies the sparse weight row
        ``design_grp/design_w[design_ptr[d]:design_ptr[d + 1]]``, d = ``test_design[t]``, to the replicate rows of pair
        ``test_pair[t]`` (device pair order, ``self.order``).  Returns (stats host [n_tests][8], ``rows(idx)`` giving the
        coefficient rows of selected tests on demand; ``to_host`` / ``out`` as in ``Bootstrap1D.contrast``)."""
        (stats,), rows = _contrast_design([self.yc], self.ld, self.B, self.ng, self.n_pairs, test_pair, test_design, design_ptr, design_grp,
                                          design_w)
        return stats, functools.partial(rows, 0)

    def family_maxt(self, family_ptr, test_pair, test_design, design_ptr, design_grp, design_w, scale, stage_cap=None):
        """Single-step max-T adjustment over families of design contrasts on the correlation rows (mm_family_maxt1), as
        ``Bootstrap1D.family_maxt`` on one plane: the tests ``family_ptr[f]:family_ptr[f + 1]`` -- consecutive, on one pair of
        ``test_pair`` (device pair order, ``self.order``) -- are family f, with the tables of ``contrast_design``; ``scale``
        [test][1] is ``family_scale`` of its records.  Returns ``maxrow`` (device [n_fam][1][ld]), ``adj`` (host [n_tests][1][2]:
        t0, n_adj) and ``fam`` (host [n_fam][1][2]: n_valid_family, n_included)."""
        return _family_maxt([self.yc], self.ld, self.B, self.ng, self.n_pairs, family_ptr, test_pair, test_design, design_ptr, design_grp,
                            design_w, scale, stage_cap)

    def joint(self, test_pair, tables):
        """Joint tests of a treatment block on the correlation rows (mm_joint1_stats): test t applies the linear forms of design
        ``tables.test_design[t]`` (``memento._ht.joint_tables``, as for ``Bootstrap1D.joint``) to the replicate rows of pair
        ``test_pair[t]`` (device pair order, ``self.order``).  Returns stats, a host array [n_tests][8]: the joint record of
        include/memento_hip.h."""
        return _joint([self.yc], self.ld, self.B, self.ng, self.n_pairs, test_pair, tables)[0]
