/* memento_hip.h -- C-ABI of libmemento_hip.so (hand-written HIP for gfx950 / MI355X).
 *
 * The reference (atarashansky/scrna-parameter-estimation, package `memento`) is pure Python; it has no
 * FFI.  These entry points are what a ctypes binding inside memento/main.py would call in place of the
 * numpy/scipy expressions cited on each function (paths relative to /root/reference/).  See
 * INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *  - every pointer named d_* is a DEVICE pointer (hipMalloc / torch .data_ptr()); h_* is host memory;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on it
 *    unless stated otherwise; the library never allocates in a launch function;
 *  - return value: 0 = ok, negative = error (mm_last_error() gives the text, thread-local);
 *  - no torch types anywhere; plain pointers and sizes only.
 *
 * Device data layout ("count blocks"): cells are ordered by group and cut into blocks of <= 8192
 * cells of ONE group.  Each block is stored gene-major as SELL-64 (sliced ELLPACK, 64 genes per slice,
 * genes sorted by their nnz inside the block so a slice has no padding to speak of):
 *      entry (uint32) = cell_local (13 bits) | count << 13 (19 bits, 0 = padding)
 *      ent[blk_base[b] + slice_ptr[b][t] + j*64 + lane]   j < slice_w[b][t],  gene = perm[b][t*64+lane]
 * so that lane-per-gene kernels read perfectly coalesced 256-B rows and need no cross-lane reduction.
 */
#ifndef MEMENTO_HIP_H
#define MEMENTO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_CELL_BITS 13
#define MM_BLOCK_CELLS (1 << MM_CELL_BITS) /* max cells per count block */
#define MM_MAX_COUNT ((1u << (32 - MM_CELL_BITS)) - 1u)

const char *mm_last_error(void);
int mm_version(void);
int mm_device_count(void);
int mm_set_device(int dev);

/* raw device-memory helpers so a ctypes-only caller needs nothing but this library */
int mm_malloc(void **d_ptr, size_t bytes);
int mm_free(void *d_ptr);
int mm_memset(void *d_ptr, int value, size_t bytes, void *stream);
int mm_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream);
int mm_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream);
int mm_sync(void *stream);
/* HIP-event timing of whatever is enqueued between begin and end on `stream` (bench.py roofline) */
int mm_timer_create(void **timer);
int mm_timer_begin(void *timer, void *stream);
int mm_timer_end(void *timer, void *stream);
int mm_timer_elapsed_ms(void *timer, float *ms); /* synchronises on the end event */
int mm_timer_destroy(void *timer);

/* Measurement aid (no reference counterpart): streaming read of n_bytes (multiple of 64 KiB) with the access pattern of
 * mm_moments1d_sell (64 KiB work items, dwordx4 per lane, 8 rows in flight).  mode 0: loads only -- the read bandwidth this
 * device reaches for that pattern; 1: + the per-entry 8-byte LDS gather; 2: + the fp64 arithmetic; 3: + five result stores per
 * (chunk, lane) (d_sink must then hold n_bytes / 65536 * 64 * 32 bytes).  tools/hbm_read_peak.py */
int mm_debug_read_probe(const void *d_src, int64_t n_bytes, int32_t n_workgroups, int32_t mode, uint32_t *d_sink, void *stream);

/* ---- K3: row sums of the CSR, optionally restricted to a gene mask ---------------------------
 * replaces X.sum(axis=1) / X.multiply(mask).sum(axis=1)   memento/estimator.py:65, :73 */
int mm_csr_rowsum(const int64_t *d_indptr, const int32_t *d_indices, const float *d_data, int64_t n_rows,
                  const uint8_t *d_gene_mask /* NULL = all genes */, double *d_out, void *stream);

/* ---- gene sharding on the device (multi-GPU: every rank keeps all cells x its own gene range) --------------------
 * replaces the host-side X[:, lo:hi] (scipy fancy indexing, O(nnz)) in front of the reference's per-gene fan-out
 * (memento/main.py:379-397).  mm_csr_colcount: d_row_nnz[r] = entries of row r with col_lo <= column < col_hi.
 * The caller builds d_out_indptr as the exclusive scan of d_row_nnz (n_rows + 1 values); mm_csr_colsplit then writes those
 * entries, in their original order and with column - col_lo, to d_out_indices / d_out_data. */
int mm_csr_colcount(const int64_t *d_indptr, const int32_t *d_indices, int64_t n_rows, int32_t col_lo, int32_t col_hi,
                    int64_t *d_row_nnz, void *stream);
int mm_csr_colsplit(const int64_t *d_indptr, const int32_t *d_indices, const float *d_data, int64_t n_rows, int32_t col_lo,
                    int32_t col_hi, const int64_t *d_out_indptr, int32_t *d_out_indices, float *d_out_data, void *stream);

/* The same for an arbitrary gene SET (cost-balanced shards are not contiguous): d_col_map[g] = new id of a kept gene, -1 = dropped;
 * the new ids must ascend with g so that rows stay sorted.  mm_csr_colsum: per-gene totals (the cost the balancing uses). */
int mm_csr_mapcount(const int64_t *d_indptr, const int32_t *d_indices, int64_t n_rows, const int32_t *d_col_map, int64_t *d_row_nnz,
                    void *stream);
int mm_csr_mapsplit(const int64_t *d_indptr, const int32_t *d_indices, const float *d_data, int64_t n_rows, const int32_t *d_col_map,
                    const int64_t *d_out_indptr, int32_t *d_out_indices, float *d_out_data, void *stream);
int mm_csr_colsum(const int32_t *d_indices, const float *d_data, int64_t nnz, double *d_out /* [n_genes], zeroed by the caller */,
                  void *stream);

/* ---- K0: ingest = CSR -> group-ordered SELL count blocks --------------------------------------
 * replaces util._select_cells(adata, group) = adata.X[mask].tocsc() per group
 *   memento/util.py:8-13, memento/main.py:128
 * d_cell_order[n_sel]: original cell index of every selected cell, sorted by group;
 * d_blk_cell0[n_blocks+1]: block b covers cell_order[blk_cell0[b] .. blk_cell0[b+1]) (one group each).
 * Step 1 counts nnz per (block, gene) and validates the data (integer valued, 0 < x <= MM_MAX_COUNT;
 * d_status[0] != 0 afterwards means invalid data).
 * Width: one set of count blocks holds n_genes <= 60000 (mm_sell_layout's per-block rank table in LDS; the K0 / K1 / K5 / K11
 * kernels that index slices stop at 65536).  A caller with more genes PARTITIONS THE COLUMNS, as the Python engine does
 * (engine.count_blocks): cut the gene axis into contiguous ranges of <= 60000 (the engine takes 59392 = 58 ranges of 1024), take
 * each range out of the CSR with mm_csr_colcount + mm_csr_colsplit, ingest it into count blocks of its own on the SAME cell
 * plan (d_cell_order / d_blk_cell0 depend only on the grouping), and launch the kernels that read count blocks once per range:
 * mm_moments1d_sell / _reduce write that range's slice of the per-gene outputs; mm_hist1d_sell and mm_extract_cols take that
 * range's slice of d_gene_pairbase / d_col_id and write into the ONE set of tables / columns, which are indexed by pair / column
 * slot, not by gene.  mm_csr_colsplit drops entries whose column lies in no range: compare the ranges' entry counts with
 * d_indptr to keep the column-index validation.
 * A CSR without a stored entry (a column range that no selected cell touches, an empty matrix) is a valid input: all-zero
 * d_blk_cnt, no rows, zero moments.  d_indices / d_data must still be non-NULL and hold one readable element -- every entry point
 * refuses NULL, and mm_sell_scatter_ranges reads element 0 on behalf of a tile without entries (engine.DeviceCSR.entry_ptrs).  */
int mm_sell_count(const int64_t *d_indptr, const int32_t *d_indices, const float *d_data, const int32_t *d_cell_order,
                  const int32_t *d_blk_cell0, int32_t n_blocks, int32_t n_genes, uint16_t *d_blk_cnt /* [nb][G] */,
                  int32_t *d_status, void *stream);
/* Step 2: per block sort genes by descending count -> rank/perm, slice widths/pointers and work items.
 * n_slices = ceil(G/64).  A slice is stored as slice_w[t] rows of 64 lanes x 4 entries (one dwordx4 per
 * lane per row; lane = gene slot, 4 consecutive entries of that gene).  slice_ptr is in rows, relative to
 * the block; d_blk_rows[b] = rows of block b (host scans it into blk_base, in rows).  A work item is
 * <= 64 rows of one slice; item_ptr[b][t] numbers them slice-major, d_blk_items[b] = items of block b. */
int mm_sell_layout(const uint16_t *d_blk_cnt, int32_t n_blocks, int32_t n_genes, int32_t *d_rank /* [nb][G] */,
                   int32_t *d_perm /* [nb][n_slices*64], -1 = no gene */, int32_t *d_slice_w /* [nb][n_slices] */,
                   int32_t *d_slice_ptr /* [nb][n_slices+1] */, int32_t *d_item_ptr /* [nb][n_slices+1] */,
                   int64_t *d_blk_rows /* [nb] */, int32_t *d_blk_items /* [nb] */, void *stream);
/* Step 3: scatter entries (d_ent must be zero-filled, 256 uint32 per row, sum(blk_rows) rows). */
int mm_sell_scatter(const int64_t *d_indptr, const int32_t *d_indices, const float *d_data, const int32_t *d_cell_order,
                    const int32_t *d_blk_cell0, int32_t n_blocks, int32_t n_genes, const int32_t *d_rank,
                    const int32_t *d_slice_ptr, const int64_t *d_blk_base, uint32_t *d_ent, void *stream);
/* Range-partitioned form of steps 1 and 3 for rows with strictly ascending column indices (canonical CSR): the path the
 * Python driver takes; mm_sell_count / mm_sell_scatter above remain for unsorted rows.  The gene ids are cut into
 * n_ranges = ceil(G / MM_RANGE_GENES) ranges of MM_RANGE_GENES = 1024 consecutive ids (G <= 65536 per ingest; more genes: see above).
 * mm_sell_split_count, one pass over the column indices: d_rowsplit[k][r], k = 0..R = absolute position in d_indices / d_data at
 * which range k begins in selected row r (block order, n_sel rows; range-major so that a (block, range) workgroup reads contiguous
 * runs); d_status |= 2 if some row is not strictly ascending or has a column outside [0, G); and d_blk_cnt as mm_sell_count fills
 * it, without the value check (d_blk_cnt must be ZERO-FILLED, 4-byte aligned and hold an even number of uint16: partial counts
 * are merged by 32-bit atomics).
 * mm_sell_scatter_ranges places the entries in the layout of mm_sell_scatter and validates the values (d_status |= 1: not a
 * positive integer count <= MM_MAX_COUNT); d_indices / d_data need no alignment beyond their element size.
 * One workgroup per (block, range).  Stores are written through on this chip -- a lone 4-byte store costs ~26 B of HBM write
 * traffic (measured: the unpartitioned scatter writes 7.8x its algorithmic bytes, profiles/r02_k1_traffic_C3.json) -- so the
 * scatter assembles entries in LDS, tile of <= 128 rows by tile, and stores only complete 16-byte groups (4 consecutive entries
 * of one gene).  An entry's position inside its gene is computed, not handed out: entries before the tile + bits below its row
 * in the gene's 128-bit row mask of the tile.  So a gene's entries are in ascending cell order and the ingest is DETERMINISTIC. */
#define MM_RANGE_SHIFT 10
#define MM_RANGE_GENES (1 << MM_RANGE_SHIFT)
#define MM_MAX_RANGES 64
int mm_sell_split_count(const int64_t *d_indptr, const int32_t *d_indices, const int32_t *d_cell_order, const int32_t *d_blk_cell0,
                        int32_t n_blocks, int64_t n_sel, int32_t n_genes, int32_t n_ranges,
                        int64_t *d_rowsplit /* [n_ranges+1][n_sel] */, uint16_t *d_blk_cnt /* [nb][G], zero-filled */,
                        int32_t *d_status, void *stream);
int mm_sell_scatter_ranges(const int64_t *d_indptr, const int32_t *d_indices, const float *d_data, const int32_t *d_cell_order,
                           const int32_t *d_blk_cell0, int32_t n_blocks, int32_t n_genes, int32_t n_ranges, int64_t n_sel,
                           const int64_t *d_rowsplit, const int32_t *d_rank, const int32_t *d_slice_ptr, const int64_t *d_blk_base,
                           uint32_t *d_ent, int32_t *d_status, void *stream);

/* ---- K1+K2: per-(item, gene slot) moment sums from the count blocks  (the HBM-roofline kernel) ---
 * replaces estimator._hyper_1d_relative sparse branch  memento/estimator.py:177-180
 *          and group_cells.mean(axis=0) / .max(axis=0)   memento/main.py:201, :206
 * d_inv_sf[n_sel]: 1/size_factor per selected cell in block order.
 * d_slab [sum(blk_items)][64] records of 32 bytes: {S1 = sum x/sf, S2 = sum x^2/sf^2, S3 = sum x/sf^2 (fp64),
 * SX = sum x (uint32, exact), MX = max x (uint32)} -- one contiguous 2 KiB run per work item.
 * d_blk_item_base = exclusive scan of blk_items. */
int mm_moments1d_sell(const uint32_t *d_ent, const int64_t *d_blk_base, const int32_t *d_slice_w, const int32_t *d_slice_ptr,
                      const int32_t *d_item_ptr, const int64_t *d_blk_item_base, const int32_t *d_blk_cell0,
                      const double *d_inv_sf, int32_t n_blocks, int32_t n_genes, void *d_slab, void *stream);
/* deterministic reduction of the slab over items and over the blocks of each group -> [n_groups][G] */
int mm_moments1d_reduce(const void *d_slab, const int32_t *d_rank, const int32_t *d_item_ptr, const int64_t *d_blk_item_base,
                        const int32_t *d_grp_blk0 /* [n_groups+1] first block of each group */, int32_t n_groups,
                        int32_t n_genes, double *d_out_S /* [3][n_groups][G] */, uint64_t *d_out_sumx /* [n_groups][G] */,
                        uint32_t *d_out_maxx /* [n_groups][G] */, void *stream);

/* ---- K5: integer histograms keyed (group, gene, sf_bin, count) --------------------------------
 * replaces bootstrap._unique_expr's np.unique over cells  memento/bootstrap.py:62-71 (the bins as a SET;
 * their replay ORDER is applied by mm_bins_order).  Pair p = gene_slot*n_groups + group for the tested
 * genes; d_gene_pairbase[G] = gene_slot*n_groups or -1 if the gene is not tested.  Table of pair p starts
 * at d_tab_ptr[p], is [n_sf_bins][xcap[p]] uint32 with xcap[p] = max count of the pair + 1
 * (column 0 is filled with the zero-count cells by mm_bins_count). Tables must be zeroed by the caller. */
int mm_hist1d_sell(const uint32_t *d_ent, const int64_t *d_blk_base, const int32_t *d_slice_w, const int32_t *d_slice_ptr,
                   const int32_t *d_item_ptr, const int32_t *d_perm, const int32_t *d_blk_cell0, const int32_t *d_blk_group,
                   const uint8_t *d_sf_bin /* [n_sel] block order */, int32_t n_blocks, int32_t n_genes,
                   const int32_t *d_gene_pairbase, const int64_t *d_tab_ptr, const int32_t *d_xcap, uint32_t *d_tab, void *stream);
/* zero-count column + number of non-empty bins per pair.  d_grp_bin_cells[n_groups][n_sf_bins] = cells per (group, sf bin) */
int mm_bins_count(uint32_t *d_tab, const int64_t *d_tab_ptr, const int32_t *d_xcap, int64_t n_pairs, int32_t n_groups,
                  int32_t n_sf_bins, const uint32_t *d_grp_bin_cells, int32_t *d_K /* [n_pairs] */, void *stream);

/* ---- K5b+K6 prep: order the bins like np.unique(code) and lay them out for the bootstrap ---------
 * code = count*r1 + r0*approx_sf[sf_bin] in IEEE fp64 (memento/bootstrap.py:62-67); ascending.
 * Pairs are assigned to lanes of 64-wide tiles (d_pair_slot[p] = tile*64+lane or -1 to skip; a tile may
 * leave lanes empty); tile t owns bin rows [tile_ptr[t], tile_ptr[t+1]) of 64 lanes each.  Per bin k the
 * kernel writes, at [(tile_ptr[t]+k)*64 + lane]:
 *   pk = pix[k]/remaining_p  with pix = mult/N_g and remaining_p as numpy's random_multinomial updates it
 *        (replicate-independent), lq = log(1-p) as the inversion sampler needs it,
 *   v = count, a = 1/sf, b = 1/sf^2                                              (fp64 each).
 * A pair may instead be given to the one-wave-per-chain kernel (mm_boot1d_chain): d_pair_slot[p] = MM_CHAIN_SLOT | row, and
 * the kernel writes the same five values of bin k as one 8-double record {pk, lq, v, a, b, -, -, -} at d_pk + 8*(row + k)
 * (the caller reserves that region behind the tile rows of the d_pk allocation).
 * d_status[0] |= 8 if two bins of a pair collide in code (np.unique would merge them). */
#define MM_CHAIN_SLOT (1LL << 62)
int mm_bins_order(const uint32_t *d_tab, const int64_t *d_tab_ptr, const int32_t *d_xcap, const int32_t *d_K,
                  const int64_t *d_pair_list, int64_t n_list /* pairs handled by this launch */,
                  int32_t big /* 0: K <= 1024 (one wave per pair); 1: K <= 8192 (512 threads per pair) */, int32_t n_groups,
                  int32_t n_sf_bins, const double *d_sf_table /* [n_sf_bins] approx size factor of each bin */,
                  const double *d_r1, const double *d_r0 /* per pair */, const int64_t *d_pair_slot, const int64_t *d_tile_ptr,
                  const double *d_grp_ncells /* [n_groups] */, double *d_pk, double *d_lq, double *d_v, double *d_a, double *d_b,
                  int32_t *d_status, void *stream);

/* Profiling hook (no reference counterpart): when d_buf != NULL, every later mm_boot1d_replay launch writes, per tile
 * (wave), {start, end (100 MHz wall clock), HW_ID, XCC_ID} into d_buf[tile*4 .. tile*4+3]; d_buf must hold 4*n_tiles
 * int64.  Pass NULL to switch it off.  Process-global; used by tools/replay_balance.py only. */
int mm_debug_wave_clock(int64_t *d_buf);
/* Measurement / test aid: exact != 0 makes the replay kernels (1D and 2D) evaluate every sampler search loop in numpy's fp64
 * arithmetic; 0 (default) uses the guarded fp32 evaluation of those loops (csrc/npy_rng.h: same integer draws, the guard sends
 * the ~0.1-0.5 % of draws that land near a decision threshold to the fp64 arithmetic).  Process-wide switch. */
int mm_debug_replay_arith(int32_t exact);
/* Test aid: the guarded fp32 inversion search (csrc/npy_rng.h, binomial_inversion_fast) of thread i's (d_U[i], d_n[i], d_p[i]) through
 * both forms of its ladder: form 0 the nested ifs, form 1 the device's one-saved-mask asm statement.  Needs n >= 1, 0 < p <= 0.5 and
 * n p <= 30, as the samplers call it.  ``count`` threads are launched (one workgroup of exactly ``count`` threads up to 256); within a
 * wave only the lanes whose bit is set in lane_mask run the searches.  d_out[(form * 4 + f) * count + i], f = 0..3: the return value
 * (X, or -1 when a decision fell inside the guard or the search ran past its cap), the steps taken, the bits of Uf and of px where the
 * search stopped; cells of masked lanes are left as they were.  d_marker[i] = i + 1 from every thread, behind the searches. */
int mm_debug_inversion_ladder(const double *d_U, const int32_t *d_n, const double *d_p, int64_t count, uint64_t lane_mask, int32_t *d_out,
                              int32_t *d_marker, void *stream);

/* ---- K6+K7: replay bootstrap -- numpy Generator(PCG64).multinomial draw-for-draw + replicate moments
 * replaces bootstrap._bootstrap_1d  memento/bootstrap.py:97-110 and the tuple branch of
 * estimator._hyper_1d_relative  memento/estimator.py:171-174, :182-183.
 * One lane per (gene, group) pair, one sequential PCG64 stream per lane (the reference re-seeds PCG64(5)
 * for every pair, bootstrap.py:102).  pcg_state = {state_hi, state_lo, inc_hi, inc_lo}.
 * d_slot_nobs = N_g, d_slot_omq = 1 - q_g of the slot's group.
 * Writes mean_b / var_b to d_out_mean[row*ld + 1 + b], row = d_slot_row[slot]; K == 1 pairs get NaN rows.
 * d_w_dump (optional, NULL in production) receives the int32 weights [slot][k][b] with stride kmax_dump: every k < K of an active
 * slot is written (0 behind the bin where a replicate's cells ran out), nothing else is. */
/* Optional argument of mm_boot1d_replay: tiles that are really chains of the one-wave-per-chain form (see mm_boot1d_chain, whose
 * operand records, per-chain arrays and jump table these are).  d_tile_chain[tile] = chain index or -1; a flagged tile owns no
 * bin rows (tile_ptr[t + 1] == tile_ptr[t]) and its wave runs the chain instead -- at the tile's place in the launch's dispatch
 * order, which is what the host's packing arranges. */
typedef struct mm_chain_tiles {
  const int32_t *d_tile_chain;
  const double *d_ops;
  const int64_t *d_ch_base;
  const int32_t *d_ch_K;
  const double *d_ch_nobs, *d_ch_omq;
  const int64_t *d_ch_row;
  const uint64_t *d_jump;
  int32_t *d_w_dump;
  int32_t kmax_dump;
} mm_chain_tiles;
int mm_boot1d_replay(const double *d_pk, const double *d_lq, const double *d_v, const double *d_a, const double *d_b,
                     const int64_t *d_tile_ptr, int64_t n_tiles, const int32_t *d_slot_K, const double *d_slot_nobs,
                     const double *d_slot_omq, const int64_t *d_slot_row, const uint64_t pcg_state[4], int32_t num_boot,
                     int32_t mean_only /* 1: estimator._mean_only_1p, replicates are [mean+1, 10] (estimator.py:188-204) */,
                     int64_t ld, double *d_out_mean, double *d_out_var, int32_t *d_w_dump, int32_t kmax_dump,
                     int64_t co_resident_waves /* waves of mm_boot1d_chain launched beside this call (0 = none): with n_tiles they
                                                  decide between the two- and the three-waves-per-SIMD build of the kernel */,
                     const mm_chain_tiles *chains /* NULL = every tile is a tile */, void *stream);
/* K6+K7, FREE-RUNNING tiles (memento/bootstrap.py:97-110, estimator.py:171-174; the launch the timed path uses): slot s = 64 * tile + lane
 * runs the chain whose 8-double operand records (mm_bins_order, MM_CHAIN_SLOT pairs) are [d_slot_rec[s], d_slot_rec[s] + d_slot_K[s]) of
 * d_recs; d_slot_rec[s] < 0 or d_slot_K[s] <= 0 = unused lane.  The lanes of a tile share the instruction stream only: a BTPE draw makes
 * one attempt per bin step and a rejected lane retries in the next, a lane that finishes a replicate starts its next one at once.  Same
 * draws, replicate means and variances as mm_boot1d_replay, bit for bit.  ``chains`` as there (tiles that are one-wave-per-chain chains).
 * d_w_dump (optional): int32 weights [slot][k][b], stride kmax_dump; as in mm_boot1d_replay every k < K of an active slot is written
 * (0 behind the bin where a replicate's cells ran out), nothing else is.  The weights of a tile that is a chain go to
 * chains->d_w_dump, [chain][k][b] with stride chains->kmax_dump, under mm_boot1d_chain's rule. */
int mm_boot1d_free(const double *d_recs, const int64_t *d_slot_rec, int64_t n_tiles, const int32_t *d_slot_K, const double *d_slot_nobs,
                   const double *d_slot_omq, const int64_t *d_slot_row, const uint64_t pcg_state[4], int32_t num_boot, int32_t mean_only,
                   int64_t ld, double *d_out_mean, double *d_out_var, int32_t *d_w_dump, int32_t kmax_dump, const mm_chain_tiles *chains,
                   void *stream);
/* d_out[i] = the (i + 1)-th uniform of Generator(PCG64(state)).random(): the ONE stream every chain of a launch replays
 * (memento/bootstrap.py:102 seeds PCG64(5) per pair), produced once by lane-parallel jump-ahead. */
int mm_pcg64_stream(const uint64_t pcg_state[4], int64_t n, double *d_out, void *stream);

/* K6+K7 for LONG chains: one WAVE per (gene, group) chain instead of one lane.  A chain is one sequential PCG64 stream
 * (memento/bootstrap.py:102 re-seeds PCG64(5) per pair), so nothing but the generator itself parallelises: the 64 lanes
 * produce the next 64 outputs of the stream in one step (PCG64 is an LCG: state j steps on = A^j s + C_j; d_jump[lane] =
 * {A^(lane+1) hi, lo, C_(lane+1) hi, lo} for the stream's increment) and the wave-uniform samplers consume them in order.
 * Draws, replicate means and variances are bit-identical to mm_boot1d_replay's.  Operands: 8-double records written by
 * mm_bins_order for MM_CHAIN_SLOT pairs; chain c reads records [d_ch_base[c], d_ch_base[c] + d_ch_K[c]) of d_ops, needs
 * d_ch_K[c] >= 2, and writes row d_ch_row[c].  d_w_dump (optional) receives int32 weights [chain][k][b], stride kmax_dump.  The
 * bins BEHIND the one where a replicate's cells ran out are not written (numpy stops the chain there): the caller zeroes the buffer. */
int mm_boot1d_chain(const double *d_ops, const int64_t *d_ch_base, const int32_t *d_ch_K, const double *d_ch_nobs,
                    const double *d_ch_omq, const int64_t *d_ch_row, int64_t n_chains, const uint64_t *d_jump /* [64][4] */,
                    const uint64_t pcg_state[4], int32_t num_boot, int32_t mean_only, int64_t ld, double *d_out_mean,
                    double *d_out_var, int32_t *d_w_dump, int32_t kmax_dump, void *stream);

/* K6+K7, lane-ASYNCHRONOUS tiles: one lane per chain like mm_boot1d_replay, but every lane walks its own chain at its own pace
 * (the draw is a small state machine, csrc/npy_rng.h: lane_begin / lane_inv / lane_att / ...; one pass of a wave runs each phase
 * for the lanes that are in it), so no lane waits for the longest search, the unluckiest BTPE draw or the longest chain of its
 * wave.  Slot s = 64 * wave + lane runs chain s: records [d_ch_base[s], d_ch_base[s] + d_ch_K[s]) of d_ops (the 8-double records
 * mm_bins_order writes for MM_CHAIN_SLOT pairs), row d_ch_row[s]; d_ch_K[s] < 2 = unused lane.  Same draws and replicate moments
 * as mm_boot1d_replay, bit for bit.  d_w_dump (optional): int32 weights [slot][k][b], stride kmax_dump.  As in mm_boot1d_chain the
 * bins behind the one where a replicate's cells ran out are not written: the caller zeroes the buffer.  (d_ch_row is not
 * looked at for an unused lane, and a K == 1 lane is unused here: its NaN row is the caller's.) */
int mm_boot1d_async(const double *d_ops, const int64_t *d_ch_base, const int32_t *d_ch_K, const double *d_ch_nobs,
                    const double *d_ch_omq, const int64_t *d_ch_row, int64_t n_slots, const uint64_t pcg_state[4], int32_t num_boot,
                    int32_t mean_only, int64_t ld, double *d_out_mean, double *d_out_var, int32_t *d_w_dump, int32_t kmax_dump,
                    void *stream);

/* FAST mode of K6+K7 (rng='fast'): one lane = one replicate, one wave = 64 replicates of one (gene, group) chain.  n_slots =
 * number of slots in the tile layout written by mm_bins_order (64 * n_tiles); d_slot_K[s] < 2 or d_slot_row[s] < 0 = nothing is
 * written.  Replicate r of slot s owns the PCG64 stream derived from (seed, d_slot_key[s], r) -- d_slot_row[s] addresses the output
 * row only: keys that number the chains independently of gene chunking, sharding and layout make the result independent of all
 * three.  The stream rule is part of the contract (restated in numpy in tests/_fast_ref.py): with mix64 the splitmix64 output
 * function, key = (uint64_t)d_slot_key[s] and everything mod 2^64,
 *     h = mix64(seed ^ mix64(key * 0x100000001B3 + r))
 *     state = (mix64(h), mix64(h + 1))     increment = (mix64(h + 2), mix64(h + 3) | 1)          (high word, low word)
 * is a plain PCG64 (the XSL-RR 128/64 generator of numpy), and the weights of replicate r are, draw for draw, what numpy's
 * Generator(PCG64 set to that state and increment).multinomial(n, multiplicities / n) returns.  Same sampler code and moment
 * arithmetic as the replay kernel: the draws are not those of the reference's single stream PCG64(seed) -- the results are
 * statistically equivalent to the reference's -- but they are numpy's own on the stated per-replicate stream.
 * d_w_dump (optional, NULL in production): int32 weights [slot][k < kmax_dump][r < num_boot]. */
int mm_boot1d_fast(const double *d_pk, const double *d_lq, const double *d_v, const double *d_a, const double *d_b,
                   const int64_t *d_tile_ptr, int64_t n_slots, const int32_t *d_slot_K, const double *d_slot_nobs,
                   const double *d_slot_omq, const int64_t *d_slot_row, const int64_t *d_slot_key, uint64_t seed, int32_t num_boot,
                   int32_t mean_only, int64_t ld, double *d_out_mean, double *d_out_var, int32_t *d_w_dump, int32_t kmax_dump,
                   void *stream);

/* mm_boot1d_fast on a replicate RANGE (sequential bootstrap, ht_1d_vs_control(max_boot=...)): local replicate i in [0, rep_n)
 * draws from the stream of global replicate rep_lo + i -- (seed, d_slot_key[s], rep_lo + i) -- and is stored in column 1 + i of
 * row d_slot_row[s]; ld >= 1 + rep_n; d_w_dump (optional) is [slot][k < kmax_dump][i < rep_n].  mm_boot1d_fast is the case
 * rep_lo = 0, rep_n = num_boot of the same kernel, so replicates [rep_lo, rep_lo + rep_n) made later, for some of the chains,
 * are bit for bit those of a one-shot launch over [0, rep_lo + rep_n).
 *   - rep_lo >= 0, rep_n >= 1 and rep_lo + rep_n <= 2^31 - 1.
 *   - The stream seed is a function of key * 0x100000001B3 + r (mod 2^64): distinct (key, r) with 0 <= r < 2^31 (below the key
 *     multiplier 0x100000001B3) and 0 <= key < 2^64 / 0x100000001B3 (= 2^24 - 1 at most; the sum does not wrap there) give distinct
 *     values, so no replicate range of one chain collides with a range of another chain.
 *   - A slot with d_slot_row[s] < 0 (or d_slot_K[s] < 2) writes nothing, as in mm_boot1d_fast: that is how the chains of closed
 *     tests are skipped without a new tile layout.
 *   - Column 0, the columns beyond rep_n and the rows of skipped slots are not written.
 * The caller (memento.ht_1d_vs_control(rng='fast', max_boot=N, min_extreme=M)): every test gets num_boot replicates, and a test
 * whose extreme count is still <= min_extreme goes on to the totals 2, 4, ... x num_boot, at most max_boot.  The 8-double test
 * records of the rounds fold into one (counts add, mean and se pool), p = (c + 1) / (n + 1) over all rounds and no tail fit is
 * made.  mm_boot_fill_log runs per round on the round's own planes: an invalid replicate is refilled from the valid replicates
 * of the same round, with a refill seed derived from (fill_seed, round) -- uniform over valid replicates like the one-shot
 * refill, statistically equivalent to it, identical where nothing is refilled. */
int mm_boot1d_fast_range(const double *d_pk, const double *d_lq, const double *d_v, const double *d_a, const double *d_b,
                         const int64_t *d_tile_ptr, int64_t n_slots, const int32_t *d_slot_K, const double *d_slot_nobs,
                         const double *d_slot_omq, const int64_t *d_slot_row, const int64_t *d_slot_key, uint64_t seed, int32_t rep_lo,
                         int32_t rep_n, int32_t mean_only, int64_t ld, double *d_out_mean, double *d_out_var, int32_t *d_w_dump,
                         int32_t kmax_dump, void *stream);

/* ---- K8: residual variance, invalid-replicate fill, log  ---------------------------------------
 * replaces estimator._residual_variance + hypothesis_test._fill + np.log
 *   memento/estimator.py:103-111, memento/hypothesis_test.py:186-197.
 * In place on rows [n_rows][ld]; column 0 (true values, already logged by the host) is left alone.
 * fill_mode 0: replace invalid entries by a uniformly chosen valid replicate using a counter-based
 *   RNG (own stream: statistically equivalent to np.random.choice, not the same draws);
 * fill_mode 1: leave invalid entries as NaN (the strict host driver patches them with np.random).
 * d_n_invalid[row][2] = number of invalid (mean, res_var) replicates; a row with no valid entry is
 * reported as -1.
 * The draw rule of fill_mode 0 (restated in numpy in tests/_replicate_ref.py).  mix() is the splitmix64 output function
 * (x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31), all
 * arithmetic is uint64.  Invalid replicate r (0-based, stored in column r + 1) of plane p (0 mean, 1 res_var) of the row with
 * key k (d_row_key[row], or the row number) starts from c = mix(fill_seed ^ mix(2 k + p) ^ (r << 20)) and makes up to 4096
 * attempts a = 0, 1, ...: c = mix(c + a), index = c mod num_boot; the first index that is an originally valid replicate of that
 * plane is taken.  If all 4096 miss (probability (1 - V / num_boot)^4096 with V valid replicates), the entry takes the valid
 * replicate of rank mix(~c0) mod V in ascending position, c0 being the starting value above.  So every invalid entry of a plane
 * with V >= 1 is filled, uniformly over the V valid ones; a plane with V = 0 stays NaN. */
int mm_boot_fill_log(double *d_mean, double *d_var, int64_t n_rows, int64_t ld, int32_t num_boot, const double mv_fit[3],
                     int32_t fill_mode, uint64_t fill_seed, int32_t *d_n_invalid,
                     const int64_t *d_row_key /* optional [n_rows]: the refill stream of a row is keyed by this instead of the row
                                                 number, so that it is the same however the rows were chunked / sharded */,
                     void *stream);

/* ---- K9+K10: per-test linear contraction over groups and null statistics ------------------------
 * replaces hypothesis_test._regress_1d (linear part) and the counting part of _compute_asl
 *   memento/hypothesis_test.py:249-251, :262-271, :290-298, :62-92.
 * test t: rows of gene test_gene[t] are [gene*n_groups + j]; coef_b = sum_j W[t][j] * y[row_j][b] over
 * good groups (d_good[gene][j] != 0); replicate b is dropped if any good row is non-finite in either
 * d_ym or d_yv (valid_boostrap_iters).  which = 0 uses d_ym, 1 uses d_yv as the response.
 * d_coef[t][ld] receives the coefficient row (NaN where dropped); d_stats[t][8] =
 *   {coef0, se (nanstd, ddof 0), n_valid_null, extreme_count, null_mean, all_equal, extreme_count_raw, range}:
 *   extreme_count / null_mean are those of null = coef[1:] - coef[0] (resampling == 'bootstrap', :66-68),
 *   extreme_count_raw counts |coef[b]| > |coef0| on the un-centred replicates (any other resampling value, :69-70; their
 *   mean is null_mean + coef0); range = max - min over all columns. */
int mm_contract_stats(const double *d_ym, const double *d_yv, int64_t ld, int32_t num_boot, int32_t n_groups,
                      const int32_t *d_test_gene, const double *d_W /* [n_tests][n_groups] */, const uint8_t *d_good /* [n_genes][n_groups] */,
                      int64_t n_tests, int32_t which, double *d_coef, double *d_stats, void *stream);

/* ---- resample_rep=True: hierarchical resampling of replicate groups ------------------------------------
 * replaces hypothesis_test._regress_1d :249-254, :273-286, _regress_2d :372-377, :393-404 and _cross_coef_resampled :231-239.
 * mm_valid_cols: the replicate columns that survive valid_boostrap_iters (:249-251): d_col_map[gene][k] = k-th column in
 * which every good group is finite in BOTH d_ym and d_yv (pass the same pointer twice for the 2D correlation rows),
 * d_n_valid[gene] = their number.  d_col_map is [n_genes][num_boot + 1]; entries beyond d_n_valid[gene] are unspecified.
 * num_boot = 0 (column 0 alone) is accepted.
 * mm_residualize: d_dst = M d_src on the [n_genes*n_groups][ld] rows (columns 0..n_cols-1; d_dst must not alias d_src);
 * gene g uses the n_groups x n_groups matrix d_M[d_gene_mask[g]] (zero rows/columns on invalid groups -> NaN rows).
 * Any number of groups (one group per donor: analysis/lupus/run_memento.py:31-52). */
int mm_valid_cols(const double *d_ym, const double *d_yv, int64_t ld, int32_t num_boot, int32_t n_groups, const uint8_t *d_good,
                  int64_t n_genes, int32_t *d_col_map, int32_t *d_n_valid, void *stream);
int mm_residualize(const double *d_src, double *d_dst, int64_t ld, int32_t n_cols, int32_t n_groups, int64_t n_genes,
                   const int32_t *d_gene_mask, const double *d_M, void *stream);
/* mm_cross_resampled: coefficient of resampled column c < nb (column 0 = observed), nb = d_n_valid[gene] - 1 (num_boot when
 * d_col_map / d_n_valid are NULL).  d_tt[test][group] = residualised treatment; d_rep/d_bcol [gene][n_groups][num_boot] =
 * group index (into the gene's valid groups) and index (1..nb, into the surviving columns) of the replicate column drawn for
 * row i of column c (np.random.choice replay), or both NULL to draw them on the device.  Columns whose drawn groups all share
 * one treatment value (0/0 in the reference) are reported as NaN.
 * The device draws (d_rep == NULL; restated in numpy in tests/_replicate_ref.py), with mix() the splitmix64 output function as
 * in mm_boot_fill_log and uint64 arithmetic: row i (position among the n good groups of gene g = d_test_gene[t]) of column
 * c >= 1 takes h = mix(seed ^ mix((g << 32) ^ (i << 24) ^ c)), group r = h mod n and surviving column bb = mix(h) mod nb + 1;
 * column 0 is the identity (r = i, bb = 0).  The draws depend on the gene, not on the test.  The packing keeps (g, i, c)
 * apart for i < 256 and c < 2^24; from 256 good groups on the bits of i run into those of g, so distinct (g, i) can share a
 * stream (left as is: repacking would move every device-drawn result). */
int mm_cross_resampled(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_gene,
                       const double *d_tt, const uint8_t *d_good, const double *d_Nc, const int16_t *d_rep, const int32_t *d_bcol,
                       const int32_t *d_col_map, const int32_t *d_n_valid, uint64_t seed, int64_t n_tests, double *d_coef,
                       double *d_stats, void *stream);
/* mm_cross_resampled with a KEY per gene: d_gene_key [n_genes] (int64) replaces g in the draw rule above,
 *   h = mix(seed ^ mix((key << 32) ^ (i << 24) ^ c)),
 * so that the draws of a gene do not depend on the slot it has in a chunk of genes (keys below 2^32 stay apart); NULL = the slot,
 * which is mm_cross_resampled itself. */
int mm_cross_resampled_keyed(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_gene,
                             const double *d_tt, const uint8_t *d_good, const double *d_Nc, const int16_t *d_rep, const int32_t *d_bcol,
                             const int32_t *d_col_map, const int32_t *d_n_valid, const int64_t *d_gene_key, uint64_t seed,
                             int64_t n_tests, double *d_coef, double *d_stats, void *stream);
/* mm_cross_resampled_block: the records of mm_cross_resampled_keyed for tests that arrive GENE-MAJOR (many cis SNPs per gene:
 * analysis/lupus/run_memento.py:84-109), without the coefficient rows.  The tests of gene slot g are the rows
 * [d_gene_ptr[g], d_gene_ptr[g + 1]) of d_tt [n_tests][n_groups]; d_gene_ptr [n_genes + 1] is a CSR pointer over the n_tests tests and
 * max_gene_tests >= the largest number of tests of a gene (it sizes the launch: tests of a gene beyond it would get no record).
 * Everything else -- d_good, d_Nc, d_rep / d_bcol (or NULL: device draws), d_col_map / d_n_valid, d_gene_key (or NULL: the slot),
 * the draw rule with the key, the degenerate-column rule -- is as in mm_cross_resampled_keyed, and for every (test, column) the
 * operations and their order are that kernel's: d_stats [n_tests][8] equals the record it writes for the same test, gene and key.
 * A workgroup takes 8 consecutive tests of one gene and obtains every draw of a column once for all of them; nothing
 * per replicate is stored (the record's second pass computes the coefficients again), so the call's memory is the records.  The
 * rows of the few tests that need them come from mm_cross_resampled_keyed on that subset.  A gene without tests costs nothing; a
 * gene without a good group, or with fewer than two surviving columns, gives NaN records.  LDS: 76 bytes per group (n_groups <= 860).
 * The tables are trusted: validate them on the host (engine.cross_resampled_block). */
int mm_cross_resampled_block(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_gene_ptr,
                             int64_t n_genes, int32_t max_gene_tests, const double *d_tt, const uint8_t *d_good, const double *d_Nc,
                             const int16_t *d_rep, const int32_t *d_bcol, const int32_t *d_col_map, const int32_t *d_n_valid,
                             const int64_t *d_gene_key, uint64_t seed, int64_t n_tests, double *d_stats, void *stream);
/* A COVARIATE PER TEST for the gene-major tests (ht_1d_eqtl(interaction=): the genotype main effect beside the tested
 * genotype x context).  d_zt [n_tests][n_groups] holds z = M g, the covariate residualised on the shared design like the response;
 * residualising on [shared | g] is then the rank-one step
 *   y_t[j][c] = y[j][c] - z[j] * beta[c],   beta[c] = sum_j Nc_j z_j y[j][c] / sum_j Nc_j z_j^2   (good groups, ascending; a zero
 * denominator -- z == 0: the host found g inside the shared span -- gives beta = 0).  The tiles are those of
 * mm_cross_resampled_block, numbered gene-major: tile = gene * ceil(max_gene_tests / 8) + (tile of 8 tests within the gene), and
 * the entry points take a RANGE [tile_lo, tile_hi) of them so that the caller bounds the scratch d_beta
 * [tile_hi - tile_lo][ld][8] doubles (test-minor: a draw reads one 64-byte line); a tile past its gene's last test leaves its
 * block unwritten.  mm_cross_cov_beta writes beta for the columns 0..num_boot of the range (columns across threads, the weights in
 * LDS).  mm_cross_resampled_block_cov launches it and then, on the same stream, the record kernel, which is
 * mm_cross_resampled_block with test k of a tile reading y - z_k * beta_k: d_stats gets the records of the tests of the range's
 * tiles and no other record is touched.  LDS: 140 bytes per group (n_groups <= 468).  d_zt == 0 gives the records of
 * mm_cross_resampled_block bit for bit.  mm_residualize_rank1 materialises y_t for a LIST of tests (test l of gene d_test_gene[l],
 * covariate row l of d_zt [n_list][n_groups]) into d_out [n_list][n_groups][ld] (columns 0..num_boot; NaN on the groups that are
 * not good) with the same weights, beta and subtraction (the library is built with -ffp-contract=off):
 * mm_cross_resampled_keyed on d_out, test l on row block l with the tables of its gene, gives the coefficient rows of the record
 * kernel bit for bit.  The tables are trusted: validate them on the host (engine.cross_resampled_block(zt=...)). */
int mm_cross_cov_beta(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_gene_ptr, int64_t n_genes,
                      int32_t max_gene_tests, const double *d_zt, const uint8_t *d_good, const double *d_Nc, int64_t n_tests,
                      int64_t tile_lo, int64_t tile_hi, double *d_beta, void *stream);
int mm_cross_resampled_block_cov(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_gene_ptr,
                                 int64_t n_genes, int32_t max_gene_tests, const double *d_tt, const double *d_zt, const uint8_t *d_good,
                                 const double *d_Nc, const int16_t *d_rep, const int32_t *d_bcol, const int32_t *d_col_map,
                                 const int32_t *d_n_valid, const int64_t *d_gene_key, uint64_t seed, int64_t n_tests, int64_t tile_lo,
                                 int64_t tile_hi, double *d_beta, double *d_stats, void *stream);
int mm_residualize_rank1(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_gene,
                         const double *d_zt, const uint8_t *d_good, const double *d_Nc, int64_t n_list, double *d_out, void *stream);
/* mm_cross_resampled_family: single-step max-T over the resampled tests of every gene, on ONE response plane -- the family of gene
 * slot g is its tests [d_gene_ptr[g], d_gene_ptr[g + 1]), whose replicate slot c is one joint draw because the draws are keyed by
 * the gene.  The tables are those of mm_cross_resampled_block (max_gene_tests is checked and otherwise unused); d_stats [n_tests][8]
 * are the records that call wrote for this plane, of which only coef0 = d_stats[t][0] is read, and d_scale [n_tests] is 1 / se, or 0
 * for a member without a test (engine.family_scale of the records).  The resampled row of a gene has the slots 0..nb - 1, nb =
 * d_n_valid[g] - 1 (num_boot without d_n_valid): slot 0 is the observed coefficient, 1..nb - 1 the replicates of the record.
 *   member j is INCLUDED when scale_j is finite and > 0 and coef0_j is finite;  t0_j = |coef0_j| * scale_j, NaN if not;
 *   slot c >= 1 is FAMILY-VALID when the coefficient of every included member is not NaN there (the degenerate-column rule of
 *   mm_cross_resampled, member by member);  M[c] = max_j |coef_j[c] - coef0_j| * scale_j over the included members, j ascending;
 *   n_adj_j = #{family-valid c : M[c] > t0_j}  (NaN on either side is not counted).
 * Every coefficient comes from the operations of mm_cross_resampled_keyed in their order (the tile routine of the block kernel),
 * so M equals that rule applied in numpy to the rows mm_cross_resampled_keyed returns, bit for bit.
 * Outputs: d_maxrow [n_genes][ld] = M (NaN at slot 0, at invalid slots and at nb..num_boot; cells past num_boot are not written);
 * d_adj [n_tests][2] = (t0, n_adj), (NaN, 0) for a member that is not included; d_fam [n_genes][2] = (n_valid_family, n_included).
 * A gene without tests, without a good group, with nb < 1 or without an included member gives an all-NaN row, (0, 0) and (NaN, 0).
 * Two kernels: (gene, slab of ``slab`` slots) workgroups in which a thread owns a slot and walks the gene's tiles of 8 tests,
 * evaluating each (test, slot) once, then one workgroup per gene for the counts.  slab = 0: the default (256); no output depends
 * on it.  LDS: 76 bytes per group + 128 (n_groups <= 860).  The tables are trusted: validate them on the host
 * (engine.cross_resampled_block). */
int mm_cross_resampled_family(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_gene_ptr,
                              int64_t n_genes, int32_t max_gene_tests, const double *d_tt, const uint8_t *d_good, const double *d_Nc,
                              const int16_t *d_rep, const int32_t *d_bcol, const int32_t *d_col_map, const int32_t *d_n_valid,
                              const int64_t *d_gene_key, uint64_t seed, int64_t n_tests, const double *d_stats, const double *d_scale,
                              int32_t slab, double *d_maxrow, double *d_adj, double *d_fam, void *stream);

/* ---- guide-vs-control contrasts: sparse weight rows over the replicate groups ------------------------------------
 * test t: coef_c = sum_p design_w[p] * y[test_gene[t], design_grp[p]][c] over p in [design_ptr[d], design_ptr[d + 1]),
 * d = test_design[t] -- the per-guide weighted regression of _regress_1d (hypothesis_test.py:242-300) on the guide's and
 * the control's stratum groups, folded into one sparse weight row per design (memento/design.py).  Column c counts only
 * if the mean and the variability rows of every listed group are finite there; if column 0 does not, coef0 is NaN on both
 * planes.  An empty design gives a NaN test.  stats layout as mm_contract_stats, for the mean and the variability response in
 * one launch; nothing per-replicate is stored.
 * The plain two-group test against a shared control (Perturb-seq batching) is the two-entry design
 * {(guide, +1.0), (control, -1.0)}: coef_b = y[gene, guide][b] - y[gene, control][b] -- what _regress_1d computes for the two
 * groups {control, guide} with a binary treatment (hypothesis_test.py:269-291); the control's bootstrap is shared by all guides
 * instead of being recomputed per guide as in the reference's per-guide loop.  The sums are unfused and start from 0.0, so
 * the coefficient is that difference bit for bit, an exact zero always being +0.0 (engine._contrast builds these tables). */
int mm_contrast_design_stats(const double *d_ym, const double *d_yv, int64_t ld, int32_t num_boot, int32_t n_groups,
                             const int32_t *d_test_gene, const int32_t *d_test_design, const int32_t *d_design_ptr,
                             const int32_t *d_design_grp, const double *d_design_w, int64_t n_tests, double *d_stats_mean,
                             double *d_stats_var, void *stream);
/* coefficient rows [n_tests][ld] of selected design contrasts (NaN where a replicate column is not valid) */
int mm_contrast_design_rows(const double *d_ym, const double *d_yv, int64_t ld, int32_t num_boot, int32_t n_groups,
                            const int32_t *d_test_gene, const int32_t *d_test_design, const int32_t *d_design_ptr,
                            const int32_t *d_design_grp, const double *d_design_w, int64_t n_tests, int32_t which, double *d_out,
                            void *stream);

/* Guide-vs-control contrasts on ONE response plane d_y (the replicate correlations of the 2D bootstrap, rows
 * [pair * n_groups + group][ld]): test t applies the sparse weight row of design d_test_design[t] to the rows of pair
 * d_test_row[t], coef_c = sum_p d_design_w[p] * y[d_test_row[t] * n_groups + d_design_grp[p]][c].  A plain two-group
 * test is the design {(guide, +1), (control, -1)}; an empty design gives a NaN test.  Column c counts only if every
 * listed group is finite there.  The index tables are trusted: validate them on the host.  d_stats [n_tests][8], layout
 * as mm_contract_stats. */
int mm_contrast_design1_stats(const double *d_y, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_row,
                              const int32_t *d_test_design, const int32_t *d_design_ptr, const int32_t *d_design_grp,
                              const double *d_design_w, int64_t n_tests, double *d_stats, void *stream);
/* coefficient rows [n_tests][ld] of selected single-plane design contrasts (NaN where a replicate column is not valid) */
int mm_contrast_design1_rows(const double *d_y, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_row,
                             const int32_t *d_test_design, const int32_t *d_design_ptr, const int32_t *d_design_grp,
                             const double *d_design_w, int64_t n_tests, double *d_out, void *stream);

/* ---- single-step max-T adjustment over families of design contrasts (ht_1d_posthoc) ---------------------------------
 * Family f is the tests [family_ptr[f], family_ptr[f + 1]) of the test arrays: consecutive, sharing one row block
 * d_test_gene, each with its design as in mm_contrast_design_stats (coef_j[c] through the same routine: p ascending, unfused).
 * d_scale [test][2] (mean, variability plane): 1 / se of the member's record, or 0 for a member without a test.  Per plane,
 * member j is INCLUDED when its scale is a finite number > 0 and its column 0 is valid; column c >= 1 is FAMILY-VALID when every
 * included member is valid at c (every listed group finite in BOTH planes).  Over the family-valid columns and the included
 * members, j ascending:
 *   M[c] = max_j |coef_j[c] - coef_j[0]| * scale_j,   t0_j = |coef_j[0]| * scale_j,   n_adj_j = #{ c : M[c] > t0_j }   (strict)
 * so that p_adj_j = (1 + n_adj_j) / (1 + n_valid_family) is the single-step max-T (Westfall-Young) adjusted p-value of member j
 * within its family.  Outputs:
 *   d_maxrow [n_fam][2][ld]   M, NaN in column 0 and in the columns that are not family-valid; the padding beyond num_boot is
 *                             not written (mm_row_quantiles on these rows gives the critical value of the simultaneous interval)
 *   d_adj    [n_tests][2][2]  (t0, n_adj); (NaN, 0) for a member that is not included
 *   d_fam    [n_fam][2][2]    (n_valid_family, n_included); an empty family or one without an included member has (0, 0) and
 *                             an all-NaN row
 * coef_j[0] and scale_j of a family's first stage_cap members (0 <= stage_cap <= 1024) are staged in LDS, those of the members
 * beyond come back from global memory: the outputs are the same bit for bit.  One workgroup per family; n_fam == 0 is a no-op.
 * The tables are trusted: validate them on the host (engine._family_tables). */
int mm_family_maxt(const double *d_ym, const double *d_yv, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_family_ptr,
                   const int32_t *d_test_gene, const int32_t *d_test_design, const int32_t *d_design_ptr, const int32_t *d_design_grp,
                   const double *d_design_w, const double *d_scale, int32_t stage_cap, int64_t n_fam, double *d_maxrow, double *d_adj,
                   double *d_fam, void *stream);
/* the same adjustment on ONE response plane (the replicate correlations of Bootstrap2D: ht_2d_posthoc), with the tables of
 * mm_contrast_design1_stats: d_scale [n_tests][1], d_maxrow [n_fam][ld], d_adj [n_tests][1][2] (t0, n_adj), d_fam [n_fam][1][2]
 * (n_valid_family, n_included).  A column is valid for a member when every listed group is finite there in this plane; everything
 * else -- inclusion, family-valid columns, the order of the maximum, stage_cap, the cells that are written -- as above. */
int mm_family_maxt1(const double *d_y, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_family_ptr,
                    const int32_t *d_test_row, const int32_t *d_test_design, const int32_t *d_design_ptr, const int32_t *d_design_grp,
                    const double *d_design_w, const double *d_scale, int32_t stage_cap, int64_t n_fam, double *d_maxrow, double *d_adj,
                    double *d_fam, void *stream);

/* ---- joint test of a block of treatment columns (ht_1d_joint) ------------------------------------------------------
 * test t applies the r = design_rank[d] linear forms of design d = test_design[t] to every replicate column of gene
 * test_gene[t]: L [r][n_d] row-major at d_design_L + design_lofs[d], over the n_d groups
 * design_grp[design_ptr[d] .. design_ptr[d + 1]) (memento/design.py: joint_rows), and reduces
 *   Q_0 = ||L y_0||^2  and, for the replicate columns c = 1..num_boot,  Q*_c = ||L y_c - L y_0||^2  (the centred bootstrap null)
 * for the mean and the variability plane in one launch.  The record, 8 doubles per test and plane (NOT the layout of
 * mm_contract_stats):
 *   [0] Q_0   [1] population sd of Q* over the valid columns   [2] n_valid   [3] n_extreme = #{ Q*_c > Q_0 } (strict)
 *   [4] mean of Q*   [5] all_equal: 1 when every valid Q*_c is exactly 0   [6] max of Q*   [7] r
 * ([1], [4], [6] are NaN and [5] is 0 when n_valid == 0).  Column c is valid only if every listed group is finite there in
 * BOTH planes.  An invalid column 0, an empty design and r = 0 give the NaN record of mm_contract_stats on both planes
 * ([2], [3], [5] zero, the rest NaN).  A form sums its groups in ascending p, Q sums its forms in ascending k, unfused; L is
 * staged in LDS when r * n_d <= 4096 doubles and read through the cache otherwise, with the same arithmetic.  Nothing
 * per-replicate is stored.  The tables are trusted -- validate them on the host: every design needs
 * 0 <= r <= n_d <= n_groups, group indices in [0, n_groups), r * n_d doubles at design_lofs[d], and every test a gene slot of
 * the planes.  Needs n_groups <= 2048 (z_0 of both planes and the staged L share 64 KB of LDS). */
int mm_joint_stats(const double *d_ym, const double *d_yv, int64_t ld, int32_t num_boot, int32_t n_groups,
                   const int32_t *d_test_gene, const int32_t *d_test_design, const int32_t *d_design_ptr,
                   const int32_t *d_design_rank, const int64_t *d_design_lofs, const int32_t *d_design_grp,
                   const double *d_design_L, int64_t n_tests, double *d_stats_mean, double *d_stats_var, void *stream);
/* The same test on ONE response plane (the replicate correlations of Bootstrap2D, ht_2d_joint): test t applies design
 * test_design[t] to the rows of row block test_row[t] of d_y [row block][group][ld] (a row block is a pair, in device pair
 * order) and writes ONE joint record, d_stats [n_tests][8], in the layout above:
 *   [0] Q_0   [1] population sd of Q*   [2] n_valid   [3] n_extreme   [4] mean of Q*   [5] all_equal   [6] max of Q*   [7] r
 * Column c is valid only if every listed group is finite there; an unlisted group is never read.  An invalid column 0, an
 * empty design and r = 0 give the NaN record.  The design tables, the arithmetic and its order, the staging of L and the
 * trust in the tables are those of mm_joint_stats: the record equals, bit for bit, the mean-plane record of mm_joint_stats
 * given the plane as both d_ym and d_yv, at one read of every operand and one evaluation of every form.  Needs
 * n_groups <= 4096 (z_0 and the staged L share 64 KB of LDS). */
int mm_joint1_stats(const double *d_y, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_row,
                    const int32_t *d_test_design, const int32_t *d_design_ptr, const int32_t *d_design_rank,
                    const int64_t *d_design_lofs, const int32_t *d_design_grp, const double *d_design_L, int64_t n_tests,
                    double *d_stats, void *stream);

/* ---- order statistics of replicate rows (percentile intervals of the coefficients) -------------------------------
 * For every row of d_rows [n_rows][ld]: the replicate columns 1..num_boot (column 0, the observed value, and the padding
 * from num_boot + 1 on are not read), NaNs dropped; d_n_valid[row] = n, the number of columns kept, and
 *   d_out[row][k] = np.nanquantile(row[1 : num_boot + 1], probs[k])   (numpy's default method, 'linear'):
 * with x_(0) <= ... <= x_(n-1) the kept values, h = probs[k] * (n - 1), a = x_(floor h), b = x_(min(floor h + 1, n - 1)) and
 * t = h - floor h, the result is a + (b - a) * t for t < 0.5 and b - (b - a) * (1 - t) otherwise (numpy's _lerp, unfused);
 * t == 0 or a == b gives a itself (the same number wherever the formula is finite; an order statistic that is +-inf comes
 * out as +-inf, where the formula has inf - inf).  n == 0 gives NaN.  +-inf are ordinary values at the ends of the order;
 * which of -0.0 and +0.0 comes out is not specified (numpy's sort does not order them either).
 * probs: HOST array of n_probs values in [0, 1], 1 <= n_probs <= 8.  Needs num_boot >= 1 and ld >= num_boot + 1; n_rows == 0
 * is a no-op.  The selection is an exact radix select on the row in place (8 reads of the row, nothing stored): ties and rows
 * of any length are handled by the same path. */
int mm_row_quantiles(const double *d_rows, int64_t n_rows, int64_t ld, int32_t num_boot, const double *probs, int32_t n_probs,
                     double *d_out /* [n_rows][n_probs] */, int32_t *d_n_valid /* [n_rows] */, void *stream);

/* ==== 2D (gene pairs) ===========================================================================
 * K11 step 1: copy the columns of the n_cols genes with d_col_id[gene] = m >= 0 out of the SELL blocks into a
 * gene-contiguous store: entries of (block b, column m) at d_out[col_ptr[b*(n_cols+1)+m] .. col_ptr[b*(n_cols+1)+m+1])
 * (same packed uint32 entries; order inside a column is the storage order of the block). */
int mm_extract_cols(const uint32_t *d_ent, const int64_t *d_blk_base, const int32_t *d_slice_w, const int32_t *d_slice_ptr,
                    const int32_t *d_item_ptr, const int32_t *d_perm, int32_t n_blocks, int32_t n_genes, const int32_t *d_col_id,
                    int32_t n_cols, const int64_t *d_col_ptr /* [nb][n_cols+1] */, uint32_t *d_out, void *stream);
/* K11 step 2: prod[group][pair] = sum_c x_ci x_cj / sf_c^2
 * replaces estimator._hyper_cov_relative sparse branch (X.multiply(Y).sum)  memento/estimator.py:225-228
 * and the Gram product of _hyper_corr_symmetric  memento/estimator.py:253-255.
 * Pairs are grouped by their left column: left l owns pairs [left_ptr[l], left_ptr[l+1]), right_col[pair] = partner
 * column.  d_scratch: [n_blocks][n_pairs] fp64; d_out: [n_groups][n_pairs]. */
int mm_pair_cross(const uint32_t *d_cols, const int64_t *d_col_ptr, int32_t n_cols, const int32_t *d_blk_cell0,
                  const int32_t *d_grp_blk0, int32_t n_blocks, int32_t n_groups, const double *d_inv_sf, const int32_t *d_left_col,
                  const int64_t *d_left_ptr, int32_t n_left, const int32_t *d_right_col, int64_t n_pairs, double *d_scratch,
                  double *d_out, void *stream);
/* 2D histograms: table of q = pair*n_groups + group is [n_sf_bins][xcap_i[q]][xcap_j[q]] uint32 at tab_ptr[q] (zeroed
 * by the caller); counts the cells with x_j > 0.  replaces np.unique over two columns, memento/bootstrap.py:62-71 */
int mm_pair_hist(const uint32_t *d_cols, const int64_t *d_col_ptr, int32_t n_cols, const int32_t *d_blk_cell0,
                 const int32_t *d_blk_group, int32_t n_blocks, const uint8_t *d_sf_bin, const int32_t *d_left_col,
                 const int64_t *d_left_ptr, int32_t n_left, const int32_t *d_right_col, int32_t n_groups, const int64_t *d_tab_ptr,
                 const int32_t *d_xcap_i, const int32_t *d_xcap_j, uint32_t *d_tab, void *stream);
/* x_j == 0 column from the left gene's 1D table (d_hist_i + hist_ptr[q], [n_sf_bins][xcap_i[q]], as completed by
 * mm_bins_count) and the number of non-empty bins K[q]. */
int mm_pair_bins_count(uint32_t *d_tab, const int64_t *d_tab_ptr, const int32_t *d_xcap_i, const int32_t *d_xcap_j,
                       const uint32_t *d_hist_i, const int64_t *d_hist_ptr, int64_t n_q, int32_t n_sf_bins, int32_t *d_K,
                       void *stream);
/* replay order of the 2D bins: code = x_i*r1a + x_j*r1b + r0*approx_sf (bootstrap.py:62-65, two-column expr);
 * big = 0: K <= 1024, big = 1: K <= 4096 */
int mm_bins_order2d(const uint32_t *d_tab, const int64_t *d_tab_ptr, const int32_t *d_xcap_i, const int32_t *d_xcap_j,
                    const int32_t *d_K, const int64_t *d_pair_list, int64_t n_list, int32_t big, int32_t n_groups, int32_t n_sf_bins,
                    const double *d_sf_table, const double *d_r1a, const double *d_r1b, const double *d_r0,
                    const int64_t *d_pair_slot, const int64_t *d_tile_ptr, const double *d_grp_ncells, double *d_pk, double *d_lq,
                    double *d_v1, double *d_v2, double *d_a, double *d_b, int32_t *d_status, void *stream);
/* 2D replay bootstrap: replicate covariance + the two variances folded into the correlation
 * replaces bootstrap._bootstrap_2d + estimator._corr_from_cov   memento/bootstrap.py:119-157, estimator.py:273-292
 * Slot s = 64 * tile + lane reads bin k of its chain at [d_tile_ptr[tile] + k][lane] of the six planes; d_slot_K[s] <= 0 or
 * d_slot_row[s] < 0 = unused lane (it reads its tile's first row and stores nothing).  A K == 1 chain is replayed like any other
 * (the reference has no shortcut for it in 2D, unlike mm_boot1d_replay's NaN row): its one bin takes every cell, a variance is
 * <= 0 and every replicate is the clipped sentinel 1.0.  Replicate b of an active slot goes to d_out_corr[row * ld + 1 + b],
 * b < num_boot; nothing outside [row][1 .. num_boot] of the active slots' rows is written (column 0 and the columns behind
 * num_boot are the caller's; ld >= num_boot + 1).  0 <= n_tiles < 2^31 - 1; n_tiles == 0 launches nothing. */
int mm_boot2d_replay(const double *d_pk, const double *d_lq, const double *d_v1, const double *d_v2, const double *d_a,
                     const double *d_b, const int64_t *d_tile_ptr, int64_t n_tiles, const int32_t *d_slot_K,
                     const double *d_slot_nobs, const double *d_slot_omq, const int64_t *d_slot_row, const uint64_t pcg_state[4],
                     int32_t num_boot, int64_t ld, double *d_out_corr, void *stream);

/* The same replay with per-chain operand RECORDS instead of shared rows: slot s = 64 * tile + lane runs the chain whose 8-double records
 * (mm_bins_order2d for pairs given as d_pair_slot[q] = MM_CHAIN_SLOT | first record: pk, lq, x_i, x_j, 1/sf, 1/sf^2, two spare) are
 * [d_slot_rec[s], d_slot_rec[s] + d_slot_K[s]) of d_recs; d_slot_rec[s] < 0 = unused lane.  A lane then reads memory of its own whatever
 * bin it is on, so a BTPE draw can make one attempt per bin step and retry in the next (as mm_boot1d_replay does).  Same draws and
 * replicate correlations as mm_boot2d_replay, bit for bit.   memento/bootstrap.py:119-157, estimator.py:273-292
 * Unused lanes: d_slot_K[s] <= 0, d_slot_row[s] < 0 or d_slot_rec[s] < 0 -- such a lane reads record 0 at most and stores nothing.
 * K == 1 chains, the cells written (only [row][1 .. num_boot] of the active slots' rows) and the n_tiles limit (< 2^31 - 1) as
 * in mm_boot2d_replay. */
int mm_boot2d_replay_rec(const double *d_recs, const int64_t *d_slot_rec, int64_t n_tiles, const int32_t *d_slot_K,
                         const double *d_slot_nobs, const double *d_slot_omq, const int64_t *d_slot_row, const uint64_t pcg_state[4],
                         int32_t num_boot, int64_t ld, double *d_out_corr, void *stream);

/* FAST mode of the 2D bootstrap (rng='fast'): one lane = one replicate, one wave = 64 replicates of one (pair, group) chain, read
 * from the six [row][64] operand planes mm_bins_order2d writes for plain tile slots (n_slots = 64 * n_tiles, slot s = 64 * tile +
 * lane; d_slot_K[s] <= 0 or d_slot_row[s] < 0 = unused).  Replicate r of slot s owns the PCG64 stream derived from
 * (seed, d_slot_key[s], r): keys that number the chains independently of chunking and layout make the result independent of both.
 * The stream rule is mm_boot1d_fast's and part of the contract (restated in numpy in tests/_fast_ref.py):
 *     h = mix64(seed ^ mix64(key * 0x100000001B3 + r))
 *     state = (mix64(h), mix64(h + 1))     increment = (mix64(h + 2), mix64(h + 3) | 1)          (high word, low word)
 * a plain PCG64, on which the weights of replicate r are numpy's Generator.multinomial(n, multiplicities / n) draw for draw.
 * Same samplers and replicate arithmetic as mm_boot2d_replay: the draws are not those of the reference's single stream -- the
 * results are statistically equivalent to the reference's -- but they are numpy's own on the stated per-replicate stream.
 * d_w_dump (optional, NULL in production): int32 weights [slot][k < kmax_dump][r < num_boot]. */
int mm_boot2d_fast(const double *d_pk, const double *d_lq, const double *d_v1, const double *d_v2, const double *d_a,
                   const double *d_b, const int64_t *d_tile_ptr, int64_t n_slots, const int32_t *d_slot_K, const double *d_slot_nobs,
                   const double *d_slot_omq, const int64_t *d_slot_row, const int64_t *d_slot_key, uint64_t seed, int32_t num_boot,
                   int64_t ld, double *d_out_corr, int32_t *d_w_dump, int32_t kmax_dump, void *stream);

/* mm_boot2d_fast on a replicate RANGE (sequential bootstrap, ht_2d_moments(rng='fast', max_boot=...)): local replicate i in
 * [0, rep_n) draws from the stream of global replicate rep_lo + i -- (seed, d_slot_key[s], rep_lo + i) -- and is stored in column
 * 1 + i of row d_slot_row[s]; ld >= 1 + rep_n; d_w_dump (optional) is [slot][k < kmax_dump][i < rep_n].  mm_boot2d_fast is the
 * case rep_lo = 0, rep_n = num_boot of the same kernel and the same launch, so replicates [rep_lo, rep_lo + rep_n) made later, for
 * some of the chains, are bit for bit those of a one-shot launch over [0, rep_lo + rep_n).
 *   - rep_lo >= 0, rep_n >= 1 and rep_lo + rep_n <= 2^31 - 1; n_slots is a multiple of 64.
 *   - The streams are those of mm_boot1d_fast_range: no replicate range of one chain collides with a range of another chain.
 *   - A slot with d_slot_row[s] < 0 (or d_slot_K[s] <= 0) writes nothing: that is how the chains of closed tests are skipped
 *     without a new tile layout.  K == 1 chains run, as in mm_boot2d_fast: every replicate is the observed sample.
 *   - Column 0, the columns beyond rep_n and the rows of skipped slots are not written.  The rows are trusted: validate them on
 *     the host.
 *   - Grid: one wave per (slot, 64 replicates), four waves per block.  Up to 2^22 blocks they are one row of gridDim.x; beyond,
 *     rows of 2^22 blocks in gridDim.y (at most 65,535, checked), since a grid dimension holds fewer than 2^32 threads.
 * The 2D path has no refill stage: an invalid replicate is a NaN column that the contraction drops, so the records of the
 * rounds (mm_contract_stats on each round's plane) fold into exactly the one-shot call's counts. */
int mm_boot2d_fast_range(const double *d_pk, const double *d_lq, const double *d_v1, const double *d_v2, const double *d_a,
                         const double *d_b, const int64_t *d_tile_ptr, int64_t n_slots, const int32_t *d_slot_K, const double *d_slot_nobs,
                         const double *d_slot_omq, const int64_t *d_slot_row, const int64_t *d_slot_key, uint64_t seed, int32_t rep_lo,
                         int32_t rep_n, int64_t ld, double *d_out_corr, int32_t *d_w_dump, int32_t kmax_dump, void *stream);

/* mm_boot2d_fast_range over a LIST of slots (sequential bootstrap of ht_2d_vs_control_sequential(rng='fast', max_boot=...)): the launch has
 * one wave per (listed slot, 64 replicates) -- wave w takes slot d_slot_list[w / chunks], chunks = ceil(rep_n / 64) -- instead of
 * one per slot of the whole tile layout, so a round's grid is sized by the chains it continues, not by the chunk.  Once the slot
 * is known it is the same kernel body: the stream (seed, d_slot_key[s], rep_lo + i), the operands and the store to column 1 + i
 * of row d_slot_row[s] are those of mm_boot2d_fast_range, and a listed slot gets bit for bit the replicates that launch gives it.
 *   - There is no weight dump.  rep_lo, rep_n, ld and n_slots are checked as in mm_boot2d_fast_range.
 *   - n_list >= 0; d_slot_list (int64 [n_list], device) may be NULL only when n_list == 0, which returns MM_OK without a launch.
 *   - The list is trusted: every entry must be a slot of the layout, 0 <= s < n_slots; validate it on the host.  A listed slot
 *     with d_slot_K[s] <= 0 or d_slot_row[s] < 0 writes nothing; a slot that is not listed is never read, whatever its row.
 *   - A slot listed twice is written twice with the same values (two waves store identical cells); the engine never does that:
 *     its lists are ascending and unique.
 *   - Grid: n_list x chunks waves, four per block, laid out as in mm_boot2d_fast_range (fewer than 2^32 threads per dimension). */
int mm_boot2d_fast_slots(const double *d_pk, const double *d_lq, const double *d_v1, const double *d_v2, const double *d_a,
                         const double *d_b, const int64_t *d_tile_ptr, int64_t n_slots, const int32_t *d_slot_K, const double *d_slot_nobs,
                         const double *d_slot_omq, const int64_t *d_slot_row, const int64_t *d_slot_key, uint64_t seed, int32_t rep_lo,
                         int32_t rep_n, int64_t ld, double *d_out_corr, const int64_t *d_slot_list, int64_t n_list, void *stream);

/* ---- synthetic data generator (replaces memento/simulate.py:52-89 and :91-115) ----
 * Counter-based: transcriptome count z[cell][gene] ~ NB(mean[gene], size theta[gene]) is a pure function of (seed_z, cell, gene),
 * so nothing dense is ever stored.  One launch per pass, selected by `mode`:
 *   0: d_totals[cell]  = sum_g z                         (needed by the hypergeometric capture)
 *   1: d_row_nnz[cell] = number of genes with a captured count > 0
 *   2: write row `cell` of the captured CSR at d_row_ptr[cell] (d_out_indices int32 ascending, d_out_data float32 counts)
 *   3: d_raw_totals[cell] = sum_g nb (Gaussian-copula branch only, before the rescaling below)
 * process 0: multivariate hypergeometric capture of rint(q[cell] * total) molecules (simulate.py:104-109; needs d_totals);
 *         1: Poisson capture x ~ Poisson(q[cell] * z) (simulate.py:110-112);  2: no capture (x = z, d_qs may be NULL).
 * Gaussian-copula branch (simulate.py:70-89): d_gauss != NULL holds the correlated standard-normal scores, [gene][cell] float32
 * (Cholesky factor of the correlation matrix x white noise from mm_std_normal: a library GEMM on the caller's side); then
 * nb = nbinom.ppf(Phi(score)) replaces the own NB draw, and with d_cell_size != NULL (needs d_raw_totals from a mode-3 pass)
 * z = rint(nb / raw_total[cell] * cell_size[cell]) (simulate.py:86-89).  d_gauss == NULL: independent branch (:66-68).
 * Draws are NOT numpy's (different generators): statistical equivalence only.
 * The stream keys (restated in numpy in tests/_simulate_ref.py).  mix() is the splitmix64 output function without the increment
 * (x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31), all arithmetic is uint64.
 * A stream is the state s0 = make(seed, a, b) = mix(seed ^ mix(a * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) ^ mix(b + 0xD1B54A32D192ED03));
 * its n-th uniform (n = 1, 2, ...) is ((mix(s0 + n * 0x9E3779B97F4A7C15) >> 11) + 0.5) / 2^53.  Three families:
 *   - the NB draw of (cell, gene):  make(seed_z, cell, gene), gene a non-negative int32, so b < 2^31;
 *   - the capture stream of a cell: make(seed_capture, cell, 2^32 + 0x5EED), consumed gene by gene in ascending order;
 *   - element i of mm_std_normal:   make(seed, i, 2^33 + 0x6A55), one Box-Muller pair, the cosine branch.
 * mix is a bijection, so for one (seed, a) two different b are two different streams: the tags of the last two families sit
 * in the high word of b, where no gene index reaches, and seed_z == seed_capture == seed is as good as any other choice.
 * Sentinels: a gene with mean <= 0 or NaN is all zero and consumes no draw; nothing outside [0, n_cells) of d_totals,
 * d_row_nnz, d_raw_totals and outside [d_row_ptr[0], d_row_ptr[n_cells]) of the CSR arrays is written; n_cells == 0 launches
 * nothing.
 * The copula quantile: the smallest k with CDF(k) >= Phi(score) in double, Phi(score) = erfc(-score / sqrt 2) / 2, by summing
 * the pmf upwards (compensated) from max(0, floor(mean - 9 sd)) until the bound on the remaining tail falls below 2^-54: no
 * finite score is cut short.  The first term is p^theta, or above 0 the binomial saddle-point form (Loader 2000), which has
 * no difference of large lgamma values in it.  Domain: the result is exact up to ties (Phi(score) within rounding of a CDF
 * step; then one off) for mean <= 1e4, theta in [0.01, 1e5] and scores in [-6.5, 6.5], which
 * tests/test_gpu_simulate_kernels.py checks against extended-precision sums, the excuse being the routine's own rounding
 * distance.  Nothing in the routine changes beyond that domain, but nothing is checked there; the rounding of the recurrence
 * grows with the number of terms between the start and the answer (~9 sd).  A score of +inf (Phi == 1, every score from 8.3)
 * returns the k at which the running sum rounds to 1 or the tail bound is reached, whichever comes first; -inf (every score
 * below -38.5) and NaN return the start of the sum.  The loop is bounded by the geometric tail (ratio mean / (mean + theta)):
 * at (1e4, 0.01) ~4e7 terms for a lane that holds a score of 8.3 or more. */
int mm_simulate(const double *d_mean, const double *d_theta, int32_t n_genes, int64_t n_cells, const double *d_qs, uint64_t seed_z,
                uint64_t seed_capture, int32_t process, int32_t mode, int64_t *d_totals, int64_t *d_row_nnz, const int64_t *d_row_ptr,
                int32_t *d_out_indices, float *d_out_data, const float *d_gauss, const double *d_cell_size, int64_t *d_raw_totals,
                void *stream);
/* n independent standard normals (float32), element i a pure function of (seed, i). */
int mm_std_normal(uint64_t seed, int64_t n, float *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEMENTO_HIP_H */
