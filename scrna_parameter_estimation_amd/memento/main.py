"""Public API: the same names, arguments and ``adata.uns['memento']`` schema as the reference's
``memento/main.py`` -- with the hot path running in hand-written HIP kernels (no CPU fallback).

Reference signatures mirrored (paths relative to /root/reference/):
  setup_memento        memento/main.py:26-34      create_groups      :94-99
  compute_1d_moments   :171-176                   ht_1d_moments      :341-350
  compute_2d_moments   :293                       ht_2d_moments      :418-427      get_corr_matrix :277
  get_groups           :156-168                   get_1d_moments / get_1d_ht_result  :523, :635
Extra keyword-only knobs (do not disturb the reference's positional order):
  ht_1d_moments(..., rng='replay', strict=False, fill_seed=0)
  ht_2d_moments(..., fill_seed=0, strict=False, rng='replay')
  compute_1d_moments(..., subset_var=True)

Host code here is argument handling, the uns schema, O(G) post-processing (polyfit, filters, design
matrix, p-values); every O(nnz) or O(G x groups x B) step is a kernel launch via ``engine``.
"""

import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pandas as pd
import scipy.stats as stats
from scipy.sparse import csr_matrix

from .. import engine
from . import _ht, _strict1d, util
from . import asl as _asl
from . import design as _design


# ----------------------------------------------------------------------------------------------
# state kept next to the AnnData (device handles are not serialisable: prepare_to_save drops them)
# ----------------------------------------------------------------------------------------------


class _HipState:
    """Device-resident data of one AnnData: CSR, count blocks, per-(group, gene) integer sums."""

    def __init__(self):
        self.csr = None
        self.blocks = None
        self.sumx = None
        self.maxx = None
        self.gene_idx = None  # original column index of every currently kept gene

    def __deepcopy__(self, memo):  # shared, read-only after construction
        return self


class _GroupCellsView:
    """Stands in for the reference's per-group CSC copy (main.py:128): only ``shape`` is ever read
    by the API (main.py:364, :534); the counts themselves live in the device count blocks."""

    def __init__(self, n_cells, n_genes):
        self.shape = (int(n_cells), int(n_genes))

    def __repr__(self):
        return f"<device count-block view {self.shape[0]} cells x {self.shape[1]} genes>"


def _mv_fit(mean, var):
    """np.polyfit(log m, log v, 2) over m>0 & v>0  (estimator.py:84-93)."""
    ok = (mean > 0) & (var > 0)
    return np.polyfit(np.log(mean[ok]), np.log(var[ok]), 2)


def _res_var(mean, var, fit):
    """estimator.py:103-111."""
    ok = (mean > 0) & (var > 0)
    out = np.full(mean.shape, np.nan)
    with np.errstate(invalid="ignore"):
        out[ok] = np.exp(np.log(var[ok]) - np.poly1d(fit)(np.log(mean[ok])))
    return out


def _moments_from_sums(S, n_obs, q):
    """mean = S1/n ; var = S2/n - (1-q) S3/n - mean^2   (estimator.py:179-183)."""
    mean = S[0] / n_obs
    var = S[1] / n_obs - (1 - q) * S[2] / n_obs - mean ** 2
    return mean, var


def _plain_means(blocks, sumx, n_cells, thresh, kind):
    """Plain per-group mean count of every gene, as the reference's scipy calls round it, for the `mean < thresh` gene filters
    (main.py:67 on the CSR of all cells, :201-203 on a group's CSC copy).

    The device returns the exact integer sum of the counts, so mean = sumx / n is exact to one rounding -- but scipy computes
    sum_c fl(x_c * (1/n)) (sequentially in cell order for a CSR, first + pairwise(rest) for a CSC), which lands a few ulp away.
    That only matters when sumx / n IS the threshold (e.g. 189 counts in 2,700 cells = 0.07): for such genes -- and only for
    them -- the gene's counts are pulled from the count blocks in cell order and summed the way scipy does, so the filter
    decides exactly like the reference.  Returns float64 [n_groups][G]."""
    n_cells = np.asarray(n_cells, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = sumx.astype(np.float64) / n_cells[:, None]
    near = np.abs(mean - thresh) <= 1e-9 * abs(thresh)
    if not near.any():
        return mean
    genes = np.flatnonzero(near.any(axis=0))
    cols = engine.GeneColumns(blocks, genes)
    data = engine.host(cols.cols, np.uint32)
    ptr = engine.host(cols.col_ptr)
    for gi, m_ in zip(*np.nonzero(near[:, genes])):
        parts = []
        for b in range(int(blocks.grp_blk0[gi]), int(blocks.grp_blk0[gi + 1])):
            e = data[int(ptr[b, m_]):int(ptr[b, m_ + 1])]
            e = e[np.argsort(e & (engine.BLOCK_CELLS - 1), kind="stable")]        # cell order inside the block
            parts.append((e >> 13).astype(np.float64))
        v = np.concatenate(parts) if parts else np.zeros(0)
        v = np.ascontiguousarray(v * (1.0 / n_cells[gi]))
        if len(v) == 0:
            val = 0.0
        elif kind == 'csr':
            val = float(np.cumsum(v)[-1])                    # csc_matvec of the transpose: sequential in cell order
        else:
            val = float(np.add.reduceat(v, [0])[0])          # _minor_reduce: first + pairwise(rest)
        mean[gi, genes[m_]] = val
    return mean


# ----------------------------------------------------------------------------------------------
# setup_memento / create_groups
# ----------------------------------------------------------------------------------------------


def setup_memento(adata, q_column, inplace=True, filter_mean_thresh=0.07, trim_percent=0.1, shrinkage=0.5, num_bins=30,
                  estimator_type='hyper_relative', *, device_csr=None, comm=None, shard=False, size_factor=None):
    """Compute size factors and the all-cell moments (reference: memento/main.py:26-91).

    Extensions: ``device_csr`` -- an ``engine.DeviceCSR`` already resident in HBM (``adata.X`` is then only
    used for its shape); ``comm`` -- a ``dist.Comm`` when the GENES are sharded over ranks (every rank holds
    all cells x its gene shard): per-cell totals are all-reduced so every rank gets the global size factors.
    ``shard=True`` (with ``comm``): ``adata`` holds ALL genes on every rank; this rank's genes are cut out of the resident CSR
    on the device -- no host-side ``X[:, genes]`` -- and the later calls work on that shard (``adata`` itself is left whole;
    ``uns['memento']['gene_list']`` etc. name the shard's genes).  ``shard=True`` / ``'balanced'``: a cost-balanced gene SET
    (``dist.shard_genes_balanced`` over the predicted chain cost of every gene, from the per-gene totals of the resident matrix:
    each rank gets the same mix of long and short bootstrap chains); ``'contiguous'``: the range ``dist.shard_genes`` gives.
    ``shard=<array>``: ``adata`` already holds only this rank's genes, at these positions of the unsharded gene order.
    ``size_factor`` -- precomputed size factors (N values, e.g. those of the whole matrix when ``adata`` is a gene subset):
    the estimation of estimator.py:49-81 is skipped and they are used as they are."""
    if not inplace:
        adata = adata.copy()
    assert adata.obs[q_column].max() < 1
    assert type(adata.X) == csr_matrix, 'please make sure that adata.X is a scipy CSR matrix'
    if estimator_type not in ('hyper_relative', 'mean_only'):
        raise NotImplementedError("the HIP path implements estimator_type 'hyper_relative' and 'mean_only'")
    m = adata.uns['memento'] = {}
    m['q_column'] = q_column
    m['all_q'] = adata.obs[q_column].values.mean()
    m['estimator_type'] = estimator_type
    m['filter_mean_thresh'] = filter_mean_thresh
    m['num_bins'] = num_bins

    st = m['_hip'] = _HipState()
    if device_csr is None:
        device_csr = getattr(adata, 'device_csr', None)       # h5ad.read_h5ad(to_device=True) attaches the resident matrix
    st.csr = device_csr if device_csr is not None else engine.DeviceCSR(adata.X)
    st.comm = comm
    N, G = adata.shape
    assert tuple(st.csr.shape) == (N, G)
    names0 = np.asarray(adata.var.index)
    st.shard = None
    if isinstance(shard, (np.ndarray, list, tuple)):
        # the caller pre-sliced X: these are the positions of adata's genes in the unsharded gene order (needed to put the
        # gathered results, and the global np.random stream, back in that order)
        st.shard = np.asarray(shard, dtype=np.int64)
        assert st.shard.shape == (G,)
    elif shard:
        if comm is None:
            raise ValueError("shard=True needs comm")
        from ..dist import gene_cost, shard_genes, shard_genes_balanced
        if shard == 'contiguous':
            lo, hi = shard_genes(G, comm.rank, comm.world)
            mine = np.arange(lo, hi)
            st.csr = st.csr.colsplit(lo, hi)         # device-side column split; the full CSR is released
        else:
            mine = shard_genes_balanced(gene_cost(st.csr.colsum() / N, filter_mean_thresh), comm.rank, comm.world)
            st.csr = st.csr.colselect(mine)
        st.shard = mine                              # this rank's genes: positions in the unsharded gene order (ascending)
        st.var_names = names0 = names0[mine]
        G = len(mine)
    st.gene_idx = np.arange(G)
    if size_factor is not None:
        size_factor = np.asarray(size_factor, dtype=np.float64)
        assert size_factor.shape == (N,)
        adata.obs['memento_size_factor'] = size_factor
        m['least_variable_genes'] = []
        blocks_all = engine.count_blocks(st.csr, np.zeros(N, dtype=np.int32), 1)
        S, _, _ = blocks_all.moments(1.0 / size_factor)
        m['all_1d_moments'] = list(_moments_from_sums(S[:, 0], N, m['all_q']))
        if estimator_type == 'mean_only':
            m['all_1d_moments'] = [m['all_1d_moments'][0] + 1, np.ones(G) * 10]
        return adata if not inplace else None
    naive = st.csr.rowsum()                                                   # estimator.py:64-69
    if comm is not None:
        naive = comm.allreduce_sum(naive)
    blocks_all = engine.count_blocks(st.csr, np.zeros(N, dtype=np.int32), 1)
    with np.errstate(divide="ignore"):
        S, sumx, _ = blocks_all.moments(1.0 / naive)
    all_m, all_v = _moments_from_sums(S[:, 0], N, m['all_q'])                 # main.py:62-66
    all_m = all_m.copy()
    all_m[_plain_means(blocks_all, sumx, [N], filter_mean_thresh, 'csr')[0] < filter_mean_thresh] = 0   # main.py:67
    if comm is None:
        all_rv = _res_var(all_m, all_v, _mv_fit(all_m, all_v))                # main.py:68
        rv_ulim = np.quantile(all_rv[np.isfinite(all_rv)], trim_percent)      # main.py:71
    else:                                   # the fit and the quantile are over ALL genes: gather the shards
        gm, gv = comm.allgather_concat(all_m), comm.allgather_concat(all_v)
        fit0 = _mv_fit(gm, gv)
        grv = _res_var(gm, gv, fit0)
        rv_ulim = np.quantile(grv[np.isfinite(grv)], trim_percent)
        all_rv = _res_var(all_m, all_v, fit0)
    all_rv[~np.isfinite(all_rv)] = np.inf
    mask = all_rv < rv_ulim                                                   # main.py:73
    m['least_variable_genes'] = names0[mask].tolist()
    nrc = st.csr.rowsum(mask)                                                 # estimator.py:73
    if comm is not None:
        nrc = comm.allreduce_sum(nrc)
    nrc = nrc + np.quantile(nrc, shrinkage)                                   # estimator.py:74
    size_factor = nrc / nrc.mean()                                            # estimator.py:75-76
    adata.obs['memento_size_factor'] = size_factor
    S, _, _ = blocks_all.moments(1.0 / size_factor)                           # main.py:86-90
    m['all_1d_moments'] = list(_moments_from_sums(S[:, 0], N, m['all_q']))
    if estimator_type == 'mean_only':                                         # estimator.py:188-204
        m['all_1d_moments'] = [m['all_1d_moments'][0] + 1, np.ones(G) * 10]
    if not inplace:
        return adata


def create_groups(adata, label_columns, label_delimiter='^', inplace=True):
    """Discrete groups from obs columns; builds the group-ordered device count blocks
    (reference: memento/main.py:94-135, util.py:8-13)."""
    if not inplace:
        adata = adata.copy()
    m = adata.uns['memento']
    lab = 'sg' + label_delimiter
    for idx, col_name in enumerate(label_columns):
        lab = lab + adata.obs[col_name].astype(str)
        if idx != len(label_columns) - 1:
            lab = lab + label_delimiter
    adata.obs['memento_group'] = lab
    m['label_columns'] = label_columns
    m['label_delimiter'] = label_delimiter
    codes, uniques = pd.factorize(adata.obs['memento_group'].values)          # first-appearance order == drop_duplicates
    m['groups'] = list(uniques)
    m['q'] = adata.obs[m['q_column']].values
    st = m['_hip']
    st.group_id = codes.astype(np.int32)
    st.blocks = engine.count_blocks(st.csr, st.group_id, len(uniques))
    G = adata.shape[1]
    m['group_cells'] = {g: _GroupCellsView(st.blocks.grp_ncells[i], G) for i, g in enumerate(m['groups'])}
    qsum = np.bincount(codes, weights=m['q'], minlength=len(uniques))
    m['group_q'] = {g: qsum[i] / st.blocks.grp_ncells[i] for i, g in enumerate(m['groups'])}
    for k in ('size_factor', 'approx_size_factor', 'all_approx_size_factor'):
        m.pop(k, None)
    if not inplace:
        return adata


def _bin_size_factor(adata):
    """30 equal-width bins over all cells' size factors; cell -> bin mean; the max keeps its own value
    (reference: memento/main.py:138-153).  Also records the integer bin id per cell for the device."""
    m = adata.uns['memento']
    size_factor = adata.obs['memento_size_factor'].values
    means, _, idx = stats.binned_statistic(size_factor, size_factor, bins=m['num_bins'], statistic='mean')
    idx = np.clip(idx, a_min=1, a_max=means.shape[0]) - 1
    max_sf = size_factor.max()
    is_max = size_factor == max_sf
    table = np.concatenate([means, [max_sf]])            # one extra "bin" for the max cell(s)
    bin_id = idx.astype(np.int64)
    bin_id[is_max] = means.shape[0]
    approx_sf = table[bin_id]
    st = m['_hip']
    st.sf_bin = bin_id.astype(np.uint8) if table.shape[0] <= 256 else None
    st.sf_table = np.nan_to_num(table, nan=1.0)          # empty bins are never referenced
    m['all_approx_size_factor'] = approx_sf
    # per-group views in the cells' original order: the count blocks' cell order is the stable sort by group (engine.plan_blocks)
    order, ends = st.blocks.cell_order, np.cumsum(st.blocks.grp_ncells)
    a_sorted, s_sorted = approx_sf[order], size_factor[order]
    m['approx_size_factor'] = {g: a_sorted[ends[i] - st.blocks.grp_ncells[i]:ends[i]] for i, g in enumerate(m['groups'])}
    m['size_factor'] = {g: s_sorted[ends[i] - st.blocks.grp_ncells[i]:ends[i]] for i, g in enumerate(m['groups'])}


def get_groups(adata):
    """DataFrame of group label components, rows in uns order (reference: memento/main.py:156-168)."""
    m = adata.uns['memento']
    rows = [g.split(m['label_delimiter'])[1:] for g in m['groups']]
    df = pd.DataFrame(rows, index=m['groups'], columns=m['label_columns'])
    for col in df.columns:
        try:
            df[col] = pd.to_numeric(df[col])
        except (ValueError, TypeError):
            pass
    return df


# ----------------------------------------------------------------------------------------------
# compute_1d_moments
# ----------------------------------------------------------------------------------------------


def compute_1d_moments(adata, inplace=True, min_perc_group=0.7, filter_genes=True, gene_list=None, subset_var=True):
    """Mean, variance and residual variance per group (reference: memento/main.py:171-274).

    ``subset_var=False`` skips the host-side column subset of ``adata`` itself (an O(nnz) scipy copy the
    reference performs at main.py:229); the device blocks and uns['memento']['gene_list'] are what the
    later calls use."""
    assert 'memento' in adata.uns
    if not inplace:
        adata = adata.copy()
    m = adata.uns['memento']
    st = m['_hip']
    if 'size_factor' not in m.keys():
        _bin_size_factor(adata)
    groups = m['groups']
    ng = len(groups)
    Nc = st.blocks.grp_ncells.astype(np.float64)
    gq = np.array([m['group_q'][g] for g in groups])
    S, sumx, maxx = st.blocks.moments(1.0 / adata.obs['memento_size_factor'].values)          # K1+K2
    cur = st.gene_idx                                    # columns of the device blocks that adata currently holds
    names_cur = _var_names(adata)
    if getattr(st, 'shard', None) is not None and adata.shape[1] != st.csr.shape[1]:
        subset_var = False                               # adata holds all genes of all ranks; only the shard's names move
    mean = S[0][:, cur] / Nc[:, None]
    var = S[1][:, cur] / Nc[:, None] - (1 - gq)[:, None] * S[2][:, cur] / Nc[:, None] - mean ** 2
    if m['estimator_type'] == 'mean_only':                                                     # estimator.py:188-204
        mean, var = mean + 1, np.ones(mean.shape) * 10
    st.sumx, st.maxx, st.S = sumx, maxx, S
    obs_mean = _plain_means(st.blocks, sumx, Nc, m['filter_mean_thresh'], 'csc')[:, cur]      # main.py:201
    gene_filter = (obs_mean > m['filter_mean_thresh']) & (var > 0)                             # main.py:202-203
    gene_rv_filter = maxx[:, cur] >= 2                                                         # main.py:206-207
    m['gene_filter'] = {g: gene_filter[i] for i, g in enumerate(groups)}
    overall = gene_filter.mean(axis=0) > min_perc_group                                        # main.py:210-212
    m['overall_gene_filter'] = overall
    m['gene_list'] = names_cur[overall].tolist()
    if filter_genes:                                                                           # main.py:219-229
        mean, var, gene_rv_filter = mean[:, overall], var[:, overall], gene_rv_filter[:, overall]
        st.gene_idx = cur[overall]
        for g in groups:
            m['group_cells'][g] = _GroupCellsView(m['group_cells'][g].shape[0], int(overall.sum()))
        if subset_var:
            adata._inplace_subset_var(overall)
        else:
            st.var_names = names_cur[overall]
    m['gene_rv_filter'] = {g: gene_rv_filter[i] for i, g in enumerate(groups)}
    fm = np.concatenate([mean[i][gene_rv_filter[i]] for i in range(ng)])
    fv = np.concatenate([var[i][gene_rv_filter[i]] for i in range(ng)])
    comm = getattr(st, 'comm', None)
    if comm is not None:                    # gene-sharded: the pooled fit sees every rank's genes
        fm, fv = comm.allgather_concat(fm), comm.allgather_concat(fv)
    fit = _mv_fit(fm, fv)                                                                      # main.py:232-245
    m['mv_regressor'] = {'all': fit}
    for g in groups:
        m['mv_regressor'][g] = fit
    m['1d_moments'] = {g: [mean[i], var[i], _res_var(mean[i], var[i], fit)] for i, g in enumerate(groups)}  # main.py:248-255
    if gene_list is not None:                                                                  # main.py:258-271
        assert type(gene_list) == list
        names = _var_names(adata)
        given = np.isin(names, gene_list)
        for g in groups:
            m['1d_moments'][g] = [a[given] for a in m['1d_moments'][g]]
            m['group_cells'][g] = _GroupCellsView(m['group_cells'][g].shape[0], int(given.sum()))
        st.gene_idx = st.gene_idx[given]
        if subset_var:
            adata._inplace_subset_var(given)
        else:
            st.var_names = names[given]
    if not inplace:
        return adata


def _var_names(adata):
    st = adata.uns['memento']['_hip']
    names = getattr(st, 'var_names', None)
    if names is not None and len(names) == len(st.gene_idx):
        return np.asarray(names)
    return np.asarray(adata.var.index)


# ----------------------------------------------------------------------------------------------
# ht_1d_moments
# ----------------------------------------------------------------------------------------------


def ht_1d_moments(adata, covariate, treatment, treatment_for_gene=None, inplace=True, num_boot=10000, verbose=1, num_cpus=1,
                  rng='replay', strict=False, fill_seed=0, max_rows=None, ci=None, **kwargs):
    """Bootstrap hypothesis test of mean / residual-variance differences (reference: memento/main.py:341-415).

    ``rng='replay'``: the multinomial resampling replays numpy's ``Generator(PCG64(5))`` stream draw for
    draw (bootstrap.py:102-103) and the bin order uses the two uniforms the reference takes from the global
    ``np.random`` state per (gene, group) (bootstrap.py:62, :65).
    ``rng='fast'``: same samplers and arithmetic, but every (pair, replicate) has its own counter-derived PCG64
    stream and replicates run in parallel lanes -- statistically equivalent, much faster, not draw-identical.
    The streams are keyed by (``fill_seed``, the gene's position among the kept genes of the unsharded call, group, replicate),
    so the result depends neither on ``max_rows`` nor on gene sharding; in a one-chunk unsharded call the key is the chain's row.
    ``strict=True`` additionally replays the reference's ``_fill`` draws from the global stream in gene order
    (exactly reproducible against the reference at ``num_cpus=1``; sequential, meant for validation);
    with ``strict=False`` invalid replicates are re-filled on the device with a counter-based RNG.
    ``ci``: a level 0 < ci < 1 adds the percentile interval of every coefficient, the (1 - ci) / 2 and (1 + ci) / 2 quantiles
    (np.nanquantile, 'linear') of the replicate coefficients the standard error is taken over (columns 1..num_boot, dropped
    columns excluded, not centred): ``uns['memento']['1d_ht']['mean_ci']`` / ``['var_ci']`` [test][2] and ``['ci']``, the level;
    ``get_1d_ht_result`` then has ``de_ci_lo, de_ci_hi, dv_ci_lo, dv_ci_hi``.  A NaN coefficient has a NaN interval.  Not gathered
    across ranks (NotImplementedError on a gene-sharded run).  ``ci=None`` (default): nothing is added and nothing more runs.
    kwargs: ``resampling`` (required, as in the reference), ``approx``, ``resample_rep``.
    """
    resampling, resample_rep, approx = _ht.check_args(rng, strict, **kwargs)
    probs = _ht.ci_probs(ci)
    if not inplace:
        adata = adata.copy()
    m = adata.uns['memento']
    st = m['_hip']
    comm = getattr(st, 'comm', None)
    sharded = comm is not None and comm.world > 1
    if sharded and probs is not None:
        raise NotImplementedError("ci= on a gene-sharded run: the intervals are not gathered across ranks")
    mv = _ht.moments_view(m)
    ng = mv.ng
    names = _var_names(adata)
    G_all = len(st.gene_idx)
    cov = np.asarray(covariate.values, dtype=np.float64)
    trt_all = np.asarray(treatment.values, dtype=np.float64)
    gene_cols = _ht.gene_columns(treatment, treatment_for_gene, names[:G_all])
    if st.sf_bin is None:
        raise NotImplementedError("more than 255 size-factor bins")
    shard_stream = gene_pos = None
    if sharded:
        # The reference scatters every gene's result back from ONE sequential np.random stream (main.py:399-404, bootstrap.py:62-65):
        # two hash uniforms per live (gene, group) chain, gene-major.  A rank must therefore use the uniforms at the positions its
        # genes have in the UNSHARDED order: gather (position, live chains) of every kept gene, draw the whole stream (the same
        # on every rank: the caller seeds all ranks alike) and keep this rank's entries.  N-rank results then equal 1-rank results.
        shard = getattr(st, 'shard', None)
        if shard is not None:
            gene_pos = np.asarray(shard, dtype=np.int64)[st.gene_idx]
        else:                               # the caller pre-sliced X: contiguous blocks in rank order
            sizes = comm.allgather_objects(int(st.csr.shape[1]))
            gene_pos = int(sum(sizes[:comm.rank])) + np.asarray(st.gene_idx, dtype=np.int64)
        if strict:
            # strict=True also replays the reference's _fill draws, which shift the global stream gene after gene: sequential over
            # ALL genes.  With contiguous shards the ranks take turns in rank order and hand the stream state on (the validation
            # mode: exact, no speed-up); interleaved (cost-balanced) shards cannot be replayed that way.
            spans = comm.allgather_objects((int(gene_pos.min()), int(gene_pos.max())) if len(gene_pos) else None)
            spans = [sp_ for sp_ in spans if sp_ is not None]
            if any(a[1] >= b[0] for a, b in zip(spans[:-1], spans[1:])):
                raise NotImplementedError("strict=True over several ranks needs contiguous gene shards in rank order "
                                          "(setup_memento(shard='contiguous') or a pre-sliced range); cost-balanced shards interleave")
        else:
            from ..dist import shard_stream_uniforms
            shard_stream = shard_stream_uniforms(comm, gene_pos, (~_ht.pair_skip(mv.true_mean, mv.true_rv)).reshape(G_all, ng))
    # position of every kept gene in the unsharded, unfiltered gene order: keys the device refill streams, so that the timed mode's
    # results do not depend on gene chunking or on the sharding over GPUs
    fill_pos = (np.asarray(st.shard, dtype=np.int64)[st.gene_idx] if getattr(st, 'shard', None) is not None
                else (gene_pos if gene_pos is not None else np.asarray(st.gene_idx, dtype=np.int64)))
    # position of every kept gene among the KEPT genes of the unsharded call: keys the rng='fast' streams of its chains, so that
    # neither gene chunking nor sharding changes a number -- and the key of a chain of an unsharded call is its row number in the
    # one-chunk call, whose results are therefore those of row-keyed streams
    chain_pos = np.arange(G_all, dtype=np.int64)
    if sharded and not strict:
        chain_pos = np.searchsorted(np.sort(np.concatenate(comm.allgather_objects(gene_pos))), gene_pos).astype(np.int64)

    def run_range(c):
        """One chunk of genes [g0, g1), opened (K5 histograms): bootstrap -> contraction -> p-values."""
        g0, g1, G, bs, skip = c.g0, c.g1, c.G, c.bs, c.skip
        rep_assign = bcol_assign = None
        if not strict:
            # gene-sharded: this rank's slice of the ONE global stream (see above)
            uniforms = None if shard_stream is None else (shard_stream[0][g0 * ng:g1 * ng], shard_stream[1][g0 * ng:g1 * ng])
            keys = (fill_pos[g0:g1, None] * ng + np.arange(ng)[None, :]).reshape(-1)      # refill streams keyed by (gene, group)
            chain_keys = (chain_pos[g0:g1, None] * ng + np.arange(ng)[None, :]).reshape(-1)     # rng='fast' streams, likewise
            good, n_inv = _ht.run_chunk_1d(c, mv, rng, fill_seed, keys, chain_keys, uniforms)    # K6-K8
            # how much of the result depends on the device refill (strict=True replays the reference's own _fill draws instead):
            # chains / genes with at least one refilled replicate -- all others are bit-identical to the strict path
            refilled = (n_inv > 0).any(axis=1) & ~skip
            rs = st.refill_stats
            rs['chains'] += int(((~skip) & (bs.K >= 2)).sum())
            rs['chains_refilled'] += int(refilled.sum())
            rs['genes'] += G
            rs['genes_refilled'] += int(refilled.reshape(G, ng).any(axis=1).sum())
            rs['gene_refilled'][g0:g1] = refilled.reshape(G, ng).any(axis=1)
        else:
            run_from = functools.partial(bs.run, skip, mv_fit=mv.fit, fill_mode=1, mean_only=mv.mean_only)
            gene_trt = [trt_all if k is None else trt_all[:, list(k)] for k in gene_cols[g0:g1]] if resample_rep else None
            replay = _strict1d.StrictReplay(c, run_from, gene_trt)
            bad_fill = replay.run()
            rep_assign, bcol_assign = replay.rep_assign, replay.bcol_assign
            active_all = (~skip) & (bs.K >= 2)                       # bootstrap.py:97-98: a single bin gives NaN replicates
            good = (active_all & ~bad_fill).reshape(G, ng)           # hypothesis_test.py:193-200
        # tests: gene-major x treatment column (main.py:399-404)
        d = _ht.design_tables(good, gene_cols[g0:g1], cov, trt_all, mv.Nc_list, resampled=resample_rep)
        test_gene = d.test_row
        no_group = ~good[test_gene].any(axis=1)
        use_rr = resample_rep and d.rr_test.any()
        col_map = n_valid = None
        if use_rr:
            col_map, n_valid = _ht.surviving_cols(bs, good, num_boot)                                     # hypothesis_test.py:249-251
        out = {}
        for which, tag in ((0, 'mean'), (1, 'var')):
            coef, stt = bs.contract(test_gene, d.Wmat, good, which)                                       # K9+K10
            if use_rr:
                coef_r, stt_r = bs.contract_resampled(test_gene, d.tt_mat, good, which, d.row_mask, d.Mstack, mv.Nc_list,
                                                      rep_assign, bcol_assign, seed=fill_seed + 17, col_map=col_map, n_valid=n_valid)
                coef, stt = _ht.merge_resampled(coef, stt, coef_r, stt_r, d.rr_test)
            c0, se = stt[:, 0].copy(), stt[:, 1].copy()
            # the tail fits of the mean tests run in the worker pool while the variance contraction is enqueued
            fin = _asl.asl_from_stats(stt, approx, lambda idx, coef=coef: engine.host(coef[engine.dev(np.asarray(idx, dtype=np.int64))]),
                                      num_cpus, resampling, defer=True)
            c0[no_group], se[no_group] = np.nan, np.nan                                                   # hypothesis_test.py:203-204
            if probs is not None:
                out[tag + '_ci'] = _ht.row_intervals(coef[:len(test_gene)], bs.ld, num_boot, probs, c0)
            out[tag + '_coef'], out[tag + '_se'], out[tag + '_asl'] = c0, se, (fin, no_group)
        for tag in ('mean', 'var'):
            fin, no_group = out[tag + '_asl']
            p = fin()
            p[no_group] = np.nan
            out[tag + '_asl'] = p
        st.last_assignments = (rep_assign, bcol_assign)
        return out

    st.refill_stats = dict(chains=0, chains_refilled=0, genes=0, genes_refilled=0, gene_refilled=np.zeros(G_all, dtype=bool))
    st.last_bootstrap = None                   # the previous call's replicate rows (GBs) go back to the caching allocator BEFORE this call allocates its own
    if max_rows is None:                       # replicate buffers sized to the free HBM (288 GB on MI355X)
        max_rows = engine.auto_max_rows(num_boot + 1, arrays=2)
    chunk = G_all if strict else max(1, int(max_rows) // max(1, ng))   # strict replay is sequential over all genes
    if sharded and strict:
        parts = []
        for turn in range(comm.world):                # rank after rank, the np.random state handed on
            if turn == comm.rank:
                parts = [run_range(c) for c in _ht.chunks_1d(st, mv, num_boot, chunk)]
            states = comm.allgather_objects(np.random.get_state() if turn == comm.rank else None)
            np.random.set_state(states[turn])
    else:
        parts = [run_range(c) for c in _ht.chunks_1d(st, mv, num_boot, chunk)]
    keys = ('mean_coef', 'mean_se', 'mean_asl', 'var_coef', 'var_se', 'var_asl')
    out = {k: (np.concatenate([p_[k] for p_ in parts]) if parts else np.zeros(0)) for k in keys}
    m['1d_ht'] = {}
    if probs is not None:
        for k in ('mean_ci', 'var_ci'):
            m['1d_ht'][k] = np.concatenate([p_[k] for p_ in parts]) if parts else np.zeros((0, 2))
        m['1d_ht']['ci'] = float(ci)
    if sharded:
        # gene-sharded run: scatter-back of the reference (main.py:399-412) across ranks -- every rank ends with the flat result
        # vectors of ALL genes in the unsharded run's order, plus the gene names they belong to
        from ..dist import gather_1d_ht
        nt_gene = np.array([trt_all.shape[1] if k is None else len(k) for k in gene_cols], dtype=np.int64)
        st.local_ht = {k: np.asarray(v).copy() for k, v in out.items()}          # this rank's own tests (bench: per-rank accounting)
        m['1d_ht']['gene_names'], out = gather_1d_ht(comm, names, out, gene_pos=gene_pos, n_tests=nt_gene)
    if treatment_for_gene is not None:
        m['1d_ht']['treatment_for_gene'] = treatment_for_gene
    m['1d_ht']['treatment'] = treatment
    m['1d_ht']['covariate'] = covariate
    for k in keys:
        m['1d_ht'][k] = out[k]
    if not inplace:
        return adata


def _vs_control_plan(m, control, treatment_col):
    """What ``ht_1d_vs_control`` / ``ht_2d_vs_control`` test: (names of the tested groups or guides, the
    ``VsControlDesigns`` or None, (control group index, the other groups' indices) or (None, None), the metadata that goes
    into ``uns`` next to the result arrays).  Without ``treatment_col``, ``control`` is a group label or index and every other
    group is tested against it; with it, ``control`` is a value of that label column and the designs carry the rest."""
    groups = m['groups']
    ng = len(groups)
    if treatment_col is None:
        ctrl = groups.index(control) if not isinstance(control, (int, np.integer)) else int(control)
        if not 0 <= ctrl < ng:
            raise ValueError(f"control index {control!r} is not one of the {ng} groups")
        others = np.array([j for j in range(ng) if j != ctrl], dtype=np.int64)
        tested = [groups[j] for j in others]
        return tested, None, (ctrl, others), dict(control=groups[ctrl], groups=tested)
    label_columns = list(m['label_columns'])
    if treatment_col not in label_columns:
        raise ValueError(f"treatment_col {treatment_col!r} is not one of the label columns {label_columns}")
    labels = [g.split(m['label_delimiter'])[1:] for g in groups]
    Nc = np.array([m['group_cells'][g].shape[0] for g in groups], dtype=np.float64)
    designs = _design.VsControlDesigns(labels, label_columns.index(treatment_col), str(control), Nc)   # ValueError for an absent control value
    covariates = [c for c in label_columns if c != treatment_col]
    return designs.guides, designs, (None, None), dict(control=str(control), groups=designs.guides, treatment_col=treatment_col,
                                                       covariates=covariates)


def ht_1d_vs_control(adata, control, num_boot=10000, num_cpus=1, rng='replay', fill_seed=0, max_rows=None, approx=False,
                     resampling='bootstrap', *, treatment_col=None, ci=None, max_boot=None, min_extreme=10):
    """Perturb-seq style batch test: every group against one shared ``control`` group (a label of
    ``adata.uns['memento']['groups']`` or its index), for all kept genes, in one call.

    The reference handles this design with a Python loop over guides (subset to control + guide, create_groups,
    compute_1d_moments, ht_1d_moments; e.g. analysis/sciplex/sciplex_dv.py:18-59), re-bootstrapping the control group
    for every guide.  Here each (gene, group) is bootstrapped once and the two-group test statistic -- for the groups
    {control, guide} with a binary treatment and an intercept, _regress_1d (hypothesis_test.py:269-291) reduces to
    log-moment(guide) - log-moment(control) -- is taken for every guide from the shared control rows.  The moments,
    gene filters and the mean-variance fit are those of ``compute_1d_moments`` over ALL groups (the per-guide loop refits
    them on each two-group subset), so numbers differ from that loop by the fit, not by the test.

    With ``treatment_col`` (one of the label columns, e.g. ``'guide'``) the groups are guide x stratum and every other label
    column is a covariate (replicate, well, dose): ``control`` is then a VALUE of that column (compared as the string it has
    in the group labels), and the test of guide value ``g`` is the per-guide regression the reference's loop runs on the
    subset ``{g, control}`` with ``create_groups([is_g, *other_columns])`` -- intercept, the is_g indicator and main-effect
    dummies of the other columns, weighted by cells per group -- over that gene's good guide and control groups of any
    stratum.  A test with no good guide or control group, or with no stratum holding both arms, is NaN.  The ``group``
    column of the result is then the guide value.

    Genes run in chunks of at most ``max_rows`` replicate rows (default: a share of the free device memory).  The device refill
    streams and, with ``rng='fast'``, the bootstrap streams are keyed by (``fill_seed``, gene, group) with the gene numbered over
    the whole call, so the chunking changes no number; in a one-chunk call the key is the chain's row.

    ``ci`` as in ``ht_1d_moments``: the percentile interval of every coefficient.  The coefficient rows are not stored here: they
    are produced for a slice of tests at a time into one bounded scratch tensor (``_ht.sliced_intervals``), which changes no
    number.  Adds the columns ``de_ci_lo, de_ci_hi, dv_ci_lo, dv_ci_hi`` and ``mean_ci`` / ``var_ci`` [test][2] and ``ci`` to ``uns``.

    ``max_boot`` (needs ``rng='fast'``, ``approx=False``, ``ci=None``; an integer >= ``num_boot``): the sequential bootstrap
    (Besag & Clifford 1991).  Every test gets ``num_boot`` replicates -- round 0, which is today's call: the same launches, keys
    and records -- and only the tests that are still open are continued, to the cumulative totals ``num_boot``, ``2 num_boot``,
    ``4 num_boot``, ..., ``max_boot`` (``_ht.sequential_schedule``).  A test is open while its record is testable and its extreme
    count is still <= ``min_extreme`` on the mean or the variability plane (default 10, the reference's own threshold for
    trusting the empirical p-value, hypothesis_test.py:90).  Under ``rng='fast'`` replicate r of a chain owns the stream of (``fill_seed``,
    chain key, r), so the replicates a later round adds are bit for bit those a one-shot call with more replicates makes; a round
    bootstraps only the chains that an open test's design reads and contracts only the open tests.  The p-value of every test is
    ``(c + 1) / (n + 1)`` with c, n the extreme and valid counts over all its rounds, and NO tail fit is made: a test that closed in
    round 0 with c > ``min_extreme`` reports exactly what the plain call reports, and a test that reaches ``max_boot`` with
    c <= ``min_extreme`` reports the reference's upper-bound form of the empirical p-value (its fallback where the tail fit fails).
    ``de_se`` / ``dv_se`` come from the merged record (``_ht.merge_records``).  Invalid replicates of a round are refilled from
    that round's valid ones, under a refill seed derived from (``fill_seed``, round): uniform over valid replicates like the
    one-shot refill and statistically equivalent to it, but not the same draws -- the two agree exactly wherever nothing was
    refilled.  Neither the chunking nor the sub-batching of a round changes a number.  Adds the columns ``de_nboot`` / ``dv_nboot``
    (the valid replicates behind each p-value) and ``mean_nboot``, ``var_nboot``, ``max_boot``, ``min_extreme`` to ``uns``.

    Returns a DataFrame (gene, group, de_coef, de_se, de_pval, dv_coef, dv_se, dv_pval) and stores the arrays in
    ``uns['memento']['1d_ht_vs_control']``."""
    _ht.check_args(rng, resampling=resampling)
    sequential = _ht.check_sequential(max_boot, min_extreme, num_boot, rng, approx, ci)
    probs = _ht.ci_probs(ci)
    m = adata.uns['memento']
    st = m['_hip']
    tested, designs, (ctrl, others), meta = _vs_control_plan(m, control, treatment_col)
    mv = _ht.moments_view(m)
    ng = mv.ng
    names = _var_names(adata)
    G_all = len(st.gene_idx)
    if max_rows is None:                       # (40 % of the free HBM: BASELINE configs[4] then runs in two chunks, the second reusing the
        max_rows = engine.auto_max_rows(num_boot + 1, arrays=2)   # first one's buffers; ONE 108 GB chunk is 1 s faster in a warm process but 1.6 s
                                                                 # slower in a fresh one -- mapping fresh device memory costs ~30 ms per GB)
    chunk = max(1, int(max_rows) // max(1, ng))
    cols = {k: [] for k in ('mean_coef', 'mean_se', 'mean_asl', 'var_coef', 'var_se', 'var_asl')}
    if probs is not None:
        cols.update(mean_ci=[], var_ci=[])
    if sequential:
        cols.update(mean_nboot=[], var_nboot=[])
        schedule = _ht.sequential_schedule(num_boot, max_boot)
        st.last_sequential = SimpleNamespace(schedule=schedule, n_open=[0] * len(schedule))   # (diagnostics: tests open after each round)
        two_group = _ht._TwoGroupDesigns(ng, ctrl) if designs is None else None
    st.last_bootstrap = st.last_good = None    # (see ht_1d_moments: free the previous call's replicate rows first)

    def run_chunk(c):
        G, bs = c.G, c.bs
        keys = np.arange(c.g0 * ng, c.g1 * ng, dtype=np.int64)  # (g0 + gene) * ng + group: the chain's row in the one-chunk call
        good, st.last_n_inv = _ht.run_chunk_1d(c, mv, rng, fill_seed, keys, keys)
        st.last_good = good                    # (diagnostics / tests: the good groups and the refilled replicates of the last gene chunk)
        test_gene = np.repeat(np.arange(G), len(tested))
        test_design = None if designs is None else designs.tests(good)
        st_m, st_v, rows = (bs.contrast(test_gene, np.tile(others, G), ctrl, good) if designs is None
                            else bs.contrast_design(test_gene, test_design, *designs.tables()))
        if sequential:
            if designs is None:      # (the designs ``bs.contrast`` builds are those of _TwoGroupDesigns)
                test_design = two_group.tests(good)
            tables = (two_group if designs is None else designs).tables()
            st_m, st_v = _ht.continue_chunk_1d(c, mv, test_gene, test_design, tables, (st_m, st_v), schedule, min_extreme, resampling,
                                               fill_seed, keys, st.last_sequential.n_open)
        st.last_records = (st_m, st_v)         # (diagnostics / tests: the test records of the last gene chunk)
        for tag, stt, which in (('mean', st_m, 0), ('var', st_v, 1)):
            if sequential:
                p = _ht.sequential_pvalues(stt, resampling)
                cols[tag + '_nboot'].append(stt[:, 2].astype(np.int64))
            else:
                p = _asl.asl_from_stats(stt, approx, lambda idx, w=which: rows(w, idx), num_cpus, resampling)
            cols[tag + '_coef'].append(stt[:, 0])
            cols[tag + '_se'].append(stt[:, 1])
            cols[tag + '_asl'].append(p)
            if probs is not None:
                cols[tag + '_ci'].append(_ht.sliced_intervals(functools.partial(rows, which), bs.ld, num_boot, probs, stt[:, 0]))

    for c in _ht.chunks_1d(st, mv, num_boot, chunk):
        run_chunk(c)
    out = {k: (np.concatenate(v) if v else np.zeros((0, 2) if k.endswith('_ci') else 0)) for k, v in cols.items()}
    m['1d_ht_vs_control'] = dict(out, **meta)
    df = pd.DataFrame({'gene': np.repeat(names, len(tested)), 'group': np.tile(tested, G_all)})
    df['de_coef'], df['de_se'], df['de_pval'] = out['mean_coef'], out['mean_se'], out['mean_asl']
    df['dv_coef'], df['dv_se'], df['dv_pval'] = out['var_coef'], out['var_se'], out['var_asl']
    if probs is not None:
        m['1d_ht_vs_control']['ci'] = float(ci)
        _ci_columns(df, ('de', out['mean_ci']), ('dv', out['var_ci']))
    if sequential:
        m['1d_ht_vs_control'].update(max_boot=int(max_boot), min_extreme=int(min_extreme))
        df['de_nboot'], df['dv_nboot'] = out['mean_nboot'], out['var_nboot']
    return df


def _label_dummies(m, columns):
    """Main-effect dummies (first level dropped) of the label columns ``columns`` of ``create_groups``: [group][...] and names."""
    label_columns = list(m['label_columns'])
    labels = np.asarray([g.split(m['label_delimiter'])[1:] for g in m['groups']], dtype=object).astype(str)
    parts, names = [np.ones((len(labels), 0))], []
    for c in columns:
        if c not in label_columns:
            raise ValueError(f"{c!r} is not one of the label columns {label_columns}")
        dm = pd.get_dummies(pd.Series(labels[:, label_columns.index(c)]), drop_first=True)
        parts.append(dm.values.astype(np.float64))
        names.extend(f"{c}={v}" for v in dm.columns)
    return np.concatenate(parts, axis=1), names


def _joint_block(m, block, what):
    """``treatment`` / ``covariate`` of ``ht_1d_joint`` -> ([group][column] fp64, column names): an array or DataFrame in the group
    order of ``uns['memento']['groups']``, the name of a label column (treatment) or a list of such names (covariate), or None."""
    ng = len(m['groups'])
    if block is None:
        return np.ones((ng, 0)), []
    if isinstance(block, str):
        return _label_dummies(m, [block])
    if isinstance(block, (list, tuple)) and all(isinstance(c, str) for c in block):
        return _label_dummies(m, block)
    names = [str(c) for c in block.columns] if isinstance(block, pd.DataFrame) else None
    a = np.asarray(block.values if isinstance(block, pd.DataFrame) else block, dtype=np.float64)
    a = a.reshape(len(a), -1)
    if a.shape[0] != ng:
        raise ValueError(f"{what} has {a.shape[0]} rows, there are {ng} groups")
    return a, names if names is not None else [f"{what}_{j}" for j in range(a.shape[1])]


def joint_pvalues(stt, approx=False):
    """P-values of joint records [test][8] (``Bootstrap1D.joint``).  ``approx=False``: (1 + n_extreme) / (1 + n_valid), never
    below 1 / (n_valid + 1).  ``approx=True``: the Satterthwaite fit Q* ~ a chi2_nu from the mean m and the population sd s of
    the valid Q*: a = s^2 / (2 m), nu = 2 m^2 / s^2, p = chi2.sf(Q_0 / a, nu).  NaN where there is no test (NaN record), no valid
    replicate or every valid Q* is exactly 0 (the replicates all equal the observed column)."""
    stt = np.asarray(stt, dtype=np.float64)
    q0, s, n, ext, mean, all_equal = (stt[:, k] for k in range(6))
    dead = np.isnan(q0) | (n < 1) | (all_equal == 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        if approx:
            p = stats.chi2.sf(q0 / (s ** 2 / (2 * mean)), 2 * mean ** 2 / s ** 2)
        else:
            p = (1 + ext) / (1 + n)
    return np.where(dead, np.nan, p)


def ht_1d_joint(adata, treatment, covariate=None, num_boot=10000, rng='replay', fill_seed=0, max_rows=None, approx=False):
    """Joint bootstrap test of several treatment columns: does the gene differ AT ALL across the levels of a factor (cell types,
    doses, time points, donors), in mean (``de``) or in variability (``dv``), after the covariates?  One test per kept gene
    instead of one p-value per dummy column, and the answer does not depend on how the factor is coded.

    ``treatment``: array or DataFrame [groups][T] in the group order of ``uns['memento']['groups']``, or the NAME of a label
    column of ``create_groups``: the block is then that column's one-hot dummies with the first level dropped.  ``covariate``:
    array or DataFrame [groups][C], a list of label-column names (main-effect dummies, first level dropped) or None; the
    intercept is always there.

    On a gene's good groups, with w = Nc / sum(Nc) and D = diag(w), M the residual maker of the weighted fit on
    [1, covariate] and the thin SVD D^1/2 M treatment = U S V' of rank r (``design.joint_rows``), the statistic of a replicate
    plane y is Q(y) = ||L y||^2, L = U[:, :r]' D^1/2 M: the weighted sum of squares of the covariate-adjusted log moment that the
    block explains.  It depends on the column space of the block only (which dummy is dropped, or all dummies given: the same
    Q) and for one column it is ss * coef^2 of the marginal test of ``ht_1d_moments``.  The null is the centred bootstrap,
    Q*_c = ||L y_c - L y_0||^2 over the valid replicate columns c >= 1, and
    p = (1 + #{Q*_c > Q_0}) / (1 + n_valid): never below 1 / (n_valid + 1) (no tail fit here).  ``approx=True`` gives smaller
    p-values for screens, from the Satterthwaite fit Q* ~ a chi2_nu to the mean and the sd of the Q* (``joint_pvalues``).
    The statistic is not studentised: the Nc weights already roughly equalise the group variances.

    The bootstrap is that of the other ``ht_*`` calls: ``rng``, ``fill_seed`` and ``max_rows`` as in ``ht_1d_vs_control``, the
    hash uniforms from the global ``np.random`` stream, refill and ``rng='fast'`` streams keyed as in ``ht_1d_moments`` with the
    gene numbered over the whole call -- chunking changes no number, and the same ``np.random`` seed and ``max_rows`` give the
    replicate planes of ``ht_1d_moments``.  Not available on a gene-sharded run (NotImplementedError).

    Returns a DataFrame (gene, df, de_stat, de_pval, dv_stat, dv_pval), df = r; a gene without a design (no good group, or no
    treatment left after the covariates on its good groups) has df 0 and NaN otherwise.  The arrays go to
    ``uns['memento']['1d_ht_joint']``: ``mean_stat``, ``mean_asl``, ``var_stat``, ``var_asl``, ``df``, ``n_valid`` and the
    ``treatment`` / ``covariate`` column names."""
    _ht.check_args(rng, resampling='bootstrap')
    m = adata.uns['memento']
    st = m['_hip']
    comm = getattr(st, 'comm', None)
    if comm is not None and comm.world > 1:
        raise NotImplementedError("ht_1d_joint on a gene-sharded run: the results are not gathered across ranks")
    trt, trt_names = _joint_block(m, treatment, 'treatment')
    cov, cov_names = _joint_block(m, covariate, 'covariate')
    mv = _ht.moments_view(m)
    ng = mv.ng
    names = _var_names(adata)
    G_all = len(st.gene_idx)
    if st.sf_bin is None:
        raise NotImplementedError("more than 255 size-factor bins")
    if max_rows is None:
        max_rows = engine.auto_max_rows(num_boot + 1, arrays=2)
    chunk = max(1, int(max_rows) // max(1, ng))
    # stream keys as in ht_1d_moments: the refill by the gene's position in the unfiltered gene order, rng='fast' by its position
    # among the kept genes
    fill_pos = (np.asarray(st.shard, dtype=np.int64)[st.gene_idx] if getattr(st, 'shard', None) is not None
                else np.asarray(st.gene_idx, dtype=np.int64))
    cols = {k: [] for k in ('mean_stat', 'mean_asl', 'var_stat', 'var_asl', 'df', 'n_valid')}
    st.last_bootstrap = st.last_good = None    # (see ht_1d_moments: free the previous call's replicate rows first)

    def run_chunk(c):
        g0, g1 = c.g0, c.g1
        keys = (fill_pos[g0:g1, None] * ng + np.arange(ng)[None, :]).reshape(-1)
        good, _ = _ht.run_chunk_1d(c, mv, rng, fill_seed, keys, np.arange(g0 * ng, g1 * ng, dtype=np.int64))
        st.last_good = good
        tables = _ht.joint_tables(good, cov, trt, mv.Nc_list)
        st.last_joint_tables = tables          # (diagnostics / tests: the designs of the last gene chunk)
        st_m, st_v = c.bs.joint(np.arange(c.G), tables)
        for tag, stt in (('mean', st_m), ('var', st_v)):
            cols[tag + '_stat'].append(stt[:, 0])
            cols[tag + '_asl'].append(joint_pvalues(stt, approx))
        cols['df'].append(tables.design_rank[tables.test_design].astype(np.int64))
        cols['n_valid'].append(st_m[:, 2].astype(np.int64))

    for c in _ht.chunks_1d(st, mv, num_boot, chunk):
        run_chunk(c)
    out = {k: (np.concatenate(v) if v else np.zeros(0, dtype=np.int64 if k in ('df', 'n_valid') else np.float64)) for k, v in cols.items()}
    m['1d_ht_joint'] = dict(out, treatment=trt_names, covariate=cov_names)
    return pd.DataFrame({'gene': names[:G_all], 'df': out['df'], 'de_stat': out['mean_stat'], 'de_pval': out['mean_asl'],
                         'dv_stat': out['var_stat'], 'dv_pval': out['var_asl']})


def ht_1d_eqtl(adata, genotypes, gene_snp_pairs, covariate=None, num_boot=5000, num_cpus=1, rng='replay', fill_seed=0, max_rows=None,
               approx=False, resampling='bootstrap', resample_rep=False, adjust=False, interaction=None, **not_offered):
    """cis-eQTL scan: every kept gene against its own list of SNPs, hundreds per gene (the reference's largest analysis,
    analysis/lupus/run_memento.py:29-52, :84-109: one group per donor, ``treatment_for_gene``, ``resample_rep=True``).

    ``genotypes``: DataFrame [groups][SNPs] in the group order of ``uns['memento']['groups']`` (what ``treatment`` is to
    ``ht_1d_moments``); ``gene_snp_pairs``: a dict gene -> list of genotype columns (what ``treatment_for_gene`` is), or a
    two-column frame (gene, snp).  Genes that are not kept are ignored, a kept gene without a list has no test, an unknown SNP
    raises ValueError.  ``covariate``: DataFrame / array [groups][C], or None.

    The tests are those of ``ht_1d_moments(adata, covariate, genotypes, treatment_for_gene=..., ...)`` -- the same bootstrap
    (``rng``, ``fill_seed``, ``max_rows``, the hash uniforms from the global ``np.random`` stream, the same stream keys), the same
    designs, coefficients bit for bit in a one-chunk call -- but no coefficient row is stored per test: the device memory of the
    call grows with tests x groups, not with tests x replicates.  The resampled tests (``resample_rep=True``, treatment not all
    ones) run gene-major (mm_cross_resampled_block: a gene's draws are made once per tile of 8 SNPs, not once per SNP), the plain
    tests as design contrasts (``contrast_design``); the few rows that the tail fits of ``approx=False`` read are produced on
    demand in slices of a bounded scratch.  The device draws of ``resample_rep`` are keyed by the gene's position among the kept
    genes, so -- unlike ``ht_1d_moments`` there -- the result does not depend on ``max_rows``.

    ``adjust=True`` adds a GENE-LEVEL correction over the gene's whole SNP list, the one FastQTL / TensorQTL make with
    permutations: the single-step max-T of ``ht_1d_posthoc`` with the gene's tests as the family (centred null, so it needs
    ``resampling='bootstrap'``: ValueError otherwise).  Replicate column c of all SNPs of a gene is one joint draw -- the plain
    tests share the gene's replicate rows, the resampled tests share the draws, which are keyed by the gene -- so with
    M[c] = max_j |coef_j[c] - coef_j[0]| / se_j over the included members (those with a test) on the columns valid for all of
    them,  p_adj_j = (1 + #{c : M[c] > |coef_j[0]| / se_j}) / (1 + n_valid);  ``*_pval_adj`` is max(p_adj_j, the SNP's own p-value)
    and NaN for a member without a test, ``n_family`` the number of included members (mean plane; ``var_n_family`` in ``uns``).
    With ``resample_rep=False`` the family is all the gene's tests (``family_maxt`` on the weight-row designs); with
    ``resample_rep=True`` it is the gene's RESAMPLED tests (mm_cross_resampled_family), and the few plain tests of such a call
    (treatment all ones) are no joint draws with them: they get NaN adjusted values and do not count in ``n_family``.  A family
    never spans gene chunks and ``max_rows`` changes no bit.  ``get_eqtl_gene_result`` turns the result into an eGene table.

    ``interaction``: one finite value per group (array, Series or one-column frame, in the group order; more than one column or a
    wrong length: ValueError) -- a context ``ctx`` such as stimulated / control, cell type or dose.  Every (gene, SNP) test is then of
    the GENOTYPE-BY-CONTEXT term of  y ~ 1 + covariate + ctx + g_s + g_s * ctx  (a response eQTL): ``ctx`` joins the shared covariates
    (the hat matrix is a pseudo-inverse, so passing it in ``covariate`` as well changes nothing), the genotype main effect g_s is a
    covariate of the test's own, taken out by a rank-one step on the device (mm_cross_resampled_block_cov), and the coefficient
    columns hold the interaction coefficient.  A pair gets NO TEST (NaN coef / se / p-value, outside any family) where the fully
    residualised treatment has a weighted sum of squares <= ``design.SS_DEGENERATE`` on the gene's good groups (carriers in one
    context only, a monomorphic SNP, a constant context) or the treatment is all ones; a genotype inside the span of the shared
    covariates counts as no covariate.  The rows, their order and every other argument are those of the plain call, and
    ``adjust=True`` with ``resample_rep=False`` takes the gene's interaction tests as the family.  ``None``: the plain call.

    Not offered: ``strict``, ``ci``, ``max_boot``, ``treatment_for_gene`` (TypeError), a gene-sharded run (NotImplementedError), and
    ``adjust=True`` together with ``resample_rep=True`` and ``interaction`` (NotImplementedError: the family kernel would need the
    rank-one coefficients of a whole gene at once).

    Returns a DataFrame (gene, snp, de_coef, de_se, de_pval, dv_coef, dv_se, dv_pval), gene-major over the kept genes, each gene's
    SNPs in its list order; with ``adjust=True`` also de_pval_adj, dv_pval_adj and n_family, after these.  The arrays go to
    ``uns['memento']['1d_ht_eqtl']`` (``mean_asl_adj``, ``var_asl_adj``, ``n_family``, ``var_n_family`` for the adjusted ones)."""
    if not_offered:
        raise TypeError(f"ht_1d_eqtl does not offer {sorted(not_offered)[0]!r}")
    _ht.check_args(rng, resampling=resampling)
    resample_rep, approx, adjust = bool(resample_rep), bool(approx), bool(adjust)
    if adjust and resampling != 'bootstrap':
        raise ValueError("ht_1d_eqtl(adjust=True) needs resampling='bootstrap': the max-T null is centred on the observed coefficient")
    if interaction is not None and adjust and resample_rep:
        raise NotImplementedError("ht_1d_eqtl(interaction=..., adjust=True, resample_rep=True): the resampled family needs the "
                                  "per-test covariate's coefficients of a whole gene at once")
    m = adata.uns['memento']
    ctx = None if interaction is None else _ht.interaction_context(interaction, len(m['groups']))
    st = m['_hip']
    comm = getattr(st, 'comm', None)
    if comm is not None and comm.world > 1:
        raise NotImplementedError("ht_1d_eqtl on a gene-sharded run: the results are not gathered across ranks")
    mv = _ht.moments_view(m)
    ng = mv.ng
    names = _var_names(adata)
    G_all = len(st.gene_idx)
    if not isinstance(genotypes, pd.DataFrame) or len(genotypes) != ng:
        raise ValueError(f"genotypes must be a DataFrame with one row per group ({ng})")
    trt_all = np.asarray(genotypes.values, dtype=np.float64)
    cov = np.ones((ng, 0)) if covariate is None else np.asarray(getattr(covariate, 'values', covariate), dtype=np.float64).reshape(ng, -1)
    gene_cols = _ht.eqtl_gene_columns(genotypes, gene_snp_pairs, names[:G_all])
    snp_names = np.asarray(genotypes.columns, dtype=object)
    if st.sf_bin is None:
        raise NotImplementedError("more than 255 size-factor bins")
    fill_pos = (np.asarray(st.shard, dtype=np.int64)[st.gene_idx] if getattr(st, 'shard', None) is not None
                else np.asarray(st.gene_idx, dtype=np.int64))
    cols = {k: [] for k in ('mean_coef', 'mean_se', 'mean_asl', 'var_coef', 'var_se', 'var_asl')}
    if adjust:
        cols.update({k: [] for k in ('mean_asl_adj', 'mean_n_family', 'var_asl_adj', 'var_n_family')})

    def run_chunk(c):
        g0, g1, G, bs = c.g0, c.g1, c.G, c.bs
        keys = (fill_pos[g0:g1, None] * ng + np.arange(ng)[None, :]).reshape(-1)          # the stream keys of ht_1d_moments
        good, n_inv = _ht.run_chunk_1d(c, mv, rng, fill_seed, keys, np.arange(g0 * ng, g1 * ng, dtype=np.int64))
        refilled = ((n_inv > 0).any(axis=1) & ~c.skip).reshape(G, ng).any(axis=1)
        rs = st.refill_stats
        rs['chains'] += int(((~c.skip) & (bs.K >= 2)).sum())
        rs['chains_refilled'] += int(((n_inv > 0).any(axis=1) & ~c.skip).sum())
        rs['genes'] += G
        rs['genes_refilled'] += int(refilled.sum())
        rs['gene_refilled'][g0:g1] = refilled
        if ctx is None:
            d = _ht.eqtl_tables(good, gene_cols[g0:g1], cov, trt_all, mv.Nc_list, resampled=resample_rep)
            zt_mat = None
        else:                                                     # no test: a zero weight row (a record that is no family member)
            d = _ht.eqtl_interaction_tables(good, gene_cols[g0:g1], cov, ctx, trt_all, mv.Nc_list)
            d.rr_test, zt_mat = d.has_test, d.zt_mat
        n_tests = len(d.test_row)
        no_group = ~good[d.test_row].any(axis=1)
        if ctx is not None:
            no_group = no_group | ~d.has_test
        is_rr = d.rr_test if resample_rep else np.zeros(n_tests, dtype=bool)
        rr_idx, pl_idx = np.flatnonzero(is_rr), np.flatnonzero(~is_rr)
        local = np.zeros(n_tests, dtype=np.int64)                 # a test's number inside its part
        local[rr_idx], local[pl_idx] = np.arange(len(rr_idx)), np.arange(len(pl_idx))
        stats = [np.full((n_tests, 8), np.nan), np.full((n_tests, 8), np.nan)]
        parts = []
        # adjust: (t0, n_adj) per test and plane, (n_valid_family, n_included) per gene and plane; a test outside the family is (NaN, 0)
        adj, fam = np.zeros((n_tests, 2, 2)), np.zeros((G, 2, 2))
        adj[:, :, 0] = np.nan
        if len(pl_idx):                                           # plain tests: the weight rows as design contrasts, records only
            tables = (d.test_row[pl_idx], *_ht.weight_row_designs(d.test_row[pl_idx], d.Wmat[pl_idx], good))
            st_m, st_v, rows_pl = bs.contrast_design(*tables)
            stats[0][pl_idx], stats[1][pl_idx] = st_m, st_v
            parts.append((~is_rr, rows_pl))
            if adjust and not resample_rep:                       # the family of a gene: all its tests, on the rows they share
                scale = engine.family_scale(st_m, st_v)
                scale[no_group[pl_idx]] = 0.0
                _, adj, fam = bs.family_maxt(d.gene_ptr, *tables, scale)
                st.last_eqtl = SimpleNamespace(gene_ptr=d.gene_ptr, tables=tables, scale=scale, adj=adj, fam=fam, rows=rows_pl, n_valid=None)
        if len(rr_idx):                                           # resampled tests: gene-major, keyed by the gene's position
            col_map, n_valid = _ht.surviving_cols(bs, good, num_boot)                                     # hypothesis_test.py:249-251
            rr_ptr = np.concatenate([[0], np.cumsum(np.bincount(d.test_row[rr_idx], minlength=G))])
            block = bs.cross_resampled_family if adjust else bs.cross_resampled_block
            per_test = {} if zt_mat is None else dict(zt=zt_mat[rr_idx])
            st_m, st_v, rows_rr, *family = block(rr_ptr, d.tt_mat[rr_idx], good, d.row_mask, d.Mstack, mv.Nc_list, seed=fill_seed + 17,
                                                 col_map=col_map, n_valid=n_valid, gene_key=np.arange(g0, g1, dtype=np.int64), **per_test)
            stats[0][rr_idx], stats[1][rr_idx] = st_m, st_v
            parts.append((is_rr, rows_rr))
            if adjust:                                            # the family of a gene: its resampled tests, which share the draws
                scale = engine.family_scale(st_m, st_v)
                _, adj_rr, fam = family[0](scale)
                adj[rr_idx] = adj_rr
                st.last_eqtl = SimpleNamespace(gene_ptr=rr_ptr, rr_idx=rr_idx, scale=scale, adj=adj_rr, fam=fam, rows=rows_rr, n_valid=n_valid)
        for which, tag in ((0, 'mean'), (1, 'var')):
            stt = stats[which]
            fetch = lambda idx, w=which: _ht.sliced_rows([(mem, local, functools.partial(r, w)) for mem, r in parts], idx, bs.ld)
            p = _asl.asl_from_stats(stt, approx, fetch, num_cpus, resampling)
            c0, se = stt[:, 0].copy(), stt[:, 1].copy()
            c0[no_group], se[no_group], p[no_group] = np.nan, np.nan, np.nan                              # hypothesis_test.py:203-204
            cols[tag + '_coef'].append(c0)
            cols[tag + '_se'].append(se)
            cols[tag + '_asl'].append(p)
            if adjust:
                p_adj, n_family, _ = _ht.adjusted_columns(p, adj[:, which], fam[:, which], np.diff(d.gene_ptr))
                cols[tag + '_asl_adj'].append(p_adj)
                cols[tag + '_n_family'].append(n_family)

    st.refill_stats = dict(chains=0, chains_refilled=0, genes=0, genes_refilled=0, gene_refilled=np.zeros(G_all, dtype=bool))
    st.last_bootstrap = st.last_eqtl = None    # (see ht_1d_moments: free the previous call's replicate rows first)
    if max_rows is None:
        max_rows = engine.auto_max_rows(num_boot + 1, arrays=2)
    for c in _ht.chunks_1d(st, mv, num_boot, max(1, int(max_rows) // max(1, ng))):
        run_chunk(c)
    out = {k: (np.concatenate(v) if v else np.zeros(0, dtype=np.int64 if k.endswith('_n_family') else np.float64)) for k, v in cols.items()}
    if adjust:
        out['n_family'] = out.pop('mean_n_family')
    n_snps = np.array([len(k) for k in gene_cols], dtype=np.int64)
    flat = np.array([j for k in gene_cols for j in k], dtype=np.int64)
    df = pd.DataFrame({'gene': np.repeat(np.asarray(names[:G_all], dtype=object), n_snps), 'snp': snp_names[flat]})
    m['1d_ht_eqtl'] = dict(out, gene=df['gene'].values, snp=df['snp'].values)
    if ctx is not None:
        m['1d_ht_eqtl'].update(interaction=True, context=ctx)
    df['de_coef'], df['de_se'], df['de_pval'] = out['mean_coef'], out['mean_se'], out['mean_asl']
    df['dv_coef'], df['dv_se'], df['dv_pval'] = out['var_coef'], out['var_se'], out['var_asl']
    if adjust:
        df['de_pval_adj'], df['dv_pval_adj'], df['n_family'] = out['mean_asl_adj'], out['var_asl_adj'], out['n_family']
    return df


def get_eqtl_gene_result(adata):
    """The eGene table of the last ``ht_1d_eqtl(adjust=True)`` call (host only): one row per kept gene that has a SNP list, in the
    order of the tests.  ``gene``, ``n_snps`` (the list's length), ``n_family`` (included members, mean plane); per plane
    (``de`` / ``dv``) the LEAD SNP -- the included member with the largest |coef| / se, the first of equals --, its
    ``*_coef``, ``*_se``, ``*_pval``, the gene-level ``*_gene_pval`` = the smallest ``*_pval_adj`` of the gene (the lead SNP's, unless
    the tail fit of another member's own p-value lifted it), and ``*_gene_qval`` = Benjamini-Hochberg (``util._fdrcorrect``) over
    the genes.  A gene without an included member on a plane has None / NaN there and q = 1.  ValueError if the stored result
    has no adjusted arrays."""
    ht = adata.uns['memento'].get('1d_ht_eqtl')
    if ht is None or 'mean_asl_adj' not in ht:
        raise ValueError("get_eqtl_gene_result needs the result of ht_1d_eqtl(adjust=True)")
    gene = np.asarray(ht['gene'], dtype=object)
    first = np.flatnonzero(np.r_[True, gene[1:] != gene[:-1]]) if len(gene) else np.zeros(0, dtype=np.int64)
    ptr = np.r_[first, len(gene)]
    df = pd.DataFrame({'gene': gene[first], 'n_snps': np.diff(ptr), 'n_family': np.asarray(ht['n_family'])[first]})
    for name, tag in (('de', 'mean'), ('dv', 'var')):
        coef, se, p, p_adj = (np.asarray(ht[tag + k], dtype=np.float64) for k in ('_coef', '_se', '_asl', '_asl_adj'))
        with np.errstate(invalid='ignore', divide='ignore'):
            t0 = np.where(np.isnan(p_adj), np.nan, np.abs(coef) * (1.0 / se))
        lead = np.full(len(first), -1, dtype=np.int64)
        gene_p = np.full(len(first), np.nan)
        for k, (lo, hi) in enumerate(zip(ptr[:-1], ptr[1:])):
            if not np.isnan(t0[lo:hi]).all():
                lead[k] = lo + np.nanargmax(t0[lo:hi])
                gene_p[k] = np.nanmin(p_adj[lo:hi])
        has = lead >= 0
        df[name + '_lead_snp'] = [ht['snp'][j] if ok else None for j, ok in zip(lead, has)]
        for col, a in (('_coef', coef), ('_se', se), ('_pval', p)):
            df[name + col] = np.where(has, a[np.maximum(lead, 0)] if len(a) else np.nan, np.nan)
        df[name + '_gene_pval'] = gene_p
        df[name + '_gene_qval'] = util._fdrcorrect(gene_p)
    return df


def _posthoc_plan(m, treatment_col, control):
    """What ``ht_1d_posthoc`` tests: (``_ht.PosthocDesigns``, the level names).  Without ``treatment_col`` a level is a group
    (``control``: a group label or index); with it, a value of that label column (``control``: such a value, compared as a string)."""
    groups = m['groups']
    Nc = np.array([m['group_cells'][g].shape[0] for g in groups], dtype=np.float64)
    labels = [g.split(m['label_delimiter'])[1:] for g in groups]
    if treatment_col is None:
        if control is not None:
            if not isinstance(control, (int, np.integer)) and control not in groups:
                raise ValueError(f"control {control!r} is not one of the groups")
            control = groups.index(control) if not isinstance(control, (int, np.integer)) else int(control)
            if not 0 <= control < len(groups):
                raise ValueError(f"control index {control!r} is not one of the {len(groups)} groups")
        return _ht.PosthocDesigns(labels, None, control, Nc), list(groups)
    label_columns = list(m['label_columns'])
    if treatment_col not in label_columns:
        raise ValueError(f"treatment_col {treatment_col!r} is not one of the label columns {label_columns}")
    designs = _ht.PosthocDesigns(labels, label_columns.index(treatment_col), None if control is None else str(control), Nc)
    return designs, designs.levels


def ht_1d_posthoc(adata, treatment_col=None, control=None, num_boot=10000, num_cpus=1, rng='replay', fill_seed=0, max_rows=None,
                  approx=False, *, ci=None):
    """WHICH levels of a factor differ: the pairwise contrasts between the levels for every kept gene, each with its own test and
    with a p-value adjusted for the gene's whole family of contrasts (``ht_1d_joint`` answers whether the gene differs at all).

    Levels and strata are those of ``ht_1d_vs_control``.  ``treatment_col=None``: every group is a level and a contrast is the
    plain two-group difference.  ``treatment_col='x'`` (a label column of ``create_groups``): the levels are the values of that
    column and every other label column is a covariate; the test of level a against level b is EXACTLY the test
    ``ht_1d_vs_control(control=b, treatment_col='x')`` makes of a -- the same subset regression, the same weight row, and with the same
    ``np.random`` seed, ``fill_seed`` and ``max_rows`` the same numbers.  ``control=None``: the family of a gene is all unordered
    pairs of levels (the Tukey form); levels are in first-appearance order, the pair (level_a, level_b) has a after b, and rows
    are ordered by b, then a.  ``control=value``: every other level against that one (the Dunnett form).

    The adjustment is the single-step max-T of Westfall and Young within the gene's family.  Every (gene, group) chain is
    bootstrapped once, so replicate column c of all contrasts of a gene is one joint draw of the family.  A member is INCLUDED when
    it has a test (finite coefficient, finite se > 0, a valid replicate, replicates that are not all equal); with
    t_j[c] = |coef_j[c] - coef_j[0]| / se_j and M[c] = max_j t_j[c] over the included members, on the replicate columns that are
    valid for all of them,  p_adj_j = (1 + #{c : M[c] > |coef_j[0]| / se_j}) / (1 + n_valid).  There is no tail fit: the floor is
    1 / (n_valid + 1).  The reported ``*_pval_adj`` is max(p_adj_j, the member's own p-value), so it is never below the
    unadjusted one whatever ``approx`` and the tail fit did to that.  A member without a test has NaN adjusted values and does not
    enter the maximum: a gene that lost a whole level keeps the family of its other levels.  ``n_family`` is the number of
    included members of the gene's family on the mean plane (``var_n_family`` in ``uns``: the variability plane).

    ``ci=level`` (0 < level < 1) adds simultaneous intervals: crit = np.nanquantile(M[1:], level) and
    coef_j[0] -+ crit * se_j, which cover all members of the family at once: ``de_sci_lo, de_sci_hi, dv_sci_lo, dv_sci_hi``.

    ``rng``, ``fill_seed``, ``max_rows``, ``num_cpus`` and ``approx`` as in ``ht_1d_vs_control``; genes run in chunks, a family never
    spans chunks and the chunking changes no number.  Not offered: ``resampling`` other than the centred bootstrap,
    ``resample_rep``, ``strict`` and ``treatment_for_gene``; a gene-sharded run raises NotImplementedError.

    Returns a DataFrame (gene, level_a, level_b, de_coef, de_se, de_pval, de_pval_adj, dv_coef, dv_se, dv_pval, dv_pval_adj,
    n_family) and stores the arrays in ``uns['memento']['1d_ht_posthoc']``."""
    _ht.check_args(rng, resampling='bootstrap')
    _ht.ci_probs(ci)
    m = adata.uns['memento']
    st = m['_hip']
    comm = getattr(st, 'comm', None)
    if comm is not None and comm.world > 1:
        raise NotImplementedError("ht_1d_posthoc on a gene-sharded run: the results are not gathered across ranks")
    designs, level_names = _posthoc_plan(m, treatment_col, control)
    pairs = designs.pairs
    n_mem = len(pairs)
    if n_mem == 0:
        raise ValueError("ht_1d_posthoc needs at least two levels")
    mv = _ht.moments_view(m)
    ng = mv.ng
    names = _var_names(adata)
    G_all = len(st.gene_idx)
    if max_rows is None:
        max_rows = engine.auto_max_rows(num_boot + 1, arrays=2)
    chunk = max(1, int(max_rows) // max(1, ng))
    cols = {tag + k: [] for tag in ('mean', 'var') for k in ('_coef', '_se', '_asl', '_asl_adj', '_n_family')}
    if ci is not None:
        cols.update(mean_sci=[], var_sci=[])
    st.last_bootstrap = st.last_good = st.last_posthoc = None    # (see ht_1d_moments: free the previous call's replicate rows first)

    def run_chunk(c):
        G, bs = c.G, c.bs
        keys = np.arange(c.g0 * ng, c.g1 * ng, dtype=np.int64)      # the keys of ht_1d_vs_control: the same replicate planes
        good, _ = _ht.run_chunk_1d(c, mv, rng, fill_seed, keys, keys)
        st.last_good = good
        test_gene = np.repeat(np.arange(G), n_mem)
        family_ptr = np.arange(G + 1, dtype=np.int64) * n_mem
        tables = (test_gene, designs.tests(good), *designs.tables())
        st_m, st_v, rows = bs.contrast_design(*tables)
        scale = engine.family_scale(st_m, st_v)
        maxrow, adj, fam = bs.family_maxt(family_ptr, *tables, scale)
        st.last_posthoc = SimpleNamespace(family_ptr=family_ptr, tables=tables, scale=scale, adj=adj, fam=fam)   # (diagnostics / tests: the last gene chunk)
        if ci is not None:
            q, _ = engine.row_quantiles(maxrow.reshape(-1, bs.ld), bs.ld, num_boot, [float(ci)])
            crit = engine.host(q).reshape(G, 2)
        for k, (tag, stt) in enumerate((('mean', st_m), ('var', st_v))):
            p = _asl.asl_from_stats(stt, approx, lambda idx, w=k: rows(w, idx), num_cpus, 'bootstrap')
            p_adj, n_family, half = _ht.adjusted_columns(p, adj[:, k], fam[:, k], n_mem, stt[:, 1], crit[:, k] if ci is not None else None)
            cols[tag + '_coef'].append(stt[:, 0])
            cols[tag + '_se'].append(stt[:, 1])
            cols[tag + '_asl'].append(p)
            cols[tag + '_asl_adj'].append(p_adj)
            cols[tag + '_n_family'].append(n_family)
            if ci is not None:
                cols[tag + '_sci'].append(np.column_stack([stt[:, 0] - half, stt[:, 0] + half]))

    for c in _ht.chunks_1d(st, mv, num_boot, chunk):
        run_chunk(c)

    def empty_of(k):
        return np.zeros((0, 2) if k.endswith('_sci') else 0, dtype=np.int64 if k.endswith('_n_family') else np.float64)

    out = {k: (np.concatenate(v) if v else empty_of(k)) for k, v in cols.items()}
    out['n_family'] = out.pop('mean_n_family')
    level_a = [level_names[a] for a, _ in pairs]
    level_b = [level_names[b] for _, b in pairs]
    m['1d_ht_posthoc'] = dict(out, levels=list(level_names), level_a=level_a, level_b=level_b, treatment_col=treatment_col,
                              control=None if control is None else level_b[0])
    df = pd.DataFrame({'gene': np.repeat(names[:G_all], n_mem), 'level_a': np.tile(np.asarray(level_a, dtype=object), G_all),
                       'level_b': np.tile(np.asarray(level_b, dtype=object), G_all)})
    df['de_coef'], df['de_se'], df['de_pval'], df['de_pval_adj'] = out['mean_coef'], out['mean_se'], out['mean_asl'], out['mean_asl_adj']
    df['dv_coef'], df['dv_se'], df['dv_pval'], df['dv_pval_adj'] = out['var_coef'], out['var_se'], out['var_asl'], out['var_asl_adj']
    df['n_family'] = out['n_family']
    if ci is not None:
        m['1d_ht_posthoc']['ci'] = float(ci)
        for name, a in (('de', out['mean_sci']), ('dv', out['var_sci'])):
            df[name + '_sci_lo'], df[name + '_sci_hi'] = a[:, 0], a[:, 1]
    return df


# ----------------------------------------------------------------------------------------------
# 2D: compute_2d_moments / ht_2d_moments / get_corr_matrix
# ----------------------------------------------------------------------------------------------


def _corr_from_cov(cov, var_1, var_2):
    """estimator._corr_from_cov (estimator.py:273-292): variances <= 0 become NaN (in place, as the
    reference does), entries without a finite sqrt(v1 v2) keep the 5.0 sentinel and are then clipped to 1."""
    corr = np.full(cov.shape, 5.0)
    var_1[var_1 <= 0] = np.nan
    var_2[var_2 <= 0] = np.nan
    vp = np.sqrt(var_1 * var_2)
    ok = np.isfinite(vp)
    corr[ok] = cov[ok] / vp[ok]
    corr[corr > 1] = 1
    corr[corr < -1] = -1
    return corr


def compute_2d_moments(adata, gene_pairs, inplace=True):
    """Covariance and correlation of the given gene pairs per group (reference: memento/main.py:293-338,
    estimator.py:207-233).  The only O(nnz) quantity, sum_c x_i x_j / sf^2, comes from mm_pair_cross; the
    means and the i == j correction reuse the 1D sums of compute_1d_moments."""
    if not inplace:
        adata = adata.copy()
    m = adata.uns['memento']
    st = m['_hip']
    if 'size_factor' not in m.keys():
        _bin_size_factor(adata)
    groups = m['groups']
    names = _var_names(adata)
    mapping = dict(zip(names, np.arange(len(names))))
    n_pairs = len(gene_pairs)
    idx1 = np.array([mapping[a] for a, _ in gene_pairs], dtype=int)
    idx2 = np.array([mapping[b] for _, b in gene_pairs], dtype=int)
    m['2d_moments'] = {'gene_pairs': gene_pairs, 'gene_idx_1': idx1, 'gene_idx_2': idx2}
    used = np.unique(np.concatenate([idx1, idx2])) if n_pairs else np.zeros(0, dtype=int)
    st.cols = engine.GeneColumns(st.blocks, st.gene_idx[used])          # columns of the genes in the pair list
    st.cols_local = used
    slot = {int(g): i for i, g in enumerate(used)}
    c1 = np.array([slot[int(i)] for i in idx1], dtype=np.int64)
    c2 = np.array([slot[int(j)] for j in idx2], dtype=np.int64)
    prod = engine.pair_cross(st.cols, c1, c2, 1.0 / adata.obs['memento_size_factor'].values)   # [n_groups][n_pairs]
    Nc = st.blocks.grp_ncells.astype(np.float64)
    same = idx1 == idx2
    g1, g2 = st.gene_idx[idx1], st.gene_idx[idx2]
    for gi, group in enumerate(groups):
        q = m['group_q'][group]
        p = prod[gi] / Nc[gi]
        if same.any():
            p[same] = p[same] - (1 - q) * st.S[2][gi, g1[same]] / Nc[gi]                       # estimator.py:229-230
        cov = p - (st.S[0][gi, g1] / Nc[gi]) * (st.S[0][gi, g2] / Nc[gi])                      # estimator.py:231
        var_1 = m['1d_moments'][group][1][idx1]
        var_2 = m['1d_moments'][group][1][idx2]
        corr = _corr_from_cov(cov, var_1, var_2)
        m['2d_moments'][group] = {'cov': cov, 'corr': corr, 'var_1': var_1, 'var_2': var_2}
    if not inplace:
        return adata


def get_corr_matrix(adata, group):
    """All-by-all correlation matrix of one group (reference: memento/main.py:277-291,
    estimator._hyper_corr_symmetric estimator.py:236-270)."""
    m = adata.uns['memento']
    st = m['_hip']
    gi = m['groups'].index(group)
    G = len(st.gene_idx)
    cols = engine.GeneColumns(st.blocks, st.gene_idx)
    iu, ju = np.triu_indices(G)
    prod = engine.pair_cross(cols, iu, ju, 1.0 / adata.obs['memento_size_factor'].values)[gi]
    n = float(st.blocks.grp_ncells[gi])
    q = m['group_q'][group]
    P = np.zeros((G, G))
    P[iu, ju] = prod / n
    P[ju, iu] = prod / n
    d = np.arange(G)
    P[d, d] -= (1 - q) * st.S[2][gi, st.gene_idx] / n                                          # estimator.py:256
    mu = st.S[0][gi, st.gene_idx] / n
    cov = P - np.outer(mu, mu)
    var = m['1d_moments'][group][1]
    # estimator.py:259-263: the reference NaNs only fancy-index copies; var_prod comes from the untouched variances
    # (negative x negative -> finite product, negative x positive -> NaN, zero -> division by zero -> NaN below)
    with np.errstate(invalid="ignore", divide="ignore"):
        vp = np.sqrt(np.outer(var, var))
        corr = np.full(cov.shape, 5.0)
        ok = np.isfinite(vp)
        corr[ok] = cov[ok] / vp[ok]
    inside = (corr < 1.05) & (corr > -1.05)
    corr[inside] = np.clip(corr[inside], a_min=-1, a_max=1)
    corr[(corr > 1) | (corr < -1)] = np.nan
    return corr


def _replay_pair_draws(c, plan, uniforms, trt, tcol, per_gene, num_boot):
    """``ht_2d_moments(strict=True, resample_rep=True)``: the global-stream order of the reference for the pairs of chunk ``c``
    (_ht_2d :319-343, _regress_2d :395-398): per pair three uniforms per live group (into ``uniforms``), then -- unless the
    treatment of the good groups is all ones -- the two np.random.choice draws.  -> (rep_assign, bcol_assign), device pair order."""
    r1a, r1b, r0 = uniforms
    lo, n_ch, ng = c.lo, c.n_ch, plan.ng
    inv = np.empty(n_ch, dtype=np.int64)
    inv[c.so] = np.arange(n_ch)
    K_orig = c.bs.K.reshape(n_ch, ng)[inv]                                # bins per (pair, group), original pair order
    rep_assign = np.zeros((n_ch, ng, num_boot), dtype=np.int16)          # device pair order
    bcol_assign = np.zeros((n_ch, ng, num_boot), dtype=np.int32)
    for pi in range(n_ch):
        lv = ~plan.skip[lo + pi]
        idx = (lo + pi) * ng + np.flatnonzero(lv)
        uu = np.random.random(3 * len(idx))
        r1a[idx], r1b[idx], r0[idx] = uu[0::3], uu[1::3], uu[2::3]
        gd = lv & (K_orig[pi] >= 1)
        n = int(gd.sum())
        t_pi = trt[:, [tcol[lo + pi]]] if per_gene else trt
        if n and not (t_pi[gd] == 1).mean() == 1:
            ra = np.random.choice(n, size=(n, num_boot))
            ra[:, 0] = np.arange(n)
            ba = np.random.choice(num_boot, (n, num_boot)) + 1
            ba[:, 0] = 0
            rep_assign[inv[pi], :n], bcol_assign[inv[pi], :n] = ra, ba
    return rep_assign, bcol_assign


def ht_2d_moments(adata, covariate, treatment, treatment_for_gene=None, inplace=True, num_boot=10000, verbose=3, num_cpus=1,
                  max_rows=None, fill_seed=0, strict=False, rng='replay', ci=None, *, max_boot=None, min_extreme=10, **kwargs):
    """Bootstrap hypothesis test of correlation differences (reference: memento/main.py:418-520,
    hypothesis_test._ht_2d :303-364).  Same replay semantics as ht_1d_moments.
    ``rng='fast'``: same samplers and replicate arithmetic, but every (pair, group, replicate) has its own counter-derived
    PCG64 stream seeded by ``fill_seed`` (mm_boot2d_fast: one wave per 64 replicates of a chain instead of one lane per chain)
    -- statistically equivalent to the reference, not draw-identical.  The global ``np.random`` stream is consumed as with
    ``rng='replay'``, so the bins, their order, ``corr_coef``, the NaN pattern and the skip rules are the replay run's; the
    streams are keyed by the pair's position among the distinct tested pairs, so the result does not depend on ``max_rows``.
    ``resample_rep=True``
    (hypothesis_test.py:393-404): with ``strict=True`` the reference's two np.random.choice draws per pair are replayed from
    the global stream in pair order (exact agreement with the reference at num_cpus=1); otherwise the group /
    replicate-column assignments are drawn on the device (seeded by ``fill_seed``): statistically equivalent, not
    draw-identical.  Without resample_rep the 2D path consumes the global stream exactly like the reference either way.
    ``treatment_for_gene`` as the reference BEHAVES (main.py:492): a pair's treatment columns are looked up under
    ``frozenset({name of the pair's first gene})`` -- the key is built from idx_1 twice -- and one number per pair is stored,
    so the list must hold exactly one column (the reference raises ValueError on more); pinned by fixture ``api_tfg2d``.
    ``ci`` as in ``ht_1d_moments``: ``uns['memento']['2d_ht']['corr_ci']`` [pair][2] (NaN for skipped pairs) and ``['ci']``;
    ``get_2d_ht_result`` then has ``corr_ci_lo, corr_ci_hi``.
    ``max_boot`` / ``min_extreme`` (keyword-only; ``max_boot`` needs ``rng='fast'``, ``approx=False``, ``ci=None`` and no
    ``resample_rep``): the sequential bootstrap of ``ht_1d_vs_control`` on the pair tests.  Round 0 is the plain call -- the same
    launches, keys and records -- and only the tests whose extreme count is still <= ``min_extreme`` go on, to the cumulative
    totals ``num_boot``, ``2 num_boot``, ..., ``max_boot`` (``_ht.sequential_schedule``); a round bootstraps only the chains of the
    good groups of the pairs with an open test (``_ht.continue_chunk_2d``).  The streams are keyed by (``fill_seed``, pair, group,
    replicate) and the 2D path refills nothing, so a test that is never closed has exactly the valid / extreme counts of the
    one-shot ``num_boot=max_boot`` call.  ``corr_asl`` is ``(c + 1) / (n + 1)`` over all rounds for every test, with NO tail fit;
    ``corr_se`` comes from the merged record (``_ht.merge_records``); ``corr_coef`` is untouched.  Adds ``corr_nboot`` [pair] (the
    valid replicates behind each p-value, 0 where there is no test), ``max_boot`` and ``min_extreme`` to ``uns['memento']['2d_ht']``;
    ``get_2d_ht_result`` then has a ``corr_nboot`` column.  Nothing here is rank-aware: pair blocks are sharded by the caller."""
    resampling, resample_rep, approx = _ht.check_args(rng, strict, **kwargs)
    sequential = _ht.check_sequential(max_boot, min_extreme, num_boot, rng, approx, ci)
    if sequential and resample_rep:
        raise ValueError("max_boot needs resample_rep=False: its replicate-column assignments are drawn over all columns of one "
                         "plane, which no round holds")
    probs = _ht.ci_probs(ci)
    if not inplace:
        adata = adata.copy()
    m = adata.uns['memento']
    st = m['_hip']
    comm = getattr(st, 'comm', None)
    if probs is not None and comm is not None and comm.world > 1:
        raise NotImplementedError("ci= on a run over several ranks: the intervals are not gathered across ranks")
    st.last_bootstrap2d = None                 # (free the previous call's replicate rows before this call allocates its own)
    Nc_list = np.array([m['group_cells'][g].shape[0] for g in m['groups']], dtype=np.float64)
    cov = np.asarray(covariate.values, dtype=np.float64)
    trt = np.asarray(treatment.values, dtype=np.float64)
    plan = _ht.pair_plan(m, st, num_boot, max_rows)
    tcol = np.zeros(plan.P_, dtype=np.int64)              # treatment column of every tested pair (column 0 without treatment_for_gene)
    per_gene = treatment_for_gene is not None
    if per_gene:
        names2, trt_cols = np.asarray(adata.var.index), list(treatment.columns)
        for k, c in enumerate(plan.first):
            cols = treatment_for_gene[frozenset({names2[int(plan.idx1[c])]})]
            if len(cols) != 1:
                raise ValueError("setting an array element with a sequence.")          # what main.py:507 does with more columns
            tcol[k] = trt_cols.index(cols[0])
    replay_rr = resample_rep and strict                   # the choice draws interleave with the hash uniforms, pair by pair
    uniforms = np.zeros((3, plan.P_ * plan.ng)) if replay_rr else _ht.hash_uniforms(~plan.skip.reshape(-1), 3)
    corr_coef, corr_se, corr_asl = (np.full(plan.n_conv, np.nan) for _ in range(3))
    corr_ci = np.full((plan.n_conv, 2), np.nan) if probs is not None else None
    if sequential:
        corr_nboot = np.zeros(plan.n_conv, dtype=np.int64)
        schedule = _ht.sequential_schedule(num_boot, max_boot)
        st.last_sequential = SimpleNamespace(schedule=schedule, n_open=[0] * len(schedule))   # (diagnostics: tests open after each round)

    def run_chunk(c):
        bs = c.bs
        rep_assign = bcol_assign = None
        if replay_rr:
            rep_assign, bcol_assign = _replay_pair_draws(c, plan, uniforms, trt, tcol, per_gene, num_boot)
        good = _ht.run_chunk_2d(c, plan, uniforms, rng, fill_seed, keep_fast=sequential)   # device order
        d = _ht.pair_design_tables(good, tcol[c.lo:c.hi][c.so], per_gene, cov, trt, Nc_list, resampled=resample_rep)
        coef, stt = bs.contract(d.test_row, d.Wmat, good)
        if sequential:
            del coef           # (the rounds' planes may take its buffer)
            stt = st.last_records2d = _ht.continue_chunk_2d(c, plan.ng, d.test_row, d.Wmat, good, stt, schedule, min_extreme, resampling,
                                                            st.last_sequential.n_open)
            for dst, src in ((corr_coef, stt[:, 0]), (corr_se, stt[:, 1]), (corr_asl, _ht.sequential_pvalues(stt, resampling)),
                             (corr_nboot, stt[:, 2].astype(np.int64))):
                _ht.scatter_pairs(c, plan, dst, src, keep=good.any(axis=1))
            return
        if resample_rep and d.rr_test.any():
            col_map, n_valid = _ht.surviving_cols(bs, good, num_boot)             # hypothesis_test.py:372-373
            if n_valid is not None and replay_rr:
                raise NotImplementedError("strict replay of resample_rep with non-finite correlation replicates")
            coef_r, stt_r = bs.contract_resampled(d.test_row, d.tt_mat, good, d.row_mask, d.Mstack, Nc_list, rep=rep_assign,
                                                  bcol=bcol_assign, seed=fill_seed + 17 + c.lo, col_map=col_map, n_valid=n_valid)
            coef, stt = _ht.merge_resampled(coef, stt, coef_r, stt_r, d.rr_test)
        st.last_records2d = stt                # (diagnostics / tests: the test records of the last pair chunk, device pair order)
        pvals = _asl.asl_from_stats(stt, approx, lambda idx: engine.host(coef[engine.dev(np.asarray(idx, dtype=np.int64))]), num_cpus, resampling)
        for dst, src in ((corr_coef, stt[:, 0]), (corr_se, stt[:, 1]), (corr_asl, pvals)):
            _ht.scatter_pairs(c, plan, dst, src, keep=good.any(axis=1))
        if probs is not None:
            _ht.scatter_pairs(c, plan, corr_ci, _ht.row_intervals(coef[:len(d.test_row)], bs.ld, num_boot, probs, stt[:, 0]),
                              keep=good.any(axis=1))

    for c in _ht.chunks_2d(st, plan, num_boot):
        run_chunk(c)
    m['2d_ht'] = {'treatment': treatment, 'covariate': covariate, 'corr_coef': corr_coef, 'corr_se': corr_se, 'corr_asl': corr_asl}
    if probs is not None:
        m['2d_ht']['corr_ci'], m['2d_ht']['ci'] = corr_ci, float(ci)
    if sequential:
        m['2d_ht'].update(corr_nboot=corr_nboot, max_boot=int(max_boot), min_extreme=int(min_extreme))
    if treatment_for_gene is not None:
        m['2d_ht']['treatment_for_gene'] = treatment_for_gene                      # main.py:513-514
    if not inplace:
        return adata


def ht_2d_vs_control(adata, control, num_boot=10000, num_cpus=1, fill_seed=0, max_rows=None, approx=False, resampling='bootstrap',
                     rng='replay', *, treatment_col=None, ci=None):
    """Perturb-seq style batch test of differential COEXPRESSION: the correlation of every pair of ``compute_2d_moments`` in
    every group against one shared ``control``, in one call.  ``control`` / ``treatment_col`` mean what they mean in
    ``ht_1d_vs_control``: without ``treatment_col`` a group label (or index) every other group is tested against; with it the
    groups are guide x stratum, ``control`` is a value of that column and every other label column is a covariate (the
    per-guide regression of the reference's loop -- subset to {guide, control}, create_groups([is_guide, *others]),
    compute_2d_moments, ht_2d_moments with intercept + main-effect dummies -- folded into weights by ``design.VsControlDesigns``).

    Every (pair, group) is bootstrapped once (``Bootstrap2D``: the control's pair histograms and chains, the largest ones, are
    not redone per guide) and the test statistic is taken per guide from the resident replicate correlations
    (mm_contrast_design1_stats): ``coef[c] = corr[pair, guide][c] - corr[pair, control][c]``, or the design's weighted sum over
    the guide's and the control's stratum groups.  The per-group correlation uses the global size factors and no mean-variance
    fit, so ``corr_coef`` equals the per-guide loop's wherever both use the same groups.  Pairs are handled as in
    ``ht_2d_moments`` (unordered duplicates share the first one's result, self pairs stay NaN, a (pair, group) with a NaN or
    +-1 correlation is skipped) and the global ``np.random`` stream is consumed as there (three uniforms per live
    (pair, group), pair-major, up front).  A test with no good guide or control group, or with no stratum holding both arms,
    is NaN.  ``rng='replay'|'fast'`` as in ``ht_2d_moments``: ``'fast'`` draws every (pair, group, replicate) from its own
    stream seeded by ``fill_seed`` (mm_boot2d_fast), with the same bins, ``corr_coef`` and NaN pattern as ``'replay'``.

    ``ci`` as in ``ht_1d_vs_control``: adds the columns ``corr_ci_lo, corr_ci_hi`` and ``corr_ci`` [test][2] and ``ci`` to ``uns``.

    The sequential bootstrap of these tests (``max_boot``) is ``ht_2d_vs_control_sequential``, of which this call is the case
    without ``max_boot``: the parameter list of this one is pinned.

    Returns a DataFrame (gene_1, gene_2, group, corr_coef, corr_se, corr_pval), pair-major, one row per (requested pair,
    tested guide), and stores the arrays in ``uns['memento']['2d_ht_vs_control']``."""
    return ht_2d_vs_control_sequential(adata, control, num_boot, num_cpus, fill_seed, max_rows, approx, resampling, rng,
                                       treatment_col=treatment_col, ci=ci)


def ht_2d_vs_control_sequential(adata, control, num_boot=10000, num_cpus=1, fill_seed=0, max_rows=None, approx=False,
                                resampling='bootstrap', rng='replay', *, treatment_col=None, ci=None, max_boot=None, min_extreme=10):
    """``ht_2d_vs_control`` with the sequential bootstrap: the same parameters, tests, result and ``uns`` entry
    (``'2d_ht_vs_control'``), and two more keywords; without ``max_boot`` it IS that call.

    ``max_boot`` / ``min_extreme`` (keyword-only; ``max_boot`` needs ``rng='fast'``, ``approx=False``, ``ci=None``): the sequential
    bootstrap of ``ht_1d_vs_control`` on the (pair, guide) tests.  Round 0 is the plain call -- the same launches, keys and records
    -- and only the tests whose extreme count is still <= ``min_extreme`` go on, to the cumulative totals ``num_boot``,
    ``2 num_boot``, ..., ``max_boot`` (``_ht.sequential_schedule``).  A round bootstraps exactly the chains that an open test's
    design reads (the guide's groups and the control's, not every group of the pair) into a compact plane of one row per chain,
    with a launch over the list of those chains (mm_boot2d_fast_slots), and contracts the open tests only
    (``_ht.continue_chunk_2d_designs``).  The streams are keyed by (``fill_seed``, pair, group, replicate) and the 2D path refills
    nothing, so a test that is never closed has exactly the valid / extreme counts of the one-shot ``num_boot=max_boot`` call,
    whatever ``max_rows`` is.  ``corr_pval`` is ``(c + 1) / (n + 1)`` over all rounds for every test, with NO tail fit; ``corr_se``
    comes from the merged record (``_ht.merge_records``); ``corr_coef`` is untouched.  Adds the column ``corr_nboot`` (the valid
    replicates behind each p-value, 0 where there is no test) and ``corr_nboot``, ``max_boot``, ``min_extreme`` to ``uns``.

    Returns a DataFrame (gene_1, gene_2, group, corr_coef, corr_se, corr_pval), pair-major, one row per (requested pair,
    tested guide), and stores the arrays in ``uns['memento']['2d_ht_vs_control']``."""
    _ht.check_args(rng, resampling=resampling)
    sequential = _ht.check_sequential(max_boot, min_extreme, num_boot, rng, approx, ci)
    probs = _ht.ci_probs(ci)
    m = adata.uns['memento']
    st = m['_hip']
    st.last_bootstrap2d = None                # (free the previous call's replicate rows before this call allocates its own)
    tested, designs, (ctrl, others), meta = _vs_control_plan(m, control, treatment_col)
    n_t = len(tested)
    plan = _ht.pair_plan(m, st, num_boot, max_rows)
    uniforms = _ht.hash_uniforms(~plan.skip.reshape(-1), 3)
    out = {k: np.full((plan.n_conv, n_t), np.nan) for k in ('corr_coef', 'corr_se', 'corr_asl')}
    corr_ci = np.full((plan.n_conv, n_t * 2), np.nan) if probs is not None else None
    if sequential:
        out['corr_nboot'] = np.zeros((plan.n_conv, n_t), dtype=np.int64)
        schedule = _ht.sequential_schedule(num_boot, max_boot)
        # (diagnostics: tests open after each round; chains bootstrapped per round; the last chunk's open mask before each round)
        seq = st.last_sequential = SimpleNamespace(schedule=schedule, n_open=[0] * len(schedule), n_chains=[0] * len(schedule), open_mask=None)
        two_group = _ht._TwoGroupDesigns(plan.ng, ctrl) if designs is None else None

    def run_chunk(c):
        good = _ht.run_chunk_2d(c, plan, uniforms, rng, fill_seed, keep_fast=sequential)   # device order
        test_pair = np.repeat(np.arange(c.n_ch), n_t)     # pair-major: a pair's control rows stay in L2 for its consecutive guides
        test_design = None if designs is None else designs.tests(good)
        stt, rows = (c.bs.contrast(test_pair, np.tile(others, c.n_ch), ctrl, good) if designs is None
                     else c.bs.contrast_design(test_pair, test_design, *designs.tables()))
        if sequential:
            del rows
            if designs is None:      # (the designs ``bs.contrast`` builds are those of _TwoGroupDesigns)
                test_design = two_group.tests(good)
            seq.n_chains[0] += int(c.bs.active.sum())
            seq.open_mask = [np.ones(len(test_pair), dtype=bool)] + [None] * (len(schedule) - 1)
            stt = st.last_records2d = _ht.continue_chunk_2d_designs(
                c, plan.ng, test_pair, test_design, (two_group if designs is None else designs).tables(), stt, schedule, min_extreme,
                resampling, seq.n_open, seq.n_chains, seq.open_mask)
            with np.errstate(invalid="ignore"):
                nboot = np.where(np.isnan(stt[:, 0]) | np.isnan(stt[:, 2]), 0, stt[:, 2]).astype(np.int64)
            for key, src in (('corr_coef', stt[:, 0]), ('corr_se', stt[:, 1]), ('corr_asl', _ht.sequential_pvalues(stt, resampling)),
                             ('corr_nboot', nboot)):
                _ht.scatter_pairs(c, plan, out[key], src)
            return
        st.last_records2d = stt                # (diagnostics / tests: the test records of the last pair chunk, device pair order)
        pvals = _asl.asl_from_stats(stt, approx, rows, num_cpus, resampling)
        for key, src in (('corr_coef', stt[:, 0]), ('corr_se', stt[:, 1]), ('corr_asl', pvals)):
            _ht.scatter_pairs(c, plan, out[key], src)
        if probs is not None:
            _ht.scatter_pairs(c, plan, corr_ci, _ht.sliced_intervals(rows, c.bs.ld, num_boot, probs, stt[:, 0]))

    for c in _ht.chunks_2d(st, plan, num_boot):
        run_chunk(c)
    out = {k: v.reshape(-1) for k, v in out.items()}
    m['2d_ht_vs_control'] = dict(out, **meta)
    if probs is not None:
        m['2d_ht_vs_control'].update(corr_ci=corr_ci.reshape(-1, 2), ci=float(ci))
    if sequential:
        m['2d_ht_vs_control'].update(max_boot=int(max_boot), min_extreme=int(min_extreme))
    n_conv = plan.n_conv
    pairs = list(m['2d_moments']['gene_pairs'])
    df = pd.DataFrame({'gene_1': np.repeat([a for a, _ in pairs], n_t), 'gene_2': np.repeat([b for _, b in pairs], n_t),
                       'group': np.tile(tested, n_conv)})
    df['corr_coef'], df['corr_se'], df['corr_pval'] = out['corr_coef'], out['corr_se'], out['corr_asl']
    if probs is not None:
        _ci_columns(df, ('corr', m['2d_ht_vs_control']['corr_ci']))
    if sequential:
        df['corr_nboot'] = out['corr_nboot']
    return df


def ht_2d_joint(adata, treatment, covariate=None, num_boot=10000, rng='replay', fill_seed=0, max_rows=None, approx=False):
    """Joint bootstrap test of several treatment columns on COEXPRESSION: does the correlation of a gene pair differ AT ALL
    across the levels of a factor (cell types, doses, time points, donors), after the covariates?  One test per pair of
    ``compute_2d_moments`` instead of one p-value per dummy column, and the answer does not depend on how the factor is coded.

    ``treatment`` / ``covariate`` exactly as in ``ht_1d_joint``: an array or DataFrame [groups][columns] in the group order of
    ``uns['memento']['groups']``, the name of a label column of ``create_groups`` (its dummies, first level dropped), a list of
    such names, or None; the intercept is always there.

    The statistic is the one of ``ht_1d_joint`` with y the RAW replicate correlations of the pair (no log, no Fisher
    transform: the quantity ``ht_2d_moments`` regresses): on the pair's good groups L = ``design.joint_rows`` with the cell
    counts ``ht_2d_moments`` gives its designs, Q_0 = ||L y_0||^2, the null Q*_c = ||L y_c - L y_0||^2 over the valid replicate
    columns c >= 1 (mm_joint1_stats) and p from ``joint_pvalues``: (1 + #{Q*_c > Q_0}) / (1 + n_valid), or the Satterthwaite
    fit with ``approx=True``.  For one treatment column Q_0 is ss * corr_coef^2 of the marginal test of ``ht_2d_moments``.

    Pairs and the random stream are those of ``ht_2d_moments`` / ``ht_2d_vs_control``: unordered duplicates share the first
    one's result, a self pair stays NaN with df 0, a (pair, group) with a NaN or +-1 correlation is skipped and the pair tested
    on its remaining good groups with the rank that design has; three hash uniforms per live (pair, group) are taken from the
    global ``np.random`` stream, pair-major, up front; ``rng='fast'`` streams are keyed by the pair's position among the
    distinct tested pairs.  The same ``np.random`` seed and ``max_rows`` give the replicate rows of ``ht_2d_moments``, and
    chunking changes no number under either generator.

    Returns a DataFrame (gene_1, gene_2, df, corr_stat, corr_pval), one row per requested pair in the order of
    ``compute_2d_moments``, df = r; a pair without a design (no good group, or no treatment left after the covariates on its
    good groups) has df 0 and NaN otherwise.  The arrays go to ``uns['memento']['2d_ht_joint']``: ``corr_stat``, ``corr_asl``,
    ``df``, ``n_valid`` and the ``treatment`` / ``covariate`` column names."""
    _ht.check_args(rng, resampling='bootstrap')
    m = adata.uns['memento']
    st = m['_hip']
    st.last_bootstrap2d = None                 # (free the previous call's replicate rows before this call allocates its own)
    trt, trt_names = _joint_block(m, treatment, 'treatment')
    cov, cov_names = _joint_block(m, covariate, 'covariate')
    Nc_list = np.array([m['group_cells'][g].shape[0] for g in m['groups']], dtype=np.float64)
    plan = _ht.pair_plan(m, st, num_boot, max_rows)
    uniforms = _ht.hash_uniforms(~plan.skip.reshape(-1), 3)
    out = {'corr_stat': np.full(plan.n_conv, np.nan), 'corr_asl': np.full(plan.n_conv, np.nan),
           'df': np.zeros(plan.n_conv, dtype=np.int64), 'n_valid': np.zeros(plan.n_conv, dtype=np.int64)}

    def run_chunk(c):
        good = _ht.run_chunk_2d(c, plan, uniforms, rng, fill_seed)                 # device order
        tables = _ht.joint_tables(good, cov, trt, Nc_list)
        st.last_joint_tables = tables          # (diagnostics / tests: the designs of the last pair chunk)
        stt = c.bs.joint(np.arange(c.n_ch), tables)
        for key, src in (('corr_stat', stt[:, 0]), ('corr_asl', joint_pvalues(stt, approx)),
                         ('df', tables.design_rank[tables.test_design].astype(np.int64)), ('n_valid', stt[:, 2].astype(np.int64))):
            _ht.scatter_pairs(c, plan, out[key], src)

    for c in _ht.chunks_2d(st, plan, num_boot):
        run_chunk(c)
    m['2d_ht_joint'] = dict(out, treatment=trt_names, covariate=cov_names)
    pairs = list(m['2d_moments']['gene_pairs'])
    return pd.DataFrame({'gene_1': [a for a, _ in pairs], 'gene_2': [b for _, b in pairs], 'df': out['df'],
                         'corr_stat': out['corr_stat'], 'corr_pval': out['corr_asl']})


def ht_2d_posthoc(adata, treatment_col=None, control=None, num_boot=10000, num_cpus=1, rng='replay', fill_seed=0, max_rows=None,
                  approx=False, *, ci=None):
    """WHICH levels of a factor differ in COEXPRESSION: the pairwise contrasts between the levels for every gene pair of
    ``compute_2d_moments``, each with its own test and with a p-value adjusted for the pair's whole family of contrasts
    (``ht_2d_joint`` answers whether the pair's correlation differs at all).

    Every argument means what it means in ``ht_1d_posthoc``.  Levels, strata, ``control`` and ``treatment_col`` are those of
    ``ht_2d_vs_control``: ``treatment_col=None`` makes every group a level and a contrast the plain two-group difference of the
    correlations; ``treatment_col='x'`` makes the values of that label column the levels and every other label column a
    covariate, and the test of level a against level b is EXACTLY the test ``ht_2d_vs_control(control=b, treatment_col='x')`` makes
    of a -- with the same ``np.random`` seed, ``fill_seed`` and ``max_rows`` the same ``corr_coef``, ``corr_se`` and ``corr_pval``,
    NaNs included.  ``control=None``: all unordered pairs of levels, levels in first-appearance order, (level_a, level_b) with a
    after b, rows ordered by b, then a.  ``control=value``: every other level against that one.

    Every (pair, group) chain is bootstrapped once (instead of once per control level in a loop of ``ht_2d_vs_control`` calls),
    so replicate column c of all contrasts of a gene pair is one joint draw of its family, and the adjustment is the single-step
    max-T of ``ht_1d_posthoc`` on the one plane of replicate correlations (mm_family_maxt1): a member is INCLUDED when it has a test;
    M[c] = max_j |coef_j[c] - coef_j[0]| / se_j over the included members on the columns valid for all of them;
    p_adj_j = (1 + #{c : M[c] > |coef_j[0]| / se_j}) / (1 + n_valid), reported as ``corr_pval_adj`` = max(p_adj_j, the member's own
    p-value); NaN for a member without a test, which does not enter the maximum.  ``n_family`` is the number of included members.
    ``ci=level`` adds the simultaneous intervals coef_j[0] -+ np.nanquantile(M[1:], level) * se_j: ``corr_sci_lo, corr_sci_hi``.

    Pairs and the random stream are those of ``ht_2d_moments`` / ``ht_2d_vs_control`` / ``ht_2d_joint``: unordered duplicates
    share the first one's result, a self pair stays NaN with ``n_family`` 0, a (pair, group) with a NaN or +-1 correlation is
    skipped and the pair keeps the family of its other groups or levels; three hash uniforms per live (pair, group) come from the
    global ``np.random`` stream, pair-major, up front.  A family is the contrasts of one pair and never spans chunks; chunking and
    ``max_rows`` (which also counts the one maximum row a pair adds) change no number under either generator.

    Not offered: ``resampling`` other than the centred bootstrap, ``resample_rep``, ``strict`` and ``treatment_for_gene``; a run
    over several ranks raises NotImplementedError.

    Returns a DataFrame (gene_1, gene_2, level_a, level_b, corr_coef, corr_se, corr_pval, corr_pval_adj, n_family), pair-major:
    one block of rows per requested pair in the order of ``compute_2d_moments``, and stores the arrays in
    ``uns['memento']['2d_ht_posthoc']``."""
    _ht.check_args(rng, resampling='bootstrap')
    _ht.ci_probs(ci)
    m = adata.uns['memento']
    st = m['_hip']
    comm = getattr(st, 'comm', None)
    if comm is not None and comm.world > 1:
        raise NotImplementedError("ht_2d_posthoc on a run over several ranks: the results are not gathered across ranks")
    designs, level_names = _posthoc_plan(m, treatment_col, control)
    n_mem = len(designs.pairs)
    if n_mem == 0:
        raise ValueError("ht_2d_posthoc needs at least two levels")
    st.last_bootstrap2d = st.last_posthoc2d = None    # (free the previous call's replicate rows before this call allocates its own)
    plan = _ht.pair_plan(m, st, num_boot, max_rows, extra_rows=1)
    uniforms = _ht.hash_uniforms(~plan.skip.reshape(-1), 3)
    out = {k: np.full((plan.n_conv, n_mem), np.nan) for k in ('corr_coef', 'corr_se', 'corr_asl', 'corr_asl_adj')}
    out['n_family'] = np.zeros((plan.n_conv, n_mem), dtype=np.int64)
    if ci is not None:
        out['corr_sci'] = np.full((plan.n_conv, n_mem * 2), np.nan)

    def run_chunk(c):
        bs, n_ch = c.bs, c.n_ch
        good = _ht.run_chunk_2d(c, plan, uniforms, rng, fill_seed)                 # device order
        test_pair = np.repeat(np.arange(n_ch), n_mem)
        family_ptr = np.arange(n_ch + 1, dtype=np.int64) * n_mem
        tables = (test_pair, designs.tests(good), *designs.tables())
        stt, rows = bs.contrast_design(*tables)
        scale = engine.family_scale(stt)
        maxrow, adj, fam = bs.family_maxt(family_ptr, *tables, scale)
        st.last_posthoc2d = SimpleNamespace(family_ptr=family_ptr, tables=tables, scale=scale, adj=adj, fam=fam)   # (diagnostics / tests: the last pair chunk)
        crit = None
        if ci is not None:
            q, _ = engine.row_quantiles(maxrow.reshape(-1, bs.ld), bs.ld, num_boot, [float(ci)])
            crit = engine.host(q).reshape(n_ch)
        p = _asl.asl_from_stats(stt, approx, rows, num_cpus, 'bootstrap')
        p_adj, n_family, half = _ht.adjusted_columns(p, adj[:, 0], fam[:, 0], n_mem, stt[:, 1], crit)
        for key, src in (('corr_coef', stt[:, 0]), ('corr_se', stt[:, 1]), ('corr_asl', p), ('corr_asl_adj', p_adj), ('n_family', n_family)):
            _ht.scatter_pairs(c, plan, out[key], src)
        if ci is not None:
            _ht.scatter_pairs(c, plan, out['corr_sci'], np.column_stack([stt[:, 0] - half, stt[:, 0] + half]))

    for c in _ht.chunks_2d(st, plan, num_boot):
        run_chunk(c)
    out = {k: v.reshape(-1, 2) if k == 'corr_sci' else v.reshape(-1) for k, v in out.items()}
    level_a = [level_names[a] for a, _ in designs.pairs]
    level_b = [level_names[b] for _, b in designs.pairs]
    m['2d_ht_posthoc'] = dict(out, levels=list(level_names), level_a=level_a, level_b=level_b, treatment_col=treatment_col,
                              control=None if control is None else level_b[0])
    n_conv = plan.n_conv
    pairs = list(m['2d_moments']['gene_pairs'])
    df = pd.DataFrame({'gene_1': np.repeat([a for a, _ in pairs], n_mem), 'gene_2': np.repeat([b for _, b in pairs], n_mem),
                       'level_a': np.tile(np.asarray(level_a, dtype=object), n_conv),
                       'level_b': np.tile(np.asarray(level_b, dtype=object), n_conv)})
    df['corr_coef'], df['corr_se'], df['corr_pval'], df['corr_pval_adj'] = out['corr_coef'], out['corr_se'], out['corr_asl'], out['corr_asl_adj']
    df['n_family'] = out['n_family']
    if ci is not None:
        m['2d_ht_posthoc']['ci'] = float(ci)
        df['corr_sci_lo'], df['corr_sci_hi'] = out['corr_sci'][:, 0], out['corr_sci'][:, 1]
    return df


# ----------------------------------------------------------------------------------------------
# getters
# ----------------------------------------------------------------------------------------------


def _ci_columns(df, *named):
    """Append ``<name>_ci_lo`` / ``<name>_ci_hi`` to a result table for every (name, interval array [test][2])."""
    for name, ci in named:
        ci = np.asarray(ci).reshape(-1, 2)
        df[name + '_ci_lo'], df[name + '_ci_hi'] = ci[:, 0], ci[:, 1]


def get_1d_moments(adata, groupby=None):
    """log-mean / log-residual-variance tables per group (reference: memento/main.py:523-582, groupby=None form)."""
    m = adata.uns['memento']
    names = _var_names(adata).tolist()
    mean_df = pd.DataFrame({'gene': names})
    var_df = pd.DataFrame({'gene': names})
    cell_counts = {k: v.shape[0] for k, v in m['group_cells'].items()}
    with np.errstate(invalid="ignore", divide="ignore"):
        for group, val in m['1d_moments'].items():
            mean_df[group] = np.log(val[0])
            var_df[group] = np.log(val[2])
    if groupby is None:
        return mean_df, var_df, cell_counts
    # cell-count weighted averages of the log moments over the groups whose label contains the key
    # (reference: memento/main.py:544-582)
    keys = adata.obs[groupby].astype(str).drop_duplicates().values if groupby != 'ALL' else ['sg']
    gm, gv = pd.DataFrame({'gene': names}), pd.DataFrame({'gene': names})
    for key in keys:
        sm = sv = cm = cv = 0
        for group, val in m['1d_moments'].items():
            if group == 'all' or key not in group:
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                lm, lv = np.log(val[0]), np.log(val[2])
            lm[np.isnan(lm)] = 0
            lv[np.isnan(lv)] = 0
            sm = sm + lm * cell_counts[group]
            cm = cm + (val[0] > 0) * cell_counts[group]
            sv = sv + lv * cell_counts[group]
            cv = cv + (val[2] > 0) * cell_counts[group]
        with np.errstate(invalid="ignore", divide="ignore"):
            gm[groupby + '_' + key] = sm / cm
            gv[groupby + '_' + key] = sv / cv
    return gm.copy(), gv.copy()


def get_1d_ht_result(adata):
    """DataFrame of DE / DV coefficients, standard errors and p-values (reference: memento/main.py:635-655)."""
    ht = adata.uns['memento']['1d_ht']
    names = ht['gene_names'] if 'gene_names' in ht else _var_names(adata)       # 'gene_names': gathered multi-GPU result
    if 'treatment_for_gene' in ht:
        pairs = [(g, t) for g in names for t in ht['treatment_for_gene'][g]]
    else:
        pairs = list(itertools.product(names, ht['treatment'].columns))
    df = pd.DataFrame(pairs, columns=['gene', 'tx'])
    df['de_coef'], df['de_se'], df['de_pval'] = ht['mean_coef'], ht['mean_se'], ht['mean_asl']
    df['dv_coef'], df['dv_se'], df['dv_pval'] = ht['var_coef'], ht['var_se'], ht['var_asl']
    if 'mean_ci' in ht and 'var_ci' in ht:      # ht_1d_moments(ci=...)
        _ci_columns(df, ('de', ht['mean_ci']), ('dv', ht['var_ci']))
    return df


def prepare_to_save(adata, keep=False):
    """Drop objects that cannot be written to disk (reference: memento/main.py:673-683) -- here also the
    device handles."""
    m = adata.uns['memento']
    m.pop('_hip', None)
    for group in m['groups'] + ['all']:
        m['mv_regressor'].pop(group, None)
    m['group_cells'] = {g: v.shape for g, v in m['group_cells'].items()}


def get_2d_moments(adata, groupby=None):
    """Correlation table per group (reference: memento/main.py:585-632, groupby=None form)."""
    m = adata.uns['memento']
    df = pd.DataFrame(m['2d_moments']['gene_pairs'], columns=['gene_1', 'gene_2'])
    cell_counts = {k: v.shape[0] for k, v in m['group_cells'].items()}
    for group, val in m['2d_moments'].items():
        if 'sg^' not in group:
            continue
        df[group] = val['corr']
    if groupby is None:
        return df, cell_counts
    keys = adata.obs[groupby].astype(str).drop_duplicates().values if groupby != 'ALL' else ['sg']
    out = pd.DataFrame({'gene_1': df['gene_1'], 'gene_2': df['gene_2']})       # reference: memento/main.py:604-632
    for key in keys:
        sc = cc = 0
        for group, val in m['2d_moments'].items():
            if 'sg^' not in group or key not in group:
                continue
            c = val['corr'].copy()
            valid = ~np.isnan(c)
            c[~valid] = 0
            sc = sc + c * cell_counts[group]
            cc = cc + valid * cell_counts[group]
        with np.errstate(invalid="ignore", divide="ignore"):
            out[groupby + '_' + key] = sc / cc
    return out.copy()


def get_2d_ht_result(adata):
    """DataFrame of correlation coefficients, standard errors and p-values (reference: memento/main.py:658-670)."""
    m = adata.uns['memento']
    df = pd.DataFrame(m['2d_moments']['gene_pairs'], columns=['gene_1', 'gene_2'])
    df['corr_coef'], df['corr_se'], df['corr_pval'] = m['2d_ht']['corr_coef'], m['2d_ht']['corr_se'], m['2d_ht']['corr_asl']
    if 'corr_ci' in m['2d_ht']:                 # ht_2d_moments(ci=...)
        _ci_columns(df, ('corr', m['2d_ht']['corr_ci']))
    if 'corr_nboot' in m['2d_ht']:              # ht_2d_moments(max_boot=...)
        df['corr_nboot'] = m['2d_ht']['corr_nboot']
    return df
