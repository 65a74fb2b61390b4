"""What the four hypothesis-test drivers of ``main.py`` share: argument checks, the moments view of a 1D call, the chunk loops
(one per dimension), the hash-uniform draw, the pair plan and the per-mask design tables.

The chunk loops are generators that yield the opened chunk.  Both follow one rule, release-before-allocate: the previous
chunk's ``Bootstrap1D`` / ``Bootstrap2D`` (tables, replicate rows, row closures) is dropped BEFORE the next one is constructed, so
that the caching allocator hands the same buffers back and a call never holds two chunks' rows.  They can only drop their own
references: a driver does a chunk's work in a function of its own, whose locals die when it returns.
"""

from types import SimpleNamespace

import numpy as np

from .. import engine
from . import design as _design


def check_args(rng, strict=False, **kwargs):
    """The ``rng`` / ``strict`` checks of all four drivers and the reference's keyword arguments of the two ``*_moments`` drivers:
    -> (resampling, resample_rep, approx).  The ``rng`` check comes first: it runs before ``adata`` is touched."""
    if rng not in ('replay', 'fast'):
        raise ValueError("rng must be 'replay' or 'fast'")
    if strict and rng != 'replay':
        raise ValueError("strict=True needs rng='replay'")
    if 'resampling' not in kwargs:
        raise TypeError("_compute_asl() missing 1 required positional argument: 'resampling'")
    # 'bootstrap' centres the null on the observed value, anything else does not (hypothesis_test.py:66-70)
    return kwargs['resampling'], bool(kwargs.get('resample_rep', False)), bool(kwargs.get('approx', False))


def ci_probs(ci):
    """The ``ci`` keyword of the four drivers: None -> None (no interval); a level 0 < ci < 1 -> the two probabilities
    ((1 - ci) / 2, (1 + ci) / 2) of the percentile interval; anything else raises ValueError.  Pure: runs before any device work."""
    if ci is None:
        return None
    if isinstance(ci, (bool, np.bool_)) or not isinstance(ci, (int, float, np.integer, np.floating)) or not 0 < float(ci) < 1:
        raise ValueError(f"ci must be None or a confidence level strictly between 0 and 1, not {ci!r}")
    ci = float(ci)
    return (1 - ci) / 2, (1 + ci) / 2


# scratch for the coefficient rows of ``sliced_intervals``: not tuned, it only has to be small next to the replicate planes
CI_SCRATCH_BYTES = 1 << 30


def row_intervals(coef_rows, ld, num_boot, probs, coef0):
    """Percentile intervals [test][2] (host) of coefficient rows that are resident (``coef_rows``: device [test][ld]): the
    ``probs`` quantiles of the replicate columns 1..num_boot, dropped (NaN) columns excluded -- the columns the standard error
    is taken over.  A test without a coefficient (``coef0`` NaN) has a NaN interval."""
    q, _ = engine.row_quantiles(coef_rows, ld, num_boot, probs)
    ci = engine.host(q).copy()
    ci[np.isnan(coef0)] = np.nan
    return ci


def sliced_intervals(rows, ld, num_boot, probs, coef0, scratch_bytes=None):
    """``row_intervals`` for tests whose coefficient rows are not stored: ``rows(idx, to_host=False, out=scratch)`` produces
    them (``contrast`` / ``contrast_design`` of Bootstrap1D / Bootstrap2D), a slice of tests at a time, into ONE scratch tensor of
    at most ``scratch_bytes`` (default ``CI_SCRATCH_BYTES``; never less than one row).  Every test's interval comes from its own
    row alone, so the slicing changes no number.  Tests without a coefficient are not produced at all."""
    if scratch_bytes is None:
        scratch_bytes = CI_SCRATCH_BYTES
    coef0 = np.asarray(coef0)
    ci = np.full((len(coef0), 2), np.nan)
    live = np.flatnonzero(~np.isnan(coef0))
    if not len(live):
        return ci
    per = int(min(len(live), max(1, int(scratch_bytes) // (8 * ld))))
    scratch = engine.empty((per, ld), engine._torch().float64)
    for lo in range(0, len(live), per):
        idx = live[lo:lo + per]
        q, _ = engine.row_quantiles(rows(idx, to_host=False, out=scratch), ld, num_boot, probs)
        ci[idx] = engine.host(q)
    return ci


def moments_view(m):
    """What a 1D test reads from ``uns['memento']``: the groups, their q and cell counts, the true moments [group][gene] and the
    mean-variance fit."""
    groups = m['groups']
    return SimpleNamespace(
        groups=groups, ng=len(groups), mean_only=m['estimator_type'] == 'mean_only',
        Nc_list=np.array([m['group_cells'][g].shape[0] for g in groups], dtype=np.float64),
        gq=np.array([m['group_q'][g] for g in groups]),
        true_mean=np.stack([m['1d_moments'][g][0] for g in groups]),
        true_rv=np.stack([m['1d_moments'][g][2] for g in groups]),
        fit=m['mv_regressor'][groups[0]])


def pair_skip(true_mean, true_rv):
    """hypothesis_test.py:167-171, vectorised over [n_groups][G] -> [pair] (gene-major)."""
    with np.errstate(invalid="ignore"):
        skip = np.isnan(true_mean) | np.isnan(true_rv) | (true_mean == 0) | (true_rv < 0)
    return skip.T.reshape(-1)


def hash_uniforms(live, k):
    """The ``k`` hash uniforms of every live chain from the global ``np.random`` stream, in chain order: -> [k][chain], dead
    chains keep 0.  The reference draws per chain -- ``random(1)`` then ``random()`` in 1D (bootstrap.py:62, :65), ``random(2)``
    then ``random()`` per (pair, group) in 2D -- and ONE ``random(k * n)`` call takes the same stream positions."""
    idx = np.flatnonzero(live)
    out = np.zeros((k, len(live)))
    u = np.random.random(k * len(idx))
    for j in range(k):
        out[j, idx] = u[j::k]
    return out


# ----------------------------------------------------------------------------------------------
# 1D: gene chunks
# ----------------------------------------------------------------------------------------------


def chunks_1d(st, mv, num_boot, chunk):
    """Open the genes in chunks of ``chunk``: yields ``c`` with ``g0``, ``g1``, ``G``, ``bs`` (K5 done, outputs allocated) and
    ``skip`` [pair]; no gene kept, no chunk.  ``c`` is ONE object, emptied before the next chunk is opened
    (release-before-allocate).  ``st.last_bootstrap`` / ``st.last_chunk`` hold the last chunk afterwards
    (diagnostics / tests / bench: the last gene chunk's replicate rows)."""
    G_all = len(st.gene_idx)
    c = SimpleNamespace(bs=None, g0=0, g1=0)
    for g0 in range(0, G_all, max(1, chunk)):
        c.__dict__.clear()      # release the previous chunk's replicate rows first: the caching allocator hands them back
        c.g0, c.g1 = g0, min(G_all, g0 + max(1, chunk))
        c.G = c.g1 - g0
        true_mean, true_rv = mv.true_mean[:, g0:c.g1], mv.true_rv[:, g0:c.g1]
        c.bs = engine.Bootstrap1D(st.blocks, st.gene_idx[g0:c.g1], st.maxx, st.sf_bin, st.sf_table, mv.gq, num_boot)   # K5
        c.skip = pair_skip(true_mean, true_rv)
        with np.errstate(invalid="ignore", divide="ignore"):
            tm_log = np.where(c.skip, np.nan, np.log(true_mean.T.reshape(-1)))
            tv_log = np.where(c.skip, np.nan, np.log(true_rv.T.reshape(-1)))
        c.bs.alloc_outputs(tm_log, tv_log)
        yield c
    st.last_bootstrap, st.last_chunk = c.bs, (c.g0, c.g1)


def run_chunk_1d(c, mv, rng, fill_seed, fill_keys, chain_keys, uniforms=None):
    """Bootstrap the chunk's chains (K6-K8, invalid replicates re-filled on the device): the two hash ``uniforms`` [2][pair] come
    from the global ``np.random`` stream unless they are passed in; ``fill_keys`` / ``chain_keys`` [pair] key the refill and the
    rng='fast' streams.  -> (``good`` [gene][group], hypothesis_test.py:193-200; ``n_inv`` [pair][2], the refilled replicates)."""
    r1, r0 = hash_uniforms(~c.skip, 2) if uniforms is None else uniforms
    n_inv = c.bs.run(c.skip, r1, r0, mv.fit, fill_mode=0, fill_seed=fill_seed, fast=(rng == 'fast'), mean_only=mv.mean_only,
                     fill_keys=fill_keys, chain_keys=chain_keys)
    good = (~c.skip) & (c.bs.K >= 2) & ~(n_inv < 0).any(axis=1)      # bootstrap.py:97-98: a single bin gives NaN replicates
    return good.reshape(c.G, mv.ng), n_inv


# ----------------------------------------------------------------------------------------------
# 1D: sequential bootstrap (ht_1d_vs_control(max_boot=...)): records, schedule, stopping rule, rounds
# ----------------------------------------------------------------------------------------------

_M64 = (1 << 64) - 1


def _mix64(x):
    """The splitmix64 output function of csrc/boot.hip (mix64) on a Python int."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def check_sequential(max_boot, min_extreme, num_boot, rng, approx, ci):
    """The ``max_boot`` / ``min_extreme`` keywords of ``ht_1d_vs_control``, ``ht_2d_moments`` and ``ht_2d_vs_control_sequential``; pure, runs before
    ``adata`` is touched.  -> whether the call is sequential (``max_boot`` given)."""
    if max_boot is None:
        return False

    def is_int(x):
        return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))

    if rng != 'fast':
        raise ValueError("max_boot needs rng='fast': only its replicates own a stream each, so that a later round continues a chain")
    if approx:
        raise ValueError("max_boot needs approx=False: the sequential bootstrap reports empirical p-values")
    if ci is not None:
        raise ValueError("max_boot needs ci=None: no round holds all replicates of a test")
    if not is_int(num_boot) or not is_int(max_boot) or max_boot < num_boot:
        raise ValueError(f"max_boot must be an integer >= num_boot ({num_boot!r}), not {max_boot!r}")
    if max_boot > 2 ** 31 - 1:
        raise ValueError("max_boot must be at most 2^31 - 1")
    if not is_int(min_extreme) or min_extreme < 0:
        raise ValueError(f"min_extreme must be an integer >= 0, not {min_extreme!r}")
    return True


def sequential_schedule(num_boot, max_boot):
    """Cumulative replicate totals of the rounds: n_0 = num_boot, n_j = min(2 n_(j-1), max_boot); round j >= 1 covers the global
    replicates [n_(j-1), n_j).  A function of these two numbers alone -- never of memory or chunking."""
    num_boot, max_boot = int(num_boot), int(max_boot)
    if num_boot < 1 or max_boot < num_boot:
        raise ValueError("sequential_schedule: need 1 <= num_boot <= max_boot")
    totals = [num_boot]
    while totals[-1] < max_boot:
        totals.append(min(2 * totals[-1], max_boot))
    return totals


def round_fill_seed(fill_seed, j):
    """Refill seed of round j: ``fill_seed`` itself for round 0 (today's call), a splitmix of (fill_seed, j) for j >= 1."""
    return int(fill_seed) & _M64 if j == 0 else _mix64((int(fill_seed) & _M64) ^ _mix64(int(j)))


def merge_records(rounds):
    """The test records [n_tests][8] of several rounds of one chain of replicates, folded into the record of all of them (THE
    TEST RECORD of csrc/contract.hip): coef0 from round 0; n_valid, n_extreme, n_raw_extreme summed -- the null is centred on the
    observed coefficient, not on the replicates' mean, so the counts add; with n_j = n_valid and mean_j = mean - coef0 of round j,
    N = sum n_j, mean = sum n_j mean_j / N and se = sqrt(sum n_j (se_j^2 + (mean_j - mean)^2) / N); all_equal only if every round
    with replicates says so; range is NaN (not mergeable, not read after round 0).  A round with n_j = 0 contributes nothing."""
    rounds = [np.asarray(r, dtype=np.float64).reshape(-1, 8) for r in rounds]
    first = rounds[0]
    if len(rounds) == 1:
        return first.copy()
    out = first.copy()
    n = np.stack([r[:, 2] for r in rounds])                    # [round][test]
    has = n > 0
    N = n.sum(axis=0)
    for k in (3, 6):
        out[:, k] = np.stack([r[:, k] for r in rounds]).sum(axis=0)
    out[:, 2] = N
    mean_j = np.where(has, np.stack([r[:, 4] for r in rounds]), 0.0)
    se_j = np.where(has, np.stack([r[:, 1] for r in rounds]), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (n * mean_j).sum(axis=0) / N
        se = np.sqrt((n * (se_j ** 2 + (mean_j - mean) ** 2)).sum(axis=0) / N)
    out[:, 4] = np.where(N > 0, mean, np.nan)
    out[:, 1] = np.where(N > 0, se, np.nan)
    alleq = np.stack([r[:, 5] for r in rounds]) != 0
    out[:, 5] = np.where(N > 0, (alleq | ~has).all(axis=0), first[:, 5] != 0).astype(np.float64)
    out[:, 7] = np.nan
    return out


def open_tests(merged, min_extreme=10, resampling='bootstrap'):
    """Which tests [n_tests] go on to the next round: the record is testable (coef0 finite, n_valid > 0, not all_equal) and its
    extreme count -- [3] for 'bootstrap', the un-centred [6] otherwise -- is still <= ``min_extreme``.  The default 10 is the
    reference's own threshold for trusting the empirical p-value (hypothesis_test.py:90)."""
    st = np.asarray(merged, dtype=np.float64).reshape(-1, 8)
    c = st[:, 3] if resampling == 'bootstrap' else st[:, 6]
    return np.isfinite(st[:, 0]) & (st[:, 2] > 0) & (st[:, 5] == 0) & (c <= min_extreme)


def sequential_pvalues(merged, resampling='bootstrap'):
    """(c + 1) / (n + 1) of every testable record, c and n the merged extreme and valid counts; NaN elsewhere.  No tail fit."""
    st = np.asarray(merged, dtype=np.float64).reshape(-1, 8)
    c = st[:, 3] if resampling == 'bootstrap' else st[:, 6]
    live = np.isfinite(st[:, 0]) & (st[:, 2] > 0) & (st[:, 5] == 0)
    return np.where(live, (c + 1) / (st[:, 2] + 1), np.nan)


def _design_chains(test_gene, test_design, design_ptr, design_grp, ng):
    """The distinct chains (gene slot * ng + group) that the designs of the given tests read."""
    lo, cnt = design_ptr[test_design].astype(np.int64), np.diff(design_ptr)[test_design].astype(np.int64)
    first = np.cumsum(cnt) - cnt
    pos = np.repeat(lo - first, cnt) + np.arange(int(cnt.sum()))
    return np.unique(np.repeat(np.asarray(test_gene, dtype=np.int64), cnt) * ng + design_grp[pos])


def continue_chunk_1d(c, mv, test_gene, test_design, tables, stats, schedule, min_extreme, resampling, fill_seed, keys, n_open):
    """Rounds 1.. of the sequential bootstrap on an open chunk whose round 0 (``run_chunk_1d`` with rng='fast', then the
    contraction) gave the records ``stats`` = (st_m, st_v) of the tests (``test_gene`` [test] gene slot, ``test_design`` [test]
    into ``tables`` = (design_ptr, design_grp, design_w)).  A test is continued while it is open on either plane
    (``open_tests``).  Round j bootstraps the global replicates [schedule[j - 1], schedule[j]) of the chains that an open test's
    design reads -- every other slot of the chunk's tile layout is skipped -- into gene-granular planes
    [open genes x groups][1 + rep_n] (column 0 copied from the chunk, the other chains' rows NaN), refills invalid replicates from
    the round's own valid ones under ``round_fill_seed`` and the chains' keys ``keys`` [pair], contracts the open tests only and
    folds their records (``merge_records``).  The round's planes are allocated once per round, released before the next, and
    never hold more bytes than the chunk's: a round with more rows takes its open genes in sub-batches (genes are independent).
    ``n_open`` [round]: the tests open after round j are added to entry j.  -> the merged (st_m, st_v)."""
    bs, ng, torch = c.bs, mv.ng, engine._torch()
    design_ptr, design_grp, design_w = (np.asarray(a) for a in tables)
    test_gene, test_design = np.asarray(test_gene, dtype=np.int64), np.asarray(test_design, dtype=np.int64)
    merged = [np.array(s, dtype=np.float64) for s in stats]
    grp = np.arange(ng)
    for j in range(1, len(schedule)):
        is_open = open_tests(merged[0], min_extreme, resampling) | open_tests(merged[1], min_extreme, resampling)
        n_open[j - 1] += int(is_open.sum())
        if not is_open.any():
            break
        idx = np.flatnonzero(is_open)
        rep_lo, rep_n = schedule[j - 1], schedule[j] - schedule[j - 1]
        genes = np.unique(test_gene[idx])
        per = int(min(len(genes), max(1, (bs.n_pairs * bs.ld) // (ng * (1 + rep_n)))))
        pm = engine.empty((per * ng, 1 + rep_n), torch.float64)
        pv = engine.empty((per * ng, 1 + rep_n), torch.float64)
        new = [np.empty((len(idx), 8)) for _ in merged]
        for lo in range(0, len(genes), per):
            gsub = genes[lo:lo + per]
            n_rows = len(gsub) * ng
            planes = [pm[:n_rows], pv[:n_rows]]
            in_sub = np.isin(test_gene[idx], gsub)
            t_gene, t_design = test_gene[idx[in_sub]], test_design[idx[in_sub]]
            chains = _design_chains(t_gene, t_design, design_ptr, design_grp, ng)
            rows_old = (gsub[:, None] * ng + grp).reshape(-1)
            d_rows = engine.dev(rows_old)
            for p, y in zip(planes, (bs.ym, bs.yv)):
                p.fill_(float("nan"))
                p[:, 0] = y[d_rows, 0]
            bs.run_range(rep_lo, rep_n, chains, planes, np.searchsorted(gsub, chains // ng) * ng + chains % ng, mv.fit,
                         round_fill_seed(fill_seed, j), keys[rows_old], mean_only=mv.mean_only)
            recs, _ = engine._contrast_design(planes, 1 + rep_n, rep_n, ng, len(gsub), np.searchsorted(gsub, t_gene), t_design, design_ptr,
                                              design_grp, design_w)
            for k, r in enumerate(recs):
                new[k][in_sub] = r
        del pm, pv, planes, p      # release-before-allocate: the next round's planes take these buffers
        for k in range(len(merged)):
            merged[k][idx] = merge_records([merged[k][idx], new[k]])
    else:
        n_open[len(schedule) - 1] += int((open_tests(merged[0], min_extreme, resampling) | open_tests(merged[1], min_extreme, resampling)).sum())
    return merged


def gene_columns(treatment, treatment_for_gene, names):
    """Treatment columns of every gene, looked up once per call: a tuple of column positions, or None = all columns."""
    if treatment_for_gene is None:
        return [None] * len(names)
    trt_cols = list(treatment.columns)
    return [tuple(trt_cols.index(c) for c in treatment_for_gene[n]) for n in names]


# ----------------------------------------------------------------------------------------------
# per-mask design tables
# ----------------------------------------------------------------------------------------------


def _take(trt, cols):
    return trt if cols is None else trt[:, list(cols)]


def design_tables(good, cols, cov, trt, Nc, resampled=False, rr_cols=None, first_only=False):
    """The design of every test of a chunk: row ``k`` of ``good`` [rows][groups] (a gene or a pair) is tested once per treatment
    column ``cols[k]`` (a tuple; None = all columns), gene-major x treatment column (main.py:399-404), or -- ``first_only`` -- on
    the first of them.  Everything is built once per distinct (good mask, columns) and shared by the rows that have it.

    -> ``test_row`` [test], ``Wmat`` [test][group] (``design.weight_rows``) and, when ``resampled``: ``tt_mat`` [test][group] /
    ``Mstack`` [mask][group][group] (``design.residual_parts``), ``row_mask`` [row] (index into ``Mstack``) and ``rr_test``
    [test].  ``rr_test`` is false where the treatment of the good groups is all ones -- those tests keep the weighted-average
    branch (hypothesis_test.py:262-265, :384-386) and are not resampled -- and for a row without a good group.
    ``rr_cols``: the columns the residual parts and the all-ones verdict are taken over, when they are not ``cols``."""
    good = np.asarray(good, dtype=bool)
    n_rows, ng = good.shape
    rr_cols = cols if rr_cols is None else rr_cols
    w_cache, r_cache = {}, {}
    test_row, w_rows, tt_rows, Ms, rr = [], [], [], [], []
    row_mask = np.zeros(n_rows, dtype=np.int32)
    for k in range(n_rows):
        key = (good[k].tobytes(), cols[k])
        W = w_cache.get(key)
        if W is None:
            W = _design.weight_rows(cov, _take(trt, cols[k]), Nc, good[k])
            W = w_cache[key] = W[:1] if first_only else W
        test_row.extend([k] * len(W))
        w_rows.append(W)
        if not resampled:
            continue
        key = (good[k].tobytes(), rr_cols[k])
        if key not in r_cache:
            t = _take(trt, rr_cols[k])
            Mg, ttg = _design.residual_parts(cov, t, Nc, good[k])
            allones = (t[good[k]] == 1).mean() == 1 if good[k].any() else True
            r_cache[key] = (len(Ms), ttg[:1] if first_only else ttg, not allones)
            Ms.append(Mg)
        row_mask[k], ttg, resample = r_cache[key]
        tt_rows.append(ttg)
        rr.extend([resample] * len(ttg))
    d = SimpleNamespace(test_row=np.asarray(test_row, dtype=np.int64), tt_mat=None, Mstack=None, row_mask=None, rr_test=None,
                        Wmat=np.concatenate(w_rows, axis=0) if w_rows else np.zeros((0, ng)))
    if resampled:
        d.tt_mat = np.concatenate(tt_rows, axis=0) if tt_rows else np.zeros((0, ng))
        d.Mstack = np.stack(Ms) if Ms else np.zeros((0, ng, ng))
        d.row_mask, d.rr_test = row_mask, np.asarray(rr, dtype=bool)
    return d


def eqtl_gene_columns(genotypes, gene_snp_pairs, names):
    """The cis SNPs of every kept gene (``ht_1d_eqtl``): a tuple of positions among the columns of ``genotypes`` per name of
    ``names``, in the gene's list order; a kept gene that is not listed has none.  ``gene_snp_pairs``: a dict gene -> list of
    genotype columns (the reference's ``treatment_for_gene``), or a two-column frame (gene, snp), whose rows keep their order
    within a gene.  Genes outside ``names`` are ignored (``gene_columns``); a SNP that is not a genotype column raises ValueError."""
    pos = {c: j for j, c in enumerate(genotypes.columns)}
    if isinstance(gene_snp_pairs, dict):
        lists = {g: list(v) for g, v in gene_snp_pairs.items()}
    else:
        if getattr(gene_snp_pairs, 'shape', (0, 0))[1:] != (2,):
            raise ValueError("gene_snp_pairs must be a dict gene -> SNP columns or a two-column frame (gene, snp)")
        lists = {}
        for g, s in zip(gene_snp_pairs.iloc[:, 0], gene_snp_pairs.iloc[:, 1]):
            lists.setdefault(g, []).append(s)
    out = []
    for n in names:
        snps = lists.get(n, ())
        missing = [s for s in snps if s not in pos]
        if missing:
            raise ValueError(f"gene {n!r}: {missing[0]!r} is not a column of genotypes")
        out.append(tuple(pos[s] for s in snps))
    return out


def eqtl_tables(good, cols, cov, trt, Nc, resampled=False):
    """``design_tables`` for tests that arrive gene-major with a SNP list of its own per gene (``ht_1d_eqtl``): row ``k`` of ``good``
    is tested on the treatment columns ``cols[k]`` (a tuple, possibly empty), and ``gene_ptr`` [rows + 1] is the CSR pointer of
    its tests.  ``Wmat``, ``tt_mat`` and ``rr_test`` come from the same calls as in ``design_tables`` (``design.weight_rows`` /
    ``design.residual_parts`` on the gene's whole column list: bit-equal rows), but ``Mstack`` holds ONE residual maker per
    distinct good mask -- it depends on the mask, the covariates and ``Nc`` alone -- where ``design_tables``, whose cache key
    includes the columns, would keep one per gene."""
    good = np.asarray(good, dtype=bool)
    n_rows, ng = good.shape
    w_cache, r_cache, m_index = {}, {}, {}
    counts, w_rows, tt_rows, Ms, rr = [], [], [], [], []
    row_mask = np.zeros(n_rows, dtype=np.int32)
    for k in range(n_rows):
        mask, ck = good[k].tobytes(), tuple(cols[k])
        counts.append(len(ck))
        if resampled and mask not in m_index:
            m_index[mask] = len(Ms)
            Ms.append(_design.residual_parts(cov, np.zeros((ng, 1)), Nc, good[k])[0])      # (M does not read the treatment)
        if resampled:
            row_mask[k] = m_index[mask]
        if not ck:
            continue
        key = (mask, ck)
        if key not in w_cache:
            w_cache[key] = _design.weight_rows(cov, _take(trt, ck), Nc, good[k])
        w_rows.append(w_cache[key])
        if not resampled:
            continue
        if key not in r_cache:
            t = _take(trt, ck)
            allones = (t[good[k]] == 1).mean() == 1 if good[k].any() else True
            r_cache[key] = (_design.residual_parts(cov, t, Nc, good[k])[1], not allones)
        ttg, resample = r_cache[key]
        tt_rows.append(ttg)
        rr.extend([resample] * len(ttg))
    gene_ptr = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    d = SimpleNamespace(gene_ptr=gene_ptr, test_row=np.repeat(np.arange(n_rows, dtype=np.int64), counts), tt_mat=None, Mstack=None,
                        row_mask=None, rr_test=None, Wmat=np.concatenate(w_rows, axis=0) if w_rows else np.zeros((0, ng)))
    if resampled:
        d.tt_mat = np.concatenate(tt_rows, axis=0) if tt_rows else np.zeros((0, ng))
        d.Mstack = np.stack(Ms) if Ms else np.zeros((0, ng, ng))
        d.row_mask, d.rr_test = row_mask, np.asarray(rr, dtype=bool)
    return d


def interaction_context(interaction, ng):
    """The context vector of ``ht_1d_eqtl(interaction=...)``: one finite value per group from an array, a Series or a one-column
    frame; ValueError otherwise (more than one column, another length, a non-finite value)."""
    ctx = np.asarray(getattr(interaction, 'values', interaction), dtype=np.float64)
    if ctx.ndim == 2 and ctx.shape[1] == 1:
        ctx = ctx[:, 0]
    if ctx.ndim != 1:
        raise ValueError("interaction must be ONE value per group (an array, a Series or a one-column frame), not several columns")
    if len(ctx) != ng or not np.isfinite(ctx).all():
        raise ValueError(f"interaction must be one finite value per group ({ng})")
    return ctx


def eqtl_interaction_tables(good, cols, cov, ctx, trt, Nc):
    """``eqtl_tables`` for the genotype-by-context tests of ``ht_1d_eqtl(interaction=ctx)``: test (row ``k``, SNP ``s`` of ``cols[k]``)
    is of ``a = g_s * ctx`` after the shared covariates ``[cov | ctx]`` and the covariate of its own ``g_s``.  With M the residual
    maker of ``[1 | cov | ctx]`` on the row's good groups (``design.residual_parts``, once per distinct mask), z = M g_s and
    a~ = M a, the per-test covariate comes out by a rank-one step (Frisch-Waugh), for all SNPs of a row at once:
      ``zt_mat`` [test][group]  z, or exactly zero where its wbar-weighted sum of squares is <= ``design.SS_DEGENERATE`` (g_s inside
                                the shared span: the test proceeds on the shared covariates alone);
      ``tt_mat`` [test][group]  tt = a~ - z (z' W a~) / (z' W z), the fully residualised treatment;
      ``Wmat``   [test][group]  Nc_j tt_j / sum Nc tt^2 on the good groups -- the weight row of ``design.weight_rows`` on
                                ``[cov | ctx | g_s]``: tt is W-orthogonal to that whole design, so its hat-matrix term drops out;
      ``has_test`` [test]       false (no test: zero rows in ``tt_mat`` and ``Wmat``) where the wbar-weighted sum of squares of tt
                                is <= ``SS_DEGENERATE`` (carriers in one context only, a monomorphic SNP, a constant context), where
                                the treatment is all ones on the good groups, and for a row without a good group;
    ``gene_ptr``, ``test_row``, ``Mstack`` / ``row_mask`` as in ``eqtl_tables`` (one maker per mask)."""
    good = np.asarray(good, dtype=bool)
    n_rows, ng = good.shape
    Nc = np.asarray(Nc, dtype=np.float64)
    ctx = np.asarray(ctx, dtype=np.float64).reshape(ng)
    covx = np.column_stack([np.asarray(cov, dtype=np.float64).reshape(ng, -1), ctx])
    cache, m_index = {}, {}
    counts, parts, Ms = [], [], []
    row_mask = np.zeros(n_rows, dtype=np.int32)
    for k in range(n_rows):
        mask, ck = good[k].tobytes(), tuple(cols[k])
        counts.append(len(ck))
        if mask not in m_index:
            m_index[mask] = len(Ms)
            Ms.append(_design.residual_parts(covx, np.zeros((ng, 1)), Nc, good[k])[0])
        row_mask[k] = m_index[mask]
        if not ck:
            continue
        key = (mask, ck)
        if key not in cache:
            S, idx = len(ck), np.flatnonzero(good[k])
            g = _take(trt, ck)
            a = g * ctx[:, None]
            zt, tt, W, has = np.zeros((S, ng)), np.zeros((S, ng)), np.zeros((S, ng)), np.zeros(S, dtype=bool)
            if len(idx):
                res = _design.residual_parts(covx, np.column_stack([g, a]), Nc, good[k])[1]
                z, at = res[:S, idx], res[S:, idx]
                w = Nc[idx]
                wbar = w / w.sum()
                z = np.where(((z * z) @ wbar > _design.SS_DEGENERATE)[:, None], z, 0.0)
                zz = (z * z) @ w
                with np.errstate(divide="ignore", invalid="ignore"):
                    slope = np.where(zz > 0, ((z * at) @ w) / zz, 0.0)
                t = at - z * slope[:, None]
                has = ((t * t) @ wbar > _design.SS_DEGENERATE) & ~(a[idx] == 1).all(axis=0)
                t = np.where(has[:, None], t, 0.0)
                with np.errstate(divide="ignore", invalid="ignore"):
                    Wg = np.where(has[:, None], t * w[None, :] / ((t * t) @ w)[:, None], 0.0)
                zt[:, idx], tt[:, idx], W[:, idx] = z, t, Wg
            cache[key] = (zt, tt, W, has)
        parts.append(cache[key])
    gene_ptr = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    cat = lambda i, empty: np.concatenate([p[i] for p in parts], axis=0) if parts else empty
    return SimpleNamespace(gene_ptr=gene_ptr, test_row=np.repeat(np.arange(n_rows, dtype=np.int64), counts),
                           zt_mat=cat(0, np.zeros((0, ng))), tt_mat=cat(1, np.zeros((0, ng))), Wmat=cat(2, np.zeros((0, ng))),
                           has_test=cat(3, np.zeros(0, dtype=bool)), Mstack=np.stack(Ms) if Ms else np.zeros((0, ng, ng)), row_mask=row_mask)


def weight_row_designs(test_row, Wmat, good):
    """The weight rows of plain tests as the CSR designs of ``contrast_design``: design t lists the good groups of row block
    ``test_row[t]`` in ascending order (zero weights included: they take part in the validity of a column) with the weights
    ``Wmat[t]`` there -- the sum ``k_contract_stats`` forms, term for term.  A row block without a good group gives the empty design
    (the NaN record).  -> (test_design, design_ptr, design_grp, design_w)."""
    good = np.asarray(good, dtype=bool)
    sel = good[test_row] if len(test_row) else np.zeros((0, good.shape[1]), dtype=bool)
    t_idx, grp = np.nonzero(sel)                       # row-major: test by test, groups ascending
    design_ptr = np.concatenate([[0], np.cumsum(sel.sum(axis=1), dtype=np.int64)])
    return np.arange(len(test_row), dtype=np.int32), design_ptr, grp.astype(np.int32), np.asarray(Wmat, dtype=np.float64)[t_idx, grp]


def sliced_rows(parts, idx, ld, scratch_bytes=None):
    """Host coefficient rows [len(idx)][ld] of the tests ``idx`` whose rows are not stored, for ``asl.asl_from_stats``: ``parts`` is a
    list of (member, local, rows) -- test t belongs to the part with ``member[t]``, where it is test ``local[t]`` of the closure
    ``rows(idx, to_host=False, out=scratch)`` -- and every part produces its rows a slice at a time into ONE device scratch of
    at most ``scratch_bytes`` (default ``CI_SCRATCH_BYTES``; never less than one row), as ``sliced_intervals`` does."""
    if scratch_bytes is None:
        scratch_bytes = CI_SCRATCH_BYTES
    idx = np.asarray(idx, dtype=np.int64)
    out = np.full((len(idx), ld), np.nan)
    if not len(idx):
        return out
    per = int(min(len(idx), max(1, int(scratch_bytes) // (8 * ld))))
    scratch = engine.empty((per, ld), engine._torch().float64)
    for member, local, rows in parts:
        mine = np.flatnonzero(member[idx])
        for lo in range(0, len(mine), per):
            sl = mine[lo:lo + per]
            out[sl] = engine.host(rows(local[idx[sl]], to_host=False, out=scratch))
    return out


def pair_design_tables(good, tcol, per_gene, cov, trt, Nc, resampled=False):
    """``design_tables`` for gene pairs: one test per pair, on treatment column ``tcol[k]``.  ``per_gene`` = the call has a
    ``treatment_for_gene``.  Without one, the weight row is that of column 0 but the residual parts and the all-ones verdict are
    taken over the WHOLE treatment (and row 0 of the result kept), as the reference does: with several treatment columns a pair is
    resampled unless all of them are all ones."""
    cols = [(int(t),) for t in tcol]
    return design_tables(good, cols, cov, trt, Nc, resampled, rr_cols=cols if per_gene else [None] * len(cols), first_only=True)


def joint_tables(good, cov, trt, Nc):
    """The designs of the joint test (``design.joint_rows``) of a chunk: row ``k`` of ``good`` [rows][groups] (a gene or a pair) is
    tested once, on its good groups; one design per distinct good mask, shared by the rows that have it.

    -> ``test_design`` [row] and the CSR-like tables the kernels take (``Bootstrap1D.joint``, ``Bootstrap2D.joint``): ``design_ptr`` [design + 1] into
    ``design_grp`` (every good group of the mask, ascending), ``design_rank`` [design], ``design_lofs`` [design] (int64 offset
    into ``design_L``) and ``design_L`` (row-major rank x n_d per design: the columns of L on the good groups)."""
    good = np.asarray(good, dtype=bool)
    cache = {}
    test_design = np.zeros(good.shape[0], dtype=np.int32)
    ptr, rank, lofs, grp, Ls, n_l = [0], [], [], [], [], 0
    for k in range(good.shape[0]):
        key = good[k].tobytes()
        d = cache.get(key)
        if d is None:
            d = cache[key] = len(rank)
            idx = np.flatnonzero(good[k])
            L = _design.joint_rows(cov, trt, Nc, good[k])[:, idx]
            grp.append(idx)
            ptr.append(ptr[-1] + len(idx))
            rank.append(L.shape[0])
            lofs.append(n_l)
            Ls.append(L.reshape(-1))
            n_l += L.size
        test_design[k] = d
    return SimpleNamespace(
        test_design=test_design, design_ptr=np.asarray(ptr, dtype=np.int32), design_rank=np.asarray(rank, dtype=np.int32),
        design_lofs=np.asarray(lofs, dtype=np.int64), design_grp=np.concatenate(grp).astype(np.int32) if grp else np.zeros(0, np.int32),
        design_L=np.concatenate(Ls).astype(np.float64) if Ls else np.zeros(0))


class _TwoGroupDesigns:
    """What ``design.VsControlDesigns`` is to a label column, for whole groups (``treatment_col=None``): every group but ``ctrl`` is a
    guide, tested by the design {(guide, +1), (ctrl, -1)} where both groups are good and by the empty design otherwise."""

    def __init__(self, ng, ctrl):
        self.ng, self.ctrl = ng, ctrl
        self.guides = [j for j in range(ng) if j != ctrl]

    def tests(self, good):
        good = np.asarray(good, dtype=bool)
        g = np.asarray(self.guides, dtype=np.int64)
        return np.where(good[:, g] & good[:, [self.ctrl]], g[None, :], self.ng).astype(np.int32).reshape(-1)

    def tables(self):
        ng = self.ng
        grp = np.column_stack([np.arange(ng), np.full(ng, self.ctrl)]).reshape(-1).astype(np.int32)
        return np.concatenate([2 * np.arange(ng + 1), [2 * ng]]).astype(np.int32), grp, np.tile([1.0, -1.0], ng)


class PosthocDesigns:
    """The families of ``ht_1d_posthoc``: pairwise contrasts between the levels of a factor, as merged vs-control design tables.

    ``labels`` [group][label column] (strings), ``k_trt``: the factor's column, or None = every group is a level of its own;
    ``control``: None = all unordered pairs, else a level (``k_trt`` None: a group index) that every other level is tested against.
    ``levels`` are in first-appearance order; ``pairs`` [(a, b)] as level indices, a after b, ordered by b then a.  The test of a
    against b is the one ``VsControlDesigns(control=b)`` makes of guide a (``k_trt`` None: the two-entry design): one such object
    per control level, whose design ids are shifted by the designs of the objects before it when the tables are merged."""

    def __init__(self, labels, k_trt, control, Nc):
        labels = np.asarray(labels, dtype=object).astype(str)
        ng = len(labels)
        self.levels = list(range(ng)) if k_trt is None else list(dict.fromkeys(labels[:, k_trt]))
        if control is None:
            ctrl_levels = range(len(self.levels) - 1)
        elif control in self.levels:
            ctrl_levels = [self.levels.index(control)]
        else:
            raise ValueError(f"control value {control!r} does not occur in the treatment column")
        self.pairs, self.parts = [], []
        for b in ctrl_levels:
            d = _TwoGroupDesigns(ng, self.levels[b]) if k_trt is None else _design.VsControlDesigns(labels, k_trt, self.levels[b], Nc)
            # with a given control every other level is tested; among all pairs, the levels after b
            guides = [self.levels.index(g) for g in d.guides]
            cols = [i for i, a in enumerate(guides) if control is not None or a > b]
            self.pairs.extend((guides[i], b) for i in cols)
            self.parts.append((d, np.asarray(cols, dtype=np.int64)))

    def tests(self, good):
        """Design id per test, into the tables ``tables()`` returns AFTER this call, for the genes of ``good`` [gene][group]:
        gene-major x pair."""
        good = np.asarray(good, dtype=bool)
        ids = [d.tests(good).reshape(good.shape[0], -1)[:, cols] for d, cols in self.parts]     # (adds this chunk's new designs)
        n_designs = [len(d.tables()[0]) - 1 for d, _ in self.parts]
        first = np.concatenate([[0], np.cumsum(n_designs)[:-1]]).astype(np.int64)
        return np.concatenate([i + f for i, f in zip(ids, first)], axis=1).astype(np.int32).reshape(-1)

    def tables(self):
        """(design_ptr, design_grp, design_w) of every part's designs, one part after the other."""
        ptr, grp, w, n = [np.zeros(1, np.int32)], [], [], 0
        for d, _ in self.parts:
            p, g, ww = d.tables()
            ptr.append(p[1:] + n)
            grp.append(g)
            w.append(ww)
            n += len(g)
        return np.concatenate(ptr).astype(np.int32), np.concatenate(grp).astype(np.int32), np.concatenate(w).astype(np.float64)


def adjusted_columns(p, adj, fam, n_mem, se=None, crit=None):
    """The adjusted columns of ``ht_1d_posthoc`` / ``ht_2d_posthoc`` on ONE plane, from what ``family_maxt`` returns for families
    of ``n_mem`` members each: ``p`` [test] the members' own p-values, ``adj`` [test][2] (t0, n_adj), ``fam`` [family][2]
    (n_valid_family, n_included).  -> (``p_adj`` [test]: max((1 + n_adj) / (1 + n_valid_family), p) where the member is included,
    NaN elsewhere; ``n_family`` [test] int64: the family's included members; ``half`` [test]: the half-width ``crit`` [family] x
    ``se`` [test] of the simultaneous interval of an included member, NaN elsewhere -- None without ``crit``)."""
    live = ~np.isnan(adj[:, 0])
    p_adj = (1 + adj[:, 1]) / (1 + np.repeat(fam[:, 0], n_mem))
    with np.errstate(invalid="ignore"):
        p_adj = np.where(live, np.maximum(p_adj, p), np.nan)
    n_family = np.repeat(fam[:, 1], n_mem).astype(np.int64)
    half = None if crit is None else np.where(live, np.repeat(crit, n_mem) * se, np.nan)
    return p_adj, n_family, half


def surviving_cols(bs, good, num_boot):
    """The replicate columns that survive hypothesis_test.py:249-251 / :372-373 (``bs.valid_cols``); (None, None) when nothing
    was dropped (the usual case): identity map."""
    col_map, n_valid = bs.valid_cols(good)
    if (n_valid[good.any(axis=1)] == num_boot + 1).all():
        return None, None
    return col_map, n_valid


def merge_resampled(coef, stt, coef_r, stt_r, rr_test):
    """Coefficient rows (device) and statistics (host) of all tests: the resampled ones where ``rr_test``, else the plain ones."""
    rr_idx = engine.dev(np.flatnonzero(rr_test))
    coef[rr_idx] = coef_r[rr_idx]
    return coef, np.where(rr_test[:, None], stt_r, stt)


# ----------------------------------------------------------------------------------------------
# 2D: pair chunks
# ----------------------------------------------------------------------------------------------


def distinct_pairs(idx1, idx2):
    """The distinct unordered pairs of a pair list: ``first`` = position of every distinct pair's first appearance (self pairs
    skipped; main.py:467-482), ``members[k]`` = all positions that share pair k's result."""
    first, members, seen = [], [], {}
    for c in range(len(idx1)):
        a, b = int(idx1[c]), int(idx2[c])
        if a == b:
            continue
        k = seen.setdefault(frozenset((a, b)), len(first))
        if k == len(first):
            first.append(c)
            members.append([])
        members[k].append(c)
    return np.asarray(first, dtype=np.int64), members


def pair_plan(m, st, num_boot, max_rows, extra_rows=0):
    """The pairs of ``compute_2d_moments`` as the 2D tests run them: ``first`` / ``members`` (``distinct_pairs`` over the
    ``n_conv`` requested pairs), ``c1`` / ``c2`` = the distinct pairs' column slots, ``true_corr`` [pair][group], ``skip``
    (hypothesis_test.py:325), ``chain_key`` and the chunk ``bounds``: pairs are independent, so they run in chunks of at most
    ``max_rows`` replicate rows ([pair x group][B+1] fp64) AND at most a third of the free HBM in histogram tables.  ``extra_rows``:
    the rows of that width a pair holds beside its groups' (the maximum row of ``ht_2d_posthoc``), counted against ``max_rows``."""
    groups = m['groups']
    ng = len(groups)
    idx1, idx2 = m['2d_moments']['gene_idx_1'], m['2d_moments']['gene_idx_2']
    first, members = distinct_pairs(idx1, idx2)
    P_ = len(first)
    slot = {int(g): i for i, g in enumerate(st.cols_local)}
    c1 = np.array([slot[int(idx1[c])] for c in first], dtype=np.int64)
    c2 = np.array([slot[int(idx2[c])] for c in first], dtype=np.int64)
    true_corr = np.stack([m['2d_moments'][g]['corr'][first] for g in groups], axis=1) if P_ else np.zeros((0, ng))   # [pair][group]
    with np.errstate(invalid="ignore"):
        skip = np.isnan(true_corr) | (np.abs(true_corr) == 1)
    if max_rows is None:
        max_rows = min(1 << 19, engine.auto_max_rows(num_boot + 1, arrays=1))   # also bounds the per-pair 2D tables
    chunk = max(1, int(max_rows) // max(1, ng + int(extra_rows)))
    tab_bytes = engine.pair_table_bytes(st.maxx, st.cols.genes, c1, c2, ng, len(st.sf_table)) if P_ else np.zeros(0, dtype=np.int64)
    budget = max(1 << 28, engine._torch().cuda.mem_get_info()[0] // 3)
    bounds, acc = [0], 0
    for k in range(P_):
        if k - bounds[-1] >= chunk or (acc + int(tab_bytes[k]) > budget and k > bounds[-1]):
            bounds.append(k)
            acc = 0
        acc += int(tab_bytes[k])
    bounds.append(P_)
    return SimpleNamespace(
        ng=ng, n_conv=idx1.shape[0], idx1=idx1, first=first, members=members, P_=P_, c1=c1, c2=c2, true_corr=true_corr, skip=skip,
        bounds=bounds, gq=np.array([m['group_q'][g] for g in groups]),
        chain_key=np.arange(P_ * ng, dtype=np.int64))        # rng='fast': stream key of (pair k, group) = k * n_groups + group


def chunks_2d(st, plan, num_boot):
    """Open the distinct pairs in the chunks of ``plan.bounds``: yields ``c`` with ``lo``, ``hi``, ``n_ch``, ``bs`` (pair tables
    built) and ``so`` = the device pair order (sorted by left column).  ``c`` is ONE object, emptied before the next chunk is opened
    (release-before-allocate).  ``st.last_bootstrap2d`` / ``st.last_chunk2d`` hold the last chunk afterwards (diagnostics / tests:
    pair range of the last chunk)."""
    c = SimpleNamespace(bs=None)
    for lo, hi in zip(plan.bounds[:-1], plan.bounds[1:]):
        if hi <= lo:
            continue
        c.__dict__.clear()      # release the previous chunk's tables and replicate rows first: the caching allocator hands them back
        c.lo, c.hi, c.n_ch = lo, hi, hi - lo
        c.bs = engine.Bootstrap2D(st.cols, plan.c1[lo:hi], plan.c2[lo:hi], st.maxx, st.sf_bin, st.sf_table, plan.gq, num_boot)
        c.so = c.bs.order
        yield c
    st.last_bootstrap2d = c.bs
    st.last_chunk2d = (plan.bounds[-2], plan.bounds[-1]) if plan.P_ else (0, 0)


def run_chunk_2d(c, plan, uniforms, rng, fill_seed, keep_fast=False):
    """Bootstrap the chunk's chains with the hash ``uniforms`` [3][pair x group] of the whole call; -> ``good`` [pair][group] in
    device pair order.  ``keep_fast`` (rng='fast'): the chunk keeps what ``continue_chunk_2d`` launches from."""
    ng = plan.ng

    def to_dev_order(a):
        return a[c.lo * ng:c.hi * ng].reshape(c.n_ch, ng)[c.so].reshape(-1)

    r1a, r1b, r0 = uniforms
    c.bs.run(to_dev_order(plan.skip.reshape(-1)), to_dev_order(r1a), to_dev_order(r1b), to_dev_order(r0),
             to_dev_order(np.where(plan.skip, np.nan, plan.true_corr).reshape(-1)), fast=(rng == 'fast'), fast_seed=fill_seed,
             pair_key=to_dev_order(plan.chain_key), keep_fast=keep_fast)
    return c.bs.active.reshape(c.n_ch, ng)


def continue_chunk_2d(c, ng, test_pair, W, good, stats, schedule, min_extreme, resampling, n_open):
    """Rounds 1.. of the sequential bootstrap on an open pair chunk whose round 0 (``run_chunk_2d`` with rng='fast' and
    ``keep_fast``, then ``bs.contract``) gave the records ``stats`` [test][8] of the tests (``test_pair`` [test] in device pair
    order, weight rows ``W`` [test][group], ``good`` [pair][group]): the one-plane analogue of ``continue_chunk_1d``.  A test is
    continued while it is open (``open_tests``).  Round j bootstraps the global replicates [schedule[j - 1], schedule[j]) of the
    chains of the good groups of the pairs that still have an open test -- every other slot of the chunk's tile layout is skipped
    -- into a pair-granular plane [open pairs x groups][1 + rep_n] (column 0 copied from the chunk, everything else NaN until
    the launch writes it), contracts the open tests only, with their own weight rows and ``good`` rows and renumbered pairs, and
    folds their records (``merge_records``).  There is no refill in 2D: an invalid replicate is a NaN column that the contraction
    drops, so the counts of a test that is never closed are those of a one-shot call over ``schedule[-1]`` replicates.  The
    round's plane is allocated once per round and released before the next; together with the coefficient row that
    mm_contract_stats writes per open test it never holds more bytes than the chunk's replicate rows (a single pair excepted):
    a round with more takes its open pairs in sub-batches (pairs are independent, and the streams are keyed by chain, so neither
    this nor the chunking changes a number).  ``n_open`` [round]: the tests open after round j are added to entry j.
    -> the merged records."""
    bs = c.bs
    test_pair, W, good = np.asarray(test_pair, dtype=np.int64), np.asarray(W, dtype=np.float64), np.asarray(good, dtype=bool)
    grp = np.arange(ng)

    def batches(j, idx, ld):
        pairs, per_pair = np.unique(test_pair[idx], return_counts=True)
        per = int(min(len(pairs), max(1, (bs.n_q * bs.ld) // ((ng + int(per_pair.max())) * ld))))
        subs = [pairs[lo:lo + per] for lo in range(0, len(pairs), per)]
        return per * ng, [(np.flatnonzero(np.isin(test_pair[idx], psub)), psub) for psub in subs]

    def run(plane, rep_lo, rep_n, tests, psub):
        ld = 1 + rep_n
        sub = plane[:len(psub) * ng]
        rows_old = (psub[:, None] * ng + grp).reshape(-1)
        sub.fill_(float("nan"))
        sub[:, 0] = bs.yc[engine.dev(rows_old), 0]
        g_sub = good[psub]
        rows_new = np.flatnonzero(g_sub.reshape(-1))
        keep = bs.launch_range(rep_lo, rep_n, rows_old[rows_new], sub, rows_new)
        coef, new = engine.contract_plane(sub, ld, rep_n, ng, len(psub), np.searchsorted(psub, test_pair[tests]), W[tests], g_sub)
        del keep, coef
        return new

    return _rounds_2d(stats, schedule, min_extreme, resampling, n_open, batches, run)


def _rounds_2d(stats, schedule, min_extreme, resampling, n_open, batches, run, on_round=None):
    """The round loop of the sequential 2D bootstrap, shared by its drivers (``continue_chunk_2d``, ``continue_chunk_2d_designs``):
    before round j >= 1 the tests still open (``open_tests`` on the merged records) are counted into ``n_open[j - 1]``; none open
    ends the rounds.  ``batches(j, idx, ld)`` -> (rows of the round's plane, [(positions into ``idx``, job)]) says how the open tests
    ``idx`` are taken, ``run(plane, rep_lo, rep_n, tests, job)`` -> records [len(tests)][8] bootstraps and contracts one sub-batch
    on the leading rows of ``plane`` [rows][1 + rep_n], which is allocated once per round and released before the next
    (release-before-allocate); the round's records are folded by ``merge_records``.  ``on_round(j, is_open)`` sees every mask.
    -> the merged records."""
    torch = engine._torch()
    merged = np.array(stats, dtype=np.float64)
    for j in range(1, len(schedule)):
        is_open = open_tests(merged, min_extreme, resampling)
        n_open[j - 1] += int(is_open.sum())
        if on_round is not None:
            on_round(j, is_open)
        if not is_open.any():
            break
        idx = np.flatnonzero(is_open)
        rep_lo, rep_n = schedule[j - 1], schedule[j] - schedule[j - 1]
        n_rows, subs = batches(j, idx, 1 + rep_n)
        plane = engine.empty((n_rows, 1 + rep_n), torch.float64)
        new = np.empty((len(idx), 8))
        for pos, job in subs:
            new[pos] = run(plane, rep_lo, rep_n, idx[pos], job)
        del plane      # release-before-allocate: the next round's plane takes this buffer
        merged[idx] = merge_records([merged[idx], new])
    else:
        n_open[len(schedule) - 1] += int(open_tests(merged, min_extreme, resampling).sum())
    return merged


def design_round_tables(test_pair, test_design, design_ptr, design_grp, design_w, ng):
    """What a round of ``continue_chunk_2d_designs`` launches and contracts for the given (open) tests -- ``test_pair`` [test],
    ``test_design`` [test] into the CSR tables (``design_ptr``, ``design_grp``, ``design_w``) -- as plain arrays; pure numpy.
    -> ``chains``: the distinct q = pair * ng + group over the entries of the tests' designs, ascending (``_design_chains``): row i
    of the round's compact plane is chain ``chains[i]``; ``ptr`` [test + 1], ``rows``, ``w``: one design PER TEST, whose entries
    are those of the test's shared design in the same order, weights unchanged, the group replaced by the chain's plane row."""
    design_ptr, design_grp, design_w = np.asarray(design_ptr, dtype=np.int64), np.asarray(design_grp, dtype=np.int64), np.asarray(design_w, dtype=np.float64)
    test_pair, test_design = np.asarray(test_pair, dtype=np.int64).reshape(-1), np.asarray(test_design, dtype=np.int64).reshape(-1)
    lo, cnt = design_ptr[test_design], np.diff(design_ptr)[test_design]
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    pos = np.repeat(lo - ptr[:-1], cnt) + np.arange(int(ptr[-1]))
    q = np.repeat(test_pair, cnt) * ng + design_grp[pos]
    chains, rows = np.unique(q, return_inverse=True)
    return chains, ptr, np.asarray(rows, dtype=np.int64).reshape(-1), design_w[pos]


def design_batches(test_pair, test_design, design_ptr, design_grp, ng, max_chains):
    """Cut the given tests, in their order, into contiguous runs [(lo, hi)] whose designs read at most ``max_chains`` distinct
    chains each (a single test that reads more is a run of its own), taking as many tests per run as fit; pure numpy.  The tests
    of a driver are pair-major, so a pair's control chains are usually shared within one run."""
    n = len(test_pair)
    chains, ptr, rows, _ = design_round_tables(test_pair, test_design, design_ptr, design_grp, np.zeros(len(design_grp)), ng)
    if len(chains) <= max_chains or n <= 1:
        return [(0, n)] if n else []
    test_of = np.repeat(np.arange(n), np.diff(ptr))
    # prev[e]: the test of the previous entry on the same chain (-1: none); entry e adds a chain to a run from s on iff prev[e] < s
    by_row = np.argsort(rows, kind="stable")
    prev = np.full(len(rows), -1, dtype=np.int64)
    same = rows[by_row][1:] == rows[by_row][:-1]
    prev[by_row[1:][same]] = test_of[by_row[:-1][same]]
    runs, s = [], 0
    while s < n:
        e0 = int(ptr[s])
        seen = np.cumsum(prev[e0:] < s)                                # distinct chains of the entries e0..e
        per_test = seen[ptr[s + 1:] - e0 - 1] if len(seen) else np.zeros(0, dtype=np.int64)
        per_test = np.where(np.diff(ptr)[s:] > 0, per_test, 0)          # (an empty design reads nothing)
        per_test = np.maximum.accumulate(per_test)
        hi = s + max(1, int(np.searchsorted(per_test, max_chains, side="right")))
        runs.append((s, hi))
        s = hi
    return runs


def continue_chunk_2d_designs(c, ng, test_pair, test_design, tables, stats, schedule, min_extreme, resampling, n_open, n_chains=None,
                              open_mask=None, budget=None):
    """``continue_chunk_2d`` for tests given as (pair, design id) over CSR design tables ``tables`` = (design_ptr, design_grp,
    design_w): the rounds of ``ht_2d_vs_control_sequential(max_boot=...)``, on an open pair chunk whose round 0 (``run_chunk_2d`` with
    rng='fast' and ``keep_fast``, then ``bs.contrast`` / ``bs.contrast_design``) gave the records ``stats`` [test][8] of the tests
    (``test_pair`` [test] in device pair order, pair-major).  Same round loop (``_rounds_2d``); what differs is the granularity.
    Round j bootstraps exactly the chains that an open test's design reads -- the guide's groups and the control's, not every
    group of the pair -- into a COMPACT plane [chain][1 + rep_n], one row per chain (``design_round_tables``; column 0 copied
    from the chunk, everything else NaN until the launch writes it), by ONE ``bs.launch_listed``, whose grid is sized by
    those chains and not by the chunk's tile layout.  A chain that did not run in round 0 is left out by the launch; its columns
    are dropped by the contraction, as in the one-shot call.  The open tests are contracted by mm_contrast_design1_stats with the
    compact plane as ONE row block of ``len(chains)`` groups and one design per test (the shared design's entries in the same
    order and with the same weights, the group replaced by the plane row), so every coefficient is the same sum in the same order
    as in round 0 and the counts of a test that never closes are those of the one-shot call over ``schedule[-1]`` replicates.
    ``budget`` (doubles; default the chunk's own replicate rows, ``bs.n_q * bs.ld``): a round whose plane would be larger takes
    its open tests in sub-batches, contiguous runs in pair-major order (``design_batches``); the streams are keyed by chain, so
    neither this nor the chunking changes a number (a chain shared by two runs is bootstrapped in both, to the same values).
    ``n_open`` [round] as in ``continue_chunk_2d``; diagnostics: ``n_chains`` [round]: the distinct chains that the open tests of
    round j read are added to entry j; ``open_mask`` [round]: entry j is set to the open mask [test] before round j.
    -> the merged records."""
    bs = c.bs
    design_ptr, design_grp, design_w = (np.asarray(a) for a in tables)
    test_pair, test_design = np.asarray(test_pair, dtype=np.int64), np.asarray(test_design, dtype=np.int64)
    budget = bs.n_q * bs.ld if budget is None else int(budget)

    def on_round(j, is_open):
        if open_mask is not None:
            open_mask[j] = is_open.copy()

    def batches(j, idx, ld):
        runs = design_batches(test_pair[idx], test_design[idx], design_ptr, design_grp, ng, max(1, budget // ld))
        jobs = [design_round_tables(test_pair[idx[lo:hi]], test_design[idx[lo:hi]], design_ptr, design_grp, design_w, ng) for lo, hi in runs]
        if n_chains is not None:
            n_chains[j] += len(jobs[0][0]) if len(jobs) == 1 else len(_design_chains(test_pair[idx], test_design[idx], design_ptr, design_grp, ng))
        return max(1, max(len(job[0]) for job in jobs)), [(np.arange(lo, hi), job) for (lo, hi), job in zip(runs, jobs)]

    def run(plane, rep_lo, rep_n, tests, job):
        chains, ptr, rows, w = job
        sub = plane[:max(1, len(chains))]
        sub.fill_(float("nan"))
        if len(chains):
            sub[:len(chains), 0] = bs.yc[engine.dev(chains), 0]
        keep = bs.launch_listed(rep_lo, rep_n, chains, sub, np.arange(len(chains)))
        (new,), _ = engine._contrast_design([sub], 1 + rep_n, rep_n, max(1, len(chains)), 1, np.zeros(len(tests), dtype=np.int32),
                                            np.arange(len(tests)), ptr, rows, w)
        del keep
        return new

    return _rounds_2d(stats, schedule, min_extreme, resampling, n_open, batches, run, on_round)


def scatter_pairs(c, plan, dst, src, keep=None):
    """Results of the chunk's pairs (``src`` [pair][...], device pair order) to every requested pair that shares them
    (``dst`` [n_conv][...]); ``keep`` [pair]: the pairs that have a result."""
    src = np.asarray(src).reshape(c.n_ch, -1)
    for k in range(c.n_ch):
        if keep is None or keep[k]:
            dst[plan.members[c.lo + c.so[k]]] = src[k]
