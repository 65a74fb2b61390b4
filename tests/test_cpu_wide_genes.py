"""CPU tests of the gene-partitioned count blocks: the partition plan, and the premise of the wide GPU tests -- scattering a
fixture's genes among all-zero columns changes nothing the reference computes for them (checked on the oracle)."""

import numpy as np
import pytest

from _wide import embed, wide_positions
from conftest import golden_inputs

WIDTHS = [1, 1024, 59_392, 59_393, 60_000, 60_001, 65_537, 131_073]


@pytest.mark.parametrize("part_genes", [None, 1000])
@pytest.mark.parametrize("G", WIDTHS)
def test_plan_parts(G, part_genes):
    from scrna_parameter_estimation_amd import engine

    parts = engine.plan_parts(G) if part_genes is None else engine.plan_parts(G, part_genes=part_genes)
    width = engine.PART_GENES if part_genes is None else part_genes
    assert parts[0][0] == 0 and parts[-1][1] == G                                   # cover [0, G)
    assert all(a[1] == b[0] for a, b in zip(parts, parts[1:]))                      # contiguous, ascending
    assert all(0 < hi - lo <= width for lo, hi in parts)
    assert (len(parts) == 1) == (G <= width)
    assert len(parts) == -(-G // width)                                             # no more parts than the width asks for


def test_plan_parts_constants_and_arguments():
    from scrna_parameter_estimation_amd import engine

    assert engine.PART_GENES == 59_392 and engine.PART_GENES % 1024 == 0 and engine.PART_GENES <= engine.MAX_PART_GENES == 60_000
    assert engine.plan_parts(3000, part_genes=1024) == [(0, 1024), (1024, 2048), (2048, 3000)]
    assert engine.plan_parts(120_000, part_genes=60_000) == [(0, 60_000), (60_000, 120_000)]
    for bad in (0, -5, 60_001):
        with pytest.raises(ValueError):
            engine.plan_parts(1000, part_genes=bad)


def test_embed_places_columns_and_leaves_the_rest_empty(api_small):
    from scrna_parameter_estimation_amd import engine

    X, _, _, _ = golden_inputs(api_small)
    G = 2 * engine.PART_GENES + 12_289
    pos = wide_positions(X.shape[1], G, engine.PART_GENES)
    for p in (0, engine.PART_GENES - 1, engine.PART_GENES, 65_535, 65_536, 2 * engine.PART_GENES - 1, 2 * engine.PART_GENES, G - 1):
        assert p in pos
    Y = embed(X, G, pos)
    assert Y.shape == (X.shape[0], G) and Y.nnz == X.nnz and Y.has_canonical_format
    assert (Y[:, pos] != X).nnz == 0
    assert np.asarray(Y.sum(axis=0)).ravel()[np.setdiff1d(np.arange(G), pos)].sum() == 0


def test_zero_columns_change_nothing_the_reference_computes(api_small):
    """oracle.setup_size_factors and oracle.compute_1d_moments on api_small embedded at 131,073 genes: size factors, the embedded
    genes' moments, every mask and the mean-variance fit are bit-identical to the compact run, and everything at the added columns
    is zero or false (the fits keep mean > 0 & var > 0, the size factors are row sums, zero columns fail the gene filter)."""
    from oracle import memento_oracle as orc
    from scrna_parameter_estimation_amd import engine

    X, gid, ng, q = golden_inputs(api_small)
    G = 131_073
    pos = wide_positions(X.shape[1], G, engine.PART_GENES)
    added = np.setdiff1d(np.arange(G), pos)
    Y = embed(X, G, pos)
    sf, lv, am, av = orc.setup_size_factors(X, q.mean())
    sfw, lvw, amw, avw = orc.setup_size_factors(Y, q.mean())
    np.testing.assert_array_equal(sfw, sf)
    np.testing.assert_array_equal(lvw[pos], lv)
    np.testing.assert_array_equal(amw[pos], am)
    np.testing.assert_array_equal(avw[pos], av)
    assert not lvw[added].any() and not amw[added].any() and not avw[added].any()
    gq = np.array([q[gid == k].mean() for k in range(ng)])
    mom, momw = orc.compute_1d_moments(X, gid, ng, sf, gq), orc.compute_1d_moments(Y, gid, ng, sfw, gq)
    np.testing.assert_array_equal(momw["overall_gene_filter"][pos], mom["overall_gene_filter"])
    np.testing.assert_array_equal(momw["gene_filter"][:, pos], mom["gene_filter"])
    assert not momw["overall_gene_filter"][added].any() and not momw["gene_filter"][:, added].any()
    for k in ("mean", "var", "res_var", "gene_rv_filter", "mv_fit"):      # (over the kept genes: the same ones, in the same order)
        np.testing.assert_array_equal(momw[k], mom[k], err_msg=k)
