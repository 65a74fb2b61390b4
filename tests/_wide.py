"""Helpers of the wide-matrix tests (more genes than one engine.CountBlocks holds): embedding a small fixture among all-zero
columns, and sparse synthetic counts at real widths without a dense array."""

import numpy as np
import scipy.sparse as sp


def boundary_positions(G, part_genes):
    """The columns at and next to every part boundary of a G-wide matrix, and 65,535 / 65,536 (the old limit), that lie in [0, G)."""
    want = {0, part_genes - 1, part_genes, 65_535, 65_536, 2 * part_genes - 1, 2 * part_genes, G - 1}
    return np.array(sorted(p for p in want if 0 <= p < G), dtype=np.int64)


def wide_positions(n, G, part_genes, seed=0):
    """``n`` ascending columns of a G-wide matrix: boundary_positions, the rest drawn from a fixed seed."""
    must = boundary_positions(G, part_genes)
    assert len(must) <= n <= G
    rest = np.setdiff1d(np.arange(G), must)
    extra = np.random.default_rng(seed).choice(rest, size=n - len(must), replace=False)
    return np.sort(np.concatenate([must, extra])).astype(np.int64)


def embed(X, G, positions):
    """The columns of the CSR ``X``, order preserved, at the ascending ``positions`` of a G-wide CSR; every other column is empty."""
    X = sp.csr_matrix(X)
    positions = np.asarray(positions, dtype=np.int64)
    assert positions.shape == (X.shape[1],) and (np.diff(positions) > 0).all() and 0 <= positions[0] and positions[-1] < G
    Y = sp.csr_matrix((X.data.copy(), positions[X.indices].astype(np.int32), X.indptr.copy()), shape=(X.shape[0], G))
    Y.has_sorted_indices = bool(X.has_sorted_indices)      # an ascending map keeps sorted rows sorted
    return Y


def embed_names(names, G, positions):
    """The fixture's gene names at ``positions``, filler names elsewhere."""
    out = np.array([f"filler{j}" for j in range(G)], dtype=object)
    out[np.asarray(positions)] = list(names)
    return out


def sparse_counts(n_cells, G, nnz, seed, occupied=()):
    """About ``nnz`` positive integer counts (1..9, a few up to 400) scattered over an n_cells x G float32 CSR; every column of
    ``occupied`` gets some twenty of them.  Built from coordinates: no dense array."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_cells, size=nnz)
    cols = rng.integers(0, G, size=nnz)
    occupied = np.repeat(np.asarray(occupied, dtype=np.int64), 20)
    cols[:len(occupied)] = occupied
    vals = rng.integers(1, 10, size=nnz)
    big = rng.random(nnz) < 0.01
    vals[big] = rng.integers(10, 401, size=int(big.sum()))
    X = sp.coo_matrix((vals.astype(np.float32), (rows, cols)), shape=(n_cells, G)).tocsr()     # duplicates add up: still integers
    X.sort_indices()
    return X
