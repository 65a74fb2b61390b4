"""CPU tests of what the four ht_* drivers share (memento/_ht.py) and of the strict 1D replay (memento/_strict1d.py): the distinct
pairs of a pair list, the per-mask design tables against design.weight_rows / design.residual_parts called directly, the hash
uniforms and the strict replay's np.random order against the reference's order written out call by call, and the ``rng`` check
of every driver.  No device: the strict replay is driven by a fake bootstrap whose rows are numpy arrays."""

from types import SimpleNamespace

import numpy as np
import pytest

from scrna_parameter_estimation_amd import memento
from scrna_parameter_estimation_amd.memento import _ht, _strict1d
from scrna_parameter_estimation_amd.memento import design as _design


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---------------------------------------------------------------------------------------------- distinct pairs


def test_distinct_pairs_first_appearance_members_and_self_pairs():
    a, b, c = 0, 1, 2
    pairs = [(a, b), (b, a), (c, c), (b, c), (a, b)]
    first, members = _ht.distinct_pairs(np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]))
    assert first.dtype == np.int64 and first.tolist() == [0, 3]
    assert members == [[0, 1, 4], [3]]
    assert all(2 not in mem for mem in members)                 # the self pair shares nobody's result
    first, members = _ht.distinct_pairs(np.zeros(0, dtype=int), np.zeros(0, dtype=int))
    assert first.shape == (0,) and first.dtype == np.int64 and members == []


# ---------------------------------------------------------------------------------------------- design tables

# 4 groups = 2 conditions x 2 replicates; covariate: a replicate dummy; treatment: condition, and an all-ones column
COV = np.array([[0.0], [1.0], [0.0], [1.0]])
TRT = np.array([[0.0, 1.0], [0.0, 1.0], [1.0, 1.0], [1.0, 1.0]])
NC = np.array([120.0, 75.0, 210.0, 40.0])
GOOD = np.array([[1, 1, 1, 1],       # all good
                 [1, 0, 1, 1],       # one group bad
                 [1, 0, 1, 1],       # the same mask again
                 [0, 0, 0, 0]],      # no good group
                dtype=bool)


@pytest.mark.parametrize("cols", [[None] * 4, [(0,), (1,), (1,), (0, 1)]], ids=["all-columns", "per-row-columns"])
def test_design_tables_equal_the_design_functions_called_directly(cols):
    d = _ht.design_tables(GOOD, cols, COV, TRT, NC, resampled=True)
    want_row, want_W, want_tt, want_rr = [], [], [], []
    for k in range(4):
        t = TRT if cols[k] is None else TRT[:, list(cols[k])]
        W = _design.weight_rows(COV, t, NC, GOOD[k])
        M, tt = _design.residual_parts(COV, t, NC, GOOD[k])
        assert np.array_equal(d.Mstack[d.row_mask[k]], M)
        want_row += [k] * t.shape[1]
        want_W.append(W)
        want_tt.append(tt)
        # not resampled: the good groups' treatment is all ones (here: exactly the rows tested on column 1 alone), or no good group
        want_rr += [bool(GOOD[k].any() and not (t[GOOD[k]] == 1).all())] * t.shape[1]
    assert d.test_row.tolist() == want_row
    assert np.array_equal(d.Wmat, np.concatenate(want_W)) and np.array_equal(d.tt_mat, np.concatenate(want_tt))
    assert d.rr_test.dtype == bool and d.rr_test.tolist() == want_rr
    assert want_rr == ([True, True, True, True, True, True, False, False] if cols[0] is None else [True, False, False, False, False])
    assert d.row_mask[1] == d.row_mask[2] and len(d.Mstack) == 3                  # the repeated mask reuses its entry
    lo, hi = (2, 4) if cols[0] is None else (1, 2)
    assert np.array_equal(d.Wmat[lo:hi], d.Wmat[hi:2 * hi - lo]) and np.array_equal(d.tt_mat[lo:hi], d.tt_mat[hi:2 * hi - lo])
    plain = _ht.design_tables(GOOD, cols, COV, TRT, NC)
    assert np.array_equal(plain.Wmat, d.Wmat) and plain.test_row.tolist() == want_row
    assert plain.tt_mat is None and plain.Mstack is None and plain.row_mask is None and plain.rr_test is None


def test_design_tables_of_no_rows():
    d = _ht.design_tables(np.zeros((0, 4), dtype=bool), [], COV, TRT, NC, resampled=True)
    assert d.Wmat.shape == (0, 4) and d.tt_mat.shape == (0, 4) and d.Mstack.shape == (0, 4, 4) and d.rr_test.shape == (0,)


def test_pair_design_tables_take_the_all_ones_verdict_over_the_whole_treatment():
    """ht_2d_moments without treatment_for_gene, as recorded in the goldens: the weight row is column 0's, the residual parts and
    the all-ones test use ALL treatment columns and row 0 is kept -- so a pair whose column 0 is all ones is still resampled when
    another column is not."""
    trt = TRT[:, ::-1].copy()                                   # column 0 all ones, column 1 the condition
    d = _ht.pair_design_tables(GOOD, np.zeros(4, dtype=np.int64), False, COV, trt, NC, resampled=True)
    assert d.test_row.tolist() == [0, 1, 2, 3] and d.rr_test.tolist() == [True, True, True, False]
    for k in range(4):
        assert np.array_equal(d.Wmat[k], _design.weight_rows(COV, trt[:, [0]], NC, GOOD[k])[0])
        M, tt = _design.residual_parts(COV, trt, NC, GOOD[k])
        assert np.array_equal(d.Mstack[d.row_mask[k]], M) and np.array_equal(d.tt_mat[k], tt[0])
    # with treatment_for_gene the pair's own column decides: column 0 (all ones) is not resampled, column 1 is
    d = _ht.pair_design_tables(GOOD, np.array([0, 1, 1, 1]), True, COV, trt, NC, resampled=True)
    assert d.rr_test.tolist() == [False, True, True, False]
    for k, col in enumerate([0, 1, 1, 1]):
        assert np.array_equal(d.Wmat[k], _design.weight_rows(COV, trt[:, [col]], NC, GOOD[k])[0])
        assert np.array_equal(d.tt_mat[k], _design.residual_parts(COV, trt[:, [col]], NC, GOOD[k])[1][0])


# ---------------------------------------------------------------------------------------------- hash uniforms


@pytest.mark.parametrize("k", [2, 3])
def test_hash_uniforms_take_the_references_stream_positions(k):
    live = np.array([True, False, True, True, False, True])
    np.random.seed(11)
    got = _ht.hash_uniforms(live, k)
    state = np.random.get_state()
    np.random.seed(11)
    want = np.zeros((k, 6))
    for p in np.flatnonzero(live):                              # bootstrap.py:62, :65 per chain, in chain order
        want[:k - 1, p] = np.random.random(k - 1)
        want[k - 1, p] = np.random.random()
    assert np.array_equal(got, want) and (got[:, ~live] == 0).all()
    assert _same_state(state, np.random.get_state())


def test_chunks_1d_yields_nothing_when_no_gene_is_kept():
    """strict=True runs all genes as one chunk, chunk = G_all: with no gene kept (an empty shard) that is 0, and the loop must
    end without a chunk -- and without touching the device -- leaving the diagnostics of an empty call."""
    st = SimpleNamespace(gene_idx=np.zeros(0, dtype=np.int64), last_bootstrap="previous", last_chunk=None)
    for chunk in (0, 5):
        assert list(_ht.chunks_1d(st, None, 10, chunk)) == []
        assert st.last_bootstrap is None and st.last_chunk == (0, 0)


# ---------------------------------------------------------------------------------------------- strict replay

NG, B = 2, 4                                                    # 3 genes x 2 groups, 4 replicates
ROW2 = np.array([0.5, 0.1, np.nan, 0.3, 0.4])                   # mean row with one invalid replicate (column 0 = the true value)


class _FakeBootstrap:
    """Stands in for Bootstrap1D: numpy rows; ``run_from(first)`` returns n_inv of the rows >= first from the fixed ``table``."""

    def __init__(self, table, nan_rows):
        self.ng, self.B, self.n_pairs = NG, B, len(table)
        self.K = np.full(self.n_pairs, 3)
        self.table = np.asarray(table, dtype=np.int32)
        self.ym = np.tile(np.arange(B + 1, dtype=np.float64), (self.n_pairs, 1))
        self.yv = self.ym + 10
        for p in nan_rows:
            self.ym[p] = ROW2
        self.firsts = []

    def run_from(self, r1, r0, first_pair):
        self.firsts.append(first_pair)
        return self.table[first_pair:].copy()

    def valid_cols(self, good):
        return None, np.full(self.n_pairs // NG, B + 1)


def _replay(bs, gene_trt=None):
    c = SimpleNamespace(bs=bs, skip=np.zeros(bs.n_pairs, dtype=bool))
    return _strict1d.StrictReplay(c, bs.run_from, gene_trt, load=lambda t, p: t[p, 1:], store=_store)


def _store(t, p, row):
    t[p, 1:] = row


def _expect_hash(r1, r0, pairs):
    for p in pairs:
        r1[p] = np.random.random(1)[0]                          # bootstrap.py:62
        r0[p] = np.random.random()                              # bootstrap.py:65


def _expect_fill():
    row = ROW2[1:]
    return np.random.choice(row[~np.isnan(row)], 1)             # hypothesis_test.py:23-33


def _expect_assign(n):
    ra = np.random.choice(n, size=(n, B))                       # hypothesis_test.py:275-278
    ra[:, 0] = np.arange(n)
    ba = np.random.choice(B, (n, B)) + 1
    ba[:, 0] = 0
    return ra, ba


# pair 2 has one invalid mean replicate, pair 5 no valid one
TABLE = [[0, 0], [0, 0], [1, 0], [0, 0], [0, 0], [-1, -1]]


def test_strict_replay_order_without_resample_rep():
    bs = _FakeBootstrap(TABLE, nan_rows=[2])
    np.random.seed(21)
    replay = _replay(bs)
    bad_fill = replay.run()
    state = np.random.get_state()

    np.random.seed(21)
    r1, r0 = np.zeros(6), np.zeros(6)
    _expect_hash(r1, r0, [0, 1, 2])
    fill = _expect_fill()
    _expect_hash(r1, r0, [3, 4, 5])
    assert np.array_equal(replay.r1, r1) and np.array_equal(replay.r0, r0)
    assert _same_state(state, np.random.get_state())
    assert np.array_equal(bs.ym[2], [0.5, 0.1, fill[0], 0.3, 0.4])
    assert bs.firsts == [0, 3]                                  # rolled back to pair 2, went on after it
    assert replay.known_bad.tolist() == [False] * 5 + [True]
    assert bad_fill.tolist() == [False] * 5 + [True]
    assert replay.rep_assign is None and replay.bcol_assign is None


@pytest.mark.parametrize("fill_pair", [2, 3], ids=["fill-first-group", "fill-last-group"])
def test_strict_replay_order_with_resample_rep(fill_pair):
    """The reference's order: per gene the hash uniforms of its groups -- each group's _fill right after that group's bootstrap,
    before the next group's uniforms -- then the gene's two assignment draws: after its last group's uniforms, and after that
    group's fill when it needed one.  Gene 2 has one good group left (pair 5 has no valid replicate): its draws are for n = 1."""
    table = [[0, 0]] * 6
    table[fill_pair], table[5] = [1, 0], [-1, -1]
    bs = _FakeBootstrap(table, nan_rows=[fill_pair])
    trt = np.array([[0.0], [1.0]])                              # not constant: every gene with a good group is resampled
    np.random.seed(22)
    replay = _replay(bs, gene_trt=[trt] * 3)
    bad_fill = replay.run()
    state = np.random.get_state()

    np.random.seed(22)
    r1, r0 = np.zeros(6), np.zeros(6)
    _expect_hash(r1, r0, [0, 1])
    a0 = _expect_assign(2)
    if fill_pair == 2:
        _expect_hash(r1, r0, [2])
        fill = _expect_fill()
        _expect_hash(r1, r0, [3])
    else:
        _expect_hash(r1, r0, [2, 3])
        fill = _expect_fill()
    a1 = _expect_assign(2)
    _expect_hash(r1, r0, [4, 5])
    a2 = _expect_assign(1)
    assert np.array_equal(replay.r1, r1) and np.array_equal(replay.r0, r0)
    assert _same_state(state, np.random.get_state())
    assert np.array_equal(bs.ym[fill_pair], [0.5, 0.1, fill[0], 0.3, 0.4])
    assert replay.known_bad.tolist() == [False] * 5 + [True] and bad_fill.tolist() == [False] * 5 + [True]
    for gi, (ra, ba) in enumerate([a0, a1, a2]):
        n = ra.shape[0]
        assert np.array_equal(replay.rep_assign[gi, :n], ra) and np.array_equal(replay.bcol_assign[gi, :n], ba)
    assert replay.rep_assign.dtype == np.int16 and replay.bcol_assign.dtype == np.int32


# ---------------------------------------------------------------------------------------------- rng validation


@pytest.mark.parametrize("call", [
    lambda: memento.ht_1d_moments(None, None, None, rng="bogus", resampling="bootstrap"),
    lambda: memento.ht_1d_vs_control(None, 0, rng="bogus"),
    lambda: memento.ht_2d_moments(None, None, None, rng="bogus", resampling="bootstrap"),
    lambda: memento.ht_2d_vs_control(None, 0, rng="bogus"),
], ids=["ht_1d_moments", "ht_1d_vs_control", "ht_2d_moments", "ht_2d_vs_control"])
def test_every_driver_rejects_an_unknown_rng_before_touching_adata(call):
    with pytest.raises(ValueError, match="rng must be 'replay' or 'fast'"):
        call()
