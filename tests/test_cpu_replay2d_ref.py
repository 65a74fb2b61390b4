"""The numpy restatement of the strict 2D replay bootstrap (tests/_replay2d_ref.py) checked on its own (no GPU): its formulas
against oracle/memento_oracle.py on the same weights, the classes of its replicates (value / sentinel / ambiguous) against the
caps the kernel tests rely on, the special chains against their designed outcomes, the sampler regimes of the shared
multiplicities, and the index arithmetic of the slot layout against the bounds of the buffers the kernels are given -- so that
the problem tests/test_gpu_replay2d_kernels.py runs cannot drift."""

import numpy as np
import pytest

from _replay_ref import MENU_NAMES, SF8, XCAP, draw_regimes, menu, ref_weights
from _replay2d_ref import (AMBIGUOUS, SENT, SPECIAL, VALUE, chain_operands_2d, full_tiles_2d, layout2d, many_tiles_2d, menu2d,
                           ordinary_names, ref_corr_2d, twin_tiles_2d)

B = 150
SEEDS = (5, 11)


@pytest.fixture(scope="module")
def orc():
    from oracle import memento_oracle

    return memento_oracle


@pytest.fixture(scope="module")
def refs():
    """{(chain name, seed): (weights, ref_corr_2d of them)} for every chain of the menu, B = 150, seeds 5 and 11."""
    out = {}
    for seed in SEEDS:
        for name, c in menu2d().items():
            o = chain_operands_2d(c)
            w = ref_weights(c.mult, B, seed)
            out[name, seed] = (w, ref_corr_2d(c.x1, c.x2, o.ops[4], o.ops[5], w, c.N, c.q))
    return out


def test_menu_is_the_designed_one():
    m, m1 = menu2d(), menu()
    assert list(m) == list(m1) + list(SPECIAL) and len(ordinary_names()) == 63
    for n, c1 in m1.items():                                                           # the multiplicities of the 1D menu, bin for bin
        c = m[n]
        np.testing.assert_array_equal(c.mult, c1.mult, err_msg=n)
        assert c.q == c1.q and (c.x1.min(), c.x2.min()) >= (0, 0) and max(c.x1.max(), c.x2.max()) < XCAP, n
        assert len(set(zip(c.sf_bin.tolist(), c.x1.tolist(), c.x2.tolist()))) == c.K, n
        assert (c.x2 != c.x1).any(), n
    assert len({c.q for c in m.values()}) == 2
    for c in m.values():                                                               # every chain is in replay order
        code = c.x1 * c.ra + c.x2 * c.rb
        code = code + c.r0 * c.sf
        assert (np.diff(code) > 0).all(), c.name
    # population correlations (the observed sample as weights) of the chains with 10 bins and more: from below -0.4 to above 0.9
    # (the slopes of x2 on x1 span -0.98 to 0.8; the size factor both counts are divided by adds correlation of its own)
    pop = []
    for n in ordinary_names():
        c = m[n]
        o = chain_operands_2d(c)
        r = ref_corr_2d(c.x1, c.x2, o.ops[4], o.ops[5], c.mult[:, None], c.N, c.q)
        if c.K >= 10 and r.kind[0] == VALUE:
            pop.append(float(r.raw[0]))
    pop = [p for p in pop if abs(p) <= 1]
    assert min(pop) < -0.4 and max(pop) > 0.9 and sum(-0.4 < p < 0.5 for p in pop) >= 10, sorted(pop)


def test_special_chains_are_the_designed_ones():
    m = menu2d()
    assert (m["zero_left"].x1 == 0).all() and m["zero_left"].K == 12 and len(set(m["zero_left"].x2.tolist())) > 6
    assert (m["same"].x2 == m["same"].x1).all() and m["same"].K == 20
    assert (m["anti"].x2 == (XCAP - 1) - m["anti"].x1).all() and (m["anti"].sf == 1.0).all()
    assert m["overflow"].x1.min() >= 1e80 and m["overflow"].x2.min() >= 1e80 and m["overflow"].K == 3
    assert m["one_bin2d"].K == 1 and m["one_bin2d"].mult.tolist() == [777] and m["one_bin2d"].x1[0] > 0


def test_operands_are_planes_and_records_of_the_same_bins():
    for c in menu2d().values():
        o = chain_operands_2d(c)
        pk, lq, x1, x2, a, b = o.ops
        assert o.planes.shape == (c.K, 6) and o.recs.shape == (c.K, 8)
        np.testing.assert_array_equal(o.recs[:, :6], o.planes)
        assert (o.recs[:, 6:] == 0).all()
        np.testing.assert_array_equal(a, 1.0 / c.sf)
        np.testing.assert_array_equal(b, 1.0 / (c.sf * c.sf))
        np.testing.assert_array_equal(x1, c.x1)
        np.testing.assert_array_equal(x2, c.x2)
        assert pk[-1] > 0.999999 and (pk[:-1] > 0).all() and (pk[:-1] < 1).all() and np.isfinite(lq[:-1]).all(), c.name


def _oracle_on(orc, mp, c, w):
    """corr_from_cov(*bootstrap_2d(...)) of the oracle on the weights ``w``: its own multinomial draw replaced by them, bins and
    formulas untouched.  The chain is expanded to its cells (for ``huge``, 2^30 cells, the bins are handed over instead: the
    oracle's unique_bins_2d replaced too)."""
    mp.setattr(orc, "multinomial_weights", lambda n_obs, mult, nb: np.asarray(w, dtype=np.int64))
    if c.N > 10 ** 6:
        mp.setattr(orc, "unique_bins_2d", lambda v1, v2, sf, r, r0: (1.0 / c.sf, 1.0 / c.sf ** 2, c.x1, c.x2, c.mult))
        cells = np.broadcast_to(np.zeros(1), (c.N,))                                   # bootstrap_2d takes n from v1.shape[0]
        cov, var1, var2 = orc.bootstrap_2d(cells, cells, cells, c.q, w.shape[1], (c.ra, c.rb), c.r0)
    else:
        v1, v2, sf = np.repeat(c.x1, c.mult), np.repeat(c.x2, c.mult), np.repeat(c.sf, c.mult)
        a, b, e1, e2, mult = orc.unique_bins_2d(v1, v2, sf, (c.ra, c.rb), c.r0)
        np.testing.assert_array_equal(mult, c.mult, err_msg=c.name)
        np.testing.assert_array_equal(e1, c.x1, err_msg=c.name)
        np.testing.assert_array_equal(e2, c.x2, err_msg=c.name)
        cov, var1, var2 = orc.bootstrap_2d(v1, v2, sf, c.q, w.shape[1], (c.ra, c.rb), c.r0)
    return orc.corr_from_cov(cov, var1, var2), var1, var2


def test_ref_corr_2d_is_the_oracles_formulas(orc, refs):
    """Every chain of the menu, B = 150, seed 5: ref_corr_2d equals the oracle on the same weights at the tolerance of
    tests/test_gpu_kernels_2d.py (rtol 1e-9, atol 1e-12); where ref_corr_2d says sentinel the oracle met a variance <= 0 or an
    infinite root and gives exactly 1.0."""
    n_sent = 0
    for name, c in menu2d().items():
        w, r = refs[name, 5]
        with pytest.MonkeyPatch.context() as mp, np.errstate(over="ignore", invalid="ignore"):
            want, var1, var2 = _oracle_on(orc, mp, c, w)
        assert not (r.kind == AMBIGUOUS).any() or name not in SPECIAL
        ok = r.kind != AMBIGUOUS
        np.testing.assert_allclose(r.corr[ok].astype(np.float64), want[ok], rtol=1e-9, atol=1e-12, err_msg=name)
        sent = r.kind == SENT
        assert (want[sent] == 1.0).all(), name
        with np.errstate(over="ignore"):
            assert (((var1 <= 0) | (var2 <= 0) | ~np.isfinite(var1 * var2)) == sent)[ok].all(), name
        n_sent += int(sent.sum())
    assert n_sent > 4 * B


def test_ambiguous_replicates_are_rare(refs):
    """The caps of the kernel tests hold for the reference alone, seeds 5 and 11 at B = 150: over the ordinary chains at most 1 %
    of all replicates are ambiguous, and at most 5 % of any one chain's."""
    for seed in SEEDS:
        amb = {n: int((refs[n, seed][1].kind == AMBIGUOUS).sum()) for n in ordinary_names()}
        print(f"seed {seed}: {sum(amb.values())} ambiguous replicates of {len(amb) * B}; "
              f"{sum(int((refs[n, seed][1].kind == SENT).sum()) for n in amb)} sentinel ones")
        assert sum(amb.values()) <= 0.01 * len(amb) * B, (seed, amb)
        assert max(amb.values()) <= 0.05 * B, (seed, amb)
        for n in ordinary_names():
            r = refs[n, seed][1]
            v = r.kind == VALUE
            assert (r.bound[v] > 0).all() and (r.bound[v] < 1e-7).all() and (r.bound[~v] == 0).all(), n
            assert (np.abs(r.corr[r.kind != AMBIGUOUS]) <= 1).all(), n


def test_special_chains_have_their_designed_outcomes(refs):
    L_ = np.longdouble
    for seed in SEEDS:
        # zero_left: var1 is exactly 0 in every replicate (every term of its sums is 0): the sentinel, exactly 1.0
        r = refs["zero_left", seed][1]
        assert (r.var1 == 0).all() and (r.var2 > 0).all() and (r.kind == SENT).all() and (r.corr == 1).all()
        # same: the left and the right sums are identical, so var1 == var2 exactly; cov carries no (1 - q) term (bootstrap.py:141-155
        # subtracts it from the variances only), so cov = var + (1 - q) E[x / sf^2] > var: the ratio exceeds 1 and is clipped to 1.0
        r = refs["same", seed][1]
        assert (r.var1 == r.var2).all() and (r.cov > r.var1).all() and (r.kind == VALUE).all()
        assert (r.raw > 1 + 1e6 * r.bound).all() and (r.corr == 1).all()
        # anti: x2 = c - x1 at one size factor: below -1 before the clip, exactly -1.0 after it
        r = refs["anti", seed][1]
        assert (r.kind == VALUE).all() and (r.raw < -1 - 1e6 * r.bound).all() and (r.corr == -1).all()
        # overflow: both variances finite and clearly positive in fp64, their product is not: the sentinel, exactly 1.0
        r = refs["overflow", seed][1]
        v1, v2 = r.var1.astype(np.float64), r.var2.astype(np.float64)
        with np.errstate(over="ignore"):
            assert np.isfinite(v1).all() and np.isfinite(v2).all() and (v1 > 0).all() and (v2 > 0).all() and np.isinf(v1 * v2).all()
        assert (r.var1 > 1000 * r.e_v1).all() and (r.var2 > 1000 * r.e_v2).all() and (r.kind == SENT).all() and (r.corr == 1).all()
        # one_bin2d: multinomial gives [N]; var = -(1 - q) x b < 0 (sf = 1: b == a^2 exactly): the sentinel, exactly 1.0, not NaN
        w, r = refs["one_bin2d", seed]
        c = menu2d()["one_bin2d"]
        assert (w == c.N).all() and w.shape == (1, B)
        assert (r.var1 == -L_(1.0 - c.q) * 4).all() and (r.var2 == -L_(1.0 - c.q) * 7).all() and (r.kind == SENT).all()
        assert (r.corr == 1).all() and not np.isnan(r.corr.astype(np.float64)).any()


def test_numpys_draws_still_reach_every_regime():
    """draw_regimes on the 2D menu's multiplicities (they are the 1D menu's): inversion and BTPE draws, both p > 0.5 flips, early
    run-out."""
    m = menu2d()
    reg = {n: draw_regimes(m[n].mult, ref_weights(m[n].mult, B)) for n in MENU_NAMES}
    assert reg["long600"].inversion > 40000 and reg["long600"].btpe > 40000
    assert reg["btpe12"].inversion == 0 and reg["btpe12"].btpe == 11 * B
    assert reg["k3_flip"].flipped > 0 and reg["huge"].flipped > 0
    for n in ("six_ones", "tail_tiny"):
        assert reg[n].early >= 5 and reg[n].last_draw >= 5, (n, vars(reg[n]))
    for b in (1, 64, 65):                                            # the replicates of a shorter run are the first ones of a longer
        np.testing.assert_array_equal(ref_weights(m["k65"].mult, b, 11), ref_weights(m["k65"].mult, B, 11)[:, :b])
    assert (ref_weights(m["k65"].mult, B, 11) != ref_weights(m["k65"].mult, B, 5)).any()


def _tiles(which):
    return {"full": full_tiles_2d, "reduced": lambda: full_tiles_2d(with_long_twin=False, first=False), "twin": twin_tiles_2d,
            "many": many_tiles_2d}[which]()


@pytest.mark.parametrize("which", ["full", "reduced", "twin", "many"])
def test_layout_is_the_designed_one_and_stays_inside_its_buffers(which):
    """Every index a kernel forms from the layout's tables lies inside the buffer it indexes (operand rows of every lane -- an
    unused lane reads its tile's first row or record 0 --, records, output rows), planes and records agree bin by bin, the rows
    are a permutation with 7 spare ones, and the tiles are the designed ones."""
    L = layout2d(_tiles(which))
    n_plane = L.planes.shape[1]
    assert L.planes.shape[0] == 6 and n_plane == L.tile_ptr[-1] * 64 and len(L.recs) == 8 * L.n_rec
    assert np.isfinite(L.planes).all() and np.isfinite(L.recs).all()
    planes, recs = L.planes.reshape(6, -1, 64), L.recs.reshape(-1, 8)
    owner = {e.slot: e for e in L.ents}
    for s in range(L.n_slots):
        t, lane = divmod(s, 64)
        assert L.tile_ptr[t + 1] > L.tile_ptr[t]
        K, row, e = int(L.slot_K[s]), int(L.slot_row[s]), owner.get(s)
        if K > 0 and row >= 0:
            assert e.kind == "run" and K == e.K and row == e.row < L.n_rows and L.tile_ptr[t] + K <= L.tile_ptr[t + 1] and K <= L.kmax
        else:
            assert e is None or e.kind != "run"
        K, row, rec = int(L.rec_K[s]), int(L.rec_row[s]), int(L.slot_rec[s])
        if K > 0 and row >= 0 and rec >= 0:
            assert e.kind == "run" and rec == e.rec and rec + K < L.n_rec and row == e.row
            np.testing.assert_array_equal(recs[rec:rec + K, :6].T, planes[:, L.tile_ptr[t]:L.tile_ptr[t] + K, lane], err_msg=e.label)
            np.testing.assert_array_equal(recs[rec:rec + K], chain_operands_2d(e.chain).recs, err_msg=e.label)
            assert (L.slot_nobs[s], L.slot_omq[s]) == (e.chain.N, 1.0 - e.chain.q)
        else:
            assert e is None or e.kind != "run"
            assert rec < L.n_rec
    rows = [e.row for e in L.ents if e.row >= 0]
    assert len(set(rows)) == len(rows) and L.n_rows == len(rows) + 7 and max(rows) < L.n_rows
    assert all(e.row != e.slot for e in L.ents)
    init = L.out_init(9)
    assert init.shape == (L.n_rows, 13) and (init[:, 0] == 1000.0 + np.arange(L.n_rows)).all() and np.isnan(init[:, 1:]).all()
    # the lanes that must write nothing
    nothing = {e.kind: e for e in L.ents if e.kind != "run"}
    assert sorted(nothing) == ["k0", "norec", "norow"] and len({e.tile for e in nothing.values()}) == 1
    e = nothing["k0"]
    assert (L.slot_K[e.slot], L.rec_K[e.slot]) == (0, 0) and L.slot_row[e.slot] == L.rec_row[e.slot] == e.row >= 0 and L.slot_rec[e.slot] >= 0
    e = nothing["norow"]
    assert (L.slot_K[e.slot], L.rec_K[e.slot]) == (5, 5) and L.slot_row[e.slot] == L.rec_row[e.slot] == -1 and L.slot_rec[e.slot] >= 0
    e = nothing["norec"]
    assert L.slot_rec[e.slot] == -1 and L.rec_K[e.slot] == e.chain.K >= 2 and L.rec_row[e.slot] == e.row >= 0
    assert (L.slot_K[e.slot], L.slot_row[e.slot]) == (0, -1)                             # a plain empty lane in the planes tables
    per_tile = [sum(1 for e in L.ents if e.tile == t and e.kind == "run") for t in range(L.n_tiles)]
    if which == "full":
        assert per_tile == [64, 5, 4, 1, 0]
        assert [e.chain.name for e in L.ents if (e.tile, e.lane) == (1, 63)] == ["long600"]
        assert {e.chain.name for e in L.ents if e.kind == "run"} == set(menu2d())
    elif which == "reduced":
        assert per_tile == [4, 4, 1, 0] and "long600" not in {e.chain.name for e in L.ents if e.kind == "run"}
    elif which == "twin":
        full = layout2d(_tiles("full"))
        assert per_tile == [0, 1, 64, 4, 5]
        at = lambda X: sorted((e.chain.name, ) for e in X.ents if e.kind == "run")
        assert at(L) == at(full)
        where = {(e.chain.name, e.tile, e.lane) for e in full.ents if e.kind == "run"}
        assert not any((e.chain.name, e.tile, e.lane) in where for e in L.ents if e.kind == "run")
        company = lambda X, n: {frozenset(o.chain.name for o in X.ents if o.tile == e.tile and o.kind == "run") for e in X.ents
                                if e.kind == "run" and e.chain.name == n}
        assert all(company(L, n) != company(full, n) for n in SPECIAL if n != "same")
    else:
        assert L.n_tiles == 2049 > 2048 and per_tile[:5] == [64, 5, 4, 1, 0] and set(per_tile[5:]) == {1}
