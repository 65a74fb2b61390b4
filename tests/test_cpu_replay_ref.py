"""The numpy restatement of the strict 1D replay bootstrap (tests/_replay_ref.py) checked on its own (no GPU): its operands
against tests/_bins_ref.py, its weights against their own invariants, and the chain menu against the sampler regimes it was
chosen for -- so that the problem tests/test_gpu_replay_kernels.py runs cannot drift -- and the index arithmetic of the slot
layout against the bounds of the buffers the kernels are given."""

import numpy as np
import pytest

from _bins_ref import ref_order, ulp_diff
from _replay_ref import (MENU_NAMES, SF8, XCAP, chain_operands, draw_regimes, full_tiles, layout, menu, ref_moments, ref_weights)

B = 150


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def weights():
    return {name: ref_weights(menu()[name].mult, B) for name in MENU_NAMES}


def test_menu_is_the_designed_one():
    m = menu()
    assert m["k2"].mult.tolist() == [3, 2] and m["k3_flip"].mult.tolist() == [950, 30, 20] and m["six_ones"].mult.tolist() == [1] * 6
    assert (m["k64"].K, m["k65"].K) == (64, 65)
    for n in ("k64", "k65"):
        assert m[n].mult.min() >= 1 and m[n].mult.max() <= 39
    lg = m["long600"].mult
    assert len(lg) == 600 and lg[0] == 14000 and lg[1:].min() >= 1 and lg[1:].max() <= 59
    assert m["btpe12"].K == 12 and m["btpe12"].mult.min() >= 1500 and m["btpe12"].mult.max() <= 2499
    assert m["huge"].mult.tolist() == [2 ** 29, 2 ** 29 - 7, 7] and m["huge"].N == 2 ** 30 < 2 ** 31
    assert m["tail_tiny"].mult.tolist() == [5000, 3000] + [1] * 30
    fillers = [c for n, c in m.items() if n.startswith("f")]
    assert len(fillers) == 54 and {c.K for c in fillers} <= set(range(2, 41)) and len({c.K for c in fillers}) > 30
    assert len({c.q for c in m.values()}) == 2
    for c in m.values():
        assert (c.x == 0).sum() == 1 and c.x.max() < XCAP, c.name                      # a zero-count bin in every chain
        assert len(set(zip(c.sf_bin.tolist(), c.x.tolist()))) == c.K, c.name


def test_operands_equal_ref_order_on_a_table_of_the_same_bins():
    """Every chain of the menu as a [size-factor bin][count] table: ref_order leaves the bins in the chain's order, and its pk,
    1/sf and 1/sf^2 are chain_operands' bit for bit, lq within 0 ulp."""
    for c in menu().values():
        t = np.zeros((len(SF8), XCAP), dtype=np.uint32)
        t[c.sf_bin, c.x] = c.mult
        bi, xi, mult, pk, lq, a, b = ref_order(t, SF8, c.r1, c.r0, c.N)
        np.testing.assert_array_equal(bi, c.sf_bin, err_msg=c.name)
        np.testing.assert_array_equal(xi, c.x, err_msg=c.name)
        np.testing.assert_array_equal(mult, c.mult, err_msg=c.name)
        g_pk, g_lq, g_v, g_a, g_b = chain_operands(c.mult, c.v, c.sf)
        for got, want, what in ((g_pk, pk, "pk"), (g_a, a, "1/sf"), (g_b, b, "1/sf^2"), (g_v, xi.astype(np.float64), "count")):
            np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"{c.name}: {what}")
        assert ulp_diff(g_lq, lq).max() == 0, c.name
        assert g_pk[-1] > 0.999999 and (g_pk[:-1] > 0).all() and (g_pk[:-1] < 1).all(), c.name


def test_weights_sum_to_n_and_replicates_are_a_prefix(weights):
    for name, w in weights.items():
        c = menu()[name]
        assert w.shape == (c.K, B) and w.min() >= 0, name
        np.testing.assert_array_equal(w.sum(axis=0), np.full(B, c.N), err_msg=name)
    for b in (1, 64, 65):                                            # the replicates of a shorter run are the first ones of a longer
        np.testing.assert_array_equal(ref_weights(menu()["k65"].mult, b), weights["k65"][:, :b])
    assert (ref_weights(menu()["k65"].mult, B, seed=12345) != weights["k65"]).any()


def test_numpys_draws_reach_every_regime(weights):
    """Inversion and BTPE draws on either side of n min(p, 1 - p) = 30, draws with pk > 0.5, and replicates that run out of cells
    before the last bin (with draws still to make, or exactly at the last draw): counted over numpy's own weights."""
    reg = {name: draw_regimes(menu()[name].mult, w) for name, w in weights.items()}
    print({n: vars(r) for n, r in reg.items()})
    assert sum(r.inversion for r in reg.values()) > 0 and sum(r.btpe for r in reg.values()) > 0
    assert reg["long600"].inversion > 40000 and reg["long600"].btpe > 40000
    assert reg["btpe12"].inversion == 0 and reg["btpe12"].btpe == 11 * B
    assert reg["k3_flip"].flipped > 0 and reg["huge"].flipped > 0
    assert sum(r.flipped for r in reg.values()) > 0
    for name in ("six_ones", "tail_tiny"):
        assert reg[name].early >= 5 and reg[name].last_draw >= 5, (name, vars(reg[name]))
        w = weights[name]
        assert (w[-1] == 0).sum() == reg[name].early + reg[name].last_draw


def test_longdouble_is_wider_than_fp64_and_the_bounds_are_sane(weights):
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    c = menu()["k65"]
    pk, lq, v, a, b = chain_operands(c.mult, c.v, c.sf)
    m1, var, b1, bv = ref_moments(v, a, b, weights["k65"], c.N, c.q)
    e, w = v[:, None], weights["k65"].astype(np.float64)
    np.testing.assert_allclose((e * w * a[:, None]).sum(axis=0) / c.N, m1.astype(np.float64), rtol=1e-13)
    assert (b1 > 0).all() and (b1 < 1e-13 * m1).all() and (bv > 0).all()
    mo, vo, bo, bvo = ref_moments(v, a, b, weights["k65"], c.N, c.q, mean_only=True)
    assert (mo == m1 + 1).all() and (vo == 10).all() and (bo == b1).all() and (bvo == 0).all()


@pytest.mark.parametrize("which", ["full", "reduced", "flagged"])
def test_layout_stays_inside_its_buffers(which):
    """Every index a kernel forms from the layout's tables lies inside the buffer it indexes: operand rows of every lane (unused
    lanes read their tile's first row), records, output rows, weight cells."""
    tiles = {"full": full_tiles(), "reduced": full_tiles(with_long_twin=False, first=False),
             "flagged": [full_tiles()[1], "long600"] + full_tiles()[2:4] + ["six_ones", full_tiles()[4]]}[which]
    L = layout(tiles)
    n_plane = L.planes.shape[1]
    assert n_plane % 64 == 0 and L.tile_ptr[-1] * 64 <= n_plane and len(L.recs) == 8 * L.n_rec
    active = 0
    for t in range(L.n_tiles):
        if L.tile_chain[t] >= 0:
            assert L.tile_ptr[t + 1] == L.tile_ptr[t] and (L.slot_K[t * 64:(t + 1) * 64] == 0).all()
            continue
        assert L.tile_ptr[t] * 64 + 63 < n_plane
        for lane in range(64):
            s = t * 64 + lane
            K, row = int(L.slot_K[s]), int(L.slot_row[s])
            if K > 0 and row >= 0:
                assert (L.tile_ptr[t] + K) * 64 <= n_plane and L.tile_ptr[t] + K <= L.tile_ptr[t + 1] and row < L.n_rows and K <= L.kmax
                active += K >= 2
            K, row, rec = int(L.free_K[s]), int(L.free_row[s]), int(L.slot_rec[s])
            if K > 0 and row >= 0 and rec >= 0:
                assert rec + K <= L.n_rec and row < L.n_rows and K <= L.kmax
            K = int(L.as_K[s])
            assert 0 <= L.as_base[s] and L.as_base[s] + max(K, 2) <= L.n_rec
            if K >= 2:
                assert 0 <= L.as_row[s] < L.n_rows
    assert (L.ch_K >= 2).all() and (L.ch_base >= 0).all() and (L.ch_base + L.ch_K <= L.n_rec).all()
    assert (L.ch_row >= 0).all() and (L.ch_row < L.n_rows).all() and L.ch_K.max() <= L.kmax
    rows = [e.row for e in L.ents if e.row >= 0]
    assert len(set(rows)) == len(rows) and L.n_rows == len(rows) + 7
    assert all(e.row != e.slot for e in L.ents)
    if which == "full":
        per_tile = [sum(1 for e in L.ents if e.tile == t and e.kind == "run") for t in range(5)]
        assert per_tile == [64, 5, 4, 1, 0] and active == 74 and L.n_chains == 74
        assert {e.kind for e in L.ents if e.tile == 4} == {"k0", "norow", "norec", "k1"}
        assert [e.chain.name for e in L.ents if e.tile == 1 and e.lane == 63] == ["long600"]
