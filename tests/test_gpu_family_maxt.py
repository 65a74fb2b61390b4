"""mm_family_maxt (the max-T adjustment over families of design contrasts) on synthetic replicate planes through
``engine.Bootstrap1D.family_maxt``, against the numpy restatement tests/_family_ref.py, at the smallest sizes where the kernel
changes path: one member, fewer members than a count block, more than one, more members than are staged in LDS, two- and
six-entry designs, fewer replicate columns than threads, a ragged second stride, padded rows, several families and an empty one in
one launch, dropped columns, members without a test, a dropped column 0, no family at all.

The scale every case hands the kernel is ``engine.family_scale`` of the records of ``contrast_design`` on the same planes (1 / se,
equal to the restatement's own to rtol 1e-11); the restatement is given the same doubles, so the maximum row and t0 are compared
bit for bit (the library is built with contraction off and numpy rounds every operation the same way), which is within the rtol
1e-13 asked of them.  The counts are exact: every case first asserts in numpy that no M[c] lies within 1e-10 (relative) of a t0, so
the restatement alone decides every count."""

import numpy as np
import pytest

import _family_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


def _planes(eng, ym, yv, B, ng):
    """A Bootstrap1D that only holds replicate rows (what the statistics kernels read)."""
    bs = object.__new__(eng.Bootstrap1D)
    bs.ym, bs.yv, bs.ld, bs.B, bs.ng = eng.dev(ym), eng.dev(yv), ym.shape[1], B, ng
    bs.n_tested = bs.n_pairs = ym.shape[0] // ng
    return bs


def _random_planes(n_genes, ng, B, pad, seed):
    """Normal planes [n_genes * ng][B + 1 + pad]; the padding is poisoned (NaN and 1e300 alternating): it is never read."""
    rng = np.random.default_rng(seed)
    ld = B + 1 + pad
    ym = rng.normal(0, 1, size=(n_genes * ng, ld))
    yv = rng.normal(0, 1, size=(n_genes * ng, ld))
    for y in (ym, yv):
        y[:, B + 1::2] = np.nan
        y[:, B + 2::2] = 1e300
    return ym, yv


def _pairs(n_levels):
    return [([a, b], [1.0, -1.0]) for a, b in ref.pairwise(n_levels)]


def _tables(families):
    """``families``: [(gene, [(groups, weights)])] -> (family_ptr, test_gene, test_design, design_ptr, design_grp, design_w), one
    design per member."""
    family_ptr, test_gene, ptr, grp, w = [0], [], [0], [], []
    for gene, designs in families:
        for g, ww in designs:
            test_gene.append(gene)
            grp.extend(g)
            w.extend(ww)
            ptr.append(len(grp))
        family_ptr.append(len(test_gene))
    return (np.asarray(family_ptr), np.asarray(test_gene, dtype=np.int32), np.arange(len(test_gene), dtype=np.int32),
            np.asarray(ptr, dtype=np.int32), np.asarray(grp, dtype=np.int32), np.asarray(w, dtype=np.float64))


def _check(eng, ym, yv, B, ng, families, stage_cap=None, edit_scale=None):
    """Every output of every family against the restatement; returns (maxrow host [n_fam][2][ld], adj, fam, scale)."""
    bs = _planes(eng, ym, yv, B, ng)
    tab = _tables(families)
    st_m, st_v, _ = bs.contrast_design(*tab[1:])
    scale = eng.family_scale(st_m, st_v)
    if edit_scale is not None:
        edit_scale(scale)
    maxrow, adj, fam = bs.family_maxt(*tab, scale, stage_cap=stage_cap)
    maxrow = eng.host(maxrow)
    assert maxrow.shape == (len(families), 2, ym.shape[1]) and adj.shape == (len(tab[1]), 2, 2) and fam.shape == (len(families), 2, 2)
    for f, (gene, designs) in enumerate(families):
        t0, t1 = tab[0][f], tab[0][f + 1]
        rows = slice(gene * ng, (gene + 1) * ng)
        own = ref.family(ym[rows, :B + 1], yv[rows, :B + 1], designs)
        if edit_scale is None:
            np.testing.assert_allclose(scale[t0:t1], own["scale"], rtol=1e-11, err_msg=f"family {f}: scale")
        want = ref.family(ym[rows, :B + 1], yv[rows, :B + 1], designs, scale[t0:t1])
        assert ref.near_ties(want) == 0, f"family {f}: an M[c] within 1e-10 of a t0, pick another seed"
        np.testing.assert_array_equal(maxrow[f][:, :B + 1], want["maxrow"], err_msg=f"family {f}: maxrow")
        np.testing.assert_array_equal(adj[t0:t1, :, 0], want["t0"], err_msg=f"family {f}: t0")
        np.testing.assert_array_equal(adj[t0:t1, :, 1], want["n_adj"], err_msg=f"family {f}: n_adj")
        np.testing.assert_array_equal(fam[f, :, 0], want["n_valid"], err_msg=f"family {f}: n_valid")
        np.testing.assert_array_equal(fam[f, :, 1], want["n_included"], err_msg=f"family {f}: n_included")
    return maxrow, adj, fam, scale


@pytest.mark.parametrize("n_levels, m", [(2, 1), (3, 3), (5, 10)])
def test_one_three_and_ten_members(eng, n_levels, m):
    B, ng = 300, 5
    ym, yv = _random_planes(1, ng, B, 5, seed=10 + m)
    designs = _pairs(n_levels)
    assert len(designs) == m
    _, adj, fam, _ = _check(eng, ym, yv, B, ng, [(0, designs)])
    assert fam.tolist() == [[[B, m], [B, m]]]
    assert (adj[:, :, 1] > 0).all() and (adj[:, :, 1] < B).any()      # counts in the middle: the comparison matters
    if m == 1:                                                       # a family of one: the count of the member's own record
        bs = _planes(eng, ym, yv, B, ng)
        st_m, st_v, _ = bs.contrast_design(*_tables([(0, designs)])[1:])
        assert adj[0, 0, 1] == st_m[0, 3] and adj[0, 1, 1] == st_v[0, 3]


def test_either_side_of_the_staging_boundary(eng):
    """10 members: all staged (the default and stage_cap = 10), four of them, none -- the same bits every time, and against the
    restatement every time."""
    B, ng = 300, 5
    ym, yv = _random_planes(2, ng, B, 2, seed=31)
    yv[ng + 2, 17] = np.nan
    families = [(1, _pairs(5)), (0, _pairs(4))]
    outs = [_check(eng, ym, yv, B, ng, families, stage_cap=cap) for cap in (None, 10, 9, 4, 1, 0)]
    for other in outs[1:]:
        for a, b in zip(outs[0][:3], other[:3]):
            np.testing.assert_array_equal(a[..., :B + 1] if a.shape[-1] > B else a, b[..., :B + 1] if b.shape[-1] > B else b)
    assert outs[0][2][0].tolist() == [[B - 1, 10], [B - 1, 10]]


def test_more_members_than_a_wave_pass_counts(eng):
    """45 members (10 levels pairwise): more than the 32 members the four waves count in one pass, with a last block that is not full."""
    B, ng = 257, 10
    ym, yv = _random_planes(1, ng, B, 1, seed=41)
    _, adj, fam, _ = _check(eng, ym, yv, B, ng, [(0, _pairs(10))], stage_cap=40)
    assert fam[0, 0].tolist() == [B, 45]


def test_six_entry_designs_with_weights(eng):
    B, ng = 300, 8
    rng = np.random.default_rng(51)
    ym, yv = _random_planes(2, ng, B, 3, seed=52)
    designs = [(sorted(rng.choice(ng, size=6, replace=False).tolist()), rng.normal(0, 1, size=6).tolist()) for _ in range(4)]
    designs.insert(2, ([7, 1], [1.0, -1.0]))
    designs.append(([3], [0.37]))
    _check(eng, ym, yv, B, ng, [(1, designs), (0, designs[::-1])])


@pytest.mark.parametrize("B", [1, 255, 256, 300])
def test_replicate_counts_around_the_block_size(eng, B):
    ng = 4
    ym, yv = _random_planes(1, ng, B, 3, seed=60 + B)
    _, _, fam, _ = _check(eng, ym, yv, B, ng, [(0, _pairs(4))])
    # one replicate: its deviation about its own mean is 0, se = 0, so no member has a test: nothing is included
    assert fam[0].tolist() == ([[0, 0], [0, 0]] if B == 1 else [[B, 6], [B, 6]])


def test_several_families_of_different_sizes_and_an_empty_one(eng):
    B, ng = 300, 5
    ym, yv = _random_planes(4, ng, B, 1, seed=71)
    families = [(2, _pairs(2)), (0, _pairs(5)), (3, []), (1, _pairs(3)), (3, _pairs(4))]
    maxrow, adj, fam, _ = _check(eng, ym, yv, B, ng, families)
    assert fam[:, 0, 1].tolist() == [1, 10, 0, 3, 6] and fam[2].tolist() == [[0, 0], [0, 0]]
    assert np.isnan(maxrow[2][:, :B + 1]).all()


def test_a_bad_entry_drops_the_column_for_the_whole_family(eng):
    B, ng = 300, 5
    ym, yv = _random_planes(1, ng, B, 2, seed=81)
    ym[1, 40], yv[3, 41], ym[4, 300] = np.nan, np.inf, -np.inf
    maxrow, adj, fam, _ = _check(eng, ym, yv, B, ng, [(0, _pairs(5))])
    assert fam[0].tolist() == [[B - 3, 10], [B - 3, 10]]
    assert np.isnan(maxrow[0][:, [0, 40, 41, 300]]).all() and np.isfinite(maxrow[0][:, 1:40]).all()
    # without the members of group 4 its bad column stays: the family is valid where its OWN members are
    maxrow, _, fam, _ = _check(eng, ym, yv, B, ng, [(0, _pairs(4))])
    assert fam[0].tolist() == [[B - 2, 6], [B - 2, 6]] and np.isfinite(maxrow[0][:, 300]).all()


def test_members_without_a_test(eng):
    """Between included members: an empty design, a member whose replicates all equal column 0 on the variability plane only, a
    member switched off by hand; the dropped column of the switched-off member's group comes back."""
    B, ng = 300, 6
    ym, yv = _random_planes(1, ng, B, 2, seed=91)
    yv[4, :B + 1] = yv[4, 0]
    ym[5, 77] = np.nan
    designs = [([1, 0], [1.0, -1.0]), ([], []), ([2, 0], [1.0, -1.0]), ([4], [1.0]), ([5, 0], [1.0, -1.0]), ([2, 1], [1.0, -1.0])]

    def off(scale):
        assert (scale[[0, 2, 4, 5]] > 0).all() and scale[1].tolist() == [0, 0] and scale[3, 0] > 0 and scale[3, 1] == 0
        scale[4] = 0

    maxrow, adj, fam, _ = _check(eng, ym, yv, B, ng, [(0, designs)], edit_scale=off)
    assert fam[0].tolist() == [[B, 4], [B, 3]]
    assert np.isnan(adj[[1, 4], :, 0]).all() and (adj[[1, 4], :, 1] == 0).all() and np.isnan(adj[3, 1, 0]) and adj[3, 0, 0] > 0
    _, _, fam, _ = _check(eng, ym, yv, B, ng, [(0, designs)])
    assert fam[0].tolist() == [[B - 1, 5], [B - 1, 4]]


def test_a_family_without_an_included_member(eng):
    B, ng = 300, 3
    ym, yv = _random_planes(2, ng, B, 2, seed=101)

    def all_off(scale):
        scale[:3] = 0

    maxrow, adj, fam, _ = _check(eng, ym, yv, B, ng, [(0, _pairs(3)), (1, _pairs(3))], edit_scale=all_off)
    assert fam[0].tolist() == [[0, 0], [0, 0]] and fam[1].tolist() == [[B, 3], [B, 3]]
    assert np.isnan(maxrow[0][:, :B + 1]).all() and np.isnan(adj[:3, :, 0]).all() and (adj[:3, :, 1] == 0).all()


def test_a_dropped_column_zero(eng):
    """Column 0 of group 2 is not finite: its members have the NaN coefficient, scale 0, and the others go on without them -- also
    when a scale is forced on such a member by hand."""
    B, ng = 300, 4
    ym, yv = _random_planes(1, ng, B, 2, seed=111)
    yv[2, 0] = np.nan
    designs = _pairs(4)
    with_2 = [j for j, (g, _) in enumerate(designs) if 2 in g]
    _, adj, fam, scale = _check(eng, ym, yv, B, ng, [(0, designs)])
    assert (scale[with_2] == 0).all() and fam[0].tolist() == [[B, 3], [B, 3]] and np.isnan(adj[with_2, :, 0]).all()

    def force(scale):
        scale[with_2] = 1.5

    _, adj2, fam2, _ = _check(eng, ym, yv, B, ng, [(0, designs)], edit_scale=force)
    np.testing.assert_array_equal(adj2, adj)
    np.testing.assert_array_equal(fam2, fam)


def test_no_family(eng):
    B, ng = 300, 3
    ym, yv = _random_planes(1, ng, B, 0, seed=121)
    bs = _planes(eng, ym, yv, B, ng)
    empty_i, empty_f = np.zeros(0, np.int32), np.zeros(0)
    maxrow, adj, fam = bs.family_maxt([0], empty_i, empty_i, [0], empty_i, empty_f, np.zeros((0, 2)))
    assert tuple(maxrow.shape) == (0, 2, B + 1) and adj.shape == (0, 2, 2) and fam.shape == (0, 2, 2)


def test_malformed_tables_raise_before_any_launch(eng):
    B, ng = 300, 3
    ym, yv = _random_planes(2, ng, B, 0, seed=131)
    bs = _planes(eng, ym, yv, B, ng)
    ok = dict(family_ptr=[0, 2, 3], test_gene=[0, 0, 1], test_design=[0, 1, 0], design_ptr=[0, 2, 4], design_grp=[0, 1, 2, 1],
              design_w=[1.0, -1.0, 1.0, -1.0], scale=np.ones((3, 2)))
    bs.family_maxt(**ok)
    for field, value in (("family_ptr", [0, 2]), ("family_ptr", [1, 2, 3]), ("family_ptr", [0, 3, 2, 3]), ("family_ptr", [0, 1, 3]),
                         ("scale", np.ones((2, 2))), ("test_gene", [0, 0, 2]), ("test_design", [0, 2, 0]), ("design_grp", [0, 1, 3, 1]),
                         ("design_ptr", [0, 2, 5]), ("design_w", [1.0, -1.0, 1.0]), ("stage_cap", -1), ("stage_cap", 1025)):
        with pytest.raises(ValueError, match="family_maxt:"):
            bs.family_maxt(**{**ok, field: value})


def test_cells_outside_the_written_region_keep_their_sentinel(eng):
    """Through the C-ABI on sentinel-filled buffers: the kernel writes columns 0..B of the rows of its families, the adj cells of
    its tests and the fam cells of its families -- not the padding of a row, not the rows and cells beyond."""
    import torch

    B, ng, pad = 300, 5, 6
    ym, yv = _random_planes(3, ng, B, pad, seed=141)
    families = [(0, _pairs(5)), (2, []), (1, _pairs(3))]
    bs = _planes(eng, ym, yv, B, ng)
    tab = _tables(families)
    st_m, st_v, _ = bs.contrast_design(*tab[1:])
    scale = eng.family_scale(st_m, st_v)
    want = bs.family_maxt(*tab, scale)
    n_fam, n_tests, ld, S = len(families), len(tab[1]), bs.ld, -12345.5
    maxrow = torch.full((n_fam + 1, 2, ld), S, dtype=torch.float64, device="cuda")
    adj = torch.full((n_tests + 3, 2, 2), S, dtype=torch.float64, device="cuda")
    fam = torch.full((n_fam + 2, 2, 2), S, dtype=torch.float64, device="cuda")
    d = [eng.dev(np.asarray(a, dtype=np.int32)) for a in tab[:5]] + [eng.dev(tab[5]), eng.dev(scale.reshape(-1))]
    eng._lib.call("mm_family_maxt", eng.P(bs.ym), eng.P(bs.yv), ld, B, ng, *map(eng.P, d), 4, n_fam, eng.P(maxrow), eng.P(adj), eng.P(fam),
                  eng._stream())
    maxrow, adj, fam = eng.host(maxrow), eng.host(adj), eng.host(fam)
    np.testing.assert_array_equal(maxrow[:n_fam, :, :B + 1], eng.host(want[0])[:, :, :B + 1])
    np.testing.assert_array_equal(adj[:n_tests], want[1])
    np.testing.assert_array_equal(fam[:n_fam], want[2])
    assert (maxrow[:n_fam, :, B + 1:] == S).all() and (maxrow[n_fam:] == S).all() and (adj[n_tests:] == S).all() and (fam[n_fam:] == S).all()
