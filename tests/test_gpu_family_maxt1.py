"""mm_family_maxt1 (the max-T adjustment over families of design contrasts on ONE response plane) on a synthetic replicate plane
through ``engine.Bootstrap2D.family_maxt``, against the numpy restatement tests/_family_ref.py given the plane twice (plane 0 of its
answer: with both planes equal its validity rule -- every listed group finite in both -- is the one-plane rule), at the smallest sizes
where the kernel changes path: one member, fewer members than a count block of 8, more than one block, none / all but one / all of
the members staged in LDS, two- and six-entry designs, fewer replicate columns than the 256 threads, column counts that are no
multiple of 64, padded rows, three families and an empty one in one launch, dropped columns, a member with scale 0, a dropped
column 0, no family at all, malformed tables.

As in tests/test_gpu_family_maxt.py the scale every case hands the kernel is ``engine.family_scale`` of the records of
``contrast_design`` on the same plane and the restatement is given the same doubles, so the maximum row and t0 are compared bit
for bit; the counts are exact: every case first asserts in numpy that no M[c] lies within 1e-10 (relative) of a t0 (the seeds
were chosen on the CPU so that this holds: a condition, not a tolerance).  The last tests pin the one-plane kernel to the tested
two-plane one: given the plane twice, plane 0 of ``Bootstrap1D.family_maxt`` is ``Bootstrap2D.family_maxt`` bit for bit."""

import numpy as np
import pytest

import _family_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from scrna_parameter_estimation_amd import engine

    engine._lib.load(require_gpu=True)
    return engine


def _shell(eng, y, B, ng):
    """A Bootstrap2D that only holds replicate correlation rows (what the statistics kernels read)."""
    bs = object.__new__(eng.Bootstrap2D)
    bs.yc, bs.ld, bs.B, bs.ng = eng.dev(y), y.shape[1], B, ng
    bs.n_pairs = y.shape[0] // ng
    return bs


def _shell_1d(eng, y, B, ng):
    """The same plane as both planes of a Bootstrap1D."""
    bs = object.__new__(eng.Bootstrap1D)
    bs.ym, bs.yv, bs.ld, bs.B, bs.ng = eng.dev(y), eng.dev(y), y.shape[1], B, ng
    bs.n_tested = bs.n_pairs = y.shape[0] // ng
    return bs


def _random_plane(n_pairs, ng, B, pad, seed):
    """A normal plane [n_pairs * ng][B + 1 + pad]; the padding is poisoned (NaN and 1e300 alternating): it is never read."""
    rng = np.random.default_rng(seed)
    y = rng.normal(0, 1, size=(n_pairs * ng, B + 1 + pad))
    y[:, B + 1::2] = np.nan
    y[:, B + 2::2] = 1e300
    return y


def _pairs(n_levels):
    return [([a, b], [1.0, -1.0]) for a, b in ref.pairwise(n_levels)]


def _tables(families):
    """``families``: [(pair, [(groups, weights)])] -> (family_ptr, test_pair, test_design, design_ptr, design_grp, design_w), one
    design per member."""
    family_ptr, test_pair, ptr, grp, w = [0], [], [0], [], []
    for pair, designs in families:
        for g, ww in designs:
            test_pair.append(pair)
            grp.extend(g)
            w.extend(ww)
            ptr.append(len(grp))
        family_ptr.append(len(test_pair))
    return (np.asarray(family_ptr), np.asarray(test_pair, dtype=np.int32), np.arange(len(test_pair), dtype=np.int32),
            np.asarray(ptr, dtype=np.int32), np.asarray(grp, dtype=np.int32), np.asarray(w, dtype=np.float64))


def _want(y, B, ng, pair, designs, scale=None):
    """The restatement on the plane given twice: its plane 0."""
    rows = slice(pair * ng, (pair + 1) * ng)
    return ref.family(y[rows, :B + 1], y[rows, :B + 1], designs, None if scale is None else np.column_stack([scale, scale]))


def _check(eng, y, B, ng, families, stage_cap=None, edit_scale=None):
    """Every output of every family against the restatement; returns (maxrow host [n_fam][1][ld], adj, fam, scale)."""
    bs = _shell(eng, y, B, ng)
    tab = _tables(families)
    stt, _ = bs.contrast_design(*tab[1:])
    scale = eng.family_scale(stt)
    assert scale.shape == (len(tab[1]), 1)
    if edit_scale is not None:
        edit_scale(scale)
    maxrow, adj, fam = bs.family_maxt(*tab, scale, stage_cap=stage_cap)
    maxrow = eng.host(maxrow)
    assert maxrow.shape == (len(families), 1, y.shape[1]) and adj.shape == (len(tab[1]), 1, 2) and fam.shape == (len(families), 1, 2)
    for f, (pair, designs) in enumerate(families):
        t0, t1 = tab[0][f], tab[0][f + 1]
        if edit_scale is None:
            np.testing.assert_allclose(scale[t0:t1, 0], _want(y, B, ng, pair, designs)["scale"][:, 0], rtol=1e-11, err_msg=f"family {f}: scale")
        want = _want(y, B, ng, pair, designs, scale[t0:t1, 0])
        assert ref.near_ties(want) == 0, f"family {f}: an M[c] within 1e-10 of a t0, pick another seed"
        np.testing.assert_array_equal(maxrow[f, 0, :B + 1], want["maxrow"][0], err_msg=f"family {f}: maxrow")
        np.testing.assert_array_equal(adj[t0:t1, 0, 0], want["t0"][:, 0], err_msg=f"family {f}: t0")
        np.testing.assert_array_equal(adj[t0:t1, 0, 1], want["n_adj"][:, 0], err_msg=f"family {f}: n_adj")
        assert fam[f, 0, 0] == want["n_valid"][0] and fam[f, 0, 1] == want["n_included"][0], f"family {f}: counts"
    return maxrow, adj, fam, scale


@pytest.mark.parametrize("n_levels, m", [(2, 1), (3, 3), (5, 10)])
def test_one_three_and_ten_members(eng, n_levels, m):
    B, ng = 300, 5
    y = _random_plane(1, ng, B, 5, seed=210 + m)
    designs = _pairs(n_levels)
    assert len(designs) == m
    _, adj, fam, _ = _check(eng, y, B, ng, [(0, designs)])
    assert fam.tolist() == [[[B, m]]]
    assert (adj[:, 0, 1] > 0).all() and (adj[:, 0, 1] < B).any()      # counts in the middle: the comparison matters
    if m == 1:                                                       # a family of one: the count of the member's own record
        stt, _ = _shell(eng, y, B, ng).contrast_design(*_tables([(0, designs)])[1:])
        assert adj[0, 0, 1] == stt[0, 3]


def test_either_side_of_the_staging_boundary(eng):
    """10 members: all staged (the default and stage_cap = 10), all but one, none -- the same bits every time, and against the
    restatement every time."""
    B, ng = 300, 5
    y = _random_plane(2, ng, B, 2, seed=231)
    y[ng + 2, 17] = np.nan
    families = [(1, _pairs(5)), (0, _pairs(4))]
    outs = [_check(eng, y, B, ng, families, stage_cap=cap) for cap in (None, 10, 9, 0)]
    for other in outs[1:]:
        np.testing.assert_array_equal(outs[0][0][..., :B + 1], other[0][..., :B + 1])
        np.testing.assert_array_equal(outs[0][1], other[1])
        np.testing.assert_array_equal(outs[0][2], other[2])
    assert outs[0][2].tolist() == [[[B - 1, 10]], [[B, 6]]]


def test_six_entry_designs_with_weights(eng):
    B, ng = 300, 8
    rng = np.random.default_rng(251)
    y = _random_plane(2, ng, B, 3, seed=252)
    designs = [(sorted(rng.choice(ng, size=6, replace=False).tolist()), rng.normal(0, 1, size=6).tolist()) for _ in range(4)]
    designs.insert(2, ([7, 1], [1.0, -1.0]))
    designs.append(([3], [0.37]))
    _check(eng, y, B, ng, [(1, designs), (0, designs[::-1])])


@pytest.mark.parametrize("B", [1, 100, 255, 256, 300])
def test_replicate_counts_around_the_block_size(eng, B):
    ng = 4
    y = _random_plane(1, ng, B, 3, seed=260 + B)
    _, _, fam, _ = _check(eng, y, B, ng, [(0, _pairs(4))])
    # one replicate: its deviation about its own mean is 0, se = 0, so no member has a test: nothing is included
    assert fam[0].tolist() == ([[0, 0]] if B == 1 else [[B, 6]])


def test_three_families_and_an_empty_one(eng):
    B, ng = 300, 5
    y = _random_plane(4, ng, B, 1, seed=271)
    families = [(2, _pairs(2)), (0, _pairs(5)), (3, []), (1, _pairs(3))]
    maxrow, adj, fam, _ = _check(eng, y, B, ng, families)
    assert fam[:, 0, 1].tolist() == [1, 10, 0, 3] and fam[2].tolist() == [[0, 0]]
    assert np.isnan(maxrow[2][:, :B + 1]).all()


def test_a_bad_entry_drops_the_column_for_the_whole_family(eng):
    B, ng = 300, 5
    y = _random_plane(1, ng, B, 2, seed=281)
    y[1, 40], y[3, 41], y[4, 300] = np.nan, np.inf, -np.inf
    maxrow, adj, fam, _ = _check(eng, y, B, ng, [(0, _pairs(5))])
    assert fam[0].tolist() == [[B - 3, 10]]
    assert np.isnan(maxrow[0][0, [0, 40, 41, 300]]).all() and np.isfinite(maxrow[0][0, 1:40]).all()
    # without the members of group 4 its bad column stays: the family is valid where its OWN members are
    maxrow, _, fam, _ = _check(eng, y, B, ng, [(0, _pairs(4))])
    assert fam[0].tolist() == [[B - 2, 6]] and np.isfinite(maxrow[0][0, 300])


def test_members_without_a_test(eng):
    """Between included members: an empty design, a member whose replicates all equal column 0, a member switched off by hand (scale
    0); the dropped column of the switched-off member's group comes back."""
    B, ng = 300, 6
    y = _random_plane(1, ng, B, 2, seed=291)
    y[4, :B + 1] = y[4, 0]
    y[5, 77] = np.nan
    designs = [([1, 0], [1.0, -1.0]), ([], []), ([2, 0], [1.0, -1.0]), ([4], [1.0]), ([5, 0], [1.0, -1.0]), ([2, 1], [1.0, -1.0])]

    def off(scale):
        assert (scale[[0, 2, 4, 5], 0] > 0).all() and scale[[1, 3], 0].tolist() == [0, 0]
        scale[4] = 0

    maxrow, adj, fam, _ = _check(eng, y, B, ng, [(0, designs)], edit_scale=off)
    assert fam[0].tolist() == [[B, 3]]
    assert np.isnan(adj[[1, 3, 4], 0, 0]).all() and (adj[[1, 3, 4], 0, 1] == 0).all() and (adj[[0, 2, 5], 0, 0] > 0).all()
    _, _, fam, _ = _check(eng, y, B, ng, [(0, designs)])
    assert fam[0].tolist() == [[B - 1, 4]]


def test_a_family_without_an_included_member(eng):
    B, ng = 300, 3
    y = _random_plane(2, ng, B, 2, seed=301)

    def all_off(scale):
        scale[:3] = 0

    maxrow, adj, fam, _ = _check(eng, y, B, ng, [(0, _pairs(3)), (1, _pairs(3))], edit_scale=all_off)
    assert fam[0].tolist() == [[0, 0]] and fam[1].tolist() == [[B, 3]]
    assert np.isnan(maxrow[0][:, :B + 1]).all() and np.isnan(adj[:3, 0, 0]).all() and (adj[:3, 0, 1] == 0).all()


def test_a_dropped_column_zero(eng):
    """Column 0 of group 2 is not finite: its members have the NaN coefficient, scale 0, and the others go on without them -- also
    when a scale is forced on such a member by hand."""
    B, ng = 300, 4
    y = _random_plane(1, ng, B, 2, seed=311)
    y[2, 0] = np.nan
    designs = _pairs(4)
    with_2 = [j for j, (g, _) in enumerate(designs) if 2 in g]
    _, adj, fam, scale = _check(eng, y, B, ng, [(0, designs)])
    assert (scale[with_2] == 0).all() and fam[0].tolist() == [[B, 3]] and np.isnan(adj[with_2, 0, 0]).all()

    def force(scale):
        scale[with_2] = 1.5

    _, adj2, fam2, _ = _check(eng, y, B, ng, [(0, designs)], edit_scale=force)
    np.testing.assert_array_equal(adj2, adj)
    np.testing.assert_array_equal(fam2, fam)


def test_no_family(eng):
    B, ng = 300, 3
    bs = _shell(eng, _random_plane(1, ng, B, 0, seed=321), B, ng)
    empty_i, empty_f = np.zeros(0, np.int32), np.zeros(0)
    maxrow, adj, fam = bs.family_maxt([0], empty_i, empty_i, [0], empty_i, empty_f, np.zeros((0, 1)))
    assert tuple(maxrow.shape) == (0, 1, B + 1) and adj.shape == (0, 1, 2) and fam.shape == (0, 1, 2)


def test_malformed_tables_raise_before_any_launch(eng):
    B, ng = 300, 3
    bs = _shell(eng, _random_plane(2, ng, B, 0, seed=331), B, ng)
    ok = dict(family_ptr=[0, 2, 3], test_pair=[0, 0, 1], test_design=[0, 1, 0], design_ptr=[0, 2, 4], design_grp=[0, 1, 2, 1],
              design_w=[1.0, -1.0, 1.0, -1.0], scale=np.ones((3, 1)))
    bs.family_maxt(**ok)
    for field, value in (("family_ptr", [0, 2]), ("family_ptr", [1, 2, 3]), ("family_ptr", [0, 3, 2, 3]), ("family_ptr", [0, 1, 3]),
                         ("scale", np.ones((2, 1))), ("scale", np.ones((3, 2))), ("scale", np.ones(3)), ("test_pair", [0, 0, 2]),
                         ("test_design", [0, 2, 0]), ("design_grp", [0, 1, 3, 1]), ("design_ptr", [0, 2, 5]), ("design_w", [1.0, -1.0, 1.0]),
                         ("stage_cap", -1), ("stage_cap", 1025)):
        with pytest.raises(ValueError, match="family_maxt:"):
            bs.family_maxt(**{**ok, field: value})


def test_the_entry_point_refuses_a_stage_cap_out_of_range(eng):
    """Through the C-ABI, past the engine's own check: nothing is launched."""
    import torch

    B, ng = 300, 3
    bs = _shell(eng, _random_plane(1, ng, B, 0, seed=341), B, ng)
    tab = _tables([(0, _pairs(3))])
    d = [eng.dev(np.asarray(a, dtype=np.int32)) for a in tab[:5]] + [eng.dev(tab[5]), eng.dev(np.ones(3))]
    S = -12345.5
    maxrow, adj, fam = (torch.full(s, S, dtype=torch.float64, device="cuda") for s in ((1, bs.ld), (3, 1, 2), (1, 1, 2)))
    for cap in (-1, 1025):
        with pytest.raises(eng._lib.MementoHipError):
            eng._lib.call("mm_family_maxt1", eng.P(bs.yc), bs.ld, B, ng, *map(eng.P, d), cap, 1, eng.P(maxrow), eng.P(adj), eng.P(fam), eng._stream())
    assert (eng.host(maxrow) == S).all() and (eng.host(adj) == S).all() and (eng.host(fam) == S).all()


def test_cells_outside_the_written_region_keep_their_sentinel(eng):
    """Through the C-ABI on sentinel-filled buffers: the kernel writes columns 0..B of the rows of its families, the adj cells of
    its tests and the fam cells of its families -- not the padding of a row, not the rows and cells beyond."""
    import torch

    B, ng, pad = 300, 5, 6
    y = _random_plane(3, ng, B, pad, seed=351)
    families = [(0, _pairs(5)), (2, []), (1, _pairs(3))]
    bs = _shell(eng, y, B, ng)
    tab = _tables(families)
    stt, _ = bs.contrast_design(*tab[1:])
    scale = eng.family_scale(stt)
    want = bs.family_maxt(*tab, scale)
    n_fam, n_tests, ld, S = len(families), len(tab[1]), bs.ld, -12345.5
    maxrow = torch.full((n_fam + 1, 1, ld), S, dtype=torch.float64, device="cuda")
    adj = torch.full((n_tests + 3, 1, 2), S, dtype=torch.float64, device="cuda")
    fam = torch.full((n_fam + 2, 1, 2), S, dtype=torch.float64, device="cuda")
    d = [eng.dev(np.asarray(a, dtype=np.int32)) for a in tab[:5]] + [eng.dev(tab[5]), eng.dev(scale.reshape(-1))]
    eng._lib.call("mm_family_maxt1", eng.P(bs.yc), ld, B, ng, *map(eng.P, d), 4, n_fam, eng.P(maxrow), eng.P(adj), eng.P(fam), eng._stream())
    maxrow, adj, fam = eng.host(maxrow), eng.host(adj), eng.host(fam)
    np.testing.assert_array_equal(maxrow[:n_fam, :, :B + 1], eng.host(want[0])[:, :, :B + 1])
    np.testing.assert_array_equal(adj[:n_tests], want[1])
    np.testing.assert_array_equal(fam[:n_fam], want[2])
    assert (maxrow[:n_fam, :, B + 1:] == S).all() and (maxrow[n_fam:] == S).all() and (adj[n_tests:] == S).all() and (fam[n_fam:] == S).all()


@pytest.mark.parametrize("stage_cap", [None, 3, 0])
def test_the_plane_given_twice_to_the_two_plane_kernel(eng, stage_cap):
    """Parity with the tested kernel: plane 0 of ``Bootstrap1D.family_maxt`` on (y, y) is ``Bootstrap2D.family_maxt`` on y, bit for
    bit -- families of 10, 1, 0 and 6 members, dropped columns, a dropped column 0, a member without replicates that differ."""
    B, ng = 300, 5
    y = _random_plane(4, ng, B, 3, seed=361)
    y[1, 40], y[ng + 3, 41], y[2 * ng + 2, 0] = np.nan, np.inf, np.nan
    y[3 * ng + 1, :B + 1] = y[3 * ng + 1, 0]
    families = [(0, _pairs(5)), (1, _pairs(2)), (2, []), (3, _pairs(4) + [([1], [1.0])]), (2, _pairs(3))]
    tab = _tables(families)
    one, two = _shell(eng, y, B, ng), _shell_1d(eng, y, B, ng)
    stt, _ = one.contrast_design(*tab[1:])
    st_m, st_v, _ = two.contrast_design(*tab[1:])
    np.testing.assert_array_equal(stt, st_m)
    scale = eng.family_scale(stt)
    np.testing.assert_array_equal(eng.family_scale(st_m, st_v), np.column_stack([scale, scale]))
    maxrow1, adj1, fam1 = one.family_maxt(*tab, scale, stage_cap=stage_cap)
    maxrow2, adj2, fam2 = two.family_maxt(*tab, np.column_stack([scale, scale]), stage_cap=stage_cap)
    np.testing.assert_array_equal(eng.host(maxrow1)[:, 0, :B + 1], eng.host(maxrow2)[:, 0, :B + 1])
    np.testing.assert_array_equal(adj1[:, 0], adj2[:, 0])
    np.testing.assert_array_equal(fam1[:, 0], fam2[:, 0])
    np.testing.assert_array_equal(adj2[:, 0], adj2[:, 1])
    assert fam1[:, 0, 1].tolist() == [10, 1, 0, 6, 1] and fam1[0, 0, 0] == B - 1 and fam1[3, 0, 0] == B
