"""Plain numpy restatement of the strict 1D replay bootstrap (mm_boot1d_replay / _free / _chain / _async in csrc/boot.hip), for the
kernel tests.  Nothing here imports the engine: the operands are written out again from numpy's random_multinomial (the arithmetic
of tests/_bins_ref.py: ref_order), the weights are numpy's own draws, and the replicate moments are evaluated in np.longdouble with
the rounding bound of the kernels' sequential fp64 sums.

``menu`` is the fixed set of chains that tests/test_cpu_replay_ref.py pins and tests/test_gpu_replay_kernels.py runs; ``layout``
writes chains of it into the tile planes, the 8-double records and the per-chain arrays the four entry points read, on the host."""

from types import SimpleNamespace

import numpy as np

U = 2.0 ** -53
SENTINEL = np.array([0x7FF8DEADBEEF0BAD], dtype=np.uint64).view(np.float64)[0]      # tests/test_gpu_bins_1d.py: a NaN no kernel produces
PAD = 0xA5A5A5A5                                                                  # weight cells no kernel may touch
SF8 = np.array([0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 2.5, 3.0])
XCAP = 100                                                                         # counts of the menu are below this
Q2 = (0.07, 0.11)                                                                  # the two capture rates of the chains


def chain_operands(mult, v, sf):
    """(pk, lq, v, a, b) per bin of a chain already in replay order: pix = mult / N; remaining_p starts at 1.0 and loses pix[k]
    after bin k, one rounded subtraction after the other; pk = pix / remaining_p; lq = log(1 - p) with p = pk or, above one half,
    1 - pk; a = 1 / sf; b = 1 / (sf * sf)."""
    mult = np.asarray(mult, dtype=np.int64)
    sf = np.asarray(sf, dtype=np.float64)
    pix = mult.astype(np.float64) / np.float64(int(mult.sum()))
    rem = np.empty(len(pix), dtype=np.float64)
    left = np.float64(1.0)
    for k in range(len(pix)):
        rem[k] = left
        left = left - pix[k]
    pk = pix / rem
    p = np.where(pk <= 0.5, pk, 1.0 - pk)
    with np.errstate(divide="ignore", invalid="ignore"):
        lq = np.log(1.0 - p)
    return pk, lq, np.asarray(v, dtype=np.float64), 1.0 / sf, 1.0 / (sf * sf)


def ref_weights(mult, B, seed=5):
    """[K][B] weights: numpy's own multinomial draws (bootstrap.py:102-103 with the generator's seed left open)."""
    mult = np.asarray(mult, dtype=np.int64)
    gen = np.random.Generator(np.random.PCG64(seed))
    return gen.multinomial(int(mult.sum()), mult / mult.sum(), size=B).T


def ref_moments(v, a, b, w, N, q, mean_only=False):
    """(mean, var, bound_mean, bound_var), [B] each: the replicate moments of estimator.py:171-174, :182-183 in np.longdouble and how
    far a sequential fp64 sum of K terms may be from them -- (K + 4) 2^-53 sum|term| / N for the mean, the same for the second
    moment, and for the variance the second-moment bound + 2 m1 bound_mean + 4 * 2^-53 m1^2
    (test_gpu_bins_1d.test_weights_and_replicate_moments_of_the_long_chains).  mean_only (estimator._mean_only_1p): the mean is
    m1 + 1 at the same bound, the variance exactly 10."""
    L = np.longdouble
    K = len(v)
    eL, aL, bL = (np.asarray(x, dtype=np.float64).astype(L)[:, None] for x in (v, a, b))
    wL = np.asarray(w).astype(L)
    omq = L(1.0 - q)
    t1 = eL * wL * aL
    t2a, t2b = eL * eL * wL * bL, omq * eL * wL * bL
    m1 = t1.sum(axis=0) / N
    m2 = (t2a - t2b).sum(axis=0) / N
    var = m2 - m1 * m1
    bound1 = (K + 4) * U * np.abs(t1).sum(axis=0) / N
    bound2 = (K + 4) * U * (np.abs(t2a) + np.abs(t2b)).sum(axis=0) / N
    bound_v = bound2 + 2 * m1 * bound1 + 4 * U * m1 * m1
    if mean_only:
        return m1 + 1, np.full(len(m1), L(10.0)), bound1, np.zeros(len(m1), dtype=L)
    return m1, var, bound1, bound_v


def draw_regimes(mult, w):
    """How numpy drew the weights ``w`` [K][B] of a chain: counts of the binomial draws (bins k < K - 1 that still had cells left)
    by sampler -- inversion up to n min(p, 1 - p) = 30, BTPE above -- and by the p > 0.5 flip, and of the replicates whose cells
    ran out with at least one more draw to make (``early``) or exactly at the last draw (``last_draw``): in both the last bin is 0."""
    mult = np.asarray(mult, dtype=np.int64)
    K, N = len(mult), int(mult.sum())
    pk = chain_operands(mult, np.zeros(K), np.ones(K))[0]
    w = np.asarray(w, dtype=np.int64)
    left = N - np.concatenate([np.zeros((1, w.shape[1]), dtype=np.int64), np.cumsum(w, axis=0)[:-1]])     # cells left BEFORE bin k
    drawn = (left[:K - 1] > 0) & (pk[:K - 1, None] > 0)
    p = np.minimum(pk, 1.0 - pk)[:K - 1, None]
    inv = drawn & (p * left[:K - 1] <= 30.0)
    out_at = np.argmax(np.cumsum(w, axis=0) >= N, axis=0)                                                 # the bin that took the last cell
    return SimpleNamespace(inversion=int(inv.sum()), btpe=int((drawn & ~inv).sum()), flipped=int((drawn & (pk[:K - 1, None] > 0.5)).sum()),
                           early=int((out_at < K - 2).sum()), last_draw=int((out_at == K - 2).sum()))


_MENU = []


def _chain(rng, name, mult, qi):
    """A menu chain: the multiplicities as given, K distinct (size-factor bin, count) cells -- one of them with count 0 -- and two
    hash uniforms; the cells are handed to the bins in ascending code, so that the chain IS in replay order (ref_order keeps it)."""
    mult = np.asarray(mult, dtype=np.int64)
    K = len(mult)
    cells = rng.choice(len(SF8) * (XCAP - 1), size=K - 1, replace=False)
    sf_bin = np.concatenate([[rng.integers(len(SF8))], cells // (XCAP - 1)]).astype(np.int64)
    x = np.concatenate([[0], 1 + cells % (XCAP - 1)]).astype(np.int64)
    r1, r0 = rng.random(2)
    code = x.astype(np.float64) * np.float64(r1) + np.float64(r0) * SF8[sf_bin]
    o = np.argsort(code, kind="stable")
    assert (np.diff(code[o]) > 0).all()
    return SimpleNamespace(name=name, mult=mult, K=K, N=int(mult.sum()), sf_bin=sf_bin[o], x=x[o], v=x[o].astype(np.float64),
                           sf=SF8[sf_bin[o]], r1=float(r1), r0=float(r0), q=Q2[qi])


def menu():
    """The fixed chains, by name (computed once).  Behind the nine named ones 54 fillers f00 ... f53 with 2 to 40 bins."""
    if _MENU:
        return _MENU[0]
    rng = np.random.default_rng(20240607)
    ii = lambda lo, hi, n: rng.integers(lo, hi + 1, size=n)
    lists = [
        ("k2", [3, 2]),
        ("k3_flip", [950, 30, 20]),
        ("six_ones", [1] * 6),
        ("k64", ii(1, 39, 64)),
        ("k65", ii(1, 39, 65)),
        ("long600", np.concatenate([[14000], ii(1, 59, 599)])),
        ("btpe12", ii(1500, 2499, 12)),
        ("huge", [2 ** 29, 2 ** 29 - 7, 7]),
        ("tail_tiny", [5000, 3000] + [1] * 30),
    ]
    for i in range(54):
        lists.append((f"f{i:02d}", ii(1, 400, 2 + (i * 7) % 39)))
    m = {name: _chain(rng, name, mult, i % 2) for i, (name, mult) in enumerate(lists)}
    _MENU.append(m)
    return m


MENU_NAMES = ("k2", "k3_flip", "six_ones", "k64", "k65", "long600", "btpe12", "huge", "tail_tiny")


def adhoc_chain(name, mult):
    """A chain outside the menu, for ``layout``: the multiplicities as given, counts 0, 1, 2, ... and the size factors of SF8 in
    turn (arbitrary operands for tests that compare weights)."""
    mult = np.asarray(mult, dtype=np.int64)
    K = len(mult)
    sf_bin = np.arange(K) % len(SF8)
    x = np.arange(K, dtype=np.int64)
    return SimpleNamespace(name=name, mult=mult, K=K, N=int(mult.sum()), sf_bin=sf_bin, x=x, v=x.astype(np.float64), sf=SF8[sf_bin],
                           r1=0.5, r0=0.5, q=Q2[0])


def one_bin_chain():
    """The K == 1 chain of tile 4: every replicate of it is NaN (bootstrap.py:97-98)."""
    return SimpleNamespace(name="one_bin", mult=np.array([777], dtype=np.int64), K=1, N=777, sf_bin=np.array([2]), x=np.array([4]),
                           v=np.array([4.0]), sf=SF8[[2]], r1=0.5, r0=0.5, q=Q2[0])


# ------------------------------------------------------------------------------------------------------------------------
# the slot layout
# ------------------------------------------------------------------------------------------------------------------------
# kinds of a lane: "run" = an active chain; "k1" = one bin (NaN row from the tile kernels, unused in the async one);
# "k0" = K = 0 with a valid row; "norow" = K = 5 with row -1; "norec" = slot_rec -1 in the free kernel's tables (a chain of 4 bins
# with a valid row there; a plain empty lane everywhere else).  ("norow" is K = 0 in the async kernel's tables: that kernel's
# contract knows unused lanes by K < 2 alone.)


def full_tiles(with_long_twin=True, first=True):
    """The five tiles of the kernel tests as {lane: (kind, chain name)}: 64 active lanes; 5 active lanes (one more than
    BOOT_TAIL_LANES; lane 63 the twin of long600); 4; 1; lanes that write nothing and a K == 1 lane."""
    names = list(MENU_NAMES) + [f"f{i:02d}" for i in range(54)]
    lanes0 = np.random.default_rng(64).permutation(64)
    t0 = {int(lanes0[i]): ("run", n) for i, n in enumerate(names + ["k2"])}                     # 9 + 54 + a twin of k2 = 64
    t1 = {0: ("run", "tail_tiny"), 7: ("run", "btpe12"), 31: ("run", "k65"), 40: ("run", "huge"), 63: ("run", "long600")}
    if not with_long_twin:
        del t1[63]
    t2 = {5: ("run", "btpe12"), 6: ("run", "huge"), 33: ("run", "k64"), 62: ("run", "f07")}
    t3 = {17: ("run", "six_ones")}
    t4 = {3: ("k0", None), 9: ("norow", None), 20: ("norec", "f03"), 41: ("k1", None)}
    return ([t0] if first else []) + [t1, t2, t3, t4]


def layout(tiles, extra_rows=7, kmax_pad=3):
    """Host tables of a launch over ``tiles``: a list whose items are {lane: (kind, chain name)} (a tile) or a chain name (a tile
    that is a chain of the record form: mm_chain_tiles).  In a tile an ad-hoc chain (``adhoc_chain``) may stand in place of a
    menu chain's name.  Every chain's operands are written twice, into the five [rows][64]
    planes and as 8-double records; cells nobody owns hold harmless finite operands (pk 0.25, v 1e6).  Rows are a permutation of
    the row owners plus ``extra_rows`` rows nothing addresses."""
    m = menu()
    n_tiles = len(tiles)
    ents = []
    for t, tile in enumerate(tiles):
        if isinstance(tile, str):
            ents.append(SimpleNamespace(tile=t, lane=-1, slot=-1, kind="flag", chain=m[tile]))
            continue
        for lane in sorted(tile):
            kind, name = tile[lane]
            ch = (m[name] if isinstance(name, str) else name) if name is not None else (one_bin_chain() if kind == "k1" else None)
            ents.append(SimpleNamespace(tile=t, lane=lane, slot=t * 64 + lane, kind=kind, chain=ch))
    owners = [e for e in ents if e.kind != "norow"]
    n_rows = len(owners) + extra_rows
    ci = np.cumsum([e.kind in ("run", "flag") for e in owners]) - 1                                # index in the per-chain arrays
    for seed in range(n_rows, n_rows + 1000):                      # a permutation in which no row is its owner's slot or chain index
        perm = np.random.default_rng(seed).permutation(n_rows)
        if all(perm[i] != e.slot and perm[i] != ci[i] for i, e in enumerate(owners)):
            break
    else:
        raise AssertionError("no permutation found")
    for i, e in enumerate(owners):
        e.row = int(perm[i])
    for e in ents:
        if e.kind == "norow":
            e.row = -1
        e.label = f"tile {e.tile} lane {e.lane} row {e.row} ({e.kind}{': ' + e.chain.name if e.chain is not None else ''})"
        e.K = {"k0": 0, "norow": 5}.get(e.kind, e.chain.K if e.chain is not None else 0)
    # rows of the planes: a tile owns as many as its longest lane, one at least (an unused lane still reads the tile's first row)
    tile_k = np.zeros(n_tiles, dtype=np.int64)
    for e in ents:
        if e.kind not in ("flag", "norec"):
            tile_k[e.tile] = max(tile_k[e.tile], e.K)
    for t, tile in enumerate(tiles):
        tile_k[t] = 0 if isinstance(tile, str) else max(1, tile_k[t])
    tile_ptr = np.concatenate([[0], np.cumsum(tile_k)]).astype(np.int64)
    n_plane_rows = max(1, int(tile_ptr[-1]))
    planes = np.empty((5, n_plane_rows, 64))
    planes[0], planes[1], planes[2], planes[3], planes[4] = 0.25, np.log(0.75), 1e6, 1.0, 1.0
    n_slots = n_tiles * 64
    L = SimpleNamespace(n_tiles=n_tiles, n_slots=n_slots, n_rows=n_rows, tile_ptr=tile_ptr, ents=ents)
    L.slot_K, L.slot_row = np.zeros(n_slots, dtype=np.int32), np.full(n_slots, -1, dtype=np.int64)
    L.slot_nobs, L.slot_omq = np.zeros(n_slots), np.zeros(n_slots)
    L.free_K, L.free_row, L.slot_rec = L.slot_K.copy(), L.slot_row.copy(), np.full(n_slots, -1, dtype=np.int64)
    L.as_K, L.as_row, L.as_base = L.slot_K.copy(), np.zeros(n_slots, dtype=np.int64), np.zeros(n_slots, dtype=np.int64)
    recs, n_rec = [], 0
    ch = SimpleNamespace(base=[], K=[], nobs=[], omq=[], row=[])
    L.tile_chain = np.full(n_tiles, -1, dtype=np.int32)
    for e in ents:
        e.ci, e.rec = -1, -1
        if e.chain is not None:
            ops = np.stack(chain_operands(e.chain.mult, e.chain.v, e.chain.sf), axis=1)             # [K][5]
            rec = np.zeros((e.chain.K + 1, 8))                                                      # (one spare record behind each chain)
            rec[:, :5] = (0.25, np.log(0.75), 1e6, 1.0, 1.0)
            rec[:e.chain.K, :5] = ops
            e.rec, n_rec = n_rec, n_rec + len(rec)
            recs.append(rec)
        s = e.slot
        if e.kind in ("run", "k1"):
            planes[:, tile_ptr[e.tile]:tile_ptr[e.tile] + e.K, e.lane] = ops.T
            for K_, row_ in ((L.slot_K, L.slot_row), (L.free_K, L.free_row)):
                K_[s], row_[s] = e.K, e.row
            L.slot_rec[s] = e.rec
            L.slot_nobs[s], L.slot_omq[s] = e.chain.N, 1.0 - e.chain.q
            L.as_K[s], L.as_row[s], L.as_base[s] = e.K, e.row, e.rec
        elif e.kind == "k0":
            L.slot_row[s] = L.free_row[s] = L.as_row[s] = e.row
            L.slot_rec[s] = 0
            L.slot_nobs[s], L.slot_omq[s] = 1000.0, 0.9
        elif e.kind == "norow":
            L.slot_K[s] = L.free_K[s] = 5
            L.slot_rec[s] = 0
            L.slot_nobs[s], L.slot_omq[s] = 1000.0, 0.9
        elif e.kind == "norec":
            L.free_K[s], L.free_row[s] = e.K, e.row                                                 # slot_rec stays -1
            L.slot_nobs[s], L.slot_omq[s] = e.chain.N, 1.0 - e.chain.q
        if e.kind in ("run", "flag"):
            e.ci = len(ch.K)
            ch.base.append(e.rec), ch.K.append(e.K), ch.nobs.append(float(e.chain.N)), ch.omq.append(1.0 - e.chain.q), ch.row.append(e.row)
            if e.kind == "flag":
                L.tile_chain[e.tile] = e.ci
    L.as_nobs, L.as_omq = L.slot_nobs.copy(), L.slot_omq.copy()
    L.planes = planes.reshape(5, -1)
    L.recs = np.concatenate(recs).reshape(-1) if recs else np.zeros(8)
    L.n_rec = max(1, n_rec)
    L.ch_base, L.ch_K = np.array(ch.base, dtype=np.int64), np.array(ch.K, dtype=np.int32)
    L.ch_nobs, L.ch_omq, L.ch_row = np.array(ch.nobs), np.array(ch.omq), np.array(ch.row, dtype=np.int64)
    L.n_chains = len(ch.K)
    L.kmax = int(max(e.K for e in ents)) + kmax_pad
    L.row_used = sorted(e.row for e in owners)
    return L


# ------------------------------------------------------------------------------------------------------------------------
# the small ingest of the routing tests
# ------------------------------------------------------------------------------------------------------------------------


def routing_problem():
    """3,000 cells in three groups (1,800 / 1,140 / 60; the cells of the small one share a size-factor bin, so its chains start at
    two bins), 40 genes -- two dense ones with counts up to 79, the others Poisson with means from 0.02 to 3 -- and eight
    size-factor bins: K spans 2 to several hundred."""
    rng = np.random.default_rng(3000)
    n, G = 3000, 40
    gid = np.repeat(np.arange(3, dtype=np.int32), [1800, 1140, 60])[rng.permutation(n)]
    sf_bin = rng.integers(0, 8, size=n).astype(np.uint8)
    sf_bin[gid == 2] = 3
    X = rng.poisson(np.geomspace(0.02, 3.0, G), size=(n, G)).astype(np.int64)
    X[:, 0] = rng.integers(0, 80, size=n)
    X[:, 1] = rng.integers(0, 50, size=n)
    r = rng.random((2, G * 3))
    sel = [np.flatnonzero(gid == k) for k in range(3)]
    return SimpleNamespace(n=n, ng=3, n_genes=G, n_bins=8, gid=gid, sf_table=SF8, sf_bin=sf_bin, X=X, r1=r[0], r0=r[1], sel=sel,
                           sizes=[len(s) for s in sel], grp_q=np.array([0.07, 0.11, 0.09]))
