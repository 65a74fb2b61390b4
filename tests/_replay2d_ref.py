"""Plain numpy restatement of the strict gene-pair (2D) replay bootstrap (mm_boot2d_replay / mm_boot2d_replay_rec and, given its
dumped weights, mm_boot2d_fast in csrc/boot.hip), for the kernel tests.  The 2D twin of tests/_replay_ref.py, on the same
multiplicities: ``ref_weights`` and ``draw_regimes`` of that file apply unchanged.  Nothing here imports the engine.

``menu2d`` is the fixed set of chains tests/test_cpu_replay2d_ref.py pins and tests/test_gpu_replay2d_kernels.py runs; ``layout2d``
writes chains of it into the six tile planes, the 8-double records and the slot tables the entry points read, on the host."""

from types import SimpleNamespace

import numpy as np

from _replay_ref import MENU_NAMES, Q2, SENTINEL, SF8, U, XCAP, chain_operands, menu

SPECIAL = ("zero_left", "same", "anti", "overflow", "one_bin2d")
VALUE, SENT, AMBIGUOUS = 0, 1, 2          # classes of a replicate (ref_corr_2d)
RHO_LO, RHO_HI = -0.98, 0.8                # slopes of x2 on x1 over the ordinary chains (the shared 1/sf adds correlation of its own)
AMBIGUITY = 1000.0                        # a variance must exceed this many of its own bounds for the first-order propagation


# ------------------------------------------------------------------------------------------------------------------------
# the chains
# ------------------------------------------------------------------------------------------------------------------------

_MENU2D = []


def _finish(name, mult, sf_bin, x1, x2, ra, rb, r0, qi, rho):
    """Bins handed out in ascending code x1 ra + x2 rb + r0 sf (bootstrap.py:62-65, two columns), so that the chain IS in replay
    order; the multiplicities keep the order they were given in, as in tests/_replay_ref.py."""
    mult = np.asarray(mult, dtype=np.int64)
    x1, x2 = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
    sf_bin = np.asarray(sf_bin, dtype=np.int64)
    code = x1 * np.float64(ra) + x2 * np.float64(rb)
    code = code + np.float64(r0) * SF8[sf_bin]
    o = np.argsort(code, kind="stable")
    assert (np.diff(code[o]) > 0).all(), name
    return SimpleNamespace(name=name, mult=mult, K=len(mult), N=int(mult.sum()), sf_bin=sf_bin[o], x1=x1[o], x2=x2[o], sf=SF8[sf_bin[o]],
                           ra=float(ra), rb=float(rb), r0=float(r0), q=Q2[qi], rho=rho)


def _cells(rng, K):
    """K distinct (size-factor bin, count) cells, one of them with count 0 (tests/_replay_ref.py: _chain)."""
    cells = rng.choice(len(SF8) * (XCAP - 1), size=K - 1, replace=False)
    return (np.concatenate([[rng.integers(len(SF8))], cells // (XCAP - 1)]).astype(np.int64),
            np.concatenate([[0], 1 + cells % (XCAP - 1)]).astype(np.int64))


def _chain2d(rng, name, mult, qi, rho):
    """An ordinary chain: the left counts as in 1D; the right ones x2 = round(50 + rho (x1 - 50) + noise) clipped to [0, XCAP), the
    noise normal with the standard deviation that leaves x2 the spread of x1 (28.9 sqrt(1 - rho^2)).  (sf_bin, x1) is distinct
    already, so (sf_bin, x1, x2) is."""
    K = len(mult)
    sf_bin, x1 = _cells(rng, K)
    noise = rng.normal(0.0, 28.9 * np.sqrt(1.0 - rho * rho), size=K)
    x2 = np.clip(np.rint(50.0 + rho * (x1 - 50.0) + noise), 0, XCAP - 1)
    ra, rb, r0 = rng.random(3)
    return _finish(name, mult, sf_bin, x1, x2, ra, rb, r0, qi, rho)


def menu2d():
    """The fixed chains, by name (computed once): the multiplicities of tests/_replay_ref.py: menu -- nine named chains and 54
    fillers, the ordinary chains -- and the five special ones of SPECIAL."""
    if _MENU2D:
        return _MENU2D[0]
    rng = np.random.default_rng(20240611)
    m1d = menu()
    names = list(m1d)
    rhos = np.linspace(RHO_LO, RHO_HI, len(names))[np.random.default_rng(7).permutation(len(names))]
    m = {n: _chain2d(rng, n, m1d[n].mult, i % 2, float(rhos[i])) for i, n in enumerate(names)}
    ii = lambda lo, hi, n: rng.integers(lo, hi + 1, size=n)
    # zero_left: x1 == 0 in every bin (distinct (sf_bin, x2) cells)
    sf_bin, x2 = _cells(rng, 12)
    m["zero_left"] = _finish("zero_left", ii(1, 400, 12), sf_bin, np.zeros(12), x2, *rng.random(3), 0, None)
    # same: x2 == x1;  anti: x2 = (XCAP - 1) - x1
    sf_bin, x1 = _cells(rng, 20)
    m["same"] = _finish("same", ii(1, 400, 20), sf_bin, x1, x1, *rng.random(3), 1, None)
    x1 = rng.choice(XCAP, size=20, replace=False)                       # (one size factor, 1.0: x2 / sf is exactly c - x1 / sf)
    m["anti"] = _finish("anti", ii(1, 400, 20), np.full(20, 2), x1, (XCAP - 1) - x1, *rng.random(3), 0, None)
    # overflow: operands near 1e80 at sf = 1: var1 and var2 are finite (about 1e160), their product is not
    m["overflow"] = _finish("overflow", [40, 35, 25], [2, 2, 2], [1e80, 2e80, 3e80], [3e80, 1e80, 2e80], *rng.random(3), 1, None)
    # one_bin2d: K == 1 (bootstrap.py:119-157 has no shortcut for it)
    m["one_bin2d"] = _finish("one_bin2d", [777], [2], [4.0], [7.0], 0.5, 0.25, 0.5, 0, None)
    _MENU2D.append(m)
    return m


def ordinary_names():
    return [n for n in menu2d() if n not in SPECIAL]


def chain_operands_2d(c):
    """(pk, lq, x1, x2, a, b) per bin of chain ``c``, [K] each (pk and lq: tests/_replay_ref.py: chain_operands), as ``.ops``;
    the same as six columns ``.planes`` [K][6] (one plane each in a tile) and as ``.recs`` [K][8]: pk, lq, x1, x2, 1/sf, 1/sf^2, 0, 0."""
    pk, lq, _, a, b = chain_operands(c.mult, c.x1, c.sf)
    ops = (pk, lq, c.x1, c.x2, a, b)
    planes = np.stack(ops, axis=1)
    recs = np.zeros((c.K, 8))
    recs[:, :6] = planes
    return SimpleNamespace(ops=ops, planes=planes, recs=recs)


def ref_corr_2d(x1, x2, a, b, w, N, q):
    """The replicate correlations of bootstrap.py:141-155 / estimator.py:214-218, :171-174, :281-292 on the weights ``w`` [K][B],
    in np.longdouble, as accumulate_2d / close_replicate_2d of csrc/boot.hip form them: with wk the weight of bin k

        A1 = sum x1 wk a    A2 = sum x2 wk a    MX = sum x1 x2 wk b    Qi = sum (xi xi wk b - (1 - q) xi wk b)
        m1 = A1 / N   m2 = A2 / N   cov = MX / N - m1 m2   vari = Qi / N - mi mi
        corr = cov / sqrt(var1 var2) where var1 > 0, var2 > 0 and the root is finite, else 5.0; then clipped to [-1, 1].

    Returns .corr (clipped), .cov, .var1, .var2, .bound and .kind, [B] each.

    The bound (how far the fp64 kernel may be from .corr; u = 2^-53, a function of the inputs only):
      * a term of a sum is a product of at most four factors (three roundings, each relative u) or, in Qi, the difference of two
        such products (one more rounding, of at most u times the sum of the two magnitudes); K - 1 sequential additions each add
        at most u times the running sum of magnitudes; the division by N one more u.  So each sum / N is within
        e_S = (K + 6) u sum|term| / N of its exact value, |term| in Qi the sum of the two products' magnitudes (6 = 3 + 1 + 1 and
        one u for the second-order terms up to K = 10^4).
      * cov: e_cov = e_MX + |m1| e_A2 + |m2| e_A1 + e_A1 e_A2 + 2 u (|MX / N| + |m1 m2|)      (product and subtraction rounded)
        vari: e_vi = e_Qi + 2 |mi| e_Ai + e_Ai^2 + 2 u (|Qi / N| + mi^2)
      * f = cov / sqrt(var1 var2), to first order: |df| <= e_cov / sqrt(var1 var2) + |f| / 2 (e_v1 / var1 + e_v2 / var2).  With
        both variances above AMBIGUITY = 1000 of their bounds the neglected terms are below 0.2 % of that: factor 1.01.  The
        product, the root and the division round once each (the root halves the product's): 3 u |f| at most.
        bound = 1.01 (e_cov / sqrt(var1 var2) + |f| / 2 (e_v1 / var1 + e_v2 / var2)) + 3 u |f|.
      * The clip to [-1, 1] is 1-Lipschitz: the bound holds after clipping both sides.

    kind: VALUE -- both variances exceed 1000 of their bounds and var1 var2 is clearly finite: the kernel is within .bound of .corr;
    SENT -- a variance is below -1000 of its bound, or is exactly 0 with a bound of 0 (every term of its sums is 0, so the kernel's
    sums are too), or both are clearly positive and their product exceeds 2^1024 by more than 1 %: the kernel gives exactly 1.0
    (.corr is 1.0, .bound 0); AMBIGUOUS -- everything else (the sign of a variance, or the finiteness of the product, is within
    rounding): the kernel's value lies in [-1, 1], nothing more is known."""
    L = np.longdouble
    K = len(x1)
    x1L, x2L, aL, bL = (np.asarray(x, dtype=np.float64).astype(L)[:, None] for x in (x1, x2, a, b))
    wL = np.asarray(w).astype(L)
    N = L(N)
    omq = L(np.float64(1.0) - np.float64(q))
    tA1, tA2, tMX = x1L * wL * aL, x2L * wL * aL, x1L * x2L * wL * bL
    tQ1a, tQ1b = x1L * x1L * wL * bL, omq * x1L * wL * bL
    tQ2a, tQ2b = x2L * x2L * wL * bL, omq * x2L * wL * bL
    s = lambda t: t.sum(axis=0) / N
    e = lambda *ts: (K + 6) * L(U) * sum(np.abs(t) for t in ts).sum(axis=0) / N
    m1, m2, mx, q1, q2 = s(tA1), s(tA2), s(tMX), s(tQ1a - tQ1b), s(tQ2a - tQ2b)
    eA1, eA2, eMX, eQ1, eQ2 = e(tA1), e(tA2), e(tMX), e(tQ1a, tQ1b), e(tQ2a, tQ2b)
    cov, var1, var2 = mx - m1 * m2, q1 - m1 * m1, q2 - m2 * m2
    e_cov = eMX + np.abs(m1) * eA2 + np.abs(m2) * eA1 + eA1 * eA2 + 2 * L(U) * (np.abs(mx) + np.abs(m1 * m2))
    e_v1 = eQ1 + 2 * np.abs(m1) * eA1 + eA1 * eA1 + 2 * L(U) * (np.abs(q1) + m1 * m1)
    e_v2 = eQ2 + 2 * np.abs(m2) * eA2 + eA2 * eA2 + 2 * L(U) * (np.abs(q2) + m2 * m2)
    pos1, pos2 = var1 > AMBIGUITY * e_v1, var2 > AMBIGUITY * e_v2
    non1 = (var1 < -AMBIGUITY * e_v1) | ((var1 == 0) & (e_v1 == 0))
    non2 = (var2 < -AMBIGUITY * e_v2) | ((var2 == 0) & (e_v2 == 0))
    big = L(2.0) ** 1024
    prod = np.where(pos1 & pos2, var1 * var2, L(1.0))
    kind = np.full(wL.shape[1], AMBIGUOUS, dtype=np.int64)
    kind[pos1 & pos2 & (prod < big / L(1.01))] = VALUE
    kind[non1 | non2 | (pos1 & pos2 & (prod > big * L(1.01)))] = SENT
    ok = kind == VALUE
    root = np.sqrt(np.where(ok, prod, L(1.0)))
    f = np.where(ok, cov / root, L(5.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = 1.01 * (e_cov / root + np.abs(f) / 2 * (e_v1 / np.where(ok, var1, L(1.0)) + e_v2 / np.where(ok, var2, L(1.0)))) + 3 * L(U) * np.abs(f)
    bound = np.where(ok, bound, L(0.0))
    corr = np.clip(f, L(-1.0), L(1.0))
    corr[kind == AMBIGUOUS] = L("nan")
    return SimpleNamespace(corr=corr, raw=f, cov=cov, var1=var1, var2=var2, bound=bound, kind=kind, e_v1=e_v1, e_v2=e_v2, e_cov=e_cov)


# ------------------------------------------------------------------------------------------------------------------------
# the slot layout
# ------------------------------------------------------------------------------------------------------------------------
# kinds of a lane: "run" = an active chain; "k0" = K = 0 with a valid row; "norow" = K = 5 with row -1; "norec" = slot_rec -1 in the
# records tables, with a valid K and row there (a plain empty lane in the planes tables).  The last three must write nothing.


def full_tiles_2d(with_long_twin=True, first=True):
    """The five tiles of the kernel tests as {lane: (kind, chain name)}: 64 active lanes (the 63 ordinary chains and ``same``);
    5 (one more than BOOT_TAIL_LANES; lane 63 the twin of long600); 4; 1; and one of lanes that must write nothing."""
    names = list(MENU_NAMES) + [f"f{i:02d}" for i in range(54)] + ["same"]
    lanes0 = np.random.default_rng(64).permutation(64)
    t0 = {int(lanes0[i]): ("run", n) for i, n in enumerate(names)}
    t1 = {0: ("run", "tail_tiny"), 7: ("run", "btpe12"), 31: ("run", "anti"), 40: ("run", "huge"), 63: ("run", "long600")}
    if not with_long_twin:
        del t1[63]
    t2 = {5: ("run", "one_bin2d"), 6: ("run", "overflow"), 33: ("run", "k64"), 62: ("run", "zero_left")}
    t3 = {17: ("run", "six_ones")}
    t4 = {3: ("k0", None), 9: ("norow", None), 20: ("norec", "f03")}
    return ([t0] if first else []) + [t1, t2, t3, t4]


def twin_tiles_2d():
    """The chains of full_tiles_2d in other lanes, tiles and company: the tile of unused lanes first, the four special chains of
    tiles 1 and 2 inside the 64-lane tile (in place of four fillers, which take their lanes), another lane permutation, every tile
    at another index."""
    t0, t1, t2, t3, t4 = full_tiles_2d()
    lanes0 = np.random.default_rng(65).permutation(64)
    swap = {"f10": "anti", "f20": "one_bin2d", "f30": "overflow", "f40": "zero_left"}
    back = {v: k for k, v in swap.items()}
    n0 = [t0[l][1] for l in sorted(t0)]
    u0 = {int(lanes0[i]): ("run", swap.get(n, n)) for i, n in enumerate(n0)}
    u1 = {(l * 5 + 3) % 64: ("run", back.get(n, n)) for l, (_, n) in t1.items()}
    u2 = {(l * 7 + 1) % 64: ("run", back.get(n, n)) for l, (_, n) in t2.items()}
    u3 = {44: t3[17]}
    u4 = {60: t4[3], 0: t4[9], 33: t4[20]}
    return [u4, u3, u0, u2, u1]


def many_tiles_2d(n_extra=2044):
    """More than 2,048 tiles: the five real ones and ``n_extra`` tiles of one k2 chain each, the lane moving with the tile."""
    return full_tiles_2d() + [{(t * 29) % 64: ("run", "k2")} for t in range(n_extra)]


_OPS = {}


def _ops_of(c):
    if c.name not in _OPS:
        _OPS[c.name] = chain_operands_2d(c)
    return _OPS[c.name]


def layout2d(tiles, extra_rows=7, kmax_pad=3):
    """Host tables of a launch over ``tiles`` (a list of {lane: (kind, chain name)}).  Every chain's operands are written twice, into
    the six [rows][64] planes and as 8-double records (one spare record behind each chain); cells nobody owns hold harmless finite
    operands (pk 0.25, x 1e6).  Output rows are a permutation of the row owners plus ``extra_rows`` rows nothing addresses, no row
    equal to its owner's slot.  ``out_init(B)``: the output as uploaded, ld = B + 4, a payload in column 0, SENTINEL elsewhere."""
    m = menu2d()
    n_tiles = len(tiles)
    ents = []
    for t, tile in enumerate(tiles):
        for lane in sorted(tile):
            kind, name = tile[lane]
            ents.append(SimpleNamespace(tile=t, lane=lane, slot=t * 64 + lane, kind=kind, chain=m[name] if name else None))
    owners = [e for e in ents if e.kind != "norow"]
    n_rows = len(owners) + extra_rows
    for seed in range(n_rows, n_rows + 1000):
        perm = np.random.default_rng(seed).permutation(n_rows)
        if all(perm[i] != e.slot for i, e in enumerate(owners)):
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
    # rows of the planes: a tile owns as many as its longest running lane, one at least (an unused lane reads the tile's first row)
    tile_k = np.ones(n_tiles, dtype=np.int64)
    for e in ents:
        if e.kind == "run":
            tile_k[e.tile] = max(tile_k[e.tile], e.K)
    tile_ptr = np.concatenate([[0], np.cumsum(tile_k)]).astype(np.int64)
    idle = (0.25, np.log(0.75), 1e6, 1e6, 1.0, 1.0)
    planes = np.empty((6, int(tile_ptr[-1]), 64))
    for i, v in enumerate(idle):
        planes[i] = v
    n_slots = n_tiles * 64
    L = SimpleNamespace(n_tiles=n_tiles, n_slots=n_slots, n_rows=n_rows, tile_ptr=tile_ptr, ents=ents)
    L.slot_K, L.slot_row = np.zeros(n_slots, dtype=np.int32), np.full(n_slots, -1, dtype=np.int64)
    L.slot_nobs, L.slot_omq = np.zeros(n_slots), np.zeros(n_slots)
    L.rec_K, L.rec_row, L.slot_rec = L.slot_K.copy(), L.slot_row.copy(), np.full(n_slots, -1, dtype=np.int64)
    recs, n_rec = [], 0
    for e in ents:
        e.rec = -1
        s = e.slot
        if e.chain is not None:
            o = _ops_of(e.chain)
            rec = np.zeros((e.chain.K + 1, 8))
            rec[:, :6] = idle
            rec[:e.chain.K] = o.recs
            e.rec, n_rec = n_rec, n_rec + len(rec)
            recs.append(rec)
            L.slot_nobs[s], L.slot_omq[s] = e.chain.N, 1.0 - e.chain.q
        else:
            L.slot_nobs[s], L.slot_omq[s] = 1000.0, 0.9
        if e.kind == "run":
            planes[:, tile_ptr[e.tile]:tile_ptr[e.tile] + e.K, e.lane] = o.planes.T
            L.slot_K[s] = L.rec_K[s] = e.K
            L.slot_row[s] = L.rec_row[s] = e.row
            L.slot_rec[s] = e.rec
        elif e.kind == "k0":
            L.slot_row[s] = L.rec_row[s] = e.row
            L.slot_rec[s] = 0
        elif e.kind == "norow":
            L.slot_K[s] = L.rec_K[s] = 5
            L.slot_rec[s] = 0
        elif e.kind == "norec":
            L.rec_K[s], L.rec_row[s] = e.K, e.row                                                   # slot_rec stays -1
    L.planes = planes.reshape(6, -1)
    L.recs = np.concatenate(recs).reshape(-1) if recs else np.zeros(8)
    L.n_rec = max(1, n_rec)
    L.kmax = int(max(e.K for e in ents)) + kmax_pad
    L.row_used = sorted(e.row for e in owners)
    L.slot_key = (np.arange(n_slots, dtype=np.int64) * 7919 + 13) % 1000003                          # mm_boot2d_fast: stream keys

    def out_init(B):
        init = np.full((n_rows, B + 4), SENTINEL)
        init[:, 0] = 1000.0 + np.arange(n_rows)
        return init

    L.out_init = out_init
    return L
