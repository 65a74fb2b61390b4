"""``ht_1d_moments(strict=True)``: the sequential replay of the reference's global ``np.random`` stream over one chunk of genes.

The reference (num_cpus=1) consumes ONE stream gene after gene: per gene the two hash uniforms of every live group
(bootstrap.py:62,65), the ``np.random.choice`` of ``_fill`` for every group with invalid replicates (hypothesis_test.py:23-33)
right after that group's bootstrap, and -- with resample_rep -- the two ``np.random.choice`` draws of ``_regress_1d``
(hypothesis_test.py:275-278) after the gene's last group.  Which groups need a fill is known only after their bootstrap, so the
replay speculates (draw all remaining uniforms, bootstrap all remaining pairs at once) and rolls the stream back to the first
pair whose draws shift it.  Meant for validation: exactly reproducible against the reference, not fast.
"""

import numpy as np

from .. import engine


def _host_fill(row):
    """hypothesis_test._fill on an already-logged row: NaN = invalid; draws from the global np.random
    stream exactly like np.random.choice(val[~cond], num_invalid) (hypothesis_test.py:23-33)."""
    bad = np.isnan(row)
    nbad = int(bad.sum())
    if nbad == row.shape[0]:
        return None
    row = row.copy()
    row[bad] = np.random.choice(row[~bad], nbad)
    return row


def host_replicates(t, p):
    """The replicates (columns 1..) of row ``p`` of the device tensor ``t``, on the host."""
    return engine.host(t[p, 1:])


def store_replicates(t, p, row):
    t[p, 1:] = engine.dev(row)


class StrictReplay:
    """The replay over one opened chunk (``chunk.bs``, ``.skip``: see ``_ht.chunks_1d``).

    ``run_from(r1, r0, first_pair=first)`` orders the bins with the hash uniforms ``r1`` / ``r0`` [pair], bootstraps every pair >=
    ``first`` and returns their ``n_inv`` [pair - first][2] (invalid mean / variability replicates, -1 = no valid one), leaving the
    invalid replicates NaN.  ``gene_trt``: with resample_rep, the treatment matrix [group][column] of every gene of the chunk;
    None = no resample_rep.  ``load(t, p)`` / ``store(t, p, row)`` read and write the replicates of row ``p`` of ``bs.ym`` /
    ``bs.yv`` (device tensors by default).

    ``run()`` fills the invalid replicates in place and returns ``bad_fill`` [pair].  State it leaves: ``r1`` / ``r0`` [pair];
    ``known_bad`` [pair] -- live pairs whose fill found no valid replicate; ``rep_assign`` / ``bcol_assign``
    [gene][group][replicate] -- the replayed assignment draws (None without resample_rep); ``nb_eff`` -- of genes whose replicate
    columns are not all finite, the columns left after hypothesis_test.py:249-251, minus one."""

    def __init__(self, chunk, run_from, gene_trt=None, load=host_replicates, store=store_replicates):
        self.bs, self.skip = chunk.bs, chunk.skip
        self.run_from, self.load, self.store = run_from, load, store
        self.gene_trt = gene_trt
        self.resample_rep = gene_trt is not None
        self.ng, self.num_boot, self.n_pairs = self.bs.ng, self.bs.B, self.bs.n_pairs
        self.G = self.n_pairs // self.ng
        self.live = np.flatnonzero(~self.skip)
        self.r1, self.r0 = np.zeros(self.n_pairs), np.zeros(self.n_pairs)
        self.known_bad = np.zeros(self.n_pairs, dtype=bool)
        self.nb_eff = {}
        self.rep_assign = self.bcol_assign = None
        if self.resample_rep:
            self.rep_assign = np.zeros((self.G, self.ng, self.num_boot), dtype=np.int16)
            self.bcol_assign = np.zeros((self.G, self.ng, self.num_boot), dtype=np.int32)

    def good_groups(self, gi):
        return ((~self.skip) & (self.bs.K >= 2) & ~self.known_bad)[gi * self.ng:(gi + 1) * self.ng]

    def gene_uses_resampling(self, gi, n_good):
        if not self.resample_rep or n_good == 0:
            return False
        return not (self.gene_trt[gi][self.good_groups(gi)] == 1).mean() == 1                        # hypothesis_test.py:262

    def draw_assignments(self, gi):
        n = int(self.good_groups(gi).sum())
        if self.gene_uses_resampling(gi, n):
            nb = self.nb_eff.get(gi, self.num_boot)                        # hypothesis_test.py:253
            if nb < 1:
                return
            ra = np.random.choice(n, size=(n, nb))                         # hypothesis_test.py:275-278
            ra[:, 0] = np.arange(n)
            ba = np.random.choice(nb, (n, nb)) + 1
            ba[:, 0] = 0
            self.rep_assign[gi, :n, :nb], self.bcol_assign[gi, :n, :nb] = ra, ba

    def draw_hash(self, lo_p, hi_p):
        """The two hash uniforms of the live pairs lo_p..hi_p."""
        idx = self.live[(self.live >= lo_p) & (self.live <= hi_p)]
        u = np.random.random(2 * len(idx))      # same stream positions as random(1) then random() per pair
        self.r1[idx], self.r0[idx] = u[0::2], u[1::2]

    def draw_stream(self, first, stop_pair=None, pending=None):
        """Consume the global np.random stream exactly as the reference does from pair ``first`` on: per gene the two
        hash uniforms of every live group (bootstrap.py:62,65) and -- with resample_rep -- the two np.random.choice
        draws of _regress_1d (hypothesis_test.py:275-278) after the gene's last group.  ``pending``: a gene whose
        groups are all done but whose choice draws are still due; ``stop_pair``: stop right after that pair's hash."""
        ng = self.ng
        if not self.resample_rep:
            self.draw_hash(first, self.n_pairs - 1 if stop_pair is None else stop_pair)
            return
        if pending is not None:
            self.draw_assignments(pending)
        for gi in range(int(first // ng), self.G):
            self.draw_hash(max(first, gi * ng), (gi + 1) * ng - 1 if stop_pair is None else min((gi + 1) * ng - 1, stop_pair))
            if stop_pair is not None and stop_pair < (gi + 1) * ng:
                return
            self.draw_assignments(gi)

    def replay_pass(self):
        """One sequential replay of the reference's global-stream consumption over all genes (speculate, then roll back to
        the first pair whose _fill draws -- or, under resample_rep, shrinking num_rep -- shift the stream)."""
        bs, skip, ng = self.bs, self.skip, self.ng
        n_inv_all = np.zeros((self.n_pairs, 2), dtype=np.int32)
        first, pending = 0, None
        while first < self.n_pairs:
            saved = np.random.get_state()
            self.draw_stream(first, pending=pending)
            after = np.random.get_state()
            n_inv = self.run_from(self.r1, self.r0, first_pair=first)
            n_inv_all[first:] = n_inv
            event = (n_inv > 0).any(axis=1)
            if self.resample_rep:
                event |= (n_inv < 0).any(axis=1) & ~self.known_bad[first:]      # a group without valid replicates shrinks num_rep
            needs = np.flatnonzero((~skip[first:]) & event) + first
            if len(needs) == 0:
                np.random.set_state(after)
                pending = None
                break
            p = int(needs[0])
            np.random.set_state(saved)
            self.draw_stream(first, stop_pair=p, pending=pending)                # everything the reference drew up to pair p's hash
            for t, col in ((bs.ym, 0), (bs.yv, 1)):
                if n_inv_all[p, col] > 0:
                    self.store(t, p, _host_fill(self.load(t, p)))
                    n_inv_all[p, col] = 0
            if (n_inv_all[p] < 0).any():
                self.known_bad[p] = True
            pending = p // ng if (self.resample_rep and p % ng == ng - 1) else None
            first = p + 1
        if pending is not None:
            self.draw_assignments(pending)
        bad_fill = (n_inv_all < 0).any(axis=1)
        self.known_bad |= bad_fill & ~skip      # (under resample_rep every such pair was an event above and is marked already)
        return bad_fill

    def run(self):
        stream0 = np.random.get_state()
        for _attempt in range(3):
            bad_fill = self.replay_pass()
            if not self.resample_rep:
                break
            # The reference draws a gene's assignments for the replicate columns that SURVIVE hypothesis_test.py:249-251,
            # which is known only after its bootstrap: when a resampled gene lost columns, replay once more with that count.
            good_now = ((~self.skip) & (self.bs.K >= 2) & ~bad_fill).reshape(self.G, self.ng)
            _, nv = self.bs.valid_cols(good_now)
            redo = False
            for gi in np.flatnonzero(nv != self.num_boot + 1):
                gi = int(gi)
                if self.gene_uses_resampling(gi, int(good_now[gi].sum())) and self.nb_eff.get(gi, self.num_boot) != int(nv[gi]) - 1:
                    self.nb_eff[gi] = int(nv[gi]) - 1
                    redo = True
            if not redo:
                break
            np.random.set_state(stream0)
            self.known_bad[:] = False
        return bad_fill
