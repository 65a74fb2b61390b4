"""Generate tests/golden/guide_loop_strata.npz by running the REAL reference's per-guide loop with a replicate covariate.

Run on a CPU machine with the reference set up as make_golden.py sets it up:  python tests/golden/make_strata_fixture.py
(the GPU tests read only the .npz).
The pattern of analysis/perturb_thp1 and analysis/cd4_cropseq on the current API: for every guide, subset to control + guide
cells, create_groups(['is_guide', 'rep']), compute_1d_moments, ht_1d_moments with covariate = intercept + rep dummies
(drop_first) and treatment = is_guide.  Guide 4 has no cells in replicate 2 (a missing stratum).  Fixture for the batched
ht_1d_vs_control(..., treatment_col='guide') with the label columns ['guide', 'rep'].
"""

import copy
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import memento, synth_adata  # noqa: E402  (memento: the reference, importable through make_golden's set-up)


def guide_loop_strata_case(name):
    from scrna_parameter_estimation_amd.anndata_lite import AnnDataLite

    n_guides, n_rep = 4, 3
    adata = synth_adata(7000, 120, 0.15, 1, n_rep, 231, dtype=np.float64)
    rng = np.random.default_rng(232)
    guide = rng.choice(n_guides + 1, size=adata.shape[0], p=np.r_[0.32, np.full(n_guides, 0.17)])
    rep = adata.obs["rep"].values.astype(np.int64)
    move = (guide == n_guides) & (rep == n_rep - 1)               # guide 4: no cells in the last replicate
    rep = rep.copy()
    rep[move] = rng.integers(0, n_rep - 1, size=int(move.sum()))
    adata.obs["rep"] = rep
    adata.obs["guide"] = guide
    inp = dict(indptr=adata.X.indptr.copy(), indices=adata.X.indices.copy(), data=adata.X.data.copy(), shape=np.array(adata.X.shape),
               guide=guide.astype(np.int64), rep=rep, q=adata.obs["q"].values.copy(), gene_names=np.array(adata.var.index.tolist()))
    memento.setup_memento(adata, q_column="q")
    out = {"size_factor": adata.obs["memento_size_factor"].values.copy(), "n_guides": np.int64(n_guides)}
    for gid in range(1, n_guides + 1):
        rows = np.flatnonzero((guide == 0) | (guide == gid))
        sub = AnnDataLite(adata.X[rows].tocsr(), adata.obs.iloc[rows].copy(), adata.var.copy(), copy.deepcopy(adata.uns))
        sub.obs["is_guide"] = (sub.obs["guide"].values == gid).astype(int)
        memento.create_groups(sub, label_columns=["is_guide", "rep"])
        memento.compute_1d_moments(sub, min_perc_group=0.9)
        gdf = memento.get_groups(sub)
        cov = pd.concat([pd.DataFrame({"intercept": np.ones(len(gdf))}, index=gdf.index),
                         pd.get_dummies(gdf["rep"].astype(str), prefix="rep", drop_first=True).astype(float)], axis=1)
        trt = pd.DataFrame({"is_guide": gdf["is_guide"].astype(float).values}, index=gdf.index)
        np.random.seed(240 + gid)
        memento.ht_1d_moments(sub, covariate=cov, treatment=trt, num_boot=400, num_cpus=1, verbose=0, resampling="bootstrap", approx=True)
        m = sub.uns["memento"]
        ht = m["1d_ht"]
        out[f"g{gid}_genes"] = np.array(sub.var.index.tolist())
        out[f"g{gid}_groups"] = np.array([f"{a}^{b}" for a, b in zip(gdf["is_guide"], gdf["rep"])])
        # per-group moments of the subset's kept genes: which groups the reference could use for each test
        out[f"g{gid}_mean"] = np.stack([np.asarray(m["1d_moments"][k][0]) for k in m["groups"]])
        out[f"g{gid}_rv"] = np.stack([np.asarray(m["1d_moments"][k][2]) for k in m["groups"]])
        for k in ["mean_coef", "mean_se", "mean_asl", "var_coef", "var_se", "var_asl"]:
            out[f"g{gid}_{k}"] = np.asarray(ht[k]).copy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **{("in_" + k): v for k, v in inp.items()}, **out)
    print(name, [(len(out[f"g{g}_genes"]), out[f"g{g}_groups"].tolist(), int(np.isnan(out[f"g{g}_mean_asl"]).sum()))
                 for g in range(1, n_guides + 1)])


if __name__ == "__main__":
    guide_loop_strata_case("guide_loop_strata")
