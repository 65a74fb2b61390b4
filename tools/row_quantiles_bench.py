"""mm_row_quantiles alone, next to what a user had before it: HIP-event time of the launch on 20,000 coefficient rows x
num_boot = 10,000 with 2 probabilities (the interval of ci=0.95), and engine.host(rows) + np.nanquantile on the same rows;
the two results are compared.  Then the same rows with 5 % NaN (dropped replicates), where numpy goes row by row.

    python tools/row_quantiles_bench.py [--rows 20000] [--num-boot 10000] [--out FILE]    (profiles/row_quantiles.txt)"""

import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from scrna_parameter_estimation_amd import engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=20_000)
ap.add_argument("--num-boot", type=int, default=10_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
n_rows, B = args.rows, args.num_boot
ld = B + 1
probs = [0.025, 0.975]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def launch_ms(tag, t):
    """7 timed launches after 2 warm-ups; -> the last launch's (q, n_valid) on the host."""
    pr = (ctypes.c_double * len(probs))(*probs)
    q = torch.empty((n_rows, len(probs)), dtype=torch.float64, device="cuda")
    nv = torch.empty((n_rows,), dtype=torch.int32, device="cuda")
    ms = []
    for i in range(9):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        engine._lib.call("mm_row_quantiles", engine.P(t), n_rows, ld, B, pr, len(probs), engine.P(q), engine.P(nv), engine._stream())
        e1.record()
        e1.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    say(f"mm_row_quantiles, {tag}: HIP-event ms per launch, 7 launches after 2 warm-ups: " + " ".join(f"{x:.2f}" for x in ms)
        + f"  (median {med:.2f} ms; 8 reads of {n_rows * B * 8 / 1e9:.2f} GB = {8 * n_rows * B * 8 / 1e9 / (med / 1e3):.0f} GB/s)")
    return engine.host(q), engine.host(nv)


def host_alternative(tag, t, sub):
    t0 = time.perf_counter()
    h = engine.host(t)
    t1 = time.perf_counter()
    want = np.nanquantile(h[:sub, 1:B + 1], probs, axis=1, method="linear").T
    t2 = time.perf_counter()
    scale = "" if sub == n_rows else f" on the first {sub} rows (x {n_rows / sub:g} for all rows: {(t2 - t1) * n_rows / sub:.2f} s)"
    say(f"host alternative, {tag}: engine.host(rows) {t1 - t0:.2f} s + np.nanquantile(axis=1) {t2 - t1:.2f} s{scale}")
    return want


g = torch.Generator(device="cuda").manual_seed(1)
rows = torch.randn((n_rows, ld), dtype=torch.float64, device="cuda", generator=g) * 0.3 + 0.1
say(f"device: {torch.cuda.get_device_name(0)}")
say(f"rows: {n_rows} x (num_boot = {B}, ld = {ld}) fp64 = {rows.numel() * 8 / 1e9:.2f} GB, probs = {probs}")
q, nv = launch_ms("no NaN", rows)
want = host_alternative("no NaN", rows, n_rows)
say(f"agreement with np.nanquantile: max relative difference {(np.abs(q - want) / np.abs(want)).max():.3g}, bit-equal "
    f"{int((q == want).sum())} of {q.size}; n_valid == num_boot in every row: {bool((nv == B).all())}")
rows[torch.rand((n_rows, ld), device="cuda", generator=g) < 0.05] = float("nan")
q, nv = launch_ms("5 % NaN", rows)
sub = max(1, n_rows // 10)
want = host_alternative("5 % NaN", rows, sub)
say(f"agreement with np.nanquantile on those rows: max relative difference {(np.abs(q[:sub] - want) / np.abs(want)).max():.3g}, "
    f"bit-equal {int((q[:sub] == want).sum())} of {want.size}")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
