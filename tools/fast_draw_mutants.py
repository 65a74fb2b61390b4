"""How much the (n, p) sweep of tests/test_gpu_sampler_sweep.py can see -- host only, recorded in profiles/fast_draw_tests.txt.

Builds tests/host_shim/npy_rng_host.cpp (the product's csrc/npy_rng.h for the host) with one guard of the fp32 fast paths
switched off at a time, runs the sweep's 8,192 chains x 64 streams through the sampler forms the kernels run, and counts the draws
that then differ from numpy's.  A guard that can be switched off without a single difference is one the sweep does not prove
necessary (it still proves that the guarded paths agree).  Each mutant runs with the host's correctly rounded primitives and with
-DNPY_HOST_PERTURB (every cheap primitive carrying 2-4x the error of the hardware instruction it maps to).

    python tools/fast_draw_mutants.py [S]"""

import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _fast_ref import SWEEP_B, SWEEP_KEY0, SWEEP_SEED, fast_state, fast_weights_many, sweep_mults, sweep_regimes   # noqa: E402

INV_OFF = ["-DNPY_INV_G0=0.0f", "-DNPY_INV_GA=0.0f", "-DNPY_INV_GX=0.0f", "-DNPY_INV_GS=0.0f"]
MUTANTS = [("none", [], ["host_multinomial_fast", "host_multinomial_capped", "host_multinomial_async", "host_multinomial_async_bf"]),
           ("NPY_INV_G0 = GA = GX = GS = 0 (guard of the fp32 inversion search)", INV_OFF, ["host_multinomial_fast", "host_multinomial_capped"]),
           ("NPY_INV_GUARD = 0 (constant inversion guard of the resumable forms)", ["-DNPY_INV_GUARD=0.0f"],
            ["host_multinomial_async", "host_multinomial_async_bf"]),
           ("NPY_F_GUARD = 0 (guard of the fp32 explicit product of BTPE)", ["-DNPY_F_GUARD=0.0f"],
            ["host_multinomial_fast", "host_multinomial_capped", "host_multinomial_async", "host_multinomial_async_bf"])]


def build(tmp, flags):
    out = os.path.join(tmp, "shim_%d.so" % abs(hash(tuple(flags))))
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "scrna_parameter_estimation_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_shim", "npy_rng_host.cpp"), "-o", out] + flags)
    return ctypes.CDLL(out)


def run(lib, fn, mults, words):
    S, B = words.shape[:2]
    out = np.zeros((S, B, 3), dtype=np.int64)
    f = getattr(lib, fn)
    f.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    w0, o0 = words.ctypes.data, out.ctypes.data
    for s in range(S):
        N = int(mults[s].sum())
        pv = np.ascontiguousarray(mults[s] / np.float64(N))
        p = pv.ctypes.data
        for r in range(B):
            f(w0 + 32 * (s * B + r), N, p, 3, 1, o0 + 24 * (s * B + r))
    return out.transpose(0, 2, 1)


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    mults = sweep_mults(S)
    reps = np.arange(SWEEP_B)
    t0 = time.time()
    want = fast_weights_many(mults, SWEEP_SEED, SWEEP_KEY0 + np.arange(S), reps)
    t_ref = time.time() - t0
    words = np.ascontiguousarray(np.stack(fast_state(SWEEP_SEED, (SWEEP_KEY0 + np.arange(S, dtype=np.int64))[:, None], reps[None, :]), axis=2))
    reg = sweep_regimes(mults, want)
    n_draws = reg.inversion + reg.btpe
    print(f"sweep: {S} chains x {SWEEP_B} streams, {n_draws} binomial draws; numpy reference {t_ref:.1f} s on this host")
    print("regimes: " + ", ".join(f"{k} {v}" for k, v in vars(reg).items()))
    with tempfile.TemporaryDirectory() as tmp:
        for name, flags, fns in MUTANTS:
            for perturb in (False, True):
                lib = build(tmp, flags + (["-DNPY_HOST_PERTURB"] if perturb else []))
                for fn in fns:
                    got = run(lib, fn, mults, words)
                    first = got[:, 0] != want[:, 0]                        # the first draw differs
                    second = ~first & (got[:, 1] != want[:, 1])            # the first is numpy's, the second differs
                    fb = (ctypes.c_long * 2)()
                    lib.host_fallback_counts(fb, 1)
                    print(f"guard off: {name}; primitives {'perturbed' if perturb else 'exact'}; {fn}: {int(first.sum() + second.sum())} of {n_draws} "
                          f"draws differ from numpy's ({int(first.sum())} first draws, {int(second.sum())} second draws; "
                          f"fallbacks to exact arithmetic: inversion {fb[0]}, explicit product {fb[1]})", flush=True)


if __name__ == "__main__":
    main()
