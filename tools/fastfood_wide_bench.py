#!/usr/bin/env python3
"""FastFoodRBF on wide inputs (256 < Xdim <= 4096): the chain kernel (rr_fastfood64_kernel) against the dense-equivalent route
(W = _makeVX(I_d) through the random Fourier feature kernels' wide-input GEMM path), float32, device-resident, HIP-event
timed, arms alternating on one GPU.  The roofline of the chain is the HBM write of Phi, 8 n bytes per row.

    python tools/fastfood_wide_bench.py [--elbo]

Shapes (d, n): (512, 4096), (1024, 4096), (2048, 8192), (4096, 16384); 262 144 rows, timed in calls of at most 8 GiB of Phi.
--elbo adds a resident StandardLinearModel._elbo at d = 1024, F = 8192 (65 536 rows), chain against RR_FASTFOOD_FIT=dense.
"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from revrand_amd import _hip  # noqa: E402
from revrand_amd.basis_functions import FastFoodRBF  # noqa: E402

HBM_TBS = 8.0
N_TOTAL = 262144
SHAPES = [(512, 4096), (1024, 4096), (2048, 8192), (4096, 16384)]
REPS = 3


def features(shape):
    d, n = shape
    F = 2 * n
    rows = int(min(N_TOTAL, (8 << 30) // (F * 4)))
    X = np.random.RandomState(0).randn(rows, d).astype(np.float32)
    b = FastFoodRBF(nbases=n, Xdim=d, random_state=1)
    ff, lazy = b._handles()
    rff = lazy.get()
    dev = rff.dev
    dXp = rff.upload(X)               # the dense handle's padded layout
    dX = dev.upload_matrix(X)         # plain rows for the chain
    out = dev.malloc(rows * F * 4)
    ls = np.array([1.3])
    lsp = ls.ctypes.data_as(ctypes.c_void_p)
    best = {"chain": 1e30, "dense": 1e30}
    for rep in range(REPS + 1):       # (the first round warms both arms up)
        for arm in ("chain", "dense"):
            dev.timer_start()
            if arm == "chain":
                ff.transform_dev(dX, ls, out, out_dtype=np.float32, ldphi=F)
            else:
                _hip._check(dev.lib, dev.lib.rr_rff_transform_dev(rff.h, dXp.ptr, 0, rows, dXp.ld, lsp, 1, out.ptr, 0, F))
            ms = dev.timer_stop()
            if rep:
                best[arm] = min(best[arm], ms)
    Pc = None
    for arm in ("chain", "dense"):    # the two arms compute the same features
        if arm == "chain":
            ff.transform_dev(dX, ls, out, out_dtype=np.float32, ldphi=F)
        else:
            _hip._check(dev.lib, dev.lib.rr_rff_transform_dev(rff.h, dXp.ptr, 0, rows, dXp.ld, lsp, 1, out.ptr, 0, F))
        dev.sync()
        P = dev.download(out, (64, F), np.float32)
        Pc = P if Pc is None else Pc
    diff = float(np.abs(P - Pc).max() * np.sqrt(n))
    for arm in ("chain", "dense"):
        ms = best[arm]
        tbs = rows * F * 4 / ms / 1e9
        print("d=%-5d n=%-6d %-5s rows/call=%-7d %8.3f ms  %7.2f M rows/s  %5.2f TB/s of Phi (%4.1f%% of %.0f TB/s)" % (
            d, n, arm, rows, ms, rows / ms / 1e3, tbs, tbs / HBM_TBS * 100, HBM_TBS))
    print("d=%-5d n=%-6d chain / dense speed ratio %.2f;  max |chain - dense| sqrt(n) on 64 rows %.2e" % (
        d, n, best["dense"] / best["chain"], diff))
    for buf in (dXp, dX, out):
        buf.free()


def elbo():
    from revrand_amd.slm import StandardLinearModel
    N, d, n = 65536, 1024, 4096
    rs = np.random.RandomState(1)
    X = rs.randn(N, d).astype(np.float32)
    y = np.sin(X @ rs.randn(d) / np.sqrt(d)).astype(np.float32)
    f = FastFoodRBF(nbases=n, Xdim=d, random_state=1)
    best = {"chain": 1e30, "dense": 1e30}
    states = {}
    for route in ("chain", "dense"):
        os.environ["RR_FASTFOOD_FIT"] = route
        slm = StandardLinearModel(f)
        slm.obj_ = -np.inf
        slm._state = slm._make_state(X, y)
        states[route] = slm
    for rep in range(REPS + 1):
        for route, slm in states.items():
            os.environ["RR_FASTFOOD_FIT"] = route
            t0 = time.perf_counter()
            slm._elbo(X, y, 0.3, 1.5, 1.2 + 0.01 * rep)
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                best[route] = min(best[route], dt)
    for route, slm in states.items():
        slm._state.release()
        print("resident _elbo N=%d d=%d F=%d  %-5s (%s) %9.2f ms" % (N, d, 2 * n, route, type(slm._state).__name__, best[route]))
    print("resident _elbo chain / dense speed ratio %.2f" % (best["dense"] / best["chain"]))


if __name__ == "__main__":
    for shape in SHAPES:
        features(shape)
    if "--elbo" in sys.argv:
        elbo()
