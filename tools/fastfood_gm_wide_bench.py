#!/usr/bin/env python3
"""FastFoodGM on wide inputs (256 < Xdim <= 4096, wide_chain=True): the mixture mode of the wide chain kernel
(rr_fastfood64_kernel<..., GM>) next to the wide FastFoodRBF chain at the same (d, n) -- float32, device-resident x and Phi,
HIP-event timed, arms alternating on one GPU, best of three after a warm-up round.  The mixture mode writes 16 n bytes of Phi
per row (FastFoodRBF: 8 n) and evaluates twice the sines, so twice the RBF arm's time per row is the expectation.  There is no
dense arm: the dense route ends at 128 columns.

    python tools/fastfood_gm_wide_bench.py [--elbo]

Shapes (d, n): (512, 4096), (1024, 4096), (2048, 8192), (4096, 16384); at most 262 144 rows, timed in calls of at most 8 GiB of
Phi.  --elbo adds one resident StandardLinearModel._elbo at N = 65 536, d = 1024, n = 2048 (F = 8192).
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from revrand_amd.basis_functions import FastFoodGM, FastFoodRBF  # noqa: E402

HBM_TBS = 8.0
N_TOTAL = 262144
SHAPES = [(512, 4096), (1024, 4096), (2048, 8192), (4096, 16384)]
REPS = 3


def features(shape):
    d, n = shape
    rows = int(min(N_TOTAL, (8 << 30) // (4 * n * 4)))  # (the same rows for both arms: 8 GiB of the mixture's Phi at most)
    rs = np.random.RandomState(0)
    X = rs.randn(rows, d).astype(np.float32)
    mean = 0.3 * rs.randn(d)
    ls = np.linspace(0.7, 1.6, d)
    gm = FastFoodGM(nbases=n, Xdim=d, random_state=1, wide_chain=True)
    rbf = FastFoodRBF(nbases=n, Xdim=d, random_state=1)
    fg, fr = gm._handles()[0], rbf._handles()[0]
    assert fg.wide_gm and fg.n == fr.n == n
    dev = fg.dev
    dX = dev.upload_matrix(X)
    out = dev.malloc(rows * 4 * n * 4)
    run = {"gm": lambda: fg.gm_transform_dev(dX, mean, ls, out, out_dtype=np.float32, ldphi=4 * n),
           "rbf": lambda: fr.transform_dev(dX, ls, out, out_dtype=np.float32, ldphi=2 * n)}
    best = {"gm": 1e30, "rbf": 1e30}
    for rep in range(REPS + 1):       # (the first round warms both arms up)
        for arm in ("gm", "rbf"):
            dev.timer_start()
            run[arm]()
            ms = dev.timer_stop()
            if rep:
                best[arm] = min(best[arm], ms)
    for arm, width in (("gm", 4 * n), ("rbf", 2 * n)):
        ms = best[arm]
        tbs = rows * width * 4 / ms / 1e9
        print("d=%-5d n=%-6d %-4s rows/call=%-7d %8.3f ms  %7.2f M rows/s  %5.2f TB/s of Phi (%4.1f%% of %.0f TB/s)" % (
            d, n, arm, rows, ms, rows / ms / 1e3, tbs, tbs / HBM_TBS * 100, HBM_TBS))
    print("d=%-5d n=%-6d GM / RBF time ratio %.2f" % (d, n, best["gm"] / best["rbf"]))
    for buf in (dX, out):
        buf.free()


def elbo():
    from revrand_amd.slm import StandardLinearModel
    N, d, n = 65536, 1024, 2048
    rs = np.random.RandomState(1)
    X = rs.randn(N, d).astype(np.float32)
    y = np.sin(X @ rs.randn(d) / np.sqrt(d)).astype(np.float32)
    f = FastFoodGM(nbases=n, Xdim=d, random_state=1, wide_chain=True)
    mean, ls = 0.3 * rs.randn(d) / np.sqrt(d), np.linspace(0.8, 1.4, d)
    slm = StandardLinearModel(f)
    slm.obj_ = -np.inf
    slm._state = slm._make_state(X, y)
    best = 1e30
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        slm._elbo(X, y, 0.3, 1.5, [mean, ls + 0.01 * rep])
        dt = (time.perf_counter() - t0) * 1e3
        if rep:
            best = min(best, dt)
    name = type(slm._state).__name__
    slm._state.release()
    print("resident _elbo N=%d d=%d F=%d (%s) %9.2f ms" % (N, d, 4 * n, name, best))


if __name__ == "__main__":
    for shape in SHAPES:
        features(shape)
    if "--elbo" in sys.argv:
        elbo()
