#!/usr/bin/env python3
"""Kernel times of the centre bases' device kernels (docs/KERNELS.md, "Centre bases"): one JSON line.

    python tools/centres_bench.py [--rows 1000000] [--dim 21] [--centres 256,1024,4096] [--host-rows 20000]

* put_centres:   rr_featmat_put_centres (RadialBasis) into a feature matrix of M columns;
* pass2_centres: rr_featmat_pass2_centres after one rr_featmat_pass2_rows, isotropic and ARD length scales;
each the median of 5 launches after 2 warm-up launches, timed with the context's events (rr_timer_*), so the number is the
kernel(s) on an otherwise idle stream, launch overhead included.  With them the per-row work counts of docs/KERNELS.md as
rates: bytes written per second for the features, VALU flop per second for both.
* host_route_s: for orientation, the wall time of the reference-style host route -- scipy's cdist + exp in float64 and
  rr_featmat_put_host of the result -- measured on --host-rows rows and scaled to --rows (cdist is linear in rows).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from revrand_amd import _hip  # noqa: E402
from revrand_amd.basis_functions import RadialBasis  # noqa: E402
from revrand_amd.btypes import Parameter, Positive  # noqa: E402


def timed(dev, fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        dev.timer_start()
        fn()
        ms.append(dev.timer_stop())
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=21)
    ap.add_argument("--centres", default="256,1024,4096")
    ap.add_argument("--host-rows", type=int, default=20000)
    a = ap.parse_args()
    N, d = a.rows, a.dim
    dev = _hip.get_device()
    rs = np.random.RandomState(0)
    X = rs.randn(N, d).astype(np.float32)
    y = rs.randn(N).astype(np.float32)
    dX, dy = dev.upload_matrix(X), dev.upload_vector(y)
    iso, ard = np.array([1.8]), np.linspace(1.5, 2.1, d)
    out = {"rows": N, "dim": d, "device": dev.name, "shapes": []}
    for M in [int(v) for v in a.centres.split(",")]:
        C = rs.randn(M, d)
        basis = RadialBasis(centres=C, lenscale=Parameter(np.ones(d), Positive()))
        h = basis._handle()
        fm = _hip.FeatureMatrix(N, M)
        fm.begin(N)
        row = {"M": M}

        def put(ls=iso):
            fm.begin(N)   # (clears the claimed column spans; its padding fill is outside the timed region below)
            dev.timer_start()
            fm.put_centres(h, dX, ls, 0)
            return dev.timer_stop()
        for _ in range(2):
            put()
        row["put_centres_ms"] = float(np.median([put() for _ in range(5)]))
        row["put_write_GBps"] = 4.0 * M * N / row["put_centres_ms"] / 1e6
        row["put_valu_Gflops"] = 3.0 * d * M * N / row["put_centres_ms"] / 1e6
        A = rs.randn(M, M) / np.sqrt(M)
        fm.pass2_begin(0.1 * rs.randn(M), A @ A.T + np.eye(M))
        dg = dev.zeros(d * 8)
        for tag, ls in (("iso", iso), ("ard", ard)):
            put(ls)
            fm.pass2_rows(dy)
            row["pass2_centres_%s_ms" % tag] = timed(dev, lambda: fm.pass2_centres(h, dX, 0, dg))
        row["pass2_ard_read_GBps"] = 8.0 * M * N / row["pass2_centres_ard_ms"] / 1e6
        row["pass2_ard_valu_Gflops"] = 4.0 * d * M * N / row["pass2_centres_ard_ms"] / 1e6
        fm.pass2_end()
        # the reference-style host route on a row subset
        from scipy.spatial.distance import cdist
        n = min(a.host_rows, N)
        Xh = X[:n].astype(np.float64)
        fmh = _hip.FeatureMatrix(n, M)
        fmh.begin(n)
        t0 = time.perf_counter()
        den = 2 * iso ** 2
        Phi = np.exp(-cdist(Xh / den, C / den, "sqeuclidean"))
        fmh.put_host(Phi, 0)
        dev.sync()
        row["host_route_s"] = (time.perf_counter() - t0) * N / n
        row["host_route_measured_rows"] = n
        del fmh, fm
        dg.free()
        out["shapes"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
