#!/usr/bin/env python3
"""Kernel times of the centre bases' device kernels (docs/KERNELS.md, "Centre bases"): one JSON line.

    python tools/centres_bench.py [--rows 1000000] [--dim 21] [--centres 256,1024,4096] [--host-rows 20000]
                                  [--f64-rows 20000,100000] [--f64-centres 512] [--f64-reps 3] [--f64-only]
                                  [--no-host-route] [--no-f64] [--wide] [--wide-rows 3000] [--wide-reps 3]

* put_centres:   rr_featmat_put_centres (RadialBasis) into a feature matrix of M columns;
* pass2_centres: rr_featmat_pass2_centres after one rr_featmat_pass2_rows, isotropic and ARD length scales;
each the median of 5 launches after 2 warm-up launches, timed with the context's events (rr_timer_*), so the number is the
kernel(s) on an otherwise idle stream, launch overhead included.  With them the per-row work counts of docs/KERNELS.md as
rates: bytes written per second for the features, VALU flop per second for both.
* host_route_s: for orientation, the wall time of the reference-style host route -- scipy's cdist + exp in float64 and
  rr_featmat_put_host of the result -- measured on --host-rows rows and scaled to --rows (cdist is linear in rows).
* "f64": for every N of --f64-rows, one full StandardLinearModel._elbo of RadialBasis(dtype="f64") with ARD length scales
  (--dim, --f64-centres) -- wall time, the median of --f64-reps evaluations after one warm-up evaluation -- on the host route
  (resident_bases="fourier": transform / grad / one SYRK of [Phi | dPhi_i] per length scale) and on the float64 resident route
  (resident_bases="all"), in this process one after the other, with their ratio; and the kernel times (events, as above) of
  rr_featmat64_put_centres, rr_featmat64_put_poly (order 3 with bias) and rr_featmat64_pass2_centres (isotropic and ARD) at
  that N.
* --dim above 128 (up to 4096) times the dimension-blocked kernels (docs/KERNELS.md 3.38); --no-host-route / --no-f64 leave
  the host-route and "f64" parts out of such a run.
* --wide: only the "wide" block.  "yardstick": put_centres (isotropic, M = 1024, N = 1 000 000 * 21 / d rows, so that every d
  does the same number of (row, centre, dimension) terms) at d = 128 -- the unchanged narrow kernel -- then 256, then 128
  again, 1024, 128 again: picoseconds per term, each d's ratio to the median d = 128 figure, and the spread (max / min - 1) of
  the three d = 128 measurements.  "elbo": wall time of one StandardLinearModel._elbo of an ARD RadialBasis, d = 256, M = 512,
  --wide-rows rows (3000: the default route's (N, M, d) float64 gradient is 3.1 GB), resident_bases="all" and the default
  route evaluated alternately in one process, the median of --wide-reps each after one warm-up evaluation each.
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


def elbo_seconds(SLM, basis, X, y, hyp, resident_bases, reps):
    """Median wall time of one full `_elbo` (after one warm-up evaluation) on the route `resident_bases` gives."""
    slm = SLM(basis, resident_bases=resident_bases)
    slm.obj_ = -np.inf
    slm._state = slm._make_state(X, y)
    resident = slm._state is not None
    try:
        ts = []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            f, _ = slm._elbo(X, y, 0.5, 1.0, hyp)
            ts.append(time.perf_counter() - t0)
    finally:
        if slm._state is not None:
            slm._state.release()
            slm._state = None
    return float(np.median(ts[1:])), resident, float(f)


def f64_section(a, dev):
    from revrand_amd.slm import StandardLinearModel as SLM
    d, M = a.dim, a.f64_centres
    rs = np.random.RandomState(1)
    C = rs.randn(M, d)
    ard = np.linspace(2.0, 2.6, d)   # features of order one at d = 21
    rows = []
    for N in [int(v) for v in a.f64_rows.split(",") if v]:
        X = rs.randn(N, d)
        y = np.sin(X[:, 0] - X[:, 1]) + 0.1 * rs.randn(N)
        row = {"N": N, "M": M, "dim": d}

        def mk():
            return RadialBasis(centres=C, lenscale=Parameter(np.ones(d), Positive()), dtype="f64")
        resident_s, was_resident, f_res = elbo_seconds(SLM, mk(), X, y, ard, "all", a.f64_reps)
        host_s, not_host, f_host = elbo_seconds(SLM, mk(), X, y, ard, "fourier", a.f64_reps)
        assert was_resident and not not_host
        row.update(elbo_host_s=host_s, elbo_resident_s=resident_s, host_over_resident=host_s / resident_s,
                   elbo_rel_diff=abs(f_res - f_host) / abs(f_host))
        # the three kernels on their own
        h = mk()._handle()
        dX, dy = dev.upload_matrix(X), dev.upload_vector(y)
        fm = _hip.FeatureMatrix64(N, M)

        def put(ls):
            fm.begin(N)   # (clears the claimed column spans; its padding fill is outside the timed region)
            dev.timer_start()
            fm.put_centres(h, dX, ls, 0)
            return dev.timer_stop()
        for _ in range(2):
            put(ard)
        row["put_centres64_ms"] = float(np.median([put(ard) for _ in range(5)]))
        row["put64_write_GBps"] = 8.0 * M * N / row["put_centres64_ms"] / 1e6
        A = rs.randn(M, M) / np.sqrt(M)
        fm.pass2_begin(0.1 * rs.randn(M), A @ A.T + np.eye(M))
        dg = dev.zeros(d * 8)
        for tag, ls in (("iso", np.array([2.3])), ("ard", ard)):
            put(ls)
            fm.pass2_rows(dy)
            row["pass2_centres64_%s_ms" % tag] = timed(dev, lambda: fm.pass2_centres(h, dX, 0, dg))
        fm.pass2_end()
        row["pass2_64_ard_valu_Gflops"] = 4.0 * d * M * N / row["pass2_centres64_ard_ms"] / 1e6
        del fm
        W = 1 + 3 * d
        fmp = _hip.FeatureMatrix64(N, W)

        def put_poly():
            fmp.begin(N)
            dev.timer_start()
            fmp.put_poly(dX, 3, True, 0)
            return dev.timer_stop()
        for _ in range(2):
            put_poly()
        row["put_poly64_ms"] = float(np.median([put_poly() for _ in range(5)]))
        del fmp
        for buf in (dX, dy, dg):
            buf.free()
        rows.append(row)
    return rows


def wide_section(a, dev):
    from revrand_amd.slm import StandardLinearModel as SLM
    rs = np.random.RandomState(2)
    M = 1024
    runs = []
    for d in (128, 256, 128, 1024, 128):
        N = 1000000 * 21 // d
        X = rs.randn(N, d).astype(np.float32)
        dX = dev.upload_matrix(X)
        h = RadialBasis(centres=rs.randn(M, d))._handle()
        fm = _hip.FeatureMatrix(N, M)
        ls = np.array([1.1 * d ** 0.25])

        def put():
            fm.begin(N)   # (clears the claimed column spans; its padding fill is outside the timed region)
            dev.timer_start()
            fm.put_centres(h, dX, ls, 0)
            return dev.timer_stop()
        for _ in range(2):
            put()
        ms = float(np.median([put() for _ in range(5)]))
        runs.append({"dim": d, "rows": N, "M": M, "put_centres_ms": ms, "ps_per_term": ms * 1e9 / (float(N) * M * d)})
        del fm
        dX.free()
    base = [r["ps_per_term"] for r in runs if r["dim"] == 128]
    ref = float(np.median(base))
    for r in runs:
        r["over_d128"] = r["ps_per_term"] / ref
    out = {"yardstick": runs, "d128_spread": max(base) / min(base) - 1.0}
    # one _elbo on either route
    d, M, N = 256, 512, a.wide_rows
    X, C = rs.randn(N, d), rs.randn(M, d)
    y = np.sin(X[:, 0] - X[:, 1]) + 0.1 * rs.randn(N)
    hyp = 1.1 * d ** 0.25 * np.linspace(0.8, 1.3, d)
    slms = {}
    for rb in ("all", "fourier"):
        slm = SLM(RadialBasis(centres=C, lenscale=Parameter(np.ones(d), Positive())), resident_bases=rb)
        slm.obj_ = -np.inf
        slm._state = slm._make_state(X, y)
        assert (slm._state is not None) == (rb == "all")
        slms[rb] = slm
    ts, f = {"all": [], "fourier": []}, {}
    try:
        for k in range(a.wide_reps + 1):
            for rb in ("all", "fourier"):   # alternately
                t0 = time.perf_counter()
                f[rb], _ = slms[rb]._elbo(X, y, 0.5, 1.0, hyp)
                ts[rb].append(time.perf_counter() - t0)
    finally:
        slms["all"]._state.release()
        slms["all"]._state = None
    res, host = float(np.median(ts["all"][1:])), float(np.median(ts["fourier"][1:]))
    out["elbo"] = {"N": N, "M": M, "dim": d, "default_tensor_GB": 8.0 * N * M * d / 1e9, "elbo_resident_s": res,
                   "elbo_default_s": host, "default_over_resident": host / res,
                   "elbo_rel_diff": abs(float(f["all"]) - float(f["fourier"])) / abs(float(f["fourier"]))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=21)
    ap.add_argument("--centres", default="256,1024,4096")
    ap.add_argument("--host-rows", type=int, default=20000)
    ap.add_argument("--f64-rows", default="20000,100000")
    ap.add_argument("--f64-centres", type=int, default=512)
    ap.add_argument("--f64-reps", type=int, default=3)
    ap.add_argument("--f64-only", action="store_true")
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--no-f64", action="store_true")
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--wide-rows", type=int, default=3000)
    ap.add_argument("--wide-reps", type=int, default=3)
    a = ap.parse_args()
    N, d = a.rows, a.dim
    dev = _hip.get_device()
    if a.f64_only:
        print(json.dumps({"dim": d, "device": dev.name, "f64": f64_section(a, dev)}))
        return
    if a.wide:
        print(json.dumps({"device": dev.name, "wide": wide_section(a, dev)}))
        return
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
        if not a.no_host_route:   # the reference-style host route on a row subset
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
            del fmh
        del fm
        dg.free()
        out["shapes"].append(row)
    dX.free()
    dy.free()
    if not a.no_f64:
        out["f64"] = f64_section(a, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
