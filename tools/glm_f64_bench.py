#!/usr/bin/env python
"""The float64 GLM SVI step at bench.py config 5's shape, next to the f32 step in the same session.

N = 2M resident rows, d = 32, RandomRBF n = 1024 (F = 2048, ARD), K = 10, L = 50, minibatch 65 536, Poisson, host sampler.
Per route: ms per `_elbo` step (host work included) and ms per step of the device calls alone (feature assembly, the step,
the length scales' contraction), TFLOP/s over the three GEMMs' 3 * 2 * K * L * M * F flops, and for float64 the fraction
of the 78.6 TFLOP/s f64 MFMA peak.  Routes, in this order: f64, f32, f64 with RR_GLM64_KSLABS=1 (the Ed product's k-loop in
one slab), f64 again (the first session of a process runs slower: where its buffers land).  One process, one line of JSON.

    python tools/glm_f64_bench.py [--rows 2000000] [--reps 8] [--timeout 500]

The whole run is bounded by --timeout seconds (the process dumps its stacks and exits); nothing is retried."""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F64_PEAK = 78.6e12


def session(dev, X, y, dtype, reps, N, d, n, K, L, M):
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd.btypes import Parameter, Positive
    from revrand_amd.glm import GeneralizedLinearModel
    F = 2 * n
    rs = np.random.RandomState(0)
    m = 0.1 * rs.randn(F, K)
    C = rs.gamma(2., 0.5, size=(F, K))
    ls = np.linspace(0.8, 1.5, d)
    basis = bs.RandomRBF(nbases=n, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()))
    glm = GeneralizedLinearModel(lk.Poisson(), basis, K=K, nsamples=L, batch_size=M, random_state=2, dtype=dtype)
    glm.B_, glm.D_ = N / M, F
    glm._GeneralizedLinearModel__it = 1   # a plain SGD iteration (no ELBO logging)
    feats = glm._features()
    glm._resident_fit = feats.make_resident(X)
    assert glm._resident_fit
    perm = rs.permutation(N)
    Xstub = np.empty((M, 0))
    out = {}
    try:
        def step(i):
            idx = perm[(i * M) % (N - M):(i * M) % (N - M) + M]
            return glm._elbo(m, C, 1.0, [], ls, Xstub, y[idx], idx)
        step(0)
        dev.sync()
        t0 = time.perf_counter()
        for i in range(reps):
            step(i + 1)
        dev.sync()
        out["elbo_step_ms"] = 1e3 * (time.perf_counter() - t0) / reps
        idx = perm[:M]
        E = rs.standard_normal((K * L, F))
        Edev = None
        if dtype == "f32":   # as `fit`'s worker leaves them: device-resident float32 draws
            E = E.astype(np.float32)
            Edev = dev.upload_vector(E.ravel())
            Edev.shape, Edev.dtype = E.shape, E.dtype

        def device_calls():
            feats.assemble_idx(idx, [ls])
            feats.glm_step_draws(y[idx], None, lk.RR_LIK_POISSON_EXP, 0.0, m, C, K, L, E if Edev is None else Edev)
            feats.glm_basis_grads(Xstub)
        for _ in range(3):
            device_calls()
        dev.sync()
        t0 = time.perf_counter()
        for _ in range(2 * reps):
            device_calls()
        dev.sync()
        out["device_calls_ms"] = 1e3 * (time.perf_counter() - t0) / (2 * reps)
        if Edev is not None:
            Edev.free()
    finally:
        glm._resident_fit = False
        glm._release_features()
    flops = 3 * 2.0 * K * L * M * F
    out["gemm_tflops_of_device_calls"] = flops / (out["device_calls_ms"] * 1e-3) / 1e12
    if dtype == "f64":
        out["fraction_of_f64_peak"] = flops / (out["device_calls_ms"] * 1e-3) / F64_PEAK
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--timeout", type=int, default=500)
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.timeout, exit=True)
    from revrand_amd import _hip
    dev = _hip.get_device()
    N, d, n, K, L, M = args.rows, 32, 1024, 10, 50, 65536
    rng = np.random.default_rng([20260928, 5])
    X = rng.standard_normal((N, d), dtype=np.float32)
    y = rng.poisson(np.exp(0.3 * X[:, 0].astype(np.float64))).astype(np.float64)
    plan = _hip.glm64_plan(M, 2 * n, K * L, dev.compute_units)
    res = {"shape": {"N": N, "d": d, "F": 2 * n, "K": K, "L": L, "M": M}, "compute_units": dev.compute_units,
           "ed_plan_slabs_len_tiles_rowspad": plan, "sessions": []}
    os.environ.pop("RR_GLM64_KSLABS", None)
    for label, dtype, slabs in (("f64", "f64", None), ("f32", "f32", None), ("f64 one slab", "f64", "1"), ("f64 again", "f64", None)):
        if slabs is None:
            os.environ.pop("RR_GLM64_KSLABS", None)
        else:
            os.environ["RR_GLM64_KSLABS"] = slabs
        r = session(dev, X, y, dtype, args.reps, N, d, n, K, L, M)
        r["route"] = label
        res["sessions"].append(r)
        print("%-14s %s" % (label, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), file=sys.stderr, flush=True)
    os.environ.pop("RR_GLM64_KSLABS", None)
    faulthandler.cancel_dump_traceback_later()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
