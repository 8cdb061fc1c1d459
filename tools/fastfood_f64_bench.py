#!/usr/bin/env python3
"""FastFood children of the float64 feature matrix (docs/KERNELS.md 3.49): resident_bases="all" against "fourier", one process,
arms alternating, median and range of --rounds rounds.

  slm64      StandardLinearModel._elbo, FastFoodRBF(dtype="f64"), N = 100 000, Xdim = 64, nbases = 2048 (F = 4096)
  slm1024    the same at N = 20 000, Xdim = 1024, nbases = 4096 (F = 8192): the wide contraction on the float64 GEMM
  glm        the float64 GLM step at batch 65 536 with a FastFoodRBF child (d = 32, n = 1024, K = 10, L = 50); the "fourier" arm
             forms (M, F, d) on the host, so it runs at --host-batch rows (default 4096) and both arms report ms per 1000 rows
  xt         rr_featmat64_pass2_xt alone at slm1024's shape: ms per call, TFLOP/s over 2 rows d n against the 78.6 TFLOP/s
             float64 MFMA peak (the call = A-forming kernel + X staging + GEMM + slab sum; per-kernel times: run under
             rocprofv3 --kernel-trace --stats), and the float64 chain kernel's write rate as tools/fastfood_f64_bench.py
             reported it before (N = 65 536, d = 128, nbases = 8192)

    python tools/fastfood_f64_bench.py [--what slm64,slm1024,glm,xt] [--rounds 3] [--timeout 900]

An arm that cannot run (allocation failure, a refusal) is reported with its error: that is the result.  One line of JSON."""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F64_PEAK = 78.6e12


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def slm_arms(dev, N, d, nbases, rounds, evals=2):
    import revrand_amd.basis_functions as bs
    from revrand_amd.btypes import Parameter, Positive
    from revrand_amd.slm import StandardLinearModel
    rs = np.random.RandomState(0)
    X = rs.randn(N, d)
    y = np.sin(X[:, :4] @ rs.randn(4)) + 0.1 * rs.randn(N)
    ls = np.linspace(0.9, 1.4, d) * np.sqrt(d)
    basis = bs.FastFoodRBF(nbases=nbases, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()), dtype="f64")
    out, models = {}, {}
    for arm in ("all", "fourier"):
        out[arm] = {"ms": []}
        try:
            slm = StandardLinearModel(basis, resident_bases=arm)
            slm.obj_ = -np.inf
            slm._state = slm._make_state(X, y)
            out[arm]["state"] = type(slm._state).__name__ if slm._state is not None else "none (transform / grad on the host)"
            if slm._state is None:
                raise MemoryError("the host route materialises (N, F, d) = %.1f GB" % (N * 2.0 * basis.n * d * 8 / 1e9))
            slm._elbo(X, y, 0.5, 1.0, ls)   # warm: scratch, handles
            dev.sync()
            models[arm] = slm
        except Exception as e:  # noqa: BLE001 -- the failure is the measurement
            out[arm]["error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
    vals = {}
    for _ in range(rounds):
        for arm, slm in models.items():
            t0 = time.perf_counter()
            for _ in range(evals):
                vals[arm] = slm._elbo(X, y, 0.5, 1.0, ls)[0]
            dev.sync()
            out[arm]["ms"].append(1e3 * (time.perf_counter() - t0) / evals)
    for arm, slm in models.items():
        out[arm].update(_stats(out[arm].pop("ms")), nelbo=float(vals[arm]))
        slm._state.release()
    return {"shape": {"N": N, "d": d, "F": 2 * basis.n}, "arms": out}


def glm_arms(dev, rounds, host_batch, reps=3):
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd.btypes import Parameter, Positive
    from revrand_amd.glm import GeneralizedLinearModel
    N, d, n, K, L, M = 500_000, 32, 1024, 10, 50, 65536
    F = 2 * n
    rng = np.random.default_rng([20261021, 5])
    X = rng.standard_normal((N, d))
    y = rng.poisson(np.exp(0.3 * X[:, 0])).astype(np.float64)
    rs = np.random.RandomState(0)
    m, C = 0.1 * rs.randn(F, K), rs.gamma(2., 0.5, size=(F, K))
    ls = np.linspace(0.8, 1.5, d) * np.sqrt(d)
    basis = bs.FastFoodRBF(nbases=n, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()), dtype="f64")
    perm = rs.permutation(N)
    out, runs = {}, []
    for arm, batch in (("all", M), ("all", host_batch), ("fourier", host_batch)):
        glm = GeneralizedLinearModel(lk.Poisson(), basis, K=K, nsamples=L, batch_size=batch, random_state=2, dtype="f64",
                                     resident_bases=arm)
        glm.B_, glm.D_ = N / batch, F
        glm._GeneralizedLinearModel__it = 1
        feats = glm._features()
        glm._resident_fit = feats.make_resident(X, arm)
        key = "%s @ %d rows" % (arm, batch)
        out[key] = {"resident": bool(glm._resident_fit), "ms": []}

        def step(i, glm=glm, batch=batch):
            idx = perm[(i * batch) % (N - batch):(i * batch) % (N - batch) + batch]
            if glm._resident_fit:
                return glm._elbo(m, C, 1.0, [], ls, np.empty((batch, 0)), y[idx], idx)
            return glm._elbo(m, C, 1.0, [], ls, X[idx], y[idx])
        step(0)
        dev.sync()
        out[key]["children"] = [type(c).__name__ for c, _, _ in feats.children]
        runs.append((key, glm, step, batch))
    for _ in range(rounds):
        for key, glm, step, batch in runs:
            t0 = time.perf_counter()
            for i in range(reps):
                step(i + 1)
            dev.sync()
            out[key]["ms"].append(1e3 * (time.perf_counter() - t0) / reps)
    for key, glm, step, batch in runs:
        st = _stats(out[key].pop("ms"))
        out[key].update(st, ms_per_1000_rows=st["median_ms"] * 1000.0 / batch)
        glm._resident_fit = False
        glm._release_features()
    return {"shape": {"N": N, "d": d, "F": F, "K": K, "L": L}, "arms": out}


def xt_alone(dev, rounds):
    from revrand_amd import _hip
    import revrand_amd.basis_functions as bs
    rows, d, n = 20000, 1024, 4096
    F = 2 * n
    rs = np.random.RandomState(0)
    fm = _hip.FeatureMatrix64(rows, F)
    fm.begin(rows)
    fm.put_host(rs.randn(rows, F), 0)
    dy = dev.upload_vector(rs.randn(rows))
    fm.pass2_begin(rs.randn(F), np.eye(F))
    fm.pass2_rows(dy)
    dX = dev.upload_matrix(rs.randn(rows, d))
    dT = dev.zeros(d * n * 8)
    fm.pass2_xt(dX, d, n, 0, dT)
    dev.sync()
    ms = []
    for _ in range(max(rounds, 3)):
        dev.timer_start()
        fm.pass2_xt(dX, d, n, 0, dT)
        ms.append(dev.timer_stop())
    st = _stats(ms)
    rp = (rows + 127) // 128 * 128
    res = {"pass2_xt": dict(st, rows=rows, d=d, n=n, tflops_of_call=2.0 * rows * d * n / (st["median_ms"] * 1e-3) / 1e12,
                            fraction_of_f64_peak_of_call=2.0 * rows * d * n / (st["median_ms"] * 1e-3) / F64_PEAK,
                            a_kernel_bytes=rp * n * 40, x_staging_bytes=rows * d * 8 + rp * d * 8,
                            plan=_hip.glm64_plan(rows, n, d, dev.compute_units))}
    for b in (dX, dT, dy):
        b.free()
    fm = None
    # the float64 chain kernel writing float64 features (what `put` runs), device-resident
    N, dd, nb = 65536, 128, 8192
    basis = bs.FastFoodRBF(nbases=nb, Xdim=dd, random_state=1, dtype="f64")
    ff = basis._handles()[0]
    Fc = 2 * ff.n
    dX = dev.upload_matrix(rs.randn(N, dd))
    outb = dev.malloc(N * Fc * 8)
    ms = []
    for _ in range(max(rounds, 3)):
        dev.timer_start()
        ff.transform_dev(dX, 1.0, outb, np.float64)
        ms.append(dev.timer_stop())
    st = _stats(ms)
    res["chain_f64"] = dict(st, N=N, F=Fc, tb_per_s_written=N * Fc * 8 / st["median_ms"] / 1e9)
    dX.free()
    outb.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="slm64,slm1024,glm,xt")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-batch", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=900)
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.timeout, exit=True)
    from revrand_amd import _hip
    dev = _hip.get_device()
    res = {"compute_units": dev.compute_units, "rounds": args.rounds}
    for what in args.what.split(","):
        if what == "slm64":
            res[what] = slm_arms(dev, 100_000, 64, 2048, args.rounds)
        elif what == "slm1024":
            res[what] = slm_arms(dev, 20_000, 1024, 4096, args.rounds, evals=1)
        elif what == "glm":
            res[what] = glm_arms(dev, args.rounds, args.host_batch)
        elif what == "xt":
            res[what] = xt_alone(dev, args.rounds)
        else:
            raise SystemExit("unknown --what entry %r" % what)
        print("%-8s %s" % (what, json.dumps(res[what])), file=sys.stderr, flush=True)
    faulthandler.cancel_dump_traceback_later()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
