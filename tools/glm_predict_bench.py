#!/usr/bin/env python3
"""The five prediction methods of a GeneralizedLinearModel under predict_engine="host" and "device": RandomRBF F = 2048,
D = 32 inputs, 200 latent samples; Gaussian, Poisson(exp) and binomial likelihoods; N = 100 000 rows for predict /
predict_moments / predict_logpdf / predict_cdf and N = 10 000 for predict_interval (there the HOST engine sets the limit:
202 scipy CDF evaluations of the whole (N, 200) sample matrix per tail).  The model's fitted attributes are set, not learnt.
Prints one JSON line: seconds per call and engine, and host / device.

    --engines device --methods predict_interval     one engine / some methods only (A/B runs of the kernel's switches
                                                    RR_PRED_NO_STEP_CACHE=1, RR_PRED_NO_REG=1: a process each)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import revrand_amd.basis_functions as bs  # noqa: E402
from revrand_amd import likelihoods as lk  # noqa: E402
from revrand_amd.glm import GeneralizedLinearModel  # noqa: E402

METHODS = ["predict", "predict_moments", "predict_logpdf", "predict_cdf", "predict_interval"]


def model(name, engine, d, nbases, K=3):
    like = {"gaussian": lk.Gaussian, "poisson_exp": lambda: lk.Poisson("exp"), "binomial": lk.Binomial}[name]()
    glm = GeneralizedLinearModel(like, bs.RandomRBF(nbases=nbases, Xdim=d, random_state=1), K=K, random_state=0,
                                 predict_engine=engine)
    rs = np.random.RandomState(3)
    D = 2 * nbases
    glm.weights_, glm.covariance_ = rs.randn(D, K) / np.sqrt(D), 1e-3 * rs.rand(D, K) / D + 1e-6
    glm.regularizer_, glm.basis_hypers_ = 1.0, 4.0
    glm.like_hypers_ = 0.3 if name == "gaussian" else []
    return glm


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--interval-rows", type=int, default=10000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--nbases", type=int, default=1024, help="RandomRBF bases (F = 2 nbases)")
    ap.add_argument("--xdim", type=int, default=32)
    ap.add_argument("--engines", default="host,device")
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--likelihoods", default="gaussian,poisson_exp,binomial")
    ap.add_argument("--device-repeats", type=int, default=3, help="timed device calls (the fastest counts); the host gets one")
    a = ap.parse_args()
    engines, methods = a.engines.split(","), a.methods.split(",")
    rs = np.random.RandomState(0)
    X = rs.randn(max(a.rows, a.interval_rows), a.xdim).astype(np.float32)
    S = a.samples
    res = {"shape": {"F": 2 * a.nbases, "D": a.xdim, "samples": S, "rows": a.rows, "interval_rows": a.interval_rows},
           "note": "predict_interval runs at interval_rows: the host engine is the limit there", "seconds": {}, "host_over_device": {}}
    for name in a.likelihoods.split(","):
        nbin = rs.randint(5, 40, size=len(X)).astype(float)
        y = {"gaussian": rs.randn(len(X)), "poisson_exp": rs.poisson(1.5, size=len(X)).astype(float),
             "binomial": np.floor(rs.rand(len(X)) * (nbin + 1))}[name]

        def call(glm, method, n):
            Xn, largs = X[:n], ((nbin[:n],) if name == "binomial" else ())
            if method == "predict_logpdf":
                return glm.predict_logpdf(Xn, y[:n], S, likelihood_args=largs)
            if method == "predict_cdf":
                return glm.predict_cdf(Xn, 1.0, S, likelihood_args=largs)
            if method == "predict_interval":
                return glm.predict_interval(Xn, 0.9, S, likelihood_args=largs)
            return getattr(glm, method)(Xn, S, likelihood_args=largs)

        for method in methods:
            n = a.interval_rows if method == "predict_interval" else a.rows
            secs = {}
            for engine in engines:
                glm = model(name, engine, a.xdim, a.nbases)
                call(glm, method, 64)   # warm-up: handles, scratch, code objects
                best = np.inf
                for _ in range(a.device_repeats if engine == "device" else 1):
                    glm.random_ = np.random.RandomState(7)
                    t0 = time.perf_counter()
                    call(glm, method, n)
                    best = min(best, time.perf_counter() - t0)
                secs[engine] = best
                print("%-12s %-17s %-6s rows=%-7d %.4f s" % (name, method, engine, n, best), file=sys.stderr, flush=True)
                glm._drop_serving()
            res["seconds"]["%s/%s" % (name, method)] = secs
            if "host" in secs and "device" in secs:
                res["host_over_device"]["%s/%s" % (name, method)] = secs["host"] / secs["device"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
