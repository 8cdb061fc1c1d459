"""The reference report's GLM regime at SARCOS's width -- minibatches of 10 rows, K = 10, 50 samples, d = 21 ARD RandomRBF,
nbases 256 ... 8192 (F = 512 ... 16384), N = 44 484 -- through GeneralizedLinearModel(wide_fused=True) (the chain of kernels of
rr_svi_wide.hip; at nbases 256 the LDS kernel, which still takes what it can) and wide_fused=False (what those shapes took
before: the step-per-call loop above F ~ 800): microseconds per SGD step.

What is measured: the loop's own clock (`_resident_clock`).  The step-per-call loop marks the host time at which each step was
queued (its queue is two deep, so the marks follow the device) and the end of the fit after the final read; the fused loops mark
the end of each block of steps -- here 50 steps, and this tool synchronises the device at each mark -- and the end of the fit.
A figure is (end of fit - mark after the warm-up steps) / (steps after the warm-up): everything a step costs, host included.
Arms alternate in one process, three rounds; the table gives the median and the spread (min ... max) of the rounds.

    python tools/glm_wide_bench.py [--nbases 256,512,...] [--steps 300] [--warmup 50] [--rounds 3] [--extra] [--out FILE]

--extra adds minibatches of 32 and 64 rows at nbases 1024 and 8192 (where the range ends in M) and sampler="host" at nbases 1024
(there the host's generator, 0.5 M normals per step on one RandomState, bounds both arms)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import revrand_amd.basis_functions as bs  # noqa: E402
from revrand_amd import _hip  # noqa: E402
from revrand_amd import glm as glm_mod  # noqa: E402
from revrand_amd import likelihoods as lk  # noqa: E402
from revrand_amd.btypes import Parameter, Positive  # noqa: E402
from revrand_amd.glm import GeneralizedLinearModel  # noqa: E402


def one_fit(X, y, nbases, wide, batch, sampler, steps, warmup):
    d = X.shape[1]
    basis = bs.RandomRBF(nbases=nbases, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()))
    glm = GeneralizedLinearModel(lk.Gaussian(), basis, K=10, nsamples=50, batch_size=batch, maxiter=steps + warmup, nstarts=0,
                                 random_state=3, sampler=sampler, wide_fused=wide)
    ran = {"wide": 0, "fused": 0, "resident": 0}
    real = (_hip.WideSvi.run, _hip.FusedSvi.run, _hip.ResidentSgd.step)

    def wrun(self, n, *a, **k):
        ran["wide"] += n
        real[0](self, n, *a, **k)
        self.dev.sync()

    def frun(self, n, *a, **k):
        ran["fused"] += n
        real[1](self, n, *a, **k)
        self.dev.sync()

    def step(self, *a, **k):
        ran["resident"] += 1
        return real[2](self, *a, **k)
    _hip.WideSvi.run, _hip.FusedSvi.run, _hip.ResidentSgd.step = wrun, frun, step
    old = glm_mod._FusedLoop.BLOCK_STEPS
    glm_mod._FusedLoop.BLOCK_STEPS = warmup
    try:
        np.random.seed(0)
        t0 = time.perf_counter()
        glm.fit(X, y)
        total = time.perf_counter() - t0
    finally:
        _hip.WideSvi.run, _hip.FusedSvi.run, _hip.ResidentSgd.step = real
        glm_mod._FusedLoop.BLOCK_STEPS = old
    ck = glm.__dict__["_resident_clock"]
    loop = max(ran, key=ran.get)
    assert ran[loop] == steps + warmup, ran
    mark = ck[warmup] if loop == "resident" else ck[0]     # (the fused loops: the first mark closes the warm-up block)
    return loop, 1e6 * (ck[-1] - mark) / steps, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nbases", default="256,512,1024,2048,4096,8192")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=44484)
    ap.add_argument("--extra", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    X = rs.randn(args.rows, 21).astype(np.float32)
    y = (np.sin(X[:, 0]) + 0.3 * X[:, 5] + 0.1 * rs.randn(args.rows)).astype(np.float32)
    rows = [(int(n), 10, "device") for n in args.nbases.split(",") if n]
    if args.extra:
        rows += [(1024, 32, "device"), (1024, 64, "device"), (8192, 32, "device"), (8192, 64, "device"), (1024, 10, "host")]
    out = open(args.out, "w") if args.out else None
    print("%7s %6s %4s %7s | %-9s %9s (%9s ... %9s) | %-9s %9s (%9s ... %9s) | ratio" %
          ("nbases", "F", "M", "sampler", "True", "us/step", "min", "max", "False", "us/step", "min", "max"))
    for nbases, batch, sampler in rows:
        res = {True: [], False: []}
        loops = {}
        for _ in range(args.rounds):
            for wide in (True, False):
                loop, us, _ = one_fit(X, y, nbases, wide, batch, sampler, args.steps, args.warmup)
                res[wide].append(us)
                loops[wide] = loop
        med = {w: float(np.median(res[w])) for w in res}
        print("%7d %6d %4d %7s | %-9s %9.1f (%9.1f ... %9.1f) | %-9s %9.1f (%9.1f ... %9.1f) | %.2f" %
              (nbases, 2 * nbases, batch, sampler, loops[True], med[True], min(res[True]), max(res[True]),
               loops[False], med[False], min(res[False]), max(res[False]), med[False] / med[True]), flush=True)
        if out:
            out.write(json.dumps({"nbases": nbases, "F": 2 * nbases, "M": batch, "sampler": sampler, "loops": {str(k): v for k, v in loops.items()},
                                  "us_per_step": {str(k): v for k, v in res.items()}}) + "\n")
            out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
