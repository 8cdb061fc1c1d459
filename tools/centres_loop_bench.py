"""A GLM fit with a RadialBasis child through the host loop around `_elbo` (``resident_bases="fourier"``: what such a fit
always took before) and through the resident SVI loop (``resident_bases="all"``, rr_glm_sgd_step with an
RR_SGD_CHILD_CENTRES child): milliseconds per step, same process, same GPU, arms alternating.

  python tools/centres_loop_bench.py [--reps 2] [--shapes large,default] [--samplers host,device]

Shapes: "large" -- N = 100 000, d = 8, M = 512 centres + a linear child, batch = 10 000, K = 10, L = 50, 60 steps;
"default" -- the reference's default regime (glm.py:120-124), batch = 10, maxiter = 3000, K = 10, L = 50, on 2000 rows,
d = 2, M = 20.  nstarts = 0 in both: the loops are what is timed.  Per arm: wall time of `fit` / maxiter, and for the resident
loop the median interval of `_resident_clock` (the host times at which steps were queued: the queue is two deep, so it
follows the device's pace).  The "default" shape has a third arm, ``resident_bases="all", fused_bases="all"``: the
many-steps-per-launch kernel of small minibatches (rr_svi.hip) with the centres child inside it; it raises if that loop was
not taken.  One JSON line per (shape, sampler) at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import revrand_amd.basis_functions as bs  # noqa: E402
from revrand_amd import _hip  # noqa: E402
from revrand_amd import likelihoods as lk  # noqa: E402
from revrand_amd.btypes import Parameter, Positive  # noqa: E402
from revrand_amd.glm import GeneralizedLinearModel  # noqa: E402

SHAPES = {"large": dict(N=100_000, d=8, M=512, batch=10_000, K=10, L=50, maxiter=60),
          "default": dict(N=2000, d=2, M=20, batch=10, K=10, L=50, maxiter=3000)}


def one_fit(shape, sampler, arm):
    s = SHAPES[shape]
    rs = np.random.RandomState(7)
    X = rs.randn(s["N"], s["d"])
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.1 * rs.randn(s["N"])
    basis = bs.RadialBasis(centres=X[:s["M"]].copy(), lenscale=Parameter(np.ones(s["d"]), Positive())) + bs.LinearBasis(onescol=True)
    glm = GeneralizedLinearModel(lk.Gaussian(), basis, K=s["K"], nsamples=s["L"], batch_size=s["batch"], maxiter=s["maxiter"],
                                 nstarts=0, random_state=1, sampler=sampler, resident_bases="all" if arm == "fused" else arm,
                                 fused_bases="all" if arm == "fused" else "fourier")
    np.random.seed(0)
    fused_steps = [0]
    real_run = _hip.FusedSvi.run

    def run(self, n, *a, **k):
        fused_steps[0] += n
        return real_run(self, n, *a, **k)
    _hip.FusedSvi.run = run
    try:
        t0 = time.perf_counter()
        glm.fit(X, y)
        wall = time.perf_counter() - t0
    finally:
        _hip.FusedSvi.run = real_run
    out = {"wall_ms_per_step": 1e3 * wall / s["maxiter"]}
    ck = glm.__dict__.pop("_resident_clock", None)
    if arm == "fused":
        if fused_steps[0] != s["maxiter"]:
            raise RuntimeError("fused_bases='all' did not take the fused loop (%d of %d steps)" % (fused_steps[0], s["maxiter"]))
        return out
    if fused_steps[0]:
        raise RuntimeError("resident_bases=%r took the fused loop" % arm)
    if arm == "all":
        if ck is None:
            raise RuntimeError("resident_bases='all' did not take the resident loop")
        if len(ck) > 24:
            out["clock_ms_per_step"] = 1e3 * float(np.median(np.diff(ck[10:-2])))
    elif ck is not None:
        raise RuntimeError("resident_bases='fourier' took a device loop")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--shapes", default="large,default")
    ap.add_argument("--samplers", default="host,device")
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        for sampler in a.samplers.split(","):
            arms = ("fourier", "all", "fused") if shape == "default" else ("fourier", "all")
            runs = {arm: [] for arm in arms}
            for arm in arms[1:]:
                one_fit(shape, sampler, arm)   # (first use: handles, buffers, the library's lazy allocations)
            for _ in range(a.reps):
                for arm in arms:
                    runs[arm].append(one_fit(shape, sampler, arm))
            best = {arm: min(r["wall_ms_per_step"] for r in runs[arm]) for arm in runs}
            clock = [r["clock_ms_per_step"] for r in runs["all"] if "clock_ms_per_step" in r]
            line = {"tool": "centres_loop_bench", "shape": dict(SHAPES[shape], name=shape), "sampler": sampler,
                    "host_loop_ms_per_step": round(best["fourier"], 4), "resident_loop_ms_per_step": round(best["all"], 4),
                    "resident_clock_ms_per_step": round(min(clock), 4) if clock else None,
                    "speedup": round(best["fourier"] / best["all"], 2)}
            if "fused" in best:
                # (repetition by repetition: the fused arm is faster than the step-per-call arm only if it is in EVERY pair)
                line["fused_loop_ms_per_step"] = round(best["fused"], 4)
                line["fused_faster_in_every_rep"] = all(f["wall_ms_per_step"] < r["wall_ms_per_step"]
                                                        for f, r in zip(runs["fused"], runs["all"]))
            line["runs"] = runs
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
