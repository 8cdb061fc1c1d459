"""A GLM fit on a spectral mixture -- a concatenation of FastFoodGM components -- through the three loops: the
many-steps-per-launch kernel of small minibatches (``resident_bases="all", fused_bases="all+gm"``: rr_svi.hip with
RR_SGD_CHILD_GM children), the step-per-call resident loop (rr_glm_sgd_step) and the host loop around `_elbo`.  Milliseconds
per step at the reference's default GLM shape (glm.py:120-124: K = 10, nsamples = 50, batch_size = 10, maxiter = 3000) on 2000
rows, nstarts = 0 (the loops are what is timed), with sampler="device" and with the reference's stream.

  python tools/gm_loop_bench.py [--reps 2] [--cases 1,2,1s,2s] [--samplers device,host] [--maxiter 3000] [--timeout 300]

Cases:  1   four FastFoodGM(nbases=32) on Xdim = 4   (F = 512; without the opt-in no device loop takes it: Xdim <= 8)
        2   four FastFoodGM(nbases=32) on Xdim = 12  (F = 512; without the opt-in: the step-per-call loop)
        1s  four FastFoodGM(nbases=8)  on Xdim = 4   (F = 128)
        2s  three FastFoodGM(nbases=16) on Xdim = 12 (F = 192)
At K = 10 and 50 samples the kernel's state fits one CU's LDS up to F = 200 (rr_glm_svi_supported_gm): cases 1 and 2 are
outside that range and their "fused" arm reports the loop the estimator routed them to instead; 1s and 2s are the same mixtures
at widths inside it.

Arms: "fused" -- the opt-in as a user would set it; "step" -- the same estimator with the fused loop switched off (for case 2
and 2s this is also what the default keywords run); "host" -- default keywords, no device loop.  Every fit runs in a child
process of its own under a time limit: a warm-up fit, then the timed one (wall time of `fit`, which ends with the read-back of
the parameters, over maxiter).  The arms alternate, repetition by repetition; the first child that fails ends the run.  One JSON
line per (case, sampler) at the end."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"1": dict(d=4, nbases=32, ncomp=4), "2": dict(d=12, nbases=32, ncomp=4),
         "1s": dict(d=4, nbases=8, ncomp=4), "2s": dict(d=12, nbases=16, ncomp=3)}
ARMS = ("fused", "step", "host")
GLM = dict(N=2000, K=10, L=50, batch=10)


def one_fit(case, sampler, arm, maxiter):
    import numpy as np
    sys.path.insert(0, ROOT)
    import revrand_amd.basis_functions as bs
    from revrand_amd import _hip
    from revrand_amd import likelihoods as lk
    from revrand_amd.btypes import Bound, Parameter, Positive
    from revrand_amd.glm import GeneralizedLinearModel
    c = CASES[case]
    d = c["d"]
    rs = np.random.RandomState(7)
    X = rs.randn(GLM["N"], d)
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.1 * rs.randn(GLM["N"])

    def fit(steps):
        basis = None
        for i in range(c["ncomp"]):
            b = bs.FastFoodGM(nbases=c["nbases"], Xdim=d, random_state=10 + i, mean=Parameter(0.2 * (i + 1) * np.ones(d), Bound()),
                              lenscale=Parameter((1.0 + 0.25 * i) * np.ones(d), Positive()))
            basis = b if basis is None else basis + b
        opt_in = dict(resident_bases="all", fused_bases="all+gm") if arm != "host" else {}
        glm = GeneralizedLinearModel(lk.Gaussian(), basis, K=GLM["K"], nsamples=GLM["L"], batch_size=GLM["batch"], maxiter=steps,
                                     nstarts=0, random_state=1, sampler=sampler, **opt_in)
        if arm == "step":
            glm._fused_sgd = False
        if arm == "host":
            glm._resident_sgd = False
        np.random.seed(0)
        count = {"fused": 0, "step": 0}
        real_run, real_step = _hip.FusedSvi.run, _hip.ResidentSgd.step

        def run(self, n, *a, **k):
            count["fused"] += n
            return real_run(self, n, *a, **k)

        def step(self, *a, **k):
            count["step"] += 1
            return real_step(self, *a, **k)
        _hip.FusedSvi.run, _hip.ResidentSgd.step = run, step
        try:
            t0 = time.perf_counter()
            glm.fit(X, y)
            _hip.get_device().sync()
            wall = time.perf_counter() - t0
        finally:
            _hip.FusedSvi.run, _hip.ResidentSgd.step = real_run, real_step
        route = "fused" if count["fused"] == steps else ("step" if count["step"] == steps else
                                                         ("host" if not (count["fused"] or count["step"]) else "mixed"))
        return wall, route, int(glm.D_), float(np.abs(glm.weights_).sum())
    fit(min(maxiter, 64))   # (first use: handles, buffers, code objects, the library's lazy allocations)
    wall, route, F, check = fit(maxiter)
    if arm != "fused" and route != arm:
        raise RuntimeError("arm %r ran the %s loop" % (arm, route))
    return {"arm": arm, "route": route, "F": F, "ms_per_step": 1e3 * wall / maxiter, "weights_abs_sum": check}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cases", default="1,2,1s,2s")
    ap.add_argument("--samplers", default="device,host")
    ap.add_argument("--maxiter", type=int, default=3000)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process (one warm-up and one timed fit)")
    ap.add_argument("--child", nargs=3, metavar=("CASE", "SAMPLER", "ARM"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(one_fit(a.child[0], a.child[1], a.child[2], a.maxiter)), flush=True)
        return 0
    for case in a.cases.split(","):
        for sampler in a.samplers.split(","):
            runs = {arm: [] for arm in ARMS}
            for _ in range(a.reps):
                for arm in ARMS:
                    cmd = [sys.executable, os.path.abspath(__file__), "--maxiter", str(a.maxiter), "--child", case, sampler, arm]
                    try:
                        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                    except subprocess.TimeoutExpired:
                        print("gm_loop_bench: case %s sampler %s arm %s: no result within %d s; stopping" % (case, sampler, arm, a.timeout),
                              flush=True)
                        return 1
                    res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                    if r.returncode != 0 or not res:   # nothing more is started on the device after a failed child
                        print("gm_loop_bench: case %s sampler %s arm %s failed (exit %d); stopping\n%s" %
                              (case, sampler, arm, r.returncode, r.stderr[-3000:]), flush=True)
                        return 1
                    runs[arm].append(json.loads(res[-1][len("RESULT "):]))
            best = {arm: min(v["ms_per_step"] for v in runs[arm]) for arm in ARMS}
            line = {"tool": "gm_loop_bench", "case": dict(CASES[case], name=case, F=runs["fused"][0]["F"], **GLM), "sampler": sampler,
                    "maxiter": a.maxiter, "fused_arm_route": sorted(set(v["route"] for v in runs["fused"])),
                    "fused_ms_per_step": round(best["fused"], 4), "step_per_call_ms_per_step": round(best["step"], 4),
                    "host_loop_ms_per_step": round(best["host"], 4),
                    # (repetition by repetition: an arm is faster only if it is in EVERY pair)
                    "fused_faster_than_step_in_every_rep": all(f["ms_per_step"] < s["ms_per_step"]
                                                               for f, s in zip(runs["fused"], runs["step"])),
                    "fused_faster_than_host_in_every_rep": all(f["ms_per_step"] < h["ms_per_step"]
                                                               for f, h in zip(runs["fused"], runs["host"])),
                    "runs": runs}
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
