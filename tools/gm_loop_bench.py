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
line per (case, sampler) at the end.

  python tools/gm_loop_bench.py --wide [--shapes 1x32@10,2x32@10,...] [--steps 300] [--warmup 50] [--rounds 3] [--force] [--out FILE]

The wide small-minibatch loop (``wide_fused=True`` next to the opt-in: rr_svi_wide.hip with RR_SGD_CHILD_GM items) against
``wide_fused=False`` (what those shapes took before: the step-per-call loop above the LDS kernel's range), as
tools/glm_wide_bench.py measures the loop's other children: shapes are <components>x<nbases>@<minibatch> on Xdim = 4, K = 10, 50
samples, sampler="device", N = 2000; the two arms alternate in ONE process, --rounds rounds; microseconds per step from the loop's
own clock (`_resident_clock`: (end of fit - mark after the warm-up steps) / steps, the device synchronised at each mark); the
table gives the median and the spread (min ... max) of the rounds and the loop each arm ran.  --force sets the tests' switch, so
that a shape the LDS kernel would take (F <= 200) is measured on the wide loop too."""
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


def wide_fit(ncomp, nbases, batch, wide, steps, warmup, force):
    """one fit of the --wide table: (loop that ran, microseconds per step)"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import revrand_amd.basis_functions as bs
    from revrand_amd import _hip
    from revrand_amd import glm as glm_mod
    from revrand_amd import likelihoods as lk
    from revrand_amd.btypes import Bound, Parameter, Positive
    from revrand_amd.glm import GeneralizedLinearModel
    d = 4
    rs = np.random.RandomState(7)
    X = rs.randn(GLM["N"], d)
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.1 * rs.randn(GLM["N"])
    basis = None
    for i in range(ncomp):
        b = bs.FastFoodGM(nbases=nbases, Xdim=d, random_state=10 + i, mean=Parameter(0.2 * (i % 4 + 1) * np.ones(d), Bound()),
                          lenscale=Parameter((1.0 + 0.25 * (i % 4)) * np.ones(d), Positive()))
        basis = b if basis is None else basis + b
    glm = GeneralizedLinearModel(lk.Gaussian(), basis, K=GLM["K"], nsamples=GLM["L"], batch_size=batch, maxiter=steps + warmup,
                                 nstarts=0, random_state=1, sampler="device", resident_bases="all", fused_bases="all+gm",
                                 wide_fused=wide)
    glm._wide_fused_force = bool(force and wide)
    if not wide:
        glm._fused_sgd = False     # the step-per-call loop, whatever the LDS kernel would take
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
        glm.fit(X, y)
    finally:
        _hip.WideSvi.run, _hip.FusedSvi.run, _hip.ResidentSgd.step = real
        glm_mod._FusedLoop.BLOCK_STEPS = old
    ck = glm.__dict__["_resident_clock"]
    loop = max(ran, key=ran.get)
    assert ran[loop] == steps + warmup, ran
    mark = ck[warmup] if loop == "resident" else ck[0]     # (the fused loops: the first mark closes the warm-up block)
    return loop, int(glm.D_), 1e6 * (ck[-1] - mark) / steps


def wide_table(a):
    import numpy as np
    out = open(a.out, "w") if a.out else None
    print("%9s %6s %4s | %-9s %9s (%9s ... %9s) | %-9s %9s (%9s ... %9s) | ratio" %
          ("shape", "F", "M", "True", "us/step", "min", "max", "False", "us/step", "min", "max"))
    for shape in a.shapes.split(","):
        comp, batch = shape.split("@")
        ncomp, nbases = (int(v) for v in comp.split("x"))
        res, loops, F = {True: [], False: []}, {}, 0
        for _ in range(a.rounds):
            for wide in (True, False):
                loops[wide], F, us = wide_fit(ncomp, nbases, int(batch), wide, a.steps, a.warmup, a.force)
                res[wide].append(us)
        med = {w: float(np.median(res[w])) for w in res}
        print("%9s %6d %4d | %-9s %9.1f (%9.1f ... %9.1f) | %-9s %9.1f (%9.1f ... %9.1f) | %.2f" %
              (comp, F, int(batch), loops[True], med[True], min(res[True]), max(res[True]),
               loops[False], med[False], min(res[False]), max(res[False]), med[False] / med[True]), flush=True)
        if out:
            out.write(json.dumps({"shape": shape, "F": F, "M": int(batch), "loops": {str(k): v for k, v in loops.items()},
                                  "us_per_step": {str(k): v for k, v in res.items()}}) + "\n")
            out.flush()
    if out:
        out.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", action="store_true", help="the wide_fused=True / False table (one process, arms alternating)")
    ap.add_argument("--shapes", default="1x32@10,2x32@10,4x32@10,8x32@10,4x256@10,4x32@32,4x32@64")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cases", default="1,2,1s,2s")
    ap.add_argument("--samplers", default="device,host")
    ap.add_argument("--maxiter", type=int, default=3000)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process (one warm-up and one timed fit)")
    ap.add_argument("--child", nargs=3, metavar=("CASE", "SAMPLER", "ARM"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.wide:
        return wide_table(a)
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
