"""Shapes, latent values and the per-element bound of the FLOAT64 GLM step's tests (pure numpy; shared by
tests/test_glm_f64_host.py, tests/test_gpu_glm_f64.py and tests/test_gpu_glm_f64_debug.py).

Per-element bound on the likelihood terms df and ll of rr_glm64.hip's glm64_lik:

    |got - ref| <= (16 + 4 |f|) 2^-53 S + 1e-300

with S, the targets and the references of tests/lik_cases.py.  The argument is that file's, with float64's unit roundoff in
place of float32's: at most eight float64 operations at up to 2 ulp each (ocml's exp and log1p are within the 2 ulp it assumes)
give the 16, and an error of a few ulp in the argument of exp moves exp(f) by that many ulp times |f|, the 4 |f| -- here f IS
the weight sample (X = [[1]], the samples are not pre-scaled), so that term is slack.  1e-300: nothing on the grid comes near
float64's subnormal range (exp(-200) = 1.4e-87), the floor only keeps a bound of exactly 0 from dividing.

The latent values are the 64 float32 values of lik_cases.grid(lik), as float64, plus +-36.7 and +-36.8: 53 ln 2 = 36.74, where
fl(1 + exp(-|f|)) == 1 switches in float64 (the float32 grid has the same switch at 24 ln 2 = 16.6).  K = 68 weight samples, L = 1.
"""
import numpy as np

import lik_cases as lc

EPS64 = 2.0 ** -53
ABS_FLOOR64 = 1e-300
SWITCH64 = (36.7, 36.8)   # around 53 ln 2

# the step's tolerances against the reference / the oracle: the project's own float64 figures (the oracle holds 1e-10 on
# tests/golden/glm.npz on the CPU, the float64 matrix' second pass 1e-9 .. 1e-10 on the device)
TOL_OBJ = 1e-9      # relative, -ELBO
TOL_GRAD = 1e-9     # normwise: ndm, ndC, dbp, dlp
TOL_DL = 1e-10      # dL (host arithmetic on m, C alone)
TOL_SLABS = 1e-12   # normwise, one row slab against three
TOL_FIT = 1e-8      # normwise per fitted block after 20 steps (the oracle: 1e-9 on the CPU; x10 for tile-order sums and fmas)
TOL_PROJECT = 1e-12  # normwise, the latent samples of a prediction call

# test 2: the ragged concatenation;  test 3 / 5: every tile edge at once
CONCAT = dict(M=333, d=5, K=4, L=7)
EDGES = dict(M=300, n=100, K=3, L=50, d=4)


def grid(lik):
    """The latent values of a likelihood: lik_cases' 64 and the float64 switch on both sides (68 distinct float64 values)."""
    g = np.concatenate([lc.grid(lik).astype(np.float64), [v for s in SWITCH64 for v in (s, -s)]])
    assert g.size == 68 and np.unique(g).size == 68 and lc.in_domain(lik, g).all()
    return g


def bound(f, S):
    """The per-element bound on |got - ref| in float64"""
    return lc.c_of(f) * EPS64 * np.asarray(S, dtype=float) + ABS_FLOOR64


def plan_reference(rows, F, KL, num_cu):
    """What rr_glm64_plan must return, restated: (slabs, slab length, tiles, rows_pad)."""
    rp, ld, klp = -(-rows // 128) * 128, -(-F // 128) * 128, -(-KL // 128) * 128
    tiles, q, r16 = (klp // 128) * (ld // 128), rp // 128, rp // 16
    s = 1 if tiles >= 2 * num_cu else -(-num_cu // tiles)
    s = max(1, min(s, q))
    while s < q and (s - 1) * -(-r16 // s) >= r16:
        s += 1
    return s, 16 * -(-r16 // s), tiles, rp
