#!/usr/bin/env python3
"""
Generate tests/golden/fastfood_gm_wide.npz -- FastFoodGM (one spectral-mixture component) on inputs wider than 256 columns as
the REFERENCE computes it -- by importing the reference on the build machine, and hold the NumPy oracle
(oracle/revrand_oracle.py, ``fastfood_gm_transform``) to every array while doing so (1e-12 normwise, on the full arrays,
before anything is trimmed).

    PYTHONDONTWRITEBYTECODE=1 python -B tools/make_fastfood_gm_wide_golden.py

Shapes (Xdim, nbases, N): (300, 600, 4), (1000, 1500, 3), (2049, 4097, 2), (4096, 4096, 2), each with
``FastFoodGM(random_state=3)``, ``mean = 0.3 RandomState(2000 + Xdim).randn(Xdim)`` and the ARD length scale
``linspace(0.7, 1.6, Xdim)`` (the basis has no isotropic form: scalars are broadcast).

What is stored, and why not everything: the full outputs are 4.8 MB of float64 (random mantissas do not compress), the file
has to stay under 400 KB.  So
  * X is drawn in float64 and ROUNDED TO FLOAT32 before the reference sees it (stored as float32: half the bytes, and a
    float32 basis then starts from the very numbers the reference had);
  * ``transform`` (N, 4n) is stored at COLS = 256 sampled columns per shape -- the first and last column of each of the four
    blocks [cos+ | sin+ | cos- | sin-], both sides of every seam between them and of the first d2 seam, the rest drawn without
    replacement by RandomState(Xdim).
All N rows are kept.  Only data is written: inputs, means, length scales, column indices and the reference's outputs.  The
reference is imported the way oracle/make_golden.py does it (the ``decorator`` stand-in of oracle/shim, ``np.asscalar`` defined
for this process); nothing under oracle/ or in the reference is touched.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = os.environ.get("REVRAND_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(0, REFERENCE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402

if not hasattr(np, "asscalar"):
    np.asscalar = lambda a: a.item()  # process-local

import revrand.basis_functions as rb  # noqa: E402
from revrand.btypes import Bound, Parameter, Positive  # noqa: E402

import revrand_oracle as orc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fastfood_gm_wide.npz")
MAX_BYTES = 400 * 1024
SHAPES = [(300, 600, 4), (1000, 1500, 3), (2049, 4097, 2), (4096, 4096, 2)]
SEED = 3
COLS = 256


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max() / max(np.abs(a).max(), 1e-300)
    assert err <= tol, err
    return err


def sample_columns(d, d2, n):
    fixed = [0, 1, d2 - 1, d2]
    for blk in range(4):
        fixed += [blk * n - 1, blk * n, blk * n + 1, (blk + 1) * n - 1]
    fixed = sorted({c for c in fixed if 0 <= c < 4 * n})
    rest = np.setdiff1d(np.arange(4 * n), fixed)
    pick = np.random.RandomState(d).choice(rest, COLS - len(fixed), replace=False)
    return np.sort(np.concatenate((fixed, pick))).astype(np.int64)


def main():
    out = {}
    worst = 0.0
    for d, nb, N in SHAPES:
        tag = "d%d" % d
        X = np.random.RandomState(1000 + d).randn(N, d).astype(np.float32)
        X64 = X.astype(np.float64)
        mean = 0.3 * np.random.RandomState(2000 + d).randn(d)
        ard = np.linspace(0.7, 1.6, d)
        b = rb.FastFoodGM(nbases=nb, Xdim=d, mean=Parameter(np.zeros(d), Bound()), lenscale=Parameter(np.ones(d), Positive()),
                          random_state=SEED)
        mats = orc.fastfood_matrices(nb, d, SEED)
        for mine, theirs in zip(mats, (b.B, b.G, b.PI, b.S)):
            worst = max(worst, close(theirs, mine))
        d2, k, n = orc.fastfood_dims(nb, d)
        cols = sample_columns(d, d2, n)
        out["X_" + tag], out["mean_" + tag], out["ls_ard_" + tag], out["cols_" + tag] = X, mean, ard, cols
        P = b.transform(X64, mean, ard)
        assert P.shape == (N, 4 * n)
        worst = max(worst, close(P, orc.fastfood_gm_transform(X64, *mats, mean, ard)))
        out["Phi_" + tag] = P[:, cols]
        print("%-6s d2=%d k=%d: reference vs oracle so far %.2e" % (tag, d2, k, worst))
    np.savez(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote %s: %d arrays, %d bytes; worst normwise error oracle vs reference %.2e" % (OUT, len(out), size, worst))
    assert size <= MAX_BYTES, size


if __name__ == "__main__":
    main()
