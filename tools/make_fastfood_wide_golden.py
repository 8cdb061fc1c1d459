#!/usr/bin/env python3
"""
Generate tests/golden/fastfood_wide.npz -- FastFoodRBF on inputs wider than 256 columns as the REFERENCE computes it -- by
importing the reference on the build machine, and hold the NumPy oracle (oracle/revrand_oracle.py) to every array while doing
so (1e-12 normwise, on the full arrays, before anything is trimmed).

    PYTHONDONTWRITEBYTECODE=1 python -B tools/make_fastfood_wide_golden.py

Shapes (Xdim, nbases, N): (300, 600, 4), (1000, 1500, 3), (2049, 4097, 2), (4096, 4096, 2), each with
``FastFoodRBF(random_state=3)``, an isotropic length scale (1.3) and an ARD one (linspace(0.7, 1.6, Xdim)).

What is stored, and why not everything: the full outputs are 2.4 MB of float64 (random mantissas do not compress), the file
has to stay under 400 KB.  So
  * X is drawn in float64 and ROUNDED TO FLOAT32 before the reference sees it (stored as float32: half the bytes, and a
    float32 basis then starts from the very numbers the reference had);
  * ``transform`` and the isotropic ``grad`` (N, 2n) are stored at COLS = 256 sampled columns per shape -- the first and last
    column of the cosine and of the sine half, both sides of the seam between them and of the first block seam, the rest drawn
    without replacement by RandomState(Xdim);
  * the ARD ``grad`` (N, 2n, d) is stored at d = 300 only (as the issue has it: the tensor is large) and at GCOLS = 6 of those
    columns, every one of the 300 dimensions.
All N rows are kept.  Only data is written: inputs, length scales, column indices and the reference's outputs.  The reference
is imported the way oracle/make_golden.py does it (the ``decorator`` stand-in of oracle/shim, ``np.asscalar`` defined for this
process); nothing under oracle/ or in the reference is touched.
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
from revrand.btypes import Parameter, Positive  # noqa: E402

import revrand_oracle as orc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fastfood_wide.npz")
MAX_BYTES = 400 * 1024
SHAPES = [(300, 600, 4), (1000, 1500, 3), (2049, 4097, 2), (4096, 4096, 2)]
SEED = 3
LS_ISO = 1.3
COLS, GCOLS = 256, 6


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max() / max(np.abs(a).max(), 1e-300)
    assert err <= tol, err
    return err


def sample_columns(d, d2, n):
    fixed = [0, 1, d2 - 1, d2, n - 1, n, n + 1, n + d2 - 1, n + d2, 2 * n - 1]
    fixed = sorted({c for c in fixed if 0 <= c < 2 * n})
    rest = np.setdiff1d(np.arange(2 * n), fixed)
    pick = np.random.RandomState(d).choice(rest, COLS - len(fixed), replace=False)
    return np.sort(np.concatenate((fixed, pick))).astype(np.int64)


def main():
    out = {"ls_iso": np.float64(LS_ISO)}
    worst = 0.0
    for d, nb, N in SHAPES:
        tag = "d%d" % d
        X = np.random.RandomState(1000 + d).randn(N, d).astype(np.float32)
        X64 = X.astype(np.float64)
        ard = np.linspace(0.7, 1.6, d)
        iso = rb.FastFoodRBF(nbases=nb, Xdim=d, random_state=SEED)
        b = rb.FastFoodRBF(nbases=nb, Xdim=d, lenscale=Parameter(np.ones(d), Positive()), random_state=SEED)
        assert np.array_equal(iso.G, b.G) and np.array_equal(iso.PI, b.PI)
        mats = orc.fastfood_matrices(nb, d, SEED)
        for mine, theirs in zip(mats, (b.B, b.G, b.PI, b.S)):
            worst = max(worst, close(theirs, mine))
        d2, k, n = orc.fastfood_dims(nb, d)
        cols = sample_columns(d, d2, n)
        out["X_" + tag], out["ls_ard_" + tag], out["cols_" + tag] = X, ard, cols
        P_iso, P_ard = iso.transform(X64, LS_ISO), b.transform(X64, ard)
        assert P_iso.shape == P_ard.shape == (N, 2 * n)
        worst = max(worst, close(P_iso, orc.fastfood_transform(X64, *mats, LS_ISO)), close(P_ard, orc.fastfood_transform(X64, *mats, ard)))
        out["Phi_iso_" + tag], out["Phi_ard_" + tag] = P_iso[:, cols], P_ard[:, cols]
        dP = iso.grad(X64, LS_ISO)
        assert dP.shape == (N, 2 * n)
        worst = max(worst, close(dP, orc.fastfood_grad(X64, *mats, LS_ISO)))
        out["dPhi_iso_" + tag] = dP[:, cols]
        if d == 300:
            dA = b.grad(X64, ard)
            assert dA.shape == (N, 2 * n, d)
            worst = max(worst, close(dA, orc.fastfood_grad(X64, *mats, ard)))
            gcols = cols[np.linspace(0, COLS - 1, GCOLS).astype(int)]
            out["gcols_" + tag], out["dPhi_ard_" + tag] = gcols, dA[:, gcols, :]
        print("%-6s d2=%d k=%d: reference vs oracle so far %.2e" % (tag, d2, k, worst))
    np.savez(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote %s: %d arrays, %d bytes; worst normwise error oracle vs reference %.2e" % (OUT, len(out), size, worst))
    assert size <= MAX_BYTES, size


if __name__ == "__main__":
    main()
