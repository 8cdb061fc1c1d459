#!/usr/bin/env python3
"""
Generate tests/golden/centres.npz and tests/golden/centres_sigmoid.npz -- RadialBasis, SigmoidalBasis and PolynomialBasis
as the REFERENCE computes them -- by importing the reference on the build machine, and hold the float64 restatement in
tests/centres_cases.py to every array while doing so (1e-12 normwise).

Two files because the arrays asked for (X, C, Phi and dPhi of both classes at three shapes and three length scales, N = 32,
float64) are 510 KB on their own and random mantissas do not compress: centres.npz holds everything but SigmoidalBasis'
Phi / dPhi, which centres_sigmoid.npz holds; each stays under 400 KB.

    PYTHONDONTWRITEBYTECODE=1 python -B tools/make_centres_golden.py

Only data (inputs and the reference's outputs) is written.  The reference is imported the way oracle/make_golden.py does
it: the ``decorator`` stand-in of oracle/shim on the path and ``np.asscalar`` (gone from NumPy 2) defined for this process.
Nothing under oracle/ or in the reference is touched.
"""
import os
import sys
from functools import reduce
from operator import add

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = os.environ.get("REVRAND_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(0, REFERENCE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

if not hasattr(np, "asscalar"):
    np.asscalar = lambda a: a.item()  # process-local

import revrand.basis_functions as rb  # noqa: E402
import revrand.likelihoods as rl  # noqa: E402
from revrand.btypes import Bound, Parameter, Positive  # noqa: E402
from revrand.glm import GeneralizedLinearModel  # noqa: E402
from revrand.slm import StandardLinearModel  # noqa: E402

import centres_cases as cc  # noqa: E402
import revrand_oracle as orc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "centres.npz")
OUT_SIGMOID = os.path.join(ROOT, "tests", "golden", "centres_sigmoid.npz")
MAX_BYTES = 400 * 1024
SHAPES = [(1, 7), (5, 33), (8, 48)]
N = 32


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(1.0, np.abs(a).max() if a.size else 1.0)
    err = np.abs(a - b).max() if a.size else 0.0
    assert err <= tol * scale, err
    return err


def lenscales(d):
    return [("iso0.9", 0.9, Parameter(1., Positive())), ("iso1.7", 1.7, Parameter(1., Positive())),
            ("ard", np.linspace(0.7, 1.6, d), Parameter(np.ones(d), Positive()))]


def gen_bases(out):
    worst = 0.0
    for d, M in SHAPES + [(21, 40)]:   # (d = 21: checked against the restatement, not stored)
        rs = np.random.RandomState(100 + d)
        X, C = rs.randn(N, d), rs.randn(M, d)
        store = (d, M) in SHAPES
        if store:
            out["X_d%d" % d], out["C_d%d" % d] = X, C
        for name, cls in (("RadialBasis", rb.RadialBasis), ("SigmoidalBasis", rb.SigmoidalBasis)):
            for tag, ls, par in lenscales(d):
                b = cls(centres=C, lenscale=par)
                P, dP = b.transform(X, ls), b.grad(X, ls)
                assert P.shape == (N, M) and dP.shape == ((N, M) if (tag != "ard" or d == 1) else (N, M, d))
                worst = max(worst, close(P, cc.TRANSFORM[name](X, C, ls)), close(dP, cc.GRAD[name](X, C, ls)))
                if store:
                    out["%s_d%d_%s_Phi" % (name, d, tag)] = P
                    out["%s_d%d_%s_dPhi" % (name, d, tag)] = dP
    X = np.random.RandomState(7).randn(N, 3)
    out["poly_X"] = X
    for tag, order, bias in (("o0", 0, True), ("o3", 3, True), ("o3nb", 3, False)):
        P = rb.PolynomialBasis(order=order, include_bias=bias).transform(X)
        worst = max(worst, close(P, cc.poly_transform(X, order, bias)))
        out["poly_%s_Phi" % tag] = P
    print("restatement vs reference: worst normwise error %.2e" % worst)


def cat15(bs, X, nC=10):
    """The 15-way concatenation of the reference's tests/test_bases.py::test_bases."""
    d = X.shape[1]
    ard = lambda: Parameter(np.ones(d), Positive())  # noqa: E731
    return [bs.BiasBasis(), bs.LinearBasis(onescol=True), bs.PolynomialBasis(order=2),
            bs.RadialBasis(centres=X[:nC, :]), bs.RadialBasis(centres=X[:nC, :], lenscale=ard()),
            bs.SigmoidalBasis(centres=X[:nC, :]), bs.SigmoidalBasis(centres=X[:nC, :], lenscale=ard()),
            bs.RandomRBF(Xdim=d, nbases=10), bs.RandomRBF(Xdim=d, nbases=10, lenscale=ard()),
            bs.OrthogonalRBF(Xdim=d, nbases=10), bs.OrthogonalRBF(Xdim=d, nbases=10, lenscale=ard()),
            bs.FastFoodRBF(Xdim=d, nbases=10), bs.FastFoodRBF(Xdim=d, nbases=10, lenscale=ard()),
            bs.FastFoodGM(Xdim=d, nbases=10),
            bs.FastFoodGM(Xdim=d, nbases=10, mean=Parameter(np.zeros(d), Bound()), lenscale=ard())]


def gen_cat15(out):
    x = np.linspace(-5, 5, 30)
    X = np.hstack((np.ones((30, 1)), x[:, np.newaxis]))   # the shape of the reference's make_gaus_data
    bases = cat15(rb, X)
    bcat = reduce(add, bases)
    regs = np.linspace(0.5, 4.0, len(bases))
    diag, slices = bcat.regularizer_diagonal(X, *regs)
    out["cat15_X"] = X
    out["cat15_get_dim"] = np.array(int(bcat.get_dim(X)))
    out["cat15_dims"] = np.array([int(b.get_dim(X)) for b in bases])
    out["cat15_regs"] = regs
    out["cat15_regdiag"] = diag
    out["cat15_slices"] = np.array([[s.start, s.stop] for s in slices])
    # the parameter structure, child by child (the reference's BasisCat.params itself fails on the two-parameter FastFoodGM
    # children): sizes of every parameter that has a value, -1 for a scalar
    sizes = []
    for b in bases:
        ps = b.params if isinstance(b.params, list) else [b.params]
        sizes.extend([(-1 if p.shape == () else int(p.shape[0])) for p in ps if p.has_value])
    out["cat15_param_sizes"] = np.array(sizes)


def elbo_case(basis, X, y, var, reg, hypers):
    slm = StandardLinearModel(basis)
    slm.obj_ = -np.inf
    nelbo, (ndvar, ndreg, ndhyp) = slm._elbo(X, y, var, reg, hypers)
    hy = ndhyp if isinstance(ndhyp, list) else [ndhyp]
    return dict(elbo=np.array(-nelbo), dvar=np.array(-ndvar), dreg=-np.atleast_1d(np.asarray(ndreg, float)),
                dhyp=np.concatenate([-np.atleast_1d(np.asarray(h, float)) for h in hy]), m=slm.weights_, C=slm.covariance_)


def gen_elbo(out):
    Nn, d, M = 500, 4, 24
    r = np.random.RandomState(6)
    X = r.randn(Nn, d)
    y = np.sin(X @ r.randn(d)) + 0.1 * r.randn(Nn)
    C = np.random.RandomState(16).randn(M, d)
    var, ard = 0.37, np.linspace(0.8, 1.5, d)
    out.update(elbo_X=X, elbo_y=y, elbo_C=C, elbo_var=np.array(var), elbo_ard=ard, elbo_iso=np.array(1.1),
               elbo_reg=np.array([1.7, 0.6, 2.2]))
    ardp = lambda: Parameter(np.ones(d), Positive())  # noqa: E731
    cases = [
        ("radial_iso", rb.RadialBasis(centres=C), 1.7, 1.1),
        ("radial_ard", rb.RadialBasis(centres=C, lenscale=ardp()), 1.7, ard),
        ("sigmoid_ard", rb.SigmoidalBasis(centres=C, lenscale=ardp()), 1.7, ard),
        ("radial_poly_linear", rb.RadialBasis(centres=C, lenscale=ardp()) + rb.PolynomialBasis(order=2) + rb.LinearBasis(),
         [1.7, 0.6, 2.2], ard),
    ]
    for tag, basis, reg, hyp in cases:
        res = elbo_case(basis, X, y, var, reg, hyp)
        # the restatement through the oracle's _elbo on restated features
        kind = "SigmoidalBasis" if tag.startswith("sigmoid") else "RadialBasis"
        Phi, dP = cc.TRANSFORM[kind](X, C, hyp), cc.GRAD[kind](X, C, hyp)
        dPl = [dP] if dP.ndim == 2 else [dP[:, :, i] for i in range(d)]
        if tag == "radial_poly_linear":
            extra = np.hstack((cc.poly_transform(X, 2), np.hstack((np.ones((Nn, 1)), X))))
            Phi = np.hstack((Phi, extra))
            dPl = [np.hstack((g, np.zeros_like(extra))) for g in dPl]
            rd = np.concatenate((np.full(M, 1.7), np.full(1 + 2 * d, 0.6), np.full(1 + d, 2.2)))
            sl = [slice(0, M), slice(M, M + 1 + 2 * d), slice(M + 1 + 2 * d, Phi.shape[1])]
        else:
            rd, sl = np.full(M, 1.7), slice(None)
        o = orc.slm_elbo(Phi, y, var, rd, sl, dPl)
        close(res["elbo"], o["elbo"], 1e-10)
        close(res["dvar"], o["dvar"], 1e-8)
        close(res["dreg"], np.array(o["dreg"]), 1e-8)
        close(res["dhyp"], np.array(o["dhyp"]), 1e-7)
        for k, v in res.items():
            out["elbo_%s_%s" % (tag, k)] = v


def gen_fit(out):
    """One fit of RadialBasis (isotropic) + LinearBasis with fixed start values, nstarts=0, maxiter=20.

    The case is chosen so that the REFERENCE's run is a well-defined target.  (1) One input dimension: the isotropic
    gradient is input dimension 0's term only, which is the true derivative only for d = 1 -- for d > 1 L-BFGS-B's line
    searches see a gradient that does not belong to the objective.  (2) Start values near the optimum: from generic ones
    (var 0.5, lenscale 1.2, ...) the first trial step overshoots to var ~ 1e-77, the line search gives up, and fit() returns
    its start point or wherever it stalled (the same finding as gen_fit_c1 of oracle/make_golden.py).  From these the
    reference converges within the 20 iterations: no non-finite evaluation, and the gradient at the end is 1e-5 of the
    one at the start -- asserted below."""
    Nn, d, M = 400, 1, 20
    r = np.random.RandomState(7)
    X = r.uniform(-3, 3, size=(Nn, d))
    y = np.sin(2 * X[:, 0]) + 0.3 * X[:, 0] + 0.05 * r.randn(Nn)
    Xs = np.random.RandomState(8).uniform(-3, 3, size=(16, d))
    C = np.linspace(-3, 3, M)[:, None]
    b = rb.RadialBasis(centres=C, lenscale=Parameter(0.856, Positive()), regularizer=Parameter(1.3, Positive())) \
        + rb.LinearBasis(onescol=True, regularizer=Parameter(0.65, Positive()))
    slm = StandardLinearModel(b, var=Parameter(0.0032, Positive()), nstarts=0, maxiter=20)
    with np.errstate(invalid="raise"):
        slm.fit(X, y)
    g0 = slm._elbo(X, y, 0.0032, [1.3, 0.65], 0.856)[1][2]
    g1 = slm._elbo(X, y, slm.var_, slm.regularizer_, slm.hypers_)[1][2]
    assert abs(g1) < 1e-4 * abs(g0) and abs(float(slm.var_) - 0.0032) > 5e-4, (g0, g1, slm.var_)
    Ey, Vy = slm.predict_moments(Xs)
    out.update(fit_X=X, fit_y=y, fit_Xs=Xs, fit_C=C, fit_var=np.array(slm.var_),
               fit_reg=np.asarray(slm.regularizer_, float), fit_hyp=np.array(slm.hypers_, float), fit_obj=np.array(slm.obj_),
               fit_Ey=Ey, fit_Vy=Vy, fit_start=np.array([0.0032, 0.856, 1.3, 0.65]))


def gen_glm(out):
    rs = np.random.RandomState(11)
    Mb, d, Mc, K, L, seed, B = 64, 4, 24, 3, 8, 5, 10.0
    X = rs.randn(Mb, d)
    fl = np.sin(X @ rs.randn(d))
    y = (rs.rand(Mb) < 1 / (1 + np.exp(-fl))).astype(float)
    C = rs.randn(Mc, d)
    D = Mc + d + 1
    m = 0.3 * rs.randn(D, K)
    Cv = rs.gamma(2., 0.5, size=(D, K))
    ls = np.linspace(0.8, 1.4, d)
    regs = [1.3, 0.8]
    basis = rb.RadialBasis(centres=C, lenscale=Parameter(np.ones(d), Positive())) + rb.LinearBasis(onescol=True)
    glm = GeneralizedLinearModel(likelihood=rl.Bernoulli(), basis=basis, K=K, nsamples=L, random_state=seed)
    glm.B_, glm.D_ = B, D
    glm._GeneralizedLinearModel__it = -1
    nobj, (ndm, ndC, dL, dlp, dbp) = glm._elbo(m.copy(), Cv.copy(), regs, [], ls, X, y)
    e = np.stack([np.random.RandomState(seed).randn(K * L, D)[k * L:(k + 1) * L] for k in range(K)])
    Phi = np.hstack((cc.radial_transform(X, C, ls), np.ones((Mb, 1)), X))
    dP = cc.radial_grad(X, C, ls)
    dPl = [np.hstack((dP[:, :, i], np.zeros((Mb, d + 1)))) for i in range(d)]
    rd = np.concatenate((np.full(Mc, regs[0]), np.full(d + 1, regs[1])))
    o = orc.glm_elbo(m, Cv, rd, [slice(0, Mc), slice(Mc, D)], "bernoulli", [], (), Phi, dPl, y, e, B)
    close(o[0], nobj, 1e-10)
    close(o[1][0], ndm, 1e-10)
    close(o[1][1], ndC, 1e-10)
    close(np.array(o[1][2]), np.array(dL, float), 1e-10)
    close(np.array(o[1][4]), np.atleast_1d(dbp), 1e-10)
    assert dlp == []
    out.update(glm_X=X, glm_y=y, glm_C=C, glm_m=m, glm_Cv=Cv, glm_ls=ls, glm_regs=np.array(regs), glm_K=np.array(K),
               glm_L=np.array(L), glm_seed=np.array(seed), glm_B=np.array(B), glm_e=e, glm_obj=np.array(nobj), glm_ndm=ndm,
               glm_ndC=ndC, glm_dL=np.array(dL, float), glm_dbp=np.atleast_1d(dbp))


def main():
    out = {}
    gen_bases(out)
    gen_cat15(out)
    gen_elbo(out)
    gen_fit(out)
    gen_glm(out)
    assert all(v.dtype != object for v in map(np.asarray, out.values()))
    sig = {k: out.pop(k) for k in sorted(out) if k.startswith("SigmoidalBasis_")}
    for path, arrs in ((OUT, out), (OUT_SIGMOID, sig)):
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        with np.load(path, allow_pickle=False) as z:
            assert sorted(z.files) == sorted(arrs)
        print("%s: %.1f KB, %d arrays" % (path, size / 1024., len(arrs)))
        assert size <= MAX_BYTES, "fixture too large: %d bytes" % size


if __name__ == "__main__":
    main()
