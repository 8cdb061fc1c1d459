"""Float64 NumPy restatement of RadialBasis, SigmoidalBasis and PolynomialBasis, written from their formulas -- what the
GPU tests hold the device code to on shapes the golden fixture (tests/golden/centres.npz) does not carry.  Test
infrastructure: the product never imports it.  tools/make_centres_golden.py asserts, while it generates the fixture, that
every function here equals the reference to 1e-12 normwise.

With x_n a row of X (N, d), c_j a row of C (M, d) and l the length scale(s) -- a scalar / one entry (isotropic: the same
l for every dimension) or d entries (ARD):

    radial    Phi[n, j] = exp(-sum_i ((x_ni - c_ji) / (2 l_i^2))^2)          dPhi_i = Phi ((x_ni - c_ji) / l_i^3)^2
    sigmoid   Phi[n, j] = 1 / (1 + exp(-sqrt(sum_i ((x_ni - c_ji) / l_i)^2)))  dPhi_i = -(|x_ni - c_ji| / l_i^2) Phi (1 - Phi)

The gradient has one slice per ENTRY of the length-scale vector: isotropic gives input dimension 0's term only, (N, M);
ARD gives (N, M, d).
"""
import numpy as np


def _ls(lenscale, d):
    ls = np.atleast_1d(np.asarray(lenscale, dtype=float))
    assert ls.shape in ((1,), (d,))
    return ls


def _diff(X, C):
    """(N, M, d): x_ni - c_ji."""
    return np.asarray(X, dtype=float)[:, None, :] - np.asarray(C, dtype=float)[None, :, :]


def radial_transform(X, C, lenscale):
    ls = _ls(lenscale, np.shape(X)[1])
    return np.exp(-((_diff(X, C) / (2 * ls ** 2)) ** 2).sum(axis=2))


def radial_grad(X, C, lenscale):
    ls = _ls(lenscale, np.shape(X)[1])
    Phi = radial_transform(X, C, ls)
    D = _diff(X, C)[:, :, :ls.size]
    dPhi = Phi[:, :, None] * (D / ls ** 3) ** 2
    return dPhi[:, :, 0] if ls.size == 1 else dPhi


def sigmoid_transform(X, C, lenscale):
    ls = _ls(lenscale, np.shape(X)[1])
    r = np.sqrt(((_diff(X, C) / ls) ** 2).sum(axis=2))
    return 1. / (1. + np.exp(-r))


def sigmoid_grad(X, C, lenscale):
    ls = _ls(lenscale, np.shape(X)[1])
    Phi = sigmoid_transform(X, C, ls)
    D = _diff(X, C)[:, :, :ls.size]
    dPhi = -(np.abs(D) / ls ** 2) * (Phi * (1 - Phi))[:, :, None]
    return dPhi[:, :, 0] if ls.size == 1 else dPhi


def poly_transform(X, order, include_bias=True):
    """[1] (if include_bias), then x_i^1 .. x_i^order for each input dimension i in turn."""
    X = np.asarray(X, dtype=float)
    cols = [np.ones((X.shape[0], 1))] if include_bias else []
    for i in range(X.shape[1]):
        for p in range(1, order + 1):
            cols.append(X[:, [i]] ** p)
    return np.hstack(cols) if cols else np.empty((X.shape[0], 0))


TRANSFORM = {"RadialBasis": radial_transform, "SigmoidalBasis": sigmoid_transform}
GRAD = {"RadialBasis": radial_grad, "SigmoidalBasis": sigmoid_grad}
