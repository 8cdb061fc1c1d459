"""FastFoodRBF / FastFoodGM children of the float64 feature matrix, without a device: the four entry points in the header, the
built library and the ctypes table; the opt-in of ``_resident_child``; and ``dhyp`` of the float64 children against the
oracle's materialised gradients on a host-computed T = X^T A (a stub stands in for the device: the chain's V comes from the
oracle, buffers are NumPy arrays)."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import revrand_oracle as orc  # noqa: E402

NEW_ENTRY_POINTS = {"rr_featmat64_put_fastfood": 8, "rr_featmat64_put_fastfood_gm": 9, "rr_featmat64_pass2_xt": 8,
                    "rr_featmat64_glm_xt": 8}


def test_the_new_entry_points_are_declared_exported_and_in_the_ctypes_table():
    from revrand_amd import _hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "revrand_hip.h")).read(), flags=re.S)
    lib = _hip.load_library()
    for name, nargs in NEW_ENTRY_POINTS.items():
        assert re.search(r"\bint\s+%s\s*\(\s*rr_featmat64\s*\*" % name, src), name
        assert name in _hip.SIGNATURES and _hip.SIGNATURES[name][0] is _hip.ctypes.c_int
        assert len(_hip.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name) is not None   # (AttributeError: the built library does not export it)
    for meth in ("put_fastfood", "put_fastfood_gm", "pass2_xt", "glm_xt"):
        assert callable(getattr(_hip.FeatureMatrix64, meth))
    assert [_hip.xt_padded_dim(d) for d in (1, 8, 9, 100, 128, 129, 300, 4096)] == [8, 8, 16, 128, 128, 129, 300, 4096]


# ---- a stub device: buffers are NumPy arrays, the chain's V is the oracle's ---------------------------------------------------
class _Buf(object):
    def __init__(self, value=None):
        self.value, self.freed = value, False

    def free(self):
        self.freed = True


class _Dev(object):
    def upload_matrix(self, X, ld_dev=None):
        buf = _Buf(np.array(X))
        buf.ld, buf.shape, buf.dtype = ld_dev, X.shape, X.dtype
        return buf

    def zeros(self, nbytes):
        return _Buf(np.zeros(nbytes // 8))

    def memset(self, buf):
        buf.value[:] = 0.0

    def download(self, buf, shape, dtype):
        return np.asarray(buf.value, dtype=dtype).reshape(shape)


class _Chain(object):
    """_hip.FastFoodHandle's constructor and the members the children use."""

    def __init__(self, d, d2, k, B, G, PI, S, compute="f32", device=None, wide=False):
        self.dev, self.d, self.d2, self.k, self.n = _Dev(), d, d2, k, d2 * k
        self.mats = (np.asarray(B), np.asarray(G), np.asarray(PI), np.asarray(S))
        self.wide_gm = wide == "gm" and d2 > 256

    @property
    def gm_chain_ok(self):
        return self.wide_gm or 16 <= self.d2 <= 256

    def vx(self, X, lenscale=1.0):
        return orc.fastfood_VX(np.asarray(X, dtype=float) / lenscale, *self.mats)


@pytest.fixture
def stub(monkeypatch):
    from revrand_amd import _hip

    def no_dense(*a, **k):
        raise AssertionError("a float64 FastFood child built a dense random Fourier handle")
    monkeypatch.setattr(_hip, "FastFoodHandle", _Chain)
    monkeypatch.setattr(_hip, "RffHandle", no_dense)


def _bases(d, dtype="f64", ard=False):
    from revrand_amd.basis_functions import FastFoodGM, FastFoodRBF
    from revrand_amd.btypes import Parameter, Positive, Bound
    ls = Parameter(np.linspace(0.8, 1.7, d), Positive()) if ard else Parameter(1.3, Positive())
    rbf = FastFoodRBF(nbases=40, Xdim=d, lenscale=ls, random_state=3, dtype=dtype)
    gm = FastFoodGM(nbases=40, Xdim=d, mean=Parameter(np.linspace(-0.4, 0.5, d), Bound()),
                    lenscale=Parameter(np.linspace(0.8, 1.7, d), Positive()), random_state=4, dtype=dtype)
    return rbf, gm


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_resident_child_declines_a_float64_state_without_the_option_and_accepts_it_with(stub, dtype):
    from revrand_amd import basis_functions as bf
    X = np.random.RandomState(0).randn(7, 20)
    rbf, gm = _bases(20, dtype)
    for b, cls in ((rbf, bf._ResidentFastFood64), (gm, bf._ResidentFastFoodGM64)):
        assert getattr(type(b), "_child_options", False) is True
        assert b._resident_child(X, dtype="f64") is None
        assert b._resident_child(X, dtype="f64", f64_children=False, wide=True) is None
        child = b._resident_child(X, dtype="f64", f64_children=True, wide=True)
        assert type(child) is cls
        # X resident as float64, whole padded rows for the register kernel (20 columns -> 32)
        assert child.dX.dtype == np.float64 and child.dX.ld == 32 and child.dX.shape == (7, 20)
        assert child.W.shape == (20, b.n)
        np.testing.assert_array_equal(child.W, orc.fastfood_VX(np.eye(20), b.B, b.G, b.PI, b.S))
        child.release()
        assert child.dX.freed and child.dT.freed
    # a block size the chain's mixture mode does not serve (Xdim <= 8): no float64 FastFoodGM child
    assert _bases(5, dtype)[1]._resident_child(np.zeros((3, 5)), dtype="f64", f64_children=True) is None
    # above 256 columns FastFoodGM needs wide_chain=True, FastFoodRBF does not
    wide = bf.FastFoodGM(nbases=10, Xdim=300, random_state=0, dtype=dtype)
    assert wide._resident_child(np.zeros((3, 300)), dtype="f64", f64_children=True) is None
    wide = bf.FastFoodGM(nbases=10, Xdim=300, random_state=0, dtype=dtype, wide_chain=True)
    assert type(wide._resident_child(np.zeros((3, 300)), dtype="f64", f64_children=True)) is bf._ResidentFastFoodGM64
    rb = bf.FastFoodRBF(nbases=10, Xdim=300, random_state=0, dtype=dtype)
    child = rb._resident_child(np.zeros((3, 300)), dtype="f64", f64_children=True)
    assert type(child) is bf._ResidentFastFood64 and child.dX.ld == 300


def _contraction(X, P, E, n):
    """T = X^T (E_s o P_c - E_c o P_s), (d, n)."""
    return X.T @ (E[:, n:2 * n] * P[:, :n] - E[:, :n] * P[:, n:2 * n])


@pytest.mark.parametrize("d,ard", [(1, False), (5, False), (5, True), (20, True)])
def test_dhyp_of_the_float64_rbf_child_is_apply_grad_over_the_oracles_gradient(stub, d, ard):
    from revrand_amd.basis_functions import apply_grad
    rs = np.random.RandomState(d)
    X = rs.randn(11, d)
    b = _bases(d, ard=ard)[0]
    ls = b.params.value
    mats = (b.B, b.G, b.PI, b.S)
    P = orc.fastfood_transform(X, *mats, ls)
    E = rs.randn(*P.shape)
    child = b._resident_child(X, dtype="f64", f64_children=True)
    child.ls = ls
    child.dT.value[:] = _contraction(X, P, E, b.n).ravel()
    want = apply_grad(lambda dPhi: -(E * dPhi).sum(), orc.fastfood_grad(X, *mats, ls))
    got = child.dhyp(1.0)
    assert np.shape(got) == np.shape(want)   # isotropic: one number (input dimension 0 only); ARD: (d,)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(child.dhyp(0.7), np.asarray(want) / 0.7, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("d", [1, 20])
def test_dhyp_of_the_float64_gm_child_is_apply_grad_over_the_oracles_gradients(stub, d):
    from revrand_amd.basis_functions import FastFoodGM, apply_grad
    from revrand_amd.btypes import Parameter, Positive, Bound
    rs = np.random.RandomState(10 + d)
    X = rs.randn(9, d)
    if d == 1:   # (d2 = 1 has no chain child: the formula alone, on a child built by hand around the stub)
        b = FastFoodGM(nbases=6, Xdim=1, mean=Parameter(np.array([0.3]), Bound()), lenscale=Parameter(np.array([1.4]), Positive()),
                       random_state=1, dtype="f64")
        from revrand_amd.basis_functions import _ResidentFastFoodGM64
        child = _ResidentFastFoodGM64(b, X)
    else:
        b = _bases(d)[1]
        child = b._resident_child(X, dtype="f64", f64_children=True)
    mean, ls = [p.value for p in b.params]
    mats = (b.B, b.G, b.PI, b.S)
    n = b.n
    P = orc.fastfood_gm_transform(X, *mats, mean, ls)
    E = rs.randn(*P.shape)
    child.mean, child.ls = mean, ls
    child.dT.value[:] = _contraction(X, P[:, :2 * n], E[:, :2 * n], n).ravel()
    child.dTm.value[:] = _contraction(X, P[:, 2 * n:], E[:, 2 * n:], n).ravel()
    want = apply_grad(lambda dPhi: -(E * dPhi).sum(), orc.fastfood_gm_grad(X, *mats, mean, ls))
    got = child.dhyp(1.0)
    assert len(got) == 2
    for g, w in zip(got, want):
        assert np.shape(g) == np.shape(w)   # d == 1: scalars
        np.testing.assert_allclose(g, w, rtol=1e-11, atol=1e-12)
